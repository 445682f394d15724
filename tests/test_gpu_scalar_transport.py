"""IMEX scalar transport with Boussinesq buoyancy on the GPU (nsfem_set_scalar / nsfem_step_scalar_imex /
nsfem_scalar_convection, BoussinesqIMEXSolver) against the numpy restatement of tests/test_scalar_transport_host.py,
with the flow step (nsfem_step_imex with f_eff = f + T b) against IMEXRestatement of tests/test_imex_solver_host.py.

Tolerances.  Kernel: 1e-13 relative, what tests/test_gpu_parity.py applies to the velocity convection residual vector.
Steps: those of tests/test_gpu_imex.py for the same step count and Krylov settings (rtol 1e-13) -- u*, u 1e-9 and p minus
its mean 1e-8, relative; T is held to the bound of u*, 1e-9.

Meshes.  box(4, 4), box(8, 8): binary spacing, 81 and 289 P2 nodes -- below the 1024 rows from which build_stencil_dict
builds a dictionary at all, so their products run on CSR; box(16, 16) (1089 nodes) is the smallest binary lattice on
which the dictionary path runs; box(3, 5) is the small non-binary, non-square one and box(20, 28) (2337 nodes) the
non-binary one that HAS a dictionary, which is not the matrix bit for bit: CSR is required there.  3D: the Kuhn boxes of
tests/test_gpu_3d.py, (3, 2, 2) cells on a 1 x 0.8 x 0.6 box (unequal counts and lengths) and (4, 4, 4).  The kernel also
runs on the mapped box(8, 8) of tests/test_gpu_variable_viscosity.py (cells of different size and shape) and on the
general tetrahedra of tests/general_tet_mesh.py with 72 and 384 cells (both orientations, no zero in any J^-1)."""
import numpy as np
import pytest

import _native as nat
import fem_oracle as fo
from general_tet_mesh import CUBE, SMALL, general_tets
from gpu_common import box, cavity_bc, context, rel, velocity_bc
from imex_time_stepping import IMEXTimeStepping, IMEXType
from periodic_meshes import ALL as PERIODIC
from periodic_meshes import is_periodic, lengths_of, periodic_axes, periodic_fields, periodic_fixture
from test_gpu_3d import box3, context3, lid_bc
from test_imex_solver_host import IMEXRestatement
from test_scalar_transport_host import ScalarIMEXRestatement, smooth_fields

pytestmark = pytest.mark.gpu

TYPES = (IMEXType.SBDF2, IMEXType.CNAB, IMEXType.mCNAB, IMEXType.CNLF)
FORMS = ((0, "standard"), (1, "skew_symmetric"))
NO_PBC = (np.zeros(0, np.int32), np.zeros(0))


def _mesh(kind):
    """(mesh, dm, marks, space, context factory) of a 2D box (nx, ny), the "mapped" box(8, 8), a 3D Kuhn box
    ((nx, ny, nz), lengths), the general tetrahedra ((nx, ny, nz), lengths, "general") or a periodic fixture of
    tests/periodic_meshes.py by its name"""
    if is_periodic(kind):
        mesh, dm, marks = periodic_fixture(kind)
        make = context if mesh._dim == 2 else context3
    elif kind == "mapped":
        from test_gpu_variable_viscosity import _mapped_box
        mesh, dm, marks = _mapped_box()
        make = context
    elif len(kind) == 2 and isinstance(kind[0], int):
        mesh, dm, marks = box(*kind)
        make = context
    elif len(kind) == 3:
        assert kind[2] == "general"
        mesh, dm, marks = general_tets(kind[0], kind[1])
        make = context3
    else:
        mesh, dm, marks = box3(*kind)
        make = context3
    return mesh, dm, marks, fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap), make


# ---------------------------------------------------------------- 1. the kernel against the oracle
_KERNEL_MESHES = [(4, 4), (8, 8), (3, 5), (16, 16), ((3, 2, 2), (1.0, 0.8, 0.6)), ((4, 4, 4), (1.0, 1.0, 1.0)), "mapped",
                  SMALL + ("general", ), CUBE + ("general", )] + list(PERIODIC)


@pytest.mark.parametrize("form_id,form", FORMS)
@pytest.mark.parametrize("kind", _KERNEL_MESHES, ids=str)
def test_scalar_convection_kernel_matches_the_oracle(kind, form_id, form):
    """weight * C(u) T for smooth, non-polynomial nodal u and T; (16, 16) and (4, 4, 4) have more than one block of 256
    cells, the others one partly filled block; the second call returns the same bytes.  The periodic fixtures (periodic
    fields): the seam cells gather their nodal values through the identified dofs"""
    mesh, dm, marks, s, make = _mesh(kind)
    u, T = smooth_fields(dm.p2_coords)
    if is_periodic(kind):
        assert dm.n_p2 < mesh.num_vertices() + mesh.num_edges()
        u, T = periodic_fields(dm.p2_coords, lengths_of(kind), periodic_axes(kind))
    want = ScalarIMEXRestatement(s, 0.0, form).convection_matrix(u) @ T
    ctx = make(mesh, dm)
    try:
        ctx.set_state(nat.U1, u)
        ctx.set_state(nat.T1, T)
        got = ctx.scalar_convection(nat.U1, nat.T1, form_id, 1.0)
        err = rel(got, want)
        print("kernel %s form %d: rel %.2e" % (kind, form_id, err))
        assert np.linalg.norm(want) > 1e-3 and err < 1e-13
        again = ctx.scalar_convection(nat.U1, nat.T1, form_id, 1.0)
        assert got.tobytes() == again.tobytes()
        # the weight rides in the kernel: -1.5 * C(u) T, from other slots
        ctx.set_state(nat.U2, u)
        ctx.set_state(nat.T2, T)
        assert rel(ctx.scalar_convection(nat.U2, nat.T2, form_id, -1.5), -1.5 * want) < 1e-13
        # the hook touches no stored state
        assert not ctx.get_state(nat.TCONV_1).any() and not ctx.get_state(nat.TCONV_2).any()
        with pytest.raises(nat.NativeError, match="form"):
            ctx.scalar_convection(nat.U1, nat.T1, 2, 1.0)
        with pytest.raises(nat.NativeError, match="slot"):
            ctx.scalar_convection(nat.P, nat.T1, 0, 1.0)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 2. / 3. steps against the restatements
_B = (0.3, 1.0, -0.4)


def _two_sides(dm, marks, X):
    """Dirichlet T on the sides 1 (x = 0) and 2 (x = 1)"""
    left = np.unique(dm.facet_p2_nodes(marks.facets_with_id(1)))
    right = np.unique(dm.facet_p2_nodes(marks.facets_with_id(2)))
    bd = np.concatenate([left, right])
    bv = np.concatenate([0.5 + X[left, 1], -0.2 + 0.0 * X[right, 1]])
    return bd, bv


def _drive(ctx, dm, marks, s, typ, form_id, form, steps, k, change_after=None, kappa=0.05):
    """`steps` time steps of the device (transport step, flow step, advance) and of the two restatements side by side:
    cavity velocity, Dirichlet T on two sides, a source, a body force and the buoyancy b = _B"""
    X = dm.p2_coords
    dim = X.shape[1]
    b = _B[:dim]
    vbc = cavity_bc(dm, marks) if dim == 2 else lid_bc(dm, marks)
    tbc = _two_sides(dm, marks, X)
    _, T_init = smooth_fields(X)
    q = np.cos(2.0 * X[:, 0] + 0.3) * np.sin(1.5 * X[:, 1] + 0.2)
    f = np.stack([np.sin(np.pi * X[:, 1]), -1.0 + X[:, 0], 0.5 * X[:, 1]][:dim], axis=1).ravel()
    coef = dict(convective_term=1.0, pressure_term=1.0, viscous_term=0.01, body_force_term=1.0)
    flow = IMEXRestatement(s, coef, "standard")
    orc = ScalarIMEXRestatement(s, kappa, form)
    orc.source = q
    orc.T[0], orc.T[1] = T_init.copy(), T_init.copy()
    ctx.set_coeffs(1.0, 1.0, 0.01, 1.0)
    ctx.set_dirichlet(nat.VELOCITY, *vbc)
    ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
    ctx.set_dirichlet(nat.SCALAR, *tbc)
    ctx.set_scalar(kappa, b, form_id)
    ctx.set_state(nat.BODY_FORCE, f)
    ctx.set_state(nat.T_SOURCE, q)
    ctx.set_state(nat.T0, T_init)
    ctx.set_state(nat.T1, T_init)
    opts = ctx.default_step_opts()
    for ko in (opts.momentum, opts.poisson, opts.correction):
        ko.rtol = 1e-13
    ts = IMEXTimeStepping(0.0, 1.0e9, typ, desired_start_time_step=k)
    expected_reuses, expected_builds, built_from = 0, 0, None
    for step in range(steps):
        if change_after is not None and step == change_after:
            ts.set_desired_next_step_size(0.5 * k)
        ts.update_coefficients()
        kk = ts.get_next_step_size()
        ctx.set_imex(ts.alpha, ts.beta, ts.gamma, kk)
        # the matrix depends on alpha0 / k and gamma0 (kappa stays): one build whenever that pair changes
        if (ts.alpha[0] / kk, ts.gamma[0]) != built_from:
            built_from = (ts.alpha[0] / kk, ts.gamma[0])
            expected_builds += 1
        si = ctx.step_scalar_imex(rtol=1e-13)
        orc.step(ts.alpha, ts.beta, ts.gamma, kk, flow.vel[1], flow.vel[2], tbc)
        T = ctx.get_state(nat.T0)
        et = rel(T, orc.T[0])
        expected_reuses += 1 if (ts.beta[1] != 0.0 and step > 0) else 0
        # the flow step with f_eff = f + T^{n+1} b
        flow.body_force = f + np.outer(orc.T[0], b).ravel()
        ctx.step_imex(opts)
        flow.step(ts.alpha, ts.beta, ts.gamma, kk, vbc, NO_PBC)
        us, u, p = ctx.get_state(nat.USTAR), ctx.get_state(nat.U0), ctx.get_state(nat.P)
        es, eu = rel(us, flow.ustar), rel(u, flow.vel[0])
        ep = rel(p - p.mean(), flow.p - flow.p.mean())
        print("%s form %d step %d k %.4g: T %.2e u* %.2e u %.2e p %.2e cg %d" % (
            typ.name, form_id, step, kk, et, es, eu, ep, si.iterations))
        assert si.converged and et < 1e-9, (typ, form_id, step, et)
        assert es < 1e-9 and eu < 1e-9 and ep < 1e-8, (typ, form_id, step, es, eu, ep)
        ctx.advance(0)
        orc.advance()
        flow.advance()
        ts.advance_time()
    # the user's body force slot is never overwritten
    assert np.array_equal(ctx.get_state(nat.BODY_FORCE), f)
    assert np.array_equal(ctx.get_state(nat.T1), ctx.get_state(nat.T0))
    return expected_reuses, expected_builds


@pytest.fixture(scope="module")
def box8():
    return _mesh((8, 8))


@pytest.mark.parametrize("typ", TYPES, ids=lambda t: t.name)
def test_transport_and_flow_steps_match_the_restatements(box8, typ):
    """box(8, 8), 4 steps of every IMEXType, standard form"""
    mesh, dm, marks, s, make = box8
    ctx = make(mesh, dm)
    try:
        reuses, builds = _drive(ctx, dm, marks, s, typ, 0, "standard", 4, 0.5 / 8)
        info, flow_info = ctx.scalar_info(), ctx.imex_info()
        # one convection launch per step: C(u2) T2 is the vector the step before stored (first step: beta1 = 0)
        assert info["convection_launches"] == 4 and info["convection_reuses"] == reuses, info
        assert reuses == (3 if typ is not IMEXType.CNLF else 0)
        # the matrix is rebuilt exactly when the flow step's is: first-order first step, then the coefficients stay
        assert info["matrix_builds"] == flow_info["matrix_builds"] == builds == 2, (info, flow_info)
        assert info["dictionary"] is False          # 289 rows: no dictionary is built below 1024
    finally:
        ctx.close()


@pytest.mark.parametrize("kind,form_id,form,dictionary", [
    ((4, 4), 1, "skew_symmetric", False), ((3, 5), 0, "standard", False), ((3, 5), 1, "skew_symmetric", False),
    ((16, 16), 0, "standard", True), ((16, 16), 1, "skew_symmetric", True), ((20, 28), 0, "standard", False),
    (((3, 2, 2), (1.0, 0.8, 0.6)), 0, "standard", False), (((3, 2, 2), (1.0, 0.8, 0.6)), 1, "skew_symmetric", False)],
    ids=str)
def test_transport_steps_on_the_other_lattices_and_the_skew_form(kind, form_id, form, dictionary):
    """SBDF2, 4 steps of k = 1/16 (a binary step size: next_time - current_time is the same number in every step, so
    the rebuild count is that of the coefficients alone): box(3, 5) and box(20, 28) must run on CSR (non-binary spacing: the
    dictionary, which only box(20, 28) has rows enough to get, is not the matrix), box(16, 16) on the dictionary copy;
    the (3, 2, 2) Kuhn box runs the 3D kernel inside the steps, stored vector and reuse included"""
    mesh, dm, marks, s, make = _mesh(kind)
    ctx = make(mesh, dm)
    try:
        reuses, builds = _drive(ctx, dm, marks, s, IMEXType.SBDF2, form_id, form, 4, 1.0 / 16.0)
        info = ctx.scalar_info()
        assert info["convection_launches"] == 4 and info["convection_reuses"] == reuses == 3, info
        assert info["matrix_builds"] == ctx.imex_info()["matrix_builds"] == builds == 2
        assert info["dictionary"] is dictionary, info
    finally:
        ctx.close()


@pytest.mark.parametrize("typ", TYPES, ids=lambda t: t.name)
def test_step_size_change_rebuilds_the_matrix_and_reuses_the_stored_convection(box8, typ):
    """the step size is halved between steps 2 and 3: the matrix is rebuilt as the flow step's is, the stored vector is
    reused (scaled by the new beta1 over the beta0 it was evaluated with), and the fields still match"""
    mesh, dm, marks, s, make = box8
    ctx = make(mesh, dm)
    try:
        reuses, builds = _drive(ctx, dm, marks, s, typ, 0, "standard", 4, 0.5 / 8, change_after=2)
        info, flow_info = ctx.scalar_info(), ctx.imex_info()
        assert info["convection_launches"] == 4 and info["convection_reuses"] == reuses, info
        # exactly one build per change of (alpha0 / k, gamma0), counted from the coefficients in _drive: the first step,
        # the second-order coefficients, the halved step and -- where alpha0 or gamma0 depend on the step ratio -- the
        # constant step after it
        print("%s: builds %d (flow %d), expected %d" % (typ.name, info["matrix_builds"], flow_info["matrix_builds"], builds))
        assert info["matrix_builds"] == flow_info["matrix_builds"] == builds and builds >= 3, (info, flow_info, builds)
    finally:
        ctx.close()


def test_a_level_set_by_hand_or_a_changed_form_recomputes_the_stored_convection(box8):
    mesh, dm, marks, s, make = box8
    ctx = make(mesh, dm)
    try:
        _drive(ctx, dm, marks, s, IMEXType.SBDF2, 0, "standard", 2, 0.5 / 8)
        before = ctx.scalar_info()
        ctx.set_state(nat.T2, ctx.get_state(nat.T2))          # the level was touched: its stored vector is void
        ctx.step_scalar_imex(rtol=1e-13)
        info = ctx.scalar_info()
        assert info["convection_launches"] == before["convection_launches"] + 2
        assert info["convection_reuses"] == before["convection_reuses"]
        ctx.advance(0)
        ctx.set_scalar(0.05, _B[:2], 1)                         # another form: void as well
        ctx.step_scalar_imex(rtol=1e-13)
        assert ctx.scalar_info()["convection_launches"] == info["convection_launches"] + 2
        ctx.advance(0)
        ctx.step_scalar_imex(rtol=1e-13)                      # ... and from then on reused again
        assert ctx.scalar_info()["convection_launches"] == info["convection_launches"] + 3
    finally:
        ctx.close()


# ---------------------------------------------------------------- 4. coupling
@pytest.mark.parametrize("kind", [(8, 8), ((4, 4, 4), (1.0, 1.0, 1.0))], ids=str)
def test_hydrostatic_balance_of_a_uniform_temperature(kind):
    """closed unit box, no-slip walls, T = 1, b = e_y (3D: e_z), f = 0, c_b = 1: the rest state u = 0 with
    grad p = c_b T b stays -- after 3 steps |u| <= 1e-9 and |p - mean(p) - c_b (y - 1/2)| <= 1e-8 (absolute), reached by
    solver accuracy (the pressure is linear: in the P1 space).  The run starts AT that state, p = c_b (y - 1/2): the
    pressure-correction scheme reaches it from p = 0 only at the rate of its splitting error (the restatement started
    from p = 0 on box(8, 8), k = 1/16: max |u| = 2.5e-2, 2.2e-2, 1.0e-2 after steps 1, 2, 3 -- asserted in
    tests/test_scalar_transport_host.py)."""
    mesh, dm, marks, s, make = _mesh(kind)
    dim = mesh.coords.shape[1]
    nodes = np.unique(np.concatenate([dm.facet_p2_nodes(marks.facets_with_id(m)).ravel() for m in range(1, 2 * dim + 1)]))
    bd = np.sort(np.concatenate([dim * nodes + a for a in range(dim)]))
    b = np.zeros(dim)
    b[dim - 1] = 1.0
    height = dm.p1_coords[:, dim - 1]
    ctx = make(mesh, dm)
    try:
        ctx.set_coeffs(1.0, 1.0, 0.01, 1.0)
        ctx.set_dirichlet(nat.VELOCITY, bd, np.zeros(bd.size))
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        ctx.set_scalar(0.05, b, 0)
        for slot in (nat.T0, nat.T1, nat.T2):
            ctx.set_state(slot, np.ones(dm.n_p2))
        for slot in (nat.P, nat.P_OLD):
            ctx.set_state(slot, height - 0.5)
        opts = ctx.default_step_opts()
        for ko in (opts.momentum, opts.poisson, opts.correction):
            ko.rtol = 1e-13
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=1.0 / 16.0)
        for step in range(3):
            ts.update_coefficients()
            ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
            ctx.step_scalar_imex(rtol=1e-13)
            ctx.step_imex(opts)
            ctx.advance(0)
            ts.advance_time()
        u, p, T = ctx.get_state(nat.U1), ctx.get_state(nat.P_OLD), ctx.get_state(nat.T1)
        eu, ep, et = np.abs(u).max(), np.abs(p - p.mean() - (height - 0.5)).max(), np.abs(T - 1.0).max()
        print("hydrostatic %s: max |u| %.2e, max |p - mean - (y - 1/2)| %.2e, max |T - 1| %.2e" % (kind, eu, ep, et))
        assert eu <= 1e-9 and ep <= 1e-8 and et <= 1e-9
        # the balance is the buoyancy's: without it the same pressure drives a flow
        ctx.set_scalar(0.05, None, 0)
        ctx.step_scalar_imex(rtol=1e-13)
        ctx.step_imex(opts)
        assert np.abs(ctx.get_state(nat.USTAR)).max() > 1e-3
    finally:
        ctx.close()


def test_zero_buoyancy_leaves_the_flow_step_bit_identical(box8):
    """with b = 0 the states after step_imex equal, byte for byte, those of a context on which no scalar was ever
    configured -- transport steps running alongside included"""
    mesh, dm, marks, s, make = box8
    X = dm.p2_coords
    f = np.stack([np.sin(np.pi * X[:, 1]), -1.0 + X[:, 0]], axis=1).ravel()
    _, T_init = smooth_fields(X)
    out = []
    for with_scalar in (False, True):
        ctx = make(mesh, dm)
        try:
            ctx.set_coeffs(1.0, 1.0, 0.01, 1.0)
            ctx.set_dirichlet(nat.VELOCITY, *cavity_bc(dm, marks))
            ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
            ctx.set_state(nat.BODY_FORCE, f)
            if with_scalar:
                ctx.set_scalar(0.05, np.zeros(2), 0)
                ctx.set_state(nat.T0, T_init)
                ctx.set_state(nat.T1, T_init)
            opts = ctx.default_step_opts()
            ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=0.5 / 8)
            for step in range(3):
                ts.update_coefficients()
                ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
                if with_scalar:
                    ctx.step_scalar_imex()
                ctx.step_imex(opts)
                ctx.advance(0)
                ts.advance_time()
            out.append([ctx.get_state(slot) for slot in (nat.U0, nat.U1, nat.U2, nat.USTAR, nat.P, nat.P_OLD,
                                                         nat.CONV_N2)])
            if with_scalar:
                assert np.abs(ctx.get_state(nat.T1) - T_init).max() > 1e-4      # (the scalar did move)
        finally:
            ctx.close()
    assert np.abs(out[0][0]).max() > 0.5
    for a, b in zip(*out):
        assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- 5. refusals
def test_partitioned_contexts_and_rotating_frames_are_refused(box8):
    mesh, dm, marks, s, make = box8
    group = nat.local_group_create(1)
    ctx = make(mesh, dm)
    try:
        ctx.attach_local_comm(group, 0)
        with pytest.raises(nat.NativeError, match="communicator"):
            ctx.set_scalar(0.05, None, 0)
        with pytest.raises(nat.NativeError, match="communicator"):
            ctx.scalar_convection(nat.U1, nat.T1, 0, 1.0)
    finally:
        ctx.close()
        nat.local_group_destroy(group)
    ctx = make(mesh, dm)
    try:
        ctx.set_coeffs(1.0, 1.0, 0.01, None, 1.0, 1.0)
        with pytest.raises(nat.NativeError, match="nsfem_set_scalar"):
            ctx.step_scalar_imex()
        ctx.set_scalar(0.05, None, 0)
        ctx.set_state(nat.T1, np.ones(dm.n_p2))
        with pytest.raises(nat.NativeError, match="nsfem_set_imex"):
            ctx.step_scalar_imex()
        ctx.set_imex((1.0, -1.0, 0.0), (1.0, 0.0), (1.0, 0.0, 0.0), 1.0 / 16.0)
        ctx.set_angular_velocity(0.5, 0.0)
        with pytest.raises(nat.NativeError, match="rotating"):
            ctx.step_scalar_imex()
        ctx.set_angular_velocity(0.0, 0.0)
        assert ctx.step_scalar_imex().converged
        # buoyancy needs the body force coefficient
        ctx.set_dirichlet(nat.VELOCITY, *cavity_bc(dm, marks))
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        ctx.set_scalar(0.05, (0.0, 1.0), 0)
        with pytest.raises(nat.NativeError, match="body_force_term"):
            ctx.step_imex()
        with pytest.raises(nat.NativeError, match="diffusivity"):
            ctx.set_scalar(-1.0, None, 0)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 6. through the classes
_SPEC = dict(name="Cavity", mesh=("cube", 2, 8), scheme="ipcs", clock=dict(dt=0.5 / 8, steps=3),
             bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_slip", "bottom"), ("velocity", "top", (1.0, 0.0))])


def _wall_temperature(X, t):
    return -0.2 + 0.1 * t + 0.3 * X[:, 1]


def _heating(X, t):
    return (1.0 + t) * np.cos(2.0 * X[:, 0] + 0.3) * np.sin(1.5 * X[:, 1] + 0.2)


def test_boussinesq_solver_class_equals_driving_the_steps_by_hand():
    """BoussinesqIMEXSolver through InstationaryProblem.solve_problem with the three temperature hooks (time-dependent
    wall temperature and source) on the 8 x 8 cavity, 3 steps: bit for bit what set_scalar / step_scalar_imex /
    step_imex / advance give through the C ABI; the temperature is written to the XDMF file"""
    from multigrid import attach_hierarchy
    from ns_boussinesq_solver import BoussinesqIMEXSolver
    from problem_specs import build_problem
    steps, dt = _SPEC["clock"]["steps"], _SPEC["clock"]["dt"]
    spec = dict(_SPEC, numbers=dict(Re=100.0, Fr=1.0), output=1,
                start={"velocity": (0.0, 0.0), "pressure": 0.0, "temperature": 0.5})
    problem = build_problem(spec)
    cls = type(problem)

    def set_temperature_coefficients(self):
        self._temperature_coefficients = dict(diffusivity=0.05, buoyancy=(0.0, 1.0), convective_form="skew_symmetric")

    def set_temperature_boundary_conditions(self):
        self._temperature_bcs = [(self._sides["left"], 1.0), (self._sides["right"], _wall_temperature)]

    def set_temperature_source(self):
        self._temperature_source = _heating
    cls.set_temperature_coefficients = set_temperature_coefficients
    cls.set_temperature_boundary_conditions = set_temperature_boundary_conditions
    cls.set_temperature_source = set_temperature_source
    problem.set_solver_class(BoussinesqIMEXSolver)
    problem.compute_cfl = False
    problem.solve_problem()
    solver = problem._get_solver()
    assert isinstance(solver, BoussinesqIMEXSolver) and problem._time_stepping.step_number == steps
    assert solver.last_scalar_info["convection_launches"] == steps and solver.last_scalar_info["matrix_builds"] == 2
    assert solver.last_scalar_solve.converged and solver.last_step_info.krylov_iterations_momentum > 0
    T_cls, u_cls = solver._ctx.get_state(nat.T1), solver._ctx.get_state(nat.U1)
    assert np.array_equal(solver.temperature.vector(), solver._ctx.get_state(nat.T0))
    assert solver.temperature.dof_coordinates().shape == (solver._dofmap.n_p2, 2)
    with open(problem._get_filename()) as fh:
        assert fh.read().count('Name="temperature"') == steps + 1
    # ---- the same steps through the C ABI on a fresh context
    dm, mesh = solver._dofmap, solver._mesh
    X = dm.p2_coords
    left = np.unique(dm.facet_p2_nodes(solver._boundary_markers.facets_with_id(problem._sides["left"])))
    right = np.unique(dm.facet_p2_nodes(solver._boundary_markers.facets_with_id(problem._sides["right"])))
    ctx = nat.NsfemContext(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, dm.n_p2, dm.n_p1)
    try:
        if solver._mg_levels is not None:
            attach_hierarchy(ctx, mesh)
        coef = solver._equation_coefficients
        assert coef["body_force_term"] == 1.0
        ctx.set_coeffs(coef["convective_term"], coef["pressure_term"], coef["viscous_term"], coef["body_force_term"])
        bd, bv = solver._dirichlet_bcs["velocity"]
        ctx.set_dirichlet(nat.VELOCITY, np.asarray(bd, np.int32), np.asarray(bv, float))
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        ctx.set_scalar(0.05, (0.0, 1.0), 1)
        for slot in (nat.T0, nat.T1):
            ctx.set_state(slot, np.full(dm.n_p2, 0.5))
        opts = solver._step_options()
        ts = IMEXTimeStepping(0.0, 1.0, IMEXType.SBDF2, desired_start_time_step=dt)
        for _ in range(steps):
            ts.update_coefficients()
            t = float(ts.next_time)
            ctx.set_dirichlet(nat.SCALAR, np.concatenate([left, right]),
                              np.concatenate([np.ones(left.size), _wall_temperature(X[right], t)]))
            ctx.set_state(nat.T_SOURCE, _heating(X, t))
            ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
            ctx.step_scalar_imex(rtol=solver.krylov_rtol, max_iter=solver.krylov_max_iter)
            ctx.step_imex(opts)
            ts.advance_time()
            ctx.advance(0)
        T_abi, u_abi = ctx.get_state(nat.T1), ctx.get_state(nat.U1)
    finally:
        ctx.close()
    assert np.abs(T_cls - 0.5).max() > 1e-2 and np.abs(u_cls).max() > 0.5
    assert np.array_equal(T_cls, T_abi) and np.array_equal(u_cls, u_abi)


def test_problem_without_temperature_hooks_is_unchanged():
    """a problem without the hooks under IMEXIPCSSolver: the fields after 3 steps equal, byte for byte, the result
    recorded before the scalar transport existed (tests/golden/imex_cavity8_steps3.npz, written by
    tests/golden/gen_imex_cavity8_golden.py on commit 905127d), and no temperature is written"""
    import os
    from ns_imex_solver import IMEXIPCSSolver
    from problem_specs import build_problem
    spec = dict(_SPEC, numbers=dict(Re=100.0), start={"velocity": (0.0, 0.0), "pressure": 0.0}, output=1)
    problem = build_problem(spec)
    problem.set_solver_class(IMEXIPCSSolver)
    problem.compute_cfl = False
    problem.solve_problem()
    ctx = problem._get_solver()._ctx
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "imex_cavity8_steps3.npz"))
    for name, slot in (("u0", nat.U0), ("u1", nat.U1), ("ustar", nat.USTAR), ("p", nat.P), ("p_old", nat.P_OLD)):
        assert golden[name].tobytes() == ctx.get_state(slot).tobytes(), name
    assert ctx.scalar_info() == dict(matrix_builds=0, convection_launches=0, convection_reuses=0, dictionary=False)
    with open(problem._get_filename()) as fh:
        assert "temperature" not in fh.read()
