"""IMEX pressure-correction step on the GPU (nsfem_set_imex / nsfem_step_imex, IMEXIPCSSolver) against the numpy
restatement of the scheme in tests/test_imex_solver_host.py, and the one-launch right-hand side (k_jac_lattice's
right-hand-side mode) against the generic launch sequence, bit for bit.

Tolerances of the step comparisons: those of test_gpu_parity.test_ipcs_cavity_steps_match_oracle for the same
quantities after the same number of steps -- u*, u 1e-9 and p minus its mean 1e-8, relative -- with its LU-accuracy
Krylov tolerances (rtol 1e-13).

Periodic meshes (tests/periodic_meshes.py): the right-hand side of the generic path against IMEXRestatement.rhs and
three SBDF2 steps on the periodic channels and on the square and the cube without any wall, where the momentum system
has no Dirichlet row and the projection step a constant kernel; what nsfem_imex_info reports there is asserted."""
import numpy as np
import pytest

import _native as nat
import fem_oracle as fo
from gpu_common import box, cavity_bc, context, rel, velocity_bc
from imex_time_stepping import IMEXTimeStepping, IMEXType
from periodic_meshes import UNIFORM, lengths_of, periodic_axes, periodic_fields, periodic_fixture, wall_bc
from test_imex_solver_host import IMEXRestatement

pytestmark = pytest.mark.gpu

FORMS = ((0, "standard"), (1, "rotational"), (2, "divergence"), (3, "skew_symmetric"))
TYPES = (IMEXType.SBDF2, IMEXType.CNAB, IMEXType.mCNAB, IMEXType.CNLF)


def _opts(ctx, form_id, rtol=1e-13, precond=0):
    o = ctx.default_step_opts()
    o.convective_form = form_id
    for k in (o.momentum, o.poisson, o.correction):
        k.rtol = rtol
    o.momentum.precond = o.poisson.precond = precond
    return o


def _drive(ctx, orc, typ, form_id, steps, k, vbc, pbc, change_after=None, precond=0):
    """steps of the device driver and of the restatement side by side; returns the step infos"""
    ctx.set_dirichlet(nat.VELOCITY, *vbc)
    ctx.set_dirichlet(nat.PRESSURE, *pbc)
    opts = _opts(ctx, form_id, precond=precond)
    ts = IMEXTimeStepping(0.0, 1.0e9, typ, desired_start_time_step=k)
    infos = []
    for step in range(steps):
        if change_after is not None and step == change_after:
            ts.set_desired_next_step_size(0.5 * k)
        ts.update_coefficients()
        kk = ts.get_next_step_size()
        ctx.set_imex(ts.alpha, ts.beta, ts.gamma, kk)
        infos.append(ctx.step_imex(opts))
        orc.step(ts.alpha, ts.beta, ts.gamma, kk, vbc, pbc)
        us, u, p = ctx.get_state(nat.USTAR), ctx.get_state(nat.U0), ctx.get_state(nat.P)
        eu, es = rel(u, orc.vel[0]), rel(us, orc.ustar)
        ep = rel(p - p.mean(), orc.p - orc.p.mean()) if len(pbc[0]) == 0 else rel(p, orc.p)
        print("%s form %d step %d k %.4g: u* %.2e u %.2e p %.2e cg %d path %s" % (
            typ.name, form_id, step, kk, es, eu, ep, infos[-1].krylov_iterations_momentum, ctx.imex_info()["path"]))
        assert infos[-1].newton_iterations == 0
        assert es < 1e-9 and eu < 1e-9 and ep < 1e-8, (typ, form_id, step, es, eu, ep)
        ctx.advance(0)
        orc.advance()
        ts.advance_time()
    return infos


def _cavity(n=16):
    mesh, dm, marks = box(n, n)
    s = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
    return mesh, dm, marks, s


@pytest.fixture(scope="module")
def cavity16():
    return _cavity(16)


NO_PBC = (np.zeros(0, np.int32), np.zeros(0))


@pytest.mark.parametrize("form_id,form", FORMS)
@pytest.mark.parametrize("typ", TYPES, ids=lambda t: t.name)
def test_imex_cavity_steps_match_restatement(cavity16, typ, form_id, form):
    """cavity n = 16, Re = 100, k = 0.5 / 16, 4 steps"""
    mesh, dm, marks, s = cavity16
    ctx = context(mesh, dm)
    try:
        ctx.set_coeffs(1.0, 1.0, 0.01)
        orc = IMEXRestatement(s, dict(convective_term=1.0, pressure_term=1.0, viscous_term=0.01), form)
        _drive(ctx, orc, typ, form_id, 4, 0.5 / 16, cavity_bc(dm, marks), NO_PBC)
        info = ctx.imex_info()
        # a uniform binary-spacing lattice: every right-hand side in one launch; the matrix is built for the first-order
        # first step and once more for the second-order coefficients
        assert info["path"] == "lattice-kernel" and info["lattice_rhs"] == 4 and info["generic_rhs"] == 0
        assert info["matrix_builds"] == 2, info       # (step 1 is first order; then the coefficients stay)
    finally:
        ctx.close()


@pytest.mark.parametrize("form_id,form", FORMS)
@pytest.mark.parametrize("typ", TYPES, ids=lambda t: t.name)
def test_imex_step_size_change_rebuilds_matrix_and_reuses_stored_convection(cavity16, typ, form_id, form):
    """the step size is halved between steps 2 and 3: coefficients and matrix rebuilt, the stored N reused (the
    restatement keeps N(u1) in the same way; the right-hand sides stay one launch each)"""
    mesh, dm, marks, s = cavity16
    ctx = context(mesh, dm)
    try:
        ctx.set_coeffs(1.0, 1.0, 0.01)
        orc = IMEXRestatement(s, dict(convective_term=1.0, pressure_term=1.0, viscous_term=0.01), form)
        _drive(ctx, orc, typ, form_id, 4, 0.5 / 16, cavity_bc(dm, marks), NO_PBC, change_after=2)
        info = ctx.imex_info()
        assert info["lattice_rhs"] == 4 and info["generic_rhs"] == 0
        # builds: first step, second-order coefficients, the changed step, the constant step after it
        assert 3 <= info["matrix_builds"] <= 4, info
    finally:
        ctx.close()


def _open_channel(dm, marks, s, X):
    zero = lambda X: np.zeros((X.shape[0], 2))
    vbc = velocity_bc(dm, marks, [(1, zero), (3, zero), (4, zero)])
    facets = marks.facets_with_id(2)
    nodes = dm.facet_p2_nodes(facets)
    tvals = np.stack([0.3 * X[nodes, 1], -0.1 + 0.0 * X[nodes, 1]], axis=2)
    pn = np.unique(dm.facet_p1_nodes(facets))
    return vbc, (pn, 0.2 * np.ones(pn.size)), s.traction_vector(nodes, tvals)


@pytest.mark.parametrize("form_id,form", FORMS)
@pytest.mark.parametrize("typ", TYPES, ids=lambda t: t.name)
@pytest.mark.parametrize("variant", ["body_force", "traction", "traction_form"])
def test_imex_body_force_traction_and_traction_form(cavity16, variant, typ, form_id, form):
    """the cavity run with a body force / an open side carrying a traction (pressure pinned there) / both with the
    traction form of the viscous term (the generic right-hand-side path, a block system matrix)"""
    mesh, dm, marks, s = cavity16
    X = dm.p2_coords
    ctx = context(mesh, dm)
    try:
        cb = 1.0 if variant != "traction" else None
        coef = dict(convective_term=1.0, pressure_term=1.0, viscous_term=0.01, body_force_term=cb)
        orc = IMEXRestatement(s, coef, form, traction_form=(variant == "traction_form"))
        ctx.set_coeffs(1.0, 1.0, 0.01, cb)
        vbc, pbc = cavity_bc(dm, marks), NO_PBC
        if variant != "traction":
            f = np.stack([np.sin(np.pi * X[:, 1]), -1.0 + X[:, 0]], axis=1).ravel()
            orc.body_force = f
            ctx.set_state(nat.BODY_FORCE, f)
        if variant != "body_force":
            vbc, pbc, orc.traction = _open_channel(dm, marks, s, X)
            ctx.set_state(nat.TRACTION, orc.traction)
            u0 = np.zeros(dm.n_velocity)      # something to convect: a divergence-free field vanishing on the walls
            u0[0::2] = np.sin(np.pi * X[:, 1]) * 0.5
            u0[vbc[0]] = vbc[1]
            for lvl, slot in ((0, nat.U0), (1, nat.U1), (2, nat.U2)):
                orc.vel[lvl] = u0.copy()
                ctx.set_state(slot, u0)
        if variant == "traction_form":
            ctx.set_viscous_form(True)
        _drive(ctx, orc, typ, form_id, 4, 0.5 / 16, vbc, pbc)
        want = "generic" if variant == "traction_form" else "lattice-kernel"
        assert ctx.imex_info()["path"] == want
    finally:
        ctx.close()


def test_imex_multigrid_preconditioned_cg_same_answer():
    """precond = 1 (velocity and pressure V-cycles attached) gives the LU-accuracy answer"""
    from multigrid import attach_hierarchy
    mesh, dm, marks, s = _cavity(32)
    ctx = context(mesh, dm)
    try:
        assert attach_hierarchy(ctx, mesh, coarsest=4) == 3
        ctx.set_coeffs(1.0, 1.0, 0.01)
        orc = IMEXRestatement(s, dict(convective_term=1.0, pressure_term=1.0, viscous_term=0.01), "standard")
        infos = _drive(ctx, orc, IMEXType.SBDF2, 0, 4, 0.5 / 32, cavity_bc(dm, marks), NO_PBC, precond=1)
        assert all(i.newton_iterations == 0 for i in infos)
        # (Jacobi-CG needs several times as many iterations on this operator; the V-cycle count is mesh independent)
        assert all(0 < i.krylov_iterations_momentum <= 30 for i in infos), [i.krylov_iterations_momentum for i in infos]
    finally:
        ctx.close()


# ---------------------------------------------------------------- the right-hand side alone, bit for bit
def _graded(nx, ny):
    """binary spacings, 1/32 on the left half of the columns and 1/16 on the right (as test_gpu_jac_lattice_tables)"""
    from fem_mesh import FacetMarkers, TaylorHoodDofMap
    mesh, dm, marks = box(nx, ny, p1=(nx / 16.0, ny / 16.0))
    x = mesh.coords[:, 0] * 16.0
    h = nx // 2
    mesh.coords[:, 0] = np.where(x <= h, x / 32.0, h / 32.0 + (x - h) / 16.0)
    dm = TaylorHoodDofMap(mesh)
    marks = FacetMarkers(mesh)
    xr, yr = mesh.coords[:, 0].max(), mesh.coords[:, 1].max()
    marks.mark(lambda X: np.abs(X[:, 0]) < 1e-12, 1)
    marks.mark(lambda X: np.abs(X[:, 0] - xr) < 1e-12, 2)
    marks.mark(lambda X: np.abs(X[:, 1]) < 1e-12, 3)
    marks.mark(lambda X: np.abs(X[:, 1] - yr) < 1e-12, 4)
    return mesh, dm, marks


_FIRST = ((1.0, -1.0, 0.0), (1.0, 0.0), (1.0, 0.0, 0.0))                       # every type's first step: b1 = 0
_LATER = {"SBDF2": ((1.5, -2.0, 0.5), (2.0, -1.0), (1.0, 0.0, 0.0)),
          "CNAB": ((1.0, -1.0, 0.0), (1.5, -0.5), (0.5, 0.5, 0.0)),
          "mCNAB": ((1.0, -1.0, 0.0), (1.5, -0.5), (9.0 / 16.0, 3.0 / 8.0, 1.0 / 16.0)),
          "CNLF": ((0.5, 0.0, -0.5), (1.0, 0.0), (0.5, 0.0, 0.5))}


def _rhs_both_paths(mesh, dm, marks, form_ids, seed, coefficient_sets):
    bd, bv = cavity_bc(dm, marks)
    rng = np.random.default_rng(seed)
    u1, u2, f = (rng.standard_normal(dm.n_velocity) for _ in range(3))
    p_old = rng.standard_normal(dm.n_p1)
    ctx = context(mesh, dm)
    try:
        ctx.set_coeffs(0.8, 1.0, 0.02, 0.7)
        ctx.set_dirichlet(nat.VELOCITY, bd.astype(np.int32), bv)
        for slot, v in ((nat.U1, u1), (nat.U2, u2), (nat.P_OLD, p_old), (nat.BODY_FORCE, f)):
            ctx.set_state(slot, v)
        for form_id in form_ids:
            for tag, (alpha, beta, gamma) in coefficient_sets:
                ctx.set_imex(alpha, beta, gamma, 1.0 / 64.0)
                g_rhs, g_n1 = ctx.imex_rhs("generic", form_id)
                l_rhs, l_n1 = ctx.imex_rhs("lattice-kernel", form_id)
                assert np.isfinite(g_rhs).all() and np.abs(g_rhs).max() > 0.0
                assert np.array_equal(l_rhs, g_rhs), (form_id, tag, np.abs(l_rhs - g_rhs).max())
                assert np.array_equal(l_n1, g_n1), (form_id, tag, np.abs(l_n1 - g_n1).max())
        return g_rhs
    finally:
        ctx.close()


_SETS = (("first", _FIRST),) + tuple(_LATER.items())


@pytest.mark.parametrize("form_id,form", FORMS)
def test_rhs_one_launch_equals_generic_small_and_partial_tiles(form_id, form):
    """33 x 33 nodes (one partly filled tile) and 80 x 24 squares (3 x 4 tiles, the last ones partly filled)"""
    for nx, ny, p1 in ((16, 16, (1.0, 1.0)), (80, 24, (5.0, 1.5))):
        mesh, dm, marks = box(nx, ny, p1=p1)
        _rhs_both_paths(mesh, dm, marks, (form_id,), 100 * nx + form_id, _SETS)


@pytest.mark.parametrize("nx,ny", [(480, 216), (480, 224)])
def test_rhs_tile_counts_around_the_resident_slots(nx, ny):
    """496 and 528 tiles of 32 x 8 squares: just below and above the 512 resident workgroups"""
    mesh, dm, marks = box(nx, ny, p1=(nx / 16.0, ny / 16.0))
    _rhs_both_paths(mesh, dm, marks, (0, 3), nx + ny, (_SETS[0], _SETS[1]))


def test_rhs_full_size():
    """1025 x 1025 nodes"""
    mesh, dm, marks = box(512, 512)
    _rhs_both_paths(mesh, dm, marks, (0, 1, 2, 3), 512, (_SETS[0], _SETS[1]))


def test_stored_convection_vector_is_the_convection_residual():
    """NSFEM_CONV_N1 after a step = c_c N(u1) as launch_convection_residual gives it (the generic path's vector,
    which the one-launch path matches bit for bit above) and agrees with the oracle's; nsfem_advance moves it to
    NSFEM_CONV_N2"""
    mesh, dm, marks, s = _cavity(16)
    rng = np.random.default_rng(5)
    u1 = rng.standard_normal(dm.n_velocity)
    ctx = context(mesh, dm)
    try:
        ctx.set_coeffs(0.8, 1.0, 0.02)
        ctx.set_dirichlet(nat.VELOCITY, *cavity_bc(dm, marks))
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        ctx.set_state(nat.U1, u1)
        ctx.set_imex(*_LATER["SBDF2"], 1.0 / 64.0)
        _, n1_generic = ctx.imex_rhs("generic", 2)
        ctx.step_imex(_opts(ctx, 2))
        assert ctx.imex_info()["path"] == "lattice-kernel"
        n1 = ctx.get_state(nat.CONV_N1)
        assert np.array_equal(n1, n1_generic)
        assert rel(n1, 0.8 * s.convection_residual(u1, "divergence")) < 1e-13
        ctx.advance(0)
        assert np.array_equal(ctx.get_state(nat.CONV_N2), n1)
    finally:
        ctx.close()


def test_graded_lattice_takes_the_generic_path():
    mesh, dm, marks = _graded(36, 52)
    s = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
    ctx = context(mesh, dm)
    try:
        ctx.set_coeffs(1.0, 1.0, 0.01)
        orc = IMEXRestatement(s, dict(convective_term=1.0, pressure_term=1.0, viscous_term=0.01), "standard")
        _drive(ctx, orc, IMEXType.SBDF2, 0, 2, 1.0 / 64.0, cavity_bc(dm, marks), NO_PBC)
        info = ctx.imex_info()
        assert info["path"] == "generic" and info["generic_rhs"] == 2 and info["lattice_rhs"] == 0
        with pytest.raises(nat.NativeError):
            ctx.imex_rhs("lattice-kernel", 0)
    finally:
        ctx.close()


def test_rotating_frame_and_wrong_call_order_are_refused():
    mesh, dm, marks, s = _cavity(16)
    ctx = context(mesh, dm)
    try:
        ctx.set_coeffs(1.0, 1.0, 0.01, None, 1.0, 1.0)
        ctx.set_dirichlet(nat.VELOCITY, *cavity_bc(dm, marks))
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        with pytest.raises(nat.NativeError, match="nsfem_set_imex"):
            ctx.step_imex()
        ctx.set_imex(*_FIRST, 1.0 / 32.0)
        with pytest.raises(nat.NativeError, match="nsfem_set_bdf"):
            ctx.step_ipcs()
        ctx.set_angular_velocity(0.5, 0.0)
        with pytest.raises(nat.NativeError, match="rotating"):
            ctx.step_imex()
        ctx.set_angular_velocity(0.0, 0.0)
        ctx.step_imex()
        ctx.set_bdf((1.0, -1.0, 0.0), 1.0 / 32.0)       # back to the implicit scheme on the same context
        assert ctx.step_ipcs().newton_iterations > 0
    finally:
        ctx.close()


# ---------------------------------------------------------------- periodic dof maps
_PCOEF = dict(convective_term=0.8, pressure_term=1.0, viscous_term=0.02, body_force_term=0.7)
# The one-launch right-hand side runs where the stencil dictionary of the operators found a 2D lattice: every column
# offset of every row is dj * W + di with |di|, |dj| <= 2 and stays inside the W x H box (csrc/linalg.hip).  The seam
# rows of a periodic lattice couple to columns a whole line away, so no periodic lattice is eligible (and no 3D mesh
# is): nsfem_imex_info reports the generic path on all four fixtures, and asking for the other one is an argument error


def _periodic_case(name):
    mesh, dm, marks = periodic_fixture(name)
    s = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
    u, T = periodic_fields(dm.p2_coords, lengths_of(name), periodic_axes(name))
    vbc = wall_bc(name)
    assert (vbc[0].size == 0) == (name in ("psquare", "pbox3"))
    u1 = u.copy()
    u1[vbc[0]] = 0.0
    dim = mesh._dim
    f = np.roll(u.reshape(-1, dim), 1, axis=1).ravel() * 0.6
    u2 = 0.9 * u1 + 0.02 * f
    u2[vbc[0]] = 0.0
    return mesh, dm, s, vbc, u1, u2, f


@pytest.mark.parametrize("form_id,form", FORMS)
@pytest.mark.parametrize("name", UNIFORM)
def test_rhs_on_periodic_meshes_matches_the_restatement(name, form_id, form):
    """nsfem_imex_rhs, generic path, against IMEXRestatement.rhs for the first-step and the SBDF2 coefficients: 1e-13
    of the largest entry, the project's figure for element kernels against the oracle.  The one-launch path does not
    apply on a periodic lattice (above): asking for it is an argument error, not a wrong vector"""
    mesh, dm, s, vbc, u1, u2, f = _periodic_case(name)
    _, T = periodic_fields(dm.p1_coords, lengths_of(name), periodic_axes(name))
    orc = IMEXRestatement(s, _PCOEF, form)
    orc.vel[1], orc.vel[2], orc.p_old, orc.body_force = u1, u2, T, f
    ctx = context(mesh, dm)
    try:
        ctx.set_coeffs(0.8, 1.0, 0.02, 0.7)
        ctx.set_dirichlet(nat.VELOCITY, vbc[0].astype(np.int32), vbc[1])
        for slot, v in ((nat.U1, u1), (nat.U2, u2), (nat.P_OLD, T), (nat.BODY_FORCE, f)):
            ctx.set_state(slot, v)
        for tag, (alpha, beta, gamma) in (("first", _FIRST), ("SBDF2", _LATER["SBDF2"])):
            ctx.set_imex(alpha, beta, gamma, 1.0 / 64.0)
            orc.N2 = None
            want = orc.rhs(alpha, beta, gamma, 1.0 / 64.0)
            got, n1 = ctx.imex_rhs("generic", form_id)
            err = float(np.abs(got - want).max() / np.abs(want).max())
            nerr = float(np.abs(n1 - 0.8 * orc.N1).max() / np.abs(orc.N1).max())
            print("rhs %s form %d %s: %.2e, c_c N(u1) %.2e (of the largest entry)" % (name, form_id, tag, err, nerr))
            assert np.abs(orc.N1).max() > 1e-3
            assert err < 1e-13 and nerr < 1e-13
            with pytest.raises(nat.NativeError, match="one-launch") as refusal:
                ctx.imex_rhs("lattice-kernel", form_id)
            assert refusal.value.code == nat.ERR_ARG
    finally:
        ctx.close()


@pytest.mark.parametrize("name", UNIFORM)
def test_imex_steps_on_periodic_meshes_match_restatement(name):
    """three SBDF2 steps from a periodic velocity at two levels under a periodic body force, no-slip on the walls.  On
    psquare and pbox3 nothing is prescribed: the momentum matrix has no Dirichlet row, and the projection step has the
    constants in its kernel with no wall at all -- the device subtracts the mean, the restatement pins a node, the
    right-hand side is compatible (no boundary, no flux), so p is compared minus its mean"""
    mesh, dm, s, vbc, u1, u2, f = _periodic_case(name)
    ctx = context(mesh, dm)
    try:
        ctx.set_coeffs(0.8, 1.0, 0.02, 0.7)
        orc = IMEXRestatement(s, _PCOEF, "standard")
        orc.vel[1], orc.vel[2], orc.body_force = u1.copy(), u2.copy(), f
        for slot, v in ((nat.U1, u1), (nat.U2, u2), (nat.BODY_FORCE, f)):
            ctx.set_state(slot, v)
        _drive(ctx, orc, IMEXType.SBDF2, 0, 3, 0.02, (vbc[0].astype(np.int32), vbc[1]), NO_PBC)
        info = ctx.imex_info()
        assert info["path"] == "generic" and (info["lattice_rhs"], info["generic_rhs"]) == (0, 3), info
        assert np.abs(orc.vel[1]).max() > 0.5 and np.abs(orc.p_old - orc.p_old.mean()).max() > 0.1
    finally:
        ctx.close()


# ---------------------------------------------------------------- through the class
def test_solver_class_equals_driving_the_steps_by_hand():
    """IMEXIPCSSolver through InstationaryProblem (set_solver_class; the problem builds the IMEXTimeStepping the
    class names) on the cavity problem spec: bit for bit what set_imex / step_imex / advance give through the C ABI"""
    from ns_imex_solver import IMEXIPCSSolver
    from problem_specs import build_problem
    n, steps, dt = 16, 4, 0.5 / 16
    spec = dict(name="Cavity", mesh=("cube", 2, n), scheme="ipcs", numbers=dict(Re=100.0),
                clock=dict(dt=dt, steps=steps), start={"velocity": (0.0, 0.0), "pressure": 0.0},
                bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_slip", "bottom"), ("velocity", "top", (1.0, 0.0))])
    problem = build_problem(spec)
    problem.set_solver_class(IMEXIPCSSolver)
    problem.compute_cfl = False
    problem.solve_problem()
    solver = problem._get_solver()
    assert isinstance(solver, IMEXIPCSSolver) and isinstance(problem._time_stepping, IMEXTimeStepping)
    assert problem._time_stepping.step_number == steps
    info = solver._ctx.imex_info()
    assert info["lattice_rhs"] == steps and info["generic_rhs"] == 0
    assert solver.last_step_info.newton_iterations == 0 and solver.last_step_info.krylov_iterations_momentum > 0
    u_cls, p_cls = solver._ctx.get_state(nat.U1), solver._ctx.get_state(nat.P_OLD)
    assert np.array_equal(solver.solution.split()[0].vector(), solver._ctx.get_state(nat.U0))
    # ---- the same steps through the C ABI on a fresh context
    from multigrid import attach_hierarchy
    dm, mesh = solver._dofmap, solver._mesh
    ctx = nat.NsfemContext(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, dm.n_p2, dm.n_p1)
    try:
        if solver._mg_levels is not None:
            attach_hierarchy(ctx, mesh)
        coef = solver._equation_coefficients
        ctx.set_coeffs(coef["convective_term"], coef["pressure_term"], coef["viscous_term"])
        bd, bv = solver._dirichlet_bcs["velocity"]
        ctx.set_dirichlet(nat.VELOCITY, np.asarray(bd, np.int32), np.asarray(bv, float))
        ctx.set_dirichlet(nat.PRESSURE, np.zeros(0, np.int32), np.zeros(0))
        opts = solver._step_options()
        ts = IMEXTimeStepping(0.0, 1.0, IMEXType.SBDF2, desired_start_time_step=dt)
        for _ in range(steps):
            ts.update_coefficients()
            ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
            ctx.step_imex(opts)
            ts.advance_time()
            ctx.advance(0)
        u_abi, p_abi = ctx.get_state(nat.U1), ctx.get_state(nat.P_OLD)
    finally:
        ctx.close()
    assert np.abs(u_cls).max() > 0.5
    assert np.array_equal(u_cls, u_abi) and np.array_equal(p_cls, p_abi)
