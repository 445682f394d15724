"""Rotating frames in the IMEX step on the GPU (nsfem_set_imex_rotation: Coriolis term folded into the convection
element kernels, Euler term in the step-constant vector) against RotatingIMEXRestatement of
tests/test_imex_rotation_host.py, the one-launch right-hand side (k_jac_lattice's rotating right-hand-side modes)
against the generic launch sequence bit for bit, and the opt-in semantics.

Tolerances: those of tests/test_gpu_imex.py for the same quantities, step counts and Krylov settings (rtol 1e-13) -- u*, u
1e-9 and p minus its mean 1e-8, relative; the stored vector against the oracle operators 1e-13 (the bound of
test_stored_convection_vector_is_the_convection_residual); partitioned against single context u 1e-11, p 1e-10 (exact
halo mode, tests/test_gpu_imex_partition.py).

Every test here fails on a build without nsfem_set_imex_rotation: the symbol is missing."""
import numpy as np
import pytest

import _native as nat
import fem_oracle as fo
from general_tet_mesh import SMALL, general_tets, shear_bc
from gpu_common import box, cavity_bc, context, rel
from imex_time_stepping import IMEXTimeStepping, IMEXType
from partition import StripPartition
from periodic_meshes import periodic_fixture, wall_bc
from test_gpu_3d import box3, context3, lid_bc
from test_gpu_imex import _LATER, _SETS, FORMS, NO_PBC, TYPES, _graded, _opts
from test_gpu_imex_partition import _cavity_bc, _compare, _on_ranks, _plain_partition
from test_imex_rotation_host import RotatingIMEXRestatement
from test_scalar_transport_host import ScalarIMEXRestatement, smooth_fields

pytestmark = pytest.mark.gpu

_CCOR, _CE = 1.5, 0.7


def _omega(t):
    return 0.5 + 0.8 * t


@pytest.fixture(scope="module")
def cavity16():
    mesh, dm, marks = box(16, 16)
    return mesh, dm, marks, fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)


# ---------------------------------------------------------------- 1. opt-in
def test_opt_in_semantics_and_zero_rotation_is_bit_identical(cavity16):
    mesh, dm, marks, s = cavity16
    vbc = cavity_bc(dm, marks)
    rng = np.random.default_rng(11)
    u1, u2 = rng.standard_normal(dm.n_velocity), rng.standard_normal(dm.n_velocity)

    def make():
        ctx = context(mesh, dm)
        ctx.set_coeffs(1.0, 1.0, 0.01, None, _CCOR, _CE)
        ctx.set_dirichlet(nat.VELOCITY, *vbc)
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        return ctx

    ctx = make()
    try:
        assert ctx.imex_rotation_info() == dict(treatment=0, rotating_rhs=0, recomputed=0)
        ctx.set_imex(*_LATER["SBDF2"], 1.0 / 32.0)
        ctx.set_angular_velocity(0.5, 0.0)
        with pytest.raises(nat.NativeError, match="rotating"):          # default: refused, as before
            ctx.step_imex()
        with pytest.raises(nat.NativeError, match="rotating"):
            ctx.imex_rhs("generic", 0)
        ctx.set_imex_rotation(1)
        ctx.step_imex()                                                  # treatment 1: the step runs
        info = ctx.imex_rotation_info()
        assert info["treatment"] == 1 and info["rotating_rhs"] == 1, info
        assert ctx.imex_info()["path"] == "lattice-kernel"
        ctx.set_imex_rotation(0)
        with pytest.raises(nat.NativeError, match="rotating"):          # treatment 0 again: refused
            ctx.step_imex()
        with pytest.raises(nat.NativeError, match="treatment"):
            ctx.set_imex_rotation(2)
    finally:
        ctx.close()

    # treatment 1 with zero rotation: the non-rotating kernels, bit for bit a context that never made the call
    a, b = make(), make()
    try:
        a.set_imex_rotation(1, 0.0, 0.0)
        a.set_angular_velocity(0.0, 0.0)
        out = []
        for ctx in (a, b):
            ctx.set_state(nat.U1, u1)
            ctx.set_state(nat.U2, u2)
            ctx.set_imex(*_LATER["SBDF2"], 1.0 / 32.0)
            res = [ctx.imex_rhs(path, 0) for path in ("generic", "lattice-kernel")]
            ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=1.0 / 32.0)
            ctx.set_state(nat.U1, np.zeros(dm.n_velocity))
            ctx.set_state(nat.U2, np.zeros(dm.n_velocity))
            for _ in range(2):
                ts.update_coefficients()
                ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
                ctx.step_imex(_opts(ctx, 0, rtol=1e-10))
                state = [ctx.get_state(slot) for slot in (nat.U0, nat.P, nat.CONV_N1)]
                ctx.advance(0)
                ts.advance_time()
            out.append((res, state))
        (res_a, state_a), (res_b, state_b) = out
        for (rhs_a, n1_a), (rhs_b, n1_b) in zip(res_a, res_b):
            assert np.abs(rhs_b).max() > 0.0
            assert np.array_equal(rhs_a, rhs_b) and np.array_equal(n1_a, n1_b)
        for va, vb in zip(state_a, state_b):
            assert np.abs(vb).max() > 0.0 and np.array_equal(va, vb)
        assert a.imex_rotation_info()["rotating_rhs"] == 0
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 2. the stored vector
def _stored_vector_case(mesh, dm, s, make, vbc, w, cc, form_id, form, seed):
    dim = s.dim
    rng = np.random.default_rng(seed)
    u1 = rng.standard_normal(dm.n_velocity)
    coef = dict(convective_term=cc, pressure_term=1.0, viscous_term=0.02, coriolis_term=_CCOR, euler_term=_CE)
    orc = RotatingIMEXRestatement(s, coef, form)
    want = orc.explicit_vector(u1, w)
    ctx = make(mesh, dm)
    try:
        ctx.set_coeffs(cc, 1.0, 0.02, None, _CCOR, _CE)
        ctx.set_dirichlet(nat.VELOCITY, *vbc)
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        ctx.set_state(nat.U1, u1)
        ctx.set_imex(*_LATER["SBDF2"], 1.0 / 64.0)
        ctx.set_imex_rotation(1, w, w)
        _, n1_generic = ctx.imex_rhs("generic", form_id)
        ctx.step_imex(_opts(ctx, form_id))
        n1 = ctx.get_state(nat.CONV_N1)
        err = rel(n1, want)
        print("dim %d c_c %s form %d: stored vector rel %.2e path %s" % (dim, cc, form_id, err, ctx.imex_info()["path"]))
        assert np.array_equal(n1, n1_generic)
        assert np.linalg.norm(want) > 1e-3 and err < 1e-13, (dim, cc, form_id, err)
        # with c_c = None the element kernel still ran: the vector is the Coriolis vector alone
        assert ctx.imex_rotation_info()["rotating_rhs"] == 2
        if dim == 2:
            assert ctx.imex_info()["path"] == ("lattice-kernel" if cc else "generic")
        ctx.advance(0)
        assert np.array_equal(ctx.get_state(nat.CONV_N2), n1)
    finally:
        ctx.close()


@pytest.mark.parametrize("cc", [0.8, None])
@pytest.mark.parametrize("form_id,form", FORMS)
def test_stored_vector_is_convection_plus_coriolis(cavity16, form_id, form, cc):
    """box(16, 16), random u1: NSFEM_CONV_N1 after a step = the generic imex_rhs vector bit for bit, and
    0.8 conv(u1) + 2 c_cor w M J u1 from the oracle operators to 1e-13"""
    mesh, dm, marks, s = cavity16
    _stored_vector_case(mesh, dm, s, context, cavity_bc(dm, marks), 0.7, cc, form_id, form, 5)


@pytest.mark.parametrize("cc", [0.8, None])
@pytest.mark.parametrize("form_id,form", FORMS)
def test_stored_vector_3d(form_id, form, cc):
    """the Kuhn cube n = 3 with Omega = (0.3, -0.2, 0.5): k3_conv_cell's rotating instantiation"""
    mesh, dm, marks = box3((3, 3, 3))
    s = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
    _stored_vector_case(mesh, dm, s, context3, lid_bc(dm, marks), np.array([0.3, -0.2, 0.5]), cc, form_id, form, 6)


@pytest.mark.parametrize("cc", [0.8, None])
@pytest.mark.parametrize("form_id,form", FORMS)
def test_stored_vector_on_general_tetrahedra(form_id, form, cc):
    """the 72 general tetrahedra of tests/general_tet_mesh.py (cells of both orientations and of different volumes, no
    zero in any J^-1) with Omega = (0.3, -0.2, 0.5): the same instantiation, the same 1e-13"""
    mesh, dm, marks = general_tets(*SMALL)
    s = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
    _stored_vector_case(mesh, dm, s, context3, lid_bc(dm, marks), np.array([0.3, -0.2, 0.5]), cc, form_id, form, 6)


def test_stored_vector_on_the_periodic_channel():
    """pchan3 of tests/periodic_meshes.py (periodic in x and z, no-slip on the walls in y) with Omega = (0.3, -0.2, 0.5),
    the skew-symmetric form: the Coriolis vector is gathered and scattered through the identified dofs of the seam
    cells; the same 1e-13"""
    mesh, dm, marks = periodic_fixture("pchan3")
    assert dm.n_p2 == 180 and dm.n_p1 < mesh.num_vertices()
    s = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
    _stored_vector_case(mesh, dm, s, context3, wall_bc("pchan3"), np.array([0.3, -0.2, 0.5]), 0.8, *FORMS[3], 6)


# ---------------------------------------------------------------- 3. one launch against generic, bit for bit
@pytest.mark.parametrize("form_id,form", FORMS)
def test_rotating_rhs_one_launch_equals_generic(form_id, form):
    """33 x 33 nodes (one partly filled tile) and 80 x 24 squares (partly filled last tiles); the five coefficient sets of
    tests/test_gpu_imex.py; omega_n = 0.7, omega_nm1 = -0.4, c_cor = 1.5, Euler term on"""
    for nx, ny, p1 in ((16, 16, (1.0, 1.0)), (80, 24, (5.0, 1.5))):
        mesh, dm, marks = box(nx, ny, p1=p1)
        bd, bv = cavity_bc(dm, marks)
        rng = np.random.default_rng(100 * nx + form_id)
        u1, u2, f = (rng.standard_normal(dm.n_velocity) for _ in range(3))
        p_old = rng.standard_normal(dm.n_p1)
        ctx = context(mesh, dm)
        try:
            ctx.set_coeffs(0.8, 1.0, 0.02, 0.7, _CCOR, _CE)
            ctx.set_dirichlet(nat.VELOCITY, bd.astype(np.int32), bv)
            for slot, v in ((nat.U1, u1), (nat.U2, u2), (nat.P_OLD, p_old), (nat.BODY_FORCE, f)):
                ctx.set_state(slot, v)
            ctx.set_imex_rotation(0)
            ctx.set_imex(*_LATER["SBDF2"], 1.0 / 64.0)
            plain_rhs, plain_n1 = ctx.imex_rhs("generic", form_id)
            ctx.set_angular_velocity(0.7, 0.3)
            ctx.set_imex_rotation(1, 0.7, -0.4)
            for tag, (alpha, beta, gamma) in _SETS:
                ctx.set_imex(alpha, beta, gamma, 1.0 / 64.0)
                g_rhs, g_n1 = ctx.imex_rhs("generic", form_id)
                l_rhs, l_n1 = ctx.imex_rhs("lattice-kernel", form_id)
                assert np.isfinite(g_rhs).all() and np.abs(g_rhs).max() > 0.0
                assert np.array_equal(l_rhs, g_rhs), (nx, form_id, tag, np.abs(l_rhs - g_rhs).max())
                assert np.array_equal(l_n1, g_n1), (nx, form_id, tag, np.abs(l_n1 - g_n1).max())
            # (the rotation is in there: neither vector is the non-rotating one)
            assert not np.array_equal(g_n1, plain_n1) and not np.array_equal(g_rhs, plain_rhs)
            assert ctx.imex_rotation_info()["rotating_rhs"] == 2 * len(_SETS)
        finally:
            ctx.close()


# ---------------------------------------------------------------- 4. / 5. steps against the restatement
def _drive(ctx, orc, typ, form_id, steps, k, vbc, change_after=None, perturb_at=None):
    """device and restatement side by side; Omega(t) = 0.5 + 0.8 t at the old levels, dOmega/dt = 0.8"""
    ctx.set_dirichlet(nat.VELOCITY, *vbc)
    ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
    opts = _opts(ctx, form_id)
    ts = IMEXTimeStepping(0.0, 1.0e9, typ, desired_start_time_step=k)
    for step in range(steps):
        if change_after is not None and step == change_after:
            ts.set_desired_next_step_size(0.5 * k)
        ts.update_coefficients()
        kk = ts.get_next_step_size()
        w1, w2 = _omega(ts.current_time), _omega(ts.previous_time)
        if perturb_at is not None and step == perturb_at:
            w2 += 0.1                                  # not the omega_n of the step before
        ctx.set_imex(ts.alpha, ts.beta, ts.gamma, kk)
        ctx.set_angular_velocity(_omega(ts.next_time), 0.8)
        ctx.set_imex_rotation(1, w1, w2 if step > 0 else None)
        orc.w1, orc.w2, orc.w_dot = w1, w2, 0.8
        info = ctx.step_imex(opts)
        orc.step(ts.alpha, ts.beta, ts.gamma, kk, vbc, NO_PBC)
        us, u, p = ctx.get_state(nat.USTAR), ctx.get_state(nat.U0), ctx.get_state(nat.P)
        eu, es, ep = rel(u, orc.vel[0]), rel(us, orc.ustar), rel(p - p.mean(), orc.p - orc.p.mean())
        print("%s form %d step %d k %.4g: u* %.2e u %.2e p %.2e cg %d path %s" % (
            typ.name, form_id, step, kk, es, eu, ep, info.krylov_iterations_momentum, ctx.imex_info()["path"]))
        assert info.newton_iterations == 0
        assert es < 1e-9 and eu < 1e-9 and ep < 1e-8, (typ, form_id, step, es, eu, ep)
        ctx.advance(0)
        orc.advance()
        ts.advance_time()


_COEF = dict(convective_term=1.0, pressure_term=1.0, viscous_term=0.01, coriolis_term=_CCOR, euler_term=_CE)


@pytest.mark.parametrize("form_id,form", [FORMS[0], FORMS[3]])
@pytest.mark.parametrize("typ", TYPES, ids=lambda t: t.name)
def test_rotating_cavity_steps_match_restatement(cavity16, typ, form_id, form):
    """cavity n = 16, k = 0.5 / 16, 4 steps, the step size halved after step 2: one launch per right-hand side and no
    recomputation of the stored vector.  Second run: the omega_nm1 of step 2 is not the omega_n of step 1 -- the stored
    vector is formed again (where the scheme reads it: CNLF has beta_1 = 0 and never does) and the fields still match
    the restatement fed the same values"""
    mesh, dm, marks, s = cavity16
    vbc = cavity_bc(dm, marks)
    for perturb_at in (None, 2):
        ctx = context(mesh, dm)
        try:
            ctx.set_coeffs(1.0, 1.0, 0.01, None, _CCOR, _CE)
            orc = RotatingIMEXRestatement(s, _COEF, form)
            _drive(ctx, orc, typ, form_id, 4, 0.5 / 16, vbc, change_after=2, perturb_at=perturb_at)
            info, rot = ctx.imex_info(), ctx.imex_rotation_info()
            assert info["path"] == "lattice-kernel" and info["lattice_rhs"] == 4 and info["generic_rhs"] == 0
            assert rot["rotating_rhs"] == 4
            want = 0 if (perturb_at is None or typ is IMEXType.CNLF) else 1
            assert rot["recomputed"] == orc.recomputed == want, (rot, orc.recomputed)
        finally:
            ctx.close()


def test_rotating_steps_on_a_graded_lattice_take_the_generic_path():
    mesh, dm, marks = _graded(36, 52)
    s = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
    ctx = context(mesh, dm)
    try:
        ctx.set_coeffs(1.0, 1.0, 0.01, None, _CCOR, _CE)
        orc = RotatingIMEXRestatement(s, _COEF, "standard")
        _drive(ctx, orc, IMEXType.SBDF2, 0, 2, 1.0 / 64.0, cavity_bc(dm, marks))
        info = ctx.imex_info()
        assert info["path"] == "generic" and info["generic_rhs"] == 2 and info["lattice_rhs"] == 0
        assert ctx.imex_rotation_info()["rotating_rhs"] == 2
    finally:
        ctx.close()


# ---------------------------------------------------------------- 6. 3D
def test_rotating_3d_steps_match_restatement():
    """unit cube n = 4, lid-driven, SBDF2, 3 steps, Omega(t) = (0.3, -0.2, 0.5) (1 + t), dOmega/dt = (0.3, -0.2, 0.5);
    tolerances of test_imex_3d_steps_match_restatement"""
    _rotating_3d_steps(*box3((4, 4, 4)), lid_bc)


def test_rotating_3d_steps_on_general_tetrahedra_match_restatement():
    """the same three steps on the 72 general tetrahedra: the Coriolis kernel and the Euler vector M (dOmega/dt x x) on
    cells of both orientations, inside the steps; boundary values: the solenoidal shear of general_tet_mesh.shear_bc (a
    lid on the oblique face 6 has a net flux: no pure Neumann projection step)"""
    _rotating_3d_steps(*general_tets(*SMALL), shear_bc)


def _rotating_3d_steps(mesh, dm, marks, boundary_values):
    s = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
    vbc = boundary_values(dm, marks)
    axis = np.array([0.3, -0.2, 0.5])
    ctx = context3(mesh, dm)
    try:
        ctx.set_coeffs(1.0, 1.0, 0.01, None, _CCOR, _CE)
        ctx.set_dirichlet(nat.VELOCITY, *vbc)
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        orc = RotatingIMEXRestatement(s, _COEF, "standard")
        opts = _opts(ctx, 0)
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=0.05)
        for step in range(3):
            ts.update_coefficients()
            kk = ts.get_next_step_size()
            w1, w2 = axis * (1.0 + ts.current_time), axis * (1.0 + ts.previous_time)
            ctx.set_imex(ts.alpha, ts.beta, ts.gamma, kk)
            ctx.set_angular_velocity(axis * (1.0 + ts.next_time), axis)
            ctx.set_imex_rotation(1, w1, w2 if step > 0 else None)
            orc.w1, orc.w2, orc.w_dot = w1, w2, axis
            info = ctx.step_imex(opts)
            orc.step(ts.alpha, ts.beta, ts.gamma, kk, vbc, NO_PBC)
            us, u, p = ctx.get_state(nat.USTAR), ctx.get_state(nat.U0), ctx.get_state(nat.P)
            es, eu, ep = rel(us, orc.ustar), rel(u, orc.vel[0]), rel(p - p.mean(), orc.p - orc.p.mean())
            print("3D step %d: u* %.2e u %.2e p %.2e cg %d" % (step, es, eu, ep, info.krylov_iterations_momentum))
            assert info.newton_iterations == 0
            assert es < 1e-9 and eu < 1e-9 and ep < 1e-8, (step, es, eu, ep)
            ctx.advance(0)
            orc.advance()
            ts.advance_time()
        assert ctx.imex_info()["path"] == "generic"
        rot = ctx.imex_rotation_info()
        assert rot["rotating_rhs"] == 3 and rot["recomputed"] == 0, rot
    finally:
        ctx.close()


# ---------------------------------------------------------------- 7. partitioned strips
def _run_rank(ctx, dm, rotating, nsteps, k, out, key):
    ctx.set_coeffs(1.0, 1.0, 0.01, None, _CCOR, _CE)
    ctx.set_dirichlet(nat.VELOCITY, *_cavity_bc(dm))
    ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
    opts = ctx.default_step_opts()
    for o in (opts.momentum, opts.poisson, opts.correction):
        o.rtol = 1e-12
    ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=k)
    infos, per_step = [], []
    for step in range(nsteps):
        ts.update_coefficients()
        ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
        scale = 1.0 if rotating else 0.0
        ctx.set_angular_velocity(scale * _omega(ts.next_time), scale * 0.8)
        ctx.set_imex_rotation(1, scale * _omega(ts.current_time), scale * _omega(ts.previous_time) if step > 0 else None)
        c0 = ctx.comm_stats()
        infos.append(ctx.step_imex(opts))
        c1 = ctx.comm_stats()
        per_step.append((c1["exchanges"] - c0["exchanges"], c1["allreduce_calls"] - c0["allreduce_calls"]))
        ctx.advance(0)
        ts.advance_time()
    # the messages of one right-hand side alone (u2 came from advance: u1 travels, nothing else)
    c0 = ctx.comm_stats()
    ctx.imex_rhs("generic", 0)
    c1 = ctx.comm_stats()
    ctx.imex_rhs("lattice-kernel", 0)
    c2 = ctx.comm_stats()
    rhs_messages = [(b["exchanges"] - a["exchanges"], b["allreduce_calls"] - a["allreduce_calls"])
                    for a, b in ((c0, c1), (c1, c2))]
    out[key] = dict(u=ctx.get_state(nat.U1), p=ctx.get_state(nat.P_OLD), infos=infos, imex=ctx.imex_info(),
                    rot=ctx.imex_rotation_info(), per_step=per_step, rhs_messages=rhs_messages)


def _its(info):
    return info.krylov_iterations_momentum + info.krylov_iterations_poisson + info.krylov_iterations_correction


def test_partitioned_rotating_steps_equal_single_context_and_add_no_message():
    """2 in-process strip ranks, n = 32, 3 steps, exact halo mode: against the single context u 1e-11, p 1e-10; the
    one-launch path on every rank; halo exchanges and all-reduces of every step equal those of the same run with
    Omega = 0.

    The two runs solve other right-hand sides, so a CG solve of one may take an iteration more than its counterpart
    (measured: steps 1 and 2 differ by one iteration in all, step 3 by none).  An iteration of the three CG solves costs
    one halo exchange and two all-reduces (linalg.hip: one operator product, two fused dot-product launches); where the
    iteration counts of a step differ, the step's messages must differ by exactly that and by nothing else.  The
    messages of a right-hand side alone (nsfem_imex_rhs, either path) are compared without any such allowance."""
    n, size, nsteps, k = 32, 2, 3, 0.01
    mesh, dm, _ = box(n, n)
    ref = {}
    ctx0 = context(mesh, dm)
    try:
        _run_rank(ctx0, dm, True, nsteps, k, ref, 0)
    finally:
        ctx0.close()
    ref = ref[0]
    assert ref["rot"]["rotating_rhs"] == nsteps + 2 and ref["imex"]["path"] == "lattice-kernel"
    parts = [StripPartition((0.0, 0.0), (1.0, 1.0), n, n, r, size) for r in range(size)]
    runs = {}
    for rotating in (True, False):
        def work(r, part, ctx, out):
            _plain_partition(ctx, part, r, size, n, n)
            _run_rank(ctx, part.dofmap, rotating, nsteps, k, out, r)
        runs[rotating] = _on_ranks(parts, work)
    _compare(parts, runs[True], ref, False)
    for r in range(size):
        rot, plain = runs[True][r], runs[False][r]
        info = rot["imex"]
        assert info["path"] == "lattice-kernel" and info["lattice_rhs"] == nsteps and info["generic_rhs"] == 0, (r, info)
        assert rot["rot"]["rotating_rhs"] == nsteps + 2 and rot["rot"]["recomputed"] == 0, (r, rot["rot"])
        assert plain["rot"]["rotating_rhs"] == 0 and plain["imex"]["path"] == "lattice-kernel"
        print("rank %d (exchanges, all-reduces) per step: rotating %s, Omega = 0 %s; CG iterations %s, %s; one "
              "right-hand side %s, %s" % (r, rot["per_step"], plain["per_step"], [_its(i) for i in rot["infos"]],
                                          [_its(i) for i in plain["infos"]], rot["rhs_messages"], plain["rhs_messages"]))
        assert rot["rhs_messages"] == plain["rhs_messages"] == [(1, 0), (1, 0)], (r, rot["rhs_messages"])
        for (ex_r, ar_r), (ex_0, ar_0), ir, i0 in zip(rot["per_step"], plain["per_step"], rot["infos"], plain["infos"]):
            more = _its(ir) - _its(i0)
            assert (ex_r - more, ar_r - 2 * more) == (ex_0, ar_0), (r, ex_r, ar_r, ex_0, ar_0, more)


# ---------------------------------------------------------------- 8. Boussinesq
def test_rotating_boussinesq_steps_match_the_restatements():
    """box(8, 8) with buoyancy and rotation, 3 SBDF2 steps of step_scalar_imex + step_imex against
    ScalarIMEXRestatement and RotatingIMEXRestatement; tolerances of
    test_transport_and_flow_steps_match_the_restatements (T, u*, u 1e-9, p 1e-8)"""
    mesh, dm, marks = box(8, 8)
    s = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
    X = dm.p2_coords
    b = (0.3, 1.0)
    kappa, k = 0.05, 0.5 / 8
    vbc = cavity_bc(dm, marks)
    left = np.unique(dm.facet_p2_nodes(marks.facets_with_id(1)))
    right = np.unique(dm.facet_p2_nodes(marks.facets_with_id(2)))
    tbc = (np.concatenate([left, right]), np.concatenate([0.5 + X[left, 1], -0.2 + 0.0 * X[right, 1]]))
    _, T_init = smooth_fields(X)
    f = np.stack([np.sin(np.pi * X[:, 1]), -1.0 + X[:, 0]], axis=1).ravel()
    coef = dict(_COEF, body_force_term=1.0)
    flow = RotatingIMEXRestatement(s, coef, "standard")
    orc = ScalarIMEXRestatement(s, kappa, "standard")
    orc.T[0], orc.T[1] = T_init.copy(), T_init.copy()
    ctx = context(mesh, dm)
    try:
        ctx.set_coeffs(1.0, 1.0, 0.01, 1.0, _CCOR, _CE)
        ctx.set_dirichlet(nat.VELOCITY, *vbc)
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        ctx.set_dirichlet(nat.SCALAR, *tbc)
        ctx.set_scalar(kappa, b, 0)
        ctx.set_state(nat.BODY_FORCE, f)
        ctx.set_state(nat.T0, T_init)
        ctx.set_state(nat.T1, T_init)
        opts = _opts(ctx, 0)
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=k)
        for step in range(3):
            ts.update_coefficients()
            kk = ts.get_next_step_size()
            w1, w2 = _omega(ts.current_time), _omega(ts.previous_time)
            ctx.set_imex(ts.alpha, ts.beta, ts.gamma, kk)
            ctx.set_angular_velocity(_omega(ts.next_time), 0.8)
            ctx.set_imex_rotation(1, w1, w2 if step > 0 else None)
            flow.w1, flow.w2, flow.w_dot = w1, w2, 0.8
            si = ctx.step_scalar_imex(rtol=1e-13)
            orc.step(ts.alpha, ts.beta, ts.gamma, kk, flow.vel[1], flow.vel[2], tbc)
            et = rel(ctx.get_state(nat.T0), orc.T[0])
            flow.body_force = f + np.outer(orc.T[0], b).ravel()
            ctx.step_imex(opts)
            flow.step(ts.alpha, ts.beta, ts.gamma, kk, vbc, NO_PBC)
            us, u, p = ctx.get_state(nat.USTAR), ctx.get_state(nat.U0), ctx.get_state(nat.P)
            es, eu, ep = rel(us, flow.ustar), rel(u, flow.vel[0]), rel(p - p.mean(), flow.p - flow.p.mean())
            print("Boussinesq step %d: T %.2e u* %.2e u %.2e p %.2e" % (step, et, es, eu, ep))
            assert si.converged and et < 1e-9, (step, et)
            assert es < 1e-9 and eu < 1e-9 and ep < 1e-8, (step, es, eu, ep)
            ctx.advance(0)
            orc.advance()
            flow.advance()
            ts.advance_time()
        assert ctx.imex_rotation_info()["rotating_rhs"] == 3
        assert np.array_equal(ctx.get_state(nat.BODY_FORCE), f)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 9. through the class
def test_solver_class_with_an_angular_velocity_equals_driving_the_abi_by_hand():
    """IMEXIPCSSolver through InstationaryProblem with an AngularVelocityVector ramp Omega(t) = 0.8 t (spec key "spin"),
    cavity n = 16, 3 steps: bit for bit what the C ABI gives when handed the same three angular velocities per step --
    Omega and dOmega/dt where the problem classes keep the vector (t^n during the step n -> n + 1), Omega(t^n) and
    Omega(t^(n-1)) for the extrapolated Coriolis term.  The first step starts from Omega(0) = 0: non-rotating kernels
    with the Euler term; steps 2 and 3 run the rotating one-launch right-hand side."""
    from ns_imex_solver import IMEXIPCSSolver
    from problem_specs import build_problem
    n, steps, dt, rate = 16, 3, 0.5 / 16, 0.8
    spec = dict(name="RotatingCavity", mesh=("cube", 2, n), scheme="ipcs", numbers=dict(Re=100.0, Ro=0.5),
                clock=dict(dt=dt, steps=steps), start={"velocity": (0.0, 0.0), "pressure": 0.0}, spin=("ramp", 10.0, rate),
                bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_slip", "bottom"), ("velocity", "top", (1.0, 0.0))])
    problem = build_problem(spec)
    problem.set_solver_class(IMEXIPCSSolver)
    problem.compute_cfl = False
    problem.solve_problem()
    solver = problem._get_solver()
    assert isinstance(solver, IMEXIPCSSolver) and problem._time_stepping.step_number == steps
    info, rot = solver._ctx.imex_info(), solver._ctx.imex_rotation_info()
    assert info["lattice_rhs"] == steps and info["generic_rhs"] == 0
    assert rot == dict(treatment=1, rotating_rhs=steps - 1, recomputed=0), rot
    u_cls, p_cls = solver._ctx.get_state(nat.U1), solver._ctx.get_state(nat.P_OLD)
    from multigrid import attach_hierarchy
    dm, mesh = solver._dofmap, solver._mesh
    ctx = nat.NsfemContext(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, dm.n_p2, dm.n_p1)
    try:
        if solver._mg_levels is not None:
            attach_hierarchy(ctx, mesh)
        coef = solver._equation_coefficients
        assert coef["coriolis_term"] == 2.0 and coef["euler_term"] == 2.0
        ctx.set_coeffs(coef["convective_term"], coef["pressure_term"], coef["viscous_term"], coef["body_force_term"],
                       coef["coriolis_term"], coef["euler_term"])
        bd, bv = solver._dirichlet_bcs["velocity"]
        ctx.set_dirichlet(nat.VELOCITY, np.asarray(bd, np.int32), np.asarray(bv, float))
        ctx.set_dirichlet(nat.PRESSURE, np.zeros(0, np.int32), np.zeros(0))
        opts = solver._step_options()
        ts = IMEXTimeStepping(0.0, 1.0, IMEXType.SBDF2, desired_start_time_step=dt)
        for step in range(steps):
            ts.update_coefficients()
            ctx.set_angular_velocity(rate * ts.current_time, rate)
            ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
            ctx.set_imex_rotation(1, rate * ts.current_time, rate * ts.previous_time if step > 0 else None)
            ctx.step_imex(opts)
            ts.advance_time()
            ctx.advance(0)
        u_abi, p_abi = ctx.get_state(nat.U1), ctx.get_state(nat.P_OLD)
    finally:
        ctx.close()
    assert np.abs(u_cls).max() > 0.5
    assert np.array_equal(u_cls, u_abi) and np.array_equal(p_cls, p_abi)
