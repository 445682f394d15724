"""The fused step frame (k_spmv_dict_pair, k_correction_finish, k_sub_mean_dot, the projection check that also stores
p = p_old + z) against the launch sequence it replaces (NSFEM_STEP_FUSED=0, read when a context is created).  The fused
launches keep every per-entry expression and every reduction partition, so after every step the fields, the
right-hand side of the correction solve and every field of the step record must be EQUAL, not close.

Every case builds two contexts on the same problem, one per switch setting, and steps them side by side.  Sizes: the
smallest with a stencil dictionary (a level needs 1,024 rows): the 16 x 16 cavity (P2 lattice 33 x 33 = 1,089 rows:
five workgroups, the last with 65 live rows, Dirichlet rows on all four sides), a 24 x 16 box on [0, 2] x [0, 1]
(width and height differ, and so do the row strides of the two dictionaries) and a 40 x 28 box (P2 81 x 57, P1
41 x 29 = 1,189 rows: the smallest here whose PRESSURE operator has a dictionary, so the only one on which the
projection check can store p = p_old + z; on the smaller ones that counter stays 0 and k_sub_mean_dot alone runs).

The fused launches replace dictionary launches only, and a product outside a smoother runs on a dictionary only when
the dictionary equals the matrix bit for bit, which needs a binary mesh spacing.  The 24 x 16 box on [0, 2] x [0, 1]
has the spacing 1 / 12 in x: its dictionaries are not bit-exact on the MI355X build (every counter reads 0 there:
the fallbacks run, fields still equal), so on that box every counter may be 0 or the full count, and the same
24 x 16 lattice on [0, 1.5] x [0, 1] (spacing 1 / 16) is run beside it with the full counts required.
Settings of the steps: the benchmark's throughput settings (fast-diagonalisation projection, Chebyshev mass solve,
Krylov rtol 1e-8, inexact Newton with forcing 1e-4, extrapolated pressure start)."""
import numpy as np
import pytest

import _native as nat
from gpu_common import box, context, velocity_bc
from multigrid import attach_hierarchy

pytestmark = pytest.mark.gpu

SWITCH = "NSFEM_STEP_FUSED"
FIELDS = (("U0", nat.U0), ("USTAR", nat.USTAR), ("P", nat.P))
_problems = {}


def _problem(nx, ny, ext, outlet=False):
    """mesh, dof map, velocity Dirichlet set, pressure Dirichlet nodes.  Closed box: the lid-driven cavity.  Outlet: a
    parabolic inlet profile on x = 0 (non-zero Dirichlet values), no-slip walls, p = 0 on the side x = ext[0]."""
    key = (nx, ny, ext, outlet)
    if key not in _problems:
        mesh, dm, marks = box(nx, ny, p1=ext)
        mesh.structured = ((0.0, 0.0), ext, nx, ny)
        zero = lambda X: np.zeros((X.shape[0], 2))
        if outlet:
            inlet = lambda X: np.stack([4.0 * X[:, 1] * (ext[1] - X[:, 1]) / ext[1] ** 2, np.zeros(X.shape[0])], axis=1)
            bd, bv = velocity_bc(dm, marks, [(1, inlet), (3, zero), (4, zero)])
            nodes = np.where(np.abs(mesh.coords[:, 0] - ext[0]) < 1e-12)[0].astype(np.int32)
        else:
            lid = lambda X: np.tile([1.0, 0.0], (X.shape[0], 1))
            bd, bv = velocity_bc(dm, marks, [(1, zero), (2, zero), (3, zero), (4, lid)])
            nodes = np.zeros(0, np.int32)
        _problems[key] = (mesh, dm, bd.astype(np.int32), bv, nodes)
    return _problems[key]


def _context(prob, fused, monkeypatch, body_force=None):
    import poisson_fd as pf
    mesh, dm, bd, bv, nodes = prob
    if fused:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, "0")
    ctx = context(mesh, dm)
    monkeypatch.delenv(SWITCH, raising=False)
    attach_hierarchy(ctx, mesh)
    ctx.set_coeffs(1.0, 1.0, 0.01, None if body_force is None else 1.0)
    ctx.set_dirichlet(nat.VELOCITY, bd, bv)
    ctx.set_dirichlet(nat.PRESSURE, nodes, np.zeros(nodes.size))
    ctx.poisson_set_fast_diag(pf.factors(*pf.lattice_lines(mesh), nodes))
    if body_force is not None:
        ctx.set_state(nat.BODY_FORCE, body_force)
    return ctx


def _throughput_opts(ctx):
    o = ctx.default_step_opts()
    for k in (o.momentum, o.poisson, o.correction):
        k.rtol = 1e-8
    o.momentum.precond = 1
    o.poisson.precond = 3
    o.correction.precond = 2
    o.newton_forcing = 1e-4
    o.pressure_extrapolation = 1
    return o


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _record(info):
    return (info.newton_iterations, info.krylov_iterations_momentum, info.krylov_iterations_poisson,
            info.krylov_iterations_correction, tuple(_bits(np.array(info.newton_residuals[:])).tolist()),
            info.converged, info.reserved)


def _assert_equal_after_step(off, on, i_off, i_on, step):
    assert _record(i_off) == _record(i_on), (step, _record(i_off), _record(i_on))
    for name, slot in FIELDS:
        a, b = off.get_state(slot), on.get_state(slot)
        assert np.array_equal(_bits(a), _bits(b)), (step, name, int((_bits(a) != _bits(b)).sum()))
    a, b = off.get_rhs(nat.SYS_CORRECTION), on.get_rhs(nat.SYS_CORRECTION)
    assert np.array_equal(_bits(a), _bits(b)), (step, "rhs_v", int((_bits(a) != _bits(b)).sum()))


def _ipcs_steps(off, on, nsteps, dt=0.01):
    """nsteps IPCS steps (BDF-1 start, then BDF-2) on both contexts, compared after every step"""
    o_off, o_on = _throughput_opts(off), _throughput_opts(on)
    for step in range(nsteps):
        alpha = (1.0, -1.0, 0.0) if step == 0 else (1.5, -2.0, 0.5)
        infos = []
        for ctx, o in ((off, o_off), (on, o_on)):
            ctx.set_bdf(alpha, dt)
            infos.append(ctx.step_ipcs(o))
        _assert_equal_after_step(off, on, infos[0], infos[1], step)
        assert infos[1].krylov_iterations_correction >= 1
        off.advance(0)
        on.advance(0)


def _pair(prob, monkeypatch, **kw):
    return _context(prob, False, monkeypatch, **kw), _context(prob, True, monkeypatch, **kw)


ZEROS = dict(pair_begin=0, pair_correction=0, correction_finish=0, projection_sum=0)
BINARY = {(1.0, 1.0), (1.5, 1.0), (1.25, 0.875)}           # extents that give the lattices here a binary spacing


def _assert_counters(prob, ext, f, nsteps, begin=True, projection=True):
    """begin step and projection check fused in every step, the correction pair and finish in every step but the
    first ones (no predicted step count yet); the projection epilogue needs a pressure dictionary (1,024 rows)"""
    print("step frame launches", ext, f)
    want_p = nsteps if (projection and prob[1].n_p1 >= 1024) else 0
    want_b = nsteps if begin else 0
    if ext in BINARY:
        assert f["pair_begin"] == want_b and f["projection_sum"] == want_p
        assert 1 <= f["pair_correction"] < nsteps
    else:
        assert f["pair_begin"] in (0, want_b) and f["projection_sum"] in (0, want_p)
        assert f["pair_correction"] < nsteps
    assert f["correction_finish"] == f["pair_correction"]


@pytest.mark.parametrize("nx,ny,ext", [(16, 16, (1.0, 1.0)), (24, 16, (2.0, 1.0)), (24, 16, (1.5, 1.0)),
                                       (40, 28, (1.25, 0.875))])
def test_closed_box_steps_equal_the_unfused_launch_sequence(nx, ny, ext, monkeypatch):
    """six steps: the first correction solves have no predicted step count (start sums read before the sequence: the
    present launches), the later ones end in k_correction_finish; every begin step and every projection check runs
    fused"""
    off, on = _pair(_problem(nx, ny, ext), monkeypatch)
    try:
        _ipcs_steps(off, on, 6)
        assert off.step_frame_info() == ZEROS
        _assert_counters(_problem(nx, ny, ext), ext, on.step_frame_info(), 6)
    finally:
        off.close()
        on.close()


@pytest.mark.parametrize("ext", [(2.0, 1.0), (1.5, 1.0)])
def test_pressure_outlet_steps_equal_the_unfused_launch_sequence(ext, monkeypatch):
    """24 x 16 box with a pressure Dirichlet side: poisson_direct_step is not taken (the projection counter stays 0),
    the begin-step and correction fusions still run, and the start vector of the correction solve carries a non-zero
    inlet profile on its Dirichlet rows"""
    prob = _problem(24, 16, ext, outlet=True)
    assert np.abs(prob[3]).max() == 1.0
    off, on = _pair(prob, monkeypatch)
    try:
        _ipcs_steps(off, on, 6)
        assert off.step_frame_info() == ZEROS
        _assert_counters(prob, ext, on.step_frame_info(), 6, projection=False)
    finally:
        off.close()
        on.close()


def test_body_force_keeps_the_begin_step_launches(monkeypatch):
    """16 x 16 cavity with a body force: the begin step falls back (counter 0), the fields are still equal"""
    prob = _problem(16, 16, (1.0, 1.0))
    X = prob[1].p2_coords
    f = np.stack([np.sin(np.pi * X[:, 1]), -np.cos(np.pi * X[:, 0])], axis=1).ravel()
    off, on = _pair(prob, monkeypatch, body_force=f)
    try:
        _ipcs_steps(off, on, 4)
        assert off.step_frame_info() == ZEROS
        _assert_counters(prob, (1.0, 1.0), on.step_frame_info(), 4, begin=False)
    finally:
        off.close()
        on.close()


def test_imex_steps_equal_the_unfused_launch_sequence(monkeypatch):
    """nsfem_step_imex shares the projection and correction steps: three SBDF2-type steps on the 16 x 16 cavity"""
    off, on = _pair(_problem(16, 16, (1.0, 1.0)), monkeypatch)
    try:
        o_off, o_on = _throughput_opts(off), _throughput_opts(on)
        for step in range(3):
            coef = ((1.0, -1.0, 0.0), (1.0, 0.0), (1.0, 0.0, 0.0)) if step == 0 else \
                ((1.5, -2.0, 0.5), (2.0, -1.0), (1.0, 0.0, 0.0))
            infos = []
            for ctx, o in ((off, o_off), (on, o_on)):
                ctx.set_imex(*coef, 0.01)
                infos.append(ctx.step_imex(o))
            _assert_equal_after_step(off, on, infos[0], infos[1], step)
            off.advance(0)
            on.advance(0)
        assert off.step_frame_info() == ZEROS
        _assert_counters(_problem(16, 16, (1.0, 1.0)), (1.0, 1.0), on.step_frame_info(), 3, begin=False)
    finally:
        off.close()
        on.close()


@pytest.mark.parametrize("nx,ny,ext", [(16, 16, (1.0, 1.0)), (40, 28, (1.25, 0.875))])
def test_pair_kernel_begin_step_on_random_vectors(nx, ny, ext, monkeypatch):
    """No product hook reaches the pair kernel, so gconst = M (a1 u1 + a2 u2) / k - c_p D^T p_old is compared through
    the first Newton residual (nsfem_assemble of the momentum system with the new-step flag, nsfem_get_rhs), which
    adds it entry by entry: random u1, u2, u*, p_old from a fixed seed, both switch settings, bit for bit"""
    prob = _problem(nx, ny, ext)
    dm = prob[1]
    rng = np.random.default_rng(1000 * nx + ny)
    vecs = {nat.U1: rng.standard_normal(dm.n_velocity), nat.U2: rng.standard_normal(dm.n_velocity),
            nat.USTAR: rng.standard_normal(dm.n_velocity), nat.P_OLD: rng.standard_normal(dm.n_p1)}
    off, on = _pair(prob, monkeypatch)
    try:
        rhs = []
        for ctx in (off, on):
            for slot, v in vecs.items():
                ctx.set_state(slot, v)
            ctx.set_bdf((1.5, -2.0, 0.5), 0.01)
            ctx.assemble(nat.SYS_MOMENTUM, new_step=True)
            rhs.append(ctx.get_rhs(nat.SYS_MOMENTUM))
        assert np.array_equal(_bits(rhs[0]), _bits(rhs[1])), int((_bits(rhs[0]) != _bits(rhs[1])).sum())
        assert np.abs(rhs[1]).max() > 1.0
        assert off.step_frame_info() == ZEROS
        assert on.step_frame_info() == dict(ZEROS, pair_begin=1)
    finally:
        off.close()
        on.close()
