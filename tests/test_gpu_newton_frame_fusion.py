"""The frame of the Newton iteration of nsfem_step_ipcs inside the residual launch (k_jac_lattice<FORM, 7 / 8>: the
pending update u* -= dx while staging, the Dirichlet rows u* - g_D at the store, one sum of squares per tile) against
the launches it replaces (NSFEM_NEWTON_FUSED=0, read when a context is created: k_axpby, k_bc_residual_norm).

Every per-entry expression is kept, so after every step the fields and the right-hand side of the correction solve
must be EQUAL, not close, and so must every iteration count.  The Newton residual norm alone is summed in another
order (per tile, then over the tiles, instead of 512 grid-stride partitions): two sums of n non-negative squares, each
within n 2^-53 of the exact sum, differ by at most 2 n 2^-53 relative, and the square root halves that; the tests
allow 2 n 2^-53 relative on the norm with n = the number of velocity entries of their own mesh.

Every case builds two contexts on the same problem, one per switch setting, and steps them side by side with the
benchmark's throughput settings.  Sizes: the smallest on which the tile logic can go wrong (a workgroup owns 62 x 14
nodes): the 16 x 16 cavity (P2 lattice 33 x 33: three tiles in one column, the last tile row partial) and a 40 x 28
box with the binary spacing 1 / 32 (P2 81 x 57: 2 x 5 tiles, partial tiles in both directions), closed and with an
inlet profile (non-zero Dirichlet values) and a pressure outlet.

The 3D box and NSFEM_JAC_LATTICE=0 keep k_bc_residual_norm, whose loop now loads the residual entry before it looks
at the row flag: the same values in the same order, so the residual history of the 3D box must equal, bit for bit, the
one recorded from the build before that change (tests/golden/newton_frame_box3_history.npz, written by
record_box3_history below)."""
import os

import numpy as np
import pytest

import _native as nat
from gpu_common import box, context, velocity_bc
from multigrid import attach_hierarchy

pytestmark = pytest.mark.gpu

SWITCH = "NSFEM_NEWTON_FUSED"
FIELDS = (("U0", nat.U0), ("USTAR", nat.USTAR), ("P", nat.P))
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "newton_frame_box3_history.npz")
_problems = {}


def _problem(nx, ny, ext, outlet=False, lid=1.0):
    """mesh, dof map, velocity Dirichlet set, pressure Dirichlet nodes.  Closed box: the lid-driven cavity.  Outlet: a
    parabolic inlet profile on x = 0 (non-zero Dirichlet values), no-slip walls, p = 0 on the side x = ext[0]."""
    key = (nx, ny, ext, outlet, lid)
    if key not in _problems:
        mesh, dm, marks = box(nx, ny, p1=ext)
        mesh.structured = ((0.0, 0.0), ext, nx, ny)
        zero = lambda X: np.zeros((X.shape[0], 2))
        if outlet:
            inlet = lambda X: np.stack([4.0 * X[:, 1] * (ext[1] - X[:, 1]) / ext[1] ** 2, np.zeros(X.shape[0])], axis=1)
            bd, bv = velocity_bc(dm, marks, [(1, inlet), (3, zero), (4, zero)])
            nodes = np.where(np.abs(mesh.coords[:, 0] - ext[0]) < 1e-12)[0].astype(np.int32)
        else:
            top = lambda X: np.tile([lid, 0.0], (X.shape[0], 1))
            bd, bv = velocity_bc(dm, marks, [(1, zero), (2, zero), (3, zero), (4, top)])
            nodes = np.zeros(0, np.int32)
        _problems[key] = (mesh, dm, bd.astype(np.int32), bv, nodes)
    return _problems[key]


def _context(prob, fused, monkeypatch, env=None):
    import poisson_fd as pf
    mesh, dm, bd, bv, nodes = prob
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    if fused:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, "0")
    ctx = context(mesh, dm)
    monkeypatch.delenv(SWITCH, raising=False)
    for k in (env or {}):
        monkeypatch.delenv(k, raising=False)
    attach_hierarchy(ctx, mesh)
    ctx.set_coeffs(1.0, 1.0, 0.01)
    ctx.set_dirichlet(nat.VELOCITY, bd, bv)
    ctx.set_dirichlet(nat.PRESSURE, nodes, np.zeros(nodes.size))
    ctx.poisson_set_fast_diag(pf.factors(*pf.lattice_lines(mesh), nodes))
    return ctx


def _pair(prob, monkeypatch, env=None):
    return _context(prob, False, monkeypatch, env), _context(prob, True, monkeypatch, env)


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


def _exact_newton_opts(ctx):
    o = _throughput_opts(ctx)
    o.newton_forcing = 0.0
    o.momentum.rtol = 1e-12
    return o


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _counts(info):
    return (info.newton_iterations, info.krylov_iterations_momentum, info.krylov_iterations_poisson,
            info.krylov_iterations_correction, info.converged)


def _assert_fields_equal(off, on, step, slots=FIELDS, rhs=True):
    for name, slot in slots:
        a, b = off.get_state(slot), on.get_state(slot)
        assert np.array_equal(_bits(a), _bits(b)), (step, name, int((_bits(a) != _bits(b)).sum()))
    if rhs:
        a, b = off.get_rhs(nat.SYS_CORRECTION), on.get_rhs(nat.SYS_CORRECTION)
        assert np.array_equal(_bits(a), _bits(b)), (step, "rhs_v", int((_bits(a) != _bits(b)).sum()))


def _assert_equal_after_step(off, on, i_off, i_on, step, n):
    assert _counts(i_off) == _counts(i_on), (step, _counts(i_off), _counts(i_on))
    bound = 2.0 * n * 2.0 ** -53
    for k in range(i_on.newton_iterations + 1):
        a, b = i_off.newton_residuals[k], i_on.newton_residuals[k]
        print("step %d newton residual %d: off %.17e on %.17e rel diff %.3e (bound %.3e)"
              % (step, k, a, b, abs(a - b) / max(abs(a), 1e-300), bound))
        assert abs(a - b) <= bound * abs(a), (step, k, a, b)
    _assert_fields_equal(off, on, step)


def _ipcs_steps(off, on, nsteps, n, opts=_throughput_opts, dt=0.01, first=0, between=None):
    """nsteps IPCS steps (BDF-1 start, then BDF-2) on both contexts, compared after every step; returns the number of
    Newton iterations taken"""
    o_off, o_on = opts(off), opts(on)
    its = []
    for step in range(first, first + nsteps):
        alpha = (1.0, -1.0, 0.0) if step == 0 else (1.5, -2.0, 0.5)
        infos = []
        for ctx, o in ((off, o_off), (on, o_on)):
            ctx.set_bdf(alpha, dt)
            infos.append(ctx.step_ipcs(o))
        _assert_equal_after_step(off, on, infos[0], infos[1], step, n)
        its.append(infos[1].newton_iterations)
        if between is not None:
            between(step)
        off.advance(0)
        on.advance(0)
    return its


ZEROS = dict(residuals=0, updates=0)


def _assert_counters(off, on, its):
    """every residual evaluation of a step carries the frame (one more than the step's Newton iterations), every one
    but the first the update"""
    assert off.newton_frame_info() == ZEROS
    assert on.newton_frame_info() == dict(residuals=sum(its) + len(its), updates=sum(its)), (on.newton_frame_info(), its)


@pytest.mark.parametrize("nx,ny,ext,outlet", [(16, 16, (1.0, 1.0), False), (40, 28, (1.25, 0.875), False),
                                              (40, 28, (1.25, 0.875), True)])
def test_steps_equal_the_unfused_launch_sequence(nx, ny, ext, outlet, monkeypatch):
    """four steps of the cavity / the inlet-outlet box with the throughput settings"""
    prob = _problem(nx, ny, ext, outlet)
    if outlet:
        assert np.abs(prob[3]).max() == 1.0
    off, on = _pair(prob, monkeypatch)
    try:
        its = _ipcs_steps(off, on, 4, prob[1].n_velocity)
        assert sum(its) >= 4
        _assert_counters(off, on, its)
        assert on.jacobian_info()["path"] == "lattice-kernel"
    finally:
        off.close()
        on.close()


def test_exact_newton_exchanges_the_buffers_an_odd_and_an_even_number_of_times(monkeypatch):
    """Forcing 0 and Krylov rtol 1e-12 on the 40 x 28 box: a step runs three or more Newton iterations, so the two u*
    buffers change places an odd and an even number of times within and across steps; u* is read back between the steps
    (the state calls must follow the slot) and a second and third step run from there"""
    prob = _problem(40, 28, (1.25, 0.875))
    off, on = _pair(prob, monkeypatch)
    try:
        seen = []
        its = _ipcs_steps(off, on, 3, prob[1].n_velocity, opts=_exact_newton_opts,
                          between=lambda step: seen.append(on.get_state(nat.USTAR)))
        print("newton iterations per step", its)
        assert max(its) >= 3                      # (the running count of exchanges passes through both parities)
        assert not np.array_equal(seen[0], seen[1])
        _assert_counters(off, on, its)
    finally:
        off.close()
        on.close()


def test_zero_residual_at_the_start_of_a_step_runs_no_update(monkeypatch):
    """all-zero state and zero boundary values: the first residual is 0, no iteration, no update launch, u* untouched"""
    prob = _problem(16, 16, (1.0, 1.0), lid=0.0)
    assert np.abs(prob[3]).max() == 0.0
    off, on = _pair(prob, monkeypatch)
    try:
        infos = []
        for ctx in (off, on):
            ctx.set_bdf((1.0, -1.0, 0.0), 0.01)
            infos.append(ctx.step_ipcs(_throughput_opts(ctx)))
        for info in infos:
            assert info.newton_iterations == 0 and info.newton_residuals[0] == 0.0 and info.converged
        assert on.newton_frame_info() == dict(residuals=1, updates=0)
        assert off.newton_frame_info() == ZEROS
        assert not on.get_state(nat.USTAR).any()
        _assert_fields_equal(off, on, 0)
    finally:
        off.close()
        on.close()


def test_dirichlet_values_set_again_between_steps_reach_the_residual_rows(monkeypatch):
    """nsfem_set_dirichlet with scaled lid values between the steps: the dense value vector the residual launch reads
    must follow (the dof set stays, only the values move)"""
    prob = _problem(16, 16, (1.0, 1.0))
    n = prob[1].n_velocity
    off, on = _pair(prob, monkeypatch)
    try:
        its = _ipcs_steps(off, on, 2, n)
        for ctx in (off, on):
            ctx.set_dirichlet(nat.VELOCITY, prob[2], 1.5 * prob[3])
        its += _ipcs_steps(off, on, 2, n, first=2)
        u = on.get_state(nat.U0)
        assert np.array_equal(u[prob[2]], 1.5 * prob[3])
        _assert_counters(off, on, its)
    finally:
        off.close()
        on.close()


def test_one_newton_iteration_and_an_unreachable_tolerance_fail_alike(monkeypatch):
    """newton_max_iter = 1 with tolerances the step cannot meet: both contexts raise the same error after the residual
    that follows the only update, and leave the same u* bits behind the slot"""
    prob = _problem(16, 16, (1.0, 1.0))
    off, on = _pair(prob, monkeypatch)
    try:
        errs = []
        for ctx in (off, on):
            o = _throughput_opts(ctx)
            o.newton_max_iter = 1
            o.newton_atol = 1e-300
            o.newton_rtol = 1e-300
            ctx.set_bdf((1.0, -1.0, 0.0), 0.01)
            with pytest.raises(nat.NativeError) as e:
                ctx.step_ipcs(o)
            errs.append((e.value.code, str(e.value)))
        assert errs[0] == errs[1], errs
        assert "Newton solver did not converge" in errs[1][1]
        assert on.newton_frame_info() == dict(residuals=2, updates=1)
        _assert_fields_equal(off, on, 0, slots=(("USTAR", nat.USTAR),), rhs=False)
        assert on.get_state(nat.USTAR).any()
    finally:
        off.close()
        on.close()


def test_the_launch_pair_path_keeps_its_launches(monkeypatch):
    """NSFEM_JAC_LATTICE=0: no one-launch residual, so no frame: the counters stay 0 and everything, the Newton
    residual norms included (k_bc_residual_norm on both sides), equals the switch-off context bit for bit"""
    prob = _problem(16, 16, (1.0, 1.0))
    off, on = _pair(prob, monkeypatch, env={"NSFEM_JAC_LATTICE": "0"})
    try:
        assert on.jacobian_info()["path"] != "lattice-kernel"
        o_off, o_on = _throughput_opts(off), _throughput_opts(on)
        for step in range(3):
            infos = []
            for ctx, o in ((off, o_off), (on, o_on)):
                ctx.set_bdf((1.0, -1.0, 0.0) if step == 0 else (1.5, -2.0, 0.5), 0.01)
                infos.append(ctx.step_ipcs(o))
            assert _counts(infos[0]) == _counts(infos[1])
            assert np.array_equal(_bits(np.array(infos[0].newton_residuals[:])), _bits(np.array(infos[1].newton_residuals[:])))
            _assert_fields_equal(off, on, step)
            off.advance(0)
            on.advance(0)
        assert off.newton_frame_info() == ZEROS and on.newton_frame_info() == ZEROS
    finally:
        off.close()
        on.close()


def _box3_steps():
    """two IPCS steps of the lid-driven cavity on a 6 x 5 x 4 Kuhn box (P2 13 x 11 x 9 nodes, 3,861 velocity entries),
    Jacobi-preconditioned solves; returns (Newton residual histories as bit patterns, Newton counts, U0, P)"""
    from fem_mesh import FacetMarkers, TaylorHoodDofMap, box_mesh
    p1 = (1.0, 0.75, 0.5)
    mesh = box_mesh((0.0, 0.0, 0.0), p1, 6, 5, 4)
    dm = TaylorHoodDofMap(mesh)
    marks = FacetMarkers(mesh)
    for axis in range(3):
        marks.mark(lambda X, a=axis: np.abs(X[:, a]) < 1e-12, 2 * axis + 1)
        marks.mark(lambda X, a=axis: np.abs(X[:, a] - p1[a]) < 1e-12, 2 * axis + 2)
    last = {}
    for mid in (1, 2, 3, 4, 5, 6):
        nodes = np.unique(dm.facet_p2_nodes(marks.facets_with_id(mid)))
        for a in range(3):
            last.update(zip((3 * nodes + a).tolist(), [1.0 if (mid == 6 and a == 0) else 0.0] * nodes.size))
    bd = np.array(sorted(last), dtype=np.int32)
    bv = np.array([last[i] for i in bd.tolist()])
    ctx = nat.NsfemContext(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, dm.n_p2, dm.n_p1)
    try:
        ctx.set_coeffs(1.0, 1.0, 0.02)
        ctx.set_dirichlet(nat.VELOCITY, bd, bv)
        ctx.set_dirichlet(nat.PRESSURE, np.zeros(0, np.int32), np.zeros(0))
        o = ctx.default_step_opts()
        for k in (o.momentum, o.poisson, o.correction):
            k.rtol = 1e-10
        hist, its = [], []
        for step in range(2):
            ctx.set_bdf((1.0, -1.0, 0.0) if step == 0 else (1.5, -2.0, 0.5), 0.05)
            info = ctx.step_ipcs(o)
            its.append(info.newton_iterations)
            hist.extend(info.newton_residuals[k] for k in range(info.newton_iterations + 1))
            ctx.advance(0)
        frame = ctx.newton_frame_info() if hasattr(ctx, "newton_frame_info") else ZEROS
        return _bits(np.array(hist)), np.array(its), ctx.get_state(nat.U1), ctx.get_state(nat.P_OLD), frame
    finally:
        ctx.close()


def record_box3_history(path=GOLDEN):
    """writes the stored history; run with the build whose k_bc_residual_norm is the reference"""
    hist, its, _, _, _ = _box3_steps()
    np.savez(path, history_bits=hist, newton_iterations=its)


def test_3d_box_keeps_its_launches_and_the_recorded_residual_history(monkeypatch):
    """3D: no lattice kernel, counters 0, both switch settings equal, and the Newton residual history equals the one
    recorded before k_bc_residual_norm's loop was rewritten, bit for bit"""
    runs = []
    for env in ("0", None):
        if env is None:
            monkeypatch.delenv(SWITCH, raising=False)
        else:
            monkeypatch.setenv(SWITCH, env)
        runs.append(_box3_steps())
    monkeypatch.delenv(SWITCH, raising=False)
    off, on = runs
    assert off[4] == ZEROS and on[4] == ZEROS
    assert np.array_equal(off[0], on[0]) and np.array_equal(off[1], on[1])
    assert np.array_equal(_bits(off[2]), _bits(on[2])) and np.array_equal(_bits(off[3]), _bits(on[3]))
    gold = np.load(GOLDEN)
    assert np.array_equal(gold["newton_iterations"], on[1]), (gold["newton_iterations"], on[1])
    assert on[0].size >= 4
    assert np.array_equal(gold["history_bits"], on[0]), (gold["history_bits"].view(np.float64), on[0].view(np.float64))
