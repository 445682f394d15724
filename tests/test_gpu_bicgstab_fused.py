"""BiCGStab without start kernel and with the update fused to the next direction, against the launch sequence it
replaces (NSFEM_BICG_FUSED=0, read when a context is created): the new path keeps every per-entry expression and every
reduction partition (512 blocks of 256 threads, grid-stride accumulation), so fields, iteration counts, solve
residuals and Newton residual histories must be EQUAL, not close.

Sizes: the 2D cavity at n = 8 (578 velocity entries: most of the 512 blocks own nothing) and n = 192 (296,450
entries: more than the 131,072 threads of a launch, so the grid-stride loops trip more than once, the last trip
ragged).  Settings of the steps: the benchmark's throughput settings (Krylov rtol 1e-8, inexact Newton with forcing
1e-4, V-cycle preconditioned momentum and projection solves, Chebyshev mass solve)."""
import os
import threading

import numpy as np
import pytest

import _native as nat
from gpu_common import box, cavity_bc, context
from multigrid import attach_hierarchy

pytestmark = pytest.mark.gpu

SWITCH = "NSFEM_BICG_FUSED"
_meshes = {}


def _cavity(n):
    if n not in _meshes:
        mesh, dm, marks = box(n, n)
        mesh.structured = ((0.0, 0.0), (1.0, 1.0), n, n)
        bd, bv = cavity_bc(dm, marks)
        _meshes[n] = (mesh, dm, bd.astype(np.int32), bv)
    return _meshes[n]


def _throughput_opts(ctx, precond=1):
    opts = ctx.default_step_opts()
    for o in (opts.momentum, opts.poisson, opts.correction):
        o.rtol = 1e-8
    opts.momentum.precond = precond
    opts.poisson.precond = 1
    opts.correction.precond = 2
    opts.newton_forcing = 1e-4
    return opts


def _steps(ctx, opts, nsteps):
    hist = []
    for step in range(nsteps):
        ctx.set_bdf((1.0, -1.0, 0.0) if step == 0 else (1.5, -2.0, 0.5), 0.01)
        info = ctx.step_ipcs(opts)
        ctx.advance(0)
        hist.append((info.newton_iterations, info.krylov_iterations_momentum, info.krylov_iterations_poisson,
                     tuple(info.newton_residuals[k] for k in range(info.newton_iterations + 1))))
    return ctx.get_state(nat.U1), ctx.get_state(nat.P_OLD), hist


def _both(monkeypatch, run):
    out = []
    for env in ("0", None):
        if env is None:
            monkeypatch.delenv(SWITCH, raising=False)
        else:
            monkeypatch.setenv(SWITCH, env)
        out.append(run())
    return out


def _assert_same_steps(a, b):
    assert a[2] == b[2], (a[2], b[2])              # Newton / Krylov counts and the Newton residual history
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


def _run_cavity(n, tune, nsteps=3, precond=1):
    mesh, dm, bd, bv = _cavity(n)
    ctx = context(mesh, dm)
    attach_hierarchy(ctx, mesh, coarsest=4)
    ctx.set_coeffs(1.0, 1.0, 0.01)
    ctx.set_dirichlet(nat.VELOCITY, bd, bv)
    ctx.set_dirichlet(nat.PRESSURE, np.zeros(0, np.int32), np.zeros(0))
    opts = _throughput_opts(ctx, precond)
    tune(opts)
    res = _steps(ctx, opts, nsteps)
    ctx.close()
    return res


def _every_iteration_checked(opts):
    # (first_check is a floor: the predictor taken from the previous solve may postpone the first check of a later
    # solve, which then runs a fused update -- the first solves of every Newton slot check every iteration)
    opts.momentum.first_check = 1


def _fused_tail(opts):
    opts.momentum.first_check = 3
    opts.momentum.max_iter = 50


def _confirming(opts):
    opts.momentum.rtol = 1e-12
    opts.newton_forcing = 0.0


@pytest.mark.parametrize("n", [8, 192])
@pytest.mark.parametrize("case", ["checked", "tail", "confirm"])
def test_ipcs_steps_equal_the_unfused_launch_sequence(n, case, monkeypatch):
    """checked: every iteration is followed by a check until the predictor of the previous solve postpones it (start
    without start kernel, plain update + separate direction kernel after checked iterations).
    tail: first_check = 3, max_iter 50: iterations 1 and 2 of every solve end in the fused update.  The first solve of
    the first step starts from the zero state: its residual lives on the Dirichlet rows only (u* - g), every later
    residual vanishes there, rho = rhat.r = 0 after iteration 1 -- the in-kernel restart (rhat = r) runs inside the
    fused update, with rhat aliased to the right-hand side (the step driver gives it up).
    confirm: momentum.rtol = 1e-12, exact Newton: the solves confirm the true residual b - A x, so rhat is copied and
    b stays intact."""
    tune = {"checked": _every_iteration_checked, "tail": _fused_tail, "confirm": _confirming}[case]
    off, on = _both(monkeypatch, lambda: _run_cavity(n, tune))
    _assert_same_steps(off, on)
    assert sum(h[1] for h in on[2]) >= 3           # the solves did iterate


def test_jacobi_preconditioned_steps_equal_the_unfused_launch_sequence(monkeypatch):
    """precond = 0 at n = 8: phat = dinv * b / dinv * p formed by the first-direction kernel and inside the fused
    update (first_check = 3: fused tails; Jacobi needs tens of iterations, so the plain tail and the separate
    direction kernel after checked iterations run as well)"""
    off, on = _both(monkeypatch, lambda: _run_cavity(8, _fused_tail, precond=0))
    _assert_same_steps(off, on)
    assert sum(h[1] for h in on[2]) > 12


@pytest.mark.parametrize("n,precond", [(8, 0), (8, 1), (192, 0), (192, 1)])
def test_solve_from_a_dirichlet_row_residual_through_the_explicit_seam(n, precond, monkeypatch):
    """The restart case through nsfem_assemble / nsfem_solve (no driver gives the right-hand side up there: rhat is a
    copy).  State zero, lid velocity 1: the assembled momentum residual is u* - g on the Dirichlet rows and zero
    elsewhere, the case the comment above k_bicg_p describes; every iteration is checked, so the restart decision is
    taken by k_bicg_p with the previous direction still lying in b.  Equal: the update (u* after the solve),
    iterations, residual0, residual; and b is intact after the solve.  (Jacobi, precond = 0, is sure to need the second
    iteration in which the decision falls; the V-cycle may converge in one.)"""
    mesh, dm, bd, bv = _cavity(n)

    def run():
        ctx = context(mesh, dm)
        attach_hierarchy(ctx, mesh, coarsest=4)
        ctx.set_coeffs(1.0, 1.0, 0.01)
        ctx.set_bdf((1.0, -1.0, 0.0), 0.01)
        ctx.set_dirichlet(nat.VELOCITY, bd, bv)
        ctx.assemble(nat.SYS_MOMENTUM, new_step=True)
        b = ctx.get_rhs(nat.SYS_MOMENTUM)
        free = np.ones(b.size, bool)
        free[bd] = False
        assert np.abs(b[free]).max() == 0.0 and np.abs(b[bd]).max() == 1.0
        info = ctx.solve(nat.SYS_MOMENTUM, rtol=1e-8, precond=precond)
        assert np.array_equal(ctx.get_rhs(nat.SYS_MOMENTUM), b)
        res = (ctx.get_state(nat.USTAR), (info.iterations, info.residual0, info.residual))
        ctx.close()
        return res

    off, on = _both(monkeypatch, run)
    assert off[1] == on[1], (off[1], on[1])
    assert precond == 1 or on[1][0] >= 2               # (a second iteration: the restart decision was taken)
    assert np.array_equal(off[0], on[0])


def test_3d_cavity_steps_equal_the_unfused_launch_sequence(monkeypatch):
    """the lid-driven box with 4 cells a side, 2 steps: the same kernels on three interleaved components"""
    from fem_mesh import TaylorHoodDofMap, box_mesh
    n = 4
    mesh = box_mesh((0, 0, 0), (1, 1, 1), n, n, n)
    mesh.structured = ((0.0,) * 3, (1.0,) * 3) + (n,) * 3
    dm = TaylorHoodDofMap(mesh)
    X = dm.p2_coords
    on_b = np.zeros(dm.n_p2, bool)
    for a in range(3):
        on_b |= (np.abs(X[:, a]) < 1e-12) | (np.abs(X[:, a] - 1.0) < 1e-12)
    nodes = np.nonzero(on_b)[0]
    lid = np.abs(X[nodes, 2] - 1.0) < 1e-12
    dofs = np.concatenate([3 * nodes + a for a in range(3)]).astype(np.int32)
    vals = np.concatenate([np.where(lid, 1.0, 0.0)] + [np.zeros(nodes.size)] * 2)

    def run():
        ctx = context(mesh, dm)
        attach_hierarchy(ctx, mesh, coarsest=2)
        ctx.set_coeffs(1.0, 1.0, 0.01)
        ctx.set_dirichlet(nat.VELOCITY, dofs, vals)
        ctx.set_dirichlet(nat.PRESSURE, np.zeros(0, np.int32), np.zeros(0))
        opts = _throughput_opts(ctx)
        _fused_tail(opts)
        res = _steps(ctx, opts, 2)
        ctx.close()
        return res

    off, on = _both(monkeypatch, run)
    _assert_same_steps(off, on)


def test_two_thread_ranks_equal_the_unfused_launch_sequence(monkeypatch):
    """16 x 16 cells in two strips, 2 steps: partitioned solves keep the start kernel (their host reads the start
    sums after the start-up all-reduce) and take the fused update; fields equal, no more exchanges or all-reduces"""
    from partition import StripPartition
    n, size = 16, 2

    def run():
        group = nat.local_group_create(size)
        parts = [StripPartition((0.0, 0.0), (1.0, 1.0), n, n, r, size, coarsest=2) for r in range(size)]
        ctxs = []
        for r, part in enumerate(parts):
            pdm = part.dofmap
            c = nat.NsfemContext(part.mesh.coords, part.mesh.cells, pdm.p2_dofmap, pdm.p1_dofmap, pdm.n_p2, pdm.n_p1)
            c.attach_local_comm(group, r)
            ctxs.append(c)
        out, errors = {}, []

        def worker(r):
            try:
                part, ctx = parts[r], ctxs[r]
                part.attach(ctx)
                pdm = part.dofmap
                X = pdm.p2_coords
                on_b = (np.abs(X[:, 0]) < 1e-12) | (np.abs(X[:, 0] - 1) < 1e-12) | (np.abs(X[:, 1]) < 1e-12) | \
                    (np.abs(X[:, 1] - 1) < 1e-12)
                nodes = np.nonzero(on_b)[0]
                lid = np.abs(X[nodes, 1] - 1) < 1e-12
                ctx.set_coeffs(1.0, 1.0, 0.01)
                ctx.set_dirichlet(nat.VELOCITY, np.concatenate([2 * nodes, 2 * nodes + 1]).astype(np.int32),
                                  np.concatenate([np.where(lid, 1.0, 0.0), np.zeros(nodes.size)]))
                ctx.set_dirichlet(nat.PRESSURE, np.zeros(0, np.int32), np.zeros(0))
                opts = _throughput_opts(ctx)
                _fused_tail(opts)
                out[r] = _steps(ctx, opts, 2) + (ctx.comm_stats(),)
            except BaseException as exc:                     # a dead rank would deadlock the others
                errors.append((r, repr(exc)))
                os._exit(17)

        threads = [threading.Thread(target=worker, args=(r,)) for r in range(size)]
        for t in threads:
            t.start()
        for t in threads:
            t.join()
        assert not errors
        for c in ctxs:
            c.close()
        return out

    off, on = _both(monkeypatch, run)
    for r in range(size):
        _assert_same_steps(off[r], on[r])
        assert on[r][3]["exchanges"] <= off[r][3]["exchanges"]
        assert on[r][3]["allreduce_calls"] <= off[r][3]["allreduce_calls"]
