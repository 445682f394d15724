"""The Krylov solvers of csrc/linalg.hip -- bicgstab, pcg, pcg_single_reduction -- held to the host restatement
tests/krylov_host.py iterate by iterate: iterate k of the device against iterate k of the host, not converged fields.

How iterate k is observed (nsfem_assemble / nsfem_get_rhs / nsfem_solve and operator_csr only).  CG writes into the
state slot in place: a solve with max_iter = k, rtol = 1e-30, atol = 0 ends with ERR_NOT_CONVERGED and leaves x_k in
U0 (correction) resp. P (projection); the start vector is read back after the assembly.  BiCGStab hands its update
to u* only when it converges, so the solve is made to converge exactly at iteration k: rtol = 1e-9 (above kConfirmRtol:
no confirmation pass), max_iter = k and atol inside the window of the host residual history -- the geometric mean of
max(res_k, 1e-9 |b|) and the smallest residual a check sees before k; schedules whose only check is at k take twice the
lower end.  x_k = u*_before - u*_after; the rounding of that observation, eps / 2 (|u*| / |x_k| + 1) <= 1e-15
(asserted), is a tenth of the tolerance's floor.  The host runs on what the device exports: the Jacobian / mass / stiffness matrix through
operator_csr with the row mask applied on the host, the right-hand side through get_rhs, Jacobi from the exported
diagonal, the V-cycles from tests/mg_cycle_host.py (oracle matrices).

Problems: box8 (8 x 8 cavity, 578 velocity / 81 pressure entries: most of the 512 reduction blocks own nothing),
box128 (128 x 128, 132,098 velocity entries: 131,072 threads and a ragged second grid-stride trip of 1,026), cube4
(lid-driven box, 4 cells a side, 2,187 entries in three interleaved components).  States: `rest` (zero state, lid 1:
the residual lives on the Dirichlet rows, rho = 0 after iteration 1, the restart in iteration 2 is deterministic) and
`developed` (a smooth field in U1, U2, u*, nu = 0.01, BDF2: the Jacobian is nonsymmetric, Jacobi BiCGStab needs more
than six iterations).

BiCGStab cases: precond 0 and 1 (the default velocity cycle), k = 1 .. 6, schedules (first_check, check_every) =
(0, 1), (k, 1), (0, 2), (2, 3) with max_iter = k -- z0 with and without a check after it, p_in_b, fused tails, the
plain update before a check --, NSFEM_BICG_FUSED unset and 0.  Across schedules and the switch x_k is bitwise equal.
In the rest state the host restarts in iteration 2 (asserted in both precisions); the device reaches that decision
in k_bicg_p on schedule (0, 1) and with the switch at 0, and inside the fused update k_bicg_xr<true> on (k, 1) and
(2, 3) for k >= 2 -- without it alpha_2 = rho / rhat.v = 0 and x_2 = x_1, which the comparison with the host rejects.
A k is dropped from a schedule only where the atol window is narrower than a factor 4 or the host residual is below
1e-10 |b|; every (problem, state, preconditioner, schedule) keeps three values of k, one of them >= 3 (asserted).

Tolerance (as tests/test_gpu_multigrid_cycle.py): d = rel(x_k float64 host, x_k longdouble host) per case and
iteration (CG: of the increments x_k - x_0), the device is held to rel(x_k device, x_k float64 host) <= max(64 d, 1e-14)
and 64 d < 1e-10 is asserted.  Residuals: CG -- the same rule on |res_device - res_host| / res_host with d the larger of
the iterate's d and d_res = |res float64 host - res longdouble host| / res (the recurrence r -= alpha s carries the
round-off of |r_0| into a residual that has fallen by orders of magnitude: on box8 neumann precond 1, k = 5, the
float64 HOST differs from the longdouble host by 2.8e-12 where the iterate's d is 1.1e-15); BiCGStab -- the
recurrence |r|^2 = s.s - 2 omega t.s + omega^2 t.t cancels, so |res_device^2 - res_host^2| <= 4 tau C with C = s.s +
2 |omega| sqrt(s.s t.t) + omega^2 t.t of the host's own sums and tau = max(64 max(d, d_sums), 1e-14), d_sums the
relative float64 / longdouble difference of the three sums (4: every term is quadratic in the perturbed vectors, and
omega is perturbed too).

Step sizes (host alone, so that the rule above leaves three k everywhere): box8 0.01, box128 1e-4, cube4 0.01
(developed) and 0.2 (rest) -- Jacobi BiCGStab is at 1.5e-5 .. 7e-5 |b| after six iterations of the developed states.

Measured on the host (d: smallest .. largest over k = 1 .. 6; the last bits vary with the exported matrices), the kept
k per schedule (0,1) / (k,1) / (0,2) / (2,3), and the largest device deviation seen on the MI355X:

    BiCGStab case               d                    kept k                                   device
    box8 rest precond 0         1.2e-17 .. 3.7e-17   1-6 / 1-6 / 1-6 / 1-6                    1.7e-17
    box8 rest precond 1         2.5e-17 .. 3.8e-17   1-3 on every schedule (res_4 < 1e-10 |b|) 9.4e-17
    box8 developed precond 0    6.0e-17 .. 1.3e-16   1-5 / 1-6 / 1-5 / 1-6                    1.4e-16
    box8 developed precond 1    7.2e-17 .. 1.3e-16   1-5 / 1-6 / 1-6 / 1-6                    1.4e-16
    box128 rest precond 0       1.2e-17 .. 5.4e-17   1-6 / 1-6 / 1-6 / 1-6                    4.6e-17
    box128 rest precond 1       2.0e-17 .. 2.4e-17   1-3 on every schedule (res_4 < 1e-10 |b|) 7.6e-17
    box128 developed precond 0  1.2e-16 .. 1.8e-16   1-6 / 1-6 / 1-6 / 1-6                    3.4e-16
    box128 developed precond 1  9.9e-17 .. 1.3e-16   1-3 on every schedule (res_4 < 1e-10 |b|) 3.0e-16
    cube4 rest precond 0        4.4e-18 .. 2.2e-17   1,2,3,6 / 1-6 / 1,2,3,4,6 / 1,2,3,5,6    2.6e-17
    cube4 rest precond 1        1.2e-17 .. 1.2e-17   1-4 on every schedule (res_5 < 1e-10 |b|) 2.3e-17
    cube4 developed precond 0   1.1e-16 .. 4.3e-16   1,2,5 / 1-6 / 1,2,4,5,6 / 1,2,3,5,6      4.2e-16
    cube4 developed precond 1   1.1e-16 .. 3.2e-14   1,2,3,5,6 / 1-6 / 1,2,3,5,6 / 1,2,3,5,6  4.8e-15
    (rest: the iterate is dominated by the boundary values, which both sides reproduce exactly)

    CG case (every k = 1 .. 6 kept)       d                    device
    box8 correction                       1.0e-15 .. 1.8e-15   5.4e-16
    box8 poisson neumann / outlet, 0      1.3e-16 .. 5.9e-16   3.9e-16 / 2.5e-16
    box8 poisson neumann / outlet, 1      2.7e-16 .. 1.3e-15   4.3e-16 / 9.9e-16
    cube4 correction                      8.6e-16 .. 1.7e-15   4.9e-16
    cube4 poisson neumann / outlet, 0     1.6e-16 .. 2.9e-16   1.7e-16 / 1.6e-16
    cube4 poisson neumann / outlet, 1     1.5e-16 .. 7.7e-16   4.4e-16 / 6.8e-16
    box128 correction                     4.3e-15 .. 7.0e-15   6.3e-16
    box128 poisson neumann / outlet, 0    2.1e-16 .. 1.3e-15   2.6e-16 / 6.3e-16
    box128 poisson neumann / outlet, 1    4.7e-16 .. 5.1e-15   1.3e-14 / 1.6e-15
    two thread ranks (box8 developed: BiCGStab precond 0, correction, poisson neumann)   5.4e-16

The largest 64 d is 2.0e-12 (cube4 developed precond 1, k = 4, where the residual rises); the floor 1e-14 is the bound
in most cases.  With deliberately wrong kernels (a k_dot_ts_tt that drops the second grid-stride trip; the fused update
forming beta from the previous omega; k_cgcg_update with half its beta term; k_sub_mean dividing by n - 1) the iterate
tests of the affected solver fail while the tight solves of BiCGStab still pass: converged fields heal.

Tight solves (rtol 1e-12, the confirmation path): info.residual is the true |b - A x| of the returned x, recomputed in
longdouble; allowed: one fp64 residual evaluation, eps |(m + 2) (|A| |x| + |b|) + |A| (|u*_before| + |u*_after|)|_2 with
m the longest row (the second term: x is observed as a difference of two rounded fields; absent for CG), times 2 for
the norm's own sum.

Out of scope: the Chebyshev mass solve (precond 2), CG preconditioned by fast-diagonalisation factors, the IMEX
diffusion solve, HIP-graph replay, RCCL."""
import numpy as np
import pytest
import scipy.sparse as sp

import _native as nat
import krylov_host as kh
import test_gpu_multigrid_cycle as mgc

pytestmark = pytest.mark.gpu

NU, BDF2 = mgc.NU, mgc.BDF2
# step sizes per (problem, state): chosen on the host alone (see the module docstring)
STEPS = {("box8", "rest"): 0.01, ("box8", "developed"): 0.01, ("box128", "rest"): 1e-4, ("box128", "developed"): 1e-4,
         ("cube4", "rest"): 0.2, ("cube4", "developed"): 0.01}
K_MAX = 6
SCHEDULES = [(0, 1), ("k", 1), (0, 2), (2, 3)]
SWITCH = "NSFEM_BICG_FUSED"
EPS = float(np.finfo(np.float64).eps)
_MAKERS = {"box8": lambda: mgc._box(8, 8), "box128": lambda: mgc._box(128, 128), "cube4": lambda: mgc._cube(4)}
_problems, _refs = {}, {}


def problem(name):
    if name not in _problems:
        _problems[name] = _MAKERS[name]()
        _problems[name].name = name
    return _problems[name]


# --------------------------------------------------------------------------------------------------- states
def fields(pb, state):
    """slot -> values: `rest` all zero; `developed` a smooth field that is no solution of anything"""
    dm, dim = pb.dm, pb.dim
    nv = dm.n_p2 * dim
    if state == "rest":
        return {nat.U1: np.zeros(nv), nat.U2: np.zeros(nv), nat.USTAR: np.zeros(nv), nat.P_OLD: np.zeros(dm.n_p1),
                nat.P: np.zeros(dm.n_p1)}
    X, Y = dm.p2_coords, pb.mesh.coords
    s, c = np.sin(np.pi * X), np.cos(np.pi * X)
    if dim == 2:
        u = np.stack([s[:, 0] * c[:, 1] + 0.3, -c[:, 0] * s[:, 1] + 0.2 * X[:, 0]], axis=1)
        w = np.stack([X[:, 0] ** 2, np.sin(2.0 * np.pi * X[:, 1])], axis=1)          # (not solenoidal)
        p = np.cos(np.pi * Y[:, 0]) * np.cos(np.pi * Y[:, 1])
        q = np.sin(np.pi * Y[:, 0]) * Y[:, 1]
    else:
        u = np.stack([s[:, 0] * c[:, 1] * c[:, 2] + 0.3, -c[:, 0] * s[:, 1] * c[:, 2] + 0.2 * X[:, 0],
                      0.4 * s[:, 2] * c[:, 0]], axis=1)
        w = np.stack([X[:, 0] ** 2, np.sin(2.0 * np.pi * X[:, 1]), X[:, 0] * X[:, 2]], axis=1)
        p = np.cos(np.pi * Y[:, 0]) * np.cos(np.pi * Y[:, 1]) * np.cos(np.pi * Y[:, 2])
        q = np.sin(np.pi * Y[:, 0]) * Y[:, 1] + Y[:, 2] ** 2
    return {nat.U1: u.ravel(), nat.U2: 0.8 * u.ravel(), nat.USTAR: (1.1 * u + 0.05 * w).ravel(), nat.P_OLD: p,
            nat.P: p + 0.3 * q}


def load(ctx, f):
    for slot, v in f.items():
        ctx.set_state(slot, v)


def velocity_flags(pb, dofs=None):
    m = np.zeros(pb.dm.n_p2 * pb.dim, dtype=bool)
    m[np.asarray(pb.vel[0] if dofs is None else dofs, dtype=np.int64)] = True
    return m


def pressure_flags(pb, dofs):
    m = np.zeros(pb.dm.n_p1, dtype=bool)
    m[np.asarray(dofs, dtype=np.int64)] = True
    return m


# ------------------------------------------------------------------------------------------- host references
def _prec(pb, which, precond, A, flags, dirichlet, dtype, step=None):
    """M^-1 of the host in one precision: Jacobi of the (masked) operator, or the V-cycle of mg_cycle_host"""
    if precond == 0:
        dinv = kh.jacobi(A, flags)
        return dinv, (lambda r: dinv * r)
    if which == "velocity":
        cyc = pb.H.velocity(dirichlet, BDF2[0] / step, NU, pb.degree, pb.eig_ratio, trunc_ratio=0.0, dtype=dtype)
    else:
        cyc = pb.H.pressure(dirichlet, pb.degree, pb.eig_ratio, dtype=dtype)
    return None, cyc.apply


class BicgReference:
    """host iterates of one momentum system in float64 and longdouble, d per iteration, and per schedule the kept k
    with their atol"""

    def __init__(self, pb, J, b, precond, step):
        flags = velocity_flags(pb)
        self.b = b
        self.h = {}
        for dt in (np.float64, kh.LD):
            A = kh.masked(J, flags, "identity", dt)
            _, prec = _prec(pb, "velocity", precond, A, flags, pb.vel[0], dt, step)
            self.h[dt] = kh.bicgstab(A, b, np.zeros_like(b), prec, K_MAX)
        h, hl = self.h[np.float64], self.h[kh.LD]
        self.d = [None] + [kh.rel(h.x[k], hl.x[k]) for k in range(1, K_MAX + 1)]
        self.tau, self.res_bound = [None], [None]
        for k in range(1, K_MAX + 1):
            ss, tt, ts, om = (float(v[k]) for v in (hl.ss, hl.tt, hl.ts, hl.omega))
            scale = np.sqrt(ss * tt) if ss * tt > 0.0 else 1.0
            d_sums = max(abs(float(h.ss[k]) - ss) / max(ss, 1e-300), abs(float(h.tt[k]) - tt) / max(tt, 1e-300),
                         abs(float(h.ts[k]) - ts) / scale)
            tau = max(64.0 * max(self.d[k], d_sums), 1e-14)
            self.tau.append(tau)
            self.res_bound.append(4.0 * tau * (ss + 2.0 * abs(om) * np.sqrt(ss * tt) + om * om * tt))
        self.kept, self.atol = {}, {}
        res, floor = [None] + [float(r) for r in h.res[1:]], 1e-9 * float(h.bnorm)
        for sched in SCHEDULES:
            self.kept[sched] = []
            for k in range(1, K_MAX + 1):
                fc, ce = schedule(sched, k)
                seen = [res[j] for j in range(1, k) if j >= fc and j % ce == 0]
                lo = max(res[k], floor)
                if res[k] < 0.1 * floor:
                    continue                                  # host residual below 1e-10 |b|
                if seen and min(seen) < 4.0 * lo:
                    continue                                  # window narrower than a factor 4
                self.kept[sched].append(k)
                self.atol[sched, k] = np.sqrt(lo * min(seen)) if seen else 2.0 * lo

    def check_kept(self, name):
        for sched in SCHEDULES:
            ks = self.kept[sched]
            assert len(ks) >= 3 and max(ks) >= 3, (name, sched, ks, [float(r) for r in self.h[np.float64].res[1:]])
        assert 64.0 * max(self.d[1:]) < 1e-10, (name, self.d)


def schedule(sched, k):
    fc, ce = sched
    return (k if fc == "k" else fc), ce


class CgReference:
    def __init__(self, pb, which, A_csr, nv, b, x0, flags, dirichlet, precond, project_mean):
        self.h = {}
        Afull = sp.kron(A_csr, sp.identity(nv), format="csr") if nv > 1 else A_csr
        for dt in (np.float64, kh.LD):
            A = kh.masked(Afull, flags, "zero", dt)
            dinv, prec = _prec(pb, which, precond, A, flags, dirichlet, dt)
            if precond == 0:
                self.h[dt] = kh.pcg_jacobi(A, b, x0, dinv, K_MAX, project_mean, flags)
            else:
                self.h[dt] = kh.pcg_single_reduction(A, b, x0, prec, K_MAX, project_mean, flags)
        h, hl = self.h[np.float64], self.h[kh.LD]
        self.d = [None] + [kh.rel(h.x[k] - x0, hl.x[k] - x0) for k in range(1, K_MAX + 1)]
        self.d_res = [None] + [abs(float(h.res[k] - hl.res[k])) / float(hl.res[k]) for k in range(1, K_MAX + 1)]
        self.kept = [k for k in range(1, K_MAX + 1) if float(h.res[k]) >= 1e-10 * float(h.bnorm)]

    def check_kept(self, name):
        assert len(self.kept) >= 3 and max(self.kept) >= 3, (name, self.kept)
        assert 64.0 * max(self.d[k] for k in self.kept) < 1e-10, (name, self.d)


# --------------------------------------------------------------------------------------------------- device
def device(pb, monkeypatch, state, switch=None, vel=None, pres=mgc.NO_DOFS):
    if switch is None:
        monkeypatch.delenv(SWITCH, raising=False)
    else:
        monkeypatch.setenv(SWITCH, switch)
    return mgc.device(pb, monkeypatch, k=STEPS[pb.name, state], vel=vel, pres=pres)


def failed_solve(ctx, system, **kw):
    """a solve that is to run out of iterations: the SolveInfo the error carries"""
    with pytest.raises(nat.NativeError) as err:
        ctx.solve(system, **kw)
    assert err.value.code == nat.ERR_NOT_CONVERGED, err.value
    return err.value.info


# ------------------------------------------------------------------------------------------------- BiCGStab
BICG_CASES = [("box8", "rest", 0), ("box8", "rest", 1), ("box8", "developed", 0), ("box8", "developed", 1),
              ("box128", "rest", 0), ("box128", "rest", 1), ("box128", "developed", 0), ("box128", "developed", 1),
              ("cube4", "rest", 0), ("cube4", "rest", 1), ("cube4", "developed", 0), ("cube4", "developed", 1)]


@pytest.mark.parametrize("pname,state,precond", BICG_CASES)
def test_bicgstab_iterates_equal_the_host_on_every_schedule_and_both_launch_sequences(pname, state, precond,
                                                                                      monkeypatch):
    pb = problem(pname)
    f = fields(pb, state)
    name = "%s %s precond %d" % (pname, state, precond)
    first, worst = {}, 0.0
    for switch in (None, "0"):
        ctx = device(pb, monkeypatch, state, switch)
        try:
            load(ctx, f)
            ctx.assemble(nat.SYS_MOMENTUM, new_step=True)
            b = ctx.get_rhs(nat.SYS_MOMENTUM)
            if name not in _refs:
                _refs[name] = BicgReference(pb, ctx.operator_csr(nat.OP_MOMENTUM_JAC), b, precond,
                                            STEPS[pname, state])
                print("\n[krylov] %-28s d %s\n%30s res/|b| %s\n%30s kept %s" % (
                    name, " ".join("%.1e" % v for v in _refs[name].d[1:]), "",
                    " ".join("%.1e" % (float(r) / float(_refs[name].h[np.float64].bnorm))
                             for r in _refs[name].h[np.float64].res[1:]), "",
                    {s: _refs[name].kept[s] for s in SCHEDULES}))
            ref = _refs[name]
            ref.check_kept(name)
            h = ref.h[np.float64]
            assert np.array_equal(b, ref.b)
            if state == "rest":
                free = ~velocity_flags(pb)
                assert np.abs(b[free]).max() == 0.0 and np.abs(b).max() == 1.0
                for dt in ref.h:
                    assert ref.h[dt].restart[2] is True and ref.h[dt].alpha[1] == 1.0, (name, dt)
            for sched in SCHEDULES:
                for k in ref.kept[sched]:
                    fc, ce = schedule(sched, k)
                    ctx.set_state(nat.USTAR, f[nat.USTAR])
                    ctx.assemble(nat.SYS_MOMENTUM)
                    info = ctx.solve(nat.SYS_MOMENTUM, rtol=1e-9, atol=ref.atol[sched, k], max_iter=k, precond=precond,
                                     check_every=ce, first_check=fc)
                    assert np.array_equal(ctx.get_rhs(nat.SYS_MOMENTUM), b), (name, sched, k)
                    x = f[nat.USTAR] - ctx.get_state(nat.USTAR)
                    tag = (name, switch, sched, k)
                    assert np.all(np.isfinite(x)), tag
                    assert info.iterations == k and info.converged == 1, (tag, info.iterations)
                    if k not in first:
                        err, bound = kh.rel(x, h.x[k]), max(64.0 * ref.d[k], 1e-14)
                        worst = max(worst, err)
                        assert 0.5 * EPS * (np.linalg.norm(f[nat.USTAR]) / np.linalg.norm(h.x[k]) + 1.0) <= 1e-15, tag
                        assert err <= bound, (tag, err, bound)
                        first[k] = x
                    assert np.array_equal(x, first[k]), (tag, kh.rel(x, first[k]))
                    assert abs(info.residual0 - float(h.r0)) <= ref.tau[k] * float(h.r0), (tag, info.residual0)
                    dres = abs(info.residual ** 2 - float(h.res[k]) ** 2)
                    assert dres <= ref.res_bound[k], (tag, info.residual, float(h.res[k]), dres, ref.res_bound[k])
        finally:
            ctx.close()
    print("[krylov] %-28s largest device deviation %.2e" % (name, worst))


# ------------------------------------------------------------------------------------------------------- CG
CG_CASES = [(p, s, bc, pre) for p in ("box8", "cube4") for s, bc, pre in
            (("correction", "cavity", 0), ("poisson", "neumann", 0), ("poisson", "outlet", 0),
             ("poisson", "neumann", 1), ("poisson", "outlet", 1))] + \
           [("box128", "correction", "cavity", 0), ("box128", "poisson", "neumann", 0), ("box128", "poisson", "outlet", 0),
            ("box128", "poisson", "neumann", 1), ("box128", "poisson", "outlet", 1)]


def _cg_system(ctx, pb, system, bc):
    """(system id, slot of x, operator, components, flags, Dirichlet dofs, mean projection)"""
    if system == "correction":
        return (nat.SYS_CORRECTION, nat.U0, ctx.operator_csr(nat.OP_MASS_P2), pb.dim, velocity_flags(pb), pb.vel[0],
                False)
    dofs = pb.outlet if bc == "outlet" else mgc.NO_DOFS
    return nat.SYS_POISSON, nat.P, ctx.operator_csr(nat.OP_STIFF_P1), 1, pressure_flags(pb, dofs), dofs, bc == "neumann"


@pytest.mark.parametrize("pname,system,bc,precond", CG_CASES)
def test_cg_iterates_equal_the_host(pname, system, bc, precond, monkeypatch):
    """classic CG (precond 0): the correction system -- velocity mass matrix, zero rows, start vector u* with the
    boundary values -- and the projection system, closed (mean projection) and with an outlet side; single-reduction
    CG (precond 1, the V(2,2) pressure cycle) on the same two projection systems"""
    pb = problem(pname)
    f = fields(pb, "developed")
    name = "%s %s %s precond %d" % (pname, system, bc, precond)
    ctx = device(pb, monkeypatch, "developed", pres=pb.outlet if bc == "outlet" else mgc.NO_DOFS)
    try:
        load(ctx, f)
        sysid, slot, A, nv, flags, dofs, pm = _cg_system(ctx, pb, system, bc)
        ctx.assemble(sysid)
        b, x0 = ctx.get_rhs(sysid), ctx.get_state(slot)
        assert np.abs(b).max() > 0.0 and (not flags.any() or np.abs(x0[flags]).max() > 0.0 or system == "poisson")
        if name not in _refs:
            _refs[name] = CgReference(pb, "velocity" if system == "correction" else "pressure", A, nv, b, x0, flags,
                                      dofs, precond, pm)
            print("\n[krylov] %-36s d %s  res/|b| %s" % (
                name, " ".join("%.1e" % v for v in _refs[name].d[1:]),
                " ".join("%.1e" % (float(r) / float(_refs[name].h[np.float64].bnorm))
                         for r in _refs[name].h[np.float64].res[1:])))
        ref = _refs[name]
        ref.check_kept(name)
        h = ref.h[np.float64]
        worst = 0.0
        for k in ref.kept:
            ctx.assemble(sysid)
            assert np.array_equal(ctx.get_state(slot), x0)
            info = failed_solve(ctx, sysid, rtol=1e-30, atol=0.0, max_iter=k, precond=precond)
            x = ctx.get_state(slot)
            assert np.array_equal(ctx.get_rhs(sysid), b), (name, k)
            bound = max(64.0 * ref.d[k], 1e-14)
            err = kh.rel(x - x0, h.x[k] - x0)
            worst = max(worst, err)
            assert np.all(np.isfinite(x)) and err <= bound, (name, k, err, bound)
            assert np.array_equal(x[flags], x0[flags]), (name, k)
            assert info.iterations == k and info.converged == 0, (name, k, info.iterations)
            assert abs(info.residual0 - float(h.r0)) <= bound * float(h.r0), (name, k, info.residual0, float(h.r0))
            rbound = max(64.0 * ref.d_res[k], bound)
            assert abs(info.residual - float(h.res[k])) <= rbound * float(h.res[k]), (name, k, info.residual,
                                                                                       float(h.res[k]), rbound)
        print("[krylov] %-36s largest device deviation %.2e" % (name, worst))
    finally:
        ctx.close()


# ---------------------------------------------------------------------------------------------- tight solves
def _true_residual(A_ld, A_abs, b, x, extra=None):
    """(|b - A x| in longdouble, rounding allowance of one fp64 evaluation of it)"""
    r = np.asarray(b, kh.LD) - A_ld.dot(np.asarray(x, kh.LD))
    m = int(np.diff(A_abs.indptr).max())
    per_row = (m + 2.0) * (A_abs @ np.abs(x) + np.abs(b))
    if extra is not None:
        per_row = per_row + A_abs @ extra
    return float(np.sqrt(r @ r)), 2.0 * EPS * float(np.linalg.norm(per_row))


@pytest.mark.parametrize("pname,precond", [("box8", 0), ("box8", 1), ("cube4", 0), ("cube4", 1)])
def test_tight_bicgstab_solve_reports_the_true_residual(pname, precond, monkeypatch):
    pb = problem(pname)
    f = fields(pb, "developed")
    ctx = device(pb, monkeypatch, "developed")
    try:
        load(ctx, f)
        ctx.assemble(nat.SYS_MOMENTUM, new_step=True)
        b = ctx.get_rhs(nat.SYS_MOMENTUM)
        flags = velocity_flags(pb)
        J = ctx.operator_csr(nat.OP_MOMENTUM_JAC)
        info = ctx.solve(nat.SYS_MOMENTUM, rtol=1e-12, atol=0.0, max_iter=2000, precond=precond)
        after = ctx.get_state(nat.USTAR)
        x = f[nat.USTAR] - after
        A64 = kh.masked(J, flags, "identity")
        true, allow = _true_residual(kh.masked(J, flags, "identity", kh.LD), abs(A64.A), b, x,
                                     np.abs(f[nat.USTAR]) + np.abs(after))
        target = 1e-12 * np.linalg.norm(b)
        print("\n[krylov] tight bicgstab %s precond %d: its %d residual %.3e true %.3e allowance %.1e target %.1e"
              % (pname, precond, info.iterations, info.residual, true, allow, target))
        assert info.converged == 1 and info.residual <= 10.0 * target
        assert abs(info.residual - true) <= allow, (info.residual, true, allow)
        assert np.array_equal(ctx.get_rhs(nat.SYS_MOMENTUM), b)
    finally:
        ctx.close()


@pytest.mark.parametrize("pname,bc", [("box8", "neumann"), ("box8", "outlet"), ("cube4", "neumann")])
def test_tight_single_reduction_cg_solve_reports_the_true_residual(pname, bc, monkeypatch):
    pb = problem(pname)
    f = fields(pb, "developed")
    ctx = device(pb, monkeypatch, "developed", pres=pb.outlet if bc == "outlet" else mgc.NO_DOFS)
    try:
        load(ctx, f)
        sysid, slot, K, _, flags, _, pm = _cg_system(ctx, pb, "poisson", bc)
        ctx.assemble(sysid)
        b = ctx.get_rhs(sysid)
        info = ctx.solve(sysid, rtol=1e-12, atol=0.0, max_iter=500, precond=1)
        x = ctx.get_state(slot)
        rhs = b - b.mean() if pm else b
        rhs_ld = np.asarray(b, kh.LD) - (np.sum(np.asarray(b, kh.LD)) / kh.LD(b.size) if pm else kh.LD(0.0))
        A64 = kh.masked(K, flags, "zero")
        r = np.where(flags, kh.LD(0.0), rhs_ld - kh.masked(K, flags, "zero", kh.LD).dot(np.asarray(x, kh.LD)))
        true = float(np.sqrt(r @ r))
        m = int(np.diff(A64.A.indptr).max())
        allow = 2.0 * EPS * float(np.linalg.norm(np.where(flags, 0.0, (m + 2.0) * (abs(A64.A) @ np.abs(x) + np.abs(rhs)))))
        target = 1e-12 * np.linalg.norm(rhs)
        print("\n[krylov] tight cg %s %s: its %d residual %.3e true %.3e allowance %.1e target %.1e"
              % (pname, bc, info.iterations, info.residual, true, allow, target))
        assert info.converged == 1 and info.residual <= 10.0 * target
        assert abs(info.residual - true) <= allow, (info.residual, true, allow)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------------------ b = 0
@pytest.mark.parametrize("pname", ["box8", "cube4"])
def test_zero_right_hand_sides_leave_the_start_vector_and_stay_finite(pname, monkeypatch):
    """state at rest, zero boundary values, zero force: all three systems, schedules (0, 1) and (3, 1), precond 0 and
    1 -- the solution is the start vector exactly, everything finite, converged; one IPCS step at rest with the
    throughput settings returns zero fields"""
    from test_gpu_bicgstab_fused import _throughput_opts
    pb = problem(pname)
    f = fields(pb, "rest")
    ctx = device(pb, monkeypatch, "rest", vel=(pb.vel[0], np.zeros(len(pb.vel[0]))))
    try:
        for sysid, slot in ((nat.SYS_MOMENTUM, nat.USTAR), (nat.SYS_POISSON, nat.P), (nat.SYS_CORRECTION, nat.U0)):
            for fc in (0, 3):
                for precond in (0, 1):
                    load(ctx, f)
                    ctx.assemble(sysid, new_step=True)
                    b, x0 = ctx.get_rhs(sysid), ctx.get_state(slot)
                    assert np.all(b == 0.0) and np.all(x0 == 0.0)
                    info = ctx.solve(sysid, rtol=1e-9, atol=1e-14, max_iter=50, precond=precond, check_every=1,
                                     first_check=fc)
                    x = ctx.get_state(slot)
                    tag = (pname, sysid, fc, precond)
                    assert np.all(np.isfinite(x)) and np.array_equal(x, x0), tag
                    assert info.converged == 1 and np.isfinite(info.residual) and np.isfinite(info.residual0), tag
                    assert info.residual == 0.0 and info.residual0 == 0.0, tag
        load(ctx, f)
        ctx.set_bdf((1.0, -1.0, 0.0), STEPS[pname, "rest"])
        info = ctx.step_ipcs(_throughput_opts(ctx))
        assert info.converged == 1
        for slot in (nat.USTAR, nat.U0, nat.P):
            x = ctx.get_state(slot)
            assert np.all(np.isfinite(x)) and np.all(x == 0.0), slot
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------- communicator branches
def test_two_thread_ranks_hold_the_same_host_iterates(monkeypatch):
    """nsfem_solve on partitioned contexts (two in-process thread ranks on strips of box8, precond 0): BiCGStab keeps
    its start kernel, reads |r0|, |b| after the start-up all-reduce (nothing deferred) and all-reduces every sum; both
    CG systems all-reduce theirs and the mean of the projection.  The owned rows of the ranks, put together, are held
    to the host iterates of the one global system (exported by a single context)."""
    import os
    import threading
    from partition import StripPartition
    pname, state, size = "box8", "developed", 2
    pb = problem(pname)
    f = fields(pb, state)
    step = STEPS[pname, state]
    monkeypatch.delenv(SWITCH, raising=False)
    ctx = device(pb, monkeypatch, state)
    try:
        load(ctx, f)
        ctx.assemble(nat.SYS_MOMENTUM, new_step=True)
        bicg = BicgReference(pb, ctx.operator_csr(nat.OP_MOMENTUM_JAC), ctx.get_rhs(nat.SYS_MOMENTUM), 0, step)
        cg = {}
        for system, bc in (("correction", "cavity"), ("poisson", "neumann")):
            sysid, slot, A, nv, flags, dofs, pm = _cg_system(ctx, pb, system, bc)
            ctx.assemble(sysid)
            cg[system] = (CgReference(pb, None, A, nv, ctx.get_rhs(sysid), ctx.get_state(slot), flags, dofs, 0, pm),
                          ctx.get_state(slot), flags)
    finally:
        ctx.close()
    bicg.check_kept("box8 developed precond 0 (global)")

    group = nat.local_group_create(size)
    parts = [StripPartition((0.0, 0.0), (1.0, 1.0), 8, 8, r, size, coarsest=2) for r in range(size)]
    ctxs = []
    for r, part in enumerate(parts):
        pdm = part.dofmap
        assert np.array_equal(pdm.p2_coords, pb.dm.p2_coords[part.p2_global])      # one numbering
        c = nat.NsfemContext(part.mesh.coords, part.mesh.cells, pdm.p2_dofmap, pdm.p1_dofmap, pdm.n_p2, pdm.n_p1)
        c.attach_local_comm(group, r)
        ctxs.append(c)
    gflags = velocity_flags(pb)
    gvals = np.zeros(gflags.size)
    gvals[np.asarray(pb.vel[0], np.int64)] = pb.vel[1]
    out = {}

    def worker(r):
        try:
            part, c = parts[r], ctxs[r]
            part.attach(c)
            vdofs = (2 * part.p2_global[:, None] + np.arange(2)[None, :]).ravel()          # local velocity dof -> global
            local = {s: (v[vdofs] if v.size == gflags.size else v[part.p1_global]) for s, v in f.items()}
            bc = np.nonzero(gflags[vdofs])[0].astype(np.int32)
            c.set_coeffs(1.0, 1.0, NU)
            c.set_bdf(BDF2, step)
            c.set_dirichlet(nat.VELOCITY, bc, gvals[vdofs][bc])
            c.set_dirichlet(nat.PRESSURE, np.zeros(0, np.int32), np.zeros(0))
            res = {}
            load(c, local)
            c.assemble(nat.SYS_MOMENTUM, new_step=True)
            for sched in SCHEDULES:
                for k in bicg.kept[sched]:
                    fc, ce = schedule(sched, k)
                    c.set_state(nat.USTAR, local[nat.USTAR])
                    c.assemble(nat.SYS_MOMENTUM)
                    info = c.solve(nat.SYS_MOMENTUM, rtol=1e-9, atol=bicg.atol[sched, k], max_iter=k, precond=0,
                                   check_every=ce, first_check=fc)
                    res["bicg", sched, k] = (local[nat.USTAR] - c.get_state(nat.USTAR),
                                             (info.iterations, info.converged, info.residual0, info.residual))
            for system, sysid, slot in (("correction", nat.SYS_CORRECTION, nat.U0), ("poisson", nat.SYS_POISSON, nat.P)):
                for k in cg[system][0].kept:
                    load(c, local)
                    c.assemble(sysid)
                    try:
                        c.solve(sysid, rtol=1e-30, atol=0.0, max_iter=k, precond=0)
                        raise RuntimeError("solve with max_iter = k and rtol 1e-30 converged")
                    except nat.NativeError as err:
                        info = err.info
                        res[system, k] = (c.get_state(slot), (info.iterations, err.code, info.residual0, info.residual))
            out[r] = res
        except BaseException as exc:                     # a dead rank would deadlock the others
            print("rank %d: %r" % (r, exc), flush=True)
            os._exit(17)

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(size)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for c in ctxs:
        c.close()
    nat.local_group_destroy(group)

    def gather(key, n, vector):
        x = np.full(n, np.nan)
        for r, part in enumerate(parts):
            if vector:
                x.reshape(-1, 2)[part.p2_global[part.p2_owned]] = out[r][key][0].reshape(-1, 2)[part.p2_owned]
            else:
                x[part.p1_global[part.p1_owned]] = out[r][key][0][part.p1_owned]
        assert np.all(np.isfinite(x)), key
        assert out[0][key][1] == out[1][key][1], key                # the ranks saw the same all-reduced sums
        return x, out[0][key][1]

    h, worst = bicg.h[np.float64], 0.0
    for sched in SCHEDULES:
        for k in bicg.kept[sched]:
            x, (its, conv, res0, res) = gather(("bicg", sched, k), gflags.size, True)
            err, bound = kh.rel(x, h.x[k]), max(64.0 * bicg.d[k], 1e-14)
            worst = max(worst, err)
            assert its == k and conv == 1 and err <= bound, (sched, k, its, conv, err, bound)
            assert abs(res0 - float(h.r0)) <= bicg.tau[k] * float(h.r0), (sched, k, res0)
            assert abs(res ** 2 - float(h.res[k]) ** 2) <= bicg.res_bound[k], (sched, k, res, float(h.res[k]))
    for system, n, vector in (("correction", gflags.size, True), ("poisson", pb.dm.n_p1, False)):
        ref, x0, flags = cg[system]
        ref.check_kept(system)
        hc = ref.h[np.float64]
        for k in ref.kept:
            x, (its, code, res0, res) = gather((system, k), n, vector)
            err, bound = kh.rel(x - x0, hc.x[k] - x0), max(64.0 * ref.d[k], 1e-14)
            worst = max(worst, err)
            assert its == k and code == nat.ERR_NOT_CONVERGED and err <= bound, (system, k, its, code, err, bound)
            rbound = max(64.0 * ref.d_res[k], bound)
            assert abs(res0 - float(hc.r0)) <= bound * float(hc.r0), (system, k, res0, float(hc.r0))
            assert abs(res - float(hc.res[k])) <= rbound * float(hc.res[k]), (system, k, res, float(hc.res[k]))
    print("\n[krylov] two thread ranks: largest device deviation %.2e" % worst)
