"""The linear algebra of the monolithic step (nsfem_step_bdf) on the device against its host restatement: the Schur
hierarchy mg_s and the mass smoother mg_m (nsfem_mg_apply 3 / 4) against `mg_cycle_host.Hierarchy.schur` /
`.mass_smoother`, the mixed operator and the block preconditioner (nsfem_monolithic_apply 0 / 1) against
`monolithic_host.mixed_matrix` / `BlockPreconditioner`, the iterates of the block-preconditioned BiCGStab through the
explicit seam (nsfem_assemble / nsfem_solve with SYS_MONOLITHIC) against `krylov_host.bicgstab`, one Newton iteration
through the seam against nsfem_step_bdf bit for bit, and the iteration count of a step against the host's count.
Problems, states, coefficient sets and the cached host references: tests/monolithic_cases.py.

Every case builds a fresh context and asserts through mg_lattice_info / smoother_info / jacobian_info that the path
it names was taken.  Lattice levels (default switches; 0 with NSFEM_LATTICE=0 / NSFEM_DICT=0): mg_s as mg_p of
tests/test_gpu_multigrid_cycle.py -- box16 0, box48 1, box96x40 2, box32x4 / cube4 / dfg 0, and 0 on algebraic levels
below 1024 rows --; mg_m is one level M_p: a lattice level from 1024 rows on (box48, box96x40).

Tolerance (the rule of tests/test_gpu_multigrid_cycle.py): per case and object d = rel(float64 host, longdouble host)
is measured on the host alone, the device is held to max(64 d, 1e-14), on the 48 x 48 box (inexact dictionaries, also
of the D / D^T blocks) plus 2^-38 on the paths that use them; 64 d < 1e-10 is asserted for every case.  BiCGStab
iterates: as tests/test_gpu_krylov_iterates.py -- x_k observed as the change of (U0, P) over a solve that converges
exactly at iteration k (rtol 1e-9, max_iter k, atol inside the window of the host's residual history); a k is dropped
from a schedule only where the window is narrower than a factor 4 or the host residual is below 1e-10 |b|; every
(case, schedule) keeps three k (asserted).

Measured on the host (d) and on the MI355X (largest device deviation over the launch paths of the case):

    object, case                                   d                    device
    mg_s  box16 rest (singular, CSR)               2.0e-16              2.6e-16
    mg_s  box96x40 developed (2 lattice levels)    5.9e-15              1.7e-14
    mg_s  box48 developed (inexact dictionary)     3.1e-16              1.3e-15
    mg_s  box32x4 geometric: outlet / emptied set  9.5e-15 / 5.0e-15    1.3e-14 / 1.5e-14
    mg_s  box32x4 algebraic (with / without set)   1.6e-13              2.5e-13
    mg_s  cube4 rest / developed                   2.7e-16 / 2.5e-16    9.5e-16 / 9.8e-16
    mg_s  dfg algebraic                            3.5e-14              3.6e-14
    mg_m  every case                               1.1e-16 .. 1.5e-16   2.7e-16 .. 1.3e-15
    dfg levels attach_schur_laplacian uploads      4.3e-16, 3.5e-16     9.6e-16, 8.8e-16   (entries / largest entry)
    MixedOp  box16 scaled pinned (16 variants x 2) 7.4e-17 .. 9.6e-17   4.5e-16
    MixedOp  box96x40 / box48 pinned               1.0e-16 / 2.9e-17    3.2e-16 / 2.1e-16
    MixedOp  box32x4 / cube4 / dfg                 1.7e-16 / 6.5e-17 / 1.8e-16    7.5e-16 / 1.7e-16 / 5.8e-16
    BlockPrec  box16 rest / shifted pinned / pinned  1.7e-16 / 2.7e-16 / 2.5e-16  4.2e-16 / 3.7e-16 / 4.1e-16
    BlockPrec  box96x40 pinned / box48 pinned      4.9e-15 / 3.4e-16    8.4e-15 / 1.6e-15
    BlockPrec  box32x4 geometric / algebraic       9.4e-15 / 1.6e-13    1.3e-14 / 2.5e-13
    BlockPrec  cube4 developed / dfg               2.1e-16 / 3.7e-14    1.1e-15 / 3.4e-14
    iterates 1 .. 4  box16 rest                    5.2e-17 .. 2.1e-15   6.9e-15
    iterates  box16 developed / shifted            2.8e-16 .. 1.6e-15   1.7e-15
    iterates  box48 developed                      2.7e-16 .. 7.8e-16   4.2e-15
    iterates  box32x4 algebraic short step         1.2e-15 .. 6.4e-13   9.6e-13
    iterates  cube4 rest / developed               7.4e-17 .. 3.7e-13   6.7e-13
    iterates  dfg algebraic                        1.8e-15 .. 6.2e-14   6.6e-14

The largest 64 d is 4.1e-11 (first iterate of the short-step channel on algebraic levels: LAPACK inverts the coarsest
algebraic level; d of such cases varies between machines by small factors); the floor 1e-14 is the bound in most
cases.  Kept k per schedule (0, 1) / (k, 1): box16 rest, box16 shifted, channel 1-4 / 1-4; box16 developed, box48,
cube4 rest 1-3 / 1-4; cube4 developed 1,3,4 / 1-4; dfg 1,2,4 / 1-4.  Iterations of the first linear solve of a step from
rest (rtol 1e-10), device / host: box16 9 / 9, box32x4 geometric 18 / 18, algebraic 9 / 9.  Launch records: mg_s
lattice levels / launches per cycle box96x40 2 / 4 (also with NSFEM_LATTICE_TRANSFERS=0), box48 1 / 2, otherwise
0 / 0; mg_m 1 / 1 on box96x40 and box48; Jacobian action "lattice-kernel" on box16, box48, box96x40, "three-launch"
with NSFEM_DICT=0, on the channel (585 P2 rows: no dictionary), the cube and the DFG mesh.

With deliberately wrong libraries (never committed) the module fails as follows, while
test_bdf_monolithic_cavity_matches_oracle passes with every one of them: BlockPrec without prec_shift -- the shifted
preconditioner and iterate cases (3 tests); launch_copy_at removed from BlockPrec -- every pinned preconditioner case
(10); mg_s refreshed with the pressure set -- 15, among them the channel's step count (and
test_bdf_monolithic_open_channel_and_stokes_limit, the only field test that notices any of the six); three mass
steps -- 36; - c_p D^T z_p in BlockPrec -- every preconditioner, iterate and step-count case (24); the pressure
identity rows dropped from MixedOp -- every pinned operator case (9).

Out of scope: partitioned contexts (additive Schur parts, global coarse solve), HIP-graph replay, RCCL, timing."""
import numpy as np
import pytest

import _native as nat
import krylov_host as kh
import mg_cycle_host as mh
import monolithic_cases as mc
import test_gpu_krylov_iterates as gki
import test_gpu_multigrid_cycle as mgc

pytestmark = pytest.mark.gpu

K_MAX = 4
SCHEDULES = [(0, 1), ("k", 1)]
EPS = gki.EPS
INEXACT = 2.0 ** -38
_worst = {}


def note(kind, name, err):
    _worst[kind, name] = max(_worst.get((kind, name), 0.0), err)


# ------------------------------------------------------------------------------------------------- device side
def device(name, monkeypatch, env="default", switch=None, load=True):
    """a fresh context in the state of the case: hierarchy, coefficients, BDF2, the three Dirichlet sets, the
    preconditioner shift, geometric or algebraic Schur operators, the state's fields"""
    ref = mc.reference(name)
    c, pb = ref.c, ref.pb
    if switch is None:
        monkeypatch.delenv(gki.SWITCH, raising=False)
    else:
        monkeypatch.setenv(gki.SWITCH, switch)
    ctx = mgc.device(pb, monkeypatch, env, k=c.k, pres=ref.pres)
    ctx.set_coeffs(c.cc, c.cp, c.cv)
    ctx.set_dirichlet(nat.PRESSURE_PRECOND, np.asarray(ref.schur, np.int32), np.zeros(len(ref.schur)))
    if c.shift:
        ctx.set_preconditioner_shift(c.shift)
    if c.algebraic:
        attach_algebraic(ctx, pb)
    if load:
        gki.load(ctx, mc.state_fields(pb, c.state))
    return ctx


def attach_algebraic(ctx, pb):
    """multigrid.attach_schur_laplacian on the context; returns the levels it uploaded and its singular flag"""
    from multigrid import attach_schur_laplacian
    uploaded = []
    upload = ctx.mg_set_schur_operator

    def record(level, csr, singular):
        uploaded.append((level, csr.copy(), bool(singular)))
        upload(level, csr, singular)

    ctx.mg_prolongations = [(cm.coords.shape[0], P) for cm, P in pb.levels]
    ctx.mg_set_schur_operator = record
    try:
        singular = attach_schur_laplacian(ctx, pb.vel[0])
    finally:
        del ctx.mg_set_schur_operator
    return uploaded, singular


def extra_of(name, env):
    return INEXACT if mc.CASES[name].pname == "box48" and env != "dict0" else 0.0


def lattice_levels(name, env, which):
    """levels of mg_s (which = 3) / mg_m (4) on the multi-step lattice kernel"""
    c = mc.CASES[name]
    if env in ("lattice0", "dict0"):
        return 0
    if which == 3:
        return 0 if c.algebraic else {"box16": 0, "box48": 1, "box96x40": 2}.get(c.pname, 0)
    return 1 if mc.problem(c.pname).dm.n_p1 >= 1024 and c.pname in ("box48", "box96x40") else 0


def compare_cycle(ctx, name, env, which, cyc64, cycld, tag=""):
    """mg_apply(which) against the host cycle on a seeded vector with a non-zero mean"""
    n = cyc64.A[0].shape[0]
    r = mc.seeded(name, "s" if which == 3 else "m", n) + 0.5
    z64 = cyc64.apply(r)
    d = mh.rel(z64, cycld.apply(r))
    before = ctx.mg_lattice_info(which)
    z = ctx.mg_apply(which, r)
    info = ctx.mg_lattice_info(which)
    launches = info["lattice_launches"] - before["lattice_launches"]
    err, bound = mh.rel(z, z64), max(64.0 * d, 1e-14) + extra_of(name, env)
    print("\n[monolithic] %-40s %-10s mg_apply(%d)%s levels %d lattice levels %d launches %d  d %.1e  err %.2e  bound %.1e"
          % (name, env, which, tag, info["levels"], info["lattice_levels"], launches, d, err, bound))
    note("cycle %d" % which, name, err)
    assert 64.0 * d < 1e-10, (name, which, d)
    assert info["levels"] == cyc64.n_levels, (name, which, info)
    want = lattice_levels(name, env, which)
    assert info["lattice_levels"] == want, (name, env, which, info)
    assert (launches > 0) == (want > 0), (name, env, which, launches)
    assert np.all(np.isfinite(z)) and err <= bound, (name, env, which, tag, err, bound)
    return z


# ------------------------------------------------------------------------------------- mg_s and mg_m alone
CYCLE_CASES = [(n, e) for n in ("box16 rest", "box96x40 developed") for e in ("default", "lattice0", "dict0", "transfers0")] + \
              [("box48 developed", "default"), ("box48 developed", "dict0"), ("box32x4 developed geometric", "default"),
               ("box32x4 developed algebraic", "default"), ("cube4 rest", "default"), ("cube4 developed", "default")]


@pytest.mark.parametrize("name,env", CYCLE_CASES)
def test_schur_hierarchy_and_mass_smoother_equal_the_host_cycles(name, env, monkeypatch):
    """nsfem_mg_apply(3) / (4) after the refreshes of the step: singular closed cavity (box16: CSR on every path),
    lattice levels with fused and explicit transfers (box96x40), the inexact dictionary (box48), the outlet set of
    the channel on geometric and on algebraic levels, 3D"""
    ref = mc.reference(name)
    ctx = device(name, monkeypatch, env)
    try:
        P, Pl = ref.prec(), ref.prec(mh.LD)
        z = compare_cycle(ctx, name, env, 3, P.S, Pl.S)
        assert np.all(z[ref.schur] == 0.0)
        compare_cycle(ctx, name, env, 4, P.Q, Pl.Q)
        info = ctx.mg_lattice_info(4)
        assert info["levels"] == 1
    finally:
        ctx.close()


def test_schur_hierarchy_follows_its_dirichlet_set_and_its_operators(monkeypatch):
    """the channel: geometric levels with the outlet set; the set emptied (masks, the now singular coarse inverse);
    the set of the PRESSURE field changed (must NOT reach mg_s); algebraic operators attached (levels, coarse inverse,
    singular flag of the operator); the outlet set on the algebraic levels"""
    name = "box32x4 developed geometric"
    ref = mc.reference(name)
    pb, H = ref.pb, ref.pb.H
    ctx = device(name, monkeypatch)
    try:
        z0 = compare_cycle(ctx, name, "default", 3, ref.prec().S, ref.prec(mh.LD).S, " outlet set")
        ctx.set_dirichlet(nat.PRESSURE_PRECOND, np.zeros(0, np.int32), np.zeros(0))
        none = mgc.NO_DOFS
        z1 = compare_cycle(ctx, name, "default", 3, H.schur(none), H.schur(none, dtype=mh.LD), " emptied set")
        assert mh.rel(z1, z0) > 1e-3
        ctx.set_dirichlet(nat.PRESSURE, np.asarray(pb.outlet, np.int32), np.zeros(pb.outlet.size))
        compare_cycle(ctx, name, "default", 3, H.schur(none), H.schur(none, dtype=mh.LD), " pressure set changed")
        ctx.set_dirichlet(nat.PRESSURE, np.zeros(0, np.int32), np.zeros(0))
        uploaded, singular = attach_algebraic(ctx, pb)
        ops, sing = H.algebraic_laplacian(pb.vel[0])
        opl, _ = H.algebraic_laplacian(pb.vel[0], mh.LD)
        assert singular == sing and not sing
        alg = mc.reference("box32x4 developed algebraic")
        z2 = compare_cycle(ctx, "box32x4 developed algebraic", "default", 3, alg.prec().S, alg.prec(mh.LD).S,
                           " algebraic levels")
        assert mh.rel(z2, z1) > 1e-3
        ctx.set_dirichlet(nat.PRESSURE_PRECOND, np.asarray(pb.outlet, np.int32), np.zeros(pb.outlet.size))
        cyc = [H.schur(pb.outlet, dtype=dt, operators=o, singular=sing) for dt, o in ((np.float64, ops), (mh.LD, opl))]
        z3 = compare_cycle(ctx, "box32x4 developed algebraic", "default", 3, cyc[0], cyc[1], " algebraic, outlet set")
        assert np.all(z3[pb.outlet] == 0.0)
    finally:
        ctx.close()


def test_attach_schur_laplacian_uploads_the_levels_the_host_forms(monkeypatch):
    """DFG channel (unstructured, one refinement): the product's attach_schur_laplacian -- device-exported D and
    mass diagonal, scipy products -- against the host's own construction from the oracle's matrices, level by level,
    entry by entry; then the cycle on those levels"""
    name = "dfg developed algebraic"
    ref = mc.reference(name)
    pb = ref.pb
    ctx = device(name, monkeypatch, load=False)
    try:
        uploaded, singular = attach_algebraic(ctx, pb)
        ops, sing = pb.H.algebraic_laplacian(pb.vel[0])
        opl, _ = pb.H.algebraic_laplacian(pb.vel[0], mh.LD)
        assert singular == sing and not sing                              # (open outlet)
        assert [u[0] for u in uploaded] == list(range(len(ops))) and len(ops) == 1 + len(pb.levels)
        for (level, csr, flag), o64, old in zip(uploaded, ops, opl):
            assert flag == sing
            dev, host, ld = csr.toarray(), o64.toarray(), np.asarray(old.toarray(), dtype=np.float64)
            scale = np.abs(host).max()
            d = np.abs(host - ld).max() / scale
            err = np.abs(dev - host).max() / scale
            print("\n[monolithic] dfg algebraic level %d: n %d  d %.1e  err %.2e" % (level, host.shape[0], d, err))
            assert 64.0 * d < 1e-10 and err <= max(64.0 * d, 1e-14), (level, d, err)
        assert ctx.smoother_info()["kind"] != "stencil-dictionary"
        compare_cycle(ctx, name, "default", 3, ref.prec().S, ref.prec(mh.LD).S)
        compare_cycle(ctx, name, "default", 4, ref.prec().Q, ref.prec(mh.LD).Q)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------------ the mixed operator
ALL_LINEARISATIONS = [(f, p) for f in range(4) for p in (False, True)]
OPERATOR_CASES = [("box16 developed scaled pinned", "default", ALL_LINEARISATIONS),
                  ("box16 developed scaled pinned", "dict0", ALL_LINEARISATIONS),
                  ("box96x40 developed pinned", "default", [(0, False), (3, True)]),
                  ("box48 developed pinned", "default", [(0, False), (1, True)]),
                  ("box48 developed pinned", "dict0", [(2, False)]),
                  ("box32x4 developed geometric", "default", [(0, False), (2, True)]),
                  ("cube4 developed", "default", [(0, False), (3, False), (2, True)]),
                  ("dfg developed algebraic", "default", [(0, False), (3, True)])]


def _snapshot(ctx):
    slots = {s: ctx.get_state(s) for s in (nat.U0, nat.U1, nat.U2, nat.USTAR, nat.P, nat.P_OLD)}
    rhs = {s: ctx.get_rhs(s) for s in (nat.SYS_MOMENTUM, nat.SYS_POISSON, nat.SYS_MONOLITHIC)}
    return slots, rhs


@pytest.mark.parametrize("name,env,linearisations", OPERATOR_CASES)
def test_mixed_operator_equals_the_host_matrix(name, env, linearisations, monkeypatch):
    """monolithic_apply(0, x) against mixed_matrix @ x: convective forms, Newton and Picard, assembled and matrix-free,
    NSFEM_DICT unset and 0; pressure Dirichlet rows (pinned cases), c_p != 1.  Linearity, and no state slot and no
    right-hand side is written"""
    ref = mc.reference(name)
    pb = ref.pb
    n = pb.dm.n_p2 * pb.dim + pb.dm.n_p1
    nv = n - pb.dm.n_p1
    x, x2 = mc.seeded(name, "x", n), mc.seeded(name, "x2", n)
    ctx = device(name, monkeypatch, env)
    try:
        ctx.assemble(nat.SYS_MONOLITHIC, new_step=True)           # (so that rhs_m exists and holds something)
        before = _snapshot(ctx)
        path = ctx.jacobian_info()["path"]
        # (a dictionary, and with it the one-launch lattice kernel, from 1024 P2 rows on: not on the 32 x 4 channel)
        lattice = env == "default" and ref.c.pname in ("box16", "box48", "box96x40")
        print("\n[monolithic] %-40s %-8s jacobian path %s" % (name, env, path))
        assert path == ("lattice-kernel" if lattice else "three-launch"), path
        for form, picard in linearisations:
            A, Al = ref.matrix(np.float64, form, picard), ref.matrix(mh.LD, form, picard)
            y64 = A.dot(x)
            d = mh.rel(y64, Al.dot(x.astype(mh.LD)))
            ctx.set_convective_form(form, picard)
            for mf in (False, True):
                launches = ctx.jacobian_info()["lattice_launches"]
                y = ctx.monolithic_apply(0, x, matrix_free=mf)
                used = ctx.jacobian_info()["lattice_launches"] - launches
                assert (used > 0) == (mf and path == "lattice-kernel"), (name, env, form, picard, mf, used)
                err, bound = mh.rel(y, y64), max(64.0 * d, 1e-14) + extra_of(name, env)
                print("\n[monolithic] %-40s %-8s MixedOp form %d picard %d mf %d  d %.1e  err %.2e  bound %.1e"
                      % (name, env, form, picard, mf, d, err, bound))
                note("operator", name, err)
                assert 64.0 * d < 1e-10 and err <= bound, (name, env, form, picard, mf, err, bound)
                # identity rows, bit for bit
                assert np.array_equal(y[pb.vel[0]], x[pb.vel[0]]) and np.array_equal(y[nv + ref.pres], x[nv + ref.pres])
                # linear: A (2 x - 0.5 x2) = 2 A x - 0.5 A x2 to rounding
                y2 = ctx.monolithic_apply(0, x2, matrix_free=mf)
                yc = ctx.monolithic_apply(0, 2.0 * x - 0.5 * x2, matrix_free=mf)
                scale = np.abs(A.A).dot(np.abs(2.0 * x) + np.abs(0.5 * x2))
                assert np.all(np.abs(yc - (2.0 * y - 0.5 * y2)) <= 64.0 * EPS * scale), (name, env, form, picard, mf)
        after = _snapshot(ctx)
        for s in before[0]:
            assert np.array_equal(before[0][s], after[0][s]), ("state slot written", s)
        for s in before[1]:
            assert np.array_equal(before[1][s], after[1][s]), ("right-hand side written", s)
    finally:
        ctx.close()


# ------------------------------------------------------------------------------------- the block preconditioner
PREC_CASES = [("box16 rest", "default"), ("box16 developed scaled shifted pinned", "default"),
              ("box16 developed scaled shifted pinned", "dict0"), ("box16 developed scaled pinned", "default"),
              ("box96x40 developed pinned", "default"), ("box96x40 developed pinned", "transfers0"),
              ("box96x40 developed pinned", "lattice0"), ("box48 developed pinned", "default"),
              ("box48 developed pinned", "dict0"), ("box32x4 developed geometric", "default"),
              ("box32x4 developed algebraic", "default"), ("cube4 developed", "default"),
              ("dfg developed algebraic", "default")]


@pytest.mark.parametrize("name,env", PREC_CASES)
def test_block_preconditioner_equals_the_host_restatement(name, env, monkeypatch):
    """monolithic_apply(1, r) against BlockPreconditioner.apply(r): r seeded, non-zero on every Dirichlet row, r_p with
    a non-zero mean; with and without prec_shift; c_p != 1 and c_v differing between the cases"""
    ref = mc.reference(name)
    pb = ref.pb
    nv = pb.dm.n_p2 * pb.dim
    r = mc.seeded(name, "r", nv + pb.dm.n_p1)
    r[nv:] += 0.75
    assert np.all(r[pb.vel[0]] != 0.0) and np.all(r[nv + ref.pres] != 0.0)
    z64 = ref.prec().apply(r)
    d = mh.rel(z64, ref.prec(mh.LD).apply(r))
    ctx = device(name, monkeypatch, env)
    try:
        states = {s: ctx.get_state(s) for s in (nat.U0, nat.U1, nat.U2, nat.P)}
        z = ctx.monolithic_apply(1, r)
        err, bound = mh.rel(z, z64), max(64.0 * d, 1e-14) + extra_of(name, env)
        errp = mh.rel(z[nv:], z64[nv:])
        print("\n[monolithic] %-40s %-10s BlockPrec  d %.1e  err %.2e (pressure part %.2e)  bound %.1e"
              % (name, env, d, err, errp, bound))
        note("preconditioner", name, err)
        assert 64.0 * d < 1e-10, (name, d)
        assert np.all(np.isfinite(z)) and err <= bound, (name, env, err, bound)
        assert np.array_equal(z[nv + ref.pres], r[nv + ref.pres]) and np.array_equal(z[pb.vel[0]], r[pb.vel[0]])
        assert np.array_equal(ctx.monolithic_apply(1, r), z)
        for s, v in states.items():
            assert np.array_equal(ctx.get_state(s), v), ("state slot written", s)
        assert ctx.mg_lattice_info(3)["lattice_levels"] == lattice_levels(name, env, 3)
        assert ctx.mg_lattice_info(4)["lattice_levels"] == lattice_levels(name, env, 4)
    finally:
        ctx.close()


# -------------------------------------------------------------------------------------------- BiCGStab iterates
class MixedReference:
    """host iterates x_1 .. x_K_MAX of one case in float64 and longdouble, d per iterate, and per schedule the kept k
    with their atol (the rule of test_gpu_krylov_iterates.BicgReference)"""

    def __init__(self, name):
        ref = mc.reference(name)
        self.b = ref.rhs()
        h, hl = ref.history(K_MAX), ref.history(K_MAX, mh.LD)
        self.h = h
        self.d = [None] + [kh.rel(h.x[k], hl.x[k]) for k in range(1, K_MAX + 1)]
        self.kept, self.atol = {}, {}
        res, floor = [None] + [float(r) for r in h.res[1:]], 1e-9 * float(h.bnorm)
        for sched in SCHEDULES:
            self.kept[sched] = []
            for k in range(1, K_MAX + 1):
                fc, ce = gki.schedule(sched, k)
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
            assert len(self.kept[sched]) >= 3, (name, sched, self.kept[sched], [float(r) for r in self.h.res[1:]])
        assert 64.0 * max(self.d[1:]) < 1e-10, (name, self.d)


ITERATE_CASES = ["box16 rest", "box16 developed", "box16 developed shifted", "box48 developed",
                 "box32x4 developed algebraic short step", "cube4 rest", "cube4 developed", "dfg developed algebraic"]
_mixed = {}


def mixed_reference(name):
    if name not in _mixed:
        _mixed[name] = MixedReference(name)
    return _mixed[name]


@pytest.mark.parametrize("name", ITERATE_CASES)
def test_monolithic_bicgstab_iterates_equal_the_host(name, monkeypatch):
    """x_k, k = 1 .. 4, of the step's BiCGStab (MixedOp, BlockPrec, zero start, known |b|) through the seam, on the
    schedules (0, 1) and (k, 1), with NSFEM_BICG_FUSED unset and 0; across schedules and the switch x_k is bitwise
    equal.  The right-hand side the device assembled is held to the host's residual first"""
    ref = mc.reference(name)
    pb = ref.pb
    nv = pb.dm.n_p2 * pb.dim
    mref = mixed_reference(name)
    mref.check_kept(name)
    h = mref.h
    f = mc.state_fields(pb, ref.c.state)
    start = np.concatenate([f[nat.U0], f[nat.P]])
    first = {}
    for switch in (None, "0"):
        ctx = device(name, monkeypatch, "default", switch)
        try:
            ctx.assemble(nat.SYS_MONOLITHIC, new_step=True)
            b = ctx.get_rhs(nat.SYS_MONOLITHIC)
            assert kh.rel(b, mref.b) <= 1e-13, kh.rel(b, mref.b)
            assert abs(ctx.residual_norm(nat.SYS_MONOLITHIC) - np.linalg.norm(b)) <= 1e-13 * np.linalg.norm(b)
            for sched in SCHEDULES:
                for k in mref.kept[sched]:
                    fc, ce = gki.schedule(sched, k)
                    gki.load(ctx, f)
                    ctx.assemble(nat.SYS_MONOLITHIC)
                    info = ctx.solve(nat.SYS_MONOLITHIC, rtol=1e-9, atol=mref.atol[sched, k], max_iter=k,
                                     check_every=ce, first_check=fc)
                    assert np.array_equal(ctx.get_rhs(nat.SYS_MONOLITHIC), b), (name, sched, k)
                    x = start - np.concatenate([ctx.get_state(nat.U0), ctx.get_state(nat.P)])
                    tag = (name, switch, sched, k)
                    assert np.all(np.isfinite(x)), tag
                    assert info.iterations == k and info.converged == 1, (tag, info.iterations)
                    if k not in first:
                        err, bound = kh.rel(x, h.x[k]), max(64.0 * mref.d[k], 1e-14)
                        print("\n[monolithic] %-40s iterate %d  d %.1e  err %.2e  bound %.1e" % (name, k, mref.d[k], err, bound))
                        note("iterate", name, err)
                        assert 0.5 * EPS * (np.linalg.norm(start) / np.linalg.norm(h.x[k]) + 1.0) <= 1e-15, tag
                        assert err <= bound, (tag, err, bound)
                        first[k] = x
                    assert np.array_equal(x, first[k]), (tag, kh.rel(x, first[k]))
        finally:
            ctx.close()


# ------------------------------------------------------------------------------------ the seam against the step
def _one_newton_opts(ctx, matrix_free, rtol=1e-10):
    opts = ctx.default_step_opts()
    opts.momentum.rtol = rtol
    opts.momentum.precond = 1
    opts.momentum.max_iter = 500
    opts.newton_max_iter = 1
    opts.allow_nonconvergence = 1
    opts.matrix_free = 2 if matrix_free else 1
    return opts


@pytest.mark.parametrize("name", ["box16 developed", "cube4 developed"])
@pytest.mark.parametrize("matrix_free", [False, True])
def test_one_newton_iteration_through_the_seam_is_the_step_bit_for_bit(name, matrix_free, monkeypatch):
    """assemble + solve with SYS_MONOLITHIC against nsfem_step_bdf with newton_max_iter = 1 on a fresh context each
    (the step's solve-hint predictor has seen no solve: it postpones no check), same Krylov options: U0 and P equal
    bit for bit, and so do the iteration counts and the residual norms"""
    ref = mc.reference(name)
    f = mc.state_fields(ref.pb, ref.c.state)
    ctx = device(name, monkeypatch)
    try:
        opts = _one_newton_opts(ctx, matrix_free)
        info = ctx.step_bdf(opts)
        u_step, p_step = ctx.get_state(nat.U0), ctx.get_state(nat.P)
    finally:
        ctx.close()
    ctx = device(name, monkeypatch)
    try:
        ctx.assemble(nat.SYS_MONOLITHIC, new_step=True, matrix_free=matrix_free)
        r0 = ctx.residual_norm(nat.SYS_MONOLITHIC)
        si = ctx.solve(nat.SYS_MONOLITHIC, rtol=1e-10, atol=1e-14, max_iter=500)
        assert si.iterations == info.krylov_iterations_momentum and info.newton_iterations == 1
        assert abs(r0 - info.newton_residuals[0]) <= 1e-13 * r0
        assert np.array_equal(ctx.get_state(nat.U0), u_step) and np.array_equal(ctx.get_state(nat.P), p_step)
        assert not np.array_equal(u_step, f[nat.U0])
        ctx.assemble(nat.SYS_MONOLITHIC)
        assert abs(ctx.residual_norm(nat.SYS_MONOLITHIC) - info.newton_residuals[1]) <= 1e-12 * info.newton_residuals[1]
    finally:
        ctx.close()


@pytest.mark.parametrize("name", ["box16 rest", "box32x4 rest geometric", "box32x4 rest algebraic"])
def test_step_needs_the_iterations_the_host_restatement_needs(name, monkeypatch):
    """the first linear solve of nsfem_step_bdf from rest (rtol 1e-10) against the count tests/test_monolithic_host.py
    records for the host's BiCGStab on the same system: equal +- 1.  A preconditioner that is wrong in a way that
    heals shows here, and only here, among the tests of converged fields"""
    ref = mc.reference(name)
    ctx = device(name, monkeypatch)
    try:
        info = ctx.step_bdf(_one_newton_opts(ctx, False))
        print("\n[monolithic] %-40s step count %d  host %d" % (name, info.krylov_iterations_momentum, mc.HOST_COUNTS[name]))
        assert abs(info.krylov_iterations_momentum - mc.HOST_COUNTS[name]) <= 1, (name, info.krylov_iterations_momentum)
    finally:
        ctx.close()


def test_hooks_refuse_what_they_do_not_cover(monkeypatch):
    """bad selectors are refused; so is every new entry on a context with a communicator (two in-process ranks, as
    tests/test_gpu_krylov_iterates.py attaches them: the refusal comes before anything collective), with a message
    that says why"""
    ctx = device("box16 rest", monkeypatch)
    try:
        n = ctx.n_velocity + ctx.n_p1
        for call in (lambda: ctx.mg_apply(5, np.zeros(ctx.n_p1)), lambda: ctx.monolithic_apply(2, np.zeros(n))):
            with pytest.raises(nat.NativeError):
                call()
    finally:
        ctx.close()
    pb = mc.problem("box16")
    group = nat.local_group_create(2)
    ctxs = [mgc.context(pb.mesh, pb.dm) for _ in range(2)]
    try:
        for r, c in enumerate(ctxs):
            c.attach_local_comm(group, r)
        c = ctxs[0]
        n = c.n_velocity + c.n_p1
        for call in (lambda: c.mg_apply(3, np.zeros(c.n_p1)), lambda: c.mg_apply(4, np.zeros(c.n_p1)),
                     lambda: c.mg_lattice_info(3), lambda: c.mg_lattice_info(4),
                     lambda: c.monolithic_apply(0, np.zeros(n)), lambda: c.monolithic_apply(1, np.zeros(n)),
                     lambda: c.assemble(nat.SYS_MONOLITHIC, new_step=True)):
            with pytest.raises(nat.NativeError) as err:
                call()
            assert "communicator" in str(err.value), str(err.value)
    finally:
        for c in ctxs:
            c.close()
        nat.local_group_destroy(group)
