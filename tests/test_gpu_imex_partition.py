"""IMEX pressure-correction step on partitioned strips and slabs (nsfem_step_imex / nsfem_imex_rhs with a
communicator attached): several contexts in one process, one host thread per rank, coupled by the in-process
communicator (as tests/test_gpu_partition.py).

* the one-launch right-hand side on a strip (k_jac_lattice<FORM, 4>) against the generic launch sequence on the same
  strip, bit for bit on owned rows, zeros on ghost rows; against the single context's generic right-hand side to
  1e-13 relative (the project's bound for kernel-against-oracle comparisons);
* its message count: one halo exchange, no all-reduce;
* whole steps against the single context with the tolerances of test_partitioned_ipcs_equals_single_context
  (exact halo mode u 1e-11, p 1e-10; relaxed 1e-9 / 1e-8) and of test_partitioned_3d_slabs_equal_single_context;
* the single-context 3D step against the numpy restatement (tolerances of tests/test_gpu_imex.py).

Without the feature every partitioned test here stops at the first step_imex / imex_rhs with the NativeError
"IMEX pressure correction: partitioned meshes are not supported"."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import _native as nat
import fem_oracle as fo
from fem_mesh import TaylorHoodDofMap
from gpu_common import box, context, rel
from imex_time_stepping import IMEXTimeStepping, IMEXType
from multigrid import attach_hierarchy
from partition import StripPartition
from test_gpu_imex import _SETS
from test_imex_solver_host import IMEXRestatement

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NO_PBC = (np.zeros(0, np.int32), np.zeros(0))


def _cavity_bc(dm, p1=(1.0, 1.0)):
    X = dm.p2_coords
    on = (np.abs(X[:, 0]) < 1e-12) | (np.abs(X[:, 0] - p1[0]) < 1e-12) | (np.abs(X[:, 1]) < 1e-12) | \
        (np.abs(X[:, 1] - p1[1]) < 1e-12)
    nodes = np.nonzero(on)[0]
    lid = np.abs(X[nodes, 1] - p1[1]) < 1e-12
    return (np.concatenate([2 * nodes, 2 * nodes + 1]).astype(np.int32),
            np.concatenate([np.where(lid, 1.0, 0.0), np.zeros(nodes.size)]))


def _grade(mesh):
    """x spacings h / 2 on the left half of the unit square and 3 h / 2 on the right: a lattice, not a uniform one"""
    x = mesh.coords[:, 0].copy()
    mesh.coords[:, 0] = np.where(x <= 0.5, 0.5 * x, 0.25 + 1.5 * (x - 0.5))


def _on_ranks(parts, work, overlap=False):
    """work(rank, part, ctx, out) on one thread per rank; the contexts carry the in-process communicator"""
    size = len(parts)
    group = nat.local_group_create(size)
    ctxs = []
    for r, part in enumerate(parts):
        pdm = part.dofmap
        c = nat.NsfemContext(part.mesh.coords, part.mesh.cells, pdm.p2_dofmap, pdm.p1_dofmap, pdm.n_p2, pdm.n_p1)
        c.attach_local_comm(group, r)
        c.set_overlap(overlap)
        ctxs.append(c)
    out, errors = {}, []

    def worker(r):
        try:
            work(r, parts[r], ctxs[r], out)
        except BaseException as exc:                     # a dead rank would deadlock the others
            errors.append((r, repr(exc)))
            print("rank %d failed: %r" % (r, exc), flush=True)
            os._exit(17)

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(size)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    for c in ctxs:
        c.close()
    nat.local_group_destroy(group)
    return out


def _plain_partition(ctx, part, r, size, nx, ny):
    ctx.set_partition(r, size, part.p2_ghost, part.p1_ghost, part.p2_halo, part.p1_halo,
                      (2 * nx + 1) * (2 * ny + 1), (nx + 1) * (ny + 1))


# ---------------------------------------------------------------- the right-hand side alone
@pytest.mark.parametrize("nx,ny,size,p1", [(32, 32, 2, (1.0, 1.0)), (64, 64, 4, (1.0, 1.0)), (80, 24, 2, (5.0, 1.5))])
def test_strip_rhs_one_launch_equals_generic_bit_for_bit(nx, ny, size, p1):
    """Uniform strips with full and partial 32 x 8 tiles, all four convective forms, the first-order and the four
    second-order coefficient sets of tests/test_gpu_imex.py.  The ghost entries of u1 and u2 handed to the ranks are
    noise: what the kernels read there must come from the exchange.  Message count of one right-hand side: at most 2
    halo exchanges, no all-reduce (the first one of a rank sends u1 and u2 in one packed message, later ones u1)."""
    mesh, dm, _ = box(nx, ny, p1=p1)
    rng = np.random.default_rng(7 * nx + ny)
    u1, u2, f = (rng.standard_normal(dm.n_velocity) for _ in range(3))
    p_old = rng.standard_normal(dm.n_p1)
    bd, bv = _cavity_bc(dm, p1)

    def setup(ctx, d, vecs):
        ctx.set_coeffs(0.8, 1.0, 0.02, 0.7)
        ctx.set_dirichlet(nat.VELOCITY, *_cavity_bc(d, p1))
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        for slot, v in zip((nat.U1, nat.U2, nat.BODY_FORCE, nat.P_OLD), vecs):
            ctx.set_state(slot, v)

    ref = {}
    ctx0 = context(mesh, dm)
    try:
        setup(ctx0, dm, (u1, u2, f, p_old))
        for form_id in range(4):
            for tag, (alpha, beta, gamma) in _SETS:
                ctx0.set_imex(alpha, beta, gamma, 1.0 / 64.0)
                ref[(form_id, tag)] = ctx0.imex_rhs("generic", form_id)
    finally:
        ctx0.close()
    del bd, bv

    parts = [StripPartition((0.0, 0.0), p1, nx, ny, r, size) for r in range(size)]

    def work(r, part, ctx, out):
        _plain_partition(ctx, part, r, size, nx, ny)
        g2 = part.p2_global
        noise = np.random.default_rng(1000 + r)

        def local(v):
            w = v.reshape(-1, 2)[g2].copy()
            w[~part.p2_owned] = noise.standard_normal((int((~part.p2_owned).sum()), 2))
            return w.ravel()

        setup(ctx, part.dofmap, (local(u1), local(u2), f.reshape(-1, 2)[g2].ravel(), p_old[part.p1_global]))
        res = {}
        for form_id in range(4):
            for tag, (alpha, beta, gamma) in _SETS:
                ctx.set_imex(alpha, beta, gamma, 1.0 / 64.0)
                s0 = ctx.comm_stats()
                g_rhs, g_n1 = ctx.imex_rhs("generic", form_id)
                s1 = ctx.comm_stats()
                l_rhs, l_n1 = ctx.imex_rhs("lattice-kernel", form_id)
                s2 = ctx.comm_stats()
                res[(form_id, tag)] = (g_rhs, g_n1, l_rhs, l_n1,
                                       (s1["exchanges"] - s0["exchanges"], s2["exchanges"] - s1["exchanges"],
                                        s2["allreduce_calls"] - s1["allreduce_calls"]))
        out[r] = res

    out = _on_ranks(parts, work)
    bit_equal = True
    for key, (ref_rhs, ref_n1) in ref.items():
        rhs = np.zeros_like(ref_rhs)
        n1 = np.zeros_like(ref_n1)
        for r, part in enumerate(parts):
            g_rhs, g_n1, l_rhs, l_n1, (ex_g, ex_l, ar_l) = out[r][key]
            own = np.repeat(part.p2_owned, 2)
            assert np.isfinite(l_rhs).all() and np.abs(l_rhs[own]).max() > 0.0
            assert np.array_equal(l_rhs[own], g_rhs[own]), (key, r, np.abs(l_rhs - g_rhs)[own].max())
            assert np.array_equal(l_n1[own], g_n1[own]), (key, r, np.abs(l_n1 - g_n1)[own].max())
            assert not l_rhs[~own].any() and not l_n1[~own].any(), (key, r)      # ghost rows: exactly 0
            assert not g_rhs[~own].any() and not g_n1[~own].any(), (key, r)
            assert ex_l <= 2 and ar_l == 0 and ex_g <= 2, (key, r, ex_g, ex_l, ar_l)
            rhs.reshape(-1, 2)[part.p2_global[part.p2_owned]] = l_rhs.reshape(-1, 2)[part.p2_owned]
            n1.reshape(-1, 2)[part.p2_global[part.p2_owned]] = l_n1.reshape(-1, 2)[part.p2_owned]
        e_rhs, e_n1 = rel(rhs, ref_rhs), rel(n1, ref_n1)
        bit_equal = bit_equal and np.array_equal(rhs, ref_rhs) and np.array_equal(n1, ref_n1)
        assert e_rhs < 1e-13 and e_n1 < 1e-13, (key, e_rhs, e_n1)
    print("\n[%d x %d, %d ranks] strips against the single context: bit-equal = %s" % (nx, ny, size, bit_equal))
    # spacing 1 / 16, 1 / 32, 1 / 64: the operators of a strip have the bits of the global ones (same dictionary
    # entries, same element geometry), and the kernels sum in the same order -- measured bit-equal, kept so
    assert bit_equal


# ---------------------------------------------------------------- whole steps
def _run(ctx, dm, typ, nsteps, k, use_mg, cheb, out, key, fd=False, change_after=None, probe_generic=False):
    ctx.set_coeffs(1.0, 1.0, 0.01)
    ctx.set_dirichlet(nat.VELOCITY, *_cavity_bc(dm))
    ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
    opts = ctx.default_step_opts()
    for o in (opts.momentum, opts.poisson, opts.correction):
        o.rtol = 1e-12
    if use_mg:
        opts.momentum.precond = opts.poisson.precond = 1
    if fd:
        opts.poisson.precond = 3
    if cheb:
        opts.correction.precond = 2
    ts = IMEXTimeStepping(0.0, 1.0e9, typ, desired_start_time_step=k)
    infos, ex = [], []
    for step in range(nsteps):
        if change_after is not None and step == change_after:
            ts.set_desired_next_step_size(0.5 * k)
        ts.update_coefficients()
        ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
        e0 = ctx.comm_stats()["exchanges"]
        infos.append(ctx.step_imex(opts))
        ex.append(ctx.comm_stats()["exchanges"] - e0)
        ctx.advance(0)
        ts.advance_time()
    generic_ex = None
    if probe_generic:                 # u2 came from advance: what one generic right-hand side costs in this run
        e0 = ctx.comm_stats()["exchanges"]
        ctx.imex_rhs("generic", 0)
        generic_ex = ctx.comm_stats()["exchanges"] - e0
    out[key] = dict(u=ctx.get_state(nat.U1), p=ctx.get_state(nat.P_OLD), infos=infos, imex=ctx.imex_info(),
                    exchanges=ex, generic_ex=generic_ex, comm=ctx.comm_stats(), overlapped=ctx.comm_overlapped())


def _compare(parts, out, ref, relaxed, dim=2):
    u = np.zeros_like(ref["u"])
    p = np.zeros_like(ref["p"])
    for r, part in enumerate(parts):
        o = out[r]
        u.reshape(-1, dim)[part.p2_global[part.p2_owned]] = o["u"].reshape(-1, dim)[part.p2_owned]
        p[part.p1_global[part.p1_owned]] = o["p"][part.p1_owned]
        for a, b in zip(o["infos"], ref["infos"]):
            assert a.newton_iterations == b.newton_iterations == 0
            if relaxed:
                assert abs(a.krylov_iterations_momentum - b.krylov_iterations_momentum) <= 3
                assert abs(a.krylov_iterations_poisson - b.krylov_iterations_poisson) <= 3
            else:
                assert a.krylov_iterations_momentum == b.krylov_iterations_momentum
                assert a.krylov_iterations_poisson == b.krylov_iterations_poisson
    eu, ep = rel(u, ref["u"]), rel(p - p.mean(), ref["p"] - ref["p"].mean())
    print("u %.2e p %.2e cg %s / %s" % (eu, ep, [i.krylov_iterations_momentum for i in out[0]["infos"]],
                                        [i.krylov_iterations_momentum for i in ref["infos"]]))
    assert eu < (1e-9 if relaxed else 1e-11)
    assert ep < (1e-8 if relaxed else 1e-10)
    return u, p


@pytest.mark.parametrize("n,size,use_mg,tail,cheb,relaxed,overlap,typ,change", [
    (16, 2, False, False, False, False, False, "SBDF2", None), (32, 4, True, False, False, False, False, "SBDF2", None),
    (64, 2, True, False, False, False, False, "SBDF2", 2), (64, 2, True, True, False, False, False, "CNAB", None),
    (32, 2, True, False, True, False, False, "SBDF2", None), (64, 4, True, False, True, True, False, "SBDF2", None),
    (64, 2, True, True, False, True, False, "SBDF2", None),
    (64, 2, False, False, False, False, True, "SBDF2", None), (64, 2, True, False, True, False, True, "SBDF2", 1),
    (64, 4, True, True, True, True, True, "SBDF2", None)])
def test_partitioned_imex_equals_single_context(n, size, use_mg, tail, cheb, relaxed, overlap, typ, change):
    """The parameter table of test_partitioned_ipcs_equals_single_context (Jacobi and multigrid, replicated tail,
    Chebyshev mass solve, relaxed and exact halo mode, overlap on and off, 2 and 4 ranks): cavity, 3 steps, rtol
    1e-12; typ: the IMEX scheme; change: the step whose size is halved (the matrix is rebuilt on every rank)."""
    nsteps, k, coarsest = 3, 0.01, 2
    typ = IMEXType[typ]
    mesh, dm, _ = box(n, n)
    ref = {}
    ctx0 = context(mesh, dm)
    if use_mg:
        attach_hierarchy(ctx0, mesh, coarsest=coarsest)
    _run(ctx0, dm, typ, nsteps, k, use_mg, cheb, ref, 0, change_after=change)
    ctx0.close()
    ref = ref[0]
    assert ref["comm"]["exchanges"] == 0 and ref["comm"]["allreduce_calls"] == 0
    parts = [StripPartition((0.0, 0.0), (1.0, 1.0), n, n, r, size, coarsest=16 if tail else coarsest,
                            global_coarsest=coarsest if tail else None) for r in range(size)]
    assert bool(parts[0].global_tail) == tail

    def work(r, part, ctx, out):
        if use_mg:
            part.attach(ctx)
            ctx.mg_set_halo_mode(relaxed)
        else:
            _plain_partition(ctx, part, r, size, n, n)
        _run(ctx, part.dofmap, typ, nsteps, k, use_mg, cheb, out, r, change_after=change)

    out = _on_ranks(parts, work, overlap)
    u, _ = _compare(parts, out, ref, relaxed)
    for r, part in enumerate(parts):                     # ghosts are copies of the owners' values
        assert np.abs(out[r]["u"].reshape(-1, 2) - u.reshape(-1, 2)[part.p2_global]).max() < 1e-13
        info = out[r]["imex"]
        if n >= 32:                                      # the one-launch right-hand side on every rank, every step
            assert info["path"] == "lattice-kernel" and info["generic_rhs"] == 0 and info["lattice_rhs"] == nsteps, (r, info)
        assert info["matrix_builds"] == ref["imex"]["matrix_builds"], (r, info, ref["imex"])
        st = out[r]["comm"]
        assert st["exchanges"] == out[0]["comm"]["exchanges"] > 0
        assert st["allreduce_calls"] == out[0]["comm"]["allreduce_calls"] > 0
        if overlap:
            # strips of 32 cell rows: 65 (+ ghost) lattice lines, tile rows of 14 lines -- the split exists, and the
            # exchange of every right-hand side after the first (packed, blocking) one runs under the interior tile rows
            assert out[r]["overlapped"] >= nsteps - 1, (r, out[r]["overlapped"])
        else:
            assert out[r]["overlapped"] == 0


def test_partitioned_imex_rhs_exchange_is_overlapped_and_counted():
    """n = 64 on 2 ranks, Jacobi (no other overlapped exchange than the operator products of the CG solves): with
    the overlap mode on, one more overlapped exchange per step than the CG iterations explain is the right-hand
    side's.  Counted exactly: every CG iteration exchanges once, overlapped; the right-hand sides of steps 2 and 3
    add one each (step 1 sends u1 and u2 packed, blocking)."""
    n, size = 64, 2
    parts = [StripPartition((0.0, 0.0), (1.0, 1.0), n, n, r, size) for r in range(size)]

    def work(r, part, ctx, out):
        _plain_partition(ctx, part, r, size, n, n)
        ctx.set_coeffs(1.0, 1.0, 0.01)
        ctx.set_dirichlet(nat.VELOCITY, *_cavity_bc(part.dofmap))
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        rng = np.random.default_rng(3)
        ctx.set_state(nat.U1, rng.standard_normal(part.dofmap.n_velocity))
        ctx.set_imex((1.5, -2.0, 0.5), (2.0, -1.0), (1.0, 0.0, 0.0), 0.01)
        counts = []
        for _ in range(3):                               # the right-hand side alone: nsfem_imex_rhs
            o0, e0 = ctx.comm_overlapped(), ctx.comm_stats()["exchanges"]
            ctx.imex_rhs("lattice-kernel", 0)
            counts.append((ctx.comm_stats()["exchanges"] - e0, ctx.comm_overlapped() - o0))
        out[r] = counts

    out = _on_ranks(parts, work, overlap=True)
    for r in range(size):
        # first call: u2 was never exchanged -- one packed blocking message; then u1 alone under the interior tile rows
        assert out[r] == [(1, 0), (1, 1), (1, 1)], (r, out[r])


def test_step_costs_the_exchanges_of_its_solves_plus_one(monkeypatch):
    """exchanges(step i) - exchanges(step i with the right-hand side from the generic path) = 1 - (what the generic
    right-hand side needs, read from the run).  The generic path is forced by NSFEM_JAC_LATTICE=0 (read when a context
    is created); the right-hand sides agree bit for bit, so the three solves of a step exchange the same number of
    times in both runs."""
    n, size, nsteps = 32, 2, 3
    runs = {}
    for lattice in (True, False):
        if not lattice:
            monkeypatch.setenv("NSFEM_JAC_LATTICE", "0")
        parts = [StripPartition((0.0, 0.0), (1.0, 1.0), n, n, r, size, coarsest=2) for r in range(size)]

        def work(r, part, ctx, out):
            part.attach(ctx)
            _run(ctx, part.dofmap, IMEXType.SBDF2, nsteps, 0.01, True, False, out, r, probe_generic=True)

        runs[lattice] = _on_ranks(parts, work)
    monkeypatch.delenv("NSFEM_JAC_LATTICE")
    context(*box(4, 4)[:2]).close()                      # (a context created now re-reads the switch)
    for r in range(size):
        a, b = runs[True][r], runs[False][r]
        assert a["imex"]["path"] == "lattice-kernel" and b["imex"]["path"] == "generic"
        assert np.array_equal(a["u"], b["u"]) and np.array_equal(a["p"], b["p"])
        g = b["generic_ex"]
        assert g is not None and g >= 1
        print("rank %d: exchanges per step %s (one-launch) %s (generic); generic right-hand side: %d" % (
            r, a["exchanges"], b["exchanges"], g))
        for i in range(1, nsteps):                       # (steps whose u2 came from advance)
            assert a["exchanges"][i] - b["exchanges"][i] == 1 - g, (r, i, a["exchanges"], b["exchanges"], g)


@pytest.mark.parametrize("n,size,relaxed", [(32, 2, False), (64, 4, True)])
def test_partitioned_imex_with_fast_diagonalisation_projection(n, size, relaxed):
    """poisson.precond = 3 with strip factors: the projection is one pass, as in
    test_partitioned_fast_diagonalisation_projection_equals_single_context"""
    import poisson_fd as pf
    nsteps, k = 3, 0.01
    mesh, dm, _ = box(n, n)
    mesh.structured = ((0.0, 0.0), (1.0, 1.0), n, n)
    xs = np.linspace(0.0, 1.0, n + 1)
    factors = pf.factors(xs, xs, np.zeros(0, np.int64))
    ref = {}
    ctx0 = context(mesh, dm)
    attach_hierarchy(ctx0, mesh, coarsest=2)
    ctx0.poisson_set_fast_diag(factors)
    _run(ctx0, dm, IMEXType.SBDF2, nsteps, k, True, True, ref, 0, fd=True)
    ctx0.close()
    parts = [StripPartition((0.0, 0.0), (1.0, 1.0), n, n, r, size, coarsest=2) for r in range(size)]

    def work(r, part, ctx, out):
        part.attach(ctx)
        ctx.mg_set_halo_mode(relaxed)
        ctx.poisson_set_fast_diag(factors, first_line=int(part.p1_global[0]) // (n + 1))
        _run(ctx, part.dofmap, IMEXType.SBDF2, nsteps, k, True, True, out, r, fd=True)

    out = _on_ranks(parts, work)
    for r in range(size):
        for a, b in zip(out[r]["infos"], ref[0]["infos"]):
            assert a.krylov_iterations_poisson == b.krylov_iterations_poisson == 1
        assert out[r]["imex"]["path"] == "lattice-kernel" and out[r]["imex"]["generic_rhs"] == 0
    _compare(parts, out, ref[0], relaxed)


def test_graded_strips_take_the_generic_path_on_every_rank():
    """a graded lattice: "generic" on every rank, the fields still match the single context, and the one-launch
    right-hand side is refused on every rank"""
    n, size, nsteps, k = 32, 2, 3, 0.01
    mesh, dm, _ = box(n, n)
    _grade(mesh)
    dm = TaylorHoodDofMap(mesh)
    ref = {}
    ctx0 = context(mesh, dm)
    _run(ctx0, dm, IMEXType.SBDF2, nsteps, k, False, False, ref, 0)
    assert ctx0.imex_info()["path"] == "generic"
    ctx0.close()
    parts = [StripPartition((0.0, 0.0), (1.0, 1.0), n, n, r, size) for r in range(size)]
    for part in parts:
        _grade(part.mesh)
        part.dofmap = TaylorHoodDofMap(part.mesh, reorder=True)

    def work(r, part, ctx, out):
        _plain_partition(ctx, part, r, size, n, n)
        _run(ctx, part.dofmap, IMEXType.SBDF2, nsteps, k, False, False, out, r)
        with pytest.raises(nat.NativeError, match="not available"):
            ctx.imex_rhs("lattice-kernel", 0)

    out = _on_ranks(parts, work)
    for r in range(size):
        info = out[r]["imex"]
        assert info["path"] == "generic" and info["generic_rhs"] == nsteps and info["lattice_rhs"] == 0, (r, info)
    _compare(parts, out, ref[0], False)


def test_rotating_frame_is_refused_on_every_rank_before_any_collective():
    n, size = 16, 2
    parts = [StripPartition((0.0, 0.0), (1.0, 1.0), n, n, r, size) for r in range(size)]

    def work(r, part, ctx, out):
        _plain_partition(ctx, part, r, size, n, n)
        ctx.set_coeffs(1.0, 1.0, 0.01, None, 1.0, 1.0)
        ctx.set_dirichlet(nat.VELOCITY, *_cavity_bc(part.dofmap))
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        ctx.set_imex((1.0, -1.0, 0.0), (1.0, 0.0), (1.0, 0.0, 0.0), 1.0 / 32.0)
        ctx.set_angular_velocity(0.5, 0.0)
        before = ctx.comm_stats()
        with pytest.raises(nat.NativeError, match="rotating"):
            ctx.step_imex()
        with pytest.raises(nat.NativeError, match="rotating"):
            ctx.imex_rhs("generic", 0)
        out[r] = (before, ctx.comm_stats())

    out = _on_ranks(parts, work)
    for r in range(size):
        assert out[r][0] == out[r][1]


def test_message_counts_of_an_imex_step_on_eight_ranks():
    """BASELINE's strong-scaling mesh (960 x 960) on 8 thread ranks with the settings of
    test_message_counts_of_a_strong_scaling_step_on_eight_ranks (relaxed halo mode, levels thinner than 16 cell rows per
    rank replicated, fast-diagonalisation projection, Chebyshev mass solve), scripts/imex_strip_message_counts.py:
    measured 72.8 halo exchanges and 17.0 all-reduces per IMEX step (IPCS beside it: 80.8 and 31.0).  Pinned with that
    test's margin (about 5 % over the measurement) so that later changes cannot silently add messages.  (Spacing 1 / 960
    is not a binary fraction: the strips are not bit-uniform lattices and every rank takes the generic right-hand side --
    one exchange, as the one-launch path.)"""
    cmd = [sys.executable, os.path.join(ROOT, "scripts", "imex_strip_message_counts.py"), "--cells", "960", "--ranks", "8",
           "--schemes", "imex", "--json"]
    res = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stderr[-3000:]
    row = json.loads([l for l in res.stdout.strip().splitlines() if l.startswith("{")][-1])
    comm = row["per_step_rank0"]
    print("\n[imex 960^2, 8 ranks] per step: %.1f halo exchanges, %.1f all-reduces; cg %.2f" % (
        comm["exchanges"], comm["allreduce_calls"], comm["momentum_its"]))
    assert comm["exchanges"] <= 76.5 and comm["allreduce_calls"] <= 18          # (measured: 72.8 and 17.0)
    assert comm["newton_its"] == 0 and comm["momentum_its"] <= 5.5 and comm["poisson_its"] == 1.0


# ---------------------------------------------------------------- 3D
def _bc3(dmap):
    X = dmap.p2_coords
    on = np.zeros(dmap.n_p2, dtype=bool)
    for a in range(3):
        on |= (np.abs(X[:, a]) < 1e-12) | (np.abs(X[:, a] - 1.0) < 1e-12)
    nodes = np.nonzero(on)[0]
    ux = np.where(np.abs(X[nodes, 2] - 1.0) < 1e-12, 1.0, 0.0)
    return (np.concatenate([3 * nodes, 3 * nodes + 1, 3 * nodes + 2]).astype(np.int32),
            np.concatenate([ux, np.zeros(2 * nodes.size)]))


def test_imex_3d_steps_match_restatement():
    """single context, unit cube n = 4, lid-driven cavity, SBDF2, 3 steps, LU-accuracy Krylov tolerances: the generic
    right-hand-side path in 3D against IMEXRestatement (u*, u 1e-9, p minus its mean 1e-8, relative)"""
    from fem_mesh import box_mesh
    n, k = 4, 0.05
    mesh = box_mesh((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), n, n, n)
    dm = TaylorHoodDofMap(mesh)
    s = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
    vbc = _bc3(dm)
    order = np.argsort(vbc[0])
    vbc = (vbc[0][order], vbc[1][order])
    ctx = context(mesh, dm)
    try:
        ctx.set_coeffs(1.0, 1.0, 0.01)
        ctx.set_dirichlet(nat.VELOCITY, *vbc)
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        orc = IMEXRestatement(s, dict(convective_term=1.0, pressure_term=1.0, viscous_term=0.01), "standard")
        opts = ctx.default_step_opts()
        for o in (opts.momentum, opts.poisson, opts.correction):
            o.rtol = 1e-13
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=k)
        for step in range(3):
            ts.update_coefficients()
            kk = ts.get_next_step_size()
            ctx.set_imex(ts.alpha, ts.beta, ts.gamma, kk)
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
        info = ctx.imex_info()
        assert info["path"] == "generic" and info["generic_rhs"] == 3 and info["lattice_rhs"] == 0
    finally:
        ctx.close()


def test_partitioned_imex_3d_slabs_equal_single_context():
    """the cavity on two slabs of cube layers (SlabPartition, replicated global tail) against the single context:
    tolerances of test_partitioned_3d_slabs_equal_single_context (u 1e-10, p minus its mean 1e-9, equal CG counts)"""
    from fem_mesh import box_mesh
    from partition import SlabPartition
    n, size, nsteps, k = 8, 2, 2, 0.02
    mesh = box_mesh((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), n, n, n)
    dm = TaylorHoodDofMap(mesh)

    def run(ctx, dmap, out, key):
        ctx.set_coeffs(1.0, 1.0, 0.02)
        ctx.set_dirichlet(nat.VELOCITY, *_bc3(dmap))
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        opts = ctx.default_step_opts()
        for o in (opts.momentum, opts.poisson, opts.correction):
            o.rtol = 1e-12
        opts.momentum.precond = opts.poisson.precond = 1
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=k)
        infos = []
        for _ in range(nsteps):
            ts.update_coefficients()
            ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
            infos.append(ctx.step_imex(opts))
            ctx.advance(0)
            ts.advance_time()
        out[key] = dict(u=ctx.get_state(nat.U1), p=ctx.get_state(nat.P_OLD), infos=infos, imex=ctx.imex_info())

    ref = {}
    ctx0 = context(mesh, dm)
    attach_hierarchy(ctx0, mesh, coarsest=2)
    run(ctx0, dm, ref, 0)
    ctx0.close()
    ref = ref[0]
    parts = [SlabPartition((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), n, n, n, r, size, coarsest=4, global_coarsest=2)
             for r in range(size)]

    def work(r, part, ctx, out):
        part.attach(ctx)
        run(ctx, part.dofmap, out, r)

    out = _on_ranks(parts, work)
    u = np.zeros_like(ref["u"])
    p = np.zeros_like(ref["p"])
    for r, part in enumerate(parts):
        o = out[r]
        u.reshape(-1, 3)[part.p2_global[part.p2_owned]] = o["u"].reshape(-1, 3)[part.p2_owned]
        p[part.p1_global[part.p1_owned]] = o["p"][part.p1_owned]
        assert o["imex"]["path"] == "generic"
        for a, b in zip(o["infos"], ref["infos"]):
            assert a.newton_iterations == b.newton_iterations == 0
            assert a.krylov_iterations_momentum == b.krylov_iterations_momentum
            assert a.krylov_iterations_poisson == b.krylov_iterations_poisson
    eu, ep = rel(u, ref["u"]), rel(p - p.mean(), ref["p"] - ref["p"].mean())
    print("3D slabs: u %.2e p %.2e" % (eu, ep))
    assert eu < 1e-10 and ep < 1e-9
