"""Fast diagonalisation on partitioned 3D slabs (FastDiag3::apply_slab in csrc/fastdiag.hip,
nsfem_poisson_set_fast_diag_3d_planes, partition.*SlabPartition.attach_fast_diag), in-process thread ranks on one GPU:
the slab solve against the one-rank formula on every rank's local planes, ghost planes included; the projection step
of periodic slabs (one direct pass) and of closed-cavity slabs (CG preconditioned by the slab T^+) against a single
context running the one-rank 3D solve; and the refusals of the new setter."""
import os
import threading

import numpy as np
import pytest

import _native as nat
import poisson_fd as pf
from gpu_common import context, rel
from partition import GHOST, PeriodicSlabPartition, SlabPartition, global_dof_counts
from test_gpu_fast_diag_3d import _random_factors_3d, _reference_3d

pytestmark = pytest.mark.gpu
LO, HI = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)


def _on_ranks(size, fn):
    """fn(rank) on ``size`` threads -> {rank: result}; a dead rank would deadlock the others"""
    out, errors = {}, []

    def worker(r):
        try:
            out[r] = fn(r)
        except BaseException as exc:
            import sys
            import traceback
            traceback.print_exc()
            sys.stderr.flush()
            errors.append((r, repr(exc)))
            os._exit(17)

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(size)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    return out


def _parts(periodic, n, size, **kw):
    cls = PeriodicSlabPartition if periodic else SlabPartition
    return [cls(LO, HI, *n, r, size, **kw) for r in range(size)]


def _contexts(parts, group):
    ctxs = []
    for r, part in enumerate(parts):
        d = part.dofmap
        c = nat.NsfemContext(part.mesh.coords, part.mesh.cells, d.p2_dofmap, d.p1_dofmap, d.n_p2, d.n_p1)
        if group is not None:
            c.attach_local_comm(group, r)
        ctxs.append(c)
    return ctxs


def _set_partition(ctx, part, p1_ghost=None):
    """the partition data of part.attach without the multigrid hierarchy"""
    g1 = part.p1_ghost if p1_ghost is None else p1_ghost
    if isinstance(part, PeriodicSlabPartition):
        ctx.set_partition(part.rank, part.size, part.p2_ghost, g1, part.p2_halo, part.p1_halo,
                          part.n_p2_global, part.n_p1_global, periodic=True)
    else:
        n2g, n1g = global_dof_counts(part.nx, part.ny, part.nz)
        ctx.set_partition(part.rank, part.size, part.p2_ghost, g1, part.p2_halo, part.p1_halo, n2g, n1g)


def _local_planes(part, Nz, plane):
    return np.asarray(part.p1_global[::plane]) // plane % Nz


# ---------------------------------------------------------------------------------------------------------------------
# the slab solve through the test hook
# ---------------------------------------------------------------------------------------------------------------------
# (periodic, cells per direction, ranks): the lattice is (n + 1)^3 without, n^3 with periodicity; N_z = 197 and 200
# make the z expansion's K three k-blocks of 96 with a ragged tail
APPLY = [(True, (8, 8, 8), 2), (False, (5, 4, 12), 2), (False, (5, 4, 12), 3), (False, (5, 4, 12), 4),
         (True, (6, 5, 12), 3), (True, (6, 5, 12), 4), (True, (4, 4, 200), 4), (False, (3, 3, 196), 4)]


@pytest.mark.parametrize("periodic,n,size", APPLY)
def test_slab_solve_equals_the_one_rank_formula_on_every_local_plane(periodic, n, size):
    """mg_apply(2) on every rank (a collective) with random non-symmetric factors: the local planes, ghost planes
    included, equal the one-rank formula's (long double) to the tolerance of the one-rank mode-product tests.  Ghost
    entries of r filled with 1e30 leave the result bit for bit unchanged: only owned planes enter the contraction."""
    Nx, Ny, Nz = (n[0], n[1], n[2]) if periodic else (n[0] + 1, n[1] + 1, n[2] + 1)
    plane = Nx * Ny
    f, r = _random_factors_3d(Nx, Ny, Nz, 7919 * Nx + 131 * Ny + Nz + size)
    ref = _reference_3d(f, r, np.longdouble).astype(np.float64).reshape(Nz, plane)
    R = r.reshape(Nz, plane)
    parts = _parts(periodic, n, size, coarsest=64)
    group = nat.local_group_create(size)
    ctxs = _contexts(parts, group)
    for ctx, part in zip(ctxs, parts):
        _set_partition(ctx, part)

    def rank(k):
        ctx, part = ctxs[k], parts[k]
        first = int(part.p1_global[0]) // plane
        ctx.poisson_set_fast_diag_3d(f, first_plane=first)
        planes = _local_planes(part, Nz, plane)
        r_loc = R[planes].ravel()
        z = ctx.mg_apply(2, r_loc)
        r_bad = r_loc.copy()
        r_bad[part.p1_ghost != 0] = 1e30
        z_bad = ctx.mg_apply(2, r_bad)
        return planes, z, z_bad, ctx.poisson_fast_diag_3d_info()

    out = _on_ranks(size, rank)
    for c in ctxs:
        c.close()
    nat.local_group_destroy(group)
    covered = np.zeros(Nz, dtype=bool)
    for k in range(size):
        planes, z, z_bad, info = out[k]
        err = rel(z, ref[planes].ravel())
        assert err <= 1e-13, (k, err)
        assert np.array_equal(z_bad, z), k
        assert info["shape"] == (Nx, Ny, Nz) and info["applications"] == 2
        covered[planes] = True
        if periodic and k == size - 1:
            assert list(planes[-2:]) == [0, 1]                 # the last rank wraps around
    assert covered.all()


# ---------------------------------------------------------------------------------------------------------------------
# projection step: triple-periodic Taylor-Green (exact factors, one direct pass)
# ---------------------------------------------------------------------------------------------------------------------
G = 2.0 * np.pi
NSTEPS, K = 3, 0.02


def _tg_fields(dmap):
    X, Y = dmap.p2_coords, dmap.p1_coords
    u = np.stack([np.cos(G * X[:, 0]) * np.sin(G * X[:, 1]), -np.sin(G * X[:, 0]) * np.cos(G * X[:, 1]),
                  0.3 * np.sin(G * X[:, 2]) * np.cos(G * X[:, 0])], axis=1).ravel()
    return u, -0.25 * (np.cos(2 * G * Y[:, 0]) + np.cos(2 * G * Y[:, 1]))


def _opts(ctx, fd):
    o = ctx.default_step_opts()
    for k in (o.momentum, o.poisson, o.correction):
        k.rtol = 1e-12
    o.momentum.precond = 1
    o.poisson.precond = 3 if fd else 1
    o.correction.precond = 2
    return o


def _steps(ctx, opts):
    ctx.comm_stats(reset=True)
    infos = []
    for step in range(NSTEPS):
        ctx.set_bdf((1.0, -1.0, 0.0) if step == 0 else (1.5, -2.0, 0.5), K)
        infos.append(ctx.step_ipcs(opts))
        ctx.advance(0)
    return ctx.get_state(nat.U1), ctx.get_state(nat.P_OLD), infos, ctx.comm_stats(), ctx.poisson_fast_diag_3d_info()


def _tg_start(ctx, dmap, coef=0.02):
    u0, p0 = _tg_fields(dmap)
    for slot in (nat.U0, nat.U1, nat.U2):
        ctx.set_state(slot, u0)
    for slot in (nat.P, nat.P_OLD):
        ctx.set_state(slot, p0)
    ctx.set_coeffs(1.0, 1.0, coef)
    ctx.set_dirichlet(nat.VELOCITY, np.zeros(0, np.int32), np.zeros(0))
    ctx.set_dirichlet(nat.PRESSURE, np.zeros(0, np.int32), np.zeros(0))


@pytest.mark.parametrize("n,size,relaxed", [(8, 2, False), (8, 4, False), (16, 2, False), (16, 4, False),
                                            (8, 2, True), (8, 4, True), (16, 2, True), (16, 4, True)])
def test_periodic_slabs_direct_step_equals_the_single_context(n, size, relaxed):
    """PeriodicSlabPartition with attach_fast_diag, precond = 3: one Poisson pass per step on every rank, the fields of
    a single context running the one-rank 3D solve (velocity 1e-11 / 1e-9, mean-free pressure 1e-10 / 1e-8 in exact /
    relaxed halo mode), ghost planes of the pressure equal to the owners' values, and fewer halo exchanges and fewer
    all-reduces per step than the same partitioned run with multigrid-CG."""
    from fem_mesh import TaylorHoodDofMap, box_mesh, periodic_entity_map
    from multigrid import attach_hierarchy
    from test_gpu_fast_diag_3d import _TriplePeriodic

    mesh = box_mesh(LO, HI, n, n, n)
    domain = _TriplePeriodic((1.0, 1.0, 1.0)).domain
    dm = TaylorHoodDofMap(mesh, periodic_map=periodic_entity_map(mesh, domain))
    xs, ys, zs, per = pf.box_lattice(mesh, dm)
    assert per == (True, True, True)
    ctx0 = context(mesh, dm)
    attach_hierarchy(ctx0, mesh, coarsest=2, periodic=(domain, dm.p1_vertex_node))
    ctx0.poisson_set_fast_diag_3d(pf.factors_3d(xs, ys, zs, per))
    _tg_start(ctx0, dm)
    u_ref, p_ref, inf_ref, _, info0 = _steps(ctx0, _opts(ctx0, True))
    ctx0.close()
    assert info0["exact"] and info0["solves"] == NSTEPS

    results = {}
    for fd in (True, False):
        parts = _parts(True, (n, n, n), size, coarsest=2)
        group = nat.local_group_create(size)
        ctxs = _contexts(parts, group)

        def rank(r):
            parts[r].attach(ctxs[r])
            ctxs[r].mg_set_halo_mode(relaxed)
            if fd:
                assert parts[r].attach_fast_diag(ctxs[r])
            _tg_start(ctxs[r], parts[r].dofmap)
            return _steps(ctxs[r], _opts(ctxs[r], fd))

        results[fd] = (parts, _on_ranks(size, rank))
        for c in ctxs:
            c.close()
        nat.local_group_destroy(group)

    parts, out = results[True]
    key = lambda X: [tuple(r) for r in (np.round(X * 4 * n).astype(np.int64) % (4 * n))]
    ref2 = {kk: i for i, kk in enumerate(key(dm.p2_coords))}
    ref1 = {kk: i for i, kk in enumerate(key(dm.p1_coords))}
    u = np.full_like(u_ref, np.nan)
    p = np.full_like(p_ref, np.nan)
    for r, part in enumerate(parts):
        ul, pl, infos, _, info = out[r]
        own2, own1 = np.nonzero(part.p2_owned)[0], np.nonzero(part.p1_owned)[0]
        i2 = np.array([ref2[kk] for kk in key(part.dofmap.p2_coords[own2])])
        i1 = np.array([ref1[kk] for kk in key(part.dofmap.p1_coords[own1])])
        u.reshape(-1, 3)[i2] = ul.reshape(-1, 3)[own2]
        p[i1] = pl[own1]
        assert [i.krylov_iterations_poisson for i in infos] == [1] * NSTEPS, (r, infos)
        assert info["exact"] and info["solves"] == NSTEPS and info["shape"] == (n, n, n)
        for a, b in zip(infos, inf_ref):
            assert a.newton_iterations == b.newton_iterations
    assert np.isfinite(u).all() and np.isfinite(p).all()
    assert rel(u, u_ref) < (1e-9 if relaxed else 1e-11)
    assert rel(p - p.mean(), p_ref - p_ref.mean()) < (1e-8 if relaxed else 1e-10)
    for r, part in enumerate(parts):                          # ghost planes: copies of the owners' values
        pl = out[r][1]
        i1 = np.array([ref1[kk] for kk in key(part.dofmap.p1_coords)])
        assert np.abs(pl - p[i1]).max() <= 1e-12 * max(1.0, np.abs(p).max()), r
    st_fd, st_mg = results[True][1][0][3], results[False][1][0][3]
    print("\n[n = %d, %d ranks, %s] per step: exchanges %.1f -> %.1f, all-reduces %.1f -> %.1f" % (
        n, size, "relaxed" if relaxed else "exact", st_mg["exchanges"] / NSTEPS, st_fd["exchanges"] / NSTEPS,
        st_mg["allreduce_calls"] / NSTEPS, st_fd["allreduce_calls"] / NSTEPS))
    assert st_fd["exchanges"] < st_mg["exchanges"] and st_fd["allreduce_calls"] < st_mg["allreduce_calls"]


def test_refinement_passes_on_periodic_slabs_equal_the_single_context():
    """poisson_direct_step on two periodic slabs with perturbed factors (inv * (1 + DELTA) on every rank; constants
    and derivation of test_gpu_fast_diag: SIX passes per step at rtol = 3e-11, atol = 0): the same pass count on every
    rank as on the single context, and the same fields to 1e-10, as the strip counterpart
    test_refinement_passes_on_strips_equal_the_single_context asks.  The target is rtol |r| with |r|^2 all-reduced
    once: reducing it again in every pass would multiply it by the rank count each time and stop the slabs early."""
    from fem_mesh import TaylorHoodDofMap, box_mesh, periodic_entity_map
    from multigrid import attach_hierarchy
    from test_gpu_fast_diag import DELTA, PASSES, RTOL
    from test_gpu_fast_diag_3d import _TriplePeriodic
    n, size = 8, 2
    mesh = box_mesh(LO, HI, n, n, n)
    domain = _TriplePeriodic((1.0, 1.0, 1.0)).domain
    dm = TaylorHoodDofMap(mesh, periodic_map=periodic_entity_map(mesh, domain))
    f = pf.factors_3d(*pf.box_lattice(mesh, dm))
    assert f["exact"] and f["inv"].shape == (n, n, n)
    f = dict(f, inv=f["inv"] * (1.0 + DELTA))

    def opts(ctx):
        o = _opts(ctx, True)
        o.poisson.rtol = RTOL
        o.poisson.atol = 0.0
        return o

    ctx0 = context(mesh, dm)
    attach_hierarchy(ctx0, mesh, coarsest=2, periodic=(domain, dm.p1_vertex_node))
    ctx0.poisson_set_fast_diag_3d(f)
    _tg_start(ctx0, dm)
    u_ref, p_ref, inf_ref, _, info0 = _steps(ctx0, opts(ctx0))
    ctx0.close()
    passes_ref = [i.krylov_iterations_poisson for i in inf_ref]
    print("single context: passes", passes_ref, "applications", info0["applications"])
    assert passes_ref == [PASSES] * NSTEPS
    assert info0["solves"] == NSTEPS and info0["applications"] == PASSES * NSTEPS

    parts = _parts(True, (n, n, n), size, coarsest=2)
    group = nat.local_group_create(size)
    ctxs = _contexts(parts, group)

    def rank(r):
        parts[r].attach(ctxs[r])
        ctxs[r].poisson_set_fast_diag_3d(f, first_plane=int(parts[r].p1_global[0]) // (n * n))
        _tg_start(ctxs[r], parts[r].dofmap)
        return _steps(ctxs[r], opts(ctxs[r]))

    out = _on_ranks(size, rank)
    for c in ctxs:
        c.close()
    nat.local_group_destroy(group)
    key = lambda X: [tuple(r) for r in (np.round(X * 4 * n).astype(np.int64) % (4 * n))]
    ref2 = {kk: i for i, kk in enumerate(key(dm.p2_coords))}
    ref1 = {kk: i for i, kk in enumerate(key(dm.p1_coords))}
    u = np.full_like(u_ref, np.nan)
    p = np.full_like(p_ref, np.nan)
    for r, part in enumerate(parts):
        ul, pl, infos, _, info = out[r]
        own2, own1 = np.nonzero(part.p2_owned)[0], np.nonzero(part.p1_owned)[0]
        u.reshape(-1, 3)[[ref2[kk] for kk in key(part.dofmap.p2_coords[own2])]] = ul.reshape(-1, 3)[own2]
        p[[ref1[kk] for kk in key(part.dofmap.p1_coords[own1])]] = pl[own1]
        passes = [i.krylov_iterations_poisson for i in infos]
        print("rank", r, "passes", passes, "applications", info["applications"])
        assert passes == passes_ref, (r, passes, passes_ref)
        assert info["solves"] == NSTEPS and info["applications"] == PASSES * NSTEPS
    assert np.isfinite(u).all() and np.isfinite(p).all()
    eu, ep = rel(u, u_ref), rel(p - p.mean(), p_ref - p_ref.mean())
    print("velocity", eu, "pressure", ep)
    assert eu < 1e-10 and ep < 1e-10, (eu, ep)


# ---------------------------------------------------------------------------------------------------------------------
# projection step: closed cavity (inexact factors, CG preconditioned by the slab T^+)
# ---------------------------------------------------------------------------------------------------------------------
def _cavity_bc(dmap):
    X = dmap.p2_coords
    on = np.zeros(dmap.n_p2, dtype=bool)
    for a in range(3):
        on |= (np.abs(X[:, a]) < 1e-12) | (np.abs(X[:, a] - 1.0) < 1e-12)
    nodes = np.nonzero(on)[0]
    ux = np.where(np.abs(X[nodes, 2] - 1.0) < 1e-12, 1.0, 0.0)
    return (np.concatenate([3 * nodes, 3 * nodes + 1, 3 * nodes + 2]).astype(np.int32),
            np.concatenate([ux, np.zeros(2 * nodes.size)]))


def _cavity_start(ctx, dmap):
    ctx.set_coeffs(1.0, 1.0, 0.02)
    ctx.set_dirichlet(nat.VELOCITY, *_cavity_bc(dmap))
    ctx.set_dirichlet(nat.PRESSURE, np.zeros(0, np.int32), np.zeros(0))


@pytest.mark.parametrize("size", [2, 3])
def test_cavity_slabs_run_cg_preconditioned_by_the_slab_solve(size):
    """SlabPartition with attach_fast_diag (inexact factors: free box edges), precond = 3: the assembled projection
    system runs CG with the slab T^+ as its preconditioner; the fields equal a single context running CG preconditioned
    by the one-rank 3D solve (velocity 1e-11, mean-free pressure 1e-10) and the Poisson iteration counts agree to
    within one."""
    from fem_mesh import TaylorHoodDofMap, box_mesh
    from multigrid import attach_hierarchy
    n = 6
    mesh = box_mesh(LO, HI, n, n, n)
    dm = TaylorHoodDofMap(mesh)
    xs, ys, zs, per = pf.box_lattice(mesh, dm)
    ctx0 = context(mesh, dm)
    attach_hierarchy(ctx0, mesh, coarsest=2)
    f0 = pf.factors_3d(xs, ys, zs, per)
    assert not f0["exact"]
    ctx0.poisson_set_fast_diag_3d(f0)
    _cavity_start(ctx0, dm)
    u_ref, p_ref, inf_ref, _, info0 = _steps(ctx0, _opts(ctx0, True))
    ctx0.close()
    assert not info0["exact"] and info0["solves"] == NSTEPS

    parts = _parts(False, (n, n, n), size, coarsest=2)
    group = nat.local_group_create(size)
    ctxs = _contexts(parts, group)

    def rank(r):
        parts[r].attach(ctxs[r])
        assert not parts[r].attach_fast_diag(ctxs[r])
        _cavity_start(ctxs[r], parts[r].dofmap)
        return _steps(ctxs[r], _opts(ctxs[r], True))

    out = _on_ranks(size, rank)
    for c in ctxs:
        c.close()
    nat.local_group_destroy(group)
    u = np.zeros_like(u_ref)
    p = np.zeros_like(p_ref)
    for r, part in enumerate(parts):
        ul, pl, infos, _, info = out[r]
        u.reshape(-1, 3)[part.p2_global[part.p2_owned]] = ul.reshape(-1, 3)[part.p2_owned]
        p[part.p1_global[part.p1_owned]] = pl[part.p1_owned]
        assert not info["exact"] and info["solves"] == NSTEPS and info["applications"] > 0
        for a, b in zip(infos, inf_ref):
            assert a.newton_iterations == b.newton_iterations
            assert abs(a.krylov_iterations_poisson - b.krylov_iterations_poisson) <= 1, (r, a, b)
            assert a.krylov_iterations_poisson > 1
    assert rel(u, u_ref) < 1e-11
    assert rel(p - p.mean(), p_ref - p_ref.mean()) < 1e-10


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_slab_setter_refusals():
    """nsfem_poisson_set_fast_diag_3d_planes refuses (NSFEM_ERR_ARG) a context that is not partitioned or has no
    communicator, a local space that is not whole planes of Nx x Ny, Nx Ny Nz != the global P1 count, owned dofs that
    are not one contiguous run of whole planes, and planes that wrap around on a non-periodic partition"""
    from test_gpu_fast_diag_3d import _lattice_context
    n = (3, 3, 4)                                    # lattice 4 x 4 x 5, two ranks of two cube layers
    Nx, Ny, Nz = 4, 4, 5
    f, _ = _random_factors_3d(Nx, Ny, Nz, 3)
    plain = _lattice_context(Nx, Ny, Nz)
    with pytest.raises(nat.NativeError, match="partitioned context"):
        plain.poisson_set_fast_diag_3d(f, first_plane=0)
    plain.close()
    parts = _parts(False, n, 2, coarsest=64)
    lone = _contexts(parts, None)                    # partition data, no communicator
    for c, part in zip(lone, parts):
        _set_partition(c, part)
        with pytest.raises(nat.NativeError, match="communicator"):
            c.poisson_set_fast_diag_3d(f, first_plane=0)
        c.close()

    group = nat.local_group_create(2)
    ctxs = _contexts(parts, group)
    try:
        for c, part in zip(ctxs, parts):
            _set_partition(c, part)
        c, part = ctxs[1], parts[1]
        first = int(part.p1_global[0]) // (Nx * Ny)
        assert first == 2 and c.n_p1 == 3 * Nx * Ny
        g, _ = _random_factors_3d(Nx + 1, Ny, Nz, 4)
        with pytest.raises(nat.NativeError, match="whole lattice planes"):
            c.poisson_set_fast_diag_3d(g, first_plane=first)
        g, _ = _random_factors_3d(Nx, Ny, Nz + 1, 5)
        with pytest.raises(nat.NativeError, match="global number of pressure dofs"):
            c.poisson_set_fast_diag_3d(g, first_plane=first)
        with pytest.raises(nat.NativeError, match="wrap around"):
            c.poisson_set_fast_diag_3d(f, first_plane=first + 1)
        assert c.poisson_fast_diag_3d_info()["shape"] == (0, 0, 0)
        c.poisson_set_fast_diag_3d(f, first_plane=first)
        assert c.poisson_fast_diag_3d_info()["shape"] == (Nx, Ny, Nz)
    finally:
        for c in ctxs:
            c.close()
        nat.local_group_destroy(group)

    # owned dofs that are not whole planes / not one run (rank 0: owned planes 0, 1, 2, ghost plane 3)
    for bad in ("half plane", "gap"):
        group = nat.local_group_create(2)
        ctxs = _contexts(parts, group)
        try:
            g1 = parts[0].p1_ghost.copy()
            assert list(g1.reshape(4, Nx * Ny)[:, 0]) == [0, 0, 0, GHOST]
            if bad == "half plane":
                g1[Nx * Ny: Nx * Ny + Nx * Ny // 2] = GHOST
            else:
                g1[Nx * Ny: 2 * Nx * Ny] = GHOST
            _set_partition(ctxs[0], parts[0], g1)
            with pytest.raises(nat.NativeError, match="contiguous run of whole lattice planes"):
                ctxs[0].poisson_set_fast_diag_3d(f, first_plane=0)
        finally:
            for c in ctxs:
                c.close()
            nat.local_group_destroy(group)


def test_pressure_dirichlet_nodes_on_slabs_are_refused():
    """precond = 3 with pressure Dirichlet nodes on slab factors: the existing refusal of the partitioned projection
    step (every rank owns nodes of the face x = 0, so every rank raises the same error)"""
    n, size = (4, 4, 4), 2
    parts = _parts(False, n, size, coarsest=2)
    group = nat.local_group_create(size)
    ctxs = _contexts(parts, group)

    def rank(r):
        ctx, part = ctxs[r], parts[r]
        part.attach(ctx)
        part.attach_fast_diag(ctx)
        _cavity_start(ctx, part.dofmap)
        face = np.nonzero((np.abs(part.dofmap.p1_coords[:, 0]) < 1e-12) & part.p1_owned)[0].astype(np.int32)
        assert face.size > 0
        ctx.set_dirichlet(nat.PRESSURE, face, np.zeros(face.size))
        ctx.set_bdf((1.0, -1.0, 0.0), K)
        try:
            ctx.step_ipcs(_opts(ctx, True))
        except nat.NativeError as exc:
            return str(exc)
        return None

    out = _on_ranks(size, rank)
    for c in ctxs:
        c.close()
    nat.local_group_destroy(group)
    assert all(out[r] is not None and "pure Neumann projection step only" in out[r] for r in range(size)), out


def test_pressure_dirichlet_nodes_on_slabs_are_refused_by_the_imex_step():
    """the same refusal from step_imex (it shares the projection step with step_ipcs): every rank raises it before the
    Poisson system is assembled, and the pressure slot keeps its bits"""
    n, size = (4, 4, 4), 2
    parts = _parts(False, n, size, coarsest=2)
    group = nat.local_group_create(size)
    ctxs = _contexts(parts, group)

    def rank(r):
        ctx, part = ctxs[r], parts[r]
        part.attach(ctx)
        part.attach_fast_diag(ctx)
        _cavity_start(ctx, part.dofmap)
        face = np.nonzero((np.abs(part.dofmap.p1_coords[:, 0]) < 1e-12) & part.p1_owned)[0].astype(np.int32)
        assert face.size > 0
        ctx.set_dirichlet(nat.PRESSURE, face, np.zeros(face.size))
        ctx.set_imex((1.0, -1.0, 0.0), (1.0, 0.0), (1.0, 0.0, 0.0), K)
        ctx.set_state(nat.P, np.sin(part.dofmap.p1_coords @ np.array([1.0, 2.0, 3.0])))
        before = ctx.get_state(nat.P)
        try:
            ctx.step_imex(_opts(ctx, True))
        except nat.NativeError as exc:
            return str(exc), before, ctx.get_state(nat.P)
        return None

    out = _on_ranks(size, rank)
    for c in ctxs:
        c.close()
    nat.local_group_destroy(group)
    for r in range(size):
        assert out[r] is not None, r
        msg, before, after = out[r]
        assert "pure Neumann projection step only" in msg, (r, msg)
        assert before.any() and np.array_equal(before.view(np.uint64), after.view(np.uint64)), r

