"""Shared by the partitioned-cycle tests (tests/test_partitioned_cycle_host.py, tests/test_gpu_partitioned_cycle.py,
tests/test_gpu_partitioned_operators.py); a plain helper module like gpu_common.py.

Host side: the partitions the GPU tests run (`CASES`), their global meshes, Dirichlet sets, host cycles (serial
HostCycle for the exact halo mode, PartitionedCycle for the relaxed one), the references with the rounding measure d
and the device's bound.  Device side: `run_ranks`, the thread-rank scaffolding of tests/test_gpu_partition.py -- one
context per rank in one process, one host thread per rank on the in-process communicator; a rank that raises ends the
process (os._exit(17)), because the other ranks would wait for it for ever."""
import functools
import os
import threading

import numpy as np

import mg_cycle_host as mh

NU = 0.01
BDF2 = (1.5, -2.0, 0.5)
STEP = 0.01                                    # velocity operator 150 M + 0.01 K
SYSTEMS = ("pressure neumann", "pressure outlet side", "pressure outlet top", "velocity")
# name -> (kind, upper corner, cells, ranks, coarsest, global_coarsest)
CASES = {
    "box32/2": ("strip", (1.0, 1.0), (32, 32), 2, 2, None),
    "box64/4 tail": ("strip", (1.0, 1.0), (64, 64), 4, 16, 2),
    "box48/3": ("strip", (1.0, 1.0), (48, 48), 3, 3, None),
    "box64x32/2": ("strip", (2.0, 1.0), (64, 32), 2, 2, None),
    "box64/8 tail": ("strip", (1.0, 1.0), (64, 64), 8, 16, 2),
    "cube8/2": ("slab", (1.0, 1.0, 1.0), (8, 8, 8), 2, 2, None),
}
# host only (tests/test_partitioned_cycle_host.py: what kind of preconditioner the relaxed cycle is)
SMALL_CASES = {
    "box16/2": ("strip", (1.0, 1.0), (16, 16), 2, 2, None),
    "box16/4": ("strip", (1.0, 1.0), (16, 16), 4, 2, None),
}
DICT_EXTRA = {"box48/3": 2.0 ** -38}           # h = 1/48: the stencil dictionary equals the matrices to 2^-40 only


def which_of(system):
    return 1 if system == "velocity" else 0


class Case:
    """one partition of CASES: the ranks' partition objects, the global mesh and its host hierarchy"""

    def __init__(self, name):
        from fem_mesh import TaylorHoodDofMap, box_mesh, rectangle_mesh
        from multigrid import structured_hierarchy
        from partition import SlabPartition, StripPartition
        kind, hi, cells, size, coarsest, tail = {**CASES, **SMALL_CASES}[name]
        self.name, self.size, self.dim, self.hi = name, size, len(cells), hi
        lo = (0.0,) * self.dim
        make = StripPartition if kind == "strip" else SlabPartition
        self.parts = [make(lo, hi, *cells, r, size, coarsest=coarsest, global_coarsest=tail) for r in range(size)]
        self.mesh = rectangle_mesh(lo, hi, *cells) if self.dim == 2 else box_mesh(lo, hi, *cells)
        self.dm = TaylorHoodDofMap(self.mesh)
        self.levels = structured_hierarchy(lo, hi, *cells, coarsest=coarsest if tail is None else tail)
        self.n_part = 1 + len(self.parts[0].levels)            # partitioned P1 levels
        self._H, self._refs = None, {}

    @property
    def H(self):
        if self._H is None:
            self._H = mh.Hierarchy(self.mesh, self.dm, self.levels)
        return self._H

    def dirichlet(self, system, dm=None):
        """dofs of the system's Dirichlet set on the dof map `dm` (default: the global one; a rank's local one
        gives the local ids, ghost rows included): pressure nodes resp. interleaved velocity dofs"""
        dm = self.dm if dm is None else dm
        if system == "pressure neumann":
            return np.zeros(0, dtype=np.int64)
        if system == "pressure outlet side":               # x = x_max: every strip owns some of these rows
            return np.nonzero(np.abs(dm.p1_coords[:, 0] - self.hi[0]) < 1e-12)[0]
        if system == "pressure outlet top":                # the last axis at its maximum: only the last rank owns any
            return np.nonzero(np.abs(dm.p1_coords[:, -1] - self.hi[-1]) < 1e-12)[0]
        X = dm.p2_coords                                     # the cavity set: every boundary node, every component
        on = np.zeros(X.shape[0], dtype=bool)
        for a in range(self.dim):
            on |= (np.abs(X[:, a]) < 1e-12) | (np.abs(X[:, a] - self.hi[a]) < 1e-12)
        nodes = np.nonzero(on)[0]
        return np.sort((self.dim * nodes[:, None] + np.arange(self.dim)[None, :]).ravel())

    def ranks(self, system):
        return mh.partition_ranks(self.parts, system == "velocity")

    def cycle(self, system, relaxed, dtype=np.float64, revert=()):
        """the definition of one application of mg_apply on this partition: exact halo mode -- the existing serial
        HostCycle; relaxed -- PartitionedCycle"""
        make = None
        if relaxed or revert:
            make = functools.partial(mh.PartitionedCycle, ranks=self.ranks(system), relaxed=relaxed, revert=revert)
        if system == "velocity":
            return self.H.velocity(self.dirichlet(system), BDF2[0] / STEP, NU, trunc_ratio=0.0, dtype=dtype, make=make)
        return self.H.pressure(self.dirichlet(system), dtype=dtype, make=make)

    def size_of(self, system):
        return self.dm.n_p2 * self.dim if system == "velocity" else self.dm.n_p1

    def rhs(self, system):
        seed = 1000 * sorted({**CASES, **SMALL_CASES}).index(self.name) + SYSTEMS.index(system)
        return np.random.default_rng(seed).standard_normal(self.size_of(system))   # (non-zero on flagged rows too)

    def reference(self, system, relaxed):
        """(r, z of the float64 definition, d = rel(z64, z_longdouble)): computed once"""
        key = (system, bool(relaxed))
        if key not in self._refs:
            r = self.rhs(system)
            z64 = self.cycle(system, relaxed).apply(r)
            d = mh.rel(z64, self.cycle(system, relaxed, dtype=mh.LD).apply(r))
            self._refs[key] = (r, z64, d)
        return self._refs[key]

    def bound(self, system, relaxed):
        """what the device is held to: max(64 d, 1e-14), plus the dictionary's 2^-38 where it is inexact"""
        return max(64.0 * self.reference(system, relaxed)[2], 1e-14) + DICT_EXTRA.get(self.name, 0.0)

    # ---- local <-> global vectors (nv interleaved components per node)
    def node_maps(self, system, part):
        """(global node ids of the rank's local nodes, owned flags)"""
        if system == "velocity":
            return np.asarray(part.p2_global), np.asarray(part.p2_owned)
        return np.asarray(part.p1_global), np.asarray(part.p1_owned)

    def to_local(self, system, part, v, ghosts="zero"):
        nv = self.dim if system == "velocity" else 1
        glob, owned = self.node_maps(system, part)
        out = np.asarray(v).reshape(-1, nv)[glob].copy()
        if ghosts == "zero":
            out[~owned] = 0.0
        elif ghosts != "valid":
            out[~owned] = ghosts
        return out.ravel()

    def gather(self, system, local_vectors):
        """the owned rows of the ranks' vectors as one global vector"""
        nv = self.dim if system == "velocity" else 1
        out = np.full((self.size_of(system) // nv, nv), np.nan)
        for part, v in zip(self.parts, local_vectors):
            glob, owned = self.node_maps(system, part)
            out[glob[owned]] = np.asarray(v).reshape(-1, nv)[owned]
        assert not np.isnan(out).any()
        return out.ravel()


_cases = {}


def case(name):
    if name not in _cases:
        _cases[name] = Case(name)
    return _cases[name]


# ------------------------------------------------------------------------------------------------------- device side
def run_ranks(parts, body, overlap=False):
    """one context per rank on the in-process communicator, `body(rank, ctx, part)` in one host thread per rank (after
    part.attach(ctx)); returns the bodies' results by rank.  The contexts are created here, so environment switches
    read at creation have to be set before."""
    import _native as nat
    size = len(parts)
    group = nat.local_group_create(size)
    ctxs = []
    for r, part in enumerate(parts):
        pdm = part.dofmap
        c = nat.NsfemContext(part.mesh.coords, part.mesh.cells, pdm.p2_dofmap, pdm.p1_dofmap, pdm.n_p2, pdm.n_p1)
        c.attach_local_comm(group, r)
        c.set_overlap(overlap)
        ctxs.append(c)
    out, errors = [None] * size, []

    def worker(r):
        try:
            parts[r].attach(ctxs[r])
            out[r] = body(r, ctxs[r], parts[r])
        except BaseException as exc:                     # a dead rank would deadlock the others
            errors.append((r, repr(exc)))
            import traceback
            traceback.print_exc()
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
