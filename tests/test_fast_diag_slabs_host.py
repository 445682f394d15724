"""Host side of the fast-diagonalisation solve on partitioned slabs (partition.SlabPartition.attach_fast_diag,
PeriodicSlabPartition.attach_fast_diag): what every rank sends to its context -- the factors of the GLOBAL box lattice
and the rank's first lattice plane, local P1 plane i being global plane (first + i) mod N_z."""
import numpy as np
import pytest

import poisson_fd as pf
from partition import PeriodicSlabPartition, SlabPartition


class _Recorder:
    """stand-in for NsfemContext: records the calls attach_fast_diag makes"""

    def __init__(self):
        self.calls = []

    def poisson_set_fast_diag_3d(self, factors, first_plane=None):
        self.calls.append((factors, first_plane))


def _check(parts, f_ref):
    Nz, Ny, Nx = f_ref["inv"].shape
    plane = Nx * Ny
    owned = np.zeros(Nz, dtype=np.int64)
    firsts = []
    for part in parts:
        rec = _Recorder()
        assert part.attach_fast_diag(rec) == f_ref["exact"]
        assert len(rec.calls) == 1
        f, first = rec.calls[0]
        assert first is not None
        firsts.append(first)
        for k in ("Vx", "Vy", "Vz", "inv"):
            assert np.array_equal(f[k], f_ref[k]), k
        assert f["exact"] == f_ref["exact"] and f["singular"] == f_ref["singular"]
        n_p1 = part.dofmap.n_p1
        assert n_p1 % plane == 0
        n_loc = n_p1 // plane
        # every local P1 node lies on global plane (first + i) mod N_z
        planes = (first + np.arange(n_loc)) % Nz
        assert np.array_equal(np.repeat(planes, plane), np.asarray(part.p1_global) // plane)
        own = np.asarray(part.p1_owned).reshape(n_loc, plane)
        assert (own.all(axis=1) | ~own.any(axis=1)).all()           # whole planes owned or not
        owned[planes[own.all(axis=1)]] += 1
    assert (owned == 1).all()                                        # every global plane owned once
    return firsts


@pytest.mark.parametrize("size", [2, 3, 4])
def test_slab_factors_and_first_planes(size):
    n = (4, 3, 12)
    lo, hi = (0.0, 0.0, 0.0), (1.0, 0.75, 1.5)
    parts = [SlabPartition(lo, hi, *n, r, size, coarsest=2) for r in range(size)]
    lines = [np.linspace(lo[a], hi[a], n[a] + 1) for a in range(3)]
    f_ref = pf.factors_3d(*lines, periodic=(False, False, False), dirichlet_nodes=np.zeros(0, np.int64))
    assert f_ref["inv"].shape == (13, 4, 5) and not f_ref["exact"]      # closed box: T^+ preconditions CG
    firsts = _check(parts, f_ref)
    own = n[2] // size
    assert firsts == [r * own for r in range(size)]


@pytest.mark.parametrize("size", [2, 3, 4])
def test_periodic_slab_factors_and_first_planes_wrap_around(size):
    n = (4, 6, 12)
    lo, hi = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
    parts = [PeriodicSlabPartition(lo, hi, *n, r, size, coarsest=2) for r in range(size)]
    lines = [np.linspace(lo[a], hi[a], n[a] + 1) for a in range(3)]
    f_ref = pf.factors_3d(*lines, periodic=(True, True, True), dirichlet_nodes=np.zeros(0, np.int64))
    assert f_ref["inv"].shape == (12, 6, 4) and f_ref["exact"] and f_ref["singular"]
    firsts = _check(parts, f_ref)
    own = n[2] // size
    assert firsts == [r * own for r in range(size)]
    # the last rank holds global planes N_z - own ... N_z - 1, then wraps to planes 0 and 1 (its top ghost plane)
    last = parts[-1]
    n_loc = last.dofmap.n_p1 // (n[0] * n[1])
    assert n_loc == own + 2
    planes = (firsts[-1] + np.arange(n_loc)) % n[2]
    assert list(planes[-2:]) == [0, 1]
