"""Host side of the energy spectra (energy_spectrum.py): the real Fourier basis, the lattice of a field's nodes, the bin
builders, and a numpy statement of the device plan against the FFT yardstick of tests/spectrum_host.py.  No GPU."""
import os
import re

import numpy as np
import pytest

import dlfn_compat as dlfn
import energy_spectrum as es
import spectrum_host as sh
from fem_mesh import TaylorHoodDofMap, box_mesh, periodic_entity_map, rectangle_mesh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def periodic_box(cells, lengths, axes, reorder=True):
    """(mesh, dofmap) of the box [0, L] with ``cells`` cells, periodic along ``axes`` (the low sides are the masters)"""
    dim = len(cells)
    L = tuple(float(v) for v in lengths)
    mesh = rectangle_mesh((0.0, 0.0), L, *cells) if dim == 2 else box_mesh((0.0, 0.0, 0.0), L, *cells)
    if not axes:
        return mesh, TaylorHoodDofMap(mesh, reorder=reorder)
    tol = 1e-9 * max(L)

    class Periodic(dlfn.SubDomain):
        def inside(self, x, on_boundary):
            return bool(on_boundary and any(abs(x[a]) < tol for a in axes) and
                        not any(abs(x[a] - L[a]) < tol for a in axes))

        def map(self, x, y):
            for a in range(dim):
                y[a] = x[a] - L[a] if (a in axes and abs(x[a] - L[a]) < tol) else x[a]

    return mesh, TaylorHoodDofMap(mesh, reorder=reorder, periodic_map=periodic_entity_map(mesh, Periodic()))


def plan_numpy(arr, bins):
    """the device plan in numpy: one einsum with F per transformed axis, square, bincount over the bin CSR;
    arr [n_z][n_y][n_x], returns raw [n_bins]"""
    d = arr.ndim
    w = arr
    for a, F in enumerate(bins.matrices):
        if F is not None:
            w = np.moveaxis(np.tensordot(F, w, axes=([1], [d - 1 - a])), 0, d - 1 - a)
    sq = w.ravel() ** 2
    n_bins = bins.bin_ptr.size - 1
    bin_of_entry = np.repeat(np.arange(n_bins), np.diff(bins.bin_ptr))
    return np.bincount(bin_of_entry, weights=sq[bins.bin_points], minlength=n_bins)


@pytest.mark.parametrize("n", [1, 2, 7, 8, 100])
def test_fourier_basis_is_orthonormal(n):
    F, k = es.fourier_basis(n)
    assert F.shape == (n, n) and k.shape == (n, )
    assert np.abs(F @ F.T - np.eye(n)).max() <= 4.0 * n * sh.EPS
    assert k[0] == 0 and k.max() == n // 2
    # wavenumbers 1 .. (n - 1) / 2 come in pairs, 0 and (even n) n / 2 once
    counts = np.bincount(k, minlength=n // 2 + 1)
    assert counts[0] == 1 and (counts[1:(n - 1) // 2 + 1] == 2).all()
    if n % 2 == 0 and n >= 2:
        assert counts[n // 2] == 1


LATTICE_CASES = [((4, 4), (1.0, 1.0), (0, 1)), ((6, 4), (1.5, 1.0), (0, )), ((4, 3), (1.0, 2.0), ()),
                 ((3, 2, 4), (1.0, 1.0, 2.0), (0, 1, 2)), ((4, 3, 2), (2.0, 1.0, 1.0), (0, 2)),
                 ((2, 3, 2), (1.0, 1.0, 1.0), ())]


@pytest.mark.parametrize("reorder", [True, "parity"])
@pytest.mark.parametrize("cells,lengths,axes", LATTICE_CASES)
def test_lattice_of_nodes_finds_every_point_once(cells, lengths, axes, reorder):
    mesh, dm = periodic_box(cells, lengths, axes, reorder)
    assert dm.ordering == ("parity" if reorder == "parity" else "lex")
    for field, m, X in (("velocity", 2, dm.p2_coords), ("pressure", 1, dm.p1_coords)):
        lat = es.lattice_of_nodes(mesh, dm, field)
        want = tuple(m * c + (0 if a in axes else 1) for a, c in enumerate(cells))
        assert lat.shape == want and lat.periodic == tuple(a in axes for a in range(len(cells)))
        assert lat.lengths == tuple(lengths)
        assert np.array_equal(np.sort(lat.node_of_point), np.arange(X.shape[0]))
        # the node of a point sits at the point
        idx = np.indices(lat.shape[::-1])[::-1]
        for a in range(len(cells)):
            x = lengths[a] * idx[a].ravel() / (m * cells[a])
            assert np.abs(X[lat.node_of_point, a] - x).max() <= 1e-12


def test_lattice_of_nodes_refuses_what_is_no_full_lattice():
    mesh, dm = periodic_box((4, 4), (1.0, 1.0), ())
    plain = type("M", (), {"_dim": 2})()
    with pytest.raises(ValueError):
        es.lattice_of_nodes(plain, dm, "velocity")                   # no mesh.structured
    other, dm_other = periodic_box((4, 3), (1.0, 1.0), ())
    with pytest.raises(ValueError):
        es.lattice_of_nodes(mesh, dm_other, "velocity")              # nodes of another lattice
    with pytest.raises(ValueError):
        es.lattice_of_nodes(mesh, dm, "vorticity")


def _lattice(shape, lengths, periodic=None):
    n = int(np.prod(shape))
    return es.Lattice(tuple(shape), np.arange(n, dtype=np.int32), tuple(periodic or (True, ) * len(shape)),
                      tuple(lengths), (0.0, ) * len(shape))


# (side lengths in integer ratios: |kappa| / dkappa is then the root of an integer and never half-way between two shells)
SHAPES = [((8, 8), (1.0, 1.0)), ((16, 24), (1.0, 2.0)), ((9, 7), (1.0, 1.0)), ((20, 12, 8), (2.0, 1.0, 1.0)),
          ((15, 8, 6), (1.0, 1.0, 1.0))]


@pytest.mark.parametrize("shape,lengths", SHAPES)
def test_shell_and_axis_bins_partition_the_points(shape, lengths):
    n = int(np.prod(shape))
    b = es.shell_bins(_lattice(shape, lengths))
    assert b.bin_ptr[0] == 0 and b.bin_ptr[-1] == n and (np.diff(b.bin_ptr) >= 0).all()
    assert np.array_equal(np.sort(b.bin_points), np.arange(n))
    assert b.bin_ptr.dtype == np.int32 and b.bin_points.dtype == np.int32
    periodic = (True, False) + (True, ) * (len(shape) - 2)
    a = es.axis_bins(0, _lattice(shape, lengths, periodic))
    assert np.array_equal(np.sort(a.bin_points), np.arange(n)) and a.bin_ptr[-1] == n
    assert a.bin_shape == (shape[1], shape[0] // 2 + 1) and a.matrices[1] is None and a.matrices[0] is not None
    with pytest.raises(ValueError):
        es.axis_bins(1, _lattice(shape, lengths, periodic))          # a walled axis
    with pytest.raises(ValueError):
        es.shell_bins(_lattice(shape, lengths, periodic))            # not fully periodic


@pytest.mark.parametrize("shape,lengths", SHAPES)
def test_numpy_statement_of_the_plan_meets_the_fft_yardstick(shape, lengths):
    rng = np.random.default_rng(len(shape) * 1000 + shape[0])
    arr = rng.standard_normal(shape[::-1])
    # shells
    want = sh.shell_spectrum(arr, lengths)
    got = plan_numpy(arr, es.shell_bins(_lattice(shape, lengths)))
    tol = sh.tolerance(shape, want.sum())
    assert got.shape == want.shape
    ratio = np.abs(got - want).max() / tol
    print("shape %r: shells, largest error / tolerance %.3g" % (shape, ratio))
    assert ratio <= 1.0
    assert abs(got.sum() - (arr ** 2).sum()) <= tol                  # Parseval
    # E(k_x; y): x periodic, y walled, z periodic
    periodic = (True, False) + (True, ) * (len(shape) - 2)
    bins = es.axis_bins(0, _lattice(shape, lengths, periodic))
    want = sh.axis_spectrum(arr, 0, periodic)
    got = plan_numpy(arr, bins).reshape(bins.bin_shape)
    assert got.shape == want.shape
    ratio = np.abs(got - want).max() / sh.tolerance(shape, want.sum())
    print("shape %r: axis, largest error / tolerance %.3g" % (shape, ratio))
    assert ratio <= 1.0
    line = (arr ** 2).sum(axis=tuple(p for p in range(arr.ndim) if p != arr.ndim - 2))
    assert np.abs(got.sum(axis=-1) - line).max() <= sh.tolerance(shape, want.sum())


def test_single_modes_land_in_their_shell():
    shape, lengths = (24, 16), (1.0, 1.0)
    bins = es.shell_bins(_lattice(shape, lengths))
    y, x = np.meshgrid(np.arange(16) / 16.0, np.arange(24) / 24.0, indexing="ij")
    for kx, ky, fn in ((0, 0, np.cos), (3, 0, np.cos), (3, 0, np.sin), (0, 5, np.sin), (12, 0, np.cos), (0, 8, np.cos),
                       (3, 4, np.sin)):
        arr = fn(2.0 * np.pi * (kx * x + ky * y))
        got = plan_numpy(arr, bins)
        shell = int(np.rint(np.hypot(kx, ky)))
        tol = sh.tolerance(shape, (arr ** 2).sum())
        assert abs(got[shell] - (arr ** 2).sum()) <= tol, (kx, ky)
        assert np.abs(np.delete(got, shell)).max() <= tol, (kx, ky)


def test_header_declares_the_spectrum_functions():
    text = open(os.path.join(ROOT, "include", "nsfem.h")).read()
    for name in ("nsfem_spectrum_set", "nsfem_spectrum_compute", "nsfem_spectrum_info"):
        assert re.search(r"\bint\s+%s\s*\(\s*nsfem_ctx\s*\*" % name, text), name
    import _native as nat
    for name in ("nsfem_spectrum_set", "nsfem_spectrum_compute", "nsfem_spectrum_info"):
        assert name in nat.EXPORTED_SYMBOLS
