"""Host side of the device point locator (point_locator.build_bins, csrc/points.hip): candidate completeness of the bins,
the numpy restatement of ``k_locate_points`` against the brute-force search of ``fem_spaces.evaluate_lagrange``, and
points outside the mesh -- on the meshes and point sets tests/test_gpu_points.py runs on the device (it imports them
from here, brute-force cells included).

Ambiguity: host and device form the barycentric coordinates in different ways (LU solve / inverse Jacobian), a few
roundings of 2^-53 times the condition of the cell apart.  A point is ambiguous when a host coordinate of some cell
falls into the band [-1e-11, -1e-13] around the tolerance -1e-12; the seeds below are chosen so that the band is
empty, which ``brute_force`` checks for every point set."""
import functools
import os

import numpy as np
import pytest

from fem_mesh import TaylorHoodDofMap, box_mesh, rectangle_mesh
from point_locator import bin_of_points, build_bins, locate_points_numpy

HERE = os.path.dirname(os.path.abspath(__file__))
MESHES = ("rectangle", "graded", "fixture", "box", "shell")
SEEDS = dict(rectangle=1, graded=2, fixture=3, box=4, shell=5)
N_RANDOM = 1003                      # not a multiple of the workgroup size (256)


@functools.lru_cache(maxsize=None)
def mesh_of(name):
    if name == "rectangle":
        mesh = rectangle_mesh((0.0, 0.0), (1.5, 1.0), 3, 5)
    elif name == "graded":
        from test_gpu_volume_functionals import _mesh
        mesh = _mesh("graded")[0]
    elif name == "fixture":
        from mesh_io import read_msh
        mesh = read_msh(os.path.join(HERE, "golden", "square_v41.msh"))[0]
    elif name == "box":
        mesh = box_mesh((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 2, 3, 2)
    elif name == "shell":
        import grid_generator as gg
        mesh = gg.spherical_shell(3, (0.4, 1.0), 8)[0]
    else:
        raise ValueError(name)
    return mesh, TaylorHoodDofMap(mesh)


def outside_points(mesh):
    """four points outside the bounding box: beyond the low and the high corner, far away, and beside one face"""
    lo, hi = mesh.coords.min(axis=0), mesh.coords.max(axis=0)
    mid = 0.5 * (lo + hi)
    beside = mid.copy()
    beside[0] = hi[0] + 1e-3 * (hi[0] - lo[0])
    return np.stack([lo - 0.25 * (hi - lo), hi + 0.25 * (hi - lo), mid + 1e6, beside])


@functools.lru_cache(maxsize=None)
def point_sets(name):
    """{label: X [m, dim]}: seeded uniform points in the bounding box, all P2 nodes (vertices and edge midpoints), all
    cell centroids, four points outside the box, and the sizes 0 and 1"""
    mesh, dm = mesh_of(name)
    lo, hi = mesh.coords.min(axis=0), mesh.coords.max(axis=0)
    rng = np.random.default_rng(SEEDS[name])
    random = lo + (hi - lo) * rng.random((N_RANDOM, lo.size))
    centroids = mesh.coords[mesh.cells.astype(np.int64)].mean(axis=1)
    return dict(random=random, nodes=np.array(dm.p2_coords), centroids=centroids, outside=outside_points(mesh),
                empty=np.zeros((0, lo.size)), one=random[:1].copy())


def brute_force_cells(mesh, X):
    """the search of fem_spaces.evaluate_lagrange for many points: (lowest-id cell with all reference coordinates >
    -1e-12 and their sum < 1 + 1e-12, else -1; number of points with a barycentric coordinate in the ambiguity band)"""
    X = np.asarray(X, dtype=np.float64)
    x = mesh.coords[mesh.cells.astype(np.int64)]
    J = np.transpose(x[:, 1:] - x[:, :1], (0, 2, 1))
    cells = np.full(X.shape[0], -1, dtype=np.int32)
    ambiguous = 0
    for i, p in enumerate(X):
        ref = np.linalg.solve(J, (p[None, :] - x[:, 0])[:, :, None])[:, :, 0]
        inside = np.nonzero((ref > -1e-12).all(axis=1) & (ref.sum(axis=1) < 1.0 + 1e-12))[0]
        if inside.size:
            cells[i] = inside[0]
        lam = np.concatenate([ref, 1.0 - ref.sum(axis=1, keepdims=True)], axis=1)
        ambiguous += int(((lam >= -1e-11) & (lam <= -1e-13)).any())
    return cells, ambiguous


@functools.lru_cache(maxsize=None)
def brute_force(name, label):
    """brute-force cells of a point set (computed once per run, shared with the device tests); asserts that no point
    of the set is ambiguous"""
    cells, ambiguous = brute_force_cells(mesh_of(name)[0], point_sets(name)[label])
    assert ambiguous == 0, (name, label, ambiguous)
    cells.setflags(write=False)
    return cells


@functools.lru_cache(maxsize=None)
def bins_of(name):
    mesh, _ = mesh_of(name)
    return build_bins(mesh.coords, mesh.cells)


@pytest.mark.parametrize("name", MESHES)
def test_bins_are_well_formed(name):
    mesh, _ = mesh_of(name)
    b = bins_of(name)
    dim = mesh.coords.shape[1]
    assert b["origin"].shape == b["inv_h"].shape == b["nbins"].shape == (dim, )
    assert b["nbins"].dtype == b["bin_ptr"].dtype == b["bin_cells"].dtype == np.int32
    n_bins = int(np.prod(b["nbins"].astype(np.int64)))
    assert b["bin_ptr"].shape == (n_bins + 1, ) and b["bin_ptr"][0] == 0 and b["bin_ptr"][-1] == b["bin_cells"].size
    assert (np.diff(b["bin_ptr"]) >= 0).all()
    assert b["bin_cells"].min() >= 0 and b["bin_cells"].max() < mesh.num_cells()
    for k in range(n_bins):                                   # ascending cell id inside a bin, no duplicates
        assert (np.diff(b["bin_cells"][b["bin_ptr"][k]: b["bin_ptr"][k + 1]]) > 0).all()
    # about as many bins as cells, a few candidates per bin
    print("%s: %d cells, bins %s, list length %d, %.2f candidates per bin" %
          (name, mesh.num_cells(), b["nbins"], b["bin_cells"].size, b["bin_cells"].size / n_bins))
    assert n_bins <= 4 ** dim * mesh.num_cells() + 4 ** dim


@pytest.mark.parametrize("name", MESHES)
def test_every_cell_is_a_candidate_of_its_own_points(name):
    """centroid, vertices and edge midpoints of every cell find the cell among the candidates of their bin"""
    mesh, _ = mesh_of(name)
    b = bins_of(name)
    x = mesh.coords[mesh.cells.astype(np.int64)]              # [nc, dim + 1, dim]
    nv = x.shape[1]
    pts = [x.mean(axis=1)] + [x[:, i] for i in range(nv)] + \
          [0.5 * (x[:, i] + x[:, j]) for i in range(nv) for j in range(i + 1, nv)]
    for P in pts:
        bins = bin_of_points(b, P)
        assert (bins >= 0).all()
        for c, k in enumerate(bins):
            assert c in b["bin_cells"][b["bin_ptr"][k]: b["bin_ptr"][k + 1]], (name, c, k)


@pytest.mark.parametrize("name", MESHES)
def test_numpy_restatement_equals_the_brute_force_search(name):
    mesh, _ = mesh_of(name)
    b = bins_of(name)
    for label, X in point_sets(name).items():
        got, tests = locate_points_numpy(b, mesh.coords, mesh.cells, X, return_tests=True)
        want = brute_force(name, label)
        assert got.dtype == np.int32 and got.shape == (X.shape[0], )
        assert np.array_equal(got, want), (name, label, np.nonzero(got != want)[0][:10])
        if X.shape[0]:
            print("%s / %s: %d points, %d outside, %.2f cells tested per point" %
                  (name, label, X.shape[0], int((got < 0).sum()), tests.mean()))
    inside = brute_force(name, "random") >= 0
    assert inside.any()
    assert (brute_force(name, "nodes") >= 0).all() and (brute_force(name, "centroids") >= 0).all()
    assert np.array_equal(brute_force(name, "centroids"), np.arange(mesh.num_cells()))


def test_points_in_the_hole_and_outside_the_box_give_minus_one():
    mesh, _ = mesh_of("shell")
    b = bins_of("shell")
    rng = np.random.default_rng(7)
    d = rng.standard_normal((64, 3))
    d /= np.linalg.norm(d, axis=1, keepdims=True)
    hole = 0.3 * rng.random((64, 1)) * d                      # radius < 0.3: inside the inner sphere's polyhedron
    far = 1.0001 * d                                          # outside the outer sphere, inside the bounding box
    for X in (hole, far, outside_points(mesh), np.full((2, 3), np.nan)):
        assert np.array_equal(locate_points_numpy(b, mesh.coords, mesh.cells, X), np.full(X.shape[0], -1))
        if not np.isnan(X).any():
            assert np.array_equal(brute_force_cells(mesh, X)[0], np.full(X.shape[0], -1))
    # the random points of the shell's bounding box: some in the hole or outside, some inside
    cells = brute_force("shell", "random")
    assert (cells < 0).sum() > 100 and (cells >= 0).sum() > 100
    for name in MESHES:
        assert (brute_force(name, "outside") == -1).all()
