"""Host side of the device point locator (csrc/points.hip): a uniform grid of bins over the mesh.

The reference finds the cell of a point through dolfin's bounding-box tree (``Function.__call__``).  Here the host
sorts the cells into bins once and the device walks the few candidates of a point's bin (``k_locate_points``).  One
code path for every affine simplex mesh: lattices, graded and unstructured meshes, Kuhn boxes, shells with a hole.

Bin size: the edge of a cube whose volume is (bounding-box volume) / (number of cells), the same in every direction;
``nbins[d] = ceil(extent[d] / edge)``, so there are about as many bins as cells.  On a right-diagonal lattice this
gives 0.71 (2D) / 0.55 (3D) lattice spacings per bin -- deliberately not a divisor of the spacing: bins aligned with
the lattice lines would touch the closed bounding boxes of both neighbours in every direction.

A cell is listed in every bin its bounding box, inflated by 1e-9 of the mesh extent, overlaps.  The inflation is far
larger than the distance at which the barycentric test (all coordinates >= -1e-12) still accepts a point outside a
cell, so every cell that accepts a point is among the candidates of the point's bin.  Host and device compute the bin
index with the same monotone expression ``floor((x - origin) * inv_h)``: a point between the two corners of a box can
never land in a bin outside the range of bins the box was given.
"""
import numpy as np

INFLATE = 1.0e-9          # bounding-box inflation, relative to the largest extent of the mesh
INSIDE_TOL = -1.0e-12     # a cell contains a point when all barycentric coordinates are >= this (evaluate_lagrange)


def _bin_index(x, origin, inv_h):
    """per-direction bin index of the coordinates ``x`` [.., dim] as floats (NOT clipped): the device's expression"""
    return np.floor((x - origin) * inv_h)


def build_bins(coords, cells):
    """-> dict(origin [dim], inv_h [dim], nbins [dim] int32, bin_ptr [prod(nbins) + 1] int32, bin_cells int32): per
    bin (x fastest) the cells whose inflated closed bounding box overlaps it, in ascending cell id"""
    coords = np.ascontiguousarray(coords, dtype=np.float64)
    cells = np.asarray(cells).astype(np.int64)
    dim = coords.shape[1]
    assert cells.ndim == 2 and cells.shape[1] == dim + 1 and cells.shape[0] > 0
    nc = cells.shape[0]
    x = coords[cells]                                              # [nc, dim + 1, dim]
    lo_mesh, hi_mesh = coords.min(axis=0), coords.max(axis=0)
    extent = hi_mesh - lo_mesh
    pad = INFLATE * float(extent.max())
    origin = lo_mesh - pad                                         # the grid covers the inflated boxes of all cells
    span = extent + 2.0 * pad
    edge = (float(np.prod(span)) / nc) ** (1.0 / dim)
    nbins = np.maximum(1, np.ceil(span / edge)).astype(np.int64)
    assert int(np.prod(nbins)) < 2 ** 31 - 1
    inv_h = nbins / span
    lo = np.clip(_bin_index(x.min(axis=1) - pad, origin, inv_h), 0, nbins - 1).astype(np.int64)
    hi = np.clip(_bin_index(x.max(axis=1) + pad, origin, inv_h), 0, nbins - 1).astype(np.int64)
    width = hi - lo + 1                                            # bins per direction of every cell
    count = np.prod(width, axis=1)
    total = int(count.sum())
    assert total < 2 ** 31 - 1
    cell_of = np.repeat(np.arange(nc, dtype=np.int64), count)
    k = np.arange(total, dtype=np.int64) - np.repeat(np.cumsum(count) - count, count)
    bin_of = np.zeros(total, dtype=np.int64)
    stride = 1
    for d in range(dim):
        w = width[cell_of, d]
        bin_of += stride * (lo[cell_of, d] + k % w)
        k //= w
        stride *= int(nbins[d])
    order = np.argsort(bin_of, kind="stable")                      # stable: ascending cell id inside a bin
    n_bins = int(np.prod(nbins))
    bin_ptr = np.zeros(n_bins + 1, dtype=np.int64)
    np.cumsum(np.bincount(bin_of, minlength=n_bins), out=bin_ptr[1:])
    return dict(origin=origin, inv_h=inv_h, nbins=nbins.astype(np.int32), bin_ptr=bin_ptr.astype(np.int32),
                bin_cells=cell_of[order].astype(np.int32))


def bin_of_points(bins, X):
    """flat bin index of every point of X [m, dim]; -1 outside the grid (or NaN)"""
    X = np.asarray(X, dtype=np.float64).reshape(-1, len(bins["origin"]))
    nb = bins["nbins"].astype(np.int64)
    with np.errstate(invalid="ignore"):
        t = (X - bins["origin"]) * bins["inv_h"]
        ok = ((t >= 0.0) & (t < nb)).all(axis=1)
    idx = np.where(ok[:, None], np.floor(np.where(ok[:, None], t, 0.0)), 0).astype(np.int64)
    strides = np.concatenate([[1], np.cumprod(nb)[:-1]])
    return np.where(ok, idx @ strides, -1)


def barycentric(coords, cells, cell_ids, X):
    """barycentric coordinates [m, dim + 1] of point X[i] in cell cell_ids[i], through the inverse Jacobian as the
    device forms them"""
    x = np.asarray(coords)[np.asarray(cells).astype(np.int64)[cell_ids]]
    J = np.transpose(x[:, 1:] - x[:, :1], (0, 2, 1))
    ref = np.einsum("mab,mb->ma", np.linalg.inv(J), X - x[:, 0])
    return np.concatenate([1.0 - ref.sum(axis=1, keepdims=True), ref], axis=1)


def locate_points_numpy(bins, coords, cells, X, return_tests=False):
    """numpy restatement of ``k_locate_points``: the first candidate of the point's bin whose barycentric coordinates
    are all >= -1e-12, -1 outside; optionally also the number of cells tested per point"""
    dim = len(bins["origin"])
    X = np.asarray(X, dtype=np.float64).reshape(-1, dim)
    m = X.shape[0]
    found = np.full(m, -1, dtype=np.int32)
    tests = np.zeros(m, dtype=np.int64)
    b = bin_of_points(bins, X)
    ptr, lst = bins["bin_ptr"].astype(np.int64), bins["bin_cells"]
    active = np.nonzero(b >= 0)[0]
    pos = ptr[b[active]]
    end = ptr[b[active] + 1]
    while active.size:
        keep = pos < end
        active, pos, end = active[keep], pos[keep], end[keep]
        if not active.size:
            break
        c = lst[pos]
        lam = barycentric(coords, cells, c, X[active])
        hit = (lam >= INSIDE_TOL).all(axis=1)
        tests[active] += 1
        found[active[hit]] = c[hit]
        active, pos, end = active[~hit], pos[~hit] + 1, end[~hit]
    return (found, tests) if return_tests else found
