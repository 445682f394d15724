"""A general tetrahedral test mesh (inputs only; no algorithm lives here).

box_mesh gives Kuhn boxes: every cell positively oriented, all cells of one volume, 44 % of the entries of J^-1
exactly zero, axis-aligned boundary planes, regular vertex patches.  general_tets sends the vertices of such a box
through a smooth non-linear map (an interior bump, a grading in x, a shear with small sine terms: no face stays
axis-aligned, no entry of any J^-1 stays zero), renumbers the vertices by a seeded permutation and sorts every cell's
vertices, so that about half the cells are negatively oriented, and shuffles the cell order.  The faces keep the ids
of tests/test_gpu_3d.box3 (2 axis + 1 at the low end, 2 axis + 2 at the high end): they are marked on the box
before the map and carried over by their vertices.

The conditions the mesh has to meet (orientation mix, volume spread, conditioning, no small entry of J^-1, irregular
valence, oblique boundary normals) are asserted in tests/test_general_tet_mesh_host.py."""
import numpy as np

from fem_mesh import FacetMarkers, Mesh, TaylorHoodDofMap, box_mesh

SIZES = (((3, 2, 2), (1.0, 0.8, 0.6)), ((4, 4, 4), (1.0, 1.0, 1.0)), ((6, 5, 5), (1.0, 0.8, 0.6)))
SMALL, CUBE, LARGE = SIZES                  # 72 cells (one partly filled block), 384, 900 (340 boundary faces)


def mapped_coords(coords, lengths):
    """the map of the module docstring applied to the vertices of the box (0, lengths)"""
    lx, ly, lz = lengths
    x, y, z = coords[:, 0], coords[:, 1], coords[:, 2]
    b = np.sin(np.pi * x / lx) * np.sin(np.pi * y / ly) * np.sin(np.pi * z / lz)
    xi = x + 0.07 * b * (1.0 + 0.5 * y)
    yi = y - 0.05 * b * np.cos(1.3 * x)
    zi = z + 0.04 * b * (1.0 - 0.7 * x + 0.4 * y)
    xg = xi ** 1.6 / lx ** 0.6
    return np.stack([xg + 0.15 * yi + 0.05 * np.sin(2.1 * zi), yi - 0.1 * zi + 0.04 * np.sin(1.7 * xg),
                     zi + 0.08 * xg * yi + 0.03 * np.sin(2.3 * yi)], axis=1)


def _box_face_ids(m0, lengths):
    marks = FacetMarkers(m0)
    for axis in range(3):
        marks.mark(lambda X, a=axis: np.abs(X[:, a]) < 1e-12, 2 * axis + 1)
        marks.mark(lambda X, a=axis: np.abs(X[:, a] - lengths[a]) < 1e-12, 2 * axis + 2)
    return marks.values


def general_tets(n, lengths, seed=7, renumber=True):
    """(mesh, dm, marks) of the mapped box n = (nx, ny, nz) on (0, lengths).  renumber=False keeps the vertex
    numbering, the vertex order inside the cells and the cell order of box_mesh (every cell positively oriented):
    the same geometry and the same finite element spaces, for checking that a restatement is orientation-blind."""
    m0 = box_mesh((0.0, 0.0, 0.0), tuple(lengths), *n)
    nv = m0.num_vertices()
    X = mapped_coords(m0.coords, lengths)
    if renumber:
        rng = np.random.default_rng(seed)
        perm = rng.permutation(nv)
        cells = np.sort(perm[m0.cells.astype(np.int64)], axis=1)
        cells = cells[rng.permutation(cells.shape[0])]
    else:
        perm = np.arange(nv)
        cells = m0.cells
    coords = np.empty_like(X)
    coords[perm] = X
    mesh = Mesh(coords, cells)
    dm = TaylorHoodDofMap(mesh)
    # the ids of the box faces, carried over by the (renumbered, sorted) vertex triples
    ids0 = _box_face_ids(m0, lengths)
    f0 = np.sort(perm[m0.facets.astype(np.int64)], axis=1)
    key0 = (f0[:, 0] * nv + f0[:, 1]) * nv + f0[:, 2]
    f1 = mesh.facets.astype(np.int64)
    key1 = (f1[:, 0] * nv + f1[:, 1]) * nv + f1[:, 2]
    order = np.argsort(key0)
    pos = np.searchsorted(key0[order], key1)
    assert np.array_equal(key0[order][pos], key1)
    marks = FacetMarkers(mesh)
    marks.values[:] = ids0[order][pos]
    return mesh, dm, marks


def shear_bc(dm, marks):
    """velocity Dirichlet values of the step tests on this mesh: the trace of the solenoidal field (0.5 z, 0.15 x, -0.1 y)
    on all six faces.  The lid (1, 0, 0) of tests/test_gpu_3d.lid_bc is no boundary value here: face 6 is oblique, the
    lid has a net flux through it, and the pure Neumann pressure problem of the projection step has no solution then
    (the device projects the right-hand side, the host pins a node: two different answers to an ill-posed question)"""
    nodes = np.unique(dm.facet_p2_nodes(np.concatenate([marks.facets_with_id(mid) for mid in range(1, 7)])))
    X = dm.p2_coords[nodes]
    vals = np.stack([0.5 * X[:, 2], 0.15 * X[:, 0], -0.1 * X[:, 1]], axis=1)
    dofs = (3 * nodes[:, None] + np.arange(3)[None, :]).ravel()
    order = np.argsort(dofs)
    return dofs[order].astype(np.int64), vals.ravel()[order]


def jacobians(mesh):
    """J [nc, 3, 3] with J[:, :, a] = x_{a+1} - x_0, the edge vectors as columns"""
    X = mesh.coords[mesh.cells.astype(np.int64)]
    return np.transpose(X[:, 1:] - X[:, :1], (0, 2, 1))
