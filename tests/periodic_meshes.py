"""Periodic test meshes (inputs only; no algorithm lives here).

A periodic dof map identifies the nodes of the high side of a periodic axis with those of the low side: n_p1 is below
the number of mesh vertices, a vertex patch reaches across the seam, and the coordinates of the vertices of a seam cell
(taken per cell, from mesh.coords) lie a whole period away from the coordinates stored for its dofs.  Every fixture
returns (mesh, dm, marks) like gpu_common.box and test_gpu_3d.box3.

    pchan2    (4, 3) on 1 x 0.75          periodic in x, walls in y        20 vertices, n_p1 16, n_p2 56, 24 cells
    psquare   (4, 4) on the unit square   periodic in x and y, no wall     25 vertices, n_p1 16, n_p2 64, 32 cells
    pchan3    (3, 2, 3) on 1 x 0.8 x 0.6  periodic in x and z, walls in y  48 vertices, n_p1 27, n_p2 180, 108 cells
    pbox3     (3, 3, 3) on the unit cube  periodic in x, y and z, no wall  64 vertices, n_p1 27, n_p2 216, 162 cells

(the 3D dof maps in parity numbering).  Three cells along a periodic axis is the smallest count at which no cell carries
one dof twice and no vertex patch contains a neighbour twice.  Facet markers exist on the walls only, with the ids of
gpu_common.box and test_gpu_3d.box3 (2 axis + 1 at the low end, 2 axis + 2 at the high end); the velocity Dirichlet set
is no-slip on the walls and empty on psquare and pbox3.

pchan2_mapped and pchan3_mapped move the vertices of the two channels by a smooth displacement that is L-periodic along
the periodic axes and vanishes on the walls, before the dof map is built; the identification is topological and comes
from the unmapped mesh.  On the uniform fixtures a seam cell is a translated copy of an interior cell and a
volume-weighted patch mean equals the plain one; on the mapped ones the cells of every patch differ in volume.

The conditions the fixtures have to meet are asserted in tests/test_periodic_meshes_host.py."""
import numpy as np

import dlfn_compat as dlfn
from fem_mesh import FacetMarkers, Mesh, TaylorHoodDofMap, periodic_entity_map
from test_energy_spectrum_host import periodic_box

# name: (cells per axis, lengths, periodic axes, mapped)
FIXTURES = {
    "pchan2": ((4, 3), (1.0, 0.75), (0, ), False),
    "psquare": ((4, 4), (1.0, 1.0), (0, 1), False),
    "pchan3": ((3, 2, 3), (1.0, 0.8, 0.6), (0, 2), False),
    "pbox3": ((3, 3, 3), (1.0, 1.0, 1.0), (0, 1, 2), False),
    "pchan2_mapped": ((4, 3), (1.0, 0.75), (0, ), True),
    "pchan3_mapped": ((3, 2, 3), (1.0, 0.8, 0.6), (0, 2), True),
}
UNIFORM = ("pchan2", "psquare", "pchan3", "pbox3")
MAPPED = ("pchan2_mapped", "pchan3_mapped")
ALL = UNIFORM + MAPPED
CHANNELS = ("pchan2", "pchan3")
# (mesh vertices, n_p1, n_p2, cells) of the uniform fixtures; the mapped ones share those of their channel
EXPECTED = {"pchan2": (20, 16, 56, 24), "psquare": (25, 16, 64, 32), "pchan3": (48, 27, 180, 108),
            "pbox3": (64, 27, 216, 162)}


def is_periodic(kind):
    return isinstance(kind, str) and kind in FIXTURES


def cells_of(name):
    return FIXTURES[name][0]


def lengths_of(name):
    return FIXTURES[name][1]


def periodic_axes(name):
    return FIXTURES[name][2]


def wall_axes(name):
    cells, _, axes, _ = FIXTURES[name]
    return tuple(a for a in range(len(cells)) if a not in axes)


def displaced(coords, lengths, axes):
    """the vertices moved by a smooth displacement, L-periodic along ``axes`` and zero on the walls (the other axes)"""
    dim = coords.shape[1]
    L = np.asarray(lengths, dtype=np.float64)
    phase = 2.0 * np.pi * coords / L
    walls = [a for a in range(dim) if a not in axes]
    bump = np.ones(coords.shape[0])
    for a in walls:
        bump = bump * np.sin(np.pi * coords[:, a] / L[a])
    out = coords.copy()
    if dim == 2:
        out[:, 0] += 0.045 * bump * (np.sin(phase[:, 0] + 0.4) + 0.5 * np.cos(2.0 * phase[:, 0]))
        out[:, 1] += 0.040 * bump * np.cos(phase[:, 0] - 0.7)
    else:
        out[:, 0] += 0.050 * bump * (np.sin(phase[:, 0] + 0.4) + 0.6 * np.cos(phase[:, 2] + 1.1))
        out[:, 1] += 0.045 * bump * np.cos(phase[:, 0] - 0.7) * np.sin(phase[:, 2] + 0.3)
        out[:, 2] += 0.035 * bump * (np.sin(phase[:, 2] - 0.9) + 0.7 * np.sin(phase[:, 0] + 2.0))
    return out


def _wall_marks(mesh, lengths, axes, flat):
    """markers on the walls only; ``flat``: the coordinates the faces are recognised by (those of the unmapped mesh)"""
    dim = len(lengths)
    marks = FacetMarkers(mesh)
    mids = flat[mesh.facets.astype(np.int64)].mean(axis=1)
    bnd = mesh.facet_on_boundary
    for a in range(dim):
        if a in axes:
            continue
        marks.values[bnd & (np.abs(mids[:, a]) < 1e-12)] = 2 * a + 1
        marks.values[bnd & (np.abs(mids[:, a] - lengths[a]) < 1e-12)] = 2 * a + 2
    return marks


_CACHE = {}


def periodic_fixture(name):
    """(mesh, dm, marks) of the fixture ``name``; built once and left unchanged"""
    if name not in _CACHE:
        cells, lengths, axes, mapped = FIXTURES[name]
        reorder = "parity" if len(cells) == 3 else True
        m0, dm0 = periodic_box(cells, lengths, axes, reorder)
        if not mapped:
            mesh, dm = m0, dm0
        else:
            # the same cells, edges and faces (numbered from the vertex ids alone), other coordinates; the entity map
            # of the unmapped mesh
            mesh = Mesh(displaced(m0.coords, lengths, axes), m0.cells)
            assert np.array_equal(mesh.edges, m0.edges) and np.array_equal(mesh.cell_edges, m0.cell_edges)
            assert np.array_equal(mesh.facets, m0.facets)
            tol = 1e-9 * max(lengths)
            L = lengths
            dim = len(cells)

            class Periodic(dlfn.SubDomain):
                def inside(self, x, on_boundary):
                    return bool(on_boundary and any(abs(x[a]) < tol for a in axes) and
                                not any(abs(x[a] - L[a]) < tol for a in axes))

                def map(self, x, y):
                    for a in range(dim):
                        y[a] = x[a] - L[a] if (a in axes and abs(x[a] - L[a]) < tol) else x[a]

            dm = TaylorHoodDofMap(mesh, periodic_map=periodic_entity_map(m0, Periodic()))
            assert (dm.n_p1, dm.n_p2) == (dm0.n_p1, dm0.n_p2)
        _CACHE[name] = (mesh, dm, _wall_marks(mesh, lengths, axes, m0.coords))
    return _CACHE[name]


def plain_box(name):
    """(mesh, dm) of the same cells and coordinates without identification"""
    mesh = periodic_fixture(name)[0]
    if FIXTURES[name][3]:
        return mesh, TaylorHoodDofMap(mesh)
    cells, lengths, axes, _ = FIXTURES[name]
    return periodic_box(cells, lengths, (), "parity" if len(cells) == 3 else True)


def wall_bc(name):
    """velocity Dirichlet dofs and values: no-slip on the walls; empty on psquare and pbox3"""
    mesh, dm, marks = periodic_fixture(name)
    dim = mesh._dim
    ids = sorted(mid for mid in marks.ids() if mid > 0)          # (the periodic sides are boundary faces without an id)
    if not ids:
        return np.zeros(0, np.int64), np.zeros(0)
    nodes = np.unique(dm.facet_p2_nodes(np.concatenate([marks.facets_with_id(mid) for mid in ids])))
    dofs = np.sort((dim * nodes[:, None] + np.arange(dim)[None, :]).ravel()).astype(np.int64)
    return dofs, np.zeros(dofs.size)


def periodic_fields(X, lengths, axes):
    """a smooth non-polynomial velocity [n, dim] flattened and a scalar, L-periodic along ``axes``; every entry of the
    velocity gradient is non-zero"""
    dim = X.shape[1]
    L = np.asarray(lengths, dtype=np.float64)
    # the phase of a periodic axis is 2 pi x / L; a walled axis enters as it is
    s = np.stack([2.0 * np.pi * X[:, a] / L[a] if a in axes else 2.3 * X[:, a] + 0.35 for a in range(dim)], axis=1)
    K = np.array([[1.0, 1.0, -1.0], [-1.0, 1.0, 1.0], [1.0, -1.0, 1.0]])[:dim, :dim]
    arg = s @ K.T + np.array([0.2, 0.5, 0.9])[:dim]
    u = (np.sin(arg) + 0.35 * np.cos(2.0 * s @ K.T[::-1] + 0.3)) * np.array([1.0, 0.8, 1.2])[:dim]
    T = 1.1 * np.sin(s @ np.array([1.0, -1.0, 1.0])[:dim] + 0.4) + 0.3 * np.cos(s.sum(axis=1) * 1.0 + 1.3) + 0.3
    return u.ravel(), T


def seeded_modes(X, lengths, axes, seed):
    """a seeded superposition of four products of sines per component [n, dim], flattened: wave numbers 1 and 2,
    L-periodic with a random phase along ``axes``, sin(k pi x / L) along the walled axes (a no-slip trace).  The
    dynamic procedures give a negative constant for most smooth fields; the seeds used by the tests were found by a
    search over a few of them on the CPU, and the tests assert what they need on the restatement alone"""
    rng = np.random.default_rng(seed)
    dim = X.shape[1]
    s = np.stack([(2.0 if a in axes else 1.0) * np.pi * X[:, a] / lengths[a] for a in range(dim)], axis=1)
    u = np.zeros_like(X)
    for _ in range(4):
        k = rng.integers(1, 3, size=dim)
        ph = rng.uniform(0.0, 6.28, size=dim)
        c = rng.uniform(-1.0, 1.0, size=dim)
        for a in range(dim):
            f = c[a]
            for b in range(dim):
                f = f * (np.sin(k[b] * s[:, b] + ph[b]) if b in axes else np.sin(k[b] * s[:, b]))
            u[:, a] += f
    return u.ravel()


def far_images(name):
    """[cells, dim + 1] bool: the cell reads this vertex at coordinates more than L / 2 away from those stored for its
    P1 dof -- the cell lies across the seam from the dof's master image"""
    mesh, dm, _ = periodic_fixture(name)
    L = np.asarray(lengths_of(name))
    X = mesh.coords[mesh.cells.astype(np.int64)]
    return np.any(np.abs(X - dm.p1_coords[dm.p1_dofmap.astype(np.int64)]) > 0.5 * L + 1e-9, axis=2)
