"""The general tetrahedral test mesh of tests/general_tet_mesh.py: the conditions it has to meet, and the host
restatements on it.  No GPU.

1. Conditions (not measurements: a changed recipe has to meet them too), at the three sizes of ``SIZES``: both
   orientations hold at least a quarter of the cells; the cell volumes spread by a factor of 3 or more; the cells stay
   well shaped (cond J <= 10; the Kuhn box has 4.64), so the error bounds of the Kuhn cases carry over; no entry of any
   J^-1 is below 1e-7 of the largest of the mesh; the vertex valence is not constant and the cells of an interior patch
   differ in volume; at least half the boundary faces have a normal without a zero component.
2. The restatements the GPU tests compare against are orientation-blind: each is evaluated on the mapped mesh with the
   numbering of box_mesh (every cell positively oriented) and on the renumbered mesh (about half negatively), on the
   same analytic fields.  Dofs are matched by coordinates, cells and facets by centroid, the vertices of a cell by
   their coordinates.  Agreement: 1e-13 of the largest entry (of the column, where the columns of a result differ in
   kind), the project's figure for two float64 evaluations of one sum in another order."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import _native as nat
from dynamic_lagrangian_host import LagrangianDynamicRestatement
from dynamic_model_host import DynamicSmagorinskyRestatement
from dynamic_scalar_host import DynamicScalarRestatement
from general_tet_mesh import CUBE, SIZES, SMALL, general_tets, jacobians
from immersed_bodies import ImmersedBodies
from subgrid_models_host import VREMAN, WALE, SubgridModelRestatement
from test_derived_fields_host import CENTERS, QUANTITIES, derived_reference
from test_derived_fields_host import smooth_fields as nodal_fields
from test_flow_statistics_host import RunningStats
from test_immersed_bodies_host import BODY_NAMES, PenalisationRestatement, bodies_3d
from test_scalar_transport_host import smooth_fields
from test_variable_viscosity_host import CARREAU, SMAGORINSKY, VariableViscosityRestatement, rule_space
from test_wall_quantities_host import OPTS, boundary_facets, wall_reference

EXPECTED = {SIZES[0]: (72, 64, 175), SIZES[1]: (384, 192, 729), SIZES[2]: (900, 340, 1573)}    # cells, faces, n_p2
TOL = 1e-13


# ---------------------------------------------------------------- 1. the conditions
@pytest.mark.parametrize("size", SIZES, ids=str)
def test_mesh_meets_its_conditions(size):
    mesh, dm, marks = general_tets(*size)
    J = jacobians(mesh)
    det = np.linalg.det(J)
    Ji = np.linalg.inv(J)
    faces = np.flatnonzero(mesh.facet_on_boundary)
    assert (mesh.cells.shape[0], faces.size, dm.n_p2) == EXPECTED[size]
    negative = float((det < 0.0).mean())
    spread = float(np.abs(det).max() / np.abs(det).min())
    cond = float(np.linalg.cond(J).max())
    smallest = float(np.abs(Ji).min() / np.abs(Ji).max())
    valence = np.bincount(mesh.cells.ravel(), minlength=mesh.num_vertices())
    normals = mesh.facet_normals(faces)
    oblique = float((np.abs(normals).min(axis=1) > 1e-6).mean())
    print("%s: det J < 0 in %.3f of the cells, volume max / min %.2f, max cond J %.2f, min |J^-1| / max %.1e, valence "
          "%d .. %d, oblique boundary normals %.3f" % (size, negative, spread, cond, smallest, valence.min(),
                                                       valence.max(), oblique))
    assert 0.25 <= negative <= 0.75
    assert spread >= 3.0
    assert cond <= 10.0
    assert smallest >= 1e-7
    assert np.unique(valence).size > 1
    assert oblique >= 0.5
    # every cell is sorted (the orientation is the geometry's, not the numbering's) and every marker arrived
    assert np.all(np.diff(mesh.cells.astype(np.int64), axis=1) > 0)
    assert marks.ids() == {1, 2, 3, 4, 5, 6} and np.all(marks.values[faces] > 0) and not marks.values[~mesh.facet_on_boundary].any()
    # the cells of an interior patch differ in volume: a volume-weighted patch mean is not the plain one
    on_boundary = np.zeros(mesh.num_vertices(), dtype=bool)
    on_boundary[mesh.facets[faces].ravel()] = True
    vol = np.abs(det)
    lo, hi = np.full(mesh.num_vertices(), np.inf), np.zeros(mesh.num_vertices())
    np.minimum.at(lo, mesh.cells.ravel(), np.repeat(vol, 4))
    np.maximum.at(hi, mesh.cells.ravel(), np.repeat(vol, 4))
    assert (~on_boundary).sum() >= 2 and np.all(hi[~on_boundary] > 1.05 * lo[~on_boundary])


def test_markers_are_those_of_the_box_faces():
    """the ids were set on the box before the map and carried over by the vertices: per id, the faces of the renumbered
    mesh are those of the mesh in the numbering of box_mesh, and their number is that of the box"""
    n, lengths = SMALL
    plain = general_tets(n, lengths, renumber=False)
    mixed = general_tets(n, lengths)
    counts = {1: 2 * n[1] * n[2], 2: 2 * n[1] * n[2], 3: 2 * n[0] * n[2], 4: 2 * n[0] * n[2], 5: 2 * n[0] * n[1],
              6: 2 * n[0] * n[1]}
    for mid, count in counts.items():
        a = plain[0].facet_midpoints()[plain[2].facets_with_id(mid)]
        b = mixed[0].facet_midpoints()[mixed[2].facets_with_id(mid)]
        assert a.shape[0] == b.shape[0] == count
        assert np.abs(a[_match(a, b)] - b).max() < 1e-14


def test_planar_boundary_quads_are_on_four_faces_only():
    """on the faces 1 to 4 the map is a sum of functions of one surface coordinate each: the two triangles of a
    boundary quad stay in one plane there (an upstream search that leaves the domain through them meets the exact ties
    of a Kuhn box); on the faces 5 and 6 (the term xg * yi) no two neighbouring faces are coplanar"""
    mesh, dm, marks = general_tets(*SMALL)
    faces = np.flatnonzero(mesh.facet_on_boundary)
    normals = mesh.facet_normals(faces)
    coplanar = {mid: 0 for mid in range(1, 7)}
    pairs = {mid: 0 for mid in range(1, 7)}
    by_edge = {}
    for k, f in enumerate(faces):
        for e in mesh.facet_edges[f]:
            by_edge.setdefault(int(e), []).append(k)
    for ks in by_edge.values():
        assert len(ks) == 2
        a, b = ks
        ma, mb = int(marks.values[faces[a]]), int(marks.values[faces[b]])
        if ma != mb:
            continue
        pairs[ma] += 1
        coplanar[ma] += int(np.linalg.norm(np.cross(normals[a], normals[b])) < 1e-12)
    print("coplanar neighbouring boundary faces per id:", coplanar, "of", pairs)
    assert all(coplanar[mid] > 0 for mid in (1, 2, 3, 4)) and coplanar[5] == coplanar[6] == 0


# ---------------------------------------------------------------- 2. the restatements are orientation-blind
def _match(a, b):
    """idx with a[idx] = b up to 1e-12, a one-to-one match of two point sets"""
    dist, idx = cKDTree(a).query(b)
    assert dist.max() < 1e-12 and np.unique(idx).size == a.shape[0] == b.shape[0]
    return idx


class _Pair:
    """the mapped mesh in the numbering of box_mesh (``a``) and renumbered (``b``), their rule spaces, and the maps
    that bring a result on ``a`` into the order of ``b``"""

    def __init__(self, size):
        self.a, self.b = general_tets(*size, renumber=False), general_tets(*size)
        (ma, da, _), (mb, db, _) = self.a, self.b
        self.rs = [rule_space(m.coords, m.cells, d.p2_dofmap, d.p1_dofmap) for m, d, _ in (self.a, self.b)]
        det_a, det_b = np.linalg.det(jacobians(ma)), np.linalg.det(jacobians(mb))
        assert np.all(det_a > 0.0) and (det_b < 0.0).mean() > 0.25
        self.node = _match(da.p2_coords, db.p2_coords)
        self.vertex = _match(da.p1_coords, db.p1_coords)
        ca, cb = (m.coords[m.cells.astype(np.int64)] for m in (ma, mb))
        self.cell = _match(ca.mean(axis=1), cb.mean(axis=1))
        # local vertex j of cell c of b is local vertex self.local[c, j] of its partner in a
        same = np.all(ca[self.cell][:, None, :, :] == cb[:, :, None, :], axis=3)            # [c, j of b, i of a]
        assert np.all(same.sum(axis=2) == 1)
        self.local = np.argmax(same, axis=2)

    def velocity(self, which, fn):
        dm = (self.a, self.b)[which][1]
        return fn(dm.p2_coords)

    def vector(self, va, dim):
        """a nodal vector with ``dim`` interleaved components on ``a``, in the node order of ``b``"""
        return va.reshape(-1, dim)[self.node].ravel()


_PAIRS = {}


def _pair(size):
    if size not in _PAIRS:
        _PAIRS[size] = _Pair(size)
    return _PAIRS[size]


def _agree(label, got_b, got_a_in_b_order, per_column=False):
    a, b = np.asarray(got_a_in_b_order, dtype=np.float64), np.asarray(got_b, dtype=np.float64)
    assert a.shape == b.shape
    if per_column:
        a2, b2 = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
        scale = np.abs(b2).max(axis=0)
        assert scale.min() > 0.0, label
        err = float((np.abs(a2 - b2).max(axis=0) / scale).max())
    else:
        assert np.abs(b).max() > 0.0, label
        err = float(np.abs(a - b).max() / np.abs(b).max())
    print("%s: the two numberings differ by %.1e of the largest entry" % (label, err))
    assert err <= TOL, (label, err)


_LAWS = {"smagorinsky": (SMAGORINSKY, (0.9, )), "carreau": (CARREAU, (0.07, 1.7, 0.6)), "wale": (WALE, (2.0, )),
         "vreman": (VREMAN, (1.0, ))}
_PAIR_SIZES = (SMALL, CUBE)


@pytest.mark.parametrize("law", sorted(_LAWS))
@pytest.mark.parametrize("size", _PAIR_SIZES, ids=str)
def test_viscosity_restatements(size, law):
    """V(u) and the cell means of nu_x of laws 1, 2, 4 and 5"""
    pair = _pair(size)
    out = []
    for which in (0, 1):
        u = pair.velocity(which, lambda X: smooth_fields(X)[0])
        orc = SubgridModelRestatement(pair.rs[which], *_LAWS[law])
        out.append((orc.residual(u), orc.cell_means(u)))
    _agree("%s %s V" % (size, law), out[1][0], pair.vector(out[0][0], 3))
    _agree("%s %s cell means" % (size, law), out[1][1], out[0][1][pair.cell])


@pytest.mark.parametrize("size", _PAIR_SIZES, ids=str)
def test_wall_rows(size):
    """every row of every boundary face, constant viscosity and both laws of the wall tests"""
    pair = _pair(size)
    for law in (None, (SMAGORINSKY, (0.17, )), (CARREAU, (0.8, 1.3, 0.4))):
        rows, mids = [], []
        for mesh, dm, _ in (pair.a, pair.b):
            ids, cells, local = boundary_facets(mesh)
            u, p, T = nodal_fields(dm.p2_coords, dm.p1_coords)
            rows.append(wall_reference(mesh, dm, (cells, local), u, p, T, OPTS, law))
            mids.append(mesh.facet_midpoints()[ids])
        idx = _match(mids[0], mids[1])
        _agree("%s wall rows law %s" % (size, law and law[0]), rows[1], rows[0][idx])
        _agree("%s summed wall rows law %s" % (size, law and law[0]), rows[1].sum(axis=0), rows[0].sum(axis=0))


def _sines(X):
    K = np.array([[1.3, -0.7, 0.5], [0.9, 1.1, -0.6], [-0.8, 0.4, 1.2]])
    return (np.sin(3.0 * (X @ K.T) + np.array([0.2, 0.5, 0.9])) * np.array([1.0, 0.8, 1.2])).ravel()


def _sine_T(X):
    return 1.1 * np.sin(3.0 * (X @ np.array([1.7, -0.9, 1.4])) + 0.4) + 0.3


@pytest.mark.parametrize("size", _PAIR_SIZES, ids=str)
def test_dynamic_vertex_moments(size):
    """W, LM, MM of the dynamic Smagorinsky procedure and W, PR, RR of the dynamic heat flux per vertex, column by
    column; the global sums"""
    pair = _pair(size)
    flow, heat = [], []
    for which in (0, 1):
        dm = (pair.a, pair.b)[which][1]
        u, T = _sines(dm.p2_coords), _sine_T(dm.p2_coords)
        orc = DynamicSmagorinskyRestatement(pair.rs[which], (2.0, 0.09))
        flow.append((orc.vertices(u), orc.sums(u)))
        orc = DynamicScalarRestatement(pair.rs[which], (2.0, 0.2))
        heat.append((orc.vertices(u, T), orc.sums(u, T)))
    for name, out in (("dynamic viscosity", flow), ("dynamic heat flux", heat)):
        _agree("%s %s vertex rows" % (size, name), out[1][0], out[0][0][pair.vertex], per_column=True)
        _agree("%s %s global sums" % (size, name), out[1][1], out[0][1], per_column=True)


@pytest.mark.parametrize("size", _PAIR_SIZES, ids=str)
def test_lagrangian_initialisation(size):
    """LagrangianDynamicRestatement.apply(init=True): the state and the clipped quotient per vertex; the patch volumes
    and the patch means of Delta_K^2 the rules read"""
    pair = _pair(size)
    out = []
    for which in (0, 1):
        dm = (pair.a, pair.b)[which][1]
        orc = LagrangianDynamicRestatement(pair.rs[which], (2.0, 0.09))
        res = orc.apply(_sines(dm.p2_coords), 0.01, init=True)
        out.append((res["state"], res["cs2"], orc.patch_volume, orc.vertex_delta2))
    _agree("%s Lagrangian state" % (size, ), out[1][0], out[0][0][pair.vertex], per_column=True)
    _agree("%s Lagrangian cs2" % (size, ), out[1][1], out[0][1][pair.vertex])      # (rule 6: (cs2_init MM) / MM)
    _agree("%s patch volumes" % (size, ), out[1][2], out[0][2][pair.vertex])
    _agree("%s patch means of Delta^2" % (size, ), out[1][3], out[0][3][pair.vertex])


@pytest.mark.parametrize("size", _PAIR_SIZES, ids=str)
def test_lagrangian_advance_of_a_linear_state(size):
    """one advance from a seeded state that is a function of the position, at CFL 0.4 with the boundary at rest: the
    upstream values and the new state per vertex (the upstream cell is a geometric fact, not one of the numbering)"""
    pair = _pair(size)
    out = []
    for which in (0, 1):
        mesh, dm, _ = (pair.a, pair.b)[which]
        orc = LagrangianDynamicRestatement(pair.rs[which], (2.0, 0.09))
        X = dm.p2_coords
        u = (np.array([1.0, -0.738, -0.401])[None, :] + 0.05 * np.sin(7.0 * X + 0.3))
        u[np.unique(dm.facet_p2_nodes(np.flatnonzero(mesh.facet_on_boundary)))] = 0.0
        u = u.ravel()
        V = dm.p1_coords
        state = np.stack([0.03 * (1.5 + 0.4 * np.sin(2.0 * V[:, 0] + V[:, 2])), 1.5 + 0.4 * np.cos(1.5 * V[:, 1])], axis=1)
        k = 0.4 / np.sqrt((orc.grad ** 2).sum(axis=2)).max() / np.abs(u).max()
        res = orc.advance(orc.vertices(_sines(X)), orc.vertex_delta2, orc.vertex_velocity(u), k, state)
        moved = np.abs(orc.vertex_velocity(u)).max(axis=1) > 0.0
        assert np.all(res["tied"][moved] == 1)
        out.append((res["upstream"], res["state"]))
    _agree("%s Lagrangian upstream values" % (size, ), out[1][0], out[0][0][pair.vertex], per_column=True)
    _agree("%s Lagrangian new state" % (size, ), out[1][1], out[0][1][pair.vertex], per_column=True)


@pytest.mark.parametrize("size", _PAIR_SIZES, ids=str)
def test_derived_fields(size):
    """every quantity at every centre: CELL by centroid, VERTEX by centroid and vertex coordinates, NODE by coordinates"""
    pair = _pair(size)
    out = []
    for mesh, dm, _ in (pair.a, pair.b):
        u, p, T = nodal_fields(dm.p2_coords, dm.p1_coords)
        out.append({(q, c): derived_reference(mesh, dm, u, p, T, q, c) for q in QUANTITIES for c in CENTERS})
    for q in QUANTITIES:
        _agree("%s quantity %d CELL" % (size, q), out[1][q, nat.DERIVED_CELL], out[0][q, nat.DERIVED_CELL][pair.cell])
        va = out[0][q, nat.DERIVED_VERTEX][pair.cell]
        va = np.take_along_axis(va, pair.local[:, :, None], axis=1)
        _agree("%s quantity %d VERTEX" % (size, q), out[1][q, nat.DERIVED_VERTEX], va)
        _agree("%s quantity %d NODE" % (size, q), out[1][q, nat.DERIVED_NODE], out[0][q, nat.DERIVED_NODE][pair.node])


@pytest.mark.parametrize("size", _PAIR_SIZES, ids=str)
def test_statistics_sample(size):
    """three weighted samples of the running statistics: means and covariances per node (no geometry enters: the
    update is node by node, and so the agreement is that of the sampled fields)"""
    pair = _pair(size)
    out = []
    for mesh, dm, _ in (pair.a, pair.b):
        rs = RunningStats()
        for k, w in enumerate((0.7, 1.0, 0.3)):
            u, p, T = nodal_fields(dm.p2_coords + 0.1 * k, dm.p1_coords)
            rs.update(np.concatenate([np.reshape(u, (-1, 3)), T[:, None]], axis=1), w)
        out.append((rs.m, rs.covariance()))
    _agree("%s running means" % (size, ), out[1][0], out[0][0][pair.node])
    _agree("%s running covariances" % (size, ), out[1][1], out[0][1][pair.node])


@pytest.mark.parametrize("name", BODY_NAMES)
@pytest.mark.parametrize("size", _PAIR_SIZES, ids=str)
def test_body_residual(size, name):
    """B(u), the cell means of the mask and volume / force / torque per body, sharp and smoothed, moving bodies; the
    bodies of the GPU tests cut cells of both orientations"""
    pair = _pair(size)
    for eps in (0.0, 0.07):
        bodies = ImmersedBodies(bodies_3d(name, True), 0.037, eps)
        out = []
        for which in (0, 1):
            u = pair.velocity(which, lambda X: smooth_fields(X)[0])
            orc = PenalisationRestatement(pair.rs[which], bodies)
            out.append((orc.residual(u), orc.cell_means(), orc.forces(u)))
        _agree("%s %s eps %.2f B" % (size, name, eps), out[1][0], pair.vector(out[0][0], 3))
        _agree("%s %s eps %.2f cell means" % (size, name, eps), out[1][1], out[0][1][pair.cell])
        _agree("%s %s eps %.2f forces" % (size, name, eps), out[1][2], out[0][2])
        if eps == 0.0:
            means = out[1][1]
            cut = (means > 0.0) & (means < 1.0)
            det = np.linalg.det(jacobians(pair.b[0]))
            assert (cut & (det > 0.0)).sum() >= 4 and (cut & (det < 0.0)).sum() >= 4
