"""The periodic fixtures of tests/periodic_meshes.py: the conditions they have to meet, and the host restatements on
them.  No GPU.

1. Conditions (not measurements: a changed recipe has to meet them too), for every fixture: n_p1 is below the number
   of mesh vertices and n_p2 below that of the plain box; no cell carries a P1 or P2 dof twice; on the square and the
   cube without a wall every vertex has the interior valence (6 and 24); per periodic axis a vertex patch contains
   cells whose vertex coordinates lie more than L / 2 apart (the seam is inside a patch); a plane grouping along a
   periodic axis gives ``cells`` groups and ``cells + 1`` along a walled one; on the mapped variants the cells of every
   patch differ in volume by more than 5 %.
2. The restatements the GPU tests compare against are seam-blind.  A uniform fixture is invariant under the translation
   by one lattice spacing h along a periodic axis a, so a restatement applied to the translate u(x - h e_a) of a periodic
   nodal field must give the translate of what it gives for u: the seam moves by one column of cells relative to the
   field, and a restatement that treated the seam cells otherwise would differ there.  The translate is taken by
   permuting the nodal values (dofs matched by coordinates modulo L, cells by centroid), which is exact.  Agreement:
   1e-13 of the largest entry (of the column, where the columns differ in kind), the figure
   tests/test_general_tet_mesh_host.py asserts for the same kind of statement.
3. Fold.  For the assembled vectors (V, C T, B(u), H(T)) the periodic result equals the result on the plain box for the
   same periodic field with every slave row added to its master: 1e-13 of the largest entry.
4. The inputs of the GPU cases that had to be chosen (tests/periodic_inputs.py): the Lagrangian advance cases (one cell
   within the tie margin, nothing clamped at CFL 0.4 without a wall, the upstream cell across the seam) and the law-8
   kernel and step cases (the constant positive and unclipped on at least half the groups, at every step)."""
import numpy as np
import pytest
from scipy.spatial import cKDTree

import _native as nat
import fem_oracle as fo
from dynamic_lagrangian_host import LagrangianDynamicRestatement
from dynamic_model_host import DynamicSmagorinskyRestatement
from dynamic_scalar_host import DynamicScalarRestatement
from flow_statistics import groups_along_axis
from immersed_bodies import Ball, ImmersedBodies
from periodic_inputs import STEP_CASES, dynamic_host_steps, dynamic_kernel_case, half_unclipped, lagrangian_advance_case
from periodic_meshes import (ALL, EXPECTED, MAPPED, UNIFORM, cells_of, far_images, lengths_of, periodic_axes,
                             periodic_fields, periodic_fixture, plain_box, wall_axes, wall_bc)
from scalar_sgs_host import ScalarSgsRestatement
from subgrid_models_host import VREMAN, WALE, SubgridModelRestatement
from test_derived_fields_host import CENTERS, QUANTITIES, derived_reference
from test_flow_statistics_host import RunningStats, pooled_profiles
from test_heated_bodies_host import ScalarPenalRestatement, heated
from test_immersed_bodies_host import PenalisationRestatement
from test_scalar_transport_host import ScalarIMEXRestatement
from test_variable_viscosity_host import CARREAU, SMAGORINSKY, rule_space
from test_wall_quantities_host import OPTS, boundary_facets, wall_reference
from viscosity_models import DynamicSmagorinskyModel

TOL = 1e-13
_LAWS = {"smagorinsky": (SMAGORINSKY, (0.9, )), "carreau": (CARREAU, (0.07, 1.7, 0.6)), "wale": (WALE, (2.0, )),
         "vreman": (VREMAN, (1.0, ))}


# ---------------------------------------------------------------- 1. the conditions
@pytest.mark.parametrize("name", ALL)
def test_fixture_meets_its_conditions(name):
    mesh, dm, marks = periodic_fixture(name)
    dim = mesh._dim
    cells, L, axes = cells_of(name), np.array(lengths_of(name)), periodic_axes(name)
    plain = plain_box(name)[1]
    base = name.replace("_mapped", "")
    assert (mesh.num_vertices(), dm.n_p1, dm.n_p2, mesh.num_cells()) == EXPECTED[base]
    assert dm.n_p1 < mesh.num_vertices() == plain.n_p1 and dm.n_p2 < plain.n_p2
    for dofmap in (dm.p1_dofmap, dm.p2_dofmap):
        assert all(np.unique(row).size == row.size for row in dofmap)
    valence = np.bincount(dm.p1_dofmap.ravel(), minlength=dm.n_p1)
    assert valence.max() == (6 if dim == 2 else 24)              # (the patch bound of the operation counts: 8 / 24)
    if not wall_axes(name):
        assert np.all(valence == (6 if dim == 2 else 24))
    # the seam is inside a patch, along every periodic axis
    X = mesh.coords[mesh.cells.astype(np.int64)]
    lo, hi = np.full((dm.n_p1, dim), np.inf), np.full((dm.n_p1, dim), -np.inf)
    for j in range(dim + 1):
        np.minimum.at(lo, dm.p1_dofmap[:, j], X.min(axis=1))
        np.maximum.at(hi, dm.p1_dofmap[:, j], X.max(axis=1))
    for a in axes:
        assert ((hi - lo)[:, a] > 0.5 * L[a]).sum() >= 1
    assert far_images(name).any()
    # markers on the walls only; the Dirichlet set is empty without a wall
    ids = {mid for mid in marks.ids() if mid > 0}
    assert ids == {2 * a + 1 for a in wall_axes(name)} | {2 * a + 2 for a in wall_axes(name)}
    assert (wall_bc(name)[0].size == 0) == (not wall_axes(name))
    if name in UNIFORM:
        for a in range(dim):
            n_groups = DynamicSmagorinskyModel(("planes", a)).vertex_groups(dm.p1_coords)[0]
            assert n_groups == cells[a] + (0 if a in axes else 1), (a, n_groups)
    vol = np.abs(np.linalg.det(np.transpose(X[:, 1:] - X[:, :1], (0, 2, 1))))
    vlo, vhi = np.full(dm.n_p1, np.inf), np.zeros(dm.n_p1)
    np.minimum.at(vlo, dm.p1_dofmap.ravel(), np.repeat(vol, dim + 1))
    np.maximum.at(vhi, dm.p1_dofmap.ravel(), np.repeat(vol, dim + 1))
    print("%s: patch volume max / min %.3f .. %.3f" % (name, (vhi / vlo).min(), (vhi / vlo).max()))
    if name in MAPPED:
        assert np.all(vhi > 1.05 * vlo)
    else:
        assert np.all(vhi < (1.0 + 1e-12) * vlo)                  # (a seam cell is a translated copy of an interior one)


# ---------------------------------------------------------------- 2. the restatements are seam-blind
def _wrapped(X, L, axes):
    Y = np.array(X, dtype=np.float64)
    for a in axes:
        Y[:, a] = np.mod(Y[:, a], L[a])
        Y[np.abs(Y[:, a] - L[a]) < 1e-9, a] = 0.0
    return Y


def _source(X, shift, L, axes):
    """src with X[src[i]] = X[i] - shift modulo L, a one-to-one match"""
    dist, src = cKDTree(_wrapped(X, L, axes)).query(_wrapped(X - shift[None, :], L, axes))
    assert dist.max() < 1e-9 and np.unique(src).size == X.shape[0]
    return src


class _Shift:
    """a uniform fixture and the translation by one lattice spacing along the periodic axis ``a``: the maps that bring
    a result for u into the order of the result for the translate"""

    def __init__(self, name, a):
        self.name, self.a = name, a
        self.mesh, self.dm, self.marks = periodic_fixture(name)
        mesh, dm = self.mesh, self.dm
        self.dim = mesh._dim
        self.L, self.axes = np.array(lengths_of(name)), periodic_axes(name)
        self.shift = np.zeros(self.dim)
        self.shift[a] = self.L[a] / cells_of(name)[a]
        args = (mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
        self.s, self.rs = fo.Space(*args), rule_space(*args)
        self.node = _source(dm.p2_coords, self.shift, self.L, self.axes)
        self.vertex = _source(dm.p1_coords, self.shift, self.L, self.axes)
        centroid = mesh.coords[mesh.cells.astype(np.int64)].mean(axis=1)
        self.cell = _source(centroid, self.shift, self.L, self.axes)
        # a cell and its source carry their dofs in the same local order (the lattice is generated column by column)
        assert np.array_equal(self.node[dm.p2_dofmap], dm.p2_dofmap[self.cell])
        assert np.array_equal(self.vertex[dm.p1_dofmap], dm.p1_dofmap[self.cell])
        self.u, self.T = periodic_fields(dm.p2_coords, lengths_of(name), self.axes)
        self.p = periodic_fields(dm.p1_coords, lengths_of(name), self.axes)[1]
        self.u_t = self.u.reshape(-1, self.dim)[self.node].ravel()
        self.T_t, self.p_t = self.T[self.node], self.p[self.vertex]

    def vector(self, v, ncomp):
        return v.reshape(-1, ncomp)[self.node].ravel()


_SHIFTS = {}
_SHIFT_CASES = [(name, a) for name in UNIFORM for a in periodic_axes(name)]


def _shift(name, a):
    if (name, a) not in _SHIFTS:
        _SHIFTS[name, a] = _Shift(name, a)
    return _SHIFTS[name, a]


def _agree(label, translated, moved, per_column=False):
    a, b = np.asarray(moved, dtype=np.float64), np.asarray(translated, dtype=np.float64)
    assert a.shape == b.shape
    if per_column:
        a2, b2 = a.reshape(-1, a.shape[-1]), b.reshape(-1, b.shape[-1])
        scale = np.abs(b2).max(axis=0)
        assert scale.min() > 0.0, label
        err = float((np.abs(a2 - b2).max(axis=0) / scale).max())
    else:
        assert np.abs(b).max() > 0.0, label
        err = float(np.abs(a - b).max() / np.abs(b).max())
    print("%s: differs from the translate by %.1e of the largest entry" % (label, err))
    assert err <= TOL, (label, err)
    return err


@pytest.mark.parametrize("law", sorted(_LAWS))
@pytest.mark.parametrize("name,a", _SHIFT_CASES)
def test_viscosity_restatements_are_seam_blind(name, a, law):
    """V(u) and the cell means of nu_x of laws 1, 2, 4 and 5"""
    sh = _shift(name, a)
    orc = SubgridModelRestatement(sh.rs, *_LAWS[law])
    assert np.abs(orc.gradient(sh.u)).max(axis=(0, 1)).min() > 0.1
    _agree("%s axis %d %s V" % (name, a, law), orc.residual(sh.u_t), sh.vector(orc.residual(sh.u), sh.dim))
    _agree("%s axis %d %s cell means" % (name, a, law), orc.cell_means(sh.u_t), orc.cell_means(sh.u)[sh.cell])


@pytest.mark.parametrize("name,a", _SHIFT_CASES)
def test_dynamic_vertex_rows_and_group_sums_are_seam_blind(name, a):
    """W, LM, MM and W, PR, RR per vertex, column by column; the global sums and the sums over the plane groups along
    the OTHER axes, which a translation along ``a`` maps onto themselves"""
    sh = _shift(name, a)
    dm = sh.dm
    groupings = [None] + [DynamicSmagorinskyModel(("planes", b)).vertex_groups(dm.p1_coords) for b in range(sh.dim)
                          if b != a]
    for g in groupings:
        if g is not None:
            assert np.array_equal(np.asarray(g[1])[sh.vertex], np.asarray(g[1]))
        flow = DynamicSmagorinskyRestatement(sh.rs, (2.0, 0.09), g)
        heat = DynamicScalarRestatement(sh.rs, (2.0, 0.2), g)
        tag = "%s axis %d groups %s" % (name, a, "global" if g is None else g[0])
        if g is None:
            _agree(tag + " W LM MM", flow.vertices(sh.u_t), flow.vertices(sh.u)[sh.vertex], per_column=True)
            _agree(tag + " W PR RR", heat.vertices(sh.u_t, sh.T_t), heat.vertices(sh.u, sh.T)[sh.vertex], per_column=True)
        _agree(tag + " num den", flow.sums(sh.u_t), flow.sums(sh.u), per_column=True)
        _agree(tag + " heat num den", heat.sums(sh.u_t, sh.T_t), heat.sums(sh.u, sh.T), per_column=True)


@pytest.mark.parametrize("name,a", _SHIFT_CASES)
def test_lagrangian_initialisation_and_advance_are_seam_blind(name, a):
    """rule 6, and one advance at CFL 0.4 from a periodic positive state with the velocity of the GPU advance cases
    (every vertex with one cell within the tie margin, asserted): the upstream values and the new state"""
    sh = _shift(name, a)
    dm = sh.dm
    orc = LagrangianDynamicRestatement(sh.rs, (2.0, 0.09))
    init, init_t = orc.apply(sh.u, 0.01, init=True), orc.apply(sh.u_t, 0.01, init=True)
    _agree("%s axis %d Lagrangian state" % (name, a), init_t["state"], init["state"][sh.vertex], per_column=True)
    _agree("%s axis %d Lagrangian cs2" % (name, a), init_t["cs2"], init["cs2"][sh.vertex])
    _agree("%s axis %d patch volumes" % (name, a), orc.patch_volume, orc.patch_volume[sh.vertex])
    w, state, k, _, where = lagrangian_advance_case(name, 0.4)
    assert np.all(where["tied"][np.abs(orc.vertex_velocity(w)).max(axis=1) > 0.0] == 1)
    w_t, state_t = w.reshape(-1, sh.dim)[sh.node].ravel(), state[sh.vertex]
    out = orc.advance(orc.vertices(sh.u), orc.vertex_delta2, orc.vertex_velocity(w), k, state)
    out_t = orc.advance(orc.vertices(sh.u_t), orc.vertex_delta2, orc.vertex_velocity(w_t), k, state_t)
    # the same upstream cells (a vertex at rest -- the walls of pchan3 -- ties all its cells and takes the first)
    moved = np.abs(orc.vertex_velocity(w_t)).max(axis=1) > 0.0
    assert np.array_equal(sh.cell[out_t["cstar"]][moved], out["cstar"][sh.vertex][moved])
    _agree("%s axis %d upstream values" % (name, a), out_t["upstream"], out["upstream"][sh.vertex], per_column=True)
    _agree("%s axis %d new state" % (name, a), out_t["state"], out["state"][sh.vertex], per_column=True)


@pytest.mark.parametrize("name,a", _SHIFT_CASES)
def test_scalar_restatements_are_seam_blind(name, a):
    """C(u) T of both convective forms and the fixed subgrid heat flux D(u, T)"""
    sh = _shift(name, a)
    for form in ("standard", "skew_symmetric"):
        orc = ScalarIMEXRestatement(sh.s, 0.0, form)
        _agree("%s axis %d C T %s" % (name, a, form), orc.convection_matrix(sh.u_t) @ sh.T_t,
               (orc.convection_matrix(sh.u) @ sh.T)[sh.node])
    sgs = ScalarSgsRestatement(sh.rs, 1.0, 0.25)
    _agree("%s axis %d D" % (name, a), sgs.residual(sh.u_t, sh.T_t), sgs.residual(sh.u, sh.T)[sh.node])


def _inner_ball(sh, moved):
    """a ball half a spacing off the middle of the domain: away from the seam before and after the translation, its
    smoothing layer included (radius 0.13 + 0.05 < 0.2, the distance left on the shortest axis)"""
    centre = 0.5 * sh.L + (0.5 if moved else -0.5) * sh.shift
    return Ball(tuple(centre), 0.13, velocity=(0.3, -0.2, 0.15)[:sh.dim], angular=0.7 if sh.dim == 2 else (0.7, -0.4, 0.5))


@pytest.mark.parametrize("name,a", _SHIFT_CASES)
def test_body_restatements_are_seam_blind(name, a):
    """B(u), the cell means of the mask and H(T) with a body away from the seam that moves with the field, sharp and
    smoothed"""
    sh = _shift(name, a)
    for eps in (0.0, 0.05):
        here = ImmersedBodies(heated([_inner_ball(sh, False)]), 0.037, eps, 0.021)
        there = ImmersedBodies(heated([_inner_ball(sh, True)]), 0.037, eps, 0.021)
        flow, flow_t = PenalisationRestatement(sh.rs, here), PenalisationRestatement(sh.rs, there)
        assert flow.surface_clearance() >= 1e-9 and flow_t.surface_clearance() >= 1e-9
        # (the body's own velocity field U + W x (x - c) moves with it; the torque about the origin does not)
        _agree("%s axis %d eps %.2f B" % (name, a, eps), flow_t.residual(sh.u_t), sh.vector(flow.residual(sh.u), sh.dim))
        _agree("%s axis %d eps %.2f mask" % (name, a, eps), flow_t.cell_means(), flow.cell_means()[sh.cell])
        _agree("%s axis %d eps %.2f H" % (name, a, eps), ScalarPenalRestatement(sh.rs, there).residual(sh.T_t),
               ScalarPenalRestatement(sh.rs, here).residual(sh.T)[sh.node])


@pytest.mark.parametrize("name,a", _SHIFT_CASES)
def test_derived_fields_are_seam_blind(name, a):
    """every quantity at every centre; the fields hold no coordinate, so the translate of the result is the result of
    the translate"""
    sh = _shift(name, a)
    mesh, dm = sh.mesh, sh.dm
    u, u_t = sh.u.reshape(-1, sh.dim), sh.u_t.reshape(-1, sh.dim)
    for q in QUANTITIES:
        for c in CENTERS:
            moved = derived_reference(mesh, dm, u, sh.p, sh.T, q, c)
            moved = moved[sh.node] if c == nat.DERIVED_NODE else moved[sh.cell]
            _agree("%s axis %d quantity %d centre %d" % (name, a, q, c),
                   derived_reference(mesh, dm, u_t, sh.p_t, sh.T_t, q, c), moved)


@pytest.mark.parametrize("name,a", _SHIFT_CASES)
def test_pooled_profiles_are_seam_blind(name, a):
    """three weighted samples pooled over the planes of nodes along every OTHER axis (flow_statistics.groups_along_axis
    on the coordinates stored for the dofs, the grouping of the GPU profile case): a plane holds one image of every
    periodic node, a translation along ``a`` maps it onto itself, and the pooled means and covariances stay (the
    node-by-node accumulation itself reads no mesh and cannot tell a seam)"""
    sh = _shift(name, a)
    dm = sh.dm
    for b in range(sh.dim):
        if b == a:
            continue
        _, ptr, nodes = groups_along_axis(dm.p2_coords, b)
        planes = 2 * cells_of(name)[b] + (0 if b in sh.axes else 1)
        assert len(ptr) - 1 == planes and np.all(np.diff(ptr) == dm.n_p2 // planes)
        assert np.array_equal(np.sort(sh.node[nodes].reshape(planes, -1), axis=1), nodes.reshape(planes, -1))
        out = []
        for u, T in ((sh.u, sh.T), (sh.u_t, sh.T_t)):
            rs = RunningStats()
            for k, w in enumerate((0.7, 1.0, 0.3)):
                rs.update(np.concatenate([(1.0 + 0.2 * k) * u.reshape(-1, sh.dim), (T + 0.1 * k * T * T)[:, None]], axis=1), w)
            out.append(pooled_profiles(rs.m, rs.covariance(), sh.dim, ptr, nodes, np.ones(len(nodes)))[:2])
        # (a mean over a whole period cancels: the error is relative to the sum of the absolute contributions)
        err = float((np.abs(out[1][0] - out[0][0]) / out[0][1]).max())
        print("%s axis %d profiles along %d: differ by %.1e of the absolute contributions" % (name, a, b, err))
        assert out[0][1].min() > 0.0 and err <= TOL


def _facet_midpoints(mesh, cells, local):
    X = mesh.coords[mesh.cells.astype(np.int64)[cells]]
    keep = np.arange(X.shape[1])[None, :] != np.asarray(local)[:, None]
    return (X * keep[:, :, None]).sum(axis=1) / (X.shape[1] - 1)


@pytest.mark.parametrize("name,a", _SHIFT_CASES)
def test_wall_rows_are_seam_blind(name, a):
    """every row of every boundary face (walls and periodic sides, the set of the GPU cases), constant viscosity and
    the Smagorinsky law: the rows of the translate on the face (c, l) are those of the field on the face (source of c,
    l) -- an interior face where c is a seam cell --, the torque about the fixed origin moved by delta x (force), delta
    the distance of the two faces' midpoints"""
    sh = _shift(name, a)
    mesh, dm, dim = sh.mesh, sh.dm, sh.dim
    ids, cells, local = boundary_facets(mesh)
    src = sh.cell[cells]
    delta = _facet_midpoints(mesh, cells, local) - _facet_midpoints(mesh, src, local)
    assert np.abs(np.abs(delta[:, a]) - np.where(np.abs(delta[:, a]) > 0.5 * sh.L[a], sh.L[a] - sh.shift[a], sh.shift[a])).max() < 1e-12
    assert (np.abs(delta[:, a]) > 0.5 * sh.L[a]).sum() >= 2                  # (faces whose source lies across the seam)
    u, u_t = sh.u.reshape(-1, dim), sh.u_t.reshape(-1, dim)
    for law in (None, (SMAGORINSKY, (0.17, ))):
        rows_t = wall_reference(mesh, dm, (cells, local), u_t, sh.p_t, sh.T_t, OPTS, law)
        rows = wall_reference(mesh, dm, (src, local), u, sh.p, sh.T, OPTS, law).copy()
        force = rows[:, 1:1 + dim] + rows[:, 1 + dim:1 + 2 * dim]
        if dim == 2:
            rows[:, 4 + 2 * dim] += delta[:, 0] * force[:, 1] - delta[:, 1] * force[:, 0]
        else:
            rows[:, 4 + 2 * dim:] += np.cross(delta, force)
        _agree("%s axis %d wall rows law %s" % (name, a, law and law[0]), rows_t, rows, per_column=True)


# ---------------------------------------------------------------- 3. fold
@pytest.mark.parametrize("name", ALL)
def test_assembled_vectors_are_the_folded_plain_ones(name):
    """V of laws 1, 2, 4, 5, C T, D, B(u) and H(T) on the periodic dof map against the same restatement on the plain
    box of the same cells, fed the same periodic field, every slave row added to its master"""
    mesh, dm, _ = periodic_fixture(name)
    pmesh, pdm = plain_box(name)
    dim = mesh._dim
    L, axes = np.array(lengths_of(name)), periodic_axes(name)
    assert np.array_equal(pmesh.cells, mesh.cells) and np.array_equal(pmesh.coords, mesh.coords)
    if name in MAPPED:
        # (on a mapped mesh the nodes are matched through the cells: the images of a node differ by the displacement)
        to = np.full(pdm.n_p2, -1, dtype=np.int64)
        to[pdm.p2_dofmap.ravel()] = dm.p2_dofmap.ravel()
    else:
        dist, to = cKDTree(_wrapped(dm.p2_coords, L, axes)).query(_wrapped(pdm.p2_coords, L, axes))
        assert dist.max() < 1e-9
    assert np.array_equal(to[pdm.p2_dofmap], dm.p2_dofmap) and np.unique(to).size == dm.n_p2
    spaces = []
    for m, d in ((mesh, dm), (pmesh, pdm)):
        args = (m.coords, m.cells, d.p2_dofmap, d.p1_dofmap)
        spaces.append((fo.Space(*args), rule_space(*args)))
    u, T = periodic_fields(dm.p2_coords, lengths_of(name), axes)
    u_plain, T_plain = u.reshape(-1, dim)[to].ravel(), T[to]

    def fold(v, ncomp):
        out = np.zeros((dm.n_p2, ncomp))
        np.add.at(out, to, v.reshape(-1, ncomp))
        return out.ravel()

    ball = Ball(tuple(0.5 * L), 0.17, velocity=(0.3, -0.2, 0.15)[:dim], angular=0.7 if dim == 2 else (0.7, -0.4, 0.5))
    seam = Ball((0.0, ) + tuple(0.45 * L[1:]), 0.19)
    bodies = ImmersedBodies(heated([ball, seam]), 0.037, 0.07, 0.021)
    worst = 0.0
    (s, rs), (ps, prs) = spaces
    for law in sorted(_LAWS):
        got = SubgridModelRestatement(rs, *_LAWS[law]).residual(u)
        want = fold(SubgridModelRestatement(prs, *_LAWS[law]).residual(u_plain), dim)
        worst = max(worst, _agree("%s fold V %s" % (name, law), got, want))
    for form in ("standard", "skew_symmetric"):
        got = ScalarIMEXRestatement(s, 0.0, form).convection_matrix(u) @ T
        want = fold(ScalarIMEXRestatement(ps, 0.0, form).convection_matrix(u_plain) @ T_plain, 1)
        worst = max(worst, _agree("%s fold C T %s" % (name, form), got, want))
    worst = max(worst, _agree("%s fold D" % name, ScalarSgsRestatement(rs, 1.0, 0.25).residual(u, T),
                              fold(ScalarSgsRestatement(prs, 1.0, 0.25).residual(u_plain, T_plain), 1)))
    worst = max(worst, _agree("%s fold B" % name, PenalisationRestatement(rs, bodies).residual(u),
                              fold(PenalisationRestatement(prs, bodies).residual(u_plain), dim)))
    worst = max(worst, _agree("%s fold H" % name, ScalarPenalRestatement(rs, bodies).residual(T),
                              fold(ScalarPenalRestatement(prs, bodies).residual(T_plain), 1)))
    print("%s: fold, worst %.1e" % (name, worst))


# ---------------------------------------------------------------- 4. the chosen inputs of the GPU cases
@pytest.mark.parametrize("cfl", (0.4, 2.5))
@pytest.mark.parametrize("name", ALL)
def test_inputs_of_the_lagrangian_advance_cases(name, cfl):
    """tests/periodic_inputs.py, on the restatement alone: no vertex at rest but the wall vertices of pchan3, one cell
    within the tie margin at every displaced vertex, nothing clamped at CFL 0.4 where there is no wall and clamped
    vertices at CFL 2.5, the upstream cell across the seam for at least a quarter of the displaced seam vertices"""
    u, state, k, orc, where = lagrangian_advance_case(name, cfl)
    dm = periodic_fixture(name)[1]
    moved = np.abs(orc.vertex_velocity(u)).max(axis=1) > 0.0
    assert moved.sum() == (dm.n_p1 if name != "pchan3" else 9) and (state > 0.0).all() and k > 0.0
    assert np.all(where["tied"][moved] == 1) and (where["best"] - where["second"])[moved].min() > 1e-9
    if cfl < 1.0:
        assert not where["clamped"].any() or wall_axes(name)
    else:
        assert where["clamped"].sum() >= 2
    print("%s CFL %.1f: %d clamped, %d displaced seam vertices, upstream cell across the seam at %d" % (
        name, cfl, where["clamped"].sum(), where["seam"].sum(), where["across"].sum()))
    assert where["seam"].sum() >= 4 and 4 * where["across"].sum() >= where["seam"].sum()


@pytest.mark.parametrize("name", ALL)
def test_inputs_of_the_law_8_kernel_cases(name):
    """the restatement alone gives a positive, unclipped constant on at least half the groups"""
    grouping, u, orc, own = dynamic_kernel_case(name)
    print("%s %s: cs2 %s" % (name, grouping, np.array2string(own, precision=4)))
    assert own.max() > 1e-3 and 2 * ((own > 0.0) & (own < 0.09)).sum() >= own.size


@pytest.mark.parametrize("name", sorted(STEP_CASES))
def test_inputs_of_the_law_8_step_cases(name):
    """at every step of the restatement: half the groups positive and unclipped, one of them between 0.2 and 0.8 of
    the clip, and the term moves u* by at least 1e-4"""
    cs2_max = STEP_CASES[name][2]
    for i, h in enumerate(dynamic_host_steps(name)):
        print("%s step %d: cs2 / cs2_max %s, effect on u* %.2e" % (name, i, np.array2string(h["cs2"] / cs2_max, precision=3),
                                                               h["effect"]))
        assert half_unclipped(h["cs2"], cs2_max), (name, i, h["cs2"])
        assert ((h["cs2"] > 0.2 * cs2_max) & (h["cs2"] < 0.8 * cs2_max)).any() and h["effect"] >= 1e-4
