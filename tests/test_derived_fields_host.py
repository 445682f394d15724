"""Host side of the gradient-derived fields (nsfem_derived_fields, csrc/derived.hip): the numpy restatement
``derived_reference`` -- the yardstick of tests/test_gpu_derived_fields.py -- pinned against analytic values of
polynomial fields, against the existing host path (``ProblemBase._cell_gradients``) and against pointwise identities.
No GPU.

The restatement evaluates G_ab = d_b u_a at every point directly from the P2 basis gradients at THAT point (vertices,
edge midpoints, points of the degree-5 rule), cell by cell with einsums -- a different route from the kernel's, which
forms G at the vertices and combines those barycentrically.

Tolerance (derived, the rule of the volume-functional and statistics tests: terms in the sum x 2^-53 x the sum of the
absolute contributions of that entry, doubled for the restatement's own rounding).  ``derived_reference(...,
absolute=True)`` runs the same sums with |J^-1|, |d phi|, |u|, |p|, |T| and with every difference of the quantity
formulas turned into a sum: entry by entry it returns the sum of the absolute contributions A.  ``n_terms`` counts the
rounded operations along the longest chain that ends in an entry:
    geometry (differences, determinant, cofactors, division)      6 (2D) / 12 (3D)
    reference gradient at a point: N2 products and additions (+ 2: the tabulated coordinates)   N2 + 2
    physical gradient: dim products and additions, + 1            dim + 1
    barycentric combination of vertex gradients (device)          dim + 2
  = n_G;  a quantity linear in G adds dim;  Q and gamma are quadratic in G: 2 n_G + dim^2 + 1 (the error of gamma is
  bounded through Cauchy-Schwarz by n eps sqrt(2 S^:S^), S^ from the absolute sums, however small gamma itself is);
    CELL: the rule's NQ terms, weight, division                   NQ + 2
    NODE: the longest run L of cells around a node, for numerator and denominator, |K| (geometry + 1), division
                                                                  2 (L + n_geo + 1) + 1
``bound = 2 n_terms 2^-53 A`` per entry."""
import os

import numpy as np
import pytest

import _native as nat
from fem_mesh import TaylorHoodDofMap, box_mesh, rectangle_mesh
from ns_problem import ProblemBase

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -53
QUANTITIES = (nat.DERIVED_VORTICITY, nat.DERIVED_DIVERGENCE, nat.DERIVED_SHEAR_RATE, nat.DERIVED_Q_CRITERION,
              nat.DERIVED_VELOCITY_GRADIENT, nat.DERIVED_PRESSURE_GRADIENT, nat.DERIVED_SCALAR_GRADIENT)
CENTERS = (nat.DERIVED_CELL, nat.DERIVED_VERTEX, nat.DERIVED_NODE)
LINEAR = (nat.DERIVED_VORTICITY, nat.DERIVED_DIVERGENCE, nat.DERIVED_VELOCITY_GRADIENT, nat.DERIVED_PRESSURE_GRADIENT,
          nat.DERIVED_SCALAR_GRADIENT)
EDGES = {2: ((1, 2), (0, 2), (0, 1)), 3: ((2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1))}


# ---------------------------------------------------------------- the restatement
def degree5_rule(dim):
    """(barycentric points [q, dim + 1], weights [q]) of the degree-5 rules of the element kernels: Radon's 7 points
    on the triangle, Keast's 15 points on the tetrahedron"""
    s15 = np.sqrt(15.0)
    if dim == 2:
        a1, a2 = (6.0 - s15) / 21.0, (6.0 + s15) / 21.0
        w1, w2 = (155.0 - s15) / 2400.0, (155.0 + s15) / 2400.0
        pts = [(1.0 / 3.0, 1.0 / 3.0), (a1, a1), (1.0 - 2.0 * a1, a1), (a1, 1.0 - 2.0 * a1),
               (a2, a2), (1.0 - 2.0 * a2, a2), (a2, 1.0 - 2.0 * a2)]
        wts = [9.0 / 80.0, w1, w1, w1, w2, w2, w2]
    else:
        a1, a2, b = (7.0 - s15) / 34.0, (7.0 + s15) / 34.0, (10.0 - 2.0 * s15) / 40.0
        w0, w1, w2, w3 = 16.0 / 135.0, (2665.0 + 14.0 * s15) / 37800.0, (2665.0 - 14.0 * s15) / 37800.0, 10.0 / 189.0
        pts, wts = [(0.25, 0.25, 0.25)], [w0 / 6.0]
        for a, w in ((a1, w1), (a2, w2)):
            c = 1.0 - 3.0 * a
            pts += [(a, a, a), (c, a, a), (a, c, a), (a, a, c)]
            wts += [w / 6.0] * 4
        c = 0.5 - b
        pts += [(b, b, c), (b, c, b), (c, b, b), (b, c, c), (c, b, c), (c, c, b)]
        wts += [w3 / 6.0] * 6
    pts = np.array(pts)
    return np.concatenate([1.0 - pts.sum(axis=1, keepdims=True), pts], axis=1), np.array(wts)


def local_points(dim, center):
    """barycentric coordinates [q, dim + 1] of the points a centre evaluates in every cell"""
    if center == nat.DERIVED_CELL:
        return degree5_rule(dim)[0]
    lam = np.eye(dim + 1)
    if center == nat.DERIVED_VERTEX:
        return lam
    return np.concatenate([lam, [0.5 * (lam[a] + lam[b]) for a, b in EDGES[dim]]], axis=0)


def p2_reference_gradients(lam):
    """d phi_k / d xi_b of the P2 basis (vertices, then the edges in UFC order) at the points lam: [q, N2, dim]"""
    dim = lam.shape[1] - 1
    dl = np.concatenate([-np.ones((1, dim)), np.eye(dim)], axis=0)
    out = np.zeros((lam.shape[0], dim + 1 + len(EDGES[dim]), dim))
    for i in range(dim + 1):
        out[:, i] = (4.0 * lam[:, i:i + 1] - 1.0) * dl[i]
    for e, (a, b) in enumerate(EDGES[dim]):
        out[:, dim + 1 + e] = 4.0 * (lam[:, a:a + 1] * dl[b] + lam[:, b:b + 1] * dl[a])
    return out


def point_gradients(mesh, dm, u, p, T, center, absolute=False):
    """(G [c, q, a, b] = d_b u_a, gp [c, b], gT [c, q, b], vol [c]) at the points of ``center``; ``absolute``: the same
    sums over the absolute values of every factor"""
    dim = dm.dim
    mod = np.abs if absolute else (lambda a: a)
    x = np.asarray(mesh.coords, dtype=np.float64)[np.asarray(mesh.cells, dtype=np.int64)]
    J = np.stack([x[:, k + 1] - x[:, 0] for k in range(dim)], axis=2)
    JinvT = mod(np.transpose(np.linalg.inv(J), (0, 2, 1)))
    vol = np.abs(np.linalg.det(J)) / (2.0 if dim == 2 else 6.0)
    dphi2 = mod(p2_reference_gradients(local_points(dim, center)))
    dl = mod(np.concatenate([-np.ones((1, dim)), np.eye(dim)], axis=0))
    g2 = np.einsum("cab,qkb->cqka", JinvT, dphi2)
    p2 = np.asarray(dm.p2_dofmap, dtype=np.int64)
    ue = mod(np.asarray(u, dtype=np.float64).reshape(-1, dim)[p2])
    G = np.einsum("cqkb,cka->cqab", g2, ue)
    gp = np.einsum("cab,kb,ck->ca", JinvT, dl, mod(np.asarray(p, dtype=np.float64)[np.asarray(dm.p1_dofmap, np.int64)]))
    if T is None:
        gT = np.zeros(G.shape[:2] + (dim, ))
    else:
        gT = np.einsum("cqkb,ck->cqb", g2, mod(np.asarray(T, dtype=np.float64)[p2]))
    return G, gp, gT, vol


def quantity_at_points(G, gp, gT, quantity, absolute=False):
    """[c, q, ncomp] of one quantity from the gradients at the points; ``absolute``: differences become sums"""
    dim = G.shape[2]
    sgn = 1.0 if absolute else -1.0
    if quantity == nat.DERIVED_VORTICITY:
        if dim == 2:
            return (G[..., 1, 0] + sgn * G[..., 0, 1])[..., None]
        return np.stack([G[..., 2, 1] + sgn * G[..., 1, 2], G[..., 0, 2] + sgn * G[..., 2, 0],
                         G[..., 1, 0] + sgn * G[..., 0, 1]], axis=-1)
    if quantity == nat.DERIVED_DIVERGENCE:
        return np.trace(G, axis1=2, axis2=3)[..., None]
    if quantity == nat.DERIVED_SHEAR_RATE:
        s = G + np.swapaxes(G, 2, 3)
        return np.sqrt(0.5 * (s ** 2).sum(axis=(2, 3)))[..., None]
    if quantity == nat.DERIVED_Q_CRITERION:
        return (0.5 * sgn * np.einsum("cqab,cqba->cq", G, G))[..., None]
    if quantity == nat.DERIVED_VELOCITY_GRADIENT:
        return G.reshape(G.shape[:2] + (dim * dim, ))
    if quantity == nat.DERIVED_PRESSURE_GRADIENT:
        return np.broadcast_to(gp[:, None, :], G.shape[:2] + (dim, )).copy()
    if quantity == nat.DERIVED_SCALAR_GRADIENT:
        return gT
    raise ValueError(quantity)


def derived_reference(mesh, dm, u, p, T, quantity, center, absolute=False):
    """One quantity at one centre, in the layout of nsfem_derived_fields with the component axis kept: CELL
    [n_cells, ncomp], VERTEX [n_cells, dim + 1, ncomp], NODE [n_p2, ncomp].  u [n_p2, dim] (or flat), p [n_p1], T
    [n_p2] or None.  ``absolute``: the sum of the absolute contributions of every entry instead"""
    G, gp, gT, vol = point_gradients(mesh, dm, u, p, T, center, absolute)
    q = quantity_at_points(G, gp, gT, quantity, absolute)
    if center == nat.DERIVED_VERTEX:
        return q
    if center == nat.DERIVED_CELL:
        w = degree5_rule(dm.dim)[1]
        return np.einsum("q,cqj->cj", w, q) / w.sum()
    p2 = np.asarray(dm.p2_dofmap, dtype=np.int64)
    num = np.zeros((dm.n_p2, q.shape[2]))
    den = np.zeros(dm.n_p2)
    np.add.at(num, p2.ravel(), (vol[:, None, None] * q).reshape(-1, q.shape[2]))
    np.add.at(den, p2.ravel(), np.repeat(vol, p2.shape[1]))
    return num / den[:, None]


def n_terms(dm, quantity, center):
    """rounded operations along the longest chain that ends in an entry (module docstring)"""
    dim = dm.dim
    n2 = 6 if dim == 2 else 10
    n_geo = 6 if dim == 2 else 12
    n = n_geo + (n2 + 2) + (dim + 1) + (dim + 2)
    n = n + dim if quantity in LINEAR else 2 * n + dim * dim + 1
    if center == nat.DERIVED_CELL:
        n += (7 if dim == 2 else 15) + 2
    elif center == nat.DERIVED_NODE:
        longest = int(np.bincount(np.asarray(dm.p2_dofmap).ravel(), minlength=dm.n_p2).max())
        n += 2 * (longest + n_geo + 1) + 1
    return n


def derived_bound(mesh, dm, u, p, T, quantity, center):
    """per-entry tolerance: 2 n_terms 2^-53 x the sum of the absolute contributions"""
    return 2.0 * n_terms(dm, quantity, center) * EPS * derived_reference(mesh, dm, u, p, T, quantity, center, True)


# ---------------------------------------------------------------- meshes and fields
def host_meshes():
    from mesh_io import read_msh
    return {"rectangle": rectangle_mesh((0.0, 0.0), (1.5, 1.0), 6, 4),
            "box": box_mesh((0.0, 0.0, 0.0), (1.5, 1.0, 1.0), 3, 2, 2),
            "fixture": read_msh(os.path.join(HERE, "golden", "square_v41.msh"))[0]}


def polynomial_fields(dim):
    """quadratic velocity, linear pressure, quadratic scalar as coefficient sets: f(x) = c + b.x + x^T A x, A
    symmetric; returns (list of dim (c, b, A) for u, (c, b) for p, (c, b, A) for T)"""
    rng = np.random.default_rng(11 + dim)

    def quad():
        A = rng.uniform(-1.0, 1.0, (dim, dim))
        return rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0, dim), 0.5 * (A + A.T)

    return [quad() for _ in range(dim)], (rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0, dim)), quad()


def eval_quadratic(coef, X):
    c, b, A = coef
    return c + X @ b + np.einsum("na,ab,nb->n", X, A, X)


def grad_quadratic(coef, X):
    _, b, A = coef
    return b[None, :] + 2.0 * X @ A


def polynomial_nodal(dm, poly):
    cu, cp, cT = poly
    u = np.stack([eval_quadratic(c, dm.p2_coords) for c in cu], axis=1)
    p = cp[0] + dm.p1_coords @ cp[1]
    return u, p, eval_quadratic(cT, dm.p2_coords)


def analytic(mesh, dm, poly, quantity, center):
    """the exact values of the polynomial fields in the layout of ``derived_reference``; None where there is no
    closed form (the cell mean of the shear rate).

    The quantities are formed from the exact gradients with the restatement's own ``quantity_at_points``: the
    polynomial test therefore pins the GRADIENTS (basis derivatives, geometry, node order, the three centrings) and
    not the quantity formulas.  Those -- the sign of the vorticity, the formula of Q, the factor in gamma -- are pinned
    by ``test_rigid_rotation`` (closed forms), by the identities test (formulas written out independently from the
    velocity gradient) and by the comparison with ``ProblemBase._compute_vorticity``."""
    dim = dm.dim
    cu, cp, cT = poly

    def at(X):      # X [..., dim] -> G [..., a, b], gp [..., b], gT [..., b]
        flat = X.reshape(-1, dim)
        G = np.stack([grad_quadratic(c, flat) for c in cu], axis=1)
        return (G.reshape(X.shape[:-1] + (dim, dim)), np.broadcast_to(cp[1], X.shape).copy(),
                grad_quadratic(cT, flat).reshape(X.shape))

    xv = np.asarray(mesh.coords, dtype=np.float64)[np.asarray(mesh.cells, dtype=np.int64)]      # [c, dim + 1, dim]
    if center == nat.DERIVED_NODE:
        G, gp, gT = at(dm.p2_coords[:, None, :])
        return quantity_at_points(G, gp[:, 0], gT, quantity)[:, 0]
    G, gp, gT = at(xv)
    q = quantity_at_points(G, gp[:, 0], gT, quantity)
    if center == nat.DERIVED_VERTEX:
        return q
    if quantity in LINEAR:
        return q.mean(axis=1)                       # the mean of a linear function: the mean of its vertex values
    if quantity == nat.DERIVED_Q_CRITERION:
        # mean over a simplex of f g, both linear: (sum_i f_i g_i + sum_i f_i sum_j g_j) / ((d + 1)(d + 2))
        s = np.einsum("cvab,cvba->c", G, G) + np.einsum("cab,cba->c", G.sum(axis=1), G.sum(axis=1))
        return (-0.5 * s / ((dim + 1) * (dim + 2)))[:, None]
    return None


# ---------------------------------------------------------------- polynomial fields: the restatement is exact
@pytest.mark.parametrize("name", ["rectangle", "box", "fixture"])
def test_restatement_reproduces_polynomial_fields(name):
    mesh = host_meshes()[name]
    dm = TaylorHoodDofMap(mesh)
    poly = polynomial_fields(dm.dim)
    u, p, T = polynomial_nodal(dm, poly)
    checked = 0
    for center in CENTERS:
        for quantity in QUANTITIES:
            want = analytic(mesh, dm, poly, quantity, center)
            if want is None:
                assert quantity == nat.DERIVED_SHEAR_RATE and center == nat.DERIVED_CELL
                continue
            got = derived_reference(mesh, dm, u, p, T, quantity, center)
            bound = derived_bound(mesh, dm, u, p, T, quantity, center)
            assert got.shape == want.shape == bound.shape
            excess = np.abs(got - want) - bound
            print("%s centre %d quantity %d: max error %.3e, max error / bound %.3f"
                  % (name, center, quantity, np.abs(got - want).max(), (np.abs(got - want) / bound).max()))
            assert (excess <= 0.0).all(), (name, center, quantity, excess.max())
            checked += 1
    assert checked == 20


def test_shapes_and_component_counts():
    for name, mesh in host_meshes().items():
        dm = TaylorHoodDofMap(mesh)
        dim = dm.dim
        u, p, T = polynomial_nodal(dm, polynomial_fields(dim))
        ncomp = {nat.DERIVED_VORTICITY: 1 if dim == 2 else 3, nat.DERIVED_DIVERGENCE: 1, nat.DERIVED_SHEAR_RATE: 1,
                 nat.DERIVED_Q_CRITERION: 1, nat.DERIVED_VELOCITY_GRADIENT: dim * dim,
                 nat.DERIVED_PRESSURE_GRADIENT: dim, nat.DERIVED_SCALAR_GRADIENT: dim}
        nc = mesh.cells.shape[0]
        for q in QUANTITIES:
            assert derived_reference(mesh, dm, u, p, T, q, nat.DERIVED_CELL).shape == (nc, ncomp[q])
            assert derived_reference(mesh, dm, u, p, T, q, nat.DERIVED_VERTEX).shape == (nc, dim + 1, ncomp[q])
            assert derived_reference(mesh, dm, u, p, T, q, nat.DERIVED_NODE).shape == (dm.n_p2, ncomp[q])


# ---------------------------------------------------------------- the existing host path
class _HostProblem(ProblemBase):
    """just enough of a problem for ``_compute_vorticity`` / ``_compute_pressure_gradient`` on given nodal values"""

    class _Nodal:
        def __init__(self, values):
            self._values = values

        def nodal_values(self):
            return self._values

    class _Solver:
        pass

    def __init__(self, mesh, dm, u, p):
        self._mesh = mesh
        self._solver = self._Solver()
        self._solver._dofmap = dm
        self._u, self._p = self._Nodal(u), self._Nodal(p)

    def _get_solver(self):
        return self._solver

    def _get_velocity(self):
        return self._u

    def _get_pressure(self):
        return self._p


def smooth_fields(X2, X1):
    """smooth, non-polynomial (u [n2, dim], p [n1], T [n2])"""
    dim = X2.shape[1]
    x, y = X2[:, 0], X2[:, 1]
    z = X2[:, 2] if dim == 3 else np.zeros_like(x)
    u = [np.sin(1.3 * x + 0.7) * np.cos(0.9 * y + 0.2) + 0.3 * z + 0.8 * np.sin(0.9 * x),
         np.cos(0.8 * x - 0.4) * (1.0 + y) - 0.2 * z * z + 0.5 * np.sin(2.1 * y)]
    if dim == 3:
        u.append(np.sin(x + y + z + 0.3) - 0.25 * np.cos(1.7 * x * y))
    T = 1.0 + 0.5 * np.cos(1.1 * x + 0.5) * np.sin(0.7 * y - 0.3) + 0.2 * np.sin(1.9 * z)
    x1, y1 = X1[:, 0], X1[:, 1]
    p = np.sin(0.6 * x1 + 0.9) + y1 * np.cos(1.5 * x1) + (0.3 * np.sin(1.2 * X1[:, 2]) if dim == 3 else 0.0)
    return np.stack(u, axis=1), p, T


@pytest.mark.parametrize("name", ["rectangle", "box", "fixture"])
def test_restatement_equals_the_cell_gradients_path(name):
    mesh = host_meshes()[name]
    dm = TaylorHoodDofMap(mesh)
    u, p, T = smooth_fields(dm.p2_coords, dm.p1_coords)
    problem = _HostProblem(mesh, dm, u, p)
    vort = problem._compute_vorticity()
    want = vort.vertex_values.reshape(mesh.cells.shape[0], dm.dim + 1, -1)
    got = derived_reference(mesh, dm, u, p, T, nat.DERIVED_VORTICITY, nat.DERIVED_VERTEX)
    bound = derived_bound(mesh, dm, u, p, T, nat.DERIVED_VORTICITY, nat.DERIVED_VERTEX)
    assert got.shape == want.shape and (np.abs(got - want) <= bound).all()
    # the stored cell value of the host path is the mean of the vertex values = the cell mean of a linear function
    got = derived_reference(mesh, dm, u, p, T, nat.DERIVED_VORTICITY, nat.DERIVED_CELL)
    bound = derived_bound(mesh, dm, u, p, T, nat.DERIVED_VORTICITY, nat.DERIVED_CELL)
    assert (np.abs(got - vort.values.reshape(got.shape)) <= bound).all()
    want = problem._compute_pressure_gradient().values
    got = derived_reference(mesh, dm, u, p, T, nat.DERIVED_PRESSURE_GRADIENT, nat.DERIVED_CELL)
    bound = derived_bound(mesh, dm, u, p, T, nat.DERIVED_PRESSURE_GRADIENT, nat.DERIVED_CELL)
    assert got.shape == want.shape and (np.abs(got - want) <= bound).all()


# ---------------------------------------------------------------- identities
@pytest.mark.parametrize("name", ["rectangle", "box"])
@pytest.mark.parametrize("center", CENTERS)
def test_vorticity_divergence_and_q_follow_from_the_velocity_gradient(name, center):
    mesh = host_meshes()[name]
    dm = TaylorHoodDofMap(mesh)
    dim = dm.dim
    u, p, T = smooth_fields(dm.p2_coords, dm.p1_coords)
    ref = lambda q: derived_reference(mesh, dm, u, p, T, q, center)
    bnd = lambda q: derived_bound(mesh, dm, u, p, T, q, center)
    G = ref(nat.DERIVED_VELOCITY_GRADIENT)
    G = G.reshape(G.shape[:-1] + (dim, dim))
    if dim == 2:
        curl = (G[..., 1, 0] - G[..., 0, 1])[..., None]
    else:
        curl = np.stack([G[..., 2, 1] - G[..., 1, 2], G[..., 0, 2] - G[..., 2, 0], G[..., 1, 0] - G[..., 0, 1]], axis=-1)
    assert (np.abs(ref(nat.DERIVED_VORTICITY) - curl) <= bnd(nat.DERIVED_VORTICITY)).all()
    div = np.trace(G, axis1=-2, axis2=-1)[..., None]
    assert (np.abs(ref(nat.DERIVED_DIVERGENCE) - div) <= bnd(nat.DERIVED_DIVERGENCE)).all()
    if center == nat.DERIVED_VERTEX:      # (a mean of products is not the product of means: pointwise only)
        Q = (-0.5 * np.einsum("...ab,...ba->...", G, G))[..., None]
        assert (np.abs(ref(nat.DERIVED_Q_CRITERION) - Q) <= bnd(nat.DERIVED_Q_CRITERION)).all()
        S = 0.5 * (G + np.swapaxes(G, -1, -2))
        W = 0.5 * (G - np.swapaxes(G, -1, -2))
        Q2 = (0.5 * ((W ** 2).sum(axis=(-1, -2)) - (S ** 2).sum(axis=(-1, -2))))[..., None]
        assert (np.abs(ref(nat.DERIVED_Q_CRITERION) - Q2) <= 2.0 * bnd(nat.DERIVED_Q_CRITERION)).all()
        gamma = np.sqrt(2.0 * (S ** 2).sum(axis=(-1, -2)))[..., None]
        assert (np.abs(ref(nat.DERIVED_SHEAR_RATE) - gamma) <= bnd(nat.DERIVED_SHEAR_RATE)).all()


@pytest.mark.parametrize("name", ["rectangle", "box", "fixture"])
def test_a_constant_velocity_gives_zeros(name):
    mesh = host_meshes()[name]
    dm = TaylorHoodDofMap(mesh)
    u = np.tile(np.array([0.7, -1.3, 0.4])[:dm.dim], (dm.n_p2, 1))
    p, T = np.full(dm.n_p1, 2.5), np.full(dm.n_p2, -0.6)
    for center in CENTERS:
        for q in QUANTITIES:
            got = derived_reference(mesh, dm, u, p, T, q, center)
            assert (np.abs(got) <= derived_bound(mesh, dm, u, p, T, q, center)).all(), (center, q)
            assert np.abs(got).max() <= 1e-12


@pytest.mark.parametrize("name", ["rectangle", "box", "fixture"])
def test_rigid_rotation(name):
    """u = Omega x x: vorticity 2 Omega, gamma = 0, Q = |Omega|^2 (2D: Omega^2), divergence 0"""
    mesh = host_meshes()[name]
    dm = TaylorHoodDofMap(mesh)
    X = dm.p2_coords
    if dm.dim == 2:
        om = 1.7
        u = om * np.stack([-X[:, 1], X[:, 0]], axis=1)
        want_curl, om2 = np.array([2.0 * om]), om * om
    else:
        om = np.array([0.6, -1.1, 0.8])
        u = np.cross(np.broadcast_to(om, X.shape), X)
        want_curl, om2 = 2.0 * om, float(om @ om)
    p, T = np.zeros(dm.n_p1), None
    for center in CENTERS:
        bnd = lambda q: derived_bound(mesh, dm, u, p, T, q, center)
        ref = lambda q: derived_reference(mesh, dm, u, p, T, q, center)
        assert (np.abs(ref(nat.DERIVED_VORTICITY) - want_curl) <= bnd(nat.DERIVED_VORTICITY)).all()
        assert (np.abs(ref(nat.DERIVED_DIVERGENCE)) <= bnd(nat.DERIVED_DIVERGENCE)).all()
        assert (np.abs(ref(nat.DERIVED_Q_CRITERION) - om2) <= bnd(nat.DERIVED_Q_CRITERION)).all()
        # (a norm is 1-Lipschitz: the rounding of G + G^T bounds gamma itself, no square root of a residue)
        assert (np.abs(ref(nat.DERIVED_SHEAR_RATE)) <= bnd(nat.DERIVED_SHEAR_RATE)).all()


def test_the_names_of_the_python_module():
    import derived_fields
    assert derived_fields.QUANTITIES == {
        "vorticity": 0, "divergence": 1, "shear rate": 2, "q criterion": 3, "velocity gradient": 4,
        "pressure gradient": 5, "temperature gradient": 6}
    assert derived_fields.CENTERS == {"Cell": 0, "Vertex": 1, "Node": 2}
    with pytest.raises(ValueError):
        derived_fields.compute(None, ["lambda two"], "Node")
    with pytest.raises(ValueError):
        derived_fields.compute(None, ["vorticity"], "Edge")
    for name in ("nsfem_derived_components", "nsfem_derived_fields", "nsfem_derived_info"):
        assert name in nat.EXPORTED_SYMBOLS
