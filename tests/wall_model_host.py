"""Wall-stress models in the IMEX step: the numpy restatement -- the oracle of tests/test_gpu_wall_model.py and of
tests/test_wall_model_host.py.  Nothing here imports wall_models.py: the sample construction is restated in plain
loops over the facets, so that the arrays of ``wall_models.WallModel`` can be compared against it.

The term (include/nsfem.h).  A modelled facet f of cell K, unit normal n out of K, rule (x_q, w_q) --
3-point Gauss-Legendre on an edge, the symmetric 6-point degree-4 rule on a face --, per quadrature point a sample point
x_s(q) inside the flow and a wall distance y(q):

    U = u(x_s) - u_w,   u_par = U - (U.n) n,   Re_y = y |u_par| / nu,   r = y+^2 / Re_y  (r(0) = 1)
    W(u)_(i,a) = sum_f sum_q  w_q (nu r / y) u_par,a  phi_i(x_q)

Law 1 (Werner-Wengle): y+ = sqrt(Re_y) up to Re_y = A^(2 / (1 - B)), (Re_y / A)^(1 / (1 + B)) above.  Law 2 (Reichardt):
y+ u+(y+) = Re_y solved by NEWTON_ITS Newton steps from the law-1 value (A = 8.3, B = 1/7), every step floored at a
quarter of the iterate; the count is the same for every point.

Diagnostics row of a facet, DIM + 4 numbers: |f|, int tau_w [DIM] (tau_w = (nu r / y) u_par), int u_tau
(u_tau = nu y+ / y), int y+, max y+ over the facet's quadrature points."""
import math

import numpy as np

from test_immersed_bodies_host import IMEXPenalRestatement

WERNER_WENGLE, REICHARDT = 1, 2
WW_A, WW_B = 8.3, 1.0 / 7.0
RD_KAPPA, RD_C = 0.41, 7.8
# The Newton count of law 2, measured (tests/test_wall_model_host.py::test_reichardt_residual_table_and_newton_count):
# the smallest count at which |g| / Re_y <= 1e-15 over 4001 log-spaced Re_y in [1e-6, 1e8] -- 4 -- plus one
NEWTON_ITS = 5
INSIDE_TOL = -1.0e-12


# ---------------------------------------------------------------------------------------------------------- the laws
def ww_switch(A=WW_A, B=WW_B):
    return A ** (2.0 / (1.0 - B))


def ww_yplus(re, A=WW_A, B=WW_B):
    re = np.asarray(re, dtype=np.float64)
    return np.where(re <= ww_switch(A, B), np.sqrt(re), (re / A) ** (1.0 / (1.0 + B)))


def reichardt_uplus(yp, kappa=RD_KAPPA, C=RD_C):
    return np.log1p(kappa * yp) / kappa + C * (-np.expm1(-yp / 11.0) - (yp / 11.0) * np.exp(-yp / 3.0))


def reichardt_uplus_naive(yp, kappa=RD_KAPPA, C=RD_C):
    """the same law without log1p / expm1 (what the cancellation costs: test_wall_model_host.py)"""
    return np.log(1.0 + kappa * yp) / kappa + C * (1.0 - np.exp(-yp / 11.0) - (yp / 11.0) * np.exp(-yp / 3.0))


def reichardt_duplus(yp, kappa=RD_KAPPA, C=RD_C):
    e3 = np.exp(-yp / 3.0)
    return 1.0 / (1.0 + kappa * yp) + C * (np.exp(-yp / 11.0) / 11.0 - e3 / 11.0 + (yp / 33.0) * e3)


def reichardt_yplus(re, kappa=RD_KAPPA, C=RD_C, its=NEWTON_ITS, history=None):
    """``its`` Newton steps on g(y+) = y+ u+(y+) - Re_y from the law-1 value; Re_y = 0 gives y+ = 0.  ``history``: a
    list that receives |g| / Re_y after every step"""
    re = np.asarray(re, dtype=np.float64)
    pos = re > 0.0
    rs = np.where(pos, re, 1.0)
    yp = ww_yplus(rs)
    for _ in range(its):
        up = reichardt_uplus(yp, kappa, C)
        g = yp * up - rs
        dg = up + yp * reichardt_duplus(yp, kappa, C)
        yp = np.maximum(yp - g / dg, 0.25 * yp)
        if history is not None:
            history.append(np.abs(yp * reichardt_uplus(yp, kappa, C) - rs) / rs)
    return np.where(pos, yp, 0.0)


def law_yplus(law, params, re):
    if law == WERNER_WENGLE:
        return ww_yplus(re, params[0], params[1])
    assert law == REICHARDT
    return reichardt_yplus(re, params[0], params[1])


def ratio(re, yp):
    """r = y+^2 / Re_y, 1 at Re_y = 0"""
    re = np.asarray(re, dtype=np.float64)
    pos = re > 0.0
    return np.where(pos, yp * yp / np.where(pos, re, 1.0), 1.0)


# --------------------------------------------------------------------------------------------------------- the rules
def edge_rule():
    """3-point Gauss-Legendre on [0, 1]: barycentric points [3, 2] and weights (sum 1)"""
    g = 0.5 * math.sqrt(0.6)
    pts = np.array([[0.5 + g, 0.5 - g], [0.5, 0.5], [0.5 - g, 0.5 + g]])
    return pts, np.array([5.0, 8.0, 5.0]) / 18.0


def face_rule():
    """the symmetric 6-point rule of degree 4 on a triangle (closed form): barycentric points [6, 3], weights (sum 1)"""
    s10 = math.sqrt(10.0)
    t = math.sqrt(38.0 - 44.0 * math.sqrt(0.4))
    w = math.sqrt(213125.0 - 53320.0 * s10)
    pts, wts = [], []
    for sign in (1.0, -1.0):
        a = (8.0 - s10 + sign * t) / 18.0
        wa = (620.0 + sign * w) / 3720.0
        for k in range(3):
            p = [a, a, a]
            p[k] = 1.0 - 2.0 * a
            pts.append(p)
            wts.append(wa)
    return np.array(pts), np.array(wts)


def facet_rule(dim):
    return edge_rule() if dim == 2 else face_rule()


_EDGES = {2: ((1, 2), (0, 2), (0, 1)), 3: ((2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1))}


def p2_values(lam):
    """P2 basis values at barycentric points lam [.., dim + 1] -> [.., 6 | 10]: vertices, then the UFC edge nodes"""
    lam = np.asarray(lam, dtype=np.float64)
    dim = lam.shape[-1] - 1
    out = [lam[..., v] * (2.0 * lam[..., v] - 1.0) for v in range(dim + 1)]
    out += [4.0 * lam[..., a] * lam[..., b] for a, b in _EDGES[dim]]
    return np.stack(out, axis=-1)


def facet_local_nodes(dim, opp):
    """the local P2 nodes of the facet opposite vertex ``opp``: its vertices ascending, then its edge nodes ascending"""
    nv = dim + 1
    verts = [v for v in range(nv) if v != opp]
    edges = [nv + e for e, (a, b) in enumerate(_EDGES[dim]) if a != opp and b != opp]
    return verts + edges


def rule_in_cell(dim, opp):
    """the facet rule's points in the barycentric coordinates of the cell (lam[opp] = 0) and the weights"""
    fl, w = facet_rule(dim)
    keep = [v for v in range(dim + 1) if v != opp]
    lam = np.zeros((fl.shape[0], dim + 1))
    lam[:, keep] = fl
    return lam, w


# ------------------------------------------------------------------------------------------------ geometry, samples
def facet_geometry(X, opp):
    """cell vertex coordinates X [dim + 1, dim] -> (outward unit normal, |f|, |K|) of the facet opposite ``opp``"""
    dim = X.shape[1]
    keep = [v for v in range(dim + 1) if v != opp]
    F = X[keep]
    if dim == 2:
        t = F[1] - F[0]
        n = np.array([t[1], -t[0]])
        area = float(np.linalg.norm(t))
    else:
        n = np.cross(F[1] - F[0], F[2] - F[0])
        area = 0.5 * float(np.linalg.norm(n))
    n = n / np.linalg.norm(n)
    if np.dot(X[opp] - F[0], n) > 0.0:
        n = -n
    vol = abs(float(np.linalg.det(X[1:] - X[0]))) / math.factorial(dim)
    return n, area, vol


def modelled_facets(mesh, marks, boundary_ids):
    """(cells, locals, ids) of the boundary facets with one of the ids, id by id, ascending facet number inside one"""
    cells, local, ids = [], [], []
    for bid in boundary_ids:
        for f in np.nonzero(marks.values == bid)[0]:
            if not mesh.facet_on_boundary[f]:
                continue
            c = int(mesh.facet_cell[f])
            opp = [k for k in range(mesh._dim + 1) if int(mesh.cell_facets[c, k]) == int(f)]
            assert len(opp) == 1
            cells.append(c)
            local.append(opp[0])
            ids.append(int(bid))
    return np.array(cells, dtype=np.int32), np.array(local, dtype=np.int32), np.array(ids, dtype=np.int64)


def build_samples(mesh, cells, local, matching):
    """sample_cell [nf, NQ], sample_lambda [nf, NQ, dim + 1], sample_y [nf, NQ] by loops over facets and points.
    ("cell", theta): lambda_s = (1 - theta) lambda_q + theta e_opp in the facet's cell, y = theta dim |K| / |f|.
    ("distance", h): x_s = x_q - h n in the first cell (ascending) that contains it, y = h; ValueError outside"""
    dim = mesh._dim
    kind, par = matching
    coords, mc = mesh.coords, mesh.cells.astype(np.int64)
    nq = 3 if dim == 2 else 6
    nf = len(cells)
    sc = np.zeros((nf, nq), dtype=np.int32)
    sl = np.zeros((nf, nq, dim + 1))
    sy = np.zeros((nf, nq))
    XA = coords[mc]                                                   # [nc, dim + 1, dim]
    for f in range(nf):
        c, opp = int(cells[f]), int(local[f])
        X = coords[mc[c]]
        n, area, vol = facet_geometry(X, opp)
        lam, _ = rule_in_cell(dim, opp)
        for q in range(nq):
            if kind == "cell":
                e = np.zeros(dim + 1)
                e[opp] = 1.0
                sc[f, q] = c
                sl[f, q] = (1.0 - par) * lam[q] + par * e
                sy[f, q] = par * dim * vol / area
            else:
                assert kind == "distance"
                xs = lam[q] @ X - par * n
                # every cell asked (one solve each, all cells at once); the first that contains the point counts
                J = np.transpose(XA[:, 1:] - XA[:, :1], (0, 2, 1))
                ref = np.linalg.solve(J, (xs - XA[:, 0])[:, :, None])[:, :, 0]
                ball = np.concatenate([1.0 - ref.sum(axis=1, keepdims=True), ref], axis=1)
                inside = np.nonzero((ball >= INSIDE_TOL).all(axis=1))[0]
                if inside.size == 0:
                    raise ValueError("sample point of facet %d (cell %d) leaves the mesh" % (f, c))
                sc[f, q] = inside[0]
                sl[f, q] = ball[inside[0]]
                sy[f, q] = par
    return sc, sl, sy


# ----------------------------------------------------------------------------------------------------- the term
class WallModelRestatement:
    """``cells``, ``local``: the modelled facets; ``matching`` as above; ``wall_velocity`` [nf, dim] or None"""

    def __init__(self, mesh, dm, cells, local, law, params, nu, matching=("cell", 1.0), wall_velocity=None):
        self.dim = dim = mesh._dim
        self.law, self.params, self.nu = int(law), tuple(float(p) for p in params), float(nu)
        self.cells, self.local = np.asarray(cells, dtype=np.int64), np.asarray(local, dtype=np.int64)
        nf = self.nf = len(self.cells)
        self.p2 = np.asarray(dm.p2_dofmap).astype(np.int64)
        self.n_dofs = dim * dm.n_p2
        self.sc, self.sl, self.sy = build_samples(mesh, cells, local, matching)
        nq = self.sy.shape[1]
        self.normal, self.area = np.zeros((nf, dim)), np.zeros(nf)
        self.wq = np.zeros((nf, nq))
        self.phi = np.zeros((nf, nq, 3 if dim == 2 else 6))       # facet basis functions at the rule's points
        self.nodes = np.zeros((nf, self.phi.shape[2]), dtype=np.int64)
        mc = mesh.cells.astype(np.int64)
        for f in range(nf):
            c, opp = int(self.cells[f]), int(self.local[f])
            self.normal[f], self.area[f], _ = facet_geometry(mesh.coords[mc[c]], opp)
            lam, w = rule_in_cell(dim, opp)
            loc = facet_local_nodes(dim, opp)
            self.wq[f] = w * self.area[f]
            self.phi[f] = p2_values(lam)[:, loc]
            self.nodes[f] = self.p2[c, loc]
        self.uw = np.zeros((nf, dim)) if wall_velocity is None else np.asarray(wall_velocity, dtype=np.float64)
        assert self.uw.shape == (nf, dim)
        self.phis = p2_values(self.sl)                             # [nf, nq, 6 | 10]

    def _points(self, u):
        """u_par [nf, nq, dim], Re_y, y+, r [nf, nq]"""
        un = np.asarray(u).reshape(-1, self.dim)[self.p2[self.sc]]               # [nf, nq, N2, dim]
        U = np.einsum("fqk,fqka->fqa", self.phis, un) - self.uw[:, None, :]
        upar = U - np.einsum("fqa,fa->fq", U, self.normal)[:, :, None] * self.normal[:, None, :]
        re = self.sy * np.sqrt((upar * upar).sum(axis=2)) / self.nu
        yp = law_yplus(self.law, self.params, re)
        return upar, re, yp, ratio(re, yp)

    def re_y(self, u):
        return self._points(u)[1]

    def facet_vectors(self, u):
        """[nf, NF2, dim]: the facet's contributions to its nodes"""
        upar, _, _, r = self._points(u)
        coef = self.wq * (self.nu * r / self.sy)
        return np.einsum("fq,fqa,fqi->fia", coef, upar, self.phi)

    def residual(self, u):
        fv = self.facet_vectors(u)
        W = np.zeros(self.n_dofs)
        dofs = self.dim * self.nodes[:, :, None] + np.arange(self.dim)[None, None, :]
        np.add.at(W, dofs.ravel(), fv.ravel())
        return W

    def facet_rows(self, u):
        upar, _, yp, r = self._points(u)
        tau = (self.nu * r / self.sy)[:, :, None] * upar
        rows = np.zeros((self.nf, self.dim + 4))
        rows[:, 0] = self.area
        rows[:, 1:1 + self.dim] = np.einsum("fq,fqa->fa", self.wq, tau)
        rows[:, 1 + self.dim] = (self.wq * (self.nu * yp / self.sy)).sum(axis=1)
        rows[:, 2 + self.dim] = (self.wq * yp).sum(axis=1)
        rows[:, 3 + self.dim] = yp.max(axis=1)
        return rows


class IMEXWallRestatement(IMEXPenalRestatement):
    """IMEXRestatement whose stored explicit vector is N(u) = c_c conv(u) + V(u) + B(u) + W(u): ``wall`` is a
    WallModelRestatement (None: no model); W is added third, the device's order"""

    def __init__(self, space, coeffs, form="standard", traction_form=False, visc=None, penal=None, wall=None):
        super().__init__(space, coeffs, form, traction_form, visc=visc, penal=penal)
        self.wall = wall

    def explicit(self, u):
        N = super().explicit(u)
        return N + self.wall.residual(u) if self.wall is not None else N
