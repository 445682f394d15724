"""Wall-stress models for the IMEX step (csrc/wallmodel.hip): wall-modelled LES.

A modelled wall keeps ``u.n = 0`` only (``VelocityBCType.no_normal_flux``); its tangential stress comes from a law of
the wall evaluated with the velocity sampled inside the flow, and joins the extrapolated explicit vector of
``IMEXIPCSSolver`` as a third term, N(u) = c_c conv(u) + V(u) + B(u) + W(u):

    U = u(x_s) - u_w,  u_par = U - (U.n) n,  Re_y = y |u_par| / nu,  r = y+^2 / Re_y
    W(u)_(i,a) = sum_f sum_q w_q (nu r / y) u_par,a phi_i(x_q)

* ``WernerWengleModel(A=8.3, B=1/7)``: y+ = sqrt(Re_y) up to Re_y = A^(2/(1-B)), (Re_y / A)^(1/(1+B)) above -- closed.
* ``ReichardtModel(kappa=0.41, C=7.8)``: u+ = log(1 + kappa y+)/kappa + C (1 - exp(-y+/11) - (y+/11) exp(-y+/3)),
  solved on the device by a fixed number of Newton steps.
* ``WallModel(law, boundary_ids, matching=("cell", 1.0), wall_velocity=None)``; ``build(mesh, markers, dofmap)`` makes
  the facet set, the sample arrays and the node CSR.  Matching ``("cell", theta)``, 0 < theta <= 1: the sample of a
  quadrature point lies in the facet's own cell, lambda_s = (1 - theta) lambda_q + theta e_opp, at the wall distance
  y = theta dim |K| / |f|.  ``("distance", h)``: x_s = x_q - h n, located once on the host (``point_locator``), y = h;
  a sample that leaves the mesh raises ValueError.  On periodic meshes use the in-cell strategy: a located cell is
  accepted only where its own coordinates contain the point, so a sample beyond a periodic side is refused.
  ``wall_velocity``: one vector for all ids or ``{boundary_id: vector}`` (default 0).

The term is explicit: k nu r / (y h) <= 1/9 (2D) or 4/45 (3D) is sufficient for SBDF2, h the height of the wall cell
(``explicit_step_bound``).  ``wall_quantities`` differentiates the resolved velocity: on a modelled
boundary its viscous row is the resolved stress, not the wall stress -- ``ProblemBase._compute_wall_model`` gives that.
"""
import math
from types import SimpleNamespace

import numpy as np

import point_locator

WERNER_WENGLE, REICHARDT = 1, 2


class WernerWengleModel:
    law_id = WERNER_WENGLE

    def __init__(self, A=8.3, B=1.0 / 7.0):
        if not (math.isfinite(A) and A > 0.0 and math.isfinite(B) and 0.0 < B < 1.0):
            raise ValueError("Werner-Wengle: A > 0 and 0 < B < 1")
        self.A, self.B = float(A), float(B)

    def params(self):
        return (self.A, self.B)

    @property
    def switch(self):
        """Re_y at which the sublayer branch hands over to the power law"""
        return self.A ** (2.0 / (1.0 - self.B))

    def y_plus(self, re_y):
        re_y = np.asarray(re_y, dtype=np.float64)
        return np.where(re_y <= self.switch, np.sqrt(re_y), (re_y / self.A) ** (1.0 / (1.0 + self.B)))


class ReichardtModel:
    law_id = REICHARDT

    def __init__(self, kappa=0.41, C=7.8):
        if not (math.isfinite(kappa) and kappa > 0.0 and math.isfinite(C) and C >= 0.0):
            raise ValueError("Reichardt: kappa > 0 and C >= 0")
        self.kappa, self.C = float(kappa), float(C)

    def params(self):
        return (self.kappa, self.C)

    def u_plus(self, y_plus):
        yp = np.asarray(y_plus, dtype=np.float64)
        damped = -np.expm1(-yp / 11.0) - (yp / 11.0) * np.exp(-yp / 3.0)
        return np.log1p(self.kappa * yp) / self.kappa + self.C * damped


def _edge_rule():
    g = 0.5 * math.sqrt(0.6)
    return np.array([[0.5 + g, 0.5 - g], [0.5, 0.5], [0.5 - g, 0.5 + g]]), np.array([5.0, 8.0, 5.0]) / 18.0


def _face_rule():
    a1, b1, w1 = 0.44594849091596483, 0.10810301816807033, 0.22338158967801144
    a2, b2, w2 = 0.09157621350977073, 0.8168475729804585, 0.10995174365532187
    pts = [[b1, a1, a1], [a1, b1, a1], [a1, a1, b1], [b2, a2, a2], [a2, b2, a2], [a2, a2, b2]]
    return np.array(pts), np.array([w1, w1, w1, w2, w2, w2])


def facet_rule(dim):
    """(points in the facet's barycentric coordinates [NQ, dim], weights summing to 1): 3-point Gauss-Legendre on an
    edge, the symmetric 6-point rule of degree 4 on a face -- the rule of k_wm_facets, in its order"""
    return _edge_rule() if dim == 2 else _face_rule()


_EDGES = {2: ((1, 2), (0, 2), (0, 1)), 3: ((2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1))}


def facet_local_nodes(dim):
    """[dim + 1, NF2]: the local P2 nodes of the facet opposite each vertex -- vertices ascending, then edge nodes"""
    nv = dim + 1
    return np.array([[v for v in range(nv) if v != o] +
                     [nv + e for e, (a, b) in enumerate(_EDGES[dim]) if a != o and b != o] for o in range(nv)])


class WallModel:
    def __init__(self, law, boundary_ids, matching=("cell", 1.0), wall_velocity=None):
        if not (hasattr(law, "law_id") and hasattr(law, "params")):
            raise ValueError("wall model: law must be a WernerWengleModel or a ReichardtModel")
        ids = [boundary_ids] if np.isscalar(boundary_ids) else list(boundary_ids)
        if not ids or any(int(i) != i for i in ids) or len(set(ids)) != len(ids):
            raise ValueError("wall model: boundary_ids must be distinct integers, at least one")
        kind, par = matching
        if kind not in ("cell", "distance"):
            raise ValueError("wall model: matching is (\"cell\", theta) or (\"distance\", h)")
        par = float(par)
        if kind == "cell" and not 0.0 < par <= 1.0:
            raise ValueError("wall model: theta must lie in (0, 1]")
        if kind == "distance" and not (math.isfinite(par) and par > 0.0):
            raise ValueError("wall model: the matching distance h must be finite and > 0")
        self.law = law
        self.boundary_ids = tuple(int(i) for i in ids)
        self.matching = (kind, par)
        self.wall_velocity = wall_velocity

    def _wall_velocity(self, facet_id, dim):
        wv = self.wall_velocity
        if wv is None:
            return None
        out = np.zeros((facet_id.size, dim))
        if isinstance(wv, dict):
            for bid, v in wv.items():
                if int(bid) not in self.boundary_ids:
                    raise ValueError("wall model: wall velocity for boundary id %s, which is not modelled" % (bid, ))
                out[facet_id == int(bid)] = np.asarray(v, dtype=np.float64).reshape(dim)
        else:
            out[:] = np.asarray(wv, dtype=np.float64).reshape(dim)
        if not np.all(np.isfinite(out)):
            raise ValueError("wall model: non-finite wall velocity")
        return out

    def build(self, mesh, markers, dofmap):
        """-> namespace(facet_cell, facet_local, facet_id [nf]; sample_cell [nf, NQ], sample_lambda [nf, NQ, dim + 1],
        sample_y [nf, NQ]; wall_velocity [nf, dim] or None; normals [nf, dim], areas [nf]; nodes, node_ptr, node_entry:
        the P2 nodes on modelled facets ascending and per node its rows (facet NF2 + local) of the facet vectors in
        ascending facet order -- the CSR of k_wm_gather).  Facets: id by id in the order given, ascending facet
        number inside an id"""
        dim = mesh._dim
        nv = dim + 1
        cells, local, fid = [], [], []
        for bid in self.boundary_ids:
            facets = markers.facets_with_id(bid)
            facets = facets[mesh.facet_on_boundary[facets]]
            if facets.size == 0:
                raise ValueError("wall model: boundary id %d marks no boundary facet" % bid)
            c, l = mesh.facet_cell_local(facets)
            cells.append(c)
            local.append(l)
            fid.append(np.full(c.size, bid, dtype=np.int64))
        fc, fl = np.concatenate(cells).astype(np.int64), np.concatenate(local).astype(np.int64)
        fid = np.concatenate(fid)
        nf = fc.size
        coords, mc = np.asarray(mesh.coords, dtype=np.float64), np.asarray(mesh.cells).astype(np.int64)
        X = coords[mc[fc]]                                                        # [nf, nv, dim]
        keep = np.array([[v for v in range(nv) if v != o] for o in range(nv)])[fl]  # [nf, dim]
        XF = X[np.arange(nf)[:, None], keep]                                      # the facet's vertices
        if dim == 2:
            t = XF[:, 1] - XF[:, 0]
            n = np.stack([t[:, 1], -t[:, 0]], axis=1)
            area = np.linalg.norm(t, axis=1)
        else:
            n = np.cross(XF[:, 1] - XF[:, 0], XF[:, 2] - XF[:, 0])
            area = 0.5 * np.linalg.norm(n, axis=1)
        n = n / np.linalg.norm(n, axis=1, keepdims=True)
        inward = X[np.arange(nf), fl] - XF[:, 0]
        n = np.where((n * inward).sum(axis=1, keepdims=True) > 0.0, -n, n)
        vol = np.abs(np.linalg.det(X[:, 1:] - X[:, :1])) / math.factorial(dim)
        pts, _ = facet_rule(dim)
        nq = pts.shape[0]
        lam_q = np.zeros((nf, nq, nv))
        lam_q[np.arange(nf)[:, None, None], np.arange(nq)[None, :, None], keep[:, None, :]] = pts[None, :, :]
        kind, par = self.matching
        if kind == "cell":
            e_opp = np.zeros((nf, nv))
            e_opp[np.arange(nf), fl] = 1.0
            sample_cell = np.repeat(fc[:, None], nq, axis=1)
            sample_lambda = (1.0 - par) * lam_q + par * e_opp[:, None, :]
            sample_y = np.repeat((par * dim * vol / area)[:, None], nq, axis=1)
        else:
            xs = (np.einsum("fqv,fvd->fqd", lam_q, X) - par * n[:, None, :]).reshape(-1, dim)
            bins = point_locator.build_bins(coords, mc)
            found = point_locator.locate_points_numpy(bins, coords, mc, xs)
            if (found < 0).any():
                f = int(np.nonzero(found < 0)[0][0]) // nq
                raise ValueError("wall model: a sample point of facet %d (cell %d, boundary id %d) at distance %g leaves "
                                 "the mesh" % (f, fc[f], fid[f], par))
            lam = point_locator.barycentric(coords, mc, found.astype(np.int64), xs)
            # (the cell's own coordinates contain the point: holds for what the locator returns, and is what a
            # periodic mesh needs -- a sample beyond a periodic side is never wrapped)
            if not (lam >= point_locator.INSIDE_TOL).all():
                raise ValueError("wall model: a located cell does not contain its sample point")
            sample_cell = found.reshape(nf, nq)
            sample_lambda = lam.reshape(nf, nq, nv)
            sample_y = np.full((nf, nq), par)
        # the node CSR of the gather
        loc = facet_local_nodes(dim)[fl]                                          # [nf, NF2]
        nf2 = loc.shape[1]
        node_of = np.asarray(dofmap.p2_dofmap).astype(np.int64)[fc[:, None], loc]
        entry = np.arange(nf * nf2, dtype=np.int64).reshape(nf, nf2)
        order = np.lexsort((entry.ravel(), node_of.ravel()))
        sorted_nodes = node_of.ravel()[order]
        nodes, counts = np.unique(sorted_nodes, return_counts=True)
        return SimpleNamespace(
            facet_cell=fc.astype(np.int32), facet_local=fl.astype(np.int32), facet_id=fid,
            sample_cell=sample_cell.astype(np.int32), sample_lambda=np.ascontiguousarray(sample_lambda),
            sample_y=np.ascontiguousarray(sample_y), wall_velocity=self._wall_velocity(fid, dim), normals=n, areas=area,
            nodes=nodes.astype(np.int32), node_ptr=np.concatenate([[0], np.cumsum(counts)]).astype(np.int32),
            node_entry=entry.ravel()[order].astype(np.int32))


#: largest eigenvalue of (P2 mass matrix of a cell / |K|)^-1 (P2 mass matrix of one of its facets / |f|): exactly 6 on a
#: triangle and 5 on a tetrahedron (tests/test_wall_model_host.py recomputes them)
FACET_MASS_RATIO = {2: 6.0, 3: 5.0}


def explicit_step_bound(dim, scheme_bound):
    """the constant c of the sufficient step bound  k nu r / (y h) <= c  of the explicit wall term: h the
    height of the wall cell over its facet, ``scheme_bound`` the largest k sigma the scheme admits for an explicit decay
    term -sigma u (``immersed_bodies.stiff_step_bound``: 4/3 SBDF2, 1 CNAB and mCNAB, 0 CNLF).  c = scheme_bound /
    (dim mu) with mu = FACET_MASS_RATIO: 1/9 (2D) and 4/45 (3D) for SBDF2"""
    return float(scheme_bound) / (dim * FACET_MASS_RATIO[dim])
