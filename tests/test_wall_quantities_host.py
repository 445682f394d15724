"""Host side of the wall quantities (nsfem_wall_set_facets / nsfem_wall_compute, csrc/wall.hip): the numpy restatement
``wall_reference`` -- the yardstick of tests/test_gpu_wall_quantities.py -- pinned against
``fem_oracle.boundary_functionals`` and against closed forms, and the host helpers of ``wall_quantities.py``.  No GPU.

The restatement takes a route that differs from the kernel's: Gauss points on the PHYSICAL facet (4-point Gauss on an
edge, 3 x 3 collapsed Gauss on a face), pulled back to the cell's reference coordinates through J^-1, the P2 / P1 basis
evaluated there; the normal comes from the facet's own geometry (rotated tangent / cross product), oriented away from
the opposite vertex.  The kernel evaluates 2 Gauss points / 3 edge midpoints given directly in barycentric coordinates
and takes the normal from grad lambda_opp.  For the P2 / P1 interpolants every integrand is a polynomial both rules
integrate exactly.  With a viscosity law nu_x(gamma, Delta_K) the integrand is no polynomial and the kernel's rule is
part of the DEFINITION: ``rule="kernel"`` places the restatement's points (still on the physical facet, still pulled
back) at the positions of that rule; it is the default when a law is given.

Row layout (include/nsfem.h): |f|, int -p n [dim], int [nu (G + sym G^T) + nu_x (G + G^T)] n [dim], int u.n, int T,
int -kappa grad T . n, int (x - x0) x t [1 / 3].

Tolerance (derived; the rule of tests/test_derived_fields_host.py): per entry ``2 n_terms 2^-53 A``.  A = the sum of the
absolute contributions of the entry: ``wall_reference(..., absolute=True)`` runs the same sums with |J^-1|, |d phi|,
|phi|, |u|, |p|, |T|, |n|, |x| + |x0| and every difference turned into a sum (for a facet opposite vertex 0 the normal is
formed from grad lambda_0 = -(grad lambda_1 + ..), itself a difference: |n| becomes sum_v |grad lambda_v| / |grad
lambda_0| there, which keeps the rounding residue of a fused multiply-add where a component of n is zero).  ``n_terms`` = rounded operations along
the longest chain of the KERNEL that ends in an entry (a fused multiply-add counts as one), the factor 2 covers the
restatement's own rounding:
    n_geo    differences, determinant, cofactors, division                   6 (2D) / 12 (3D)
    n_gl     grad lambda_0 = -sum of the others                              n_geo + dim
    n_nrm    |grad lambda_opp| (dim + 1: squares, sum, sqrt), division, sign n_gl + dim + 2
    n_w      area = gn vol / (d-1)!, w = area / NQ                           n_nrm + 3
    n_G      the point (2), d phi = 4 (lam_a gl_b + lam_b gl_a) (3),
             N2 fused terms of sum_k u_k d phi_k, + 1                        n_gl + 5 + N2 + 1
    n_t      G + sym G^T (2), nu (1), n_b (n_nrm + 1), dim terms, t_p + t_v  n_G + 4 + n_nrm + dim + 1
    n_force  w (n_w + 1), the rule's NQ terms                                n_t + n_w + 1 + NQ
    n_torque x_q = sum lam_v x_v - x0 (NV + 3), product and difference (3)   n_force + NV + 6
  = 66 (2D) / 96 (3D); every entry of a facet row gets n_torque, the longest (heat flux, mass flux, int T are shorter
  chains of the same kind).
  With a law: gamma = sqrt(1/2 sum (G_ab + G_ba)^2): n_G + dim^2 + 3 (bounded through Cauchy-Schwarz by that many eps
  times gamma^ = the same expression of the absolute sums, however small gamma is), Delta_K^2: n_geo + 7 (cbrt: 2 ulp),
  the law 3, the second traction term n_G + 2 + n_nrm + dim + 1:      + 2 n_G + n_geo + n_nrm + dim^2 + dim + 16.
  The absolute version of nu_x: Smagorinsky (C_s Delta_K)^2 gamma^; Carreau |a| (P (1 + |n - 1|/2 lambda gamma^) + 1),
  P = (1 + (lambda gamma)^2)^((n - 1)/2) -- the relative error of P from that of gamma is at most |n - 1|/2 times
  2 x / (1 + x^2) <= 1 (x = lambda gamma) times lambda delta gamma.  The device pow adds its own error: the OpenCL C
  specification (7.4, relative error of double precision built-ins), to which the device math library is built, bounds
  pow at 16 ulp = 16 * 2^-52 relative; times |a| P times the rest of the term (``absolute="pow"``).
  Group rows: a group of L facets adds ceil(L / 256) strided terms, 6 shuffle levels and 3 wave sums:
  n_torque + ceil(L / 256) + 9, A = the sum of the facets' A."""
import os

import numpy as np
import pytest

import fem_oracle as fo
import wall_quantities as wq
from fem_mesh import FacetMarkers, TaylorHoodDofMap, box_mesh, rectangle_mesh
from test_derived_fields_host import eval_quadratic, grad_quadratic, polynomial_fields, polynomial_nodal, smooth_fields

HERE = os.path.dirname(os.path.abspath(__file__))
EPS = 2.0 ** -53
POW_ULP = 16.0
EDGES = {2: ((1, 2), (0, 2), (0, 1)), 3: ((2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1))}
SMAGORINSKY, CARREAU = 1, 2


# ---------------------------------------------------------------- the restatement
def facet_rule(dim, rule):
    """(barycentric points within the facet [q, dim], weights [q], sum 1)"""
    if rule == "kernel":
        if dim == 2:
            g = 0.5 * (1.0 - 1.0 / np.sqrt(3.0))
            return np.array([[g, 1.0 - g], [1.0 - g, g]]), np.array([0.5, 0.5])
        return np.array([[0.0, 0.5, 0.5], [0.5, 0.0, 0.5], [0.5, 0.5, 0.0]]), np.full(3, 1.0 / 3.0)
    assert rule == "gauss"
    if dim == 2:
        g, w = np.polynomial.legendre.leggauss(4)
        return np.stack([0.5 * (1.0 - g), 0.5 * (1.0 + g)], axis=1), 0.5 * w
    g, w = np.polynomial.legendre.leggauss(3)
    s, ws = 0.5 * (1.0 + g), 0.5 * w
    pts, wts = [], []
    for si, wi in zip(s, ws):           # collapsed square: lam = (1 - s, s (1 - t), s t), Jacobian s, |ref face| = 1/2
        for tj, wj in zip(s, ws):
            pts.append((1.0 - si, si * (1.0 - tj), si * tj))
            wts.append(2.0 * wi * wj * si)
    return np.array(pts), np.array(wts)


def p2_basis(lam, mod):
    """(phi [.., N2], d phi / d xi [.., N2, dim]) of the P2 basis (vertices, then edges in UFC order) at barycentric
    points lam [.., dim + 1]; ``mod`` is applied to every factor"""
    dim = lam.shape[-1] - 1
    dl = np.concatenate([-np.ones((1, dim)), np.eye(dim)], axis=0)
    phi = [mod(lam[..., i] * (2.0 * lam[..., i] - 1.0)) for i in range(dim + 1)]
    dphi = [mod(4.0 * lam[..., i, None] - 1.0) * mod(dl[i]) for i in range(dim + 1)]
    for a, b in EDGES[dim]:
        phi.append(mod(4.0 * lam[..., a] * lam[..., b]))
        dphi.append(4.0 * (mod(lam[..., a, None]) * mod(dl[b]) + mod(lam[..., b, None]) * mod(dl[a])))
    return np.stack(phi, axis=-1), np.stack(dphi, axis=-2)


def law_viscosity(law, gamma, gamma_hat, delta2, absolute):
    """nu_x at the points; with ``absolute`` its absolute version (module docstring), "pow": |a| P alone"""
    if law is None:
        return np.zeros_like(gamma)
    kind, prm = law
    if kind == SMAGORINSKY:
        if absolute == "pow":
            return np.zeros_like(gamma)
        return (prm[0] * prm[0] * delta2)[:, None] * (gamma_hat if absolute else gamma)
    a, lmb, n = prm
    P = (1.0 + (lmb * gamma) ** 2) ** (0.5 * (n - 1.0))
    if absolute == "pow":
        return abs(a) * P
    if absolute:
        return abs(a) * (P * (1.0 + 0.5 * abs(n - 1.0) * abs(lmb) * gamma_hat) + 1.0)
    return a * (P - 1.0)


def wall_reference(mesh, dm, facets, u, p, T, opts, law=None, absolute=False, rule=None):
    """rows [nf, NW] of the facets ``facets = (cells, local)`` (the facet of cell c opposite its local vertex l):
    the restatement of k_wall_facets.  u [n_p2, dim], p [n_p1], T [n_p2] or None; opts = dict(nu, sym, kappa, origin);
    law = None or (SMAGORINSKY, (C_s, )) / (CARREAU, (a, lambda, n)).  ``absolute``: the sums of the absolute
    contributions instead ("pow": only the part the error of pow multiplies)"""
    dim = dm.dim
    rule = rule or ("kernel" if law is not None else "gauss")
    mod = np.abs if absolute else (lambda a: a)
    sgn = 1.0 if absolute else -1.0
    cells, local = (np.asarray(a, dtype=np.int64) for a in facets)
    nf = cells.size
    nw = wq.row_width(dim)
    if nf == 0:
        return np.zeros((0, nw))
    x = np.asarray(mesh.coords, dtype=np.float64)[np.asarray(mesh.cells, dtype=np.int64)[cells]][:, :, :dim]
    keep = np.array([[v for v in range(dim + 1) if v != o] for o in range(dim + 1)], dtype=np.int64)[local]
    xf = x[np.arange(nf)[:, None], keep]                                 # the facet's own vertices [nf, dim, dim]
    if dim == 2:
        t = xf[:, 1] - xf[:, 0]
        area = np.linalg.norm(t, axis=1)
        nrm = np.stack([t[:, 1], -t[:, 0]], axis=1) / area[:, None]
    else:
        cr = np.cross(xf[:, 1] - xf[:, 0], xf[:, 2] - xf[:, 0])
        area = 0.5 * np.linalg.norm(cr, axis=1)
        nrm = cr / np.linalg.norm(cr, axis=1)[:, None]
    inward = x[np.arange(nf), local] - xf.mean(axis=1)
    nrm = np.where((nrm * inward).sum(axis=1, keepdims=True) > 0.0, -nrm, nrm)
    pts, wts = facet_rule(dim, rule)
    xq = np.einsum("qv,fvd->fqd", pts, xf)                                # physical points
    J = np.stack([x[:, k + 1] - x[:, 0] for k in range(dim)], axis=2)
    Jinv = np.linalg.inv(J)
    xi = np.einsum("fab,fqb->fqa", Jinv, xq - x[:, None, 0, :])
    lam = np.concatenate([1.0 - xi.sum(axis=2, keepdims=True), xi], axis=2)
    phi, dphi = p2_basis(lam, mod)
    g2 = np.einsum("fba,fqkb->fqka", mod(Jinv), dphi)                     # physical gradients d_a phi_k
    p2 = np.asarray(dm.p2_dofmap, dtype=np.int64)[cells]
    ue = mod(np.asarray(u, dtype=np.float64).reshape(-1, dim)[p2])
    pe = mod(np.asarray(p, dtype=np.float64)[np.asarray(dm.p1_dofmap, dtype=np.int64)[cells]])
    uq = np.einsum("fqk,fka->fqa", phi, ue)
    G = np.einsum("fqkb,fka->fqab", g2, ue)                               # d_b u_a
    pq = np.einsum("fqv,fv->fq", mod(lam), pe)
    n = mod(nrm)
    if absolute:
        # the kernel's normal is -grad lambda_opp / |grad lambda_opp|, and grad lambda_0 = -(grad lambda_1 + ...) is a
        # difference: its absolute version is the sum of the |rows of J^-1|, which does not vanish where n_a does
        gl0 = np.abs(Jinv).sum(axis=1)
        n = np.where((local == 0)[:, None], gl0 / np.linalg.norm(Jinv.sum(axis=1), axis=1, keepdims=True), n)
    nu, sym, kappa = (mod(float(opts[k])) for k in ("nu", "sym", "kappa"))
    org = np.zeros(dim)
    if opts.get("origin") is not None:
        org = np.asarray(opts["origin"], dtype=np.float64)[:dim]
    Gt = np.swapaxes(G, 2, 3)
    tv = nu * np.einsum("fqab,fb->fqa", G + sym * Gt, n)
    if law is not None:
        # gamma of the TRUE gradient (the argument of the law), gamma^ of the absolute sums (its error scale)
        Gtrue = np.einsum("fba,fqkb,fkc->fqca", Jinv, p2_basis(lam, lambda a: a)[1],
                          np.asarray(u, dtype=np.float64).reshape(-1, dim)[p2])
        gamma = np.sqrt(0.5 * ((Gtrue + np.swapaxes(Gtrue, 2, 3)) ** 2).sum(axis=(2, 3)))
        gamma_hat = np.sqrt(0.5 * ((G + Gt) ** 2).sum(axis=(2, 3)))
        vol = np.abs(np.linalg.det(J)) / (2.0 if dim == 2 else 6.0)
        delta2 = vol ** (2.0 / dim)
        nux = law_viscosity(law, gamma, gamma_hat, delta2, absolute)
        tlaw = nux[:, :, None] * np.einsum("fqab,fb->fqa", G + Gt, n)
        tv = tlaw if absolute == "pow" else tv + tlaw
    tp = (1.0 if absolute else -1.0) * pq[:, :, None] * n[:, None, :]
    if absolute == "pow":
        tp = np.zeros_like(tp)
    tr = tp + tv
    r = mod(xq) + sgn * mod(org)[None, None, :]
    if dim == 2:
        tq = (r[..., 0] * tr[..., 1] + sgn * r[..., 1] * tr[..., 0])[..., None]
    else:
        tq = np.stack([r[..., 1] * tr[..., 2] + sgn * r[..., 2] * tr[..., 1],
                       r[..., 2] * tr[..., 0] + sgn * r[..., 0] * tr[..., 2],
                       r[..., 0] * tr[..., 1] + sgn * r[..., 1] * tr[..., 0]], axis=-1)
    w = area[:, None] * wts[None, :]
    out = np.zeros((nf, nw))
    if absolute != "pow":
        out[:, 0] = area
        out[:, 1:1 + dim] = np.einsum("fq,fqa->fa", w, tp)
        out[:, 1 + 2 * dim] = np.einsum("fq,fqa,fa->f", w, uq, n)
        if T is not None:
            Te = mod(np.asarray(T, dtype=np.float64)[p2])
            out[:, 2 + 2 * dim] = np.einsum("fq,fqk,fk->f", w, phi, Te)
            out[:, 3 + 2 * dim] = (1.0 if absolute else -1.0) * kappa * np.einsum("fq,fqkb,fk,fb->f", w, g2, Te, n)
    out[:, 1 + dim:1 + 2 * dim] = np.einsum("fq,fqa->fa", w, tv)
    out[:, 4 + 2 * dim:] = np.einsum("fq,fqa->fa", w, tq)
    return out


def n_terms(dim, law=False):
    """rounded operations along the longest chain of the kernel that ends in an entry of a facet row (docstring)"""
    n2, nq, nv = (6, 2, 3) if dim == 2 else (10, 3, 4)
    n_geo = 6 if dim == 2 else 12
    n_gl = n_geo + dim
    n_nrm = n_gl + dim + 2
    n_w = n_nrm + 3
    n_G = n_gl + 5 + n2 + 1
    n_t = n_G + 4 + n_nrm + dim + 1
    n_force = n_t + n_w + 1 + nq
    n = n_force + nv + 6
    if law:
        n += 2 * n_G + n_geo + n_nrm + dim * dim + dim + 16
    return n


def wall_bounds(mesh, dm, facets, u, p, T, opts, law=None, groups=None):
    """per-entry tolerance of the facet rows [nf, NW]; with ``groups = (facet_group, n_groups)`` the pair (facet
    bounds, group bounds [n_groups, NW])"""
    dim = dm.dim
    A = wall_reference(mesh, dm, facets, u, p, T, opts, law, absolute=True)
    n = n_terms(dim, law is not None)
    extra = 0.0
    if law is not None and law[0] == CARREAU:
        extra = POW_ULP * 2.0 * EPS * wall_reference(mesh, dm, facets, u, p, T, opts, law, absolute="pow")
    bf = 2.0 * n * EPS * A + extra
    if groups is None:
        return bf
    g, ng = np.asarray(groups[0], dtype=np.int64), int(groups[1])
    bg = np.zeros((ng, A.shape[1]))
    for k in range(ng):
        sel = g == k
        L = int(sel.sum())
        bg[k] = 2.0 * (n + (L + 255) // 256 + 9) * EPS * A[sel].sum(axis=0) + (extra[sel].sum(axis=0) if law is not None and law[0] == CARREAU else 0.0)
    return bf, bg


def group_sums(rows, facet_group, n_groups):
    out = np.zeros((n_groups, rows.shape[1]))
    np.add.at(out, np.asarray(facet_group, dtype=np.int64), rows)
    return out


# ---------------------------------------------------------------- meshes
def boundary_facets(mesh):
    """(facet ids, cells, local) of all boundary facets, in ascending facet number"""
    ids = np.flatnonzero(mesh.facet_on_boundary)
    cells, local = mesh.facet_cell_local(ids)
    return ids, cells, local


def host_meshes():
    from mesh_io import read_msh
    return {"rectangle": rectangle_mesh((0.0, 0.0), (1.5, 1.0), 6, 4),
            "box": box_mesh((0.0, 0.0, 0.0), (1.5, 1.0, 1.0), 3, 2, 2),
            "fixture": read_msh(os.path.join(HERE, "golden", "square_v41.msh"))[0]}


OPTS = dict(nu=0.37, sym=0.5, kappa=0.21, origin=(0.3, -0.2, 0.45))


# ---------------------------------------------------------------- pinned by the oracle
@pytest.mark.parametrize("name", ["rectangle", "box", "fixture"])
def test_summed_rows_equal_the_oracle_boundary_functionals(name):
    mesh = host_meshes()[name]
    dm = TaylorHoodDofMap(mesh)
    dim = dm.dim
    assert (name == "box") == (dim == 3)
    ids, cells, local = boundary_facets(mesh)
    u, p, T = smooth_fields(dm.p2_coords, dm.p1_coords)
    rows = wall_reference(mesh, dm, (cells, local), u, p, T, OPTS)
    space = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
    force, flux, meas = fo.boundary_functionals(space, mesh.facets[ids], cells, np.ascontiguousarray(u).ravel(), p,
                                                OPTS["nu"], OPTS["sym"])
    cols = wq.split_rows(rows, dim)
    total = (cols["pressure_force"] + cols["viscous_force"]).sum(axis=0)
    scale = np.abs(wall_reference(mesh, dm, (cells, local), u, p, T, OPTS, absolute=True)).sum(axis=0)
    tol = 4.0 * (n_terms(dim) + ids.size) * EPS
    assert np.all(np.abs(total - force) <= tol * (scale[1:1 + dim] + scale[1 + dim:1 + 2 * dim]))
    assert abs(cols["mass_flux"].sum() - flux) <= tol * scale[1 + 2 * dim]
    assert abs(cols["area"].sum() - meas) <= tol * scale[0]
    # the kernel's rule integrates the same polynomials exactly
    rows_k = wall_reference(mesh, dm, (cells, local), u, p, T, OPTS, rule="kernel")
    assert np.all(np.abs(rows_k - rows) <= wall_bounds(mesh, dm, (cells, local), u, p, T, OPTS))


# ---------------------------------------------------------------- closed forms
def _channel(nx=6, ny=4, L=1.5, H=1.0):
    mesh = rectangle_mesh((0.0, 0.0), (L, H), nx, ny)
    dm = TaylorHoodDofMap(mesh)
    ids, cells, local = boundary_facets(mesh)
    mid = mesh.coords[mesh.facets[ids]].mean(axis=1)
    return mesh, dm, cells, local, mid


def test_poiseuille_and_couette_shear_and_pressure_force():
    L, H, nu, dpdx, U = 1.5, 1.0, 0.3, -2.0, 0.7
    mesh, dm, cells, local, mid = _channel(L=L, H=H)
    X, X1 = dm.p2_coords, dm.p1_coords
    opts = dict(nu=nu, sym=1.0, kappa=0.0, origin=None)
    # Poiseuille: u = -dpdx / (2 nu) y (H - y), p = dpdx x: the wall shear force balances the pressure drop
    u = np.stack([-dpdx / (2.0 * nu) * X[:, 1] * (H - X[:, 1]), np.zeros(X.shape[0])], axis=1)
    p = dpdx * X1[:, 0]
    rows = wall_reference(mesh, dm, (cells, local), u, p, None, opts)
    cols = wq.split_rows(rows, 2)
    bottom, top = np.abs(mid[:, 1]) < 1e-12, np.abs(mid[:, 1] - H) < 1e-12
    inlet, outlet = np.abs(mid[:, 0]) < 1e-12, np.abs(mid[:, 0] - L) < 1e-12
    for wall in (bottom, top):
        # traction on the fluid boundary: nu du/dy n_y in x; du/dy = -/+ dpdx H / (2 nu) at bottom / top, n_y = -/+ 1
        assert np.allclose(cols["viscous_force"][wall].sum(axis=0), [dpdx * H * L / 2.0, 0.0], atol=1e-13)
        assert np.allclose(cols["pressure_force"][wall][:, 0], 0.0, atol=1e-14)
    assert np.allclose(cols["pressure_force"][inlet].sum(axis=0), [0.0, 0.0], atol=1e-13)          # p = 0 at x = 0
    assert np.allclose(cols["pressure_force"][outlet].sum(axis=0), [-dpdx * L * H, 0.0], atol=1e-13)
    q = -dpdx * H ** 3 / (12.0 * nu)
    assert np.isclose(cols["mass_flux"][outlet].sum(), q, rtol=1e-13)
    assert np.isclose(cols["mass_flux"][inlet].sum(), -q, rtol=1e-13)
    assert np.allclose(cols["mass_flux"][bottom | top], 0.0, atol=1e-15)
    # Couette: u = U y / H, p = 0: shear nu U / H on the top wall (in +x), the opposite on the bottom
    u = np.stack([U * X[:, 1] / H, np.zeros(X.shape[0])], axis=1)
    cols = wq.split_rows(wall_reference(mesh, dm, (cells, local), u, 0.0 * p, None, opts), 2)
    assert np.allclose(cols["viscous_force"][top].sum(axis=0), [nu * U / H * L, 0.0], atol=1e-14)
    assert np.allclose(cols["viscous_force"][bottom].sum(axis=0), [-nu * U / H * L, 0.0], atol=1e-14)
    tau = wq.tangential_part(cols["viscous_force"][top] / cols["area"][top][:, None], np.tile([0.0, 1.0], (top.sum(), 1)))
    assert np.allclose(tau, [nu * U / H, 0.0], atol=1e-14)


@pytest.mark.parametrize("dim", [2, 3])
def test_rigid_rotation_gives_no_viscous_traction_and_the_torque_of_a_given_traction(dim):
    """u = Omega x x: G + G^T = 0 (no viscous traction with sym = 1, twice the antisymmetric part with sym = 0);
    constant p = p0: traction -p0 n, torque about x0 = int (x - x0) x (-p0 n) -- per facet (m - x0) x (-p0 n |f|) with
    the facet midpoint m, summing to zero over a closed surface"""
    mesh = host_meshes()["rectangle" if dim == 2 else "box"]
    dm = TaylorHoodDofMap(mesh)
    ids, cells, local = boundary_facets(mesh)
    X = dm.p2_coords
    if dim == 2:
        om = 1.7
        u = om * np.stack([-X[:, 1], X[:, 0]], axis=1)
    else:
        om = np.array([0.4, -1.1, 0.8])
        u = np.cross(np.broadcast_to(om, X.shape), X)
    p0 = 2.5
    p = np.full(dm.n_p1, p0)
    x0 = np.array([0.3, -0.2, 0.45])[:dim]
    rows = wall_reference(mesh, dm, (cells, local), u, p, None, dict(nu=0.9, sym=1.0, kappa=0.0, origin=x0))
    cols = wq.split_rows(rows, dim)
    assert np.abs(cols["viscous_force"]).max() <= 1e-13
    mid, n = wq.facet_geometry(mesh, cells, local)
    f = -p0 * n * cols["area"][:, None]
    assert np.allclose(cols["pressure_force"], f, atol=1e-14)
    r = mid - x0
    want = r[:, 0] * f[:, 1] - r[:, 1] * f[:, 0] if dim == 2 else np.cross(r, f)
    assert np.allclose(cols["torque"], want, atol=1e-13)
    assert np.abs(cols["torque"].sum(axis=0)).max() <= 1e-12
    # sym = 0: the traction nu G n with G = the rotation matrix
    rows0 = wall_reference(mesh, dm, (cells, local), u, 0.0 * p, None, dict(nu=0.9, sym=0.0, kappa=0.0, origin=x0))
    W = np.array([[0.0, -om], [om, 0.0]]) if dim == 2 else np.array([[0.0, -om[2], om[1]], [om[2], 0.0, -om[0]],
                                                                     [-om[1], om[0], 0.0]])
    want = 0.9 * (n @ W.T) * cols["area"][:, None]
    assert np.allclose(wq.split_rows(rows0, dim)["viscous_force"], want, atol=1e-13)


@pytest.mark.parametrize("dim", [2, 3])
def test_linear_and_quadratic_temperature(dim):
    mesh = host_meshes()["rectangle" if dim == 2 else "box"]
    dm = TaylorHoodDofMap(mesh)
    ids, cells, local = boundary_facets(mesh)
    X = dm.p2_coords
    mid, n = wq.facet_geometry(mesh, cells, local)
    kappa = 0.21
    opts = dict(nu=0.0, sym=1.0, kappa=kappa, origin=None)
    zero_u, zero_p = np.zeros((dm.n_p2, dim)), np.zeros(dm.n_p1)
    # linear: heat_flux = -kappa grad T . n |f|
    g = np.array([0.7, -1.3, 0.4])[:dim]
    cols = wq.split_rows(wall_reference(mesh, dm, (cells, local), zero_u, zero_p, 0.5 + X @ g, opts), dim)
    assert np.allclose(cols["heat_flux"], -kappa * (n @ g) * cols["area"], atol=1e-14)
    assert np.allclose(cols["temperature_integral"], (0.5 + mid @ g) * cols["area"], atol=1e-14)
    # conduction between the walls y = 0 (T = 1) and y = H = 1 (T = 0): Nu = 1 on both
    Tc = 1.0 - X[:, 1]
    cols = wq.split_rows(wall_reference(mesh, dm, (cells, local), zero_u, zero_p, Tc, opts), dim)
    hot, cold = np.abs(mid[:, 1]) < 1e-12, np.abs(mid[:, 1] - 1.0) < 1e-12
    nu_hot = wq.nusselt_number(cols["heat_flux"][hot].sum(), cols["area"][hot].sum(), kappa, 1.0, 1.0)
    # the cold wall: heat leaves the fluid there; seen from the cold wall delta_T = -1
    nu_cold = wq.nusselt_number(cols["heat_flux"][cold].sum(), cols["area"][cold].sum(), kappa, -1.0, 1.0)
    assert abs(nu_hot - 1.0) <= 1e-13 and abs(nu_cold - 1.0) <= 1e-13
    # quadratic: int T and int grad T . n against the midpoint / Simpson closed forms of a quadratic on a facet
    _, _, cT = polynomial_fields(dim)
    cols = wq.split_rows(wall_reference(mesh, dm, (cells, local), zero_u, zero_p, eval_quadratic(cT, X), opts), dim)
    assert np.allclose(cols["heat_flux"], -kappa * (grad_quadratic(cT, mid) * n).sum(axis=1) * cols["area"], atol=1e-13)
    cv = np.asarray(mesh.cells, dtype=np.int64)[cells]
    keep = np.array([[v for v in range(dim + 1) if v != o] for o in range(dim + 1)])[local]
    xf = mesh.coords[cv[np.arange(cells.size)[:, None], keep]][:, :, :dim]
    if dim == 2:      # Simpson
        want = (eval_quadratic(cT, xf[:, 0]) + 4.0 * eval_quadratic(cT, mid) + eval_quadratic(cT, xf[:, 1])) / 6.0
    else:             # the edge-midpoint rule of the triangle
        want = sum(eval_quadratic(cT, 0.5 * (xf[:, a] + xf[:, b])) for a, b in ((0, 1), (0, 2), (1, 2))) / 3.0
    assert np.allclose(cols["temperature_integral"], want * cols["area"], atol=1e-13)


def test_hydrostatic_pressure_gives_the_buoyancy_of_the_box():
    """p = rho g (H - y): int -p n over the closed boundary = -int grad p = rho g |Omega| e_y"""
    for name in ("rectangle", "box", "fixture"):
        mesh = host_meshes()[name]
        dm = TaylorHoodDofMap(mesh)
        dim = dm.dim
        ids, cells, local = boundary_facets(mesh)
        rg = 3.0
        p = rg * (1.0 - dm.p1_coords[:, 1])
        rows = wall_reference(mesh, dm, (cells, local), np.zeros((dm.n_p2, dim)), p, None,
                              dict(nu=1.0, sym=1.0, kappa=0.0, origin=None))
        cols = wq.split_rows(rows, dim)
        x = mesh.coords[np.asarray(mesh.cells, dtype=np.int64)][:, :, :dim]
        J = np.stack([x[:, k + 1] - x[:, 0] for k in range(dim)], axis=2)
        volume = (np.abs(np.linalg.det(J)) / (2.0 if dim == 2 else 6.0)).sum()
        want = np.zeros(dim)
        want[1] = rg * volume
        assert np.allclose(cols["pressure_force"].sum(axis=0), want, atol=1e-12)
        assert np.abs(cols["viscous_force"]).max() == 0.0


@pytest.mark.parametrize("name", ["rectangle", "box"])
def test_polynomial_fields_equal_the_analytic_integrals(name):
    """quadratic u, linear p, quadratic T: every entry against integrals written out from the coefficients (Gauss
    points of high order on the physical facet applied to the EXACT fields, not to the interpolant)"""
    mesh = host_meshes()[name]
    dm = TaylorHoodDofMap(mesh)
    ids, cells, local = boundary_facets(mesh)
    poly = polynomial_fields(dm.dim)
    u, p, T = polynomial_nodal(dm, poly)
    rows = wall_reference(mesh, dm, (cells, local), u, p, T, OPTS)
    want = analytic_rows(mesh, dm, cells, local, poly, OPTS)
    assert np.all(np.abs(rows - want) <= wall_bounds(mesh, dm, (cells, local), u, p, T, OPTS))


def analytic_rows(mesh, dm, cells, local, poly, opts):
    """the rows of the exact polynomial fields ``poly`` (test_derived_fields_host.polynomial_fields): the integrands
    are evaluated from the coefficients at the points of the high-order facet rule -- no basis, no dof map"""
    dim = dm.dim
    cu, cp, cT = poly
    mid, n = wq.facet_geometry(mesh, cells, local)
    cv = np.asarray(mesh.cells, dtype=np.int64)[np.asarray(cells, dtype=np.int64)]
    keep = np.array([[v for v in range(dim + 1) if v != o] for o in range(dim + 1)])[np.asarray(local, dtype=np.int64)]
    xf = np.asarray(mesh.coords, dtype=np.float64)[cv[np.arange(cv.shape[0])[:, None], keep]][:, :, :dim]
    if dim == 2:
        area = np.linalg.norm(xf[:, 1] - xf[:, 0], axis=1)
    else:
        area = 0.5 * np.linalg.norm(np.cross(xf[:, 1] - xf[:, 0], xf[:, 2] - xf[:, 0]), axis=1)
    pts, wts = facet_rule(dim, "gauss")
    out = np.zeros((cv.shape[0], wq.row_width(dim)))
    out[:, 0] = area
    org = np.asarray(opts["origin"], dtype=np.float64)[:dim]
    for q in range(pts.shape[0]):
        X = np.einsum("v,fvd->fd", pts[q], xf)
        w = wts[q] * area
        uq = np.stack([eval_quadratic(c, X) for c in cu], axis=1)
        G = np.stack([grad_quadratic(c, X) for c in cu], axis=1)
        pq = cp[0] + X @ cp[1]
        tp = -pq[:, None] * n
        tv = opts["nu"] * np.einsum("fab,fb->fa", G + opts["sym"] * np.swapaxes(G, 1, 2), n)
        tr = tp + tv
        r = X - org
        out[:, 1:1 + dim] += w[:, None] * tp
        out[:, 1 + dim:1 + 2 * dim] += w[:, None] * tv
        out[:, 1 + 2 * dim] += w * (uq * n).sum(axis=1)
        out[:, 2 + 2 * dim] += w * eval_quadratic(cT, X)
        out[:, 3 + 2 * dim] += w * (-opts["kappa"]) * (grad_quadratic(cT, X) * n).sum(axis=1)
        if dim == 2:
            out[:, 8] += w * (r[:, 0] * tr[:, 1] - r[:, 1] * tr[:, 0])
        else:
            out[:, 10:13] += w[:, None] * np.cross(r, tr)
    return out


@pytest.mark.parametrize("dim", [2, 3])
def test_laws_on_a_uniform_shear(dim):
    """u = (s y, 0 (, 0)): gamma = |s| everywhere, nu_x constant on cells of equal size: the law's traction is
    nu_x (G + G^T) n in closed form"""
    mesh = rectangle_mesh((0.0, 0.0), (1.0, 1.0), 4, 4) if dim == 2 else box_mesh((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 2, 2, 2)
    dm = TaylorHoodDofMap(mesh)
    ids, cells, local = boundary_facets(mesh)
    s = 1.9
    u = np.zeros((dm.n_p2, dim))
    u[:, 0] = s * dm.p2_coords[:, 1]
    mid, n = wq.facet_geometry(mesh, cells, local)
    vol = (1.0 / 32.0) if dim == 2 else (1.0 / 48.0)
    delta2 = vol ** (2.0 / dim)
    S = np.zeros((dim, dim))
    S[0, 1] = S[1, 0] = s
    opts = dict(nu=0.0, sym=1.0, kappa=0.0, origin=None)
    for law, nux in (((SMAGORINSKY, (0.17, )), 0.17 ** 2 * delta2 * s),
                     ((CARREAU, (0.8, 1.3, 0.4)), 0.8 * ((1.0 + (1.3 * s) ** 2) ** (0.5 * (0.4 - 1.0)) - 1.0))):
        rows = wall_reference(mesh, dm, (cells, local), u, np.zeros(dm.n_p1), None, opts, law)
        cols = wq.split_rows(rows, dim)
        assert np.allclose(cols["viscous_force"], nux * (n @ S) * cols["area"][:, None], atol=1e-13)


# ---------------------------------------------------------------- helpers of wall_quantities.py
def test_nusselt_formula_and_tangential_projection():
    assert wq.nusselt_number(heat_flux=-0.6, area=2.0, kappa=0.1, delta_T=1.5, length=0.5) == \
        pytest.approx(0.6 * 0.5 / (0.1 * 1.5 * 2.0), rel=1e-15)
    assert wq.nusselt_number(0.6, 2.0, 0.1, 1.5, 0.5) < 0.0                  # heat leaving the fluid
    for bad in (dict(kappa=0.0), dict(area=0.0), dict(delta_T=0.0), dict(length=-1.0)):
        kw = dict(heat_flux=1.0, area=1.0, kappa=1.0, delta_T=1.0, length=1.0)
        kw.update(bad)
        with pytest.raises(ValueError):
            wq.nusselt_number(**kw)
    rng = np.random.default_rng(5)
    n = rng.normal(size=(7, 3))
    n /= np.linalg.norm(n, axis=1, keepdims=True)
    t = rng.normal(size=(7, 3))
    tau = wq.tangential_part(t, n)
    assert np.abs((tau * n).sum(axis=1)).max() <= 1e-15
    assert np.allclose(tau + (t * n).sum(axis=1, keepdims=True) * n, t, atol=1e-15)
    assert np.allclose(wq.tangential_part([[3.0, 4.0]], [[0.0, 1.0]]), [[3.0, 0.0]])


def test_grouping_and_permutation_helper():
    g = np.array([2, 0, 3, 0, 2, 2, 0], dtype=np.int32)
    perm, off = wq.sort_by_group(g, 5)
    assert perm.tolist() == [1, 3, 6, 0, 4, 5, 2] and off.tolist() == [0, 3, 3, 6, 7, 7]       # stable; 1, 4 empty
    assert perm.dtype == np.int32 and off.dtype == np.int32
    perm0, off0 = wq.sort_by_group(np.zeros(0, dtype=np.int32), 2)
    assert perm0.size == 0 and off0.tolist() == [0, 0, 0]
    for bad, ng in ((np.array([0, 2]), 2), (np.array([-1]), 1), (np.array([0]), 0)):
        with pytest.raises(ValueError):
            wq.sort_by_group(bad, ng)
    rows = np.arange(14.0).reshape(7, 2)
    sums = group_sums(rows, g, 5)
    for k in range(5):
        assert np.array_equal(sums[k], rows[perm[off[k]:off[k + 1]]].sum(axis=0))
    assert wq.row_width(2) == 9 and wq.row_width(3) == 13
    cols = wq.split_rows(np.arange(13.0), 3)
    assert cols["area"] == 0.0 and cols["pressure_force"].tolist() == [1.0, 2.0, 3.0]
    assert cols["viscous_force"].tolist() == [4.0, 5.0, 6.0] and cols["mass_flux"] == 7.0
    assert cols["temperature_integral"] == 8.0 and cols["heat_flux"] == 9.0 and cols["torque"].tolist() == [10.0, 11.0, 12.0]
    cols = wq.split_rows(np.arange(9.0), 2)
    assert cols["viscous_force"].tolist() == [3.0, 4.0] and cols["mass_flux"] == 5.0 and cols["torque"] == 8.0


def test_facet_geometry_points_out_of_the_cell():
    for name in ("rectangle", "box", "fixture"):
        mesh = host_meshes()[name]
        ids, cells, local = boundary_facets(mesh)
        mid, n = wq.facet_geometry(mesh, cells, local)
        dim = mid.shape[1]
        centre = mesh.coords[np.asarray(mesh.cells, dtype=np.int64)[cells]][:, :, :dim].mean(axis=1)
        assert np.all(((mid - centre) * n).sum(axis=1) > 0.0)
        assert np.allclose(np.linalg.norm(n, axis=1), 1.0, atol=1e-15)
        assert np.allclose(mid, mesh.coords[mesh.facets[ids]][:, :, :dim].mean(axis=1), atol=1e-15)


def test_argument_checks_of_wall_quantities():
    for kw in (dict(boundary_ids=()), dict(boundary_ids=(1, 1)), dict(boundary_ids=(1.5, )),
               dict(boundary_ids=(1, ), origin=(0.0, )), dict(boundary_ids=(1, ), origin=(0.0, np.nan)),
               dict(boundary_ids=(1, ), symmetric_gradient_factor=np.inf), dict(boundary_ids=(1, ), every=0)):
        with pytest.raises(ValueError):
            wq.WallQuantities(None, **kw)
    w = wq.WallQuantities(None, (3, 1), origin=(0.5, 0.5))
    assert w.boundary_ids == (3, 1) and w.times == [] and sorted(w.series) == [1, 3]
    assert sorted(w.series[1]) == sorted(wq.KEYS)
    with pytest.raises(AssertionError):
        w.compute()                                                           # not bound to a solver


def test_abi_is_declared_and_bound():
    import re
    import _native as nat
    with open(os.path.join(HERE, os.pardir, "include", "nsfem.h")) as fh:
        header = fh.read()
    for name in ("nsfem_wall_set_facets", "nsfem_wall_compute", "nsfem_wall_components", "nsfem_wall_info"):
        assert re.search(r"\b%s\s*\(" % name, header) and name in nat.EXPORTED_SYMBOLS
    assert [f[0] for f in nat.WallOpts._fields_] == ["nu", "sym", "kappa", "origin", "use_law"]
    assert "typedef struct {\n  double nu, sym, kappa, origin[3];\n  int use_law;\n} nsfem_wall_opts;" in header
