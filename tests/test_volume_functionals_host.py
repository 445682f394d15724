"""Host side of the volume functionals (nsfem_volume_functionals, csrc/functionals.hip): a per-cell numpy restatement
of the 11 quantities -- the yardstick of tests/test_gpu_volume_functionals.py -- pinned against the oracle's matrices,
a pointwise identity and closed forms; the cell flags of every partition class; the host path of ``errornorm``."""
import os

import numpy as np
import pytest

import _native as nat
import fem_oracle as fo
from fem_mesh import TaylorHoodDofMap, box_mesh, rectangle_mesh

HERE = os.path.dirname(os.path.abspath(__file__))
N_FUNCTIONALS = nat.N_FUNCTIONALS          # NSFEM_N_FUNCTIONALS of include/nsfem.h
NAMES = ("measure", "u.u", "grad u:grad u", "|curl u|^2", "(div u)^2", "u_x", "u_y", "u_z", "p", "p^2", "|grad p|^2")


# ---------------------------------------------------------------- the restatement
def pointwise(coords, cells, p2map, p1map, u, p):
    """values at the points of a collapsed Gauss rule (exact for degree 7) of every cell: dict of w [c, q] (weights
    times |det J|), u [c, q, d], G [c, q, a, b] = d_b u_a, p [c, q], gp [c, q, d]"""
    coords = np.asarray(coords, dtype=np.float64)
    dim = coords.shape[1]
    pts, wts = fo.collapsed_gauss_rule(5, dim)
    phi2, dphi2 = fo.p2_basis(pts)
    phi1, dphi1 = fo.p1_basis(pts)
    x = coords[np.asarray(cells, dtype=np.int64)]
    J = np.stack([x[:, k + 1] - x[:, 0] for k in range(dim)], axis=2)
    JinvT = np.transpose(np.linalg.inv(J), (0, 2, 1))
    g2 = np.einsum("cab,qnb->cqna", JinvT, dphi2)
    g1 = np.einsum("cab,qnb->cqna", JinvT, dphi1)
    ue = np.asarray(u, dtype=np.float64).reshape(-1, dim)[np.asarray(p2map, dtype=np.int64)]   # [c, n2, d]
    pe = np.asarray(p, dtype=np.float64)[np.asarray(p1map, dtype=np.int64)]                    # [c, n1]
    return dict(w=np.abs(np.linalg.det(J))[:, None] * wts[None, :],
                u=np.einsum("qk,cka->cqa", phi2, ue), G=np.einsum("cqkb,cka->cqab", g2, ue),
                p=np.einsum("qk,ck->cq", phi1, pe), gp=np.einsum("cqka,ck->cqa", g1, pe))


def cell_contributions(coords, cells, p2map, p1map, u, p):
    """[n_cells, 11]: the integral of every quantity of include/nsfem.h (NSFEM_N_FUNCTIONALS) over every cell"""
    v = pointwise(coords, cells, p2map, p1map, u, p)
    dim = v["u"].shape[2]
    w, G = v["w"], v["G"]
    out = np.zeros((w.shape[0], N_FUNCTIONALS))
    out[:, 0] = w.sum(axis=1)
    out[:, 1] = (w * (v["u"] ** 2).sum(axis=2)).sum(axis=1)
    out[:, 2] = (w * (G ** 2).sum(axis=(2, 3))).sum(axis=1)
    if dim == 2:
        curl2 = (G[:, :, 1, 0] - G[:, :, 0, 1]) ** 2
    else:
        curl2 = (G[:, :, 2, 1] - G[:, :, 1, 2]) ** 2 + (G[:, :, 0, 2] - G[:, :, 2, 0]) ** 2 + \
                (G[:, :, 1, 0] - G[:, :, 0, 1]) ** 2
    out[:, 3] = (w * curl2).sum(axis=1)
    out[:, 4] = (w * np.trace(G, axis1=2, axis2=3) ** 2).sum(axis=1)
    for a in range(dim):
        out[:, 5 + a] = (w * v["u"][:, :, a]).sum(axis=1)
    out[:, 8] = (w * v["p"]).sum(axis=1)
    out[:, 9] = (w * v["p"] ** 2).sum(axis=1)
    out[:, 10] = (w * (v["gp"] ** 2).sum(axis=2)).sum(axis=1)
    return out


def vol_functionals_numpy(coords, cells, p2map, p1map, u, p, flags=None):
    """(values [11], scale [11]): the sums over the flagged cells and the sums of the absolute per-cell
    contributions (the scale every tolerance of these tests is relative to)"""
    c = cell_contributions(coords, cells, p2map, p1map, u, p)
    if flags is not None:
        c = c[np.asarray(flags) != 0]
    return c.sum(axis=0), np.abs(c).sum(axis=0)


def oracle_values(space, u, p):
    """the quantities the oracle's matrices define (index -> value); divergence and curl have no matrix"""
    dim = space.dim
    M, K = space.vector_mass(), space.vector_stiffness(False)
    M2, M1, K1 = space.mass_p2(), space.mass_p1(), space.stiffness_p1()
    one1 = np.ones(space.n1)
    out = {0: float(one1 @ (M1 @ one1)), 1: float(u @ (M @ u)), 2: float(u @ (K @ u)), 8: float(one1 @ (M1 @ p)),
           9: float(p @ (M1 @ p)), 10: float(p @ (K1 @ p))}
    for a in range(dim):
        out[5 + a] = float(np.ones(space.n2) @ (M2 @ u[a::dim]))
    return out


# ---------------------------------------------------------------- meshes and fields
def smooth_fields(X2, X1):
    """smooth, non-polynomial velocity [n2, d] and pressure [n1] at the given node coordinates.

    Wave numbers of 3 to 5 and no constant parts, on purpose: the oracle evaluates int grad u : grad u as the
    quadratic form u^T K u, whose rounding error is eps * sum_ij |K_ij u_i u_j| -- it grows with the VALUES of u
    (K annihilates constants only by cancellation), while the tolerance of these tests is relative to the integral
    of |grad u|^2.  A field whose gradient is a few times its value keeps the oracle's own rounding an order of
    magnitude inside 1e-12 on meshes of up to 4096 cells; a field like 1 + small wiggle would not."""
    dim = X2.shape[1]
    x, y = X2[:, 0], X2[:, 1]
    z = X2[:, 2] if dim == 3 else np.zeros_like(x)
    comps = [np.sin(5.1 * x + 0.4) * np.cos(4.3 * y - 0.2) + 0.3 * np.sin(3.7 * z),
             0.6 * np.sin(4.7 * x - 3.9 * y) * np.exp(0.3 * x) - 0.7 * np.sin(4.1 * z + 3.3 * x)]
    if dim == 3:
        comps.append(np.sin(3.8 * z + 2.6 * x * y))
    p = np.cos(4.7 * X1[:, 0] + 0.3) * np.sin(3.4 * X1[:, 1] + 0.5) * np.exp(0.4 * X1[:, 1]) + \
        (0.5 * np.sin(3.9 * X1[:, 2]) if dim == 3 else 0.0)
    return np.stack(comps, axis=1), p


def host_meshes():
    from mesh_io import read_msh
    out = {"rectangle": rectangle_mesh((0.0, 0.0), (1.5, 1.0), 6, 4),
           "fixture": read_msh(os.path.join(HERE, "golden", "square_v41.msh"))[0],
           "box": box_mesh((0.0, 0.0, 0.0), (1.0, 0.75, 1.25), 3, 2, 3)}
    return out


@pytest.mark.parametrize("name", ["rectangle", "fixture", "box"])
def test_restatement_equals_the_oracle_matrices(name):
    mesh = host_meshes()[name]
    dm = TaylorHoodDofMap(mesh)
    u, p = smooth_fields(dm.p2_coords, dm.p1_coords)
    u = u.ravel()
    space = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
    val, scale = vol_functionals_numpy(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, u, p)
    for j, ref in oracle_values(space, u, p).items():
        assert abs(val[j] - ref) <= 1e-12 * scale[j], (NAMES[j], val[j], ref)
    if dm.dim == 2:
        assert val[7] == 0.0
    assert np.all(scale[[0, 1, 2, 3, 4, 9, 10]] > 0.0)


@pytest.mark.parametrize("name", ["rectangle", "fixture", "box"])
def test_curl_identity_pointwise(name):
    """|curl u|^2 = grad u : grad u - grad u : grad u^T at every quadrature point"""
    mesh = host_meshes()[name]
    dm = TaylorHoodDofMap(mesh)
    u, p = smooth_fields(dm.p2_coords, dm.p1_coords)
    v = pointwise(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, u.ravel(), p)
    G = v["G"]
    gg, ggt = (G * G).sum(axis=(2, 3)), (G * np.transpose(G, (0, 1, 3, 2))).sum(axis=(2, 3))
    c = cell_contributions(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, u.ravel(), p)
    assert np.abs((v["w"] * (gg - ggt)).sum(axis=1) - c[:, 3]).max() <= 1e-13 * np.abs(c[:, 2]).max()


def test_closed_forms_on_the_unit_square():
    """u = (x^2, y^2 + x), p = 1 + 2 x - 3 y: P2 / P1 represent them exactly, the integrals are rational numbers"""
    mesh = rectangle_mesh((0.0, 0.0), (1.0, 1.0), 5, 3)
    dm = TaylorHoodDofMap(mesh)
    X, X1 = dm.p2_coords, dm.p1_coords
    u = np.stack([X[:, 0] ** 2, X[:, 1] ** 2 + X[:, 0]], axis=1).ravel()
    p = 1.0 + 2.0 * X1[:, 0] - 3.0 * X1[:, 1]
    val, scale = vol_functionals_numpy(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, u, p)
    exact = [1.0, 16.0 / 15.0, 11.0 / 3.0, 1.0, 14.0 / 3.0, 1.0 / 3.0, 5.0 / 6.0, 0.0, 0.5, 4.0 / 3.0, 13.0]
    for j in range(N_FUNCTIONALS):
        assert abs(val[j] - exact[j]) <= 1e-12 * max(scale[j], 1e-300), (NAMES[j], val[j], exact[j])


def test_closed_forms_on_the_unit_cube():
    """u = (x^2, y^2 + x, z^2 + x y), p = 1 + 2 x - 3 y + z against a tensor Gauss rule of the analytic integrands"""
    mesh = box_mesh((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 2, 3, 2)
    dm = TaylorHoodDofMap(mesh)
    X, X1 = dm.p2_coords, dm.p1_coords
    u = np.stack([X[:, 0] ** 2, X[:, 1] ** 2 + X[:, 0], X[:, 2] ** 2 + X[:, 0] * X[:, 1]], axis=1).ravel()
    p = 1.0 + 2.0 * X1[:, 0] - 3.0 * X1[:, 1] + X1[:, 2]
    val, scale = vol_functionals_numpy(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, u, p)
    g, w = np.polynomial.legendre.leggauss(4)
    g, w = 0.5 * (g + 1.0), 0.5 * w
    x, y, z = [a.ravel() for a in np.meshgrid(g, g, g, indexing="ij")]
    W = np.einsum("i,j,k->ijk", w, w, w).ravel()
    ux, uy, uz = x ** 2, y ** 2 + x, z ** 2 + x * y
    G = np.zeros((x.size, 3, 3))
    G[:, 0, 0] = 2 * x
    G[:, 1, 0], G[:, 1, 1] = 1.0, 2 * y
    G[:, 2, 0], G[:, 2, 1], G[:, 2, 2] = y, x, 2 * z
    curl2 = (G[:, 2, 1] - G[:, 1, 2]) ** 2 + (G[:, 0, 2] - G[:, 2, 0]) ** 2 + (G[:, 1, 0] - G[:, 0, 1]) ** 2
    pq = 1.0 + 2.0 * x - 3.0 * y + z
    exact = [1.0, W @ (ux ** 2 + uy ** 2 + uz ** 2), W @ (G ** 2).sum(axis=(1, 2)), W @ curl2,
             W @ (2 * x + 2 * y + 2 * z) ** 2, W @ ux, W @ uy, W @ uz, W @ pq, W @ pq ** 2, 14.0]
    assert abs(exact[1] - (1.0 / 5 + 13.0 / 15 + 1.0 / 5 + 1.0 / 6 + 1.0 / 9)) < 1e-14
    for j in range(N_FUNCTIONALS):
        assert abs(val[j] - exact[j]) <= 1e-12 * scale[j], (NAMES[j], val[j], exact[j])


def test_flags_select_cells():
    mesh = host_meshes()["fixture"]
    dm = TaylorHoodDofMap(mesh)
    u, p = smooth_fields(dm.p2_coords, dm.p1_coords)
    flags = (np.arange(mesh.num_cells()) * 7 % 5 < 2).astype(np.uint8)
    args = (mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, u.ravel(), p)
    a, _ = vol_functionals_numpy(*args, flags=flags)
    b, _ = vol_functionals_numpy(*args, flags=1 - flags)
    full, scale = vol_functionals_numpy(*args)
    assert np.all(np.abs(a + b - full) <= 1e-13 * scale + 1e-300)


# ---------------------------------------------------------------- cell flags of the partitions
def _check_cover(parts, global_mesh):
    count = np.zeros(global_mesh.num_cells(), dtype=np.int64)
    gx = global_mesh.coords[global_mesh.cells.astype(np.int64)]
    for part in parts:
        flags, glob = part.owned_cell_flags(), part.cell_global()
        assert flags.dtype == np.uint8 and flags.shape == (part.mesh.num_cells(), ) == glob.shape
        own = flags != 0
        np.add.at(count, glob[own], 1)
        lx = part.mesh.coords[part.mesh.cells.astype(np.int64)][own]
        # the flagged local cell IS the global cell: same vertex coordinates (as a set)
        assert np.abs(np.sort(lx.sum(axis=2), axis=1) - np.sort(gx[glob[own]].sum(axis=2), axis=1)).max() < 1e-12
        assert np.abs(lx.mean(axis=1) - gx[glob[own]].mean(axis=1)).max() < 1e-12
    assert np.array_equal(count, np.ones_like(count))


@pytest.mark.parametrize("size", [2, 3, 4])
def test_owned_cell_flags_cover_every_cell_once(size):
    from partition import (GraphPartition, PeriodicSlabPartition, PeriodicStripPartition, SlabPartition,
                           StripPartition)
    import grid_generator as gg
    lo2, hi2 = (0.0, 0.0), (1.25, 1.0)
    _check_cover([StripPartition(lo2, hi2, 5, 12, r, size, coarsest=2) for r in range(size)],
                 rectangle_mesh(lo2, hi2, 5, 12))
    _check_cover([PeriodicStripPartition((0.0, 0.0), (1.0, 1.0), 4, 12, r, size, coarsest=2) for r in range(size)],
                 rectangle_mesh((0.0, 0.0), (1.0, 1.0), 4, 12))
    lo3, hi3 = (0.0, 0.0, 0.0), (1.0, 0.75, 1.5)
    _check_cover([SlabPartition(lo3, hi3, 3, 2, 12, r, size, coarsest=2) for r in range(size)],
                 box_mesh(lo3, hi3, 3, 2, 12))
    one = (1.0, 1.0, 1.0)
    _check_cover([PeriodicSlabPartition((0.0, 0.0, 0.0), one, 4, 4, 12, r, size, coarsest=2) for r in range(size)],
                 box_mesh((0.0, 0.0, 0.0), one, 4, 4, 12))
    gm, marks = gg.dfg_channel(2, 1)
    parts = [GraphPartition(gm, r, size, marks) for r in range(size)]
    _check_cover(parts, gm)
    for part in parts:      # the rule of the class: cell_owner == rank on the finest level
        assert np.array_equal(part.owned_cell_flags() != 0, part.cell_owner[0][part.fine.cells] == part.rank)


# ---------------------------------------------------------------- errornorm, host path
def test_errornorm_host_path_equals_the_closed_form():
    """uh = 0 and uh = the interpolant of a polynomial: |u - uh| through the host dx quadrature (degree_rise > 0)"""
    import dlfn_compat as dlfn
    import fem_spaces
    mesh = rectangle_mesh((0.0, 0.0), (1.0, 1.0), 4, 4)
    dm = TaylorHoodDofMap(mesh)
    V, Q = fem_spaces.FunctionSpace(dm, "velocity"), fem_spaces.FunctionSpace(dm, "pressure")
    u = dlfn.Expression(("x[0]*x[0]", "x[1]*x[1] + x[0]"), degree=2)
    p = dlfn.Expression("1.0 + 2.0*x[0] - 3.0*x[1]", degree=1)
    zero_u, zero_p = fem_spaces.Function(V), fem_spaces.Function(Q)
    assert abs(dlfn.errornorm(u, zero_u) - np.sqrt(16.0 / 15.0)) < 1e-13
    assert abs(dlfn.errornorm(p, zero_p, "L2", degree_rise=3) - np.sqrt(4.0 / 3.0)) < 1e-13
    X = dm.p2_coords
    uh = fem_spaces.Function(V, np.stack([X[:, 0] ** 2, X[:, 1] ** 2 + X[:, 0]], axis=1).ravel())
    assert dlfn.errornorm(u, uh) < 1e-14
    # finite element function against finite element function: the H1 norms are available on the host path
    assert abs(dlfn.errornorm(zero_u, uh, "H10") - np.sqrt(11.0 / 3.0)) < 1e-13
    assert abs(dlfn.errornorm(zero_u, uh, "H1") - np.sqrt(16.0 / 15.0 + 11.0 / 3.0)) < 1e-13
    with pytest.raises(NotImplementedError):
        dlfn.errornorm(u, uh, "H1")
    with pytest.raises(ValueError):
        dlfn.errornorm(u, uh, "Linf")
    with pytest.raises(TypeError):          # degree_rise = 0 is the device path: needs a solver's function
        dlfn.errornorm(u, uh, degree_rise=0)
    with pytest.raises(TypeError):
        dlfn.norm(uh)


def test_native_layer_declares_the_entry_point():
    assert "nsfem_volume_functionals" in nat.EXPORTED_SYMBOLS and N_FUNCTIONALS == 11 == len(NAMES)
    assert callable(nat.NsfemContext.volume_functionals)
    import ns_problem
    assert callable(ns_problem.ProblemBase._compute_flow_diagnostics)
