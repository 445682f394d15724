"""Dynamic Smagorinsky model (law 8): the numpy restatement of tests/dynamic_model_host.py pinned to
things that do not come from itself, and what can be checked of the feature without a GPU."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from dynamic_model_host import DYNAMIC, DynamicSmagorinskyRestatement, pairs
from fem_mesh import TaylorHoodDofMap, box_mesh, rectangle_mesh
from test_scalar_transport_host import smooth_fields
from test_variable_viscosity_host import rule_space


def _space(dim, n=None, scale=1.0):
    if dim == 2:
        n = n or (2, 2)
        mesh = rectangle_mesh((0.0, 0.0), (scale, scale), *n)
    else:
        n = n or (2, 2, 2)
        mesh = box_mesh((0.0, 0.0, 0.0), (scale, scale, scale), *n)
    dm = TaylorHoodDofMap(mesh)
    return mesh, dm, rule_space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)


def _field(dm, dim):
    """the smooth non-polynomial velocity of the kernel tests"""
    return smooth_fields(dm.p2_coords)[0]


# ---------------------------------------------------------------- closed form
_A = {2: ((Fraction(1, 2), Fraction(-3, 4)), (Fraction(5, 4), Fraction(1, 3))),
      3: ((Fraction(1, 2), Fraction(-3, 4), Fraction(2, 5)), (Fraction(5, 4), Fraction(1, 3), Fraction(-1, 2)),
          (Fraction(-2, 3), Fraction(3, 5), Fraction(-7, 8)))}


def _frac(x):
    return Fraction(x).limit_denominator(1 << 20)


def _patch_covariance(s, vertex):
    """exact area-weighted second moments of x over the cells at ``vertex``: (hat(x x^T) - hat x hat x^T, sum |K|), by
    int_K x_i x_j = |K| / ((d + 1)(d + 2)) (sum_v x_vi x_vj + sum_v x_vi sum_v x_vj)"""
    dim = s.dim
    cells = [c for c in range(s.geo.n_cells) if vertex in s.p1[c]]
    W, X1 = Fraction(0), [Fraction(0)] * dim
    X2 = [[Fraction(0)] * dim for _ in range(dim)]
    for c in cells:
        xv = [[_frac(t) for t in s.coords[v]] for v in s.cells[c]]
        # |K| from the exact determinant
        J = [[xv[k + 1][a] - xv[0][a] for k in range(dim)] for a in range(dim)]
        if dim == 2:
            det = J[0][0] * J[1][1] - J[0][1] * J[1][0]
        else:
            det = (J[0][0] * (J[1][1] * J[2][2] - J[1][2] * J[2][1]) - J[0][1] * (J[1][0] * J[2][2] - J[1][2] * J[2][0]) +
                   J[0][2] * (J[1][0] * J[2][1] - J[1][1] * J[2][0]))
        vol = abs(det) / math.factorial(dim)
        W += vol
        sums = [sum(x[a] for x in xv) for a in range(dim)]
        for a in range(dim):
            X1[a] += vol * sums[a] / (dim + 1)
            for b in range(dim):
                X2[a][b] += vol * (sum(x[a] * x[b] for x in xv) + sums[a] * sums[b]) / ((dim + 1) * (dim + 2))
    cov = [[X2[a][b] / W - (X1[a] / W) * (X1[b] / W) for b in range(dim)] for a in range(dim)]
    return cov, W, len(cells)


@pytest.mark.parametrize("dim", (2, 3))
def test_linear_field_has_the_closed_form_at_the_interior_vertex(dim):
    """u = A x on the uniform box(2, 2) / Kuhn (2, 2, 2) box, the interior vertex in a group of its own: gamma S is
    constant, every moment a polynomial integral of degree <= 2.  L = A cov A^T with cov the exact patch covariance of
    x (rational arithmetic), M = 2 Delta^2 (1 - alpha^2) gamma S (Delta and gamma: one sqrt / cbrt of a rational),
    num / den = Ld : M / M : M; L, M and cs2 to 1e-14 relative to their largest entry"""
    mesh, dm, s = _space(dim)
    X1 = dm.p1_coords
    centre = int(np.flatnonzero(np.all(np.abs(X1 - 0.5) < 1e-12, axis=1))[0])
    A = _A[dim]
    u = (dm.p2_coords @ np.array([[float(t) for t in row] for row in A]).T).ravel()
    ids = np.zeros(s.n1, dtype=np.int64)
    ids[centre] = 1
    alpha, cs2_max = 2.0, 1.0e6
    orc = DynamicSmagorinskyRestatement(s, (alpha, cs2_max), (2, ids))
    vert, d = orc.vertices(u, details=True)
    cov, W, n_patch = _patch_covariance(s, centre)
    assert n_patch == (6 if dim == 2 else 24) and abs(vert[centre, 0] - float(W)) < 1e-15
    ab, mult = pairs(dim)
    L = [[sum(A[a][i] * cov[i][j] * A[b][j] for i in range(dim) for j in range(dim)) for b in range(dim)] for a in range(dim)]
    S = [[(A[a][b] + A[b][a]) / 2 for b in range(dim)] for a in range(dim)]
    gamma = math.sqrt(float(2 * sum(S[a][b] * S[a][b] for a in range(dim) for b in range(dim))))
    vol = Fraction(1, 8) if dim == 2 else Fraction(1, 48)
    delta2 = float(vol) if dim == 2 else float(vol) ** (2.0 / 3.0)
    tr = sum(L[a][a] for a in range(dim)) / dim
    want_L = np.array([float(L[a][b]) for a, b in ab])
    want_M = np.array([2.0 * delta2 * (1.0 - alpha * alpha) * gamma * float(S[a][b]) for a, b in ab])
    want_Ld = np.array([float(L[a][b] - (tr if a == b else 0)) for a, b in ab])
    eL = np.abs(d["L"][centre] - want_L).max() / np.abs(want_L).max()
    eM = np.abs(d["M"][centre] - want_M).max() / np.abs(want_M).max()
    ratio = float((mult * want_Ld * want_M).sum() / (mult * want_M * want_M).sum())
    sums = orc.sums(u)
    got = sums[1, 0] / sums[1, 1]
    print("closed form dim %d: L %.2e M %.2e, num / den %.15g against %.15g" % (dim, eL, eM, got, ratio))
    assert np.abs(want_L).max() > 1e-3 and np.abs(want_M).max() > 1e-3 and abs(ratio) > 1e-3
    assert eL < 1e-14 and eM < 1e-14
    assert abs(got - ratio) < 1e-14 * abs(ratio)
    assert orc.constant(u)[1] == min(max(got, 0.0), cs2_max)


# ---------------------------------------------------------------- invariances
@pytest.mark.parametrize("dim", (2, 3))
def test_scaling_the_velocity_by_two_keeps_the_bits(dim):
    """u -> 2 u: L and M both scale by 4 exactly (powers of two commute with every rounding), cs2_g keeps its bits;
    unclipped values, several plane groups"""
    mesh, dm, s = _space(dim, (4, 4) if dim == 2 else (3, 2, 2))
    u = _field(dm, dim)
    groups = _planes(dm, 1)
    orc = DynamicSmagorinskyRestatement(s, (2.0, 1.0e6), groups)
    a, b = orc.sums(u), orc.sums(2.0 * u)
    assert np.array_equal(16.0 * a, b)
    assert np.array_equal(orc.constant(u), orc.constant(2.0 * u)) and np.abs(a).min() > 0.0
    assert np.array_equal(orc.sums(u)[:, 0] / orc.sums(u)[:, 1], b[:, 0] / b[:, 1])


def _planes(dm, axis):
    from viscosity_models import DynamicSmagorinskyModel
    return DynamicSmagorinskyModel(("planes", axis)).vertex_groups(dm.p1_coords)


@pytest.mark.parametrize("dim", (2, 3))
def test_galilean_shift_moves_the_constant_by_rounding_only(dim):
    """u -> u + U with |U| = max |u|: only the covariance L sees u itself; num / den of every group moves by at most
    1e-10 relative"""
    mesh, dm, s = _space(dim, (4, 4) if dim == 2 else (3, 2, 2))
    u = _field(dm, dim)
    U = np.array([0.6, -0.8, 0.0][:dim]) * np.abs(u).max()
    shifted = (u.reshape(-1, dim) + U[None, :]).ravel()
    orc = DynamicSmagorinskyRestatement(s, (2.0, 1.0e6), _planes(dm, 0))
    a, b = orc.sums(u), orc.sums(shifted)
    qa, qb = a[:, 0] / a[:, 1], b[:, 0] / b[:, 1]
    err = np.abs(qa - qb).max() / np.abs(qa).max()
    print("galilean dim %d: %.2e" % (dim, err))
    assert err <= 1e-10


@pytest.mark.parametrize("dim", (2, 3))
def test_scaling_the_mesh_by_two_keeps_the_constant(dim):
    """x -> 2 x with the same nodal values: G halves, Delta^2 gamma S doubles in 2D, L stays -- everything by powers of
    two in 2D (bitwise); in 3D Delta_K = cbrt(|K|) is rounded, so to 1e-13"""
    n = (4, 4) if dim == 2 else (3, 2, 2)
    mesh, dm, s = _space(dim, n)
    mesh2, dm2, s2 = _space(dim, n, scale=2.0)
    assert np.array_equal(dm.p2_dofmap, dm2.p2_dofmap)
    u = _field(dm, dim)
    a = DynamicSmagorinskyRestatement(s, (2.0, 1.0e6)).sums(u)
    b = DynamicSmagorinskyRestatement(s2, (2.0, 1.0e6)).sums(u)
    qa, qb = a[0, 0] / a[0, 1], b[0, 0] / b[0, 1]
    print("mesh scaling dim %d: %.17g %.17g" % (dim, qa, qb))
    if dim == 2:
        assert qa == qb
    else:
        assert abs(qa - qb) <= 1e-13 * abs(qa)


@pytest.mark.parametrize("dim", (2, 3))
def test_rest_and_constant_fields_give_exact_zeros(dim):
    mesh, dm, s = _space(dim, (4, 4) if dim == 2 else (3, 2, 2))
    orc = DynamicSmagorinskyRestatement(s, (2.0, 0.09), _planes(dm, 1))
    for u in (np.zeros(dim * dm.n_p2), np.tile([0.3, -1.7, 0.9][:dim], dm.n_p2)):
        vert, sums, c = orc.vertices(u), orc.sums(u), orc.constant(u)
        assert np.all(vert[:, 1:] == 0.0) and np.all(sums == 0.0) and np.all(c == 0.0)
        assert np.all(np.isfinite(vert)) and np.all(orc.residual(u) == 0.0) and np.all(orc.cell_means(u) == 0.0)


@pytest.mark.parametrize("dim", (2, 3))
def test_energy_sign(dim):
    """u . V(u) = int nu_x gamma^2 >= 0, the two sides equal to 1e-13"""
    mesh, dm, s = _space(dim, (4, 4) if dim == 2 else (3, 2, 2))
    u = _field(dm, dim)
    orc = DynamicSmagorinskyRestatement(s, (2.0, 0.09))
    orc.vertex_constants = np.linspace(0.01, 0.09, s.n1)       # (a constant that varies over the mesh)
    lhs, rhs = float(u @ orc.residual(u)), orc.dissipation(u)
    print("energy dim %d: %.12e %.12e" % (dim, lhs, rhs))
    assert rhs > 1e-6 and lhs >= 0.0 and abs(lhs - rhs) <= 1e-13 * rhs


# ---------------------------------------------------------------- grouping, model class, layers
def test_plane_groups_of_a_box():
    mesh, dm, s = _space(2, (4, 6))
    from viscosity_models import DynamicSmagorinskyModel
    n, ids = DynamicSmagorinskyModel(("planes", 1)).vertex_groups(dm.p1_coords)
    assert n == 7 and ids.dtype == np.int32 and np.array_equal(np.bincount(ids), np.full(7, 5))
    assert np.allclose(dm.p1_coords[:, 1], ids / 6.0)
    n, ids = DynamicSmagorinskyModel(("planes", 0)).vertex_groups(dm.p1_coords)
    assert n == 5 and np.array_equal(np.bincount(ids), np.full(5, 7))
    n, ids = DynamicSmagorinskyModel().vertex_groups(dm.p1_coords)
    assert n == 1 and not ids.any() and ids.size == dm.n_p1


def test_model_class_validates_and_every_layer_carries_the_feature():
    import _native as nat
    import viscosity_models as vm
    from ns_imex_solver import IMEXIPCSSolver
    from ns_problem import ProblemBase
    assert vm.LAW_DYNAMIC == DYNAMIC == 8
    m = vm.DynamicSmagorinskyModel()
    assert m.law_id == 8 and m.prandtl_t is None and tuple(m.params(None)) == (2.0, 0.09, 0.0, 0.0)
    m = vm.DynamicSmagorinskyModel(("planes", 2), filter_ratio=1.5, cs2_max=0.04)
    assert m.averaging == ("planes", 2) and tuple(m.params(dict(viscous_term=0.01))) == (1.5, 0.04, 0.0, 0.0)
    for bad in (1.0, 0.5, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="filter_ratio"):
            vm.DynamicSmagorinskyModel(filter_ratio=bad)
    for bad in (0.0, -0.1, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="cs2_max"):
            vm.DynamicSmagorinskyModel(cs2_max=bad)
    for bad in ("planes", ("planes", 3), ("planes", -1), ("lines", 0), ("planes", 0.5), None):
        with pytest.raises(ValueError, match="averaging"):
            vm.DynamicSmagorinskyModel(bad)
    with pytest.raises(ValueError, match="axis 2"):
        vm.DynamicSmagorinskyModel(("planes", 2)).vertex_groups(np.zeros((4, 2)))
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "nsfem.h")) as fh:
        header = fh.read()
    for name in ("nsfem_set_dynamic_groups", "nsfem_dynamic_constant", "nsfem_dynamic_info"):
        assert re.search(r"\bint\s+%s\s*\(\s*nsfem_ctx\s*\*" % name, header), name
        assert name in nat.EXPORTED_SYMBOLS
    for method in ("set_dynamic_groups", "dynamic_constant", "dynamic_info"):
        assert callable(getattr(nat.NsfemContext, method))
    assert callable(ProblemBase._compute_model_constant) and callable(IMEXIPCSSolver.set_viscosity_model)
