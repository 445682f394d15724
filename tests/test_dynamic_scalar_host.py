"""Dynamic subgrid heat flux (nsfem_set_scalar_sgs_dynamic): the numpy restatement of
tests/dynamic_scalar_host.py pinned to things that do not come from itself, and what can be checked of the feature
without a GPU."""
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

from dynamic_scalar_host import DynamicScalarRestatement
from test_dynamic_model_host import _A, _field, _patch_covariance, _planes, _space
from test_scalar_transport_host import smooth_fields

# (3D: the entries sum to zero, so hat T = b . hat x vanishes at the centre of the point-symmetric patch and the
# covariance P = hat(T u) - hat T hat u is formed without cancellation)
_B = {2: (Fraction(7, 10), Fraction(-11, 10)), 3: (Fraction(1, 2), Fraction(-5, 4), Fraction(3, 4))}


def _fields(dm):
    return smooth_fields(dm.p2_coords)


# ---------------------------------------------------------------- closed form
@pytest.mark.parametrize("dim", (2, 3))
def test_linear_fields_have_the_closed_form_at_the_interior_vertex(dim):
    """u = A x, T = b . x on the uniform box(2, 2) / Kuhn (2, 2, 2) box, the interior vertex in a group of its own:
    gamma grad T is constant, every moment a polynomial integral of degree <= 2.  P = A cov b with cov the exact patch
    covariance of x (rational arithmetic), R = (1 - alpha^2) Delta^2 gamma b (Delta and gamma: one sqrt / cbrt of a
    rational), num / den = P . R / R . R; P, R and the quotient to 1e-14 relative to their largest entry"""
    mesh, dm, s = _space(dim)
    X1 = dm.p1_coords
    centre = int(np.flatnonzero(np.all(np.abs(X1 - 0.5) < 1e-12, axis=1))[0])
    A, b = _A[dim], _B[dim]
    u = (dm.p2_coords @ np.array([[float(t) for t in row] for row in A]).T).ravel()
    T = dm.p2_coords @ np.array([float(t) for t in b])
    ids = np.zeros(s.n1, dtype=np.int64)
    ids[centre] = 1
    alpha, cmax = 2.0, 1.0e6
    orc = DynamicScalarRestatement(s, (alpha, cmax), (2, ids))
    vert, d = orc.vertices(u, T, details=True)
    cov, W, n_patch = _patch_covariance(s, centre)
    assert n_patch == (6 if dim == 2 else 24) and abs(vert[centre, 0] - float(W)) < 1e-15
    P = [sum(A[a][i] * cov[i][j] * b[j] for i in range(dim) for j in range(dim)) for a in range(dim)]
    S = [[(A[a][c] + A[c][a]) / 2 for c in range(dim)] for a in range(dim)]
    gamma = math.sqrt(float(2 * sum(S[a][c] * S[a][c] for a in range(dim) for c in range(dim))))
    vol = Fraction(1, 8) if dim == 2 else Fraction(1, 48)
    delta2 = float(vol) if dim == 2 else float(vol) ** (2.0 / 3.0)
    want_P = np.array([float(p) for p in P])
    want_R = np.array([(1.0 - alpha * alpha) * delta2 * gamma * float(t) for t in b])
    eP = np.abs(d["P"][centre] - want_P).max() / np.abs(want_P).max()
    eR = np.abs(d["R"][centre] - want_R).max() / np.abs(want_R).max()
    ratio = float(want_P @ want_R / (want_R @ want_R))
    sums = orc.sums(u, T)
    got = sums[1, 0] / sums[1, 1]
    print("closed form dim %d: P %.2e R %.2e, num / den %.15g against %.15g" % (dim, eP, eR, got, ratio))
    assert np.abs(want_P).max() > 1e-3 and np.abs(want_R).max() > 1e-3 and abs(ratio) > 1e-3
    assert eP < 1e-14 and eR < 1e-14
    assert abs(got - ratio) < 1e-14 * abs(ratio)
    assert orc.constant(u, T)[1] == min(max(got, 0.0), cmax)


# ---------------------------------------------------------------- exact zeros
@pytest.mark.parametrize("dim", (2, 3))
def test_rest_and_constant_fields_give_exact_zeros(dim):
    """T = const (grad T = 0 exactly), u = const and rest (gamma = 0 exactly): PR, RR, the sums, the constant, D and the
    cell means are 0.0, nothing is NaN"""
    mesh, dm, s = _space(dim, (4, 4) if dim == 2 else (3, 2, 2))
    orc = DynamicScalarRestatement(s, (2.0, 0.2), _planes(dm, 1))
    u, T = _fields(dm)
    uc = np.tile([0.3, -1.7, 0.9][:dim], dm.n_p2)
    for uu, TT in ((u, np.full(dm.n_p2, 0.7)), (uc, T), (np.zeros_like(u), T), (np.zeros_like(u), np.zeros_like(T))):
        vert, sums, c = orc.vertices(uu, TT), orc.sums(uu, TT), orc.constant(uu, TT)
        assert np.all(np.isfinite(vert)) and np.all(vert[:, 0] > 0.0)
        assert np.all(vert[:, 1:] == 0.0) and np.all(sums == 0.0) and np.all(c == 0.0)
        assert np.all(orc.residual(uu, TT) == 0.0) and np.all(orc.cell_means(uu, TT) == 0.0)


# ---------------------------------------------------------------- invariances
@pytest.mark.parametrize("dim", (2, 3))
def test_scaling_by_two_keeps_the_bits(dim):
    """T -> 2 T: P and R double; u -> 2 u: P doubles, gamma and hat gamma double, so R doubles -- powers of two commute
    with every rounding, num and den scale by 4 exactly and ctheta_g keeps its bits; unclipped, several plane groups"""
    mesh, dm, s = _space(dim, (4, 4) if dim == 2 else (3, 2, 2))
    u, T = _fields(dm)
    orc = DynamicScalarRestatement(s, (2.0, 1.0e6), _planes(dm, 1))
    a = orc.sums(u, T)
    assert np.abs(a).min() > 0.0
    for b in (orc.sums(u, 2.0 * T), orc.sums(2.0 * u, T)):
        assert np.array_equal(4.0 * a, b)
        assert np.array_equal(a[:, 0] / a[:, 1], b[:, 0] / b[:, 1])
    assert np.array_equal(orc.constant(u, T), orc.constant(u, 2.0 * T))
    assert np.array_equal(orc.constant(u, T), orc.constant(2.0 * u, T))


@pytest.mark.parametrize("dim", (2, 3))
def test_galilean_shift_moves_the_constant_by_rounding_only(dim):
    """u -> u + U with |U| = max |u|: only the covariance P sees u itself; num / den of every group moves by at most
    1e-10 relative"""
    mesh, dm, s = _space(dim, (4, 4) if dim == 2 else (3, 2, 2))
    u, T = _fields(dm)
    U = np.array([0.6, -0.8, 0.0][:dim]) * np.abs(u).max()
    shifted = (u.reshape(-1, dim) + U[None, :]).ravel()
    orc = DynamicScalarRestatement(s, (2.0, 1.0e6), _planes(dm, 0))
    a, b = orc.sums(u, T), orc.sums(shifted, T)
    qa, qb = a[:, 0] / a[:, 1], b[:, 0] / b[:, 1]
    err = np.abs(qa - qb).max() / np.abs(qa).max()
    print("galilean dim %d: %.2e" % (dim, err))
    assert err <= 1e-10


@pytest.mark.parametrize("dim", (2, 3))
def test_variance_sign(dim):
    """T . D(u, T) = int kappa_x |grad T|^2 >= 0, the two sides equal to 1e-13"""
    mesh, dm, s = _space(dim, (4, 4) if dim == 2 else (3, 2, 2))
    u, T = _fields(dm)
    orc = DynamicScalarRestatement(s, (2.0, 0.2))
    orc.vertex_constants = np.linspace(0.01, 0.2, s.n1)        # (a constant that varies over the mesh)
    lhs, rhs = float(T @ orc.residual(u, T)), orc.dissipation(u, T)
    print("variance dim %d: %.12e %.12e" % (dim, lhs, rhs))
    assert rhs > 1e-6 and lhs >= 0.0 and abs(lhs - rhs) <= 1e-13 * rhs


# ---------------------------------------------------------------- grouping
@pytest.mark.parametrize("dim", (2, 3))
def test_plane_groups_partition_the_global_sums(dim):
    """the plane groups along every axis: their sums add up to those of the global group (to rounding, against the sums
    of absolute contributions), every group holds vertices, and the clip acts group by group"""
    mesh, dm, s = _space(dim, (4, 4) if dim == 2 else (3, 2, 2))
    u, T = _fields(dm)
    glob = DynamicScalarRestatement(s, (2.0, 0.2))
    total, scale = glob.sums(u, T)[0], glob.sums(u, T, absolute=True)[0]
    for axis in range(dim):
        n, ids = _planes(dm, axis)
        orc = DynamicScalarRestatement(s, (2.0, 0.2), (n, ids))
        sums = orc.sums(u, T)
        assert sums.shape == (n, 2) and n == (5 if dim == 2 else (4, 3, 3)[axis])
        assert np.all(np.abs(sums.sum(axis=0) - total) <= 64 * 2.0 ** -53 * scale)
        c = orc.constant(u, T)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = sums[:, 0] / sums[:, 1]
        assert np.array_equal(c, np.where(sums[:, 1] > 0.0, np.minimum(np.maximum(q, 0.0), 0.2), 0.0))
        assert np.array_equal(orc.cell_constant(c[ids]), orc.cell_constant(c[orc.group]))


# ---------------------------------------------------------------- model class, layers
def test_model_class_validates_and_every_layer_carries_the_feature():
    import _native as nat
    import viscosity_models as vm
    from ns_boussinesq_solver import BoussinesqIMEXSolver
    from ns_problem import ProblemBase
    m = vm.DynamicSmagorinskyModel()
    assert m.heat_flux is None and m.prandtl_t is None and m.ctheta_max == 0.2
    assert tuple(m.params(None)) == (2.0, 0.09, 0.0, 0.0)
    m = vm.DynamicSmagorinskyModel(("planes", 1), heat_flux="dynamic", ctheta_max=0.05)
    assert m.heat_flux == "dynamic" and m.ctheta_max == 0.05 and m.prandtl_t is None
    assert tuple(m.params(None)) == (2.0, 0.09, 0.0, 0.0)              # (the law's parameters do not carry the clip)
    for bad in ("fixed", "Dynamic", 1, True, 0.85):
        with pytest.raises(ValueError, match="heat_flux"):
            vm.DynamicSmagorinskyModel(heat_flux=bad)
    for bad in (0.0, -0.1, float("nan"), float("inf"), True):
        with pytest.raises(ValueError, match="ctheta_max"):
            vm.DynamicSmagorinskyModel(heat_flux="dynamic", ctheta_max=bad)
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "nsfem.h")) as fh:
        header = fh.read()
    for name in ("nsfem_set_scalar_sgs_dynamic", "nsfem_scalar_dynamic_constant", "nsfem_scalar_diffusivity_cells",
                 "nsfem_scalar_dynamic_info"):
        assert re.search(r"\bint\s+%s\s*\(\s*nsfem_ctx\s*\*" % name, header), name
        assert name in nat.EXPORTED_SYMBOLS
    assert "No subgrid heat flux goes with this law" not in header
    assert "No subgrid heat flux goes with this model" not in vm.DynamicSmagorinskyModel.__doc__
    for method in ("set_scalar_sgs_dynamic", "scalar_dynamic_constant", "scalar_diffusivity_cells",
                   "scalar_dynamic_info"):
        assert callable(getattr(nat.NsfemContext, method))
    assert callable(ProblemBase._compute_model_scalar_constant) and callable(ProblemBase._compute_model_diffusivity)
    import inspect
    assert "set_scalar_sgs_dynamic" in inspect.getsource(BoussinesqIMEXSolver._push_scalar_sgs)
