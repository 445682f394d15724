"""Subgrid heat flux of the scalar step: what can be checked of its numpy restatement
(tests/scalar_sgs_host.py) without a GPU, in 2D and 3D, and that every layer carries the feature."""
import math
import os
import re

import numpy as np
import pytest

from scalar_sgs_host import ScalarIMEXSgsRestatement, ScalarSgsRestatement
from test_scalar_transport_host import smooth_fields
from test_variable_viscosity_host import _cube, _shear, _square

_CS, _PRT = 0.9, 0.6


def _case(dim):
    return _square(4) if dim == 2 else _cube()


def _linear_T(X):
    a = np.array([0.7, -1.1, 0.4])[:X.shape[1]]
    return X @ a + 0.3


@pytest.mark.parametrize("dim", (2, 3))
def test_constant_scalar_feels_no_subgrid_flux(dim):
    """grad of a constant: T = 0 gives D = 0 exactly.  For T = 1 the 6 / 10 physical P2 gradients of a point sum to zero
    only to rounding (a few eps of their size, about 3 / h), so D is held to 1e-13 of the D of a linear T with
    |grad T| of order one -- measured 3e-18 and 6e-18 against 3e-2"""
    mesh, dm, s = _case(dim)
    u, _ = smooth_fields(dm.p2_coords)
    sgs = ScalarSgsRestatement(s, _CS, _PRT)
    assert np.all(sgs.residual(u, np.zeros(s.n2)) == 0.0)
    one = np.abs(sgs.residual(u, np.ones(s.n2))).max()
    scale = np.abs(sgs.residual(u, _linear_T(dm.p2_coords))).max()
    print("constant T dim %d: |D| %.2e of %.2e" % (dim, one, scale))
    assert scale > 1e-4 and one <= 1e-13 * scale


@pytest.mark.parametrize("dim", (2, 3))
def test_rigid_motion_feels_no_subgrid_flux(dim):
    """u = a + W x with W skew: g + g^T is round-off, a few eps of the gradient sums (6 / 10 terms of size |u| / h), and
    kappa_x is linear in it: |D| <= 1e-12 of the shear case"""
    mesh, dm, s = _case(dim)
    X = dm.p2_coords
    if dim == 2:
        W, a = np.array([[0.0, -0.7], [0.7, 0.0]]), np.array([0.3, -0.2])
    else:
        W, a = np.array([[0.0, -0.7, 0.4], [0.7, 0.0, -1.1], [-0.4, 1.1, 0.0]]), np.array([0.3, -0.2, 0.5])
    u = (a[None, :] + X @ W.T).ravel()
    _, T = smooth_fields(X)
    sgs = ScalarSgsRestatement(s, _CS, _PRT)
    rigid = np.abs(sgs.residual(u, T)).max()
    shear = np.abs(sgs.residual(_shear(X), T)).max()
    print("rigid dim %d: %.2e of shear %.2e" % (dim, rigid, shear))
    assert shear > 1e-4 and rigid <= 1e-12 * shear


@pytest.mark.parametrize("dim", (2, 3))
def test_linear_shear_with_linear_scalar_is_a_constant_diffusivity(dim):
    """u = (s y, 0 (, 0)), T linear on box(4, 4) and the (2, 2, 2) Kuhn box: gamma = |s| and Delta_K are the same
    everywhere, so D(u, T) = kappa_x K T with the closed form kappa_x = (C_s Delta)^2 |s| / Pr_t; 1e-13 relative"""
    mesh, dm, s = _case(dim)
    shear = 1.3
    u, T = _shear(dm.p2_coords, shear), _linear_T(dm.p2_coords)
    sgs = ScalarSgsRestatement(s, _CS, _PRT)
    delta = (1.0 / 16.0 / 2.0) ** 0.5 if dim == 2 else (1.0 / 8.0 / 6.0) ** (1.0 / 3.0)
    kx = (_CS * delta) ** 2 * abs(shear) / _PRT
    want = kx * (s.stiffness_p2() @ T)
    got = sgs.residual(u, T)
    err = np.linalg.norm(got - want) / np.linalg.norm(want)
    print("shear dim %d: kappa_x %.6g rel %.2e" % (dim, kx, err))
    assert kx > 1e-3 and np.linalg.norm(want) > 1e-3 and err < 1e-13
    assert np.abs(sgs.kappa_x(u) - kx).max() < 1e-13 * kx
    assert np.abs(sgs.cell_means(u) - kx).max() < 1e-13 * kx


@pytest.mark.parametrize("dim", (2, 3))
def test_scalar_dissipation_identity(dim):
    """T . D(u, T) = sum_K sum_q w_q |det J| kappa_x |grad T|^2 (the test function is T itself) and is >= 0: the term
    drains the scalar variance; smooth non-polynomial fields, 1e-13 relative"""
    mesh, dm, s = _square(4) if dim == 2 else _cube((3, 2, 2), (1.0, 0.8, 0.6))
    u, T = smooth_fields(dm.p2_coords)
    sgs = ScalarSgsRestatement(s, _CS, _PRT)
    lhs, rhs = float(T @ sgs.residual(u, T)), sgs.dissipation(u, T)
    print("scalar dissipation dim %d: %.12e against %.12e" % (dim, lhs, rhs))
    assert rhs > 1e-4 and abs(lhs - rhs) < 1e-13 * rhs and lhs >= 0.0


@pytest.mark.parametrize("dim", (2, 3))
def test_turbulent_prandtl_number_is_an_exact_divisor(dim):
    """Pr_t -> 2 Pr_t, 4 Pr_t halves and quarters every byte-level quantity exactly (a power of two); Pr_t = 1 gives
    nu_x of the viscosity restatement itself"""
    mesh, dm, s = _case(dim)
    u, T = smooth_fields(dm.p2_coords)
    base = ScalarSgsRestatement(s, _CS, _PRT)
    for factor in (2.0, 4.0):
        other = ScalarSgsRestatement(s, _CS, factor * _PRT)
        assert np.array_equal(other.kappa_x(u) * factor, base.kappa_x(u))
        assert np.array_equal(other.residual(u, T) * factor, base.residual(u, T))
    unit = ScalarSgsRestatement(s, _CS, 1.0)
    assert np.array_equal(unit.kappa_x(u), unit.visc._at_points(u)[2])
    assert np.array_equal(unit.cell_means(u), unit.visc.cell_means(u))


def test_restated_step_carries_the_term_in_both_stored_vectors():
    """one SBDF2 step of ScalarIMEXSgsRestatement: N1 = C T1 + D(u1, T1), a missing N2 is formed with D(u2, T2), and
    sgs = None is the parent's step byte for byte"""
    import fem_oracle as fo
    from test_scalar_transport_host import ScalarIMEXRestatement
    mesh, dm, s = _square(4)
    base = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
    u, T = smooth_fields(dm.p2_coords)
    sgs = ScalarSgsRestatement(s, _CS, _PRT)
    alpha, beta, gamma, k = (1.5, -2.0, 0.5), (2.0, -1.0), (1.0, 0.0, 0.0), 1.0 / 16.0
    orc = ScalarIMEXSgsRestatement(base, 0.05, "standard", sgs)
    off = ScalarIMEXSgsRestatement(base, 0.05, "standard", None)
    ref = ScalarIMEXRestatement(base, 0.05, "standard")
    for o in (orc, off, ref):
        o.T[1], o.T[2] = T.copy(), 0.9 * T
        o.step(alpha, beta, gamma, k, u, 0.8 * u)
    assert np.array_equal(off.T[0], ref.T[0]) and np.array_equal(off.N1, ref.N1)
    assert np.array_equal(orc.N1, ref.N1 + sgs.residual(u, T))
    A = (alpha[0] / k) * orc.M + gamma[0] * 0.05 * orc.K
    extra = beta[0] * sgs.residual(u, T) + beta[1] * sgs.residual(0.8 * u, 0.9 * T)
    assert np.abs(A @ (orc.T[0] - ref.T[0]) + extra).max() < 1e-12 * np.abs(extra).max()


def test_model_validates_the_turbulent_prandtl_number():
    import viscosity_models as vm
    m = vm.SmagorinskyModel(0.17)
    assert m.prandtl_t is None and tuple(m.params()) == (0.17, 0.0, 0.0, 0.0)
    m = vm.SmagorinskyModel(0.17, prandtl_t=0.85)
    assert m.prandtl_t == 0.85 and m.law_id == 1 and tuple(m.params()) == (0.17, 0.0, 0.0, 0.0)
    assert vm.SmagorinskyModel(0.17, 2).prandtl_t == 2.0
    for bad in (0.0, -0.4, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            vm.SmagorinskyModel(0.17, prandtl_t=bad)
    assert math.isfinite(vm.SmagorinskyModel(0.0, prandtl_t=1e-3).prandtl_t)


def test_every_layer_carries_the_feature():
    """the C header declares the three entry points, _native lists and binds them, the solver pushes prandtl_t with the
    model and with the scalar coefficients, the problem base has the output helper"""
    import _native as nat
    import viscosity_models as vm
    from ns_boussinesq_solver import BoussinesqIMEXSolver
    from ns_imex_solver import IMEXIPCSSolver
    from ns_problem import ProblemBase
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "nsfem.h")) as fh:
        header = fh.read()
    for name in ("nsfem_set_scalar_sgs", "nsfem_scalar_explicit", "nsfem_scalar_sgs_info"):
        assert re.search(r"\bint\s+%s\s*\(\s*nsfem_ctx\s*\*" % name, header), name
        assert name in nat.EXPORTED_SYMBOLS
    for method in ("set_scalar_sgs", "scalar_explicit", "scalar_sgs_info"):
        assert callable(getattr(nat.NsfemContext, method))
    assert callable(ProblemBase._compute_model_diffusivity)
    assert callable(BoussinesqIMEXSolver._push_scalar_sgs)
    assert BoussinesqIMEXSolver._push_viscosity_model is not IMEXIPCSSolver._push_viscosity_model
    assert not hasattr(IMEXIPCSSolver, "_push_scalar_sgs")          # (no other solver class changes)

    class _Ctx:
        def __init__(self):
            self.calls = []

        def set_scalar_sgs(self, value):
            self.calls.append(("sgs", value))

        def set_viscosity_law(self, *args):
            self.calls.append(("law", ) + args)

        def set_scalar(self, *args):
            self.calls.append(("scalar", ) + args)

    solver = BoussinesqIMEXSolver.__new__(BoussinesqIMEXSolver)
    solver._ctx = _Ctx()
    solver._equation_coefficients = dict(viscous_term=0.01)
    solver._space_dim = 2
    solver.set_viscosity_model(vm.SmagorinskyModel(0.2, prandtl_t=0.5))
    assert solver._ctx.calls == [("law", 1, (0.2, 0.0, 0.0, 0.0)), ("sgs", 0.5)]
    solver._ctx.calls.clear()
    solver.set_scalar_coefficients(0.05, (0.0, 1.0))
    assert solver._ctx.calls == [("scalar", 0.05, (0.0, 1.0), 0), ("sgs", 0.5)]
    solver._ctx.calls.clear()
    solver.set_viscosity_model(vm.SmagorinskyModel(0.2))            # no prandtl_t: 0
    solver.set_viscosity_model(None)                                # no model: 0
    assert [c for c in solver._ctx.calls if c[0] == "sgs"] == [("sgs", 0.0), ("sgs", 0.0)]
