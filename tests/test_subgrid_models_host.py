"""WALE and Vreman subgrid viscosities (laws 4 and 5): what can be checked of their numpy restatement
(tests/subgrid_models_host.py) without a GPU -- the pointwise laws, the restatement on the test meshes, the model
classes and that every layer documents the laws."""
import os
import re

import numpy as np
import pytest

from scalar_sgs_host import ScalarIMEXSgsRestatement, ScalarSgsRestatement
from subgrid_models_host import (VREMAN, WALE, SubgridModelRestatement, SubgridScalarSgsRestatement, embed, tensor_nu,
                                 vreman_nu, wale_nu)
from test_scalar_transport_host import smooth_fields
from test_variable_viscosity_host import (SMAGORINSKY, IMEXViscRestatement, VariableViscosityRestatement, _cube, _shear,
                                          _square)

_LAWS = ((WALE, (0.5, )), (VREMAN, (0.07, )))


# ---------------------------------------------------------------- the pointwise laws
def _near_wall_gradient(y):
    """G of u = (a y, b y^2, c y) at height y over the wall y = 0, a, b, c smooth in (x, z) with a_x + c_z = -2 b
    (divergence free to the order kept)"""
    a, c = 1.0, 0.6
    a_x, a_z, c_x, c_z = 0.7, -0.4, 0.5, 0.3
    b, b_x, b_z = -0.5 * (a_x + c_z), 0.2, -0.3
    return np.array([[a_x * y, a, a_z * y], [b_x * y * y, 2.0 * b * y, b_z * y * y], [c_x * y, c, c_z * y]])


def _smagorinsky_nu(G, delta2, cs):
    sym = G + np.swapaxes(G, -1, -2)
    return cs * cs * delta2 * np.sqrt(0.5 * (sym * sym).sum(axis=(-1, -2)))


@pytest.mark.parametrize("name,law,exponent", [("WALE", lambda G: wale_nu(G, 1.0, 0.5), 3.0),
                                               ("Vreman", lambda G: vreman_nu(G, 1.0, 0.07), 1.0),
                                               ("Smagorinsky", lambda G: _smagorinsky_nu(G, 1.0, 0.17), 0.0)])
def test_near_wall_exponents(name, law, exponent):
    """nu_x ~ y^3 (WALE), y (Vreman), const (Smagorinsky) on the near-wall field: the slope of log nu_x against log y
    between y = 1e-2 and y = 1e-4, within 0.01"""
    hi, lo = law(_near_wall_gradient(1e-2)), law(_near_wall_gradient(1e-4))
    slope = np.log(hi / lo) / np.log(1e-2 / 1e-4)
    print("near wall %s: nu_x %.3e at 1e-2, %.3e at 1e-4, exponent %.4f" % (name, hi, lo, slope))
    assert hi > 0.0 and lo > 0.0 and abs(slope - exponent) < 0.01


@pytest.mark.parametrize("law,params", _LAWS)
def test_pure_shear_and_zero_gradient_give_zero(law, params):
    """G = s e_x e_y^T: H = 0 so Sd = 0, every 2x2 minor is 0 -- nu_x is exactly 0 in both dimensions where Smagorinsky
    gives (C_s Delta)^2 |s|; G = 0 gives 0, not NaN (the 0 / 0 guards)"""
    for d in (2, 3):
        G = np.zeros((d, d))
        zero = tensor_nu(law, G, 0.3, params[0])
        assert zero == 0.0 and np.isfinite(zero)
        G[0, 1] = 1.3
        assert tensor_nu(law, G, 0.3, params[0]) == 0.0
        assert _smagorinsky_nu(G, 0.3, 0.17) > 1e-3


@pytest.mark.parametrize("law,params", _LAWS)
def test_two_dimensional_value_is_that_of_the_z_independent_extension(law, params):
    """the d = 2 code path (Sd_33 kept, one minor) against the d = 3 path on the embedded tensor: 4 eps relative, the
    sums differ only in exact zeros and their order"""
    rng = np.random.default_rng(7)
    G2 = rng.standard_normal((200, 2, 2))
    two, three = tensor_nu(law, G2, 0.3, params[0]), tensor_nu(law, embed(G2), 0.3, params[0])
    err = np.abs(two - three).max() / np.abs(three).max()
    print("2D against embedded 3D law %d: %.2e" % (law, err))
    assert np.abs(three).min() > 0.0 and err <= 4.0 * 2.0 ** -52


def test_wale_is_the_textbook_formula_where_that_is_well_conditioned():
    """(C_w Delta)^2 (Sd:Sd)^(3/2) / ((S:S)^(5/2) + (Sd:Sd)^(5/4)) with pow and the traceless part formed from the full
    3x3 matrices, on random tensors; Vreman against beta = G G^T (alpha_ij = d_i u_j = G^T): B_beta = the second invariant
    b11 b22 - b12^2 + b11 b33 - b13^2 + b22 b33 - b23^2 of alpha^T alpha = G G^T; 1e-12 relative (the invariant cancels)"""
    rng = np.random.default_rng(11)
    G = rng.standard_normal((100, 3, 3))
    S = 0.5 * (G + np.swapaxes(G, 1, 2))
    H = G @ G
    Sd = 0.5 * (H + np.swapaxes(H, 1, 2)) - np.trace(H, axis1=1, axis2=2)[:, None, None] / 3.0 * np.eye(3)
    A, B = (S * S).sum(axis=(1, 2)), (Sd * Sd).sum(axis=(1, 2))
    want = 0.25 * 0.3 * B ** 1.5 / (A ** 2.5 + B ** 1.25)
    assert np.abs(wale_nu(G, 0.3, 0.5) - want).max() < 1e-14 * want.max()
    beta = G @ np.swapaxes(G, 1, 2)
    bb = (beta[:, 0, 0] * beta[:, 1, 1] - beta[:, 0, 1] ** 2 + beta[:, 0, 0] * beta[:, 2, 2] - beta[:, 0, 2] ** 2 +
          beta[:, 1, 1] * beta[:, 2, 2] - beta[:, 1, 2] ** 2)
    want = 0.07 * 0.3 * np.sqrt(bb / np.trace(beta, axis1=1, axis2=2))
    assert np.abs(vreman_nu(G, 0.3, 0.07) - want).max() < 1e-12 * want.max()


# ---------------------------------------------------------------- the restatement on the test meshes
def _case(dim):
    return _square(4) if dim == 2 else _cube((3, 2, 2), (1.0, 0.8, 0.6))


@pytest.mark.parametrize("law,params", _LAWS)
@pytest.mark.parametrize("dim", (2, 3))
def test_dissipation_identity_and_sign(dim, law, params):
    """u . V(u) = sum_K sum_q w_q |det J| nu_x gamma^2 for the smooth non-polynomial field, 1e-13 relative, and >= 0:
    both laws are non-negative by construction"""
    mesh, dm, s = _case(dim)
    u, _ = smooth_fields(dm.p2_coords)
    v = SubgridModelRestatement(s, law, params)
    lhs, rhs = float(u @ v.residual(u)), v.dissipation(u)
    print("dissipation dim %d law %d: %.12e against %.12e, max nu_x %.3e" % (dim, law, lhs, rhs, v.nu_max(u)))
    assert rhs > 1e-5 and abs(lhs - rhs) < 1e-13 * rhs and lhs >= 0.0
    assert v._at_points(u)[2].min() >= 0.0


@pytest.mark.parametrize("law,params", _LAWS)
@pytest.mark.parametrize("dim", (2, 3))
def test_linear_shear_and_rest_feel_no_model_viscosity(dim, law, params):
    """u = (1.3 y, 0 (, 0)) as a P2 field: the point gradients carry rounding, so WALE is tiny instead of zero (its
    B is the square of a rounding error: <= 5e-46 measured), Vreman exactly 0 in 2D and rounding squared in 3D; both
    below 1e-20 of Smagorinsky's C_s = 0.17 cell mean.  u = 0: V and the cell means are exactly 0 and finite"""
    mesh, dm, s = _case(dim)
    v = SubgridModelRestatement(s, law, params)
    u = _shear(dm.p2_coords)
    means = v.cell_means(u)
    smag = VariableViscosityRestatement(s, SMAGORINSKY, (0.17, )).cell_means(u)
    print("shear dim %d law %d: largest cell mean %.2e, Smagorinsky %.2e" % (dim, law, means.max(), smag.min()))
    assert smag.min() > 1e-5 and means.max() <= 1e-20 * smag.min()
    zero = np.zeros_like(u)
    assert np.all(v.residual(zero) == 0.0) and np.all(v.cell_means(zero) == 0.0)
    assert np.all(np.isfinite(v._at_points(zero)[2]))


@pytest.mark.parametrize("law,params", _LAWS)
@pytest.mark.parametrize("dim", (2, 3))
def test_rigid_rotation_has_a_viscosity_but_no_force(dim, law, params):
    """u = W x with W skew.  Known of both laws: nu_x does NOT vanish in solid-body rotation (WALE: S = 0 but
    Sd = sym(W W) - tr/3 I is not; Vreman: the minors of W are not zero) -- asserted non-zero here.  V = 0 all the same,
    to rounding, because the strain nu_x multiplies vanishes: max |V| < 1e-12 of the pure strain u = (x, -y (, 0))"""
    mesh, dm, s = _case(dim)
    X = dm.p2_coords
    W = np.array([[0.0, -0.7], [0.7, 0.0]]) if dim == 2 else np.array([[0.0, -0.7, 0.4], [0.7, 0.0, -1.1],
                                                                          [-0.4, 1.1, 0.0]])
    v = SubgridModelRestatement(s, law, params)
    rot = (X @ W.T).ravel()
    strain = np.zeros_like(X)
    strain[:, 0], strain[:, 1] = X[:, 0], -X[:, 1]
    rigid, ref = np.abs(v.residual(rot)).max(), np.abs(v.residual(strain.ravel())).max()
    nu = v.cell_means(rot)
    print("rotation dim %d law %d: |V| %.2e of strain %.2e, nu_x in rotation %.3e" % (dim, law, rigid, ref, nu.min()))
    assert nu.min() > 1e-5 and ref > 1e-5 and rigid < 1e-12 * ref


@pytest.mark.parametrize("law,params", _LAWS)
def test_the_other_restatements_take_the_new_laws(law, params):
    """IMEXViscRestatement(visc=...), ScalarSgsRestatement's subclass and ScalarIMEXSgsRestatement accept the new
    restatement: the explicit vectors are convection plus V, and C T plus D with kappa_x = nu_x / Pr_t; laws 1 and 2
    through the new class are the parent's bytes"""
    import fem_oracle as fo
    mesh, dm, rs = _square(4)
    s = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
    u, T = smooth_fields(dm.p2_coords)
    v = SubgridModelRestatement(rs, law, params)
    coef = dict(convective_term=1.0, pressure_term=1.0, viscous_term=0.01, body_force_term=None)
    flow = IMEXViscRestatement(s, coef, "standard", visc=v)
    assert np.array_equal(flow.explicit(u), s.convection_residual(u, "standard") + v.residual(u))
    sgs = SubgridScalarSgsRestatement(rs, law, params, 0.85)
    assert isinstance(sgs, ScalarSgsRestatement)
    assert np.array_equal(sgs.kappa_x(u), v._at_points(u)[2] / 0.85)
    assert np.array_equal(sgs.cell_means(u), v.cell_means(u) / 0.85)
    orc = ScalarIMEXSgsRestatement(s, 0.05, "standard", sgs)
    assert np.array_equal(orc.explicit(u, T), orc.convection_matrix(u) @ T + sgs.residual(u, T))
    assert np.abs(sgs.residual(u, T)).max() > 1e-5
    # the identity of the scalar term: T . D(u, T) = int kappa_x |grad T|^2 >= 0
    lhs, rhs = float(T @ sgs.residual(u, T)), sgs.dissipation(u, T)
    assert rhs > 0.0 and abs(lhs - rhs) < 1e-13 * rhs
    for old, prm in ((1, (0.9, )), (2, (0.07, 1.7, 0.6))):
        assert np.array_equal(SubgridModelRestatement(rs, old, prm).residual(u),
                              VariableViscosityRestatement(rs, old, prm).residual(u))


# ---------------------------------------------------------------- model classes and layers
def test_model_classes_validate_and_carry_their_law():
    import viscosity_models as vm
    assert (vm.LAW_WALE, vm.LAW_VREMAN) == (4, 5) == (WALE, VREMAN)
    m = vm.WALEModel(0.5)
    assert m.law_id == 4 and tuple(m.params(dict(viscous_term=0.01))) == (0.5, 0.0, 0.0, 0.0) and m.prandtl_t is None
    assert tuple(m.params()) == (0.5, 0.0, 0.0, 0.0)
    m = vm.VremanModel(0.07, prandtl_t=0.85)
    assert m.law_id == 5 and tuple(m.params(None)) == (0.07, 0.0, 0.0, 0.0) and m.prandtl_t == 0.85
    assert vm.WALEModel(0.0).cw == 0.0 and vm.VremanModel(0).c == 0.0 and vm.WALEModel(0.5, 0.4).prandtl_t == 0.4
    for cls in (vm.WALEModel, vm.VremanModel):
        for bad in (-0.1, float("nan"), float("inf"), -float("inf")):
            with pytest.raises(ValueError, match=cls.__name__):
                cls(bad)
        for bad in (0.0, -0.5, float("nan"), float("inf")):
            with pytest.raises(ValueError, match="prandtl_t"):
                cls(0.1, prandtl_t=bad)
    # what was there stays
    assert vm.SmagorinskyModel(0.17).law_id == 1 and vm.CarreauModel(0.002, 1.5, 0.6).law_id == 2


def test_every_layer_documents_the_laws():
    """the header defines laws 4 and 5 next to nsfem_set_viscosity_law, the integration notes, the design notes and
    the README name them, and the Python binding's docstring lists them"""
    import _native as nat
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    with open(os.path.join(root, "include", "nsfem.h")) as fh:
        header = fh.read()
    doc = header[header.index("variable viscosity in the IMEX step"):header.index("int nsfem_set_viscosity_law")]
    assert re.search(r"law 4\s+WALE", doc) and re.search(r"law 5\s+Vreman", doc)
    for word in ("Sd:Sd", "2x2 minors", "G:G", "C_w", "sqrt(sqrt(B))", "zero third row and column"):
        assert word in doc, word
    for name in ("INTEGRATION.md", "DESIGN.md", "README.md"):
        with open(os.path.join(root, name)) as fh:
            text = fh.read()
        assert "WALE" in text and "Vreman" in text, name
    assert "4 WALE" in nat.NsfemContext.set_viscosity_law.__doc__ and "5 Vreman" in nat.NsfemContext.set_viscosity_law.__doc__
