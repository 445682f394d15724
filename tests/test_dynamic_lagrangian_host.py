"""Lagrangian-averaged dynamic Smagorinsky model: what can be checked of its restatement (tests/dynamic_lagrangian_host.py)
and of the model class without a GPU.  DESIGN.md 4w.

Meshes: box(4, 4) and the Kuhn box (3, 2, 2) on 1 x 0.8 x 0.6 of the GPU tests.  Tolerances: locate-and-interpolate of
a linear field is exact up to rounding -- 1e-13 of the largest value, a few hundred eps for the dozen operations of
rules 1 to 3 with gradients of size 1 / h <= 8."""
import math

import numpy as np
import pytest

from dynamic_lagrangian_host import LagrangianDynamicRestatement
from test_variable_viscosity_host import _cube, _square
from viscosity_models import DynamicSmagorinskyModel

_KUHN = ((3, 2, 2), (1.0, 0.8, 0.6))
_CACHE = {}


def _case(dim):
    if dim not in _CACHE:
        mesh, dm, rs = _square(4) if dim == 2 else _cube(*_KUHN)
        _CACHE[dim] = (mesh, dm, rs, LagrangianDynamicRestatement(rs))
    return _CACHE[dim]


def _interior(dm, lengths):
    X = dm.p1_coords
    return np.all((X > 1e-12) & (X < np.asarray(lengths)[None, :] - 1e-12), axis=1)


def _linear_state(X):
    dim = X.shape[1]
    b = np.array([[0.7, -0.4, 0.25], [0.3, 0.5, -0.2]])[:, :dim]
    return np.stack([2.0 + X @ b[0], 1.5 + X @ b[1]], axis=1), b


def _uniform(dim):
    return np.array([0.6, -0.35, 0.45])[:dim]


def _spacing(dim):
    return 0.25 if dim == 2 else min(1.0 / 3.0, 0.4, 0.3)


def _vert(orc, lm=0.02, mm=1.0):
    return np.stack([orc.patch_volume, np.full(orc.s.n1, lm), np.full(orc.s.n1, mm)], axis=1)


@pytest.mark.parametrize("dim", (2, 3))
def test_linear_state_is_interpolated_exactly_upstream(dim):
    """I = a + b . x, uniform u at CFL 0.4: at the interior vertices I_up = I(x_v + d) to rounding, nothing is clamped"""
    mesh, dm, rs, orc = _case(dim)
    X = dm.p1_coords
    state, b = _linear_state(X)
    w = _uniform(dim)
    k = 0.4 * _spacing(dim) / np.abs(w).max()
    out = orc.advance(_vert(orc), orc.vertex_delta2, np.tile(w, (rs.n1, 1)), k, state)
    inside = _interior(dm, (1.0, 1.0) if dim == 2 else _KUHN[1])
    assert inside.sum() >= 2 and not out["clamped"][inside].any()
    want, _ = _linear_state(X - k * w[None, :])
    err = np.abs(out["upstream"] - want)[inside].max() / np.abs(want).max()
    print("linear state dim %d: upstream error %.2e" % (dim, err))
    assert err < 1e-13
    assert np.abs(out["upstream"] - state)[inside].max() > 1e-3          # (the point did move)


@pytest.mark.parametrize("dim", (2, 3))
def test_zero_displacement_returns_the_vertex_value_bit_for_bit(dim):
    mesh, dm, rs, orc = _case(dim)
    rng = np.random.default_rng(5)
    state = rng.uniform(0.1, 2.0, (rs.n1, 2))
    out = orc.advance(_vert(orc), orc.vertex_delta2, np.zeros((rs.n1, dim)), 0.01, state)
    assert out["upstream"].tobytes() == state.tobytes()
    assert not out["clamped"].any() and np.all(out["best"] == 0.0)
    own = out["ids"] == np.arange(rs.n1)[:, None]
    assert np.all(out["lam"][own] == 1.0) and np.all(out["lam"][~own] == 0.0)


def test_relaxation_drives_the_ratio_to_the_local_one_monotonically():
    """fixed vert, zero displacement: I_LM / I_MM moves from cs2_init = 0.0256 to LM / MM = 0.06 without overshoot"""
    mesh, dm, rs, orc = _case(2)
    vert = _vert(orc, lm=0.06, mm=1.0)
    state = orc.advance(vert, orc.vertex_delta2, None, 0.05, None)["state"]
    assert np.allclose(state[:, 0] / state[:, 1], 0.0256, rtol=1e-15)
    ratios = [state[:, 0] / state[:, 1]]
    for _ in range(400):
        out = orc.advance(vert, orc.vertex_delta2, np.zeros((rs.n1, 2)), 0.05, state)
        assert np.all((out["eps"] > 0.0) & (out["eps"] < 1.0))
        state = out["state"]
        ratios.append(state[:, 0] / state[:, 1])
    r = np.array(ratios)
    assert np.all(np.diff(r, axis=0) >= 0.0) and np.all(r <= 0.06 * (1 + 1e-14))
    print("relaxation: ratio after 400 steps %.6f (local 0.06)" % r[-1].min())
    assert np.abs(r[-1] - 0.06).max() < 1e-6
    assert np.array_equal(out["cs2"], np.minimum(np.maximum(state[:, 0] / state[:, 1], 0.0), 0.09))


def test_floor_and_the_memoryless_branch():
    """a negative LM_v is held at cs2_floor I_MM'; a state whose product is not > 0 has no memory: eps = 1"""
    mesh, dm, rs, orc = _case(2)
    n1 = rs.n1
    floored = LagrangianDynamicRestatement(rs, lagrangian=(1.5, 0.0256, 1e-3))
    vert = _vert(floored, lm=-0.5, mm=2.0)
    state = np.tile([0.01, 1.0], (n1, 1))
    out = floored.advance(vert, floored.vertex_delta2, np.zeros((n1, 2)), 0.05, state)
    assert np.all(out["eps"] < 1.0) and np.all(out["state"][:, 0] == 1e-3 * out["state"][:, 1])
    assert np.all(out["cs2"] == 1e-3)
    for dead in (np.tile([0.0, 1.0], (n1, 1)), np.tile([-0.3, 1.0], (n1, 1)), np.zeros((n1, 2))):
        out = floored.advance(vert, floored.vertex_delta2, np.zeros((n1, 2)), 0.05, dead)
        assert np.all(out["eps"] == 1.0)
        assert np.all(out["state"][:, 1] == 2.0) and np.all(out["state"][:, 0] == 2e-3)


@pytest.mark.parametrize("dim", (2, 3))
def test_rest_and_constant_velocity_give_exact_zeros(dim):
    mesh, dm, rs, orc = _case(dim)
    for u in (np.zeros(dim * dm.n_p2), np.tile([0.3, -1.7, 0.9][:dim], dm.n_p2)):
        vert = orc.vertices(u)
        assert np.all(vert[:, 1:] == 0.0)
        first = orc.advance(vert, orc.vertex_delta2, None, 0.05, None)
        out = orc.advance(vert, orc.vertex_delta2, orc.vertex_velocity(u), 0.05, first["state"])
        for o in (first, out):
            assert np.all(o["state"] == 0.0) and np.all(o["upstream"] == 0.0) and np.all(o["cs2"] == 0.0)
        orc.vertex_constants = out["cs2"]
        assert np.all(orc.residual(u) == 0.0)
        orc.vertex_constants = None


@pytest.mark.parametrize("dim", (2, 3))
def test_clamped_upstream_value_is_a_convex_combination(dim):
    """CFL 2.5: the point leaves the patch at every vertex; the clamped coordinates are >= 0 and sum to 1, so the
    upstream value lies within the extremes of the vertices of c*"""
    mesh, dm, rs, orc = _case(dim)
    rng = np.random.default_rng(11)
    state = rng.uniform(0.1, 2.0, (rs.n1, 2))
    w = _uniform(dim)
    k = 2.5 * _spacing(dim) / np.abs(w).min()
    out = orc.advance(_vert(orc), orc.vertex_delta2, np.tile(w, (rs.n1, 1)), k, state)
    assert out["clamped"].all()
    assert np.all(out["lam"] >= 0.0) and np.abs(out["lam"].sum(axis=1) - 1.0).max() < 4e-16
    lo, hi = state[out["ids"]].min(axis=1), state[out["ids"]].max(axis=1)
    tol = 4e-16 * np.abs(state).max()
    assert np.all(out["upstream"] >= lo - tol) and np.all(out["upstream"] <= hi + tol)


def test_time_levels_form_once_rotate_and_initialise():
    mesh, dm, rs, orc = _case(2)
    X = dm.p2_coords
    u = np.stack([np.sin(2.0 * X[:, 1]) + X[:, 0] ** 2, np.cos(1.5 * X[:, 0]) * X[:, 1]], axis=1).ravel()
    orc.reset()
    prev = orc.level_constants(0.9 * u, 1, 0.01)                       # no cs2_prev: rule 6 on u2, nothing written
    assert orc.I is None and orc.cs2_prev is None and orc.cs2_cur is None
    first = orc.form_level(u, 0.01)
    assert first is orc.form_level(1.1 * u, 0.01)                      # formed once
    assert np.array_equal(orc.I_new[:, 0], orc.cs2_init * orc.I_new[:, 1]) and orc.I is None
    orc.rotate()
    assert orc.cs2_cur is None and orc.cs2_prev is first and orc.I is not None
    assert orc.level_constants(0.9 * u, 1, 0.01) is first and prev.shape == first.shape
    second = orc.form_level(1.1 * u, 0.01)
    assert np.all(second >= 0.0) and np.all(second <= 0.09)
    orc.reset()


def test_model_class_takes_the_lagrangian_mode_and_refuses_what_does_not_go_with_it():
    m = DynamicSmagorinskyModel(averaging="lagrangian", relaxation=1.5, cs2_init=0.0256)
    assert m.lagrangian and m.law_id == 8 and m.averaging_params() == (1.5, 0.0256, 1e-12)
    assert m.params() == (2.0, 0.09, 0.0, 0.0) and m.prandtl_t is None
    n, ids = m.vertex_groups(np.zeros((5, 2)))
    assert n == 1 and not ids.any()
    assert not DynamicSmagorinskyModel().lagrangian and not DynamicSmagorinskyModel(("planes", 1)).lagrangian
    with pytest.raises(ValueError, match="heat_flux"):
        DynamicSmagorinskyModel(averaging="lagrangian", heat_flux="dynamic")
    for bad in (0.0, -1.0, math.nan, math.inf):
        with pytest.raises(ValueError, match="relaxation"):
            DynamicSmagorinskyModel(averaging="lagrangian", relaxation=bad)
    for name in ("cs2_init", "cs2_floor"):
        for bad in (-1e-3, math.nan, math.inf):
            with pytest.raises(ValueError, match=name):
                DynamicSmagorinskyModel(averaging="lagrangian", **{name: bad})
    with pytest.raises(ValueError, match="averaging"):
        DynamicSmagorinskyModel(averaging="pathlines")
