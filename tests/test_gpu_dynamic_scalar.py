"""Dynamic subgrid heat flux on the GPU (nsfem_set_scalar_sgs_dynamic: k_dyn_scalar_moments, k_dyn_scalar_vertex,
k_dyn_reduce, k_scalar_conv_cell<FORM, PENAL, 8> / k3_scalar_conv_cell<FORM, PENAL, 8>, k_wall_facets<DIM, 8> with the
second vertex field; nsfem_scalar_dynamic_constant, nsfem_scalar_diffusivity_cells, nsfem_scalar_dynamic_info;
DynamicSmagorinskyModel(heat_flux="dynamic") under BoussinesqIMEXSolver) against the numpy restatement of
tests/dynamic_scalar_host.py.  DESIGN.md 4u.

Tolerances.
  Procedure (W, PR, RR per vertex, num, den per group): the per-entry bound of the wall tests,
    2 n eps times the sum of the absolute contributions (``absolute=True`` of the restatement), n the rounded operations
    along the longest chain that ends in the entry, counted in ``_n_vertex``: a physical gradient 3 / 5, an entry of G or
    grad T over the 5 / 9 differences 1 + 10 / 1 + 18, gamma 7 / 11, gamma d_a T 1, the weight and the sum over the
    points 1 + 7 / 1 + 15, the scaling |K| Delta_K^2 / sum w with Delta_K 5 / 8, the patch sum of at most 8 / 24 cells and
    that of W with the division, hat gamma 8 / 14, alpha^2 Delta_v^2 hat gamma hat(d_a T) and the difference 5, the
    covariance 3, the contraction 2 dim: 72 / 137.  Group sums: one product, the strided sum ceil(n_g / 256), the tree
    6 + 3, on top of the vertex chain.
  ctheta_g: bit for bit clip(num / den) of the device's own sums (the fp64 division is correctly rounded).
  Element kernel (C T + D, cell means): 1e-13 of the largest entry, the tolerance of the family (4r, 4t); with a heated
    body (C T + D + H) the two figures of tests/test_gpu_heated_bodies.py for sharp and smoothed masks.
  Steps: T 1e-9 relative, the figure of 4t's step test for u -- the same mechanism sits between device and host, a
    quotient of sums taken in different orders; u*, u as there.
  Wall heat row: the bound of tests/test_gpu_scalar_sgs.py for the fixed model, with dim + 4 more operations (the mean
    over the vertices, the product with c_K, the sum of the two parts of the reference).

Fields.  ``_sines`` with a sine temperature: every entry of G and grad T non-zero, for the procedure.  ``_les`` with
``_t5`` (2D) / T = y (3D): the fields of the step tests; the kernel cases are listed in ``_KERNEL_CASES`` with the
grouping, alpha and clip for which the restatement alone has c_K > 0 in at least half the cells and a term of at least
a quarter of C T (found by a search over the groupings on the CPU).  ``_clipped``: the fields for which every group
quotient is above 0.0625 at alpha = 1.1.

Meshes.  Those of tests/test_gpu_dynamic_model.py: the general tetrahedra with 72 and 384 cells run the procedure and
the element kernel with the global group."""

import numpy as np
import pytest

import _native as nat
from dynamic_model_host import DYNAMIC
from dynamic_scalar_host import DynamicScalarIMEXRestatement, DynamicScalarRestatement
from gpu_common import rel
from imex_time_stepping import IMEXTimeStepping, IMEXType
from periodic_meshes import is_periodic, lengths_of, periodic_axes, periodic_fields
from test_gpu_dynamic_model import CUBE, KUHN, _groupings, _groups, _host_steps, _les, _set, _sines, _step_setup
from test_gpu_variable_viscosity import GENERAL72, GENERAL384, NO_PBC, _max_rel, _mesh, _opts
from test_scalar_transport_host import ScalarIMEXRestatement, smooth_fields
from test_variable_viscosity_host import SMAGORINSKY
from viscosity_models import DynamicSmagorinskyModel

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
_MESHES = [(4, 4), (3, 5), "mapped", KUHN, CUBE, GENERAL72, GENERAL384, "pchan3"]
_FORMS = ((0, "standard"), (1, "skew_symmetric"))
_V_SLOTS = (nat.U0, nat.U1, nat.U2, nat.USTAR, nat.CONV_N1, nat.CONV_N2)
_T_SLOTS = (nat.T0, nat.T1)


def _n_vertex(dim):
    """rounded operations along the longest chain that ends in PR_v or RR_v (module docstring)"""
    two = dim == 2
    n_diff, n_q, patch = (5, 7, 8) if two else (9, 15, 24)
    return ((3 if two else 5) + (1 + 2 * n_diff) + (7 if two else 11) + 1 + (1 + n_q) + (5 if two else 8) +
            (2 * patch + 1) + (8 if two else 14) + 5 + 3 + 2 * dim)


def _sine_T(X):
    k = np.array([1.7, -0.9, 1.4])[:X.shape[1]]
    return 1.1 * np.sin(3.0 * (X @ k) + 0.4) + 0.3


def _t5(X):
    return X[:, 1] + 0.9 * np.sin(3.0 * np.pi * X[:, 0] + 1.7) * np.sin(3.0 * np.pi * X[:, 1] + 2.1)


def _periodic(X, kind="pchan3"):
    """the periodic velocity and scalar of tests/periodic_meshes.py: every entry of G and of grad T non-zero"""
    return periodic_fields(X, lengths_of(kind), periodic_axes(kind))


def _switch_on(ctx, dm, grouping, alpha, ctheta_max, cs2_max=0.09):
    _set(ctx, dm, grouping, (alpha, cs2_max))
    ctx.set_scalar_sgs_dynamic(True, ctheta_max)


def _convection(s, form, u, T):
    return ScalarIMEXRestatement(s, 0.0, form).convection_matrix(u) @ T


# ---------------------------------------------------------------- 1. the procedure against the restatement
_PROC_REF = {}


def _procedure_reference(kind, grouping):
    key = (kind, str(grouping))
    if key not in _PROC_REF:
        mesh, dm, marks, s, rs, make = _mesh(kind)
        u, T = _sines(dm.p2_coords), _sine_T(dm.p2_coords)
        if is_periodic(kind):
            u, T = _periodic(dm.p2_coords, kind)
        orc = DynamicScalarRestatement(rs, (2.0, 0.2), _groups(dm, grouping))
        _PROC_REF[key] = (u, T, orc, orc.vertices(u, T), orc.vertices(u, T, absolute=True), orc.sums(u, T),
                          orc.sums(u, T, absolute=True))
    return _PROC_REF[key]


@pytest.mark.parametrize("kind,grouping", [(k, g) for k in _MESHES for g in _groupings(k)], ids=str)
def test_procedure_matches_the_restatement(kind, grouping):
    """W, PR, RR per vertex and num, den per group inside their per-entry bounds; ctheta_g bit for bit the clipped
    quotient of the device's own sums; a second call returns the same bytes; no slot is written; the counters count and
    the procedure of law 8 itself does not run"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    u, T, orc, vert, vert_abs, sums, sums_abs = _procedure_reference(kind, grouping)
    dim = dm.dim
    g = orc.group
    assert np.abs(orc.gradient(u)).max(axis=(0, 1)).min() > 0.1 and np.abs(orc.grad_T(T)).max(axis=(0, 1)).min() > 0.1
    n_v = _n_vertex(dim)
    assert n_v == (72 if dim == 2 else 137)
    bound_v = 2.0 * n_v * EPS * vert_abs
    counts = np.bincount(g, minlength=orc.n_groups)
    bound_g = 2.0 * (n_v + 1 + (counts[:, None] + 255) // 256 + 9) * EPS * sums_abs
    ctx = make(mesh, dm)
    try:
        for slot in (nat.U0, nat.U1, nat.U2, nat.USTAR):
            ctx.set_state(slot, u if slot == nat.U1 else 0.5 * u)
        ctx.set_state(nat.T1, T)
        ctx.set_state(nat.T0, 0.5 * T)
        before = {slot: ctx.get_state(slot) for slot in _V_SLOTS + _T_SLOTS}
        assert ctx.scalar_dynamic_info() == dict(active=False, runs=0, launches=0, bytes=0)
        _switch_on(ctx, dm, grouping, 2.0, 0.2)
        assert ctx.scalar_dynamic_info() == dict(active=True, runs=0, launches=0, bytes=0)
        cth, got_s, got_v = ctx.scalar_dynamic_constant(nat.U1, nat.T1, details=True)
        ev, eg = np.abs(got_v - vert), np.abs(got_s - sums)
        with np.errstate(divide="ignore", invalid="ignore"):
            print("procedure %s %s: error / bound vertices %.3f groups %.3f; ctheta %s" % (
                kind, grouping, np.nanmax(ev / bound_v), np.nanmax(eg / bound_g), np.array2string(cth[:6], precision=4)))
        assert np.abs(vert[:, 1]).max() > 1e-6 and np.abs(vert[:, 2]).max() > 1e-6
        assert (ev <= bound_v).all() and (eg <= bound_g).all()
        assert cth.shape == (orc.n_groups, ) and cth.tobytes() == orc.clip(got_s).tobytes()
        again = ctx.scalar_dynamic_constant(nat.U1, nat.T1, details=True)
        for a, b in zip((cth, got_s, got_v), again):
            assert a.tobytes() == b.tobytes()
        assert np.array_equal(ctx.scalar_dynamic_constant(nat.U1, nat.T1), cth)
        for slot in _V_SLOTS + _T_SLOTS:
            assert ctx.get_state(slot).tobytes() == before[slot].tobytes()
        info = ctx.scalar_dynamic_info()
        assert info["active"] and info["runs"] == 3 and info["launches"] == 9 and info["bytes"] > 0
        assert ctx.dynamic_info()["runs"] == 0 and ctx.scalar_sgs_info() == dict(active=False, launches=0, recomputed=0)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 2. the element kernel against C T + D
def _les_fields(X):
    return _les(X), (_t5(X) if X.shape[1] == 2 else X[:, 1].copy())


def _les_smooth(X):
    return _les(X), smooth_fields(X)[1]


# kind: (fields, grouping, alpha, ctheta_max).  alpha = 1.1 gives the larger constants the 3D meshes need for a term of
# a quarter of C T (the quotient grows as alpha -> 1: R carries 1 - alpha^2)
_KERNEL_CASES = {(4, 4): (_les_fields, ("planes", 1), 2.0, 0.2), (3, 5): (_les_fields, ("planes", 0), 2.0, 0.2),
                 "mapped": (_les_fields, ("planes", 0), 2.0, 0.2), KUHN: (_les_smooth, ("planes", 0), 1.1, 1.0),
                 CUBE: (smooth_fields, ("planes", 1), 1.1, 1.0), GENERAL72: (_les_smooth, "global", 1.1, 1.0),
                 GENERAL384: (_les_smooth, "global", 1.1, 1.0),
                 # the periodic channel, plane groups parallel to the walls: the restatement gives 0.136, 0.267, 0.269
                 "pchan3": (_periodic, ("planes", 1), 1.1, 1.0)}


@pytest.mark.parametrize("kind", _MESHES, ids=str)
def test_explicit_kernel_matches_the_restatement(kind):
    """weight [C(u) T + D(u, T)] of nsfem_scalar_explicit and the cell means of kappa_x against the restatement fed the
    device's vertex constants, both forms, weights 1 and -1.5, 1e-13 of the largest entry.  The restatement alone: at
    least half the cells have c_K > 0 and max |D| >= 0.25 max |C T|.  Second calls return the same bytes, no slot is
    written, one procedure run per element launch"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    fields, grouping, alpha, cmax = _KERNEL_CASES[kind]
    u, T = fields(dm.p2_coords)
    orc = DynamicScalarRestatement(rs, (alpha, cmax), _groups(dm, grouping))
    own = orc.constant(u, T)
    ck = orc.cell_constant(own[orc.group])
    D_own, CT = orc.residual(u, T), _convection(s, "standard", u, T)
    ratio = np.abs(D_own).max() / np.abs(CT).max()
    print("kernel %s: restatement ctheta %s, cells with c_K > 0 %.2f, max |D| / max |C T| %.3f" % (
        kind, np.array2string(own, precision=4), (ck > 0.0).mean(), ratio))
    assert (ck > 0.0).mean() >= 0.5 and ratio >= 0.25
    ctx = make(mesh, dm)
    try:
        ctx.set_state(nat.U1, u)
        ctx.set_state(nat.T1, T)
        _switch_on(ctx, dm, grouping, alpha, cmax)
        cth = ctx.scalar_dynamic_constant(nat.U1, nat.T1)
        assert np.abs(cth - own).max() < 1e-9 * own.max()
        orc.vertex_constants = cth[orc.group]
        D, means = orc.residual(u, T), orc.cell_means(u, T)
        launches = 0
        for form_id, form in _FORMS:
            want = _convection(s, form, u, T) + D
            for weight in (1.0, -1.5):
                got = ctx.scalar_explicit(nat.U1, nat.T1, form_id, weight)
                err = _max_rel(got, weight * want)
                print("kernel %s form %d weight %g: %.2e of the largest entry" % (kind, form_id, weight, err))
                assert err < 1e-13
                assert got.tobytes() == ctx.scalar_explicit(nat.U1, nat.T1, form_id, weight).tobytes()
                launches += 2
            plain = ctx.scalar_convection(nat.U1, nat.T1, form_id, 1.0)         # (C T alone keeps its meaning)
            assert _max_rel(plain, _convection(s, form, u, T)) < 1e-13
        cells = ctx.scalar_diffusivity_cells(nat.U1, nat.T1)
        cerr = _max_rel(cells, means)
        print("kernel %s: cell means of kappa_x %.2e, up to %.3e" % (kind, cerr, cells.max()))
        assert means.max() > 1e-6 and cerr < 1e-13
        assert cells.tobytes() == ctx.scalar_diffusivity_cells(nat.U1, nat.T1).tobytes()
        assert np.array_equal(ctx.get_state(nat.U1), u) and np.array_equal(ctx.get_state(nat.T1), T)
        assert not ctx.get_state(nat.TCONV_1).any() and not ctx.get_state(nat.TCONV_2).any()
        info = ctx.scalar_dynamic_info()
        assert info["runs"] == launches + 3 and info["launches"] == 3 * (launches + 3), info
        assert ctx.scalar_sgs_info()["launches"] == launches and ctx.dynamic_info()["runs"] == 0
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", [(4, 4), KUHN], ids=str)
def test_fused_kernel_with_a_heated_body_matches_the_restatement(kind):
    """the PENAL = 1 (sharp) and PENAL = 2 (smoothed mask) instantiations of the SGS = 8 element kernel: with the heated
    disc / ball of tests/test_gpu_heated_bodies.py the one launch forms C T + D + H, both forms, against the
    restatements fed the device's vertex constants -- the tolerances of that file (1e-13 sharp; its smoothed-mask
    figure, which the distance function sets, not the subgrid term)"""
    from test_gpu_heated_bodies import _ETA, _ETA_T, _TOL
    from test_gpu_heated_bodies import EPS as SMOOTHING
    from test_heated_bodies_host import ScalarPenalRestatement, heated_set
    mesh, dm, marks, s, rs, make = _mesh(kind)
    fields, grouping, alpha, cmax = _KERNEL_CASES[kind]
    u, T = fields(dm.p2_coords)
    orc = DynamicScalarRestatement(rs, (alpha, cmax), _groups(dm, grouping))
    ctx = make(mesh, dm)
    try:
        ctx.set_state(nat.U1, u)
        ctx.set_state(nat.T1, T)
        _switch_on(ctx, dm, grouping, alpha, cmax)
        orc.vertex_constants = ctx.scalar_dynamic_constant(nat.U1, nat.T1)[orc.group]
        D = orc.residual(u, T)
        without = {form_id: ctx.scalar_explicit(nat.U1, nat.T1, form_id, 1.0) for form_id, _ in _FORMS}
        for eps in (0.0, SMOOTHING):
            bodies = heated_set(dm.dim, "disc", _ETA, eps, _ETA_T)
            H = ScalarPenalRestatement(rs, bodies).residual(T)
            ctx.set_bodies(bodies.rows(), bodies.eta, bodies.smoothing)
            ctx.set_body_temperatures(*bodies.temperatures(), bodies.eta_scalar)
            fused = ctx.body_heat_info()["fused_launches"]
            for form_id, form in _FORMS:
                want = _convection(s, form, u, T) + D + H
                assert np.abs(H).max() >= 1e-3 * np.abs(want).max() and np.abs(D).max() >= 1e-3 * np.abs(want).max()
                got = ctx.scalar_explicit(nat.U1, nat.T1, form_id, 1.0)
                err = _max_rel(got, want)
                print("heated %s eps %.2f form %d: %.2e of the largest entry" % (kind, eps, form_id, err))
                assert err < _TOL[eps]
                assert got.tobytes() == ctx.scalar_explicit(nat.U1, nat.T1, form_id, 1.0).tobytes()
                assert got.tobytes() != without[form_id].tobytes()
            assert ctx.body_heat_info()["fused_launches"] == fused + 4
    finally:
        ctx.close()


# ---------------------------------------------------------------- 3. every group clipped: the fixed model
_A3 = np.array([[0.5, -0.75, 0.4], [1.25, 0.375, -0.5], [-2.0 / 3.0, 0.6, -0.875]])


def _clipped(X):
    """2D: a plane strain u = (x / 2, -y / 2) (a linear T needs a compressive strain direction) and T = y, each with
    5 % of ``_sines``; 3D: u = A x, T = z"""
    dim = X.shape[1]
    if dim == 2:
        sn = _sines(X).reshape(-1, 2)
        return (np.stack([0.5 * X[:, 0], -0.5 * X[:, 1]], axis=1) + 0.05 * sn).ravel(), X[:, 1] + 0.05 * sn[:, 0]
    return (X @ _A3.T).ravel(), X[:, 2].copy()


@pytest.mark.parametrize("kind", [(3, 5), (4, 4), KUHN, CUBE], ids=str)
def test_clipped_everywhere_equals_the_fixed_model(kind):
    """``_clipped`` with alpha = 1.1 and ctheta_max = 0.0625: the restatement alone has every group of the global and
    of every plane grouping above the clip, so c_K = 0.0625 in every cell and the dynamic term is, byte for byte, law 1
    with C_s = 0.25 and Pr_t = 1 (0.25^2, the mean of equal numbers and the factor 1 / Pr_t = 1 are all exact)"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    u, T = _clipped(dm.p2_coords)
    cmax = 0.0625
    for grouping in _groupings(kind):
        orc = DynamicScalarRestatement(rs, (1.1, cmax), _groups(dm, grouping))
        sums = orc.sums(u, T)
        q = sums[:, 0] / sums[:, 1]
        print("clipped %s %s: smallest group quotient %.3f" % (kind, grouping, q.min()))
        assert np.all(q > 1.1 * cmax) and np.all(orc.constant(u, T) == cmax), (grouping, sums)
        ctx = make(mesh, dm)
        try:
            ctx.set_state(nat.U1, u)
            ctx.set_state(nat.T1, T)
            _switch_on(ctx, dm, grouping, 1.1, cmax)
            assert np.all(ctx.scalar_dynamic_constant(nat.U1, nat.T1) == cmax)
            dynamic = [ctx.scalar_explicit(nat.U1, nat.T1, form_id, 1.0) for form_id, _ in _FORMS]
            cells8 = ctx.scalar_diffusivity_cells(nat.U1, nat.T1)
            ctx.set_scalar_sgs_dynamic(False)
            ctx.set_viscosity_law(SMAGORINSKY, (0.25, ))
            ctx.set_scalar_sgs(1.0)
            fixed = [ctx.scalar_explicit(nat.U1, nat.T1, form_id, 1.0) for form_id, _ in _FORMS]
            cells1 = ctx.viscosity_cells(nat.U1)
            plain = ctx.scalar_convection(nat.U1, nat.T1, 0, 1.0)
            assert np.abs(fixed[0] - plain).max() > 1e-3 * np.abs(plain).max()      # (the term is there)
            for a, b in zip(dynamic, fixed):
                assert a.tobytes() == b.tobytes()
            assert _max_rel(cells8, cells1) < 1e-13
        finally:
            ctx.close()


# ---------------------------------------------------------------- 4. degenerate states
@pytest.mark.parametrize("kind", [(4, 4), KUHN], ids=str)
def test_rest_and_constant_fields_give_exact_zeros(kind):
    """rest, u = const (gamma = 0 exactly) and T = const (grad T = 0 exactly): PR, RR, the sums and the constants are
    0.0, D = 0 -- the explicit vector keeps the bytes of C T alone -- and the cell means of kappa_x are 0.0"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    dim = dm.dim
    u, T = smooth_fields(dm.p2_coords)
    uc = np.tile([0.3, -1.7, 0.9][:dim], dm.n_p2)
    ctx = make(mesh, dm)
    try:
        _switch_on(ctx, dm, ("planes", 1), 2.0, 0.2)
        for uu, TT in ((np.zeros_like(u), T), (uc, T), (u, np.full(dm.n_p2, 0.7)), (np.zeros_like(u), np.zeros_like(T))):
            ctx.set_state(nat.U1, uu)
            ctx.set_state(nat.T1, TT)
            cth, sums, vert = ctx.scalar_dynamic_constant(nat.U1, nat.T1, details=True)
            assert np.all(np.isfinite(vert)) and np.all(vert[:, 0] > 0.0)
            assert np.all(vert[:, 1:] == 0.0) and np.all(sums == 0.0) and np.all(cth == 0.0)
            for form_id, _ in _FORMS:
                both = ctx.scalar_explicit(nat.U1, nat.T1, form_id, 1.0)
                assert both.tobytes() == ctx.scalar_convection(nat.U1, nat.T1, form_id, 1.0).tobytes()
            assert np.all(ctx.scalar_diffusivity_cells(nat.U1, nat.T1) == 0.0)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 5. steps against the restatement
# case of tests/test_gpu_dynamic_model.py (mesh, grouping, flow with law 8): (ctheta_max, kappa).  3D: T0 = y is the
# conductive state of its own trace, and with kappa = 2 the constant stays inside the window while the flow bends T
# (0.32, 0.46, 0.58, 0.58 of the clip on the CPU); with kappa = 0.05 it triples within two steps
_STEP_CASES = {"box8-global": (0.05, 0.05), "box16-planes": (0.05, 0.05), "kuhn4-global": (0.03, 2.0),
               "pchan3-planes": (0.03, 0.5)}
_STEP_HOST = {}
_PERIODIC_STEPS = {"pchan3-planes": 1.0}
_STEP_CASES_KIND = {"pchan3-planes": "pchan3"}


def _scalar_setup(name):
    mesh, dm, s, rs, make, grouping, cs2_max, k, vbc, f, u0 = _step_setup(name)
    X = dm.p2_coords
    T0 = _t5(X) if dm.dim == 2 else X[:, 1].copy()
    if name in _PERIODIC_STEPS:
        # between the walls the conductive profile, bent by the periodic scalar of tests/periodic_meshes.py
        T0 = T0 + _PERIODIC_STEPS[name] * _periodic(X, _STEP_CASES_KIND[name])[1]
    nodes = np.unique(np.asarray(vbc[0]) // dm.dim).astype(np.int32)         # (every boundary node: the trace of T0)
    return T0, (nodes, T0[nodes])


def _scalar_host_steps(name):
    """the scalar restatement with its own constants on the velocities of the law-8 flow restatement
    (``_host_steps`` of tests/test_gpu_dynamic_model.py; the scalar is passive), and beside it the one without the term.
    Host only; computed once"""
    if name not in _STEP_HOST:
        mesh, dm, s, rs, make, grouping, cs2_max, k, vbc, f, u0 = _step_setup(name)
        cmax, kappa = _STEP_CASES[name]
        flow = _host_steps(name)
        T0, tbc = _scalar_setup(name)
        sgs = DynamicScalarRestatement(rs, (2.0, cmax), _groups(dm, grouping))
        runs = []
        for term in (sgs, None):
            orc = DynamicScalarIMEXRestatement(s, kappa, "standard", term)
            orc.T[0], orc.T[1], orc.T[2] = T0.copy(), T0.copy(), T0.copy()
            runs.append(orc)
        levels = [u0, u0] + [h["u"] for h in flow]
        out = []
        for i, h in enumerate(flow):
            alpha, beta, gamma, kk = h["coef"]
            u1, u2 = levels[i + 1], levels[i]
            ctheta = sgs.constant(u1, runs[0].T[1])
            kx = float(sgs.cell_means(u1, runs[0].T[1]).max())
            for orc in runs:
                orc.step(alpha, beta, gamma, kk, u1, u2, tbc)
            out.append(dict(ctheta=ctheta, kappa_x=kx, effect=rel(runs[0].T[0], runs[1].T[0]), T=runs[0].T[0].copy()))
            for orc in runs:
                orc.advance()
        assert len(runs[0].constants) == len(flow)                 # (one evaluation per step: N2 is the stored N1)
        _STEP_HOST[name] = out
    return _STEP_HOST[name]


@pytest.mark.parametrize("name", list(_STEP_CASES))
def test_scalar_steps_match_the_restatement(name):
    """4 SBDF2 transport steps with the law-8 flow step alongside: T 1e-9 against the restatement with its own
    constants (u*, u as in tests/test_gpu_dynamic_model.py).  The restatement alone: at every step a group lies inside
    (0.2, 0.8) ctheta_max, the term moves T by at least 1e-5 relative and the largest cell mean of kappa_x stays below
    kappa / 3.  One procedure run and one element launch per step, nothing recomputed"""
    mesh, dm, s, rs, make, grouping, cs2_max, k, vbc, f, u0 = _step_setup(name)
    cmax, kappa = _STEP_CASES[name]
    flow, host = _host_steps(name), _scalar_host_steps(name)
    T0, tbc = _scalar_setup(name)
    for i, h in enumerate(host):
        inside = (h["ctheta"] > 0.2 * cmax) & (h["ctheta"] < 0.8 * cmax)
        print("%s step %d: ctheta / ctheta_max %s, effect on T %.2e, kappa_x / kappa %.3f" % (
            name, i, np.array2string(h["ctheta"] / cmax, precision=3), h["effect"], h["kappa_x"] / kappa))
        assert inside.any(), (name, i, h["ctheta"])
        assert h["effect"] >= 1e-5 and h["kappa_x"] < kappa / 3.0, (name, i, h["effect"], h["kappa_x"])
    ctx = make(mesh, dm)
    try:
        ctx.set_coeffs(1.0, 1.0, 0.01, 1.0)
        ctx.set_dirichlet(nat.VELOCITY, *vbc)
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        ctx.set_dirichlet(nat.SCALAR, *tbc)
        ctx.set_state(nat.BODY_FORCE, f)
        ctx.set_scalar(kappa, None, 0)
        _switch_on(ctx, dm, grouping, 2.0, cmax, cs2_max)
        ctx.set_state(nat.U1, u0)
        ctx.set_state(nat.U2, u0)
        ctx.set_state(nat.T0, T0)
        ctx.set_state(nat.T1, T0)
        opts = _opts(ctx)
        worst = 0.0
        for i, (hf, hs) in enumerate(zip(flow, host)):
            ctx.set_imex(*hf["coef"])
            si = ctx.step_scalar_imex(rtol=1e-13)
            et = rel(ctx.get_state(nat.T0), hs["T"])
            ctx.step_imex(opts)
            es, eu = rel(ctx.get_state(nat.USTAR), hf["ustar"]), rel(ctx.get_state(nat.U0), hf["u"])
            print("%s step %d: T %.2e u* %.2e u %.2e cg %d" % (name, i, et, es, eu, si.iterations))
            assert si.converged and et < 1e-9, (name, i, et)
            assert es < 1e-9 and eu < 1e-9, (name, i, es, eu)
            worst = max(worst, et)
            ctx.advance(0)
        print("%s: largest error of T %.2e" % (name, worst))
        # (the first SBDF2 step is of first order and reads no stored vector; from the second on it is the stored one)
        info = ctx.scalar_info()
        assert info["convection_launches"] == 4 and info["convection_reuses"] == 3, info
        assert ctx.scalar_sgs_info() == dict(active=False, launches=4, recomputed=0)
        dinfo = ctx.scalar_dynamic_info()
        assert dinfo["runs"] == 4 and dinfo["launches"] == 12, dinfo
        assert ctx.dynamic_info()["runs"] == 4                      # (the flow's own procedure: one run per step)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 6. the stored vector
class _Transport:
    """transport steps alone on box(8, 8), SBDF2, ``_les`` at every velocity level, ``_t5`` with its trace as Dirichlet
    data; law 8 is set, the restatement steps beside the device"""

    def __init__(self, with_orc=True):
        self.mesh, self.dm, s, self.rs, make, grouping, cs2_max, k, vbc, f, self.u = _step_setup("box8-global")
        self.T_init, self.tbc = _scalar_setup("box8-global")
        self.kappa = 0.05
        self.orc = None
        if with_orc:
            self.orc = DynamicScalarIMEXRestatement(s, self.kappa, "standard", None)
            self.orc.T[0], self.orc.T[1] = self.T_init.copy(), self.T_init.copy()
        self.ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=1.0 / 128.0)
        self.ctx = ctx = make(self.mesh, self.dm)
        try:
            ctx.set_dirichlet(nat.SCALAR, *self.tbc)
            ctx.set_scalar(self.kappa, None, 0)
            ctx.set_viscosity_law(DYNAMIC, (2.0, 0.09))
            for slot in (nat.T0, nat.T1):
                ctx.set_state(slot, self.T_init)
            for slot in (nat.U0, nat.U1, nat.U2):
                ctx.set_state(slot, self.u)
        except BaseException:
            ctx.close()
            raise

    def model(self, params, groups):
        """the restatement's term from now on (None: off); its stored vector is dropped"""
        self.orc.sgs = DynamicScalarRestatement(self.rs, params, groups) if params is not None else None
        self.orc.N2 = None

    def step(self, tag=""):
        ts = self.ts
        ts.update_coefficients()
        kk = ts.get_next_step_size()
        self.ctx.set_imex(ts.alpha, ts.beta, ts.gamma, kk)
        assert self.ctx.step_scalar_imex(rtol=1e-13).converged
        if self.orc is not None:
            self.orc.step(ts.alpha, ts.beta, ts.gamma, kk, self.u, self.u, self.tbc)
            et = rel(self.ctx.get_state(nat.T0), self.orc.T[0])
            print("stored vector, %s step %d: T %.2e" % (tag, ts.step_number, et))
            assert et < 1e-9, (tag, et)
            self.orc.advance()
        self.ctx.advance(0)
        ts.advance_time()


def test_stored_vector_follows_switch_clip_groups_and_alpha_and_off_returns_to_the_plain_bytes():
    """switch on -> another ctheta_max -> other groups -> another alpha -> off, two steps after each: NSFEM_TCONV_2 is
    formed again exactly at the changes -- never because the constant moved, which it does at every step -- and every
    step matches the restatement.  After switching off the bytes are those of a context that never called the setter"""
    run, plain = _Transport(), _Transport(with_orc=False)
    ctx = run.ctx
    try:
        planes = _groups(run.dm, ("planes", 1))
        run.step("off")
        run.step("off")
        assert ctx.scalar_info()["convection_reuses"] == 1 and ctx.scalar_dynamic_info()["runs"] == 0
        launches, recomputed, reuses, runs = 0, 0, 1, 0
        constants = []
        sequence = (("on 0.05", lambda: ctx.set_scalar_sgs_dynamic(True, 0.05), (2.0, 0.05), None),
                    ("clip 0.03", lambda: ctx.set_scalar_sgs_dynamic(True, 0.03), (2.0, 0.03), None),
                    ("planes", lambda: ctx.set_dynamic_groups(*planes), (2.0, 0.03), planes),
                    ("alpha 1.5", lambda: (ctx.set_viscosity_law(DYNAMIC, (1.5, 0.09)), ctx.set_dynamic_groups(*planes)),
                     (1.5, 0.03), planes))
        for tag, change, params, groups in sequence:
            change()
            run.model(params, groups)
            for again in (False, True):
                if again and not tag.startswith("alpha"):
                    change()         # (the same setting again changes nothing; setting the law again resets the groups)
                constants.append(ctx.scalar_dynamic_constant(nat.U1, nat.T1).tobytes())
                runs += 1
                run.step(tag)
                launches += 1 if again else 2
                recomputed += 0 if again else 1
                reuses += 1 if again else 0
                runs += 1 if again else 2
                assert ctx.scalar_sgs_info() == dict(active=False, launches=launches, recomputed=recomputed), tag
                assert ctx.scalar_info()["convection_reuses"] == reuses, tag
                assert ctx.scalar_dynamic_info()["runs"] == runs, tag
        for a, b in zip(constants[0::2], constants[1::2]):
            assert a != b                                              # the constant moved, nothing was recomputed
        ctx.set_scalar_sgs_dynamic(False)
        run.model(None, None)
        run.step("off again")
        assert ctx.scalar_sgs_info() == dict(active=False, launches=launches, recomputed=recomputed + 1)
        assert ctx.scalar_dynamic_info() == dict(active=False, runs=runs, launches=3 * runs,
                                                 bytes=ctx.scalar_dynamic_info()["bytes"])
        # the levels of the plain context on both: both form their vectors afresh, the bytes agree
        for _ in range(2):
            plain.step()
        levels = {slot: plain.ctx.get_state(slot) for slot in (nat.T0, nat.T1, nat.T2)}
        for c in (ctx, plain.ctx):
            for slot, value in levels.items():
                c.set_state(slot, value)
        plain.ts.update_coefficients()
        for c in (ctx, plain.ctx):
            c.set_imex(plain.ts.alpha, plain.ts.beta, plain.ts.gamma, plain.ts.get_next_step_size())
            assert c.step_scalar_imex(rtol=1e-13).converged
        assert plain.ctx.get_state(nat.TCONV_1).any() and plain.ctx.get_state(nat.TCONV_2).any()
        for slot in (nat.T0, nat.TCONV_1, nat.TCONV_2):
            assert ctx.get_state(slot).tobytes() == plain.ctx.get_state(slot).tobytes()
        assert ctx.scalar_dynamic_info()["runs"] == runs
        assert plain.ctx.scalar_dynamic_info() == dict(active=False, runs=0, launches=0, bytes=0)
    finally:
        ctx.close()
        plain.ctx.close()


# ---------------------------------------------------------------- 7. the conductive row of the wall quantities
@pytest.mark.parametrize("name", ["box4x4", "kuhn3x2x2"])
def test_wall_heat_row_carries_the_dynamic_diffusivity(name):
    """every boundary facet, law 8 with the plane groups along x, use_law and the switch on: c_K differs from cell to
    cell (the mean of the device's vertex constants), and the conductive row is int -(kappa + c_K Delta_K^2 gamma)
    grad T . n -- the molecular row plus c_K times the row of a unit constant, both by the reference of
    tests/test_gpu_scalar_sgs.py -- inside the per-entry bound of that file with dim + 4 operations more (the mean over
    the vertices, the product with c_K, the sum of the two parts); every other entry keeps its bytes, and with the
    switch off the row is bitwise the present one"""
    import test_wall_quantities_host as wh
    from test_derived_fields_host import smooth_fields as wall_fields
    from test_gpu_scalar_sgs import _wall_heat_reference
    mesh, dm, marks, s, rs, make = _mesh((4, 4) if name == "box4x4" else KUHN)
    dim = dm.dim
    ids, cells, local = wh.boundary_facets(mesh)
    _, p, T = wall_fields(dm.p2_coords, dm.p1_coords)
    u = _les(dm.p2_coords)
    o = wh.OPTS
    grouping = ("planes", 0)
    orc = DynamicScalarRestatement(rs, (2.0, 0.2), _groups(dm, grouping))
    own = orc.constant(u, T)
    ck_own = orc.cell_constant(own[orc.group])[np.asarray(cells, dtype=np.int64)]
    assert np.unique(np.round(ck_own, 6)).size >= 3 and ck_own.max() > 1e-2, own      # (c_K varies over the facets)
    ctx = make(mesh, dm)
    try:
        ctx.set_scalar(o["kappa"])
        ctx.set_state(nat.T0, T)
        ctx.set_state(nat.U0, u)
        ctx.set_state(nat.P, p)
        ctx.wall_set_facets(cells, local, np.zeros(ids.size, dtype=np.int32), 1)
        _set(ctx, dm, grouping, (2.0, 0.09))

        def compute(use_law=True):
            return ctx.wall_compute(o["nu"], o["sym"], o["kappa"], o["origin"], use_law=use_law, scalar_slot=nat.T0,
                                    facets=True)
        sums_off, rows_off = compute()
        ctx.set_scalar_sgs_dynamic(True, 0.2)
        cth = ctx.scalar_dynamic_constant(nat.U0, nat.T0)
        assert np.abs(cth - own).max() < 1e-9 * own.max()
        runs = ctx.scalar_dynamic_info()["runs"]
        sums_on, rows_on = compute()
        assert ctx.scalar_dynamic_info()["runs"] == runs + 1
        sums_nolaw, rows_nolaw = compute(False)
        assert ctx.scalar_dynamic_info()["runs"] == runs + 1
        ctx.set_scalar_sgs_dynamic(False)
        sums_back, rows_back = compute()
        sums_nolaw_ref, rows_nolaw_ref = compute(False)
    finally:
        ctx.close()
    ck = orc.cell_constant(cth[orc.group])[np.asarray(cells, dtype=np.int64)]
    molecular, mol_abs = _wall_heat_reference(mesh, dm, cells, local, u, T, o["kappa"], 0.0, 1.0)
    unit, unit_abs = _wall_heat_reference(mesh, dm, cells, local, u, T, 0.0, 1.0, 1.0)
    want, scale = molecular + ck * unit, mol_abs + ck * unit_abs
    bound = 2.0 * (wh.n_terms(dim, True) + 2 + dim + 4) * wh.EPS * scale
    heat = 3 + 2 * dim
    err = np.abs(rows_on[:, heat] - want)
    eddy = np.abs(want - molecular).max()
    print("wall heat %s: c_K %.4f .. %.4f, max error %.3e, max error / bound %.3f, eddy part %.3e" % (
        name, ck.min(), ck.max(), err.max(), (err / bound).max(), eddy))
    assert eddy > 1e3 * bound.max()
    assert (err <= bound).all()
    others = [c for c in range(rows_on.shape[1]) if c != heat]
    assert rows_on[:, others].tobytes() == rows_off[:, others].tobytes()
    assert rows_back.tobytes() == rows_off.tobytes() and sums_back.tobytes() == sums_off.tobytes()
    assert rows_nolaw.tobytes() == rows_nolaw_ref.tobytes() and sums_nolaw.tobytes() == sums_nolaw_ref.tobytes()
    assert not np.array_equal(rows_on[:, heat], rows_off[:, heat])


# ---------------------------------------------------------------- 8. refusals
def test_bad_clips_both_switches_other_laws_partitions_and_wrong_slots_are_refused():
    mesh, dm, marks, s, rs, make = _mesh((8, 8))
    u, T = _les(dm.p2_coords), _t5(dm.p2_coords)
    ctx = make(mesh, dm)
    try:
        for bad in (0.0, -0.1, np.nan, np.inf):
            with pytest.raises(nat.NativeError, match="ctheta_max"):
                ctx.set_scalar_sgs_dynamic(True, bad)
        assert ctx.scalar_dynamic_info() == dict(active=False, runs=0, launches=0, bytes=0)
        ctx.set_scalar_sgs_dynamic(False, np.nan)                          # (off reads no clip)
        ctx.set_state(nat.U1, u)
        ctx.set_state(nat.T1, T)
        ctx.set_scalar(0.05, None, 0)
        ctx.set_imex((1.0, -1.0, 0.0), (1.0, 0.0), (1.0, 0.0, 0.0), 1.0 / 16.0)
        # the switch off: the hooks refuse
        ctx.set_viscosity_law(DYNAMIC, (2.0, 0.09))
        with pytest.raises(nat.NativeError, match="switch is off"):
            ctx.scalar_dynamic_constant(nat.U1, nat.T1)
        with pytest.raises(nat.NativeError, match="switch is off"):
            ctx.scalar_diffusivity_cells(nat.U1, nat.T1)
        # both switches at once, in either order
        ctx.set_scalar_sgs(0.85)
        with pytest.raises(nat.NativeError, match="fixed Pr_t"):
            ctx.set_scalar_sgs_dynamic(True, 0.2)
        assert ctx.scalar_dynamic_info()["active"] is False and ctx.scalar_sgs_info()["active"] is True
        # (a fixed Pr_t with law 8 keeps refusing at the step, with its present message)
        with pytest.raises(nat.NativeError, match=r"viscosity law is not 1 \(Smagorinsky\), 4 \(WALE\) or 5 \(Vreman\)"):
            ctx.scalar_explicit(nat.U1, nat.T1, 0, 1.0)
        ctx.set_scalar_sgs(0.0)
        ctx.set_scalar_sgs_dynamic(True, 0.2)
        with pytest.raises(nat.NativeError, match="dynamic diffusivity is on"):
            ctx.set_scalar_sgs(0.85)
        ctx.set_scalar_sgs(0.0)                                            # (off is no conflict)
        assert ctx.scalar_dynamic_info()["active"] is True and ctx.scalar_sgs_info()["active"] is False
        # the law is not 8: step and hooks refuse, state untouched
        before = [ctx.get_state(slot).tobytes() for slot in (nat.T0, nat.T1, nat.TCONV_1, nat.TCONV_2)]
        for law, params in ((0, None), (SMAGORINSKY, (0.2, )), (4, (0.5, ))):
            ctx.set_viscosity_law(law, params)
            with pytest.raises(nat.NativeError, match="viscosity law is not 8"):
                ctx.step_scalar_imex(rtol=1e-13)
            with pytest.raises(nat.NativeError, match="viscosity law is not 8"):
                ctx.scalar_explicit(nat.U1, nat.T1, 0, 1.0)
            with pytest.raises(nat.NativeError, match="viscosity law is not 8"):
                ctx.scalar_dynamic_constant(nat.U1, nat.T1)
            with pytest.raises(nat.NativeError, match="viscosity law is not 8"):
                ctx.scalar_diffusivity_cells(nat.U1, nat.T1)
            assert ctx.scalar_convection(nat.U1, nat.T1, 0, 1.0).any()     # (C T alone needs no law)
        assert before == [ctx.get_state(slot).tobytes() for slot in (nat.T0, nat.T1, nat.TCONV_1, nat.TCONV_2)]
        assert ctx.scalar_dynamic_info() == dict(active=True, runs=0, launches=0, bytes=0)
        assert ctx.scalar_info()["convection_launches"] == 0
        # wrong slots
        ctx.set_viscosity_law(DYNAMIC, (2.0, 0.09))
        for vslot, tslot in ((nat.P, nat.T1), (nat.T1, nat.T1), (nat.U1, nat.U1), (nat.U1, nat.TCONV_1), (nat.U1, nat.P)):
            with pytest.raises(nat.NativeError, match="slot"):
                ctx.scalar_dynamic_constant(vslot, tslot)
            with pytest.raises(nat.NativeError, match="slot"):
                ctx.scalar_diffusivity_cells(vslot, tslot)
        assert ctx.scalar_dynamic_info()["runs"] == 0
        assert ctx.scalar_dynamic_constant(nat.U1, nat.T1).shape == (1, )
    finally:
        ctx.close()
    group = nat.local_group_create(1)
    ctx = make(mesh, dm)
    try:
        ctx.attach_local_comm(group, 0)
        with pytest.raises(nat.NativeError, match="communicator"):
            ctx.set_scalar_sgs_dynamic(True, 0.2)
        with pytest.raises(nat.NativeError, match="communicator"):
            ctx.scalar_dynamic_constant(nat.U1, nat.T1)
        assert ctx.scalar_dynamic_info() == dict(active=False, runs=0, launches=0, bytes=0)
    finally:
        ctx.close()
        nat.local_group_destroy(group)


# ---------------------------------------------------------------- 9. through the classes
_SPEC = dict(name="Cavity", mesh=("cube", 2, 8), scheme="ipcs", clock=dict(dt=0.5 / 8, steps=3),
             numbers=dict(Re=100.0, Fr=1.0), start={"velocity": (0.0, 0.0), "pressure": 0.0, "temperature": 0.5},
             bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_slip", "bottom"), ("velocity", "top", (1.0, 0.0))])
_KAPPA_CLS = 0.05


def test_boussinesq_solver_with_the_dynamic_heat_flux_equals_driving_the_steps_by_hand(monkeypatch):
    """BoussinesqIMEXSolver through InstationaryProblem.solve_problem with DynamicSmagorinskyModel(("planes", 1),
    heat_flux="dynamic") on the 8 x 8 cavity, 3 steps: bit for bit what set_viscosity_law(8) / set_dynamic_groups /
    set_scalar_sgs_dynamic / step_scalar_imex / step_imex / advance give through the C ABI; without the switch the
    scalar differs.  _compute_model_scalar_constant returns the device's C_theta and Pr_t = cs2 / ctheta,
    _compute_model_diffusivity nsfem_scalar_diffusivity_cells; WallQuantities runs the procedure"""
    from fem_function import HostField
    from multigrid import attach_hierarchy
    from ns_boussinesq_solver import BoussinesqIMEXSolver
    from problem_specs import build_problem
    from viscosity_models import SmagorinskyModel
    from wall_quantities import WallQuantities
    steps, dt = _SPEC["clock"]["steps"], _SPEC["clock"]["dt"]
    model = DynamicSmagorinskyModel(("planes", 1), heat_flux="dynamic")
    assert model.ctheta_max == 0.2
    monkeypatch.setenv("NSFEM_NO_OUTPUT", "1")
    problem = build_problem(dict(_SPEC))
    cls = type(problem)

    def set_viscosity_model(self):
        self._viscosity_model = model

    def set_temperature_coefficients(self):
        self._temperature_coefficients = dict(diffusivity=_KAPPA_CLS, buoyancy=(0.0, 1.0), convective_form="standard")

    def set_temperature_boundary_conditions(self):
        self._temperature_bcs = [(self._sides["left"], 1.0), (self._sides["right"], 0.0)]
    cls.set_viscosity_model = set_viscosity_model
    cls.set_temperature_coefficients = set_temperature_coefficients
    cls.set_temperature_boundary_conditions = set_temperature_boundary_conditions
    problem.set_solver_class(BoussinesqIMEXSolver)
    problem.compute_cfl = False
    problem.solve_problem()
    solver = problem._get_solver()
    assert isinstance(solver, BoussinesqIMEXSolver) and problem._time_stepping.step_number == steps
    cctx = solver._ctx
    assert cctx.scalar_sgs_info() == dict(active=False, launches=steps, recomputed=0)
    dinfo = cctx.scalar_dynamic_info()
    assert dinfo["active"] and dinfo["runs"] == steps and dinfo["launches"] == 3 * steps
    T_cls, u_cls = cctx.get_state(nat.T1), cctx.get_state(nat.U1)
    ctheta, prandtl_t = problem._compute_model_scalar_constant()
    want_c, want_s = cctx.scalar_dynamic_constant(nat.U0, nat.T0), cctx.dynamic_constant(nat.U0)
    assert ctheta.shape == (9, ) and np.array_equal(ctheta, want_c) and ctheta.max() > 0.0
    pos = want_c > 0.0
    assert np.array_equal(prandtl_t[pos], want_s[pos] / want_c[pos]) and np.all(np.isinf(prandtl_t[~pos]))
    field = problem._compute_model_diffusivity()
    assert isinstance(field, HostField) and field.center == "Cell" and field.name() == "model diffusivity"
    assert np.array_equal(field.values, cctx.scalar_diffusivity_cells(nat.U0, nat.T0)) and field.values.max() > 1e-6
    runs = cctx.scalar_dynamic_info()["runs"]
    wall = WallQuantities(solver, boundary_ids=(problem._sides["left"], ))
    wall.compute()
    assert cctx.scalar_dynamic_info()["runs"] == runs + 1          # (the conductive row carries kappa_x)
    # ---- the same steps through the C ABI on a fresh context
    dm, mesh = solver._dofmap, solver._mesh
    left = np.unique(dm.facet_p2_nodes(solver._boundary_markers.facets_with_id(problem._sides["left"])))
    right = np.unique(dm.facet_p2_nodes(solver._boundary_markers.facets_with_id(problem._sides["right"])))
    out = {}
    for on in (True, False):
        ctx = nat.NsfemContext(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, dm.n_p2, dm.n_p1)
        try:
            if solver._mg_levels is not None:
                attach_hierarchy(ctx, mesh)
            coef = solver._equation_coefficients
            ctx.set_coeffs(coef["convective_term"], coef["pressure_term"], coef["viscous_term"], coef["body_force_term"])
            bd, bv = solver._dirichlet_bcs["velocity"]
            ctx.set_dirichlet(nat.VELOCITY, np.asarray(bd, np.int32), np.asarray(bv, float))
            ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
            ctx.set_dirichlet(nat.SCALAR, np.concatenate([left, right]),
                              np.concatenate([np.ones(left.size), np.zeros(right.size)]))
            ctx.set_scalar(_KAPPA_CLS, (0.0, 1.0), 0)
            ctx.set_viscosity_law(DYNAMIC, model.params(coef))
            ctx.set_dynamic_groups(*model.vertex_groups(dm.p1_coords))
            if on:
                ctx.set_scalar_sgs_dynamic(True, model.ctheta_max)
            for slot in (nat.T0, nat.T1):
                ctx.set_state(slot, np.full(dm.n_p2, 0.5))
            opts = solver._step_options()
            ts = IMEXTimeStepping(0.0, 1.0, IMEXType.SBDF2, desired_start_time_step=dt)
            for _ in range(steps):
                ts.update_coefficients()
                ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
                ctx.step_scalar_imex(rtol=solver.krylov_rtol, max_iter=solver.krylov_max_iter)
                ctx.step_imex(opts)
                ts.advance_time()
                ctx.advance(0)
            out[on] = (ctx.get_state(nat.T1), ctx.get_state(nat.U1))
        finally:
            ctx.close()
    assert np.abs(u_cls).max() > 0.5 and np.abs(T_cls - 0.5).max() > 1e-2
    assert np.array_equal(T_cls, out[True][0]) and np.array_equal(u_cls, out[True][1])
    assert rel(out[False][0], T_cls) > 1e-6                                  # (without the switch the scalar differs)
    # a model with a fixed Pr_t, or the dynamic model without the heat flux, handed over in the middle of the run
    solver.set_viscosity_model(SmagorinskyModel(0.2, prandtl_t=0.5))
    assert cctx.scalar_dynamic_info()["active"] is False and cctx.scalar_sgs_info()["active"] is True
    solver.set_viscosity_model(model)
    assert cctx.scalar_dynamic_info()["active"] is True and cctx.scalar_sgs_info()["active"] is False
    solver.set_viscosity_model(DynamicSmagorinskyModel(("planes", 1)))
    assert cctx.scalar_dynamic_info()["active"] is False and cctx.scalar_sgs_info()["active"] is False
    with pytest.raises(RuntimeError, match="prandtl_t"):
        problem._compute_model_diffusivity()
