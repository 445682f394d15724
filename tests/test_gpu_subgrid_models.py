"""WALE and Vreman subgrid models on the GPU (laws 4 and 5 of nsfem_set_viscosity_law in k_visc_var_cell /
k3_visc_var_cell, the SGS = 4 / 5 scalar convection kernels, k_wall_facets<DIM, 4 | 5>, WALEModel / VremanModel under
the solver classes) against the numpy restatement of tests/subgrid_models_host.py.

Tolerances.  Kernels (V, cell means, scalar explicit vector): 1e-13 of the largest entry, the project's figure for
element kernels against the oracle and the tolerance of the Smagorinsky kernel.  The figure is flat there (tests/
test_gpu_scalar_sgs.py section 1 states no operation count); the new laws lengthen the chain of a quadrature point by
28 (WALE, 3D) / 22 (Vreman, 3D) rounded operations to about 150, 1.7e-14 at one eps each, below the figure, and both
laws are formed without cancellation (sums of squares), so the figure is kept.  Steps: those of tests/
test_gpu_variable_viscosity.py and tests/test_gpu_scalar_sgs.py (Krylov rtol 1e-13) -- T, u*, u 1e-9, p minus its
mean 1e-8, relative.  Wall rows: the per-entry bound of tests/test_wall_quantities_host.py, 2 n eps times the sums of
the absolute contributions (``_wall_reference``).

Conditions, asserted on the restatement alone so that no test passes by the term being small.  Steps: the largest
nu_x at a quadrature point of every level used stays below c_v = 0.01 while the term changes u* by more than 1e-3
after the steps (C_w = 0.5, the value of the literature, and c = 0.1 = 2.5 * 0.2^2 do both on every mesh used).
Scalar kernel: max |D| >= 0.25 max |C T| at Pr_t = 0.85 -- the constants of ``_C_SCALAR`` are that large for this
reason only.  Coupled steps: kappa_x < kappa / 3 and an effect on T of at least 1e-4."""
import numpy as np
import pytest

import _native as nat
import test_gpu_variable_viscosity as tgv
from gpu_common import cavity_bc, rel
from imex_time_stepping import IMEXTimeStepping, IMEXType
from scalar_sgs_host import ScalarIMEXSgsRestatement
from subgrid_models_host import VREMAN, WALE, SubgridModelRestatement, SubgridScalarSgsRestatement, tensor_nu
from test_gpu_3d import lid_bc
from test_gpu_scalar_transport import _B, _two_sides
from test_gpu_variable_viscosity import (_COEF, GENERAL72, GENERAL384, NO_PBC, _advance, _max_rel, _mesh, _opts, _setup,
                                         _solve, _step, is_general, is_periodic)
from test_heated_bodies_host import ScalarPenalRestatement, heated_set
from test_scalar_transport_host import ScalarIMEXRestatement, smooth_fields
from test_variable_viscosity_host import CARREAU, SMAGORINSKY, IMEXViscRestatement

pytestmark = pytest.mark.gpu

KUHN = ((3, 2, 2), (1.0, 0.8, 0.6))
_KERNEL_MESHES = [(4, 4), (3, 5), (16, 16), "mapped", KUHN, ((4, 4, 4), (1.0, 1.0, 1.0)), GENERAL72, GENERAL384] + \
    list(tgv.PERIODIC)
_KERNEL_LAWS = {WALE: (2.0, ), VREMAN: (1.0, )}
_STEP_LAWS = {WALE: (0.5, ), VREMAN: (0.1, )}
_CV = _COEF["viscous_term"]
# amplitude of the periodic start velocity of the step cases on pchan2 / pchan3 (cells of width 1 / 4 and 1 / 3): with it
# nu_x of both laws stays below c_v, as in the other step cases (asserted)
_PERIODIC_AMP = 0.1


@pytest.fixture(autouse=True)
def _new_restatement(monkeypatch):
    """``_setup`` of tests/test_gpu_variable_viscosity.py builds its restatement through the module's name
    VariableViscosityRestatement; here that name is the subclass that knows laws 4 and 5 (laws 1 and 2 unchanged)"""
    monkeypatch.setattr(tgv, "VariableViscosityRestatement", SubgridModelRestatement)


def _fields(X, which):
    """velocity fields of the degenerate states, interleaved"""
    u = np.zeros_like(X)
    if which == "shear":
        u[:, 0] = 1.3 * X[:, 1]
    elif which == "strain":
        u[:, 0], u[:, 1] = X[:, 0], -X[:, 1]
    elif which == "rotation":
        W = np.array([[0.0, -0.7, 0.4], [0.7, 0.0, -1.1], [-0.4, 1.1, 0.0]])[:X.shape[1], :X.shape[1]]
        u = X @ W.T
    else:
        assert which == "rest"
    return np.ascontiguousarray(u).ravel()


# ---------------------------------------------------------------- 1. the kernels against the restatement
_KERNEL_REF = {}


def _kernel_reference(kind, law):
    if (kind, law) not in _KERNEL_REF:
        mesh, dm, marks, s, rs, make = _mesh(kind)
        u = tgv.velocity_on(kind, dm)
        orc = SubgridModelRestatement(rs, law, _KERNEL_LAWS[law])
        _KERNEL_REF[kind, law] = (u, orc.residual(u), orc.cell_means(u), orc)
    return _KERNEL_REF[kind, law]


@pytest.mark.parametrize("law", (WALE, VREMAN))
@pytest.mark.parametrize("kind", _KERNEL_MESHES, ids=str)
def test_viscosity_kernel_matches_the_restatement(kind, law):
    """weight * V(u) and the cell means of nu_x for the smooth non-polynomial velocity; a second call returns the same
    bytes, a weight of -1.5 rides in the kernel, no slot is written, viscosity_info counts the launches"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    u, want, means, orc = _kernel_reference(kind, law)
    if kind == "mapped" or is_general(kind) or (is_periodic(kind) and kind.endswith("mapped")):
        assert orc.delta.max() > 1.2 * orc.delta.min()
    if is_periodic(kind):
        # the seam is there, and every entry of G takes part
        assert dm.n_p1 < mesh.num_vertices() and np.abs(orc.gradient(u)).max(axis=(0, 1)).min() > 0.1
    if is_general(kind):
        # every entry of G takes part, and through a J^-1 without zeros: a transposed or mis-indexed J^-1 shows
        assert np.abs(orc.gradient(u)).max(axis=(0, 1)).min() > 0.1
        assert np.abs(rs.g1).min() > 1e-7 * np.abs(rs.g1).max()
    ctx = make(mesh, dm)
    try:
        ctx.set_state(nat.U1, u)
        ctx.set_viscosity_law(law, _KERNEL_LAWS[law])
        got = ctx.viscosity_residual(nat.U1, 1.0)
        cells = ctx.viscosity_cells(nat.U1)
        err, cerr = _max_rel(got, want), _max_rel(cells, means)
        print("kernel %s law %d: V %.2e cell means %.2e (of the largest entry)" % (kind, law, err, cerr))
        assert np.abs(want).max() > 1e-4 and np.abs(means).max() > 1e-4
        assert err < 1e-13 and cerr < 1e-13
        assert got.tobytes() == ctx.viscosity_residual(nat.U1, 1.0).tobytes()
        assert cells.tobytes() == ctx.viscosity_cells(nat.U1).tobytes()
        ctx.set_state(nat.USTAR, u)
        assert _max_rel(ctx.viscosity_residual(nat.USTAR, -1.5), -1.5 * want) < 1e-13
        assert not ctx.get_state(nat.CONV_N1).any() and not ctx.get_state(nat.CONV_N2).any()
        assert np.array_equal(ctx.get_state(nat.U1), u) and np.array_equal(ctx.get_state(nat.USTAR), u)
        assert ctx.viscosity_info() == dict(law=law, element_launches=5, recomputed=0)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 2. degenerate states
@pytest.mark.parametrize("law", (WALE, VREMAN))
@pytest.mark.parametrize("kind", [(4, 4), KUHN], ids=str)
def test_degenerate_states(kind, law):
    """rest: V and the cell means are exactly 0.0 and finite (the 0 / 0 guards: a run started from rest meets this
    state).  Linear shear u = (1.3 y, 0 (, 0)): the cell means are below 1e-20 of those of Smagorinsky, C_s = 0.17, on
    the same state (the restatement gives <= 5e-46 for WALE and 0 for Vreman), which are not zero.  Rigid rotation:
    max |V| below 1e-12 of max |V| of the pure strain u = (x, -y (, 0)), although nu_x itself is not zero there"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    X = dm.p2_coords
    params = _KERNEL_LAWS[law]
    ctx = make(mesh, dm)
    try:
        ctx.set_viscosity_law(law, params)
        ctx.set_state(nat.U1, _fields(X, "rest"))
        V, cells = ctx.viscosity_residual(nat.U1, 1.0), ctx.viscosity_cells(nat.U1)
        assert np.all(np.isfinite(V)) and np.all(np.isfinite(cells))
        assert np.all(V == 0.0) and np.all(cells == 0.0)
        ctx.set_state(nat.U1, _fields(X, "shear"))
        cells = ctx.viscosity_cells(nat.U1)
        ctx.set_viscosity_law(SMAGORINSKY, (0.17, ))
        smag = ctx.viscosity_cells(nat.U1)
        ctx.set_viscosity_law(law, params)
        print("shear %s law %d: largest cell mean %.2e, Smagorinsky %.2e .. %.2e" % (kind, law, cells.max(), smag.min(),
                                                                                    smag.max()))
        assert np.all(smag > 1e-5) and np.all(cells >= 0.0) and np.all(cells <= 1e-20 * smag)
        ctx.set_state(nat.U1, _fields(X, "rotation"))
        rigid, nu_rot = np.abs(ctx.viscosity_residual(nat.U1, 1.0)).max(), ctx.viscosity_cells(nat.U1)
        ctx.set_state(nat.U1, _fields(X, "strain"))
        strain = np.abs(ctx.viscosity_residual(nat.U1, 1.0)).max()
        print("rotation %s law %d: |V| %.2e of strain %.2e, nu_x in rotation %.2e" % (kind, law, rigid, strain,
                                                                                     nu_rot.min()))
        assert strain > 1e-5 and nu_rot.min() > 1e-5 and rigid < 1e-12 * strain
    finally:
        ctx.close()


# ---------------------------------------------------------------- 3. steps against the restatement
def _steps(kind, typ, law, steps=4):
    """`steps` steps of the device beside the restatement (``_setup`` / ``_solve`` of the Smagorinsky tests), and beside
    them, host only, the restatement WITHOUT the term: returns the largest nu_x met at a quadrature point of a level the
    steps read, the effect of the term on the last u*, and the counters"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    params = _STEP_LAWS[law]
    ctx = make(mesh, dm)
    try:
        orc, vbc = _setup(ctx, dm, marks, s, rs, law, params, general=is_general(kind),
                          periodic=kind if is_periodic(kind) else None, amp=_PERIODIC_AMP)
        assert isinstance(orc.visc, SubgridModelRestatement) and orc.visc.law == law
        plain = IMEXViscRestatement(s, _COEF, "standard", visc=None)
        plain.body_force = orc.body_force
        plain.vel[1], plain.vel[2] = orc.vel[1].copy(), orc.vel[2].copy()
        n = 16 if is_periodic(kind) else kind[0] if isinstance(kind[0], int) else (8 if kind == "mapped" else kind[0][0])
        ts = IMEXTimeStepping(0.0, 1.0e9, typ, desired_start_time_step=0.5 / n)
        opts = _opts(ctx)
        nu_max = 0.0
        for _ in range(steps):
            ts.update_coefficients()
            for level in (1, 2) if ts.beta[1] != 0.0 else (1, ):
                nu_max = max(nu_max, orc.visc.nu_max(orc.vel[level]))
            plain.step(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size(), vbc, NO_PBC)
            _solve(ctx, orc, ts, vbc, opts, "%s %s law %d" % (kind, typ.name, law))
            effect = rel(orc.ustar, plain.ustar)
            plain.advance()
            _advance(ctx, orc, ts)
        print("%s %s law %d: max nu_x %.3e = %.2f c_v, effect on u* %.2e" % (kind, typ.name, law, nu_max, nu_max / _CV,
                                                                           effect))
        assert 0.0 < nu_max < _CV and effect > 1e-3
        return ctx.imex_info(), ctx.viscosity_info()
    finally:
        ctx.close()


@pytest.mark.parametrize("kind,typ,law,path", [
    ((8, 8), IMEXType.SBDF2, WALE, "generic"), ((8, 8), IMEXType.SBDF2, VREMAN, "generic"),
    ((8, 8), IMEXType.CNAB, WALE, "generic"), ((16, 16), IMEXType.SBDF2, WALE, "lattice-kernel"),
    ("mapped", IMEXType.SBDF2, VREMAN, "generic"), (KUHN, IMEXType.SBDF2, WALE, "generic"),
    (KUHN, IMEXType.SBDF2, VREMAN, "generic"), (GENERAL72, IMEXType.SBDF2, WALE, "generic"),
    (GENERAL72, IMEXType.SBDF2, VREMAN, "generic"),
    ("pchan2", IMEXType.SBDF2, WALE, "generic"), ("pchan2", IMEXType.SBDF2, VREMAN, "generic"),
    ("pchan3", IMEXType.SBDF2, WALE, "generic"), ("pchan3", IMEXType.SBDF2, VREMAN, "generic")], ids=str)
def test_steps_match_the_restatement(kind, typ, law, path):
    """lid-driven cavity from rest, 4 steps: box(8, 8) on the generic right-hand side for both laws and CNAB for WALE,
    box(16, 16) on the one-launch lattice right-hand side, the mapped box (varying Delta_K), the (3, 2, 2) Kuhn box and the
    72 general tetrahedra (3D kernels inside the steps); the periodic channels of tests/periodic_meshes.py, no-slip on
    their walls, from a periodic velocity at both old levels under a periodic body force.  One element launch per step, the stored vector is never recomputed"""
    info, vinfo = _steps(kind, typ, law)
    assert info["path"] == path, info
    if path == "lattice-kernel":
        assert info["lattice_rhs"] == 4 and info["generic_rhs"] == 0, info
    else:
        assert info["generic_rhs"] == 4, info
    assert vinfo == dict(law=law, element_launches=4, recomputed=0), vinfo


# ---------------------------------------------------------------- 4. the stored vector
def test_stored_vector_follows_the_law_and_law_zero_returns_to_the_plain_bytes():
    """SBDF2 on box(8, 8): law 1, then 4, then 4 with the same and with another constant, then 5 -- N(u2) is formed
    again exactly when the law or its constant changed, and the step matches the restatement every time.  Law 0
    afterwards: from the levels of a context that never set a law, the step stores the bytes that context stores, and
    launches no element kernel"""
    mesh, dm, marks, s, rs, make = _mesh((8, 8))
    ctx, plain = make(mesh, dm), make(mesh, dm)
    try:
        orc, vbc = _setup(ctx, dm, marks, s, rs, SMAGORINSKY, (0.2, ))
        _setup(plain, dm, marks, s, rs, None, None)
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=1.0 / 16.0)
        opts = _opts(ctx)
        for _ in range(2):
            _step(ctx, orc, ts, vbc, opts, "law 1")
        assert ctx.viscosity_info() == dict(law=1, element_launches=2, recomputed=0)
        sequence = ((WALE, (0.5, ), 1), (WALE, (0.5, ), 1), (WALE, (0.4, ), 2), (VREMAN, (0.1, ), 3), (VREMAN, (0.1, ), 3))
        launches, before = 2, 0
        for law, params, recomputed in sequence:
            ctx.set_viscosity_law(law, params)
            if recomputed != before:
                orc.visc, orc.N2 = SubgridModelRestatement(rs, law, params), None
            _step(ctx, orc, ts, vbc, opts, "law %d %s" % (law, params))
            launches += 1 + (recomputed - before)
            before = recomputed
            assert ctx.viscosity_info() == dict(law=law, element_launches=launches, recomputed=recomputed)
        # law 0: the levels of the plain context on both, both form N(u2) afresh
        ts_plain = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=1.0 / 16.0)
        popts = _opts(plain)
        for _ in range(2):
            ts_plain.update_coefficients()
            plain.set_imex(ts_plain.alpha, ts_plain.beta, ts_plain.gamma, ts_plain.get_next_step_size())
            plain.step_imex(popts)
            plain.advance(0)
            ts_plain.advance_time()
        ctx.set_viscosity_law(0)
        levels = {slot: plain.get_state(slot) for slot in (nat.U0, nat.U1, nat.U2, nat.USTAR, nat.P, nat.P_OLD)}
        for c in (ctx, plain):
            for slot, value in levels.items():
                c.set_state(slot, value)
        ts_plain.update_coefficients()
        for c, o in ((ctx, opts), (plain, popts)):
            c.set_imex(ts_plain.alpha, ts_plain.beta, ts_plain.gamma, ts_plain.get_next_step_size())
            c.step_imex(o)
        assert plain.get_state(nat.CONV_N1).any() and plain.get_state(nat.CONV_N2).any()     # (nothing trivial compared)
        for slot in (nat.CONV_N1, nat.CONV_N2):
            assert ctx.get_state(slot).tobytes() == plain.get_state(slot).tobytes()
        assert ctx.viscosity_info()["law"] == 0 and ctx.viscosity_info()["element_launches"] == launches
        assert plain.viscosity_info() == dict(law=0, element_launches=0, recomputed=0)
    finally:
        ctx.close()
        plain.close()


# ---------------------------------------------------------------- 5. refusals
def test_bad_constants_unknown_laws_partitions_and_the_other_schemes_are_refused():
    mesh, dm, marks, s, rs, make = _mesh((8, 8))
    ctx = make(mesh, dm)
    try:
        for law, word in ((WALE, "C_w"), (VREMAN, "Vreman: c ")):
            for bad in (-0.1, np.nan, np.inf, -np.inf):
                with pytest.raises(nat.NativeError, match=word):
                    ctx.set_viscosity_law(law, (bad, ))
        with pytest.raises(nat.NativeError, match="WALE"):
            ctx.set_viscosity_law(WALE, (-1.0, ))
        for law in (3, 6):
            with pytest.raises(nat.NativeError, match="unknown law"):
                ctx.set_viscosity_law(law, (0.1, ))
        assert ctx.viscosity_info() == dict(law=0, element_launches=0, recomputed=0)
        ctx.set_viscosity_law(WALE, (0.0, ))                          # zero constants are allowed
        ctx.set_viscosity_law(VREMAN, (0.0, ))
        ctx.set_coeffs(1.0, 1.0, 0.01)
        ctx.set_dirichlet(nat.VELOCITY, *cavity_bc(dm, marks))
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        ctx.set_bdf((1.0, -1.0, 0.0), 1.0 / 16.0)
        ctx.set_viscosity_law(WALE, (0.5, ))
        with pytest.raises(nat.NativeError, match="variable viscosity"):
            ctx.step_ipcs()
        with pytest.raises(nat.NativeError, match="variable viscosity"):
            ctx.step_bdf()
        ctx.set_viscosity_law(0)
        assert ctx.step_ipcs().converged
    finally:
        ctx.close()
    group = nat.local_group_create(1)
    ctx = make(mesh, dm)
    try:
        ctx.attach_local_comm(group, 0)
        for law, params in ((WALE, (0.5, )), (VREMAN, (0.1, ))):
            with pytest.raises(nat.NativeError, match="communicator"):
                ctx.set_viscosity_law(law, params)
        assert ctx.viscosity_info()["law"] == 0
    finally:
        ctx.close()
        nat.local_group_destroy(group)


# ---------------------------------------------------------------- 6. the subgrid heat flux
_PRT = 0.85
_EPS = 0.07
# constants of the scalar kernel cases, by (law, form): large enough for max |D| >= 0.25 max |C T| at Pr_t = 0.85 on every
# mesh below (the skew form's C T is larger against D, and D falls with the cell size: box(16, 16) decides)
_C_SCALAR = {(WALE, 0): 2.5, (WALE, 1): 11.0, (VREMAN, 0): 6.0, (VREMAN, 1): 56.0}
FORMS = ((0, "standard"), (1, "skew_symmetric"))
_SCALAR_REF = {}


def _scalar_reference(kind, law, form_id):
    key = (kind, law, form_id)
    if key not in _SCALAR_REF:
        mesh, dm, marks, s, rs, make = _mesh(kind)
        u, T = smooth_fields(dm.p2_coords)
        conv = ScalarIMEXRestatement(s, 0.0, FORMS[form_id][1]).convection_matrix(u) @ T
        D = SubgridScalarSgsRestatement(rs, law, (_C_SCALAR[law, form_id], ), _PRT).residual(u, T)
        _SCALAR_REF[key] = (u, T, conv, D)
    return _SCALAR_REF[key]


@pytest.mark.parametrize("form_id", (0, 1))
@pytest.mark.parametrize("law", (WALE, VREMAN))
@pytest.mark.parametrize("kind,body_eps", [((4, 4), None), ((16, 16), None), (KUHN, None), ((8, 8), 0.0), ((4, 4), _EPS),
                                           (KUHN, 0.0), (KUHN, _EPS)], ids=str)
def test_scalar_explicit_kernel_matches_the_restatement(kind, body_eps, law, form_id):
    """weight [C(u) T + D(u, T) (+ H(T))] with kappa_x = nu_x / 0.85 of laws 4 and 5, both forms; body_eps 0.0: with the
    thermal ball of tests/test_heated_bodies_host.py and sharp masks (PENAL = 1), 0.07: smoothed masks (PENAL = 2) -- the
    combined instantiations of both dimensions.  A law alone leaves the bytes of scalar_convection; second call, weight
    -1.5 on other slots, no stored state touched, scalar_sgs_info counts the launches"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    u, T, conv, D = _scalar_reference(kind, law, form_id)
    ratio = np.abs(D).max() / np.abs(conv).max()
    assert ratio >= 0.25, ratio
    want = conv + D
    bodies = None
    if body_eps is not None:
        bodies = heated_set(dm.dim, "disc", 0.037, body_eps, 0.021)
        H = ScalarPenalRestatement(rs, bodies).residual(T)
        assert np.abs(H).max() > 1e-3 * np.abs(want).max()
        want = want + H
    ctx = make(mesh, dm)
    try:
        ctx.set_state(nat.U1, u)
        ctx.set_state(nat.T1, T)
        plain = ctx.scalar_convection(nat.U1, nat.T1, form_id, 1.0)
        ctx.set_viscosity_law(law, (_C_SCALAR[law, form_id], ))
        assert ctx.scalar_explicit(nat.U1, nat.T1, form_id, 1.0).tobytes() == plain.tobytes()      # a law alone: off
        assert ctx.scalar_sgs_info() == dict(active=False, launches=0, recomputed=0)
        if bodies is not None:
            ctx.set_bodies(bodies.rows(), bodies.eta, bodies.smoothing)
            ctx.set_body_temperatures(*bodies.temperatures(), bodies.eta_scalar)
        ctx.set_scalar_sgs(_PRT)
        got = ctx.scalar_explicit(nat.U1, nat.T1, form_id, 1.0)
        err = _max_rel(got, want)
        print("scalar kernel %s bodies %s law %d form %d: max |D| / max |C T| %.3g, error %.2e of the largest entry" % (
            kind, body_eps, law, form_id, ratio, err))
        assert err < 1e-13
        assert got.tobytes() == ctx.scalar_explicit(nat.U1, nat.T1, form_id, 1.0).tobytes()
        assert ctx.scalar_convection(nat.U1, nat.T1, form_id, 1.0).tobytes() == plain.tobytes()
        ctx.set_state(nat.U2, u)
        ctx.set_state(nat.T2, T)
        assert _max_rel(ctx.scalar_explicit(nat.U2, nat.T2, form_id, -1.5), -1.5 * want) < 1e-13
        assert not ctx.get_state(nat.TCONV_1).any() and not ctx.get_state(nat.TCONV_2).any()
        assert np.array_equal(ctx.get_state(nat.T1), T) and np.array_equal(ctx.get_state(nat.U1), u)
        assert ctx.scalar_sgs_info() == dict(active=True, launches=3, recomputed=0)
    finally:
        ctx.close()


def test_prandtl_number_without_a_subgrid_law_is_still_refused():
    """Pr_t set with law 0 or Carreau: the step and the hook refuse with the words the Smagorinsky tests match, now
    naming the three subgrid laws; with law 4 or 5 they run"""
    mesh, dm, marks, s, rs, make = _mesh((4, 4))
    u, T = smooth_fields(dm.p2_coords)
    ctx = make(mesh, dm)
    try:
        ctx.set_dirichlet(nat.SCALAR, *_two_sides(dm, marks, dm.p2_coords))
        ctx.set_scalar(0.05, None, 0)
        ctx.set_scalar_sgs(_PRT)
        for slot in (nat.U0, nat.U1, nat.U2):
            ctx.set_state(slot, u)
        for slot in (nat.T0, nat.T1):
            ctx.set_state(slot, T)
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=1.0 / 16.0)
        ts.update_coefficients()
        ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
        for law, params in ((0, None), (CARREAU, (0.008, 1.0, 0.5))):
            ctx.set_viscosity_law(law, params)
            for call in (lambda: ctx.step_scalar_imex(rtol=1e-13), lambda: ctx.scalar_explicit(nat.U1, nat.T1, 0, 1.0)):
                with pytest.raises(nat.NativeError, match=r"viscosity law is not 1 \(Smagorinsky\), 4 \(WALE\) or 5 \(Vreman\)"):
                    call()
        assert ctx.scalar_info()["convection_launches"] == 0 and ctx.scalar_sgs_info()["launches"] == 0
        for law, params in ((WALE, (0.5, )), (VREMAN, (0.1, ))):
            ctx.set_viscosity_law(law, params)
            assert ctx.step_scalar_imex(rtol=1e-13).converged
        assert ctx.scalar_sgs_info()["launches"] == 2
    finally:
        ctx.close()


_KAPPA = 0.05


@pytest.mark.parametrize("law", (WALE, VREMAN))
def test_coupled_steps_match_the_restatements(law):
    """box(8, 8) cavity, SBDF2, 3 coupled steps (set_scalar_sgs, step_scalar_imex, step_imex, advance) with buoyancy,
    Dirichlet sides and a source, the law in the flow step and kappa_x = nu_x / 0.85 in the transport step, against
    IMEXViscRestatement and ScalarIMEXSgsRestatement with the new nu_x; beside them on the host the same pair without
    the subgrid heat flux.  One launch per step, nothing recomputed"""
    mesh, dm, marks, s, rs, make = _mesh((8, 8))
    params = _STEP_LAWS[law]
    X = dm.p2_coords
    b = _B[:2]
    vbc, tbc = cavity_bc(dm, marks), _two_sides(dm, marks, X)
    _, T_init = smooth_fields(X)
    q = np.cos(2.0 * X[:, 0] + 0.3) * np.sin(1.5 * X[:, 1] + 0.2)
    f = np.stack([np.sin(np.pi * X[:, 1]), -1.0 + X[:, 0]], axis=1).ravel()
    visc = SubgridModelRestatement(rs, law, params)
    sgs = SubgridScalarSgsRestatement(rs, law, params, _PRT)
    pairs = []
    for term in (sgs, None):
        flow = IMEXViscRestatement(s, _COEF, "standard", visc=visc)
        orc = ScalarIMEXSgsRestatement(s, _KAPPA, "standard", term)
        orc.source = q
        orc.T[0], orc.T[1] = T_init.copy(), T_init.copy()
        pairs.append((flow, orc))
    ctx = make(mesh, dm)
    try:
        ctx.set_coeffs(1.0, 1.0, 0.01, 1.0)
        ctx.set_dirichlet(nat.VELOCITY, *vbc)
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        ctx.set_dirichlet(nat.SCALAR, *tbc)
        ctx.set_scalar(_KAPPA, b, 0)
        ctx.set_viscosity_law(law, params)
        ctx.set_scalar_sgs(_PRT)
        ctx.set_state(nat.BODY_FORCE, f)
        ctx.set_state(nat.T_SOURCE, q)
        ctx.set_state(nat.T0, T_init)
        ctx.set_state(nat.T1, T_init)
        opts = _opts(ctx)
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=1.0 / 16.0)
        kappa_x_max = 0.0
        for step in range(3):
            ts.update_coefficients()
            kk = ts.get_next_step_size()
            for flow, orc in pairs:
                if orc.sgs is not None:
                    for level in (1, 2) if ts.beta[1] != 0.0 else (1, ):
                        kappa_x_max = max(kappa_x_max, float(sgs.kappa_x(flow.vel[level]).max()))
                orc.step(ts.alpha, ts.beta, ts.gamma, kk, flow.vel[1], flow.vel[2], tbc)
                flow.body_force = f + np.outer(orc.T[0], b).ravel()
                flow.step(ts.alpha, ts.beta, ts.gamma, kk, vbc, NO_PBC)
            flow, orc = pairs[0]
            ctx.set_imex(ts.alpha, ts.beta, ts.gamma, kk)
            si = ctx.step_scalar_imex(rtol=1e-13)
            et = rel(ctx.get_state(nat.T0), orc.T[0])
            ctx.step_imex(opts)
            us, u, p = ctx.get_state(nat.USTAR), ctx.get_state(nat.U0), ctx.get_state(nat.P)
            es, eu, ep = rel(us, flow.ustar), rel(u, flow.vel[0]), rel(p - p.mean(), flow.p - flow.p.mean())
            print("coupled law %d step %d: T %.2e u* %.2e u %.2e p %.2e cg %d" % (law, step, et, es, eu, ep, si.iterations))
            assert si.converged and et < 1e-9, (step, et)
            assert es < 1e-9 and eu < 1e-9 and ep < 1e-8, (step, es, eu, ep)
            ctx.advance(0)
            for fl, o in pairs:
                o.advance()
                fl.advance()
            ts.advance_time()
        effect = rel(pairs[0][1].T[1], pairs[1][1].T[1])
        print("coupled law %d: effect of D on T %.2e, max kappa_x %.3e = %.3f kappa" % (law, effect, kappa_x_max,
                                                                                      kappa_x_max / _KAPPA))
        assert effect >= 1e-4 and 0.0 < kappa_x_max < _KAPPA / 3.0
        info = ctx.scalar_info()
        assert info["convection_launches"] == 3 and info["convection_reuses"] == 2, info
        assert ctx.scalar_sgs_info() == dict(active=True, launches=3, recomputed=0)
        assert ctx.viscosity_info() == dict(law=law, element_launches=3, recomputed=0)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 7. the wall rows
_WALL_PRT = 0.4
_WALL_CW = 2.0
# rounded operations the WALE law adds to the chain of a point over the 3 of Smagorinsky: an entry of G G (3 fused
# terms), its symmetric part (2), the trace and its third (3), the difference (1), 9 squares summed (9), B sqrt(B) (2),
# B sqrt(sqrt(B)) (3), the sum of the denominator (1), the quotient (1), (C_w^2 Delta^2) times it (3)
_WALE_OPS = 28 - 3


def _wall_reference(mesh, dm, cells, local, u, T, p, opts, cw, prt):
    """rows of k_wall_facets<DIM, 4> with use_law and Pr_t, and their per-entry bounds: the molecular rows of
    ``wall_reference`` plus int nu_x (G + G^T) n in the viscous-force and torque entries and int -(nu_x / Pr_t)
    grad T . n in the conductive entry, by the kernel's facet rule -- the evaluation of section 5 of tests/
    test_gpu_scalar_sgs.py with the WALE nu_x.  Bound: 2 n eps times the sums of the absolute contributions, n =
    n_terms(dim, law) + 2 + _WALE_OPS.  The absolute version of nu_x: the law is homogeneous of degree one in G, so
    nu_x = sum_ab G_ab d nu_x / d G_ab (Euler) and a relative error eps_ab of the entries moves it by
    sum_ab |d nu_x / d G_ab| |G_ab| eps_ab to first order; with G^ the absolute sums of the entries (the scale of their
    rounding errors) that is nu^ = sum_ab |d nu_x / d G_ab| G^_ab >= nu_x, for Smagorinsky the gamma^ of the module this
    comes from.  The derivatives are central differences of the restatement's own law"""
    import test_wall_quantities_host as wh
    dim = dm.dim
    cells, local = np.asarray(cells, dtype=np.int64), np.asarray(local, dtype=np.int64)
    nf = cells.size
    x = np.asarray(mesh.coords, dtype=np.float64)[np.asarray(mesh.cells, dtype=np.int64)[cells]][:, :, :dim]
    keep = np.array([[v for v in range(dim + 1) if v != o] for o in range(dim + 1)], dtype=np.int64)[local]
    xf = x[np.arange(nf)[:, None], keep]
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
    pts, wts = wh.facet_rule(dim, "kernel")
    xq = np.einsum("qv,fvd->fqd", pts, xf)
    J = np.stack([x[:, k + 1] - x[:, 0] for k in range(dim)], axis=2)
    Jinv = np.linalg.inv(J)
    xi = np.einsum("fab,fqb->fqa", Jinv, xq - x[:, None, 0, :])
    lam = np.concatenate([1.0 - xi.sum(axis=2, keepdims=True), xi], axis=2)
    p2 = np.asarray(dm.p2_dofmap, dtype=np.int64)[cells]
    ue = np.asarray(u, dtype=np.float64).reshape(-1, dim)[p2]
    Te = np.asarray(T, dtype=np.float64)[p2]
    delta2 = ((np.abs(np.linalg.det(J)) / (2.0 if dim == 2 else 6.0)) ** (2.0 / dim))[:, None]
    w = area[:, None] * wts[None, :]
    org = np.asarray(opts["origin"], dtype=np.float64)[:dim]
    ident = lambda a: a
    g2 = np.einsum("fba,fqkb->fqka", Jinv, wh.p2_basis(lam, ident)[1])
    G = np.einsum("fqkb,fka->fqab", g2, ue)                               # d_b u_a
    g2h = np.einsum("fba,fqkb->fqka", np.abs(Jinv), wh.p2_basis(lam, np.abs)[1])
    Gh = np.einsum("fqkb,fka->fqab", g2h, np.abs(ue))
    nu = tensor_nu(WALE, G, delta2, cw)
    nuh = np.zeros_like(nu)
    h = 1e-6 * np.sqrt((G * G).sum(axis=(2, 3)))
    for a in range(dim):
        for b in range(dim):
            E = np.zeros((dim, dim))
            E[a, b] = 1.0
            d = (tensor_nu(WALE, G + h[..., None, None] * E, delta2, cw) -
                 tensor_nu(WALE, G - h[..., None, None] * E, delta2, cw)) / (2.0 * h)
            nuh += np.abs(d) * Gh[..., a, b]
    assert np.all(nuh >= nu * (1.0 - 1e-6))
    nh = np.abs(nrm)
    gl0 = np.abs(Jinv).sum(axis=1)
    nh = np.where((local == 0)[:, None], gl0 / np.linalg.norm(Jinv.sum(axis=1), axis=1, keepdims=True), nh)
    rows = wh.wall_reference(mesh, dm, (cells, local), u, p, T, opts, rule="kernel")
    scale = wh.wall_reference(mesh, dm, (cells, local), u, p, T, opts, absolute=True, rule="kernel")
    tl = nu[:, :, None] * np.einsum("fqab,fb->fqa", G + np.swapaxes(G, 2, 3), nrm)
    tlh = nuh[:, :, None] * np.einsum("fqab,fb->fqa", Gh + np.swapaxes(Gh, 2, 3), nh)
    r, rh = xq - org[None, None, :], np.abs(xq) + np.abs(org)[None, None, :]
    if dim == 2:
        tq = (r[..., 0] * tl[..., 1] - r[..., 1] * tl[..., 0])[..., None]
        tqh = (rh[..., 0] * tlh[..., 1] + rh[..., 1] * tlh[..., 0])[..., None]
    else:
        tq = np.stack([r[..., 1] * tl[..., 2] - r[..., 2] * tl[..., 1], r[..., 2] * tl[..., 0] - r[..., 0] * tl[..., 2],
                       r[..., 0] * tl[..., 1] - r[..., 1] * tl[..., 0]], axis=-1)
        tqh = np.stack([rh[..., 1] * tlh[..., 2] + rh[..., 2] * tlh[..., 1], rh[..., 2] * tlh[..., 0] + rh[..., 0] * tlh[..., 2],
                        rh[..., 0] * tlh[..., 1] + rh[..., 1] * tlh[..., 0]], axis=-1)
    add, addh = np.zeros_like(rows), np.zeros_like(rows)
    add[:, 1 + dim:1 + 2 * dim], addh[:, 1 + dim:1 + 2 * dim] = np.einsum("fq,fqa->fa", w, tl), np.einsum("fq,fqa->fa", w, tlh)
    add[:, 4 + 2 * dim:], addh[:, 4 + 2 * dim:] = np.einsum("fq,fqa->fa", w, tq), np.einsum("fq,fqa->fa", w, tqh)
    add[:, 3 + 2 * dim] = -np.einsum("fq,fq,fqkb,fk,fb->f", w, nu / prt, g2, Te, nrm)
    addh[:, 3 + 2 * dim] = np.einsum("fq,fq,fqkb,fk,fb->f", w, nuh / prt, g2h, np.abs(Te), nh)
    bound = 2.0 * (wh.n_terms(dim, True) + 2 + _WALE_OPS) * wh.EPS * (scale + addh)
    return rows, add, bound


@pytest.mark.parametrize("name", ["box4x4", "kuhn3x2x2"])
def test_wall_rows_carry_the_wale_viscosity_and_diffusivity(name):
    """box(4, 4) and the (3, 2, 2) Kuhn box, every boundary facet, law 4, use_law, Pr_t = 0.4: the viscous-force (and
    torque) entries carry nu_x (G + G^T) n, the conductive entry -(kappa + nu_x / Pr_t) grad T . n; with Pr_t off the
    conductive entry keeps the molecular bytes; with use_law off every row keeps the bytes of a context without a law"""
    import test_wall_quantities_host as wh
    from test_derived_fields_host import smooth_fields as wall_fields
    mesh, dm, marks, s, rs, make = _mesh((4, 4) if name == "box4x4" else KUHN)
    dim = dm.dim
    ids, cells, local = wh.boundary_facets(mesh)
    u, p, T = wall_fields(dm.p2_coords, dm.p1_coords)
    o = wh.OPTS
    rows, add, bound = _wall_reference(mesh, dm, cells, local, u, T, p, o, _WALL_CW, _WALL_PRT)
    want = rows + add
    heat, force = 3 + 2 * dim, slice(1 + dim, 1 + 2 * dim)
    assert np.abs(add[:, heat]).max() > 1e3 * bound[:, heat].max() and np.abs(add[:, heat]).max() > 1e-3
    assert np.abs(add[:, force]).max() > 1e3 * bound[:, force].max() and np.abs(add[:, force]).max() > 1e-3
    group = np.zeros(ids.size, dtype=np.int32)
    out = {}
    for with_law in (True, False):
        ctx = make(mesh, dm)
        try:
            ctx.set_scalar(o["kappa"])
            ctx.set_state(nat.T0, T)
            ctx.set_state(nat.U0, np.ascontiguousarray(u).ravel())
            ctx.set_state(nat.P, p)
            ctx.wall_set_facets(cells, local, group, 1)

            def compute(use_law):
                return ctx.wall_compute(o["nu"], o["sym"], o["kappa"], o["origin"], use_law=use_law, scalar_slot=nat.T0,
                                        facets=True)
            if with_law:
                ctx.set_viscosity_law(WALE, (_WALL_CW, ))
                out["no Pr_t"] = compute(True)
                ctx.set_scalar_sgs(_WALL_PRT)
                out["on"] = compute(True)
                out["use_law off"] = compute(False)
            else:
                out["no law"] = compute(True)
        finally:
            ctx.close()
    rows_on = out["on"][1]
    err = np.abs(rows_on - want)
    print("wall %s: max error %.3e; error / bound: viscous force %.2e, heat %.2e; eddy parts %.3e %.3e" % (
        name, err.max(), (err[:, force] / bound[:, force]).max(), (err[:, heat] / bound[:, heat]).max(),
        np.abs(add[:, force]).max(), np.abs(add[:, heat]).max()))
    assert (err <= bound).all()
    others = [c for c in range(rows_on.shape[1]) if c != heat]
    assert rows_on[:, others].tobytes() == out["no Pr_t"][1][:, others].tobytes()
    assert (np.abs(out["no Pr_t"][1][:, heat] - rows[:, heat]) <= bound[:, heat]).all()
    for k in (0, 1):
        assert out["use_law off"][k].tobytes() == out["no law"][k].tobytes()


# ---------------------------------------------------------------- 8. through the classes
_SPEC = dict(name="Cavity", mesh=("cube", 2, 8), scheme="ipcs", clock=dict(dt=0.5 / 8, steps=3),
             numbers=dict(Re=100.0, Fr=1.0), start={"velocity": (0.0, 0.0), "pressure": 0.0, "temperature": 0.5},
             bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_slip", "bottom"), ("velocity", "top", (1.0, 0.0))])


def test_boussinesq_solver_with_the_wale_model_equals_driving_the_steps_by_hand(monkeypatch):
    """BoussinesqIMEXSolver through InstationaryProblem.solve_problem with WALEModel(cw, prandtl_t = 0.85) on the 8 x 8
    cavity, 3 steps: T and u are bit for bit what set_viscosity_law(4) / set_scalar_sgs / step_scalar_imex / step_imex /
    advance give through the C ABI on a second context; _compute_model_viscosity returns viscosity_cells and
    _compute_model_diffusivity that divided by Pr_t"""
    from fem_function import HostField
    from multigrid import attach_hierarchy
    from ns_boussinesq_solver import BoussinesqIMEXSolver
    from problem_specs import build_problem
    from viscosity_models import VremanModel, WALEModel
    steps, dt = _SPEC["clock"]["steps"], _SPEC["clock"]["dt"]
    cw = _STEP_LAWS[WALE][0]
    monkeypatch.setenv("NSFEM_NO_OUTPUT", "1")
    problem = build_problem(dict(_SPEC))
    cls = type(problem)

    def set_viscosity_model(self):
        self._viscosity_model = WALEModel(cw, prandtl_t=_PRT)

    def set_temperature_coefficients(self):
        self._temperature_coefficients = dict(diffusivity=_KAPPA, buoyancy=(0.0, 1.0), convective_form="standard")

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
    assert solver._ctx.viscosity_info() == dict(law=WALE, element_launches=steps, recomputed=0)
    assert solver._ctx.scalar_sgs_info() == dict(active=True, launches=steps, recomputed=0)
    T_cls, u_cls = solver._ctx.get_state(nat.T1), solver._ctx.get_state(nat.U1)
    means = solver._ctx.viscosity_cells(nat.U0)
    field = problem._compute_model_viscosity()
    assert isinstance(field, HostField) and field.center == "Cell" and field.name() == "model viscosity"
    assert np.array_equal(field.values, means) and means.max() > 1e-4
    field = problem._compute_model_diffusivity()
    assert field.name() == "model diffusivity" and np.array_equal(field.values, means / _PRT)
    # ---- the same steps through the C ABI on a fresh context
    dm, mesh = solver._dofmap, solver._mesh
    left = np.unique(dm.facet_p2_nodes(solver._boundary_markers.facets_with_id(problem._sides["left"])))
    right = np.unique(dm.facet_p2_nodes(solver._boundary_markers.facets_with_id(problem._sides["right"])))
    out = {}
    for law, params in ((WALE, (cw, )), (SMAGORINSKY, (0.2, ))):
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
            ctx.set_scalar(_KAPPA, (0.0, 1.0), 0)
            ctx.set_viscosity_law(law, params)
            ctx.set_scalar_sgs(_PRT)
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
            out[law] = (ctx.get_state(nat.T1), ctx.get_state(nat.U1))
        finally:
            ctx.close()
    assert np.abs(u_cls).max() > 0.5 and np.abs(T_cls - 0.5).max() > 1e-2
    assert np.array_equal(T_cls, out[WALE][0]) and np.array_equal(u_cls, out[WALE][1])
    assert rel(out[SMAGORINSKY][1], u_cls) > 1e-5                            # (another law is another flow)
    # the Vreman model handed over in the middle of the run: law 5 on the device, the term off without prandtl_t
    solver.set_viscosity_model(VremanModel(0.1))
    assert solver._ctx.viscosity_info()["law"] == VREMAN and solver._ctx.scalar_sgs_info()["active"] is False
    with pytest.raises(RuntimeError, match="prandtl_t"):
        problem._compute_model_diffusivity()
    solver.set_viscosity_model(VremanModel(0.1, prandtl_t=_PRT))
    assert solver._ctx.scalar_sgs_info()["active"] is True
