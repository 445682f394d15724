"""Wall-stress models in the IMEX step on the GPU (nsfem_set_wall_model / nsfem_wall_model_residual /
nsfem_wall_model_facets / nsfem_wall_model_info) against the numpy restatement of tests/wall_model_host.py.

Tolerances.  The facet kernel calls sqrt, pow, log1p, expm1 and exp.  The largest difference of W(u) and of the
diagnostics rows, relative to the largest entry, over the 94 cases of test 1 below was measured as 7.35e-16
(MEASURED_KERNEL_ERROR; the cases lie between 5e-17 and that, so this is the rounding of the sums, not of the library);
the tests assert ten times that, capped at 1e-11 (the project's rule for kernels with library functions; DESIGN.md
4x).  Steps: those of tests/test_gpu_imex.py for the same Krylov settings (rtol 1e-13) -- u*, u 1e-9 and p minus its
mean 1e-8, relative.

Meshes.  Test 1: ``_KERNEL_MESHES`` of tests/test_gpu_variable_viscosity.py with every marked wall modelled (the two
periodic fixtures without a wall have no facet to model and are no case).  nu is chosen per case, on the host, so that
the facets fall on both sides of law 1's switch Re_y = A^(2/(1-B)): at least 4 facets with a quadrature point below,
4 with one above (pchan2 has 8 modelled facets in all), and no point within 1e-9 (relative) of the switch.  Tests 2
to 4: the periodic channels, box(16, 16) -- the smallest lattice on which the one-launch right-hand side runs -- and
the (3, 2, 2) Kuhn box."""
import copy
import math

import numpy as np
import pytest

import _native as nat
import wall_model_host as wm
from gpu_common import cavity_bc, rel
from imex_time_stepping import IMEXTimeStepping, IMEXType
from immersed_bodies import ImmersedBodies
from periodic_meshes import is_periodic, lengths_of, wall_axes
from test_gpu_3d import lid_bc
from test_gpu_variable_viscosity import (_COEF, _CS_STEPS, _KERNEL_MESHES, NO_PBC, _advance, _mesh, _opts, _solve,
                                         velocity_on)
from test_immersed_bodies_host import PenalisationRestatement, bodies_2d, bodies_3d
from test_variable_viscosity_host import SMAGORINSKY, VariableViscosityRestatement

pytestmark = pytest.mark.gpu

PARAMS = {wm.WERNER_WENGLE: (wm.WW_A, wm.WW_B), wm.REICHARDT: (wm.RD_KAPPA, wm.RD_C)}
# largest |device - restatement| / max |restatement| over all cases of test 1 (W and the rows), as measured on an MI355X
MEASURED_KERNEL_ERROR = 7.35e-16
KERNEL_TOL = min(10.0 * MEASURED_KERNEL_ERROR, 1e-11)
WALL_KINDS = [k for k in _KERNEL_MESHES if not is_periodic(k) or wall_axes(k)]
BOX2, BOX3 = (16, 16), ((3, 2, 2), (1.0, 0.8, 0.6))

_ORC = {}


def wall_ids(marks):
    return tuple(sorted(i for i in marks.ids() if i > 0))


def restatement(kind, matching, ids=None):
    """the WallModelRestatement of a mesh kind, a matching and a set of boundary ids (all marked walls by default) with
    law 1, nu = 1 and no wall velocity: built once, the tests work on shallow copies"""
    mesh, dm, marks = _mesh(kind)[:3]
    ids = wall_ids(marks) if ids is None else tuple(ids)
    key = (str(kind), matching, ids)
    if key not in _ORC:
        cells, local, _ = wm.modelled_facets(mesh, marks, ids)
        _ORC[key] = wm.WallModelRestatement(mesh, dm, cells, local, wm.WERNER_WENGLE, PARAMS[wm.WERNER_WENGLE], 1.0,
                                            matching)
    return copy.copy(_ORC[key])


def wall_velocity(nf, dim):
    return np.array([0.3, -0.2, 0.15])[None, :dim] * (1.0 + 0.25 * np.sin(1.7 * np.arange(nf)))[:, None]


def kernel_case(kind, law, matching, with_uw):
    """(restatement with the case's law, wall velocity and nu, velocity): nu splits the facets about law 1's switch"""
    dm = _mesh(kind)[1]
    orc = restatement(kind, matching)
    orc.law, orc.params = law, PARAMS[law]
    if with_uw:
        orc.uw = wall_velocity(orc.nf, orc.dim)
    u = velocity_on(kind, dm)
    orc.nu = 1.0
    s = orc.re_y(u)                                     # y |u_par|
    v = np.sort(s.ravel())
    # the gap between two sorted values nearest to the middle (with theta = 1 the points of a facet share one sample)
    gaps = np.nonzero(v[1:] > (1.0 + 1e-6) * v[:-1])[0] + 1
    m = int(gaps[np.abs(gaps - v.size // 2).argmin()])
    switch = wm.ww_switch()
    orc.nu = math.sqrt(v[m - 1] * v[m]) / switch
    re = orc.re_y(u)
    # a facet falls on a side when one of its quadrature points does: each branch of the law runs in >= 4 facets
    below, above = int((re.min(axis=1) <= switch).sum()), int((re.max(axis=1) > switch).sum())
    assert below >= 4 and above >= 4, (kind, law, matching, below, above)
    assert np.abs(re / switch - 1.0).min() > 1e-9
    return orc, u


def set_model(ctx, orc):
    ctx.set_wall_model(orc.law, orc.params, orc.cells, orc.local, orc.sc, orc.sl, orc.sy,
                       orc.uw if orc.uw.any() else None)


def _max_rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def _rows_rel(got, want):
    """the largest difference of a column relative to its largest entry; the dim columns of int tau_w count as one (on
    an axis-aligned wall the normal one is zero)"""
    dim = want.shape[1] - 4
    groups = [slice(0, 1), slice(1, 1 + dim)] + [slice(j, j + 1) for j in range(1 + dim, 4 + dim)]
    return float(max(np.abs(got[:, g] - want[:, g]).max() / np.abs(want[:, g]).max() for g in groups))


def kernel_cases(kind):
    dim = _mesh(kind)[0]._dim
    cases = [(law, ("cell", theta), uw) for law in (wm.WERNER_WENGLE, wm.REICHARDT) for theta in (1.0, 0.5)
             for uw in (False, True)]
    if kind in ((8, 8), BOX3):
        cases.append((wm.REICHARDT, ("distance", 0.07 if dim == 2 else 0.11), True))
    return cases


# ---------------------------------------------------------------- 1. the kernels against the restatement
@pytest.mark.parametrize("kind", WALL_KINDS, ids=str)
def test_wall_model_kernels_match_the_restatement(kind):
    """weight * W(u) and the diagnostics rows for the smooth non-polynomial velocity: both laws, theta 1 and 1/2, with
    and without a wall velocity, one "distance" case per dimension; a second call returns the same bytes, the weight
    rides in the kernel, no stored state is touched"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    ctx = make(mesh, dm)
    worst = 0.0
    try:
        launches = 0
        for law, matching, with_uw in kernel_cases(kind):
            orc, u = kernel_case(kind, law, matching, with_uw)
            want, rows = orc.residual(u), orc.facet_rows(u)
            ctx.set_coeffs(1.0, 1.0, orc.nu, 1.0)
            ctx.set_state(nat.U1, u)
            ctx.set_state(nat.USTAR, u)
            set_model(ctx, orc)
            got = ctx.wall_model_residual(nat.U1, 1.0)
            got_rows = ctx.wall_model_facets(nat.U1)
            err, rerr = _max_rel(got, want), _rows_rel(got_rows, rows)
            worst = max(worst, err, rerr)
            print("kernel %s law %d %s uw %d: W %.2e rows %.2e (of the largest entry), nu %.3e, max y+ %.1f"
                  % (kind, law, matching, with_uw, err, rerr, orc.nu, rows[:, -1].max()))
            assert np.abs(want).max() > 1e-6 and got_rows.shape == rows.shape
            assert err < KERNEL_TOL and rerr < KERNEL_TOL, (kind, law, matching, with_uw, err, rerr)
            assert got.tobytes() == ctx.wall_model_residual(nat.U1, 1.0).tobytes()
            assert got_rows.tobytes() == ctx.wall_model_facets(nat.U1).tobytes()
            assert _max_rel(ctx.wall_model_residual(nat.USTAR, -1.5), -1.5 * want) < KERNEL_TOL
            launches += 5
            info = ctx.wall_model_info()
            assert info == dict(facets=orc.nf, launches=launches, recomputed=0, law=law), info
        print("kernel %s: largest difference %.2e" % (kind, worst))
        assert not ctx.get_state(nat.CONV_N1).any() and not ctx.get_state(nat.CONV_N2).any()
        assert np.array_equal(ctx.get_state(nat.U1), u)
        for slot in (nat.P, nat.CONV_N1, nat.BODY_FORCE):
            with pytest.raises(nat.NativeError, match="slot"):
                ctx.wall_model_residual(slot, 1.0)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 2. the fixed point of a channel
def channel_case(kind, law, G, nu=0.05):
    """both walls of a periodic channel modelled, body force G e_x: the exact steady flow u = G/(2 nu) y (H - y) + u_s
    with u_s from G H / 2 = nu r(Re_y) U_m / y_m, i.e. y+ = y_m sqrt(G H / 2) / nu and Re_y = y+ u+(y+)"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    dim = mesh._dim
    H = lengths_of(kind)[1]
    orc = restatement(kind, ("cell", 1.0), (3, 4))
    orc.law, orc.params, orc.nu = law, PARAMS[law], nu
    y_m = float(orc.sy[0, 0])
    assert np.abs(orc.sy - y_m).max() < 1e-14
    yp = y_m * math.sqrt(0.5 * G * H) / nu
    if law == wm.WERNER_WENGLE:
        re = yp * yp if yp * yp <= wm.ww_switch() else wm.WW_A * yp ** (1.0 + wm.WW_B)
    else:
        re = yp * float(wm.reichardt_uplus(yp))
    U_m = re * nu / y_m
    u_s = U_m - 0.5 * G / nu * y_m * (H - y_m)
    y = dm.p2_coords[:, 1]
    u = np.zeros((dm.n_p2, dim))
    u[:, 0] = 0.5 * G / nu * y * (H - y) + u_s
    f = np.zeros((dm.n_p2, dim))
    f[:, 0] = G
    nodes = np.unique(dm.facet_p2_nodes(np.concatenate([marks.facets_with_id(i) for i in (3, 4)])))
    vbc = (np.sort(dim * nodes + 1).astype(np.int64), np.zeros(nodes.size))
    return orc, u.ravel(), f.ravel(), vbc, re, u_s


@pytest.mark.parametrize("law,G", [(wm.WERNER_WENGLE, 1.0), (wm.WERNER_WENGLE, 40.0), (wm.REICHARDT, 40.0)])
@pytest.mark.parametrize("kind", ("pchan2", "pchan3"))
def test_the_modelled_channel_keeps_its_steady_flow(kind, law, G):
    """old levels = the exact flow, p = 0: one SBDF2 step and one CNAB step leave u unchanged -- the sign of W, its
    scaling by nu and y and the treatment of the normal.  Law 1 in the sublayer (G = 1: u_s = G y_m^2 / (2 nu)) and
    beyond the switch (G = 40), law 2"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    nu = 0.05
    orc, u, f, vbc, re, u_s = channel_case(kind, law, G, nu)
    y_m = float(orc.sy[0, 0])
    if law == wm.WERNER_WENGLE:
        assert (re < wm.ww_switch()) == (G == 1.0)
        if G == 1.0:
            assert abs(u_s - G * y_m * y_m / (2.0 * nu)) < 1e-13 * u_s
    # the restatement holds the flow: c_v K u + W(u) = M f on the rows without a Dirichlet condition
    defect = nu * (s.vector_stiffness(False) @ u) + orc.residual(u) - s.vector_mass() @ f
    free = np.ones(u.size, dtype=bool)
    free[vbc[0]] = False
    assert np.abs(defect[free]).max() < 1e-11 * np.abs(s.vector_mass() @ f).max() * max(1.0, re)
    ctx = make(mesh, dm)
    try:
        ctx.set_coeffs(1.0, 1.0, nu, 1.0)
        ctx.set_dirichlet(nat.VELOCITY, *vbc)
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        ctx.set_state(nat.BODY_FORCE, f)
        ctx.set_state(nat.U1, u)
        ctx.set_state(nat.U2, u)
        set_model(ctx, orc)
        opts = _opts(ctx)
        for typ in (IMEXType.SBDF2, IMEXType.CNAB):
            alpha, beta, gamma = IMEXTimeStepping(0.0, 1.0, typ, desired_start_time_step=0.1).uniform_coefficients()
            assert beta[1] != 0.0
            ctx.set_imex(alpha, beta, gamma, 2.0e-3)
            ctx.step_imex(opts)
            us, u0, p = ctx.get_state(nat.USTAR), ctx.get_state(nat.U0), ctx.get_state(nat.P)
            es, eu, ep = rel(us, u), rel(u0, u), float(np.abs(p - p.mean()).max())
            print("channel %s law %d G %g %s: Re_y %.1f u_s %.3f  u* %.2e u %.2e  max |p - mean| %.2e"
                  % (kind, law, G, typ.name, re, u_s, es, eu, ep))
            assert es < 1e-9 and eu < 1e-9, (kind, law, G, typ.name, es, eu)
        assert ctx.wall_model_info()["launches"] == 3          # N(u2) once, N(u1) per step
    finally:
        ctx.close()


# ---------------------------------------------------------------- 3. steps against the composed restatement
def modelled_floor_bc(dm, marks):
    """the cavity / lid conditions with the floor y = 0 (id 3) modelled: its nodes off the other walls keep
    u.n = u_y = 0 only"""
    dim = dm.p2_coords.shape[1]
    dofs, vals = cavity_bc(dm, marks) if dim == 2 else lid_bc(dm, marks)
    floor = np.unique(dm.facet_p2_nodes(marks.facets_with_id(3)))
    others = np.unique(dm.facet_p2_nodes(np.concatenate([marks.facets_with_id(i) for i in wall_ids(marks) if i != 3])))
    inner = np.setdiff1d(floor, others)
    drop = np.concatenate([dim * inner + a for a in range(dim) if a != 1])
    keep = ~np.isin(dofs, drop)
    assert inner.size > 0 and keep.sum() == dofs.size - drop.size
    return (dofs[keep], vals[keep]), inner


def step_setup(ctx, kind, law, with_others, on_device=True):
    mesh, dm, marks, s, rs, make = _mesh(kind)
    dim = mesh._dim
    X = dm.p2_coords
    vbc, inner = modelled_floor_bc(dm, marks)
    wall = restatement(kind, ("cell", 1.0), (3, ))
    wall.law, wall.params, wall.nu = law, PARAMS[law], _COEF["viscous_term"]
    wall.uw = np.tile(np.array([0.5, 0.0, -0.2])[:dim], (wall.nf, 1))          # the floor slides: W acts from step 1
    visc = penal = None
    k = 0.5 / (kind[0] if isinstance(kind[0], int) else kind[0][0])
    if with_others:
        visc = VariableViscosityRestatement(rs, SMAGORINSKY, (_CS_STEPS, ))
        bodies = ImmersedBodies((bodies_2d if dim == 2 else bodies_3d)("disc"), 2.0 * k, 0.07)
        penal = PenalisationRestatement(rs, bodies)
        ctx.set_viscosity_law(SMAGORINSKY, (_CS_STEPS, ))
        ctx.set_bodies(bodies.rows(), bodies.eta, bodies.smoothing)
    orc = wm.IMEXWallRestatement(s, _COEF, "standard", visc=visc, penal=penal, wall=wall)
    f = np.stack([np.sin(np.pi * X[:, 1]), -1.0 + X[:, 0], 0.5 * X[:, 1]][:dim], axis=1).ravel()
    orc.body_force = f
    ctx.set_coeffs(1.0, 1.0, _COEF["viscous_term"], 1.0)
    ctx.set_dirichlet(nat.VELOCITY, *vbc)
    ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
    ctx.set_state(nat.BODY_FORCE, f)
    if on_device:
        set_model(ctx, wall)
    return orc, vbc, inner, k


@pytest.mark.parametrize("with_others", (False, True), ids=("alone", "with-smagorinsky-and-a-body"))
@pytest.mark.parametrize("kind", (BOX2, BOX3), ids=str)
def test_steps_with_a_modelled_floor_match_the_restatement(kind, with_others):
    """three SBDF2 steps (the third reads the stored N2) of the cavity whose floor is modelled and slides: u*, u and p
    against the composed restatement, alone (law 2) and together with a Smagorinsky law and a body (law 1; the order
    V, B, W)"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    ctx = make(mesh, dm)
    try:
        law = wm.WERNER_WENGLE if with_others else wm.REICHARDT
        orc, vbc, inner, k = step_setup(ctx, kind, law, with_others)
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=k)
        opts = _opts(ctx)
        for _ in range(3):
            _solve(ctx, orc, ts, vbc, opts, "%s wall law %d others %d" % (kind, law, with_others))
            _advance(ctx, orc, ts)
        drag = np.abs(orc.vel[1][mesh._dim * inner]).max()
        print("%s: tangential velocity at the modelled floor %.3e" % (kind, drag))
        assert drag > 1e-4
        assert ctx.wall_model_info() == dict(facets=orc.wall.nf, launches=3, recomputed=0, law=law)
        if with_others:
            assert ctx.viscosity_info()["element_launches"] == 3 and ctx.body_info()["element_launches"] == 3
    finally:
        ctx.close()


# ---------------------------------------------------------------- 4. bookkeeping
def _plain_run(kind, steps, touch=None, model=False):
    """``steps`` SBDF2 steps with the modelled-floor conditions, with the model on the device or without any call of
    its setter; ``touch(ctx, orc)`` before the first step"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    ctx = make(mesh, dm)
    try:
        orc, vbc, inner, k = step_setup(ctx, kind, wm.WERNER_WENGLE, False, on_device=model)
        if touch:
            touch(ctx, orc)
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=k)
        opts = _opts(ctx)
        for _ in range(steps):
            ts.update_coefficients()
            ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
            ctx.step_imex(opts)
            ctx.advance(0)
            ts.advance_time()
        return ctx.get_state(nat.U1), ctx.get_state(nat.P_OLD), ctx.imex_info(), ctx.wall_model_info()
    finally:
        ctx.close()


def test_a_model_switched_off_leaves_no_trace_and_a_model_keeps_the_path():
    """box(16, 16): a context that never had a model and one that set a model and switched it off give the same bytes;
    with a model the same right-hand-side paths are counted (the model does not change which path runs)"""
    def on_and_off(ctx, orc):
        set_model(ctx, orc.wall)
        ctx.set_wall_model(0)
    u_a, p_a, info_a, w_a = _plain_run(BOX2, 3)
    u_b, p_b, info_b, w_b = _plain_run(BOX2, 3, touch=on_and_off)
    assert u_a.tobytes() == u_b.tobytes() and p_a.tobytes() == p_b.tobytes()
    assert w_a == dict(facets=0, launches=0, recomputed=0, law=0) and w_b == w_a
    u_c, p_c, info_c, w_c = _plain_run(BOX2, 3, model=True)
    assert info_a == info_b and info_c == info_a, (info_a, info_c)
    assert w_c["launches"] == 3 and w_c["recomputed"] == 0 and rel(u_c, u_a) > 1e-6


def test_changing_the_model_recomputes_the_stored_vector():
    """two steps with law 1, then law 2: the third step forms N(u2) afresh with the new law (counter 1) and agrees with
    the restatement that does the same; the same model again recomputes nothing"""
    kind = BOX2
    mesh, dm, marks, s, rs, make = _mesh(kind)
    ctx = make(mesh, dm)
    try:
        orc, vbc, inner, k = step_setup(ctx, kind, wm.WERNER_WENGLE, False)
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=k)
        opts = _opts(ctx)
        for _ in range(2):
            _solve(ctx, orc, ts, vbc, opts, "law 1")
            _advance(ctx, orc, ts)
        set_model(ctx, orc.wall)                             # the same data again: the stored vector stays
        orc.wall.law, orc.wall.params = wm.REICHARDT, PARAMS[wm.REICHARDT]
        set_model(ctx, orc.wall)
        stored = orc.N2.copy()
        orc.N2 = None                                        # (the restatement forms N(u2) afresh with the new law)
        _solve(ctx, orc, ts, vbc, opts, "law 2")
        assert rel(stored, orc.explicit(orc.vel[2])) > 1e-6  # ... which is another vector than the stored one
        assert ctx.wall_model_info() == dict(facets=orc.wall.nf, launches=4, recomputed=1, law=wm.REICHARDT)
        _advance(ctx, orc, ts)
        _solve(ctx, orc, ts, vbc, opts, "law 2, stored")
        assert ctx.wall_model_info()["recomputed"] == 1 and ctx.wall_model_info()["launches"] == 5
    finally:
        ctx.close()


def test_advance_and_restore_behave_as_for_the_other_terms():
    """after nsfem_advance the slot NSFEM_CONV_N2 holds N(u1) with W; a second context that is handed the levels, the
    pressure and that vector goes on with the same bytes and recomputes nothing"""
    kind = BOX3
    mesh, dm, marks, s, rs, make = _mesh(kind)
    a, b = make(mesh, dm), make(mesh, dm)
    try:
        orc, vbc, inner, k = step_setup(a, kind, wm.REICHARDT, False)
        step_setup(b, kind, wm.REICHARDT, False)
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=k)
        opts = _opts(a)
        for _ in range(2):
            _solve(a, orc, ts, vbc, opts, "save")
            _advance(a, orc, ts)
        n2 = a.get_state(nat.CONV_N2)
        assert rel(n2, orc.N2) < 1e-9 and np.abs(orc.wall.residual(orc.vel[2])).max() > 1e-6
        for slot in (nat.U1, nat.U2, nat.P_OLD, nat.P, nat.CONV_N2):
            b.set_state(slot, a.get_state(slot))
        ts.update_coefficients()
        for ctx in (a, b):
            ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
            ctx.step_imex(_opts(ctx))
        assert a.get_state(nat.U0).tobytes() == b.get_state(nat.U0).tobytes()
        assert a.get_state(nat.P).tobytes() == b.get_state(nat.P).tobytes()
        assert b.wall_model_info()["recomputed"] == 0 and b.wall_model_info()["launches"] == 1
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- 5. refusals
def test_everything_the_header_refuses_is_refused():
    kind = (8, 8)
    mesh, dm, marks, s, rs, make = _mesh(kind)
    orc = restatement(kind, ("cell", 1.0), (3, ))
    group = nat.local_group_create(1)
    ctx = make(mesh, dm)
    try:
        ctx.attach_local_comm(group, 0)
        with pytest.raises(nat.NativeError, match="wall model: contexts with a communicator"):
            set_model(ctx, orc)
        ctx.set_wall_model(0)                                # no model is no feature: allowed
        assert ctx.wall_model_info()["law"] == 0
    finally:
        ctx.close()
        nat.local_group_destroy(group)
    ctx = make(mesh, dm)
    try:
        with pytest.raises(nat.NativeError, match="no model set"):
            ctx.wall_model_residual(nat.U1, 1.0)
        with pytest.raises(nat.NativeError, match="unknown law"):
            ctx.set_wall_model(3, (1.0, 0.1), orc.cells, orc.local, orc.sc, orc.sl, orc.sy)
        for bad, word in (((-1.0, 0.1), "A must"), ((8.3, 1.0), "B must"), ((8.3, np.nan), "B must")):
            with pytest.raises(nat.NativeError, match=word):
                ctx.set_wall_model(1, bad, orc.cells, orc.local, orc.sc, orc.sl, orc.sy)
        with pytest.raises(nat.NativeError, match="kappa"):
            ctx.set_wall_model(2, (0.0, 7.8), orc.cells, orc.local, orc.sc, orc.sl, orc.sy)
        cells = orc.cells.copy()
        cells[1] = mesh.num_cells()
        with pytest.raises(nat.NativeError, match="facet cell out of range"):
            ctx.set_wall_model(1, PARAMS[1], cells, orc.local, orc.sc, orc.sl, orc.sy)
        sc = orc.sc.copy()
        sc[2, 1] = -1
        with pytest.raises(nat.NativeError, match="sample cell out of range"):
            ctx.set_wall_model(1, PARAMS[1], orc.cells, orc.local, sc, orc.sl, orc.sy)
        local = orc.local.copy()
        local[0] = 3
        with pytest.raises(nat.NativeError, match="local facet index out of range"):
            ctx.set_wall_model(1, PARAMS[1], orc.cells, local, orc.sc, orc.sl, orc.sy)
        sy = orc.sy.copy()
        sy[0, 0] = 0.0
        with pytest.raises(nat.NativeError, match="wall distance"):
            ctx.set_wall_model(1, PARAMS[1], orc.cells, orc.local, orc.sc, orc.sl, sy)
        assert ctx.wall_model_info() == dict(facets=0, launches=0, recomputed=0, law=0)
        # a viscous coefficient of None, nsfem_step_ipcs and nsfem_step_bdf with a model; the context stays usable
        vbc, _ = modelled_floor_bc(dm, marks)
        ctx.set_dirichlet(nat.VELOCITY, *vbc)
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        # (nsfem_set_coeffs itself refuses a viscous coefficient of None, so no call ever sees the law without its nu)
        ctx.set_coeffs(1.0, 1.0, 0.01, 1.0)
        set_model(ctx, orc)
        with pytest.raises(nat.NativeError, match="viscous coefficients are required"):
            ctx.set_coeffs(1.0, 1.0, None, 1.0)
        ctx.set_imex((1.0, -1.0, 0.0), (1.0, 0.0), (1.0, 0.0, 0.0), 1.0 / 16.0)
        assert ctx.step_imex(_opts(ctx)).converged
        assert ctx.wall_model_info()["launches"] == 1
        ctx.set_bdf((1.0, -1.0, 0.0), 1.0 / 16.0)
        with pytest.raises(nat.NativeError, match="wall model: only nsfem_step_imex"):
            ctx.step_ipcs()
        with pytest.raises(nat.NativeError, match="wall model: only nsfem_step_imex"):
            ctx.step_bdf()
        ctx.set_wall_model(0)
        assert ctx.step_ipcs().converged                     # a run without a model goes on as before
    finally:
        ctx.close()


# ---------------------------------------------------------------- 6. through the classes
_SPEC = dict(name="Cavity", mesh=("cube", 2, 8), scheme="ipcs", clock=dict(dt=0.5 / 8, steps=3),
             numbers=dict(Re=100.0), start={"velocity": (0.0, 0.0), "pressure": 0.0},
             bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_normal_flux", "bottom"),
                  ("velocity", "top", (1.0, 0.0))])


def test_solver_class_with_the_hook_equals_driving_the_steps_by_hand(monkeypatch):
    """IMEXIPCSSolver through InstationaryProblem.solve_problem with the set_wall_model hook on the 8 x 8 cavity whose
    floor is modelled and slides, 3 steps: bit for bit what nsfem_set_wall_model / step_imex / advance give through the
    C ABI with the restatement's arrays; ``_compute_wall_model`` returns what the device returns"""
    from grid_generator import HyperCubeBoundaryMarkers
    from multigrid import attach_hierarchy
    from ns_imex_solver import IMEXIPCSSolver
    from problem_specs import build_problem
    from wall_models import ReichardtModel, WallModel
    monkeypatch.setenv("NSFEM_NO_OUTPUT", "1")
    bottom = HyperCubeBoundaryMarkers.bottom.value
    model = WallModel(ReichardtModel(), (bottom, ), ("cell", 0.5), wall_velocity={bottom: (0.5, 0.0)})
    problem = build_problem(dict(_SPEC))

    def set_wall_model(self):
        self._wall_model = model
    type(problem).set_wall_model = set_wall_model
    problem.set_solver_class(IMEXIPCSSolver)
    problem.compute_cfl = False
    problem.solve_problem()
    solver = problem._get_solver()
    steps, dt = _SPEC["clock"]["steps"], _SPEC["clock"]["dt"]
    assert isinstance(solver, IMEXIPCSSolver) and problem._time_stepping.step_number == steps
    mesh, dm, marks = solver._mesh, solver._dofmap, solver._boundary_markers
    cells, local, _ = wm.modelled_facets(mesh, marks, (bottom, ))
    assert solver._ctx.wall_model_info() == dict(facets=cells.size, launches=steps, recomputed=0, law=wm.REICHARDT)
    u_cls, p_cls = solver._ctx.get_state(nat.U1), solver._ctx.get_state(nat.P_OLD)
    out = problem._compute_wall_model()
    rows = solver._ctx.wall_model_facets(nat.U0)
    assert np.array_equal(out["facets"], rows) and abs(out[bottom]["area"] - 1.0) < 1e-14
    assert np.array_equal(out[bottom]["friction_force"], -rows[:, 1:3].sum(axis=0))
    # (the floor drags the fluid along, and the wall stress has no normal part)
    assert out[bottom]["friction_force"][0] > 1e-4 and abs(out[bottom]["friction_force"][1]) < 1e-15
    assert out[bottom]["max_y_plus"] == rows[:, -1].max()
    assert 0.0 < out[bottom]["mean_y_plus"] <= out[bottom]["max_y_plus"] and out[bottom]["mean_u_tau"] > 0.0
    # ---- the same steps through the C ABI on a fresh context, the arrays from the restatement
    orc = wm.WallModelRestatement(mesh, dm, cells, local, wm.REICHARDT, PARAMS[wm.REICHARDT],
                                  solver._equation_coefficients["viscous_term"], ("cell", 0.5),
                                  np.tile([0.5, 0.0], (cells.size, 1)))
    ctx = nat.NsfemContext(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, dm.n_p2, dm.n_p1)
    try:
        if solver._mg_levels is not None:
            attach_hierarchy(ctx, mesh)
        coef = solver._equation_coefficients
        ctx.set_coeffs(coef["convective_term"], coef["pressure_term"], coef["viscous_term"], coef["body_force_term"])
        bd, bv = solver._dirichlet_bcs["velocity"]
        ctx.set_dirichlet(nat.VELOCITY, bd, bv)
        ctx.set_dirichlet(nat.PRESSURE, *solver._dirichlet_bcs["pressure"])
        floor = np.unique(dm.facet_p2_nodes(marks.facets_with_id(bottom)))
        assert np.isin(2 * floor + 1, bd).all() and not np.isin(2 * floor[2:-2], bd).any()
        set_model(ctx, orc)
        opts = solver._step_options()
        ts = IMEXTimeStepping(0.0, 1.0, IMEXType.SBDF2, desired_start_time_step=dt)
        for _ in range(steps):
            ts.update_coefficients()
            ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
            ctx.step_imex(opts)
            ctx.advance(0)
            ts.advance_time()
        assert ctx.get_state(nat.U1).tobytes() == u_cls.tobytes()
        assert ctx.get_state(nat.P_OLD).tobytes() == p_cls.tobytes()
    finally:
        ctx.close()
    solver.set_wall_model(None)
    assert solver._ctx.wall_model_info()["law"] == 0
    with pytest.raises(RuntimeError, match="no wall model"):
        problem._compute_wall_model()
