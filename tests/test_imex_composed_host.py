"""The cache-free composed IMEX definition (tests/imex_composed_host.py) checked without a GPU.

1. Single features reduce to the existing classes.  With exactly one feature on, ComposedIMEX reproduces
   IMEXRestatement, RotatingIMEXRestatement, IMEXPenalRestatement (law, bodies, both) and ScalarIMEXPenalRestatement
   over 4 steps on box(8, 8) and on the (4, 4, 4) cube.  The older classes reuse their N2, the new one recomputes it:
   the sums are the same, only their order differs, so every step vector agrees to 1e-13 of its largest entry (the
   largest difference is printed).
2. Every term is visible in the cases of tests/test_gpu_imex_composed.py: each switched-on term is at least 1e-3 of the
   largest entry of the right-hand side it enters (the ``_effect`` criterion of the bodies module, per term), and every
   pose that is compared with a sharp mask keeps its quadrature points >= 1e-9 away from the surfaces.
3. One failing test per reverted rule.  ``ComposedIMEX.revert`` replaces one rule of the class by the mistake a driver
   could make; test_a_reverted_rule_fails_its_test runs the named check with the rule reverted and expects it to fail:

     rule reverted in the class                                 the test that fails
     ---------------------------------------------------------  -----------------------------------------------------
     "pose"   pose of level n-1 replaced by the pose of n       test_reduces_to_the_penalisation_restatement[box-bodies]
     "omega"  Omega_(n-1) replaced by Omega_n                   test_reduces_to_the_rotating_restatement[box]
     "order"  V added after B                                   test_explicit_vector_has_the_bits_of_v_before_b
     "law"    law of the previous settings kept for level n-1   test_a_law_change_reaches_level_n_minus_1
     "eta_T"  H formed with the flow's eta instead of eta_T     test_reduces_to_the_heated_scalar_restatement[box]
"""
import numpy as np
import pytest

import imex_composed_host as ch
from imex_composed_host import ComposedIMEX
from gpu_common import cavity_bc
from imex_time_stepping import IMEXTimeStepping, IMEXType
from test_gpu_3d import lid_bc
from test_gpu_variable_viscosity import _mesh
from test_heated_bodies_host import ScalarIMEXPenalRestatement, ScalarPenalRestatement
from test_imex_rotation_host import RotatingIMEXRestatement
from test_imex_solver_host import IMEXRestatement
from test_immersed_bodies_host import IMEXPenalRestatement, PenalisationRestatement
from test_scalar_transport_host import smooth_fields
from test_variable_viscosity_host import VariableViscosityRestatement

NO_PBC = (np.zeros(0, np.int64), np.zeros(0))
BOX, CUBE = (8, 8), ch.CUBE
_KINDS = [pytest.param(BOX, id="box"), pytest.param(CUBE, id="cube")]
TOL = 1e-13


def _max_rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def _flow_setup(kind):
    mesh, dm, marks, s, rs, _ = _mesh(kind)
    X = dm.p2_coords
    dim = X.shape[1]
    vbc = cavity_bc(dm, marks) if dim == 2 else lid_bc(dm, marks)
    f = np.stack([np.sin(np.pi * X[:, 1]), -1.0 + X[:, 0], 0.5 * X[:, 1]][:dim], axis=1).ravel()
    u0 = 0.3 * smooth_fields(X)[0]
    return s, rs, dim, vbc, f, u0


def _drive_flow(new, old, vbc, k, per_step=None, steps=4, typ=IMEXType.SBDF2, tag=""):
    """both classes side by side; every step vector (N1, u*, p, u) within TOL of its largest entry"""
    ts = IMEXTimeStepping(0.0, 1.0e9, typ, desired_start_time_step=k)
    worst = 0.0
    for i in range(steps):
        ts.update_coefficients()
        kk = ts.get_next_step_size()
        if per_step is not None:
            per_step(i, ts)
        old.step(ts.alpha, ts.beta, ts.gamma, kk, vbc, NO_PBC)
        new.step(ts.alpha, ts.beta, ts.gamma, kk, vbc, NO_PBC)
        errs = [_max_rel(new.N1, old.N1), _max_rel(new.ustar, old.ustar), _max_rel(new.p, old.p),
                _max_rel(new.vel[0], old.vel[0])]
        worst = max(worst, *errs)
        assert max(errs) < TOL, (tag, i, errs)
        old.advance()
        new.advance()
        ts.advance_time()
    print("%s: largest difference over %d steps %.2e (of the largest entry)" % (tag, steps, worst))
    return worst


def _start(new, old, u0, f):
    for o in (new, old):
        o.vel[0], o.vel[1] = u0.copy(), u0.copy()
        o.body_force = f


# ---------------------------------------------------------------- 1. reductions
@pytest.mark.parametrize("kind,form,traction", [(BOX, "standard", False), (BOX, "skew_symmetric", True),
                                                (BOX, "rotational", False), (BOX, "divergence", True),
                                                (CUBE, "standard", False)], ids=str)
def test_reduces_to_the_plain_restatement(kind, form, traction):
    s, rs, dim, vbc, f, u0 = _flow_setup(kind)
    coef = dict(convective_term=1.0, pressure_term=1.0, viscous_term=0.01, body_force_term=1.0)
    new, old = ComposedIMEX(s, rs, coef, traction), IMEXRestatement(s, coef, form, traction)
    new.form = form
    _start(new, old, u0, f)
    if traction:
        new.traction = old.traction = ch.rhs_fields(s)[4]
    _drive_flow(new, old, vbc, ch.step_size(kind), tag="plain %s %s" % (kind, form))


def _rotating(kind, revert=()):
    s, rs, dim, vbc, f, u0 = _flow_setup(kind)
    new, old = ComposedIMEX(s, rs, ch.STEP_COEF), RotatingIMEXRestatement(s, ch.STEP_COEF, "standard")
    new.revert = set(revert)
    _start(new, old, u0, f)

    def per_step(i, ts):
        w1, w2 = ch.omega_of_time(dim, ts.current_time), ch.omega_of_time(dim, ts.previous_time)
        wd = 0.8 * ch._axis(dim)
        old.w1, old.w2, old.w_dot = w1, w2, wd
        new.set_angular_velocity(ch.omega_of_time(dim, ts.next_time), wd)
        new.set_imex_rotation(1, w1, w2 if i > 0 else None)
    _drive_flow(new, old, vbc, ch.step_size(kind), per_step, tag="rotating %s" % (kind, ))
    assert old.recomputed == 0


@pytest.mark.parametrize("kind", _KINDS)
def test_reduces_to_the_rotating_restatement(kind):
    """Omega(t) = 0.5 + 0.8 t at the two old levels, the Euler term on"""
    _rotating(kind)


def _penalised(kind, what, revert=(), law_change_at=None):
    """``what``: "law", "bodies" (a moving smoothed pair: the older class is handed the pose of t^n before each step
    and keeps the N2 it formed with the pose before) or "both" """
    s, rs, dim, vbc, f, u0 = _flow_setup(kind)
    coef = dict(convective_term=1.0, pressure_term=1.0, viscous_term=0.01, body_force_term=1.0)
    k = ch.step_size(kind)
    new, old = ComposedIMEX(s, rs, coef), IMEXPenalRestatement(s, coef, "standard")
    new.revert = set(revert)
    _start(new, old, u0, f)
    bodies = ch.moving_pair(dim, 2.0 * k, ch.EPS) if what != "law" else None
    if what != "bodies":
        new.set_viscosity_law(ch.SMAGORINSKY, (ch.CS_STEPS, ))
        old.visc = VariableViscosityRestatement(rs, ch.SMAGORINSKY, (ch.CS_STEPS, ))
    if bodies is not None:
        new.set_bodies(bodies, 0.0)

    def per_step(i, ts):
        if bodies is not None:
            new.move_bodies(ts.current_time)
            old.penal = PenalisationRestatement(rs, bodies, ts.current_time)
        if law_change_at == i:
            # (as tests/test_gpu_variable_viscosity.py drives the older class through a change: a new law, N2 dropped)
            new.set_viscosity_law(ch.CARREAU, ch.STEP_LAWS[ch.CARREAU])
            old.visc, old.N2 = VariableViscosityRestatement(rs, ch.CARREAU, ch.STEP_LAWS[ch.CARREAU]), None
    _drive_flow(new, old, vbc, k, per_step, tag="penalised %s %s" % (kind, what))
    return new, old


@pytest.mark.parametrize("kind,what", [pytest.param(BOX, "law", id="box-law"), pytest.param(BOX, "bodies", id="box-bodies"),
                                       pytest.param(BOX, "both", id="box-both"), pytest.param(CUBE, "both", id="cube-both")])
def test_reduces_to_the_penalisation_restatement(kind, what):
    _penalised(kind, what)


def _law_change(revert=()):
    _penalised(BOX, "law", revert, law_change_at=2)


def test_a_law_change_reaches_level_n_minus_1():
    """Smagorinsky -> Carreau before step 3: N(u2) of that step is formed with the Carreau law"""
    _law_change()


def _order(revert=()):
    s, rs, dim, vbc, f, u0 = _flow_setup(BOX)
    coef = dict(convective_term=1.0, pressure_term=1.0, viscous_term=0.01, body_force_term=1.0)
    bodies = ch.moving_pair(dim, 0.1, ch.EPS)
    new = ComposedIMEX(s, rs, coef)
    new.revert = set(revert)
    new.set_viscosity_law(ch.SMAGORINSKY, (0.9, ))
    new.set_bodies(bodies, 0.0)
    old = IMEXPenalRestatement(s, coef, "standard", visc=VariableViscosityRestatement(rs, ch.SMAGORINSKY, (0.9, )),
                               penal=PenalisationRestatement(rs, bodies, 0.0))
    u = smooth_fields(s.p2_nodes())[0]
    assert np.array_equal(new.explicit(u, 0), old.explicit(u))


def test_explicit_vector_has_the_bits_of_v_before_b():
    """(c_c conv + V) + B, the order of IMEXPenalRestatement and of the device's launches: bit for bit"""
    _order()


def _heated(kind, revert=()):
    """transport steps with a fixed smooth velocity and the heated moving pair, eta_T != eta"""
    mesh, dm, marks, s, rs, _ = _mesh(kind)
    X = dm.p2_coords
    dim = X.shape[1]
    k = ch.step_size(kind)
    u, T_init = smooth_fields(X)
    bodies = ch.heated_pair(dim, 2.0 * k, ch.EPS, 1.5 * k)
    new = ComposedIMEX(s, rs, ch.STEP_COEF)
    new.revert = set(revert)
    old = ScalarIMEXPenalRestatement(s, ch.KAPPA, "standard")
    new.set_scalar(ch.KAPPA, None, 0)
    new.set_bodies(bodies, 0.0)
    new.set_body_temperatures(*bodies.temperatures(), bodies.eta_scalar)
    q = np.cos(2.0 * X[:, 0] + 0.3) * np.sin(1.5 * X[:, 1] + 0.2)
    new.source = old.source = q
    new.vel = [u.copy(), u.copy(), u.copy()]
    for o in (new, old):
        o.T[0], o.T[1] = T_init.copy(), T_init.copy()
    left = np.unique(dm.facet_p2_nodes(marks.facets_with_id(1)))
    tbc = (left, 0.5 + X[left, 1])
    ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=k)
    worst = 0.0
    for i in range(4):
        ts.update_coefficients()
        kk = ts.get_next_step_size()
        new.move_bodies(ts.current_time)
        old.penal = ScalarPenalRestatement(rs, bodies, ts.current_time)
        old.step(ts.alpha, ts.beta, ts.gamma, kk, u, u, tbc)
        new.step_scalar(ts.alpha, ts.beta, ts.gamma, kk, tbc)
        errs = [_max_rel(new.TN1, old.N1), _max_rel(new.T[0], old.T[0])]
        worst = max(worst, *errs)
        assert max(errs) < TOL, (kind, i, errs)
        old.advance()
        new.T[2], new.T[1] = new.T[1].copy(), new.T[0].copy()
        ts.advance_time()
    print("heated scalar %s: largest difference over 4 steps %.2e (of the largest entry)" % (kind, worst))


@pytest.mark.parametrize("kind", _KINDS)
def test_reduces_to_the_heated_scalar_restatement(kind):
    _heated(kind)


# ---------------------------------------------------------------- 3. one failing test per reverted rule
@pytest.mark.parametrize("rule,check", [("pose", lambda r: _penalised(BOX, "bodies", r)),
                                        ("omega", lambda r: _rotating(BOX, r)),
                                        ("order", _order),
                                        ("law", _law_change),
                                        ("eta_T", lambda r: _heated(BOX, r))], ids=lambda x: x if isinstance(x, str) else "")
def test_a_reverted_rule_fails_its_test(rule, check):
    """the body of the named test (module docstring) with the one rule reverted inside the class"""
    assert rule in ch.RULES
    with pytest.raises(AssertionError):
        check((rule, ))


def test_a_vouched_vector_is_used_for_one_step_only():
    """the one exception to "no stored vector": vouch_N2 / vouch_TN2 replace level n-1's vector until the advance"""
    s, rs, dim, vbc, f, u0 = _flow_setup(BOX)
    h = ComposedIMEX(s, rs, ch.STEP_COEF)
    h.vel[1], h.vel[2] = u0.copy(), 0.9 * u0
    h.T[1], h.T[2] = smooth_fields(s.p2_nodes())[1], 0.8 * smooth_fields(s.p2_nodes())[1]
    fresh = h.rhs(*ch.SBDF2_LATER, 0.1)
    fresh_T = h.scalar_rhs(*ch.SBDF2_LATER, 0.1)
    v, vT = np.ones_like(u0), np.ones(s.n2)
    h.vouch_N2(v)
    h.vouch_TN2(vT)
    assert np.allclose(h.rhs(*ch.SBDF2_LATER, 0.1) - fresh, -ch.SBDF2_LATER[1][1] * (v - h.explicit(h.vel[2], 1)))
    assert np.allclose(h.scalar_rhs(*ch.SBDF2_LATER, 0.1) - fresh_T,
                       -ch.SBDF2_LATER[1][1] * (vT - h.scalar_explicit(h.vel[2], h.T[2], 1)))
    h.advance()
    T = smooth_fields(s.p2_nodes())[1]
    h.vel[1], h.vel[2], h.T[1], h.T[2] = u0.copy(), 0.9 * u0, T, 0.8 * T
    assert np.array_equal(h.rhs(*ch.SBDF2_LATER, 0.1), fresh)
    assert np.array_equal(h.scalar_rhs(*ch.SBDF2_LATER, 0.1), fresh_T)


# ---------------------------------------------------------------- 2. visibility and clearance of the GPU cases
VISIBLE = 1e-3


def _bracket_parts(h):
    """the mass-weighted members of the bracket and the traction vector, one by one"""
    c, parts = h.c, {}
    if h.body_force is not None:
        parts["body force"] = c["body_force_term"] * (h.M @ h.body_force)
    if h.buoyancy is not None:
        parts["buoyancy"] = c["body_force_term"] * (h.M @ np.outer(h.T[0], h.buoyancy).ravel())
    saved = h.body_force, h.buoyancy
    h.body_force = h.buoyancy = None
    euler = h.bracket()
    h.body_force, h.buoyancy = saved
    if euler is not None:
        parts["euler"] = h.M @ euler
    if h.traction is not None:
        parts["traction"] = h.traction
    return parts


@pytest.mark.parametrize("traction", (False, True), ids=("laplace", "traction-form"))
@pytest.mark.parametrize("kind", ch.RHS_MESHES, ids=str)
def test_every_term_of_the_right_hand_side_cases_is_visible(kind, traction):
    mesh, dm, marks, s, rs, _ = _mesh(kind)
    for name, bodies in ch.rhs_body_sets(kind):
        for form_id in range(4):
            h = ch.rhs_case(s, rs, kind, form_id, traction, bodies)
            full, parts, n1_parts = ch.rhs_parts(h, *ch.SBDF2_LATER, ch.RHS_K)
            assert set(n1_parts) == {"convection", "coriolis", "viscosity", "bodies"}
            parts.update(_bracket_parts(h))
            assert {"body force", "euler"} <= set(parts) and ("traction" in parts) == traction
            big, big1 = np.abs(full).max(), np.abs(h.N1).max()
            share = {k: float(np.abs(v).max() / big) for k, v in parts.items()}
            share1 = {k: float(np.abs(v).max() / big1) for k, v in n1_parts.items()}
            print(kind, name, form_id, traction, {k: "%.1e" % v for k, v in share.items()})
            assert min(share.values()) >= VISIBLE and min(share1.values()) >= VISIBLE, (share, share1)
            # the two levels differ in pose and Omega: a vector formed with the wrong level's setting shows
            for rule in ("pose", "omega"):
                h.revert = {rule}
                assert _max_rel(h.rhs(*ch.SBDF2_LATER, ch.RHS_K), full) >= VISIBLE, rule
                h.revert = set()
            if bodies.smoothing == 0.0:
                for level in (0, 1):
                    assert h._penal(level).surface_clearance() >= 1e-9


_STEP_CASES = [((8, 8), t) for t in (IMEXType.SBDF2, IMEXType.CNAB, IMEXType.mCNAB)] + \
              [((16, 16), t) for t in (IMEXType.SBDF2, IMEXType.CNAB, IMEXType.mCNAB)] + \
              [("mapped", IMEXType.SBDF2), (CUBE, IMEXType.SBDF2)]


@pytest.mark.parametrize("kind,typ", _STEP_CASES, ids=lambda x: x.name if isinstance(x, IMEXType) else str(x))
def test_every_term_of_the_step_cases_is_visible(kind, typ):
    """the run of the GPU module's step tests (and the start of its event sequences) on the host alone: in the last of
    the 4 steps every explicit term, the body force, the buoyancy and the Euler term reach VISIBLE of the flow's
    right-hand side, and convection and heating that of the scalar's"""
    run = ch.ComposedRun(kind, typ, _mesh(kind))
    for i in range(4):
        if i == 2:
            run.apply("dk")
        if i == 3:
            h = run.h
            saved = [v.copy() for v in h.vel], [v.copy() for v in h.T], h.p_old.copy()
        run.step()
    h = run.h
    alpha, beta, gamma, kk = run.coefficients
    assert beta[1] != 0.0
    T0 = h.T[1].copy()                                    # (what the last flow step saw as T^(n+1))
    h.vel, h.T, h.p_old = saved[0], saved[1], saved[2]
    srhs = h.scalar_rhs(alpha, beta, gamma, kk)
    sparts = {}
    t2 = dict(h.scalar_terms(h.vel[2], h.T[2], 1))
    for name, v in h.scalar_terms(h.vel[1], h.T[1], 0):
        sparts[name] = beta[0] * v + beta[1] * t2[name]
    h.T[0] = T0
    full, parts, n1_parts = ch.rhs_parts(h, alpha, beta, gamma, kk)
    parts.update(_bracket_parts(h))
    share = {k: float(np.abs(v).max() / np.abs(full).max()) for k, v in parts.items()}
    sshare = {k: float(np.abs(v).max() / np.abs(srhs).max()) for k, v in sparts.items()}
    print(kind, typ.name, {k: "%.1e" % v for k, v in share.items()}, {k: "%.1e" % v for k, v in sshare.items()})
    assert set(share) == {"convection", "coriolis", "viscosity", "bodies", "operators", "body force", "buoyancy", "euler"}
    assert set(sshare) == {"convection", "heat"}
    assert min(share.values()) >= VISIBLE and min(sshare.values()) >= VISIBLE, (share, sshare)
