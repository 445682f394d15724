"""The composed IMEX step on the GPU -- every explicit term of nsfem_step_imex / nsfem_step_scalar_imex / nsfem_imex_rhs at
once, and the bookkeeping of the two stored vectors under every change of a setting -- against the cache-free host
definition of tests/imex_composed_host.py (ComposedIMEX: no stored vector, both levels formed afresh from the
settings in every step).  Cases, fields and events are defined there; tests/test_imex_composed_host.py shows without a
GPU that every term is visible in them and that the definition fails its own tests when one of its rules is reverted.

a. Right-hand sides with everything on (nsfem_imex_rhs): all four convective forms x traction form off / on on
   box(8, 8), box(16, 16), the mapped box and the (4, 4, 4) cube; Omega_n != Omega_(n-1), dOmega/dt != 0, a law
   (Smagorinsky / Carreau alternating), the moving smoothed "overlap" pair (plus the sharp moving disc on the boxes),
   a body force, SBDF2 coefficients with b1 != 0.  Tolerance: the sum over the switched-on parts of (the project's bound
   for the part) x (its largest entry on the host), divided by the largest entry of the composed vector -- 1e-13 for
   operator and element terms, min(10 x 1.25e-15, 1e-11) for smoothed masks (tests/test_gpu_immersed_bodies.py).
   Where the one-launch lattice kernel exists it equals the generic path bit for bit in both outputs.
b. Steps with everything on: flow and scalar step per time step, Boussinesq coupling, a heated moving disc and a
   passive box, rotation varying in time, a law, the step size halved before step 3; u*, u 1e-9, p minus its mean
   1e-8 (tests/test_gpu_imex.py), T 1e-9 (tests/test_gpu_scalar_transport.py).
c. Bookkeeping under change: 8-step sequences with one event after step 5 (every entry of EVENTS), and six seeded
   sequences with two events in every gap.  After every step the device is held to the host at the tolerances of (b),
   and the counters of the five info calls to CacheModel below -- the rule "recompute iff a key changed", stated once
   outside the C++.  A twin context gets the same calls plus set_state(U2, get_state(U2)) and set_state(T2,
   get_state(T2)) before every step, so it recomputes both stored vectors in every step.
   Flow side: CONV_N1, USTAR, U0 and P of the twins are bit-identical -- a stored and a recomputed N(u2) are the same
   launches in the same order.  Scalar side: the stored vector carries the weight b0' of the step that formed it and is
   rescaled by b1 / b0', the fresh one is formed with weight 1, so the two are no bit copies by construction (they are
   where b0' is a power of two); T0 of the twins is held to the element-vector bound 1e-13 of the largest entry
   instead.  So that the flow comparison stays one of the flow's own launches, the twin's T0 is overwritten with the
   first context's after the scalar comparison (T0 enters the flow through the buoyancy, and the next levels).
d. BoussinesqIMEXSolver with a viscosity model, moving heated bodies and an angular velocity at once equals the same
   calls made by hand through the C ABI, bit for bit.

Measured on the MI355X (largest over the cases; every case prints its own figures):
    a. 48 right-hand sides: rhs 1.29e-15 of the largest entry (smallest bound over the cases 1.11e-13), N1 1.05e-15
       (smallest bound 2.74e-14); the largest error / bound is 0.03; lattice = generic bit for bit in the 8 cases
       that have the kernel.
    b. / c. 438 scalar and 448 flow steps: T 1.16e-12, u* 1.09e-11, u 1.12e-11, p minus its mean 3.16e-12.
    c. twins: flow side bit-identical in every step; T0 differs by at most 2.96e-16 of the largest entry (0 wherever
       b0' = 2, as in SBDF2 with uniform steps; nonzero only after a step-size change).  All counter predictions held.
    Times: 69 tests in 20.8 s; the slowest are the three on the (4, 4, 4) cube (1.1 - 1.6 s, most of it the host's 3D
    assembly), a sequence of 8 steps with its twin takes 0.15 s on box(8, 8) and 0.4 s on box(16, 16).

That the module can fail: five libraries built with one line of the driver (csrc/api.hip) changed each, each run once
against this module and once against the six older IMEX feature modules (test_gpu_imex, _imex_rotation,
_variable_viscosity, _immersed_bodies, _scalar_transport, _heated_bodies; 271 tests):
    one-line change                                                   this module    the six older modules
    visc dropped from ImexKey::serves (the step's ``stored`` test)    12 of 69 fail  1 of 271 fails (viscosity: stored vector)
    gam dropped from ImexKey::serves                                   8 of 69 fail  6 of 271 fail (rotating cavity steps)
    bodies.cur for bodies.prev where the step forms N(u2) afresh      52 of 69 fail  0 of 271 fail
    body dropped from Scalar::Key::same_heat                          12 of 69 fail  1 of 271 fails (heated bodies: epoch)
    V and B swapped after imex_rhs in the step                        50 of 69 fail  0 of 271 fail
(The runs were made when the driver spelled these lines out in the step itself; the comparisons now live in the two
keys of csrc/nsfem_internal.hpp, the order of V and B and the pose of a level in imex_explicit_add of csrc/api.hip.)
The first, second and fourth fail in the sequences whose events move the dropped key (values against the host at 1e-2,
or the counters where the vector happens to be the same); the third and fifth fail wherever the twin recomputes --
the two mistakes the older modules cannot see, because no older test recomputes N(u2) with a moved pose in a step, and
none compares a stored with a recomputed vector bit for bit with a law and bodies set.
"""
import numpy as np
import pytest

import _native as nat
import imex_composed_host as ch
from gpu_common import cavity_bc, rel
from imex_time_stepping import IMEXTimeStepping, IMEXType
from test_gpu_3d import lid_bc
from test_gpu_variable_viscosity import _mesh

pytestmark = pytest.mark.gpu

NO_PBC = (np.zeros(0, np.int32), np.zeros(0))
ELEMENT_BOUND = 1e-13
SMOOTH_BOUND = min(10.0 * 1.25e-15, 1e-11)
_PATH = {(8, 8): "generic", (16, 16): "lattice-kernel", "mapped": "generic", ch.CUBE: "generic"}


def _max_rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


# ---------------------------------------------------------------- a. right-hand sides with everything on
def _composed_bound(parts, smoothed):
    """sum of the parts' bounds times their largest entries, over the largest entry of the sum"""
    total = sum(parts.values())
    bound = sum((SMOOTH_BOUND if (name == "bodies" and smoothed) else ELEMENT_BOUND) * np.abs(v).max()
                for name, v in parts.items())
    return float(bound / np.abs(total).max())


@pytest.mark.parametrize("traction", (False, True), ids=("laplace", "traction-form"))
@pytest.mark.parametrize("kind", ch.RHS_MESHES, ids=str)
def test_right_hand_sides_with_everything_on(kind, traction):
    mesh, dm, marks, s, rs, make = _mesh(kind)
    bd, bv = cavity_bc(dm, marks) if s.dim == 2 else lid_bc(dm, marks)
    free = np.ones(s.dim * s.n2, dtype=bool)              # (the hook returns no Dirichlet rows: compare the others)
    free[bd] = False
    lattice = kind == (16, 16) and not traction
    ctx = make(mesh, dm)
    worst = 0.0
    try:
        ctx.set_dirichlet(nat.VELOCITY, bd.astype(np.int32), bv)
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        for name, bodies in ch.rhs_body_sets(kind):
            for form_id in range(4):
                h = ch.rhs_case(s, rs, kind, form_id, traction, bodies, ctx, nat)
                full, parts, n1_parts = ch.rhs_parts(h, *ch.SBDF2_LATER, ch.RHS_K)
                tol, tol1 = _composed_bound(parts, bodies.smoothing > 0.0), _composed_bound(n1_parts, bodies.smoothing > 0.0)
                got, n1 = ctx.imex_rhs("generic", form_id)
                err = float(np.abs(got - full)[free].max() / np.abs(full[free]).max())
                err1 = _max_rel(n1, h.N1)
                worst = max(worst, err / tol, err1 / tol1)
                print("%s %s form %d traction %d law %d: rhs %.2e (bound %.2e)  N1 %.2e (bound %.2e)" % (
                    kind, name, form_id, traction, h.law, err, tol, err1, tol1))
                assert err < tol and err1 < tol1, (name, form_id, err, tol, err1, tol1)
                if lattice:
                    l_rhs, l_n1 = ctx.imex_rhs("lattice-kernel", form_id)
                    assert np.array_equal(l_rhs, got), (name, form_id, np.abs(l_rhs - got).max())
                    assert np.array_equal(l_n1, n1), (name, form_id, np.abs(l_n1 - n1).max())
                else:
                    with pytest.raises(nat.NativeError, match="not available"):
                        ctx.imex_rhs("lattice-kernel", form_id)
        print("%s traction %d: largest error / bound %.2f" % (kind, traction, worst))
    finally:
        ctx.close()


# ---------------------------------------------------------------- the comparison of a step
def _check(tag):
    def check(run, what):
        h, ctx = run.h, run.ctxs[0]
        if what == "scalar":
            assert all(si.converged for si in run.infos)
            et = rel(ctx.get_state(nat.T0), h.T[0])
            print("%s step %d: T %.2e" % (tag, run.step_index, et))
            assert et < 1e-9, (tag, run.step_index, et)
            return
        us, u, p = ctx.get_state(nat.USTAR), ctx.get_state(nat.U0), ctx.get_state(nat.P)
        es, eu, ep = rel(us, h.ustar), rel(u, h.vel[0]), rel(p - p.mean(), h.p - h.p.mean())
        print("%s step %d: u* %.2e u %.2e p %.2e path %s" % (tag, run.step_index, es, eu, ep, ctx.imex_info()["path"]))
        assert es < 1e-9 and eu < 1e-9 and ep < 1e-8, (tag, run.step_index, es, eu, ep)
    return check


# ---------------------------------------------------------------- b. steps with everything on
_STEP_CASES = [((8, 8), t) for t in (IMEXType.SBDF2, IMEXType.CNAB, IMEXType.mCNAB)] + \
              [((16, 16), t) for t in (IMEXType.SBDF2, IMEXType.CNAB, IMEXType.mCNAB)] + \
              [("mapped", IMEXType.SBDF2), (ch.CUBE, IMEXType.SBDF2)]


@pytest.mark.parametrize("kind,typ", _STEP_CASES, ids=lambda x: x.name if isinstance(x, IMEXType) else str(x))
def test_steps_with_everything_on(kind, typ):
    mesh_tuple = _mesh(kind)
    ctx = mesh_tuple[5](mesh_tuple[0], mesh_tuple[1])
    try:
        model = CacheModel()
        run = ch.ComposedRun(kind, typ, mesh_tuple, [ctx], nat, model)
        check = _check("%s %s" % (kind, typ.name))
        for i in range(4):
            if i == 2:
                run.apply("dk")
            run.step(check=check)
            model.compare(ctx, (kind, typ.name, i))
        info = ctx.imex_info()
        assert info["path"] == _PATH[kind], info
        assert info["lattice_rhs" if _PATH[kind] == "lattice-kernel" else "generic_rhs"] == 4, info
        # nothing was recomputed: every key either stood still or moved with its level
        assert model.count["visc_recomputed"] == model.count["body_recomputed"] == model.count["rot_recomputed"] == 0
        assert model.count["thermal_recomputed"] == 0 and model.count["scalar_reuses"] == 3
    finally:
        ctx.close()


# ---------------------------------------------------------------- c. bookkeeping under change
class CacheModel:
    """The validity rule of the two stored vectors, stated once outside the C++: a stored vector is reused iff it is
    valid (it belongs to the level: formed in the step before, no level rewritten since) and no key moved since it
    was formed.  Keys of N(u2): convective form, c_c, changes of the law, changes of the body set, 2 c_cor
    Omega(t^(n-1)).  Keys of the scalar's vector: scalar form, changes of the thermal data a kernel sees, and -- while
    a body is thermal -- changes of the body set.  ``count`` predicts the counters of the info calls."""

    def __init__(self):
        self.count = dict.fromkeys(("visc_launches", "visc_recomputed", "body_launches", "body_recomputed", "rot_rhs",
                                    "rot_recomputed", "scalar_launches", "scalar_reuses", "fused_launches",
                                    "thermal_recomputed"), 0)
        self.law, self.tables, self.seen, self.n_thermal = (0, ()), (None, None), None, 0
        self.epoch = dict(law=0, bodies=0, thermal=0)
        self.flow = dict(valid=False, fresh=False, key=None)
        self.scalar = dict(valid=False, fresh=False, key=None)

    def __call__(self, action, *args):
        getattr(self, "on_" + action)(*args)

    def on_law(self, law, params):
        self.epoch["law"] += (law, tuple(params)) != self.law
        self.law = (law, tuple(params))

    def on_set_bodies(self, table):
        self.epoch["bodies"] += self.tables != (table, table)
        self.tables = (table, table)

    def on_move(self, table):
        self.tables = (table, self.tables[0])              # (moves no key: the stored vector was formed with the pose
        #                                                     that is now the older one)

    def on_thermal(self, flags, values, eta_T, n_thermal):
        seen = (flags, values, eta_T) if n_thermal else None
        self.epoch["thermal"] += seen != self.seen
        self.seen, self.n_thermal = seen, n_thermal

    def on_set_state(self, name):
        if name == "u1":
            self.flow["fresh"] = self.scalar["fresh"] = False
        if name == "u2":
            self.flow["valid"] = False
        if name in ("u2", "t2"):
            self.scalar["valid"] = False

    def on_flow_step(self, b1, form, cc, gam_n, gam_nm1):
        c, key = self.count, (form, cc, self.epoch["law"], self.epoch["bodies"])
        law = self.law[0] != 0
        if b1 != 0.0 and not (self.flow["valid"] and self.flow["key"] == key + (gam_nm1, )):
            c["visc_launches"] += law
            c["visc_recomputed"] += law
            c["body_launches"] += 1
            c["body_recomputed"] += 1
            c["rot_recomputed"] += self.flow["valid"]      # (counts a recomputation of a vector that was there)
        c["visc_launches"] += law
        c["body_launches"] += 1
        c["rot_rhs"] += 1
        self.flow.update(fresh=True, key=key + (gam_n, ))

    def on_scalar_step(self, b1, form):
        c, heated = self.count, self.n_thermal > 0
        key = (form, self.epoch["thermal"], self.epoch["bodies"])
        if b1 != 0.0:
            old = self.scalar["key"]
            usable = self.scalar["valid"] and old[0] == form
            if usable and old[1] == key[1] and (not heated or old[2] == key[2]):
                c["scalar_reuses"] += 1
            else:
                c["thermal_recomputed"] += usable
                c["fused_launches"] += heated
                c["scalar_launches"] += 1
        c["fused_launches"] += heated
        c["scalar_launches"] += 1
        self.scalar.update(fresh=True, key=key)

    def on_advance(self):
        for v in (self.flow, self.scalar):
            v.update(valid=v["fresh"], fresh=False)

    def compare(self, ctx, tag):
        c = self.count
        v, b, r = ctx.viscosity_info(), ctx.body_info(), ctx.imex_rotation_info()
        sc, hi = ctx.scalar_info(), ctx.body_heat_info()
        got = dict(visc_launches=v["element_launches"], visc_recomputed=v["recomputed"],
                   body_launches=b["element_launches"], body_recomputed=b["recomputed"], rot_rhs=r["rotating_rhs"],
                   rot_recomputed=r["recomputed"], scalar_launches=sc["convection_launches"],
                   scalar_reuses=sc["convection_reuses"], fused_launches=hi["fused_launches"],
                   thermal_recomputed=hi["recomputed"])
        assert got == c, (tag, {k: (got[k], c[k]) for k in c if got[k] != c[k]})
        assert hi["thermal"] == self.n_thermal and v["law"] == self.law[0], tag


class _Both:
    """the observer of a run with a twin: both models hear every call"""

    def __init__(self):
        self.first, self.twin = CacheModel(), CacheModel()

    def __call__(self, action, *args):
        self.first(action, *args)
        self.twin(action, *args)


_FLOW_SLOTS = (("CONV_N1", nat.CONV_N1), ("USTAR", nat.USTAR), ("U0", nat.U0), ("P", nat.P))


def _run_sequence(kind, gaps, tag):
    """8 SBDF2 steps; ``gaps[i]``: the events between step i and step i + 1 (1-based steps; "u1" before the advance,
    the others after it)"""
    mesh_tuple = _mesh(kind)
    ctx = mesh_tuple[5](mesh_tuple[0], mesh_tuple[1])
    twin = None
    try:
        twin = mesh_tuple[5](mesh_tuple[0], mesh_tuple[1])
        models = _Both()
        run = ch.ComposedRun(kind, IMEXType.SBDF2, mesh_tuple, [ctx, twin], nat, models)
        check = _check(tag)
        worst_T = [0.0]

        def before_step(run):
            for name, slot in (("u2", nat.U2), ("t2", nat.T2)):
                twin.set_state(slot, twin.get_state(slot))
                models.twin("set_state", name)

        def check_both(run, what):
            check(run, what)
            if what == "scalar":
                T0, T0_twin = ctx.get_state(nat.T0), twin.get_state(nat.T0)
                worst_T[0] = max(worst_T[0], _max_rel(T0_twin, T0))
                assert _max_rel(T0_twin, T0) < ELEMENT_BOUND, (tag, run.step_index, _max_rel(T0_twin, T0))
                twin.set_state(nat.T0, T0)                 # (the flow twins get the same buoyancy; docstring c)
                return
            for name, slot in _FLOW_SLOTS:
                assert np.array_equal(ctx.get_state(slot), twin.get_state(slot)), (tag, run.step_index, name)

        for i in range(8):
            events = gaps.get(i + 1, ())
            run.step(before_step, check_both, pre_advance=[e for e in events if e == "u1"])
            models.first.compare(ctx, (tag, i, "first"))
            models.twin.compare(twin, (tag, i, "twin"))
            for e in events:
                if e != "u1":
                    run.apply(e)
        print("%s: twins' T0 differ by at most %.2e (of the largest entry)" % (tag, worst_T[0]))
        assert ctx.imex_info()["path"] == _PATH[kind]
        return models.first.count
    finally:
        ctx.close()
        if twin is not None:
            twin.close()


#: recomputations the event costs the first context over the 8 steps, as (N(u2) recomputed, the scalar's vector
#: recomputed although usable, N(u2) recomputed while a vector was there).  Levels rewritten by hand (u2, u1) drop the
#: flow's vector, so the third count stays; t2, ns and a changed scalar form drop the scalar's vector (no count, seen
#: in the launches); without Omega levels the context's single Omega moves every step, and so does the key (wn)
_EXPECT = {"lp": (1, 0, 1), "l2": (1, 0, 1), "l0": (1, 0, 1), "w2": (1, 0, 1), "cc": (1, 0, 1), "cf": (1, 0, 1),
           "be": (1, 1, 1), "bs": (1, 1, 1), "pb": (1, 1, 1), "ts": (0, 1, 0), "wn": (3, 0, 3), "u2": (1, 0, 0),
           "u1": (1, 0, 0), "mv": (0, 0, 0), "tt": (0, 0, 0), "wg": (0, 0, 0), "dk": (0, 0, 0), "sf": (0, 0, 0),
           "t2": (0, 0, 0), "ns": (0, 0, 0)}


@pytest.mark.parametrize("event", list(ch.EVENTS))
@pytest.mark.parametrize("kind", [(8, 8), (16, 16)], ids=str)
def test_one_event_between_two_steps(kind, event):
    """everything on, one event between steps 5 and 6 ("u1": after step 5, before its advance); _EXPECT pins what the
    event costs, so the model cannot drift along with the device"""
    count = _run_sequence(kind, {5: (event, )}, "%s %s" % (kind, event))
    assert (count["body_recomputed"], count["thermal_recomputed"], count["rot_recomputed"]) == _EXPECT[event], count
    assert count["visc_recomputed"] == count["body_recomputed"]


def _draw(seed):
    rng = np.random.default_rng(seed)
    codes = list(ch.EVENTS)
    return {gap: tuple(codes[j] for j in rng.integers(0, len(codes), 2)) for gap in range(1, 8)}


_SEEDED = [(seed, _draw(seed)) for seed in (11, 12, 13, 14, 15, 16)]


@pytest.mark.parametrize("seed,gaps", _SEEDED,
                         ids=["seed%d-%s" % (s, ".".join("+".join(g[i]) for i in range(1, 8))) for s, g in _SEEDED])
@pytest.mark.parametrize("kind", [(8, 8), (16, 16)], ids=str)
def test_two_events_in_every_gap(kind, seed, gaps):
    _run_sequence(kind, gaps, "%s seed %d" % (kind, seed))


# ---------------------------------------------------------------- d. through the classes
_SPEC = dict(name="RotatingCavity", mesh=("cube", 2, 8), scheme="ipcs", clock=dict(dt=0.5 / 8, steps=3),
             numbers=dict(Re=100.0, Fr=1.0, Ro=0.5), start={"velocity": (0.0, 0.0), "pressure": 0.0, "temperature": 0.5},
             spin=("ramp", 10.0, 0.8),
             bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_slip", "bottom"), ("velocity", "top", (1.0, 0.0))])


def test_boussinesq_solver_with_everything_equals_driving_the_steps_by_hand(monkeypatch):
    """BoussinesqIMEXSolver through InstationaryProblem.solve_problem on the 8 x 8 cavity with a Smagorinsky model, a
    heated disc that moves and a passive box, and the angular velocity Omega(t) = 0.8 t, 3 steps: bit for bit what
    set_viscosity_law / set_bodies / set_body_temperatures / move_bodies / set_angular_velocity / set_imex_rotation /
    step_scalar_imex / step_imex / advance give through the C ABI"""
    from immersed_bodies import Ball, Box, ImmersedBodies
    from multigrid import attach_hierarchy
    from ns_boussinesq_solver import BoussinesqIMEXSolver
    from problem_specs import build_problem
    from viscosity_models import SmagorinskyModel
    monkeypatch.setenv("NSFEM_NO_OUTPUT", "1")
    steps, dt, rate = _SPEC["clock"]["steps"], _SPEC["clock"]["dt"], _SPEC["spin"][2]
    disc = Ball((0.4, 0.7), 0.15, motion=lambda t: ((0.4 + 0.3 * t, 0.7), (0.3, 0.0), 0.0), temperature=1.5)
    bodies = ImmersedBodies([disc, Box((0.5, 0.25), (0.2, 0.1))], 2.0 * dt, 0.05, eta_scalar=1.5 * dt)
    problem = build_problem(dict(_SPEC))
    cls = type(problem)

    def set_immersed_bodies(self):
        self._immersed_bodies = bodies
        self._immersed_allow_stiff = False

    def set_temperature_coefficients(self):
        self._temperature_coefficients = dict(diffusivity=0.05, buoyancy=(0.0, 1.0), convective_form="standard")

    def set_temperature_boundary_conditions(self):
        self._temperature_bcs = [(self._sides["left"], 1.0), (self._sides["right"], 0.0)]

    def set_viscosity_model(self):
        self._viscosity_model = SmagorinskyModel(ch.CS_STEPS)
    cls.set_immersed_bodies = set_immersed_bodies
    cls.set_temperature_coefficients = set_temperature_coefficients
    cls.set_temperature_boundary_conditions = set_temperature_boundary_conditions
    cls.set_viscosity_model = set_viscosity_model
    problem.set_solver_class(BoussinesqIMEXSolver)
    problem.compute_cfl = False
    problem.solve_problem()
    solver = problem._get_solver()
    assert isinstance(solver, BoussinesqIMEXSolver) and problem._time_stepping.step_number == steps
    sctx = solver._ctx
    assert sctx.viscosity_info() == dict(law=1, element_launches=steps, recomputed=0)
    assert sctx.body_info() == dict(bodies=2, element_launches=steps, recomputed=0)
    assert sctx.body_heat_info() == dict(thermal=1, fused_launches=steps, recomputed=0)
    assert sctx.imex_rotation_info() == dict(treatment=1, rotating_rhs=steps - 1, recomputed=0)   # (Omega(0) = 0)
    fields = (nat.T1, nat.U1, nat.P_OLD)
    got = [sctx.get_state(slot) for slot in fields]
    # ---- the same steps through the C ABI on a fresh context
    dm, mesh = solver._dofmap, solver._mesh
    left = np.unique(dm.facet_p2_nodes(solver._boundary_markers.facets_with_id(problem._sides["left"])))
    right = np.unique(dm.facet_p2_nodes(solver._boundary_markers.facets_with_id(problem._sides["right"])))
    ctx = nat.NsfemContext(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, dm.n_p2, dm.n_p1)
    try:
        if solver._mg_levels is not None:
            attach_hierarchy(ctx, mesh)
        coef = solver._equation_coefficients
        ctx.set_coeffs(coef["convective_term"], coef["pressure_term"], coef["viscous_term"], coef["body_force_term"],
                       coef["coriolis_term"], coef["euler_term"])
        bd, bv = solver._dirichlet_bcs["velocity"]
        ctx.set_dirichlet(nat.VELOCITY, np.asarray(bd, np.int32), np.asarray(bv, float))
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        ctx.set_dirichlet(nat.SCALAR, np.concatenate([left, right]),
                          np.concatenate([np.ones(left.size), np.zeros(right.size)]))
        ctx.set_scalar(0.05, (0.0, 1.0), 0)
        for slot in (nat.T0, nat.T1):
            ctx.set_state(slot, np.full(dm.n_p2, 0.5))
        ctx.set_viscosity_law(1, (ch.CS_STEPS, ))
        ctx.set_bodies(bodies.rows(0.0), bodies.eta, bodies.smoothing)
        ctx.set_body_temperatures(*bodies.temperatures(), bodies.eta_scalar)
        opts = solver._step_options()
        ts = IMEXTimeStepping(0.0, 1.0, IMEXType.SBDF2, desired_start_time_step=dt)
        for step in range(steps):
            ts.update_coefficients()
            ctx.set_angular_velocity(rate * ts.current_time, rate)
            ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
            ctx.set_imex_rotation(1, rate * ts.current_time, rate * ts.previous_time if step > 0 else None)
            ctx.move_bodies(bodies.rows(ts.current_time))
            ctx.step_scalar_imex(rtol=solver.krylov_rtol, max_iter=solver.krylov_max_iter)
            ctx.step_imex(opts)
            ts.advance_time()
            ctx.advance(0)
        by_hand = [ctx.get_state(slot) for slot in fields]
    finally:
        ctx.close()
    assert np.abs(got[1]).max() > 0.5 and np.abs(got[0] - 0.5).max() > 1e-2
    for a, b in zip(got, by_hand):
        assert np.array_equal(a, b)
