"""Subgrid heat flux of the scalar step on the GPU (nsfem_set_scalar_sgs / nsfem_scalar_explicit /
nsfem_scalar_sgs_info, SmagorinskyModel(cs, prandtl_t) under BoussinesqIMEXSolver, the conductive row of
nsfem_wall_compute) against the numpy restatements of tests/scalar_sgs_host.py.

Tolerances.  Kernel: 1e-13 of the largest entry, the project's figure for element kernels against the oracle.  Steps:
those of tests/test_gpu_scalar_transport.py with its Krylov settings (rtol 1e-13) -- T, u*, u 1e-9 and p minus its mean
1e-8, relative.  Wall: the per-entry bound of tests/test_wall_quantities_host.py (2 n eps times the sums of the
absolute contributions, n the rounded operations of the longest chain with a law, plus the two of kappa + nu_x / Pr_t).

Conditions, asserted on the restatements so that a test cannot pass by the term being small.  Kernel: max |D| >= 0.25
max |C T| (C_s = 1; Pr_t = 0.25 in the standard form, 0.025 in the skew form, whose C T is larger against D).  Steps: the
restatement with and without the term differs in T by at least 1e-4 relative after the four steps while kappa_x stays
below kappa / 3 at every quadrature point of every level used (the range in which SBDF2 is stable for every k)."""
import numpy as np
import pytest

import _native as nat
from gpu_common import cavity_bc, rel
from imex_time_stepping import IMEXTimeStepping, IMEXType
from periodic_meshes import is_periodic, lengths_of, periodic_axes, periodic_fields
from scalar_sgs_host import ScalarIMEXSgsRestatement, ScalarSgsRestatement
from test_gpu_3d import lid_bc
from test_gpu_scalar_transport import _B, _two_sides
from test_gpu_variable_viscosity import _COEF, _KERNEL_MESHES, NO_PBC, _max_rel, _mesh, _opts
from test_heated_bodies_host import ScalarPenalRestatement, heated_set
from test_immersed_bodies_host import IMEXPenalRestatement, PenalisationRestatement
from test_scalar_transport_host import ScalarIMEXRestatement, smooth_fields
from test_variable_viscosity_host import SMAGORINSKY, VariableViscosityRestatement

pytestmark = pytest.mark.gpu

TYPES = (IMEXType.SBDF2, IMEXType.CNAB, IMEXType.mCNAB, IMEXType.CNLF)
FORMS = ((0, "standard"), (1, "skew_symmetric"))
KUHN = ((3, 2, 2), (1.0, 0.8, 0.6))

# ---------------------------------------------------------------- 1. the kernel against the restatement
_CS_KERNEL = 1.0
_PRT_KERNEL = {0: 0.25, 1: 0.025}
_KERNEL_REF = {}


def _kernel_reference(kind, form_id, form):
    """C(u) T, D(u, T) of the smooth fields, once per case"""
    key = (kind, form_id)
    if key not in _KERNEL_REF:
        mesh, dm, marks, s, rs, make = _mesh(kind)
        u, T = smooth_fields(dm.p2_coords)
        if is_periodic(kind):
            u, T = periodic_fields(dm.p2_coords, lengths_of(kind), periodic_axes(kind))
        conv = ScalarIMEXRestatement(s, 0.0, form).convection_matrix(u) @ T
        D = ScalarSgsRestatement(rs, _CS_KERNEL, _PRT_KERNEL[form_id]).residual(u, T)
        _KERNEL_REF[key] = (u, T, conv, D)
    return _KERNEL_REF[key]


@pytest.mark.parametrize("form_id,form", FORMS)
@pytest.mark.parametrize("kind", _KERNEL_MESHES, ids=str)
def test_explicit_kernel_matches_the_restatement(kind, form_id, form):
    """weight [C(u) T + D(u, T)] for the smooth non-polynomial fields; with the term off the hook returns the bytes of
    scalar_convection; a second call returns the same bytes, the weight rides in the kernel (slots U2 / T2), no stored
    state is touched and scalar_convection keeps returning C T alone"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    u, T, conv, D = _kernel_reference(kind, form_id, form)
    want = conv + D
    ratio = np.abs(D).max() / np.abs(conv).max()
    assert ratio >= 0.25, ratio
    ctx = make(mesh, dm)
    try:
        ctx.set_state(nat.U1, u)
        ctx.set_state(nat.T1, T)
        plain = ctx.scalar_convection(nat.U1, nat.T1, form_id, 1.0)
        assert ctx.scalar_explicit(nat.U1, nat.T1, form_id, 1.0).tobytes() == plain.tobytes()      # never switched on
        ctx.set_viscosity_law(SMAGORINSKY, (_CS_KERNEL, ))
        assert ctx.scalar_explicit(nat.U1, nat.T1, form_id, 1.0).tobytes() == plain.tobytes()      # a law alone: off
        assert ctx.scalar_sgs_info() == dict(active=False, launches=0, recomputed=0)
        ctx.set_scalar_sgs(_PRT_KERNEL[form_id])
        got = ctx.scalar_explicit(nat.U1, nat.T1, form_id, 1.0)
        err = _max_rel(got, want)
        print("kernel %s form %d: max |D| / max |C T| %.3g, error %.2e of the largest entry" % (kind, form_id, ratio, err))
        assert err < 1e-13
        assert got.tobytes() == ctx.scalar_explicit(nat.U1, nat.T1, form_id, 1.0).tobytes()
        assert ctx.scalar_convection(nat.U1, nat.T1, form_id, 1.0).tobytes() == plain.tobytes()
        ctx.set_state(nat.U2, u)
        ctx.set_state(nat.T2, T)
        assert _max_rel(ctx.scalar_explicit(nat.U2, nat.T2, form_id, -1.5), -1.5 * want) < 1e-13
        assert not ctx.get_state(nat.TCONV_1).any() and not ctx.get_state(nat.TCONV_2).any()
        assert np.array_equal(ctx.get_state(nat.T1), T) and np.array_equal(ctx.get_state(nat.U1), u)
        assert ctx.scalar_sgs_info() == dict(active=True, launches=3, recomputed=0)
        ctx.set_scalar_sgs(0.0)                                                                   # switched off again
        assert ctx.scalar_explicit(nat.U1, nat.T1, form_id, 1.0).tobytes() == plain.tobytes()
        assert ctx.scalar_sgs_info() == dict(active=False, launches=3, recomputed=0)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 2. steps against the restatements
# C_s, Pr_t and kappa of the step tests, chosen on the restatement (conditions in the module docstring; the figures
# each case reaches are printed by its test)
_CS_STEPS, _PRT_STEPS, _KAPPA_STEPS = 0.2, 0.5, 0.05
# (the cells of the (3, 2, 2) Kuhn box are wide: kappa_x reaches 0.031 there, 0.62 of 0.05 -- its case runs with 0.12)
_KAPPA_OF = {KUHN: 0.12}
_HOST = {}


def _step_size(kind):
    """binary step sizes (next_time - current_time is the same number in every step: the rebuild count is that of the
    coefficients alone): 1/16, as tests/test_gpu_scalar_transport.py steps these meshes"""
    return 1.0 / 16.0


class _Host:
    """the restatements of one case -- flow with the Smagorinsky term (and the penalisation of ``bodies``), the scalar
    with the subgrid flux (and H of the bodies) -- stepped `steps` times with cavity / lid velocity data, a body force,
    buoyancy b = _B, Dirichlet T on two sides and a source; beside them the same pair WITHOUT the subgrid flux.  Keeps
    (T0, u*, u0, p) of every step, the largest kappa_x met and the effect of the term on T"""

    def __init__(self, kind, typ, form_id=0, bodies=None, steps=4, cs=_CS_STEPS, prt=_PRT_STEPS):
        mesh, dm, marks, s, rs, make = _mesh(kind)
        kappa = _KAPPA_OF.get(kind, _KAPPA_STEPS)
        X = dm.p2_coords
        dim = X.shape[1]
        self.b = _B[:dim]
        self.vbc = cavity_bc(dm, marks) if dim == 2 else lid_bc(dm, marks)
        self.tbc = _two_sides(dm, marks, X)
        _, self.T_init = smooth_fields(X)
        self.q = np.cos(2.0 * X[:, 0] + 0.3) * np.sin(1.5 * X[:, 1] + 0.2)
        self.f = np.stack([np.sin(np.pi * X[:, 1]), -1.0 + X[:, 0], 0.5 * X[:, 1]][:dim], axis=1).ravel()
        self.k, self.kappa = _step_size(kind), kappa
        form = FORMS[form_id][1]
        visc = VariableViscosityRestatement(rs, SMAGORINSKY, (cs, ))
        sgs = ScalarSgsRestatement(rs, cs, prt)
        pairs = []
        for term in (sgs, None):
            flow = IMEXPenalRestatement(s, _COEF, "standard", visc=visc,
                                        penal=PenalisationRestatement(rs, bodies, 0.0) if bodies is not None else None)
            orc = ScalarIMEXSgsRestatement(s, kappa, form, term,
                                           ScalarPenalRestatement(rs, bodies, 0.0) if bodies is not None else None)
            orc.source = self.q
            orc.T[0], orc.T[1] = self.T_init.copy(), self.T_init.copy()
            pairs.append((flow, orc))
        ts = IMEXTimeStepping(0.0, 1.0e9, typ, desired_start_time_step=self.k)
        self.coefficients, self.snapshots, self.kappa_x_max = [], [], 0.0
        for step in range(steps):
            ts.update_coefficients()
            kk = ts.get_next_step_size()
            self.coefficients.append((tuple(ts.alpha), tuple(ts.beta), tuple(ts.gamma), kk))
            for flow, orc in pairs:
                if orc.sgs is not None:
                    for level in (1, 2) if ts.beta[1] != 0.0 else (1, ):
                        self.kappa_x_max = max(self.kappa_x_max, float(sgs.kappa_x(flow.vel[level]).max()))
                orc.step(ts.alpha, ts.beta, ts.gamma, kk, flow.vel[1], flow.vel[2], self.tbc)
                flow.body_force = self.f + np.outer(orc.T[0], self.b).ravel()
                flow.step(ts.alpha, ts.beta, ts.gamma, kk, self.vbc, NO_PBC)
            flow, orc = pairs[0]
            self.snapshots.append((orc.T[0].copy(), flow.ustar.copy(), flow.vel[0].copy(), flow.p.copy()))
            for flow, orc in pairs:
                orc.advance()
                flow.advance()
            ts.advance_time()
        self.effect = rel(pairs[0][1].T[1], pairs[1][1].T[1])


def _host(kind, typ, form_id=0, bodies_key=None):
    key = (kind, typ, form_id, bodies_key)
    if key not in _HOST:
        bodies = None
        if bodies_key is not None:
            k = _step_size(kind)
            bodies = heated_set(2, bodies_key, 2.0 * k, 0.0, 2.0 * k)
        _HOST[key] = (_Host(kind, typ, form_id, bodies), bodies)
    return _HOST[key]


def _drive(kind, typ, form_id=0, bodies_key=None):
    """the device beside the snapshots of the restatements; returns the counters"""
    host, bodies = _host(kind, typ, form_id, bodies_key)
    tag = "%s %s form %d%s" % (kind, typ.name, form_id, " heated " + bodies_key if bodies_key else "")
    print("%s: effect of D on T %.2e, max kappa_x %.3e = %.3f kappa" % (tag, host.effect, host.kappa_x_max,
                                                                       host.kappa_x_max / host.kappa))
    assert host.effect >= 1e-4 and host.kappa_x_max < host.kappa / 3.0
    mesh, dm, marks, s, rs, make = _mesh(kind)
    ctx = make(mesh, dm)
    try:
        ctx.set_coeffs(1.0, 1.0, 0.01, 1.0)
        ctx.set_dirichlet(nat.VELOCITY, *host.vbc)
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        ctx.set_dirichlet(nat.SCALAR, *host.tbc)
        ctx.set_scalar(host.kappa, host.b, form_id)
        ctx.set_viscosity_law(SMAGORINSKY, (_CS_STEPS, ))
        ctx.set_scalar_sgs(_PRT_STEPS)
        ctx.set_state(nat.BODY_FORCE, host.f)
        ctx.set_state(nat.T_SOURCE, host.q)
        ctx.set_state(nat.T0, host.T_init)
        ctx.set_state(nat.T1, host.T_init)
        if bodies is not None:
            ctx.set_bodies(bodies.rows(0.0), bodies.eta, bodies.smoothing)
            ctx.set_body_temperatures(*bodies.temperatures(), bodies.eta_scalar)
        opts = _opts(ctx)
        for step, ((alpha, beta, gamma, kk), (T0, ustar, u0, p0)) in enumerate(zip(host.coefficients, host.snapshots)):
            ctx.set_imex(alpha, beta, gamma, kk)
            si = ctx.step_scalar_imex(rtol=1e-13)
            et = rel(ctx.get_state(nat.T0), T0)
            ctx.step_imex(opts)
            us, u, p = ctx.get_state(nat.USTAR), ctx.get_state(nat.U0), ctx.get_state(nat.P)
            es, eu, ep = rel(us, ustar), rel(u, u0), rel(p - p.mean(), p0 - p0.mean())
            print("%s step %d: T %.2e u* %.2e u %.2e p %.2e cg %d" % (tag, step, et, es, eu, ep, si.iterations))
            assert si.converged and et < 1e-9, (tag, step, et)
            assert es < 1e-9 and eu < 1e-9 and ep < 1e-8, (tag, step, es, eu, ep)
            ctx.advance(0)
        return ctx.scalar_info(), ctx.scalar_sgs_info(), ctx.viscosity_info(), ctx.body_heat_info()
    finally:
        ctx.close()


@pytest.mark.parametrize("typ", TYPES, ids=lambda t: t.name)
def test_steps_with_the_subgrid_flux_match_the_restatements(typ):
    """box(8, 8), 4 steps of every IMEXType with buoyancy and Dirichlet sides, the Smagorinsky term in the flow step
    alongside; one launch per step -- C(u2) T2 + D(u2, T2) is the vector the step before stored"""
    info, sgs, visc, heat = _drive((8, 8), typ)
    reuses = 3 if typ is not IMEXType.CNLF else 0
    assert info["convection_launches"] == 4 and info["convection_reuses"] == reuses and info["dictionary"] is False, info
    assert sgs == dict(active=True, launches=4, recomputed=0), sgs
    assert visc["law"] == SMAGORINSKY and visc["recomputed"] == 0, visc


@pytest.mark.parametrize("kind,form_id,dictionary", [((16, 16), 0, True), ((16, 16), 1, True), (KUHN, 0, False),
                                                     (KUHN, 1, False)], ids=str)
def test_sbdf2_steps_on_the_dictionary_path_and_in_3d(kind, form_id, dictionary):
    """SBDF2, 4 steps: box(16, 16) solves on the dictionary copy of the matrix (which the term must not touch), the
    (3, 2, 2) Kuhn box runs the 3D kernel inside the steps; both forms"""
    info, sgs, visc, heat = _drive(kind, IMEXType.SBDF2, form_id)
    assert info["convection_launches"] == 4 and info["convection_reuses"] == 3 and info["matrix_builds"] == 2, info
    assert info["dictionary"] is dictionary, info
    assert sgs == dict(active=True, launches=4, recomputed=0), sgs


def test_sbdf2_steps_with_a_heated_disc():
    """box(8, 8), SBDF2, 4 steps with the sharp heated disc of tests/test_gpu_heated_bodies.py, eta = eta_T = 2 k: the
    PENAL = 1, SGS = 1 kernel forms C T + D + H in the one launch of a step"""
    info, sgs, visc, heat = _drive((8, 8), IMEXType.SBDF2, 0, "disc")
    assert info["convection_launches"] == 4 and info["convection_reuses"] == 3, info
    assert sgs == dict(active=True, launches=4, recomputed=0), sgs
    assert heat == dict(thermal=1, fused_launches=4, recomputed=0), heat


# ---------------------------------------------------------------- 3. bookkeeping
class _Transport:
    """transport steps alone with a fixed smooth velocity at every level (no flow step), SBDF2, Dirichlet sides and a
    source, on box(8, 8); the restatement beside the device"""

    def __init__(self, prt=_PRT_STEPS, cs=_CS_STEPS, law=True, with_orc=True):
        self.mesh, self.dm, marks, self.s, self.rs, make = _mesh((8, 8))
        X = self.dm.p2_coords
        self.u, T_init = smooth_fields(X)
        self.tbc = _two_sides(self.dm, marks, X)
        q = np.cos(2.0 * X[:, 0] + 0.3) * np.sin(1.5 * X[:, 1] + 0.2)
        self.orc = None
        if with_orc:
            sgs = ScalarSgsRestatement(self.rs, cs, prt) if prt else None
            self.orc = ScalarIMEXSgsRestatement(self.s, _KAPPA_STEPS, "standard", sgs)
            self.orc.source = q
            self.orc.T[0], self.orc.T[1] = T_init.copy(), T_init.copy()
        self.ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=1.0 / 16.0)
        self.ctx = ctx = make(self.mesh, self.dm)
        try:
            ctx.set_dirichlet(nat.SCALAR, *self.tbc)
            ctx.set_scalar(_KAPPA_STEPS, None, 0)
            if law:
                ctx.set_viscosity_law(SMAGORINSKY, (cs, ))
            if prt is not None:
                ctx.set_scalar_sgs(prt)
            ctx.set_state(nat.T_SOURCE, q)
            for slot in (nat.T0, nat.T1):
                ctx.set_state(slot, T_init)
            for slot in (nat.U0, nat.U1, nat.U2):
                ctx.set_state(slot, self.u)
        except BaseException:
            ctx.close()
            raise

    def step(self, check=True):
        ts = self.ts
        ts.update_coefficients()
        kk = ts.get_next_step_size()
        self.ctx.set_imex(ts.alpha, ts.beta, ts.gamma, kk)
        si = self.ctx.step_scalar_imex(rtol=1e-13)
        assert si.converged
        if self.orc is not None:
            self.orc.step(ts.alpha, ts.beta, ts.gamma, kk, self.u, self.u, self.tbc)
            if check:
                et = rel(self.ctx.get_state(nat.T0), self.orc.T[0])
                print("transport step %d: T %.2e" % (ts.step_number, et))
                assert et < 1e-9, et
            self.orc.advance()
        self.ctx.advance(0)
        ts.advance_time()

    def states(self):
        return [self.ctx.get_state(slot).tobytes() for slot in (nat.T0, nat.T1, nat.T2, nat.TCONV_1, nat.TCONV_2)]


def test_changes_of_prandtl_number_or_constant_recompute_the_stored_vector_once():
    """a reused TCONV_2 is counted as reused; another Pr_t, or another C_s while the term is on, makes the next step
    form it again with the level's own data (one more launch, counted) and the result matches a restatement restarted
    without its N2; the same values again change nothing"""
    run = _Transport()
    ctx = run.ctx
    try:
        run.step()
        run.step()
        info, sgs = ctx.scalar_info(), ctx.scalar_sgs_info()
        assert info["convection_launches"] == 2 and info["convection_reuses"] == 1, info
        assert sgs == dict(active=True, launches=2, recomputed=0), sgs
        ctx.set_scalar_sgs(_PRT_STEPS)                                     # the same value: no change
        ctx.set_viscosity_law(SMAGORINSKY, (_CS_STEPS, ))
        run.step()
        assert ctx.scalar_info()["convection_reuses"] == 2 and ctx.scalar_sgs_info()["recomputed"] == 0
        # another Pr_t
        ctx.set_scalar_sgs(0.8)
        run.orc.sgs = ScalarSgsRestatement(run.rs, _CS_STEPS, 0.8)
        run.orc.N2 = None
        run.step()
        info, sgs = ctx.scalar_info(), ctx.scalar_sgs_info()
        assert info["convection_launches"] == 5 and info["convection_reuses"] == 2, info
        assert sgs == dict(active=True, launches=5, recomputed=1), sgs
        run.step()
        assert ctx.scalar_info()["convection_reuses"] == 3 and ctx.scalar_sgs_info()["recomputed"] == 1
        # another C_s while the term is on
        ctx.set_viscosity_law(SMAGORINSKY, (0.3, ))
        run.orc.sgs = ScalarSgsRestatement(run.rs, 0.3, 0.8)
        run.orc.N2 = None
        run.step()
        info, sgs = ctx.scalar_info(), ctx.scalar_sgs_info()
        assert info["convection_launches"] == 8 and info["convection_reuses"] == 3, info
        assert sgs == dict(active=True, launches=8, recomputed=2), sgs
        assert ctx.body_heat_info()["recomputed"] == 0
        # with the term off a change of C_s is nothing to the scalar
        ctx.set_scalar_sgs(0.0)
        run.orc.sgs = None
        run.orc.N2 = None
        run.step()
        assert ctx.scalar_sgs_info() == dict(active=False, launches=8, recomputed=3)
        ctx.set_viscosity_law(SMAGORINSKY, (0.1, ))
        run.step()
        assert ctx.scalar_sgs_info() == dict(active=False, launches=8, recomputed=3)
        assert ctx.scalar_info()["convection_reuses"] == 4
    finally:
        ctx.close()


def test_heat_and_sgs_keys_stale_in_one_gap():
    """box(8, 8), SBDF2, the Smagorinsky term with Pr_t and the sharp heated disc, three full time steps (flow step,
    scalar step, advance); then another Pr_t AND another body temperature before step four: the stored TCONV_2 is stale
    on both counts, each cause is counted once, nothing is reused and both element launches of the step are fused ones
    with the term.  A twin context that gets the same calls and forms TCONV_2 afresh in every step (T2 written back by
    hand) agrees in T0 to 1e-13 of the largest entry after every step, the element-vector bound of
    tests/test_gpu_imex_composed.py for the same comparison"""
    mesh, dm, marks, s, rs, make = _mesh((8, 8))
    X = dm.p2_coords
    k = _step_size((8, 8))
    bodies = heated_set(2, "disc", 2.0 * k, 0.0, 2.0 * k)
    vbc, tbc = cavity_bc(dm, marks), _two_sides(dm, marks, X)
    _, T_init = smooth_fields(X)
    q = np.cos(2.0 * X[:, 0] + 0.3) * np.sin(1.5 * X[:, 1] + 0.2)
    f = np.stack([np.sin(np.pi * X[:, 1]), -1.0 + X[:, 0]], axis=1).ravel()
    flags, temps = bodies.temperatures()
    ctxs = [make(mesh, dm), make(mesh, dm)]
    try:
        for ctx in ctxs:
            ctx.set_coeffs(1.0, 1.0, 0.01, 1.0)
            ctx.set_dirichlet(nat.VELOCITY, *vbc)
            ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
            ctx.set_dirichlet(nat.SCALAR, *tbc)
            ctx.set_scalar(_KAPPA_STEPS, _B[:2], 0)
            ctx.set_viscosity_law(SMAGORINSKY, (_CS_STEPS, ))
            ctx.set_scalar_sgs(_PRT_STEPS)
            ctx.set_state(nat.BODY_FORCE, f)
            ctx.set_state(nat.T_SOURCE, q)
            ctx.set_state(nat.T0, T_init)
            ctx.set_state(nat.T1, T_init)
            ctx.set_bodies(bodies.rows(0.0), bodies.eta, bodies.smoothing)
            ctx.set_body_temperatures(flags, temps, bodies.eta_scalar)
        dev, twin = ctxs
        opts = [_opts(ctx) for ctx in ctxs]
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=k)

        def counters():
            sgs, heat, info = dev.scalar_sgs_info(), dev.body_heat_info(), dev.scalar_info()
            return np.array([sgs["recomputed"], heat["recomputed"], info["convection_reuses"],
                             info["convection_launches"], sgs["launches"], heat["fused_launches"]])

        def full_step(step):
            ts.update_coefficients()
            for ctx, o in zip(ctxs, opts):
                ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
                ctx.step_imex(o)
                if ctx is twin:
                    ctx.set_state(nat.T2, ctx.get_state(nat.T2))
                assert ctx.step_scalar_imex(rtol=1e-13).converged
            T, Tt = dev.get_state(nat.T0), twin.get_state(nat.T0)
            err = _max_rel(T, Tt)
            print("stale in one gap, step %d: T0 against the twin %.2e of the largest entry" % (step, err))
            assert err < 1e-13, (step, err)
            for ctx in ctxs:
                ctx.advance(0)
            ts.advance_time()
        for step in range(3):
            full_step(step)
        assert dev.scalar_info()["convection_reuses"] == 2 and dev.scalar_sgs_info()["recomputed"] == 0
        assert dev.body_heat_info() == dict(thermal=1, fused_launches=3, recomputed=0)
        for ctx in ctxs:
            ctx.set_scalar_sgs(0.8)
            ctx.set_body_temperatures(flags, np.where(flags == 1, temps + 0.35, 0.0), bodies.eta_scalar)
        before = counters()
        full_step(3)
        diff = counters() - before
        print("stale in one gap, step 3: sgs recomputed, heat recomputed, reuses, launches, sgs launches, fused", diff)
        assert diff.tolist() == [1, 1, 0, 2, 2, 2], diff
    finally:
        for ctx in ctxs:
            ctx.close()


def test_same_state_gives_the_same_bytes_and_switching_off_returns_to_the_old_bytes():
    """three steps on two fresh contexts give the same bytes in every scalar slot; a context on which Pr_t was set and
    set back to 0 before the first step ends on the bytes of a context that never called the setter; one on which the
    term was on for two steps and then off forms, from the levels of the plain run, the plain run's stored vector (the
    solve itself is not compared there: its check schedule follows the iteration counts of the steps before)"""
    def three_steps(**kw):
        run = _Transport(with_orc=False, **kw)
        try:
            for _ in range(3):
                run.step()
            return run.states(), run.ctx.scalar_sgs_info()
        finally:
            run.ctx.close()
    on_a, info_a = three_steps()
    on_b, info_b = three_steps()
    assert on_a == on_b and info_a == info_b == dict(active=True, launches=3, recomputed=0)
    never, info_never = three_steps(prt=None, law=False)
    assert never != on_a and info_never == dict(active=False, launches=0, recomputed=0)
    # set and set back before the first step
    run = _Transport(with_orc=False)
    try:
        run.ctx.set_scalar_sgs(0.0)
        for _ in range(3):
            run.step()
        assert run.states() == never
        assert run.ctx.scalar_sgs_info() == dict(active=False, launches=0, recomputed=0)
    finally:
        run.ctx.close()
    # on for two steps, then off: from the levels of the plain run the third step gives the plain bytes
    plain = _Transport(prt=None, law=False, with_orc=False)
    run = _Transport(with_orc=False)
    try:
        for _ in range(2):
            plain.step()
            run.step()
        run.ctx.set_scalar_sgs(0.0)
        for slot in (nat.T1, nat.T2):
            run.ctx.set_state(slot, plain.ctx.get_state(slot))
        plain.ctx.set_state(nat.T2, plain.ctx.get_state(nat.T2))           # (both form C(u2) T2 afresh)
        plain.step()
        run.step()
        assert run.ctx.scalar_sgs_info() == dict(active=False, launches=2, recomputed=0)       # (T2 by hand: not usable)
        assert run.ctx.get_state(nat.TCONV_2).tobytes() == plain.ctx.get_state(nat.TCONV_2).tobytes()
    finally:
        plain.ctx.close()
        run.ctx.close()


def test_every_refusal_leaves_state_and_counters_unchanged():
    """bad Pr_t values; the term on without law 1 (no law, Carreau) in the step and in the hook; bad slots and forms of
    the hook: NativeError, and every scalar slot and counter is what it was"""
    run = _Transport(with_orc=False)
    ctx = run.ctx
    try:
        run.step()
        run.step()
        ctx.set_imex(run.ts.alpha, run.ts.beta, run.ts.gamma, run.ts.get_next_step_size())
        before = (run.states(), ctx.scalar_info(), ctx.scalar_sgs_info(), ctx.viscosity_info())
        for bad in (-0.5, np.nan, np.inf, -np.inf):
            with pytest.raises(nat.NativeError, match="Pr_t"):
                ctx.set_scalar_sgs(bad)
        with pytest.raises(nat.NativeError, match="form"):
            ctx.scalar_explicit(nat.U1, nat.T1, 2, 1.0)
        with pytest.raises(nat.NativeError, match="slot"):
            ctx.scalar_explicit(nat.P, nat.T1, 0, 1.0)
        with pytest.raises(nat.NativeError, match="slot"):
            ctx.scalar_explicit(nat.U1, nat.U2, 0, 1.0)
        with pytest.raises(nat.NativeError, match="weight"):
            ctx.scalar_explicit(nat.U1, nat.T1, 0, np.nan)
        assert (run.states(), ctx.scalar_info(), ctx.scalar_sgs_info(), ctx.viscosity_info()) == before
        for law, params in ((0, None), (2, (0.008, 1.0, 0.5))):
            ctx.set_viscosity_law(law, params)
            base = (run.states(), ctx.scalar_info(), ctx.scalar_sgs_info())
            with pytest.raises(nat.NativeError, match="viscosity law is not 1"):
                ctx.step_scalar_imex(rtol=1e-13)
            with pytest.raises(nat.NativeError, match="viscosity law is not 1"):
                ctx.scalar_explicit(nat.U1, nat.T1, 0, 1.0)
            assert (run.states(), ctx.scalar_info(), ctx.scalar_sgs_info()) == base
        # a fresh context: the refused step allocates no scalar level
        other = _Transport(law=False, with_orc=False)
        try:
            other.ctx.set_imex(run.ts.alpha, run.ts.beta, run.ts.gamma, run.ts.get_next_step_size())
            with pytest.raises(nat.NativeError, match="viscosity law is not 1"):
                other.ctx.step_scalar_imex(rtol=1e-13)
            assert not other.ctx.get_state(nat.TCONV_1).any()
            assert other.ctx.scalar_info()["convection_launches"] == 0
        finally:
            other.ctx.close()
        # back to law 1 with the C_s of before: the epoch moved (the law changed twice), so the step forms TCONV_2 again
        ctx.set_viscosity_law(SMAGORINSKY, (_CS_STEPS, ))
        run.step()
        assert ctx.scalar_sgs_info() == dict(active=True, launches=4, recomputed=1)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 4. through the classes
_SPEC = dict(name="Cavity", mesh=("cube", 2, 8), scheme="ipcs", clock=dict(dt=0.5 / 8, steps=3),
             numbers=dict(Re=100.0, Fr=1.0), start={"velocity": (0.0, 0.0), "pressure": 0.0, "temperature": 0.5},
             bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_slip", "bottom"), ("velocity", "top", (1.0, 0.0))])


def test_boussinesq_solver_with_a_turbulent_prandtl_number_equals_driving_the_steps_by_hand(monkeypatch):
    """BoussinesqIMEXSolver through InstationaryProblem.solve_problem with SmagorinskyModel(cs, prandtl_t) on the 8 x 8
    cavity, 3 steps: bit for bit what set_viscosity_law / set_scalar_sgs / step_scalar_imex / step_imex / advance give
    through the C ABI; _compute_model_diffusivity returns the device cell means of nu_x divided by Pr_t"""
    from fem_function import HostField
    from multigrid import attach_hierarchy
    from ns_boussinesq_solver import BoussinesqIMEXSolver
    from problem_specs import build_problem
    from viscosity_models import SmagorinskyModel
    steps, dt = _SPEC["clock"]["steps"], _SPEC["clock"]["dt"]
    monkeypatch.setenv("NSFEM_NO_OUTPUT", "1")
    problem = build_problem(dict(_SPEC))
    cls = type(problem)

    def set_viscosity_model(self):
        self._viscosity_model = SmagorinskyModel(_CS_STEPS, prandtl_t=_PRT_STEPS)

    def set_temperature_coefficients(self):
        self._temperature_coefficients = dict(diffusivity=_KAPPA_STEPS, buoyancy=(0.0, 1.0), convective_form="standard")

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
    assert solver._ctx.scalar_sgs_info() == dict(active=True, launches=steps, recomputed=0)
    T_cls, u_cls = solver._ctx.get_state(nat.T1), solver._ctx.get_state(nat.U1)
    field = problem._compute_model_diffusivity()
    assert isinstance(field, HostField) and field.center == "Cell" and field.name() == "model diffusivity"
    means = solver._ctx.viscosity_cells(nat.U0)
    assert np.array_equal(field.values, means / _PRT_STEPS) and field.values.max() > 1e-4
    assert np.array_equal(problem._compute_model_viscosity().values, means)
    # ---- the same steps through the C ABI on a fresh context
    dm, mesh = solver._dofmap, solver._mesh
    left = np.unique(dm.facet_p2_nodes(solver._boundary_markers.facets_with_id(problem._sides["left"])))
    right = np.unique(dm.facet_p2_nodes(solver._boundary_markers.facets_with_id(problem._sides["right"])))
    out = {}
    for prt in (_PRT_STEPS, 0.0):
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
            ctx.set_scalar(_KAPPA_STEPS, (0.0, 1.0), 0)
            ctx.set_viscosity_law(SMAGORINSKY, (_CS_STEPS, ))
            ctx.set_scalar_sgs(prt)
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
            out[prt] = (ctx.get_state(nat.T1), ctx.get_state(nat.U1))
        finally:
            ctx.close()
    assert np.abs(u_cls).max() > 0.5 and np.abs(T_cls - 0.5).max() > 1e-2
    assert np.array_equal(T_cls, out[_PRT_STEPS][0]) and np.array_equal(u_cls, out[_PRT_STEPS][1])
    assert rel(out[0.0][0], T_cls) > 1e-5                                    # (without Pr_t the scalar differs)
    # a model without prandtl_t handed over in the middle of the run switches the term off
    solver.set_viscosity_model(SmagorinskyModel(_CS_STEPS))
    assert solver._ctx.scalar_sgs_info()["active"] is False
    with pytest.raises(RuntimeError, match="prandtl_t"):
        problem._compute_model_diffusivity()


# ---------------------------------------------------------------- 5. the conductive row of the wall quantities
_WALL_PRT = 0.4


def _wall_heat_reference(mesh, dm, cells, local, u, T, kappa, cs, prt):
    """heat rows int -(kappa + nu_x / Pr_t) grad T . n of the facets (cells, local) by the kernel's facet rule, and
    the sums of the absolute contributions (the scale of the rounding bound)"""
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
    delta2 = (np.abs(np.linalg.det(J)) / (2.0 if dim == 2 else 6.0)) ** (2.0 / dim)
    w = area[:, None] * wts[None, :]
    out = []
    for mod in ((lambda a: a), np.abs):
        g2 = np.einsum("fba,fqkb->fqka", mod(Jinv), wh.p2_basis(lam, mod)[1])
        G = np.einsum("fqkb,fka->fqab", g2, mod(ue))
        gamma = np.sqrt(0.5 * ((G + np.swapaxes(G, 2, 3)) ** 2).sum(axis=(2, 3)))
        kap = abs(kappa) + (cs * cs * delta2)[:, None] * gamma / prt
        sign = -1.0 if mod is not np.abs else 1.0
        out.append(sign * np.einsum("fq,fq,fqkb,fk,fb->f", w, kap, g2, mod(Te), mod(nrm)))
    return out[0], out[1]


@pytest.mark.parametrize("name", ["box4x4", "kuhn3x2x2"])
def test_wall_heat_row_carries_the_eddy_diffusivity(name):
    """box(4, 4) and the (3, 2, 2) Kuhn box, every boundary facet: with law 1, use_law and Pr_t the conductive row is
    int -(kappa + nu_x / Pr_t) grad T . n; every other entry, and with the term off (or use_law off) that row too, keeps
    its bytes"""
    import test_wall_quantities_host as wh
    from test_derived_fields_host import smooth_fields as wall_fields
    mesh, dm, marks, s, rs, make = _mesh((4, 4) if name == "box4x4" else KUHN)
    dim = dm.dim
    ids, cells, local = wh.boundary_facets(mesh)
    u, p, T = wall_fields(dm.p2_coords, dm.p1_coords)
    o = wh.OPTS
    cs = 0.9
    want, scale = _wall_heat_reference(mesh, dm, cells, local, u, T, o["kappa"], cs, _WALL_PRT)
    molecular = wh.wall_reference(mesh, dm, (cells, local), u, p, T, o)[:, 3 + 2 * dim]
    bound = 2.0 * (wh.n_terms(dim, True) + 2) * wh.EPS * scale
    assert np.abs(want - molecular).max() > 1e3 * bound.max() and np.abs(want - molecular).max() > 1e-3
    group = np.zeros(ids.size, dtype=np.int32)
    ctx = make(mesh, dm)
    try:
        ctx.set_scalar(o["kappa"])
        ctx.set_state(nat.T0, T)
        ctx.set_state(nat.U0, np.ascontiguousarray(u).ravel())
        ctx.set_state(nat.P, p)
        ctx.set_viscosity_law(SMAGORINSKY, (cs, ))
        ctx.wall_set_facets(cells, local, group, 1)

        def compute(use_law):
            return ctx.wall_compute(o["nu"], o["sym"], o["kappa"], o["origin"], use_law=use_law, scalar_slot=nat.T0,
                                    facets=True)
        sums_off, rows_off = compute(True)
        ctx.set_scalar_sgs(_WALL_PRT)
        sums_on, rows_on = compute(True)
        sums_nolaw, rows_nolaw = compute(False)
        ctx.set_scalar_sgs(0.0)
        sums_back, rows_back = compute(True)
        sums_nolaw_ref, rows_nolaw_ref = compute(False)
    finally:
        ctx.close()
    heat = 3 + 2 * dim
    err = np.abs(rows_on[:, heat] - want)
    print("wall heat %s: max error %.3e, max error / bound %.3f, eddy part %.3e" % (
        name, err.max(), (err / bound).max(), np.abs(want - molecular).max()))
    assert (err <= bound).all()
    others = [c for c in range(rows_on.shape[1]) if c != heat]
    assert rows_on[:, others].tobytes() == rows_off[:, others].tobytes()
    assert rows_back.tobytes() == rows_off.tobytes() and sums_back.tobytes() == sums_off.tobytes()
    assert rows_nolaw.tobytes() == rows_nolaw_ref.tobytes() and sums_nolaw.tobytes() == sums_nolaw_ref.tobytes()
    assert (np.abs(rows_off[:, heat] - molecular) <= bound).all()
