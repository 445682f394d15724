"""Heated immersed bodies on the GPU (nsfem_set_body_temperatures / nsfem_body_scalar_residual / nsfem_body_heat /
nsfem_body_heat_info, the fused launches of nsfem_step_scalar_imex, BoussinesqIMEXSolver) against the numpy
restatements of tests/test_heated_bodies_host.py.

Tolerances.  Sharp masks: 1e-13 relative to the largest entry, the project's figure for element kernels against the
oracle.  Smoothed masks call sin: ten times the largest difference measured over the cases below (SMOOTH_MEASURED),
capped at 1e-11.  Steps: those of tests/test_gpu_imex.py and tests/test_gpu_scalar_transport.py -- T, u*, u 1e-9 and p
minus its mean 1e-8, relative, with Krylov rtol 1e-13.

Meshes.  Those of tests/test_gpu_immersed_bodies.py; bodies ``bodies_2d`` / ``bodies_3d`` with temperatures
(``heated_set`` of the host file; in ``overlap`` the disc is thermal and the box passive).  The quadrature clearances of
these pairs are pinned by tests/test_immersed_bodies_host.py; the mapped box(8, 8) is not among them and runs with the
smoothed mask only, and so does every pose that is a shift of those bodies (the pose a ``nsfem_move_bodies`` brings).  On
the general tetrahedra the clearance of the set pose is asserted here before the sharp comparison (>= 1e-9), and that
every body cuts cells of both orientations."""
import numpy as np
import pytest

import _native as nat
from gpu_common import cavity_bc, rel
from imex_time_stepping import IMEXTimeStepping, IMEXType
from immersed_bodies import Ball, Box, ImmersedBodies
from test_gpu_3d import lid_bc
from test_gpu_immersed_bodies import _dim, _step_size, body_cases, cut_cells_by_orientation, velocity_and_scalar
from test_gpu_scalar_transport import _B, _two_sides
from test_gpu_variable_viscosity import _COEF, _KERNEL_MESHES, NO_PBC, _mesh, _opts, is_general
from test_heated_bodies_host import ScalarIMEXPenalRestatement, ScalarPenalRestatement, heated, heated_set
from test_immersed_bodies_host import BODY_NAMES, IMEXPenalRestatement, PenalisationRestatement, bodies_2d
from test_scalar_transport_host import ScalarIMEXRestatement, smooth_fields

pytestmark = pytest.mark.gpu

EPS = 0.07
# the largest smoothed-mask difference printed by test_fused_kernel_and_heat_numbers_match_the_restatement over all its
# cases (of the largest entry): box(16, 16), half-space, standard form -- the sharp masks show the same 2.02e-15 there,
# so this is the rounding of the sums, not of sin
SMOOTH_MEASURED = 2.02e-15
_TOL = {0.0: 1e-13, EPS: min(10.0 * SMOOTH_MEASURED, 1e-11)}
_SHIFT = (0.06, 0.045, 0.05)
_ETA, _ETA_T = 0.037, 0.021


def _max_rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


_CONV = {}


def _convection(kind, s, u, T, form):
    """C(u) T of the oracle for the smooth fields, once per mesh and form"""
    if (kind, form) not in _CONV:
        _CONV[kind, form] = ScalarIMEXRestatement(s, 0.0, ("standard", "skew_symmetric")[form]).convection_matrix(u) @ T
    return _CONV[kind, form]


def _shifted(dim, name, eps):
    """the set of ``heated_set`` with every centre moved by _SHIFT: the pose a move brings"""
    bodies = heated_set(dim, name, _ETA, eps, _ETA_T)
    for b in bodies.bodies:
        b.centre = b.centre + np.array(_SHIFT[:dim])
    return bodies


# ---------------------------------------------------------------- a. / b. the kernels against the restatement
@pytest.mark.parametrize("kind,name", body_cases(), ids=str)
def test_fused_kernel_and_heat_numbers_match_the_restatement(kind, name):
    """weight (C(u) T + H(T)) from the fused launch and the heat numbers per body for the smooth non-polynomial fields:
    sharp and smoothed masks, both forms, weights 1 and -1.5 (other slots), the pose of t^n and -- after one
    nsfem_move_bodies -- that of t^(n-1); with a zero velocity the hook returns H alone, whose node sum equals the summed
    heat rates of the device; second calls return the same bytes; nsfem_scalar_convection returns what it returned
    before; no stored state is touched.

    Sum identity: both sides are sums of the same products in another order; each is within (number of terms) * 2.2e-16
    * (sum of the absolute terms) of the exact value, so their difference is within the sum of the two bounds."""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    dim = _dim(kind)
    u, T = velocity_and_scalar(kind, dm)
    ctx = make(mesh, dm)
    try:
        for slot in (nat.U1, nat.USTAR):
            ctx.set_state(slot, u)
        ctx.set_state(nat.U2, np.zeros_like(u))
        for slot in (nat.T1, nat.T2):
            ctx.set_state(slot, T)
        plain = {form: ctx.scalar_convection(nat.U1, nat.T1, form, 1.0) for form in (0, 1)}
        launches = 0
        for eps in ((EPS, ) if kind == "mapped" else (0.0, EPS)):
            tol = _TOL[eps]
            bodies, moved = heated_set(dim, name, _ETA, eps, _ETA_T), _shifted(dim, name, eps)
            orc, orc_moved = ScalarPenalRestatement(rs, bodies), ScalarPenalRestatement(rs, moved)
            H, H_moved, heat = orc.residual(T), orc_moved.residual(T), orc.heat(T)
            if is_general(kind) and eps == 0.0:
                assert PenalisationRestatement(rs, bodies).surface_clearance() >= 1e-9
                means = np.einsum("q,cq->c", rs.wts, orc.chi) / rs.wts.sum()
                assert min(cut_cells_by_orientation(mesh, means)) >= 4
            ctx.set_bodies(bodies.rows(), bodies.eta, bodies.smoothing)
            ctx.set_body_temperatures(*bodies.temperatures(), bodies.eta_scalar)
            # ---- the pose set: H alone, the heat numbers, the sum identity
            alone = ctx.body_scalar_residual(nat.U2, nat.T1, 0, 1.0, 0)
            Q = ctx.body_heat(nat.T1)
            herr, qerr = _max_rel(alone, H), _max_rel(Q, heat)
            print("%s %s eps %.2f: H alone %.2e heat numbers %.2e (of the largest entry)" % (kind, name, eps, herr, qerr))
            assert Q.shape == heat.shape == (len(bodies.bodies), 3) and np.abs(heat[:, 1]).max() > 1e-3
            assert herr < tol and qerr < tol, (herr, qerr)
            assert alone.tobytes() == ctx.body_scalar_residual(nat.U2, nat.T1, 0, 1.0, 0).tobytes()
            assert Q.tobytes() == ctx.body_heat(nat.T1).tobytes()
            absq = float((rs.wdet * np.abs(orc._density(T))).sum())
            bound = 2.2e-16 * (alone.size * np.abs(alone).sum() + orc.chi.size * absq)
            assert abs(alone.sum() - Q[:, 1].sum()) <= bound
            if name == "overlap":
                assert Q[1, 1] == 0.0 and Q[1, 0] > 0.0          # (the passive box: a volume, no heat)
            launches += 2
            for form in (0, 1):
                conv = _convection(kind, s, u, T, form)
                want = conv + H
                assert np.linalg.norm(H) >= 1e-3 * np.linalg.norm(want)
                got = ctx.body_scalar_residual(nat.U1, nat.T1, form, 1.0, 0)
                err = _max_rel(got, want)
                assert got.tobytes() == ctx.body_scalar_residual(nat.U1, nat.T1, form, 1.0, 1).tobytes()   # (no move yet)
                werr = _max_rel(ctx.body_scalar_residual(nat.USTAR, nat.T2, form, -1.5, 0), -1.5 * want)
                print("  form %d: fused %.2e, weight -1.5 %.2e" % (form, err, werr))
                assert err < tol and werr < tol, (err, werr)
                assert ctx.scalar_convection(nat.U1, nat.T1, form, 1.0).tobytes() == plain[form].tobytes()
                assert _max_rel(plain[form], conv) < 1e-13
                launches += 3
            # ---- one move: pose 1 is the set's, pose 0 the moved one (a shifted pose: compared smoothed only)
            ctx.move_bodies(moved.rows())
            for form in (0, 1):
                conv = _convection(kind, s, u, T, form)
                older = ctx.body_scalar_residual(nat.U1, nat.T1, form, 1.0, 1)
                newer = ctx.body_scalar_residual(nat.U1, nat.T1, form, 1.0, 0)
                oerr = _max_rel(older, conv + H)
                assert oerr < tol, oerr
                assert _max_rel(newer, older) > 1e-3 if eps > 0.0 else not np.array_equal(newer, older)
                if eps > 0.0:
                    nerr = _max_rel(newer, conv + H_moved)
                    print("  form %d after the move: pose 1 %.2e pose 0 %.2e" % (form, oerr, nerr))
                    assert nerr < tol, nerr
                launches += 2
        assert not ctx.get_state(nat.TCONV_1).any() and not ctx.get_state(nat.TCONV_2).any()
        assert np.array_equal(ctx.get_state(nat.T1), T)
        info = ctx.body_heat_info()
        assert info == dict(thermal=1 if name == "overlap" else len(bodies.bodies), fused_launches=launches,
                            recomputed=0), info
        assert ctx.scalar_info()["convection_launches"] == 0
    finally:
        ctx.close()


# ---------------------------------------------------------------- c. steps against the restatements
class _Run:
    """the device and the restatements side by side: cavity / lid flow with a body force, buoyancy b = _B, Dirichlet T on
    two sides and a source, the flow's penalisation and the scalar's (``bodies``; None: no bodies at all); ``plain`` is
    the scalar restatement without the term, driven with the same velocities"""

    def __init__(self, kind, typ, bodies, form=0, kappa=0.05, flow=True, temperatures=True):
        self.mesh, self.dm, self.marks, self.s, self.rs, make = _mesh(kind)
        dm, s = self.dm, self.s
        X = dm.p2_coords
        self.dim = dim = X.shape[1]
        self.k = _step_size(kind)
        self.bodies, self.with_flow = bodies, flow
        self.b = _B[:dim]
        self.vbc = cavity_bc(dm, self.marks) if dim == 2 else lid_bc(dm, self.marks)
        self.tbc = _two_sides(dm, self.marks, X)
        _, T_init = smooth_fields(X)
        q = np.cos(2.0 * X[:, 0] + 0.3) * np.sin(1.5 * X[:, 1] + 0.2)
        self.f = np.stack([np.sin(np.pi * X[:, 1]), -1.0 + X[:, 0], 0.5 * X[:, 1]][:dim], axis=1).ravel()
        name = ("standard", "skew_symmetric")[form]
        self.flow = IMEXPenalRestatement(s, _COEF, "standard", penal=None)
        self.orc = ScalarIMEXPenalRestatement(s, kappa, name)
        self.plain = ScalarIMEXPenalRestatement(s, kappa, name)
        for o in (self.orc, self.plain):
            o.source = q
            o.T[0], o.T[1] = T_init.copy(), T_init.copy()
        self.ctx = ctx = make(self.mesh, dm)
        try:
            ctx.set_coeffs(1.0, 1.0, 0.01, 1.0)
            ctx.set_dirichlet(nat.VELOCITY, *self.vbc)
            ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
            ctx.set_dirichlet(nat.SCALAR, *self.tbc)
            ctx.set_scalar(kappa, self.b, form)
            ctx.set_state(nat.BODY_FORCE, self.f)
            ctx.set_state(nat.T_SOURCE, q)
            ctx.set_state(nat.T0, T_init)
            ctx.set_state(nat.T1, T_init)
            if not flow:                    # a fixed smooth velocity at every level
                u, _ = smooth_fields(X)
                for slot in (nat.U0, nat.U1, nat.U2):
                    ctx.set_state(slot, u)
                self.flow.vel = [u.copy(), u.copy(), u.copy()]
            if bodies is not None:
                ctx.set_bodies(bodies.rows(0.0), bodies.eta, bodies.smoothing)
                if temperatures:
                    ctx.set_body_temperatures(*bodies.temperatures(), bodies.eta_scalar)
                self.pose(0.0)
            self.opts = _opts(ctx)
            self.ts = IMEXTimeStepping(0.0, 1.0e9, typ, desired_start_time_step=self.k)
        except BaseException:
            ctx.close()
            raise

    def pose(self, t):
        """the restatements' bodies at time t (N2 of either keeps the pose it was formed with)"""
        self.flow.penal = PenalisationRestatement(self.rs, self.bodies, t)
        self.orc.penal = ScalarPenalRestatement(self.rs, self.bodies, t) if self.bodies.thermal else None

    def step(self, tag="", move=False):
        ctx, ts = self.ctx, self.ts
        ts.update_coefficients()
        kk = ts.get_next_step_size()
        ctx.set_imex(ts.alpha, ts.beta, ts.gamma, kk)
        if move:
            ctx.move_bodies(self.bodies.rows(ts.current_time))
            self.pose(ts.current_time)
        si = ctx.step_scalar_imex(rtol=1e-13)
        u1, u2 = self.flow.vel[1], self.flow.vel[2]
        self.orc.step(ts.alpha, ts.beta, ts.gamma, kk, u1, u2, self.tbc)
        self.plain.step(ts.alpha, ts.beta, ts.gamma, kk, u1, u2, self.tbc)
        et = rel(ctx.get_state(nat.T0), self.orc.T[0])
        print("%s step %d k %.4g: T %.2e cg %d" % (tag, ts.step_number, kk, et, si.iterations))
        assert si.converged and et < 1e-9, (tag, et)
        if self.with_flow:
            self.flow.body_force = self.f + np.outer(self.orc.T[0], self.b).ravel()
            ctx.step_imex(self.opts)
            self.flow.step(ts.alpha, ts.beta, ts.gamma, kk, self.vbc, NO_PBC)
            us, u, p = ctx.get_state(nat.USTAR), ctx.get_state(nat.U0), ctx.get_state(nat.P)
            es, eu = rel(us, self.flow.ustar), rel(u, self.flow.vel[0])
            ep = rel(p - p.mean(), self.flow.p - self.flow.p.mean())
            print("%s        u* %.2e u %.2e p %.2e" % (tag, es, eu, ep))
            assert es < 1e-9 and eu < 1e-9 and ep < 1e-8, (tag, es, eu, ep)
        ctx.advance(0)
        self.orc.advance()
        self.plain.advance()
        if self.with_flow:
            self.flow.advance()
        ts.advance_time()

    def effect(self, tag):
        change = rel(self.orc.T[1], self.plain.T[1])
        print("%s: effect of H on T %.2e" % (tag, change))
        assert change > 1e-3
        return change


def _heated_disc(kind, eps=0.0):
    k = _step_size(kind)
    return heated_set(_dim(kind), "disc", 2.0 * k, eps, 2.0 * k)


@pytest.mark.parametrize("typ", (IMEXType.SBDF2, IMEXType.CNAB, IMEXType.mCNAB), ids=lambda t: t.name)
def test_steps_with_a_heated_disc_match_the_restatements(typ):
    """box(8, 8), 4 steps: cavity flow, buoyancy, the flow's penalisation and the sharp heated disc, eta = eta_T = 2 k"""
    run = _Run((8, 8), typ, _heated_disc((8, 8)))
    try:
        for _ in range(4):
            run.step("%s" % typ.name)
        run.effect(typ.name)
        info, hinfo = run.ctx.scalar_info(), run.ctx.body_heat_info()
        # one fused launch per step: C(u2) T2 + H(T2) is what the step before stored
        assert info["convection_launches"] == 4 and info["convection_reuses"] == 3 and info["dictionary"] is False, info
        assert hinfo == dict(thermal=1, fused_launches=4, recomputed=0), hinfo
        assert run.ctx.body_info() == dict(bodies=1, element_launches=4, recomputed=0)
    finally:
        run.ctx.close()


@pytest.mark.parametrize("kind,form,dictionary", [((16, 16), 0, True), ((8, 8), 1, False),
                                                  (((4, 4, 4), (1.0, 1.0, 1.0)), 0, False)], ids=str)
def test_sbdf2_steps_on_the_dictionary_path_in_the_skew_form_and_in_3d(kind, form, dictionary):
    """SBDF2, 4 steps with the smoothed heated disc / ball: box(16, 16) solves on the dictionary copy of the matrix,
    box(8, 8) runs the skew form of the fused kernel, the (4, 4, 4) Kuhn box the 3D one"""
    run = _Run(kind, IMEXType.SBDF2, _heated_disc(kind, EPS), form=form)
    try:
        for _ in range(4):
            run.step("%s form %d" % (kind, form))
        run.effect(str(kind))
        info = run.ctx.scalar_info()
        assert info["convection_launches"] == 4 and info["convection_reuses"] == 3, info
        assert info["dictionary"] is dictionary, info
        assert run.ctx.body_heat_info() == dict(thermal=1, fused_launches=4, recomputed=0)
    finally:
        run.ctx.close()


# ---------------------------------------------------------------- d. a moving disc and a step-size change
def test_a_moving_heated_disc_and_a_step_size_change_keep_the_stored_vector():
    """transport steps with a fixed smooth velocity and a smoothed disc that moves (nsfem_move_bodies before every
    step): the stored vector -- formed with the pose of t^(n-1) -- is reused in every step and never recomputed; the step
    size halves before step 3, which rebuilds the matrix and still reuses the vector"""
    kind = (8, 8)
    k = _step_size(kind)
    disc = Ball((0.4, 0.55), 0.2, motion=lambda t: ((0.4 + 0.4 * t, 0.55), (0.4, 0.0), 0.6), temperature=0.9)
    run = _Run(kind, IMEXType.SBDF2, ImmersedBodies([disc], 2.0 * k, EPS, 2.0 * k), flow=False)
    try:
        for i in range(5):
            if i == 2:
                run.ts.set_desired_next_step_size(0.5 * k)
            before = run.ctx.scalar_info()
            run.step("moving", move=True)
            info = run.ctx.scalar_info()
            assert info["convection_launches"] == before["convection_launches"] + 1
            assert info["convection_reuses"] == before["convection_reuses"] + (1 if i > 0 else 0), (i, info)
            if i == 2:
                assert info["matrix_builds"] == before["matrix_builds"] + 1
        run.effect("moving disc")
        assert run.ctx.body_heat_info() == dict(thermal=1, fused_launches=5, recomputed=0)
        # (with the pose of t^n for T2 instead the stored vector would differ visibly: the comparison is no tautology)
        older = ScalarPenalRestatement(run.rs, run.bodies, run.ts.previous_time).residual(run.orc.T[2])
        newer = ScalarPenalRestatement(run.rs, run.bodies, run.ts.current_time).residual(run.orc.T[2])
        assert rel(newer, older) > 1e-3
    finally:
        run.ctx.close()


# ---------------------------------------------------------------- e. the epoch
def test_new_thermal_data_recompute_the_stored_vector_once_and_the_same_data_do_not():
    kind = (8, 8)
    k = _step_size(kind)
    run = _Run(kind, IMEXType.SBDF2, _heated_disc(kind, EPS), flow=False)
    ctx = run.ctx
    try:
        def push(bodies, smoothing_only=False):
            run.bodies = bodies
            if smoothing_only:
                ctx.set_bodies(bodies.rows(), bodies.eta, bodies.smoothing)
            else:
                ctx.set_body_temperatures(*bodies.temperatures(), bodies.eta_scalar)
            run.pose(0.0)
            run.orc.N2 = None

        def counters():
            h, i = ctx.body_heat_info(), ctx.scalar_info()
            return h["recomputed"], h["fused_launches"], i["convection_launches"], i["convection_reuses"]

        for _ in range(2):
            run.step("epoch")
        assert counters() == (0, 2, 2, 1)
        same = run.bodies
        ctx.set_body_temperatures(*same.temperatures(), same.eta_scalar)                 # the same data again
        ctx.set_bodies(same.rows(), same.eta, same.smoothing)
        run.step("same data")
        assert counters() == (0, 3, 3, 2)
        disc = lambda T_s: heated(bodies_2d("disc"), (T_s, ))                           # noqa: E731
        push(ImmersedBodies(disc(-0.4), 2.0 * k, EPS, 2.0 * k))                          # a new T_s
        run.step("T_s")
        assert counters() == (1, 5, 5, 2)
        push(ImmersedBodies(disc(-0.4), 2.0 * k, EPS, 3.0 * k))                          # a new eta_T
        run.step("eta_T")
        assert counters() == (2, 7, 7, 2)
        run.step("unchanged")
        assert counters() == (2, 8, 8, 3)
        push(ImmersedBodies(disc(-0.4), 2.0 * k, 0.5 * EPS, 3.0 * k), smoothing_only=True)   # the body set (smoothing)
        assert ctx.body_heat_info()["thermal"] == 1                                      # (same count: temperatures kept)
        run.step("smoothing")
        assert counters() == (3, 10, 10, 3)
        run.effect("epoch")
        passive = ImmersedBodies(bodies_2d("disc"), 2.0 * k, 0.5 * EPS, 3.0 * k)         # the flag: no thermal body left
        push(passive)
        assert ctx.body_heat_info()["thermal"] == 0
        run.step("flag")                                                                  # (two plain launches)
        assert counters() == (4, 10, 12, 3)
        ctx.set_body_temperatures(*passive.temperatures(), 7.0 * k)                      # passive data: nothing to see
        run.step("passive")
        assert counters() == (4, 10, 13, 4)
    finally:
        ctx.close()


# ---------------------------------------------------------------- f. no temperatures
def test_no_temperatures_leave_the_steps_bit_identical():
    """bodies set (the flow's penalisation acts) and (1) the new entry points never called, (2) temperatures with all
    flags 0, (3) thermal data set, used once by the hook and removed with n = 0: T0 and the flow fields after 3 steps
    are the same bytes, the launch counts are equal, and no fused launch is made by a step"""
    kind = (8, 8)
    k = _step_size(kind)
    out, infos = [], []
    for mode in ("never", "flags 0", "removed"):
        bodies = ImmersedBodies(bodies_2d("overlap"), 2.0 * k, EPS, 2.0 * k)
        run = _Run(kind, IMEXType.SBDF2, bodies, temperatures=False)
        ctx = run.ctx
        try:
            if mode == "flags 0":
                ctx.set_body_temperatures([0, 0], [0.3, -1.0], 2.0 * k)
            elif mode == "removed":
                ctx.set_body_temperatures([1, 1], [0.3, -1.0], 2.0 * k)
                assert np.abs(ctx.body_scalar_residual(nat.U1, nat.T1, 0, 1.0, 0)).max() > 1e-3
                ctx.set_body_temperatures([], [])
            for _ in range(3):
                run.step(mode)
            out.append([ctx.get_state(slot) for slot in (nat.T0, nat.T1, nat.T2, nat.TCONV_2, nat.U0, nat.U1, nat.U2,
                                                         nat.USTAR, nat.P, nat.P_OLD, nat.CONV_N2)])
            infos.append((ctx.scalar_info(), ctx.body_info(), ctx.imex_info()))
            assert ctx.body_heat_info() == dict(thermal=0, fused_launches=1 if mode == "removed" else 0, recomputed=0)
        finally:
            ctx.close()
    assert infos[0][0]["convection_launches"] == 3 and infos[0][0]["convection_reuses"] == 2
    for other, info in zip(out[1:], infos[1:]):
        assert info == infos[0]
        for a, b in zip(out[0], other):
            assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- g. refusals
def test_everything_the_header_refuses_is_refused():
    mesh, dm, marks, s, rs, make = _mesh((8, 8))
    disc = (1, (0.5, 0.5), (0.2, ), (0.0, 0.0), 0.0)
    box = (2, (0.3, 0.3), (0.1, 0.1), (0.0, 0.0), 0.0)
    ctx = make(mesh, dm)
    try:
        with pytest.raises(nat.NativeError, match="no body set"):
            ctx.set_body_temperatures([1], [0.5], 0.1)
        ctx.set_body_temperatures([], [])                               # nothing to remove: allowed
        for call in (lambda: ctx.body_scalar_residual(nat.U1, nat.T1, 0, 1.0, 0), lambda: ctx.body_heat(nat.T1)):
            with pytest.raises(nat.NativeError, match="no body set"):
                call()
        ctx.set_bodies([disc, box], 0.1)
        for call in (lambda: ctx.body_scalar_residual(nat.U1, nat.T1, 0, 1.0, 0), lambda: ctx.body_heat(nat.T1)):
            with pytest.raises(nat.NativeError, match="no temperatures set"):
                call()
        for flags, values in (([1], [0.5]), ([1, 0, 1], [0.5, 0.0, 0.5])):
            with pytest.raises(nat.NativeError, match="another count"):
                ctx.set_body_temperatures(flags, values, 0.1)
        for flag in (2, -1):
            with pytest.raises(nat.NativeError, match="flag"):
                ctx.set_body_temperatures([1, flag], [0.5, 0.5], 0.1)
        for value in (np.nan, np.inf, -np.inf):
            with pytest.raises(nat.NativeError, match="temperature not finite"):
                ctx.set_body_temperatures([1, 0], [0.5, value], 0.1)
        for eta_T in (0.0, -0.1, np.nan, np.inf):
            with pytest.raises(nat.NativeError, match="eta_T"):
                ctx.set_body_temperatures([1, 0], [0.5, 0.5], eta_T)
        assert ctx.body_heat_info() == dict(thermal=0, fused_launches=0, recomputed=0)
        ctx.set_body_temperatures([1, 0], [0.5, 0.5], 0.1)
        assert ctx.body_heat_info()["thermal"] == 1
        for slot in (nat.P, nat.CONV_N1, nat.T0):
            with pytest.raises(nat.NativeError, match="velocity_slot"):
                ctx.body_scalar_residual(slot, nat.T1, 0, 1.0, 0)
        for slot in (nat.P, nat.U1, nat.TCONV_1):
            with pytest.raises(nat.NativeError, match="scalar slot"):
                ctx.body_scalar_residual(nat.U1, slot, 0, 1.0, 0)
            with pytest.raises(nat.NativeError, match="scalar slot"):
                ctx.body_heat(slot)
        with pytest.raises(nat.NativeError, match="form"):
            ctx.body_scalar_residual(nat.U1, nat.T1, 2, 1.0, 0)
        with pytest.raises(nat.NativeError, match="pose"):
            ctx.body_scalar_residual(nat.U1, nat.T1, 0, 1.0, 2)
        with pytest.raises(nat.NativeError, match="weight"):
            ctx.body_scalar_residual(nat.U1, nat.T1, 0, np.nan, 0)
        # the same count keeps the temperatures, another count drops them
        ctx.set_bodies([box, disc], 0.2)
        assert ctx.body_heat_info()["thermal"] == 1 and ctx.body_heat(nat.T1).shape == (2, 3)
        ctx.set_bodies([disc], 0.2)
        assert ctx.body_heat_info()["thermal"] == 0
        with pytest.raises(nat.NativeError, match="no temperatures set"):
            ctx.body_heat(nat.T1)
        ctx.set_body_temperatures([1], [0.5], 0.1)
        ctx.set_bodies([])
        assert ctx.body_heat_info()["thermal"] == 0
        with pytest.raises(nat.NativeError, match="no body set"):
            ctx.body_heat(nat.T1)
    finally:
        ctx.close()


# ---------------------------------------------------------------- h. through the classes
_SPEC = dict(name="Cavity", mesh=("cube", 2, 8), scheme="ipcs", clock=dict(dt=0.5 / 8, steps=3),
             numbers=dict(Re=100.0, Fr=1.0), start={"velocity": (0.0, 0.0), "pressure": 0.0, "temperature": 0.5},
             bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_slip", "bottom"), ("velocity", "top", (1.0, 0.0))])


def _problem(monkeypatch, bodies, solver_class=None, allow_stiff=False):
    from ns_boussinesq_solver import BoussinesqIMEXSolver
    from problem_specs import build_problem
    monkeypatch.setenv("NSFEM_NO_OUTPUT", "1")
    problem = build_problem(dict(_SPEC))
    cls = type(problem)

    def set_immersed_bodies(self):
        self._immersed_bodies = bodies
        self._immersed_allow_stiff = allow_stiff

    def set_temperature_coefficients(self):
        self._temperature_coefficients = dict(diffusivity=0.05, buoyancy=(0.0, 1.0), convective_form="standard")

    def set_temperature_boundary_conditions(self):
        self._temperature_bcs = [(self._sides["left"], 1.0), (self._sides["right"], 0.0)]
    cls.set_immersed_bodies = set_immersed_bodies
    cls.set_temperature_coefficients = set_temperature_coefficients
    cls.set_temperature_boundary_conditions = set_temperature_boundary_conditions
    problem.set_solver_class(solver_class or BoussinesqIMEXSolver)
    problem.compute_cfl = False
    return problem


def test_boussinesq_solver_with_heated_bodies_equals_driving_the_steps_by_hand(monkeypatch):
    """BoussinesqIMEXSolver through InstationaryProblem.solve_problem with the set_immersed_bodies hook on the 8 x 8
    cavity -- a heated disc that moves and a passive box --, 3 steps: bit for bit what set_bodies /
    set_body_temperatures / move_bodies / step_scalar_imex / step_imex / advance give through the C ABI; the output
    helper returns the device's heat numbers"""
    from multigrid import attach_hierarchy
    from ns_boussinesq_solver import BoussinesqIMEXSolver
    steps, dt = _SPEC["clock"]["steps"], _SPEC["clock"]["dt"]
    disc = Ball((0.4, 0.7), 0.15, motion=lambda t: ((0.4 + 0.3 * t, 0.7), (0.3, 0.0), 0.0), temperature=1.5)
    bodies = ImmersedBodies([disc, Box((0.5, 0.25), (0.2, 0.1))], 2.0 * dt, 0.05, eta_scalar=1.5 * dt)
    problem = _problem(monkeypatch, bodies)
    problem.solve_problem()
    solver = problem._get_solver()
    assert isinstance(solver, BoussinesqIMEXSolver) and problem._time_stepping.step_number == steps
    assert solver._ctx.body_heat_info() == dict(thermal=1, fused_launches=steps, recomputed=0)
    assert solver._ctx.body_info() == dict(bodies=2, element_launches=steps, recomputed=0)
    T_cls, u_cls = solver._ctx.get_state(nat.T1), solver._ctx.get_state(nat.U1)
    heat = problem._compute_body_heat()
    raw = solver._ctx.body_heat(nat.T0)
    assert heat.shape == (2, 3) and np.array_equal(heat[:, :2], raw[:, :2])
    assert np.array_equal(heat[:, 2], raw[:, 2] / raw[:, 0])
    assert heat[0, 1] < 0.0 and heat[1, 1] == 0.0 and 0.5 < heat[0, 2] < 1.5     # (the disc heats the fluid at 0.5)
    # ---- the same steps through the C ABI on a fresh context
    dm, mesh = solver._dofmap, solver._mesh
    left = np.unique(dm.facet_p2_nodes(solver._boundary_markers.facets_with_id(problem._sides["left"])))
    right = np.unique(dm.facet_p2_nodes(solver._boundary_markers.facets_with_id(problem._sides["right"])))
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
        ctx.set_scalar(0.05, (0.0, 1.0), 0)
        for slot in (nat.T0, nat.T1):
            ctx.set_state(slot, np.full(dm.n_p2, 0.5))
        ctx.set_bodies(bodies.rows(0.0), bodies.eta, bodies.smoothing)
        ctx.set_body_temperatures(*bodies.temperatures(), bodies.eta_scalar)
        opts = solver._step_options()
        ts = IMEXTimeStepping(0.0, 1.0, IMEXType.SBDF2, desired_start_time_step=dt)
        for _ in range(steps):
            ts.update_coefficients()
            ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
            ctx.move_bodies(bodies.rows(ts.current_time))
            ctx.step_scalar_imex(rtol=solver.krylov_rtol, max_iter=solver.krylov_max_iter)
            ctx.step_imex(opts)
            ts.advance_time()
            ctx.advance(0)
        T_abi, u_abi = ctx.get_state(nat.T1), ctx.get_state(nat.U1)
        # ... and without the temperatures the scalar differs visibly
        ctx.set_body_temperatures([], [])
    finally:
        ctx.close()
    assert np.abs(u_cls).max() > 0.5 and np.abs(T_cls - 0.5).max() > 1e-2
    assert np.array_equal(T_cls, T_abi) and np.array_equal(u_cls, u_abi)
    # the same set handed over again in the middle of the run: the temperatures follow the bodies
    calls = []
    real = solver._ctx.set_body_temperatures
    monkeypatch.setattr(solver._ctx, "set_body_temperatures",
                        lambda flags, values, *a: (calls.append((list(flags), list(values)) + a), real(flags, values, *a))[1])
    solver.set_immersed_bodies(bodies)
    assert calls == [([1, 0], [1.5, 0.0], bodies.eta_scalar)], calls
    assert solver._ctx.body_heat_info()["recomputed"] == 0
    solver.set_immersed_bodies(ImmersedBodies([Box((0.5, 0.25), (0.2, 0.1))], 2.0 * dt))      # a passive set
    assert calls[-1] == ([], []) and solver._ctx.body_heat_info()["thermal"] == 0
    monkeypatch.undo()
    solver.set_immersed_bodies(None)
    with pytest.raises(RuntimeError, match="no body set"):
        problem._compute_body_heat()


def test_boussinesq_solver_refuses_scalar_steps_above_the_stability_bound(monkeypatch):
    """k / eta_scalar above 4/3 under SBDF2 raises ValueError although k / eta is fine, allow_stiff lets it run; CNLF
    always raises"""
    from ns_boussinesq_solver import BoussinesqIMEXSolver
    dt, steps = _SPEC["clock"]["dt"], _SPEC["clock"]["steps"]
    hot = Ball((0.5, 0.5), 0.2, temperature=1.0)
    ok = ImmersedBodies([hot], dt / 1.0, eta_scalar=dt / 1.3)
    stiff = ImmersedBodies([hot], dt / 1.0, eta_scalar=dt / 1.4)
    problem = _problem(monkeypatch, ok)
    problem.solve_problem()
    assert problem._get_solver()._ctx.body_heat_info()["fused_launches"] == steps
    with pytest.raises(ValueError, match="k / eta_scalar"):
        _problem(monkeypatch, stiff).solve_problem()
    problem = _problem(monkeypatch, stiff, allow_stiff=True)
    problem.solve_problem()
    assert problem._get_solver()._ctx.body_heat_info()["fused_launches"] == steps

    class LeapfrogSolver(BoussinesqIMEXSolver):
        imex_type = IMEXType.CNLF
    with pytest.raises(ValueError, match="CNLF"):
        _problem(monkeypatch, ImmersedBodies([hot], 1.0e3 * dt), LeapfrogSolver).solve_problem()
