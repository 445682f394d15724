"""The composed IMEX step -- flow and scalar with every explicit term at once -- as one cache-free host definition: the
oracle of tests/test_gpu_imex_composed.py, checked without a GPU by tests/test_imex_composed_host.py.

Nothing here is new numerics.  The pieces are the ones the suite already trusts: fem_oracle.Space operators and
``convection_residual``, ``rule_space`` and ``VariableViscosityRestatement.residual``, ``PenalisationRestatement
.residual``, ``RotatingIMEXRestatement.coriolis_matrix`` and its Euler bracket, ``ScalarPenalRestatement`` and the scalar
convection matrix of ``ScalarIMEXRestatement``; the solves are fem_oracle.linear_solve_dirichlet (sparse LU).

What is new is that the class keeps NO stored explicit vector: the older restatements mirror the device's cache (their
N2 is the N1 of the step before), so a key that is missing from the device's validity rule is missing from them too.
Here every step forms both levels afresh from the *settings* the caller last installed, which is the definition a
reuse on the device has to be equivalent to: a reuse is legal exactly when recomputing would give the same vector."""
import numpy as np

import fem_oracle as fo
from gpu_common import cavity_bc
from imex_time_stepping import IMEXTimeStepping
from immersed_bodies import Ball, Box, ImmersedBodies
from test_heated_bodies_host import ScalarPenalRestatement
from test_imex_rotation_host import RotatingIMEXRestatement
from test_immersed_bodies_host import PenalisationRestatement
from test_scalar_transport_host import ScalarIMEXRestatement, smooth_fields
from test_variable_viscosity_host import VariableViscosityRestatement

NO_BC = (np.zeros(0, np.int64), np.zeros(0))
FLOW_FORMS = ("standard", "rotational", "divergence", "skew_symmetric")
SCALAR_FORMS = ("standard", "skew_symmetric")
#: the rules of the class that tests/test_imex_composed_host.py reverts one at a time (``revert``)
RULES = ("pose", "omega", "order", "law", "eta_T")


class _ThermalView:
    """the body set as ScalarPenalRestatement reads it, with the thermal data installed separately from the bodies
    (nsfem_set_body_temperatures): flags, temperatures and eta_T of the settings, poses and smoothing of the set"""

    def __init__(self, bodies, flags, values, eta_scalar):
        self.bodies, self.smoothing, self.eta_scalar = bodies.bodies, bodies.smoothing, float(eta_scalar)
        self._set = bodies
        self._flags, self._values = np.asarray(flags, dtype=np.int32), np.asarray(values, dtype=np.float64)

    def winner(self, X, t=None):
        return self._set.winner(X, t)

    def temperatures(self):
        return self._flags, np.where(self._flags == 1, self._values, 0.0)


class ComposedIMEX:
    """alpha = (a0, a1, a2), beta = (b0, b1), gamma = (g0, g1, g2) of IMEXTimeStepping, step size k.  Level "n" is that
    of u1 / T1 (index 0 of the per-level settings), level "n-1" that of u2 / T2 (index 1).

    Explicit vector of a level:
        N(u, level) = c_c conv_form(u) + M (2 c_cor Omega_level x u) + V_law(u) + B_(pose_level)(u)
    V is added before B (the device's order); a term that is switched off adds nothing.
    Flow step: the three steps of IMEXRestatement with b0 N(u1, n) + b1 N(u2, n-1); the traction form is in K; the
    mass-weighted bracket holds - c_b (f + T0 b) (body force and Boussinesq buoyancy) and + c_e (dOmega/dt x x); the
    traction vector is added.
    Scalar step: that of ScalarIMEXRestatement with b0 (C_form(u1) T1 + H_(pose_n)(T1)) + b1 (C_form(u2) T2 +
    H_(pose_(n-1))(T2)), plus the source.

    Settings (what the caller last installed; the ``set_*`` methods carry the names of the device's calls):
    convective form and c_c (``form``, ``c``), law and parameters, the body set with eta and smoothing and the two poses
    (``set_bodies`` gives one pose for both levels, ``move_bodies`` shifts them), thermal flags, T_s and eta_T, Omega per
    level as given to ``set_imex_rotation`` or the single Omega of ``set_angular_velocity`` for a level not given,
    scalar form and kappa.

    No explicit vector is kept from one step to the next.  ONE deliberate exception: a vector written through
    ``vouch_N2`` / ``vouch_TN2`` -- nsfem_set_state of NSFEM_CONV_N2 / NSFEM_TCONV_2 -- is the caller's vouched vector
    for level n-1 and is used as given for the one step that follows; ``advance`` drops it.  (The device agrees as long
    as no setting changes between the vouching call and the step; what it does when one changes is written down in
    INTEGRATION.md and is not part of this definition.)

    ``revert``: a set of names from RULES, each of which replaces one rule by the mistake a driver could make; used only
    by the host tests that show the named tests can fail."""

    def __init__(self, space, rspace, coeffs, traction_form=False):
        s = self.s = space
        self.rs = rspace
        self.c = dict(coeffs)
        self.M, self.D, self.G, self.Ap = s.vector_mass(), s.divergence(), s.pressure_gradient(), s.stiffness_p1()
        self._K = {}
        self._Mp2 = s.mass_p2()
        self.K2 = s.stiffness_p2()
        self.traction_form = bool(traction_form)
        # levels
        self.vel = [np.zeros(s.dim * s.n2) for _ in range(3)]
        self.ustar = np.zeros(s.dim * s.n2)
        self.p, self.p_old = np.zeros(s.n1), np.zeros(s.n1)
        self.T = [np.zeros(s.n2) for _ in range(3)]
        self.body_force = self.traction = self.source = None
        # settings
        self.form, self.scalar_form = "standard", "standard"
        self.law, self.law_params = 0, ()
        self.bodies, self.poses = None, [None, None]
        self.thermal = None                                 # (flags, values, eta_T)
        zero = 0.0 if s.dim == 2 else np.zeros(3)
        self.omega, self.omega_dot, self.omega_levels = zero, zero, [None, None]
        self.rotation = False
        self.kappa, self.buoyancy = 0.0, None
        # the vouched vectors and the last explicit vectors formed (for comparison only; never read by a step)
        self._vouched_N2 = self._vouched_TN2 = None
        self.N1 = self.N2 = self.TN1 = self.TN2 = None
        self.revert = set()
        self._law_before = (0, ())
        self._memo = {}
        self._scalar_ops = {}

    # ---------------------------------------------------------------- settings
    def set_viscosity_law(self, law, params=()):
        self._law_before = (self.law, self.law_params)
        self.law, self.law_params = int(law), tuple(float(p) for p in params) if law else ()

    def set_bodies(self, bodies, t=None):
        """``bodies``: an ImmersedBodies or None; ``t``: the time of the one pose both levels get"""
        self.bodies, self.poses = bodies, [t, t]
        if bodies is None or (self.thermal is not None and len(self.thermal[0]) != len(bodies.bodies)):
            self.thermal = None                             # (temperatures belong to the bodies by index)

    def move_bodies(self, t):
        self.poses = [t, self.poses[0]]

    def set_body_temperatures(self, flags, values, eta_scalar=1.0):
        flags = np.asarray(flags, dtype=np.int32)
        self.thermal = (flags, np.asarray(values, dtype=np.float64), float(eta_scalar)) if flags.size else None

    def set_angular_velocity(self, omega, omega_dot=None):
        self.omega = omega
        self.omega_dot = (0.0 if self.s.dim == 2 else np.zeros(3)) if omega_dot is None else omega_dot

    def set_imex_rotation(self, treatment, omega_n=None, omega_nm1=None):
        self.rotation = bool(treatment)
        self.omega_levels = [omega_n, omega_nm1] if treatment else [None, None]

    def set_scalar(self, kappa, buoyancy=None, form=0):
        self.kappa, self.scalar_form = float(kappa), SCALAR_FORMS[form] if isinstance(form, int) else form
        self.buoyancy = None if buoyancy is None or not np.any(buoyancy) else np.asarray(buoyancy, dtype=np.float64)

    def vouch_N2(self, vector):
        self._vouched_N2 = np.array(vector, dtype=np.float64)

    def vouch_TN2(self, vector):
        self._vouched_TN2 = np.array(vector, dtype=np.float64)

    # ---------------------------------------------------------------- the terms
    def _stiffness(self):
        if self.traction_form not in self._K:
            self._K[self.traction_form] = self.s.vector_stiffness(self.traction_form)
        return self._K[self.traction_form]

    coriolis_matrix = RotatingIMEXRestatement.coriolis_matrix

    def omega_of(self, level):
        if not self.rotation:
            return 0.0 if self.s.dim == 2 else np.zeros(3)
        if "omega" in self.revert:
            level = 0
        w = self.omega_levels[level]
        return self.omega if w is None else w

    def _signature(self, t):
        """what a pose object depends on (the memo below holds constructed restatements, never a vector)"""
        rows = self.bodies.rows(t)
        return (self.bodies.eta, self.bodies.smoothing,
                b"".join(np.asarray(x, dtype=np.float64).tobytes() for r in rows for x in (r[0], ) + tuple(r[1:])))

    def _penal(self, level):
        t = self.poses[0 if "pose" in self.revert else level]
        key = ("B", self._signature(t))
        if key not in self._memo:
            self._memo[key] = PenalisationRestatement(self.rs, self.bodies, t)
        return self._memo[key]

    def _heat(self, level):
        """ScalarPenalRestatement of the level's pose, None without a thermal body"""
        if self.bodies is None or self.thermal is None or not (self.thermal[0] == 1).any():
            return None
        flags, values, eta_T = self.thermal
        if "eta_T" in self.revert:
            eta_T = self.bodies.eta
        t = self.poses[0 if "pose" in self.revert else level]
        key = ("H", self._signature(t), flags.tobytes(), values.tobytes(), eta_T)
        if key not in self._memo:
            self._memo[key] = ScalarPenalRestatement(self.rs, _ThermalView(self.bodies, flags, values, eta_T), t)
        return self._memo[key]

    def terms(self, u, level):
        """the switched-on terms of N(u, level) in the order they are added: [(name, vector)]"""
        c = self.c
        out = []
        cc = c.get("convective_term") or 0.0
        if cc:
            out.append(("convection", cc * self.s.convection_residual(u, self.form)))
        w = self.omega_of(level)
        if np.any(w):
            out.append(("coriolis", 2.0 * c["coriolis_term"] * (self.coriolis_matrix(w) @ u)))
        law, params = self.law, self.law_params
        if "law" in self.revert and level == 1:
            law, params = self._law_before
        V = B = None
        if law:
            V = ("viscosity", VariableViscosityRestatement(self.rs, law, params).residual(u))
        if self.bodies is not None:
            B = ("bodies", self._penal(level).residual(u))
        out += [x for x in ((B, V) if "order" in self.revert else (V, B)) if x is not None]
        return out

    def explicit(self, u, level):
        N = np.zeros_like(u)
        for _, v in self.terms(u, level):
            N = N + v
        return N

    def bracket(self):
        """- c_b (f + T0 b) + c_e (dOmega/dt x x), nodal, to be weighted with M; None when nothing is in it"""
        c = self.c
        out = None
        f = self.body_force
        if self.buoyancy is not None:
            f = (0.0 if f is None else f) + np.outer(self.T[0], self.buoyancy).ravel()
        if f is not None:
            out = -c["body_force_term"] * f
        if self.rotation and np.any(self.omega_dot):
            X = self.s.p2_nodes()
            if self.s.dim == 2:
                e = c["euler_term"] * float(self.omega_dot) * np.stack([-X[:, 1], X[:, 0]], axis=1).ravel()
            else:
                e = c["euler_term"] * np.cross(np.asarray(self.omega_dot, dtype=float)[None, :], X).ravel()
            out = e if out is None else out + e
        return out

    # ---------------------------------------------------------------- the flow step
    def rhs(self, alpha, beta, gamma, k):
        """right-hand side of the diffusion step before the Dirichlet rows; sets N1, N2"""
        c = self.c
        cp, cv = c["pressure_term"], c["viscous_term"]
        u1, u2 = self.vel[1], self.vel[2]
        K = self._stiffness()
        self.N1 = self.explicit(u1, 0)
        if beta[1] == 0.0:
            self.N2 = np.zeros_like(u1)
        elif self._vouched_N2 is not None:
            self.N2 = self._vouched_N2
        else:
            self.N2 = self.explicit(u2, 1)
        b = self.M @ (alpha[1] * u1 + alpha[2] * u2) / k + cv * (K @ (gamma[1] * u1 + gamma[2] * u2))
        b += beta[0] * self.N1 + beta[1] * self.N2 - cp * (self.D.T @ self.p_old)
        br = self.bracket()
        if br is not None:
            b += self.M @ br
        if self.traction is not None:
            b += self.traction
        return -b

    def step(self, alpha, beta, gamma, k, vel_bc, p_bc=NO_BC):
        a0, g0 = alpha[0], gamma[0]
        A = (a0 / k) * self.M + g0 * self.c["viscous_term"] * self._stiffness()
        self.ustar = fo.linear_solve_dirichlet(A, self.rhs(alpha, beta, gamma, k), *vel_bc)
        r = self.Ap @ self.p_old - (a0 / k) * (self.D @ self.ustar)
        self.p = fo.linear_solve_dirichlet(self.Ap, r, *p_bc, pin_nullspace=(len(p_bc[0]) == 0))
        r = self.M @ self.ustar - (k / a0) * (self.G @ (self.p - self.p_old))
        self.vel[0] = fo.linear_solve_dirichlet(self.M, r, *vel_bc)

    # ---------------------------------------------------------------- the scalar step
    def _scalar(self):
        if self.scalar_form not in self._scalar_ops:
            self._scalar_ops[self.scalar_form] = ScalarIMEXRestatement(self.s, 0.0, self.scalar_form)
        return self._scalar_ops[self.scalar_form]

    def scalar_terms(self, u, T, level):
        out = [("convection", self._scalar().convection_matrix(u) @ T)]
        heat = self._heat(level)
        if heat is not None:
            out.append(("heat", heat.residual(T)))
        return out

    def scalar_explicit(self, u, T, level):
        return sum(v for _, v in self.scalar_terms(u, T, level))

    def scalar_rhs(self, alpha, beta, gamma, k):
        T1, T2 = self.T[1], self.T[2]
        M = self._Mp2
        self.TN1 = self.scalar_explicit(self.vel[1], T1, 0)
        if beta[1] == 0.0:
            self.TN2 = np.zeros_like(T1)
        elif self._vouched_TN2 is not None:
            self.TN2 = self._vouched_TN2
        else:
            self.TN2 = self.scalar_explicit(self.vel[2], T2, 1)
        b = M @ (alpha[1] * T1 + alpha[2] * T2) / k + self.kappa * (self.K2 @ (gamma[1] * T1 + gamma[2] * T2))
        b += beta[0] * self.TN1 + beta[1] * self.TN2
        rhs = -b
        if self.source is not None:
            rhs += M @ self.source
        return rhs

    def step_scalar(self, alpha, beta, gamma, k, bc=NO_BC):
        A = (alpha[0] / k) * self._Mp2 + gamma[0] * self.kappa * self.K2
        self.T[0] = fo.linear_solve_dirichlet(A.tocsr(), self.scalar_rhs(alpha, beta, gamma, k), *bc)

    # ---------------------------------------------------------------- between steps
    def advance(self, scalar=True):
        self.vel[2] = self.vel[1].copy()
        self.vel[1] = self.vel[0].copy()
        self.p_old = self.p.copy()
        if scalar:
            self.T[2] = self.T[1].copy()
            self.T[1] = self.T[0].copy()
        self._vouched_N2 = self._vouched_TN2 = None
        self._law_before = (self.law, self.law_params)


# ================================================================ the cases of tests/test_gpu_imex_composed.py
# (inputs only: meshes, fields, settings, event lists.  Both the GPU module and tests/test_imex_composed_host.py build
# their runs from here, so the host file can state what every GPU case contains without a GPU.)
EPS = 0.07
SMAGORINSKY, CARREAU = 1, 2
LAWS = {SMAGORINSKY: (0.9, ), CARREAU: (0.07, 1.7, 0.6)}
CUBE = ((4, 4, 4), (1.0, 1.0, 1.0))
RHS_MESHES = [(8, 8), (16, 16), "mapped", CUBE]
#: coefficients of the right-hand-side cases (those of tests/test_gpu_imex_rotation.py's hook test)
RHS_COEF = dict(convective_term=0.8, pressure_term=1.0, viscous_term=0.02, body_force_term=0.7, coriolis_term=1.5,
                euler_term=0.7)
SBDF2_LATER = ((1.5, -2.0, 0.5), (2.0, -1.0), (1.0, 0.0, 0.0))
RHS_K = 1.0 / 64.0
RHS_ETA = 0.037
#: pose times of the two levels in the right-hand-side cases
RHS_T = (0.2, 0.0)
STEP_COEF = dict(convective_term=1.0, pressure_term=1.0, viscous_term=0.01, body_force_term=1.0, coriolis_term=1.5,
                 euler_term=0.7)
CS_STEPS = 0.2
#: the laws of the step runs (those of the step tests of tests/test_gpu_variable_viscosity.py)
STEP_LAWS = {SMAGORINSKY: (CS_STEPS, ), CARREAU: (0.008, 1.0, 0.5)}
BUOYANCY = (0.3, 1.0, -0.4)
KAPPA = 0.05


def dim_of(kind):
    return 2 if kind == "mapped" or isinstance(kind[0], int) else 3


def step_size(kind):
    n = kind[0] if isinstance(kind[0], int) else (8 if kind == "mapped" else kind[0][0])
    return 0.5 / n


def _axis(dim):
    """2D: rotation about e_z (a number); 3D: a fixed direction scaled by the same number"""
    return 1.0 if dim == 2 else np.array([0.2, -0.3, 1.0])


def _drift(c0, v, w):
    c0, v = np.asarray(c0, dtype=float), np.asarray(v, dtype=float)
    return lambda t: (tuple(c0 + t * v), tuple(v), w)


def moving_pair(dim, eta, eps, eta_scalar=None):
    """the "overlap" pair of the body modules (disc / ball and box), both translating and spinning"""
    if dim == 2:
        disc = Ball((0.43, 0.57), 0.21, motion=_drift((0.43, 0.57), (0.3, -0.2), 0.7))
        box_ = Box((0.55, 0.4), (0.17, 0.23), motion=_drift((0.55, 0.4), (-0.1, 0.25), -0.4))
    else:
        disc = Ball((0.43, 0.37, 0.31), 0.23, motion=_drift((0.43, 0.37, 0.31), (0.3, -0.2, 0.15), (0.7, -0.4, 0.5)))
        box_ = Box((0.55, 0.4, 0.33), (0.17, 0.23, 0.19),
                   motion=_drift((0.55, 0.4, 0.33), (-0.1, 0.25, 0.05), (0.0, -0.4, 0.2)))
    return ImmersedBodies([disc, box_], eta, eps, eta_scalar)


def moving_disc(eta, eps=0.0):
    """the disc of the body modules, translating and spinning (2D; used with the sharp mask on the box meshes)"""
    return ImmersedBodies([Ball((0.43, 0.57), 0.21, motion=_drift((0.43, 0.57), (0.3, -0.2), 0.7))], eta, eps)


def heated_pair(dim, eta, eps, eta_scalar, T_s=0.9):
    """a heated disc / ball that translates and spins, and a passive box at rest"""
    if dim == 2:
        disc = Ball((0.4, 0.55), 0.2, motion=_drift((0.4, 0.55), (0.4, 0.0), 0.6), temperature=T_s)
        box_ = Box((0.55, 0.25), (0.17, 0.1))
    else:
        disc = Ball((0.4, 0.5, 0.45), 0.25, motion=_drift((0.4, 0.5, 0.45), (0.4, 0.0, 0.1), (0.0, 0.3, 0.6)),
                    temperature=T_s)
        box_ = Box((0.6, 0.3, 0.3), (0.17, 0.1, 0.15))
    return ImmersedBodies([disc, box_], eta, eps, eta_scalar)


def rhs_fields(s):
    """u1, u2, p_old, f, traction: smooth, non-polynomial, no symmetry; different at the two levels"""
    X, dim = s.p2_nodes(), s.dim
    u1, _ = smooth_fields(X)
    u2 = 0.9 * smooth_fields(0.8 * X[:, ::-1] + 0.1)[0]
    P = s.p1_nodes()
    p_old = np.sin(2.0 * P[:, 0] + 0.3) * np.cos(1.7 * P[:, 1] - 0.2)
    f = np.stack([np.sin(np.pi * X[:, 1]), -1.0 + X[:, 0], 0.5 * X[:, 1]][:dim], axis=1).ravel()
    tr = 0.05 * np.stack([np.cos(1.1 * X[:, 0]), np.sin(0.9 * X[:, 1] + 0.4), np.cos(0.7 * X[:, 0] + 0.2)][:dim],
                         axis=1).ravel()
    return u1, u2, p_old, f, tr


RHS_OMEGA = (0.7, -0.4, 0.3)            # Omega_n, Omega_(n-1), dOmega/dt (times _axis in 3D)


def rhs_body_sets(kind):
    """[(name, ImmersedBodies)]: the smoothed moving pair everywhere, plus the sharp moving disc on the box meshes"""
    sets = [("pair", moving_pair(dim_of(kind), RHS_ETA, EPS))]
    if kind in ((8, 8), (16, 16)):
        sets.append(("sharp disc", moving_disc(RHS_ETA, 0.0)))
    return sets


def rhs_law(form_id, traction):
    """Smagorinsky / Carreau alternating over the cases"""
    return (SMAGORINSKY, CARREAU)[(form_id + int(traction)) % 2]


def rhs_case(s, rs, kind, form_id, traction, bodies, ctx=None, nat=None):
    """a ComposedIMEX with everything on for one right-hand-side case; with ``ctx`` the same calls go to the device"""
    dim = s.dim
    u1, u2, p_old, f, tr = rhs_fields(s)
    law = rhs_law(form_id, traction)
    ax = _axis(dim)
    w1, w2, wd = (RHS_OMEGA[i] * ax for i in range(3))
    h = ComposedIMEX(s, rs, RHS_COEF, traction_form=traction)
    h.form = FLOW_FORMS[form_id]
    h.vel[1], h.vel[2], h.p_old, h.body_force = u1, u2, p_old, f
    h.traction = tr if traction else None
    h.set_viscosity_law(law, LAWS[law])
    h.set_bodies(bodies, RHS_T[1])
    h.move_bodies(RHS_T[0])
    h.set_angular_velocity(w1, wd)
    h.set_imex_rotation(1, w1, w2)
    if ctx is not None:
        c = RHS_COEF
        ctx.set_coeffs(c["convective_term"], c["pressure_term"], c["viscous_term"], c["body_force_term"],
                       c["coriolis_term"], c["euler_term"])
        ctx.set_viscous_form(traction)
        for slot, v in ((nat.U1, u1), (nat.U2, u2), (nat.P_OLD, p_old), (nat.BODY_FORCE, f)):
            ctx.set_state(slot, v)
        if traction:
            ctx.set_state(nat.TRACTION, tr)
        ctx.set_viscosity_law(law, LAWS[law])
        ctx.set_bodies(bodies.rows(RHS_T[1]), bodies.eta, bodies.smoothing)
        ctx.move_bodies(bodies.rows(RHS_T[0]))
        ctx.set_angular_velocity(w1, wd)
        ctx.set_imex_rotation(1, w1, w2)
        ctx.set_imex(*SBDF2_LATER, RHS_K)
    return h


def rhs_parts(h, alpha, beta, gamma, k):
    """the right-hand side of ``h`` split into the parts a tolerance is summed over:
    {"operators": linear part (mass, stiffness, pressure, bracket, traction vector), name: - (b0 term(u1) + b1 term(u2))}
    and the same for N1: {name: term(u1)}"""
    full = h.rhs(alpha, beta, gamma, k)
    parts, n1_parts = {}, {}
    t2 = dict(h.terms(h.vel[2], 1)) if beta[1] != 0.0 else {}
    for name, v in h.terms(h.vel[1], 0):
        n1_parts[name] = v
        parts[name] = -(beta[0] * v + beta[1] * t2.get(name, 0.0))
    parts["operators"] = full - sum(parts.values())
    return full, parts, n1_parts


# ---------------------------------------------------------------- steps with everything on, and the events
def omega_of_time(dim, t):
    """Omega(t) = 0.5 + 0.8 t about the axis of ``_axis``; dOmega/dt = 0.8"""
    return (0.5 + 0.8 * t) * _axis(dim)


#: code -> what happens between two steps (ComposedRun.apply); the codes go into the test ids
EVENTS = {
    "lp": "new law parameters", "l2": "law 1 <-> 2", "l0": "law -> 0 -> back",
    "be": "set_bodies with another eta", "bs": "set_bodies with the same table again",
    "mv": "move_bodies to a pose off the path", "ts": "set_body_temperatures with a new T_s",
    "tt": "the same thermal data again", "pb": "a passive body added / removed",
    "wg": "Omega levels given", "wn": "Omega levels not given", "w2": "Omega of level n-1 changed for one step",
    "cc": "c_c changed through set_coeffs", "cf": "convective form changed through the step options",
    "sf": "scalar form changed", "dk": "step size changed",
    "u2": "set_state of U2", "t2": "set_state of T2", "u1": "set_state of U1",
    "ns": "advance after a flow step without a scalar step",
}


class ComposedRun:
    """cavity / lid flow with a body force, Boussinesq buoyancy, rotation varying in time, a Smagorinsky law, a heated
    moving disc / ball and a passive box (smoothed), Dirichlet T on two sides and a source: the cache-free host
    ``self.h`` and any number of device contexts receive the same calls.  ``observer(action, *args)`` is told every
    call that can move a validity key (the counter model of the GPU module listens there).

    Per time step: set_imex, move_bodies(pose of t^n), set_angular_velocity(Omega(t^(n+1)), dOmega/dt),
    set_imex_rotation, step_scalar_imex, step_imex, advance."""

    def __init__(self, kind, typ, mesh_tuple, contexts=(), nat=None, observer=None, levels_given=True):
        self.kind, self.typ, self.nat = kind, typ, nat
        self.mesh, self.dm, self.marks, self.s, self.rs, _ = mesh_tuple
        self.ctxs = list(contexts)
        self.observer = observer or (lambda *a: None)
        dm, s = self.dm, self.s
        X = dm.p2_coords
        self.dim = dim = X.shape[1]
        self.k = step_size(kind)
        if dim == 2:
            self.vbc = cavity_bc(dm, self.marks)
        else:
            from test_gpu_3d import lid_bc
            self.vbc = lid_bc(dm, self.marks)
        left = np.unique(dm.facet_p2_nodes(self.marks.facets_with_id(1)))
        right = np.unique(dm.facet_p2_nodes(self.marks.facets_with_id(2)))
        self.tbc = (np.concatenate([left, right]), np.concatenate([0.5 + X[left, 1], -0.2 + 0.0 * X[right, 1]]))
        self.pbc = (np.zeros(0, np.int32), np.zeros(0))
        _, T_init = smooth_fields(X)
        self.q = np.cos(2.0 * X[:, 0] + 0.3) * np.sin(1.5 * X[:, 1] + 0.2)
        self.f = np.stack([np.sin(np.pi * X[:, 1]), -1.0 + X[:, 0], 0.5 * X[:, 1]][:dim], axis=1).ravel()
        self.b = BUOYANCY[:dim]
        self.coef = dict(STEP_COEF)
        self.form_id, self.scalar_form = 0, 0
        self.law, self.law_params = SMAGORINSKY, STEP_LAWS[SMAGORINSKY]
        self.eta, self.eta_T, self.T_s, self.extra_body = 2.0 * self.k, 1.5 * self.k, 0.9, False
        self.levels_given = levels_given
        self.once = {}                                     # modifiers of the next step only
        self.step_index = 0
        self.ts = IMEXTimeStepping(0.0, 1.0e9, typ, desired_start_time_step=self.k)
        h = self.h = ComposedIMEX(s, self.rs, self.coef)
        h.body_force, h.source = self.f, self.q
        h.T[0], h.T[1] = T_init.copy(), T_init.copy()
        h.set_scalar(KAPPA, self.b, 0)
        h.set_viscosity_law(self.law, self.law_params)
        self.bodies = self._make_bodies()
        h.set_bodies(self.bodies, 0.0)
        h.set_body_temperatures(*self.bodies.temperatures(), self.bodies.eta_scalar)
        self.pose_time = 0.0                               # the time of the pose the device holds as "cur"
        for ctx in self.ctxs:
            ctx.set_dirichlet(nat.VELOCITY, *self.vbc)
            ctx.set_dirichlet(nat.PRESSURE, *self.pbc)
            ctx.set_dirichlet(nat.SCALAR, *self.tbc)
            ctx.set_state(nat.BODY_FORCE, self.f)
            ctx.set_state(nat.T_SOURCE, self.q)
            ctx.set_state(nat.T0, T_init)
            ctx.set_state(nat.T1, T_init)
        self._coeffs()
        self._scalar()
        self._dev(lambda c: c.set_viscosity_law(self.law, self.law_params))
        self.observer("law", self.law, self.law_params)
        self._dev(lambda c: c.set_bodies(self.bodies.rows(0.0), self.bodies.eta, self.bodies.smoothing))
        self.observer("set_bodies", self._table(0.0))
        self._thermal()

    # ---- the calls, to every device
    def _dev(self, call):
        for ctx in self.ctxs:
            call(ctx)

    def _coeffs(self):
        c = self.coef
        self.h.c = dict(c)
        self._dev(lambda x: x.set_coeffs(c["convective_term"], c["pressure_term"], c["viscous_term"],
                                         c["body_force_term"], c["coriolis_term"], c["euler_term"]))

    def _scalar(self):
        self.h.set_scalar(KAPPA, self.b, self.scalar_form)
        self._dev(lambda c: c.set_scalar(KAPPA, self.b, self.scalar_form))

    def _make_bodies(self):
        bodies = heated_pair(self.dim, self.eta, EPS, self.eta_T, self.T_s)
        if self.extra_body:
            extra = Ball((0.75, 0.75), 0.12) if self.dim == 2 else Ball((0.75, 0.75, 0.7), 0.15)
            bodies = ImmersedBodies(bodies.bodies + [extra], self.eta, EPS, self.eta_T)
        return bodies

    def _table(self, t):
        """what the device compares: rows, eta and smoothing as bytes"""
        rows = self.bodies.rows(t)
        flat = np.concatenate([np.concatenate([[r[0]], *[np.atleast_1d(x) for x in r[1:]]]) for r in rows])
        return (flat.tobytes(), self.bodies.eta, self.bodies.smoothing)

    def _thermal(self):
        flags, values = self.bodies.temperatures()
        self.h.set_body_temperatures(flags, values, self.bodies.eta_scalar)
        self._dev(lambda c: c.set_body_temperatures(flags, values, self.bodies.eta_scalar))
        self.observer("thermal", flags.tobytes(), values.tobytes(), self.bodies.eta_scalar, int(flags.sum()))

    def _set_bodies(self):
        """the set at the pose the device holds (that of the step before): both levels get it"""
        t = self.pose_time
        self.h.set_bodies(self.bodies, t)
        self._dev(lambda c: c.set_bodies(self.bodies.rows(t), self.bodies.eta, self.bodies.smoothing))
        self.observer("set_bodies", self._table(t))

    def _set_state(self, name, factor):
        nat, h = self.nat, self.h
        vec = {"u2": h.vel[2], "u1": h.vel[1], "t2": h.T[2]}[name]
        slot = getattr(nat, name.upper()) if nat is not None else None
        vec *= factor                                      # (in place: the host's level)
        self._dev(lambda c: c.set_state(slot, vec))
        self.observer("set_state", name)

    # ---- the events
    def apply(self, code):
        assert code in EVENTS, code
        if code == "lp":
            base = STEP_LAWS[self.law]
            self.law_params = (1.5 * base[0], ) + base[1:] if self.law_params == base else base
        elif code == "l2":
            self.law = CARREAU if self.law == SMAGORINSKY else SMAGORINSKY
            self.law_params = STEP_LAWS[self.law]
        if code in ("lp", "l2", "l0"):
            if code == "l0":
                self.h.set_viscosity_law(0)
                self._dev(lambda c: c.set_viscosity_law(0))
                self.observer("law", 0, ())
            self.h.set_viscosity_law(self.law, self.law_params)
            self._dev(lambda c: c.set_viscosity_law(self.law, self.law_params))
            self.observer("law", self.law, self.law_params)
        elif code in ("be", "bs", "pb"):
            if code == "be":
                self.eta = 2.5 * self.k if self.eta == 2.0 * self.k else 2.0 * self.k
            if code == "pb":
                self.extra_body = not self.extra_body
            if code != "bs":
                self.bodies = self._make_bodies()
            self._set_bodies()
            if code == "pb":                               # (another count dropped the temperatures)
                self.observer("thermal", b"", b"", 0.0, 0)
                self._thermal()
        elif code == "mv":
            self.once["jump"] = 0.4 * self.k
        elif code in ("ts", "tt"):
            if code == "ts":
                self.T_s = -0.4 if self.T_s == 0.9 else 0.9
                for b in self.bodies.bodies[:1]:
                    b.temperature = self.T_s
            self._thermal()
        elif code == "wg":
            self.levels_given = True
        elif code == "wn":
            self.levels_given = False
        elif code == "w2":
            self.once["w2"] = 0.1
        elif code == "cc":
            self.coef["convective_term"] = 0.7 if self.coef["convective_term"] == 1.0 else 1.0
            self._coeffs()
        elif code == "cf":
            self.form_id = 3 if self.form_id == 0 else 0
        elif code == "sf":
            self.scalar_form = 1 - self.scalar_form
            self._scalar()
        elif code == "dk":
            self.ts.set_desired_next_step_size(0.5 * self.k if self.ts.get_next_step_size() == self.k else self.k)
        elif code in ("u2", "t2"):
            self._set_state(code, 0.97)
        elif code == "u1":
            raise AssertionError("u1 is applied before the advance (step(pre_advance=...))")
        elif code == "ns":
            self.once["no scalar"] = True

    # ---- one time step
    def step(self, before_step=None, check=None, pre_advance=()):
        """``before_step(run)``: called after the per-step settings, before the two steps; ``check(run, what)``: called
        after the scalar step (what = "scalar") and after the flow step ("flow") to compare devices and host;
        ``pre_advance``: events applied after the flow step and before the advance ("u1": the level that becomes u2
        is rewritten, so the vector just stored no longer belongs to it)"""
        ts, h, dim = self.ts, self.h, self.dim
        once, self.once = self.once, {}
        ts.update_coefficients()
        kk = ts.get_next_step_size()
        self.coefficients = (ts.alpha, ts.beta, ts.gamma, kk)
        self._dev(lambda c: c.set_imex(ts.alpha, ts.beta, ts.gamma, kk))
        t = ts.current_time + once.get("jump", 0.0)
        h.move_bodies(t)
        self._dev(lambda c: c.move_bodies(self.bodies.rows(t)))
        self.observer("move", self._table(t))
        self.pose_time = t
        w_next, wd = omega_of_time(dim, ts.next_time), 0.8 * _axis(dim)
        w1 = omega_of_time(dim, ts.current_time) if self.levels_given else None
        w2 = None
        if self.levels_given and self.step_index > 0:
            w2 = omega_of_time(dim, ts.previous_time) + once.get("w2", 0.0) * _axis(dim)
        h.set_angular_velocity(w_next, wd)
        h.set_imex_rotation(1, w1, w2)
        self._dev(lambda c: (c.set_angular_velocity(w_next, wd), c.set_imex_rotation(1, w1, w2)))
        ccor = self.coef["coriolis_term"]
        gam = [tuple(np.atleast_1d(2.0 * ccor * (w_next if w is None else w)).tolist()) for w in (w1, w2)]
        h.form = FLOW_FORMS[self.form_id]
        if before_step is not None:
            before_step(self)
        b1 = ts.beta[1]
        if not once.get("no scalar"):
            self.infos = []
            self._dev(lambda c: self.infos.append(c.step_scalar_imex(rtol=1e-13)))
            self.observer("scalar_step", b1, self.scalar_form)
            h.step_scalar(ts.alpha, ts.beta, ts.gamma, kk, self.tbc)
            if check is not None:
                check(self, "scalar")
        for ctx in self.ctxs:
            ctx.step_imex(self.opts(ctx))
        self.observer("flow_step", b1, self.form_id, self.coef["convective_term"], gam[0], gam[1])
        h.step(ts.alpha, ts.beta, ts.gamma, kk, self.vbc, self.pbc)
        if check is not None:
            check(self, "flow")
        for code in pre_advance:
            assert code == "u1"
            self._set_state(code, 0.97)
        self._dev(lambda c: c.advance(0))
        self.observer("advance")
        h.advance()
        ts.advance_time()
        self.step_index += 1

    def opts(self, ctx):
        o = ctx.default_step_opts()
        o.convective_form = self.form_id
        for ko in (o.momentum, o.poisson, o.correction):
            ko.rtol = 1e-13
        return o
