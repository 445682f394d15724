"""Implicit-explicit (IMEX) incremental pressure-correction scheme on the MI355X.

The reference lists the decoupled IMEX schemes as solvers "to be included"; this class drives the
coefficients of ``imex_time_stepping.IMEXTimeStepping`` (SBDF2, CNAB, mCNAB, CNLF).  The convective
term is extrapolated from the known time levels, so the diffusion step is ONE linear solve with the
constant, symmetric positive definite matrix  alpha_0/k M + gamma_0 c_v K  -- CG instead of the
Newton / BiCGStab iteration of ``IPCSSolver``.  With alpha, beta, gamma of the time stepping, step
size k, u1 = u^n, u2 = u^(n-1) and N(u) the convective weak form vector in the selected form:

  1. diffusion step (CG):
       (alpha_0/k M + gamma_0 c_v K) u* = -[ M (alpha_1 u1 + alpha_2 u2)/k
           + c_v K (gamma_1 u1 + gamma_2 u2) + c_c (beta_0 N(u1) + beta_1 N(u2))
           - c_p D^T p_old - c_b M f + traction ],     Dirichlet rows u*_i = g_i
     (traction-form viscosity: K is the traction-form stiffness)
  2. projection step:     A_p p = A_p p_old - alpha_0/k D u*          (as ``IPCSSolver``)
  3. velocity correction: M u = M u* - k/alpha_0 G (p - p_old)        (as ``IPCSSolver``)

N(u2) is not recomputed: the device keeps N(u1) of a step for the next one.  On 2D lattice meshes
with exact stencil dictionaries the whole right-hand side of step 1 is one kernel launch.

The scheme is conditionally stable (a CFL-type restriction on k, reported by the problem classes'
CFL diagnostic).  A strain-rate dependent viscosity (``set_viscosity_model``, ``viscosity_models``) keeps
all of this: c_v K stays in the matrix and the remainder V(u) joins the extrapolated vector,
N(u) = c_c conv(u) + V(u); that treatment is unconditionally stable only while |nu_x| stays a fraction
of c_v, otherwise k is bounded by about Delta^2 / nu_x.  Solid bodies inside the box
(``set_immersed_bodies``, ``immersed_bodies``) join the same vector as a Brinkman penalisation term B(u); that term
bounds k / eta.  Modelled walls (``set_wall_model``, ``wall_models``) add a third explicit term W(u), the
wall stress of a law of the wall sampled inside the flow; it bounds k nu r / (y h).

Rotating frames (``set_angular_velocity``): the Coriolis term is extrapolated with the convective
term, N(u) = c_c conv(u) + V(u) + M (2 c_cor Omega x u) with Omega taken at the time of the level
u belongs to, and the Euler term c_e M (dOmega/dt x x) joins the step-constant vector.  The
convection element kernel forms the Coriolis vector itself: no launch, no pass over memory and no
halo exchange is added, and uniform 2D lattices keep the one-launch right-hand side.  The device
driver refuses rotating frames unless asked (``nsfem_set_imex_rotation``); the solver asks on its
own when an angular velocity has been set, and hands over Omega(t^n), Omega(t^(n-1)) before every
step.  The explicit treatment bounds the step: keep 2 c_cor |Omega| k at or below about 0.1 unless
viscosity damps the mode.  3D meshes run through the generic right-hand-side path.

Partitioned meshes (a context with a communicator, ``partition.py``'s ``attach``): the step runs on
strips, slabs and recursive-bisection partitions.  Its right-hand side costs one halo exchange (u1;
u2 travels with it in one packed message only when its slot was written since the last step); on
uniform strips it stays one kernel launch, which writes zeros to the rows of ghost nodes.  The ranks
agree once on the right-hand-side path, so every rank runs the same sequence of collectives.
"""
import numpy as np

import _native as nat
from fem_function import DeviceFunction, MixedFunction
from imex_time_stepping import IMEXTimeStepping, IMEXType
from immersed_bodies import ImmersedBodies, stiff_step_bound, stiff_step_stable
from ns_ipcs_solver import _FORM_ID, _DeviceSystem
from ns_solver_base import InstationarySolverBase


class IMEXIPCSSolver(InstationarySolverBase):
    _required_objects = ("_diffusion_solver", "_projection_solver", "_velocity_correction_solver")
    _scheme_id = 0
    #: what InstationaryProblem.solve_problem builds for this solver class
    time_stepping_class = IMEXTimeStepping
    imex_type = IMEXType.SBDF2

    def __init__(self, mesh, boundary_markers, form_convective_term, time_stepping, tol=1e-10,
                 max_iter=50, device=0):
        assert isinstance(time_stepping, IMEXTimeStepping)
        super().__init__(mesh, boundary_markers, form_convective_term, time_stepping, tol,
                         max_iter, device=device)
        self.last_step_info = None

    def set_viscosity_model(self, model):
        """a model of ``viscosity_models`` (``SmagorinskyModel``, ``WALEModel``, ``VremanModel``, ``CarreauModel``,
        ``DynamicSmagorinskyModel``) or None for the constant
        viscosity.  Its parameters are formed from the equation coefficients, so it is pushed to the device again
        whenever they change; partitioned meshes are refused by the device driver."""
        assert model is None or (hasattr(model, "law_id") and hasattr(model, "params"))
        self._viscosity_model = model
        self._push_viscosity_model()

    def _push_viscosity_model(self):
        if not (hasattr(self, "_ctx") and hasattr(self, "_viscosity_model")):
            return
        model = self._viscosity_model
        try:
            if model is None:
                self._ctx.set_viscosity_law(0)
            elif hasattr(self, "_equation_coefficients"):
                params = tuple(model.params(self._equation_coefficients))
                if hasattr(model, "vertex_groups"):
                    # the dynamic model: the law first (which resets the groups), then its groups -- and only when
                    # something changed, since a push of other groups invalidates the stored explicit vectors
                    # (Lagrangian averaging: the law, then the mode -- setting the law anew would reset its state)
                    lagrangian = getattr(model, "lagrangian", False)
                    n_groups, ids = model.vertex_groups(self._dofmap.p1_coords)
                    pushed = (id(self._ctx), params, n_groups, ids.tobytes(),
                              tuple(model.averaging_params()) if lagrangian else None)
                    if getattr(self, "_pushed_dynamic", None) == pushed and \
                            self._ctx.viscosity_info()["law"] == model.law_id:
                        return
                    self._ctx.set_viscosity_law(model.law_id, params)
                    if lagrangian:
                        self._ctx.set_dynamic_averaging(1, *model.averaging_params())
                    else:
                        self._ctx.set_dynamic_groups(n_groups, ids)
                    self._pushed_dynamic = pushed
                else:
                    self._ctx.set_viscosity_law(model.law_id, params)
        except nat.NativeError as err:
            raise RuntimeError(str(err))

    def _push_coefficients(self):
        super()._push_coefficients()
        self._push_viscosity_model()

    def dynamic_lagrangian_state(self):
        """the state of ``DynamicSmagorinskyModel(averaging="lagrangian")`` for a restart file, [n_p1, 4]
        (``nsfem_dynamic_lagrangian_state``); it goes beside the velocity levels and the stored explicit vector"""
        return self._ctx.dynamic_lagrangian_state()

    def set_dynamic_lagrangian_state(self, state):
        """restore what ``dynamic_lagrangian_state`` returned.  The model must be on the device already (set and
        pushed with the equation coefficients): RuntimeError otherwise, since a later push of the law would drop the
        restored state.  A push happens again only when the model's parameters change -- which resets the state by
        definition -- so restore after the coefficients are final"""
        if not (hasattr(self, "_ctx") and self._ctx.dynamic_lagrangian_info()["active"]):
            raise RuntimeError("set_dynamic_lagrangian_state: no DynamicSmagorinskyModel(averaging=\"lagrangian\") is "
                               "active on the device; set the model and the equation coefficients first")
        try:
            self._ctx.set_dynamic_lagrangian_state(state)
        except nat.NativeError as err:
            raise RuntimeError(str(err))

    def set_immersed_bodies(self, bodies, allow_stiff=False):
        """an ``immersed_bodies.ImmersedBodies`` or None for none.  The penalisation term is explicit: a step with
        k / eta above ``stiff_step_bound`` of the scheme's coefficients (always the case for CNLF) raises ValueError
        unless ``allow_stiff``.  Bodies with a ``motion`` are moved to t^n once before every step; a set handed over in
        the middle of a run goes to the device with its poses of t^(n-1) and t^n.  Partitioned meshes are refused by
        the device driver.  Temperatures of the bodies (heated bodies) act on a transported scalar only: this class has
        none and ignores them, ``BoussinesqIMEXSolver`` pushes them with the bodies."""
        assert bodies is None or isinstance(bodies, ImmersedBodies)
        self._immersed_bodies = bodies
        self._immersed_allow_stiff = bool(allow_stiff)
        self._immersed_on_device = False
        self._push_immersed_bodies()

    def _push_immersed_bodies(self):
        if not (hasattr(self, "_ctx") and hasattr(self, "_immersed_bodies")):
            return
        bodies, ts = self._immersed_bodies, self._time_stepping
        self._immersed_moved_to = None
        try:
            if bodies is None:
                self._ctx.set_bodies([])
            elif not bodies.moving:
                assert bodies.dim == self._space_dim
                self._ctx.set_bodies(bodies.rows(), bodies.eta, bodies.smoothing)
            else:
                assert bodies.dim == self._space_dim
                # (a new set makes the next step form N(u2) afresh, with the older of the device's two poses: in the
                # middle of a run that is the pose of t^(n-1), and the pose of t^n follows as a move)
                if ts.step_number > 0:
                    self._ctx.set_bodies(bodies.rows(ts.previous_time), bodies.eta, bodies.smoothing)
                    self._move_immersed_bodies()
                else:
                    self._ctx.set_bodies(bodies.rows(ts.current_time), bodies.eta, bodies.smoothing)
        except nat.NativeError as err:
            raise RuntimeError(str(err))
        self._immersed_on_device = True

    def _move_immersed_bodies(self):
        """the pose of t^n -> device, once per time level: a second call for the same t^n (the coefficients are
        refreshed again, a step is tried again) would push the pose of t^(n-1) out of the device's memory"""
        t = self._time_stepping.current_time
        if getattr(self, "_immersed_moved_to", None) == t:
            return
        self._ctx.move_bodies(self._immersed_bodies.rows(t))
        self._immersed_moved_to = t

    def immersed_step_bound(self):
        """the largest admissible k / eta: ``stiff_step_bound`` of the current coefficients and of the scheme's
        uniform-step coefficients (the first step is first order and would admit more than the steps after it).  Two
        bisections, about a millisecond: for diagnostics and the error message, not for every step"""
        ts = self._time_stepping
        alpha, beta, _ = ts.uniform_coefficients()
        return min(stiff_step_bound(alpha, beta), stiff_step_bound(ts.alpha, ts.beta))

    def _immersed_ratios(self, bodies, k):
        """the ratios held to the stability test, as (name, value) pairs: k / eta of the flow's term here; a solver
        with a transported scalar adds k / eta_scalar"""
        return (("k / eta", k / bodies.eta), )

    def _immersed_step_is_stable(self, ratio, ratio_scalar=None):
        """k / eta = ratio (and k / eta_scalar = ratio_scalar, where a body is thermal) against the current and the
        uniform-step coefficients: two root solves each, and none while coefficients and ratios stay what they were at
        the last step (uniform steps).  With adaptive steps every step asks anew, at the cost of the root solves"""
        ts = self._time_stepping
        key = (ts.imex_type, tuple(ts.alpha), tuple(ts.beta), ratio, ratio_scalar)
        if getattr(self, "_immersed_stable_memo", (None, None))[0] != key:
            uniform = self.__dict__.setdefault("_immersed_uniform", {})
            if ts.imex_type not in uniform:
                uniform[ts.imex_type] = ts.uniform_coefficients()
            alpha, beta, _ = uniform[ts.imex_type]
            ok = all(stiff_step_stable(alpha, beta, x) and stiff_step_stable(ts.alpha, ts.beta, x)
                     for x in (ratio, ratio_scalar) if x is not None)
            self._immersed_stable_memo = (key, ok)
        return self._immersed_stable_memo[1]

    def _step_immersed_bodies(self):
        """before a step: the stability check, and the pose of t^n for bodies that move"""
        bodies = getattr(self, "_immersed_bodies", None)
        if bodies is None:
            return
        ts = self._time_stepping
        ratios = self._immersed_ratios(bodies, ts.get_next_step_size())
        if not self._immersed_allow_stiff and not self._immersed_step_is_stable(*(x for _, x in ratios)):
            name, ratio = next(((n, x) for n, x in ratios if not self._immersed_step_is_stable(x)), ratios[0])
            raise ValueError("immersed bodies: %s = %.6g exceeds %.6g, the stability bound of the explicit "
                             "penalisation term for %s (raise eta, lower k, or pass allow_stiff=True)"
                             % (name, ratio, self.immersed_step_bound(), ts.imex_type.name))
        if not getattr(self, "_immersed_on_device", False):
            self._push_immersed_bodies()
        if bodies.moving:
            try:
                self._move_immersed_bodies()
            except nat.NativeError as err:
                raise RuntimeError(str(err))

    def set_wall_model(self, model):
        """a ``wall_models.WallModel`` or None for none: the walls with the model's boundary ids keep u.n = 0 only and
        take their tangential stress from the law -- the explicit term W(u), third in the extrapolated vector after
        V(u) and B(u).  ValueError if a modelled boundary id carries ``no_slip`` or any other condition
        that fixes a tangential component, or no condition that fixes the normal component (``no_normal_flux``; that
        condition is axis-aligned).  Partitioned meshes and a viscous coefficient of None are refused by the device
        driver.  ``wall_quantities``' viscous row stays the RESOLVED stress on such a boundary; the modelled wall
        stress is ``ProblemBase._compute_wall_model``."""
        from wall_models import WallModel
        assert model is None or isinstance(model, WallModel)
        self._wall_model = model
        if hasattr(self, "_velocity_bcs"):
            self._check_wall_model_bcs()
        self._push_wall_model()

    def _check_wall_model_bcs(self):
        from ns_solver_base import VelocityBCType as T
        model = getattr(self, "_wall_model", None)
        if model is None:
            return
        import fem_host
        for bid in model.boundary_ids:
            normal = np.array(fem_host.boundary_normal(self._mesh, self._boundary_markers, bid))
            k = int(np.abs(normal).argmax())
            if abs(abs(normal[k]) - 1.0) >= 5.0e-14:
                raise ValueError("wall model: boundary id %d is not axis aligned (no_normal_flux needs that)" % bid)
            normal_fixed = False
            for bc in (bc for bc in self._velocity_bcs if bc[1] == bid):
                if bc[0] is T.no_normal_flux:
                    normal_fixed = True
                elif bc[0] in (T.constant_component, T.function_component) and bc[2] == k:
                    normal_fixed = True
                else:
                    raise ValueError("wall model: boundary id %d carries %s, which fixes a tangential component; a "
                                     "modelled wall takes no_normal_flux only" % (bid, bc[0].name))
            if not normal_fixed:
                raise ValueError("wall model: boundary id %d carries no condition that fixes the normal component "
                                 "(no_normal_flux)" % bid)

    def _push_wall_model(self):
        if not (hasattr(self, "_ctx") and hasattr(self, "_wall_model") and hasattr(self, "_dofmap")):
            return
        model = self._wall_model
        try:
            if model is None:
                self._wall_model_arrays = None
                self._ctx.set_wall_model(0)
                return
            if hasattr(self, "_velocity_bcs"):
                self._check_wall_model_bcs()
            a = model.build(self._mesh, self._boundary_markers, self._dofmap)
            self._ctx.set_wall_model(model.law.law_id, model.law.params(), a.facet_cell, a.facet_local, a.sample_cell,
                                     a.sample_lambda, a.sample_y, a.wall_velocity)
            self._wall_model_arrays = a
        except nat.NativeError as err:
            raise RuntimeError(str(err))

    def _setup_function_spaces(self):
        if not hasattr(self, "_Wh"):
            super()._setup_function_spaces()
        slots = (nat.U0, nat.U1, nat.U2)
        self._velocities = []
        for i in range(self._n_time_levels() + 1):
            name = i * "old" + (i > 0) * "_" + "velocity"
            self._velocities.append(DeviceFunction(self, "velocity", slots[i], name))
        self._intermediate_velocity = DeviceFunction(self, "velocity", nat.USTAR,
                                                     "intermediate_velocity")
        self._pressure = DeviceFunction(self, "pressure", nat.P, "pressure")
        self._old_pressure = DeviceFunction(self, "pressure", nat.P_OLD, "old_pressure")

    def _setup_problem(self):
        if not all(hasattr(self, a) for a in ("_Wh", "_solutions", "_intermediate_velocity",
                                              "_velocities", "_pressure", "_old_pressure")):  # pragma: no cover
            self._setup_function_spaces()
        self._ctx.set_convective_form(_FORM_ID[self._form_convective_term])
        if not all(hasattr(self, a) for a in ("_next_step_size", "_alpha", "_beta", "_gamma")):
            self._update_time_stepping_coefficients()
        self._setup_boundary_conditions()
        self._push_viscosity_model()
        if not getattr(self, "_immersed_on_device", False):
            self._push_immersed_bodies()
        self._push_wall_model()
        self._diffusion_solver = _DeviceSystem(self, nat.SYS_MOMENTUM)
        self._projection_solver = _DeviceSystem(self, nat.SYS_POISSON)
        self._velocity_correction_solver = _DeviceSystem(self, nat.SYS_CORRECTION)

    def _update_time_stepping_coefficients(self):
        """alpha, beta, gamma and the step size k -> device"""
        ts = self._time_stepping
        self._next_step_size = ts.get_next_step_size()
        self._alpha, self._beta, self._gamma = list(ts.alpha), list(ts.beta), list(ts.gamma)
        assert len(self._alpha) == 3 and len(self._beta) == 2 and len(self._gamma) == 3
        self._ctx.set_imex(self._alpha, self._beta, self._gamma, self._next_step_size)
        self._push_imex_rotation()
        self._step_immersed_bodies()

    def _push_imex_rotation(self):
        """rotating frame: opt in and hand the device Omega(t^n), Omega(t^(n-1)) -- the levels the Coriolis term is
        extrapolated from (the first step reads t^n only: beta_1 = 0).  The base class pushes the new level's Omega
        and dOmega/dt.  Without an angular velocity nothing is called."""
        if not hasattr(self, "_angular_velocity"):
            return
        ts, av = self._time_stepping, self._angular_velocity
        omega_n = av.value_at(ts.current_time)
        omega_nm1 = av.value_at(ts.previous_time) if ts.step_number > 0 else None
        self._ctx.set_imex_rotation(1, omega_n, omega_nm1)

    def _step_options(self):
        o = self._common_step_options(self._ctx.default_step_opts())
        o.convective_form = _FORM_ID[self._form_convective_term]
        for k in (o.momentum, o.poisson, o.correction):
            k.rtol = self.krylov_rtol
            k.max_iter = self.krylov_max_iter
        if self._mg_levels is not None:
            o.momentum.precond = o.poisson.precond = 1
        assert self.poisson_solver in ("multigrid", "fast_diagonalization")
        if self.poisson_solver == "fast_diagonalization" and self._fast_diagonalization_ready():
            o.poisson.precond = 3
        assert self.mass_solver in ("chebyshev", "cg")
        o.correction.precond = 2 if self.mass_solver == "chebyshev" else 0
        return o

    def _solve_time_step(self):
        try:
            self.last_step_info = self._ctx.step_imex(self._step_options())
        except nat.NativeError as err:
            raise RuntimeError(str(err))

    def set_initial_conditions(self, initial_conditions):
        super().set_initial_conditions(initial_conditions)
        assert all(hasattr(self, x) for x in ("_velocities", "_intermediate_velocity",
                                              "_pressure", "_old_pressure"))

    @property
    def solution(self):
        """(velocity, pressure) at the new time level (split fields on the device)"""
        return MixedFunction(self, nat.U0, nat.P, name="solution")
