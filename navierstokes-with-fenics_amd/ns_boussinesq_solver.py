"""IMEX pressure correction with a transported scalar and Boussinesq buoyancy on the MI355X.

``BoussinesqIMEXSolver`` adds a P2 scalar T (a temperature, a concentration) on the velocity nodes to
``IMEXIPCSSolver``.  With alpha, beta, gamma and k of the ``IMEXTimeStepping``, T1 = T^n, T2 = T^(n-1),
u1 = u^n, u2 = u^(n-1), the diffusivity kappa, an optional nodal source q and C(u) the convection
matrix in the chosen form (standard: C_ij = int (u . grad phi_j) phi_i; skew-symmetric: 1/2 (C - C^T)):

  transport step (CG):
       (alpha_0/k M + gamma_0 kappa K) T^{n+1} = -[ M (alpha_1 T1 + alpha_2 T2)/k
           + kappa K (gamma_1 T1 + gamma_2 T2) + beta_0 C(u1) T1 + beta_1 C(u2) T2 ] + M q,
       Dirichlet rows T_i = g_i
  flow step: the three steps of ``IMEXIPCSSolver`` with the body force  f_eff = f + T^{n+1} b

The transport step comes first (it needs the known levels only); b is the constant buoyancy vector.
The device keeps beta_0 C(u1) T1 of a step for the next one and rebuilds the system matrix only when
alpha_0/k, gamma_0 or kappa change.  The reference has no transported quantity: its gravity-driven
cases prescribe the body force.  Partitioned meshes are refused by the device driver.  Rotating
frames (rotating convection) run as in ``IMEXIPCSSolver``: explicit Coriolis term, opted in by the
solver when an angular velocity has been set.

Heated bodies: immersed bodies with a ``temperature`` (``immersed_bodies``) add the explicit term
H(T) = (chi / eta_scalar) (T - T_s) to the transport step, inside the convection launch.
The solver pushes the temperatures wherever it pushes the bodies and holds k / eta_scalar to the same
stability test as k / eta.

Subgrid heat flux: a subgrid model of ``viscosity_models`` with a turbulent Prandtl number --
``SmagorinskyModel(cs, prandtl_t)``, ``WALEModel(cw, prandtl_t)`` or ``VremanModel(c, prandtl_t)`` -- adds the explicit term D(u, T) with the
eddy diffusivity kappa_x = nu_x / prandtl_t to the transport step, inside the same convection launch (DESIGN.md
4r).  The solver pushes prandtl_t wherever it pushes the viscosity model and the scalar coefficients; a model
without prandtl_t, or no model, pushes 0 (off).  The term is explicit: unconditionally stable only while kappa_x <
kappa / 3, otherwise k is bounded by about Delta^2 / kappa_x.

Dynamic subgrid heat flux: ``DynamicSmagorinskyModel(..., heat_flux="dynamic", ctheta_max=...)`` adds D(u, T) with
kappa_x = c_K Delta_K^2 gamma, C_theta computed on the device from the Germano identity of the scalar flux on the
level pair of every launch.  The solver pushes the fixed switch as before and then the dynamic one.
"""
import numpy as np

import _native as nat
import dlfn_compat as dlfn
from fem_function import DeviceFunction
from ns_imex_solver import IMEXIPCSSolver

_SCALAR_FORM_ID = {"standard": 0, "skew_symmetric": 1}


class BoussinesqIMEXSolver(IMEXIPCSSolver):
    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        #: result of ``scalar_info`` after the last transport step: dict(matrix_builds,
        #: convection_launches, convection_reuses, dictionary)
        self.last_scalar_info = None
        #: SolveInfo of the last transport solve (CG iterations, residuals)
        self.last_scalar_solve = None

    # ------------------------------------------------------------------ setters
    def set_scalar_coefficients(self, diffusivity, buoyancy=None, convective_form="standard"):
        """diffusivity kappa >= 0, buoyancy vector b (``dim`` entries; None: the scalar is passive)
        and the weak form of the scalar convection, "standard" or "skew_symmetric"."""
        diffusivity = float(diffusivity)
        assert np.isfinite(diffusivity) and diffusivity >= 0.0
        assert convective_form in _SCALAR_FORM_ID
        if buoyancy is not None:
            buoyancy = tuple(float(b) for b in buoyancy)
            assert len(buoyancy) == self._space_dim and all(np.isfinite(b) for b in buoyancy)
        self._scalar_coefficients = (diffusivity, buoyancy, convective_form)
        self._push_scalar_coefficients()

    def set_scalar_boundary_conditions(self, bcs):
        """``[(boundary_id, value), ...]`` Dirichlet conditions of the scalar; value: a number, a
        Constant / Expression (time-dependent ones are moved to the new time level every step) or a
        python callable ``f(X, t)`` of the node coordinates [n, dim] and the new time.  Later
        entries win at shared nodes."""
        assert isinstance(bcs, (list, tuple))
        for bc in bcs:
            assert len(bc) == 2 and isinstance(bc[0], int)
        self._scalar_bcs = [tuple(bc) for bc in bcs]
        self._push_scalar_boundary_conditions()

    def set_scalar_source(self, value):
        """nodal P2 source q (a number, Constant / Expression or callable ``f(X, t)``)"""
        self._scalar_source = value
        self._push_scalar_source()

    # ------------------------------------------------------------------ host -> device
    def _scalar_time(self):
        """the time level the next solve computes: data of the scalar are evaluated there"""
        return float(self._time_stepping.next_time)

    def _scalar_nodal(self, value, X, t):
        """values of a scalar datum at the nodes X and the time t"""
        if dlfn.is_time_dependent(value):
            if "time" in value._params:
                value.time = t
            else:
                value.t = t
        if callable(value) and not hasattr(value, "eval_at"):
            return np.broadcast_to(np.asarray(value(X, t), dtype=np.float64), (X.shape[0], )).copy()
        return np.asarray(dlfn.evaluate(value, X), dtype=np.float64).reshape(X.shape[0])

    def _scalar_dirichlet_arrays(self, t):
        dm = self._dofmap
        dofs, vals = [], []
        for bndry_id, value in getattr(self, "_scalar_bcs", []):
            nodes = np.unique(dm.facet_p2_nodes(self._boundary_markers.facets_with_id(bndry_id)))
            dofs.append(nodes)
            vals.append(self._scalar_nodal(value, dm.p2_coords[nodes], t))
        if not dofs:
            return np.zeros(0, dtype=np.int32), np.zeros(0)
        return np.concatenate(dofs).astype(np.int32), np.concatenate(vals)

    def _push_scalar_coefficients(self):
        if hasattr(self, "_ctx") and hasattr(self, "_scalar_coefficients"):
            kappa, b, form = self._scalar_coefficients
            try:
                self._ctx.set_scalar(kappa, b, _SCALAR_FORM_ID[form])
            except nat.NativeError as err:
                raise RuntimeError(str(err))
            self._push_scalar_sgs()

    def _push_viscosity_model(self):
        """the model as ``IMEXIPCSSolver`` pushes it, then its turbulent Prandtl number (none: 0, the term off)"""
        super()._push_viscosity_model()
        self._push_scalar_sgs()

    def _push_scalar_sgs(self):
        if not hasattr(self, "_ctx"):
            return
        model = getattr(self, "_viscosity_model", None)
        prandtl_t = getattr(model, "prandtl_t", None)
        dynamic = getattr(model, "heat_flux", None) == "dynamic"
        try:
            # (the two switches exclude each other on the device: the one that goes off goes first; a run that never
            # asked for the dynamic one never calls its setter)
            if not dynamic and getattr(self, "_pushed_dynamic_flux", None) is self._ctx:
                self._ctx.set_scalar_sgs_dynamic(False)
                self._pushed_dynamic_flux = None
            self._ctx.set_scalar_sgs(0.0 if prandtl_t is None else prandtl_t)
            if dynamic:
                self._ctx.set_scalar_sgs_dynamic(True, model.ctheta_max)
                self._pushed_dynamic_flux = self._ctx
        except nat.NativeError as err:
            raise RuntimeError(str(err))

    def _push_scalar_boundary_conditions(self, t=None):
        if hasattr(self, "_ctx") and hasattr(self, "_scalar_bcs"):
            d, v = self._scalar_dirichlet_arrays(self._scalar_time() if t is None else t)
            self._scalar_dirichlet = (d, v)
            self._ctx.set_dirichlet(nat.SCALAR, d, v)

    def _push_scalar_source(self, t=None):
        if hasattr(self, "_ctx") and hasattr(self, "_scalar_source"):
            q = self._scalar_nodal(self._scalar_source, self._dofmap.p2_coords,
                                   self._scalar_time() if t is None else t)
            self._ctx.set_state(nat.T_SOURCE, q)

    @staticmethod
    def _moves_in_time(value):
        return dlfn.is_time_dependent(value) or (callable(value) and not hasattr(value, "eval_at"))

    def _set_time(self, next_time=None, current_time=None):
        super()._set_time(next_time, current_time)
        t = float(self._time_stepping.next_time if next_time is None else next_time)
        if any(self._moves_in_time(value) for _, value in getattr(self, "_scalar_bcs", [])):
            self._push_scalar_boundary_conditions(t)
        if hasattr(self, "_scalar_source") and self._moves_in_time(self._scalar_source):
            self._push_scalar_source(t)

    # ------------------------------------------------------------------ heated bodies
    def _push_immersed_bodies(self):
        """the bodies as ``IMEXIPCSSolver`` pushes them, then their temperatures (none: removed)"""
        super()._push_immersed_bodies()
        if not (hasattr(self, "_ctx") and hasattr(self, "_immersed_bodies")):
            return
        bodies = self._immersed_bodies
        try:
            if bodies is None or not bodies.thermal:
                self._ctx.set_body_temperatures([], [])
            else:
                flags, values = bodies.temperatures()
                self._ctx.set_body_temperatures(flags, values, bodies.eta_scalar)
        except nat.NativeError as err:
            raise RuntimeError(str(err))

    def _immersed_ratios(self, bodies, k):
        """with a thermal body k / eta_scalar is held to the test of k / eta: the scalar recursion is the same"""
        ratios = super()._immersed_ratios(bodies, k)
        if bodies.thermal:
            ratios += (("k / eta_scalar", k / bodies.eta_scalar), )
        return ratios

    # ------------------------------------------------------------------ set-up
    def _setup_function_spaces(self):
        super()._setup_function_spaces()
        self._temperatures = [DeviceFunction(self, "scalar", slot, name)
                              for slot, name in ((nat.T0, "temperature"), (nat.T1, "old_temperature"),
                                                 (nat.T2, "old_old_temperature"))]

    def _setup_problem(self):
        super()._setup_problem()
        assert hasattr(self, "_scalar_coefficients"), "set_scalar_coefficients has not been called"
        self._push_scalar_coefficients()
        self._push_scalar_boundary_conditions()
        self._push_scalar_source()

    def set_initial_conditions(self, initial_conditions):
        """as ``IMEXIPCSSolver``; the optional key "temperature" (a number, Constant / Expression or
        callable ``f(X, t)``) is interpolated at the P2 nodes into the new and the old level"""
        initial_conditions = dict(initial_conditions)
        temperature = initial_conditions.pop("temperature", None)
        super().set_initial_conditions(initial_conditions)
        if temperature is not None:
            t0 = self._scalar_nodal(temperature, self._dofmap.p2_coords,
                                    float(self._time_stepping.current_time))
            for level in (0, 1):
                self._temperatures[level].assign(t0)

    # ------------------------------------------------------------------ the step
    def _solve_time_step(self):
        """the transport step (known levels only), then the flow step with f_eff = f + T^{n+1} b"""
        try:
            self.last_scalar_solve = self._ctx.step_scalar_imex(rtol=self.krylov_rtol,
                                                                max_iter=self.krylov_max_iter)
        except nat.NativeError as err:
            raise RuntimeError(str(err))
        self.last_scalar_info = self._ctx.scalar_info()
        super()._solve_time_step()

    @property
    def temperature(self):
        """the transported scalar at the new time level (a ``DeviceFunction`` on the P2 nodes)"""
        if not hasattr(self, "_temperatures"):
            self._setup_function_spaces()
        return self._temperatures[0]
