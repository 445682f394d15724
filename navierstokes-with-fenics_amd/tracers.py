"""Probe points and passive tracer particles on device-resident solutions (csrc/points.hip).

The reference's drivers evaluate ``velocity(x)`` / ``pressure(x)`` of dolfin Functions in their post-processing
(demo/dfg_benchmark.py: the pressure difference over the cylinder; centre-line profiles of the cavity); particles are
new.  Both rest on the device point locator: the host sorts the cells into bins once per solver
(``point_locator.build_bins``), everything per point runs in one kernel launch.

* ``PointProbes(solver, X)``: locates X once, ``sample()`` evaluates velocity, pressure (and temperature) there,
  ``record(t)`` / ``series()`` keep a time series.
* ``TracerCloud(solver, X)``: particles kept in the device context; ``advect()`` moves them with RK4 through the
  velocity blended linearly in time from ``U1`` to ``U0`` -- the interval just solved, so it belongs between
  ``solver.solve()`` and ``solver.advance_time()``.  A particle that reaches a point outside the mesh keeps its last
  position with status 1.  The context holds one cloud at a time: a second cloud of the same solver takes the device
  storage over and the first is parked on the host until it is used again.
  Note: ``theta`` runs from 0 to 1 within ONE call, so two calls over dt / 2 see the whole blend twice and do not
  equal one call over dt; split a step with ``substeps`` instead.

Partitioned meshes are not supported (the device refuses contexts with a communicator).
"""
import numpy as np

import _native as nat
from point_locator import build_bins


def ensure_point_locator(solver):
    """build the bins of the solver's mesh and upload them, once per solver"""
    if getattr(solver, "_point_locator_ready", False):
        return
    if not hasattr(solver, "_ctx"):
        solver._setup_function_spaces()
    mesh = solver._mesh
    solver._ctx.set_point_locator(**build_bins(mesh.coords, mesh.cells))
    solver._point_locator_ready = True


class _Bound:
    """points handed over before the solver exists are bound to it later (ProblemBase._add_*)"""

    def __init__(self, solver, X):
        X = np.array(X, dtype=np.float64)
        assert X.ndim == 2, "points: expected an [m, dim] array"
        self._x0 = X
        self._solver = None
        if solver is not None:
            self.bind(solver)

    def bind(self, solver):
        if self._solver is not None:
            assert self._solver is solver
            return
        ensure_point_locator(solver)
        assert self._x0.shape[1] == solver._ctx.dim
        self._solver = solver
        self._on_bind()


class PointProbes(_Bound):
    def _on_bind(self):
        solver = self._solver
        self._cells = solver._ctx.locate_points(self._x0)
        self._with_temperature = hasattr(solver, "_scalar_coefficients")
        if self._with_temperature:
            solver._push_scalar_coefficients()
        self._times, self._records = [], []

    @property
    def points(self):
        return self._x0

    @property
    def cells(self):
        """cell of every probe point (-1: outside the mesh, its samples are NaN)"""
        return self._cells

    def sample(self):
        """dict(velocity [m, dim], pressure [m][, temperature [m]]) of the solution at the new time level"""
        ctx = self._solver._ctx
        out = dict(velocity=ctx.eval_points(nat.U0, self._x0, self._cells),
                   pressure=ctx.eval_points(nat.P, self._x0, self._cells))
        if self._with_temperature:
            out["temperature"] = ctx.eval_points(nat.T0, self._x0, self._cells)
        return out

    def record(self, t):
        self._times.append(float(t))
        self._records.append(self.sample())

    def series(self):
        """dict(time [k], velocity [k, m, dim], pressure [k, m][, temperature [k, m]])"""
        out = dict(time=np.array(self._times))
        m, dim = self._x0.shape
        shapes = dict(velocity=(0, m, dim), pressure=(0, m), temperature=(0, m))
        for key in ("velocity", "pressure") + (("temperature", ) if self._with_temperature else ()):
            out[key] = np.stack([r[key] for r in self._records]) if self._records else np.zeros(shapes[key])
        return out


class TracerCloud(_Bound):
    def _on_bind(self):
        self._x = self._x0.copy()
        self._status = None                       # host copy while parked
        self._activate()

    # the context keeps ONE cloud: whoever is used takes the device storage, the other waits on the host
    def _activate(self):
        ctx = self._solver._ctx
        active = getattr(ctx, "_active_cloud", None)
        if active is self:
            return
        if active is not None:
            active._park()
        X = self._x.copy()
        if self._status is not None:
            X[self._status != 0] = np.nan         # located outside: status 1 again; their positions stay in self._x
        ctx.tracers_set(X)
        ctx._active_cloud = self

    def _pull(self):
        x, cells, status = self._solver._ctx.tracers_get()
        if self._status is not None:              # particles that had left before the cloud was parked
            gone = self._status != 0
            x[gone] = self._x[gone]
        return x, cells, status

    def _park(self):
        self._x, _, self._status = self._pull()

    def advect(self, dt=None, substeps=1, slot_begin=nat.U1, slot_end=nat.U0):
        """RK4 with ``substeps`` substeps over dt (default: the step size of the solver's last ``solve()``) in the
        velocity blended from ``slot_begin`` (t_n) to ``slot_end`` (t_n+1)"""
        assert self._solver is not None, "the cloud is not bound to a solver yet"
        if dt is None:
            dt = self._solver._next_step_size
        self._activate()
        self._solver._ctx.tracers_advect(slot_begin, slot_end, float(dt), int(substeps))

    def positions(self):
        self._activate()
        return self._pull()[0]

    def cells(self):
        self._activate()
        return self._pull()[1]

    def status(self):
        """uint8 [n]: 0 moving, 1 left the mesh"""
        self._activate()
        return self._pull()[2]

    @property
    def n_left(self):
        self._activate()
        return self._solver._ctx.tracers_info()["n_left"]

    def info(self):
        self._activate()
        return self._solver._ctx.tracers_info()

    def sample(self, function):
        """values of a DeviceFunction at the particles ([n, dim] / [n]); particles that left sample their last
        position"""
        self._activate()
        return self._solver._ctx.eval_points(function.slot, self._pull()[0])
