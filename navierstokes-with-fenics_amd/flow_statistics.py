"""Running flow statistics on device-resident solutions (csrc/statistics.hip).

Time averages of a transient run -- mean velocity, Reynolds stresses <u_i' u_j'>, turbulent kinetic energy, mean and
variance of pressure and temperature, the turbulent heat flux <u' T'> -- and their profiles over the nodes of equal
coordinate along one axis (the wall-normal direction of a channel).  The reference has nothing like it; its drivers
would copy the solution to the host after every step and keep numpy sums.  Here a sample is ONE kernel launch that
streams the nodal vectors where they are, and a result leaves the device as one copy.

* ``FlowStatistics(solver, pressure=True, scalar=None, start_time=0.0, every=1)``: the accumulators live in the
  solver's device context (one set per context: binding a second instance to the same solver raises).
  ``scalar=None``: the temperature is sampled iff the solver transports one.  ``sample(weight)`` adds ``U0``, ``P`` (and ``T0``) with the given weight -- the step size just
  taken, for a time average; it belongs between ``solver.solve()`` and ``solver.advance_time()``, where
  ``InstationaryProblem.solve_problem`` calls it for a registered instance (``ProblemBase._add_flow_statistics``) once
  ``next_time >= start_time`` and on every ``every``-th step.
* ``mean_velocity()`` ... ``turbulent_heat_flux()``: ``HostField``s at the mesh vertices for
  ``ProblemBase._add_to_field_output``; ``nodal(quantity)``: the values at all P2 / P1 nodes.
* ``set_profile_axis(axis, tol)`` groups the nodes by their coordinate along ``axis``; ``profiles()`` returns the
  coordinates and the pooled statistics of every group: the mean over the group, and the covariance about THAT mean
  (within-node plus between-node part, so what varies along the group is not lost).

Partitioned meshes are not supported (the device refuses them: the profiles would need a merge across ranks).
"""
import numpy as np

import _native as nat

COV_NAMES = {2: ("xx", "xy", "yy"), 3: ("xx", "xy", "xz", "yy", "yz", "zz")}


def groups_along_axis(coords, axis, tol=1e-9):
    """(values [g], group_ptr [g + 1], nodes): the nodes at ``coords`` [n, dim] grouped by their coordinate along
    ``axis`` -- coordinates closer than ``tol`` (times the extent along the axis) to their predecessor in sorted order
    belong to one group; groups in ascending coordinate, nodes of a group in ascending index.  Every node is in
    exactly one group."""
    x = np.asarray(coords, dtype=np.float64)[:, axis]
    order = np.argsort(x, kind="stable")
    xs = x[order]
    extent = float(xs[-1] - xs[0]) if xs.size else 0.0
    new = np.ones(xs.size, dtype=bool)
    new[1:] = np.diff(xs) > tol * max(extent, 1e-300)
    start = np.flatnonzero(new)
    group_ptr = np.append(start, xs.size).astype(np.int32)
    group_of = np.cumsum(new) - 1
    # stable sort by (group, node index)
    nodes = order[np.lexsort((order, group_of))].astype(np.int32)
    values = np.array([xs[a:b].mean() for a, b in zip(group_ptr[:-1], group_ptr[1:])])
    return values, group_ptr, nodes


class FlowStatistics:
    groups_along_axis = staticmethod(groups_along_axis)

    def __init__(self, solver=None, pressure=True, scalar=None, start_time=0.0, every=1):
        assert int(every) >= 1
        self._pressure, self._scalar = bool(pressure), scalar
        self.start_time, self.every = float(start_time), int(every)
        self._solver = None
        self._axis = None
        self._steps_seen = 0
        if solver is not None:
            self.bind(solver)

    def bind(self, solver):
        if self._solver is not None:
            assert self._solver is solver
            return
        if not hasattr(solver, "_ctx"):
            solver._setup_function_spaces()
        # one set of accumulators per context: a second instance would zero the first one's samples and share its arrays
        if getattr(solver, "_bound_flow_statistics", self) is not self:
            raise ValueError("this solver's context already serves another FlowStatistics (one set of accumulators "
                             "per context)")
        solver._bound_flow_statistics = self
        with_scalar = hasattr(solver, "_scalar_coefficients") if self._scalar is None else bool(self._scalar)
        if with_scalar:
            assert hasattr(solver, "_scalar_coefficients"), "scalar statistics need a solver that transports a scalar"
            solver._push_scalar_coefficients()
        self._scalar = with_scalar
        self._solver = solver
        flags = nat.STATS_VELOCITY | (nat.STATS_PRESSURE if self._pressure else 0) | \
            (nat.STATS_SCALAR if with_scalar else 0)
        solver._ctx.stats_enable(flags)
        if self._axis is not None:
            self.set_profile_axis(*self._axis)

    def _ctx(self):
        assert self._solver is not None, "the statistics are not bound to a solver yet"
        return self._solver._ctx

    def reset(self):
        """drop all samples (the profile groups stay)"""
        ctx = self._ctx()
        ctx.stats_enable(ctx.stats_info()["flags"])

    def sample(self, weight=1.0):
        """add the solution at the new time level (U0, P, T0) with ``weight``: one launch"""
        self._ctx().stats_sample(nat.U0, nat.P if self._pressure else -1, nat.T0 if self._scalar else -1, weight)

    def sample_step(self, next_time, step_size):
        """what ``solve_problem`` calls after every step: sample with the step size as weight once ``next_time`` has
        reached ``start_time``, on every ``every``-th such step"""
        if next_time < self.start_time * (1.0 - 1e-12) - 1e-300:
            return False
        self._steps_seen += 1
        if (self._steps_seen - 1) % self.every != 0:
            return False
        self.sample(step_size)
        return True

    def info(self):
        return self._ctx().stats_info()

    @property
    def weight(self):
        return self._ctx().stats_weight()

    # -- node values and fields -------------------------------------------------------
    def nodal(self, quantity):
        return self._ctx().stats_get(quantity)

    def _field(self, quantity, name):
        from fem_function import HostField
        dm = self._solver._dofmap
        vertex_node = dm.p1_vertex_node if quantity in (nat.STATS_MEAN_P, nat.STATS_VAR_P) else dm.vertex_node
        return HostField(dm.mesh, name, "Node", self.nodal(quantity)[vertex_node])

    def mean_velocity(self):
        return self._field(nat.STATS_MEAN_U, "mean velocity")

    def reynolds_stress(self):
        """[vertices, dim (dim + 1) / 2]: <u_i' u_j'> in the order xx, xy, yy / xx, xy, xz, yy, yz, zz"""
        return self._field(nat.STATS_COV_U, "reynolds stress")

    def turbulent_kinetic_energy(self):
        return self._field(nat.STATS_TKE, "turbulent kinetic energy")

    def mean_pressure(self):
        return self._field(nat.STATS_MEAN_P, "mean pressure")

    def pressure_variance(self):
        return self._field(nat.STATS_VAR_P, "pressure variance")

    def mean_temperature(self):
        return self._field(nat.STATS_MEAN_T, "mean temperature")

    def temperature_variance(self):
        return self._field(nat.STATS_VAR_T, "temperature variance")

    def turbulent_heat_flux(self):
        return self._field(nat.STATS_FLUX_UT, "turbulent heat flux")

    # -- profiles -----------------------------------------------------------------------
    def set_profile_axis(self, axis, tol=1e-9):
        """group the P2 (and, with pressure, the P1) nodes by their coordinate along ``axis`` (uniform weights;
        periodic images are one node of the dof map already)"""
        self._axis = (int(axis), float(tol))
        if self._solver is None:
            return
        dm, ctx = self._solver._dofmap, self._solver._ctx
        assert 0 <= axis < dm.dim
        self._coords2, ptr, nodes = groups_along_axis(dm.p2_coords, axis, tol)
        ctx.stats_set_groups(0, ptr, nodes)
        if self._pressure:
            self._coords1, ptr, nodes = groups_along_axis(dm.p1_coords, axis, tol)
            ctx.stats_set_groups(1, ptr, nodes)

    def profiles(self):
        """(coordinates, dict) of the P2 groups: ``mean_velocity`` [g, dim], ``reynolds_stress`` [g, dim (dim + 1) / 2],
        ``turbulent_kinetic_energy`` [g] and, with the scalar, ``mean_temperature``, ``temperature_variance`` [g],
        ``turbulent_heat_flux`` [g, dim]; with pressure also ``pressure_coordinates``, ``mean_pressure`` and
        ``pressure_variance`` of the P1 groups"""
        assert self._axis is not None and self._solver is not None, "set_profile_axis on a bound instance first"
        ctx = self._ctx()
        dim = ctx.dim
        ncov = dim * (dim + 1) // 2
        r = ctx.stats_profiles(0)
        diag = [0, 2] if dim == 2 else [0, 3, 5]
        out = dict(mean_velocity=r[:, :dim].copy(), reynolds_stress=r[:, dim:dim + ncov].copy(),
                   turbulent_kinetic_energy=0.5 * r[:, dim:dim + ncov][:, diag].sum(axis=1))
        if self._scalar:
            c = dim + ncov
            out.update(mean_temperature=r[:, c].copy(), temperature_variance=r[:, c + 1].copy(),
                       turbulent_heat_flux=r[:, c + 2:c + 2 + dim].copy())
        if self._pressure:
            rp = ctx.stats_profiles(1)
            out.update(pressure_coordinates=self._coords1, mean_pressure=rp[:, 0].copy(),
                       pressure_variance=rp[:, 1].copy())
        return self._coords2, out
