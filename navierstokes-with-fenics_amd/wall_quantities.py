"""Wall quantities of the device-resident solution (csrc/wall.hip): everything a driver evaluates on a boundary.

Per boundary id (one group of facets each) the measure, the pressure and the viscous part of the surface force, the
torque of the traction about a point, the mass flux, the mean temperature and the conductive heat flux; per facet the
distributions behind them -- pressure, wall shear stress, normal velocity, heat flux.  The facets are made resident
once (``nsfem_wall_set_facets``); every evaluation is two kernel launches and one small copy
(``nsfem_wall_compute``), so it can run at every time step.  ``ProblemBase._compute_boundary_force`` (one summed
traction of one boundary id, lists uploaded at every call) stays as it is.

* ``WallQuantities(solver, boundary_ids, origin=None, symmetric_gradient_factor=1.0)``; ``bind(solver)`` when the
  solver comes later (``ProblemBase._add_wall_quantities``).  Traction ``-p n + c_v f (grad u + grad u^T) n`` with
  ``c_v`` the solver's viscous coefficient and ``f`` the factor (1: the Newtonian stress, 1/2: the traction of the
  reference's dfg_benchmark driver) -- the convention of ``_compute_boundary_force`` --, plus ``nu_x (grad u +
  grad u^T) n`` when the solver has a viscosity model.  ``n`` points out of the fluid.  The viscous row is the
  RESOLVED stress: on a boundary with a wall-stress model (``wall_models``, ``IMEXIPCSSolver.set_wall_model``) it is
  not the wall stress -- ``ProblemBase._compute_wall_model`` returns that.
* ``compute()``: ``{boundary_id: dict(area, pressure_force, viscous_force, force, torque, mass_flux, mean_temperature,
  heat_flux)}``; ``heat_flux`` = ``int -kappa grad T . n``, the conductive heat LEAVING the fluid (temperature
  entries are 0 for a solver without a scalar).  With a subgrid heat flux the device forms the row with ``kappa +
  kappa_x``: ``nu_x / Pr_t`` of a model with ``prandtl_t``, ``c_K Delta_K^2 gamma`` of a
  ``DynamicSmagorinskyModel(heat_flux="dynamic")`` with the constant of the evaluated velocity and scalar.
* ``distribution(boundary_id)``: arrays in facet order (``midpoints``, ``normals``, ``area``, ``pressure``,
  ``wall_shear_stress``, ``normal_velocity``, ``heat_flux``).
* ``nusselt_number(boundary_id, delta_T, length)`` = ``-heat_flux length / (kappa delta_T area)``: positive when heat
  enters the fluid.
* ``record(t)`` appends to ``times`` and ``series[boundary_id][key]``.

The context keeps ONE facet set: a second instance on the same solver takes it over when it is used, the first one
makes its set resident again at its next use.  Partitioned meshes are refused by the device.
"""
import numpy as np

import _native as nat

KEYS = ("area", "pressure_force", "viscous_force", "force", "torque", "mass_flux", "mean_temperature", "heat_flux")


def row_width(dim):
    """NW of nsfem_wall_compute"""
    return 9 if dim == 2 else 13


def split_rows(rows, dim):
    """the columns of wall rows [..., NW] by name: area, pressure_force [.., dim], viscous_force [.., dim],
    mass_flux, temperature_integral, heat_flux, torque ([..] in 2D, [.., 3] in 3D)"""
    rows = np.asarray(rows, dtype=np.float64)
    assert rows.shape[-1] == row_width(dim)
    tq = rows[..., 4 + 2 * dim] if dim == 2 else rows[..., 4 + 2 * dim:7 + 2 * dim]
    return dict(area=rows[..., 0], pressure_force=rows[..., 1:1 + dim], viscous_force=rows[..., 1 + dim:1 + 2 * dim],
                mass_flux=rows[..., 1 + 2 * dim], temperature_integral=rows[..., 2 + 2 * dim],
                heat_flux=rows[..., 3 + 2 * dim], torque=tq)


def sort_by_group(facet_group, n_groups):
    """(perm, offsets) of the stable sort by group nsfem_wall_set_facets performs: resident facet k is input facet
    perm[k], group g owns the resident facets offsets[g] .. offsets[g + 1]"""
    g = np.asarray(facet_group, dtype=np.int64).ravel()
    n_groups = int(n_groups)
    if n_groups < 1:
        raise ValueError("n_groups < 1")
    if g.size and (g.min() < 0 or g.max() >= n_groups):
        raise ValueError("facet group out of range")
    perm = np.argsort(g, kind="stable").astype(np.int32)
    offsets = np.concatenate([[0], np.cumsum(np.bincount(g, minlength=n_groups))]).astype(np.int32)
    return perm, offsets


def tangential_part(t, n):
    """t - (t.n) n along the last axis (n: unit vectors)"""
    t, n = np.asarray(t, dtype=np.float64), np.asarray(n, dtype=np.float64)
    return t - (t * n).sum(axis=-1, keepdims=True) * n


def nusselt_number(heat_flux, area, kappa, delta_T, length):
    """-heat_flux length / (kappa delta_T area) with heat_flux = int -kappa grad T . n (heat leaving the fluid):
    positive when heat enters the fluid, 1 for pure conduction between walls ``length`` apart"""
    if not (kappa > 0.0 and area > 0.0 and delta_T != 0.0 and length > 0.0):
        raise ValueError("nusselt number: kappa, area and length must be positive and delta_T nonzero")
    return -float(heat_flux) * float(length) / (float(kappa) * float(delta_T) * float(area))


def facet_geometry(mesh, cells, local):
    """(midpoints [nf, dim], outward unit normals [nf, dim]) of the facets opposite vertex ``local`` of ``cells``"""
    coords = np.asarray(mesh.coords, dtype=np.float64)
    cv = np.asarray(mesh.cells, dtype=np.int64)[np.asarray(cells, dtype=np.int64)]
    dim = cv.shape[1] - 1
    nf = cv.shape[0]
    x = coords[cv][:, :, :dim]
    local = np.asarray(local, dtype=np.int64)
    keep = np.array([[v for v in range(dim + 1) if v != o] for o in range(dim + 1)], dtype=np.int64)[local]
    xf = x[np.arange(nf)[:, None], keep]
    mid = xf.mean(axis=1)
    if dim == 2:
        t = xf[:, 1] - xf[:, 0]
        n = np.stack([t[:, 1], -t[:, 0]], axis=1)
    else:
        n = np.cross(xf[:, 1] - xf[:, 0], xf[:, 2] - xf[:, 0])
    n = n / np.linalg.norm(n, axis=1, keepdims=True)
    inward = x[np.arange(nf), local] - mid
    n = np.where((n * inward).sum(axis=1, keepdims=True) > 0.0, -n, n)
    return mid, n


class WallQuantities:
    def __init__(self, solver=None, boundary_ids=(), origin=None, symmetric_gradient_factor=1.0, every=1):
        ids = [boundary_ids] if np.isscalar(boundary_ids) else list(boundary_ids)
        if not ids:
            raise ValueError("wall quantities: no boundary id given")
        if any(int(i) != i for i in ids):
            raise ValueError("wall quantities: boundary ids must be integers")
        ids = [int(i) for i in ids]
        if len(set(ids)) != len(ids):
            raise ValueError("wall quantities: a boundary id is listed twice")
        factor = float(symmetric_gradient_factor)
        if not np.isfinite(factor):
            raise ValueError("wall quantities: symmetric_gradient_factor is not finite")
        if origin is not None:
            origin = np.array(origin, dtype=np.float64).ravel()
            if origin.size not in (2, 3) or not np.all(np.isfinite(origin)):
                raise ValueError("wall quantities: origin must be 2 or 3 finite numbers")
        if int(every) < 1:
            raise ValueError("wall quantities: every < 1")
        self.boundary_ids = tuple(ids)
        self.every = int(every)
        self._origin, self._factor = origin, factor
        self._solver = None
        self._steps_seen = 0
        self.times = []
        self.series = {i: {key: [] for key in KEYS} for i in self.boundary_ids}
        if solver is not None:
            self.bind(solver)

    def bind(self, solver):
        if self._solver is not None:
            assert self._solver is solver
            return
        if not hasattr(solver, "_ctx"):
            solver._setup_function_spaces()
        mesh, marks = solver._mesh, solver._boundary_markers
        dim = solver._ctx.dim
        if self._origin is not None and self._origin.size != dim:
            raise ValueError("wall quantities: origin has %d entries on a %dD mesh" % (self._origin.size, dim))
        cells, local, group = [], [], []
        for g, bid in enumerate(self.boundary_ids):
            facets = marks.facets_with_id(bid)
            facets = facets[mesh.facet_on_boundary[facets]]
            c, l = mesh.facet_cell_local(facets)
            cells.append(c)
            local.append(l)
            group.append(np.full(c.size, g, dtype=np.int32))
        self._cells, self._local, self._group = (np.concatenate(a).astype(np.int32) for a in (cells, local, group))
        self._ranges = np.concatenate([[0], np.cumsum([c.size for c in cells])])
        self._with_scalar = hasattr(solver, "_scalar_coefficients")
        if self._with_scalar:
            solver._push_scalar_coefficients()
        self._solver = solver
        self._activate()

    # the context keeps ONE facet set: whoever is used makes its own resident
    def _activate(self):
        assert self._solver is not None, "the wall quantities are not bound to a solver yet"
        ctx = self._solver._ctx
        if getattr(ctx, "_active_wall_set", None) is not self:
            try:
                ctx.wall_set_facets(self._cells, self._local, self._group, len(self.boundary_ids))
            except nat.NativeError as err:
                raise RuntimeError(str(err))
            ctx._active_wall_set = self
        return ctx

    @property
    def kappa(self):
        return float(self._solver._scalar_coefficients[0]) if self._with_scalar else 0.0

    def _options(self):
        solver = self._solver
        nu = float(solver._equation_coefficients["viscous_term"]) * self._factor
        use_law = getattr(solver, "_viscosity_model", None) is not None
        return dict(nu=nu, symmetric=1.0, kappa=self.kappa, origin=self._origin, use_law=use_law,
                    velocity_slot=nat.U0, pressure_slot=nat.P, scalar_slot=nat.T0 if self._with_scalar else -1)

    def rows(self, facets=False):
        """the raw rows of nsfem_wall_compute: group rows [n_ids, NW] (and facet rows [n_facets, NW] in the order of
        the boundary ids, the facets of one id in ascending facet number)"""
        ctx = self._activate()
        try:
            return ctx.wall_compute(facets=facets, **self._options())
        except nat.NativeError as err:
            raise RuntimeError(str(err))

    def compute(self):
        """{boundary_id: dict of KEYS} of the solution at the new time level (U0, P, T0)"""
        rows = self.rows()
        dim = self._solver._ctx.dim
        cols = split_rows(rows, dim)
        out = {}
        for g, bid in enumerate(self.boundary_ids):
            area = float(cols["area"][g])
            pf, vf = cols["pressure_force"][g].copy(), cols["viscous_force"][g].copy()
            tq = cols["torque"][g]
            out[bid] = dict(area=area, pressure_force=pf, viscous_force=vf, force=pf + vf,
                            torque=float(tq) if dim == 2 else tq.copy(), mass_flux=float(cols["mass_flux"][g]),
                            mean_temperature=float(cols["temperature_integral"][g]) / area if area > 0.0 else 0.0,
                            heat_flux=float(cols["heat_flux"][g]))
        return out

    def distribution(self, boundary_id):
        """arrays over the facets of one boundary id, in facet order: midpoints [nf, dim], normals [nf, dim], area,
        pressure (facet mean), wall_shear_stress [nf, dim] (tangential part of the viscous traction per area),
        normal_velocity (facet mean of u.n), heat_flux (per area)"""
        g = self.boundary_ids.index(int(boundary_id))
        a, b = int(self._ranges[g]), int(self._ranges[g + 1])
        dim = self._solver._ctx.dim
        cols = split_rows(self.rows(facets=True)[1][a:b], dim)
        mid, n = facet_geometry(self._solver._mesh, self._cells[a:b], self._local[a:b])
        area = cols["area"]
        # int -p n = -(mean p) |f| n on a flat facet
        pressure = -(cols["pressure_force"] * n).sum(axis=1) / area
        return dict(midpoints=mid, normals=n, area=area.copy(), pressure=pressure,
                    wall_shear_stress=tangential_part(cols["viscous_force"] / area[:, None], n),
                    normal_velocity=cols["mass_flux"] / area, heat_flux=cols["heat_flux"] / area)

    def nusselt_number(self, boundary_id, delta_T, length):
        r = self.compute()[int(boundary_id)]
        return nusselt_number(r["heat_flux"], r["area"], self.kappa, delta_T, length)

    def record(self, t):
        """append the quantities of every boundary id to ``times`` / ``series[boundary_id][key]``"""
        res = self.compute()
        self.times.append(float(t))
        for bid, r in res.items():
            for key in KEYS:
                self.series[bid][key].append(r[key])

    def record_step(self, t):
        """what ``solve_problem`` calls after every step: record on every ``every``-th step"""
        self._steps_seen += 1
        if self._steps_seen % self.every != 0:
            return False
        self.record(t)
        return True
