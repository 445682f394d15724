"""Strain-rate dependent viscosity models of the IMEX pressure-correction step.

The viscosity is  nu = c_v + nu_x(gamma, Delta_K)  with the shear rate gamma = sqrt(2 S:S) of the P2 velocity and the
filter width Delta_K = |K|^(1/dim) of the cell.  c_v (the solver's ``viscous_term`` coefficient) stays in the
implicit matrix; the device evaluates the remainder explicitly (``nsfem_set_viscosity_law``, include/nsfem.h).  A model
exposes ``law_id`` and ``params(coefficients)`` -- the four numbers the device driver takes, formed from the solver's
equation coefficients where the model needs them -- and goes to ``IMEXIPCSSolver.set_viscosity_model``.
"""
import math

LAW_NONE, LAW_SMAGORINSKY, LAW_CARREAU = 0, 1, 2
LAW_WALE, LAW_VREMAN = 4, 5          # (3 is no law)
LAW_DYNAMIC = 8                      # (6 and 7 are no laws)


def _checked_constant(model, name, value):
    value = float(value)
    if not (math.isfinite(value) and value >= 0.0):
        raise ValueError("%s: %s must be finite and >= 0, got %r" % (model, name, value))
    return value


def _checked_prandtl_t(model, prandtl_t):
    if prandtl_t is None:
        return None
    prandtl_t = float(prandtl_t)
    if not (math.isfinite(prandtl_t) and prandtl_t > 0.0):
        raise ValueError("%s: prandtl_t must be finite and > 0, got %r" % (model, prandtl_t))
    return prandtl_t


class SmagorinskyModel:
    """nu_x = (C_s Delta_K)^2 gamma: the Smagorinsky subgrid viscosity with the constant ``cs`` >= 0.  With a
    turbulent Prandtl number ``prandtl_t`` > 0 a solver with a transported scalar (``BoussinesqIMEXSolver``) adds the
    subgrid heat flux with the eddy diffusivity kappa_x = nu_x / prandtl_t to its transport step
    (``nsfem_set_scalar_sgs``); None: the scalar sees its molecular diffusivity alone."""
    law_id = LAW_SMAGORINSKY

    def __init__(self, cs, prandtl_t=None):
        cs = float(cs)
        if not (math.isfinite(cs) and cs >= 0.0):
            raise ValueError("SmagorinskyModel: cs must be finite and >= 0, got %r" % (cs, ))
        if prandtl_t is not None:
            prandtl_t = float(prandtl_t)
            if not (math.isfinite(prandtl_t) and prandtl_t > 0.0):
                raise ValueError("SmagorinskyModel: prandtl_t must be finite and > 0, got %r" % (prandtl_t, ))
        self.cs = cs
        self.prandtl_t = prandtl_t

    def params(self, coefficients=None):
        return (self.cs, 0.0, 0.0, 0.0)


class WALEModel:
    """nu_x = (C_w Delta_K)^2 (Sd:Sd)^(3/2) / ((S:S)^(5/2) + (Sd:Sd)^(5/4)): the wall-adapting local eddy viscosity of
    Nicoud & Ducros (1999) with the constant ``cw`` >= 0; S = sym G, Sd the traceless symmetric part of G G,
    G_ab = d_b u_a (law 4 of ``nsfem_set_viscosity_law``).  Zero in pure shear, O(y^3) at a wall.  ``prandtl_t`` as in
    ``SmagorinskyModel``."""
    law_id = LAW_WALE

    def __init__(self, cw, prandtl_t=None):
        self.cw = _checked_constant("WALEModel", "cw", cw)
        self.prandtl_t = _checked_prandtl_t("WALEModel", prandtl_t)

    def params(self, coefficients=None):
        return (self.cw, 0.0, 0.0, 0.0)


class VremanModel:
    """nu_x = c Delta_K^2 sqrt(B_beta / G:G): the eddy viscosity of Vreman (2004) with the constant ``c`` >= 0
    (c ~ 2.5 C_s^2); B_beta is the sum of the squares of the 2x2 minors of G_ab = d_b u_a (law 5 of
    ``nsfem_set_viscosity_law``).  Zero in pure shear, O(y) at a wall.  ``prandtl_t`` as in ``SmagorinskyModel``."""
    law_id = LAW_VREMAN

    def __init__(self, c, prandtl_t=None):
        self.c = _checked_constant("VremanModel", "c", c)
        self.prandtl_t = _checked_prandtl_t("VremanModel", prandtl_t)

    def params(self, coefficients=None):
        return (self.c, 0.0, 0.0, 0.0)


class CarreauModel:
    """nu = nu_inf + (nu_0 - nu_inf) (1 + (lam gamma)^2)^((n - 1)/2): the Carreau law.  nu_0, the zero-shear
    viscosity, is the solver's ``viscous_term`` coefficient, so nu_x = a [(1 + (lam gamma)^2)^((n - 1)/2) - 1] with
    a = viscous_term - nu_inf.  ``nu_inf`` finite, ``lam`` >= 0, ``n`` > 0 (n < 1 shear thinning)."""
    law_id = LAW_CARREAU

    def __init__(self, nu_inf, lam, n):
        nu_inf, lam, n = float(nu_inf), float(lam), float(n)
        if not math.isfinite(nu_inf):
            raise ValueError("CarreauModel: nu_inf must be finite, got %r" % (nu_inf, ))
        if not (math.isfinite(lam) and lam >= 0.0):
            raise ValueError("CarreauModel: lam must be finite and >= 0, got %r" % (lam, ))
        if not (math.isfinite(n) and n > 0.0):
            raise ValueError("CarreauModel: n must be finite and > 0, got %r" % (n, ))
        self.nu_inf, self.lam, self.n = nu_inf, lam, n

    def params(self, coefficients):
        nu0 = coefficients["viscous_term"]
        if nu0 is None or not math.isfinite(float(nu0)):
            raise ValueError("CarreauModel: the viscous_term coefficient (zero-shear viscosity) is not set")
        return (float(nu0) - self.nu_inf, self.lam, self.n, 0.0)


class DynamicSmagorinskyModel:
    """nu_x = c_K Delta_K^2 gamma with C_s^2 computed on the device by the Germano-Lilly procedure (law 8 of
    ``nsfem_set_viscosity_law``): test filter over the vertex patches of width ``filter_ratio`` > 1 times the grid
    filter, least squares over averaging groups of vertices, clipped to [0, ``cs2_max``].  ``averaging``: "global" (one
    group of all vertices) or ("planes", axis) -- one group per set of vertices of equal coordinate along ``axis``, for
    a channel -- or "lagrangian": LM and MM averaged along fluid path lines with an exponential memory (Meneveau, Lund &
    Cabot 1996; ``nsfem_set_dynamic_averaging``), which needs no homogeneous direction: the constant is a vertex field
    and state of the time levels.  ``relaxation`` > 0 is theta of the memory time T = theta Delta (I_LM I_MM)^(-1/8),
    ``cs2_init`` >= 0 the ratio I_LM / I_MM the state starts from and ``cs2_floor`` >= 0 the ratio it is kept above;
    the three are read in this mode only.  ``heat_flux``: None -- the scalar sees its molecular diffusivity alone -- or "dynamic": a solver with a
    transported scalar (``BoussinesqIMEXSolver``) adds the subgrid heat flux with the eddy diffusivity kappa_x = c_K
    Delta_K^2 gamma, its constant C_theta from the Germano identity of the scalar flux over the same groups, clipped to
    [0, ``ctheta_max``] (``nsfem_set_scalar_sgs_dynamic``); refused with "lagrangian" (there is no Lagrangian
    C_theta).  No fixed Pr_t goes with this model (``prandtl_t`` is
    None): Pr_t = C_s^2 / C_theta is an output."""
    law_id = LAW_DYNAMIC
    prandtl_t = None

    def __init__(self, averaging="global", filter_ratio=2.0, cs2_max=0.09, heat_flux=None, ctheta_max=0.2,
                 relaxation=1.5, cs2_init=0.0256, cs2_floor=1e-12):
        if averaging not in ("global", "lagrangian"):
            ok = isinstance(averaging, (tuple, list)) and len(averaging) == 2 and averaging[0] == "planes"
            ok = ok and isinstance(averaging[1], (int, )) and not isinstance(averaging[1], bool) and 0 <= averaging[1] <= 2
            if not ok:
                raise ValueError('DynamicSmagorinskyModel: averaging must be "global", "lagrangian" or ("planes", axis) '
                                 "with axis 0, 1 or 2, got %r" % (averaging, ))
            averaging = ("planes", int(averaging[1]))
        filter_ratio, cs2_max = float(filter_ratio), float(cs2_max)
        if not (math.isfinite(filter_ratio) and filter_ratio > 1.0):
            raise ValueError("DynamicSmagorinskyModel: filter_ratio must be finite and > 1, got %r" % (filter_ratio, ))
        if not (math.isfinite(cs2_max) and cs2_max > 0.0):
            raise ValueError("DynamicSmagorinskyModel: cs2_max must be finite and > 0, got %r" % (cs2_max, ))
        if heat_flux is not None and heat_flux != "dynamic":
            raise ValueError('DynamicSmagorinskyModel: heat_flux must be None or "dynamic", got %r' % (heat_flux, ))
        if isinstance(ctheta_max, bool):
            raise ValueError("DynamicSmagorinskyModel: ctheta_max must be a number, got %r" % (ctheta_max, ))
        ctheta_max = float(ctheta_max)
        if not (math.isfinite(ctheta_max) and ctheta_max > 0.0):
            raise ValueError("DynamicSmagorinskyModel: ctheta_max must be finite and > 0, got %r" % (ctheta_max, ))
        for name, value in (("relaxation", relaxation), ("cs2_init", cs2_init), ("cs2_floor", cs2_floor)):
            if isinstance(value, bool) or not math.isfinite(float(value)) or float(value) < 0.0 or \
                    (name == "relaxation" and float(value) == 0.0):
                raise ValueError("DynamicSmagorinskyModel: %s must be finite and %s 0, got %r"
                                 % (name, ">" if name == "relaxation" else ">=", value))
        if averaging == "lagrangian" and heat_flux == "dynamic":
            raise ValueError('DynamicSmagorinskyModel: heat_flux="dynamic" does not go with averaging="lagrangian" '
                             "(a Lagrangian C_theta is not supported)")
        self.averaging, self.filter_ratio, self.cs2_max = averaging, filter_ratio, cs2_max
        self.heat_flux, self.ctheta_max = heat_flux, ctheta_max
        self.relaxation, self.cs2_init, self.cs2_floor = float(relaxation), float(cs2_init), float(cs2_floor)

    def params(self, coefficients=None):
        return (self.filter_ratio, self.cs2_max, 0.0, 0.0)

    @property
    def lagrangian(self):
        return self.averaging == "lagrangian"

    def averaging_params(self):
        """(theta, cs2_init, cs2_floor) of ``nsfem_set_dynamic_averaging`` mode 1"""
        return (self.relaxation, self.cs2_init, self.cs2_floor)

    def vertex_groups(self, coordinates):
        """(n_groups, ids [n_vertices]) for the vertices at ``coordinates`` [n, dim]: planes in ascending coordinate,
        by the binning of ``flow_statistics.groups_along_axis``.  "lagrangian" has no groups: the global one, which
        the device keeps beside the mode and does not read"""
        import numpy as np
        coordinates = np.asarray(coordinates, dtype=np.float64)
        if self.averaging in ("global", "lagrangian"):
            return 1, np.zeros(coordinates.shape[0], dtype=np.int32)
        axis = self.averaging[1]
        if axis >= coordinates.shape[1]:
            raise ValueError("DynamicSmagorinskyModel: axis %d on a %dD mesh" % (axis, coordinates.shape[1]))
        from flow_statistics import groups_along_axis
        values, ptr, nodes = groups_along_axis(coordinates, axis)
        ids = np.empty(coordinates.shape[0], dtype=np.int32)
        for g in range(values.size):
            ids[nodes[ptr[g]:ptr[g + 1]]] = g
        return int(values.size), ids
