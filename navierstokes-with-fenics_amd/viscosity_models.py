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
