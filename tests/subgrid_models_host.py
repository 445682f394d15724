"""WALE and Vreman subgrid viscosities (laws 4 and 5 of nsfem_set_viscosity_law): their numpy restatement
-- the oracle of tests/test_gpu_subgrid_models.py and tests/test_subgrid_models_host.py.  No tests in here.

Both laws take the whole velocity-gradient tensor G_ab = d_b u_a at a quadrature point, not the shear rate alone.  A
2D field is the 3D field that does not depend on z (G with a zero third row and column).  With Delta_K as for laws 1
and 2:

    law 4, WALE    S = sym G, H = G G, Sd = sym H - (tr H / 3) I_3, A = S:S, B = Sd:Sd (entry by entry),
                   nu_x = (C_w Delta_K)^2 B sqrt(B) / (A^2 sqrt(A) + B sqrt(sqrt(B))),  0 where the denominator is not > 0
    law 5, Vreman  B_beta = the sum of the squares of the 2x2 minors of G,
                   nu_x = c Delta_K^2 sqrt(B_beta / G:G),  0 where G:G is not > 0

V(u), the cell means and the dissipation are those of ``VariableViscosityRestatement`` with this nu_x in place of its
own, by the same 7-point / 15-point rules (``rule_space``)."""
import math

import numpy as np

from scalar_sgs_host import ScalarSgsRestatement
from test_variable_viscosity_host import CARREAU, SMAGORINSKY, VariableViscosityRestatement

WALE, VREMAN = 4, 5


def wale_nu(G, delta2, cw):
    """G [..., d, d] with d = 2 or 3, delta2 broadcastable against G[..., 0, 0]"""
    d = G.shape[-1]
    Gt = np.swapaxes(G, -1, -2)
    S = 0.5 * (G + Gt)
    A = (S * S).sum(axis=(-1, -2))
    H = G @ G
    t3 = np.trace(H, axis1=-2, axis2=-1) / 3.0
    Sd = 0.5 * (H + np.swapaxes(H, -1, -2)) - t3[..., None, None] * np.eye(d)
    B = (Sd * Sd).sum(axis=(-1, -2))
    if d == 2:
        B = B + t3 * t3                     # Sd_33 = -tr H / 3 of the z-independent extension
    den = A * A * np.sqrt(A) + B * np.sqrt(np.sqrt(B))
    with np.errstate(divide="ignore", invalid="ignore"):
        nu = (cw * cw * delta2) * (B * np.sqrt(B) / den)
    return np.where(den > 0.0, nu, 0.0)


def vreman_nu(G, delta2, c):
    """G [..., d, d] with d = 2 or 3"""
    d = G.shape[-1]
    gg = (G * G).sum(axis=(-1, -2))
    bb = np.zeros_like(gg)
    for a in range(d):
        for a2 in range(a + 1, d):
            for b in range(d):
                for b2 in range(b + 1, d):
                    minor = G[..., a, b] * G[..., a2, b2] - G[..., a, b2] * G[..., a2, b]
                    bb = bb + minor * minor
    with np.errstate(divide="ignore", invalid="ignore"):
        nu = (c * delta2) * np.sqrt(bb / gg)
    return np.where(gg > 0.0, nu, 0.0)


def tensor_nu(law, G, delta2, p0):
    assert law in (WALE, VREMAN)
    return wale_nu(G, delta2, p0) if law == WALE else vreman_nu(G, delta2, p0)


def embed(G2):
    """the 3 x 3 tensor of the z-independent extension of a 2D field"""
    G3 = np.zeros(G2.shape[:-2] + (3, 3))
    G3[..., :2, :2] = G2
    return G3


class SubgridModelRestatement(VariableViscosityRestatement):
    """law 4 WALE params = (C_w, ), law 5 Vreman params = (c, ); laws 1 and 2 are the parent's.  ``space`` from
    ``rule_space``.  ``residual``, ``cell_means`` and ``dissipation`` are inherited: they read ``_at_points`` only"""

    def __init__(self, space, law, params):
        if law in (SMAGORINSKY, CARREAU):
            super().__init__(space, law, params)
            return
        assert law in (WALE, VREMAN)
        self.s, self.law, self.params = space, law, tuple(float(p) for p in params)
        self.delta = (space.geo.absdet / math.factorial(space.dim)) ** (1.0 / space.dim)     # [c]

    def gradient(self, u):
        """G [c, q, a, b] = d_b u_a at the quadrature points"""
        return np.einsum("cqkb,cka->cqab", self.s.g2, u[self.s.vdof])

    def _at_points(self, u):
        if self.law in (SMAGORINSKY, CARREAU):
            return super()._at_points(u)
        g = self.gradient(u)
        sym = g + np.transpose(g, (0, 1, 3, 2))
        gamma = np.sqrt(0.5 * np.einsum("cqab,cqab->cq", sym, sym))
        return sym, gamma, tensor_nu(self.law, g, (self.delta * self.delta)[:, None], self.params[0])

    def nu_max(self, u):
        return float(self._at_points(u)[2].max())


class SubgridScalarSgsRestatement(ScalarSgsRestatement):
    """ScalarSgsRestatement with kappa_x = nu_x / Pr_t of any subgrid law (1, 4, 5): only ``visc`` differs"""

    def __init__(self, space, law, params, prandtl_t):
        assert prandtl_t > 0.0 and law in (SMAGORINSKY, WALE, VREMAN)
        self.s, self.cs, self.prandtl_t = space, float(params[0]), float(prandtl_t)
        self.visc = SubgridModelRestatement(space, law, params)
