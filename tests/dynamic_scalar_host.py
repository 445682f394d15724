"""Dynamic subgrid heat flux (nsfem_set_scalar_sgs_dynamic): its numpy restatement -- the oracle of
tests/test_gpu_dynamic_scalar.py and tests/test_dynamic_scalar_host.py.  No tests in here.

Written from the definition of include/nsfem.h, on top of ``DynamicSmagorinskyRestatement`` (volumes, Delta_K^2, the
groups, ``clip``, ``cell_constant``).  With |K| = |det J_K| / dim!, G_ab = d_b u_a, S = sym G, gamma = sqrt(2 S:S) and
the 7-point / 15-point rule of ``rule_space``:

  1. cell moments   m_K[f] = |K| sum_q w_q f(x_q) / sum_q w_q  for f = T | T u_a | u_a | d_a T | Delta_K^2 gamma d_a T |
                    S_ab (pairs a <= b in row order), then |K| and |K| Delta_K^2: 14 / 21 numbers.  grad T and G are
                    formed from the differences T_k - T_0, u_k - u_0 of the nodal values, so a constant T or u gives an
                    exact 0.0
  2. test filter    at a vertex v over its cells in ascending order: W_v, hat f_v, Delta_v^2, hat gamma_v
  3. Germano        P_a = hat(T u_a) - hat T hat u_a, R_a = hat(Delta^2 gamma d_a T) - alpha^2 Delta_v^2 hat gamma
                    hat(d_a T), PR_v = P . R, RR_v = R . R
  4. groups         num_g = sum W_v PR_v, den_g = sum W_v RR_v from +0.0, ctheta_g = min(max(num_g / den_g, 0),
                    ctheta_max) where den_g > 0, else 0
  5. use            c_K = the mean over the vertices of K of ctheta_g(v), kappa_x = c_K Delta_K^2 gamma,
                    D(u, T)_i = sum_K sum_q w_q |det J_K| kappa_x grad T_q . grad phi_i(x_q)

``absolute=True`` evaluates the same chain with every input replaced by its absolute value and every difference by a
sum: the sums of the absolute contributions of each output, the scale of its rounding error."""
import numpy as np

from dynamic_model_host import DynamicSmagorinskyRestatement, pairs
from scalar_sgs_host import ScalarIMEXSgsRestatement


class DynamicScalarRestatement(DynamicSmagorinskyRestatement):
    """params = (alpha, ctheta_max); ``groups`` = (n_groups, ids [n_p1]) or None for the global group.  ``space`` from
    ``rule_space``.  ``vertex_constants``: use this vertex field C_theta instead of the restatement's own"""

    def __init__(self, space, params=(2.0, 0.2), groups=None):
        super().__init__(space, params, groups)

    # ---- 1. cell moments
    def moments(self, u, T, absolute=False):
        """[c, NM], NM = 1 + 4 dim + NS + 2"""
        s = self.s
        dim = s.dim
        ab, _ = pairs(dim)
        ue, Te = u[s.vdof], T[s.p2]                                        # [c, k, a], [c, k]
        phi2, g2 = s.phi2, s.g2[:, :, 1:]
        if absolute:
            ue, Te, phi2, g2 = np.abs(ue), np.abs(Te), np.abs(phi2), np.abs(g2)
            d, dT = ue[:, 1:] + ue[:, :1], Te[:, 1:] + Te[:, :1]
        else:
            d, dT = ue[:, 1:] - ue[:, :1], Te[:, 1:] - Te[:, :1]
        uq = np.einsum("qk,cka->cqa", phi2, ue)
        tq = np.einsum("qk,ck->cq", phi2, Te)
        G = np.einsum("cqkb,cka->cqab", g2, d)
        gT = np.einsum("cqkb,ck->cqb", g2, dT)
        sym = G + np.transpose(G, (0, 1, 3, 2))
        gamma = np.sqrt(0.5 * np.einsum("cqab,cqab->cq", sym, sym))
        f = [tq] + [tq * uq[:, :, a] for a in range(dim)] + [uq[:, :, a] for a in range(dim)]
        f += [gT[:, :, a] for a in range(dim)]
        wsum = 0.0
        for w in s.wts:
            wsum += w
        nm = 1 + 4 * dim + len(ab) + 2
        out = np.empty((s.geo.n_cells, nm))
        scale = self.vol / wsum
        for i, fi in enumerate(f):
            out[:, i] = scale * self._rule(fi)
        for a in range(dim):
            out[:, 1 + 3 * dim + a] = (scale * self.delta2) * self._rule(gamma * gT[:, :, a])
        for i, (a, b) in enumerate(ab):
            out[:, 1 + 4 * dim + i] = scale * self._rule(0.5 * sym[:, :, a, b])
        out[:, -2] = self.vol
        out[:, -1] = self.vol * self.delta2
        return out

    # ---- 2. and 3. test filter and Germano identity
    def vertices(self, u, T, absolute=False, details=False):
        """[n_p1, 3] = W, PR, RR (``details``: also dict(P, R [n_p1, dim], hat fields))"""
        s = self.s
        dim, alpha2 = s.dim, self.params[0] * self.params[0]
        _, mult = pairs(dim)
        m = self.moments(u, T, absolute)
        A = np.zeros((s.n1, m.shape[1]))
        np.add.at(A, s.p1.ravel(), np.repeat(m, dim + 1, axis=0))          # cell-major: ascending cells per vertex
        W = A[:, -2].copy()
        has = W > 0.0
        A[has] /= W[has, None]
        hT, hTu, hu = A[:, 0], A[:, 1:1 + dim], A[:, 1 + dim:1 + 2 * dim]
        hd, hgd, hs, d2 = A[:, 1 + 2 * dim:1 + 3 * dim], A[:, 1 + 3 * dim:1 + 4 * dim], A[:, 1 + 4 * dim:-2], A[:, -1]
        sgn = 1.0 if absolute else -1.0
        hgam = np.sqrt(2.0 * (mult[None, :] * hs * hs).sum(axis=1))
        P = hTu + sgn * hT[:, None] * hu
        R = hgd + sgn * ((alpha2 * d2) * hgam)[:, None] * hd
        PR, RR = np.zeros(s.n1), np.zeros(s.n1)
        for a in range(dim):
            PR = PR + P[:, a] * R[:, a]
            RR = RR + R[:, a] * R[:, a]
        out = np.stack([W, np.where(has, PR, 0.0), np.where(has, RR, 0.0)], axis=1)
        if details:
            return out, dict(P=P, R=R, hT=hT, hTu=hTu, hu=hu, hd=hd, hgd=hgd, hs=hs, d2=d2, hgam=hgam)
        return out

    # ---- 4. averaging groups
    def sums(self, u, T, absolute=False):
        """[n_groups, 2] = num, den"""
        v = self.vertices(u, T, absolute)
        out = np.zeros((self.n_groups, 2))
        np.add.at(out, self.group, np.stack([v[:, 0] * v[:, 1], v[:, 0] * v[:, 2]], axis=1))
        return out

    def constant(self, u, T):
        """ctheta [n_groups]"""
        return self.clip(self.sums(u, T))

    # ---- 5. use
    def _vertex_field(self, u, T):
        return self.vertex_constants if self.vertex_constants is not None else self.constant(u, T)[self.group]

    def kappa_x(self, u, T):
        """kappa_x [c, q] at the quadrature points; the gradient here is the full nodal sum, as the element kernel's"""
        g = self.gradient(u)
        sym = g + np.transpose(g, (0, 1, 3, 2))
        gamma = np.sqrt(0.5 * np.einsum("cqab,cqab->cq", sym, sym))
        return (self.cell_constant(self._vertex_field(u, T)) * self.delta2)[:, None] * gamma

    def grad_T(self, T):
        return np.einsum("cqkb,ck->cqb", self.s.g2, T[self.s.p2])

    def residual(self, u, T):
        """D(u, T) [n2]"""
        de = np.einsum("cq,cq,cqb,cqib->ci", self.s.wdet, self.kappa_x(u, T), self.grad_T(T), self.s.g2)
        d = np.zeros(self.s.n2)
        np.add.at(d, self.s.p2.ravel(), de.ravel())
        return d

    def dissipation(self, u, T):
        """direct quadrature of kappa_x |grad T|^2 over the mesh"""
        gT = self.grad_T(T)
        return float(np.einsum("cq,cq,cqb,cqb->", self.s.wdet, self.kappa_x(u, T), gT, gT))

    def cell_means(self, u, T):
        """sum_q w_q kappa_x / sum_q w_q per cell"""
        k = self.kappa_x(u, T)
        w = np.asarray(self.s.wts)
        return (k * w[None, :]).sum(axis=1) / w.sum()


class DynamicScalarIMEXRestatement(ScalarIMEXSgsRestatement):
    """ScalarIMEXSgsRestatement whose D(u, T) evaluates C_theta on each level pair it is formed on: ``sgs`` is a
    DynamicScalarRestatement (``residual(u, T)`` calls ``constant(u, T)``).  ``constants``: the list of the group
    constants of every explicit vector formed, in order"""

    def __init__(self, space, diffusivity, form="standard", sgs=None, penal=None):
        assert sgs is None or isinstance(sgs, DynamicScalarRestatement)
        super().__init__(space, diffusivity, form, sgs=sgs, penal=penal)
        self.constants = []

    def explicit(self, u, T):
        if self.sgs is not None:
            assert self.sgs.vertex_constants is None
            self.constants.append(self.sgs.constant(u, T))
        return super().explicit(u, T)
