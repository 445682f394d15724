"""Dynamic Smagorinsky model (law 8 of nsfem_set_viscosity_law): its numpy restatement -- the oracle of
tests/test_gpu_dynamic_model.py and tests/test_dynamic_model_host.py.  No tests in here.

Written from the definition of include/nsfem.h.  With |K| = |det J_K| / dim!, Delta_K^2, G_ab = d_b u_a, S = sym G,
gamma = sqrt(2 S:S) and the 7-point / 15-point rule of ``rule_space``:

  1. cell moments   m_K[f] = |K| sum_q w_q f(x_q) / sum_q w_q  for f = u_a | u_a u_b | S_ab | Delta_K^2 gamma S_ab
                    (pairs a <= b in row order), then |K| and |K| Delta_K^2.  G is formed from the differences
                    u_k - u_0 of the nodal values (the basis gradients sum to zero), so a constant field has G = 0
                    exactly
  2. test filter    at a vertex v over its cells in ascending order: W_v = sum |K|, hat f_v = (sum m_K[f]) / W_v,
                    Delta_v^2 = (sum |K| Delta_K^2) / W_v, hat gamma_v = sqrt(2 hat S : hat S)
  3. Germano        L = hat(u u) - hat u hat u, Ld = L - (tr L / dim) I, M = 2 (hat(Delta^2 gamma S) - alpha^2 Delta_v^2
                    hat gamma hat S), LM_v = Ld : M, MM_v = M : M (full contractions)
  4. groups         num_g = sum W_v LM_v, den_g = sum W_v MM_v over the vertices of g in ascending order from +0.0,
                    cs2_g = min(max(num_g / den_g, 0), cs2_max) where den_g > 0, else 0
  5. use            c_K = the mean over the vertices of K of cs2_g(v), nu_x = c_K Delta_K^2 gamma

``absolute=True`` evaluates the same chain with every input replaced by its absolute value and every difference by a
sum: the sums of the absolute contributions of each output, the scale of its rounding error (the idiom of
tests/test_wall_quantities_host.py)."""
import math

import numpy as np

from subgrid_models_host import SubgridModelRestatement

DYNAMIC = 8


def pairs(dim):
    """the index pairs a <= b in row order and their multiplicity in a full contraction"""
    ab = [(a, b) for a in range(dim) for b in range(a, dim)]
    return ab, np.array([1.0 if a == b else 2.0 for a, b in ab])


class DynamicSmagorinskyRestatement(SubgridModelRestatement):
    """params = (alpha, cs2_max); ``groups`` = (n_groups, ids [n_p1]) or None for the global group.  ``space`` from
    ``rule_space``.  ``residual``, ``cell_means``, ``dissipation`` and ``nu_max`` are inherited: they read ``_at_points``,
    which evaluates the constant on the field it is given (``vertex_constants``: use this vertex field instead)"""

    def __init__(self, space, params=(2.0, 0.09), groups=None):
        alpha, cs2_max = (float(p) for p in params[:2])
        assert alpha > 1.0 and cs2_max > 0.0
        self.s, self.law, self.params = space, DYNAMIC, (alpha, cs2_max)
        dim = space.dim
        self.vol = space.geo.absdet / math.factorial(dim)                  # [c]
        self.delta = self.vol ** (1.0 / dim)
        self.delta2 = self.delta * self.delta
        if groups is None:
            groups = (1, np.zeros(space.n1, dtype=np.int64))
        self.n_groups, self.group = int(groups[0]), np.asarray(groups[1], dtype=np.int64)
        assert self.group.shape == (space.n1, ) and self.group.min() >= 0 and self.group.max() < self.n_groups
        self.vertex_constants = None

    # ---- 1. cell moments
    def moments(self, u, absolute=False):
        """[c, NM], NM = dim + 3 NS + 2"""
        s = self.s
        dim = s.dim
        ab, _ = pairs(dim)
        ue = u[s.vdof]                                                     # [c, k, a]
        phi2, g2 = s.phi2, s.g2[:, :, 1:]
        if absolute:
            ue, phi2, g2 = np.abs(ue), np.abs(phi2), np.abs(g2)
            d = ue[:, 1:] + ue[:, :1]
        else:
            d = ue[:, 1:] - ue[:, :1]
        uq = np.einsum("qk,cka->cqa", phi2, ue)
        G = np.einsum("cqkb,cka->cqab", g2, d)
        sym = G + np.transpose(G, (0, 1, 3, 2))
        gamma = np.sqrt(0.5 * np.einsum("cqab,cqab->cq", sym, sym))
        f = [uq[:, :, a] for a in range(dim)]
        f += [uq[:, :, a] * uq[:, :, b] for a, b in ab]
        f += [0.5 * sym[:, :, a, b] for a, b in ab]
        ns = len(ab)
        wsum = 0.0
        for w in s.wts:
            wsum += w
        out = np.empty((s.geo.n_cells, dim + 3 * ns + 2))
        scale = self.vol / wsum
        for i, fi in enumerate(f):
            out[:, i] = scale * self._rule(fi)
        for i, (a, b) in enumerate(ab):
            out[:, dim + 2 * ns + i] = (scale * self.delta2) * self._rule(gamma * (0.5 * sym[:, :, a, b]))
        out[:, -2] = self.vol
        out[:, -1] = self.vol * self.delta2
        return out

    def _rule(self, f):
        acc = np.zeros(f.shape[0])
        for q, w in enumerate(self.s.wts):
            acc = acc + w * f[:, q]
        return acc

    # ---- 2. and 3. test filter and Germano identity
    def vertices(self, u, absolute=False, details=False):
        """[n_p1, 3] = W, LM, MM (``details``: also dict(L, Ld, M [n_p1, NS], hat fields))"""
        s = self.s
        dim, alpha2 = s.dim, self.params[0] * self.params[0]
        ab, mult = pairs(dim)
        ns = len(ab)
        m = self.moments(u, absolute)
        A = np.zeros((s.n1, m.shape[1]))
        np.add.at(A, s.p1.ravel(), np.repeat(m, dim + 1, axis=0))          # cell-major: ascending cells per vertex
        W = A[:, -2].copy()
        has = W > 0.0
        A[has] /= W[has, None]
        hu, huu, hs, hg, d2 = A[:, :dim], A[:, dim:dim + ns], A[:, dim + ns:dim + 2 * ns], A[:, dim + 2 * ns:dim + 3 * ns], A[:, -1]
        sgn = 1.0 if absolute else -1.0
        hgam = np.sqrt(2.0 * (mult[None, :] * hs * hs).sum(axis=1))
        L = np.stack([huu[:, i] + sgn * hu[:, a] * hu[:, b] for i, (a, b) in enumerate(ab)], axis=1)
        tr = sum(L[:, i] for i, (a, b) in enumerate(ab) if a == b) / dim
        Ld = np.stack([L[:, i] + sgn * tr if a == b else L[:, i] for i, (a, b) in enumerate(ab)], axis=1)
        M = 2.0 * (hg + sgn * ((alpha2 * d2) * hgam)[:, None] * hs)
        LM = (mult[None, :] * Ld * M).sum(axis=1)
        MM = (mult[None, :] * M * M).sum(axis=1)
        out = np.stack([W, np.where(has, LM, 0.0), np.where(has, MM, 0.0)], axis=1)
        if details:
            return out, dict(L=L, Ld=Ld, M=M, hu=hu, huu=huu, hs=hs, hg=hg, d2=d2, hgam=hgam)
        return out

    # ---- 4. averaging groups
    def sums(self, u, absolute=False):
        """[n_groups, 2] = num, den"""
        v = self.vertices(u, absolute)
        out = np.zeros((self.n_groups, 2))
        np.add.at(out, self.group, np.stack([v[:, 0] * v[:, 1], v[:, 0] * v[:, 2]], axis=1))
        return out

    def clip(self, sums):
        num, den = sums[:, 0], sums[:, 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.minimum(np.maximum(num / den, 0.0), self.params[1])
        return np.where(den > 0.0, q, 0.0)

    def constant(self, u):
        """cs2 [n_groups]"""
        return self.clip(self.sums(u))

    # ---- 5. use
    def cell_constant(self, cs2v):
        p1 = self.s.p1
        c = cs2v[p1[:, 0]]
        for v in range(1, self.s.dim + 1):
            c = c + cs2v[p1[:, v]]
        return c / (self.s.dim + 1.0)

    def _at_points(self, u):
        g = self.gradient(u)
        sym = g + np.transpose(g, (0, 1, 3, 2))
        gamma = np.sqrt(0.5 * np.einsum("cqab,cqab->cq", sym, sym))
        cs2v = self.vertex_constants if self.vertex_constants is not None else self.constant(u)[self.group]
        return sym, gamma, (self.cell_constant(cs2v) * self.delta2)[:, None] * gamma
