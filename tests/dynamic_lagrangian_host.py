"""Lagrangian-averaged dynamic Smagorinsky model (mode 1 of nsfem_set_dynamic_averaging; Meneveau, Lund &
Cabot, JFM 319, 1996): its numpy restatement -- the oracle of tests/test_gpu_dynamic_lagrangian.py and
tests/test_dynamic_lagrangian_host.py.  No tests in here.

Written from the definition of include/nsfem.h, line by line.  With k the step size, vert[v] = (W_v, LM_v, MM_v) of the
level, Delta_v^2 the patch mean of Delta_K^2, I = (I_LM, I_MM) the state of the level before; plain IEEE double
arithmetic (Python floats, numpy entry by entry), sums from +0.0 in the order written:

  1. displacement    d = -k u_v, u_v the velocity at the P2 node of v
  2. upstream cell   per patch cell c (ascending), i the local index of v: lambda_j = grad(lambda_j) . d (j != i),
                     lambda_i = 1 - sum_{j != i} lambda_j, m_c = min_j lambda_j; c* the first cell of the largest m_c;
                     m_c* < 0: lambda_j <- max(lambda_j, 0), each divided by their sum
  3. upstream value  I_up = sum_j lambda_j I[p1[c*][j]]
  4. relaxation      prod = I_LM_up I_MM_up; prod > 0: T = theta sqrt(Delta_v^2) / sqrt(sqrt(sqrt(prod))), eps = k / (k + T),
                     else eps = 1; I_MM' = eps MM_v + (1 - eps) I_MM_up, I_LM' = max(eps LM_v + (1 - eps) I_LM_up,
                     cs2_floor I_MM'); a vertex of no cell: I' = 0
  5. constant        cs2_v = min(max(I_LM' / I_MM', 0), cs2_max) where I_MM' > 0, else 0
  6. initialisation  state None: I_MM = MM_v, I_LM = cs2_init MM_v, cs2_v by 5

``absolute=True``: the sums of the absolute contributions of I' and I_up, eps |LM_v| + (1 - eps) sum_j lambda_j |I_j| and
sum_j lambda_j |I_j| -- the scale of their rounding error.

The time levels of the device (``form_level`` / ``rotate`` / ``level_constants``): level n is formed once from the stored
state, ``rotate`` is nsfem_advance."""
import math

import numpy as np

from dynamic_model_host import DynamicSmagorinskyRestatement


class LagrangianDynamicRestatement(DynamicSmagorinskyRestatement):
    """params = (alpha, cs2_max) of law 8, lagrangian = (theta, cs2_init, cs2_floor).  ``space`` from ``rule_space``"""

    def __init__(self, space, params=(2.0, 0.09), lagrangian=(1.5, 0.0256, 1e-12)):
        super().__init__(space, params, None)
        self.theta, self.cs2_init, self.cs2_floor = (float(x) for x in lagrangian)
        assert self.theta > 0.0 and self.cs2_init >= 0.0 and self.cs2_floor >= 0.0
        s = space
        nl = s.dim + 1
        self.grad = s.g1[:, 0]                                             # [c, j, a] = d lambda_j / d x_a
        self.patch = [[] for _ in range(s.n1)]                             # per vertex: (cell, local index), ascending
        for c in range(s.p1.shape[0]):
            for i in range(nl):
                self.patch[int(s.p1[c, i])].append((c, i))
        self.vnode = np.array([s.p2[p[0][0], p[0][1]] if p else 0 for p in self.patch], dtype=np.int64)
        W, D = np.zeros(s.n1), np.zeros(s.n1)
        np.add.at(W, s.p1.ravel(), np.repeat(self.vol, nl))                # cell-major: ascending cells per vertex
        np.add.at(D, s.p1.ravel(), np.repeat(self.vol * self.delta2, nl))
        self.patch_volume = W
        with np.errstate(divide="ignore", invalid="ignore"):
            self.vertex_delta2 = np.where(W > 0.0, D / W, 0.0)
        # the time levels
        self.I = self.I_new = self.cs2_cur = self.cs2_prev = None

    def vertex_velocity(self, u):
        """u_v [n_p1, dim]: the velocity at the P2 node of every vertex"""
        return u.reshape(-1, self.s.dim)[self.vnode]

    # ---- rules 1 and 2
    def locate(self, u_vertices, k, rank=0, tie=1e-9):
        """lam [n_p1, dim + 1], ids [n_p1, dim + 1] (the vertices of c*), dict(cstar, clamped, best, second, tied):
        ``second`` the second-largest m_c of the patch (-inf with one cell), ``tied`` the number of cells whose m_c lies
        within ``tie`` of the best.  ``rank`` = 0 is the definition.  ``rank`` = r > 0 takes, at a vertex with at
        least r tied cells beside c*, the r-th of those (ascending) in the place of c* -- what a device that rounds
        m_c otherwise may choose where the tie is exact by the mesh's structure (tests only)"""
        s = self.s
        dim, nl, n1 = s.dim, s.dim + 1, s.n1
        lam, ids = np.zeros((n1, nl)), np.tile(np.arange(n1)[:, None], (1, nl))
        cstar, clamped = np.full(n1, -1), np.zeros(n1, dtype=bool)
        best_m, second_m, tied_n = np.full(n1, -math.inf), np.full(n1, -math.inf), np.zeros(n1, dtype=np.int64)
        for v in range(n1):
            d = [-(k * float(u_vertices[v, a])) for a in range(dim)]
            best, second, keep, every = -math.inf, -math.inf, None, []
            for c, i in self.patch[v]:
                l, total = [0.0] * nl, 0.0
                for j in range(nl):
                    if j == i:
                        continue
                    t = 0.0
                    for a in range(dim):
                        t += float(self.grad[c, j, a]) * d[a]
                    l[j] = t
                    total += t
                l[i] = 1.0 - total
                m = min(l)
                every.append((m, c, l))
                if m > best:
                    second, best, keep = best, m, (c, l)
                elif m > second:
                    second = m
            if keep is None:
                continue
            c, l = keep
            close = [(cc, ll) for m, cc, ll in every if m >= best - tie]
            tied_n[v] = len(close)
            others = [x for x in close if x[0] != c]
            if 0 < rank <= len(others):
                c, l = others[rank - 1]
            if best < 0.0:
                clamped[v] = True
                l = [max(x, 0.0) for x in l]
                total = 0.0
                for x in l:
                    total += x
                l = [x / total for x in l]
            lam[v], ids[v], cstar[v], best_m[v], second_m[v] = l, s.p1[c], c, best, second
        return lam, ids, dict(cstar=cstar, clamped=clamped, best=best_m, second=second_m, tied=tied_n)

    # ---- rules 3 to 6
    def advance(self, vert, delta2, u_vertices, k, state, absolute=False, rank=0):
        """one application to ``state`` [n_p1, 2] = I_LM, I_MM (None: rule 6) -> dict(state [n_p1, 2], upstream
        [n_p1, 2], cs2 [n_p1], eps, lam, ids, cstar, clamped, best, second); ``absolute``: (|I'| scale, |I_up| scale)"""
        n1 = self.s.n1
        has = vert[:, 0] > 0.0
        LM, MM = vert[:, 1], vert[:, 2]
        if state is None:
            imm = np.where(has, MM, 0.0)
            ilm = np.where(has, self.cs2_init * MM, 0.0)
            new = np.stack([ilm, imm], axis=1)
            if absolute:
                return np.abs(new), np.abs(new)
            return dict(state=new, upstream=new.copy(), cs2=self.clip_quotient(new), eps=np.ones(n1))
        lam, ids, where = self.locate(u_vertices, k, rank)
        src = np.abs(state) if absolute else state
        up = np.zeros((n1, 2))
        for j in range(self.s.dim + 1):
            up = up + lam[:, j, None] * src[ids[:, j]]
        real_up = up
        if absolute:
            real_up = np.zeros((n1, 2))
            for j in range(self.s.dim + 1):
                real_up = real_up + lam[:, j, None] * state[ids[:, j]]
        prod = real_up[:, 0] * real_up[:, 1]
        eps = np.ones(n1)
        pos = prod > 0.0
        T = (self.theta * np.sqrt(delta2[pos])) / np.sqrt(np.sqrt(np.sqrt(prod[pos])))
        eps[pos] = k / (k + T)
        keep = 1.0 - eps
        if absolute:
            amm = eps * np.abs(MM) + keep * up[:, 1]
            alm = np.maximum(eps * np.abs(LM) + keep * up[:, 0], self.cs2_floor * amm)
            return np.where(has[:, None], np.stack([alm, amm], axis=1), 0.0), np.where(has[:, None], up, 0.0)
        imm = eps * MM + keep * up[:, 1]
        ilm = np.maximum(eps * LM + keep * up[:, 0], self.cs2_floor * imm)
        new = np.where(has[:, None], np.stack([ilm, imm], axis=1), 0.0)
        up = np.where(has[:, None], up, 0.0)
        return dict(state=new, upstream=up, cs2=self.clip_quotient(new), eps=eps, lam=lam, ids=ids, **where)

    def clip_quotient(self, state):
        """rule 5"""
        ilm, imm = state[:, 0], state[:, 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.minimum(np.maximum(ilm / imm, 0.0), self.params[1])
        return np.where(imm > 0.0, q, 0.0)

    # ---- the time levels
    def reset(self):
        self.I = self.I_new = self.cs2_cur = self.cs2_prev = None

    def apply(self, u, k, init=False):
        """the rules on the velocity u with the stored state (``init``: rule 6); writes nothing"""
        return self.advance(self.vertices(u), self.vertex_delta2, self.vertex_velocity(u), k, None if init else self.I)

    def form_level(self, u, k):
        """level n, once (nsfem_step_imex); returns cs2_cur"""
        if self.cs2_cur is None:
            out = self.apply(u, k)
            self.I_new, self.cs2_cur = out["state"], out["cs2"]
        return self.cs2_cur

    def rotate(self):
        """nsfem_advance"""
        if self.cs2_cur is not None:
            self.I = self.I_new
        self.cs2_prev, self.cs2_cur, self.I_new = self.cs2_cur, None, None

    def level_constants(self, u, level, k):
        """the vertex field an explicit vector of the level is formed with: 0 = n (formed and kept), 1 = n-1 (cs2_prev,
        else rule 6 on u, nothing written)"""
        if level == 0:
            return self.form_level(u, k)
        return self.cs2_prev if self.cs2_prev is not None else self.apply(u, k, init=True)["cs2"]
