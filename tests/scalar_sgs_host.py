"""Subgrid heat flux of the scalar step (Smagorinsky eddy diffusivity): its numpy restatement -- the
oracle of tests/test_gpu_scalar_sgs.py and tests/test_scalar_sgs_host.py.  No tests in here.

With g_ab = d_b u_a, gamma = sqrt(2 S:S), Delta_K = (|det J_K| / dim!)^(1/dim), the Smagorinsky constant C_s and a
turbulent Prandtl number Pr_t > 0:

    kappa_x(gamma, Delta_K) = (C_s Delta_K)^2 gamma / Pr_t
    D(u, T)_i = sum_K sum_q w_q |det J_K| kappa_x(gamma_q, Delta_K) grad T_q . grad phi_i(x_q)

by the 7-point Radon / 15-point Keast rule (``rule_space`` of tests/test_variable_viscosity_host.py: the rule is part
of the definition).  gamma and nu_x at the points are those of ``VariableViscosityRestatement._at_points``."""
import numpy as np

from test_scalar_transport_host import NO_BC, ScalarIMEXRestatement
from test_variable_viscosity_host import SMAGORINSKY, VariableViscosityRestatement


class ScalarSgsRestatement:
    """``space`` from ``rule_space``; Pr_t divides, it is never inverted first"""

    def __init__(self, space, cs, prandtl_t):
        assert prandtl_t > 0.0
        self.s, self.cs, self.prandtl_t = space, float(cs), float(prandtl_t)
        self.visc = VariableViscosityRestatement(space, SMAGORINSKY, (cs, ))

    def kappa_x(self, u):
        """kappa_x [c, q] at the quadrature points"""
        return self.visc._at_points(u)[2] / self.prandtl_t

    def grad_T(self, T):
        """grad T [c, q, b] at the quadrature points"""
        return np.einsum("cqkb,ck->cqb", self.s.g2, T[self.s.p2])

    def residual(self, u, T):
        """D(u, T) [n2]"""
        de = np.einsum("cq,cq,cqb,cqib->ci", self.s.wdet, self.kappa_x(u), self.grad_T(T), self.s.g2)
        d = np.zeros(self.s.n2)
        np.add.at(d, self.s.p2.ravel(), de.ravel())
        return d

    def dissipation(self, u, T):
        """direct quadrature of kappa_x |grad T|^2 over the mesh"""
        gT = self.grad_T(T)
        return float(np.einsum("cq,cq,cqb,cqb->", self.s.wdet, self.kappa_x(u), gT, gT))

    def cell_means(self, u):
        """cell means of kappa_x: those of nu_x divided by Pr_t"""
        return self.visc.cell_means(u) / self.prandtl_t


class ScalarIMEXSgsRestatement(ScalarIMEXRestatement):
    """ScalarIMEXRestatement whose stored explicit vector is C(u) T + D(u, T): N1, and an N2 that has to be recomputed,
    carry D (``sgs``: a ScalarSgsRestatement on the rule space of the same mesh, None = the parent's scheme).
    ``penal``: a ScalarPenalRestatement of tests/test_heated_bodies_host.py for fixed heated bodies, whose H(T) joins
    the same vectors (None: no thermal body)."""

    def __init__(self, space, diffusivity, form="standard", sgs=None, penal=None):
        super().__init__(space, diffusivity, form)
        self.sgs, self.penal = sgs, penal

    def explicit(self, u, T):
        N = self.convection_matrix(u) @ T
        if self.sgs is not None:
            N = N + self.sgs.residual(u, T)
        if self.penal is not None:
            N = N + self.penal.residual(T)
        return N

    def step(self, alpha, beta, gamma, k, u1, u2, bc=NO_BC):
        import fem_oracle as fo
        T1, T2 = self.T[1], self.T[2]
        self.N1 = self.explicit(u1, T1)
        N2 = self.N2
        if N2 is None:
            N2 = self.explicit(u2, T2) if beta[1] != 0.0 else np.zeros_like(T1)
        b = self.M @ (alpha[1] * T1 + alpha[2] * T2) / k + self.kappa * (self.K @ (gamma[1] * T1 + gamma[2] * T2))
        b += beta[0] * self.N1 + beta[1] * N2
        rhs = -b
        if self.source is not None:
            rhs += self.M @ self.source
        A = (alpha[0] / k) * self.M + gamma[0] * self.kappa * self.K
        self.T[0] = fo.linear_solve_dirichlet(A.tocsr(), rhs, *bc)
