"""IMEX pressure-correction scheme: its numpy restatement (the oracle of tests/test_gpu_imex.py) and what can be
checked without a GPU -- the temporal order of the scheme and the time-stepping classes the solver classes accept.

The restatement is the three steps of ns_imex_solver.py's docstring, built from fem_oracle.Space operators and
fem_oracle.linear_solve_dirichlet (sparse LU)."""
import numpy as np
import pytest

import fem_oracle as fo
from bdf_time_stepping import BDFTimeStepping
from fem_mesh import FacetMarkers, TaylorHoodDofMap, rectangle_mesh
from imex_time_stepping import IMEXTimeStepping, IMEXType


class IMEXRestatement:
    """alpha = (a0, a1, a2), beta = (b0, b1), gamma = (g0, g1, g2) of IMEXTimeStepping, step size k:
      1. (a0/k M + g0 c_v K) u* = -[ M (a1 u1 + a2 u2)/k + c_v K (g1 u1 + g2 u2) + c_c (b0 N(u1) + b1 N(u2))
                                      - c_p D^T p_old - c_b M f + traction ],  Dirichlet rows u*_i = g_i
      2. A_p p = A_p p_old - a0/k D u*
      3. M u = M u* - k/a0 G (p - p_old)
    N(u2) is the vector kept from the previous step (recomputed when there is none)."""

    def __init__(self, space, coeffs, form="standard", traction_form=False):
        s = self.s = space
        self.c, self.form = coeffs, form
        self.M, self.K = s.vector_mass(), s.vector_stiffness(traction_form)
        self.D, self.G, self.Ap = s.divergence(), s.pressure_gradient(), s.stiffness_p1()
        self.vel = [np.zeros(s.dim * s.n2) for _ in range(3)]
        self.ustar = np.zeros(s.dim * s.n2)
        self.p, self.p_old = np.zeros(s.n1), np.zeros(s.n1)
        self.body_force = self.traction = None
        self.N1 = self.N2 = None

    def rhs(self, alpha, beta, gamma, k):
        """right-hand side of step 1 before the Dirichlet rows; sets N1"""
        c = self.c
        cc, cp, cv = c.get("convective_term") or 0.0, c["pressure_term"], c["viscous_term"]
        u1, u2 = self.vel[1], self.vel[2]
        self.N1 = self.s.convection_residual(u1, self.form)
        N2 = self.N2
        if N2 is None:
            N2 = self.s.convection_residual(u2, self.form) if beta[1] != 0.0 else np.zeros_like(u1)
        b = self.M @ (alpha[1] * u1 + alpha[2] * u2) / k + cv * (self.K @ (gamma[1] * u1 + gamma[2] * u2))
        b += cc * (beta[0] * self.N1 + beta[1] * N2) - cp * (self.D.T @ self.p_old)
        if self.body_force is not None:
            b -= c["body_force_term"] * (self.M @ self.body_force)
        if self.traction is not None:
            b += self.traction
        return -b

    def step(self, alpha, beta, gamma, k, vel_bc, p_bc=(np.zeros(0, int), np.zeros(0))):
        a0, g0 = alpha[0], gamma[0]
        A = (a0 / k) * self.M + g0 * self.c["viscous_term"] * self.K
        self.ustar = fo.linear_solve_dirichlet(A, self.rhs(alpha, beta, gamma, k), *vel_bc)
        r = self.Ap @ self.p_old - (a0 / k) * (self.D @ self.ustar)
        self.p = fo.linear_solve_dirichlet(self.Ap, r, *p_bc, pin_nullspace=(len(p_bc[0]) == 0))
        r = self.M @ self.ustar - (k / a0) * (self.G @ (self.p - self.p_old))
        self.vel[0] = fo.linear_solve_dirichlet(self.M, r, *vel_bc)

    def advance(self):
        self.vel[2] = self.vel[1].copy()
        self.vel[1] = self.vel[0].copy()
        self.p_old = self.p.copy()
        self.N2, self.N1 = self.N1, None


# ---------------------------------------------------------------- Taylor-Green vortex on the unit square
_NU = 0.1
_A = np.pi


def _tgv_velocity(X, t):
    f = np.exp(-2.0 * _A * _A * _NU * t)
    x, y = X[:, 0], X[:, 1]
    return np.stack([np.sin(_A * x) * np.cos(_A * y) * f, -np.cos(_A * x) * np.sin(_A * y) * f], axis=1)


def _tgv_pressure(X, t):
    f = np.exp(-4.0 * _A * _A * _NU * t)
    return 0.25 * (np.cos(2.0 * _A * X[:, 0]) + np.cos(2.0 * _A * X[:, 1])) * f


def _tgv_run(space, dm, bnodes, k, t_end):
    """SBDF2 from exact data at t = -k and t = 0 (so that the first-order start-up step does not enter) to t_end"""
    orc = IMEXRestatement(space, dict(convective_term=1.0, pressure_term=1.0, viscous_term=_NU), "standard")
    orc.vel[2] = _tgv_velocity(dm.p2_coords, -k).ravel()
    orc.vel[1] = _tgv_velocity(dm.p2_coords, 0.0).ravel()
    orc.p_old = _tgv_pressure(dm.p1_coords, 0.0)
    ts = IMEXTimeStepping(-k, t_end, IMEXType.SBDF2, desired_start_time_step=k)
    ts.update_coefficients()
    ts.advance_time()                      # the level t = -k is data: the scheme starts at its second step
    bd = np.sort(np.concatenate([2 * bnodes, 2 * bnodes + 1]))
    while not ts.is_at_end():
        ts.update_coefficients()
        assert ts.get_next_step_size() == k and ts.alpha[0] == 1.5
        g = _tgv_velocity(dm.p2_coords, ts.next_time).ravel()
        orc.step(ts.alpha, ts.beta, ts.gamma, k, (bd, g[bd]))
        orc.advance()
        ts.advance_time()
    return orc.vel[1]


def test_sbdf2_restatement_is_second_order_on_taylor_green():
    """Taylor-Green vortex (nu = 0.1, wave number pi) on the unit square, n = 8, Dirichlet data from the analytic
    solution, SBDF2 started from exact data at two levels, t_end = 0.5.  Velocity error in the mass-matrix norm
    against k = 1/1024 on the same mesh for k = 1/16, 1/32, 1/64.

    Measured ratios (this test prints them): e(1/16) / e(1/32) = 4.51, e(1/32) / e(1/64) = 4.18
    (errors 1.01e-3, 2.24e-4, 5.36e-5; above 4 because the reference run is not infinitely fine);
    asserted: each > 2.5, half way between first (2) and second order (4)."""
    mesh = rectangle_mesh((0.0, 0.0), (1.0, 1.0), 8, 8)
    dm = TaylorHoodDofMap(mesh)
    marks = FacetMarkers(mesh)
    marks.mark(lambda X: (np.abs(X[:, 0]) < 1e-12) | (np.abs(X[:, 0] - 1.0) < 1e-12) |
               (np.abs(X[:, 1]) < 1e-12) | (np.abs(X[:, 1] - 1.0) < 1e-12), 1)
    bnodes = np.unique(dm.facet_p2_nodes(marks.facets_with_id(1)))
    space = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
    M = space.vector_mass()
    t_end = 0.5
    ref = _tgv_run(space, dm, bnodes, 1.0 / 1024.0, t_end)
    err = []
    for k in (1.0 / 16.0, 1.0 / 32.0, 1.0 / 64.0):
        d = _tgv_run(space, dm, bnodes, k, t_end) - ref
        err.append(float(np.sqrt(d @ (M @ d))))
    ratios = [err[0] / err[1], err[1] / err[2]]
    print("SBDF2 Taylor-Green errors %s ratios %s" % (err, ratios))
    assert all(np.isfinite(err)) and err[2] > 0.0
    assert ratios[0] > 2.5 and ratios[1] > 2.5, (err, ratios)


def test_solver_classes_accept_their_own_time_stepping_only():
    """IMEXIPCSSolver refuses a BDFTimeStepping, IPCSSolver still refuses an IMEXTimeStepping (both assert in their
    constructors before anything touches a device)"""
    from grid_generator import hyper_cube
    from ns_imex_solver import IMEXIPCSSolver
    from ns_ipcs_solver import IPCSSolver
    from ns_solver_base import WeakFormConvectiveTerm
    mesh, marks = hyper_cube(2, 4)
    form = WeakFormConvectiveTerm.standard_form
    with pytest.raises(AssertionError):
        IMEXIPCSSolver(mesh, marks, form, BDFTimeStepping(0.0, 1.0, desired_start_time_step=0.1))
    with pytest.raises(AssertionError):
        IPCSSolver(mesh, marks, form, IMEXTimeStepping(0.0, 1.0, IMEXType.SBDF2, desired_start_time_step=0.1))
    assert IMEXIPCSSolver.time_stepping_class is IMEXTimeStepping and IMEXIPCSSolver.imex_type is IMEXType.SBDF2
    assert not hasattr(IPCSSolver, "time_stepping_class")
