"""IMEX scalar transport (a P2 temperature on the velocity nodes): its numpy / scipy restatement -- the oracle of
tests/test_gpu_scalar_transport.py -- and what can be checked without a GPU: the two structural identities of the
convection matrix, the steady conduction profile and the temporal order of the scheme.

The restatement is ns_boussinesq_solver.py's transport step built only from fem_oracle: the scalar convection matrix is
a diagonal component block of Space.picard_convection(u, "standard") (that operator is delta -> (grad delta) u . w,
block diagonal with the blocks int (u . grad phi_j) phi_i), the skew form is 1/2 (C - C^T), M and K are mass_p2 /
stiffness_p2, the solve is linear_solve_dirichlet (sparse LU)."""
import numpy as np

import fem_oracle as fo
from fem_mesh import FacetMarkers, TaylorHoodDofMap, box_mesh, rectangle_mesh
from imex_time_stepping import IMEXTimeStepping, IMEXType

NO_BC = (np.zeros(0, np.int64), np.zeros(0))


class ScalarIMEXRestatement:
    """alpha = (a0, a1, a2), beta = (b0, b1), gamma = (g0, g1, g2) of IMEXTimeStepping, step size k, diffusivity kappa:
      (a0/k M + g0 kappa K) T0 = -[ M (a1 T1 + a2 T2)/k + kappa K (g1 T1 + g2 T2) + b0 C(u1) T1 + b1 C(u2) T2 ] + M q,
      Dirichlet rows T0_i = g_i
    C(u2) T2 is the vector C(u1) T1 kept from the previous step (recomputed when there is none)."""

    def __init__(self, space, diffusivity, form="standard"):
        assert form in ("standard", "skew_symmetric")
        self.s, self.kappa, self.form = space, float(diffusivity), form
        self.M, self.K = space.mass_p2(), space.stiffness_p2()
        self.T = [np.zeros(space.n2) for _ in range(3)]
        self.source = None
        self.N1 = self.N2 = None
        self._cached = (None, None)

    def convection_matrix(self, u):
        """C(u) in the chosen form (cached for a velocity that does not change)"""
        if self._cached[0] is not None and np.array_equal(self._cached[0], u):
            return self._cached[1]
        dim = self.s.dim
        C = self.s.picard_convection(u, "standard").tocsr()[0::dim, :][:, 0::dim].tocsr()
        if self.form == "skew_symmetric":
            C = (0.5 * (C - C.T)).tocsr()
        self._cached = (u.copy(), C)
        return C

    def step(self, alpha, beta, gamma, k, u1, u2, bc=NO_BC):
        T1, T2 = self.T[1], self.T[2]
        self.N1 = self.convection_matrix(u1) @ T1
        N2 = self.N2
        if N2 is None:
            N2 = self.convection_matrix(u2) @ T2 if beta[1] != 0.0 else np.zeros_like(T1)
        b = self.M @ (alpha[1] * T1 + alpha[2] * T2) / k + self.kappa * (self.K @ (gamma[1] * T1 + gamma[2] * T2))
        b += beta[0] * self.N1 + beta[1] * N2
        rhs = -b
        if self.source is not None:
            rhs += self.M @ self.source
        A = (alpha[0] / k) * self.M + gamma[0] * self.kappa * self.K
        self.T[0] = fo.linear_solve_dirichlet(A.tocsr(), rhs, *bc)

    def advance(self):
        self.T[2] = self.T[1].copy()
        self.T[1] = self.T[0].copy()
        self.N2, self.N1 = self.N1, None


def _square(n=8):
    mesh = rectangle_mesh((0.0, 0.0), (1.0, 1.0), n, n)
    dm = TaylorHoodDofMap(mesh)
    return mesh, dm, fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)


def _cube():
    mesh = box_mesh((0.0, 0.0, 0.0), (1.0, 0.8, 0.6), 3, 2, 2)
    dm = TaylorHoodDofMap(mesh)
    return mesh, dm, fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)


def smooth_fields(X):
    """nodal velocity (interleaved) and scalar: products of sines with different wave numbers per component, no
    symmetry, not polynomial"""
    dim = X.shape[1]
    x, y = X[:, 0], X[:, 1]
    z = X[:, 2] if dim == 3 else np.zeros_like(x)
    comps = [np.sin(1.3 * x + 0.2) * np.sin(2.1 * y + 0.5) * np.cos(0.7 * z),
             np.sin(2.7 * x + 0.9) * np.sin(0.8 * y + 0.1) * np.cos(1.9 * z + 0.3),
             np.sin(0.6 * x + 1.1) * np.sin(1.7 * y + 0.4) * np.sin(2.3 * z + 0.8)]
    u = np.stack(comps[:dim], axis=1).ravel()
    T = np.sin(1.9 * x + 0.3) * np.sin(1.1 * y + 0.7) * np.cos(1.4 * z + 0.2) + 0.4
    return u, T


def _sides(mesh, dm, axis=0):
    """P2 nodes of the two sides x_axis = 0 and x_axis = 1"""
    marks = FacetMarkers(mesh)
    marks.mark(lambda X: np.abs(X[:, axis]) < 1e-12, 1)
    marks.mark(lambda X: np.abs(X[:, axis] - 1.0) < 1e-12, 2)
    return (np.unique(dm.facet_p2_nodes(marks.facets_with_id(1))), np.unique(dm.facet_p2_nodes(marks.facets_with_id(2))))


def test_convection_matrix_annihilates_constants():
    """C(u) 1 = 0 (grad of a constant) for any u, 2D and 3D; bound: the rounding of one row sum, a few eps times the
    sum of the magnitudes of the row's entries"""
    for mesh, dm, s in (_square(4), _cube()):
        u, _ = smooth_fields(dm.p2_coords)
        C = ScalarIMEXRestatement(s, 0.0, "standard").convection_matrix(u)
        scale = abs(C).sum(axis=1).max()
        assert scale > 1e-3
        assert np.abs(C @ np.ones(s.n2)).max() <= 1e-14 * scale


def test_skew_form_conserves_the_quadratic_invariant():
    """T^T 1/2 (C - C^T) T = 0 for any u and T, 2D and 3D; bound: rounding of the quadratic form, eps-many times
    |T|^T |S| |T|"""
    for mesh, dm, s in (_square(4), _cube()):
        u, T = smooth_fields(dm.p2_coords)
        S = ScalarIMEXRestatement(s, 0.0, "skew_symmetric").convection_matrix(u)
        scale = np.abs(T) @ (abs(S) @ np.abs(T))
        assert scale > 1e-3 and abs(S + S.T).max() == 0.0
        assert abs(T @ (S @ T)) <= 1e-14 * scale
        # ... which the standard form does not have for a field that is not divergence free
        C = ScalarIMEXRestatement(s, 0.0, "standard").convection_matrix(u)
        assert abs(T @ (C @ T)) > 1e-6 * scale


def test_pure_conduction_reaches_the_linear_profile():
    """u = 0, T = 0 at x = 0 and T = 1 at x = 1, insulated elsewhere, start from zero: the steady state T = x lies in
    the P2 space.  The transient e_n = T_n - x obeys (a0/k M + K) e_(n+1) = -M (a1 e_n + a2 e_(n-1)) / k, so with
    r = 1 / (k kappa lambda_min) = 1e-6 / pi^2 about 1e-7: |e_1| <= r |e_0| (first-order start), |e_2| <= r |e_0| / 2
    (e_0 is still a level of the second step), |e_3| and |e_4| <= 3 r^2 -- below 1e-13.  What is left after four steps
    is the accuracy of the sparse LU solve, cond(A) eps with cond(A) about 1e4 on this mesh: asserted 1e-11"""
    mesh, dm, s = _square(8)
    left, right = _sides(mesh, dm)
    bd = np.concatenate([left, right])
    bv = np.concatenate([np.zeros(left.size), np.ones(right.size)])
    orc = ScalarIMEXRestatement(s, 1.0, "standard")
    u = np.zeros(2 * s.n2)
    ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=1.0e6)
    for _ in range(4):
        ts.update_coefficients()
        orc.step(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size(), u, u, (bd, bv))
        orc.advance()
        ts.advance_time()
    err = np.abs(orc.T[1] - dm.p2_coords[:, 0]).max()
    print("pure conduction: max |T - x| = %.2e" % err)
    assert err < 1e-11


# ---------------------------------------------------------------- temporal order
_KAPPA, _SPEED = 0.1, 0.5
_RATE = _KAPPA * np.pi ** 2


def _mode(X, t):
    """T = exp(-kappa pi^2 t) sin(pi x): with u = (c, 0) it solves T_t + u . grad T - kappa lap T = q for
    q = c pi cos(pi x) exp(-kappa pi^2 t); zero on x = 0 and x = 1, no flux through y = 0 and y = 1"""
    return np.exp(-_RATE * t) * np.sin(np.pi * X[:, 0])


def _mode_source(X, t):
    return _SPEED * np.pi * np.cos(np.pi * X[:, 0]) * np.exp(-_RATE * t)


def _mode_run(s, dm, bd, k, t_end):
    """SBDF2 from exact data at t = -k and t = 0 (the first-order start-up step does not enter) to t_end"""
    X = dm.p2_coords
    orc = ScalarIMEXRestatement(s, _KAPPA, "standard")
    u = np.zeros(2 * s.n2)
    u[0::2] = _SPEED
    orc.T[2], orc.T[1] = _mode(X, -k), _mode(X, 0.0)
    ts = IMEXTimeStepping(-k, t_end, IMEXType.SBDF2, desired_start_time_step=k)
    ts.update_coefficients()
    ts.advance_time()
    while not ts.is_at_end():
        ts.update_coefficients()
        assert ts.get_next_step_size() == k and ts.alpha[0] == 1.5
        orc.source = _mode_source(X, ts.next_time)
        orc.step(ts.alpha, ts.beta, ts.gamma, k, u, u, (bd, np.zeros(bd.size)))
        orc.advance()
        ts.advance_time()
    return orc.T[1]


def test_sbdf2_transport_is_second_order_in_the_step_size():
    """the decaying mode above on the unit square, n = 8, SBDF2 started from exact data at two levels, t_end = 0.5;
    error in the mass-matrix norm against k = 1/1024 on the same mesh for k = 1/16, 1/32, 1/64.  Asserted as
    test_imex_solver_host.py asserts its own order check: each ratio > 2.5, half way between first (2) and second
    order (4)."""
    mesh, dm, s = _square(8)
    left, right = _sides(mesh, dm)
    bd = np.concatenate([left, right])
    M = s.mass_p2()
    t_end = 0.5
    ref = _mode_run(s, dm, bd, 1.0 / 1024.0, t_end)
    err = []
    for k in (1.0 / 16.0, 1.0 / 32.0, 1.0 / 64.0):
        d = _mode_run(s, dm, bd, k, t_end) - ref
        err.append(float(np.sqrt(d @ (M @ d))))
    ratios = [err[0] / err[1], err[1] / err[2]]
    print("SBDF2 scalar transport errors %s ratios %s" % (err, ratios))
    assert all(np.isfinite(err)) and err[2] > 0.0
    assert ratios[0] > 2.5 and ratios[1] > 2.5, (err, ratios)


def test_hydrostatic_state_is_a_fixed_point_reached_from_rest_only_slowly():
    """closed unit box, no-slip walls, body force c_b T b = e_y (T = 1): the flow restatement started AT u = 0,
    p = y - 1/2 stays there to rounding, while started from p = 0 the splitting error of the pressure-correction scheme
    leaves max |u| of the order 1e-2 after 3 steps of k = 1/16 on box(8, 8) (2.5e-2, 2.2e-2, 1.0e-2 after steps 1, 2,
    3).  This is why tests/test_gpu_scalar_transport.py starts its hydrostatic case at the balanced pressure."""
    from test_imex_solver_host import IMEXRestatement
    mesh, dm, s = _square(8)
    marks = FacetMarkers(mesh)
    marks.mark(lambda X: (np.abs(X[:, 0]) < 1e-12) | (np.abs(X[:, 0] - 1.0) < 1e-12) |
               (np.abs(X[:, 1]) < 1e-12) | (np.abs(X[:, 1] - 1.0) < 1e-12), 1)
    nodes = np.unique(dm.facet_p2_nodes(marks.facets_with_id(1)))
    bd = np.sort(np.concatenate([2 * nodes, 2 * nodes + 1]))
    y = dm.p1_coords[:, 1]
    last = {}
    for start in ("rest", "balanced"):
        orc = IMEXRestatement(s, dict(convective_term=1.0, pressure_term=1.0, viscous_term=0.01, body_force_term=1.0))
        orc.body_force = np.outer(np.ones(s.n2), (0.0, 1.0)).ravel()
        if start == "balanced":
            orc.p_old = y - 0.5
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=1.0 / 16.0)
        for _ in range(3):
            ts.update_coefficients()
            orc.step(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size(), (bd, np.zeros(bd.size)))
            last[start] = (np.abs(orc.vel[0]).max(), np.abs(orc.p - orc.p.mean() - (y - 0.5)).max())
            orc.advance()
            ts.advance_time()
    print("hydrostatic restatement after 3 steps (max |u|, max |p - p_h|): %s" % last)
    assert last["balanced"][0] < 1e-13 and last["balanced"][1] < 1e-13
    assert 1e-3 < last["rest"][0] < 1e-1 and last["rest"][1] > 1e-3


def test_point_evaluation_of_a_p2_scalar():
    """fem_spaces.evaluate_lagrange with field "scalar" (what DeviceFunction.__call__ uses for the temperature): a
    quadratic lies in the P2 space, so the value at any point is exact to rounding; 2D and 3D"""
    from fem_spaces import evaluate_lagrange

    def fn(P):
        return 0.3 + P[..., 0] - 2.0 * P[..., 1] + 0.7 * P[..., 0] * P[..., -1] + P[..., -1] ** 2
    for mesh, dm, s in (_square(4), _cube()):
        for point in ((0.31, 0.47, 0.22), (0.9, 0.05, 0.55)):
            pt = np.array(point[:s.dim])
            value = evaluate_lagrange(dm, "scalar", fn(dm.p2_coords), pt)
            assert isinstance(value, float) and abs(value - fn(pt)) < 1e-13


def test_python_layer_of_the_feature_is_in_place():
    """the binding names the new slots, field and entry points; the solver class exists and refuses a wrong convective
    form before anything touches a device"""
    import pytest
    import _native as nat
    from grid_generator import hyper_cube
    from ns_boussinesq_solver import BoussinesqIMEXSolver
    from ns_imex_solver import IMEXIPCSSolver
    assert (nat.T0, nat.T1, nat.T2, nat.T_SOURCE, nat.TCONV_1, nat.TCONV_2) == tuple(range(11, 17))
    assert nat.SCALAR not in (nat.VELOCITY, nat.PRESSURE, nat.PRESSURE_PRECOND)
    for name in ("nsfem_set_scalar", "nsfem_step_scalar_imex", "nsfem_scalar_convection", "nsfem_scalar_info"):
        assert name in nat.EXPORTED_SYMBOLS
    for method in ("set_scalar", "step_scalar_imex", "scalar_convection", "scalar_info"):
        assert callable(getattr(nat.NsfemContext, method))
    assert issubclass(BoussinesqIMEXSolver, IMEXIPCSSolver)
    mesh, marks = hyper_cube(2, 4)
    solver = BoussinesqIMEXSolver(mesh, marks, "standard",
                                  IMEXTimeStepping(0.0, 1.0, IMEXType.SBDF2, desired_start_time_step=0.1))
    with pytest.raises(AssertionError):
        solver.set_scalar_coefficients(0.1, convective_form="rotational")
    with pytest.raises(AssertionError):
        solver.set_scalar_coefficients(0.1, buoyancy=(0.0, 1.0, 0.0))       # three entries on a 2D mesh
    solver.set_scalar_coefficients(0.1, buoyancy=(0.0, 1.0), convective_form="skew_symmetric")
    assert solver._scalar_coefficients == (0.1, (0.0, 1.0), "skew_symmetric")
