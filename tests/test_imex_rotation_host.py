"""Rotating frames in the IMEX pressure-correction scheme: the numpy restatement (the oracle of
tests/test_gpu_imex_rotation.py) and what can be checked without a GPU -- sign, factor and temporal order of the
explicit Coriolis term on a Taylor-Green vortex seen from a rotating frame, the stability of the explicit treatment on
the scalar test equation, and the Python layer's opt-in.

Scheme: the Coriolis vector is extrapolated with the convective term, N(u) = c_c conv(u) + M (2 c_cor Omega x u) with
Omega taken at the time of the level u belongs to, and the Euler term c_e M (dOmega/dt x x) joins the step-constant
vector; matrix, projection and correction are those of IMEXRestatement."""
import os
import re

import numpy as np
import scipy.sparse as sp

import fem_oracle as fo
from fem_mesh import FacetMarkers, TaylorHoodDofMap, rectangle_mesh
from imex_time_stepping import IMEXTimeStepping, IMEXType
from test_imex_solver_host import _A, _NU, IMEXRestatement, _tgv_pressure, _tgv_velocity

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


class RotatingIMEXRestatement(IMEXRestatement):
    """IMEXRestatement in a rotating frame.  w1, w2: the angular velocity at t^n, t^(n-1) (a number about e_z in 2D, a
    3-vector in 3D), w_dot: dOmega/dt of the step.  Stored explicit vectors (c_c inside, as the device stores them):
      N1 = c_c conv(u1) + 2 c_cor w1 (M J u1),  J = kron(I, [[0, -1], [1, 0]])   (3D: kron(M_p2, [Omega]_x) u1)
      N2 likewise with w2 -- the vector kept from the previous step while it was formed with this w2, else recomputed;
    the Euler term is + c_e M (w_dot x x) inside the bracket of the right-hand side, next to - c_b M f."""

    def __init__(self, space, coeffs, form="standard", traction_form=False):
        super().__init__(space, coeffs, form, traction_form)
        zero = 0.0 if space.dim == 2 else np.zeros(3)
        self.w1, self.w2, self.w_dot = zero, zero, zero
        self.N1_w = self.N2_w = None
        self.recomputed = 0
        self._Mp2 = space.mass_p2()

    def coriolis_matrix(self, w):
        """M (w x .) on the interleaved velocity vector"""
        if self.s.dim == 2:
            return float(w) * sp.kron(self._Mp2, np.array([[0.0, -1.0], [1.0, 0.0]]), format="csr")
        wx, wy, wz = (float(v) for v in w)
        return sp.kron(self._Mp2, np.array([[0.0, -wz, wy], [wz, 0.0, -wx], [-wy, wx, 0.0]]), format="csr")

    def explicit_vector(self, u, w):
        cc = self.c.get("convective_term") or 0.0
        N = cc * self.s.convection_residual(u, self.form) if cc else np.zeros_like(u)
        if np.any(w):
            N = N + 2.0 * self.c["coriolis_term"] * (self.coriolis_matrix(w) @ u)
        return N

    def rhs(self, alpha, beta, gamma, k):
        c = self.c
        cp, cv = c["pressure_term"], c["viscous_term"]
        u1, u2 = self.vel[1], self.vel[2]
        self.N1 = self.explicit_vector(u1, self.w1)
        self.N1_w = np.array(self.w1, dtype=float)
        N2 = np.zeros_like(u1)
        if beta[1] != 0.0:
            if self.N2 is not None and np.array_equal(self.N2_w, np.array(self.w2, dtype=float)):
                N2 = self.N2
            else:
                self.recomputed += self.N2 is not None
                N2 = self.explicit_vector(u2, self.w2)
        b = self.M @ (alpha[1] * u1 + alpha[2] * u2) / k + cv * (self.K @ (gamma[1] * u1 + gamma[2] * u2))
        b += beta[0] * self.N1 + beta[1] * N2 - cp * (self.D.T @ self.p_old)
        bracket = np.zeros_like(u1)
        if self.body_force is not None:
            bracket -= c["body_force_term"] * self.body_force
        if np.any(self.w_dot):
            X = self.s.p2_nodes()
            if self.s.dim == 2:
                bracket += c["euler_term"] * float(self.w_dot) * np.stack([-X[:, 1], X[:, 0]], axis=1).ravel()
            else:
                bracket += c["euler_term"] * np.cross(np.asarray(self.w_dot, dtype=float)[None, :], X).ravel()
        b += self.M @ bracket
        if self.traction is not None:
            b += self.traction
        return -b

    def advance(self):
        super().advance()
        self.N2_w, self.N1_w = self.N1_w, None


# ---------------------------------------------------------------- Taylor-Green vortex seen from a rotating frame
_OMEGA, _CCOR = 2.0, 1.0


def _psi(X, t):
    """stream function of the Taylor-Green velocity, u = (d psi / dy, -d psi / dx)"""
    return np.sin(_A * X[:, 0]) * np.sin(_A * X[:, 1]) * np.exp(-2.0 * _A * _A * _NU * t) / _A


def _rotating_tgv_run(space, dm, bnodes, k, t_end):
    """SBDF2 from exact data at t = -k and t = 0 to t_end, steady frame; returns (velocity, pressure) at t_end"""
    coef = dict(convective_term=1.0, pressure_term=1.0, viscous_term=_NU, coriolis_term=_CCOR, euler_term=_CCOR)
    orc = RotatingIMEXRestatement(space, coef, "standard")
    orc.w1 = orc.w2 = _OMEGA
    orc.vel[2] = _tgv_velocity(dm.p2_coords, -k).ravel()
    orc.vel[1] = _tgv_velocity(dm.p2_coords, 0.0).ravel()
    orc.p_old = _tgv_pressure(dm.p1_coords, 0.0) - 2.0 * _CCOR * _OMEGA * _psi(dm.p1_coords, 0.0)
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
    return orc.vel[1], orc.p_old


def test_rotating_taylor_green_keeps_second_order_and_shifts_the_pressure():
    """In 2D the Coriolis force of a solenoidal field is a gradient, 2 c_cor Omega e_z x u = grad(2 c_cor Omega psi):
    the velocity is the non-rotating Taylor-Green one and p = p_tgv - 2 c_cor Omega psi.  Unit square n = 8, nu = 0.1,
    Omega = 2, c_cor = 1, SBDF2 from exact data at two levels, t_end = 0.5; velocity error in the mass norm against
    k = 1/1024 for k = 1/16, 1/32, 1/64.

    Measured (printed): errors 1.64e-3, 3.79e-4, 9.10e-5, ratios 4.33 and 4.16; fine-run pressure error 5.8e-3 against
    |2 c_cor Omega psi| = 1.36e-1 (P1 mass norm, means removed); against p_tgv alone the fine-run pressure is off by
    1.40e-1.  Asserted: both ratios > 2.5 (the bound of the non-rotating order test) and the pressure error below a
    tenth of the Coriolis pressure -- a wrong sign doubles it, a missing factor 2 halves the correction."""
    mesh = rectangle_mesh((0.0, 0.0), (1.0, 1.0), 8, 8)
    dm = TaylorHoodDofMap(mesh)
    marks = FacetMarkers(mesh)
    marks.mark(lambda X: (np.abs(X[:, 0]) < 1e-12) | (np.abs(X[:, 0] - 1.0) < 1e-12) |
               (np.abs(X[:, 1]) < 1e-12) | (np.abs(X[:, 1] - 1.0) < 1e-12), 1)
    bnodes = np.unique(dm.facet_p2_nodes(marks.facets_with_id(1)))
    space = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
    M, M1 = space.vector_mass(), space.mass_p1()
    t_end = 0.5
    ref, p_fine = _rotating_tgv_run(space, dm, bnodes, 1.0 / 1024.0, t_end)
    err = []
    for k in (1.0 / 16.0, 1.0 / 32.0, 1.0 / 64.0):
        d = _rotating_tgv_run(space, dm, bnodes, k, t_end)[0] - ref
        err.append(float(np.sqrt(d @ (M @ d))))
    ratios = [err[0] / err[1], err[1] / err[2]]

    def norm1(p):
        one = np.ones_like(p)
        q = p - (one @ (M1 @ p)) / (one @ (M1 @ one))
        return float(np.sqrt(q @ (M1 @ q)))

    p_cor = 2.0 * _CCOR * _OMEGA * _psi(dm.p1_coords, t_end)
    p_tgv = _tgv_pressure(dm.p1_coords, t_end)
    e_p, e_plain, size = norm1(p_fine - (p_tgv - p_cor)), norm1(p_fine - p_tgv), norm1(p_cor)
    print("rotating Taylor-Green errors %s ratios %s; pressure error %.3e, without the correction %.3e, |2 c Omega psi| "
          "%.3e" % (err, ratios, e_p, e_plain, size))
    assert all(np.isfinite(err)) and err[2] > 0.0
    assert ratios[0] > 2.5 and ratios[1] > 2.5, (err, ratios)
    assert e_p < 0.1 * size, (e_p, size)


# ---------------------------------------------------------------- stability of the explicit treatment
def _second_order_coefficients(typ):
    ts = IMEXTimeStepping(0.0, 1.0, typ, desired_start_time_step=0.125)
    for _ in range(3):                     # past the first-order step, constant step size
        ts.update_coefficients()
        ts.advance_time()
    ts.update_coefficients()
    return list(ts.alpha), list(ts.beta), list(ts.gamma)


def _largest_root(typ, x, z):
    """y' = -x/k y + i z/k y, x implicit and z explicit:
    (a0 + g0 x) r^2 + (a1 + g1 x - i z b0) r + (a2 + g2 x - i z b1) = 0"""
    a, b, g = _second_order_coefficients(typ)
    return float(np.abs(np.roots([a[0] + g[0] * x, a[1] + g[1] * x - 1j * z * b[0], a[2] + g[2] * x - 1j * z * b[1]])).max())


# the table of DESIGN.md 4n: (scheme, x) -> moduli at z = 0.03, 0.1, 0.3, 0.6
_TABLE = {("SBDF2", 0.0): (1.000001, 1.000077, 1.00745, 1.132), ("SBDF2", 0.1): (0.9044, 0.9035, 0.9033, 1.031),
          ("CNAB", 0.0): (1.000000, 1.000026, 1.00244, 1.068), ("mCNAB", 0.0): (1.000000, 1.000026, 1.00244, 1.068),
          ("CNAB", 0.1): (0.9047, 0.9040, 0.8997, 0.945), ("CNLF", 0.0): (1.0, 1.0, 1.0, 1.0)}


def test_stability_table_of_the_explicit_coriolis_term():
    """the largest root moduli of the design document, recomputed from IMEXTimeStepping's coefficients; without damping
    SBDF2, CNAB and mCNAB grow by no more than 1 + z^4 per step up to z = 0.3, CNLF is neutral"""
    zs = (0.03, 0.1, 0.3, 0.6)
    for (name, x), want in _TABLE.items():
        got = [_largest_root(IMEXType[name], x, z) for z in zs]
        print("%-6s x = %.1f: %s" % (name, x, ", ".join("%.6f" % v for v in got)))
        for v, w in zip(got, want):
            digits = len(repr(w).split(".")[1]) if w != 1.0 else 6
            assert abs(v - w) <= 0.51 * 10.0 ** -digits + 1e-12, (name, x, got, want)
    for name in ("SBDF2", "CNAB", "mCNAB"):
        for z in (0.01, 0.03, 0.1, 0.2, 0.3):
            r = _largest_root(IMEXType[name], 0.0, z)
            assert 1.0 <= r + 1e-14 and r <= 1.0 + z ** 4, (name, z, r)
    for z in (0.03, 0.1, 0.3, 0.6, 0.99):
        assert abs(_largest_root(IMEXType.CNLF, 0.0, z) - 1.0) < 1e-13, z


# ---------------------------------------------------------------- the Python layer
class _RecordingContext:
    def __init__(self):
        self.calls = []

    def set_imex(self, *args):
        self.calls.append(("set_imex", ) + args)

    def set_imex_rotation(self, *args):
        self.calls.append(("set_imex_rotation", ) + args)


def test_python_layer_declares_wraps_and_opts_in():
    """the header declares the two exports, _native lists them and wraps them, and the solver classes opt in only when
    an angular velocity has been set -- with Omega at the two OLD levels of the time stepping"""
    import _native as nat
    from auxiliary_classes import AngularVelocityVector, FunctionTime
    from ns_boussinesq_solver import BoussinesqIMEXSolver
    from ns_imex_solver import IMEXIPCSSolver

    header = open(os.path.join(ROOT, "include", "nsfem.h")).read()
    assert re.search(r"int nsfem_set_imex_rotation\(nsfem_ctx\* ctx, int treatment, const double\* omega_n, "
                     r"const double\* omega_nm1\);", header)
    assert re.search(r"int nsfem_imex_rotation_info\(nsfem_ctx\* ctx, int64_t out\[4\]\);", header)
    source = open(nat.__file__).read()
    for name in ("nsfem_set_imex_rotation", "nsfem_imex_rotation_info"):
        assert name in nat.EXPORTED_SYMBOLS
        assert re.search(r'"%s": \(C\.c_int, \[vp, ' % name, source), name
    assert callable(nat.NsfemContext.set_imex_rotation) and callable(nat.NsfemContext.imex_rotation_info)
    integration = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "`nsfem_set_imex_rotation`" in integration and "`nsfem_imex_rotation_info`" in integration

    class Ramp(FunctionTime):
        def __init__(self):
            super().__init__(1)

        def value(self):
            return 0.5 + 0.8 * self._current_time

        def derivative(self):
            return 0.8

    assert issubclass(BoussinesqIMEXSolver, IMEXIPCSSolver)
    for cls in (IMEXIPCSSolver, BoussinesqIMEXSolver):
        solver = object.__new__(cls)
        solver._ctx = _RecordingContext()
        solver._time_stepping = ts = IMEXTimeStepping(0.0, 1.0, IMEXType.SBDF2, desired_start_time_step=0.125)
        solver._update_time_stepping_coefficients()
        assert [c[0] for c in solver._ctx.calls] == ["set_imex"]          # no angular velocity: nothing else is called
        av = AngularVelocityVector(2, Ramp())
        solver._angular_velocity = av
        solver._update_time_stepping_coefficients()
        assert solver._ctx.calls[-1] == ("set_imex_rotation", 1, 0.5, None)  # first step: t^n only
        ts.advance_time()
        ts.update_coefficients()
        ts.advance_time()                                                    # t^n = 0.25, t^(n-1) = 0.125
        av.set_time(ts.next_time)                                            # the vector itself sits at the new level
        solver._update_time_stepping_coefficients()
        assert solver._ctx.calls[-1] == ("set_imex_rotation", 1, 0.5 + 0.8 * 0.25, 0.5 + 0.8 * 0.125)
        assert av.value == 0.5 + 0.8 * 0.375                                 # ... and was not moved
