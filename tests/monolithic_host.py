"""The linear algebra of the monolithic BDF step (csrc/api.hip: nsfem_ctx::MixedOp, nsfem_ctx::BlockPrec) restated on
the host.  A plain helper module like mg_cycle_host.py, which it imports: nothing here comes from the device; the
matrices are the oracle's (`fem_oracle.Space`: mass_p2, stiffness_p2, divergence, convection_jacobian,
picard_convection), the three inner cycles are `mg_cycle_host.Hierarchy.schur`, `.mass_smoother`, `.velocity`.

mixed_matrix          A = [[J, -c_p D^T], [-c_p D, 0]] with J = (alpha0 / k) M + c_v K + c_c C'(u) (Newton:
                      convection_jacobian; Picard: picard_convection), and identity rows exactly as MixedOp::apply
                      leaves them:
                        rule M1  velocity Dirichlet rows are rows of the identity (J with MASK_IDENTITY);
                        rule M2  -c_p D^T p is NOT added on those rows;
                        rule M3  pressure Dirichlet rows are rows of the identity (launch_copy_at after -c_p D u);
                        rule M4  the off-diagonal blocks carry -c_p, both of them.
BlockPreconditioner   z = BlockPrec r, upper block-triangular with the Cahouet-Chabard Schur approximation:
                        rule B1  a = alpha0 / k + prec_shift (the shift enters the Schur part AND the velocity cycle);
                        rule B2  z_p = -(1 / c_p^2) (a S r_p + c_v Q r_p), S = one mg_s cycle (A_p^+), Q = the mass
                                 smoother (M_p^-1): a goes with S, c_v with Q;
                        rule B3  z_p = r_p on the pressure Dirichlet dofs (the set of the SYSTEM, not PRESSURE_PRECOND);
                        rule B4  z_u = F (r_u + c_p D^T z_p), + c_p, D^T not added on velocity Dirichlet rows, F = one
                                 default velocity cycle on a M + c_v K (identity rows: z_u = r_u on Dirichlet dofs);
                        rule B5  S is built on the PRESSURE_PRECOND set, with the singular flag of mg_refresh_schur /
                                 attach_schur_laplacian;
                        rule B6  Q is four steps with ratio 8.
                      `exact=True` replaces S, Q, F by exact solves (pseudo-inverse of the flagged / singular
                      Laplacian, M_p^-1, F^-1 with identity rows): the ideal preconditioner whose spectrum
                      tests/test_monolithic_host.py bounds.

Which host test fails when one rule is reverted (tests/test_monolithic_host.py, each by a `revert=` switch of this
module that the test flips): M1, M2, M3, M4 -- test_mixed_matrix_equals_the_oracle_jacobian_with_dirichlet_rows;
B1 .. B6 -- test_reverting_a_rule_of_the_block_preconditioner_is_noticed (B2, B4 also move the spectrum out of the
bound of test_ideal_preconditioner_puts_the_spectrum_where_cahouet_chabard_puts_it).

Precision: float64 and numpy.longdouble as in mg_cycle_host; `rel` of the two sets the device tolerance
(tests/test_gpu_monolithic_linear.py).

Out of scope: partitioned contexts, traction-form viscosity, rotating frames."""
import numpy as np
import scipy.sparse as sp

import krylov_host as kh
import mg_cycle_host as mh
from mg_cycle_host import LD, rel  # noqa: F401

FORMS = ("standard", "rotational", "divergence", "skew_symmetric")        # nsfem_step_opts.convective_form 0 .. 3


def jacobian(H, u, a, cv, cc, form=0, picard=False):
    """J = a M + c_v K + c_c C'(u) on the interleaved velocity space (scipy CSR, float64); cc None / 0: no convection"""
    I = sp.identity(H.dim, format="csr")
    J = a * sp.kron(H.M2, I, format="csr") + cv * sp.kron(H.K2, I, format="csr")
    if cc:
        s = H.space
        C = s.picard_convection(u, FORMS[form]) if picard else s.convection_jacobian(u, FORMS[form])
        J = J + cc * C
    return sp.csr_matrix(J)


def mixed_flags(H, velocity_dirichlet, pressure_dirichlet):
    nv = H.n_p2 * H.dim
    flags = np.zeros(nv + H.n_p1, dtype=bool)
    flags[np.asarray(velocity_dirichlet, dtype=np.int64)] = True
    flags[nv + np.asarray(pressure_dirichlet, dtype=np.int64)] = True
    return flags


def mixed_matrix(H, u, a, cv, cc, cp, velocity_dirichlet, pressure_dirichlet, form=0, picard=False, dtype=np.float64,
                 revert=None):
    """MixedOp as a `mg_cycle_host._Mat` of `dtype` (rules M1 .. M4 of the module docstring)"""
    nv = H.n_p2 * H.dim
    D = H.divergence()
    J = jacobian(H, u, a, cv, cc, form, picard)
    Bt = (cp if revert == "M4" else -cp) * sp.csr_matrix(D.T)
    A = sp.bmat([[J, Bt], [-cp * D, None]], format="csr")
    flags = mixed_flags(H, velocity_dirichlet, [] if revert == "M3" else pressure_dirichlet)
    if revert == "M1":
        flags[:nv] = False
    M = kh.masked(A, flags, "identity", np.float64).A
    if revert == "M2":          # D^T added on the velocity Dirichlet rows
        keep = sp.diags(np.concatenate([mixed_flags(H, velocity_dirichlet, [])[:nv], np.zeros(H.n_p1, bool)]).astype(float))
        M = M + keep @ sp.bmat([[None, Bt], [sp.csr_matrix((H.n_p1, nv)), None]], format="csr")
    M = sp.csr_matrix(M)
    M.sort_indices()
    return mh._Mat(M, dtype)


def residual(H, u, p, u1, u2, alpha, k, cv, cc, cp, velocity_bc, pressure_bc, form=0):
    """bdf_residual: F_u = L u + M (a1 u1 + a2 u2) / k + c_c conv(u) - c_p D^T p, F_p = -c_p D u, Dirichlet rows
    x_i - g_i (no body force, no traction); velocity_bc / pressure_bc: (dofs, values)"""
    s, D = H.space, H.divergence()
    I = sp.identity(H.dim, format="csr")
    M, K = sp.kron(H.M2, I, format="csr"), sp.kron(H.K2, I, format="csr")
    fu = (alpha[0] / k) * (M @ u) + cv * (K @ u) + M @ (alpha[1] * u1 + alpha[2] * u2) / k - cp * (D.T @ p)
    if cc:
        fu = fu + cc * s.convection_residual(u, FORMS[form])
    fp = -cp * (D @ u)
    vd, vv = velocity_bc
    pd, pv = pressure_bc
    vd, pd = np.asarray(vd, dtype=np.int64), np.asarray(pd, dtype=np.int64)
    fu[vd] = u[vd] - vv
    fp[pd] = p[pd] - pv
    return np.concatenate([fu, fp])


class _Exact:
    """exact inner solves in place of the three cycles (dense float64)"""

    def __init__(self, A, flags, identity_rows, singular):
        a = np.array(sp.csr_matrix(A).todense(), dtype=np.float64)
        m = np.asarray(flags, dtype=bool)
        self.m, self.identity_rows = m, identity_rows
        a[m, :] = 0.0
        a[:, m] = 0.0
        a[m, m] = 1.0
        self.inv = np.linalg.pinv(a, hermitian=True) if singular else np.linalg.inv(a)
        self.inv[m, :] = 0.0
        self.inv[:, m] = 0.0

    def apply(self, r):
        z = self.inv @ r
        return np.where(self.m, r, z) if self.identity_rows else z


class BlockPreconditioner:
    """z = BlockPrec r (rules B1 .. B6).  schur_dirichlet: the PRESSURE_PRECOND set; algebraic: level operators of
    `Hierarchy.algebraic_laplacian(velocity_dirichlet)` instead of K"""

    def __init__(self, H, alpha0, k, cv, cp, velocity_dirichlet, pressure_dirichlet, schur_dirichlet, prec_shift=0.0,
                 degree=2, eig_ratio=4.0, coarse_dense_max=1200, algebraic=False, dtype=np.float64, exact=False,
                 revert=None):
        self.H, self.dtype, self.cp, self.cv = H, dtype, dtype(cp), dtype(cv)
        self.nv = H.n_p2 * H.dim
        shift = 0.0 if revert == "B1" else prec_shift
        a, b = mh.operator_coefficients(alpha0, k, cv, prec_shift=prec_shift)
        self.a = dtype(alpha0) / dtype(k) + dtype(shift)
        self.vflags = mixed_flags(H, velocity_dirichlet, [])[:self.nv]
        self.pdofs = np.asarray([] if revert == "B3" else pressure_dirichlet, dtype=np.int64)
        self.Dt = mh._Mat(sp.csr_matrix(H.divergence().T), dtype)
        self.revert = revert
        sdofs = pressure_dirichlet if revert == "B5" else schur_dirichlet
        if exact:
            assert dtype == np.float64
            pf = np.zeros(H.n_p1, dtype=bool)
            pf[np.asarray(sdofs, dtype=np.int64)] = True
            if algebraic:
                ops, singular = H.algebraic_laplacian(velocity_dirichlet)
                Ap = ops[0].A
            else:
                Ap, singular = H.K1[0], len(sdofs) == 0
            self.S = _Exact(Ap, pf, False, singular and not pf.any())
            self.Q = _Exact(H.M1[0], np.zeros(H.n_p1, bool), False, False)
            I = sp.identity(H.dim, format="csr")
            self.F = _Exact(a * sp.kron(H.M2, I) + b * sp.kron(H.K2, I), self.vflags, True, False)
            return
        if algebraic:
            ops, singular = H.algebraic_laplacian(velocity_dirichlet, dtype)
            self.S = H.schur(sdofs, degree, eig_ratio, coarse_dense_max, dtype, operators=ops, singular=singular)
        else:
            self.S = H.schur(sdofs, degree, eig_ratio, coarse_dense_max, dtype)
        self.Q = H.mass_smoother(dtype)
        if revert == "B6":
            self.Q.coarse_steps = 3
        self.F = H.velocity(velocity_dirichlet, a, b, degree, eig_ratio, coarse_dense_max=coarse_dense_max,
                            trunc_ratio=0.0, dtype=dtype)

    def apply(self, r):
        dt = self.dtype
        r = np.asarray(r, dtype=dt)
        ru, rp = r[:self.nv], r[self.nv:]
        ca, cq = (self.cv, self.a) if self.revert == "B2" else (self.a, self.cv)
        zp = (-ca / (self.cp * self.cp)) * self.S.apply(rp) + (-cq / (self.cp * self.cp)) * self.Q.apply(rp)
        zp[self.pdofs] = rp[self.pdofs]
        g = self.Dt.dot(zp)
        sign = -self.cp if self.revert == "B4" else self.cp
        t = np.where(self.vflags, ru, ru + sign * g)
        return np.concatenate([self.F.apply(t), zp])
