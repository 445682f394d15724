"""The host restatement of the Krylov solvers (tests/krylov_host.py) checked on its own, without a GPU: what correct
iterations must satisfy whatever the device does, on matrices small enough for dense algebra -- the oracle's P1
stiffness and P2 mass matrix on a 4 x 4 box and a nonsymmetric a M + b K + convection block of the oracle's Jacobian.

  * CG iterate k minimises the A-norm of the error over x0 + K_k(M^-1 A, M^-1 r0): compared with the dense solution of
    that least-squares problem for k = 1 .. 5 (both CG forms, Jacobi and a dense SSOR preconditioner, zero-row mask
    with boundary values in the start vector).
  * The single-reduction form produces the iterates of the classic form.  In exact arithmetic the two are equal; the
    drift is measured in longdouble (it must be at the level of THAT precision: the identity is algebraic) and the
    float64 drift is held to the longdouble drift scaled by the ratio of the unit round-offs.
  * BiCGStab reaches numpy.linalg.solve; both CGs reach the solution of the mean-projected singular Neumann problem.
  * The restart rule: a right-hand side on identity rows gives alpha = 1, rho = 0 exactly and the restart in iteration
    2; perturbed right-hand sides put rho^2 / (|r|^2 |rhat|^2) on both sides of 1e-16 and the flag has to follow.
  * b = 0 and a start vector that solves the system exactly leave x unchanged and finite.
  * A skew-symmetric operator gives omega = 0 with rho far from 0: the restart that only the omega clause asks for."""
import numpy as np
import pytest
import scipy.sparse as sp

import fem_oracle as fo
import krylov_host as kh
from fem_mesh import FacetMarkers, TaylorHoodDofMap, rectangle_mesh

DTYPES = [np.float64, kh.LD]
EPS = {np.float64: float(np.finfo(np.float64).eps), kh.LD: float(np.finfo(kh.LD).eps)}


@pytest.fixture(scope="module")
def mats():
    mesh = rectangle_mesh((0.0, 0.0), (1.0, 1.0), 4, 4)
    dm = TaylorHoodDofMap(mesh)
    s = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
    marks = FacetMarkers(mesh)
    marks.mark(lambda X: np.ones(X.shape[0], bool), 1)
    marks.mark(lambda X: np.abs(X[:, 0] - 1.0) < 1e-12, 2)
    b2 = np.unique(dm.facet_p2_nodes(np.concatenate([marks.facets_with_id(1), marks.facets_with_id(2)])))
    out1 = np.unique(dm.facet_p1_nodes(marks.facets_with_id(2)))
    X = dm.p2_coords
    u = np.stack([np.sin(np.pi * X[:, 0]) * np.cos(np.pi * X[:, 1]) + 0.5,
                  -np.cos(np.pi * X[:, 0]) * np.sin(np.pi * X[:, 1]) + X[:, 0]], axis=1).ravel()
    J = (1.5 / 0.5) * s.vector_mass() + 0.01 * s.vector_stiffness() + s.convection_jacobian(u)
    flags_v = np.zeros(2 * dm.n_p2, bool)
    flags_v[np.concatenate([2 * b2, 2 * b2 + 1])] = True
    flags_p = np.zeros(dm.n_p1, bool)
    flags_p[out1] = True
    flags_m = np.zeros(dm.n_p2, bool)
    flags_m[b2] = True
    return dict(K1=sp.csr_matrix(s.stiffness_p1()), M2=sp.csr_matrix(s.mass_p2()), J=sp.csr_matrix(J),
                flags_v=flags_v, flags_p=flags_p, flags_m=flags_m)


def _ssor(A, flags):
    """dense inverse of (D + L) D^-1 (D + U) on the unflagged dofs, zero on the flagged ones"""
    a = np.asarray(A.todense(), dtype=kh.LD)
    free = np.nonzero(~flags)[0]
    ar = a[np.ix_(free, free)]
    D = np.diag(np.diag(ar))
    Minv = np.linalg.inv(((D + np.tril(ar, -1)) @ np.diag(1.0 / np.diag(ar)) @ (D + np.triu(ar, 1))).astype(np.float64))
    Minv = 0.5 * (Minv + Minv.T)
    full = np.zeros(a.shape)
    full[np.ix_(free, free)] = Minv
    return full


def _galerkin(A, Minv, b, x0, free, k):
    """argmin ||x - x*||_A over x0 + K_k(M^-1 A, M^-1 r0) on the unflagged dofs (dense, longdouble)"""
    Af = np.asarray(A.todense(), dtype=kh.LD)
    r0 = (np.asarray(b, kh.LD) - Af @ np.asarray(x0, kh.LD))[free]
    Ar, Mr = Af[np.ix_(free, free)], np.asarray(Minv, kh.LD)[np.ix_(free, free)]
    V = np.zeros((free.size, k), dtype=kh.LD)
    v = Mr @ r0
    for j in range(k):                                   # Gram-Schmidt in the A inner product, twice
        for _ in range(2):
            for i in range(j):
                v = v - (V[:, i] @ (Ar @ v)) * V[:, i]
        V[:, j] = v / np.sqrt(v @ (Ar @ v))
        v = Mr @ (Ar @ V[:, j])
    x = np.asarray(x0, kh.LD).copy()
    x[free] += V @ (V.T @ r0)                            # (V^T A V = 1)
    return x


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("which", ["stiffness jacobi", "mass jacobi", "stiffness ssor"])
def test_cg_iterates_minimise_the_energy_norm_of_the_error_over_the_krylov_space(mats, which, dtype):
    K, flags = (mats["M2"], mats["flags_m"]) if which.startswith("mass") else (mats["K1"], mats["flags_p"])
    rng = np.random.default_rng(3)
    n = K.shape[0]
    b = rng.standard_normal(n)
    x0 = np.where(flags, rng.standard_normal(n), 0.3 * rng.standard_normal(n))      # boundary values + a free part
    A = kh.masked(K, flags, "zero", dtype)
    free = np.nonzero(~flags)[0]
    if which.endswith("jacobi"):
        dinv = kh.jacobi(A, flags)
        Minv = np.diag(np.asarray(dinv, np.float64))
        runs = [kh.pcg_jacobi(A, b, x0, dinv, 5, flags=flags),
                kh.pcg_single_reduction(A, b, x0, lambda r: dinv * r, 5, flags=flags)]
    else:
        Minv = _ssor(K, flags)
        Md = Minv.astype(dtype)
        runs = [kh.pcg_single_reduction(A, b, x0, lambda r: Md @ r, 5, flags=flags)]
    for h in runs:
        for k in range(1, 6):
            ref = _galerkin(K, Minv, b, x0, free, k)
            assert np.array_equal(h.x[k][flags], np.asarray(x0, dtype)[flags])       # boundary values stay
            # (five steps of a well conditioned 5 x 5 projected problem: round-off of the working precision
            # times a modest growth factor)
            assert kh.rel(h.x[k] - x0, ref - x0) < 1e5 * EPS[dtype], (which, k)
            assert h.res[k] < h.r0 * 10.0


def _drift(mats, dtype):
    K, flags = mats["K1"], mats["flags_p"]
    rng = np.random.default_rng(5)
    n = K.shape[0]
    b, x0 = rng.standard_normal(n), rng.standard_normal(n)
    A = kh.masked(K, flags, "zero", dtype)
    dinv = kh.jacobi(A, flags)
    a = kh.pcg_jacobi(A, b, x0, dinv, 8, flags=flags)
    c = kh.pcg_single_reduction(A, b, x0, lambda r: dinv * r, 8, flags=flags)
    return max(kh.rel(c.x[k] - x0, a.x[k] - x0) for k in range(1, 9)), \
        max(abs(float(c.res[k] - a.res[k])) / float(a.res[k]) for k in range(1, 9))


def test_single_reduction_cg_gives_the_iterates_of_classic_cg(mats):
    dx_ld, dr_ld = _drift(mats, kh.LD)
    dx_64, dr_64 = _drift(mats, np.float64)
    print("\n[krylov host] drift of the single-reduction form: longdouble x %.1e res %.1e, float64 x %.1e res %.1e"
          % (dx_ld, dr_ld, dx_64, dr_64))
    # the identity is algebraic: in longdouble the drift is round-off of longdouble, far below float64's
    assert dx_ld < 1e4 * EPS[kh.LD] and dr_ld < 1e4 * EPS[kh.LD]
    scale = EPS[np.float64] / EPS[kh.LD]
    assert dx_64 <= 16.0 * scale * max(dx_ld, EPS[kh.LD]) and dr_64 <= 16.0 * scale * max(dr_ld, EPS[kh.LD])


@pytest.mark.parametrize("dtype", DTYPES)
def test_bicgstab_reaches_the_dense_solution_of_the_nonsymmetric_system(mats, dtype):
    J, flags = mats["J"], mats["flags_v"]
    assert abs(J - J.T).max() > 1e-3 * abs(J).max()                      # genuinely nonsymmetric
    rng = np.random.default_rng(7)
    b = rng.standard_normal(J.shape[0])
    A = kh.masked(J, flags, "identity", dtype)
    dinv = kh.jacobi(A, flags)
    h = kh.bicgstab(A, b, np.zeros_like(b), lambda r: dinv * r, 120)
    ref = np.linalg.solve(kh.masked(J, flags, "identity").A.toarray(), b)
    done = [j for j in range(1, 121) if h.res[j] <= 1e-12 * h.bnorm]
    assert done, min(h.res[1:])
    assert kh.rel(h.x[done[0]], ref) < 1e-9
    assert np.array_equal(np.asarray(h.x[done[0]][flags], np.float64), b[flags]) or \
        kh.rel(h.x[done[0]][flags], b[flags]) < 1e-12                    # identity rows: x = b there
    # the recurrence residual is the true one while no cancellation has happened
    true1 = np.asarray(b, dtype) - A.dot(h.x[1])
    assert abs(float(np.sqrt(true1 @ true1) - h.res[1])) < 1e-10 * float(h.r0)


@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("form", ["classic", "single reduction"])
def test_cg_solves_the_mean_projected_singular_neumann_problem(mats, form, dtype):
    K = mats["K1"]
    n = K.shape[0]
    rng = np.random.default_rng(9)
    b = rng.standard_normal(n) + 0.7                                      # not compatible: mean(b) != 0
    x0 = rng.standard_normal(n)
    A = kh.masked(K, None, None, dtype)
    dinv = kh.jacobi(A)
    if form == "classic":
        h = kh.pcg_jacobi(A, b, x0, dinv, 60, project_mean=True)
    else:
        h = kh.pcg_single_reduction(A, b, x0, lambda r: dinv * r, 60, project_mean=True)
    assert abs(float(h.bnorm) - np.linalg.norm(b - b.mean())) < 1e-13 * np.linalg.norm(b)
    done = [j for j in range(1, 61) if h.res[j] <= 1e-11 * h.bnorm]
    assert done, min(h.res[1:])
    ref = np.linalg.lstsq(K.toarray(), b - b.mean(), rcond=None)[0]
    x = np.asarray(h.x[done[0]], np.float64)
    assert kh.rel(x - x.mean(), ref - ref.mean()) < 1e-8


@pytest.mark.parametrize("dtype", DTYPES)
def test_right_hand_side_on_identity_rows_restarts_in_the_second_iteration(mats, dtype):
    J, flags = mats["J"], mats["flags_v"]
    rng = np.random.default_rng(11)
    b = np.where(flags, rng.standard_normal(J.shape[0]), 0.0)
    A = kh.masked(J, flags, "identity", dtype)
    dinv = kh.jacobi(A, flags)
    h = kh.bicgstab(A, b, np.zeros_like(b), lambda r: dinv * r, 3)
    assert h.alpha[1] == 1.0 and h.restart[1] is False
    assert kh.bicgstab(A, b, np.zeros_like(b), lambda r: dinv * r, 1).rho_next == 0.0
    assert h.restart[2] is True and h.restart[3] is False
    assert h.rho[2] == h.res[1] ** 2 or abs(float(h.rho[2] - h.res[1] ** 2)) <= 4 * EPS[dtype] * float(h.rho[2])
    assert h.alpha[2] != 0.0 and h.omega[2] != 0.0 and h.res[2] > 0.0     # the restarted iteration moves on ...
    assert np.array_equal(h.x[2][flags], h.x[1][flags]) and np.abs(h.x[2] - h.x[1])[~flags].max() > 0.0   # off the rows
    assert np.all(np.isfinite(np.asarray(h.x[3], np.float64)))


@pytest.mark.parametrize("dtype", DTYPES)
def test_restart_flag_follows_the_threshold(mats, dtype):
    """b = (identity-row part) + eps (free part): rho = rhat.r after iteration 1 grows with eps; the flag of iteration 2
    has to be rho^2 <= 1e-16 |r|^2 |rhat|^2 evaluated on the sums of iteration 1, on both sides of the threshold"""
    J, flags = mats["J"], mats["flags_v"]
    rng = np.random.default_rng(13)
    bid = np.where(flags, rng.standard_normal(J.shape[0]), 0.0)
    bfree = np.where(flags, 0.0, rng.standard_normal(J.shape[0]))
    A = kh.masked(J, flags, "identity", dtype)
    dinv = kh.jacobi(A, flags)
    seen, ratios = set(), []
    for eps in 10.0 ** np.arange(-13.0, -1.0, 0.5):
        b = bid + eps * bfree
        h1 = kh.bicgstab(A, b, np.zeros_like(b), lambda r: dinv * r, 1)
        h2 = kh.bicgstab(A, b, np.zeros_like(b), lambda r: dinv * r, 2)
        ratio = float(h1.rho_next ** 2 / (h1.res[1] ** 2 * h1.r0 ** 2))
        if abs(np.log10(max(ratio, 1e-300)) + 16.0) < 0.05:
            continue                                                      # (too close to call in float arithmetic)
        ratios.append(ratio)
        assert h1.rho_next != 0.0
        assert h2.restart[2] == (ratio <= 1e-16), (eps, ratio)
        seen.add(h2.restart[2])
    assert seen == {True, False}, ratios
    assert min(ratios) < 1e-19 and any(1e-16 < r < 1e-13 for r in ratios), ratios


@pytest.mark.parametrize("dtype", DTYPES)
def test_zero_right_hand_side_and_exact_start_vector_leave_x_unchanged(mats, dtype):
    rng = np.random.default_rng(15)
    J, fv = mats["J"], mats["flags_v"]
    K, fp = mats["K1"], mats["flags_p"]
    Aj, Ak, An = kh.masked(J, fv, "identity", dtype), kh.masked(K, fp, "zero", dtype), kh.masked(K, None, None, dtype)
    dj, dk, dn = kh.jacobi(Aj, fv), kh.jacobi(Ak, fp), kh.jacobi(An)
    xs = rng.integers(-4, 5, J.shape[0]).astype(dtype)
    xp = rng.integers(-4, 5, K.shape[0]).astype(dtype)
    cases = [(Aj, np.zeros(J.shape[0], dtype), np.zeros(J.shape[0], dtype)), (Aj, Aj.dot(xs), xs)]
    for A, b, x0 in cases:
        h = kh.bicgstab(A, b, x0, lambda r: dj * r, 4)
        assert h.r0 == 0.0
        for k in range(1, 5):
            assert np.array_equal(h.x[k], x0) and h.res[k] == 0.0 and np.isfinite(float(h.alpha[k] + h.omega[k]))
        assert h.restart[2] is True                                       # (omega = 0)
    zero = np.zeros(K.shape[0], dtype)
    # (zero-row mask, exact start: b = A x0 formed by the same product; Neumann: the projection of 0 is 0)
    for A, d, pm, b, x0, fl in ((Ak, dk, False, zero, zero, fp), (Ak, dk, False, Ak.dot(xp) + np.where(fp, 3.0, 0.0), xp, fp),
                                (An, dn, True, zero, zero, None)):
        for h in (kh.pcg_jacobi(A, b, x0, d, 3, pm, fl), kh.pcg_single_reduction(A, b, x0, lambda r: d * r, 3, pm, fl)):
            assert h.r0 == 0.0
            for k in range(1, 4):
                assert np.array_equal(h.x[k], x0) and h.res[k] == 0.0
                assert np.isfinite(float(h.alpha[k])) and np.isfinite(float(h.beta[k]))


@pytest.mark.parametrize("dtype", DTYPES)
def test_skew_symmetric_operator_gives_zero_alpha_and_omega_and_restarts_on_omega(dtype):
    """A = -A^T, M = 1: rhat.v = r.A r = 0 (alpha = 0 by the guard), t.s = s.A s = 0 with t.t > 0 (omega = 0) while
    rho = rhat.r = |r|^2 is as far from 0 as can be -- the restart of iteration 2 is the one the omega = 0 clause asks for"""
    S = sp.csr_matrix(np.array([[0.0, 2.0, 0.0, 0.0], [-2.0, 0.0, 1.0, 0.0], [0.0, -1.0, 0.0, 4.0], [0.0, 0.0, -4.0, 0.0]]))
    A = kh.masked(S, None, None, dtype)
    b = np.array([1.0, 2.0, -1.0, 0.5])
    h = kh.bicgstab(A, b, np.zeros(4), lambda r: r, 2)
    assert h.alpha[1] == 0.0 and h.omega[1] == 0.0 and h.tt[1] > 0.0
    assert np.all(h.x[1] == 0.0) and h.res[1] == h.r0
    assert kh.bicgstab(A, b, np.zeros(4), lambda r: r, 1).rho_next == h.r0 ** 2
    assert h.restart[2] is True and np.all(np.isfinite(np.asarray(h.x[2], np.float64)))
