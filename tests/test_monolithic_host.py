"""The host restatement of the monolithic step's linear algebra (tests/monolithic_host.py, the Schur hierarchy and
the mass smoother of tests/mg_cycle_host.py) checked on its own, without a GPU.

  * mixed_matrix equals the Jacobian BDFOracle itself hands to its Newton solver, with apply_dirichlet_rows, entry by
    entry (captured from BDFOracle.step, not rebuilt here); every identity-row rule reverted is noticed.
  * With exact inner solves the preconditioned Stokes operator has its spectrum where Cahouet-Chabard puts it (bound
    and derivation: test_ideal_preconditioner_puts_the_spectrum_where_cahouet_chabard_puts_it).
  * The algebraic Laplacian: the host's own entry-by-entry products equal scipy's D W D^T and P^T A P; it is singular
    exactly when every velocity boundary dof that carries flux (int phi . n != 0) is constrained.
  * krylov_host.bicgstab with the host preconditioner reaches 1e-10 |b| on every case of tests/monolithic_cases.py, in
    the recorded number of iterations (monolithic_cases.HOST_COUNTS: what the device's step is compared with).
  * Reverting any single rule of the restatement fails a named test:
        M1 .. M4 (mixed_matrix)               test_mixed_matrix_equals_the_oracle_jacobian_with_dirichlet_rows
        B1 prec_shift dropped                 test_reverting_a_rule_of_the_block_preconditioner_is_noticed[B1]
        B2 a and c_v swapped                  ...[B2], and the spectrum test (lambda_max >> 1)
        B3 z_p = r_p on pressure rows         ...[B3]
        B4 + c_p D^T z_p                      ...[B4], and the spectrum test (complex / negative eigenvalues)
        B5 mg_s on PRESSURE_PRECOND           ...[B5]
        B6 four mass steps                    ...[B6]
        singular flag of mg_s                 test_schur_cycle_singular_flag_and_dirichlet_set
        ratio 8 of mg_m                       test_mass_smoother_is_four_chebyshev_steps_with_ratio_8"""
import numpy as np
import pytest
import scipy.linalg as sla
import scipy.sparse as sp

import fem_oracle as fo
import krylov_host as kh
import mg_cycle_host as mh
import monolithic_cases as mc
import monolithic_host as mo
from fem_mesh import FacetMarkers, TaylorHoodDofMap, box_mesh, rectangle_mesh
from multigrid import structured_hierarchy


def _small(kind):
    if kind == "8x8":
        mesh = rectangle_mesh((0.0, 0.0), (1.0, 1.0), 8, 8)
        levels = structured_hierarchy((0.0, 0.0), (1.0, 1.0), 8, 8, coarsest=2)
    else:
        mesh = box_mesh((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 2, 2, 2)
        levels = []
    dm = TaylorHoodDofMap(mesh)
    H = mh.Hierarchy(mesh, dm, levels)
    marks = FacetMarkers(mesh)
    marks.mark(lambda X: np.ones(X.shape[0], bool), 1)
    marks.mark(lambda X: np.abs(X[:, 0] - 1.0) < 1e-12, 2)
    wall = np.unique(dm.facet_p2_nodes(marks.facets_with_id(1)))
    side = np.unique(dm.facet_p2_nodes(marks.facets_with_id(2)))
    dofs = lambda nodes: np.sort((H.dim * nodes[:, None] + np.arange(H.dim)[None, :]).ravel())
    outlet = np.unique(dm.facet_p1_nodes(marks.facets_with_id(2)))
    X = dm.p2_coords
    u = np.stack([np.sin(np.pi * X[:, a]) * np.cos(np.pi * X[:, (a + 1) % H.dim]) + 0.3 * a for a in range(H.dim)],
                 axis=1).ravel()
    return dict(H=H, dm=dm, closed=dofs(np.union1d(wall, side)), open=dofs(wall), side=dofs(side), outlet=outlet, u=u)


_smalls = {}


def _cached(kind):
    if kind not in _smalls:
        _smalls[kind] = _small(kind)
    return _smalls[kind]


@pytest.fixture(scope="module", params=["8x8", "2^3"])
def small(request):
    return _cached(request.param)


@pytest.fixture(scope="module")
def box8():
    return _cached("8x8")


# ------------------------------------------------------------------------------------------------ mixed matrix
@pytest.mark.parametrize("kind,form", [("8x8", 0), ("8x8", 1), ("8x8", 2), ("8x8", 3), ("2^3", 0), ("2^3", 3)])
def test_mixed_matrix_equals_the_oracle_jacobian_with_dirichlet_rows(kind, form, monkeypatch):
    """BDFOracle.step hands (residual, jacobian, x, dofs, values) to fem_oracle.newton_solve, which applies
    apply_dirichlet_rows to the Jacobian: both are captured there.  The sign convention is shared: -c_p D^T, -c_p D."""
    small = _cached(kind)
    H = small["H"]
    nv = H.n_p2 * H.dim
    cc, cp, cv, k = 0.7, 1.7, 0.03, 0.05
    vd, pd = small["open"], small["outlet"]
    captured = {}

    def capture(residual, jacobian, x, bc_dofs, bc_vals, *a, **kw):
        captured["A"] = fo.apply_dirichlet_rows(jacobian(x), bc_dofs)
        return x, 0

    monkeypatch.setattr(fo, "newton_solve", capture)
    orc = fo.BDFOracle(H.space, dict(convective_term=cc, pressure_term=cp, viscous_term=cv, body_force_term=None),
                       form=mo.FORMS[form])
    orc.sol[0][:nv] = small["u"]
    bd = np.concatenate([vd, nv + pd])
    orc.step(mc.BDF2, k, (bd, np.zeros(bd.size)))
    ref = sp.csr_matrix(captured["A"])
    args = (H, small["u"], mc.BDF2[0] / k, cv, cc, cp, vd, pd, form)
    A = mo.mixed_matrix(*args).A
    scale = np.abs(ref.data).max()
    assert np.abs((A - ref).data).max(initial=0.0) <= 4e-16 * scale
    for rule in ("M1", "M2", "M3", "M4"):
        wrong = mo.mixed_matrix(*args, revert=rule).A
        assert np.abs((wrong - ref).data).max(initial=0.0) > 1e-3 * scale, rule
    # Picard: the oracle's picard_convection in place of the Newton linearisation; no convection: the Stokes operator
    P = mo.mixed_matrix(*args, picard=True).A
    J = (mc.BDF2[0] / k) * H.space.vector_mass() + cv * H.space.vector_stiffness()
    want = fo.apply_dirichlet_rows(sp.bmat([[J + cc * H.space.picard_convection(small["u"], mo.FORMS[form]),
                                             -cp * orc.D.T], [-cp * orc.D, None]], format="csr"), bd)
    assert np.abs((P - want).data).max(initial=0.0) <= 4e-16 * scale
    assert np.abs((P - ref).data).max() > 1e-3 * scale
    # identity rows: the product returns the input on every Dirichlet dof
    x = np.random.default_rng(form).standard_normal(nv + H.n_p1)
    y = mo.mixed_matrix(*args, dtype=mh.LD).dot(x.astype(mh.LD))
    assert np.array_equal(np.asarray(y[bd], float), x[bd])


# --------------------------------------------------------------------------------------- ideal preconditioner
def _constants(H, vfree, a, cv):
    """beta^2, gamma^2, lambda_K, Lambda of the docstring below, by dense eigen-solves on the free velocity dofs"""
    I = sp.identity(H.dim)
    M = sp.kron(H.M2, I).toarray()[np.ix_(vfree, vfree)]
    K = sp.kron(H.K2, I).toarray()[np.ix_(vfree, vfree)]
    D = H.divergence().toarray()[:, vfree]
    Mp, Ap = H.M1[0].toarray(), H.K1[0].toarray()
    Q = sla.null_space(np.ones((1, H.n_p1)) @ Mp)                        # pressures with zero mean
    red = lambda B: Q.T @ B @ Q
    beta2 = sla.eigh(red(D @ np.linalg.solve(K, D.T)), red(Mp), eigvals_only=True).min()
    gamma2 = sla.eigh(red(D @ np.linalg.solve(M, D.T)), red(Ap), eigvals_only=True).min()
    ev = sla.eigh(K, M, eigvals_only=True)
    return beta2, gamma2, ev.min(), ev.max()


@pytest.mark.parametrize("k,cv", [(0.01, 0.01), (0.5, 0.1), (10.0, 1.0)])
def test_ideal_preconditioner_puts_the_spectrum_where_cahouet_chabard_puts_it(box8, k, cv):
    """Closed cavity, Stokes (c_c = 0), exact inner solves: F^-1 with F = a M + c_v K on the free velocity dofs,
    A_p^+ the pseudo-inverse of the Neumann Laplacian, M_p^-1.  With B = -c_p D_f and X = -(1 / c_p^2) (a A_p^+ +
    c_v M_p^-1) the preconditioner is P^-1 = [[F^-1, -F^-1 B^T X], [0, X]] and

        A P^-1 = [[I, 0], [B F^-1, -B F^-1 B^T X]] ,      -B F^-1 B^T X = S Shat^-1 ,
        S = D_f F^-1 D_f^T ,   Shat^-1 = a A_p^+ + c_v M_p^-1 :

    block triangular, so the spectrum is {1} (the velocity block and every Dirichlet row) together with the spectrum of
    S Shat^-1; c_p has cancelled.  On pressures of zero mean S and Shat are symmetric positive definite, so those
    eigenvalues are real and positive; the constant pressure gives the one eigenvalue 0 of the singular cavity problem.

    Upper bound 1.  <S q, q> = sup_v (q, div v)^2 / (a |v|^2 + c_v |grad v|^2) over the free velocity space V_h in
    H^1_0.  For ANY splitting q = q1 + q2 into continuous piecewise linears, (q, div v) = -(grad q1, v) + (q2, div v)
    <= |grad q1| |v| + |q2| |grad v| (|div v| <= |grad v| on H^1_0) <= (|grad q1|^2 / a + |q2|^2 / c_v)^(1/2)
    (a |v|^2 + c_v |grad v|^2)^(1/2).  The infimum over the splittings of |q1|^2_(A_p / a) + |q2|^2_(M_p / c_v) is the
    parallel sum <(a A_p^+ + c_v M_p^-1)^-1 q, q> = <Shat q, q>.  Hence S <= Shat, lambda <= 1.

    Lower bound.  beta^2 = lambda_min(M_p^-1 D_f K^-1 D_f^T), gamma^2 = lambda_min(A_p^+ D_f M^-1 D_f^T) (the two
    discrete inf-sup constants, zero-mean pressures), lambda_K <= K / M <= Lambda on V_h.  F <= (a / lambda_K + c_v) K
    gives S >= beta^2 / (a / lambda_K + c_v) M_p, and Shat <= M_p / c_v (the splitting q1 = 0): lambda >= beta^2 /
    (1 + a / (c_v lambda_K)).  F <= (a + c_v Lambda) M gives S >= gamma^2 / (a + c_v Lambda) A_p, and Shat <= A_p / a
    (q2 = 0): lambda >= gamma^2 / (1 + c_v Lambda / a).  Asserted: every eigenvalue other than the single 0 lies in
    [max of the two lower bounds, 1] up to 1e-8, with imaginary parts below 1e-8, and at least n_v of them equal 1.
    (The constants are computed from the oracle's matrices on this mesh; the three (k, c_v) put the first, neither
    and the second lower bound in front.)"""
    H, vd = box8["H"], box8["closed"]
    nv, n1 = H.n_p2 * H.dim, H.n_p1
    a, cp = mc.BDF2[0] / k, 1.7
    none = np.zeros(0, dtype=np.int64)

    def spectrum(**kw):
        A = mo.mixed_matrix(H, box8["u"], a, cv, 0.0, cp, vd, none).A.toarray()
        P = mo.BlockPreconditioner(H, mc.BDF2[0], k, cv, cp, vd, none, none, exact=True, **kw)
        Pinv = np.stack([P.apply(e) for e in np.eye(nv + n1)], axis=1)
        return np.linalg.eigvals(A @ Pinv)

    ev = spectrum()
    vfree = np.setdiff1d(np.arange(nv), vd)
    beta2, gamma2, lam_k, lam_max = _constants(H, vfree, a, cv)
    lower = max(beta2 / (1.0 + a / (cv * lam_k)), gamma2 / (1.0 + cv * lam_max / a))
    print("\n[cahouet-chabard] k %g c_v %g: beta^2 %.3f gamma^2 %.3f lower %.4f  spectrum [%.4f, %.4f]"
          % (k, cv, beta2, gamma2, lower, np.sort(ev.real)[1], ev.real.max()))
    assert 0.0 < beta2 <= 1.0 + 1e-10 and 0.0 < gamma2 <= 1.0 + 1e-10
    assert np.abs(ev.imag).max() < 1e-8
    order = np.sort(ev.real)
    assert abs(order[0]) < 1e-8 and order[1] >= lower - 1e-8 and order[-1] <= 1.0 + 1e-8, (order[:3], order[-1], lower)
    assert np.sum(np.abs(ev - 1.0) < 1e-8) >= nv
    # a and c_v swapped / the sign of the D^T term: the spectrum leaves the interval
    swapped = spectrum(revert="B2")
    assert swapped.real.max() > 1.0 + 1e-3 or np.sort(swapped.real)[1] < lower - 1e-3
    flipped = spectrum(revert="B4")
    assert np.abs(flipped.imag).max() > 1e-3 or flipped.real.min() < -1e-3


# ------------------------------------------------------------------------------------------ algebraic Laplacian
def test_algebraic_laplacian_equals_scipy_products_and_is_singular_only_for_a_closed_boundary(small):
    H = small["H"]
    D = H.divergence()
    nv = D.shape[1]

    def scipy_levels(vd):
        w = np.repeat(1.0 / H.M2.diagonal(), H.dim)
        w[vd] = 0.0
        A = sp.csr_matrix(D @ sp.diags(w) @ D.T)
        out = [A]
        for l, t in enumerate(H.transfers):
            P = sp.csr_matrix((t[2], t[1], t[0]), shape=(A.shape[0], H.K1[l + 1].shape[0]))
            A = sp.csr_matrix(P.T @ A @ P)
            out.append(A)
        return out

    for vd, singular in ((small["closed"], True), (small["open"], False)):
        ops, sing = H.algebraic_laplacian(vd)
        opl, singl = H.algebraic_laplacian(vd, mh.LD)
        assert sing is singular and singl is singular
        assert len(ops) == 1 + len(H.transfers)
        for mine, ld, want in zip(ops, opl, scipy_levels(vd)):
            scale = np.abs(want.data).max()
            assert np.abs(mine.toarray() - want.toarray()).max() <= 1e-14 * scale
            assert np.abs(np.asarray(ld.toarray(), float) - want.toarray()).max() <= 1e-14 * scale
            assert np.abs(mine.toarray() - mine.toarray().T).max() <= 1e-14 * scale
    # A_L 1 = D_f W D_f^T 1 and (D^T 1)_j = int div phi_j = int phi_j . n: zero for interior dofs, for tangential
    # components and (3D, P2) for the vertex functions, whose face integral vanishes.  ONE free boundary dof that
    # carries flux is enough to lose the constants; a free dof without flux is not
    ones = np.ones(H.n_p1)
    flux = D.T @ ones
    interior = np.setdiff1d(np.arange(nv), small["closed"])
    assert np.abs(flux[interior]).max() <= 1e-14
    side = small["side"]
    assert np.sum(np.abs(flux[side]) > 1e-6) >= 3 and np.sum(np.abs(flux[side]) <= 1e-14) >= 3
    for free in side:
        ops, sing = H.algebraic_laplacian(np.setdiff1d(small["closed"], [free]))
        assert sing == (abs(flux[free]) <= 1e-14), free
        if not sing:
            assert np.abs(ops[0].dot(ones)).max() > 1e-6 * np.abs(ops[0].diagonal()).max(), free
    # fewer free dofs in the interior: constants stay in the kernel whatever happens inside
    assert H.algebraic_laplacian(np.union1d(small["closed"], interior[::3]))[1] is True


# ---------------------------------------------------------------------------------- the two pressure hierarchies
def test_schur_cycle_singular_flag_and_dirichlet_set(box8):
    """geometric levels: singular <=> the PRESSURE_PRECOND set is empty, flags = that set (z = 0 there); algebraic
    levels keep the flag of the operator whatever the set holds"""
    H, outlet = box8["H"], box8["outlet"]
    none = np.zeros(0, dtype=np.int64)
    r = np.random.default_rng(3).standard_normal(H.n_p1) + 2.0           # (non-zero mean)
    closed = H.schur(none)
    z = closed.apply(r)
    ones = np.ones(closed.A[-1].shape[0])
    assert np.abs(closed.coarse_inv[0] @ ones).max() <= 1e-10 * np.abs(closed.coarse_inv[0]).max()    # pseudo-inverse
    assert np.array_equal(closed.apply(r), H.pressure(none).apply(r))     # K, V(2,2): the Poisson cycle itself
    regular = mh.HostCycle(closed.A, H.transfers, H.nested, closed.flags[0], 1, 2, 2, singular=False)
    assert mh.rel(regular.apply(r), z) > 1e-3                             # a wrong flag is no rounding matter
    pinned = H.schur(outlet)
    assert np.all(pinned.apply(r)[outlet] == 0.0) and mh.rel(pinned.apply(r), z) > 1e-3
    ops, sing = H.algebraic_laplacian(box8["closed"])
    assert sing
    alg = H.schur(none, operators=ops, singular=sing)
    za = alg.apply(r)
    assert np.abs(alg.coarse_inv[0] @ ones).max() <= 1e-10 * np.abs(alg.coarse_inv[0]).max() and mh.rel(za, z) > 1e-3
    # contraction on zero-mean pressures: the cycle approximates the pseudo-inverse of ITS operator
    Q = sla.null_space(np.ones((1, H.n_p1)))
    for cyc in (closed, alg):
        E = Q.T @ (np.eye(H.n_p1) - cyc.matrix() @ cyc.operator().toarray()) @ Q
        assert np.abs(np.linalg.eigvals(E)).max() < 1.0


def test_mass_smoother_is_four_chebyshev_steps_with_ratio_8(box8):
    """against the polynomial written out: z = p(dinv M) dinv r with the degree-3 Chebyshev residual polynomial of
    [1.05 lmax / 8, 1.05 lmax]; three steps or ratio 4 are different vectors"""
    H = box8["H"]
    M = H.M1[0].toarray()
    dinv = 1.0 / np.diag(M)
    lmax = (np.abs(M).sum(axis=1) * dinv).max()
    hi, lo = 1.05 * lmax, 1.05 * lmax / 8.0
    r = np.random.default_rng(5).standard_normal(H.n_p1)
    G = dinv[:, None] * M
    ev = np.linalg.eigvals(G).real
    assert lo < ev.min() and ev.max() <= hi                               # the interval holds the spectrum
    # x_4 = (I - q_4(G)) G^-1 dinv r with q_4 the Chebyshev polynomial of degree 4 scaled to q_4(0) = 1
    theta, delta = 0.5 * (hi + lo), 0.5 * (hi - lo)
    T = [np.eye(H.n_p1), (theta * np.eye(H.n_p1) - G) / delta]
    t = [1.0, theta / delta]
    for _ in range(3):
        T.append(2.0 * T[1] @ T[-1] - T[-2])
        t.append(2.0 * t[1] * t[-1] - t[-2])
    want = np.linalg.solve(G, (np.eye(H.n_p1) - T[4] / t[4]) @ (dinv * r))
    z = H.mass_smoother().apply(r)
    assert mh.rel(z, want) < 1e-12
    assert mh.rel(z, np.linalg.solve(M, r)) < 1.0 / t[4] * 8.0             # ... and it approximates M^-1 r
    three = H.mass_smoother()
    three.coarse_steps = 3
    assert mh.rel(three.apply(r), z) > 1e-4
    four = mh.HostCycle(three.A, [], [], three.flags[0], 1, 0, 0, eig_ratio=4.0, coarse_dense_max=0, coarse_steps=4)
    assert mh.rel(four.apply(r), z) > 1e-4


# ------------------------------------------------------------------------------------ rules of the restatement
RULE_CASE = "box16 developed scaled shifted pinned"        # c_p = 1.7, c_v = 0.03, shift 40, pressure set != Schur set


@pytest.mark.parametrize("rule", ["B1", "B2", "B3", "B4", "B5", "B6"])
def test_reverting_a_rule_of_the_block_preconditioner_is_noticed(rule):
    """on a case where no coefficient is 1 or equal to another and the two pressure sets differ, every reverted rule
    moves z by far more than rounding (the float64 / longdouble difference d of the case is < 1e-14)"""
    ref = mc.reference(RULE_CASE)
    n = ref.pb.dm.n_p2 * ref.pb.dim + ref.pb.dm.n_p1
    r = mc.seeded(RULE_CASE, "r", n)
    z = ref.prec().apply(r)
    d = mh.rel(z, ref.prec(mh.LD).apply(r))
    assert 64.0 * d < 1e-10
    wrong = ref.prec(revert=rule).apply(r)
    assert mh.rel(wrong, z) > 1e-4, (rule, mh.rel(wrong, z))
    # the rows the rules speak about
    nv = ref.pb.dm.n_p2 * ref.pb.dim
    assert np.array_equal(z[nv + ref.pres], r[nv + ref.pres]) and np.array_equal(z[ref.pb.vel[0]], r[ref.pb.vel[0]])


# ------------------------------------------------------------------------------------------------- convergence
@pytest.mark.parametrize("name", sorted(mc.CASES))
def test_host_bicgstab_reaches_1e_10_in_the_recorded_count(name):
    """right-hand side: the Newton residual of the case's state.  The count is what
    tests/test_gpu_monolithic_linear.py holds a full nsfem_step_bdf to (+- 1); the true residual confirms the
    recurrence's claim; 64 d < 1e-10 for the operator and the preconditioner of every case"""
    ref = mc.reference(name)
    count = ref.count()
    h = ref.history(40)
    print("\n[monolithic host] %-40s count %s" % (name, count))
    assert count is not None and count == mc.HOST_COUNTS[name], (name, count)
    A, b = ref.matrix(), ref.rhs()
    true = np.linalg.norm(b - A.dot(h.x[count]))
    assert true <= 1e-9 * float(h.bnorm), (name, true / float(h.bnorm))
    n = b.size
    x, r = mc.seeded(name, "x", n), mc.seeded(name, "r", n)
    assert 64.0 * mh.rel(A.dot(x), ref.matrix(mh.LD).dot(x.astype(mh.LD))) < 1e-10
    assert 64.0 * mh.rel(ref.prec().apply(r), ref.prec(mh.LD).apply(r)) < 1e-10
