"""The host restatement of the multigrid cycles (tests/mg_cycle_host.py) checked on its own, without a GPU: what a
correct V-cycle must satisfy whatever the device does -- symmetry and definiteness of the symmetric cycles,
contraction of every cycle, the pseudo-inverse of the singular coarsest level, the hand-over of row flags through a
non-nested transfer -- on an 8 x 8 box and a 4^3 box."""
import numpy as np
import pytest
import scipy.linalg as sla

import mg_cycle_host as mh
from fem_mesh import FacetMarkers, TaylorHoodDofMap, box_mesh, rectangle_mesh
from multigrid import interpolation_prolongation, structured_hierarchy

A_COEF, B_COEF = 1.5 / 0.05, 0.01            # BDF-2 step 0.05, viscosity 0.01 (full cycles: trunc_ratio = 0)


def _boundary_p2(dm, mesh):
    marks = FacetMarkers(mesh)
    marks.mark(lambda X: np.ones(X.shape[0], bool), 1)
    return np.unique(dm.facet_p2_nodes(marks.facets_with_id(1)))


@pytest.fixture(scope="module", params=["8x8", "4^3"])
def hier(request):
    if request.param == "8x8":
        mesh = rectangle_mesh((0.0, 0.0), (1.0, 1.0), 8, 8)
        levels = structured_hierarchy((0.0, 0.0), (1.0, 1.0), 8, 8, coarsest=2)
    else:
        mesh = box_mesh((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 4, 4, 4)
        levels = structured_hierarchy((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 4, 4, 4, coarsest=2)
    dm = TaylorHoodDofMap(mesh)
    H = mh.Hierarchy(mesh, dm, levels)
    nodes = _boundary_p2(dm, mesh)
    vel = np.sort((H.dim * nodes[:, None] + np.arange(H.dim)[None, :]).ravel())          # no-slip on every side
    outlet = np.nonzero(np.abs(mesh.coords[:, 0] - 1.0) < 1e-12)[0]                      # pressure: the side x = 1
    return H, vel, outlet


def _reduced(cyc, basis):
    """(B^T M B, B^T A B) of the cycle matrix M and the level-0 operator A"""
    M = cyc.matrix()
    A = cyc.operator().toarray()
    return basis.T @ M @ basis, basis.T @ A @ basis


def _unflagged_basis(cyc):
    free = np.nonzero(~cyc.flags[0].ravel())[0]
    B = np.zeros((cyc.flags[0].size, free.size))
    B[free, np.arange(free.size)] = 1.0
    return B


def _symmetric_spectrum(Mq, Aq):
    """eigenvalues of M A for a symmetric positive definite M (the Cholesky factorisation proves it)"""
    assert np.abs(Mq - Mq.T).max() <= 1e-12 * np.abs(Mq).max()
    L = np.linalg.cholesky(0.5 * (Mq + Mq.T))
    return sla.eigvalsh(L.T @ Aq @ L)


def test_pressure_cycle_with_an_outlet_is_symmetric_definite_and_contracts(hier):
    H, _, outlet = hier
    cyc = H.pressure(outlet)
    M = cyc.matrix()
    assert np.all(M[outlet] == 0.0) and np.all(M[:, outlet] == 0.0)      # flagged rows: z = 0, r ignored
    ev = _symmetric_spectrum(*_reduced(cyc, _unflagged_basis(cyc)))
    assert ev.min() > 0.0 and np.abs(1.0 - ev).max() < 1.0, (ev.min(), ev.max())


def test_singular_neumann_pressure_cycle_on_the_mean_free_subspace(hier):
    H, _, _ = hier
    cyc = H.pressure(np.zeros(0, dtype=np.int64))
    n = H.n_p1
    Q = sla.null_space(np.ones((1, n)))                                    # orthonormal basis of the mean-free vectors
    M = cyc.matrix()
    assert np.abs(M - M.T).max() <= 1e-12 * np.abs(M).max()
    ev = _symmetric_spectrum(*_reduced(cyc, Q))
    assert ev.min() > 0.0 and np.abs(1.0 - ev).max() < 1.0, (ev.min(), ev.max())


def test_symmetric_velocity_cycle_is_symmetric_definite_and_contracts(hier):
    H, vel, _ = hier
    cyc = H.velocity(vel, A_COEF, B_COEF, symmetric=True, trunc_ratio=0.0)
    assert not cyc.truncated and cyc.pre == cyc.post == 2
    M = cyc.matrix()
    flagged = cyc.flags[0].ravel()
    assert np.array_equal(M[flagged], np.eye(M.shape[0])[flagged])         # identity rows: z = r
    assert np.all(M[np.ix_(~flagged, flagged)] == 0.0)
    ev = _symmetric_spectrum(*_reduced(cyc, _unflagged_basis(cyc)))
    assert ev.min() > 0.0 and np.abs(1.0 - ev).max() < 1.0, (ev.min(), ev.max())


def test_default_velocity_cycle_contracts(hier):
    """V(0, 3) is not symmetric (BiCGStab does not need it): spectral radius of I - M A on the unflagged rows"""
    H, vel, _ = hier
    cyc = H.velocity(vel, A_COEF, B_COEF, trunc_ratio=0.0)
    assert not cyc.truncated and (cyc.pre, cyc.post) == (0, 3)
    Mq, Aq = _reduced(cyc, _unflagged_basis(cyc))
    assert np.abs(Mq - Mq.T).max() > 1e-8 * np.abs(Mq).max()
    rho = np.abs(np.linalg.eigvals(np.eye(Mq.shape[0]) - Mq @ Aq)).max()
    assert rho < 1.0, rho


def test_truncated_velocity_cycle_solves_the_mass_dominated_level(hier):
    """a small step: level 1 is spectrally a mass matrix, the cycle stops there and still contracts; the step count
    is the one the error bound 2 ((sqrt(kappa) - 1) / (sqrt(kappa) + 1))^steps <= tol asks for"""
    H, vel, _ = hier
    a = 1.5 / 1e-5
    cyc = H.velocity(vel, a, B_COEF, symmetric=True)
    assert cyc.truncated and cyc.active == 2 and len(cyc.flags) == 2
    sk = np.sqrt(float(cyc.ratio[1]))
    q = (sk - 1.0) / (sk + 1.0)
    assert 2.0 * q ** cyc.trunc_steps <= 0.1 and (cyc.trunc_steps == 2 or 2.0 * q ** (cyc.trunc_steps - 1) > 0.1)
    ev = _symmetric_spectrum(*_reduced(cyc, _unflagged_basis(cyc)))
    assert ev.min() > 0.0 and np.abs(1.0 - ev).max() < 1.0, (ev.min(), ev.max())
    assert not H.velocity(vel, a, B_COEF, trunc_ratio=0.0).truncated


def test_regularised_coarse_inverse_is_the_pseudo_inverse(hier):
    H, _, _ = hier
    for dtype in (np.float64, mh.LD):
        cyc = H.pressure(np.zeros(0, dtype=np.int64), dtype=dtype)
        Ac = H.K1[-1].toarray()
        n = Ac.shape[0]
        assert np.abs(Ac @ np.ones(n)).max() < 1e-12                        # singular: constants
        rng = np.random.default_rng(n)
        v = rng.standard_normal((n, 4))
        v -= v.mean(axis=0)
        got = np.asarray(cyc.coarse_inv[0] @ v.astype(dtype), dtype=np.float64)
        want = np.linalg.pinv(Ac) @ v
        assert mh.rel(got, want) < 1e-12
        assert np.abs(got.mean(axis=0)).max() < 1e-13 * np.abs(got).max()
    # a flagged level is inverted as it is, flagged rows and columns act as zero
    cyc = H.pressure(hier[2])
    m = cyc.flags[-1][:, 0]
    assert m.any()
    inv = cyc.coarse_inv[0]
    assert np.all(inv[m] == 0.0) and np.all(inv[:, m] == 0.0)
    Ac = H.K1[-1].toarray()
    assert np.abs(inv[np.ix_(~m, ~m)] @ Ac[np.ix_(~m, ~m)] - np.eye((~m).sum())).max() < 1e-12


def test_longdouble_cycle_agrees_with_the_float64_cycle(hier):
    """the two evaluations that set the tolerance of the device comparison differ by rounding only; the longdouble
    products on CSR rows (large levels) equal the dense ones"""
    assert np.finfo(mh.LD).eps < 1e-18
    H, vel, outlet = hier
    rng = np.random.default_rng(5)
    for make, n in ((lambda dt: H.pressure(outlet, dtype=dt), H.n_p1),
                    (lambda dt: H.pressure(np.zeros(0, dtype=np.int64), dtype=dt), H.n_p1),
                    (lambda dt: H.velocity(vel, A_COEF, B_COEF, trunc_ratio=0.0, dtype=dt), H.n_p2 * H.dim),
                    (lambda dt: H.velocity(vel, A_COEF, B_COEF, symmetric=True, dtype=dt), H.n_p2 * H.dim)):
        r = rng.standard_normal(n)
        z64, zld = make(np.float64).apply(r), make(mh.LD).apply(r)
        assert mh.rel(z64, zld) < 1e-13
        old = mh.DENSE_LD_MAX
        try:
            mh.DENSE_LD_MAX = 0
            zrows = make(mh.LD).apply(r)
        finally:
            mh.DENSE_LD_MAX = old
        assert mh.rel(zrows, zld) < 1e-17


def test_row_flags_through_the_non_nested_transfer_5_to_3():
    """interpolation_prolongation(5, 5, 3, 3): fine vertices i = 0 .. 5 lie at 3 i / 5 = 0, 0.6, 1.2, 1.8, 2.4, 3 in
    coarse cell units.  Along one axis the coarse hat J weighs them
        J = 0: 1, 0.4          J = 1: 0.6 (i = 1), 0.8 (i = 2), 0.2          J = 2: 0.2, 0.8 (i = 3), 0.6 (i = 4)
        J = 3: 0.4, 1 (i = 5),
    so its representative is i = 0, 2, 3, 5.  In the right-diagonal triangles the weight of coarse node (Jx, Jy) at
    fine (ix, iy) with local coordinates (s, t) is 1 - max(s, t) at the cell's first vertex, min(s, t) at its
    last and |s - t| at the vertex between: at (rep(Jx), rep(Jy)) that is 0.8 or 1 in every one of the 16 cases
    except the two off-diagonal interior nodes (1, 2) and (2, 1), where it is |0.8 - 0.2| = 0.6 -- still the largest
    (the rival (2, 4) resp. (4, 2) has 1 - 0.4 = 0.6 and comes later).  Boundary nodes stay on their boundary line."""
    rep1 = [0, 2, 3, 5]
    t = interpolation_prolongation(5, 5, 3, 3)
    inj = mh.representatives(t, 16, nested=False)
    want = np.array([rep1[Jy] * 6 + rep1[Jx] for Jy in range(4) for Jx in range(4)])
    assert np.array_equal(inj, want)
    assert np.array_equal(mh.representatives(t, 16, nested=None), want)     # decided from the values: not nested
    # flags of the fine boundary reach exactly the coarse boundary
    ix, iy = np.arange(36) % 6, np.arange(36) // 6
    fine = (ix == 0) | (ix == 5) | (iy == 0) | (iy == 5)
    Jx, Jy = np.arange(16) % 4, np.arange(16) // 4
    assert np.array_equal(fine[inj], (Jx == 0) | (Jx == 3) | (Jy == 0) | (Jy == 3))
    # no fine node with weight >= 1/2: the coarse node is unflagged; ties: the first fine row
    rowptr, col, val = np.array([0, 2, 4, 5]), np.array([0, 1, 0, 1, 1]), np.array([0.6, 0.4, 0.6, 0.4, 0.2])
    assert np.array_equal(mh.representatives((rowptr, col, val), 2, nested=False), [0, -1])
    # nested transfers: the coinciding node, whatever the weights of the others
    from multigrid import structured_prolongation
    inj = mh.representatives(structured_prolongation(4, 4), 9)
    assert np.array_equal(inj, [2 * (j // 3) * 5 + 2 * (j % 3) for j in range(9)])


def test_p2_from_p1_is_linear_interpolation_at_the_p2_nodes():
    mesh = rectangle_mesh((0.0, 0.0), (2.0, 1.0), 3, 2)
    dm = TaylorHoodDofMap(mesh)
    rp, col, val = mh.p2_from_p1(dm.p2_dofmap, dm.p1_dofmap)
    import scipy.sparse as sp
    P = sp.csr_matrix((val, col, rp), shape=(dm.n_p2, dm.n_p1))
    f = lambda X: 0.3 + 1.7 * X[:, 0] - 0.9 * X[:, 1]
    assert np.abs(P @ f(dm.p1_coords) - f(dm.p2_coords)).max() < 1e-14
    inj = mh.representatives((rp, col, val), dm.n_p1, nested=True)
    assert np.abs(dm.p2_coords[inj] - dm.p1_coords).max() == 0.0
