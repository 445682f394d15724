"""The multigrid V-cycles of csrc/multigrid.hip restated on the host (numpy / scipy), as ONE definition that every
launch path of the device has to reproduce.  A plain helper module like gpu_common.py: it uses nothing from the
device; everything is built from the oracle's matrices (`fem_oracle.Space`: stiffness_p1, mass_p1, stiffness_p2,
mass_p2) on the fine mesh and on every coarse mesh of `multigrid.structured_hierarchy` / `mesh.mg_levels`, from the
prolongation triplets those functions return, and from the P2 <- P1 transfer as nsfem_mg_finalize defines it
(identity at vertices, 1/2 + 1/2 at edge midpoints).

The cycle (header comment and code of csrc/multigrid.hip; `Hierarchy.pressure` / `Hierarchy.velocity` say which
numbers the C ABI puts in):

levels      pressure: P1 fine -> coarse P1 levels, operator K.  Velocity: P2 fine -> P1 fine -> coarse P1 levels,
            operator a M + b K on every level, nv = dim interleaved components; a, b as in ensure_L
            (`operator_coefficients`).
row flags   level 0: the Dirichlet set.  Level l + 1: injection through the representative finer node of each coarse
            node (`representatives`): nested levels -- the finer row of P with the single entry 1; non-nested levels
            -- the finer node with the largest weight if that weight is >= 1/2, else the coarse node is unflagged.
smoother    dinv = 1 / diag (0 on flagged rows), lmax = max_i dinv_i sum_j |a_ij| over unflagged rows (2 when there
            is none), coefficients of Multigrid::cheb_coeffs over [1.05 lmax / ratio, 1.05 lmax]; each step
            d = c1 d + c2 dinv (b - A x), x += d, flagged rows held at 0.  Every smoothing sequence starts its
            recurrence anew.
cycle       `pre` steps from zero; residual with flagged rows zeroed; b_c = R r with the coarse flagged rows zeroed;
            recursion; x += P x_c with flagged rows zeroed; `post` steps; velocity only: z = r on the flagged rows of
            level 0 in the last step (identity rows of the Newton preconditioner).
            R acts on the vector AS IT IS: for pre = 0 that vector is the input itself, INCLUDING its entries on
            flagged fine rows -- the device restricts the caller's vector without masking it, so does this module.
coarsest    dense inverse of the operator with flagged rows / columns eliminated, per component; a singular
            unflagged level: A + (gamma / n) 1 1^T inverted, 1 / (gamma n) 1 1^T removed (gamma = mean diagonal), as
            Multigrid::refresh does; more than `coarse_dense_max` unknowns: `coarse_steps` smoothing steps from zero.
truncated   (velocity, mass-dominated operators) the first P1 level with r = max_i b K_ii / (a M_ii) <= trunc_ratio
            is the last one used and is solved by trunc_steps Chebyshev steps over [0.5 / (1 + r), 1.05 lmax]:
            kappa = 1.05 lmax / (0.5 / (1 + r)), trunc_steps = max(2, ceil(log(2 / tol) / log((sqrt(kappa) + 1) /
            (sqrt(kappa) - 1)))).
shapes      V(2,2) pressure; V(0, degree + 1) default velocity cycle; V(degree, degree) symmetric velocity cycle
            (set_velocity_cycle_symmetric: what CG and the IMEX diffusion step run).
schur       (mg_s, `Hierarchy.schur`) the pressure cycle with a Dirichlet set of its own (PRESSURE_PRECOND) on K, or on
            the algebraic Laplacian A_L = D_f diag(M_v)^-1 D_f^T (D_f: the divergence block without the Dirichlet
            velocity columns) and its Galerkin coarsenings P^T A P (`Hierarchy.algebraic_laplacian`: formed here, entry
            by entry in the precision asked for, from the oracle's divergence(), the diagonal of mass_p2() and the
            prolongation triplets).  singular: geometric levels -- the Dirichlet set is empty; algebraic levels --
            max_i |A_L 1|_i <= 1e-10 max_i |A_L,ii| (attach_schur_laplacian), whatever the Dirichlet set holds.
mass        (mg_m, `Hierarchy.mass_smoother`) one level M_p without flags, never solved: four Chebyshev-Jacobi steps
            from zero over [1.05 lmax / 8, 1.05 lmax].

Precision: every cycle exists in float64 (scipy products) and in numpy.longdouble (dense matrices, or -- levels too
large for that -- the same row sums on the CSR arrays); `rel(z64, zld)` measures what rounding does to one case and
sets the tolerance of the device comparison (tests/test_gpu_multigrid_cycle.py).

Partitioned contexts (strips, slabs): `PartitionedCycle` below -- exact halo mode is the serial cycle, relaxed halo
mode freezes the ghost values inside a smoothing sequence; the replicated global coarse solve and its tail are levels of
the serial hierarchy.  Checked on the host by tests/test_partitioned_cycle_host.py, on the device by
tests/test_gpu_partitioned_cycle.py.  Still out of scope: additive (algebraic Schur) levels, periodic partitions with
wrapped global numbering, the RCB graph partition, Krylov iterates on N ranks."""
import math

import numpy as np
import scipy.sparse as sp

LD = np.longdouble
DENSE_LD_MAX = 1300          # longdouble levels up to this many rows are dense matrices


def rel(a, b):
    a, b = np.asarray(a, dtype=LD), np.asarray(b, dtype=LD)
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), LD(1e-300)))


class _Mat:
    """a sparse matrix with values of one precision and its product with [n, ...] arrays"""

    def __init__(self, A, dtype, data=None):
        A = sp.csr_matrix(A)
        self.shape = A.shape
        self.dtype = dtype
        self.indptr, self.indices = A.indptr.astype(np.int64), A.indices.astype(np.int64)
        self.data = (A.data if data is None else data).astype(dtype)
        if dtype == np.float64:
            self.kind = "scipy"
            self.A = sp.csr_matrix((self.data, A.indices, A.indptr), shape=A.shape)
        elif max(A.shape) <= DENSE_LD_MAX:
            self.kind = "dense"
            self.A = self.toarray()
        else:
            self.kind = "rows"
            self.nonempty = np.nonzero(np.diff(self.indptr) > 0)[0]

    def toarray(self):
        out = np.zeros(self.shape, dtype=self.dtype)
        rows = np.repeat(np.arange(self.shape[0]), np.diff(self.indptr))
        np.add.at(out, (rows, self.indices), self.data)
        return out

    def diagonal(self):
        rows = np.repeat(np.arange(self.shape[0]), np.diff(self.indptr))
        out = np.zeros(self.shape[0], dtype=self.dtype)
        on = rows == self.indices
        np.add.at(out, rows[on], self.data[on])
        return out

    def abs_row_sums(self):
        rows = np.repeat(np.arange(self.shape[0]), np.diff(self.indptr))
        out = np.zeros(self.shape[0], dtype=self.dtype)
        np.add.at(out, rows, np.abs(self.data))
        return out

    def dot(self, X):
        sh = X.shape
        X2 = X.reshape(sh[0], -1)
        if self.kind == "rows":
            Y = np.zeros((self.shape[0], X2.shape[1]), dtype=self.dtype)
            if self.data.size:
                prod = self.data[:, None] * X2[self.indices]
                Y[self.nonempty] = np.add.reduceat(prod, self.indptr[:-1][self.nonempty], axis=0)
        else:
            Y = self.A @ X2
        return Y.reshape((self.shape[0],) + sh[1:])


def combine(a, M, b, K, dtype):
    """a M + b K entry by entry in `dtype` (M, K on one pattern, as the device's scale-and-add); M None: b K"""
    K = sp.csr_matrix(K)
    K.sort_indices()
    if M is None:
        return _Mat(K, dtype, data=dtype(b) * K.data.astype(dtype))
    M = sp.csr_matrix(M)
    M.sort_indices()
    assert np.array_equal(M.indptr, K.indptr) and np.array_equal(M.indices, K.indices)
    return _Mat(K, dtype, data=dtype(a) * M.data.astype(dtype) + dtype(b) * K.data.astype(dtype))


def spgemm(A, B, dtype, a_data=None, b_data=None):
    """A B with every product and every sum in `dtype`: (scipy CSR pattern of the result, its values in `dtype`, in
    the order of the pattern's sorted indices).  a_data / b_data replace the values of A / B (sorted CSR order)"""
    A, B = sp.csr_matrix(A), sp.csr_matrix(B)
    A.sort_indices()
    B.sort_indices()
    av = (A.data if a_data is None else a_data).astype(dtype)
    bv = (B.data if b_data is None else b_data).astype(dtype)
    rows = np.repeat(np.arange(A.shape[0], dtype=np.int64), np.diff(A.indptr))
    k = A.indices.astype(np.int64)
    cnt = np.diff(B.indptr).astype(np.int64)[k]                   # products per entry of A
    a = np.repeat(np.arange(A.nnz, dtype=np.int64), cnt)
    b = np.repeat(B.indptr[:-1].astype(np.int64)[k], cnt) + (np.arange(cnt.sum()) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    key = rows[a] * B.shape[1] + B.indices.astype(np.int64)[b]
    uniq, inv = np.unique(key, return_inverse=True)
    vals = np.zeros(uniq.size, dtype=dtype)
    np.add.at(vals, inv, av[a] * bv[b])
    r, c = uniq // B.shape[1], uniq % B.shape[1]
    indptr = np.concatenate([[0], np.cumsum(np.bincount(r, minlength=A.shape[0]))])
    pattern = sp.csr_matrix((vals.astype(np.float64), c, indptr), shape=(A.shape[0], B.shape[1]))
    return pattern, vals


def operator_coefficients(alpha0, k, viscous, gamma0=None, prec_shift=0.0):
    """(a, b) of the velocity hierarchy's operator a M + b K (ensure_L): BDF alpha0 / k, c_v; IMEX alpha0 / k,
    gamma0 c_v; stationary problems add the mass shift 1 / tau of the time-step preconditioner to a"""
    return alpha0 / k + prec_shift, (viscous if gamma0 is None else gamma0 * viscous)


def p2_from_p1(p2_dofmap, p1_dofmap):
    """CSR triplets of the P2 <- P1 transfer of nsfem_mg_finalize: identity at vertices, 1/2 + 1/2 at edge
    midpoints (smaller P1 id first); local P2 order: vertices, then the UFC edges"""
    p2, p1 = np.asarray(p2_dofmap, dtype=np.int64), np.asarray(p1_dofmap, dtype=np.int64)
    nl1 = p1.shape[1]
    ends = {3: [(1, 2), (0, 2), (0, 1)], 4: [(2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1)]}[nl1]
    n2 = int(p2.max()) + 1
    a, b = np.full(n2, -1, dtype=np.int64), np.full(n2, -1, dtype=np.int64)
    for e, (e0, e1) in enumerate(ends):
        a[p2[:, nl1 + e]] = np.minimum(p1[:, e0], p1[:, e1])
        b[p2[:, nl1 + e]] = np.maximum(p1[:, e0], p1[:, e1])
    for v in range(nl1):
        a[p2[:, v]] = p1[:, v]
        b[p2[:, v]] = -1
    assert (a >= 0).all()
    two = (b >= 0) & (b != a)
    rowptr = np.concatenate([[0], np.cumsum(np.where(two, 2, 1))]).astype(np.int32)
    col = np.empty(rowptr[-1], dtype=np.int32)
    val = np.empty(rowptr[-1])
    col[rowptr[:-1]] = a
    val[rowptr[:-1]] = np.where(two, 0.5, 1.0)
    col[rowptr[:-1][two] + 1] = b[two]
    val[rowptr[:-1][two] + 1] = 0.5
    return rowptr, col, val


def representatives(triplets, n_coarse, nested=None):
    """the finer node that hands its row flags to each coarse node (-1: none; Transfer::build, h_inj).
    nested None: decided from the values (only 1 and 1/2 occur <=> nested)"""
    rowptr, col, val = (np.asarray(t) for t in triplets)
    rows = np.repeat(np.arange(rowptr.size - 1), np.diff(rowptr))
    if nested is None:
        nested = bool(np.all((val == 1.0) | (val == 0.5)))
    inj = np.full(n_coarse, -1, dtype=np.int64)
    if nested:
        single = (np.diff(rowptr) == 1)[rows] & (np.abs(val - 1.0) < 1e-14)
        inj[col[single]] = rows[single]               # (one such row per coarse node)
        return inj
    ok = np.nonzero(val >= 0.5)[0]
    # largest weight, the first finer row among equals
    order = ok[np.lexsort((ok, -val[ok], col[ok]))]
    first = np.concatenate([[True], col[order][1:] != col[order][:-1]]) if order.size else np.zeros(0, bool)
    inj[col[order][first]] = rows[order][first]
    return inj


def _inverse(a):
    """dense inverse: LAPACK in float64, Gauss-Jordan with partial pivoting in longdouble"""
    if a.dtype == np.float64:
        return np.linalg.inv(a)
    n = a.shape[0]
    w = np.concatenate([a.copy(), np.eye(n, dtype=a.dtype)], axis=1)
    for c in range(n):
        p = c + int(np.argmax(np.abs(w[c:, c])))
        if p != c:
            w[[c, p]] = w[[p, c]]
        w[c] /= w[c, c]
        f = w[:, c].copy()
        f[c] = 0.0
        w -= f[:, None] * w[c][None, :]
    return w[:, n:]


class HostCycle:
    """one hierarchy: `ops` the level operators (_Mat, scalar), `transfers` the prolongation triplets level l + 1 ->
    level l, `nested` one entry per transfer (True / False / None: from the values), `flags0` [n0, nv] bool"""

    def __init__(self, ops, transfers, nested, flags0, nv, pre, post, eig_ratio=4.0, singular=False,
                 coarse_dense_max=1200, coarse_steps=30, identity_rows=False, truncation=None, dtype=np.float64):
        self.dtype, self.nv, self.pre, self.post = dtype, nv, pre, post
        self.eig_ratio, self.identity_rows, self.coarse_steps = eig_ratio, identity_rows, coarse_steps
        self.A = list(ops)
        self.n_levels = len(self.A)
        self.active = self.n_levels
        if truncation is not None and 0 < truncation[0] < self.n_levels:
            self.active = truncation[0]
        self.truncated = self.active < self.n_levels
        self.P, self.R, self.inj = [], [], []
        for l, t in enumerate(transfers):
            nf, nc = self.A[l].shape[0], self.A[l + 1].shape[0]
            P = sp.csr_matrix((t[2], t[1], t[0]), shape=(nf, nc))
            self.P.append(_Mat(P, dtype))
            self.R.append(_Mat(P.T.tocsr(), dtype))
            self.inj.append(representatives(t, nc, nested[l]))
        # row flags down the levels, smoother data
        self.flags, self.dinv, self.lmax, self.ratio = [], [], [], []
        cur = np.asarray(flags0, dtype=bool).reshape(self.A[0].shape[0], nv)
        for l in range(self.active):
            A = self.A[l]
            cur = self.level_flags(l, cur)
            self.flags.append(cur)
            dinv = np.where(cur, dtype(0.0), (dtype(1.0) / A.diagonal())[:, None])
            gersh = (A.abs_row_sums()[:, None] * dinv)[~cur]
            lmax = gersh.max() if gersh.size else dtype(0.0)
            self.dinv.append(dinv)
            self.lmax.append(lmax if lmax > 0.0 else dtype(2.0))
            self.ratio.append(dtype(eig_ratio))
            if l + 1 < self.active:
                inj = self.inj[l]
                cur = np.where((inj >= 0)[:, None], cur[np.maximum(inj, 0)], False)
        self.trunc_steps = 0
        self.coarse_inv = None
        if self.truncated:
            lmin, tol = dtype(truncation[1]), truncation[2]
            kappa = max(dtype(1.05) * self.lmax[-1] / lmin, dtype(1.0 + 1e-9))
            self.ratio[-1] = kappa
            sk = math.sqrt(float(kappa))
            self.trunc_steps = max(2, int(math.ceil(math.log(2.0 / tol) / math.log((sk + 1.0) / (sk - 1.0)))))
        elif self.A[-1].shape[0] <= coarse_dense_max:
            self.coarse_inv = [self._coarse_inverse(c, singular) for c in range(nv)]

    def level_flags(self, l, flags):
        """the row flags of level l as injection hands them down (PartitionedCycle: the global coarse mask)"""
        return flags

    def _coarse_inverse(self, c, singular):
        dtype = self.dtype
        a = self.A[-1].toarray()
        m = self.flags[-1][:, c]
        n = a.shape[0]
        a[m, :] = 0.0
        a[:, m] = 0.0
        a[m, m] = 1.0
        sing = singular and not m.any()
        if sing:
            gamma = a.diagonal().sum() / dtype(n)
            a = a + gamma / dtype(n)
        a = _inverse(a)
        if sing:
            a = a - dtype(1.0) / (gamma * dtype(n))
        a[m, :] = 0.0
        a[:, m] = 0.0
        return a

    def cheb(self, l, k, rho_prev, lmax=None):
        dtype = self.dtype
        b = dtype(1.05) * (self.lmax[l] if lmax is None else lmax)
        a = b / self.ratio[l]
        theta, delta = dtype(0.5) * (b + a), dtype(0.5) * (b - a)
        sigma = theta / delta
        if k == 0:
            return dtype(0.0), dtype(1.0) / theta, dtype(1.0) / sigma
        rho = dtype(1.0) / (dtype(2.0) * sigma - rho_prev)
        return rho * rho_prev, dtype(2.0) * rho / delta, rho

    def smooth(self, l, b, x, steps, ident=False):
        """`steps` Chebyshev steps on level l from x (None: zero); vectors are [n, nv, m]"""
        m = self.flags[l][:, :, None]
        dinv = self.dinv[l][:, :, None]
        d = np.zeros_like(b)
        rho = self.dtype(0.0)
        for k in range(steps):
            c1, c2, rho = self.cheb(l, k, rho)
            res = b if x is None else b - self.A[l].dot(x)
            d = np.where(m, self.dtype(0.0), c1 * d + c2 * dinv * res)
            x = d if x is None else np.where(m, self.dtype(0.0), x + d)
            if ident and k == steps - 1:
                x = np.where(m, b, x)
        return x

    def cycle(self, l, b):
        if self.truncated and l + 1 == self.active:
            return self.smooth(l, b, None, self.trunc_steps, self.identity_rows and l == 0 and self.trunc_steps >= 2)
        if l + 1 == self.n_levels:
            if self.coarse_inv is None:
                return self.smooth(l, b, None, self.coarse_steps)
            return np.stack([self.coarse_inv[c] @ b[:, c, :] for c in range(self.nv)], axis=1)
        m, mc = self.flags[l][:, :, None], self.flags[l + 1][:, :, None]
        if self.pre > 0:
            x = self.smooth(l, b, None, self.pre)
            r = np.where(m, self.dtype(0.0), b - self.A[l].dot(x))
        else:
            x, r = None, b                             # (the input as it is, flagged rows included)
        bc = np.where(mc, self.dtype(0.0), self.R[l].dot(r))
        px = np.where(m, self.dtype(0.0), self.P[l].dot(self.cycle(l + 1, bc)))
        return self.post_smooth(l, b, x, px)

    def post_smooth(self, l, b, x, px):
        """the `post` steps from x + P x_c (x None: no pre-smoothing, the start vector is P x_c)"""
        x = px if x is None else x + px
        return self.smooth(l, b, x, self.post, self.identity_rows and l == 0)

    def apply(self, r):
        """z = M^-1 r for one vector [n0 nv] or the columns of [n0 nv, m]"""
        r = np.asarray(r, dtype=self.dtype)
        n0 = self.A[0].shape[0]
        b = r.reshape(n0, self.nv, -1)
        return self.cycle(0, b).reshape(r.shape)

    def matrix(self):
        """the cycle as a matrix, column by column (the columns of the identity through `apply`)"""
        n = self.A[0].shape[0] * self.nv
        return self.apply(np.eye(n, dtype=self.dtype))

    def operator(self):
        """scipy matrix of level 0 on the interleaved components"""
        A = self.A[0]
        S = sp.csr_matrix((A.data.astype(np.float64), A.indices, A.indptr), shape=A.shape)
        return sp.kron(S, sp.identity(self.nv), format="csr")


def submatrix(M, rows, cols):
    """the rows `rows` of the _Mat M over the columns `cols` (both global ids; every entry of those rows has to lie in
    `cols`: an owned row of a partition is complete), values untouched, column ids sorted as in M"""
    nnz = M.data.size
    pos = sp.csr_matrix((np.arange(1, nnz + 1, dtype=np.int64), M.indices, M.indptr), shape=M.shape)
    where = np.full(M.shape[1], -1, dtype=np.int64)
    where[cols] = np.arange(len(cols))
    S = pos[rows]
    assert (where[S.indices] >= 0).all(), "an owned row reaches a column that is neither owned nor a ghost"
    S = sp.csr_matrix((S.data, where[S.indices], S.indptr), shape=(len(rows), len(cols)))
    S.sort_indices()
    return _Mat(S, M.dtype, data=M.data[S.data - 1])


RULES = ("refresh_every_step", "zero_ghosts", "no_ghost_correction", "local_lmax", "rank0_coarse_mask")


class PartitionedCycle(HostCycle):
    """The cycle of a partitioned context (strips, slabs: Multigrid::vcycle / smooth with a communicator), stated on
    the GLOBAL matrices of `Hierarchy`.  `ranks[l]`, one entry per partitioned level l (finest first; the last one is
    the level that is gathered and solved on the replicated mesh): per rank (O_r, G_r), the global rows it owns and
    the global rows it keeps ghost copies of.  The levels after the last partitioned one are the replicated tail (or
    none: the last partitioned level is the dense coarsest level) -- together the serial hierarchy.

    exact halo mode (relaxed=False)   the serial cycle: every product sees ghosts exchanged just before it.
    relaxed halo mode                 a smoothing sequence of s steps on a partitioned level other than the last, from
        x or from zero, is run by every rank on its own: y = x[O_r u G_r] (zeros from zero), d = 0; per step and owned
        unflagged row i: res_i = b_i - sum_{j in O_r u G_r} A_ij y_j, d_i = c1_k d_i + c2_k dinv_i res_i, y_i += d_i;
        ghost rows of y never change; x[O_r] = y[O_r].  Coefficients from the global lmax (Multigrid::refresh
        all-reduces the maximum, and every owned row is complete, so that is the serial number).  Everything else is
        the serial algorithm on global vectors: the residual after pre-smoothing sees exact ghosts (halo_fill before
        launch_residual), restriction and prolongation are serial, post-smoothing starts from x + P x_c with the
        owners' values of x + P x_c on the ghost rows (the `ghost = 2` prolongation), the last partitioned level is
        solved by the replicated hierarchy or the dense (pseudo-)inverse under the union of the ranks' masks.

    `revert`: names out of RULES, each putting one plausible bug in the place of one rule (host tests only):
        refresh_every_step    ghosts exchanged before every step (the exact cycle)
        zero_ghosts           ghost values zero instead of the start vector's
        no_ghost_correction   post-smoothing: ghost rows hold x without the prolongated correction
        local_lmax            every rank smooths with the Gershgorin bound of its own rows
        rank0_coarse_mask     the replicated solve flags the rows that rank 0 owns and flags, not the union"""

    def __init__(self, *args, ranks, relaxed=True, revert=(), **kw):
        assert set(revert) <= set(RULES), revert
        self.ranks, self.relaxed, self.revert = ranks, relaxed, tuple(revert)
        self.n_part = len(ranks)
        super().__init__(*args, **kw)
        assert self.n_part <= self.active
        self.local, self.local_lmax = [], []
        for l in range(self.n_part - 1):
            A, n = self.A[l], self.A[l].shape[0]
            own = np.concatenate([O for O, _ in ranks[l]])
            assert np.array_equal(np.sort(own), np.arange(n)), "the ranks' owned rows partition the level"
            self.local.append([submatrix(A, O, np.concatenate([O, G])) for O, G in ranks[l]])
            gersh = A.abs_row_sums()[:, None] * self.dinv[l]
            lm = []
            for O, _ in ranks[l]:
                g = gersh[O][~self.flags[l][O]]
                v = g.max() if g.size else self.dtype(0.0)
                lm.append(v if v > 0.0 else self.dtype(2.0))
            self.local_lmax.append(lm)

    def level_flags(self, l, flags):
        if "rank0_coarse_mask" in self.revert and l == self.n_part - 1:
            mine = np.zeros(flags.shape[0], dtype=bool)
            mine[self.ranks[l][0][0]] = True
            return flags & mine[:, None]
        return flags

    def smooth(self, l, b, x, steps, ident=False, ghost_x=None):
        if not self.relaxed or l >= self.n_part - 1 or "refresh_every_step" in self.revert:
            return super().smooth(l, b, x, steps, ident)
        zero = self.dtype(0.0)
        out = np.zeros_like(b)
        for r, (O, G) in enumerate(self.ranks[l]):
            A, no = self.local[l][r], len(O)
            m, dinv, bo = self.flags[l][O][:, :, None], self.dinv[l][O][:, :, None], b[O]
            y = np.zeros((no + len(G),) + b.shape[1:], dtype=self.dtype)
            if x is not None:
                y[:no] = x[O]
                if "zero_ghosts" not in self.revert:
                    y[no:] = (x if ghost_x is None else ghost_x)[G]
            d = np.zeros_like(bo)
            rho = zero
            lmax = self.local_lmax[l][r] if "local_lmax" in self.revert else None
            for k in range(steps):
                c1, c2, rho = self.cheb(l, k, rho, lmax)
                res = bo if x is None and k == 0 else bo - A.dot(y)
                d = np.where(m, zero, c1 * d + c2 * dinv * res)
                y[:no] = d if x is None and k == 0 else np.where(m, zero, y[:no] + d)
                if ident and k == steps - 1:
                    y[:no] = np.where(m, bo, y[:no])
            out[O] = y[:no]
        return out

    def post_smooth(self, l, b, x, px):
        ghost_x = None
        if "no_ghost_correction" in self.revert:
            ghost_x = np.zeros_like(px) if x is None else x
        x = px if x is None else x + px
        return self.smooth(l, b, x, self.post, self.identity_rows and l == 0, ghost_x=ghost_x)


def partition_ranks(parts, velocity):
    """`ranks` of PartitionedCycle from the StripPartition / SlabPartition objects of all ranks: the P1 fine level and
    every local level (global ids: global_p1_offset + local id), for the velocity hierarchy the P2 level first"""
    def split(glob, ghost):
        glob, ghost = np.asarray(glob, dtype=np.int64), np.asarray(ghost) != 0
        return glob[~ghost], glob[ghost]

    levels = [[split(p.p2_global, p.p2_ghost) for p in parts]] if velocity else []
    levels.append([split(p.p1_global, p.p1_ghost) for p in parts])
    for k in range(len(parts[0].levels)):
        levs = [p.levels[k][0] for p in parts]
        levels.append([split(lv.global_p1_offset() + np.arange(lv.n_p1), lv.p1_ghost) for lv in levs])
    return levels


class Hierarchy:
    """the oracle's matrices of one mesh hierarchy, assembled once: fine P2 and P1 spaces, every coarse P1 level
    (`levels`: finest-first [(coarse mesh, prolongation triplets)] of structured_hierarchy / mesh.mg_levels)"""

    def __init__(self, mesh, dm, levels):
        import fem_oracle as fo
        from fem_mesh import TaylorHoodDofMap
        assert np.array_equal(dm.p1_dofmap, mesh.cells), "P1 dofs are the vertices"
        s = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
        self.space = s
        self.dim = s.dim
        self.n_p2, self.n_p1 = dm.n_p2, dm.n_p1
        self.M2, self.K2 = s.mass_p2(), s.stiffness_p2()
        self.M1, self.K1 = [s.mass_p1()], [s.stiffness_p1()]
        self.transfers, self.nested = [], []
        for cm, P in levels:
            cs = fo.Space(cm.coords, cm.cells, TaylorHoodDofMap(cm).p2_dofmap, cm.cells)
            self.M1.append(cs.mass_p1())
            self.K1.append(cs.stiffness_p1())
            self.transfers.append(P)
            self.nested.append(getattr(cm, "nested_in_finer", None))
        self.p2p1 = p2_from_p1(dm.p2_dofmap, dm.p1_dofmap)

    def pressure(self, dirichlet, degree=2, eig_ratio=4.0, coarse_dense_max=1200, dtype=np.float64, make=None):
        """mg_p: V(degree, degree) on K; singular when the Dirichlet set is empty.  make: the cycle class (HostCycle;
        functools.partial(PartitionedCycle, ranks=...) for a partitioned context)"""
        flags = np.zeros((self.n_p1, 1), dtype=bool)
        flags[np.asarray(dirichlet, dtype=np.int64)] = True
        ops = [combine(0.0, None, 1.0, K, dtype) for K in self.K1]
        return (make or HostCycle)(ops, self.transfers, self.nested, flags, 1, degree, degree, eig_ratio,
                                   singular=len(dirichlet) == 0, coarse_dense_max=coarse_dense_max, dtype=dtype)

    def divergence(self):
        if not hasattr(self, "_D"):
            self._D = sp.csr_matrix(self.space.divergence())
            self._D.sort_indices()
        return self._D

    def algebraic_laplacian(self, velocity_dirichlet, dtype=np.float64):
        """(level operators, singular) of the algebraic Schur Laplacian: A_L = D diag(w) D^T with w = 1 / M_v,jj on
        free velocity dofs and 0 on the Dirichlet ones, then P^T A P level by level -- every entry summed in `dtype`"""
        D = self.divergence()
        w = np.repeat(dtype(1.0) / self.M2.diagonal().astype(dtype), self.dim)
        w[np.asarray(velocity_dirichlet, dtype=np.int64)] = dtype(0.0)
        Dt = sp.csr_matrix(D.T)
        Dt.sort_indices()
        pat, vals = spgemm(D, Dt, dtype, a_data=D.data.astype(dtype) * w[D.indices])
        ops = [_Mat(pat, dtype, data=vals)]
        for l, t in enumerate(self.transfers):
            P = sp.csr_matrix((t[2], t[1], t[0]), shape=(pat.shape[0], self.K1[l + 1].shape[0]))
            P.sort_indices()
            Pt = sp.csr_matrix(P.T)
            Pt.sort_indices()
            ap, apv = spgemm(pat, P, dtype, a_data=vals)
            pat, vals = spgemm(Pt, ap, dtype, b_data=apv)
            ops.append(_Mat(pat, dtype, data=vals))
        A0 = ops[0]
        ones = A0.dot(np.ones(A0.shape[0], dtype=dtype))
        singular = bool(float(np.abs(ones).max()) / max(float(np.abs(A0.diagonal()).max()), 1e-300) <= 1e-10)
        return ops, singular

    def schur(self, dirichlet, degree=2, eig_ratio=4.0, coarse_dense_max=1200, dtype=np.float64, operators=None,
              singular=None):
        """mg_s: V(degree, degree) with the flags of the PRESSURE_PRECOND set `dirichlet`, on K (singular when the
        set is empty: mg_refresh_schur) or on the caller's level operators with the caller's singular flag
        (`algebraic_laplacian`: nsfem_mg_set_schur_operator fixes the flag whatever the set holds)"""
        flags = np.zeros((self.n_p1, 1), dtype=bool)
        flags[np.asarray(dirichlet, dtype=np.int64)] = True
        if operators is None:
            operators = [combine(0.0, None, 1.0, K, dtype) for K in self.K1]
            singular = len(dirichlet) == 0
        assert singular is not None and len(operators) == len(self.K1)
        return HostCycle(operators, self.transfers, self.nested, flags, 1, degree, degree, eig_ratio,
                         singular=singular, coarse_dense_max=coarse_dense_max, dtype=dtype)

    def mass_smoother(self, dtype=np.float64):
        """mg_m: one level M_p, no flags, four Chebyshev-Jacobi steps from zero, ratio 8"""
        flags = np.zeros((self.n_p1, 1), dtype=bool)
        return HostCycle([combine(0.0, None, 1.0, self.M1[0], dtype)], [], [], flags, 1, 0, 0, eig_ratio=8.0,
                         singular=False, coarse_dense_max=0, coarse_steps=4, dtype=dtype)

    def truncation(self, a, b, trunc_ratio, trunc_tol):
        """select_velocity_cycle_depth: (levels in use, lower spectral bound, tolerance) or None"""
        n_levels = 2 + len(self.transfers)
        if not (trunc_ratio > 0.0) or not (a > 0.0) or n_levels < 3:
            return None
        for l in range(1, n_levels - 1):
            K, M = self.K1[l - 1].diagonal(), self.M1[l - 1].diagonal()
            r = float((K[M > 0.0] / M[M > 0.0]).max()) * (b / a)
            if r <= trunc_ratio:
                return (l + 1, 0.5 / (1.0 + r), trunc_tol)
        return None

    def velocity(self, dirichlet, a, b, degree=2, eig_ratio=4.0, symmetric=False, coarse_dense_max=1200,
                 trunc_ratio=4.0, trunc_tol=0.1, dtype=np.float64, make=None):
        """mg_v on a M + b K: V(0, degree + 1), or V(degree, degree) in symmetric mode; identity rows on level 0;
        `dirichlet`: interleaved velocity dofs; make: as in `pressure`"""
        flags = np.zeros(self.n_p2 * self.dim, dtype=bool)
        flags[np.asarray(dirichlet, dtype=np.int64)] = True
        post = degree + 1
        pre, post = (max(1, post - 1),) * 2 if symmetric else (0, post)
        ops = [combine(a, self.M2, b, self.K2, dtype)] + [combine(a, M, b, K, dtype) for M, K in zip(self.M1, self.K1)]
        return (make or HostCycle)(ops, [self.p2p1] + self.transfers, [True] + self.nested,
                                   flags.reshape(self.n_p2, self.dim), self.dim, pre, post, eig_ratio, singular=False,
                                   coarse_dense_max=coarse_dense_max, identity_rows=True,
                                   truncation=self.truncation(a, b, trunc_ratio, trunc_tol), dtype=dtype)
