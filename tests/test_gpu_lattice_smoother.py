"""k_cheb_lattice pinned to the ORACLE at the launches production makes.

The multi-step lattice smoother is driven through the C ABI test hook nsfem_kernel_apply (family 4) with every
tile height the launcher can pick (16, 24, 32, 48 lines, forced or chosen), the compile-time-offset stages on and
off, up to 7 steps (6 operator applications on P1 lattices), the fused prolongation of a coarse correction (xc),
the fused restriction of a finer residual (rf, returned as b_formed) and the frozen ghost lines of partitioned
strips.  Every result is compared with the same sequence computed in numpy on the oracle's matrices
(`fo.Space(...)`, a M + b K) and with prolongations built on the host by multigrid.structured_prolongation, not
by the kernel.  The standalone restrictions k_restrict_lattice / k_restrict_lattice2 run through
nsfem_lattice_restrict.

Lattices have binary spacing (h = 1/64 unless stated), so the stencil dictionary equals the CSR values bit for bit
and the tolerance is 1e-13 relative; one inexact lattice is held to 2^-36.  Launches that differ only in tile
height or stage path compute the same row sums in the same order: they must agree bitwise."""
import numpy as np
import pytest
import scipy.sparse as sp

import _native as nat
import fem_oracle as fo
from gpu_common import context, rel
from multigrid import structured_prolongation

pytestmark = pytest.mark.gpu

DICT, LATTICE = 3, 4
A_COEF, B_COEF = 1500.0, 0.01          # alpha0 / k M + nu K of a time step
C1 = [0.0, 0.31, 0.22, 0.17, 0.12, 0.09, 0.05]
C2 = [0.72, 0.63, 0.54, 0.45, 0.40, 0.36, 0.30]
TILE_LINES = (16, 24, 32, 48)


class Lattice:
    """rectangle mesh of nx x ny cells of side h (right diagonals) in lattice numbering, the oracle's operator of
    one space on it (space 0: P2, W = 2 nx + 1; space 1: P1, W = nx + 1) and its transfers"""

    def __init__(self, space, nx, ny, h=1.0 / 64):
        from fem_mesh import TaylorHoodDofMap, rectangle_mesh
        p1 = (nx * h, ny * h)
        mesh = rectangle_mesh((0.0, 0.0), p1, nx, ny)
        mesh.structured = ((0.0, 0.0), p1, nx, ny)
        self.mesh, self.dm = mesh, TaylorHoodDofMap(mesh, reorder=True)
        s = fo.Space(mesh.coords, mesh.cells, self.dm.p2_dofmap, self.dm.p1_dofmap)
        self.space, self.reach = space, (2 if space == 0 else 1)
        self.W, self.H = (2 * nx + 1, 2 * ny + 1) if space == 0 else (nx + 1, ny + 1)
        if space == 0:
            self.A = (A_COEF * s.mass_p2() + B_COEF * s.stiffness_p2()).tocsr()
        else:
            self.A = (A_COEF * s.mass_p1() + B_COEF * s.stiffness_p1()).tocsr()
        self.n = self.A.shape[0]
        assert self.n == self.W * self.H
        self.dinv = 1.0 / self.A.diagonal()
        self.mv_max = 3 if self.reach == 2 else 6
        self.steps_max = 4 if self.reach == 2 else 7
        self.ctx = context(mesh, self.dm)

    def nested(self):
        return self.W % 2 == 1 and self.H % 2 == 1

    def P(self):
        """prolongation from the even-even sublattice ((W + 1) / 2 x (H + 1) / 2) to this lattice"""
        rp, col, val = structured_prolongation(self.W - 1, self.H - 1)
        return sp.csr_matrix((val, col, rp), shape=(self.n, ((self.W + 1) // 2) * ((self.H + 1) // 2)))

    def R(self):
        """restriction from the finer lattice (2 W - 1) x (2 H - 1) to this one: P^T of that pair"""
        rp, col, val = structured_prolongation(2 * self.W - 2, 2 * self.H - 2)
        return sp.csr_matrix((val, col, rp), shape=((2 * self.W - 1) * (2 * self.H - 1), self.n)).T.tocsr()

    def mv(self, steps, from_zero, with_res):
        return steps - (1 if from_zero else 0) + (1 if with_res else 0)

    def admissible(self, steps, from_zero, with_res):
        return 1 <= steps <= self.steps_max and self.mv(steps, from_zero, with_res) <= self.mv_max

    def apply(self, nv, steps, **kw):
        kw.setdefault("x", None)
        x = kw.pop("x")
        return self.ctx.kernel_apply(self.space, nv, x, a=A_COEF, b_coef=B_COEF, family=LATTICE, epilogue=3,
                                     steps=steps, c1=C1[:steps], c2=C2[:steps], maskmode=2, **kw)

    def close(self):
        self.ctx.close()


def _geometry(W, H, G, lines):
    """output tile of the launcher for a halo of G nodes and extended tiles of `lines` lines: (TX, TY, tiles)"""
    Ge = (G + 1) & ~1
    tmx, tmy = 64 - 2 * Ge, lines - 2 * Ge
    ncx, ncy = -(-W // tmx), -(-H // tmy)
    TX = min(tmx, (-(-W // ncx) + 1) & ~1)
    TY = min(tmy, (-(-H // ncy) + 1) & ~1)
    return TX, TY, -(-W // TX) * -(-H // TY)


def _fits(G, lines):
    return lines >= 32 or lines - 2 * ((G + 1) & ~1) >= 8


def _natural_lines(W, H, G):
    """the launcher's own choice (default thresholds: 24 lines from 20 000 nodes, 48 from 2 M nodes)"""
    lines = 24 if W * H >= 20000 else 16
    if W * H >= 2000000 and H >= 96:
        lines = 48
    while lines < 32 and not _fits(G, lines):
        lines += 8
    return lines


def _reference(L, nv, steps, x=None, b=None, d=None, mask=None, ident=False, xc=None, rf=None, with_res=False,
               ghost_rows=None, gh_zero=False):
    """the smoothing sequence of one launch in numpy on the oracle's matrix:
    b = R rf (flagged rows 0) when rf is given; start [x +] P xc (flagged rows 0), x, or zero;
    d = c1[k] d + c2[k] D^-1 (b - A x), x += d; flagged rows x = d = 0 (x = b on the last step with ident);
    ghost rows keep their start value through every step (output 0 with gh_zero, d = 0)"""
    n, A = L.n, L.A
    M = np.zeros((n, nv), bool) if mask is None else (mask.reshape(n, nv) == 1)
    B = (L.R() @ rf.reshape(-1, nv)) if rf is not None else b.reshape(n, nv).copy()
    if rf is not None:
        B[M] = 0.0
    zero_start = x is None and xc is None
    if xc is not None:
        X = L.P() @ xc.reshape(-1, nv)
        if x is not None:
            X = x.reshape(n, nv) + X
        X[M] = 0.0
    elif x is not None:
        X = x.reshape(n, nv).copy()
    else:
        X = np.zeros((n, nv))
    D = d.reshape(n, nv).copy() if (d is not None and not zero_start) else np.zeros((n, nv))
    X0 = X.copy()
    gr = np.zeros(n, bool) if ghost_rows is None else ghost_rows
    for k in range(steps):
        D = np.where(M, 0.0, C1[k] * D + C2[k] * L.dinv[:, None] * (B - A @ X))
        X = np.where(M, 0.0, X + D)
        X[gr] = X0[gr]
        if ident and k == steps - 1:
            X = np.where(M & ~gr[:, None], B, X)
    r = np.where(M, 0.0, B - A @ X) if with_res else None
    Y = X.copy()
    if gh_zero:
        Y[gr] = 0.0
    return Y.ravel(), D.ravel(), (None if r is None else r.ravel()), B.ravel()


def _tol(exact):
    return 1e-13 if exact else 2.0 ** -36


def _check(out, ref, tol, key, with_res=False, b_scale=1.0):
    y, dd, r, _ = ref
    assert out["used_family"] == LATTICE, key
    assert rel(out["y"], y) < tol, (key, rel(out["y"], y))
    assert rel(out["d"], dd) < tol, (key, rel(out["d"], dd))
    if with_res:
        assert np.abs(out["r"] - r).max() < max(tol, 1e-12) * b_scale * 30, key


def _same(a, b, key):
    """bitwise equality of two launches that sum the same rows in the same order"""
    for k in ("y", "d", "r"):
        if a[k] is None:
            continue
        diff = np.abs(a[k] - b[k]).max()
        assert np.array_equal(a[k], b[k]), (key, k, diff, rel(a[k], b[k]))


# (space, nx, ny); the kernel runs on lattices of >= 1024 rows and >= 8 columns (smaller levels get no stencil
# dictionary)
SHAPE_CASES = [
    (1, 8, 120),         # P1 9 x 121: the narrowest lattice the kernel takes, one tile in x, taller than wide
    (1, 56, 24),         # P1 57 x 25: just above the 56-node output width of a 4-node halo, wider than tall
    (1, 40, 30),         # P1 41 x 31: one tile at 48 lines
    (1, 150, 90),        # P1 151 x 91: 6 .. 36 tiles, tiles mod 8 = 0, 1, 2, 4, 6, 7
    (0, 18, 15),         # P2 37 x 31: one tile at 48 lines
    (0, 26, 20),         # P2 53 x 41: just above the 52-node output width of a 6-node halo
    (0, 30, 40),         # P2 61 x 81
    (0, 75, 50),         # P2 151 x 101: 9 .. 39 tiles, tiles mod 8 = 1, 2, 3, 4, 5, 7
]


@pytest.mark.parametrize("space,nx,ny", SHAPE_CASES)
def test_every_tile_height_and_stage_path_matches_the_oracle(space, nx, ny):
    """every admissible (steps, zero start, fused residual) at every tile height and with the compile-time-offset
    stages on and off, nv = 1, 2, with and without a zero-row mask and identity rows on the last step; the reported
    geometry is the launcher's formula; all variants of one sequence are bitwise equal"""
    L = Lattice(space, nx, ny)
    rng = np.random.default_rng(100 * nx + ny + space)
    seen = set()
    shape_id = 1 if space == 0 else 2
    for nv in (1, 2):
        n = L.n * nv
        x, b, d = (rng.standard_normal(n) for _ in range(3))
        mask = (rng.random(n) < 0.07).astype(np.uint8)
        for steps in range(1, L.steps_max + 1):
            for from_zero in (False, True):
                for with_res in (False, True):
                    if not L.admissible(steps, from_zero, with_res):
                        continue
                    G = L.reach * L.mv(steps, from_zero, with_res)
                    for mk, ident in ((None, False), (mask, False), (mask, True)):
                        ref = _reference(L, nv, steps, x=None if from_zero else x, b=b, mask=mk, ident=ident,
                                         with_res=with_res)
                        first = None
                        for lines in (0,) + TILE_LINES:
                            for fixed in (-1, 0):
                                key = (nv, steps, from_zero, with_res, mk is not None, ident, lines, fixed)
                                kw = dict(x=x, b=b, mask=mk, ident=ident, from_zero=from_zero,
                                          with_residual=with_res, tile_lines=lines, fixed=fixed)
                                if lines and not _fits(G, lines):
                                    with pytest.raises(nat.NativeError, match="halo too wide"):
                                        L.apply(nv, steps, **kw)
                                    continue
                                out = L.apply(nv, steps, **kw)
                                assert out["dict_exact"] and out["lattice_w"] == L.W, key
                                want = lines if lines else _natural_lines(L.W, L.H, G)
                                assert out["lattice_tile_lines"] == want, key
                                TX, TY, tiles = _geometry(L.W, L.H, G, want)
                                assert (out["lattice_tx"], out["lattice_ty"], out["lattice_tiles"]) == (TX, TY, tiles), key
                                assert out["lattice_fixed_shape"] == (shape_id if fixed else 0), key
                                seen.add((want, tiles, out["lattice_fixed_shape"]))
                                _check(out, ref, _tol(True), key, with_res, np.abs(b).max())
                                if first is None:
                                    first = out
                                else:
                                    _same(out, first, key)
        # carried direction (a later launch of a long sequence): d_in given, c1 != 0 in the first step
        c1, c2 = [0.3, 0.2, 0.1], [0.6, 0.5, 0.4]
        M = (mask.reshape(L.n, nv) == 1)
        X, D = x.reshape(L.n, nv).copy(), d.reshape(L.n, nv).copy()
        for k in range(3):
            D = np.where(M, 0.0, c1[k] * D + c2[k] * L.dinv[:, None] * (b.reshape(L.n, nv) - L.A @ X))
            X = np.where(M, 0.0, X + D)
        for lines in TILE_LINES:
            if not _fits(L.reach * 3, lines):
                continue
            out = L.ctx.kernel_apply(space, nv, x, a=A_COEF, b_coef=B_COEF, family=LATTICE, epilogue=3, steps=3, b=b,
                                     d=d, mask=mask, maskmode=2, c1=c1, c2=c2, tile_lines=lines)
            assert out["lattice_tile_lines"] == lines
            assert rel(out["y"], X.ravel()) < 1e-13 and rel(out["d"], D.ravel()) < 1e-13, (nv, lines)
    print("\ncovered (tile_lines, tiles, fixed_shape) on %d x %d:" % (L.W, L.H), sorted(seen))
    L.close()


def test_inexact_lattice_at_every_tile_height():
    """h = 1/48: the dictionary equals the CSR values only to round-off (2^-36 relative)"""
    L = Lattice(0, 48, 30, h=1.0 / 48)
    rng = np.random.default_rng(48)
    for nv in (1, 2):
        n = L.n * nv
        x, b = rng.standard_normal(n), rng.standard_normal(n)
        mask = (rng.random(n) < 0.07).astype(np.uint8)
        ref = _reference(L, nv, 3, b=b, mask=mask, ident=True, with_res=True)
        for lines in (24, 32, 48):
            out = L.apply(nv, 3, x=x, b=b, mask=mask, ident=True, from_zero=True, with_residual=True, tile_lines=lines)
            assert not out["dict_exact"] and out["lattice_tile_lines"] == lines
            _check(out, ref, _tol(False), (nv, lines))
    L.close()


TRANSFER_CASES = [(1, 8, 120), (1, 150, 90), (0, 18, 15), (0, 30, 40), (0, 75, 50)]


@pytest.mark.parametrize("space,nx,ny", TRANSFER_CASES)
def test_fused_transfers_of_the_cycles_match_the_oracle(space, nx, ny):
    """the launches vcycle_lattice makes: pre-smoothing from zero on b = R rf with the residual, post-smoothing from
    x + P xc, post-smoothing from P xc alone (no pre-smoothing), identity rows on the last step with xc, and on P1
    the truncated cycle's coarse solve (7 steps from zero on R rf, one launch); b_formed = R rf (flagged rows 0)
    equals the oracle, k_restrict_lattice bitwise, and smoothing on it bitwise equals the fused launch"""
    L = Lattice(space, nx, ny)
    assert L.nested()
    rng = np.random.default_rng(7 * nx + ny)
    Wc, Hc = (L.W + 1) // 2, (L.H + 1) // 2
    nfine = (2 * L.W - 1) * (2 * L.H - 1)
    for nv in (1, 2):
        n = L.n * nv
        x, b = rng.standard_normal(n), rng.standard_normal(n)
        xc, rf = rng.standard_normal(Wc * Hc * nv), rng.standard_normal(nfine * nv)
        mask = (rng.random(n) < 0.07).astype(np.uint8)
        pre = min(L.steps_max, L.mv_max)              # longest pre-smoothing with the residual
        post = L.mv_max                               # longest sequence from a given start
        combos = [("pre", pre, dict(rf=rf, from_zero=True, with_residual=True)),
                  ("pre2", 2, dict(rf=rf, from_zero=True, with_residual=True)),
                  ("post", post, dict(x=x, xc=xc, b=b)),
                  ("post-res", post - 1, dict(x=x, xc=xc, b=b, with_residual=True)),
                  ("post-only", post, dict(xc=xc, b=b)),
                  ("post-ident", 2, dict(x=x, xc=xc, b=b, ident=True)),
                  ("post-only-ident", 2, dict(xc=xc, b=b, ident=True))]
        if space == 1:
            combos.append(("coarse-solve", 7, dict(rf=rf, from_zero=True)))
        for name, steps, kw in combos:
            for mk in (None, mask):
                ref = _reference(L, nv, steps, x=kw.get("x"), b=kw.get("b"), mask=mk, ident=kw.get("ident", False),
                                 xc=kw.get("xc"), rf=kw.get("rf"), with_res=kw.get("with_residual", False))
                first = None
                for lines in (0,) + TILE_LINES:
                    G = L.reach * L.mv(steps, "x" not in kw and "xc" not in kw, kw.get("with_residual", False))
                    if lines and not _fits(G, lines):
                        continue
                    key = (name, nv, mk is not None, lines)
                    out = L.apply(nv, steps, mask=mk, tile_lines=lines, **kw)
                    if lines:
                        assert out["lattice_tile_lines"] == lines, key
                    _check(out, ref, _tol(True), key, kw.get("with_residual", False), np.abs(ref[3]).max())
                    if "rf" in kw:
                        bf = out["b_formed"]
                        assert rel(bf, ref[3]) < 1e-15, (key, rel(bf, ref[3]))
                        if mk is not None:
                            assert np.all(bf[mk == 1] == 0.0), key
                        b1, _ = L.ctx.lattice_restrict(nv, L.W, L.H, rf, mask1=mk)
                        assert np.array_equal(bf, b1), key
                        kw2 = {k: v for k, v in kw.items() if k != "rf"}
                        again = L.apply(nv, steps, mask=mk, tile_lines=lines, b=bf, **kw2)
                        _same(again, out, key + ("b = b_formed",))
                    if first is None:
                        first = out
                    else:
                        _same(out, first, key)
    L.close()


@pytest.mark.parametrize("nv", [1, 2])
@pytest.mark.parametrize("w,h", [(5, 9), (16, 16), (17, 33), (33, 17), (24, 7)])
def test_standalone_restrictions_match_the_transpose_of_the_prolongation(w, h, nv):
    """k_restrict_lattice: b = P^T rf (flagged rows 0); k_restrict_lattice2: b1 = P1^T rf, b2 = P2^T b1 with masks
    on both levels, on coarsest lattices smaller than its 16 x 16 tile, exactly one tile and one node past a
    multiple of 16; equal bitwise to two launches of k_restrict_lattice"""
    from fem_mesh import TaylorHoodDofMap, rectangle_mesh
    mesh = rectangle_mesh((0.0, 0.0), (1.0, 1.0), 2, 2)
    dm = TaylorHoodDofMap(mesh)
    ctx = context(mesh, dm)
    rng = np.random.default_rng(w * 100 + h + nv)
    w1, h1 = 2 * w - 1, 2 * h - 1
    wf, hf = 2 * w1 - 1, 2 * h1 - 1

    def RT(W, H):          # P^T of (W x H) <- ((2 W - 1) x (2 H - 1))
        rp, col, val = structured_prolongation(2 * W - 2, 2 * H - 2)
        return sp.csr_matrix((val, col, rp), shape=((2 * W - 1) * (2 * H - 1), W * H)).T.tocsr()

    rf = rng.standard_normal(wf * hf * nv)
    m1 = (rng.random(w1 * h1 * nv) < 0.1).astype(np.uint8)
    m2 = (rng.random(w * h * nv) < 0.1).astype(np.uint8)
    r1 = np.where(m1.reshape(-1, nv) == 1, 0.0, RT(w1, h1) @ rf.reshape(-1, nv)).ravel()
    r2 = np.where(m2.reshape(-1, nv) == 1, 0.0, RT(w, h) @ r1.reshape(-1, nv)).ravel()
    for masks in ((None, None), (m1, m2)):
        one1, _ = ctx.lattice_restrict(nv, w1, h1, rf, mask1=masks[0])
        one2, _ = ctx.lattice_restrict(nv, w, h, one1, mask1=masks[1])
        b1, b2 = ctx.lattice_restrict(nv, w, h, rf, mask1=masks[0], mask2=masks[1], levels=2)
        want1 = r1 if masks[0] is not None else (RT(w1, h1) @ rf.reshape(-1, nv)).ravel()
        want2 = r2 if masks[0] is not None else (RT(w, h) @ want1.reshape(-1, nv)).ravel()
        assert rel(one1, want1) < 1e-15 and rel(one2, want2) < 1e-15
        assert np.array_equal(b1, one1) and np.array_equal(b2, one2), masks[0] is not None
    ctx.close()


GHOST_CASES = [(1, 40, 60), (0, 20, 30)]


@pytest.mark.parametrize("space,nx,ny", GHOST_CASES)
def test_frozen_ghost_lines_match_the_oracle(space, nx, ny):
    """the first gh_lo and the last gh_hi lattice lines are ghost rows (every component flagged, as the partitioned
    levels do): frozen at x through all steps, read by their neighbours, stored as x (0 with gh_zero), d = 0;
    one step equals the one-step dictionary kernel with ghost = 1"""
    L = Lattice(space, nx, ny)
    rng = np.random.default_rng(11 + space)
    line = np.arange(L.n) // L.W
    for nv in (1, 2):
        n = L.n * nv
        x, b = rng.standard_normal(n), rng.standard_normal(n)
        base = (rng.random(n) < 0.07).astype(np.uint8)
        for lo, hi in ((0, 1), (1, 2), (2, 0), (3, 3)):
            gr = (line < lo) | (line >= L.H - hi)
            mask = base.copy().reshape(L.n, nv)
            mask[gr] = 1
            mask = mask.ravel()
            for steps in range(1, min(4, L.mv_max) + 1):
                for gh_zero in (False, True):
                    for ident in (False, True):
                        ref = _reference(L, nv, steps, x=x, b=b, mask=mask, ident=ident, ghost_rows=gr,
                                         gh_zero=gh_zero)
                        first = None
                        for lines in (0, 48):
                            key = (nv, lo, hi, steps, gh_zero, ident, lines)
                            out = L.apply(nv, steps, x=x, b=b, mask=mask, ident=ident, gh_lo=lo, gh_hi=hi,
                                          gh_zero=gh_zero, tile_lines=lines)
                            _check(out, ref, _tol(True), key)
                            if first is None:
                                first = out
                            else:
                                _same(out, first, key)
            # one step: the dictionary kernel's frozen ghost rows (flag 2, ghost = 1)
            gmask = mask.copy().reshape(L.n, nv)
            gmask[gr] = 2
            one = L.ctx.kernel_apply(space, nv, x, a=A_COEF, b_coef=B_COEF, family=DICT, epilogue=3, steps=1, b=b,
                                     mask=gmask.ravel(), maskmode=2, c1=C1[:1], c2=C2[:1], ghost=1)
            out = L.apply(nv, 1, x=x, b=b, mask=mask, gh_lo=lo, gh_hi=hi)
            assert rel(out["y"], one["y"]) < 1e-14 and rel(out["d"], one["d"]) < 1e-14, (nv, lo, hi)
    L.close()


@pytest.mark.parametrize("n,lines", [(512, 24), (708, 48)])
def test_natural_geometry_at_production_sizes(n, lines):
    """the launcher's own choice on the benchmark's finest P2 level (n = 512: 1025^2 nodes, 24 lines) and on the
    first square size that gets 48 lines (n = 708: 1417^2 = 2.008 M nodes): the two launches of a benchmark cycle,
    3 steps from zero with the residual and 3 steps from x + P xc, velocity (nv = 2)"""
    L = Lattice(0, n, n, h=1.0 / 1024)
    rng = np.random.default_rng(n)
    nv = 2
    N = L.n * nv
    x, b = rng.standard_normal(N), rng.standard_normal(N)
    xc = rng.standard_normal(((L.W + 1) // 2) * ((L.H + 1) // 2) * nv)
    mask = np.zeros(N, np.uint8)
    line, col = np.arange(L.n) // L.W, np.arange(L.n) % L.W
    mask.reshape(L.n, nv)[(line == 0) | (line == L.H - 1) | (col == 0) | (col == L.W - 1)] = 1   # Dirichlet sides
    out = L.apply(nv, 3, x=x, b=b, mask=mask, from_zero=True, with_residual=True)
    assert out["dict_exact"] and out["lattice_tile_lines"] == lines and out["lattice_fixed_shape"] == 1
    _check(out, _reference(L, nv, 3, b=b, mask=mask, with_res=True), _tol(True), "pre", True, np.abs(b).max())
    out = L.apply(nv, 3, x=x, xc=xc, b=b, mask=mask, ident=True)
    assert out["lattice_tile_lines"] == lines
    _check(out, _reference(L, nv, 3, x=x, b=b, mask=mask, ident=True, xc=xc), _tol(True), "post")
    L.close()


def test_refused_launches_raise_instead_of_faulting():
    """ghost lines with a fused transfer, more steps than one launch allows, a tile height the halo does not fit,
    an unknown tile height and a lattice below 1024 rows are refused with NativeError; the context stays usable"""
    small = Lattice(1, 8, 12)
    with pytest.raises(nat.NativeError, match="no lattice structure"):
        small.apply(1, 1, x=np.zeros(small.n), b=np.ones(small.n))
    small.close()
    for space in (0, 1):
        L = Lattice(space, 32, 40)
        rng = np.random.default_rng(3)
        nv = 2
        n = L.n * nv
        x, b = rng.standard_normal(n), rng.standard_normal(n)
        xc = rng.standard_normal(((L.W + 1) // 2) * ((L.H + 1) // 2) * nv)
        rf = rng.standard_normal((2 * L.W - 1) * (2 * L.H - 1) * nv)
        mask = np.zeros(n, np.uint8)
        mask.reshape(L.n, nv)[:L.W] = 1
        with pytest.raises(nat.NativeError, match="ghost"):
            L.apply(nv, 2, x=x, xc=xc, b=b, mask=mask, gh_lo=1)
        with pytest.raises(nat.NativeError, match="ghost"):
            L.apply(nv, 2, rf=rf, from_zero=True, mask=mask, gh_hi=1)
        steps_from_x = L.mv_max
        with pytest.raises(nat.NativeError, match="too many steps"):
            L.apply(nv, steps_from_x + 1, x=x, b=b)
        with pytest.raises(nat.NativeError, match="too many steps"):
            L.apply(nv, steps_from_x, x=x, b=b, with_residual=True)
        with pytest.raises(nat.NativeError, match="too many steps"):
            L.apply(nv, L.steps_max + 1, b=b, from_zero=True)
        with pytest.raises(nat.NativeError, match="halo too wide"):
            L.apply(nv, 3 if space == 0 else 6, x=x, b=b, tile_lines=16)
        with pytest.raises(nat.NativeError, match="tile height"):
            L.apply(nv, 1, x=x, b=b, tile_lines=20)
        ref = _reference(L, nv, 2, x=x, b=b)
        _check(L.apply(nv, 2, x=x, b=b), ref, _tol(True), space)
        L.close()
