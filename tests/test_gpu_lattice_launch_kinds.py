"""k_cheb_lattice: the instantiations specialised per launch kind against the runtime-flag kernel.

A launch kind is the set of operands a launch has (x_in, the fused prolongation xc, the fused restriction rf, d_in,
d_out, r_out; no x_in and no xc is a zero start).  The kinds the multigrid cycles and the mass solve launch run
instantiations with these flags fixed at compile time; every other combination runs the runtime-flag kernel.
NSFEM_LATTICE_KINDS=0 (read when a context is created) sends every launch to the runtime-flag kernel.

Both compute every row sum with the same terms in the same order, so each specialised launch must equal the
runtime-flag launch on the same inputs bit for bit: at every tile height the halo admits, with the compile-time
offset stages on and off, nv = 1 and 2, with and without masks and identity rows, on lattices 9 to 1417 nodes
wide.  The launch kind that ran comes back through the test hook."""
import numpy as np
import pytest

from test_gpu_lattice_smoother import TILE_LINES, Lattice, _fits

pytestmark = pytest.mark.gpu

LK_XIN, LK_XC, LK_RF, LK_DIN, LK_DOUT, LK_ROUT, LK_FIXED = 1, 2, 4, 8, 16, 32, 64

# (kind flags, steps, operands): steps at the limit of one launch where the halo allows it
KINDS = [
    (LK_XC, ("xc",)),
    (LK_XIN | LK_XC, ("x", "xc")),
    (LK_RF, ("rf",)),
    (LK_RF | LK_ROUT, ("rf", "res")),
    (0, ()),
    (LK_ROUT, ("res",)),
    (LK_DOUT, ("dout",)),
    (LK_XIN | LK_DIN | LK_DOUT, ("x", "d", "dout")),
    (LK_XIN | LK_DIN, ("x", "d")),
    (LK_XIN | LK_DIN | LK_ROUT, ("x", "d", "res")),
    (LK_XIN, ("x",)),
]


def _steps(L, ops):
    from_zero = "x" not in ops and "xc" not in ops
    with_res = "res" in ops
    s = L.steps_max
    while not L.admissible(s, from_zero, with_res):
        s -= 1
    return s, from_zero, with_res


def _launches(L, rng, cases, nv_list=(1, 2), lines_list=(0,) + TILE_LINES, fixed_list=(-1, 0)):
    """every (kind, nv, mask / ident, tile height, fixed stages) of the list on one lattice: key -> output"""
    out = {}
    for nv in nv_list:
        n = L.n * nv
        x, b, d = (rng.standard_normal(n) for _ in range(3))
        nc = ((L.W + 1) // 2) * ((L.H + 1) // 2) * nv
        nf = (2 * L.W - 1) * (2 * L.H - 1) * nv
        xc, rf = rng.standard_normal(nc), rng.standard_normal(nf)
        mask = (rng.random(n) < 0.07).astype(np.uint8)
        for flags, ops in cases:
            if ("xc" in ops or "rf" in ops) and not L.nested():
                continue
            steps, from_zero, with_res = _steps(L, ops)
            G = L.reach * L.mv(steps, from_zero, with_res)
            for mk, ident in ((None, False), (mask, False), (mask, True)):
                for lines in lines_list:
                    if lines and not _fits(G, lines):
                        continue
                    for fixed in fixed_list:
                        kw = dict(x=x if "x" in ops else None, b=b, d=d if "d" in ops else None,
                                  xc=xc if "xc" in ops else None, rf=rf if "rf" in ops else None, mask=mk,
                                  ident=ident, from_zero=from_zero, with_residual=with_res, tile_lines=lines,
                                  fixed=fixed, want_d="dout" in ops)
                        key = (flags, nv, mk is not None, ident, lines, fixed)
                        out[key] = L.apply(nv, steps, **kw)
    return out


def _compare(L_args, cases, monkeypatch, **kw):
    monkeypatch.setenv("NSFEM_LATTICE_KINDS", "0")
    L = Lattice(*L_args)
    generic = _launches(L, np.random.default_rng(sum(L_args)), cases, **kw)
    L.close()
    monkeypatch.setenv("NSFEM_LATTICE_KINDS", "1")
    L = Lattice(*L_args)
    special = _launches(L, np.random.default_rng(sum(L_args)), cases, **kw)
    L.close()
    assert generic.keys() == special.keys() and generic
    for key, g in generic.items():
        s = special[key]
        assert g["lattice_kind"] == 0, key
        assert s["lattice_kind"] == LK_FIXED | key[0], (key, s["lattice_kind"])
        assert (s["lattice_tile_lines"], s["lattice_tiles"]) == (g["lattice_tile_lines"], g["lattice_tiles"]), key
        for k in ("y", "d", "r"):
            if g[k] is None:
                assert s[k] is None, key
                continue
            if k == "r" and not (key[0] & LK_ROUT):
                continue
            assert np.array_equal(g[k], s[k]), (key, k, np.abs(g[k] - s[k]).max())
    return len(generic)


# (space, nx, ny): P1 9 x 121 (one tile in x), P1 151 x 91 (many tiles), P2 61 x 81, P2 151 x 101
@pytest.mark.parametrize("space,nx,ny", [(1, 8, 120), (1, 150, 90), (0, 30, 40), (0, 75, 50)])
def test_specialised_kinds_equal_runtime_kernel_bitwise(space, nx, ny, monkeypatch):
    n = _compare((space, nx, ny), KINDS, monkeypatch)
    print("\n%d launches compared on space %d, %d x %d cells" % (n, space, nx, ny))


def test_specialised_kinds_on_the_widest_lattice(monkeypatch):
    """P1 1417 x 1417 (2 M nodes: the 48-line tiles of the launcher's own choice), nv = 2, the cycle's kinds"""
    cases = [k for k in KINDS if k[0] in (LK_XC, LK_XIN | LK_XC, LK_RF, LK_RF | LK_ROUT, LK_XIN | LK_DIN | LK_DOUT)]
    _compare((1, 1416, 1416), cases, monkeypatch, nv_list=(2,), lines_list=(0, 24), fixed_list=(-1,))


def test_kinds_without_an_instantiation_run_the_runtime_kernel(monkeypatch):
    """x_in with d_out but no d_in, and xc with d_out, have no specialised instantiation"""
    monkeypatch.setenv("NSFEM_LATTICE_KINDS", "1")
    L = Lattice(1, 40, 30)
    rng = np.random.default_rng(7)
    n = L.n
    x, b = rng.standard_normal(n), rng.standard_normal(n)
    xc = rng.standard_normal(((L.W + 1) // 2) * ((L.H + 1) // 2))
    out = L.apply(1, 3, x=x, b=b)
    assert out["lattice_kind"] == 0
    out = L.apply(1, 3, x=None, xc=xc, b=b)
    assert out["lattice_kind"] == 0
    out = L.apply(1, 3, x=None, xc=xc, b=b, want_d=False)
    assert out["lattice_kind"] == LK_FIXED | LK_XC
    L.close()
