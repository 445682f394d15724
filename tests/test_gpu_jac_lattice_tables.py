"""k_jac_lattice variants against each other and against the launch pair, bit for bit.

Variant 2 (one cell type per wave, node sums by gather, physical gradients from tables: uniform lattices), variant 1
(the same with the geometry of every cell: graded lattices, or NSFEM_JL_UNIFORM_GEO=0) and the round-4 kernel
(NSFEM_JL_KERNEL=0) must produce the Newton and Picard actions and the momentum residual of the launches they replace
(NSFEM_JAC_LATTICE=0) with the same bits, for every convective form, on partial tiles in both directions, around
tile counts just below and above the resident workgroup slots and at full size (the strips of a partitioned
lattice: tests/test_gpu_partition.py).  The gradient tables themselves must equal phys() evaluated per cell."""
import numpy as np
import pytest

import _native as nat
from gpu_common import box, cavity_bc, context

pytestmark = pytest.mark.gpu

FORMS = ((0, "standard"), (1, "rotational"), (2, "divergence"), (3, "skew_symmetric"))
KERNELS = (("pair", {"NSFEM_JAC_LATTICE": "0"}, None),
           ("round4", {"NSFEM_JL_KERNEL": "0"}, 0),
           ("gather", {}, None))


def _graded(nx, ny):
    """binary spacings, 1/32 on the left half of the columns and 1/16 on the right: exact stencil dictionary, but
    the cells of a type do not share their geometry"""
    mesh, dm, marks = box(nx, ny, p1=(nx / 16.0, ny / 16.0))
    x = mesh.coords[:, 0] * 16.0
    h = nx // 2
    mesh.coords[:, 0] = np.where(x <= h, x / 32.0, h / 32.0 + (x - h) / 16.0)
    from fem_mesh import FacetMarkers, TaylorHoodDofMap
    dm = TaylorHoodDofMap(mesh)
    marks = FacetMarkers(mesh)
    xr, yr = mesh.coords[:, 0].max(), mesh.coords[:, 1].max()
    marks.mark(lambda X: np.abs(X[:, 0]) < 1e-12, 1)
    marks.mark(lambda X: np.abs(X[:, 0] - xr) < 1e-12, 2)
    marks.mark(lambda X: np.abs(X[:, 1]) < 1e-12, 3)
    marks.mark(lambda X: np.abs(X[:, 1] - yr) < 1e-12, 4)
    return mesh, dm, marks


def _run(monkeypatch, mesh, dm, marks, form_id, picard, env, seed, residual=True):
    for k in ("NSFEM_JAC_LATTICE", "NSFEM_JL_KERNEL", "NSFEM_JL_UNIFORM_GEO"):
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    bd, bv = cavity_bc(dm, marks)
    rng = np.random.default_rng(seed)
    u, x, u1, u2 = (rng.standard_normal(dm.n_velocity) for _ in range(4))
    ctx = context(mesh, dm)
    try:
        ctx.set_coeffs(0.8, 1.0, 0.02)
        ctx.set_bdf((1.5, -2.0, 0.5), 0.05)
        ctx.set_dirichlet(nat.VELOCITY, bd.astype(np.int32), bv)
        for slot, v in ((nat.U1, u1), (nat.U2, u2), (nat.USTAR, u)):
            ctx.set_state(slot, v)
        ctx.set_convective_form(form_id, picard=picard)
        out = {"action": ctx.operator_apply(nat.OP_MOMENTUM_JAC_MF, x)}
        if residual:
            ctx.assemble(nat.SYS_MOMENTUM, new_step=True)
            out["residual"] = ctx.get_rhs(nat.SYS_MOMENTUM)
        info = ctx.jacobian_info()
        out["tables"] = ctx.jacobian_table_check()
    finally:
        ctx.close()
    return out, info


def _compare(monkeypatch, mesh, dm, marks, form_id, picard, variant, seed, residual=True, kernels=KERNELS):
    res = {}
    for tag, env, want in kernels:
        out, info = _run(monkeypatch, mesh, dm, marks, form_id, picard, env, seed, residual)
        if tag == "pair":
            assert info["path"] == "fused-gather"
        else:
            assert info["path"] == "lattice-kernel"
            assert info["lattice_variant"] == (variant if want is None else want), (tag, info)
        res[tag] = out
    ref = res[kernels[0][0]]
    for tag in res:
        for k in ("action", "residual") if residual else ("action",):
            assert np.array_equal(res[tag][k], ref[k]), (tag, k, np.abs(res[tag][k] - ref[k]).max())
    return res


@pytest.mark.parametrize("form_id,form", FORMS)
@pytest.mark.parametrize("picard", [False, True])
def test_uniform_lattice_every_form_and_linearisation(form_id, form, picard, monkeypatch):
    """partial tiles in both directions (80 x 24 squares: 3 x 4 tiles of 31 x 7, the last ones partly filled)"""
    mesh, dm, marks = box(80, 24, p1=(5.0, 1.5))
    res = _compare(monkeypatch, mesh, dm, marks, form_id, picard, 2, 80 + form_id)
    assert res["gather"]["tables"] == 0


@pytest.mark.parametrize("form_id,form", FORMS)
@pytest.mark.parametrize("picard", [False, True])
def test_graded_lattice_takes_the_per_cell_geometry(form_id, form, picard, monkeypatch):
    mesh, dm, marks = _graded(36, 52)
    res = _compare(monkeypatch, mesh, dm, marks, form_id, picard, 1, 36 + form_id)
    assert res["gather"]["tables"] == -1


def test_uniform_geometry_switch_selects_the_per_cell_variant(monkeypatch):
    mesh, dm, marks = box(40, 40, p1=(2.5, 2.5))
    kernels = (("pair", {"NSFEM_JAC_LATTICE": "0"}, None), ("round4", {"NSFEM_JL_KERNEL": "0"}, 0),
               ("gather", {"NSFEM_JL_UNIFORM_GEO": "0"}, 1), ("tables", {}, 2))
    _compare(monkeypatch, mesh, dm, marks, 2, False, None, 40, kernels=kernels)


@pytest.mark.parametrize("nx,ny", [(480, 216), (480, 224)])
def test_tile_counts_around_the_resident_slots(nx, ny, monkeypatch):
    """16 x 31 = 496 and 16 x 33 = 528 tiles of 32 x 8 squares: just below and above the 512 resident workgroups"""
    mesh, dm, marks = box(nx, ny, p1=(nx / 16.0, ny / 16.0))
    _compare(monkeypatch, mesh, dm, marks, 0, False, 2, nx + ny)


@pytest.mark.parametrize("n", [512, 1024])
def test_full_size_against_the_round4_kernel(n, monkeypatch):
    mesh, dm, marks = box(n, n)
    kernels = KERNELS[1:] if n == 1024 else KERNELS
    res = _compare(monkeypatch, mesh, dm, marks, 0, False, 2, n, kernels=kernels)
    assert res["gather"]["tables"] == 0
