"""The two multigrid V-cycles as a whole -- nsfem_mg_apply(0 | 1, r) -- against ONE host definition of the cycle
(tests/mg_cycle_host.py, built from the oracle's matrices) on every launch path: the multi-step lattice kernel with
fused and with explicit transfers, the one-step dictionary kernels, CSR, the runtime-flag lattice kernel; nested and
non-nested levels, 3D, an unstructured refinement hierarchy, dense / device-inverted / smoothed coarsest levels, the
truncated and the symmetric velocity cycle, and the state changes that rebuild masks, operators and cycle depth.

Every case builds a fresh context and asserts through mg_lattice_info / smoother_info that the path it names was
taken: the number of levels on the lattice kernel and whether it was launched at all.  A level gets a stencil
dictionary (and with it the lattice kernel) from 1024 rows on, so on the 16 x 16 box only the P2 level of the
velocity hierarchy (33 x 33 nodes) runs on it and the pressure hierarchy is CSR on every path; the 96 x 40 box
(h = 1/32: P2 193 x 81, P1 97 x 41, 49 x 21, dense 25 x 11) carries three lattice levels and fused transfers in both
hierarchies.  It is also the case that reaches launch_restrict_lattice2: the default velocity cycle has no
pre-smoothing, levels 0, 1, 2 are lattice levels joined by lattice interpolations and level 2 does not form its own
right-hand side (vcycle_lattice: `tl && pre == 0 && ... && !chain_child_forms_b(l + 1)`), so the P2 level forms
b_1 and b_2 in one launch and `restricted_to` carries that to level 1.

Tolerance.  The cycle is a fixed sequence of fp64 operations; how rounding shows in z depends on the case.  Per case
d = rel(z_float64_host, z_longdouble_host) is measured on the reference alone and the device is held to
rel(z_device, z_float64_host) <= max(64 d, 1e-14) (64: the summation orders of the device paths differ from the
host's one), on the 48 x 48 box (h = 1/48, inexact dictionary) plus the dictionary's 2^-38 on the paths that use it.
64 d < 1e-10 is asserted for every case.  Measured d (host only):

    case                               d            case                               d
    box16 pressure neumann             2.1e-16      box48 pressure neumann             4.9e-16
    box16 pressure outlet              1.8e-16      box48 velocity                     1.5e-16
    box16 velocity                     1.5e-16      cube8 pressure neumann             1.9e-16
    box16 velocity shifted             1.6e-16      cube8 velocity                     1.3e-16
    box16 velocity truncated           5.1e-17      dfg pressure outlet                2.8e-14
    box16 velocity symmetric           1.4e-16      dfg velocity                       1.9e-16
    box16 velocity no lid              1.5e-16      box32 pressure neumann             5.7e-15
    box16 velocity long step           2.4e-16      box32 velocity                     1.2e-16
    box16 velocity default depth       1.5e-16      box96x40 pressure neumann          3.1e-15
    box16 velocity smoothed coarse     1.5e-16      box96x40 pressure outlet           1.2e-14
    box16 pressure smoothed coarse     4.3e-16      box96x40 velocity                  1.2e-16
    box16x8 pressure neumann           2.0e-16      box96x40 velocity symmetric        1.5e-16
    box16x8 velocity                   1.3e-16      box32 velocity truncated           1.2e-16
    box20 pressure neumann             2.8e-16      box32flat pressure outlet          9.0e-17
    box20 pressure outlet              3.8e-16      box32flat velocity                 1.2e-16
    box20 velocity                     1.4e-16

(LAPACK inverts the float64 coarsest level: where that level is the least conditioned -- 289 and 275 unknowns, the
outlet sets -- d varies between machines by small factors, 7.7e-15 .. 1.8e-14 have been seen.  The largest 64 d is
1.8e-12, the floor 1e-14 is the bound in the well conditioned cases.)  The device's errors were 4e-16 .. 5e-14.

Which launches each case made (lattice levels / lattice launches per cycle, MI355X): box16 velocity 1 / 1 (0 / 0 with
NSFEM_LATTICE=0 and NSFEM_DICT=0), symmetric 1 / 2; box16 pressure 0 / 0; box20 velocity 1 / 1; box32 pressure 1 / 2,
velocity 2 / 2; box48 pressure 1 / 2, velocity 2 / 2; box96x40 pressure 2 / 4, velocity 3 / 3, symmetric 3 / 6;
box16x8, cube8, dfg 0 / 0; box32 truncated velocity 2 / 2; box32flat (smoothed lattice coarsest level) pressure
1 / 5, velocity 2 / 6.

Partitioned contexts (strips, slabs, exact and relaxed halo mode, the replicated coarse solve):
tests/test_gpu_partitioned_cycle.py; still out of scope there: additive (algebraic Schur) levels, periodic partitions
with wrapped global numbering, the RCB graph partition, Krylov iterates on N ranks.  The Schur hierarchy
mg_s and the mass smoother mg_m (nsfem_mg_apply 3 / 4): tests/test_gpu_monolithic_linear.py."""
import numpy as np
import pytest

import _native as nat
import mg_cycle_host as mh
from gpu_common import box, cavity_bc, context, velocity_bc

pytestmark = pytest.mark.gpu

NU = 0.01
BDF2 = (1.5, -2.0, 0.5)
STEP = 0.01                        # a = 150, b = 0.01
SWITCHES = ("NSFEM_LATTICE", "NSFEM_LATTICE_TRANSFERS", "NSFEM_DICT", "NSFEM_LATTICE_KINDS")
ENVS = {"default": {}, "transfers0": {"NSFEM_LATTICE_TRANSFERS": "0"}, "lattice0": {"NSFEM_LATTICE": "0"},
        "dict0": {"NSFEM_DICT": "0"}, "kinds0": {"NSFEM_LATTICE_KINDS": "0"}}
NO_DOFS = np.zeros(0, dtype=np.int64)


# ------------------------------------------------------------------------------------------ problems (built once)
class Problem:
    def __init__(self, mesh, dm, levels, vel, outlet, degree=2, eig_ratio=4.0):
        self.mesh, self.dm, self.levels = mesh, dm, levels
        self.vel, self.outlet = vel, outlet                    # (dofs, values) of the velocity set; pressure outlet dofs
        self.degree, self.eig_ratio = degree, eig_ratio
        self.H = mh.Hierarchy(mesh, dm, levels)
        self.dim = self.H.dim


def _box(nx, ny, p1=(1.0, 1.0), coarsest=2):
    from multigrid import structured_hierarchy
    mesh, dm, marks = box(nx, ny, p1)
    mesh.structured = ((0.0, 0.0), p1, nx, ny)
    levels = structured_hierarchy((0.0, 0.0), p1, nx, ny, coarsest=coarsest)
    outlet = np.unique(dm.facet_p1_nodes(marks.facets_with_id(2)))
    pb = Problem(mesh, dm, levels, cavity_bc(dm, marks), outlet)
    zero = lambda X: np.zeros((X.shape[0], 2))
    pb.no_lid = velocity_bc(dm, marks, [(1, zero), (2, zero), (3, zero)])
    return pb


def _cube(n):
    from multigrid import structured_hierarchy
    from test_gpu_3d import box3, lid_bc
    mesh, dm, marks = box3((n, n, n))
    levels = structured_hierarchy((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), n, n, n, coarsest=2)
    return Problem(mesh, dm, levels, lid_bc(dm, marks), np.unique(dm.facet_p1_nodes(marks.facets_with_id(2))))


def _dfg():
    import grid_generator as gg
    from fem_mesh import TaylorHoodDofMap
    mesh, marks = gg.dfg_channel(2, 1)                         # refinement_hierarchy, one refinement
    dm = TaylorHoodDofMap(mesh)
    ids = gg.DFGBoundaryMarkers
    walls = np.concatenate([marks.facets_with_id(i.value) for i in (ids.inlet, ids.bottom, ids.top, ids.cylinder)])
    nodes = np.unique(dm.facet_p2_nodes(walls))
    dofs = np.sort((2 * nodes[:, None] + np.arange(2)[None, :]).ravel())
    outlet = np.unique(dm.facet_p1_nodes(marks.facets_with_id(ids.outlet.value)))
    return Problem(mesh, dm, mesh.mg_levels, (dofs, np.zeros(dofs.size)), outlet, degree=3, eig_ratio=16.0)


_MAKERS = {
    "box16": lambda: _box(16, 16),                               # levels 16, 8, 4, 2
    "box16x8": lambda: _box(16, 8, (2.0, 1.0)),                  # lat_w != lat_h; levels 16 x 8, 8 x 4, 4 x 2
    "box20": lambda: _box(20, 20),                               # 20, 10, 5, then the non-nested 3
    "box48": lambda: _box(48, 48, coarsest=3),                   # h = 1/48: inexact dictionary; 48, 24, 12, 6, 3
    "cube8": lambda: _cube(8),                                   # 8, 4, 2; nv = 3
    "dfg": _dfg,
    "box32": lambda: _box(32, 32, coarsest=16),                  # coarsest level 17 x 17 = 289 >= 256: device Gauss-Jordan
    "box96x40": lambda: _box(96, 40, (3.0, 1.25), coarsest=10),  # h = 1/32: 96 x 40, 48 x 20, 24 x 10 (275 nodes)
    "box32flat": lambda: _box(32, 32, coarsest=32),              # no coarse mesh: P2 -> P1 (33 x 33, a lattice level)
}
_problems, _references = {}, {}


def problem(name):
    if name not in _problems:
        _problems[name] = _MAKERS[name]()
    return _problems[name]


# --------------------------------------------------------------------------------- cases: host cycle + device state
# name -> (problem, which, host cycle factory(problem, dtype)); the tests put the device into the same state
def _pressure(dirichlet_of, **kw):
    return lambda pb, dt: pb.H.pressure(dirichlet_of(pb), pb.degree, pb.eig_ratio, dtype=dt, **kw)


def _velocity(a=BDF2[0] / STEP, b=NU, bc=lambda pb: pb.vel[0], **kw):
    kw.setdefault("trunc_ratio", 0.0)
    return lambda pb, dt: pb.H.velocity(bc(pb), a, b, pb.degree, pb.eig_ratio, dtype=dt, **kw)


SMALL_COARSE = 8                   # below the 9 nodes of the 2 x 2 level: the coarsest level is smoothed (30 steps)
LATTICE_COARSE = 1000              # below the 1089 nodes of the 33 x 33 level
SHIFT = 40.0
SMALL_STEP = 1e-4                  # K_ii / M_ii * nu k / alpha0 = 1.4e-3 on the fine P1 level: truncated at level 1
LONG_STEP = 10.0                   # a = 0.15: no level is mass dominated
CASES = {
    "box16 pressure neumann": ("box16", 0, _pressure(lambda pb: NO_DOFS)),
    "box16 pressure outlet": ("box16", 0, _pressure(lambda pb: pb.outlet)),
    "box16 velocity": ("box16", 1, _velocity()),
    "box16 velocity shifted": ("box16", 1, _velocity(a=BDF2[0] / STEP + SHIFT)),
    "box16 velocity truncated": ("box16", 1, _velocity(a=BDF2[0] / SMALL_STEP, trunc_ratio=4.0, trunc_tol=0.1)),
    "box16 velocity symmetric": ("box16", 1, None),            # (coefficients of the IMEX step: filled in below)
    "box16 velocity no lid": ("box16", 1, _velocity(bc=lambda pb: pb.no_lid[0])),
    "box16 velocity long step": ("box16", 1, _velocity(a=BDF2[0] / LONG_STEP, trunc_ratio=4.0)),
    "box16 velocity default depth": ("box16", 1, _velocity(trunc_ratio=4.0)),
    "box16 velocity smoothed coarse": ("box16", 1, _velocity(coarse_dense_max=SMALL_COARSE)),
    "box16 pressure smoothed coarse": ("box16", 0, _pressure(lambda pb: pb.outlet, coarse_dense_max=SMALL_COARSE)),
    "box16x8 pressure neumann": ("box16x8", 0, _pressure(lambda pb: NO_DOFS)),
    "box16x8 velocity": ("box16x8", 1, _velocity()),
    "box20 pressure neumann": ("box20", 0, _pressure(lambda pb: NO_DOFS)),
    "box20 pressure outlet": ("box20", 0, _pressure(lambda pb: pb.outlet)),
    "box20 velocity": ("box20", 1, _velocity()),
    "box48 pressure neumann": ("box48", 0, _pressure(lambda pb: NO_DOFS)),
    "box48 velocity": ("box48", 1, _velocity()),
    "cube8 pressure neumann": ("cube8", 0, _pressure(lambda pb: NO_DOFS)),
    "cube8 velocity": ("cube8", 1, _velocity()),
    "dfg pressure outlet": ("dfg", 0, _pressure(lambda pb: pb.outlet)),
    "dfg velocity": ("dfg", 1, _velocity()),
    "box32 pressure neumann": ("box32", 0, _pressure(lambda pb: NO_DOFS)),
    "box32 velocity": ("box32", 1, _velocity()),
    "box96x40 pressure neumann": ("box96x40", 0, _pressure(lambda pb: NO_DOFS)),
    "box96x40 pressure outlet": ("box96x40", 0, _pressure(lambda pb: pb.outlet)),
    "box96x40 velocity": ("box96x40", 1, _velocity()),
    "box96x40 velocity symmetric": ("box96x40", 1, None),
    "box32 velocity truncated": ("box32", 1, _velocity(a=BDF2[0] / SMALL_STEP, trunc_ratio=4.0, trunc_tol=0.1)),
    "box32flat pressure outlet": ("box32flat", 0, _pressure(lambda pb: pb.outlet, coarse_dense_max=LATTICE_COARSE)),
    "box32flat velocity": ("box32flat", 1, _velocity(coarse_dense_max=LATTICE_COARSE)),
}


def _imex_coefficients():
    """first step of SBDF2 at the step size STEP, as IMEXTimeStepping hands it to nsfem_set_imex"""
    from imex_time_stepping import IMEXTimeStepping, IMEXType
    ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=STEP)
    ts.update_coefficients()
    return np.array(ts.alpha, float), np.array(ts.beta, float), np.array(ts.gamma, float), float(ts.get_next_step_size())


def _symmetric():
    alpha, _, gamma, k = _imex_coefficients()
    a, b = mh.operator_coefficients(alpha[0], k, NU, gamma0=gamma[0])
    return _velocity(a=a, b=b, symmetric=True)


for _name in ("box16 velocity symmetric", "box96x40 velocity symmetric"):
    CASES[_name] = CASES[_name][:2] + (_symmetric(),)


def reference(name):
    """(r, z of the float64 host cycle, d = rel(z64, z_longdouble), float64 cycle): computed once per case"""
    if name not in _references:
        pname, which, make = CASES[name]
        pb = problem(pname)
        n = pb.dm.n_p1 if which == 0 else pb.dm.n_p2 * pb.dim
        seed = sorted(CASES).index(name)
        r = np.random.default_rng(seed).standard_normal(n)      # (non-zero on flagged rows too)
        c64 = make(pb, np.float64)
        z64 = c64.apply(r)
        d = mh.rel(z64, make(pb, mh.LD).apply(r))
        _references[name] = (r, z64, d, c64)
    return _references[name]


# ------------------------------------------------------------------------------------------------- device side
def device(pb, monkeypatch, env="default", coarse_dense_max=1200, trunc_ratio=0.0, k=STEP, vel=None, pres=NO_DOFS):
    """a fresh context with the hierarchy attached and the state of the common cases"""
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for s, v in ENVS[env].items():
        monkeypatch.setenv(s, v)
    ctx = context(pb.mesh, pb.dm)
    for cm, (rp, col, val) in pb.levels:
        ctx.mg_add_level(cm.coords, cm.cells, rp, col, val, nested=getattr(cm, "nested_in_finer", None))
    ctx.mg_finalize(pb.degree, pb.eig_ratio, coarse_dense_max)
    ctx.set_coeffs(1.0, 1.0, NU)
    ctx.set_bdf(BDF2, k)
    vd, vv = pb.vel if vel is None else vel
    ctx.set_dirichlet(nat.VELOCITY, np.asarray(vd, np.int32), vv)
    ctx.set_dirichlet(nat.PRESSURE, np.asarray(pres, np.int32), np.zeros(len(pres)))
    ctx.mg_set_truncation(trunc_ratio, 0.1)
    return ctx


def compare(ctx, name, tag, lattice_levels, extra=0.0):
    """one application on the device against the case's host vector; asserts the launch path: `lattice_levels`
    levels of the hierarchy on the multi-step lattice kernel, launched if and only if there is one"""
    _, which, _ = CASES[name]
    r, z64, d, cyc = reference(name)
    before = ctx.mg_lattice_info(which)
    z = ctx.mg_apply(which, r)
    info = ctx.mg_lattice_info(which)
    launches = info["lattice_launches"] - before["lattice_launches"]
    err = mh.rel(z, z64)
    bound = max(64.0 * d, 1e-14) + extra
    print("\n[mg cycle] %-34s %-11s levels %d lattice levels %d launches %d  d %.1e  err %.2e  bound %.1e"
          % (name, tag, info["levels"], info["lattice_levels"], launches, d, err, bound))
    assert 64.0 * d < 1e-10, (name, d)
    assert info["levels"] == cyc.active, (name, tag, info, cyc.active)
    assert info["lattice_levels"] == lattice_levels, (name, tag, info)
    assert (launches > 0) == (lattice_levels > 0), (name, tag, launches)
    assert np.all(np.isfinite(z)) and err <= bound, (name, tag, err, bound)
    return z, launches


# lattice levels per switch setting: (pressure, velocity)
def _lattice_levels(pname, env):
    if env in ("lattice0", "dict0"):
        return 0, 0
    return {"box16": (0, 1), "box16x8": (0, 0), "box20": (0, 1), "box48": (1, 2), "cube8": (0, 0), "dfg": (0, 0),
            "box32": (1, 2), "box96x40": (2, 3), "box32flat": (1, 2)}[pname]


# ------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("env", list(ENVS))
@pytest.mark.parametrize("case,pres", [("box16 velocity", None), ("box16 pressure neumann", "neumann"),
                                       ("box16 pressure outlet", "outlet")])
def test_box16_every_launch_path_equals_the_one_host_vector(case, pres, env, monkeypatch):
    """2D 16 x 16, coarsest 2 (levels 16, 8, 4, 2): cavity velocity set, all-Neumann (singular) pressure, pressure
    with a Dirichlet outlet column -- under the default switches, NSFEM_LATTICE_TRANSFERS=0, NSFEM_LATTICE=0 (one-step
    dictionary kernels, launch_spmv_cheb_first), NSFEM_DICT=0 (CSR) and NSFEM_LATTICE_KINDS=0"""
    pb = problem("box16")
    ctx = device(pb, monkeypatch, env, pres=pb.outlet if pres == "outlet" else NO_DOFS)
    try:
        which = CASES[case][1]
        if which == 1:
            si = ctx.smoother_info()
            assert si["multistep_lattice_kernel"] == (env not in ("lattice0", "dict0")), si
            assert (si["kind"] == "stencil-dictionary") == (env != "dict0"), si
        compare(ctx, case, env, _lattice_levels("box16", env)[which])
    finally:
        ctx.close()


@pytest.mark.parametrize("env", ["default", "transfers0", "lattice0", "dict0", "kinds0"])
@pytest.mark.parametrize("case,pres", [("box96x40 velocity", None), ("box96x40 pressure neumann", "neumann"),
                                       ("box96x40 pressure outlet", "outlet")])
def test_three_lattice_levels_with_fused_transfers_and_the_two_level_restriction(case, pres, env, monkeypatch):
    """96 x 40 cells of side 1/32: three lattice levels in either hierarchy, lattice interpolations between them
    (fused into the smoothing launches by default, k_restrict_lattice / k_restrict_lattice2 and CSR prolongations
    with NSFEM_LATTICE_TRANSFERS=0 resp. in the cycle without pre-smoothing), a CSR transfer below the last lattice
    level, and a dense coarsest level of 275 >= 256 unknowns inverted by the device Gauss-Jordan kernels"""
    pb = problem("box96x40")
    ctx = device(pb, monkeypatch, env, pres=pb.outlet if pres == "outlet" else NO_DOFS)
    try:
        which = CASES[case][1]
        compare(ctx, case, env, _lattice_levels("box96x40", env)[which])
    finally:
        ctx.close()


@pytest.mark.parametrize("pname,env", [("box16x8", "default"), ("box20", "default"), ("box20", "dict0"),
                                       ("cube8", "default"), ("box32", "default"), ("box32", "lattice0")])
def test_other_shapes(pname, env, monkeypatch):
    """16 x 8 on (0,2) x (0,1) (lat_w != lat_h); 20 x 20 (20, 10, 5, the non-nested 3: the weight rule of h_inj,
    CSR transfers below a lattice level); 3D 8^3 (nv = 3: dictionary kernels, no lattice kernel); 32 x 32 with a
    17 x 17 coarsest level (289 unknowns: k_gj_save / k_gj_update) and a fused P2 -> P1 transfer"""
    pb = problem(pname)
    ctx = device(pb, monkeypatch, env)
    try:
        lp, lv = _lattice_levels(pname, env)
        compare(ctx, pname + " pressure neumann", env, lp)
        compare(ctx, pname + " velocity", env, lv)
        if pname == "box20":
            ctx.set_dirichlet(nat.PRESSURE, np.asarray(pb.outlet, np.int32), np.zeros(pb.outlet.size))
            compare(ctx, "box20 pressure outlet", env, lp)
    finally:
        ctx.close()


@pytest.mark.parametrize("env", ["default", "dict0"])
def test_inexact_dictionary_48(env, monkeypatch):
    """48 x 48, h = 1/48: the dictionary equals the matrices to 2^-40 only; its stated 2^-38 is added to the bound
    on the path that smooths with it"""
    pb = problem("box48")
    ctx = device(pb, monkeypatch, env)
    try:
        if env == "default":
            assert not ctx.smoother_info()["bitwise_exact"]
        extra = 2.0 ** -38 if env == "default" else 0.0
        lp, lv = _lattice_levels("box48", env)
        compare(ctx, "box48 pressure neumann", env, lp, extra)
        compare(ctx, "box48 velocity", env, lv, extra)
    finally:
        ctx.close()


def test_unstructured_refinement_hierarchy(monkeypatch):
    """DFG channel, one refinement: CSR kernels on every level, degree 3, ratio 16"""
    pb = problem("dfg")
    ctx = device(pb, monkeypatch, pres=pb.outlet)
    try:
        assert ctx.smoother_info()["kind"] != "stencil-dictionary"
        compare(ctx, "dfg pressure outlet", "default", 0)
        compare(ctx, "dfg velocity", "default", 0)
    finally:
        ctx.close()


@pytest.mark.parametrize("env", ["default", "lattice0"])
def test_smoothed_coarsest_level(env, monkeypatch):
    """coarse_dense_max below the 9 nodes of the coarsest level: 30 smoothing steps from zero there (after
    launch_spmv_cheb_first on the one-step paths)"""
    pb = problem("box16")
    ctx = device(pb, monkeypatch, env, coarse_dense_max=SMALL_COARSE, pres=pb.outlet)
    try:
        lp, lv = _lattice_levels("box16", env)
        compare(ctx, "box16 pressure smoothed coarse", env, lp)
        compare(ctx, "box16 velocity smoothed coarse", env, lv)
    finally:
        ctx.close()


@pytest.mark.parametrize("env", ["default", "transfers0", "lattice0"])
def test_smoothed_coarsest_level_on_the_lattice_kernel(env, monkeypatch):
    """32 x 32 without a coarse mesh, coarse_dense_max below the 1089 nodes of the P1 level: the last level is a
    lattice level smoothed by 30 steps from zero -- several launches with the direction carried between them, the
    first of which forms b = R r itself in the velocity cycle; the pressure hierarchy is that one level"""
    pb = problem("box32flat")
    ctx = device(pb, monkeypatch, env, coarse_dense_max=LATTICE_COARSE, pres=pb.outlet)
    try:
        lp, lv = _lattice_levels("box32flat", env)
        compare(ctx, "box32flat pressure outlet", env, lp)
        compare(ctx, "box32flat velocity", env, lv)
    finally:
        ctx.close()


@pytest.mark.parametrize("env", ["default", "transfers0"])
def test_truncated_velocity_cycle_on_two_lattice_levels(env, monkeypatch):
    """32 x 32, step 1e-4: the truncated level is a lattice level -- its trunc_steps from zero are one launch that
    (fused transfers) restricts the input itself"""
    pb = problem("box32")
    ctx = device(pb, monkeypatch, env, trunc_ratio=4.0, k=SMALL_STEP)
    try:
        assert reference("box32 velocity truncated")[3].active == 2
        compare(ctx, "box32 velocity truncated", env, 2)
    finally:
        ctx.close()


@pytest.mark.parametrize("env", ["default", "lattice0"])
def test_truncated_velocity_cycle(env, monkeypatch):
    """step 1e-4: select_velocity_cycle_depth stops at level 1 (two levels in use), solved by trunc_steps Chebyshev
    steps over [0.5 / (1 + r), 1.05 lmax]"""
    pb = problem("box16")
    ctx = device(pb, monkeypatch, env, trunc_ratio=4.0, k=SMALL_STEP)
    try:
        cyc = reference("box16 velocity truncated")[3]
        assert cyc.truncated and cyc.active == 2 and cyc.trunc_steps >= 2
        assert ctx.mg_lattice_info(1)["levels"] == 2
        compare(ctx, "box16 velocity truncated", env, _lattice_levels("box16", env)[1])
    finally:
        ctx.close()


def test_preconditioner_shift(monkeypatch):
    """the hierarchy of the time-step preconditioner: (alpha0 / k + 1 / tau) M + c_v K on every level"""
    pb = problem("box16")
    ctx = device(pb, monkeypatch)
    try:
        ctx.set_preconditioner_shift(SHIFT)
        compare(ctx, "box16 velocity shifted", "default", 1)
    finally:
        ctx.close()


@pytest.mark.parametrize("pname,env", [("box16", "default"), ("box96x40", "default"), ("box96x40", "transfers0"),
                                       ("box96x40", "lattice0")])
def test_symmetric_velocity_cycle_as_an_imex_step_leaves_it(pname, env, monkeypatch):
    """reached the way production reaches it (nsfem_step_imex is the only caller of set_velocity_cycle_symmetric(true);
    the hook needs no extension): a multigrid-preconditioned IMEX diffusion step (CG) switches the hierarchy to
    V(degree, degree) on alpha0 / k M + gamma0 c_v K and leaves it so; pre-smoothing with the fused residual,
    restriction inside the child's first launch, prolongation inside the post-smoothing launch"""
    pb = problem(pname)
    ctx = device(pb, monkeypatch, env)
    try:
        # (the default cycle first: what it leaves behind -- `restricted_to`, level buffers -- must not reach the next)
        compare(ctx, pname + " velocity", env + " bdf", _lattice_levels(pname, env)[1])
        alpha, beta, gamma, k = _imex_coefficients()
        ctx.set_imex(alpha, beta, gamma, k)
        opts = ctx.default_step_opts()
        opts.momentum.precond = opts.poisson.precond = 1
        info = ctx.step_imex(opts)
        assert info.krylov_iterations_momentum > 0
        cyc = reference(pname + " velocity symmetric")[3]
        assert cyc.pre == cyc.post == 2
        compare(ctx, pname + " velocity symmetric", env, _lattice_levels(pname, env)[1])
    finally:
        ctx.close()


def test_changing_the_dirichlet_sets_rebuilds_masks_and_coarse_inverse(monkeypatch):
    """apply, set_dirichlet, apply: flags down the levels, the lattice kernel's mask bytes, dinv, lmax and the
    (now regular) coarse inverse belong to the new sets"""
    pb = problem("box16")
    ctx = device(pb, monkeypatch)
    try:
        compare(ctx, "box16 velocity", "before", 1)
        compare(ctx, "box16 pressure neumann", "before", 0)
        vd, vv = pb.no_lid
        ctx.set_dirichlet(nat.VELOCITY, np.asarray(vd, np.int32), vv)
        ctx.set_dirichlet(nat.PRESSURE, np.asarray(pb.outlet, np.int32), np.zeros(pb.outlet.size))
        compare(ctx, "box16 velocity no lid", "after", 1)
        compare(ctx, "box16 pressure outlet", "after", 0)
        ctx.set_dirichlet(nat.VELOCITY, np.asarray(pb.vel[0], np.int32), pb.vel[1])
        ctx.set_dirichlet(nat.PRESSURE, np.zeros(0, np.int32), np.zeros(0))
        compare(ctx, "box16 velocity", "back", 1)
        compare(ctx, "box16 pressure neumann", "back", 0)
    finally:
        ctx.close()


def test_changing_the_step_size_rebuilds_operators_and_cycle_depth(monkeypatch):
    """apply, set_bdf with another step size, apply: L on every level, lmax, and the truncation going on (step 1e-4:
    two levels), staying on at the default depth rule (step 0.01) and off (step 10: all five levels)"""
    pb = problem("box16")
    ctx = device(pb, monkeypatch, trunc_ratio=4.0, k=LONG_STEP)
    try:
        assert reference("box16 velocity long step")[3].active == 5
        compare(ctx, "box16 velocity long step", "k=10", 1)
        ctx.set_bdf(BDF2, SMALL_STEP)
        assert reference("box16 velocity truncated")[3].active == 2
        compare(ctx, "box16 velocity truncated", "k=1e-4", 1)
        ctx.set_bdf(BDF2, STEP)
        compare(ctx, "box16 velocity default depth", "k=0.01", 1)
        ctx.set_bdf(BDF2, LONG_STEP)
        compare(ctx, "box16 velocity long step", "k=10 again", 1)
    finally:
        ctx.close()


def test_repeatable_zero_and_flagged_rows(monkeypatch):
    """two applies of one input are bit-identical; r = 0 gives z = 0; flagged rows: z = 0 (pressure), z = r
    (velocity)"""
    pb = problem("box16")
    ctx = device(pb, monkeypatch, pres=pb.outlet)
    try:
        for name in ("box16 velocity", "box16 pressure outlet"):
            which = CASES[name][1]
            r = reference(name)[0]
            z1, z2 = ctx.mg_apply(which, r), ctx.mg_apply(which, r)
            assert np.array_equal(z1, z2), name
            assert np.all(ctx.mg_apply(which, np.zeros_like(r)) == 0.0), name
            if which == 0:
                assert np.all(z1[pb.outlet] == 0.0)
            else:
                assert np.array_equal(z1[pb.vel[0]], r[pb.vel[0]])
    finally:
        ctx.close()
