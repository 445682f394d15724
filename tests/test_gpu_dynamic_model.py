"""Dynamic Smagorinsky model on the GPU (law 8 of nsfem_set_viscosity_law: k_dyn_moments, k_dyn_vertex, k_dyn_reduce,
k_visc_var_cell<8> / k3_visc_var_cell<8>, k_wall_facets<DIM, 8>; nsfem_set_dynamic_groups, nsfem_dynamic_constant,
nsfem_dynamic_info; DynamicSmagorinskyModel under the solver classes) against the numpy restatement of
tests/dynamic_model_host.py.  DESIGN.md 4t.

Tolerances.
  Procedure (W, LM, MM per vertex, num, den per group): the per-entry bound of the wall tests,
    2 n eps times the sum of the absolute contributions (``absolute=True`` of the restatement), n the rounded operations
    along the longest chain that ends in the entry.  Vertex entries, 2D / 3D: a physical gradient 3 / 5, an entry of G
    over the 5 / 9 differences 1 + 10 / 1 + 18, gamma 7 / 11, gamma S 1, the weight and the sum over the points 1 + 7 /
    1 + 15, the scaling |K| Delta_K^2 / sum w with Delta_K 5 / 8; the patch sum of at most 8 / 24 cells and that of W,
    the division; hat gamma 8 / 14, alpha^2 Delta_v^2 hat gamma hat S and the difference 5, the covariance 3, the
    deviator dim + 1, the contraction 2 dim^2: 80 / 160 in round numbers (``_N_VERTEX``).  Group sums: one product, the
    strided sum ceil(n_g / 256), the tree 6 + 3, on top of the vertex chain.
  cs2_g: bit for bit clip(num / den) of the device's own sums (the fp64 division is correctly rounded).
  Kernel (V, cell means) and the cross-check with law 1: 1e-13 of the largest entry, the tolerance of the family.
  Steps: u*, u 1e-9, p minus its mean 1e-8, relative -- those of the other subgrid step tests (Krylov rtol 1e-13).
  Wall rows: the bound of tests/test_wall_quantities_host.py for a law, with dim + 3 more operations (c_K).

Fields.  ``_sines``: every entry of G non-zero, for the procedure.  ``_les``: the fields of the kernel, step and wall
tests -- in 2D a superposition of stream functions sin^2(k pi x) sin^2(l pi y) (no-slip traces), in 3D a perturbed
Taylor-Green vortex; found by a search over a few seeded superpositions on the CPU (smooth solenoidal 2D fields have a
vanishing leading order of L : M, most give a negative constant), written here with their coefficients.  ``_linear``:
u = A x plus 5 % of ``_sines`` with alpha = 1.1, for which every group is clipped at cs2_max = 0.0625.

Meshes.  Beside the 2D boxes and the Kuhn boxes, the general tetrahedra of tests/general_tet_mesh.py with 72 and 384
cells, with the global group (there are no planes): the patch volumes differ, so the volume-weighted patch means are
not the unweighted ones, and a moment read from the wrong cell is a wrong moment.  The periodic fixtures of
tests/periodic_meshes.py: the vertex-to-cell lists are those of the P1 dofs, so a patch reaches across the seam and a
plane group along a periodic axis holds one image of each plane (``cells`` groups, not ``cells + 1``); the uniform ones
with the global group and every plane grouping, the mapped ones (no planes) with the global group."""
import math

import numpy as np
import pytest

import _native as nat
from dynamic_model_host import DYNAMIC, DynamicSmagorinskyRestatement
from gpu_common import cavity_bc, rel
from imex_time_stepping import IMEXTimeStepping, IMEXType
from periodic_inputs import KERNEL_CASES, dynamic_host_steps, dynamic_kernel_case, dynamic_step_setup, half_unclipped
from periodic_inputs import STEP_CASES as PERIODIC_STEP_CASES
from periodic_meshes import ALL as PERIODIC
from periodic_meshes import MAPPED, cells_of, is_periodic, lengths_of, periodic_axes, periodic_fields
from test_gpu_3d import lid_bc
from test_gpu_variable_viscosity import _COEF, GENERAL72, GENERAL384, NO_PBC, _max_rel, _mesh, _opts, is_general
from test_variable_viscosity_host import SMAGORINSKY, IMEXViscRestatement, VariableViscosityRestatement
from viscosity_models import DynamicSmagorinskyModel

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
KUHN = ((3, 2, 2), (1.0, 0.8, 0.6))
CUBE = ((4, 4, 4), (1.0, 1.0, 1.0))
_MESHES = [(4, 4), (3, 5), "mapped", KUHN, CUBE, GENERAL72, GENERAL384] + list(PERIODIC)
_N_VERTEX = {2: 80, 3: 160}
_SLOTS = (nat.U0, nat.U1, nat.U2, nat.USTAR, nat.CONV_N1, nat.CONV_N2)


def _sines(X):
    dim = X.shape[1]
    K = np.array([[1.3, -0.7, 0.5], [0.9, 1.1, -0.6], [-0.8, 0.4, 1.2]])[:dim, :dim]
    return (np.sin(3.0 * (X @ K.T) + np.array([0.2, 0.5, 0.9])[:dim]) * np.array([1.0, 0.8, 1.2])[:dim]).ravel()


_C2 = ((0.13, -0.13, 0.64), (0.10, -0.54, 0.36), (1.30, 0.95, -0.70))
_C3 = (0.35, 0.82, 0.33, -1.30, 0.91, 0.45)


def _les(X, amp=None):
    dim = X.shape[1]
    if dim == 2:
        x, y = X.T
        u = np.zeros_like(X)
        for k in (1, 2, 3):
            for l in (1, 2, 3):
                c = _C2[k - 1][l - 1] / (k * l)
                sx, sy = np.sin(k * np.pi * x), np.sin(l * np.pi * y)
                u[:, 0] += c * sx * sx * 2 * l * np.pi * sy * np.cos(l * np.pi * y)
                u[:, 1] -= c * 2 * k * np.pi * sx * np.cos(k * np.pi * x) * sy * sy
        return (0.3 if amp is None else amp) * u.ravel()
    x, y, z = X.T
    c = _C3
    u = np.stack([np.sin(np.pi * x) * np.cos(np.pi * y) * np.cos(np.pi * z) * (1 + 0.3 * c[0]) + 0.3 * c[3] * np.sin(2 * np.pi * y),
                  -np.cos(np.pi * x) * np.sin(np.pi * y) * np.cos(np.pi * z) * (1 + 0.3 * c[1]) + 0.3 * c[4] * np.sin(2 * np.pi * z),
                  0.5 * c[2] * np.cos(np.pi * x) * np.cos(np.pi * y) * np.sin(np.pi * z) + 0.3 * c[5] * np.sin(2 * np.pi * x)],
                 axis=1)
    return (4.0 if amp is None else amp) * u.ravel()


_A = np.array([[0.5, -0.75, 0.4], [1.25, 1.0 / 3.0, -0.5], [-2.0 / 3.0, 0.6, -0.875]])


def _linear(X):
    dim = X.shape[1]
    return (X @ _A[:dim, :dim].T).ravel() + 0.05 * _sines(X)


def _groups(dm, grouping):
    return DynamicSmagorinskyModel(grouping).vertex_groups(dm.p1_coords)


def _groupings(kind):
    if is_general(kind) or kind in MAPPED:
        return ["global"]
    if is_periodic(kind):
        return ["global"] + [("planes", a) for a in range(len(cells_of(kind)))]
    dim = 2 if kind == "mapped" or isinstance(kind[0], int) else 3
    return ["global"] + [("planes", a) for a in range(dim)]


def _set(ctx, dm, grouping, params):
    ctx.set_viscosity_law(DYNAMIC, params)
    if grouping != "global":
        ctx.set_dynamic_groups(*_groups(dm, grouping))


# ---------------------------------------------------------------- 1. the procedure against the restatement
_PROC_REF = {}


def _procedure_reference(kind, grouping):
    key = (kind, str(grouping))
    if key not in _PROC_REF:
        mesh, dm, marks, s, rs, make = _mesh(kind)
        u = _sines(dm.p2_coords)
        if is_periodic(kind):
            u = periodic_fields(dm.p2_coords, lengths_of(kind), periodic_axes(kind))[0]
        orc = DynamicSmagorinskyRestatement(rs, (2.0, 0.09), _groups(dm, grouping))
        _PROC_REF[key] = (u, orc, orc.vertices(u), orc.vertices(u, absolute=True), orc.sums(u), orc.sums(u, absolute=True))
    return _PROC_REF[key]


@pytest.mark.parametrize("kind,grouping", [(k, g) for k in _MESHES for g in _groupings(k)], ids=str)
def test_procedure_matches_the_restatement(kind, grouping):
    """W, LM, MM per vertex and num, den per group inside their per-entry bounds; cs2_g bit for bit the clipped quotient
    of the device's own sums; a second call returns the same bytes; no slot is written; the counters count"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    u, orc, vert, vert_abs, sums, sums_abs = _procedure_reference(kind, grouping)
    dim = dm.dim
    g = orc.group
    assert np.abs(orc.gradient(u)).max(axis=(0, 1)).min() > 0.1              # (every entry of G takes part)
    if is_general(kind):
        assert orc.vol.max() > 3.0 * orc.vol.min()                           # (weighted patch means are not plain ones)
    if is_periodic(kind):
        assert dm.n_p1 < mesh.num_vertices()
        # the patch bound of the operation count holds: 6 / 24 cells at an interior vertex, and every vertex of a
        # fixture without a wall is one
        assert np.bincount(dm.p1_dofmap.ravel()).max() == (6 if dim == 2 else 24)
        if grouping != "global":
            axis = grouping[1]
            assert orc.n_groups == cells_of(kind)[axis] + (0 if axis in periodic_axes(kind) else 1)
    n_v = _N_VERTEX[dim]
    bound_v = 2.0 * n_v * EPS * vert_abs
    counts = np.bincount(g, minlength=orc.n_groups)
    bound_g = 2.0 * (n_v + 1 + (counts[:, None] + 255) // 256 + 9) * EPS * sums_abs
    ctx = make(mesh, dm)
    try:
        for slot in (nat.U0, nat.U1, nat.U2, nat.USTAR):
            ctx.set_state(slot, u if slot == nat.U1 else 0.5 * u)
        before = {slot: ctx.get_state(slot) for slot in _SLOTS}
        _set(ctx, dm, grouping, (2.0, 0.09))
        assert ctx.dynamic_info()["groups"] == orc.n_groups and ctx.dynamic_info()["runs"] == 0
        cs2, got_s, got_v = ctx.dynamic_constant(nat.U1, details=True)
        ev, eg = np.abs(got_v - vert), np.abs(got_s - sums)
        with np.errstate(divide="ignore", invalid="ignore"):
            print("procedure %s %s: error / bound vertices %.3f groups %.3f; cs2 %s" % (
                kind, grouping, np.nanmax(ev / bound_v), np.nanmax(eg / bound_g), np.array2string(cs2[:6], precision=4)))
        assert np.abs(vert[:, 1]).max() > 1e-6 and np.abs(vert[:, 2]).max() > 1e-6
        assert (ev <= bound_v).all() and (eg <= bound_g).all()
        assert cs2.tobytes() == orc.clip(got_s).tobytes()
        again = ctx.dynamic_constant(nat.U1, details=True)
        for a, b in zip((cs2, got_s, got_v), again):
            assert a.tobytes() == b.tobytes()
        for slot in _SLOTS:
            assert ctx.get_state(slot).tobytes() == before[slot].tobytes()
        info = ctx.dynamic_info()
        assert info["runs"] == 2 and info["launches"] == 6 and info["bytes"] > 0
        assert ctx.viscosity_info() == dict(law=DYNAMIC, element_launches=0, recomputed=0)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 2. the element kernel against the restatement
# grouping of the kernel cases: one for which the restatement gives positive constants in some groups (asserted)
_KERNEL_GROUPING = {(4, 4): ("planes", 1), (3, 5): ("planes", 1), "mapped": "global", KUHN: ("planes", 0), CUBE: ("planes", 1),
                    GENERAL72: "global", GENERAL384: "global"}
# (the periodic fixtures: grouping and field of tests/periodic_inputs.py, where the restatement alone is asserted to give a
# positive, unclipped constant on at least half the groups)
_KERNEL_GROUPING.update({kind: case[0] for kind, case in KERNEL_CASES.items()})


@pytest.mark.parametrize("kind", _MESHES, ids=str)
def test_viscosity_kernel_matches_the_restatement(kind):
    """weight * V(u) and the cell means of nu_x with law 8 against the restatement fed the device's vertex constants;
    second calls return the same bytes, a weight of -1.5 rides in the kernel, no slot is written; one procedure run per
    element launch"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    grouping = _KERNEL_GROUPING[kind]
    u = dynamic_kernel_case(kind)[1] if is_periodic(kind) else _les(dm.p2_coords)
    orc = DynamicSmagorinskyRestatement(rs, (2.0, 0.09), _groups(dm, grouping))
    own = orc.constant(u)
    assert own.max() > 1e-3, own                                   # (the restatement alone: the term is not zero)
    if is_periodic(kind):
        assert half_unclipped(own, 0.09), own
    ctx = make(mesh, dm)
    try:
        ctx.set_state(nat.U1, u)
        ctx.set_state(nat.USTAR, u)
        _set(ctx, dm, grouping, (2.0, 0.09))
        cs2 = ctx.dynamic_constant(nat.U1)
        assert np.abs(cs2 - own).max() < 1e-9 * own.max()
        orc.vertex_constants = cs2[orc.group]
        want, means = orc.residual(u), orc.cell_means(u)
        got, cells = ctx.viscosity_residual(nat.U1, 1.0), ctx.viscosity_cells(nat.U1)
        err, cerr = _max_rel(got, want), _max_rel(cells, means)
        print("kernel %s law 8: V %.2e cell means %.2e (of the largest entry), cs2 up to %.4f" % (kind, err, cerr, cs2.max()))
        assert np.abs(want).max() > 1e-5 and np.abs(means).max() > 1e-6
        assert err < 1e-13 and cerr < 1e-13
        assert got.tobytes() == ctx.viscosity_residual(nat.U1, 1.0).tobytes()
        assert cells.tobytes() == ctx.viscosity_cells(nat.U1).tobytes()
        assert _max_rel(ctx.viscosity_residual(nat.USTAR, -1.5), -1.5 * want) < 1e-13
        assert not ctx.get_state(nat.CONV_N1).any() and not ctx.get_state(nat.CONV_N2).any()
        assert np.array_equal(ctx.get_state(nat.U1), u) and np.array_equal(ctx.get_state(nat.USTAR), u)
        assert ctx.viscosity_info() == dict(law=DYNAMIC, element_launches=5, recomputed=0)
        assert ctx.dynamic_info()["runs"] == 6 and ctx.dynamic_info()["launches"] == 18
    finally:
        ctx.close()


# ---------------------------------------------------------------- 3. the cross-check with law 1
@pytest.mark.parametrize("kind", [(4, 4), CUBE], ids=str)
def test_clipped_everywhere_equals_smagorinsky(kind):
    """``_linear`` with alpha = 1.1 and cs2_max = 0.0625: the restatement alone has every group at the clip, so
    c_K = cs2_max in every cell and law 8 is law 1 with C_s = 0.25; V and the cell means to 1e-13 of the largest entry"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    u = _linear(dm.p2_coords)
    cs2_max = 0.0625
    for grouping in (("global", ) if kind == (4, 4) else ("global", ("planes", 0))):
        orc = DynamicSmagorinskyRestatement(rs, (1.1, cs2_max), _groups(dm, grouping))
        sums = orc.sums(u)
        assert np.all(sums[:, 0] / sums[:, 1] > 1.1 * cs2_max) and np.all(orc.constant(u) == cs2_max), (grouping, sums)
        ctx = make(mesh, dm)
        try:
            ctx.set_state(nat.U1, u)
            _set(ctx, dm, grouping, (1.1, cs2_max))
            assert np.all(ctx.dynamic_constant(nat.U1) == cs2_max)
            V8, c8 = ctx.viscosity_residual(nat.U1, 1.0), ctx.viscosity_cells(nat.U1)
            ctx.set_viscosity_law(SMAGORINSKY, (math.sqrt(cs2_max), ))
            V1, c1 = ctx.viscosity_residual(nat.U1, 1.0), ctx.viscosity_cells(nat.U1)
            print("law 8 against law 1 %s %s: V %.2e cells %.2e" % (kind, grouping, _max_rel(V8, V1), _max_rel(c8, c1)))
            assert np.abs(V1).max() > 1e-5 and _max_rel(V8, V1) < 1e-13 and _max_rel(c8, c1) < 1e-13
        finally:
            ctx.close()


# ---------------------------------------------------------------- 4. degenerate states
@pytest.mark.parametrize("kind", [(4, 4), KUHN], ids=str)
def test_rest_and_constant_fields_give_exact_zeros(kind):
    mesh, dm, marks, s, rs, make = _mesh(kind)
    dim = dm.dim
    ctx = make(mesh, dm)
    try:
        _set(ctx, dm, ("planes", 1), (2.0, 0.09))
        for u in (np.zeros(dim * dm.n_p2), np.tile([0.3, -1.7, 0.9][:dim], dm.n_p2)):
            ctx.set_state(nat.U1, u)
            cs2, sums, vert = ctx.dynamic_constant(nat.U1, details=True)
            assert np.all(np.isfinite(vert)) and np.all(vert[:, 0] > 0.0)
            assert np.all(vert[:, 1:] == 0.0) and np.all(sums == 0.0) and np.all(cs2 == 0.0)
            V, cells = ctx.viscosity_residual(nat.U1, 1.0), ctx.viscosity_cells(nat.U1)
            assert np.all(V == 0.0) and np.all(cells == 0.0)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 5. steps against the restatement
# case: (mesh, grouping, cs2_max, step size, lid-driven boundary values?)
_STEP_CASES = {"box8-global": ((8, 8), "global", 0.04, 0.05 / 8, False),
               "box16-planes": ((16, 16), ("planes", 1), 0.04, 0.05 / 16, False),
               "kuhn4-global": (CUBE, "global", 0.005, 0.05 / 4, True),
               # the periodic channels with plane groups parallel to their walls (tests/periodic_inputs.py)
               "pchan2-planes": PERIODIC_STEP_CASES["pchan2-planes"][:4] + (False, ),
               "pchan3-planes": PERIODIC_STEP_CASES["pchan3-planes"][:4] + (False, )}
_STEP_HOST = {}


def _step_setup(name):
    kind, grouping, cs2_max, k, lid = _STEP_CASES[name]
    mesh, dm, marks, s, rs, make = _mesh(kind)
    X = dm.p2_coords
    dim = dm.dim
    if is_periodic(kind):
        pm, pd, ps, prs, grouping, cs2_max, k, vbc, f, u0 = dynamic_step_setup(name)
        return mesh, dm, s, rs, make, grouping, cs2_max, k, vbc, f, u0
    vbc = cavity_bc(dm, marks) if dim == 2 else lid_bc(dm, marks)
    if not lid:
        vbc = (vbc[0], np.zeros_like(vbc[1]))                  # (the 2D fields have no-slip traces)
    f = np.stack([np.sin(np.pi * X[:, 1]), -1.0 + X[:, 0], 0.5 * X[:, 1]][:dim], axis=1).ravel()
    return mesh, dm, s, rs, make, grouping, cs2_max, k, vbc, f, _les(X)


def _host_steps(name, steps=4):
    """the restatement with its own constants, and beside it the restatement without the term: per step the states, the
    constants of level n and the effect of the term on u*.  Host only; computed once"""
    if name in PERIODIC_STEP_CASES:
        return dynamic_host_steps(name, steps)           # (asserts half the groups positive and unclipped at every step)
    if name not in _STEP_HOST:
        mesh, dm, s, rs, make, grouping, cs2_max, k, vbc, f, u0 = _step_setup(name)
        visc = DynamicSmagorinskyRestatement(rs, (2.0, cs2_max), _groups(dm, grouping))
        runs = []
        for term in (visc, None):
            orc = IMEXViscRestatement(s, _COEF, "standard", visc=term)
            orc.body_force = f
            orc.vel[1], orc.vel[2] = u0.copy(), u0.copy()
            runs.append(orc)
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=k)
        out = []
        for _ in range(steps):
            ts.update_coefficients()
            cs2 = visc.constant(runs[0].vel[1])
            for orc in runs:
                orc.step(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size(), vbc, NO_PBC)
            out.append(dict(coef=(tuple(ts.alpha), tuple(ts.beta), tuple(ts.gamma), ts.get_next_step_size()), cs2=cs2,
                            effect=rel(runs[0].ustar, runs[1].ustar), ustar=runs[0].ustar.copy(),
                            u=runs[0].vel[0].copy(), p=runs[0].p.copy()))
            for orc in runs:
                orc.advance()
            ts.advance_time()
        _STEP_HOST[name] = out
    return _STEP_HOST[name]


def _assert_not_vacuous(name, host):
    cs2_max = _STEP_CASES[name][2]
    for i, h in enumerate(host):
        inside = (h["cs2"] > 0.2 * cs2_max) & (h["cs2"] < 0.8 * cs2_max)
        print("%s step %d: cs2 / cs2_max %s, effect on u* %.2e" % (name, i, np.array2string(h["cs2"] / cs2_max, precision=3),
                                                               h["effect"]))
        assert inside.any(), (name, i, h["cs2"])
        assert h["effect"] >= 1e-4, (name, i, h["effect"])
        if name in PERIODIC_STEP_CASES:
            assert half_unclipped(h["cs2"], cs2_max), (name, i, h["cs2"])


@pytest.mark.parametrize("name", list(_STEP_CASES))
def test_steps_match_the_restatement(name):
    """4 SBDF2 steps from ``_les`` in U1 and U2: u*, u 1e-9 and p 1e-8 against the restatement with its own constants.
    The restatement alone: at every step a group has 0.2 cs2_max < cs2_g < 0.8 cs2_max and the term moves u* by at
    least 1e-4.  One procedure run and one element launch per step, nothing recomputed"""
    mesh, dm, s, rs, make, grouping, cs2_max, k, vbc, f, u0 = _step_setup(name)
    host = _host_steps(name)
    _assert_not_vacuous(name, host)
    ctx = make(mesh, dm)
    try:
        ctx.set_coeffs(1.0, 1.0, 0.01, 1.0)
        ctx.set_dirichlet(nat.VELOCITY, *vbc)
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        ctx.set_state(nat.BODY_FORCE, f)
        _set(ctx, dm, grouping, (2.0, cs2_max))
        ctx.set_state(nat.U1, u0)
        ctx.set_state(nat.U2, u0)
        opts = _opts(ctx)
        for i, h in enumerate(host):
            ctx.set_imex(*h["coef"])
            ctx.step_imex(opts)
            us, u, p = ctx.get_state(nat.USTAR), ctx.get_state(nat.U0), ctx.get_state(nat.P)
            es, eu, ep = rel(us, h["ustar"]), rel(u, h["u"]), rel(p - p.mean(), h["p"] - h["p"].mean())
            print("%s step %d: u* %.2e u %.2e p %.2e path %s" % (name, i, es, eu, ep, ctx.imex_info()["path"]))
            assert es < 1e-9 and eu < 1e-9 and ep < 1e-8, (name, i, es, eu, ep)
            ctx.advance(0)
        info = ctx.imex_info()
        if name == "box16-planes":
            assert info["path"] == "lattice-kernel" and info["lattice_rhs"] == 4 and info["generic_rhs"] == 0, info
        else:
            assert info["generic_rhs"] == 4, info
        # (the first SBDF2 step is of first order and reads no N(u2); from the second on it is the stored N(u1))
        assert ctx.viscosity_info() == dict(law=DYNAMIC, element_launches=4, recomputed=0)
        dinfo = ctx.dynamic_info()
        assert dinfo["runs"] == 4 and dinfo["launches"] == 12, dinfo
    finally:
        ctx.close()


# ---------------------------------------------------------------- 6. the stored vector
def test_stored_vector_follows_law_groups_and_alpha_and_law_zero_returns_to_the_plain_bytes():
    """SBDF2 on box(8, 8): law 1 -> 8 -> 8 again -> 8 with plane groups -> the same groups again -> 8 with another alpha
    -> 0.  N(u2) is formed again exactly at the changes -- never because the constant moved, which it does at every
    step -- and every step matches the restatement.  After law 0 the stored bytes are those of a context that never set a
    law"""
    name = "box8-global"
    mesh, dm, s, rs, make, grouping, cs2_max, k, vbc, f, u0 = _step_setup(name)
    ctx, plain = make(mesh, dm), make(mesh, dm)
    try:
        for c in (ctx, plain):
            c.set_coeffs(1.0, 1.0, 0.01, 1.0)
            c.set_dirichlet(nat.VELOCITY, *vbc)
            c.set_dirichlet(nat.PRESSURE, *NO_PBC)
            c.set_state(nat.BODY_FORCE, f)
            c.set_state(nat.U1, u0)
            c.set_state(nat.U2, u0)
        orc = IMEXViscRestatement(s, _COEF, "standard", visc=VariableViscosityRestatement(rs, SMAGORINSKY, (0.2, )))
        orc.body_force = f
        orc.vel[1], orc.vel[2] = u0.copy(), u0.copy()
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=k)
        opts = _opts(ctx)
        planes = _groups(dm, ("planes", 1))
        constants = []

        def step(tag):
            ts.update_coefficients()
            kk = ts.get_next_step_size()
            ctx.set_imex(ts.alpha, ts.beta, ts.gamma, kk)
            ctx.step_imex(opts)
            orc.step(ts.alpha, ts.beta, ts.gamma, kk, vbc, NO_PBC)
            us, u = ctx.get_state(nat.USTAR), ctx.get_state(nat.U0)
            es, eu = rel(us, orc.ustar), rel(u, orc.vel[0])
            print("stored vector, %s: u* %.2e u %.2e" % (tag, es, eu))
            assert es < 1e-9 and eu < 1e-9, (tag, es, eu)
            ctx.advance(0)
            orc.advance()
            ts.advance_time()

        ctx.set_viscosity_law(SMAGORINSKY, (0.2, ))
        step("law 1")
        step("law 1")
        assert ctx.viscosity_info() == dict(law=1, element_launches=2, recomputed=0)
        sequence = (("8 global", (2.0, cs2_max), None, True), ("8 global again", (2.0, cs2_max), None, False),
                    ("8 planes", None, planes, True), ("8 the same planes", None, planes, False),
                    ("8 alpha 1.5", (1.5, cs2_max), planes, True), ("8 alpha 1.5 again", None, None, False))
        launches, recomputed, groups_now, params_now = 2, 0, None, None
        for tag, params, groups, changed in sequence:
            if params is not None:
                ctx.set_viscosity_law(DYNAMIC, params)           # (resets the groups to the global one)
                params_now, groups_now = params, None
            if groups is not None:
                ctx.set_dynamic_groups(*groups)
                groups_now = groups
            if changed:
                orc.visc, orc.N2 = DynamicSmagorinskyRestatement(rs, params_now, groups_now), None
            constants.append(ctx.dynamic_constant(nat.U1).tobytes())
            step(tag)
            launches += 2 if changed else 1
            recomputed += 1 if changed else 0
            assert ctx.viscosity_info() == dict(law=DYNAMIC, element_launches=launches, recomputed=recomputed), tag
        assert len(set(constants[:2])) == 2 and len(set(constants[2:4])) == 2      # the constant moved, nothing recomputed
        # law 0: the levels of the plain context on both, both form N(u2) afresh
        ts_plain = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=k)
        popts = _opts(plain)
        for _ in range(2):
            ts_plain.update_coefficients()
            plain.set_imex(ts_plain.alpha, ts_plain.beta, ts_plain.gamma, ts_plain.get_next_step_size())
            plain.step_imex(popts)
            plain.advance(0)
            ts_plain.advance_time()
        ctx.set_viscosity_law(0)
        levels = {slot: plain.get_state(slot) for slot in (nat.U0, nat.U1, nat.U2, nat.USTAR, nat.P, nat.P_OLD)}
        for c in (ctx, plain):
            for slot, value in levels.items():
                c.set_state(slot, value)
        ts_plain.update_coefficients()
        runs = ctx.dynamic_info()["runs"]
        for c, o in ((ctx, opts), (plain, popts)):
            c.set_imex(ts_plain.alpha, ts_plain.beta, ts_plain.gamma, ts_plain.get_next_step_size())
            c.step_imex(o)
        assert plain.get_state(nat.CONV_N1).any() and plain.get_state(nat.CONV_N2).any()
        for slot in (nat.CONV_N1, nat.CONV_N2):
            assert ctx.get_state(slot).tobytes() == plain.get_state(slot).tobytes()
        assert ctx.viscosity_info()["law"] == 0 and ctx.viscosity_info()["element_launches"] == launches
        assert ctx.dynamic_info()["runs"] == runs
        assert plain.dynamic_info() == dict(groups=0, runs=0, launches=0, bytes=0)
    finally:
        ctx.close()
        plain.close()


# ---------------------------------------------------------------- 7. the wall rows
@pytest.mark.parametrize("name", ["box4x4", "kuhn3x2x2", "general72", "pchan3"])
def test_wall_rows_carry_the_dynamic_viscosity(name):
    """every boundary facet, law 8 with the global group, use_law: c_K is the device's one constant in every cell, so the
    rows are those of the Smagorinsky restatement of tests/test_wall_quantities_host.py with C_s^2 = that constant --
    viscous force and torque inside its per-entry bound (dim + 3 operations more: the mean over the vertices, the host's
    sqrt and square); the conductive row is bitwise that of use_law off"""
    import test_wall_quantities_host as wh
    from test_derived_fields_host import smooth_fields as wall_fields
    mesh, dm, marks, s, rs, make = _mesh({"box4x4": (4, 4), "kuhn3x2x2": KUHN, "general72": GENERAL72}.get(name, name))
    dim = dm.dim
    ids, cells, local = wh.boundary_facets(mesh)
    _, p, T = wall_fields(dm.p2_coords, dm.p1_coords)
    u = _les(dm.p2_coords).reshape(-1, dim)
    if is_periodic(name):
        # (the periodic velocity of tests/periodic_meshes.py.  ``_les`` is exactly 0 on the walls but for a term that is
        # 0 in the identified nodes at z = L and 1e-16 at z = L / 2: the mass flux of three wall faces is a sum of such
        # terms, 6e-18 in absolute value, beside a vertex value of 0.64 whose basis function vanishes at the rule points
        # to rounding only; the per-entry bound, relative to the terms, cannot cover that entry -- DESIGN.md 5c)
        u = periodic_fields(dm.p2_coords, lengths_of(name), periodic_axes(name))[0].reshape(-1, dim)
    o = wh.OPTS
    own = DynamicSmagorinskyRestatement(rs, (2.0, 0.09)).constant(u.ravel())[0]
    assert own > 1e-3
    ctx = make(mesh, dm)
    try:
        ctx.set_scalar(o["kappa"])
        ctx.set_state(nat.T0, T)
        ctx.set_state(nat.U0, np.ascontiguousarray(u).ravel())
        ctx.set_state(nat.P, p)
        ctx.wall_set_facets(cells, local, np.zeros(ids.size, dtype=np.int32), 1)
        ctx.set_viscosity_law(DYNAMIC, (2.0, 0.09))
        cs2 = float(ctx.dynamic_constant(nat.U0)[0])
        assert abs(cs2 - own) < 1e-9 * own
        runs = ctx.dynamic_info()["runs"]
        on = ctx.wall_compute(o["nu"], o["sym"], o["kappa"], o["origin"], use_law=True, scalar_slot=nat.T0, facets=True)
        assert ctx.dynamic_info()["runs"] == runs + 1
        off = ctx.wall_compute(o["nu"], o["sym"], o["kappa"], o["origin"], use_law=False, scalar_slot=nat.T0, facets=True)
        assert ctx.dynamic_info()["runs"] == runs + 1
    finally:
        ctx.close()
    law = (SMAGORINSKY, (math.sqrt(cs2), ))
    want = wh.wall_reference(mesh, dm, (cells, local), u, p, T, o, law)
    plain = wh.wall_reference(mesh, dm, (cells, local), u, p, T, o, None, rule="kernel")
    scale = wh.wall_reference(mesh, dm, (cells, local), u, p, T, o, law, absolute=True)
    bound = 2.0 * (wh.n_terms(dim, True) + dim + 3) * EPS * scale
    force, heat = slice(1 + dim, 1 + 2 * dim), 3 + 2 * dim
    err = np.abs(on[1] - want)
    eddy = np.abs(want - plain)[:, force].max()
    with np.errstate(divide="ignore", invalid="ignore"):
        print("wall %s: cs2 %.4f, error / bound %.3f, eddy part %.3e" % (name, cs2, np.nanmax(err / bound), eddy))
    assert eddy > 1e3 * bound[:, force].max()
    assert (err <= bound).all()
    assert on[1][:, heat].tobytes() == off[1][:, heat].tobytes()
    assert not np.array_equal(on[1][:, force], off[1][:, force])


# ---------------------------------------------------------------- 8. refusals
def test_bad_parameters_groups_partitions_and_the_other_schemes_are_refused():
    mesh, dm, marks, s, rs, make = _mesh((8, 8))
    ctx = make(mesh, dm)
    try:
        for bad in (1.0, 0.5, -2.0, np.nan, np.inf):
            with pytest.raises(nat.NativeError, match="alpha"):
                ctx.set_viscosity_law(DYNAMIC, (bad, 0.09))
        for bad in (0.0, -0.1, np.nan, np.inf):
            with pytest.raises(nat.NativeError, match="cs2_max"):
                ctx.set_viscosity_law(DYNAMIC, (2.0, bad))
        for law in (3, 6, 7, 9):
            with pytest.raises(nat.NativeError, match="unknown law.*8 dynamic Smagorinsky"):
                ctx.set_viscosity_law(law, (2.0, 0.09))
        ids = np.zeros(dm.n_p1, dtype=np.int32)
        with pytest.raises(nat.NativeError, match="without law 8"):
            ctx.set_dynamic_groups(1, ids)
        with pytest.raises(nat.NativeError, match="law 8 is not set"):
            ctx.dynamic_constant(nat.U1)
        ctx.set_viscosity_law(SMAGORINSKY, (0.2, ))
        with pytest.raises(nat.NativeError, match="without law 8"):
            ctx.set_dynamic_groups(1, ids)
        assert ctx.dynamic_info() == dict(groups=0, runs=0, launches=0, bytes=0)
        ctx.set_viscosity_law(DYNAMIC, (2.0, 0.09))
        for n, bad in ((1, 1), (3, 3), (3, -1)):
            wrong = ids.copy()
            wrong[5] = bad
            with pytest.raises(nat.NativeError, match="out of range"):
                ctx.set_dynamic_groups(n, wrong)
        with pytest.raises(nat.NativeError, match="n_groups"):
            ctx.set_dynamic_groups(0, ids)
        for slot in (nat.P, nat.CONV_N1):
            with pytest.raises(nat.NativeError, match="slot"):
                ctx.dynamic_constant(slot)
        assert ctx.dynamic_info()["groups"] == 1 and ctx.dynamic_info()["runs"] == 0
        # an empty group is allowed and has cs2 = 0
        ctx.set_state(nat.U1, _les(dm.p2_coords))
        ctx.set_dynamic_groups(3, 2 * (dm.p1_coords[:, 1] > 0.5).astype(np.int32))
        cs2, sums, _ = ctx.dynamic_constant(nat.U1, details=True)
        assert cs2[1] == 0.0 and np.all(sums[1] == 0.0) and np.all(sums[[0, 2], 1] > 0.0)
        # the other schemes and the subgrid heat flux
        ctx.set_coeffs(1.0, 1.0, 0.01)
        ctx.set_dirichlet(nat.VELOCITY, *cavity_bc(dm, marks))
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        ctx.set_bdf((1.0, -1.0, 0.0), 1.0 / 16.0)
        with pytest.raises(nat.NativeError, match="variable viscosity"):
            ctx.step_ipcs()
        with pytest.raises(nat.NativeError, match="variable viscosity"):
            ctx.step_bdf()
        ctx.set_scalar(0.05, None, 0)
        ctx.set_scalar_sgs(0.85)
        ctx.set_state(nat.T1, np.ones(dm.n_p2))
        with pytest.raises(nat.NativeError, match=r"viscosity law is not 1 \(Smagorinsky\), 4 \(WALE\) or 5 \(Vreman\)"):
            ctx.scalar_explicit(nat.U1, nat.T1, 0, 1.0)
    finally:
        ctx.close()
    group = nat.local_group_create(1)
    ctx = make(mesh, dm)
    try:
        ctx.attach_local_comm(group, 0)
        with pytest.raises(nat.NativeError, match="communicator"):
            ctx.set_viscosity_law(DYNAMIC, (2.0, 0.09))
        assert ctx.viscosity_info()["law"] == 0 and ctx.dynamic_info()["bytes"] == 0
    finally:
        ctx.close()
        nat.local_group_destroy(group)


# ---------------------------------------------------------------- 9. through the classes
_SPEC = dict(name="Cavity", mesh=("cube", 2, 8), scheme="ipcs", clock=dict(dt=0.5 / 8, steps=3),
             numbers=dict(Re=100.0, Fr=1.0), start={"velocity": (0.0, 0.0), "pressure": 0.0},
             bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_slip", "bottom"), ("velocity", "top", (1.0, 0.0))])


def test_imex_solver_with_the_dynamic_model_equals_driving_the_steps_by_hand(monkeypatch):
    """IMEXIPCSSolver through InstationaryProblem.solve_problem with DynamicSmagorinskyModel(("planes", 1)) on the 8 x 8
    cavity, 3 steps: u and p are bit for bit what set_viscosity_law(8) / set_dynamic_groups / step_imex / advance give
    through the C ABI on a second context; _compute_model_constant returns nsfem_dynamic_constant,
    _compute_model_viscosity viscosity_cells, and WallQuantities runs with the law"""
    from fem_function import HostField
    from multigrid import attach_hierarchy
    from ns_imex_solver import IMEXIPCSSolver
    from problem_specs import build_problem
    from wall_quantities import WallQuantities
    steps, dt = _SPEC["clock"]["steps"], _SPEC["clock"]["dt"]
    model = DynamicSmagorinskyModel(("planes", 1), filter_ratio=2.0, cs2_max=0.09)
    monkeypatch.setenv("NSFEM_NO_OUTPUT", "1")
    problem = build_problem(dict(_SPEC))

    def set_viscosity_model(self):
        self._viscosity_model = model
    type(problem).set_viscosity_model = set_viscosity_model
    problem.set_solver_class(IMEXIPCSSolver)
    problem.compute_cfl = False
    problem.solve_problem()
    solver = problem._get_solver()
    assert isinstance(solver, IMEXIPCSSolver) and problem._time_stepping.step_number == steps
    cctx = solver._ctx
    assert cctx.viscosity_info()["law"] == DYNAMIC and cctx.viscosity_info()["recomputed"] == 0
    assert cctx.dynamic_info()["groups"] == 9 and cctx.dynamic_info()["runs"] == steps
    u_cls, p_cls = cctx.get_state(nat.U1), cctx.get_state(nat.P_OLD)
    constant = problem._compute_model_constant()
    assert constant.shape == (9, ) and np.array_equal(constant, cctx.dynamic_constant(nat.U0)) and constant.max() > 0.0
    field = problem._compute_model_viscosity()
    assert isinstance(field, HostField) and field.center == "Cell" and field.name() == "model viscosity"
    assert np.array_equal(field.values, cctx.viscosity_cells(nat.U0)) and field.values.max() > 1e-6
    runs = cctx.dynamic_info()["runs"]
    wall = WallQuantities(solver, boundary_ids=(problem._sides["top"], ))
    wall.compute()
    assert cctx.dynamic_info()["runs"] == runs + 1              # (use_law is on with a model: the procedure ran)
    # ---- the same steps through the C ABI on a fresh context
    dm, mesh = solver._dofmap, solver._mesh
    ctx = nat.NsfemContext(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, dm.n_p2, dm.n_p1)
    try:
        if solver._mg_levels is not None:
            attach_hierarchy(ctx, mesh)
        coef = solver._equation_coefficients
        ctx.set_coeffs(coef["convective_term"], coef["pressure_term"], coef["viscous_term"], coef["body_force_term"])
        bd, bv = solver._dirichlet_bcs["velocity"]
        ctx.set_dirichlet(nat.VELOCITY, np.asarray(bd, np.int32), np.asarray(bv, float))
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        ctx.set_viscosity_law(DYNAMIC, model.params(coef))
        ctx.set_dynamic_groups(*model.vertex_groups(dm.p1_coords))
        opts = solver._step_options()
        ts = IMEXTimeStepping(0.0, 1.0, IMEXType.SBDF2, desired_start_time_step=dt)
        for _ in range(steps):
            ts.update_coefficients()
            ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
            ctx.step_imex(opts)
            ts.advance_time()
            ctx.advance(0)
        u_abi, p_abi = ctx.get_state(nat.U1), ctx.get_state(nat.P_OLD)
    finally:
        ctx.close()
    assert np.abs(u_cls).max() > 0.5
    assert np.array_equal(u_cls, u_abi) and np.array_equal(p_cls, p_abi)


def test_imex_solver_on_a_periodic_channel_equals_driving_the_steps_by_hand(monkeypatch):
    """the 4 x 4 unit square periodic in x (``periodic=`` of tests/problem_specs.py), no-slip on bottom and top, set in
    motion from rest by a constant body force along x; IMEXIPCSSolver with DynamicSmagorinskyModel(("planes", 1)), 3 steps.
    The dof map the class builds has the identified nodes, the plane groups come from its P1 dofs -- 5 planes between the
    walls -- and u and p are bit for bit what the C ABI gives on a second context with that dof map"""
    from multigrid import attach_hierarchy
    from ns_imex_solver import IMEXIPCSSolver
    from problem_specs import build_problem
    n, steps, dt = 4, 3, 0.05
    spec = dict(name="PeriodicChannel", mesh=("cube", 2, n), scheme="ipcs", clock=dict(dt=dt, steps=steps),
                numbers=dict(Re=100.0, Fr=1.0), start={"velocity": (0.0, 0.0), "pressure": 0.0}, gravity=(1.0, 0.0),
                periodic=((0, ), ("left", "right")), bcs=[("no_slip", "bottom"), ("no_slip", "top")])
    model = DynamicSmagorinskyModel(("planes", 1), filter_ratio=2.0, cs2_max=0.09)
    monkeypatch.setenv("NSFEM_NO_OUTPUT", "1")
    problem = build_problem(spec)

    def set_viscosity_model(self):
        self._viscosity_model = model
    type(problem).set_viscosity_model = set_viscosity_model
    problem.set_solver_class(IMEXIPCSSolver)
    problem.compute_cfl = False
    problem.solve_problem()
    solver = problem._get_solver()
    assert isinstance(solver, IMEXIPCSSolver) and problem._time_stepping.step_number == steps
    dm, mesh = solver._dofmap, solver._mesh
    assert (mesh.num_vertices(), dm.n_p1, dm.n_p2) == ((n + 1) ** 2, n * (n + 1), 2 * n * (2 * n + 1))
    cctx = solver._ctx
    assert cctx.viscosity_info()["law"] == DYNAMIC and cctx.viscosity_info()["recomputed"] == 0
    assert cctx.dynamic_info()["groups"] == n + 1 and cctx.dynamic_info()["runs"] == steps
    u_cls, p_cls = cctx.get_state(nat.U1), cctx.get_state(nat.P_OLD)
    constant = problem._compute_model_constant()
    assert constant.shape == (n + 1, ) and np.array_equal(constant, cctx.dynamic_constant(nat.U0))
    # ---- the same steps through the C ABI on a fresh context
    ctx = nat.NsfemContext(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, dm.n_p2, dm.n_p1)
    try:
        if solver._mg_levels is not None:
            attach_hierarchy(ctx, mesh)
        coef = solver._equation_coefficients
        ctx.set_coeffs(coef["convective_term"], coef["pressure_term"], coef["viscous_term"], coef["body_force_term"])
        bd, bv = solver._dirichlet_bcs["velocity"]
        ctx.set_dirichlet(nat.VELOCITY, np.asarray(bd, np.int32), np.asarray(bv, float))
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        ctx.set_state(nat.BODY_FORCE, np.tile([1.0, 0.0], dm.n_p2))
        ctx.set_viscosity_law(DYNAMIC, model.params(coef))
        groups = model.vertex_groups(dm.p1_coords)
        assert groups[0] == n + 1
        ctx.set_dynamic_groups(*groups)
        opts = solver._step_options()
        ts = IMEXTimeStepping(0.0, 1.0, IMEXType.SBDF2, desired_start_time_step=dt)
        for _ in range(steps):
            ts.update_coefficients()
            ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
            ctx.step_imex(opts)
            ts.advance_time()
            ctx.advance(0)
        u_abi, p_abi = ctx.get_state(nat.U1), ctx.get_state(nat.P_OLD)
    finally:
        ctx.close()
    assert np.abs(u_cls).max() > 0.05
    assert np.array_equal(u_cls, u_abi) and np.array_equal(p_cls, p_abi)
