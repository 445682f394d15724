"""Lagrangian-averaged dynamic Smagorinsky model on the GPU (mode 1 of nsfem_set_dynamic_averaging: k_dyn_lagrange<DIM>
in the place of k_dyn_reduce; nsfem_dynamic_lagrangian_state / _advance / _info; the time-level rules of
nsfem_step_imex, nsfem_advance, nsfem_imex_rhs and the hooks; DynamicSmagorinskyModel(averaging="lagrangian") under the
solver classes) against the numpy restatement of tests/dynamic_lagrangian_host.py.  DESIGN.md 4w.

Tolerances.
  One advance (I', I_up per vertex): n eps times the sum of the absolute contributions, eps |LM_v| + (1 - eps)
    sum_j lambda_j |I_j| resp. sum_j lambda_j |I_j| (``absolute=True`` of the restatement).  n, counted from the
    operations (``_n_ops``): a barycentric coordinate takes the geometry (a difference, the determinant 3 / 5 + 6, the
    reciprocal and a product: 7 / 14; the gradient of lambda_0 1 / 2 more), the displacement 1 and the dot product
    2 dim - 1: n_g = 11 / 20 in 2D / 3D.  Its rounding error is absolute, relative to sum_a |g_ja d_a| <= sqrt(dim) CFL
    (|d|_inf <= CFL h with 1 / h the largest gradient) and not to the coordinate, which may be small; the own
    coordinate collects the dim others.  With the seeded state inside a factor 2 (max |I| <= 2 sum_j lambda_j |I_j|)
    the dim + 1 coordinates give 2 * 2 (dim + 1) n_g sqrt(dim) max(CFL, 1).  On top: the own coordinate dim + 1, the
    clamp (max, sum, division) dim + 3, the interpolation 2 (dim + 1), rule 4 16 (product, three roots, the root of
    Delta^2, theta, two divisions, a sum, 1 - eps, two products and a sum, the floor).
  cs2: bit for bit the clipped quotient of the device's own I' (the fp64 division is correctly rounded).
  Steps: u*, u 1e-9, p minus its mean 1e-8, relative -- those of tests/test_gpu_dynamic_model.py.
  Wall rows: the bound of tests/test_wall_quantities_host.py for a law with dim + 3 more operations.

The choice of the upstream cell is discrete: ``_advance_case`` asserts on the restatement alone that at every clamped
vertex the best and the second-best m_c differ by more than 1e-9 (inside the patch a tie is harmless: P1 interpolation
is continuous across faces); the seeds of ``_SEEDS`` were searched on the CPU so that every vertex of every case
passes.  On the general tetrahedra of tests/general_tet_mesh.py the interior patches are generic: the advance cases
assert first that NO displaced vertex, clamped or not, has a second cell within the restatement's tie margin of the
best -- the upstream cell is unique there, and the choice of the definition is the only one accepted.  The boundary
nodes are at rest in these cases: on four of the six faces the map of the mesh is a sum of functions of one surface
coordinate each, so the two triangles of a boundary quad stay in one plane and an inflow vertex there meets the same
exact tie as on a Kuhn box (tests/test_general_tet_mesh_host.py counts them).

Periodic fixtures (tests/periodic_meshes.py).  k_dyn_lagrange works with barycentric coordinates relative to the vertex,
so the upstream cell of a vertex on the seam may lie on the far side of the mesh: tests/periodic_inputs.py asserts, on the
restatement alone, that it does for at least a quarter of the displaced seam vertices, that every displaced vertex has
exactly one cell within the tie margin (directions and seeds searched on the CPU; on pchan3 the velocity vanishes on
the two walls, whose coplanar faces give the exact inflow ties of a Kuhn box), and that at CFL 0.4 nothing is clamped
on the square and the cube without a wall -- there is no boundary to leave through."""
import math

import numpy as np
import pytest

import _native as nat
from dynamic_lagrangian_host import LagrangianDynamicRestatement
from dynamic_model_host import DYNAMIC, DynamicSmagorinskyRestatement
from gpu_common import rel
from imex_composed_host import ComposedIMEX
from imex_time_stepping import IMEXTimeStepping, IMEXType
from periodic_inputs import DIRECTION as PERIODIC_DIRECTION
from periodic_inputs import across_the_seam, lagrangian_advance_case
from periodic_meshes import ALL as PERIODIC
from periodic_meshes import is_periodic, lengths_of
from test_gpu_dynamic_model import CUBE, KUHN, _SPEC, _les, _step_setup
from test_gpu_variable_viscosity import _COEF, GENERAL72, GENERAL384, NO_PBC, _mesh, _opts, is_general
from test_variable_viscosity_host import SMAGORINSKY
from viscosity_models import DynamicSmagorinskyModel

pytestmark = pytest.mark.gpu

EPS = 2.0 ** -53
_MESHES = [(4, 4), (3, 5), "mapped", KUHN, CUBE, GENERAL72, GENERAL384] + list(PERIODIC)
_CFLS = (0.4, 2.5)
_SEEDS = {}                                            # (kind, cfl) -> seed; default 0
# the mean direction of the seeded velocity of the advance cases (see ``_velocity``)
_DIRECTION = {str(KUHN): (1.0, -0.738, -0.401), str(CUBE): (-1.0, 0.596, 0.978),
              str(GENERAL72): (1.0, -0.738, -0.401), str(GENERAL384): (-1.0, 0.596, 0.978)}
_DIRECTION.update(PERIODIC_DIRECTION)                  # (the periodic fixtures: tests/periodic_inputs.py)
_SLOTS = (nat.U0, nat.U1, nat.U2, nat.USTAR, nat.CONV_N1, nat.CONV_N2)
NAN = float("nan")


def _n_ops(dim, cfl):
    n_g = 11 if dim == 2 else 20
    return int(math.ceil(4 * (dim + 1) * n_g * math.sqrt(dim) * max(cfl, 1.0))) + (dim + 1) + (dim + 3) + 2 * (dim + 1) + 16


def _height(orc):
    """h with 1 / h the largest barycentric gradient of the mesh (the smallest height of a cell)"""
    return 1.0 / np.sqrt((orc.grad ** 2).sum(axis=2)).max()


def _state4(state, prev=None):
    out = np.full((state.shape[0], 4), NAN)
    out[:, :2] = state
    if prev is not None:
        out[:, 3] = prev
    return out


def _lagrangian(ctx, params=(2.0, 0.09), lag=(1.5, 0.0256, 1e-12)):
    ctx.set_viscosity_law(DYNAMIC, params)
    ctx.set_dynamic_averaging(1, *lag)


# ---------------------------------------------------------------- 1. one advance against the restatement
_ADVANCE = {}


def _velocity(kind, dm, rng):
    """the seeded velocity of the advance cases: a mean direction plus noise at every node.  2D: 10 % noise, inflow and
    outflow at the boundary (vertices there are clamped at every CFL number).  3D: 5 % noise, times a bubble that
    vanishes on the boundary.  On the Kuhn boxes exact ties of m_c are structural -- the far faces of two cells of a
    patch lie in one coordinate plane, and so do the boundary faces at an inflow vertex, where the limiting coordinate
    of several cells is the same number -- and the clamped values of tied cells differ: the definition settles them by
    the order of the cells, a comparison of roundings that no tolerance covers.  The directions of ``_DIRECTION`` were
    searched on the CPU so that the interior vertices leave their patches at CFL 2.5 through no such pair.  The inflow
    boundaries of the Kuhn boxes have a test of their own, which accepts the choice of any tied cell.  General
    tetrahedra: the direction of the Kuhn box of the same size and 5 % noise at every interior node, zero at the nodes
    of the boundary faces (module docstring)"""
    X = dm.p2_coords
    if dm.dim == 2:
        return (np.array([0.3, 1.0])[None, :] + 0.1 * rng.standard_normal((dm.n_p2, 2))).ravel()
    if is_general(kind):
        u = np.array(_DIRECTION[str(kind)])[None, :] + 0.05 * rng.standard_normal((dm.n_p2, 3))
        u[np.unique(dm.facet_p2_nodes(np.flatnonzero(dm.mesh.facet_on_boundary)))] = 0.0
        return u.ravel()
    bubble = np.prod(np.sin(np.pi * X / X.max(axis=0)[None, :]), axis=1) ** 0.5
    bubble[bubble < 1e-7] = 0.0
    return ((np.array(_DIRECTION[str(kind)])[None, :] + 0.05 * rng.standard_normal((dm.n_p2, 3))) * bubble[:, None]).ravel()


def _advance_case(kind, cfl):
    """inputs of one advance, host only, built once: the seeded velocity and positive state, k for the CFL number, and
    the discrete choices of the restatement (with the tie assertion)"""
    key = (str(kind), cfl)
    if is_periodic(kind):
        return lagrangian_advance_case(kind, cfl)        # (tests/periodic_inputs.py, with the assertions named above)
    if key not in _ADVANCE:
        mesh, dm, marks, s, rs, make = _mesh(kind)
        orc = LagrangianDynamicRestatement(rs, (2.0, 0.09))
        rng = np.random.default_rng(_SEEDS.get(key, 0))
        u = _velocity(kind, dm, rng)
        state = rng.uniform(1.0, 2.0, (dm.n_p1, 2)) * np.array([0.03, 1.0])
        k = cfl * _height(orc) / np.abs(u).max()
        _, _, where = orc.locate(orc.vertex_velocity(u), k)
        gap = (where["best"] - where["second"])[where["clamped"]]
        assert gap.size == 0 or gap.min() > 1e-9, (key, gap.min())
        if is_general(kind):
            # generic patches: the upstream cell of every displaced vertex is unique (``tied`` counts the best cell
            # itself); the others are the boundary vertices, at rest
            moved = np.abs(orc.vertex_velocity(u)).max(axis=1) > 0.0
            assert moved.sum() >= 2 and not where["clamped"][~moved].any()
            assert np.all(where["tied"][moved] == 1), (key, np.bincount(where["tied"][moved]))
            assert (where["best"] - where["second"])[moved].min() > 1e-9
        _ADVANCE[key] = (u, state, k, orc, where)
    return _ADVANCE[key]


@pytest.mark.parametrize("cfl", _CFLS)
@pytest.mark.parametrize("kind", _MESHES, ids=str)
def test_one_advance_matches_the_restatement(kind, cfl):
    """I' and I_up inside n eps times the sums of their absolute contributions, the restatement fed the device's own
    vertex rows; cs2 bit for bit the clipped quotient of the device's I'; a second call returns the same bytes; no
    stored state and no slot is touched"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    u, state, k, orc, where = _advance_case(kind, cfl)
    assert not where["clamped"].all() if cfl < 1.0 else where["clamped"].sum() >= 2
    ctx = make(mesh, dm)
    try:
        for slot in (nat.U0, nat.U1, nat.U2, nat.USTAR):
            ctx.set_state(slot, u if slot == nat.U1 else 0.5 * u)
        _lagrangian(ctx)
        assert ctx.dynamic_lagrangian_info() == dict(active=True, have_state=False, level_formed=False, have_previous=False)
        ctx.set_dynamic_lagrangian_state(_state4(state))
        before = {slot: ctx.get_state(slot) for slot in _SLOTS}
        field, none, vert = ctx.dynamic_constant(nat.U1, details=True)
        assert none is None and field.shape == (dm.n_p1, ) and np.abs(vert[:, 1:]).max() > 1e-6
        new, up, cs2 = ctx.dynamic_lagrangian_advance(nat.U1, k, upstream=True)
        want = orc.advance(vert, orc.vertex_delta2, orc.vertex_velocity(u), k, state)
        a_new, a_up = orc.advance(vert, orc.vertex_delta2, orc.vertex_velocity(u), k, state, absolute=True)
        n = _n_ops(dm.dim, cfl)
        e_new, e_up = np.abs(new - want["state"]), np.abs(up - want["upstream"])
        with np.errstate(divide="ignore", invalid="ignore"):
            print("advance %s CFL %.1f: clamped %d of %d, error / bound I' %.3f I_up %.3f (n = %d)" % (
                kind, cfl, where["clamped"].sum(), dm.n_p1, np.nanmax(e_new / (n * EPS * a_new)),
                np.nanmax(e_up / (n * EPS * a_up)), n))
        assert (e_new <= n * EPS * a_new).all() and (e_up <= n * EPS * a_up).all()
        assert cs2.tobytes() == orc.clip_quotient(new).tobytes()
        assert (cs2 > 0.0).any() and np.all(new[:, 1] > 0.0)
        again = ctx.dynamic_lagrangian_advance(nat.U1, k, upstream=True)
        for a, b in zip((new, up, cs2), again):
            assert a.tobytes() == b.tobytes()
        got = ctx.dynamic_lagrangian_state()
        assert got[:, :2].tobytes() == state.tobytes() and np.isnan(got[:, 2:]).all()
        for slot in _SLOTS:
            assert ctx.get_state(slot).tobytes() == before[slot].tobytes()
        assert ctx.viscosity_info() == dict(law=DYNAMIC, element_launches=0, recomputed=0)
    finally:
        ctx.close()


@pytest.mark.parametrize("cfl", _CFLS)
@pytest.mark.parametrize("kind", [KUHN, CUBE], ids=str)
def test_one_advance_at_the_inflow_boundaries_of_kuhn_boxes(kind, cfl):
    """the velocity of the 3D advance cases WITHOUT the bubble: boundary vertices are displaced, those at an inflow face
    leave the domain and are clamped.  There the limiting coordinate of several cells is the same number (their faces
    lie in the boundary plane), the tie of m_c is exact up to rounding and the clamped values of the tied cells
    differ: the definition takes the first cell of the largest m_c, which the device and the restatement settle each
    by its own rounding.  So a vertex passes if I' and I_up lie inside the bound of the advance test for the choice
    of ANY cell whose m_c is within 1e-9 of the best (``rank`` of the restatement); a vertex without a tie has one
    choice, the definition's.  cs2 stays bit for bit the clipped quotient of the device's I'"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    orc = LagrangianDynamicRestatement(rs, (2.0, 0.09))
    rng = np.random.default_rng(0)
    u = (np.array(_DIRECTION[str(kind)])[None, :] + 0.05 * rng.standard_normal((dm.n_p2, 3))).ravel()
    state = rng.uniform(1.0, 2.0, (dm.n_p1, 2)) * np.array([0.03, 1.0])
    k = cfl * _height(orc) / np.abs(u).max()
    uv = orc.vertex_velocity(u)
    _, _, where = orc.locate(uv, k)
    tied = where["clamped"] & (where["tied"] > 1)
    boundary = np.any((dm.p1_coords < 1e-12) | (dm.p1_coords > np.array(kind[1])[None, :] - 1e-12), axis=1)
    assert (tied & boundary).sum() >= 4 and (where["clamped"] & ~tied & boundary).sum() >= 4
    ctx = make(mesh, dm)
    try:
        ctx.set_state(nat.U1, u)
        _lagrangian(ctx)
        ctx.set_dynamic_lagrangian_state(_state4(state))
        vert = ctx.dynamic_constant(nat.U1, details=True)[2]
        new, up, cs2 = ctx.dynamic_lagrangian_advance(nat.U1, k, upstream=True)
    finally:
        ctx.close()
    n = _n_ops(3, cfl)
    ok = np.zeros(dm.n_p1, dtype=bool)
    first = None
    for rank in range(int(where["tied"].max())):
        want = orc.advance(vert, orc.vertex_delta2, uv, k, state, rank=rank)
        a_new, a_up = orc.advance(vert, orc.vertex_delta2, uv, k, state, absolute=True, rank=rank)
        fits = np.all(np.abs(new - want["state"]) <= n * EPS * a_new, axis=1) & \
            np.all(np.abs(up - want["upstream"]) <= n * EPS * a_up, axis=1)
        first = fits if first is None else first
        ok |= fits
    print("inflow %s CFL %.1f: clamped %d, of them tied %d (up to %d cells); the definition's own choice fits at %d of %d "
          "vertices, another tied cell's at %d" % (kind, cfl, where["clamped"].sum(), tied.sum(), where["tied"].max(),
                                                  first.sum(), dm.n_p1, (ok & ~first).sum()))
    assert first[~tied].all()
    assert ok.all()
    assert cs2.tobytes() == orc.clip_quotient(new).tobytes()


# ---------------------------------------------------------------- 2. linear state, uniform velocity
@pytest.mark.parametrize("kind", [(4, 4), KUHN], ids=str)
def test_linear_state_is_interpolated_exactly_upstream(kind):
    """I = a + b . x > 0, uniform u at CFL 0.4: the device's I_up at the interior vertices is I(x_v - k u) inside the
    bound of the advance test -- the coordinates are a convex combination there, so the sum of the absolute
    contributions is the value itself.  Independent of the restatement"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    dim = dm.dim
    X = dm.p1_coords
    b = np.array([[0.7, -0.4, 0.25], [0.3, 0.5, -0.2]])[:, :dim]
    w = np.array([0.6, -0.35, 0.45])[:dim]
    lengths = np.array((1.0, 1.0) if dim == 2 else KUHN[1])
    h = 0.25 if dim == 2 else 0.3
    k = 0.4 * h / np.abs(w).max()

    def linear(x):
        return np.stack([2.0 + x @ b[0], 1.5 + x @ b[1]], axis=1)
    inside = np.all((X > 1e-12) & (X < lengths[None, :] - 1e-12), axis=1)
    assert inside.sum() >= 2
    ctx = make(mesh, dm)
    try:
        ctx.set_state(nat.U1, np.tile(w, dm.n_p2))
        _lagrangian(ctx)
        ctx.set_dynamic_lagrangian_state(_state4(linear(X)))
        new, up, cs2 = ctx.dynamic_lagrangian_advance(nat.U1, k, upstream=True)
    finally:
        ctx.close()
    want = linear(X - k * w[None, :])
    bound = _n_ops(dim, 0.4) * EPS * np.abs(want)
    err = np.abs(up - want)
    print("linear %s: error / bound %.3f" % (kind, (err / bound)[inside].max()))
    assert (err <= bound)[inside].all() and np.abs(up - linear(X))[inside].max() > 1e-3


@pytest.mark.parametrize("kind", ["psquare", "pbox3"])
def test_periodic_state_is_interpolated_upstream_across_the_seam(kind):
    """the periodic twin of the test above.  A linear function of x is no function of the dof on a periodic mesh (it
    jumps by b . L at the seam), so the state is trigonometric, I = 2 + 0.5 sin(2 pi x / L + ...) > 0 per component, and
    the yardstick is the restatement: uniform u with a component along every axis at CFL 0.4, nothing clamped, one
    cell within the tie margin at every vertex (asserted on the restatement), I_up inside the bound of the advance
    test.  Independent of the vertex rows: with the uniform velocity LM = MM = 0"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    dim = dm.dim
    X = dm.p1_coords
    w = np.array(_DIRECTION[kind])
    orc = LagrangianDynamicRestatement(rs, (2.0, 0.09))
    k = 0.4 * _height(orc) / np.abs(w).max()
    phase = 2.0 * np.pi * X / np.array(lengths_of(kind))[None, :]
    state = np.stack([2.0 + 0.5 * np.sin(phase @ np.array([1.0, -1.0, 1.0])[:dim] + 0.3),
                      1.5 + 0.4 * np.cos(phase @ np.array([1.0, 1.0, -1.0])[:dim] - 0.8)], axis=1)
    uv = np.tile(w, (dm.n_p1, 1))
    lam, ids, where = orc.locate(uv, k)
    assert not where["clamped"].any() and np.all(where["tied"] == 1)
    across = across_the_seam(kind, dm, where["cstar"])[1]
    assert 4 * across.sum() >= dm.n_p1
    want = np.zeros((dm.n_p1, 2))
    for j in range(dim + 1):
        want = want + lam[:, j, None] * state[ids[:, j]]
    ctx = make(mesh, dm)
    try:
        ctx.set_state(nat.U1, np.tile(w, dm.n_p2))
        _lagrangian(ctx)
        ctx.set_dynamic_lagrangian_state(_state4(state))
        new, up, cs2 = ctx.dynamic_lagrangian_advance(nat.U1, k, upstream=True)
    finally:
        ctx.close()
    bound = _n_ops(dim, 0.4) * EPS * np.abs(want)
    err = np.abs(up - want)
    print("periodic state %s: error / bound %.3f, %d of %d upstream cells across the seam" % (
        kind, (err / bound).max(), across.sum(), dm.n_p1))
    assert (err <= bound).all() and np.abs(up - state).max() > 1e-3


# ---------------------------------------------------------------- 3. exact zeros
@pytest.mark.parametrize("kind", [(4, 4), KUHN], ids=str)
def test_exact_zeros(kind):
    """u = 0: I_up is the old vertex value bit for bit.  Rest and a constant velocity with a zero state: every output is
    exactly 0.0 and V = 0"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    dim = dm.dim
    rng = np.random.default_rng(3)
    state = rng.uniform(0.1, 2.0, (dm.n_p1, 2))
    ctx = make(mesh, dm)
    try:
        _lagrangian(ctx)
        ctx.set_state(nat.U1, np.zeros(dim * dm.n_p2))
        ctx.set_dynamic_lagrangian_state(_state4(state))
        new, up, cs2 = ctx.dynamic_lagrangian_advance(nat.U1, 0.05, upstream=True)
        assert up.tobytes() == state.tobytes()
        ctx.set_dynamic_lagrangian_state(_state4(np.zeros((dm.n_p1, 2)), np.zeros(dm.n_p1)))
        for u in (np.zeros(dim * dm.n_p2), np.tile([0.3, -1.7, 0.9][:dim], dm.n_p2)):
            ctx.set_state(nat.U1, u)
            new, up, cs2 = ctx.dynamic_lagrangian_advance(nat.U1, 0.05, upstream=True)
            assert np.all(new == 0.0) and np.all(up == 0.0) and np.all(cs2 == 0.0)
            V, cells = ctx.viscosity_residual(nat.U1, 1.0), ctx.viscosity_cells(nat.U1)
            assert np.all(V == 0.0) and np.all(cells == 0.0)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 4. composed SBDF2 steps
class _Composed(ComposedIMEX):
    """the composed host step with the Lagrangian restatement plugged in: the explicit vector of a level carries V(u)
    with the vertex field of that level -- cs2_cur, formed once, for level n; cs2_prev, or rule 6 on u2, for level n-1.
    The host keeps no vector, so its N(u2) is formed again at every step with cs2_prev: what the device stored"""

    def __init__(self, space, rspace, coeffs, visc):
        super().__init__(space, rspace, coeffs)
        self.visc, self.k = visc, None

    def terms(self, u, level):
        out = list(super().terms(u, level))
        if self.visc is not None:
            self.visc.vertex_constants = self.visc.level_constants(u, level, self.k)
            out.append(("viscosity", self.visc.residual(u)))
        return out

    def rhs(self, alpha, beta, gamma, k):
        self.k = k
        return super().rhs(alpha, beta, gamma, k)

    def advance(self, scalar=False):
        super().advance(scalar=False)
        if self.visc is not None:
            self.visc.rotate()


# case: the mesh case of tests/test_gpu_dynamic_model.py and cs2_init (inside (0, cs2_max) of that case)
_STEP_CASES = {"box8-global": 0.0256, "box16-planes": 0.0256, "kuhn4-global": 0.002, "pchan2-planes": 0.0256}
_STEP_HOST = {}


def _host_steps(name, steps=4):
    if name not in _STEP_HOST:
        mesh, dm, s, rs, make, grouping, cs2_max, k, vbc, f, u0 = _step_setup(name)
        visc = LagrangianDynamicRestatement(rs, (2.0, cs2_max), (1.5, _STEP_CASES[name], 1e-12))
        runs = []
        for term in (visc, None):
            orc = _Composed(s, rs, _COEF, term)
            orc.body_force = f
            orc.vel[1], orc.vel[2] = u0.copy(), u0.copy()
            runs.append(orc)
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=k)
        out = []
        for _ in range(steps):
            ts.update_coefficients()
            for orc in runs:
                orc.step(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size(), vbc, NO_PBC)
            out.append(dict(coef=(tuple(ts.alpha), tuple(ts.beta), tuple(ts.gamma), ts.get_next_step_size()),
                            cs2=visc.cs2_cur.copy(), state=visc.I_new.copy(), effect=rel(runs[0].ustar, runs[1].ustar),
                            ustar=runs[0].ustar.copy(), u=runs[0].vel[0].copy(), p=runs[0].p.copy()))
            for orc in runs:
                orc.advance()
            ts.advance_time()
        visc.reset()
        _STEP_HOST[name] = out
    return _STEP_HOST[name]


def _prepare(ctx, name):
    mesh, dm, s, rs, make, grouping, cs2_max, k, vbc, f, u0 = _step_setup(name)
    ctx.set_coeffs(1.0, 1.0, 0.01, 1.0)
    ctx.set_dirichlet(nat.VELOCITY, *vbc)
    ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
    ctx.set_state(nat.BODY_FORCE, f)
    _lagrangian(ctx, (2.0, cs2_max), (1.5, _STEP_CASES[name], 1e-12))
    ctx.set_state(nat.U1, u0)
    ctx.set_state(nat.U2, u0)
    return cs2_max


@pytest.mark.parametrize("name", list(_STEP_CASES))
def test_steps_match_the_composed_host(name):
    """4 SBDF2 steps from the fields of tests/test_gpu_dynamic_model.py in U1 and U2, no prior state (rule 6 at the first
    step).  The restatement alone: at every step some vertices sit strictly inside (0, cs2_max) and the model moves u*.
    One advance (procedure run) and one element launch per step, three procedure launches per step, nothing formed
    again"""
    mesh, dm, s, rs, make, grouping, cs2_max, k, vbc, f, u0 = _step_setup(name)
    host = _host_steps(name)
    for i, h in enumerate(host):
        inside = (h["cs2"] > 0.0) & (h["cs2"] < cs2_max)
        print("%s step %d: %d of %d vertices inside (0, cs2_max), mean cs2 / cs2_max %.3f, effect on u* %.2e" % (
            name, i, inside.sum(), inside.size, h["cs2"].mean() / cs2_max, h["effect"]))
        assert inside.any() and h["effect"] >= 1e-5, (name, i, h["effect"])
    assert not np.array_equal(host[0]["cs2"], host[1]["cs2"])
    ctx = make(mesh, dm)
    try:
        _prepare(ctx, name)
        opts = _opts(ctx)
        for i, h in enumerate(host):
            ctx.set_imex(*h["coef"])
            ctx.step_imex(opts)
            us, u, p = ctx.get_state(nat.USTAR), ctx.get_state(nat.U0), ctx.get_state(nat.P)
            es, eu, ep = rel(us, h["ustar"]), rel(u, h["u"]), rel(p - p.mean(), h["p"] - h["p"].mean())
            ec = np.abs(ctx.dynamic_constant(nat.U1) - h["cs2"]).max() / cs2_max
            print("%s step %d: u* %.2e u %.2e p %.2e cs2 %.2e path %s" % (name, i, es, eu, ep, ec, ctx.imex_info()["path"]))
            assert es < 1e-9 and eu < 1e-9 and ep < 1e-8 and ec < 1e-7, (name, i, es, eu, ep, ec)
            assert ctx.dynamic_lagrangian_info()["level_formed"]
            ctx.advance(0)
            assert ctx.dynamic_lagrangian_info() == dict(active=True, have_state=True, level_formed=False, have_previous=True)
        info = ctx.imex_info()
        if name == "box16-planes":
            assert info["path"] == "lattice-kernel" and info["lattice_rhs"] == 4 and info["generic_rhs"] == 0, info
        else:
            assert info["generic_rhs"] == 4, info
        assert ctx.viscosity_info() == dict(law=DYNAMIC, element_launches=4, recomputed=0)
        dinfo = ctx.dynamic_info()
        assert dinfo["runs"] == 4 and dinfo["launches"] == 12, dinfo
    finally:
        ctx.close()


# ---------------------------------------------------------------- 5. the time-level rules
def _step(ctx, ts, opts, advance=True):
    ts.update_coefficients()
    ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
    info = ctx.step_imex(opts)
    if advance:
        ctx.advance(0)
        ts.advance_time()
    return info


def test_time_level_rules():
    """box(8, 8).  A second nsfem_step_imex without nsfem_advance launches nothing of the procedure and returns the same
    bytes (the explicit vector, the state, the field, u*, u and p); nsfem_imex_rhs does not move the state; an invalidated N(u2) is formed with
    cs2_prev (against the restatement); mode 1 -> 0 -> 1 resets the state and N(u2) is formed again exactly at the
    changes; after mode 0 the bytes of law 8 with the global group are those of a context that never switched"""
    name = "box8-global"
    mesh, dm, s, rs, make, grouping, cs2_max, k, vbc, f, u0 = _step_setup(name)
    ctx, plain, probe = make(mesh, dm), make(mesh, dm), make(mesh, dm)
    try:
        # (the Krylov solves postpone their first convergence check by the count of the solve before -- a memory that
        # is no part of the state and that the first of two equal steps does not share with the second: a probe finds
        # the counts of the first two steps, and first_check pinned to their maximum takes it out, as in the restart test)
        _prepare(probe, name)
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=k)
        counts = []
        for _ in range(2):
            info = _step(probe, ts, _opts(probe))
            counts.append((info.krylov_iterations_momentum, info.krylov_iterations_poisson, info.krylov_iterations_correction))
        probe.close()
        _prepare(ctx, name)
        opts, pinned = _opts(ctx), _opts(ctx)
        for ko, floor in zip((pinned.momentum, pinned.poisson, pinned.correction), np.max(counts, axis=0)):
            ko.first_check = int(floor)
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=k)
        _step(ctx, ts, pinned)
        _step(ctx, ts, pinned, advance=False)
        runs = ctx.dynamic_info()["runs"]

        def everything():
            return (ctx.get_state(nat.CONV_N1), ctx.dynamic_lagrangian_state(), ctx.dynamic_constant(nat.U1),
                    ctx.get_state(nat.USTAR), ctx.get_state(nat.U0), ctx.get_state(nat.P))
        first = everything()
        ctx.step_imex(pinned)
        assert ctx.dynamic_info()["runs"] == runs and ctx.viscosity_info()["element_launches"] == 3
        for a, b in zip(first, everything()):
            assert a.tobytes() == b.tobytes()
        # nsfem_imex_rhs: N(u2) afresh with cs2_prev, N(u1) with cs2_cur; the state stays
        state = ctx.dynamic_lagrangian_state()
        launches = ctx.dynamic_info()["launches"]
        rhs, n1 = ctx.imex_rhs("generic")
        assert ctx.dynamic_info()["launches"] == launches                    # (both fields exist: nothing to run)
        assert ctx.dynamic_lagrangian_state().tobytes() == state.tobytes()
        assert n1.tobytes() == first[0].tobytes()
        ts.advance_time()
        ctx.advance(0)
        state = ctx.dynamic_lagrangian_state()
        rhs, n1 = ctx.imex_rhs("generic")                           # (level n not formed: scratch only)
        assert ctx.dynamic_info()["launches"] == launches + 3
        assert ctx.dynamic_lagrangian_state().tobytes() == state.tobytes()
        assert not ctx.dynamic_lagrangian_info()["level_formed"]
        # an invalidated N(u2) is formed with cs2_prev: V(u2) of the hook is that of the restatement with that field
        recomputed = ctx.viscosity_info()["recomputed"]
        u2 = ctx.get_state(nat.U2)
        ctx.set_state(nat.U2, u2)
        orc = DynamicSmagorinskyRestatement(rs, (2.0, cs2_max))
        orc.vertex_constants = state[:, 3]
        V2 = ctx.viscosity_residual(nat.U2, 1.0)
        want = orc.residual(u2)
        assert np.abs(want).max() > 1e-6 and np.abs(V2 - want).max() < 1e-13 * np.abs(want).max()
        # ... and the vector the step forms again is, byte for byte, the one it had stored with that field
        conv = ctx.get_state(nat.CONV_N2)
        assert conv.any()
        _step(ctx, ts, opts, advance=False)
        assert ctx.viscosity_info()["recomputed"] == recomputed + 1
        assert ctx.get_state(nat.CONV_N2).tobytes() == conv.tobytes()
        ctx.advance(0)
        ts.advance_time()
        # mode 1 -> 0 -> 1
        for mode in (0, 1):
            before = ctx.viscosity_info()["recomputed"]
            ctx.set_dynamic_averaging(mode)
            info = ctx.dynamic_lagrangian_info()
            assert info == dict(active=bool(mode), have_state=False, level_formed=False, have_previous=False)
            _step(ctx, ts, opts)
            assert ctx.viscosity_info()["recomputed"] == before + 1
            ctx.set_dynamic_averaging(mode)                                    # (the same again: nothing changes)
            _step(ctx, ts, opts)
            assert ctx.viscosity_info()["recomputed"] == before + 1
        # mode 0 after mode 1: the bytes of a context that never switched
        ctx.set_dynamic_averaging(0)
        plain.set_coeffs(1.0, 1.0, 0.01, 1.0)
        plain.set_dirichlet(nat.VELOCITY, *vbc)
        plain.set_dirichlet(nat.PRESSURE, *NO_PBC)
        plain.set_state(nat.BODY_FORCE, f)
        plain.set_viscosity_law(DYNAMIC, (2.0, cs2_max))
        for c in (ctx, plain):
            c.set_state(nat.U1, u0)
            c.set_state(nat.U2, 0.9 * u0)
        assert ctx.dynamic_constant(nat.U1, details=True)[0].tobytes() == plain.dynamic_constant(nat.U1, details=True)[0].tobytes()
        assert ctx.viscosity_residual(nat.U1, 1.0).tobytes() == plain.viscosity_residual(nat.U1, 1.0).tobytes()
        plain.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
        assert ctx.imex_rhs("generic")[1].tobytes() == plain.imex_rhs("generic")[1].tobytes()
    finally:
        ctx.close()
        plain.close()
        probe.close()


# ---------------------------------------------------------------- 6. restart
def test_restart_in_a_fresh_context_is_bit_for_bit():
    """four steps in one context against two steps, the state and the slots carried into a fresh context, two more.
    The Krylov solves postpone their first convergence check by the iteration count of the solve before, a memory that
    a fresh context does not have and that is no part of the state: a first run of the four steps finds the largest
    count of each of the three solves, and first_check set to it takes that memory out of the compared runs (every
    solve then runs to that count)"""
    name = "box8-global"
    mesh, dm, s, rs, make, grouping, cs2_max, k, vbc, f, u0 = _step_setup(name)
    levels = (nat.U1, nat.U2, nat.P_OLD, nat.CONV_N2)

    floors = [0, 0, 0]

    def options(c):
        o = _opts(c)
        for ko, floor in zip((o.momentum, o.poisson, o.correction), floors):
            ko.first_check = floor
        return o
    probe, one, two, three = make(mesh, dm), make(mesh, dm), make(mesh, dm), make(mesh, dm)
    try:
        _prepare(probe, name)
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=k)
        counts = []
        for _ in range(4):
            info = _step(probe, ts, options(probe))
            counts.append((info.krylov_iterations_momentum, info.krylov_iterations_poisson, info.krylov_iterations_correction))
        floors[:] = [int(c) for c in np.max(counts, axis=0)]
        print("restart: iteration counts %s" % (counts, ))
        _prepare(one, name)
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=k)
        for _ in range(4):
            _step(one, ts, options(one))
        _prepare(two, name)
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=k)
        for _ in range(2):
            _step(two, ts, options(two))
        saved = {slot: two.get_state(slot) for slot in levels}
        state = two.dynamic_lagrangian_state()
        assert not np.isnan(state).any() and np.array_equal(state[:, 2], state[:, 3])
        _prepare(three, name)
        for slot in levels:
            three.set_state(slot, saved[slot])
        three.set_dynamic_lagrangian_state(state)
        for _ in range(2):
            _step(three, ts, options(three))
        for slot in (nat.U1, nat.U2, nat.P_OLD):
            assert np.isfinite(one.get_state(slot)).all()
            assert three.get_state(slot).tobytes() == one.get_state(slot).tobytes(), slot
        assert three.dynamic_lagrangian_state().tobytes() == one.dynamic_lagrangian_state().tobytes()
        assert three.viscosity_info()["recomputed"] == 0 and three.dynamic_info()["runs"] == 2
    finally:
        for c in (probe, one, two, three):
            c.close()


# ---------------------------------------------------------------- 7. wall rows, refusals, the classes
def test_wall_rows_read_the_stored_field():
    """every boundary facet of box(4, 4), use_law: the rows carry the STORED field -- a uniform 0.05 put there through
    the state call, which no run of the procedure on this velocity gives -- so they are those of the Smagorinsky
    restatement with C_s^2 = 0.05, inside its bound with dim + 3 more operations; the procedure is not run"""
    import test_wall_quantities_host as wh
    from test_derived_fields_host import smooth_fields as wall_fields
    mesh, dm, marks, s, rs, make = _mesh((4, 4))
    dim = dm.dim
    ids, cells, local = wh.boundary_facets(mesh)
    _, p, T = wall_fields(dm.p2_coords, dm.p1_coords)
    u = _les(dm.p2_coords).reshape(-1, dim)
    o = wh.OPTS
    cs2 = 0.05
    ctx = make(mesh, dm)
    try:
        ctx.set_scalar(o["kappa"])
        ctx.set_state(nat.T0, T)
        ctx.set_state(nat.U0, np.ascontiguousarray(u).ravel())
        ctx.set_state(nat.P, p)
        ctx.wall_set_facets(cells, local, np.zeros(ids.size, dtype=np.int32), 1)
        _lagrangian(ctx)
        ctx.set_dynamic_lagrangian_state(_state4(np.tile([cs2, 1.0], (dm.n_p1, 1)), np.full(dm.n_p1, cs2)))
        runs = ctx.dynamic_info()["runs"]
        assert np.all(ctx.dynamic_constant(nat.U0) == cs2)
        on = ctx.wall_compute(o["nu"], o["sym"], o["kappa"], o["origin"], use_law=True, scalar_slot=nat.T0, facets=True)
        off = ctx.wall_compute(o["nu"], o["sym"], o["kappa"], o["origin"], use_law=False, scalar_slot=nat.T0, facets=True)
        assert ctx.dynamic_info()["runs"] == runs
    finally:
        ctx.close()
    law = (SMAGORINSKY, (math.sqrt(cs2), ))
    want = wh.wall_reference(mesh, dm, (cells, local), u, p, T, o, law)
    scale = wh.wall_reference(mesh, dm, (cells, local), u, p, T, o, law, absolute=True)
    bound = 2.0 * (wh.n_terms(dim, True) + dim + 3) * EPS * scale
    force = slice(1 + dim, 1 + 2 * dim)
    err = np.abs(on[1] - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        print("wall rows, stored field: error / bound %.3f" % np.nanmax(err / bound))
    assert (err <= bound).all()
    assert not np.array_equal(on[1][:, force], off[1][:, force])


def test_refusals():
    mesh, dm, marks, s, rs, make = _mesh((8, 8))
    ctx = make(mesh, dm)
    try:
        with pytest.raises(nat.NativeError, match="without law 8"):
            ctx.set_dynamic_averaging(1)
        ctx.set_viscosity_law(DYNAMIC, (2.0, 0.09))
        for call in (ctx.dynamic_lagrangian_state, lambda: ctx.dynamic_lagrangian_advance(nat.U1, 0.1)):
            with pytest.raises(nat.NativeError, match="Lagrangian averaging is not set"):
                call()
        with pytest.raises(nat.NativeError, match="unknown averaging mode"):
            ctx.set_dynamic_averaging(2)
        for bad in (0.0, -1.0, np.nan, np.inf):
            with pytest.raises(nat.NativeError, match="theta"):
                ctx.set_dynamic_averaging(1, theta=bad)
        for bad in (-1e-3, np.nan, np.inf):
            with pytest.raises(nat.NativeError, match="cs2_init"):
                ctx.set_dynamic_averaging(1, cs2_init=bad)
            with pytest.raises(nat.NativeError, match="cs2_floor"):
                ctx.set_dynamic_averaging(1, cs2_floor=bad)
        assert not ctx.dynamic_lagrangian_info()["active"]
        # the scalar dynamic flux and mode 1 refuse each other
        ctx.set_scalar(0.05, None, 0)
        ctx.set_scalar_sgs_dynamic(True, 0.2)
        with pytest.raises(nat.NativeError, match="Lagrangian C_theta is not supported"):
            ctx.set_dynamic_averaging(1)
        ctx.set_scalar_sgs_dynamic(False)
        ctx.set_dynamic_averaging(1)
        with pytest.raises(nat.NativeError, match="Lagrangian C_theta is not supported"):
            ctx.set_scalar_sgs_dynamic(True, 0.2)
        # the hooks of mode 1
        ctx.set_state(nat.U1, _les(dm.p2_coords))
        with pytest.raises(nat.NativeError, match="sums must be NULL"):
            ctx._check(ctx._lib.nsfem_dynamic_constant(ctx._h, nat.U1, nat._dp(np.empty(dm.n_p1)),
                                                       nat._dp(np.empty(2)), None))
        for slot in (nat.P, nat.CONV_N1):
            with pytest.raises(nat.NativeError, match="slot"):
                ctx.dynamic_lagrangian_advance(slot, 0.1)
        for bad in (0.0, -0.1, np.nan):
            with pytest.raises(nat.NativeError, match="step size"):
                ctx.dynamic_lagrangian_advance(nat.U1, bad)
        half = np.full((dm.n_p1, 4), NAN)
        half[: dm.n_p1 // 2, :2] = 1.0
        with pytest.raises(nat.NativeError, match="NaN for every vertex"):
            ctx.set_dynamic_lagrangian_state(half)
        with pytest.raises(nat.NativeError, match="I_MM"):
            ctx.set_dynamic_lagrangian_state(_state4(np.tile([0.1, -1.0], (dm.n_p1, 1))))
        # setting the groups or the law anew returns to mode 0
        ctx.set_dynamic_groups(1, np.zeros(dm.n_p1, dtype=np.int32))
        assert not ctx.dynamic_lagrangian_info()["active"]
        ctx.set_dynamic_averaging(1)
        ctx.set_viscosity_law(DYNAMIC, (2.0, 0.09))
        assert not ctx.dynamic_lagrangian_info()["active"]
        ctx.set_dynamic_averaging(1)
        # the other step calls
        ctx.set_coeffs(1.0, 1.0, 0.01)
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        ctx.set_bdf((1.0, -1.0, 0.0), 1.0 / 16.0)
        with pytest.raises(nat.NativeError, match="variable viscosity"):
            ctx.step_ipcs()
        with pytest.raises(nat.NativeError, match="variable viscosity"):
            ctx.step_bdf()
    finally:
        ctx.close()
    group = nat.local_group_create(1)
    ctx = make(mesh, dm)
    try:
        ctx.attach_local_comm(group, 0)
        with pytest.raises(nat.NativeError, match="communicator"):
            ctx.set_dynamic_averaging(1)
        assert ctx.dynamic_info()["bytes"] == 0
    finally:
        ctx.close()
        nat.local_group_destroy(group)


def test_imex_solver_with_the_lagrangian_model_equals_driving_the_steps_by_hand(monkeypatch):
    """IMEXIPCSSolver through InstationaryProblem.solve_problem with DynamicSmagorinskyModel(averaging="lagrangian") on
    the 8 x 8 cavity, 3 steps: u, p and the Lagrangian state are bit for bit what the C ABI gives on a second context;
    _compute_model_constant returns the stored vertex field"""
    from multigrid import attach_hierarchy
    from ns_imex_solver import IMEXIPCSSolver
    from problem_specs import build_problem
    steps, dt = _SPEC["clock"]["steps"], _SPEC["clock"]["dt"]
    model = DynamicSmagorinskyModel(averaging="lagrangian", relaxation=1.5, cs2_init=0.0256, filter_ratio=2.0, cs2_max=0.09)
    monkeypatch.setenv("NSFEM_NO_OUTPUT", "1")
    problem = build_problem(dict(_SPEC))

    problem.set_viscosity_model = lambda: setattr(problem, "_viscosity_model", model)     # (this instance alone)
    problem.set_solver_class(IMEXIPCSSolver)
    problem.compute_cfl = False
    problem.solve_problem()
    solver = problem._get_solver()
    cctx = solver._ctx
    assert cctx.viscosity_info()["law"] == DYNAMIC and cctx.viscosity_info()["recomputed"] == 0
    assert cctx.dynamic_lagrangian_info()["active"] and cctx.dynamic_info()["runs"] == steps
    u_cls, p_cls, state_cls = cctx.get_state(nat.U1), cctx.get_state(nat.P_OLD), solver.dynamic_lagrangian_state()
    # the solver-level restore: refused while no Lagrangian model is active, and a round trip keeps the bytes
    solver.set_dynamic_lagrangian_state(np.where(np.isnan(state_cls), state_cls, 0.5 * state_cls))
    assert not np.array_equal(solver.dynamic_lagrangian_state()[:, :2], state_cls[:, :2])
    solver.set_dynamic_lagrangian_state(state_cls)
    assert solver.dynamic_lagrangian_state().tobytes() == state_cls.tobytes()
    constant = problem._compute_model_constant()
    dm, mesh = solver._dofmap, solver._mesh
    assert constant.shape == (dm.n_p1, ) and np.array_equal(constant, state_cls[:, 3]) and constant.max() > 0.0
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
        ctx.set_dynamic_averaging(1, *model.averaging_params())
        opts = solver._step_options()
        ts = IMEXTimeStepping(0.0, 1.0, IMEXType.SBDF2, desired_start_time_step=dt)
        for _ in range(steps):
            _step(ctx, ts, opts)
        u_abi, p_abi, state_abi = ctx.get_state(nat.U1), ctx.get_state(nat.P_OLD), ctx.dynamic_lagrangian_state()
    finally:
        ctx.close()
    assert np.abs(u_cls).max() > 0.5
    assert np.array_equal(u_cls, u_abi) and np.array_equal(p_cls, p_abi) and state_cls.tobytes() == state_abi.tobytes()
    solver.set_viscosity_model(DynamicSmagorinskyModel("global"))
    with pytest.raises(RuntimeError, match="lagrangian"):
        solver.set_dynamic_lagrangian_state(state_cls)
