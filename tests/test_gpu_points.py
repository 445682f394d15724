"""Point location, point evaluation and tracer particles on the device (csrc/points.hip: k_locate_points<2|3>,
k_eval_points<2|3>, k_advect_tracers<2|3>) against host code that is not under test: the brute-force cell search and
the basis of ``fem_spaces.evaluate_lagrange``, closed forms, and a numpy RK4 on analytic velocity fields.

Tolerances.  Evaluation: 1e-13 x max|nodal values|, the project's figure for a kernel against the oracle.  Tracer
positions: 1e-12 absolute -- 64 substeps x 4 stages x about 20 roundings of 2^-53 at unit magnitude are 6e-13 if every
rounding adds.

Two calls of ``tracers_advect`` with n_sub = 4 over dt / 2 do NOT equal one call with n_sub = 8 over dt in a blended
field: theta runs from 0 to 1 within each call.  (Documented, not asserted.)"""
import types

import numpy as np
import pytest

import _native as nat
from fem_spaces import evaluate_lagrange
from gpu_common import context
from periodic_meshes import CHANNELS, far_images, lengths_of, periodic_axes, periodic_fields, periodic_fixture
from point_locator import barycentric, build_bins
from test_point_locator_host import MESHES, brute_force, brute_force_cells, mesh_of, point_sets
from test_volume_functionals_host import smooth_fields

pytestmark = pytest.mark.gpu
EVAL_TOL = 1e-13
PATH_TOL = 1e-12
PAIRS = {2: ((1, 2), (0, 2), (0, 1)), 3: ((2, 3), (1, 3), (1, 2), (0, 3), (0, 2), (0, 1))}


def _context(name, locator=True):
    mesh, dm = mesh_of(name)
    ctx = context(mesh, dm)
    if locator:
        ctx.set_point_locator(**build_bins(mesh.coords, mesh.cells))
    return mesh, dm, ctx


def _all_slots(ctx):
    return [ctx.get_state(slot) for slot in range(11)]


# ---------------------------------------------------------------- 1: location
@pytest.mark.parametrize("name", MESHES)
def test_cells_equal_the_brute_force_search(name):
    mesh, dm, ctx = _context(name)
    for label, X in point_sets(name).items():
        want = brute_force(name, label)               # asserts that the ambiguity band is empty for this set
        got = ctx.locate_points(X)
        assert got.dtype == np.int32 and got.shape == (X.shape[0], )
        bad = np.nonzero(got != want)[0]
        print("%s / %s: %d points, %d outside, %d differ" % (name, label, X.shape[0], int((want < 0).sum()), bad.size))
        assert bad.size == 0, (name, label, bad[:10], got[bad[:10]], want[bad[:10]])
    assert np.array_equal(ctx.locate_points(np.full((3, dm.dim), np.nan)), np.full(3, -1))
    ctx.close()


# ---------------------------------------------------------------- 2: evaluation
def _lagrange_at(dm, field, values, X, cells):
    """evaluate_lagrange's arithmetic (LU solve for the reference coordinates, its basis and local numbering) in the
    GIVEN cells; NaN where the cell is -1"""
    mesh, dim = dm.mesh, dm.dim
    ok = cells >= 0
    c = cells[ok].astype(np.int64)
    x = mesh.coords[mesh.cells.astype(np.int64)[c]]
    J = np.transpose(x[:, 1:] - x[:, :1], (0, 2, 1))
    ref = np.linalg.solve(J, (X[ok] - x[:, 0])[:, :, None])[:, :, 0]
    l = np.concatenate([1.0 - ref.sum(axis=1, keepdims=True), ref], axis=1)
    values = np.asarray(values)
    if field == "pressure":
        res = np.einsum("mk,mk->m", l, values[np.asarray(dm.p1_dofmap)[c]])
        out = np.full(X.shape[0], np.nan)
    else:
        N = np.concatenate([l * (2.0 * l - 1.0)] + [4.0 * l[:, [a]] * l[:, [b]] for a, b in PAIRS[dim]], axis=1)
        nodes = np.asarray(dm.p2_dofmap)[c]
        if field == "scalar":
            res = np.einsum("mk,mk->m", N, values[nodes])
            out = np.full(X.shape[0], np.nan)
        else:
            res = np.einsum("mk,mka->ma", N, values.reshape(-1, dim)[nodes])
            out = np.full((X.shape[0], dim), np.nan)
    out[ok] = res
    return out


def _smooth_scalar(X2):
    z = X2[:, 2] if X2.shape[1] == 3 else 0.0
    return np.cos(3.3 * X2[:, 0] - 0.7) * np.sin(4.4 * X2[:, 1] + 0.2) + 0.4 * np.sin(2.9 * z + X2[:, 0])


def _check_field(label, got, want, scale, cells):
    assert got.shape == want.shape
    out = cells < 0
    assert np.isnan(got[out]).all() and not np.isnan(got[~out]).any()
    err = float(np.abs(got[~out] - want[~out]).max()) if (~out).any() else 0.0
    print("%s: %d points, max error %.3e = %.2e x max|nodal values|" % (label, cells.size, err, err / scale))
    assert err <= EVAL_TOL * scale, (label, err, scale)


@pytest.mark.parametrize("name", MESHES)
def test_values_equal_evaluate_lagrange(name):
    mesh, dm, ctx = _context(name)
    ctx.set_scalar(0.01)
    u, p = smooth_fields(dm.p2_coords, dm.p1_coords)
    T = _smooth_scalar(dm.p2_coords)
    fields = (("velocity", nat.U0, u.ravel()), ("pressure", nat.P, p), ("scalar", nat.T0, T),
              ("velocity", nat.USTAR, -0.5 * u.ravel()), ("pressure", nat.P2_OLD, 3.0 * p), ("scalar", nat.T2, 2.0 * T))
    for _, slot, values in fields:
        ctx.set_state(slot, values)
    before = _all_slots(ctx)
    rng = np.random.default_rng(17)
    for label, X in point_sets(name).items():
        cells = brute_force(name, label)
        for field, slot, values in fields:
            scale = float(np.abs(values).max())
            got = ctx.eval_points(slot, X)
            _check_field("%s / %s / %s" % (name, label, field), got, _lagrange_at(dm, field, values, X, cells), scale,
                         cells)
            # the restatement above IS evaluate_lagrange on a sample of the points (it searches all cells itself)
            inside = np.nonzero(cells >= 0)[0]
            for i in rng.permutation(inside)[:8]:
                want = evaluate_lagrange(dm, field, values, X[i])
                assert np.abs(got[i] - want).max() <= EVAL_TOL * scale
            # cells handed over: the same bytes as locating inside the call; a second call: the same bytes again
            assert ctx.eval_points(slot, X, cells=ctx.locate_points(X)).tobytes() == got.tobytes()
            assert ctx.eval_points(slot, X).tobytes() == got.tobytes()
            # -1 cells give NaN, whatever the point
            if X.shape[0]:
                forced = cells.copy()
                forced[::2] = -1
                part = ctx.eval_points(slot, X, cells=forced)
                assert np.isnan(part[::2]).all() and part[1::2].tobytes() == got[1::2].tobytes()
    for a, b in zip(before, _all_slots(ctx)):
        assert a.tobytes() == b.tobytes()
    ctx.close()


@pytest.mark.parametrize("name", CHANNELS)
def test_values_in_the_seam_cells_of_periodic_channels(name):
    """pchan2 / pchan3 of tests/periodic_meshes.py: three points strictly inside every cell that reads a dof across the
    seam (its vertex lies a period away from the coordinates stored for the dof).  The device finds the cell, and
    velocity, pressure and scalar there equal evaluate_lagrange's arithmetic in that cell and evaluate_lagrange itself:
    the nodal values come through the identified dofs, the geometry from the cell"""
    mesh, dm, _ = periodic_fixture(name)
    dim = dm.dim
    seam = np.flatnonzero(far_images(name).any(axis=1))
    assert seam.size >= 2 * (dim + 1) and dm.n_p1 < mesh.num_vertices()
    rng = np.random.default_rng(29)
    lam = rng.uniform(0.15, 1.0, (3 * seam.size, dim + 1))
    lam /= lam.sum(axis=1, keepdims=True)
    cells = np.repeat(seam, 3).astype(np.int32)
    X = np.einsum("mk,mka->ma", lam, mesh.coords[mesh.cells.astype(np.int64)[cells]])
    u, T = periodic_fields(dm.p2_coords, lengths_of(name), periodic_axes(name))
    p = periodic_fields(dm.p1_coords, lengths_of(name), periodic_axes(name))[1]
    ctx = context(mesh, dm)
    try:
        ctx.set_point_locator(**build_bins(mesh.coords, mesh.cells))
        ctx.set_scalar(0.01)
        assert np.array_equal(ctx.locate_points(X), cells)
        for field, slot, values in (("velocity", nat.U0, u), ("pressure", nat.P, p), ("scalar", nat.T0, T)):
            ctx.set_state(slot, values)
            scale = float(np.abs(values).max())
            got = ctx.eval_points(slot, X)
            _check_field("%s / seam cells / %s" % (name, field), got, _lagrange_at(dm, field, values, X, cells), scale, cells)
            for i in rng.permutation(X.shape[0])[:8]:
                assert np.abs(got[i] - evaluate_lagrange(dm, field, values, X[i])).max() <= EVAL_TOL * scale
    finally:
        ctx.close()


@pytest.mark.parametrize("name", MESHES)
def test_quadratic_fields_are_reproduced(name):
    """P2 reproduces quadratic polynomials, P1 linear ones: the device value is the closed form"""
    mesh, dm, ctx = _context(name)
    ctx.set_scalar(0.0)
    dim = dm.dim

    def quad(X, k):
        x, y = X[:, 0], X[:, 1]
        z = X[:, 2] if dim == 3 else np.zeros_like(x)
        return (0.3 + k) + 0.7 * x - 1.1 * y + 0.5 * z + (0.9 - 0.2 * k) * x * x - 0.6 * x * y + 0.8 * y * y + \
            0.4 * z * z - 0.5 * y * z + 0.35 * x * z

    def lin(X):
        return 0.25 - 1.3 * X[:, 0] + 0.6 * X[:, 1] + (0.9 * X[:, 2] if dim == 3 else 0.0)

    u = np.stack([quad(dm.p2_coords, k) for k in range(dim)], axis=1)
    ctx.set_state(nat.U1, u.ravel())
    ctx.set_state(nat.T1, quad(dm.p2_coords, 5))
    ctx.set_state(nat.P_OLD, lin(dm.p1_coords))
    for label in ("random", "nodes", "centroids", "one"):
        X = point_sets(name)[label]
        cells = brute_force(name, label)
        _check_field(name + " / " + label + " / quadratic velocity", ctx.eval_points(nat.U1, X),
                     np.stack([quad(X, k) for k in range(dim)], axis=1), float(np.abs(u).max()), cells)
        _check_field(name + " / " + label + " / quadratic scalar", ctx.eval_points(nat.T1, X), quad(X, 5),
                     float(np.abs(quad(dm.p2_coords, 5)).max()), cells)
        _check_field(name + " / " + label + " / linear pressure", ctx.eval_points(nat.P_OLD, X), lin(X),
                     float(np.abs(lin(dm.p1_coords)).max()), cells)
    ctx.close()


# ---------------------------------------------------------------- 3, 4: tracers against a numpy RK4
def _rk4(field, X, dt, n_sub):
    """classical RK4 of dx/dt = field(x, theta), theta from 0 to 1 over dt; also every point the field was asked at"""
    X = X.copy()
    h = dt / n_sub
    asked = []

    def f(x, th):
        asked.append(x.copy())
        return field(x, th)

    for s in range(n_sub):
        th0, th1, th2 = s / n_sub, (s + 0.5) / n_sub, (s + 1) / n_sub
        k1 = f(X, th0)
        k2 = f(X + 0.5 * h * k1, th1)
        k3 = f(X + 0.5 * h * k2, th1)
        k4 = f(X + h * k3, th2)
        X = X + (h / 6.0) * ((k1 + 2.0 * k2) + (2.0 * k3 + k4))
    asked.append(X.copy())
    return X, np.concatenate(asked)


def _rotation(dim):
    centre = np.array([0.75, 0.5]) if dim == 2 else np.array([0.5, 0.5, 0.0])

    def a(X):
        out = np.zeros_like(X)
        out[:, 0] = -(X[:, 1] - centre[1])
        out[:, 1] = X[:, 0] - centre[0]
        return out
    return centre, a


def _circle_particles(dim, n=257, seed=23):
    centre, _ = _rotation(dim)
    rng = np.random.default_rng(seed)
    r = 0.4 * np.sqrt(rng.random(n))
    r[0] = 0.4
    phi = 2.0 * np.pi * rng.random(n)
    X = np.tile(centre, (n, 1))
    X[:, 0] += r * np.cos(phi)
    X[:, 1] += r * np.sin(phi)
    if dim == 3:
        X[:, 2] = 0.05 + 0.9 * rng.random(n)
    return X


def _assert_cells_contain(mesh, x, cells):
    assert (cells >= 0).all()
    lam = barycentric(mesh.coords, mesh.cells, cells.astype(np.int64), x)
    assert lam.min() >= -1.1e-12, lam.min()


@pytest.mark.parametrize("name", ["rectangle", "box"])
def test_rigid_rotation_against_numpy_rk4(name):
    mesh, dm, ctx = _context(name)
    _, a = _rotation(dm.dim)
    for slot in (nat.U0, nat.U1):
        ctx.set_state(slot, a(dm.p2_coords).ravel())           # P2 reproduces the linear field exactly
    X = _circle_particles(dm.dim)
    want, asked = _rk4(lambda x, th: a(x), X, 2.0 * np.pi, 64)
    assert (brute_force_cells(mesh, asked[:: 97])[0] >= 0).all()
    lo, hi = mesh.coords.min(axis=0), mesh.coords.max(axis=0)
    assert (asked > lo + 0.04).all() and (asked < hi - 0.04).all()           # every stage point well inside the box
    before = _all_slots(ctx)
    for begin, end in ((nat.U1, nat.U0), (nat.U0, nat.U0)):     # equal values in two slots, and the frozen field
        ctx.tracers_set(X)
        assert ctx.tracers_info() == dict(n=257, n_left=0, advect_calls=0, fallbacks=0)
        ctx.tracers_advect(begin, end, 2.0 * np.pi, 64)
        x, cells, status = ctx.tracers_get()
        info = ctx.tracers_info()
        err = float(np.abs(x - want).max())
        print("%s rotation (%d -> %d): max |x - numpy RK4| %.3e, after one turn %.3e from the start, %d bin searches "
              "for %d located points" % (name, begin, end, err, float(np.abs(x - X).max()), info["fallbacks"],
                                         257 * 64 * 4))
        assert err <= PATH_TOL
        assert not status.any() and info["n_left"] == 0 and info["advect_calls"] == 1
        _assert_cells_contain(mesh, x, cells)
    for p, q in zip(before, _all_slots(ctx)):
        assert p.tobytes() == q.tobytes()
    ctx.close()


def test_time_blended_quadratic_field_against_numpy_rk4():
    mesh, dm, ctx = _context("rectangle")
    _, a = _rotation(2)

    def extra(X):
        out = np.zeros_like(X)
        out[:, 0] = X[:, 1] * (1.0 - X[:, 1])
        return out

    ctx.set_state(nat.U1, a(dm.p2_coords).ravel())
    ctx.set_state(nat.U0, (2.0 * a(dm.p2_coords) + extra(dm.p2_coords)).ravel())
    X = _circle_particles(2, seed=29)
    dt, n_sub = 1.0, 8
    want, asked = _rk4(lambda x, th: (1.0 - th) * a(x) + th * (2.0 * a(x) + extra(x)), X, dt, n_sub)
    assert (asked[:, 0] > 0.02).all() and (asked[:, 0] < 1.48).all()         # the numpy paths stay inside 1.5 x 1
    assert (asked[:, 1] > 0.02).all() and (asked[:, 1] < 0.98).all()
    ctx.tracers_set(X)
    ctx.tracers_advect(nat.U1, nat.U0, dt, n_sub)
    x, cells, status = ctx.tracers_get()
    err = float(np.abs(x - want).max())
    print("blended field: max |x - numpy RK4| %.3e, moved up to %.3f" % (err, float(np.abs(x - X).max())))
    assert err <= PATH_TOL and not status.any()
    _assert_cells_contain(mesh, x, cells)
    # the blend matters: the frozen begin field ends elsewhere
    frozen, _ = _rk4(lambda x, th: a(x), X, dt, n_sub)
    assert np.abs(frozen - want).max() > 1e-2
    ctx.close()


# ---------------------------------------------------------------- 5: leaving
def test_a_particle_that_leaves_keeps_its_last_position():
    mesh, dm, ctx = _context("rectangle")
    flow = np.tile([1.0, 0.0], dm.n_p2)
    ctx.set_state(nat.U0, flow)
    ctx.set_state(nat.U1, flow)
    ctx.tracers_set(np.array([[0.2, 0.5], [1.42, 0.5]]))
    ctx.tracers_advect(nat.U1, nat.U0, 0.2, 4)
    x, cells, status = ctx.tracers_get()
    print("leaving: positions %r status %r" % (x.tolist(), status.tolist()))
    assert status.tolist() == [0, 1]
    assert np.abs(x - [[0.4, 0.5], [1.47, 0.5]]).max() <= 1e-14      # the last stage of the second substep is at 1.52
    assert ctx.tracers_info()["n_left"] == 1
    _assert_cells_contain(mesh, x, cells)
    ctx.tracers_advect(nat.U1, nat.U0, 0.2, 4)
    x2, cells2, status2 = ctx.tracers_get()
    assert x2[1].tobytes() == x[1].tobytes() and cells2[1] == cells[1] and status2.tolist() == [0, 1]
    assert abs(x2[0, 0] - 0.6) <= 1e-14
    info = ctx.tracers_info()
    assert info["n"] == 2 and info["n_left"] == 1 and info["advect_calls"] == 2
    # a particle set outside the mesh has left from the start
    ctx.tracers_set(np.array([[0.2, 0.5], [1.6, 0.5], [np.nan, 0.0]]))
    assert ctx.tracers_get()[2].tolist() == [0, 1, 1] and ctx.tracers_info()["n_left"] == 2
    ctx.tracers_set(np.zeros((0, 2)))                                 # an empty cloud is valid
    ctx.tracers_advect(nat.U1, nat.U0, 0.2, 4)
    assert ctx.tracers_get()[0].shape == (0, 2) and ctx.tracers_info()["n"] == 0
    ctx.close()


@pytest.mark.parametrize("name", CHANNELS)
def test_a_particle_driven_through_a_periodic_side_has_left(name):
    """tracers know the mesh, not the dof map: a periodic side is a side (include/nsfem.h).  Uniform flow along x in a
    periodic channel: the particle that reaches x = L ends with status 1 at its last position inside the mesh and does
    not come back in at x = 0; the other one goes on"""
    mesh, dm, _ = periodic_fixture(name)
    dim = dm.dim
    L = lengths_of(name)
    flow = np.tile([1.0, 0.0, 0.0][:dim], dm.n_p2)
    mid = [0.43 * l for l in L[1:]]
    ctx = context(mesh, dm)
    try:
        ctx.set_point_locator(**build_bins(mesh.coords, mesh.cells))
        ctx.set_state(nat.U0, flow)
        ctx.set_state(nat.U1, flow)
        ctx.tracers_set(np.array([[0.2] + mid, [L[0] - 0.08] + mid]))
        ctx.tracers_advect(nat.U1, nat.U0, 0.2, 4)
        x, cells, status = ctx.tracers_get()
        print("%s: positions %r status %r" % (name, x.tolist(), status.tolist()))
        assert status.tolist() == [0, 1] and ctx.tracers_info()["n_left"] == 1
        # (the last stage of the second substep is at L + 0.02: one substep of 0.05 was taken)
        assert np.abs(x - np.array([[0.4] + mid, [L[0] - 0.03] + mid])).max() <= 1e-14
        _assert_cells_contain(mesh, x, cells)
        ctx.tracers_advect(nat.U1, nat.U0, 0.2, 4)
        x2, cells2, status2 = ctx.tracers_get()
        assert x2[1].tobytes() == x[1].tobytes() and cells2[1] == cells[1] and status2.tolist() == [0, 1]
        assert abs(x2[0, 0] - 0.6) <= 1e-14
    finally:
        ctx.close()


def test_a_particle_driven_into_the_hole_of_the_shell_stops_inside_the_mesh():
    mesh, dm, ctx = _context("shell")
    inwards = -np.array(dm.p2_coords)                                 # u = -x: |x(t)| = |x(0)| exp(-t)
    ctx.set_state(nat.U0, inwards.ravel())
    d = np.array([[0.3, -0.5, 0.81], [-0.6, 0.2, 0.3]])
    X = 0.6 * d / np.linalg.norm(d, axis=1, keepdims=True)
    ctx.tracers_set(X)
    assert ctx.tracers_info()["n_left"] == 0
    ctx.tracers_advect(nat.U0, nat.U0, 1.0, 16)                       # radius 0.4 is reached at t = log(1.5) = 0.405
    x, cells, status = ctx.tracers_get()
    r = np.linalg.norm(x, axis=1)
    print("shell: final radii %r status %r" % (r.tolist(), status.tolist()))
    assert status.tolist() == [1, 1] and ctx.tracers_info()["n_left"] == 2
    assert (r < 0.5).all() and (r > 0.35).all()
    assert (brute_force_cells(mesh, x)[0] >= 0).all()
    _assert_cells_contain(mesh, x, cells)
    ctx.close()


# ---------------------------------------------------------------- 6: refusals
def test_refusals():
    def refused(call):
        with pytest.raises(nat.NativeError) as e:
            call()
        assert e.value.code == nat.ERR_ARG

    mesh, dm, ctx = _context("rectangle", locator=False)
    u, p = smooth_fields(dm.p2_coords, dm.p1_coords)
    ctx.set_state(nat.U0, u.ravel())
    ctx.set_state(nat.P, p)
    before = _all_slots(ctx)
    X = point_sets("rectangle")["centroids"]
    # no locator
    refused(lambda: ctx.locate_points(X))
    refused(lambda: ctx.eval_points(nat.U0, X))
    refused(lambda: ctx.eval_points(nat.U0, X, cells=np.zeros(X.shape[0], np.int32)))
    refused(lambda: ctx.tracers_set(X))
    # lists that do not fit the mesh
    bins = build_bins(mesh.coords, mesh.cells)
    bad = dict(bins, bin_cells=np.where(np.arange(bins["bin_cells"].size) == 3, mesh.num_cells(), bins["bin_cells"]))
    refused(lambda: ctx.set_point_locator(**bad))
    refused(lambda: ctx.locate_points(X))
    ctx.set_point_locator(**bins)
    assert (ctx.locate_points(X) >= 0).all()
    # slots that hold no state field, a temperature slot without a scalar
    for slot in (nat.TRACTION, nat.BODY_FORCE, nat.CONV_N1, nat.T_SOURCE, nat.TCONV_1, -1, 17):
        refused(lambda: ctx._check(ctx._lib.nsfem_eval_points(ctx._h, slot, 1, nat._dp(X), None,
                                                              nat._dp(np.zeros(2)))))
    refused(lambda: ctx.eval_points(nat.T0, X))
    # n < 0
    refused(lambda: ctx._check(ctx._lib.nsfem_locate_points(ctx._h, -1, nat._dp(X), nat._ip(np.zeros(1, np.int32)))))
    refused(lambda: ctx._check(ctx._lib.nsfem_tracers_set(ctx._h, -1, nat._dp(X))))
    # advect: before tracers_set, n_sub = 0, dt not finite, slots that are no velocity
    refused(lambda: ctx.tracers_advect(nat.U0, nat.U0, 0.1, 1))
    ctx.tracers_set(X)
    refused(lambda: ctx.tracers_advect(nat.U0, nat.U0, 0.1, 0))
    refused(lambda: ctx.tracers_advect(nat.U0, nat.U0, np.inf, 1))
    refused(lambda: ctx.tracers_advect(nat.U0, nat.U0, np.nan, 1))
    refused(lambda: ctx.tracers_advect(nat.U0, nat.P, 0.1, 1))
    refused(lambda: ctx.tracers_advect(nat.TRACTION, nat.U0, 0.1, 1))
    x, _, status = ctx.tracers_get()
    assert x.tobytes() == X.tobytes() and not status.any()            # no refused call moved a particle
    # n = 0 is valid
    assert ctx.locate_points(np.zeros((0, 2))).shape == (0, )
    assert ctx.eval_points(nat.U0, np.zeros((0, 2))).shape == (0, 2) and ctx.eval_points(nat.P, np.zeros((0, 2))).shape == (0, )
    # a context with a communicator
    group = nat.local_group_create(1)
    ctx.attach_local_comm(group, 0)
    refused(lambda: ctx.set_point_locator(**bins))
    refused(lambda: ctx.locate_points(X))
    refused(lambda: ctx.eval_points(nat.U0, X))
    refused(lambda: ctx.tracers_set(X))
    refused(lambda: ctx.tracers_advect(nat.U0, nat.U0, 0.1, 1))
    for a, b in zip(before, _all_slots(ctx)):
        assert a.tobytes() == b.tobytes()
    ctx.close()
    nat.local_group_destroy(group)


# ---------------------------------------------------------------- 7: the surface
def _cavity(steps):
    from problem_specs import build_problem
    return build_problem(dict(
        name="Cavity", mesh=("cube", 2, 16), scheme="ipcs", numbers=dict(Re=100.0),
        clock=dict(dt=0.01, steps=steps), start={"velocity": (0.0, 0.0), "pressure": 0.0},
        bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_slip", "bottom"), ("velocity", "top", (1.0, 0.0))]))


def _fields(solver):
    return [solver._ctx.get_state(s) for s in (nat.U0, nat.U1, nat.U2, nat.P, nat.P_OLD)]


def test_problem_loop_equals_driving_the_c_abi_by_hand():
    rng = np.random.default_rng(31)
    Xt = 0.05 + 0.9 * rng.random((300, 2))
    Xt[:3] = [[0.5, 0.9999], [0.999, 0.99], [0.3, 0.98]]              # next to the moving lid
    Xp = np.array([[0.5, 0.5], [0.5, 0.95], [0.1, 0.9], [1.5, 0.5]])  # the last one lies outside
    # through InstationaryProblem
    problem = _cavity(4)
    cloud = problem._add_tracer_cloud(Xt)
    probes = problem._add_point_probes(Xp)
    problem.solve_problem()
    solver = problem._get_solver()
    series = probes.series()
    assert series["time"].shape == (4, ) and np.allclose(series["time"], [0.01, 0.02, 0.03, 0.04])
    assert series["velocity"].shape == (4, 4, 2) and series["pressure"].shape == (4, 4)
    assert set(series) == {"time", "velocity", "pressure"}
    assert np.isnan(series["velocity"][:, 3]).all() and not np.isnan(series["velocity"][:, :3]).any()
    assert probes.cells[3] == -1
    assert cloud.info()["advect_calls"] == 4
    moved = np.abs(cloud.positions() - Xt).max()
    assert 1e-4 < moved < 0.05, moved
    # DeviceFunction.eval_points is ctx.eval_points
    velocity, pressure = solver.solution.split()
    assert velocity.eval_points(Xp).tobytes() == solver._ctx.eval_points(nat.U0, Xp).tobytes()
    assert pressure.eval_points(Xt).tobytes() == solver._ctx.eval_points(nat.P, Xt).tobytes()
    assert cloud.sample(velocity).tobytes() == solver._ctx.eval_points(nat.U0, cloud.positions()).tobytes()
    assert np.abs(velocity.eval_points(Xp[:1])[0] - velocity(Xp[0])).max() <= EVAL_TOL      # the host path it replaces
    # by hand: the same set-up with an empty time loop, then solve / tracers_advect / eval_points / advance
    hand = _cavity(4)
    hand._n_max_steps = 0
    hand.solve_problem()
    hs, ts = hand._get_solver(), hand._time_stepping
    ctx = hs._ctx
    ctx.set_point_locator(**build_bins(hs._mesh.coords, hs._mesh.cells))
    ctx.tracers_set(Xt)
    cells = ctx.locate_points(Xp)
    rec_u, rec_p = [], []
    for _ in range(4):
        hand._set_next_step_size()
        ts.update_coefficients()
        dt = ts.get_next_step_size()
        hs.solve()
        ctx.tracers_advect(nat.U1, nat.U0, dt, 1)
        rec_u.append(ctx.eval_points(nat.U0, Xp, cells))
        rec_p.append(ctx.eval_points(nat.P, Xp, cells))
        ts.advance_time()
        hs.advance_time()
    x, _, status = ctx.tracers_get()
    assert cloud.positions().tobytes() == x.tobytes() and cloud.status().tobytes() == status.tobytes()
    assert series["velocity"].tobytes() == np.stack(rec_u).tobytes()
    assert series["pressure"].tobytes() == np.stack(rec_p).tobytes()
    # the tracers only read: the fields equal those of a run without registrations, and of the run by hand
    plain = _cavity(4)
    plain.solve_problem()
    for a, b, c in zip(_fields(solver), _fields(plain._get_solver()), _fields(hs)):
        assert a.tobytes() == b.tobytes() == c.tobytes()
    assert not hasattr(plain._get_solver(), "_point_locator_ready")   # nothing registered: no locator was built


def test_two_clouds_share_the_device_storage_of_one_context():
    mesh, dm, ctx = _context("rectangle", locator=False)
    flow = np.tile([1.0, 0.0], dm.n_p2)
    ctx.set_state(nat.U0, flow)
    ctx.set_state(nat.U1, flow)
    from tracers import PointProbes, TracerCloud
    solver = types.SimpleNamespace(_ctx=ctx, _mesh=mesh, _next_step_size=0.2)
    A = TracerCloud(solver, [[0.2, 0.5], [1.42, 0.5]])
    B = TracerCloud(solver, [[0.1, 0.3], [0.3, 0.7], [1.49, 0.1]])
    for _ in range(2):
        A.advect(substeps=4)
        B.advect(substeps=4)
    assert A.status().tolist() == [0, 1] and B.status().tolist() == [0, 0, 1]
    assert np.abs(A.positions() - [[0.6, 0.5], [1.47, 0.5]]).max() <= 1e-14
    assert np.abs(B.positions() - [[0.5, 0.3], [0.7, 0.7], [1.49, 0.1]]).max() <= 1e-14
    assert A.n_left == 1 and B.n_left == 1
    probes = PointProbes(solver, [[0.4, 0.4], [2.0, 0.0]])
    s = probes.sample()
    assert np.array_equal(s["velocity"][0], [1.0, 0.0]) and np.isnan(s["velocity"][1]).all() and "temperature" not in s
    ctx.close()
