"""Running flow statistics on the device (csrc/statistics.hip: k_stats_update<2|3, scalar>, k_stats_profile,
k_stats_gather; nsfem_stats_*) against the numpy restatement pinned in tests/test_flow_statistics_host.py and against
two-pass numpy, and the callers: ``FlowStatistics`` and ``ProblemBase._add_flow_statistics``.

Tolerances (derived, not measured).  Node statistics: 1e-12 relative to max|x| (means) and to (max|x|)^2 (second
moments), max|x| over all samples of the variables involved -- every update commits a handful of roundings of that
size, 16 samples x about 8 x 2^-53 is roughly 1.5e-14, a factor of 50 or more below the bound.  Profiles: 1e-12
relative to the sum of the absolute contributions of the group (the rule of the volume functionals' tests: the worst
case of a recursive sum over <= 4096 terms is terms x 2^-53, doubled for the restatement's own rounding)."""
import os

import numpy as np
import pytest

import _native as nat
from fem_mesh import TaylorHoodDofMap, box_mesh, rectangle_mesh
from general_tet_mesh import CUBE, SMALL, general_tets
from gpu_common import context
from periodic_meshes import periodic_fixture
from test_flow_statistics_host import (WEIGHTS, RunningStats, columns, periodic_square, pooled_profiles, two_pass)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-12
Q_P2 = (nat.STATS_MEAN_U, nat.STATS_COV_U, nat.STATS_TKE)
Q_P1 = (nat.STATS_MEAN_P, nat.STATS_VAR_P)
Q_T = (nat.STATS_MEAN_T, nat.STATS_VAR_T, nat.STATS_FLUX_UT)


def _mesh(name):
    from mesh_io import read_msh
    if name == "rect6x4":            # 117 P2 nodes: fewer than two waves, odd tail
        mesh = rectangle_mesh((0.0, 0.0), (1.5, 1.0), 6, 4)
    elif name == "rect24x16":        # 1617 P2 nodes: several workgroups, the P2 / P1 split of the grid
        mesh = rectangle_mesh((0.0, 0.0), (1.5, 1.0), 24, 16)
    elif name == "rect160x2":        # lines of 321 nodes (> the 256 threads of a workgroup) and of 5 nodes
        mesh = rectangle_mesh((0.0, 0.0), (8.0, 0.1), 160, 2)
    elif name == "box3x2x2":         # 175 P2 nodes, 3D: 24-byte node stride
        mesh = box_mesh((0.0, 0.0, 0.0), (1.5, 1.0, 1.0), 3, 2, 2)
    elif name == "box4x4x4":         # 729 P2 nodes
        mesh = box_mesh((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 4, 4, 4)
    elif name == "fixture":
        mesh = read_msh(os.path.join(HERE, "golden", "square_v41.msh"))[0]
    elif name == "periodic":
        return periodic_square(8)
    elif name == "pchan3":                       # the 3D periodic channel of tests/periodic_meshes.py: 180 P2 nodes and
        return periodic_fixture(name)[:2]        # 27 P1 nodes on 48 mesh vertices
    elif name in ("general72", "general384"):    # the general tetrahedra of tests/general_tet_mesh.py: the node and
        return general_tets(*(SMALL if name == "general72" else CUBE))[:2]   # vertex numbering of a renumbered mesh
    else:
        raise ValueError(name)
    return mesh, TaylorHoodDofMap(mesh)


EXPECTED_NODES = dict(pchan3=180, rect6x4=117, rect24x16=1617, box3x2x2=175, box4x4x4=729, general72=175, general384=729)
_CACHE = {}


def fields(X2, X1, k):
    """smooth, distinct sample k: (u [n2, dim], T [n2], p [n1])"""
    dim = X2.shape[1]
    x, y = X2[:, 0], X2[:, 1]
    z = X2[:, 2] if dim == 3 else np.zeros_like(x)
    # (the steady 0.8 sin(0.9 x): the time mean of u_x varies along a line of constant y)
    u = [np.sin(1.3 * x + 0.7 * k) * np.cos(0.9 * y + 0.2 * k) + 0.1 * k + 0.3 * z + 0.8 * np.sin(0.9 * x),
         np.cos(0.8 * x - 0.4 * k) * (1.0 + y) + 0.5 * np.sin(1.0 * k) - 0.2 * z * z]
    if dim == 3:
        u.append(np.sin(x + y + z + 0.3 * k) - 0.25)
    T = 1.0 + 0.5 * np.cos(1.1 * x + 0.5 * k) * np.sin(0.7 * y - 0.3 * k) + 0.2 * z + 0.05 * k
    x1, y1 = X1[:, 0], X1[:, 1]
    p = np.sin(0.6 * x1 + 0.9 * k) + y1 * np.cos(0.5 * k) + (0.3 * X1[:, 2] if dim == 3 else 0.0)
    return np.stack(u, axis=1), T, p


def reference(name):
    """mesh, dof map, the 8 samples and both host references, computed once per mesh and left unchanged"""
    if name not in _CACHE:
        mesh, dm = _mesh(name)
        if name in EXPECTED_NODES:
            assert dm.n_p2 == EXPECTED_NODES[name]
        S = [fields(dm.p2_coords, dm.p1_coords, k) for k in range(len(WEIGHTS))]
        X2 = np.stack([np.concatenate([u, T[:, None]], axis=1) for u, T, _ in S])       # [k, n2, dim + 1]
        X1 = np.stack([p[:, None] for _, _, p in S])
        rs2, rs1 = RunningStats(), RunningStats()
        for k, w in enumerate(WEIGHTS):
            rs2.update(X2[k], w)
            rs1.update(X1[k], w)
        _CACHE[name] = dict(mesh=mesh, dm=dm, samples=S, X2=X2, X1=X1, run2=(rs2.m, rs2.covariance()),
                            run1=(rs1.m, rs1.covariance()), two2=two_pass(X2, WEIGHTS), two1=two_pass(X1, WEIGHTS))
    return _CACHE[name]


def feed(ref, scalar, pressure=True, weights=WEIGHTS):
    """a fresh context with the samples of ``ref`` taken"""
    dm = ref["dm"]
    ctx = context(ref["mesh"], dm)
    if scalar:
        ctx.set_scalar(0.01)
    ctx.stats_enable(nat.STATS_VELOCITY | (nat.STATS_PRESSURE if pressure else 0) | (nat.STATS_SCALAR if scalar else 0))
    for (u, T, p), w in zip(ref["samples"], weights):
        ctx.set_state(nat.U0, u.ravel())
        ctx.set_state(nat.P, p)
        if scalar:
            ctx.set_state(nat.T0, T)
        ctx.stats_sample(nat.U0, nat.P if pressure else -1, nat.T0 if scalar else -1, w)
    return ctx


def expected(quantity, m, cov, dim):
    """the quantity from means [n, nv] and covariances [n, nv, nv] of the variables (u, T) or (p)"""
    if quantity in (nat.STATS_MEAN_U, ):
        return m[:, :dim]
    if quantity == nat.STATS_COV_U:
        return np.stack([cov[:, i, j] for i in range(dim) for j in range(i, dim)], axis=1)
    if quantity == nat.STATS_TKE:
        return 0.5 * sum(cov[:, i, i] for i in range(dim))
    if quantity in (nat.STATS_MEAN_P, ):
        return m[:, 0]
    if quantity == nat.STATS_VAR_P:
        return cov[:, 0, 0]
    if quantity == nat.STATS_MEAN_T:
        return m[:, dim]
    if quantity == nat.STATS_VAR_T:
        return cov[:, dim, dim]
    if quantity == nat.STATS_FLUX_UT:
        return cov[:, :dim, dim]
    raise ValueError(quantity)


def scale_of(quantity, ref):
    dim = ref["dm"].dim
    umax, tmax, pmax = np.abs(ref["X2"][:, :, :dim]).max(), np.abs(ref["X2"][:, :, dim]).max(), np.abs(ref["X1"]).max()
    return {nat.STATS_MEAN_U: umax, nat.STATS_COV_U: umax ** 2, nat.STATS_TKE: umax ** 2, nat.STATS_MEAN_P: pmax,
            nat.STATS_VAR_P: pmax ** 2, nat.STATS_MEAN_T: tmax, nat.STATS_VAR_T: tmax ** 2,
            nat.STATS_FLUX_UT: max(umax, tmax) ** 2}[quantity]


def compare_nodes(ctx, ref, scalar, label):
    dim = ref["dm"].dim
    worst = 0.0
    checks = []
    for q in Q_P2 + Q_P1 + (Q_T if scalar else ()):
        got = ctx.stats_get(q)
        for kind, (m2, c2), (m1, c1) in (("running", ref["run2"], ref["run1"]), ("two-pass", ref["two2"], ref["two1"])):
            want = expected(q, m1, c1, 1) if q in Q_P1 else expected(q, m2, c2, dim)
            assert got.shape == want.shape
            err = np.abs(got - want).max() / scale_of(q, ref)
            worst = max(worst, err)
            print("%s quantity %d vs %-8s max error / scale %.3e" % (label, q, kind, err))
            checks.append((q, kind, err))
    for q, kind, err in checks:
        assert err <= TOL, (label, q, kind, err)
    return worst


CASES = [("rect6x4", True), ("rect6x4", False), ("rect24x16", True), ("rect160x2", False), ("box3x2x2", True),
         ("box3x2x2", False), ("box4x4x4", True), ("fixture", True), ("periodic", False), ("general72", True),
         ("general72", False), ("general384", True), ("pchan3", True), ("pchan3", False)]


@pytest.mark.parametrize("name,scalar", CASES)
def test_eight_weighted_samples_equal_the_restatement_and_two_pass_numpy(name, scalar):
    ref = reference(name)
    ctx = feed(ref, scalar)
    dm = ref["dm"]
    info = ctx.stats_info()
    ncol = dm.dim + dm.dim * (dm.dim + 1) // 2 + (2 + dm.dim if scalar else 0)
    assert info["samples"] == info["launches"] == len(WEIGHTS)                     # ONE launch per sample
    assert info["bytes"] == 8 * (ncol * (dm.n_p2 + dm.n_p2 % 2) + 2 * (dm.n_p1 + dm.n_p1 % 2))
    assert ctx.stats_weight() == sum(WEIGHTS)
    compare_nodes(ctx, ref, scalar, "%s%s" % (name, " +T" if scalar else ""))
    # the samples are read, never written
    u, T, p = ref["samples"][-1]
    assert ctx.get_state(nat.U0).tobytes() == u.ravel().tobytes() and ctx.get_state(nat.P).tobytes() == p.tobytes()
    ctx.close()


@pytest.mark.parametrize("name", ["rect6x4", "rect24x16", "box3x2x2", "general72"])
def test_first_sample_is_the_mean_bit_for_bit_and_a_constant_field_has_zero_moments(name):
    ref = reference(name)
    dm = ref["dm"]
    u, T, p = ref["samples"][3]
    ctx = context(ref["mesh"], dm)
    ctx.set_scalar(0.01)
    ctx.stats_enable(nat.STATS_VELOCITY | nat.STATS_PRESSURE | nat.STATS_SCALAR)
    for s, v in ((nat.U0, u.ravel()), (nat.P, p), (nat.T0, T)):
        ctx.set_state(s, v)

    def check():
        assert ctx.stats_get(nat.STATS_MEAN_U).tobytes() == u.tobytes()
        assert ctx.stats_get(nat.STATS_MEAN_P).tobytes() == p.tobytes()
        assert ctx.stats_get(nat.STATS_MEAN_T).tobytes() == T.tobytes()
        for q in (nat.STATS_COV_U, nat.STATS_TKE, nat.STATS_VAR_P, nat.STATS_VAR_T, nat.STATS_FLUX_UT):
            got = ctx.stats_get(q)
            assert got.tobytes() == np.zeros_like(got).tobytes(), q                # +0.0 everywhere

    ctx.stats_sample(nat.U0, nat.P, nat.T0, 0.7)
    check()
    for w in (1.0, 0.3, 2.0, 1.0):
        ctx.stats_sample(nat.U0, nat.P, nat.T0, w)
    assert ctx.stats_info()["samples"] == 5
    check()
    # enabling again starts over
    ctx.stats_enable(nat.STATS_VELOCITY | nat.STATS_PRESSURE | nat.STATS_SCALAR)
    assert ctx.stats_info()["samples"] == 0 and ctx.stats_weight() == 0.0
    ctx.set_state(nat.U0, 2.0 * u.ravel())
    ctx.stats_sample(nat.U0, nat.P, nat.T0, 1.0)
    assert ctx.stats_get(nat.STATS_MEAN_U).tobytes() == (2.0 * u).tobytes()
    ctx.close()


def test_velocity_only_allocates_less_and_refuses_the_pressure():
    ref = reference("rect24x16")
    dm = ref["dm"]
    ctx = feed(ref, scalar=False, pressure=False)
    full = feed(ref, scalar=False, pressure=True)
    small, big = ctx.stats_info(), full.stats_info()
    assert small["flags"] == nat.STATS_VELOCITY and big["flags"] == nat.STATS_VELOCITY | nat.STATS_PRESSURE
    assert small["bytes"] == 8 * 5 * (dm.n_p2 + 1) and big["bytes"] == small["bytes"] + 8 * 2 * (dm.n_p1 + dm.n_p1 % 2)
    for q in Q_P1 + Q_T:
        with pytest.raises(nat.NativeError, match="not enabled"):
            ctx.stats_get(q)
    for q in Q_P2:
        assert ctx.stats_get(q).tobytes() == full.stats_get(q).tobytes()
    # a context that never enables statistics holds nothing
    plain = context(ref["mesh"], dm)
    assert plain.stats_info() == dict(samples=0, flags=0, bytes=0, launches=0)
    plain.close()
    ctx.stats_enable(0)
    assert ctx.stats_info() == dict(samples=0, flags=0, bytes=0, launches=0)
    ctx.close()
    full.close()


def _hand_made_groups(n, rng):
    """every node as a group of its own, then 12 random groups with repeated nodes across groups and unequal weights"""
    ptr, nodes = list(range(n + 1)), list(range(n))
    for _ in range(12):
        nodes += rng.choice(n, size=int(rng.integers(2, min(40, n) + 1)), replace=False).tolist()
        ptr.append(len(nodes))
    return np.array(ptr, np.int32), np.array(nodes, np.int32), rng.uniform(0.25, 4.0, len(nodes))


def compare_profiles(ctx, ref, scalar, groups2, groups1, label):
    dim = ref["dm"].dim
    m2, c2 = ref["run2"]
    if not scalar:
        m2, c2 = m2[:, :dim], c2[:, :dim, :dim]
    out = {}
    for field, groups, (m, c), d in ((0, groups2, (m2, c2), dim), (1, groups1, ref["run1"], 1)):
        ptr, nodes, w = groups
        assert np.diff(ptr).max() <= 4096
        ctx.stats_set_groups(field, ptr, nodes, w)
        got = ctx.stats_profiles(field)
        want, scale, between = pooled_profiles(m, c, d, ptr, nodes, np.ones(len(nodes)) if w is None else w)
        assert got.shape == want.shape
        err = np.abs(got - want) / np.maximum(scale, 1e-300)
        print("%s field %d: %d groups (sizes %d .. %d), worst error / scale %.3e" %
              (label, field, len(ptr) - 1, np.diff(ptr).min(), np.diff(ptr).max(), err.max()))
        assert (np.abs(got - want) <= TOL * scale + 1e-300).all(), (label, field, err.max())
        out[field] = (got, want, between)
    return out


def _axis_groups(dm, axis):
    from flow_statistics import groups_along_axis
    g2 = groups_along_axis(dm.p2_coords, axis)[1:] + (None, )
    g1 = groups_along_axis(dm.p1_coords, axis)[1:] + (None, )
    return g2, g1


@pytest.mark.parametrize("name,scalar,axis", [("rect160x2", False, 1), ("rect160x2", True, 0), ("rect24x16", True, 1),
                                              ("box4x4x4", True, 2), ("box3x2x2", False, 0), ("periodic", False, 1),
                                              ("pchan3", True, 1)])
def test_profiles_along_an_axis_equal_the_restatement(name, scalar, axis):
    ref = reference(name)
    ctx = feed(ref, scalar)
    g2, g1 = _axis_groups(ref["dm"], axis)
    if name == "rect160x2":
        assert np.diff(g2[0]).tolist() == ([321] * 5 if axis == 1 else [5] * 321)
    if name == "pchan3":
        # profiles along y, between the walls: 5 planes of P2 nodes and 3 of P1 nodes, each holding one image of every
        # periodic node (6 x 6 and 3 x 3 of them, not 7 x 7 and 4 x 4)
        assert np.diff(g2[0]).tolist() == [36] * 5 and np.diff(g1[0]).tolist() == [9] * 3
    res = compare_profiles(ctx, ref, scalar, g2, g1, "%s axis %d" % (name, axis))
    if name == "rect160x2" and axis == 1:
        # the mean velocity varies along the 321-node lines: the between-node part must be there -- at least 10 % of
        # <u_x' u_x'> in every line, so a kernel that drops it cannot pass
        got, want, between = res[0]
        dim = ref["dm"].dim
        share = between[:, dim] / want[:, dim]
        print("between-node share of C_xx per line:", share)
        assert (share >= 0.1).all()
        assert (np.abs(got[:, dim] - (want[:, dim] - between[:, dim])) > 0.05 * want[:, dim]).all()
    ctx.close()


def test_hand_made_groups_on_the_unstructured_fixture():
    ref = reference("fixture")
    dm = ref["dm"]
    ctx = feed(ref, scalar=True)
    rng = np.random.default_rng(5)
    res = compare_profiles(ctx, ref, True, _hand_made_groups(dm.n_p2, rng), _hand_made_groups(dm.n_p1, rng), "fixture")
    # a one-node group is the node's own statistics
    got = res[0][0][:dm.n_p2]
    want = columns(ref["run2"][0], ref["run2"][1], dm.dim)
    assert np.abs(got - want).max() <= TOL * np.abs(ref["X2"]).max() ** 2
    ctx.close()


def test_two_fresh_contexts_give_the_same_bytes():
    ref = reference("rect24x16")
    g2, g1 = _axis_groups(ref["dm"], 1)
    blobs = []
    for _ in range(2):
        ctx = feed(ref, scalar=True)
        ctx.stats_set_groups(0, g2[0], g2[1])
        ctx.stats_set_groups(1, g1[0], g1[1])
        blob = b"".join(ctx.stats_get(q).tobytes() for q in Q_P2 + Q_P1 + Q_T)
        first = ctx.stats_profiles(0)
        assert first.shape == (33, 9) and ctx.stats_profiles(0).tobytes() == first.tobytes()   # and a second call
        blobs.append(blob + first.tobytes() + ctx.stats_profiles(1).tobytes())
        ctx.close()
    assert blobs[0] == blobs[1]


def test_refusals_leave_the_accumulators_unchanged():
    ref = reference("rect6x4")
    dm = ref["dm"]
    # before nsfem_stats_enable / nsfem_set_scalar
    ctx = context(ref["mesh"], dm)
    with pytest.raises(nat.NativeError, match="nsfem_stats_enable"):
        ctx.stats_sample(nat.U0, -1, -1, 1.0)
    with pytest.raises(nat.NativeError, match="nsfem_set_scalar"):
        ctx.stats_enable(nat.STATS_VELOCITY | nat.STATS_SCALAR)
    with pytest.raises(nat.NativeError, match="mandatory"):
        ctx.stats_enable(nat.STATS_PRESSURE)
    ctx.stats_enable(nat.STATS_VELOCITY | nat.STATS_PRESSURE)
    g2, g1 = _axis_groups(dm, 1)
    ctx.stats_set_groups(0, g2[0], g2[1])
    for call in (lambda: ctx.stats_get(nat.STATS_MEAN_U), lambda: ctx.stats_profiles(0)):
        with pytest.raises(nat.NativeError, match="no sample"):
            call()
    ctx.close()

    ctx = feed(ref, scalar=False)
    ctx.stats_set_groups(0, g2[0], g2[1])

    def snapshot():
        return (b"".join(ctx.stats_get(q).tobytes() for q in Q_P2 + Q_P1) + ctx.stats_profiles(0).tobytes(),
                ctx.stats_info(), ctx.stats_weight())

    before = snapshot()
    lib, h = ctx._lib, ctx._h
    buf = np.zeros(4 * dm.n_p2)
    refusals = [
        ("weight", lambda: ctx.stats_sample(nat.U0, nat.P, -1, 0.0)),
        ("weight", lambda: ctx.stats_sample(nat.U0, nat.P, -1, -1.0)),
        ("weight", lambda: ctx.stats_sample(nat.U0, nat.P, -1, float("nan"))),
        ("weight", lambda: ctx.stats_sample(nat.U0, nat.P, -1, float("inf"))),
        ("velocity slot", lambda: ctx.stats_sample(nat.P, nat.P, -1, 1.0)),
        ("velocity slot", lambda: ctx.stats_sample(-1, nat.P, -1, 1.0)),
        ("pressure slot", lambda: ctx.stats_sample(nat.U0, nat.U1, -1, 1.0)),
        ("pressure slot", lambda: ctx.stats_sample(nat.U0, -1, -1, 1.0)),
        ("NSFEM_STATS_SCALAR is not enabled", lambda: ctx.stats_sample(nat.U0, nat.P, nat.T0, 1.0)),
        ("NSFEM_STATS_SCALAR is not enabled", lambda: ctx.stats_get(nat.STATS_MEAN_T)),
        ("unknown quantity", lambda: ctx._check(lib.nsfem_stats_get(h, 99, nat._dp(buf), buf.size))),
        ("wrong size", lambda: ctx._check(lib.nsfem_stats_get(h, nat.STATS_MEAN_U, nat._dp(buf), 2 * dm.n_p2 - 1))),
        ("wrong size", lambda: ctx._check(lib.nsfem_stats_get(h, nat.STATS_MEAN_P, nat._dp(buf), dm.n_p2))),
        ("wrong size", lambda: ctx._check(lib.nsfem_stats_profiles(h, 0, nat._dp(buf), 9 * 5 + 1))),
        ("nsfem_stats_set_groups", lambda: ctx.stats_profiles(1)),
        ("out of range", lambda: ctx.stats_set_groups(0, [0, 2], [0, dm.n_p2])),
        ("out of range", lambda: ctx.stats_set_groups(0, [0, 2], [-1, 0])),
        ("out of range", lambda: ctx.stats_set_groups(1, [0, 1], [dm.n_p1])),          # a P2 index in a P1 list
        ("group_ptr", lambda: ctx.stats_set_groups(0, [0, 1, 1], [3])),
        ("weights", lambda: ctx.stats_set_groups(0, [0, 2], [0, 1], [1.0, 0.0])),
        ("field", lambda: ctx.stats_set_groups(2, [0, 1], [0])),
        ("unknown flag", lambda: ctx.stats_enable(8 | nat.STATS_VELOCITY)),
    ]
    for message, call in refusals:
        with pytest.raises(nat.NativeError, match=message) as exc:
            call()
        assert exc.value.code == nat.ERR_ARG
    with pytest.raises(ValueError):
        ctx.stats_set_groups(0, [0, 3], [0, 1])
    with pytest.raises(ValueError):
        ctx.stats_get(42)
    assert snapshot() == before
    ctx.close()

    # a partitioned context: two thread ranks of one GPU
    group = nat.local_group_create(2)
    ranks = [context(ref["mesh"], dm) for _ in range(2)]
    for r, c in enumerate(ranks):
        c.attach_local_comm(group, r)
    for c in ranks:
        for call in (lambda: c.stats_enable(nat.STATS_VELOCITY), lambda: c.stats_sample(nat.U0, -1, -1, 1.0),
                     lambda: c.stats_get(nat.STATS_MEAN_U), lambda: c.stats_profiles(0),
                     lambda: c.stats_set_groups(0, [0, 1], [0])):
            with pytest.raises(nat.NativeError, match="partitioned"):
                call()
        assert c.stats_info() == dict(samples=0, flags=0, bytes=0, launches=0)
    for c in ranks:
        c.close()
    nat.local_group_destroy(group)


def test_flow_statistics_class_fields_and_profiles():
    """FlowStatistics on a solver-like holder of a context: HostFields at the vertices, profiles by name"""
    from flow_statistics import FlowStatistics
    ref = reference("rect24x16")
    dm = ref["dm"]

    class Holder:
        pass

    holder = Holder()
    holder._ctx, holder._dofmap, holder._mesh = context(ref["mesh"], dm), dm, ref["mesh"]
    stats = FlowStatistics(holder, pressure=True)
    stats.set_profile_axis(1)
    for (u, T, p), w in zip(ref["samples"], WEIGHTS):
        holder._ctx.set_state(nat.U0, u.ravel())
        holder._ctx.set_state(nat.P, p)
        stats.sample(w)
    assert stats.weight == sum(WEIGHTS) and stats.info()["samples"] == 8
    m2, c2 = ref["run2"]
    nv = ref["mesh"].coords.shape[0]
    mu, rs, tke, mp = stats.mean_velocity(), stats.reynolds_stress(), stats.turbulent_kinetic_energy(), stats.mean_pressure()
    assert mu.center == "Node" and mu.values.shape == (nv, 2) and rs.values.shape == (nv, 3) and tke.values.shape == (nv, )
    assert mp.values.shape == (nv, ) and stats.pressure_variance().values.shape == (nv, )
    assert np.abs(mu.values - m2[dm.vertex_node, :2]).max() <= TOL * np.abs(ref["X2"][:, :, :2]).max()
    assert np.abs(mp.values - ref["run1"][0][dm.p1_vertex_node, 0]).max() <= TOL * np.abs(ref["X1"]).max()
    with pytest.raises(nat.NativeError, match="not enabled"):
        stats.mean_temperature()
    y, prof = stats.profiles()
    assert y.shape == (33, ) and np.abs(y - np.linspace(0.0, 1.0, 33)).max() <= 1e-14
    assert prof["mean_velocity"].shape == (33, 2) and prof["reynolds_stress"].shape == (33, 3)
    assert prof["pressure_coordinates"].shape == (17, ) and prof["mean_pressure"].shape == (17, )
    raw = holder._ctx.stats_profiles(0)
    assert prof["mean_velocity"].tobytes() == raw[:, :2].tobytes()
    assert np.array_equal(prof["turbulent_kinetic_energy"], 0.5 * (raw[:, 2] + raw[:, 4]))
    stats.reset()
    assert stats.info()["samples"] == 0
    holder._ctx.close()


def test_profiles_after_reset_and_after_enabling_again_keep_the_groups():
    """reset() and a second stats_enable drop the samples and keep the groups: the same samples fed again give the
    profiles' bytes again; only stats_enable(0) frees the groups"""
    from flow_statistics import FlowStatistics
    ref = reference("rect24x16")
    dm = ref["dm"]

    class Holder:
        pass

    holder = Holder()
    ctx = context(ref["mesh"], dm)
    holder._ctx, holder._dofmap, holder._mesh = ctx, dm, ref["mesh"]
    stats = FlowStatistics(holder, pressure=True)
    stats.set_profile_axis(1)

    def feed_all():
        for (u, T, p), w in zip(ref["samples"], WEIGHTS):
            ctx.set_state(nat.U0, u.ravel())
            ctx.set_state(nat.P, p)
            stats.sample(w)
        return ctx.stats_profiles(0), ctx.stats_profiles(1)

    first2, first1 = feed_all()
    g2, g1 = _axis_groups(dm, 1)
    m2, c2 = ref["run2"]
    want, scale, _ = pooled_profiles(m2[:, :2], c2[:, :2, :2], 2, g2[0], g2[1], np.ones(len(g2[1])))
    assert first2.shape == want.shape == (33, 5) and first1.shape == (17, 2)
    assert (np.abs(first2 - want) <= TOL * scale + 1e-300).all()
    flags = nat.STATS_VELOCITY | nat.STATS_PRESSURE
    for again in (stats.reset, lambda: ctx.stats_enable(flags)):
        again()
        assert stats.info() == dict(samples=0, flags=flags, bytes=stats.info()["bytes"], launches=0)
        with pytest.raises(nat.NativeError, match="no sample has been taken"):
            ctx.stats_profiles(0)
        got2, got1 = feed_all()
        assert got2.tobytes() == first2.tobytes() and got1.tobytes() == first1.tobytes()
        y, prof = stats.profiles()
        assert y.shape == (33, ) and prof["mean_velocity"].tobytes() == first2[:, :2].tobytes()
        assert prof["mean_pressure"].tobytes() == first1[:, 0].tobytes()
    # flags = 0 frees the groups as well, on both sides
    ctx.stats_enable(0)
    ctx.stats_enable(flags)
    ctx.set_state(nat.U0, ref["samples"][0][0].ravel())
    stats.sample(1.0)
    with pytest.raises(nat.NativeError, match="nsfem_stats_set_groups has not been called"):
        ctx.stats_profiles(0)
    ctx.close()


def test_a_second_flow_statistics_on_one_solver_is_refused():
    """one set of accumulators per context: a second instance must not silently zero and share the first one's"""
    from flow_statistics import FlowStatistics
    ref = reference("rect6x4")

    class Holder:
        pass

    holder = Holder()
    holder._ctx, holder._dofmap, holder._mesh = context(ref["mesh"], ref["dm"]), ref["dm"], ref["mesh"]
    stats = FlowStatistics(holder, pressure=True)
    holder._ctx.set_state(nat.U0, ref["samples"][0][0].ravel())
    stats.sample(1.0)
    with pytest.raises(ValueError, match="already serves another FlowStatistics"):
        FlowStatistics(holder, pressure=False)
    stats.bind(holder)                                                             # binding the same one again is fine
    assert stats.info()["samples"] == 1 and stats.info()["flags"] == nat.STATS_VELOCITY | nat.STATS_PRESSURE
    holder._ctx.close()
    problem = _cavity(2, 1.0 / 32.0)
    problem._add_flow_statistics()
    with pytest.raises(ValueError, match="already registered"):
        problem._add_flow_statistics(every=2)


@pytest.mark.parametrize("name", ["rect6x4", "box3x2x2"])
def test_an_unchanged_field_keeps_a_negative_zero_in_the_mean(name):
    """entries that are -0.0 (and +0.0): d = x - m = +0.0 there, and the mean must keep its bytes, not take -0.0 + a 0.0"""
    ref = reference(name)
    dm = ref["dm"]
    u, T, p = (np.array(a) for a in ref["samples"][2])
    u[::3], T[1::4], p[::2] = -0.0, -0.0, -0.0
    u[1::3], T[2::4], p[1::2] = 0.0, 0.0, 0.0
    u[-1], p[-1] = -0.0, -0.0                                                      # the odd last node: the 8-byte path
    assert np.signbit(u).any() and np.signbit(p).any()
    ctx = context(ref["mesh"], dm)
    ctx.set_scalar(0.01)
    ctx.stats_enable(nat.STATS_VELOCITY | nat.STATS_PRESSURE | nat.STATS_SCALAR)
    for s, v in ((nat.U0, u.ravel()), (nat.P, p), (nat.T0, T)):
        ctx.set_state(s, v)
    for w in (0.7, 1.0, 0.3, 2.0):
        ctx.stats_sample(nat.U0, nat.P, nat.T0, w)
        assert ctx.stats_get(nat.STATS_MEAN_U).tobytes() == u.tobytes()
        assert ctx.stats_get(nat.STATS_MEAN_P).tobytes() == p.tobytes()
        assert ctx.stats_get(nat.STATS_MEAN_T).tobytes() == T.tobytes()
    for q in (nat.STATS_COV_U, nat.STATS_TKE, nat.STATS_VAR_P, nat.STATS_VAR_T, nat.STATS_FLUX_UT):
        got = ctx.stats_get(q)
        assert got.tobytes() == np.zeros_like(got).tobytes(), q
    ctx.close()


# ---------------------------------------------------------------- through the problem loop
def _cavity(steps, dt, hook=None):
    from ns_imex_solver import IMEXIPCSSolver
    from problem_specs import build_problem
    spec = dict(name="Cavity", mesh=("cube", 2, 8), scheme="ipcs", numbers=dict(Re=100.0),
                clock=dict(dt=dt, steps=steps), start={"velocity": (0.0, 0.0), "pressure": 0.0}, postprocessing=1,
                bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_slip", "bottom"), ("velocity", "top", (1.0, 0.0))])
    if hook is not None:
        spec["hook"] = hook
    problem = build_problem(spec)
    problem.set_solver_class(IMEXIPCSSolver)
    problem.compute_cfl = False
    return problem


def test_registered_statistics_in_the_problem_loop_equal_the_restatement_and_leave_the_flow_alone():
    steps, dt = 6, 1.0 / 32.0
    record = []

    def hook(problem):
        ctx, ts = problem._get_solver()._ctx, problem._time_stepping
        record.append((ts.next_time, ts.get_next_step_size(), ctx.get_state(nat.U0), ctx.get_state(nat.P)))

    problem = _cavity(steps, dt, hook)
    stats = problem._add_flow_statistics(start_time=3 * dt, every=1)
    problem.solve_problem()
    solver = problem._get_solver()
    assert len(record) == steps and abs(record[2][0] - 3 * dt) <= 1e-12
    info = solver._ctx.stats_info()
    assert info["samples"] == 4 and info["launches"] == 4
    assert info["flags"] == nat.STATS_VELOCITY | nat.STATS_PRESSURE
    rs2, rs1 = RunningStats(), RunningStats()
    for t, k, u, p in record[2:]:
        rs2.update(u.reshape(-1, 2), k)
        rs1.update(p[:, None], k)
    assert abs(stats.weight - 4 * dt) <= 1e-15
    umax = max(np.abs(r[2]).max() for r in record)
    pmax = max(np.abs(r[3]).max() for r in record)
    errs = dict(mean_u=np.abs(stats.nodal(nat.STATS_MEAN_U) - rs2.m).max() / umax,
                cov_u=np.abs(stats.nodal(nat.STATS_COV_U) - columns(rs2.m, rs2.covariance(), 2)[:, 2:]).max() / umax ** 2,
                tke=np.abs(stats.nodal(nat.STATS_TKE) - 0.5 * (rs2.covariance()[:, 0, 0] + rs2.covariance()[:, 1, 1])).max()
                / umax ** 2,
                mean_p=np.abs(stats.nodal(nat.STATS_MEAN_P) - rs1.m[:, 0]).max() / pmax,
                var_p=np.abs(stats.nodal(nat.STATS_VAR_P) - rs1.covariance()[:, 0, 0]).max() / pmax ** 2)
    print("problem loop, error / scale:", errs)
    assert stats.nodal(nat.STATS_TKE).max() > 0.0                                   # the start-up of the cavity is not steady
    assert all(e <= TOL for e in errs.values()), errs
    # every = 2 from the start: steps 1, 3, 5
    other = _cavity(steps, dt)
    thinned = other._add_flow_statistics(pressure=False, every=2)
    other.solve_problem()
    assert thinned.info()["samples"] == 3 and thinned.info()["flags"] == nat.STATS_VELOCITY
    # the same problem without a registration: the flow is bit-identical
    plain = _cavity(steps, dt)
    plain.solve_problem()
    assert plain._get_solver()._ctx.stats_info() == dict(samples=0, flags=0, bytes=0, launches=0)
    for slot in (nat.U0, nat.P):
        a = solver._ctx.get_state(slot)
        assert a.tobytes() == plain._get_solver()._ctx.get_state(slot).tobytes()
        assert a.tobytes() == other._get_solver()._ctx.get_state(slot).tobytes()
