"""Host restatement of the running flow statistics (csrc/statistics.hip) -- the pinned yardstick of
tests/test_gpu_flow_statistics.py -- and the group builder of ``FlowStatistics.set_profile_axis``.  No GPU.

``RunningStats`` restates the weighted Welford / Chan update of one field's nodes in numpy, ``pooled_profiles`` the
reduction over groups of nodes; both are pinned here against two-pass numpy (``np.average``, ``np.cov(...,
aweights=w, ddof=0)``) on random data with unequal weights."""
import numpy as np
import pytest

from fem_mesh import TaylorHoodDofMap, periodic_entity_map, rectangle_mesh
from flow_statistics import FlowStatistics, groups_along_axis

WEIGHTS = (1.0, 0.5, 2.0, 1.0, 0.25, 1.0, 3.0, 1.0)


class RunningStats:
    """m [n, nv], C [n, nv, nv] (sum of weighted products of deviations: divide by W) and W after any number of
    ``update(x [n, nv], w)`` calls -- the update of k_stats_update, variable by variable"""

    def __init__(self):
        self.W, self.m, self.C = 0.0, None, None

    def update(self, x, w):
        x = np.asarray(x, dtype=np.float64)
        if self.m is None:
            self.m = np.zeros_like(x)
            self.C = np.zeros(x.shape + (x.shape[1], ))
        a, b = w / (self.W + w), w * self.W / (self.W + w)
        d = x - self.m
        # (d == 0 keeps the mean's bytes, a -0.0 included)
        self.m = x.copy() if self.W == 0.0 else np.where(d == 0.0, self.m, self.m + a * d)
        self.C = self.C + b * d[:, :, None] * d[:, None, :]
        self.W += w

    def covariance(self):
        return self.C / self.W


def two_pass(X, w):
    """(mean [n, nv], covariance [n, nv, nv]) of the samples X [k, n, nv] with weights w [k], mean first"""
    w = np.asarray(w, dtype=np.float64)
    mean = np.average(X, axis=0, weights=w)
    dev = X - mean
    return mean, np.einsum("k,kni,knj->nij", w, dev, dev) / w.sum()


def columns(m, cov, dim):
    """[n, n_q] in the column order of the accumulators / nsfem_stats_profiles: m_u, the upper triangle of C_uu row by
    row, and where there is one more variable (the scalar) m_T, C_TT, C_uT"""
    cols = [m[:, i] for i in range(dim)]
    cols += [cov[:, i, j] for i in range(dim) for j in range(i, dim)]
    if m.shape[1] > dim:
        cols += [m[:, dim], cov[:, dim, dim]] + [cov[:, i, dim] for i in range(dim)]
    return np.stack(cols, axis=1)


def pooled_profiles(m, cov, dim, group_ptr, nodes, weights):
    """(values [g, n_q], scale [g, n_q], between [g, n_q]) of the groups: m_g = sum a m / A, C_g = sum a C_n / A +
    sum a (m - m_g)(m - m_g)^T / A; scale = the sum of the absolute contributions / A (what a tolerance on a sum is
    relative to), between = the second term alone (0 in the mean columns)"""
    n_groups = len(group_ptr) - 1
    vals, scale, between = [], [], []
    for g in range(n_groups):
        idx = np.asarray(nodes[group_ptr[g]:group_ptr[g + 1]], dtype=np.int64)
        a = np.asarray(weights[group_ptr[g]:group_ptr[g + 1]], dtype=np.float64)
        A = a.sum()
        mn, cn = m[idx], cov[idx]
        mg = (a[:, None] * mn).sum(axis=0) / A
        dm = mn - mg
        within = a[:, None, None] * cn
        betw = a[:, None, None] * dm[:, :, None] * dm[:, None, :]
        cg = (within.sum(axis=0) + betw.sum(axis=0)) / A
        one = np.ones((1, ) + mg.shape)
        vals.append(columns(mg[None], cg[None], dim)[0])
        scale.append(columns((np.abs(a[:, None] * mn).sum(axis=0) / A)[None],
                             ((np.abs(within) + np.abs(betw)).sum(axis=0) / A)[None], dim)[0])
        between.append(columns(0.0 * one, (betw.sum(axis=0) / A)[None], dim)[0])
    return np.array(vals), np.array(scale), np.array(between)


# ---------------------------------------------------------------- the restatement against two-pass numpy
@pytest.mark.parametrize("nv", [1, 3, 4])
def test_running_update_equals_two_pass_numpy(nv):
    rng = np.random.default_rng(7 + nv)
    n, k = 40, len(WEIGHTS)
    X = rng.standard_normal((k, n, nv)) + 3.0 * rng.standard_normal((1, n, nv))
    rs = RunningStats()
    for j in range(k):
        rs.update(X[j], WEIGHTS[j])
    assert rs.W == sum(WEIGHTS)
    mean, cov = two_pass(X, WEIGHTS)
    xmax = np.abs(X).max()
    assert np.abs(rs.m - mean).max() <= 1e-13 * xmax
    assert np.abs(rs.covariance() - cov).max() <= 1e-13 * xmax ** 2
    for node in (0, 17, n - 1):                                  # ... and two_pass against numpy's own estimators
        ref_m = np.average(X[:, node, :], axis=0, weights=WEIGHTS)
        ref_c = np.cov(X[:, node, :], rowvar=False, aweights=WEIGHTS, ddof=0).reshape(nv, nv)
        assert np.abs(rs.m[node] - ref_m).max() <= 1e-13 * xmax
        assert np.abs(rs.covariance()[node] - ref_c).max() <= 1e-13 * xmax ** 2


def test_first_sample_is_the_mean_and_a_constant_field_has_no_variance():
    rng = np.random.default_rng(1)
    x = rng.standard_normal((11, 3))
    rs = RunningStats()
    rs.update(x, 0.7)
    assert rs.m.tobytes() == x.tobytes() and not rs.C.any()
    for w in (1.0, 0.3, 2.0):
        rs.update(x, w)
    assert rs.m.tobytes() == x.tobytes() and not rs.C.any()


def test_pooled_profile_equals_the_covariance_of_all_samples_of_the_group():
    """pooling the nodes of a group = treating every (sample, node) pair as one sample of weight w_k a_n"""
    rng = np.random.default_rng(3)
    n, k, nv, dim = 12, len(WEIGHTS), 3, 2
    X = rng.standard_normal((k, n, nv)) + 2.0 * rng.standard_normal((1, n, nv))
    mean, cov = two_pass(X, WEIGHTS)
    group_ptr = np.array([0, 5, 6, 12])
    nodes = rng.permutation(n)
    a = rng.uniform(0.5, 2.0, n)
    vals, scale, between = pooled_profiles(mean, cov, dim, group_ptr, nodes, a)
    assert vals.shape == (3, 2 + 3 + 2 + 2)
    for g in range(3):
        idx = nodes[group_ptr[g]:group_ptr[g + 1]]
        ag = a[group_ptr[g]:group_ptr[g + 1]]
        flat = X[:, idx, :].reshape(-1, nv)
        wts = (np.asarray(WEIGHTS)[:, None] * ag[None, :]).ravel()
        ref_m = np.average(flat, axis=0, weights=wts)
        ref_c = np.cov(flat, rowvar=False, aweights=wts, ddof=0)
        ref = columns(ref_m[None], ref_c[None], dim)[0]
        assert np.abs(vals[g] - ref).max() <= 1e-13 * np.abs(X).max() ** 2
        assert (scale[g] >= np.abs(vals[g]) * (1.0 - 1e-14)).all()
    assert np.abs(between[1]).max() <= 1e-28                      # a one-node group has no between-node part (a m / a
                                                                  # may round: squares of 1e-16 at the most)
    assert between[0][dim] > 0.0


# ---------------------------------------------------------------- the group builder
def periodic_square(n):
    import dlfn_compat as dlfn

    class Periodic(dlfn.SubDomain):
        def inside(self, x, on_boundary):
            return bool((dlfn.near(x[0], 0.0) or dlfn.near(x[1], 0.0)) and
                        not (dlfn.near(x[0], 1.0) or dlfn.near(x[1], 1.0)) and on_boundary)

        def map(self, x, y):
            for a in range(2):
                y[a] = x[a] - 1.0 if dlfn.near(x[a], 1.0) else x[a]

    mesh = rectangle_mesh((0.0, 0.0), (1.0, 1.0), n, n)
    return mesh, TaylorHoodDofMap(mesh, periodic_map=periodic_entity_map(mesh, Periodic()))


def _check_partition(values, group_ptr, nodes, coords, axis, n_groups, per_group):
    assert group_ptr[0] == 0 and group_ptr[-1] == nodes.size == coords.shape[0]
    assert group_ptr.dtype == np.int32 and nodes.dtype == np.int32
    assert len(values) == n_groups == len(group_ptr) - 1
    assert (np.diff(group_ptr) == per_group).all()
    assert (np.diff(values) > 0.0).all()                                     # sorted by coordinate
    assert np.array_equal(np.sort(nodes), np.arange(coords.shape[0]))        # every node in exactly one group
    for g in range(n_groups):
        idx = nodes[group_ptr[g]:group_ptr[g + 1]]
        assert (np.diff(idx) > 0).all()                                      # ascending within a group
        assert np.abs(coords[idx, axis] - values[g]).max() <= 1e-12


def test_groups_of_a_rectangle():
    mesh = rectangle_mesh((0.0, 0.0), (1.5, 1.0), 6, 4)
    dm = TaylorHoodDofMap(mesh)
    assert dm.n_p2 == 13 * 9 and dm.n_p1 == 7 * 5
    _check_partition(*FlowStatistics.groups_along_axis(dm.p2_coords, 1), dm.p2_coords, 1, 9, 13)
    _check_partition(*FlowStatistics.groups_along_axis(dm.p2_coords, 0), dm.p2_coords, 0, 13, 9)
    _check_partition(*FlowStatistics.groups_along_axis(dm.p1_coords, 1), dm.p1_coords, 1, 5, 7)
    values, _, _ = groups_along_axis(dm.p2_coords, 1)
    assert np.abs(values - np.linspace(0.0, 1.0, 9)).max() <= 1e-14


def test_groups_of_a_periodic_square():
    mesh, dm = periodic_square(4)
    assert dm.n_p2 == 8 * 8 and dm.n_p1 == 4 * 4                             # the images are one node each
    for axis in (0, 1):
        _check_partition(*groups_along_axis(dm.p2_coords, axis), dm.p2_coords, axis, 8, 8)
        _check_partition(*groups_along_axis(dm.p1_coords, axis), dm.p1_coords, axis, 4, 4)


def test_tolerance_merges_close_coordinates():
    coords = np.array([[0.0, 0.0], [1.0, 1e-13], [2.0, 1.0], [3.0, 1.0 - 1e-13], [4.0, 0.5]])
    values, ptr, nodes = groups_along_axis(coords, 1, tol=1e-9)
    assert ptr.tolist() == [0, 2, 3, 5] and nodes.tolist() == [0, 1, 4, 2, 3]
    assert np.abs(values - [0.0, 0.5, 1.0]).max() <= 1e-12
