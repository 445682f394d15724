"""Energy spectra on the device (csrc/spectrum.hip: k_spec_pack, k_spec_bin, k_spec_bin_sum; the axis passes through
fd_transform_axes of csrc/fastdiag.hip; nsfem_spectrum_set / _compute / _info) against the complex-FFT yardstick of
tests/spectrum_host.py, and the callers: ``energy_spectrum.EnergySpectrum`` and ``ProblemBase._add_energy_spectrum``.

Tolerance (derived, not measured): every bin is compared absolutely against ``8 d N_max eps S`` -- the worst-case
``gamma_N`` of a length-N dot product once per pass, doubled for the square, a factor 4 for the accumulation order of
the matrix instruction; ``eps = 2.2e-16``, ``S`` the yardstick's total of that component.  Two calls on the same state
are compared for equal bytes.

Shapes: the smallest that take each path of the GEMM tile -- one partial 32-tile (8 x 8), ragged 32-tiles (24 x 16),
K = 200 (more than two 96-blocks: both halves of the register double buffer and a ragged tail) and K = 100 (one block
plus a tail of 4) in 2D, on the x pass and on the z pass in 3D, three passes with different tile fill, odd sizes below
every tile edge (9 x 7, the 5 x 3 pressure lattice)."""
import ctypes as C
import types

import numpy as np
import pytest

import _native as nat
import energy_spectrum as es
import spectrum_host as sh
from gpu_common import context
from test_energy_spectrum_host import periodic_box

pytestmark = pytest.mark.gpu
_CACHE = {}


def _box(cells, axes, lengths=None):
    """(mesh, dofmap): parity numbering in 3D (the nodes are then NOT in lattice order), lexicographic in 2D"""
    lengths = tuple(lengths or (1.0, ) * len(cells))
    key = (tuple(cells), tuple(axes), lengths)
    if key not in _CACHE:
        _CACHE[key] = periodic_box(cells, lengths, tuple(axes), "parity" if len(cells) == 3 else True)
    return _CACHE[key] + (lengths, )


def _spacing(cells, lengths, m=2):
    return [L / (m * c) for L, c in zip(lengths, cells)]


def _loaded(mesh, dm, seed):
    rng = np.random.default_rng(seed)
    U = rng.standard_normal((dm.n_p2, dm.dim))
    ctx = context(mesh, dm)
    ctx.set_state(nat.U0, U.ravel())
    return ctx, U


def _check(got, want, shape, label):
    """got, want [n_bins]: absolute error of every bin against 8 d N_max eps S"""
    assert got.shape == want.shape, (label, got.shape, want.shape)
    tol = sh.tolerance(shape, want.sum())
    ratio = np.abs(got - want).max() / tol
    print("%s: largest error / tolerance %.3g" % (label, ratio))
    assert ratio <= 1.0, (label, ratio)
    return ratio


def _as_solver(ctx, dm):
    return types.SimpleNamespace(_ctx=ctx, _dofmap=dm)


# ---------------------------------------------------------------- the generic transform
def test_generic_transform_with_random_orthogonal_matrices_and_overlapping_bins():
    mesh, dm, lengths = _box((4, 3), ())
    ctx, U = _loaded(mesh, dm, 1)
    lat = es.lattice_of_nodes(mesh, dm, "velocity")
    assert lat.shape == (9, 7)
    rng = np.random.default_rng(2)
    Fx = np.linalg.qr(rng.standard_normal((9, 9)))[0]
    Fy = np.linalg.qr(rng.standard_normal((7, 7)))[0]
    # bins that overlap, leave points out (point 0 and the last five are in none) and one that is empty
    sizes = (11, 1, 0, 40, 63, 7)
    lists = [rng.integers(1, 58, size=s) for s in sizes]
    ptr = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    pts = np.concatenate(lists).astype(np.int32)
    arr = sh.lattice_array(U, dm.p2_coords, _spacing((4, 3), lengths), lat.shape)       # [7][9][2]
    try:
        for label, mats in (("random orthogonal", (Fx, Fy)), ("x only", (Fx, None)), ("no transform", (None, None))):
            ctx.spectrum_set(lat.shape, mats, lat.node_of_point, ptr, pts)
            got = ctx.spectrum_compute(nat.U0)
            assert got.shape == (len(sizes), 2)
            for c in range(2):
                w = arr[..., c]
                if mats[0] is not None:
                    w = np.einsum("ki,ji->jk", mats[0], w)
                if mats[1] is not None:
                    w = np.einsum("kj,ji->ki", mats[1], w)
                sq = w.ravel() ** 2
                want = np.array([sq[l].sum() for l in lists])
                tol = sh.tolerance(lat.shape, sq.sum())
                err = np.abs(got[:, c] - want).max()
                print("%s, component %d: error / tolerance %.3g" % (label, c, err / tol))
                assert err <= tol, (label, c)
            assert got[2].tobytes() == np.zeros(2).tobytes()                              # the empty bin: +0.0
        info = ctx.spectrum_info()
        assert info["calls"] == 3 and info["transform_launches"] == 2 * (2 + 1 + 0) and info["bin_launches"] == 3 * 2 * 2
        assert info["bytes"] > 2 * 63 * 8
    finally:
        ctx.close()


# ---------------------------------------------------------------- shells of a random field
SHELL_CASES = [(4, 4), (12, 8), (100, 50), (4, 6, 10), (50, 2, 2), (2, 2, 50)]


@pytest.mark.parametrize("cells", SHELL_CASES, ids=lambda c: "x".join(str(v) for v in c))
def test_shell_spectrum_of_a_random_field_meets_the_fft_yardstick(cells):
    dim = len(cells)
    mesh, dm, lengths = _box(cells, range(dim))
    ctx, U = _loaded(mesh, dm, 10 + sum(cells))
    try:
        spec = es.EnergySpectrum(_as_solver(ctx, dm), kind="shell")
        shape = spec.lattice.shape
        assert shape == tuple(2 * c for c in cells) and dm.n_p2 == int(np.prod(shape))
        res = spec.compute()
        raw = spec.raw()
        arr = sh.lattice_array(U, dm.p2_coords, _spacing(cells, lengths), shape)
        n_points = float(np.prod(shape))
        total = 0.0
        for c in range(dim):
            want = sh.shell_spectrum(arr[..., c], lengths)
            _check(raw[:, c], want, shape, "cells %r component %d" % (cells, c))
            # Parseval, component by component
            assert abs(raw[:, c].sum() - (U[:, c] ** 2).sum()) <= sh.tolerance(shape, want.sum())
            assert np.abs(res["components"][:, c] - 0.5 * want / n_points).max() <= \
                sh.tolerance(shape, 0.5 * want.sum() / n_points)
            total += want.sum()
        # sum_b E[b] = 1/2 <|u|^2> over the lattice points
        assert res["E"].shape == res["k"].shape == (raw.shape[0], )
        assert abs(res["E"].sum() - 0.5 * (U ** 2).sum() / n_points) <= sh.tolerance(shape, 0.5 * total / n_points)
        assert np.allclose(res["k"], 2.0 * np.pi * np.arange(raw.shape[0]))
        assert spec.raw().tobytes() == raw.tobytes()
    finally:
        ctx.close()


# ---------------------------------------------------------------- single modes
MODES = [(0, 0, "cos"), (3, 0, "cos"), (3, 0, "sin"), (0, 5, "cos"), (0, 5, "sin"), (7, 3, "sin"), (12, 0, "cos"),
         (0, 8, "cos"), (12, 8, "cos")]


def test_single_modes_on_24x16_sit_in_the_predicted_shell():
    """cos and sin modes at k = 0, at interior k and at the Nyquist k = n / 2 along each axis (the sin mode of the
    Nyquist wavenumber vanishes at every lattice point: there is nothing to test)"""
    cells = (12, 8)
    mesh, dm, lengths = _box(cells, (0, 1))
    ctx = context(mesh, dm)
    try:
        spec = es.EnergySpectrum(_as_solver(ctx, dm), kind="shell")
        assert spec.lattice.shape == (24, 16)
        X = dm.p2_coords
        for kx, ky, kind in MODES:
            phase = 2.0 * np.pi * (kx * X[:, 0] + ky * X[:, 1])
            U = np.zeros((dm.n_p2, 2))
            U[:, 0] = np.cos(phase) if kind == "cos" else np.sin(phase)
            U[:, 1] = -0.5 * U[:, 0]
            ctx.set_state(nat.U0, U.ravel())
            raw = spec.raw()
            shell = int(np.rint(np.hypot(kx, ky)))
            for c in range(2):
                S = (U[:, c] ** 2).sum()
                tol = sh.tolerance((24, 16), S)
                assert S > 1.0
                assert abs(raw[shell, c] - S) <= tol, (kx, ky, kind, c)
                assert np.abs(np.delete(raw[:, c], shell)).max() <= tol, (kx, ky, kind, c)
    finally:
        ctx.close()


# ---------------------------------------------------------------- analytic Taylor-Green
def test_taylor_green_2d_has_a_quarter_in_shell_one():
    cells, L = (8, 8), (2.0 * np.pi, ) * 2
    mesh, dm, lengths = _box(cells, (0, 1), L)
    ctx = context(mesh, dm)
    try:
        x, y = dm.p2_coords.T
        U = np.stack([np.cos(x) * np.sin(y), -np.sin(x) * np.cos(y)], axis=1)
        ctx.set_state(nat.U0, U.ravel())
        res = es.EnergySpectrum(_as_solver(ctx, dm), kind="shell").compute()
        tol = sh.tolerance((16, 16), 0.25)
        assert np.allclose(res["k"], np.arange(res["k"].size))            # dkappa = 1 on [0, 2 pi]^2
        assert abs(res["E"].sum() - 0.25) <= tol and abs(res["E"][1] - 0.25) <= tol
        assert np.abs(np.delete(res["E"], 1)).max() <= tol
    finally:
        ctx.close()


def test_taylor_green_3d_has_an_eighth_in_shell_two():
    cells, L = (4, 4, 4), (2.0 * np.pi, ) * 3
    mesh, dm, lengths = _box(cells, (0, 1, 2), L)
    assert dm.ordering == "parity"
    ctx = context(mesh, dm)
    try:
        x, y, z = dm.p2_coords.T
        U = np.stack([np.sin(x) * np.cos(y) * np.cos(z), -np.cos(x) * np.sin(y) * np.cos(z), 0.0 * x], axis=1)
        ctx.set_state(nat.U0, U.ravel())
        res = es.EnergySpectrum(_as_solver(ctx, dm), kind="shell").compute()
        tol = sh.tolerance((8, 8, 8), 0.125)
        assert abs(res["E"].sum() - 0.125) <= tol and abs(res["E"][2] - 0.125) <= tol
        assert np.abs(np.delete(res["E"], 2)).max() <= tol
        assert np.abs(res["components"][:, 2]).max() == 0.0
    finally:
        ctx.close()


# ---------------------------------------------------------------- channels: E(k_x; y)
@pytest.mark.parametrize("cells,axes", [((8, 4), (0, )), ((4, 3, 6), (0, 2))], ids=["2d", "3d"])
def test_channel_spectra_along_x_at_every_wall_distance(cells, axes):
    dim = len(cells)
    mesh, dm, lengths = _box(cells, axes)
    ctx, U = _loaded(mesh, dm, 77 + dim)
    try:
        spec = es.EnergySpectrum(_as_solver(ctx, dm), kind="axis", axis=0)
        shape = spec.lattice.shape
        periodic = tuple(a in axes for a in range(dim))
        assert shape == tuple(2 * c + (0 if p else 1) for c, p in zip(cells, periodic))
        res = spec.compute()
        n_k, n_y = shape[0] // 2 + 1, shape[1]
        assert res["E"].shape == (n_y, n_k) and res["components"].shape == (n_y, n_k, dim)
        assert np.allclose(res["walls"][0], np.linspace(0.0, 1.0, n_y)) and len(res["walls"]) == 1
        assert np.allclose(res["k"], 2.0 * np.pi * np.arange(n_k))
        arr = sh.lattice_array(U, dm.p2_coords, _spacing(cells, lengths), shape)
        per_plane = float(np.prod(shape)) / n_y
        raw = spec.raw().reshape(n_y, n_k, dim)
        E = np.zeros((n_y, n_k))
        for c in range(dim):
            want = sh.axis_spectrum(arr[..., c], 0, periodic)            # the yardstick: fft along x only
            _check(raw[..., c].ravel(), want.ravel(), shape, "channel %r component %d" % (cells, c))
            E += 0.5 * want / per_plane
        tol = sh.tolerance(shape, E.sum())
        assert np.abs(res["E"] - E).max() <= tol
        # at every y the sum over k is the physical 1/2 mean square of that line / plane
        sq = 0.5 * (arr ** 2).sum(axis=-1)
        plane = sq.sum(axis=tuple(p for p in range(dim) if p != dim - 2)) / per_plane
        assert np.abs(res["E"].sum(axis=1) - plane).max() <= tol
    finally:
        ctx.close()


# ---------------------------------------------------------------- scalar and pressure slots
def test_scalar_and_pressure_slots_have_one_component():
    cells = (5, 3)
    mesh, dm, lengths = _box(cells, (0, 1))
    ctx, U = _loaded(mesh, dm, 5)
    rng = np.random.default_rng(6)
    T, p = rng.standard_normal(dm.n_p2), rng.standard_normal(dm.n_p1)
    ctx.set_state(nat.T0, T)
    ctx.set_state(nat.P, p)
    solver = _as_solver(ctx, dm)
    solver._scalar_coefficients = {}
    try:
        st = es.EnergySpectrum.one_shot(solver, field="temperature")
        sp = es.EnergySpectrum.one_shot(solver, field="pressure")
        assert st.lattice.shape == (10, 6) and sp.lattice.shape == (5, 3)
        for spec, values, X, m in ((st, T, dm.p2_coords, 2), (sp, p, dm.p1_coords, 1), (st, T, dm.p2_coords, 2)):
            shape = spec.lattice.shape
            raw = spec.raw()
            assert raw.shape[1] == 1
            arr = sh.lattice_array(values, X, _spacing(cells, lengths, m), shape)
            _check(raw[:, 0], sh.shell_spectrum(arr, lengths), shape, "field %s" % spec.field)
            res = spec.compute()
            assert abs(res["E"].sum() - (values ** 2).mean()) <= sh.tolerance(shape, (values ** 2).mean())   # no 1/2
        # the pressure plan fits the P2 slots as well (its nodes are a subset), the P2 plan does not fit the pressure
        assert ctx.spectrum_compute(nat.T0).shape[1] == 1
        sp.raw()
        assert ctx.spectrum_compute(nat.U0).shape == (sp.bins.bin_ptr.size - 1, 2)
        st.raw()
        with pytest.raises(nat.NativeError, match="does not have"):
            ctx.spectrum_compute(nat.P)
    finally:
        ctx.close()


# ---------------------------------------------------------------- determinism
def test_same_state_same_bytes_whatever_ran_in_between():
    cells = (4, 6, 10)
    mesh, dm, lengths = _box(cells, (0, 1, 2))
    ctx, U = _loaded(mesh, dm, 9)
    ctx.set_state(nat.P, np.random.default_rng(3).standard_normal(dm.n_p1))
    solver = _as_solver(ctx, dm)
    try:
        sv = es.EnergySpectrum.one_shot(solver)
        first = sv.raw()
        assert sv.raw().tobytes() == first.tobytes()
        sp = es.EnergySpectrum.one_shot(solver, field="pressure")
        p1 = sp.raw()
        assert sp.raw().tobytes() == p1.tobytes()
        assert sv.raw().tobytes() == first.tobytes()                 # the plan was replaced twice in between
        # a fresh context gives the same bytes
        other = context(mesh, dm)
        other.set_state(nat.U0, U.ravel())
        try:
            assert es.EnergySpectrum(_as_solver(other, dm), kind="shell").raw().tobytes() == first.tobytes()
        finally:
            other.close()
    finally:
        ctx.close()


# ---------------------------------------------------------------- refusals
def test_refusals_leave_the_plan_and_the_counters_unchanged():
    mesh, dm, lengths = _box((4, 3), ())
    ctx, U = _loaded(mesh, dm, 4)
    lat = es.lattice_of_nodes(mesh, dm, "velocity")
    n = 63
    ptr, pts = np.array([0, 10, 63], dtype=np.int32), np.arange(n, dtype=np.int32)
    try:
        # before set
        with pytest.raises(nat.NativeError, match="has not been called"):
            ctx.spectrum_info()
        ctx._spectrum_bins = 2
        with pytest.raises(nat.NativeError, match="has not been called"):
            ctx.spectrum_compute(nat.U0)
        ctx.spectrum_set(lat.shape, (None, None), lat.node_of_point, ptr, pts)
        good = ctx.spectrum_compute(nat.U0)
        info = ctx.spectrum_info()
        assert info["calls"] == 1
        bad_node = lat.node_of_point.copy()
        bad_node[5] = dm.n_p2
        neg_node = lat.node_of_point.copy()
        neg_node[0] = -1
        bad_pts = pts.copy()
        bad_pts[-1] = n
        F = np.eye(9)
        F[3, 3] = np.nan
        refused = [
            ("non-positive", lambda: ctx.spectrum_set((9, -7), (None, None), lat.node_of_point, ptr, pts)),
            ("non-positive", lambda: ctx.spectrum_set((-9, 7), (None, None), lat.node_of_point, ptr, pts)),
            ("non-positive", lambda: ctx.spectrum_set((9, 0), (None, None), lat.node_of_point, ptr, pts)),
            ("node_of_point", lambda: ctx.spectrum_set(lat.shape, (None, None), bad_node, ptr, pts)),
            ("node_of_point", lambda: ctx.spectrum_set(lat.shape, (None, None), neg_node, ptr, pts)),
            ("bin point", lambda: ctx.spectrum_set(lat.shape, (None, None), lat.node_of_point, ptr, bad_pts)),
            ("bin point", lambda: ctx.spectrum_set(lat.shape, (None, None), lat.node_of_point, ptr, -pts - 1)),
            ("bin_ptr", lambda: ctx.spectrum_set(lat.shape, (None, None), lat.node_of_point,
                                                 np.array([0, 40, 10, 63], dtype=np.int32), pts)),
            ("bin_ptr", lambda: ctx.spectrum_set(lat.shape, (None, None), lat.node_of_point,
                                                 np.array([1, 10, 63], dtype=np.int32), pts)),
            ("not finite", lambda: ctx.spectrum_set(lat.shape, (F, None), lat.node_of_point, ptr, pts)),
            ("no nodal field", lambda: ctx.spectrum_compute(nat.TRACTION)),
            ("no nodal field", lambda: ctx.spectrum_compute(nat.CONV_N1)),
            ("no nodal field", lambda: ctx.spectrum_compute(99)),
            ("no storage", lambda: ctx.spectrum_compute(nat.T1)),
            ("does not have", lambda: ctx.spectrum_compute(nat.P)),
        ]
        for match, call in refused:
            with pytest.raises(nat.NativeError, match=match):
                call()
            assert ctx.spectrum_info() == info, match
        out = np.empty(8)
        rc = ctx._lib.nsfem_spectrum_compute(ctx._h, nat.U0, out.ctypes.data_as(C.POINTER(C.c_double)), 3)
        assert rc == nat.ERR_ARG and b"wrong size" in ctx._lib.nsfem_last_error(ctx._h)
        assert ctx.spectrum_info() == info
        # the plan survived all of it
        assert ctx.spectrum_compute(nat.U0).tobytes() == good.tobytes()
        # freed: compute and info refuse again
        ctx.spectrum_set(None, None, None, None, None)
        with pytest.raises(nat.NativeError, match="has not been called"):
            ctx.spectrum_info()
    finally:
        ctx.close()


def test_a_context_with_a_communicator_is_refused():
    mesh, dm, lengths = _box((4, 3), ())
    lat = es.lattice_of_nodes(mesh, dm, "velocity")
    group = nat.local_group_create(1)
    ctx = context(mesh, dm)
    try:
        ctx.attach_local_comm(group, 0)
        with pytest.raises(nat.NativeError, match="communicator"):
            ctx.spectrum_set(lat.shape, (None, None), lat.node_of_point, np.array([0, 63], dtype=np.int32),
                             np.arange(63, dtype=np.int32))
        with pytest.raises(nat.NativeError):
            ctx.spectrum_info()
    finally:
        ctx.close()
        nat.local_group_destroy(group)


# ---------------------------------------------------------------- through the solver classes and the problem loop
TWO_PI = 2.0 * np.pi
TG_VELOCITY = ("cos(gamma * x[0]) * sin(gamma * x[1])", "-sin(gamma * x[0]) * cos(gamma * x[1])")
TG_PRESSURE = "-1.0/4.0 * (cos(2.0 * gamma * x[0]) + cos(2.0 * gamma * x[1]))"


def _taylor_green(steps, dt, hook=None):
    from ns_imex_solver import IMEXIPCSSolver
    from problem_specs import build_problem, expr
    spec = dict(name="TaylorGreenVortex", mesh=("cube", 2, 8), scheme="ipcs", numbers=dict(Re=100.0),
                clock=dict(dt=dt, steps=steps, t1=1.0), postprocessing=1,
                start={"velocity": expr(TG_VELOCITY, 3, gamma=TWO_PI), "pressure": expr(TG_PRESSURE, 3, gamma=TWO_PI)},
                bcs=[("pressure_mean", None, 0.0)], periodic=((0, 1), ("left", "right", "top", "bottom")))
    if hook is not None:
        spec["hook"] = hook
    problem = build_problem(spec)
    problem.set_solver_class(IMEXIPCSSolver)
    problem.compute_cfl = False
    return problem


def test_registered_spectrum_in_the_problem_loop_meets_the_yardstick_and_leaves_the_flow_alone():
    steps, dt = 3, 0.02
    record = []

    def hook(problem):
        solver, ts = problem._get_solver(), problem._time_stepping
        spec = problem._energy_spectrum[0]
        record.append((ts.get_next_step_size(), solver._ctx.get_state(nat.U0), spec.compute(),
                       problem._compute_energy_spectrum(field="pressure")))

    problem = _taylor_green(steps, dt, hook)
    spectrum = problem._add_energy_spectrum(every=1)
    with pytest.raises(ValueError, match="already registered"):
        problem._add_energy_spectrum()
    problem.solve_problem()
    solver = problem._get_solver()
    dm = solver._dofmap
    assert len(record) == steps and spectrum.samples == steps and abs(spectrum.weight - steps * dt) <= 1e-15
    assert spectrum.lattice.shape == (16, 16)
    with pytest.raises(ValueError, match="one plan per context"):
        es.EnergySpectrum(solver)
    mean_E, weight = 0.0, 0.0
    for k, u, res, res_p in record:
        U = u.reshape(-1, 2)
        arr = sh.lattice_array(U, dm.p2_coords, [1.0 / 16.0] * 2, (16, 16))
        want = sum(0.5 * sh.shell_spectrum(arr[..., c], (1.0, 1.0)) / 256.0 for c in range(2))
        _check(res["E"], want, (16, 16), "sample")
        assert abs(res["E"].sum() - 0.5 * (U ** 2).sum() / 256.0) <= sh.tolerance((16, 16), want.sum())
        # the vortex sits in shell rint(sqrt(2)) = 1 and decays
        assert res["E"][1] > 0.99 * res["E"].sum()
        assert res_p["E"].shape[0] >= 1 and res_p["components"].shape[1] == 1
        mean_E, weight = mean_E + k * res["E"], weight + k
    assert record[-1][2]["E"][1] < record[0][2]["E"][1]
    mean = spectrum.mean()
    # (the same raw bytes averaged before instead of after the normalisation: a dozen roundings of positive terms)
    assert np.abs(mean["E"] - mean_E / weight).max() <= 16.0 * sh.EPS * np.abs(mean_E / weight).max()
    spectrum.reset()
    assert spectrum.samples == 0 and spectrum.weight == 0.0
    # the same problem with nothing registered: the flow is bit-identical
    plain = _taylor_green(steps, dt)
    plain.solve_problem()
    with pytest.raises(nat.NativeError, match="has not been called"):
        plain._get_solver()._ctx.spectrum_info()
    for slot in (nat.U0, nat.P):
        assert solver._ctx.get_state(slot).tobytes() == plain._get_solver()._ctx.get_state(slot).tobytes()
