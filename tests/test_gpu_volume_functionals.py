"""nsfem_volume_functionals on the device (csrc/functionals.hip: k_vol_functionals<2>, <3>, k_fold_partials) against the
oracle's matrices and the numpy restatement pinned in tests/test_volume_functionals_host.py -- plain and reference
mode, cell flags, determinism, thread ranks on one GPU, and the callers: ``norm`` / ``errornorm`` of the dolfin shim
and ``ProblemBase._compute_flow_diagnostics``.

Tolerance of every comparison of integrals: 1e-12 relative to the sum of the absolute per-cell contributions -- the
worst case cells * 2^-53 of a recursive sum over <= 4096 cells, doubled for the oracle's own rounding."""
import os
import threading

import numpy as np
import pytest

import _native as nat
import fem_oracle as fo
from fem_mesh import TaylorHoodDofMap, box_mesh, periodic_entity_map, rectangle_mesh
from gpu_common import box, cavity_bc, context
from test_volume_functionals_host import (N_FUNCTIONALS, NAMES, oracle_values, smooth_fields, vol_functionals_numpy)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
TOL = 1e-12
KEYS = ("measure", "u_l2_sq", "grad_u_l2_sq", "curl_l2_sq", "div_l2_sq", "momentum", "p_integral", "p_l2_sq",
        "grad_p_l2_sq")


def _periodic_square(n):
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


def _mesh(name):
    import grid_generator as gg
    from mesh_io import read_msh
    if name == "rectangle":
        mesh = rectangle_mesh((0.0, 0.0), (1.5, 1.0), 24, 16)
    elif name == "graded":
        mesh = rectangle_mesh((0.0, 0.0), (1.0, 0.75), 16, 12)
        x = mesh.coords[:, 0] * 16.0
        mesh.coords[:, 0] = np.where(x <= 8, x / 32.0, 0.25 + (x - 8) / 16.0)
    elif name == "fixture":
        mesh = read_msh(os.path.join(HERE, "golden", "square_v41.msh"))[0]
    elif name == "periodic":
        return _periodic_square(16)
    elif name == "box":
        mesh = box_mesh((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 4, 4, 4)
    elif name == "shell":
        mesh = gg.spherical_shell(3, (0.4, 1.0), 8)[0]
    else:
        raise ValueError(name)
    return mesh, TaylorHoodDofMap(mesh)


MESHES = ("rectangle", "graded", "fixture", "periodic", "box", "shell")


def _setup(name):
    mesh, dm = _mesh(name)
    assert mesh.num_cells() <= 4096
    u, p = smooth_fields(dm.p2_coords, dm.p1_coords)
    u = u.ravel()
    ctx = context(mesh, dm)
    ctx.set_state(nat.U0, u)
    ctx.set_state(nat.P, p)
    return mesh, dm, ctx, u, p


def _compare(got, mesh, dm, u, p, label, flags=None):
    """device values against the oracle's matrices (where one exists and all cells are selected) and the pinned
    restatement (all 11), printing every figure before asserting"""
    val, scale = vol_functionals_numpy(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, u, p, flags)
    ref = {j: val[j] for j in range(N_FUNCTIONALS)}
    if flags is None:
        space = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
        ref.update(oracle_values(space, u, p))
    worst = 0.0
    for j in range(N_FUNCTIONALS):
        err = abs(got[j] - ref[j]) / max(scale[j], 1e-300)
        worst = max(worst, err)
        print("%s %-14s device %+.17e  reference %+.17e  error / scale %.2e" % (label, NAMES[j], got[j], ref[j], err))
    for j in range(N_FUNCTIONALS):
        assert abs(got[j] - ref[j]) <= TOL * scale[j], (label, NAMES[j], got[j], ref[j], scale[j])
    return worst


@pytest.mark.parametrize("name", MESHES)
def test_values_equal_the_oracle(name):
    mesh, dm, ctx, u, p = _setup(name)
    r = ctx.volume_functionals(nat.U0, nat.P)
    assert set(KEYS) <= set(r) and r["momentum"].shape == (dm.dim, )
    got = r["values"]
    assert got.shape == (N_FUNCTIONALS, )
    _compare(got, mesh, dm, u, p, name)
    if dm.dim == 2:
        assert got[7] == 0.0 and not np.signbit(got[7])
    assert r["measure"] == got[0] and r["u_l2_sq"] == got[1] and r["grad_u_l2_sq"] == got[2]
    assert r["curl_l2_sq"] == got[3] and r["div_l2_sq"] == got[4] and np.array_equal(r["momentum"], got[5:5 + dm.dim])
    assert r["p_integral"] == got[8] and r["p_l2_sq"] == got[9] and r["grad_p_l2_sq"] == got[10]
    # other slot pairs read those slots
    ctx.set_state(nat.U1, 2.0 * u)
    ctx.set_state(nat.P_OLD, -p)
    r2 = ctx.volume_functionals(nat.U1, nat.P_OLD)["values"]
    _compare(r2, mesh, dm, 2.0 * u, -p, name + " (U1, P_OLD)")
    ctx.close()


def test_a_second_trip_of_the_cell_loop_equals_the_restatement():
    """364 x 364 = 264,992 cells, the smallest square box with more cells than the 1024 x 256 threads of
    k_vol_functionals: 2,848 threads integrate a second cell.  Against the pinned restatement alone (the oracle's
    matrices are not formed at this size), under the file's TOL"""
    mesh = rectangle_mesh((0.0, 0.0), (1.0, 1.0), 364, 364)
    dm = TaylorHoodDofMap(mesh)
    assert mesh.num_cells() == 264992 > 1024 * 256
    u, p = smooth_fields(dm.p2_coords, dm.p1_coords)
    u = u.ravel()
    ctx = context(mesh, dm)
    ctx.set_state(nat.U0, u)
    ctx.set_state(nat.P, p)
    got = ctx.volume_functionals(nat.U0, nat.P)["values"]
    again = ctx.volume_functionals(nat.U0, nat.P)["values"]
    ctx.close()
    val, scale = vol_functionals_numpy(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, u, p, None)
    for j in range(N_FUNCTIONALS):
        print("364x364 %-14s device %+.17e  reference %+.17e  error / scale %.2e" %
              (NAMES[j], got[j], val[j], abs(got[j] - val[j]) / max(scale[j], 1e-300)))
    for j in range(N_FUNCTIONALS):
        assert abs(got[j] - val[j]) <= TOL * scale[j], (NAMES[j], got[j], val[j], scale[j])
    assert got.tobytes() == again.tobytes()


@pytest.mark.parametrize("name", MESHES)
def test_reference_mode(name):
    mesh, dm, ctx, u, p = _setup(name)
    plain = ctx.volume_functionals(nat.U0, nat.P)["values"]
    same = ctx.volume_functionals(nat.U0, nat.P, ref_velocity=u, ref_pressure=p)["values"]
    assert same[0] == plain[0]
    assert np.array_equal(same[1:], np.zeros(N_FUNCTIONALS - 1)), same
    rng = np.random.default_rng(5)
    v = u + 1e-3 * rng.standard_normal(u.size)
    q = p + 1e-3 * rng.standard_normal(p.size)
    got = ctx.volume_functionals(nat.U0, nat.P, ref_velocity=v, ref_pressure=q)["values"]
    _compare(got, mesh, dm, u - v, p - q, name + " (u - v)")
    # one reference only: the other field stays the state's
    got = ctx.volume_functionals(nat.U0, nat.P, ref_velocity=v)["values"]
    _compare(got, mesh, dm, u - v, p, name + " (u - v, p)")
    got = ctx.volume_functionals(nat.U0, nat.P, ref_pressure=q)["values"]
    _compare(got, mesh, dm, u, p - q, name + " (u, p - q)")
    ctx.close()


def _all_slots(ctx):
    out = []
    for slot in range(11):
        n = ctx.state_size(slot)
        out.append(ctx.get_state(slot) if n > 0 else np.zeros(0))
    return out


@pytest.mark.parametrize("name", ["fixture", "shell"])
def test_two_calls_return_the_same_bytes_and_write_no_state(name):
    mesh, dm, ctx, u, p = _setup(name)
    rng = np.random.default_rng(11)
    for slot in (nat.U1, nat.U2, nat.USTAR):
        ctx.set_state(slot, rng.standard_normal(u.size))
    for slot in (nat.P_OLD, nat.P2_OLD):
        ctx.set_state(slot, rng.standard_normal(p.size))
    before = _all_slots(ctx)
    flags = (rng.random(mesh.num_cells()) < 0.5).astype(np.uint8)
    a = ctx.volume_functionals(nat.U0, nat.P)["values"]
    b = ctx.volume_functionals(nat.U0, nat.P)["values"]
    assert a.tobytes() == b.tobytes()
    c = ctx.volume_functionals(nat.U0, nat.P, ref_velocity=0.5 * u, ref_pressure=2.0 * p, cell_flags=flags)["values"]
    d = ctx.volume_functionals(nat.U0, nat.P, ref_velocity=0.5 * u, ref_pressure=2.0 * p, cell_flags=flags)["values"]
    assert c.tobytes() == d.tobytes()
    assert ctx.volume_functionals(nat.U0, nat.P)["values"].tobytes() == a.tobytes()
    after = _all_slots(ctx)
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    ctx.close()


def test_ten_cavity_steps_with_a_call_after_each_equal_ten_steps_without():
    def run(call):
        mesh, dm, marks = box(16, 16)
        ctx = context(mesh, dm)
        ctx.set_coeffs(1.0, 1.0, 0.01)
        ctx.set_dirichlet(nat.VELOCITY, *cavity_bc(dm, marks))
        ctx.set_dirichlet(nat.PRESSURE, np.zeros(0, np.int32), np.zeros(0))
        energies = []
        for step in range(10):
            ctx.set_bdf((1.0, -1.0, 0.0) if step == 0 else (1.5, -2.0, 0.5), 0.01)
            ctx.step_ipcs()
            if call:
                energies.append(ctx.volume_functionals(nat.U0, nat.P, ref_velocity=ctx.get_state(nat.U1))["u_l2_sq"])
                energies.append(ctx.volume_functionals(nat.U0, nat.P)["u_l2_sq"])
            ctx.advance(0)
        out = [ctx.get_state(s) for s in (nat.U0, nat.U1, nat.U2, nat.P, nat.P_OLD)]
        ctx.close()
        return out, energies
    with_calls, energies = run(True)
    without, _ = run(False)
    for a, b in zip(with_calls, without):
        assert a.tobytes() == b.tobytes()
    assert all(e > 0.0 for e in energies[1::2])


@pytest.mark.parametrize("name", ["fixture", "box"])
def test_flags_and_their_complement_sum_to_the_whole(name):
    mesh, dm, ctx, u, p = _setup(name)
    rng = np.random.default_rng(3)
    flags = np.zeros(mesh.num_cells(), dtype=np.uint8)
    flags[rng.permutation(mesh.num_cells())[: mesh.num_cells() // 2]] = 1
    whole = ctx.volume_functionals(nat.U0, nat.P)["values"]
    a = ctx.volume_functionals(nat.U0, nat.P, cell_flags=flags)["values"]
    _compare(a, mesh, dm, u, p, name + " (half)", flags=flags)
    # the same host array with new contents: the resident flags must follow the contents, not the pointer
    flags[:] = 1 - flags
    b = ctx.volume_functionals(nat.U0, nat.P, cell_flags=flags)["values"]
    _compare(b, mesh, dm, u, p, name + " (complement)", flags=flags)
    fresh = ctx.volume_functionals(nat.U0, nat.P, cell_flags=flags.copy())["values"]
    assert fresh.tobytes() == b.tobytes()
    _, scale = vol_functionals_numpy(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, u, p)
    for j in range(N_FUNCTIONALS):
        assert abs(a[j] + b[j] - whole[j]) <= TOL * scale[j], (NAMES[j], a[j], b[j], whole[j])
    none = ctx.volume_functionals(nat.U0, nat.P, cell_flags=np.zeros(mesh.num_cells(), np.uint8))["values"]
    assert np.array_equal(none, np.zeros(N_FUNCTIONALS))
    all_on = ctx.volume_functionals(nat.U0, nat.P, cell_flags=np.full(mesh.num_cells(), 7, np.uint8))["values"]
    assert all_on.tobytes() == whole.tobytes()
    ctx.close()


def test_wrong_slot_kind_raises():
    mesh, dm, ctx, u, p = _setup("rectangle")
    for vs, ps in ((nat.P, nat.P), (nat.U0, nat.U1), (nat.U0, 11), (-1, nat.P), (nat.P, nat.U0)):
        with pytest.raises(nat.NativeError):
            ctx.volume_functionals(vs, ps)
    with pytest.raises(ValueError):
        ctx.volume_functionals(nat.U0, nat.P, cell_flags=np.ones(3, np.uint8))
    with pytest.raises(ValueError):
        ctx.volume_functionals(nat.U0, nat.P, ref_velocity=np.zeros(5))
    assert ctx.volume_functionals(nat.U0, nat.P)["measure"] > 0.0          # the context is still usable
    ctx.close()


# ---------------------------------------------------------------- thread ranks on one GPU
def _periodic_fields(X2, X1):
    g = 2.0 * np.pi
    x, y = X2[:, 0], X2[:, 1]
    z = X2[:, 2] if X2.shape[1] == 3 else np.zeros_like(x)
    comps = [np.cos(g * x) * np.sin(g * y) + 0.3 * np.sin(g * z) + 0.2,
             -np.sin(g * x) * np.cos(g * y) * np.cos(g * z) + 0.1]
    if X2.shape[1] == 3:
        comps.append(0.5 * np.sin(g * (x + y)) * np.cos(g * z) - 0.3)
    p = np.cos(g * X1[:, 0]) + np.sin(g * X1[:, 1]) * (np.cos(g * X1[:, 2]) if X1.shape[1] == 3 else 1.0) + 0.4
    return np.stack(comps, axis=1), p


def _run_ranks(parts, fields):
    """one thread per rank: attach, state = fields at the local nodes with NOISE in the ghost entries, one call with
    the partition's flags -> the 11 values of every rank"""
    size = len(parts)
    group = nat.local_group_create(size)
    ctxs = []
    for r, part in enumerate(parts):
        pdm = part.dofmap
        c = nat.NsfemContext(part.mesh.coords, part.mesh.cells, pdm.p2_dofmap, pdm.p1_dofmap, pdm.n_p2, pdm.n_p1)
        c.attach_local_comm(group, r)
        ctxs.append(c)
    out, errors = {}, []

    def worker(r):
        try:
            part, ctx = parts[r], ctxs[r]
            part.attach(ctx)
            dm = part.dofmap
            u, p = fields(dm.p2_coords, dm.p1_coords)
            rng = np.random.default_rng(100 + r)
            g2, g1 = part.p2_ghost != 0, part.p1_ghost != 0
            assert g2.any() and g1.any()
            u[g2] = 1e3 * rng.standard_normal((int(g2.sum()), dm.dim))
            p[g1] = 1e3 * rng.standard_normal(int(g1.sum()))
            ctx.set_state(nat.U0, u.ravel())
            ctx.set_state(nat.P, p)
            before = (ctx.get_state(nat.U0), ctx.get_state(nat.P))
            a = ctx.volume_functionals(nat.U0, nat.P, cell_flags=part.owned_cell_flags())["values"]
            b = ctx.volume_functionals(nat.U0, nat.P, cell_flags=part.owned_cell_flags())["values"]
            assert a.tobytes() == b.tobytes()
            assert np.array_equal(before[0], ctx.get_state(nat.U0)) and np.array_equal(before[1], ctx.get_state(nat.P))
            out[r] = a
        except BaseException as exc:                     # a dead rank would deadlock the others
            import traceback
            traceback.print_exc()
            errors.append((r, repr(exc)))
            os._exit(17)

    threads = [threading.Thread(target=worker, args=(r, )) for r in range(size)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors
    for c in ctxs:
        c.close()
    nat.local_group_destroy(group)
    return [out[r] for r in range(size)]


def _check_ranks(label, parts, mesh, dm, fields, volume):
    u, p = fields(dm.p2_coords, dm.p1_coords)
    u = u.ravel()
    assert mesh.num_cells() <= 4096
    ctx = context(mesh, dm)
    ctx.set_state(nat.U0, u)
    ctx.set_state(nat.P, p)
    single = ctx.volume_functionals(nat.U0, nat.P)["values"]
    ctx.close()
    _, scale = vol_functionals_numpy(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, u, p)
    ranks = _run_ranks(parts, fields)
    for r, got in enumerate(ranks):
        assert got.tobytes() == ranks[0].tobytes()                      # one all-reduce: every rank holds the same sums
        for j in range(N_FUNCTIONALS):
            err = abs(got[j] - single[j]) / max(scale[j], 1e-300)
            print("%s rank %d %-14s ranks %+.17e  single %+.17e  error / scale %.2e"
                  % (label, r, NAMES[j], got[j], single[j], err))
        for j in range(N_FUNCTIONALS):
            assert abs(got[j] - single[j]) <= TOL * scale[j], (label, r, NAMES[j], got[j], single[j])
        assert abs(got[0] - volume) <= 1e-14 * volume, (label, got[0], volume)


@pytest.mark.parametrize("size", [2, 4])
def test_strips_equal_the_single_context(size):
    from partition import StripPartition
    lo, hi, nx, ny = (0.0, 0.0), (1.25, 1.0), 20, 16
    parts = [StripPartition(lo, hi, nx, ny, r, size, coarsest=2) for r in range(size)]
    mesh = rectangle_mesh(lo, hi, nx, ny)
    _check_ranks("strips/%d" % size, parts, mesh, TaylorHoodDofMap(mesh), smooth_fields, 1.25)


def test_slabs_equal_the_single_context():
    from partition import SlabPartition
    lo, hi, n = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 8
    parts = [SlabPartition(lo, hi, n, n, n, r, 2, coarsest=2) for r in range(2)]
    mesh = box_mesh(lo, hi, n, n, n)
    _check_ranks("slabs/2", parts, mesh, TaylorHoodDofMap(mesh), smooth_fields, 1.0)


def test_periodic_slabs_equal_the_single_context():
    """fields with period 1 in every direction: the function on the periodic slabs is the function on the plain box"""
    from partition import PeriodicSlabPartition
    lo, hi, n = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 8
    parts = [PeriodicSlabPartition(lo, hi, n, n, n, r, 2, coarsest=2) for r in range(2)]
    mesh = box_mesh(lo, hi, n, n, n)
    _check_ranks("periodic slabs/2", parts, mesh, TaylorHoodDofMap(mesh), _periodic_fields, 1.0)


def test_recursive_bisection_equals_the_single_context():
    import grid_generator as gg
    from partition import GraphPartition
    mesh, marks = gg.dfg_channel(2, 1)
    dm = TaylorHoodDofMap(mesh)
    parts = [GraphPartition(mesh, r, 3, marks) for r in range(3)]
    volume = float(vol_functionals_numpy(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap,
                                         np.zeros(dm.n_velocity), np.zeros(dm.n_p1))[0][0])
    _check_ranks("bisection/3", parts, mesh, dm, smooth_fields, volume)


# ---------------------------------------------------------------- through the surface
TWO_PI = 2.0 * np.pi
TG_VELOCITY = ("amp * cos(gamma * x[0]) * sin(gamma * x[1])", "-amp * sin(gamma * x[0]) * cos(gamma * x[1])")
TG_PRESSURE = "-amp * amp / 4.0 * (cos(2.0 * gamma * x[0]) + cos(2.0 * gamma * x[1]))"


def _taylor_green(n, steps, dt, hook=None):
    from problem_specs import build_problem, expr
    spec = dict(name="TaylorGreenVortex", mesh=("cube", 2, n), scheme="bdf", numbers=dict(Re=100.0),
                clock=dict(dt=dt, steps=steps, t1=dt * steps), postprocessing=1,
                start={"velocity": expr(TG_VELOCITY, 3, gamma=TWO_PI, amp=1.0),
                       "pressure": expr(TG_PRESSURE, 3, gamma=TWO_PI, amp=1.0)},
                bcs=[("pressure_mean", None, 0.0)], periodic=((0, 1), ("left", "right", "top", "bottom")))
    if hook is not None:
        spec["hook"] = hook
    problem = build_problem(spec)
    problem.solve_problem()
    return problem, problem._get_solver()


def test_flow_diagnostics_in_the_hook_of_the_periodic_taylor_green_vortex():
    record, cache = [], {}

    def hook(problem):
        solver = problem._get_solver()
        dm = solver._dofmap
        if "M" not in cache:
            s = fo.Space(dm.mesh.coords, dm.mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
            cache["M"], cache["M1"] = s.vector_mass(), s.mass_p1()
        d = problem._compute_flow_diagnostics()
        u = solver._ctx.get_state(nat.U0)
        p = solver._ctx.get_state(nat.P)
        record.append((d, 0.5 * float(u @ (cache["M"] @ u)), float(p @ (cache["M1"] @ p))))

    problem, solver = _taylor_green(16, 8, 0.05, hook)
    assert len(record) >= 8
    for d, ke, p2 in record:
        assert set(d) == {"kinetic_energy", "enstrophy", "divergence_l2", "dissipation_integrand", "pressure_l2",
                          "volume"}
        print("kinetic energy %.15e (1/2 u^T M u %.15e)  enstrophy %.6e  |div u| %.3e" %
              (d["kinetic_energy"], ke, d["enstrophy"], d["divergence_l2"]))
        assert abs(d["kinetic_energy"] - ke) <= 1e-12 * ke
        assert abs(d["pressure_l2"] ** 2 - p2) <= 1e-12 * max(p2, 1e-300)
        assert abs(d["volume"] - 1.0) <= 1e-14
        assert d["enstrophy"] > 0.0 and d["dissipation_integrand"] >= 2.0 * d["enstrophy"] * (1.0 - 1e-12) - 1e-12
    energies = [d["kinetic_energy"] for d, _, _ in record]
    assert all(b < a for a, b in zip(energies, energies[1:])), energies


def test_norm_and_errornorm_are_the_device_functionals():
    """norm / errornorm(degree_rise=0) are the device functionals, bit for bit; the default errornorm (host quadrature,
    u evaluated at the points) agrees with degree_rise=0 to within the interpolation error.

    With e3 = |u - uh| (default), e0 = |Iu - uh| (degree_rise=0) and a = |u - Iu| the triangle inequality gives
    a - 2 e0 <= e3 - e0 <= a.  The difference has the rate of a (h^3 for P2: a = 6.07e-3 at n = 8 and 7.74e-4 at n = 16
    for the unit-amplitude vortex, from the host quadrature alone) only where the discrete error e0 is small against a;
    where e0 dominates, e3 - e0 is (u - Iu, Iu - uh) / e0 to first order, of either sign and of no definite rate.
    So the run is two steps of 1e-3 from the interpolated vortex: the time discretisation error has had no time to
    grow, e0 is what the first steps' projection leaves, itself O(h^3) and below a, and the difference follows the
    rate of a.  (Two steps of 0.05 at Re = 100 give e0 = 3.1e-2 / 2.1e-3, five times a at n = 8, and differences of
    8.6e-6 / 7.3e-5: no rate at all.)  Measured on an MI355X with the short run: e0 3.746e-3 / 5.322e-4, e3 5.337e-3 /
    8.751e-4, differences 1.590e-3 / 3.428e-4, ratio 4.64."""
    import dlfn_compat as dlfn
    from problem_specs import expr
    diffs = []
    for n in (8, 16):
        problem, solver = _taylor_green(n, 2, 1e-3)
        t = problem._time_stepping.current_time
        amp = float(np.exp(-2.0 * TWO_PI ** 2 * t / 100.0))
        velocity, pressure = solver.solution.split()
        ctx, dm = solver._ctx, solver._dofmap
        exact_u = dlfn.Expression(TG_VELOCITY, degree=3, gamma=TWO_PI, amp=amp)
        exact_p = dlfn.Expression(TG_PRESSURE, degree=3, gamma=TWO_PI, amp=amp)
        r = ctx.volume_functionals(nat.U0, nat.P)
        assert dlfn.norm(velocity) == np.sqrt(r["u_l2_sq"])
        assert dlfn.norm(velocity, "H10") == np.sqrt(r["grad_u_l2_sq"])
        assert dlfn.norm(velocity, "H1") == np.sqrt(r["u_l2_sq"] + r["grad_u_l2_sq"])
        assert dlfn.norm(pressure, "L2") == np.sqrt(r["p_l2_sq"])
        assert dlfn.norm(pressure, "H10") == np.sqrt(r["grad_p_l2_sq"])
        iu = np.asarray(exact_u.eval_at(dm.p2_coords), dtype=np.float64).ravel()
        ip = np.asarray(exact_p.eval_at(dm.p1_coords), dtype=np.float64)
        e = ctx.volume_functionals(nat.U0, nat.P, ref_velocity=iu, ref_pressure=ip)
        assert dlfn.errornorm(exact_u, velocity, degree_rise=0) == np.sqrt(e["u_l2_sq"])
        assert dlfn.errornorm(exact_u, velocity, "H1", degree_rise=0) == np.sqrt(e["u_l2_sq"] + e["grad_u_l2_sq"])
        assert dlfn.errornorm(exact_p, pressure, "L2", degree_rise=0) == np.sqrt(e["p_l2_sq"])
        assert dlfn.errornorm(exact_p, pressure, "H10", degree_rise=0) == np.sqrt(e["grad_p_l2_sq"])
        e0 = dlfn.errornorm(exact_u, velocity, degree_rise=0)
        e3 = dlfn.errornorm(exact_u, velocity)                         # dolfin's default: the host quadrature path
        print("n = %d: errornorm degree_rise 0 %.6e, default %.6e, difference %.3e" % (n, e0, e3, abs(e3 - e0)))
        diffs.append(abs(e3 - e0))
        with pytest.raises(ValueError):
            dlfn.norm(velocity, "Linf")
    assert diffs[0] > 4.0 * diffs[1], diffs
