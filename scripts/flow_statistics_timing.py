"""Timing record of the running flow statistics (csrc/statistics.hip).

For every case -- cavity Re = 100 at n x n (2D) and the triple-periodic Taylor-Green vortex at n^3 (3D), IPCS through
InstationaryProblem with throughput settings -- `steps` time steps with ONE statistics sample per step (registered
with ProblemBase._add_flow_statistics), then, on the final state:

* wall clock of one device sample (nsfem_stats_sample followed by a synchronise, average of `reps` calls),
* the route it replaces: get_state of U0 and P plus the same Welford / Chan update in numpy on the host,
* the algorithmic bytes of one k_stats_update launch.

One JSON line per case on stdout.  Kernel times: run this script under `rocprofv3 --kernel-trace --stats` in a run of
its own and read the rows of k_stats_update and of the project's vector kernels in the same trace.

    python scripts/flow_statistics_timing.py --case cavity --n 512 --steps 12
    python scripts/flow_statistics_timing.py --case tgv3d --n 64 --steps 12
"""
import argparse
import contextlib
import io
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "navierstokes-with-fenics_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

import _native as nat  # noqa: E402
from problem_specs import build_problem, expr  # noqa: E402
from test_flow_statistics_host import RunningStats  # noqa: E402  (the pinned numpy restatement of the update)


def spec(case, n, dt, steps):
    clock = dict(dt=dt, steps=steps, t1=1.0e3)
    if case == "cavity":
        return dict(name="Cavity", mesh=("cube", 2, n), scheme="ipcs", numbers=dict(Re=100.0), clock=clock, output=0,
                    start={"velocity": (0.0, 0.0), "pressure": 0.0},
                    bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_slip", "bottom"),
                         ("velocity", "top", (1.0, 0.0))])
    if case == "tgv3d":
        g = 2.0 * np.pi
        return dict(name="TaylorGreenVortex3D", mesh=("cube", 3, n), scheme="ipcs", numbers=dict(Re=100.0),
                    clock=clock, output=0,
                    start={"velocity": expr(("cos(gamma*x[0])*sin(gamma*x[1])", "-sin(gamma*x[0])*cos(gamma*x[1])",
                                             "0.0"), 3, gamma=g),
                           "pressure": expr("-0.25*(cos(2.0*gamma*x[0])+cos(2.0*gamma*x[1]))", 3, gamma=g)},
                    bcs=[("pressure_mean", None, 0.0)],
                    periodic=((0, 1, 2), ("left", "right", "top", "bottom", "back", "front")))
    raise ValueError(case)


def run(args, case):
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        problem = build_problem(spec(case, args.n, args.dt, args.steps))
        problem._write_xdmf_file = lambda current_time=0.0: None
        problem.compute_cfl = False
        problem.solver_settings = "throughput"
        stats = problem._add_flow_statistics()
        problem.solve_problem()
    solver = problem._get_solver()
    ctx, dm = solver._ctx, solver._dofmap
    dim = dm.dim
    info = ctx.stats_info()
    assert info["samples"] == info["launches"] == args.steps
    ctx.synchronize()
    t0 = time.perf_counter()
    for _ in range(args.reps):
        stats.sample(args.dt)
        ctx.synchronize()
    device_ms = 1e3 * (time.perf_counter() - t0) / args.reps
    # the host route: two copies and the same update in numpy
    s2, s1 = RunningStats(), RunningStats()
    copy_ms, numpy_ms = [], []
    for _ in range(3):
        t0 = time.perf_counter()
        u, p = ctx.get_state(nat.U0), ctx.get_state(nat.P)
        t1 = time.perf_counter()
        s2.update(u.reshape(-1, dim), args.dt)
        s1.update(p[:, None], args.dt)
        t2 = time.perf_counter()
        copy_ms.append(1e3 * (t1 - t0))
        numpy_ms.append(1e3 * (t2 - t1))
    ncov = dim * (dim + 1) // 2
    bytes_p2 = 8 * (dim + 2 * (dim + ncov))
    return dict(case=case, n=args.n, dim=dim, n_p2=dm.n_p2, n_p1=dm.n_p1, steps=args.steps, samples=info["samples"],
                accumulator_bytes=info["bytes"], device_sample_wall_ms=device_ms,
                host_route_copy_ms=min(copy_ms), host_route_numpy_ms=min(numpy_ms),
                bytes_per_p2_node=bytes_p2, bytes_per_p1_node=8 * 5,
                update_bytes=bytes_p2 * dm.n_p2 + 40 * dm.n_p1, copied_bytes=8 * (dim * dm.n_p2 + dm.n_p1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=("cavity", "tgv3d"))
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--steps", type=int, default=12)
    ap.add_argument("--dt", type=float, default=1.0e-3)
    ap.add_argument("--reps", type=int, default=20)
    args = ap.parse_args()
    for case in args.case or ["cavity"]:
        print(json.dumps(run(args, case)), flush=True)


if __name__ == "__main__":
    main()
