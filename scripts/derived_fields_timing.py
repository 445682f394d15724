"""Timing record of the device-side derived fields (csrc/derived.hip).

The n x n lid-driven cavity (Re = 100, IPCS through InstationaryProblem with throughput settings) is advanced `steps`
time steps; then, on the final state, alternating between the two routes `reps` times after `warmup` untimed rounds:

* wall clock of one ``derived_fields(vorticity | q criterion, NODE)`` call, read-back included (the call ends in a
  stream synchronise),
* wall clock of the present ``ProblemBase._compute_vorticity()``: get_state of U0 plus the numpy einsums,
* and of the other centres and of all seven quantities at once, for the record.

One JSON line on stdout (milliseconds: median and minimum of the repetitions).

    python scripts/derived_fields_timing.py --n 512 --steps 6
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "navierstokes-with-fenics_amd"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

import _native as nat  # noqa: E402
from problem_specs import build_problem  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--steps", type=int, default=6)
    ap.add_argument("--dt", type=float, default=1.0e-3)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    spec = dict(name="Cavity", mesh=("cube", 2, args.n), scheme="ipcs", numbers=dict(Re=100.0),
                clock=dict(dt=args.dt, steps=args.steps, t1=1.0e3), output=0,
                start={"velocity": (0.0, 0.0), "pressure": 0.0},
                bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_slip", "bottom"), ("velocity", "top", (1.0, 0.0))])
    with contextlib.redirect_stdout(io.StringIO()):
        problem = build_problem(spec)
        problem._write_xdmf_file = lambda current_time=0.0: None
        problem.compute_cfl = False
        problem.solver_settings = "throughput"
        problem.solve_problem()
    solver = problem._get_solver()
    ctx, dm = solver._ctx, solver._dofmap
    ctx.synchronize()
    all_q = tuple(range(nat.N_DERIVED - 1))          # (no scalar in this run)
    pair = (nat.DERIVED_VORTICITY, nat.DERIVED_Q_CRITERION)
    routes = {
        "device_vorticity_q_node_ms": lambda: ctx.derived_fields(pair, nat.DERIVED_NODE),
        "host_compute_vorticity_ms": lambda: problem._compute_vorticity(),
        "device_vorticity_cell_ms": lambda: ctx.derived_fields(nat.DERIVED_VORTICITY, nat.DERIVED_CELL),
        "device_vorticity_vertex_ms": lambda: ctx.derived_fields(nat.DERIVED_VORTICITY, nat.DERIVED_VERTEX),
        "device_six_quantities_node_ms": lambda: ctx.derived_fields(all_q, nat.DERIVED_NODE),
        "host_get_state_u0_ms": lambda: ctx.get_state(nat.U0),
    }
    times = {k: [] for k in routes}
    for rep in range(args.warmup + args.reps):
        for key, fn in routes.items():              # alternating: every round times every route once
            t = timed(fn)
            if rep >= args.warmup:
                times[key].append(t)
    # the two routes compute the same vorticity
    dev = ctx.derived_fields(nat.DERIVED_VORTICITY, nat.DERIVED_VERTEX)[nat.DERIVED_VORTICITY]
    host = problem._compute_vorticity().vertex_values
    out = dict(case="cavity", n=args.n, n_cells=int(dm.mesh.cells.shape[0]), n_p2=int(dm.n_p2), steps=args.steps,
               warmup=args.warmup, reps=args.reps, work_buffer_bytes=ctx.derived_info()["bytes"],
               state_bytes_velocity=8 * 2 * int(dm.n_p2),
               vertex_vorticity_max_difference=float(np.abs(dev - host).max()),
               vertex_vorticity_max=float(np.abs(host).max()))
    for key, v in times.items():
        out[key] = dict(median=statistics.median(v), min=min(v))
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
