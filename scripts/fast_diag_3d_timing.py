"""Times the 3D projection-step solvers through the solver classes: poisson_solver = "fast_diagonalization" (the tensor
solve of csrc/fastdiag.hip, direct or as a CG preconditioner) against "multigrid" (CG with the pressure V-cycle).

For every case and solver: ms per time step (IPCSSolver.solve() + advance inside the InstationaryProblem loop, after
the warm-up steps of solve_problem()), the projection solve alone (nsfem_solve on the assembled Poisson system of the
last step, same start vector every repetition) with its iteration count, and the 3D factors' info.  One JSON line per
(case, solver) on stdout; the kernel times of one tensor solve come from a rocprofv3 --kernel-trace --stats run of
this script (k_fd_gemm / k_fd_gemm_batched rows).

    python scripts/fast_diag_3d_timing.py --case tgv3d --n 64 --steps 20 --warmup 3
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


def spec(case, n, dt, steps):
    clock = dict(dt=dt, steps=steps, t1=1.0e3)
    if case == "tgv3d":
        g = 2.0 * np.pi
        return dict(name="TaylorGreenVortex3D", mesh=("cube", 3, n), scheme="ipcs", numbers=dict(Re=100.0),
                    clock=clock, output=0,
                    start={"velocity": expr(("cos(gamma*x[0])*sin(gamma*x[1])", "-sin(gamma*x[0])*cos(gamma*x[1])",
                                             "0.0"), 3, gamma=g),
                           "pressure": expr("-0.25*(cos(2.0*gamma*x[0])+cos(2.0*gamma*x[1]))", 3, gamma=g)},
                    bcs=[("pressure_mean", None, 0.0)],
                    periodic=((0, 1, 2), ("left", "right", "top", "bottom", "back", "front")))
    if case == "cavity":
        return dict(name="Cavity3D", mesh=("cube", 3, n), scheme="ipcs", numbers=dict(Re=100.0), clock=clock,
                    output=0, start={"velocity": (0.0, 0.0, 0.0), "pressure": 0.0},
                    bcs=[("no_slip", s) for s in ("left", "right", "bottom", "top", "back")] +
                    [("velocity", "front", (1.0, 0.0, 0.0))])
    if case == "channel":
        return dict(name="ChannelFlow3D", mesh=("rectangle", (0.0, 0.0, 0.0), (2.0, 1.0, 1.0), (2 * n, n, n)),
                    scheme="ipcs", numbers=dict(Re=100.0), clock=clock, output=0,
                    start={"velocity": (0.0, 0.0, 0.0), "pressure": 0.0},
                    bcs=[("pressure", "right", 0.0),
                         ("velocity_function", "left", expr(("16.0*x[1]*(1.0-x[1])*x[2]*(1.0-x[2])", "0.0", "0.0")))] +
                    [("no_slip", s) for s in ("bottom", "top", "back", "front")])
    raise ValueError(case)


def run(args, case, poisson_solver):
    log = io.StringIO()
    with contextlib.redirect_stdout(log):
        problem = build_problem(spec(case, args.n, args.dt, args.warmup))
        problem._write_xdmf_file = lambda current_time=0.0: None
        settings = dict(poisson_solver=poisson_solver)
        if args.throughput:
            settings.update(krylov_rtol=1.0e-8, newton_forcing=1.0e-4, pressure_start="extrapolated")
        problem.solver_settings = settings
        t0 = time.perf_counter()
        problem.solve_problem()                     # set-up + warm-up steps
        t_setup = time.perf_counter() - t0
        solver, ts = problem._get_solver(), problem._time_stepping
        ctx = solver._ctx
        ctx.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.steps):
            problem._set_next_step_size()
            ts.update_coefficients()
            solver.solve()
            ts.advance_time()
            solver.advance_time()
        ctx.synchronize()
        ms_step = 1e3 * (time.perf_counter() - t0) / args.steps
        last = getattr(solver, "last_step_info", None)
        poisson_its = last.krylov_iterations_poisson if last is not None else -1
        # the projection solve alone: the Poisson system of the last step, assembled again before every repetition
        # (start vector p_old), solved with the option's preconditioner
        precond = 3 if (poisson_solver == "fast_diagonalization" and solver._fast_diagonalization_ready()) else 1
        rtol = solver.krylov_rtol
        times, its = [], []
        for rep in range(args.solve_reps + 2):
            ctx.assemble(nat.SYS_POISSON)
            ctx.synchronize()
            t0 = time.perf_counter()
            info = ctx.solve(nat.SYS_POISSON, rtol=rtol, precond=precond)
            ctx.synchronize()
            if rep >= 2:
                times.append(1e3 * (time.perf_counter() - t0))
                its.append(info.iterations)
        info3 = ctx.poisson_fast_diag_3d_info()
        ctx.close()
    return {"case": case, "n": args.n, "poisson_solver": poisson_solver, "n_p1": int(solver._dofmap.n_p1),
            "n_dofs": int(solver._dofmap.n_dofs), "ms_per_step": ms_step, "steps": args.steps, "warmup": args.warmup,
            "poisson_iterations_last_step": int(poisson_its), "projection_solve_ms_median": float(np.median(times)),
            "projection_solve_ms_min": float(np.min(times)), "projection_solve_iterations": its,
            "precond": precond, "krylov_rtol": rtol, "fast_diag_3d": info3, "setup_and_warmup_s": t_setup}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("tgv3d", "cavity", "channel"), action="append")
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--dt", type=float, default=0.25 / 64)
    ap.add_argument("--solve-reps", type=int, default=10)
    ap.add_argument("--solver", choices=("fast_diagonalization", "multigrid"), action="append")
    ap.add_argument("--throughput", action="store_true", help="Krylov rtol 1e-8, inexact Newton, extrapolated start")
    args = ap.parse_args()
    for case in args.case or ["tgv3d", "cavity"]:
        for s in args.solver or ["fast_diagonalization", "multigrid"]:
            print(json.dumps(run(args, case, s)), flush=True)


if __name__ == "__main__":
    main()
