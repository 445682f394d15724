"""Timing record of the heated immersed bodies (scalar penalisation in the convection kernel).

    python scripts/heated_bodies_timing.py steps --n 512
        the lid-driven cavity with a transported temperature on n x n squares through ``BoussinesqIMEXSolver`` (SBDF2)
        with ``throughput_settings()``, alternating no body, one passive disc of radius 0.1 (the flow's penalisation
        alone, eta = k) and the same disc heated (eta_scalar = k) in one process; wall clock of ``solver.solve()`` and of
        the transport step inside it (synchronised before and after) per step, median and minimum of ``--steps``
        steps after ``--warmup``; one JSON line per case.

    rocprofv3 --kernel-trace -d DIR -- python scripts/heated_bodies_timing.py kernels
        ``--reps`` dispatches each of the fused kernel (k_scalar_conv_cell<FORM, PENAL> / k3_scalar_conv_cell, through
        nsfem_body_scalar_residual), of the plain scalar convection kernel (PENAL 0, through nsfem_scalar_convection)
        and of the flow's penalisation pair (k_penal_cell / k3_penal_cell + k_visc_gather, through
        nsfem_body_residual) on the cavity at n = 512 with one disc of radius 0.1 and on a 64^3 box with one ball of
        radius 0.1, sharp and smoothed, both forms; then the heat numbers (k_body_heat + k_fold_partials).

    python scripts/heated_bodies_timing.py summary DIR
        median, minimum and maximum per kernel name and grid size of the trace under DIR, microseconds.
"""
import argparse
import contextlib
import csv
import glob
import io
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, d) for d in ("navierstokes-with-fenics_amd", "tests", "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

os.environ.setdefault("NSFEM_NO_OUTPUT", "1")      # no XDMF files: the run is a timing


def run_steps(args):
    from immersed_bodies import Ball, ImmersedBodies
    from ns_boussinesq_solver import BoussinesqIMEXSolver
    from problem_specs import build_problem

    class TimedSolver(BoussinesqIMEXSolver):
        """the transport step timed on its own: the stream is idle before it and after it"""
        transport_times = []

        def _solve_time_step(self):
            ctx = self._ctx
            real = ctx.step_scalar_imex

            def timed(*a, **kw):
                ctx.synchronize()
                t0 = time.perf_counter()
                out = real(*a, **kw)
                ctx.synchronize()
                type(self).transport_times.append(time.perf_counter() - t0)
                return out
            ctx.step_scalar_imex = timed
            try:
                super()._solve_time_step()
            finally:
                del ctx.step_scalar_imex

    for round_ in range(args.rounds):
        for name in ("plain", "passive disc", "heated disc"):
            spec = dict(name="cavity", mesh=("cube", 2, args.n), scheme="ipcs", numbers=dict(Re=100.0, Fr=1.0),
                        clock=dict(dt=args.dt, steps=args.warmup + args.steps),
                        start={"velocity": (0.0, 0.0), "pressure": 0.0, "temperature": 0.5},
                        bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_slip", "bottom"),
                             ("velocity", "top", (1.0, 0.0))])
            problem = build_problem(spec)
            cls = type(problem)

            def set_temperature_coefficients(self):
                self._temperature_coefficients = dict(diffusivity=0.01, buoyancy=(0.0, 1.0), convective_form="standard")

            def set_temperature_boundary_conditions(self):
                self._temperature_bcs = [(self._sides["left"], 1.0), (self._sides["right"], 0.0)]
            cls.set_temperature_coefficients = set_temperature_coefficients
            cls.set_temperature_boundary_conditions = set_temperature_boundary_conditions
            if name != "plain":
                disc = Ball((0.5, 0.5), 0.1, temperature=1.0 if name == "heated disc" else None)
                bodies = ImmersedBodies([disc], args.dt, args.smoothing)

                def set_immersed_bodies(self, bodies=bodies):
                    self._immersed_bodies = bodies
                cls.set_immersed_bodies = set_immersed_bodies
            TimedSolver.transport_times = []
            problem.set_solver_class(TimedSolver)
            problem.compute_cfl = False
            problem.solver_settings = "throughput"
            with contextlib.redirect_stdout(io.StringIO()):
                problem.solve_problem()
            solver = problem._get_solver()
            ms = [1e3 * t for t in problem.step_wall_times[args.warmup:]]
            tr = [1e3 * t for t in TimedSolver.transport_times[args.warmup:]]
            out = dict(case=name, round=round_, n=args.n, dt=args.dt, steps=args.steps, warmup=args.warmup,
                       step_ms=dict(median=statistics.median(ms), min=min(ms)),
                       transport_ms=dict(median=statistics.median(tr), min=min(tr)), imex=solver._ctx.imex_info(),
                       scalar=solver._ctx.scalar_info(), bodies=solver._ctx.body_info(),
                       heat_info=solver._ctx.body_heat_info(), cg_scalar=solver.last_scalar_solve.iterations)
            if name == "heated disc":
                out["heat"] = problem._compute_body_heat().tolist()
            print(json.dumps(out), flush=True)


def run_kernels(args):
    import numpy as np
    import _native as nat
    from gpu_common import box, cavity_bc, context
    from test_gpu_3d import box3, context3, lid_bc
    from test_scalar_transport_host import smooth_fields
    cases = [("2d", lambda: box(args.n, args.n), context, cavity_bc, (1, (0.5, 0.5), (0.1, ), (0.0, 0.0), 0.0)),
             ("3d", lambda: box3((args.n3, ) * 3), context3, lid_bc,
              (1, (0.5, 0.5, 0.5), (0.1, ), (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)))]
    for tag, make_mesh, make_ctx, bc, body in cases:
        mesh, dm, marks = make_mesh()
        u, T = smooth_fields(dm.p2_coords)
        ctx = make_ctx(mesh, dm)
        try:
            ctx.set_coeffs(1.0, 1.0, 0.01)
            ctx.set_dirichlet(nat.VELOCITY, *bc(dm, marks))
            ctx.set_dirichlet(nat.PRESSURE, np.zeros(0, np.int32), np.zeros(0))
            ctx.set_state(nat.U1, u)
            ctx.set_state(nat.T1, T)
            for eps in (0.0, args.smoothing):
                ctx.set_bodies([body], 1.0e-3, eps)
                ctx.set_body_temperatures([1], [1.0], 1.0e-3)
                for form in (0, 1):
                    for _ in range(args.reps):
                        ctx.body_scalar_residual(nat.U1, nat.T1, form, 1.0, 0)
                for _ in range(args.reps):
                    ctx.body_residual(nat.U1, 1.0)
                heat = ctx.body_heat(nat.T1)
                for _ in range(4):
                    ctx.body_heat(nat.T1)
                print(json.dumps(dict(case=tag, cells=int(mesh.cells.shape[0]), smoothing=eps, heat=heat.tolist())),
                      flush=True)
            for form in (0, 1):
                for _ in range(args.reps):
                    ctx.scalar_convection(nat.U1, nat.T1, form, 1.0)
        finally:
            ctx.close()


def run_summary(args):
    """per kernel name AND grid size: the 2D and the 3D mesh launch the shared kernels with different grids"""
    rows = {}
    for path in glob.glob(os.path.join(args.dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path, newline="") as fh:
            for r in csv.DictReader(fh):
                key = (r["Kernel_Name"], int(r["Grid_Size_X"]))
                rows.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) * 1e-3)
    for name, grid in sorted(rows):
        if any(w in name for w in args.match.split(",")):
            v = rows[(name, grid)]
            print("%6d  median %9.2f  min %9.2f  max %9.2f  grid %10d  %s" % (len(v), statistics.median(v), min(v), max(v),
                                                                            grid, name))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    p = sub.add_parser("steps")
    p.add_argument("--n", type=int, default=512)
    p.add_argument("--dt", type=float, default=1.0e-3)
    p.add_argument("--steps", type=int, default=30)
    p.add_argument("--warmup", type=int, default=10)
    p.add_argument("--rounds", type=int, default=2)
    p.add_argument("--smoothing", type=float, default=0.0)
    p = sub.add_parser("kernels")
    p.add_argument("--n", type=int, default=512)
    p.add_argument("--n3", type=int, default=64)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--smoothing", type=float, default=0.01)
    p = sub.add_parser("summary")
    p.add_argument("dir")
    p.add_argument("--match", default="scalar_conv_cell,scalar_gather,penal,fold_partials,visc_gather,body_heat")
    args = ap.parse_args()
    dict(steps=run_steps, kernels=run_kernels, summary=run_summary)[args.mode](args)


if __name__ == "__main__":
    main()
