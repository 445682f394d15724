"""Timing record of the Lagrangian-averaged dynamic Smagorinsky model (mode 1 of nsfem_set_dynamic_averaging, DESIGN.md
4w); the output goes to profiles/dynamic_lagrangian_timing.txt.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/dynamic_lagrangian_timing.py kernels
        ``--reps`` runs of the procedure of law 8 with the global group (k_dyn_moments, k_dyn_vertex, k_dyn_reduce,
        through nsfem_dynamic_constant) and then ``--reps`` applications of the Lagrangian rules (k_dyn_moments,
        k_dyn_vertex, k_dyn_lagrange, through nsfem_dynamic_lagrangian_advance on a stored state) in ONE run with no
        counters, on the cavity mesh at n = 512 and on a 64^3 box, with the smooth field of the tests and a step size of
        CFL 0.4.  ``python scripts/scalar_sgs_timing.py summary DIR --match k_dyn_`` prints median, minimum and maximum per kernel
        name and grid size: k_dyn_lagrange stands beside k_dyn_reduce of the same trace.

    python scripts/dynamic_lagrangian_timing.py steps --n 512
        the lid-driven cavity on n x n squares through ``IMEXIPCSSolver`` (SBDF2) with ``throughput_settings()``,
        ``DynamicSmagorinskyModel("global")`` and ``DynamicSmagorinskyModel("lagrangian")`` alternated, ``--rounds``
        times in one process; wall clock of ``solver.solve()`` per step (synchronised), median, minimum and maximum of
        ``--steps`` steps after ``--warmup``; one JSON line per case.

The headline (plain ``bench.py``, no law set) is compared by running the parent's and this build alternately.
"""
import argparse
import contextlib
import io
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, d) for d in ("navierstokes-with-fenics_amd", "tests", "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

os.environ.setdefault("NSFEM_NO_OUTPUT", "1")      # no XDMF files: the run is a timing


def run_kernels(args):
    import numpy as np
    import _native as nat
    from gpu_common import box, context
    from test_gpu_3d import box3, context3
    from test_scalar_transport_host import smooth_fields
    cases = [("2d", lambda: box(args.n, args.n), context, 1.0 / args.n),
             ("3d", lambda: box3((args.n3, ) * 3), context3, 1.0 / args.n3)]
    for tag, make_mesh, make_ctx, h in cases:
        mesh, dm, marks = make_mesh()
        u, _ = smooth_fields(dm.p2_coords)
        k = 0.4 * h / float(np.abs(u).max())
        ctx = make_ctx(mesh, dm)
        try:
            ctx.set_state(nat.U1, u)
            ctx.set_viscosity_law(8, (args.alpha, args.cs2_max))
            for _ in range(args.reps):
                cs2 = ctx.dynamic_constant(nat.U1)
            ctx.set_dynamic_averaging(1)
            state = np.full((dm.n_p1, 4), np.nan)
            state[:, 0], state[:, 1] = 0.0256, 1.0
            ctx.set_dynamic_lagrangian_state(state)
            for _ in range(args.reps):
                new, field = ctx.dynamic_lagrangian_advance(nat.U1, k)
            print(json.dumps(dict(case=tag, cells=int(mesh.cells.shape[0]), vertices=int(dm.n_p1), k=k,
                                  dynamic=ctx.dynamic_info(), cs2_global=cs2.tolist(),
                                  cs2_lagrangian=dict(min=float(field.min()), mean=float(field.mean()),
                                                      max=float(field.max())))), flush=True)
        finally:
            ctx.close()


def run_steps(args):
    from ns_imex_solver import IMEXIPCSSolver
    from problem_specs import build_problem
    from viscosity_models import DynamicSmagorinskyModel
    for round_ in range(args.rounds):
        models = (("global", DynamicSmagorinskyModel("global", args.alpha, args.cs2_max)),
                  ("lagrangian", DynamicSmagorinskyModel("lagrangian", args.alpha, args.cs2_max)))
        for name, model in models:
            spec = dict(name="cavity", mesh=("cube", 2, args.n), scheme="ipcs", numbers=dict(Re=100.0),
                        clock=dict(dt=args.dt, steps=args.warmup + args.steps),
                        start={"velocity": (0.0, 0.0), "pressure": 0.0},
                        bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_slip", "bottom"),
                             ("velocity", "top", (1.0, 0.0))])
            problem = build_problem(spec)

            # (the hook of ns_problem, on this instance alone: the problem class stays as it is)
            problem.set_viscosity_model = lambda problem=problem, model=model: setattr(problem, "_viscosity_model", model)
            problem.set_solver_class(IMEXIPCSSolver)
            problem.compute_cfl = False
            problem.solver_settings = "throughput"
            with contextlib.redirect_stdout(io.StringIO()):
                problem.solve_problem()
            solver = problem._get_solver()
            ms = [1e3 * t for t in problem.step_wall_times[args.warmup:]]
            print(json.dumps(dict(case=name, round=round_, n=args.n, dt=args.dt, steps=args.steps, warmup=args.warmup,
                                  step_ms=dict(median=statistics.median(ms), min=min(ms), max=max(ms)),
                                  imex=solver._ctx.imex_info(), viscosity=solver._ctx.viscosity_info(),
                                  dynamic=solver._ctx.dynamic_info())), flush=True)


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    p = sub.add_parser("kernels")
    p.add_argument("--n", type=int, default=512)
    p.add_argument("--n3", type=int, default=64)
    p.add_argument("--reps", type=int, default=30)
    q = sub.add_parser("steps")
    q.add_argument("--n", type=int, default=512)
    q.add_argument("--dt", type=float, default=0.5 / 512)
    q.add_argument("--steps", type=int, default=20)
    q.add_argument("--warmup", type=int, default=5)
    q.add_argument("--rounds", type=int, default=2)
    for parser in (p, q):
        parser.add_argument("--alpha", type=float, default=2.0)
        parser.add_argument("--cs2-max", dest="cs2_max", type=float, default=0.09)
    args = ap.parse_args()
    dict(kernels=run_kernels, steps=run_steps)[args.mode](args)


if __name__ == "__main__":
    main()
