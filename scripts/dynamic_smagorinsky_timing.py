"""Timing record of the dynamic Smagorinsky model (law 8 of nsfem_set_viscosity_law); the output goes to
profiles/dynamic_smagorinsky_timing.txt.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/dynamic_smagorinsky_timing.py kernels
        ``--reps`` dispatches each of k_visc_var_cell<1, false> / k3_visc_var_cell (law 1, the yardstick) and of the
        law-8 sequence k_dyn_moments, k_dyn_vertex, k_dyn_reduce, k_visc_var_cell<8, false> (through
        nsfem_viscosity_residual) in one run with no counters, on the cavity mesh at n = 512 and on a 64^3 box, with the
        smooth field of the tests and the global group.  ``python scripts/scalar_sgs_timing.py summary DIR`` prints
        median, minimum and maximum per kernel name and grid size.

    python scripts/dynamic_smagorinsky_timing.py steps --n 512
        the lid-driven cavity on n x n squares through ``IMEXIPCSSolver`` (SBDF2) with ``throughput_settings()``,
        ``SmagorinskyModel(cs)`` and ``DynamicSmagorinskyModel()`` in turn, ``--rounds`` times in one process; wall clock
        of ``solver.solve()`` per step (synchronised), median, minimum and maximum of ``--steps`` steps after
        ``--warmup``; one JSON line per case.

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
    import _native as nat
    from gpu_common import box, context
    from test_gpu_3d import box3, context3
    from test_scalar_transport_host import smooth_fields
    cases = [("2d", lambda: box(args.n, args.n), context), ("3d", lambda: box3((args.n3, ) * 3), context3)]
    for tag, make_mesh, make_ctx in cases:
        mesh, dm, marks = make_mesh()
        u, _ = smooth_fields(dm.p2_coords)
        ctx = make_ctx(mesh, dm)
        try:
            ctx.set_state(nat.U1, u)
            for law, params in ((1, (args.cs, )), (8, (args.alpha, args.cs2_max))):
                ctx.set_viscosity_law(law, params)
                for _ in range(args.reps):
                    ctx.viscosity_residual(nat.U1, 1.0)
            print(json.dumps(dict(case=tag, cells=int(mesh.cells.shape[0]), viscosity=ctx.viscosity_info(),
                                  dynamic=ctx.dynamic_info(), cs2=ctx.dynamic_constant(nat.U1).tolist())), flush=True)
        finally:
            ctx.close()


def run_steps(args):
    from ns_imex_solver import IMEXIPCSSolver
    from problem_specs import build_problem
    from viscosity_models import DynamicSmagorinskyModel, SmagorinskyModel
    for round_ in range(args.rounds):
        models = (("Smagorinsky", SmagorinskyModel(args.cs)),
                  ("dynamic", DynamicSmagorinskyModel("global", args.alpha, args.cs2_max)))
        for name, model in models:
            spec = dict(name="cavity", mesh=("cube", 2, args.n), scheme="ipcs", numbers=dict(Re=100.0),
                        clock=dict(dt=args.dt, steps=args.warmup + args.steps),
                        start={"velocity": (0.0, 0.0), "pressure": 0.0},
                        bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_slip", "bottom"),
                             ("velocity", "top", (1.0, 0.0))])
            problem = build_problem(spec)

            def set_viscosity_model(self, model=model):
                self._viscosity_model = model
            type(problem).set_viscosity_model = set_viscosity_model
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
    q.add_argument("--steps", type=int, default=30)
    q.add_argument("--warmup", type=int, default=10)
    q.add_argument("--rounds", type=int, default=2)
    for parser in (p, q):
        parser.add_argument("--cs", type=float, default=0.17)
        parser.add_argument("--alpha", type=float, default=2.0)
        parser.add_argument("--cs2-max", dest="cs2_max", type=float, default=0.09)
    args = ap.parse_args()
    dict(kernels=run_kernels, steps=run_steps)[args.mode](args)


if __name__ == "__main__":
    main()
