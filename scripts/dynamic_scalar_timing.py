"""Timing record of the dynamic subgrid heat flux (nsfem_set_scalar_sgs_dynamic); the output goes to
profiles/dynamic_scalar_timing.txt.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/dynamic_scalar_timing.py kernels
        one run with no counters, on the cavity mesh at n = 512 and on a 64^3 box, with the smooth fields of the tests
        and the global group; ``--reps`` dispatches each of
          * the law-8 sequence k_dyn_moments, k_dyn_vertex, k_dyn_reduce (through nsfem_dynamic_constant), the yardstick
            of the procedure kernels,
          * k_scalar_conv_cell<0, 0, 1> / k3_scalar_conv_cell (law 1 with a fixed Pr_t, through nsfem_scalar_explicit),
            the yardstick of the element kernel,
          * k_dyn_scalar_moments, k_dyn_scalar_vertex, k_dyn_reduce, k_scalar_conv_cell<0, 0, 8> (the dynamic switch,
            through nsfem_scalar_explicit).
        ``python scripts/dynamic_scalar_timing.py summary DIR`` prints median, minimum and maximum per kernel name and
        grid size (k_dyn_reduce appears once: the velocity and the scalar procedure launch the same kernel).

    python scripts/dynamic_scalar_timing.py steps --n 512
        the heated lid-driven cavity on n x n squares through ``BoussinesqIMEXSolver`` (SBDF2) with
        ``throughput_settings()``, ``DynamicSmagorinskyModel()`` without and with ``heat_flux="dynamic"`` in turn,
        ``--rounds`` times in one process; wall clock of ``solver.solve()`` per step (transport step and flow step,
        synchronised), median, minimum and maximum of ``--steps`` steps after ``--warmup``; one JSON line per case.

The headline (plain ``bench.py``, which sets no scalar) is compared by running the parent's and this build alternately.
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
        u, T = smooth_fields(dm.p2_coords)
        ctx = make_ctx(mesh, dm)
        try:
            ctx.set_state(nat.U1, u)
            ctx.set_state(nat.T1, T)
            ctx.set_viscosity_law(8, (args.alpha, args.cs2_max))
            for _ in range(args.reps):
                ctx.dynamic_constant(nat.U1)
            ctx.set_viscosity_law(1, (args.cs, ))
            ctx.set_scalar_sgs(args.prandtl_t)
            for _ in range(args.reps):
                ctx.scalar_explicit(nat.U1, nat.T1, 0, 1.0)
            ctx.set_scalar_sgs(0.0)
            ctx.set_viscosity_law(8, (args.alpha, args.cs2_max))
            ctx.set_scalar_sgs_dynamic(True, args.ctheta_max)
            for _ in range(args.reps):
                ctx.scalar_explicit(nat.U1, nat.T1, 0, 1.0)
            print(json.dumps(dict(case=tag, cells=int(mesh.cells.shape[0]), sgs=ctx.scalar_sgs_info(),
                                  dynamic=ctx.dynamic_info(), scalar_dynamic=ctx.scalar_dynamic_info(),
                                  ctheta=ctx.scalar_dynamic_constant(nat.U1, nat.T1).tolist())), flush=True)
        finally:
            ctx.close()


def run_steps(args):
    from ns_boussinesq_solver import BoussinesqIMEXSolver
    from problem_specs import build_problem
    from viscosity_models import DynamicSmagorinskyModel
    for round_ in range(args.rounds):
        models = (("dynamic viscosity alone", DynamicSmagorinskyModel("global", args.alpha, args.cs2_max)),
                  ("with the dynamic heat flux", DynamicSmagorinskyModel("global", args.alpha, args.cs2_max,
                                                                         heat_flux="dynamic", ctheta_max=args.ctheta_max)))
        for name, model in models:
            spec = dict(name="cavity", mesh=("cube", 2, args.n), scheme="ipcs", numbers=dict(Re=100.0, Fr=1.0),
                        clock=dict(dt=args.dt, steps=args.warmup + args.steps),
                        start={"velocity": (0.0, 0.0), "pressure": 0.0, "temperature": 0.5},
                        bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_slip", "bottom"),
                             ("velocity", "top", (1.0, 0.0))])
            problem = build_problem(spec)
            cls = type(problem)

            def set_viscosity_model(self, model=model):
                self._viscosity_model = model

            def set_temperature_coefficients(self):
                self._temperature_coefficients = dict(diffusivity=args.kappa, buoyancy=(0.0, 1.0),
                                                      convective_form="standard")

            def set_temperature_boundary_conditions(self):
                self._temperature_bcs = [(self._sides["left"], 1.0), (self._sides["right"], 0.0)]
            cls.set_viscosity_model = set_viscosity_model
            cls.set_temperature_coefficients = set_temperature_coefficients
            cls.set_temperature_boundary_conditions = set_temperature_boundary_conditions
            problem.set_solver_class(BoussinesqIMEXSolver)
            problem.compute_cfl = False
            problem.solver_settings = "throughput"
            with contextlib.redirect_stdout(io.StringIO()):
                problem.solve_problem()
            ctx = problem._get_solver()._ctx
            ms = [1e3 * t for t in problem.step_wall_times[args.warmup:]]
            print(json.dumps(dict(case=name, round=round_, n=args.n, dt=args.dt, steps=args.steps, warmup=args.warmup,
                                  step_ms=dict(median=statistics.median(ms), min=min(ms), max=max(ms)),
                                  scalar=ctx.scalar_info(), sgs=ctx.scalar_sgs_info(), dynamic=ctx.dynamic_info(),
                                  scalar_dynamic=ctx.scalar_dynamic_info())), flush=True)


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
            print("%6d  median %9.2f  min %9.2f  max %9.2f us  grid %10d  %s" % (
                len(v), statistics.median(v), min(v), max(v), grid, name))


def main():
    ap = argparse.ArgumentParser()
    sub = ap.add_subparsers(dest="mode", required=True)
    p = sub.add_parser("kernels")
    p.add_argument("--n", type=int, default=512)
    p.add_argument("--n3", type=int, default=64)
    p.add_argument("--reps", type=int, default=30)
    p.add_argument("--cs", type=float, default=0.17)
    p.add_argument("--prandtl-t", dest="prandtl_t", type=float, default=0.85)
    q = sub.add_parser("steps")
    q.add_argument("--n", type=int, default=512)
    q.add_argument("--dt", type=float, default=0.5 / 512)
    q.add_argument("--steps", type=int, default=30)
    q.add_argument("--warmup", type=int, default=10)
    q.add_argument("--rounds", type=int, default=2)
    q.add_argument("--kappa", type=float, default=0.01)
    for parser in (p, q):
        parser.add_argument("--alpha", type=float, default=2.0)
        parser.add_argument("--cs2-max", dest="cs2_max", type=float, default=0.09)
        parser.add_argument("--ctheta-max", dest="ctheta_max", type=float, default=0.2)
    r = sub.add_parser("summary")
    r.add_argument("dir")
    r.add_argument("--match", default="k_dyn_,scalar_conv_cell,scalar_gather")
    args = ap.parse_args()
    dict(kernels=run_kernels, steps=run_steps, summary=run_summary)[args.mode](args)


if __name__ == "__main__":
    main()
