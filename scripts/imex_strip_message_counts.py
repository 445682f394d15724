"""Halo exchanges, all-reduces and bytes per time step of nsfem_step_ipcs and nsfem_step_imex on N in-process thread
ranks sharing one GPU: the lid-driven cavity on n x n cells cut into N strips, with the N > 1 settings of bench.py's
strong-scaling run (relaxed halo mode, levels thinner than 16 cell rows per rank replicated, fast-diagonalisation
projection, Chebyshev mass solve, Krylov rtol 1e-8, inexact Newton 1e-4, dt 1e-3, overlap on).

    python scripts/imex_strip_message_counts.py --cells 960 --ranks 2 4 8 --out profiles/r08_imex_strip_message_counts.json

The counters are the communicator's own (nsfem_comm_stats) on rank 0, averaged over the timed steps.  Message COUNTS
do not depend on the transport; the wall time of thread ranks sharing one GPU is not scaling data and is not printed."""
import argparse
import json
import os
import sys
import threading

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "navierstokes-with-fenics_amd"))

import _native as nat                       # noqa: E402
import poisson_fd                           # noqa: E402
from imex_time_stepping import IMEXTimeStepping, IMEXType   # noqa: E402
from partition import StripPartition        # noqa: E402


def cavity_dirichlet(dm):
    X = dm.p2_coords
    on = (np.abs(X[:, 0]) < 1e-12) | (np.abs(X[:, 0] - 1) < 1e-12) | (np.abs(X[:, 1]) < 1e-12) | \
        (np.abs(X[:, 1] - 1.0) < 1e-12)
    nodes = np.nonzero(on)[0]
    lid = np.abs(X[nodes, 1] - 1.0) < 1e-12
    return (np.concatenate([2 * nodes, 2 * nodes + 1]).astype(np.int32),
            np.concatenate([np.where(lid, 1.0, 0.0), np.zeros(nodes.size)]))


def run(scheme, n, size, args):
    group = nat.local_group_create(size)
    parts = [StripPartition((0.0, 0.0), (1.0, 1.0), n, n, r, size, coarsest=64, global_coarsest=8,
                            min_rows=args.min_rows) for r in range(size)]
    ctxs = []
    for r, part in enumerate(parts):
        dm = part.dofmap
        c = nat.NsfemContext(part.mesh.coords, part.mesh.cells, dm.p2_dofmap, dm.p1_dofmap, dm.n_p2, dm.n_p1)
        c.attach_local_comm(group, r)
        ctxs.append(c)
    out = {}

    def worker(r):
        try:
            part, ctx = parts[r], ctxs[r]
            dm = part.dofmap
            part.attach(ctx)
            ctx.set_coeffs(1.0, 1.0, 1.0 / 100.0)
            ctx.set_dirichlet(nat.VELOCITY, *cavity_dirichlet(dm))
            ctx.set_dirichlet(nat.PRESSURE, np.zeros(0, np.int32), np.zeros(0))
            ctx.mg_set_truncation(4.0, 0.1)
            ctx.mg_set_halo_mode(args.halo_mode)
            ctx.set_overlap(True)
            xs = np.linspace(0.0, 1.0, n + 1)
            ctx.poisson_set_fast_diag(poisson_fd.factors(xs, xs, np.zeros(0, np.int64)),
                                      first_line=int(part.p1_global[0]) // (n + 1))
            o = ctx.default_step_opts()
            for k in (o.momentum, o.poisson, o.correction):
                k.rtol = args.krylov_rtol
            o.momentum.precond = 1
            o.poisson.precond = 3
            o.correction.precond = 2
            o.newton_forcing = 1.0e-4
            o.pressure_extrapolation = 1
            ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=args.dt)
            its = np.zeros(4)
            for i in range(args.warmup + args.steps):
                if i == args.warmup:
                    ctx.synchronize()
                    ctx.comm_stats(reset=True)
                if scheme == "ipcs":
                    ctx.set_bdf((1.0, -1.0, 0.0) if i == 0 else (1.5, -2.0, 0.5), args.dt)
                    info = ctx.step_ipcs(o)
                else:
                    ts.update_coefficients()
                    ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
                    info = ctx.step_imex(o)
                    ts.advance_time()
                ctx.advance(0)
                if i >= args.warmup:
                    its += (info.newton_iterations, info.krylov_iterations_momentum, info.krylov_iterations_poisson,
                            info.krylov_iterations_correction)
            st = ctx.comm_stats()
            res = {k: v / args.steps for k, v in st.items()}
            res.update(newton_its=its[0] / args.steps, momentum_its=its[1] / args.steps,
                       poisson_its=its[2] / args.steps, correction_its=its[3] / args.steps)
            if scheme == "imex":
                res["rhs_path"] = ctx.imex_info()["path"]
            out[r] = res
        except BaseException as exc:            # a dead rank would deadlock the others
            print("rank %d failed: %r" % (r, exc), flush=True)
            os._exit(17)

    threads = [threading.Thread(target=worker, args=(r,)) for r in range(size)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    for c in ctxs:
        c.close()
    nat.local_group_destroy(group)
    return out[0]


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cells", type=int, default=960)
    ap.add_argument("--ranks", type=int, nargs="+", default=[2, 4, 8])
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--dt", type=float, default=1.0e-3)
    ap.add_argument("--krylov-rtol", type=float, default=1.0e-8)
    ap.add_argument("--min-rows", type=int, default=16)
    ap.add_argument("--halo-mode", choices=("relaxed", "exact"), default="relaxed")
    ap.add_argument("--schemes", nargs="+", choices=("ipcs", "imex"), default=["ipcs", "imex"])
    ap.add_argument("--json", action="store_true", help="print every row as one JSON line as well")
    ap.add_argument("--out", default=None, help="write the rows as JSON to this file")
    args = ap.parse_args()
    rows = []
    for size in args.ranks:
        for scheme in args.schemes:
            res = run(scheme, args.cells, size, args)
            row = dict(scheme=scheme, cells=args.cells, ranks=size, halo_mode=args.halo_mode, steps=args.steps,
                       warmup=args.warmup, per_step_rank0=res)
            rows.append(row)
            print("%-4s n = %d, %d ranks: %.1f exchanges (%.3f MB), %.1f all-reduces (%.3f MB) per step; "
                  "its newton %.2f momentum %.2f poisson %.2f correction %.2f%s" % (
                      scheme, args.cells, size, res["exchanges"], res["exchange_bytes"] / 1e6, res["allreduce_calls"],
                      res["allreduce_bytes"] / 1e6, res["newton_its"], res["momentum_its"], res["poisson_its"],
                      res["correction_its"], " rhs " + res["rhs_path"] if "rhs_path" in res else ""), flush=True)
            if args.json:
                print(json.dumps(row), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(dict(note="per-step communicator counters of rank 0, thread ranks on one GPU; counts, not times",
                           rows=rows), f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
