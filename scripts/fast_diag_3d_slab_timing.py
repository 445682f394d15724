"""Message counts and times of the projection step on partitioned 3D slabs: fast diagonalisation (slab factors,
FastDiag3::apply_slab: one all-reduce per solve) against multigrid-CG, with thread ranks in ONE process on ONE GPU
(nat.local_group_create).  The ranks share the device, so the times are not a scaling curve; the counts are what a
multi-GPU run would send.

Cases: tgv3d (PeriodicSlabPartition, exact factors: one direct pass per step) and cavity (SlabPartition, inexact
factors: CG preconditioned by the slab T^+).  For every (case, n, ranks, solver), rank 0's JSON line on stdout:
per-step halo exchanges, all-reduce calls and bytes (comm_stats over the timed steps), ms per step, and the projection
solve alone where nsfem_solve can run it on a partition (the assembled Poisson system of the last step, start vector
p_old, every rank at once): multigrid-CG always, CG preconditioned by the slab T^+ for the cavity.  The direct slab
pass of tgv3d is timed as mg_apply(2) (host copies of the local vector included) -- an upper bound.

    python scripts/fast_diag_3d_slab_timing.py --case tgv3d --n 32 --ranks 2 --ranks 4
"""
import argparse
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "navierstokes-with-fenics_amd"), os.path.join(ROOT, "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

import _native as nat  # noqa: E402
from partition import PeriodicSlabPartition, SlabPartition  # noqa: E402

LO, HI = (0.0, 0.0, 0.0), (1.0, 1.0, 1.0)
G = 2.0 * np.pi


def setup(ctx, part, case):
    if case == "tgv3d":
        X, Y = part.dofmap.p2_coords, part.dofmap.p1_coords
        u0 = np.stack([np.cos(G * X[:, 0]) * np.sin(G * X[:, 1]), -np.sin(G * X[:, 0]) * np.cos(G * X[:, 1]),
                       np.zeros(X.shape[0])], axis=1).ravel()
        p0 = -0.25 * (np.cos(2 * G * Y[:, 0]) + np.cos(2 * G * Y[:, 1]))
        for slot in (nat.U0, nat.U1, nat.U2):
            ctx.set_state(slot, u0)
        for slot in (nat.P, nat.P_OLD):
            ctx.set_state(slot, p0)
        ctx.set_coeffs(1.0, 1.0, 0.01)
        ctx.set_dirichlet(nat.VELOCITY, np.zeros(0, np.int32), np.zeros(0))
    else:
        X = part.dofmap.p2_coords
        on = np.zeros(X.shape[0], dtype=bool)
        for a in range(3):
            on |= (np.abs(X[:, a]) < 1e-12) | (np.abs(X[:, a] - 1.0) < 1e-12)
        nodes = np.nonzero(on)[0]
        ux = np.where(np.abs(X[nodes, 2] - 1.0) < 1e-12, 1.0, 0.0)
        ctx.set_coeffs(1.0, 1.0, 0.01)
        ctx.set_dirichlet(nat.VELOCITY, np.concatenate([3 * nodes, 3 * nodes + 1, 3 * nodes + 2]).astype(np.int32),
                          np.concatenate([ux, np.zeros(2 * nodes.size)]))
    ctx.set_dirichlet(nat.PRESSURE, np.zeros(0, np.int32), np.zeros(0))


def partitions(case, n, size):
    cls = PeriodicSlabPartition if case == "tgv3d" else SlabPartition
    return [cls(LO, HI, n, n, n, r, size, coarsest=4, global_coarsest=2) for r in range(size)]


def run(args, case, n, size, solver, parts):
    group = nat.local_group_create(size)
    ctxs = []
    for r, part in enumerate(parts):
        d = part.dofmap
        c = nat.NsfemContext(part.mesh.coords, part.mesh.cells, d.p2_dofmap, d.p1_dofmap, d.n_p2, d.n_p1)
        c.attach_local_comm(group, r)
        ctxs.append(c)
    barrier = threading.Barrier(size)
    out, errors = {}, []
    dt = 0.25 / n

    def rank(r):
        ctx, part = ctxs[r], parts[r]
        part.attach(ctx)
        ctx.mg_set_halo_mode(True)                              # (bench.py's default on several GPUs)
        exact = part.attach_fast_diag(ctx) if solver == "fd" else None
        setup(ctx, part, case)
        o = ctx.default_step_opts()
        for k in (o.momentum, o.poisson, o.correction):
            k.rtol = args.rtol
        o.momentum.precond = 1
        o.poisson.precond = 3 if solver == "fd" else 1
        o.correction.precond = 2
        step = 0

        def advance():
            nonlocal step
            ctx.set_bdf((1.0, -1.0, 0.0) if step == 0 else (1.5, -2.0, 0.5), dt)
            info = ctx.step_ipcs(o)
            ctx.advance(0)
            step += 1
            return info

        for _ in range(args.warmup):
            advance()
        ctx.synchronize()
        ctx.comm_stats(reset=True)
        barrier.wait()
        t0 = time.perf_counter()
        its = [advance().krylov_iterations_poisson for _ in range(args.steps)]
        ctx.synchronize()
        barrier.wait()
        ms_step = 1e3 * (time.perf_counter() - t0) / args.steps
        st = ctx.comm_stats()
        # the projection solve alone
        times, solve_its, how = [], [], None
        for rep in range(args.solve_reps + 2):
            if solver == "fd" and exact:
                how = "mg_apply(2), host copies included"
                r_loc = np.ones(ctx.n_p1)
                barrier.wait()
                t1 = time.perf_counter()
                ctx.mg_apply(2, r_loc)
            else:
                how = "nsfem_solve, precond %d" % o.poisson.precond
                ctx.assemble(nat.SYS_POISSON)
                ctx.synchronize()
                barrier.wait()
                t1 = time.perf_counter()
                info = ctx.solve(nat.SYS_POISSON, rtol=args.rtol, precond=o.poisson.precond)
                solve_its.append(info.iterations)
            ctx.synchronize()
            barrier.wait()
            if rep >= 2:
                times.append(1e3 * (time.perf_counter() - t1))
        out[r] = dict(case=case, n=n, ranks=size, solver=solver, exact=exact, steps=args.steps, warmup=args.warmup,
                      krylov_rtol=args.rtol, ms_per_step=ms_step, poisson_iterations=its,
                      exchanges_per_step=st["exchanges"] / args.steps,
                      allreduce_calls_per_step=st["allreduce_calls"] / args.steps,
                      allreduce_bytes_per_step=st["allreduce_bytes"] / args.steps,
                      exchange_bytes_per_step=st["exchange_bytes"] / args.steps,
                      projection_solve_ms_median=float(np.median(times)), projection_solve_ms_min=float(np.min(times)),
                      projection_solve_how=how, projection_solve_iterations=solve_its[-args.solve_reps:],
                      fast_diag_3d=ctx.poisson_fast_diag_3d_info())

    def worker(r):
        try:
            rank(r)
        except BaseException as exc:                            # a dead rank would deadlock the others
            import traceback
            traceback.print_exc()
            errors.append((r, repr(exc)))
            sys.stderr.flush()
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
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", choices=("tgv3d", "cavity"), action="append")
    ap.add_argument("--n", type=int, action="append")
    ap.add_argument("--ranks", type=int, action="append")
    ap.add_argument("--solver", choices=("fd", "mg"), action="append")
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--solve-reps", type=int, default=10)
    ap.add_argument("--rtol", type=float, default=1e-12)
    args = ap.parse_args()
    for case in args.case or ["tgv3d", "cavity"]:
        for n in args.n or [32]:
            for size in args.ranks or [2, 4]:
                parts = partitions(case, n, size)
                for solver in args.solver or ["fd", "mg"]:
                    print(json.dumps(run(args, case, n, size, solver, parts)), flush=True)


if __name__ == "__main__":
    main()
