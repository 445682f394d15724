"""Timing record of the device-side wall quantities (csrc/wall.hip).

On three facet sets -- the cylinder of the DFG channel, the four walls of the n x n cavity, the six walls of the
m x m x m box -- with a smooth state in U0 / P, alternating between the two routes `reps` times after `warmup` untimed
rounds:

* wall clock of one ``boundary_force`` call (nsfem_boundary_force: uploads both facet lists, allocates, copies
  n_facets * (dim + 2) doubles back, sums on the host),
* wall clock of one ``wall_compute`` call without facet rows on the resident set of the same facets (two launches,
  one copy of NW doubles).

Both end in a stream synchronise.  One JSON line per case on stdout (milliseconds: median and minimum).

    python scripts/wall_quantities_timing.py --n 512 --m 48
    python scripts/wall_quantities_timing.py --only cavity --n 64 --reps 3      # short run for a kernel trace
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "navierstokes-with-fenics_amd"), ):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

import _native as nat  # noqa: E402
import grid_generator as gg  # noqa: E402
from fem_mesh import TaylorHoodDofMap  # noqa: E402


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return 1e3 * (time.perf_counter() - t0)


def smooth_state(dm):
    X2, X1 = dm.p2_coords, dm.p1_coords
    u = np.stack([np.sin(1.3 * X2[:, 0] + 0.7) * np.cos(0.9 * X2[:, 1] + 0.2)] +
                 [np.cos(0.8 * X2[:, 0] - 0.4 + 0.3 * a) * (1.0 + X2[:, 1]) for a in range(1, dm.dim)], axis=1)
    return u, np.sin(0.6 * X1[:, 0] + 0.9) + X1[:, 1] * np.cos(1.5 * X1[:, 0])


def run_case(name, mesh, facets, warmup, reps):
    dm = TaylorHoodDofMap(mesh)
    cells, local = mesh.facet_cell_local(facets)
    ctx = nat.NsfemContext(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, dm.n_p2, dm.n_p1)
    u, p = smooth_state(dm)
    ctx.set_state(nat.U0, np.ascontiguousarray(u).ravel())
    ctx.set_state(nat.P, p)
    ctx.wall_set_facets(cells, local)
    ctx.synchronize()
    nu, sym = 0.01, 1.0
    routes = {"boundary_force_ms": lambda: ctx.boundary_force(cells, local, nu, sym),
              "wall_compute_ms": lambda: ctx.wall_compute(nu, sym)}
    times = {k: [] for k in routes}
    for rep in range(warmup + reps):
        for key, fn in routes.items():              # alternating: every round times every route once
            t = timed(fn)
            if rep >= warmup:
                times[key].append(t)
    force, flux, measure = ctx.boundary_force(cells, local, nu, sym)
    row = ctx.wall_compute(nu, sym)[0]
    dim = dm.dim
    out = dict(case=name, dim=dim, n_cells=int(mesh.cells.shape[0]), n_facets=int(cells.size), warmup=warmup, reps=reps,
               info=ctx.wall_info(),
               force_max_difference=float(np.abs(row[1:1 + dim] + row[1 + dim:1 + 2 * dim] - force).max()),
               measure=float(measure))
    for key, v in times.items():
        out[key] = dict(median=statistics.median(v), min=min(v))
    ctx.close()
    print(json.dumps(out), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--m", type=int, default=48)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--only", choices=("dfg", "cavity", "box"), default=None)
    args = ap.parse_args()
    if args.only in (None, "dfg"):
        mesh, marks = gg.dfg_channel(4, 2)
        run_case("dfg cylinder", mesh, marks.facets_with_id(gg.DFGBoundaryMarkers.cylinder.value), args.warmup, args.reps)
    if args.only in (None, "cavity"):
        mesh, _ = gg.hyper_cube(2, args.n)
        run_case("cavity walls n = %d" % args.n, mesh, np.flatnonzero(mesh.facet_on_boundary), args.warmup, args.reps)
    if args.only in (None, "box"):
        mesh, _ = gg.hyper_cube(3, args.m)
        run_case("box walls m = %d" % args.m, mesh, np.flatnonzero(mesh.facet_on_boundary), args.warmup, args.reps)


if __name__ == "__main__":
    main()
