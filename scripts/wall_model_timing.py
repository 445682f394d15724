"""Timing record of the wall-stress models (nsfem_set_wall_model); the output goes to
profiles/wall_model_timing.txt.

    rocprofv3 --kernel-trace --output-format csv -d DIR -- python scripts/wall_model_timing.py kernels
        ``--reps`` evaluations of weight * W(u) (k_wm_facets, k_wm_gather, through nsfem_wall_model_residual) per law on
        the four walls of the n x n cavity mesh (n = 512) and on the six walls of an n3^3 box (n3 = 48), in-cell matching
        with theta = 1, the smooth field of the tests, nu = 1e-4, in ONE run with no counters.
        ``python scripts/scalar_sgs_timing.py summary DIR --match k_wm_`` prints median, minimum and maximum per kernel
        name and grid size.

No threshold is set: nobody has measured these launches before.
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, d) for d in ("navierstokes-with-fenics_amd", "tests", "oracle")):
    if _p not in sys.path:
        sys.path.insert(0, _p)


def run_kernels(args):
    import _native as nat
    from gpu_common import box, context
    from test_gpu_3d import box3, context3
    from test_scalar_transport_host import smooth_fields
    from wall_models import ReichardtModel, WallModel, WernerWengleModel
    cases = [("2d", lambda: box(args.n, args.n), context, (1, 2, 3, 4)),
             ("3d", lambda: box3((args.n3, ) * 3), context3, (1, 2, 3, 4, 5, 6))]
    for tag, make_mesh, make_ctx, ids in cases:
        mesh, dm, marks = make_mesh()
        u, _ = smooth_fields(dm.p2_coords)
        ctx = make_ctx(mesh, dm)
        try:
            ctx.set_coeffs(1.0, 1.0, args.nu, 1.0)
            ctx.set_state(nat.U1, u)
            for law in (WernerWengleModel(), ReichardtModel()):
                a = WallModel(law, ids, ("cell", 1.0)).build(mesh, marks, dm)
                ctx.set_wall_model(law.law_id, law.params(), a.facet_cell, a.facet_local, a.sample_cell,
                                   a.sample_lambda, a.sample_y, a.wall_velocity)
                for _ in range(args.reps):
                    ctx.wall_model_residual(nat.U1, 1.0)
                rows = ctx.wall_model_facets(nat.U1)
                print(json.dumps(dict(case=tag, law=law.law_id, cells=int(mesh.cells.shape[0]),
                                      facets=int(a.facet_cell.size), nodes=int(a.nodes.size),
                                      max_y_plus=float(rows[:, -1].max()), reps=args.reps)))
        finally:
            ctx.close()


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("mode", choices=("kernels", ))
    ap.add_argument("--n", type=int, default=512)
    ap.add_argument("--n3", type=int, default=48)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--nu", type=float, default=1.0e-4)
    args = ap.parse_args()
    run_kernels(args)


if __name__ == "__main__":
    main()
