"""Same bytes before and after a change of the post-processing kernels: every device-side diagnostic
-- boundary force, volume functionals, body forces and heat, wall quantities, point location / evaluation / tracers,
flow statistics, derived fields -- is called through two builds of the library and every returned array and info
record is compared byte for byte.

    python scripts/postproc_front_identity.py compare --parent PATH/libnsfem_hip.so [--new PATH] [--out FILE]
    python scripts/postproc_front_identity.py child --lib PATH --out FILE.npz        (what ``compare`` starts)

``compare`` starts one fresh process per library (``_native.load_library(path)``), each of which runs the same calls
and stores its results; the parent's library is built from a clean export of the parent commit with the same flags.

Meshes: the box 4 x 4, a mapped (non-uniform) box 6 x 5, the 3 x 2 x 2 Kuhn box, a mapped 4^3 cube; and the smallest
shapes that take the reduction loops round a second time -- the box 72 x 64 (272 boundary facets in one group of
k_wall_reduce), 192 x 192 (73,728 cells: k_penal_forces / k_body_heat stride twice), 364 x 364 (264,992 cells:
k_vol_functionals strides twice); the statistics groups of the large boxes hold more than 256 nodes."""
import argparse
import json
import os
import subprocess
import sys
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, os.path.join(ROOT, "navierstokes-with-fenics_amd"))

LAWS = ((0, None), (1, (0.17, )), (2, (0.8, 1.3, 0.4)), (4, (0.5, )), (5, (0.07, )), (8, (2.0, 0.1)))


def meshes():
    """name -> (mesh, what runs on it): 'all' every call, 'wall' / 'bodies' / 'functionals' the one that needs the size"""
    from fem_mesh import box_mesh, rectangle_mesh

    def mapped(mesh):
        x = mesh.coords
        s = np.sin(np.pi * x)
        if x.shape[1] == 2:
            x[:, 0] += 0.06 * s[:, 0] * s[:, 1]
            x[:, 1] += 0.04 * s[:, 0] * s[:, 1] + 0.1 * x[:, 1] * (1.0 - x[:, 1])
        else:
            w = 0.05 * s[:, 0] * s[:, 1] * s[:, 2]
            x[:, 0] += w
            x[:, 1] -= 0.8 * w
            x[:, 2] += 0.1 * x[:, 2] * (1.0 - x[:, 2])
        return mesh

    return {
        "box 4x4": (rectangle_mesh((0.0, 0.0), (1.0, 1.0), 4, 4), "all"),
        "mapped 6x5": (mapped(rectangle_mesh((0.0, 0.0), (1.0, 1.0), 6, 5)), "all"),
        "kuhn 3x2x2": (box_mesh((0.0, 0.0, 0.0), (1.0, 0.8, 0.6), 3, 2, 2), "all"),
        "mapped 4x4x4": (mapped(box_mesh((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 4, 4, 4)), "all"),
        "box 72x64": (rectangle_mesh((0.0, 0.0), (1.0, 1.0), 72, 64), "wall"),
        "box 192x192": (rectangle_mesh((0.0, 0.0), (1.0, 1.0), 192, 192), "bodies"),
        "box 364x364": (rectangle_mesh((0.0, 0.0), (1.0, 1.0), 364, 364), "functionals"),
    }


def fields(X2, X1, k=0):
    """smooth non-polynomial u [n_p2, dim], p [n_p1], T [n_p2]; k shifts the phases (another sample)"""
    dim = X2.shape[1]
    a = 0.3 * k
    u = np.stack([np.sin((1.3 + d) * X2[:, 0] + 0.7 * X2[:, (d + 1) % dim] + a) * np.cos(0.9 * X2[:, -1] - d + a)
                  for d in range(dim)], axis=1)
    p = np.cos(1.1 * X1[:, 0] + a) * np.sin(0.8 * X1[:, -1] + 0.3) + 0.5 * X1[:, 0]
    T = np.sin(1.7 * X2[:, 0] - 0.4 * X2[:, -1] + a) + 0.25 * X2[:, -1] ** 2
    return np.ascontiguousarray(u), p, T


class Record:
    def __init__(self):
        self.arrays, self.infos = {}, {}

    def arr(self, mesh, call, *values):
        for i, v in enumerate(values):
            self.arrays["%s | %s | %d" % (mesh, call, i)] = np.ascontiguousarray(v)

    def info(self, mesh, call, d):
        self.infos["%s | %s" % (mesh, call)] = {k: (v if not isinstance(v, np.ndarray) else v.tolist()) for k, v in d.items()}


def bodies_of(dim, heated):
    from immersed_bodies import Ball, Box
    if dim == 2:
        bs = [Ball((0.37, 0.52), 0.21, velocity=(0.3, -0.2), angular=0.7, temperature=1.5 if heated else None),
              Box((0.71, 0.33), (0.17, 0.12), velocity=(-0.1, 0.25), angular=-0.4)]
    else:
        bs = [Ball((0.41, 0.47, 0.36), 0.27, velocity=(0.3, -0.2, 0.1), angular=(0.2, -0.5, 0.7),
                   temperature=1.5 if heated else None),
              Box((0.74, 0.3, 0.3), (0.15, 0.2, 0.2), velocity=(-0.1, 0.25, 0.0), angular=(0.0, 0.3, -0.4))]
    return bs


def run_functionals(rec, name, ctx, nat, u, p, n_cells):
    rng = np.random.default_rng(11)
    rec.arr(name, "volume_functionals", ctx.volume_functionals(nat.U0, nat.P)["values"])
    v = u.ravel() + 1e-3 * rng.standard_normal(u.size)
    q = p + 1e-3 * rng.standard_normal(p.size)
    rec.arr(name, "volume_functionals ref u p", ctx.volume_functionals(nat.U0, nat.P, v, q)["values"])
    rec.arr(name, "volume_functionals ref u", ctx.volume_functionals(nat.U0, nat.P, ref_velocity=v)["values"])
    flags = rng.integers(0, 2, n_cells)
    rec.arr(name, "volume_functionals flags", ctx.volume_functionals(nat.U0, nat.P, cell_flags=flags)["values"])
    rec.arr(name, "volume_functionals flags ref", ctx.volume_functionals(nat.U0, nat.P, v, q, flags)["values"])


def run_bodies(rec, name, ctx, nat, dim):
    from immersed_bodies import ImmersedBodies
    for eps in (0.0, 0.07):
        tag = "sharp" if eps == 0.0 else "smoothed"
        b = ImmersedBodies(bodies_of(dim, True), 0.037, eps)
        ctx.set_bodies(b.rows(), 0.037, eps)
        rec.arr(name, "body_forces " + tag, ctx.body_forces(nat.U0))
        rec.arr(name, "body_forces U1 " + tag, ctx.body_forces(nat.U1))
        flags, values = b.temperatures()
        ctx.set_body_temperatures(flags, values, 0.05)
        rec.arr(name, "body_heat " + tag, ctx.body_heat(nat.T0))
        rec.info(name, "body_info " + tag, ctx.body_info())
        rec.info(name, "body_heat_info " + tag, ctx.body_heat_info())
    ctx.set_body_temperatures([], [])
    ctx.set_bodies([])


def run_wall(rec, name, ctx, nat, mesh, dim, laws, one_group):
    ids = np.flatnonzero(mesh.facet_on_boundary)
    cells, local = mesh.facet_cell_local(ids)
    rec.arr(name, "boundary_force", *[np.atleast_1d(v) for v in ctx.boundary_force(cells, local, 0.013, 1.0)])
    rec.arr(name, "boundary_force sym 0", *[np.atleast_1d(v) for v in ctx.boundary_force(cells[::2], local[::2], 0.02, 0.0)])
    if one_group:
        ctx.wall_set_facets(cells, local)
    else:
        ctx.wall_set_facets(cells, local, np.arange(ids.size, dtype=np.int32) % 3, 4)
    origin = (0.3, -0.2, 0.1)[:dim]
    for law, params in laws:
        ctx.set_viscosity_law(law, params)
        for use_law in ((False, ) if law == 0 else (False, True)):
            for scalar in (-1, nat.T0):
                groups, rows = ctx.wall_compute(0.013, 1.0, 0.021, origin, use_law=use_law, scalar_slot=scalar, facets=True)
                rec.arr(name, "wall_compute law%d use_law%d scalar%d" % (law, use_law, scalar), groups, rows)
        if law in (1, 4, 5):
            ctx.set_scalar_sgs(0.85)
            rec.arr(name, "wall_compute law%d Pr_t" % law,
                    *ctx.wall_compute(0.013, 0.0, 0.021, origin, use_law=True, scalar_slot=nat.T0, facets=True))
            ctx.set_scalar_sgs(0.0)
        if law == 8:
            ctx.set_scalar_sgs_dynamic(True, 0.2)
            rec.arr(name, "wall_compute law8 dynamic flux",
                    *ctx.wall_compute(0.013, 1.0, 0.021, origin, use_law=True, scalar_slot=nat.T0, facets=True))
            ctx.set_scalar_sgs_dynamic(False)
        rec.info(name, "wall_info law%d" % law, ctx.wall_info())
    ctx.set_viscosity_law(0)


def run_points(rec, name, ctx, nat, mesh, dim):
    from point_locator import build_bins
    ctx.set_point_locator(**build_bins(mesh.coords, mesh.cells))
    rng = np.random.default_rng(5)
    lo, hi = mesh.coords.min(axis=0), mesh.coords.max(axis=0)
    X = lo + (hi - lo) * rng.uniform(-0.05, 1.05, (700, dim))
    cells = ctx.locate_points(X)
    rec.arr(name, "locate_points", cells)
    for slot, tag in ((nat.U0, "velocity"), (nat.P, "pressure"), (nat.T0, "scalar")):
        rec.arr(name, "eval_points " + tag, ctx.eval_points(slot, X))
        rec.arr(name, "eval_points cells given " + tag, ctx.eval_points(slot, X, cells))
    ctx.tracers_set(X)
    rec.info(name, "tracers_info set", ctx.tracers_info())
    ctx.tracers_advect(nat.U0, nat.U0, 0.05, 1)
    rec.arr(name, "tracers_advect frozen", *ctx.tracers_get())
    rec.info(name, "tracers_info frozen", ctx.tracers_info())
    ctx.tracers_advect(nat.U1, nat.U0, 0.11, 3)
    rec.arr(name, "tracers_advect blended", *ctx.tracers_get())
    rec.info(name, "tracers_info blended", ctx.tracers_info())


def run_stats(rec, name, ctx, nat, dm, dim, samples):
    from flow_statistics import groups_along_axis
    for scalar in (False, True):
        tag = "scalar" if scalar else "plain"
        ctx.stats_enable(nat.STATS_VELOCITY | nat.STATS_PRESSURE | (nat.STATS_SCALAR if scalar else 0))
        for k, (u, p, T) in enumerate(samples):
            ctx.set_state(nat.U2, u.ravel())
            ctx.set_state(nat.P_OLD, p)
            ctx.set_state(nat.T2, T)
            ctx.stats_sample(nat.U2, nat.P_OLD, nat.T2 if scalar else -1, 0.5 + 0.75 * k)
        qs = [nat.STATS_MEAN_U, nat.STATS_COV_U, nat.STATS_TKE, nat.STATS_MEAN_P, nat.STATS_VAR_P]
        if scalar:
            qs += [nat.STATS_MEAN_T, nat.STATS_VAR_T, nat.STATS_FLUX_UT]
        for q in qs:
            rec.arr(name, "stats_get %d %s" % (q, tag), ctx.stats_get(q))
        rng = np.random.default_rng(7)
        for axis in range(dim):
            for field, X in ((0, dm.p2_coords), (1, dm.p1_coords)):
                _, ptr, nodes = groups_along_axis(X, axis)
                ctx.stats_set_groups(field, ptr, nodes, rng.uniform(0.25, 4.0, nodes.size))
                rec.arr(name, "stats_profiles axis%d field%d %s" % (axis, field, tag), ctx.stats_profiles(field))
        for field, n in ((0, dm.n_p2), (1, dm.n_p1)):      # every node in one group
            ctx.stats_set_groups(field, np.array([0, n], np.int32), np.arange(n, dtype=np.int32))
            rec.arr(name, "stats_profiles one group field%d %s" % (field, tag), ctx.stats_profiles(field))
        rec.info(name, "stats_info " + tag, ctx.stats_info())
        rec.arr(name, "stats_weight " + tag, np.array([ctx.stats_weight()]))
    ctx.stats_enable(0)


def run_derived(rec, name, ctx, nat):
    every = list(range(nat.N_DERIVED))
    for center, tag in ((nat.DERIVED_CELL, "cell"), (nat.DERIVED_VERTEX, "vertex"), (nat.DERIVED_NODE, "node")):
        res = ctx.derived_fields(every, center, nat.U0, nat.P, nat.T0)
        rec.arr(name, "derived_fields all " + tag, *[res[q] for q in every])
        res = ctx.derived_fields([nat.DERIVED_VORTICITY, nat.DERIVED_Q_CRITERION], center, nat.U1, -1, -1)
        rec.arr(name, "derived_fields two " + tag, *[res[q] for q in sorted(res)])
        rec.info(name, "derived_info " + tag, ctx.derived_info())


def child(lib, out):
    import _native as nat
    from fem_mesh import TaylorHoodDofMap
    nat._lib = nat.load_library(lib)              # every context of this process goes through this build
    with open("/proc/self/maps") as f:
        mapped = {line.split()[-1] for line in f if "libnsfem_hip" in line}
    assert mapped == {os.path.realpath(lib)}, mapped
    rec = Record()
    for name, (mesh, what) in meshes().items():
        dm = TaylorHoodDofMap(mesh)
        dim = dm.dim
        ctx = nat.NsfemContext(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, dm.n_p2, dm.n_p1)
        samples = [fields(dm.p2_coords, dm.p1_coords, k) for k in range(3)]
        u, p, T = samples[0]
        ctx.set_scalar(0.021)
        ctx.set_state(nat.U0, u.ravel())
        ctx.set_state(nat.U1, 0.5 * samples[1][0].ravel())
        ctx.set_state(nat.P, p)
        ctx.set_state(nat.T0, T)
        if what in ("all", "functionals"):
            run_functionals(rec, name, ctx, nat, u, p, mesh.num_cells())
        if what in ("all", "bodies"):
            run_bodies(rec, name, ctx, nat, dim)
        if what in ("all", "wall"):
            run_wall(rec, name, ctx, nat, mesh, dim, LAWS if what == "all" else LAWS[:2], what == "wall")
        if what == "all":
            run_points(rec, name, ctx, nat, mesh, dim)
            run_derived(rec, name, ctx, nat)
        if what in ("all", "wall", "bodies"):
            run_stats(rec, name, ctx, nat, dm, dim, samples if what == "all" else samples[:2])
        ctx.close()
        print("child %s: %s done, %d arrays so far" % (os.path.basename(os.path.dirname(lib)) or lib, name, len(rec.arrays)),
              flush=True)
    np.savez(out, __infos__=np.array(json.dumps(rec.infos, sort_keys=True)), **rec.arrays)


def run_child(lib, path):
    """the calls through the build ``lib`` in a fresh process -> {name: array}, the info records under __infos__"""
    subprocess.run([sys.executable, os.path.abspath(__file__), "child", "--lib", os.path.abspath(lib), "--out", path],
                   check=True)
    with np.load(path) as z:
        return {k: z[k] for k in z.files}


def compare(parent, new, out):
    with tempfile.TemporaryDirectory() as tmp:
        results = {tag: run_child(lib, os.path.join(tmp, tag + ".npz")) for tag, lib in (("parent", parent), ("new", new))}
    return report(results["parent"], results["new"], parent, new, out)


def report(a, b, parent, new, out):
    a, b = dict(a), dict(b)
    ia, ib = json.loads(str(a.pop("__infos__"))), json.loads(str(b.pop("__infos__")))
    assert sorted(a) == sorted(b) and sorted(ia) == sorted(ib), "the two runs made different calls"
    table = {}
    n_bytes = n_diff_arrays = 0
    for key in sorted(a):
        _, call, _ = key.split(" | ")
        x, y = a[key], b[key]
        same_shape = x.shape == y.shape and x.dtype == y.dtype
        diff = int((np.frombuffer(x.tobytes(), np.uint8) != np.frombuffer(y.tobytes(), np.uint8)).sum()) if same_shape \
            else max(x.nbytes, y.nbytes)
        row = table.setdefault(call, [0, 0, 0, 0.0])
        row[0] += 1
        row[1] += x.nbytes
        row[2] += diff
        finite = x[np.isfinite(x)] if x.dtype.kind == "f" else x
        row[3] = max(row[3], float(np.abs(finite).max()) if finite.size else 0.0)
        n_bytes += x.nbytes
        n_diff_arrays += diff != 0
    detail = []
    for key in sorted(a):
        x, y = a[key], b[key]
        if x.shape == y.shape and x.tobytes() != y.tobytes():
            where = np.flatnonzero((x != y).ravel() & ~(np.isnan(x) & np.isnan(y)).ravel()) if x.dtype.kind == "f" \
                else np.flatnonzero((x != y).ravel())
            ulps = np.abs(x.ravel().view(np.int64)[where] - y.ravel().view(np.int64)[where]) if x.dtype == np.float64 else where
            detail.append("  %s: %d of %d entries differ (first at flat index %s of shape %s), largest distance %d ulp" %
                          (key, where.size, x.size, where[:6].tolist(), x.shape, int(ulps.max()) if where.size else 0))
    info_diff = [k for k in sorted(ia) if ia[k] != ib[k]]
    total_diff = sum(r[2] for r in table.values())
    import hashlib
    sha = {tag: hashlib.sha256(open(lib, "rb").read()).hexdigest()[:16] for tag, lib in (("parent", parent), ("new", new))}
    lines = ["libraries: parent sha256 %s, new sha256 %s" % (sha["parent"], sha["new"]), "",
             "%d arrays, %d bytes compared; %d info records compared; %d differing bytes in %d arrays, %d differing info "
             "records" % (len(a), n_bytes, len(ia), total_diff, n_diff_arrays, len(info_diff)), "",
             "%-58s %8s %10s %10s  %s" % ("compared array", "arrays", "bytes", "differing", "largest |entry|")]
    for call in sorted(table):
        r = table[call]
        lines.append("%-58s %8d %10d %10d  %.3e" % (call, r[0], r[1], r[2], r[3]))
    lines += ["", "differing arrays (mesh | call | index of the returned array):"] + (detail if detail else ["  none"])
    lines += ["", "differing info records: %s" % (info_diff if info_diff else "none")]
    text = "\n".join(lines) + "\n"
    print(text)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "w") as f:
            f.write(text)
    return 0 if total_diff == 0 and not info_diff else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    sub = ap.add_subparsers(dest="mode", required=True)
    c = sub.add_parser("child")
    c.add_argument("--lib", required=True)
    c.add_argument("--out", required=True)
    m = sub.add_parser("compare")
    m.add_argument("--parent", required=True)
    m.add_argument("--new", default=os.path.join(ROOT, "navierstokes-with-fenics_amd", "libnsfem_hip.so"))
    m.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.mode == "child":
        child(args.lib, args.out)
        return 0
    return compare(args.parent, args.new, args.out)


if __name__ == "__main__":
    sys.exit(main())
