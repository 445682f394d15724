"""Timing record of the device-side energy spectra (csrc/spectrum.hip).

For every case -- the triple-periodic cube at n^3 cubes (tgv3d, 2 n points per axis) and the doubly periodic square at
n x n cells (tg2d) -- a context with the nodal interpolant of the Taylor-Green vortex plus a small random field in U0,
then:

* wall clock of ``EnergySpectrum.compute()`` for the velocity (all components, result on the host; median and minimum
  of `reps` calls),
* the route it replaces on the same state: ``get_state(U0)``, ``numpy.fft.fftn`` of every component of the lattice
  array and the binning (``numpy.bincount``; a Python loop over the shells would be slower still),
* the largest difference of the two spectra relative to the total.

One JSON line per case on stdout.  Kernel times (pack, passes, binning): run this script under
``rocprofv3 --kernel-trace --stats`` in a run of its own and read the rows of k_spec_pack, k_fd_gemm*, k_spec_bin and
k_spec_bin_sum.

    python scripts/energy_spectrum_timing.py --case tgv3d --n 64
    python scripts/energy_spectrum_timing.py --case tg2d --n 512
"""
import argparse
import json
import os
import sys
import time
import types

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (os.path.join(ROOT, "navierstokes-with-fenics_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import numpy as np  # noqa: E402

import _native as nat  # noqa: E402
import dlfn_compat as dlfn  # noqa: E402
import energy_spectrum as es  # noqa: E402
import spectrum_host as sh  # noqa: E402
from fem_mesh import TaylorHoodDofMap, box_mesh, periodic_entity_map, preferred_p2_order, rectangle_mesh  # noqa: E402


class Periodic(dlfn.SubDomain):
    def __init__(self, dim):
        super().__init__()
        self.dim = dim

    def inside(self, x, on_boundary):
        return bool(on_boundary and any(dlfn.near(x[a], 0.0) for a in range(self.dim)))

    def map(self, x_slave, x_master):
        for a in range(self.dim):
            if dlfn.near(x_slave[a], 1.0):
                x_master[:] = x_slave
                x_master[a] -= 1.0
                return
        x_master[:] = -10.0


def run(args, case):
    dim = 3 if case == "tgv3d" else 2
    n = args.n
    t0 = time.perf_counter()
    mesh = box_mesh((0.0, ) * 3, (1.0, ) * 3, n, n, n) if dim == 3 else rectangle_mesh((0.0, 0.0), (1.0, 1.0), n, n)
    dm = TaylorHoodDofMap(mesh, reorder=preferred_p2_order(dim), periodic_map=periodic_entity_map(mesh, Periodic(dim)))
    ctx = nat.NsfemContext(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, dm.n_p2, dm.n_p1)
    g = 2.0 * np.pi
    X = dm.p2_coords
    U = 1e-3 * np.random.default_rng(0).standard_normal((dm.n_p2, dim))
    U[:, 0] += np.cos(g * X[:, 0]) * np.sin(g * X[:, 1])
    U[:, 1] -= np.sin(g * X[:, 0]) * np.cos(g * X[:, 1])
    ctx.set_state(nat.U0, U.ravel())
    spec = es.EnergySpectrum(types.SimpleNamespace(_ctx=ctx, _dofmap=dm), kind="shell")
    setup_s = time.perf_counter() - t0
    shape = spec.lattice.shape
    for _ in range(args.warmup):
        res = spec.compute()
    device_ms = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        res = spec.compute()
        device_ms.append(1e3 * (time.perf_counter() - t0))
    # the host route
    copy_ms, fft_ms, bin_ms, host = [], [], [], None
    spacing = [1.0 / s for s in shape]
    for _ in range(args.host_reps):
        t0 = time.perf_counter()
        u = ctx.get_state(nat.U0)
        t1 = time.perf_counter()
        arr = sh.lattice_array(u.reshape(-1, dim), X, spacing, shape)
        power = [np.abs(np.fft.fftn(arr[..., c])) ** 2 / arr[..., c].size for c in range(dim)]
        t2 = time.perf_counter()
        k2 = np.zeros(shape[::-1])
        for pos in range(dim):
            sh_ = [1] * dim
            sh_[pos] = shape[dim - 1 - pos]
            k2 = k2 + (np.fft.fftfreq(shape[dim - 1 - pos], d=1.0 / shape[dim - 1 - pos]) ** 2).reshape(sh_)
        shell = np.rint(np.sqrt(k2)).astype(np.int64).ravel()
        host = sum(np.bincount(shell, weights=p.ravel()) for p in power) * 0.5 / float(np.prod(shape))
        t3 = time.perf_counter()
        copy_ms.append(1e3 * (t1 - t0))
        fft_ms.append(1e3 * (t2 - t1))
        bin_ms.append(1e3 * (t3 - t2))
    info = spec.info()
    out = dict(case=case, n=n, lattice=list(shape), n_p2=dm.n_p2, n_bins=int(res["E"].size), setup_s=setup_s,
               plan_bytes=info["bytes"], launches_per_compute=dict(
                   transform=info["transform_launches"] // info["calls"], bin=info["bin_launches"] // info["calls"]),
               device_compute_ms=dict(median=float(np.median(device_ms)), min=min(device_ms)),
               total_energy=float(res["E"].sum()))
    if host is not None:      # (--host-reps 0: a profiler run of the device route alone)
        out.update(host_get_state_ms=min(copy_ms), host_gather_fftn_ms=min(fft_ms), host_binning_ms=min(bin_ms),
                   largest_difference_over_total=float(np.abs(res["E"] - host).max() / host.sum()))
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--case", action="append", choices=("tgv3d", "tg2d"))
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--host-reps", type=int, default=2)
    args = ap.parse_args()
    for case in args.case or ["tgv3d"]:
        print(json.dumps(run(args, case)), flush=True)


if __name__ == "__main__":
    main()
