"""Writes tests/golden/imex_cavity8_steps3.npz: the fields of the 8 x 8 lid-driven cavity after 3 steps of
IMEXIPCSSolver through InstationaryProblem.solve_problem (Re = 100, k = 1/16, default solver settings), as
tests/test_gpu_scalar_transport.py::test_problem_without_temperature_hooks_is_unchanged runs it.

The committed file was written on commit 905127d (the parent of the scalar transport), library built by
csrc/Makefile (hipcc -O3 --offload-arch=gfx950), on one MI355X.  The test compares bytes, so the file pins the
behaviour of a problem without temperature hooks; after a compiler or ROCm update that changes the last bits, check out
a commit known to be good, build, and run

    python tests/golden/gen_imex_cavity8_golden.py

from the repository root (needs the GPU)."""
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle"), os.path.join(ROOT, "navierstokes-with-fenics_amd")):
    sys.path.insert(0, p)

import numpy as np  # noqa: E402

import _native as nat  # noqa: E402
from ns_imex_solver import IMEXIPCSSolver  # noqa: E402
from problem_specs import build_problem  # noqa: E402


def main():
    os.environ["NSFEM_NO_OUTPUT"] = "1"
    spec = dict(name="Cavity", mesh=("cube", 2, 8), scheme="ipcs", numbers=dict(Re=100.0),
                clock=dict(dt=0.5 / 8, steps=3), start={"velocity": (0.0, 0.0), "pressure": 0.0},
                bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_slip", "bottom"), ("velocity", "top", (1.0, 0.0))])
    problem = build_problem(spec)
    problem.set_solver_class(IMEXIPCSSolver)
    problem.compute_cfl = False
    problem.solve_problem()
    ctx = problem._get_solver()._ctx
    np.savez(os.path.join(HERE, "imex_cavity8_steps3.npz"), u0=ctx.get_state(nat.U0), u1=ctx.get_state(nat.U1),
             ustar=ctx.get_state(nat.USTAR), p=ctx.get_state(nat.P), p_old=ctx.get_state(nat.P_OLD))


if __name__ == "__main__":
    main()
