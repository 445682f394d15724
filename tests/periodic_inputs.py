"""Inputs of the GPU cases on the periodic fixtures of tests/periodic_meshes.py that had to be chosen: the fields of the
law-8 kernel and step cases and the velocities of the Lagrangian advance cases.  Host only (no GPU, no test in here):
every condition an input has to meet is asserted here on the restatement alone, so tests/test_periodic_meshes_host.py
checks the same objects the GPU tests use.

Law 8.  The dynamic procedures give a negative constant for most smooth fields; fields, seeds and groupings were found
by a search over a few seeded superpositions on the CPU.  Asserted: the constant is positive and unclipped on at least
half the groups -- for the kernel cases on the field itself, for the step cases at every step of the restatement.
Lagrangian advance.  Directions and seeds searched on the CPU; asserted: every displaced vertex has exactly one cell
within the tie margin, at CFL 0.4 nothing is clamped where there is no wall, and the upstream cell lies across the
seam for at least a quarter of the displaced seam vertices."""
import numpy as np

import fem_oracle as fo
from dynamic_lagrangian_host import LagrangianDynamicRestatement
from dynamic_model_host import DynamicSmagorinskyRestatement
from imex_time_stepping import IMEXTimeStepping, IMEXType
from periodic_meshes import (far_images, lengths_of, periodic_axes, periodic_fields, periodic_fixture, seeded_modes,
                             wall_axes, wall_bc)
from test_variable_viscosity_host import IMEXViscRestatement, rule_space
from viscosity_models import DynamicSmagorinskyModel

NO_PBC = (np.zeros(0, np.int32), np.zeros(0))


def rel(a, b):
    return np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-300)


COEF = dict(convective_term=1.0, pressure_term=1.0, viscous_term=0.01, body_force_term=1.0)
_SPACES = {}


def spaces(kind):
    """(mesh, dm, oracle space, rule space) of a fixture, built once"""
    if kind not in _SPACES:
        mesh, dm, _ = periodic_fixture(kind)
        args = (mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
        _SPACES[kind] = (mesh, dm, fo.Space(*args), rule_space(*args))
    return _SPACES[kind]


def groups(dm, grouping):
    return DynamicSmagorinskyModel(grouping).vertex_groups(dm.p1_coords)


def half_unclipped(cs2, cs2_max):
    """the constant is positive and below the clip on at least half the groups"""
    return 2 * int(((cs2 > 0.0) & (cs2 < cs2_max)).sum()) >= cs2.size


# ---------------------------------------------------------------- law 8: the kernel cases
# fixture: (grouping, seed of periodic_meshes.seeded_modes or None for periodic_fields)
KERNEL_CASES = {"pchan2": (("planes", 1), 5), "psquare": (("planes", 0), 0), "pchan3": (("planes", 1), None),
                "pbox3": (("planes", 1), None), "pchan2_mapped": ("global", 5), "pchan3_mapped": ("global", None)}


def dynamic_kernel_case(kind, params=(2.0, 0.09)):
    """(grouping, u, restatement, its own constants) of the law-8 kernel case on ``kind``"""
    mesh, dm, s, rs = spaces(kind)
    grouping, seed = KERNEL_CASES[kind]
    L, axes = lengths_of(kind), periodic_axes(kind)
    u = periodic_fields(dm.p2_coords, L, axes)[0] if seed is None else seeded_modes(dm.p2_coords, L, axes, seed)
    orc = DynamicSmagorinskyRestatement(rs, params, groups(dm, grouping))
    own = orc.constant(u)
    assert own.max() > 1e-3 and half_unclipped(own, params[1]), (kind, own)
    return grouping, u, orc, own


# ---------------------------------------------------------------- law 8: the step cases
# name: (fixture, grouping, cs2_max, step size, seed of the start velocity -- a no-slip trace)
STEP_CASES = {"pchan2-planes": ("pchan2", ("planes", 1), 0.09, 0.002, 5),
              "pchan3-planes": ("pchan3", ("planes", 1), 0.05, 0.002, 7)}
_STEP_HOST = {}


def dynamic_step_setup(name):
    """(mesh, dm, s, rs, grouping, cs2_max, k, velocity Dirichlet data, body force, start velocity): no-slip on the
    walls, a periodic body force, a periodic velocity with a no-slip trace at both old levels"""
    kind, grouping, cs2_max, k, seed = STEP_CASES[name]
    mesh, dm, s, rs = spaces(kind)
    L, axes = lengths_of(kind), periodic_axes(kind)
    X = dm.p2_coords
    f = 0.6 * np.roll(periodic_fields(X, L, axes)[0].reshape(-1, dm.dim), 1, axis=1).ravel()
    return mesh, dm, s, rs, grouping, cs2_max, k, wall_bc(kind), f, seeded_modes(X, L, axes, seed)


def dynamic_host_steps(name, steps=4):
    """the restatement with its own constants and, beside it, the one without the term: per step the coefficients, the
    constants of level n, the effect of the term on u* and the states.  Asserted at every step: half the groups
    positive and unclipped.  Computed once"""
    if name not in _STEP_HOST:
        mesh, dm, s, rs, grouping, cs2_max, k, vbc, f, u0 = dynamic_step_setup(name)
        visc = DynamicSmagorinskyRestatement(rs, (2.0, cs2_max), groups(dm, grouping))
        runs = []
        for term in (visc, None):
            orc = IMEXViscRestatement(s, COEF, "standard", visc=term)
            orc.body_force = f
            orc.vel[1], orc.vel[2] = u0.copy(), u0.copy()
            runs.append(orc)
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=k)
        out = []
        for step in range(steps):
            ts.update_coefficients()
            cs2 = visc.constant(runs[0].vel[1])
            assert half_unclipped(cs2, cs2_max), (name, step, cs2)
            for orc in runs:
                orc.step(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size(), vbc, NO_PBC)
            out.append(dict(coef=(tuple(ts.alpha), tuple(ts.beta), tuple(ts.gamma), ts.get_next_step_size()), cs2=cs2,
                            effect=rel(runs[0].ustar, runs[1].ustar), ustar=runs[0].ustar.copy(),
                            u=runs[0].vel[0].copy(), p=runs[0].p.copy()))
            for orc in runs:
                orc.advance()
            ts.advance_time()
        _STEP_HOST[name] = out
    return _STEP_HOST[name]


# ---------------------------------------------------------------- the Lagrangian advance cases
DIRECTION = {"pchan2": (1.0, 0.37), "psquare": (1.0, 0.62), "pchan2_mapped": (1.0, 0.37),
             "pchan3": (1.0, -0.738, 0.401), "pbox3": (1.0, -0.738, -0.401), "pchan3_mapped": (-1.0, 0.596, 0.978)}
SEED = {"psquare": 2, "pchan2_mapped": 1, "pchan3_mapped": 2}            # default 0
_ADVANCE = {}


def lagrangian_velocity(kind, dm, rng):
    """a mean direction with a component along every periodic axis plus 10 % (2D) / 5 % (3D) noise at every node.
    pchan3: times a bubble that vanishes on the two walls, whose coplanar faces give the exact inflow ties of a Kuhn
    box; the other channels have inflow and outflow there"""
    u = np.array(DIRECTION[kind])[None, :] + (0.1 if dm.dim == 2 else 0.05) * rng.standard_normal((dm.n_p2, dm.dim))
    if kind == "pchan3":
        bubble = np.sin(np.pi * dm.p2_coords[:, 1] / lengths_of(kind)[1]) ** 0.5
        bubble[bubble < 1e-7] = 0.0
        u = u * bubble[:, None]
    return u.ravel()


def across_the_seam(kind, dm, cstar):
    """(seam [n_p1]: a cell of the dof's patch is a far image; across [n_p1]: the upstream cell is one)"""
    far = far_images(kind)
    p1 = dm.p1_dofmap.astype(np.int64)
    seam = np.zeros(dm.n_p1, dtype=bool)
    seam[p1[far]] = True
    across = np.array([far[cstar[v]][p1[cstar[v]] == v].any() for v in range(dm.n_p1)])
    return seam, across


def lagrangian_advance_case(kind, cfl):
    """(u, state, k, restatement, discrete choices) of one advance on ``kind``, with the assertions of the module
    docstring; built once"""
    if (kind, cfl) not in _ADVANCE:
        mesh, dm, s, rs = spaces(kind)
        orc = LagrangianDynamicRestatement(rs, (2.0, 0.09))
        rng = np.random.default_rng(SEED.get(kind, 0))
        u = lagrangian_velocity(kind, dm, rng)
        state = rng.uniform(1.0, 2.0, (dm.n_p1, 2)) * np.array([0.03, 1.0])
        height = 1.0 / np.sqrt((orc.grad ** 2).sum(axis=2)).max()
        k = cfl * height / np.abs(u).max()
        uv = orc.vertex_velocity(u)
        _, _, where = orc.locate(uv, k)
        moved = np.abs(uv).max(axis=1) > 0.0
        assert moved.all() or kind == "pchan3"
        assert not where["clamped"][~moved].any()
        assert np.all(where["tied"][moved] == 1), (kind, cfl, np.bincount(where["tied"][moved]))
        assert (where["best"] - where["second"])[moved].min() > 1e-9
        if cfl < 1.0 and not wall_axes(kind):
            assert not where["clamped"].any()
        seam, across = across_the_seam(kind, dm, where["cstar"])
        where = dict(where, seam=seam & moved, across=across & moved)
        assert where["seam"].sum() >= 4 and 4 * where["across"].sum() >= where["seam"].sum()
        _ADVANCE[kind, cfl] = (u, state, k, orc, where)
    return _ADVANCE[kind, cfl]
