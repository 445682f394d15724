"""Wall quantities on the device (csrc/wall.hip: k_wall_facets<2|3, 0|1|2>, k_wall_reduce<9|13>; nsfem_wall_set_facets /
_compute / _components / _info) against the numpy restatement pinned in tests/test_wall_quantities_host.py, and the
callers: ``wall_quantities.WallQuantities``, ``ProblemBase._add_wall_quantities`` / ``_compute_wall_quantities``.

Tolerance (derived, not measured; the derivation with every count is in the docstring of
tests/test_wall_quantities_host.py): per entry ``2 n_terms 2^-53 A`` -- A the sum of the absolute contributions of the
entry (``wall_reference(..., absolute=True)``), n_terms = 66 (2D) / 96 (3D) rounded operations along the longest chain
of k_wall_facets that ends in an entry of a facet row (geometry 6 / 12, grad lambda_0 dim, the normal dim + 2, the
weight 3, the point 2, d phi 3, the N2 fused terms of G and 1, the traction 4 + n_nrm + dim + 1, the weight and the
rule's NQ terms, the arm NV + 3 and the cross product 3); a group row of L facets adds the reduction: ceil(L / 256)
strided terms, 6 shuffle levels, 3 wave sums.  With a viscosity law 2 n_G + n_geo + n_nrm + dim^2 + dim + 16 more and
the absolute version of nu_x; Carreau adds 16 ulp (the bound of the OpenCL C specification for double precision pow,
to which the device math library is built) times |a| P times the rest of its term.

Meshes: the smallest that take each path -- 20 facets (under one wave), 272 (two workgroups of k_wall_facets, a
ragged last one), 64 faces (under one workgroup), 528 faces (three strided passes of k_wall_reduce when in one group),
the unstructured fixture, the periodic square (identified nodes).  The general tetrahedra of tests/general_tet_mesh.py:
72 cells (64 faces) and 900 cells (340 faces: a second, ragged workgroup of k_wall_facets<3, ...>) -- cells of both
orientations and of different sizes, no zero in any J^-1, boundary faces that are planar but not axis-aligned (every
component of almost every normal is non-zero), so that the analytic integrals of the polynomial fields are the sums over
the planar faces and the facet rules stay exact."""
import math
import os

import numpy as np
import pytest

import _native as nat
import wall_quantities as wq
from fem_mesh import TaylorHoodDofMap, box_mesh, rectangle_mesh
from general_tet_mesh import LARGE, SMALL, general_tets
from gpu_common import context
from periodic_meshes import periodic_fixture
from test_derived_fields_host import polynomial_fields, polynomial_nodal, smooth_fields
from test_flow_statistics_host import periodic_square
from test_wall_quantities_host import (CARREAU, EPS, OPTS, SMAGORINSKY, analytic_rows, boundary_facets, group_sums,
                                       n_terms, wall_bounds, wall_reference)

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MESHES = ("rect6x4", "rect96x40", "box3x2x2", "box8x6x6", "fixture", "periodic", "general72", "general900", "pchan3")
# (pchan3: the 2 x 18 wall faces and the 4 x 12 faces of the periodic sides, which are boundary faces of the mesh)
EXPECTED_FACETS = dict(pchan3=84, rect6x4=20, rect96x40=272, box3x2x2=64, box8x6x6=528, general72=64, general900=340)
N_GROUPS = 4                                           # interleaved ids 0, 1, 3; group 2 stays empty
LAWS = {"smagorinsky": (SMAGORINSKY, (0.17, )), "carreau": (CARREAU, (0.8, 1.3, 0.4))}
_CACHE = {}


def _mesh(name):
    from mesh_io import read_msh
    if name == "rect6x4":
        mesh = rectangle_mesh((0.0, 0.0), (1.5, 1.0), 6, 4)
    elif name == "rect96x40":
        mesh = rectangle_mesh((0.0, 0.0), (2.4, 1.0), 96, 40)
    elif name == "box3x2x2":
        mesh = box_mesh((0.0, 0.0, 0.0), (1.5, 1.0, 1.0), 3, 2, 2)
    elif name == "box8x6x6":
        mesh = box_mesh((0.0, 0.0, 0.0), (1.0, 0.75, 0.75), 8, 6, 6)
    elif name == "fixture":
        mesh = read_msh(os.path.join(HERE, "golden", "square_v41.msh"))[0]
    elif name == "periodic":
        return periodic_square(8)
    elif name == "pchan3":
        return periodic_fixture(name)[:2]
    elif name in ("general72", "general900"):
        return general_tets(*(SMALL if name == "general72" else LARGE))[:2]
    else:
        raise ValueError(name)
    return mesh, TaylorHoodDofMap(mesh)


def interleaved_groups(n):
    g = np.arange(n, dtype=np.int32) % 3
    g[g == 2] = 3
    return g


def reference(name):
    """mesh, dof map, the boundary facets, the smooth fields, the restatement's rows and the bounds -- computed once
    per mesh and left unchanged"""
    if name not in _CACHE:
        mesh, dm = _mesh(name)
        ids, cells, local = boundary_facets(mesh)
        if name in EXPECTED_FACETS:
            assert ids.size == EXPECTED_FACETS[name]
        u, p, T = smooth_fields(dm.p2_coords, dm.p1_coords)
        group = interleaved_groups(ids.size)
        rows = wall_reference(mesh, dm, (cells, local), u, p, T, OPTS)
        bf, bg = wall_bounds(mesh, dm, (cells, local), u, p, T, OPTS, groups=(group, N_GROUPS))
        _CACHE[name] = dict(mesh=mesh, dm=dm, cells=cells, local=local, group=group, u=u, p=p, T=T, rows=rows,
                            sums=group_sums(rows, group, N_GROUPS), bound_rows=bf, bound_sums=bg)
    return _CACHE[name]


def loaded_context(ref, scalar=True, fields=None):
    u, p, T = fields if fields is not None else (ref["u"], ref["p"], ref["T"])
    ctx = context(ref["mesh"], ref["dm"])
    if scalar:
        ctx.set_scalar(OPTS["kappa"])
        ctx.set_state(nat.T0, T)
    ctx.set_state(nat.U0, np.ascontiguousarray(u).ravel())
    ctx.set_state(nat.P, p)
    return ctx


def compute(ctx, scalar=True, use_law=False, opts=OPTS):
    return ctx.wall_compute(opts["nu"], opts["sym"], opts["kappa"], opts["origin"], use_law=use_law,
                            scalar_slot=nat.T0 if scalar else -1, facets=True)


def check(label, got, want, bound, failures):
    err = np.abs(got - want)
    ratio = float((err / np.maximum(bound, 1e-300)).max()) if err.size else 0.0
    print("%s: max error %.3e, max error / bound %.3f (max |value| %.3e)"
          % (label, err.max() if err.size else 0.0, ratio, np.abs(want).max() if want.size else 0.0))
    if not (err <= bound).all():
        failures.append((label, ratio))


# ---------------------------------------------------------------- agreement with the restatement
@pytest.mark.parametrize("name", MESHES)
def test_every_entry_equals_the_restatement(name):
    ref = reference(name)
    ctx = loaded_context(ref)
    dim = ref["dm"].dim
    assert ctx.wall_components() == wq.row_width(dim) == ref["rows"].shape[1]
    ctx.wall_set_facets(ref["cells"], ref["local"], ref["group"], N_GROUPS)
    sums, rows = compute(ctx)
    ctx.close()
    assert rows.shape == ref["rows"].shape and sums.shape == (N_GROUPS, rows.shape[1])
    assert np.abs(ref["rows"]).max(axis=0).min() > 1e-4                 # the fields exercise every component
    failures = []
    check(name + " facet rows", rows, ref["rows"], ref["bound_rows"], failures)
    check(name + " group rows", sums, ref["sums"], ref["bound_sums"], failures)
    assert np.array_equal(sums[2], np.zeros(rows.shape[1])) and not np.signbit(sums[2]).any()     # the empty group
    assert not failures, failures


@pytest.mark.parametrize("name", ["rect6x4", "box3x2x2", "fixture", "general72", "general900"])
def test_polynomial_fields_return_the_analytic_integrals(name):
    """quadratic u, linear p, quadratic T: the facet rules are exact, every entry equals the integral of the exact
    fields written out from their coefficients"""
    ref = reference(name)
    mesh, dm = ref["mesh"], ref["dm"]
    poly = polynomial_fields(dm.dim)
    u, p, T = polynomial_nodal(dm, poly)
    facets = (ref["cells"], ref["local"])
    want = analytic_rows(mesh, dm, ref["cells"], ref["local"], poly, OPTS)
    bf, bg = wall_bounds(mesh, dm, facets, u, p, T, OPTS, groups=(ref["group"], N_GROUPS))
    ctx = loaded_context(ref, fields=(u, p, T))
    ctx.wall_set_facets(ref["cells"], ref["local"], ref["group"], N_GROUPS)
    sums, rows = compute(ctx)
    ctx.close()
    failures = []
    check(name + " polynomial facet rows", rows, want, bf, failures)
    check(name + " polynomial group rows", sums, group_sums(want, ref["group"], N_GROUPS), bg, failures)
    assert not failures, failures


@pytest.mark.parametrize("name", ["rect96x40", "box8x6x6", "fixture"])
def test_sums_equal_the_old_call(name):
    """force, flux and measure of one group of all facets against nsfem_boundary_force with the same nu and sym.
    Bound: both calls carry the facet chain (n_terms; the old kernel's is shorter), the new one its reduction
    (ceil(L / 256) + 9 <= L), the old one its host sum of L terms: 2 (n_terms + L) 2^-53 A"""
    ref = reference(name)
    dim = ref["dm"].dim
    facets = (ref["cells"], ref["local"])
    L = ref["cells"].size
    A = wall_reference(ref["mesh"], ref["dm"], facets, ref["u"], ref["p"], ref["T"], OPTS, absolute=True).sum(axis=0)
    bound = 2.0 * (n_terms(dim) + L) * EPS * A
    ctx = loaded_context(ref)
    ctx.wall_set_facets(*facets)
    cols = wq.split_rows(compute(ctx)[0][0], dim)
    force, flux, measure = ctx.boundary_force(ref["cells"], ref["local"], OPTS["nu"], OPTS["sym"])
    ctx.close()
    failures = []
    check(name + " force", cols["pressure_force"] + cols["viscous_force"], force,
          bound[1:1 + dim] + bound[1 + dim:1 + 2 * dim], failures)
    check(name + " flux", np.array([cols["mass_flux"]]), np.array([flux]), bound[1 + 2 * dim:2 + 2 * dim], failures)
    check(name + " measure", np.array([cols["area"]]), np.array([measure]), bound[0:1], failures)
    assert not failures, failures


# ---------------------------------------------------------------- groups
def _exact_sums(rows, group, n_groups):
    out = np.zeros((n_groups, rows.shape[1]))
    for g in range(n_groups):
        sel = rows[group == g]
        for k in range(rows.shape[1]):
            out[g, k] = math.fsum(sel[:, k])
    return out


def test_groups_sum_their_own_facets_in_a_fixed_order():
    """528 faces: interleaved ids with an empty group and a one-facet group, and all faces in one group (three strided
    passes).  Group rows against the exactly rounded sums (math.fsum) of the RETURNED facet rows: the reduction alone,
    (ceil(L / 256) + 9) 2^-53 sum |row|, doubled as everywhere.  The bytes of a group do not change when other groups
    come or go, nor when the call is repeated; shuffled input comes back in input order"""
    ref = reference("box8x6x6")
    cells, local = ref["cells"], ref["local"]
    n = cells.size
    ctx = loaded_context(ref)
    failures = []
    group = interleaved_groups(n)
    group[group == 3] = 1
    group[77] = 3                                                            # group 3: one facet; group 2: empty
    layouts = {"interleaved": (group, 5), "one group": (np.zeros(n, dtype=np.int32), 1)}
    kept = {}
    for label, (g, ng) in layouts.items():
        ctx.wall_set_facets(cells, local, g, ng)
        sums, rows = compute(ctx)
        again, rows_again = compute(ctx)
        assert sums.tobytes() == again.tobytes() and rows.tobytes() == rows_again.tobytes()
        counts = np.bincount(g, minlength=ng)
        n_red = (counts + 255) // 256 + 9
        bound = 2.0 * n_red[:, None] * EPS * group_sums(np.abs(rows), g, ng)
        check("box8x6x6 %s: group rows against their facet rows" % label, sums, _exact_sums(rows, g, ng), bound,
              failures)
        kept[label] = (sums, rows)
    sums, rows = kept["interleaved"]
    assert np.array_equal(sums[3], rows[77]) and np.array_equal(sums[2], np.zeros(rows.shape[1]))
    assert sums[4].tobytes() == np.zeros(rows.shape[1]).tobytes()
    assert kept["one group"][1].tobytes() == rows.tobytes()                  # a facet row does not depend on the groups
    # a group alone, and with other groups around it in another numbering
    for gid in (0, 1, 3):
        sel = group == gid
        ctx.wall_set_facets(cells[sel], local[sel])
        alone, rows_alone = compute(ctx)
        assert alone[0].tobytes() == sums[gid].tobytes() and rows_alone.tobytes() == rows[sel].tobytes()
    renumbered = np.array([6, 2, 0, 4, 1], dtype=np.int32)[group]
    ctx.wall_set_facets(cells, local, renumbered, 7)
    moved = compute(ctx)[0]
    for gid in (0, 1, 3):
        assert moved[renumbered[group == gid][0]].tobytes() == sums[gid].tobytes()
    assert not moved[[1, 3, 5]].any()
    # shuffled input: the rows come back in the caller's order
    order = np.random.default_rng(3).permutation(n)
    ctx.wall_set_facets(cells[order], local[order], group[order], 5)
    sums_shuffled, rows_shuffled = compute(ctx)
    assert rows_shuffled.tobytes() == rows[order].tobytes()
    g_shuffled = group[order]
    bound = 2.0 * ((np.bincount(g_shuffled, minlength=5) + 255) // 256 + 9)[:, None] * EPS * \
        group_sums(np.abs(rows_shuffled), g_shuffled, 5)
    check("box8x6x6 shuffled: group rows against their facet rows", sums_shuffled,
          _exact_sums(rows_shuffled, g_shuffled, 5), bound, failures)
    # no facets at all
    ctx.wall_set_facets(np.zeros(0, np.int32), np.zeros(0, np.int32), None, 2)
    empty, no_rows = compute(ctx)
    assert empty.tobytes() == np.zeros((2, rows.shape[1])).tobytes() and no_rows.shape == (0, rows.shape[1])
    ctx.close()
    assert not failures, failures


def test_interior_facets_give_the_one_sided_trace():
    ref = reference("rect6x4")
    mesh, dm = ref["mesh"], ref["dm"]
    interior = np.flatnonzero(~mesh.facet_on_boundary)[:7]
    cells, local = mesh.facet_cell_local(interior)
    want = wall_reference(mesh, dm, (cells, local), ref["u"], ref["p"], ref["T"], OPTS)
    bound = wall_bounds(mesh, dm, (cells, local), ref["u"], ref["p"], ref["T"], OPTS)
    ctx = loaded_context(ref)
    ctx.wall_set_facets(cells, local)
    rows = compute(ctx)[1]
    ctx.close()
    failures = []
    check("rect6x4 interior facets", rows, want, bound, failures)
    assert not failures, failures


# ---------------------------------------------------------------- viscosity laws
@pytest.mark.parametrize("name", ["rect6x4", "rect96x40", "box3x2x2", "box8x6x6", "general72", "general900"])
@pytest.mark.parametrize("law", sorted(LAWS))
def test_laws_equal_the_restatement(name, law):
    ref = reference(name)
    mesh, dm = ref["mesh"], ref["dm"]
    facets = (ref["cells"], ref["local"])
    key = ("law", law)
    if key not in ref:
        ref[key] = (wall_reference(mesh, dm, facets, ref["u"], ref["p"], ref["T"], OPTS, LAWS[law]),
                    wall_bounds(mesh, dm, facets, ref["u"], ref["p"], ref["T"], OPTS, LAWS[law],
                                groups=(ref["group"], N_GROUPS)))
    want, (bf, bg) = ref[key]
    ctx = loaded_context(ref)
    ctx.set_viscosity_law(*LAWS[law])
    ctx.wall_set_facets(ref["cells"], ref["local"], ref["group"], N_GROUPS)
    sums, rows = compute(ctx, use_law=True)
    sums_off, rows_off = compute(ctx, use_law=False)
    ctx.close()
    dim = dm.dim
    visc = slice(1 + dim, 1 + 2 * dim)
    assert np.abs(want[:, visc] - ref["rows"][:, visc]).max() > 1e3 * bf[:, visc].max()     # the law changes the traction
    failures = []
    check("%s %s facet rows" % (name, law), rows, want, bf, failures)
    check("%s %s group rows" % (name, law), sums, group_sums(want, ref["group"], N_GROUPS), bg, failures)
    check("%s %s switched off" % (name, law), rows_off, ref["rows"], ref["bound_rows"], failures)
    assert not failures, failures


@pytest.mark.parametrize("name", ["rect6x4", "box3x2x2"])
def test_use_law_without_a_law_is_the_constant_viscosity_code(name):
    ref = reference(name)
    ctx = loaded_context(ref)
    ctx.wall_set_facets(ref["cells"], ref["local"], ref["group"], N_GROUPS)
    sums, rows = compute(ctx, use_law=False)
    sums_law, rows_law = compute(ctx, use_law=True)
    ctx.set_viscosity_law(SMAGORINSKY, (0.17, ))
    ctx.set_viscosity_law(0)
    sums_back, rows_back = compute(ctx, use_law=True)
    ctx.close()
    assert sums.tobytes() == sums_law.tobytes() == sums_back.tobytes()
    assert rows.tobytes() == rows_law.tobytes() == rows_back.tobytes()


# ---------------------------------------------------------------- refused calls, untouched state, uploads
def _all_states(ctx):
    """the bytes of every state slot of the ABI (NSFEM_N_SLOTS of include/nsfem.h); slots that hold no data on this
    context (get_state refuses them) are recorded as None; the velocity and pressure levels must be there"""
    import re
    with open(os.path.join(HERE, os.pardir, "include", "nsfem.h")) as fh:
        n_slots = int(re.search(r"NSFEM_N_SLOTS\s*=\s*(\d+)", fh.read()).group(1))
    assert n_slots == nat.N_SLOTS
    out = {}
    for slot in range(n_slots):
        try:
            out[slot] = ctx.get_state(slot).tobytes()
        except nat.NativeError:
            out[slot] = None
    assert all(out[slot] is not None for slot in (nat.U0, nat.U1, nat.U2, nat.USTAR, nat.P, nat.P_OLD))
    return out


def test_refusals_leave_the_counters_and_the_state_alone():
    import ctypes as C
    ref = reference("rect6x4")
    cells, local, group = ref["cells"], ref["local"], ref["group"]
    n_cells = ref["mesh"].cells.shape[0]
    ctx = loaded_context(ref, scalar=False)
    assert ctx.wall_info() == dict(facets=0, groups=0, computes=0, uploads=0)
    with pytest.raises(nat.NativeError, match="no facet set"):
        compute(ctx, scalar=False)
    assert ctx.wall_info() == dict(facets=0, groups=0, computes=0, uploads=0)
    # bad facet sets: nothing becomes resident
    bad_cell, bad_local, bad_group = cells.copy(), local.copy(), group.copy()
    bad_cell[3], bad_local[5], bad_group[7] = n_cells, 3, N_GROUPS
    low_cell, low_local, low_group = cells.copy(), local.copy(), group.copy()
    low_cell[0], low_local[0], low_group[0] = -1, -1, -1
    for args, what in (((bad_cell, local, group, N_GROUPS), "cell"), ((low_cell, local, group, N_GROUPS), "cell"),
                       ((cells, bad_local, group, N_GROUPS), "local"), ((cells, low_local, group, N_GROUPS), "local"),
                       ((cells, local, bad_group, N_GROUPS), "group"), ((cells, local, low_group, N_GROUPS), "group"),
                       ((cells, local, None, 0), "n_groups"), ((cells, local, group, -2), "n_groups")):
        with pytest.raises(nat.NativeError, match=what):
            ctx.wall_set_facets(*args)
        assert ctx.wall_info() == dict(facets=0, groups=0, computes=0, uploads=0)
    ctx.wall_set_facets(cells, local, group, N_GROUPS)
    info = dict(facets=cells.size, groups=N_GROUPS, computes=0, uploads=1)
    assert ctx.wall_info() == info
    # a refused replacement keeps the resident set
    with pytest.raises(nat.NativeError, match="cell"):
        ctx.wall_set_facets(bad_cell, local, group, N_GROUPS)
    assert ctx.wall_info() == info
    before = _all_states(ctx)
    out = np.zeros((N_GROUPS, 9))
    opts = nat.WallOpts(0.1, 1.0, 0.0, (C.c_double * 3)(0.0, 0.0, 0.0), 0)
    lib, h = ctx._lib, ctx._h
    dp = out.ctypes.data_as(C.POINTER(C.c_double))
    assert lib.nsfem_wall_compute(h, nat.U0, nat.P, -1, None, dp, None) == -1           # null opts
    assert lib.nsfem_wall_compute(h, nat.U0, nat.P, -1, C.byref(opts), None, None) == -1    # null out_groups
    assert ctx.wall_info() == info
    for kw, what in ((dict(velocity_slot=nat.P), "velocity"), (dict(velocity_slot=nat.BODY_FORCE), "velocity"),
                     (dict(velocity_slot=99), "velocity"), (dict(pressure_slot=nat.U0), "pressure"),
                     (dict(pressure_slot=-1), "pressure"), (dict(scalar_slot=nat.T_SOURCE), "scalar"),
                     (dict(scalar_slot=nat.U0), "scalar"), (dict(scalar_slot=nat.T0), "nsfem_set_scalar"),
                     (dict(nu=np.nan), "finite"), (dict(symmetric=np.inf), "finite"), (dict(kappa=-np.inf), "finite"),
                     (dict(origin=(0.0, np.nan)), "finite"), (dict(origin=(0.0, 0.0, np.inf)), "finite")):
        args = dict(nu=0.1)
        args.update(kw)
        with pytest.raises(nat.NativeError, match=what):
            ctx.wall_compute(**args)
        assert ctx.wall_info() == info
    assert not out.any()
    # a compute call reads the state and writes none of it; the second call of a set uploads nothing
    compute(ctx, scalar=False)
    assert ctx.wall_info() == dict(info, computes=1)
    compute(ctx, scalar=False)
    assert ctx.wall_info() == dict(info, computes=2)
    assert _all_states(ctx) == before
    ctx.set_scalar(OPTS["kappa"])
    ctx.set_state(nat.T0, ref["T"])
    before = _all_states(ctx)
    assert all(before[slot] is not None for slot in (nat.U0, nat.U1, nat.P, nat.T0, nat.T1, nat.T2))
    sums, rows = compute(ctx)
    assert _all_states(ctx) == before and ctx.wall_info() == dict(info, computes=3)
    failures = []
    check("rect6x4 after the refusals", rows, ref["rows"], ref["bound_rows"], failures)
    assert not failures, failures
    # without a scalar slot the two temperature entries are +0.0
    rows_no_T = compute(ctx, scalar=False)[1]
    assert rows_no_T[:, 6:8].tobytes() == np.zeros((cells.size, 2)).tobytes()
    keep = [0, 1, 2, 3, 4, 5, 8]
    assert rows_no_T[:, keep].tobytes() == rows[:, keep].tobytes()
    ctx.close()


def test_a_scalar_level_without_storage_is_refused_and_not_allocated():
    """a compute call allocates nothing: a level of the scalar that was never set or stepped is refused"""
    ref = reference("rect6x4")
    ctx = loaded_context(ref, scalar=False)
    ctx.set_scalar(OPTS["kappa"])
    ctx.wall_set_facets(ref["cells"], ref["local"])
    info = ctx.wall_info()
    with pytest.raises(nat.NativeError, match="no data"):
        ctx.wall_compute(0.1, scalar_slot=nat.T1)
    assert ctx.wall_info() == info
    ctx.set_state(nat.T1, ref["T"])
    rows = ctx.wall_compute(0.1, kappa=OPTS["kappa"], scalar_slot=nat.T1, facets=True)[1]
    assert np.abs(rows[:, 6:8]).min() > 0.0 and ctx.wall_info() == dict(info, computes=1)
    ctx.close()


def test_a_context_with_a_communicator_is_refused():
    ref = reference("rect6x4")
    group = nat.local_group_create(1)
    ctx = loaded_context(ref, scalar=False)
    ctx.attach_local_comm(group, 0)
    with pytest.raises(nat.NativeError, match="communicator"):
        ctx.wall_set_facets(ref["cells"], ref["local"])
    with pytest.raises(nat.NativeError, match="communicator"):
        compute(ctx, scalar=False)
    assert ctx.wall_info() == dict(facets=0, groups=0, computes=0, uploads=0)
    ctx.close()


# ---------------------------------------------------------------- python layer and the solvers
_CAVITY = dict(name="Cavity", mesh=("cube", 2, 8), scheme="ipcs", clock=dict(dt=0.5 / 8, steps=3),
               bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_slip", "bottom"), ("velocity", "top", (1.0, 0.0))])


def _solver_reference(solver, wall, T=None, law=None):
    """restatement rows, facet bounds and group bounds of the solver's own returned state for the facets of ``wall``"""
    ctx, dm, mesh = solver._ctx, solver._dofmap, solver._mesh
    u, p = ctx.get_state(nat.U0).reshape(-1, dm.dim), ctx.get_state(nat.P)
    opts = dict(nu=wall._options()["nu"], sym=1.0, kappa=wall.kappa, origin=wall._origin)
    facets = (wall._cells, wall._local)
    rows = wall_reference(mesh, dm, facets, u, p, T, opts, law)
    bf, bg = wall_bounds(mesh, dm, facets, u, p, T, opts, law, groups=(wall._group, len(wall.boundary_ids)))
    return rows, bf, bg


def test_wall_quantities_through_the_imex_problem():
    """cavity 8 x 8, IMEXIPCSSolver, 3 steps through InstationaryProblem with _add_wall_quantities(every=1): three
    records, the last equal to a direct compute() on the final state; compute() / distribution() equal the ABI rows"""
    from ns_imex_solver import IMEXIPCSSolver
    from problem_specs import build_problem
    problem = build_problem(dict(_CAVITY, numbers=dict(Re=100.0), start={"velocity": (0.0, 0.0), "pressure": 0.0}))
    problem.set_solver_class(IMEXIPCSSolver)
    problem.compute_cfl = False
    problem.setup_mesh()
    ids = (problem._sides["top"], problem._sides["bottom"], problem._sides["left"])
    wall = problem._add_wall_quantities(ids, origin=(0.5, 0.5), every=1)
    problem.solve_problem()
    solver = problem._get_solver()
    assert problem._time_stepping.step_number == 3 and len(wall.times) == 3
    assert np.allclose(wall.times, [0.0625, 0.125, 0.1875], atol=1e-14)
    # nsfem_advance copies U0 -> U1, P -> P_OLD and keeps U0 / P: a direct compute() sees the state of the last record
    ctx = solver._ctx
    assert ctx.wall_info()["uploads"] == 1 and ctx.wall_info()["computes"] == 3
    res = wall.compute()
    sums0, rows0 = wall.rows(facets=True)
    cols0 = wq.split_rows(sums0, 2)
    for g, bid in enumerate(ids):
        last = {key: wall.series[bid][key][-1] for key in wq.KEYS}
        for key in wq.KEYS:
            assert np.array_equal(last[key], res[bid][key]), key
        assert last["area"] == cols0["area"][g] == 1.0
        assert np.array_equal(last["pressure_force"], cols0["pressure_force"][g])
        assert np.array_equal(last["viscous_force"], cols0["viscous_force"][g])
        assert np.array_equal(last["force"], cols0["pressure_force"][g] + cols0["viscous_force"][g])
        assert last["torque"] == cols0["torque"][g] and last["mass_flux"] == cols0["mass_flux"][g]
        assert last["mean_temperature"] == 0.0 and last["heat_flux"] == 0.0
        assert not np.array_equal(wall.series[bid]["force"][0], wall.series[bid]["force"][-1])     # the flow develops
    assert abs(wall.series[ids[0]]["viscous_force"][-1][0]) > 1e-3           # the lid drags the fluid
    dist = wall.distribution(ids[0])
    top = wq.split_rows(rows0[:8], 2)
    assert dist["area"].shape == (8, ) and np.allclose(dist["normals"], [0.0, 1.0]) and np.allclose(dist["midpoints"][:, 1], 1.0)
    assert np.array_equal(dist["wall_shear_stress"][:, 0], (top["viscous_force"] / top["area"][:, None])[:, 0])
    assert np.array_equal(dist["wall_shear_stress"][:, 1], np.zeros(8))
    assert np.array_equal(dist["pressure"], -top["pressure_force"][:, 1] / top["area"])
    assert np.array_equal(dist["normal_velocity"], top["mass_flux"] / top["area"])
    # against the restatement of the returned state
    want, bf, bg = _solver_reference(solver, wall)
    failures = []
    check("cavity facet rows", rows0, want, bf, failures)
    check("cavity group rows", sums0, group_sums(want, wall._group, 3), bg, failures)
    assert not failures, failures
    # the one-shot form
    one = problem._compute_wall_quantities(ids, origin=(0.5, 0.5))
    assert np.array_equal(one[ids[0]]["force"], res[ids[0]]["force"]) and ctx.wall_info()["uploads"] == 2
    problem._compute_wall_quantities(ids, origin=(0.5, 0.5))
    assert ctx.wall_info()["uploads"] == 2                                   # its facet set stayed resident
    # a facet set made resident by hand takes the context's one set over: the instance notices and uploads its own again
    ctx.wall_set_facets(wall._cells[:3], wall._local[:3])
    assert ctx.wall_info()["facets"] == 3
    back = wall.compute()
    assert ctx.wall_info()["facets"] == wall._cells.size and ctx.wall_info()["uploads"] == 4
    for bid in ids:
        assert np.array_equal(back[bid]["force"], res[bid]["force"])


def test_conduction_between_heated_walls_has_nusselt_number_one():
    """BoussinesqIMEXSolver on 8 x 8, b = 0, u = 0, T = 1 - y as initial state between T = 1 (bottom) and T = 0 (top):
    after 3 steps Nu = 1 on both walls -- to the restatement of the solver's returned T under the derived bound, and
    to the analytic value with the tolerance of the conduction test of tests/test_scalar_transport_host.py (1e-11)"""
    from ns_boussinesq_solver import BoussinesqIMEXSolver
    from problem_specs import build_problem
    walls = [("no_slip", s) for s in ("left", "right", "bottom", "top")]
    problem = build_problem(dict(_CAVITY, bcs=walls, numbers=dict(Re=100.0),
                                 start={"velocity": (0.0, 0.0), "pressure": 0.0,
                                        "temperature": lambda X, t: 1.0 - X[:, 1]}))
    cls = type(problem)
    kappa = 0.05

    def set_temperature_coefficients(self):
        self._temperature_coefficients = dict(diffusivity=kappa, buoyancy=None)

    def set_temperature_boundary_conditions(self):
        self._temperature_bcs = [(self._sides["bottom"], 1.0), (self._sides["top"], 0.0)]
    cls.set_temperature_coefficients = set_temperature_coefficients
    cls.set_temperature_boundary_conditions = set_temperature_boundary_conditions
    problem.set_solver_class(BoussinesqIMEXSolver)
    problem.compute_cfl = False
    problem.setup_mesh()
    hot, cold = problem._sides["bottom"], problem._sides["top"]
    wall = problem._add_wall_quantities((hot, cold))
    problem.solve_problem()
    solver = problem._get_solver()
    assert len(wall.times) == 3 and wall.kappa == kappa
    nu_hot = wall.nusselt_number(hot, 1.0, 1.0)
    nu_cold = wall.nusselt_number(cold, -1.0, 1.0)
    res = wall.compute()
    print("conduction: Nu(hot) - 1 = %.3e, Nu(cold) - 1 = %.3e" % (nu_hot - 1.0, nu_cold - 1.0))
    # the restatement of the returned T
    T = solver._ctx.get_state(nat.T0)
    want, bf, bg = _solver_reference(solver, wall, T=T)
    sums, rows = wall.rows(facets=True)
    failures = []
    check("conduction facet rows", rows, want, bf, failures)
    check("conduction group rows", sums, group_sums(want, wall._group, 2), bg, failures)
    heat = wq.split_rows(group_sums(want, wall._group, 2), 2)["heat_flux"]
    heat_bound = wq.split_rows(bg, 2)["heat_flux"]
    area = wq.split_rows(group_sums(want, wall._group, 2), 2)["area"]
    area_bound = wq.split_rows(bg, 2)["area"]
    for g, (bid, dT, nus) in enumerate(((hot, 1.0, nu_hot), (cold, -1.0, nu_cold))):
        # Nu = -heat / (kappa dT area), length 1: the bound of the heat flux, the relative one of the area, the formula
        nu_ref = wq.nusselt_number(heat[g], area[g], kappa, dT, 1.0)
        tol = heat_bound[g] / (kappa * area[g]) + abs(nu_ref) * (area_bound[g] / area[g] + 8.0 * EPS)
        print("conduction wall %d: |Nu - Nu(restatement)| / bound = %.3f" % (bid, abs(nus - nu_ref) / tol))
        assert abs(nus - nu_ref) <= tol
        assert res[bid]["heat_flux"] == wq.split_rows(sums, 2)["heat_flux"][g]
    assert abs(res[hot]["mean_temperature"] - 1.0) <= 1e-11 and abs(res[cold]["mean_temperature"]) <= 1e-11
    assert not failures, failures
    assert abs(nu_hot - 1.0) <= 1e-11 and abs(nu_cold - 1.0) <= 1e-11
    assert wall.series[hot]["heat_flux"][-1] == res[hot]["heat_flux"]
    assert res[hot]["heat_flux"] < 0.0 < res[cold]["heat_flux"]              # heat enters at the hot wall


def test_wall_shear_of_the_stationary_channel():
    """the Re = 1 channel of tests/test_solver_classes_gpu.py (CASES["stationary_channel"]: 10 x 1, n = 3, Poiseuille
    inlet 6 y (1 - y)) through the stationary solver: wall shear against the restatement of the returned state under
    the derived bound, and against the analytic value -- the traction of the wall on the fluid, c_v (grad u +
    grad u^T) n = -6 c_v e_x on both walls -- with the tolerance of that configuration's own velocity check, 1e-9
    (test_stationary_channel_flow_reproduces_poiseuille); the force is the shear integrated over the area 10"""
    from problem_specs import build_problem
    from test_solver_classes_gpu import CASES
    problem = build_problem(CASES["stationary_channel"]())
    problem.solve_problem()
    solver = problem._get_solver()
    bottom, top = problem._sides["bottom"], problem._sides["top"]
    res = problem._compute_wall_quantities((bottom, top))
    wall = next(iter(solver._wall_one_shot.values()))
    c_v = float(solver._equation_coefficients["viscous_term"])
    assert c_v == 1.0
    sums, rows = wall.rows(facets=True)
    want, bf, bg = _solver_reference(solver, wall)
    failures = []
    check("channel facet rows", rows, want, bf, failures)
    check("channel group rows", sums, group_sums(want, wall._group, 2), bg, failures)
    assert not failures, failures
    tol = 1e-9
    for bid in (bottom, top):
        dist = wall.distribution(bid)
        assert dist["area"].size == 30 and res[bid]["area"] == pytest.approx(10.0, abs=1e-13)
        print("channel wall %d: max |tau_x + 6| = %.3e, |F_x + 60| = %.3e"
              % (bid, np.abs(dist["wall_shear_stress"][:, 0] + 6.0 * c_v).max(), abs(res[bid]["viscous_force"][0] + 60.0)))
        assert np.abs(dist["wall_shear_stress"][:, 0] + 6.0 * c_v).max() <= tol
        assert np.abs(dist["wall_shear_stress"][:, 1]).max() == 0.0
        assert abs(res[bid]["viscous_force"][0] + 60.0 * c_v) <= tol * 10.0
        assert abs(res[bid]["mass_flux"]) <= tol * 10.0
