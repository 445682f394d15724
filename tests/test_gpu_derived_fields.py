"""Gradient-derived fields on the device (csrc/derived.hip: k_derived_cell<2|3, CELL|VERTEX|NODE>, k_derived_gather;
nsfem_derived_fields / _components / _info) against the numpy restatement pinned in tests/test_derived_fields_host.py,
and the callers: ``derived_fields.compute`` and ``ProblemBase._compute_derived_field(s)``.

Tolerance (derived, not measured; the derivation is in the docstring of tests/test_derived_fields_host.py): per entry
``2 n_terms 2^-53 A`` -- A the sum of the absolute contributions of that entry, from the absolute-value version of
the same sums (``derived_reference(..., absolute=True)``), n_terms the rounded operations along the longest chain that
ends in the entry (geometry, reference gradient, physical gradient, the kernel's barycentric combination of vertex
gradients, the quantity, and the rule's 7 / 15 terms for CELL or twice the longest run of cells around a node for
NODE), doubled for the restatement's own rounding.  The kernel forms G at the vertices and combines those; the
restatement evaluates the basis gradients at every point itself -- two routes to the same numbers.

Meshes: the smallest that take each path -- 48 cells (less than one wave), 768 cells (three workgroups, a ragged last
one), two tetrahedral boxes (24-byte node stride), the unstructured fixture (runs of uneven length in the node index)
and the periodic square (identified nodes).  The general tetrahedra of tests/general_tet_mesh.py with 72 and 384 cells:
cells of both orientations and of different volumes (the NODE weights |K| differ around a node), no zero in any
J^-1 (every entry of it takes part in every G_ab), irregular runs of cells around the nodes."""
import os

import numpy as np
import pytest

import _native as nat
from fem_mesh import TaylorHoodDofMap, box_mesh, rectangle_mesh
from general_tet_mesh import CUBE, SMALL, general_tets
from gpu_common import context
from periodic_meshes import periodic_fixture
from test_derived_fields_host import (CENTERS, QUANTITIES, analytic, derived_bound, derived_reference,
                                      polynomial_fields, polynomial_nodal, smooth_fields)
from test_flow_statistics_host import periodic_square

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
MESHES = ("rect6x4", "rect24x16", "box3x2x2", "box4x4x4", "fixture", "periodic", "general72", "general384", "pchan3")
EXPECTED_CELLS = dict(pchan3=108, rect6x4=48, rect24x16=768, box3x2x2=72, box4x4x4=384, general72=72, general384=384)
CENTER_NAMES = {nat.DERIVED_CELL: "CELL", nat.DERIVED_VERTEX: "VERTEX", nat.DERIVED_NODE: "NODE"}
_CACHE = {}


def _mesh(name):
    from mesh_io import read_msh
    if name == "rect6x4":
        mesh = rectangle_mesh((0.0, 0.0), (1.5, 1.0), 6, 4)
    elif name == "rect24x16":
        mesh = rectangle_mesh((0.0, 0.0), (1.5, 1.0), 24, 16)
    elif name == "box3x2x2":
        mesh = box_mesh((0.0, 0.0, 0.0), (1.5, 1.0, 1.0), 3, 2, 2)
    elif name == "box4x4x4":
        mesh = box_mesh((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 4, 4, 4)
    elif name == "fixture":
        mesh = read_msh(os.path.join(HERE, "golden", "square_v41.msh"))[0]
    elif name == "periodic":
        return periodic_square(8)
    elif name == "pchan3":                       # the 3D periodic channel of tests/periodic_meshes.py: identified nodes,
        return periodic_fixture(name)[:2]        # VERTEX values per cell corner, NODE values through the seam patches
    elif name in ("general72", "general384"):
        return general_tets(*(SMALL if name == "general72" else CUBE))[:2]
    else:
        raise ValueError(name)
    return mesh, TaylorHoodDofMap(mesh)


def reference(name):
    """mesh, dof map, the smooth fields and, per (quantity, centre), the restatement and the bound -- computed once per
    mesh and left unchanged"""
    if name not in _CACHE:
        mesh, dm = _mesh(name)
        if name in EXPECTED_CELLS:
            assert mesh.cells.shape[0] == EXPECTED_CELLS[name]
        u, p, T = smooth_fields(dm.p2_coords, dm.p1_coords)
        want = {(q, c): derived_reference(mesh, dm, u, p, T, q, c) for q in QUANTITIES for c in CENTERS}
        bound = {(q, c): derived_bound(mesh, dm, u, p, T, q, c) for q in QUANTITIES for c in CENTERS}
        _CACHE[name] = dict(mesh=mesh, dm=dm, u=u, p=p, T=T, want=want, bound=bound)
    return _CACHE[name]


def loaded_context(ref, scalar=True, fields=None):
    u, p, T = fields if fields is not None else (ref["u"], ref["p"], ref["T"])
    ctx = context(ref["mesh"], ref["dm"])
    if scalar:
        ctx.set_scalar(0.01)
        ctx.set_state(nat.T0, T)
    ctx.set_state(nat.U0, np.ascontiguousarray(u).ravel())
    ctx.set_state(nat.P, p)
    return ctx


def with_axis(a, want):
    """the device result with the component axis the restatement keeps"""
    return a.reshape(want.shape)


# ---------------------------------------------------------------- agreement with the restatement
@pytest.mark.parametrize("name", MESHES)
def test_every_quantity_at_every_centre_equals_the_restatement(name):
    ref = reference(name)
    ctx = loaded_context(ref)
    failures = []
    for center in CENTERS:
        got = ctx.derived_fields(QUANTITIES, center, nat.U0, nat.P, nat.T0)
        assert sorted(got) == list(QUANTITIES)
        for q in QUANTITIES:
            want, bound = ref["want"][(q, center)], ref["bound"][(q, center)]
            assert got[q].size == want.size and got[q].shape == (want.shape if want.shape[-1] > 1 else want.shape[:-1])
            err = np.abs(with_axis(got[q], want) - want)
            ratio = (err / np.maximum(bound, 1e-300)).max()
            print("%s %s quantity %d: max error %.3e, max error / bound %.3f (max |value| %.3e)"
                  % (name, CENTER_NAMES[center], q, err.max(), ratio, np.abs(want).max()))
            assert np.abs(want).max() > 1e-3                    # the fields exercise every quantity
            if not (err <= bound).all():
                failures.append((CENTER_NAMES[center], q, ratio))
    ctx.close()
    assert not failures, failures


@pytest.mark.parametrize("name", ["rect6x4", "box3x2x2", "fixture", "general72", "general384"])
def test_polynomial_fields_are_reproduced(name):
    """quadratic velocity, linear pressure, quadratic scalar: G is linear, every centre returns the analytic values"""
    ref = reference(name)
    mesh, dm = ref["mesh"], ref["dm"]
    poly = polynomial_fields(dm.dim)
    u, p, T = polynomial_nodal(dm, poly)
    ctx = loaded_context(ref, fields=(u, p, T))
    checked, failures = 0, []
    for center in CENTERS:
        got = ctx.derived_fields(QUANTITIES, center, nat.U0, nat.P, nat.T0)
        for q in QUANTITIES:
            want = analytic(mesh, dm, poly, q, center)
            if want is None:
                continue
            bound = derived_bound(mesh, dm, u, p, T, q, center)
            err = np.abs(with_axis(got[q], want) - want)
            print("%s %s quantity %d: max error %.3e, max error / bound %.3f"
                  % (name, CENTER_NAMES[center], q, err.max(), (err / bound).max()))
            if not (err <= bound).all():
                failures.append((CENTER_NAMES[center], q, (err / bound).max()))
            checked += 1
    ctx.close()
    assert checked == 20 and not failures, failures


# ---------------------------------------------------------------- masks, repeatability, launches
@pytest.mark.parametrize("name", ["rect24x16", "box3x2x2"])
def test_a_quantity_has_the_same_bytes_whatever_else_is_in_the_mask(name):
    ref = reference(name)
    ctx = loaded_context(ref)
    for center in CENTERS:
        together = ctx.derived_fields(QUANTITIES, center, nat.U0, nat.P, nat.T0)
        again = ctx.derived_fields(QUANTITIES, center, nat.U0, nat.P, nat.T0)
        for q in QUANTITIES:
            alone = ctx.derived_fields(q, center, nat.U0, nat.P, nat.T0 if q == nat.DERIVED_SCALAR_GRADIENT else -1)
            assert list(alone) == [q]
            assert alone[q].tobytes() == together[q].tobytes(), (center, q)
            assert again[q].tobytes() == together[q].tobytes(), (center, q)
        pair = ctx.derived_fields((nat.DERIVED_Q_CRITERION, nat.DERIVED_VORTICITY), center)
        assert sorted(pair) == [nat.DERIVED_VORTICITY, nat.DERIVED_Q_CRITERION]
        assert all(pair[q].tobytes() == together[q].tobytes() for q in pair)
    ctx.close()


def test_one_element_launch_per_call_and_one_gather_launch_for_nodes():
    ref = reference("rect6x4")
    ctx = loaded_context(ref)
    assert ctx.derived_info() == dict(cell_launches=0, gather_launches=0, calls=0, bytes=0)
    dim = ref["dm"].dim
    assert [ctx.derived_components(q) for q in QUANTITIES] == [1, 1, 1, 1, dim * dim, dim, dim]
    for center, gathers in ((nat.DERIVED_CELL, 0), (nat.DERIVED_VERTEX, 0), (nat.DERIVED_NODE, 1)):
        for quantities in (QUANTITIES, (nat.DERIVED_VORTICITY, ), (nat.DERIVED_SHEAR_RATE, nat.DERIVED_PRESSURE_GRADIENT)):
            before = ctx.derived_info()
            ctx.derived_fields(quantities, center, nat.U0, nat.P, nat.T0)
            after = ctx.derived_info()
            assert after["cell_launches"] - before["cell_launches"] == 1
            assert after["gather_launches"] - before["gather_launches"] == gathers
            assert after["calls"] - before["calls"] == 1
            assert after["bytes"] >= before["bytes"] > 0 or before["calls"] == 0
    # the private buffer is reused: the largest request so far sizes it
    size = ctx.derived_info()["bytes"]
    ctx.derived_fields(nat.DERIVED_DIVERGENCE, nat.DERIVED_CELL)
    assert ctx.derived_info()["bytes"] == size
    ctx.close()
    ctx3 = loaded_context(reference("box3x2x2"))
    assert [ctx3.derived_components(q) for q in QUANTITIES] == [3, 1, 1, 1, 9, 3, 3]
    ctx3.close()


def test_live_contexts_of_both_dimensions_keep_their_quadrature_rules():
    """the rule's tables sit in constant memory of the device, not in a context: a 2D context created and used while a
    3D context lives (and the other way round) must leave the other's CELL means as they were and as the restatement
    has them"""
    ref3, ref2 = reference("box3x2x2"), reference("rect6x4")

    def check(ctx, ref, first):
        got = ctx.derived_fields(QUANTITIES, nat.DERIVED_CELL, nat.U0, nat.P, nat.T0)
        for q in QUANTITIES:
            want, bound = ref["want"][(q, nat.DERIVED_CELL)], ref["bound"][(q, nat.DERIVED_CELL)]
            assert np.isfinite(got[q]).all(), q
            assert (np.abs(with_axis(got[q], want) - want) <= bound).all(), q
            if first is not None:
                assert got[q].tobytes() == first[q].tobytes(), q
        return got

    ctx3 = loaded_context(ref3)
    first3 = check(ctx3, ref3, None)
    ctx2 = loaded_context(ref2)                 # created while the 3D context lives, and after its first call
    first2 = check(ctx2, ref2, None)
    check(ctx3, ref3, first3)
    other3 = loaded_context(ref3)               # ... and a 3D context created after the 2D one has made its call
    check(other3, ref3, first3)
    check(ctx2, ref2, first2)
    check(ctx3, ref3, first3)
    for ctx in (ctx3, ctx2, other3):
        ctx.close()


# ---------------------------------------------------------------- nothing else is touched
@pytest.mark.parametrize("name", ["rect24x16", "box3x2x2"])
def test_a_call_leaves_the_state_and_the_element_buffers_alone(name):
    ref = reference(name)
    ctx = loaded_context(ref)
    ctx.set_viscosity_law(1, [0.17])

    def snapshot():
        return [ctx.get_state(s).tobytes() for s in (nat.U0, nat.P, nat.T0)] + \
            [ctx.viscosity_residual(nat.U0).tobytes(), ctx.scalar_convection(nat.U0, nat.T0).tobytes()]

    before = snapshot()
    for center in CENTERS:
        ctx.derived_fields(QUANTITIES, center, nat.U0, nat.P, nat.T0)
    assert snapshot() == before
    # ... and the other way round: the element kernels of the step in between do not change a derived field
    first = ctx.derived_fields(QUANTITIES, nat.DERIVED_NODE, nat.U0, nat.P, nat.T0)
    ctx.viscosity_residual(nat.U0)
    ctx.scalar_convection(nat.U0, nat.T0)
    second = ctx.derived_fields(QUANTITIES, nat.DERIVED_NODE, nat.U0, nat.P, nat.T0)
    assert all(first[q].tobytes() == second[q].tobytes() for q in QUANTITIES)
    ctx.close()


# ---------------------------------------------------------------- refused calls
def test_bad_arguments_are_refused_before_anything_is_launched():
    ref = reference("rect6x4")
    dm = ref["dm"]
    ctx = loaded_context(ref, scalar=False)
    ctx.derived_fields(nat.DERIVED_VORTICITY, nat.DERIVED_NODE)
    info = ctx.derived_info()
    V, D, S, PG = nat.DERIVED_VORTICITY, nat.DERIVED_DIVERGENCE, nat.DERIVED_SCALAR_GRADIENT, nat.DERIVED_PRESSURE_GRADIENT
    cases = [
        ("unknown quantity bit", lambda: ctx.derived_fields((V, 7), nat.DERIVED_CELL)),
        ("unknown quantity bit", lambda: ctx.derived_fields(31, nat.DERIVED_CELL)),
        ("unknown centre", lambda: ctx.derived_fields(V, 3)),
        ("unknown centre", lambda: ctx.derived_fields(V, -1)),
        ("empty quantity mask", lambda: ctx.derived_fields((), nat.DERIVED_CELL)),
        ("not a velocity slot", lambda: ctx.derived_fields(V, nat.DERIVED_CELL, velocity_slot=nat.P)),
        ("not a velocity slot", lambda: ctx.derived_fields(V, nat.DERIVED_CELL, velocity_slot=nat.BODY_FORCE)),
        ("not a velocity slot", lambda: ctx.derived_fields(V, nat.DERIVED_CELL, velocity_slot=99)),
        ("not a pressure slot", lambda: ctx.derived_fields(PG, nat.DERIVED_CELL, pressure_slot=nat.U1)),
        ("not a pressure slot", lambda: ctx.derived_fields(PG, nat.DERIVED_CELL, pressure_slot=-1)),
        ("not a pressure slot", lambda: ctx.derived_fields(V, nat.DERIVED_CELL, pressure_slot=nat.T0)),
        ("without nsfem_set_scalar", lambda: ctx.derived_fields(S, nat.DERIVED_NODE, scalar_slot=nat.T0)),
        ("without nsfem_set_scalar", lambda: ctx.derived_fields((V, S), nat.DERIVED_CELL, scalar_slot=-1)),
        ("not a level of the transported scalar", lambda: ctx.derived_fields(V, nat.DERIVED_CELL, scalar_slot=nat.U0)),
    ]
    for message, call in cases:
        with pytest.raises(nat.NativeError, match=message):
            call()
        assert ctx.derived_info() == info, message
    # a wrong out_len: through the C entry point itself
    import ctypes as C
    n = ref["mesh"].cells.shape[0]
    out = np.zeros(2 * n + 8)
    ptr = out.ctypes.data_as(C.POINTER(C.c_double))
    mask = (1 << V) | (1 << D)
    for bad in (2 * n - 1, 2 * n + 1, n, 0, -1):
        assert ctx._lib.nsfem_derived_fields(ctx._h, nat.U0, nat.P, -1, mask, nat.DERIVED_CELL, ptr, bad) == nat.ERR_ARG
        assert b"wrong size of the output" in ctx._lib.nsfem_last_error(ctx._h)
        assert ctx.derived_info() == info and not out.any()
    assert ctx._lib.nsfem_derived_fields(ctx._h, nat.U0, nat.P, -1, mask, nat.DERIVED_CELL, ptr, 2 * n) == nat.OK
    assert out[:2 * n].any() and not out[2 * n:].any()
    with pytest.raises(nat.NativeError, match="unknown quantity"):
        ctx.derived_components(7)
    # with a scalar: the slot must be one of its levels
    ctx.set_scalar(0.01)
    info = ctx.derived_info()
    for slot in (-1, nat.T_SOURCE, nat.P):
        with pytest.raises(nat.NativeError, match="not a level of the transported scalar"):
            ctx.derived_fields(S, nat.DERIVED_CELL, scalar_slot=slot)
        assert ctx.derived_info() == info
    assert ctx.derived_fields(S, nat.DERIVED_CELL, scalar_slot=nat.T0)[S].shape == (n, dm.dim)
    ctx.close()


def test_a_context_with_a_communicator_is_refused():
    ref = reference("rect6x4")
    group = nat.local_group_create(1)
    ctx = loaded_context(ref, scalar=False)
    ctx.attach_local_comm(group, 0)
    with pytest.raises(nat.NativeError, match="communicator"):
        ctx.derived_fields(nat.DERIVED_VORTICITY, nat.DERIVED_NODE)
    assert ctx.derived_info() == dict(cell_launches=0, gather_launches=0, calls=0, bytes=0)
    ctx.close()
    nat.local_group_destroy(group)


# ---------------------------------------------------------------- through the solver and the problem loop
def test_fields_of_a_cavity_run_through_the_problem_hooks():
    from ns_imex_solver import IMEXIPCSSolver
    from problem_specs import build_problem
    seen = []

    def hook(problem):
        ctx = problem._get_solver()._ctx
        before = ctx.derived_info()
        q_node, vort_cell = problem._compute_derived_field("q criterion"), problem._compute_derived_field("vorticity", "Cell")
        both = problem._compute_derived_fields(["q criterion", "shear rate", "velocity gradient"], "Node")
        after = ctx.derived_info()
        assert after["calls"] - before["calls"] == 3 and after["cell_launches"] - before["cell_launches"] == 3
        assert after["gather_launches"] - before["gather_launches"] == 2
        problem._add_to_field_output(q_node)
        problem._add_to_field_output(vort_cell)
        problem._add_to_field_output(both[2])
        host = problem._compute_vorticity()
        dm, mesh = problem._get_solver()._dofmap, problem._mesh
        u, p = ctx.get_state(nat.U0), ctx.get_state(nat.P)
        bound = derived_bound(mesh, dm, u, p, None, nat.DERIVED_VORTICITY, nat.DERIVED_CELL)[:, 0]
        seen.append(dict(q=q_node, vort=vort_cell, both=both, host=host.values.copy(), bound=bound,
                         n_vertices=mesh.coords.shape[0], n_cells=mesh.cells.shape[0]))

    spec = dict(name="Cavity", mesh=("cube", 2, 8), scheme="ipcs", numbers=dict(Re=100.0),
                clock=dict(dt=1.0 / 32.0, steps=2), start={"velocity": (0.0, 0.0), "pressure": 0.0}, postprocessing=1,
                output=1, hook=hook,
                bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_slip", "bottom"), ("velocity", "top", (1.0, 0.0))])
    problem = build_problem(spec)
    problem.set_solver_class(IMEXIPCSSolver)
    problem.compute_cfl = False
    problem.solve_problem()
    assert len(seen) == 2
    for s in seen:
        assert s["q"].center == "Node" and s["q"].name() == "q criterion" and s["q"].values.shape == (s["n_vertices"], )
        assert s["vort"].center == "Cell" and s["vort"].values.shape == (s["n_cells"], )
        err = np.abs(s["vort"].values - s["host"])
        print("cavity: cell vorticity, max error %.3e, max error / bound %.3f, max |value| %.3e"
              % (err.max(), (err / np.maximum(s["bound"], 1e-300)).max(), np.abs(s["host"]).max()))
        assert np.abs(s["host"]).max() > 1.0                     # the lid shears the top row of cells
        assert (err <= s["bound"]).all()
        assert s["both"][0].values.tobytes() == s["q"].values.tobytes()
        assert (s["both"][1].values >= 0.0).all() and s["both"][2].values.shape == (s["n_vertices"], 9)
    fname = problem._get_filename()
    assert os.path.isfile(fname)
    text = open(fname).read()
    assert 'Name="q criterion"' in text and 'Name="vorticity"' in text
    # what was handed to the output is what a reader finds: the velocity gradient as a 3 x 3 tensor per vertex
    from xdmf_io import read_xdmf
    assert '<Attribute Name="velocity gradient" AttributeType="Tensor" Center="Node">' in text
    assert '<Attribute Name="q criterion" AttributeType="Scalar" Center="Node">' in text
    assert '<Attribute Name="vorticity" AttributeType="Scalar" Center="Cell">' in text
    assert '<Attribute Name="velocity" AttributeType="Vector" Center="Node">' in text
    back = read_xdmf(fname)
    assert back["centers"]["velocity gradient"] == "Node" and back["centers"]["vorticity"] == "Cell"
    for key, pick in (("velocity gradient", lambda s: s["both"][2].values), ("q criterion", lambda s: s["q"].values),
                      ("vorticity", lambda s: s["vort"].values)):
        assert len(back["fields"][key]) == len(seen)
        for stored, s in zip(back["fields"][key], seen):
            assert stored.shape == pick(s).shape and stored.tobytes() == pick(s).tobytes(), key
    grad = back["fields"]["velocity gradient"][-1].reshape(-1, 3, 3)
    assert not grad[:, 2, :].any() and not grad[:, :, 2].any() and np.abs(grad[:, :2, :2]).max() > 1.0
    # the names and the error wrapping of the module
    import derived_fields
    solver = problem._get_solver()
    res = derived_fields.compute(solver, ["divergence", "pressure gradient"], "Vertex")
    n = seen[0]["n_cells"]
    assert res["divergence"].shape == (n, 3) and res["pressure gradient"].shape == (n, 3, 2)
    with pytest.raises(RuntimeError, match="without nsfem_set_scalar"):
        derived_fields.compute(solver, "temperature gradient", "Node")
