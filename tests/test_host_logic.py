"""CPU-only checks of the host side: mesh/dof-map counts, marker ids,
boundary-condition validation mirroring source/ns_solver_base.py:722-827, coefficient
handler arithmetic (source/auxiliary_classes.py:251-306), Expression stand-ins, and
that the C-ABI shared library loads and exports every symbol declared in
include/nsfem.h (no compute call is made without a GPU)."""
import os
import re

import numpy as np
import pytest

import _native as nat
import dlfn_compat as dlfn
import fem_host
from auxiliary_classes import EquationCoefficientHandler
from bdf_time_stepping import BDFTimeStepping
from fem_mesh import TaylorHoodDofMap, rectangle_mesh
from grid_generator import HyperCubeBoundaryMarkers, hyper_cube, hyper_rectangle, open_hyper_cube
from ns_ipcs_solver import IPCSSolver
from ns_solver_base import PressureBCType, TractionBCType, VelocityBCType

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("n", [1, 4, 25, 64])
def test_taylor_hood_counts(n):
    mesh, _ = hyper_cube(2, n)
    dm = TaylorHoodDofMap(mesh)
    assert mesh.num_cells() == 2 * n * n
    assert dm.n_p2 == (2 * n + 1) ** 2 and dm.n_p1 == (n + 1) ** 2
    assert dm.n_dofs == 2 * (2 * n + 1) ** 2 + (n + 1) ** 2
    # every cell sees 6 distinct P2 nodes; edge nodes sit at edge midpoints
    assert all(len(set(row)) == 6 for row in dm.p2_dofmap[:50])
    c = mesh.cells[0]
    mid = 0.5 * (mesh.coords[c[1]] + mesh.coords[c[2]])
    assert np.allclose(dm.p2_coords[dm.p2_dofmap[0, 3]], mid)
    # lexicographic lattice numbering
    assert np.all(np.diff(np.round(dm.p2_coords[:, 1] * 4 * n)) >= 0)


def test_config_sizes_of_the_survey():
    # S = 37,507 dofs (n = 64), L = 2,364,419 dofs (n = 512)
    for n, ndof in ((64, 37507), (512, 2364419), (333, 1001334), (25, 5878)):
        assert 2 * (2 * n + 1) ** 2 + (n + 1) ** 2 == ndof


def test_right_diagonal_and_markers():
    mesh, marks = hyper_rectangle((0.0, 0.0), (10.0, 1.0), (20, 2))
    assert mesh.num_vertices() == 21 * 3
    assert list(mesh.cells[0]) == [0, 1, 22] and list(mesh.cells[1]) == [0, 21, 22]
    ids = HyperCubeBoundaryMarkers
    assert [m.value for m in (ids.left, ids.right, ids.bottom, ids.top, ids.back, ids.front,
                              ids.opening)] == [1, 2, 3, 4, 5, 6, 7]
    assert marks.ids() == {1, 2, 3, 4}
    assert len(marks.facets_with_id(ids.left.value)) == 2
    assert len(marks.facets_with_id(ids.top.value)) == 20
    assert fem_host.boundary_normal(mesh, marks, ids.left.value) == (-1.0, 0.0)
    assert fem_host.boundary_normal(mesh, marks, ids.top.value) == (0.0, 1.0)
    mesh, marks = open_hyper_cube(2, 8, (("top", (0.5, 1.0), 0.5), ("left", (0.0, 0.5), 0.25)))
    assert marks.ids() == {1, 2, 3, 4, 7}
    assert len(marks.facets_with_id(7)) == 4 + 2


def test_coefficient_handler():
    c = EquationCoefficientHandler(Re=100.0, Fr=2.0).equation_coefficients
    assert c == dict(convective_term=1.0, coriolis_term=None, euler_term=None, pressure_term=1.0,
                     viscous_term=0.01, body_force_term=0.25)
    c = EquationCoefficientHandler(Ro=4.0, Ek=2.0).equation_coefficients
    assert c["coriolis_term"] == 0.25 and c["viscous_term"] == 0.5 and c["body_force_term"] is None
    c = EquationCoefficientHandler(Ek=0.1, Reynolds=10.0).equation_coefficients
    assert c["coriolis_term"] == 1.0 and c["viscous_term"] == 0.1
    h = EquationCoefficientHandler(Re=10.0)
    h.Re = 20.0
    assert h.Re == 20.0 and h.equation_coefficients["viscous_term"] == 0.05
    h.close()
    with pytest.raises(AssertionError):
        h.Re = 30.0


def test_expression_standin():
    e = dlfn.Expression(("6.0*x[1]/h*(1.0-x[1]/h)", "0.0"), h=1.0, degree=2)
    X = np.array([[0.0, 0.5], [1.0, 0.25]])
    np.testing.assert_allclose(e.eval_at(X), [[1.5, 0.0], [1.125, 0.0]])
    assert e.value_rank() == 1 and not dlfn.is_time_dependent(e)
    e = dlfn.Expression("sin(M_PI * t) * pow(x[0], 2)", t=0.5, degree=2)
    assert dlfn.is_time_dependent(e) and e.value_rank() == 0
    np.testing.assert_allclose(e.eval_at(X), [0.0, 1.0])
    e.t = 1.5
    np.testing.assert_allclose(e.eval_at(X), [0.0, -1.0])
    k = dlfn.Constant((0.0, -1.0))
    assert k.value_rank() == 1 and k.ufl_shape == (2,)
    np.testing.assert_allclose(dlfn.evaluate(k, X), [[0.0, -1.0], [0.0, -1.0]])


def test_load_and_traction_vectors():
    mesh, marks = hyper_rectangle((0.0, 0.0), (2.0, 1.0), (4, 3))
    dm = TaylorHoodDofMap(mesh)
    b = fem_host.load_vector(mesh, dm.p2_dofmap, dm.n_p2, lambda X: np.ones(X.shape[0]), degree=2)
    assert abs(b.sum() - 2.0) < 1e-13
    b = fem_host.load_vector(mesh, dm.p1_dofmap, dm.n_p1, lambda X: X[:, 0], degree=1)
    assert abs(b.sum() - 2.0) < 1e-13                      # int x over [0,2]x[0,1]
    t = fem_host.traction_vector(dm, marks.facets_with_id(2),
                                 lambda X: np.stack([X[:, 1] * (1 - X[:, 1]), 0 * X[:, 1]], axis=1))
    assert abs(t[0::2].sum() - 1.0 / 6.0) < 1e-14 and abs(t[1::2]).max() == 0.0


def _solver(bcs, traction=False):
    mesh, marks = hyper_cube(2, 2)
    s = IPCSSolver(mesh, marks, "standard", BDFTimeStepping(0.0, 1.0, desired_start_time_step=0.1))
    s.set_boundary_conditions(bcs)
    return s


def test_boundary_condition_validation():
    V, P, T = VelocityBCType, PressureBCType, TractionBCType
    s = _solver([(V.no_slip, 1, None), (V.constant, 4, (1.0, 0.0)), (P.constant, 2, 0.0)])
    assert len(s._velocity_bcs) == 2 and len(s._pressure_bcs) == 1
    with pytest.raises(AssertionError):      # unknown boundary id
        _solver([(V.no_slip, 9, None)])
    with pytest.raises(AssertionError):      # at least one velocity condition
        _solver([(P.constant, 2, 0.0)])
    with pytest.raises(AssertionError):      # wrong tuple size for the value
        _solver([(V.constant, 1, (1.0,))])
    with pytest.raises(AssertionError):      # full velocity + traction on one boundary
        _solver([(V.no_slip, 1, None), (T.constant, 1, (1.0, 0.0))])
    with pytest.raises(AssertionError):      # same component constrained twice
        _solver([(V.constant_component, 1, 0, 0.0), (T.constant_component, 1, 0, 1.0)])
    s = _solver([(V.constant_component, 1, 0, 0.0), (T.constant_component, 1, 1, 1.0),
                 (V.no_slip, 3, None)])
    from ns_solver_base import WeakFormViscousTerm
    assert s._form_viscous_term is WeakFormViscousTerm.traction_form


def test_solver_constructor_checks():
    mesh, marks = hyper_cube(2, 2)
    ts = BDFTimeStepping(0.0, 1.0, desired_start_time_step=0.1)
    with pytest.raises(AssertionError):
        IPCSSolver(mesh, marks, "upwind", ts)
    with pytest.raises(AssertionError):
        IPCSSolver(mesh, marks, "standard", ts, tol=1)
    s = IPCSSolver(mesh, marks, "standard", ts)
    assert s.field_association == {"velocity": 0, "pressure": 1}
    assert s.sub_space_association == {0: "velocity", 1: "pressure"}
    with pytest.raises(AssertionError):
        s.set_equation_coefficients({"viscosity": 1.0})


def test_library_exports_every_declared_symbol():
    header = open(os.path.join(ROOT, "include", "nsfem.h")).read()
    declared = set(re.findall(r"\b(nsfem_[a-z_0-9]+)\s*\(", header))
    assert declared, "no declarations parsed"
    assert declared == set(nat.EXPORTED_SYMBOLS)
    lib = nat.load_library()              # raises ImportError when the .so is missing
    for name in sorted(declared):
        assert hasattr(lib, name), name
    assert lib.nsfem_version() >= 1


def test_product_never_imports_the_oracle():
    pkg = os.path.join(ROOT, "navierstokes-with-fenics_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            text = open(os.path.join(pkg, fn)).read()
            assert "fem_oracle" not in text and "import oracle" not in text, fn


def test_expression_conditional_operator_and_annulus_mesh():
    """C++ conditional operator in Expression strings (used by the reference's rotating-flow test)
    and the in-repo annulus replacing mshr's spherical_shell."""
    import dlfn_compat as dlfn
    from grid_generator import SphericalAnnulusBoundaryMarkers, spherical_shell
    e = dlfn.Expression(("x[1]*w*((t >= ta) ? 1.0: t / ta)", "x[0] < 0.5 ? (x[1] > 0.2 ? 1.0 : 2.0) : pow(x[0], 2)"),
                        degree=2, w=2.0, ta=1.0, t=0.25)
    X = np.array([[0.1, 0.1], [0.1, 0.5], [2.0, 3.0]])
    assert np.allclose(e.eval_at(X), [[0.05, 2.0], [0.25, 1.0], [1.5, 4.0]])
    e.t = 3.0
    assert np.allclose(e.eval_at(X)[:, 0], 2.0 * X[:, 1])
    mesh, marks = spherical_shell(2, (0.25, 1.0), 60)
    ids = SphericalAnnulusBoundaryMarkers
    assert len(mesh.mg_levels) == 1
    r = np.hypot(*mesh.coords.T)
    assert abs(r.min() - 0.25) < 1e-14 and abs(r.max() - 1.0) < 1e-14
    for value, radius in ((ids.interior_boundary.value, 0.25), (ids.exterior_boundary.value, 1.0)):
        ends = mesh.edges[marks.facets_with_id(value)]
        assert ends.size and np.allclose(r[ends], radius)          # refined boundary vertices projected
    d1 = mesh.coords[mesh.cells[:, 1]] - mesh.coords[mesh.cells[:, 0]]
    d2 = mesh.coords[mesh.cells[:, 2]] - mesh.coords[mesh.cells[:, 0]]
    area = 0.5 * np.abs(d1[:, 0] * d2[:, 1] - d1[:, 1] * d2[:, 0]).sum()
    assert abs(area - np.pi * (1.0 - 0.25 ** 2)) < 5e-3


def test_box_mesh_kuhn_split_dofmap_and_nested_prolongation():
    """3D host pieces: dolfin BoxMesh vertex order and 6-tet Kuhn split, face markers, Taylor-Hood
    counts 3(2n+1)^3 + (n+1)^3, and the structured P1 prolongation -- exact for
    linear functions AND every fine vertex sits on a coarse edge (nested spaces)."""
    from fem_mesh import box_mesh
    from grid_generator import HyperCubeBoundaryMarkers as M, hyper_cube, hyper_rectangle
    from multigrid import structured_hierarchy, structured_prolongation_3d
    mesh, marks = hyper_cube(3, 4)
    assert mesh.num_cells() == 6 * 4 ** 3 and mesh.num_vertices() == 5 ** 3
    x = mesh.coords[mesh.cells.astype(np.int64)]
    vol = np.einsum("ci,ci->c", x[:, 1] - x[:, 0], np.cross(x[:, 2] - x[:, 0], x[:, 3] - x[:, 0])) / 6.0
    assert (vol > 0).all() and abs(vol.sum() - 1.0) < 1e-14
    assert np.allclose(mesh.coords[1], [0.25, 0, 0]) and np.allclose(mesh.coords[5], [0, 0.25, 0])
    # every cell contains the main diagonal of its cube
    lo, hi = x.min(axis=1), x.max(axis=1)
    has = lambda P: (np.abs(x - P[:, None, :]).max(axis=2) < 1e-14).any(axis=1)
    assert has(lo).all() and has(hi).all()
    dm = TaylorHoodDofMap(mesh)
    assert dm.n_dofs == 3 * 9 ** 3 + 5 ** 3
    for name, axis, value in (("left", 0, 0.0), ("right", 0, 1.0), ("bottom", 1, 0.0),
                              ("top", 1, 1.0), ("back", 2, 0.0), ("front", 2, 1.0)):
        f = marks.facets_with_id(M[name].value)
        assert f.size == 2 * 16 and np.allclose(mesh.facet_midpoints()[f, axis], value)
        nodes = np.unique(dm.facet_p2_nodes(f))
        assert nodes.size == 81 and np.allclose(dm.p2_coords[nodes, axis], value)
    assert marks.ids() == {m.value for m in (M.left, M.right, M.bottom, M.top, M.back, M.front)}
    mesh2, _ = hyper_rectangle((0.0, 0.0, 0.0), (2.0, 1.0, 0.5), (4, 2, 2))
    rowptr, col, val = structured_prolongation_3d(4, 2, 2)
    coarse = box_mesh((0.0, 0.0, 0.0), (2.0, 1.0, 0.5), 2, 1, 1)
    import scipy.sparse as sp
    P = sp.csr_matrix((val, col, rowptr), shape=(mesh2.num_vertices(), coarse.num_vertices()))
    lin = lambda X: 0.3 + 1.1 * X[:, 0] - 0.7 * X[:, 1] + 2.0 * X[:, 2]
    assert np.abs(P @ lin(coarse.coords) - lin(mesh2.coords)).max() < 1e-14
    ce = {tuple(e) for e in coarse.edges.tolist()}
    for r in range(P.shape[0]):
        cols = sorted(P.indices[P.indptr[r]:P.indptr[r + 1]].tolist())
        assert len(cols) == 1 or tuple(cols) in ce          # midpoint of an actual coarse edge
    levels = structured_hierarchy((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 8, 8, 8, coarsest=2)
    assert [lv[0].num_vertices() for lv in levels] == [125, 27]


def test_reference_module_names_resolve():
    """a user of the reference imports these names from these modules (PYTHONPATH=source)"""
    from auxiliary_methods import boundary_normal, extract_all_boundary_markers
    from grid_generator import hyper_cube, HyperCubeBoundaryMarkers as M
    mesh, marks = hyper_cube(2, 4)
    assert boundary_normal(mesh, marks, M.top.value) == (0.0, 1.0)
    assert boundary_normal(mesh, marks, M.left.value) == (-1.0, 0.0)
    assert extract_all_boundary_markers(mesh, marks) == {1, 2, 3, 4}
    mesh3, marks3 = hyper_cube(3, 2)
    assert boundary_normal(mesh3, marks3, M.front.value) == (0.0, 0.0, 1.0)
    import importlib
    for module, names in (("ns_problem", ("InstationaryProblem", "StationaryProblem", "VelocityBCType",
                                          "PressureBCType", "TractionBCType")),
                          ("ns_solver_base", ("SolverBase", "InstationarySolverBase", "StationarySolverBase")),
                          ("ns_bdf_solver", ("ImplicitBDFSolver",)), ("ns_ipcs_solver", ("IPCSSolver",)),
                          ("bdf_time_stepping", ("BDFTimeStepping",)), ("discrete_time", ("DiscreteTime",)),
                          ("imex_time_stepping", ("IMEXTimeStepping", "IMEXType")),
                          ("theta_time_stepping", ("GeneralThetaTimeStepping", "ThetaTimeSteppingType")),
                          ("auxiliary_classes", ("EquationCoefficientHandler", "AngularVelocityVector",
                                                 "FunctionTime")),
                          ("grid_generator", ("hyper_cube", "hyper_rectangle", "open_hyper_cube",
                                              "spherical_shell", "channel_with_cylinder", "blasius_plate",
                                              "backward_facing_step", "_extract_facet_markers")),
                          ("grid_tools", ("generate_xdmf_mesh",))):
        mod = importlib.import_module(module)
        for name in names:
            assert hasattr(mod, name), (module, name)


def test_p2_mass_element_bounds():
    """Extreme eigenvalues of diag(M_e)^-1 M_e for the P2 element mass matrix (affine elements:
    shape independent) = Wathen's bounds for the Jacobi-scaled global mass matrix; the native
    library computes them on the host for the Chebyshev mass solve."""
    import ctypes as C
    import _native as nat
    import sympy as sp
    lib = nat.load_library()
    for dim, expect in ((2, (0.39237, 2.05982)), (3, (0.25, 4.34747))):
        lo, hi = C.c_double(), C.c_double()
        assert lib.nsfem_p2_mass_bounds(dim, C.byref(lo), C.byref(hi)) == 0
        assert abs(lo.value - expect[0]) < 2e-5 and abs(hi.value - expect[1]) < 2e-5
    assert lib.nsfem_p2_mass_bounds(4, C.byref(lo), C.byref(hi)) != 0
    # independent check in 2D from exactly integrated P2 shape functions
    x, y = sp.symbols("x y")
    l = [1 - x - y, x, y]
    phi = [li * (2 * li - 1) for li in l] + [4 * l[1] * l[2], 4 * l[0] * l[2], 4 * l[0] * l[1]]
    M = np.array([[float(sp.integrate(sp.integrate(a * b, (y, 0, 1 - x)), (x, 0, 1))) for b in phi]
                  for a in phi])
    d = 1.0 / np.sqrt(np.diag(M))
    ev = np.linalg.eigvalsh(d[:, None] * M * d[None, :])
    lo, hi = C.c_double(), C.c_double()
    lib.nsfem_p2_mass_bounds(2, C.byref(lo), C.byref(hi))
    assert abs(ev[0] - lo.value) < 1e-10 and abs(ev[-1] - hi.value) < 1e-10


def test_grid_generator_entry_points_of_the_reference_tests(tmp_path):
    """tests/test_grid_generator.py:17-55 of the reference: every call it makes must construct a
    mesh; plus the properties the solver relies on (conformity, marker ids, radii)."""
    from grid_generator import (HyperCubeBoundaryMarkers as H, SphericalAnnulusBoundaryMarkers as S,
                                _extract_facet_markers, hyper_cube, hyper_rectangle, open_hyper_cube,
                                spherical_shell)
    hyper_cube(2, 8), hyper_cube(3, 8)
    hyper_rectangle((0.0, 0.0), (10.0, 1.0), 10), hyper_rectangle((0.0, 0.0), (10.0, 1.0), (50, 5))
    hyper_rectangle((0.0, 0.0, 0.0), (10.0, 1.0, 2.0), 8)
    hyper_rectangle((0.0, 0.0, 0.0), (10.0, 1.0, 2.0), (50, 5, 10))
    openings = (("left", (0.0, 0.5), 0.1), ("right", (1.0, 0.7), 0.1), ("bottom", (0.7, 0.0), 0.05),
                ("top", (0.5, 1.0), 0.8))
    _, marks = open_hyper_cube(2, 8, openings)
    assert H.opening.value in marks.ids()
    openings = (("left", (0.0, 0.5, 0.5), (0.1, 0.2)), ("right", (1.0, 0.7, 0.3), (0.1, 0.1)),
                ("bottom", (0.7, 0.0, 0.7), (0.05, 0.2)), ("top", (0.5, 1.0, 0.2), (0.8, 0.8)),
                ("back", (0.7, 0.3, 0.0), (0.05, 0.1)), ("front", (0.5, 0.25, 1.0), (0.2, 0.3)))
    mesh, marks = open_hyper_cube(3, 8, openings)
    opening = marks.facets_with_id(H.opening.value)
    # only the "top" window (0.8 x 0.8 around (0.5, ., 0.2), clipped by the cube) holds whole faces
    mid = mesh.facet_midpoints()[opening]
    assert opening.size == 48 and np.abs(mid[:, 1] - 1.0).max() < 1e-14
    assert marks.ids() == {1, 2, 3, 4, 5, 6, 7}
    with pytest.raises(AssertionError):
        open_hyper_cube(2, 8, (("front", (0.5, 0.5), 0.1), ))
    spherical_shell(2, (0.3, 1.0), 25)
    mesh, marks = spherical_shell(3, (0.3, 1.0), 25)
    # conforming: 4 faces per cell = 2 x interior faces + boundary faces
    assert 4 * mesh.cells.shape[0] == 2 * (mesh.facets.shape[0] - mesh.facet_on_boundary.sum()) + \
        mesh.facet_on_boundary.sum()
    x = mesh.coords[mesh.cells]
    vol = np.abs(np.linalg.det(x[:, 1:] - x[:, :1])) / 6.0
    assert vol.min() > 0.0 and abs(vol.sum() / (4.0 / 3.0 * np.pi * (1.0 - 0.3 ** 3)) - 1.0) < 0.01
    for marker, radius in ((S.interior_boundary, 0.3), (S.exterior_boundary, 1.0)):
        f = marks.facets_with_id(marker.value)
        assert f.size > 0
        assert np.abs(np.linalg.norm(mesh.coords[mesh.facets[f]], axis=2) - radius).max() < 1e-12
    assert marks.ids() == {S.interior_boundary.value, S.exterior_boundary.value}
    geo = tmp_path / "Example.geo"
    geo.write_text('Point(1) = {0, 0, 0};\nPhysical Curve("inlet", 100) = {1};\n'
                   "Physical Line('upper wall', 101) = {2, 3};\nPhysical Surface(\"fluid\", 5) = {1};\n")
    assert _extract_facet_markers(str(geo)) == {"inlet": 100, "upper wall": 101}


def _check_joint_and_split_assignments(solver, dlfn, Wh, WhSub):
    """Every variant of SolverBase._assign_function the reference's tests/test_function_assigner.py
    exercises -- joint -> split and split -> joint, with a two-entry dictionary, with one-entry
    dictionaries on the parts of ``joint.split()``, and with bare functions -- checked through
    point values of projected constants at (0.1, 0.1)."""
    point = (0.1, 0.1)
    joint = dlfn.Function(Wh)
    parts = {"velocity": dlfn.Function(WhSub["velocity"]), "pressure": dlfn.Function(WhSub["pressure"])}
    index = {"velocity": 0, "pressure": 1}

    def values_of_parts():
        return np.concatenate([np.atleast_1d(parts["velocity"](*point)), np.atleast_1d(parts["pressure"](*point))])

    for scale, style in ((1.0, "both"), (10.0, "single"), (100.0, "bare")):           # joint -> split
        target = scale * np.array([1.0, 2.0, 3.0])
        dlfn.project(dlfn.Constant(tuple(target)), Wh, function=joint)
        views = joint.split()
        if style == "both":
            solver._assign_function(parts, joint)
        for field in (() if style == "both" else ("velocity", "pressure")):
            receiver = {field: parts[field]} if style == "single" else parts[field]
            solver._assign_function(receiver, views[index[field]])
        assert np.allclose(values_of_parts(), target)
    expected = np.array(joint(*point))
    for scale, style in ((1.0, "both"), (10.0, "single"), (100.0, "bare")):           # split -> joint
        target = -scale * np.array([1.0, 2.0, 3.0])
        dlfn.project(dlfn.Constant(tuple(target[:2])), WhSub["velocity"], function=parts["velocity"])
        dlfn.project(dlfn.Constant(float(target[2])), WhSub["pressure"], function=parts["pressure"])
        if style == "both":
            solver._assign_function(joint, parts)
            assert np.allclose(joint(*point), target)
            expected = target.copy()
            continue
        views = joint.split()
        for field, entries in (("velocity", slice(0, 2)), ("pressure", slice(2, 3))):
            giver = {field: parts[field]} if style == "single" else parts[field]
            solver._assign_function(views[index[field]], giver)
            expected[entries] = target[entries]                  # the other field keeps its values
            assert np.allclose(joint(*point), expected)
    return joint, parts


def test_function_assigner_host_logic():
    """The checks of the reference's tests/test_function_assigner.py (forward / backward assignment
    between the joint Taylor-Hood space and its collapsed sub-spaces, with and without
    dictionaries, point values of projected constants) on the host-side function spaces -- the
    dof map stands in for the device context, which this logic never touches."""
    import dlfn_compat as dlfn
    from fem_mesh import TaylorHoodDofMap
    from fem_spaces import FunctionSpace
    from grid_generator import hyper_cube
    from ns_solver_base import SolverBase
    mesh, boundary_markers = hyper_cube(2, 5)
    solver = SolverBase(mesh, boundary_markers)
    solver._Wh = FunctionSpace(TaylorHoodDofMap(mesh), "mixed")
    Wh, WhSub = solver._Wh, solver._get_subspaces()
    assert solver._get_subspace("velocity") is WhSub["velocity"]
    joint, parts = _check_joint_and_split_assignments(solver, dlfn, Wh, WhSub)
    assert joint in Wh and parts["velocity"] in WhSub["velocity"]
    assert joint.split()[0] in Wh.sub(0) and joint.split()[0] not in WhSub["velocity"]
    # misuse is refused
    with pytest.raises(AssertionError):
        solver._assign_function(joint, joint)
    with pytest.raises(AssertionError):
        solver._assign_function({"velocity": parts["pressure"]}, joint)
    # non-constant data: a P2-representable field survives the round trip exactly
    u = dlfn.project(dlfn.Expression(("x[0]*x[1]", "1.0 - x[1]*x[1]"), degree=2), WhSub["velocity"])
    solver._assign_function(joint, {"velocity": u})
    assert np.allclose(joint(0.3, 0.7)[:2], [0.21, 0.51])



def test_periodic_multigrid_levels():
    """multigrid.periodic_levels: coarse levels of a periodic (constrained) P1 space -- slaves
    share their master's dof on every level, the prolongation rows sum to one, every coarse dof
    is injected from a finer dof, and smooth periodic functions interpolate with O(h^2) error."""
    import dlfn_compat as dlfn
    from fem_mesh import _compact, periodic_entity_map, rectangle_mesh
    from multigrid import periodic_levels, structured_hierarchy

    class Periodic(dlfn.SubDomain):
        def inside(self, x, on_boundary):
            return bool((dlfn.near(x[0], 0.0) or dlfn.near(x[1], 0.0)) and
                        not (dlfn.near(x[0], 1.0) or dlfn.near(x[1], 1.0)) and on_boundary)

        def map(self, x, y):
            for a in range(2):
                y[a] = x[a] - 1.0 if dlfn.near(x[a], 1.0) else x[a]

    import scipy.sparse as sp
    mesh = rectangle_mesh((0.0, 0.0), (1.0, 1.0), 16, 16)
    dm = TaylorHoodDofMap(mesh, periodic_map=periodic_entity_map(mesh, Periodic()))
    assert dm.n_p1 == 16 * 16
    levels = periodic_levels(structured_hierarchy(*mesh.structured, coarsest=2), dm.p1_vertex_node, Periodic())
    assert [int(d.max()) + 1 for _, _, d in levels] == [64, 16, 4]
    fine_xy = dm.p1_coords
    f = lambda X: np.sin(2 * np.pi * X[:, 0]) * np.cos(2 * np.pi * X[:, 1])
    errs = []
    for cmesh, (rowptr, col, val), dofmap in levels:
        n_c = int(dofmap.max()) + 1
        P = sp.csr_matrix((val, col, rowptr), shape=(fine_xy.shape[0], n_c))
        assert abs(P.sum(axis=1) - 1.0).max() < 1e-14
        single = np.diff(rowptr) == 1
        assert np.array_equal(np.sort(col[rowptr[:-1][single]]), np.arange(n_c))      # injection
        vm = periodic_entity_map(cmesh, Periodic())[1]
        cdof = _compact(np.arange(cmesh.num_vertices())[vm])
        assert np.array_equal(cdof[cmesh.cells], dofmap)
        xy = np.zeros((n_c, 2))
        masters = np.nonzero(vm == np.arange(cmesh.num_vertices()))[0]
        xy[cdof[masters]] = cmesh.coords[masters]
        errs.append(np.abs(P @ f(xy) - f(fine_xy)).max())
        fine_xy = xy
    assert errs[0] < 0.16 and errs[0] < errs[1]


def test_periodic_slab_partition_host_side():
    """partition.PeriodicSlabPartition: every global dof of the triple-periodic box is owned by
    exactly one rank, ghost copies sit at the owners' coordinates (mod the period), the halo
    ranges are whole lattice planes, the periodic prolongations interpolate constants."""
    import scipy.sparse as sp
    from partition import PeriodicSlabPartition
    size = 4
    parts = [PeriodicSlabPartition((0.0, 0.0, 0.0), (1.0, 1.0, 2.0), 4, 4, 8, r, size, coarsest=2,
                                   global_coarsest=None) for r in range(size)]
    p = parts[0]
    assert p.n_p2_global == 4 * 16 * 16 and p.n_p1_global == 16 * 8
    cov2, cov1 = np.zeros(p.n_p2_global, int), np.zeros(p.n_p1_global, int)
    G2 = np.zeros((p.n_p2_global, 3))
    for q in parts:
        np.add.at(cov2, q.p2_global[q.p2_owned], 1)
        np.add.at(cov1, q.p1_global[q.p1_owned], 1)
        G2[q.p2_global[q.p2_owned]] = q.dofmap.p2_coords[q.p2_owned]
    assert cov2.min() == cov2.max() == 1 and cov1.min() == cov1.max() == 1
    for q in parts:
        d = np.abs(G2[q.p2_global] - q.dofmap.p2_coords)
        d[:, 2] = np.minimum(d[:, 2], np.abs(d[:, 2] - 2.0))              # z period 2
        assert d.max() < 1e-14
        w2, w1 = q.w2, q.fine.w1
        assert q.p2_halo["send_up"] == (w2 * 4, w2) and q.p2_halo["recv_below"] == (0, w2)
        assert q.p1_halo["recv_above"] == (w1 * 3, w1) and q.p1_halo["send_down"] == (w1, w1)
        assert len(q.levels) == 1
        lev, (rowptr, col, val) = q.levels[0]
        P = sp.csr_matrix((val, col, rowptr))
        assert P.shape == (q.dofmap.n_p1, lev.n_p1) and abs(P.sum(axis=1) - 1.0).max() < 1e-14
        assert lev.dofmap.max() + 1 == lev.n_p1 == 2 * 2 * 3
    assert p.coarse_global_shape == (2, 2, 4)


def test_dolfin_shim_and_loud_failure_without_a_device():
    """``import dolfin`` resolves to the dolfin-free stand-ins when this package is on the path
    (the reference's demos run unchanged), and without a GPU the stationary driver reports the
    missing device instead of wandering into the Reynolds-number continuation."""
    import subprocess
    import sys
    code = (
        "import dolfin as dlfn\n"
        "from ns_problem import StationaryProblem, VelocityBCType\n"
        "from grid_generator import hyper_cube, HyperCubeBoundaryMarkers as M\n"
        "from auxiliary_classes import EquationCoefficientHandler\n"
        "assert dlfn.near(1.0, 1.0 + 1e-16) and dlfn.DOLFIN_EPS < 1e-14 and abs(dlfn.pi - 3.14159265) < 1e-6\n"
        "class P(StationaryProblem):\n"
        "    def setup_mesh(self):\n"
        "        self._mesh, self._boundary_markers = hyper_cube(2, 4)\n"
        "    def set_boundary_conditions(self):\n"
        "        lid = dlfn.Expression(('1.0', '0.0'), degree=2)\n"
        "        self._bcs = tuple((VelocityBCType.no_slip, m.value, None) for m in (M.left, M.right, M.bottom)) + \\\n"
        "            ((VelocityBCType.function, M.top.value, lid), )\n"
        "    def set_equation_coefficients(self):\n"
        "        self._coefficient_handler = EquationCoefficientHandler(Re=50.0)\n"
        "dlfn.set_log_level(40)\n"
        "P().solve_problem()\n")
    import torch
    env = dict(os.environ, PYTHONPATH=os.path.join(ROOT, "navierstokes-with-fenics_amd"), NSFEM_NO_OUTPUT="1")
    res = subprocess.run([sys.executable, "-c", code], env=env, capture_output=True, text=True, timeout=300,
                         cwd=os.getcwd())
    if torch.cuda.is_available():
        assert res.returncode == 0, res.stderr[-1500:]
    else:
        assert res.returncode != 0 and "no ROCm-capable device" in res.stderr and \
            "nonlinear solve failed" not in res.stderr


def test_cpp_expression_strings_follow_cpp_semantics():
    """dolfin compiles Expression strings as C++: ``&&`` / ``||`` / ``!`` are logical operators with
    lower precedence than comparisons, ``c ? a : b`` nests to the right, and a quotient of two
    integer literals truncates (``1/2*x[0]`` is zero)."""
    import dlfn_compat as dlfn
    X = np.array([[0.2, 0.3], [0.7, 0.2], [0.9, 0.9]])
    cases = {
        "x[0] > 0.5 && x[1] < 0.5 ? 1 : 0": [0.0, 1.0, 0.0],
        "!(x[0] > 0.5) ? 2.0 : -1.0": [2.0, -1.0, -1.0],
        "x[0] < 0.3 || x[1] > 0.8 ? 1.0 : (x[0] > 0.6 ? 2.0 : 3.0)": [1.0, 2.0, 1.0],
        "1/2*x[0]": [0.0, 0.0, 0.0],
        "7 / 2 * x[0]": [0.6, 2.1, 2.7],
        "1.0/2*x[0]": [0.1, 0.35, 0.45],
        "std::pow(x[0], 2) + fabs(-x[1])": [0.34, 0.69, 1.71],
        "x[1]*omega* ( (t >= t_acc) ? 1.0: t / t_acc)": [0.075, 0.05, 0.225],
        "-1.0/4.0 * x[0]": [-0.05, -0.175, -0.225],
        "1e-3*x[0] + 2.5E2": [250.0002, 250.0007, 250.0009],
    }
    for code, expect in cases.items():
        e = dlfn.Expression(code, degree=2, omega=1.0, t_acc=1.0, t=0.25)
        assert np.allclose(e.eval_at(X), expect, rtol=0, atol=1e-14), code
    e = dlfn.Expression(("x[0] >= 0.5 && x[1] >= 0.5 ? 1.0 : 0.0", "0.0"), degree=1)
    assert e.eval_at(X).tolist() == [[0.0, 0.0], [0.0, 0.0], [1.0, 0.0]]
    with pytest.raises(SyntaxError):
        dlfn.Expression("x[0] +* 2", degree=1)
    with pytest.raises(SyntaxError):
        dlfn.Expression("x[0] ? 1.0", degree=1)


def test_form_language_functionals_on_host_functions():
    """The slice of dolfin's form language the reference's post-processing hooks use (FacetNormal,
    Measure / ds / dx, grad, .T, dot, indexing, assemble) on host Functions of the solver spaces:
    polynomial fields on the unit square / cube against values integrated by hand (Gauss' theorem)."""
    import dlfn_compat as dlfn
    import fem_spaces
    from fem_mesh import TaylorHoodDofMap
    from grid_generator import hyper_cube
    for dim, n in ((2, 3), (3, 2)):
        mesh, marks = hyper_cube(dim, n)
        dm = TaylorHoodDofMap(mesh)
        w = fem_spaces.Function(fem_spaces.FunctionSpace(dm, "mixed"))
        X, Y = dm.p2_coords, dm.p1_coords
        if dim == 2:
            u = np.stack([X[:, 0] ** 2 + X[:, 1], X[:, 0] * X[:, 1]], axis=1)
            force, flux, kinetic = [-0.5, 1.0], 1.5, 0.5 * (1 / 5 + 1 / 3 + 1 / 3 + 1 / 9)
        else:
            u = np.stack([X[:, 0] ** 2 + X[:, 1], X[:, 0] * X[:, 2], X[:, 2] ** 2 - X[:, 1]], axis=1)
            force, flux, kinetic = [-0.8, 1.0, 1.2], 2.0, None
        w.vector()[: dm.n_velocity] = u.ravel()
        w.vector()[dm.n_velocity:] = 1.0 + 2.0 * Y[:, 0] - Y[:, 1]
        vel, p = w.split()
        nrm = dlfn.FacetNormal(mesh)
        dA = dlfn.Measure("ds", domain=mesh, subdomain_data=marks)
        assert abs(dlfn.assemble(dlfn.dot(nrm, vel) * dA) - flux) < 1e-13
        d = dlfn.Constant(0.5) * (dlfn.grad(vel) + dlfn.grad(vel).T)
        traction = -p * nrm + 0.6 * dlfn.dot(d, nrm)
        assert np.allclose([dlfn.assemble(traction[i] * dA) for i in range(dim)], force, atol=1e-13)
        assert abs(dlfn.assemble(dlfn.Constant(1.0) * dA(1)) - 1.0) < 1e-14          # one side of the box
        assert abs(dlfn.assemble(dlfn.Constant(1.0) * dlfn.ds(domain=mesh)) - 2.0 * dim) < 1e-13
        if kinetic is not None:
            assert abs(dlfn.assemble(dlfn.Constant(0.5) * dlfn.dot(vel, vel) * dlfn.dx(domain=mesh)) - kinetic) < 1e-14
        # position-dependent coefficients and powers: int x_0^2 p dx
        xe = dlfn.Expression("x[0]", degree=1)
        val = dlfn.assemble(xe ** 2 * p * dlfn.dx(domain=mesh))
        assert abs(val - (1 / 3 + 2 / 4 - 0.5 / 3)) < 1e-14


@pytest.mark.parametrize("size", [2, 3, 5])
def test_graph_partition_of_the_dfg_hierarchy_host_side(size):
    """partition.GraphPartition (unstructured meshes, recursive coordinate bisection) without a
    device: balanced coarse cells, every node owned exactly once, the two sides of every
    neighbour pair list the same global nodes in the same order on every level, an emulated halo
    exchange + reverse add reproduce global vectors, the rank-local prolongations are the rows of
    the global one, and the interior-first numbering puts all ghosts at the end."""
    import scipy.sparse as sp
    import grid_generator as gg
    from partition import GraphPartition, recursive_bisection
    pts = np.random.default_rng(3).random((1000, 2))
    own = recursive_bisection(pts, size)
    counts = np.bincount(own, minlength=size)
    assert counts.max() - counts.min() <= size               # balanced to rounding at every split
    mesh, marks = gg.dfg_channel(4, 2)
    dm = TaylorHoodDofMap(mesh)
    parts = [GraphPartition(mesh, r, size, marks) for r in range(size)]
    assert sum(int(p.p2_owned.sum()) for p in parts) == dm.n_p2
    assert sum(int(p.p1_owned.sum()) for p in parts) == dm.n_p1
    coarse_counts = np.bincount(parts[0].cell_owner[-1], minlength=size)
    assert coarse_counts.max() - coarse_counts.min() <= size
    # ownership is a partition of unity in the global numbering
    seen = np.zeros(dm.n_p2, dtype=int)
    for p in parts:
        g2 = p.p2_global(dm)
        assert np.abs(p.dofmap.p2_coords - dm.p2_coords[g2]).max() < 1e-12
        seen[g2[p.p2_owned]] += 1
        # ghosts last, interior rows first
        first_ghost = int(np.argmax(p.p2_ghost != 0)) if p.p2_ghost.any() else p.p2_ghost.size
        assert not p.p2_ghost[:first_ghost].any() and p.p2_ghost[first_ghost:].all()
    assert (seen == 1).all()

    def families(p):
        yield p.p2_lists, p.p2_global(dm), dm.n_p2
        yield p.p1_lists, p.p1_global, dm.n_p1
        for l, (lev, _) in enumerate(p.levels):
            yield lev.p1_lists, lev.vertices, p.global_meshes[l + 1].num_vertices()

    fams = [list(families(p)) for p in parts]
    rng = np.random.default_rng(0)
    for f in range(len(fams[0])):
        n_glob = fams[0][f][2]
        xg = rng.standard_normal(n_glob)
        local = []
        for r, p in enumerate(parts):
            lists, gid, _ = fams[r][f]
            ghost = np.ones(gid.size, dtype=bool)
            x = xg[gid].copy()
            # which of my nodes are ghosts: everything in a receive list
            mask = np.zeros(gid.size, dtype=bool)
            mask[lists["recv_idx"]] = True
            x[mask] = np.nan                                   # to be filled by the exchange
            local.append((x, mask))
        # forward exchange: owners -> ghosts
        for r in range(size):
            lists, gid, _ = fams[r][f]
            for k, q in enumerate(lists["neighbour"]):
                lq, gq, _ = fams[q][f]
                m = list(lq["neighbour"]).index(r)
                s_idx = lq["send_idx"][lq["send_ptr"][m]:lq["send_ptr"][m + 1]]
                r_idx = lists["recv_idx"][lists["recv_ptr"][k]:lists["recv_ptr"][k + 1]]
                assert np.array_equal(gq[s_idx], gid[r_idx])
                assert not local[q][1][s_idx].any()             # only owned values are sent
                local[r][0][r_idx] = local[q][0][s_idx]
        for r in range(size):
            assert np.array_equal(local[r][0], xg[fams[r][f][1]])
        # reverse add: every local copy contributes 1 -> owners end up with the multiplicity
        mult = np.zeros(n_glob)
        for r in range(size):
            mult[fams[r][f][1]] += 1.0
        acc = [np.ones(fams[r][f][1].size) for r in range(size)]
        for r in range(size):
            lists, gid, _ = fams[r][f]
            for k, q in enumerate(lists["neighbour"]):
                lq = fams[q][f][0]
                m = list(lq["neighbour"]).index(r)
                s_idx = lists["send_idx"][lists["send_ptr"][k]:lists["send_ptr"][k + 1]]
                r_idx = lq["recv_idx"][lq["recv_ptr"][m]:lq["recv_ptr"][m + 1]]
                np.add.at(acc[r], s_idx, 1.0)
                assert r_idx.size == s_idx.size
        for r in range(size):
            gid, mask = fams[r][f][1], local[r][1]
            assert np.array_equal(acc[r][~mask], mult[gid][~mask])
    # rank-local prolongations = rows / columns of the global ones
    for p in parts:
        fine_vertices = p.fine.vertices
        for l, (lev, (rowptr, col, val)) in enumerate(p.levels):
            gr, gc, gv = mesh.mg_levels[l][1]
            G = sp.csr_matrix((gv, gc, gr), shape=(p.global_meshes[l].num_vertices(), p.global_meshes[l + 1].num_vertices()))
            L = sp.csr_matrix((val, col, rowptr), shape=(fine_vertices.size, lev.n_p1))
            assert abs(G[fine_vertices][:, lev.vertices] - L).max() < 1e-15
            assert np.allclose(np.asarray(L.sum(axis=1)).ravel(), 1.0)      # complete rows
            fine_vertices = lev.vertices
    # the local markers are the global ones: boundary nodes found per rank add up to the global set
    cyl = gg.DFGBoundaryMarkers.cylinder.value
    glob = set(np.unique(dm.facet_p2_nodes(marks.facets_with_id(cyl))).tolist())
    found = set()
    for p in parts:
        loc = np.unique(p.dofmap.facet_p2_nodes(p.markers.facets_with_id(cyl)))
        found |= set(p.p2_global(dm)[loc].tolist())
    assert found == glob


def test_bench_parent_only_spawns_and_supervises_its_ranks():
    """`python bench.py --gpus N` without a launcher environment: the parent decides to spawn BEFORE the HIP library or
    torch is loaded (so it never initialises a GPU), hands every child the rendezvous environment of
    torch.distributed.run, and turns a failing rank into a non-zero exit code.  In this GPU-less container every rank
    fails at nsfem_create -- the supervision is what is tested; the working path is the -m gpu test
    test_bench_spawns_its_own_rank_processes_on_a_shared_gpu."""
    import ast
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "bench.py")).read()
    tree = ast.parse(src)
    # the decision sits above the first import of the native module
    body = [n for n in tree.body]
    first_native = next(i for i, n in enumerate(body) if isinstance(n, ast.Import) and any(a.name == "_native" for a in n.names))
    spawn_if = next(i for i, n in enumerate(body) if isinstance(n, ast.If) and "_ranks_to_spawn" in ast.unparse(n.test))
    assert spawn_if < first_native
    ns = {"__file__": os.path.join(root, "bench.py"), "__name__": "bench_head"}
    exec(compile(ast.Module([n for n in body[:spawn_if] if isinstance(n, (ast.Import, ast.FunctionDef, ast.Assign))],
                            type_ignores=[]), "bench_head", "exec"), ns)
    env_keep = {k: os.environ.pop(k) for k in ("WORLD_SIZE",) if k in os.environ}
    try:
        assert ns["_ranks_to_spawn"](["--gpus", "4", "--steps", "3"]) == 4
        assert ns["_ranks_to_spawn"](["--gpus=2"]) == 2
        assert ns["_ranks_to_spawn"](["--steps", "3"]) == 0 and ns["_ranks_to_spawn"](["--gpus", "1"]) == 0
        assert ns["_ranks_to_spawn"](["--gpus", "4", "--local-ranks", "4"]) == 0
        os.environ["WORLD_SIZE"] = "4"
        assert ns["_ranks_to_spawn"](["--gpus", "4"]) == 0          # launched by torch.distributed.run: a rank, not a parent
    finally:
        os.environ.pop("WORLD_SIZE", None)
        os.environ.update(env_keep)
    from gpu_common import have_gpu
    if have_gpu():
        pytest.skip("a GPU is present: the spawned ranks would run (covered by the -m gpu test)")
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}
    res = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--cells", "16", "--steps", "1",
                          "--warmup", "1"], env=env, capture_output=True, text=True, timeout=300)
    assert res.returncode != 0
    assert "exited with code" in res.stderr and "no ROCm-capable device" in res.stderr
    assert res.stdout.strip() == ""


def test_bench_dump_outputs_whole_or_seeded_sample_within_the_budget(tmp_path):
    """bench.py --dump-outputs DIR: float64 .npy files, the arrays whole while they fit the 64 MB budget, beyond it a
    sample at sorted indices that is the same in every run; several ranks split the budget and suffix their files"""
    import importlib.util
    import types
    spec = importlib.util.spec_from_file_location("bench_module", os.path.join(ROOT, "bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    rng = np.random.default_rng(3)
    small = {"velocity": rng.random(2 * 65 * 65), "pressure": rng.random(33 * 33).astype(np.float32)}
    big = {"velocity": rng.random(6 * 10 ** 6), "pressure": rng.random(3 * 10 ** 6)}

    def dump(name, arrays, world=1):
        d = tmp_path / name
        for r in range(world):
            bench._dump_outputs(types.SimpleNamespace(dump_outputs=str(d)), r, world, arrays)
        return {f.name: np.load(f) for f in sorted(d.iterdir())}, sum(f.stat().st_size for f in d.iterdir())

    out, _ = dump("small", small)
    assert sorted(out) == ["pressure.npy", "velocity.npy"] and all(a.dtype == np.float64 for a in out.values())
    assert np.array_equal(out["velocity.npy"], small["velocity"]) and np.array_equal(out["pressure.npy"], small["pressure"])
    out1, size1 = dump("big1", big)
    out2, _ = dump("big2", big)
    assert size1 <= bench.DUMP_LIMIT_BYTES and out1["velocity.npy"].size > 0.9 * bench.DUMP_LIMIT_BYTES / 8 * 2 / 3
    for k in out1:
        assert np.array_equal(out1[k], out2[k]) and np.isin(out1[k], big[k.split(".")[0]]).all()
    outr, sizer = dump("ranks", big, world=2)
    assert sorted(outr) == ["pressure.rank0.npy", "pressure.rank1.npy", "velocity.rank0.npy", "velocity.rank1.npy"]
    assert sizer <= bench.DUMP_LIMIT_BYTES
    bench._dump_outputs(types.SimpleNamespace(dump_outputs=None), 0, 1, small)       # (no flag: a no-op)


def test_row_parallel_sparse_product_equals_the_serial_product_bitwise(monkeypatch):
    """Set-up of the algebraic Schur Laplacian (multigrid.attach_schur_laplacian): the sparse products D W D^T and
    P^T A P run in row blocks on host threads -- same arrays as scipy's serial product, bit for bit, sorted columns,
    empty rows and the single-thread path included."""
    import scipy.sparse as sp
    from multigrid import _matmul_rows_parallel
    rng = np.random.default_rng(11)
    n, k = 60000, 6
    A = sp.csr_matrix((rng.standard_normal(n * k), (np.repeat(np.arange(n), k), rng.integers(0, n // 3, n * k))),
                      shape=(n, n // 3))
    A.sum_duplicates()
    A = A.tolil(); A[100:140] = 0; A = A.tocsr(); A.eliminate_zeros()          # a stretch of empty rows
    B = A.T.tocsr()
    ref = (A @ B).tocsr()
    ref.sort_indices()
    for threads in ("1", "3", "8"):
        monkeypatch.setenv("NSFEM_HOST_THREADS", threads)
        C = _matmul_rows_parallel(A, B, min_rows=5000)
        assert C.shape == ref.shape and C.has_sorted_indices
        assert np.array_equal(C.indptr, ref.indptr) and np.array_equal(C.indices, ref.indices)
        assert np.array_equal(C.data, ref.data)


def test_interpolation_prolongation_between_non_nested_meshes():
    """multigrid.interpolation_prolongation: equals the nested prolongation for even sizes, reproduces linear functions
    between meshes of ceil(n / 2) cells, rows sum to 1 with weights in (0, 1], at most 3 entries per row; the structured
    hierarchy of BASELINE's 333 x 333 mesh runs down to 21 cells."""
    import scipy.sparse as sp
    from multigrid import interpolation_prolongation, structured_hierarchy, structured_prolongation
    for nx, ny in ((8, 6), (16, 16)):
        a = structured_prolongation(nx, ny)
        b = interpolation_prolongation(nx, ny, nx // 2, ny // 2)
        shape = ((nx + 1) * (ny + 1), (nx // 2 + 1) * (ny // 2 + 1))
        assert abs(sp.csr_matrix((a[2], a[1], a[0]), shape=shape) - sp.csr_matrix((b[2], b[1], b[0]), shape=shape)).max() == 0.0
    for nx, ny, cx, cy in ((333, 333, 167, 167), (25, 13, 13, 7), (9, 8, 5, 4)):
        rp, c, v = interpolation_prolongation(nx, ny, cx, cy)
        P = sp.csr_matrix((v, c, rp), shape=((nx + 1) * (ny + 1), (cx + 1) * (cy + 1)))
        X, Y = np.meshgrid(np.linspace(0, 1, nx + 1), np.linspace(0, 2, ny + 1), indexing="xy")
        Xc, Yc = np.meshgrid(np.linspace(0, 1, cx + 1), np.linspace(0, 2, cy + 1), indexing="xy")
        f = lambda x, y: 1.5 + 2.0 * x - 3.0 * y
        assert abs(P @ f(Xc, Yc).ravel() - f(X, Y).ravel()).max() < 1e-14
        assert abs(np.asarray(P.sum(axis=1)).ravel() - 1.0).max() < 1e-15
        assert v.min() > 0.0 and v.max() <= 1.0 and np.diff(rp).max() <= 3
        assert all(np.all(np.diff(c[rp[i]:rp[i + 1]]) > 0) for i in range(0, rp.size - 1, 97))     # sorted columns
    assert [m.structured[2:] for m, _ in structured_hierarchy((0, 0), (1, 1), 333, 333)] == \
        [(167, 167), (84, 84), (42, 42), (21, 21)]
    assert [m.structured[2:] for m, _ in structured_hierarchy((0, 0), (1, 1), 512, 512)] == \
        [(256, 256), (128, 128), (64, 64), (32, 32)]
    assert [m.structured[2:] for m, _ in structured_hierarchy((0, 0), (1, 1), 333, 333, allow_non_nested=False)] == []
    # 3D Kuhn meshes: equal to the nested prolongation for even sizes, linear functions reproduced otherwise
    from multigrid import interpolation_prolongation_3d, structured_prolongation_3d
    from fem_mesh import box_mesh
    a = structured_prolongation_3d(4, 6, 8)
    b = interpolation_prolongation_3d(4, 6, 8, 2, 3, 4)
    shape = (5 * 7 * 9, 3 * 4 * 5)
    assert abs(sp.csr_matrix((a[2], a[1], a[0]), shape=shape) - sp.csr_matrix((b[2], b[1], b[0]), shape=shape)).max() == 0.0
    rp, c, v = interpolation_prolongation_3d(9, 7, 5, 5, 4, 3)
    mf, mc = box_mesh((0, 0, 0), (1, 2, 3), 9, 7, 5), box_mesh((0, 0, 0), (1, 2, 3), 5, 4, 3)
    P = sp.csr_matrix((v, c, rp), shape=(mf.coords.shape[0], mc.coords.shape[0]))
    g = lambda X: 0.5 + X[:, 0] - 2.0 * X[:, 1] + 3.0 * X[:, 2]
    assert abs(P @ g(mc.coords) - g(mf.coords)).max() < 1e-13
    assert abs(np.asarray(P.sum(axis=1)).ravel() - 1.0).max() < 1e-15 and v.min() > 0.0 and np.diff(rp).max() <= 4
    # ... and it is the interpolant of THIS triangulation: a random nodal field evaluated in the coarse mesh's own cells
    rng = np.random.default_rng(0)
    field = rng.standard_normal(mc.coords.shape[0])
    T = mc.coords[mc.cells]
    A = np.stack([T[:, 1] - T[:, 0], T[:, 2] - T[:, 0], T[:, 3] - T[:, 0]], axis=2)
    for i in rng.integers(0, mf.coords.shape[0], 60):
        lam = np.linalg.solve(A, (mf.coords[i] - T[:, 0])[:, :, None])[:, :, 0]
        L = np.concatenate([1.0 - lam.sum(axis=1, keepdims=True), lam], axis=1)
        k = int(np.argmax(L.min(axis=1)))                     # the cell that holds the point
        assert abs((P @ field)[i] - (L[k] * field[mc.cells[k]]).sum()) < 1e-13
    assert [m.structured[2:] for m, _ in structured_hierarchy((0, 0, 0), (1, 1, 1), 50, 50, 50)] == \
        [(25, 25, 25), (13, 13, 13), (7, 7, 7)]


def test_fast_diagonalisation_factors_invert_the_oracle_stiffness_matrix():
    """poisson_fd: on the right-diagonal triangulation of a rectangle the P1 stiffness matrix of the ORACLE is the
    tensor sum K_y (x) W_x + W_y (x) K_x to round-off, and  V_y ((V_y^T R V_x) .* inv) V_x^T  solves with it -- all
    Neumann (singular, compatible right-hand side), Dirichlet on one or two whole sides, non-square lattices.  A
    Dirichlet set that is not a union of whole sides is refused."""
    import scipy.sparse as sp
    import fem_oracle as fo
    import poisson_fd as pf
    from fem_mesh import TaylorHoodDofMap, rectangle_mesh
    rng = np.random.default_rng(5)
    for nx, ny, sides in ((12, 7, ()), (16, 16, ("x1",)), (9, 20, ("y0", "x0")), (24, 24, ())):
        mesh = rectangle_mesh((0.0, 0.0), (1.5, 0.7), nx, ny)
        dm = TaylorHoodDofMap(mesh)
        A = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap).stiffness_p1().tocsr()
        W, H = nx + 1, ny + 1
        xs, ys = pf.lattice_lines(mesh)
        Kx, wx = pf.line_matrices(xs)
        Ky, wy = pf.line_matrices(ys)
        T = sp.kron(Ky, sp.diags(wx)) + sp.kron(sp.diags(wy), Kx)
        assert abs(A - T).max() < 1e-13 * abs(A).max()
        ids = np.arange(W * H).reshape(H, W)
        pick = {"x0": ids[:, 0], "x1": ids[:, -1], "y0": ids[0, :], "y1": ids[-1, :]}
        dn = np.unique(np.concatenate([pick[k] for k in sides])) if sides else np.zeros(0, np.int64)
        f = pf.factors(xs, ys, dn)
        assert f is not None and f["singular"] == (len(sides) == 0)
        r = rng.standard_normal(W * H)
        free = np.ones(W * H, bool)
        free[dn] = False
        r[~free] = 0.0
        if not sides:
            r -= r.mean()
        z = pf.apply_reference(f, r)
        assert np.abs((r - A @ z)[free]).max() < 1e-11 * np.abs(r).max()
        assert not sides or np.abs(z[~free]).max() == 0.0
    assert pf.side_pattern(5, 4, [0, 1]) is None
    assert pf.factors(np.linspace(0, 1, 5), np.linspace(0, 1, 4), [0, 1]) is None
    unstructured = rectangle_mesh((0.0, 0.0), (1.0, 1.0), 4, 4)
    unstructured.coords = unstructured.coords + 1e-3 * rng.standard_normal(unstructured.coords.shape)
    assert pf.lattice_lines(unstructured) is None


def test_structured_mesh_shortcuts_reproduce_the_sorted_entities_and_numberings():
    """Set-up shortcuts of round 4 (13.4 M-dof channel: mesh + dof-map construction 2.9 -> 0.8 s): the edges of
    box_mesh in closed form, the lexicographic P2 numbering of a structured mesh from the half-lattice position, the
    parity-class numbering from ONE composite sort key -- each must give exactly the arrays of the generic path
    (np.unique over the cell edges, np.lexsort over the coordinates)."""
    import fem_mesh as fm
    for shape in ((3, 2, 4), (5, 5, 5), (8, 3, 2)):
        m = fm.box_mesh((0.0, 0.0, 0.0), (2.0, 1.0, 1.5), *shape)
        ref = fm.Mesh(m.coords, m.cells)                      # no box shape: generic entity construction
        assert "edges" not in m.__dict__ and "facets" not in m.__dict__          # built on first use
        assert np.array_equal(ref.edges, m.edges) and np.array_equal(ref.cell_edges, m.cell_edges)
        assert np.array_equal(ref.facets, m.facets) and np.array_equal(ref.facet_edges, m.facet_edges)
        a = m.coords[m.cells.astype(np.int64)]
        vol = np.einsum("ci,ci->c", a[:, 1] - a[:, 0], np.cross(a[:, 2] - a[:, 0], a[:, 3] - a[:, 0]))
        assert (vol > 0).all()
    for mesh in (fm.box_mesh((0.0, 0.0, 0.0), (2.0, 1.0, 1.5), 3, 2, 4), fm.rectangle_mesh((0.0, 0.0), (1.0, 2.0), 5, 3)):
        fast = fm.TaylorHoodDofMap(mesh, reorder=True)
        structured = mesh.__dict__.pop("structured")
        slow = fm.TaylorHoodDofMap(mesh, reorder=True)        # coordinate lexsort
        mesh.structured = structured
        assert np.array_equal(fast.p2_dofmap, slow.p2_dofmap) and np.array_equal(fast.vertex_node, slow.vertex_node)
        assert np.array_equal(fast.edge_node, slow.edge_node) and np.array_equal(fast.p2_coords, slow.p2_coords)
    for mesh in (fm.box_mesh((0.0, 0.0, 0.0), (2.0, 1.0, 1.5), 6, 5, 9), fm.rectangle_mesh((0.0, 0.0), (1.0, 2.0), 12, 20)):
        dm = fm.TaylorHoodDofMap(mesh, reorder="parity")
        nv, dim = mesh.num_vertices(), mesh._dim
        xy = np.concatenate([mesh.coords, mesh.edge_midpoints()], axis=0)
        lo, hi = np.asarray(mesh.structured[0], float), np.asarray(mesh.structured[1], float)
        cells = np.asarray(mesh.structured[2:], float)
        q = np.round((xy - lo) * (2.0 * cells / (hi - lo))).astype(np.int64)
        cls = np.zeros(xy.shape[0], dtype=np.int64)
        for a in range(dim):
            cls |= (q[:, a] & 1) << a
        keys = tuple(q[:, k] for k in range(dim)) + (cls,)
        if dm.parity_block_y > 0:
            keys += (q[:, 1] // dm.parity_block_y,)
        order = np.lexsort(keys + (q[:, dim - 1] // dm.parity_block,))
        e2n = np.empty(xy.shape[0], dtype=np.int64)
        e2n[order] = np.arange(xy.shape[0])
        assert np.array_equal(e2n[:nv], dm.vertex_node) and np.array_equal(e2n[nv:], dm.edge_node)
