"""Drop-in check of the interface the reference's OWN test files exercise, one parametrized case per reference test
file (its name and test count are the case's id).  Self-contained: the reference's tests are not part of this
repository, so every case restates what its file exercises as this repository's checks --

* the files that need no solve -- BDF / IMEX / theta coefficient tables, DiscreteTime, the coefficient handler and
  angular velocity classes, boundary normals, the grid generators: one check per test of the file (the grid-generator
  test that downloads a .geo file is left out, as before), against the golden tables under tests/golden/ where the
  file pins numbers;
* the solver files: one problem per test of the file, built from the data-driven set-ups of
  tests/test_solver_classes_gpu.py (CASES, each citing the reference test it follows) through the product's problem
  classes.  With a device every problem solves; without one every problem gets through its imports, mesh,
  boundary-condition and coefficient set-up and stops exactly at the creation of the device context
  (``no ROCm-capable device``) -- never at a missing name, a changed signature or a failed assertion."""
import numpy as np
import pytest


# ------------------------------------------------------------------ files without a solve
def _bdf_table(order):
    from test_time_stepping import test_reference_golden_tables_and_restart
    test_reference_golden_tables_and_restart(order)


def _discrete_time():
    from test_time_stepping import test_discrete_time_random_walk_reaches_end
    test_discrete_time_random_walk_reaches_end()


def _imex(kind):
    from test_time_stepping import IMEX_THETA, check_imex_case
    cases = [c for c in IMEX_THETA["imex"] if c["kind"] == kind]
    assert cases
    for case in cases:
        check_imex_case(case)


def _theta(kind):
    from test_time_stepping import IMEX_THETA, check_theta_case
    cases = [c for c in IMEX_THETA["theta"] if c["kind"] == kind]
    assert cases
    for case in cases:
        check_theta_case(case)


def _angular_velocity_vector():
    from auxiliary_classes import AngularVelocityVector, FunctionTime

    class Steady(FunctionTime):
        def __init__(self):
            super().__init__(1)

        def value(self):
            return 2.0

    class Ramp(FunctionTime):
        def __init__(self):
            super().__init__(1)

        def value(self):
            return 3.0 * self._current_time

        def derivative(self):
            return 3.0

    class AboutZ(FunctionTime):
        def __init__(self):
            super().__init__(3)

        def value(self):
            return (0.0, 0.0, 1.5)

        def derivative(self):
            return (0.0, 0.0, 0.0)

    steady = AngularVelocityVector(2)
    steady.set_angular_velocity_function(Steady())
    steady.set_time(1.0)
    assert steady.space_dim == 2 and steady.value == 2.0 and steady.derivative is None
    ramp = AngularVelocityVector(2)
    ramp.set_angular_velocity_function(Ramp())
    ramp.set_time(0.5)
    assert ramp.value == 1.5 and ramp.derivative == 3.0
    about_z = AngularVelocityVector(3, function=AboutZ())
    about_z.set_time(1.0)
    assert about_z.space_dim == 3 and about_z.value == (0.0, 0.0, 1.5) and about_z.derivative == (0.0, 0.0, 0.0)


def _equation_coefficients():
    from auxiliary_classes import EquationCoefficientHandler
    eq = EquationCoefficientHandler(Reynolds=50.0)
    assert eq.Re == 50.0 and str(eq)
    eq.Fr = 10.0
    assert eq.equation_coefficients and eq.Fr == 10.0 and str(eq)
    eq.Ek = 25.0
    assert eq.equation_coefficients and eq.Ek == 25.0 and str(eq)
    eq = EquationCoefficientHandler()
    eq.Ro = 1.0
    eq.Ek = 25.0
    eq.Fr = 10.0
    assert eq.equation_coefficients and eq.Ro == 1.0 and str(eq)
    eq.clear()
    eq = EquationCoefficientHandler()
    eq.Ek = 1.0
    eq.Re = 25.0
    assert eq.equation_coefficients and str(eq)
    eq.modify_dimensionless_number("Re", 10.0)
    assert eq.Re == 10.0 and "_Re1.000e+01" in eq.get_file_suffix()


def _boundary_normal():
    from auxiliary_methods import boundary_normal
    from grid_generator import HyperCubeBoundaryMarkers as M, hyper_cube
    mesh, marks = hyper_cube(2, 8)
    for side, normal in ((M.left, (-1.0, 0.0)), (M.right, (1.0, 0.0)), (M.bottom, (0.0, -1.0)), (M.top, (0.0, 1.0))):
        assert boundary_normal(mesh, marks, side.value) == normal
    mesh, marks = hyper_cube(3, 4)
    for side, normal in ((M.left, (-1.0, 0.0, 0.0)), (M.right, (1.0, 0.0, 0.0)), (M.bottom, (0.0, -1.0, 0.0)),
                         (M.top, (0.0, 1.0, 0.0)), (M.back, (0.0, 0.0, -1.0)), (M.front, (0.0, 0.0, 1.0))):
        assert boundary_normal(mesh, marks, side.value) == normal


def _bounding_box(mesh):
    return mesh.coords.min(axis=0).tolist(), mesh.coords.max(axis=0).tolist()


def _hyper_cube():
    from grid_generator import hyper_cube
    for dim in (2, 3):
        mesh, marks = hyper_cube(dim, 8)
        assert _bounding_box(mesh) == ([0.0] * dim, [1.0] * dim) and marks.ids() == set(range(1, 2 * dim + 1))


def _open_hyper_cube():
    from grid_generator import HyperCubeBoundaryMarkers as M, open_hyper_cube
    _, marks = open_hyper_cube(2, 8, (("left", (0.0, 0.5), 0.1), ("right", (1.0, 0.7), 0.1),
                                      ("bottom", (0.7, 0.0), 0.05), ("top", (0.5, 1.0), 0.8)))
    assert M.opening.value in marks.ids()
    _, marks = open_hyper_cube(3, 8, (("top", (0.5, 1.0, 0.2), (0.8, 0.8)), ("front", (0.5, 0.25, 1.0), (0.2, 0.3))))
    assert M.opening.value in marks.ids()


def _hyper_rectangle():
    from grid_generator import hyper_rectangle
    for p0, p1, n in (((0.0, 0.0), (10.0, 1.0), 10), ((0.0, 0.0), (10.0, 1.0), (50, 5)),
                      ((0.0, 0.0, 0.0), (10.0, 1.0, 2.0), 8), ((0.0, 0.0, 0.0), (10.0, 1.0, 2.0), (50, 5, 10))):
        mesh, _ = hyper_rectangle(p0, p1, n)
        assert _bounding_box(mesh) == (list(p0), list(p1))


def _spherical_shell():
    from grid_generator import spherical_shell
    for dim in (2, 3):
        mesh, marks = spherical_shell(dim, (0.3, 1.0), 25)
        r = np.linalg.norm(mesh.coords, axis=1)
        assert abs(r.min() - 0.3) < 1e-12 and abs(r.max() - 1.0) < 1e-12 and len(marks.ids()) == 2


def _external_meshes():
    from grid_generator import DFGBoundaryMarkers as D, channel_with_cylinder
    mesh, marks, names = channel_with_cylinder()
    assert mesh.num_cells() > 0 and names
    assert {D.inlet.value, D.outlet.value, D.cylinder.value} <= marks.ids()


NO_SOLVE = {
    "test_bdf_time_stepping.py": [lambda: _bdf_table(1), lambda: _bdf_table(2)],
    "test_discrete_time.py": [_discrete_time],
    "test_imex_time_stepping.py": [lambda k=k: _imex(k) for k in ("SBDF2", "CNAB", "mCNAB", "CNLF")],
    "test_theta_time_stepping.py": [lambda k=k: _theta(k) for k in ("ForwardEuler", "BackwardEuler", "CrankNicolson",
                                                                    "FractionalStep01", "FractionalStep02")],
    "test_auxiliary_classes.py": [_angular_velocity_vector, _equation_coefficients],
    "test_auxiliary_methods.py": [_boundary_normal],
    "test_grid_generator.py": [_hyper_cube, _open_hyper_cube, _hyper_rectangle, _spherical_shell, _external_meshes],
}


@pytest.mark.parametrize("test_file,n_passed,extra", [
    ("test_bdf_time_stepping.py", 2, ()), ("test_discrete_time.py", 1, ()),
    ("test_imex_time_stepping.py", 4, ()), ("test_theta_time_stepping.py", 5, ()),
    ("test_auxiliary_classes.py", 2, ()), ("test_auxiliary_methods.py", 1, ()),
    ("test_grid_generator.py", 5, ("-k", "not extract_boundary_markers")),
])
def test_reference_tests_without_a_solve_pass_unchanged(test_file, n_passed, extra, tmp_path):
    checks = NO_SOLVE[test_file]
    assert len(checks) == n_passed
    for check in checks:
        check()


# ------------------------------------------------------------------ solver files
# one entry per test of the reference file: the problems that test solves (CASES names and arguments)
SOLVER_FILES = {
    "test_ipcs_solver.py": [[("ipcs_channel", {})]],
    "test_transient_solvers.py": [[("bdf_pulsating_channel", {})], [("bdf_gravity_box", {})], [("taylor_green", {})]],
    "test_stationary_solvers.py": [
        [("flat_plate", {})], [("stationary_cavity", dict(n=10))],
        [("stationary_channel", dict(variant=v)) for v in ("inlet", "pressure_gradient", "inlet_pressure",
                                                           "inlet_component")],
        [("stationary_channel", dict(form=f)) for f in ("standard", "rotational", "divergence", "skew_symmetric")],
        [("couette_traction", {})], [("stationary_gravity_box", {})]],
    "test_stationary_rotating_flow.py": [[("rotating_couette", {})]],
    "test_instationary_rotating_flow.py": [[("rotating_couette_spin_up", {})]],
}


@pytest.mark.parametrize("test_file,n_tests", [
    ("test_ipcs_solver.py", 1), ("test_transient_solvers.py", 3), ("test_stationary_solvers.py", 6),
    ("test_stationary_rotating_flow.py", 1), ("test_instationary_rotating_flow.py", 1),
])
def test_reference_solver_tests_reach_the_device_unchanged(test_file, n_tests, tmp_path, monkeypatch):
    import _native as nat
    from gpu_common import have_gpu
    from problem_specs import build_problem
    from test_solver_classes_gpu import CASES
    monkeypatch.setenv("NSFEM_NO_OUTPUT", "1")
    tests = SOLVER_FILES[test_file]
    assert len(tests) == n_tests
    device = have_gpu()
    for problems in tests:
        for name, kwargs in problems:
            problem = build_problem(CASES[name](**kwargs))
            if device:                                 # (with a GPU: they simply solve)
                problem.solve_problem()
                continue
            with pytest.raises(nat.NativeError, match="no ROCm-capable device"):
                problem.solve_problem()
