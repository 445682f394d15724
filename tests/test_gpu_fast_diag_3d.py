"""Fast diagonalisation on 3D box lattices (FastDiag3 in csrc/fastdiag.hip, poisson_fd.factors_3d): the six mode
products against the numpy formula at the edges of the k-loop pipeline; the projection step with precond = 3 against
the LU oracle --
a direct solve where the tensor sum is the stiffness matrix (triple-periodic Taylor-Green box), CG preconditioned by it
where it is not (closed cavity, open-outlet channel); the option poisson_solver = "fast_diagonalization" through the
solver classes; and the refusals."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import _native as nat
import fem_oracle as fo
import poisson_fd as pf
from fem_mesh import FacetMarkers, TaylorHoodDofMap, box_mesh, periodic_entity_map, preferred_p2_order
from gpu_common import rel

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


def _context(mesh, dm):
    return nat.NsfemContext(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, dm.n_p2, dm.n_p1)


def _lattice_context(Nx, Ny, Nz):
    """a context whose P1 space is the Nz x Ny x Nx lattice (box_mesh with Nd - 1 cells per direction)"""
    mesh = box_mesh((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), Nx - 1, Ny - 1, Nz - 1)
    dm = TaylorHoodDofMap(mesh)
    assert dm.n_p1 == Nx * Ny * Nz
    return _context(mesh, dm)


def _random_factors_3d(Nx, Ny, Nz, seed):
    """non-symmetric Vx, Vy, Vz scaled by 1/sqrt(n) (a transposed operand, a swapped mode or a misplaced plane changes
    the result), positive inv"""
    rng = np.random.default_rng(seed)
    f = dict(Vx=rng.standard_normal((Nx, Nx)) / np.sqrt(Nx), Vy=rng.standard_normal((Ny, Ny)) / np.sqrt(Ny),
             Vz=rng.standard_normal((Nz, Nz)) / np.sqrt(Nz), inv=rng.uniform(0.5, 1.5, (Nz, Ny, Nx)), exact=True)
    return f, rng.standard_normal(Nx * Ny * Nz)


def _reference_3d(f, r, dtype):
    """pf.apply_reference_3d's formula evaluated in ``dtype``"""
    g = {k: np.asarray(f[k], dtype=dtype) for k in ("Vx", "Vy", "Vz", "inv")}
    Nz, Ny, Nx = g["inv"].shape
    R = np.asarray(r, dtype=dtype).reshape(Nz, Ny, Nx)
    U = R @ g["Vx"]
    U = np.matmul(g["Vy"].T, U)
    U = (g["Vz"].T @ U.reshape(Nz, Ny * Nx)).reshape(Nz, Ny, Nx) * g["inv"]
    U = (g["Vz"] @ U.reshape(Nz, Ny * Nx)).reshape(Nz, Ny, Nx)
    U = np.matmul(g["Vy"], U)
    return (U @ g["Vx"].T).ravel()


# (Nx, Ny, Nz): each mode's K (= its extent) at one k-block of 96, one block + a tail of 1, several blocks (289 = three
# blocks + 1), 65 and 129; ragged Nx != Ny != Nz throughout, 2 and 3 narrower than one 16-wide wave tile
SHAPES = [(96, 3, 5), (5, 96, 3), (3, 5, 96), (97, 4, 3), (4, 97, 3), (3, 4, 97), (289, 3, 2), (3, 289, 2),
          (2, 3, 289), (65, 129, 7), (129, 7, 65), (7, 65, 129), (65, 33, 17), (17, 65, 33)]


@pytest.mark.parametrize("Nx,Ny,Nz", SHAPES)
def test_mode_products_match_the_reference(Nx, Ny, Nz):
    """FastDiag3::apply (k_fd_gemm for the x and z products, inv fused into the forward z product, k_fd_gemm_batched
    for the y products of every plane) with arbitrary factors against the formula in long double: 1e-13 relative.
    Two applications agree bit for bit; the info call reports the dims, the flag and the applications."""
    ctx = _lattice_context(Nx, Ny, Nz)
    f, r = _random_factors_3d(Nx, Ny, Nz, 7919 * Nx + 131 * Ny + Nz)
    ctx.poisson_set_fast_diag_3d(f)
    z = ctx.mg_apply(2, r)
    ref = _reference_3d(f, r, np.longdouble).astype(np.float64)
    err = rel(z, ref)
    assert err <= 1e-13, (Nx, Ny, Nz, err)
    assert np.array_equal(ctx.mg_apply(2, r), z)
    info = ctx.poisson_fast_diag_3d_info()
    assert info["shape"] == (Nx, Ny, Nz) and info["exact"] and info["applications"] == 2 and info["solves"] == 0
    ctx.close()


def test_true_factors_invert_the_oracle_stiffness_matrix():
    """triple-periodic 32^3 and all-Dirichlet 33 x 25 x 17 lattices: z = T^+ r solves the oracle's stiffness system to
    1e-11 |r| (periodic: mean-free r and residual)"""
    for n, periodic in (((32, 32, 32), True), ((32, 24, 16), False)):
        mesh, dm = _box(n, (1.0, 1.0, 1.0), (0, 1, 2) if periodic else ())
        xs, ys, zs, per = pf.box_lattice(mesh, dm)
        faces = np.zeros(0, np.int64) if periodic else _face_p1_nodes(dm, range(6))
        f = pf.factors_3d(xs, ys, zs, per, faces)
        assert f["exact"] and f["singular"] == periodic
        ctx = _context(mesh, dm)
        ctx.poisson_set_fast_diag_3d(f)
        rng = np.random.default_rng(5)
        r = rng.standard_normal(dm.n_p1)
        if periodic:
            r -= r.mean()
        else:
            r[faces] = 0.0
        z = ctx.mg_apply(2, r)
        A = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap).stiffness_p1()
        res = A @ z - r
        if periodic:
            res -= res.mean()
        else:
            res[faces] = 0.0
        assert np.linalg.norm(res) <= 1e-11 * np.linalg.norm(r), np.linalg.norm(res) / np.linalg.norm(r)
        ctx.close()


# ---------------------------------------------------------------------------------------------------------------------
# the projection step against the LU oracle
# ---------------------------------------------------------------------------------------------------------------------
class _TriplePeriodic:
    def __init__(self, lengths):
        import dlfn_compat as dlfn

        class Domain(dlfn.SubDomain):
            def inside(self, x, on_boundary):
                return bool(on_boundary and any(dlfn.near(x[a], 0.0) for a in range(3)))

            def map(self, x_slave, x_master):
                for a in range(3):
                    if dlfn.near(x_slave[a], lengths[a]):
                        x_master[:] = x_slave
                        x_master[a] -= lengths[a]
                        return
                x_master[:] = -10.0
        self.domain = Domain()


def _box(n, lengths, periodic_axes=()):
    mesh = box_mesh((0.0, 0.0, 0.0), lengths, *n)
    assert periodic_axes in ((), (0, 1, 2))
    pm = periodic_entity_map(mesh, _TriplePeriodic(lengths).domain) if periodic_axes else None
    return mesh, TaylorHoodDofMap(mesh, reorder=preferred_p2_order(3), periodic_map=pm)


def _marks(mesh, lengths):
    marks = FacetMarkers(mesh)
    for axis in range(3):
        marks.mark(lambda X, a=axis: np.abs(X[:, a]) < 1e-12, 2 * axis + 1)
        marks.mark(lambda X, a=axis: np.abs(X[:, a] - lengths[a]) < 1e-12, 2 * axis + 2)
    return marks


def _face_p1_nodes(dm, faces, lengths=(1.0, 1.0, 1.0)):
    X = dm.p1_coords
    d = [np.nonzero(np.abs(X[:, f // 2] - (0.0 if f % 2 == 0 else lengths[f // 2])) < 1e-12)[0] for f in faces]
    return np.unique(np.concatenate(d)).astype(np.int64)


def _velocity_bc(dm, marks, spec):
    """spec: [(marker id, fn(X) -> [n, 3])], later entries win"""
    last = {}
    for mid, fn in spec:
        nodes = np.unique(dm.facet_p2_nodes(marks.facets_with_id(mid)))
        v = np.asarray(fn(dm.p2_coords[nodes]), dtype=np.float64)
        for a in range(3):
            last.update(zip((3 * nodes + a).tolist(), v[:, a].tolist()))
    d = np.array(sorted(last), dtype=np.int64)
    return d, np.array([last[i] for i in d.tolist()])


def _zero(X):
    return np.zeros((X.shape[0], 3))


def _run_against_oracle(mesh, dm, vbc, pbc, nu, k, nsteps, u0=None, p0=None):
    """nsteps IPCS steps with precond = 3 on the device and the LU oracle; -> (Poisson iteration counts, 3D info,
    velocity error, pressure error modulo a constant)"""
    ctx = _context(mesh, dm)
    xs, ys, zs, per = pf.box_lattice(mesh, dm)
    f = pf.factors_3d(xs, ys, zs, per, pbc[0])
    ctx.poisson_set_fast_diag_3d(f)
    s = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
    coef = dict(convective_term=1.0, pressure_term=1.0, viscous_term=nu, body_force_term=None)
    orc = fo.IPCSOracle(s, coef, refactor_every_step=False)
    if u0 is not None:
        orc.set_initial(u0, p0)
        for slot in (nat.U0, nat.U1, nat.U2):
            ctx.set_state(slot, u0)
        for slot in (nat.P, nat.P_OLD):
            ctx.set_state(slot, p0)
    ctx.set_coeffs(1.0, 1.0, nu)
    ctx.set_dirichlet(nat.VELOCITY, *vbc)
    ctx.set_dirichlet(nat.PRESSURE, *pbc)
    opts = ctx.default_step_opts()
    for o in (opts.momentum, opts.correction):
        o.rtol = 1e-13
    opts.poisson.rtol = 1e-12
    opts.poisson.precond = 3
    its = []
    for step in range(nsteps):
        alpha = fo.bdf_alpha(step, 1.0)
        ctx.set_bdf(alpha, k)
        info = ctx.step_ipcs(opts)
        orc.step(alpha, k, vbc, pbc)
        assert info.newton_iterations == orc.newton_its[step]
        its.append(info.krylov_iterations_poisson)
        ctx.advance(0)
        orc.advance()
    eu = rel(ctx.get_state(nat.U1), orc.vel[1])
    pg, po = ctx.get_state(nat.P_OLD), orc.p_old
    ep = rel(pg - pg.mean(), po - po.mean())
    info3 = ctx.poisson_fast_diag_3d_info()
    ctx.close()
    return its, info3, f, eu, ep


def test_projection_step_triple_periodic_taylor_green_is_one_direct_pass():
    """triple-periodic Taylor-Green box (tgv3d in small): exact factors, the projection step is one pass of the direct
    solve (poisson_direct_step); fields equal the LU oracle to 1e-9, the pressure modulo a constant"""
    n = (8, 8, 8)
    mesh, dm = _box(n, (1.0, 1.0, 1.0), (0, 1, 2))
    g = 2.0 * np.pi
    X = dm.p2_coords
    u0 = np.stack([np.cos(g * X[:, 0]) * np.sin(g * X[:, 1]), -np.sin(g * X[:, 0]) * np.cos(g * X[:, 1]),
                   np.zeros(dm.n_p2)], axis=1).ravel()
    Y = dm.p1_coords
    p0 = -0.25 * (np.cos(2 * g * Y[:, 0]) + np.cos(2 * g * Y[:, 1]))
    empty = (np.zeros(0, np.int64), np.zeros(0))
    its, info, f, eu, ep = _run_against_oracle(mesh, dm, empty, empty, 0.01, 0.25 / 8, 3, u0, p0)
    assert f["exact"] and f["singular"] and info["exact"]
    assert its == [1, 1, 1], its
    assert info["solves"] == 3 and info["applications"] == 3
    assert eu < 1e-9 and ep < 1e-9, (eu, ep)


def test_refinement_passes_of_the_direct_step_on_a_box():
    """The same triple-periodic Taylor-Green box with the exact factors and with inv * (1 + DELTA) (constants and
    derivation of test_gpu_fast_diag: uniformly scaled factors leave DELTA^k |r| after pass k, so rtol = 3e-11 with
    atol = 0 takes SIX passes): poisson_direct_step refines with the 3D object -- one pass per step with the exact
    factors, six with the perturbed ones, one solve per step and one application per pass, and the same fields to
    1e-10 (the pressure modulo a constant)."""
    from test_gpu_fast_diag import DELTA, PASSES, RTOL
    mesh, dm = _box((8, 8, 8), (1.0, 1.0, 1.0), (0, 1, 2))
    g = 2.0 * np.pi
    X, Y = dm.p2_coords, dm.p1_coords
    u0 = np.stack([np.cos(g * X[:, 0]) * np.sin(g * X[:, 1]), -np.sin(g * X[:, 0]) * np.cos(g * X[:, 1]),
                   np.zeros(dm.n_p2)], axis=1).ravel()
    p0 = -0.25 * (np.cos(2 * g * Y[:, 0]) + np.cos(2 * g * Y[:, 1]))
    f = pf.factors_3d(*pf.box_lattice(mesh, dm), np.zeros(0, np.int64))
    assert f["exact"] and f["singular"]
    nsteps, fields = 3, {}
    for refine in (False, True):
        ctx = _context(mesh, dm)
        ctx.poisson_set_fast_diag_3d(dict(f, inv=f["inv"] * (1.0 + DELTA)) if refine else f)
        for slot in (nat.U0, nat.U1, nat.U2):
            ctx.set_state(slot, u0)
        for slot in (nat.P, nat.P_OLD):
            ctx.set_state(slot, p0)
        ctx.set_coeffs(1.0, 1.0, 0.01)
        ctx.set_dirichlet(nat.VELOCITY, np.zeros(0, np.int64), np.zeros(0))
        ctx.set_dirichlet(nat.PRESSURE, np.zeros(0, np.int64), np.zeros(0))
        opts = ctx.default_step_opts()
        for o in (opts.momentum, opts.correction):
            o.rtol = 1e-13
        opts.poisson.precond = 3
        opts.poisson.rtol = RTOL
        opts.poisson.atol = 0.0
        passes = []
        for step in range(nsteps):
            ctx.set_bdf(fo.bdf_alpha(step, 1.0), 0.25 / 8)
            passes.append(ctx.step_ipcs(opts).krylov_iterations_poisson)
            ctx.advance(0)
        info = ctx.poisson_fast_diag_3d_info()
        print("refine", refine, "passes", passes, "solves", info["solves"], "applications", info["applications"])
        assert passes == [PASSES if refine else 1] * nsteps, passes
        assert info["solves"] == nsteps and info["applications"] == (PASSES if refine else 1) * nsteps
        fields[refine] = (ctx.get_state(nat.U1), ctx.get_state(nat.P_OLD))
        ctx.close()
    (ua, pa), (ub, pb) = fields[False], fields[True]
    eu, ep = rel(ub, ua), rel(pb - pb.mean(), pa - pa.mean())
    print("velocity", eu, "pressure", ep)
    assert eu < 1e-10 and ep < 1e-10, (eu, ep)


@pytest.mark.parametrize("n", [6, 10])
def test_projection_step_closed_cavity_runs_preconditioned_cg(n):
    """closed lid-driven cavity (all-Neumann pressure, free box edges): inexact factors, CG preconditioned by T^+ at
    rtol 1e-12 within 20 iterations; fields equal the LU oracle"""
    lengths = (1.0, 1.0, 1.0)
    mesh, dm = _box((n, n, n), lengths)
    marks = _marks(mesh, lengths)
    lid = lambda X: np.tile([1.0, 0.0, 0.0], (X.shape[0], 1))
    vbc = _velocity_bc(dm, marks, [(m, _zero) for m in (1, 2, 3, 4, 5)] + [(6, lid)])
    empty = (np.zeros(0, np.int64), np.zeros(0))
    its, info, f, eu, ep = _run_against_oracle(mesh, dm, vbc, empty, 0.02, 0.05, 2)
    assert not f["exact"] and not info["exact"] and info["solves"] == 2
    assert max(its) <= 20, its
    assert eu < 1e-9 and ep < 1e-9, (eu, ep)


def test_projection_step_open_outlet_channel_iterations_do_not_grow():
    """channel 2 x 1 x 1 with a parabolic inflow, no-slip walls and a pressure outlet (Dirichlet on x = 2 only):
    inexact factors, CG preconditioned by T^+ at two sizes, at most 20 iterations (the host bound predicts ~13) and
    not more at the finer size; fields equal the LU oracle"""
    lengths = (2.0, 1.0, 1.0)
    inflow = lambda X: np.stack([16.0 * X[:, 1] * (1.0 - X[:, 1]) * X[:, 2] * (1.0 - X[:, 2]),
                                 np.zeros(X.shape[0]), np.zeros(X.shape[0])], axis=1)
    counts = []
    for n in ((8, 4, 4), (16, 8, 8)):
        mesh, dm = _box(n, lengths)
        marks = _marks(mesh, lengths)
        vbc = _velocity_bc(dm, marks, [(m, _zero) for m in (3, 4, 5, 6)] + [(1, inflow)])
        pd = _face_p1_nodes(dm, [1], lengths)
        its, info, f, eu, ep = _run_against_oracle(mesh, dm, vbc, (pd, np.zeros(pd.size)), 0.05, 0.02, 2)
        assert not f["exact"] and not f["singular"] and info["solves"] == 2
        assert max(its) <= 20, its
        assert eu < 1e-9 and ep < 1e-9, (n, eu, ep)
        counts.append(max(its))
    assert counts[1] <= counts[0] + 1, counts


# ---------------------------------------------------------------------------------------------------------------------
# the option through the solver classes
# ---------------------------------------------------------------------------------------------------------------------
def _surface_run(spec, poisson_solver):
    from problem_specs import build_problem
    problem = build_problem(spec)
    problem.solver_settings = dict(poisson_solver=poisson_solver)
    problem.solve_problem()
    solver = problem._get_solver()
    velocity, pressure = solver.solution.split()
    return solver, velocity.vector().copy(), pressure.vector().copy()


SURFACE = {
    "cavity_3d": lambda: dict(
        name="Cavity3D", mesh=("cube", 3, 6), scheme="ipcs", numbers=dict(Re=50.0), clock=dict(dt=0.05, steps=3),
        output=0, start={"velocity": (0.0, 0.0, 0.0), "pressure": 0.0},
        bcs=[("no_slip", s) for s in ("left", "right", "bottom", "top", "back")] +
        [("velocity", "front", (1.0, 0.0, 0.0))]),
    "channel_3d": lambda: dict(
        name="ChannelFlow3D", mesh=("rectangle", (0.0, 0.0, 0.0), (2.0, 1.0, 1.0), (8, 4, 4)), scheme="ipcs",
        numbers=dict(Re=20.0), clock=dict(dt=0.02, steps=3), output=0,
        start={"velocity": (0.0, 0.0, 0.0), "pressure": 0.0},
        bcs=[("pressure", "right", 0.0)] +
        [("velocity_function", "left", _inflow_expr())] +
        [("no_slip", s) for s in ("bottom", "top", "back", "front")]),
    "taylor_green_3d": lambda: dict(
        name="TaylorGreenVortex3D", mesh=("cube", 3, 8), scheme="ipcs", numbers=dict(Re=100.0),
        clock=dict(dt=0.05, steps=3, t1=1.0), output=0,
        start={"velocity": _tg_expr(("cos(gamma*x[0])*sin(gamma*x[1])", "-sin(gamma*x[0])*cos(gamma*x[1])", "0.0")),
               "pressure": _tg_expr("-0.25*(cos(2.0*gamma*x[0])+cos(2.0*gamma*x[1]))")},
        bcs=[("pressure_mean", None, 0.0)],
        periodic=((0, 1, 2), ("left", "right", "top", "bottom", "back", "front"))),
}


def _inflow_expr():
    from problem_specs import expr
    return expr(("16.0*x[1]*(1.0-x[1])*x[2]*(1.0-x[2])", "0.0", "0.0"))


def _tg_expr(code):
    from problem_specs import expr
    return expr(code, 3, gamma=2.0 * np.pi)


@pytest.mark.parametrize("case,exact", [("cavity_3d", False), ("channel_3d", False), ("taylor_green_3d", True)])
def test_poisson_solver_option_uses_the_3d_solve_through_the_solver_classes(case, exact):
    """poisson_solver = "fast_diagonalization" on a 3D box lattice ships the 3D factors and runs the projection steps
    with them (before the 3D branch, the option silently ran multigrid-CG); the fields equal the multigrid run's to the
    Krylov tolerance"""
    solver, u_fd, p_fd = _surface_run(SURFACE[case](), "fast_diagonalization")
    info = solver._ctx.poisson_fast_diag_3d_info()
    assert solver._fast_diagonalization_ready()
    assert info["solves"] == 3 and info["applications"] > 0 and info["exact"] == exact
    assert info["shape"][0] * info["shape"][1] * info["shape"][2] == solver._dofmap.n_p1
    solver_mg, u_mg, p_mg = _surface_run(SURFACE[case](), "multigrid")
    assert solver_mg._ctx.poisson_fast_diag_3d_info()["solves"] == 0
    assert rel(u_fd, u_mg) < 1e-9, rel(u_fd, u_mg)
    assert rel(p_fd - p_fd.mean(), p_mg - p_mg.mean()) < 1e-8


# ---------------------------------------------------------------------------------------------------------------------
# refusals
# ---------------------------------------------------------------------------------------------------------------------
def test_wrong_dims_and_missing_factors_are_refused():
    ctx = _lattice_context(4, 3, 5)
    f, r = _random_factors_3d(4, 3, 5, 1)
    g, _ = _random_factors_3d(4, 3, 4, 1)
    with pytest.raises(nat.NativeError, match="number of pressure dofs"):
        ctx.poisson_set_fast_diag_3d(g)
    assert ctx.poisson_fast_diag_3d_info()["shape"] == (0, 0, 0)
    # precond = 3 with no factors set: refused, not replaced by another solver
    mesh, dm = _box((3, 3, 3), (1.0, 1.0, 1.0))
    ctx2 = _context(mesh, dm)
    ctx2.set_coeffs(1.0, 1.0, 0.02)
    ctx2.set_dirichlet(nat.VELOCITY, *_velocity_bc(dm, _marks(mesh, (1.0,) * 3), [(m, _zero) for m in range(1, 7)]))
    ctx2.set_dirichlet(nat.PRESSURE, np.zeros(0, np.int32), np.zeros(0))
    opts = ctx2.default_step_opts()
    opts.poisson.precond = 3
    ctx2.set_bdf((1.0, -1.0, 0.0), 0.05)
    with pytest.raises(nat.NativeError, match="no factors were set"):
        ctx2.step_ipcs(opts)
    ctx2.close()
    ctx.poisson_set_fast_diag_3d(f)
    assert ctx.poisson_fast_diag_3d_info()["shape"] == (4, 3, 5)
    ctx.close()


def test_partitioned_context_is_refused():
    from test_gpu_fast_diag import _strip_contexts
    group = nat.local_group_create(2)
    strips = _strip_contexts(8, [4, 4], group)
    try:
        for ctx, _ in strips:
            n = ctx.n_p1
            assert n % 9 == 0
            f, _ = _random_factors_3d(3, 3, n // 9, 2)
            with pytest.raises(nat.NativeError, match="partitioned"):
                ctx.poisson_set_fast_diag_3d(f)
    finally:
        for ctx, _ in strips:
            ctx.close()
        nat.local_group_destroy(group)


# ---------------------------------------------------------------------------------------------------------------------
# replacing factors: the factors set last are the ones used, also by CG iteration bodies replayed from captured graphs
# ---------------------------------------------------------------------------------------------------------------------
def test_the_factors_set_last_are_the_ones_applied():
    """3D factors, then 2D factors of the same pressure space (W x H = Nx Ny Nz), then 3D factors again: the test hook
    applies the 2D solve while the 2D factors are the last ones set (the 3D info then reports none) and the 3D solve
    after that"""
    Nx, Ny, Nz = 4, 3, 5
    ctx = _lattice_context(Nx, Ny, Nz)
    f, r = _random_factors_3d(Nx, Ny, Nz, 11)
    rng = np.random.default_rng(12)
    W, H = Nx * Ny, Nz
    g = dict(Vx=rng.standard_normal((W, W)) / np.sqrt(W), Vy=rng.standard_normal((H, H)) / np.sqrt(H),
             inv=rng.uniform(0.5, 1.5, (H, W)))
    ref3 = _reference_3d(f, r, np.longdouble).astype(np.float64)
    ctx.poisson_set_fast_diag_3d(f)
    assert rel(ctx.mg_apply(2, r), ref3) <= 1e-13
    ctx.poisson_set_fast_diag(g)
    assert ctx.poisson_fast_diag_3d_info()["shape"] == (0, 0, 0)
    assert rel(ctx.mg_apply(2, r), pf.apply_reference(g, r)) <= 1e-13
    ctx.poisson_set_fast_diag_3d(f)
    assert ctx.poisson_fast_diag_3d_info()["shape"] == (Nx, Ny, Nz)
    assert rel(ctx.mg_apply(2, r), ref3) <= 1e-13
    ctx.close()


_RESEND_UNDER_GRAPHS = r"""
import json, sys
import numpy as np
import _native as nat
import poisson_fd as pf
from fem_mesh import FacetMarkers, TaylorHoodDofMap, box_mesh

n = 6
mesh = box_mesh((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), n, n, n)
dm = TaylorHoodDofMap(mesh)
marks = FacetMarkers(mesh)
for axis in range(3):
    marks.mark(lambda X, a=axis: np.abs(X[:, a]) < 1e-12, 2 * axis + 1)
    marks.mark(lambda X, a=axis: np.abs(X[:, a] - 1.0) < 1e-12, 2 * axis + 2)
last = {}
for mid in range(1, 7):
    nodes = np.unique(dm.facet_p2_nodes(marks.facets_with_id(mid)))
    for a in range(3):
        last.update(zip((3 * nodes + a).tolist(), [1.0 if (mid == 6 and a == 0) else 0.0] * nodes.size))
vd = np.array(sorted(last), dtype=np.int64)
vv = np.array([last[i] for i in vd.tolist()])
f = pf.factors_3d(*pf.box_lattice(mesh, dm), dirichlet_nodes=np.zeros(0, np.int64))
assert not f["exact"]
W, H = 49, 7
assert W * H == dm.n_p1
rng = np.random.default_rng(1)
g = dict(Vx=rng.standard_normal((W, W)), Vy=rng.standard_normal((H, H)), inv=rng.uniform(0.5, 1.5, (H, W)))


def run(resend):
    ctx = nat.NsfemContext(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, dm.n_p2, dm.n_p1)
    ctx.set_coeffs(1.0, 1.0, 0.02)
    ctx.set_dirichlet(nat.VELOCITY, vd, vv)
    ctx.set_dirichlet(nat.PRESSURE, np.zeros(0, np.int64), np.zeros(0))
    ctx.poisson_set_fast_diag_3d(f)
    o = ctx.default_step_opts()
    for k in (o.momentum, o.poisson, o.correction):
        k.rtol = 1e-12
    o.poisson.precond = 3
    its = []
    for step in range(4):
        if resend and step == 2:        # other factors in between: the 3D buffers are freed and allocated anew
            ctx.poisson_set_fast_diag(g)
            ctx.poisson_set_fast_diag_3d(f)
        elif resend and step == 3:      # the same factors again (buffers of an unchanged size are kept)
            ctx.poisson_set_fast_diag_3d(f)
        ctx.set_bdf((1.0, -1.0, 0.0) if step == 0 else (1.5, -2.0, 0.5), 0.05)
        its.append(ctx.step_ipcs(o).krylov_iterations_poisson)
        ctx.advance(0)
    u, p = ctx.get_state(nat.U1), ctx.get_state(nat.P_OLD)
    solves = ctx.poisson_fast_diag_3d_info()["solves"]
    ctx.close()
    return u, p, its, solves


u0, p0, its0, s0 = run(False)
u1, p1, its1, s1 = run(True)
print(json.dumps(dict(du=float(np.linalg.norm(u1 - u0) / np.linalg.norm(u0)),
                      dp=float(np.linalg.norm((p1 - p1.mean()) - (p0 - p0.mean())) / np.linalg.norm(p0 - p0.mean())),
                      its0=its0, its1=its1, solves=[s0, s1])))
"""


def test_factors_sent_again_between_graph_replayed_steps():
    """With the CG iteration bodies captured into graphs (NSFEM_GRAPHS=1, a child process: the switch is read once),
    closed cavity with inexact factors (FastDiag3 is the captured preconditioner): sending other factors and then the
    3D factors again between two steps, and the same factors once more before the next, changes nothing -- the fields
    and iteration counts equal those of a run without the re-sends.  (Each setter bumps the context's graph epoch, so
    no graph recorded with the addresses of released buffers is replayed.)"""
    env = dict(os.environ)
    env["NSFEM_GRAPHS"] = "1"
    env["PYTHONPATH"] = os.pathsep.join([os.path.join(ROOT, "navierstokes-with-fenics_amd"), os.path.join(ROOT, "oracle"),
                                         env.get("PYTHONPATH", "")])
    res = subprocess.run([sys.executable, "-c", _RESEND_UNDER_GRAPHS], capture_output=True, text=True, timeout=600,
                         env=env)
    assert res.returncode == 0, res.stderr[-3000:]
    out = json.loads(res.stdout.strip().splitlines()[-1])
    assert out["its0"] == out["its1"] and max(out["its0"]) <= 20, out
    assert out["solves"] == [4, 4], out
    assert out["du"] < 1e-12 and out["dp"] < 1e-12, out
