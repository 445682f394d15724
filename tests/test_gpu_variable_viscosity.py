"""Variable viscosity in the IMEX step on the GPU (nsfem_set_viscosity_law / nsfem_viscosity_residual /
nsfem_viscosity_cells / nsfem_viscosity_info, IMEXIPCSSolver.set_viscosity_model) against the numpy restatement of
tests/test_variable_viscosity_host.py.

Tolerances.  Smagorinsky kernel: 1e-13 relative to max |V|, the project's figure for element kernels against the oracle.
Carreau kernel: the law calls pow; the largest difference measured over the meshes below is 3.95e-15 of max |V|
(box(16, 16); DESIGN.md 4j -- the Smagorinsky kernel shows 3.75e-15 there, so this is the rounding of the sums, not
of pow), asserted ten times that, 3.95e-14 (library roundings differ between compilers), below the cap of 1e-11.  Steps: those of tests/test_gpu_imex.py for the same step count and Krylov settings (rtol 1e-13) -- u*, u
1e-9 and p minus its mean 1e-8, relative.

Meshes.  box(4, 4), box(3, 5), box(8, 8): one partly filled block of cells; box(16, 16): two blocks, and the smallest
lattice on which the one-launch right-hand side runs.  The mapped mesh is box(8, 8) whose vertices went through a
smooth non-linear map (the boundary stays) before the dof map was built: cells of different size and shape, Delta_K
varies.  3D: the Kuhn boxes of tests/test_gpu_3d.py, (3, 2, 2) on 1 x 0.8 x 0.6 and (4, 4, 4) (more than one block),
and the general tetrahedra of tests/general_tet_mesh.py at the same two sizes (72 and 384 cells): cells of both
orientations, Delta_K varies by a factor of 1.5 and more, no entry of any J^-1 is zero.  Periodic dof maps: the six
fixtures of tests/periodic_meshes.py (channels, the square and the cube without a wall, two mapped channels) with the
periodic fields of that module; n_p1 is below the vertex count there and the seam cells read coordinates a period away
from those of their dofs."""
import os

import numpy as np
import pytest

import _native as nat
import fem_oracle as fo
from fem_mesh import FacetMarkers, Mesh, TaylorHoodDofMap, rectangle_mesh
from general_tet_mesh import CUBE, SMALL, general_tets, shear_bc
from gpu_common import box, cavity_bc, context, rel
from imex_time_stepping import IMEXTimeStepping, IMEXType
from periodic_meshes import ALL as PERIODIC
from periodic_meshes import is_periodic, lengths_of, periodic_axes, periodic_fields, periodic_fixture, wall_bc
from test_gpu_3d import box3, context3, lid_bc
from test_scalar_transport_host import smooth_fields
from test_variable_viscosity_host import (CARREAU, SMAGORINSKY, IMEXViscRestatement, VariableViscosityRestatement,
                                          rule_space)

pytestmark = pytest.mark.gpu

TYPES = (IMEXType.SBDF2, IMEXType.CNAB, IMEXType.mCNAB, IMEXType.CNLF)
NO_PBC = (np.zeros(0, np.int32), np.zeros(0))
_LAWS = {SMAGORINSKY: (0.9, ), CARREAU: (0.07, 1.7, 0.6)}
_KERNEL_TOL = {SMAGORINSKY: 1e-13, CARREAU: 3.95e-14}
_COEF = dict(convective_term=1.0, pressure_term=1.0, viscous_term=0.01, body_force_term=1.0)
# Smagorinsky constant of the step tests: on the 8 x 8 cavity nu_x reaches 0.7 c_v (c_v = 0.01) under the lid
_CS_STEPS = 0.2


def _mapped_box(n=8):
    """box(n, n) with the vertices moved by a smooth map that keeps the boundary; markers as gpu_common.box"""
    m0 = rectangle_mesh((0.0, 0.0), (1.0, 1.0), n, n)
    x, y = m0.coords[:, 0], m0.coords[:, 1]
    bump = np.sin(np.pi * x) * np.sin(np.pi * y)
    coords = np.stack([x + 0.07 * bump * (1.0 + 0.5 * y), y - 0.05 * bump * np.cos(1.3 * x)], axis=1)
    mesh = Mesh(coords, m0.cells)
    dm = TaylorHoodDofMap(mesh)
    marks = FacetMarkers(mesh)
    marks.mark(lambda X: np.abs(X[:, 0]) < 1e-12, 1)
    marks.mark(lambda X: np.abs(X[:, 0] - 1.0) < 1e-12, 2)
    marks.mark(lambda X: np.abs(X[:, 1]) < 1e-12, 3)
    marks.mark(lambda X: np.abs(X[:, 1] - 1.0) < 1e-12, 4)
    return mesh, dm, marks


_CACHE = {}


def _mesh(kind):
    """(mesh, dm, marks, oracle space, rule space, context factory) of a 2D box (nx, ny), "mapped", a 3D Kuhn box
    ((nx, ny, nz), lengths), the general tetrahedra ((nx, ny, nz), lengths, "general") or a periodic fixture by its
    name; built once per kind and left unchanged"""
    if kind not in _CACHE:
        if is_periodic(kind):
            mesh, dm, marks = periodic_fixture(kind)
            make = context if mesh._dim == 2 else context3
        elif kind == "mapped":
            mesh, dm, marks = _mapped_box()
            make = context
        elif isinstance(kind[0], int):
            mesh, dm, marks = box(*kind)
            make = context
        elif len(kind) == 3:
            assert kind[2] == "general"
            mesh, dm, marks = general_tets(kind[0], kind[1])
            make = context3
        else:
            mesh, dm, marks = box3(*kind)
            make = context3
        args = (mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap)
        _CACHE[kind] = (mesh, dm, marks, fo.Space(*args), rule_space(*args), make)
    return _CACHE[kind]


GENERAL72, GENERAL384 = SMALL + ("general", ), CUBE + ("general", )


def is_general(kind):
    return isinstance(kind, tuple) and len(kind) == 3 and kind[2] == "general"


_KERNEL_MESHES = [(4, 4), (3, 5), (8, 8), (16, 16), "mapped", ((3, 2, 2), (1.0, 0.8, 0.6)), ((4, 4, 4), (1.0, 1.0, 1.0)),
                  GENERAL72, GENERAL384] + list(PERIODIC)


def velocity_on(kind, dm):
    """the smooth non-polynomial velocity of the kernel tests; on a periodic fixture a periodic one"""
    if is_periodic(kind):
        return periodic_fields(dm.p2_coords, lengths_of(kind), periodic_axes(kind))[0]
    return smooth_fields(dm.p2_coords)[0]


def _max_rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


# ---------------------------------------------------------------- 1. the kernels against the restatement
@pytest.mark.parametrize("law", (SMAGORINSKY, CARREAU))
@pytest.mark.parametrize("kind", _KERNEL_MESHES, ids=str)
def test_viscosity_kernel_matches_the_restatement(kind, law):
    """weight * V(u) and the cell means of nu_x for the smooth non-polynomial velocity; a second call returns the same
    bytes, the weight rides in the kernel, no stored state is touched, bad slots raise"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    u = velocity_on(kind, dm)
    orc = VariableViscosityRestatement(rs, law, _LAWS[law])
    want, means = orc.residual(u), orc.cell_means(u)
    if is_periodic(kind):
        assert dm.n_p1 < mesh.num_vertices()
    if kind == "mapped" or is_general(kind) or (is_periodic(kind) and kind.endswith("mapped")):
        assert orc.delta.max() > 1.2 * orc.delta.min()
    ctx = make(mesh, dm)
    try:
        ctx.set_state(nat.U1, u)
        ctx.set_viscosity_law(law, _LAWS[law])
        got = ctx.viscosity_residual(nat.U1, 1.0)
        err = _max_rel(got, want)
        cells = ctx.viscosity_cells(nat.U1)
        cerr = _max_rel(cells, means)
        print("kernel %s law %d: V %.2e cell means %.2e (of the largest entry)" % (kind, law, err, cerr))
        assert np.abs(want).max() > 1e-4 and np.abs(means).max() > 1e-4
        assert err < _KERNEL_TOL[law] and cerr < _KERNEL_TOL[law]
        assert got.tobytes() == ctx.viscosity_residual(nat.U1, 1.0).tobytes()
        assert cells.tobytes() == ctx.viscosity_cells(nat.U1).tobytes()
        ctx.set_state(nat.USTAR, u)
        assert _max_rel(ctx.viscosity_residual(nat.USTAR, -1.5), -1.5 * want) < _KERNEL_TOL[law]
        assert not ctx.get_state(nat.CONV_N1).any() and not ctx.get_state(nat.CONV_N2).any()
        assert np.array_equal(ctx.get_state(nat.U1), u)
        info = ctx.viscosity_info()
        assert info["law"] == law and info["element_launches"] == 5 and info["recomputed"] == 0
        for slot in (nat.P, nat.CONV_N1, nat.BODY_FORCE):
            with pytest.raises(nat.NativeError, match="slot"):
                ctx.viscosity_residual(slot, 1.0)
            with pytest.raises(nat.NativeError, match="slot"):
                ctx.viscosity_cells(slot)
    finally:
        ctx.close()


def test_bad_laws_and_parameters_raise():
    mesh, dm, marks, s, rs, make = _mesh((4, 4))
    ctx = make(mesh, dm)
    try:
        with pytest.raises(nat.NativeError, match="no law"):
            ctx.viscosity_residual(nat.U1, 1.0)
        for law in (-1, 3, 7):
            with pytest.raises(nat.NativeError, match="unknown law"):
                ctx.set_viscosity_law(law, (0.1, ))
        for bad in ((-0.1, ), (np.nan, ), (np.inf, )):
            with pytest.raises(nat.NativeError, match="C_s"):
                ctx.set_viscosity_law(SMAGORINSKY, bad)
        for bad, word in (((np.nan, 1.0, 0.5), "a ="), ((np.inf, 1.0, 0.5), "a ="), ((0.1, -1.0, 0.5), "lambda"),
                          ((0.1, np.inf, 0.5), "lambda"), ((0.1, 1.0, 0.0), "n must"), ((0.1, 1.0, -1.0), "n must"),
                          ((0.1, 1.0, np.nan), "n must")):
            with pytest.raises(nat.NativeError, match=word):
                ctx.set_viscosity_law(CARREAU, bad)
        assert ctx.viscosity_info() == dict(law=0, element_launches=0, recomputed=0)
        ctx.set_viscosity_law(CARREAU, (-0.3, 0.0, 2.5))          # negative a, lambda = 0, n > 1 are all allowed
        ctx.set_viscosity_law(0)
        assert ctx.viscosity_info()["law"] == 0
    finally:
        ctx.close()


# ---------------------------------------------------------------- 2. steps against the restatement
def _setup(ctx, dm, marks, s, rs, law, params, form="standard", general=False, periodic=None, amp=1.0):
    """coefficients, cavity / lid boundary values and the body force of test_gpu_scalar_transport._drive; ``general``:
    the solenoidal shear of general_tet_mesh.shear_bc on every face (a lid on an oblique face has a net flux);
    ``periodic``: the name of a periodic fixture -- no-slip on its walls, a periodic body force, and a periodic velocity
    at both old levels, ``amp`` times that of tests/periodic_meshes.py (there is no lid to set the fluid in motion)"""
    X = dm.p2_coords
    dim = X.shape[1]
    if periodic:
        vbc = wall_bc(periodic)
        u = amp * periodic_fields(X, lengths_of(periodic), periodic_axes(periodic))[0]
        f = 0.6 * np.roll(u.reshape(-1, dim), 1, axis=1).ravel()
        u[vbc[0]] = 0.0
    else:
        vbc = cavity_bc(dm, marks) if dim == 2 else (shear_bc if general else lid_bc)(dm, marks)
        f = np.stack([np.sin(np.pi * X[:, 1]), -1.0 + X[:, 0], 0.5 * X[:, 1]][:dim], axis=1).ravel()
    visc = VariableViscosityRestatement(rs, law, params) if law else None
    orc = IMEXViscRestatement(s, _COEF, form, visc=visc)
    orc.body_force = f
    ctx.set_coeffs(1.0, 1.0, 0.01, 1.0)
    ctx.set_dirichlet(nat.VELOCITY, *vbc)
    ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
    ctx.set_state(nat.BODY_FORCE, f)
    if law is not None:
        ctx.set_viscosity_law(law, params)
    if periodic:
        for lvl, slot, scale in ((1, nat.U1, 1.0), (2, nat.U2, 0.9)):
            orc.vel[lvl] = scale * u
            ctx.set_state(slot, scale * u)
    return orc, vbc


def _opts(ctx, form_id=0):
    opts = ctx.default_step_opts()
    opts.convective_form = form_id
    for ko in (opts.momentum, opts.poisson, opts.correction):
        ko.rtol = 1e-13
    return opts


def _solve(ctx, orc, ts, vbc, opts, tag=""):
    """one step of the device and of the restatement, compared; not yet advanced"""
    ts.update_coefficients()
    kk = ts.get_next_step_size()
    ctx.set_imex(ts.alpha, ts.beta, ts.gamma, kk)
    ctx.step_imex(opts)
    orc.step(ts.alpha, ts.beta, ts.gamma, kk, vbc, NO_PBC)
    us, u, p = ctx.get_state(nat.USTAR), ctx.get_state(nat.U0), ctx.get_state(nat.P)
    es, eu = rel(us, orc.ustar), rel(u, orc.vel[0])
    ep = rel(p - p.mean(), orc.p - orc.p.mean())
    print("%s step %d k %.4g: u* %.2e u %.2e p %.2e path %s" % (tag, ts.step_number, kk, es, eu, ep,
                                                                ctx.imex_info()["path"]))
    assert es < 1e-9 and eu < 1e-9 and ep < 1e-8, (tag, es, eu, ep)


def _advance(ctx, orc, ts):
    ctx.advance(0)
    orc.advance()
    ts.advance_time()


def _step(ctx, orc, ts, vbc, opts, tag=""):
    _solve(ctx, orc, ts, vbc, opts, tag)
    _advance(ctx, orc, ts)


def _run(kind, typ, law, params, steps=4, k=None):
    mesh, dm, marks, s, rs, make = _mesh(kind)
    ctx = make(mesh, dm)
    try:
        orc, vbc = _setup(ctx, dm, marks, s, rs, law, params, general=is_general(kind),
                          periodic=kind if is_periodic(kind) else None)
        n = 16 if is_periodic(kind) else kind[0] if isinstance(kind[0], int) else (8 if kind == "mapped" else kind[0][0])
        ts = IMEXTimeStepping(0.0, 1.0e9, typ, desired_start_time_step=k or 0.5 / n)
        opts = _opts(ctx)
        for _ in range(steps):
            _step(ctx, orc, ts, vbc, opts, "%s %s law %s" % (kind, typ.name, law))
        return orc, ctx.imex_info(), ctx.viscosity_info()
    finally:
        ctx.close()


@pytest.fixture(scope="module")
def newtonian_ustar():
    """u* of the restatement WITHOUT the term after the 4 SBDF2 steps of the box(8, 8) test (host only)"""
    mesh, dm, marks, s, rs, make = _mesh((8, 8))
    X = dm.p2_coords
    orc = IMEXViscRestatement(s, _COEF, "standard", visc=None)
    orc.body_force = np.stack([np.sin(np.pi * X[:, 1]), -1.0 + X[:, 0]], axis=1).ravel()
    vbc = cavity_bc(dm, marks)
    ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=0.5 / 8)
    for _ in range(4):
        ts.update_coefficients()
        orc.step(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size(), vbc, NO_PBC)
        last = orc.ustar.copy()
        orc.advance()
        ts.advance_time()
    return last


@pytest.mark.parametrize("typ", TYPES, ids=lambda t: t.name)
def test_steps_with_smagorinsky_match_the_restatement(typ, newtonian_ustar):
    """lid-driven cavity on box(8, 8) (generic right-hand-side path), 4 steps of every IMEXType, C_s = 0.2"""
    orc, info, vinfo = _run((8, 8), typ, SMAGORINSKY, (_CS_STEPS, ))
    assert info["path"] == "generic" and info["generic_rhs"] == 4, info
    # one element launch per step for V(u1); V(u2) is in what the step before stored (first step and CNLF: beta1 = 0,
    # no old vector is read)
    assert vinfo["law"] == SMAGORINSKY and vinfo["element_launches"] == 4 and vinfo["recomputed"] == 0, vinfo
    if typ is IMEXType.SBDF2:
        change = rel(orc.ustar, newtonian_ustar)
        print("effect of V on u* after 4 steps: %.2e" % change)
        assert change > 1e-3


@pytest.mark.parametrize("kind,law,params,path", [
    ((16, 16), SMAGORINSKY, (_CS_STEPS, ), "lattice-kernel"), ("mapped", SMAGORINSKY, (_CS_STEPS, ), "generic"),
    (((3, 2, 2), (1.0, 0.8, 0.6)), SMAGORINSKY, (_CS_STEPS, ), "generic"),
    (((3, 2, 2), (1.0, 0.8, 0.6)), CARREAU, (0.008, 1.0, 0.5), "generic"),
    (GENERAL72, SMAGORINSKY, (_CS_STEPS, ), "generic"), (GENERAL72, CARREAU, (0.008, 1.0, 0.5), "generic"),
    ((8, 8), CARREAU, (0.008, 1.0, 0.5), "generic"),
    ("pchan2", SMAGORINSKY, (_CS_STEPS, ), "generic"), ("pchan2", CARREAU, (0.008, 1.0, 0.5), "generic"),
    ("pchan3", SMAGORINSKY, (_CS_STEPS, ), "generic"), ("pchan3", CARREAU, (0.008, 1.0, 0.5), "generic")], ids=str)
def test_sbdf2_steps_on_the_other_meshes_and_the_carreau_law(kind, law, params, path):
    """SBDF2, 4 steps: box(16, 16) runs the one-launch lattice right-hand side and the two extra launches after it;
    the mapped mesh has a varying Delta_K; the Kuhn box and the general tetrahedra run the 3D kernel inside the steps; the
    Carreau law (zero
    shear viscosity c_v = 0.01, nu_inf = 0.002) in both dimensions; the periodic channels, no-slip on their walls, from a
    periodic velocity under a periodic body force"""
    orc, info, vinfo = _run(kind, IMEXType.SBDF2, law, params)
    assert info["path"] == path, info
    if path == "lattice-kernel":
        assert info["lattice_rhs"] == 4 and info["generic_rhs"] == 0
    assert vinfo["element_launches"] == 4 and vinfo["recomputed"] == 0, vinfo


# ---------------------------------------------------------------- 3. the stored vector
def test_stored_vector_is_reused_and_recomputed_when_it_must_be():
    """SBDF2 on box(8, 8).  The stored N = c_c conv + V is reused from step 2 on (the recompute counter stands still),
    a step-size change keeps it; setting U1 by hand, changing the convective form, changing C_s and switching the law
    each make the next step recompute N(u2) -- which then matches the restatement again"""
    mesh, dm, marks, s, rs, make = _mesh((8, 8))
    ctx = make(mesh, dm)
    try:
        orc, vbc = _setup(ctx, dm, marks, s, rs, SMAGORINSKY, (_CS_STEPS, ))
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=1.0 / 16.0)
        opts = _opts(ctx)
        for _ in range(3):
            _step(ctx, orc, ts, vbc, opts, "reuse")
        assert ctx.viscosity_info() == dict(law=SMAGORINSKY, element_launches=3, recomputed=0)
        # a step-size change keeps the stored vector
        ts.set_desired_next_step_size(1.0 / 32.0)
        _step(ctx, orc, ts, vbc, opts, "step size")
        assert ctx.viscosity_info()["recomputed"] == 0
        # U1 set by hand after a step, before the advance: the N1 just stored no longer belongs to the level that
        # becomes u2, so the next step evaluates N(u2) afresh
        _solve(ctx, orc, ts, vbc, opts, "before u1 by hand")
        u1 = ctx.get_state(nat.U1) * 0.98
        ctx.set_state(nat.U1, u1)
        orc.vel[1], orc.N1 = u1.copy(), None
        _advance(ctx, orc, ts)
        assert orc.N2 is None and ctx.viscosity_info()["recomputed"] == 0
        _step(ctx, orc, ts, vbc, opts, "u1 by hand")
        assert ctx.viscosity_info()["recomputed"] == 1
        # the convective form changes
        orc.form, orc.N2 = "skew_symmetric", None
        _step(ctx, orc, ts, vbc, _opts(ctx, 3), "form")
        assert ctx.viscosity_info()["recomputed"] == 2
        # C_s changes
        ctx.set_viscosity_law(SMAGORINSKY, (0.5 * _CS_STEPS, ))
        orc.visc, orc.N2 = VariableViscosityRestatement(rs, SMAGORINSKY, (0.5 * _CS_STEPS, )), None
        _step(ctx, orc, ts, vbc, _opts(ctx, 3), "C_s")
        assert ctx.viscosity_info()["recomputed"] == 3
        # the same parameters again: nothing changed, nothing recomputed
        ctx.set_viscosity_law(SMAGORINSKY, (0.5 * _CS_STEPS, ))
        _step(ctx, orc, ts, vbc, _opts(ctx, 3), "same law")
        assert ctx.viscosity_info()["recomputed"] == 3
        # the law is switched
        ctx.set_viscosity_law(CARREAU, (0.008, 1.0, 0.5))
        orc.visc, orc.N2 = VariableViscosityRestatement(rs, CARREAU, (0.008, 1.0, 0.5)), None
        _step(ctx, orc, ts, vbc, _opts(ctx, 3), "law")
        info = ctx.viscosity_info()
        assert info["law"] == CARREAU and info["recomputed"] == 4
        # 10 steps with one launch each, 4 recomputations of N(u2)
        assert info["element_launches"] == 10 + 4, info
    finally:
        ctx.close()


# ---------------------------------------------------------------- 4. law 0
def test_law_zero_leaves_the_step_bit_identical():
    """after set_viscosity_law(0) -- following a law that was set and never used in a step -- and on a context that
    never called it, 3 steps give the same bytes as a context that knows nothing of the feature's calls; no element
    kernel is launched"""
    mesh, dm, marks, s, rs, make = _mesh((8, 8))
    out = []
    for mode in ("never", "zero", "set then zero"):
        ctx = make(mesh, dm)
        try:
            _setup(ctx, dm, marks, s, rs, None, None)
            if mode == "zero":
                ctx.set_viscosity_law(0)
            elif mode == "set then zero":
                ctx.set_viscosity_law(SMAGORINSKY, (0.3, ))
                ctx.set_viscosity_law(0, None)
            opts = ctx.default_step_opts()
            ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=0.5 / 8)
            for step in range(3):
                ts.update_coefficients()
                ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
                ctx.step_imex(opts)
                ctx.advance(0)
                ts.advance_time()
            out.append([ctx.get_state(slot) for slot in (nat.U0, nat.U1, nat.U2, nat.USTAR, nat.P, nat.P_OLD,
                                                         nat.CONV_N2)])
            info = ctx.viscosity_info()
            assert info["law"] == 0 and info["element_launches"] == 0 and info["recomputed"] == 0, info
        finally:
            ctx.close()
    assert np.abs(out[0][0]).max() > 0.5
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- 5. refusals
def test_partitioned_contexts_and_the_other_schemes_are_refused():
    mesh, dm, marks, s, rs, make = _mesh((8, 8))
    group = nat.local_group_create(1)
    ctx = make(mesh, dm)
    try:
        ctx.attach_local_comm(group, 0)
        with pytest.raises(nat.NativeError, match="communicator"):
            ctx.set_viscosity_law(SMAGORINSKY, (0.2, ))
        with pytest.raises(nat.NativeError, match="communicator"):
            ctx.viscosity_residual(nat.U1, 1.0)
        with pytest.raises(nat.NativeError, match="communicator"):
            ctx.viscosity_cells(nat.U1)
        ctx.set_viscosity_law(0)                       # law 0 is no feature: allowed
    finally:
        ctx.close()
        nat.local_group_destroy(group)
    ctx = make(mesh, dm)
    try:
        ctx.set_coeffs(1.0, 1.0, 0.01)
        ctx.set_dirichlet(nat.VELOCITY, *cavity_bc(dm, marks))
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        ctx.set_bdf((1.0, -1.0, 0.0), 1.0 / 16.0)
        ctx.set_viscosity_law(SMAGORINSKY, (0.2, ))
        with pytest.raises(nat.NativeError, match="variable viscosity"):
            ctx.step_ipcs()
        with pytest.raises(nat.NativeError, match="variable viscosity"):
            ctx.step_bdf()
        ctx.set_viscosity_law(0)
        assert ctx.step_ipcs().converged               # a Newtonian run goes on as before
    finally:
        ctx.close()


# ---------------------------------------------------------------- 6. through the classes
_SPEC = dict(name="Cavity", mesh=("cube", 2, 8), scheme="ipcs", clock=dict(dt=0.5 / 8, steps=3),
             numbers=dict(Re=100.0), start={"velocity": (0.0, 0.0), "pressure": 0.0},
             bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_slip", "bottom"), ("velocity", "top", (1.0, 0.0))])


def test_solver_class_with_the_hook_equals_driving_the_steps_by_hand(monkeypatch):
    """IMEXIPCSSolver through InstationaryProblem.solve_problem with the set_viscosity_model hook on the 8 x 8 cavity,
    3 steps: bit for bit what set_viscosity_law / step_imex / advance give through the C ABI;
    _compute_model_viscosity returns the device cell means as a cell field"""
    from fem_function import HostField
    from multigrid import attach_hierarchy
    from ns_imex_solver import IMEXIPCSSolver
    from problem_specs import build_problem
    from viscosity_models import SmagorinskyModel
    monkeypatch.setenv("NSFEM_NO_OUTPUT", "1")
    steps, dt = _SPEC["clock"]["steps"], _SPEC["clock"]["dt"]
    problem = build_problem(dict(_SPEC))

    def set_viscosity_model(self):
        self._viscosity_model = SmagorinskyModel(_CS_STEPS)
    type(problem).set_viscosity_model = set_viscosity_model
    problem.set_solver_class(IMEXIPCSSolver)
    problem.compute_cfl = False
    problem.solve_problem()
    solver = problem._get_solver()
    assert isinstance(solver, IMEXIPCSSolver) and problem._time_stepping.step_number == steps
    info = solver._ctx.viscosity_info()
    assert info["law"] == 1 and info["element_launches"] == steps and info["recomputed"] == 0, info
    u_cls, p_cls = solver._ctx.get_state(nat.U1), solver._ctx.get_state(nat.P_OLD)
    field = problem._compute_model_viscosity()
    assert isinstance(field, HostField) and field.center == "Cell" and field.name() == "model viscosity"
    assert field.values.shape == (solver._mesh.num_cells(), ) and field.values.max() > 1e-4
    assert np.array_equal(field.values, solver._ctx.viscosity_cells(nat.U0))
    problem._add_to_field_output(field)
    # ---- the same steps through the C ABI on a fresh context
    dm, mesh = solver._dofmap, solver._mesh
    ctx = nat.NsfemContext(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap, dm.n_p2, dm.n_p1)
    try:
        if solver._mg_levels is not None:
            attach_hierarchy(ctx, mesh)
        coef = solver._equation_coefficients
        ctx.set_coeffs(coef["convective_term"], coef["pressure_term"], coef["viscous_term"])
        bd, bv = solver._dirichlet_bcs["velocity"]
        ctx.set_dirichlet(nat.VELOCITY, np.asarray(bd, np.int32), np.asarray(bv, float))
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        ctx.set_viscosity_law(1, (_CS_STEPS, ))
        opts = solver._step_options()
        ts = IMEXTimeStepping(0.0, 1.0, IMEXType.SBDF2, desired_start_time_step=dt)
        for _ in range(steps):
            ts.update_coefficients()
            ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
            ctx.step_imex(opts)
            ts.advance_time()
            ctx.advance(0)
        u_abi, p_abi = ctx.get_state(nat.U1), ctx.get_state(nat.P_OLD)
    finally:
        ctx.close()
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "imex_cavity8_steps3.npz"))
    assert rel(u_cls, golden["u1"]) > 1e-3                # (the model did change the flow)
    assert np.array_equal(u_cls, u_abi) and np.array_equal(p_cls, p_abi)
    # the model is dropped again: law 0 on the device
    solver.set_viscosity_model(None)
    assert solver._ctx.viscosity_info()["law"] == 0


def test_problem_without_the_hook_is_unchanged(monkeypatch):
    """a problem without set_viscosity_model under IMEXIPCSSolver: the fields after 3 steps equal, byte for byte, the
    result recorded before this feature (tests/golden/imex_cavity8_steps3.npz), and no element kernel was launched"""
    from ns_imex_solver import IMEXIPCSSolver
    from problem_specs import build_problem
    monkeypatch.setenv("NSFEM_NO_OUTPUT", "1")
    problem = build_problem(dict(_SPEC))
    problem.set_solver_class(IMEXIPCSSolver)
    problem.compute_cfl = False
    problem.solve_problem()
    ctx = problem._get_solver()._ctx
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "imex_cavity8_steps3.npz"))
    for name, slot in (("u0", nat.U0), ("u1", nat.U1), ("ustar", nat.USTAR), ("p", nat.P), ("p_old", nat.P_OLD)):
        assert golden[name].tobytes() == ctx.get_state(slot).tobytes(), name
    assert ctx.viscosity_info() == dict(law=0, element_launches=0, recomputed=0)
    with pytest.raises(RuntimeError, match="no law"):
        problem._compute_model_viscosity()
