"""Immersed bodies in the IMEX step on the GPU (nsfem_set_bodies / nsfem_move_bodies / nsfem_body_residual /
nsfem_body_mask_cells / nsfem_body_forces / nsfem_body_info, IMEXIPCSSolver.set_immersed_bodies) against the numpy
restatement of tests/test_immersed_bodies_host.py.

Tolerances.  Sharp masks: 1e-13 relative to the largest entry, the project's figure for element kernels against the
oracle.  Smoothed masks call sin: the largest difference measured over the meshes below is 1.25e-15 of the largest
entry (box(16, 16), moving disc; the sharp kernels show 1.15e-15, so this is the rounding of the sums, not of sin;
DESIGN.md 4o), asserted ten times that, 1.25e-14 (library roundings differ between compilers), below the cap of 1e-11.
Steps: those of tests/test_gpu_imex.py -- u*, u 1e-9 and p minus its mean 1e-8, relative.

Meshes.  Those of tests/test_gpu_variable_viscosity.py; on its general tetrahedra every body cuts cells of both
orientations (asserted on the host: cells whose sharp mask is neither empty nor full, by the sign of det J).  On its
periodic fixtures the body set "seam": one ball inside the domain and one cut by the periodic side x = 0.  The kernels
take the coordinates of the cells, so the cut ball has NO periodic image at x = L (include/nsfem.h says so, and
test_a_body_cut_by_a_periodic_side_has_no_image pins it).  Bodies: ``bodies_2d`` / ``bodies_3d`` of the host file; no
quadrature point lies within 1e-9 of a surface (asserted on the host before every sharp comparison, which would hang on
one rounding otherwise; the host file pins the actual clearances, >= 1.2e-4 in 2D)."""
import os

import numpy as np
import pytest

import _native as nat
from general_tet_mesh import jacobians
from gpu_common import cavity_bc, rel
from imex_time_stepping import IMEXTimeStepping, IMEXType
from immersed_bodies import Ball, Box, HalfSpace, ImmersedBodies
from periodic_meshes import CHANNELS, is_periodic, lengths_of, periodic_axes, periodic_fields
from test_gpu_3d import lid_bc
from test_gpu_variable_viscosity import _COEF, _CS_STEPS, _KERNEL_MESHES, NO_PBC, _advance, _mesh, _opts, is_general
from test_immersed_bodies_host import (BODY_NAMES, IMEXPenalRestatement, PenalisationRestatement, bodies_2d,
                                       bodies_3d)
from test_scalar_transport_host import smooth_fields
from test_variable_viscosity_host import SMAGORINSKY, VariableViscosityRestatement

pytestmark = pytest.mark.gpu

EPS = 0.07
# the largest smoothed-mask difference printed by test_body_kernels_match_the_restatement over all its cases
SMOOTH_MEASURED = 1.25e-15
_TOL = {0.0: 1e-13, EPS: min(10.0 * SMOOTH_MEASURED, 1e-11)}


def _max_rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def _dim(kind):
    if is_periodic(kind):
        return len(lengths_of(kind))
    return 2 if kind == "mapped" or isinstance(kind[0], int) else 3


def body_cases(names=BODY_NAMES):
    """(mesh kind, body set) of the kernel tests: every set on the other meshes, "seam" on the periodic fixtures"""
    return [(k, n) for k in _KERNEL_MESHES for n in (("seam", ) if is_periodic(k) else names)]


def velocity_and_scalar(kind, dm):
    """the smooth non-polynomial fields of the kernel tests; periodic ones on a periodic fixture"""
    if is_periodic(kind):
        return periodic_fields(dm.p2_coords, lengths_of(kind), periodic_axes(kind))
    return smooth_fields(dm.p2_coords)


def cut_cells_by_orientation(mesh, means):
    """(number of cut cells with det J > 0, with det J < 0): cells whose mean of the sharp mask is neither 0 nor 1"""
    cut = (means > 0.0) & (means < 1.0)
    det = np.linalg.det(jacobians(mesh))
    return int((cut & (det > 0.0)).sum()), int((cut & (det < 0.0)).sum())


# ---------------------------------------------------------------- 1. the kernels against the restatement
@pytest.mark.parametrize("kind,name", body_cases(), ids=str)
def test_body_kernels_match_the_restatement(kind, name):
    """(weight / eta) B(u), the cell means of chi and volumes / forces / torques for the smooth non-polynomial velocity,
    each body sharp and smoothed, at rest and with U and W; second calls return the same bytes, the weight rides in the
    kernel, the node sums equal the summed forces, no stored state is touched.

    Sum identity: both sides are sums of the same products in another order; each is within (number of terms) * 2.2e-16
    * (sum of the absolute terms) of the exact value, so their difference is within the sum of the two bounds."""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    dim = _dim(kind)
    u, _ = velocity_and_scalar(kind, dm)
    eta = 0.037
    ctx = make(mesh, dm)
    try:
        ctx.set_state(nat.U1, u)
        ctx.set_state(nat.USTAR, u)
        launches = 0
        for eps in (0.0, EPS):
            for moving in (False, True):
                bodies = ImmersedBodies((bodies_2d if dim == 2 else bodies_3d)(name, moving), eta, eps)
                orc = PenalisationRestatement(rs, bodies)
                assert orc.surface_clearance() >= 1e-9
                want, means, forces = orc.residual(u), orc.cell_means(), orc.forces(u)
                if is_general(kind) and eps == 0.0:
                    assert min(cut_cells_by_orientation(mesh, means)) >= 4
                ctx.set_bodies(bodies.rows(), eta, eps)
                got = ctx.body_residual(nat.U1, 1.0)
                cells = ctx.body_mask_cells()
                F = ctx.body_forces(nat.U1)
                err, cerr, ferr = _max_rel(got, want), _max_rel(cells, means), _max_rel(F, forces)
                print("kernel %s %s eps %.2f moving %d: B %.2e cell means %.2e forces %.2e (of the largest entry)" % (
                    kind, name, eps, moving, err, cerr, ferr))
                assert np.abs(want).max() > 1e-3 and 0.0 < means.max() <= 1.0
                assert F.shape == forces.shape == (len(bodies.bodies), 4 if dim == 2 else 7)
                assert err < _TOL[eps] and cerr < _TOL[eps] and ferr < _TOL[eps], (err, cerr, ferr)
                assert got.tobytes() == ctx.body_residual(nat.U1, 1.0).tobytes()
                assert cells.tobytes() == ctx.body_mask_cells().tobytes()
                assert F.tobytes() == ctx.body_forces(nat.U1).tobytes()
                assert _max_rel(ctx.body_residual(nat.USTAR, -1.5), -1.5 * want) < _TOL[eps]
                launches += 5
                B = got.reshape(-1, dim)
                absf = np.einsum("cq,cqa->a", rs.wdet, np.abs(orc._density(u)))
                bound = 2.2e-16 * (B.shape[0] * np.abs(B).sum(axis=0) + orc.chi.size * absf)
                assert (np.abs(B.sum(axis=0) - F[:, 1:1 + dim].sum(axis=0)) <= bound).all()
        assert not ctx.get_state(nat.CONV_N1).any() and not ctx.get_state(nat.CONV_N2).any()
        assert np.array_equal(ctx.get_state(nat.U1), u)
        info = ctx.body_info()
        assert info == dict(bodies=len(bodies.bodies), element_launches=launches, recomputed=0), info
    finally:
        ctx.close()


def test_body_forces_on_a_second_trip_of_the_cell_loop():
    """box(192, 192) = 73,728 cells, the smallest square box with more cells than the 256 x 256 threads of a grid row
    of k_penal_forces: 8,192 threads integrate a second cell.  Volume, force and torque of the moving disc, sharp and
    smoothed, against the restatement under the tolerances of the kernel test"""
    mesh, dm, marks, s, rs, make = _mesh((192, 192))
    assert mesh.num_cells() == 73728 > 256 * 256
    u, _ = smooth_fields(dm.p2_coords)
    eta = 0.037
    ctx = make(mesh, dm)
    try:
        ctx.set_state(nat.U1, u)
        for eps in (0.0, EPS):
            bodies = ImmersedBodies(bodies_2d("disc", True), eta, eps)
            orc = PenalisationRestatement(rs, bodies)
            assert orc.surface_clearance() >= 1e-9
            forces = orc.forces(u)
            ctx.set_bodies(bodies.rows(), eta, eps)
            F = ctx.body_forces(nat.U1)
            ferr = _max_rel(F, forces)
            print("box(192, 192) disc eps %.2f: forces %.2e (of the largest entry)" % (eps, ferr))
            assert F.shape == forces.shape == (1, 4) and np.abs(forces).min() > 1e-6
            assert ferr < _TOL[eps], ferr
            assert F.tobytes() == ctx.body_forces(nat.U1).tobytes()
    finally:
        ctx.close()


@pytest.mark.parametrize("kind", CHANNELS)
def test_a_body_cut_by_a_periodic_side_has_no_image(kind):
    """a ball of radius 0.2 centred on the periodic side x = 0 of a channel, sharp mask, on the device alone: every cell
    with a vertex on x = 0 -- the seam cells of the low side -- may carry mask, the cells of the high half of the
    domain (all vertices at x >= L / 2), where a periodic image would cover the last column, have exactly zero, and
    the volume is that of the half ball inside the domain, not of the whole one: the kernels take cell coordinates, bodies are not periodic"""
    mesh, dm, marks, s, rs, make = _mesh(kind)
    dim = _dim(kind)
    L = lengths_of(kind)
    r = 0.2
    ball = Ball((0.0, ) + tuple(0.5 * l for l in L[1:]), r)
    bodies = ImmersedBodies([ball], 0.037, 0.0)
    orc = PenalisationRestatement(rs, bodies)
    assert orc.surface_clearance() >= 1e-9
    x = mesh.coords[mesh.cells.astype(np.int64)][:, :, 0]
    high, low = x.min(axis=1) > 0.5 * L[0] - 1e-12, x.min(axis=1) < 1e-12
    assert high.sum() >= 2 and low.sum() >= 2
    u, _ = velocity_and_scalar(kind, dm)
    ctx = make(mesh, dm)
    try:
        ctx.set_state(nat.U1, u)
        ctx.set_bodies(bodies.rows(), 0.037, 0.0)
        cells, F = ctx.body_mask_cells(), ctx.body_forces(nat.U1)
    finally:
        ctx.close()
    whole = np.pi * r * r if dim == 2 else 4.0 / 3.0 * np.pi * r ** 3
    print("%s: mask at the low side up to %.3f, at the high side %.1e; volume %.5f of %.5f for the whole ball" % (
        kind, cells[low].max(), cells[high].max(), F[0, 0], whole))
    assert cells[low].max() > 0.05 and np.all(cells[high] == 0.0)
    assert 0.3 * whole < F[0, 0] < 0.7 * whole
    assert _max_rel(cells, orc.cell_means()) < 1e-13


# ---------------------------------------------------------------- 2. steps against the restatement
def _setup(ctx, dm, marks, s, penal, visc=None):
    """coefficients, cavity / lid boundary values and the body force of the viscosity tests; two restatements, with
    and without the bodies"""
    X = dm.p2_coords
    dim = X.shape[1]
    vbc = cavity_bc(dm, marks) if dim == 2 else lid_bc(dm, marks)
    f = np.stack([np.sin(np.pi * X[:, 1]), -1.0 + X[:, 0], 0.5 * X[:, 1]][:dim], axis=1).ravel()
    orc = IMEXPenalRestatement(s, _COEF, "standard", visc=visc, penal=penal)
    plain = IMEXPenalRestatement(s, _COEF, "standard", visc=visc, penal=None)
    orc.body_force = plain.body_force = f
    ctx.set_coeffs(1.0, 1.0, 0.01, 1.0)
    ctx.set_dirichlet(nat.VELOCITY, *vbc)
    ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
    ctx.set_state(nat.BODY_FORCE, f)
    return orc, plain, vbc


def _solve(ctx, orc, plain, ts, vbc, opts, tag=""):
    """one step of the device and of the two restatements; the device against the one with bodies"""
    ts.update_coefficients()
    kk = ts.get_next_step_size()
    ctx.set_imex(ts.alpha, ts.beta, ts.gamma, kk)
    ctx.step_imex(opts)
    orc.step(ts.alpha, ts.beta, ts.gamma, kk, vbc, NO_PBC)
    plain.step(ts.alpha, ts.beta, ts.gamma, kk, vbc, NO_PBC)
    us, u, p = ctx.get_state(nat.USTAR), ctx.get_state(nat.U0), ctx.get_state(nat.P)
    es, eu = rel(us, orc.ustar), rel(u, orc.vel[0])
    ep = rel(p - p.mean(), orc.p - orc.p.mean())
    print("%s step %d k %.4g: u* %.2e u %.2e p %.2e path %s" % (tag, ts.step_number, kk, es, eu, ep,
                                                                ctx.imex_info()["path"]))
    assert es < 1e-9 and eu < 1e-9 and ep < 1e-8, (tag, es, eu, ep)


def _effect(orc, plain, tag):
    change = rel(orc.ustar, plain.ustar)
    print("%s: effect of B on u* %.2e" % (tag, change))
    assert change > 1e-3
    return change


def _step_size(kind):
    n = kind[0] if isinstance(kind[0], int) else (8 if kind == "mapped" else kind[0][0])
    return 0.5 / n


def _run(kind, typ, make_bodies, steps=4, visc_cs=None, change_k_at=None):
    mesh, dm, marks, s, rs, make = _mesh(kind)
    k = _step_size(kind)
    bodies = make_bodies(k)
    ctx = make(mesh, dm)
    try:
        penal = PenalisationRestatement(rs, bodies)
        assert penal.surface_clearance() >= 1e-9
        visc = VariableViscosityRestatement(rs, SMAGORINSKY, (visc_cs, )) if visc_cs else None
        orc, plain, vbc = _setup(ctx, dm, marks, s, penal, visc)
        if visc_cs:
            ctx.set_viscosity_law(SMAGORINSKY, (visc_cs, ))
        ctx.set_bodies(bodies.rows(), bodies.eta, bodies.smoothing)
        ts = IMEXTimeStepping(0.0, 1.0e9, typ, desired_start_time_step=k)
        opts = _opts(ctx)
        tag = "%s %s" % (kind, typ.name)
        for i in range(steps):
            if change_k_at == i:
                ts.set_desired_next_step_size(0.5 * k)
            _solve(ctx, orc, plain, ts, vbc, opts, tag)
            _advance(ctx, orc, ts)
            plain.advance()
        _effect(orc, plain, tag)
        return ctx.imex_info(), ctx.body_info(), ctx.viscosity_info()
    finally:
        ctx.close()


def _disc(k, eps=0.0):
    return ImmersedBodies(bodies_2d("disc"), 2.0 * k, eps)


@pytest.mark.parametrize("typ", (IMEXType.SBDF2, IMEXType.CNAB, IMEXType.mCNAB), ids=lambda t: t.name)
def test_steps_with_a_disc_match_the_restatement(typ):
    """lid-driven cavity on box(8, 8) (generic right-hand-side path) with the sharp disc at rest and eta = 2 k, 4 steps"""
    info, binfo, _ = _run((8, 8), typ, _disc)
    assert info["path"] == "generic" and info["generic_rhs"] == 4, info
    # one element launch per step for B(u1); B(u2) is in what the step before stored
    assert binfo == dict(bodies=1, element_launches=4, recomputed=0), binfo


@pytest.mark.parametrize("kind,path", [((16, 16), "lattice-kernel"), ("mapped", "generic"),
                                       (((4, 4, 4), (1.0, 1.0, 1.0)), "generic")], ids=str)
def test_sbdf2_steps_on_the_other_meshes(kind, path):
    """SBDF2, 4 steps: box(16, 16) runs the one-launch lattice right-hand side (path 2) and the two extra launches after
    it; the mapped mesh has cells of different shape; the (4, 4, 4) cube runs the 3D kernel with the ball.  The bodies
    are smoothed here (eps = 0.07)"""
    def make_bodies(k):
        return ImmersedBodies((bodies_2d if _dim(kind) == 2 else bodies_3d)("disc"), 2.0 * k, EPS)
    info, binfo, _ = _run(kind, IMEXType.SBDF2, make_bodies)
    assert info["path"] == path, info
    if path == "lattice-kernel":
        assert info["lattice_rhs"] == 4 and info["generic_rhs"] == 0
    assert binfo == dict(bodies=1, element_launches=4, recomputed=0), binfo


def test_bodies_together_with_smagorinsky_and_a_step_size_change():
    """both explicit additions: viscosity cells, gather, penalisation cells, gather (the restatement adds V before B);
    the step size halves before step 3 and the stored vector is kept"""
    info, binfo, vinfo = _run((8, 8), IMEXType.SBDF2, lambda k: _disc(k, EPS), steps=5, visc_cs=_CS_STEPS, change_k_at=2)
    assert binfo == dict(bodies=1, element_launches=5, recomputed=0), binfo
    assert vinfo["element_launches"] == 5 and vinfo["recomputed"] == 0, vinfo


def test_a_moving_disc_keeps_the_stored_vector():
    """a smoothed disc that translates and spins, nsfem_move_bodies before every step: N(u2) stays the vector stored
    with the pose of t^(n-1) (never recomputed), and a right-hand side evaluated afresh (nsfem_imex_rhs) forms N(u2)
    with that older pose again"""
    kind = (8, 8)
    mesh, dm, marks, s, rs, make = _mesh(kind)
    k = _step_size(kind)
    disc = Ball((0.4, 0.55), 0.2, motion=lambda t: ((0.4 + 0.4 * t, 0.55), (0.4, 0.0), 0.6))
    bodies = ImmersedBodies([disc], 2.0 * k, EPS)
    ctx = make(mesh, dm)
    try:
        orc, plain, vbc = _setup(ctx, dm, marks, s, None)
        ctx.set_bodies(bodies.rows(0.0), bodies.eta, bodies.smoothing)
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=k)
        opts = _opts(ctx)
        for _ in range(4):
            t = ts.current_time
            ctx.move_bodies(bodies.rows(t))
            orc.penal = PenalisationRestatement(rs, bodies, t)
            _solve(ctx, orc, plain, ts, vbc, opts, "moving disc t %.4f" % t)
            _advance(ctx, orc, ts)
            plain.advance()
        _effect(orc, plain, "moving disc")
        assert ctx.body_info() == dict(bodies=1, element_launches=4, recomputed=0)
        # the step that would come next, its right-hand side evaluated afresh: orc.N2 is B(u2) with the pose of t^(n-1)
        t = ts.current_time
        ctx.move_bodies(bodies.rows(t))
        orc.penal = PenalisationRestatement(rs, bodies, t)
        ts.update_coefficients()
        kk = ts.get_next_step_size()
        ctx.set_imex(ts.alpha, ts.beta, ts.gamma, kk)
        got, n1 = ctx.imex_rhs("generic", 0)
        want = orc.rhs(ts.alpha, ts.beta, ts.gamma, kk)
        free = np.ones(got.size, dtype=bool)              # (the hook returns no Dirichlet rows: compare the others)
        free[vbc[0]] = False
        print("moving disc, fresh right-hand side: %.2e, N1 %.2e" % (rel(got[free], want[free]), rel(n1, orc.N1)))
        assert rel(got[free], want[free]) < 1e-9 and rel(n1, orc.N1) < 1e-9
        # (with the pose of t^n for u2 instead the difference is visible: the check above is no tautology)
        wrong = want + ts.beta[1] * (orc.N2 - orc.explicit(orc.vel[2]))
        assert rel(wrong[free], want[free]) > 1e-6
    finally:
        ctx.close()


# ---------------------------------------------------------------- 3. no bodies
def test_no_bodies_leaves_the_step_bit_identical():
    """nsfem_set_bodies(n = 0) -- after a set that was never used in a step -- and a context that never made the call
    give the same bytes over 4 steps; no element kernel is launched"""
    mesh, dm, marks, s, rs, make = _mesh((8, 8))
    out = []
    for mode in ("never", "zero", "set then zero"):
        ctx = make(mesh, dm)
        try:
            _setup(ctx, dm, marks, s, None)
            if mode == "zero":
                ctx.set_bodies([])
            elif mode == "set then zero":
                ctx.set_bodies(ImmersedBodies(bodies_2d("overlap"), 0.1).rows(), 0.1, EPS)
                ctx.set_bodies([])
            opts = ctx.default_step_opts()
            ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=0.5 / 8)
            for step in range(4):
                ts.update_coefficients()
                ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
                ctx.step_imex(opts)
                ctx.advance(0)
                ts.advance_time()
            out.append([ctx.get_state(slot) for slot in (nat.U0, nat.U1, nat.U2, nat.USTAR, nat.P, nat.P_OLD,
                                                         nat.CONV_N2)])
            assert ctx.body_info() == dict(bodies=0, element_launches=0, recomputed=0)
        finally:
            ctx.close()
    assert np.abs(out[0][0]).max() > 0.5
    for other in out[1:]:
        for a, b in zip(out[0], other):
            assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- 4. the epoch
def test_changing_eta_recomputes_the_stored_vector_and_the_same_set_does_not():
    mesh, dm, marks, s, rs, make = _mesh((8, 8))
    k = _step_size((8, 8))
    ctx = make(mesh, dm)
    try:
        bodies = _disc(k, EPS)
        orc, plain, vbc = _setup(ctx, dm, marks, s, PenalisationRestatement(rs, bodies))
        ctx.set_bodies(bodies.rows(), bodies.eta, bodies.smoothing)
        ts = IMEXTimeStepping(0.0, 1.0e9, IMEXType.SBDF2, desired_start_time_step=k)
        opts = _opts(ctx)

        def step(tag):
            _solve(ctx, orc, plain, ts, vbc, opts, tag)
            _advance(ctx, orc, ts)
            plain.advance()

        for _ in range(2):
            step("epoch")
        assert ctx.body_info()["recomputed"] == 0
        ctx.set_bodies(bodies.rows(), bodies.eta, bodies.smoothing)            # the same set again
        step("same set")
        assert ctx.body_info()["recomputed"] == 0
        bodies = ImmersedBodies(bodies.bodies, 3.0 * k, EPS)                    # eta changes
        ctx.set_bodies(bodies.rows(), bodies.eta, bodies.smoothing)
        orc.penal, orc.N2 = PenalisationRestatement(rs, bodies), None
        step("eta")
        assert ctx.body_info()["recomputed"] == 1
        bodies = ImmersedBodies(bodies.bodies, 3.0 * k, 0.5 * EPS)              # the smoothing changes
        ctx.set_bodies(bodies.rows(), bodies.eta, bodies.smoothing)
        orc.penal, orc.N2 = PenalisationRestatement(rs, bodies), None
        step("smoothing")
        assert ctx.body_info() == dict(bodies=1, element_launches=5 + 2, recomputed=2)
    finally:
        ctx.close()


# ---------------------------------------------------------------- 5. refusals
def test_everything_the_header_refuses_is_refused():
    mesh, dm, marks, s, rs, make = _mesh((8, 8))
    disc = (1, (0.5, 0.5), (0.2, ), (0.0, 0.0), 0.0)
    group = nat.local_group_create(1)
    ctx = make(mesh, dm)
    try:
        ctx.attach_local_comm(group, 0)
        with pytest.raises(nat.NativeError, match="communicator"):
            ctx.set_bodies([disc], 0.1)
        ctx.set_bodies([])                              # no bodies is no feature: allowed
    finally:
        ctx.close()
        nat.local_group_destroy(group)
    ctx = make(mesh, dm)
    try:
        for call in (lambda: ctx.body_residual(nat.U1, 1.0), ctx.body_mask_cells, lambda: ctx.body_forces(nat.U1),
                     lambda: ctx.move_bodies([disc])):
            with pytest.raises(nat.NativeError, match="no body set"):
                call()
        with pytest.raises(nat.NativeError, match="NSFEM_MAX_BODIES"):
            ctx.set_bodies([disc] * 17, 0.1)
        for kind in (0, 4, -1):
            with pytest.raises(nat.NativeError, match="unknown kind"):
                ctx.set_bodies([(kind, ) + disc[1:]], 0.1)
        for size in ((0.0, ), (-0.2, ), (np.nan, ), (np.inf, )):
            with pytest.raises(nat.NativeError, match="size"):
                ctx.set_bodies([(1, (0.5, 0.5), size, (0.0, 0.0), 0.0)], 0.1)
        for size in ((0.1, 0.0), (0.1, -0.1), (np.nan, 0.1)):
            with pytest.raises(nat.NativeError, match="size"):
                ctx.set_bodies([(2, (0.5, 0.5), size, (0.0, 0.0), 0.0)], 0.1)
        for size in ((0.6, 0.81), (0.0, 0.0), (1.0, 1e-5)):
            with pytest.raises(nat.NativeError, match="unit normal"):
                ctx.set_bodies([(3, (0.5, 0.5), size, (0.0, 0.0), 0.0)], 0.1)
        for eta in (0.0, -0.1, np.nan, np.inf):
            with pytest.raises(nat.NativeError, match="eta"):
                ctx.set_bodies([disc], eta)
        for eps in (-0.01, np.nan):
            with pytest.raises(nat.NativeError, match="smoothing"):
                ctx.set_bodies([disc], 0.1, eps)
        assert ctx.body_info() == dict(bodies=0, element_launches=0, recomputed=0)
        ctx.set_bodies([disc, (3, (0.3, 0.2), (0.6, 0.8), (0.0, 0.0), 0.0)], 0.1)
        with pytest.raises(nat.NativeError, match="another count"):
            ctx.move_bodies([disc])
        with pytest.raises(nat.NativeError, match="another kind"):
            ctx.move_bodies([disc, disc])
        for slot in (nat.P, nat.CONV_N1, nat.BODY_FORCE):
            with pytest.raises(nat.NativeError, match="slot"):
                ctx.body_residual(slot, 1.0)
            with pytest.raises(nat.NativeError, match="slot"):
                ctx.body_forces(slot)
        ctx.set_coeffs(1.0, 1.0, 0.01)
        ctx.set_dirichlet(nat.VELOCITY, *cavity_bc(dm, marks))
        ctx.set_dirichlet(nat.PRESSURE, *NO_PBC)
        ctx.set_bdf((1.0, -1.0, 0.0), 1.0 / 16.0)
        with pytest.raises(nat.NativeError, match="immersed bodies"):
            ctx.step_ipcs()
        with pytest.raises(nat.NativeError, match="immersed bodies"):
            ctx.step_bdf()
        ctx.set_bodies([])
        assert ctx.step_ipcs().converged               # a run without bodies goes on as before
    finally:
        ctx.close()


# ---------------------------------------------------------------- 6. through the classes
_SPEC = dict(name="Cavity", mesh=("cube", 2, 8), scheme="ipcs", clock=dict(dt=0.5 / 8, steps=3),
             numbers=dict(Re=100.0), start={"velocity": (0.0, 0.0), "pressure": 0.0},
             bcs=[("no_slip", "left"), ("no_slip", "right"), ("no_slip", "bottom"), ("velocity", "top", (1.0, 0.0))])


def _problem(monkeypatch, bodies, solver_class=None, allow_stiff=False):
    from ns_imex_solver import IMEXIPCSSolver
    from problem_specs import build_problem
    monkeypatch.setenv("NSFEM_NO_OUTPUT", "1")
    problem = build_problem(dict(_SPEC))

    def set_immersed_bodies(self):
        self._immersed_bodies = bodies
        self._immersed_allow_stiff = allow_stiff
    type(problem).set_immersed_bodies = set_immersed_bodies
    problem.set_solver_class(solver_class or IMEXIPCSSolver)
    problem.compute_cfl = False
    return problem


def test_solver_class_with_the_hook_equals_driving_the_steps_by_hand(monkeypatch):
    """IMEXIPCSSolver through InstationaryProblem.solve_problem with the set_immersed_bodies hook on the 8 x 8 cavity, a
    disc under the lid that moves with the lid's direction, 3 steps: bit for bit what set_bodies / move_bodies /
    step_imex / advance give through the C ABI; the two output helpers return what the device returns"""
    from fem_function import HostField
    from multigrid import attach_hierarchy
    from ns_imex_solver import IMEXIPCSSolver
    steps, dt = _SPEC["clock"]["steps"], _SPEC["clock"]["dt"]
    disc = Ball((0.4, 0.7), 0.15, motion=lambda t: ((0.4 + 0.3 * t, 0.7), (0.3, 0.0), 0.0))
    bodies = ImmersedBodies([disc, Box((0.5, 0.25), (0.2, 0.1))], 2.0 * dt, 0.05)
    problem = _problem(monkeypatch, bodies)
    problem.solve_problem()
    solver = problem._get_solver()
    assert isinstance(solver, IMEXIPCSSolver) and problem._time_stepping.step_number == steps
    assert solver._ctx.body_info() == dict(bodies=2, element_launches=steps, recomputed=0)
    u_cls, p_cls = solver._ctx.get_state(nat.U1), solver._ctx.get_state(nat.P_OLD)
    field = problem._compute_body_mask()
    assert isinstance(field, HostField) and field.center == "Cell" and field.name() == "body mask"
    assert field.values.shape == (solver._mesh.num_cells(), ) and field.values.max() == 1.0
    assert np.array_equal(field.values, solver._ctx.body_mask_cells())
    problem._add_to_field_output(field)
    forces = problem._compute_body_forces()
    assert forces.shape == (2, 4) and np.array_equal(forces, solver._ctx.body_forces(nat.U0))
    assert abs(forces[1, 0] - 0.08) < 0.01                  # (the box: 0.4 x 0.2, smoothed)
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
        ctx.set_bodies(bodies.rows(0.0), bodies.eta, bodies.smoothing)
        opts = solver._step_options()
        ts = IMEXTimeStepping(0.0, 1.0, IMEXType.SBDF2, desired_start_time_step=dt)
        for _ in range(steps):
            ts.update_coefficients()
            ctx.set_imex(ts.alpha, ts.beta, ts.gamma, ts.get_next_step_size())
            ctx.move_bodies(bodies.rows(ts.current_time))
            ctx.step_imex(opts)
            ts.advance_time()
            ctx.advance(0)
        u_abi, p_abi = ctx.get_state(nat.U1), ctx.get_state(nat.P_OLD)
    finally:
        ctx.close()
    golden = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "imex_cavity8_steps3.npz"))
    assert rel(u_cls, golden["u1"]) > 1e-3                # (the bodies did change the flow)
    assert np.array_equal(u_cls, u_abi) and np.array_equal(p_cls, p_abi)
    # the same set handed over again in the middle of the run: the device gets the pose of t^(n-1) as the set and that
    # of t^n as ONE move, however often the step's preparations run after it
    calls, ts = [], problem._time_stepping
    real_set, real_move = solver._ctx.set_bodies, solver._ctx.move_bodies
    monkeypatch.setattr(solver._ctx, "set_bodies", lambda rows, *a: (calls.append(("set", rows[0][1].tolist())),
                                                                     real_set(rows, *a))[1])
    monkeypatch.setattr(solver._ctx, "move_bodies", lambda rows: (calls.append(("move", rows[0][1].tolist())),
                                                                  real_move(rows))[1])
    solver.set_immersed_bodies(bodies)
    solver._step_immersed_bodies()
    solver._step_immersed_bodies()
    assert ts.step_number == steps and ts.previous_time < ts.current_time
    assert calls == [("set", [0.4 + 0.3 * ts.previous_time, 0.7]), ("move", [0.4 + 0.3 * ts.current_time, 0.7])], calls
    monkeypatch.undo()
    # the bodies are dropped again
    solver.set_immersed_bodies(None)
    assert solver._ctx.body_info()["bodies"] == 0
    with pytest.raises(RuntimeError, match="no body set"):
        problem._compute_body_mask()


def test_solver_class_refuses_steps_above_the_stability_bound(monkeypatch):
    """k / eta above 4/3 under SBDF2 raises ValueError, allow_stiff lets it run; CNLF always raises"""
    from ns_imex_solver import IMEXIPCSSolver
    dt = _SPEC["clock"]["dt"]
    ok = ImmersedBodies([Ball((0.5, 0.5), 0.2)], dt / 1.3)
    stiff = ImmersedBodies([Ball((0.5, 0.5), 0.2)], dt / 1.4)
    problem = _problem(monkeypatch, ok)
    problem.solve_problem()
    assert problem._get_solver()._ctx.body_info()["element_launches"] == _SPEC["clock"]["steps"]
    with pytest.raises(ValueError, match="k / eta"):
        _problem(monkeypatch, stiff).solve_problem()
    problem = _problem(monkeypatch, stiff, allow_stiff=True)
    problem.solve_problem()
    assert problem._get_solver()._ctx.body_info()["element_launches"] == _SPEC["clock"]["steps"]

    class LeapfrogSolver(IMEXIPCSSolver):
        imex_type = IMEXType.CNLF
    with pytest.raises(ValueError, match="CNLF"):
        _problem(monkeypatch, ImmersedBodies([Ball((0.5, 0.5), 0.2)], 1.0e3 * dt), LeapfrogSolver).solve_problem()
