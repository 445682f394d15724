"""Operators of a partitioned context against the global oracle, one call at a time: the matrix-free momentum Jacobian
(k_jac_lattice after one halo exchange of the input; under the overlapped exchange split into tile rows) and the
momentum residual on strips -- 32 x 32 on 2 ranks and 64 x 64 on 4 ranks (strips of 35 / 33 P2 lines), thread ranks on
one GPU (tests/partitioned_common.py).  Until now the strips' Jacobian was checked through Newton counts of whole steps
only (tests/test_gpu_partition.py).

Re = 20, BDF2 with step 0.01, random U1, U2, USTAR, P_OLD from one global seed restricted to every rank with valid
ghost values, lid-cavity Dirichlet set.  The owned rows of the ranks' results, gathered, against
apply_dirichlet_rows(L + convection_jacobian, bd) @ x resp. the residual of
tests/test_gpu_parity.py::test_momentum_residual_and_jacobian_match_oracle at rel < 1e-13 (that test's bound).  Ghost
rows of the Jacobian action are exactly 0.0; ghost entries of the input set to 1e30 change nothing, bit for bit (the
exchange overwrites them before any tile reads them); set_overlap(1) changes nothing, bit for bit, and every
application counts one overlapped exchange (the tile-row split was taken).

Measured on an MI355X: Jacobian action rel 4.1e-16 .. 4.2e-16 (32 x 32), 1.1e-15 (64 x 64), all four forms, Newton and
Picard; residual 4.1e-16 / 1.1e-15.  The file takes 5 s, most of it the oracle's global matrices."""
import numpy as np
import pytest

import _native as nat
import fem_oracle as fo
import partitioned_common as pc
from gpu_common import rel

pytestmark = pytest.mark.gpu

RE, STEP, ALPHA = 20.0, 0.01, (1.5, -2.0, 0.5)
FORMS = [(0, "standard"), (1, "rotational"), (2, "divergence"), (3, "skew_symmetric")]


def _lid_values(c, dm, dofs):
    """lid-driven cavity: u_x = 1 on the top side, 0 elsewhere"""
    node, comp = dofs // c.dim, dofs % c.dim
    top = np.abs(dm.p2_coords[node, -1] - c.hi[-1]) < 1e-12
    return np.where(top & (comp == 0), 1.0, 0.0)


@pytest.mark.parametrize("name", ["box32/2", "box64/4 tail"])
def test_jacobian_action_and_residual_on_strips_match_the_global_oracle(name):
    c = pc.case(name)
    s = c.H.space
    rng = np.random.default_rng(31 + c.size)
    nvel = c.size_of("velocity")
    u = [rng.standard_normal(nvel) for _ in range(3)]                 # U1, U2, USTAR
    p_old = rng.standard_normal(c.dm.n_p1)
    x = rng.standard_normal(nvel)
    bd = c.dirichlet("velocity")
    bv = _lid_values(c, c.dm, bd)

    def body(r, ctx, part):
        ctx.set_coeffs(1.0, 1.0, 1.0 / RE)
        ctx.set_bdf(ALPHA, STEP)
        ld = c.dirichlet("velocity", part.dofmap)
        ctx.set_dirichlet(nat.VELOCITY, ld.astype(np.int32), _lid_values(c, part.dofmap, ld))
        ctx.set_dirichlet(nat.PRESSURE, np.zeros(0, np.int32), np.zeros(0))
        for slot, v in ((nat.U1, u[0]), (nat.U2, u[1]), (nat.USTAR, u[2])):
            ctx.set_state(slot, c.to_local("velocity", part, v, ghosts="valid"))
        ctx.set_state(nat.P_OLD, c.to_local("pressure", part, p_old, ghosts="valid"))
        x_zero = c.to_local("velocity", part, x)                       # ghost entries 0 (a Krylov vector)
        x_poison = c.to_local("velocity", part, x, ghosts=1e30)
        out = {}
        for form_id, _ in FORMS:
            for picard in (False, True):
                ctx.set_convective_form(form_id, picard=picard)
                ctx.set_overlap(0)
                y = ctx.operator_apply(nat.OP_MOMENTUM_JAC_MF, x_zero)
                y_poison = ctx.operator_apply(nat.OP_MOMENTUM_JAC_MF, x_poison)
                info = ctx.jacobian_info()
                o0 = ctx.comm_overlapped()
                ctx.set_overlap(1)
                y_over = ctx.operator_apply(nat.OP_MOMENTUM_JAC_MF, x_zero)
                o1 = ctx.comm_overlapped()
                y_over_poison = ctx.operator_apply(nat.OP_MOMENTUM_JAC_MF, x_poison)
                o2 = ctx.comm_overlapped()
                ctx.set_overlap(0)
                out[(form_id, picard)] = dict(y=y, y_poison=y_poison, y_over=y_over, y_over_poison=y_over_poison,
                                              path=info["path"], overlapped=(o0, o1, o2))
        ctx.set_convective_form(0)
        ctx.assemble(nat.SYS_MOMENTUM, new_step=True)
        out["rhs"] = ctx.get_rhs(nat.SYS_MOMENTUM)
        return out

    ranks_out = pc.run_ranks(c.parts, body)
    M, K, D = s.vector_mass(), s.vector_stiffness(), s.divergence()
    L = ALPHA[0] / STEP * M + K / RE
    for form_id, form in FORMS:
        for picard in (False, True):
            conv = s.picard_convection(u[2], form) if picard else s.convection_jacobian(u[2], form)
            want = fo.apply_dirichlet_rows(L + conv, bd) @ x
            got = c.gather("velocity", [o[(form_id, picard)]["y"] for o in ranks_out])
            err = rel(got, want)
            print("\n[strip jacobian] %-13s %-15s %-6s rel %.2e" % (name, form, "picard" if picard else "newton", err))
            assert err < 1e-13, (name, form, picard, err)
            for rank, (part, o) in enumerate(zip(c.parts, ranks_out)):
                o = o[(form_id, picard)]
                assert o["path"] == "lattice-kernel", (rank, o["path"])
                ghost = ~np.asarray(part.p2_owned)
                assert np.all(o["y"].reshape(-1, c.dim)[ghost] == 0.0), "ghost rows of the action are 0.0"
                assert np.array_equal(o["y"], o["y_poison"]), "poisoned ghost entries of the input change nothing"
                assert np.array_equal(o["y"], o["y_over"]), "the overlapped exchange changes nothing"
                assert np.array_equal(o["y"], o["y_over_poison"])
                o0, o1, o2 = o["overlapped"]
                assert (o1 - o0, o2 - o1) == (1, 1), "one overlapped exchange per application: the tile-row split"
    b = L @ u[2] + M @ (ALPHA[1] * u[0] + ALPHA[2] * u[1]) / STEP - D.T @ p_old + s.convection_residual(u[2])
    b[bd] = u[2][bd] - bv
    got = c.gather("velocity", [o["rhs"] for o in ranks_out])
    err = rel(got, b)
    print("\n[strip residual] %-13s rel %.2e" % (name, err))
    assert err < 1e-13, (name, err)
