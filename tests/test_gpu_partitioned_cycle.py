"""The multigrid V-cycles of PARTITIONED contexts -- nsfem_mg_apply(0 | 1, r) on strips, slabs, thread ranks on one
GPU -- against the host definition, cycle by cycle: exact halo mode against the serial HostCycle, relaxed halo mode
(what bench.py runs for N > 1) against PartitionedCycle (tests/mg_cycle_host.py), which states what the relaxed cycle
is: frozen ghosts inside a smoothing sequence, exact ghosts for the residual, the `ghost = 2` prolongation, the
gathered / all-reduced replicated coarse solve under the union mask, the all-reduced lmax.  Whole time steps
(tests/test_gpu_partition.py) cannot see an error in any of these: a preconditioner does not change the converged
answer.  tests/test_partitioned_cycle_host.py shows on the host that reverting any one rule but the all-reduce of lmax
(invisible on uniform strips, see there) moves z by at least 1e5 times the bound used here.

Every rank calls mg_set_halo_mode(mode), then mg_apply(which, r_local): r_local the global random vector on the
owned rows and zeros on the ghost rows (the callers' contract: Krylov vectors keep zero ghosts); the owned rows of the
results are gathered into one global z.  Cases (tests/partitioned_common.py; rows per rank P2 / P1):

    box32/2       32 x 32, 2 strips, coarsest 2: P2 2275 / 2145 on the lattice kernel, every P1 level (594 and fewer)
                  below the dictionary threshold of 1024 rows; dense 2 x 2 global coarse level (singular: pseudo-inverse)
    box64/4 tail  64 x 64, 4 strips, partitioned down to 16, replicated tail 8, 4, 2: interior ranks with ghosts on both
                  sides, P1 level 0 (1170 / 1105 rows) on the lattice kernel as well
    box48/3       48 x 48, 3 strips, coarsest 3: h = 1/48, inexact dictionary (2^-38 added to the bound), levels 24, 12, 6, 3
    box64x32/2    64 x 32 on (0, 2) x (0, 1), 2 strips: lattice width != height, global coarse level 4 x 2
    box64/8 tail  64 x 64, 8 strips of 19 / 17 P2 lines (3 of them ghosts): bench.py's N = 8 layout in small
    cube8/2       8^3, 2 slabs, nv = 3: no lattice kernel (0 lattice levels, one-step dictionary / CSR kernels in both modes)

Systems per case, each in both halo modes: all-Neumann pressure; pressure outlet on x = x_max (every rank owns
Dirichlet rows); pressure outlet on the top side y = y_max / z = z_max (ONLY the last rank owns Dirichlet rows: the
replicated level knows them through the all-reduced union alone); velocity with the cavity set, 150 M + 0.01 K.

Tolerance: the rule of tests/test_gpu_multigrid_cycle.py.  d = rel(z_float64_host, z_longdouble_host) measured on the
definition alone, the device held to max(64 d, 1e-14) (+ 2^-38 on box48), 64 d < 1e-10 asserted.

Asserted per rank and cycle: levels in use; the number of levels on the multi-step lattice kernel (relaxed mode: the
partitioned levels of >= 1024 local rows in 2D; exact mode and NSFEM_LATTICE=0: none) and that it was launched if and
only if there is one; ghost_lines of level 0 (1 below, 2 above on P2 strips, 1 / 1 on a P1 lattice level, 0 at the
domain ends); one relaxed cycle makes fewer halo exchanges than the exact cycle, both make the same number of
all-reduces; two applications are bit-identical.

Ghost rows of the returned z (contract, from the code): zeros in both modes.  Exact: the last smoothing step of level 0
runs with ghost mode 0 (k_spmv_*: rows flagged 2 store 0); relaxed: the last launch of a sequence stores zeros on the
frozen lines (smooth_lattice: `strip && last`), the one-step path ends with ghost mode 0 as well.

Measured on an MI355X (d: host only; err: rel(z_device, z_host); lv / ln: levels on the lattice kernel / its launches
per relaxed cycle, none in exact mode; halo exchanges per exact / relaxed cycle; all-reduces per cycle, the same in both
modes -- a pressure application counts the refresh mg_apply makes before it as well: one allreduce_max per partitioned
level, the mask union, and the cycle's own all-reduce of the coarse right-hand side; all of rank 0):

case          system                exact: d   bound    err        relaxed: d bound    err        lattice  exchanges  all-
                                                                                                  lv / ln  ex / rel   reduces
box32/2       pressure neumann      2.4e-16    1.6e-14  3.5e-16    2.1e-16    1.4e-14  4.6e-16    0 / 0    23 / 11    7
box32/2       pressure outlet side  2.7e-16    1.7e-14  5.8e-16    1.5e-16    1.0e-14  3.4e-16    0 / 0    23 / 11    7
box32/2       pressure outlet top   2.6e-16    1.7e-14  2.8e-16    3.3e-16    2.1e-14  3.1e-16    0 / 0    23 / 11    7
box32/2       velocity              1.2e-16    1.0e-14  4.3e-16    1.3e-16    1.0e-14  4.3e-16    1 / 1    24 / 9     1
box64/4 tail  pressure neumann      1.8e-16    1.2e-14  3.1e-16    3.0e-16    1.9e-14  5.0e-16    1 / 2    11 / 5     5
box64/4 tail  pressure outlet side  4.1e-16    2.6e-14  3.3e-16    3.8e-16    2.4e-14  3.3e-16    1 / 2    11 / 5     5
box64/4 tail  pressure outlet top   1.8e-16    1.2e-14  2.1e-16    1.9e-16    1.2e-14  3.6e-16    1 / 2    11 / 5     5
box64/4 tail  velocity              1.3e-16    1.0e-14  8.0e-16    1.3e-16    1.0e-14  8.1e-16    2 / 2    14 / 5     1
box48/3       pressure neumann      1.8e-16    3.6e-12  1.1e-15    1.8e-16    3.6e-12  1.1e-15    0 / 0    23 / 11    7
box48/3       pressure outlet side  4.6e-16    3.7e-12  8.5e-16    4.7e-16    3.7e-12  9.2e-16    0 / 0    23 / 11    7
box48/3       pressure outlet top   5.5e-16    3.7e-12  2.6e-15    5.6e-16    3.7e-12  2.5e-15    0 / 0    23 / 11    7
box48/3       velocity              1.5e-16    3.6e-12  1.3e-15    1.5e-16    3.6e-12  1.3e-15    1 / 1    24 / 9     1
box64x32/2    pressure neumann      1.2e-16    1.0e-14  2.0e-16    1.5e-16    1.0e-14  2.0e-16    1 / 2    23 / 11    7
box64x32/2    pressure outlet side  3.8e-16    2.5e-14  4.0e-16    3.1e-16    2.0e-14  2.7e-16    1 / 2    23 / 11    7
box64x32/2    pressure outlet top   3.6e-16    2.3e-14  5.4e-16    4.5e-16    2.9e-14  6.0e-16    1 / 2    23 / 11    7
box64x32/2    velocity              1.2e-16    1.0e-14  4.5e-16    1.2e-16    1.0e-14  4.4e-16    2 / 2    24 / 9     1
box64/8 tail  pressure neumann      1.9e-16    1.2e-14  5.1e-16    1.6e-16    1.0e-14  3.0e-16    0 / 0    11 / 5     5
box64/8 tail  pressure outlet side  3.0e-16    1.9e-14  2.8e-16    1.2e-16    1.0e-14  2.3e-16    0 / 0    11 / 5     5
box64/8 tail  pressure outlet top   2.3e-16    1.4e-14  2.5e-16    2.8e-16    1.8e-14  2.3e-16    0 / 0    11 / 5     5
box64/8 tail  velocity              1.2e-16    1.0e-14  8.1e-16    1.3e-16    1.0e-14  8.1e-16    1 / 1    14 / 5     1
cube8/2       pressure neumann      2.1e-16    1.4e-14  8.3e-16    1.6e-16    1.0e-14  8.4e-16    0 / 0    11 / 5     5
cube8/2       pressure outlet side  5.0e-16    3.2e-14  7.1e-16    2.6e-16    1.7e-14  5.9e-16    0 / 0    11 / 5     5
cube8/2       pressure outlet top   3.7e-16    2.4e-14  6.4e-16    4.5e-16    2.9e-14  5.6e-16    0 / 0    11 / 5     5
cube8/2       velocity              1.3e-16    1.0e-14  1.1e-15    1.4e-16    1.0e-14  1.1e-15    0 / 0    14 / 5     1

NSFEM_LATTICE=0 (box32/2, box64/4 tail, relaxed): the same errors to the digits shown, 0 lattice levels, the same
exchange counts.  set_overlap(1) (exact): bit-identical.  The whole file: 5 s on the device machine (22 tests).
"""
import numpy as np
import pytest

import _native as nat
import mg_cycle_host as mh
import partitioned_common as pc

pytestmark = pytest.mark.gpu

SWITCHES = ("NSFEM_LATTICE", "NSFEM_LATTICE_TRANSFERS", "NSFEM_DICT", "NSFEM_LATTICE_KINDS")
DICT_MIN_ROWS = 1024                   # a level gets a stencil dictionary (and the lattice kernel) from 1024 rows on
_results = {}


def run(name, relaxed, monkeypatch, env=None, overlap=False):
    """per rank {system: dict(z, z_first, info, launches, exchanges, allreduces, overlapped)} of fresh contexts:
    every system applied twice, the counters taken around the second application"""
    for s in SWITCHES:
        monkeypatch.delenv(s, raising=False)
    for s, v in (env or {}).items():
        monkeypatch.setenv(s, v)
    c = pc.case(name)
    rhs = {system: c.rhs(system) for system in pc.SYSTEMS}

    def body(r, ctx, part):
        ctx.mg_set_halo_mode(relaxed)
        ctx.mg_set_truncation(0.0, 0.1)
        ctx.set_coeffs(1.0, 1.0, pc.NU)
        ctx.set_bdf(pc.BDF2, pc.STEP)
        vd = c.dirichlet("velocity", part.dofmap)
        ctx.set_dirichlet(nat.VELOCITY, vd.astype(np.int32), np.zeros(vd.size))
        out = {}
        for system in pc.SYSTEMS:
            which = pc.which_of(system)
            if which == 0:
                pd = c.dirichlet(system, part.dofmap)
                ctx.set_dirichlet(nat.PRESSURE, pd.astype(np.int32), np.zeros(pd.size))
            r_local = c.to_local(system, part, rhs[system])
            z_first = ctx.mg_apply(which, r_local)
            i0, s0, o0 = ctx.mg_lattice_info(which), ctx.comm_stats(), ctx.comm_overlapped()
            z = ctx.mg_apply(which, r_local)
            s1, o1, i1 = ctx.comm_stats(), ctx.comm_overlapped(), ctx.mg_lattice_info(which)
            out[system] = dict(z=z, z_first=z_first, info=i1, launches=i1["lattice_launches"] - i0["lattice_launches"],
                               exchanges=s1["exchanges"] - s0["exchanges"],
                               allreduces=s1["allreduce_calls"] - s0["allreduce_calls"], overlapped=o1 - o0)
        return out

    return pc.run_ranks(c.parts, body, overlap=overlap)


def results(name, relaxed, monkeypatch):
    """the default-switch run of one case and mode, made once per module"""
    if (name, relaxed) not in _results:
        _results[(name, relaxed)] = run(name, relaxed, monkeypatch)
    return _results[(name, relaxed)]


def lattice_levels(c, system, relaxed, env=None):
    """levels of the hierarchy on the multi-step lattice kernel: relaxed halo mode, 2D, >= 1024 local rows (the same
    on every rank of these cases)"""
    if not relaxed or c.dim != 2 or (env or {}).get("NSFEM_LATTICE") == "0":
        return 0
    counts = []
    for part in c.parts:
        rows = ([part.dofmap.n_p2] if system == "velocity" else []) + [part.dofmap.n_p1] + \
               [lev.n_p1 for lev, _ in part.levels]
        counts.append(sum(n >= DICT_MIN_ROWS for n in rows))
    assert len(set(counts)) == 1, counts
    return counts[0]


def check(c, system, relaxed, ranks_out, tag, env=None):
    """the gathered z against the definition, the launch path and the ghost rows of every rank"""
    r, z_host, d = c.reference(system, relaxed)
    bound = c.bound(system, relaxed)
    z = c.gather(system, [o[system]["z"] for o in ranks_out])
    err = mh.rel(z, z_host)
    want_lattice = lattice_levels(c, system, relaxed, env)
    o0 = ranks_out[0][system]
    print("\n[partitioned cycle] %-13s %-21s %-7s %-9s d %.1e  bound %.1e  err %.2e  lattice levels %d launches %d  "
          "exchanges %d  all-reduces %d" % (c.name, system, "relaxed" if relaxed else "exact", tag, d, bound, err,
                                             o0["info"]["lattice_levels"], o0["launches"], o0["exchanges"],
                                             o0["allreduces"]))
    assert 64.0 * d < 1e-10, (c.name, system, d)
    assert np.all(np.isfinite(z)) and err <= bound, (c.name, system, relaxed, tag, err, bound)
    velocity = system == "velocity"
    for rank, (part, out) in enumerate(zip(c.parts, ranks_out)):
        o = out[system]
        info = o["info"]
        assert info["levels"] == c.n_part + (1 if velocity else 0), (rank, info)
        assert info["lattice_levels"] == want_lattice, (c.name, system, relaxed, tag, rank, info)
        assert (o["launches"] > 0) == (want_lattice > 0), (rank, o["launches"])
        level0_rows = part.dofmap.n_p2 if velocity else part.dofmap.n_p1
        if want_lattice > 0 and level0_rows >= DICT_MIN_ROWS:
            up = 2 if velocity else 1
            want_ghost = (0 if rank == 0 else 1, 0 if rank == c.size - 1 else up)
        else:
            want_ghost = (0, 0)
        assert info["ghost_lines"] == want_ghost, (c.name, system, rank, info)
        _, owned = c.node_maps(system, part)
        nv = c.dim if velocity else 1
        assert np.all(o["z"].reshape(-1, nv)[~owned] == 0.0), "ghost rows of z are zeros"
        assert np.array_equal(o["z"], o["z_first"]), "two applications are bit-identical"
        assert (o["exchanges"], o["allreduces"]) == (o0["exchanges"], o0["allreduces"]), "every rank: same collectives"
    return z


@pytest.mark.parametrize("relaxed", [False, True], ids=["exact", "relaxed"])
@pytest.mark.parametrize("name", list(pc.CASES))
def test_partitioned_cycle_equals_the_host_definition(name, relaxed, monkeypatch):
    c = pc.case(name)
    out = results(name, relaxed, monkeypatch)
    for system in pc.SYSTEMS:
        check(c, system, relaxed, out, "default")


@pytest.mark.parametrize("name", list(pc.CASES))
def test_relaxed_cycle_exchanges_less_and_reduces_as_often(name, monkeypatch):
    exact, relaxed = results(name, False, monkeypatch), results(name, True, monkeypatch)
    for system in pc.SYSTEMS:
        e, r = exact[0][system], relaxed[0][system]
        print("\n[collectives per cycle] %-13s %-21s exchanges exact %d relaxed %d  all-reduces exact %d relaxed %d"
              % (name, system, e["exchanges"], r["exchanges"], e["allreduces"], r["allreduces"]))
        assert 0 < r["exchanges"] < e["exchanges"], (name, system, r["exchanges"], e["exchanges"])
        assert r["allreduces"] == e["allreduces"] > 0, (name, system, r["allreduces"], e["allreduces"])
        assert e["overlapped"] == r["overlapped"] == 0


@pytest.mark.parametrize("name", ["box32/2", "box64/4 tail"])
def test_relaxed_one_step_kernels_meet_the_same_definition(name, monkeypatch):
    """NSFEM_LATTICE=0 (read at creation: fresh contexts): the relaxed sequences run on the one-step kernels with
    ghost mode 1 (carry the frozen values) -- the same definition, the same bound"""
    env = {"NSFEM_LATTICE": "0"}
    c = pc.case(name)
    out = run(name, True, monkeypatch, env=env)
    for system in pc.SYSTEMS:
        check(c, system, True, out, "lattice0", env=env)


@pytest.mark.parametrize("name", ["box32/2", "box64/4 tail"])
def test_overlapped_exchanges_leave_the_exact_cycle_bit_for_bit(name, monkeypatch):
    """set_overlap(1): the exchanges run under the interior row blocks (product_with_halo) -- the same arithmetic"""
    c = pc.case(name)
    plain = results(name, False, monkeypatch)
    over = run(name, False, monkeypatch, overlap=True)
    for system in pc.SYSTEMS:
        check(c, system, False, over, "overlap")
        for a, b in zip(plain, over):
            assert np.array_equal(a[system]["z"], b[system]["z"]), (name, system)
            assert b[system]["overlapped"] > 0 and a[system]["overlapped"] == 0, (name, system, b[system]["overlapped"])
