"""Problems, states and coefficient sets shared by tests/test_monolithic_host.py (host only) and
tests/test_gpu_monolithic_linear.py (device against host): inputs and cached host references, no algorithm.

Problems -- the smallest at which each launch path of the monolithic linear solve exists:
    box16      closed cavity 16 x 16 (levels 16, 8, 4, 2): singular Schur level, the pressure hierarchy all CSR
    box96x40   96 x 40 cells of side 1/32: lattice levels and fused transfers in mg_s, mg_m on the lattice kernel
    box48      h = 1/48: inexact dictionaries; the block dictionaries serve D / D^T
    box32x4    the channel of test_bdf_monolithic_open_channel_and_stokes_limit (8 x 1, parabolic inlet, natural
               outlet whose nodes are the PRESSURE_PRECOND set); geometric and algebraic Schur operators
    cube4      3D, nv = 3
    dfg        unstructured refinement hierarchy, algebraic Schur levels
States: `rest` (zero fields; the Newton residual lives on the Dirichlet rows) and `developed` (the smooth fields of
tests/test_gpu_krylov_iterates.py: U0 <- its u*, U1, U2, P), BDF2, nu = 0.01.

A case fixes everything the linear algebra depends on: problem, state, step size, (c_c, c_p, c_v), prec_shift, the
pressure Dirichlet set of the system, the PRESSURE_PRECOND set, geometric / algebraic Schur operators.  `pinned` cases
put the pressure Dirichlet set on the side x = x_max and leave PRESSURE_PRECOND empty, the channel does the opposite:
in no case are the two sets equal unless both are empty.  Step sizes: 0.01, except where the BiCGStab iterate tests
need another one to keep three iterates per schedule under the rule of tests/test_gpu_krylov_iterates.py (chosen on
the host alone): 0.002 for the shifted cavity and the `short step` channel, 0.05 for the cube at rest."""
import numpy as np

import krylov_host as kh
import mg_cycle_host as mh
import monolithic_host as mo
import test_gpu_krylov_iterates as gki
import test_gpu_multigrid_cycle as mgc

NU, BDF2 = mgc.NU, mgc.BDF2
NO_DOFS = mgc.NO_DOFS


def _channel():
    from gpu_common import box, velocity_bc
    from multigrid import structured_hierarchy
    p1 = (8.0, 1.0)
    mesh, dm, marks = box(32, 4, p1)
    mesh.structured = ((0.0, 0.0), p1, 32, 4)
    levels = structured_hierarchy((0.0, 0.0), p1, 32, 4, coarsest=2)
    zero = lambda X: np.zeros((X.shape[0], 2))
    inlet = lambda X: np.stack([6.0 * X[:, 1] * (1.0 - X[:, 1]), 0.0 * X[:, 1]], axis=1)
    vel = velocity_bc(dm, marks, [(1, inlet), (3, zero), (4, zero)])
    outlet = np.unique(dm.facet_p1_nodes(marks.facets_with_id(2)))
    return mgc.Problem(mesh, dm, levels, vel, outlet)


_MAKERS = {"box16": mgc._MAKERS["box16"], "box96x40": mgc._MAKERS["box96x40"], "box48": mgc._MAKERS["box48"],
           "box32x4": _channel, "cube4": lambda: mgc._cube(4), "dfg": mgc._dfg}
_problems, _refs = {}, {}


def problem(name):
    if name not in _problems:
        _problems[name] = mgc.problem(name) if name in ("box16", "box96x40", "box48") else _MAKERS[name]()
        _problems[name].name = name
    return _problems[name]


class Case:
    def __init__(self, pname, state, k=0.01, cc=1.0, cp=1.0, cv=NU, shift=0.0, pres="none", schur="none",
                 algebraic=False):
        self.pname, self.state, self.k, self.cc, self.cp, self.cv, self.shift = pname, state, k, cc, cp, cv, shift
        self.pres, self.schur, self.algebraic = pres, schur, algebraic

    def sets(self, pb):
        pick = lambda which: pb.outlet if which == "outlet" else NO_DOFS
        return pick(self.pres), pick(self.schur)


SHIFT = 40.0
CASES = {
    "box16 rest": Case("box16", "rest"),
    "box16 developed": Case("box16", "developed"),
    "box16 developed scaled shifted pinned": Case("box16", "developed", cp=1.7, cv=0.03, shift=SHIFT, pres="outlet"),
    "box16 developed shifted": Case("box16", "developed", k=0.002, shift=SHIFT),
    "box16 developed scaled pinned": Case("box16", "developed", cp=1.7, cv=0.03, pres="outlet"),
    "box96x40 developed": Case("box96x40", "developed"),
    "box96x40 developed pinned": Case("box96x40", "developed", cp=0.6, cv=0.02, pres="outlet"),
    "box48 developed": Case("box48", "developed"),
    "box48 developed pinned": Case("box48", "developed", cp=1.3, cv=0.004, pres="outlet"),
    "box32x4 rest geometric": Case("box32x4", "rest", cv=0.1, schur="outlet"),
    "box32x4 rest algebraic": Case("box32x4", "rest", cv=0.1, algebraic=True),
    "box32x4 developed geometric": Case("box32x4", "developed", schur="outlet"),
    "box32x4 developed algebraic": Case("box32x4", "developed", algebraic=True),
    "box32x4 developed algebraic short step": Case("box32x4", "developed", k=0.002, algebraic=True),
    "cube4 rest": Case("cube4", "rest", k=0.05),
    "cube4 developed": Case("cube4", "developed", cp=0.8, cv=0.05, pres="outlet"),
    "dfg developed algebraic": Case("dfg", "developed", algebraic=True),
}


def state_fields(pb, state):
    """slot values of the monolithic step: U0 (the linearisation point), U1, U2, P"""
    import _native as nat
    f = gki.fields(pb, state)
    return {nat.U0: f[nat.USTAR], nat.U1: f[nat.U1], nat.U2: f[nat.U2], nat.P: f[nat.P]}


def seeded(name, tag, n):
    seed = sum(ord(ch) * (i + 1) for i, ch in enumerate(name)) * 16 + {"x": 1, "r": 2, "s": 3, "m": 4, "x2": 5}[tag]
    return np.random.default_rng(seed).standard_normal(n)


class Reference:
    """host objects of one case, each built on first use and kept"""

    def __init__(self, name):
        self.name, self.c = name, CASES[name]
        self.pb = problem(self.c.pname)
        self.pres, self.schur = self.c.sets(self.pb)
        self._cache = {}

    def _get(self, key, make):
        if key not in self._cache:
            self._cache[key] = make()
        return self._cache[key]

    def u0(self):
        import _native as nat
        return state_fields(self.pb, self.c.state)[nat.U0]

    def matrix(self, dtype=np.float64, form=0, picard=False, cc="case"):
        c, pb = self.c, self.pb
        cc = c.cc if cc == "case" else cc
        return self._get(("A", dtype, form, picard, cc), lambda: mo.mixed_matrix(
            pb.H, self.u0(), BDF2[0] / c.k, c.cv, cc, c.cp, pb.vel[0], self.pres, form, picard, dtype))

    def prec(self, dtype=np.float64, **kw):
        c, pb = self.c, self.pb
        key = ("P", dtype) + tuple(sorted(kw.items()))
        return self._get(key, lambda: mo.BlockPreconditioner(
            pb.H, BDF2[0], c.k, c.cv, c.cp, pb.vel[0], self.pres, self.schur, prec_shift=c.shift, degree=pb.degree,
            eig_ratio=pb.eig_ratio, algebraic=c.algebraic, dtype=dtype, **kw))

    def schur_cycle(self, dtype=np.float64):
        return self.prec(dtype).S

    def rhs(self):
        """the Newton residual of nsfem_step_bdf at the state (bdf_residual): the right-hand side of its linear solve"""
        import _native as nat
        c, pb = self.c, self.pb

        def make():
            f = state_fields(pb, c.state)
            return mo.residual(pb.H, f[nat.U0], f[nat.P], f[nat.U1], f[nat.U2], BDF2, c.k, c.cv, c.cc, c.cp, pb.vel,
                               (self.pres, np.zeros(len(self.pres))))
        return self._get("b", make)

    def history(self, kmax, dtype=np.float64):
        b = self.rhs()
        return self._get(("h", kmax, dtype), lambda: kh.bicgstab(self.matrix(dtype), b, np.zeros_like(b),
                                                                  self.prec(dtype).apply, kmax))

    def count(self, rtol=1e-10, kmax=40):
        """iterations of the host BiCGStab until the recurrence residual is <= rtol |b|"""
        h = self.history(kmax)
        res = np.array([float(r) for r in h.res[1:]])
        hit = np.nonzero(res <= rtol * float(h.bnorm))[0]
        return int(hit[0]) + 1 if hit.size else None


def reference(name):
    if name not in _refs:
        _refs[name] = Reference(name)
    return _refs[name]


# BiCGStab iterations of the host restatement down to 1e-10 |b| (right-hand side: the Newton residual at the state),
# recorded by tests/test_monolithic_host.py::test_host_bicgstab_reaches_1e_10_in_the_recorded_count
HOST_COUNTS = {
    "box16 rest": 9, "box16 developed": 13, "box16 developed shifted": 10,
    "box32x4 developed algebraic short step": 9, "box16 developed scaled shifted pinned": 19,
    "box16 developed scaled pinned": 22, "box96x40 developed": 20, "box96x40 developed pinned": 30,
    "box48 developed": 20, "box48 developed pinned": 32, "box32x4 rest geometric": 18, "box32x4 rest algebraic": 9,
    "box32x4 developed geometric": 36, "box32x4 developed algebraic": 14, "cube4 rest": 18, "cube4 developed": 23,
    "dfg developed algebraic": 23,
}
