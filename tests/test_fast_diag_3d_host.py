"""Host side of the 3D fast diagonalisation (poisson_fd.factors_3d / box_lattice / apply_reference_3d): on box_mesh
lattices (six Kuhn tetrahedra per cube) the tensor sum T of the 1D stiffness and lumped mass matrices inverts the
oracle's P1 stiffness matrix A exactly where the `exact` flag says so -- triple-periodic, periodic in x and y with
walls in z, Dirichlet on the whole boundary -- and is a spectrally equivalent preconditioner where it does not (closed
box, outlet-only channel, graded lines)."""
import numpy as np
import pytest

import dlfn_compat as dlfn
import fem_oracle as fo
import poisson_fd as pf
from fem_mesh import TaylorHoodDofMap, box_mesh, periodic_entity_map, preferred_p2_order, rectangle_mesh


class _BoxPeriodic(dlfn.SubDomain):
    """periodic identification of the faces x_a = L_a with x_a = 0 for the axes given"""

    def __init__(self, axes, lengths):
        super().__init__()
        self.axes, self.lengths = tuple(axes), tuple(lengths)

    def inside(self, x, on_boundary):
        return bool(on_boundary and any(dlfn.near(x[a], 0.0) for a in self.axes))

    def map(self, x_slave, x_master):
        for a in self.axes:
            if dlfn.near(x_slave[a], self.lengths[a]):
                x_master[:] = x_slave
                x_master[a] -= self.lengths[a]
                return
        x_master[:] = -10.0


def _box(n, lengths, periodic_axes=(), grading=None):
    """box_mesh lattice, its dof map (periodic identifications on the given axes) and the lattice description.
    grading: per axis None or a map [0, 1] -> [0, 1] applied to the line coordinates"""
    mesh = box_mesh((0.0, 0.0, 0.0), lengths, *n)
    if grading is not None:
        X = mesh.coords
        for a, g in enumerate(grading):
            if g is not None:
                X[:, a] = lengths[a] * g(X[:, a] / lengths[a])
    pm = periodic_entity_map(mesh, _BoxPeriodic(periodic_axes, lengths)) if periodic_axes else None
    dm = TaylorHoodDofMap(mesh, reorder=preferred_p2_order(3), periodic_map=pm)
    return mesh, dm


def _face_nodes(dm, lengths, faces):
    """P1 nodes on the faces (axis, 0 | 1)"""
    X = dm.p1_coords
    d = [np.nonzero(np.abs(X[:, a] - (0.0 if e == 0 else lengths[a])) < 1e-12)[0] for a, e in faces]
    return np.unique(np.concatenate(d)) if d else np.zeros(0, dtype=np.int64)


def _setup(n, lengths, periodic_axes=(), faces=(), grading=None):
    mesh, dm = _box(n, lengths, periodic_axes, grading)
    lattice = pf.box_lattice(mesh, dm)
    assert lattice is not None
    xs, ys, zs, per = lattice
    assert per == tuple(a in periodic_axes for a in range(3))
    d = _face_nodes(dm, lengths, faces)
    f = pf.factors_3d(xs, ys, zs, per, d)
    assert f is not None
    A = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap).stiffness_p1().toarray()
    free = np.setdiff1d(np.arange(dm.n_p1), d)
    return f, A[np.ix_(free, free)], free, dm.n_p1


def _tplus(f, free, n_p1):
    """T^+ restricted to the free nodes, column by column through apply_reference_3d"""
    E = np.zeros((n_p1, free.size))
    E[free, np.arange(free.size)] = 1.0
    return np.stack([pf.apply_reference_3d(f, E[:, c]) for c in range(free.size)], axis=1)[free]


def _pencil_eigenvalues(f, Af, free, n_p1):
    """eigenvalues of T^+ A on the free space (all-Neumann: the zero of the constant dropped)"""
    ev = np.sort(np.linalg.eigvals(_tplus(f, free, n_p1) @ Af).real)
    return ev[1:] if f["singular"] else ev


EXACT = [
    ("triple-periodic", (4, 4, 4), (1.0, 1.0, 1.0), (0, 1, 2), ()),
    ("triple-periodic-ragged", (4, 6, 3), (1.0, 1.4, 0.6), (0, 1, 2), ()),
    ("xy-periodic-z-walls", (4, 5, 3), (1.0, 1.3, 0.7), (0, 1), ()),
    ("x-periodic-z-dirichlet", (4, 5, 3), (1.0, 1.3, 0.7), (0,), ((2, 0), (2, 1))),
    ("all-dirichlet", (4, 5, 3), (1.0, 1.3, 0.7), (), tuple((a, e) for a in range(3) for e in range(2))),
    ("all-dirichlet-cube", (5, 5, 5), (1.0, 1.0, 1.0), (), tuple((a, e) for a in range(3) for e in range(2))),
    ("four-dirichlet-faces", (3, 4, 5), (0.8, 1.0, 1.2), (), ((0, 0), (0, 1), (1, 0), (1, 1))),
]


@pytest.mark.parametrize("name,n,lengths,periodic_axes,faces", EXACT, ids=[c[0] for c in EXACT])
def test_exact_factors_invert_the_oracle_stiffness(name, n, lengths, periodic_axes, faces):
    """exact cases: T^+ A = I on the free space (all-Neumann: on the mean-free space) to 1e-12"""
    f, Af, free, n_p1 = _setup(n, lengths, periodic_axes, faces)
    assert f["exact"]
    assert f["singular"] == (len(faces) == 0)
    Z = _tplus(f, free, n_p1)
    I = np.eye(free.size)
    if f["singular"]:
        P = I - 1.0 / free.size
        err = np.abs(P @ (Af @ Z) @ P - P).max()
    else:
        err = np.abs(Af @ Z - I).max()
    assert err < 1e-12, err


INEXACT = [
    ("closed-box", (6, 6, 6), (1.0, 1.0, 1.0), (), ()),
    ("closed-box-ragged", (4, 5, 3), (1.0, 1.3, 0.7), (), ()),
    ("outlet-only", (8, 4, 4), (2.0, 1.0, 1.0), (), ((0, 1),)),
    ("x-periodic-closed", (4, 5, 3), (1.0, 1.3, 0.7), (0,), ()),
    ("dirichlet-x-faces-only", (4, 4, 4), (1.0, 1.0, 1.0), (), ((0, 0), (0, 1))),
]


@pytest.mark.parametrize("name,n,lengths,periodic_axes,faces", INEXACT, ids=[c[0] for c in INEXACT])
def test_inexact_factors_are_flagged_and_spectrally_equivalent(name, n, lengths, periodic_axes, faces):
    """free box edges (two non-periodic faces meeting, neither Dirichlet): exact is False, A != T, and the eigenvalues
    of (A, T) on the free (mean-free) space lie in [0.75, 1.4]"""
    f, Af, free, n_p1 = _setup(n, lengths, periodic_axes, faces)
    assert not f["exact"]
    Z = _tplus(f, free, n_p1)
    assert np.abs(Af @ Z - np.eye(free.size)).max() > 0.1
    ev = _pencil_eigenvalues(f, Af, free, n_p1)
    assert ev.min() > 0.75 and ev.max() < 1.4, (ev.min(), ev.max())


def _tensor_sum(xs, ys, zs):
    """T = K_z (x) W_y (x) W_x + W_z (x) K_y (x) W_x + W_z (x) W_y (x) K_x, dense, from poisson_fd.line_matrices"""
    (Kx, wx), (Ky, wy), (Kz, wz) = (pf.line_matrices(l) for l in (xs, ys, zs))
    Wx, Wy, Wz = np.diag(wx), np.diag(wy), np.diag(wz)
    return np.kron(Kz, np.kron(Wy, Wx)) + np.kron(Wz, np.kron(Ky, Wx)) + np.kron(Wz, np.kron(Wy, Kx))


def _pencil_range(lengths, n, outlet):
    """extreme generalised eigenvalues of (A, T): on the free nodes (outlet: Dirichlet on x = L_x), closed box on the
    mean-free space (an orthonormal basis of the complement of the constant)"""
    import scipy.linalg as sla
    mesh = box_mesh((0.0, 0.0, 0.0), lengths, *n)
    dm = TaylorHoodDofMap(mesh)
    A = fo.Space(mesh.coords, mesh.cells, dm.p2_dofmap, dm.p1_dofmap).stiffness_p1().toarray()
    xs, ys, zs, _ = pf.box_lattice(mesh, dm)
    T = _tensor_sum(xs, ys, zs)
    N = A.shape[0]
    if outlet:
        free = _face_nodes(dm, lengths, ((0, 1),))
        free = np.setdiff1d(np.arange(N), free)
        ev = sla.eigh(A[np.ix_(free, free)], T[np.ix_(free, free)], eigvals_only=True)
    else:
        Q, _ = np.linalg.qr(np.hstack([np.ones((N, 1)), np.eye(N)[:, :N - 1]]))
        Q = Q[:, 1:]
        ev = sla.eigh(Q.T @ A @ Q, Q.T @ T @ Q, eigvals_only=True)
    return ev.min(), ev.max()


@pytest.mark.parametrize("outlet,sizes", [(False, (6, 10, 14)), (True, (4, 8, 10))], ids=["closed-box", "outlet-only"])
def test_pencil_bounds_are_the_same_at_every_size(outlet, sizes):
    """uniform lines with free edges: the eigenvalues of (A, T) lie in [0.798, 1.334] at every size -- the closed unit
    cube at n = 6, 10, 14, the 2 x 1 x 1 outlet-only channel at (2n, n, n), n = 4, 8, 10 -- and the extremes agree
    to 1e-3 across the sizes: preconditioned CG takes a mesh-independent number of iterations"""
    lengths = (2.0, 1.0, 1.0) if outlet else (1.0, 1.0, 1.0)
    out = [_pencil_range(lengths, (2 * n, n, n) if outlet else (n, n, n), outlet) for n in sizes]
    for lo, hi in out:
        assert 0.798 < lo and hi < 1.334, out
    assert np.ptp([o[0] for o in out]) < 1e-3 and np.ptp([o[1] for o in out]) < 1e-3, out


def _cosine(t):
    return 0.5 * (1.0 - np.cos(np.pi * t))


def test_graded_lines_are_inexact_but_precondition_well():
    """graded lines: T != A even on interior rows, so exact is False even where every edge is Dirichlet; the
    eigenvalues of (A, T) stay near 1 (cosine grading in x: within [0.9, 1.1]).  Graded lines combined with free
    edges: only recorded (positive, finite), no bound is asserted."""
    grading = (_cosine, None, None)
    faces = tuple((a, e) for a in range(3) for e in range(2))
    f, Af, free, n_p1 = _setup((6, 5, 4), (1.0, 1.0, 1.0), faces=faces, grading=grading)
    assert not f["exact"]
    ev = _pencil_eigenvalues(f, Af, free, n_p1)
    assert ev.min() > 0.9 and ev.max() < 1.1, (ev.min(), ev.max())
    f, Af, free, n_p1 = _setup((6, 5, 4), (1.0, 1.0, 1.0), grading=grading)
    assert not f["exact"]
    ev = _pencil_eigenvalues(f, Af, free, n_p1)
    assert np.isfinite(ev).all() and ev.min() > 0.0
    print("graded x, closed box: eigenvalues of (A, T) in [%.3f, %.3f]" % (ev.min(), ev.max()))


def test_box_lattice_refuses_non_lattices_and_wrong_numberings():
    mesh, dm = _box((3, 4, 2), (1.0, 1.0, 1.0))
    assert pf.box_lattice(mesh, dm) is not None
    # a 2D rectangle lattice
    m2 = rectangle_mesh((0.0, 0.0), (1.0, 1.0), 3, 3)
    assert pf.box_lattice(m2, TaylorHoodDofMap(m2)) is None
    # an unstructured mesh (no lattice description)
    saved = mesh.structured
    mesh.structured = None
    assert pf.box_lattice(mesh, dm) is None
    mesh.structured = saved
    # a vertex moved off its lattice line
    X0 = mesh.coords.copy()
    mesh.coords[7, 1] += 0.01
    assert pf.box_lattice(mesh, dm) is None
    mesh.coords[:] = X0

    # P1 numbering that is not lexicographic: swap two node ids
    class _Swapped:
        n_p1 = dm.n_p1
        p1_vertex_node = dm.p1_vertex_node.copy()
    _Swapped.p1_vertex_node[[0, 5]] = _Swapped.p1_vertex_node[[5, 0]]
    assert pf.box_lattice(mesh, _Swapped) is None

    # a dof map that belongs to another lattice
    other_mesh, other = _box((4, 4, 2), (1.0, 1.0, 1.0))
    assert pf.box_lattice(mesh, other) is None
    assert pf.box_lattice(other_mesh, other) is not None


def test_periodic_numbering_is_lexicographic_on_the_reduced_lattice():
    """triple-periodic n = 4 with the production P2 order: P1 nodes number the 4^3 lattice x fastest"""
    mesh, dm = _box((4, 4, 4), (1.0, 1.0, 1.0), (0, 1, 2))
    xs, ys, zs, per = pf.box_lattice(mesh, dm)
    assert per == (True, True, True) and dm.n_p1 == 64
    k, j, i = np.meshgrid(np.arange(4), np.arange(4), np.arange(4), indexing="ij")
    X = np.stack([xs[i.ravel()], ys[j.ravel()], zs[k.ravel()]], axis=1)
    assert np.abs(dm.p1_coords - X).max() < 1e-14
    mesh, dm = _box((3, 4, 5), (1.0, 1.0, 1.0), (0, 1))
    assert pf.box_lattice(mesh, dm)[3] == (True, True, False) and dm.n_p1 == 3 * 4 * 6


def test_face_pattern_needs_whole_faces():
    shape = (4, 3, 5)
    m = np.zeros((5, 3, 4), dtype=bool)
    m[:, :, 0] = True
    m[0, :, :] = True
    ids = np.nonzero(m.ravel())[0]
    assert pf.face_pattern(shape, (False,) * 3, ids) == (True, False, False, False, True, False)
    assert pf.face_pattern(shape, (False,) * 3, ids[:-1]) is None
    assert pf.face_pattern(shape, (False,) * 3, []) == (False,) * 6
    # periodic directions have no faces: a full x = 0 plane is then not a face
    assert pf.face_pattern(shape, (True, False, False), np.nonzero(m.reshape(5, 3, 4)[:, :, 0].ravel())[0]) is None
    assert pf.factors_3d(np.linspace(0, 1, 4), np.linspace(0, 1, 3), np.linspace(0, 1, 5), (False,) * 3,
                         ids[:-1]) is None


@pytest.mark.parametrize("nc", [2, 3, 8, 17])
def test_periodic_line_factors(nc):
    """V^T W V = I, K V = W V diag(lam), one zero eigenvalue (the constant), on uniform and graded periodic lines"""
    for x in (np.linspace(0.0, 1.0, nc + 1), _cosine(np.linspace(0.0, 1.0, nc + 1)) * 2.0):
        K, w = pf.periodic_line_matrices(x)
        assert np.allclose(K, K.T) and np.abs(K.sum(axis=1)).max() < 1e-12 * np.abs(K).max()
        assert abs(w.sum() - (x[-1] - x[0])) < 1e-14
        V, lam = pf.periodic_line_eigenpairs(x)
        assert np.abs(V.T @ (w[:, None] * V) - np.eye(nc)).max() < 1e-12
        assert np.abs(K @ V - (w[:, None] * V) * lam[None, :]).max() < 1e-11 * max(1.0, lam.max())
        assert lam[0] == 0.0 and (lam[1:] > 1e-8).all()
        assert np.ptp(V[:, 0]) < 1e-12                                  # the constant


def test_apply_reference_3d_is_the_kronecker_formula():
    """apply_reference_3d with arbitrary non-symmetric factors against (Vz (x) Vy (x) Vx) diag(inv) (...)^T"""
    rng = np.random.default_rng(3)
    Nx, Ny, Nz = 4, 3, 5
    f = dict(Vx=rng.standard_normal((Nx, Nx)), Vy=rng.standard_normal((Ny, Ny)), Vz=rng.standard_normal((Nz, Nz)),
             inv=rng.uniform(0.5, 1.5, (Nz, Ny, Nx)))
    V = np.kron(f["Vz"], np.kron(f["Vy"], f["Vx"]))
    r = rng.standard_normal(Nx * Ny * Nz)
    ref = V @ (f["inv"].ravel() * (V.T @ r))
    assert np.abs(pf.apply_reference_3d(f, r) - ref).max() < 1e-12 * np.abs(ref).max()
