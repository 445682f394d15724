"""Fast diagonalisation of the pressure Poisson operator on tensor-product lattices.

The reference solves the projection step (grad p, grad q) = ... with a sparse LU factorisation every step
(source/ns_ipcs_solver.py:160-171).  On the right-diagonal triangulation of a rectangle (``fem_mesh.rectangle_mesh``,
any line spacing) the P1 stiffness matrix is EXACTLY the tensor sum

    A = K_y (x) W_x + W_y (x) K_x        (node id = j (n_x + 1) + i)

of the 1D P1 stiffness matrices K and the 1D lumped (trapezoid) mass matrices W of the two line meshes -- the cross
terms of the two triangles of a cell cancel.  With the generalised eigenpairs  K v = lambda W v  (V^T W V = I) of
each direction

    A^-1 = (V_y (x) V_x) diag(1 / (lambda_y,j + lambda_x,i)) (V_y (x) V_x)^T ,

i.e. four dense products with (n + 1)-sized matrices: the direct solve the device runs in ``csrc/fastdiag.hip``
(GEMM-shaped work on the matrix cores) instead of a multigrid-preconditioned CG iteration.  Dirichlet conditions on
whole sides drop the side's line from that direction's eigenproblem; the all-Neumann operator is singular
(lambda = 0 + 0): that mode's coefficient is set to zero, the solution is the one without a constant mode in the
W (x) W inner product (pressures are compared modulo a constant, as everywhere else)."""
import numpy as np


def line_matrices(x):
    """1D P1 stiffness matrix (dense) and lumped mass (trapezoid weights) of the line mesh with nodes x"""
    x = np.asarray(x, dtype=np.float64)
    h = np.diff(x)
    assert h.size >= 1 and (h > 0.0).all()
    n = x.size
    K = np.zeros((n, n))
    idx = np.arange(n - 1)
    K[idx, idx] += 1.0 / h
    K[idx + 1, idx + 1] += 1.0 / h
    K[idx, idx + 1] -= 1.0 / h
    K[idx + 1, idx] -= 1.0 / h
    w = np.zeros(n)
    w[:-1] += 0.5 * h
    w[1:] += 0.5 * h
    return K, w


def line_eigenpairs(x, dirichlet_first=False, dirichlet_last=False):
    """(V, lam): K v = lam W v on the free nodes of the line, V^T W V = I; rows of Dirichlet end nodes are zero and
    their eigenvalue slots carry lam = inf (coefficient 0), so V stays square"""
    K, w = line_matrices(x)
    n = w.size
    free = np.ones(n, dtype=bool)
    free[0] = not dirichlet_first
    free[-1] = not dirichlet_last
    f = np.where(free)[0]
    s = 1.0 / np.sqrt(w[f])
    lam_f, Q = np.linalg.eigh(s[:, None] * K[np.ix_(f, f)] * s[None, :])
    V = np.zeros((n, n))
    lam = np.full(n, np.inf)
    V[np.ix_(f, np.arange(f.size))] = s[:, None] * Q
    lam[:f.size] = np.maximum(lam_f, 0.0)
    if not dirichlet_first and not dirichlet_last:
        lam[0] = 0.0                       # the constant: exactly singular (eigh returns ~1e-16)
    return V, lam


def side_pattern(W, H, dirichlet_nodes):
    """Is the Dirichlet node set of a W x H lattice a union of whole sides?  -> (x_first, x_last, y_first, y_last)
    flags, or None when it is not (then the fast solver does not apply)"""
    mask = np.zeros(W * H, dtype=bool)
    mask[np.asarray(dirichlet_nodes, dtype=np.int64)] = True
    m = mask.reshape(H, W)
    flags = (bool(m[:, 0].all()), bool(m[:, -1].all()), bool(m[0, :].all()), bool(m[-1, :].all()))
    want = np.zeros((H, W), dtype=bool)
    if flags[0]:
        want[:, 0] = True
    if flags[1]:
        want[:, -1] = True
    if flags[2]:
        want[0, :] = True
    if flags[3]:
        want[-1, :] = True
    return flags if np.array_equal(want, m) else None


def factors(xs, ys, dirichlet_nodes=()):
    """dict(Vx, Vy, inv) of the W x H lattice with line coordinates xs, ys, or None when the Dirichlet set is not a
    union of whole sides.  inv[j, i] = 1 / (lam_y[j] + lam_x[i]), 0 for the singular mode and the Dirichlet slots"""
    W, H = len(xs), len(ys)
    flags = side_pattern(W, H, dirichlet_nodes)
    if flags is None:
        return None
    Vx, lx = line_eigenpairs(xs, flags[0], flags[1])
    Vy, ly = line_eigenpairs(ys, flags[2], flags[3])
    s = ly[:, None] + lx[None, :]
    with np.errstate(divide="ignore"):
        inv = np.where(np.isfinite(s) & (s > 0.0), 1.0 / np.where(s > 0.0, s, 1.0), 0.0)
    scale = s[np.isfinite(s)].max()
    inv[s <= 1e-13 * scale] = 0.0          # the constant mode of the all-Neumann operator
    return dict(Vx=np.ascontiguousarray(Vx), Vy=np.ascontiguousarray(Vy), inv=np.ascontiguousarray(inv),
                singular=not any(flags))


def apply_reference(f, r):
    """z = A^+ r in numpy (the sums the device kernels compute): r, z of length W * H, node id j W + i"""
    H, W = f["inv"].shape
    R = np.asarray(r, dtype=np.float64).reshape(H, W)
    U = f["Vy"].T @ (R @ f["Vx"])
    U *= f["inv"]
    return (f["Vy"] @ (U @ f["Vx"].T)).ravel()


def lattice_lines(mesh):
    """(xs, ys) when the mesh is a rectangle_mesh lattice (vertex id = j (n_x + 1) + i, any line spacing), else None"""
    info = getattr(mesh, "structured", None)
    if info is None or len(info) != 4:
        return None
    nx, ny = int(info[2]), int(info[3])
    X = np.asarray(mesh.coords, dtype=np.float64)
    if X.shape != ((nx + 1) * (ny + 1), 2):
        return None
    G = X.reshape(ny + 1, nx + 1, 2)
    xs, ys = G[0, :, 0].copy(), G[:, 0, 1].copy()
    if not (np.abs(G[:, :, 0] - xs[None, :]).max() <= 1e-14 * max(1.0, np.abs(xs).max()) and
            np.abs(G[:, :, 1] - ys[:, None]).max() <= 1e-14 * max(1.0, np.abs(ys).max())):
        return None
    return xs, ys


# ---------------------------------------------------------------------------------------------------------------------
# 3D box lattices (fem_mesh.box_mesh: six Kuhn tetrahedra per cube around the main diagonal; csrc/fastdiag.hip).
#
# With the 1D matrices of the three line meshes, T = K_z (x) W_y (x) W_x + W_z (x) K_y (x) W_x + W_z (x) W_y (x) K_x
# equals the P1 stiffness matrix A on every row away from the box's edges when each direction is uniformly spaced (the
# cross terms of the six tetrahedra cancel there, as those of the two triangles do in 2D).  On the rows of an edge where
# two non-periodic faces meet the Kuhn split weights the couplings along the edge's axis by 2/6 or 1/6 where T puts
# 1/4: A != T.  Those rows drop out when a Dirichlet face touches the edge, so
#
#     T == A   iff   every direction is uniform and every edge between two non-periodic faces has a Dirichlet face
#                    next to it (triple-periodic, periodic in x and y with walls in z, Dirichlet on the whole boundary)
#
# and the solve z = T^+ r is then the direct projection-step solve.  Elsewhere (closed box, channel with an outlet only,
# graded lines) T^+ is a spectrally equivalent preconditioner: the generalised eigenvalues of (A, T) on the free,
# mean-free space stay in [0.798, 1.334] for uniform lines, independently of the size -- CG preconditioned by T^+ takes
# a mesh-independent ~10 iterations to 1e-10.

def periodic_line_matrices(x):
    """1D P1 stiffness (dense, circulant) and lumped mass of the periodic line with nodes x[0] ... x[nc - 1]; x[nc] is
    the periodic image of x[0] (its coordinate gives the length of the last cell)"""
    x = np.asarray(x, dtype=np.float64)
    h = np.diff(x)
    assert h.size >= 2 and (h > 0.0).all()
    nc = h.size
    K = np.zeros((nc, nc))
    a = np.arange(nc)
    b = (a + 1) % nc
    np.add.at(K, (a, a), 1.0 / h)
    np.add.at(K, (b, b), 1.0 / h)
    np.add.at(K, (a, b), -1.0 / h)
    np.add.at(K, (b, a), -1.0 / h)
    w = 0.5 * (h + np.roll(h, 1))
    return K, w


def periodic_line_eigenpairs(x):
    """(V, lam): K v = lam W v on the periodic line (nc = len(x) - 1 nodes), V^T W V = I; lam[0] = 0 is the constant"""
    K, w = periodic_line_matrices(x)
    s = 1.0 / np.sqrt(w)
    lam, Q = np.linalg.eigh(s[:, None] * K * s[None, :])
    lam = np.maximum(lam, 0.0)
    lam[0] = 0.0                           # the constant: exactly singular (eigh returns ~1e-16)
    return np.ascontiguousarray(s[:, None] * Q), lam


def box_lattice(mesh, dofmap):
    """(xs, ys, zs, (px, py, pz)) when the mesh is a box_mesh lattice (any line spacing) whose P1 nodes are numbered
    lexicographically, x fastest, on the lattice that remains after the periodic identifications; else None.  xs etc.
    hold all n_d + 1 line coordinates; a direction is periodic when the dof map puts the node at i_d = n_d on the node
    at i_d = 0 everywhere.  The P1 nodes then number (N_z x N_y x N_x), N_d = n_d (periodic) or n_d + 1."""
    info = getattr(mesh, "structured", None)
    if info is None or len(info) != 5:
        return None
    nx, ny, nz = int(info[2]), int(info[3]), int(info[4])
    X = np.asarray(mesh.coords, dtype=np.float64)
    if X.shape != ((nx + 1) * (ny + 1) * (nz + 1), 3):
        return None
    G = X.reshape(nz + 1, ny + 1, nx + 1, 3)
    xs, ys, zs = G[0, 0, :, 0].copy(), G[0, :, 0, 1].copy(), G[:, 0, 0, 2].copy()
    for a, line, shape in ((0, xs, (1, 1, nx + 1)), (1, ys, (1, ny + 1, 1)), (2, zs, (nz + 1, 1, 1))):
        if np.abs(G[..., a] - line.reshape(shape)).max() > 1e-14 * max(1.0, np.abs(line).max()):
            return None
    P = np.asarray(dofmap.p1_vertex_node, dtype=np.int64)
    if P.shape != (X.shape[0],):
        return None
    P = P.reshape(nz + 1, ny + 1, nx + 1)
    per = (bool(np.array_equal(P[:, :, -1], P[:, :, 0])), bool(np.array_equal(P[:, -1, :], P[:, 0, :])),
           bool(np.array_equal(P[-1, :, :], P[0, :, :])))
    n = (nx, ny, nz)
    N = [n[a] if per[a] else n[a] + 1 for a in range(3)]
    k, j, i = np.meshgrid(np.arange(nz + 1), np.arange(ny + 1), np.arange(nx + 1), indexing="ij")
    lex = ((k % N[2]) * N[1] + (j % N[1])) * N[0] + (i % N[0])
    if int(dofmap.n_p1) != N[0] * N[1] * N[2] or not np.array_equal(P, lex):
        return None
    return xs, ys, zs, per


def face_pattern(shape, periodic, dirichlet_nodes):
    """Is the Dirichlet node set of an (N_z x N_y x N_x) lattice, shape = (N_x, N_y, N_z), a union of whole faces?
    -> (x_first, x_last, y_first, y_last, z_first, z_last) flags, or None when it is not.  Periodic directions have
    no faces (their flags are False)."""
    Nx, Ny, Nz = shape
    mask = np.zeros(Nx * Ny * Nz, dtype=bool)
    mask[np.asarray(dirichlet_nodes, dtype=np.int64)] = True
    m = mask.reshape(Nz, Ny, Nx)
    faces = ((np.s_[:, :, 0], np.s_[:, :, -1]), (np.s_[:, 0, :], np.s_[:, -1, :]), (np.s_[0, :, :], np.s_[-1, :, :]))
    flags = []
    want = np.zeros_like(m)
    for a in range(3):
        for sl in faces[a]:
            on = not periodic[a] and bool(m[sl].all())
            flags.append(on)
            if on:
                want[sl] = True
    return tuple(flags) if np.array_equal(want, m) else None


def _uniform(x):
    h = np.diff(np.asarray(x, dtype=np.float64))
    return bool(np.abs(h - h[0]).max() <= 1e-12 * np.abs(h).max())


def factors_3d(xs, ys, zs, periodic=(False, False, False), dirichlet_nodes=()):
    """dict(Vx, Vy, Vz, inv, singular, exact) of the box lattice with line coordinates xs, ys, zs (all n_d + 1 of them,
    periodic directions included), or None when the Dirichlet set is not a union of whole faces.
    inv[k, j, i] = 1 / (lam_z[k] + lam_y[j] + lam_x[i]), 0 for the singular mode and the Dirichlet slots.
    exact: T^+ is the inverse of the P1 stiffness matrix (module comment above); otherwise it is a preconditioner."""
    lines = (xs, ys, zs)
    shape = tuple(len(l) - 1 if periodic[a] else len(l) for a, l in enumerate(lines))
    flags = face_pattern(shape, periodic, dirichlet_nodes)
    if flags is None:
        return None
    V, lam = [], []
    for a in range(3):
        v, l = (periodic_line_eigenpairs(lines[a]) if periodic[a] else
                line_eigenpairs(lines[a], flags[2 * a], flags[2 * a + 1]))
        V.append(np.ascontiguousarray(v))
        lam.append(l)
    s = lam[2][:, None, None] + lam[1][None, :, None] + lam[0][None, None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = np.where(np.isfinite(s) & (s > 0.0), 1.0 / np.where(s > 0.0, s, 1.0), 0.0)
    scale = s[np.isfinite(s)].max()
    inv[s <= 1e-13 * scale] = 0.0          # the constant mode of the all-Neumann operator
    exact = all(_uniform(l) for l in lines)
    for a in range(3):                     # the 12 edges: axis a, the other two directions b < c at an end each
        b, c = [d for d in range(3) if d != a]
        if periodic[b] or periodic[c]:
            continue
        for eb in range(2):
            for ec in range(2):
                if not (flags[2 * b + eb] or flags[2 * c + ec]):
                    exact = False
    return dict(Vx=V[0], Vy=V[1], Vz=V[2], inv=np.ascontiguousarray(inv), singular=not any(flags), exact=exact)


def apply_reference_3d(f, r):
    """z = T^+ r in numpy (the six mode products the device kernels compute): r, z of length N_z N_y N_x, node id
    (k N_y + j) N_x + i"""
    Nz, Ny, Nx = f["inv"].shape
    R = np.asarray(r, dtype=np.float64).reshape(Nz, Ny, Nx)
    U = R @ f["Vx"]                                                   # x
    U = np.matmul(f["Vy"].T, U)                                       # y (every z-plane)
    U = (f["Vz"].T @ U.reshape(Nz, Ny * Nx)).reshape(Nz, Ny, Nx)      # z
    U *= f["inv"]
    U = (f["Vz"] @ U.reshape(Nz, Ny * Nx)).reshape(Nz, Ny, Nx)
    U = np.matmul(f["Vy"], U)
    return (U @ f["Vx"].T).ravel()
