"""Energy spectra of device-resident solutions on box lattices (csrc/spectrum.hip).

The wavenumber spectrum ``E(k)`` of a fully periodic box -- what a Taylor-Green or a decaying-turbulence run is judged
on -- and the one-dimensional spectra ``E(k_x; y)`` of a channel.  The reference has nothing like it; its drivers would
copy the solution to the host and run ``numpy.fft.fftn`` plus a binning loop per sample.

On a box mesh the P2 nodes (vertices and edge midpoints) occupy every point of the half-spacing lattice exactly once,
the P1 nodes every point of the vertex lattice, so the nodal values are a regular sample: ``2 n_a`` (P1: ``n_a``) points
along a periodic axis, one more along a walled one.  The device part is generic -- a dense matrix along every
transformed axis (on the matrix cores), then sums of squares over bins of lattice points; this module decides what the
matrices and the bins are.

* ``fourier_basis(n)``: the real orthonormal Fourier basis.  Row 0 is constant, then cos / sin pairs, then the
  alternating row when ``n`` is even.  The squares of the cos and sin coefficients of wavenumber ``k`` add up to
  ``n (|u^_k|^2 + |u^_-k|^2)`` (``u^`` the normalised DFT), so no complex arithmetic is needed; in ``d`` dimensions the
  sum over the ``2^d`` cos / sin products is the energy of all sign combinations of ``(k_x, k_y, k_z)``.
* ``lattice_of_nodes(mesh, dofmap, field)``: the lattice of a field's nodes.
* ``shell_bins(lattice)``: fully periodic boxes, bin ``rint(|kappa| / dkappa)`` with
  ``kappa = 2 pi (k_x / L_x, k_y / L_y, k_z / L_z)`` and ``dkappa = 2 pi / max L`` (integer shells on a cube).
* ``axis_bins(axis, lattice)``: only ``axis`` (periodic) is transformed; a bin is (the indices along the walled axes,
  ``|k_axis|``); the other periodic axes are summed in physical space, which by Parseval equals summing their modes.
* ``EnergySpectrum``: the plan in a solver's device context, one-shot ``compute()`` and a running time mean.

Normalisation: ``E = 1/2 sum_c sum c^2 / n_points`` for the velocity (no 1/2 for a scalar), so ``sum_b E[b]`` is
``1/2 <|u|^2>`` over the lattice points.  This is the DISCRETE NODAL energy -- the mean over the nodes of the nodal
values -- not the finite-element integral ``1/2 int |u_h|^2`` of ``ProblemBase._compute_flow_diagnostics``; the two
agree up to the quadrature error of the nodal mean, O(h^2) for a smooth field.

Out of scope: partitioned meshes (the device refuses them), co-spectra, sine / cosine transforms for walled
directions (the device takes any matrix: host work), unstructured meshes.
"""
from collections import namedtuple

import numpy as np

import _native as nat

Lattice = namedtuple("Lattice", "shape node_of_point periodic lengths origin")
Bins = namedtuple("Bins", "matrices bin_ptr bin_points k walls bin_shape points_per_wall")

FIELDS = {"velocity": nat.U0, "temperature": nat.T0, "pressure": nat.P}


def fourier_basis(n):
    """(F [n, n], wavenumber_of_row [n]): the real orthonormal Fourier basis of ``n`` equispaced points -- row 0
    ``1 / sqrt(n)``, rows ``2 k - 1``, ``2 k`` ``sqrt(2 / n) cos / sin(2 pi k j / n)`` for ``1 <= k < n / 2``, and for
    even ``n`` the last row ``(-1)^j / sqrt(n)`` (wavenumber ``n / 2``); ``F F^T = 1``"""
    n = int(n)
    assert n >= 1
    j = np.arange(n)
    F = np.empty((n, n))
    k_of = np.zeros(n, dtype=np.int64)
    F[0] = 1.0 / np.sqrt(n)
    row = 1
    for k in range(1, (n - 1) // 2 + 1):
        # (the angle from the integer k j mod n: no error growth with k j)
        ang = 2.0 * np.pi * ((k * j) % n) / n
        F[row] = np.sqrt(2.0 / n) * np.cos(ang)
        F[row + 1] = np.sqrt(2.0 / n) * np.sin(ang)
        k_of[row] = k_of[row + 1] = k
        row += 2
    if n % 2 == 0 and n >= 2:
        F[row] = np.where(j % 2 == 0, 1.0, -1.0) / np.sqrt(n)
        k_of[row] = n // 2
    return F, k_of


def lattice_of_nodes(mesh, dofmap, field="velocity"):
    """``Lattice(shape, node_of_point, periodic, lengths, origin)`` of the nodes of ``field`` ("velocity" and
    "temperature": P2 nodes, "pressure": P1 nodes) on a box mesh: ``shape`` = points per axis (x first),
    ``node_of_point`` [prod(shape)] with x fastest, ``periodic`` one flag per axis.  An axis is periodic when it carries
    ``m n_a`` distinct positions (``m`` = 2 for P2, 1 for P1, ``n_a`` cells) and walled when it carries one more.
    ValueError on meshes without ``structured`` or when a lattice point is missing or doubled."""
    lat = getattr(mesh, "structured", None)
    if lat is None:
        raise ValueError("energy spectrum: the mesh has no box lattice (mesh.structured)")
    if field not in FIELDS:
        raise ValueError("unknown field %r" % (field, ))
    dim = mesh._dim
    lo = np.asarray(lat[0], dtype=np.float64)
    hi = np.asarray(lat[1], dtype=np.float64)
    cells = np.asarray(lat[2:2 + dim], dtype=np.int64)
    m = 1 if field == "pressure" else 2
    X = dofmap.p1_coords if field == "pressure" else dofmap.p2_coords
    f = (X - lo) * (m * cells / (hi - lo))
    q = np.round(f).astype(np.int64)
    if np.abs(f - q).max() > 1e-6 or (q < 0).any() or (q > m * cells).any():
        raise ValueError("energy spectrum: a node is off the lattice")
    shape, periodic = [], []
    for a in range(dim):
        count = np.unique(q[:, a]).size
        if count == m * cells[a] + 1:
            periodic.append(False)
        elif count == m * cells[a]:
            periodic.append(True)
            q[:, a] %= m * cells[a]          # (whichever side carries the masters)
        else:
            raise ValueError("energy spectrum: axis %d carries %d positions, neither %d nor %d"
                             % (a, count, m * cells[a], m * cells[a] + 1))
        shape.append(int(count))
    n_points = int(np.prod(shape, dtype=np.int64))
    ids = q[:, dim - 1]
    for a in range(dim - 2, -1, -1):
        ids = ids * shape[a] + q[:, a]
    if X.shape[0] != n_points or np.bincount(ids, minlength=n_points).max() != 1:
        raise ValueError("energy spectrum: a lattice point is missing or doubled (%d nodes, %d points)"
                         % (X.shape[0], n_points))
    node_of_point = np.empty(n_points, dtype=np.int32)
    node_of_point[ids] = np.arange(n_points, dtype=np.int32)
    return Lattice(tuple(shape), node_of_point, tuple(periodic), tuple(float(v) for v in hi - lo),
                   tuple(float(v) for v in lo))


def _csr(bin_of_point, n_bins):
    """CSR of the points of every bin, ascending within a bin"""
    order = np.argsort(bin_of_point, kind="stable").astype(np.int32)
    ptr = np.zeros(n_bins + 1, dtype=np.int32)
    np.cumsum(np.bincount(bin_of_point, minlength=n_bins), out=ptr[1:])
    return ptr, order


def shell_bins(lattice):
    """the plan of ``E(k)`` on a fully periodic box: every axis transformed by ``fourier_basis``, the coefficient at
    rows ``(r_x, r_y, r_z)`` in shell ``rint(|kappa| / dkappa)``; every lattice point is in exactly one bin.  (With side
    lengths in integer ratios ``|kappa| / dkappa`` is the root of an integer and never half-way between two shells;
    with other ratios a mode may sit exactly between two shells, and rounding error decides which one takes it.)"""
    if not all(lattice.periodic):
        raise ValueError("shell spectra need a fully periodic box (use kind='axis' along a periodic axis)")
    shape, L = lattice.shape, np.asarray(lattice.lengths)
    dk = 2.0 * np.pi / L.max()
    bases = [fourier_basis(n) for n in shape]
    # |kappa|^2 of every lattice point, x fastest
    k2 = np.zeros(shape[::-1])
    for a, (_, k_of) in enumerate(bases):
        kap = (2.0 * np.pi / L[a]) * k_of
        k2 = k2 + (kap ** 2).reshape([-1 if b == a else 1 for b in range(len(shape) - 1, -1, -1)])
    shell = np.rint(np.sqrt(k2) / dk).astype(np.int64).ravel()
    n_bins = int(shell.max()) + 1
    ptr, pts = _csr(shell, n_bins)
    return Bins([F for F, _ in bases], ptr, pts, dk * np.arange(n_bins), (), (n_bins, ), int(np.prod(shape)))


def axis_bins(axis, lattice):
    """the plan of ``E(k_axis; walls)``: only ``axis`` (periodic) is transformed; bin = (indices along the walled
    axes in ascending axis order, ``|k_axis|``), the other periodic axes summed in physical space"""
    shape, dim = lattice.shape, len(lattice.shape)
    axis = int(axis)
    if not 0 <= axis < dim or not lattice.periodic[axis]:
        raise ValueError("axis spectra need a periodic axis")
    F, k_of = fourier_basis(shape[axis])
    n_k = shape[axis] // 2 + 1
    walls = [a for a in range(dim) if not lattice.periodic[a]]
    idx = np.indices(shape[::-1])[::-1]          # idx[a]: index along axis a of every point, x fastest when ravelled
    b = np.zeros(shape[::-1], dtype=np.int64)
    for a in walls:
        b = b * shape[a] + idx[a]
    b = (b * n_k + k_of[idx[axis]]).ravel()
    bin_shape = tuple(shape[a] for a in walls) + (n_k, )
    n_bins = int(np.prod(bin_shape))
    ptr, pts = _csr(b, n_bins)
    coords = tuple(lattice.origin[a] + lattice.lengths[a] * np.arange(shape[a]) / (shape[a] - 1) for a in walls)
    per_wall = int(np.prod(shape)) // int(np.prod([shape[a] for a in walls], dtype=np.int64))
    return Bins([F if a == axis else None for a in range(dim)], ptr, pts,
                (2.0 * np.pi / lattice.lengths[axis]) * np.arange(n_k), coords, bin_shape, per_wall)


class EnergySpectrum:
    """``EnergySpectrum(solver=None, kind="shell" | "axis", axis=None, field="velocity" | "temperature" | "pressure",
    start_time=0.0, every=1)``: the spectrum plan lives in the solver's device context.

    ``compute()`` returns a dict.  ``kind="shell"``: ``k`` [n_bins] (``shell index * dkappa``), ``E`` [n_bins],
    ``components`` [n_bins, ncomp].  ``kind="axis"``: ``k`` [n_k], ``walls`` (one coordinate array per walled axis, in
    ascending axis order), ``E`` [walls..., n_k] and ``components`` [walls..., n_k, ncomp].
    ``E = 1/2 sum_c sum c^2 / n_points`` for the velocity, without the 1/2 for a scalar (axis kind: ``n_points`` of one
    line or plane), so the sum over the bins is ``1/2 <|u|^2>`` over the lattice points: the discrete nodal energy, NOT
    the finite-element integral of ``ProblemBase._compute_flow_diagnostics``.

    ``sample_step(next_time, step_size)`` is what ``InstationaryProblem.solve_problem`` calls for a registered instance
    (``ProblemBase._add_energy_spectrum``): it keeps a step-size-weighted running mean on the host (the arrays are
    small) once ``next_time >= start_time``, on every ``every``-th step; ``mean()`` returns it in the form of
    ``compute()``.  The context keeps one plan: binding a second instance to a solver raises."""

    def __init__(self, solver=None, kind="shell", axis=None, field="velocity", start_time=0.0, every=1):
        assert int(every) >= 1
        if kind not in ("shell", "axis"):
            raise ValueError("kind must be 'shell' or 'axis'")
        if field not in FIELDS:
            raise ValueError("unknown field %r" % (field, ))
        if kind == "axis" and axis is None:
            raise ValueError("kind='axis' needs the axis")
        self.kind, self.axis, self.field = kind, axis, field
        self.start_time, self.every = float(start_time), int(every)
        self._solver = None
        self._registered = True
        self.reset()
        if solver is not None:
            self.bind(solver)

    @classmethod
    def one_shot(cls, solver, kind="shell", axis=None, field="velocity"):
        """an instance that does not claim the solver's registration: it shares the context's one plan with whatever
        else computes there (whichever instance computes uploads its own plan first)"""
        self = cls(None, kind=kind, axis=axis, field=field)
        self._registered = False
        self.bind(solver)
        return self

    def bind(self, solver):
        if self._solver is not None:
            assert self._solver is solver
            return
        if not hasattr(solver, "_ctx"):
            solver._setup_function_spaces()
        # one plan per context: a second registered instance would replace the first one's plan under its feet
        if self._registered:
            if getattr(solver, "_bound_energy_spectrum", self) is not self:
                raise ValueError("this solver's context already serves another EnergySpectrum (one plan per context)")
            solver._bound_energy_spectrum = self
        if self.field == "temperature":
            assert hasattr(solver, "_scalar_coefficients"), "temperature spectra need a solver that transports a scalar"
        dm = solver._dofmap
        self.lattice = lattice_of_nodes(dm.mesh, dm, self.field)
        self.bins = shell_bins(self.lattice) if self.kind == "shell" else axis_bins(self.axis, self.lattice)
        self._solver = solver
        self._upload()

    def _ctx(self):
        assert self._solver is not None, "the spectrum is not bound to a solver yet"
        return self._solver._ctx

    def _upload(self):
        b = self.bins
        self._ctx().spectrum_set(self.lattice.shape, b.matrices, self.lattice.node_of_point, b.bin_ptr, b.bin_points)
        self._solver._spectrum_plan_owner = self

    def _result(self, raw):
        b = self.bins
        scale = (0.5 if self.field == "velocity" else 1.0) / b.points_per_wall
        comp = (scale * raw).reshape(b.bin_shape + (raw.shape[1], ))
        out = dict(k=b.k.copy(), E=comp.sum(axis=-1), components=comp)
        if self.kind == "axis":
            out["walls"] = b.walls
        return out

    def raw(self):
        """[n_bins, ncomp]: the device's raw sums of squares of the solution at the new time level"""
        if getattr(self._solver, "_spectrum_plan_owner", None) is not self:      # (a one-shot of another kind ran)
            self._upload()
        return self._ctx().spectrum_compute(FIELDS[self.field])

    def compute(self):
        """the spectrum of the solution at the new time level (U0 / T0 / P)"""
        return self._result(self.raw())

    def reset(self):
        """drop the running mean (the plan stays)"""
        self._sum, self._weight, self._steps_seen, self.samples = None, 0.0, 0, 0

    def sample(self, weight=1.0):
        raw = self.raw()
        self._sum = weight * raw if self._sum is None else self._sum + weight * raw
        self._weight += float(weight)
        self.samples += 1

    def sample_step(self, next_time, step_size):
        """the cadence rule of ``FlowStatistics.sample_step``"""
        if next_time < self.start_time * (1.0 - 1e-12) - 1e-300:
            return False
        self._steps_seen += 1
        if (self._steps_seen - 1) % self.every != 0:
            return False
        self.sample(step_size)
        return True

    @property
    def weight(self):
        return self._weight

    def mean(self):
        """the step-size-weighted mean of the samples so far, in the form of ``compute()``"""
        assert self._sum is not None, "no sample has been taken"
        return self._result(self._sum / self._weight)

    def info(self):
        return self._ctx().spectrum_info()
