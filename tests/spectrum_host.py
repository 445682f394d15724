"""Host yardstick of the energy spectra: an independent restatement with the complex FFT.

``numpy.fft.fftn`` of the lattice array, ``|u^|^2 / n_points`` per mode, binned by wavenumbers computed here from
``numpy.fft.fftfreq``.  Nothing of ``energy_spectrum`` is used: not its real Fourier basis, not its bin builders.  The
figures are the RAW sums the device returns (``sum c^2`` per bin and component); the normalised spectra follow by the
factors stated in ``energy_spectrum``.

Arrays are lattice arrays ``[n_z][n_y][n_x]`` (2D: ``[n_y][n_x]``), x fastest; ``shape`` and ``lengths`` are given x first.
"""
import numpy as np

EPS = 2.2e-16


def tolerance(shape, total):
    """8 d N_max eps S: the worst-case gamma_N of a length-N dot product once per pass (d passes), doubled for the
    square, a factor 4 for the accumulation order of the matrix instruction; S = the yardstick's total"""
    return 8.0 * len(shape) * max(shape) * EPS * total


def lattice_array(values, X, spacing, shape):
    """[n_z][n_y][n_x] (+ trailing component axis) from nodal values [n_nodes(, ncomp)] at the coordinates X [n_nodes,
    dim] of a lattice with the given spacing per axis that starts at the origin; every point must be hit once"""
    values, X = np.asarray(values), np.asarray(X)
    q = np.rint(X / np.asarray(spacing)).astype(np.int64)
    assert np.abs(X / np.asarray(spacing) - q).max() < 1e-6 and (q >= 0).all() and (q < np.asarray(shape)).all()
    idx = tuple(q[:, a] for a in range(X.shape[1] - 1, -1, -1))
    hits = np.zeros(shape[::-1], dtype=np.int64)
    np.add.at(hits, idx, 1)
    assert (hits == 1).all()
    arr = np.empty(tuple(shape[::-1]) + values.shape[1:])
    arr[idx] = values
    return arr


def shell_spectrum(arr, lengths):
    """raw [n_shells]: sum over the modes of shell b of |fftn(arr)|^2 / n_points, b = rint(|kappa| / dkappa),
    kappa = 2 pi (k_x / L_x, ...), dkappa = 2 pi / max L"""
    arr = np.asarray(arr, dtype=np.float64)
    d = arr.ndim
    power = np.abs(np.fft.fftn(arr)) ** 2 / arr.size
    L = np.asarray(lengths, dtype=np.float64)            # x first
    k2 = np.zeros(arr.shape)
    for pos in range(d):                                  # array axis pos is space axis d - 1 - pos
        a = d - 1 - pos
        n = arr.shape[pos]
        kap = 2.0 * np.pi * np.fft.fftfreq(n, d=1.0 / n) / L[a]
        sh = [1] * d
        sh[pos] = n
        k2 = k2 + (kap ** 2).reshape(sh)
    shell = np.rint(np.sqrt(k2) / (2.0 * np.pi / L.max())).astype(np.int64)
    return np.bincount(shell.ravel(), weights=power.ravel(), minlength=int(shell.max()) + 1)


def axis_spectrum(arr, axis, periodic):
    """raw [walls...][n_k] (walled axes in ascending space-axis order): |fft along `axis`|^2 / n_axis, the modes +k and
    -k in the bin |k|, the other periodic axes summed as squares"""
    arr = np.asarray(arr, dtype=np.float64)
    d = arr.ndim
    pos = d - 1 - axis
    n = arr.shape[pos]
    power = np.abs(np.fft.fft(arr, axis=pos)) ** 2 / n
    kabs = np.abs(np.rint(np.fft.fftfreq(n, d=1.0 / n))).astype(np.int64)
    n_k = n // 2 + 1
    folded = np.zeros(arr.shape[:pos] + (n_k, ) + arr.shape[pos + 1:])
    idx = [slice(None)] * d
    for j in range(n):
        idx[pos] = kabs[j]
        src = list(idx)
        src[pos] = j
        folded[tuple(idx)] += power[tuple(src)]
    other = tuple(d - 1 - a for a in range(d) if a != axis and periodic[a])
    folded = folded.sum(axis=other) if other else folded
    # remaining array axes: the walled space axes in DESCENDING order and the k axis among them; reorder to
    # (walls ascending..., k)
    remaining = [a for a in range(d - 1, -1, -1) if a == axis or not periodic[a]]
    walls = sorted(a for a in remaining if a != axis)
    return np.transpose(folded, [remaining.index(a) for a in walls] + [remaining.index(axis)])
