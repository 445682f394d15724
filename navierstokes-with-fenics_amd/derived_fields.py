"""Gradient-derived fields of the device-resident solution (csrc/derived.hip).

Vorticity, divergence, shear rate, Q-criterion, the velocity gradient, the pressure gradient and the temperature
gradient of the CURRENT solution (``U0``, ``P``, ``T0``), centred per cell (means), per cell vertex (DG1 data) or
recovered at the P2 nodes -- every requested quantity from ONE element-kernel launch and one copy of the result, instead
of a copy of the whole state and numpy einsums on the host (``ProblemBase._compute_vorticity`` and its relatives,
which stay as they are).

* ``compute(solver, names, center)``: dict name -> array; ``center`` "Cell" ``[n_cells(, ncomp)]``, "Vertex"
  ``[n_cells, dim + 1(, ncomp)]``, "Node" ``[n_p2(, ncomp)]``.  Quantities with one component have no component axis;
  the velocity gradient comes as ``[..., dim, dim]`` (``G[a, b] = d_b u_a``).
* ``ProblemBase._compute_derived_field(name, center)`` wraps a result into a ``HostField`` for
  ``_add_to_field_output``.

Partitioned meshes are not supported (the device refuses them: the recovery at a node on a partition boundary needs
the cells of other ranks).
"""
import _native as nat

QUANTITIES = {
    "vorticity": nat.DERIVED_VORTICITY,
    "divergence": nat.DERIVED_DIVERGENCE,
    "shear rate": nat.DERIVED_SHEAR_RATE,
    "q criterion": nat.DERIVED_Q_CRITERION,
    "velocity gradient": nat.DERIVED_VELOCITY_GRADIENT,
    "pressure gradient": nat.DERIVED_PRESSURE_GRADIENT,
    "temperature gradient": nat.DERIVED_SCALAR_GRADIENT,
}
CENTERS = {"Cell": nat.DERIVED_CELL, "Vertex": nat.DERIVED_VERTEX, "Node": nat.DERIVED_NODE}


def compute(solver, names, center="Node"):
    """{name: array} of the quantities ``names`` (one name or several, keys of ``QUANTITIES``) of the solver's current
    solution at ``center`` (a key of ``CENTERS``): one device call for all of them"""
    names = [names] if isinstance(names, str) else list(names)
    for name in names:
        if name not in QUANTITIES:
            raise ValueError("unknown derived field %r (known: %s)" % (name, ", ".join(sorted(QUANTITIES))))
    if center not in CENTERS:
        raise ValueError("unknown centre %r (known: %s)" % (center, ", ".join(CENTERS)))
    ids = [QUANTITIES[name] for name in names]
    scalar_slot = nat.T0 if nat.DERIVED_SCALAR_GRADIENT in ids else -1
    try:
        res = solver._ctx.derived_fields(ids, CENTERS[center], nat.U0, nat.P, scalar_slot)
    except nat.NativeError as err:
        raise RuntimeError(str(err))
    out = {}
    for name, q in zip(names, ids):
        a = res[q]
        if q == nat.DERIVED_VELOCITY_GRADIENT:
            dim = solver._ctx.dim
            a = a.reshape(a.shape[:-1] + (dim, dim))
        out[name] = a
    return out
