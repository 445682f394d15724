"""ctypes binding of libnsfem_hip.so (C ABI: include/nsfem.h).

This is the only way the Python host code reaches the device.  There is NO CPU
fallback: if the shared library is missing or no MI355X is visible, every entry
point raises.  (The reference reaches its native layer -- DOLFIN/PETSc -- through
pybind11 inside ``import dolfin``; this thin ctypes layer replaces that import.)
"""
import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libnsfem_hip.so")

# ---- enums (mirror include/nsfem.h) ------------------------------------------
OK, ERR_ARG, ERR_HIP, ERR_BREAKDOWN, ERR_NOT_CONVERGED, ERR_COMM = 0, -1, -2, -3, -4, -5
U0, U1, U2, USTAR, P, P_OLD, BODY_FORCE, TRACTION, P2_OLD, CONV_N1, CONV_N2 = range(11)
T0, T1, T2, T_SOURCE, TCONV_1, TCONV_2 = range(11, 17)       # transported P2 scalar (set_scalar / step_scalar_imex)
N_SLOTS = 17                # NSFEM_N_SLOTS
VELOCITY, PRESSURE, PRESSURE_PRECOND, SCALAR = 0, 1, 2, 3
(OP_MASS_P2, OP_STIFF_P2, OP_STIFF_P1, OP_MASS_P1, OP_DIV, OP_GRAD, OP_DIVT,
 OP_MOMENTUM_JAC, OP_VISCOUS_EXTRA, OP_MOMENTUM_JAC_MF, OP_MOMENTUM_SMOOTHER,
 OP_CONVECTION_ACTION) = range(12)
SYS_MOMENTUM, SYS_POISSON, SYS_CORRECTION, SYS_MONOLITHIC = range(4)
MAX_NEWTON = 64
N_FUNCTIONALS = 11          # NSFEM_N_FUNCTIONALS
STATS_VELOCITY, STATS_PRESSURE, STATS_SCALAR = 1, 2, 4      # nsfem_stats_flags
(STATS_MEAN_U, STATS_COV_U, STATS_TKE, STATS_MEAN_P, STATS_VAR_P, STATS_MEAN_T, STATS_VAR_T,
 STATS_FLUX_UT) = range(8)                                  # nsfem_stats_quantity
(DERIVED_VORTICITY, DERIVED_DIVERGENCE, DERIVED_SHEAR_RATE, DERIVED_Q_CRITERION, DERIVED_VELOCITY_GRADIENT,
 DERIVED_PRESSURE_GRADIENT, DERIVED_SCALAR_GRADIENT) = range(7)      # nsfem_derived_quantity
N_DERIVED = 7
DERIVED_CELL, DERIVED_VERTEX, DERIVED_NODE = range(3)      # nsfem_derived_center

EXPORTED_SYMBOLS = (
    "nsfem_create", "nsfem_destroy", "nsfem_last_error", "nsfem_version",
    "nsfem_set_coeffs", "nsfem_set_bdf", "nsfem_set_dirichlet", "nsfem_set_viscous_form",
    "nsfem_set_convective_form",
    "nsfem_set_state", "nsfem_get_state", "nsfem_state_size", "nsfem_state_devptr",
    "nsfem_assemble", "nsfem_residual_norm", "nsfem_get_rhs", "nsfem_solve",
    "nsfem_operator_shape", "nsfem_operator_export", "nsfem_operator_apply", "nsfem_kernel_apply",
    "nsfem_lattice_restrict",
    "nsfem_default_step_opts", "nsfem_step_ipcs", "nsfem_step_bdf", "nsfem_advance",
    "nsfem_shift_mean_pressure", "nsfem_time_spmv", "nsfem_synchronize", "nsfem_mass_solve",
    "nsfem_mg_add_level", "nsfem_mg_finalize", "nsfem_mg_set_global_coarse", "nsfem_mg_set_global_coarse_constrained",
    "nsfem_mg_set_schur_operator", "nsfem_mg_set_schur_mode", "nsfem_set_halo_lists", "nsfem_smoother_info", "nsfem_mg_set_global_index", "nsfem_comm_allreduce", "nsfem_mg_add_global_level", "nsfem_cfl_number", "nsfem_set_angular_velocity", "nsfem_set_angular_velocity_3d", "nsfem_profile_smoother", "nsfem_profile_smoother_detail", "nsfem_profile_convection", "nsfem_jacobian_info", "nsfem_step_frame_info", "nsfem_newton_frame_info", "nsfem_jacobian_table_check", "nsfem_set_preconditioner_shift", "nsfem_poisson_solve", "nsfem_p2_mass_bounds", "nsfem_mg_set_truncation", "nsfem_comm_stats", "nsfem_mg_set_halo_mode", "nsfem_set_overlap", "nsfem_comm_overlapped", "nsfem_boundary_force",
    "nsfem_set_partition", "nsfem_comm_unique_id", "nsfem_comm_attach_rccl",
    "nsfem_comm_local_create", "nsfem_comm_local_destroy", "nsfem_comm_attach_local", "nsfem_comm_attach_shm",
    "nsfem_mg_apply", "nsfem_mg_info", "nsfem_monolithic_apply", "nsfem_poisson_set_fast_diag", "nsfem_poisson_set_fast_diag_rows",
    "nsfem_poisson_set_fast_diag_3d", "nsfem_poisson_set_fast_diag_3d_planes", "nsfem_poisson_fast_diag_3d_info",
    "nsfem_operator_diagonal",
    "nsfem_set_imex", "nsfem_step_imex", "nsfem_imex_info", "nsfem_imex_rhs",
    "nsfem_set_imex_rotation", "nsfem_imex_rotation_info",
    "nsfem_volume_functionals",
    "nsfem_set_scalar", "nsfem_step_scalar_imex", "nsfem_scalar_convection", "nsfem_scalar_info",
    "nsfem_set_scalar_sgs", "nsfem_scalar_explicit", "nsfem_scalar_sgs_info",
    "nsfem_set_scalar_sgs_dynamic", "nsfem_scalar_dynamic_constant", "nsfem_scalar_diffusivity_cells",
    "nsfem_scalar_dynamic_info",
    "nsfem_set_viscosity_law", "nsfem_viscosity_residual", "nsfem_viscosity_cells", "nsfem_viscosity_info",
    "nsfem_set_dynamic_groups", "nsfem_dynamic_constant", "nsfem_dynamic_info",
    "nsfem_set_dynamic_averaging", "nsfem_dynamic_lagrangian_state", "nsfem_dynamic_lagrangian_advance",
    "nsfem_dynamic_lagrangian_info",
    "nsfem_set_bodies", "nsfem_move_bodies", "nsfem_body_residual", "nsfem_body_mask_cells", "nsfem_body_forces",
    "nsfem_body_info",
    "nsfem_set_wall_model", "nsfem_wall_model_residual", "nsfem_wall_model_facets", "nsfem_wall_model_info",
    "nsfem_set_body_temperatures", "nsfem_body_scalar_residual", "nsfem_body_heat", "nsfem_body_heat_info",
    "nsfem_set_point_locator", "nsfem_locate_points", "nsfem_eval_points",
    "nsfem_tracers_set", "nsfem_tracers_advect", "nsfem_tracers_get", "nsfem_tracers_info",
    "nsfem_stats_enable", "nsfem_stats_sample", "nsfem_stats_get", "nsfem_stats_set_groups", "nsfem_stats_profiles",
    "nsfem_stats_info", "nsfem_stats_weight",
    "nsfem_derived_components", "nsfem_derived_fields", "nsfem_derived_info",
    "nsfem_spectrum_set", "nsfem_spectrum_compute", "nsfem_spectrum_info",
    "nsfem_wall_set_facets", "nsfem_wall_compute", "nsfem_wall_components", "nsfem_wall_info",
)


class MeshDesc(C.Structure):
    _fields_ = [("dim", C.c_int32), ("n_cells", C.c_int32), ("n_vertices", C.c_int32),
                ("n_p2", C.c_int32), ("n_p1", C.c_int32),
                ("coords", C.POINTER(C.c_double)), ("cells", C.POINTER(C.c_int32)),
                ("p2_dofmap", C.POINTER(C.c_int32)), ("p1_dofmap", C.POINTER(C.c_int32))]


class KernelTest(C.Structure):
    _fields_ = [(k, C.c_int32) for k in ("space", "nv", "family", "epilogue", "steps", "maskmode", "ghost", "ident",
                                          "from_zero", "with_residual", "dict_ok", "used_family", "dict_entries",
                                          "dict_exact", "lattice_w", "lattice_kind")] + \
               [("a", C.c_double), ("b_coef", C.c_double), ("c1", C.c_double * 8), ("c2", C.c_double * 8),
                ("x", C.POINTER(C.c_double)), ("b", C.POINTER(C.c_double)), ("d", C.POINTER(C.c_double)),
                ("mask", C.POINTER(C.c_uint8)),
                ("y", C.POINTER(C.c_double)), ("d_out", C.POINTER(C.c_double)), ("r_out", C.POINTER(C.c_double)),
                ("xc", C.POINTER(C.c_double)), ("rf", C.POINTER(C.c_double)), ("b_formed", C.POINTER(C.c_double))] + \
               [(k, C.c_int32) for k in ("gh_lo", "gh_hi", "gh_zero", "tile_lines", "fixed", "lattice_tile_lines",
                                          "lattice_tx", "lattice_ty", "lattice_tiles", "lattice_fixed_shape")]


class WallOpts(C.Structure):
    """nsfem_wall_opts"""
    _fields_ = [("nu", C.c_double), ("sym", C.c_double), ("kappa", C.c_double), ("origin", C.c_double * 3),
                ("use_law", C.c_int)]


class Body(C.Structure):
    """nsfem_body: kind 1 ball, 2 axis-aligned box, 3 half-space (include/nsfem.h)"""
    _fields_ = [("kind", C.c_int32), ("centre", C.c_double * 3), ("size", C.c_double * 3),
                ("velocity", C.c_double * 3), ("angular", C.c_double * 3)]


MAX_BODIES = 16


class KrylovOpts(C.Structure):
    _fields_ = [("rtol", C.c_double), ("atol", C.c_double), ("max_iter", C.c_int32),
                ("precond", C.c_int32), ("check_every", C.c_int32), ("first_check", C.c_int32)]


class SolveInfo(C.Structure):
    _fields_ = [("iterations", C.c_int32), ("converged", C.c_int32),
                ("residual", C.c_double), ("residual0", C.c_double)]


class StepOpts(C.Structure):
    _fields_ = [("newton_atol", C.c_double), ("newton_rtol", C.c_double),
                ("newton_max_iter", C.c_int32), ("convective_form", C.c_int32),
                ("momentum", KrylovOpts), ("poisson", KrylovOpts), ("correction", KrylovOpts),
                ("picard", C.c_int32), ("allow_nonconvergence", C.c_int32),
                ("newton_forcing", C.c_double), ("matrix_free", C.c_int32),
                ("pressure_extrapolation", C.c_int32)]


class StepInfo(C.Structure):
    _fields_ = [("newton_iterations", C.c_int32), ("krylov_iterations_momentum", C.c_int32),
                ("krylov_iterations_poisson", C.c_int32),
                ("krylov_iterations_correction", C.c_int32),
                ("newton_residuals", C.c_double * MAX_NEWTON),
                ("converged", C.c_int32), ("reserved", C.c_int32)]


class Halo(C.Structure):
    _fields_ = [(k, C.c_int64) for k in ("send_up_off", "send_up_cnt", "recv_above_off",
                                         "recv_above_cnt", "send_down_off", "send_down_cnt",
                                         "recv_below_off", "recv_below_cnt")]

    @classmethod
    def from_dict(cls, d):
        h = cls()
        if d:
            for key in ("send_up", "recv_above", "send_down", "recv_below"):
                setattr(h, key + "_off", int(d[key][0]))
                setattr(h, key + "_cnt", int(d[key][1]))
        return h


class HaloLists(C.Structure):
    _fields_ = [("n_neighbours", C.c_int32), ("neighbour", C.POINTER(C.c_int32)),
                ("send_ptr", C.POINTER(C.c_int64)), ("send_idx", C.POINTER(C.c_int32)),
                ("recv_ptr", C.POINTER(C.c_int64)), ("recv_idx", C.POINTER(C.c_int32))]


class MgLevelDesc(C.Structure):
    _fields_ = [("n_vertices", C.c_int32), ("n_cells", C.c_int32),
                ("coords", C.POINTER(C.c_double)), ("cells", C.POINTER(C.c_int32)),
                ("n_fine", C.c_int32), ("p_rowptr", C.POINTER(C.c_int32)),
                ("p_col", C.POINTER(C.c_int32)), ("p_val", C.POINTER(C.c_double)),
                ("ghost", C.POINTER(C.c_uint8)), ("halo", Halo),
                ("dofmap", C.POINTER(C.c_int32)), ("n_dofs", C.c_int32), ("transfer_kind", C.c_int32)]


class PartitionDesc(C.Structure):
    _fields_ = [("rank", C.c_int32), ("size", C.c_int32),
                ("p2_ghost", C.POINTER(C.c_uint8)), ("p1_ghost", C.POINTER(C.c_uint8)),
                ("p2_halo", Halo), ("p1_halo", Halo),
                ("n_p2_global", C.c_int64), ("n_p1_global", C.c_int64), ("periodic", C.c_int32)]


class MgOpts(C.Structure):
    _fields_ = [("smoother_degree", C.c_int32), ("coarse_dense_max", C.c_int32),
                ("eig_ratio", C.c_double)]


class NativeError(RuntimeError):
    def __init__(self, code, message):
        super().__init__("libnsfem_hip: %s (status %d)" % (message, code))
        self.code = code


_lib = None


def load_library(path=None):
    """dlopen the shared library and declare the prototypes.  Raises loudly when
    the library has not been built (``python -c 'import __graft_entry__ as g; g.build()'``)."""
    global _lib
    if _lib is not None and path is None:
        return _lib
    path = path or LIB_PATH
    if not os.path.exists(path):
        raise ImportError("libnsfem_hip.so is not built (%s): the HIP extension is mandatory, "
                          "there is no CPU fallback; run __graft_entry__.build()" % path)
    lib = C.CDLL(path)
    vp, i32, i64, dbl = C.c_void_p, C.c_int32, C.c_int64, C.c_double
    pd, pi = C.POINTER(C.c_double), C.POINTER(C.c_int32)
    protos = {
        "nsfem_create": (C.c_int, [C.POINTER(MeshDesc), C.c_int, C.POINTER(vp)]),
        "nsfem_destroy": (None, [vp]),
        "nsfem_last_error": (C.c_char_p, [vp]),
        "nsfem_version": (C.c_int, []),
        "nsfem_set_coeffs": (C.c_int, [vp, pd]),
        "nsfem_set_bdf": (C.c_int, [vp, pd, dbl]),
        "nsfem_set_imex": (C.c_int, [vp, pd, pd, pd, dbl]),
        "nsfem_step_imex": (C.c_int, [vp, C.POINTER(StepOpts), C.POINTER(StepInfo)]),
        "nsfem_imex_info": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "nsfem_imex_rhs": (C.c_int, [vp, C.c_int, C.c_int, pd, pd]),
        "nsfem_set_imex_rotation": (C.c_int, [vp, C.c_int, pd, pd]),
        "nsfem_imex_rotation_info": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "nsfem_set_dirichlet": (C.c_int, [vp, C.c_int, i32, pi, pd]),
        "nsfem_set_scalar": (C.c_int, [vp, dbl, pd, C.c_int]),
        "nsfem_step_scalar_imex": (C.c_int, [vp, C.POINTER(KrylovOpts), C.POINTER(SolveInfo)]),
        "nsfem_scalar_convection": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, dbl, pd]),
        "nsfem_scalar_info": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "nsfem_set_scalar_sgs": (C.c_int, [vp, dbl]),
        "nsfem_scalar_explicit": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, dbl, pd]),
        "nsfem_scalar_sgs_info": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "nsfem_set_scalar_sgs_dynamic": (C.c_int, [vp, C.c_int, dbl]),
        "nsfem_scalar_dynamic_constant": (C.c_int, [vp, C.c_int, C.c_int, pd, pd, pd]),
        "nsfem_scalar_diffusivity_cells": (C.c_int, [vp, C.c_int, C.c_int, pd]),
        "nsfem_scalar_dynamic_info": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "nsfem_set_viscosity_law": (C.c_int, [vp, C.c_int, pd]),
        "nsfem_viscosity_residual": (C.c_int, [vp, C.c_int, dbl, pd]),
        "nsfem_viscosity_cells": (C.c_int, [vp, C.c_int, pd]),
        "nsfem_viscosity_info": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "nsfem_set_dynamic_groups": (C.c_int, [vp, C.c_int, C.POINTER(C.c_int32)]),
        "nsfem_dynamic_constant": (C.c_int, [vp, C.c_int, pd, pd, pd]),
        "nsfem_dynamic_info": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "nsfem_set_dynamic_averaging": (C.c_int, [vp, C.c_int, pd]),
        "nsfem_dynamic_lagrangian_state": (C.c_int, [vp, C.c_int, pd]),
        "nsfem_dynamic_lagrangian_advance": (C.c_int, [vp, C.c_int, dbl, pd, pd, pd]),
        "nsfem_dynamic_lagrangian_info": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "nsfem_set_bodies": (C.c_int, [vp, C.c_int32, C.POINTER(Body), dbl, dbl]),
        "nsfem_move_bodies": (C.c_int, [vp, C.c_int32, C.POINTER(Body)]),
        "nsfem_body_residual": (C.c_int, [vp, C.c_int, dbl, pd]),
        "nsfem_body_mask_cells": (C.c_int, [vp, pd]),
        "nsfem_body_forces": (C.c_int, [vp, C.c_int, pd]),
        "nsfem_body_info": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "nsfem_set_wall_model": (C.c_int, [vp, C.c_int, pd, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32),
                                           C.POINTER(C.c_int32), pd, pd, pd]),
        "nsfem_wall_model_residual": (C.c_int, [vp, C.c_int, dbl, pd]),
        "nsfem_wall_model_facets": (C.c_int, [vp, C.c_int, pd]),
        "nsfem_wall_model_info": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "nsfem_set_body_temperatures": (C.c_int, [vp, C.c_int32, C.POINTER(C.c_int32), pd, dbl]),
        "nsfem_body_scalar_residual": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, dbl, C.c_int, pd]),
        "nsfem_body_heat": (C.c_int, [vp, C.c_int, pd]),
        "nsfem_body_heat_info": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "nsfem_set_viscous_form": (C.c_int, [vp, C.c_int]),
        "nsfem_set_convective_form": (C.c_int, [vp, C.c_int, C.c_int]),
        "nsfem_set_state": (C.c_int, [vp, C.c_int, pd, i64]),
        "nsfem_get_state": (C.c_int, [vp, C.c_int, pd, i64]),
        "nsfem_state_size": (i64, [vp, C.c_int]),
        "nsfem_state_devptr": (vp, [vp, C.c_int]),
        "nsfem_assemble": (C.c_int, [vp, C.c_int, C.c_uint32]),
        "nsfem_residual_norm": (C.c_int, [vp, C.c_int, pd]),
        "nsfem_get_rhs": (C.c_int, [vp, C.c_int, pd, i64]),
        "nsfem_solve": (C.c_int, [vp, C.c_int, C.POINTER(KrylovOpts), C.POINTER(SolveInfo)]),
        "nsfem_operator_shape": (C.c_int, [vp, C.c_int, C.POINTER(i64), C.POINTER(i64),
                                           C.POINTER(i64)]),
        "nsfem_operator_export": (C.c_int, [vp, C.c_int, pi, pi, pd]),
        "nsfem_operator_apply": (C.c_int, [vp, C.c_int, pd, pd]),
        "nsfem_kernel_apply": (C.c_int, [vp, C.POINTER(KernelTest)]),
        "nsfem_lattice_restrict": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_int, pd, C.POINTER(C.c_uint8),
                                             C.POINTER(C.c_uint8), pd, pd]),
        "nsfem_default_step_opts": (C.c_int, [C.POINTER(StepOpts)]),
        "nsfem_step_ipcs": (C.c_int, [vp, C.POINTER(StepOpts), C.POINTER(StepInfo)]),
        "nsfem_step_bdf": (C.c_int, [vp, C.POINTER(StepOpts), C.POINTER(StepInfo)]),
        "nsfem_advance": (C.c_int, [vp, C.c_int]),
        "nsfem_shift_mean_pressure": (C.c_int, [vp, dbl, pd]),
        "nsfem_cfl_number": (C.c_int, [vp, C.c_int, dbl, pd]),
        "nsfem_set_angular_velocity": (C.c_int, [vp, dbl, dbl]),
        "nsfem_set_angular_velocity_3d": (C.c_int, [vp, pd, pd]),
        "nsfem_set_preconditioner_shift": (C.c_int, [vp, dbl]),
        "nsfem_p2_mass_bounds": (C.c_int, [C.c_int, pd, pd]),
        "nsfem_mg_set_truncation": (C.c_int, [vp, dbl, dbl]),
        "nsfem_comm_stats": (C.c_int, [vp, C.POINTER(C.c_int64), C.c_int]),
        "nsfem_mg_set_halo_mode": (C.c_int, [vp, C.c_int]),
        "nsfem_set_overlap": (C.c_int, [vp, C.c_int]),
        "nsfem_boundary_force": (C.c_int, [vp, C.c_int, C.c_int, i32, pi, pi, dbl, dbl, pd]),
        "nsfem_volume_functionals": (C.c_int, [vp, C.c_int, C.c_int, pd, pd, C.POINTER(C.c_uint8), pd]),
        "nsfem_comm_overlapped": (C.c_int, [vp, C.POINTER(C.c_int64), C.c_int]),
        "nsfem_set_point_locator": (C.c_int, [vp, pd, pd, pi, pi, pi]),
        "nsfem_locate_points": (C.c_int, [vp, i64, pd, pi]),
        "nsfem_eval_points": (C.c_int, [vp, C.c_int, i64, pd, pi, pd]),
        "nsfem_tracers_set": (C.c_int, [vp, i64, pd]),
        "nsfem_tracers_advect": (C.c_int, [vp, C.c_int, C.c_int, dbl, C.c_int]),
        "nsfem_tracers_get": (C.c_int, [vp, pd, pi, C.POINTER(C.c_uint8)]),
        "nsfem_tracers_info": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "nsfem_stats_enable": (C.c_int, [vp, C.c_uint32]),
        "nsfem_stats_sample": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, dbl]),
        "nsfem_stats_get": (C.c_int, [vp, C.c_int, pd, i64]),
        "nsfem_stats_set_groups": (C.c_int, [vp, C.c_int, i32, pi, pi, pd]),
        "nsfem_stats_profiles": (C.c_int, [vp, C.c_int, pd, i64]),
        "nsfem_stats_info": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "nsfem_stats_weight": (C.c_int, [vp, pd]),
        "nsfem_derived_components": (C.c_int, [vp, C.c_int, C.POINTER(C.c_int)]),
        "nsfem_derived_fields": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.c_uint, C.c_int, pd, i64]),
        "nsfem_derived_info": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "nsfem_spectrum_set": (C.c_int, [vp, pi, pd, pd, pd, pi, i32, pi, pi]),
        "nsfem_spectrum_compute": (C.c_int, [vp, C.c_int, pd, i64]),
        "nsfem_spectrum_info": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "nsfem_wall_set_facets": (C.c_int, [vp, i32, pi, pi, pi, i32]),
        "nsfem_wall_compute": (C.c_int, [vp, C.c_int, C.c_int, C.c_int, C.POINTER(WallOpts), pd, pd]),
        "nsfem_wall_components": (C.c_int, [vp, C.POINTER(C.c_int)]),
        "nsfem_wall_info": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "nsfem_poisson_solve": (C.c_int, [vp, pd, i64, pi, pd, C.POINTER(KrylovOpts), C.POINTER(SolveInfo)]),
        "nsfem_profile_smoother": (C.c_int, [vp, C.c_int, pd, C.POINTER(i64), C.POINTER(i64)]),
        "nsfem_profile_convection": (C.c_int, [vp, C.c_int, pd, C.POINTER(i64), C.POINTER(i64)]),
        "nsfem_profile_smoother_detail": (C.c_int, [vp, C.POINTER(i64)]),
        "nsfem_time_spmv": (C.c_int, [vp, C.c_int, C.c_int, pd, C.POINTER(i64)]),
        "nsfem_synchronize": (C.c_int, [vp]),
        "nsfem_mg_add_level": (C.c_int, [vp, C.POINTER(MgLevelDesc)]),
        "nsfem_mg_finalize": (C.c_int, [vp, C.POINTER(MgOpts)]),
        "nsfem_mg_add_global_level": (C.c_int, [vp, C.POINTER(MgLevelDesc)]),
        "nsfem_mg_set_schur_operator": (C.c_int, [vp, C.c_int, C.c_int32, C.POINTER(C.c_int32),
                                                  C.POINTER(C.c_int32), C.POINTER(C.c_double),
                                                  C.c_int]),
        "nsfem_mg_set_schur_mode": (C.c_int, [vp, C.c_int]),
        "nsfem_smoother_info": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "nsfem_jacobian_info": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "nsfem_step_frame_info": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "nsfem_newton_frame_info": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "nsfem_jacobian_table_check": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "nsfem_mg_apply": (C.c_int, [vp, C.c_int, pd, pd]),
        "nsfem_mg_info": (C.c_int, [vp, C.c_int, C.POINTER(C.c_int64)]),
        "nsfem_monolithic_apply": (C.c_int, [vp, C.c_int, C.c_int, pd, pd]),
        "nsfem_poisson_set_fast_diag": (C.c_int, [vp, i32, i32, pd, pd, pd]),
        "nsfem_operator_diagonal": (C.c_int, [vp, C.c_int, pd]),
        "nsfem_poisson_set_fast_diag_rows": (C.c_int, [vp, i32, i32, i32, pd, pd, pd]),
        "nsfem_poisson_set_fast_diag_3d": (C.c_int, [vp, i32, i32, i32, pd, pd, pd, pd, i32]),
        "nsfem_poisson_set_fast_diag_3d_planes": (C.c_int, [vp, i32, i32, i32, i32, pd, pd, pd, pd, i32]),
        "nsfem_poisson_fast_diag_3d_info": (C.c_int, [vp, C.POINTER(C.c_int64)]),
        "nsfem_set_halo_lists": (C.c_int, [vp, C.c_int, C.POINTER(HaloLists)]),
        "nsfem_mg_set_global_index": (C.c_int, [vp, i32, pi]),
        "nsfem_comm_allreduce": (C.c_int, [vp, pd, C.c_int, C.c_int]),
        "nsfem_mg_set_global_coarse": (C.c_int, [vp, i32, i32, pd, pi, i64]),
        "nsfem_mg_set_global_coarse_constrained": (C.c_int, [vp, i32, i32, pd, pi, pi, i32, i64]),
        "nsfem_set_partition": (C.c_int, [vp, C.POINTER(PartitionDesc)]),
        "nsfem_comm_unique_id": (C.c_int, [C.c_char_p]),
        "nsfem_comm_attach_rccl": (C.c_int, [vp, C.c_char_p, C.c_int, C.c_int]),
        "nsfem_comm_local_create": (C.c_int, [C.c_int, C.POINTER(vp)]),
        "nsfem_comm_local_destroy": (None, [vp]),
        "nsfem_comm_attach_local": (C.c_int, [vp, vp, C.c_int]),
        "nsfem_comm_attach_shm": (C.c_int, [vp, C.c_char_p, C.c_int, C.c_int, C.c_int64]),
        "nsfem_mass_solve": (C.c_int, [vp, C.c_int, pd, pd, C.POINTER(KrylovOpts),
                                       C.POINTER(SolveInfo)]),
    }
    for name, (res, args) in protos.items():
        fn = getattr(lib, name)      # AttributeError = missing export: fail loudly
        fn.restype = res
        fn.argtypes = args
    if path == LIB_PATH:
        _lib = lib
    return lib


def local_group_create(size):
    """In-process communicator group (several contexts on one device; testing only)."""
    lib = load_library()
    g = C.c_void_p()
    rc = lib.nsfem_comm_local_create(int(size), C.byref(g))
    if rc != OK:
        raise NativeError(rc, "nsfem_comm_local_create failed")
    return g


def local_group_destroy(group):
    load_library().nsfem_comm_local_destroy(group)


def rccl_unique_id():
    buf = C.create_string_buffer(128)
    rc = load_library().nsfem_comm_unique_id(buf)
    if rc != OK:
        raise NativeError(rc, "ncclGetUniqueId failed")
    return buf.raw


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _ip(a):
    return a.ctypes.data_as(C.POINTER(C.c_int32))


class NsfemContext:
    """RAII wrapper of one ``nsfem_ctx`` (one mesh, one GPU, one stream)."""

    def __init__(self, coords, cells, p2_dofmap, p1_dofmap, n_p2, n_p1, device=0):
        self._lib = load_library()
        self._h = C.c_void_p()
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        cells = np.ascontiguousarray(cells, dtype=np.int32)
        p2 = np.ascontiguousarray(p2_dofmap, dtype=np.int32)
        p1 = np.ascontiguousarray(p1_dofmap, dtype=np.int32)
        assert coords.ndim == 2 and coords.shape[1] in (2, 3)
        dim = int(coords.shape[1])                        # 2: triangles, 3: tetrahedra
        assert cells.shape == (p2.shape[0], dim + 1) and p1.shape == cells.shape
        assert p2.shape[1] == (6 if dim == 2 else 10)
        self.dim = dim
        self.n_cells = int(cells.shape[0])
        desc = MeshDesc(dim, cells.shape[0], coords.shape[0], int(n_p2), int(n_p1),
                        _dp(coords), _ip(cells), _ip(p2), _ip(p1))
        rc = self._lib.nsfem_create(C.byref(desc), int(device), C.byref(self._h))
        if rc != OK:
            msg = self._lib.nsfem_last_error(None)
            raise NativeError(rc, msg.decode() if msg else "nsfem_create failed")
        self.n_p2, self.n_p1 = int(n_p2), int(n_p1)
        self.n_velocity = dim * self.n_p2

    def close(self):
        if getattr(self, "_h", None) is not None and self._h.value:
            self._lib.nsfem_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc):
        if rc != OK:
            msg = self._lib.nsfem_last_error(self._h)
            raise NativeError(rc, msg.decode() if msg else "error")

    # -- coefficients / BCs ---------------------------------------------------
    def set_coeffs(self, convective, pressure, viscous, body_force=None, coriolis=None, euler=None):
        c = np.array([np.nan if v is None else float(v)
                      for v in (convective, pressure, viscous, body_force, coriolis, euler)])
        self._check(self._lib.nsfem_set_coeffs(self._h, _dp(c)))

    def set_bdf(self, alpha, k):
        a = np.ascontiguousarray(alpha, dtype=np.float64)
        assert a.shape == (3,)
        self._check(self._lib.nsfem_set_bdf(self._h, _dp(a), float(k)))

    def set_imex(self, alpha, beta, gamma, k):
        """coefficients of IMEXTimeStepping (alpha, beta, gamma) and the step size for step_imex"""
        a = np.ascontiguousarray(alpha, dtype=np.float64)
        b = np.ascontiguousarray(beta, dtype=np.float64)
        g = np.ascontiguousarray(gamma, dtype=np.float64)
        assert a.shape == (3,) and b.shape == (2,) and g.shape == (3,)
        self._check(self._lib.nsfem_set_imex(self._h, _dp(a), _dp(b), _dp(g), float(k)))

    def set_dirichlet(self, field, dofs, vals):
        d = np.ascontiguousarray(dofs, dtype=np.int32)
        v = np.ascontiguousarray(vals, dtype=np.float64)
        assert d.shape == v.shape and d.ndim == 1
        self._check(self._lib.nsfem_set_dirichlet(self._h, field, d.size, _ip(d), _dp(v)))

    def set_convective_form(self, form, picard=False):
        self._check(self._lib.nsfem_set_convective_form(self._h, int(form), int(bool(picard))))

    def set_viscous_form(self, traction_form):
        self._check(self._lib.nsfem_set_viscous_form(self._h, int(bool(traction_form))))

    # -- state ------------------------------------------------------------------
    def state_size(self, slot):
        return int(self._lib.nsfem_state_size(self._h, slot))

    def set_state(self, slot, values):
        v = np.ascontiguousarray(values, dtype=np.float64)
        self._check(self._lib.nsfem_set_state(self._h, slot, _dp(v), v.size))

    def get_state(self, slot):
        out = np.empty(self.state_size(slot), dtype=np.float64)
        self._check(self._lib.nsfem_get_state(self._h, slot, _dp(out), out.size))
        return out

    def state_devptr(self, slot):
        return self._lib.nsfem_state_devptr(self._h, slot)

    # -- assembly seam + solves -------------------------------------------------
    def assemble(self, system, new_step=False, matrix_free=False):
        """matrix_free (SYS_MONOLITHIC only): the solve that follows applies the velocity Jacobian matrix-free"""
        self._check(self._lib.nsfem_assemble(self._h, system, (1 if new_step else 0) | (2 if matrix_free else 0)))

    def residual_norm(self, system):
        out = C.c_double()
        self._check(self._lib.nsfem_residual_norm(self._h, system, C.byref(out)))
        return out.value

    def get_rhs(self, system):
        n = self.n_p1 if system == SYS_POISSON else self.n_velocity
        if system == SYS_MONOLITHIC:
            n = self.n_velocity + self.n_p1
        out = np.empty(n, dtype=np.float64)
        self._check(self._lib.nsfem_get_rhs(self._h, system, _dp(out), n))
        return out

    def solve(self, system, rtol=1e-12, atol=1e-14, max_iter=20000, precond=0, check_every=1, first_check=0):
        """a failed solve raises NativeError with the status in `code` (ERR_NOT_CONVERGED, ERR_BREAKDOWN, ...) and
        what the solver reported up to then in `info`"""
        o = KrylovOpts(rtol, atol, max_iter, precond, check_every, first_check)
        info = SolveInfo()
        try:
            self._check(self._lib.nsfem_solve(self._h, system, C.byref(o), C.byref(info)))
        except NativeError as err:
            err.info = info
            raise
        return info

    def default_step_opts(self):
        o = StepOpts()
        self._lib.nsfem_default_step_opts(C.byref(o))
        return o

    def step_ipcs(self, opts=None):
        o = opts or self.default_step_opts()
        info = StepInfo()
        self._check(self._lib.nsfem_step_ipcs(self._h, C.byref(o), C.byref(info)))
        return info

    def step_imex(self, opts=None):
        """one IMEX pressure-correction step (set_imex): a CG solve for the diffusion step, then projection and
        velocity correction as step_ipcs"""
        o = opts or self.default_step_opts()
        info = StepInfo()
        self._check(self._lib.nsfem_step_imex(self._h, C.byref(o), C.byref(info)))
        return info

    def imex_info(self):
        """dict(path = None | "generic" | "lattice-kernel" of the last step_imex's right-hand side, lattice_rhs,
        generic_rhs, matrix_builds)"""
        out = (C.c_int64 * 4)()
        self._check(self._lib.nsfem_imex_info(self._h, out))
        return dict(path=(None, "generic", "lattice-kernel")[int(out[0])], lattice_rhs=int(out[1]),
                    generic_rhs=int(out[2]), matrix_builds=int(out[3]))

    def imex_rhs(self, path, convective_form=0):
        """test hook: (right-hand side of the IMEX diffusion step without its Dirichlet rows, c_c N(u1)) formed by
        the "generic" or the "lattice-kernel" path from the current state; the stored vectors stay untouched"""
        n = self.state_size(U0)
        rhs, n1 = np.empty(n), np.empty(n)
        self._check(self._lib.nsfem_imex_rhs(self._h, {"generic": 1, "lattice-kernel": 2}[path], int(convective_form),
                                             _dp(rhs), _dp(n1)))
        return rhs, n1

    def set_imex_rotation(self, treatment, omega_n=None, omega_nm1=None):
        """rotating frames in the IMEX calls: treatment 0 refuse (default), 1 Coriolis term extrapolated with the
        convective term and Euler term in the step-constant vector.  omega_n / omega_nm1: the angular velocity at
        t^n / t^(n-1) (a number in 2D, 3 numbers in 3D); None = the value of set_angular_velocity (steady frame)"""
        ptr = []
        for w in (omega_n, omega_nm1):
            if w is None:
                ptr.append(None)
                continue
            w = np.ascontiguousarray(np.atleast_1d(w), dtype=np.float64)
            assert w.shape == ((1, ) if self.dim == 2 else (3, ))
            ptr.append(w)
        self._check(self._lib.nsfem_set_imex_rotation(self._h, int(treatment), *[None if w is None else _dp(w)
                                                                                 for w in ptr]))

    def imex_rotation_info(self):
        """dict(treatment, rotating_rhs = right-hand sides formed with the rotation folded in, recomputed = times
        the stored N(u2) was formed again because it belonged to another angular velocity)"""
        out = (C.c_int64 * 4)()
        self._check(self._lib.nsfem_imex_rotation_info(self._h, out))
        return dict(treatment=int(out[0]), rotating_rhs=int(out[1]), recomputed=int(out[2]))

    # -- IMEX scalar transport with Boussinesq buoyancy ----------------------------------
    def set_scalar(self, diffusivity, buoyancy=None, convective_form=0):
        """configure the transported P2 scalar: diffusivity kappa, buoyancy vector b (dim entries, None = 0: step_imex
        then runs exactly as without a scalar) and the convective form 0 standard / 1 skew-symmetric"""
        b = None
        if buoyancy is not None:
            b = np.ascontiguousarray(buoyancy, dtype=np.float64)
            assert b.shape == (self.dim, )
        self._check(self._lib.nsfem_set_scalar(self._h, float(diffusivity), None if b is None else _dp(b),
                                               int(convective_form)))

    def step_scalar_imex(self, rtol=1e-12, atol=0.0, max_iter=20000):
        """one IMEX transport step (coefficients: set_imex) T1, T2, u1, u2 -> T0, Jacobi-CG; call it before step_imex
        of the same time step.  Returns the SolveInfo of the CG solve"""
        o = KrylovOpts(rtol, atol, max_iter, 0, 1, 0)
        info = SolveInfo()
        self._check(self._lib.nsfem_step_scalar_imex(self._h, C.byref(o), C.byref(info)))
        return info

    def scalar_convection(self, velocity_slot=U1, scalar_slot=T1, form=0, weight=1.0):
        """test hook: weight * C(u) T (element kernel + node sums; no Dirichlet rows, no stored state touched)"""
        out = np.empty(self.n_p2, dtype=np.float64)
        self._check(self._lib.nsfem_scalar_convection(self._h, int(velocity_slot), int(scalar_slot), int(form),
                                                      float(weight), _dp(out)))
        return out

    def scalar_info(self):
        """dict(matrix_builds, convection_launches, convection_reuses, dictionary) of the transport steps so far;
        dictionary: the last solve's products ran on the stencil-dictionary copy of the matrix"""
        out = (C.c_int64 * 4)()
        self._check(self._lib.nsfem_scalar_info(self._h, out))
        return dict(matrix_builds=int(out[0]), convection_launches=int(out[1]), convection_reuses=int(out[2]),
                    dictionary=bool(out[3]))

    # -- subgrid heat flux in the scalar step ---------------------------------------------
    def set_scalar_sgs(self, prandtl_t):
        """turbulent Prandtl number of the subgrid heat flux kappa_x = nu_x / Pr_t (a subgrid law of
        set_viscosity_law: 1 Smagorinsky, 4 WALE, 5 Vreman): 0 switches the term off (step_scalar_imex runs exactly as without this call), a finite value > 0 on"""
        self._check(self._lib.nsfem_set_scalar_sgs(self._h, float(prandtl_t)))

    def scalar_explicit(self, velocity_slot=U1, scalar_slot=T1, form=0, weight=1.0):
        """test hook: what one launch of the transport step forms, weight * [C(u) T + D(u, T) (+ H(T))] (element kernel
        + node sums; no stored state touched); D with the subgrid heat flux on, H with a thermal body"""
        out = np.empty(self.n_p2, dtype=np.float64)
        self._check(self._lib.nsfem_scalar_explicit(self._h, int(velocity_slot), int(scalar_slot), int(form),
                                                    float(weight), _dp(out)))
        return out

    def scalar_sgs_info(self):
        """dict(active, launches = launches of the kernels with the subgrid term, recomputed = stored vectors formed
        again because Pr_t or, with the term on, the viscosity law changed)"""
        out = (C.c_int64 * 4)()
        self._check(self._lib.nsfem_scalar_sgs_info(self._h, out))
        return dict(active=bool(out[0]), launches=int(out[1]), recomputed=int(out[2]))

    # -- dynamic subgrid heat flux (the partner of viscosity law 8) ------------------------
    def set_scalar_sgs_dynamic(self, enable, ctheta_max=0.2):
        """the eddy diffusivity kappa_x = c_K Delta_K^2 gamma with C_theta from the Germano identity of the scalar
        flux, computed on the device on the level pair of every launch (include/nsfem.h); ``ctheta_max`` the clip.
        Refused while a fixed Pr_t is on; the step then needs viscosity law 8"""
        self._check(self._lib.nsfem_set_scalar_sgs_dynamic(self._h, 1 if enable else 0, float(ctheta_max)))

    def scalar_dynamic_constant(self, velocity_slot=U0, scalar_slot=T0, details=False):
        """C_theta of every averaging group for the pair of slots, [n_groups] (no stored state touched);
        ``details``: also the sums [n_groups, 2] = num, den and the vertex rows [n_p1, 3] = W, PR, RR"""
        return self._dynamic_constant(self._lib.nsfem_scalar_dynamic_constant, (velocity_slot, scalar_slot), details)

    def scalar_diffusivity_cells(self, velocity_slot=U0, scalar_slot=T0):
        """cell means of kappa_x = c_K Delta_K^2 gamma, the constant formed on the pair of slots, [n_cells]"""
        out = np.empty(self.n_cells, dtype=np.float64)
        self._check(self._lib.nsfem_scalar_diffusivity_cells(self._h, int(velocity_slot), int(scalar_slot), _dp(out)))
        return out

    def scalar_dynamic_info(self):
        """dict(active, runs, launches, bytes): the switch, the runs of the procedure, the launches of its three
        kernels and the bytes of its device buffers"""
        out = (C.c_int64 * 4)()
        self._check(self._lib.nsfem_scalar_dynamic_info(self._h, out))
        return dict(active=bool(out[0]), runs=int(out[1]), launches=int(out[2]), bytes=int(out[3]))

    # -- variable viscosity in the IMEX step ---------------------------------------------
    def set_viscosity_law(self, law, params=None):
        """law 0 none (step_imex runs exactly as without this call), 1 Smagorinsky params = (C_s, ), 2 Carreau
        params = (a, lambda, n), 4 WALE params = (C_w, ), 5 Vreman params = (c, ) -- the last two from the whole
        velocity-gradient tensor (include/nsfem.h); 8 dynamic Smagorinsky params = (alpha, cs2_max), its constant
        computed on the device, averaging groups reset to the global one (``set_dynamic_groups``); 3, 6 and 7 are no
        laws; up to four numbers, the rest are zeros"""
        p = np.zeros(4, dtype=np.float64)
        if params is not None:
            given = np.asarray(params, dtype=np.float64).ravel()
            assert given.size <= 4
            p[:given.size] = given
        self._check(self._lib.nsfem_set_viscosity_law(self._h, int(law), _dp(p)))

    def viscosity_residual(self, velocity_slot=U1, weight=1.0):
        """test hook: weight * V(u), interleaved [dim * n_p2] (element kernel + node sums; no stored state touched)"""
        out = np.empty(self.dim * self.n_p2, dtype=np.float64)
        self._check(self._lib.nsfem_viscosity_residual(self._h, int(velocity_slot), float(weight), _dp(out)))
        return out

    def viscosity_cells(self, velocity_slot=U0):
        """cell means of nu_x for the velocity of the slot, [n_cells]"""
        out = np.empty(self.n_cells, dtype=np.float64)
        self._check(self._lib.nsfem_viscosity_cells(self._h, int(velocity_slot), _dp(out)))
        return out

    def viscosity_info(self):
        """dict(law, element_launches, recomputed): the current law, the element-kernel launches so far and how
        often a stored explicit vector had to be recomputed with a law set"""
        out = (C.c_int64 * 4)()
        self._check(self._lib.nsfem_viscosity_info(self._h, out))
        return dict(law=int(out[0]), element_launches=int(out[1]), recomputed=int(out[2]))

    # -- dynamic Smagorinsky (law 8) ------------------------------------------------------
    def set_dynamic_groups(self, n_groups, group_of_vertex):
        """averaging groups of law 8: ``group_of_vertex`` [n_p1] with ids in [0, n_groups); empty groups give cs2 = 0"""
        ids = np.ascontiguousarray(np.asarray(group_of_vertex).ravel(), dtype=np.int32)
        if ids.size != self.n_p1:
            raise ValueError("set_dynamic_groups: %d group ids for %d vertices" % (ids.size, self.n_p1))
        self._check(self._lib.nsfem_set_dynamic_groups(self._h, int(n_groups), ids.ctypes.data_as(C.POINTER(C.c_int32))))

    def dynamic_constant(self, velocity_slot=U0, details=False):
        """C_s^2 of every averaging group for the velocity of the slot, [n_groups] (law 8; no stored state touched);
        ``details``: also the sums [n_groups, 2] = num, den and the vertex rows [n_p1, 3] = W, LM, MM.  With
        Lagrangian averaging (``set_dynamic_averaging``): the stored vertex field of the slot's level, [n_p1]; with
        ``details`` (field, None, vertex rows) -- there are no group sums"""
        if self.dynamic_lagrangian_info()["active"]:
            field = np.empty(self.n_p1, dtype=np.float64)
            vert = np.empty((self.n_p1, 3), dtype=np.float64) if details else None
            self._check(self._lib.nsfem_dynamic_constant(self._h, int(velocity_slot), _dp(field), None,
                                                         _dp(vert) if details else None))
            return (field, None, vert) if details else field
        return self._dynamic_constant(self._lib.nsfem_dynamic_constant, (velocity_slot, ), details)

    def set_dynamic_averaging(self, mode, theta=1.5, cs2_init=0.0256, cs2_floor=1e-12):
        """averaging of law 8: ``mode`` 0 / "groups" -- the averaging groups --, 1 / "lagrangian" -- along fluid path
        lines with the relaxation time theta Delta (I_LM I_MM)^(-1/8) (include/nsfem.h); the state starts from
        I_LM = cs2_init I_MM and I_LM stays above cs2_floor I_MM"""
        mode = {"groups": 0, "lagrangian": 1}.get(mode, mode)
        p = np.array([theta, cs2_init, cs2_floor, 0.0], dtype=np.float64)
        self._check(self._lib.nsfem_set_dynamic_averaging(self._h, int(mode), _dp(p)))

    def dynamic_lagrangian_state(self):
        """[n_p1, 4] = I_LM, I_MM, cs2 of level n, cs2 of level n-1 for restart files; NaN columns do not exist yet"""
        out = np.empty((self.n_p1, 4), dtype=np.float64)
        self._check(self._lib.nsfem_dynamic_lagrangian_state(self._h, 0, _dp(out)))
        return out

    def set_dynamic_lagrangian_state(self, state):
        """columns 0, 1 (I of level n-1) and 3 (cs2 of level n-1) are taken, each unless it is NaN throughout; column 2
        is not read"""
        state = np.ascontiguousarray(state, dtype=np.float64)
        if state.shape != (self.n_p1, 4):
            raise ValueError("set_dynamic_lagrangian_state: shape %r, expected (%d, 4)" % (state.shape, self.n_p1))
        self._check(self._lib.nsfem_dynamic_lagrangian_state(self._h, 1, _dp(state)))

    def dynamic_lagrangian_advance(self, velocity_slot, k, upstream=False):
        """test and output hook: one application of the Lagrangian rules to the stored state on the slot's velocity
        with step size k -> (I' [n_p1, 2], cs2 [n_p1]) or, with ``upstream``, (I', I_up [n_p1, 2], cs2); nothing stored
        is touched"""
        new = np.empty((self.n_p1, 2), dtype=np.float64)
        up = np.empty((self.n_p1, 2), dtype=np.float64) if upstream else None
        cs2 = np.empty(self.n_p1, dtype=np.float64)
        self._check(self._lib.nsfem_dynamic_lagrangian_advance(self._h, int(velocity_slot), float(k), _dp(new),
                                                               _dp(up) if upstream else None, _dp(cs2)))
        return (new, up, cs2) if upstream else (new, cs2)

    def dynamic_lagrangian_info(self):
        """dict(active, have_state, level_formed, have_previous)"""
        out = (C.c_int64 * 4)()
        self._check(self._lib.nsfem_dynamic_lagrangian_info(self._h, out))
        return dict(active=bool(out[0]), have_state=bool(out[1]), level_formed=bool(out[2]), have_previous=bool(out[3]))

    def _dynamic_constant(self, call, slots, details):
        """one run of the Germano-Lilly procedure through ``call`` on ``slots``: the constant of every group, with
        ``details`` the sums and the vertex rows as well"""
        n = max(self.dynamic_info()["groups"], 1)     # (law 8 never set: let the driver say so)
        const = np.empty(n, dtype=np.float64)
        sums = np.empty((n, 2), dtype=np.float64) if details else None
        vert = np.empty((self.n_p1, 3), dtype=np.float64) if details else None
        self._check(call(self._h, *map(int, slots), _dp(const), _dp(sums) if details else None,
                         _dp(vert) if details else None))
        return (const, sums, vert) if details else const

    def dynamic_info(self):
        """dict(groups, runs, launches, bytes): the averaging groups, the runs of the procedure, the launches of its
        three kernels and the bytes of its device buffers"""
        out = (C.c_int64 * 4)()
        self._check(self._lib.nsfem_dynamic_info(self._h, out))
        return dict(groups=int(out[0]), runs=int(out[1]), launches=int(out[2]), bytes=int(out[3]))

    # -- immersed bodies in the IMEX step (volume penalisation) --------------------------
    def _body_array(self, bodies):
        """rows (kind, centre, size, velocity, angular) -> a C array of nsfem_body; short vectors are padded with
        zeros, a scalar angular velocity (2D) goes to the z component"""
        arr = (Body * max(len(bodies), 1))()
        for b, row in zip(arr, bodies):
            kind, centre, size, velocity, angular = row
            b.kind = int(kind)
            for name, val in (("centre", centre), ("size", size), ("velocity", velocity)):
                v = np.atleast_1d(np.asarray(val, dtype=np.float64)).ravel()
                assert v.size <= 3
                for a in range(v.size):
                    getattr(b, name)[a] = v[a]
            w = np.atleast_1d(np.asarray(angular, dtype=np.float64)).ravel()
            assert w.size in (1, 3)
            if w.size == 1:
                b.angular[2] = w[0]
            else:
                b.angular[0], b.angular[1], b.angular[2] = w
        return arr

    def set_bodies(self, bodies, eta=1.0, smoothing=0.0):
        """bodies: rows (kind, centre, size, velocity, angular); an empty list removes them"""
        bodies = list(bodies)
        self._check(self._lib.nsfem_set_bodies(self._h, len(bodies), self._body_array(bodies), float(eta),
                                               float(smoothing)))

    def move_bodies(self, bodies):
        """pose and velocity of the bodies at t^n (same count and kinds as set); once per step"""
        bodies = list(bodies)
        self._check(self._lib.nsfem_move_bodies(self._h, len(bodies), self._body_array(bodies)))

    def body_residual(self, velocity_slot=U1, weight=1.0):
        """test hook: weight * B(u), interleaved [dim * n_p2] (element kernel + node sums; no stored state touched)"""
        out = np.empty(self.dim * self.n_p2, dtype=np.float64)
        self._check(self._lib.nsfem_body_residual(self._h, int(velocity_slot), float(weight), _dp(out)))
        return out

    def body_mask_cells(self):
        """cell means of chi, [n_cells]"""
        out = np.empty(self.n_cells, dtype=np.float64)
        self._check(self._lib.nsfem_body_mask_cells(self._h, _dp(out)))
        return out

    def body_forces(self, velocity_slot=U0):
        """[n_bodies, 1 + dim + ntorque]: volume, force on the body, torque about its centre (2D: 1, 3D: 3)"""
        n = self.body_info()["bodies"]
        out = np.empty((max(n, 1), 4 if self.dim == 2 else 7), dtype=np.float64)
        self._check(self._lib.nsfem_body_forces(self._h, int(velocity_slot), _dp(out)))
        return out[:n]

    def body_info(self):
        """dict(bodies, element_launches, recomputed): the number of bodies set, the element-kernel launches so far
        and how often a stored explicit vector had to be recomputed with bodies set"""
        out = (C.c_int64 * 4)()
        self._check(self._lib.nsfem_body_info(self._h, out))
        return dict(bodies=int(out[0]), element_launches=int(out[1]), recomputed=int(out[2]))

    # -- wall-stress models (the explicit term W(u) of the IMEX step) ---------------------
    def set_wall_model(self, law, params=None, facet_cell=(), facet_local=(), sample_cell=(), sample_lambda=(),
                       sample_y=(), wall_velocity=None):
        """law 0 none, 1 Werner-Wengle (A, B), 2 Reichardt (kappa, C); facet_cell, facet_local [nf], sample_cell
        [nf, NQ], sample_lambda [nf, NQ, dim + 1], sample_y [nf, NQ], wall_velocity [nf, dim] or None (the arrays of
        ``wall_models.WallModel.build``).  Law 0 or no facet switches the term off"""
        fc = np.ascontiguousarray(facet_cell, dtype=np.int32).ravel()
        if int(law) == 0 or fc.size == 0:
            self._check(self._lib.nsfem_set_wall_model(self._h, 0, None, 0, None, None, None, None, None, None))
            return
        nq, nv = (3 if self.dim == 2 else 6), self.dim + 1
        fl = np.ascontiguousarray(facet_local, dtype=np.int32).ravel()
        sc = np.ascontiguousarray(sample_cell, dtype=np.int32).ravel()
        sl = np.ascontiguousarray(sample_lambda, dtype=np.float64).ravel()
        sy = np.ascontiguousarray(sample_y, dtype=np.float64).ravel()
        assert fl.size == fc.size and sc.size == fc.size * nq and sy.size == sc.size and sl.size == sc.size * nv
        p = np.zeros(4)
        params = tuple(params or ())
        p[:len(params)] = params
        uw = None
        if wall_velocity is not None:
            uw = np.ascontiguousarray(wall_velocity, dtype=np.float64).ravel()
            assert uw.size == fc.size * self.dim
        self._check(self._lib.nsfem_set_wall_model(self._h, int(law), _dp(p), fc.size, _ip(fc), _ip(fl), _ip(sc),
                                                   _dp(sl), _dp(sy), None if uw is None else _dp(uw)))

    def wall_model_residual(self, velocity_slot=U1, weight=1.0):
        """test hook: weight * W(u), interleaved [dim * n_p2] (facet kernel + node sums; no stored state touched)"""
        out = np.empty(self.dim * self.n_p2, dtype=np.float64)
        self._check(self._lib.nsfem_wall_model_residual(self._h, int(velocity_slot), float(weight), _dp(out)))
        return out

    def wall_model_facets(self, velocity_slot=U0):
        """[n_facets, dim + 4] in input order: |f|, int tau_w [dim], int u_tau, int y+, max y+"""
        n = self.wall_model_info()["facets"]
        out = np.empty((max(n, 1), self.dim + 4), dtype=np.float64)
        self._check(self._lib.nsfem_wall_model_facets(self._h, int(velocity_slot), _dp(out)))
        return out[:n]

    def wall_model_info(self):
        """dict(facets, launches, recomputed, law): modelled facets, facet-kernel launches so far, how often a stored
        explicit vector had to be recomputed with a model set, and the law"""
        out = (C.c_int64 * 4)()
        self._check(self._lib.nsfem_wall_model_info(self._h, out))
        return dict(facets=int(out[0]), launches=int(out[1]), recomputed=int(out[2]), law=int(out[3]))

    # -- heated immersed bodies (scalar penalisation in the convection kernel) -----------
    def set_body_temperatures(self, thermal, temperatures, eta_scalar=1.0):
        """flag (0 passive, 1 thermal) and temperature per body set, one eta_T; empty lists remove them"""
        flags = np.ascontiguousarray(thermal, dtype=np.int32).ravel()
        values = np.ascontiguousarray(temperatures, dtype=np.float64).ravel()
        assert flags.size == values.size
        self._check(self._lib.nsfem_set_body_temperatures(self._h, flags.size, _ip(flags), _dp(values),
                                                          float(eta_scalar)))

    def body_scalar_residual(self, velocity_slot=U1, scalar_slot=T1, form=0, weight=1.0, pose=0):
        """test hook: weight * (C(u) T + H(T)), [n_p2], from the fused element launch; pose 0 the bodies at t^n, 1 at
        t^(n-1); no stored state touched"""
        out = np.empty(self.n_p2, dtype=np.float64)
        self._check(self._lib.nsfem_body_scalar_residual(self._h, int(velocity_slot), int(scalar_slot), int(form),
                                                         float(weight), int(pose), _dp(out)))
        return out

    def body_heat(self, scalar_slot=T0):
        """[n_bodies, 3]: volume, heat rate the body takes from the fluid (0 for passive bodies), int chi_s T"""
        n = self.body_info()["bodies"]
        out = np.empty((max(n, 1), 3), dtype=np.float64)
        self._check(self._lib.nsfem_body_heat(self._h, int(scalar_slot), _dp(out)))
        return out[:n]

    def body_heat_info(self):
        """dict(thermal, fused_launches, recomputed): bodies with flag 1, fused element launches so far and how often
        a stored scalar vector had to be recomputed because the thermal data or the body set changed"""
        out = (C.c_int64 * 4)()
        self._check(self._lib.nsfem_body_heat_info(self._h, out))
        return dict(thermal=int(out[0]), fused_launches=int(out[1]), recomputed=int(out[2]))

    def step_bdf(self, opts=None):
        o = opts or self.default_step_opts()
        info = StepInfo()
        self._check(self._lib.nsfem_step_bdf(self._h, C.byref(o), C.byref(info)))
        return info

    def comm_stats(self, reset=False):
        """{allreduce_calls, allreduce_bytes, exchanges, exchange_bytes} of this rank"""
        out = (C.c_int64 * 4)()
        self._check(self._lib.nsfem_comm_stats(self._h, out, 1 if reset else 0))
        return dict(zip(("allreduce_calls", "allreduce_bytes", "exchanges", "exchange_bytes"), [int(v) for v in out]))

    def set_overlap(self, enable):
        """halo exchanges on the communicator's stream under the interior rows of the products"""
        self._check(self._lib.nsfem_set_overlap(self._h, 1 if enable else 0))

    def comm_overlapped(self, reset=False):
        out = C.c_int64()
        self._check(self._lib.nsfem_comm_overlapped(self._h, C.byref(out), 1 if reset else 0))
        return int(out.value)

    def mg_set_halo_mode(self, relaxed):
        """partitioned multigrid cycles: False / "exact" one halo exchange per product (the serial cycle),
        True / "relaxed" one per smoothing sequence (frozen ghosts in between)"""
        if isinstance(relaxed, str):
            relaxed = {"exact": False, "relaxed": True}[relaxed]
        self._check(self._lib.nsfem_mg_set_halo_mode(self._h, 1 if relaxed else 0))

    def mg_set_truncation(self, max_ratio, coarse_tol=0.1):
        self._check(self._lib.nsfem_mg_set_truncation(self._h, float(max_ratio), float(coarse_tol)))

    def advance(self, scheme=0):
        self._check(self._lib.nsfem_advance(self._h, scheme))

    def shift_mean_pressure(self, target):
        out = C.c_double()
        self._check(self._lib.nsfem_shift_mean_pressure(self._h, float(target), C.byref(out)))
        return out.value

    def mass_solve(self, field, b, rtol=1e-13, max_iter=2000):
        b = np.ascontiguousarray(b, dtype=np.float64)
        x = np.empty_like(b)
        o = KrylovOpts(rtol, 0.0, max_iter, 0, 1, 0)
        info = SolveInfo()
        self._check(self._lib.nsfem_mass_solve(self._h, field, _dp(b), _dp(x), C.byref(o),
                                               C.byref(info)))
        return x

    def poisson_solve(self, rhs, dirichlet_dofs, rtol=1e-12, max_iter=20000):
        """post-processing P1 Poisson solve with homogeneous Dirichlet dofs (may be empty)"""
        rhs = np.ascontiguousarray(rhs, dtype=np.float64)
        assert rhs.size == self.n_p1
        d = np.ascontiguousarray(dirichlet_dofs, dtype=np.int32)
        x = np.empty(self.n_p1, dtype=np.float64)
        o = KrylovOpts(rtol, 1e-300, max_iter, 0, 1, 0)
        info = SolveInfo()
        self._check(self._lib.nsfem_poisson_solve(self._h, _dp(rhs), d.size, _ip(d), _dp(x), C.byref(o),
                                                  C.byref(info)))
        return x

    def mg_add_level(self, coords, cells, p_rowptr, p_col, p_val, ghost=None, halo=None, dofmap=None, nested=None):
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        cells = np.ascontiguousarray(cells, dtype=np.int32)
        rp = np.ascontiguousarray(p_rowptr, dtype=np.int32)
        pc = np.ascontiguousarray(p_col, dtype=np.int32)
        pv = np.ascontiguousarray(p_val, dtype=np.float64)
        g = None if ghost is None else np.ascontiguousarray(ghost, dtype=np.uint8)
        gp = g.ctypes.data_as(C.POINTER(C.c_uint8)) if g is not None else None
        dm = None if dofmap is None else np.ascontiguousarray(dofmap, dtype=np.int32)
        assert dm is None or dm.shape == cells.shape
        d = MgLevelDesc(coords.shape[0], cells.shape[0], _dp(coords), _ip(cells), rp.size - 1,
                        _ip(rp), _ip(pc), _dp(pv), gp, Halo.from_dict(halo),
                        _ip(dm) if dm is not None else None, int(dm.max()) + 1 if dm is not None else 0,
                        0 if nested is None else (1 if nested else 2))
        self._check(self._lib.nsfem_mg_add_level(self._h, C.byref(d)))

    def mg_set_schur_operator(self, level, csr, singular):
        """Level ``level`` of the algebraic Schur-complement Laplacian (scipy CSR, sorted)."""
        csr = csr.tocsr()
        csr.sort_indices()
        rp = np.ascontiguousarray(csr.indptr, dtype=np.int32)
        ci = np.ascontiguousarray(csr.indices, dtype=np.int32)
        cv = np.ascontiguousarray(csr.data, dtype=np.float64)
        self._check(self._lib.nsfem_mg_set_schur_operator(self._h, int(level), csr.shape[0],
                                                          _ip(rp), _ip(ci), _dp(cv),
                                                          1 if singular else 0))

    def smoother_info(self):
        """finest-level smoothing kernel of the velocity multigrid: dict(kind, stencils, longest_row,
        csr_bytes) -- kind "csr-stream" | "sell-64" | "stencil-dictionary" """
        out = (C.c_int64 * 4)()
        self._check(self._lib.nsfem_smoother_info(self._h, out))
        return dict(kind=("csr-stream", "sell-64", "stencil-dictionary", "stencil-dictionary")[int(out[0])],
                    multistep_lattice_kernel=int(out[0]) == 3, stencils=int(out[1]),
                    longest_row=abs(int(out[2])), bitwise_exact=int(out[2]) < 0, csr_bytes=int(out[3]))

    def mg_apply(self, which, r):
        """one cycle z = M^-1 r of the pressure (which=0) or velocity (which=1) multigrid preconditioner; which=2: the
        fast-diagonalisation solve z = A^+ r (strip factors: a collective, every rank calls it; 3D factors: z = T^+ r);
        which=3: the Schur hierarchy of the monolithic block preconditioner, which=4: its pressure mass smoother"""
        r = np.ascontiguousarray(r, dtype=np.float64)
        z = np.zeros_like(r)
        self._check(self._lib.nsfem_mg_apply(self._h, int(which), _dp(r), _dp(z)))
        return z

    def monolithic_apply(self, what, x, matrix_free=False):
        """what=0: y = MixedOp x, the operator of the monolithic step's linear solve about U0 (convective form and
        Picard flag: set_convective_form); what=1: y = BlockPrec x, its block preconditioner; mixed host vectors"""
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.size == self.n_velocity + self.n_p1
        y = np.zeros_like(x)
        self._check(self._lib.nsfem_monolithic_apply(self._h, int(what), 1 if matrix_free else 0, _dp(x), _dp(y)))
        return y

    def poisson_set_fast_diag(self, factors, first_line=None):
        """factors of poisson_fd.factors(): the projection step may then run with Krylov option precond = 3.
        first_line (partitioned strips): the factors belong to the GLOBAL lattice, this context's pressure space is
        its lines first_line, first_line + 1, ... (ghost lines included)"""
        inv = np.ascontiguousarray(factors["inv"], dtype=np.float64)
        vx = np.ascontiguousarray(factors["Vx"], dtype=np.float64)
        vy = np.ascontiguousarray(factors["Vy"], dtype=np.float64)
        H, W = inv.shape
        assert vx.shape == (W, W) and vy.shape == (H, H)
        if first_line is None:
            self._check(self._lib.nsfem_poisson_set_fast_diag(self._h, W, H, _dp(vx), _dp(vy), _dp(inv)))
        else:
            self._check(self._lib.nsfem_poisson_set_fast_diag_rows(self._h, W, H, int(first_line), _dp(vx), _dp(vy),
                                                                   _dp(inv)))

    def poisson_set_fast_diag_3d(self, factors, first_plane=None):
        """factors of poisson_fd.factors_3d(): the projection step may then run with Krylov option precond = 3 -- a
        direct solve when factors["exact"], CG preconditioned by T^+ otherwise.  Replaces factors set before.
        first_plane (partitioned slabs): the factors belong to the GLOBAL lattice, this context's pressure space is
        its planes (first_plane + i) mod N_z (ghost planes included); the solve is then a collective"""
        inv = np.ascontiguousarray(factors["inv"], dtype=np.float64)
        vx, vy, vz = (np.ascontiguousarray(factors[k], dtype=np.float64) for k in ("Vx", "Vy", "Vz"))
        Nz, Ny, Nx = inv.shape
        assert vx.shape == (Nx, Nx) and vy.shape == (Ny, Ny) and vz.shape == (Nz, Nz)
        exact = 1 if factors["exact"] else 0
        if first_plane is None:
            self._check(self._lib.nsfem_poisson_set_fast_diag_3d(self._h, Nx, Ny, Nz, _dp(vx), _dp(vy), _dp(vz),
                                                                 _dp(inv), exact))
        else:
            self._check(self._lib.nsfem_poisson_set_fast_diag_3d_planes(self._h, Nx, Ny, Nz, int(first_plane), _dp(vx),
                                                                        _dp(vy), _dp(vz), _dp(inv), exact))

    def poisson_fast_diag_3d_info(self):
        """dict(shape=(Nx, Ny, Nz), exact, applications, solves) of the 3D factors (zeros when none are set);
        applications counts the host-issued applications of T^+ (CG iterations replayed from a captured graph
        apply it without the host), solves the projection solves that ran with the factors"""
        out = (C.c_int64 * 6)()
        self._check(self._lib.nsfem_poisson_fast_diag_3d_info(self._h, out))
        return dict(shape=(int(out[0]), int(out[1]), int(out[2])), exact=bool(out[3]), applications=int(out[4]),
                    solves=int(out[5]))

    def mg_lattice_info(self, which):
        """dict(lattice_levels, lattice_launches, levels, ghost_lines): the multi-step lattice kernel on the Poisson
        (which = 0) / velocity (1) hierarchy; on partitioned strips it runs in relaxed halo mode only.  which = 3 / 4:
        the Schur hierarchy / the pressure mass smoother of the monolithic block preconditioner (as mg_apply)"""
        out = (C.c_int64 * 4)()
        self._check(self._lib.nsfem_mg_info(self._h, (3 + int(which)) if int(which) >= 3 else 2 + int(which), out))
        return dict(lattice_levels=int(out[0]), lattice_launches=int(out[1]), levels=int(out[2]),
                    ghost_lines=(int(out[3]) // 256, int(out[3]) % 256))

    def mg_set_schur_mode(self, additive):
        """partitioned meshes: the Schur operators set afterwards are this rank's additive parts"""
        self._check(self._lib.nsfem_mg_set_schur_mode(self._h, 1 if additive else 0))

    def comm_allreduce(self, values, op="sum"):
        """sum / max over the ranks of a few host doubles (a copy; single contexts: unchanged)"""
        v = np.ascontiguousarray(np.atleast_1d(values), dtype=np.float64).copy()
        self._check(self._lib.nsfem_comm_allreduce(self._h, _dp(v), int(v.size), 1 if op == "max" else 0))
        return v

    def mg_add_global_level(self, coords, cells, p_rowptr, p_col, p_val, dofmap=None):
        """coarser level of the replicated hierarchy below the global coarsest mesh"""
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        cells = np.ascontiguousarray(cells, dtype=np.int32)
        rp = np.ascontiguousarray(p_rowptr, dtype=np.int32)
        pc = np.ascontiguousarray(p_col, dtype=np.int32)
        pv = np.ascontiguousarray(p_val, dtype=np.float64)
        d = MgLevelDesc(coords.shape[0], cells.shape[0], _dp(coords), _ip(cells), rp.size - 1,
                        _ip(rp), _ip(pc), _dp(pv), None, Halo.from_dict(None), None, 0)
        if dofmap is not None:
            dm = np.ascontiguousarray(dofmap, dtype=np.int32)
            assert dm.shape == cells.shape
            d.dofmap, d.n_dofs = _ip(dm), int(dm.max()) + 1
        self._check(self._lib.nsfem_mg_add_global_level(self._h, C.byref(d)))

    def mg_set_global_coarse(self, coords, cells, offset, dofmap=None):
        coords = np.ascontiguousarray(coords, dtype=np.float64)
        cells = np.ascontiguousarray(cells, dtype=np.int32)
        if dofmap is not None:                     # constrained (periodic) global coarse space
            dm = np.ascontiguousarray(dofmap, dtype=np.int32)
            assert dm.shape == cells.shape
            self._check(self._lib.nsfem_mg_set_global_coarse_constrained(
                self._h, coords.shape[0], cells.shape[0], _dp(coords), _ip(cells), _ip(dm),
                int(dm.max()) + 1, int(offset)))
            return
        self._check(self._lib.nsfem_mg_set_global_coarse(self._h, coords.shape[0], cells.shape[0],
                                                         _dp(coords), _ip(cells), int(offset)))

    # -- multi-GPU --------------------------------------------------------------------
    def set_partition(self, rank, size, p2_ghost, p1_ghost, p2_halo, p1_halo, n_p2_global,
                      n_p1_global, periodic=False):
        g2 = np.ascontiguousarray(p2_ghost, dtype=np.uint8)
        g1 = np.ascontiguousarray(p1_ghost, dtype=np.uint8)
        assert g2.size == self.n_p2 and g1.size == self.n_p1
        d = PartitionDesc(rank, size, g2.ctypes.data_as(C.POINTER(C.c_uint8)),
                          g1.ctypes.data_as(C.POINTER(C.c_uint8)), Halo.from_dict(p2_halo),
                          Halo.from_dict(p1_halo), int(n_p2_global), int(n_p1_global), 1 if periodic else 0)
        self._check(self._lib.nsfem_set_partition(self._h, C.byref(d)))

    def set_halo_lists(self, target, lists):
        """index-list halo of an unstructured partition; ``lists`` = dict(neighbour, send_ptr,
        send_idx, recv_ptr, recv_idx); target 0 P2 nodes, 1 P1 nodes, 2 + l multigrid level l"""
        nb = np.ascontiguousarray(lists["neighbour"], dtype=np.int32)
        sp = np.ascontiguousarray(lists["send_ptr"], dtype=np.int64)
        si = np.ascontiguousarray(lists["send_idx"], dtype=np.int32)
        rp = np.ascontiguousarray(lists["recv_ptr"], dtype=np.int64)
        ri = np.ascontiguousarray(lists["recv_idx"], dtype=np.int32)
        assert sp.size == nb.size + 1 and rp.size == nb.size + 1 and sp[-1] == si.size and rp[-1] == ri.size
        p64 = C.POINTER(C.c_int64)
        d = HaloLists(int(nb.size), _ip(nb), sp.ctypes.data_as(p64), _ip(si), rp.ctypes.data_as(p64), _ip(ri))
        self._check(self._lib.nsfem_set_halo_lists(self._h, int(target), C.byref(d)))

    def mg_set_global_index(self, local_to_global):
        idx = np.ascontiguousarray(local_to_global, dtype=np.int32)
        self._check(self._lib.nsfem_mg_set_global_index(self._h, int(idx.size), _ip(idx)))

    def attach_local_comm(self, group, rank):
        self._check(self._lib.nsfem_comm_attach_local(self._h, group, rank))

    def attach_shm_comm(self, name, rank, size, slot_bytes=0):
        """one process per rank on a SHARED device: host-staged shared-memory communicator"""
        self._check(self._lib.nsfem_comm_attach_shm(self._h, name.encode(), rank, size, int(slot_bytes)))

    def attach_rccl_comm(self, unique_id, rank, size):
        assert len(unique_id) == 128
        self._check(self._lib.nsfem_comm_attach_rccl(self._h, unique_id, rank, size))

    def mg_finalize(self, degree=2, eig_ratio=4.0, coarse_dense_max=1200):
        o = MgOpts(int(degree), int(coarse_dense_max), float(eig_ratio))
        self._check(self._lib.nsfem_mg_finalize(self._h, C.byref(o)))

    def synchronize(self):
        self._check(self._lib.nsfem_synchronize(self._h))

    # -- operator introspection ---------------------------------------------------
    def operator_csr(self, op):
        """scipy CSR copy of a device operator (parity tests)."""
        import scipy.sparse as sp
        nr, ncol, nnz = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.nsfem_operator_shape(self._h, op, C.byref(nr), C.byref(ncol),
                                                   C.byref(nnz)))
        rowptr = np.empty(nr.value + 1, dtype=np.int32)
        col = np.empty(nnz.value, dtype=np.int32)
        val = np.empty(nnz.value, dtype=np.float64)
        self._check(self._lib.nsfem_operator_export(self._h, op, _ip(rowptr), _ip(col), _dp(val)))
        return sp.csr_matrix((val, col, rowptr), shape=(nr.value, ncol.value))

    def operator_diagonal(self, op):
        """diagonal of a square scalar device operator (no matrix export)"""
        nr, ncol, nnz = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.nsfem_operator_shape(self._h, op, C.byref(nr), C.byref(ncol), C.byref(nnz)))
        out = np.empty(nr.value, dtype=np.float64)
        self._check(self._lib.nsfem_operator_diagonal(self._h, op, _dp(out)))
        return out

    def operator_nnz(self, op):
        """block-nonzeros x block size of a device operator"""
        nr, ncol, nnz = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.nsfem_operator_shape(self._h, op, C.byref(nr), C.byref(ncol),
                                                   C.byref(nnz)))
        return nnz.value

    def operator_apply(self, op, x):
        if op == OP_MOMENTUM_JAC_MF:                 # matrix-free Jacobian at u = USTAR
            x = np.ascontiguousarray(x, dtype=np.float64)
            assert x.size == self.n_velocity
            y = np.empty(self.n_velocity, dtype=np.float64)
            self._check(self._lib.nsfem_operator_apply(self._h, op, _dp(x), _dp(y)))
            return y
        nr, ncol, nnz = C.c_int64(), C.c_int64(), C.c_int64()
        self._check(self._lib.nsfem_operator_shape(self._h, op, C.byref(nr), C.byref(ncol),
                                                   C.byref(nnz)))
        x = np.ascontiguousarray(x, dtype=np.float64)
        assert x.size == ncol.value
        y = np.empty(nr.value, dtype=np.float64)
        self._check(self._lib.nsfem_operator_apply(self._h, op, _dp(x), _dp(y)))
        return y

    def kernel_apply(self, space, nv, x, a=1.0, b_coef=0.0, family=0, epilogue=0, b=None, d=None, mask=None,
                     maskmode=0, steps=0, c1=(), c2=(), ghost=0, ident=False, from_zero=False,
                     with_residual=False, dict_ok=True, xc=None, rf=None, gh_lo=0, gh_hi=0, gh_zero=False,
                     tile_lines=0, fixed=-1, want_d=True):
        """test hook (nsfem_kernel_apply): product / residual / smoothing sequence of a M + b K through a chosen
        kernel family; returns dict(y, d, r, used_family, dict_entries, dict_exact, lattice_w).  Lattice kernel
        (family 4) only: xc (fused prolongation; x may then be None), rf (fused restriction: the stored right-hand
        side comes back as b_formed), frozen ghost lines, a forced tile height and the fixed-offset stages on / off;
        the launch geometry comes back as lattice_tile_lines, lattice_tx, lattice_ty, lattice_tiles,
        lattice_fixed_shape, the launch kind as lattice_kind (want_d=False: no direction stored, d comes back None)"""
        t = KernelTest()
        t.space, t.nv, t.family, t.epilogue, t.steps = int(space), int(nv), int(family), int(epilogue), int(steps)
        t.maskmode, t.ghost, t.ident = int(maskmode), int(ghost), 1 if ident else 0
        t.from_zero, t.with_residual, t.dict_ok = 1 if from_zero else 0, 1 if with_residual else 0, 1 if dict_ok else 0
        t.a, t.b_coef = float(a), float(b_coef)
        for k, v in enumerate(c1):
            t.c1[k] = float(v)
        for k, v in enumerate(c2):
            t.c2[k] = float(v)
        keep = []

        def arr(v, dtype=np.float64):
            if v is None:
                return None
            v = np.ascontiguousarray(v, dtype=dtype)
            keep.append(v)
            return v
        x = arr(x)
        n = x.size if x is not None else (self.n_p2 if space == 0 else self.n_p1) * int(nv)
        bb, dd, mm = arr(b), arr(d), arr(mask, np.uint8)
        y, d_out, r_out, b_formed = np.empty(n), np.empty(n), np.empty(n), np.zeros(n)
        t.y, t.r_out = _dp(y), _dp(r_out)
        if want_d:
            t.d_out = _dp(d_out)
        else:
            d_out = None
        if x is not None:
            t.x = _dp(x)
        xcc, rff = arr(xc), arr(rf)
        if xcc is not None:
            t.xc = _dp(xcc)
        if rff is not None:
            t.rf, t.b_formed = _dp(rff), _dp(b_formed)
        t.gh_lo, t.gh_hi, t.gh_zero = int(gh_lo), int(gh_hi), 1 if gh_zero else 0
        t.tile_lines, t.fixed = int(tile_lines), int(fixed)
        if bb is not None:
            assert bb.size == n
            t.b = _dp(bb)
        if dd is not None:
            assert dd.size == n
            t.d = _dp(dd)
        if mm is not None:
            assert mm.size == n
            t.mask = mm.ctypes.data_as(C.POINTER(C.c_uint8))
        self._check(self._lib.nsfem_kernel_apply(self._h, C.byref(t)))
        return dict(y=y, d=d_out, r=r_out, used_family=int(t.used_family), dict_entries=int(t.dict_entries),
                    dict_exact=bool(t.dict_exact), lattice_w=int(t.lattice_w),
                    b_formed=b_formed if rff is not None else None,
                    lattice_tile_lines=int(t.lattice_tile_lines), lattice_tx=int(t.lattice_tx),
                    lattice_ty=int(t.lattice_ty), lattice_tiles=int(t.lattice_tiles),
                    lattice_fixed_shape=int(t.lattice_fixed_shape), lattice_kind=int(t.lattice_kind))

    def lattice_restrict(self, nv, w, h, rf, mask1=None, mask2=None, levels=1):
        """test hook (nsfem_lattice_restrict): levels = 1: b1 = R rf (k_restrict_lattice) onto the w x h lattice;
        levels = 2: b1 = R rf, b2 = R b1 (k_restrict_lattice2), w x h the coarsest lattice.  Returns (b1, b2)."""
        w1, h1 = (w, h) if levels == 1 else (2 * w - 1, 2 * h - 1)
        f = np.ascontiguousarray(rf, dtype=np.float64)
        assert f.size == (2 * w1 - 1) * (2 * h1 - 1) * nv
        m1 = None if mask1 is None else np.ascontiguousarray(mask1, dtype=np.uint8)
        m2 = None if mask2 is None else np.ascontiguousarray(mask2, dtype=np.uint8)
        assert m1 is None or m1.size == w1 * h1 * nv
        assert m2 is None or m2.size == w * h * nv
        b1 = np.empty(w1 * h1 * nv)
        b2 = np.empty(w * h * nv) if levels == 2 else None
        up = C.POINTER(C.c_uint8)
        self._check(self._lib.nsfem_lattice_restrict(
            self._h, int(nv), int(levels), int(w), int(h), _dp(f),
            None if m1 is None else m1.ctypes.data_as(up), None if m2 is None else m2.ctypes.data_as(up),
            _dp(b1), None if b2 is None else _dp(b2)))
        return b1, b2

    def set_preconditioner_shift(self, shift):
        self._check(self._lib.nsfem_set_preconditioner_shift(self._h, float(shift)))

    def set_angular_velocity(self, omega, omega_dot=0.0):
        if np.ndim(omega) > 0:                       # 3D: vectors
            w = np.ascontiguousarray(omega, dtype=np.float64)
            wd = np.ascontiguousarray(omega_dot if np.ndim(omega_dot) > 0 else np.zeros(3), dtype=np.float64)
            assert w.shape == (3, ) and wd.shape == (3, )
            self._check(self._lib.nsfem_set_angular_velocity_3d(self._h, _dp(w), _dp(wd)))
            return
        self._check(self._lib.nsfem_set_angular_velocity(self._h, float(omega), float(omega_dot)))

    def boundary_force(self, facet_cell, facet_local, nu, symmetric=1.0, velocity_slot=U0,
                       pressure_slot=P):
        """(force [dim], flux, measure) over the given boundary facets:
        force = int (-p n + nu (grad u + symmetric grad u^T) n) dS, flux = int u.n dS"""
        fc = np.ascontiguousarray(facet_cell, dtype=np.int32)
        fl = np.ascontiguousarray(facet_local, dtype=np.int32)
        assert fc.shape == fl.shape and fc.ndim == 1
        out = np.zeros(self.dim + 2)
        self._check(self._lib.nsfem_boundary_force(self._h, int(velocity_slot), int(pressure_slot),
                                                   fc.size, _ip(fc), _ip(fl), float(nu),
                                                   float(symmetric), _dp(out)))
        return out[:self.dim].copy(), float(out[self.dim]), float(out[self.dim + 1])

    def volume_functionals(self, velocity_slot=U0, pressure_slot=P, ref_velocity=None, ref_pressure=None,
                           cell_flags=None):
        """integrals over the cells with a nonzero flag (None: all cells) of (v, q) = (u, p) of the two slots, or of
        (u - ref_velocity, p - ref_pressure) where a reference (host vector in the slot's layout) is given: dict of
        measure, u_l2_sq = int v.v, grad_u_l2_sq = int grad v : grad v, curl_l2_sq, div_l2_sq, momentum [dim] = int v,
        p_integral, p_l2_sq, grad_p_l2_sq, and values = the N_FUNCTIONALS doubles as returned.  One device call; on
        contexts with a communicator every rank calls and receives the global sums."""
        ru = rp = fl = None
        if ref_velocity is not None:
            ru = np.ascontiguousarray(ref_velocity, dtype=np.float64)
            if ru.shape != (self.n_velocity, ):
                raise ValueError("ref_velocity: expected %d values, got shape %s" % (self.n_velocity, ru.shape))
        if ref_pressure is not None:
            rp = np.ascontiguousarray(ref_pressure, dtype=np.float64)
            if rp.shape != (self.n_p1, ):
                raise ValueError("ref_pressure: expected %d values, got shape %s" % (self.n_p1, rp.shape))
        if cell_flags is not None:
            fl = np.ascontiguousarray(np.asarray(cell_flags) != 0, dtype=np.uint8)
            if fl.shape != (self.n_cells, ):
                raise ValueError("cell_flags: expected %d flags, got shape %s" % (self.n_cells, fl.shape))
        out = np.zeros(N_FUNCTIONALS)
        self._check(self._lib.nsfem_volume_functionals(
            self._h, int(velocity_slot), int(pressure_slot), None if ru is None else _dp(ru),
            None if rp is None else _dp(rp), None if fl is None else fl.ctypes.data_as(C.POINTER(C.c_uint8)),
            _dp(out)))
        return dict(measure=float(out[0]), u_l2_sq=float(out[1]), grad_u_l2_sq=float(out[2]),
                    curl_l2_sq=float(out[3]), div_l2_sq=float(out[4]), momentum=out[5:5 + self.dim].copy(),
                    p_integral=float(out[8]), p_l2_sq=float(out[9]), grad_p_l2_sq=float(out[10]), values=out)

    # -- point location / evaluation / tracer particles (csrc/points.hip) ------------
    def set_point_locator(self, origin, inv_h, nbins, bin_ptr, bin_cells):
        """upload the bins of point_locator.build_bins (once per context; ``set_point_locator(**build_bins(..))``)"""
        o = np.ascontiguousarray(origin, dtype=np.float64)
        ih = np.ascontiguousarray(inv_h, dtype=np.float64)
        nb = np.ascontiguousarray(nbins, dtype=np.int32)
        bp = np.ascontiguousarray(bin_ptr, dtype=np.int32)
        bc = np.ascontiguousarray(bin_cells, dtype=np.int32)
        if not (o.shape == ih.shape == nb.shape == (self.dim, )):
            raise ValueError("origin, inv_h, nbins: expected %d entries each" % self.dim)
        if bp.shape != (int(np.prod(nb.astype(np.int64))) + 1, ) or bc.shape != (int(bp[-1]), ):
            raise ValueError("bin_ptr / bin_cells do not match nbins")
        self._check(self._lib.nsfem_set_point_locator(self._h, _dp(o), _dp(ih), _ip(nb), _ip(bp), _ip(bc)))

    def _points(self, X):
        X = np.ascontiguousarray(X, dtype=np.float64)
        if X.ndim != 2 or X.shape[1] != self.dim:
            raise ValueError("points: expected shape [m, %d], got %s" % (self.dim, X.shape))
        return X

    def locate_points(self, X):
        """int32 [m]: the lowest-id cell containing each point of X [m, dim] (-1: outside the mesh)"""
        X = self._points(X)
        cells = np.empty(X.shape[0], dtype=np.int32)
        self._check(self._lib.nsfem_locate_points(self._h, X.shape[0], _dp(X), _ip(cells)))
        return cells

    def eval_points(self, slot, X, cells=None):
        """values at X [m, dim] of the field in ``slot``: [m, dim] for a velocity slot, [m] for a pressure or scalar
        slot; ``cells``: their cells if already known (locate_points), NaN where a cell is -1"""
        X = self._points(X)
        m = X.shape[0]
        c = None
        if cells is not None:
            c = np.ascontiguousarray(cells, dtype=np.int32)
            if c.shape != (m, ):
                raise ValueError("cells: expected %d entries, got shape %s" % (m, c.shape))
        vector = self.state_size(slot) == self.n_velocity
        out = np.empty((m, self.dim) if vector else m, dtype=np.float64)
        self._check(self._lib.nsfem_eval_points(self._h, int(slot), m, _dp(X), None if c is None else _ip(c),
                                                _dp(out)))
        return out

    def tracers_set(self, X):
        """replace the context's particle cloud by the points X [n, dim] (located; outside the mesh: status 1)"""
        X = self._points(X)
        self._check(self._lib.nsfem_tracers_set(self._h, X.shape[0], _dp(X)))
        self._n_tracers = X.shape[0]

    def tracers_advect(self, slot_begin, slot_end, dt, n_sub=1):
        """RK4 over n_sub substeps of dt / n_sub in the velocity blended linearly from slot_begin to slot_end"""
        self._check(self._lib.nsfem_tracers_advect(self._h, int(slot_begin), int(slot_end), float(dt), int(n_sub)))

    def tracers_get(self):
        """(positions [n, dim], cells int32 [n], status uint8 [n]: 0 moving, 1 left)"""
        n = int(self.tracers_info()["n"])
        x = np.empty((n, self.dim), dtype=np.float64)
        cells = np.empty(n, dtype=np.int32)
        status = np.empty(n, dtype=np.uint8)
        self._check(self._lib.nsfem_tracers_get(self._h, _dp(x), _ip(cells), status.ctypes.data_as(C.POINTER(C.c_uint8))))
        return x, cells, status

    def tracers_info(self):
        """dict(n, n_left, advect_calls, fallbacks = bin searches of the last advect call)"""
        out = (C.c_int64 * 4)()
        self._check(self._lib.nsfem_tracers_info(self._h, out))
        return dict(n=int(out[0]), n_left=int(out[1]), advect_calls=int(out[2]), fallbacks=int(out[3]))

    # -- running flow statistics (csrc/statistics.hip) ----------------------------------
    def stats_enable(self, flags):
        """allocate and zero the accumulators for ``flags`` (STATS_VELOCITY [| STATS_PRESSURE] [| STATS_SCALAR]);
        calling again drops the samples and keeps the groups of ``stats_set_groups``, 0 frees everything"""
        self._check(self._lib.nsfem_stats_enable(self._h, int(flags)))
        if int(flags) == 0 or not hasattr(self, "_stats_groups"):
            self._stats_groups = {}      # field -> number of groups, as the library keeps them

    def stats_sample(self, velocity_slot=U0, pressure_slot=-1, scalar_slot=-1, weight=1.0):
        """one launch: add the fields of the slots (-1: none) with ``weight`` to the running means and moments"""
        self._check(self._lib.nsfem_stats_sample(self._h, int(velocity_slot), int(pressure_slot), int(scalar_slot),
                                                 float(weight)))

    def stats_columns(self, field=0):
        """columns of a profile row: P2 (field 0) dim + dim (dim + 1) / 2, + 2 + dim with the scalar; P1 (field 1) 2"""
        if field == 1:
            return 2
        dim = self.dim
        return dim + dim * (dim + 1) // 2 + (2 + dim if self.stats_info()["flags"] & STATS_SCALAR else 0)

    def stats_get(self, quantity):
        """one quantity at every node (covariances divided by the accumulated weight): MEAN_U, FLUX_UT [n_p2, dim];
        COV_U [n_p2, dim (dim + 1) / 2] (xx, xy, yy / xx, xy, xz, yy, yz, zz); TKE, MEAN_T, VAR_T [n_p2]; MEAN_P,
        VAR_P [n_p1]"""
        dim = self.dim
        shape = {STATS_MEAN_U: (self.n_p2, dim), STATS_COV_U: (self.n_p2, dim * (dim + 1) // 2),
                 STATS_TKE: (self.n_p2, ), STATS_MEAN_P: (self.n_p1, ), STATS_VAR_P: (self.n_p1, ),
                 STATS_MEAN_T: (self.n_p2, ), STATS_VAR_T: (self.n_p2, ), STATS_FLUX_UT: (self.n_p2, dim)}.get(
                     int(quantity))
        if shape is None:
            raise ValueError("unknown statistics quantity %r" % (quantity, ))
        out = np.empty(shape, dtype=np.float64)
        self._check(self._lib.nsfem_stats_get(self._h, int(quantity), _dp(out), out.size))
        return out

    def stats_set_groups(self, field, group_ptr, nodes, weights=None):
        """groups of nodes of ``field`` (0: P2, 1: P1) as a CSR; ``weights`` None: uniform"""
        gp = np.ascontiguousarray(group_ptr, dtype=np.int32)
        nd = np.ascontiguousarray(nodes, dtype=np.int32)
        w = np.ones(nd.size) if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
        if gp.ndim != 1 or gp.size < 2 or nd.shape != (int(gp[-1]), ) or w.shape != nd.shape:
            raise ValueError("group_ptr / nodes / weights do not match")
        self._check(self._lib.nsfem_stats_set_groups(self._h, int(field), gp.size - 1, _ip(gp), _ip(nd), _dp(w)))
        self._stats_groups[int(field)] = gp.size - 1

    def stats_profiles(self, field=0):
        """[n_groups, n_q]: pooled means and covariances (within-node plus between-node part) of every group, columns
        in the order of the accumulators (m_u, C_uu[, m_T, C_TT, C_uT] / m_p, C_pp)"""
        n_groups = getattr(self, "_stats_groups", {}).get(int(field), 0)
        ncol = self.stats_columns(field)
        out = np.empty((max(n_groups, 1), ncol), dtype=np.float64)      # (no groups yet: the library says so)
        self._check(self._lib.nsfem_stats_profiles(self._h, int(field), _dp(out), n_groups * ncol))
        return out

    def stats_info(self):
        """dict(samples, flags, bytes = size of the accumulators, launches = update launches)"""
        out = (C.c_int64 * 4)()
        self._check(self._lib.nsfem_stats_info(self._h, out))
        return dict(samples=int(out[0]), flags=int(out[1]), bytes=int(out[2]), launches=int(out[3]))

    def stats_weight(self):
        out = C.c_double()
        self._check(self._lib.nsfem_stats_weight(self._h, C.byref(out)))
        return out.value

    # -- gradient-derived fields (csrc/derived.hip) -------------------------------------
    def derived_components(self, quantity):
        """components of one DERIVED_* quantity on this mesh (vorticity 1 / 3, velocity gradient dim^2, ...)"""
        out = C.c_int()
        self._check(self._lib.nsfem_derived_components(self._h, int(quantity), C.byref(out)))
        return out.value

    def derived_fields(self, quantities, center, velocity_slot=U0, pressure_slot=P, scalar_slot=-1):
        """{quantity: array} of the DERIVED_* ``quantities`` (one id or several) of the state in the slots, from ONE
        element launch (DERIVED_NODE: plus one gather launch) and one copy: DERIVED_CELL [n_cells, ncomp] cell means,
        DERIVED_VERTEX [n_cells, dim + 1, ncomp] values at the vertices of every cell, DERIVED_NODE [n_p2, ncomp]
        volume-weighted recovery at the P2 nodes; quantities with one component come without the last axis"""
        ids = [int(quantities)] if np.isscalar(quantities) else [int(q) for q in quantities]
        mask = 0
        for q in ids:
            if not 0 <= q < 32:
                raise ValueError("unknown derived quantity %r" % (q, ))
            mask |= 1 << q
        ids = sorted(set(ids))
        center = int(center)
        lead = {DERIVED_CELL: (self.n_cells, ), DERIVED_VERTEX: (self.n_cells, self.dim + 1),
                DERIVED_NODE: (self.n_p2, )}.get(center, (0, ))
        # (an unknown quantity or centre, or an empty mask, is the library's to refuse: it says why)
        ncomp = [self.derived_components(q) if q < N_DERIVED else 0 for q in ids]
        n_out = int(np.prod(lead)) * sum(ncomp)
        flat = np.empty(max(n_out, 1), dtype=np.float64)
        self._check(self._lib.nsfem_derived_fields(self._h, int(velocity_slot), int(pressure_slot), int(scalar_slot),
                                                   mask, center, _dp(flat), n_out))
        out = flat[:n_out].reshape(lead + (sum(ncomp), ))
        res, col = {}, 0
        for q, n in zip(ids, ncomp):
            res[q] = out[..., col].copy() if n == 1 else out[..., col:col + n].copy()
            col += n
        return res

    def derived_info(self):
        """dict(cell_launches, gather_launches, calls, bytes = size of the private work buffer)"""
        out = (C.c_int64 * 4)()
        self._check(self._lib.nsfem_derived_info(self._h, out))
        return dict(cell_launches=int(out[0]), gather_launches=int(out[1]), calls=int(out[2]), bytes=int(out[3]))

    # -- energy spectra (csrc/spectrum.hip) ----------------------------------------------
    def spectrum_set(self, shape, matrices, node_of_point, bin_ptr, bin_points):
        """the transform-and-bin plan of this context (replaces an earlier one): ``shape`` = lattice points per axis, x
        first (2 or 3 entries); ``matrices`` = per axis a row-major [n_a, n_a] matrix (row = basis function) or None
        (axis not transformed); ``node_of_point`` [prod(shape)] with x fastest; the bins as a CSR of lattice points.
        ``shape = None`` frees the plan."""
        n = np.ones(3, dtype=np.int32)
        if shape is None:
            n[0] = 0
            self._check(self._lib.nsfem_spectrum_set(self._h, _ip(n), None, None, None, None, 0, None, None))
            self._spectrum_bins = 0
            return
        shape = [int(v) for v in shape]
        matrices = list(matrices)
        if not 1 <= len(shape) <= 3 or len(matrices) != len(shape):
            raise ValueError("shape / matrices do not match")
        n[:len(shape)] = shape
        F = []
        for a, m in enumerate(matrices):
            if m is None:
                F.append(None)
                continue
            m = np.ascontiguousarray(m, dtype=np.float64)
            if m.shape != (shape[a], shape[a]):
                raise ValueError("matrix of axis %d is not [%d, %d]" % (a, shape[a], shape[a]))
            F.append(m)
        F += [None] * (3 - len(F))
        nop = np.ascontiguousarray(node_of_point, dtype=np.int32).ravel()
        gp = np.ascontiguousarray(bin_ptr, dtype=np.int32)
        bp = np.ascontiguousarray(bin_points, dtype=np.int32).ravel()
        if min(shape) >= 1 and nop.size != int(np.prod(shape, dtype=np.int64)):
            raise ValueError("node_of_point does not match the lattice")
        if gp.ndim != 1 or gp.size < 2 or bp.size != int(gp[-1]):
            raise ValueError("bin_ptr / bin_points do not match")
        self._check(self._lib.nsfem_spectrum_set(self._h, _ip(n), *[None if m is None else _dp(m) for m in F],
                                                 _ip(nop), gp.size - 1, _ip(gp), _ip(bp)))
        self._spectrum_bins = gp.size - 1

    def spectrum_compute(self, slot=U0):
        """[n_bins, ncomp]: the raw sums of squares of the transformed values per bin and component of the nodal field
        in ``slot`` (velocity slots: ncomp = dim; scalar and pressure slots: 1)"""
        slot = int(slot)
        ncomp = self.dim if slot in (U0, U1, U2, USTAR, BODY_FORCE) else 1
        n_bins = getattr(self, "_spectrum_bins", 0)
        out = np.empty((max(n_bins, 1), ncomp), dtype=np.float64)      # (no plan yet: the library says so)
        self._check(self._lib.nsfem_spectrum_compute(self._h, slot, _dp(out), n_bins * ncomp))
        return out[:n_bins]

    def spectrum_info(self):
        """dict(transform_launches, bin_launches, calls, bytes = size of the plan)"""
        out = (C.c_int64 * 4)()
        self._check(self._lib.nsfem_spectrum_info(self._h, out))
        return dict(transform_launches=int(out[0]), bin_launches=int(out[1]), calls=int(out[2]), bytes=int(out[3]))

    # -- wall quantities (csrc/wall.hip) ------------------------------------------------
    def wall_components(self):
        """NW: doubles per facet / group row of wall_compute (9 in 2D, 13 in 3D)"""
        out = C.c_int()
        self._check(self._lib.nsfem_wall_components(self._h, C.byref(out)))
        return out.value

    def wall_set_facets(self, facet_cell, facet_local, facet_group=None, n_groups=1):
        """make a facet set resident (validated, sorted by group, uploaded once; replaces an earlier set): facet f =
        the facet of cell ``facet_cell[f]`` opposite its local vertex ``facet_local[f]``, in group ``facet_group[f]``
        (None: all in group 0)"""
        fc = np.ascontiguousarray(facet_cell, dtype=np.int32).ravel()
        fl = np.ascontiguousarray(facet_local, dtype=np.int32).ravel()
        if fl.size != fc.size:
            raise ValueError("facet_cell and facet_local differ in length")
        fg = None
        if facet_group is not None:
            fg = np.ascontiguousarray(facet_group, dtype=np.int32).ravel()
            if fg.size != fc.size:
                raise ValueError("facet_cell and facet_group differ in length")
        # whoever calls this owns the context's one facet set from here on: a wall_quantities.WallQuantities that made
        # its set resident earlier sees that it has to do so again
        self._active_wall_set = None
        self._check(self._lib.nsfem_wall_set_facets(self._h, fc.size, _ip(fc), _ip(fl),
                                                    _ip(fg) if fg is not None else None, int(n_groups)))
        # sizes of the resident set and its output buffers, kept for wall_compute: no ABI round trip and no
        # allocation per call there
        nw = self.wall_components()
        self._wall = dict(facets=int(fc.size), groups=int(n_groups), nw=nw, opts=WallOpts(),
                          group_rows=np.zeros((int(n_groups), nw)), facet_rows=np.zeros((int(fc.size), nw)))

    def wall_compute(self, nu, symmetric=1.0, kappa=0.0, origin=None, use_law=False, velocity_slot=U0,
                     pressure_slot=P, scalar_slot=-1, facets=False):
        """group rows [n_groups, NW] of the resident facet set -- with ``facets`` the pair (group rows, facet rows
        [n_facets, NW] in the input order of wall_set_facets).  Row: |f|, int -p n [dim], int viscous traction [dim],
        int u.n, int T, int -kappa grad T.n, int (x - origin) x traction [1 / 3] (include/nsfem.h)"""
        w = getattr(self, "_wall", None)
        if w is None:       # no resident set: the library refuses the call and says why
            w = dict(facets=0, groups=0, nw=1, opts=WallOpts(), group_rows=np.zeros((1, 1)), facet_rows=np.zeros((0, 1)))
        opts = w["opts"]
        opts.nu, opts.sym, opts.kappa = float(nu), float(symmetric), float(kappa)
        opts.origin[0] = opts.origin[1] = opts.origin[2] = 0.0
        if origin is not None:
            for d, v in enumerate(origin):
                opts.origin[d] = float(v)
        opts.use_law = 1 if use_law else 0
        groups, rows = w["group_rows"], w["facet_rows"]
        self._check(self._lib.nsfem_wall_compute(self._h, int(velocity_slot), int(pressure_slot), int(scalar_slot),
                                                 C.byref(opts), _dp(groups), _dp(rows) if facets and rows.size else None))
        # (copies: the buffers are reused by the next call)
        return (groups.copy(), rows.copy()) if facets else groups.copy()

    def wall_info(self):
        """dict(facets, groups, computes, uploads = facet sets made resident so far)"""
        out = (C.c_int64 * 4)()
        self._check(self._lib.nsfem_wall_info(self._h, out))
        return dict(facets=int(out[0]), groups=int(out[1]), computes=int(out[2]), uploads=int(out[3]))

    def cfl_number(self, slot, step_size):
        out = C.c_double()
        self._check(self._lib.nsfem_cfl_number(self._h, int(slot), float(step_size), C.byref(out)))
        return out.value

    def profile_smoother(self, enable):
        """start (True) / stop (False -> (avg ms per launch, launches, algorithmic bytes per launch))
        the in-situ timing of the finest-level smoothing launches of the velocity multigrid"""
        ms, n, nbytes = C.c_double(), C.c_int64(), C.c_int64()
        self._check(self._lib.nsfem_profile_smoother(self._h, 1 if enable else 0, C.byref(ms),
                                                     C.byref(n), C.byref(nbytes)))
        return None if enable else (ms.value, n.value, nbytes.value)

    def profile_smoother_detail(self):
        """the window profile_smoother(False) just closed: dict(launches, steps, bytes, lattice)"""
        out = (C.c_int64 * 4)()
        self._check(self._lib.nsfem_profile_smoother_detail(self._h, out))
        return dict(launches=int(out[0]), steps=int(out[1]), bytes=int(out[2]), lattice=bool(out[3]))

    def jacobian_info(self):
        """the matrix-free velocity Jacobian action: dict(path = "three-launch" | "fused-gather" | "lattice-kernel",
        lattice_launches, lattice_bytes)"""
        out = (C.c_int64 * 4)()
        self._check(self._lib.nsfem_jacobian_info(self._h, out))
        return dict(path=("three-launch", "fused-gather", "lattice-kernel")[int(out[0])],
                    lattice_launches=int(out[1]), lattice_bytes=int(out[2]), lattice_variant=int(out[3]))

    def step_frame_info(self):
        """launches so far of the fused step frame (NSFEM_STEP_FUSED): dict(pair_begin, pair_correction,
        correction_finish, projection_sum)"""
        out = (C.c_int64 * 4)()
        self._check(self._lib.nsfem_step_frame_info(self._h, out))
        return dict(pair_begin=int(out[0]), pair_correction=int(out[1]), correction_finish=int(out[2]),
                    projection_sum=int(out[3]))

    def newton_frame_info(self):
        """residual launches so far with the frame of the Newton iteration (NSFEM_NEWTON_FUSED): dict(residuals,
        updates)"""
        out = (C.c_int64 * 2)()
        self._check(self._lib.nsfem_newton_frame_info(self._h, out))
        return dict(residuals=int(out[0]), updates=int(out[1]))

    def jacobian_table_check(self):
        """cells whose per-cell basis gradients / weights differ from k_jac_lattice's tables in any bit (-1: no tables)"""
        out = C.c_int64(0)
        self._check(self._lib.nsfem_jacobian_table_check(self._h, C.byref(out)))
        return int(out.value)

    def profile_convection(self, enable):
        """start (True) / stop (False -> (avg ms per application, applications, algorithmic bytes))
        the in-situ timing of the matrix-free convection action (element kernel + node gather)"""
        ms, n, nbytes = C.c_double(), C.c_int64(), C.c_int64()
        self._check(self._lib.nsfem_profile_convection(self._h, 1 if enable else 0, C.byref(ms),
                                                       C.byref(n), C.byref(nbytes)))
        return None if enable else (ms.value, n.value, nbytes.value)

    def time_spmv(self, op, reps=50):
        ms = C.c_double()
        nbytes = C.c_int64()
        self._check(self._lib.nsfem_time_spmv(self._h, op, reps, C.byref(ms), C.byref(nbytes)))
        return ms.value, nbytes.value
