"""ctypes binding of libcfdh.so (include/cfdh.h).  No CPU fallback: a missing
library or a missing GPU is an error, never a silent detour."""
from __future__ import annotations

import ctypes as C
import os
import subprocess

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
_SO = os.path.join(_HERE, "libcfdh.so")
_LIB = None

dp = C.POINTER(C.c_double)
ip = C.POINTER(C.c_int32)
lp = C.POINTER(C.c_int64)


class Options(C.Structure):
    _fields_ = [
        ("snes_rtol", C.c_double), ("snes_atol", C.c_double), ("snes_stol", C.c_double), ("snes_max_it", C.c_int32),
        ("ksp_rtol", C.c_double), ("ksp_atol", C.c_double), ("ksp_max_it", C.c_int32), ("ksp_restart", C.c_int32),
        ("cheb_degree", C.c_int32), ("cheb_ratio", C.c_double), ("schur_full", C.c_int32),
        ("amg_smooth_degree", C.c_int32), ("amg_smooth_ratio", C.c_double), ("amg_theta", C.c_double),
        ("amg_max_coarse", C.c_int32), ("pc_refresh", C.c_int32), ("remove_p_mean", C.c_int32), ("verbose", C.c_int32),
        ("pc_type", C.c_int32), ("cc_smooth_degree", C.c_int32), ("ksp_guess", C.c_int32),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("newton_its", C.c_int32), ("krylov_its", C.c_int32), ("reason", C.c_int32), ("pc_refreshes", C.c_int32),
        ("fnorm0", C.c_double), ("fnorm", C.c_double), ("ms_assemble", C.c_double), ("ms_solve", C.c_double),
        ("ms_pc_setup", C.c_double), ("ms_total", C.c_double),
    ]


class IpcsStats(C.Structure):
    _fields_ = [
        ("its", C.c_int32 * 3), ("reason", C.c_int32 * 3), ("rel_res", C.c_double * 3), ("ms_assemble", C.c_double),
        ("ms_solve", C.c_double * 3), ("ms_total", C.c_double), ("launches", C.c_int32), ("host_syncs", C.c_int32),
    ]


class ScalarStats(C.Structure):
    _fields_ = [("its", C.c_int32), ("reason", C.c_int32), ("rel_res", C.c_double), ("ms_assemble", C.c_double), ("ms_total", C.c_double)]


class ParticleStats(C.Structure):
    _fields_ = [("active", C.c_int64), ("exited", C.c_int64), ("lost", C.c_int64), ("stepped", C.c_int64), ("ms_kernel", C.c_double),
                ("ms_total", C.c_double)]


class FgmresTrace(C.Structure):
    _fields_ = [
        ("m", C.c_int32), ("max_res", C.c_int32), ("max_cycles", C.c_int32),
        ("cycles", C.c_int32), ("k", C.c_int32), ("guess_used", C.c_int32), ("fp32_used", C.c_int32), ("n_res", C.c_int32), ("pad_", C.c_int32),
        ("bn", C.c_double), ("tol", C.c_double), ("beta", C.c_double),
        ("V", dp), ("Z", dp), ("H", dp), ("ww", dp), ("nrm2", dp), ("y", dp), ("x0", dp), ("x_start", dp), ("res", dp),
        ("cycle_beta", dp), ("cycle_est", dp), ("second_pass", ip),
    ]


ALLREDUCE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, dp, C.c_int, C.c_int)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, dp, dp)

# every symbol include/cfdh.h declares (checked by tests/test_abi.py)
SYMBOLS = [
    "cfdh_create", "cfdh_create_elem", "cfdh_create_elem_part", "cfdh_set_facet_markers", "cfdh_destroy", "cfdh_last_error", "cfdh_abi_version", "cfdh_set_params", "cfdh_default_options",
    "cfdh_set_options", "cfdh_clear_dirichlet", "cfdh_add_dirichlet", "cfdh_update_dirichlet", "cfdh_set_state", "cfdh_get_solution",
    "cfdh_get_previous", "cfdh_get_residual", "cfdh_advance", "cfdh_advance_field", "cfdh_set_time_scheme", "cfdh_set_previous2", "cfdh_get_previous2",
    "cfdh_shift_history", "cfdh_set_boundary_terms", "cfdh_set_formulation", "cfdh_set_pressure_boundaries", "cfdh_set_pressure_boundaries_ex", "cfdh_set_traction_boundaries", "cfdh_assemble", "cfdh_get_csr", "cfdh_spmv", "cfdh_solve_step",
    "cfdh_functional", "cfdh_wall_shear_stress", "cfdh_set_global_pressure_space", "cfdh_set_halo", "cfdh_comm_unique_id", "cfdh_comm_init", "cfdh_comm_set_callbacks",
    "cfdh_profile_enable", "cfdh_profile_get", "cfdh_profile_reset", "cfdh_info",
    "cfdh_set_schur_pcd", "cfdh_set_ksp_forcing", "cfdh_get_newton_history", "cfdh_get_pcd_operator", "cfdh_apply_preconditioner", "cfdh_apply_operator",
    "cfdh_get_amg_operator", "cfdh_get_amg_vectors", "cfdh_get_amg_head", "cfdh_krylov_vec_op", "cfdh_fgmres_solve",
    "cfdh_create_ipcs", "cfdh_ipcs_set_form", "cfdh_ipcs_set_tolerances", "cfdh_ipcs_step", "cfdh_ipcs_get_operator", "cfdh_ipcs_get_intermediate",
    "cfdh_ipcs_apply_pressure_pc", "cfdh_ipcs_krylov_solve", "cfdh_ipcs_set_scheme", "cfdh_ipcs_get_block_operator",
    "cfdh_wall_stats_reset", "cfdh_wall_stats_accumulate", "cfdh_wall_stats_get",
    "cfdh_scalar_enable", "cfdh_scalar_set_dirichlet", "cfdh_scalar_set_state", "cfdh_scalar_get_state", "cfdh_scalar_set_tolerances",
    "cfdh_scalar_step", "cfdh_scalar_get_operator", "cfdh_scalar_functional", "cfdh_scalar_krylov_solve", "cfdh_scalar_get_order",
    "cfdh_particles_enable", "cfdh_particles_seed", "cfdh_particles_clear", "cfdh_particles_step", "cfdh_particles_get",
    "cfdh_flow_field", "cfdh_flow_integrals", "cfdh_flow_stats_reset", "cfdh_flow_stats_accumulate", "cfdh_flow_stats_get",
    "cfdh_sample_set_points", "cfdh_sample_set_grid", "cfdh_sample_get_location", "cfdh_sample_now", "cfdh_sample_series_enable",
    "cfdh_sample_record", "cfdh_sample_series_get", "cfdh_sample_mean_reset", "cfdh_sample_mean_accumulate", "cfdh_sample_mean_get",
    "cfdh_section_set", "cfdh_section_get_cut", "cfdh_section_now", "cfdh_section_series_enable", "cfdh_section_record",
    "cfdh_section_series_get", "cfdh_section_mean_reset", "cfdh_section_mean_accumulate", "cfdh_section_mean_get",
]


def build(force=False):
    """Compile libcfdh.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    src = os.path.join(_HERE, "csrc")
    newest = max(os.path.getmtime(os.path.join(src, f)) for f in os.listdir(src)
                 if f.endswith((".hip", ".cpp", ".hpp", ".h")))
    hdr = os.path.join(os.path.dirname(_HERE), "include", "cfdh.h")
    if os.path.exists(hdr):
        newest = max(newest, os.path.getmtime(hdr))
    if force or not os.path.exists(_SO) or os.path.getmtime(_SO) < newest:
        if not os.path.exists("/opt/rocm/bin/hipcc") and os.path.exists(_SO):
            return _SO
        subprocess.check_call(["make", "-C", src, "-s", "-j4"])
    return _SO


def lib():
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(_SO):
        raise RuntimeError(
            "libcfdh.so is missing (%s): build it with `python -c 'import __graft_entry__ as g; g.build()'`; "
            "this package has no CPU fallback" % _SO)
    L = C.CDLL(_SO)
    vp = C.c_void_p
    L.cfdh_create.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, ip, dp, C.c_int64, ip, ip, ip]
    L.cfdh_create_elem.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, ip, dp, C.c_int64, ip, ip, ip]
    L.cfdh_create_elem_part.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, ip, dp, C.c_int64, ip, ip, ip]
    L.cfdh_set_facet_markers.argtypes = [vp, C.c_int64, ip]
    L.cfdh_destroy.argtypes = [vp]
    L.cfdh_destroy.restype = None
    L.cfdh_last_error.argtypes = [vp]
    L.cfdh_last_error.restype = C.c_char_p
    L.cfdh_set_params.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.c_double, dp]
    L.cfdh_default_options.argtypes = [C.POINTER(Options)]
    L.cfdh_set_options.argtypes = [vp, C.POINTER(Options)]
    L.cfdh_clear_dirichlet.argtypes = [vp]
    L.cfdh_add_dirichlet.argtypes = [vp, C.c_int, C.c_int64, ip, dp]
    L.cfdh_update_dirichlet.argtypes = [vp, C.c_int, C.c_int64, ip, dp]
    L.cfdh_set_state.argtypes = [vp, dp, dp, dp, dp]
    L.cfdh_get_solution.argtypes = [vp, dp, dp]
    L.cfdh_set_time_scheme.argtypes = [vp, C.c_double, C.c_double, C.c_double, C.c_double]
    L.cfdh_set_previous2.argtypes = [vp, dp]
    L.cfdh_get_previous2.argtypes = [vp, dp]
    L.cfdh_shift_history.argtypes = [vp]
    L.cfdh_wall_shear_stress.argtypes = [vp, dp]
    L.cfdh_set_boundary_terms.argtypes = [vp, C.c_int, C.c_int, C.c_double]
    L.cfdh_set_formulation.argtypes = [vp, C.c_int]
    L.cfdh_set_pressure_boundaries.argtypes = [vp, C.c_int, ip, dp, C.c_double]
    L.cfdh_set_pressure_boundaries_ex.argtypes = [vp, C.c_int, ip, dp, C.c_double, C.POINTER(C.c_uint8), dp]
    L.cfdh_set_traction_boundaries.argtypes = [vp, C.c_int, ip, dp, C.c_double, C.POINTER(C.c_uint8), dp]
    L.cfdh_get_residual.argtypes = [vp, dp, dp]
    L.cfdh_get_previous.argtypes = [vp, dp, dp]
    L.cfdh_advance.argtypes = [vp]
    L.cfdh_advance_field.argtypes = [vp, C.c_int]
    L.cfdh_assemble.argtypes = [vp, C.c_int]
    L.cfdh_get_csr.argtypes = [vp, lp, ip, ip, dp]
    L.cfdh_spmv.argtypes = [vp, dp, dp]
    L.cfdh_solve_step.argtypes = [vp, C.POINTER(Stats)]
    L.cfdh_functional.argtypes = [vp, C.c_int, C.c_int, dp]
    L.cfdh_set_halo.argtypes = [vp, C.c_int, ip, lp, ip, lp, ip]
    L.cfdh_set_global_pressure_space.argtypes = [vp, C.c_int64, C.c_int64, ip, dp, ip, C.c_int64, ip]
    L.cfdh_comm_unique_id.argtypes = [C.c_void_p]
    L.cfdh_comm_init.argtypes = [vp, C.c_void_p, C.c_int, C.c_int]
    L.cfdh_comm_set_callbacks.argtypes = [vp, ALLREDUCE_FN, EXCHANGE_FN, C.c_void_p, C.c_int, C.c_int]
    L.cfdh_profile_enable.argtypes = [vp, C.c_int]
    L.cfdh_profile_get.argtypes = [vp, C.c_int, dp, lp]
    L.cfdh_profile_reset.argtypes = [vp]
    L.cfdh_info.argtypes = [vp, C.c_int]
    L.cfdh_info.restype = C.c_int64
    L.cfdh_set_schur_pcd.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    L.cfdh_set_ksp_forcing.argtypes = [vp, C.c_int, C.c_double, C.c_double, C.c_double, C.c_double, C.c_double]
    L.cfdh_get_newton_history.argtypes = [vp, ip, dp, dp, ip, dp]
    L.cfdh_get_pcd_operator.argtypes = [vp, lp, ip, ip, dp, dp]
    L.cfdh_apply_preconditioner.argtypes = [vp, dp, dp]
    L.cfdh_apply_operator.argtypes = [vp, dp, dp, dp]
    L.cfdh_get_amg_operator.argtypes = [vp, C.c_int, C.c_int, C.c_int, lp, lp, lp, ip, ip, dp]
    L.cfdh_get_amg_vectors.argtypes = [vp, C.c_int, C.c_int, C.c_int, lp, dp]
    L.cfdh_get_amg_head.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32)]
    L.cfdh_krylov_vec_op.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.c_int, dp, dp, dp, dp, dp, C.c_double, C.c_int, dp, dp,
                                     C.POINTER(C.c_float), ip, dp, dp, dp]
    L.cfdh_fgmres_solve.argtypes = [vp, dp, C.c_int, dp, ip, ip, C.POINTER(FgmresTrace)]
    L.cfdh_create_ipcs.argtypes = [C.POINTER(vp), C.c_int, C.c_int, C.c_int64, C.c_int64, C.c_int64, ip, dp, C.c_int64, ip, ip, ip]
    L.cfdh_ipcs_set_form.argtypes = [vp, C.c_double, C.c_double]
    L.cfdh_ipcs_set_tolerances.argtypes = [vp, dp, C.c_double, ip]
    L.cfdh_ipcs_step.argtypes = [vp, C.POINTER(IpcsStats)]
    L.cfdh_ipcs_get_operator.argtypes = [vp, C.c_int, lp, ip, ip, dp]
    L.cfdh_ipcs_get_intermediate.argtypes = [vp, C.c_int, dp]
    L.cfdh_ipcs_set_scheme.argtypes = [vp, C.c_int]
    L.cfdh_ipcs_get_block_operator.argtypes = [vp, C.c_int, lp, ip, ip, dp]
    L.cfdh_ipcs_apply_pressure_pc.argtypes = [vp, dp, dp]
    L.cfdh_ipcs_krylov_solve.argtypes = [vp, C.c_int, dp, dp, C.c_double, C.c_double, C.c_int, dp, C.POINTER(IpcsStats), dp]
    L.cfdh_wall_stats_reset.argtypes = [vp]
    L.cfdh_wall_stats_accumulate.argtypes = [vp, C.c_double]
    L.cfdh_wall_stats_get.argtypes = [vp, C.c_int, lp, dp]
    L.cfdh_scalar_enable.argtypes = [vp, C.c_double, C.c_double, C.c_double]
    L.cfdh_scalar_set_dirichlet.argtypes = [vp, C.c_int64, ip, dp]
    L.cfdh_scalar_set_state.argtypes = [vp, dp]
    L.cfdh_scalar_get_state.argtypes = [vp, dp]
    L.cfdh_scalar_set_tolerances.argtypes = [vp, C.c_double, C.c_double, C.c_int32]
    L.cfdh_scalar_step.argtypes = [vp, C.POINTER(ScalarStats)]
    L.cfdh_scalar_get_operator.argtypes = [vp, lp, ip, ip, dp, dp]
    L.cfdh_scalar_functional.argtypes = [vp, C.c_int, C.c_int, dp]
    L.cfdh_scalar_krylov_solve.argtypes = [vp, dp, dp, C.c_double, C.c_double, C.c_int, dp, C.POINTER(ScalarStats), dp, dp]
    L.cfdh_scalar_get_order.argtypes = [vp, ip]
    L.cfdh_particles_enable.argtypes = [vp, C.c_int64, C.c_int32]
    L.cfdh_particles_seed.argtypes = [vp, C.c_int64, dp, ip, C.c_double]
    L.cfdh_particles_clear.argtypes = [vp]
    L.cfdh_particles_step.argtypes = [vp, C.c_double, C.POINTER(ParticleStats)]
    L.cfdh_particles_get.argtypes = [vp, C.c_int, lp, C.c_void_p]
    L.cfdh_flow_field.argtypes = [vp, C.c_int, lp, dp]
    L.cfdh_flow_integrals.argtypes = [vp, dp]
    L.cfdh_flow_stats_reset.argtypes = [vp]
    L.cfdh_flow_stats_accumulate.argtypes = [vp, C.c_double]
    L.cfdh_flow_stats_get.argtypes = [vp, C.c_int, lp, dp]
    L.cfdh_sample_set_points.argtypes = [vp, C.c_int64, dp, C.c_double]
    L.cfdh_sample_set_grid.argtypes = [vp, dp, dp, lp, C.c_double]
    L.cfdh_sample_get_location.argtypes = [vp, lp, ip, dp, dp]
    L.cfdh_sample_now.argtypes = [vp, lp, dp]
    L.cfdh_sample_series_enable.argtypes = [vp, C.c_int64]
    L.cfdh_sample_record.argtypes = [vp, C.c_double]
    L.cfdh_sample_series_get.argtypes = [vp, lp, dp, dp]
    L.cfdh_sample_mean_reset.argtypes = [vp]
    L.cfdh_sample_mean_accumulate.argtypes = [vp, C.c_double]
    L.cfdh_sample_mean_get.argtypes = [vp, C.c_int, lp, dp]
    i32p = C.POINTER(C.c_int32)
    L.cfdh_section_set.argtypes = [vp, C.c_int32, dp, dp, dp]
    L.cfdh_section_get_cut.argtypes = [vp, i32p, lp, ip, dp, ip]
    L.cfdh_section_now.argtypes = [vp, i32p, dp]
    L.cfdh_section_series_enable.argtypes = [vp, C.c_int64]
    L.cfdh_section_record.argtypes = [vp, C.c_double]
    L.cfdh_section_series_get.argtypes = [vp, lp, dp, dp]
    L.cfdh_section_mean_reset.argtypes = [vp]
    L.cfdh_section_mean_accumulate.argtypes = [vp, C.c_double]
    L.cfdh_section_mean_get.argtypes = [vp, i32p, dp, dp]
    _LIB = L
    return L


def _dp(a):
    return None if a is None else a.ctypes.data_as(dp)


def _ip(a):
    return None if a is None else a.ctypes.data_as(ip)


def _lp(a):
    return None if a is None else a.ctypes.data_as(lp)


class CfdhError(RuntimeError):
    pass


def _raise(code, msg):
    # error mapping of the reference: ValueError bad config, RuntimeError init/convergence
    # (/root/reference/main.py:56-82, stabilized_schur.py:332-334)
    if code == -1:
        raise ValueError(msg)
    raise CfdhError(msg)


FORM_CONVECTIVE, FORM_ROTATIONAL = 0, 1  # cfdh_set_formulation
PC_SELFP, PC_CAHOUET_CHABARD, PC_PCD = 0, 1, 2  # cfdh_options.pc_type
AMG_HIER_A, AMG_HIER_P, AMG_HIER_H = 0, 1, 2  # cfdh_get_amg_operator / cfdh_get_amg_vectors
AMG_HIER_PG, AMG_HIER_DL0 = 3, 4  # partitioned run: the replicated pressure hierarchy, this rank's share of its finest level
AMG_OP_A, AMG_OP_P, AMG_OP_G, AMG_OP_SB, AMG_OP_SC, AMG_OP_PT = 0, 1, 2, 3, 4, 5
(AMG_VEC_DINV, AMG_VEC_WDINV, AMG_VEC_AGG, AMG_VEC_COARSE_INV, AMG_VEC_D, AMG_VEC_LAMBDA, AMG_VEC_CC_SCALARS, AMG_VEC_CC_ML,
 AMG_VEC_CC_PBC, AMG_VEC_SPGEMM_ROWS, AMG_VEC_SHAPE, AMG_VEC_ORDER, AMG_VEC_A00_LMAX, AMG_VEC_A00_DINV, AMG_VEC_DL0_SHAPE) = range(15)
# cfdh_ipcs_set_scheme
IPCS_BDF2, IPCS_MIDPOINT = 0, 1
# cfdh_ipcs_krylov_solve: words of the scalar block
IP_RHO, IP_RHO_OLD, IP_ALPHA, IP_OMEGA, IP_BETA, IP_RZ, IP_TOL2, IP_BN2, IP_RN2, IP_DONE, IP_ITS, IP_BAD = range(12)
IP_NSCAL = 16

# cfdh_krylov_vec_op
(KVOP_DOT, KVOP_NORM2, KVOP_NORM2_PAIR, KVOP_NORM2_TRIPLE, KVOP_NORMINF_DIFF, KVOP_SUB_MEAN, KVOP_NORM_SCALE_INV, KVOP_MULTIDOT,
 KVOP_MULTIDOT32, KVOP_GRAM, KVOP_MULTIAXPY, KVOP_LINCOMB, KVOP_LINCOMB_KEEP, KVOP_GS_UPDATE_NORMALIZE, KVOP_GS_UPDATE32, KVOP_STORE32,
 KVOP_GUESS, KVOP_AXPY, KVOP_WAXPY, KVOP_SCALE, KVOP_SCALE_TO, KVOP_PMULT) = range(22)
KVOP_FLAG_OPTION, KVOP_FLAG_RING = 1, 2  # the op's own switch (with y / with w.w / scale r) ; mirror into a slot of the read-back ring
# Eisenstat-Walker version 2 with PETSc's defaults: rtol_0, rtol_max, gamma, alpha, threshold (cfdh_set_ksp_forcing)
EW_DEFAULTS = (0.3, 0.9, 1.0, (1.0 + 5.0 ** 0.5) / 2.0, 0.1)
# cfdh_wall_stats_get
WALL_TAWSS, WALL_OSI, WALL_RRT, WALL_MEAN, WALL_PEAK, WALL_TOTALS = range(6)
INFO_WALL_STATS_COUNT = 90  # cfdh_info: accumulations since the last cfdh_wall_stats_reset
# cfdh_scalar_functional; cfdh_info: scalar enabled, scalar steps taken, launches of the scalar assembly kernel
SCALAR_INTEGRAL, SCALAR_FLUX, SCALAR_MIN, SCALAR_MAX = range(4)
INFO_SCALAR_ENABLED, INFO_SCALAR_STEPS, INFO_SCALAR_ASSEMBLIES = 95, 96, 97
# cfdh_scalar_krylov_solve: words of the scalar block
SC_RHO, SC_RHO_OLD, SC_ALPHA, SC_OMEGA, SC_BETA, SC_TOL2, SC_BN2, SC_RN2, SC_DONE, SC_ITS, SC_BAD = range(11)
SC_NSCAL = 16
# cfdh_particles_get; particle status; cfdh_info: particles enabled, particle steps taken, launches of the advection kernel
PARTICLE_X, PARTICLE_CELL, PARTICLE_STATUS, PARTICLE_AGE, PARTICLE_PATH, PARTICLE_EXPOSURE, PARTICLE_T_END = range(7)
PARTICLE_ACTIVE, PARTICLE_LOST = 0, -1  # an exit through a facet of marker m is 1 + m
INFO_PARTICLES_ENABLED, INFO_PARTICLE_STEPS, INFO_PARTICLE_LAUNCHES = 103, 104, 105
# cfdh_flow_field; the names Scenario.solve and the command line use; cfdh_flow_integrals; cfdh_flow_stats_get; cfdh_info: a
# flow-diagnostics buffer exists, launches of the cell-gradient pass, accumulations since the last reset, kernel times
FLOW_GRADIENT, FLOW_VORTICITY, FLOW_Q, FLOW_SHEAR_RATE, FLOW_DISSIPATION, FLOW_HELICITY, FLOW_LNH = range(7)
FLOW_FIELDS = {"gradient": FLOW_GRADIENT, "vorticity": FLOW_VORTICITY, "q_criterion": FLOW_Q, "shear_rate": FLOW_SHEAR_RATE,
               "dissipation": FLOW_DISSIPATION, "helicity": FLOW_HELICITY, "lnh": FLOW_LNH}
FLOW_INT_VOLUME, FLOW_INT_KINETIC, FLOW_INT_ENSTROPHY, FLOW_INT_DISSIPATION, FLOW_INT_HELICITY, FLOW_INT_DIV, FLOW_INT_Q, FLOW_INT_DIV2 = range(8)
FLOW_MEAN_U, FLOW_FLUCTUATION, FLOW_MEAN_DISSIPATION, FLOW_MEAN_SHEAR_RATE, FLOW_PEAK_SHEAR_RATE, FLOW_TOTALS = range(6)
INFO_FLOW_BUFFERS, INFO_FLOW_CELL_PASSES, INFO_FLOW_STATS_COUNT = 106, 107, 108
INFO_FLOW_CELL_PASS_NS, INFO_FLOW_KERNEL_NS = 109, 110  # device time of the last cell pass / of the last vertex, accumulation or integral kernel
# cfdh_sample_mean_get; cfdh_info: points in the sample set, points located, launches of the sample kernel, row blocks waiting in the
# series, device time of the last locate / sample kernel, the bin grid (doublings of its edge, total and longest list)
SAMPLE_MEAN_U, SAMPLE_MEAN_P, SAMPLE_FLUCTUATION, SAMPLE_TOTALS = range(4)
SAMPLE_TOL = 1e-9  # the default containment tolerance on the barycentric coordinates
INFO_SAMPLE_POINTS, INFO_SAMPLE_LOCATED, INFO_SAMPLE_LAUNCHES, INFO_SAMPLE_SERIES_ROWS = 111, 112, 113, 114
INFO_SAMPLE_LOCATE_NS, INFO_SAMPLE_KERNEL_NS = 115, 116
INFO_SAMPLE_BIN_DOUBLINGS, INFO_SAMPLE_BIN_TOTAL, INFO_SAMPLE_BIN_LONGEST = 117, 118, 119
# cut-plane sections (cfdh_section_*): the slots of a row; cfdh_info: sections, entries of the cut lists in all, the longest list,
# evaluations launched, row blocks waiting in the series, device time of the last evaluation
SECTION_NQ = 10
(SECTION_AREA, SECTION_FLOW, SECTION_P, SECTION_UN2, SECTION_U2, SECTION_P_UN, SECTION_KINETIC_FLUX, SECTION_UX, SECTION_UY,
 SECTION_UZ) = range(10)
SECTION_MAX = 256
INFO_SECTION_COUNT, INFO_SECTION_ENTRIES, INFO_SECTION_LONGEST, INFO_SECTION_LAUNCHES, INFO_SECTION_SERIES_ROWS = 120, 121, 122, 123, 124
INFO_SECTION_KERNEL_NS = 125


class Context:
    """Thin owner of a cfdh_ctx: arrays in, arrays out, exceptions for error codes."""

    def __init__(self, x, cells, facet_cells, facet_local, facet_marker, nv_owned=None, device=0, etype=0):
        """etype 0: P1 triangles / tetrahedra (cfdh_create); 1 P2 triangles, 2 Q1 quadrilaterals, 3 P1 triangles through the
        generic kernels (cfdh_create_elem: `x` are node coordinates, `cells` list nloc nodes)."""
        L = lib()
        self.L = L
        x = np.asarray(x, dtype=np.float64)
        cells = np.asarray(cells)
        self.etype = int(etype)
        # generic elements: the geometric dimension follows from the coordinates (P2: 6 nodes -> triangles, 10 -> tetrahedra;
        # Q1: 4 -> quadrilaterals, 8 -> hexahedra; P1 through the generic kernels: 3 / 4)
        self.dim = (3 if x.shape[1] >= 3 and cells.shape[1] in (8, 10) or (self.etype == 3 and cells.shape[1] == 4) else 2) if self.etype \
            else cells.shape[1] - 1  # triangles -> 2, tetrahedra -> 3
        if self.dim not in (2, 3) or x.shape[1] < self.dim:
            raise ValueError("cells must be triangles [nc,3] or tetrahedra [nc,4] with matching coordinates")
        nodes = {(1, 2): 6, (2, 2): 4, (3, 2): 3, (1, 3): 10, (2, 3): 8, (3, 3): 4}
        if self.etype and cells.shape[1] != nodes[(self.etype, self.dim)]:
            raise ValueError("element type %d needs %d nodes per cell for gdim %d" % (self.etype, nodes[(self.etype, self.dim)], self.dim))
        self.x = np.ascontiguousarray(x[:, : self.dim]).copy()
        self.cells = np.ascontiguousarray(cells, dtype=np.int32)
        self.nv = len(self.x)
        self.nvo = self.nv if nv_owned is None else int(nv_owned)
        fc = np.ascontiguousarray(facet_cells, dtype=np.int32)
        fl = np.ascontiguousarray(facet_local, dtype=np.int32)
        fm = np.ascontiguousarray(facet_marker, dtype=np.int32)
        h = C.c_void_p()
        if self.etype:
            if self.nvo != self.nv:   # one part of a partitioned run (owned nodes first, ghosts after)
                rc = L.cfdh_create_elem_part(C.byref(h), int(device), self.dim, self.etype, self.nv, self.nvo, len(self.cells), _ip(self.cells),
                                             _dp(self.x), len(fc), _ip(fc), _ip(fl), _ip(fm))
            else:
                rc = L.cfdh_create_elem(C.byref(h), int(device), self.dim, self.etype, self.nv, len(self.cells), _ip(self.cells), _dp(self.x),
                                        len(fc), _ip(fc), _ip(fl), _ip(fm))
        else:
            rc = L.cfdh_create(C.byref(h), int(device), self.dim, self.nv, self.nvo, len(self.cells), _ip(self.cells), _dp(self.x),
                               len(fc), _ip(fc), _ip(fl), _ip(fm))
        if rc != 0:
            _raise(rc, "cfdh_create failed: " + L.cfdh_last_error(None).decode())
        self.h = h
        self._cb = None

    def close(self):
        if getattr(self, "h", None):
            self.L.cfdh_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _chk(self, rc):
        if rc != 0:
            _raise(rc, self.L.cfdh_last_error(self.h).decode())

    def set_params(self, dt, rho, mu, mu_facet=None, f=(0.0, 0.0)):
        ff = np.zeros(3)
        f = np.atleast_1d(np.asarray(f, dtype=np.float64))[:3]
        ff[: len(f)] = f
        self._chk(self.L.cfdh_set_params(self.h, dt, rho, mu, mu if mu_facet is None else mu_facet, _dp(ff)))

    def default_options(self):
        o = Options()
        self.L.cfdh_default_options(C.byref(o))
        return o

    def set_options(self, o):
        self._chk(self.L.cfdh_set_options(self.h, C.byref(o)))
        self._ksp_restart = int(o.ksp_restart)  # sizes the trace arrays of fgmres_solve

    def clear_dirichlet(self):
        self._chk(self.L.cfdh_clear_dirichlet(self.h))

    def add_dirichlet(self, field, nodes, values):
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        values = np.ascontiguousarray(values, dtype=np.float64)
        self._chk(self.L.cfdh_add_dirichlet(self.h, int(field), len(nodes), _ip(nodes), _dp(values)))

    def update_dirichlet(self, field, nodes, values):
        """New values for dofs that are already constrained (no object added, diagonal counts unchanged)."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int32)
        values = np.ascontiguousarray(values, dtype=np.float64)
        self._chk(self.L.cfdh_update_dirichlet(self.h, int(field), len(nodes), _ip(nodes), _dp(values)))

    def set_state(self, u_prev=None, p_prev=None, u=None, p=None):
        a = [None if v is None else np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in (u_prev, p_prev, u, p)]
        for v, n in zip(a, (self.dim * self.nv, self.nv, self.dim * self.nv, self.nv)):
            if v is not None and v.size != n:
                raise ValueError("state array has wrong size")
        self._chk(self.L.cfdh_set_state(self.h, _dp(a[0]), _dp(a[1]), _dp(a[2]), _dp(a[3])))

    def get_solution(self, u=None, p=None):
        u = np.empty(self.dim * self.nv) if u is None else u
        p = np.empty(self.nv) if p is None else p
        self._chk(self.L.cfdh_get_solution(self.h, _dp(u), _dp(p)))
        return u, p

    def get_previous(self, u=None, p=None):
        u = np.empty(self.dim * self.nv) if u is None else u
        p = np.empty(self.nv) if p is None else p
        self._chk(self.L.cfdh_get_previous(self.h, _dp(u), _dp(p)))
        return u, p

    def get_residual(self):
        ru, rp = np.zeros(self.dim * self.nv), np.zeros(self.nv)
        self._chk(self.L.cfdh_get_residual(self.h, _dp(ru), _dp(rp)))
        return ru, rp

    def advance(self):
        self._chk(self.L.cfdh_advance(self.h))

    def advance_field(self, field):
        self._chk(self.L.cfdh_advance_field(self.h, int(field)))

    def set_time_scheme(self, theta, a0, a1, a2):
        self._chk(self.L.cfdh_set_time_scheme(self.h, float(theta), float(a0), float(a1), float(a2)))

    def set_facet_markers(self, markers):
        """Markers of the exterior facets in the order given to the constructor (Solver.setup's facet_tags)."""
        m = np.ascontiguousarray(markers, dtype=np.int32)
        self._chk(self.L.cfdh_set_facet_markers(self.h, len(m), _ip(m)))

    def set_boundary_terms(self, ds_terms=True, backflow_marker=-1, beta=0.0):
        self._chk(self.L.cfdh_set_boundary_terms(self.h, int(bool(ds_terms)), int(backflow_marker), float(beta)))

    def set_formulation(self, form):
        """FORM_CONVECTIVE (default) or FORM_ROTATIONAL (the curl-curl form of the pressure-driven solvers)."""
        self._chk(self.L.cfdh_set_formulation(self.h, int(form)))

    def set_pressure_boundaries(self, markers, values, beta_nitsche=0.0, nitsche=None, beta_backflow=None):
        """Natural pressure + Nitsche tangential terms on the exterior facets of each marker (rotational form).  A call that
        changes only `values` keeps the Jacobian and the preconditioner.  Per boundary (cfdh_set_pressure_boundaries_ex):
        `nitsche[k]` false drops the tangential terms there (None: all on), `beta_backflow[k]` > 0 adds the backflow
        stabilisation -beta rho (u_prev . n)_- (u_mid . v) (None: none)."""
        m = np.ascontiguousarray(markers, dtype=np.int32).reshape(-1)
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        if len(m) != len(v):
            raise ValueError("one value per pressure-boundary marker")
        if nitsche is None and beta_backflow is None:
            self._chk(self.L.cfdh_set_pressure_boundaries(self.h, len(m), _ip(m), _dp(v), float(beta_nitsche)))
            return
        nit = None if nitsche is None else np.ascontiguousarray(np.asarray(nitsche, dtype=bool), dtype=np.uint8).reshape(-1)
        bf = None if beta_backflow is None else np.ascontiguousarray(beta_backflow, dtype=np.float64).reshape(-1)
        if (nit is not None and len(nit) != len(m)) or (bf is not None and len(bf) != len(m)):
            raise ValueError("one Nitsche switch and one backflow coefficient per pressure-boundary marker")
        self._chk(self.L.cfdh_set_pressure_boundaries_ex(
            self.h, len(m), _ip(m), _dp(v), float(beta_nitsche),
            None if nit is None else nit.ctypes.data_as(C.POINTER(C.c_uint8)), None if bf is None else _dp(bf)))

    def set_traction_boundaries(self, markers, values, beta_nitsche=0.0, tangential=None, beta_backflow=None):
        """Traction boundaries of the convective form on the closed-form P1 kernels (cfdh_set_traction_boundaries): values[k] v . n
        and the viscous boundary stress on the exterior facets of markers[k]; `tangential[k]` true (None: all on) makes it the weak
        pressure inlet with its Nitsche tangential condition, `beta_backflow[k]` > 0 (None: none) adds the backflow stabilisation.
        A call that changes only `values` keeps the Jacobian and the preconditioner; empty lists remove the terms."""
        m = np.ascontiguousarray(markers, dtype=np.int32).reshape(-1)
        v = np.ascontiguousarray(values, dtype=np.float64).reshape(-1)
        if len(m) != len(v):
            raise ValueError("one value per traction-boundary marker")
        tg = None if tangential is None else np.ascontiguousarray(np.asarray(tangential, dtype=bool), dtype=np.uint8).reshape(-1)
        bf = None if beta_backflow is None else np.ascontiguousarray(beta_backflow, dtype=np.float64).reshape(-1)
        if (tg is not None and len(tg) != len(m)) or (bf is not None and len(bf) != len(m)):
            raise ValueError("one tangential switch and one backflow coefficient per traction-boundary marker")
        self._chk(self.L.cfdh_set_traction_boundaries(
            self.h, len(m), _ip(m), _dp(v), float(beta_nitsche),
            None if tg is None else tg.ctypes.data_as(C.POINTER(C.c_uint8)), None if bf is None else _dp(bf)))

    def wall_shear_stress(self, download=True):
        if not download:
            self._chk(self.L.cfdh_wall_shear_stress(self.h, None))
            return None
        out = np.zeros(self.dim * self.nv)
        self._chk(self.L.cfdh_wall_shear_stress(self.h, _dp(out)))
        return out

    def wall_stats_reset(self):
        """Zero the accumulators of the cycle-averaged wall shear indices (allocated on first use)."""
        self._chk(self.L.cfdh_wall_stats_reset(self.h))

    def wall_stats_accumulate(self, weight):
        """Add the wall shear stress of the current solution with this weight (the step's dt)."""
        self._chk(self.L.cfdh_wall_stats_accumulate(self.h, float(weight)))

    def wall_stats_get(self, which):
        """WALL_TAWSS / WALL_OSI / WALL_RRT / WALL_PEAK [nv], WALL_MEAN [nv, gdim], WALL_TOTALS (W, count) as float64."""
        n = C.c_int64()
        self._chk(self.L.cfdh_wall_stats_get(self.h, int(which), C.byref(n), None))
        out = np.empty(n.value)
        self._chk(self.L.cfdh_wall_stats_get(self.h, int(which), C.byref(n), _dp(out)))
        return out.reshape(-1, self.dim) if int(which) == WALL_MEAN else out

    def set_previous2(self, u_prev2):
        u_prev2 = np.ascontiguousarray(u_prev2, dtype=np.float64).reshape(-1)
        assert u_prev2.size == self.dim * self.nv
        self._chk(self.L.cfdh_set_previous2(self.h, _dp(u_prev2)))

    def get_previous2(self):
        u = np.empty(self.dim * self.nv)
        self._chk(self.L.cfdh_get_previous2(self.h, _dp(u)))
        return u

    def shift_history(self):
        self._chk(self.L.cfdh_shift_history(self.h))

    def assemble(self, want_jacobian=True):
        self._chk(self.L.cfdh_assemble(self.h, int(want_jacobian)))

    def get_csr(self):
        import scipy.sparse as sp
        nnz = C.c_int64()
        self._chk(self.L.cfdh_get_csr(self.h, C.byref(nnz), None, None, None))
        n1 = self.dim + 1
        rowptr = np.empty(n1 * self.nvo + 1, dtype=np.int32)
        col = np.empty(nnz.value, dtype=np.int32)
        val = np.empty(nnz.value)
        self._chk(self.L.cfdh_get_csr(self.h, C.byref(nnz), _ip(rowptr), _ip(col), _dp(val)))
        return sp.csr_matrix((val, col, rowptr), shape=(n1 * self.nvo, n1 * self.nv))

    def spmv(self, xvec):
        xvec = np.ascontiguousarray(xvec, dtype=np.float64)
        y = np.empty((self.dim + 1) * self.nvo)
        self._chk(self.L.cfdh_spmv(self.h, _dp(xvec), _dp(y)))
        return y

    def solve_step(self):
        st = Stats()
        rc = self.L.cfdh_solve_step(self.h, C.byref(st))
        if rc != 0:
            msg = self.L.cfdh_last_error(self.h).decode()
            if rc == -4:
                # the reference raises RuntimeError(f"Did not converge, reason: {reason}.") (stabilized_schur.py:332-334)
                raise RuntimeError("Did not converge, reason: %d. (%s)" % (st.reason, msg))
            _raise(rc, msg)
        return st

    def functional(self, kind, marker=0):
        out = C.c_double()
        self._chk(self.L.cfdh_functional(self.h, int(kind), int(marker), C.byref(out)))
        return out.value

    def set_halo(self, nbr_rank, send_ptr, send_idx, recv_ptr, recv_idx):
        a = np.ascontiguousarray(nbr_rank, dtype=np.int32)
        sp_ = np.ascontiguousarray(send_ptr, dtype=np.int64)
        si = np.ascontiguousarray(send_idx, dtype=np.int32)
        rp = np.ascontiguousarray(recv_ptr, dtype=np.int64)
        ri = np.ascontiguousarray(recv_idx, dtype=np.int32)
        self._chk(self.L.cfdh_set_halo(self.h, len(a), _ip(a), _lp(sp_), _ip(si), _lp(rp), _ip(ri)))

    def set_global_pressure_space(self, x_global, cells_global, owned_global, pbc_nodes_global):
        xg = np.ascontiguousarray(x_global, dtype=np.float64)[:, : self.dim].copy()
        cg = np.ascontiguousarray(cells_global, dtype=np.int32)
        og = np.ascontiguousarray(owned_global, dtype=np.int32)
        pb = np.ascontiguousarray(pbc_nodes_global, dtype=np.int32)
        self._chk(self.L.cfdh_set_global_pressure_space(self.h, len(xg), len(cg), _ip(cg), _dp(xg), _ip(og), len(pb), _ip(pb)))

    def comm_init_rccl(self, uid_bytes, rank, nranks):
        buf = C.create_string_buffer(bytes(uid_bytes), 128)
        self._chk(self.L.cfdh_comm_init(self.h, buf, int(rank), int(nranks)))

    def comm_set_callbacks(self, allreduce, exchange, rank, nranks):
        self._cb = (ALLREDUCE_FN(allreduce), EXCHANGE_FN(exchange))
        self._chk(self.L.cfdh_comm_set_callbacks(self.h, self._cb[0], self._cb[1], None, int(rank), int(nranks)))

    def profile_enable(self, on=True):
        self._chk(self.L.cfdh_profile_enable(self.h, int(on)))

    def profile_reset(self):
        self._chk(self.L.cfdh_profile_reset(self.h))

    def profile_get(self, kind):
        ms, n = C.c_double(), C.c_int64()
        self._chk(self.L.cfdh_profile_get(self.h, int(kind), C.byref(ms), C.byref(n)))
        return ms.value, n.value

    def info(self, what):
        return int(self.L.cfdh_info(self.h, int(what)))

    def set_schur_pcd(self, inlet_marker, outlet_marker, time_term=1):
        """Operator data of the PCD Schur approximation (options.pc_type = 2): inlet facets of the Robin term, outlet facets of
        A_p's Dirichlet rows, with (1) or without (0) the time term rho a0 / (theta dt) M in K."""
        self._chk(self.L.cfdh_set_schur_pcd(self.h, int(inlet_marker), int(outlet_marker), int(time_term)))

    def set_ksp_forcing(self, version=2, rtol_0=None, rtol_max=None, gamma=None, alpha=None, threshold=None):
        """Eisenstat-Walker forcing of the linear tolerance: version 0 off, 2 PETSc's default variant (defaults EW_DEFAULTS)."""
        a = [d if v is None else float(v) for v, d in zip((rtol_0, rtol_max, gamma, alpha, threshold), EW_DEFAULTS)]
        self._chk(self.L.cfdh_set_ksp_forcing(self.h, int(version), *a))

    def newton_history(self):
        """Per Newton iteration of the last step: dict of |F|, the linear tolerance, FGMRES iterations, achieved true |r| / |b|."""
        n = C.c_int32()
        self._chk(self.L.cfdh_get_newton_history(self.h, C.byref(n), None, None, None, None))
        fn, rt, rr = np.zeros(n.value), np.zeros(n.value), np.zeros(n.value)
        its = np.zeros(n.value, dtype=np.int32)
        self._chk(self.L.cfdh_get_newton_history(self.h, C.byref(n), _dp(fn), _dp(rt), _ip(its), _dp(rr)))
        return {"fnorm": fn, "ksp_rtol": rt, "ksp_its": its, "ksp_rel_res": rr}

    def get_pcd_operator(self):
        """(K as scipy CSR [nvo x nv] at the current state, M_d [nvo])."""
        import scipy.sparse as sp
        nnz = C.c_int64()
        self._chk(self.L.cfdh_get_pcd_operator(self.h, C.byref(nnz), None, None, None, None))
        rowptr = np.empty(self.nvo + 1, dtype=np.int32)
        col = np.empty(nnz.value, dtype=np.int32)
        val = np.empty(nnz.value)
        md = np.empty(self.nvo)
        self._chk(self.L.cfdh_get_pcd_operator(self.h, C.byref(nnz), _ip(rowptr), _ip(col), _dp(val), _dp(md)))
        return sp.csr_matrix((val, col, rowptr), shape=(self.nvo, self.nv)), md

    def apply_preconditioner(self, r):
        """z = P^-1 r with the current preconditioner on the assembled Jacobian (monolithic [u | p] vectors)."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        if r.size != (self.dim + 1) * self.nv:
            raise ValueError("monolithic vector of (gdim + 1) nv entries expected")
        z = np.zeros_like(r)
        self._chk(self.L.cfdh_apply_preconditioner(self.h, _dp(r), _dp(z)))
        return z

    def apply_operator(self, r):
        """(z, w) = (P^-1 r, J z) launched as one FGMRES iteration launches them (test entry; one GPU)."""
        r = np.ascontiguousarray(r, dtype=np.float64)
        if r.size != (self.dim + 1) * self.nv:
            raise ValueError("monolithic vector of (gdim + 1) nv entries expected")
        z = np.zeros_like(r)
        w = np.zeros((self.dim + 1) * self.nvo)
        self._chk(self.L.cfdh_apply_operator(self.h, _dp(r), _dp(z), _dp(w)))
        return z, w

    def fgmres_solve(self, b, newton_index=-1, trace=True, max_res=4096, max_cycles=256):
        """The step's own FGMRES on the caller's right-hand side (cfdh_fgmres_solve; test entry, one GPU): J d = b under the context's
        current options, from zero (newton_index -1) or from the projected guess of that Newton index's ring, which a converged solve
        then feeds.  Returns (x, its, reason, trace): `trace` (None unless asked for) is a dict describing the LAST cycle -- k, beta,
        V [k + 1, n], Z [k, n], H [k + 1, k] unrotated, ww / nrm2 / second_pass [k] of the first Gram-Schmidt pass, y [k], x_start --
        and the whole solve: bn, tol, cycles, guess_used, fp32_used, x0, res [its], cycle_beta / cycle_est [cycles]."""
        n = (self.dim + 1) * self.nv
        b = np.ascontiguousarray(b, dtype=np.float64)
        if b.size != n:
            raise ValueError("monolithic vector of (gdim + 1) nv entries expected")
        x = np.zeros(n)
        its, reason = C.c_int32(), C.c_int32()
        if not trace:
            self._chk(self.L.cfdh_fgmres_solve(self.h, _dp(b), int(newton_index), _dp(x), C.byref(its), C.byref(reason), None))
            return x, its.value, reason.value, None
        m = getattr(self, "_ksp_restart", None) or int(self.default_options().ksp_restart)
        a = {"V": np.zeros((m + 1, n)), "Z": np.zeros((m, n)), "H": np.zeros((m, m + 1)), "ww": np.zeros(m), "nrm2": np.zeros(m),
             "y": np.zeros(m), "x0": np.zeros(n), "x_start": np.zeros(n), "res": np.zeros(max_res), "cycle_beta": np.zeros(max_cycles),
             "cycle_est": np.zeros(max_cycles)}
        sp2 = np.zeros(m, dtype=np.int32)
        t = FgmresTrace(m=m, max_res=max_res, max_cycles=max_cycles, second_pass=_ip(sp2), **{k: _dp(v) for k, v in a.items()})
        self._chk(self.L.cfdh_fgmres_solve(self.h, _dp(b), int(newton_index), _dp(x), C.byref(its), C.byref(reason), C.byref(t)))
        k = t.k
        out = {"k": k, "cycles": t.cycles, "guess_used": bool(t.guess_used), "fp32_used": bool(t.fp32_used), "bn": t.bn, "tol": t.tol,
               "beta": t.beta, "V": a["V"][:k + 1].copy(), "Z": a["Z"][:k].copy(), "H": a["H"][:k, :k + 1].T.copy(),
               "ww": a["ww"][:k].copy(), "nrm2": a["nrm2"][:k].copy(), "second_pass": sp2[:k].copy(), "y": a["y"][:k].copy(),
               "x0": a["x0"], "x_start": a["x_start"], "res": a["res"][:min(t.n_res, max_res)].copy(),
               "cycle_beta": a["cycle_beta"][:min(t.cycles, max_cycles)].copy(), "cycle_est": a["cycle_est"][:min(t.cycles, max_cycles)].copy()}
        return x, its.value, reason.value, out

    def krylov_vec_op(self, op, n, ld, nvec=1, A=None, B=None, x=None, y=None, coef=None, scalar=0.0, flags=0):
        """One Krylov vector wrapper (KVOP_*) on caller data, launched as the solver launches it (test entry; one GPU).
        A, B: column-major blocks flattened to [ld * nvec]; x, y: [n]; coef: the op's coefficients.  Returns a dict with
        out1, out2 [n], out32 [n] (float32) and the scalars the wrapper returned (host), left on the device (dev) and wrote into
        the host-mapped words (mirror)."""
        def arr(a, need, what):
            if a is None:
                return None
            a = np.ascontiguousarray(a, dtype=np.float64).ravel()
            if a.size < need:
                raise ValueError("%s: %d entries, %d needed" % (what, a.size, need))
            return a
        blk = max(n, 0) if op == KVOP_NORM2_TRIPLE else max(ld, 0) * max(nvec, 0)
        ncoef = {KVOP_GS_UPDATE_NORMALIZE: nvec + 1, KVOP_GUESS: 8 * (nvec + 1)}.get(op, nvec)
        A, B = arr(A, blk, "A"), arr(B, blk, "B")
        x, y, coef = arr(x, n, "x"), arr(y, n, "y"), arr(coef, ncoef, "coef")
        m = max(n, 1)
        out1, out2, out32 = np.zeros(m), np.zeros(m), np.zeros(m, dtype=np.float32)
        ns = max(nvec + 2, 72)
        host, dev, mir = np.zeros(ns), np.zeros(ns), np.zeros(ns)
        cnt = np.zeros(3, dtype=np.int32)
        self._chk(self.L.cfdh_krylov_vec_op(self.h, int(op), int(n), int(ld), int(nvec), _dp(A), _dp(B), _dp(x), _dp(y), _dp(coef),
                                            float(scalar), int(flags), _dp(out1), _dp(out2), out32.ctypes.data_as(C.POINTER(C.c_float)),
                                            _ip(cnt), _dp(host), _dp(dev), _dp(mir)))
        return {"out1": out1, "out2": out2, "out32": out32, "host": host[:cnt[0]], "dev": dev[:cnt[1]], "mirror": mir[:cnt[2]]}

    # -- passive scalar transport (cfdh_scalar_*): closed-form P1 contexts, one GPU ------------------------------------
    def scalar_enable(self, D=0.0, s=0.0, theta_c=0.5):
        """dc/dt + w . grad c - D lap c = s on the vertices, advected by the flow step's velocity; allocates on first use, a
        later call changes the parameters and keeps c."""
        self._chk(self.L.cfdh_scalar_enable(self.h, float(D), float(s), float(theta_c)))

    def scalar_set_dirichlet(self, nodes, values):
        """Replaces the Dirichlet set of the scalar; empty arrays clear it."""
        nodes = np.ascontiguousarray(nodes, dtype=np.int32).reshape(-1)
        values = np.ascontiguousarray(np.broadcast_to(np.asarray(values, dtype=np.float64), nodes.shape))
        self._chk(self.L.cfdh_scalar_set_dirichlet(self.h, len(nodes), _ip(nodes), _dp(values)))

    def scalar_state(self, c=None):
        """Without an argument: the scalar field [nv]; with one: sets it."""
        if c is None:
            out = np.empty(self.nv)
            self._chk(self.L.cfdh_scalar_get_state(self.h, _dp(out)))
            return out
        c = np.ascontiguousarray(c, dtype=np.float64).reshape(-1)
        if c.size != self.nv:
            raise ValueError("one value per vertex expected")
        self._chk(self.L.cfdh_scalar_set_state(self.h, _dp(c)))
        return None

    def scalar_set_tolerances(self, rtol=1e-8, atol=1e-50, max_it=1000):
        self._chk(self.L.cfdh_scalar_set_tolerances(self.h, float(rtol), float(atol), int(max_it)))

    def scalar_step(self):
        """One transport step, after solve_step() and before advance()."""
        st = ScalarStats()
        rc = self.L.cfdh_scalar_step(self.h, C.byref(st))
        if rc != 0:
            msg = self.L.cfdh_last_error(self.h).decode()
            if rc == -4:
                raise RuntimeError("Did not converge, reason: %d. (%s)" % (st.reason, msg))
            _raise(rc, msg)
        return st

    def scalar_operator(self):
        """(left-hand matrix as scipy CSR [nv x nv], right-hand side [nv]) of the next transport step at the current state."""
        import scipy.sparse as sp
        nnz = C.c_int64()
        self._chk(self.L.cfdh_scalar_get_operator(self.h, C.byref(nnz), None, None, None, None))
        rowptr = np.empty(self.nv + 1, dtype=np.int32)
        col = np.empty(nnz.value, dtype=np.int32)
        val = np.empty(nnz.value)
        rhs = np.empty(self.nv)
        self._chk(self.L.cfdh_scalar_get_operator(self.h, C.byref(nnz), _ip(rowptr), _ip(col), _dp(val), _dp(rhs)))
        return sp.csr_matrix((val, col, rowptr), shape=(self.nv, self.nv)), rhs

    def scalar_functional(self, kind, marker=0):
        """SCALAR_INTEGRAL, SCALAR_FLUX (through the facets of `marker`), SCALAR_MIN, SCALAR_MAX."""
        out = C.c_double()
        self._chk(self.L.cfdh_scalar_functional(self.h, int(kind), int(marker), C.byref(out)))
        return out.value

    def scalar_krylov_solve(self, b, x0, rtol, atol, max_it):
        """The transport step's BiCGStab + Jacobi on the caller's right-hand side and initial guess, on the left-hand matrix of the
        next step (cfdh_scalar_krylov_solve).  Returns (x, its, reason, rel_res, scalars, p): `scalars` holds the 16 words of the
        device scalar block, indexed by SC_RHO .. SC_BAD, `p` the search direction.  A capped solve returns, it does not raise."""
        b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1)
        if b.size != self.nv or x0.size != self.nv:
            raise ValueError("one value per vertex expected")
        x, p, scal, st = np.empty(self.nv), np.empty(self.nv), np.zeros(SC_NSCAL), ScalarStats()
        self._chk(self.L.cfdh_scalar_krylov_solve(self.h, _dp(b), _dp(x0), float(rtol), float(atol), int(max_it), _dp(x), C.byref(st),
                                                  _dp(scal), _dp(p)))
        return x, st.its, st.reason, st.rel_res, scal, p

    # -- Lagrangian particle tracking (cfdh_particles_*): closed-form P1 contexts, one GPU ------------------------------
    def particles_enable(self, capacity, nsub=2):
        """Room for `capacity` particles and the neighbour / affine-map tables; a later call may change nsub only."""
        self._chk(self.L.cfdh_particles_enable(self.h, int(capacity), int(nsub)))

    def particles_seed(self, x, cell, t_birth=0.0):
        """Appends active particles at x [n, gdim] in the cells `cell` [n] (the constructor's cell numbering)."""
        x = np.ascontiguousarray(x, dtype=np.float64).reshape(-1, self.dim)
        cell = np.ascontiguousarray(cell, dtype=np.int32).reshape(-1)
        if len(cell) != len(x):
            raise ValueError("one cell per particle")
        self._chk(self.L.cfdh_particles_seed(self.h, len(x), _dp(x), _ip(cell), float(t_birth)))

    def particles_clear(self):
        self._chk(self.L.cfdh_particles_clear(self.h))

    def particles_step(self, t0):
        """One step over [t0, t0 + dt], after solve_step() and before advance().  Returns the ParticleStats."""
        st = ParticleStats()
        self._chk(self.L.cfdh_particles_step(self.h, float(t0), C.byref(st)))
        return st

    def particles_count(self):
        n = C.c_int64(0)
        self._chk(self.L.cfdh_particles_get(self.h, PARTICLE_X, C.byref(n), None))
        return int(n.value)

    def particles_get(self, which):
        """Field `which` (PARTICLE_X .. PARTICLE_T_END) of all particles in seeding order."""
        n = C.c_int64(0)
        self._chk(self.L.cfdh_particles_get(self.h, int(which), C.byref(n), None))
        m = int(n.value)
        if which == PARTICLE_X:
            out = np.zeros((m, self.dim))
        elif which in (PARTICLE_CELL, PARTICLE_STATUS):
            out = np.zeros(m, dtype=np.int32)
        else:
            out = np.zeros(m)
        if m:
            self._chk(self.L.cfdh_particles_get(self.h, int(which), C.byref(n), out.ctypes.data_as(C.c_void_p)))
        return out

    # -- volumetric flow diagnostics (cfdh_flow_*): closed-form P1 contexts, one GPU -------------------------------------------
    def flow_field(self, which):
        """FLOW_GRADIENT [nv, d, d], FLOW_VORTICITY [nv] (2-D) / [nv, 3], FLOW_Q / FLOW_SHEAR_RATE / FLOW_DISSIPATION / FLOW_HELICITY /
        FLOW_LNH [nv] of the current u_sol, recovered to the vertices."""
        n = C.c_int64()
        self._chk(self.L.cfdh_flow_field(self.h, int(which), C.byref(n), None))
        out = np.empty(n.value)
        self._chk(self.L.cfdh_flow_field(self.h, int(which), C.byref(n), _dp(out)))
        if int(which) == FLOW_GRADIENT:
            return out.reshape(-1, self.dim, self.dim)
        return out.reshape(-1, 3) if int(which) == FLOW_VORTICITY and self.dim == 3 else out

    def flow_integrals(self):
        """The 8 cell-exact integrals of the current u_sol (FLOW_INT_VOLUME .. FLOW_INT_DIV2)."""
        out = np.empty(8)
        self._chk(self.L.cfdh_flow_integrals(self.h, _dp(out)))
        return out

    def flow_stats_reset(self):
        """Zero the accumulators of the window averages (allocated on first use)."""
        self._chk(self.L.cfdh_flow_stats_reset(self.h))

    def flow_stats_accumulate(self, weight):
        """Add the current u_sol and its recovered shear rate / dissipation with this weight (the step's dt)."""
        self._chk(self.L.cfdh_flow_stats_accumulate(self.h, float(weight)))

    def flow_stats_get(self, which):
        """FLOW_MEAN_U [nv, gdim], FLOW_FLUCTUATION / FLOW_MEAN_DISSIPATION / FLOW_MEAN_SHEAR_RATE / FLOW_PEAK_SHEAR_RATE [nv],
        FLOW_TOTALS (W, count)."""
        n = C.c_int64()
        self._chk(self.L.cfdh_flow_stats_get(self.h, int(which), C.byref(n), None))
        out = np.empty(n.value)
        self._chk(self.L.cfdh_flow_stats_get(self.h, int(which), C.byref(n), _dp(out)))
        return out.reshape(-1, self.dim) if int(which) == FLOW_MEAN_U else out

    # -- point sampler (cfdh_sample_*): closed-form P1 contexts, one GPU ---------------------------------------------------------
    def sample_set_points(self, x, tol=SAMPLE_TOL):
        """Explicit points [n, gdim]; located once, on the device.  An empty array removes the set."""
        x = np.ascontiguousarray(np.asarray(x, dtype=np.float64).reshape(-1, self.dim))
        self._chk(self.L.cfdh_sample_set_points(self.h, len(x), _dp(x) if len(x) else None, float(tol)))

    def sample_set_grid(self, origin, spacing, dims, tol=SAMPLE_TOL):
        """A regular grid: node (i, j, k) at origin + (i, j, k) * spacing, index i + dims[0] (j + dims[1] k); generated on the device."""
        o, h, d = np.zeros(3), np.ones(3), np.ones(3, dtype=np.int64)
        o[:len(origin)], h[:len(spacing)], d[:len(dims)] = origin, spacing, dims
        self._chk(self.L.cfdh_sample_set_grid(self.h, _dp(o), _dp(h), _lp(d), float(tol)))

    def sample_location(self):
        """(cell [n] in the caller's numbering, -1: none; lambda [n, gdim + 1]; x [n, gdim] as the device used them)."""
        n = C.c_int64()
        self._chk(self.L.cfdh_sample_get_location(self.h, C.byref(n), None, None, None))
        cell, lam, x = np.empty(n.value, dtype=np.int32), np.empty((n.value, self.dim + 1)), np.empty((n.value, self.dim))
        if n.value:
            self._chk(self.L.cfdh_sample_get_location(self.h, C.byref(n), _ip(cell), _dp(lam), _dp(x)))
        return cell, lam, x

    def sample_now(self):
        """[n, gdim + 1]: the rows (u, p) of the current state at the points of the set; zeros at unlocated points."""
        n = C.c_int64()
        self._chk(self.L.cfdh_sample_now(self.h, C.byref(n), None))
        out = np.empty((n.value, self.dim + 1))
        self._chk(self.L.cfdh_sample_now(self.h, C.byref(n), _dp(out)))
        return out

    def sample_series_enable(self, rows):
        """Room for `rows` row blocks on the device (0 frees it)."""
        self._chk(self.L.cfdh_sample_series_enable(self.h, int(rows)))

    def sample_record(self, t):
        """Append the rows of the current state to the series: one launch, no synchronisation, no copy."""
        self._chk(self.L.cfdh_sample_record(self.h, float(t)))

    def sample_series_get(self):
        """(t [rows], out [rows, n, gdim + 1]) of what was recorded; empties the buffer."""
        rows = C.c_int64()
        self._chk(self.L.cfdh_sample_series_get(self.h, C.byref(rows), None, None))
        n = self.info(INFO_SAMPLE_POINTS)
        t, out = np.empty(rows.value), np.empty((rows.value, n, self.dim + 1))
        self._chk(self.L.cfdh_sample_series_get(self.h, C.byref(rows), _dp(t), _dp(out)))
        return t, out

    def sample_mean_reset(self):
        """Zero the per-point accumulators of the means (allocated on first use)."""
        self._chk(self.L.cfdh_sample_mean_reset(self.h))

    def sample_mean_accumulate(self, weight):
        """Add the rows of the current state with this weight (the step's dt)."""
        self._chk(self.L.cfdh_sample_mean_accumulate(self.h, float(weight)))

    def sample_mean_get(self, which):
        """SAMPLE_MEAN_U [n, gdim], SAMPLE_MEAN_P / SAMPLE_FLUCTUATION [n], SAMPLE_TOTALS (W, count)."""
        n = C.c_int64()
        self._chk(self.L.cfdh_sample_mean_get(self.h, int(which), C.byref(n), None))
        out = np.empty(n.value)
        self._chk(self.L.cfdh_sample_mean_get(self.h, int(which), C.byref(n), _dp(out)))
        return out.reshape(-1, self.dim) if int(which) == SAMPLE_MEAN_U else out

    # -- cut-plane sections (cfdh_section_*): closed-form P1 contexts, one GPU ----------------------------------------------------
    def section_set(self, origin, normal, radius=None):
        """K sections: origin [K, gdim], normal [K, gdim] (any non-zero length), radius [K] or None (<= 0: unbounded).  The cut is
        built once, on the host.  Empty arrays remove the set."""
        o = np.ascontiguousarray(np.asarray(origin, dtype=np.float64).reshape(-1, self.dim))
        n = np.ascontiguousarray(np.asarray(normal, dtype=np.float64).reshape(-1, self.dim))
        if len(o) != len(n):
            raise ValueError("section_set: %d origins and %d normals" % (len(o), len(n)))
        r = None
        if radius is not None:
            r = np.ascontiguousarray(np.asarray(radius, dtype=np.float64).reshape(-1))
            if len(r) != len(o):
                raise ValueError("section_set: %d origins and %d radii" % (len(o), len(r)))
        K = len(o)
        self._chk(self.L.cfdh_section_set(self.h, K, _dp(o) if K else None, _dp(n) if K else None, _dp(r) if r is not None and K else None))

    def section_get_cut(self):
        """(ptr [K + 1], cell [entries] in the caller's numbering, measure [entries], straddling [K]) of the cut lists."""
        K = C.c_int32()
        self._chk(self.L.cfdh_section_get_cut(self.h, C.byref(K), None, None, None, None))
        ptr, strad = np.zeros(K.value + 1, dtype=np.int64), np.zeros(K.value, dtype=np.int32)
        if K.value:
            self._chk(self.L.cfdh_section_get_cut(self.h, C.byref(K), _lp(ptr), None, None, _ip(strad)))
        cell, meas = np.empty(int(ptr[-1]), dtype=np.int32), np.empty(int(ptr[-1]))
        if ptr[-1]:
            self._chk(self.L.cfdh_section_get_cut(self.h, C.byref(K), None, _ip(cell), _dp(meas), None))
        return ptr, cell, meas, strad

    def section_now(self):
        """[K, 10]: the rows of the current state (SECTION_AREA .. SECTION_UZ)."""
        K = C.c_int32()
        self._chk(self.L.cfdh_section_now(self.h, C.byref(K), None))
        out = np.empty((K.value, SECTION_NQ))
        self._chk(self.L.cfdh_section_now(self.h, C.byref(K), _dp(out)))
        return out

    def section_series_enable(self, rows):
        """Room for `rows` row blocks on the device (0 frees it)."""
        self._chk(self.L.cfdh_section_series_enable(self.h, int(rows)))

    def section_record(self, t):
        """Append the rows of the current state to the series: no synchronisation, no copy."""
        self._chk(self.L.cfdh_section_record(self.h, float(t)))

    def section_series_get(self):
        """(t [rows], out [rows, K, 10]) of what was recorded; empties the buffer."""
        rows = C.c_int64()
        self._chk(self.L.cfdh_section_series_get(self.h, C.byref(rows), None, None))
        K = self.info(INFO_SECTION_COUNT)
        t, out = np.empty(rows.value), np.empty((rows.value, K, SECTION_NQ))
        self._chk(self.L.cfdh_section_series_get(self.h, C.byref(rows), _dp(t), _dp(out)))
        return t, out

    def section_mean_reset(self):
        """Zero the K x 10 accumulators of the window means (allocated on first use)."""
        self._chk(self.L.cfdh_section_mean_reset(self.h))

    def section_mean_accumulate(self, weight):
        """Add the rows of the current state with this weight (the step's dt)."""
        self._chk(self.L.cfdh_section_mean_accumulate(self.h, float(weight)))

    def section_mean_get(self):
        """(rows [K, 10] = sum w row / W, or None while nothing is accumulated; W; count)."""
        K, wc = C.c_int32(), np.zeros(2)
        self._chk(self.L.cfdh_section_mean_get(self.h, C.byref(K), None, _dp(wc)))
        if not wc[0] > 0.0:
            return None, float(wc[0]), int(wc[1])
        out = np.empty((K.value, SECTION_NQ))
        self._chk(self.L.cfdh_section_mean_get(self.h, C.byref(K), _dp(out), _dp(wc)))
        return out, float(wc[0]), int(wc[1])

    def scalar_order(self):
        """The device row of every vertex (cfdh_scalar_get_order)."""
        row = np.empty(self.nv, dtype=np.int32)
        self._chk(self.L.cfdh_scalar_get_order(self.h, _ip(row)))
        return row

    def get_amg_operator(self, hier, level, which, raw=False):
        """One operator of a built hierarchy as scipy CSR (AMG_HIER_*, AMG_OP_*); level-0 indices in the caller's numbering.
        raw: the (rowptr, col, vals, shape) arrays as downloaded, unchecked (scipy would sum duplicates and sort)."""
        import scipy.sparse as sp
        nr, nc, nnz = C.c_int64(), C.c_int64(), C.c_int64()
        self._chk(self.L.cfdh_get_amg_operator(self.h, int(hier), int(level), int(which), C.byref(nr), C.byref(nc), C.byref(nnz), None, None, None))
        rowptr = np.empty(nr.value + 1, dtype=np.int32)
        col = np.empty(nnz.value, dtype=np.int32)
        val = np.empty(nnz.value)
        self._chk(self.L.cfdh_get_amg_operator(self.h, int(hier), int(level), int(which), C.byref(nr), C.byref(nc), C.byref(nnz), _ip(rowptr),
                                               _ip(col), _dp(val)))
        if raw:
            return rowptr, col, val, (nr.value, nc.value), nnz.value
        return sp.csr_matrix((val, col, rowptr), shape=(nr.value, nc.value))

    def get_amg_head(self, hier, level, which):
        """Width of the head copy of one SELL-64 operator (AMG_HIER_*, AMG_OP_SB / _SC, AMG_OP_A of AMG_HIER_H); 0: it has none."""
        w = C.c_int32()
        self._chk(self.L.cfdh_get_amg_head(self.h, int(hier), int(level), int(which), C.byref(w)))
        return w.value

    def get_amg_vectors(self, hier, level, which):
        """Vectors / scalars of a built hierarchy as float64 (AMG_VEC_*)."""
        n = C.c_int64()
        self._chk(self.L.cfdh_get_amg_vectors(self.h, int(hier), int(level), int(which), C.byref(n), None))
        out = np.empty(n.value)
        self._chk(self.L.cfdh_get_amg_vectors(self.h, int(hier), int(level), int(which), C.byref(n), _dp(out)))
        return out


class IpcsContext(Context):
    """Owner of a cfdh_ctx made by cfdh_create_ipcs: the incremental pressure-correction scheme on P2/P1 triangles or tetrahedra.
    `x`, `cells`: the P2 node mesh (elements.NodeMesh / NodeMesh3D: vertices first), `nvert`: number of vertices (= pressure dofs).
    Velocity arrays have nn * gdim entries, pressure arrays nvert."""

    def __init__(self, x, cells, nvert, facet_cells, facet_local, facet_marker, device=0):
        L = lib()
        self.L = L
        cells = np.ascontiguousarray(cells, dtype=np.int32)
        if cells.ndim != 2 or cells.shape[1] not in (6, 10):
            raise ValueError("cells must list the 6 nodes of P2 triangles or the 10 nodes of P2 tetrahedra")
        self.dim = 2 if cells.shape[1] == 6 else 3
        self.etype = 1
        self.x = np.ascontiguousarray(np.asarray(x, dtype=np.float64)[:, : self.dim]).copy()
        self.cells = cells
        self.nv = self.nvo = len(self.x)
        self.nvert = int(nvert)
        fc = np.ascontiguousarray(facet_cells, dtype=np.int32)
        fl = np.ascontiguousarray(facet_local, dtype=np.int32)
        fm = np.ascontiguousarray(facet_marker, dtype=np.int32)
        h = C.c_void_p()
        rc = L.cfdh_create_ipcs(C.byref(h), int(device), self.dim, self.nv, self.nvert, len(cells), _ip(cells), _dp(self.x), len(fc), _ip(fc), _ip(fl),
                                _ip(fm))
        if rc != 0:
            _raise(rc, "cfdh_create_ipcs failed: " + L.cfdh_last_error(None).decode())
        self.h = h
        self._cb = None

    def set_state(self, u_prev=None, p_prev=None, u=None, p=None):
        a = [None if v is None else np.ascontiguousarray(v, dtype=np.float64).reshape(-1) for v in (u_prev, p_prev, u, p)]
        for v, n in zip(a, (self.dim * self.nv, self.nvert, self.dim * self.nv, self.nvert)):
            if v is not None and v.size != n:
                raise ValueError("state array has wrong size")
        self._chk(self.L.cfdh_set_state(self.h, _dp(a[0]), _dp(a[1]), _dp(a[2]), _dp(a[3])))

    def get_solution(self, u=None, p=None):
        u = np.empty(self.dim * self.nv) if u is None else u
        p = np.empty(self.nvert) if p is None else p
        self._chk(self.L.cfdh_get_solution(self.h, _dp(u), _dp(p)))
        return u, p

    def get_previous(self, u=None, p=None):
        u = np.empty(self.dim * self.nv) if u is None else u
        p = np.empty(self.nvert) if p is None else p
        self._chk(self.L.cfdh_get_previous(self.h, _dp(u), _dp(p)))
        return u, p

    def wall_shear_stress(self, download=True):
        """Wall shear stress of the P2 u_sol as a P1 field on the vertices, nvert * gdim values."""
        if not download:
            self._chk(self.L.cfdh_wall_shear_stress(self.h, None))
            return None
        out = np.zeros(self.dim * self.nvert)
        self._chk(self.L.cfdh_wall_shear_stress(self.h, _dp(out)))
        return out

    def set_form(self, conv_coeff, force_coeff):
        """Coefficients c (convection) and s_f (force) of the scheme; the context's default is (rho, +rho)."""
        self._chk(self.L.cfdh_ipcs_set_form(self.h, float(conv_coeff), float(force_coeff)))

    def set_scheme(self, scheme):
        """IPCS_BDF2 (0, the default) or IPCS_MIDPOINT (1, or the name "midpoint"): cfdh_ipcs_set_scheme."""
        k = {"bdf2": IPCS_BDF2, "ipcs_bdf2": IPCS_BDF2, "midpoint": IPCS_MIDPOINT, "ipcs_midpoint": IPCS_MIDPOINT}.get(scheme, scheme)
        self._chk(self.L.cfdh_ipcs_set_scheme(self.h, int(k)))

    def get_block_operator(self, which):
        """scipy BSR of size gdim * nn with gdim x gdim blocks on the P2 node pattern (ipcs_midpoint): 0 A1 with the Dirichlet
        treatment, 1 A1_free.  Rows and columns are (node, component), as the interleaved velocity arrays."""
        import scipy.sparse as sp
        nnz = C.c_int64()
        self._chk(self.L.cfdh_ipcs_get_block_operator(self.h, int(which), C.byref(nnz), None, None, None))
        d = self.dim
        rowptr = np.empty(self.nv + 1, dtype=np.int32)
        col = np.empty(nnz.value, dtype=np.int32)
        val = np.empty((nnz.value, d, d))
        self._chk(self.L.cfdh_ipcs_get_block_operator(self.h, int(which), C.byref(nnz), _ip(rowptr), _ip(col), _dp(val)))
        return sp.bsr_matrix((val, col, rowptr), shape=(d * self.nv, d * self.nv))

    def set_tolerances(self, rtol=(1e-5, 1e-5, 1e-5), atol=1e-50, max_it=(10000, 10000, 10000)):
        r = np.ascontiguousarray(np.broadcast_to(np.asarray(rtol, dtype=np.float64), (3,)))
        m = np.ascontiguousarray(np.broadcast_to(np.asarray(max_it, dtype=np.int32), (3,)))
        self._chk(self.L.cfdh_ipcs_set_tolerances(self.h, _dp(r), float(atol), _ip(m)))

    def step(self):
        st = IpcsStats()
        rc = self.L.cfdh_ipcs_step(self.h, C.byref(st))
        if rc != 0:
            msg = self.L.cfdh_last_error(self.h).decode()
            if rc == -4:
                bad = [r for r in st.reason if r <= 0]
                raise RuntimeError("Did not converge, reason: %d. (%s)" % (bad[0] if bad else 0, msg))
            _raise(rc, msg)
        return st

    def get_operator(self, which):
        """scipy CSR: 0 A1 (Dirichlet treatment included), 1 L, 2 rho M, 3.. B_d, 3 + gdim.. G_d."""
        import scipy.sparse as sp
        nnz = C.c_int64()
        self._chk(self.L.cfdh_ipcs_get_operator(self.h, int(which), C.byref(nnz), None, None, None))
        d = self.dim
        shape = (self.nvert, self.nvert) if which == 1 else (self.nv, self.nv) if which < 3 else (self.nvert, self.nv) if which < 3 + d \
            else (self.nv, self.nvert)
        rowptr = np.empty(shape[0] + 1, dtype=np.int32)
        col = np.empty(nnz.value, dtype=np.int32)
        val = np.empty(nnz.value)
        self._chk(self.L.cfdh_ipcs_get_operator(self.h, int(which), C.byref(nnz), _ip(rowptr), _ip(col), _dp(val)))
        return sp.csr_matrix((val, col, rowptr), shape=shape)

    def get_intermediate(self, which):
        """0 u*, 1 phi, 2 b1, 3 b2, 4 b3 of the last step / assembly; 5, 6: the search direction of the last velocity-sized /
        pressure Krylov solve."""
        out = np.empty(self.nvert if which in (1, 3, 6) else self.dim * self.nv)
        self._chk(self.L.cfdh_ipcs_get_intermediate(self.h, int(which), _dp(out)))
        return out

    def apply_pressure_pc(self, r):
        r = np.ascontiguousarray(r, dtype=np.float64)
        if r.size != self.nvert:
            raise ValueError("one value per vertex expected")
        z = np.zeros_like(r)
        self._chk(self.L.cfdh_ipcs_apply_pressure_pc(self.h, _dp(r), _dp(z)))
        return z

    def krylov_solve(self, which, b, x0, rtol, atol, max_it):
        """One Krylov driver of the step on the caller's right-hand side and initial guess (cfdh_ipcs_krylov_solve): which 0
        BiCGStab on A1, 1 flexible PCG on L, 2 CG on rho M.  Returns (x, its, reason, rel_res, scalars); `scalars` holds the 16
        words of the device scalar block, indexed by IP_RHO .. IP_BAD.  A capped solve returns, it does not raise."""
        n = self.nvert if which == 1 else self.dim * self.nv
        b = np.ascontiguousarray(b, dtype=np.float64).reshape(-1)
        x0 = np.ascontiguousarray(x0, dtype=np.float64).reshape(-1)
        if which in (0, 1, 2) and (b.size != n or x0.size != n):
            raise ValueError("b and x0 need %d entries" % n)
        x, scal, st = np.empty(n), np.zeros(IP_NSCAL), IpcsStats()
        self._chk(self.L.cfdh_ipcs_krylov_solve(self.h, int(which), _dp(b), _dp(x0), float(rtol), float(atol), int(max_it), _dp(x),
                                                C.byref(st), _dp(scal)))
        k = int(which)
        return x, st.its[k], st.reason[k], st.rel_res[k], scal


def rccl_unique_id():
    buf = C.create_string_buffer(128)
    rc = lib().cfdh_comm_unique_id(buf)
    if rc != 0:
        raise CfdhError("cfdh_comm_unique_id failed: " + lib().cfdh_last_error(None).decode())
    return bytes(buf.raw)
