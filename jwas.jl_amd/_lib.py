"""ctypes binding of libjwas_hip.so (the C ABI declared in include/jwas_hip.h).

The library is built in-tree by jwas.jl_amd/csrc/build.sh (hipcc --offload-arch=gfx950).  There is
no CPU fallback: if the shared object is missing or no gfx950 device is present, loading /
context creation raises.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libjwas_hip.so")

MAX_TRAITS = 4
MAX_STATES = 16

BAYESC, BAYESB, BAYESR, MTBAYESC1, MTBAYESC2, MEGABAYESC, MTBAYESB1, MTBAYESB2, MEGABAYESB = 0, 1, 2, 3, 4, 5, 6, 7, 8
GRAM_F64, GRAM_MFMA = 0, 1

ANNOT_MAX_COLS = 64                     # columns of the annotation design matrix, the intercept included (JWAS_HIP_ANNOT_MAX_COLS)
ANNOT_BAYESC, ANNOT_BAYESR, ANNOT_TREE = 0, 1, 2
LOCPAR_MAX_GROUPS = 8                   # random effects per model (JWAS_HIP_LOCPAR_MAX_GROUPS)
RRM_MIN_COEFF, RRM_MAX_COEFF, RRM_MAX_TIMES, RRM_MAX_BLOCK = 2, 4, 64, 256      # csrc/rrm.hpp
MEGA_MAX_TRAITS, MEGA_MAX_BLOCK, MEGA_TRAIT_TILE = 64, 256, 8                   # csrc/mega.hpp (JWAS_HIP_MEGA_MAX_TRAITS, _MAX_BLOCK, kTT)
MTJ_MIN_TRAITS, MTJ_MAX_TRAITS = 5, 8                                           # csrc/mtjoint.hpp (JWAS_HIP_MTJ_MIN_TRAITS, _MAX_TRAITS)
GRM_CHUNK = 64                          # markers per fp32 accumulation chunk of jwas_hip_grm (JWAS_HIP_GRM_CHUNK, csrc/gblup.hpp kGrmChunk)
SS_CHUNK_GRANULE, SS_MAX_CHUNK = 64, 65536                                     # csrc/ssbr.hpp (kChunkGranule, kMaxChunk)
MAX_THRESHOLDS = 16                     # per categorical trait, -Inf and +Inf included
STORAGE_DENSE_F32, STORAGE_PACKED2BIT = 0, 1
# enum jwas_hip_schedule_flags (jwas_hip_last_sweep_schedule): name -> bit
SCHEDULE_FLAGS = {
    "INDEPENDENT": 1 << 0, "GROUPED": 1 << 1, "GROUP_PP_KERNEL": 1 << 2, "GROUP_PINGPONG": 1 << 3, "GROUP_COOP": 1 << 4,
    "QUIET_XCD": 1 << 5, "COOP_APPLY": 1 << 6, "DENSE_BIG": 1 << 7, "DENSE_MT": 1 << 8, "CORR_HELPER": 1 << 9,
    "SECTION_SOLVE": 1 << 10,
}
SCHEDULE_COMPACT_OFF_SHIFT, SCHEDULE_COMPACT_OFF_MASK = 11, 3 << 11


class SweepParams(C.Structure):
    _fields_ = [
        ("method", C.c_int32), ("ntraits", C.c_int32), ("nreps", C.c_int32), ("iteration", C.c_uint32),
        ("seed", C.c_uint64), ("marker_offset", C.c_uint32), ("independent_blocks", C.c_uint32),
        ("vare", C.c_float * (MAX_TRAITS * MAX_TRAITS)),
        ("var_effect", C.c_float * (MAX_TRAITS * MAX_TRAITS)),
        ("pi", C.c_double), ("pi_classes", C.c_double * 4), ("gamma", C.c_double * 4),
        ("log_prior_states", C.c_double * MAX_STATES),
        ("var_effect_vec", C.POINTER(C.c_float)),
        ("pi_vec", C.POINTER(C.c_double)),
        ("pi_matrix", C.POINTER(C.c_double)),
        ("log_prior_states_matrix", C.POINTER(C.c_double)),
        ("var_effect_matrix", C.POINTER(C.c_float)),
        ("vare_f64", C.c_double * (MAX_TRAITS * MAX_TRAITS)),
        ("var_effect_f64", C.c_double * (MAX_TRAITS * MAX_TRAITS)),
        ("var_effect_vec_f64", C.POINTER(C.c_double)),
        ("section_solve", C.c_int32),
        ("group_launch", C.c_int32),
    ]


class SweepStats(C.Structure):
    _fields_ = [
        ("sum_delta", C.c_double * MAX_TRAITS),
        ("alpha_ss", C.c_double * (MAX_TRAITS * MAX_TRAITS)),
        ("beta_ss", C.c_double * (MAX_TRAITS * MAX_TRAITS)),
        ("resid_ss", C.c_double * (MAX_TRAITS * MAX_TRAITS)),
        ("resid_sum", C.c_double * MAX_TRAITS),
        ("class_counts", C.c_double * 4),
        ("bayesr_ssq", C.c_double), ("bayesr_nnz", C.c_double),
        ("state_counts", C.c_double * MAX_STATES),
        ("n_events", C.c_double), ("sweep_ms", C.c_double),
        ("update_kernel_ms", C.c_double), ("update_kernel_samples", C.c_double), ("update_kernel_bytes", C.c_double),
        ("event_overhead_ms", C.c_double),
    ]


class LiabilityParams(C.Structure):
    _fields_ = [("iteration", C.c_uint32), ("ngibbs", C.c_int32), ("seed", C.c_uint64), ("R", C.c_double * (MAX_TRAITS * MAX_TRAITS))]


class LocparParams(C.Structure):
    _fields_ = [("iteration", C.c_uint32), ("first_term", C.c_int32), ("last_term", C.c_int32), ("reserved", C.c_int32),
                ("seed", C.c_uint64), ("vare", C.c_double), ("Rinv", C.c_double * (MAX_TRAITS * MAX_TRAITS)),
                ("Gi", C.c_double * (LOCPAR_MAX_GROUPS * 16))]


class LocparStats(C.Structure):
    _fields_ = [("utu", C.c_double * (LOCPAR_MAX_GROUPS * 16)), ("step_ms", C.c_double)]


class MtmissParams(C.Structure):
    _fields_ = [("iteration", C.c_uint32), ("reserved", C.c_uint32), ("seed", C.c_uint64), ("B", C.c_void_p), ("U", C.c_void_p)]


class AnnotParams(C.Structure):
    _fields_ = [("iteration", C.c_uint32), ("reserved", C.c_uint32), ("seed", C.c_uint64), ("variance", C.c_double * 3)]


class AnnotStats(C.Structure):
    _fields_ = [("coef", C.c_double * (3 * ANNOT_MAX_COLS)), ("n_active", C.c_int64 * 3), ("means", C.c_double * 4), ("step_ms", C.c_double)]


class SemParams(C.Structure):
    _fields_ = [("iteration", C.c_uint32), ("reserved", C.c_uint32), ("seed", C.c_uint64), ("R_diag", C.c_double * MAX_TRAITS)]


class SemStats(C.Structure):
    _fields_ = [("lambda_", C.c_double * (MAX_TRAITS * MAX_TRAITS)), ("mean", C.c_double * (MAX_TRAITS * MAX_TRAITS)),
                ("ypr", C.c_double * (MAX_TRAITS * MAX_TRAITS)), ("step_ms", C.c_double)]


class RrmParams(C.Structure):
    _fields_ = [("iteration", C.c_uint32), ("reserved", C.c_uint32), ("seed", C.c_uint64), ("vare", C.c_double),
                ("G", C.c_double * (MAX_TRAITS * MAX_TRAITS)), ("log_pi", C.c_double * MAX_STATES)]


class RrmStats(C.Structure):
    _fields_ = [("state_counts", C.c_double * MAX_STATES), ("beta_ss", C.c_double * (MAX_TRAITS * MAX_TRAITS)), ("alpha_ss", C.c_double),
                ("resid_ss", C.c_double), ("n_changed", C.c_double), ("step_ms", C.c_double)]


class MegaParams(C.Structure):
    _fields_ = [("iteration", C.c_uint32), ("reserved", C.c_uint32), ("seed", C.c_uint64), ("vare", C.c_void_p), ("var_effect", C.c_void_p),
                ("pi", C.c_void_p)]


class MegaStats(C.Structure):
    _fields_ = [("sum_delta", C.c_void_p), ("beta_ss", C.c_void_p), ("alpha_ss", C.c_void_p), ("resid_ss", C.c_void_p), ("resid_sum", C.c_void_p),
                ("n_changed", C.c_void_p), ("step_ms", C.c_double)]


class MtjParams(C.Structure):
    _fields_ = [("iteration", C.c_uint32), ("reserved", C.c_uint32), ("seed", C.c_uint64), ("rinv", C.c_void_p), ("ginv", C.c_void_p),
                ("log_pi", C.c_void_p), ("npi", C.c_int64)]


class MtjStats(C.Structure):
    _fields_ = [("state_counts", C.c_void_p), ("beta_ss", C.c_void_p), ("alpha_ss", C.c_void_p), ("resid_cp", C.c_void_p), ("resid_sum", C.c_void_p),
                ("n_changed", C.c_double), ("step_ms", C.c_double)]


class GblupParams(C.Structure):
    _fields_ = [("iteration", C.c_uint32), ("diagonal", C.c_int32), ("seed", C.c_uint64), ("first_trait", C.c_uint32), ("reserved", C.c_uint32),
                ("vare", C.c_double * 16), ("G", C.c_double * 16)]


class GblupStats(C.Structure):
    _fields_ = [("alpha_ss", C.c_double * 16), ("resid_ss", C.c_double * 16), ("resid_sum", C.c_double * 4), ("step_ms", C.c_double)]


class MegaRParams(C.Structure):
    _fields_ = [("iteration", C.c_uint32), ("reserved", C.c_uint32), ("seed", C.c_uint64), ("vare", C.c_void_p), ("var_effect", C.c_void_p),
                ("gamma", C.c_void_p), ("pi", C.c_void_p)]


class MegaRStats(C.Structure):
    _fields_ = [("class_counts", C.c_void_p), ("ssq", C.c_void_p), ("nnz", C.c_void_p), ("alpha_ss", C.c_void_p), ("resid_ss", C.c_void_p),
                ("resid_sum", C.c_void_p), ("n_changed", C.c_void_p), ("step_ms", C.c_double)]


class JwasHipError(RuntimeError):
    """Raised for any non-zero status of the C ABI (the analogue of the reference's error(...))."""

    def __init__(self, code, message):
        super().__init__(f"libjwas_hip error {code}: {message}")
        self.code = code
        self.message = message


_vp, _i32, _i64, _u64, _f64p, _INT, _P = C.c_void_p, C.c_int32, C.c_int64, C.c_uint64, C.POINTER(C.c_double), C.c_int, C.POINTER

# every entry point include/jwas_hip.h declares: name -> (restype, argtypes).  SYMBOLS and load()'s declarations derive from it
# (tests/test_abi.py checks the names against the header and the library's exports).
PROTOTYPES = {
    "jwas_hip_create": (_INT, [C.c_int, _P(_vp)]),
    "jwas_hip_destroy": (None, [_vp]),
    "jwas_hip_last_error": (C.c_char_p, [_vp]),
    "jwas_hip_set_stream": (_INT, [_vp, _vp]),
    "jwas_hip_device_info": (_INT, [_vp, _P(C.c_int), _P(_i64), _P(_i64)]),
    "jwas_hip_load_dense_f32": (_INT, [_vp, _vp, _i64, _i64, _i64]),
    "jwas_hip_alloc_dense_f32": (_INT, [_vp, _i64, _i64]),
    "jwas_hip_dense_layout": (_INT, [_vp, _P(_i64), _P(_i64), _P(_i64), _P(_vp)]),
    "jwas_hip_get_columns": (_INT, [_vp, _i64, _i64, _vp]),
    "jwas_hip_estimate_bytes": (_i64, [_i64, _i64, _i32, _i32]),
    "jwas_hip_synth_genotypes": (_INT, [_vp, _u64, _i32, _i32, _i64]),
    "jwas_hip_setup_blocks": (_INT, [_vp, _i32, _i32]),
    "jwas_hip_get_xpx": (_INT, [_vp, _vp]),
    "jwas_hip_get_gram": (_INT, [_vp, _i64, _vp]),
    "jwas_hip_set_gram": (_INT, [_vp, _i64, _vp]),
    "jwas_hip_num_blocks": (_INT, [_vp, _P(_i64), _P(_i32)]),
    "jwas_hip_init_state": (_INT, [_vp, _i32, _i32]),
    "jwas_hip_set_state": (_INT, [_vp, _i32, _vp, _vp, _vp]),
    "jwas_hip_get_state": (_INT, [_vp, _i32, _vp, _vp, _vp]),
    "jwas_hip_set_residual": (_INT, [_vp, _i32, _vp]),
    "jwas_hip_get_residual": (_INT, [_vp, _i32, _vp]),
    "jwas_hip_residual_dev": (_INT, [_vp, _P(_vp), _P(_i64)]),
    "jwas_hip_residual_to_dev": (_INT, [_vp, _i32, _vp]),
    "jwas_hip_residual_from_dev": (_INT, [_vp, _i32, _vp]),
    "jwas_hip_residual_handover": (_INT, [_vp, _vp]),
    "jwas_hip_residual_sub_xalpha": (_INT, [_vp, _i32]),
    "jwas_hip_mul_alpha": (_INT, [_vp, _i32, _vp]),
    "jwas_hip_load_output_dense_f32": (_INT, [_vp, _vp, _i64, _i64, _i64]),
    "jwas_hip_mul_alpha_output": (_INT, [_vp, _i32, _vp]),
    "jwas_hip_window_sums": (_INT, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "jwas_hip_window_sums2": (_INT, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "jwas_hip_set_kernel_timing": (_INT, [_vp, _i32]),
    "jwas_hip_sweep": (_INT, [_vp, _P(SweepParams), _P(SweepStats)]),
    "jwas_hip_last_sweep_counters": (_INT, [_vp, _P(_u64), _i32]),
    "jwas_hip_last_sweep_schedule": (_INT, [_vp, _P(C.c_uint32)]),
    "jwas_hip_accumulate": (_INT, [_vp, C.c_double]),
    "jwas_hip_get_posterior": (_INT, [_vp, _i32, _vp, _vp, _vp]),
    "jwas_hip_load_jgb2": (_INT, [_vp, C.c_char_p]),
    "jwas_hip_load_packed2bit": (_INT, [_vp, _vp, _i64, _i64, _i64, _vp, _i32]),
    "jwas_hip_alloc_packed2bit": (_INT, [_vp, _i64, _i64, _i32]),
    "jwas_hip_plink_scan": (_INT, [_vp, C.c_char_p, _i64, _i64, _vp, _i64, _i32, _vp]),
    "jwas_hip_plink_commit": (_INT, [_vp, _vp, _i64, _vp, _i32]),
    "jwas_hip_plink_discard": (_INT, [_vp]),
    "jwas_hip_get_packed2bit": (_INT, [_vp, _i64, _i64, _vp, _i64]),
    "jwas_hip_load_output_packed2bit": (_INT, [_vp, _vp, _i64, _i64, _i64]),
    "jwas_hip_plink_commit_output": (_INT, [_vp, _vp, _i64]),
    "jwas_hip_get_output_packed2bit": (_INT, [_vp, _i64, _i64, _vp, _i64]),
    "jwas_hip_ebv_output": (_INT, [_vp, _vp]),
    "jwas_hip_storage_info": (_INT, [_vp, _P(_i32), _P(_i64), _P(_i64), _P(_i64)]),
    "jwas_hip_set_xpx": (_INT, [_vp, _vp]),
    "jwas_hip_estimate_bytes_storage": (_i64, [_i64, _i64, _i32, _i32, _i32]),
    "jwas_hip_add_block_size": (_INT, [_vp, _i32, _i32]),
    "jwas_hip_select_block_size": (_INT, [_vp, _i32]),
    "jwas_hip_set_weights": (_INT, [_vp, _vp]),
    "jwas_hip_set_weights_f64": (_INT, [_vp, _vp]),
    "jwas_hip_synth_single_step": (_INT, [_vp, _u64, _i64, _i32, _i64]),
    "jwas_hip_setup_blocks_explicit": (_INT, [_vp, _P(_i64), _i64, _i32]),
    "jwas_hip_comm_row_shards": (_INT, [_vp, _i32]),
    "jwas_hip_comm_init_loopback": (_INT, [_vp, _i32, _i32, _i32]),
    "jwas_hip_update_geometry": (_INT, [_vp, _P(_i32), _P(_i32), _P(_i32)]),
    "jwas_hip_set_cross_gram": (_INT, [_vp, _i64, _vp]),
    "jwas_hip_get_cross_gram": (_INT, [_vp, _i32, _i64, _vp]),
    "jwas_hip_set_columns": (_INT, [_vp, _i64, _i64, _vp, _i64]),
    "jwas_hip_get_alpha_sparse": (_INT, [_vp, _i32, _i64, _vp, _vp, _P(_i64)]),
    "jwas_hip_comm_unique_id": (_INT, [_vp]),
    "jwas_hip_comm_init": (_INT, [_vp, _vp, _i32, _i32]),
    "jwas_hip_comm_destroy": (_INT, [_vp]),
    "jwas_hip_sweep_sharded": (_INT, [_vp, _P(SweepParams), _P(SweepStats)]),
    "jwas_hip_residual_add_scalar": (_INT, [_vp, _i32, C.c_double]),
    "jwas_hip_comm_info": (_INT, [_vp, _P(_i32), _P(_i32)]),
    "jwas_hip_sample_marker_covariances": (_INT, [_vp, C.c_double, _f64p, _u64, C.c_uint32, C.c_uint32]),
    "jwas_hip_get_marker_covariances": (_INT, [_vp, _vp]),
    "jwas_hip_set_precision": (_INT, [_vp, _i32]),
    "jwas_hip_load_dense_f64": (_INT, [_vp, _vp, _i64, _i64, _i64]),
    "jwas_hip_get_xpx_f64": (_INT, [_vp, _vp]),
    "jwas_hip_set_state_f64": (_INT, [_vp, _i32, _vp, _vp, _vp]),
    "jwas_hip_get_state_f64": (_INT, [_vp, _i32, _vp, _vp, _vp]),
    "jwas_hip_set_residual_f64": (_INT, [_vp, _i32, _vp]),
    "jwas_hip_get_residual_f64": (_INT, [_vp, _i32, _vp]),
    "jwas_hip_mul_alpha_f64": (_INT, [_vp, _i32, _vp]),
    "jwas_hip_get_posterior_f64": (_INT, [_vp, _i32, _vp, _vp, _vp]),
    "jwas_hip_setup_groups": (_INT, [_vp, _i32, _i32]),
    "jwas_hip_set_marker_covariances_f64": (_INT, [_vp, _vp]),
    "jwas_hip_get_marker_covariances_f64": (_INT, [_vp, _vp]),
    "jwas_hip_load_output_dense_f64": (_INT, [_vp, _vp, _i64, _i64, _i64]),
    "jwas_hip_mul_alpha_output_f64": (_INT, [_vp, _i32, _vp]),
    "jwas_hip_get_alpha_sparse_f64": (_INT, [_vp, _i32, _i64, _vp, _vp, _P(_i64)]),
    "jwas_hip_window_sums_f64": (_INT, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "jwas_hip_window_sums2_f64": (_INT, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "jwas_hip_gwas_begin": (_INT, [_vp, _i32, _i32, _vp, _vp, _i32]),
    "jwas_hip_gwas_sample": (_INT, [_vp, _i32, _vp, _vp, _vp, _vp]),
    "jwas_hip_gwas_sample_f64": (_INT, [_vp, _i32, _vp, _vp, _vp, _vp]),
    "jwas_hip_gwas_local_ebv": (_INT, [_vp, _vp, _P(_i64)]),
    "jwas_hip_gwas_geometry": (_INT, [_vp, _P(_i32), _P(_i32), _P(_i32)]),
    "jwas_hip_gwas_end": (_INT, [_vp]),
    "jwas_hip_gwas_estimate_bytes": (_i64, [_i64, _i64, _i64, _i32]),
    "jwas_hip_liability_begin": (_INT, [_vp, _i32]),
    "jwas_hip_liability_set_categorical": (_INT, [_vp, _i32, _i64, _vp, _i32, _vp]),
    "jwas_hip_liability_set_censored": (_INT, [_vp, _i32, _i64, _vp, _vp]),
    "jwas_hip_liability_set_thresholds": (_INT, [_vp, _i32, _i32, _vp]),
    "jwas_hip_liability_init": (_INT, [_vp, _P(LiabilityParams)]),
    "jwas_hip_liability_sample": (_INT, [_vp, _P(LiabilityParams)]),
    "jwas_hip_liability_minmax": (_INT, [_vp, _i32, _vp, _vp]),
    "jwas_hip_get_liabilities": (_INT, [_vp, _i32, _vp]),
    "jwas_hip_liability_end": (_INT, [_vp]),
    "jwas_hip_locpar_begin": (_INT, [_vp, _i32]),
    "jwas_hip_locpar_add_covariate": (_INT, [_vp, _i32, _i64, _vp]),
    "jwas_hip_locpar_add_factor": (_INT, [_vp, _i32, _i64, _vp, _i64, _i32]),
    "jwas_hip_locpar_size": (_INT, [_vp, _P(_i64)]),
    "jwas_hip_locpar_set_sol": (_INT, [_vp, _i64, _vp]),
    "jwas_hip_locpar_get_sol": (_INT, [_vp, _i64, _vp]),
    "jwas_hip_locpar_step": (_INT, [_vp, _P(LocparParams), _P(LocparStats)]),
    "jwas_hip_locpar_accumulate": (_INT, [_vp, C.c_double]),
    "jwas_hip_locpar_get_means": (_INT, [_vp, _i64, _vp, _vp]),
    "jwas_hip_locpar_estimate_bytes": (_i64, [_i64, _i64, _i64]),
    "jwas_hip_locpar_end": (_INT, [_vp]),
    "jwas_hip_lp_set_group_structure": (_INT, [_vp, _i32, _i64, _vp, _vp, _vp]),
    "jwas_hip_lp_get_group_colors": (_INT, [_vp, _i32, _i64, _vp, _P(_i32)]),
    "jwas_hip_lp_structure_estimate_bytes": (_i64, [_i64, _i64]),
    "jwas_hip_mtmiss_begin": (_INT, [_vp, _i64, _vp]),
    "jwas_hip_mtmiss_impute": (_INT, [_vp, _P(MtmissParams)]),
    "jwas_hip_mtmiss_set_record_weights": (_INT, [_vp, _vp]),
    "jwas_hip_mtmiss_estimate_bytes": (_i64, [_i64]),
    "jwas_hip_mtmiss_end": (_INT, [_vp]),
    "jwas_hip_annot_begin": (_INT, [_vp, _i32, _i64, _i32, _vp, _vp, _vp, _vp]),
    "jwas_hip_annot_step": (_INT, [_vp, _P(AnnotParams), _P(AnnotStats)]),
    "jwas_hip_annot_accumulate": (_INT, [_vp, C.c_double]),
    "jwas_hip_annot_get_prior": (_INT, [_vp, _i64, _vp]),
    "jwas_hip_annot_get_means": (_INT, [_vp, _i64, _vp, _vp]),
    "jwas_hip_annot_get_liability": (_INT, [_vp, _i64, _vp]),
    "jwas_hip_annot_get_mu": (_INT, [_vp, _i64, _vp]),
    "jwas_hip_annot_estimate_bytes": (_i64, [_i64, _i32, _i32]),
    "jwas_hip_annot_end": (_INT, [_vp]),
    "jwas_hip_sem_begin": (_INT, [_vp, _i32, _i64, _vp, _vp]),
    "jwas_hip_sem_step": (_INT, [_vp, _P(SemParams), _P(SemStats)]),
    "jwas_hip_sem_get_lambda": (_INT, [_vp, _vp]),
    "jwas_hip_sem_set_lambda": (_INT, [_vp, _vp]),
    "jwas_hip_sem_get_gram": (_INT, [_vp, _vp]),
    "jwas_hip_sem_accumulate": (_INT, [_vp, _vp, C.c_double]),
    "jwas_hip_sem_get_effects": (_INT, [_vp, _i32, _i32, _vp, _vp, _vp]),
    "jwas_hip_sem_estimate_bytes": (_i64, [_i64, _i64, _i32]),
    "jwas_hip_sem_end": (_INT, [_vp]),
    "jwas_hip_rrm_begin": (_INT, [_vp, _i32, _i32, _i64, _vp, _vp, _i32]),
    "jwas_hip_rrm_set_residual": (_INT, [_vp, _i64, _vp]),
    "jwas_hip_rrm_get_residual": (_INT, [_vp, _i64, _vp]),
    "jwas_hip_rrm_set_state": (_INT, [_vp, _vp, _vp, _vp]),
    "jwas_hip_rrm_get_state": (_INT, [_vp, _vp, _vp, _vp]),
    "jwas_hip_rrm_sweep": (_INT, [_vp, _P(RrmParams), _P(RrmStats)]),
    "jwas_hip_rrm_accumulate": (_INT, [_vp, C.c_double]),
    "jwas_hip_rrm_get_posterior": (_INT, [_vp, _i32, _vp, _vp, _vp]),
    "jwas_hip_rrm_mul_alpha": (_INT, [_vp, _i32, _vp]),
    "jwas_hip_rrm_get_m": (_INT, [_vp, _i64, _vp]),
    "jwas_hip_rrm_get_gram": (_INT, [_vp, _i64, _i64, _vp]),
    "jwas_hip_rrm_estimate_bytes": (_i64, [_i64, _i64, _i32, _i32, _i32]),
    "jwas_hip_rrm_end": (_INT, [_vp]),
    "jwas_hip_mega_begin": (_INT, [_vp, _i32, _i32, _i32]),
    "jwas_hip_mega_set_missing": (_INT, [_vp, _i64, _vp]),
    "jwas_hip_mega_set_residual": (_INT, [_vp, _i32, _vp]),
    "jwas_hip_mega_get_residual": (_INT, [_vp, _i32, _vp]),
    "jwas_hip_mega_set_state": (_INT, [_vp, _i32, _vp, _vp, _vp]),
    "jwas_hip_mega_get_state": (_INT, [_vp, _i32, _vp, _vp, _vp]),
    "jwas_hip_mega_impute": (_INT, [_vp, _P(MegaParams)]),
    "jwas_hip_mega_sweep": (_INT, [_vp, _P(MegaParams), _P(MegaStats)]),
    "jwas_hip_mega_accumulate": (_INT, [_vp, C.c_double]),
    "jwas_hip_mega_sweep_r": (_INT, [_vp, _P(MegaRParams), _P(MegaRStats)]),
    "jwas_hip_mega_accumulate_r": (_INT, [_vp, C.c_double]),
    "jwas_hip_mega_psrf": (_INT, [_vp, C.c_double, _vp]),
    "jwas_hip_mega_get_posterior": (_INT, [_vp, _i32, _vp, _vp, _vp]),
    "jwas_hip_mega_mul_alpha": (_INT, [_vp, _i32, _i32, _vp]),
    "jwas_hip_mega_get_gram": (_INT, [_vp, _i64, _i64, _vp, _vp]),
    "jwas_hip_mega_estimate_bytes": (_i64, [_i64, _i64, _i32, _i32]),
    "jwas_hip_mega_end": (_INT, [_vp]),
    "jwas_hip_mtj_begin": (_INT, [_vp, _i32, _i32]),
    "jwas_hip_mtj_set_residual": (_INT, [_vp, _i32, _vp]),
    "jwas_hip_mtj_get_residual": (_INT, [_vp, _i32, _vp]),
    "jwas_hip_mtj_set_state": (_INT, [_vp, _i32, _vp, _vp, _vp]),
    "jwas_hip_mtj_get_state": (_INT, [_vp, _i32, _vp, _vp, _vp]),
    "jwas_hip_mtj_gram": (_INT, [_vp, _i64, _i64, _vp, _vp]),
    "jwas_hip_mtj_sweep": (_INT, [_vp, _P(MtjParams), _P(MtjStats)]),
    "jwas_hip_mtj_accumulate": (_INT, [_vp, C.c_double]),
    "jwas_hip_mtj_posterior": (_INT, [_vp, _i32, _vp, _vp, _vp]),
    "jwas_hip_mtj_mul_alpha": (_INT, [_vp, _i32, _i32, _vp]),
    "jwas_hip_mtj_end": (_INT, [_vp]),
    "jwas_hip_grm": (_INT, [_vp, _vp, _vp]),
    "jwas_hip_grm_packed2bit": (_INT, [_vp, _vp, _vp]),
    "jwas_hip_grm_estimate_bytes": (_i64, [_i64, _i64, _i32]),
    "jwas_hip_gblup_begin": (_INT, [_vp, _vp]),
    "jwas_hip_gblup_step": (_INT, [_vp, _P(GblupParams), _P(GblupStats)]),
    "jwas_hip_gblup_get_rhs": (_INT, [_vp, _i64, _vp]),
    "jwas_hip_gblup_estimate_bytes": (_i64, [_i64, _i32, _i32]),
    "jwas_hip_gblup_end": (_INT, [_vp]),
    "jwas_hip_ss_begin": (_INT, [_vp, _i64, _i64, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i64, _P(_i64)]),
    "jwas_hip_ss_set_rows": (_INT, [_vp, _i32, _i64, _vp]),
    "jwas_hip_ss_impute": (_INT, [_vp, _i64, _i64, _vp, _i64]),
    "jwas_hip_ss_get_columns": (_INT, [_vp, _i32, _i64, _i64, _i64, _vp]),
    "jwas_hip_ss_solve_host": (_INT, [_vp, _i64, _vp, _i64, _i64, _vp, _vp]),
    "jwas_hip_ss_estimate_bytes": (_i64, [_i64, _i64, _i64, _i64, _i64, _i64]),
    "jwas_hip_ss_end": (_INT, [_vp]),
}
SYMBOLS = list(PROTOTYPES)

_lib = None


def load():
    """Load libjwas_hip.so and declare prototypes.  Fails loudly if the HIP library is absent."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError(
            f"{LIB_PATH} not found: build it with jwas.jl_amd/csrc/build.sh (hipcc, gfx950). "
            "The MI355X path has no CPU fallback.")
    L = C.CDLL(LIB_PATH)
    for name, (restype, argtypes) in PROTOTYPES.items():
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L
