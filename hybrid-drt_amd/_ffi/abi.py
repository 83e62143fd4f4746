"""The ctypes mirror of include/hipdrt.h and include/hipdrt_debug.h: constants, structures, the SIGNATURES table, and
load_library, which attaches it to libhipdrt.so."""
from __future__ import annotations

import ctypes as C
import os
import sys
import threading

import numpy as np

_HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))      # the package's directory: the library lies beside its __init__.py
LIB_PATH = os.environ.get("HIPDRT_LIB", os.path.join(_HERE, "libhipdrt.so"))

MODE_INTERP, MODE_TRAPZ = 0, 1
RESPONSE_POT, RESPONSE_EXPDECAY = 0, 1
QP_OPTIMAL, QP_MAXITER, QP_SINGULAR_LATE, QP_SINGULAR, QP_ABORTED = 0, 1, 2, -1, -2
PREDICT_NOT_PD = -3          # HIPDRT_PREDICT_NOT_PD: the band of a spectrum whose P is not positive definite


class HipDrtError(RuntimeError):
    pass


class QpOpts(C.Structure):
    _fields_ = [("abstol", C.c_double), ("reltol", C.c_double), ("feastol", C.c_double), ("maxiters", C.c_int)]


class FitOpts(C.Structure):
    _fields_ = [
        ("rp_scale", C.c_double), ("derivative_weights", C.c_double * 3), ("sigma_ds", C.c_double * 3),
        ("l1_lambda_0", C.c_double), ("l2_lambda_0", C.c_double), ("s_alpha", C.c_double * 3),
        ("s_0", C.c_double * 3), ("rho_alpha", C.c_double * 3), ("rho_0", C.c_double * 3),
        ("iw_l1_lambda_0", C.c_double), ("iw_l2_lambda_0", C.c_double),
        ("ohmic_penalty", C.c_double), ("inductance_penalty", C.c_double), ("inductance_scale", C.c_double),
        ("eis_vmm_epsilon", C.c_double), ("eis_reim_cor", C.c_double), ("xtol", C.c_double),
        ("max_iter", C.c_int), ("nonneg", C.c_int), ("scale_data", C.c_int), ("fit_ohmic", C.c_int),
        ("fit_inductance", C.c_int), ("eis_error_uniform", C.c_int), ("update_scale", C.c_int),
        ("eff_hp", C.c_int),
        ("outlier_p", C.c_double), ("iw_alpha", C.c_double), ("iw_beta", C.c_double), ("qp", QpOpts),
    ]


class PreparedDesc(C.Structure):
    """hipdrt_prepared_desc (include/hipdrt.h)"""
    _fields_ = [
        ("m", C.c_int), ("n", C.c_int), ("ns", C.c_int), ("dop_start", C.c_int), ("dop_size", C.c_int),
        ("vz_index", C.c_int), ("vb_start", C.c_int), ("vb_size", C.c_int), ("num_chrono", C.c_int),
        ("toeplitz_m", C.c_int), ("chrono_vmm_uniform", C.c_int), ("basis_area", C.c_double), ("init_weights_separately", C.c_int),
        ("weight_method", C.c_int), ("fixed_chrono_factor", C.c_double), ("fixed_eis_factor", C.c_double),
        ("dop_l2_lambda_0", C.c_double),
        ("dop_derivative_weights", C.c_double * 3),
        ("dop_s_alpha", C.c_double * 3), ("dop_rho_alpha", C.c_double * 3), ("dop_s_0", C.c_double * 3),
        ("dop_rho_0", C.c_double * 3),
    ]


_dp = C.POINTER(C.c_double)
_ip = C.POINTER(C.c_int)
_vp = C.c_void_p


class IterateState(C.Structure):
    """hipdrt_iterate_state (include/hipdrt.h): the arrays iterate_qphb takes; NULL keeps the device value"""
    _fields_ = [(name, C.POINTER(C.c_double)) for name in
                ("x_in", "s_vectors", "rho", "dop_rho", "weights", "est_weights", "xmx_norms", "dop_xmx_norms")]


class KkOpts(C.Structure):
    """hipdrt_kk_opts (include/hipdrt.h)"""
    _fields_ = [("n_outlier_iter", C.c_int), ("p_thresh", C.c_double), ("n_sigma", C.c_double),
                ("std_sample_fraction", C.c_double), ("n_std", C.c_double), ("max_num_outliers", C.c_int),
                ("outlier_weight", C.c_double)]


class PeakOpts(C.Structure):
    """hipdrt_peak_opts (include/hipdrt.h)"""
    _fields_ = [("eval_sign", C.c_int), ("search", C.c_int), ("normalize", C.c_int), ("method", C.c_int),
                ("height", C.c_double), ("prominence", C.c_double), ("prob_thresh", C.c_double), ("num_peaks", C.c_int),
                ("fxx_var_floor", C.c_double), ("ext_left", C.c_int), ("ext_right", C.c_int)]


class PeakProbOpts(C.Structure):
    """hipdrt_peak_prob_opts (include/hipdrt.h)"""
    _fields_ = [("bayes_cov", C.c_int), ("std_size", C.c_int), ("std_baseline", C.c_double), ("sigma_floor", C.c_int),
                ("ext_left", C.c_int), ("ext_right", C.c_int), ("search", C.c_int), ("height", C.c_double),
                ("prominence", C.c_double)]


class PfrtOpts(C.Structure):
    """hipdrt_pfrt_opts (include/hipdrt.h)"""
    _fields_ = [("eval_sign", C.c_int), ("search", C.c_int), ("height", C.c_double), ("prominence", C.c_double),
                ("prior_mu", C.c_double), ("prior_sigma", C.c_double), ("n_eff_factor", C.c_double), ("fxx_var_floor", C.c_double),
                ("ext_left", C.c_int), ("ext_right", C.c_int), ("smooth", C.c_int), ("smooth_order", C.c_double),
                ("smooth_epsilon", C.c_double), ("integrate", C.c_int), ("integrate_threshold", C.c_double), ("normalize", C.c_int)]


class PfrtSelectOpts(C.Structure):
    """hipdrt_pfrt_select_opts (include/hipdrt.h)"""
    _fields_ = [("start_thresh", C.c_double), ("end_thresh", C.c_double), ("peak_thresh", C.c_double), ("max_peaks", C.c_int),
                ("ln_tau_out", _dp), ("neval_out", C.c_int)]


class PeakResolveOpts(C.Structure):
    """hipdrt_peak_resolve_opts (include/hipdrt.h)"""
    _fields_ = [("sign", C.c_int), ("max_peaks", C.c_int), ("epsilon_factor", C.c_double), ("max_epsilon", C.c_double),
                ("min_epsilon", C.c_double), ("epsilon_uniform", C.c_double)]


class PeakResolveIn(C.Structure):
    """hipdrt_peak_resolve_in (include/hipdrt.h)"""
    _fields_ = [("source", C.c_int), ("peak_opts", C.POINTER(PeakOpts)), ("peak_indices", _ip), ("win_start", _ip), ("win_end", _ip),
                ("nwin", C.c_int), ("ln_tau_find", _dp), ("nfind", C.c_int), ("ln_tau_out", _dp), ("nout", C.c_int),
                ("row_scale", _dp)]


class PeakResolveOut(C.Structure):
    """hipdrt_peak_resolve_out (include/hipdrt.h)"""
    _fields_ = [("count", _ip), ("peak_index", _ip), ("trough_index", _ip), ("eps_l", _dp), ("eps_r", _dp), ("r_peaks", _dp),
                ("r_coef", _dp), ("x_peaks", _dp), ("peak_gammas", _dp), ("status", _ip)]


class CandidatesIn(C.Structure):
    """hipdrt_candidates_in (include/hipdrt.h)"""
    _fields_ = [("source", C.c_int), ("C", C.c_int), ("x", _dp), ("ncand", _ip), ("ln_tau_find", _dp), ("nfind", C.c_int),
                ("peak_opts", C.POINTER(PeakOpts)), ("max_peaks", C.c_int)]


class CandidatesOut(C.Structure):
    """hipdrt_candidates_out (include/hipdrt.h)"""
    _fields_ = [("rss", _dp), ("sum_log_w", _dp), ("count", _ip), ("peak_index", _ip), ("heights", _dp), ("prominences", _dp),
                ("status", _ip)]


class PfrtSelectOut(C.Structure):
    """hipdrt_pfrt_select_out (include/hipdrt.h)"""
    _fields_ = [("num_peaks", _ip), ("ranked_index", _ip), ("first", _ip), ("num_candidates", _ip), ("step_index", _ip),
                ("magnitude", _dp), ("match_quality", _dp), ("raw_pfrt", _dp), ("step_pfrt", _dp), ("post_prob", _dp),
                ("pfrt", _dp)]


class LmlIn(C.Structure):
    """hipdrt_lml_in (include/hipdrt.h)"""
    _fields_ = [("step", C.c_int), ("x", _dp), ("rho", _dp), ("s", _dp), ("dop_rho", _dp), ("weights", _dp),
                ("override_hypers", C.c_int), ("l2_lambda_0", C.c_double), ("derivative_weights", C.c_double * 3),
                ("dop_l2_lambda_0", C.c_double), ("dop_derivative_weights", C.c_double * 3)]


class LmlOut(C.Structure):
    """hipdrt_lml_out (include/hipdrt.h)"""
    _fields_ = [("logdet_p", _dp), ("logdet_prior", _dp), ("wy2", _dp), ("fit2", _dp), ("cross", _dp), ("slw", _dp), ("xox", _dp),
                ("l1x", _dp), ("status", _ip)]


class ResolveArgs(C.Structure):
    """hipdrt_resolve_args (include/hipdrt.h)"""
    _fields_ = [("nb", C.c_int), ("nr", C.c_int), ("num_remove", C.c_int), ("so", C.c_int), ("lambda_psi", C.c_double),
                ("tau_filter_sigma", C.c_double), ("special_filter_sigma", C.c_double), ("first", _ip), ("match", _ip),
                ("tau_indices", _ip), ("my", _dp), ("param_scale", _dp), ("x_remove", _dp), ("h", _dp)]


LML_TERMS = ("logdet_p", "logdet_prior", "wy2", "fit2", "cross", "slw", "xox", "l1x")


class DebugPeakResolveArgs(C.Structure):
    """hipdrt_debug_peak_resolve_args (include/hipdrt_debug.h)"""
    _fields_ = [("B", C.c_int), ("nfind", C.c_int), ("nb", C.c_int), ("nout", C.c_int), ("copies", C.c_int), ("source", C.c_int),
                ("nwin", C.c_int), ("f", _dp), ("fxx", _dp), ("keep", _ip), ("indices", _ip), ("win_start", _ip), ("win_end", _ip),
                ("x", _dp), ("ln_tau_find", _dp), ("ln_basis", _dp), ("ln_tau_out", _dp), ("basis_eps", C.c_double),
                ("fit_status", _ip), ("opts", C.POINTER(PeakResolveOpts)), ("out", PeakResolveOut),
                ("lds_bytes", C.POINTER(C.c_longlong))]


class DebugGramArgs(C.Structure):
    """hipdrt_debug_gram_args (include/hipdrt_debug.h)"""
    _fields_ = [
        ("B", C.c_int), ("m", C.c_int), ("n", C.c_int), ("A", _dp), ("a_batched", C.c_int), ("lda", C.c_int),
        ("w", _dp), ("y", _dp), ("l1", _dp), ("l1_scalar", C.c_double),
        ("l2", _dp), ("l2_batched", C.c_int), ("ldl2", C.c_int),
        ("mk", _dp * 3), ("ldm", C.c_int), ("s", _dp), ("rho", _dp), ("dfac", C.c_double * 3),
        ("ns", C.c_int), ("sym", C.c_int), ("toep", C.c_int), ("toep_maxd", C.c_int), ("spec_zero", C.c_int),
        ("dop_start", C.c_int), ("dop_size", C.c_int), ("dop_rho", _dp), ("dop_dfac", C.c_double * 3),
        ("active", _ip), ("P", _dp), ("ldp", C.c_int), ("Ppk", _dp), ("q", _dp),
    ]


class DebugHyperArgs(C.Structure):
    """hipdrt_debug_hyper_args (include/hipdrt_debug.h)"""
    _fields_ = [
        ("B", C.c_int), ("m", C.c_int), ("n", C.c_int), ("ns", C.c_int), ("ldrm", C.c_int), ("ldm", C.c_int),
        ("rm", _dp), ("rm_batched", C.c_int), ("vmm", _dp), ("mk", _dp * 3), ("toeplitz", C.c_int), ("toep_reach", C.c_int),
        ("x", _dp), ("x_in", _dp), ("s", _dp), ("rho", _dp), ("xmx", _dp), ("rv", _dp), ("est_w", _dp), ("w", _dp),
        ("var_floor", _dp), ("coef_scale", _dp), ("qp_status", _ip), ("active", _ip), ("fit_status", _ip), ("outer_iters", _ip),
        ("n_active", _ip), ("outlier_t", _dp), ("opts", C.POINTER(FitOpts)), ("it", C.c_int), ("continue_mode", C.c_int),
        ("min_iter", C.c_int), ("basis_area", C.c_double), ("desc", C.POINTER(PreparedDesc)), ("dop_rho", _dp), ("dop_xmx", _dp),
        ("vz_strength", _dp), ("vz_entry", _dp), ("rm_col", _dp), ("products", C.c_int),
    ]


class DebugSetupArgs(C.Structure):
    """hipdrt_debug_setup_args (include/hipdrt_debug.h)"""
    _fields_ = [
        ("B", C.c_int), ("nf", C.c_int), ("m", C.c_int), ("n", C.c_int), ("ldrm", C.c_int), ("opts", C.POINTER(FitOpts)),
        ("desc", C.POINTER(PreparedDesc)), ("z_re", _dp), ("z_im", _dp), ("rm", _dp), ("rm_batched", C.c_int), ("vmm", _dp),
        ("vmm_iw", _dp), ("qp_status", _ip), ("rv", _dp), ("w", _dp), ("est_w", _dp), ("x", _dp), ("x_in", _dp), ("s", _dp),
        ("rho", _dp), ("xmx", _dp), ("dop_rho", _dp), ("dop_xmx", _dp), ("coef_scale", _dp), ("var_floor", _dp), ("active", _ip),
        ("outer_iters", _ip), ("fit_status", _ip), ("qp_iters_total", _ip), ("outlier_t", _dp), ("stage", C.c_int), ("r0", C.c_int),
        ("r1", C.c_int), ("row_mask", C.c_int), ("fixed_chrono", C.c_double), ("fixed_eis", C.c_double), ("wrow", _dp), ("wfac", _dp),
        ("stored", C.c_int), ("scalar_w", C.c_double), ("rss", _dp), ("slw", _dp), ("w_out", _dp),
    ]


class DebugRowopArgs(C.Structure):
    """hipdrt_debug_rowop_args (include/hipdrt_debug.h)"""
    _fields_ = [(k, C.c_int) for k in ("op", "B", "m", "n", "ns", "nf", "ld", "col", "idx_rinf", "idx_induc", "nonneg", "batched")] + [
        ("factor", C.c_double), ("pen_r", C.c_double), ("pen_l", C.c_double), ("in0", _dp), ("in1", _dp), ("in2", _dp),
        ("active", _ip), ("out0", _dp), ("out1", _dp), ("out2", _dp)]


class DebugPosteriorArgs(C.Structure):
    """hipdrt_debug_posterior_args (include/hipdrt_debug.h)"""
    _fields_ = [("B", C.c_int), ("n", C.c_int), ("P", _dp), ("p_batched", C.c_int), ("ldp", C.c_int), ("rows", _dp),
                ("neval", C.c_int), ("ncol", C.c_int), ("col_offset", C.c_int), ("scale", _dp), ("cov_member", C.c_int),
                ("var", _dp), ("status", _ip), ("cov", _dp), ("bex", _dp), ("tail", _dp)]


class DebugDopPosteriorArgs(C.Structure):
    """hipdrt_debug_dop_posterior_args (include/hipdrt_debug.h)"""
    _fields_ = [("post", DebugPosteriorArgs), ("dop_start", C.c_int), ("dop_size", C.c_int), ("dop_scale_vector", _dp),
                ("dop_scale_batched", C.c_int), ("ppk", _dp)]


class DebugQpArgs(C.Structure):
    """hipdrt_debug_qp_args (include/hipdrt_debug.h)"""
    _fields_ = [("B", C.c_int), ("n", C.c_int), ("P", _dp), ("p_batched", C.c_int), ("ldp", C.c_int), ("q", _dp), ("h", _dp),
                ("h_batched", C.c_int), ("opts", C.POINTER(QpOpts)), ("active", _ip), ("order", _ip), ("use_lpt", C.c_int),
                ("form", _ip), ("x", _dp), ("iters", _ip), ("pcost", _dp), ("status", _ip), ("iters_accum", _ip),
                ("s", _dp), ("z", _dp), ("order_out", _ip)]


class PredictDesc(C.Structure):
    """hipdrt_predict_desc (include/hipdrt.h)"""
    _fields_ = [("idx_rinf", C.c_int), ("idx_induc", C.c_int), ("idx_cinv", C.c_int), ("inductance_scale", C.c_double),
                ("capacitance_scale", C.c_double), ("dop_scale_vector", _dp), ("dop_scale_batched", C.c_int), ("v_baseline_scale", _dp),
                ("coefficient_scale", _dp), ("response_signal_scale", _dp), ("scaled_response_offset", _dp)]


class DopArgs(C.Structure):
    """hipdrt_dop_args (include/hipdrt.h)"""
    _fields_ = [("nu", _dp), ("nn", C.c_int), ("basis_nu", _dp), ("nu_epsilon", C.c_double), ("order", C.c_int),
                ("normalize_by", _dp), ("nu_basis_area", C.c_double), ("include_ideal", C.c_int), ("s_lo", C.c_double),
                ("s_hi", C.c_double)]


class ResponseArgs(C.Structure):
    """hipdrt_response_args (include/hipdrt.h)"""
    _fields_ = [("times", _dp), ("nt", C.c_int), ("step_times", _dp), ("nsteps", C.c_int), ("step_sizes", _dp),
                ("sizes_batched", C.c_int), ("basis_tau", _dp), ("mode", C.c_int), ("ny", C.c_int), ("ngrid", C.c_int),
                ("log_td", _dp), ("v", _dp), ("basis_nu", _dp), ("nu_epsilon", C.c_double), ("inf_rv", _dp),
                ("inf_batched", C.c_int), ("cap_rv", _dp), ("cap_batched", C.c_int), ("vz_strength", _dp), ("vb_mat", _dp),
                ("include_mask", C.c_int)]


class ZModelArgs(C.Structure):
    """hipdrt_z_model_args (include/hipdrt.h)"""
    _fields_ = [("freq", _dp), ("nf", C.c_int), ("basis_tau", _dp), ("mode", C.c_int), ("ny", C.c_int), ("ngrid", C.c_int),
                ("log_wt_re", _dp), ("z_re", _dp), ("log_wt_im", _dp), ("z_im", _dp), ("basis_nu", _dp), ("nu_epsilon", C.c_double),
                ("vz_strength", _dp), ("include_mask", C.c_int)]


class DebugResponseArgs(C.Structure):
    """hipdrt_debug_response_args (include/hipdrt_debug.h)"""
    _fields_ = [("B", C.c_int), ("S", C.c_int), ("nt", C.c_int), ("ntau", C.c_int), ("copies", C.c_int), ("ns", C.c_int),
                ("n", C.c_int), ("X", _dp), ("U", _dp), ("Ud", _dp), ("dop_start", C.c_int), ("dop_size", C.c_int),
                ("dop_scale_vector", _dp), ("step_sizes", _dp), ("sizes_batched", C.c_int), ("coefficient_scale", _dp), ("response_signal_scale", _dp),
                ("scaled_response_offset", _dp), ("idx_rinf", C.c_int), ("idx_cinv", C.c_int), ("vz_index", C.c_int),
                ("vb_start", C.c_int), ("vb_size", C.c_int), ("capacitance_scale", C.c_double), ("inf_rv", _dp),
                ("inf_batched", C.c_int), ("cap_rv", _dp), ("cap_batched", C.c_int), ("vz_strength", _dp), ("vb_mat", _dp),
                ("v_baseline_scale", _dp), ("fit_status", _ip), ("include_mask", C.c_int), ("out", _dp)]


class FilterTable(C.Structure):
    """hipdrt_filter_table (include/hipdrt.h): centre and right half of a symmetric table; radius < 0 skips the axis"""
    _fields_ = [("w", _dp), ("radius", C.c_int)]


MAP_FILTER_MAX_NODES = 16
MAP_FILTER, MAP_SIGMAS = 0, 1


class NodeTables(C.Structure):
    """hipdrt_node_tables (include/hipdrt.h)"""
    _fields_ = [("count", C.c_int), ("node", C.c_double * MAP_FILTER_MAX_NODES), ("node_delta", C.c_double), ("floor", C.c_double),
                ("radius", C.c_int * MAP_FILTER_MAX_NODES), ("w", _dp * MAP_FILTER_MAX_NODES)]


NODE_TABLE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_double, C.POINTER(NodeTables))


class MapFilterArgs(C.Structure):
    """hipdrt_map_filter_args (include/hipdrt.h)"""
    _fields_ = [("ndim", C.c_int), ("rows", C.c_int), ("cols", C.c_int), ("op", C.c_int), ("iterative", C.c_int),
                ("adaptive", C.c_int), ("mask_nans", C.c_int), ("empty", C.c_int), ("iter", C.c_int), ("nstd", C.c_double),
                ("box_size", C.c_int), ("init_weights", _dp), ("sigmas_in", _dp), ("gauss", FilterTable * 2), ("empty_gauss", FilterTable * 2),
                ("box", FilterTable * 2), ("pre_gauss", FilterTable * 2), ("pre_empty", FilterTable * 2), ("curv", FilterTable),
                ("k_factor", C.c_double * 2), ("max_sigma", C.c_double * 2), ("nodes", NODE_TABLE_FN), ("user", C.c_void_p)]


RANK_ONE, RANK_DIFF = 0, 1
Q_NANMEDIAN = -1.0
E_NUMERIC, E_UNSUPPORTED = -4, -5


class MapBadnessArgs(C.Structure):
    """hipdrt_map_badness_args (include/hipdrt.h)"""
    _fields_ = [("rows", C.c_int), ("cols", C.c_int), ("scale", C.c_int), ("flag_outliers", C.c_int), ("flag_size", C.c_int * 2),
                ("median_size", C.c_int * 2), ("std_size", C.c_int * 2), ("thresh", C.c_double), ("p_prior", C.c_double),
                ("full_std_contribution", C.c_double), ("n_std", C.c_double), ("impute", C.c_int), ("impute_gauss", FilterTable * 2), ("score", C.c_int),
                ("filt_in", _dp)]


class MapPredictArgs(C.Structure):
    """hipdrt_map_predict_args (include/hipdrt.h)"""
    _fields_ = [("rows", C.c_int), ("nsup", C.c_int), ("neval", C.c_int), ("ln_tau_sup", _dp), ("ln_tau_eval", _dp),
                ("epsilon", C.c_double), ("basis_area", C.c_double), ("normalize", C.c_int), ("x_filter", FilterTable * 2),
                ("f_var", _dp), ("fxx_var", _dp), ("var_stored", C.c_int), ("ext", _ip), ("search", C.c_int), ("height", C.c_double),
                ("prominence", C.c_double), ("spread", FilterTable), ("spread_factor", C.c_double)]


PEAKS_OVERFLOW, PEAKS_UNORDERED = -4, -5            # per-spectrum statuses of hipdrt_plan_resolve_peaks
PEAKS_FROM_FIND, PEAKS_FROM_INDICES, PEAKS_FROM_WINDOWS = 0, 1, 2
CANDIDATES_FROM_STEPS, CANDIDATES_FROM_HOST = 0, 1
CANDIDATE_ABSENT = -6                               # status of a slot at or past the spectrum's ncand (hipdrt_plan_score_candidates)
CANDIDATE_OUTPUTS = ("rss", "sum_log_w", "count", "peak_index", "heights", "prominences", "status")
PFRT_NO_PEAK, PFRT_TOO_MANY_PEAKS = 16, 17           # per-spectrum statuses of hipdrt_plan_pfrt_select
PFRT_SELECT_COMPACT = ("num_peaks", "ranked_index", "first", "num_candidates", "step_index", "magnitude", "match_quality")
PFRT_SELECT_ROWS = ("raw_pfrt", "step_pfrt", "post_prob", "pfrt")
RESOLVE_OUTPUTS = ("count", "peak_index", "trough_index", "eps_l", "eps_r", "r_peaks", "r_coef", "x_peaks", "peak_gammas", "status")

# include_mask bits of hipdrt_plan_predict_response and hipdrt_plan_predict_z_model (HIPDRT_INCLUDE_*)
INCLUDE_DRT, INCLUDE_OHMIC, INCLUDE_CAP, INCLUDE_DOP, INCLUDE_VZ_OFFSET, INCLUDE_BASELINE, INCLUDE_INDUCTANCE = 1, 2, 4, 8, 16, 32, 64
INCLUDE_ALL = 127


# name -> argtypes (all return int unless listed in _RESTYPES).  Mirrors include/hipdrt.h one-to-one;
# tests/test_cabi_symbols.py checks the header and this table against the built library.
SIGNATURES = {
    "hipdrt_create": [C.c_int, C.POINTER(_vp)],
    "hipdrt_destroy": [_vp],
    "hipdrt_last_error": [],
    "hipdrt_stream": [_vp],
    "hipdrt_synchronize": [_vp],
    "hipdrt_device_info": [_vp, C.c_char_p, C.c_int, _ip, C.POINTER(C.c_longlong)],
    "hipdrt_impedance_lookup": [_vp, C.c_double, C.c_int, C.c_int, _dp, _dp, _dp, _dp],
    "hipdrt_impedance_matrix": [_vp, C.c_int, C.c_int, _dp, C.c_int, _dp, C.c_int, C.c_int, C.c_int, C.c_double,
                                C.c_int, _dp, _dp, _dp, _dp, C.c_int, _dp, _dp],
    "hipdrt_impedance_matrix_dev": [_vp, C.c_int, C.c_int, _dp, C.c_int, _dp, C.c_int, C.c_int, C.c_int, C.c_double,
                                    C.c_int, _dp, _dp, _dp, _dp, C.c_int, _vp, _vp, C.c_int, C.POINTER(C.c_float)],
    "hipdrt_phasor_z_matrix": [_vp, _dp, C.c_int, _dp, C.c_int, C.c_double, _dp, _dp],
    "hipdrt_phasor_v_matrix": [_vp, _dp, C.c_int, _dp, C.c_int, C.c_double, _dp, _dp, C.c_int, _dp, _dp],
    "hipdrt_chrono_var_matrix": [_vp, _dp, C.c_int, _ip, C.c_int, C.c_double, C.c_int, _dp],
    "hipdrt_response_lookup": [_vp, C.c_double, C.c_int, C.c_int, _dp, _dp],
    "hipdrt_response_matrix": [_vp, _dp, C.c_int, _dp, C.c_int, _dp, _dp, C.c_int, C.c_int, C.c_double, C.c_int, _dp, _dp,
                               C.c_int, _dp, _dp],
    "hipdrt_plan_bytes_per_spectrum": [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_longlong)],
    "hipdrt_response_matrix_variant": [_vp, _dp, C.c_int, _dp, C.c_int, _dp, _dp, _dp, C.c_int, C.c_int, C.c_double, C.c_int,
                                       _dp, _dp],
    "hipdrt_nonuniform_gaussian_filter1d": [_vp, _dp, C.c_int, _dp, _ip, C.c_int, _ip, _dp, C.c_int, _dp, _dp, C.c_longlong,
                                            _ip, _ip, _dp],
    "hipdrt_map_filter": [_vp, C.POINTER(MapFilterArgs), _dp, _dp, _dp, _dp],
    "hipdrt_rank_filter": [_vp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _dp],
    "hipdrt_percentiles": [_vp, _dp, C.c_int, C.c_int, C.c_int, _dp, C.c_int, _dp],
    "hipdrt_map_badness": [_vp, C.POINTER(MapBadnessArgs), _dp, _dp, _dp, C.POINTER(C.c_ubyte), _dp],
    "hipdrt_map_predict": [_vp, C.POINTER(MapPredictArgs), _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp],
    "hipdrt_penalty_matrices": [_vp, _dp, C.c_int, C.c_double, C.c_int, _dp, _dp, _dp],
    "hipdrt_eis_var_matrix": [_vp, _dp, C.c_int, C.c_double, C.c_double, C.c_int, _dp],
    "hipdrt_qp_batch": [_vp, C.c_int, C.c_int, C.c_int, _dp, _dp, C.c_int, _dp, C.POINTER(QpOpts), _dp, _ip, _dp, _ip],
    "hipdrt_qp_profile": [_vp, C.POINTER(C.c_ulonglong), C.c_int, C.c_int],
    "hipdrt_debug_qp_occupancy": [_vp, C.c_int, C.c_int],
    "hipdrt_debug_qp_group": [_vp, C.c_int],
    "hipdrt_debug_exact_zero_shortcuts": [_vp, C.c_int],
    "hipdrt_debug_qp_waves": [_vp, C.c_int],
    "hipdrt_debug_stream_pool": [_vp, C.c_int, C.POINTER(C.c_void_p), _ip, _ip, _ip],
    "hipdrt_debug_gram_l2": [_vp, C.POINTER(DebugGramArgs)],
    "hipdrt_debug_pack_p": [_vp, C.c_int, C.c_int, _dp, C.c_int, _dp],
    "hipdrt_debug_hyper_step": [_vp, C.POINTER(DebugHyperArgs)],
    "hipdrt_debug_prep": [_vp, C.POINTER(DebugSetupArgs)],
    "hipdrt_debug_init_weights": [_vp, C.POINTER(DebugSetupArgs)],
    "hipdrt_debug_weight_method": [_vp, C.POINTER(DebugSetupArgs)],
    "hipdrt_debug_llh": [_vp, C.POINTER(DebugSetupArgs)],
    "hipdrt_debug_rowop": [_vp, C.POINTER(DebugRowopArgs)],
    "hipdrt_debug_hyper_form": [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, C.POINTER(C.c_longlong)],
    "hipdrt_debug_impedance_interp_form": [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _ip, _ip, C.POINTER(C.c_longlong)],
    "hipdrt_debug_kk_stats": [_vp, C.c_int, C.c_int, _dp, _dp, _dp, C.POINTER(KkOpts), _dp, _ip, _dp, _ip, _ip],
    "hipdrt_default_kk_opts": [C.POINTER(KkOpts)],
    "hipdrt_plan_kk_screen": [_vp, C.POINTER(KkOpts), C.c_int, _dp, _dp, _dp, _dp, _dp, _ip, _dp, _ip, _ip],
    "hipdrt_func_eval_matrix": [_vp, _dp, C.c_int, _dp, C.c_int, C.c_double, C.c_int, _dp],
    "hipdrt_plan_set_tau_basis": [_vp, _dp, C.c_int, C.c_double],
    "hipdrt_plan_predict_drt": [_vp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_double, C.c_double, _dp, _dp, _dp, _ip],
    "hipdrt_plan_predict_z": [_vp, _dp, C.c_int, C.c_int, _dp, _dp, _ip],
    "hipdrt_plan_predict_resistances": [_vp, _dp, _dp, _dp, C.c_int],
    "hipdrt_plan_set_predict_desc": [_vp, C.POINTER(PredictDesc)],
    "hipdrt_plan_predict_response": [_vp, C.POINTER(ResponseArgs), _dp, _ip],
    "hipdrt_plan_predict_z_model": [_vp, C.POINTER(ZModelArgs), _dp, _dp, _ip],
    "hipdrt_plan_predict_dop": [_vp, _dp, C.c_int, _dp, C.c_double, _dp, C.c_double, C.c_int, _dp, _ip],
    "hipdrt_plan_dop_posterior": [_vp, C.POINTER(DopArgs), _dp, _dp, _dp, _dp, _ip],
    "hipdrt_plan_dop_cov": [_vp, C.c_int, C.POINTER(DopArgs), _dp, _ip],
    "hipdrt_debug_response": [_vp, C.POINTER(DebugResponseArgs)],
    "hipdrt_peak_opts_default": [C.POINTER(PeakOpts)],
    "hipdrt_plan_find_peaks": [_vp, _dp, C.c_int, C.POINTER(PeakOpts), _dp, _ip, _ip, _dp, _dp, _dp, _ip, _ip, _ip, _dp, _dp, _dp,
                               _ip],
    "hipdrt_debug_find_peaks": [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.POINTER(PeakOpts), _ip, _ip, _dp, _dp, _dp, _ip, _ip,
                                _ip, _dp, _dp, _dp],
    "hipdrt_peak_prob_opts_default": [C.POINTER(PeakProbOpts)],
    "hipdrt_plan_peak_trough_probs": [_vp, _dp, C.c_int, C.POINTER(PeakProbOpts), _dp, C.c_int, _ip, _ip, _dp, _dp, _dp, _dp, _dp,
                                      _ip, _dp, _dp, _ip, _ip, _ip, _ip, _ip],
    "hipdrt_debug_peak_trough_probs": [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.POINTER(PeakProbOpts), C.c_int,
                                       _ip, _ip, _dp, _dp, _dp, _dp, _ip, _dp, _dp, _ip, _ip, _ip, _ip],
    "hipdrt_peak_resolve_opts_default": [C.POINTER(PeakResolveOpts)],
    "hipdrt_plan_resolve_peaks": [_vp, C.POINTER(PeakResolveIn), C.POINTER(PeakResolveOpts), C.POINTER(PeakResolveOut)],
    "hipdrt_plan_integrate_drt": [_vp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _ip, _ip, C.c_int, _dp, _ip],
    "hipdrt_debug_peak_resolve": [_vp, C.POINTER(DebugPeakResolveArgs)],
    "hipdrt_plan_score_candidates": [_vp, C.POINTER(CandidatesIn), C.POINTER(CandidatesOut)],
    "hipdrt_default_lml_in": [C.POINTER(LmlIn)],
    "hipdrt_plan_lml_terms": [_vp, C.POINTER(LmlIn), C.POINTER(LmlOut)],
    "hipdrt_debug_logdet": [_vp, C.c_int, C.c_int, _dp, _dp, _ip],
    "hipdrt_plan_resolve_group": [_vp, C.POINTER(ResolveArgs), _dp, _ip, _ip],
    "hipdrt_debug_resolve_assemble": [_vp, C.POINTER(ResolveArgs), C.c_int, _dp, _dp, _dp, _dp],
    "hipdrt_debug_candidate_llh": [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp],
    "hipdrt_debug_candidate_form": [_vp, C.c_int],
    "hipdrt_debug_posterior": [_vp, C.POINTER(DebugPosteriorArgs)],
    "hipdrt_debug_dop_posterior": [_vp, C.POINTER(DebugDopPosteriorArgs)],
    "hipdrt_debug_qp": [_vp, C.POINTER(DebugQpArgs)],
    "hipdrt_debug_lpt_order": [_vp, C.c_int, _ip, _ip, _ip],
    "hipdrt_plan_pfrt_bytes_per_spectrum": [C.c_int, C.c_int, C.POINTER(C.c_longlong)],
    "hipdrt_plan_pfrt_begin": [_vp, C.c_int],
    "hipdrt_plan_pfrt_record": [_vp],
    "hipdrt_plan_pfrt_steps": [_vp, _ip],
    "hipdrt_plan_pfrt_restore_s": [_vp, C.c_int, C.c_double],
    "hipdrt_plan_pfrt_get_step": [_vp, C.c_int, _dp, _dp, _dp, _dp, _dp, _ip],
    "hipdrt_plan_get_step_p_matrix": [_vp, C.c_int, C.c_int, _dp],
    "hipdrt_pfrt_opts_default": [C.POINTER(PfrtOpts)],
    "hipdrt_plan_predict_pfrt": [_vp, _dp, _dp, C.c_int, _dp, C.c_int, C.POINTER(PfrtOpts), _dp, _dp, _dp, _dp, _ip],
    "hipdrt_pfrt_select_opts_default": [C.POINTER(PfrtSelectOpts)],
    "hipdrt_plan_pfrt_select": [_vp, _dp, _dp, C.c_int, C.POINTER(PfrtOpts), C.POINTER(PfrtSelectOpts), C.POINTER(PfrtSelectOut),
                                _ip],
    "hipdrt_debug_pfrt_select": [_vp, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int, C.POINTER(PfrtSelectOpts),
                                 C.POINTER(PfrtSelectOut), _ip],
    "hipdrt_debug_pfrt_step": [_vp, C.c_int, C.c_int, _ip, _dp, _dp, _dp, _dp, _dp, C.c_double, C.c_int, C.c_int, _dp],
    "hipdrt_debug_pfrt_combine": [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.c_int, C.POINTER(PfrtOpts), _dp, _dp,
                                  _dp, _dp, _dp],
    "hipdrt_debug_last_predict_ms": [_vp, C.POINTER(C.c_float)],
    "hipdrt_debug_map_filter_stats": [_vp, _dp],
    "hipdrt_debug_map_badness_ms": [_vp, _dp],
    "hipdrt_debug_map_gaussian": [_vp, _dp, C.c_int, C.c_int, C.POINTER(FilterTable), C.c_int, _dp],
    "hipdrt_debug_map_reduce": [_vp, _dp, C.c_longlong, C.c_int, _dp],
    "hipdrt_debug_map_prob": [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, _ip, C.c_int, C.c_int, C.c_double, C.c_double, C.c_int,
                              _dp, _dp, _dp, _dp],
    "hipdrt_debug_apply_rows": [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, _dp],
    "hipdrt_comm_unique_id": [C.c_char_p],
    "hipdrt_comm_create": [C.c_int, C.c_int, C.c_int, C.c_char_p, C.POINTER(_vp)],
    "hipdrt_comm_destroy": [_vp],
    "hipdrt_comm_info": [_vp, _ip, _ip, _ip],
    "hipdrt_comm_broadcast_dev": [_vp, _vp, C.c_longlong, C.c_int],
    "hipdrt_comm_gather_dev": [_vp, _vp, C.c_longlong, _vp, C.c_int],
    "hipdrt_comm_broadcast": [_vp, _dp, C.c_longlong, C.c_int],
    "hipdrt_comm_gather": [_vp, _dp, C.c_longlong, _dp, C.c_int],
    "hipdrt_comm_allreduce_max": [_vp, _dp],
    "hipdrt_comm_barrier": [_vp],
    "hipdrt_device_alloc": [_vp, C.c_longlong, C.POINTER(_vp)],
    "hipdrt_device_free": [_vp, _vp],
    "hipdrt_device_synchronize": [_vp],
    "hipdrt_device_probe": [C.c_int],
    "hipdrt_weighted_gram": [_vp, C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, C.c_int, _dp, _dp, _dp, _dp],
    "hipdrt_default_fit_opts": [C.POINTER(FitOpts)],
    "hipdrt_plan_create": [_vp, _dp, C.c_int, _dp, C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                           _dp, _dp, _dp, _dp, C.POINTER(FitOpts), C.c_int, C.POINTER(_vp)],
    "hipdrt_plan_create_prepared": [_vp, C.POINTER(PreparedDesc), _dp, _dp, _dp, _dp, _dp, _dp, _dp, C.POINTER(FitOpts),
                                    C.c_int, C.POINTER(_vp)],
    "hipdrt_plan_upload_prepared": [_vp, C.c_int, C.c_int, _dp, _dp],
    "hipdrt_plan_set_weight_factors": [_vp, C.c_double, _dp, C.c_int],
    "hipdrt_plan_set_init_h": [_vp, _dp],
    "hipdrt_plan_destroy": [_vp],
    "hipdrt_plan_dims": [_vp, _ip, _ip, _ip],
    "hipdrt_plan_get": [_vp, C.c_char_p, _dp, C.c_longlong],
    "hipdrt_plan_set_lookup": [_vp, _dp, _dp],
    "hipdrt_plan_upload": [_vp, C.c_int, _dp, _dp],
    "hipdrt_plan_fit": [_vp],
    "hipdrt_plan_set_subbatches": [_vp, C.c_int],
    "hipdrt_plan_download": [_vp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _dp, _ip, _ip, _ip],
    "hipdrt_plan_get_p_matrix": [_vp, C.c_int, _dp],
    "hipdrt_plan_distribution_var": [_vp, _dp, C.c_int, _dp, _ip],
    "hipdrt_plan_llh_terms": [_vp, _dp, _dp],
    "hipdrt_plan_obs_llh_terms": [_vp, _dp, _dp],
    "hipdrt_plan_obs_llh_terms_w": [_vp, C.c_int, C.c_double, _dp, _dp],
    "hipdrt_plan_set_state": [_vp, _dp, _dp, _dp, _dp],
    "hipdrt_plan_set_state_dop": [_vp, _dp],
    "hipdrt_plan_continue": [_vp, C.POINTER(FitOpts), C.c_double, C.c_int],
    "hipdrt_plan_iterate": [_vp, C.POINTER(IterateState), _ip, _ip, _ip, _dp],
    "hipdrt_plan_param_var": [_vp, _dp, _ip],
    "hipdrt_plan_param_cov": [_vp, C.c_int, _dp, _ip],
    "hipdrt_plan_distribution_cov": [_vp, C.c_int, _dp, C.c_int, _dp, _ip],
    "hipdrt_plan_record_history": [_vp, C.c_int],
    "hipdrt_plan_get_history": [_vp, _dp, _dp, _dp, _ip, C.c_int, _ip],
    "hipdrt_plan_timings": [_vp, C.POINTER(C.c_float), _ip],
    "hipdrt_fit_eis_batch": [_vp, C.c_int, _dp, C.c_int, _dp, _dp, _dp, C.c_int, C.c_double, C.c_int, C.c_int,
                             C.c_int, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.POINTER(FitOpts), _dp, _dp, _dp, _dp,
                             _dp, _dp, _dp, _dp, _ip, _ip],
}
_RESTYPES = {"hipdrt_last_error": C.c_char_p, "hipdrt_stream": C.c_void_p, "hipdrt_default_fit_opts": None,
             "hipdrt_default_kk_opts": None, "hipdrt_default_lml_in": None, "hipdrt_peak_opts_default": None, "hipdrt_peak_prob_opts_default": None,
             "hipdrt_peak_resolve_opts_default": None, "hipdrt_pfrt_opts_default": None,
             "hipdrt_pfrt_select_opts_default": None}

_lib = None
_lock = threading.Lock()


def load_library():
    """dlopen libhipdrt.so and attach the prototypes (no device is touched)."""
    global _lib
    with _lock:
        if _lib is None:
            # The HIP runtime maps streams onto 4 hardware queues by default (one of them the null stream's).  libhipdrt creates
            # its streams once per device, one per remaining queue, and deals them to contexts and to the ranges of a fit by
            # activity and compute pipe (csrc/api.hip: StreamPool; profiles/r06_trace_queue_placement.txt) -- with 8 queues it has
            # seven streams over the four pipes, enough for four ranges or four plans side by side on a pipe each; with 4 it
            # has three.  The variable is read when the runtime starts, i.e. at the first HIP call of the process: set here, as
            # a default the caller's environment overrides, it takes effect unless something else in the process has started HIP.
            # (If torch is loaded and has started HIP already, the runtime runs with whatever it found then: exporting 8 now
            # would only make libhipdrt size its stream pool for queues that do not exist.)
            torch_mod = sys.modules.get("torch")
            hip_started = False
            try:
                hip_started = bool(torch_mod is not None and torch_mod.cuda.is_initialized())
            except Exception:                    # noqa: BLE001 (a torch build without the cuda module)
                hip_started = False
            if not hip_started:
                os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
            if not os.path.exists(LIB_PATH):
                raise HipDrtError(f"{LIB_PATH} not found: build it with `python -c 'import __graft_entry__ as g; "
                                  f"g.build()'` (hipdrt has no CPU fallback)")
            lib = C.CDLL(LIB_PATH)
            for name, argtypes in SIGNATURES.items():
                fn = getattr(lib, name, None)
                if fn is None:
                    # (tools/: A/B against an OLDER build through HIPDRT_LIB -- a debug hook it does not have yet is simply not
                    # bound; every other missing symbol is an error, as is any missing symbol of the in-tree library)
                    if name.startswith("hipdrt_debug_") and "HIPDRT_LIB" in os.environ:
                        continue
                    raise HipDrtError(f"{LIB_PATH} does not export {name}")
                fn.argtypes = argtypes
                fn.restype = _RESTYPES.get(name, C.c_int)
            _lib = lib
    return _lib


def _check(rc, raises=None):
    """a non-zero return code raises HipDrtError, or what `raises` maps it to, e.g. {E_UNSUPPORTED: NotImplementedError}"""
    if rc != 0:
        msg = load_library().hipdrt_last_error().decode()
        if raises and rc in raises:
            raise raises[rc](msg)
        raise HipDrtError(f"hipdrt error {rc}: {msg}")


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _pi(a):
    return None if a is None else a.ctypes.data_as(_ip)
