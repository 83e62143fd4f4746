"""ctypes binding of libhipdrt.so (C-ABI declared in include/hipdrt.h).  numpy in, numpy out.

There is deliberately no CPU fallback: if the shared library is missing, or no gfx950 device is visible,
every compute entry point raises ``HipDrtError``.
"""
from __future__ import annotations

import ctypes as C
import os
import sys
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
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
class IterateState(C.Structure):
    """hipdrt_iterate_state (include/hipdrt.h): the arrays iterate_qphb takes; NULL keeps the device value"""
    _fields_ = [(name, C.POINTER(C.c_double)) for name in
                ("x_in", "s_vectors", "rho", "dop_rho", "weights", "est_weights", "xmx_norms", "dop_xmx_norms")]


_vp = C.c_void_p


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


class PfrtOpts(C.Structure):
    """hipdrt_pfrt_opts (include/hipdrt.h)"""
    _fields_ = [("eval_sign", C.c_int), ("search", C.c_int), ("height", C.c_double), ("prominence", C.c_double),
                ("prior_mu", C.c_double), ("prior_sigma", C.c_double), ("n_eff_factor", C.c_double), ("fxx_var_floor", C.c_double),
                ("ext_left", C.c_int), ("ext_right", C.c_int), ("smooth", C.c_int), ("smooth_order", C.c_double),
                ("smooth_epsilon", C.c_double), ("integrate", C.c_int), ("integrate_threshold", C.c_double), ("normalize", C.c_int)]


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


class DebugPosteriorArgs(C.Structure):
    """hipdrt_debug_posterior_args (include/hipdrt_debug.h)"""
    _fields_ = [("B", C.c_int), ("n", C.c_int), ("P", _dp), ("p_batched", C.c_int), ("ldp", C.c_int), ("rows", _dp),
                ("neval", C.c_int), ("ncol", C.c_int), ("col_offset", C.c_int), ("scale", _dp), ("cov_member", C.c_int),
                ("var", _dp), ("status", _ip), ("cov", _dp), ("bex", _dp), ("tail", _dp)]


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
    "hipdrt_debug_hyper_form": [_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _ip, C.POINTER(C.c_longlong)],
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
    "hipdrt_debug_response": [_vp, C.POINTER(DebugResponseArgs)],
    "hipdrt_peak_opts_default": [C.POINTER(PeakOpts)],
    "hipdrt_plan_find_peaks": [_vp, _dp, C.c_int, C.POINTER(PeakOpts), _dp, _ip, _ip, _dp, _dp, _dp, _ip, _ip, _ip, _dp, _dp, _dp,
                               _ip],
    "hipdrt_debug_find_peaks": [_vp, C.c_int, C.c_int, _dp, _dp, _dp, _dp, C.POINTER(PeakOpts), _ip, _ip, _dp, _dp, _dp, _ip, _ip,
                                _ip, _dp, _dp, _dp],
    "hipdrt_peak_resolve_opts_default": [C.POINTER(PeakResolveOpts)],
    "hipdrt_plan_resolve_peaks": [_vp, C.POINTER(PeakResolveIn), C.POINTER(PeakResolveOpts), C.POINTER(PeakResolveOut)],
    "hipdrt_plan_integrate_drt": [_vp, _dp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, _ip, _ip, C.c_int, _dp, _ip],
    "hipdrt_debug_peak_resolve": [_vp, C.POINTER(DebugPeakResolveArgs)],
    "hipdrt_plan_score_candidates": [_vp, C.POINTER(CandidatesIn), C.POINTER(CandidatesOut)],
    "hipdrt_debug_candidate_llh": [_vp, C.c_int, C.c_int, C.c_int, C.c_int, _dp, C.c_int, _dp, _dp, _dp, _dp, _dp, _dp],
    "hipdrt_debug_candidate_form": [_vp, C.c_int],
    "hipdrt_debug_posterior": [_vp, C.POINTER(DebugPosteriorArgs)],
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
             "hipdrt_default_kk_opts": None, "hipdrt_peak_opts_default": None,
             "hipdrt_peak_resolve_opts_default": None, "hipdrt_pfrt_opts_default": None}

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


def _check(rc):
    if rc != 0:
        raise HipDrtError(f"hipdrt error {rc}: {load_library().hipdrt_last_error().decode()}")


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _p(a):
    return None if a is None else a.ctypes.data_as(_dp)


def _pi(a):
    return None if a is None else a.ctypes.data_as(_ip)


def default_fit_opts() -> FitOpts:
    o = FitOpts()
    load_library().hipdrt_default_fit_opts(C.byref(o))
    return o


def kk_opts(n_outlier_iter=2, p_thresh=1e-4, n_sigma=None, std_sample_fraction=0.6, n_std=None, max_num_outliers=2,
            outlier_weight=1e-10) -> KkOpts:
    """hipdrt_kk_opts from the keywords of DRT.kk_test (None <-> -1 for n_sigma); n_std=None: the library's default for a
    std_sample_fraction of 0.6, otherwise the caller supplies the quantile that goes with its fraction"""
    o = KkOpts()
    load_library().hipdrt_default_kk_opts(C.byref(o))
    o.n_outlier_iter, o.p_thresh = int(n_outlier_iter), float(p_thresh)
    o.n_sigma = -1.0 if n_sigma is None else float(n_sigma)
    if n_std is None and float(std_sample_fraction) != o.std_sample_fraction:
        raise ValueError("n_std must be given with a std_sample_fraction other than the default")
    o.std_sample_fraction = float(std_sample_fraction)
    if n_std is not None:
        o.n_std = float(n_std)
    o.max_num_outliers, o.outlier_weight = int(max_num_outliers), float(outlier_weight)
    return o


PEAK_METHODS = {'thresh': 0, 'prob': 1, 'map': 2}


def peak_opts(eval_sign=1, search=1, normalize=1, method='thresh', height=None, prominence=None, prob_thresh=0.25, num_peaks=None,
              fxx_var_floor=1e-5, ext_left=-1, ext_right=-1) -> PeakOpts:
    """hipdrt_peak_opts from the keywords of DRT.find_peaks (None <-> NaN for the automatic thresholds, None <-> 0 for num_peaks);
    method 'thresh', 'prob' or 'map' (the peak_prob / curv_prob rows), or its number"""
    o = PeakOpts()
    load_library().hipdrt_peak_opts_default(C.byref(o))
    o.eval_sign, o.search, o.normalize = int(eval_sign), int(search), int(normalize)
    o.method = PEAK_METHODS[method] if isinstance(method, str) else int(method)
    o.height = float('nan') if height is None else float(height)
    o.prominence = float('nan') if prominence is None else float(prominence)
    o.prob_thresh, o.num_peaks, o.fxx_var_floor = float(prob_thresh), int(num_peaks or 0), float(fxx_var_floor)
    o.ext_left, o.ext_right = int(ext_left), int(ext_right)
    return o


def pfrt_opts(**kw) -> PfrtOpts:
    """hipdrt_pfrt_opts: the library's defaults (DRT.predict_pfrt's) with the given fields replaced"""
    o = PfrtOpts()
    load_library().hipdrt_pfrt_opts_default(C.byref(o))
    names = {name for name, _ in PfrtOpts._fields_}
    for k, v in kw.items():
        if k not in names:
            raise TypeError(f"hipdrt_pfrt_opts has no field {k!r}")
        setattr(o, k, type(getattr(o, k))(v))
    return o


def pfrt_bytes_per_spectrum(n, steps):
    """bytes the PFRT step store takes per spectrum of the plan's capacity (hipdrt_plan_pfrt_bytes_per_spectrum)"""
    out = C.c_longlong()
    _check(load_library().hipdrt_plan_pfrt_bytes_per_spectrum(int(n), int(steps), C.byref(out)))
    return int(out.value)


PEAKS_OVERFLOW, PEAKS_UNORDERED = -4, -5            # per-spectrum statuses of hipdrt_plan_resolve_peaks
PEAKS_FROM_FIND, PEAKS_FROM_INDICES, PEAKS_FROM_WINDOWS = 0, 1, 2
CANDIDATES_FROM_STEPS, CANDIDATES_FROM_HOST = 0, 1
CANDIDATE_ABSENT = -6                               # status of a slot at or past the spectrum's ncand (hipdrt_plan_score_candidates)
CANDIDATE_OUTPUTS = ("rss", "sum_log_w", "count", "peak_index", "heights", "prominences", "status")
RESOLVE_OUTPUTS = ("count", "peak_index", "trough_index", "eps_l", "eps_r", "r_peaks", "r_coef", "x_peaks", "peak_gammas", "status")


def peak_resolve_opts(sign=1, max_peaks=16, epsilon_factor=1.25, max_epsilon=1.25, min_epsilon=None,
                      epsilon_uniform=None) -> PeakResolveOpts:
    """hipdrt_peak_resolve_opts from the keywords of DRT.estimate_peak_coef (None <-> NaN for min_epsilon and epsilon_uniform)"""
    o = PeakResolveOpts()
    load_library().hipdrt_peak_resolve_opts_default(C.byref(o))
    o.sign, o.max_peaks = int(sign), int(max_peaks)
    o.epsilon_factor, o.max_epsilon = float(epsilon_factor), float(max_epsilon)
    o.min_epsilon = float('nan') if min_epsilon is None else float(min_epsilon)
    o.epsilon_uniform = float('nan') if epsilon_uniform is None else float(epsilon_uniform)
    return o


def _resolve_outputs(B, mp, nb, nout, want=None):
    """host arrays of the resolve entry points, poisoned so that anything the kernel leaves unwritten shows (-77 / 7e77: NaN
    is a legitimate padding value); want: the names to allocate (None: all) -- count and status always come"""
    shapes = dict(count=(B,), status=(B,), peak_index=(B, mp), trough_index=(B, mp), eps_l=(B, mp), eps_r=(B, mp),
                  r_peaks=(B, mp), r_coef=(B, mp), x_peaks=(B, mp, nb), peak_gammas=(B, mp, nout))
    out = {}
    for k, shape in shapes.items():
        if want is not None and k not in want and k not in ("count", "status"):
            continue
        if nout == 0 and k in ("r_peaks", "peak_gammas"):
            continue
        integer = k in ("count", "status", "peak_index", "trough_index")
        out[k] = np.full(shape, -77, dtype=np.int32) if integer else np.full(shape, 7e77)
    return out


def _resolve_out_struct(out):
    u = PeakResolveOut()
    for k in RESOLVE_OUTPUTS:
        a = out.get(k)
        setattr(u, k, None if a is None else (_pi(a) if a.dtype == np.int32 else _p(a)))
    return u


def _i32(a):
    return np.ascontiguousarray(a, dtype=np.int32)


_PEAK_INT = ("peak_sign", "keep", "left_bases", "right_bases")
_PEAK_F64 = ("heights", "prominences", "probs", "peak_prob", "curv_prob")


def _peak_outputs(B, n, method, want=None):
    """host arrays of the peak entry points, poisoned so that anything a kernel leaves unwritten shows; want: the names to
    allocate (None: all the method has) -- what is left out is passed as NULL and neither formed nor downloaded"""
    names = _PEAK_INT + _PEAK_F64[:3] + (_PEAK_F64[3:] if method == 2 else ()) + ("count", "used_prominence")
    out = {}
    for k in names:
        if want is not None and k not in want:
            continue
        shape = B if k in ("count", "used_prominence") else (B, n)
        out[k] = np.full(shape, -77, dtype=np.int32) if k in _PEAK_INT + ("count",) else np.full(shape, np.nan)
    return out


def _peak_out_args(out):
    g = out.get
    return (_pi(g("peak_sign")), _pi(g("keep")), _p(g("heights")), _p(g("prominences")), _p(g("probs")), _pi(g("left_bases")),
            _pi(g("right_bases")), _pi(g("count")), _p(g("used_prominence")), _p(g("peak_prob")), _p(g("curv_prob")))


def _kk_outputs(B, nf):
    return dict(std=np.empty(B), outlier_mask=np.empty((B, nf), dtype=np.int32), f_lim=np.empty((B, 2)),
                i_lim=np.empty((B, 2), dtype=np.int32), status=np.empty(B, dtype=np.int32))


class Context:
    """One hipdrt_ctx (device + stream)."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        h = _vp()
        _check(self._lib.hipdrt_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.hipdrt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self):
        return self._lib.hipdrt_stream(self._h)

    def synchronize(self):
        _check(self._lib.hipdrt_synchronize(self._h))

    def plan_bytes_per_spectrum(self, nf, ntau, ns):
        """device bytes one staged spectrum costs an EIS plan of this shape (hipdrt_plan_bytes_per_spectrum)"""
        out = C.c_longlong(0)
        _check(self._lib.hipdrt_plan_bytes_per_spectrum(int(nf), int(ntau), int(ns), C.byref(out)))
        return out.value

    def device_info(self):
        buf = C.create_string_buffer(64)
        ncu = C.c_int()
        hbm = C.c_longlong()
        _check(self._lib.hipdrt_device_info(self._h, buf, 64, C.byref(ncu), C.byref(hbm)))
        return dict(arch=buf.value.decode(), num_cu=ncu.value, hbm_bytes=hbm.value)

    # ---- L1 ------------------------------------------------------------------------------------------
    def impedance_lookup(self, epsilon, wt_re, wt_im, ny=1000):
        wt_re, wt_im = _f64(wt_re), _f64(wt_im)
        z_re, z_im = np.empty_like(wt_re), np.empty_like(wt_im)
        _check(self._lib.hipdrt_impedance_lookup(self._h, float(epsilon), wt_re.size, int(ny), _p(wt_re), _p(wt_im),
                                                 _p(z_re), _p(z_im)))
        return z_re, z_im

    def impedance_matrix(self, freq, tau, epsilon, mode=MODE_INTERP, toeplitz=False, lookups=None, ny=1000):
        freq, tau = _f64(freq), _f64(tau)
        batched = freq.ndim == 2
        B = freq.shape[0] if batched else 1
        nf = freq.shape[-1]
        if lookups is not None:
            (lre, zre), (lim, zim) = lookups
            lre, zre, lim, zim = _f64(lre), _f64(zre), _f64(lim), _f64(zim)
            ng = lre.size
        else:
            lre = zre = lim = zim = None
            ng = 0
        a_re = np.empty((B, nf, tau.size))
        a_im = np.empty((B, nf, tau.size))
        _check(self._lib.hipdrt_impedance_matrix(self._h, B, int(batched), _p(freq), nf, _p(tau), tau.size, int(mode),
                                                 int(bool(toeplitz)), float(epsilon), ng, _p(lre), _p(zre), _p(lim),
                                                 _p(zim), int(ny), _p(a_re), _p(a_im)))
        if not batched:
            return a_re[0], a_im[0]
        return a_re, a_im

    def impedance_matrix_timed(self, freq, tau, epsilon, dev_re, dev_im, mode=MODE_INTERP, toeplitz=False,
                               lookups=None, ny=1000, repeat=1):
        """Device-resident build (dev_re/dev_im: integer device pointers); returns elapsed ms of `repeat` launches."""
        freq, tau = _f64(freq), _f64(tau)
        batched = freq.ndim == 2
        B = freq.shape[0] if batched else 1
        nf = freq.shape[-1]
        (lre, zre), (lim, zim) = lookups if lookups is not None else ((None, None), (None, None))
        arrs = [None if a is None else _f64(a) for a in (lre, zre, lim, zim)]
        ng = 0 if arrs[0] is None else arrs[0].size
        ms = C.c_float()
        _check(self._lib.hipdrt_impedance_matrix_dev(self._h, B, int(batched), _p(freq), nf, _p(tau), tau.size,
                                                     int(mode), int(bool(toeplitz)), float(epsilon), ng, _p(arrs[0]),
                                                     _p(arrs[1]), _p(arrs[2]), _p(arrs[3]), int(ny), _vp(dev_re),
                                                     _vp(dev_im), int(repeat), C.byref(ms)))
        return ms.value

    def phasor_z_matrix(self, freq, nu, nu_epsilon):
        freq, nu = _f64(freq), _f64(nu)
        zr, zi = np.empty((freq.size, nu.size)), np.empty((freq.size, nu.size))
        _check(self._lib.hipdrt_phasor_z_matrix(self._h, _p(freq), freq.size, _p(nu), nu.size, float(nu_epsilon), _p(zr),
                                                _p(zi)))
        return zr + 1j * zi

    def phasor_v_matrix(self, times, nu, nu_epsilon, step_times, step_sizes):
        times, nu, st, sa = _f64(times), _f64(nu), _f64(step_times), _f64(step_sizes)
        rm = np.empty((times.size, nu.size))
        lay = np.empty((st.size, times.size, nu.size))
        _check(self._lib.hipdrt_phasor_v_matrix(self._h, _p(times), times.size, _p(nu), nu.size, float(nu_epsilon), _p(st),
                                                _p(sa), st.size, _p(rm), _p(lay)))
        return rm, lay

    def chrono_var_matrix(self, tt, seg, vmm_epsilon, uniform=False):
        tt = _f64(tt)
        seg = np.ascontiguousarray(seg, dtype=np.int32)
        out = np.empty((tt.size, tt.size))
        _check(self._lib.hipdrt_chrono_var_matrix(self._h, _p(tt), tt.size, _pi(seg), seg.size - 1, float(vmm_epsilon),
                                                  int(bool(uniform)), _p(out)))
        return out

    def response_lookup(self, epsilon, td, ny=1000):
        td = _f64(td)
        v = np.empty_like(td)
        _check(self._lib.hipdrt_response_lookup(self._h, float(epsilon), td.size, int(ny), _p(td), _p(v)))
        return v

    def response_matrix(self, times, tau, step_times, step_sizes, epsilon, mode=MODE_INTERP, lookup=None, ny=1000,
                        layered=True):
        times, tau, st, sa = _f64(times), _f64(tau), _f64(step_times), _f64(step_sizes)
        if st.size != sa.size:
            raise ValueError("step_times and step_sizes must have the same length")
        a = np.empty((times.size, tau.size))
        lay = np.empty((st.size, times.size, tau.size)) if layered else None
        if lookup is not None:
            log_td, v = _f64(lookup[0]), _f64(lookup[1])
            ng, plt, pv = log_td.size, _p(log_td), _p(v)
        else:
            ng, plt, pv = 0, None, None
        _check(self._lib.hipdrt_response_matrix(self._h, _p(times), times.size, _p(tau), tau.size, _p(st), _p(sa), st.size,
                                                int(mode), float(epsilon), ng, plt, pv, int(ny), _p(a),
                                                _p(lay) if layered else None))
        return a, lay

    def response_matrix_variant(self, times, tau, step_times, step_sizes, variant, tau_rise=None, epsilon=1.0, ny=1000,
                                layered=True):
        """the potentiostatic (RESPONSE_POT) and the expdecay-step (RESPONSE_EXPDECAY, trapz) forms of construct_response_matrix"""
        times, tau, st, sa = _f64(times), _f64(tau), _f64(step_times), _f64(step_sizes)
        if st.size != sa.size:
            raise ValueError("step_times and step_sizes must have the same length")
        tr = None
        if tau_rise is not None:
            tr = _f64(tau_rise)
            if tr.size != st.size:
                raise ValueError("tau_rise needs one entry per step")
        a = np.empty((times.size, tau.size))
        lay = np.empty((st.size, times.size, tau.size)) if layered else None
        _check(self._lib.hipdrt_response_matrix_variant(self._h, _p(times), times.size, _p(tau), tau.size, _p(st), _p(sa),
                                                        _p(tr) if tr is not None else None, st.size, int(variant), float(epsilon),
                                                        int(ny), _p(a), _p(lay) if layered else None))
        return a, lay

    def nonuniform_gaussian_filter1d(self, y, sigma, seg, filtered, nodes, node_delta, weights, woff, radius):
        """segment-wise blended Gaussian filter; see hipdrt.filters.nonuniform_gaussian_filter1d for the set-up"""
        y, sigma, nodes, node_delta, weights = _f64(y), _f64(sigma), _f64(nodes), _f64(node_delta), _f64(weights)
        seg, filtered, woff, radius = (np.ascontiguousarray(a, dtype=np.int32) for a in (seg, filtered, woff, radius))
        out = np.empty_like(y)
        _check(self._lib.hipdrt_nonuniform_gaussian_filter1d(self._h, _p(y), y.size, _p(sigma), _pi(seg), seg.size - 1,
                                                             _pi(filtered), _p(nodes), nodes.shape[1], _p(node_delta),
                                                             _p(weights), weights.size, _pi(woff), _pi(radius), _p(out)))
        return out

    def map_filter(self, a, args: MapFilterArgs, want_weights=False, want_sigmas=False):
        """hipdrt_map_filter on a 1-D or 2-D array (NaN = missing); `args` comes filled but for the shape (hipdrt.filters builds
        it).  Returns dict(out=, weights=, sigmas=) with the entries the call produces."""
        a = _f64(a)
        if a.ndim not in (1, 2):
            raise ValueError("a 1-D or 2-D array")
        args.ndim, args.rows, args.cols = a.ndim, a.shape[0], (a.shape[1] if a.ndim == 2 else 1)
        res = {}
        if args.op == MAP_FILTER:
            res["out"] = np.empty_like(a)
            if want_weights:
                res["weights"] = np.empty_like(a)
        if want_sigmas or args.op == MAP_SIGMAS:
            res["sigmas"] = np.empty((a.ndim,) + a.shape)
        _check(self._lib.hipdrt_map_filter(self._h, C.byref(args), _p(a), _p(res.get("out")), _p(res.get("weights")),
                                           _p(res.get("sigmas"))))
        return res

    def debug_map_filter_stats(self):
        """tools: (kernel launches, full-array reads + writes, device ms) of this context's last map_filter"""
        st = (C.c_double * 3)()
        _check(self._lib.hipdrt_debug_map_filter_stats(self._h, st))
        return int(st[0]), int(st[1]), float(st[2])

    def debug_map_badness_ms(self):
        """tools: device ms of this context's last map_badness"""
        ms = C.c_double()
        _check(self._lib.hipdrt_debug_map_badness_ms(self._h, C.cast(C.byref(ms), _dp)))
        return float(ms.value)

    def rank_filter(self, a, size, rank_lo, rank_hi=None):
        """hipdrt_rank_filter on a 2-D array: rank rank_lo of every size[0] x size[1] window, or (rank_hi given) the difference
        rank_hi - rank_lo of the same window.  A window of more than 49 entries raises NotImplementedError."""
        a = _f64(a)
        if a.ndim != 2:
            raise ValueError("a 2-D array")
        out = np.empty_like(a)
        rc = self._lib.hipdrt_rank_filter(self._h, _p(a), a.shape[0], a.shape[1], int(size[0]), int(size[1]),
                                          RANK_ONE if rank_hi is None else RANK_DIFF, int(rank_lo),
                                          int(rank_lo if rank_hi is None else rank_hi), _p(out))
        if rc == E_UNSUPPORTED:
            raise NotImplementedError(self._lib.hipdrt_last_error().decode())
        _check(rc)
        return out

    def percentiles(self, a, q, by_row=False):
        """hipdrt_percentiles: np.nanpercentile(a, q) over the whole array (out[nq]) or by row of a 2-D one (out[rows, nq]);
        an entry Q_NANMEDIAN of q asks for np.nanmedian"""
        a = _f64(a)
        q = _f64(np.atleast_1d(q))
        rows, cols = (a.shape if (by_row and a.ndim == 2) else (1, a.size))
        out = np.empty((rows, q.size) if by_row else q.size)
        _check(self._lib.hipdrt_percentiles(self._h, _p(a), rows, cols, int(bool(by_row)), _p(q), q.size, _p(out)))
        return out

    def map_badness(self, a, args: MapBadnessArgs, scale_src=None, want_flags=False, want_filt=False):
        """hipdrt_map_badness on a 2-D array; `args` comes filled but for the shape (hipdrt.mapping.nddata builds it).  Returns
        dict(rss=, flags=, filt=); ValueError when x_std contains NaNs, as the reference raises it."""
        a = _f64(a)
        if a.ndim != 2:
            raise ValueError("a 2-D array")
        args.rows, args.cols = a.shape
        if scale_src is not None:
            scale_src = _f64(scale_src)
            if scale_src.shape != a.shape:
                raise ValueError("scale_src must have the shape of a")
        res = {}
        if args.score:
            res["rss"] = np.empty(a.shape[0])
        if want_flags:
            res["flags"] = np.empty(a.shape, dtype=np.uint8)
        if want_filt:
            res["filt"] = np.empty_like(a)
        flags = res["flags"].ctypes.data_as(C.POINTER(C.c_ubyte)) if want_flags else None
        rc = self._lib.hipdrt_map_badness(self._h, C.byref(args), _p(a), _p(scale_src), _p(res.get("rss")), flags, _p(res.get("filt")))
        if rc == E_NUMERIC:
            raise ValueError(self._lib.hipdrt_last_error().decode())
        _check(rc)
        if want_flags:
            res["flags"] = res["flags"].astype(bool)
        return res

    def map_predict(self, x, ln_tau_sup, ln_tau_eval=None, epsilon=1.0, basis_area=1.0, normalize=False, filter_tables=None,
                    f_var=None, fxx_var=None, var_stored=False, ext=None, search=1, height=1e-3, prominence=5e-3, spread_table=None,
                    spread_factor=1.0, want=("x",)):
        """hipdrt_map_predict on the rows x (rows, nsup) of a map (hipdrt.mapping.predict states it in numpy).  filter_tables: None
        or one full symmetric table per axis (psi, tau; None skips the axis); f_var / fxx_var (rows, neval): the caller's variances,
        or with var_stored the raw stored ones, which take the clamp ext (rows, 2) and the filter; spread_table: the full tau table of
        peak_spread_sigma.  want: any of x, f, fxx, f_var, fxx_var, peak_prob, curv_prob -> dict.  An evaluation grid beyond what
        LDS holds raises NotImplementedError."""
        names = ("x", "f", "fxx", "f_var", "fxx_var", "peak_prob", "curv_prob")
        unknown = [w for w in want if w not in names]
        if unknown:
            raise ValueError(f"unknown outputs {unknown}")
        x = _f64(x)
        if x.ndim != 2:
            raise ValueError("x: a 2-D array (rows, nsup)")
        a = MapPredictArgs()
        keep = []

        def table(slot, full):
            slot.radius = -1
            if full is not None:
                r = len(full) // 2
                half = np.ascontiguousarray(np.asarray(full, dtype=np.float64)[r:])
                keep.append(half)
                slot.w, slot.radius = _p(half), r

        a.rows, a.nsup = x.shape
        lts = _f64(ln_tau_sup).ravel()
        if lts.size != x.shape[1]:
            raise ValueError("ln_tau_sup must have one entry per column of x")
        lte = _f64(ln_tau_eval).ravel() if ln_tau_eval is not None else lts
        a.neval, a.ln_tau_sup, a.ln_tau_eval = lte.size, _p(lts), _p(lte)
        a.epsilon, a.basis_area, a.normalize = float(epsilon), float(basis_area), int(bool(normalize))
        tabs = list(filter_tables) if filter_tables is not None else [None, None]
        if len(tabs) != 2:
            raise ValueError("filter_tables: one table per axis (psi, tau)")
        for slot, full in zip(a.x_filter, tabs):
            table(slot, full)
        table(a.spread, spread_table)
        a.spread_factor = float(spread_factor)
        shape = (x.shape[0], lte.size)
        if (f_var is None) != (fxx_var is None):
            raise ValueError("f_var and fxx_var: both or none")
        if f_var is not None:
            f_var, fxx_var = _f64(f_var), _f64(fxx_var)
            if f_var.shape != shape or fxx_var.shape != shape:
                raise ValueError(f"f_var and fxx_var must have the shape {shape}")
            a.f_var, a.fxx_var, a.var_stored = _p(f_var), _p(fxx_var), int(bool(var_stored))
        if ext is not None:
            ext = np.ascontiguousarray(ext, dtype=np.int32)
            if ext.shape != (x.shape[0], 2):
                raise ValueError("ext: (rows, 2)")
            a.ext = _pi(ext)
        a.search, a.height, a.prominence = int(search), float(height), float(prominence)
        res = {w: np.empty(x.shape if w == "x" else shape) for w in names if w in want}
        rc = self._lib.hipdrt_map_predict(self._h, C.byref(a), _p(x), *[_p(res.get(w)) for w in names])
        if rc == E_UNSUPPORTED:
            raise NotImplementedError(self._lib.hipdrt_last_error().decode())
        _check(rc)
        return res

    def penalty_matrices(self, ln_tau, epsilon, toeplitz):
        ln_tau = _f64(ln_tau)
        n = ln_tau.size
        out = [np.empty((n, n)) for _ in range(3)]
        _check(self._lib.hipdrt_penalty_matrices(self._h, _p(ln_tau), n, float(epsilon), int(bool(toeplitz)),
                                                 _p(out[0]), _p(out[1]), _p(out[2])))
        return out

    def eis_var_matrix(self, freq, vmm_epsilon=0.25, reim_cor=0.25, uniform=False):
        freq = _f64(freq)
        vmm = np.empty((2 * freq.size, 2 * freq.size))
        _check(self._lib.hipdrt_eis_var_matrix(self._h, _p(freq), freq.size, float(vmm_epsilon), float(reim_cor),
                                               int(bool(uniform)), _p(vmm)))
        return vmm

    # ---- L2 ------------------------------------------------------------------------------------------
    def qp_batch(self, P, q, h, opts: QpOpts | None = None):
        P, q, h = _f64(P), _f64(q), _f64(h)
        if q.ndim == 1:
            q = q[None, :]
        B, n = q.shape
        p_batched = P.ndim == 3
        h_batched = h.ndim == 2
        x = np.empty((B, n))
        iters = np.empty(B, dtype=np.int32)
        pcost = np.empty(B)
        status = np.empty(B, dtype=np.int32)
        _check(self._lib.hipdrt_qp_batch(self._h, B, n, int(p_batched), _p(P), _p(q), int(h_batched), _p(h),
                                         C.byref(opts) if opts is not None else None, _p(x), _pi(iters), _p(pcost),
                                         _pi(status)))
        return dict(x=x, iterations=iters, pcost=pcost, status=status)

    def fit_eis_batch(self, freq, z, tau, epsilon, wt_re, wt_im, toeplitz_a=False, toeplitz_m=False, opts=None,
                      ny=1000):
        """the one-shot C entry point hipdrt_fit_eis_batch (interp mode): plan create, upload, fit, download, destroy"""
        freq, tau, wt_re, wt_im = _f64(freq), _f64(tau), _f64(wt_re), _f64(wt_im)
        z = np.atleast_2d(np.asarray(z))
        z_re, z_im = _f64(z.real), _f64(z.imag)
        lre, lim = np.log(wt_re), np.log(wt_im)
        opts = opts if opts is not None else default_fit_opts()
        B, nf, ntau = z.shape[0], freq.size, tau.size
        n = ntau + int(opts.fit_ohmic) + int(opts.fit_inductance)
        out = {"x": np.empty((B, n)), "fit_x": np.empty((B, ntau)), "R_inf": np.empty(B), "inductance": np.empty(B),
               "weights": np.empty((B, 2 * nf)), "coefficient_scale": np.empty(B), "rho": np.empty((B, 3)),
               "q_vector": np.empty((B, n)), "outer_iters": np.empty(B, dtype=np.int32),
               "status": np.empty(B, dtype=np.int32)}
        _check(self._lib.hipdrt_fit_eis_batch(self._h, B, _p(freq), nf, _p(z_re), _p(z_im), _p(tau), ntau, float(epsilon),
                                              MODE_INTERP, int(bool(toeplitz_a)), int(bool(toeplitz_m)), wt_re.size,
                                              int(ny), _p(wt_re), _p(wt_im), _p(lre), _p(lim), C.byref(opts),
                                              _p(out["x"]), _p(out["fit_x"]), _p(out["R_inf"]), _p(out["inductance"]),
                                              _p(out["weights"]), _p(out["coefficient_scale"]), _p(out["rho"]),
                                              _p(out["q_vector"]), _pi(out["outer_iters"]), _pi(out["status"])))
        return out

    def device_alloc(self, nbytes):
        """device memory as an integer pointer (hipdrt_device_alloc): for the *_dev entry points; free with device_free"""
        ptr = _vp()
        _check(self._lib.hipdrt_device_alloc(self._h, int(nbytes), C.byref(ptr)))
        return ptr.value

    def device_free(self, ptr):
        _check(self._lib.hipdrt_device_free(self._h, _vp(ptr)))

    def device_synchronize(self):
        """hipDeviceSynchronize on this context's device (every stream, every context of the process on that GPU)"""
        _check(self._lib.hipdrt_device_synchronize(self._h))

    def debug_qp_group(self, members):
        """tests / diagnostics: force the workgroups per problem of this context's coneqp launches sized from now on
        (hipdrt_debug_qp_group, include/hipdrt_debug.h)"""
        _check(self._lib.hipdrt_debug_qp_group(self._h, int(members)))
        self._qp_group_override = int(members)          # (remembered for callers that switch it temporarily: mapping._one_kernel)

    def debug_qp_waves(self, waves):
        """tests / tools: 4 = this context's batch coneqp launches (n <= 528) use the fat four-wavefront kernel, 8 = the
        eight-wavefront one, -1 = the library's choice (hipdrt_debug_qp_waves, include/hipdrt_debug.h)"""
        _check(self._lib.hipdrt_debug_qp_waves(self._h, int(waves)))

    def debug_stream_pool(self):
        """tests: (streams, holders, running) of the library's own streams on this context's device
        (hipdrt_debug_stream_pool, include/hipdrt_debug.h)"""
        size = C.c_int(0)
        _check(self._lib.hipdrt_debug_stream_pool(self._h, 0, None, None, None, C.byref(size)))
        n = size.value
        st, ho, ru = (C.c_void_p * n)(), (C.c_int * n)(), (C.c_int * n)()
        _check(self._lib.hipdrt_debug_stream_pool(self._h, n, st, ho, ru, C.byref(size)))
        return [st[i] for i in range(n)], [ho[i] for i in range(n)], [ru[i] for i in range(n)]

    def debug_exact_zero_shortcuts(self, on):
        """tests: with on = False this context's fits visit the penalty matrices' exact zeros as well (same bits, slower)
        (hipdrt_debug_exact_zero_shortcuts, include/hipdrt_debug.h)"""
        _check(self._lib.hipdrt_debug_exact_zero_shortcuts(self._h, int(bool(on))))

    def debug_gram_l2(self, A, w, y=None, l1=None, l1_scalar=0.0, l2=None, mk=None, s=None, rho=None, dfac=(0.0, 0.0, 0.0),
                      ns=0, sym=False, toep=False, toep_maxd=-1, spec_zero=False, dop_start=0, dop_size=0, dop_rho=None,
                      dop_dfac=(0.0, 0.0, 0.0), active=None, n=None, P=None, Ppk=None, q=None):
        """tests: the fit loop's Gram / q launchers on host arrays (hipdrt_debug_gram_l2, include/hipdrt_debug.h).
        A [m][lda] (shared) or [B][m][lda], w [B][m], y [B][m] or None (no q); `n` = the number of unknowns when A's rows are
        padded (lda = A.shape[-1] > n).  Either l2 ([n][ldl2] or [B][n][ldl2]) or the hyper-parameter form mk (three [n][ldm]
        matrices) + s [B][3][n] (+ rho [B][3]); see GramL2 in csrc/common.hpp for the rest.  P [B][n][ldp], Ppk [B][nchp^2 * 256]
        and q [B][n] are float64 C-contiguous arrays the CALLER fills beforehand (poison): they are uploaded, the kernels
        run, and they are overwritten in place with what the device holds afterwards.  P=None runs the kernel form without the
        row-major copy.  Returns (P, Ppk, q)."""
        A, w = _f64(A), _f64(w)
        B, m = w.shape
        a = DebugGramArgs()
        a.B, a.m, a.lda = B, m, A.shape[-1]
        a.n = n = A.shape[-1] if n is None else int(n)
        a.a_batched = int(A.ndim == 3)
        if A.shape[-2] != m or (A.ndim == 3 and A.shape[0] != B):
            raise ValueError("A does not match w")
        keep = [A, w]

        def arr(v, shape, what):
            if v is None:
                return None
            v = _f64(v)
            if v.shape != tuple(shape):
                raise ValueError(f"{what}: shape {v.shape}, expected {tuple(shape)}")
            keep.append(v)
            return _p(v)

        def out(v, shape, what):
            if v is None:
                return None
            if not (isinstance(v, np.ndarray) and v.dtype == np.float64 and v.flags.c_contiguous and v.flags.writeable):
                raise ValueError(f"{what}: a writeable C-contiguous float64 array")
            if v.shape != tuple(shape):
                raise ValueError(f"{what}: shape {v.shape}, expected {tuple(shape)}")
            return _p(v)

        a.A, a.w = _p(A), _p(w)
        a.y = arr(y, (B, m), "y")
        a.l1 = arr(l1, (n,), "l1")
        a.l1_scalar = float(l1_scalar)
        if s is not None:
            if mk is None or len(mk) != 3 or l2 is not None:
                raise ValueError("hyper-parameter form: three penalty matrices and no explicit l2")
            mk = [_f64(v) for v in mk]
            a.ldm = mk[0].shape[-1]
            for k in range(3):
                a.mk[k] = arr(mk[k], (n, a.ldm), "mk")
            a.s = arr(s, (B, 3, n), "s")
            a.rho = arr(rho, (B, 3), "rho")
            a.dop_rho = arr(dop_rho, (B, 3), "dop_rho")
        elif l2 is not None:
            l2 = _f64(l2)
            a.l2_batched, a.ldl2 = int(l2.ndim == 3), l2.shape[-1]
            a.l2 = arr(l2, ((B, n, a.ldl2) if l2.ndim == 3 else (n, a.ldl2)), "l2")
        for k in range(3):
            a.dfac[k], a.dop_dfac[k] = float(dfac[k]), float(dop_dfac[k])
        a.ns, a.sym, a.toep, a.toep_maxd, a.spec_zero = int(ns), int(bool(sym)), int(bool(toep)), int(toep_maxd), int(bool(spec_zero))
        a.dop_start, a.dop_size = int(dop_start), int(dop_size)
        if active is not None:
            active = np.ascontiguousarray(active, dtype=np.int32)
            if active.shape != (B,):
                raise ValueError("active: one flag per spectrum")
            keep.append(active)
            a.active = _pi(active)
        if P is not None:
            a.ldp = P.shape[-1]
            a.P = out(P, (B, n, a.ldp), "P")
        nchp = (n + 31) // 32 * 2
        a.Ppk = out(Ppk, (B, nchp * nchp * 256), "Ppk")
        a.q = out(q, (B, n), "q")
        _check(self._lib.hipdrt_debug_gram_l2(self._h, C.byref(a)))
        return P, Ppk, q

    def debug_hyper_form(self, n, m, ns, toeplitz=True, outlier=False):
        """tests: (form, lds_bytes) of the LDS layout launch_hyper picks -- 1: Toeplitz columns beside the two m-vectors, 2: inside
        the second one, 0: the general row-streaming form; raises when none fits (hipdrt_debug_hyper_form, include/hipdrt_debug.h)"""
        form, lds = C.c_int(-1), C.c_longlong(0)
        _check(self._lib.hipdrt_debug_hyper_form(self._h, int(n), int(m), int(ns), int(bool(toeplitz)), int(bool(outlier)),
                                                 C.byref(form), C.byref(lds)))
        return form.value, lds.value

    def debug_hyper_step(self, rm, vmm, mk, x, x_in, s, rho, xmx, rv, est_w, w, var_floor, coef_scale, opts: FitOpts, ns=0, n=None,
                         toeplitz=False, toep_reach=-1, qp_status=None, active=None, fit_status=None, outer_iters=None, n_active=0,
                         outlier_t=None, it=0, continue_mode=0, min_iter=1, basis_area=1.0, desc: PreparedDesc | None = None,
                         dop_rho=None, dop_xmx=None, vz_strength=None, vz_entry=None, products=0):
        """tests: one hyper-parameter step (launch_hyper as it is) on host arrays (hipdrt_debug_hyper_step, include/hipdrt_debug.h).
        rm [m][ldrm] (shared) or [B][m][ldrm], vmm [m][m], mk three [n][ldm]; `n` = the number of unknowns when the rows of rm are
        padded.  x [B][n] is the QP's result; the other per-spectrum arrays are the state BEFORE the step (poison where the step is
        to write without reading).  Nothing passed in is modified.  Returns a dict of the state AFTER the step: s, rho, xmx, dop_rho,
        dop_xmx, w, x_in, outlier_t, active, fit_status, outer_iters, n_active, rv, est_w, coef_scale, var_floor, rm_col."""
        rm, vmm, x = _f64(rm), _f64(vmm), _f64(x)
        B = x.shape[0]
        m = vmm.shape[0]
        a = DebugHyperArgs()
        a.B, a.m, a.ldrm = B, m, rm.shape[-1]
        a.n = n = x.shape[1] if n is None else int(n)
        a.ns, a.rm_batched = int(ns), int(rm.ndim == 3)
        if rm.shape[-2] != m or (rm.ndim == 3 and rm.shape[0] != B) or vmm.shape != (m, m) or x.shape != (B, n):
            raise ValueError("rm, vmm and x do not match")
        mk = [_f64(v) for v in mk]
        if len(mk) != 3 or any(v.shape != (n, mk[0].shape[-1]) for v in mk):
            raise ValueError("mk: three [n][ldm] matrices")
        a.ldm = mk[0].shape[-1]
        keep = [rm, vmm, x] + mk
        a.rm, a.vmm, a.x = _p(rm), _p(vmm), _p(x)
        for k in range(3):
            a.mk[k] = _p(mk[k])
        a.toeplitz, a.toep_reach = int(bool(toeplitz)), int(toep_reach)
        out = {}

        def state(name, v, shape, dtype=np.float64, required=True):
            if v is None:
                if required:
                    raise ValueError(f"{name} is required")
                return None
            v = np.array(v, dtype=dtype, order="C")           # a copy: the caller's array stays as it is
            if v.shape != tuple(shape):
                raise ValueError(f"{name}: shape {v.shape}, expected {tuple(shape)}")
            out[name] = v
            return _p(v) if dtype == np.float64 else _pi(v)

        a.x_in = state("x_in", x_in, (B, n))
        a.s = state("s", s, (B, 3, n))
        a.rho, a.xmx = state("rho", rho, (B, 3)), state("xmx", xmx, (B, 3))
        a.rv, a.est_w, a.w = state("rv", rv, (B, m)), state("est_w", est_w, (B, m)), state("w", w, (B, m))
        a.var_floor, a.coef_scale = state("var_floor", var_floor, (B,)), state("coef_scale", coef_scale, (B,))
        qs = np.ascontiguousarray(np.zeros(B) if qp_status is None else qp_status, dtype=np.int32)
        if qs.shape != (B,):
            raise ValueError("qp_status: one per spectrum")
        keep.append(qs)
        a.qp_status = _pi(qs)
        a.active = state("active", np.ones(B) if active is None else active, (B,), np.int32)
        a.fit_status = state("fit_status", np.full(B, -77) if fit_status is None else fit_status, (B,), np.int32)
        a.outer_iters = state("outer_iters", np.full(B, -77) if outer_iters is None else outer_iters, (B,), np.int32)
        a.n_active = state("n_active", np.array([n_active]), (1,), np.int32)
        a.outlier_t = state("outlier_t", outlier_t, (B, m), required=False)
        a.opts = C.pointer(opts)
        a.it, a.continue_mode, a.min_iter, a.basis_area = int(it), int(continue_mode), int(min_iter), float(basis_area)
        a.products = int(products)
        if desc is not None:
            a.desc = C.pointer(desc)
            a.dop_rho, a.dop_xmx = state("dop_rho", dop_rho, (B, 3)), state("dop_xmx", dop_xmx, (B, 3))
            if desc.vz_index >= 0:
                vs = _f64(vz_strength)
                if vs.shape != (m,):
                    raise ValueError("vz_strength: [m]")
                keep.append(vs)
                a.vz_strength = _p(vs)
                a.rm_col = state("rm_col", np.full((B if rm.ndim == 3 else 1, m), np.nan), (B if rm.ndim == 3 else 1, m))
        if vz_entry is not None:
            ve = _f64(vz_entry)
            if ve.shape != (B, m):
                raise ValueError("vz_entry: [B][m]")
            keep.append(ve)
            a.vz_entry = _p(ve)
        _check(self._lib.hipdrt_debug_hyper_step(self._h, C.byref(a)))
        out["n_active"] = int(out["n_active"][0])
        return out

    def debug_kk_stats(self, freq, err, opts: KkOpts | None = None):
        """tests: the statistics stage of the KK screen kernel on host residuals err (B, nf) complex
        (hipdrt_debug_kk_stats, include/hipdrt_debug.h) -> dict(std, outlier_mask, f_lim, i_lim, status)"""
        freq = _f64(freq)
        err = np.atleast_2d(np.asarray(err, dtype=complex))
        if err.shape[1] != freq.size:
            raise ValueError("err must have shape (B, len(freq))")
        e_re, e_im = _f64(err.real), _f64(err.imag)
        out = _kk_outputs(err.shape[0], freq.size)
        _check(self._lib.hipdrt_debug_kk_stats(self._h, err.shape[0], freq.size, _p(freq), _p(e_re), _p(e_im),
                                               C.byref(opts) if opts is not None else None, _p(out["std"]),
                                               _pi(out["outlier_mask"]), _p(out["f_lim"]), _pi(out["i_lim"]),
                                               _pi(out["status"])))
        return out

    def func_eval_matrix(self, basis_grid, eval_grid, epsilon, order=0):
        """hipdrt_func_eval_matrix: E[i, j] = phi^(order)(eval_i - basis_j; epsilon) of the gaussian basis, orders 0-2, on the
        device (natural-log grids) -> (len(eval_grid), len(basis_grid))"""
        basis_grid, eval_grid = _f64(basis_grid).ravel(), _f64(eval_grid).ravel()
        out = np.empty((eval_grid.size, basis_grid.size))
        _check(self._lib.hipdrt_func_eval_matrix(self._h, _p(basis_grid), basis_grid.size, _p(eval_grid), eval_grid.size,
                                                 float(epsilon), int(order), _p(out)))
        return out

    def debug_apply_rows(self, X, E, col_offset=0, scale=None):
        """tests: the row-application kernel of the predictions on host arrays (hipdrt_debug_apply_rows, include/hipdrt_debug.h):
        out[b, i] = scale[b] * sum_j E[i, j] X[b, col_offset + j]; X (B, ldx), E (r, K).  Raises when the kernel wrote outside
        its B x r block of the padded device output."""
        X, E = _f64(X), _f64(E)
        B, ldx = X.shape
        r, K = E.shape
        sc = None if scale is None else _f64(scale)
        if sc is not None and sc.shape != (B,):
            raise ValueError("scale must have shape (B,)")
        out = np.empty((B, r))
        _check(self._lib.hipdrt_debug_apply_rows(self._h, B, K, ldx, int(col_offset), _p(X), r, _p(E), _p(sc), _p(out)))
        return out

    def debug_response(self, X, ns, step_sizes, coefficient_scale, U=None, Ud=None, dop_start=0, copies=1, idx_rinf=-1,
                       idx_cinv=-1, vz_index=-1, vb_start=0, capacitance_scale=1.0, response_signal_scale=None,
                       scaled_response_offset=None, inf_rv=None, cap_rv=None, vz_strength=None, vb_mat=None,
                       v_baseline_scale=None, fit_status=None, include_mask=INCLUDE_ALL, nt=None, dop_scale_vector=None):
        """tests: the device chain of hipdrt_plan_predict_response behind its layer builders, on host arrays
        (hipdrt_debug_response, include/hipdrt_debug.h) -> (B, nt).  X (B, n); U (S, nt, ntau) unit-step layers; Ud (S, nt, dop_size)
        unit phasor layers, dop_scale_vector (B, dop_size) or None; step_sizes (S,) or (B, S); inf_rv / cap_rv (nt,) or (B, nt).  Raises when the kernel
        wrote outside its output."""
        a, keep = DebugResponseArgs(), []

        def arr(name, v, dtype=np.float64):
            if v is not None:
                v = np.ascontiguousarray(v, dtype=dtype)
                keep.append(v)
                setattr(a, name, v.ctypes.data_as(_ip if dtype == np.int32 else _dp))
            return v
        X = arr('X', X)
        sz = arr('step_sizes', step_sizes)
        U, Ud = arr('U', U), arr('Ud', Ud)
        a.B, a.n = X.shape
        a.S = sz.shape[-1]
        a.sizes_batched = int(sz.ndim == 2)
        layers = U if U is not None else Ud
        a.nt = int(nt) if layers is None else layers.shape[1]
        a.ntau = U.shape[2] if U is not None else 1
        a.copies, a.ns = int(copies), int(ns)
        a.dop_start, a.dop_size = int(dop_start), (Ud.shape[2] if Ud is not None else 0)
        dsv = arr('dop_scale_vector', dop_scale_vector)
        if dsv is not None and dsv.shape != (a.B, a.dop_size):
            raise ValueError("dop_scale_vector must have shape (B, dop_size)")
        for name, v in (('coefficient_scale', coefficient_scale), ('response_signal_scale', response_signal_scale),
                        ('scaled_response_offset', scaled_response_offset)):
            v = arr(name, v)
            if v is not None and v.shape != (a.B,):
                raise ValueError(f"{name} must have shape (B,)")
        a.idx_rinf, a.idx_cinv, a.vz_index, a.vb_start = int(idx_rinf), int(idx_cinv), int(vz_index), int(vb_start)
        a.capacitance_scale = float(capacitance_scale)
        for name, v in (('inf_rv', inf_rv), ('cap_rv', cap_rv)):
            v = arr(name, v)
            if v is not None:
                if v.shape not in ((a.nt,), (a.B, a.nt)):
                    raise ValueError(f"{name} must have shape (nt,) or (B, nt)")
                setattr(a, name[:3] + '_batched', int(v.ndim == 2))
        vs = arr('vz_strength', vz_strength)
        if vs is not None and vs.shape != (a.nt,):
            raise ValueError("vz_strength must have shape (nt,)")
        vb, vbs = arr('vb_mat', vb_mat), arr('v_baseline_scale', v_baseline_scale)
        a.vb_size = 0 if vb is None else vb.shape[1]
        if vb is not None and (vb.shape[0] != a.nt or vbs is None or vbs.shape != (a.vb_size,)):
            raise ValueError("vb_mat must have shape (nt, vb_size) and v_baseline_scale (vb_size,)")
        for name, v in (('U', U), ('Ud', Ud)):
            if v is not None and v.shape[:2] != (a.S, a.nt):
                raise ValueError(f"{name} must have shape (S, nt, columns)")
        fs = arr('fit_status', fit_status, np.int32)
        if fs is not None and fs.shape != (a.B,):
            raise ValueError("fit_status must have shape (B,)")
        a.include_mask = int(include_mask)
        out = arr('out', np.empty((a.B, a.nt)))
        _check(self._lib.hipdrt_debug_response(self._h, C.byref(a)))
        return out

    def debug_find_peaks(self, fxx, f=None, var_fxx=None, var_f=None, opts: PeakOpts | None = None):
        """tests: peaks_kernel on host rows (B, neval) (hipdrt_debug_find_peaks, include/hipdrt_debug.h) -> dict(peak_sign, keep,
        heights, prominences, probs, left_bases, right_bases, count, used_prominence[, peak_prob, curv_prob]).  Raises when the
        kernel wrote outside an output."""
        rows = [None if r is None else np.atleast_2d(_f64(r)) for r in (fxx, f, var_fxx, var_f)]
        B, n = rows[0].shape
        if any(r is not None and r.shape != (B, n) for r in rows):
            raise ValueError("all rows must have the shape of fxx")
        opts = opts if opts is not None else peak_opts()
        out = _peak_outputs(B, n, opts.method)
        _check(self._lib.hipdrt_debug_find_peaks(self._h, B, n, *[_p(r) for r in rows], C.byref(opts), *_peak_out_args(out)))
        return out

    def debug_peak_resolve(self, f, fxx, x, ln_tau_find, ln_basis, ln_tau_out=None, basis_eps=1.0, keep=None, indices=None,
                           windows=None, copies=1, fit_status=None, opts: PeakResolveOpts | None = None, want=None):
        """tests: peak_resolve_kernel on host arrays (hipdrt_debug_peak_resolve, include/hipdrt_debug.h): rows f, fxx (B, nfind),
        x (B, copies * nb) in data units, the peak source keep (B, nfind) / indices (B, max_peaks) / windows (start, end) ->
        dict of the padded outputs of hipdrt_plan_resolve_peaks plus lds_bytes.  Raises when the kernel wrote outside an output."""
        f, fxx, x = np.atleast_2d(_f64(f)), np.atleast_2d(_f64(fxx)), np.atleast_2d(_f64(x))
        lt, lb = _f64(ln_tau_find).ravel(), _f64(ln_basis).ravel()
        lo = None if ln_tau_out is None else _f64(ln_tau_out).ravel()
        B, nfind = f.shape
        nb, nout = lb.size, 0 if lo is None else lo.size
        if fxx.shape != f.shape or lt.size != nfind or x.shape != (B, copies * nb):
            raise ValueError("shapes: f, fxx (B, nfind); x (B, copies * nb)")
        opts = opts if opts is not None else peak_resolve_opts()
        a = DebugPeakResolveArgs()
        a.B, a.nfind, a.nb, a.nout, a.copies = B, nfind, nb, nout, int(copies)
        keepers = [f, fxx, x, lt, lb, lo]
        a.f, a.fxx, a.x, a.ln_tau_find, a.ln_basis, a.ln_tau_out, a.basis_eps = _p(f), _p(fxx), _p(x), _p(lt), _p(lb), _p(lo), float(basis_eps)
        if keep is not None:
            k = np.atleast_2d(_i32(keep)); keepers.append(k)
            if k.shape != f.shape:
                raise ValueError("keep must have the shape of f")
            a.source, a.keep = PEAKS_FROM_FIND, _pi(k)
        elif indices is not None:
            k = np.atleast_2d(_i32(indices)); keepers.append(k)
            if k.shape != (B, opts.max_peaks):
                raise ValueError("indices must have shape (B, max_peaks)")
            a.source, a.indices = PEAKS_FROM_INDICES, _pi(k)
        else:
            ws, we = _i32(windows[0]).ravel(), _i32(windows[1]).ravel(); keepers += [ws, we]
            a.source, a.win_start, a.win_end, a.nwin = PEAKS_FROM_WINDOWS, _pi(ws), _pi(we), ws.size
        if fit_status is not None:
            fs = _i32(fit_status); keepers.append(fs)
            a.fit_status = _pi(fs)
        a.opts = C.pointer(opts)
        out = _resolve_outputs(B, opts.max_peaks, nb, nout, want)
        a.out = _resolve_out_struct(out)
        lds = C.c_longlong(-1)
        a.lds_bytes = C.pointer(lds)
        try:
            _check(self._lib.hipdrt_debug_peak_resolve(self._h, C.byref(a)))
        finally:
            self.last_peak_resolve_lds = int(lds.value)
        out["lds_bytes"] = int(lds.value)
        return out

    def debug_pfrt_step(self, peak_sign, heights, prominences, f, var_f, var_fxx, var_floor=1e-5, ext_left=-1, ext_right=-1):
        """tests: pfrt_step_kernel on host rows (B, neval) (hipdrt_debug_pfrt_step, include/hipdrt_debug.h) -> (B, neval).  Raises
        when the kernel wrote outside its output."""
        sg = np.atleast_2d(_i32(peak_sign))
        rows = [np.atleast_2d(_f64(r)) for r in (heights, prominences, f, var_f, var_fxx)]
        B, n = sg.shape
        if any(r.shape != (B, n) for r in rows):
            raise ValueError("all rows must have the shape of peak_sign")
        out = np.full((B, n), 7e77)
        _check(self._lib.hipdrt_debug_pfrt_step(self._h, B, n, _pi(sg), *[_p(r) for r in rows], float(var_floor), int(ext_left),
                                                int(ext_right), _p(out)))
        return out

    def debug_pfrt_combine(self, step_pfrt, rss, sum_log_w, factors, m, ln_tau_pfrt, ln_tau_out=None, opts: PfrtOpts | None = None):
        """tests: pfrt_combine_kernel on host arrays (hipdrt_debug_pfrt_combine): step_pfrt (S, B, np), rss and sum_log_w (S, B),
        factors (S,) -> dict(pfrt (B, nout), raw_pfrt (B, np), post_prob (S, B)).  Raises when the kernel wrote outside an output."""
        sp, rss, slw, fac = _f64(step_pfrt), _f64(rss), _f64(sum_log_w), _f64(factors).ravel()
        S, B, npf = sp.shape
        if rss.shape != (S, B) or slw.shape != (S, B) or fac.size != S:
            raise ValueError("shapes: step_pfrt (S, B, np); rss, sum_log_w (S, B); factors (S,)")
        opts = opts if opts is not None else pfrt_opts()
        ltp = _f64(ln_tau_pfrt).ravel()
        lto = None if ln_tau_out is None else _f64(ln_tau_out).ravel()
        nout = npf if lto is None else lto.size
        if ltp.size != npf:
            raise ValueError("ln_tau_pfrt must have np points")
        out = dict(pfrt=np.full((B, nout), 7e77), raw_pfrt=np.full((B, npf), 7e77), post_prob=np.full((S, B), 7e77))
        _check(self._lib.hipdrt_debug_pfrt_combine(self._h, B, S, npf, nout, _p(sp), _p(rss), _p(slw), _p(fac), int(m), C.byref(opts),
                                                   _p(ltp), _p(lto), _p(out["pfrt"]), _p(out["raw_pfrt"]), _p(out["post_prob"])))
        return out

    def debug_candidate_llh(self, x, rm, rv, vmm, var_floor):
        """tests: the likelihood kernels of csrc/candidates.hip on host arrays (hipdrt_debug_candidate_llh): x (C, B, n), rm (m, n)
        or (B, m, n), rv (B, m), vmm (m, m), var_floor (B,) -> (rss, sum_log_w), each (C, B).  Raises when a kernel wrote outside
        an output."""
        x, rm, rv, vmm, vf = _f64(x), _f64(rm), _f64(rv), _f64(vmm), _f64(var_floor).ravel()
        Cn, B, n = x.shape
        m = rv.shape[1]
        if rm.shape not in ((m, n), (B, m, n)) or rv.shape != (B, m) or vmm.shape != (m, m) or vf.shape != (B,):
            raise ValueError("shapes: x (C, B, n); rm (m, n) or (B, m, n); rv (B, m); vmm (m, m); var_floor (B,)")
        rss, slw = np.full((Cn, B), 7e77), np.full((Cn, B), 7e77)
        _check(self._lib.hipdrt_debug_candidate_llh(self._h, Cn, B, m, n, _p(rm), int(rm.ndim == 3), _p(rv), _p(vmm), _p(vf), _p(x),
                                                    _p(rss), _p(slw)))
        return rss, slw

    def debug_posterior(self, P, rows, col_offset=0, B=None, scale=None, cov_member=-1, n=None, want=("var", "status")):
        """tests: the posterior variance and covariance chain on host arrays (hipdrt_debug_posterior, include/hipdrt_debug.h):
        P (n, ldp) shared by B spectra or (B, n, ldp), rows (neval, ncol) at unknowns col_offset.., scale (B,) or None ->
        dict of the outputs named in `want`: var (nb, neval), status (nb,), cov (neval, neval), bex (nex, nchp, 256),
        tail (nb, nex, nchp, 256); nb = B, or 1 with cov_member >= 0.  Raises when a kernel wrote outside an output or outside a
        spectrum's factor scratch."""
        P, rows = _f64(P), np.atleast_2d(_f64(rows))
        batched = P.ndim == 3
        B = (P.shape[0] if batched else 1) if B is None else int(B)
        n = P.shape[-2] if n is None else int(n)
        if P.ndim not in (2, 3) or P.shape[-2] != n or (batched and P.shape[0] != B):
            raise ValueError("P: (n, ldp) or (B, n, ldp)")
        neval, ncol = rows.shape
        sc = None if scale is None else _f64(scale).ravel()
        if sc is not None and sc.size != B:
            raise ValueError("scale: (B,)")
        nb = 1 if cov_member >= 0 else max(B, 0)
        nex, nchp = max((neval + 15) // 16, 0), (max(n, 0) + 31) // 32 * 2
        shapes = dict(var=(nb, neval), status=(nb,), cov=(neval, neval), bex=(nex, nchp, 256), tail=(nb, nex, nchp, 256))
        out = {k: (np.full(shapes[k], -7, dtype=np.int32) if k == "status" else np.full(shapes[k], 7e77)) for k in want}
        a = DebugPosteriorArgs()
        a.B, a.n, a.P, a.p_batched, a.ldp = B, n, _p(P), int(batched), P.shape[-1]
        a.rows, a.neval, a.ncol, a.col_offset, a.scale, a.cov_member = _p(rows), neval, ncol, int(col_offset), _p(sc), int(cov_member)
        for k in want:
            setattr(a, k, _pi(out[k]) if k == "status" else _p(out[k]))
        _check(self._lib.hipdrt_debug_posterior(self._h, C.byref(a)))
        return out

    def debug_qp(self, P, q, h, opts: QpOpts | None = None, active=None, order=None, use_lpt=False, x=None, iters=None, pcost=None,
                 status=None, iters_accum=None):
        """tests: launch_qp in the fit loop's form on host arrays (hipdrt_debug_qp, include/hipdrt_debug.h): P (n, ldp) shared or
        (B, n, ldp), q (B, n), h (n,) or (B, n).  x, iters, pcost, status, iters_accum are what the in/out arrays hold before the launch
        (sentinels by default; they are copied, not changed) -> dict with x, iterations, pcost, status, iters_accum, s, z (NaN rows
        for inactive problems), order (the table the kernel used), form (G, inverse blocks in global memory, wavefronts).  Raises when
        a kernel wrote outside an array, a problem's state block or factor scratch, or the sync words."""
        P, q, h = _f64(P), np.atleast_2d(_f64(q)), _f64(h)
        B, n = q.shape
        if P.ndim not in (2, 3) or P.shape[-2] != n or (P.ndim == 3 and P.shape[0] != B) or h.shape not in ((n,), (B, n)):
            raise ValueError("P: (n, ldp) or (B, n, ldp); q: (B, n); h: (n,) or (B, n)")

        def inout(v, shape, dtype, fill):
            out = np.full(shape, fill, dtype=dtype)
            if v is not None:
                out[...] = v
            return out
        out = dict(x=inout(x, (B, n), np.float64, 7e77), iterations=inout(iters, B, np.int32, -7), pcost=inout(pcost, B, np.float64, 7e77),
                   status=inout(status, B, np.int32, -7), iters_accum=inout(iters_accum, B, np.int32, 0),
                   s=np.full((B, n), np.nan), z=np.full((B, n), np.nan), order=np.full(B, -7, dtype=np.int32),
                   form=np.full(3, -7, dtype=np.int32))
        act = None if active is None else _i32(active).ravel()
        order_in = None if order is None else _i32(order).ravel()
        if (act is not None and act.size != B) or (order_in is not None and order_in.size != B):
            raise ValueError("active, order: (B,)")
        a = DebugQpArgs()
        a.B, a.n, a.P, a.p_batched, a.ldp, a.q, a.h, a.h_batched = B, n, _p(P), int(P.ndim == 3), P.shape[-1], _p(q), _p(h), int(h.ndim == 2)
        a.opts = C.pointer(opts) if opts is not None else None
        a.active, a.order, a.use_lpt, a.form = _pi(act), _pi(order_in), int(bool(use_lpt)), _pi(out["form"])
        a.x, a.iters, a.pcost, a.status, a.iters_accum = (_p(out["x"]), _pi(out["iterations"]), _p(out["pcost"]), _pi(out["status"]),
                                                          _pi(out["iters_accum"]))
        a.s, a.z, a.order_out = _p(out["s"]), _p(out["z"]), _pi(out["order"])
        _check(self._lib.hipdrt_debug_qp(self._h, C.byref(a)))
        return out

    def debug_lpt_order(self, iters, active=None):
        """tests: lpt_order_kernel alone (hipdrt_debug_lpt_order, include/hipdrt_debug.h) -> order (B,), -7 where the kernel wrote nothing"""
        iters = _i32(iters).ravel()
        act = None if active is None else _i32(active).ravel()
        order = np.full(iters.size, -7, dtype=np.int32)
        _check(self._lib.hipdrt_debug_lpt_order(self._h, iters.size, _pi(iters), _pi(act), _pi(order)))
        return order

    def debug_map_gaussian(self, a, tables, masked=False):
        """tests: plain_gaussian_device / masked_gaussian_device (csrc/map_filter.hip) on a 2-D host array
        (hipdrt_debug_map_gaussian, include/hipdrt_debug.h); tables: one full symmetric table per axis, None skips the axis;
        masked: the NaNs of `a` are the mask.  Entries no kernel wrote come back as -7e77."""
        a = _f64(a)
        if a.ndim != 2 or len(tables) != 2:
            raise ValueError("a 2-D array and one table (or None) per axis")
        tabs, keep = (FilterTable * 2)(), []
        for slot, full in zip(tabs, tables):
            slot.radius = -1
            if full is not None:
                r = len(full) // 2
                keep.append(np.ascontiguousarray(np.asarray(full, dtype=np.float64)[r:]))
                slot.w, slot.radius = _p(keep[-1]), r
        out = np.full(a.shape, -7.0e77)
        _check(self._lib.hipdrt_debug_map_gaussian(self._h, _p(a), a.shape[0], a.shape[1], tabs, int(bool(masked)), _p(out)))
        return out

    def debug_map_reduce(self, x, mode):
        """tests: the fixed-order reductions of csrc/map_filter.hip alone (hipdrt_debug_map_reduce) on a host vector ->
        mode 0: (mean, 0), 1: (np.std, the mean it was taken about), 2: (min, max)"""
        x = _f64(x).ravel()
        out = np.full(2, -7.0e77)
        _check(self._lib.hipdrt_debug_map_reduce(self._h, _p(x), x.size, int(mode), _p(out)))
        return float(out[0]), float(out[1])

    def debug_map_prob(self, f, fxx, f_var, fxx_var, ext=None, clamp_first=False, search=1, height=1e-3, prominence=5e-3,
                       sign_now=True, want=("pk", "curv", "f_var", "fxx_var")):
        """tests: clamp_kernel and / or map_prob_kernel (csrc/map_predict.hip) as stage 3 of hipdrt_map_predict launches them, on
        host rows (rows, n) (hipdrt_debug_map_prob, include/hipdrt_debug.h) -> dict of the rows in `want`; entries no kernel wrote
        come back as -7e77.  A grid beyond what LDS holds raises NotImplementedError, as Context.map_predict does."""
        names = ("pk", "curv", "f_var", "fxx_var")
        unknown = [w for w in want if w not in names]
        if unknown:
            raise ValueError(f"unknown outputs {unknown}")
        f_var, fxx_var = _f64(f_var), _f64(fxx_var)
        shape = f_var.shape
        f, fxx = (None if r is None else _f64(r) for r in (f, fxx))
        if len(shape) != 2 or any(r is not None and r.shape != shape for r in (f, fxx, fxx_var)):
            raise ValueError("f, fxx, f_var, fxx_var: 2-D arrays of one shape (rows, n)")
        if ext is not None:
            ext = np.ascontiguousarray(ext, dtype=np.int32)
            if ext.shape != (shape[0], 2):
                raise ValueError("ext: (rows, 2)")
        res = {w: np.full(shape, -7.0e77) for w in names if w in want}
        rc = self._lib.hipdrt_debug_map_prob(self._h, shape[0], shape[1], _p(f), _p(fxx), _p(f_var), _p(fxx_var), _pi(ext),
                                             int(bool(clamp_first)), int(search), float(height), float(prominence),
                                             int(bool(sign_now)), *[_p(res.get(w)) for w in names])
        if rc == E_UNSUPPORTED:
            raise NotImplementedError(self._lib.hipdrt_last_error().decode())
        _check(rc)
        return res

    def debug_candidate_form(self, form):
        """tests: how candidate scoring on this context keeps rm x between its two products: 0 LDS, 1 scratch, -1 automatic"""
        _check(self._lib.hipdrt_debug_candidate_form(self._h, int(form)))

    def debug_last_predict_ms(self):
        """tools: kernel time in ms of the last predict_drt / predict_z of a plan of this context -> (mean or impedance, with band)"""
        ms = (C.c_float * 2)()
        _check(self._lib.hipdrt_debug_last_predict_ms(self._h, ms))
        return float(ms[0]), float(ms[1])

    def debug_pack_p(self, P, n=None):
        """tests: launch_pack_p on row-major symmetric P [B][n][ldp] -> Ppk [B][nchp^2 * 256]; slots the kernel does not write
        come back as NaN (hipdrt_debug_pack_p, include/hipdrt_debug.h)"""
        P = _f64(P)
        B, rows, ldp = P.shape
        n = rows if n is None else int(n)
        if rows != n:
            raise ValueError("P: [B][n][ldp]")
        nchp = (n + 31) // 32 * 2
        Ppk = np.full((B, nchp * nchp * 256), np.nan)
        _check(self._lib.hipdrt_debug_pack_p(self._h, B, n, _p(P), ldp, _p(Ppk)))
        return Ppk

    def qp_profile(self, reset=True):
        buf = (C.c_ulonglong * 64)()        # 0..47 the QP kernel's phases, 48..63 hyper_kernel's (PROFILE=1 builds)
        _check(self._lib.hipdrt_qp_profile(self._h, buf, 64, int(reset)))
        return [int(v) for v in buf]

    def qp_timeline(self):
        """PROFILE builds: s_memtime stamps [wavefront 8][super column 16][stamp 8] of workgroup 0's last factorisation
        (csrc/qp_common.hpp, g_qp_tl); zeros otherwise"""
        n = 64 + 8 * 16 * 8
        buf = (C.c_ulonglong * n)()
        _check(self._lib.hipdrt_qp_profile(self._h, buf, n, 0))
        return np.array(buf[64:], dtype=np.uint64).reshape(8, 16, 8)

    def qp_timeline_mean(self, reset=True):
        """PROFILE builds: the same stamps as mean cycles since the start of the factorisation, over all factorisations of
        workgroup 0 since the last reset -> (array [8][16][8], number of factorisations)"""
        nt = 8 * 16 * 8
        n = 64 + 2 * nt + 1
        buf = (C.c_ulonglong * n)()
        _check(self._lib.hipdrt_qp_profile(self._h, buf, n, int(reset)))
        cnt = int(buf[64 + 2 * nt])
        return np.array(buf[64 + nt:64 + 2 * nt], dtype=np.float64).reshape(8, 16, 8) / max(cnt, 1), cnt

    def weighted_gram(self, A, w, b, l2=None, l1=None):
        A, w, b = _f64(A), _f64(w), _f64(b)
        if w.ndim == 1:
            w, b = w[None, :], b[None, :]
        B, m = w.shape
        n = A.shape[1]
        l2a = None if l2 is None else _f64(l2)
        l1a = None if l1 is None else _f64(l1)
        P = np.empty((B, n, n))
        q = np.empty((B, n))
        _check(self._lib.hipdrt_weighted_gram(self._h, B, m, n, _p(A), _p(w), _p(b),
                                              int(l2a is not None and l2a.ndim == 3), _p(l2a), _p(l1a), _p(P), _p(q)))
        return P, q


class Plan:
    """hipdrt_plan: shared matrices + work space for `capacity` spectra on one frequency / tau grid."""

    def __init__(self, ctx: Context, freq, tau, epsilon, wt_re=None, wt_im=None, mode=MODE_INTERP,
                 toeplitz_a=False, toeplitz_m=False, opts: FitOpts | None = None, capacity=1, ny=1000):
        self._lib = load_library()
        self.ctx = ctx
        freq, tau = _f64(freq), _f64(tau)
        self.freq, self.tau = freq, tau
        if mode == MODE_INTERP:
            wt_re, wt_im = _f64(wt_re), _f64(wt_im)
            lre, lim = np.log(wt_re), np.log(wt_im)
            ng = wt_re.size
        else:
            wt_re = wt_im = lre = lim = None
            ng = 0
        self.log_wt_re, self.log_wt_im = lre, lim
        self.opts = opts if opts is not None else default_fit_opts()
        h = _vp()
        _check(self._lib.hipdrt_plan_create(ctx._h, _p(freq), freq.size, _p(tau), tau.size, float(epsilon), int(mode),
                                            int(bool(toeplitz_a)), int(bool(toeplitz_m)), ng, int(ny), _p(wt_re),
                                            _p(wt_im), _p(lre), _p(lim), C.byref(self.opts), int(capacity),
                                            C.byref(h)))
        self._h = h
        if os.environ.get("HIPDRT_SUBBATCHES"):           # tools / A-B runs
            self.set_subbatches(int(os.environ["HIPDRT_SUBBATCHES"]))
        n, m, ns = C.c_int(), C.c_int(), C.c_int()
        _check(self._lib.hipdrt_plan_dims(self._h, C.byref(n), C.byref(m), C.byref(ns)))
        self.n, self.m, self.ns = n.value, m.value, ns.value
        self.nf, self.ntau, self.ngrid = freq.size, tau.size, ng
        self.capacity = int(capacity)
        self.B = 0

    def close(self):
        if getattr(self, "_h", None):
            self._lib.hipdrt_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def get(self, which):
        shapes = {"lut_z_re": (self.ngrid,), "lut_z_im": (self.ngrid,), "a_re": (self.nf, self.ntau),
                  "a_im": (self.nf, self.ntau), "rm": (self.m, self.n), "m0": (self.n, self.n),
                  "m1": (self.n, self.n), "m2": (self.n, self.n), "vmm": (self.m, self.m), "h": (self.n,),
                  "est_weights": (self.batch, self.m), "rv": (self.batch, self.m), "xmx": (self.batch, 3),
                  "outlier_t": (self.batch, self.m), "row_factors": (self.batch, self.m), "x": (self.batch, self.n),
                  "coef_scale": (self.batch,), "var_floor": (self.batch,)}
        out = np.empty(shapes[which])
        _check(self._lib.hipdrt_plan_get(self._h, which.encode(), _p(out), out.size))
        return out

    def set_lookup(self, z_re, z_im):
        z_re, z_im = _f64(z_re), _f64(z_im)
        _check(self._lib.hipdrt_plan_set_lookup(self._h, _p(z_re), _p(z_im)))

    batch = 0      # spectra of the last upload

    def upload(self, z):
        z = np.asarray(z)
        if z.ndim == 1:
            z = z[None, :]
        z_re, z_im = _f64(z.real), _f64(z.imag)
        _check(self._lib.hipdrt_plan_upload(self._h, z.shape[0], _p(z_re), _p(z_im)))
        self.batch = z.shape[0]
        self.B = z.shape[0]

    def fit(self):
        _check(self._lib.hipdrt_plan_fit(self._h))

    def set_subbatches(self, k):
        """ranges the staged batch is fitted in, side by side inside one fit() call (hipdrt_plan_set_subbatches): 0 = the
        library chooses from the batch size (default; env HIPDRT_SUBBATCHES overrides at plan creation), 1 = one launch sequence"""
        _check(self._lib.hipdrt_plan_set_subbatches(self._h, int(k)))

    def llh_terms(self, stored=False, weights=None):
        """(rss, sum(log w)) per spectrum; stored=False: weights re-estimated from the current x (PFRT steps),
        stored=True: the `weights` argument of DRT.evaluate_rss() / evaluate_llh(): None = the fit's own est_weights,
        'uniform' = per-domain means of them (DRTMD's default), a positive scalar = that weight for every row."""
        rss, slw = np.empty(self.batch), np.empty(self.batch)
        if not stored:
            _check(self._lib.hipdrt_plan_llh_terms(self._h, _p(rss), _p(slw)))
        elif weights is None:
            _check(self._lib.hipdrt_plan_obs_llh_terms(self._h, _p(rss), _p(slw)))
        elif isinstance(weights, str):
            if weights != 'uniform':
                raise ValueError(f"weights must be None, 'uniform' or a scalar, got {weights!r}")
            _check(self._lib.hipdrt_plan_obs_llh_terms_w(self._h, 2, 1.0, _p(rss), _p(slw)))
        else:
            _check(self._lib.hipdrt_plan_obs_llh_terms_w(self._h, 3, float(weights), _p(rss), _p(slw)))
        return rss, slw

    def set_state(self, x=None, rho=None, s=None, weights=None, dop_rho=None):
        arrs = [None if a is None else _f64(a) for a in (x, rho, s, weights)]
        _check(self._lib.hipdrt_plan_set_state(self._h, *[None if a is None else _p(a) for a in arrs]))
        if dop_rho is not None:
            _check(self._lib.hipdrt_plan_set_state_dop(self._h, _p(_f64(dop_rho))))

    def continue_fit(self, opts, weight_factor=1.0, min_iter=2):
        _check(self._lib.hipdrt_plan_continue(self._h, C.byref(opts), float(weight_factor), int(min_iter)))

    def set_weight_factors(self, weight_factor=1.0, row_factors=None, late=False):
        """weight_factor / chrono- and EIS-row factors of _qphb_fit_core; row_factors (m,) or (capacity, m); late=True: the
        rows are a vector-valued weight_factor (applied from the second iteration on)"""
        rf = None if row_factors is None else _f64(row_factors)
        if rf is not None and rf.ndim == 2 and rf.shape[0] < self.capacity:     # the C side reads capacity rows
            rf = _f64(np.vstack([rf, np.ones((self.capacity - rf.shape[0], rf.shape[1]))]))
        _check(self._lib.hipdrt_plan_set_weight_factors(self._h, float(weight_factor), _p(rf),
                                                        int(rf is not None and rf.ndim == 2) | (2 if late else 0)))

    def kk_screen(self, opts: KkOpts | None = None, set_row_factors=False, z_hat=True, residuals=True):
        """hipdrt_plan_kk_screen: prediction at the fit frequencies, residuals in percent of |Z|, outlier mask and clean window
        of every spectrum of the fitted batch, on the device.  Returns dict(z_hat (B, nf) complex, residuals (B, nf) complex,
        std (B,), outlier_mask (B, nf) int32, f_lim (B, 2) = f_min, f_max, i_lim (B, 2), status (B,)); z_hat / residuals are
        left out on request.  set_row_factors: the next fit's row factors (outlier_weight on the rows of masked frequencies)
        are written on the device and the plan is left as set_weight_factors(1.0, rows, late=True) would leave it."""
        B, nf = self.B, self.nf
        out = _kk_outputs(B, nf)
        zr, zi = (np.empty((B, nf)), np.empty((B, nf))) if z_hat else (None, None)
        er, ei = (np.empty((B, nf)), np.empty((B, nf))) if residuals else (None, None)
        _check(self._lib.hipdrt_plan_kk_screen(self._h, C.byref(opts) if opts is not None else None, int(bool(set_row_factors)),
                                               _p(zr), _p(zi), _p(er), _p(ei), _p(out["std"]), _pi(out["outlier_mask"]),
                                               _p(out["f_lim"]), _pi(out["i_lim"]), _pi(out["status"])))
        if z_hat:
            out["z_hat"] = zr + 1j * zi
        if residuals:
            out["residuals"] = er + 1j * ei
        return out

    def set_tau_basis(self, ln_basis_tau, epsilon):
        """prepared plans: the tau basis the DRT block stands on (hipdrt_plan_set_tau_basis), needed by predict_drt"""
        ln_tau = _f64(ln_basis_tau)
        _check(self._lib.hipdrt_plan_set_tau_basis(self._h, _p(ln_tau), ln_tau.size, float(epsilon)))
        self._basis_nb = ln_tau.size

    def basis_size(self):
        """points of the tau basis the DRT block stands on (a prepared plan: what set_tau_basis gave)"""
        return getattr(self, '_basis_nb', None) or self.ntau

    def predict_drt(self, ln_tau_eval, order=0, sign=1, normalize=0, n_sigma=None):
        """hipdrt_plan_predict_drt for the fitted batch: mu (B, neval) = scale_b E x_b on the device; normalize 0 / 1 (by R_p) /
        2 (by absolute R_p); n_sigma = (s_lo, s_hi) adds the band.  Returns (mu, lo, hi, status) with lo = hi = None without
        n_sigma; status (B,): the fit's status, or PREDICT_NOT_PD."""
        ev = _f64(ln_tau_eval).ravel()
        B = self.B
        mu = np.empty((B, ev.size))
        lo, hi = (np.empty((B, ev.size)), np.empty((B, ev.size))) if n_sigma is not None else (None, None)
        s_lo, s_hi = (0.0, 0.0) if n_sigma is None else (float(n_sigma[0]), float(n_sigma[1]))
        status = np.empty(B, dtype=np.int32)
        _check(self._lib.hipdrt_plan_predict_drt(self._h, _p(ev), ev.size, int(order), int(sign), int(normalize), s_lo, s_hi,
                                                 _p(mu), _p(lo), _p(hi), _pi(status)))
        return mu, lo, hi, status

    def find_peaks(self, ln_tau_eval, opts: PeakOpts, row_scale=None, want=None):
        """hipdrt_plan_find_peaks for the fitted batch -> dict of dense (B, neval) rows peak_sign, keep, heights, prominences,
        probs, left_bases, right_bases (and peak_prob, curv_prob for method 2), count (B,), used_prominence (B,), status (B,).
        row_scale (B,): per-spectrum factor on the coefficient scale (prepared plans, normalize = 0).  want: the names to
        download (None: all); status always comes."""
        ev = _f64(ln_tau_eval).ravel()
        out = _peak_outputs(self.B, ev.size, opts.method, want)
        out["status"] = np.empty(self.B, dtype=np.int32)
        rs = None if row_scale is None else _f64(row_scale)
        if rs is not None and rs.shape != (self.B,):
            raise ValueError("row_scale must have shape (B,)")
        _check(self._lib.hipdrt_plan_find_peaks(self._h, _p(ev), ev.size, C.byref(opts), _p(rs), *_peak_out_args(out),
                                                _pi(out["status"])))
        return out

    def resolve_peaks(self, ln_tau_find, ln_tau_out=None, opts: PeakResolveOpts | None = None, find_opts: PeakOpts | None = None,
                      peak_indices=None, windows=None, row_scale=None, want=None):
        """hipdrt_plan_resolve_peaks for the fitted batch -> dict of the padded outputs count (B,), status (B,), peak_index,
        trough_index, eps_l, eps_r, r_peaks, r_coef (B, max_peaks), x_peaks (B, max_peaks, nb), peak_gammas (B, max_peaks,
        nout); absent slots hold -1 / NaN.  Peak source: peak_indices (B, max_peaks) -1 padded, or windows = (start, end), else
        find_peaks with find_opts.  want: the names to form and download (None: all)."""
        opts = opts if opts is not None else peak_resolve_opts()
        lt = _f64(ln_tau_find).ravel()
        lo = None if ln_tau_out is None else _f64(ln_tau_out).ravel()
        nb = self.basis_size()
        i = PeakResolveIn()
        keepers = [lt, lo]
        i.ln_tau_find, i.nfind, i.ln_tau_out, i.nout = _p(lt), lt.size, _p(lo), 0 if lo is None else lo.size
        if peak_indices is not None:
            k = _i32(peak_indices); keepers.append(k)
            if k.shape != (self.B, opts.max_peaks):
                raise ValueError("peak_indices must have shape (B, max_peaks)")
            i.source, i.peak_indices = PEAKS_FROM_INDICES, _pi(k)
        elif windows is not None:
            ws, we = _i32(windows[0]).ravel(), _i32(windows[1]).ravel(); keepers += [ws, we]
            i.source, i.win_start, i.win_end, i.nwin = PEAKS_FROM_WINDOWS, _pi(ws), _pi(we), ws.size
        else:
            po = find_opts if find_opts is not None else peak_opts()
            keepers.append(po)
            i.source, i.peak_opts = PEAKS_FROM_FIND, C.pointer(po)
        rs = None if row_scale is None else _f64(row_scale)
        if rs is not None and rs.shape != (self.B,):
            raise ValueError("row_scale must have shape (B,)")
        i.row_scale = _p(rs)
        out = _resolve_outputs(self.B, opts.max_peaks, nb, i.nout, want)
        u = _resolve_out_struct(out)
        _check(self._lib.hipdrt_plan_resolve_peaks(self._h, C.byref(i), C.byref(opts), C.byref(u)))
        return out

    def score_candidates(self, x=None, ncand=None, ln_tau_find=None, opts: PeakOpts | None = None, max_peaks=16, want=None):
        """hipdrt_plan_score_candidates for the fitted batch: x (C, B, n) scaled candidate vectors to upload, or None for every
        recorded step of the step store; ncand (B,) candidates per spectrum (None: all); ln_tau_find: the grid of the peak
        search (None: likelihood sums only) -> dict of rss, sum_log_w, count, status (C, B), peak_index, heights, prominences
        (C, B, max_peaks); absent slots hold -1 / NaN.  want: the names to form and download (None: all); status always comes."""
        B, n = self.B, self.n
        i = CandidatesIn()
        keepers = []
        if x is None:
            Cn = self.pfrt_steps()
            i.source, i.C = CANDIDATES_FROM_STEPS, 0
        else:
            xa = _f64(x); keepers.append(xa)
            if xa.ndim != 3 or xa.shape[1:] != (B, n):
                raise ValueError("x must have shape (C, B, n)")
            Cn = xa.shape[0]
            i.source, i.C, i.x = CANDIDATES_FROM_HOST, Cn, _p(xa)
        if ncand is not None:
            nc = _i32(ncand); keepers.append(nc)
            if nc.shape != (B,):
                raise ValueError("ncand must have shape (B,)")
            i.ncand = _pi(nc)
        lt = None if ln_tau_find is None else _f64(ln_tau_find).ravel()
        po = opts if opts is not None else peak_opts()
        keepers += [lt, po]
        i.ln_tau_find, i.nfind, i.peak_opts, i.max_peaks = _p(lt), 0 if lt is None else lt.size, C.pointer(po), int(max_peaks)
        mp = int(max_peaks) or 16
        shapes = dict(rss=(Cn, B), sum_log_w=(Cn, B), count=(Cn, B), peak_index=(Cn, B, mp), heights=(Cn, B, mp),
                      prominences=(Cn, B, mp), status=(Cn, B))
        out = {}
        for k, shape in shapes.items():
            if (want is not None and k not in want and k != "status") or (lt is None and k in CANDIDATE_OUTPUTS[2:6]):
                continue
            out[k] = np.full(shape, -77, dtype=np.int32) if k in ("count", "peak_index", "status") else np.full(shape, 7e77)
        u = CandidatesOut()
        for k in CANDIDATE_OUTPUTS:
            a = out.get(k)
            setattr(u, k, None if a is None else (_pi(a) if a.dtype == np.int32 else _p(a)))
        _check(self._lib.hipdrt_plan_score_candidates(self._h, C.byref(i), C.byref(u)))
        return out

    def integrate_drt(self, ln_tau_eval, windows, order=0, sign=1, normalize=0, row_scale=None):
        """hipdrt_plan_integrate_drt: the trapezoid of predict_drt's row over every window (start, end) -> ((B, nwin), status)"""
        ev = _f64(ln_tau_eval).ravel()
        ws, we = _i32(windows[0]).ravel(), _i32(windows[1]).ravel()
        rs = None if row_scale is None else _f64(row_scale)
        if rs is not None and rs.shape != (self.B,):
            raise ValueError("row_scale must have shape (B,)")
        out = np.empty((self.B, ws.size))
        status = np.empty(self.B, dtype=np.int32)
        _check(self._lib.hipdrt_plan_integrate_drt(self._h, _p(ev), ev.size, int(order), int(sign), int(normalize), _p(rs), _pi(ws),
                                                   _pi(we), ws.size, _p(out), _pi(status)))
        return out, status

    def predict_z(self, frequencies, include_drt=True, include_ohmic=True, include_inductance=True):
        """hipdrt_plan_predict_z: complex (B, nf) impedance of the fitted batch at any frequencies, and the status (B,)"""
        f = _f64(frequencies).ravel()
        B = self.B
        zr, zi = np.empty((B, f.size)), np.empty((B, f.size))
        status = np.empty(B, dtype=np.int32)
        mask = int(bool(include_drt)) | (int(bool(include_ohmic)) << 1) | (int(bool(include_inductance)) << 2)
        _check(self._lib.hipdrt_plan_predict_z(self._h, _p(f), f.size, mask, _p(zr), _p(zi), _pi(status)))
        return zr + 1j * zi, status

    def predict_resistances(self, absolute=False, r_p_only=False):
        """hipdrt_plan_predict_resistances: (r_p, r_inf, r_tot), each (B,); r_p_only (prepared plans): (r_p, None, None)"""
        B = self.B
        r_p = np.empty(B)
        r_inf, r_tot = (None, None) if r_p_only else (np.empty(B), np.empty(B))
        _check(self._lib.hipdrt_plan_predict_resistances(self._h, _p(r_p), _p(r_inf), _p(r_tot), int(bool(absolute))))
        return r_p, r_inf, r_tot

    def pfrt_begin(self, max_steps):
        """size and empty the PFRT step store (hipdrt_plan_pfrt_begin)"""
        _check(self._lib.hipdrt_plan_pfrt_begin(self._h, int(max_steps)))

    def pfrt_record(self):
        """append the state the last fit / warm restart left to the PFRT step store (hipdrt_plan_pfrt_record)"""
        _check(self._lib.hipdrt_plan_pfrt_record(self._h))

    def pfrt_restore_s(self, step, factor=1.0):
        """the live s vectors become factor times those step `step` recorded, on the device (hipdrt_plan_pfrt_restore_s)"""
        _check(self._lib.hipdrt_plan_pfrt_restore_s(self._h, int(step), float(factor)))

    def pfrt_steps(self):
        n = C.c_int()
        _check(self._lib.hipdrt_plan_pfrt_steps(self._h, C.byref(n)))
        return n.value

    def pfrt_step_state(self, step):
        """what step `step` recorded -> dict(x (B, n), rho (B, 3), s_vectors (B, 3, n), rss (B,), sum_log_w (B,), status (B,))"""
        B, n = self.B, self.n
        out = dict(x=np.empty((B, n)), rho=np.empty((B, 3)), s_vectors=np.empty((B, 3, n)), rss=np.empty(B), sum_log_w=np.empty(B),
                   status=np.empty(B, dtype=np.int32))
        _check(self._lib.hipdrt_plan_pfrt_get_step(self._h, int(step), _p(out["x"]), _p(out["rho"]), _p(out["s_vectors"]),
                                                   _p(out["rss"]), _p(out["sum_log_w"]), _pi(out["status"])))
        return out

    def step_p_matrix(self, step, b=0):
        """pfrt_result['step_p_mat'][step] of spectrum b (hipdrt_plan_get_step_p_matrix)"""
        out = np.empty((self.n, self.n))
        _check(self._lib.hipdrt_plan_get_step_p_matrix(self._h, int(step), int(b), _p(out)))
        return out

    def predict_pfrt(self, factors, ln_tau_pfrt, ln_tau_out=None, opts: PfrtOpts | None = None, want=None):
        """hipdrt_plan_predict_pfrt over the recorded steps -> dict(pfrt (B, nout), raw_pfrt (B, np), step_pfrt (S, B, np),
        post_prob (S, B), status (B,)); want: the names to form and download (None: all); status always comes"""
        fac, ltp = _f64(factors).ravel(), _f64(ln_tau_pfrt).ravel()
        lto = None if ln_tau_out is None else _f64(ln_tau_out).ravel()
        S, B, npf = fac.size, self.B, ltp.size
        if S != self.pfrt_steps():
            raise ValueError(f"factors has {S} entries, the plan has recorded {self.pfrt_steps()} PFRT steps")
        nout = npf if lto is None else lto.size
        opts = opts if opts is not None else pfrt_opts()
        shapes = dict(pfrt=(B, nout), raw_pfrt=(B, npf), step_pfrt=(S, B, npf), post_prob=(S, B))
        out = {k: np.full(shape, 7e77) for k, shape in shapes.items() if want is None or k in want}
        out["status"] = np.empty(B, dtype=np.int32)
        g = out.get
        _check(self._lib.hipdrt_plan_predict_pfrt(self._h, _p(fac), _p(ltp), npf, _p(lto), nout, C.byref(opts), _p(g("pfrt")),
                                                  _p(g("raw_pfrt")), _p(g("step_pfrt")), _p(g("post_prob")), _pi(out["status"])))
        return out

    def set_init_h(self, h_init):
        h = None if h_init is None else _f64(h_init)
        _check(self._lib.hipdrt_plan_set_init_h(self._h, _p(h)))

    def record_history(self, b):
        _check(self._lib.hipdrt_plan_record_history(self._h, int(b)))

    def download(self, s_vectors=False, lean=False):
        """results of the staged spectra; ``lean``: only what a map records per observation (fit_x, R_inf, inductance, the
        coefficient scale, iteration counts, status) -- 4 kB instead of 29 kB per spectrum at 256 x 512"""
        B, n, m = self.B, self.n, self.m
        out = dict(fit_x=np.empty((B, self.ntau)), R_inf=np.empty(B), inductance=np.empty(B), coefficient_scale=np.empty(B),
                   outer_iters=np.empty(B, dtype=np.int32), qp_iters_total=np.empty(B, dtype=np.int32),
                   status=np.empty(B, dtype=np.int32))
        if not lean:
            out.update(x=np.empty((B, n)), weights=np.empty((B, m)), rho=np.empty((B, 3)), q_vector=np.empty((B, n)))
        sv = np.empty((B, 3, n)) if (s_vectors and not lean) else None
        opt = lambda key: _p(out[key]) if key in out else None          # noqa: E731 (NULL = not wanted, include/hipdrt.h)
        _check(self._lib.hipdrt_plan_download(self._h, opt("x"), _p(out["fit_x"]), _p(out["R_inf"]),
                                              _p(out["inductance"]), opt("weights"), _p(out["coefficient_scale"]),
                                              opt("rho"), _p(sv) if sv is not None else None, opt("q_vector"),
                                              _pi(out["outer_iters"]), _pi(out["qp_iters_total"]), _pi(out["status"])))
        if sv is not None:
            out["s_vectors"] = sv
        return out

    def p_matrix(self, b):
        out = np.empty((self.n, self.n))
        _check(self._lib.hipdrt_plan_get_p_matrix(self._h, int(b), _p(out)))
        return out

    def distribution_var(self, basis_eval, batch):
        """diag(B P^-1 B') cs^2 for every fitted spectrum; basis_eval (neval, ntau)."""
        basis_eval = _f64(basis_eval)
        out = np.empty((int(batch), basis_eval.shape[0]))
        status = np.empty(int(batch), dtype=np.int32)
        _check(self._lib.hipdrt_plan_distribution_var(self._h, _p(basis_eval), basis_eval.shape[0], _p(out), _pi(status)))
        return out, status

    def param_cov(self, b=0):
        """inv(P_b) cs_b^2 (n, n) of fitted spectrum b, and whether P_b was positive definite"""
        out = np.empty((self.n, self.n))
        status = C.c_int()
        _check(self._lib.hipdrt_plan_param_cov(self._h, int(b), _p(out), C.byref(status)))
        return out, status.value == 0

    def distribution_cov(self, basis_eval, b=0):
        """basis_eval inv(P_b)[DRT block] basis_eval' cs_b^2 (neval, neval) of fitted spectrum b"""
        basis_eval = _f64(basis_eval)
        out = np.empty((basis_eval.shape[0], basis_eval.shape[0]))
        status = C.c_int()
        _check(self._lib.hipdrt_plan_distribution_cov(self._h, int(b), _p(basis_eval), basis_eval.shape[0], _p(out),
                                                      C.byref(status)))
        return out, status.value == 0

    def param_var(self, batch):
        out = np.empty((int(batch), self.n))
        status = np.empty(int(batch), dtype=np.int32)
        _check(self._lib.hipdrt_plan_param_var(self._h, _p(out), _pi(status)))
        return out, status

    def history(self):
        cap = int(self.opts.max_iter)
        hx, hr, hw = np.empty((cap, self.n)), np.empty((cap, 3)), np.empty((cap, self.m))
        qi = np.empty(cap + 1, dtype=np.int32)
        rows = C.c_int()
        _check(self._lib.hipdrt_plan_get_history(self._h, _p(hx), _p(hr), _p(hw), _pi(qi), cap, C.byref(rows)))
        r = rows.value
        return dict(x=hx[:r], rho=hr[:r], weights=hw[:r], qp_iterations=qi[:r + 1])

    def timings(self):
        t = (C.c_float * 5)()
        l = (C.c_int * 5)()
        _check(self._lib.hipdrt_plan_timings(self._h, t, l))
        names = ("total", "gram", "qp", "hyper", "other")
        return {k: float(t[i]) for i, k in enumerate(names)}, {k: int(l[i]) for i, k in enumerate(names)}


class PreparedPlan(Plan):
    """hipdrt_plan_create_prepared: the device loop on caller-prepared matrices (any data type; optional x_dop block
    and vz_offset column).  `desc` is a PreparedDesc, penalty = [m0, m1, m2] (n, n), vmm (m, m), h / l1 (n,)."""

    def __init__(self, ctx: Context, desc: PreparedDesc, penalty, vmm, h, l1, vz_strength=None,
                 opts: FitOpts | None = None, capacity=1):
        self._lib = load_library()
        self.ctx = ctx
        self.desc = desc
        self.opts = opts if opts is not None else default_fit_opts()
        mk = [_f64(a) for a in penalty]
        vmm, h, l1 = _f64(vmm), _f64(h), _f64(l1)
        vzs = None if vz_strength is None else _f64(vz_strength)
        hnd = _vp()
        _check(self._lib.hipdrt_plan_create_prepared(ctx._h, C.byref(desc), _p(mk[0]), _p(mk[1]), _p(mk[2]), _p(vmm),
                                                     _p(h), _p(l1), _p(vzs), C.byref(self.opts), int(capacity),
                                                     C.byref(hnd)))
        self._h = hnd
        self.n, self.m, self.ns = desc.n, desc.m, desc.ns
        self.nf, self.ntau, self.ngrid = 0, desc.n - desc.ns, 0
        self.capacity = int(capacity)
        self.B = 0
        self.rm_batched = False

    def upload(self, rzm, rzv):
        """rzm (m, n) shared or (B, m, n) per measurement; rzv (B, m)"""
        rzm, rzv = _f64(rzm), _f64(rzv)
        if rzv.ndim == 1:
            rzv = rzv[None, :]
        batched = rzm.ndim == 3
        _check(self._lib.hipdrt_plan_upload_prepared(self._h, rzv.shape[0], int(batched), _p(rzm), _p(rzv)))
        self.batch = self.B = rzv.shape[0]
        self.rm_batched = batched

    def iterate(self, x_in=None, s_vectors=None, rho=None, dop_rho=None, weights=None, est_weights=None,
                xmx_norms=None, dop_xmx_norms=None):
        """hipdrt_plan_iterate: one qphb.iterate_qphb on every staged measurement; arrays are (B, ...) or None to keep
        what the device holds.  Returns dict(converged, qp_status, qp_iters, primal_objective), each (B,)."""
        B, n, m = self.batch, self.n, self.m
        shapes = dict(x_in=(B, n), s_vectors=(B, 3, n), rho=(B, 3), dop_rho=(B, 3), weights=(B, m),
                      est_weights=(B, m), xmx_norms=(B, 3), dop_xmx_norms=(B, 3))
        given = dict(x_in=x_in, s_vectors=s_vectors, rho=rho, dop_rho=dop_rho, weights=weights,
                     est_weights=est_weights, xmx_norms=xmx_norms, dop_xmx_norms=dop_xmx_norms)
        st, keep = IterateState(), []
        for name, arr in given.items():
            if arr is None:
                continue
            a = _f64(arr)
            if a.shape != shapes[name]:
                raise ValueError(f"{name}: expected shape {shapes[name]}, got {a.shape}")
            keep.append(a)
            setattr(st, name, _p(a))
        conv, status, iters = (np.empty(B, dtype=np.int32) for _ in range(3))
        pobj = np.empty(B)
        _check(self._lib.hipdrt_plan_iterate(self._h, C.byref(st), _pi(conv), _pi(status), _pi(iters), _p(pobj)))
        return dict(converged=conv.astype(bool), qp_status=status, qp_iters=iters, primal_objective=pobj)

    def set_predict_desc(self, idx_rinf, idx_induc, idx_cinv, inductance_scale, capacitance_scale, coefficient_scale,
                         dop_scale_vector=None, v_baseline_scale=None, response_signal_scale=None, scaled_response_offset=None):
        """hipdrt_plan_set_predict_desc: what the special columns mean and the post-fit scales of the fitted batch (per member:
        coefficient_scale, response_signal_scale, scaled_response_offset, each (B,); dop_scale_vector (dop_size,) shared or (B, dop_size))"""
        d, keep = PredictDesc(), []
        d.idx_rinf, d.idx_induc, d.idx_cinv = int(idx_rinf), int(idx_induc), int(idx_cinv)
        d.inductance_scale, d.capacitance_scale = float(inductance_scale), float(capacitance_scale)
        if dop_scale_vector is not None and np.ndim(dop_scale_vector) == 2:
            if np.shape(dop_scale_vector) != (self.batch, self.desc.dop_size):
                raise ValueError(f"dop_scale_vector: expected shape {(self.batch, self.desc.dop_size)} or {(self.desc.dop_size,)}")
            d.dop_scale_batched = 1
        sizes = dict(dop_scale_vector=self.desc.dop_size * (self.batch if d.dop_scale_batched else 1),
                     v_baseline_scale=self.desc.vb_size, coefficient_scale=self.batch,
                     response_signal_scale=self.batch, scaled_response_offset=self.batch)
        given = dict(dop_scale_vector=dop_scale_vector, v_baseline_scale=v_baseline_scale, coefficient_scale=coefficient_scale,
                     response_signal_scale=response_signal_scale, scaled_response_offset=scaled_response_offset)
        for name, v in given.items():
            if v is None:
                continue
            v = _f64(v).ravel()
            if v.size != sizes[name]:
                raise ValueError(f"{name}: expected {sizes[name]} values, got {v.size}")
            keep.append(v)
            setattr(d, name, _p(v))
        _check(self._lib.hipdrt_plan_set_predict_desc(self._h, C.byref(d)))

    def predict_response(self, times, step_times, step_sizes, basis_tau=None, mode=MODE_TRAPZ, ny=1000, lookup=None,
                         basis_nu=None, nu_epsilon=0.0, inf_rv=None, cap_rv=None, vz_strength=None, vb_mat=None,
                         include_mask=INCLUDE_ALL):
        """hipdrt_plan_predict_response: (B, nt) voltage response of the fitted batch at any times, and the status (B,).
        step_sizes (S,) or (B, S); inf_rv / cap_rv (nt,) or (B, nt); lookup = (log_td, v) for MODE_INTERP; vb_mat (nt, vb_size)."""
        a, keep = ResponseArgs(), []
        B = self.batch

        def arr(name, v, shapes=None):
            if v is not None:
                v = _f64(v)
                if shapes is not None and v.shape not in shapes:
                    raise ValueError(f"{name}: expected shape {' or '.join(map(str, shapes))}, got {v.shape}")
                keep.append(v)
                setattr(a, name, _p(v))
            return v
        t = arr('times', np.ravel(times))
        st = arr('step_times', np.ravel(step_times))
        a.nt, a.nsteps = t.size, st.size
        sz = arr('step_sizes', step_sizes, [(st.size,), (B, st.size)])
        a.sizes_batched = int(sz.ndim == 2)
        # (without set_tau_basis the library refuses before it reads the basis)
        arr('basis_tau', basis_tau, [(self._basis_nb,)] if getattr(self, '_basis_nb', None) else None)
        a.mode, a.ny = int(mode), int(ny)
        if lookup is not None:
            ltd, v = arr('log_td', lookup[0]), arr('v', lookup[1])
            a.ngrid = ltd.size
        arr('basis_nu', basis_nu, [(self.desc.dop_size,)])
        a.nu_epsilon = float(nu_epsilon)
        for name, v in (('inf_rv', inf_rv), ('cap_rv', cap_rv)):
            v = arr(name, v, [(t.size,), (B, t.size)])
            if v is not None:
                setattr(a, name[:3] + '_batched', int(v.ndim == 2))
        arr('vz_strength', vz_strength, [(t.size,)])
        arr('vb_mat', vb_mat, [(t.size, self.desc.vb_size)])
        a.include_mask = int(include_mask)
        out = np.empty((B, t.size))
        status = np.empty(B, dtype=np.int32)
        _check(self._lib.hipdrt_plan_predict_response(self._h, C.byref(a), _p(out), _pi(status)))
        return out, status

    def predict_z_model(self, frequencies, basis_tau=None, mode=MODE_TRAPZ, ny=1000, lookups=None, basis_nu=None, nu_epsilon=0.0,
                        vz_strength=None, include_mask=INCLUDE_ALL):
        """hipdrt_plan_predict_z_model: complex (B, nf) impedance of the fitted batch of a prepared plan at any frequencies, and
        the status (B,).  lookups = ((log_wt_re, z_re), (log_wt_im, z_im)) for MODE_INTERP; vz_strength (nf,) or None."""
        a, keep = ZModelArgs(), []

        def arr(name, v, shape=None):
            if v is not None:
                v = _f64(v)
                if shape is not None and v.shape != shape:
                    raise ValueError(f"{name}: expected shape {shape}, got {v.shape}")
                keep.append(v)
                setattr(a, name, _p(v))
            return v
        f = arr('freq', np.ravel(frequencies))
        a.nf = f.size
        arr('basis_tau', basis_tau, (self._basis_nb,) if getattr(self, '_basis_nb', None) else None)
        a.mode, a.ny = int(mode), int(ny)
        if lookups is not None:
            (lwr, zr), (lwi, zi) = lookups
            lwr = arr('log_wt_re', lwr)
            a.ngrid = lwr.size
            for name, v in (('z_re', zr), ('log_wt_im', lwi), ('z_im', zi)):
                arr(name, v, (lwr.size,))
        arr('basis_nu', basis_nu, (self.desc.dop_size,))
        a.nu_epsilon = float(nu_epsilon)
        arr('vz_strength', vz_strength, (f.size,))
        a.include_mask = int(include_mask)
        B = self.batch
        zr, zi = np.empty((B, f.size)), np.empty((B, f.size))
        status = np.empty(B, dtype=np.int32)
        _check(self._lib.hipdrt_plan_predict_z_model(self._h, C.byref(a), _p(zr), _p(zi), _pi(status)))
        return zr + 1j * zi, status

    def predict_dop(self, nu, basis_nu, nu_epsilon, normalize_by=None, nu_basis_area=1.0, include_ideal=True):
        """hipdrt_plan_predict_dop: (B, len(nu)) distribution of phasances of the fitted batch on the ascending grid nu, and the
        status (B,); normalize_by (len(nu),) divides it (get_dop_norm), None leaves it as it is"""
        nu, bn = _f64(nu).ravel(), _f64(basis_nu).ravel()
        if bn.size != self.desc.dop_size:
            raise ValueError(f"basis_nu: expected {self.desc.dop_size} points, got {bn.size}")
        nb = None if normalize_by is None else _f64(normalize_by).ravel()
        if nb is not None and nb.size != nu.size:
            raise ValueError("normalize_by must have one entry per point of nu")
        B = self.batch
        out = np.empty((B, nu.size))
        status = np.empty(B, dtype=np.int32)
        _check(self._lib.hipdrt_plan_predict_dop(self._h, _p(nu), nu.size, _p(bn), float(nu_epsilon), _p(nb), float(nu_basis_area),
                                                 int(bool(include_ideal)), _p(out), _pi(status)))
        return out, status

    def get(self, which):
        B = self.batch
        shapes = {"m0": (self.n, self.n), "m1": (self.n, self.n), "m2": (self.n, self.n), "vmm": (self.m, self.m),
                  "h": (self.n,), "est_weights": (B, self.m), "rv": (B, self.m), "xmx": (B, 3), "dop_rho": (B, 3),
                  "dop_xmx": (B, 3), "hist_dop_rho": (int(self.opts.max_iter), 3), "outlier_t": (B, self.m),
                  "weight_factors": (B, 2), "x": (B, self.n), "var_floor": (B,),
                  "rzm": (B, self.m, self.n) if self.rm_batched else (self.m, self.n)}
        out = np.empty(shapes[which])
        _check(self._lib.hipdrt_plan_get(self._h, which.encode(), _p(out), out.size))
        return out

    def history(self):
        h = super().history()
        if self.desc.dop_size > 0:
            h["dop_rho"] = self.get("hist_dop_rho")[:len(h["x"])]
        return h


_default_ctx = {}


def device_usable(device: int = 0) -> bool:
    """can this process open gfx950 device `device`? (no exception, and nothing is created on the device -- not even a stream:
    streams are dealt to the hardware queues in the order they are made; mapping.dist picks its default backend with this)"""
    try:
        lib = load_library()
    except HipDrtError:
        return False
    return lib.hipdrt_device_probe(int(device)) == 0


def comm_unique_id() -> bytes:
    """128 opaque bytes of a fresh RCCL communicator id (rank 0 makes them, every rank passes them to Comm)"""
    buf = C.create_string_buffer(128)
    _check(load_library().hipdrt_comm_unique_id(buf))
    return buf.raw


class Comm:
    """RCCL communicator behind the C ABI (include/hipdrt.h: hipdrt_comm_*): one per process, numpy in / numpy out"""

    def __init__(self, device, rank, world, unique_id):
        self._lib = load_library()
        self._h = _vp()
        self.rank, self.world, self.device = int(rank), int(world), int(device)
        if len(unique_id) != 128:
            raise HipDrtError("a RCCL unique id has 128 bytes")
        _check(self._lib.hipdrt_comm_create(self.device, self.rank, self.world, C.c_char_p(bytes(unique_id)), C.byref(self._h)))

    def close(self):
        if self._h:
            self._lib.hipdrt_comm_destroy(self._h)
            self._h = _vp()

    def __del__(self):
        try:
            self.close()
        except Exception:       # noqa: BLE001 (interpreter shutdown)
            pass

    def broadcast(self, array, root=0):
        """`array` (contiguous float64) of `root` into every rank's `array`, in place"""
        if not (isinstance(array, np.ndarray) and array.dtype == np.float64 and array.flags.c_contiguous):
            raise HipDrtError("broadcast needs a C-contiguous float64 array (it is filled in place)")
        _check(self._lib.hipdrt_comm_broadcast(self._h, _p(array), array.size, int(root)))
        return array

    def gather(self, block, root=0):
        """every rank's `block` (same size everywhere) to `root`: returns (world, block.size) there, None elsewhere"""
        block = _f64(block).ravel()
        out = np.empty((self.world, block.size)) if self.rank == root else None
        _check(self._lib.hipdrt_comm_gather(self._h, _p(block), block.size, _p(out), int(root)))
        return out

    def allreduce_max(self, value):
        v = C.c_double(float(value))
        _check(self._lib.hipdrt_comm_allreduce_max(self._h, C.byref(v)))
        return v.value

    def barrier(self):
        _check(self._lib.hipdrt_comm_barrier(self._h))


def get_context(device: int = 0) -> Context:
    """Process-wide context per device (created on first use)."""
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]
