"""Option structures filled from the library's defaults, and the host arrays the post-fit entry points write into."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .abi import (FitOpts, KkOpts, PeakOpts, PeakProbOpts, PeakResolveOpts, PeakResolveOut, PfrtOpts, PfrtSelectOpts, RESOLVE_OUTPUTS, _check, _p, _pi,
                  load_library)


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


PEAK_PROB_SEARCH = {'rows': 0, 'thresh': 1, 'ranges': 2}


def peak_prob_opts(bayes_cov=True, std_size=5, std_baseline=0.1, sigma_floor=True, ext_left=-1, ext_right=-1, search='rows',
                   height=None, prominence=None) -> PeakProbOpts:
    """hipdrt_peak_prob_opts from the keywords of DRT.find_peaks_byprob (None <-> NaN: that condition is off); search 'rows'
    (no search), 'thresh' (height and prominence) or 'ranges', or its number"""
    o = PeakProbOpts()
    load_library().hipdrt_peak_prob_opts_default(C.byref(o))
    o.bayes_cov, o.std_size, o.std_baseline, o.sigma_floor = int(bool(bayes_cov)), int(std_size), float(std_baseline), int(bool(sigma_floor))
    o.ext_left, o.ext_right = int(ext_left), int(ext_right)
    o.search = PEAK_PROB_SEARCH[search] if isinstance(search, str) else int(search)
    o.height = float('nan') if height is None else float(height)
    o.prominence = float('nan') if prominence is None else float(prominence)
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


def pfrt_select_opts(start_thresh=0.99, end_thresh=0.01, peak_thresh=1e-6, max_peaks=16) -> PfrtSelectOpts:
    """hipdrt_pfrt_select_opts from the keywords of DRT.select_pfrt_candidates"""
    o = PfrtSelectOpts()
    load_library().hipdrt_pfrt_select_opts_default(C.byref(o))
    o.start_thresh, o.end_thresh, o.peak_thresh, o.max_peaks = float(start_thresh), float(end_thresh), float(peak_thresh), int(max_peaks)
    return o


def pfrt_bytes_per_spectrum(n, steps):
    """bytes the PFRT step store takes per spectrum of the plan's capacity (hipdrt_plan_pfrt_bytes_per_spectrum)"""
    out = C.c_longlong()
    _check(load_library().hipdrt_plan_pfrt_bytes_per_spectrum(int(n), int(steps), C.byref(out)))
    return int(out.value)


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


_PEAK_PROB_INT = ("keep", "left_bases", "right_bases")
_PEAK_PROB_F64 = ("pp", "tp", "prob", "sigma", "heights", "prominences")


def _peak_prob_outputs(B, n, search, nranges, want=None, given_prob=False):
    """host arrays of the peak-probability entry points, poisoned like _peak_outputs'; only what the search mode writes is
    allocated (0: the rows, 1: also the dense peak rows and count, 2: also range_peaks), and of that only `want` (None: all)"""
    names = (() if given_prob else ("pp", "tp", "sigma")) + ("prob",)
    if search == 1:
        names += ("keep", "heights", "prominences", "left_bases", "right_bases", "count")
    if search == 2:
        names += ("range_peaks",)
    out = {}
    for k in names:
        if want is not None and k not in want:
            continue
        shape = {"count": (B,), "range_peaks": (B, nranges), "sigma": (3, B, n)}.get(k, (B, n))
        out[k] = np.full(shape, -77, dtype=np.int32) if k in _PEAK_PROB_INT + ("count", "range_peaks") else np.full(shape, np.nan)
    return out


def _peak_prob_out_args(out):
    g = out.get
    return (_p(g("pp")), _p(g("tp")), _p(g("prob")), _p(g("sigma")), _pi(g("keep")), _p(g("heights")), _p(g("prominences")),
            _pi(g("left_bases")), _pi(g("right_bases")), _pi(g("count")), _pi(g("range_peaks")))


def _index_windows(ranges):
    """(lo, hi) int32 arrays of the index windows [lo, hi] of search 2; None: no windows"""
    if ranges is None:
        return None, None
    r = np.asarray(ranges, dtype=np.int64).reshape(-1, 2)
    return np.ascontiguousarray(r[:, 0], dtype=np.int32), np.ascontiguousarray(r[:, 1], dtype=np.int32)


def _kk_outputs(B, nf):
    return dict(std=np.empty(B), outlier_mask=np.empty((B, nf), dtype=np.int32), f_lim=np.empty((B, 2)),
                i_lim=np.empty((B, 2), dtype=np.int32), status=np.empty(B, dtype=np.int32))
