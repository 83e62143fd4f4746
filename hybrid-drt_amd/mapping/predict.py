"""The prediction block of DRTMD (hybdrt/mapping/drtmd.py:788-1106) on the arrays a store keeps: the numpy statement of
csrc/map_predict.hip (hipdrt_map_predict), as mapping/nddata.py is of csrc/map_rank.hip.  Built from what is already stated in
numpy: matrices.basis.construct_func_eval_matrix, filters.ndfilters (the plain 'reflect' correlation of scipy.ndimage.gaussian_filter)
and models.peaks (scipy.signal.find_peaks restated, the two upper-tail probabilities).  No scipy.

The reference's rules, as they are:
  predict_x (815-833)            normalise first (x / (sum|x| area) by row), then filter
  apply_filter (_filters.py:506-518)   with nothing given gaussian_filter(sigma=(1, 0)), 'reflect', truncate 4 -- a plain correlation:
                                 a NaN row spreads to its neighbours as scipy spreads it (it is not the masked filter)
  predict_drt_cov (993-1008)     the map clamp of the variances: li = nearest_index(tau, tau_supergrid[left] * 10) + 1,
                                 ri = nearest_index(tau, tau_supergrid[right] / 10) with `right` the exclusive end -- the grid point one
                                 past the basis; the left side is clamped first, then the right; a row that holds a NaN is left alone
  predict_peak_prob (1023-1064)  x normalised and filtered, the variances not divided by r_p^2; variances passed by the caller are used as
                                 given (neither clamped nor filtered); peak_spread_sigma smooths along tau only, times sigma sqrt(2 pi),
                                 and the product with sign(f) comes after the smoothing
  predict_curv_prob (1066-1106)  x unnormalised

Two extensions where upstream raises an IndexError: right == len(tau_supergrid) takes tau_supergrid[right - 1], and
li >= len(tau) raises the ValueError of PostFitMixin._peak_ext."""
import numpy as np

from ..filters import ndfilters
from ..matrices import basis
from ..models import peaks

DEFAULT_PPD = 10


def tau_eval(tau_supergrid, ppd, extend_decades=0):
    """DRTMD.get_tau_eval (drtmd.py:1252-1263)"""
    log_min = np.min(np.log10(tau_supergrid)) - extend_decades
    log_max = np.max(np.log10(tau_supergrid)) + extend_decades
    return np.logspace(log_min, log_max, int((log_max - log_min) * ppd) + 1)


def rel_round(x, precision):
    """utils.array.rel_round (hybdrt/utils/array.py:23-45) of an array: `precision` digits after the leading one"""
    x = np.asarray(x, dtype=float)
    digits = (precision - np.floor(np.log10(np.abs(x) + 1e-30))).astype(int)
    return np.array([round(xi, di) for xi, di in zip(x.flatten().tolist(), digits.flatten().tolist())]).reshape(x.shape)


def row_match_index(a, b, precision=None):
    """utils.array.row_match_index (array.py:312-335): for every row of b the index of the matching row of a, -1 without one"""
    if precision is not None:
        a, b = rel_round(a, precision), rel_round(b, precision)
    # upstream compares every row of a with every row of b (an M x N table); the same answer from one dictionary: of several equal
    # rows of a the last one wins there as well
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    where = {tuple(row): k for k, row in enumerate(a.tolist())}
    return np.array([where.get(tuple(row), -1) for row in b.tolist()], dtype=int).reshape(len(b))


def filter_sigma(filter_kw, ndim=2):
    """the per-axis sigma of apply_filter(x, None, filter_kw) (_filters.py:506-518): (1, ..., 1, 0) with nothing given"""
    if filter_kw is None:
        sigma = np.ones(ndim)
        sigma[-1] = 0
        return tuple(sigma.tolist())
    kw = dict(filter_kw)
    if 'sigma' not in kw:
        raise TypeError("the Gaussian filter needs sigma=")
    sigma = kw.pop('sigma')
    if kw.pop('mode', 'reflect') != 'reflect':
        raise NotImplementedError("only mode='reflect' is built")
    truncate = kw.pop('truncate', 4.0)
    if kw:
        raise TypeError(f"unexpected filter keywords {sorted(kw)}")
    if truncate != 4.0:
        raise NotImplementedError("only truncate=4 is built")
    sigma = tuple(float(s) for s in (np.atleast_1d(sigma) if np.ndim(sigma) else [sigma] * ndim))
    if len(sigma) != ndim:
        raise RuntimeError("sequence argument must have length equal to input rank")
    return sigma


def gaussian_tables(sigma, truncate=4.0):
    """one full symmetric order-0 table per axis as scipy.ndimage.gaussian_filter builds it, None where sigma <= 1e-15"""
    return [ndfilters.gaussian_kernel1d(s, 0, ndfilters.kernel_radius(s, truncate)) if s > 1e-15 else None for s in sigma]


def filter_tables(ndfilter, filter_kw=None, ndim=2):
    """the tables of predict_*(ndfilter=, filter_func=None, filter_kw=); None without a filter"""
    return gaussian_tables(filter_sigma(filter_kw, ndim)) if ndfilter else None


def correlate_tables(a, tables):
    """the axes in order, as gaussian_filter runs them"""
    a = np.array(a, dtype=float)
    for axis, tab in enumerate(tables or ()):
        if tab is not None:
            a = ndfilters.correlate1d_reflect(a, tab, axis)
    return a


def map_x_statement(x, basis_area, normalize, filter_tables=None):
    """predict_x (drtmd.py:815-833) on rows that are already selected"""
    x = np.array(x, dtype=float)
    if normalize:
        rp = np.sum(np.abs(x), axis=-1) * basis_area
        with np.errstate(divide='ignore', invalid='ignore'):
            x = x / rp[:, None]
    return correlate_tables(x, filter_tables)


def map_drt_statement(x, ln_tau_sup, ln_tau_eval, epsilon, order=0):
    """predict_drt (drtmd.py:848-851)"""
    em = basis.construct_func_eval_matrix(np.asarray(ln_tau_sup, dtype=float), np.asarray(ln_tau_eval, dtype=float), 'gaussian',
                                          epsilon, order=order)
    return np.asarray(x, dtype=float) @ em.T


def clamp_indices(tau_eval, tau_supergrid, tau_indices):
    """(li, ri) of the map clamp (drtmd.py:998-1003) for one observation's (left, right)"""
    tau_supergrid = np.asarray(tau_supergrid, dtype=float)
    left, right = int(tau_indices[0]), int(tau_indices[1])
    if right >= len(tau_supergrid):                     # upstream: IndexError for an observation that uses the whole supergrid
        right = len(tau_supergrid) - 1
    li = peaks.nearest_index(tau_eval, tau_supergrid[left] * 10) + 1
    ri = peaks.nearest_index(tau_eval, tau_supergrid[right] / 10)
    if li >= len(tau_eval):                             # upstream: IndexError; the message of PostFitMixin._peak_ext
        raise ValueError('extend_var: the measured tau range ends at the last point of the evaluation grid')
    return li, ri


def clamp_index_rows(tau_eval, tau_supergrid, obs_tau_indices):
    """(rows, 2) int32; (-1, -1) for an observation without slots (unfitted)"""
    out = np.full((len(obs_tau_indices), 2), -1, dtype=np.int32)
    for k, ti in enumerate(obs_tau_indices):
        if ti is not None:
            out[k] = clamp_indices(tau_eval, tau_supergrid, ti)
    return out


def clamp_rows(var, ext):
    """the clamp itself: left first, then right; rows that hold a NaN and rows without indices are left alone"""
    var = np.array(var, dtype=float)
    for k in range(len(var)):
        li, ri = int(ext[k][0]), int(ext[k][1])
        if li < 0 or np.any(np.isnan(var[k])):
            continue
        var[k, :li] = np.maximum(var[k, :li], var[k, li])
        var[k, ri:] = np.maximum(var[k, ri:], var[k, ri])
    return var


def map_var_statement(var, tau_eval, tau_supergrid, obs_tau_indices, extend_var=True, filter_tables=None):
    """predict_drt_var (drtmd.py:1012-1021) on rows that already are diag(B x_cov B'): the clamp of 993-1008, then the filter"""
    var = np.array(var, dtype=float)
    if extend_var:
        var = clamp_rows(var, clamp_index_rows(tau_eval, tau_supergrid, obs_tau_indices))
    return correlate_tables(var, filter_tables)


def search_kind(nonneg, sign):
    """curvature.py:15: one pass on -sign fxx for a nonneg fit with sign != 0, else the two-pass search (0)"""
    return int(sign) if (nonneg and sign != 0) else 0


def peak_rows(f, fxx, f_var, fxx_var, search, height, prominence):
    """curvature.peak_prob_1d along the last axis: the unsigned probability at every peak, zeros elsewhere (a NaN row has no
    peaks: every comparison is false; it becomes a NaN row through sign(f))"""
    f, fxx = np.asarray(f, dtype=float), np.asarray(fxx, dtype=float)
    out = np.zeros(f.shape)
    for k in range(len(f)):
        idx, probs = peaks._peak_prob_at_peaks(f[k], fxx[k], f_var[k], fxx_var[k], search, height, prominence)
        out[k, idx] = probs
    return out


def spread_statement(peak_prob, peak_spread_sigma):
    """drtmd.py:1057-1062: gaussian_filter along tau only, times 1 / pdf_normal(0, 0, sigma) = sigma sqrt(2 pi)"""
    tabs = gaussian_tables((0.0,) * (np.ndim(peak_prob) - 1) + (float(peak_spread_sigma),))
    return correlate_tables(peak_prob, tabs) * spread_factor(peak_spread_sigma)


def spread_factor(peak_spread_sigma):
    """1 / utils.stats.pdf_normal(0, 0, sigma)"""
    return 1 / (1 / (peak_spread_sigma * np.sqrt(2 * np.pi)) * np.exp(-0.5 * (0 / peak_spread_sigma) ** 2))


def _map_rows(x, tau_supergrid, tau, epsilon, basis_area, normalize, tables, f_var, fxx_var, given, obs_tau_indices, extend_var):
    ln_sup, ln_ev = np.log(tau_supergrid), np.log(tau)
    xf = map_x_statement(x, basis_area, normalize, tables)
    f, fxx = map_drt_statement(xf, ln_sup, ln_ev, epsilon, 0), map_drt_statement(xf, ln_sup, ln_ev, epsilon, 2)
    if not given:
        f_var = map_var_statement(f_var, tau, tau_supergrid, obs_tau_indices, extend_var, tables)
        fxx_var = map_var_statement(fxx_var, tau, tau_supergrid, obs_tau_indices, extend_var, tables)
    return xf, f, fxx, np.asarray(f_var, dtype=float), np.asarray(fxx_var, dtype=float)


def peak_prob_map_statement(x, f_var, fxx_var, tau_supergrid, tau, epsilon, basis_area, nonneg=True, sign=1, prominence=5e-3,
                            height=1e-3, peak_spread_sigma=None, filter_tables=None, var_given=True, obs_tau_indices=None,
                            extend_var=True, x_given=False, return_info=False):
    """predict_peak_prob (drtmd.py:1023-1064) on the rows x (raw coefficients; x_given: the caller's x=, used as it is).  var_given:
    f_var / fxx_var are the caller's and used as given; otherwise they are the stored raw rows and take the clamp (extend_var, with
    obs_tau_indices) and the filter."""
    xf, f, fxx, vf, vxx = _map_rows(x, tau_supergrid, tau, epsilon, basis_area, not x_given, None if x_given else filter_tables,
                                    f_var, fxx_var, var_given, obs_tau_indices, extend_var)
    with np.errstate(invalid='ignore', divide='ignore'):
        pk = peak_rows(f, fxx, vf, vxx, search_kind(nonneg, sign), height, prominence)
        if peak_spread_sigma is not None:
            pk = spread_statement(pk, peak_spread_sigma)
        out = pk * np.sign(f)
    if return_info:
        return out, dict(x=xf, f=f, fxx=fxx, f_var=vf, fxx_var=vxx)
    return out


def curv_prob_map_statement(x, f_var, fxx_var, tau_supergrid, tau, epsilon, basis_area, filter_tables=None, var_given=True,
                            obs_tau_indices=None, extend_var=True, x_given=False, return_info=False):
    """predict_curv_prob (drtmd.py:1066-1106): x unnormalised"""
    xf, f, fxx, vf, vxx = _map_rows(x, tau_supergrid, tau, epsilon, basis_area, False, None if x_given else filter_tables,
                                    f_var, fxx_var, var_given, obs_tau_indices, extend_var)
    with np.errstate(invalid='ignore', divide='ignore'):
        out = peaks.curv_prob_row(f, fxx, vf, vxx)
    if return_info:
        return out, dict(x=xf, f=f, fxx=fxx, f_var=vf, fxx_var=vxx)
    return out
