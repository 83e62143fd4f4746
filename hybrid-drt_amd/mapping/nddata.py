"""The quality-control chains of hybdrt/mapping/nddata.py -- impute_nans (135-149), flag_outliers (152-175) and flag_bad_obs
(178-295, without its correction branches) -- and the row score that DRTMD.score_group_data_badness / score_group_fit_badness
(hybdrt/mapping/drtmd.py:642-783) build from them, on the device (csrc/map_rank.hip, hipdrt_map_badness) and, as
``*_statement``, in numpy alone (filters/ndfilters.py for the rank filters and the masked Gaussian, models.kk.robust_std): the
statement is what the device is read against and what runs without a GPU; the device functions have no numpy fall-back."""
import warnings

import numpy as np

from .. import _ffi, filters
from ..filters import ndfilters
from ..models import kk

# what drtmd.py:695-696 passes to flag_outliers, and flag_outliers' own defaults
FLAG_SIZE, FLAG_THRESH, P_PRIOR, FULL_STD_CONTRIBUTION = (5, 1), 0.7, 0.01, 0.05
IMPUTE_SIGMA = 0.5


def _size2(size):
    size = [int(s) for s in ndfilters._normalize_sequence(size, 2)]
    if min(size) < 1:
        raise RuntimeError("incorrect filter size")
    return size


def _array2(a, what):
    if type(a) in (list, tuple):
        raise NotImplementedError(f"{what}: lists of arrays are not built; pass one 2-D array")
    a = np.asarray(a, dtype=float)
    if a.ndim != 2:
        raise NotImplementedError(f"{what}: the chains take 2-D arrays")
    return a


def _impute_sigma(impute_kw):
    kw = dict(impute_kw or {'sigma': IMPUTE_SIGMA})
    if kw.pop('method', 'filter') != 'filter':
        raise ValueError('Imputation method not implemented')
    if kw.pop('filter_func', None) is not None:
        raise NotImplementedError("filter_func: impute_nans runs the Gaussian masked filter")
    if 'sigma' not in kw:
        raise TypeError("impute_nans needs sigma= (upstream's masked Gaussian has no default)")
    sigma = kw.pop('sigma')
    truncate = float(kw.pop('truncate', 4.0))
    if kw:
        raise NotImplementedError(f"impute_kw: {sorted(kw)} are not built")
    return [float(s) for s in ndfilters._normalize_sequence(sigma, 2)], truncate


def _check_bad_obs(test_factor_correction, test_offset_correction, robust_std):
    if test_factor_correction:
        raise NotImplementedError("test_factor_correction: the correction branches are not built")
    if test_offset_correction:
        raise NotImplementedError("test_offset_correction: the correction branches are not built")
    if not robust_std:
        raise NotImplementedError("robust_std=False: only the IQR form of the local spread is built")


# ---- the numpy statement -------------------------------------------------------------------------------------------------------
def impute_nans_statement(ndy, method='filter', filter_func=None, **filter_kw):
    """nddata.impute_nans (135-149)"""
    if method != 'filter':
        raise ValueError(f'Imputation method {method} not implemented')
    ndy = np.asarray(ndy, dtype=float)
    nan_index = np.isnan(ndy)
    y_filt = ndfilters.masked_filter(np.nan_to_num(ndy), (~nan_index).astype(float), filter_func=filter_func, **filter_kw)
    y_out = ndy.copy()
    y_out[nan_index] = y_filt[nan_index]
    return y_out


def pdf_normal(x, loc, scale):
    """stats.pdf_normal (hybdrt/utils/stats.py:11-12)"""
    return 1 / (scale * np.sqrt(2 * np.pi)) * np.exp(-0.5 * (x - loc) ** 2 / scale ** 2)


def outlier_prob(x, mu_in, sigma_in, sigma_out, p_prior):
    """preprocessing.outlier_prob (hybdrt/preprocessing.py:860-876)"""
    pdf_in = pdf_normal(x, mu_in, sigma_in)
    pdf_out = pdf_normal(x, mu_in, sigma_out)
    p_out = p_prior * pdf_out / ((1 - p_prior) * pdf_in + p_prior * pdf_out)
    p_out[np.abs(x - mu_in) <= sigma_in] = 0
    return p_out


def flag_outliers_statement(ndy, filter_size, thresh=0.9, p_prior=0.01, full_std_contribution=0.05, impute=True, impute_kw=None,
                            return_prob=False):
    """nddata.flag_outliers (152-175).  (Its np.nan_to_num(y_filt, np.nanmedian(y_filt)) passes the median as nan_to_num's
    `copy`: NaNs become 0, which is what is stated here.)  return_prob: also p_out, mu_in and sigma_in (the fixture generator's
    margins)"""
    ndy = _array2(ndy, 'ndy')
    size = _size2(filter_size)
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        if impute and np.any(np.isnan(ndy)):
            sigma, truncate = _impute_sigma(impute_kw)
            y_filt = impute_nans_statement(ndy, sigma=sigma, truncate=truncate)
        else:
            y_filt = ndy
        mu_in = ndfilters.median_filter(y_filt, size)
        sigma_in = ndfilters.iqr_filter(y_filt, size=size) / 1.349
        sigma_in += full_std_contribution * kk.robust_std(np.nan_to_num(y_filt))
        sigma_in += 1e-8
        sigma_out = np.abs(ndy - mu_in) + 1e-8
        p_out = np.nan_to_num(outlier_prob(ndy, mu_in, sigma_in, sigma_out, p_prior))
    if return_prob:
        return p_out > thresh, p_out, mu_in, sigma_in
    return p_out > thresh


def bad_obs_std(x_filt, std_size):
    """the local spread of flag_bad_obs (193-198, robust_std=True)"""
    tmp = x_filt.copy()
    with warnings.catch_warnings():
        warnings.simplefilter('ignore', RuntimeWarning)
        tmp[np.isnan(tmp)] = np.nanmedian(tmp)
    x_std = ndfilters.iqr_filter(tmp, size=_size2(std_size)) / 1.349
    x_std += 0.1 * kk.robust_std(x_filt[~np.isnan(x_filt)])
    return x_std


def flag_bad_obs_statement(x_raw, x_filt, std_size=5, thresh=2, test_factor_correction=False, test_offset_correction=False,
                           return_rss=False, robust_std=True):
    """nddata.flag_bad_obs (178-218, 286-295) for one array"""
    _check_bad_obs(test_factor_correction, test_offset_correction, robust_std)
    x_raw, x_filt = _array2(x_raw, 'x_raw'), _array2(x_filt, 'x_filt')
    x_std = bad_obs_std(x_filt, std_size)
    if np.any(np.isnan(x_std)):
        raise ValueError('x_std contains nans!')
    with np.errstate(invalid='ignore', divide='ignore', over='ignore'):
        resid = np.nan_to_num((x_raw - x_filt) / x_std)
        rss = np.sum(resid ** 2, axis=-1) / x_raw.shape[-1]
    bad = np.zeros(x_raw.shape, dtype=bool)
    bad[rss >= thresh] = 1
    return (bad, rss) if return_rss else bad


def score_rows_statement(a, median_size, std_size, scale_src=None, ignore_outliers=False, return_info=False):
    """the score of one array of drtmd.py:642-747: optionally (a - mid(a)) / range(scale_src) by row (675-679), optionally
    flag_outliers with the 5 % rule (693-707), then the median filter and flag_bad_obs' rss.  return_info: dict(rss=, flags=,
    filt=, a=) -- `a` the array that was scored"""
    a = _array2(a, 'a').copy()
    flags = None
    with warnings.catch_warnings(), np.errstate(invalid='ignore', divide='ignore'):
        warnings.simplefilter('ignore', RuntimeWarning)
        if scale_src is not None:
            src = _array2(scale_src, 'scale_src')
            v_hi = np.nanpercentile(a, 98, axis=1)
            v_lo = np.nanpercentile(a, 2, axis=1)
            v_mid = 0.5 * (v_hi + v_lo)
            i_range = np.nanpercentile(src, 98, axis=1) - np.nanpercentile(src, 2, axis=1)
            a = (a - v_mid[:, None]) / i_range[:, None]
        if ignore_outliers:
            flags = flag_outliers_statement(a, filter_size=FLAG_SIZE, thresh=FLAG_THRESH)
            count_index = np.sum(flags, axis=1) < int(a.shape[1] * 0.05)
            a[count_index[:, None] & flags] = np.nan
    filt = ndfilters.median_filter(a, size=_size2(median_size))
    _, rss = flag_bad_obs_statement(a, filt, std_size=std_size, return_rss=True)
    return dict(rss=rss, flags=flags, filt=filt, a=a) if return_info else rss


# ---- the device chain ----------------------------------------------------------------------------------------------------------
class _Args(_ffi.Bound):
    """hipdrt_map_badness_args with its defaults and the numpy tables its pointers refer to"""

    def __init__(self, median_size=(1, 1), std_size=(1, 1)):
        super().__init__(_ffi.MapBadnessArgs())
        c = self.c
        c.median_size[:] = _size2(median_size)
        c.std_size[:] = _size2(std_size)
        c.flag_size[:] = [1, 1]
        c.n_std = kk.std_normal_quantile(0.75)          # robust_std's sample_fraction = 0.5
        c.score = 1
        for t in c.impute_gauss:
            self.table(t, None)

    def flags(self, filter_size, thresh, p_prior, full_std_contribution, impute, impute_kw):
        c = self.c
        c.flag_outliers, c.impute = 1, int(bool(impute))
        c.flag_size[:] = _size2(filter_size)
        c.thresh, c.p_prior, c.full_std_contribution = float(thresh), float(p_prior), float(full_std_contribution)
        if impute:
            sigma, truncate = _impute_sigma(impute_kw)
            for l, s in enumerate(sigma):
                if s > 1e-15:
                    self.table(c.impute_gauss[l], ndfilters.gaussian_kernel1d(s, 0, ndfilters.kernel_radius(s, truncate)))


def impute_nans(ndy, method='filter', filter_func=None, device=0, **filter_kw):
    """nddata.impute_nans (135-149): NaNs replaced by the masked Gaussian of their neighbours (hipdrt.filters.masked_filter)"""
    if method != 'filter':
        raise ValueError(f'Imputation method {method} not implemented')
    ndy = np.asarray(ndy, dtype=float)
    nan_index = np.isnan(ndy)
    y_filt = filters.masked_filter(np.nan_to_num(ndy), (~nan_index).astype(float), filter_func=filter_func, device=device, **filter_kw)
    y_out = ndy.copy()
    y_out[nan_index] = y_filt[nan_index]
    return y_out


def flag_outliers(ndy, filter_size, thresh=0.9, p_prior=0.01, full_std_contribution=0.05, impute=True, impute_kw=None, device=0):
    """nddata.flag_outliers (152-175): the boolean outlier flags of a 2-D array"""
    ndy = _array2(ndy, 'ndy')
    args = _Args()
    args.flags(filter_size, thresh, p_prior, full_std_contribution, impute, impute_kw)
    args.c.score = 0
    return _ffi.get_context(device).map_badness(ndy, args.c, want_flags=True)["flags"]


def flag_bad_obs(x_raw, x_filt, std_size=5, thresh=2, test_factor_correction=False, test_offset_correction=False, return_rss=False,
                 robust_std=True, device=0):
    """nddata.flag_bad_obs (178-218, 286-295) for one array: rows whose mean squared residual against x_filt, in units of the
    local robust spread of x_filt, reaches thresh"""
    _check_bad_obs(test_factor_correction, test_offset_correction, robust_std)
    x_raw, x_filt = _array2(x_raw, 'x_raw'), _array2(x_filt, 'x_filt')
    if x_raw.shape != x_filt.shape:
        raise ValueError("x_raw and x_filt must have one shape")
    args = _Args(std_size=std_size)
    args.array("filt_in", x_filt)
    rss = _ffi.get_context(device).map_badness(x_raw, args.c)["rss"]
    bad = np.zeros(x_raw.shape, dtype=bool)
    bad[rss >= thresh] = 1
    return (bad, rss) if return_rss else bad


def score_rows(a, median_size, std_size, scale_src=None, ignore_outliers=False, return_info=False, device=0):
    """score_rows_statement on the device, between one upload and one download (return_info: rss, flags and filt only)"""
    a = _array2(a, 'a')
    args = _Args(median_size, std_size)
    if scale_src is not None:
        scale_src = _array2(scale_src, 'scale_src')
        args.c.scale = 1
    if ignore_outliers:
        args.flags(FLAG_SIZE, FLAG_THRESH, P_PRIOR, FULL_STD_CONTRIBUTION, True, None)
    res = _ffi.get_context(device).map_badness(a, args.c, scale_src=scale_src, want_flags=bool(return_info and ignore_outliers),
                                               want_filt=bool(return_info))
    return res if return_info else res["rss"]
