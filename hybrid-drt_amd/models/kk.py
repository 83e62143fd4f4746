"""Kramers-Kronig test helpers, the counterpart of hybdrt.models.kk (hybdrt/models/kk.py) in numpy.

They serve two purposes: they are the helpers the reference exposes to its users (same names, same arguments), and they are the
specification of the statistics stage of the device kernel (csrc/kk.hip), which tests/test_gpu_kk.py checks against them.  A
fitted ``DRT`` does not use them: its residuals, outliers and limits come from ``hipdrt_plan_kk_screen`` on the device.

Where the reference leans on scipy the arithmetic is written out, so that host and device do the same operations:

* ``1 - chi2.cdf(|e|^2, 2, scale=std^2)`` (stats.outer_cdf_chi2, hybdrt/utils/stats.py:23-25) is ``exp(-|e|^2 / (2 std^2))``;
* ``ndimage.uniform_filter1d(is_outlier, size=3)`` with its default 'reflect' ends, compared with zero, is a sum of three
  neighbours with the end points repeated;
* the search of get_limits over all pairs of boundary moves is a search over the running outlier counts.
"""
import numpy as np
from scipy.special import ndtr


def normalize_residuals(z_meas, z_pred, norm="modulus"):
    """kk.normalize_residuals (kk.py:9-19): residuals in percent of |z_meas|.  Only norm="modulus" exists (the reference's other
    branch divides by the string it was handed)."""
    if norm != "modulus":
        raise ValueError(f'norm must be "modulus", got {norm!r}')
    z_meas = np.asarray(z_meas)
    return 100 * (z_meas - np.asarray(z_pred)) / np.abs(z_meas)


def std_normal_quantile(quantile):
    """stats.std_normal_quantile (hybdrt/utils/stats.py:108-116): the standard-normal quantile read off the cdf tabulated at 2000
    points of [0, 14] by linear interpolation -- 0.84162417 for 0.8, where the exact quantile is 0.84162123.  The table is kept
    so that ``std`` agrees with the reference to rounding; it is the ``n_std`` handed to the device."""
    s = np.linspace(0, 14, 2000)
    q = float(quantile)
    return float(np.interp(abs(q - 0.5) + 0.5, ndtr(s), s) * np.sign(q - 0.5))


def robust_std(x, sample_fraction=0.5):
    """stats.robust_std (stats.py:124-134): width of the central ``sample_fraction`` of the sample (numpy's linear percentiles)
    over the width of the same fraction of a standard normal.  NaN for fewer than two values."""
    if sample_fraction > 1 or sample_fraction <= 0:
        raise ValueError("sample_fraction must be in (0, 1]")
    x = np.asarray(x, dtype=float)
    if x.size < 2:
        return np.nan
    q_lo = np.percentile(x, 50 - 100 * sample_fraction / 2)
    q_hi = np.percentile(x, 50 + 100 * sample_fraction / 2)
    return (q_hi - q_lo) / (2 * std_normal_quantile(0.5 + sample_fraction / 2))


def _outlier_pass(z_err_norm, n_iter, p_thresh, n_sigma, std_sample_fraction):
    """(mask, std of the last iteration) of kk.get_outliers"""
    z = np.asarray(z_err_norm, dtype=complex)
    mask = np.zeros(len(z), dtype=bool)
    std = np.nan
    e2 = z.real ** 2 + z.imag ** 2
    for _ in range(int(n_iter)):
        keep = z[~mask]
        std = robust_std(np.concatenate([keep.real, keep.imag]), std_sample_fraction)
        if not (np.isfinite(std) and std > 0):
            mask = np.zeros(len(z), dtype=bool)       # the reference compares against NaN here: nothing is an outlier
        elif n_sigma is None:
            with np.errstate(under="ignore"):
                mask = np.exp(-e2 / (2 * std * std)) < p_thresh
        else:
            mask = np.sqrt(e2) > n_sigma * std
    return mask, std


def get_outliers(z_err_norm, n_iter=2, p_thresh=1e-4, n_sigma=None, std_sample_fraction=0.6, return_std=False):
    """kk.get_outliers (kk.py:21-53): indices of the residuals that are too large for a circular normal distribution whose
    scale is estimated robustly from the residuals not yet marked, ``n_iter`` times.  ``return_std`` adds the last scale."""
    if p_thresh is not None and n_sigma is None and not 0 < p_thresh < 1:
        raise ValueError("p_thresh must be in (0, 1)")
    if n_sigma is not None and not n_sigma > 0:
        raise ValueError("n_sigma must be positive")
    mask, std = _outlier_pass(z_err_norm, n_iter, p_thresh, n_sigma, std_sample_fraction)
    index = np.where(mask)[0]
    return (index, std) if return_std else index


def get_limits(f_fit, outlier_index, max_num_outliers=2, return_index=False):
    """kk.get_limits (kk.py:56-123): (f_min, f_max) of the widest window of clean data -- it starts and ends at points that are
    clean and have clean neighbours, and holds at most ``max_num_outliers`` outliers.  IndexError when no such point exists (as
    upstream).  ``return_index`` adds (i_left, i_right), positions in descending-frequency order."""
    f_fit = np.asarray(f_fit, dtype=float)
    nf = len(f_fit)
    if max_num_outliers < 0:
        raise ValueError("max_num_outliers must not be negative")
    order = np.argsort(f_fit)[::-1]
    mask = np.zeros(nf, dtype=bool)
    mask[np.asarray(outlier_index, dtype=int)] = True
    o = mask[order].astype(int)
    padded = np.concatenate([o[:1], o, o[-1:]])
    clean = np.where(padded[:-2] + padded[1:-1] + padded[2:] == 0)[0]
    if len(clean) == 0:
        raise IndexError("no clean point with clean neighbours: the frequency limits are undefined")
    i_left, i_right = int(clean[0]), int(clean[-1])
    inside = int(o[i_left:i_right].sum())                  # (the right end is excluded upstream, and so it is here)
    if inside > max_num_outliers:
        need = inside - max_num_outliers
        window = o[i_left:i_right + 1]
        fl, fr = np.cumsum(window), np.cumsum(window[::-1])
        best = None
        for r in range(len(window)):                       # fl is non-decreasing: the first admissible l is the best for this r
            l = int(np.searchsorted(fl, need - fr[r], side="left"))
            if l < len(window) and (best is None or r + l < best[0] + best[1]):
                best = (r, l)
        r, l = best
        i_left, i_right = i_left + l, i_right - r
    if o[i_left]:
        i_left = int(clean[clean >= i_left].min())
    if o[i_right]:
        i_right = int(clean[clean <= i_right].max())
    f_sorted = f_fit[order]
    f_max, f_min = f_sorted[i_left], f_sorted[i_right]
    if return_index:
        return (f_min, f_max), (i_left, i_right)
    return f_min, f_max


def trim_data(frequencies, z, f_min, f_max):
    """kk.trim_data (kk.py:125-128): the data inside [f_min, f_max]"""
    frequencies, z = np.asarray(frequencies), np.asarray(z)
    mask = (frequencies <= f_max) & (frequencies >= f_min)
    return frequencies[mask], z[mask]
