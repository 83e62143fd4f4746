"""Candidate models of a fit in numpy: what DRT.generate_candidates (hybdrt/models/drt1d.py:1632-1821) does with the candidates'
log-likelihoods and peaks once it has them -- BIC, the best candidate per number of peaks, the filling of missing peak counts,
the two tables, the Bayes factors (hybdrt/utils/stats.py:137-165) -- and the statement of the device's likelihood sums
(csrc/candidates.hip).  The device gives rss, sum_log_w and the peak lists of every candidate (hipdrt_plan_score_candidates);
everything here is host arithmetic on those few numbers per candidate."""
import numpy as np


def candidate_llh_terms(x, rm, rv, vmm, var_floor):
    """(rss, sum_log_w) of candidate vectors x (..., n) for one spectrum: r = rm x - rv, s = vmm r^2 floored at var_floor,
    w = max(s^-1/2, 1e-10) (qphb.estimate_weights, qphb.py:1347-1377), rss = |w rm x|^2 - 2 (w rv).(w rm x) + |w rv|^2 and
    sum log w, as llh_kernel (csrc/hyper.hip) with re-estimated weights expands them.  The dtype of x decides the precision."""
    x = np.asarray(x)
    dt = x.dtype
    rm, rv, vmm = np.asarray(rm, dtype=dt), np.asarray(rv, dtype=dt), np.asarray(vmm, dtype=dt)
    yh = x @ rm.T
    r = yh - rv
    s = np.maximum((r * r) @ vmm.T, dt.type(var_floor))
    w = np.maximum(1 / np.sqrt(s), dt.type(1e-10))
    wy, wr = w * yh, w * rv
    rss = np.sum(wy * wy, axis=-1) - 2 * np.sum(wr * wy, axis=-1) + np.sum(wr * wr, axis=-1)
    return rss, np.sum(np.log(w), axis=-1)


def bic(k, n, llh):
    """stats.bic: k ln n - 2 llh"""
    return k * np.log(n) - 2 * llh


def bayes_factor(c1, c2, criterion='bic'):
    if criterion == 'bic':
        return np.exp(-0.5 * (c1 - c2))
    elif criterion in ('lml', 'lml-bic'):
        return np.exp(c1 - c2)
    raise ValueError(f'Invalid criterion {criterion}')


def norm_bayes_factors(crit_values, criterion='bic'):
    crit_values = np.asarray(crit_values)
    if criterion == 'bic':
        return np.exp(-0.5 * (crit_values - np.min(crit_values)))
    elif criterion in ('lml', 'lml-bic'):
        return np.exp(crit_values - np.max(crit_values))
    raise ValueError(f'Invalid criterion {criterion}')


def best_per_num_peaks(num_peaks, llh):
    """(unique_num_peaks ascending, best_indices): for every number of peaks the first candidate that attains the largest
    log-likelihood among the candidates with that many peaks (drt1d.py:1731-1750; numpy's where gives the first index at ties)"""
    num_peaks, llh = np.asarray(num_peaks), np.asarray(llh)
    unique = np.unique(num_peaks)
    best = np.empty(len(unique), dtype=int)
    for i, k in enumerate(unique):
        best[i] = np.where((num_peaks == k) & (llh == np.max(llh[num_peaks == k])))[0][0]
    return unique, best


def fill_candidates(unique_num_peaks, best_peaks, min_fill_num=None):
    """The missing peak counts of drt1d.py:1752-1812.  unique_num_peaks: ascending counts that have a candidate; best_peaks:
    {count: (prominences, heights)} of the best candidate of every count.  min_fill_num None: no filling below the simplest
    candidate; negative: that many counts below it (not below 1); otherwise fill from that count up.  Returns
    {new count j: (source count, order)}: the entry for j peaks takes everything from the best candidate with `source count`
    peaks and keeps its peaks order[:j], in descending order of min(prominence, height)."""
    unique = np.asarray(unique_num_peaks)
    if min_fill_num is None:
        min_fill_num = unique[0]
    elif min_fill_num < 0:
        min_fill_num = max(1, unique[0] + min_fill_num)
    if min_fill_num < unique[0]:
        unique = np.insert(unique, 0, min_fill_num - 1)      # a dummy entry: the loop below fills from min_fill_num
    new = {}
    for fi in np.where(np.diff(unique) > 1)[0]:
        lo_num, hi_num = int(unique[fi]), int(unique[fi + 1])
        prom, height = best_peaks[hi_num]
        order = np.argsort(np.minimum(prom, height))[::-1]
        for j in range(lo_num + 1, hi_num):
            new[j] = (hi_num, order[:j])
    return new


def candidate_table(num_peaks, llh, bic_values, indices=None):
    """upstream's candidate_df (indices None) or best_candidate_df (indices = best_indices) as a dict of arrays: model_id (the
    table of best candidates only), num_peaks, llh, bic, rel_llh = llh - max llh and rel_bic = bic - min bic over ALL
    candidates.  Every column is float, as the DataFrame built from one stacked array is."""
    num_peaks, llh, bic_values = (np.asarray(a, dtype=float) for a in (num_peaks, llh, bic_values))
    best_llh, best_bic = np.max(llh), np.min(bic_values)
    sel = slice(None) if indices is None else np.asarray(indices, dtype=int)
    table = {}
    if indices is not None:
        table['model_id'] = num_peaks[sel]
    table.update(num_peaks=num_peaks[sel], llh=llh[sel], bic=bic_values[sel], rel_llh=llh[sel] - best_llh,
                 rel_bic=bic_values[sel] - best_bic)
    return table


def rank_candidates(num_peaks, llh, num_special, num_data, peak_prominences, peak_heights, fill=True, min_fill_num=None):
    """Everything generate_candidates derives from the scored candidates of ONE spectrum: num_peaks (C,), llh (C,),
    peak_prominences / peak_heights: per-candidate arrays of its peaks.  k = num_special + 4 num_peaks parameters
    (drt1d.py:1716-1721).  Returns dict(bic (C,), candidate_table, unique_num_peaks, best_indices, best_table,
    best_keys: the sorted peak counts of best_candidate_dict after filling, filled: fill_candidates' result)."""
    num_peaks, llh = np.asarray(num_peaks), np.asarray(llh, dtype=float)
    bic_values = np.array([bic(num_special + k * 4, num_data, v) for k, v in zip(num_peaks, llh)])
    unique, best = best_per_num_peaks(num_peaks, llh)
    filled = {}
    if fill:
        filled = fill_candidates(unique, {int(k): (np.asarray(peak_prominences[i]), np.asarray(peak_heights[i]))
                                          for k, i in zip(unique, best)}, min_fill_num)
    return dict(bic=bic_values, candidate_table=candidate_table(num_peaks, llh, bic_values), unique_num_peaks=unique,
                best_indices=best, best_table=candidate_table(num_peaks, llh, bic_values, best),
                best_keys=sorted(set(int(k) for k in unique) | set(filled)), filled=filled)
