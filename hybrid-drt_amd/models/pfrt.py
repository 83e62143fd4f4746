"""The probability function of relaxation times (PFRT) on evaluated rows: the numpy statement of csrc/pfrt.hip (as models/peaks.py
is of csrc/peaks.hip).

DRT.predict_pfrt (hybdrt/models/drt1d.py:2716-2858) over the S solutions of a PFRT fit: the posterior weights of the steps
(2730-2749), per step the credibility of every curvature peak (2789-2829), their weighted sum (2831-2834), the smoothing matrix of
evaluation.get_similarity_function('gaussian') (2840-2848), pfrt.integrate_peaks (hybdrt/models/pfrt.py:22-46 over
utils.array.find_contiguous_ranges) and the normalisation by the maximum.  Everything acts on rows that are already evaluated: per
step f (order 0), fxx (order 2) and their posterior variances before extend_var and the floor.  No scipy.

DRT.select_pfrt_candidates (drt1d.py:2860-2865 over hybdrt/models/pfrt.py:49-213) on the raw PFRT, the steps' rows and the step
likelihoods: rank_peaks, shift_candidate, candidate_corr, select_candidates and the compact result form that pfrt_select_kernel
writes (select_compact / candidates_from_compact).

Sums run in the order the kernels use (over the steps ascending, over the grid ascending); where upstream lets numpy choose the
order (np.trapezoid, the matrix product) the difference is a reordering of non-negative terms.
"""
import math

import numpy as np

from . import peaks

LOG_2PI = math.log(2 * math.pi)


def llh_consts(m, alpha_0=2, beta_0=1):
    """(c, alpha_n, beta_0) of evaluate_llh(marginalize_weights=True) for m data rows (drt1d.py:4457-4496):
    llh = (c - alpha_n ln(beta_0 + rss / 2)) + sum(log w)"""
    alpha_n = alpha_0 - 1 + m / 2
    return alpha_0 * math.log(beta_0) + math.lgamma(alpha_n) - math.lgamma(alpha_0), alpha_n, beta_0


def step_llh(rss, sum_log_w, m, alpha_0=2, beta_0=1):
    """the step likelihoods from the two recorded sums, (S,) or (S, B)"""
    c, alpha_n, beta_0 = llh_consts(m, alpha_0, beta_0)
    return (c - alpha_n * np.log(beta_0 + 0.5 * np.asarray(rss, dtype=float))) + np.asarray(sum_log_w, dtype=float)


def step_posterior(factors, llh, prior_mu=-4, prior_sigma=0.5, n_eff_factor=0.5):
    """drt1d.py:2730-2749 -> post_prob_eff (S,): log-normal prior on ln(factor) plus the step likelihood, shifted by its maximum,
    times n_eff_factor, exponentiated and divided by the trapezoid area over ln(factors) (one factor: by the value itself)"""
    lf = np.log(np.asarray(factors, dtype=float))
    llh = np.asarray(llh, dtype=float)
    log_post = -0.5 * (LOG_2PI + 2.0 * math.log(prior_sigma) + ((lf - prior_mu) / prior_sigma) ** 2) + llh
    e = np.exp((log_post - np.max(log_post)) * n_eff_factor)
    if len(lf) > 1:
        area = 0.0
        for i in range(len(lf) - 1):
            area += ((lf[i + 1] - lf[i]) * (e[i + 1] + e[i])) / 2.0
    else:
        area = e[0]
    return e / area


def step_peak_probs(f, fxx, var_f, var_fxx, search=1, height=1e-3, prominence=5e-3, fxx_var_floor=1e-5, ext_left=-1,
                    ext_right=-1):
    """drt1d.py:2766-2829 for one step -> dense (n,) row: at every peak of the search (peaks.search_peaks) the lower of the two
    two-sided probabilities 1 - erfc(|f| / (sigma_f sqrt 2)) and 1 - erfc(min(prominence, height) / (sigma_fxx sqrt 2)), zero
    elsewhere.  var_f, var_fxx: the variances before extend_var's clamp and the floor, which both get (2772-2786)."""
    f = np.asarray(f, dtype=float)
    idx, info, _ = peaks.search_peaks(fxx, f, search, height, prominence)
    sf = peaks.extend_var(var_f, ext_left, ext_right, fxx_var_floor) ** 0.5
    sxx = peaks.extend_var(var_fxx, ext_left, ext_right, fxx_var_floor) ** 0.5
    min_prom = np.minimum(info['prominences'], info['peak_heights'])
    out = np.zeros(len(f))
    out[idx] = np.minimum(peaks.peak_probs(np.abs(f[idx]), sf[idx]), peaks.peak_probs(min_prom, sxx[idx]))
    return out


def combine(post_prob, step_pfrt):
    """drt1d.py:2831-2834: sum_i post_i step_pfrt_i / sum_i post_i, the steps added in ascending order"""
    post_prob, step_pfrt = np.asarray(post_prob, dtype=float), np.asarray(step_pfrt, dtype=float)
    tot = np.zeros(step_pfrt.shape[1])
    psum = 0.0
    for i in range(len(post_prob)):
        tot = tot + post_prob[i] * step_pfrt[i]
        psum += post_prob[i]
    return tot / psum


def smooth_matrix(ln_tau_out, ln_tau_pfrt, order=2, epsilon=5):
    """evaluation.get_similarity_function('gaussian') on the grid differences (drt1d.py:2843-2847): (len(out), len(pfrt))"""
    d = np.asarray(ln_tau_out, dtype=float)[:, None] - np.asarray(ln_tau_pfrt, dtype=float)[None, :]
    return np.exp(-(epsilon * np.abs(d)) ** (2 * order))


def smooth(raw, ln_tau_out, ln_tau_pfrt, order=2, epsilon=5):
    """smooth_matrix @ raw, every row summed in ascending order of the tau_pfrt grid"""
    raw = np.asarray(raw, dtype=float)
    nz = np.nonzero(raw)[0]
    sm = smooth_matrix(ln_tau_out, np.asarray(ln_tau_pfrt, dtype=float)[nz], order, epsilon)
    out = np.zeros(sm.shape[0])
    for c, j in enumerate(nz):
        out = out + sm[:, c] * raw[j]
    return out


def get_peak_ranges(pf, min_prob):
    """pfrt.get_peak_ranges: (starts, ends) of the contiguous ranges [start, end) with pf >= min_prob (none: two empty arrays;
    upstream raises on its empty index array)"""
    index = np.where(np.asarray(pf, dtype=float) >= min_prob)[0]
    if len(index) == 0:
        return np.zeros(0, dtype=np.intp), np.zeros(0, dtype=np.intp)
    cut = np.where(np.diff(index) > 1)[0] + 1
    starts = np.concatenate([[0], cut])
    ends = np.concatenate([cut, [len(index)]])
    return index[starts], index[ends - 1] + 1


def identify_peaks(pf, min_prob):
    """pfrt.identify_peaks: the first maximum of pf inside every range"""
    pf = np.asarray(pf, dtype=float)
    return np.array([s + int(np.argmax(pf[s:e])) for s, e in zip(*get_peak_ranges(pf, min_prob))], dtype=np.intp)


def integrate_peaks(pf, min_prob):
    """pfrt.integrate_peaks -> (peak indices, areas): np.trapezoid(pf[start - 1:end + 1]) with unit spacing.  For a range that
    starts at index 0 the slice pf[-1:end + 1] is empty (or one sample) and the area is 0, as upstream."""
    pf = np.asarray(pf, dtype=float)
    areas = []
    for s, e in zip(*get_peak_ranges(pf, min_prob)):
        seg = pf[s - 1:e + 1]
        a = 0.0
        for i in range(len(seg) - 1):
            a += (seg[i + 1] + seg[i]) / 2.0
        areas.append(a)
    return identify_peaks(pf, min_prob), np.array(areas, dtype=float)


def finish(raw, ln_tau_pfrt, ln_tau_out=None, smooth_on=True, smooth_order=2, smooth_epsilon=5, integrate=False,
           integrate_threshold=1e-6, normalize=True):
    """drt1d.py:2840-2858 on the raw PFRT: smoothing (onto ln_tau_out; None: the tau_pfrt grid), integration, normalisation"""
    tot = np.asarray(raw, dtype=float)
    if smooth_on:
        tot = smooth(tot, ln_tau_pfrt if ln_tau_out is None else ln_tau_out, ln_tau_pfrt, smooth_order, smooth_epsilon)
    if integrate:
        idx, area = integrate_peaks(tot, integrate_threshold)
        tot = np.zeros_like(tot)
        tot[idx] = area
    if normalize:
        with np.errstate(invalid='ignore', divide='ignore'):
            tot = tot / np.max(tot)
    return tot


def predict_pfrt_rows(factors, llh, f, fxx, var_f, var_fxx, ln_tau_pfrt, ln_tau_out=None, search=1, height=1e-3,
                      prominence=5e-3, prior_mu=-4, prior_sigma=0.5, n_eff_factor=0.5, fxx_var_floor=1e-5, ext_left=-1,
                      ext_right=-1, smooth=True, smooth_order=2, smooth_epsilon=5, integrate=False, integrate_threshold=1e-6,
                      normalize=True):
    """DRT.predict_pfrt on given rows: factors, llh (S,); f, fxx, var_f, var_fxx (S, n) of every step on the tau_pfrt grid ->
    dict(pfrt (len(ln_tau_out),), raw_pfrt (n,), step_pfrt (S, n), post_prob (S,))"""
    post = step_posterior(factors, llh, prior_mu, prior_sigma, n_eff_factor)
    steps = np.array([step_peak_probs(f[i], fxx[i], var_f[i], var_fxx[i], search, height, prominence, fxx_var_floor, ext_left,
                                      ext_right) for i in range(len(post))])
    raw = combine(post, steps)
    out = finish(raw, ln_tau_pfrt, ln_tau_out, smooth, smooth_order, smooth_epsilon, integrate, integrate_threshold, normalize)
    return dict(pfrt=out, raw_pfrt=raw, step_pfrt=steps, post_prob=post)


# ---- select_pfrt_candidates (hybdrt/models/pfrt.py:49-213) ------------------------------------------------------------------------
def rank_peaks(pf, min_prob):
    """pfrt.rank_peaks(integrate=True): (peak indices, areas) by descending area.  Equal areas put the higher index first: what
    np.argsort(areas)[::-1] gives for the at most 16 entries numpy sorts by insertion, made the rule for any count."""
    idx, area = integrate_peaks(pf, min_prob)
    order = np.array(sorted(range(len(area)), key=lambda r: (-area[r], -r)), dtype=np.intp)
    return idx[order], area[order]


def shift_candidate(cand_pf, ranges, peak_indices):
    """pfrt.shift_candidate_pfrt: every entry > 0 at ti moves to the peak index of the one range with start <= ti <= end (end is
    the exclusive end, so the point one past a range still belongs to it) and stays where it is otherwise.  Entries that land on
    the same peak: the highest ti wins, as numpy's fancy assignment in ascending ti leaves it."""
    cand_pf = np.asarray(cand_pf, dtype=float)
    starts, ends = ranges
    out = np.zeros(len(cand_pf))
    for ti in np.where(cand_pf > 0)[0]:
        match = [r for r in range(len(starts)) if starts[r] <= ti <= ends[r]]
        out[peak_indices[match[0]] if len(match) == 1 else ti] = cand_pf[ti]
    return out


def _corr(target, cand):
    """np.corrcoef(target, cand)[0, 1] with np.cov's steps in one fixed order: both rows centred by their means, the three sums of
    products in ascending index order, each times 1 / (n - 1), the covariance divided by the two standard deviations in turn,
    the result clipped to [-1, 1]"""
    n = len(cand)
    seq = lambda v: np.cumsum(v)[-1]          # (np.cumsum adds one term after the other: the sum in ascending index order)
    with np.errstate(invalid='ignore', divide='ignore'):
        target, cand = np.asarray(target, dtype=float), np.asarray(cand, dtype=float)
        dt, dc = target - seq(target) / np.float64(n), cand - seq(cand) / np.float64(n)
        stt, scc, stc = seq(dt * dt), seq(dc * dc), seq(dt * dc)
        fac = np.float64(1.0) / np.float64(n - 1)
        r = ((stc * fac) / np.sqrt(stt * fac)) / np.sqrt(scc * fac)
    if r > 1.0:
        r = np.float64(1.0)
    if r < -1.0:
        r = np.float64(-1.0)
    return r


def candidate_corr(target_indices, cand_pf):
    """pfrt.candidate_corr: the correlation of the 0/1 row with ones at target_indices and the (shifted) candidate row; an
    all-zero candidate row gives NaN"""
    cand_pf = np.asarray(cand_pf, dtype=float)
    target = np.zeros(len(cand_pf))
    target[np.asarray(target_indices, dtype=np.intp)] = 1.0
    return _corr(target, cand_pf)


def select_compact(tot_pf, step_pfs, step_llh, start_thresh=0.99, end_thresh=0.01, peak_thresh=1e-6):
    """pfrt.select_candidates in the compact form the device writes -> dict(num_peaks K, ranked_index (K,), magnitude (K,)
    normalised by the largest, first (the prefix length minus one of the first target), num_candidates, step_index and
    match_quality (num_candidates,)).  Candidate j has target ranked_index[:first + j + 1] and step step_index[j], the np.argmax
    of corr * llh over the steps (the first NaN wins); match_quality[j] is that winning value.  K peaks give at most K - 1
    candidates.  A row with no value at or above peak_thresh raises ValueError."""
    tot_pf, step_llh = np.asarray(tot_pf, dtype=float), np.asarray(step_llh, dtype=float)
    ranges = get_peak_ranges(tot_pf, peak_thresh)
    if len(ranges[0]) == 0:
        raise ValueError('select_candidates: no value of the PFRT at or above peak_thresh')
    peak_indices = identify_peaks(tot_pf, peak_thresh)
    shifted = [shift_candidate(c, ranges, peak_indices) for c in step_pfs]
    ranked, mag = rank_peaks(tot_pf, peak_thresh)
    with np.errstate(invalid='ignore', divide='ignore'):
        mag = mag / np.max(mag)
    K = len(mag)
    inc = np.where(mag >= start_thresh)[0]
    first = inc = int(inc[-1]) if len(inc) > 0 else 0
    step_index, quality = [], []
    while inc < K - 1:
        mq = np.array([candidate_corr(ranked[:inc + 1], sh) * llh for sh, llh in zip(shifted, step_llh)])
        step_index.append(int(np.argmax(mq)))
        quality.append(mq[step_index[-1]])
        inc += 1
        if mag[inc] < end_thresh:
            break
    return dict(num_peaks=K, ranked_index=np.asarray(ranked, dtype=np.intp), magnitude=mag, first=first,
                num_candidates=len(step_index), step_index=np.array(step_index, dtype=np.intp),
                match_quality=np.array(quality, dtype=float))


def candidates_from_compact(c):
    """the compact form -> upstream's (target_peak_indices, candidate_indices): a list of index arrays and a list of step indices"""
    ranked, first = np.asarray(c['ranked_index'], dtype=np.intp), int(c['first'])
    n = int(c['num_candidates'])
    return [ranked[:first + j + 1].copy() for j in range(n)], [int(s) for s in np.asarray(c['step_index'])[:n]]


def select_candidates(tot_pf, step_pfs, step_llh, start_thresh=0.99, end_thresh=0.01, peak_thresh=1e-6):
    """pfrt.select_candidates (hybdrt/models/pfrt.py:164-213, without its print) -> (target_peak_indices, candidate_indices)"""
    return candidates_from_compact(select_compact(tot_pf, step_pfs, step_llh, start_thresh, end_thresh, peak_thresh))
