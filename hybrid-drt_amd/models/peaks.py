"""Peak finding on rows of the DRT's curvature: the numpy statement of csrc/peaks.hip (as models/kk.py is of csrc/kk.hip).

``find_peaks_1d`` restates scipy.signal.find_peaks(v, height=, prominence=) (_local_maxima_1d, _peak_prominences without wlen);
on top of it sit DRT.find_peaks (hybdrt/models/drt1d.py:3753-3947), curvature.peak_prob_1d (hybdrt/mapping/curvature.py:12-58)
and the elementwise formula of DRTMD.predict_curv_prob (hybdrt/mapping/drtmd.py:1100-1104).  Everything acts on rows that are
already evaluated: fxx (order 2), f (order 0) and their posterior variances.  No scipy: the product layer does not depend on it.

``peak_trough_probs_rows`` and its neighbours state csrc/peak_prob.hip: DRT.predict_peak_trough_probs, predict_peak_prob and
find_peaks_byprob (drt1d.py:3655-3750) over surface.peak_prob / trough_prob (hybdrt/mapping/surface.py:265-350), filters.std_filter
(hybdrt/filters/_filters.py:29-40) and peaks.find_peaks_byrange (hybdrt/peaks.py:423-441), on the rows of orders 0, 1, 2.

The last part states csrc/peak_resolve.hip: peaks.find_troughs and peaks.estimate_peak_weight_distributions
(hybdrt/peaks.py:92-217) under DRT.estimate_peak_coef, estimate_peak_drts, quantify_peaks (drt1d.py:3949-4111), split_r_p and
integrate_drt (3586-3620).  Upstream's np.log(tau_i / trough) is taken as a difference of the ln grids (a rounding-level deviation).
"""
import math

import numpy as np

from ..filters.ndfilters import reflect_index

SQRT2 = 2 ** 0.5
METHODS = ('thresh', 'prob')
_erfc = np.vectorize(math.erfc, otypes=[float])


def find_peaks_1d(v, height=None, prominence=None):
    """scipy.signal.find_peaks(v, height=height, prominence=prominence) -> (indices, dict(peak_heights, prominences,
    left_bases, right_bases)).  None switches a condition off (the properties are returned all the same)."""
    v = np.asarray(v, dtype=float).tolist()          # (plain floats: the loops below are the statement, not numpy's)
    n = len(v)
    peaks = []
    i = 1
    while i < n - 1:
        if v[i - 1] < v[i]:
            a = i + 1
            while a < n - 1 and v[a] == v[i]:
                a += 1
            if v[a] < v[i]:
                peaks.append((i + a - 1) // 2)
                i = a
                continue
        i += 1
    idx, hts, proms, lbs, rbs = [], [], [], [], []
    for p in peaks:
        if height is not None and not v[p] >= height:
            continue
        lmin, lb, i = v[p], p, p
        while i >= 0 and v[i] <= v[p]:
            if v[i] < lmin:
                lmin, lb = v[i], i
            i -= 1
        rmin, rb, i = v[p], p, p
        while i < n and v[i] <= v[p]:
            if v[i] < rmin:
                rmin, rb = v[i], i
            i += 1
        prom = v[p] - max(lmin, rmin)
        if prominence is not None and not prom >= prominence:
            continue
        idx.append(p); hts.append(v[p]); proms.append(prom); lbs.append(lb); rbs.append(rb)
    return np.array(idx, dtype=np.intp), dict(peak_heights=np.array(hts, dtype=float), prominences=np.array(proms, dtype=float),
                                              left_bases=np.array(lbs, dtype=np.intp), right_bases=np.array(rbs, dtype=np.intp))


def auto_thresholds(fxx, method, prominence=None, height=None):
    """drt1d.py:3846-3858 -> (prominence, height); method 'thresh', or 'prob' (also the map forms' defaults)"""
    if prominence is None:
        fxx = np.asarray(fxx, dtype=float)
        prominence = 0.05 * np.std(fxx[~np.isinf(fxx)]) + 5e-3 if method == 'thresh' else 5e-3
    if height is None:
        height = 0 if method == 'thresh' else 1e-3
    return prominence, height


def search_peaks(fxx, f, search, height, prominence):
    """drt1d.py:3886-3913 -> (indices, info, signs).  search = +1 / -1: one pass on -search * fxx; 0: the passes -1 and +1, each
    keeping the peaks with pass * f[p] > 0, merged in ascending index.  signs: the pass every peak came from."""
    fxx = np.asarray(fxx, dtype=float)
    if search != 0:
        idx, info = find_peaks_1d(-search * fxx, height, prominence)
        return idx, info, np.full(len(idx), search, dtype=np.intp)
    f = np.asarray(f, dtype=float)
    parts = []
    for s in (-1, 1):
        idx, info = find_peaks_1d(-s * fxx, height, prominence)
        pos = s * f[idx] > 0
        parts.append((idx[pos], {k: w[pos] for k, w in info.items()}, np.full(int(np.sum(pos)), s, dtype=np.intp)))
    idx = np.concatenate([q[0] for q in parts])
    order = np.argsort(idx, kind='stable')
    info = {k: np.concatenate([q[1][k] for q in parts])[order] for k in parts[0][1]}
    return idx[order], info, np.concatenate([q[2] for q in parts])[order]


def extend_var(var, ext_left=-1, ext_right=-1, floor=0.0):
    """estimate_distribution_cov's extend_var clamp (drt1d.py:3123-3140; -1: off) and var_floor (3142-3146) on one row"""
    var = np.array(var, dtype=float)
    if ext_left >= 0:
        var[:ext_left] = np.maximum(var[:ext_left], var[ext_left])
    if ext_right >= 0:
        var[ext_right:] = np.maximum(var[ext_right:], var[ext_right])
    if floor > 0:
        var[var < floor] = floor
    return var


def peak_probs(min_prom, sigma):
    """drt1d.py:3927: 1 - 2 Phi(0; min_prom, sigma) = 1 - erfc(min_prom / (sigma sqrt 2))"""
    min_prom, sigma = np.asarray(min_prom, dtype=float), np.asarray(sigma, dtype=float)
    with np.errstate(divide='ignore', invalid='ignore'):
        return 1.0 - _erfc(min_prom / (sigma * SQRT2))


def _upper(mu, sigma):
    """1 - Phi(0; mu, sigma)"""
    with np.errstate(divide='ignore', invalid='ignore'):
        return 1.0 - 0.5 * _erfc(np.asarray(mu, dtype=float) / (np.asarray(sigma, dtype=float) * SQRT2))


def find_peaks_row(fxx, f=None, var_fxx=None, search=1, method='thresh', prominence=None, height=None, prob_thresh=0.25,
                   num_peaks=None, fxx_var_floor=1e-5, ext_left=-1, ext_right=-1):
    """DRT.find_peaks on evaluated rows -> (kept indices, all indices, info, signs, used prominence).  info has scipy's four keys and,
    for 'prob', 'probs'; like upstream it covers every peak that passed height and prominence (and the f test), kept or not.
    var_fxx: the curvature's variance before extend_var and the floor ('prob' only)."""
    if method not in METHODS:
        raise ValueError(f'Invalid method {method}. Options: {list(METHODS)}')
    prominence, height = auto_thresholds(fxx, method, prominence, height)
    idx, info, signs = search_peaks(fxx, f, search, height, prominence)
    kept = idx
    if method == 'prob':
        min_prom = np.minimum(info['prominences'], info['peak_heights'])
        sigma = extend_var(var_fxx, ext_left, ext_right, fxx_var_floor) ** 0.5
        prob = peak_probs(min_prom, sigma[idx])
        if num_peaks is not None and len(prob):
            prob_thresh = np.sort(prob)[::-1][min(num_peaks - 1, len(prob) - 1)]
        kept = idx[prob >= prob_thresh]
        info['probs'] = prob
    return kept, idx, info, signs, prominence


def peak_prob_row(f, fxx, var_f, var_fxx, search=1, height=1e-3, prominence=5e-3):
    """curvature.peak_prob_1d times sign(f) (drtmd.py:1064) on one row; the variances as they enter the square root"""
    f = np.asarray(f, dtype=float)
    idx, probs = _peak_prob_at_peaks(f, fxx, var_f, var_fxx, search, height, prominence)
    out = np.zeros(len(f))
    out[idx] = probs
    return out * np.sign(f)


def _peak_prob_at_peaks(f, fxx, var_f, var_fxx, search, height, prominence, found=None):
    """curvature.py:46-53 -> (indices, min(curvature probability, probability that |f| > 0)); found: search_peaks' result"""
    f, fxx = np.asarray(f, dtype=float), np.asarray(fxx, dtype=float)
    idx, info = found if found is not None else search_peaks(fxx, f, search, height, prominence)[:2]
    min_prom = np.minimum(info['prominences'], info['peak_heights'])
    curv = _upper(min_prom, np.asarray(var_fxx, dtype=float)[idx] ** 0.5)
    fpr = _upper(np.sign(f[idx]) * f[idx], np.asarray(var_f, dtype=float)[idx] ** 0.5)
    return idx, np.minimum(curv, fpr)


def curv_prob_row(f, fxx, var_f, var_fxx):
    """DRTMD.predict_curv_prob's formula (drtmd.py:1097-1104), elementwise"""
    f, fxx = np.asarray(f, dtype=float), np.asarray(fxx, dtype=float)
    f_prob = _upper(-np.sign(fxx) * f, np.asarray(var_f, dtype=float) ** 0.5)
    c_prob = _upper(-np.sign(f) * fxx, np.asarray(var_fxx, dtype=float) ** 0.5)
    f_prob = 2 * np.maximum(f_prob - 0.5, 0)
    c_prob = 2 * np.maximum(c_prob - 0.5, 0)
    return np.minimum(f_prob, c_prob) * np.sign(f)


def find_peaks_dense(fxx, f=None, var_fxx=None, var_f=None, search=1, method=0, prominence=None, height=None, prob_thresh=0.25,
                     num_peaks=0, fxx_var_floor=1e-5, ext_left=-1, ext_right=-1):
    """What peaks_kernel writes for one row, dense on the evaluation grid: dict(peak_sign, keep, heights, prominences, probs,
    left_bases, right_bases, count, used_prominence) and for method 2 also peak_prob and curv_prob.  method 0 'thresh', 1 'prob',
    2 the map probabilities (the thresholds default as for 'prob'; extend_var acts on both variances, the floor on var_fxx)."""
    fxx = np.asarray(fxx, dtype=float)
    n = len(fxx)
    name = 'thresh' if method == 0 else 'prob'
    out = dict(peak_sign=np.zeros(n, dtype=np.int32), keep=np.zeros(n, dtype=np.int32), heights=np.zeros(n), prominences=np.zeros(n),
               probs=np.zeros(n), left_bases=np.full(n, -1, dtype=np.int32), right_bases=np.full(n, -1, dtype=np.int32))
    if method == 2:
        prominence, height = auto_thresholds(fxx, name, prominence, height)
        idx, info, signs = search_peaks(fxx, f, search, height, prominence)
        vxx = extend_var(var_fxx, ext_left, ext_right, fxx_var_floor)
        vf = extend_var(var_f, ext_left, ext_right, 0.0)
        idx, info['probs'] = _peak_prob_at_peaks(f, fxx, vf, vxx, search, height, prominence, found=(idx, info))
        out['peak_prob'] = np.zeros(n)
        out['peak_prob'][idx] = info['probs']
        out['peak_prob'] *= np.sign(f)
        out['curv_prob'] = curv_prob_row(f, fxx, vf, vxx)
        kept, used = idx, prominence
    else:
        kept, idx, info, signs, used = find_peaks_row(fxx, f, var_fxx, search, name, prominence, height, prob_thresh,
                                                      num_peaks if num_peaks else None, fxx_var_floor, ext_left, ext_right)
    out['peak_sign'][idx] = signs
    out['keep'][kept] = 1
    out['heights'][idx], out['prominences'][idx] = info['peak_heights'], info['prominences']
    out['left_bases'][idx], out['right_bases'][idx] = info['left_bases'], info['right_bases']
    if 'probs' in info:
        out['probs'][idx] = info['probs']
    out['count'], out['used_prominence'] = len(kept), float(used)
    return out


# ---- peak and trough probabilities and the search on their product: the numpy statement of csrc/peak_prob.hip -------------------
def _phi(z):
    """scipy.stats.norm.cdf: Phi(z) = erfc(-z / sqrt 2) / 2"""
    with np.errstate(divide='ignore', invalid='ignore'):
        return 0.5 * _erfc(-np.asarray(z, dtype=float) / SQRT2)


def linear_quantile(srt, q):
    """np.percentile(srt, 100 q) of an ascending row, numpy's default 'linear' method: the virtual index q (n - 1), interpolated
    with numpy's _lerp -- a + (b - a) t, and b - (b - a) (1 - t) for t >= 0.5"""
    n = len(srt)
    vi = (n - 1) * q
    lo = int(math.floor(vi))
    hi = min(lo + 1, n - 1)
    t, a, b = vi - lo, float(srt[lo]), float(srt[hi])
    d = b - a
    return b - d * (1.0 - t) if t >= 0.5 else a + d * t


def sigma_floor_value(sigma):
    """drt1d.py:3677-3678: np.median(sigma) - 1.5 * (np.percentile(sigma, 75) - np.percentile(sigma, 25)); the median is the
    mean of the two middle samples for even n"""
    srt = np.sort(np.asarray(sigma, dtype=float))
    n = len(srt)
    med = float(srt[n // 2]) if n % 2 else (float(srt[n // 2 - 1]) + float(srt[n // 2])) / 2.0
    return med - 1.5 * (linear_quantile(srt, 0.75) - linear_quantile(srt, 0.25))


def sigma_floor(sigma):
    """drt1d.py:3676-3679 on one row: sigma[sigma < floor] = floor"""
    sigma = np.array(sigma, dtype=float)
    fl = sigma_floor_value(sigma)
    sigma[sigma < fl] = fl
    return sigma


def _window_mean(row, size):
    """scipy.ndimage.uniform_filter(row, size, mode='reflect') over masked_filter's mask of ones (whose filtered value is 1):
    the terms of a window added in ascending offset, divided by size"""
    n, h = len(row), size // 2
    pos = np.arange(n)
    tot = np.zeros(n)
    for j in range(-h, h + 1):
        tot = tot + row[reflect_index(pos + j, n)]
    return tot / size


def filtered_sigma(row, size=5, baseline=0.1):
    """surface.py:272-274 with f_var=None: std_filter(row, size, mask=ones) + baseline * np.std(row).  std_filter
    (_filters.py:29-40) is the windowed mean of the squared deviations from the windowed mean ROW, negatives set to 0, rooted."""
    row = np.asarray(row, dtype=float)
    if size < 3 or size % 2 != 1:
        raise ValueError('size must be odd and at least 3')
    mean = _window_mean(row, size)
    var = _window_mean((row - mean) ** 2, size)
    var[var < 0] = 0
    return var ** 0.5 + baseline * np.std(row)


def peak_trough_probs_rows(f, fx, fxx, var_f=None, var_fx=None, var_fxx=None, std_size=5, std_baseline=0.1, floor=True,
                           ext_left=-1, ext_right=-1, sigma=None):
    """DRT.predict_peak_trough_probs on evaluated rows -> (pp, tp, sigma (3, n)).  With the variances (bayes_cov=True; before
    extend_var) sigma is the root after the clamp, floored per order (drt1d.py:3670-3680); without them the filtered sigma of
    every row (surface.py:272-291); sigma (3, n): the rows as they enter the formulas, given.  surface.peak_prob
    (constrain_sign=False) and trough_prob follow (surface.py:293-309, 336-350)."""
    f, fx, fxx = (np.asarray(r, dtype=float) for r in (f, fx, fxx))
    if sigma is not None:
        sig = [np.asarray(s, dtype=float) for s in sigma]
    elif var_f is None:
        sig = [filtered_sigma(r, std_size, std_baseline) for r in (f, fx, fxx)]
    else:
        sig = [extend_var(v, ext_left, ext_right) ** 0.5 for v in (var_f, var_fx, var_fxx)]
        if floor:
            sig = [sigma_floor(s) for s in sig]
    sf, sx, sxx = sig
    sg = np.sign(f)
    with np.errstate(divide='ignore', invalid='ignore'):
        fxx_prob = 1.0 - _phi(sg * fxx / sxx)
        fx_prob = _phi((5.0 * sx - fx) / sx) - _phi((-5.0 * sx - fx) / sx)
        f_prob = 1.0 - _phi((sf - np.abs(f)) / sf)
        pp = f_prob * fx_prob * fxx_prob
        tp = fx_prob * (1.0 - _phi(-sg * fxx / sxx))
    return pp, tp, np.array(sig)


def peak_prob_of(pp, tp):
    """DRT.predict_peak_prob (drt1d.py:3718)"""
    return pp * (1.0 - tp)


def find_peaks_byrange(tau, prob, ranges):
    """peaks.find_peaks_byrange (hybdrt/peaks.py:423-441): per range (t0, t1) np.argmax of prob with every sample outside it
    set to zero -- the first maximum; index 0 when nothing in the window is positive"""
    tau, prob = np.asarray(tau, dtype=float), np.asarray(prob, dtype=float)
    out = []
    for t0, t1 in ranges:
        g = prob.copy()
        g[(tau < t0) | (tau > t1)] = 0
        out.append(int(np.argmax(g)))
    return np.array(out, dtype=np.intp)


def range_windows(tau, ranges):
    """the index windows [lo, hi] (an (nranges, 2) array) that find_peaks_byrange's masks tau < t0, tau > t1 leave on a strictly
    increasing grid; an empty window is (0, -1)"""
    tau = np.asarray(tau, dtype=float)
    if tau.ndim != 1 or np.any(np.diff(tau) <= 0):
        raise ValueError('tau must be strictly increasing')
    win = []
    for t0, t1 in ranges:
        lo, hi = int(np.sum(tau < t0)), len(tau) - 1 - int(np.sum(tau > t1))
        win.append((lo, hi) if lo <= hi else (0, -1))
    return np.array(win, dtype=np.intp).reshape(-1, 2)


def find_peaks_byindex(prob, windows):
    """find_peaks_byrange on index windows [lo, hi]: what peak_trough_prob_kernel's search 2 writes for one row"""
    prob = np.asarray(prob, dtype=float)
    out = []
    for lo, hi in windows:
        g = np.zeros(len(prob))
        g[lo:hi + 1] = prob[lo:hi + 1]
        out.append(int(np.argmax(g)))
    return np.array(out, dtype=np.intp)


def find_peaks_byprob_row(prob, height=None, prominence=None):
    """find_peaks_byprob with thresholds (drt1d.py:3744): scipy.signal.find_peaks(prob, height=, prominence=) -> (indices, info);
    like scipy, info carries peak_heights only with a height and prominences, left_bases, right_bases only with a prominence"""
    idx, info = find_peaks_1d(prob, height, prominence)
    keys = (('peak_heights',) if height is not None else ()) + \
        (('prominences', 'left_bases', 'right_bases') if prominence is not None else ())
    return idx, {k: info[k] for k in keys}


def find_peaks_byprob_dense(prob, height=None, prominence=None):
    """What peak_trough_prob_kernel's search 1 writes for one row, dense on the grid: dict(keep, heights, prominences, left_bases,
    right_bases, count); heights and prominences are reported whether their condition is on or not"""
    prob = np.asarray(prob, dtype=float)
    n = len(prob)
    idx, info = find_peaks_1d(prob, height, prominence)
    out = dict(keep=np.zeros(n, dtype=np.int32), heights=np.zeros(n), prominences=np.zeros(n),
               left_bases=np.full(n, -1, dtype=np.int32), right_bases=np.full(n, -1, dtype=np.int32), count=len(idx))
    out['keep'][idx] = 1
    out['heights'][idx], out['prominences'][idx] = info['peak_heights'], info['prominences']
    out['left_bases'][idx], out['right_bases'][idx] = info['left_bases'], info['right_bases']
    return out


# ---- per-peak coefficients, distributions and resistances: the numpy statement of csrc/peak_resolve.hip ------------------------
def find_troughs(f, fxx, peak_indices):
    """peaks.find_troughs (hybdrt/peaks.py:92-136) for sorted peak indices -> one trough index per neighbouring pair"""
    f, fxx = np.asarray(f, dtype=float), np.asarray(fxx, dtype=float)
    f_mix = -(f - fxx)
    pk = sorted(int(p) for p in peak_indices)
    troughs = []
    for s, e in zip(pk[:-1], pk[1:]):
        ls, rs = np.sign(f[s]), np.sign(f[e])
        if ls == rs:
            v = ls * f[s:e]
            if np.min(v) < min(ls * f[s], ls * f[e]):
                t = s + int(np.argmin(v))
            else:
                t = s + int(np.argmax(ls * f_mix[s:e]))
                if t in (s, e):
                    t = int((s + e + 2 * t) / 4)
        else:
            t = s + int(np.argmin(np.abs(f[s:e])))
        troughs.append(t)
    return np.array(troughs, dtype=np.intp)


def peak_epsilons(ln_tau, peak_indices, trough_indices, epsilon_factor=1.25, max_epsilon=1.25, min_epsilon=None,
                  epsilon_uniform=None):
    """the inverse length scales of every peak's weighting function (hybdrt/peaks.py:164-199) -> (eps_l, eps_r); a zero
    distance gives +inf and hence max_epsilon, as IEEE division gives upstream"""
    lt = np.asarray(ln_tau, dtype=float)
    P = len(peak_indices)
    eps_l, eps_r = np.empty(P), np.empty(P)
    for i, p in enumerate(peak_indices):
        if epsilon_uniform is not None:
            eps_l[i] = eps_r[i] = epsilon_uniform
            continue
        prev = lt[0] if i == 0 else lt[trough_indices[i - 1]]
        nxt = lt[-1] if i == P - 1 else lt[trough_indices[i]]
        with np.errstate(divide='ignore'):
            el = min(np.float64(epsilon_factor) / (lt[p] - prev), max_epsilon)
            er = min(np.float64(epsilon_factor) / (nxt - lt[p]), max_epsilon)
        if min_epsilon is not None:
            el, er = max(el, min_epsilon), max(er, min_epsilon)
        eps_l[i], eps_r[i] = el, er
    return eps_l, eps_r


def peak_weights(ln_basis, ln_peak, eps_l, eps_r):
    """hybdrt/peaks.py:201-217: w[i][j] = exp(-(eps y)^2), y = ln_basis[j] - ln_peak[i], eps_l left of the peak and eps_r on it and
    right of it, every column divided by its sum over the peaks (0 / 0 = NaN where all weights underflow: more than about 9.5
    decades from every peak at eps = 1.25).  One peak or none: ones."""
    lb = np.asarray(ln_basis, dtype=float)
    P = len(ln_peak)
    if P <= 1:
        return np.ones((P, len(lb)))
    w = np.empty((P, len(lb)))
    for i in range(P):
        y = lb - ln_peak[i]
        w[i] = np.exp(-(np.where(y < 0, eps_l[i], eps_r[i]) * y) ** 2)
    tot = np.zeros(len(lb))
    for i in range(P):                                   # (ascending i)
        tot = tot + w[i]
    with np.errstate(invalid='ignore', divide='ignore'):
        return w / tot


def trapezoid(y, x):
    """np.trapezoid(y, x=x): the sum of the terms (dx (y1 + y0)) / 2 (the kernels add them in a fixed order of their own)"""
    y, x = np.asarray(y, dtype=float), np.asarray(x, dtype=float)
    if len(y) < 2:
        return 0.0
    return float(np.sum((np.diff(x) * (y[1:] + y[:-1])) / 2.0))


def resolve_peaks_row(f, fxx, peak_indices, x_red, ln_tau_find, ln_basis, e0=None, ln_tau_out=None, basis_area=1.0,
                      epsilon_factor=1.25, max_epsilon=1.25, min_epsilon=None, epsilon_uniform=None):
    """estimate_peak_coef / estimate_peak_drts / quantify_peaks for one spectrum on evaluated rows -> dict(peak_index, troughs,
    eps_l, eps_r, x_peaks (P, nb), peak_gammas (P, nout), r_peaks (P,), r_coef (P,)).  f, fxx: the unnormalised rows on the find
    grid; x_red: get_drt_params in data units; e0: the order-0 evaluation matrix (nout, nb) of the output grid (None: no
    peak_gammas / r_peaks); basis_area = sqrt(pi) / epsilon of the basis (predict_r_p)."""
    pk = np.array(sorted(int(p) for p in peak_indices), dtype=np.intp)
    lt, lb, x_red = np.asarray(ln_tau_find, dtype=float), np.asarray(ln_basis, dtype=float), np.asarray(x_red, dtype=float)
    tr = find_troughs(f, fxx, pk)
    eps_l, eps_r = peak_epsilons(lt, pk, tr, epsilon_factor, max_epsilon, min_epsilon, epsilon_uniform)
    w = peak_weights(lb, lt[pk], eps_l, eps_r)
    x_peaks = x_red * w
    out = dict(peak_index=pk, troughs=tr, eps_l=eps_l, eps_r=eps_r, x_peaks=x_peaks,
               r_coef=np.array([np.sum(xp) * basis_area for xp in x_peaks]))
    if e0 is not None:
        out['peak_gammas'] = x_peaks @ np.asarray(e0, dtype=float).T
        out['r_peaks'] = np.array([trapezoid(g, ln_tau_out) for g in out['peak_gammas']])
    return out


def nearest_index(arr, val):
    """utils.array.nearest_index without a constraint: the first minimum of |arr - val|"""
    return int(np.argmin(np.abs(np.asarray(arr, dtype=float) - val)))


def split_windows(tau, tau_splits):
    """split_r_p's windows (drt1d.py:3606-3608) -> (start, end): [start, end) with end = split + 1, the last one len(tau) + 1
    (numpy's slice clips it)"""
    split = [nearest_index(tau, ts) for ts in sorted(tau_splits)]
    return np.array([0] + split, dtype=np.intp), np.array(split + [len(tau)], dtype=np.intp) + 1


def window_peaks(fxx, start, end):
    """split_r_p(resolve_peaks=True): one peak per window, i + argmin(fxx[i:j])"""
    fxx = np.asarray(fxx, dtype=float)
    return np.array([i + int(np.argmin(fxx[i:j])) for i, j in zip(start, end)], dtype=np.intp)


def window_integrals(gamma, ln_tau, start, end):
    """split_r_p without resolve_peaks and integrate_drt: the trapezoid of one row over every window [start, end)"""
    gamma, ln_tau = np.asarray(gamma, dtype=float), np.asarray(ln_tau, dtype=float)
    return np.array([trapezoid(gamma[i:j], ln_tau[i:j]) for i, j in zip(start, end)])
