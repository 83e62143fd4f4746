"""The map filters of hybdrt/filters/_filters.py (149-256, 261-475) and the scipy.ndimage pieces they stand on, stated in
numpy alone for 1-D and 2-D arrays with the 'reflect' boundary -- no scipy import.  This is the statement csrc/map_filter.hip
is read against (like models/peaks.py for peaks.hip): every function keeps the reference's signature, defaults and order of
operations, and the correlations keep scipy's order of summation,

    y[i] w[0] + sum_{j = r .. 1} (y[i - j] + y[i + j]) w[j]        (NI_Correlate1D, symmetric table)

so that on the CPU the results agree with the reference to the last bits (tests/map_filter_bounds.json records how closely).
"""
import numbers

import numpy as np


def _check_mode(mode):
    modes = (mode,) if isinstance(mode, str) else tuple(mode)
    if any(m != 'reflect' for m in modes):
        raise NotImplementedError("mode: only the 'reflect' boundary is built")


def _normalize_sequence(value, ndim):
    if np.ndim(value) == 0:
        return [value] * ndim
    value = list(value)
    if len(value) != ndim:
        raise RuntimeError("sequence argument must have length equal to input rank")
    return value


def reflect_index(idx, n):
    """scipy's 'reflect' (d c b a | a b c d | d c b a): period 2 n, mirrored about the half-sample edges; any distance"""
    idx = np.mod(idx, 2 * n)
    return np.where(idx >= n, 2 * n - 1 - idx, idx)


def correlate1d_reflect(a, weights, axis=-1):
    """scipy.ndimage.correlate1d(a, weights, axis, mode='reflect', origin=0) for an odd-length table; a symmetric table is
    summed in scipy's symmetric order, any other in its plain order (left to right)"""
    a = np.asarray(a, dtype=float)
    w = np.asarray(weights, dtype=float)
    if w.ndim != 1 or len(w) % 2 != 1:
        raise ValueError("weights: a 1-D table of odd length")
    r = len(w) // 2
    y = np.moveaxis(a, axis, 0)
    n = y.shape[0]
    pos = np.arange(n)

    def take(shift):
        return y[reflect_index(pos + shift, n)]

    # scipy's test: fabs(fw[ii + size1] - fw[size1 - ii]) > DBL_EPSILON breaks the symmetry
    symmetric = all(abs(w[r + j] - w[r - j]) <= np.finfo(float).eps for j in range(1, r + 1))
    out = y * w[r]
    if symmetric:
        for j in range(r, 0, -1):
            out = out + (take(-j) + take(j)) * w[r - j]
    else:
        out = take(-r) * w[0]
        for j in range(-r + 1, r + 1):
            out = out + take(j) * w[r + j]
    return np.moveaxis(out, 0, axis)


def gaussian_kernel1d(sigma, order, radius, empty=False):
    """scipy.ndimage._filters._gaussian_kernel1d, or _scifilters._empty_gaussian_kernel1d (centre weight zeroed before the
    normalisation) with empty=True"""
    if order < 0:
        raise ValueError('order must be non-negative')
    sigma2 = sigma * sigma
    x = np.arange(-radius, radius + 1)
    phi_x = np.exp(-0.5 / sigma2 * x ** 2)
    if empty:
        phi_x[x == 0] = 0
    phi_x = phi_x / phi_x.sum()
    if order == 0:
        return phi_x
    exponent_range = np.arange(order + 1)
    q = np.zeros(order + 1)
    q[0] = 1
    D = np.diag(exponent_range[1:], 1)
    P = np.diag(np.ones(order) / -sigma2, -1)
    Q_deriv = D + P
    for _ in range(order):
        q = Q_deriv.dot(q)
    q = (x[:, None] ** exponent_range).dot(q)
    return q * phi_x


def kernel_radius(sigma, truncate=4.0, radius=None):
    lw = int(truncate * float(sigma) + 0.5)
    if radius is not None:
        lw = radius
    if not isinstance(lw, numbers.Integral) or lw < 0:
        raise ValueError('Radius must be a nonnegative integer.')
    return lw


def gaussian_filter1d(input, sigma, axis=-1, order=0, mode="reflect", cval=0.0, truncate=4.0, *, radius=None, empty=False):
    """scipy.ndimage.gaussian_filter1d / _scifilters.empty_gaussian_filter1d (empty=True)"""
    _check_mode(mode)
    lw = kernel_radius(sigma, truncate, radius)
    weights = gaussian_kernel1d(sigma, order, lw, empty)[::-1]
    return correlate1d_reflect(input, weights, axis)


def empty_gaussian_filter1d(input, sigma, axis=-1, order=0, mode="reflect", cval=0.0, truncate=4.0, *, radius=None):
    return gaussian_filter1d(input, sigma, axis, order, mode, cval, truncate, radius=radius, empty=True)


def gaussian_filter(input, sigma, order=0, mode="reflect", cval=0.0, truncate=4.0, *, radius=None, empty=False):
    """scipy.ndimage.gaussian_filter: a sequence of 1-D filters over the axes whose sigma exceeds 1e-15"""
    _check_mode(mode)
    out = np.array(input, dtype=float)
    orders = _normalize_sequence(order, out.ndim)
    sigmas = _normalize_sequence(sigma, out.ndim)
    radiuses = _normalize_sequence(radius, out.ndim)
    for axis in range(out.ndim):
        if sigmas[axis] > 1e-15:
            out = gaussian_filter1d(out, sigmas[axis], axis, orders[axis], truncate=truncate, radius=radiuses[axis], empty=empty)
    return out


def empty_gaussian_filter(input, sigma, order=0, mode="reflect", cval=0.0, truncate=4.0, *, radius=None):
    """_scifilters.empty_gaussian_filter (116-177)"""
    return gaussian_filter(input, sigma, order, mode, cval, truncate, radius=radius, empty=True)


def gaussian_laplace1d(input, sigma, axis=-1, mode="reflect", cval=0.0, **kwargs):
    """_scifilters.gaussian_laplace1d (229-253): the order-2 Gaussian along one axis"""
    return gaussian_filter1d(input, sigma, axis, 2, mode, cval, **kwargs)


def uniform_filter1d(input, size, axis=-1, mode="reflect", cval=0.0):
    """scipy.ndimage.uniform_filter1d with origin 0: a running sum along the line, divided by size at every sample"""
    _check_mode(mode)
    if size < 1:
        raise RuntimeError('incorrect filter size')
    y = np.moveaxis(np.asarray(input, dtype=float), axis, 0)
    n = y.shape[0]
    size1 = size // 2
    out = np.empty_like(y)
    tmp = np.zeros(y.shape[1:])
    for j in range(-size1, size - size1):
        tmp = tmp + y[reflect_index(j, n)]
    out[0] = tmp / size
    for l in range(1, n):
        tmp = tmp + (y[reflect_index(l - size1 + size - 1, n)] - y[reflect_index(l - 1 - size1, n)])
        out[l] = tmp / size
    return np.moveaxis(out, 0, axis)


def uniform_filter(input, size=3, mode="reflect", cval=0.0):
    """scipy.ndimage.uniform_filter: uniform_filter1d over the axes whose size exceeds 1"""
    _check_mode(mode)
    out = np.array(input, dtype=float)
    sizes = _normalize_sequence(size, out.ndim)
    for axis in range(out.ndim):
        if sizes[axis] > 1:
            out = uniform_filter1d(out, int(sizes[axis]), axis)
    return out


def rms_filter(a, size, empty=False, **kw):
    """_filters.rms_filter (8-26)"""
    a2 = a ** 2
    a2_mean = uniform_filter(a2, size, **kw)
    if empty:
        if np.isscalar(size):
            n = size ** np.ndim(a)
        else:
            n = np.prod(size)
        a2_mean -= a2 / n
        a2_mean *= n / (n - 1)
    a2_mean[a2_mean < 0] = 0
    return a2_mean ** 0.5


def masked_filter(a, mask, filter_func=None, **filter_kw):
    """_filters.masked_filter (149-175): f(a mask) / f(mask); filter_func defaults to gaussian_filter"""
    if filter_func is None:
        filter_func = gaussian_filter
    mask = mask.astype(float)
    x_filt = filter_func(a * mask, **filter_kw)
    mask_filt = filter_func(mask, **filter_kw)
    with np.errstate(invalid='ignore', divide='ignore'):
        return x_filt / mask_filt


def iterate_gaussian_weights(a, init_weights=None, adaptive=False, iter=2, nstd=5, dev_rms_size=5, nan_mask=None, **filter_kw):
    """_filters.iterate_gaussian_weights (183-232)"""
    weights = np.ones(a.shape) if init_weights is None else init_weights
    if nan_mask is not None:
        weights[nan_mask] = 0
    for _ in range(iter):
        if adaptive:
            sigmas = get_adaptive_sigmas(a, empty=True, weights=weights, **filter_kw)

            def filter_func(a_in, **kw):
                return adaptive_gaussian_filter(a_in, sigmas=sigmas, empty=True, **kw)
        else:
            filter_func = empty_gaussian_filter
        dev = a - masked_filter(a, weights, filter_func=filter_func, **filter_kw)
        dev_rms = masked_filter(dev, weights, rms_filter, size=dev_rms_size, empty=True)
        with np.errstate(invalid='ignore', divide='ignore'):
            weights = np.exp(-(dev / (nstd * dev_rms + 0.1 * np.std(dev))) ** 6)
        if nan_mask is not None:
            weights[nan_mask] = 0
    return weights


def iterative_gaussian_filter(a, adaptive=False, iter=2, nstd=5, dev_rms_size=5, nan_mask=None, fill_nans=False, **filter_kw):
    """_filters.iterative_gaussian_filter (235-256)"""
    weights = iterate_gaussian_weights(a, None, adaptive, iter, nstd, dev_rms_size=dev_rms_size, nan_mask=nan_mask, **filter_kw)
    if adaptive:
        sigmas = get_adaptive_sigmas(a, empty=False, weights=weights, **filter_kw)

        def filter_func(a_in, **kw):
            return adaptive_gaussian_filter(a_in, sigmas=sigmas, **kw)
    else:
        filter_func = gaussian_filter
    out = masked_filter(a, weights, filter_func=filter_func, **filter_kw)
    if nan_mask is not None and not fill_nans:
        out[nan_mask] = np.nan
    return out


def sigma_nodes(sigma_min, sigma_max, sigma_node_factor=1.5, min_sigma=0.25):
    """node grid of _filters.nonuniform_gaussian_filter1d (264-295) from the extremes of the sigma field (as they stand after
    the floor at 1e-8): (nodes, node_delta, floor) -- `floor` is the value the reference raises smaller sigmas to (0: none).
    ceil_arg is returned last: the argument of the ceil that sets the node count (the fixture generator keeps it off integers)."""
    min_ls = max(np.log10(sigma_min), np.log10(min_sigma))
    max_ls = max(np.log10(sigma_max), np.log10(min_sigma))
    ceil_arg = (max_ls - min_ls) / np.log10(sigma_node_factor)
    num_nodes = int(np.ceil(ceil_arg)) + 1
    nodes = np.logspace(min_ls, max_ls, num_nodes)
    floor = 0.0
    if sigma_min < min_sigma:
        factor = nodes[-1] / nodes[-2] if len(nodes) > 1 else sigma_node_factor
        floor = min_sigma / (factor ** 2)
        while nodes[0] > max(sigma_min, floor) * 1.001:
            nodes = np.insert(nodes, 0, nodes[0] / factor)
    node_delta = np.log(nodes[-1] / nodes[-2]) if len(nodes) > 1 else 1
    return nodes, node_delta, floor, ceil_arg


def nonuniform_gaussian_filter1d(a, sigma, axis=-1, empty=False, mode='reflect', cval=0.0, truncate=4, order=0,
                                 sigma_node_factor=1.5, min_sigma=0.25):
    """_filters.nonuniform_gaussian_filter1d (261-345)"""
    _check_mode(mode)
    if not np.max(sigma) > 0:
        return a
    sigma = np.maximum(sigma, 1e-8)
    nodes, node_delta, floor, _ = sigma_nodes(np.min(sigma), np.max(sigma), sigma_node_factor, min_sigma)
    if floor > 0:
        sigma[sigma < floor] = floor
    out = np.zeros(np.shape(a))
    for node in nodes:
        if node < min_sigma and not empty:
            node_out = a
        else:
            node_out = gaussian_filter1d(a, max(node, min_sigma), axis, order, truncate=truncate, empty=empty)
        nw = np.abs(np.log(sigma / node)) / node_delta
        nw[nw >= 1] = 1
        nw = 1 - nw
        out = out + node_out * nw
    return out


def nonuniform_gaussian_filter(a, sigma, empty=False, mode='reflect', cval=0.0, truncate=4, order=0, sigma_node_factor=1.5):
    """_filters.nonuniform_gaussian_filter (348-358)"""
    out = a
    for axis in range(np.ndim(a)):
        out = nonuniform_gaussian_filter1d(out, sigma[axis], axis, empty, mode, cval, truncate, order, sigma_node_factor)
    return out


def get_adaptive_sigma1d(a, axis=-1, presmooth_sigma=1, empty=False, weights=None, curv_func=None, curv_kw=None, k_factor=1.0,
                         max_sigma=5.0, mode='reflect', cval=0.0, truncate=4.0):
    """_filters.get_adaptive_sigma1d (363-413) with the default curvature function (gaussian_laplace1d, curv_sigma = 1)"""
    if curv_func is not None or curv_kw is not None:
        raise NotImplementedError("curv_func / curv_kw: only the default curvature (gaussian_laplace1d, curv_sigma=1) is built")
    _check_mode(mode)
    if not max_sigma > 0:
        return np.zeros_like(a)
    filter_func = empty_gaussian_filter if empty else gaussian_filter
    if np.isscalar(presmooth_sigma):
        presmooth_sigma = [presmooth_sigma] * np.ndim(a)
    if np.max(presmooth_sigma) > 0:
        if weights is None:
            a_smooth = filter_func(a, sigma=presmooth_sigma, truncate=truncate)
        else:
            a_smooth = masked_filter(a, weights, filter_func, sigma=presmooth_sigma, truncate=truncate)
    else:
        a_smooth = a
    curv = gaussian_laplace1d(a_smooth, sigma=1, axis=axis, truncate=truncate)
    curv /= (np.abs(a_smooth) + np.std(a_smooth))
    if np.std(curv) == 0:
        return np.ones(a.shape) * max_sigma
    curv /= np.std(curv)
    curv = gaussian_filter(np.abs(curv), presmooth_sigma)
    c = k_factor / (max_sigma ** 2)
    return (k_factor / (np.abs(curv) + c)) ** 0.5


def get_adaptive_sigmas(a, presmooth_sigma=None, empty=False, weights=None, curv_func=None, curv_kw=None, k_factor=1.0,
                        max_sigma=1.0, mode='reflect', cval=0.0, truncate=4.0):
    """_filters.get_adaptive_sigmas (416-435)"""
    ndim = np.ndim(a)
    if np.isscalar(k_factor):
        k_factor = [k_factor] * ndim
    if np.isscalar(max_sigma):
        max_sigma = [max_sigma] * ndim
    if presmooth_sigma is None:
        presmooth_sigma = max_sigma
    return [get_adaptive_sigma1d(a, axis, presmooth_sigma, empty, weights, curv_func, curv_kw, k_factor[axis], max_sigma[axis],
                                 mode, cval, truncate) for axis in range(ndim)]


def adaptive_gaussian_filter1d(a, sigma=None, axis=-1, presmooth_sigma=1, empty=False, curv_func=None, curv_kw=None, k_factor=1,
                               max_sigma=1.0, mode='reflect', cval=0.0, truncate=4, order=0, sigma_node_factor=1.5):
    """_filters.adaptive_gaussian_filter1d (438-448)"""
    if sigma is None:
        sigma = get_adaptive_sigma1d(a, axis, presmooth_sigma, empty, None, curv_func, curv_kw, k_factor, max_sigma, mode, cval,
                                     truncate)
    return nonuniform_gaussian_filter1d(a, sigma, axis, empty, mode, cval, truncate, order, sigma_node_factor)


def adaptive_gaussian_filter(a, sigmas=None, presmooth_sigma=None, empty=False, curv_func=None, curv_kw=None, k_factor=1,
                             max_sigma=5, mode='reflect', cval=0.0, truncate=4, order=0, sigma_node_factor=1.5):
    """_filters.adaptive_gaussian_filter (451-475)"""
    ndim = np.ndim(a)
    if np.isscalar(k_factor):
        k_factor = [k_factor] * ndim
    if np.isscalar(max_sigma):
        max_sigma = [max_sigma] * ndim
    if sigmas is None:
        sigmas = [None] * ndim
    if presmooth_sigma is None:
        presmooth_sigma = max_sigma
    out = a
    for axis in range(ndim):
        if max_sigma[axis] > 0:
            out = adaptive_gaussian_filter1d(out, sigmas[axis], axis, presmooth_sigma, empty, curv_func, curv_kw, k_factor[axis],
                                             max_sigma[axis], mode, cval, truncate, order, sigma_node_factor)
    return out


# ---- scipy.ndimage's rank filters (median_filter, percentile_filter) and _filters.iqr_filter (43-46) --------------------------
RANK_MAX_WINDOW = 49        # the device's window cap (csrc/map_rank.hip)


def ni_select(buf, lo, hi, rank):
    """scipy's NI_Select (ni_filters.c): Hoare quickselect on buf[lo .. hi], in place.  On a window without NaNs it returns the
    rank-th smallest entry; on one with NaNs, where every comparison with a NaN is false, what it returns is a property of
    these very steps and of the order of the entries -- which is why they are restated and not replaced by a sort."""
    while True:
        if lo == hi:
            return buf[lo]
        x = buf[lo]
        i, j = lo - 1, hi + 1
        while True:
            j -= 1
            while buf[j] > x:
                j -= 1
            i += 1
            while buf[i] < x:
                i += 1
            if i < j:
                buf[i], buf[j] = buf[j], buf[i]
            else:
                break
        k = j - lo + 1
        if rank < k:
            hi = j
        else:
            lo, rank = j + 1, rank - k


def _check_rank_args(input, size, footprint, output, mode, origin):
    _check_mode(mode)
    if footprint is not None:
        raise NotImplementedError("footprint: only size= windows are built")
    if output is not None:
        raise NotImplementedError("output: the filters return a new array")
    if np.any(np.asarray(origin) != 0):
        raise NotImplementedError("origin: only origin 0 is built")
    if size is None:
        raise RuntimeError("no footprint or filter size provided")
    a = np.asarray(input, dtype=float)
    if a.ndim != 2:
        raise NotImplementedError("input: the rank filters take 2-D arrays")
    size = [int(s) for s in _normalize_sequence(size, 2)]
    if min(size) < 1:
        raise RuntimeError("incorrect filter size")
    return a, size


def percentile_rank(filter_size, percentile):
    """scipy's rank of a percentile in a window of filter_size entries (percentile_filter, _filters.py)"""
    percentile = float(percentile)
    if percentile < 0.0:
        percentile += 100.0
    if percentile < 0 or percentile > 100:
        raise RuntimeError('invalid percentile')
    if percentile == 100.0:
        return filter_size - 1
    return int(float(filter_size) * percentile / 100.0)


def window_values(a, size):
    """[rows, cols, size[0] * size[1]]: every entry's window, rows outer (the order of scipy's filter buffer), starting size // 2
    before the entry on either axis, on the 'reflect' boundary"""
    rows = reflect_index(np.arange(a.shape[0])[:, None] - size[0] // 2 + np.arange(size[0])[None, :], a.shape[0])
    cols = reflect_index(np.arange(a.shape[1])[:, None] - size[1] // 2 + np.arange(size[1])[None, :], a.shape[1])
    return a[rows[:, None, :, None], cols[None, :, None, :]].reshape(a.shape + (size[0] * size[1],))


def rank_filter(a, size, rank):
    """entry `rank` of every sorted window; a window with a NaN goes through ni_select for 0 < rank < size - 1 and is NaN at
    ranks 0 and size - 1 (numpy's min / max; scipy switches to its own minimum / maximum filter there)"""
    win = window_values(a, size)
    n = win.shape[-1]
    if not 0 <= rank < n:
        raise RuntimeError('rank not within filter footprint size')
    has_nan = np.isnan(win).any(axis=-1)
    out = np.where(has_nan, np.nan, np.sort(np.where(has_nan[..., None], 0.0, win), axis=-1)[..., rank])
    if 0 < rank < n - 1:
        for i, j in zip(*np.nonzero(has_nan)):
            out[i, j] = ni_select(win[i, j].tolist(), 0, n - 1, rank)
    return out


def median_filter(input, size=None, footprint=None, output=None, mode="reflect", cval=0.0, origin=0):
    """scipy.ndimage.median_filter for a 2-D array and size="""
    a, size = _check_rank_args(input, size, footprint, output, mode, origin)
    return rank_filter(a, size, size[0] * size[1] // 2)


def percentile_filter(input, percentile, size=None, footprint=None, output=None, mode="reflect", cval=0.0, origin=0):
    """scipy.ndimage.percentile_filter for a 2-D array and size="""
    a, size = _check_rank_args(input, size, footprint, output, mode, origin)
    return rank_filter(a, size, percentile_rank(size[0] * size[1], percentile))


def iqr_filter(a, size, **kw):
    """_filters.iqr_filter (43-46)"""
    return percentile_filter(a, 75, size=size, **kw) - percentile_filter(a, 25, size=size, **kw)


Q_NANMEDIAN = -1.0          # the entry of q that asks nan_percentiles for np.nanmedian's rule (HIPDRT_Q_NANMEDIAN)


def nan_percentiles(a, q, by_row=False):
    """np.nanpercentile(a, q) / np.nanpercentile(a, q, axis=1).T with numpy's 'linear' rule, written out as the device forms it
    (csrc/map_rank.hip): among the n sorted non-NaN values, virtual index v = (n - 1) (q / 100), neighbours a = x[floor v] and
    b = x[min(floor v + 1, n - 1)], t = v - floor v, a + (b - a) t, and b - (b - a) (1 - t) where t >= 0.5.  An entry
    Q_NANMEDIAN of q is np.nanmedian: the mean of the middle pair.  No non-NaN value: NaN.  Returns [nq] or [rows, nq]."""
    a = np.asarray(a, dtype=float)
    q = np.atleast_1d(np.asarray(q, dtype=float))
    rows = a if by_row else a.reshape(1, -1)
    out = np.full((rows.shape[0], len(q)), np.nan)
    for r, row in enumerate(rows):
        x = np.sort(row[~np.isnan(row)])
        n = len(x)
        if n == 0:
            continue
        for k, p in enumerate(q):
            if p == Q_NANMEDIAN:
                out[r, k] = (x[(n - 1) // 2] + x[n // 2]) / 2.0
                continue
            v = (n - 1) * (p / 100)
            lo = min(int(np.floor(v)), n - 1)
            lo_v, hi_v, t = x[lo], x[min(lo + 1, n - 1)], v - lo
            d = hi_v - lo_v
            out[r, k] = hi_v - d * (1 - t) if t >= 0.5 else lo_v + d * t
    return out if by_row else out[0]
