"""Shared by tests/test_map_kernels_util.py (CPU) and tests/test_gpu_map_kernels.py: the cases, inputs, references and derived
bounds of the isolation tests of csrc/map_filter.hip, csrc/map_rank.hip and csrc/map_predict.hip.

Filters and rank filters are read against hipdrt.filters.ndfilters (numpy; the CPU test pins it to scipy.ndimage bit for bit at
every shape used here).  The reductions are read against math.fsum / np.longdouble with bounds derived from the launch geometry
below; probability rows against hipdrt.mapping.predict and hipdrt.models.peaks.  Nothing here touches a GPU."""
import math

import numpy as np

from hipdrt.filters import ndfilters
from hipdrt.mapping import predict
from hipdrt.models import peaks

U = 2.0 ** -53

# ---- filter passes (csrc/map_filter.hip: filter_pass_kernel through MapFilter::pass) ---------------------------------------------
TILE_R0, TILE_R1, TILE_C, LDS_BUDGET = 32, 4, 64, 65536          # the launcher's tiles and its LDS budget

TILE_SHAPES = ((1, 1), (1, 64), (1, 65), (32, 1), (33, 1), (31, 63), (32, 64), (33, 65), (65, 129))
TILE_SIGMAS = ((1.5, 0.5), (1, 0), (0, 1))
MULTI_PERIOD = ((2, 3), (3, 3))                                  # (shape, sigma): the LDS form, several reflection periods

# (shape, sigma, masked, axis, radius, form): the launch at exactly 64 KiB of dynamic LDS and the first radius past it.  Every array
# is shorter than its radius.
EDGE_CASES = (
    ((5, 70), (4, 0), True, 0, 16, "lds"), ((5, 70), (4.25, 0), True, 0, 17, "uncached"),
    ((20, 70), (12, 0), False, 0, 48, "lds"), ((20, 70), (12.25, 0), False, 0, 49, "uncached"),
    ((3, 300), (0, 120), True, 1, 480, "lds"), ((3, 300), (0, 120.25), True, 1, 481, "uncached"),
    ((300,), 120, True, 1, 480, "lds"), ((300,), 120.25, True, 1, 481, "uncached"),
    ((3, 300), (0, 248), False, 1, 992, "lds"), ((3, 300), (0, 248.25), False, 1, 993, "uncached"),
    ((300,), 248, False, 1, 992, "lds"), ((300,), 248.25, False, 1, 993, "uncached"),
)


def case_id(case):
    return "-".join(str(c).replace(" ", "") for c in case)


def sigma_seq(sigma, ndim):
    return [float(sigma)] * ndim if np.ndim(sigma) == 0 else [float(s) for s in sigma]


def lds_bytes(axis, radius, pair):
    """dynamic LDS MapFilter::pass asks for: the tile with its halo along the axis, once or (masked pair) twice"""
    wr = (TILE_R0 + 2 * radius) if axis == 0 else TILE_R1
    wc = TILE_C + (2 * radius if axis == 1 else 0)
    return wr * wc * 8 * (2 if pair else 1)


def full_tables(sigma, ndim=2):
    """one full symmetric Gaussian table per axis of a 2-D launch (a 1-D array is one row: axis 0 skipped), None where scipy
    skips the axis"""
    tabs = [None if s <= 1e-15 else ndfilters.gaussian_kernel1d(s, 0, ndfilters.kernel_radius(s)) for s in sigma_seq(sigma, ndim)]
    return [None] * (2 - ndim) + tabs


def filter_input(shape, seed=0):
    rng = np.random.default_rng([seed, 17] + list(shape))
    return rng.normal(size=shape) * 10.0 ** rng.integers(-1, 2, shape)


def filter_mask(shape, sigma, seed=0):
    """about 10 % zeros, then every entry whose whole window is masked is given back, until no output of the masked filter is NaN"""
    rng = np.random.default_rng([seed, 29] + list(shape))
    mask = (rng.random(shape) >= 0.1).astype(float)
    for _ in range(8):
        empty = ndfilters.gaussian_filter(mask, sigma) == 0
        if not empty.any():
            break
        mask[empty] = 1.0
    return mask


def plain_reference(a, sigma):
    return ndfilters.gaussian_filter(a, sigma)


def masked_reference(x, mask, sigma):
    return ndfilters.masked_filter(x, mask, sigma=sigma)


def masked_row_case():
    """a fully masked row with sigma (0, 1): that row, and only that row, is NaN"""
    x, mask = filter_input((7, 70), seed=3), filter_mask((7, 70), (0, 1), seed=3)
    mask[4] = 0.0
    return x, mask, (0, 1)


def adaptive_case(name):
    """(a, sigma fields, max_sigma) of the adaptive cases: 'adaptive_40x70' is the sigma field 0.1 ... 6 along axis 0 (node radii up to
    24); 'adaptive_wide_40x70' reaches 13 (radius 52: with one operand the window passes the LDS budget from radius 49 on)"""
    top = {"adaptive_40x70": 6.0, "adaptive_wide_40x70": 13.0}[name]
    a = filter_input((40, 70), seed=5)
    rng = np.random.default_rng(41)
    s0 = np.geomspace(0.1, top, 40)[:, None] * np.ones((1, 70))
    s0[1:-1] *= rng.uniform(0.9, 1.0, (38, 70))                  # the extremes stay 0.1 and top
    s1 = rng.uniform(0.3, 1.0, (40, 70))
    return a, [s0, s1], (top, 1)


ADAPTIVE_CASES = ("adaptive_40x70", "adaptive_wide_40x70")


def deviation(actual, ref):
    assert np.array_equal(np.isnan(actual), np.isnan(ref))
    return float(np.nanmax(np.abs(actual - ref)) / np.nanmax(np.abs(ref)))


# ---- reductions (csrc/map_filter.hip: reduce_partial, reduce_final) ------------------------------------------------------------
REDUCE_N = (1, 2, 255, 256, 257, 65537, 262144, 262145, 600001)
REDUCE_G = 1024                                                  # MapFilter::G, the cap on the grid of reduce_partial


def reduce_geometry(n):
    """(blocks, T, F, L): workgroups of reduce_partial, elements a thread adds serially, partials a thread of reduce_final adds
    serially, and the longest chain of additions behind the result: T serial + 8 tree levels, then F serial + 8 tree levels"""
    blocks = min(REDUCE_G, -(-n // 256))
    T = -(-n // (256 * blocks))
    F = -(-blocks // 256)
    return blocks, T, F, T + 8 + F + 8


def gamma(k):
    return k * U / (1 - k * U)


def reduce_data(n, seed=0):
    """mixed signs over six decades"""
    rng = np.random.default_rng([seed, n])
    return rng.normal(size=n) * 10.0 ** rng.uniform(-3, 3, n)


def mean_exact(x):
    return math.fsum(x) / len(x)


def mean_bound(x):
    """every element passes through at most L additions and the division: |dev - exact| <= gamma(L + 1) sum|x| / n (Higham,
    Accuracy and Stability of Numerical Algorithms, 4.2: any order of summation)"""
    L = reduce_geometry(len(x))[3]
    return gamma(L + 1) * math.fsum(np.abs(x)) / len(x)


def std_exact(x, mean):
    """sqrt(sum (x - mean)^2 / n) about the given mean (the device's own), in extended precision"""
    d = np.asarray(x, dtype=np.longdouble) - np.longdouble(mean)
    return float(np.sqrt(np.sum(d * d) / np.longdouble(len(x))))


def std_bound(x, exact):
    """non-negative terms, three roundings a term (x - mu, its square, the addition chain of length L counted apart), then the
    division and the square root: |dev - exact| <= (L + 6) u exact"""
    return (reduce_geometry(len(x))[3] + 6) * U * exact


def _tree(s):
    """block_tree: s[t] += s[t + h] for h = 128 ... 1 over the 256 threads (any number of leading axes)"""
    h = 128
    while h >= 1:
        s = s[..., :h] + s[..., h:2 * h]
        h //= 2
    return s[..., 0]


def _strided_serial(v, groups):
    """v[k * groups * 256 + g * 256 + t] added in ascending k into the accumulator of thread t of group g, from 0.0"""
    pad = (-len(v)) % (groups * 256)
    w = np.concatenate([v, np.zeros(pad)]).reshape(-1, groups, 256)
    acc = np.zeros((groups, 256))
    for k in range(w.shape[0]):
        acc = acc + w[k]
    return acc


def emulate_sum(terms):
    """the device's fixed order on the terms: per-thread grid-strided serial sum, binary tree over 256, then the same again over the
    partials in one workgroup"""
    blocks = reduce_geometry(len(terms))[0]
    partial = _tree(_strided_serial(np.asarray(terms, dtype=float), blocks))
    return float(_tree(_strided_serial(partial, 1))[0])


def emulate_mean(x):
    return emulate_sum(x) / float(len(x))


def emulate_std(x, mean):
    d = np.asarray(x, dtype=float) - mean
    return float(np.sqrt(emulate_sum(d * d) / float(len(x))))


# ---- rank filters (csrc/map_rank.hip: rank_kernel through hipdrt.filters) ---------------------------------------------------------
# (2 rows or columns: the only length at which a window of 7 reflects past one period and the entry it lands on is not
# the one a clamp would give -- with 1 every index is entry 0)
RANK_SHAPES = ((1, 1), (3, 5), (1, 70), (70, 1), (16, 64), (17, 65), (2, 2), (2, 70), (70, 2))
RANK_WINDOWS = ((7, 7), (5, 3), (3, 3), (1, 7), (7, 1))
RANK_KINDS = ("median", "p25", "p75", "iqr")


def rank_input(shape):
    """exact doubles with repeats and about 3 % NaNs (none in a single entry)"""
    rng = np.random.default_rng([53] + list(shape))
    a = rng.integers(-40, 41, shape) / 8.0
    if a.size > 1:
        a.flat[rng.choice(a.size, max(1, round(0.03 * a.size)), replace=False)] = np.nan
    return a


def rank_reference(a, kind, size):
    if kind == "median":
        return ndfilters.median_filter(a, size=size)
    if kind == "iqr":
        return ndfilters.iqr_filter(a, size=size)
    return ndfilters.percentile_filter(a, int(kind[1:]), size=size)


# ---- probability rows (csrc/map_predict.hip: clamp_kernel, map_prob_kernel) ------------------------------------------------------
PROB_N = (1, 2, 3, 255, 256, 257, 1260, 1261, 3145)             # 1261: the first n past 64 KiB of LDS; 3145: the last one that fits
PROB_N_REFUSED = 3146


def integer_rows(rng, B, n):
    """(fxx, f, var_fxx, var_f) as tests/test_gpu_peaks.py draws them: small integers (plateaus, ties, zeros of f), variances 1, 4, 16"""
    return (rng.integers(-3, 4, (B, n)).astype(float), rng.integers(-2, 3, (B, n)).astype(float),
            4.0 ** rng.integers(0, 3, (B, n)), 4.0 ** rng.integers(0, 3, (B, n)))


def ext_rows(rng, B, n):
    """clamp indices of B rows of n points: a quarter in from either end, the first row without a clamp when there are several"""
    ext = np.stack([np.full(B, n // 4), np.full(B, n - 1 - n // 4)], axis=1).astype(np.int32)
    ext[:, 0] += rng.integers(0, max(1, n // 8), B).astype(np.int32)
    if B > 1:
        ext[0] = -1
    return ext


def prob_reference(f, fxx, vf, vxx, ext, search, height, prominence, sign_now):
    """dict(pk, curv, f_var, fxx_var): the statement of stage 3 on the given rows"""
    if ext is not None:
        vf, vxx = predict.clamp_rows(vf, ext), predict.clamp_rows(vxx, ext)
    with np.errstate(invalid="ignore", divide="ignore"):
        pk = predict.peak_rows(f, fxx, vf, vxx, search, height, prominence)
        if sign_now:
            pk = pk * np.sign(f)
        curv = peaks.curv_prob_row(f, fxx, vf, vxx)
    return dict(pk=pk, curv=curv, f_var=np.array(vf, dtype=float), fxx_var=np.array(vxx, dtype=float))
