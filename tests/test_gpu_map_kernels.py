"""GPU: the kernels of csrc/map_filter.hip, csrc/map_rank.hip and csrc/map_predict.hip alone, at the launch forms and edges the
fixtures of their entry points never reach (tests/map_kernels_util.py holds cases, inputs and references; tests/test_map_kernels_util.py
pins those on the CPU).

  filter passes     hipdrt_debug_map_gaussian (plain_gaussian_device / masked_gaussian_device) and the same cases through
                    hipdrt_map_filter's driver, bit for bit against hipdrt.filters.ndfilters: tile edges, several reflection
                    periods in the LDS form, the launch at exactly 64 KiB of dynamic LDS and the uncached form one radius further,
                    on either axis, with one operand and with the masked pair.  The adaptive (sigma field) passes have a log per
                    element: max |difference| / max |reference| at the bound of tests/map_filter_bounds.json, section "kernels"
                    ([measured on an MI355X, bound = the next 1-2-5 step at least 10 x above]; only the bound is read)
  reductions        hipdrt_debug_map_reduce against math.fsum / np.longdouble at bounds derived from the launch geometry
                    (map_kernels_util.mean_bound, std_bound); min and max exact
  rank filters      hipdrt.filters.{median,percentile,iqr}_filter bit for bit against ndfilters, arrays shorter than the window
  probability rows  hipdrt_debug_map_prob on integer rows against hipdrt.mapping.predict / hipdrt.models.peaks: peak indices, zeros
                    and NaNs exact, values at atol 1e-13 (the figure tests/test_gpu_peaks.py holds this arithmetic to), the clamped
                    variances bit for bit

Every hook keeps its device arrays between borders of marker bytes and fails with HIPDRT_E_NUMERIC when one changed."""
import json
import os

import numpy as np
import pytest

import map_badness_util
import map_kernels_util as util
from conftest import ROOT

pytestmark = pytest.mark.gpu

UNWRITTEN = -7.0e77                 # what the hooks' outputs hold where no kernel wrote


@pytest.fixture(scope="module")
def ctx():
    from hipdrt import _ffi
    return _ffi.get_context(0)


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


# ---- filter passes ---------------------------------------------------------------------------------------------------------------
def run_filter_case(ctx, shape, sigma, forms):
    """one (shape, sigma) through the hook and through hipdrt_map_filter's driver, plain and / or masked, bit for bit"""
    from hipdrt import filters
    a = util.filter_input(shape)
    tabs = util.full_tables(sigma, len(shape))
    a2 = a.reshape(1, -1) if a.ndim == 1 else a
    if "plain" in forms:
        ref = util.plain_reference(a, sigma)
        assert same(ctx.debug_map_gaussian(a2, tabs, masked=False).reshape(shape), ref), ("hook", "plain", shape, sigma)
        assert same(filters.filter_array(a, iterative=False, mask_nans=False, sigma=sigma), ref), ("driver", "plain", shape, sigma)
    if "masked" in forms:
        mask = util.filter_mask(shape, sigma)
        ref = util.masked_reference(a, mask, sigma)
        assert not np.isnan(ref).any()
        got = ctx.debug_map_gaussian(np.where(mask == 0, np.nan, a).reshape(a2.shape), tabs, masked=True).reshape(shape)
        assert same(got, ref), ("hook", "masked", shape, sigma)
        assert same(filters.masked_filter(a, mask, sigma=sigma), ref), ("driver", "masked", shape, sigma)


@pytest.mark.parametrize("shape", util.TILE_SHAPES, ids=str)
def test_filter_passes_at_tile_edges(ctx, shape):
    for sigma in util.TILE_SIGMAS:
        run_filter_case(ctx, shape, sigma, ("plain", "masked"))


def test_filter_lds_form_with_several_reflection_periods(ctx):
    run_filter_case(ctx, *util.MULTI_PERIOD, ("plain", "masked"))


@pytest.mark.parametrize("case", util.EDGE_CASES, ids=util.case_id)
def test_filter_at_the_64_kib_edge_and_uncached(ctx, case):
    """radius at which the window takes exactly 65536 bytes of LDS, and the next one, read through the caches; every array is
    shorter than its radius, so the reflection wraps more than once"""
    shape, sigma, masked = case[:3]
    run_filter_case(ctx, shape, sigma, ("masked",) if masked else ("plain",))


def test_fully_masked_row_is_nan_and_nothing_else(ctx):
    from hipdrt import filters
    x, mask, sigma = util.masked_row_case()
    ref = util.masked_reference(x, mask, sigma)
    assert np.isnan(ref[4]).all() and np.isnan(ref).sum() == ref.shape[1]
    got = ctx.debug_map_gaussian(np.where(mask == 0, np.nan, x), util.full_tables(sigma), masked=True)
    assert same(got, ref)
    assert same(filters.masked_filter(x, mask, sigma=sigma), ref)


@pytest.mark.parametrize("name", util.ADAPTIVE_CASES)
def test_adaptive_passes_with_wide_nodes(ctx, name):
    from hipdrt import filters
    from hipdrt.filters import ndfilters
    a, sigmas, max_sigma = util.adaptive_case(name)
    ref = ndfilters.adaptive_gaussian_filter(a, sigmas=[s.copy() for s in sigmas], max_sigma=max_sigma)
    got = filters.adaptive_gaussian_filter(a, sigmas=sigmas, max_sigma=max_sigma)
    err = util.deviation(got, ref)
    with open(os.path.join(ROOT, "tests", "map_filter_bounds.json")) as f:
        entry = json.load(f).get("kernels", {}).get(name)
    print(f"map_filter kernels {name}: measured {err:.2e} bound {entry[1] if entry else None}")
    assert entry is not None, f"{name}: no bound in tests/map_filter_bounds.json yet (measured {err:.2e})"
    assert err <= entry[1], (name, err, entry)


def test_gaussian_hook_refusals(ctx):
    from hipdrt import _ffi
    a = np.zeros((3, 4))
    with pytest.raises(_ffi.HipDrtError, match="invalid argument"):
        ctx.debug_map_gaussian(np.zeros((0, 4)), [None, None])
    tabs = (_ffi.FilterTable * 2)()
    tabs[0].radius, tabs[1].radius = 2, -1                                      # a radius without its weights
    out = np.empty_like(a)
    assert ctx._lib.hipdrt_debug_map_gaussian(ctx._h, _ffi._p(a), 3, 4, tabs, 0, _ffi._p(out)) == -1
    tabs[0].radius = -1
    assert ctx._lib.hipdrt_debug_map_gaussian(ctx._h, _ffi._p(a), 3, 4, tabs, 2, _ffi._p(out)) == -1      # masked: 0 or 1


# ---- reductions ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", util.REDUCE_N)
def test_reductions_within_the_derived_bounds(ctx, n):
    x = util.reduce_data(n)
    mean, zero = ctx.debug_map_reduce(x, 0)
    err, bound = abs(mean - util.mean_exact(x)), util.mean_bound(x)
    print(f"map_reduce n {n}: mean |error| {err:.3e} bound {bound:.3e}")
    assert zero == 0.0 and err <= bound, (n, err, bound)
    std, mean_used = ctx.debug_map_reduce(x, 1)
    assert mean_used == mean                                                    # the same launch twice: the same bits
    exact = util.std_exact(x, mean_used)
    serr, sbound = abs(std - exact), util.std_bound(x, exact)
    print(f"map_reduce n {n}: std |error| {serr:.3e} bound {sbound:.3e}")
    assert serr <= sbound, (n, serr, sbound)
    assert ctx.debug_map_reduce(x, 2) == (x.min(), x.max())
    # the extremes in the last element a thread reaches, and in the first
    y = x.copy()
    y[-1], y[0] = 2 * abs(x).max() + 1, -2 * abs(x).max() - 1
    assert ctx.debug_map_reduce(y, 2) == (y[0], y[-1])


def test_reductions_of_constant_arrays(ctx):
    const = np.full(256, 0.1)
    assert ctx.debug_map_reduce(const, 0)[0] == 0.1
    assert ctx.debug_map_reduce(const, 1) == (0.0, 0.1)
    for n in (1, 256, 262145):
        assert ctx.debug_map_reduce(np.full(n, -3.5), 2) == (-3.5, -3.5)


def test_reduce_hook_refusals(ctx):
    from hipdrt import _ffi
    with pytest.raises(_ffi.HipDrtError, match="invalid argument"):
        ctx.debug_map_reduce(np.zeros(0), 0)
    with pytest.raises(_ffi.HipDrtError, match="mode"):
        ctx.debug_map_reduce(np.zeros(4), 3)


# ---- rank filters ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", util.RANK_SHAPES, ids=str)
def test_rank_filters_on_arrays_shorter_than_the_window(shape):
    from hipdrt import filters
    a = util.rank_input(shape)
    for size in util.RANK_WINDOWS:
        for kind in util.RANK_KINDS:
            if kind == "median":
                got = filters.median_filter(a, size=size)
            elif kind == "iqr":
                got = filters.iqr_filter(a, size=size)
            else:
                got = filters.percentile_filter(a, int(kind[1:]), size=size)
            assert map_badness_util.rank_rule_equal(a, kind, size, got, util.rank_reference(a, kind, size)), (shape, size, kind)


# ---- probability rows ------------------------------------------------------------------------------------------------------------
def check_prob(ctx, rows, ext, search, height, prominence, sign_now, clamp_first=False):
    fxx, f, vxx, vf = rows
    ref = util.prob_reference(f, fxx, vf, vxx, ext, search, height, prominence, sign_now)
    got = ctx.debug_map_prob(f, fxx, vf, vxx, ext=ext, clamp_first=clamp_first, search=search, height=height, prominence=prominence,
                             sign_now=sign_now)
    tag = f"n {f.shape[1]} search {search} sign_now {sign_now} clamp_first {clamp_first}"
    for k in got:
        assert not (got[k] == UNWRITTEN).any(), f"{k} {tag}: entries no kernel wrote"
    for k in ("pk", "curv"):
        assert np.array_equal(np.isnan(got[k]), np.isnan(ref[k])), f"{k} {tag}: NaN entries differ"
        assert np.array_equal(got[k] == 0, ref[k] == 0), f"{k} {tag}: peak indices / zeros differ"
        np.testing.assert_allclose(got[k], ref[k], rtol=0, atol=1e-13, err_msg=f"{k} {tag}")
    assert same(got["f_var"], ref["f_var"]) and same(got["fxx_var"], ref["fxx_var"]), f"clamped variances {tag}"
    return got


@pytest.mark.parametrize("n", util.PROB_N)
def test_probability_rows_on_integer_rows(ctx, n):
    rng = np.random.default_rng(2000 + n)
    big = n > 257                    # (the statement's walks are Python loops: one row and one search kind)
    B = 1 if big else 3
    rows = util.integer_rows(rng, B, n)
    ext = util.ext_rows(rng, B, n)
    for search in ((0,) if big else (-1, 0, 1)):
        check_prob(ctx, rows, ext, search, 1e-3, 5e-3, True)                    # the clamp inside map_prob_kernel
        check_prob(ctx, rows, ext, search, 1.0, 2.0, False, clamp_first=True)   # clamp_kernel first
        if not big:
            check_prob(ctx, rows, None, search, 1e-3, 5e-3, False)
    if not big:
        # the clamp kernel alone
        got = ctx.debug_map_prob(None, None, rows[3], rows[2], ext=ext, clamp_first=True, want=("f_var", "fxx_var"))
        assert same(got["f_var"], util.predict.clamp_rows(rows[3], ext)) and same(got["fxx_var"], util.predict.clamp_rows(rows[2], ext))


def test_probability_rows_adversarial(ctx):
    from test_gpu_peaks import adversarial_rows
    fxx = adversarial_rows()
    B, n = fxx.shape
    rng = np.random.default_rng(5)
    _, f, vxx, vf = util.integer_rows(rng, B, n)
    ext = util.ext_rows(rng, B, n)
    ext[1] = (-1, -1)
    ext[2] = (200, 40)                                                          # crossed: the right side reads what the left raised
    ext[3] = (n - 1, 0)
    vf[4, 77] = np.nan                                                          # a NaN variance: the clamp leaves the row alone
    vxx[5, 0] = np.nan
    f[6], fxx[6] = np.nan, np.nan                                               # a NaN row: no peaks, NaN through sign(f)
    for search in (1, -1, 0):
        for sign_now in (True, False):
            got = check_prob(ctx, (fxx, f, vxx, vf), ext, search, 0.0, 0.0, sign_now)
            assert np.isnan(got["pk"][6]).all() == sign_now
            check_prob(ctx, (fxx, f, vxx, vf), ext, search, 1.0, 1.0, sign_now, clamp_first=True)
    # (search 0, unsigned: the last call of the loop) the plateaus across lane 63|64 and thread 255|256, the plateau ending at n - 2
    one = check_prob(ctx, (fxx, f, vxx, vf), ext, 1, 0.0, 0.0, False)
    assert one["pk"][0].nonzero()[0].tolist() == [64, 100, 256]
    assert one["pk"][1].nonzero()[0].tolist() == [42, n - 4] and one["pk"][2].nonzero()[0].tolist() == [42]
    assert np.isnan(one["pk"][4, 77]) and not np.isnan(one["pk"][6]).any()
    assert same(one["f_var"][4], vf[4]) and same(one["fxx_var"][5], vxx[5])


def test_probability_row_position_does_not_change_the_bits(ctx):
    rng = np.random.default_rng(11)
    n = 257
    batch = [rng.normal(size=(37, n)), rng.normal(size=(37, n)), rng.random((37, n)) + 0.1, rng.random((37, n)) + 0.1]
    ext = util.ext_rows(rng, 37, n)
    ext[0] = ext[1]
    for search, sign_now, clamp_first in ((1, True, False), (0, False, False), (-1, True, True)):
        kw = dict(search=search, sign_now=sign_now, clamp_first=clamp_first)
        many = ctx.debug_map_prob(batch[1], batch[0], batch[3], batch[2], ext=ext, **kw)
        assert (many["pk"] != 0).any(axis=1).all()
        for b in (0, 36):
            one = ctx.debug_map_prob(*[batch[k][b:b + 1] for k in (1, 0, 3, 2)], ext=ext[b:b + 1], **kw)
            for k, v in one.items():
                assert np.array_equal(v[0], many[k][b]), (k, b, kw)


def test_prob_hook_refusals(ctx):
    from hipdrt import _ffi
    n = util.PROB_N_REFUSED
    ones = np.ones((1, n))
    with pytest.raises(NotImplementedError, match="neval <= 3145"):
        ctx.debug_map_prob(ones, ones, ones, ones)
    fxx, f, vxx, vf = util.integer_rows(np.random.default_rng(1), 2, 40)
    for bad in ([[0, 40], [1, 2]], [[1, 2], [-1, 3]], [[1, 2], [3, -2]], [[40, 0], [1, 2]]):
        with pytest.raises(_ffi.HipDrtError, match="ext"):
            ctx.debug_map_prob(f, fxx, vf, vxx, ext=bad)
    with pytest.raises(_ffi.HipDrtError, match="nothing to launch"):
        ctx.debug_map_prob(f, fxx, vf, vxx, want=("f_var",))
    with pytest.raises(_ffi.HipDrtError, match="f and fxx"):
        ctx.debug_map_prob(None, None, vf, vxx, want=("curv",))
    with pytest.raises(_ffi.HipDrtError, match="search"):
        ctx.debug_map_prob(f, fxx, vf, vxx, search=2)
