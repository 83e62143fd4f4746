"""Device rank filters, percentiles and the map-badness chain (csrc/map_rank.hip: hipdrt_rank_filter, hipdrt_percentiles,
hipdrt_map_badness) behind hipdrt.filters.{median,percentile,iqr}_filter, hipdrt.mapping.nddata and
DRTMD.score_group_*_badness, against the reference's fixture tests/golden/refrun_map_badness.npz
(tools/make_map_badness_golden.py).

Rank filters, percentiles and flags are exact.  A row's rss is a sum of `cols` non-negative terms, each formed by the same
correctly rounded operations (-, /, *, +; no exp: that enters the flags only, whose margins the fixture generator guards) on the
device and in numpy, added in a different order and divided by cols: per row

    |device - reference| <= (cols + c) 2^-52 reference

with less than cols 2^-53 for either summation order, and c the roundings of one term and of the final division, counted once
for either side (tools/update_map_badness_bounds.py lists them).  tests/map_badness_bounds.json holds that bound next to the
deviation measured on an MI355X; only the bound is read here."""
import json
import os

import numpy as np
import pytest

import map_badness_util as util
from conftest import ROOT

pytestmark = pytest.mark.gpu

G = util.load()
RANK_KEYS = sorted(k for k in G.files if k.startswith("rank.") and not k.endswith(".in"))


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def check(label, actual, ref):
    """per row: |actual - ref| <= bound * ref (a zero stays a zero); prints the measured figure before it asserts"""
    with open(os.path.join(ROOT, "tests", "map_badness_bounds.json")) as f:
        bound = json.load(f)[label]["bound"]
    actual, ref = np.asarray(actual), np.asarray(ref)
    assert actual.shape == ref.shape and np.all(np.isfinite(actual)) and np.all(ref >= 0)
    rel = np.abs(actual - ref) / np.where(ref > 0, ref, 1.0)
    assert np.all(actual[ref == 0] == 0)
    print(f"map_badness {label}: measured {rel.max():.3e} bound {bound:.3e}")
    assert rel.max() <= bound, (label, rel.max(), bound)


def device_rank(key):
    from hipdrt import filters
    a, kind, size = util.rank_case(G, key)
    if kind == "median":
        return filters.median_filter(a, size=size)
    if kind == "iqr":
        return filters.iqr_filter(a, size=size)
    return filters.percentile_filter(a, int(kind[1:]), size=size)


@pytest.mark.parametrize("key", RANK_KEYS)
def test_rank_filter_bit_for_bit(key):
    assert util.rank_equal(G, key, device_rank(key)), key


def test_rank_filter_window_cap_and_min_max_rule():
    from hipdrt import _ffi
    ctx = _ffi.get_context(0)
    with pytest.raises(NotImplementedError, match="49"):
        ctx.rank_filter(G["rank.a23.in"], (8, 7), 3)
    a = np.arange(9.0).reshape(3, 3)
    assert ctx.rank_filter(a, (3, 3), 0)[1, 1] == 0 and ctx.rank_filter(a, (3, 3), 8)[1, 1] == 8
    a[1, 1] = np.nan                                   # ranks 0 and size - 1 of a NaN window: NaN
    assert np.isnan(ctx.rank_filter(a, (3, 3), 0)).all() and np.isnan(ctx.rank_filter(a, (3, 3), 8)).all()


def test_rank_filter_of_a_slab_equals_the_full_call():
    """a row filtered inside the array of its neighbours alone (other tiles, other reflections further out) is the same row"""
    from hipdrt import filters
    a = G["rank.a70.in"]
    for size, halo in (((7, 7), 3), ((5, 3), 2), ((3, 1), 1)):
        full = filters.median_filter(a, size=size)
        iqr = filters.iqr_filter(a, size=size)
        for row in (21, 34, 46, 63):
            slab = a[row - halo:row + halo + 1]
            assert same(filters.median_filter(slab, size=size)[halo], full[row]), (size, row)
            assert same(filters.iqr_filter(slab, size=size)[halo], iqr[row]), (size, row)


def test_percentiles_bit_for_bit():
    from hipdrt import _ffi
    ctx = _ffi.get_context(0)
    q = np.array(util.WHOLE_Q)
    for n in util.SEGMENT_LENGTHS:
        for kind in ("plain", "nan", "equal", "zeros"):
            seg = util.segment(n, kind)
            got = np.concatenate([ctx.percentiles(seg, q[:4]), ctx.percentiles(seg, q[4:])])
            assert same(got, G[f"pct.{n}.{kind}.nanpercentile"]), (n, kind)
            if kind != "nan":
                assert same(got, G[f"pct.{n}.{kind}.percentile"]), (n, kind)
            assert same(ctx.percentiles(seg, [_ffi.Q_NANMEDIAN])[0], G[f"pct.{n}.{kind}.nanmedian"]), (n, kind)
    for name in util.ROW_CASES:
        a = util.row_case(name)
        assert same(ctx.percentiles(a, util.ROW_Q, by_row=True), G[f"pct.{name}.nanpercentile"]), name
        assert same(ctx.percentiles(a, [_ffi.Q_NANMEDIAN], by_row=True)[:, 0], G[f"pct.{name}.nanmedian"]), name
        # the whole array as one segment, whatever its shape
        assert same(ctx.percentiles(a, util.ROW_Q), ctx.percentiles(np.ascontiguousarray(a.T), util.ROW_Q))
        assert same(ctx.percentiles(a, util.ROW_Q), np.nanpercentile(a, util.ROW_Q))
    assert np.isnan(ctx.percentiles(util.segment(5, "allnan"), [50.0, _ffi.Q_NANMEDIAN])).all()


@pytest.mark.parametrize("name", ["a23", "a70"])
def test_flags_exact_and_rss_within_the_derived_bound(name):
    from hipdrt import filters
    from hipdrt.mapping import nddata
    y = G[f"chain.{name}.in"]
    assert np.array_equal(nddata.flag_outliers(y, filter_size=(5, 1), thresh=0.7), G[f"chain.{name}.flags"])
    bad, rss = nddata.flag_bad_obs(y, filters.median_filter(y, size=(3, 3)), std_size=(5, 3), return_rss=True)
    check(f"chain.{name}.rss", rss, G[f"chain.{name}.rss"])
    assert np.array_equal(bad, G[f"chain.{name}.bad"])
    info = nddata.score_rows(y, (3, 3), (5, 3), return_info=True)
    check(f"chain.{name}.rss", info["rss"], G[f"chain.{name}.rss"])
    assert same(info["filt"], filters.median_filter(y, size=(3, 3)))
    # flags and the 5 % rule inside the chain: the rows the rule leaves alone keep their values, the others lose their flagged points
    ref = nddata.score_rows_statement(y, (3, 1), (5, 3), ignore_outliers=True, return_info=True)
    got = nddata.score_rows(y, (3, 1), (5, 3), ignore_outliers=True, return_info=True)
    assert np.array_equal(got["flags"], G[f"chain.{name}.flags"]) and same(got["filt"], ref["filt"])
    check(f"chain.{name}.rss", got["rss"], ref["rss"])


def test_chain_repeats_itself_bit_for_bit():
    from hipdrt.mapping import nddata
    y = G["chain.a70.in"]
    first = nddata.score_rows(y, (3, 1), (5, 3), scale_src=np.abs(y) + 1.0, ignore_outliers=True, return_info=True)
    again = nddata.score_rows(y, (3, 1), (5, 3), scale_src=np.abs(y) + 1.0, ignore_outliers=True, return_info=True)
    for k in ("rss", "flags", "filt"):
        assert same(first[k], again[k]), k
    ref = nddata.score_rows_statement(y, (3, 1), (5, 3), scale_src=np.abs(y) + 1.0, ignore_outliers=True, return_info=True)
    assert np.array_equal(first["flags"], ref["flags"]) and same(first["filt"], ref["filt"])


def test_x_std_with_nans_is_the_reference_error():
    from hipdrt.mapping import nddata
    a = np.full((6, 9), np.nan)
    with pytest.raises(ValueError, match="x_std contains nans"):
        nddata.flag_bad_obs(a, a, std_size=(5, 3))


def test_store_scores_within_the_derived_bound():
    import test_host_map_badness as host
    md = host.fit_store()
    md.score_group_fit_badness("g", ["T"])
    check("fit.badness", md.obs_fit_badness, G["fit.badness"])
    for kind in ("hybrid", "mixed"):
        md, order = host.data_store(kind)
        md.score_group_data_badness("g", ["T"])
        check(f"data.{kind}.badness", md.obs_data_badness, G[f"data.{kind}.badness"][order])
