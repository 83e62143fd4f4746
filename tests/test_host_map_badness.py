"""CPU: the numpy statement of the map-badness chains (hipdrt.filters.ndfilters rank filters and percentiles,
hipdrt.mapping.nddata, DRTMD.score_group_*_badness with statement=True) against the reference's fixture
tests/golden/refrun_map_badness.npz (tools/make_map_badness_golden.py), the NotImplementedErrors, the extension beyond
upstream's domain and the store's bookkeeping."""
import numpy as np
import pytest

import map_badness_util as util
from hipdrt.filters import ndfilters
from hipdrt.mapping import nddata
from hipdrt.mapping.store import DRTMD

G = util.load()
RANK_KEYS = sorted(k for k in G.files if k.startswith("rank.") and not k.endswith(".in"))


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def rank_statement(key):
    a, kind, size = util.rank_case(G, key)
    if kind == "median":
        return ndfilters.median_filter(a, size=size)
    if kind == "iqr":
        return ndfilters.iqr_filter(a, size=size)
    return ndfilters.percentile_filter(a, int(kind[1:]), size=size)


@pytest.mark.parametrize("key", RANK_KEYS)
def test_rank_filters_bit_for_bit(key):
    assert util.rank_equal(G, key, rank_statement(key)), key


def test_fixture_has_nan_windows_and_every_size():
    assert np.isnan(G["rank.a70.in"]).all(axis=1).sum() == 3 and np.isnan(G["rank.a23.in"]).any()
    for size in util.SIZES:
        for name in ("a3x5", "a1x40", "a23", "a70"):
            assert any(k.startswith(f"rank.{name}.") and k.endswith(f".{size[0]}x{size[1]}") for k in RANK_KEYS), (name, size)
    # a NaN inside a window does not simply sort last: some outputs next to the NaN rows are numbers, some are NaN
    med = G["rank.a70.median.3x3"]
    assert np.isnan(med[19:22]).any() and not np.isnan(med[19:22]).all()


def test_rank_filter_of_nan_window_at_extreme_ranks_is_nan():
    a = np.arange(9.0).reshape(3, 3)
    a[1, 1] = np.nan                                  # inside every 3 x 3 window of a 3 x 3 array
    lo, hi = ndfilters.percentile_filter(a, 0, size=(3, 3)), ndfilters.percentile_filter(a, 100, size=(3, 3))
    assert np.isnan(lo).all() and np.isnan(hi).all()
    b = np.arange(12.0).reshape(3, 4)
    assert ndfilters.percentile_filter(b, 0, size=(3, 3))[1, 1] == 0 and ndfilters.percentile_filter(b, 100, size=(3, 3))[1, 1] == 10


@pytest.mark.parametrize("name", ["a23", "a70"])
def test_flags_and_rss_bit_for_bit(name):
    y = G[f"chain.{name}.in"]
    flags = nddata.flag_outliers_statement(y, filter_size=(5, 1), thresh=0.7)
    assert np.array_equal(flags, G[f"chain.{name}.flags"])
    bad, rss = nddata.flag_bad_obs_statement(y, ndfilters.median_filter(y, size=(3, 3)), std_size=(5, 3), return_rss=True)
    assert same(rss, G[f"chain.{name}.rss"]) and np.array_equal(bad, G[f"chain.{name}.bad"])
    info = nddata.score_rows_statement(y, (3, 3), (5, 3), return_info=True)
    assert same(info["rss"], G[f"chain.{name}.rss"])


def test_percentile_formula_against_numpy():
    for n in util.SEGMENT_LENGTHS:
        for kind in ("plain", "nan", "equal", "zeros"):
            seg = util.segment(n, kind)
            got = ndfilters.nan_percentiles(seg, util.WHOLE_Q)
            assert same(got, G[f"pct.{n}.{kind}.nanpercentile"]), (n, kind)
            if kind != "nan":
                assert same(got, G[f"pct.{n}.{kind}.percentile"]), (n, kind)
            assert same(ndfilters.nan_percentiles(seg, [ndfilters.Q_NANMEDIAN])[0], G[f"pct.{n}.{kind}.nanmedian"]), (n, kind)
    for name in util.ROW_CASES:
        a = util.row_case(name)
        assert same(ndfilters.nan_percentiles(a, util.ROW_Q, by_row=True), G[f"pct.{name}.nanpercentile"]), name
        assert same(ndfilters.nan_percentiles(a, [ndfilters.Q_NANMEDIAN], by_row=True)[:, 0], G[f"pct.{name}.nanmedian"]), name
    assert np.isnan(ndfilters.nan_percentiles(util.segment(5, "allnan"), [50.0, ndfilters.Q_NANMEDIAN])).all()


def fit_store():
    md = DRTMD(np.logspace(-7, 2, 91), drt=object(), psi_dim_names=["T"])
    for k, psi in enumerate(G["fit.psi"][:, 0]):
        md.add_observation([psi], None, None, group_id="g" if psi < 14 else "other")
    md.obs_x = G["fit.obs_x"].copy()
    md.obs_ignore_flag, md.obs_fit_status = G["fit.ignore"].copy(), G["fit.status"].copy()
    return md


def data_store(kind, chrono=True, eis=True):
    md = DRTMD(np.logspace(-7, 2, 91), drt=object(), psi_dim_names=["T"])
    t, f = G[f"data.{kind}.t"], G[f"data.{kind}.f"]
    order = [7, 3, 11, 0, 5, 9, 1, 8, 2, 10, 4, 6]              # entered out of psi order
    for k in order:
        has = bool(G[f"data.{kind}.has_chrono"][k]) and chrono
        md.add_observation([float(k)], (t, G[f"data.{kind}.i"][k], G[f"data.{kind}.v"][k]) if has else None,
                           (f, G[f"data.{kind}.z"][k]) if eis else None, group_id="g")
    return md, np.array(order)


def test_store_fit_score_bit_for_bit_and_bookkeeping():
    md = fit_store()
    assert md.obs_fit_badness.shape == (16,) and md.obs_data_badness.shape == (16,) and not md.obs_fit_badness.any()
    md.score_group_fit_badness("g", ["T"], statement=True)
    assert same(md.obs_fit_badness, G["fit.badness"])
    psi = G["fit.psi"][:, 0]
    assert md.obs_fit_badness[psi == 8][0] == 0 and md.obs_fit_badness[psi == 11][0] == 0      # ignored, unfitted: NaN rows score 0
    assert not md.obs_fit_badness[psi >= 14].any()                                              # the other group is untouched
    assert md.obs_fit_badness[psi == 5][0] > 2
    md.add_observation([20.0], None, None, group_id="g")
    assert md.obs_fit_badness.shape == (17,) and md.obs_fit_badness[-1] == 0 and md.obs_data_badness.shape == (17,)


@pytest.mark.parametrize("kind", ["hybrid", "mixed"])
def test_store_data_score_bit_for_bit(kind):
    md, order = data_store(kind)
    md.score_group_data_badness("g", ["T"], statement=True)
    assert same(md.obs_data_badness, G[f"data.{kind}.badness"][order])             # rows land at get_group_index order
    assert np.argmax(md.obs_data_badness) == list(order).index(5)


def test_store_extension_beyond_upstream():
    """a group without chrono data is scored on its EIS part alone, one without EIS data on its chrono part alone"""
    md, order = data_store("hybrid")
    t, f = G["data.hybrid.t"], G["data.hybrid.f"]
    z = np.stack([np.concatenate([G["data.hybrid.z"][k].real, G["data.hybrid.z"][k].imag]) for k in range(12)])
    z_rss = nddata.score_rows_statement(z, (3, 1), (5, 3), ignore_outliers=True)
    v_rss = nddata.score_rows_statement(G["data.hybrid.v"], (3, 1), (5, 3), scale_src=G["data.hybrid.i"], ignore_outliers=True)
    assert same(0.5 * (v_rss + z_rss), G["data.hybrid.badness"])
    eis_only, _ = data_store("hybrid", chrono=False)
    eis_only.score_group_data_badness("g", ["T"], statement=True)
    assert same(eis_only.obs_data_badness, z_rss[order])
    chrono_only, _ = data_store("hybrid", eis=False)
    chrono_only.score_group_data_badness("g", ["T"], statement=True)
    assert same(chrono_only.obs_data_badness, v_rss[order])
    # an observation without EIS data among hybrid ones: a NaN row of the impedance array, scored on its chrono part
    md = DRTMD(np.logspace(-7, 2, 91), drt=object(), psi_dim_names=["T"])
    for k in range(12):
        md.add_observation([float(k)], (t, G["data.hybrid.i"][k], G["data.hybrid.v"][k]), None if k == 3 else (f, G["data.hybrid.z"][k]),
                           group_id="g")
    md.score_group_data_badness("g", ["T"], statement=True)
    assert md.obs_data_badness[3] == v_rss[3] and np.all(np.isfinite(md.obs_data_badness))


def test_not_implemented_name_the_argument():
    a = G["rank.a23.in"]
    md = fit_store()
    from hipdrt import filters
    for mod in (ndfilters, filters):
        with pytest.raises(NotImplementedError, match="footprint"):
            mod.median_filter(a, footprint=np.ones((3, 3)))
        with pytest.raises(NotImplementedError, match="origin"):
            mod.percentile_filter(a, 25, size=3, origin=1)
        with pytest.raises(NotImplementedError, match="mode"):
            mod.iqr_filter(a, size=(5, 3), mode="nearest")
        with pytest.raises(NotImplementedError, match="input"):
            mod.median_filter(a[0], size=3)
    with pytest.raises(NotImplementedError, match="size"):
        filters.median_filter(a, size=(8, 7))
    for fn in (nddata.flag_bad_obs, nddata.flag_bad_obs_statement):
        with pytest.raises(NotImplementedError, match="test_factor_correction"):
            fn(a, a, test_factor_correction=True)
        with pytest.raises(NotImplementedError, match="test_offset_correction"):
            fn(a, a, test_offset_correction=True)
        with pytest.raises(NotImplementedError, match="robust_std"):
            fn(a, a, robust_std=False)
        with pytest.raises(NotImplementedError, match="x_raw"):
            fn([a], [a])
    with pytest.raises(NotImplementedError, match="include_special"):
        md.score_group_fit_badness("g", ["T"], include_special=True, statement=True)
    with pytest.raises(NotImplementedError, match="impute"):
        md.score_group_data_badness("g", ["T"], impute=True, statement=True)


def test_x_std_with_nans_is_the_reference_error():
    a = np.full((6, 9), np.nan)
    with pytest.raises(ValueError, match="x_std contains nans"):
        nddata.flag_bad_obs_statement(a, a, std_size=(5, 3))
