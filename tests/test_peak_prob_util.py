"""CPU: the peak-probability part of hipdrt.models.peaks, the numpy statement of csrc/peak_prob.hip.

1. against the reference's recorded run (tools/make_peak_prob_golden.py): pp, tp and prob from the recorded rows for both
   bayes_cov, the floor, the filtered sigma -- each at the bound tests/peak_prob_bounds.json holds for it (30 x what the
   generator measured, rounded up to 1 / 2 / 5 x 10^k, never below 1e-12: the margin is for scipy's running-sum uniform_filter
   and ndtr against a direct sum and math.erfc) -- and the indices of find_peaks_byprob, by thresholds and by ranges, which must
   be equal (the generator writes the fixture only when they are decided with a margin);
2. the conventions: numpy's 'linear' percentile and the median for n = 1, 2, 3, 4, 5, 8; 'reflect' indices for rows shorter than
   the window; sgn(0) = 0; an all-zero row; a window without a positive sample."""
import json
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

from hipdrt.models import peaks

TAGS = ("plain", "nn", "sneg")
ORDERS = ("f", "fx", "fxx")
INFO_KEYS = ("peak_heights", "prominences", "left_bases", "right_bases")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "refrun_peak_prob_golden71x91.npz"))


@pytest.fixture(scope="module")
def bounds():
    with open(os.path.join(ROOT, "tests", "peak_prob_bounds.json")) as f:
        return json.load(f)


def within(bounds, label, actual, desired, relative=False):
    actual, desired = np.asarray(actual, dtype=float), np.asarray(desired, dtype=float)
    err = float(np.max(np.abs(actual - desired)))
    if relative:
        err /= float(np.max(np.abs(desired)))
    print(f"{label}: measured {err:.2e} bound {bounds[label][1]:.0e}")
    assert err <= bounds[label][1], (label, err, bounds[label])


# ---- 1. the recorded run ------------------------------------------------------------------------------------------------------------
def test_bounds_table_follows_its_rule(bounds):
    assert len(bounds) == 3 * (6 + 6)
    for label, (measured, bound) in bounds.items():
        assert bound >= 1e-12 and bound >= 30 * measured * (1 - 1e-9), label
        mant = bound / 10.0 ** math.floor(math.log10(bound) + 1e-9)
        assert min(abs(mant - m) for m in (1, 2, 5)) < 1e-6, (label, bound)
        assert bound <= max(1e-12, 30 * measured * 2.5 * (1 + 1e-9)), label          # (the next step of 1 / 2 / 5 is at most 2.5 x)


@pytest.mark.parametrize("tag", TAGS)
def test_floor_and_filtered_sigma_against_the_recorded_run(golden, bounds, tag):
    rows, sig = golden[f"{tag}_rows"], golden[f"{tag}_sigma"]
    for k, name in enumerate(ORDERS):
        within(bounds, f"{tag}:sigma_floor_{name}", peaks.sigma_floor_value(sig[k]), golden[f"{tag}_sigma_floors"][k], True)
        within(bounds, f"{tag}:filtered_sigma_{name}", peaks.filtered_sigma(rows[k]), golden[f"{tag}_filtered_sigma"][k], True)
        fl = golden[f"{tag}_sigma_floors"][k]
        np.testing.assert_array_equal(peaks.sigma_floor(sig[k]), np.where(sig[k] < fl, peaks.sigma_floor_value(sig[k]), sig[k]))
    # what the issue observed of the reference: the floor of order 0 is active for 'plain' and 'nn' (6 samples), and for nothing else
    active = [int(np.sum(sig[k] < golden[f"{tag}_sigma_floors"][k])) for k in range(3)]
    assert active == ([6, 0, 0] if tag != "sneg" else [0, 0, 0])


@pytest.mark.parametrize("bayes_cov", [1, 0])
@pytest.mark.parametrize("tag", TAGS)
def test_probabilities_and_searches_against_the_recorded_run(golden, bounds, tag, bayes_cov):
    g, tau = golden, golden["tau"]
    rows = g[f"{tag}_rows"]
    var = g[f"{tag}_sigma"] ** 2 if bayes_cov else (None, None, None)       # extend_var is in the recorded rows already
    pp, tp, sigma = peaks.peak_trough_probs_rows(*rows, *var)
    prob = peaks.peak_prob_of(pp, tp)
    ref_pp, ref_tp = g[f"{tag}_pp_b{bayes_cov}"], g[f"{tag}_tp_b{bayes_cov}"]
    within(bounds, f"{tag}:pp_b{bayes_cov}", pp, ref_pp)
    within(bounds, f"{tag}:tp_b{bayes_cov}", tp, ref_tp)
    within(bounds, f"{tag}:prob_b{bayes_cov}", prob, ref_pp * (1 - ref_tp))
    assert sigma.shape == rows.shape and (sigma > 0).all()
    for height, prominence in g["thresholds"]:
        key = f"{tag}_b{bayes_cov}_h{height:g}_p{prominence:g}"
        idx, info = peaks.find_peaks_byprob_row(prob, height, prominence)
        np.testing.assert_array_equal(idx, g[f"{key}_idx"], err_msg=key)
        assert set(info) == set(INFO_KEYS)
        for k in ("left_bases", "right_bases"):
            np.testing.assert_array_equal(info[k], g[f"{key}_{k}"], err_msg=key)
        for k in ("peak_heights", "prominences"):
            np.testing.assert_allclose(info[k], g[f"{key}_{k}"], rtol=0, atol=bounds[f"{tag}:prob_b{bayes_cov}"][1], err_msg=key)
    ranges = [tuple(r) for r in g["ranges"]]
    np.testing.assert_array_equal(peaks.find_peaks_byrange(tau, prob, ranges), g[f"{tag}_b{bayes_cov}_ranges_idx"])
    np.testing.assert_array_equal(peaks.find_peaks_byindex(prob, peaks.range_windows(tau, ranges)), g[f"{tag}_b{bayes_cov}_ranges_idx"])
    if bayes_cov:
        # what the issue observed of the reference: both searches find tau = 1.004e-5 and 7.977e-3
        np.testing.assert_allclose(tau[peaks.find_peaks_byprob_row(prob, 0.5, 0.25)[0]], [1.004e-5, 7.977e-3], rtol=1e-3)
        np.testing.assert_allclose(tau[g[f"{tag}_b1_ranges_idx"]], [1.004e-5, 7.977e-3], rtol=1e-3)


def test_info_keys_follow_the_conditions_given(golden):
    pp, tp, _ = peaks.peak_trough_probs_rows(*golden["plain_rows"], *(golden["plain_sigma"] ** 2))
    prob = peaks.peak_prob_of(pp, tp)
    assert set(peaks.find_peaks_byprob_row(prob)[1]) == set()
    assert set(peaks.find_peaks_byprob_row(prob, height=0.1)[1]) == {"peak_heights"}
    assert set(peaks.find_peaks_byprob_row(prob, prominence=0.1)[1]) == {"prominences", "left_bases", "right_bases"}
    assert len(peaks.find_peaks_byprob_row(prob)[0]) == 5                             # (None, None): every local maximum
    signal = pytest.importorskip("scipy.signal")
    for height, prominence in ((None, None), (0.1, None), (None, 0.1), (0.5, 0.25)):
        idx, info = peaks.find_peaks_byprob_row(prob, height, prominence)
        ref_idx, ref = signal.find_peaks(prob, height=height, prominence=prominence)
        np.testing.assert_array_equal(idx, ref_idx)
        assert set(info) == set(ref)
        for k in ref:
            np.testing.assert_array_equal(info[k], ref[k])


# ---- 2. the conventions ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 8])
def test_percentile_and_median_conventions_against_numpy(n):
    rng = np.random.default_rng(n)
    for trial in range(50):
        s = rng.random(n) * 10.0 ** rng.integers(-3, 4) if trial % 2 else rng.integers(0, 4, n).astype(float)
        srt = np.sort(s)
        for q in (25, 75, 50):
            assert peaks.linear_quantile(srt, q / 100) == np.percentile(s, q), (s, q)
        ref = np.median(s) - 1.5 * (np.percentile(s, 75) - np.percentile(s, 25))
        assert peaks.sigma_floor_value(s) == ref, s
        out = s.copy()
        out[out < ref] = ref
        np.testing.assert_array_equal(peaks.sigma_floor(s), out)


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 9])
@pytest.mark.parametrize("size", [3, 5, 7])
def test_reflect_indices_for_rows_shorter_than_the_window(n, size):
    ndimage = pytest.importorskip("scipy.ndimage")
    rng = np.random.default_rng(10 * n + size)
    row = rng.integers(-3, 4, n).astype(float)                  # small integers: every order of summation gives the same bits
    mean = ndimage.uniform_filter(row, size, mode="reflect") / ndimage.uniform_filter(np.ones(n), size, mode="reflect")
    var = ndimage.uniform_filter((row - mean) ** 2, size, mode="reflect")
    var[var < 0] = 0
    np.testing.assert_allclose(peaks.filtered_sigma(row, size, 0.1), var ** 0.5 + 0.1 * np.std(row), rtol=1e-14, atol=1e-15)
    h = size // 2
    direct = np.array([sum(row[peaks.reflect_index(i + j, n)] for j in range(-h, h + 1)) / size for i in range(n)])
    np.testing.assert_array_equal(peaks._window_mean(row, size), direct)
    with pytest.raises(ValueError):
        peaks.filtered_sigma(row, size + 1)


def phi(z):
    return 0.5 * math.erfc(-z / 2 ** 0.5)


def test_sign_of_zero_is_zero():
    """np.sign(0) = 0: where f is zero the curvature's sign does not matter, fxx_prob and the trough factor are both 1 - Phi(0)"""
    f, fx, fxx = np.array([0.0, 0.0, 2.0]), np.array([0.5, 0.5, 0.5]), np.array([-3.0, 3.0, -3.0])
    pp, tp, sigma = peaks.peak_trough_probs_rows(f, fx, fxx, np.ones(3), np.full(3, 4.0), np.full(3, 16.0), floor=False)
    np.testing.assert_array_equal(sigma, [[1.0] * 3, [2.0] * 3, [4.0] * 3])
    fx_prob = phi((10.0 - 0.5) / 2.0) - phi((-10.0 - 0.5) / 2.0)
    assert pp[0] == pp[1] == (1.0 - phi(1.0)) * fx_prob * 0.5 and tp[0] == tp[1] == fx_prob * 0.5
    assert pp[2] == (1.0 - phi((1.0 - 2.0) / 1.0)) * fx_prob * (1.0 - phi(-3.0 / 4.0))
    assert tp[2] == fx_prob * (1.0 - phi(3.0 / 4.0))


def test_all_zero_row():
    z = np.zeros(7)
    np.testing.assert_array_equal(peaks.filtered_sigma(z), z)
    pp, tp, sigma = peaks.peak_trough_probs_rows(z, z, z)                              # sigma = 0: 0 / 0 in every argument
    assert np.isnan(pp).all() and np.isnan(tp).all() and not sigma.any()
    pp, tp, sigma = peaks.peak_trough_probs_rows(z, z, z, np.ones(7), np.ones(7), np.ones(7))
    fx_prob = phi(5.0) - phi(-5.0)
    np.testing.assert_array_equal(pp, np.full(7, (1.0 - phi(1.0)) * fx_prob * 0.5))
    np.testing.assert_array_equal(tp, np.full(7, fx_prob * 0.5))
    prob = peaks.peak_prob_of(pp, tp)
    assert len(peaks.find_peaks_byprob_row(prob)[0]) == 0                             # a constant row has no local maximum
    assert peaks.find_peaks_byprob_dense(np.zeros(7))["count"] == 0


def test_window_without_a_positive_sample_gives_index_zero():
    tau = np.logspace(-3, 3, 7)
    prob = np.array([0.2, 0.0, 0.0, 0.7, 0.7, 0.0, 0.1])
    ranges = [(5e-3, 5e-2), (1e-9, 1e9), (5e-1, 50.0), (50.0, 2000.0), (1e4, 1e5), (1.0, 0.1)]
    np.testing.assert_array_equal(peaks.find_peaks_byrange(tau, prob, ranges), [0, 3, 3, 6, 0, 0])
    win = peaks.range_windows(tau, ranges)
    np.testing.assert_array_equal(win, [(1, 1), (0, 6), (3, 4), (5, 6), (0, -1), (0, -1)])
    np.testing.assert_array_equal(peaks.find_peaks_byindex(prob, win), [0, 3, 3, 6, 0, 0])
    with pytest.raises(ValueError, match="strictly increasing"):
        peaks.range_windows(tau[::-1], ranges)
