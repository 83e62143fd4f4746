"""CPU: hipdrt.models.peaks, the numpy statement of csrc/peaks.hip.

1. find_peaks_1d against scipy.signal.find_peaks (height and prominence) on random small-integer rows, which are full of plateaus
   and ties, and on the hand cases;
2. the automatic thresholds, the two-pass merge, the 'prob' filter, num_peaks with a tie and the map forms against the formulas
   written out with math.erfc, on the rows of the reference's recorded run (tools/make_peaks_golden.py): masks and indices
   exactly as the reference recorded them, floats at 1e-12."""
import math
import os

import numpy as np
import pytest

from conftest import GOLDEN

from hipdrt.models import peaks

FITS = {"plain": 1, "nn": 0, "sneg": 0}           # tag -> search (upstream: sign if nonneg and sign != 0 else 0)
KEYS = ("peak_heights", "prominences", "left_bases", "right_bases")


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "refrun_peaks_golden71x91.npz"))


# ---- 1. the restated scipy rule -------------------------------------------------------------------------------------------------
def same_as_scipy(v, height, prominence):
    signal = pytest.importorskip("scipy.signal")
    ref_idx, ref = signal.find_peaks(np.asarray(v, dtype=float), height=height, prominence=prominence)
    idx, info = peaks.find_peaks_1d(v, height, prominence)
    np.testing.assert_array_equal(idx, ref_idx, err_msg=str(v))
    for k in ref:                    # (scipy returns the properties of the conditions it was given)
        np.testing.assert_array_equal(info[k], ref[k], err_msg=f"{k} {v}")
    return len(idx)


def test_local_maxima_and_prominences_against_scipy_on_random_rows():
    rng = np.random.default_rng(20261018)
    total = 0
    for _ in range(4000):
        n = int(rng.integers(1, 41))
        v = rng.integers(-4, 5, n).astype(float)
        total += same_as_scipy(v, float(rng.integers(-4, 4)), float(rng.integers(0, 5)))
    assert total > 5000          # the comparison is not vacuous


@pytest.mark.parametrize("v", [
    [1], [1, 2], [2, 1], [1, 2, 1], [1, 1, 1], [2, 1, 2],
    [3, 3, 1, 2, 1],                 # a plateau touching the left end
    [1, 2, 1, 3, 3],                 # a plateau touching the right end: no peak
    [1, 3, 3, 1], [1, 3, 3, 3, 1], [0, 1, 3, 3, 3, 3, 0],
    [5, 5, 5, 5, 5],                 # all equal
    [1, 2, 3, 4, 5], [5, 4, 3, 2, 1],
    [0, 2, 0, 1, 0, 5, 0, 3],        # two equal minima on the left of the highest peak: the nearest is the base
    [3, 0, 5, 0, 1, 0, 2, 4],        # ... and on the right
    [0, 1, 0],                       # both walks reach the array edge
    [2, 0, 3, 0, 9, 1, 4, 1],        # the highest peak's walks reach both edges
    [1, 2, 2, 1, 2, 2, 1, 0, 3, 3, 3, 0],
])
def test_hand_cases_against_scipy(v):
    for height in (None, 0, 3):
        for prominence in (None, 0, 1, 2):
            same_as_scipy(v, height, prominence)


# ---- 2. the reference's logic on the recorded rows ---------------------------------------------------------------------------------
def manual_std(x):
    mean = math.fsum(x) / len(x)
    return math.sqrt(math.fsum(abs(t - mean) ** 2 for t in x) / len(x))


@pytest.mark.parametrize("tag", list(FITS))
def test_thresholds_merge_and_prob_filter_on_the_recorded_rows(golden, tag):
    g, search = golden, FITS[tag]
    f, fxx = g[f"{tag}_f"], g[f"{tag}_fxx"]
    var = g[f"{tag}_sigma_fxx"] ** 2                  # extend_var is in the recorded row already; the floor is not
    # automatic thresholds
    prom, height = peaks.auto_thresholds(fxx, "thresh")
    assert abs(prom - (0.05 * manual_std(fxx.tolist()) + 5e-3)) <= 1e-12 and height == 0
    assert peaks.auto_thresholds(fxx, "prob") == (5e-3, 1e-3)
    assert peaks.auto_thresholds(fxx, "thresh", prominence=0.3, height=0.1) == (0.3, 0.1)
    # the two-pass merge is the ascending union of the passes that survive the f test
    if search == 0:
        idx, info, signs = peaks.search_peaks(fxx, f, 0, height, prom)
        want = []
        for s in (-1, 1):
            i_s, d_s = peaks.find_peaks_1d(-s * fxx, height, prom)
            want += [(int(i), s, float(h)) for i, h in zip(i_s, d_s["peak_heights"]) if s * f[i] > 0]
        want.sort()
        assert [(int(i), int(s), float(h)) for i, s, h in zip(idx, signs, info["peak_heights"])] == want
    for m, kw in (("thresh", dict(method="thresh")), ("prob", dict(method="prob")), ("prob1", dict(method="prob", num_peaks=1))):
        kept, idx, info, _, _ = peaks.find_peaks_row(fxx, f, var, search=search, **kw)
        np.testing.assert_array_equal(kept, g[f"{tag}_{m}_idx"])
        for k in KEYS:
            np.testing.assert_allclose(info[k], g[f"{tag}_{m}_{k}"], rtol=0, atol=1e-12)
        if kw["method"] == "prob":
            mp = np.minimum(info["prominences"], info["peak_heights"])
            sig = np.sqrt(np.maximum(var, 1e-5))[idx]
            manual = np.array([1 - math.erfc(a / (s * math.sqrt(2))) for a, s in zip(mp, sig)])
            np.testing.assert_allclose(info["probs"], manual, rtol=0, atol=1e-12)
            np.testing.assert_allclose(info["probs"], g[f"{tag}_{m}_probs"], rtol=0, atol=1e-12)
            thr = 0.25 if "num_peaks" not in kw else np.sort(manual)[::-1][min(kw["num_peaks"], len(manual)) - 1]
            np.testing.assert_array_equal(kept, idx[manual >= thr])


def test_num_peaks_keeps_ties():
    fxx = -np.array([0, 4, 0, 4, 0, 2, 0], dtype=float)          # two equal peaks and a smaller one
    var = np.full(7, 4.0)
    for k, want in ((1, [1, 3]), (2, [1, 3]), (3, [1, 3, 5]), (7, [1, 3, 5])):
        kept, idx, info, _, _ = peaks.find_peaks_row(fxx, None, var, method="prob", prominence=1, height=1, num_peaks=k)
        assert kept.tolist() == want and idx.tolist() == [1, 3, 5]
    assert info["probs"][0] == info["probs"][1] == 1 - math.erfc(4 / (2 * math.sqrt(2)))
    with pytest.raises(ValueError, match="Invalid method"):
        peaks.find_peaks_row(fxx, method="best")


def test_extend_var_and_floor():
    var = np.array([1, 5, 2, 9, 3, 1, 4], dtype=float)
    np.testing.assert_array_equal(peaks.extend_var(var, 2, 4), [2, 5, 2, 9, 3, 3, 4])
    np.testing.assert_array_equal(peaks.extend_var(var, -1, -1, 2.5), [2.5, 5, 2.5, 9, 3, 2.5, 4])
    np.testing.assert_array_equal(peaks.extend_var(var, 4, 1), [3, 5, 5, 9, 5, 5, 5])      # the right bound is a clamped value


@pytest.mark.parametrize("tag", list(FITS))
def test_map_forms_on_the_recorded_rows(golden, tag):
    g, search = golden, FITS[tag]
    f, fxx, sf, sxx = (g[f"{tag}_{k}"] for k in ("f", "fxx", "sigma_f", "sigma_fxx"))
    pp = peaks.peak_prob_row(f, fxx, sf ** 2, sxx ** 2, search=search)
    cp = peaks.curv_prob_row(f, fxx, sf ** 2, sxx ** 2)
    np.testing.assert_array_equal(np.flatnonzero(pp), np.flatnonzero(g[f"{tag}_peak_prob"]))
    np.testing.assert_allclose(pp, g[f"{tag}_peak_prob"], rtol=0, atol=1e-12)
    np.testing.assert_allclose(cp, g[f"{tag}_curv_prob"], rtol=0, atol=1e-12)
    up = lambda mu, s: 1 - 0.5 * math.erfc(mu / (s * math.sqrt(2)))          # noqa: E731
    idx, info, _ = peaks.search_peaks(fxx, f, search, 1e-3, 5e-3)
    manual = np.zeros(len(f))
    for i, a in zip(idx, np.minimum(info["prominences"], info["peak_heights"])):
        manual[i] = min(up(a, sxx[i]), up(abs(f[i]), sf[i])) * np.sign(f[i])
    np.testing.assert_allclose(pp, manual, rtol=0, atol=1e-12)
    manual = [min(2 * max(up(-np.sign(b) * a, s1) - 0.5, 0), 2 * max(up(-np.sign(a) * b, s2) - 0.5, 0)) * np.sign(a)
              for a, b, s1, s2 in zip(f, fxx, sf, sxx)]
    np.testing.assert_allclose(cp, manual, rtol=0, atol=1e-12)
    dense = peaks.find_peaks_dense(fxx, f, sxx ** 2, sf ** 2, search=search, method=2, fxx_var_floor=0.0)
    np.testing.assert_array_equal(dense["peak_prob"], pp)
    np.testing.assert_array_equal(dense["curv_prob"], cp)
    assert dense["count"] == len(idx) and dense["keep"].sum() == len(idx)
