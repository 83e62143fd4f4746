"""CPU: the numpy statement of csrc/peak_resolve.hip (hipdrt/models/peaks.py: find_troughs, peak_epsilons, peak_weights,
resolve_peaks_row, window_integrals) against a run of the reference (tests/golden/refrun_peak_resolve_golden71x91.npz, made by
tools/make_peak_resolve_golden.py) and against hand-written cases of every branch of the rule."""
import os

import numpy as np
import pytest

from conftest import ROOT

from hipdrt.models import peaks, predict

GOLD = os.path.join(ROOT, "tests", "golden", "refrun_peak_resolve_golden71x91.npz")
TAGS = ("plain", "nn", "sneg")
RTOL = 1e-12          # of the array's peak: the statement differs from upstream by the rounding of ln differences only


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD)


def close(a, ref, tol=RTOL):
    a, ref = np.asarray(a, dtype=float), np.asarray(ref, dtype=float)
    assert a.shape == ref.shape, (a.shape, ref.shape)
    assert np.max(np.abs(a - ref)) <= tol * np.max(np.abs(ref)), np.max(np.abs(a - ref)) / np.max(np.abs(ref))


def resolve(g, tag, tau_out=None):
    bt, eps = g[f"{tag}_basis_tau"], float(g[f"{tag}_tau_epsilon"])
    e0 = None if tau_out is None else predict.eval_matrix(bt, tau_out, eps)
    return peaks.resolve_peaks_row(g[f"{tag}_f"], g[f"{tag}_fxx"], g[f"{tag}_peak_index"], g[f"{tag}_x_red"],
                                   np.log(g[f"{tag}_tau10"]), np.log(bt), e0=e0,
                                   ln_tau_out=None if tau_out is None else np.log(tau_out), basis_area=predict.basis_area(eps))


@pytest.mark.parametrize("tag", TAGS)
def test_troughs_and_coefficients_match_the_reference(gold, tag):
    out = resolve(gold, tag)
    assert out["peak_index"].tolist() == gold[f"{tag}_peak_index"].tolist()
    assert out["troughs"].tolist() == gold[f"{tag}_trough_index"].tolist()
    close(out["x_peaks"], gold[f"{tag}_x_peaks"])
    # the weights are a partition of unity: the peak coefficients add up to the reduced coefficients
    close(np.sum(out["x_peaks"], axis=0), gold[f"{tag}_x_red"], 1e-14)


def test_the_fixture_covers_both_same_sign_branches(gold):
    assert gold["plain_peak_index"].tolist() == [19, 38, 67, 82] and gold["plain_trough_index"].tolist() == [23, 47, 81]
    assert gold["nn_peak_index"].tolist() == [38, 67, 82] and gold["nn_trough_index"].tolist() == [47, 81]
    assert gold["sneg_missing"].tolist() == ["split_resolved"] and not len(gold["plain_missing"]) and not len(gold["nn_missing"])


@pytest.mark.parametrize("tag", TAGS)
@pytest.mark.parametrize("grid", ("10", "20"))
def test_peak_drts_and_resistances_match_the_reference(gold, tag, grid):
    out = resolve(gold, tag, gold[f"{tag}_tau{grid}"])
    close(out["peak_gammas"], gold[f"{tag}_peak_gammas{grid}"])
    close(out["r_peaks"], gold[f"{tag}_r_peaks{grid}"])


@pytest.mark.parametrize("tag", TAGS)
def test_windows_match_the_reference(gold, tag):
    tau20, bt, eps = gold[f"{tag}_tau20"], gold[f"{tag}_basis_tau"], float(gold[f"{tag}_tau_epsilon"])
    start, end = peaks.split_windows(tau20, gold["tau_splits"])
    assert len(start) == 3 and start[0] == 0 and end[-1] == len(tau20) + 1
    close(peaks.window_integrals(gold[f"{tag}_f20"], np.log(tau20), start, end), gold[f"{tag}_split"])
    lo, hi = gold["integrate_lim"]
    tau = np.logspace(np.log10(lo), np.log10(hi), int((np.log10(hi) - np.log10(lo)) * 10) + 1)
    row = predict.drt(gold[f"{tag}_x"], bt, tau, eps)
    close(peaks.window_integrals(row, np.log(tau), [0], [len(tau)]), [gold[f"{tag}_integral"]])
    if f"{tag}_split_resolved" in gold.files:
        pk = peaks.window_peaks(gold[f"{tag}_fxx20"], start, end)
        out = peaks.resolve_peaks_row(gold[f"{tag}_f20"], gold[f"{tag}_fxx20"], pk, gold[f"{tag}_x_red"], np.log(tau20), np.log(bt),
                                      basis_area=predict.basis_area(eps))
        close(out["r_coef"], gold[f"{tag}_split_resolved"])


# ---- hand-written cases -------------------------------------------------------------------------------------------------------
Z5 = np.zeros(5)


def test_trough_local_minimum_branch():
    assert peaks.find_troughs([0, 3, 1, 2, 0], Z5, [1, 3]).tolist() == [2]
    assert peaks.find_troughs([0, -3, -1, -2, 0], Z5, [1, 3]).tolist() == [2]          # (negative peaks: the sign is taken out)


def test_trough_f_minus_fxx_branch():
    # f falls from the left peak to the right one: no local minimum; -(f - fxx) is largest at index 2
    assert peaks.find_troughs([0, 5, 4, 3, 0], [0, 0, 10, 0, 0], [1, 3]).tolist() == [2]


def test_trough_halfway_rule():
    # the maximum of -(f - fxx) is at the left peak: halfway between it and the middle of the pair
    f = np.array([0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 0], dtype=float)
    assert peaks.find_troughs(f, np.zeros(11), [1, 9]).tolist() == [int((1 + 9 + 2) / 4)] == [3]
    # ... which lands on the peak itself for neighbours two apart: a zero distance, eps = max_epsilon
    tr = peaks.find_troughs([0, 3, 4, 5, 0], Z5, [1, 3])
    assert tr.tolist() == [1]
    lt = np.arange(5, dtype=float)
    el, er = peaks.peak_epsilons(lt, [1, 3], tr, epsilon_factor=1.25, max_epsilon=0.7)
    assert er[0] == 0.7 and el[1] == 1.25 / 2 and el[0] == 0.7 and er[1] == 0.7          # (1.25 / 1 is clipped too)


def test_trough_sign_change_and_exact_zero():
    assert peaks.find_troughs([0, 2, 1, -0.5, -3, 0], np.zeros(6), [1, 4]).tolist() == [3]
    # np.sign(0) = 0: two zero peaks take the same-sign branch with v = 0 everywhere, i.e. the halfway rule from s
    assert peaks.find_troughs([0, 0, 7, 7, 7, 0, 0], np.ones(7), [1, 5]).tolist() == [int((1 + 5 + 2) / 4)] == [2]
    # a zero peak beside a positive one: the signs differ, the trough is the first smallest |f|, the zero peak itself
    assert peaks.find_troughs([0, 0, 7, 2, 0], Z5, [1, 3]).tolist() == [1]


def test_first_index_wins_ties():
    assert peaks.find_troughs([0, 3, 1, 1, 1, 2, 0], np.zeros(7), [1, 5]).tolist() == [2]
    assert peaks.find_troughs([0, 5, 4, 4, 3, 0], [0, 0, 10, 10, 0, 0], [1, 4]).tolist() == [2]
    assert peaks.find_troughs([0, 2, 1, -1, -3, 0], np.zeros(6), [1, 4]).tolist() == [2]
    assert peaks.window_peaks([3, 1, 1, 4, 0, 0], [0, 2], [3, 7]).tolist() == [1, 4]


def test_no_peak_and_one_peak():
    lt, lb, x = np.arange(6.0), np.array([0.5, 2.5, 4.5]), np.array([1.0, -2.0, 3.0])
    f = np.array([0, 1, 2, 1, 0, 0], dtype=float)
    out = peaks.resolve_peaks_row(f, -f, [], x, lt, lb, basis_area=2.0)
    assert out["x_peaks"].shape == (0, 3) and out["troughs"].shape == (0,) and out["r_coef"].shape == (0,)
    out = peaks.resolve_peaks_row(f, -f, [2], x, lt, lb, basis_area=2.0)
    assert out["x_peaks"].tolist() == [x.tolist()] and out["r_coef"].tolist() == [4.0] and out["troughs"].shape == (0,)
    assert out["eps_l"].tolist() == [1.25 / 2] and out["eps_r"].tolist() == [1.25 / 3]


def test_min_epsilon_and_epsilon_uniform():
    lt = np.arange(0.0, 40.0, 4.0)
    el, er = peaks.peak_epsilons(lt, [2, 6], [4])
    assert el.tolist() == [1.25 / 8, 1.25 / 8] and er.tolist() == [1.25 / 8, 1.25 / 12]
    el, er = peaks.peak_epsilons(lt, [2, 6], [4], min_epsilon=0.15)
    assert el.tolist() == [1.25 / 8, 1.25 / 8] and er.tolist() == [1.25 / 8, 0.15]
    el, er = peaks.peak_epsilons(lt, [2, 6], [4], epsilon_uniform=0.3, min_epsilon=0.5)
    assert el.tolist() == [0.3, 0.3] and er.tolist() == [0.3, 0.3]


def test_weights_sides_normalisation_and_the_nan_column():
    lb = np.array([-2.0, 0.0, 1.0, 3.0, 400.0])
    w = peaks.peak_weights(lb, [0.0, 3.0], [0.5, 0.25], [1.0, 2.0])
    raw = np.array([[np.exp(-(0.5 * -2.0) ** 2), 1.0, np.exp(-(1.0 * 1.0) ** 2), np.exp(-(1.0 * 3.0) ** 2)],
                    [np.exp(-(0.25 * -5.0) ** 2), np.exp(-(0.25 * -3.0) ** 2), np.exp(-(0.25 * -2.0) ** 2), 1.0]])
    assert np.array_equal(w[:, :4], raw / (raw[0] + raw[1]))
    # a basis point on a peak has y = 0: weight 1 before the normalisation, whichever side's eps it takes (it takes the right one)
    assert w[0, 1] == 1.0 / (1.0 + raw[1, 1]) and w[1, 3] == 1.0 / (raw[0, 3] + 1.0)
    # 400 ln units from every peak all weights underflow: 0 / 0 = NaN, as the reference gives
    assert np.isnan(w[:, 4]).all() and np.isfinite(w[:, :4]).all()


def test_window_integrals_clip_like_a_slice():
    y, lt = np.array([1.0, 3.0, 2.0, 5.0]), np.array([0.0, 1.0, 3.0, 4.0])
    got = peaks.window_integrals(y, lt, [0, 1, 2], [2, 3, 5])
    assert got.tolist() == [2.0, 5.0, 3.5]
    assert peaks.split_windows(np.array([1e-3, 1e-2, 1e-1, 1.0]), [0.2, 1e-3])[0].tolist() == [0, 0, 2]
