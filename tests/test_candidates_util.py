"""CPU: the numpy statement of candidate ranking (hipdrt/models/candidates.py) against the reference's own generate_candidates runs
(tests/golden/refrun_generate_candidates_*.npz, tools/make_candidates_golden.py) and on hand-made cases.

Against the fixtures the discrete results are exact: BIC's parameter counts, the best index per peak count, the keys of the filled
best_candidate_dict with every entry's peaks, the order of both tables.  BIC, the relative columns and the Bayes factors are formed
from the fixture's own llh by the same few operations in the same order: a few ulp.

The llh bound.  The statement and the reference are two float64 evaluations of the same sums from the same rm, rv, vmm and x.
candidates_util.reference_and_bound bounds what any evaluation of "yh = rm x first" may deviate (derivation in
tests/test_gpu_candidates.py): b_rss, b_slw.  The reference forms rss as ((x (W rm)') (W rm)) x - 2 (W rv)'(W rm) x + (W rv)'(W rv)
instead, whose first two terms sum n products of magnitudes w |rm| |x| after the m products: with ay = |rm| |x| they add
(m + 2 n + 4) u sum (w ay)^2 and 2 (m + n + 4) u sum |w rv| w ay to its side; its s^-1/2 is a pow (2 u, as the square root and
division it replaces).  llh = alpha_0 ln beta_0 - alpha_n ln(beta_0 + rss / 2) + lgamma terms + slw moves by
alpha_n drss / (2 beta_0 + rss) for a change drss of rss and by drss_w for slw; both sides form it with the same routine from
their own rss, each rounding the logarithm, the product and three sums: 8 u (alpha_n |ln beta_n| + |lgamma(alpha_n)| + |slw|).
"""
import os

import numpy as np
import pytest

from candidates_util import U, llh_case, reference_and_bound
from conftest import GOLDEN

from hipdrt.models import candidates, qphb

CASES = ("golden71x91", "golden71x91_neg", "hybrid_s0")


@pytest.fixture(scope="module", params=CASES)
def golden(request):
    return np.load(os.path.join(GOLDEN, f"refrun_generate_candidates_{request.param}.npz"))


def rows_of(padded):
    return [r[~np.isnan(r)] for r in padded]


def ulp_close(a, b, ulps=8):
    a, b = np.asarray(a, dtype=float), np.asarray(b, dtype=float)
    assert a.shape == b.shape
    assert np.all(np.abs(a - b) <= ulps * np.spacing(np.maximum(np.abs(a), np.abs(b)))), np.max(np.abs(a - b))


def test_llh_statement_against_the_reference_run(golden):
    from scipy.special import loggamma
    g = golden
    x, rm, rv, vmm = g["x"], g["rm"], g["rv"], g["vmm"]
    m, n = rm.shape
    vf = np.var(rv) * 1e-7                                  # qphb.estimate_weights' default floor (qphb.py:1560-1561)
    rss, slw = candidates.candidate_llh_terms(x, rm, rv, vmm, vf)
    llh = qphb.marginal_llh(rss, m) + slw
    _, _, b_rss, b_slw = reference_and_bound(x[:, None, :], rm, rv[None], vmm, np.array([vf]))
    b_rss, b_slw = b_rss[:, 0], b_slw[:, 0]
    yh, ay = x @ rm.T, np.abs(x) @ np.abs(rm).T
    s = np.maximum(((yh - rv) ** 2) @ vmm.T, vf)
    w = np.maximum(1 / np.sqrt(s), 1e-10)
    ref_extra = (m + 2 * n + 4) * U * np.sum((w * ay) ** 2, -1) + 2 * (m + n + 4) * U * np.sum(np.abs(w * rv) * w * ay, -1)
    alpha_n = 2 - 1 + m / 2
    drss = 2 * b_rss + ref_extra
    bound = alpha_n * drss / (2 + rss) + 2 * b_slw + \
        2 * 8 * U * (alpha_n * np.abs(np.log(1 + 0.5 * rss)) + abs(float(loggamma(alpha_n))) + np.abs(slw))
    err = np.abs(llh - g["llh"])
    print(f"llh: worst deviation / bound {np.max(err / bound):.3f}, bound relative to |llh| {np.max(bound / np.abs(g['llh'])):.1e}")
    assert np.all(err <= bound), np.max(err / bound)


def test_ranking_against_the_reference_run(golden):
    g = golden
    heights, proms = rows_of(g["peak_heights"]), rows_of(g["prominences"])
    assert [len(h) for h in heights] == g["num_peaks"].tolist()
    r = candidates.rank_candidates(g["num_peaks"], g["llh"], int(g["num_special"]), int(g["num_independent_data"]), proms, heights)
    ulp_close(r["bic"], g["bic"])
    # candidate_df: every candidate in order; best_candidate_df: one row per peak count, ascending, model_id first
    cols = list(g["candidate_df_columns"])
    assert cols == list(r["candidate_table"]) and list(g["best_candidate_df_columns"]) == list(r["best_table"])
    for k, name in enumerate(cols):
        ulp_close(r["candidate_table"][name], g["candidate_df"][:, k])
    for k, name in enumerate(r["best_table"]):
        ulp_close(r["best_table"][name], g["best_candidate_df"][:, k])
    np.testing.assert_array_equal(r["best_table"]["num_peaks"], np.unique(g["num_peaks"]))
    # the best index per peak count reproduces the reference's entries exactly (llh and bic are copied, not recomputed)
    np.testing.assert_array_equal(g["llh"][r["best_indices"]], g["best_candidate_df"][:, 2])
    # the filled dict: keys, and every entry's peaks in the reference's order
    assert r["best_keys"] == g["best_keys"].tolist()
    peak_tau = rows_of(g["peak_tau"])
    best_tau = rows_of(g["best_peak_tau"])
    own = {int(k): i for k, i in zip(r["unique_num_peaks"], r["best_indices"])}
    for key, want, llh, bic in zip(g["best_keys"], best_tau, g["best_llh"], g["best_bic"]):
        if int(key) in own:
            i, tau = own[int(key)], peak_tau[own[int(key)]]
        else:
            hi_num, order = r["filled"][int(key)]
            i, tau = own[hi_num], peak_tau[own[hi_num]][order]
        np.testing.assert_array_equal(tau, want)
        assert g["llh"][i] == llh and len(want) == key
        ulp_close(r["bic"][i], bic)
    # evaluate_bic of the fit itself: stats.bic on the reference's own evaluate_llh() and peak count
    ulp_close(candidates.bic(int(g["num_special"]) + 4 * int(g["fit_num_peaks"]), int(g["num_independent_data"]), float(g["evaluate_llh"])),
              float(g["evaluate_bic"]))
    ulp_close(candidates.norm_bayes_factors(r["best_table"]["bic"]), g["norm_bayes_factors"])
    assert r["best_table"]["model_id"][np.argmin(r["best_table"]["bic"])] == g["best_id"]


def test_statement_in_float64_stays_inside_the_derived_bound():
    """the bound the GPU tests assert, exercised on the CPU: numpy's own float64 evaluation against np.longdouble"""
    for m, n in ((2, 1), (18, 5), (142, 93)):
        x, rm, rv, vmm, vf = llh_case(np.random.default_rng(m), 17, 2, m, n, True)
        r_rss, r_slw, b_rss, b_slw = reference_and_bound(x, rm, rv, vmm, vf)
        for b in range(2):
            rss, slw = candidates.candidate_llh_terms(x[:, b], rm[b], rv[b], vmm, vf[b])
            assert np.all(np.abs(rss - r_rss[:, b]) <= b_rss[:, b]) and np.all(np.abs(slw - r_slw[:, b]) <= b_slw[:, b])
        assert np.max(b_rss / np.abs(r_rss)) < 1e-11 and np.max(b_slw / np.abs(r_slw)) < 1e-11       # (and it is not vacuous)


# ---- hand-made cases ------------------------------------------------------------------------------------------------------------------
def test_best_per_num_peaks_takes_the_first_index_at_ties():
    num_peaks = np.array([3, 1, 3, 1, 3, 2])
    llh = np.array([5.0, -1.0, 7.0, -1.0, 7.0, 0.5])
    unique, best = candidates.best_per_num_peaks(num_peaks, llh)
    assert unique.tolist() == [1, 2, 3] and best.tolist() == [1, 5, 2]


def peaks_of(k):
    """k peaks whose min(prominence, height) descends in the order k - 1, 0, k - 2, 1, ...: (prominences, heights)"""
    order = [k - 1, 0] + [j for pair in zip(range(k - 2, 0, -1), range(1, k - 1)) for j in pair]
    order = list(dict.fromkeys(order))[:k]
    value = np.empty(k)
    value[order] = np.arange(k, 0, -1.0)
    prom, height = value + 10.0, value.copy()
    prom[::2], height[::2] = value[::2], value[::2] + 10.0       # the minimum alternates between the two
    return prom, height, order


def test_fill_none_negative_and_below_the_simplest():
    prom3, height3, order3 = peaks_of(3)
    best = {3: (prom3, height3), 4: peaks_of(4)[:2]}
    assert candidates.fill_candidates([3, 4], best) == {}                       # None: nothing below the simplest candidate
    got = candidates.fill_candidates([3, 4], best, min_fill_num=-1)             # one count below it
    assert sorted(got) == [2] and got[2][0] == 3 and got[2][1].tolist() == order3[:2]
    got = candidates.fill_candidates([3, 4], best, min_fill_num=-7)             # never below one peak
    assert sorted(got) == [1, 2] and got[1][1].tolist() == order3[:1] and got[2][1].tolist() == order3[:2]
    got = candidates.fill_candidates([3, 4], best, min_fill_num=2)              # an explicit count below the simplest
    assert sorted(got) == [2] and got[2][0] == 3
    assert candidates.fill_candidates([3, 4], best, min_fill_num=3) == {}       # the simplest itself: nothing to add
    assert candidates.fill_candidates([3, 4], best, min_fill_num=9) == {}       # above it: nothing either


def test_fill_a_gap_of_three_counts():
    prom6, height6, order6 = peaks_of(6)
    best = {2: peaks_of(2)[:2], 6: (prom6, height6), 7: peaks_of(7)[:2]}
    got = candidates.fill_candidates([2, 6, 7], best)
    assert sorted(got) == [3, 4, 5]
    for j in (3, 4, 5):
        assert got[j][0] == 6 and got[j][1].tolist() == order6[:j]              # the j most prominent peaks of the richer candidate
    r = candidates.rank_candidates([2, 6, 7, 6], [1.0, 3.0, 2.0, 2.5], 2, 71, [peaks_of(k)[0] for k in (2, 6, 7, 6)],
                                   [peaks_of(k)[1] for k in (2, 6, 7, 6)])
    assert r["best_keys"] == [2, 3, 4, 5, 6, 7] and r["best_indices"].tolist() == [0, 1, 2]
    assert r["best_table"]["model_id"].tolist() == [2.0, 6.0, 7.0]
    np.testing.assert_array_equal(r["bic"], (2 + 4 * np.array([2, 6, 7, 6])) * np.log(71) - 2 * np.array([1.0, 3.0, 2.0, 2.5]))
    np.testing.assert_array_equal(r["candidate_table"]["rel_llh"], np.array([1.0, 3.0, 2.0, 2.5]) - 3.0)
    np.testing.assert_array_equal(r["candidate_table"]["rel_bic"], r["bic"] - r["bic"].min())
    assert candidates.rank_candidates([2, 6], [1.0, 3.0], 2, 71, [peaks_of(2)[0], prom6], [peaks_of(2)[1], height6],
                                      fill=False)["best_keys"] == [2, 6]


def test_bayes_factors():
    bic = np.array([10.0, 4.0, 6.0])
    np.testing.assert_array_equal(candidates.norm_bayes_factors(bic, "bic"), np.exp(-0.5 * (bic - 4.0)))
    lml = np.array([-3.0, -1.0, -8.0])
    for crit in ("lml", "lml-bic"):
        np.testing.assert_array_equal(candidates.norm_bayes_factors(lml, crit), np.exp(lml + 1.0))
        assert candidates.bayes_factor(-3.0, -1.0, crit) == np.exp(-2.0)
    assert candidates.bayes_factor(10.0, 4.0) == np.exp(-3.0)
    assert candidates.bic(6, 71, -2.5) == 6 * np.log(71) + 5.0
    for f in (lambda: candidates.norm_bayes_factors(bic, "aic"), lambda: candidates.bayes_factor(1.0, 2.0, "aic")):
        with pytest.raises(ValueError, match="Invalid criterion aic"):
            f()
