"""CPU: hipdrt.models.pfrt, the numpy statement of csrc/pfrt.hip, against the reference's recorded run
(tools/make_pfrt_golden.py: DRT.pfrt_fit_eis plain and with nonneg=False on the 71-frequency known-answer spectrum).

The statement is fed the recorded rows (f, fxx and both variances BEFORE extend_var's clamp and the floor, so that both are
exercised), the recorded step likelihoods and factors, and must reproduce step_pfrt (the non-zero positions exactly), raw_pfrt
and predict_pfrt's output for four option sets.

The float bound, 1e-13 of the row's peak.  One unit roundoff is u = 1.1e-16.
  * A step probability is 1 - erfc(z) against the reference's 1 - 2 ndtr(-z sqrt 2): two special functions of a few u relative
    error each, whose values lie in [0, 1], so the difference is a few u ABSOLUTE; z itself (a quotient, a square root, a product)
    carries 3 u relative, which moves a probability by at most 0.49 * 3 u.  The smallest row peak here is above 0.1: < 1e-14.
  * The posterior weights: the exponent (log_post - max) * n_eff is below 40 in magnitude for every step that matters (a weight
    below exp(-40) adds less than u), so exp carries 40 u relative; the area and the sum of the weights are sums of 11 positive terms
    in another order than numpy's, 11 u relative each.
  * raw_pfrt: 11 positive terms, each a product (2 u) of the two above: below (40 + 22 + 11 + 4) u = 8.5e-15 relative.
  * The smoothed row: at most 111 positive terms exp(-t^4) raw_j in another order than the BLAS product's (111 u); a term matters
    only while exp(-t^4) > u, i.e. t^4 < 37, where the power (4 u relative) and the exponential carry 37 * 5 u: 3.3e-14.
  * Integration adds at most 111 positive terms once more (1.2e-14), normalisation one division.
Together below 6e-14 of the peak; the bound is 1e-13.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN

from hipdrt.models import pfrt

BOUND = 1e-13
FITS = ("plain", "nn")
OPTION_SETS = {"default": dict(), "raw": dict(smooth=False, normalize=False), "int": dict(integrate=True), "tau181": dict()}


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "refrun_pfrt_golden71x91.npz"))


def close(actual, desired, what):
    actual, desired = np.asarray(actual, dtype=float), np.asarray(desired, dtype=float)
    assert actual.shape == desired.shape, what
    err = float(np.max(np.abs(actual - desired))) / float(np.max(np.abs(desired)))
    print(f"{what}: {err:.2e} of the peak")
    assert err <= BOUND, (what, err)


def rows_result(g, tag, **kw):
    lt = np.log(g[f"{tag}_tau_pfrt"])
    ext = g[f"{tag}_ext"]
    return pfrt.predict_pfrt_rows(g[f"{tag}_factors"], g[f"{tag}_step_llh"], g[f"{tag}_f"], g[f"{tag}_fxx"], g[f"{tag}_var_f_raw"],
                                  g[f"{tag}_var_fxx_raw"], lt, search=int(g[f"{tag}_search"]), ext_left=int(ext[0]),
                                  ext_right=int(ext[1]), **kw)


@pytest.mark.parametrize("tag", FITS)
def test_recorded_variances_are_the_clamped_and_floored_raw_ones(golden, tag):
    from hipdrt.models import peaks
    ext = golden[f"{tag}_ext"]
    for name in ("var_f", "var_fxx"):
        for raw, rec in zip(golden[f"{tag}_{name}_raw"], golden[f"{tag}_{name}"]):
            np.testing.assert_array_equal(peaks.extend_var(raw, int(ext[0]), int(ext[1]), 1e-5), rec)
    assert (golden[f"{tag}_var_f_raw"] < 1e-5).any()          # the floor acts on the order-0 variance too


@pytest.mark.parametrize("tag", FITS)
def test_steps_and_raw_pfrt_against_the_reference(golden, tag):
    out = rows_result(golden, tag)
    ref = golden[f"{tag}_step_pfrt"]
    np.testing.assert_array_equal(out["step_pfrt"] != 0, ref != 0)
    counts = {"plain": [2, 2, 3, 4, 4, 4, 4, 5, 5, 6, 7], "nn": [2, 2, 3, 3, 3, 4, 4, 5, 5, 6, 7]}[tag]
    assert np.count_nonzero(ref, axis=1).tolist() == counts
    for i in range(len(ref)):
        close(out["step_pfrt"][i], ref[i], f"{tag} step_pfrt[{i}]")
    close(out["raw_pfrt"], golden[f"{tag}_raw_pfrt"], f"{tag} raw_pfrt")


@pytest.mark.parametrize("name", list(OPTION_SETS))
@pytest.mark.parametrize("tag", FITS)
def test_predict_pfrt_option_sets_against_the_reference(golden, tag, name):
    kw = dict(OPTION_SETS[name])
    if name == "tau181":
        kw["ln_tau_out"] = np.log(golden["tau181"])
    out = rows_result(golden, tag, **kw)["pfrt"]
    ref = golden[f"{tag}_pfrt_{name}"]
    if name == "int":
        np.testing.assert_array_equal(out != 0, ref != 0)
    if name == "default":
        assert int(np.argmax(ref)) == 38 and int(np.argmax(out)) == 38
    close(out, ref, f"{tag} predict_pfrt[{name}]")


def test_a_range_that_starts_at_index_zero_integrates_to_nothing():
    pf = np.array([0.5, 0.25, 0.0, 0.0, 0.25, 0.75, 0.5, 0.0, 1.0])
    starts, ends = pfrt.get_peak_ranges(pf, 0.125)
    assert starts.tolist() == [0, 4, 8] and ends.tolist() == [2, 7, 9]
    idx, area = pfrt.integrate_peaks(pf, 0.125)
    assert idx.tolist() == [0, 5, 8]
    # [0, 2): pf[-1:3] is empty; [4, 7): trapezoid of pf[3:8]; [8, 9): pf[7:10] = (0, 1)
    assert area.tolist() == [0.0, 0.125 + 0.5 + 0.625 + 0.25, 0.5]
    out = pfrt.finish(pf, np.arange(9.0), smooth_on=False, integrate=True, integrate_threshold=0.125, normalize=False)
    assert out.tolist() == [0.0, 0, 0, 0, 0, 1.5, 0, 0, 0.5]
    # ... also when the range reaches the end of the row: pf[-1:n + 1] is one sample
    idx, area = pfrt.integrate_peaks(np.ones(4), 0.5)
    assert idx.tolist() == [0] and area.tolist() == [0.0]


def test_a_single_factor_is_divided_by_its_own_value():
    post = pfrt.step_posterior([0.7], [-123.0], n_eff_factor=0.5)
    assert post.tolist() == [1.0]
    step = np.array([[0.0, 0.5, 0.0, 0.25]])
    np.testing.assert_array_equal(pfrt.combine(post, step), step[0])
    # two factors: exp(log-posterior difference * n_eff) over the trapezoid
    lf = np.log([0.5, 2.0])
    lp = -0.5 * (np.log(2 * np.pi) + 2 * np.log(0.5) + ((lf + 4) / 0.5) ** 2) + np.array([-10.0, -12.0])
    e = np.exp((lp - lp.max()) * 0.5)
    np.testing.assert_allclose(pfrt.step_posterior([0.5, 2.0], [-10.0, -12.0]), e / ((lf[1] - lf[0]) * (e[0] + e[1]) / 2), rtol=1e-15)


def test_an_all_zero_row_normalises_to_nan_as_upstream():
    n = 12
    rows = np.zeros((2, n))            # flat curvature: no peak in any step
    out = pfrt.predict_pfrt_rows([0.5, 2.0], [-10.0, -12.0], rows, rows, rows + 1.0, rows + 1.0, np.linspace(-3, 3, n))
    assert not out["step_pfrt"].any() and not out["raw_pfrt"].any()
    assert np.isnan(out["pfrt"]).all()
    out = pfrt.predict_pfrt_rows([0.5, 2.0], [-10.0, -12.0], rows, rows, rows + 1.0, rows + 1.0, np.linspace(-3, 3, n),
                                 integrate=True, normalize=False)
    assert not out["pfrt"].any()


def test_smooth_matrix_is_the_gaussian_similarity_function():
    lo, lp = np.array([0.0, 0.1]), np.array([0.0, 0.2, 1.0])
    m = pfrt.smooth_matrix(lo, lp)
    assert m.shape == (2, 3) and m[0, 0] == 1.0
    np.testing.assert_allclose(m[1, 1], np.exp(-(5 * 0.1) ** 4), rtol=1e-15)
    np.testing.assert_allclose(pfrt.smooth([0.0, 2.0, 0.5], lo, lp), m @ np.array([0.0, 2.0, 0.5]), rtol=1e-15)
