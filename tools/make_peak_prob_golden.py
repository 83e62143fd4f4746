"""Generate the peak-probability fixture under tests/golden/ and the bounds table of its CPU test (build container only: imports
the reference through the shims of oracle/refshim, like tools/make_peaks_golden.py):

  refrun_peak_prob_golden71x91.npz   the reference's 71-frequency known-answer spectrum (tests/golden/ref_test_drt_fit_eis.npz)
                                     fitted three ways -- plain, nonneg=False and series_neg=True -- and for each fit, on
                                     get_tau_eval(10): f, fx, fxx (predict_drt at its defaults), the three sigma rows with
                                     extend_var=True (no floor), the floors drt1d.py:3677-3678 gives them, the filtered sigma rows
                                     of surface.py:272-291, pp and tp of DRT.predict_peak_trough_probs for bayes_cov True and
                                     False, DRT.find_peaks_byprob with return_info for (height, prominence) = (0.5, 0.25) and
                                     (0.1, 0.1) and for the two ranges (1e-5, 1e-3), (1e-3, 1e-1), and coefficient_scale.
  tests/peak_prob_bounds.json        label -> [measured, bound]: how far hipdrt/models/peaks.py, fed the recorded rows, lies from
                                     the recorded results, and 30 x that rounded up to 1 / 2 / 5 x 10^k (never below 1e-12) --
                                     the margin is for scipy's running-sum uniform_filter and ndtr against a direct sum and
                                     math.erfc.

(hybdrt/models/drt1d.py:3655-3750 predict_peak_trough_probs / predict_peak_prob / find_peaks_byprob, 3063-3151
estimate_distribution_cov; hybdrt/mapping/surface.py:265-350; hybdrt/filters/_filters.py:29-40, 149-175; hybdrt/peaks.py:423-441)

The fixture is only written when every local maximum of every recorded prob row keeps 1 % from each threshold it is tested
against, and the winner of every range beats the runner-up inside its window by 1 %: the tests compare indices exactly.  The
runner-up of a range is the next highest local maximum of the masked row (a window edge that falls off to the zeros outside
counts as one): the samples beside the winner lie on its own flank, at 10 points per decade within 1 % of it.  Of those, and
of every other sample in the window, the winner must keep 1e-5 of its height: two rows that each lie within 1e-6 of the
reference's (the tolerance of the device's probabilities) order two samples alike once these are 2e-6 apart.

    python tools/make_peak_prob_golden.py
"""
import contextlib
import io
import json
import math
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "refshim"))
import oracle_boot  # noqa: E402,F401

from hybdrt.filters import std_filter  # noqa: E402
from hybdrt.models import DRT  # noqa: E402

from hipdrt.models import peaks  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CTOR = dict(fit_inductance=True, fit_capacitance=False, fit_dop=False, fit_ohmic=True)
FITS = {"plain": dict(), "nn": dict(nonneg=False), "sneg": dict(series_neg=True)}
THRESHOLDS = ((0.5, 0.25), (0.1, 0.1))
RANGES = [(1e-5, 1e-3), (1e-3, 1e-1)]
MARGIN = 0.01


@contextlib.contextmanager
def quiet():
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter("ignore")
        yield


def thr_key(height, prominence):
    return f"h{height:g}_p{prominence:g}"


def check_margins(tag, tau, prob):
    _, info = peaks.find_peaks_1d(prob)
    for height, prominence in THRESHOLDS:
        # (scipy drops what fails the height before it looks at a prominence: those are never tested against the second threshold)
        high = info["peak_heights"] >= height
        for values, thresh in ((info["peak_heights"], height), (info["prominences"][high], prominence)):
            assert (np.abs(values - thresh) > MARGIN * thresh).all(), (tag, values, thresh)
    for t0, t1 in RANGES:
        g = prob.copy()
        g[(tau < t0) | (tau > t1)] = 0
        win = int(np.argmax(g))
        assert g[win] > 0, (tag, t0, t1)
        maxima = [i for i in peaks.find_peaks_1d(g)[0] if i != win] + [i for i in (0, len(g) - 1) if i != win and g[i] > 0]
        assert all(g[win] - g[i] > MARGIN * g[win] for i in maxima), (tag, t0, t1, g[win], g[maxima])
        assert np.all(g[win] - np.delete(g, win) > 1e-5 * g[win]), (tag, t0, t1, np.sort(g)[::-1][:3])


def make(freq, z):
    out = dict(freq=freq, z=z, ranges=np.array(RANGES), thresholds=np.array(THRESHOLDS))
    for tag, fit_kw in FITS.items():
        with quiet():
            drt = DRT(**CTOR)
            drt.fit_eis(freq, z, **fit_kw)
            tau = drt.get_tau_eval(10)
            rows, sig = [], []
            for order in (0, 1, 2):
                rows.append(drt.predict_drt(tau, order=order))
                sig.append(np.diag(drt.estimate_distribution_cov(tau, order=order, extend_var=True)) ** 0.5)
            floors = [np.median(s) - 1.5 * (np.percentile(s, 75) - np.percentile(s, 25)) for s in sig]
            filt = [std_filter(r, size=5, mask=np.ones(len(r))) + 0.1 * np.std(r) for r in rows]
            assert "tau" not in out or np.array_equal(out["tau"], tau)        # (one basis grid: one evaluation grid)
            out["tau"] = tau
            out.update({f"{tag}_rows": np.array(rows), f"{tag}_sigma": np.array(sig),
                        f"{tag}_sigma_floors": np.array(floors), f"{tag}_filtered_sigma": np.array(filt),
                        f"{tag}_coefficient_scale": np.float64(drt.coefficient_scale)})
            for bc in (1, 0):
                pp, tp = drt.predict_peak_trough_probs(tau, bayes_cov=bool(bc))
                prob = drt.predict_peak_prob(tau, bayes_cov=bool(bc))
                assert np.array_equal(prob, pp * (1 - tp))
                out[f"{tag}_pp_b{bc}"], out[f"{tag}_tp_b{bc}"] = pp, tp
                check_margins(f"{tag} bayes_cov={bc}", tau, prob)
                for height, prominence in THRESHOLDS:
                    _, _, idx, info = drt.find_peaks_byprob(tau, height=height, prominence=prominence, bayes_cov=bool(bc),
                                                            return_info=True)
                    key = f"{tag}_b{bc}_{thr_key(height, prominence)}"
                    out[f"{key}_idx"] = np.asarray(idx)
                    for k, v in info.items():
                        out[f"{key}_{k}"] = np.asarray(v)
                ptau, _, idx, info = drt.find_peaks_byprob(tau, peak_tau_ranges=RANGES, bayes_cov=bool(bc), return_info=True)
                assert info == {}
                out[f"{tag}_b{bc}_ranges_idx"] = np.asarray(idx)
                _, pinfo = peaks.find_peaks_1d(prob)
                print(tag, "bayes_cov", bc, "maxima heights", np.round(pinfo["peak_heights"], 4).tolist(), "prominences",
                      np.round(pinfo["prominences"], 4).tolist(), "range peaks", ptau.tolist(),
                      "clamped by the floor", [int(np.sum(s < fl)) for s, fl in zip(sig, floors)], file=sys.stderr)
    np.savez_compressed(os.path.join(GOLDEN, "refrun_peak_prob_golden71x91.npz"), **out)
    return out


def deviation(actual, desired, relative=False):
    actual, desired = np.asarray(actual, dtype=float), np.asarray(desired, dtype=float)
    err = float(np.max(np.abs(actual - desired)))
    return err / float(np.max(np.abs(desired))) if relative else err


def bound_of(measured):
    """30 x measured, rounded up to 1 / 2 / 5 x 10^k, never below 1e-12"""
    v = max(30.0 * measured, 1e-12)
    k = math.floor(math.log10(v))
    for m in (1, 2, 5, 10):
        if m * 10.0 ** k >= v * (1 - 1e-12):
            return float(f"{m * 10.0 ** k:.0e}")


def measure(out):
    """the deviations of the numpy statement from the recorded results; probabilities absolute, sigma as a fraction of its peak"""
    table = {}
    for tag in FITS:
        rows, sig = out[f"{tag}_rows"], out[f"{tag}_sigma"]
        for k, name in enumerate(("f", "fx", "fxx")):
            table[f"{tag}:sigma_floor_{name}"] = deviation(peaks.sigma_floor_value(sig[k]), out[f"{tag}_sigma_floors"][k], True)
            table[f"{tag}:filtered_sigma_{name}"] = deviation(peaks.filtered_sigma(rows[k]), out[f"{tag}_filtered_sigma"][k], True)
        for bc in (1, 0):
            var = sig ** 2 if bc else (None, None, None)
            pp, tp, _ = peaks.peak_trough_probs_rows(*rows, *var)
            ref_pp, ref_tp = out[f"{tag}_pp_b{bc}"], out[f"{tag}_tp_b{bc}"]
            table[f"{tag}:pp_b{bc}"] = deviation(pp, ref_pp)
            table[f"{tag}:tp_b{bc}"] = deviation(tp, ref_tp)
            table[f"{tag}:prob_b{bc}"] = deviation(peaks.peak_prob_of(pp, tp), ref_pp * (1 - ref_tp))
    return {k: [float(f"{v:.2e}"), bound_of(v)] for k, v in sorted(table.items())}


if __name__ == "__main__":
    g = np.load(os.path.join(GOLDEN, "ref_test_drt_fit_eis.npz"))
    table = measure(make(g["freq"], g["z"]))
    with open(os.path.join(ROOT, "tests", "peak_prob_bounds.json"), "w") as f:
        json.dump(table, f, indent=1)
        f.write("\n")
    print(json.dumps(table, indent=1))
