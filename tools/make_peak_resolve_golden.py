"""Generate the per-peak resolution fixture under tests/golden/ (build container only: imports the reference through the shims of
oracle/refshim, like tools/make_peaks_golden.py):

  refrun_peak_resolve_golden71x91.npz   the reference's 71-frequency known-answer spectrum (tests/golden/ref_test_drt_fit_eis.npz)
                                        fitted three ways -- plain, nonneg=False and series_neg=True (sign=1; normalize=False for
                                        its find_peaks, which raises with normalize=True for such a fit) -- and for each fit, with
                                        get_tau_eval(10) as the find grid: the coefficients in data units, the unnormalised rows f
                                        and fxx, peak and trough indices, DRT.estimate_peak_coef, estimate_peak_drts and
                                        quantify_peaks on get_tau_eval(10) and get_tau_eval(20), split_r_p([1e-4, 1e-2]) in both
                                        forms and integrate_drt(1e-5, 1e-1).

(hybdrt/models/drt1d.py:3586-3620, 3949-4111; hybdrt/peaks.py:92-217)

A call the reference itself raises for is left out of the fixture and named on the console (``<tag>_missing`` lists them).
One does: split_r_p(resolve_peaks=True) on the series_neg fit (ValueError in get_drt_params, which is handed the reduced
coefficients a second time), so ``sneg_split_resolved`` is absent.

The fixture is only written when every trough decision keeps a margin of 1e-6 of max |f| (resp. max |f - fxx|): the sign test
of the two peaks, the local-minimum test, and the runner-up of each argmin / argmax.

    python tools/make_peak_resolve_golden.py
"""
import contextlib
import io
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "refshim"))
import oracle_boot  # noqa: E402,F401

from hybdrt import peaks as ref_peaks  # noqa: E402
from hybdrt.models import DRT  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CTOR = dict(fit_inductance=True, fit_capacitance=False, fit_dop=False, fit_ohmic=True)
FITS = {"plain": (dict(), dict()),
        "nn": (dict(nonneg=False), dict()),
        "sneg": (dict(series_neg=True), dict(normalize=False))}
SPLITS = [1e-4, 1e-2]
MARGIN = 1e-6


@contextlib.contextmanager
def quiet():
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter("ignore")
        yield


def runner_up(values, best, scale, what):
    """the best value of an argmin / argmax against the next one"""
    others = np.delete(values, best)
    if len(others):
        gap = np.min(np.abs(others - values[best]))
        assert gap > MARGIN * scale, (what, gap / scale)
        return gap / scale
    return np.inf


def trough_margins(tag, f, fxx, pk):
    """the smallest margin, relative to its scale, of the decisions find_troughs takes between the peaks pk; the branches taken"""
    sf, sm = np.max(np.abs(f)), np.max(np.abs(f - fxx))
    worst, branches = np.inf, []
    for s, e in zip(pk[:-1], pk[1:]):
        assert abs(f[s]) > MARGIN * sf and abs(f[e]) > MARGIN * sf, (tag, "sign of a peak", s, e)
        worst = min(worst, abs(f[s]) / sf, abs(f[e]) / sf)
        ls, rs = np.sign(f[s]), np.sign(f[e])
        if ls == rs:
            v = ls * f[s:e]
            edge = min(ls * f[s], ls * f[e])
            if len(v) > 1:
                # (when the left peak is the lower edge, v[0] is the edge itself: an identity, not a rounding matter)
                gap = np.min(np.abs(v[1:] - edge)) if ls * f[s] <= ls * f[e] else np.min(np.abs(v - edge))
                assert gap > MARGIN * sf, (tag, "local-minimum test", s, e, gap / sf)
                worst = min(worst, gap / sf)
            if np.min(v) < edge:
                branches.append("local_min")
                worst = min(worst, runner_up(v, int(np.argmin(v)), sf, (tag, "argmin f", s, e)))
            else:
                branches.append("f_minus_fxx")
                w = ls * -(f - fxx)[s:e]
                worst = min(worst, runner_up(w, int(np.argmax(w)), sm, (tag, "argmax f - fxx", s, e)))
        else:
            branches.append("sign_change")
            w = np.abs(f[s:e])
            worst = min(worst, runner_up(w, int(np.argmin(w)), sf, (tag, "argmin |f|", s, e)))
    return worst, branches


def make(freq, z):
    out = dict(freq=freq, z=z, tau_splits=np.array(SPLITS), integrate_lim=np.array([1e-5, 1e-1]))
    worst = np.inf
    for tag, (fit_kw, fkw) in FITS.items():
        missing = []

        def attempt(name, fn):
            try:
                with quiet():
                    out[f"{tag}_{name}"] = np.asarray(fn())
            except Exception as e:                       # noqa: BLE001 (the reference raises: the item is left out)
                missing.append(name)
                print(f"{tag}: {name} left out, the reference raises {type(e).__name__}: {e}")

        with quiet():
            drt = DRT(**CTOR)
            drt.fit_eis(freq, z, **fit_kw)
            tau10, tau20 = drt.get_tau_eval(10), drt.get_tau_eval(20)
            x_red = drt.get_drt_params(None, 1)
            f = drt.predict_drt(tau10, x=x_red, sign=1)
            fxx = drt.predict_drt(tau10, x=x_red, sign=1, order=2)
            _, _, pk, _ = drt.find_peaks(x=x_red, sign=1, return_info=True, **fkw)
            pk = np.asarray(pk)
            tr = np.asarray(ref_peaks.find_troughs(f, fxx, list(pk)), dtype=np.int64)
        out.update({f"{tag}_x": np.asarray(drt.fit_parameters["x"]), f"{tag}_x_red": np.asarray(x_red), f"{tag}_basis_tau": drt.basis_tau,
                    f"{tag}_tau_epsilon": np.float64(drt.tau_epsilon), f"{tag}_tau10": tau10, f"{tag}_tau20": tau20,
                    f"{tag}_f": f, f"{tag}_fxx": fxx, f"{tag}_peak_index": pk.astype(np.int64), f"{tag}_trough_index": tr,
                    f"{tag}_coefficient_scale": np.float64(drt.coefficient_scale), f"{tag}_nonneg": np.int64(bool(drt.fit_kwargs["nonneg"]))})
        attempt("x_peaks", lambda: drt.estimate_peak_coef(sign=1, **fkw))
        for k, tau in (("10", tau10), ("20", tau20)):
            attempt(f"peak_gammas{k}", lambda: drt.estimate_peak_drts(tau=tau, sign=1, find_peaks_kw=dict(fkw)))
            attempt(f"r_peaks{k}", lambda: drt.quantify_peaks(tau=tau, sign=1, find_peaks_kw=dict(fkw)))
        attempt("split", lambda: drt.split_r_p(list(SPLITS)))
        attempt("split_resolved", lambda: drt.split_r_p(list(SPLITS), resolve_peaks=True))
        attempt("integral", lambda: drt.integrate_drt(1e-5, 1e-1))
        with quiet():
            out[f"{tag}_f20"] = drt.predict_drt(tau20)
            out[f"{tag}_fxx20"] = drt.predict_drt(tau20, order=2)
        out[f"{tag}_missing"] = np.array(missing, dtype="U32")
        w, branches = trough_margins(tag, f, fxx, pk)
        worst = min(worst, w)
        print(tag, "peaks", pk.tolist(), "troughs", tr.tolist(), "branches", branches, "smallest margin %.2e" % w)
    print("smallest margin of all trough decisions: %.2e" % worst)
    np.savez_compressed(os.path.join(GOLDEN, "refrun_peak_resolve_golden71x91.npz"), **out)


if __name__ == "__main__":
    g = np.load(os.path.join(GOLDEN, "ref_test_drt_fit_eis.npz"))
    make(g["freq"], g["z"])
