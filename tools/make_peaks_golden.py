"""Generate the peak-finding fixture under tests/golden/ (build container only: imports the reference through the shims of
oracle/refshim, like tools/make_predict_golden.py):

  refrun_peaks_golden71x91.npz   the reference's 71-frequency known-answer spectrum (tests/golden/ref_test_drt_fit_eis.npz) fitted
                                 three ways -- plain, nonneg=False (two-pass search) and series_neg=True (sign=0, normalize=False:
                                 upstream's find_peaks(normalize=True) raises for such a fit) -- and for each fit, on
                                 get_tau_eval(10): f, fxx, the two sigma rows with extend_var=True (no floor), DRT.find_peaks with
                                 return_info for 'thresh', 'prob' and 'prob' with num_peaks=1, curvature.peak_prob_1d times sign(f)
                                 and DRTMD.predict_curv_prob's formula on those rows.

(hybdrt/models/drt1d.py:3753-3947 find_peaks, 3063-3151 estimate_distribution_cov; hybdrt/mapping/curvature.py:12-58;
hybdrt/mapping/drtmd.py:1097-1104)

The fixture is only written when every recorded peak, and every candidate the thresholds reject, keeps the margin the tests'
exact comparisons rely on: 1 % from its height, prominence and probability threshold, and |f| above 1e-6 of max |f| at the
candidates of a two-pass search.

    python tools/make_peaks_golden.py
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

from hybdrt.mapping import curvature  # noqa: E402
from hybdrt.models import DRT  # noqa: E402
from hybdrt.utils import stats  # noqa: E402

from hipdrt.models import peaks  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CTOR = dict(fit_inductance=True, fit_capacitance=False, fit_dop=False, fit_ohmic=True)
FITS = {"plain": (dict(), dict(sign=1, normalize=True)),
        "nn": (dict(nonneg=False), dict(sign=1, normalize=True)),
        "sneg": (dict(series_neg=True), dict(sign=0, normalize=False))}
METHODS = {"thresh": dict(method="thresh"), "prob": dict(method="prob"), "prob1": dict(method="prob", num_peaks=1)}
MARGIN = 0.01


@contextlib.contextmanager
def quiet():
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter("ignore")
        yield


def off_threshold(values, thresh, what, scale):
    values = np.asarray(values, dtype=float)
    gap = np.abs(values - thresh)
    assert (gap > MARGIN * abs(thresh)).all() and (gap > 1e-9 * scale).all(), (what, values, thresh)


def check_margins(tag, f, fxx, search, nonneg, out):
    """every candidate (a local maximum of a pass) against the thresholds the reference used"""
    passes = (search,) if search != 0 else (-1, 1)
    scale = np.max(np.abs(fxx))
    for m, kw in METHODS.items():
        prom, height = peaks.auto_thresholds(fxx, kw["method"])
        for s in passes:
            idx, info = peaks.find_peaks_1d(-s * fxx)
            off_threshold(info["peak_heights"], height, f"{tag} {m} height", scale)
            off_threshold(info["prominences"], prom, f"{tag} {m} prominence", scale)
            if search == 0:
                assert (np.abs(f[idx]) > 1e-6 * np.max(np.abs(f))).all(), (tag, m, "f at a candidate")
        if kw["method"] == "prob":
            pr = np.sort(out[f"{tag}_{m}_probs"])[::-1]
            if "num_peaks" in kw:
                assert len(pr) < 2 or pr[0] - pr[1] > MARGIN * pr[0], (tag, m, pr)
            else:
                off_threshold(pr, 0.25, f"{tag} {m} probability", 1.0)


def make(freq, z):
    out = dict(freq=freq, z=z)
    for tag, (fit_kw, pk_kw) in FITS.items():
        with quiet():
            drt = DRT(**CTOR)
            drt.fit_eis(freq, z, **fit_kw)
            tau = drt.get_tau_eval(10)
            nonneg = bool(drt.fit_kwargs["nonneg"])
            rows = {}
            for name, order in (("f", 0), ("fxx", 2)):
                rows[name] = drt.predict_drt(tau=tau, order=order, **pk_kw)
                rows[f"sigma_{name}"] = np.diag(drt.estimate_distribution_cov(tau, order=order, extend_var=True, **pk_kw)) ** 0.5
            for m, kw in METHODS.items():
                _, _, idx, info = drt.find_peaks(tau=tau, return_info=True, **pk_kw, **kw)
                out[f"{tag}_{m}_idx"] = np.asarray(idx)
                for k, v in info.items():
                    out[f"{tag}_{m}_{k}"] = np.asarray(v)
            f, fxx, sf, sxx = rows["f"], rows["fxx"], rows["sigma_f"], rows["sigma_fxx"]
            pp = curvature.peak_prob_1d([f, fxx, sf, sxx], nonneg, pk_kw["sign"], 1e-3, 5e-3) * np.sign(f)
            f_prob = 1 - stats.cdf_normal(0, -np.sign(fxx) * f, sf)
            c_prob = 1 - stats.cdf_normal(0, -np.sign(f) * fxx, sxx)
            cp = np.minimum(2 * np.maximum(f_prob - 0.5, 0), 2 * np.maximum(c_prob - 0.5, 0)) * np.sign(f)
        out.update({f"{tag}_tau": tau, f"{tag}_nonneg": np.int64(nonneg), f"{tag}_peak_prob": pp, f"{tag}_curv_prob": cp,
                    f"{tag}_coefficient_scale": np.float64(drt.coefficient_scale)})
        out.update({f"{tag}_{k}": v for k, v in rows.items()})
        search = pk_kw["sign"] if (nonneg and pk_kw["sign"] != 0) else 0
        check_margins(tag, f, fxx, search, nonneg, out)
        print(tag, "search", search, {m: out[f"{tag}_{m}_idx"].tolist() for m in METHODS},
              "probs", np.round(out[f"{tag}_prob_probs"], 3).tolist())
    np.savez_compressed(os.path.join(GOLDEN, "refrun_peaks_golden71x91.npz"), **out)


if __name__ == "__main__":
    g = np.load(os.path.join(GOLDEN, "ref_test_drt_fit_eis.npz"))
    make(g["freq"], g["z"])
