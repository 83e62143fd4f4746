"""Generate the candidate-model fixtures under tests/golden/ (build container only: imports the reference through the shims of
oracle/refshim, like tools/make_pfrt_golden.py) by calling the reference's own DRT.generate_candidates
(hybdrt/models/drt1d.py:1632-1821) with its defaults:

  refrun_generate_candidates_golden71x91.npz       the 71-frequency known-answer spectrum (tests/golden/ref_test_drt_fit_eis.npz)
  refrun_generate_candidates_golden71x91_neg.npz   the same spectrum with nonneg=False (two-pass peak search)
  refrun_generate_candidates_hybrid_s0.npz         fit_hybrid on synth.hybrid_measurement(seed=0), a prepared-plan fit

Each holds: x, llh, num_peaks and bic of every candidate; peak_tau / peak_heights / prominences, NaN padded; the two tables
(candidate_df, best_candidate_df) as arrays with their column names; the keys of the filled best_candidate_dict with every
entry's peak_tau, llh and bic; the normalised Bayes factors and the best candidate id; the find grid, the number of special
parameters and of independent data; evaluate_bic(), evaluate_llh() and the peak count of the fit itself, taken before the
restarts; how many candidates the base history, the s_0 pass and the weight pass gave; and rm, rv and vmm of qphb_params as
generate_candidates read them, so that the likelihoods can be re-formed without a device.

A fixture is only written when no candidate's peak count is decided by a margin below 1e-9 relative: every local maximum of a
pass keeps that distance from the height threshold (relative to max |fxx|) and from the prominence threshold (relative to it),
every local maximum with at least half the prominence threshold differs from both neighbouring samples by that much of max
|fxx|, and in a two-pass search |f| there is at least that much of max |f|.  Were the known-answer spectrum to violate this, the
plain and nn cases fall back to a synthetic 2-ZARC spectrum (hipdrt.synth.zarc2_batch), the seed raised until the margins hold
and recorded in the fixture (seed = -1: the known-answer spectrum).

    python tools/make_candidates_golden.py
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

from hybdrt.models import DRT  # noqa: E402

from hipdrt import synth  # noqa: E402
from hipdrt.models import peaks  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CTOR = dict(fit_inductance=True, fit_capacitance=False, fit_dop=False, fit_ohmic=True)
MARGIN = 1e-9


@contextlib.contextmanager
def quiet():
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter("ignore")
        yield


def margin_of(drt, x_raw, tau):
    """the smallest relative margin by which find_peaks(x=..., method='thresh') decides the peak count of one candidate"""
    x_drt = drt.extract_qphb_parameters(x_raw)["x"]
    fxx = drt.predict_drt(tau=tau, x=x_drt, order=2, sign=1, normalize=True)
    f = drt.predict_drt(tau=tau, x=x_drt, order=0, sign=1, normalize=True)
    prominence = 0.05 * np.std(fxx[~np.isinf(fxx)]) + 5e-3
    top, ftop = float(np.max(np.abs(fxx))), float(np.max(np.abs(f)))
    two = not drt.fit_kwargs["nonneg"]
    gap = np.inf
    for s in ((-1, 1) if two else (1,)):
        v = -s * fxx
        idx, info = peaks.find_peaks_1d(v)
        if not len(idx):
            continue
        gap = min(gap, float(np.min(np.abs(info["peak_heights"]))) / top,
                  float(np.min(np.abs(info["prominences"] - prominence))) / prominence)
        big = idx[info["prominences"] >= 0.5 * prominence]
        if len(big):
            gap = min(gap, float(np.min(np.abs(v[big] - v[big - 1]))) / top, float(np.min(np.abs(v[big] - v[big + 1]))) / top)
            if two:
                gap = min(gap, float(np.min(np.abs(f[big]))) / ftop)
    return gap


def pad(rows):
    width = max([len(r) for r in rows] + [1])
    out = np.full((len(rows), width), np.nan)
    for i, r in enumerate(rows):
        out[i, :len(r)] = r
    return out


def run(fit):
    """fit(drt) fits; -> (fixture dict, smallest margin)"""
    with quiet():
        drt = DRT(**CTOR)
        fit(drt)
        base_len = len(drt.qphb_history)
        # the reference's evaluate_bic of the fit itself (drt1d.py:4498-4511: llh under the fit's own est_weights), before the
        # restarts touch qphb_params
        fit_bic, fit_llh, fit_num_peaks = drt.evaluate_bic(), drt.evaluate_llh(), len(drt.find_peaks())
        cd = drt.generate_candidates()
        tau = drt.get_tau_eval(10)
        gap = min(margin_of(drt, x, tau) for x in cd["x"])
        nbf = drt.evaluate_norm_bayes_factors("continuous")
        best_id = drt.get_best_candidate_id("continuous")
    best = drt.best_candidate_dict
    keys = np.array(sorted(best), dtype=np.int64)
    n_up = sum(1 for h in cd["hypers"] if "s_0" in h and "weight_factor" not in h)
    out = dict(
        x=np.asarray(cd["x"]), llh=np.asarray(cd["llh"], dtype=float), num_peaks=np.asarray(cd["num_peaks"], dtype=np.int64),
        bic=np.asarray(cd["bic"], dtype=float), peak_tau=pad(cd["peak_tau"]),
        peak_heights=pad([i["peak_heights"] for i in cd["peak_info"]]), prominences=pad([i["prominences"] for i in cd["peak_info"]]),
        candidate_df=drt.candidate_df.values, candidate_df_columns=np.array(list(drt.candidate_df.columns)),
        best_candidate_df=drt.best_candidate_df.values, best_candidate_df_columns=np.array(list(drt.best_candidate_df.columns)),
        best_keys=keys, best_peak_tau=pad([best[k]["peak_tau"] for k in keys]),
        best_llh=np.array([best[k]["llh"] for k in keys], dtype=float), best_bic=np.array([best[k]["bic"] for k in keys], dtype=float),
        norm_bayes_factors=np.asarray(nbf, dtype=float), best_id=np.float64(best_id), tau=tau,
        num_special=np.int64(drt.get_qp_mat_offset()), num_independent_data=np.int64(drt.num_independent_data),
        counts=np.array([base_len, n_up, len(cd["x"]) - base_len - n_up], dtype=np.int64), margin=np.float64(gap),
        coefficient_scale=np.float64(drt.coefficient_scale),
        evaluate_bic=np.float64(fit_bic), evaluate_llh=np.float64(fit_llh), fit_num_peaks=np.int64(fit_num_peaks),
        # what the candidates were scored with (the matrix as the restarts left it: a vz_offset column is rewritten in place)
        rm=np.asarray(drt.qphb_params["rm"]), rv=np.asarray(drt.qphb_params["rv"]), vmm=np.asarray(drt.qphb_params["vmm"]))
    return out, gap


def save(name, out):
    path = os.path.join(GOLDEN, f"refrun_generate_candidates_{name}.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    print(name, os.path.getsize(path), "bytes; candidates", out["counts"].tolist(), "peaks", out["num_peaks"].tolist(),
          "best keys", out["best_keys"].tolist(), "margin %.2g" % float(out["margin"]), "seed", int(out["seed"]))


def make_eis(name, fit_kw):
    g = np.load(os.path.join(GOLDEN, "ref_test_drt_fit_eis.npz"))
    freq = np.asarray(g["freq"], dtype=float)
    seed, z = -1, np.asarray(g["z"], dtype=complex)
    while True:
        out, gap = run(lambda drt: drt.fit_eis(freq, z, **fit_kw))
        if gap >= MARGIN:
            break
        seed += 1
        assert seed < 20, (name, "no seed below 20 keeps every margin above 1e-9", gap)
        z = synth.zarc2_batch(freq, 1, first_seed=seed)[0]
    save(name, dict(out, freq=freq, z=z, seed=np.int64(seed)))


def make_hybrid():
    meas = synth.hybrid_measurement(seed=0)
    out, gap = run(lambda drt: drt.fit_hybrid(*meas))
    assert gap >= MARGIN, ("hybrid_s0", "a peak count is decided by a margin below 1e-9", gap)
    save("hybrid_s0", dict(out, seed=np.int64(0)))


if __name__ == "__main__":
    make_eis("golden71x91", dict())
    make_eis("golden71x91_neg", dict(nonneg=False))
    make_hybrid()
