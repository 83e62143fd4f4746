"""Time the peak-probability methods on the device for a fitted batch, beside find_peaks_batch(method='prob') on the same batch.

    python tools/bench_peak_prob.py [--spectra 1024] [--nf 256] [--ntau 512] [--repeat 7] [--out profiles/peak_prob_bench.json]

device    predict_peak_prob_batch and find_peaks_byprob_batch (thresholds, and two ranges) for bayes_cov True and False, and
          find_peaks_batch(method='prob'), all on the resident batch and the 10-points-per-decade grid: kernel time by HIP events
          around the launches of one call (hipdrt_debug_last_predict_ms: [0] the mean rows, [1] all launches -- what follows the
          rows is the factorisation of every P fed three (find_peaks: two) orders' rows, then the one-workgroup-per-spectrum
          kernel), and the wall time of the whole call with its download.  The calls alternate inside every repeat, so that a
          drift of the machine touches all of them alike.
profile   --profile runs each call three times and nothing else: the process rocprofv3 --kernel-trace --stats wraps to give
          peak_trough_prob_kernel's share of the call."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hipdrt import synth  # noqa: E402
from hipdrt.models import DRT  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spectra", type=int, default=1024)
    ap.add_argument("--nf", type=int, default=256)
    ap.add_argument("--ntau", type=int, default=512)
    ap.add_argument("--repeat", type=int, default=7)
    ap.add_argument("--profile", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    freq = np.logspace(6, -1, a.nf)
    tau = np.logspace(-8, 2, a.ntau)
    z = synth.zarc2_batch(freq, a.spectra)
    drt = DRT(fixed_basis_tau=tau, warn=False)
    t0 = time.perf_counter()
    drt.fit_eis_batch(freq, z)
    fit_wall = time.perf_counter() - t0
    ctx = drt._plan.ctx
    tau_eval = drt.get_tau_eval(10)
    ranges = [(1e-5, 1e-3), (1e-3, 1e-1)]
    calls = {
        "find_peaks_prob": lambda: drt.find_peaks_batch(tau=tau_eval, method="prob"),
        "predict_peak_prob": lambda: drt.predict_peak_prob_batch(tau=tau_eval),
        "find_peaks_byprob": lambda: drt.find_peaks_byprob_batch(tau=tau_eval, height=0.5, prominence=0.25),
        "find_peaks_byprob_ranges": lambda: drt.find_peaks_byprob_batch(tau=tau_eval, peak_tau_ranges=ranges),
        "predict_peak_prob_filtered": lambda: drt.predict_peak_prob_batch(tau=tau_eval, bayes_cov=False),
        "find_peaks_byprob_filtered": lambda: drt.find_peaks_byprob_batch(tau=tau_eval, height=0.5, prominence=0.25, bayes_cov=False),
    }
    if a.profile:
        for _ in range(3):
            for call in calls.values():
                call()
        return
    ms = {k: [] for k in calls}
    wall = {k: [] for k in calls}
    out = {}
    for r in range(a.repeat + 1):                       # (the first round warms every shape up and is left out)
        for k, call in calls.items():
            t0 = time.perf_counter()
            out[k] = call()
            wall[k].append((time.perf_counter() - t0) * 1e3)
            ms[k].append(ctx.debug_last_predict_ms())
    res = {}
    for k in calls:
        rows, total = np.array([m[0] for m in ms[k][1:]]), np.array([m[1] for m in ms[k][1:]])
        res[k] = {"kernel_ms_first": ms[k][0][1], "kernel_ms_min": float(total.min()), "kernel_ms_median": float(np.median(total)),
                  "kernel_ms_max": float(total.max()), "mean_rows_ms_min": float(rows.min()),
                  "after_the_rows_ms_min": float((total - rows).min()), "call_wall_ms_median": float(np.median(wall[k][1:]))}
    base = res["find_peaks_prob"]
    doc = {"spectra": a.spectra, "nf": a.nf, "ntau": a.ntau, "n": drt._plan.n, "neval": len(tau_eval), "fit_wall_s": fit_wall,
           "device": res,
           "kernel_time_over_find_peaks_prob": {k: res[k]["kernel_ms_median"] / base["kernel_ms_median"] for k in calls},
           "whole_call_over_find_peaks_prob": {k: res[k]["call_wall_ms_median"] / base["call_wall_ms_median"] for k in calls},
           "peaks_mean": {k: float(np.mean([len(p) for p in out[k]])) for k in calls if k.startswith("find")},
           "finite_prob_rows": int(np.isfinite(out["predict_peak_prob"]).all(axis=1).sum())}
    text = json.dumps(doc, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
