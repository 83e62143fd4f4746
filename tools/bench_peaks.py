"""Time peak finding on the device for a fitted batch against the host route it replaces.

    python tools/bench_peaks.py [--spectra 10000] [--nf 256] [--ntau 512] [--repeat 5] [--out profiles/peaks_bench.json]

device    find_peaks_batch for 'thresh', 'prob' and the map probabilities (peak_prob_batch) on the 10-points-per-decade grid:
          kernel time by HIP events around the launches of one call (hipdrt_debug_last_predict_ms: [0] the mean rows, [1] all
          launches -- for 'thresh' the difference is peaks_kernel alone, for the others the factorisation of every P and
          peaks_kernel), and the wall time of the whole call with its download and the per-spectrum lists built on the host,
          without and with return_info
host      what the code before these methods forced for the same result: predict_drt_batch(order=2, normalize=True), then a
          Python loop of scipy.signal.find_peaks over the rows; for 'prob' also sigma backed out of predict_drt_ci_batch's band
          (the only way that route had to it), the clamp and the floor in numpy, and the probabilities with scipy's erfc
check     the two routes' kept peaks are compared; spectra that differ are counted (a peak on a threshold may fall either way)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hipdrt import synth  # noqa: E402
from hipdrt.models import DRT, peaks, predict  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spectra", type=int, default=10000)
    ap.add_argument("--nf", type=int, default=256)
    ap.add_argument("--ntau", type=int, default=512)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    from scipy import signal, special

    freq = np.logspace(6, -1, a.nf)
    tau = np.logspace(-8, 2, a.ntau)
    z = synth.zarc2_batch(freq, a.spectra)
    drt = DRT(fixed_basis_tau=tau, warn=False)
    t0 = time.perf_counter()
    drt.fit_eis_batch(freq, z)
    fit_wall = time.perf_counter() - t0
    ctx = drt._plan.ctx
    tau_eval = drt.get_tau_eval(10)
    B = a.spectra

    def timed(call, repeat=a.repeat):
        ms, wall = [], []
        for _ in range(repeat + 1):
            t0 = time.perf_counter()
            out = call()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(ctx.debug_last_predict_ms())
        rows, total = np.array([m[0] for m in ms[1:]]), np.array([m[1] for m in ms[1:]])
        return out, {"kernel_ms_first": ms[0][1], "kernel_ms_min": float(total.min()), "kernel_ms_median": float(np.median(total)),
                     "mean_rows_ms_min": float(rows.min()), "after_the_rows_ms_min": float((total - rows).min()),
                     "call_wall_ms_median": float(np.median(wall[1:]))}

    _, t_pred = timed(lambda: drt.predict_drt_batch(tau=tau_eval, order=2, normalize=True))
    dev, t_dev = {}, {}
    # timed as a user calls it (the peaks' tau: only the kept mask comes down), and once more with return_info (every dense row)
    for name in ("thresh", "prob"):
        _, t_dev[name] = timed(lambda: drt.find_peaks_batch(tau=tau_eval, method=name))
        info, t_info = timed(lambda: drt.find_peaks_batch(tau=tau_eval, method=name, return_info=True), repeat=2)
        dev[name], t_dev[name]["call_wall_ms_median_with_return_info"] = info[2], t_info["call_wall_ms_median"]
    _, t_dev["map"] = timed(lambda: drt.peak_prob_batch(tau=tau_eval))

    # the host route
    def host_thresh():
        fxx = drt.predict_drt_batch(tau=tau_eval, order=2, normalize=True)
        out = []
        for row in fxx:
            prom = 0.05 * np.std(row[~np.isinf(row)]) + 5e-3
            out.append(signal.find_peaks(-row, height=0, prominence=prom)[0])
        return out

    li, ri = drt._extend_var_indices(tau_eval)
    s_lo, s_hi = predict.n_sigma((0.025, 0.975))

    def host_prob():
        fxx = drt.predict_drt_batch(tau=tau_eval, order=2, normalize=True)
        lo, hi, _ = drt.predict_drt_ci_batch(tau=tau_eval, order=2, normalize=True)
        var = ((hi - lo) / (s_hi - s_lo)) ** 2
        out = []
        for row, v in zip(fxx, var):
            idx, info = signal.find_peaks(-row, height=1e-3, prominence=5e-3)
            sigma = peaks.extend_var(v, li, ri, 1e-5)[idx] ** 0.5
            prob = 1 - special.erfc(np.minimum(info["prominences"], info["peak_heights"]) / (sigma * 2 ** 0.5))
            out.append(idx[prob >= 0.25])
        return out

    host, t_host = {}, {}
    for name, call in (("thresh", host_thresh), ("prob", host_prob)):
        wall = []
        for _ in range(max(1, a.repeat // 2)):
            t0 = time.perf_counter()
            host[name] = call()
            wall.append((time.perf_counter() - t0) * 1e3)
        t_host[name] = {"wall_ms_min": min(wall), "wall_ms_median": float(np.median(wall))}

    out = {"spectra": B, "nf": a.nf, "ntau": a.ntau, "n": drt._plan.n, "neval": len(tau_eval), "fit_wall_s": fit_wall,
           "predict_drt_order2": t_pred, "device": t_dev, "host_route": t_host,
           "host_over_device_whole_call": {k: t_host[k]["wall_ms_median"] / t_dev[k]["call_wall_ms_median"] for k in t_host},
           "thresh_kernels_over_one_predict_drt": t_dev["thresh"]["kernel_ms_min"] / t_pred["kernel_ms_min"],
           "prob_share_of_kernel_time_after_the_rows": t_dev["prob"]["after_the_rows_ms_min"] / t_dev["prob"]["kernel_ms_min"],
           "spectra_whose_kept_peaks_differ": {k: int(sum(not np.array_equal(p, q) for p, q in zip(dev[k], host[k]))) for k in host},
           "peaks_kept_mean": {k: float(np.mean([len(p) for p in dev[k]])) for k in dev}}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
