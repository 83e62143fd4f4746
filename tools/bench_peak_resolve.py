"""Time the per-peak resolution of a fitted batch on the device against the host route it replaces.

    python tools/bench_peak_resolve.py [--spectra 10000] [--nf 256] [--ntau 512] [--repeat 5] [--out profiles/peak_resolve_bench.json]

device    quantify_peaks_batch() and estimate_peak_drts_batch() on a 121-point output grid, peaks found on the
          10-points-per-decade grid: kernel time by HIP events around the launches of one call
          (hipdrt_debug_last_predict_ms: [0] the mean rows, [1] all launches, peaks_kernel and peak_resolve_kernel included),
          best of --repeat after a warm-up, and the wall time of the whole call with its download and the per-spectrum lists
host      what the code before these methods forced for the same result: find_peaks_batch(return_info=True),
          predict_drt_batch for both orders (unnormalised), the download of x, and the numpy statement
          (models/peaks.py resolve_peaks_row) per spectrum in a Python loop -- every device call of it is one the parent
          commit has, unchanged
check     the two routes' peaks and troughs are compared on every spectrum; the resistances by their largest deviation"""
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
    ap.add_argument("--nout", type=int, default=121)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    freq = np.logspace(6, -1, a.nf)
    tau = np.logspace(-8, 2, a.ntau)
    z = synth.zarc2_batch(freq, a.spectra)
    drt = DRT(fixed_basis_tau=tau, warn=False)
    t0 = time.perf_counter()
    drt.fit_eis_batch(freq, z)
    fit_wall = time.perf_counter() - t0
    ctx, plan = drt._plan.ctx, drt._plan
    tau_find = drt.get_tau_eval(10)
    tau_out = np.logspace(np.log10(tau_find[0]), np.log10(tau_find[-1]), a.nout)
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
                     "call_wall_ms_min": float(np.min(wall[1:])), "call_wall_ms_median": float(np.median(wall[1:]))}

    t_dev = {}
    _, t_dev["find_peaks_batch"] = timed(lambda: drt.find_peaks_batch(tau=tau_find))
    (r_dev, info), t_dev["quantify_peaks_batch"] = timed(lambda: drt.quantify_peaks_batch(tau=tau_out, tau_find_peaks=tau_find,
                                                                                          return_info=True))
    _, t_dev["quantify_peaks_batch_resistances_only"] = timed(lambda: drt.quantify_peaks_batch(tau=tau_out, tau_find_peaks=tau_find))
    _, t_dev["estimate_peak_drts_batch"] = timed(lambda: drt.estimate_peak_drts_batch(tau=tau_out, tau_find_peaks=tau_find))

    # the host route
    e0 = predict.eval_matrix(drt.basis_tau, tau_out, drt.tau_epsilon)
    ln_find, ln_basis, ln_out = np.log(tau_find), np.log(drt.basis_tau), np.log(tau_out)
    area = predict.basis_area(drt.tau_epsilon)
    parts = {}

    def host():
        t = [time.perf_counter()]
        _, _, idx, _ = drt.find_peaks_batch(tau=tau_find, return_info=True)
        t.append(time.perf_counter())
        f = drt.predict_drt_batch(tau=tau_find, order=0)
        fxx = drt.predict_drt_batch(tau=tau_find, order=2)
        t.append(time.perf_counter())
        x = plan.get("x")[:, plan.ns:] * plan.get("coef_scale")[:, None]
        t.append(time.perf_counter())
        out = [peaks.resolve_peaks_row(f[b], fxx[b], idx[b], x[b], ln_find, ln_basis, e0, ln_out, area) for b in range(B)]
        t.append(time.perf_counter())
        for k, (u, v) in zip(("find_peaks_ms", "two_predictions_ms", "download_x_ms", "numpy_loop_ms"), zip(t[:-1], t[1:])):
            parts.setdefault(k, []).append((v - u) * 1e3)
        return out

    wall = []
    for _ in range(max(1, a.repeat // 2)):
        t0 = time.perf_counter()
        ref = host()
        wall.append((time.perf_counter() - t0) * 1e3)
    t_host = {"wall_ms_min": min(wall), "wall_ms_median": float(np.median(wall)), **{k: float(np.median(v)) for k, v in parts.items()}}

    differ = sum(not (np.array_equal(info["peak_index"][b], ref[b]["peak_index"]) and
                      np.array_equal(info["trough_index"][b], ref[b]["troughs"])) for b in range(B))
    dev_r = max((float(np.max(np.abs(r_dev[b] - ref[b]["r_peaks"]) / np.max(np.abs(ref[b]["r_peaks"])))) for b in range(B)
                 if len(r_dev[b]) and len(r_dev[b]) == len(ref[b]["r_peaks"])), default=0.0)
    q, e = t_dev["quantify_peaks_batch"], t_dev["estimate_peak_drts_batch"]
    out = {"spectra": B, "nf": a.nf, "ntau": a.ntau, "n": plan.n, "nfind": len(tau_find), "nout": a.nout, "fit_wall_s": fit_wall,
           "device": t_dev, "host_route": t_host,
           "resolve_kernel_ms_min": q["kernel_ms_min"] - t_dev["find_peaks_batch"]["kernel_ms_min"],
           "host_over_device_whole_call": {"quantify_peaks_batch": t_host["wall_ms_median"] / q["call_wall_ms_median"],
                                           "estimate_peak_drts_batch": t_host["wall_ms_median"] / e["call_wall_ms_median"]},
           "spectra_whose_peaks_or_troughs_differ": int(differ), "largest_r_peaks_deviation_of_the_spectrums_peak": dev_r,
           "peaks_mean": float(np.mean([len(p) for p in r_dev])), "peaks_max": int(max(len(p) for p in r_dev))}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
