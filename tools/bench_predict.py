"""Time the device predictions of a fitted batch against the host route they replace.

    python tools/bench_predict.py [--spectra 10000] [--nf 256] [--ntau 512] [--neval 241] [--npred 256] [--out profiles/<tag>.json]

device    kernel time of predict_drt_batch (evaluation matrix + row application) and predict_z_batch (impedance matrices at the
          requested frequencies + row application + assembly) by HIP events around the launches (hipdrt_debug_last_predict_ms),
          and the wall time of the whole call with its download of the result
host      what the code before these methods forced: download x, then numpy ``x @ E.T`` with E built on the host, same process
bandwidth bytes = x read + Y written + E, over the kernel time, as a fraction of the device's HBM peak (8 TB/s on an MI355X)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hipdrt import synth  # noqa: E402
from hipdrt.matrices import basis  # noqa: E402
from hipdrt.models import DRT  # noqa: E402

HBM_PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spectra", type=int, default=10000)
    ap.add_argument("--nf", type=int, default=256)
    ap.add_argument("--ntau", type=int, default=512)
    ap.add_argument("--neval", type=int, default=241)
    ap.add_argument("--npred", type=int, default=256)
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
    plan, ctx = drt._plan, drt._plan.ctx
    tau_eval = np.logspace(-9, 3, a.neval)
    f_pred = np.logspace(6.5, -1.5, a.npred)
    B, n, K = a.spectra, plan.n, a.ntau

    def timed(call):
        ms, wall = [], []
        for _ in range(a.repeat + 1):
            t0 = time.perf_counter()
            out = call()
            wall.append((time.perf_counter() - t0) * 1e3)
            ms.append(ctx.debug_last_predict_ms()[0])
        return out, {"kernel_ms_first": ms[0], "kernel_ms_min": min(ms[1:]), "kernel_ms_median": float(np.median(ms[1:])),
                     "call_wall_ms_median": float(np.median(wall[1:]))}

    mu, t_drt = timed(lambda: drt.predict_drt_batch(tau=tau_eval))
    zz, t_z = timed(lambda: drt.predict_z_batch(f_pred))

    def traffic(r, t):
        nbytes = 8.0 * (B * K + B * r + r * K)
        return {"bytes": nbytes, "GB_per_s": nbytes / (t["kernel_ms_min"] * 1e-3) / 1e9,
                "fraction_of_hbm_peak": nbytes / (t["kernel_ms_min"] * 1e-3) / HBM_PEAK}

    # the host route: x comes down, the product is numpy's
    host = []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        res = plan.download(lean=True)
        e = basis.construct_func_eval_matrix(np.log(tau), np.log(tau_eval), epsilon=drt.tau_epsilon, order=0)
        mu_host = res["fit_x"] @ e.T
        host.append((time.perf_counter() - t0) * 1e3)
    dev = float(np.abs(mu - mu_host).max() / np.abs(mu_host).max())

    out = {"spectra": B, "nf": a.nf, "ntau": a.ntau, "n": n, "neval": a.neval, "npred": a.npred, "fit_wall_s": fit_wall,
           "predict_drt": dict(t_drt, **traffic(a.neval, t_drt)),
           "predict_z": dict(t_z, **traffic(2 * a.npred, t_z)),
           "host_route_download_plus_numpy_ms": {"min": min(host), "median": float(np.median(host))},
           "device_vs_host_max_deviation_of_peak": dev, "z_finite": bool(np.isfinite(zz).all())}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
