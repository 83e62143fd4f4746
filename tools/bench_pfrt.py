"""Time predict_pfrt_batch next to the PFRT fit whose steps it reads.

    python tools/bench_pfrt.py [--spectra 1024] [--nf 256] [--ntau 512] [--steps 11] [--repeat 5] [--out profiles/pfrt_bench.json]

fit        pfrt_fit_eis_batch: one warm-up call, then `--fits` timed calls; the wall time of the whole call (every step ends with
           a download, i.e. a device synchronise), the step recording included
predict    predict_pfrt_batch on the 10-points-per-decade grid with the defaults, with return_info (every row comes down) and
           without (the PFRT alone): one warm-up call each, then `--repeat` timed calls, host clock around the call (it ends with
           the downloads); per step it forms the step P of the batch, factorises every one of them with both orders' rows, applies
           the peak rule and the step kernel, then one combine kernel
store      bytes of the step store per spectrum (hipdrt_plan_pfrt_bytes_per_spectrum)"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hipdrt import _ffi, synth  # noqa: E402
from hipdrt.models import DRT  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--spectra", type=int, default=1024)
    ap.add_argument("--nf", type=int, default=256)
    ap.add_argument("--ntau", type=int, default=512)
    ap.add_argument("--steps", type=int, default=11)
    ap.add_argument("--fits", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    freq = np.logspace(6, -1, a.nf)
    tau = np.logspace(-8, 2, a.ntau)
    z = synth.zarc2_batch(freq, a.spectra)
    factors = np.logspace(-1, 1, a.steps)
    drt = DRT(fixed_basis_tau=tau, warn=False)

    def wall_ms(call, repeat):
        out, t = None, []
        for _ in range(repeat + 1):                 # (the first call is the warm-up)
            t0 = time.perf_counter()
            out = call()
            t.append((time.perf_counter() - t0) * 1e3)
        return out, {"first_ms": t[0], "min_ms": min(t[1:]), "median_ms": float(np.median(t[1:])), "max_ms": max(t[1:])}

    pr, t_fit = wall_ms(lambda: drt.pfrt_fit_eis_batch(freq, z, factors=factors), a.fits)
    tau_eval = drt.get_tau_eval(10)
    (tot, info), t_info = wall_ms(lambda: drt.predict_pfrt_batch(tau_pfrt=tau_eval, return_info=True), a.repeat)
    _, t_lean = wall_ms(lambda: drt.predict_pfrt_batch(tau_pfrt=tau_eval), a.repeat)
    ok = info["status"] >= 0
    out = {"spectra": a.spectra, "nf": a.nf, "ntau": a.ntau, "n": drt._plan.n, "steps": a.steps, "neval": len(tau_eval),
           "pfrt_fit_eis_batch_wall": t_fit, "predict_pfrt_batch_wall_with_info": t_info, "predict_pfrt_batch_wall": t_lean,
           "predict_over_fit": t_lean["median_ms"] / t_fit["median_ms"],
           "outer_iterations_total_mean": float(np.mean(np.sum(pr["step_iters"], axis=0))),
           "store_bytes_per_spectrum": _ffi.pfrt_bytes_per_spectrum(drt._plan.n, a.steps),
           "spectra_ok": int(ok.sum()), "peaks_per_spectrum_last_step_mean": float(np.mean(np.count_nonzero(info["step_pfrt"][-1][ok], axis=1))),
           "finite_rows": int(np.isfinite(tot[ok]).all(axis=1).sum())}
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
