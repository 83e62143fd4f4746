"""Time DRT.kk_test_batch: the two KK fits (hipdrt_plan_timings), the screen kernel (HIP events on the context's stream, around a
screen call that downloads nothing but the masks and limits) and, for scale, the production fit of the same batch.

    python tools/bench_kk.py [--spectra 1024] [--nf 256] [--ntau 512] [--out profiles/<tag>_kk_bench.json]
    rocprofv3 --kernel-trace --stats -d <dir> -- python tools/bench_kk.py --spectra 1024      (kernel durations, a run of its own)

The comparison of interest: the screen kernel against the hyper-parameter step of ONE outer iteration of the same batch -- both
are one workgroup per spectrum around an m x n matrix-vector product.  The second KK fit carries row factors and therefore runs
in one range (hipdrt_plan_set_subbatches); its fits/s beside the first KK fit's and the production fit's show what that costs."""
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
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    freq = np.logspace(6, -1, a.nf)
    tau = np.logspace(-8, 2, a.ntau)
    z = synth.zarc2_batch(freq, a.spectra)
    rng = np.random.default_rng(1)
    for b in range(a.spectra):                                  # a few points per spectrum off by about 5 %
        for k in rng.choice(a.nf, size=3, replace=False):
            z[b, k] *= 1 + 0.05 * rng.choice([-1, 1])

    drt = DRT(fixed_basis_tau=tau)
    drt.fit_eis_batch(freq, z[:8])                               # library start-up, lookups
    t0 = time.perf_counter()
    prod = drt.fit_eis_batch(freq, z)
    prod_wall = time.perf_counter() - t0
    t0 = time.perf_counter()
    prod = drt.fit_eis_batch(freq, z)
    prod_wall = min(prod_wall, time.perf_counter() - t0)

    kkd = DRT(fixed_basis_tau=tau)
    kkd.kk_test_batch(freq, z[:8])
    t0 = time.perf_counter()
    out = kkd.kk_test_batch(freq, z)
    kk_wall = time.perf_counter() - t0

    # the screen alone: HIP events on the context's stream, small downloads only
    plan = kkd._plan
    stream = torch.cuda.ExternalStream(plan.ctx.stream)
    opts = kkd._kk_opts()
    screen_ms = []
    for _ in range(a.repeat + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record(stream)
        plan.kk_screen(opts, z_hat=False, residuals=False)
        e1.record(stream)
        e1.synchronize()
        screen_ms.append(e0.elapsed_time(e1))
    t_w = []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        plan.kk_screen(opts)
        t_w.append((time.perf_counter() - t0) * 1e3)

    passes = out["passes"]
    t_kk = [p["timings_ms"] for p in passes]
    # (launch counts of the last fit, the one with row factors: one range, so hyper time / launches is one outer iteration's step)
    t_last, l_last = plan.timings()
    res = {
        "spectra": a.spectra, "nf": a.nf, "ntau": a.ntau, "n": plan.n,
        "production_fit": {"wall_s": prod_wall, "fits_per_s": a.spectra / prod_wall, "timings_ms": prod["timings_ms"],
                           "outer_iters_mean": float(np.mean(prod["outer_iters"]))},
        "kk_test_batch_wall_s": kk_wall,
        "kk_fit_1": {"timings_ms": t_kk[0], "fits_per_s": a.spectra / (t_kk[0]["total"] * 1e-3)},
        "kk_fit_2_row_factors_one_range": {"timings_ms": t_kk[1], "fits_per_s": a.spectra / (t_kk[1]["total"] * 1e-3),
                                           "launches": l_last,
                                           "hyper_ms_per_outer_iteration": t_last["hyper"] / max(l_last["hyper"], 1)},
        "screen_events_ms": {"first": screen_ms[0], "min": min(screen_ms[1:]), "median": float(np.median(screen_ms[1:]))},
        "screen_call_with_all_downloads_wall_ms": float(np.median(t_w)),
        "outliers_per_spectrum_mean": [float(p["outlier_mask"].sum(axis=1).mean()) for p in passes],
        "status_counts": {int(k): int(v) for k, v in zip(*np.unique(out["status"], return_counts=True))},
    }
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
