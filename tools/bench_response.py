"""Time the device response prediction of a fitted hybrid batch next to a host loop of its numpy statement (information only).

    python tools/bench_response.py [--members 5] [--repeat 5] [--out profiles/<tag>.json]

device    kernel time of predict_response_batch (unit-step layers + row application + assembly) by HIP events around the launches
          (hipdrt_debug_last_predict_ms), and the wall time of the whole call with its uploads and the download of the result
host      hipdrt.models.response.predict_response_rows, one member at a time, on unit-step layers that are already built (the
          stand-alone builder's, its time not counted) and the members' own fit parameters"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from hipdrt import _ffi, synth  # noqa: E402
from hipdrt.matrices import mat1d  # noqa: E402
from hipdrt.models import DRT, background, response  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--members", type=int, default=5)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    i_steps = [1e-3 * (0.5 + 0.25 * (b % 7)) for b in range(a.members)]
    meas = [synth.hybrid_measurement(seed=b, jitter=True, i_step=i_steps[b]) for b in range(a.members)]
    times = meas[0][0]
    drt = DRT(warn=False)
    drt.fit_hybrid_batch(times, [m[1] for m in meas], [m[2] for m in meas], meas[0][3], [m[4] for m in meas])
    ctx = drt._plan.ctx
    ms, wall = [], []
    for _ in range(a.repeat + 1):
        t0 = time.perf_counter()
        out = drt.predict_response_batch()
        wall.append((time.perf_counter() - t0) * 1e3)
        ms.append(ctx.debug_last_predict_ms()[0])

    preps, fps = drt._last_prepared
    p0 = preps[0]
    _, u = ctx.response_matrix(times, drt.basis_tau, p0["step_times"], np.ones(len(p0["step_times"])), drt.tau_epsilon,
                               mode=_ffi.MODE_INTERP, lookup=drt._lookups(ctx)["response"], layered=True)
    strength = drt._vz_strength(p0["sample_times"], p0["frequencies"], p0["nonconsec_step_times"], drt.fit_kwargs["vz_offset_eps"])[0]
    vb_mat = background.get_baseline_matrix(times, 0, normalize=False)
    host = []
    for _ in range(a.repeat):
        t0 = time.perf_counter()
        rows = np.array([response.predict_response_rows(
            u, pr["step_sizes"], fp, vz_strength=strength, vb_mat=vb_mat,
            inf_rv=mat1d.construct_ohmic_response_vector(times, "ideal", pr["step_times"], pr["step_sizes"], None, None, True))
            for pr, fp in zip(preps, fps)])
        host.append((time.perf_counter() - t0) * 1e3)
    res = {"members": a.members, "nt": len(times), "ntau": len(drt.basis_tau), "steps": len(p0["step_times"]),
           "device_kernel_ms": {"first": ms[0], "min": min(ms[1:]), "median": float(np.median(ms[1:]))},
           "device_call_wall_ms_median": float(np.median(wall[1:])),
           "host_statement_loop_ms": {"min": min(host), "median": float(np.median(host))},
           "device_vs_host_max_deviation_of_peak": float(np.abs(out - rows).max() / np.abs(rows).max())}
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
