"""Time DRT.evaluate_lml_batch() on a fitted batch next to DRT.estimate_param_var_batch() on the same plan, which runs the same
factorisation once per spectrum with n appended rows where the evidence runs it twice with none.

    python tools/bench_lml.py [--spectra 1024] [--nf 256] [--ntau 512] [--repeat 5] [--out FILE]

Each call is run once to warm up and then --repeat times; reported are the median of the time between HIP events around the
launches (hipdrt_debug_last_predict_ms; the variance entry point does not time itself, so only its wall time is given) and of
the wall time of the whole call, which ends in a device synchronise and adds allocations, uploads, downloads and the host side.
For information only: nothing is asserted."""
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

    freq = np.logspace(6, -1, a.nf)
    drt = DRT(fixed_basis_tau=np.logspace(-8, 2, a.ntau), warn=False)
    drt.fit_eis_batch(freq, synth.zarc2_batch(freq, a.spectra))
    plan, ctx = drt._plan, drt._plan.ctx

    def timed(call, events=None):
        wall, ev = [], []
        out = None
        for _ in range(a.repeat + 1):
            t0 = time.perf_counter()
            out = call()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(events() if events else np.nan)
        res = dict(wall_ms_median=float(np.median(wall[1:])), wall_ms_min=float(np.min(wall[1:])))
        if events:
            res.update(event_ms_median=float(np.median(ev[1:])), event_ms_min=float(np.min(ev[1:])))
        return out, res

    lml, t_lml = timed(drt.evaluate_lml_batch, lambda: ctx.debug_last_predict_ms()[0])
    (var, ok), t_var = timed(drt.estimate_param_var_batch)
    out = dict(spectra=plan.B, nf=a.nf, ntau=a.ntau, n=plan.n, m=plan.m, repeat=a.repeat, evaluate_lml_batch=t_lml,
               estimate_param_var_batch=t_var, lml_finite=int(np.isfinite(lml).sum()), lml_nan=int(np.isnan(lml).sum()),
               var_ok=int(np.sum(ok)))
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
