"""Time the scoring of C candidates per spectrum of a fitted batch through hipdrt_plan_score_candidates against the only route
the code before it had: C rounds of set_state + hipdrt_plan_llh_terms + hipdrt_plan_find_peaks.

    python tools/bench_candidates.py [--spectra 1024] [--nf 256] [--ntau 512] [--candidates 6] [--repeat 20] [--out FILE]

Both routes start from the same host array x (C, B, n) (the fit's solution scaled by C different factors: the values do not
matter to the time) and end with the same numbers on the host: rss, sum_log_w, the peak count and the peaks' positions, heights
and prominences of every candidate.  Each is run once to warm up and then --repeat times; reported are the median and the
minimum of the time between HIP events around the launches (hipdrt_debug_last_predict_ms: of the scoring entry as a whole; of
the old route the sum over its 2 C calls, each llh_terms launch and each find_peaks chain), and of the wall time of the whole
call (it ends in a device synchronise), which adds uploads, downloads and the host side.  The two routes' results are
compared: counts and positions exactly; the sums are two float64 evaluations of differences of large terms and agree to about
1e-10 relative (the largest relative difference is reported, 1e-8 is refused)."""
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
    ap.add_argument("--candidates", type=int, default=6)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    freq = np.logspace(6, -1, a.nf)
    tau = np.logspace(-8, 2, a.ntau)
    drt = DRT(fixed_basis_tau=tau, warn=False)
    drt.fit_eis_batch(freq, synth.zarc2_batch(freq, a.spectra))
    plan, ctx = drt._plan, drt._plan.ctx
    ln_tau = np.log(drt.get_tau_eval(10))
    opts = _ffi.peak_opts(search=1)
    x0 = plan.get("x")
    x = np.array([x0 * (1.0 + 0.02 * c) for c in range(a.candidates)])
    C, B, n, m = x.shape[0], plan.B, plan.n, plan.m

    def new_route():
        return plan.score_candidates(x, ln_tau_find=ln_tau, opts=opts)

    def old_route():
        out = dict(rss=[], sum_log_w=[], count=[], keep=[], heights=[], prominences=[])
        ms = 0.0
        for c in range(C):
            plan.set_state(x=x[c])
            rss, slw = plan.llh_terms()
            ms += ctx.debug_last_predict_ms()[1]
            pk = plan.find_peaks(ln_tau, opts, want=("keep", "heights", "prominences", "count"))
            ms += ctx.debug_last_predict_ms()[1]
            out["rss"].append(rss); out["sum_log_w"].append(slw)
            for k in ("count", "keep", "heights", "prominences"):
                out[k].append(pk[k])
        out["event_ms"] = ms
        return out

    def timed(call, events):
        wall, ev = [], []
        out = None
        for i in range(a.repeat + 1):
            t0 = time.perf_counter()
            out = call()
            wall.append((time.perf_counter() - t0) * 1e3)
            ev.append(events(out))
        wall, ev = np.array(wall[1:]), np.array(ev[1:])
        return out, dict(wall_ms_median=float(np.median(wall)), wall_ms_min=float(wall.min()), wall_ms_max=float(wall.max()),
                         event_ms_median=float(np.median(ev)), event_ms_min=float(ev.min()))

    # alternate the two routes once before timing (code objects, allocations), then time each
    new_route(); old_route()
    new, t_new = timed(new_route, lambda out: ctx.debug_last_predict_ms()[1])
    old, t_old = timed(old_route, lambda out: out["event_ms"])
    plan.set_state(x=x0)

    same = True
    for c in range(C):
        same &= bool(np.array_equal(new["count"][c], old["count"][c]))
        for b in range(B):
            k = np.nonzero(old["keep"][c][b])[0]
            same &= bool(np.array_equal(new["peak_index"][c, b][:len(k)], k[:new["peak_index"].shape[2]]))
    rel = max(float(np.max(np.abs(new["rss"] - np.array(old["rss"])) / np.abs(old["rss"]))),
              float(np.max(np.abs(new["sum_log_w"] - np.array(old["sum_log_w"])) / np.abs(old["sum_log_w"]))))
    # algorithmic bytes of the likelihood sums: rm (shared by the batch) and vmm once per call; x in, yh kept on chip
    out = dict(spectra=B, nf=a.nf, ntau=a.ntau, n=n, m=m, candidates=C, nfind=len(ln_tau), repeat=a.repeat,
               score_candidates=t_new, rounds_of_set_state_llh_terms_find_peaks=t_old,
               old_over_new_wall_median=t_old["wall_ms_median"] / t_new["wall_ms_median"],
               peaks_agree_exactly=same, sums_largest_relative_difference=rel,
               llh_matrix_bytes_read_per_workgroup=(m * n + m * m) * 8, llh_workgroups=B * ((C + 15) // 16),
               llh_flops=2.0 * 16 * ((C + 15) // 16) * B * (m * n + m * m))
    text = json.dumps(out, indent=1)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    assert same and rel < 1e-8, "the two routes disagree"


if __name__ == "__main__":
    main()
