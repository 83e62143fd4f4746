"""Time DRTMD.predict_peak_prob on a synthetic map (default: 10 000 observations x 512 coefficients, the default evaluation grid
get_tau_eval(10), ndfilter=True, peak_spread_sigma=1, stored variances) on the device and with statement=True on the host -- the
figure DESIGN.md quotes.  For the record only: nothing asserts on it.

    python tools/map_predict_time.py [rows] [nsup]
"""
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from hipdrt.mapping.store import DRTMD  # noqa: E402


def main():
    rows = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    nsup = int(sys.argv[2]) if len(sys.argv) > 2 else 512
    rng = np.random.default_rng(0)
    tau = np.logspace(-7, 3, nsup)
    md = DRTMD(tau, psi_dim_names=["T"], store_eval_var=True, warn=False)
    psi, u = np.meshgrid(np.linspace(0, 1, rows), np.linspace(0, 1, nsup), indexing="ij")
    x = np.exp(-((u - 0.3 - 0.1 * psi) / 0.04) ** 2) + (0.4 + 0.5 * psi) * np.exp(-((u - 0.7) / 0.06) ** 2) + 0.01
    md.obs_psi = np.linspace(0, 1, rows)[:, None]
    md.obs_x = x * (1 + 0.01 * rng.standard_normal(x.shape))
    md.obs_fit_status, md.obs_ignore_flag = np.ones(rows, bool), np.zeros(rows, bool)
    md.obs_tau_indices = [(0, nsup)] * rows
    neval = len(md.get_tau_eval(10))
    md.obs_f_var = 1e-3 * (1 + rng.random((rows, neval)))
    md.obs_fxx_var = 1e-2 * (1 + rng.random((rows, neval)))
    kw = dict(ndfilter=True, peak_spread_sigma=1)
    md.predict_peak_prob(md.obs_psi[:64], **kw)                                   # the context, the library, the first launches
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        dev = md.predict_peak_prob(md.obs_psi, **kw)
        times.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    ref = md.predict_peak_prob(md.obs_psi, statement=True, **kw)
    t_host = time.perf_counter() - t0
    same = np.array_equal(dev == 0, ref == 0)
    print(f"map_predict {rows} x {nsup} -> {neval}: device {min(times) * 1e3:.1f} ms (best of 3, psi lookup, upload and download included), "
          f"statement {t_host:.2f} s, same peaks: {same}, max |difference| {np.nanmax(np.abs(dev - ref)):.1e}")


if __name__ == "__main__":
    main()
