"""Time the device badness scores on a 10 000-observation map (needs the GPU): the fit score of a 10 000 x 512 array
(score_group_fit_badness: median (3, 3), std (5, 3)) and the data score of a 10 000 x 4096 chrono array with its current array
plus a 10 000 x 512 impedance array (score_group_data_badness: scaling, flag_outliers with the 5 % rule, median (3, 1), std
(5, 3)), through mapping.nddata.score_rows with upload and download inside.  Printed per case: the end-to-end host time, the
device time between upload and download (HIP events), and the time the same chain takes on this host with scipy.ndimage's
rank filters and numpy's percentiles in the reference's order of operations (hybdrt/mapping/nddata.py: flag_outliers 152-175,
flag_bad_obs 178-211; skipped with --no-host or where scipy is missing).

    python tools/probe_map_badness.py [--rows 10000] [--repeats 5] [--no-host] [--json FILE]
"""
import argparse
import json
import os
import sys
import time
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def surface(rows, cols, seed):
    rng = np.random.default_rng(seed)
    psi, lt = np.meshgrid(np.linspace(0, 1, rows), np.linspace(0, 1, cols), indexing="ij")
    a = np.exp(-((lt - 0.3 - 0.1 * psi) / 0.12) ** 2) + (0.4 + 0.5 * psi) * np.exp(-((lt - 0.7) / 0.2) ** 2) + 0.05
    a = a * (1 + 0.02 * rng.standard_normal(a.shape))
    a[(2 * rows) // 3] *= 2.5
    a[rows // 3] = np.nan
    n = rows * cols // 500
    a[rng.integers(0, rows, n), rng.integers(0, cols, n)] *= 1.8
    return a


def host_chain(a, median_size, std_size, scale_src=None, ignore_outliers=False):
    """the reference's chain with scipy's filters (what DRTMD.score_group_*_badness runs per array)"""
    from scipy import ndimage

    from hipdrt.mapping import nddata
    from hipdrt.models import kk

    def iqr(x, size):
        return ndimage.percentile_filter(x, 75, size=size) - ndimage.percentile_filter(x, 25, size=size)

    a = a.copy()
    if scale_src is not None:
        mid = 0.5 * (np.nanpercentile(a, 98, axis=1) + np.nanpercentile(a, 2, axis=1))
        rng = np.nanpercentile(scale_src, 98, axis=1) - np.nanpercentile(scale_src, 2, axis=1)
        a = (a - mid[:, None]) / rng[:, None]
    if ignore_outliers:
        y_filt = nddata.impute_nans_statement(a, sigma=0.5) if np.any(np.isnan(a)) else a
        mu_in = ndimage.median_filter(y_filt, nddata.FLAG_SIZE)
        sigma_in = iqr(y_filt, nddata.FLAG_SIZE) / 1.349 + 0.05 * kk.robust_std(np.nan_to_num(y_filt)) + 1e-8
        p_out = np.nan_to_num(nddata.outlier_prob(a, mu_in, sigma_in, np.abs(a - mu_in) + 1e-8, 0.01))
        flags = p_out > nddata.FLAG_THRESH
        a[(np.sum(flags, axis=1) < int(a.shape[1] * 0.05))[:, None] & flags] = np.nan
    filt = ndimage.median_filter(a, size=median_size)
    tmp = filt.copy()
    tmp[np.isnan(tmp)] = np.nanmedian(tmp)
    x_std = iqr(tmp, std_size) / 1.349 + 0.1 * kk.robust_std(filt[~np.isnan(filt)])
    return np.sum(np.nan_to_num((a - filt) / x_std) ** 2, axis=-1) / a.shape[-1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-host", action="store_true")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    warnings.simplefilter("ignore")
    from hipdrt import _ffi
    from hipdrt.mapping import nddata
    ctx = _ffi.get_context(0)
    rows = args.rows
    x = surface(rows, 512, 7)
    v = surface(rows, 4096, 8)
    i = 1e-3 * (1 + 0.01 * np.random.default_rng(9).standard_normal(v.shape))
    z = surface(rows, 512, 10)
    cases = {"fit_512": [(x, dict(median_size=(3, 3), std_size=(5, 3)))],
             "data_4096_512": [(v, dict(median_size=(3, 1), std_size=(5, 3), scale_src=i, ignore_outliers=True)),
                               (z, dict(median_size=(3, 1), std_size=(5, 3), ignore_outliers=True))]}
    results = {"rows": rows, "device": ctx.device_info()["arch"], "repeats": args.repeats}
    for name, calls in cases.items():
        host, dev = [], []
        for rep in range(args.warmup + args.repeats):
            t0, ms, rss = time.perf_counter(), 0.0, []
            for a, kw in calls:
                rss.append(nddata.score_rows(a, **kw))
                ms += ctx.debug_map_badness_ms()
            if rep >= args.warmup:
                host.append((time.perf_counter() - t0) * 1e3)
                dev.append(ms)
        r = results[name] = dict(host_ms=dict(median=float(np.median(host)), min=min(host), max=max(host)),
                                 device_ms=dict(median=float(np.median(dev)), min=min(dev), max=max(dev)),
                                 array_gb=sum(a.size for a, _ in calls) * 8 / 1e9)
        line = (f"{name}: end to end {r['host_ms']['median']:.1f} ms ({r['host_ms']['min']:.1f} .. {r['host_ms']['max']:.1f}), "
                f"device {r['device_ms']['median']:.2f} ms ({min(dev):.2f} .. {max(dev):.2f})")
        if not args.no_host:
            t0 = time.perf_counter()
            ref = [host_chain(a, **kw) for a, kw in calls]
            r["reference_host_ms"] = (time.perf_counter() - t0) * 1e3
            r["max_rel_deviation"] = max(float(np.max(np.abs(g - h) / np.where(h > 0, h, 1.0))) for g, h in zip(rss, ref))
            line += f", scipy chain on this host {r['reference_host_ms']:.0f} ms, max relative deviation {r['max_rel_deviation']:.1e}"
        print(line, flush=True)
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
