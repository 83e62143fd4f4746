"""Time the device map filter on a 10 000 x 512 map (needs the GPU): mapping.ndx.filter_ndx with upload and download inside,
for the defaults with sigma=(1, 0) and for adaptive=True, max_sigma=(2, 1).  After warm-up calls the same call is repeated and
the median, the fastest and the slowest are printed: the end-to-end host time (table building, allocation, upload, kernels,
download), the device time between upload and download (HIP events), and the share of the HBM peak (8 TB/s) the full-array
reads and writes the driver counts as it launches would need in that device time.

    python tools/probe_map_filter.py [--rows 10000] [--cols 512] [--repeats 9] [--json FILE]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HBM_PEAK = 8.0e12


def surface(rows, cols, seed=7):
    rng = np.random.default_rng(seed)
    psi, lt = np.meshgrid(np.linspace(0, 1, rows), np.linspace(0, 1, cols), indexing="ij")
    a = np.exp(-((lt - 0.3 - 0.1 * psi) / 0.12) ** 2) + (0.4 + 0.5 * psi) * np.exp(-((lt - 0.7) / 0.2) ** 2) + 0.05
    a = a * (1 + 0.02 * rng.standard_normal(a.shape))
    a[(2 * rows) // 3] *= 3
    a[rows // 3] = np.nan
    a[rng.integers(0, rows, rows * cols // 150), rng.integers(0, cols, rows * cols // 150)] = np.nan
    return a


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=10000)
    ap.add_argument("--cols", type=int, default=512)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    from hipdrt import _ffi
    from hipdrt.mapping.ndx import filter_ndx
    ctx = _ffi.get_context(0)
    a = surface(args.rows, args.cols)
    array_bytes = a.size * 8
    results = {"shape": [args.rows, args.cols], "device": ctx.device_info()["arch"], "repeats": args.repeats}
    for name, kw in (("default_sigma_1_0", dict(sigma=(1, 0))), ("adaptive_max_sigma_2_1", dict(adaptive=True, max_sigma=(2, 1)))):
        for _ in range(args.warmup):
            out = filter_ndx(a, 0, **kw)
        host, dev = [], []
        for _ in range(args.repeats):
            t0 = time.perf_counter()
            out = filter_ndx(a, 0, **kw)
            host.append((time.perf_counter() - t0) * 1e3)
            launches, arrays, ms = ctx.debug_map_filter_stats()
            dev.append(ms)
        assert np.isfinite(out[~np.isnan(a)]).all()
        traffic = arrays * array_bytes
        med = float(np.median(dev))
        results[name] = dict(host_ms=dict(median=float(np.median(host)), min=min(host), max=max(host)),
                             device_ms=dict(median=med, min=min(dev), max=max(dev)), launches=launches, array_passes=arrays,
                             traffic_gb=traffic / 1e9, hbm_fraction=traffic / (med * 1e-3) / HBM_PEAK)
        r = results[name]
        print(f"{name}: host {r['host_ms']['median']:.1f} ms ({r['host_ms']['min']:.1f} .. {r['host_ms']['max']:.1f}), "
              f"device {med:.2f} ms ({min(dev):.2f} .. {max(dev):.2f}), {launches} launches, {arrays} array passes = "
              f"{traffic / 1e9:.2f} GB, {100 * r['hbm_fraction']:.1f} % of 8 TB/s")
    if args.json:
        with open(args.json, "w") as f:
            json.dump(results, f, indent=1)
    print(json.dumps(results))


if __name__ == "__main__":
    main()
