"""Generate the map-badness fixture tests/golden/refrun_map_badness.npz (build container only: imports the reference through the
shims of oracle/refshim, like tools/make_map_filter_golden.py, and needs scipy).

Recorded:
  rank filters   scipy.ndimage.median_filter / percentile_filter (25, 75) and the reference's iqr_filter on deterministic
                 surfaces of shapes (3, 5) (smaller than a 5 x 3 window: the reflection repeats), (1, 40), (23, 37) (one partial
                 tile, scattered NaNs) and (70, 130) (several tiles and wavefronts on both axes; one NaN row, two adjacent NaN
                 rows, scattered NaNs, one row scaled by 2.5).  The small shapes carry every filter at every size of
                 map_badness_util.SIZES; the (70, 130) one a selection that still visits every size (A70_FILTERS), to keep the
                 file small.  Inputs are rounded to float32 values, so the outputs (window entries and their differences)
                 compress.
  chains         the reference's flag_outliers(filter_size=(5, 1), thresh=0.7) and flag_bad_obs(std_size=(5, 3),
                 return_rss=True) against scipy's (3, 3) median on the (23, 37) and (70, 130) surfaces with spikes added.
  store          DRTMD.score_group_fit_badness on a 14 x 91 map with an ignored and an unfitted observation, and
                 DRTMD.score_group_data_badness on a hybrid group and on a mixed one (every second observation EIS-only) of 12
                 observations x 200 chrono samples x 31 frequencies.
  percentiles    np.percentile / np.nanpercentile / np.nanmedian on the segments of tests/map_badness_util.py.

The file is only written when no flag hinges on a rounding: no p_out within 1e-9 of thresh, no |x - mu_in| within 4 ulp of
sigma_in, one row with fewer flagged points than int(0.05 cols) and one with more, no x_std equal to 0.

    python tools/make_map_badness_golden.py
"""
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle", "refshim"))
import oracle_boot  # noqa: E402,F401

from scipy import ndimage  # noqa: E402
from hybdrt.filters import _filters as rf  # noqa: E402
from hybdrt.mapping import nddata as rnd  # noqa: E402
from hybdrt.mapping.drtmd import DRTMD as RefDRTMD  # noqa: E402

import map_badness_util as util  # noqa: E402
from hipdrt.mapping import nddata  # noqa: E402

A70_FILTERS = (("median", (3, 3)), ("median", (7, 7)), ("median", (4, 3)), ("median", (5, 1)), ("iqr", (5, 3)), ("iqr", (5, 1)),
               ("iqr", (3, 1)), ("p25", (4, 3)))


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def surface(shape, seed):
    rng = np.random.default_rng(seed)
    r, c = shape
    psi, lt = np.meshgrid(np.linspace(0, 1, r), np.linspace(0, 1, c), indexing="ij")
    a = np.exp(-((lt - 0.3 - 0.1 * psi) / 0.12) ** 2) + (0.4 + 0.5 * psi) * np.exp(-((lt - 0.7) / 0.2) ** 2) + 0.05
    a = a * (1 + 0.02 * rng.standard_normal(shape))
    if shape == (70, 130):
        a[46] *= 2.5
        a[20] = np.nan
        a[33:35] = np.nan
    if r >= 20:
        for k in range(r * c // 150):
            a[(7 * k + 5) % r, (11 * k + 3) % c] = np.nan
    return f32(a)


def rank_outputs(a, size):
    return {"median": ndimage.median_filter(a, size=size), "p25": ndimage.percentile_filter(a, 25, size=size),
            "p75": ndimage.percentile_filter(a, 75, size=size), "iqr": rf.iqr_filter(a, size=size)}


def spiked(a, seed):
    """single-point outliers: a few in many rows, more than 5 % of the columns in one"""
    rng = np.random.default_rng(seed)
    y = a.copy()
    r, c = a.shape
    rows, cols = rng.integers(0, r, r // 2), rng.integers(0, c, r // 2)
    y[rows, cols] *= 1.8
    busy = r // 2 + 1
    y[busy, rng.choice(c, max(3, c // 8), replace=False)] *= 1.8
    return f32(y)


def check_flags(name, y, ref_flags):
    flags, p_out, mu_in, sigma_in = nddata.flag_outliers_statement(y, filter_size=(5, 1), thresh=0.7, return_prob=True)
    assert np.array_equal(flags, ref_flags), f"{name}: the numpy statement's flags differ from the reference's"
    assert np.min(np.abs(p_out - 0.7)) > 1e-9, f"{name}: a p_out within 1e-9 of thresh"
    dev = np.abs(y - mu_in)
    ok = ~np.isnan(dev)
    assert np.all(np.abs(dev[ok] - sigma_in[ok]) > 4 * np.spacing(sigma_in[ok])), f"{name}: |x - mu_in| within 4 ulp of sigma_in"
    count, least = flags.sum(axis=1), int(y.shape[1] * 0.05)
    assert np.any(count < least) and np.any(count > least), f"{name}: both branches of the 5 % rule must run"
    if least > 1:
        assert np.any((count > 0) & (count < least)), f"{name}: no row whose flagged points the 5 % rule removes"
    print(name, "flagged per row", count.tolist(), "against", least)
    return count


def data_group(kind, seed):
    """12 observations: (psi, (t, i, v) or None, (f, z)) -- a charging step and an RC arc that grow with psi, observation 5
    scaled by 2.5, a few spikes"""
    rng = np.random.default_rng(seed)
    f = np.logspace(5, -1, 31)
    t = np.linspace(0, 1, 200)
    obs = []
    for k in range(12):
        z = (1 + 0.1 * k) * (1 / (1 + 1j * 2 * np.pi * f * 1e-3)) + 0.01 * rng.standard_normal(31) + 0.01j * rng.standard_normal(31)
        i = np.where(t > 0.1, 1e-3, 0.0) + 1e-7 * rng.standard_normal(200)
        v = (1 + 0.1 * k) * 1e-3 * (t > 0.1) * (1 - np.exp(-np.maximum(t - 0.1, 0) / 1e-2)) + 1e-6 * rng.standard_normal(200)
        if k == 5:
            z, v = z * 2.5, v * 2.5
        if k in (2, 7):
            v[rng.choice(200, 3, replace=False)] += 4e-4
            z[rng.choice(31, 1)] *= 1.5
        if k == 9:
            v[rng.choice(200, 30, replace=False)] += 4e-4
            z[rng.choice(31, 6, replace=False)] *= 1.5
        chrono = (t, i, v) if kind == "hybrid" or k % 2 == 0 else None
        obs.append((float(k), chrono, (f, z)))
    return obs


def main():
    warnings.simplefilter("ignore")
    out = {}
    surfaces = {"a3x5": surface((3, 5), 1), "a1x40": surface((1, 40), 2), "a23": surface((23, 37), 3), "a70": surface((70, 130), 4)}
    for name, a in surfaces.items():
        out[f"rank.{name}.in"] = a
        for size in util.SIZES:
            res = rank_outputs(a, size)
            for kind, val in res.items():
                if name != "a70" or (kind, size) in A70_FILTERS:
                    out[f"rank.{name}.{kind}.{size[0]}x{size[1]}"] = val

    for name, seed in (("a23", 11), ("a70", 12)):
        y = spiked(surfaces[name], seed)
        ref_flags = rnd.flag_outliers(y, filter_size=(5, 1), thresh=0.7)
        count = check_flags(name, y, ref_flags)
        x_filt = ndimage.median_filter(y, size=(3, 3))
        x_std = nddata.bad_obs_std(x_filt, (5, 3))
        assert not np.any(x_std == 0), f"{name}: an x_std of 0"
        bad, rss = rnd.flag_bad_obs(y, x_filt, std_size=(5, 3), return_rss=True)
        out[f"chain.{name}.in"], out[f"chain.{name}.flags"], out[f"chain.{name}.count"] = y, ref_flags, count
        out[f"chain.{name}.rss"], out[f"chain.{name}.bad"] = rss, bad

    # the fit score: a 14 x 91 map in a store of 16 observations (two of another group), rows entered out of psi order
    rng = np.random.default_rng(21)
    tau = np.logspace(-7, 2, 91)
    u = np.linspace(0, 1, 91)
    order = rng.permutation(14)
    md = RefDRTMD(tau_supergrid=tau, psi_dim_names=["T"])
    for k in list(order) + [14, 15]:
        md.add_observation(np.array([float(k)]), None, None, group_id="g" if k < 14 else "other")
    x = np.array([np.exp(-((u - 0.3 - 0.01 * k) / 0.1) ** 2) + 0.5 * np.exp(-((u - 0.7) / 0.15) ** 2) for k in range(16)])
    x = f32(x * (1 + 0.02 * rng.standard_normal(x.shape)))
    psi = md.obs_psi[:, 0].astype(int)
    md.obs_x = x[psi].copy()
    md.obs_x[psi == 5] *= 2.5
    md.obs_fit_status = np.ones(16, bool)
    md.obs_ignore_flag = np.zeros(16, bool)
    md.obs_ignore_flag[psi == 8] = True
    md.obs_fit_status[psi == 11] = False
    md.obs_special = {}
    md.score_group_fit_badness("g", ["T"])
    out["fit.psi"], out["fit.obs_x"] = md.obs_psi.copy(), md.obs_x.copy()
    out["fit.ignore"], out["fit.status"] = md.obs_ignore_flag.copy(), md.obs_fit_status.copy()
    out["fit.badness"] = md.obs_fit_badness.copy()
    assert out["fit.badness"][psi == 5][0] > 2 and np.all(out["fit.badness"][psi >= 14] == 0)

    for kind in ("hybrid", "mixed"):
        obs = data_group(kind, 31)
        md = RefDRTMD(tau_supergrid=tau, psi_dim_names=["T"])
        for k, chrono, eis in obs:
            md.add_observation(np.array([k]), chrono, eis, group_id="g")
        md.score_group_data_badness("g", ["T"])
        out[f"data.{kind}.t"], out[f"data.{kind}.f"] = np.linspace(0, 1, 200), obs[0][2][0]
        out[f"data.{kind}.has_chrono"] = np.array([c is not None for _, c, _ in obs])
        out[f"data.{kind}.i"] = np.stack([c[1] if c is not None else np.full(200, np.nan) for _, c, _ in obs])
        out[f"data.{kind}.v"] = np.stack([c[2] if c is not None else np.full(200, np.nan) for _, c, _ in obs])
        out[f"data.{kind}.z"] = np.stack([e[1] for _, _, e in obs])
        out[f"data.{kind}.badness"] = md.obs_data_badness.copy()
        assert np.all(np.isfinite(md.obs_data_badness)) and np.argmax(md.obs_data_badness) == 5

    for n in util.SEGMENT_LENGTHS:
        for kind in ("plain", "nan", "equal", "zeros"):
            seg = util.segment(n, kind)
            if kind != "nan":
                out[f"pct.{n}.{kind}.percentile"] = np.percentile(seg, util.WHOLE_Q)
            out[f"pct.{n}.{kind}.nanpercentile"] = np.nanpercentile(seg, util.WHOLE_Q)
            out[f"pct.{n}.{kind}.nanmedian"] = np.array(np.nanmedian(seg))
    for name in util.ROW_CASES:
        a = util.row_case(name)
        out[f"pct.{name}.nanpercentile"] = np.nanpercentile(a, util.ROW_Q, axis=1).T
        out[f"pct.{name}.nanmedian"] = np.nanmedian(a, axis=1)

    np.savez_compressed(util.GOLDEN, **out)
    print(f"wrote {util.GOLDEN}: {len(out)} arrays, {os.path.getsize(util.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
