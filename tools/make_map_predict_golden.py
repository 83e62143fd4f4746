"""Generate the map-prediction fixture tests/golden/refrun_map_predict.npz (build container only: imports the reference through the
shims of oracle/refshim, like tools/make_map_badness_golden.py, and needs scipy).

No fit is run: obs_x, obs_tau_indices and fit_kw are set on the reference's DRTMD, and the variances come from
predict_drt_var(obs_index, x_cov=<synthetic SPD blocks>).  Recorded per case of tests/map_predict_util.CASES (rows x nsup x neval:
1 x 9 x 11, 3 x 37 x 41, 23 x 37 x 41 with an all-NaN row, a row whose right == nsup and rows with left > 0, 70 x 130 x 131):
  x, tau_supergrid, tau_eval, epsilon, tau_indices         the map (coefficients rounded to float32 values)
  x.default, x.sigma2                                      predict_x(normalize=True, ndfilter=True[, filter_kw sigma (2, 0.5)])
  f_var_raw, fxx_var_raw                                   predict_drt_var(extend_var=False): the chain's raw input
  var.ext.f / .fxx, var.extfilt.f / .fxx                   predict_drt_var(extend_var=True, ndfilter=False / True)
  f_var_in, fxx_var_in                                     the raw rows rounded to float32 values: passed as f_var= / fxx_var=
  peak.<config>, curv.<config>                             predict_peak_prob / predict_curv_prob with those passed
The row whose right == nsup raises IndexError upstream; its expectation is upstream's with right - 1, which reads the same grid point
as the extension.  The one-decade case has its clamp beyond the evaluation grid: no var.ext* there.

The file is only written when no decision hinges on a rounding: no height or prominence within 1e-9 relative of its threshold, no
plateau in fxx, no |f| below 1e-12, no variance <= 0; and it holds a row with no peak, one with three or more, and a negative-f peak
under sign=0.

    python tools/make_map_predict_golden.py
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

from hybdrt.mapping.drtmd import DRTMD as RefDRTMD  # noqa: E402
from hybdrt import utils as ref_utils  # noqa: E402

import map_predict_util as util  # noqa: E402
from hipdrt.mapping import predict  # noqa: E402
from hipdrt.models import peaks  # noqa: E402


def rows_multi(func1d, axis, arrays, *args, **kwargs):
    """utils.array.apply_along_axis_multi for 2-D arrays along their last axis: upstream's copy of np.apply_along_axis calls
    ndarray.__array_prepare__, which numpy 2 no longer has (for a plain ndarray it returned its argument)"""
    arrays = [np.asarray(a) for a in arrays]
    assert axis in (-1, 1) and all(a.ndim == 2 for a in arrays)
    return np.array([func1d([a[k] for a in arrays], *args, **kwargs) for k in range(len(arrays[0]))])


if not hasattr(np.ndarray, "__array_prepare__"):
    ref_utils.array.apply_along_axis_multi = rows_multi


def f32(a):
    return np.asarray(a, dtype=np.float32).astype(np.float64)


def surface(case):
    """two drifting peaks plus one that fades out along psi (the number of peaks changes), a negative lobe in some rows"""
    rows, nsup, _ = util.CASES[case]
    psi, u = np.meshgrid(np.linspace(0, 1, rows) if rows > 1 else np.array([0.3]), np.linspace(0, 1, nsup), indexing="ij")
    w = 0.05 if nsup > 40 else 0.09
    x = np.exp(-((u - 0.25 - 0.1 * psi) / w) ** 2) + (0.4 + 0.5 * psi) * np.exp(-((u - 0.7 + 0.08 * psi) / (1.3 * w)) ** 2)
    x += 0.7 * np.maximum(0.0, 1 - 2.2 * psi) * np.exp(-((u - 0.47) / (0.8 * w)) ** 2)
    x -= 0.35 * (psi > 0.55) * np.exp(-((u - 0.9) / w) ** 2)
    x = 0.2 * x + 2e-3 * (1.2 + np.cos(7 * u + 3 * psi))
    ti = np.tile(np.array([[0, nsup - 1]]), (rows, 1))
    if case == "a23":
        x[9] = np.nan
        ti[4], ti[5], ti[12], ti[17] = (0, nsup), (3, nsup - 1), (2, nsup - 3), (4, nsup)
    if case == "a70":
        x[31] = 0.2 * np.exp(-((u[31] - 0.5) / 0.55) ** 2)            # one broad bump: no peak passes the height
        ti[3], ti[40] = (5, nsup - 2), (0, nsup)
    return f32(x), ti          # (the slots only steer the clamp: coefficients outside them stay, so that no f underflows to 0)


def synthetic_cov(case, x):
    """one SPD block per row (a Gaussian kernel between coefficients, scaled along the grid and with psi); NaN for a NaN row"""
    rows, nsup, _ = util.CASES[case]
    i = np.arange(nsup)
    kern = np.exp(-((i[:, None] - i[None, :]) / 2.5) ** 2) + 0.05 * np.eye(nsup)
    cov = np.empty((rows, nsup, nsup))
    for k in range(rows):
        g = 0.02 * (1 + 0.5 * np.sin(0.2 * i + 0.3 * k)) * (1 + 0.03 * k)
        cov[k] = kern * g[:, None] * g[None, :]
        if np.isnan(x[k]).any():
            cov[k] = np.nan
    return cov


def check_decisions(name, info, search, height, prominence, stats):
    f, fxx, vf, vxx = info["f"], info["fxx"], info["f_var"], info["fxx_var"]
    for k in range(len(f)):
        if np.isnan(f[k]).any():
            continue
        assert np.all(np.abs(f[k]) > 1e-12), f"{name} row {k}: an f within 1e-12 of 0"
        assert np.all(np.diff(fxx[k]) != 0), f"{name} row {k}: a plateau in fxx"
        assert np.all(vf[k] > 0) and np.all(vxx[k] > 0), f"{name} row {k}: a variance <= 0"
        for s in ((search,) if search != 0 else (-1, 1)):
            _, pi = peaks.find_peaks_1d(-s * fxx[k], None, None)
            assert np.all(np.abs(pi["peak_heights"] - height) > 1e-9 * height), f"{name} row {k}: a height at its threshold"
            assert np.all(np.abs(pi["prominences"] - prominence) > 1e-9 * prominence), f"{name} row {k}: a prominence at its threshold"
        idx, _, signs = peaks.search_peaks(fxx[k], f[k], search, height, prominence)
        stats["none"] |= len(idx) == 0
        stats["many"] |= len(idx) >= 3
        stats["negative"] |= search == 0 and bool(np.any(f[k][idx] < 0))


def main():
    warnings.simplefilter("ignore")
    out, stats = {}, dict(none=False, many=False, negative=False)
    for case, (rows, nsup, (lo, hi)) in util.CASES.items():
        tau = np.logspace(lo, hi, nsup)
        x, ti = surface(case)
        out[f"{case}.x"], out[f"{case}.tau_supergrid"], out[f"{case}.tau_indices"] = x, tau, ti
        G = {k: v for k, v in out.items()}

        class Files(dict):
            files = property(lambda self: list(self))

        def ref_store(nonneg=True):
            md = util.make_store(Files(G), case, RefDRTMD, nonneg=nonneg, store_eval_var=False)
            md.obs_tau_indices = [(int(l_), min(int(r_), nsup - 1)) for l_, r_ in ti]       # upstream: IndexError at right == nsup
            return md

        md = ref_store()
        psi, index = util.psi_of(G, case), np.arange(rows)
        tau_ev = md.get_tau_eval(10)
        assert len(tau_ev) == util.NEVAL[case], (case, len(tau_ev))
        out[f"{case}.tau_eval"], out[f"{case}.epsilon"] = tau_ev, np.array(md.tau_epsilon)
        skip = util.A70_SKIP if case == "a70" else ()
        out[f"{case}.x.default"] = md.predict_x(psi, normalize=True, ndfilter=True)
        if "x.sigma2" not in skip:
            out[f"{case}.x.sigma2"] = md.predict_x(psi, normalize=True, ndfilter=True, filter_kw={"sigma": (2, 0.5)})
        x_cov = synthetic_cov(case, x)
        raw = {o: md.predict_drt_var(index, tau=tau_ev, x_cov=x_cov, order=o, extend_var=False) for o in (0, 2)}
        out[f"{case}.f_var_raw"], out[f"{case}.fxx_var_raw"] = raw[0], raw[2]
        if util.has_ext(case):
            for tag, nd in (("ext", False), ("extfilt", True)):
                if f"var.{tag}" in skip:
                    continue
                for o, nm in ((0, "f"), (2, "fxx")):
                    out[f"{case}.var.{tag}.{nm}"] = md.predict_drt_var(index, tau=tau_ev, x_cov=x_cov, order=o, extend_var=True, ndfilter=nd)
                    got = predict.map_var_statement(raw[o], tau_ev, tau, [tuple(p) for p in ti], True, predict.filter_tables(nd))
                    assert util.deviation(got, out[f"{case}.var.{tag}.{nm}"]) < 1e-12, (case, tag, nm)
        vf_in, vxx_in = f32(raw[0]), f32(raw[2])
        out[f"{case}.f_var_in"], out[f"{case}.fxx_var_in"] = vf_in, vxx_in
        area = md.tau_basis_area
        for cfg in util.PEAK_CONFIGS:
            nonneg, kw = util.peak_kw(cfg)
            out[f"{case}.peak.{cfg}"] = ref_store(nonneg).predict_peak_prob(psi, f_var=vf_in, fxx_var=vxx_in, **kw)
            tabs = predict.filter_tables(kw["ndfilter"], kw.get("filter_kw"))
            got, info = predict.peak_prob_map_statement(x, vf_in, vxx_in, tau, tau_ev, float(md.tau_epsilon), area, nonneg=nonneg,
                                                        sign=kw["sign"], peak_spread_sigma=kw["peak_spread_sigma"], filter_tables=tabs,
                                                        return_info=True)
            check_decisions(f"{case}.peak.{cfg}", info, predict.search_kind(nonneg, kw["sign"]), 1e-3, 5e-3, stats)
            ref = out[f"{case}.peak.{cfg}"]
            assert np.array_equal(got == 0, ref == 0), f"{case}.{cfg}: the statement's peaks differ from the reference's"
        for cfg, kw in util.CURV_CONFIGS.items():
            if f"curv.{cfg}" not in skip:
                out[f"{case}.curv.{cfg}"] = md.predict_curv_prob(psi, f_var=vf_in, fxx_var=vxx_in, **kw)
        print(case, "peaks per row (plain):", (out[f"{case}.peak.plain"] != 0).sum(axis=1).tolist())
    assert all(stats.values()), f"row kinds missing: {stats}"
    np.savez_compressed(util.GOLDEN, **out)
    print(f"wrote {util.GOLDEN}: {len(out)} arrays, {os.path.getsize(util.GOLDEN)} bytes")


if __name__ == "__main__":
    main()
