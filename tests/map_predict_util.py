"""Shared by tests/test_host_map_predict.py, tests/test_gpu_map_predict.py and tools/make_map_predict_golden.py: the cases and
configurations of the map-prediction fixture tests/golden/refrun_map_predict.npz, its loader, a store filled from it and the
bounds table tests/map_predict_bounds.json."""
import json
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
GOLDEN = os.path.join(HERE, "golden", "refrun_map_predict.npz")
BOUNDS = os.path.join(HERE, "map_predict_bounds.json")

# name -> (rows, nsup, decades of the supergrid); neval = 10 decades + 1 (get_tau_eval(10))
CASES = {"a1": (1, 9, (-2, -1)), "a3": (3, 37, (-3, 1)), "a23": (23, 37, (-3, 1)), "a70": (70, 130, (-7, 6))}
NEVAL = {"a1": 11, "a3": 41, "a23": 41, "a70": 131}

# peak_prob configurations: name -> keywords of predict_peak_prob (nonneg goes into fit_kw)
PEAK_CONFIGS = {
    "plain": dict(ndfilter=False, peak_spread_sigma=None, sign=1, nonneg=True),
    "filt_spread": dict(ndfilter=True, peak_spread_sigma=1.5, sign=1, nonneg=True),
    "sign0": dict(ndfilter=False, peak_spread_sigma=None, sign=0, nonneg=True),
    "signed_fit": dict(ndfilter=True, peak_spread_sigma=None, sign=1, nonneg=False),
    "sigma2": dict(ndfilter=True, peak_spread_sigma=None, sign=1, nonneg=True, filter_kw={"sigma": (2, 0.5)}),
}
CURV_CONFIGS = {"plain": dict(ndfilter=False), "filt": dict(ndfilter=True)}
# what the large case records (the rest is covered by the small ones; keeps the file small)
A70_SKIP = ("var.ext", "curv.plain", "x.sigma2")


def load():
    return np.load(GOLDEN, allow_pickle=False)


def case_names(G):
    return [c for c in CASES if f"{c}.x" in G.files]


def tau_indices(G, case):
    return [tuple(int(v) for v in pair) for pair in G[f"{case}.tau_indices"]]


def has_ext(case):
    """a1's basis spans one decade: the clamp's left index lies beyond the evaluation grid (upstream: IndexError)"""
    return case != "a1"


def peak_kw(cfg):
    kw = dict(PEAK_CONFIGS[cfg])
    nonneg = kw.pop("nonneg")
    return nonneg, kw


def make_store(G, case, cls, nonneg=True, store_eval_var=True, **kw):
    """a store (ours or the reference's class) that holds the case's map: observations entered in psi order"""
    x = G[f"{case}.x"]
    if store_eval_var:
        kw["store_eval_var"] = True
    md = cls(tau_supergrid=G[f"{case}.tau_supergrid"], psi_dim_names=["T"], fit_kw={"nonneg": nonneg}, **kw)
    for k in range(len(x)):
        md.add_observation(np.array([float(k)]), None, None, group_id="g")
    md.obs_x = x.copy()
    md.obs_fit_status = ~np.isnan(x).all(axis=1)
    md.obs_ignore_flag = np.zeros(len(x), bool)
    md.obs_tau_indices = tau_indices(G, case)
    if store_eval_var:
        md.obs_f_var, md.obs_fxx_var = G[f"{case}.f_var_raw"].copy(), G[f"{case}.fxx_var_raw"].copy()
    return md


def psi_of(G, case):
    return np.arange(len(G[f"{case}.x"]), dtype=float)[:, None]


def step_125(value):
    """the next 1-2-5 step at least 10 x above `value`; a measured 0 (the fixture's float32-valued inputs make the row sums, the
    clamp and scipy's own summation order exact) counts as one unit roundoff of a double, 2^-52"""
    target = 10.0 * max(float(value), 2.0 ** -52)
    k = int(np.floor(np.log10(target)))
    for m, e in ((1, k), (2, k), (5, k), (1, k + 1)):
        if float(f"{m}e{e}") >= target:
            return float(f"{m}e{e}")
    raise AssertionError


def bounds():
    with open(BOUNDS) as f:
        return json.load(f)


def deviation(actual, ref):
    """max |difference| / max |reference| over the entries where the reference is a number; NaNs must coincide"""
    actual, ref = np.asarray(actual, dtype=float), np.asarray(ref, dtype=float)
    assert actual.shape == ref.shape, (actual.shape, ref.shape)
    assert np.array_equal(np.isnan(actual), np.isnan(ref)), "NaN entries differ"
    ok = ~np.isnan(ref)
    if not ok.any():
        return 0.0
    return float(np.abs(actual[ok] - ref[ok]).max() / np.abs(ref[ok]).max())
