"""Device map prediction (csrc/map_predict.hip: hipdrt_map_predict) behind Context.map_predict and DRTMD.predict_*, against the
reference's fixture tests/golden/refrun_map_predict.npz (tools/make_map_predict_golden.py).

  peak indices, zeros, NaNs     exact, against the fixture
  filtered x, variances         max |difference| / max |reference| against the fixture, asserted at the bound of
                                tests/map_predict_bounds.json ("device": [measured on the GPU, bound = the next 1-2-5 step at least
                                10 x above]); only the bound is read here
  f, fxx                        against x_filtered @ E.T in numpy with E downloaded from Context.func_eval_matrix (the basis evaluation is
                                not part of the figure), by element at (nsup + 8) 2^-52 (|x| @ |E|.T): nsup products and sums of the
                                MFMA chain, each rounded once, and 8 for numpy's own pairwise sums -- derived, no stored number
  probabilities                 against the statement evaluated on the device's own f, fxx and variance rows, atol 1e-13 (the figure
                                tests/test_gpu_peaks.py holds the same arithmetic to)
A row predicted alone and inside the 70-row map, and a slab of 2 * 4 + 1 rows against the full map: the same bits."""
import numpy as np
import pytest

import map_predict_util as util
from hipdrt.mapping import predict
from hipdrt.mapping.store import DRTMD
from hipdrt.models import peaks

pytestmark = pytest.mark.gpu

G = util.load()
CASES = util.case_names(G)
EVERY = ("x", "f", "fxx", "f_var", "fxx_var", "peak_prob", "curv_prob")


@pytest.fixture(scope="module")
def ctx():
    from hipdrt import _ffi
    return _ffi.get_context(0)


def check(label, actual, ref):
    err = util.deviation(actual, ref)
    entry = util.bounds()["device"].get(label)
    print(f"map_predict device {label}: measured {err:.3e} bound {entry[1] if entry else None}")
    assert entry is not None, f"{label}: no bound in tests/map_predict_bounds.json yet (measured {err:.3e})"
    assert err <= entry[1], (label, err, entry)


def same_decisions(got, ref, what):
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN entries differ"
    assert np.array_equal(got == 0, ref == 0), f"{what}: peak indices / zeros differ"


def grids(case):
    eps = float(G[f"{case}.epsilon"])
    return dict(ln_tau_sup=np.log(G[f"{case}.tau_supergrid"]), ln_tau_eval=np.log(G[f"{case}.tau_eval"]), epsilon=eps,
                basis_area=float(np.sqrt(np.pi) / eps))


_RUNS = {}


def run(ctx, case, cfg):
    """the whole chain for one peak configuration with the fixture's variances passed as given (computed once per module)"""
    if (case, cfg) not in _RUNS:
        nonneg, kw = util.peak_kw(cfg)
        sp = kw["peak_spread_sigma"]
        spread = {} if sp is None else dict(spread_table=predict.gaussian_tables((sp,))[0], spread_factor=predict.spread_factor(sp))
        _RUNS[case, cfg] = ctx.map_predict(G[f"{case}.x"], normalize=True, filter_tables=predict.filter_tables(kw["ndfilter"], kw.get("filter_kw")),
                                           f_var=G[f"{case}.f_var_in"], fxx_var=G[f"{case}.fxx_var_in"],
                                           search=predict.search_kind(nonneg, kw["sign"]), want=EVERY, **spread, **grids(case))
    return _RUNS[case, cfg]


@pytest.mark.parametrize("case", CASES)
def test_filtered_x_against_the_fixture(ctx, case):
    check(f"x.{case}.default", run(ctx, case, "filt_spread")["x"], G[f"{case}.x.default"])
    if f"{case}.x.sigma2" in G.files:
        check(f"x.{case}.sigma2", run(ctx, case, "sigma2")["x"], G[f"{case}.x.sigma2"])


@pytest.mark.parametrize("case", [c for c in CASES if util.has_ext(c)])
def test_stored_variances_clamped_and_filtered_against_the_fixture(ctx, case):
    ext = predict.clamp_index_rows(G[f"{case}.tau_eval"], G[f"{case}.tau_supergrid"], util.tau_indices(G, case))
    for tag, nd in (("ext", False), ("extfilt", True)):
        if f"{case}.var.{tag}.f" not in G.files:
            continue
        for want in (("f_var", "fxx_var"), ("f_var", "fxx_var", "curv_prob")):      # the clamp kernel, and the clamp inside map_prob_kernel
            res = ctx.map_predict(G[f"{case}.x"], filter_tables=predict.filter_tables(nd), f_var=G[f"{case}.f_var_raw"],
                                  fxx_var=G[f"{case}.fxx_var_raw"], var_stored=True, ext=ext, want=want, **grids(case))
            check(f"var.{case}.{tag}", np.stack([res["f_var"], res["fxx_var"]]),
                  np.stack([G[f"{case}.var.{tag}.f"], G[f"{case}.var.{tag}.fxx"]]))
    given = run(ctx, case, "plain")                                               # variances passed by the caller: as given
    assert np.array_equal(given["f_var"], G[f"{case}.f_var_in"], equal_nan=True)
    assert np.array_equal(given["fxx_var"], G[f"{case}.fxx_var_in"], equal_nan=True)


@pytest.mark.parametrize("cfg", ["plain", "sigma2"])
@pytest.mark.parametrize("case", CASES)
def test_f_and_fxx_within_the_derived_bound(ctx, case, cfg):
    res, g = run(ctx, case, cfg), grids(case)
    x = res["x"]
    nsup = x.shape[1]
    for name, order in (("f", 0), ("fxx", 2)):
        E = ctx.func_eval_matrix(g["ln_tau_sup"], g["ln_tau_eval"], g["epsilon"], order)
        ok = ~np.isnan(x).any(axis=1)
        assert np.isnan(res[name][~ok]).all() and ok.any()
        want, bound = x[ok] @ E.T, (nsup + 8) * 2.0 ** -52 * (np.abs(x[ok]) @ np.abs(E).T)
        excess = np.abs(res[name][ok] - want) / bound
        print(f"map_predict device {name}.{case}.{cfg}: largest |difference| / bound {excess.max():.3f}")
        assert np.all(excess <= 1.0), (case, cfg, name, float(excess.max()))


@pytest.mark.parametrize("cfg", list(util.PEAK_CONFIGS))
@pytest.mark.parametrize("case", CASES)
def test_probabilities_equal_the_statement_on_the_devices_own_rows(ctx, case, cfg):
    nonneg, kw = util.peak_kw(cfg)
    res = run(ctx, case, cfg)
    same_decisions(res["peak_prob"], G[f"{case}.peak.{cfg}"], f"{case}.peak.{cfg}")
    with np.errstate(invalid="ignore", divide="ignore"):
        pk = predict.peak_rows(res["f"], res["fxx"], res["f_var"], res["fxx_var"], predict.search_kind(nonneg, kw["sign"]), 1e-3, 5e-3)
        if kw["peak_spread_sigma"] is not None:
            pk = predict.spread_statement(pk, kw["peak_spread_sigma"])
        want = pk * np.sign(res["f"])
        curv = peaks.curv_prob_row(res["f"], res["fxx"], res["f_var"], res["fxx_var"])
    same_decisions(res["peak_prob"], want, f"{case}.peak.{cfg} (statement)")
    np.testing.assert_allclose(res["peak_prob"], want, rtol=0, atol=1e-13)
    np.testing.assert_allclose(res["curv_prob"], curv, rtol=0, atol=1e-13)
    np.testing.assert_allclose(res["peak_prob"], G[f"{case}.peak.{cfg}"], rtol=0, atol=1e-9)      # (a coarse look at the reference's values)


@pytest.mark.parametrize("case", CASES)
def test_curv_prob_unnormalised_against_the_fixture(ctx, case):
    for cfg, kw in util.CURV_CONFIGS.items():
        if f"{case}.curv.{cfg}" not in G.files:
            continue
        res = ctx.map_predict(G[f"{case}.x"], filter_tables=predict.filter_tables(kw["ndfilter"]), f_var=G[f"{case}.f_var_in"],
                              fxx_var=G[f"{case}.fxx_var_in"], want=EVERY[:5] + ("curv_prob",), **grids(case))
        with np.errstate(invalid="ignore", divide="ignore"):
            want = peaks.curv_prob_row(res["f"], res["fxx"], res["f_var"], res["fxx_var"])
        np.testing.assert_allclose(res["curv_prob"], want, rtol=0, atol=1e-13)
        assert np.array_equal(np.isnan(res["curv_prob"]), np.isnan(G[f"{case}.curv.{cfg}"]))
        np.testing.assert_allclose(res["curv_prob"], G[f"{case}.curv.{cfg}"], rtol=0, atol=1e-9)


@pytest.mark.parametrize("case", CASES)
def test_store_methods_run_the_same_chain(ctx, case):
    """DRTMD.predict_* on the device give the bits of the Context call they are built on"""
    psi, vf, vxx = util.psi_of(G, case), G[f"{case}.f_var_in"], G[f"{case}.fxx_var_in"]
    for cfg in util.PEAK_CONFIGS:
        nonneg, kw = util.peak_kw(cfg)
        md = util.make_store(G, case, DRTMD, nonneg=nonneg)
        got = md.predict_peak_prob(psi, f_var=vf, fxx_var=vxx, **kw)
        same_decisions(got, G[f"{case}.peak.{cfg}"], f"store {case}.peak.{cfg}")
        assert np.array_equal(got, run(ctx, case, cfg)["peak_prob"], equal_nan=True)
    md = util.make_store(G, case, DRTMD)
    assert np.array_equal(md.predict_x(psi, normalize=True, ndfilter=True), run(ctx, case, "filt_spread")["x"], equal_nan=True)
    assert np.array_equal(md.predict_drt(psi, tau=G[f"{case}.tau_eval"], x=run(ctx, case, "plain")["x"], order=2),
                          run(ctx, case, "plain")["fxx"], equal_nan=True)
    curv = md.predict_curv_prob(psi, f_var=vf, fxx_var=vxx, ndfilter=True)
    if f"{case}.curv.filt" in G.files:
        np.testing.assert_allclose(curv, G[f"{case}.curv.filt"], rtol=0, atol=1e-9)
    if util.has_ext(case):
        # the stored rows: clamp and filter inside the one call, against the variance methods and the caller's-variances path
        got = md.predict_peak_prob(psi, ndfilter=True)
        vfp, vxxp = md.predict_drt_var(np.arange(len(psi)), order=0, ndfilter=True), md.predict_drt_var(np.arange(len(psi)), order=2, ndfilter=True)
        if f"{case}.var.extfilt.f" in G.files:
            check(f"var.{case}.extfilt", np.stack([vfp, vxxp]), np.stack([G[f"{case}.var.extfilt.f"], G[f"{case}.var.extfilt.fxx"]]))
        assert np.array_equal(got, md.predict_peak_prob(psi, f_var=vfp, fxx_var=vxxp, ndfilter=True), equal_nan=True)
        want = md.predict_peak_prob(psi, ndfilter=True, statement=True)
        same_decisions(got, want, f"store {case} stored variances")
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-9)
    # a callable filter runs on the host; a device-backed one from hipdrt.filters included
    from hipdrt.filters import ndfilters
    host = md.predict_x(psi, normalize=True, ndfilter=True, filter_func=ndfilters.gaussian_filter, filter_kw={"sigma": (1, 0)})
    check(f"x.{case}.default", host, G[f"{case}.x.default"])


def test_a_row_alone_gives_the_bits_it_has_inside_the_map(ctx):
    full = run(ctx, "a70", "plain")
    for r in (0, 33, 69):
        one = ctx.map_predict(G["a70.x"][r:r + 1], normalize=True, f_var=G["a70.f_var_in"][r:r + 1], fxx_var=G["a70.fxx_var_in"][r:r + 1],
                              want=EVERY, **grids("a70"))
        for name in EVERY:
            assert np.array_equal(one[name][0], full[name][r]), (r, name)
        assert (one["peak_prob"] != 0).any()


def test_a_slab_around_a_row_gives_that_rows_bits_from_the_full_map(ctx):
    """the default psi filter (sigma 1, truncate 4) reaches 4 rows: a slab of 2 * 4 + 1 rows holds everything row r depends on"""
    full = run(ctx, "a70", "filt_spread")
    sp = predict.gaussian_tables((1.5,))[0]
    for r in (4, 35, 65):
        sl = slice(r - 4, r + 5)
        slab = ctx.map_predict(G["a70.x"][sl], normalize=True, filter_tables=predict.filter_tables(True), f_var=G["a70.f_var_in"][sl],
                               fxx_var=G["a70.fxx_var_in"][sl], spread_table=sp, spread_factor=predict.spread_factor(1.5), want=EVERY,
                               **grids("a70"))
        for name in EVERY:
            assert np.array_equal(slab[name][4], full[name][r]), (r, name)


def test_an_evaluation_grid_beyond_lds_is_refused(ctx):
    n = 3200
    tau = np.logspace(-3, 1, n)
    with pytest.raises(NotImplementedError, match="neval <= 3145"):
        ctx.map_predict(G["a3.x"], np.log(G["a3.tau_supergrid"]), np.log(tau), float(G["a3.epsilon"]), f_var=np.ones((3, n)),
                        fxx_var=np.ones((3, n)), want=("curv_prob",))
    assert ctx.map_predict(G["a3.x"], np.log(G["a3.tau_supergrid"]), np.log(tau), float(G["a3.epsilon"]), want=("f",))["f"].shape == (3, n)


def test_a_small_real_map_keeps_its_variances_and_predicts_its_peaks():
    """8 EIS observations on the 41-point frequency grid of tests/test_gpu_mapping.py, store_eval_var=True"""
    import os
    from conftest import GOLDEN
    from hipdrt import synth
    g = np.load(os.path.join(GOLDEN, "refrun_drtmd_mixed16.npz"))
    freq = np.logspace(5, 0, 41)
    md = DRTMD(g["tau_supergrid"], psi_dim_names=["T"], store_eval_var=True, warn=False)
    for k in range(8):
        md.add_observation([300.0 + k], None, (freq, synth.zarc2_spectrum(freq, 300 + k, jitter=True)))
    assert np.isnan(md.obs_f_var).all()
    md.fit_all()
    assert md.obs_fit_status.all()
    tau = md.get_tau_eval(10)
    for order, stored in ((0, md.obs_f_var), (2, md.obs_fxx_var)):
        var, ok = md.drt1d.estimate_distribution_var_batch(tau=tau, order=order)
        assert ok.all() and np.all(stored >= 0) and np.any(stored > 0)        # (0: evaluation points the basis does not reach)
        assert np.array_equal(stored, var)
    psi = md.obs_psi[[5, 0, 3, 7, 1, 2, 4, 6]]
    got = md.predict_peak_prob(psi, ndfilter=True, peak_spread_sigma=1)
    want = md.predict_peak_prob(psi, ndfilter=True, peak_spread_sigma=1, statement=True)
    same_decisions(got, want, "real map")
    assert (got != 0).any()
    np.testing.assert_allclose(got, want, rtol=0, atol=1e-13 * max(1.0, float(np.abs(want).max())))
    check("x.real_map", md.predict_x(psi, normalize=True, ndfilter=True), md.predict_x(psi, normalize=True, ndfilter=True, statement=True))
