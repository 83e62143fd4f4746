"""CPU: the numpy statement of the map-prediction chain (hipdrt.mapping.predict; DRTMD.predict_* with statement=True) against the
reference's fixture tests/golden/refrun_map_predict.npz (tools/make_map_predict_golden.py): decisions -- which indices are peaks,
zeros elsewhere, where the NaNs are -- exact, values at the bound of tests/map_predict_bounds.json ("statement": rtol 1e-12 by
element: numpy's erfc against scipy's erf, and the order of the matmul's sums); then the store's bookkeeping: psi lookup, row order,
NaN rows, the two IndexError extensions, every NotImplementedError, and that a store built without store_eval_var is today's store."""
import inspect

import numpy as np
import pytest

import map_predict_util as util
from hipdrt.mapping import predict, table
from hipdrt.mapping.store import DRTMD

G = util.load()
CASES = util.case_names(G)
RTOL = util.bounds()["statement"]["rtol"]


def close(got, ref, what):
    """decisions exact, values by element"""
    got, ref = np.asarray(got), np.asarray(ref)
    assert got.shape == ref.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(ref)), f"{what}: NaN entries differ"
    assert np.array_equal(got == 0, ref == 0), f"{what}: zero entries (the decisions) differ"
    ok = ~np.isnan(ref) & (ref != 0)
    err = float(np.max(np.abs(got[ok] - ref[ok]) / np.abs(ref[ok]))) if ok.any() else 0.0
    print(f"map_predict statement {what}: measured {err:.2e} bound {RTOL:.1e}")
    assert err <= RTOL, (what, err)


def statement_kw(case):
    return dict(tau_supergrid=G[f"{case}.tau_supergrid"], tau=G[f"{case}.tau_eval"], epsilon=float(G[f"{case}.epsilon"]),
                basis_area=float(np.sqrt(np.pi) / G[f"{case}.epsilon"]))


def test_fixture_covers_the_shapes_and_row_kinds():
    assert CASES == list(util.CASES)
    for case, (rows, nsup, _) in util.CASES.items():
        assert G[f"{case}.x"].shape == (rows, nsup) and G[f"{case}.tau_eval"].shape == (util.NEVAL[case],)
        assert np.array_equal(G[f"{case}.x"], G[f"{case}.x"].astype(np.float32).astype(float), equal_nan=True)
    ti, nsup = G["a23.tau_indices"], util.CASES["a23"][1]
    assert np.isnan(G["a23.x"]).all(axis=1).sum() == 1 and (ti[:, 1] == nsup).any() and (ti[:, 0] > 0).any()
    counts = np.concatenate([(G[f"{c}.peak.plain"] > 0).sum(axis=1) for c in CASES])
    assert (counts == 0).any() and (counts >= 3).any()
    assert any((G[f"{c}.peak.sign0"] < 0).any() for c in CASES)             # a negative-f peak under sign = 0


@pytest.mark.parametrize("case", CASES)
def test_x_statement(case):
    area = statement_kw(case)["basis_area"]
    close(predict.map_x_statement(G[f"{case}.x"], area, True, predict.filter_tables(True)), G[f"{case}.x.default"], f"{case}.x.default")
    if f"{case}.x.sigma2" in G.files:
        tabs = predict.filter_tables(True, {"sigma": (2, 0.5)})
        close(predict.map_x_statement(G[f"{case}.x"], area, True, tabs), G[f"{case}.x.sigma2"], f"{case}.x.sigma2")


@pytest.mark.parametrize("case", [c for c in CASES if util.has_ext(c)])
def test_var_statement(case):
    for tag, nd in (("ext", False), ("extfilt", True)):
        for nm in ("f", "fxx"):
            key = f"{case}.var.{tag}.{nm}"
            if key in G.files:
                got = predict.map_var_statement(G[f"{case}.{nm}_var_raw"], G[f"{case}.tau_eval"], G[f"{case}.tau_supergrid"],
                                                util.tau_indices(G, case), True, predict.filter_tables(nd))
                close(got, G[key], key)
    if case == "a23":                                                       # the clamp changes rows, the NaN row is left alone
        raw, ext = G["a23.f_var_raw"], G["a23.var.ext.f"]
        assert not np.array_equal(raw[0], ext[0]) and np.isnan(ext[9]).all()


@pytest.mark.parametrize("cfg", list(util.PEAK_CONFIGS))
@pytest.mark.parametrize("case", CASES)
def test_peak_prob_statement(case, cfg):
    nonneg, kw = util.peak_kw(cfg)
    tabs = predict.filter_tables(kw["ndfilter"], kw.get("filter_kw"))
    got = predict.peak_prob_map_statement(G[f"{case}.x"], G[f"{case}.f_var_in"], G[f"{case}.fxx_var_in"], nonneg=nonneg, sign=kw["sign"],
                                          peak_spread_sigma=kw["peak_spread_sigma"], filter_tables=tabs, **statement_kw(case))
    close(got, G[f"{case}.peak.{cfg}"], f"{case}.peak.{cfg}")


@pytest.mark.parametrize("case", CASES)
def test_curv_prob_statement(case):
    for cfg, kw in util.CURV_CONFIGS.items():
        if f"{case}.curv.{cfg}" in G.files:
            got = predict.curv_prob_map_statement(G[f"{case}.x"], G[f"{case}.f_var_in"], G[f"{case}.fxx_var_in"],
                                                  filter_tables=predict.filter_tables(kw["ndfilter"]), **statement_kw(case))
            close(got, G[f"{case}.curv.{cfg}"], f"{case}.curv.{cfg}")


# ---- the store with statement=True ----
@pytest.fixture(scope="module")
def md23():
    md = util.make_store(G, "a23", DRTMD)
    assert md.drt1d.tau_epsilon == float(G["a23.epsilon"])
    return md


def test_store_statement_equals_the_fixture(md23):
    psi = util.psi_of(G, "a23")
    assert np.array_equal(md23.get_tau_eval(10), G["a23.tau_eval"])
    close(md23.predict_x(psi, normalize=True, ndfilter=True, statement=True), G["a23.x.default"], "store x")
    close(md23.predict_drt_var(np.arange(23), order=2, ndfilter=True, statement=True), G["a23.var.extfilt.fxx"], "store var")
    close(md23.predict_drt_var(np.arange(23), tau=G["a23.tau_eval"], order=0, statement=True), G["a23.var.ext.f"], "store var ext")
    vf, vxx = G["a23.f_var_in"], G["a23.fxx_var_in"]
    got = md23.predict_peak_prob(psi, f_var=vf, fxx_var=vxx, ndfilter=True, peak_spread_sigma=1.5, statement=True)
    close(got, G["a23.peak.filt_spread"], "store peak")
    close(md23.predict_curv_prob(psi, f_var=vf, fxx_var=vxx, ndfilter=True, statement=True), G["a23.curv.filt"], "store curv")
    # a callable filter runs on the host as apply_filter runs it, and needs its keywords
    from hipdrt.filters import ndfilters
    got = md23.predict_x(psi, normalize=True, ndfilter=True, filter_func=ndfilters.gaussian_filter, filter_kw={"sigma": (1, 0)}, statement=True)
    close(got, G["a23.x.default"], "store x, callable filter")
    with pytest.raises(TypeError):
        md23.predict_x(psi, ndfilter=True, filter_func=ndfilters.gaussian_filter, statement=True)


def test_stored_variances_feed_the_probabilities(md23):
    """without f_var / fxx_var the stored raw rows take the clamp and the filter: the statement fed with the same arrays"""
    psi = util.psi_of(G, "a23")
    got = md23.predict_peak_prob(psi, ndfilter=True, statement=True)
    vf = md23.predict_drt_var(np.arange(23), order=0, ndfilter=True, statement=True)
    vxx = md23.predict_drt_var(np.arange(23), order=2, ndfilter=True, statement=True)
    want = md23.predict_peak_prob(psi, f_var=vf, fxx_var=vxx, ndfilter=True, statement=True)
    assert np.array_equal(got, want, equal_nan=True) and (got[0] != 0).any()
    got = md23.predict_curv_prob(psi, extend_var=False, statement=True)
    want = md23.predict_curv_prob(psi, f_var=md23.obs_f_var, fxx_var=md23.obs_fxx_var, statement=True)
    assert np.array_equal(got, want, equal_nan=True)


def test_psi_lookup_and_row_order(md23):
    assert md23.get_psi_index([[3.0], [0.0], [22.0], [99.0]]).tolist() == [3, 0, 22, -1]
    assert md23.get_psi_index([[3.0 * (1 + 1e-12)]]).tolist() == [3]                      # 8 significant digits
    with pytest.raises(ValueError):
        md23.validate_psi([[1.0, 2.0]])
    psi = np.array([[7.0], [2.0], [9.0], [4.0]])
    x = md23.predict_x(psi, statement=True)
    assert np.array_equal(x[:2], md23.obs_x[[7, 2]]) and np.isnan(x[2]).all()                # row 9 was never fitted: NaN
    md = util.make_store(G, "a23", DRTMD)
    md.obs_ignore_flag[4] = True
    assert np.isnan(md.predict_x(psi, statement=True)[3]).all()                              # an ignored row as well
    full = md23.predict_drt(util.psi_of(G, "a23"), statement=True)
    assert np.array_equal(md23.predict_drt(psi, statement=True)[[0, 1, 3]], full[[7, 2, 4]])
    assert full.shape == (23, 37) and md23.predict_drt(psi, tau=G["a23.tau_eval"], order=1, statement=True).shape == (4, 41)
    r_p = md23.predict_r_p(psi[:2], absolute=True, statement=True)
    assert np.allclose(r_p, np.abs(md23.obs_x[[7, 2]]).sum(axis=1) * md23.tau_basis_area, rtol=1e-15)
    assert np.allclose(md23.predict_r_p(psi[:2], normalize=True, absolute=True, statement=True), 1.0, rtol=1e-14)


def test_the_two_index_error_extensions():
    tau, sup = G["a23.tau_eval"], G["a23.tau_supergrid"]
    nsup = len(sup)
    # right == len(tau_supergrid) (upstream: IndexError) reads the last grid point
    assert predict.clamp_indices(tau, sup, (0, nsup)) == predict.clamp_indices(tau, sup, (0, nsup - 1))
    assert predict.clamp_indices(tau, sup, (0, nsup)) == (11, 30)
    # li >= len(tau) (upstream: IndexError): the ValueError of PostFitMixin._peak_ext
    with pytest.raises(ValueError, match="measured tau range ends at the last point"):
        predict.clamp_indices(G["a1.tau_eval"], G["a1.tau_supergrid"], (0, 8))
    md = util.make_store(G, "a1", DRTMD)
    with pytest.raises(ValueError, match="measured tau range ends at the last point"):
        md.predict_drt_var([0], statement=True)
    assert md.predict_drt_var([0], extend_var=False, statement=True).shape == (1, 11)


def test_what_is_not_built_says_so(md23):
    psi = util.psi_of(G, "a23")
    with pytest.raises(NotImplementedError, match="not an observed coordinate"):
        md23.predict_x([[0.5]], statement=True)
    with pytest.raises(NotImplementedError, match="percentile"):
        md23.predict_x(psi, percentile=90, statement=True)
    for call in (md23.predict_dop, md23.predict_x_cov, md23.predict_drt_cov, md23.predict_param_cov):
        with pytest.raises(NotImplementedError):
            call(psi)
    with pytest.raises(NotImplementedError, match="x_cov"):
        md23.predict_drt_var([0], x_cov=np.eye(37)[None], statement=True)
    with pytest.raises(NotImplementedError, match="get_tau_eval"):
        md23.predict_drt_var([0], tau=md23.get_tau_eval(20), statement=True)
    with pytest.raises(NotImplementedError, match="orders 0 and 2"):
        md23.predict_drt_var([0], order=1, statement=True)
    with pytest.raises(NotImplementedError, match="orders 0 and 2"):
        md23.predict_drt(psi, order=1)                                                      # (the device chain; raised on the host)
    plain = util.make_store(G, "a23", DRTMD, store_eval_var=False)
    with pytest.raises(NotImplementedError, match="store_eval_var"):
        plain.predict_drt_var([0], statement=True)
    with pytest.raises(NotImplementedError, match="store_eval_var"):
        plain.predict_peak_prob(psi, statement=True)
    assert plain.predict_peak_prob(psi, f_var=G["a23.f_var_in"], fxx_var=G["a23.fxx_var_in"], statement=True).shape == (23, 41)
    pf = DRTMD(G["a23.tau_supergrid"], psi_dim_names=["T"], fit_type="pfrt")
    pf.add_observation([0.0], None, None)
    with pytest.raises(NotImplementedError, match="pfrt"):
        pf.predict_x([[0.0]], statement=True)
    with pytest.raises(NotImplementedError, match="pfrt"):
        DRTMD(G["a23.tau_supergrid"], fit_type="pfrt", store_eval_var=True)
    with pytest.raises(ValueError, match="psi is not provided"):
        md23.predict_curv_prob(x=md23.obs_x, statement=True)


def test_store_without_the_keyword_is_todays_store():
    tau = np.logspace(-4, 1, 7)
    md, ev = DRTMD(tau, psi_dim_names=["T"]), DRTMD(tau, psi_dim_names=["T"], store_eval_var=True)
    for m in (md, ev):
        m.add_observation([1.0], None, None)
    extra = set(vars(ev)) - set(vars(md))
    assert extra == {"obs_f_var", "obs_fxx_var"} and set(vars(md)) - set(vars(ev)) == set()
    assert md.store_eval_var is False
    assert ev.obs_f_var.shape == (1, 51) and np.isnan(ev.obs_f_var).all() and np.isnan(ev.obs_fxx_var).all()
    # the rows a rank sends: the layout of pack_rows does not know the keyword
    obs_x = np.arange(6.0).reshape(2, 3)
    res = dict(obs_llh=np.ones(2), obs_rss=np.ones(2), outer_iters=np.ones(2), qp_iters_total=np.ones(2), status=np.zeros(2))
    packed = table.pack_rows(obs_x, {"R_inf": np.ones(2)}, res, False)
    assert packed.shape == (3, 3 + 1 + 5 + 2) and packed[0, :6].tolist() == [3.0, 0.0, 1.0, 2.0, 1.0, 1.0]


def test_the_gathered_rows_carry_the_variances_only_on_request():
    rng = np.random.default_rng(3)
    obs_x = rng.standard_normal((4, 5))
    res = dict(obs_llh=np.ones(4), obs_rss=np.ones(4), outer_iters=np.ones(4), qp_iters_total=np.ones(4), status=np.array([0, 0, -1, 0]),
               obs_drt_var=np.abs(obs_x), obs_drt_var_ok=np.ones(4, bool))
    special = {"R_inf": np.arange(4.0), "x_dop": rng.standard_normal((4, 3))}
    plain = table.pack_rows(obs_x, special, res, True)
    res2 = dict(res, obs_f_var=rng.random((4, 7)), obs_fxx_var=rng.random((4, 7)))
    res2["obs_f_var"][2] = np.nan
    packed = table.pack_rows(obs_x, special, res2, True)
    assert packed.shape == (5, plain.shape[1] + 14) and np.array_equal(packed[1:, :plain.shape[1]], plain[1:])
    assert packed[0, 1] == 3.0 and plain[0, 1] == 1.0 and np.array_equal(packed[0, [0, 2, 3, 4, 5, 6, 7, 8]], plain[0, [0, 2, 3, 4, 5, 6, 7, 8]])
    cols = table.unpack_block(packed)[2]
    assert np.array_equal(cols["obs_f_var"], res2["obs_f_var"], equal_nan=True) and np.array_equal(cols["obs_fxx_var"], res2["obs_fxx_var"])
    assert "obs_f_var" not in table.unpack_block(plain)[2]
    tab = table.ObsTable(4, (5,), True, dict(table.GATHER_COLUMNS, obs_f_var=(float, (7,)), obs_fxx_var=(float, (7,))))
    tab.scatter_rows(np.arange(4), packed)
    assert np.array_equal(tab.res["obs_f_var"], res2["obs_f_var"], equal_nan=True) and np.array_equal(tab.obs_x[[0, 1, 3]], obs_x[[0, 1, 3]])


def test_the_order_keyword_defaults_to_today():
    from hipdrt.matrices import basis
    from hipdrt.models import DRT
    assert inspect.signature(DRT.estimate_distribution_var_batch).parameters["order"].default == 0

    class Plan:
        def distribution_var(self, bm, batch):
            self.bm = np.array(bm)
            return np.ones((batch, len(bm))), np.zeros(batch, dtype=np.int32)

    drt = DRT(warn=False)
    drt.basis_tau, drt._plan, drt._last_batch, drt.f_fit = np.logspace(-5, 1, 31), Plan(), 2, np.logspace(4, 0, 21)
    tau = np.logspace(-5, 1, 61)
    for kw, order in (({}, 0), ({"order": 0}, 0), ({"order": 2}, 2)):
        drt.estimate_distribution_var_batch(tau=tau, **kw)
        want = basis.construct_func_eval_matrix(np.log(drt.basis_tau), np.log(tau), "gaussian", epsilon=drt.tau_epsilon, order=order)
        assert np.array_equal(drt._plan.bm, want)
