"""GPU: the posterior of the distribution of phasances on the device (hipdrt_plan_dop_posterior, hipdrt_plan_dop_cov;
csrc/predict.hip: scale_p_kernel, dop_band_kernel in front of and behind the posterior chain of csrc/plan_post.hip).

1. the chain alone through its hook (hipdrt_debug_dop_posterior) on matrices of known condition with per-member scales over four
   decades, against the extended-precision statement of tests/dop_posterior_util.py: every variance inside the derived bound, the
   packed image after the scaling bit for bit (padding included), the marker borders (the hook raises);
2. what a scaling kernel gets wrong: unit scales against hipdrt_debug_posterior bit for bit, shared against tiled scales, a member
   alone, 257 members, an indefinite P, the full matrix, the refusals;
3. fits of the fixtures' measurements against the reference's recorded run (tools/make_dop_posterior_golden.py);
4. a solve_rp batch, every member against the numpy statement (models/response.py: dop_cov_rows) fed its own P and scales, and
   against the same member fitted alone (same bits); a member whose P is not positive definite; a batch with a member without data.

Bound of 1 and 2 (and of 4, with kappa_2 of the member's own P): dop_posterior_util.bound -- posterior_util's
C_BOUND (n + 16) u kappa_2 plus 2 sqrt(n) u kappa_2 for the two roundings of every scaled entry; nothing in it is taken from the kernel.  Bound of 3: the project's parity contract, 1e-7 (variances
relative to the row's largest variance, bands relative to the largest |mu|); tests/dop_posterior_bounds.json records what a GPU run
measured (label -> [measured, bound = 20 x measured rounded up to 1 / 2 / 5 x 10^k, at least 1e-12 and at most 1e-7]).
Every numerical check prints its figure before it asserts."""
import json
import os
import warnings

import numpy as np
import pytest

import dop_posterior_util as du
import gram_util as gu
import posterior_util as pu
from conftest import GOLDEN, ROOT, parity

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(gu.extended_dtype() is None, reason="no extended type on this platform")]

WANT = ("var", "status", "ppk")


@pytest.fixture(scope="module")
def ctx():
    from hipdrt import _ffi
    return _ffi.get_context(0)


# ---- 1. the chain alone ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", du.SHAPES, ids=lambda s: f"n{s[0]}")
def test_chain_alone_variances_and_packed_image(ctx, shape):
    n, ds, dz = shape
    for neval in du.NEVALS:
        m, rows, refs = du.get_case(n, ds, dz, neval)
        out = ctx.debug_dop_posterior(m["P"], rows, ds, m["dsv"], want=WANT)       # (raises when a border changed)
        assert out["status"].tolist() == [0] * du.B, (shape, neval, out["status"])
        assert np.all(out["var"] >= 0.0)
        worst = max(du.var_ratio(out["var"][b], refs[b], n, m["kappa"][b]) for b in range(du.B))
        print(f"n {n} block [{ds}, {ds + dz}) neval {neval}: kappa_2(SPS) up to {m['kappa'].max():.3g}, worst deviation / bound {worst:.2e}")
        assert worst <= 1.0, (shape, neval, worst)
        # the image: fl(fl(P_ij s_i) s_j) on the lower tiles, and the padding exactly as the packing left it
        for b in range(du.B):
            np.testing.assert_array_equal(out["ppk"][b], du.scaled_image(m["P"][b], m["s"][b]))
    assert not np.array_equal(out["var"][0], out["var"][1])                      # (the members are different problems)


# ---- 2. what a scaling kernel gets wrong ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(23, 2, 13), (70, 5, 50), (600, 3, 50)], ids=lambda s: f"n{s[0]}")
def test_unit_scales_change_no_bit(ctx, shape):
    n, ds, dz = shape
    m, rows, _ = du.get_case(n, ds, dz, 17)
    want = ("var", "status", "tail", "bex")
    plain = ctx.debug_posterior(m["P"], rows, ds, want=want)
    unit = ctx.debug_dop_posterior(m["P"], rows, ds, np.ones((du.B, dz)), want=want + ("ppk",))
    for k in want:
        np.testing.assert_array_equal(unit[k], plain[k], err_msg=k)
    for b in range(du.B):
        np.testing.assert_array_equal(unit["ppk"][b], gu.pack_tiles(m["P"][b], n, fill=0.0))
    p1 = ctx.debug_posterior(m["P"], rows, ds, cov_member=1, want=("var", "status", "cov"))
    u1 = ctx.debug_dop_posterior(m["P"], rows, ds, np.ones(dz), cov_member=1, want=("var", "status", "cov"))
    for k in ("var", "status", "cov"):
        np.testing.assert_array_equal(u1[k], p1[k], err_msg=k)


def test_shared_and_tiled_scales_and_a_member_alone(ctx):
    n, ds, dz = 70, 5, 50
    m, rows, _ = du.get_case(n, ds, dz, 40)
    batch = ctx.debug_dop_posterior(m["P"], rows, ds, m["dsv"], want=WANT)
    # one shared vector, and the same vector given per member
    shared = ctx.debug_dop_posterior(m["P"], rows, ds, m["dsv"][1], want=WANT)
    tiled = ctx.debug_dop_posterior(m["P"], rows, ds, np.tile(m["dsv"][1], (du.B, 1)), want=WANT)
    for k in WANT:
        np.testing.assert_array_equal(shared[k], tiled[k], err_msg=k)
    np.testing.assert_array_equal(shared["var"][1], batch["var"][1])
    assert not np.array_equal(shared["var"][0], batch["var"][0])
    # a shared P under per-member scales: every member its own image
    sp = ctx.debug_dop_posterior(m["P"][0], rows, ds, m["dsv"], want=WANT)
    for b in range(du.B):
        np.testing.assert_array_equal(sp["ppk"][b], du.scaled_image(m["P"][0], m["s"][b]))
    np.testing.assert_array_equal(sp["var"][0], batch["var"][0])
    # the single-member form: strides 0, member b's own scale row
    for b in (0, 2):
        one = ctx.debug_dop_posterior(m["P"], rows, ds, m["dsv"], cov_member=b, want=WANT)
        assert one["status"].tolist() == [0]
        np.testing.assert_array_equal(one["var"][0], batch["var"][b])
        np.testing.assert_array_equal(one["ppk"][0], batch["ppk"][b])
        alone = ctx.debug_dop_posterior(m["P"][b], rows, ds, m["dsv"][b], want=WANT)
        np.testing.assert_array_equal(alone["var"][0], batch["var"][b])


def test_257_members_keep_their_own_scale_rows(ctx):
    n, ds, dz, nb = 23, 2, 13, 257
    m, rows, _ = du.get_case(n, ds, dz, 17)
    dsv = du.make_dsv(nb, dz, 4242)
    out = ctx.debug_dop_posterior(m["P"][0], rows, ds, dsv, want=WANT)
    assert not out["status"].any()
    for b in (0, 255, 256):
        s = du.scale_vector(n, ds, dsv[b])
        np.testing.assert_array_equal(out["ppk"][b], du.scaled_image(m["P"][0], s))
        kappa = du.kappa_of(du.scaled_ext(m["P"][0], s))
        ref = du.reference(du.scaled_ext(m["P"][0], s), pu.full_rows(rows, n, ds), kappa)
        r = du.var_ratio(out["var"][b], ref, n, kappa)
        print(f"member {b} of 257: deviation / bound {r:.2e}")
        assert r <= 1.0
        np.testing.assert_array_equal(ctx.debug_dop_posterior(m["P"][0], rows, ds, dsv[b])["var"][0], out["var"][b])


def indefinite(P, k):
    """P with its k-th Cholesky pivot turned into -1 (tests/test_gpu_posterior.py, section j)"""
    L = np.linalg.cholesky(P)
    Q = P.copy()
    Q[k, k] = np.sum(L[k, :k] ** 2) - 1.0
    return Q


@pytest.mark.parametrize("k", [0, 20, 69])
def test_an_indefinite_p_is_reported_and_stays_with_its_member(ctx, k):
    n, ds, dz = 70, 5, 50
    m, rows, _ = du.get_case(n, ds, dz, 17)
    good = ctx.debug_dop_posterior(m["P"], rows, ds, m["dsv"])
    P = m["P"].copy()
    P[1] = indefinite(P[1], k)               # (a congruence keeps the inertia: S P S is as indefinite as P)
    bad = ctx.debug_dop_posterior(P, rows, ds, m["dsv"])
    assert bad["status"].tolist() == [0, -1, 0] and np.all(np.isnan(bad["var"][1]))
    np.testing.assert_array_equal(bad["var"][[0, 2]], good["var"][[0, 2]])
    one = ctx.debug_dop_posterior(P, rows, ds, m["dsv"], cov_member=1, want=("var", "status", "cov"))
    assert one["status"].tolist() == [-1] and np.all(np.isnan(one["cov"])) and np.all(np.isnan(one["var"]))


@pytest.mark.parametrize("shape", [(70, 5, 50), (600, 3, 50)], ids=lambda s: f"n{s[0]}")
def test_full_covariance_of_one_member(ctx, shape):
    n, ds, dz = shape
    m, rows, refs = du.get_case(n, ds, dz, 17, True)
    scale = np.array([1.0, 1.7, 1.0])
    out = ctx.debug_dop_posterior(m["P"], rows, ds, m["dsv"], cov_member=1, scale=scale, want=("var", "status", "cov"))
    assert out["status"].tolist() == [0]
    ref = dict(var=refs[1]["var"] * 1.7, cov=refs[1]["cov"] * 1.7)
    r = du.cov_ratio(out["cov"], ref, n, m["kappa"][1])
    print(f"n {n}: cov worst deviation / bound {r:.2e}")
    assert r <= 1.0
    np.testing.assert_array_equal(out["cov"], out["cov"].T)
    assert np.all(np.abs(np.diag(out["cov"]) - out["var"][0]) <= 2 * (n + 2) * du.U * out["var"][0])


def test_hook_refusals(ctx):
    from hipdrt._ffi import HipDrtError
    n, ds, dz = 23, 2, 13
    m, rows, _ = du.get_case(n, ds, dz, 16)
    P, dsv = m["P"], m["dsv"]
    neg, inf, nan = dsv.copy(), dsv.copy(), dsv.copy()
    neg[2, 3], inf[0, 0], nan[1, 12] = -1.0, np.inf, np.nan
    zero = dsv.copy()
    zero[0, 5] = 0.0
    calls = dict(
        block_past_n=lambda: ctx.debug_dop_posterior(P, rows[:, :5], 11, dsv, col_offset=2),
        block_start_negative=lambda: ctx.debug_dop_posterior(P, rows, -1, dsv, col_offset=2),
        dop_size_zero=lambda: ctx.debug_dop_posterior(P, rows, ds, np.ones((du.B, 0)), col_offset=2),
        negative_scale=lambda: ctx.debug_dop_posterior(P, rows, ds, neg),
        zero_scale=lambda: ctx.debug_dop_posterior(P, rows, ds, zero),
        infinite_scale=lambda: ctx.debug_dop_posterior(P, rows, ds, inf),
        nan_scale=lambda: ctx.debug_dop_posterior(P, rows, ds, nan),
    )
    for what, call in calls.items():
        with pytest.raises(HipDrtError, match="error -1"):
            call()
        print("refused:", what)
    assert ctx.debug_dop_posterior(P, rows, ds, dsv)["status"].tolist() == [0, 0, 0]


# ---- 3. fits against the reference's run ---------------------------------------------------------------------------------------------
def fitted(name):
    from hipdrt import synth
    from hipdrt.models import DRT
    g = np.load(os.path.join(GOLDEN, f"refrun_dop_posterior_{name}.npz"))
    drt = DRT(fit_dop=True, warn=False)
    if name.startswith("golden71"):
        e = np.load(os.path.join(GOLDEN, "ref_test_drt_fit_eis.npz"))
        drt.fit_eis(np.asarray(e["freq"], dtype=float), np.asarray(e["z"], dtype=complex))
    else:
        drt.fit_hybrid(*synth.hybrid_measurement(seed=0), **(dict(solve_rp=True) if name.endswith("_solverp") else {}))
    return drt, g


def ref_parity(label, got, ref, scale):
    """conftest.parity against the reference's recorded values: the bound of tests/dop_posterior_bounds.json, never above the parity
    contract of 1e-7, and 1e-7 for a label not measured yet"""
    with open(os.path.join(ROOT, "tests", "dop_posterior_bounds.json")) as f:
        entry = json.load(f).get(label)
    return parity(label, got, ref, bound=1e-7 if entry is None else min(1e-7, float(entry[1])), label=label, scale=scale)


@pytest.mark.parametrize("name", ["golden71_dop", "hybrid_s0_dop", "hybrid_s0_dop_solverp"])
def test_fit_against_the_reference_run(name):
    drt, g = fitted(name)
    nu = g["nu"]
    for order in (0, 1, 2):
        for norm in (0, 1):
            tag = f"o{order}_n{norm}"
            var, ok = drt.estimate_dop_var_batch(nu=nu, order=order, normalize=bool(norm))
            assert ok.tolist() == [True] and np.all(var >= 0)
            ref_parity(f"{name}.var_{tag}", var[0], g[f"var_{tag}"], float(np.max(g[f"var_{tag}"])))
            lo, hi = drt.predict_dop_ci(nu=nu, order=order, normalize=bool(norm))
            peak = float(np.max(np.abs(g[f"mu_{tag}"])))
            ref_parity(f"{name}.lo_{tag}", lo, g[f"lo_{tag}"], peak)
            ref_parity(f"{name}.hi_{tag}", hi, g[f"hi_{tag}"], peak)
    lo, hi, ok, info = drt.predict_dop_ci_batch(quantiles=tuple(g["q2"]), return_info=True)
    peak = float(np.max(np.abs(g["mu_o0_n0"])))
    np.testing.assert_array_equal(info["nu"], nu)                         # nu=None: predict_dop's grid for mean and sigma
    ref_parity(f"{name}.lo_q2", lo[0], g["lo_q2"], peak)
    ref_parity(f"{name}.hi_q2", hi[0], g["hi_q2"], peak)
    ref_parity(f"{name}.sigma_q2", info["sigma"][0] ** 2, g["var_o0_n0"], float(np.max(g["var_o0_n0"])))
    assert np.array_equal(info["mu"], drt.predict_dop_batch()) and info["status"].tolist() == [0] and ok.tolist() == [True]
    for tag, grid in (("basis", None), ("nu7", g["nu7"])):
        for norm in (0, 1):
            cov = drt.estimate_dop_cov(nu=grid, normalize=bool(norm))
            ref = g[f"cov_{tag}_n{norm}"]
            ref_parity(f"{name}.cov_{tag}_n{norm}", cov, ref, float(np.max(np.abs(ref))))
    cov = drt.estimate_dop_cov(var_floor=float(g["var_floor"]))
    ref_parity(f"{name}.cov_basis_floor", cov, g["cov_basis_floor"], float(np.max(np.abs(g["cov_basis_floor"]))))
    assert np.min(np.diag(cov)) == float(g["var_floor"])
    # an unsorted grid comes back in the caller's order
    nu7u = np.array([0.9, -1.0, 0.0, -0.45, 0.5, 1.0, -0.8])
    covu = drt.estimate_dop_cov(nu=nu7u)
    order7 = np.argsort(nu7u)
    assert np.array_equal(covu[np.ix_(order7, order7)], drt.estimate_dop_cov(nu=g["nu7"]))
    # the existing prediction keeps its refusal of derivative orders
    with pytest.raises(NotImplementedError, match="order"):
        drt.predict_dop(order=1)


def test_entry_point_refusals():
    from hipdrt import _ffi, synth
    from hipdrt.models import DRT
    meas = synth.hybrid_measurement(seed=0)
    drt = DRT(fit_dop=True, warn=False)
    drt.fit_hybrid(*meas)
    plan, bn, eps = drt._plan, drt.basis_nu, drt.nu_epsilon
    with pytest.raises(_ffi.HipDrtError, match="error -1.*prediction description is missing"):
        plan.dop_posterior([0.0, 0.5], bn, eps)
    drt._set_predict_desc(plan)
    for bad in (dict(nu=[0.5, 0.0]), dict(order=3), dict(order=-1)):
        kw = dict(nu=[0.0, 0.5], order=0)
        kw.update(bad)
        with pytest.raises(_ffi.HipDrtError, match="error -1"):
            plan.dop_posterior(kw["nu"], bn, eps, order=kw["order"])
        with pytest.raises(_ffi.HipDrtError, match="error -1"):
            plan.dop_cov(0, kw["nu"], bn, eps, order=kw["order"])
    with pytest.raises(_ffi.HipDrtError, match="error -1.*out of range"):
        plan.dop_cov(1, [0.0, 0.5], bn, eps)
    pr = drt._prep
    for v in (-1.0, 0.0, np.inf, np.nan):
        dsv = np.array(pr["dop_scale_vector"], dtype=float)[None, :].copy()
        dsv[0, 7] = v
        plan.set_predict_desc(-1, -1, -1, 1.0, 1.0, [pr["coefficient_scale"]], dop_scale_vector=dsv,
                              v_baseline_scale=pr["v_baseline_scale"], response_signal_scale=[pr["response_signal_scale"]],
                              scaled_response_offset=[pr["scaled_response_offset"]])
        with pytest.raises(_ffi.HipDrtError, match="error -1.*dop_scale_vector must be finite and positive"):
            plan.dop_posterior([0.0, 0.5], bn, eps)
        with pytest.raises(_ffi.HipDrtError, match="error -1.*dop_scale_vector must be finite and positive"):
            plan.dop_cov(0, [0.0, 0.5], bn, eps)
        # the mean alone factorises nothing and reads no reciprocal
        mu, lo, hi, var, status = plan.dop_posterior([0.0, 0.5], bn, eps, want_var=False)
        assert lo is None and var is None and status.tolist() == [0]
    drt._set_predict_desc(plan)
    assert plan.dop_posterior([0.0, 0.5], bn, eps)[4].tolist() == [0]
    # a plan without a DOP block
    nodop = DRT(warn=False)
    nodop.fit_hybrid(*meas)
    nodop._set_predict_desc(nodop._plan)
    with pytest.raises(_ffi.HipDrtError, match="error -1.*DOP block"):
        nodop._plan.dop_posterior([0.0, 0.5], np.zeros(0), eps)
    with pytest.raises(RuntimeError, match="fit_dop=True"):
        nodop.predict_dop_ci_batch()


# ---- 4. a batch with per-member scales -------------------------------------------------------------------------------------------------
I_STEPS = (1e-3, 0.5e-3, 2e-3)


def test_solve_rp_batch_every_member_against_the_statement_with_its_own_scales(ctx):
    from hipdrt import synth
    from hipdrt.models import DRT, response
    ms = [synth.hybrid_measurement(seed=b, jitter=True, i_step=I_STEPS[b]) for b in range(3)]
    args = (ms[0][0], [m[1] for m in ms], [m[2] for m in ms], ms[0][3])
    batch = DRT(fit_dop=True, warn=False)
    res = batch.fit_hybrid_batch(*args, [m[4] for m in ms], solve_rp=True)
    assert (res["status"] >= 0).all()
    preps = batch._last_prepared[0]
    dsv = np.array([pr["dop_scale_vector"] for pr in preps])
    assert not np.array_equal(dsv[0], dsv[1]) and not np.array_equal(dsv[0], dsv[2])
    nu = np.linspace(-1.0, 1.0, 41)
    a, e = preps[0]["dop"]
    n = batch._plan.n
    for order in (0, 2):
        var, ok = batch.estimate_dop_var_batch(nu=nu, order=order)
        assert ok.all() and np.all(var >= 0)
        bm = ctx.func_eval_matrix(batch.basis_nu, nu, batch.nu_epsilon, order=order)
        for b in range(3):
            P = batch._plan.p_matrix(b)
            want = np.diag(response.dop_cov_rows(P, a, dsv[b], preps[b]["coefficient_scale"], bm))
            kappa = du.kappa_of(P)
            err = np.max(np.abs(var[b] - want) / (du.bound(n, kappa) * np.abs(want)))
            print(f"order {order} member {b}: kappa_2(P) {kappa:.3g}, deviation / bound {err:.2e}")
            assert err <= 1.0
        assert not np.allclose(var[0], var[1], rtol=1e-3) and not np.allclose(var[1], var[2], rtol=1e-3)
        if order == 0:
            var0 = var
    # a member fitted alone gives the row it gives inside the batch
    single = DRT(fit_dop=True, warn=False)
    single.fit_hybrid(*ms[1], solve_rp=True)
    assert np.array_equal(res["x_dop"][1], single.fit_parameters["x_dop"])
    v1, ok1 = single.estimate_dop_var_batch(nu=nu)
    dev = np.max(np.abs(v1[0] - var0[1]) / var0[1])
    print(f"member 1 alone against the batch: {dev:.2e}")
    assert np.array_equal(v1[0], var0[1])
    lo, hi, okb = batch.predict_dop_ci_batch(nu=nu)
    lo1, hi1 = single.predict_dop_ci(nu=nu)
    assert np.array_equal(lo[1], lo1) and np.array_equal(hi[1], hi1)
    cov1 = batch.estimate_dop_cov(nu=nu, b=1)
    assert np.array_equal(cov1, single.estimate_dop_cov(nu=nu))
    assert np.all(np.abs(np.diag(cov1) - var0[1]) <= 2 * (n + 2) * du.U * var0[1])
    # a P that is not positive definite -- member 1's penalty strengths turned negative on the device: NaN band and ok False for that
    # member with a valid mean, (None, None) with upstream's warning from the single forms, the neighbours' bits unchanged
    from hipdrt import _ffi
    rho = np.array(res["rho"], dtype=float)
    assert rho.shape == (3, 3) and np.all(rho > 0)
    bad_rho = rho.copy()
    bad_rho[1] = -1e3 * rho[1]
    batch._plan.set_state(rho=bad_rho)
    lob, hib, okb, info = batch.predict_dop_ci_batch(nu=nu, return_info=True)
    assert okb.tolist() == [True, False, True] and info["status"][1] == _ffi.PREDICT_NOT_PD
    assert np.isnan(lob[1]).all() and np.isnan(hib[1]).all() and np.isnan(info["sigma"][1]).all()
    assert np.array_equal(info["mu"], batch.predict_dop_batch(nu=nu)) and np.isfinite(info["mu"]).all()
    assert np.array_equal(lob[[0, 2]], lo[[0, 2]]) and np.array_equal(hib[[0, 2]], hi[[0, 2]])
    assert batch.estimate_dop_var_batch(nu=nu)[1].tolist() == [True, False, True]
    with pytest.warns(UserWarning, match="Singular P matrix - could not obtain covariance estimate"):
        assert batch.predict_dop_ci(nu=nu, b=1) == (None, None)
    with pytest.warns(UserWarning, match="Singular P matrix - could not obtain covariance estimate"):
        assert batch.estimate_dop_cov(nu=nu, b=1) is None
    batch._plan.set_state(rho=rho)
    assert np.array_equal(batch.estimate_dop_var_batch(nu=nu)[0], var0)


def test_failed_member_gives_nan_rows_and_leaves_the_others_bits():
    """a member without data (a solve_rp batch refuses such a member before the fit, so the batch is fitted without it)"""
    from hipdrt import synth
    from hipdrt.models import DRT
    ms = [synth.hybrid_measurement(seed=b, jitter=True) for b in range(3)]
    args = (ms[0][0], [m[1] for m in ms], [m[2] for m in ms], ms[0][3])
    nu = np.linspace(-1.0, 1.0, 41)
    good, bad = DRT(fit_dop=True, warn=False), DRT(fit_dop=True, warn=False)
    good.fit_hybrid_batch(*args, [m[4] for m in ms])
    var, ok = good.estimate_dop_var_batch(nu=nu)
    lo, hi, okc = good.predict_dop_ci_batch(nu=nu)
    assert ok.all() and okc.all() and np.isfinite(var).all() and np.isfinite(lo).all() and np.isfinite(hi).all()
    z_bad = [ms[0][4], np.full_like(ms[1][4], np.nan), ms[2][4]]
    with np.errstate(all="ignore"):
        resb = bad.fit_hybrid_batch(*args, z_bad)
        varb, okb = bad.estimate_dop_var_batch(nu=nu)
        lob, hib, okd = bad.predict_dop_ci_batch(nu=nu)
    assert resb["status"][1] < 0 and okb.tolist() == [True, False, True] and okd.tolist() == [True, False, True]
    assert np.isnan(varb[1]).all() and np.isnan(lob[1]).all() and np.isnan(hib[1]).all()
    assert np.array_equal(varb[[0, 2]], var[[0, 2]]) and np.array_equal(lob[[0, 2]], lo[[0, 2]]) and np.array_equal(hib[[0, 2]], hi[[0, 2]])
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with np.errstate(all="ignore"):
            assert bad.predict_dop_ci(nu=nu, b=1) == (None, None)
            assert bad.estimate_dop_cov(nu=nu, b=1) is None
    assert sum("Singular P matrix" in str(x.message) for x in w) == 2
    assert np.array_equal(bad.estimate_dop_cov(nu=nu, b=2), good.estimate_dop_cov(nu=nu, b=2))
