"""GPU: peak finding of a fitted batch on the device (csrc/peaks.hip; hipdrt_plan_find_peaks, hipdrt_debug_find_peaks) and the DRT
methods on top (find_peaks_batch, find_peaks, peak_prob_batch, curv_prob_batch).

1. the kernel alone (hipdrt_debug_find_peaks) against hipdrt.models.peaks on rows of small integers, integer heights and
   prominences and variances that are powers of four: every comparison and the one subtraction of the rule are exact, so all
   integer outputs, heights and prominences compare with assert_array_equal; probabilities at 1e-13 (the kernel's erfc is the
   device library's, the statement's math.erfc);
2. adversarial rows; position independence; the refusals of the hook;
3. the whole chain on a fitted batch against the statement applied to the rows downloaded from the same plan;
4. the chain against the reference's recorded run (tools/make_peaks_golden.py);
5. a spectrum alone and inside a batch gives the same bits; a failed fit; the refusals of the methods.

Tolerances that are not exact.
 - The automatic prominence 0.05 np.std(fxx) + 5e-3: the kernel sums per thread and then over a fixed tree, numpy pairwise.  On
   integer rows the sum of the row, the mean and every squared deviation are the same bits in both; only the order of the sum of
   squared deviations differs: (n + 8) u relative (Higham, Accuracy and Stability of Numerical Algorithms, 4.2).  The rows' prominences are integers, so the
   discrete results agree as long as the threshold keeps 1e-9 from an integer, which the tests assert on the statement's value.
 - In 1 the probabilities' arguments min_prom / (sigma sqrt 2) take the values k / (2^j sqrt 2), k <= 6, j <= 2: distinct values
   differ by at least 0.17 and stay below 4.3, so distinct probabilities differ by more than 1e-9 and none rounds to 1: ties are
   exact ties in both implementations and the k-th largest is the same peak.
 - In 3 sigma is recovered from the band, (hi - lo) / (s_hi - s_lo): the two roundings of mu + s sigma leave sigma with a relative
   error of at most 4 u max(|lo|, |hi|) / ((s_hi - s_lo) sigma), squaring it and taking the root again add 4 u, and 1e-12 is the
   RTOL at which test_gpu_predict.py ties the band to the variance path (here the factorisation is fed both orders' rows at once).
   A probability 1 - c erfc(a / (sigma sqrt 2)), c <= 1, moves by at most (2 / sqrt pi) x exp(-x^2) <= 0.49 times the relative
   error of sigma (twice that for c = 1/2 doubled, as in curv_prob); 1e-13 covers erfc itself.  extend_var copies a variance, and
   with it its error, to other grid points, so the largest error of the row is taken (function prob_bound).  Nothing in the
   bound is measured from the kernel."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, parity

from hipdrt.models import peaks

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
FREQ71 = np.logspace(6, -1, 71)
INT_KEYS = ("peak_sign", "keep", "left_bases", "right_bases")
COMBOS = [(s, m) for s in (1, -1, 0) for m in (0, 1, 2)]


@pytest.fixture(scope="module")
def ctx():
    from hipdrt import _ffi
    return _ffi.get_context(0)


def integer_rows(rng, B, n):
    """(fxx, f, var_fxx, var_f): small integers (plateaus, ties, zeros of f) and variances 1, 4, 16"""
    return (rng.integers(-3, 4, (B, n)).astype(float), rng.integers(-2, 3, (B, n)).astype(float),
            4.0 ** rng.integers(0, 3, (B, n)), 4.0 ** rng.integers(0, 3, (B, n)))


def run_and_compare(ctx, rows, search, method, **kw):
    """the kernel on the rows against the statement, row by row; kw: the statement's keywords (None / 0 = automatic / off)"""
    from hipdrt import _ffi
    fxx, f, vxx, vf = rows
    opts = _ffi.peak_opts(search=search, method=method, **kw)
    out = ctx.debug_find_peaks(fxx, f, vxx, vf, opts)
    auto = kw.get("prominence") is None and method == 0
    for b in range(fxx.shape[0]):
        ref = peaks.find_peaks_dense(fxx[b], f[b], vxx[b], vf[b], search=search, method=method,
                                     **{k: (v if v is not None else None) for k, v in kw.items()})
        tag = f"search {search} method {method} row {b} {kw}"
        if auto:
            t = ref["used_prominence"]
            assert abs(t - round(t)) > 1e-9, "the test's own row puts the automatic threshold on an integer"
            np.testing.assert_allclose(out["used_prominence"][b], t, rtol=(fxx.shape[1] + 8) * U, atol=0, err_msg=tag)
        else:
            assert out["used_prominence"][b] == ref["used_prominence"], tag
        for k in INT_KEYS:
            np.testing.assert_array_equal(out[k][b], ref[k], err_msg=f"{k} {tag}")
        assert out["count"][b] == ref["count"], tag
        np.testing.assert_array_equal(out["heights"][b], ref["heights"], err_msg=tag)
        np.testing.assert_array_equal(out["prominences"][b], ref["prominences"], err_msg=tag)
        np.testing.assert_allclose(out["probs"][b], ref["probs"], rtol=0, atol=1e-13, err_msg=tag)
        if method == 2:
            np.testing.assert_allclose(out["peak_prob"][b], ref["peak_prob"], rtol=0, atol=1e-13, err_msg=tag)
            np.testing.assert_allclose(out["curv_prob"][b], ref["curv_prob"], rtol=0, atol=1e-13, err_msg=tag)
    return out


# ---- 1. the kernel alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("neval", [1, 2, 3, 4, 63, 64, 65, 255, 256, 257, 1025, 2048])
def test_kernel_alone_on_integer_rows(ctx, neval):
    rng = np.random.default_rng(1000 + neval)
    big = neval > 257            # (the statement's walks are Python loops, quadratic on such rows: one spectrum, fewer options)
    rows = integer_rows(rng, 1 if big else 3, neval)
    for search, method in COMBOS:
        run_and_compare(ctx, rows, search, method)                                   # automatic thresholds
        if not big:
            run_and_compare(ctx, rows, search, method, height=1.0, prominence=2.0, prob_thresh=0.3)
    if neval >= 4:
        li, ri = neval // 4, neval - 1 - neval // 4
        for search in (1, 0):
            for k in ((2,) if big else (1, 2, 10 * neval)):                          # ties are everywhere on such rows
                run_and_compare(ctx, rows, search, 1, height=0.0, prominence=1.0, num_peaks=k, ext_left=li, ext_right=ri)
            if big:
                continue
            run_and_compare(ctx, rows, search, 1, height=0.0, prominence=1.0, fxx_var_floor=4.0, prob_thresh=0.3)
            run_and_compare(ctx, rows, search, 2, ext_left=li, ext_right=ri, fxx_var_floor=4.0)
            run_and_compare(ctx, rows, search, 2, ext_left=ri, ext_right=li)         # crossed bounds: the right one is clamped first


@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("neval", [65, 257])
def test_kernel_alone_batch_sizes(ctx, B, neval):
    rows = integer_rows(np.random.default_rng(7 * B + neval), B, neval)
    for search, method in COMBOS:
        run_and_compare(ctx, rows, search, method)
    run_and_compare(ctx, rows, 0, 1, height=0.0, prominence=1.0, num_peaks=2)


# ---- 2. adversarial rows, position, refusals -----------------------------------------------------------------------------------
def adversarial_rows(n=300):
    rows = []
    v = np.zeros(n); v[60:69] = 2; v[250:263] = 3; v[100] = 1                       # plateaus across lane 63|64 and thread 255|256
    rows.append(v)
    v = np.zeros(n); v[n - 5:n - 1] = 2; v[40:45] = 1                                # a plateau ending at n - 2: a peak
    rows.append(v)
    v = np.zeros(n); v[n - 5:n] = 2; v[40:45] = 1                                    # ... ending at n - 1: none
    rows.append(v)
    v = np.zeros(n); v[1] = 3; v[n - 2] = 2                                          # peaks at index 1 and n - 2
    rows.append(v)
    rows.append(np.tile([0.0, 1.0], n // 2))                                         # alternating: the most peaks a row can hold
    rows.append(np.tile([2.0, -1.0, 1.0, -2.0], n // 4))
    rows.append(np.full(n, 2.0))                                                     # constant
    v = np.abs(np.arange(n) - 150) % 7.0; v[150] = 50                                # the highest peak's walks cover the whole row
    rows.append(v)
    v = np.zeros(n); v[::10] = -3; v[5::10] = 1; v[155] = 4                          # equal minima on both sides of every peak
    rows.append(v)
    return -np.array(rows)                                                           # (search = 1 looks at -fxx)


def test_adversarial_rows(ctx):
    fxx = adversarial_rows()
    rng = np.random.default_rng(5)
    _, f, vxx, vf = integer_rows(rng, *fxx.shape)
    for search, method in COMBOS:
        run_and_compare(ctx, (fxx, f, vxx, vf), search, method)
        run_and_compare(ctx, (fxx, f, vxx, vf), search, method, height=1.0, prominence=1.0)
    out = run_and_compare(ctx, (fxx, f, vxx, vf), 1, 0, height=0.0, prominence=0.0)
    assert out["count"].tolist()[:5] == [3, 2, 1, 2, 149] and out["count"][6] == 0
    assert out["peak_sign"][0].nonzero()[0].tolist() == [64, 100, 256]
    assert (out["left_bases"][7, 150], out["right_bases"][7, 150]) == (143, 157)     # the nearest of the equal minima
    # the largest row every mode must hold, alternating: 1023 peaks in one pass, neighbouring peaks in two
    # (peak heights 1 .. 5 in turn, so that the statement's walks stay short)
    big = np.zeros((1, 2048)); big[0, 1::2] = -(1.0 + np.arange(1024) % 5)
    _, f, vxx, vf = integer_rows(rng, 1, 2048)
    for search in (1, 0):
        for method in (0, 1, 2):
            out = run_and_compare(ctx, (big, f, vxx, vf), search, method, height=0.0, prominence=1.0,
                                  num_peaks=3 if method == 1 else None)
            # one pass: every odd sample but the last; two: the odd ones where f > 0 and the even interior ones where f < 0
            want = 1023 if search else int((f[0, 1:2047:2] > 0).sum() + (f[0, 2:2047:2] < 0).sum())
            assert method != 0 or out["count"][0] == want, (search, method)


def test_position_in_the_batch_does_not_change_the_bits(ctx):
    from hipdrt import _ffi
    rng = np.random.default_rng(11)
    n = 257
    batch = [rng.normal(size=(37, n)), rng.normal(size=(37, n)), rng.random((37, n)) + 0.1, rng.random((37, n)) + 0.1]
    for search, method, kw in ((1, 0, {}), (0, 0, {}), (0, 1, dict(num_peaks=2, ext_left=20, ext_right=200)), (1, 2, {})):
        opts = _ffi.peak_opts(search=search, method=method, **kw)
        many = ctx.debug_find_peaks(*batch, opts)
        for b in (0, 36):
            one = ctx.debug_find_peaks(*[r[b:b + 1] for r in batch], opts)
            for k, v in one.items():
                assert np.array_equal(v[0], many[k][b], equal_nan=True), (k, b, search, method)
        assert np.isfinite(many["used_prominence"]).all() and (many["count"] > 0).all()


def test_hook_refusals(ctx):
    from hipdrt import _ffi
    fxx, f, vxx, vf = integer_rows(np.random.default_rng(3), 2, 40)
    with pytest.raises(_ffi.HipDrtError, match="LDS"):                               # nothing is launched
        ctx.debug_find_peaks(np.zeros((1, 6000)), np.zeros((1, 6000)), np.ones((1, 6000)), np.ones((1, 6000)),
                             _ffi.peak_opts(method=2))
    for bad in (np.nan, np.inf):
        for k in range(4):
            rows = [fxx.copy(), f.copy(), vxx.copy(), vf.copy()]
            rows[k][1, 7] = bad
            with pytest.raises(_ffi.HipDrtError, match="non-finite"):
                ctx.debug_find_peaks(*rows, _ffi.peak_opts(search=0, method=2))
    with pytest.raises(_ffi.HipDrtError, match="f rows"):
        ctx.debug_find_peaks(fxx, None, vxx, vf, _ffi.peak_opts(search=0))
    with pytest.raises(_ffi.HipDrtError, match="var_fxx"):
        ctx.debug_find_peaks(fxx, f, None, None, _ffi.peak_opts(method=1))
    for kw in (dict(search=2), dict(method=3), dict(num_peaks=-1), dict(ext_left=40), dict(ext_right=-2), dict(height=np.inf)):
        with pytest.raises(_ffi.HipDrtError, match="invalid argument"):
            ctx.debug_find_peaks(fxx, f, vxx, vf, _ffi.peak_opts(**kw))


# ---- 3. the whole chain against the statement on downloaded rows ---------------------------------------------------------------------
@pytest.fixture(scope="module")
def fit37():
    from hipdrt import synth
    from hipdrt.models import DRT
    z = synth.zarc2_batch(FREQ71, 37, first_seed=900)
    drt = DRT(warn=False)
    res = drt.fit_eis_batch(FREQ71, z)
    assert (res["status"] >= 0).all()
    return drt, z, res


@pytest.fixture(scope="module")
def rows37(fit37):
    """f, fxx (normalised, as find_peaks evaluates them) and the two variances before extend_var, downloaded once"""
    from hipdrt.models import predict
    drt = fit37[0]
    tau = drt.get_tau_eval(10)
    q = (0.025, 0.975)
    s_lo, s_hi = predict.n_sigma(q)
    out = dict(tau=tau, ext=drt._extend_var_indices(tau))
    for name, order in (("f", 0), ("fxx", 2)):
        out[name] = drt.predict_drt_batch(tau=tau, order=order, normalize=True, sign=1)
        lo, hi, ok = drt.predict_drt_ci_batch(tau=tau, order=order, normalize=True, sign=1, quantiles=q)
        assert ok.all()
        sigma = (hi - lo) / (s_hi - s_lo)
        out[f"var_{name}"] = sigma ** 2
        rel = 4 * U * np.maximum(np.abs(lo), np.abs(hi)) / ((s_hi - s_lo) * sigma) + 4 * U + 1e-12      # relative error of sigma
        out[f"rel_{name}"] = rel.max(axis=1)
    return out


def on_a_threshold(fxx, f, search, height, prominence, probs=None, prob_thresh=None):
    """the margin condition, on the statement's own rows: some candidate (a local maximum of a pass) is decided by a test it sits
    on -- it is within 1 % of its height or prominence threshold, or (two passes) its |f| is below 1e-6 of max |f|, and no other
    test rejects it clearly; or a peak's probability is within 1 % of the probability threshold"""
    fmax = np.abs(f).max()
    for s in ((search,) if search else (-1, 1)):
        idx, info = peaks.find_peaks_1d(-s * fxx)
        h, p = info["peak_heights"], info["prominences"]
        out = (h < height - 0.01 * abs(height)) | (p < prominence - 0.01 * abs(prominence))
        inside = (h > height + 0.01 * abs(height)) & (p > prominence + 0.01 * abs(prominence))
        if search == 0:
            out |= s * f[idx] < -1e-6 * fmax
            inside &= s * f[idx] > 1e-6 * fmax
        if (~out & ~inside).any():
            return True
    return probs is not None and bool((np.abs(np.asarray(probs) - prob_thresh) <= 0.01 * abs(prob_thresh)).any())


def prob_bound(rel_sigma):
    return 0.49 * rel_sigma + 1e-13


@pytest.mark.parametrize("sign", [1, 0])
def test_chain_against_the_statement_on_downloaded_rows(fit37, rows37, sign):
    drt, r = fit37[0], rows37
    tau, (li, ri), B = r["tau"], r["ext"], 37
    search = sign                                    # a nonneg fit: sign 1 searches one pass, sign 0 two
    skipped = on_kth = 0
    results = {m: drt.find_peaks_batch(tau=tau, sign=sign, method=kw["method"], num_peaks=kw.get("num_peaks"), return_info=True)
               for m, kw in (("thresh", dict(method="thresh")), ("prob", dict(method="prob")), ("prob2", dict(method="prob", num_peaks=2)))}
    pp, cp = drt.peak_prob_batch(tau=tau, sign=sign), drt.curv_prob_batch(tau=tau, sign=sign)
    assert pp.shape == cp.shape == (B, len(tau))
    for b in range(B):
        f, fxx, vxx, vf = r["f"][b], r["fxx"][b], r["var_fxx"][b], r["var_f"][b]
        prom_t, _ = peaks.auto_thresholds(fxx, "thresh")
        if on_a_threshold(fxx, f, search, 0.0, prom_t) or on_a_threshold(fxx, f, search, 1e-3, 5e-3):
            skipped += 1
            continue
        ref_p = peaks.find_peaks_row(fxx, f, vxx, search=search, method="prob", ext_left=li, ext_right=ri)
        if on_a_threshold(fxx, f, search, 1e-3, 5e-3, ref_p[2]["probs"], 0.25):
            skipped += 1
            continue
        for m, kw in (("thresh", dict(method="thresh")), ("prob", dict(method="prob")), ("prob2", dict(method="prob", num_peaks=2))):
            kept, idx, info, _, _ = peaks.find_peaks_row(fxx, f, vxx, search=search, ext_left=li, ext_right=ri, **kw)
            peak_tau, tau_out, got_idx, got_info = results[m]
            if m == "prob2" and len(info["probs"]) > 2:
                top = np.sort(info["probs"])[::-1]
                if top[1] - top[2] <= 0.01 * top[1]:      # the probability threshold IS the second largest: same margin
                    on_kth += 1
                    continue
            np.testing.assert_array_equal(got_idx[b], kept, err_msg=f"{m} {b}")
            np.testing.assert_array_equal(peak_tau[b], tau[kept])
            np.testing.assert_array_equal(got_info[b]["peak_heights"], info["peak_heights"])
            np.testing.assert_array_equal(got_info[b]["prominences"], info["prominences"])
            np.testing.assert_array_equal(got_info[b]["left_bases"], info["left_bases"])
            np.testing.assert_array_equal(got_info[b]["right_bases"], info["right_bases"])
            if "probs" in info:
                assert (np.abs(got_info[b]["probs"] - info["probs"]) <= prob_bound(r["rel_fxx"][b])).all(), (m, b)
        vxx_c, vf_c = peaks.extend_var(vxx, li, ri), peaks.extend_var(vf, li, ri)
        bound = prob_bound(max(r["rel_fxx"][b], r["rel_f"][b]))
        ref_pp = peaks.peak_prob_row(f, fxx, vf_c, vxx_c, search=search)
        np.testing.assert_array_equal(np.flatnonzero(pp[b]), np.flatnonzero(ref_pp))
        assert (np.abs(pp[b] - ref_pp) <= bound).all(), b
        assert (np.abs(cp[b] - peaks.curv_prob_row(f, fxx, vf_c, vxx_c)) <= 2 * bound).all(), b
    print(f"sign {sign}: {skipped} of {B} spectra sit on a threshold and are left out ({100 * skipped / B:.0f} %), "
          f"{on_kth} more for num_peaks alone")
    assert skipped + on_kth <= 0.1 * B
    # the single-spectrum form is a member of the batch
    one = drt.find_peaks(tau=tau, sign=sign, return_info=True, b=5)
    assert np.array_equal(one[0], results["thresh"][0][5]) and np.array_equal(one[2], results["thresh"][2][5])
    assert np.array_equal(drt.find_peaks(tau=tau, sign=sign, b=5), one[0])


# ---- 4. the chain against the reference's recorded run ----------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["plain", "nn", "sneg"])
def test_fit_against_the_reference_run(tag):
    from hipdrt.models import DRT
    g = np.load(os.path.join(GOLDEN, "refrun_peaks_golden71x91.npz"))
    fit_kw, pk_kw = {"plain": (dict(), dict(sign=1, normalize=True)), "nn": (dict(nonneg=False), dict(sign=1, normalize=True)),
                     "sneg": (dict(series_neg=True), dict(sign=0, normalize=False))}[tag]
    drt = DRT()
    drt.fit_eis(g["freq"], g["z"], **fit_kw)
    tau = g[f"{tag}_tau"]
    np.testing.assert_allclose(drt.get_tau_eval(10), tau, rtol=1e-13)
    scale = float(np.abs(g[f"{tag}_fxx"]).max())
    for m, kw in (("thresh", dict(method="thresh")), ("prob", dict(method="prob")), ("prob1", dict(method="prob", num_peaks=1))):
        peak_tau, tau_out, idx, info = drt.find_peaks(return_info=True, **pk_kw, **kw)
        np.testing.assert_array_equal(idx, g[f"{tag}_{m}_idx"], err_msg=m)
        np.testing.assert_array_equal(peak_tau, tau_out[idx])
        assert len(info["peak_heights"]) == len(g[f"{tag}_{m}_peak_heights"]), m
        parity(f"{m}_heights", info["peak_heights"], g[f"{tag}_{m}_peak_heights"], default=1e-7, scale=scale)
        parity(f"{m}_prominences", info["prominences"], g[f"{tag}_{m}_prominences"], default=1e-7, scale=scale)
        if kw["method"] == "prob":
            parity(f"{m}_probs", info["probs"], g[f"{tag}_{m}_probs"], default=1e-6, scale=1.0)
    parity("peak_prob", drt.peak_prob_batch(**pk_kw)[0], g[f"{tag}_peak_prob"], default=1e-6, scale=1.0)
    parity("curv_prob", drt.curv_prob_batch(**pk_kw)[0], g[f"{tag}_curv_prob"], default=1e-6, scale=1.0)


# ---- 5. position independence of the chain, failure rows, refusals --------------------------------------------------------------------
def test_alone_and_in_a_batch_give_the_same_bits(fit37):
    from hipdrt import _ffi
    from hipdrt.models import DRT
    drt, z, res = fit37
    ln_tau = np.log(drt.get_tau_eval(10))
    li, ri = drt._extend_var_indices(drt.get_tau_eval(10))
    all_opts = [_ffi.peak_opts(search=1, method=0), _ffi.peak_opts(search=0, method=0),
                _ffi.peak_opts(search=1, method=1, num_peaks=2, ext_left=li, ext_right=ri),
                _ffi.peak_opts(search=0, method=2, ext_left=li, ext_right=ri, normalize=0)]
    many = [drt._plan.find_peaks(ln_tau, o) for o in all_opts]
    one = DRT(warn=False)
    for b in (0, 16, 36):
        r1 = one.fit_eis_batch(FREQ71, z[b:b + 1])
        assert np.array_equal(r1["x"][0], res["x"][b]), "the fit itself differs between batch sizes: nothing to compare"
        for o, m in zip(all_opts, many):
            single = one._plan.find_peaks(ln_tau, o)
            for k, v in single.items():
                assert np.array_equal(v[0], m[k][b], equal_nan=True), (k, b, o.method, o.search)


def test_failed_fit_gives_no_peaks_nan_rows_and_a_negative_status():
    from hipdrt import _ffi, synth
    from hipdrt.models import DRT
    z = synth.zarc2_batch(FREQ71, 5, first_seed=300)
    zbad = z.copy()
    zbad[2] = np.nan
    good, bad = DRT(warn=False), DRT(warn=False)
    good.fit_eis_batch(FREQ71, z)
    res = bad.fit_eis_batch(FREQ71, zbad)
    assert res["status"][2] < 0
    ln_tau = np.log(bad.get_tau_eval(10))
    for method in (0, 1, 2):
        o = _ffi.peak_opts(method=method)
        a, c = bad._plan.find_peaks(ln_tau, o), good._plan.find_peaks(ln_tau, o)
        assert a["status"][2] < 0 and a["count"][2] == 0 and not a["peak_sign"][2].any() and not a["keep"][2].any()
        assert (a["left_bases"][2] == -1).all() and (a["right_bases"][2] == -1).all() and np.isnan(a["used_prominence"][2])
        for k in ("heights", "prominences", "probs") + (("peak_prob", "curv_prob") if method == 2 else ()):
            assert np.isnan(a[k][2]).all(), k
        for k, v in a.items():
            assert np.array_equal(np.delete(v, 2, axis=0), np.delete(c[k], 2, axis=0)), k
    assert [len(p) for p in bad.find_peaks_batch()][2] == 0


def test_refusals(fit37):
    from hipdrt import _ffi
    drt = fit37[0]
    with pytest.raises(ValueError, match="Invalid method"):
        drt.find_peaks_batch(method="best")
    for name, value in (("distance", 3), ("width", 2), ("wlen", 11), ("threshold", 0.1), ("plateau_size", 2), ("x", np.ones(3))):
        with pytest.raises(NotImplementedError, match=name):
            drt.find_peaks_batch(**{name: value})
    with pytest.raises(NotImplementedError, match="x"):
        drt.find_peaks(x=np.ones(3))
    with pytest.raises(NotImplementedError, match="p_matrix"):
        drt.find_peaks_batch(method="prob", p_matrix=np.eye(3))
    with pytest.raises(_ffi.HipDrtError, match="LDS"):
        drt._plan.find_peaks(np.linspace(-20, 5, 6000), _ffi.peak_opts(method=2))
    with pytest.raises(_ffi.HipDrtError, match="eval_sign"):
        drt._plan.find_peaks(np.log(drt.get_tau_eval(10)), _ffi.peak_opts(eval_sign=0))
