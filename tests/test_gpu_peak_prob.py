"""GPU: peak and trough probabilities of a fitted batch and the peak search on them (csrc/peak_prob.hip;
hipdrt_plan_peak_trough_probs, hipdrt_debug_peak_trough_probs) and the DRT methods on top (predict_peak_trough_probs,
predict_peak_prob, find_peaks_byprob and their _batch forms).

1. the kernel alone (the hook) against hipdrt.models.peaks on rows of small integers: f, fx, fxx in -3 .. 3 (zeros of f included),
   variances 1, 4, 16.  The search is checked against the statement's search applied to the KERNEL'S OWN downloaded prob row, so
   every integer output, height and prominence is exact; prob_in rows with plateaus across lanes 63|64 and threads 255|256;
2. position independence; 3. the refusals of the hook and of the entry;
4. the whole chain on 37 fitted spectra, on get_tau_eval(10) and on a 257-point grid;
5. the chain against the reference's recorded run (tools/make_peak_prob_golden.py), three fits, both bayes_cov;
6. a member alone and inside a batch; a failed fit; a prepared (hybrid) plan with row_scale; the methods' refusals and info keys.

Tolerances that are not exact.  Nothing in a bound is measured from the kernel.
 - bayes_cov = 1 on the integer rows: sigma is 1, 2 or 4, the clamp copies values, the percentiles sit at quarter-multiples of
   n - 1 between small integers and the floor is a multiple of 1/8: the sigma rows are exact (assert_array_equal), and the
   arguments of every Phi are the same bits in the kernel and in the statement (both compiled / evaluated without fused
   multiply-add).  What differs is erfc itself -- the device library's against math.erfc -- which the sibling test
   (test_gpu_peaks.py) bounds by 1e-13 per erfc-based term.  All factors lie in [0, 1], so a product's error is at most the sum of
   its factors' errors: pp = f_prob (1 term) x fx_prob (2 terms) x fxx_prob (1 term): 4e-13; tp = fx_prob (2) x (1 term): 3e-13;
   prob = pp (1 - tp): 4e-13 + 3e-13 = 7e-13.
 - bayes_cov = 0 on the integer rows: the window sums of small integers, the windowed mean, the deviations from it, their
   squares and the window sums of those (added in ascending offset by both) are the same bits.  Only np.std differs: the sum of
   the n squared deviations runs per thread and over a fixed tree in the kernel and pairwise in numpy, each within (n - 1) u of
   the exact sum of the same terms (Higham, Accuracy and Stability of Numerical Algorithms, 4.2), the division, the root (which
   halves a relative error), the product with the baseline and the final sum add a few u: sigma = filtered + baseline >= baseline
   agrees to (n + 16) u relative.  A term Phi(c - a / sigma) moves by at most |x| phi(x) <= 0.242 times the relative error of sigma
   -- the sibling's 0.49 rel(sigma) for a factor of up to two such terms -- so pp (three factors) is bounded by
   3 x 0.49 rel + 4e-13, tp (two) by 2 x 0.49 rel + 3e-13 and prob by their sum.
 - 4: the means must be the bits of predict_drt_batch.  The sigma rows against estimate_distribution_var_batch(order=k,
   extend_var=True) (root, then the statement's floor) at rtol 1e-12, the RTOL at which test_gpu_predict.py ties the variance
   paths (here the factorisation is fed three orders' rows at once).  pp, tp and prob against the statement on the downloaded means
   and the entry's OWN sigma rows: the arguments are again the same bits, the bounds those of bayes_cov = 1 above.
 - 5: parity(..., default=1e-6, scale=1.0), the tolerance test_gpu_peaks.py asserts for probabilities against the reference;
   indices and range peaks must be equal (the fixture is only written when they are decided with a margin)."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, parity

from hipdrt.models import peaks

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
FREQ71 = np.logspace(6, -1, 71)
PP_ERFC, TP_ERFC = 4e-13, 3e-13
DENSE_KEYS = ("keep", "heights", "prominences", "left_bases", "right_bases")
THRESHOLDS = ((None, None), (0.25, 0.125), (0.25, None), (None, 0.125))
ALL = ("mu", "pp", "tp", "prob", "sigma", "keep", "heights", "prominences", "left_bases", "right_bases", "count", "range_peaks")


@pytest.fixture(scope="module")
def ctx():
    from hipdrt import _ffi
    return _ffi.get_context(0)


def integer_rows(rng, B, n):
    """(f, fx, fxx, var_f, var_fx, var_fxx): small integers (zeros of f included) and variances 1, 4, 16"""
    return tuple(rng.integers(-3, 4, (B, n)).astype(float) for _ in range(3)) + tuple(4.0 ** rng.integers(0, 3, (B, n)) for _ in range(3))


def windows_of(n, rng, count=0):
    """interior, touching both ends, single-sample and empty index windows of a grid of n points, then `count` random ones"""
    win = [(n // 4, n // 2), (0, n - 1), (n // 3, n // 3), (0, -1), (n, n - 1)]
    for _ in range(count):
        lo = int(rng.integers(0, n))
        win.append((lo, int(rng.integers(lo, n))))
    return np.array(win)


def prob_bounds(rel_sigma):
    """(pp, tp, prob) absolute bounds for a relative error rel_sigma of the sigma rows (docstring)"""
    pp, tp = 3 * 0.49 * rel_sigma + PP_ERFC, 2 * 0.49 * rel_sigma + TP_ERFC
    return pp, tp, pp + tp


def check_search(out, b, search, height=None, prominence=None, windows=None):
    """the search outputs of row b against the statement's search on the kernel's own prob row: exact"""
    prob = out["prob"][b]
    if search == "thresh":
        ref = peaks.find_peaks_byprob_dense(prob, height, prominence)
        for k in DENSE_KEYS:
            np.testing.assert_array_equal(out[k][b], ref[k], err_msg=f"{k} row {b} height {height} prominence {prominence}")
        assert out["count"][b] == ref["count"]
        return ref["count"]
    np.testing.assert_array_equal(out["range_peaks"][b], peaks.find_peaks_byindex(prob, windows), err_msg=f"row {b}")
    return len(windows)


def run_and_compare(ctx, rows, bayes_cov, search="rows", height=None, prominence=None, windows=None, **kw):
    """the kernel on the rows against the statement, row by row; kw: ext_left, ext_right, sigma_floor, std_size, std_baseline"""
    from hipdrt import _ffi
    f, fx, fxx = rows[:3]
    var = rows[3:] if bayes_cov else (None, None, None)
    B, n = f.shape
    opts = _ffi.peak_prob_opts(bayes_cov=bayes_cov, search=search, height=height, prominence=prominence, **kw)
    out = ctx.debug_peak_trough_probs(f, fx, fxx, *var, opts=opts, ranges=windows)
    rel = 0.0 if bayes_cov else (n + 16) * U
    b_pp, b_tp, b_prob = prob_bounds(rel)
    found = 0
    for b in range(B):
        pp, tp, sig = peaks.peak_trough_probs_rows(f[b], fx[b], fxx[b], *[None if v is None else v[b] for v in var],
                                                   std_size=kw.get("std_size", 5), std_baseline=kw.get("std_baseline", 0.1),
                                                   floor=kw.get("sigma_floor", True), ext_left=kw.get("ext_left", -1),
                                                   ext_right=kw.get("ext_right", -1))
        tag = f"bayes_cov {bayes_cov} row {b} n {n} {kw}"
        if bayes_cov:
            np.testing.assert_array_equal(out["sigma"][:, b], sig, err_msg=tag)
        else:
            np.testing.assert_allclose(out["sigma"][:, b], sig, rtol=rel, atol=0, err_msg=tag)
        np.testing.assert_allclose(out["pp"][b], pp, rtol=0, atol=b_pp, err_msg=tag)
        np.testing.assert_allclose(out["tp"][b], tp, rtol=0, atol=b_tp, err_msg=tag)
        np.testing.assert_allclose(out["prob"][b], peaks.peak_prob_of(pp, tp), rtol=0, atol=b_prob, err_msg=tag)
        if search != "rows":
            found += check_search(out, b, search, height, prominence, windows)
    return out, found


# ---- 1. the kernel alone -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("neval", [1, 2, 3, 4, 5, 63, 64, 65, 255, 256, 257, 1024])
def test_kernel_alone_on_integer_rows(ctx, neval):
    rng = np.random.default_rng(2000 + neval)
    rows = integer_rows(rng, 1 if neval > 257 else 3, neval)
    peaks_found = 0
    for bayes_cov in (1, 0):
        for height, prominence in THRESHOLDS:
            peaks_found += run_and_compare(ctx, rows, bayes_cov, "thresh", height, prominence)[1]
        run_and_compare(ctx, rows, bayes_cov, "ranges", windows=windows_of(neval, rng))
        run_and_compare(ctx, rows, bayes_cov, "ranges", windows=windows_of(neval, rng, 59))              # 64 of them
    assert peaks_found > 0 or neval < 5                    # the comparison is not vacuous
    run_and_compare(ctx, rows, 1, sigma_floor=False)
    run_and_compare(ctx, rows, 0, std_size=3, std_baseline=0.5)
    run_and_compare(ctx, rows, 0, std_size=9, std_baseline=0.0)                     # (a window longer than a short row: reflection with period 2 n)
    if neval >= 4:
        li, ri = neval // 4, neval - 1 - neval // 4
        for floor in (True, False):
            run_and_compare(ctx, rows, 1, "thresh", ext_left=li, ext_right=ri, sigma_floor=floor)
            run_and_compare(ctx, rows, 1, "thresh", ext_left=ri, ext_right=li, sigma_floor=floor)       # crossed: the right bound is clamped first


def test_the_floor_is_active_on_the_integer_rows(ctx):
    """a row whose sigma has a few small values below median - 1.5 iqr: the floor lifts them (and nothing else)"""
    from hipdrt import _ffi
    n = 65
    rows = list(integer_rows(np.random.default_rng(8), 1, n))
    for k in (3, 4, 5):
        rows[k] = np.full((1, n), 16.0)
        rows[k][0, 10:13] = 1.0
    out, _ = run_and_compare(ctx, tuple(rows), 1)
    assert (out["sigma"][:, 0, 10:13] == 4.0).all()          # median 4, iqr 0: floor 4
    raw = ctx.debug_peak_trough_probs(*rows, opts=_ffi.peak_prob_opts(sigma_floor=False))
    assert (raw["sigma"][:, 0, 10:13] == 1.0).all()


@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("neval", [65, 257])
def test_kernel_alone_batch_sizes(ctx, B, neval):
    rng = np.random.default_rng(7 * B + neval)
    rows = integer_rows(rng, B, neval)
    for bayes_cov in (1, 0):
        run_and_compare(ctx, rows, bayes_cov, "thresh", 0.25, 0.125, ext_left=5, ext_right=neval - 9)
        run_and_compare(ctx, rows, bayes_cov, "ranges", windows=windows_of(neval, rng, 3))


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
    rows.append(np.full(n, 2.0))                                                     # constant
    v = np.abs(np.arange(n) - 150) % 7.0; v[150] = 50                                # the highest peak's walks cover the whole row
    rows.append(v)
    rows.append(np.zeros(n))                                                         # nothing positive anywhere
    return np.array(rows) / 64.0


def test_search_alone_on_given_prob_rows(ctx):
    from hipdrt import _ffi
    prob_in = adversarial_rows()
    B, n = prob_in.shape
    for height, prominence in THRESHOLDS + ((1 / 64, 1 / 64),):
        out = ctx.debug_peak_trough_probs(prob_in=prob_in, opts=_ffi.peak_prob_opts(search="thresh", height=height, prominence=prominence))
        np.testing.assert_array_equal(out["prob"], prob_in)
        assert "pp" not in out and "sigma" not in out
        for b in range(B):
            check_search(out, b, "thresh", height, prominence)
    out = ctx.debug_peak_trough_probs(prob_in=prob_in, opts=_ffi.peak_prob_opts(search="thresh"))
    assert out["count"].tolist() == [3, 2, 1, 2, 149, 0, 43, 0]
    assert out["keep"][0].nonzero()[0].tolist() == [64, 100, 256]
    assert (out["left_bases"][6, 150], out["right_bases"][6, 150]) == (143, 157)     # the nearest of the equal minima
    # windows: the first sample of a plateau wins; a window without a positive sample gives index 0
    win = np.array([(0, n - 1), (61, 300 - 1), (0, 59), (1, 59), (70, 99), (251, 262), (256, 256), (0, -1), (n, n - 1)] +
                   [(k, k + 200) for k in range(55)])
    assert len(win) == 64
    out = ctx.debug_peak_trough_probs(prob_in=prob_in, opts=_ffi.peak_prob_opts(search="ranges"), ranges=win)
    for b in range(B):
        check_search(out, b, "ranges", windows=win)
    assert out["range_peaks"][0, :9].tolist() == [250, 250, 0, 0, 0, 251, 256, 0, 0]
    assert (out["range_peaks"][7] == 0).all()


# ---- 2. position independence ------------------------------------------------------------------------------------------------------
def test_position_in_the_batch_does_not_change_the_bits(ctx):
    from hipdrt import _ffi
    rng = np.random.default_rng(11)
    n = 257
    batch = [rng.normal(size=(37, n)) for _ in range(3)] + [rng.random((37, n)) + 0.1 for _ in range(3)]
    win = windows_of(n, rng, 20)
    for bayes_cov in (1, 0):
        rows = batch if bayes_cov else batch[:3]
        for kw, ranges in ((dict(search="thresh", ext_left=20, ext_right=200), None), (dict(search="thresh", height=0.1, prominence=0.05), None),
                           (dict(search="ranges"), win)):
            opts = _ffi.peak_prob_opts(bayes_cov=bayes_cov, **kw)
            many = ctx.debug_peak_trough_probs(*rows, opts=opts, ranges=ranges)
            one = ctx.debug_peak_trough_probs(*[r[17:18] for r in rows], opts=opts, ranges=ranges)
            for k, v in one.items():
                got = many[k][:, 17] if k == "sigma" else many[k][17]
                assert np.array_equal(v[:, 0] if k == "sigma" else v[0], got, equal_nan=True), (k, bayes_cov, kw)
            assert np.isfinite(many["prob"]).all() and (kw["search"] != "thresh" or (many["count"] > 0).all())


# ---- 3. refusals -------------------------------------------------------------------------------------------------------------------
def test_hook_refusals(ctx):
    from hipdrt import _ffi
    rows = integer_rows(np.random.default_rng(3), 2, 40)
    big = [np.zeros((1, 4096))] * 3 + [np.ones((1, 4096))] * 3
    with pytest.raises(_ffi.HipDrtError, match="LDS"):                               # nothing is launched
        ctx.debug_peak_trough_probs(*big)
    with pytest.raises(_ffi.HipDrtError, match="nranges"):
        ctx.debug_peak_trough_probs(*rows, opts=_ffi.peak_prob_opts(search="ranges"), ranges=[(0, 5)] * 65)
    for bad in ((0, 40), (-1, 5), (7, 5)):
        with pytest.raises(_ffi.HipDrtError, match="ranges"):
            ctx.debug_peak_trough_probs(*rows, opts=_ffi.peak_prob_opts(search="ranges"), ranges=[(0, 5), bad])
    with pytest.raises(_ffi.HipDrtError, match="search 2 needs"):
        ctx.debug_peak_trough_probs(*rows, opts=_ffi.peak_prob_opts(search="ranges"))
    for kw in (dict(std_size=4), dict(std_size=1), dict(std_baseline=-1.0), dict(search=3), dict(ext_left=40), dict(ext_right=-2),
               dict(height=np.inf)):
        with pytest.raises(_ffi.HipDrtError, match="invalid argument"):
            ctx.debug_peak_trough_probs(*rows, opts=_ffi.peak_prob_opts(**kw))
    with pytest.raises(_ffi.HipDrtError, match="variance rows"):
        ctx.debug_peak_trough_probs(*rows[:3])
    for bad in (np.nan, np.inf):
        for k in range(6):
            r = [x.copy() for x in rows]
            r[k][1, 7] = bad
            with pytest.raises(_ffi.HipDrtError, match="non-finite"):
                ctx.debug_peak_trough_probs(*r)


@pytest.fixture(scope="module")
def fit37():
    from hipdrt import synth
    from hipdrt.models import DRT
    z = synth.zarc2_batch(FREQ71, 37, first_seed=900)
    drt = DRT(warn=False)
    res = drt.fit_eis_batch(FREQ71, z)
    assert (res["status"] >= 0).all()
    return drt, z, res


def test_entry_refusals(ctx, fit37):
    from hipdrt import _ffi
    drt = fit37[0]
    plan = drt._plan
    ln_tau = np.log(drt.get_tau_eval(10))
    with pytest.raises(_ffi.HipDrtError, match="LDS"):
        plan.peak_trough_probs(np.linspace(-20, 5, 4096), _ffi.peak_prob_opts())
    with pytest.raises(_ffi.HipDrtError, match="nranges"):
        plan.peak_trough_probs(ln_tau, _ffi.peak_prob_opts(search="ranges"), ranges=[(0, 5)] * 65)
    with pytest.raises(_ffi.HipDrtError, match="ranges"):
        plan.peak_trough_probs(ln_tau, _ffi.peak_prob_opts(search="ranges"), ranges=[(0, len(ln_tau))])
    with pytest.raises(_ffi.HipDrtError, match="std_size"):
        plan.peak_trough_probs(ln_tau, _ffi.peak_prob_opts(std_size=6))
    with pytest.raises(_ffi.HipDrtError, match="row_scale"):
        plan.peak_trough_probs(ln_tau, _ffi.peak_prob_opts(), row_scale=np.zeros(37))
    fresh = _ffi.Plan(ctx, plan.freq, plan.tau, drt.tau_epsilon, mode=_ffi.MODE_TRAPZ, capacity=2)
    with pytest.raises(_ffi.HipDrtError, match="no fitted batch"):
        fresh.peak_trough_probs(ln_tau, _ffi.peak_prob_opts())
    with pytest.raises(ValueError, match="64"):
        drt.find_peaks_byprob_batch(peak_tau_ranges=[(1e-4, 1e-2)] * 65)
    with pytest.raises(ValueError, match="strictly increasing"):
        drt.find_peaks_byprob_batch(tau=drt.get_tau_eval(10)[::-1], peak_tau_ranges=[(1e-4, 1e-2)])


# ---- 4. the whole chain against the statement on downloaded rows ---------------------------------------------------------------------
@pytest.mark.parametrize("grid", ["tau_eval10", "257 points"])
def test_chain_against_the_statement_on_downloaded_rows(fit37, grid):
    from hipdrt import _ffi
    drt = fit37[0]
    tau = drt.get_tau_eval(10)
    if grid != "tau_eval10":
        tau = np.logspace(np.log10(tau[0]), np.log10(tau[-1]), 257)
    n, B = len(tau), 37
    li, ri = drt._extend_var_indices(tau)
    means = [drt.predict_drt_batch(tau=tau, order=k, sign=1) for k in range(3)]
    sig_ref = []
    for k in range(3):
        var, ok = drt.estimate_distribution_var_batch(tau=tau, order=k, extend_var=True)
        assert ok.all()
        sig_ref.append(np.array([peaks.sigma_floor(v ** 0.5) for v in var]))
    win = peaks.range_windows(tau, [(1e-5, 1e-3), (1e-3, 1e-1), (tau[0], tau[-1]), (tau[5], tau[5]), (1e-9, 1e-8)])
    total = 0
    for bayes_cov in (1, 0):
        kw = dict(bayes_cov=bayes_cov, ext_left=li if bayes_cov else -1, ext_right=ri if bayes_cov else -1)
        out = drt._plan.peak_trough_probs(np.log(tau), _ffi.peak_prob_opts(search="thresh", height=0.25, prominence=0.125, **kw), want=ALL)
        byr = drt._plan.peak_trough_probs(np.log(tau), _ffi.peak_prob_opts(search="ranges", **kw), ranges=win, want=ALL)
        assert (out["status"] >= 0).all() and out["mu"].shape == (3, B, n)
        for k in range(3):
            np.testing.assert_array_equal(out["mu"][k], means[k], err_msg=f"order {k}")            # bit for bit
            if bayes_cov:
                np.testing.assert_allclose(out["sigma"][k], sig_ref[k], rtol=1e-12, atol=0, err_msg=f"order {k}")
        np.testing.assert_array_equal(byr["prob"], out["prob"])
        for b in range(B):
            rows = [out["mu"][k][b] for k in range(3)]
            pp, tp, _ = peaks.peak_trough_probs_rows(*rows, sigma=out["sigma"][:, b])
            np.testing.assert_allclose(out["pp"][b], pp, rtol=0, atol=PP_ERFC, err_msg=f"row {b}")
            np.testing.assert_allclose(out["tp"][b], tp, rtol=0, atol=TP_ERFC, err_msg=f"row {b}")
            np.testing.assert_allclose(out["prob"][b], peaks.peak_prob_of(pp, tp), rtol=0, atol=PP_ERFC + TP_ERFC, err_msg=f"row {b}")
            if not bayes_cov:
                filt = [peaks.filtered_sigma(r) for r in rows]
                np.testing.assert_allclose(out["sigma"][:, b], filt, rtol=(n + 16) * U, atol=0, err_msg=f"row {b}")
            total += check_search(out, b, "thresh", 0.25, 0.125)
            check_search(byr, b, "ranges", windows=win)
        # the methods are these calls
        pp_m, tp_m = drt.predict_peak_trough_probs_batch(tau=tau, bayes_cov=bool(bayes_cov))
        assert np.array_equal(pp_m, out["pp"]) and np.array_equal(tp_m, out["tp"])
        assert np.array_equal(drt.predict_peak_prob_batch(tau=tau, bayes_cov=bool(bayes_cov)), out["prob"])
        got = drt.find_peaks_byprob_batch(tau=tau, height=0.25, prominence=0.125, bayes_cov=bool(bayes_cov), return_info=True)
        for b in range(B):
            np.testing.assert_array_equal(got[2][b], np.flatnonzero(out["keep"][b]))
            np.testing.assert_array_equal(got[0][b], tau[got[2][b]])
            np.testing.assert_array_equal(got[3][b]["peak_heights"], out["prob"][b][got[2][b]])
        byrange = drt.find_peaks_byprob_batch(tau=tau, bayes_cov=bool(bayes_cov), peak_tau_ranges=[(1e-5, 1e-3), (1e-3, 1e-1)])
        for b in range(B):
            np.testing.assert_array_equal(byrange[b], tau[byr["range_peaks"][b, :2]])
    assert total >= B                                     # at least a peak per spectrum and mode on average: not vacuous


# ---- 5. the chain against the reference's recorded run ----------------------------------------------------------------------------
@pytest.mark.parametrize("bayes_cov", [1, 0])
@pytest.mark.parametrize("tag", ["plain", "nn", "sneg"])
def test_fit_against_the_reference_run(tag, bayes_cov):
    from hipdrt.models import DRT
    g = np.load(os.path.join(GOLDEN, "refrun_peak_prob_golden71x91.npz"))
    drt = DRT()
    drt.fit_eis(g["freq"], g["z"], **{"plain": dict(), "nn": dict(nonneg=False), "sneg": dict(series_neg=True)}[tag])
    tau = g["tau"]
    np.testing.assert_allclose(drt.get_tau_eval(10), tau, rtol=1e-13)
    bc = bool(bayes_cov)
    ref_pp, ref_tp = g[f"{tag}_pp_b{bayes_cov}"], g[f"{tag}_tp_b{bayes_cov}"]
    pp, tp = drt.predict_peak_trough_probs(tau, bayes_cov=bc)
    parity("pp", pp, ref_pp, default=1e-6, scale=1.0)
    parity("tp", tp, ref_tp, default=1e-6, scale=1.0)
    parity("prob", drt.predict_peak_prob(bayes_cov=bc), ref_pp * (1 - ref_tp), default=1e-6, scale=1.0)
    for height, prominence in g["thresholds"]:
        key = f"{tag}_b{bayes_cov}_h{height:g}_p{prominence:g}"
        peak_tau, tau_out, idx, info = drt.find_peaks_byprob(tau, height=height, prominence=prominence, bayes_cov=bc, return_info=True)
        np.testing.assert_array_equal(idx, g[f"{key}_idx"], err_msg=key)
        np.testing.assert_array_equal(peak_tau, tau[idx])
        assert set(info) == {"peak_heights", "prominences", "left_bases", "right_bases"}
        np.testing.assert_array_equal(info["left_bases"], g[f"{key}_left_bases"])
        np.testing.assert_array_equal(info["right_bases"], g[f"{key}_right_bases"])
        parity(f"heights_h{height:g}_p{prominence:g}", info["peak_heights"], g[f"{key}_peak_heights"], default=1e-6, scale=1.0)
        parity(f"prominences_h{height:g}_p{prominence:g}", info["prominences"], g[f"{key}_prominences"], default=1e-6, scale=1.0)
    ranges = [tuple(r) for r in g["ranges"]]
    peak_tau, _, idx, info = drt.find_peaks_byprob(tau, bayes_cov=bc, peak_tau_ranges=ranges, return_info=True)
    np.testing.assert_array_equal(idx, g[f"{tag}_b{bayes_cov}_ranges_idx"])
    assert info == {} and np.array_equal(peak_tau, tau[idx])
    np.testing.assert_allclose(drt.find_peaks_byprob(bayes_cov=bc, peak_tau_ranges=ranges), peak_tau, rtol=1e-13)   # tau=None: get_tau_eval(10)


# ---- 6. other behaviour ----------------------------------------------------------------------------------------------------------------
def test_alone_and_in_a_batch_give_the_same_bits(fit37):
    from hipdrt import _ffi
    from hipdrt.models import DRT
    drt, z, res = fit37
    tau = drt.get_tau_eval(10)
    ln_tau = np.log(tau)
    li, ri = drt._extend_var_indices(tau)
    win = peaks.range_windows(tau, [(1e-5, 1e-3), (1e-3, 1e-1)])
    calls = [(_ffi.peak_prob_opts(search="thresh", ext_left=li, ext_right=ri), None),
             (_ffi.peak_prob_opts(search="thresh", height=0.25, prominence=0.125, bayes_cov=False), None),
             (_ffi.peak_prob_opts(search="ranges", ext_left=li, ext_right=ri), win)]
    many = [drt._plan.peak_trough_probs(ln_tau, o, ranges=w, want=ALL) for o, w in calls]
    one = DRT(warn=False)
    for b in (0, 16, 36):
        r1 = one.fit_eis_batch(FREQ71, z[b:b + 1])
        assert np.array_equal(r1["x"][0], res["x"][b]), "the fit itself differs between batch sizes: nothing to compare"
        for (o, w), m in zip(calls, many):
            single = one._plan.peak_trough_probs(ln_tau, o, ranges=w, want=ALL)
            for k, v in single.items():
                three = k in ("mu", "sigma")
                assert np.array_equal(v[:, 0] if three else v[0], m[k][:, b] if three else m[k][b], equal_nan=True), (k, b, o.search)
    # the single-member forms are members of the batch
    assert np.array_equal(drt.predict_peak_prob(b=5), many[0]["prob"][5])
    assert np.array_equal(drt.predict_peak_trough_probs(b=5)[1], many[0]["tp"][5])
    assert np.array_equal(drt.find_peaks_byprob(b=5), tau[np.flatnonzero(many[0]["keep"][5])])


def test_failed_fit_gives_nan_rows_no_peaks_and_a_negative_status():
    from hipdrt import _ffi, synth
    from hipdrt.models import DRT
    z = synth.zarc2_batch(FREQ71, 5, first_seed=300)
    zbad = z.copy()
    zbad[2] = np.nan
    good, bad = DRT(warn=False), DRT(warn=False)
    good.fit_eis_batch(FREQ71, z)
    res = bad.fit_eis_batch(FREQ71, zbad)
    assert res["status"][2] < 0
    tau = bad.get_tau_eval(10)
    win = peaks.range_windows(tau, [(1e-5, 1e-3), (1e-3, 1e-1)])
    for bayes_cov in (True, False):
        for search, w in (("thresh", None), ("ranges", win)):
            o = _ffi.peak_prob_opts(bayes_cov=bayes_cov, search=search)
            a, c = bad._plan.peak_trough_probs(np.log(tau), o, ranges=w, want=ALL), good._plan.peak_trough_probs(np.log(tau), o, ranges=w, want=ALL)
            assert a["status"][2] < 0 and (np.delete(a["status"], 2) >= 0).all()
            for k in ("pp", "tp", "prob"):
                assert np.isnan(a[k][2]).all(), k
            assert np.isnan(a["sigma"][:, 2]).all() and np.isnan(a["mu"][:, 2]).all()
            if search == "thresh":
                assert a["count"][2] == 0 and not a["keep"][2].any() and (a["left_bases"][2] == -1).all() and (a["right_bases"][2] == -1).all()
                assert np.isnan(a["heights"][2]).all() and np.isnan(a["prominences"][2]).all()
            else:
                assert (a["range_peaks"][2] == -1).all()
            for k, v in a.items():
                ax = 1 if k in ("mu", "sigma") else 0
                assert np.array_equal(np.delete(v, 2, axis=ax), np.delete(c[k], 2, axis=ax)), k
        assert np.isnan(bad.predict_peak_prob_batch(bayes_cov=bayes_cov)[2]).all()
        assert [len(p) for p in bad.find_peaks_byprob_batch(bayes_cov=bayes_cov)][2] == 0
        assert [len(p) for p in bad.find_peaks_byprob_batch(bayes_cov=bayes_cov, peak_tau_ranges=[(1e-5, 1e-3)])] == [1, 1, 0, 1, 1]


def test_prepared_hybrid_plan_with_row_scale_against_the_statement():
    """a hybrid fit runs on a prepared plan at unit scale: the coefficient scale travels as row_scale"""
    from hipdrt import _ffi, synth
    from hipdrt.models import DRT
    drt = DRT(warn=False)
    drt.fit_hybrid(*synth.hybrid_measurement(seed=0))
    plan, scales = drt._predict_plan("test")
    assert scales is not None and scales[0] != 1.0
    tau = drt.get_tau_eval(10)
    n = len(tau)
    li, ri = drt._extend_var_indices(tau)
    for bayes_cov in (1, 0):
        kw = dict(bayes_cov=bayes_cov, ext_left=li if bayes_cov else -1, ext_right=ri if bayes_cov else -1)
        out = plan.peak_trough_probs(np.log(tau), _ffi.peak_prob_opts(search="thresh", height=0.25, prominence=0.125, **kw),
                                     row_scale=scales, want=ALL)
        assert (out["status"] >= 0).all()
        for k in range(3):
            # (the scale multiplies on the device here and on the host there: a rounding apart)
            ref = drt.predict_drt_batch(tau=tau, order=k, sign=1)
            np.testing.assert_allclose(out["mu"][k], ref, rtol=1e-13, atol=1e-13 * np.abs(ref).max())
            if bayes_cov:
                var, ok = drt.estimate_distribution_var_batch(tau=tau, order=k, extend_var=True)
                assert ok.all()
                np.testing.assert_allclose(out["sigma"][k][0], peaks.sigma_floor(var[0] ** 0.5), rtol=1e-12, atol=0)
        rows = [out["mu"][k][0] for k in range(3)]
        pp, tp, _ = peaks.peak_trough_probs_rows(*rows, sigma=out["sigma"][:, 0])
        np.testing.assert_allclose(out["pp"][0], pp, rtol=0, atol=PP_ERFC)
        np.testing.assert_allclose(out["tp"][0], tp, rtol=0, atol=TP_ERFC)
        np.testing.assert_allclose(out["prob"][0], peaks.peak_prob_of(pp, tp), rtol=0, atol=PP_ERFC + TP_ERFC)
        if not bayes_cov:
            np.testing.assert_allclose(out["sigma"][:, 0], [peaks.filtered_sigma(r) for r in rows], rtol=(n + 16) * U, atol=0)
        check_search(out, 0, "thresh", 0.25, 0.125)
        assert np.array_equal(drt.predict_peak_prob(tau, bayes_cov=bool(bayes_cov)), out["prob"][0])


def test_refusals_and_info_keys_of_the_methods(fit37):
    from hipdrt.models import DRT
    drt = fit37[0]
    for method in (drt.predict_peak_trough_probs, drt.predict_peak_prob, drt.find_peaks_byprob):
        with pytest.raises(NotImplementedError, match="x="):
            method(x=np.ones(3))
        with pytest.raises(NotImplementedError, match="p_matrix="):
            method(p_matrix=np.eye(3))
    with pytest.raises(NotImplementedError, match="prob="):
        drt.find_peaks_byprob(prob=np.ones(111))
    with pytest.raises(RuntimeError, match="finished"):
        DRT(warn=False).predict_peak_prob_batch()
    keys = {(None, None): set(), (0.1, None): {"peak_heights"}, (None, 0.1): {"prominences", "left_bases", "right_bases"},
            (0.1, 0.1): {"peak_heights", "prominences", "left_bases", "right_bases"}}
    for (height, prominence), want in keys.items():
        peak_tau, tau, idx, info = drt.find_peaks_byprob_batch(height=height, prominence=prominence, return_info=True)
        assert len(peak_tau) == len(idx) == len(info) == 37 and len(tau) == len(drt.get_tau_eval(10))
        for b in range(37):
            assert set(info[b]) == want and all(len(v) == len(idx[b]) for v in info[b].values())
            assert info[b].get("left_bases", np.zeros(0, dtype=np.intp)).dtype == np.intp
        one = drt.find_peaks_byprob(height=height, prominence=prominence, return_info=True, b=3)
        assert np.array_equal(one[2], idx[3]) and set(one[3]) == want
    peak_tau, tau, idx, info = drt.find_peaks_byprob_batch(peak_tau_ranges=[(1e-5, 1e-3), (1e-3, 1e-1)], return_info=True)
    assert all(i == {} for i in info) and all(len(p) == 2 for p in idx)
