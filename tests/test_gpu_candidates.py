"""GPU: candidate models of a fitted batch scored on the device (csrc/candidates.hip; hipdrt_plan_score_candidates and the hook
hipdrt_debug_candidate_llh).

1. the likelihood kernels alone against the statement (hipdrt.models.candidates.candidate_llh_terms) in np.longdouble;
2. invariance, bit for bit: a candidate alone and inside C = 17, a spectrum alone and as member 2 of 5, yh kept in LDS and passed
   through the scratch buffer;
3. the entry point on the live x of a fit against hipdrt_plan_llh_terms (bound of 1, twice: both are float64 evaluations of the
   same sums) and against hipdrt_plan_find_peaks (exact), uploaded and from the step store;
4. failed fits, ncand padding, more than max_peaks peaks, the refusals;
5. the fit's downloaded results are the same bits with and without a scoring call in between;
6. generate_candidates on a fresh fit, and the entry point on the reference's recorded candidates, against the reference's own
   generate_candidates runs (tools/make_candidates_golden.py), bounds from tests/candidates_bounds.json;
7. generate_candidates_batch on five spectra: a member equals its own single run, the step store equals the same x uploaded;
8. a recorded step that failed for a spectrum is no candidate of it; hipdrt_plan_pfrt_restore_s and its refusals.

Bound of 1 (u = 2^-53; nothing is measured from the kernel; candidates_util.reference_and_bound evaluates it per case from the
operands).  yh = rm x is a sum of n products: whatever the order and whether or not the products are fused, it is off by at most
dy = (n + 2) u |rm| |x|.  r = yh - rv rounds once more: d = dy + u |r|.  r^2 is off by e2 = 2 |r| d + d^2 + u r^2, s = vmm r^2, a
sum of m products, by es = |vmm| e2 + (m + 2) u |vmm| r^2; the floor is a maximum and adds nothing.  w = v^-1/2 has at most the
relative error of v (es / (v - es), asserted below 1/3) plus the roundings of the square root and the division (2 u): rw; the
floor at 1e-10 is again a maximum.  w yh is off by w dy + |w yh| (rw + u), w rv by |w rv| (rw + u).  Each of the three sums of m
products of those takes the first-order propagation of its factors plus (m + 4) u of the sum of the magnitudes; rss = a - 2 c + d
adds 3 u (a + 2 |c| + d).  log w moves by at most 2 rw for rw < 1/2 and the routine itself by 2 ulp (4 u |log w|); the sum of m
of them by (m + 4) u sum |log w|.

The scratch form.  cand_llh_kernel keeps 16 rows of round_up(m, 32) + 4 doubles of yh in dynamic LDS beside 45,568 bytes of
static LDS (two staging slabs of 16 x 68 and 64 x 68 doubles and a 4 x 16 x 4 reduction table); a workgroup has 160 KiB =
163,840 bytes, of which the launcher keeps 512 in reserve.  128 (round_up(m, 32) + 4) <= 163,840 - 45,568 - 512 = 117,760 gives
round_up(m, 32) <= 916, i.e. m <= 896: m = 897 is the smallest m that takes the scratch form.
"""
import json
import os

import numpy as np
import pytest

from candidates_util import llh_case, reference_and_bound
from conftest import GOLDEN, ROOT, parity

pytestmark = pytest.mark.gpu

FREQ71 = np.logspace(6, -1, 71)
M_SCRATCH = 897


@pytest.fixture(scope="module")
def ctx():
    from hipdrt import _ffi
    return _ffi.get_context(0)


@pytest.fixture(scope="module")
def fit5():
    from hipdrt import synth
    from hipdrt.models import DRT
    z = synth.zarc2_batch(FREQ71, 5, first_seed=7)
    drt = DRT(warn=False)
    res = drt.fit_eis_batch(FREQ71, z)
    return drt, z, res


def check_against_reference(ctx, x, rm, rv, vmm, vf):
    rss, slw = ctx.debug_candidate_llh(x, rm, rv, vmm, vf)
    r_rss, r_slw, b_rss, b_slw = reference_and_bound(x, rm, rv, vmm, vf)
    e_rss, e_slw = np.abs(rss - r_rss), np.abs(slw - r_slw)
    print(f"rss: worst deviation / bound {np.max(e_rss / b_rss):.3f}; sum_log_w: {np.max(e_slw / b_slw):.3f}; "
          f"bounds relative to the values {np.max(b_rss / np.abs(r_rss)):.1e} {np.max(b_slw / np.maximum(np.abs(r_slw), 1.0)):.1e}")
    assert np.all(e_rss <= b_rss), (e_rss / b_rss).max()
    assert np.all(e_slw <= b_slw), (e_slw / b_slw).max()
    return rss, slw


# ---- 1. the likelihood kernels alone --------------------------------------------------------------------------------------------
@pytest.mark.parametrize("batched", [False, True], ids=["shared", "batched"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("shape", [(2, 1), (6, 3), (18, 5), (142, 93), (515, 514)])
def test_llh_kernels_against_the_statement(ctx, shape, B, batched):
    m, n = shape
    for C in (1, 15, 16, 17, 33):
        rng = np.random.default_rng(10000 * m + 100 * C + 2 * B + batched)
        check_against_reference(ctx, *llh_case(rng, C, B, m, n, batched))


def test_llh_kernels_scratch_form(ctx):
    from hipdrt import _ffi
    rng = np.random.default_rng(897)
    case = llh_case(rng, 17, 2, M_SCRATCH, 3, True)
    check_against_reference(ctx, *case)
    # one row fewer fits in LDS; asking for the LDS form at M_SCRATCH is refused before anything is launched
    check_against_reference(ctx, *llh_case(rng, 3, 1, M_SCRATCH - 1, 3, False))
    ctx.debug_candidate_form(0)
    try:
        with pytest.raises(_ffi.HipDrtError, match="LDS"):
            ctx.debug_candidate_llh(*case)
    finally:
        ctx.debug_candidate_form(-1)


def test_llh_kernels_with_both_floors_active(ctx):
    rng = np.random.default_rng(5)
    C, B, m, n = 17, 3, 142, 93
    x, rm, rv, vmm, vf = llh_case(rng, C, B, m, n, False)
    s = ((x[:, 1] @ rm.T - rv[1]) ** 2) @ vmm.T
    vf = np.array([1e-30, float(np.median(s)), 1e22])       # no floor; the variance floor on about half the rows; both floors
    rss, slw = check_against_reference(ctx, x, rm, rv, vmm, vf)
    assert np.count_nonzero(s < vf[1]) > 0 and np.count_nonzero(s > vf[1]) > 0
    np.testing.assert_allclose(slw[:, 2], m * np.log(1e-10), rtol=1e-14)      # every weight of spectrum 2 is the floor 1e-10


# ---- 2. invariance, bit for bit ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(18, 5), (142, 93), (515, 514)])
def test_a_candidate_gives_the_same_bits_alone_and_among_seventeen(ctx, shape):
    m, n = shape
    x, rm, rv, vmm, vf = llh_case(np.random.default_rng(m), 17, 2, m, n, True)
    rss, slw = ctx.debug_candidate_llh(x, rm, rv, vmm, vf)
    for c in (0, 5, 16):
        r1, s1 = ctx.debug_candidate_llh(x[c:c + 1], rm, rv, vmm, vf)
        assert np.array_equal(r1[0], rss[c]) and np.array_equal(s1[0], slw[c]), c


@pytest.mark.parametrize("batched", [False, True], ids=["shared", "batched"])
def test_a_spectrum_gives_the_same_bits_alone_and_as_member_2_of_5(ctx, batched):
    x, rm, rv, vmm, vf = llh_case(np.random.default_rng(25), 6, 5, 142, 93, batched)
    rss, slw = ctx.debug_candidate_llh(x, rm, rv, vmm, vf)
    r1, s1 = ctx.debug_candidate_llh(x[:, 2:3], rm[2] if batched else rm, rv[2:3], vmm, vf[2:3])
    assert np.array_equal(r1[:, 0], rss[:, 2]) and np.array_equal(s1[:, 0], slw[:, 2])


@pytest.mark.parametrize("shape", [(2, 1), (142, 93), (515, 514)])
def test_both_ways_of_keeping_yh_give_the_same_bits(ctx, shape):
    m, n = shape
    case = llh_case(np.random.default_rng(n), 33, 3, m, n, True)
    try:
        ctx.debug_candidate_form(0)
        lds = ctx.debug_candidate_llh(*case)
        ctx.debug_candidate_form(1)
        scr = ctx.debug_candidate_llh(*case)
    finally:
        ctx.debug_candidate_form(-1)
    assert np.array_equal(lds[0], scr[0]) and np.array_equal(lds[1], scr[1])


# ---- 3. the entry point against the existing ones ---------------------------------------------------------------------------------
def compact(dense, max_peaks=16):
    """find_peaks' dense rows -> the padded lists of hipdrt_plan_score_candidates"""
    B = dense["keep"].shape[0]
    idx = np.full((B, max_peaks), -1, dtype=np.int32)
    ht, pr = np.full((B, max_peaks), np.nan), np.full((B, max_peaks), np.nan)
    for b in range(B):
        k = np.nonzero(dense["keep"][b])[0]
        idx[b, :len(k)], ht[b, :len(k)], pr[b, :len(k)] = k, dense["heights"][b, k], dense["prominences"][b, k]
    return idx, ht, pr


def test_live_x_agrees_with_llh_terms_and_find_peaks(fit5):
    from hipdrt import _ffi
    drt, z, res = fit5
    plan = drt._plan
    x = plan.get("x")[None]
    ln_tau = np.log(drt.get_tau_eval(10))
    rss0, slw0 = plan.llh_terms()
    _, _, b_rss, b_slw = reference_and_bound(x, plan.get("rm"), plan.get("rv"), plan.get("vmm"), plan.get("var_floor"))
    for opts in (_ffi.peak_opts(search=1), _ffi.peak_opts(search=0), _ffi.peak_opts(search=1, normalize=0, height=0.0, prominence=1e-3)):
        out = plan.score_candidates(x, ln_tau_find=ln_tau, opts=opts)
        assert np.all(np.abs(out["rss"][0] - rss0) <= 2 * b_rss[0]) and np.all(np.abs(out["sum_log_w"][0] - slw0) <= 2 * b_slw[0])
        dense = plan.find_peaks(ln_tau, opts)
        idx, ht, pr = compact(dense)
        assert dense["count"].sum() > 0
        np.testing.assert_array_equal(out["count"][0], dense["count"])
        np.testing.assert_array_equal(out["peak_index"][0], idx)
        assert np.array_equal(out["heights"][0], ht, equal_nan=True) and np.array_equal(out["prominences"][0], pr, equal_nan=True)
        np.testing.assert_array_equal(out["status"][0], dense["status"])


def test_step_store_scoring_equals_the_same_x_uploaded(fit5):
    from hipdrt import _ffi, synth
    from hipdrt.models import DRT
    drt = DRT(warn=False)
    res = drt.fit_eis_batch(FREQ71, synth.zarc2_batch(FREQ71, 5, first_seed=7))
    plan = drt._plan
    ln_tau = np.log(drt.get_tau_eval(10))
    plan.pfrt_begin(3)
    plan.pfrt_record()
    xs = [plan.get("x")]
    for f in (2.0, 4.0):
        drt.continue_from_init(s_0=np.asarray(drt.fit_kwargs["s_0"], dtype=float) * f, l2_lambda_0=drt.fit_kwargs["l2_lambda_0"] / f)
        plan.pfrt_record()
        xs.append(plan.get("x"))
    xs = np.array(xs)
    assert not np.array_equal(xs[0], xs[2])
    a = plan.score_candidates(None, ln_tau_find=ln_tau)
    b = plan.score_candidates(xs, ln_tau_find=ln_tau)
    for k in set(a) - {"status"}:
        assert a[k].shape[0] == 3 and np.array_equal(a[k], b[k], equal_nan=True), k
    # the status of a slot: recorded with the step when the steps are scored, the live fit's for uploaded candidates
    np.testing.assert_array_equal(a["status"], [plan.pfrt_step_state(c)["status"] for c in range(3)])
    np.testing.assert_array_equal(b["status"], np.broadcast_to(plan.download()["status"], (3, 5)))
    # and a member of the batch equals the same candidates of that member scored alone (shared rm: any plan of one spectrum)
    one = DRT(warn=False)
    r1 = one.fit_eis_batch(FREQ71, synth.zarc2_batch(FREQ71, 5, first_seed=7)[2:3])
    assert np.array_equal(r1["x"][0], res["x"][2]), "the fit itself differs between batch sizes: nothing to compare"
    c = one._plan.score_candidates(xs[:, 2:3], ln_tau_find=ln_tau)
    for k in set(a) - {"status"}:           # (the status is the live fit's: restarted in the batch, freshly fitted alone)
        assert np.array_equal(a[k][:, 2], c[k][:, 0], equal_nan=True), k


# ---- 4. failures, padding, overflow, refusals -------------------------------------------------------------------------------------
def test_failed_fit_and_ncand_padding():
    from hipdrt import _ffi, synth
    from hipdrt.models import DRT
    z = synth.zarc2_batch(FREQ71, 4, first_seed=300)
    z[2] = np.nan
    drt = DRT(warn=False)
    res = drt.fit_eis_batch(FREQ71, z)
    assert res["status"][2] < 0
    plan = drt._plan
    ln_tau = np.log(drt.get_tau_eval(10))
    x = np.repeat(np.nan_to_num(plan.get("x"))[None], 3, axis=0)
    ncand = np.array([3, 1, 3, 0], dtype=np.int32)
    out = plan.score_candidates(x, ncand=ncand, ln_tau_find=ln_tau)
    full = plan.score_candidates(x, ln_tau_find=ln_tau)
    absent = np.arange(3)[:, None] >= ncand[None, :]
    absent[:, 2] = True
    for k, v in out.items():
        if k == "status":
            continue
        pad = -1 if v.dtype == np.int32 else np.nan
        assert np.array_equal(v[absent], np.full_like(v[absent], pad), equal_nan=True), k
        assert np.array_equal(v[~absent], full[k][~absent], equal_nan=True), k
        assert not np.any(v == (-77 if v.dtype == np.int32 else 7e77)), k      # every slot was written
    assert (out["status"][:, 2] == res["status"][2]).all() and (full["status"][:, 2] == res["status"][2]).all()
    assert (out["status"][1:, 1] == _ffi.CANDIDATE_ABSENT).all() and (out["status"][:, 3] == _ffi.CANDIDATE_ABSENT).all()
    assert (out["status"][:, 0] == res["status"][0]).all() and out["status"][0, 1] == res["status"][1]
    # likelihood sums alone (no find grid) carry the same padding and statuses
    llh = plan.score_candidates(x, ncand=ncand)
    assert set(llh) == {"rss", "sum_log_w", "status"}
    for k in llh:
        assert np.array_equal(llh[k], out[k], equal_nan=True), k


def test_more_peaks_than_max_peaks(fit5):
    from hipdrt import _ffi
    drt = fit5[0]
    plan = drt._plan
    ln_tau = np.log(drt.get_tau_eval(10))
    x = plan.get("x")[None]
    opts = _ffi.peak_opts(search=1)
    full = plan.score_candidates(x, ln_tau_find=ln_tau, opts=opts)
    k = int(full["count"].max())
    assert k >= 2
    out = plan.score_candidates(x, ln_tau_find=ln_tau, opts=opts, max_peaks=k - 1)
    over = full["count"][0] > k - 1
    np.testing.assert_array_equal(out["count"], full["count"])
    assert (out["status"][0][over] == _ffi.PEAKS_OVERFLOW).all() and (out["status"][0][~over] >= 0).all()
    assert (out["peak_index"][0][over] == -1).all() and np.isnan(out["heights"][0][over]).all()
    np.testing.assert_array_equal(out["peak_index"][0][~over], full["peak_index"][0][~over][:, :k - 1])


def test_refusals(fit5, ctx):
    from hipdrt import _ffi
    drt = fit5[0]
    plan = drt._plan
    ln_tau = np.log(drt.get_tau_eval(10))
    x = plan.get("x")[None]
    with pytest.raises(_ffi.HipDrtError, match="method must be 0"):
        plan.score_candidates(x, ln_tau_find=ln_tau, opts=_ffi.peak_opts(method="prob"))
    with pytest.raises(_ffi.HipDrtError, match="max_peaks"):
        plan.score_candidates(x, ln_tau_find=ln_tau, max_peaks=65)
    with pytest.raises(_ffi.HipDrtError, match="ncand"):
        plan.score_candidates(x, ncand=np.full(plan.B, 2, dtype=np.int32))
    with pytest.raises(_ffi.HipDrtError, match="LDS"):
        plan.score_candidates(x, ln_tau_find=np.linspace(-20, 5, 20000))
    with pytest.raises(_ffi.HipDrtError, match="eval_sign"):
        plan.score_candidates(x, ln_tau_find=ln_tau, opts=_ffi.peak_opts(eval_sign=0))
    fresh = _ffi.Plan(ctx, plan.freq, plan.tau, drt.tau_epsilon, mode=_ffi.MODE_TRAPZ, capacity=2)
    fresh.B = 2                                     # (the wrapper sizes its arrays by it; the library knows nothing is staged)
    with pytest.raises(_ffi.HipDrtError, match="no fitted batch"):
        fresh.score_candidates(np.zeros((1, 2, fresh.n)))
    one_more = type(drt)(warn=False)
    one_more.fit_eis_batch(FREQ71, fit5[1][:1])
    with pytest.raises(_ffi.HipDrtError, match="no recorded steps"):
        one_more._plan.score_candidates(None)


# ---- 5. scoring leaves the fit alone ----------------------------------------------------------------------------------------------
def test_fit_results_do_not_depend_on_a_scoring_call(fit5):
    from hipdrt.models import DRT
    z = fit5[1]
    a, b = DRT(warn=False), DRT(warn=False)
    a.fit_eis_batch(FREQ71, z)
    b.fit_eis_batch(FREQ71, z)
    ln_tau = np.log(b.get_tau_eval(10))
    b._plan.score_candidates(np.repeat(b._plan.get("x")[None], 17, axis=0), ln_tau_find=ln_tau)
    ra, rb = a.continue_from_init(weight_factor=0.5), b.continue_from_init(weight_factor=0.5)
    da, db = a._plan.download(s_vectors=True), b._plan.download(s_vectors=True)
    for k in da:
        assert np.array_equal(da[k], db[k], equal_nan=True), k
    for k in ("x", "rho", "weights", "s_vectors"):
        assert np.array_equal(ra[k], rb[k], equal_nan=True), k


# ---- 6. against the reference's generate_candidates runs --------------------------------------------------------------------------
def ref_parity(label, got, ref, scale):
    """conftest.parity against the reference's recorded values, the bound from tests/candidates_bounds.json (label -> [measured
    on the GPU, bound = 20 x measured rounded up to 1 / 2 / 5 x 10^k, never below 1e-13: a deviation of a few ulp is no
    measurement]); a label not measured yet: 1e-7 of the scale, the largest |llh| of the fixture (Bayes factors: 1, the largest
    of them)"""
    with open(os.path.join(ROOT, "tests", "candidates_bounds.json")) as f:
        entry = json.load(f).get(label)
    return parity(label, got, ref, bound=1e-7 if entry is None else float(entry[1]), label=label, scale=scale)


def fit_case(name):
    from hipdrt import synth
    from hipdrt.models import DRT
    g = np.load(os.path.join(GOLDEN, f"refrun_generate_candidates_{name}.npz"))
    drt = DRT(warn=False)
    if name == "hybrid_s0":
        drt.fit_hybrid(*synth.hybrid_measurement(seed=0))
    else:
        drt.fit_eis(g["freq"], g["z"], **(dict(nonneg=False) if name.endswith("_neg") else {}))
    return g, drt


def rows_of(padded):
    return [r[~np.isnan(r)] for r in padded]


@pytest.mark.parametrize("name", ["golden71x91", "golden71x91_neg", "hybrid_s0"])
def test_generate_candidates_against_the_reference_run(name):
    """generate_candidates on a fresh fit: every recorded iterate of the base fit, the s_0 pass and the weight pass is a candidate,
    none is left out of the comparison -- peak counts, peak positions, best and filled keys exact (the fixture script asserts
    that no count of the reference is decided by a margin below 1e-9); llh, bic and the Bayes factors within the table's
    bounds.  Then the entry point on the REFERENCE's recorded candidate x, uploaded to the same plan (its matrix as the
    restarts left it, as the reference's own scoring found it): counts and positions exact, llh and bic within the table."""
    g, drt = fit_case(name)
    top = float(np.abs(g["llh"]).max())
    # evaluate_bic of the fit itself, before any restart: upstream's rule, llh under the fit's own est_weights
    assert len(drt.find_peaks()) == int(g["fit_num_peaks"])
    ref_parity(f"{name}:evaluate_bic", [drt.evaluate_bic()], [g["evaluate_bic"]], top)
    n_data = drt._num_independent_data()
    own = (drt._plan.ns + 4 * int(g["fit_num_peaks"])) * np.log(n_data) - 2 * drt.evaluate_llh()      # the package's own evaluate_llh
    assert abs(drt.evaluate_bic() - own) <= 1e-9 * top
    cd = drt.generate_candidates()
    tau = drt.get_tau_eval(10)
    np.testing.assert_allclose(tau, g["tau"], rtol=1e-13)
    assert drt._plan.ns == int(g["num_special"]) and drt._num_independent_data() == int(g["num_independent_data"])
    C = len(g["x"])
    assert len(cd["x"]) == C and len(drt.qphb_history) == int(g["counts"][0])
    ref_tau = rows_of(g["peak_tau"])
    # -- end to end
    np.testing.assert_array_equal(cd["num_peaks"], g["num_peaks"])
    for c in range(C):
        np.testing.assert_allclose(cd["peak_tau"][c], ref_tau[c], rtol=1e-13, err_msg=str(c))
    assert list(drt.best_candidate_dict) == g["best_keys"].tolist()
    for key, want in zip(g["best_keys"], rows_of(g["best_peak_tau"])):
        np.testing.assert_allclose(drt.best_candidate_dict[int(key)]["peak_tau"], want, rtol=1e-13, err_msg=str(key))
    np.testing.assert_array_equal(drt.best_candidate_df["num_peaks"], g["best_candidate_df"][:, 1])
    assert drt.get_best_candidate_id("continuous") == g["best_id"]
    ref_parity(f"{name}:e2e_x", cd["x"], g["x"], float(np.abs(g["x"]).max()))
    ref_parity(f"{name}:e2e_llh", cd["llh"], g["llh"], top)
    ref_parity(f"{name}:e2e_bic", cd["bic"], g["bic"], top)
    ref_parity(f"{name}:e2e_best_llh", drt.best_candidate_df["llh"], g["best_candidate_df"][:, 2], top)
    ref_parity(f"{name}:e2e_norm_bayes_factors", drt.evaluate_norm_bayes_factors("continuous"), g["norm_bayes_factors"], 1.0)
    # -- the reference's own candidates through the entry point
    plan, tau_, opts = drt._candidate_peak_request("test", None)
    out = drt._score_candidates(plan, g["x"][:, None, :], tau_, opts, None)
    np.testing.assert_array_equal(out["count"][:, 0], g["num_peaks"])
    for c in range(C):
        idx = out["peak_index"][c, 0]
        np.testing.assert_allclose(tau[idx[idx >= 0]], ref_tau[c], rtol=1e-13, err_msg=str(c))
    scale_f = float(np.nanmax(np.abs(g["peak_heights"])))
    ref_parity(f"{name}:ref_x_heights", np.nan_to_num(out["heights"][:, 0, :g["peak_heights"].shape[1]]), np.nan_to_num(g["peak_heights"]), scale_f)
    ref_parity(f"{name}:ref_x_prominences", np.nan_to_num(out["prominences"][:, 0, :g["prominences"].shape[1]]), np.nan_to_num(g["prominences"]), scale_f)
    ref_parity(f"{name}:ref_x_llh", out["llh"][:, 0], g["llh"], top)
    bic = (plan.ns + 4 * out["count"][:, 0]) * np.log(drt._num_independent_data()) - 2 * out["llh"][:, 0]
    ref_parity(f"{name}:ref_x_bic", bic, g["bic"], top)


# ---- 7. the batch method ------------------------------------------------------------------------------------------------------------
def test_batch_members_equal_single_runs_bit_for_bit(fit5):
    from hipdrt.models import DRT
    z = fit5[1]
    drt = DRT(warn=False)
    drt.fit_eis_batch(FREQ71, z)
    out = drt.generate_candidates_batch()
    assert out["x"].shape == (6, 5, drt._plan.n) and (out["status"] >= 0).all()
    # step-store scoring equals the same x uploaded
    plan, tau, opts = drt._candidate_peak_request("test", None)
    up = drt._score_candidates(plan, out["x"], tau, opts, None)
    for k, name in (("llh", "llh"), ("num_peaks", "count"), ("peak_index", "peak_index"), ("peak_heights", "heights"),
                    ("prominences", "prominences")):
        assert np.array_equal(out[k], up[name], equal_nan=True), k
    # member b equals the batch of that one spectrum
    for b in (0, 3):
        one = DRT(warn=False)
        one.fit_eis_batch(FREQ71, z[b:b + 1])
        o1 = one.generate_candidates_batch()
        for k in ("x", "llh", "bic", "num_peaks", "peak_index", "peak_heights", "prominences"):
            assert np.array_equal(out[k][:, b], o1[k][:, 0], equal_nan=True), (k, b)
        assert out["best"][b]["keys"] == o1["best"][0]["keys"]
        for k, v in out["best"][b]["table"].items():
            assert np.array_equal(v, o1["best"][0]["table"][k]), (k, b)
    # ... and the single-fit method restricted to the last iterate of the fit and of every restart
    single = DRT(warn=False)
    single.fit_eis(FREQ71, z[0])
    cd = single.generate_candidates()
    last = [i for i in range(len(cd["x"])) if i + 1 == len(cd["x"]) or cd["hypers"][i + 1] is not cd["hypers"][i]]
    assert len(last) == 6
    assert np.array_equal(cd["x"][last], out["x"][:, 0]) and np.array_equal(cd["llh"][last], out["llh"][:, 0])
    assert np.array_equal(cd["num_peaks"][last], out["num_peaks"][:, 0]) and np.array_equal(cd["bic"][last], out["bic"][:, 0])
    # evaluate_bic is upstream's: the live solution under the fit's own est_weights, not the candidates' re-estimated weights
    llh = drt.evaluate_obs_llh_rss_batch()[0]
    counts = np.array([len(p) for p in drt.find_peaks_batch()])
    assert np.array_equal(drt.evaluate_bic_batch(), (drt._plan.ns + 4 * counts) * np.log(71) - 2 * llh)
    assert np.array_equal(counts, out["num_peaks"][2]) and not np.array_equal(llh, out["llh"][2])


# ---- 8. a step that failed is no candidate; the refusals of hipdrt_plan_pfrt_restore_s ---------------------------------------------
def test_a_recorded_step_that_failed_is_no_candidate_whatever_later_steps_did():
    """member 1 is handed NaN weights before the second step, so that step fails for it (a numerical failure status, as a NaN
    spectrum gives); the third step starts every member from the fit's state again and succeeds.  Scoring the steps: slot (1, 1)
    is empty with the step's negative status, every other slot is that of the same x uploaded."""
    from hipdrt import synth
    from hipdrt.models import DRT
    drt = DRT(warn=False)
    drt.fit_eis_batch(FREQ71, synth.zarc2_batch(FREQ71, 3, first_seed=7))
    plan = drt._plan
    ln_tau = np.log(drt.get_tau_eval(10))
    base = plan.download(s_vectors=True)
    plan.pfrt_begin(3)
    plan.pfrt_record()
    bad = base["weights"].copy()
    bad[1] = np.nan
    drt.continue_from_init(weights=bad, max_iter=2)
    plan.pfrt_record()
    drt.continue_from_init(x_init=base["x"], rho_vector=base["rho"], s_vectors=base["s_vectors"], weights=base["weights"], max_iter=2)
    plan.pfrt_record()
    recorded = np.array([plan.pfrt_step_state(c)["status"] for c in range(3)])
    assert recorded[1, 1] < 0 and (np.delete(recorded, 4) >= 0).all() and (plan.download()["status"] >= 0).all()
    xs = np.array([plan.pfrt_step_state(c)["x"] for c in range(3)])
    a = plan.score_candidates(None, ln_tau_find=ln_tau)
    b = plan.score_candidates(np.nan_to_num(xs), ln_tau_find=ln_tau)
    np.testing.assert_array_equal(a["status"], recorded)
    for k in set(a) - {"status"}:
        v = a[k][1, 1]
        assert np.array_equal(v, np.full_like(v, -1 if v.dtype == np.int32 else np.nan), equal_nan=True), k
        keep = np.ones((3, 3), dtype=bool)
        keep[1, 1] = False
        assert np.array_equal(a[k][keep], b[k][keep], equal_nan=True) and np.isfinite(a[k][keep].astype(float)).any(), k


def test_restore_s_and_its_refusals(fit5, ctx):
    from hipdrt import _ffi, synth
    from hipdrt.models import DRT
    drt = DRT(warn=False)
    drt.fit_eis_batch(FREQ71, synth.zarc2_batch(FREQ71, 2, first_seed=7))
    plan = drt._plan
    with pytest.raises(_ffi.HipDrtError, match="step out of range"):
        plan.pfrt_restore_s(0, 2.0)                     # nothing recorded yet
    plan.pfrt_begin(2)
    plan.pfrt_record()
    s0 = plan.download(s_vectors=True)["s_vectors"]
    drt.continue_from_init(weight_factor=0.5, max_iter=2)
    assert not np.array_equal(plan.download(s_vectors=True)["s_vectors"], s0)
    plan.pfrt_restore_s(0, 4.0)
    assert np.array_equal(plan.download(s_vectors=True)["s_vectors"], s0 * 4.0)
    for step in (-1, 1):
        with pytest.raises(_ffi.HipDrtError, match="step out of range"):
            plan.pfrt_restore_s(step, 2.0)
    for factor in (0.0, -1.0, np.nan, np.inf):
        with pytest.raises(_ffi.HipDrtError, match="factor must be positive and finite"):
            plan.pfrt_restore_s(0, factor)
    assert np.array_equal(plan.download(s_vectors=True)["s_vectors"], s0 * 4.0)     # a refused call changes nothing
    fresh = _ffi.Plan(ctx, plan.freq, plan.tau, drt.tau_epsilon, mode=_ffi.MODE_TRAPZ, capacity=2)
    with pytest.raises(_ffi.HipDrtError, match="no fitted batch"):
        fresh.pfrt_restore_s(0, 2.0)
