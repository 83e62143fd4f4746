"""GPU: the probability function of relaxation times of a PFRT fit on the device (csrc/pfrt.hip; hipdrt_plan_pfrt_begin / _record,
hipdrt_plan_get_step_p_matrix, hipdrt_plan_predict_pfrt and the two debug hooks) and the DRT methods on top (predict_pfrt_batch,
predict_pfrt, step_p_matrix, fit_observations_pfrt(predict_pfrt_kw=)).

1. pfrt_step_kernel alone against hipdrt.models.pfrt on integer rows, integer heights and prominences and variances that are powers
   of four: the positions compare exactly, the probabilities at 1e-13 (the kernel's erfc is the device library's, the statement's
   math.erfc; every argument is the same bits in both);
2. pfrt_combine_kernel alone against the statement, bounds below; the refusal of a 2049-point grid;
3. the step P against the oracle's estimate_weights + calculate_qp_l2_matrix on the recorded state, and against the reference's;
4. the whole chain against the statement on rows formed in numpy from the plan's own recorded x and step P;
5. the chain against the reference's recorded run (tools/make_pfrt_golden.py), bounds from tests/pfrt_bounds.json;
6. a spectrum alone and as member 2 of a batch of 5 gives the same bits; 7. failed fits and refusals; 8. the fit's results are the
   same bits with and without a prediction in between; 9. the map level.

Bounds of 2 (u = 2^-53; nothing is measured from the kernel).  With L the largest |llh| of a step, the kernel and the statement
form llh = (c - alpha_n ln(beta_0 + rss / 2)) + slw in the same order but with different log routines: 4 u L absolute covers the
logarithm's rounding through the product and the two sums.  The exponent (log_post - max) n_eff inherits n_eff times twice that
(both operands of the difference) and is itself below 745 in magnitude for any weight that does not underflow, which exp turns
into a relative error of 745 u plus its own rounding: e_post = (8 n_eff L + 750) u.  The area and the sum of the weights add S
positive terms each in the same ascending order in both implementations: (S + 2) u each.  So a posterior weight is off by at most
e_post + (S + 4) u relative, raw_pfrt (S positive terms, quotient of two such sums) by e_raw = 2 (e_post + (S + 4) u) + (S + 3) u
of the row's peak.  Smoothing adds np positive terms (np u) whose factors exp(-t^(2 order)) matter only while they exceed u, i.e.
t^(2 order) < 37, where pow (4 u relative on the device) and exp give 37 * 5 u: e_smooth = e_raw + (np + 190) u.  Integration sums
at most nout positive terms once more, (nout + 2) u, and its discrete decisions (v >= threshold) are the same as long as no value
lies within 1e-9 relative of the threshold, which the test asserts on the statement's values.  Normalisation divides by the
maximum, which carries the same relative error: twice the bound so far plus 2 u.

Bound of 3.  With r = rm x - rv and d_j = (n + 2) u (|rm| |x| + |rv|)_j the rounding of r_j in any order of summation, r_j^2 is off
by 2 |r_j| d_j + d_j^2, s_hat = vmm r^2 by vmm applied to that plus (m + 2) u s_hat, the weight s_hat^-1/2 by half the relative
error of s_hat plus 2 u, and an entry of (w rm)'(w rm) + L2, a sum of m products over the squared weights, by twice the largest
relative error of a weight plus (m + 4) u of the diagonal's peak; the penalty part is formed in the same order (4 u).

Bound of 4: test_gpu_peaks.py's prob_bound, 0.49 times the relative error of sigma plus 1e-13.  Here sigma^2 comes from numpy's
inverse of the downloaded step P against the device's Cholesky factor of the same matrix: both are backward stable, so either is
off by at most about n cond(P) u relative (Higham 10.1), sigma by half the sum of the two.
"""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, parity

from hipdrt.models import peaks, pfrt

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
FITS = {"plain": dict(), "nn": dict(nonneg=False)}
OPTION_SETS = {"default": dict(), "raw": dict(smooth=False, normalize=False), "int": dict(integrate=True), "tau181": dict()}


@pytest.fixture(scope="module")
def ctx():
    from hipdrt import _ffi
    return _ffi.get_context(0)


@pytest.fixture(scope="module")
def golden():
    return np.load(os.path.join(GOLDEN, "refrun_pfrt_golden71x91.npz"))


@pytest.fixture(scope="module")
def spectrum():
    g = np.load(os.path.join(GOLDEN, "ref_test_drt_fit_eis.npz"))
    return np.asarray(g["freq"], dtype=float), np.asarray(g["z"], dtype=complex)


def ref_parity(label, got, ref):
    """conftest.parity against the reference's recorded values, the bound from tests/pfrt_bounds.json (label -> [measured on the GPU,
    bound = 20 x measured rounded up to 1 / 2 / 5 x 10^k]); 1e-7, the project's stated parity, for a label not measured yet"""
    with open(os.path.join(ROOT, "tests", "pfrt_bounds.json")) as f:
        entry = json.load(f).get(label)
    return parity(label, got, ref, bound=1e-7 if entry is None else float(entry[1]), label=label)


# ---- 1. pfrt_step_kernel alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 37])
@pytest.mark.parametrize("neval", [1, 2, 63, 64, 65, 257, 2048])
def test_step_kernel_against_the_statement(ctx, neval, B):
    rng = np.random.default_rng(100 * neval + B)
    fxx = rng.integers(-40, 41, (B, neval)).astype(float)
    f = rng.integers(-3, 4, (B, neval)).astype(float)
    var_f, var_fxx = 4.0 ** rng.integers(0, 4, (B, neval)), 4.0 ** rng.integers(0, 6, (B, neval))
    height, prominence = 3.0, 7.0
    cases = [dict(fxx_var_floor=0.0), dict(fxx_var_floor=16.0)]
    if neval >= 4:
        li, ri = neval // 4, neval - 1 - neval // 4
        cases += [dict(fxx_var_floor=1e-5, ext_left=li, ext_right=ri), dict(fxx_var_floor=4.0, ext_left=ri, ext_right=li)]
    total = 0
    for search in (1, -1, 0):
        dense = [peaks.find_peaks_dense(fxx[b], f[b], search=search, method=0, height=height, prominence=prominence) for b in range(B)]
        sg = np.array([d["peak_sign"] for d in dense])
        ht, pr = np.array([d["heights"] for d in dense]), np.array([d["prominences"] for d in dense])
        for kw in cases:
            out = ctx.debug_pfrt_step(sg, ht, pr, f, var_f, var_fxx, var_floor=kw["fxx_var_floor"], ext_left=kw.get("ext_left", -1),
                                      ext_right=kw.get("ext_right", -1))
            ref = np.array([pfrt.step_peak_probs(f[b], fxx[b], var_f[b], var_fxx[b], search, height, prominence, **kw) for b in range(B)])
            # (a peak whose f is zero has probability zero of |f| > 0: the positions are those of the peaks with f != 0)
            np.testing.assert_array_equal(out != 0, ref != 0, err_msg=f"{search} {kw}")
            np.testing.assert_array_equal((sg != 0) & (f != 0), ref != 0)
            np.testing.assert_allclose(out, ref, rtol=0, atol=1e-13, err_msg=f"{search} {kw}")
            total += int(np.count_nonzero(ref))
    assert total > 0 or neval < 63          # the comparison is not vacuous


# ---- 2. pfrt_combine_kernel alone ---------------------------------------------------------------------------------------------------
def combine_case(rng, S, npf, nout, B=3, m=142):
    step = rng.choice([0.0, 0.25, 0.5, 1.0], size=(S, B, npf), p=[0.9, 0.04, 0.03, 0.03])
    # (neighbouring likelihoods a few units apart, as a regularisation path's are: several steps carry weight)
    rss = rng.uniform(50.0, 5000.0, (1, B)) * np.exp(np.cumsum(rng.uniform(-0.02, 0.02, (S, B)), axis=0))
    slw = rng.uniform(-700.0, 700.0, (1, B)) + np.cumsum(rng.uniform(-3.0, 3.0, (S, B)), axis=0)
    factors = np.logspace(-1, 1, S) if S > 1 else np.array([0.7])
    ltp = np.linspace(-18.0, 7.0, npf) if npf > 1 else np.array([0.3])
    lto = np.linspace(-17.0, 6.0, nout) if nout > 1 else np.array([0.25])
    return step, rss, slw, factors, ltp, lto, m


@pytest.mark.parametrize("grid", [(1, 1), (64, 65), (111, 181), (2048, 2048)])
@pytest.mark.parametrize("S", [1, 2, 11, 64])
def test_combine_kernel_against_the_statement(ctx, S, grid):
    from hipdrt import _ffi
    npf, nout = grid
    step, rss, slw, factors, ltp, lto, m = combine_case(np.random.default_rng(1000 * S + npf), S, npf, nout)
    B = step.shape[1]
    llh = pfrt.step_llh(rss, slw, m)
    n_eff, thr = 0.5, 1e-6
    e_post = (8 * n_eff * float(np.abs(llh).max()) + 750) * U
    e_raw = 2 * (e_post + (S + 4) * U) + (S + 3) * U
    for smooth in (True, False):
        for integrate in (False, True):
            for normalize in ((True, False) if (smooth and not integrate) else (True,)):
                no = nout if smooth else npf
                opts = _ffi.pfrt_opts(smooth=smooth, integrate=integrate, integrate_threshold=thr, normalize=normalize,
                                      n_eff_factor=n_eff)
                out = ctx.debug_pfrt_combine(step, rss, slw, factors, m, ltp, lto if smooth else None, opts)
                assert out["pfrt"].shape == (B, no)
                e_out = e_raw + ((npf + 190) * U if smooth else 0.0)
                e_fin = e_out + ((no + 2) * U if integrate else 0.0)
                e_fin = 2 * e_fin + 2 * U if normalize else e_fin
                for b in range(B):
                    post = pfrt.step_posterior(factors, llh[:, b], n_eff_factor=n_eff)
                    raw = pfrt.combine(post, step[:, b])
                    sm = pfrt.finish(raw, ltp, lto if smooth else None, smooth_on=smooth, integrate=False, normalize=False)
                    assert (np.abs(sm - thr) > 1e-9 * thr).all(), "the test's own row puts a value on the integration threshold"
                    ref = pfrt.finish(raw, ltp, lto if smooth else None, smooth_on=smooth, integrate=integrate,
                                      integrate_threshold=thr, normalize=normalize)
                    tag = f"S {S} grid {grid} smooth {smooth} integrate {integrate} normalize {normalize} b {b}"
                    assert (np.abs(out["post_prob"][:, b] - post) <= (e_post + (S + 4) * U) * post.max()).all(), tag
                    np.testing.assert_array_equal(out["raw_pfrt"][b] != 0, raw != 0, err_msg=tag)
                    assert (np.abs(out["raw_pfrt"][b] - raw) <= e_raw * max(raw.max(), 1e-300)).all(), tag
                    if np.isnan(ref).any():              # an all-zero row, normalised
                        assert np.isnan(ref).all() and np.isnan(out["pfrt"][b]).all(), tag
                        continue
                    if integrate:
                        np.testing.assert_array_equal(out["pfrt"][b] != 0, ref != 0, err_msg=tag)
                    assert (np.abs(out["pfrt"][b] - ref) <= e_fin * max(np.abs(ref).max(), 1e-300)).all(), tag


def test_combine_hook_refuses_a_grid_of_2049_points(ctx):
    from hipdrt import _ffi
    step, rss, slw, factors, ltp, lto, m = combine_case(np.random.default_rng(5), 2, 2049, 64)
    with pytest.raises(_ffi.HipDrtError, match="2048"):
        ctx.debug_pfrt_combine(step, rss, slw, factors, m, ltp, lto)
    step, rss, slw, factors, ltp, lto, m = combine_case(np.random.default_rng(6), 2, 64, 2049)
    with pytest.raises(_ffi.HipDrtError, match="2048"):
        ctx.debug_pfrt_combine(step, rss, slw, factors, m, ltp, lto)
    with pytest.raises(_ffi.HipDrtError, match="neval_out == neval_pfrt"):
        ctx.debug_pfrt_combine(step[:, :, :64], rss, slw, factors, m, ltp, lto[:65], _ffi.pfrt_opts(smooth=False))


# ---- the fits the remaining tests share -----------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fit3(spectrum):
    """pfrt_fit_eis_batch of the fixture spectrum and two synthetic members"""
    from hipdrt import synth
    from hipdrt.models import DRT
    freq, z = spectrum
    zb = np.vstack([z[None, :], synth.zarc2_batch(freq, 2, first_seed=40)])
    drt = DRT(warn=False)
    pr = drt.pfrt_fit_eis_batch(freq, zb)
    assert (pr["status"] >= 0).all() and drt._plan.pfrt_steps() == 11
    return drt, zb, pr


# ---- 3. the step P --------------------------------------------------------------------------------------------------------------------
def test_step_p_against_the_oracle_and_the_reference(fit3, golden):
    from oracle import drt_oracle as orc
    drt, zb, pr = fit3
    plan = drt._plan
    rm, vmm, rv_all = plan.get("rm"), plan.get("vmm"), plan.get("rv")
    pen = [plan.get(k) for k in ("m0", "m1", "m2")]
    n, m, ns = plan.n, plan.m, plan.ns
    hypers = orc.get_default_hypers()
    hypers["l2_lambda_0"] = hypers["l2_lambda_0"] / pr["factors"][0]        # the hypers of the first step serve every step P
    before = plan.p_matrix(0)
    for s in (0, 5, 10):
        st = plan.pfrt_step_state(s)
        np.testing.assert_array_equal(st["x"], pr["step_x"][s])
        for b in range(3):
            x, rv = st["x"][b], rv_all[b]
            w = orc.estimate_weights(x, rv, vmm, rm)
            wrm = w[:, None] * rm
            ref = orc.calculate_qp_l2_matrix(hypers, st["rho"][b], pen, list(st["s_vectors"][b]), ns) + wrm.T @ wrm
            r = rm @ x - rv
            d = (n + 2) * U * (np.abs(rm) @ np.abs(x) + np.abs(rv))
            s_hat = vmm @ r ** 2
            e_s = np.abs(vmm) @ (2 * np.abs(r) * d + d ** 2) / s_hat + (m + 2) * U
            bound = 2 * (0.5 * float(e_s.max()) + 2 * U) + (m + 8) * U
            got = drt.step_p_matrix(s, b)
            parity(f"step_p_oracle_s{s}_b{b}", got, ref, bound=bound)
            if b == 0:
                k = list(golden["p_steps"]).index(s)
                ref_parity(f"pfrt:step_p_s{s}", got, golden["plain_step_p_mat"][k])
    # the step P is not the plan's final P, and reading it leaves that one alone
    assert not np.array_equal(drt.step_p_matrix(10, 0), before)
    drt.predict_pfrt_batch()
    assert np.array_equal(plan.p_matrix(0), before)


# ---- 4. the whole chain against the statement -------------------------------------------------------------------------------------------
def test_chain_against_the_statement_on_rows_from_the_same_plan(fit3, ctx):
    drt, zb, pr = fit3
    plan = drt._plan
    tau = drt.get_tau_eval(10)
    lt, lb = np.log(tau), np.log(drt.basis_tau)
    li, ri = drt._extend_var_indices(tau)
    ns, S = plan.ns, len(pr["factors"])
    E0, E2 = ctx.func_eval_matrix(lb, lt, drt.tau_epsilon, 0), ctx.func_eval_matrix(lb, lt, drt.tau_epsilon, 2)
    area = np.pi ** 0.5 / drt.tau_epsilon
    tot, info = drt.predict_pfrt_batch(return_info=True)
    assert tot.shape == (3, len(tau)) and (info["status"] >= 0).all()
    checked = 0
    for b in range(3):
        cs = pr["coefficient_scale"][b]
        rows = {k: [] for k in ("f", "fxx", "var_f", "var_fxx")}
        rel, llh, on_threshold = 0.0, [], False
        for s in range(S):
            st = plan.pfrt_step_state(s)
            x = st["x"][b, ns:] * cs
            rp = np.sum(x) * area
            if s == 0:
                rp0 = rp
            P = drt.step_p_matrix(s, b)
            cov = np.linalg.inv(P)[ns:, ns:] * cs ** 2
            rel = max(rel, plan.n * float(np.linalg.cond(P)) * U)
            rows["f"].append(E0 @ x / rp); rows["fxx"].append(E2 @ x / rp)
            rows["var_f"].append(np.einsum("ij,jk,ik->i", E0, cov, E0) / rp0 ** 2)
            rows["var_fxx"].append(np.einsum("ij,jk,ik->i", E2, cov, E2) / rp0 ** 2)
            llh.append(pfrt.step_llh(st["rss"][b], st["sum_log_w"][b], plan.m))
            for sgn in (1,):
                idx, pk = peaks.find_peaks_1d(-sgn * rows["fxx"][-1])
                for vals, thr in ((pk["peak_heights"], 1e-3), (pk["prominences"], 5e-3)):
                    on_threshold |= bool((np.abs(vals - thr) <= 0.01 * thr).any())
        np.testing.assert_allclose(llh, pr["step_llh"][:, b], rtol=1e-12)
        if on_threshold:
            continue
        checked += 1
        rows = {k: np.array(v) for k, v in rows.items()}
        ref = pfrt.predict_pfrt_rows(pr["factors"], np.array(llh), rows["f"], rows["fxx"], rows["var_f"], rows["var_fxx"], lt,
                                     ext_left=li, ext_right=ri)
        bound = 0.49 * rel + 1e-13
        print(f"member {b}: relative error of sigma up to {rel:.1e}, probability bound {bound:.1e}")
        np.testing.assert_array_equal(info["step_pfrt"][:, b] != 0, ref["step_pfrt"] != 0)
        assert (np.abs(info["step_pfrt"][:, b] - ref["step_pfrt"]) <= bound).all(), b
        # (the posterior weights come from the same sums: raw and the smoothed row are averages of the step probabilities with
        # non-negative weights, so they inherit the bound relative to their peak, doubled by the normalisation)
        assert (np.abs(info["raw_pfrt"][b] - ref["raw_pfrt"]) <= bound + 1e-12).all(), b
        # (a row of the smoothing matrix sums to less than 1.5 on this grid, and the smoothed maximum is at least the raw one)
        assert (np.abs(tot[b] - ref["pfrt"]) <= 3 * (bound + 1e-12) / max(ref["raw_pfrt"].max(), 1e-300)).all(), b
    assert checked >= 2
    # the single-spectrum form is a member of the batch and leaves upstream's keys behind
    one = drt.predict_pfrt(b=1)
    assert np.array_equal(one, tot[1]) and np.array_equal(drt.pfrt_result["raw_pfrt"], info["raw_pfrt"][1])
    assert np.array_equal(drt.pfrt_result["step_pfrt"], info["step_pfrt"][:, 1]) and np.array_equal(drt.pfrt_result["tau_pfrt"], tau)


# ---- 5. against the reference's run ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", list(FITS))
def test_fit_against_the_reference_run(spectrum, golden, tag):
    from hipdrt.models import DRT
    freq, z = spectrum
    drt = DRT(warn=False)
    pr = drt.pfrt_fit_eis_batch(freq, z[None, :], **FITS[tag])
    tau = golden[f"{tag}_tau_pfrt"]
    np.testing.assert_allclose(drt.get_tau_eval(10), tau, rtol=1e-13)
    np.testing.assert_array_equal(pr["factors"], golden[f"{tag}_factors"])
    tot, info = drt.predict_pfrt_batch(return_info=True)
    ref_steps = golden[f"{tag}_step_pfrt"]
    np.testing.assert_array_equal(info["step_pfrt"][:, 0] != 0, ref_steps != 0)
    assert int(np.argmax(tot[0])) == 38
    for name in ("step_pfrt", "raw_pfrt"):
        got = info[name][:, 0] if name == "step_pfrt" else info[name][0]
        ref_parity(f"pfrt:{tag}:{name}", got, golden[f"{tag}_{name}"])
    for name, kw in OPTION_SETS.items():
        kw = dict(kw, tau=golden["tau181"]) if name == "tau181" else kw
        out = drt.predict_pfrt(**kw)
        ref = golden[f"{tag}_pfrt_{name}"]
        if name == "int":
            np.testing.assert_array_equal(out != 0, ref != 0)
        ref_parity(f"pfrt:{tag}:pfrt_{name}", out, ref)


# ---- 6. batch independence -------------------------------------------------------------------------------------------------------------
def test_alone_and_as_member_2_of_5_give_the_same_bits(spectrum):
    from hipdrt import synth
    from hipdrt.models import DRT
    freq, z = spectrum
    zb = synth.zarc2_batch(freq, 5, first_seed=70)
    zb[2] = z
    one, many = DRT(warn=False), DRT(warn=False)
    p1, p5 = one.pfrt_fit_eis_batch(freq, z[None, :]), many.pfrt_fit_eis_batch(freq, zb)
    assert np.array_equal(p1["step_x"][:, 0], p5["step_x"][:, 2]), "the fit itself differs between batch sizes: nothing to compare"
    for kw in (dict(), dict(smooth=False, normalize=False), dict(integrate=True), dict(tau=np.logspace(-7, 2, 181))):
        t1, i1 = one.predict_pfrt_batch(return_info=True, **kw)
        t5, i5 = many.predict_pfrt_batch(return_info=True, **kw)
        assert np.array_equal(t1[0], t5[2], equal_nan=True), kw
        assert np.array_equal(i1["raw_pfrt"][0], i5["raw_pfrt"][2]) and np.array_equal(i1["step_pfrt"][:, 0], i5["step_pfrt"][:, 2])
        assert np.array_equal(i1["post_prob"][:, 0], i5["post_prob"][:, 2]) and i1["status"][0] == i5["status"][2]
    for s in (0, 10):
        assert np.array_equal(one.step_p_matrix(s, 0), many.step_p_matrix(s, 2))


# ---- 7. failure handling and refusals -----------------------------------------------------------------------------------------------------
def test_failed_member_has_nan_rows_and_leaves_its_neighbours_alone(spectrum):
    from hipdrt import synth
    from hipdrt.models import DRT
    freq, _ = spectrum
    z = synth.zarc2_batch(freq, 4, first_seed=300)
    zbad = z.copy()
    zbad[2] = np.nan
    good, bad = DRT(warn=False), DRT(warn=False)
    good.pfrt_fit_eis_batch(freq, z, factors=np.logspace(-0.5, 0.5, 3))
    pr = bad.pfrt_fit_eis_batch(freq, zbad, factors=np.logspace(-0.5, 0.5, 3))
    assert pr["status"][2] < 0
    tg, ig = good.predict_pfrt_batch(return_info=True)
    tb, ib = bad.predict_pfrt_batch(return_info=True)
    assert ib["status"][2] < 0 and (np.delete(ib["status"], 2) >= 0).all()
    assert np.isnan(tb[2]).all() and np.isnan(ib["raw_pfrt"][2]).all() and np.isnan(ib["step_pfrt"][:, 2]).all()
    assert np.isnan(ib["post_prob"][:, 2]).all()
    keep = [0, 1, 3]
    assert np.array_equal(tb[keep], tg[keep]) and np.array_equal(ib["raw_pfrt"][keep], ig["raw_pfrt"][keep])
    assert np.array_equal(ib["step_pfrt"][:, keep], ig["step_pfrt"][:, keep])
    assert np.isfinite(tg).all()


def test_refusals(spectrum, fit3):
    from hipdrt import _ffi
    from hipdrt.models import DRT
    freq, z = spectrum
    drt = fit3[0]
    for name, value in (("distance", 3), ("width", 2), ("wlen", 11), ("threshold", 0.1)):
        with pytest.raises(NotImplementedError, match=name):
            drt.predict_pfrt_batch(find_peaks_kw={name: value})
    with pytest.raises(ValueError, match="recorded"):
        drt._plan.predict_pfrt(np.logspace(-1, 1, 7), np.log(drt.get_tau_eval(10)))
    with pytest.raises(_ffi.HipDrtError, match="2048"):
        drt.predict_pfrt_batch(tau_pfrt=np.logspace(-8, 3, 2049), extend_var=False)
    with pytest.raises(_ffi.HipDrtError, match="2048"):
        drt.predict_pfrt_batch(tau=np.logspace(-8, 3, 2049))
    with pytest.raises(_ffi.HipDrtError, match="step out of range"):
        drt.step_p_matrix(11, 0)
    plain = DRT(warn=False)
    with pytest.raises(RuntimeError, match="PFRT fit"):
        plain.predict_pfrt()
    plain.fit_eis_batch(freq, z[None, :])
    with pytest.raises(RuntimeError, match="PFRT fit"):
        plain.predict_pfrt_batch()
    sneg = DRT(warn=False)
    sneg._pfrt_prepared([(None, None, None, freq, z)], [0.5, 1.0], 10, 20, 1e-2, True, dict(series_neg=True))
    assert sneg.series_neg and sneg._plan.pfrt_steps() == 2
    with pytest.raises(NotImplementedError, match="series_neg"):
        sneg.predict_pfrt_batch()
    prepared = DRT(warn=False)
    prepared._pfrt_prepared([(None, None, None, freq, z)], [0.5, 1.0], 10, 20, 1e-2, True, dict(solve_rp=True))
    assert isinstance(prepared._plan, _ffi.PreparedPlan) and prepared._plan.pfrt_steps() == 2
    with pytest.raises(NotImplementedError, match="prepared"):
        prepared.predict_pfrt_batch()
    with pytest.raises(_ffi.HipDrtError, match="not supported"):
        prepared._plan.predict_pfrt([0.5, 1.0], np.log(prepared.get_tau_eval(10)))
    p = prepared.step_p_matrix(1, 0)              # step recording and the step P do work for a prepared plan
    assert p.shape == (prepared._plan.n,) * 2 and np.isfinite(p).all() and np.allclose(p, p.T, rtol=1e-12, atol=0)


# ---- 8. the fit's own results do not change -------------------------------------------------------------------------------------------
def test_fit_results_are_the_same_bits_with_a_prediction_in_between(spectrum, fit3):
    from hipdrt.models import DRT
    freq, _ = spectrum
    drt0, zb, pr0 = fit3
    keys = {"factors", "step_x", "step_llh", "step_iters", "status", "coefficient_scale", "basis_tau"}
    drt = DRT(warn=False)
    first = dict(drt.pfrt_fit_eis_batch(freq, zb))
    assert set(first) == keys
    drt.predict_pfrt_batch(return_info=True)          # (adds upstream's keys to pfrt_result, as upstream's method does)
    drt.step_p_matrix(3, 1)
    second = drt.pfrt_fit_eis_batch(freq, zb)
    assert set(second) == keys
    for k in ("step_x", "step_llh", "step_iters", "status", "coefficient_scale"):
        assert np.array_equal(first[k], second[k]), k
        assert np.array_equal(first[k], pr0[k]), k


# ---- 9. the map level -----------------------------------------------------------------------------------------------------------------
def test_map_level_fills_obs_pfrt(spectrum):
    from hipdrt import mapping, synth
    from hipdrt.models import DRT
    freq, _ = spectrum
    z = synth.zarc2_batch(freq, 4, first_seed=500)
    sup = np.logspace(-8, 2, 101)
    factors = np.logspace(-0.5, 0.5, 3)
    obs = [(None, (freq, z[b])) for b in range(4)]
    drt = DRT(warn=False, tau_supergrid=sup)
    x0, sp0, r0 = mapping.fit_observations_pfrt(drt, obs, sup, pfrt_factors=factors)
    x1, sp1, r1 = mapping.fit_observations_pfrt(drt, obs, sup, pfrt_factors=factors, predict_pfrt_kw={})
    assert set(r1) - set(r0) == {"obs_pfrt", "obs_raw_pfrt"} and np.array_equal(x0, x1)
    assert np.array_equal(r0["step_llh"], r1["step_llh"])
    direct = DRT(warn=False, tau_supergrid=sup)
    direct.pfrt_fit_eis_batch(freq, z, factors=factors)
    tot, info = direct.predict_pfrt_batch(tau=sup, tau_pfrt=sup, return_info=True)
    assert r1["obs_pfrt"].shape == (4, 101)
    assert np.array_equal(r1["obs_pfrt"], tot, equal_nan=True) and np.array_equal(r1["obs_raw_pfrt"], info["raw_pfrt"])
