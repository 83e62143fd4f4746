"""GPU: model evaluation of a fitted batch on the device (csrc/predict.hip, func_eval_kernel in csrc/matrices.hip;
hipdrt_func_eval_matrix, hipdrt_plan_predict_drt, hipdrt_plan_predict_z, hipdrt_plan_predict_resistances,
hipdrt_debug_apply_rows) and the DRT methods on top.

1. the evaluation-matrix kernel against its numpy statement;
2. the row-application kernel alone on random host data against a product formed in np.longdouble, with a derived bound;
3. a spectrum predicted alone and inside a batch gives the same bits;
4. the device against hipdrt.models.predict applied to the coefficients downloaded from the same plan (isolates the kernels from
   fit parity), against kk_screen's prediction, and the band against the existing variance method;
5. the device against the reference's recorded runs (tools/make_predict_golden.py);
6. a failed fit gives a NaN row and a negative status and leaves the other rows alone;
7. the refusals.

The bound of 2 and 4.  For y_i = scale * sum_j E_ij x_j accumulated in floating point in ANY order, with or without fused
multiply-add, |err_i| <= gamma_K * scale * sum_j |E_ij| |x_j| with gamma_K = K u / (1 - K u), u = 2^-53 (Higham, Accuracy and
Stability of Numerical Algorithms, 3.1).  The scale multiplication, the store and the (1 - K u) denominator add a few more u:
(K + 8) u covers them.  1e-300 absorbs products that underflow.  Nothing here is measured from the kernel."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, parity

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
RTOL = 1e-12                      # the RTOL of test_gpu_matrices.py


@pytest.fixture(scope="module")
def ctx():
    from hipdrt import _ffi
    return _ffi.get_context(0)


def grids(nb, ne):
    """natural-log grids: a basis over nine decades and evaluation points reaching 1.5 decades beyond it on both sides"""
    return np.linspace(np.log(1e-7), np.log(1e2), nb), np.linspace(-8.5 * np.log(10), 3.5 * np.log(10), ne)


def eval_matrix_numpy(basis, ev, eps, order):
    y = ev[:, None] - basis[None, :]
    phi = np.exp(-(eps * y) ** 2)
    if order == 0:
        return phi
    if order == 1:
        return -2 * eps ** 2 * y * phi
    return (-2 * eps ** 2 + 4 * eps ** 4 * y ** 2) * phi


# ---- 1. evaluation matrix ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("order", [0, 1, 2])
@pytest.mark.parametrize("eps", [4.3429, 22.19])
def test_eval_matrix_kernel(ctx, eps, order):
    for nb in (1, 5, 16, 17, 91):
        for ne in (1, 15, 16, 17, 241):
            basis, ev = grids(nb, ne)
            ref = eval_matrix_numpy(basis, ev, eps, order)
            out = ctx.func_eval_matrix(basis, ev, eps, order)
            assert out.shape == (ne, nb)
            atol = 1e-300 + (RTOL * np.abs(ref).max() if order else 0.0)     # the polynomial factor cancels near its roots
            np.testing.assert_allclose(out, ref, rtol=RTOL, atol=atol, err_msg=f"nb={nb} ne={ne}")


def test_eval_matrix_refuses_other_orders(ctx):
    from hipdrt import _ffi
    with pytest.raises(_ffi.HipDrtError, match="order"):
        ctx.func_eval_matrix(np.zeros(3), np.zeros(2), 1.0, 3)


# ---- 2. row application alone ----------------------------------------------------------------------------------------------------
B_SET, R_SET, OFFSETS = (1, 5, 17, 37), (1, 15, 16, 17, 241), (0, 2, 3)


@pytest.mark.parametrize("K", [1, 3, 4, 5, 93, 514])
def test_apply_rows_kernel_alone(ctx, K):
    """hipdrt_debug_apply_rows (the kernel as the predictions launch it) on random data whose magnitudes span 14 decades; the
    hook itself fails when the kernel touches the marker-filled row and columns around its B x r output block"""
    rng = np.random.default_rng(7000 + K)
    bmax, rmax = max(B_SET), max(R_SET)
    basis, ev = grids(K, rmax)
    e_full = ctx.func_eval_matrix(basis, ev, 4.3429, 1)                   # (241, K) from the kernel of test 1, signed entries
    worst = 0.0
    for off in OFFSETS:
        ldx = K + off + 3
        x_full = rng.standard_normal((bmax, ldx)) * 10.0 ** rng.uniform(-7, 7, (bmax, ldx))
        scale_full = 10.0 ** rng.uniform(-2, 2, bmax)
        xl = x_full[:, off:off + K].astype(np.longdouble)
        ref_full = xl @ e_full.astype(np.longdouble).T                   # (37, 241), shared by every B and r below
        mag_full = np.abs(xl) @ np.abs(e_full).astype(np.longdouble).T
        for B in B_SET:
            for r in R_SET:
                scale = None if (B + r + off) % 2 else scale_full[:B]
                out = ctx.debug_apply_rows(x_full[:B], e_full[:r], col_offset=off, scale=scale)
                sc = np.ones(B) if scale is None else scale
                err = np.abs(out.astype(np.longdouble) - sc[:, None] * ref_full[:B, :r])
                bound = (K + 8) * U * sc[:, None] * mag_full[:B, :r] + 1e-300
                ratio = float((err / bound).max())
                worst = max(worst, ratio)
                assert ratio <= 1.0, f"K={K} B={B} r={r} offset={off}: error {ratio:.3g} of the bound"
    print(f"apply_rows K={K}: worst error {worst:.3g} of the derived bound")


def test_apply_rows_refuses_short_rows(ctx):
    from hipdrt import _ffi
    with pytest.raises(_ffi.HipDrtError, match="ldx"):
        ctx.debug_apply_rows(np.ones((2, 4)), np.ones((3, 4)), col_offset=1)


# ---- the fitted plan shared by 3, 4 ----------------------------------------------------------------------------------------------
FREQ71 = np.logspace(6, -1, 71)
F57 = np.logspace(7, -3, 57)


@pytest.fixture(scope="module")
def fit37():
    from hipdrt import synth
    from hipdrt.models import DRT
    z = synth.zarc2_batch(FREQ71, 37, first_seed=900)
    drt = DRT(warn=False)
    res = drt.fit_eis_batch(FREQ71, z)
    assert (res["status"] >= 0).all()
    return drt, z, res


def wide_tau(basis_tau):
    return np.logspace(np.log10(basis_tau.min()) - 1.5, np.log10(basis_tau.max()) + 1.5, 37)


# ---- 3. position independence ------------------------------------------------------------------------------------------------------
def test_alone_and_in_a_batch_give_the_same_bits(fit37):
    from hipdrt.models import DRT
    drt, z, res = fit37
    tau = wide_tau(drt.basis_tau)
    mu = [drt.predict_drt_batch(order=o) for o in (0, 1, 2)] + [drt.predict_drt_batch(tau=tau, normalize=True)]
    zz = [drt.predict_z_batch(), drt.predict_z_batch(F57)]
    rr = [drt.predict_r_p_batch(), drt.predict_r_tot_batch()]
    one = DRT(warn=False)
    for b in (0, 16, 36):
        r1 = one.fit_eis_batch(FREQ71, z[b:b + 1])
        assert np.array_equal(r1["x"][0], res["x"][b]), "the fit itself differs between batch sizes: nothing to compare"
        mu1 = [one.predict_drt_batch(order=o) for o in (0, 1, 2)] + [one.predict_drt_batch(tau=tau, normalize=True)]
        for a, c in zip(mu1, mu):
            assert np.array_equal(a[0], c[b]), b
        for a, c in zip([one.predict_z_batch(), one.predict_z_batch(F57)], zz):
            assert np.array_equal(a[0], c[b]), b
        for a, c in zip([one.predict_r_p_batch(), one.predict_r_tot_batch()], rr):
            assert a[0] == c[b], b


# ---- 4. the device against its own fit ----------------------------------------------------------------------------------------------
def within(label, out, ref, mag, K, factor=1.0):
    ratio = float((np.abs(out - ref) / (factor * ((K + 8) * U * mag + 1e-300))).max())
    print(f"{label}: error {ratio:.3g} of the bound")
    assert ratio <= 1.0, f"{label}: error {ratio:.3g} of the bound"


@pytest.mark.parametrize("order", [0, 1, 2])
def test_drt_against_numpy_on_downloaded_x(fit37, order):
    from hipdrt.models import predict
    drt, _, res = fit37
    bt, eps, x = drt.basis_tau, drt.tau_epsilon, res["fit_x"]
    K = len(bt)
    for name, tau in (("default", drt.get_tau_eval(20)), ("wide", wide_tau(bt))):
        mu = drt.predict_drt_batch(tau=tau, order=order)
        assert mu.shape == (37, len(tau))
        e = predict.eval_matrix(bt, tau, eps, order)
        ref = np.array([predict.drt(xb, bt, tau, eps, order=order) for xb in x])
        within(f"drt order {order} {name}", mu, ref, np.abs(x) @ np.abs(e).T, K)
    # the single-spectrum form is a row of the batch
    assert np.array_equal(drt.predict_drt(order=order, b=5), drt.predict_drt_batch(order=order)[5])


def test_normalised_drt_and_resistances_against_numpy(fit37):
    from hipdrt.models import predict
    drt, _, res = fit37
    bt, eps, x = drt.basis_tau, drt.tau_epsilon, res["fit_x"]
    K = len(bt)
    tau = drt.get_tau_eval(20)
    mag = np.abs(x) @ np.abs(predict.eval_matrix(bt, tau, eps)).T
    for abs_norm in (False, True):
        rp = predict.r_p(x, eps, absolute=abs_norm)
        ref = np.array([predict.drt(xb, bt, tau, eps, normalize=True, abs_norm=abs_norm) for xb in x])
        # the normaliser carries its own summation error, relative (K + 8) u: twice the bound in all
        within(f"drt normalised abs={abs_norm}", drt.predict_drt_batch(normalize=True, abs_norm=abs_norm), ref,
               mag / np.abs(rp)[:, None], K, factor=2.0)
        within(f"r_p abs={abs_norm}", drt.predict_r_p_batch(absolute=abs_norm), rp,
               np.sum(np.abs(x), axis=1) * predict.basis_area(eps), K)
    assert np.array_equal(drt.predict_r_inf_batch(), res["R_inf"])
    within("r_tot", drt.predict_r_tot_batch(), predict.r_tot(x, res["R_inf"], eps),
           np.sum(np.abs(x), axis=1) * predict.basis_area(eps) + np.abs(res["R_inf"]), K)
    np.testing.assert_allclose(drt.predict_drt_batch(normalize_by=2.5), drt.predict_drt_batch() / 2.5, rtol=4 * U)
    assert drt.predict_r_p(b=3) == drt.predict_r_p_batch()[3] and drt.predict_r_tot(b=3) == drt.predict_r_tot_batch()[3]


def test_impedance_against_numpy_on_downloaded_x(fit37, ctx):
    from hipdrt.models import predict
    drt, _, res = fit37
    bt, eps, x = drt.basis_tau, drt.tau_epsilon, res["fit_x"]
    K = len(bt)
    lut = drt.interpolate_lookups
    a_re, a_im = ctx.impedance_matrix(F57, bt, eps, lookups=(lut["z_real"], lut["z_imag"]))
    for kw in ({}, {"include_drt": False}, {"include_ohmic": False}, {"include_inductance": False}):
        z = drt.predict_z_batch(F57, **kw)
        assert z.shape == (37, 57) and np.iscomplexobj(z)
        ref = np.array([predict.impedance(a_re, a_im, x[b], res["R_inf"][b], res["inductance"][b], F57, **kw) for b in range(37)])
        # the two scalar terms and their additions join the sum of magnitudes
        within(f"z real {kw}", z.real, ref.real, np.abs(x) @ np.abs(a_re).T + np.abs(res["R_inf"])[:, None], K)
        within(f"z imag {kw}", z.imag, ref.imag,
               np.abs(x) @ np.abs(a_im).T + np.abs(res["inductance"])[:, None] * 2 * np.pi * F57[None, :], K)
    # at the fit frequencies the KK screen forms the same terms in another order (and from the plan's Toeplitz-built matrix)
    a_re, a_im = drt._plan.get("a_re"), drt._plan.get("a_im")
    z_hat = drt._plan.kk_screen(residuals=False)["z_hat"]
    z = drt.predict_z_batch()
    within("z real vs kk_screen", z.real, z_hat.real, np.abs(x) @ np.abs(a_re).T + np.abs(res["R_inf"])[:, None], K, factor=2.0)
    within("z imag vs kk_screen", z.imag, z_hat.imag,
           np.abs(x) @ np.abs(a_im).T + np.abs(res["inductance"])[:, None] * 2 * np.pi * FREQ71[None, :], K, factor=2.0)


def test_band_against_the_existing_variance_method(fit37):
    from hipdrt.models import predict
    drt, _, _ = fit37
    for tau in (None, wide_tau(drt.basis_tau)):
        for q in ((0.025, 0.975), (0.1, 0.9)):
            lo, hi, ok = drt.predict_drt_ci_batch(tau=tau, quantiles=q)
            var, vok = drt.estimate_distribution_var_batch(tau=tau)
            mu = drt.predict_drt_batch(tau=tau)
            assert ok.all() and vok.all()
            rlo, rhi = predict.band(mu, np.sqrt(var), q)
            np.testing.assert_allclose(lo, rlo, rtol=RTOL)
            np.testing.assert_allclose(hi, rhi, rtol=RTOL)
    lo1, hi1 = drt.predict_drt_ci(b=7)
    lo, hi, _ = drt.predict_drt_ci_batch()
    assert np.array_equal(lo1, lo[7]) and np.array_equal(hi1, hi[7])


# ---- 5. the device against the reference's runs -----------------------------------------------------------------------------------
def sigma_of(lo, hi, q):
    from hipdrt.models import predict
    s_lo, s_hi = predict.n_sigma(q)
    return (hi - lo) / (s_hi - s_lo)


def check_resistances_of_a_prepared_fit(drt, sign):
    """R_p / R_inf / R_tot of a single fit on a prepared plan against models.predict on its fit_parameters (bound of test 2)"""
    from hipdrt.models import predict
    fp, eps, nb = drt.fit_parameters, drt.tau_epsilon, len(drt.basis_tau)
    xs = predict.drt_params(fp["x"], nb, sign)
    mag = np.array([np.sum(np.abs(fp["x"])) * predict.basis_area(eps)])
    within("prepared r_p", np.array([drt.predict_r_p()]), np.array([predict.r_p(xs, eps)]), mag, nb)
    within("prepared r_p abs", np.array([drt.predict_r_p(absolute=True)]), np.array([predict.r_p(xs, eps, absolute=True)]), mag, nb)
    assert drt.predict_r_inf() == fp["R_inf"]
    within("prepared r_tot", np.array([drt.predict_r_tot()]), np.array([predict.r_tot(xs, fp["R_inf"], eps)]),
           mag + abs(fp["R_inf"]), nb)


def test_plain_fit_against_the_reference_run():
    from hipdrt.models import DRT
    g = np.load(os.path.join(GOLDEN, "refrun_predict_golden71x91.npz"))
    drt = DRT()
    drt.fit_eis(g["freq"], g["z"])
    for order in (0, 1, 2):
        parity(f"drt_o{order}", drt.predict_drt(order=order), g[f"drt_o{order}"], default=1e-7)
        parity(f"drt_wide_o{order}", drt.predict_drt(tau=g["tau_wide"], order=order), g[f"drt_wide_o{order}"], default=1e-7)
    parity("drt_norm", drt.predict_drt(normalize=True), g["drt_norm"], default=1e-7)
    parity("drt_absnorm", drt.predict_drt(normalize=True, abs_norm=True), g["drt_absnorm"], default=1e-7)
    for i in (0, 1):
        q = tuple(g[f"ci{i}_q"])
        lo, hi = drt.predict_drt_ci(quantiles=q)
        parity(f"ci{i}_lo", lo, g[f"ci{i}_lo"], default=1e-6)
        parity(f"ci{i}_hi", hi, g[f"ci{i}_hi"], default=1e-6)
        parity(f"ci{i}_sigma", sigma_of(lo, hi, q), g["sigma"], default=1e-6, rel=True, floor=1e-6)
    lo, hi = drt.predict_drt_ci(tau=g["tau_wide"])
    parity("ci_wide_lo", lo, g["ci_wide_lo"], default=1e-6)
    parity("ci_wide_hi", hi, g["ci_wide_hi"], default=1e-6)
    parity("z_fit", drt.predict_z_batch()[0], g["z_fit"], default=1e-7)
    parity("z_fit_given", drt.predict_z_batch(g["freq"])[0], g["z_fit"], default=1e-7)
    parity("z57", drt.predict_z_batch(g["freq57"])[0], g["z57"], default=1e-7)
    for off in ("drt", "ohmic", "inductance"):
        parity(f"z57_no_{off}", drt.predict_z_batch(g["freq57"], **{f"include_{off}": False})[0], g[f"z57_no_{off}"],
               default=1e-7)
    parity("r_p", [drt.predict_r_p()], [g["r_p"]], default=1e-7)
    parity("r_p_abs", [drt.predict_r_p(absolute=True)], [g["r_p_abs"]], default=1e-7)
    parity("r_inf", [drt.predict_r_inf()], [g["r_inf"]], default=1e-7)
    parity("r_tot", [drt.predict_r_tot()], [g["r_tot"]], default=1e-7)
    with pytest.warns(DeprecationWarning):
        assert np.array_equal(drt.predict_distribution(order=1), drt.predict_drt(order=1))


def test_series_neg_fit_against_the_reference_run():
    from hipdrt.models import DRT
    g = np.load(os.path.join(GOLDEN, "refrun_predict_sneg71x91.npz"))
    drt = DRT()
    drt.fit_eis(g["freq"], g["z"], series_neg=True)
    for sign, tag in ((1, "pos"), (-1, "neg"), (0, "both")):
        parity(f"drt_{tag}", drt.predict_drt(sign=sign), g[f"drt_{tag}"], default=1e-7)
        lo, hi = drt.predict_drt_ci(sign=sign)
        parity(f"ci_{tag}_lo", lo, g[f"ci_{tag}_lo"], default=1e-6)
        parity(f"ci_{tag}_hi", hi, g[f"ci_{tag}_hi"], default=1e-6)
        parity(f"sigma_{tag}", sigma_of(lo, hi, (0.025, 0.975)), g[f"sigma_{tag}"], default=1e-6, rel=True, floor=1e-6)
    check_resistances_of_a_prepared_fit(drt, 0)
    # sign=None is the reference's default for such a fit: the net distribution
    assert np.array_equal(drt.predict_drt_batch()[0], drt.predict_drt(sign=0))
    with pytest.raises(ValueError, match="sign"):
        drt.predict_drt(sign=2)
    # 7: a prepared plan holds no lookup tables: no impedance prediction
    with pytest.raises(NotImplementedError, match="plain EIS"):
        drt.predict_z_batch()


def test_hybrid_fit_against_the_reference_run():
    from hipdrt import synth
    from hipdrt.models import DRT
    g = np.load(os.path.join(GOLDEN, "refrun_predict_hybrid_s0.npz"))
    drt = DRT()
    drt.fit_hybrid(*synth.hybrid_measurement(seed=0))
    parity("drt_o0", drt.predict_drt(order=0), g["drt_o0"], default=1e-7)
    parity("drt_o2", drt.predict_drt(order=2), g["drt_o2"], default=1e-7)
    lo, hi = drt.predict_drt_ci()
    parity("ci_lo", lo, g["ci_lo"], default=1e-6)
    parity("ci_hi", hi, g["ci_hi"], default=1e-6)
    parity("sigma", sigma_of(lo, hi, (0.025, 0.975)), g["sigma"], default=1e-6, rel=True, floor=1e-6)
    check_resistances_of_a_prepared_fit(drt, 1)
    with pytest.raises(NotImplementedError, match="plain EIS"):
        drt.predict_z_batch()


# ---- 6. failure rows ------------------------------------------------------------------------------------------------------------------
def test_failed_fit_gives_a_nan_row_and_a_negative_status():
    """all-NaN data break the QP at its start point (the input of the mapping tests' ignore_errors=True case)"""
    from hipdrt import synth
    from hipdrt.models import DRT
    z = synth.zarc2_batch(FREQ71, 5, first_seed=300)
    zbad = z.copy()
    zbad[2] = np.nan
    good, bad = DRT(warn=False), DRT(warn=False)
    good.fit_eis_batch(FREQ71, z)
    res = bad.fit_eis_batch(FREQ71, zbad)
    assert res["status"][2] < 0 and (np.delete(res["status"], 2) >= 0).all()
    keep = [0, 1, 3, 4]
    mu, mu_good = bad.predict_drt_batch(order=1), good.predict_drt_batch(order=1)
    lo, hi, ok = bad.predict_drt_ci_batch()
    lo_good, hi_good, _ = good.predict_drt_ci_batch()
    zz, zz_good = bad.predict_z_batch(F57), good.predict_z_batch(F57)
    assert np.isnan(mu[2]).all() and np.isnan(lo[2]).all() and np.isnan(hi[2]).all() and np.isnan(zz[2]).all()
    assert ok.tolist() == [True, True, False, True, True]
    _, _, _, status = bad._plan.predict_drt(np.log(bad.get_tau_eval(20)))
    assert status[2] < 0 and (status[keep] >= 0).all()
    assert bad._plan.predict_z(F57)[1][2] < 0
    for a, c in ((mu, mu_good), (lo, lo_good), (hi, hi_good), (zz, zz_good)):
        assert np.array_equal(a[keep], c[keep])


# ---- 7. refusals ----------------------------------------------------------------------------------------------------------------------
def test_refusals(fit37):
    from hipdrt import _ffi
    from hipdrt.models import DRT
    drt, z, _ = fit37
    with pytest.raises(NotImplementedError):
        drt.predict_z(FREQ71[:-1])                                    # DRT.predict_z keeps to the fit frequencies
    with pytest.raises(NotImplementedError, match="x="):
        drt.predict_drt_batch(x=np.ones(3))
    dop = DRT(fit_dop=True, warn=False)
    dop.fit_eis(FREQ71, z[0])
    with pytest.raises(NotImplementedError, match="fit_dop"):
        dop.predict_z_batch()
    # the C entry point itself refuses a prepared plan with the library's "not supported" status
    with pytest.raises(_ffi.HipDrtError, match="not supported"):
        dop._plan.predict_z(FREQ71)
    assert dop.predict_drt_batch().shape == (1, len(dop.get_tau_eval(20)))
