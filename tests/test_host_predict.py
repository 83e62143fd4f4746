"""CPU: hipdrt.models.predict (the numpy statement of the device predictions) against runs of the reference recorded by
tools/make_predict_golden.py, fed the fixture's own coefficients, and the argument checks of the DRT prediction methods.

Tolerance: rtol 1e-12 (the same formulas on the same inputs; what differs is the summation order of the matrix product), plus
1e-12 max|.| absolute for the derivative orders 1 and 2 and for the imaginary part of Z, whose terms cancel near their zeros."""
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN

RTOL = 1e-12


def close(actual, desired, absolute=False):
    atol = RTOL * float(np.abs(desired).max()) if absolute else 0.0
    np.testing.assert_allclose(actual, desired, rtol=RTOL, atol=atol)


@pytest.fixture(scope="module")
def plain():
    return np.load(os.path.join(GOLDEN, "refrun_predict_golden71x91.npz"))


@pytest.fixture(scope="module")
def sneg():
    return np.load(os.path.join(GOLDEN, "refrun_predict_sneg71x91.npz"))


@pytest.fixture(scope="module")
def hybrid():
    return np.load(os.path.join(GOLDEN, "refrun_predict_hybrid_s0.npz"))


def test_fixtures_are_what_the_tool_says(plain, sneg, hybrid):
    assert len(plain["freq"]) == 71 and len(plain["basis_tau"]) == 91 and len(plain["x"]) == 91
    assert len(plain["tau_wide"]) == 37 and len(plain["freq57"]) == 57
    assert plain["tau_wide"][0] < plain["basis_tau"].min() / 30 and plain["tau_wide"][-1] > plain["basis_tau"].max() * 30
    assert len(sneg["x"]) == 2 * len(sneg["basis_tau"])
    assert len(hybrid["x"]) == len(hybrid["basis_tau"])


@pytest.mark.parametrize("order", [0, 1, 2])
def test_drt_orders_on_both_grids(plain, order):
    from hipdrt.models import predict
    x, bt, eps = plain["x"], plain["basis_tau"], float(plain["tau_epsilon"])
    close(predict.drt(x, bt, plain["tau_default"], eps, order=order), plain[f"drt_o{order}"], absolute=order > 0)
    close(predict.drt(x, bt, plain["tau_wide"], eps, order=order), plain[f"drt_wide_o{order}"], absolute=order > 0)


def test_eval_matrix_is_the_boundary_mirror(plain):
    """matrices.basis.construct_func_eval_matrix: order 0 bit for bit what it was, orders 1 and 2 the same formula as predict's"""
    from hipdrt.matrices import basis
    from hipdrt.models import predict
    bt, tau, eps = plain["basis_tau"], plain["tau_wide"], float(plain["tau_epsilon"])
    xx_b, xx_e = np.meshgrid(np.log(bt), np.log(tau))
    assert np.array_equal(basis.construct_func_eval_matrix(np.log(bt), np.log(tau), epsilon=eps, order=0),
                          np.exp(-(eps * (xx_e - xx_b)) ** 2))
    for order in (0, 1, 2):
        assert np.array_equal(basis.construct_func_eval_matrix(np.log(bt), np.log(tau), epsilon=eps, order=order),
                              predict.eval_matrix(bt, tau, eps, order))
    with pytest.raises(NotImplementedError):
        basis.construct_func_eval_matrix(np.log(bt), np.log(tau), epsilon=eps, order=3)


def test_normalised_drt_and_resistances(plain):
    from hipdrt.models import predict
    x, bt, eps = plain["x"], plain["basis_tau"], float(plain["tau_epsilon"])
    close(predict.drt(x, bt, plain["tau_default"], eps, normalize=True), plain["drt_norm"])
    close(predict.drt(x, bt, plain["tau_default"], eps, normalize=True, abs_norm=True), plain["drt_absnorm"])
    close(predict.drt(x, bt, plain["tau_default"], eps, normalize_by=2.5), plain["drt_o0"] / 2.5)
    close(predict.r_p(x, eps), plain["r_p"])
    close(predict.r_p(x, eps, absolute=True), plain["r_p_abs"])
    close(predict.r_tot(x, float(plain["R_inf"]), eps), plain["r_tot"])
    assert float(plain["r_inf"]) == float(plain["R_inf"])


def test_band_from_mean_and_sigma(plain, hybrid):
    from hipdrt.models import predict
    for i in (0, 1):
        lo, hi = predict.band(plain["drt_o0"], plain["sigma"], tuple(plain[f"ci{i}_q"]))
        close(lo, plain[f"ci{i}_lo"])
        close(hi, plain[f"ci{i}_hi"])
    lo, hi = predict.band(plain["drt_wide_o0"], plain["sigma_wide"])
    close(lo, plain["ci_wide_lo"])
    close(hi, plain["ci_wide_hi"])
    lo, hi = predict.band(hybrid["drt_o0"], hybrid["sigma"])
    close(lo, hybrid["ci_lo"])
    close(hi, hybrid["ci_hi"])


@pytest.mark.parametrize("sign,tag", [(1, "pos"), (-1, "neg"), (0, "both")])
def test_series_neg_sign_rule(sneg, sign, tag):
    from hipdrt.models import predict
    bt, eps = sneg["basis_tau"], float(sneg["tau_epsilon"])
    mu = predict.drt(sneg["x"], bt, sneg["tau_default"], eps, sign=sign)
    close(mu, sneg[f"drt_{tag}"])
    lo, hi = predict.band(mu, sneg[f"sigma_{tag}"])
    close(lo, sneg[f"ci_{tag}_lo"])
    close(hi, sneg[f"ci_{tag}_hi"])
    assert predict.default_sign(True) == 0 and predict.default_sign(False) == 1


@pytest.mark.parametrize("order", [0, 2])
def test_hybrid_fit(hybrid, order):
    from hipdrt.models import predict
    close(predict.drt(hybrid["x"], hybrid["basis_tau"], hybrid["tau_default"], float(hybrid["tau_epsilon"]), order=order),
          hybrid[f"drt_o{order}"], absolute=order > 0)


def test_impedance_assembly(plain):
    from hipdrt.models import predict
    x, r_inf, induc = plain["x"], float(plain["R_inf"]), float(plain["inductance"])

    def check(z, ref):
        close(z.real, ref.real)
        close(z.imag, ref.imag, absolute=True)

    zm = plain["zm_fit"]
    check(predict.impedance(zm.real, zm.imag, x, r_inf, induc, plain["freq"]), plain["z_fit"])
    zm, f = plain["zm57"], plain["freq57"]
    assert f.max() * plain["basis_tau"].max() * 2 * np.pi > 10 ** 5.4 and f.min() * plain["basis_tau"].min() * 2 * np.pi < 10 ** -5.4
    check(predict.impedance(zm.real, zm.imag, x, r_inf, induc, f), plain["z57"])
    for off in ("drt", "ohmic", "inductance"):
        check(predict.impedance(zm.real, zm.imag, x, r_inf, induc, f, **{f"include_{off}": False}), plain[f"z57_no_{off}"])


def test_argument_errors(sneg, plain):
    from hipdrt.models import DRT, predict
    bt, eps = sneg["basis_tau"], float(sneg["tau_epsilon"])
    with pytest.raises(ValueError, match="sign"):
        predict.drt(sneg["x"], bt, sneg["tau_default"], eps, sign=2)
    with pytest.raises(ValueError, match="order"):
        predict.drt(plain["x"], plain["basis_tau"], plain["tau_default"], eps, order=3)
    with pytest.raises(ValueError):
        predict.drt_params(np.ones(7), 5)
    drt = DRT()
    with pytest.raises(ValueError, match="order"):
        drt.predict_drt_batch(order=3)
    for call in (drt.predict_drt_batch, drt.predict_drt_ci_batch, drt.predict_z_batch, drt.predict_drt, drt.predict_drt_ci,
                 drt.predict_r_p):
        with pytest.raises(NotImplementedError, match="x="):
            call(x=np.ones(3))
    with pytest.raises(NotImplementedError, match="p_matrix="):
        drt.predict_drt_ci(p_matrix=np.eye(3))
    for call in (drt.predict_drt_batch, drt.predict_drt_ci_batch, drt.predict_z_batch, drt.predict_r_p_batch,
                 drt.predict_r_inf_batch, drt.predict_r_tot_batch, drt.predict_drt, drt.predict_drt_ci, drt.predict_r_p,
                 drt.predict_r_inf, drt.predict_r_tot):
        with pytest.raises(RuntimeError, match="finished qphb fit"):
            call()
    with pytest.raises(NotImplementedError, match="fit_dop"):
        DRT(fit_dop=True, fixed_basis_nu=np.linspace(-1, 1, 5)).predict_z_batch()


def test_predict_distribution_warns():
    from hipdrt.models import DRT
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter("always")
        with pytest.raises(RuntimeError):
            DRT().predict_distribution()
    assert any(issubclass(i.category, DeprecationWarning) and "predict_drt" in str(i.message) for i in w)
