"""GPU: the optional outputs of the post-fit entry points (hipdrt_plan_find_peaks, hipdrt_plan_resolve_peaks, hipdrt_plan_kk_screen,
hipdrt_plan_predict_pfrt).  Every output pointer of these calls may be NULL; what is left out is neither formed nor downloaded.

Each entry point is called once with every output and then once per output with that output alone: the output that remains, and
the status, must be the bytes of the full call (NaN padding included).  The library is compared with itself across two calls on
the same fitted plan, so no tolerance is involved."""
import os

import numpy as np
import pytest

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

FREQ71 = np.logspace(6, -1, 71)


def same_bytes(tag, got, full):
    assert got.dtype == full.dtype and got.shape == full.shape, tag
    assert np.array_equal(got.view(np.uint8), full.view(np.uint8)), tag


@pytest.fixture(scope="module")
def fit3():
    """one plain fit of 3 synthetic spectra, 71 frequencies on the default 91-point basis"""
    from hipdrt import synth
    from hipdrt.models import DRT
    drt = DRT(warn=False)
    res = drt.fit_eis_batch(FREQ71, synth.zarc2_batch(FREQ71, 3, first_seed=900))
    assert (res["status"] >= 0).all()
    return drt


@pytest.fixture(scope="module")
def pfrt3():
    """the 3-member, 11-step PFRT fit of test_gpu_pfrt.py"""
    from hipdrt import synth
    from hipdrt.models import DRT
    g = np.load(os.path.join(GOLDEN, "ref_test_drt_fit_eis.npz"))
    freq, z = np.asarray(g["freq"], dtype=float), np.asarray(g["z"], dtype=complex)
    drt = DRT(warn=False)
    pr = drt.pfrt_fit_eis_batch(freq, np.vstack([z[None, :], synth.zarc2_batch(freq, 2, first_seed=40)]))
    assert (pr["status"] >= 0).all() and drt._plan.pfrt_steps() == 11
    return drt, pr


def one_by_one(tag, call, always=("status",)):
    """call(want) -> dict of arrays: the full call, then every output alone"""
    full = call(None)
    names = [k for k in full if k not in always]
    assert names, tag
    for name in names:
        part = call((name,))
        assert set(part) == {name, *always}, (tag, name, sorted(part))
        for k in part:
            same_bytes(f"{tag}: {k} with want=({name!r},)", part[k], full[k])
    return full


@pytest.mark.parametrize("method", [0, 2])
def test_find_peaks_one_output_at_a_time(fit3, method):
    from hipdrt import _ffi
    ln_tau = np.log(fit3.get_tau_eval(10))
    li, ri = fit3._extend_var_indices(fit3.get_tau_eval(10))
    opts = _ffi.peak_opts(method=method, ext_left=li if method else -1, ext_right=ri if method else -1)
    full = one_by_one(f"find_peaks method {method}", lambda want: fit3._plan.find_peaks(ln_tau, opts, want=want))
    assert len(full) == (12 if method == 2 else 10)
    assert (full["count"] >= 1).all() and (full["status"] >= 0).all()


@pytest.mark.parametrize("grid", [True, False], ids=["grid", "nogrid"])
def test_resolve_peaks_one_output_at_a_time(fit3, grid):
    ln_find = np.log(fit3.get_tau_eval(10))
    ln_out = np.log(fit3.get_tau_eval(20)) if grid else None
    full = one_by_one(f"resolve_peaks grid {grid}", lambda want: fit3._plan.resolve_peaks(ln_find, ln_out, want=want),
                      always=("count", "status"))
    assert len(full) == (10 if grid else 8)
    assert (full["count"] >= 1).all() and (full["status"] >= 0).all()


def test_kk_screen_with_and_without_the_prediction_and_the_residuals(fit3):
    plan = fit3._plan
    full = plan.kk_screen()
    assert set(full) == {"std", "outlier_mask", "f_lim", "i_lim", "status", "z_hat", "residuals"}
    for z_hat, residuals in ((False, True), (True, False), (False, False)):
        part = plan.kk_screen(z_hat=z_hat, residuals=residuals)
        assert ("z_hat" in part) == z_hat and ("residuals" in part) == residuals
        for k in part:
            same_bytes(f"kk_screen: {k} with z_hat={z_hat}, residuals={residuals}", part[k], full[k])


def test_predict_pfrt_one_output_at_a_time(pfrt3):
    from hipdrt import _ffi
    drt, pr = pfrt3
    tau = drt.get_tau_eval(10)
    li, ri = drt._extend_var_indices(tau)
    opts = _ffi.pfrt_opts(ext_left=li, ext_right=ri)
    factors = np.asarray(pr["factors"], dtype=float)
    full = one_by_one("predict_pfrt", lambda want: drt._plan.predict_pfrt(factors, np.log(tau), np.log(tau), opts, want=want))
    assert set(full) == {"pfrt", "raw_pfrt", "step_pfrt", "post_prob", "status"}
    assert (full["status"] >= 0).all() and np.isfinite(full["pfrt"]).all()
