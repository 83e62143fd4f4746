"""Generate the model-evaluation fixtures under tests/golden/ (build container only: imports the reference through the shims of
oracle/refshim, like tools/make_kk_golden.py):

  refrun_predict_golden71x91.npz   the reference's 71-frequency known-answer spectrum (tests/golden/ref_test_drt_fit_eis.npz) fitted
                                   with fit_eis: predict_drt (orders 0-2, default and wide grid, normalised), predict_drt_ci,
                                   predict_z on the fit grid and on a grid that leaves the lookup tables, the three resistances
  refrun_predict_sneg71x91.npz     the same spectrum with series_neg=True: predict_drt / predict_drt_ci for sign 1, -1, 0
  refrun_predict_hybrid_s0.npz     fit_hybrid on synth.hybrid_measurement(seed=0): predict_drt orders 0 and 2, predict_drt_ci

(hybdrt/models/drt1d.py:2965-3061 predict_drt, 3063-3151 estimate_distribution_cov, 3209-3231 predict_drt_ci, 3500-3542
predict_z, 3552-3584 the resistances)

    python tools/make_predict_golden.py
"""
import contextlib
import io
import os
import sys
import warnings

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle", "refshim"))
import oracle_boot  # noqa: E402,F401

from hybdrt.models import DRT  # noqa: E402

from hipdrt import synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CTOR = dict(fit_inductance=True, fit_capacitance=False, fit_dop=False, fit_ohmic=True)
QUANTILES = ((0.025, 0.975), (0.1, 0.9))


@contextlib.contextmanager
def quiet():
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter("ignore")
        yield


def common(drt):
    fp = drt.fit_parameters
    return dict(x=fp["x"], R_inf=np.float64(fp.get("R_inf", 0)), inductance=np.float64(fp.get("inductance", 0)),
                coefficient_scale=np.float64(drt.coefficient_scale), basis_tau=drt.basis_tau,
                tau_epsilon=np.float64(drt.tau_epsilon), tau_default=drt.get_tau_eval(20))


def wide_grid(basis_tau):
    """37 points reaching 1.5 decades beyond the basis on both sides"""
    return np.logspace(np.log10(basis_tau.min()) - 1.5, np.log10(basis_tau.max()) + 1.5, 37)


def sigma_of(drt, **kw):
    return np.diag(drt.estimate_distribution_cov(**kw)) ** 0.5


def make_plain(freq, z):
    with quiet():
        drt = DRT(**CTOR)
        drt.fit_eis(freq, z)
        out = dict(common(drt), freq=freq, z=z)
        tau_wide = wide_grid(drt.basis_tau)
        out["tau_wide"] = tau_wide
        for order in (0, 1, 2):
            out[f"drt_o{order}"] = drt.predict_drt(order=order)
            out[f"drt_wide_o{order}"] = drt.predict_drt(tau=tau_wide, order=order)
        out["drt_norm"] = drt.predict_drt(normalize=True)
        out["drt_absnorm"] = drt.predict_drt(normalize=True, abs_norm=True)
        for i, q in enumerate(QUANTILES):
            lo, hi = drt.predict_drt_ci(quantiles=list(q))
            out[f"ci{i}_q"], out[f"ci{i}_lo"], out[f"ci{i}_hi"] = np.array(q), lo, hi
        out["sigma"] = sigma_of(drt)
        lo, hi = drt.predict_drt_ci(tau=tau_wide)
        out["ci_wide_lo"], out["ci_wide_hi"], out["sigma_wide"] = lo, hi, sigma_of(drt, tau=tau_wide)
        out["z_fit"] = drt.predict_z(freq, include_vz_offset=False)
        zm, _ = drt._prep_impedance_prediction_matrix(freq)
        out["zm_fit"] = np.asarray(zm)
        f57 = np.logspace(7, -3, 57)
        out["freq57"] = f57
        zm, _ = drt._prep_impedance_prediction_matrix(f57)
        out["zm57"] = np.asarray(zm)
        out["z57"] = drt.predict_z(f57, include_vz_offset=False)
        out["z57_no_drt"] = drt.predict_z(f57, include_vz_offset=False, include_drt=False)
        out["z57_no_ohmic"] = drt.predict_z(f57, include_vz_offset=False, include_ohmic=False)
        out["z57_no_inductance"] = drt.predict_z(f57, include_vz_offset=False, include_inductance=False)
        out["r_p"], out["r_p_abs"] = np.float64(drt.predict_r_p()), np.float64(drt.predict_r_p(absolute=True))
        out["r_inf"], out["r_tot"] = np.float64(drt.predict_r_inf()), np.float64(drt.predict_r_tot())
    np.savez_compressed(os.path.join(GOLDEN, "refrun_predict_golden71x91.npz"), **out)
    print("refrun_predict_golden71x91.npz: n_tau", len(out["x"]), "R_p", float(out["r_p"]), "peak", float(out["drt_o0"].max()))


def make_sneg(freq, z):
    with quiet():
        drt = DRT(**CTOR)
        drt.fit_eis(freq, z, series_neg=True)
        out = dict(common(drt), freq=freq, z=z)
        for sign, tag in ((1, "pos"), (-1, "neg"), (0, "both")):
            out[f"drt_{tag}"] = drt.predict_drt(sign=sign)
            out[f"ci_{tag}_lo"], out[f"ci_{tag}_hi"] = drt.predict_drt_ci(sign=sign)
            out[f"sigma_{tag}"] = sigma_of(drt, sign=sign)
    assert len(out["x"]) == 2 * len(out["basis_tau"])
    np.savez_compressed(os.path.join(GOLDEN, "refrun_predict_sneg71x91.npz"), **out)
    print("refrun_predict_sneg71x91.npz: peaks", {t: float(np.abs(out[f"drt_{t}"]).max()) for t in ("pos", "neg", "both")})


def make_hybrid():
    meas = synth.hybrid_measurement(seed=0)
    with quiet():
        drt = DRT(**CTOR)
        drt.fit_hybrid(*meas)
        out = dict(common(drt))
        out["drt_o0"], out["drt_o2"] = drt.predict_drt(order=0), drt.predict_drt(order=2)
        out["ci_lo"], out["ci_hi"] = drt.predict_drt_ci()
        out["sigma"] = sigma_of(drt)
    np.savez_compressed(os.path.join(GOLDEN, "refrun_predict_hybrid_s0.npz"), **out)
    print("refrun_predict_hybrid_s0.npz: n_tau", len(out["x"]), "peak", float(out["drt_o0"].max()))


if __name__ == "__main__":
    g = np.load(os.path.join(GOLDEN, "ref_test_drt_fit_eis.npz"))
    make_plain(g["freq"], g["z"])
    make_sneg(g["freq"], g["z"])
    make_hybrid()
