"""Generate the response-prediction fixtures under tests/golden/ (build container only: imports the reference through the shims of
oracle/refshim, like tools/make_predict_golden.py).  One file per case, runs of the reference on inputs the project already uses:

  refrun_response_predict_hybrid_s0.npz       fit_hybrid on synth.hybrid_measurement(seed=0)
  refrun_response_predict_hybrid_s0_dop.npz   the same measurement with fit_dop=True
  refrun_response_predict_hybrid_s0_dop_solverp.npz   ... with fit_dop=True and solve_rp=True (post-fit scales, rescaled DOP columns)
  refrun_response_predict_hybrid_3step.npz    the three-step measurement of refrun_hybrid_3step (vz_offset_scale=0.5, vz_offset_eps=2)
  refrun_response_predict_chrono_s1.npz       fit_chrono on the chrono half of the seed-0 measurement
  refrun_response_predict_golden71_dop.npz    fit_eis of the 71-point known-answer spectrum with fit_dop=True (no response)
  refrun_response_predict_golden71_cap.npz    the same spectrum with fit_capacitance=True (no response)

Each holds predict_response() at the fit times and at off-grid times that start before the first step and end past the last
sample (all terms, and with single terms switched off), predict_v_baseline at both, predict_z at the fit frequencies and on a wider
grid with and without include_vz_offset, predict_dop(return_nu=True) plain and normalised for the fit_dop case, the reference's
fit_parameters, and what the numpy statement (hipdrt/models/response.py) needs beside them: the unit-step layers of
mat1d.construct_response_matrix and phasance.construct_phasor_v_matrix, the response vectors, the vz-offset strengths, the
impedance and phasor-Z prediction matrices and the DOP evaluation matrix with its norm (hybdrt/models/drt1d.py:3273-3542,
6020-6226).

    python tools/make_response_golden.py
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

from hybdrt.matrices import basis, mat1d, phasance  # noqa: E402
from hybdrt.models import DRT, background  # noqa: E402

from hipdrt import synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
BASE = dict(fit_inductance=True, fit_capacitance=False, fit_ohmic=True)
TERMS = ("drt", "ohmic", "cap", "dop", "vz_offset")


@contextlib.contextmanager
def quiet():
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter("ignore")
        yield


def off_grid(times, step_times):
    """41 times: three before the first step, the rest log-spaced after it to 1.7 x the measured span"""
    t0, span = step_times[0], times[-1] - step_times[0]
    return np.concatenate([np.linspace(times[0] - 0.01, t0 - 1e-4, 3), t0 + np.logspace(-4.3, np.log10(1.7 * span), 38)])


def layers(drt, times):
    """what predict_response multiplies the parameters with, per unit step"""
    ones = np.ones(len(drt.step_times))
    _, u = mat1d.construct_response_matrix(drt.basis_tau, times, drt.step_model, drt.step_times, ones,
                                           basis_type=drt.tau_basis_type, epsilon=drt.tau_epsilon, tau_rise=None, op_mode="galv",
                                           integrate_method=drt.integrate_method, zga_params=drt.zga_params,
                                           interpolate_grids=drt.interpolate_lookups["response"])
    out = dict(u=np.asarray(u),
               inf_rv=mat1d.construct_ohmic_response_vector(times, drt.step_model, drt.step_times, drt.step_sizes, None, None,
                                                            True, "galv"),
               cap_rv=mat1d.construct_capacitance_response_vector(times, drt.step_model, drt.step_times, drt.step_sizes, None, "galv"),
               strength=drt._get_vz_strength_vec(times, vz_offset_eps=drt.fit_parameters.get("vz_offset_eps", None))[0],
               vb_mat=background.get_baseline_matrix(times, drt.v_baseline_deg, normalize=False, sqrt=drt.v_baseline_sqrt))
    if drt.fit_dop:
        _, ud = phasance.construct_phasor_v_matrix(times, drt.basis_nu, drt.nu_basis_type, drt.nu_epsilon, drt.step_model,
                                                   drt.step_times, ones, "galv")
        out["u_dop"] = np.asarray(ud)
    return out


def make(name, meas, ctor_kw, fit_kw):
    times, i_signal, v_signal, freq, z = meas
    with quiet():
        drt = DRT(**ctor_kw)
        if times is None:
            drt.fit_eis(freq, z, **fit_kw)
        elif freq is None:
            drt.fit_chrono(times, i_signal, v_signal, **fit_kw)
        else:
            drt.fit_hybrid(times, i_signal, v_signal, freq, z, **fit_kw)
        fp = drt.fit_parameters
        out = {f"fp_{k}": np.asarray(fp[k], dtype=float) for k in ("x", "R_inf", "inductance", "C_inv", "v_baseline", "vz_offset", "x_dop")
               if fp.get(k) is not None}
        out.update(basis_tau=drt.basis_tau, tau_epsilon=np.float64(drt.tau_epsilon), coefficient_scale=np.float64(drt.coefficient_scale),
                   vz_offset_eps=np.float64(fp.get("vz_offset_eps") or np.nan))
        if times is not None:
            t_fit = drt.get_fit_times()
            t_off = off_grid(t_fit, drt.step_times)
            out.update(step_times=drt.step_times, step_sizes=drt.step_sizes, t_fit=t_fit, t_off=t_off,
                       response_signal_scale=np.float64(drt.response_signal_scale), v_signal=np.asarray(v_signal, dtype=float),
                       nonconsec_step_times=drt.nonconsec_step_times)
            for tag, t in (("fit", None), ("off", t_off)):
                out[f"response_{tag}"] = drt.predict_response(times=t)
                for term in TERMS:
                    out[f"response_{tag}_no_{term}"] = drt.predict_response(times=t, **{f"include_{term}": False})
                tt = t_fit if t is None else t
                out[f"v_baseline_{tag}"] = drt.predict_v_baseline(tt)
                for k, v in layers(drt, tt).items():
                    out[f"{k}_{tag}"] = v
        if freq is not None:
            f_wide = np.logspace(np.log10(freq.max()) + 1.5, np.log10(freq.min()) - 1.5, 47)
            out.update(freq=freq, f_wide=f_wide)
            for tag, f in (("fit", freq), ("wide", f_wide)):
                out[f"z_{tag}"] = drt.predict_z(f)
                out[f"z_{tag}_no_vz"] = drt.predict_z(f, include_vz_offset=False)
                out[f"eis_strength_{tag}"] = drt._get_vz_strength_vec(None, f, vz_offset_eps=fp.get("vz_offset_eps", None))[1]
                for term in ("drt", "ohmic", "inductance", "cap", "dop"):
                    out[f"z_{tag}_no_{term}"] = drt.predict_z(f, **{f"include_{term}": False})
                drt._recalc_eis_prediction_matrix = True
                zm, zm_dop = drt._prep_impedance_prediction_matrix(f)
                if drt.series_neg:
                    zm = zm[:, :len(drt.basis_tau)]
                out[f"zm_{tag}"] = np.asarray(zm)
                if zm_dop is not None:
                    out[f"zm_dop_{tag}"] = np.asarray(zm_dop)
        if drt.fit_dop:
            out["dop_nu"], out["dop"] = drt.predict_dop(return_nu=True)
            out["dop_norm"] = drt.predict_dop(normalize=True)
            out["dop_no_ideal"] = drt.predict_dop(include_ideal=False)
            nu7 = np.array([0.9, -1.0, 0.0, -0.45, 0.5, 1.0, -0.8])              # (given unsorted: predict_dop sorts)
            out["nu7"], out["dop_nu7_norm"] = drt.predict_dop(nu=nu7, normalize=True, return_nu=True)
            out["dop_basis_matrix"] = basis.construct_func_eval_matrix(drt.basis_nu, out["dop_nu"], drt.nu_basis_type,
                                                                       epsilon=drt.nu_epsilon, order=0, zga_params=None)
            out["dop_normalize_by"] = drt.get_dop_norm(out["dop_nu"], True, None, (0, 1))
            out.update(basis_nu=drt.basis_nu, nu_epsilon=np.float64(drt.nu_epsilon), dop_scale_vector=drt.dop_scale_vector,
                       nu_basis_area=np.float64(drt.nu_basis_area))
    path = os.path.join(GOLDEN, f"refrun_response_predict_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{os.path.basename(path)}: {os.path.getsize(path) // 1024} KiB, {len(out)} arrays, n_tau {len(drt.basis_tau)}")


if __name__ == "__main__":
    meas = synth.hybrid_measurement(seed=0)
    make("hybrid_s0", meas, dict(BASE, fit_dop=False), {})
    make("hybrid_s0_dop", meas, dict(BASE, fit_dop=True), {})
    make("hybrid_s0_dop_solverp", meas, dict(BASE, fit_dop=True), dict(solve_rp=True))
    meas3 = synth.hybrid_measurement(seed=2, n_post=80, extra_steps=((2.0, -2e-3), (3.0, 1e-3)))
    make("hybrid_3step", meas3, dict(BASE, fit_dop=False), dict(vz_offset_scale=0.5, vz_offset_eps=2))
    make("chrono_s1", meas[:3] + (None, None), dict(BASE, fit_dop=False), {})
    g = np.load(os.path.join(GOLDEN, "ref_test_drt_fit_eis.npz"))
    eis = (None, None, None, np.asarray(g["freq"], dtype=float), np.asarray(g["z"], dtype=complex))
    make("golden71_dop", eis, dict(BASE, fit_dop=True), {})
    make("golden71_cap", eis, dict(BASE, fit_capacitance=True, fit_dop=False), {})
