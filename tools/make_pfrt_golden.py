"""Generate the PFRT fixture under tests/golden/ (build container only: imports the reference through the shims of
oracle/refshim, like tools/make_peaks_golden.py):

  refrun_pfrt_golden71x91.npz   the reference's 71-frequency known-answer spectrum (tests/golden/ref_test_drt_fit_eis.npz) through
                                DRT.pfrt_fit_eis plain and with nonneg=False (two-pass search), and for each fit: factors, step_x,
                                step_llh, step_p_mat of the steps 0, 5 and 10 (all eleven would pass the size limit of a committed
                                file), per step on get_tau_eval(10) the rows f and fxx and both variances as predict_pfrt forms
                                them (extend_var, floor 1e-5) and before the clamp and the floor, step_pfrt, raw_pfrt, and
                                predict_pfrt for four option sets: defaults, smooth=False with normalize=False, integrate=True,
                                and tau=np.logspace(-7, 2, 181).

(hybdrt/models/drt1d.py:2558-2698 _pfrt_fit_core, 2716-2858 predict_pfrt, 3063-3151 estimate_distribution_cov)

The fixture is only written when the margins hold that the tests' exact comparisons of peak positions rely on: every peak
candidate of every step (a local maximum of a pass) keeps a relative distance of at least 1e-4 from the height and the prominence
threshold, and in the two-pass run |f| at every candidate is at least 1e-6 of max |f|.

    python tools/make_pfrt_golden.py
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

from hipdrt.models import peaks  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CTOR = dict(fit_inductance=True, fit_capacitance=False, fit_dop=False, fit_ohmic=True)
FITS = {"plain": dict(), "nn": dict(nonneg=False)}
OPTION_SETS = {"default": dict(), "raw": dict(smooth=False, normalize=False), "int": dict(integrate=True),
               "tau181": dict(tau=np.logspace(-7, 2, 181))}
P_STEPS = (0, 5, 10)
HEIGHT, PROMINENCE, FLOOR = 1e-3, 5e-3, 1e-5
MARGIN, F_MARGIN = 1e-4, 1e-6


@contextlib.contextmanager
def quiet():
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter("ignore")
        yield


def margins(f, fxx, search):
    """(smallest relative distance of a candidate from a threshold, smallest |f| / max |f| at a candidate of a two-pass search)"""
    gap, fgap = np.inf, np.inf
    for s in ((search,) if search != 0 else (-1, 1)):
        idx, info = peaks.find_peaks_1d(-s * fxx)
        for vals, thr in ((info["peak_heights"], HEIGHT), (info["prominences"], PROMINENCE)):
            if len(vals):
                gap = min(gap, float(np.min(np.abs(vals - thr))) / thr)
        if search == 0 and len(idx):
            fgap = min(fgap, float(np.min(np.abs(f[idx]))) / float(np.max(np.abs(f))))
    return gap, fgap


def make(freq, z):
    out = dict(p_steps=np.array(P_STEPS))
    for tag, fit_kw in FITS.items():
        with quiet():
            drt = DRT(**CTOR)
            drt.pfrt_fit_eis(freq, z, **fit_kw)
            pr = drt.pfrt_result
            sign = drt.default_dist_sign
            tau = drt.get_tau_eval(10)
            nonneg = bool(drt.fit_kwargs["nonneg"])
            search = sign if (nonneg and sign != 0) else 0
            rows = {k: [] for k in ("f", "fxx", "var_f", "var_fxx", "var_f_raw", "var_fxx_raw")}
            for x_raw, p_mat in zip(pr["step_x"], pr["step_p_mat"]):
                x_drt = drt.extract_qphb_parameters(x_raw)["x"]
                for name, order in (("f", 0), ("fxx", 2)):
                    rows[name].append(drt.predict_drt(tau, x=x_drt, sign=sign, order=order, normalize=True))
                    kw = dict(p_matrix=p_mat, order=order, sign=sign, normalize=True)
                    rows[f"var_{name}"].append(np.diag(drt.estimate_distribution_cov(tau, var_floor=FLOOR, extend_var=True, **kw)))
                    rows[f"var_{name}_raw"].append(np.diag(drt.estimate_distribution_cov(tau, **kw)))
            for name, kw in OPTION_SETS.items():
                out[f"{tag}_pfrt_{name}"] = np.asarray(drt.predict_pfrt(**kw))
            # (predict_pfrt leaves tau_pfrt, raw_pfrt and step_pfrt in pfrt_result; they do not depend on the option set)
            assert np.array_equal(pr["tau_pfrt"], tau)
        rows = {k: np.array(v) for k, v in rows.items()}
        gap, fgap = np.inf, np.inf
        for f, fxx in zip(rows["f"], rows["fxx"]):
            g1, g2 = margins(f, fxx, search)
            gap, fgap = min(gap, g1), min(fgap, g2)
        assert gap >= MARGIN, (tag, "a peak candidate sits within 1e-4 of a threshold", gap)
        assert search != 0 or fgap >= F_MARGIN, (tag, "|f| at a candidate of the two-pass search below 1e-6 of max |f|", fgap)
        out.update({f"{tag}_{k}": v for k, v in rows.items()})
        t_left, t_right = 1 / (2 * np.pi * np.max(freq)), 1 / (2 * np.pi * np.min(freq))
        out.update({f"{tag}_factors": np.asarray(pr["factors"]), f"{tag}_step_x": np.array(pr["step_x"]),
                    f"{tag}_step_llh": np.array(pr["step_llh"], dtype=float),
                    f"{tag}_step_p_mat": np.array([pr["step_p_mat"][i] for i in P_STEPS]),
                    f"{tag}_step_pfrt": np.array(pr["step_pfrt"]), f"{tag}_raw_pfrt": np.array(pr["raw_pfrt"]),
                    f"{tag}_tau_pfrt": tau, f"{tag}_search": np.int64(search), f"{tag}_nonneg": np.int64(nonneg),
                    f"{tag}_ext": np.array([int(np.argmin(np.abs(tau - t_left))) + 1, int(np.argmin(np.abs(tau - t_right)))]),
                    f"{tag}_coefficient_scale": np.float64(drt.coefficient_scale)})
        print(tag, "search", search, "peaks per step", [int(np.count_nonzero(r)) for r in pr["step_pfrt"]],
              "argmax", int(np.argmax(out[f"{tag}_pfrt_default"])), "margins %.2g %.2g" % (gap, fgap))
    out["tau181"] = OPTION_SETS["tau181"]["tau"]
    path = os.path.join(GOLDEN, "refrun_pfrt_golden71x91.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    g = np.load(os.path.join(GOLDEN, "ref_test_drt_fit_eis.npz"))
    make(g["freq"], g["z"])
