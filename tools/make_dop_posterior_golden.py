"""Generate the DOP posterior fixtures under tests/golden/ (build container only: imports the reference through the shims of
oracle/refshim, like tools/make_response_golden.py).  One file per case, runs of the reference on the inputs of the
refrun_response_predict_* files of the same name:

  refrun_dop_posterior_golden71_dop.npz            fit_eis of the 71-point known-answer spectrum with fit_dop=True
  refrun_dop_posterior_hybrid_s0_dop.npz           fit_hybrid on synth.hybrid_measurement(seed=0) with fit_dop=True
  refrun_dop_posterior_hybrid_s0_dop_solverp.npz   ... with solve_rp=True (post-fit scales, rescaled DOP columns)

Each holds the reference's p_matrix, dop_scale_vector, coefficient_scale and dop_indices; on predict_dop's own 1034-point grid, for
order 0, 1, 2 and normalize False / True (keys ..._o<order>_n<0|1>): np.diag(estimate_dop_cov), predict_dop_ci's lo and hi, the mean
(predict_dop with predict_dop_ci's normalize_quantiles), and per order the evaluation matrix, with normalize_by once; the full
estimate_dop_cov on basis_nu and on the sorted seven-point grid of the response fixture, plain and normalised; one var_floor case;
a second quantile pair (0.16, 0.84).  No 1034 x 1034 matrix is stored (hybdrt/models/drt1d.py:3153-3258, 4116-4138).

    python tools/make_dop_posterior_golden.py
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

from hybdrt.matrices import basis  # noqa: E402
from hybdrt.models import DRT  # noqa: E402

from hipdrt import synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
BASE = dict(fit_inductance=True, fit_capacitance=False, fit_ohmic=True, fit_dop=True)
NQ = (0.25, 0.75)                       # predict_dop_ci's normalize_quantiles
Q2 = (0.16, 0.84)


@contextlib.contextmanager
def quiet():
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()):
        warnings.simplefilter("ignore")
        yield


def make(name, meas, fit_kw):
    times, i_signal, v_signal, freq, z = meas
    with quiet():
        drt = DRT(**BASE)
        if times is None:
            drt.fit_eis(freq, z, **fit_kw)
        else:
            drt.fit_hybrid(times, i_signal, v_signal, freq, z, **fit_kw)
        nu, _ = drt.predict_dop(return_nu=True)
        out = dict(p_matrix=np.asarray(drt.fit_parameters["p_matrix"], dtype=float), dop_scale_vector=np.asarray(drt.dop_scale_vector, dtype=float),
                   coefficient_scale=np.float64(drt.coefficient_scale), dop_indices=np.asarray(drt.dop_indices, dtype=np.int64),
                   basis_nu=drt.basis_nu, nu_epsilon=np.float64(drt.nu_epsilon), nu_basis_area=np.float64(drt.nu_basis_area), nu=nu,
                   normalize_by=drt.get_dop_norm(nu, True, None, NQ))
        for order in (0, 1, 2):
            out[f"basis_matrix_o{order}"] = basis.construct_func_eval_matrix(drt.basis_nu, nu, drt.nu_basis_type, epsilon=drt.nu_epsilon,
                                                                             order=order, zga_params=None)
            for norm in (False, True):
                tag = f"o{order}_n{int(norm)}"
                out[f"var_{tag}"] = np.diag(drt.estimate_dop_cov(nu, order=order, normalize=norm)).copy()
                out[f"lo_{tag}"], out[f"hi_{tag}"] = drt.predict_dop_ci(nu=nu, order=order, normalize=norm)
                out[f"mu_{tag}"] = drt.predict_dop(nu=nu, order=order, normalize=norm, normalize_quantiles=NQ)
        out["q2"] = np.array(Q2)
        out["lo_q2"], out["hi_q2"] = drt.predict_dop_ci(nu=nu, quantiles=list(Q2))
        nu7 = np.sort(np.array([0.9, -1.0, 0.0, -0.45, 0.5, 1.0, -0.8]))
        out["nu7"] = nu7
        for tag, grid in (("basis", drt.basis_nu), ("nu7", nu7)):
            out[f"cov_{tag}_n0"] = drt.estimate_dop_cov(grid)
            out[f"cov_{tag}_n1"] = drt.estimate_dop_cov(grid, normalize=True)
            out[f"normalize_by_{tag}"] = drt.get_dop_norm(grid, True, None, NQ)
        floor = float(np.median(np.diag(out["cov_basis_n0"])))
        out["var_floor"] = np.float64(floor)
        out["cov_basis_floor"] = drt.estimate_dop_cov(drt.basis_nu, var_floor=floor)
    path = os.path.join(GOLDEN, f"refrun_dop_posterior_{name}.npz")
    np.savez_compressed(path, **out)
    print(f"{os.path.basename(path)}: {os.path.getsize(path) // 1024} KiB, {len(out)} arrays, n {out['p_matrix'].shape[0]}, "
          f"nu {len(nu)}, dop_indices {out['dop_indices'].tolist()}")


if __name__ == "__main__":
    g = np.load(os.path.join(GOLDEN, "ref_test_drt_fit_eis.npz"))
    make("golden71_dop", (None, None, None, np.asarray(g["freq"], dtype=float), np.asarray(g["z"], dtype=complex)), {})
    meas = synth.hybrid_measurement(seed=0)
    make("hybrid_s0_dop", meas, {})
    make("hybrid_s0_dop_solverp", meas, dict(solve_rp=True))
