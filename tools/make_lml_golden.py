"""Generate the log-marginal-likelihood fixtures under tests/golden/ (build container only: imports the reference through the shims
of oracle/refshim, like tools/make_candidates_golden.py) by calling the reference's own DRT.evaluate_lml
(hybdrt/models/drt1d.py:4513-4543 over qphb.evaluate_lml, hybdrt/models/qphb.py:1279-1344) on every history entry of four fits:

  refrun_evaluate_lml_golden71x91.npz       the 71-frequency known-answer spectrum (tests/golden/ref_test_drt_fit_eis.npz)
  refrun_evaluate_lml_golden71x91_neg.npz   the same spectrum with nonneg=False
  refrun_evaluate_lml_hybrid_s0.npz         fit_hybrid on synth.hybrid_measurement(seed=0)
  refrun_evaluate_lml_hybrid_dop_s0.npz     the same with DRT(fit_dop=True)

Per stored history entry: x, rho_vector, s_vectors, dop_rho_vector (zeros without a DOP block), upstream's
evaluate_lml(history_entry=...) (NaN where its beta is negative) and the eight terms logdet_p, logdet_prior, wy2, fit2, cross, slw,
xox, l1x formed with upstream's own calculate_qp_l2_matrix / calculate_pq / np.linalg.slogdet, plus beta.  For the final state
also the value and the terms under update_hypers={'l2_lambda_0': 2 l2_lambda_0}, update_hypers={'derivative_weights': [1.5, 1, 0]}
and weights=0.5 est_weights.  And what the statement (hipdrt/models/lml.py) needs to be checked without a device: est_weights, rm,
rv, the padded penalty matrices, the l1 vector, the hyper-parameters that reach the formula, the special-parameter layout; and the
fit inputs.

Condition, asserted here: every stored entry has |beta| >= 1e-6 |W y|^2, so that the sign of beta -- the NaN pattern -- is out of
reach of rounding.  An entry that misses it is dropped and named in `dropped` (at most one per fit).  Every fixture keeps at least
one finite entry and, except golden71x91_neg if it has none, one NaN entry.

    python tools/make_lml_golden.py
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

from hybdrt.models import DRT, qphb  # noqa: E402

from hipdrt import synth  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
CTOR = dict(fit_inductance=True, fit_capacitance=False, fit_dop=False, fit_ohmic=True)
TERMS = ("logdet_p", "logdet_prior", "wy2", "fit2", "cross", "slw", "xox", "l1x")
BETA_MARGIN = 1e-6


@contextlib.contextmanager
def quiet():
    with warnings.catch_warnings(), contextlib.redirect_stdout(io.StringIO()), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        yield


def terms_of(drt, entry, weights=None, update_hypers=None):
    """the eight terms and beta of one state, by upstream's own functions"""
    qp = drt.qphb_params
    hypers = dict(qp["hypers"], **(update_hypers or {}))
    w = qp["est_weights"] if weights is None else weights
    args = (hypers, entry["rho_vector"], entry["dop_rho_vector"], qp["penalty_matrices"], entry["s_vectors"],
            drt.fit_kwargs["penalty_type"], drt.special_qp_params)
    omega = qphb.calculate_qp_l2_matrix(*args)
    p_matrix, _ = qphb.calculate_pq(qp["rm"], qp["rv"], qp["penalty_matrices"], drt.fit_kwargs["penalty_type"], hypers,
                                    qp["l1_lambda_vector"], entry["rho_vector"], entry["dop_rho_vector"], entry["s_vectors"], w,
                                    drt.special_qp_params)
    (sp, ld_p), (so, ld_o) = np.linalg.slogdet(p_matrix), np.linalg.slogdet(omega)
    assert sp > 0 and so > 0
    x = entry["x"]
    wr, wy = w * (qp["rm"] @ x), w * qp["rv"]
    t = dict(logdet_p=ld_p, logdet_prior=ld_o, wy2=wy @ wy, fit2=wr @ wr, cross=wr @ wy, slw=np.sum(np.log(w)), xox=x @ omega @ x,
             l1x=np.sum(np.broadcast_to(qp["l1_lambda_vector"], x.shape) * x))
    beta = 0.5 * (t["wy2"] - t["fit2"] - t["xox"]) + 1
    return np.array([t[k] for k in TERMS], dtype=float), float(beta)


def make(name, ctor, fit, inputs):
    with quiet():
        drt = DRT(**ctor)
        fit(drt)
        qp, hist = drt.qphb_params, drt.qphb_history
        has_dop = "x_dop" in drt.special_qp_params
        rows, dropped = [], []
        for i, e in enumerate(hist):
            t, beta = terms_of(drt, e)
            if abs(beta) < BETA_MARGIN * t[TERMS.index("wy2")]:
                dropped.append(i)
                continue
            rows.append(dict(index=i, x=e["x"], rho=e["rho_vector"], s=np.asarray(e["s_vectors"], dtype=float),
                             dop_rho=np.asarray(e["dop_rho_vector"], dtype=float) if has_dop else np.zeros(3),
                             lml=float(drt.evaluate_lml(history_entry=e)), terms=t, beta=beta))
        assert len(dropped) <= 1, (name, dropped)
        final = hist[-1]
        l2 = float(qp["hypers"]["l2_lambda_0"])
        variants = {}
        for tag, kw in (("l2x2", dict(update_hypers={"l2_lambda_0": 2 * l2})),
                        ("dw", dict(update_hypers={"derivative_weights": np.array([1.5, 1.0, 0.0])})),
                        ("halfw", dict(weights=0.5 * qp["est_weights"]))):
            t, beta = terms_of(drt, final, **kw)
            variants[tag] = (float(drt.evaluate_lml(**kw)), t, beta)
        lml_default = float(drt.evaluate_lml())
    lml = np.array([r["lml"] for r in rows])
    assert np.any(np.isfinite(lml)), name
    assert np.any(np.isnan(lml)) or name == "golden71x91_neg", name
    # upstream returns NaN exactly where its beta is negative
    assert np.array_equal(np.isnan(lml), np.array([r["beta"] < 0 for r in rows])), name
    sp = drt.special_qp_params
    names = sorted(sp, key=lambda k: sp[k]["index"])
    hyp = qp["hypers"]
    out = dict(
        entry_index=np.array([r["index"] for r in rows], dtype=np.int64), dropped=np.array(dropped, dtype=np.int64),
        x=np.array([r["x"] for r in rows]), rho_vector=np.array([r["rho"] for r in rows]), s_vectors=np.array([r["s"] for r in rows]),
        dop_rho_vector=np.array([r["dop_rho"] for r in rows]), has_dop=np.int64(has_dop), lml=lml,
        terms=np.array([r["terms"] for r in rows]), term_names=np.array(TERMS), beta=np.array([r["beta"] for r in rows]),
        lml_final=np.float64(lml_default), final_is_last=np.int64(rows[-1]["index"] == len(hist) - 1),
        est_weights=np.asarray(qp["est_weights"], dtype=float), rm=np.asarray(qp["rm"], dtype=float), rv=np.asarray(qp["rv"], dtype=float),
        l1_lambda_vector=np.broadcast_to(np.asarray(qp["l1_lambda_vector"], dtype=float), final["x"].shape).copy(),
        **{f"m{k}": np.asarray(qp["penalty_matrices"][f"m{k}"], dtype=float) for k in range(3)},
        l2_lambda_0=np.float64(l2), derivative_weights=np.asarray(hyp["derivative_weights"], dtype=float),
        dop_l2_lambda_0=np.float64(hyp.get("dop_l2_lambda_0", 0.0)),
        dop_derivative_weights=np.asarray(hyp.get("dop_derivative_weights", np.zeros(3)), dtype=float),
        special_names=np.array(names), special_index=np.array([sp[k]["index"] for k in names], dtype=np.int64),
        special_size=np.array([sp[k].get("size", 1) for k in names], dtype=np.int64),
        coefficient_scale=np.float64(drt.coefficient_scale), **inputs)
    for tag, (val, t, beta) in variants.items():
        assert abs(beta) >= BETA_MARGIN * t[TERMS.index("wy2")], (name, tag, beta)
        out[f"lml_{tag}"], out[f"terms_{tag}"], out[f"beta_{tag}"] = np.float64(val), t, np.float64(beta)
    path = os.path.join(GOLDEN, f"refrun_evaluate_lml_{name}.npz")
    np.savez_compressed(path, **out)
    assert os.path.getsize(path) < (1 << 20), os.path.getsize(path)
    ratio = np.abs(out["beta"]) / out["terms"][:, TERMS.index("wy2")]
    print(f"{name}: {os.path.getsize(path)} bytes; entries {out['entry_index'].tolist()} dropped {dropped}; lml {np.round(lml, 6).tolist()}; "
          f"min |beta| / |Wy|^2 {ratio.min():.2g}; final {lml_default:.9f}; variants "
          + ", ".join(f"{k} {v[0]:.9f}" for k, v in variants.items()))


if __name__ == "__main__":
    g = np.load(os.path.join(GOLDEN, "ref_test_drt_fit_eis.npz"))
    freq, z = np.asarray(g["freq"], dtype=float), np.asarray(g["z"], dtype=complex)
    make("golden71x91", CTOR, lambda drt: drt.fit_eis(freq, z), dict(freq=freq, z=z))
    make("golden71x91_neg", CTOR, lambda drt: drt.fit_eis(freq, z, nonneg=False), dict(freq=freq, z=z))
    meas = synth.hybrid_measurement(seed=0)
    inputs = dict(zip(("times", "i_signal", "v_signal", "freq", "z"), (np.asarray(a) for a in meas)), seed=np.int64(0))
    make("hybrid_s0", CTOR, lambda drt: drt.fit_hybrid(*meas), inputs)
    make("hybrid_dop_s0", dict(CTOR, fit_dop=True), lambda drt: drt.fit_hybrid(*meas), inputs)
