"""The log marginal likelihood (evidence) of a fit, stated in numpy: what ``DRT.evaluate_lml`` (hybdrt/models/drt1d.py:4513-4543)
computes through ``qphb.evaluate_lml`` (hybdrt/models/qphb.py:1279-1344), split where the device splits it.

``lml_terms`` gives the eight numbers ``hipdrt_plan_lml_terms`` (include/hipdrt.h) gives per spectrum; ``lml_from_terms`` is
upstream's last two lines on them, for a scalar or a batch.  ``DRT.evaluate_lml_batch`` runs the first on the device and the second
here; this module is the statement both are tested against, and it needs no device.

The determinants are ``2 sum(log(diag(L)))`` of the Cholesky factor, as the device forms them (the kernel reads ``1 / L_ii`` off the
inverted diagonal blocks its factorisation keeps and returns minus twice the sum of their logarithms: the same number).  Upstream
calls ``np.linalg.slogdet``; for the positive definite matrices of a fit the two agree to rounding, and a matrix whose Cholesky
factorisation fails is reported where upstream either raises ('... is negative - not PSD') or carries on with a meaningless number."""
import numpy as np

TERMS = ("logdet_p", "logdet_prior", "wy2", "fit2", "cross", "slw", "xox", "l1x")
# the keys of a hyper dict that reach the formula (qphb.py:68-78); every other key of get_default_hypers is accepted and ignored
LML_HYPERS = ("l2_lambda_0", "derivative_weights", "dop_l2_lambda_0", "dop_derivative_weights")


def get_num_special(special):
    return int(sum(sp.get("size", 1) for sp in special.values())) if special else 0


def l2_matrix(hypers, rho_vector, dop_rho_vector, penalty_matrices, s_vectors, special):
    """qphb.calculate_qp_l2_matrix for the integral penalty (hybdrt/models/qphb.py:53-120): sum over the orders with a positive
    derivative weight of S_k^1/2 M_k' S_k^1/2, M_k' = M_k with its DRT block (indices >= the number of special unknowns) times
    l2_lambda_0 w_k rho_k and its DOP block times dop_l2_lambda_0 dop_w_k dop_rho_k.  The special diagonal of M_k (the 1e-6-scale
    penalties of R_inf, inductance, ...) is in it unscaled.  ``special``: special_qp_params ({name: {'index', 'size'}})."""
    ns = get_num_special(special)
    dop = special.get("x_dop") if special else None
    out = np.zeros_like(np.asarray(penalty_matrices["m0"], dtype=float))
    for k, dw in enumerate(np.broadcast_to(np.asarray(hypers["derivative_weights"], dtype=float), (3,))):
        if dw > 0:
            sq = np.asarray(s_vectors[k], dtype=float) ** 0.5
            mk = np.array(penalty_matrices[f"m{k}"], dtype=float)
            mk[ns:, ns:] *= hypers["l2_lambda_0"] * dw * rho_vector[k]
            if dop is not None:
                lo, hi = dop["index"], dop["index"] + dop.get("size", 1)
                mk[lo:hi, lo:hi] *= hypers["dop_l2_lambda_0"] * np.asarray(hypers["dop_derivative_weights"], dtype=float)[k] * dop_rho_vector[k]
            out += sq[:, None] * mk * sq[None, :]
    return out


def cholesky_logdet(a):
    """2 sum(log(diag(chol(a)))) -> (logdet, status): status -1 and NaN where a is not positive definite"""
    try:
        return 2.0 * float(np.sum(np.log(np.diag(np.linalg.cholesky(np.asarray(a, dtype=float)))))), 0
    except np.linalg.LinAlgError:
        return np.nan, -1


def lml_terms(x, rho, s, dop_rho, w, rm, rv, penalty_matrices, hypers, special, l1=None):
    """The eight terms of one spectrum, and the status of the two factorisations: x (n,), rho (3,), s (3, n), dop_rho (3,) or None,
    w, rv (m,), rm (m, n) -> (dict over TERMS, status)."""
    x, w, rv, rm = (np.asarray(a, dtype=float) for a in (x, w, rv, rm))
    omega = l2_matrix(hypers, rho, dop_rho, penalty_matrices, s, special)
    wrm = w[:, None] * rm
    ld_p, st_p = cholesky_logdet(omega + wrm.T @ wrm)
    ld_o, st_o = cholesky_logdet(omega)
    wy, wr = w * rv, w * (rm @ x)
    terms = dict(logdet_p=ld_p, logdet_prior=ld_o, wy2=float(wy @ wy), fit2=float(wr @ wr), cross=float(wr @ wy),
                 slw=float(np.sum(np.log(w))), xox=float(x @ omega @ x),
                 l1x=0.0 if l1 is None else float(np.sum(np.broadcast_to(np.asarray(l1, dtype=float), x.shape) * x)))
    return terms, (-1 if st_p or st_o else 0)


def lml_from_terms(terms, m, alpha_0=1, beta_0=1):
    """qphb.py:1336-1342 on the terms (scalars or arrays over a batch).  A negative beta gives NaN and beta == 0 gives +inf, as
    upstream's np.log does, without its warnings."""
    from scipy.special import loggamma
    t = {k: np.asarray(terms[k], dtype=float) for k in ("logdet_p", "logdet_prior", "wy2", "fit2", "slw", "xox")}
    alpha = m / 2 + alpha_0
    beta = 0.5 * (t["wy2"] - t["fit2"] - t["xox"]) + beta_0
    with np.errstate(invalid="ignore", divide="ignore"):
        lml = 0.5 * (t["logdet_prior"] - t["logdet_p"]) + t["slw"] + loggamma(alpha) - loggamma(alpha_0) \
            + alpha_0 * np.log(beta_0) - alpha * np.log(beta)
    return lml if np.ndim(lml) else float(lml)


def updated_hypers(hypers, update_hypers, known):
    """upstream's ``qphb_hypers.update(update_hypers)`` with a check it lacks: a key outside ``known`` (the keys of a hyper dict) is a
    ValueError instead of a silent no-op"""
    update_hypers = dict(update_hypers or {})
    bad = sorted(set(update_hypers) - set(known))
    if bad:
        raise ValueError(f"update_hypers: unknown key(s) {bad}; of the hyper-parameters only {list(LML_HYPERS)} reach the evidence")
    return dict(hypers, **update_hypers)


def entry_state(history_entry):
    """(x, rho_vector, s_vectors, dop_rho_vector) of a history entry in upstream's form (qphb.py:947-964)"""
    missing = [k for k in ("x", "rho_vector", "s_vectors") if history_entry.get(k) is None]
    if missing:
        raise ValueError(f"history_entry lacks {missing}: the evidence needs x, rho_vector and s_vectors (and dop_rho_vector for a fit "
                         "with fit_dop), as upstream's history entries hold them.  The entries of this project's qphb_history carry no "
                         "s_vectors; pass the state of a recorded step with evaluate_lml_batch(step=...) or any state with state=...")
    return history_entry["x"], history_entry["rho_vector"], history_entry["s_vectors"], history_entry.get("dop_rho_vector")
