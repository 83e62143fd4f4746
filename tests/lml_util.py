"""Helpers of tests/test_lml_util.py (CPU) and tests/test_gpu_lml.py: the fixtures of tools/make_lml_golden.py, the extended-precision
log-determinant the kernel is measured against, the test matrices of the kernel test and the bounds of tests/lml_bounds.json."""
import json
import os

import numpy as np

from conftest import GOLDEN, ROOT

FIXTURES = ("golden71x91", "golden71x91_neg", "hybrid_s0", "hybrid_dop_s0")
TERMS = ("logdet_p", "logdet_prior", "wy2", "fit2", "cross", "slw", "xox", "l1x")
VARIANTS = ("l2x2", "dw", "halfw")
KERNEL_N = (1, 31, 33, 93, 528, 529, 1030)       # both LDS forms (<= 528 | > 528), the 32-block edge on both sides, padding 1 and 31


def load(name):
    return np.load(os.path.join(GOLDEN, f"refrun_evaluate_lml_{name}.npz"))


def hypers_of(g, **update):
    h = dict(l2_lambda_0=float(g["l2_lambda_0"]), derivative_weights=g["derivative_weights"].copy(),
             dop_l2_lambda_0=float(g["dop_l2_lambda_0"]), dop_derivative_weights=g["dop_derivative_weights"].copy())
    h.update(update)
    return h


def special_of(g):
    return {str(k): dict(index=int(i), size=int(s)) for k, i, s in zip(g["special_names"], g["special_index"], g["special_size"])}


def penalty_of(g):
    return {f"m{k}": g[f"m{k}"] for k in range(3)}


def variant_kw(g, tag):
    """(update_hypers, weights) of the three recorded variants of the final state"""
    if tag == "l2x2":
        return dict(l2_lambda_0=2 * float(g["l2_lambda_0"])), None
    if tag == "dw":
        return dict(derivative_weights=np.array([1.5, 1.0, 0.0])), None
    return {}, 0.5 * g["est_weights"]


def statement_terms(g, i, update=None, weights=None):
    """models/lml.py on recorded entry i of fixture g -> (terms as an array in TERMS order, status)"""
    from hipdrt.models import lml
    t, status = lml.lml_terms(g["x"][i], g["rho_vector"][i], g["s_vectors"][i], g["dop_rho_vector"][i] if int(g["has_dop"]) else None,
                              g["est_weights"] if weights is None else weights, g["rm"], g["rv"], penalty_of(g),
                              hypers_of(g, **(update or {})), special_of(g), l1=g["l1_lambda_vector"])
    return np.array([t[k] for k in TERMS]), status


def omega_and_p(g, i):
    from hipdrt.models import lml
    omega = lml.l2_matrix(hypers_of(g), g["rho_vector"][i], g["dop_rho_vector"][i], penalty_of(g), g["s_vectors"][i], special_of(g))
    wrm = g["est_weights"][:, None] * g["rm"]
    return omega, omega + wrm.T @ wrm


def longdouble_logdet(a):
    """2 sum(log(diag(L))) of the Cholesky factor of a, formed left-looking in np.longdouble (x87 extended precision: 64-bit
    mantissa) from the lower triangle -- the reference of the kernel test.  Raises LinAlgError for a matrix that is not positive
    definite."""
    a = np.asarray(a, dtype=np.longdouble)
    n = a.shape[0]
    L = np.zeros((n, n), dtype=np.longdouble)
    for j in range(n):
        v = a[j:, j] - L[j:, :j] @ L[j, :j]
        if not v[0] > 0:
            raise np.linalg.LinAlgError(f"pivot {j} is not positive")
        L[j:, j] = v / np.sqrt(v[0])
    return float(2 * np.sum(np.log(np.diag(L))))


def embed(a, n, rng):
    """a symmetric positive definite matrix at size n: its leading block, or a on the diagonal beside a positive diagonal"""
    k = a.shape[0]
    if n <= k:
        return np.array(a[:n, :n])
    out = np.diag(np.exp(rng.uniform(-3, 3, n)))
    out[:k, :k] = a
    return out


def kernel_matrices(n, seed=0):
    """(gram + ridge, prescribed eigenvalues log-spaced over 3e-6 ... 3e4, the known-answer fixture's final P embedded) at size n"""
    rng = np.random.default_rng(1000 * seed + n)
    a = rng.standard_normal((n + 5, n))
    gram = a.T @ a + 1e-3 * np.eye(n)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    eig = (q * np.logspace(np.log10(3e-6), np.log10(3e4), n)[None, :]) @ q.T
    eig = 0.5 * (eig + eig.T)
    g = load("golden71x91")
    _, p = omega_and_p(g, len(g["lml"]) - 1)
    return np.stack([gram, eig, embed(p, n, rng)])


_bounds = None
MEASURED = []          # (label, measured) of this process, for the measuring scripts


def bound_of(label):
    global _bounds
    if _bounds is None:
        with open(os.path.join(ROOT, "tests", "lml_bounds.json")) as f:
            _bounds = json.load(f)
    return float(_bounds[label][1])


def rel_dev(got, ref):
    """largest deviation relative to max(1, |reference value|), entry by entry"""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float(np.max(np.abs(got - ref) / np.maximum(1.0, np.abs(ref)))) if got.size else 0.0


def check(label, got, ref, absolute=False):
    """got against the recorded reference within tests/lml_bounds.json[label]: relative to max(1, |ref|) per entry, or absolute
    (lml, over the finite entries; the NaN pattern must be identical).  Prints and records the figure before it asserts."""
    got, ref = np.asarray(got, dtype=float), np.asarray(ref, dtype=float)
    assert got.shape == ref.shape, (label, got.shape, ref.shape)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), (label, "NaN pattern", got, ref)
    fin = ~np.isnan(ref)
    dev = (float(np.max(np.abs(got[fin] - ref[fin]))) if fin.any() else 0.0) if absolute else rel_dev(got[fin], ref[fin])
    MEASURED.append((label, dev))
    print(f"lml {label}: measured {dev:.3e}")
    bound = bound_of(label)
    assert dev <= bound, f"{label}: deviation {dev:.3e} exceeds the bound {bound:.1e}"
    return dev
