"""Helpers of the candidate-scoring tests: the likelihood sums in extended precision and a bound on what any float64 evaluation
of them may deviate, from u = 2^-53 and the operand magnitudes alone."""
import numpy as np

from gram_util import extended_dtype

U = 2.0 ** -53


def reference_and_bound(x, rm, rv, vmm, var_floor):
    """x (C, B, n), rm (m, n) or (B, m, n), rv (B, m), vmm (m, m), var_floor (B,) -> (rss, slw, rss_bound, slw_bound), all (C, B):
    hipdrt.models.candidates.candidate_llh_terms in np.longdouble (64-bit significand, asserted) and absolute bounds on
    |float64 result - exact| for an evaluation that sums in any order, with or without fused multiply-adds.  Derivation in
    tests/test_gpu_candidates.py's docstring; every line below is one sentence of it."""
    from hipdrt.models.candidates import candidate_llh_terms
    ld = extended_dtype()
    assert ld is not None, "np.longdouble carries no 64-bit significand here"
    C, B, n = x.shape
    m = rv.shape[1]
    u = ld(U)
    out = [np.empty((C, B)) for _ in range(4)]
    for b in range(B):
        A = np.asarray(rm[b] if rm.ndim == 3 else rm, dtype=ld)
        X, y, V, vf = np.asarray(x[:, b], dtype=ld), np.asarray(rv[b], dtype=ld), np.asarray(vmm, dtype=ld), ld(var_floor[b])
        rss, slw = candidate_llh_terms(X, A, y, V, vf)
        yh = X @ A.T
        dy = (n + 2) * u * (np.abs(X) @ np.abs(A).T)                    # rm x, n products summed in any order
        r = yh - y
        d = dy + u * np.abs(r)                                          # the subtraction rounds once
        e2 = 2 * np.abs(r) * d + d * d + u * r * r                      # r^2
        s = (r * r) @ V.T
        es = e2 @ np.abs(V).T + (m + 2) * u * ((r * r) @ np.abs(V).T)   # vmm r^2, m products
        v = np.maximum(s, vf)                                           # (max is 1-Lipschitz: the floor adds nothing)
        assert np.all(es < 0.25 * v), "the case is too ill-conditioned for a first-order bound"
        rw = es / (v - es) + 2 * u                                      # v^-1/2: at most the relative error of v; sqrt, division
        w = np.maximum(1 / np.sqrt(v), ld(1e-10))
        wy, wr = w * yh, w * y
        dwy = w * dy + np.abs(wy) * (rw + u)
        dwr = np.abs(wr) * (rw + u)
        k = (m + 4) * u                                                 # a sum of m terms, each product rounded
        da = np.sum(2 * np.abs(wy) * dwy + dwy * dwy, -1) + k * np.sum(wy * wy, -1)
        dc = np.sum(np.abs(wy) * dwr + np.abs(wr) * dwy + dwy * dwr, -1) + k * np.sum(np.abs(wy * wr), -1)
        dd = np.sum(2 * np.abs(wr) * dwr + dwr * dwr, -1) + k * np.sum(wr * wr, -1)
        mag = np.sum(wy * wy, -1) + 2 * np.sum(np.abs(wy * wr), -1) + np.sum(wr * wr, -1)
        drss = da + 2 * dc + dd + 3 * u * mag                           # a - 2 c + d
        lw = np.abs(np.log(w))
        dslw = np.sum(2 * rw + 4 * u * lw, -1) + k * np.sum(lw, -1)      # log: d(log w) <= 2 rw for rw < 1/2; 2 ulp of the routine
        # (the extended-precision reference is itself off by 2^-11 of these bounds)
        for o, val in zip(out, (rss, slw, 1.001 * drss, 1.001 * dslw)):
            o[:, b] = np.asarray(val, dtype=float)
    return out


def llh_case(rng, C, B, m, n, batched):
    """well-scaled random operands: rm (m, n) or (B, m, n), rv (B, m), a non-negative vmm with unit row sums (as the variance
    smoothing matrices are), x (C, B, n) and a floor far below every variance"""
    rm = rng.standard_normal((B, m, n) if batched else (m, n))
    rv = rng.standard_normal((B, m))
    vmm = rng.uniform(0.0, 1.0, (m, m))
    vmm /= vmm.sum(axis=1, keepdims=True)
    x = rng.standard_normal((C, B, n))
    return x, rm, rv, vmm, np.full(B, 1e-30)
