"""Cases, exact statement and error bound of the DOP posterior chain alone -- the reference of the chain-alone tests of
tests/test_gpu_dop_posterior.py (hipdrt_debug_dop_posterior), checked on the CPU by tests/test_dop_posterior_util.py.  Imports
posterior_util and gram_util and changes neither; imports neither the package under test nor the oracle.

    var_bi = rows_i' (S_b P_b S_b)^-1 rows_i        S_b = diag(s_b), s_b = 1 / dsv_b on the DOP block, 1 elsewhere
    rows sit at the unknowns dop_start .. dop_start + dop_size - 1 and are zero elsewhere

The device multiplies entry (i, j) of the packed P by s_i, then by s_j, with s = float64(1 / dsv): two float64 roundings per entry.

Exact target: s = float64(1 / dsv) is taken as DATA (the one correctly rounded division is part of the statement, not of the error),
the product S P S is formed in gram_util.extended_dtype() (64-bit significand), and the quadratic form comes from posterior_util's
refinement scheme: float64 Cholesky of the rounded product as the solver, residual and iterate in extended precision against the
extended product, converged when the last correction is at most 2^-60 kappa of the solution.

Bound: posterior_util's C_BOUND (n + 16) u kappa_2(SPS) var for the chain, plus 2 sqrt(n) u kappa_2(SPS) var for the scaling: the
device factors P' = fl(fl(P_ij s_i) s_j) instead of S P S, |dP'| <= 2 u |P'| elementwise (second-order terms dropped),
|| |A| ||_2 <= sqrt(n) ||A||_2, and a relative perturbation eps of P' in the 2-norm moves a quadratic form of its inverse by at most
eps kappa_2 of its value.  kappa_2 is computed the way posterior_util computes it (eigvalsh, n <= 600 here).
"""
import functools

import numpy as np

import gram_util as gu
import posterior_util as pu

U = gu.U
B = 3
# (n, dop_start, dop_size): one tile padded to 32; exactly one aligned tile; three tile edges crossed at both ends unaligned; the
# fixture's shape; the n > 528 form of the factor scratch
SHAPES = ((23, 2, 13), (64, 16, 16), (70, 5, 50), (150, 5, 50), (600, 3, 50))
NEVALS = (1, 16, 17, 40)
KAPPA_P = 1e3            # of every member's P before the scaling; S spans about four decades, so kappa_2(SPS) reaches ~1e10


def bound(n, kappa):
    """the relative bound on a variance, |var - exact| <= bound * exact"""
    return (pu.C_BOUND * (n + 16) + 2.0 * np.sqrt(n)) * U * kappa


def scale_vector(n, dop_start, dsv):
    """s [n]: float64(1 / dsv) on the DOP block, 1 elsewhere"""
    s = np.ones(n)
    s[dop_start:dop_start + len(dsv)] = 1.0 / np.asarray(dsv, dtype=np.float64)
    return s


def scaled_f64(P, s):
    """fl(fl(P_ij s_i) s_j) of the symmetric matrix of P's lower triangle: what the device's image holds"""
    return (gu.mirror_lower(np.asarray(P, dtype=np.float64)) * s[:, None]) * s[None, :]


def scaled_image(P, s):
    """the exact packed image [nchp^2 * 256] of the scaled P: lower tiles of scaled_f64, zeros beyond n and above the diagonal tiles"""
    return gu.pack_tiles(scaled_f64(P, s), P.shape[0], fill=0.0)


def scaled_ext(P, s):
    ext = gu.extended_dtype()
    return (gu.mirror_lower(np.asarray(P, dtype=np.float64)).astype(ext) * s.astype(ext)[:, None]) * s.astype(ext)[None, :]


def kappa_of(M):
    ev = np.linalg.eigvalsh(np.asarray(M, dtype=np.float64))
    return float(ev[-1] / ev[0])


def reference(Me, R, kappa, want_cov=False, max_iter=12):
    """posterior_util.reference for a matrix given in extended precision: dict(var, cov or None, corrections, iters, tol)"""
    from scipy.linalg import cho_factor, cho_solve
    ext = gu.extended_dtype()
    R = np.atleast_2d(np.asarray(R, dtype=np.float64))
    c = cho_factor(Me.astype(np.float64), lower=True)
    be = R.T.astype(ext)
    live = np.any(R != 0.0, axis=1)
    xe = cho_solve(c, R.T).astype(ext)
    tol = 2.0 ** -60 * max(kappa, 1.0)
    hist, ok = [], False
    for _ in range(max_iter):
        d = cho_solve(c, (be - Me @ xe).astype(np.float64))
        xe = xe + d.astype(ext)
        rel = np.max(np.abs(d), axis=0)[live] / np.max(np.abs(xe), axis=0)[live].astype(np.float64) if live.any() else np.zeros(1)
        hist.append(float(np.max(rel)))
        if hist[-1] <= tol:
            ok = True
            break
    if not ok:
        raise RuntimeError(f"refinement did not converge: corrections {hist}, wanted {tol:.3g}")
    return dict(var=np.sum(be * xe, axis=0), cov=(be.T @ xe) if want_cov else None, corrections=hist, iters=len(hist), tol=tol)


def make_dsv(nb, dop_size, seed):
    """exp of seeded Gaussians per member: about 1e-2 .. 1e2"""
    return np.exp(1.5 * np.random.default_rng(seed).standard_normal((nb, dop_size)))


@functools.lru_cache(maxsize=None)
def get_matrices(n, dop_start, dop_size):
    """the B members of a shape: P [B][n][n], dsv [B][dop_size], s [B][n], kappa [B] of S P S; read-only"""
    P = np.stack([pu.spd_matrix(n, KAPPA_P, 7000 + 10 * n + b)[0] for b in range(B)])
    dsv = make_dsv(B, dop_size, 9000 + n)
    s = np.stack([scale_vector(n, dop_start, dsv[b]) for b in range(B)])
    kappa = np.array([kappa_of(scaled_ext(P[b], s[b])) for b in range(B)])
    for v in (P, dsv, s, kappa):
        v.setflags(write=False)
    return dict(n=n, dop_start=dop_start, dop_size=dop_size, P=P, dsv=dsv, s=s, kappa=kappa)


@functools.lru_cache(maxsize=None)
def get_case(n, dop_start, dop_size, neval, want_cov=False):
    """(matrices, rows [neval][dop_size], references [B]); built once and shared: read-only"""
    m = get_matrices(n, dop_start, dop_size)
    rows = pu.make_rows("mixed", neval, dop_size, 100 * n + neval)
    R = pu.full_rows(rows, n, dop_start)
    refs = [reference(scaled_ext(m["P"][b], m["s"][b]), R, m["kappa"][b], want_cov) for b in range(B)]
    rows.setflags(write=False)
    return m, rows, refs


def var_ratio(var, ref, n, kappa):
    """worst |var - exact| / (bound * exact) over the rows; a zero row must give zero exactly"""
    exact = np.asarray(ref["var"])
    return gu.worst_ratio(var, exact, bound(n, kappa) * np.abs(exact).astype(np.float64))


def cov_ratio(cov, ref, n, kappa):
    sd = np.sqrt(np.abs(np.asarray(ref["var"])).astype(np.float64))
    return gu.worst_ratio(cov, np.asarray(ref["cov"]), bound(n, kappa) * sd[:, None] * sd[None, :])
