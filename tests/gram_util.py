"""numpy restatement of what the Gram and q kernels of the fit loop compute, and of the packed-tile layout they write -- the
reference of tests/test_gpu_gram.py, checked on the CPU by tests/test_gram_util.py.  Imports neither the package under test nor
the oracle: it is written from the comments of GramL2 (csrc/common.hpp) and from qphb.py:53-120 / 465-466 of the reference.

    P_b = (W_b A_b)' (W_b A_b) + L2_b          L2_b = sum_k S_bk^1/2 (M_k o scale_bk) S_bk^1/2     (orders with dfac_k > 0)
    q_b = -(W_b A_b)' (W_b y_b) + l1

scale_bk is dfac_k * rho_bk where both indices are DRT coefficients (>= ns), dop_dfac_k * dop_rho_bk where both lie in the x_dop
block [dop_start, dop_start + dop_size) (a part of the special block [0, ns)), and 1 elsewhere.

Packed tiles (csrc/qp_resident.hpp, csrc/gram.hip): P as 16 x 16 tiles on an nchp x nchp grid, nchp = round_up(n, 32) / 16, tile
(tr, tc) at doubles [(tr * nchp + tc) * 256, +256); only tiles with tc <= tr exist.  Inside a tile, double2 slot h*64 + i*4 + q
holds columns q + 8h and q + 8h + 4 of row i (h in 0..1, i in 0..15, q in 0..3).
"""
import numpy as np

U = 2.0 ** -53          # unit roundoff of binary64


def gamma(k):
    """Higham's gamma_k = k u / (1 - k u)"""
    return k * U / (1.0 - k * U)


def nchp_of(n):
    return (n + 31) // 32 * 2


def _tile_index():
    """(256,) arrays: row and column inside a tile of each of its 256 doubles"""
    d = np.arange(256)
    slot, e = d // 2, d % 2
    h, i, q = slot // 64, (slot % 64) // 4, slot % 4
    return i, q + 8 * h + 4 * e


_TI, _TJ = _tile_index()


def pack_tiles(P, n, fill=np.nan):
    """row-major P [n][>= n] -> packed buffer [nchp^2 * 256]: every tile tc <= tr holds P's own entries (upper parts of diagonal
    tiles included: P[i][j], not the mirror), 0.0 beyond n; the slots of tiles tc > tr hold `fill`"""
    P = np.asarray(P)
    nc = nchp_of(n)
    full = np.zeros((nc * 16, nc * 16), dtype=P.dtype)
    full[:n, :n] = P[:n, :n]
    out = np.full(nc * nc * 256, fill, dtype=P.dtype)
    for tr in range(nc):
        for tc in range(tr + 1):
            out[(tr * nc + tc) * 256:(tr * nc + tc + 1) * 256] = full[tr * 16 + _TI, tc * 16 + _TJ]
    return out


def unpack_tiles(ppk, n, fill=np.nan):
    """packed buffer -> (nchp * 16)^2 matrix: tiles tc <= tr from the buffer, everything above them `fill`"""
    ppk = np.asarray(ppk)
    nc = nchp_of(n)
    assert ppk.shape == (nc * nc * 256,), ppk.shape
    full = np.full((nc * 16, nc * 16), fill, dtype=ppk.dtype)
    for tr in range(nc):
        for tc in range(tr + 1):
            full[tr * 16 + _TI, tc * 16 + _TJ] = ppk[(tr * nc + tc) * 256:(tr * nc + tc + 1) * 256]
    return full


def lower_tile_mask(n):
    """bool [nchp^2 * 256]: the doubles of the packed buffer that belong to a tile tc <= tr"""
    nc = nchp_of(n)
    t = np.arange(nc * nc)
    return np.repeat((t % nc) <= (t // nc), 256)


def mirror_lower(P):
    """[..., n, n] -> the symmetric matrix of its lower triangle (what the row-major copy holds)"""
    lo = np.tril(P)
    return lo + np.swapaxes(np.tril(P, -1), -1, -2)


def l2_matrix(mk, s, rho, dfac, ns, dop=None, dop_rho=None, dop_dfac=None, dtype=np.float64, absolute=False):
    """L2 of ONE spectrum, [n][n] (not symmetrised: entry (i, j) uses M_k[i][j]).  mk: three [n][>= n] matrices, s [3][n],
    rho [3] or None (= 1), dop = (start, size) or None.  absolute=True: sum of the absolute values of the terms."""
    n = s.shape[-1]
    out = np.zeros((n, n), dtype=dtype)
    for k in range(3):
        if not dfac[k] > 0.0:
            continue
        m = np.array(np.asarray(mk[k])[:n, :n], dtype=dtype)
        m[ns:, ns:] *= dtype(dfac[k]) * (dtype(1) if rho is None else dtype(rho[k]))
        if dop is not None and dop[1] > 0:
            a, b = dop[0], dop[0] + dop[1]
            m[a:b, a:b] *= dtype(dop_dfac[k]) * (dtype(1) if rho is None else dtype(dop_rho[k]))
        sq = np.sqrt(np.asarray(s[k], dtype=dtype))
        term = (sq[:, None] * m) * sq[None, :]
        out += np.abs(term) if absolute else term
    return out


def reference_pq(A, w, y=None, n=None, l1=None, l1_scalar=0.0, l2=None, mk=None, s=None, rho=None, dfac=(0.0, 0.0, 0.0), ns=0,
                 dop=None, dop_rho=None, dop_dfac=(0.0, 0.0, 0.0), dtype=np.float64, absolute=False):
    """(P [B][n][n], q [B][n] or None) in `dtype` arithmetic.  A [m][lda] or [B][m][lda] (columns >= n are padding), w, y [B][m].
    P is not symmetrised where the penalty matrices are not (see l2_matrix).  absolute=True gives the magnitudes the error bounds
    are made of: |WA|'|WA| + sum |L2 terms| and |WA|'|Wy| + |l1|."""
    A, w = np.asarray(A), np.asarray(w)
    B, m = w.shape
    n = A.shape[-1] if n is None else n
    P = np.zeros((B, n, n), dtype=dtype)
    q = None if y is None else np.zeros((B, n), dtype=dtype)
    for b in range(B):
        Ab = np.array((A[b] if A.ndim == 3 else A)[:, :n], dtype=dtype)
        wa = np.asarray(w[b], dtype=dtype)[:, None] * Ab
        if absolute:
            wa = np.abs(wa)
        P[b] = wa.T @ wa
        if s is not None:
            P[b] += l2_matrix(mk, np.asarray(s[b]), None if rho is None else rho[b], dfac, ns, dop,
                              None if dop_rho is None else dop_rho[b], dop_dfac, dtype, absolute)
        elif l2 is not None:
            lb = np.asarray(l2[b] if np.ndim(l2) == 3 else l2)[:n, :n].astype(dtype)
            P[b] += np.abs(lb) if absolute else lb
        if y is not None:
            wy = np.asarray(w[b], dtype=dtype) * np.asarray(y[b], dtype=dtype)
            lin = np.full(n, l1_scalar, dtype=dtype) if l1 is None else np.asarray(l1, dtype=dtype)
            q[b] = (wa.T @ np.abs(wy) + np.abs(lin)) if absolute else (-(wa.T @ wy) + lin)
    return P, q


def extended_dtype():
    """np.longdouble where it carries a 64-bit significand (x87), else None: the caller then uses reference_pq_exact"""
    return np.longdouble if np.finfo(np.longdouble).nmant >= 63 else None


def reference_pq_exact(A, w, y, n, **kw):
    """reference_pq for platforms without an extended type: the Gram part and q summed in exact rational arithmetic and rounded
    once; the L2 part in float64 (three terms of five roundings each: well inside its 8u share of the bound)."""
    from fractions import Fraction
    A, w = np.asarray(A, dtype=np.float64), np.asarray(w, dtype=np.float64)
    B, m = w.shape
    P, q = reference_pq(A, w, y, n, **kw)
    Pl2, _ = reference_pq(np.zeros_like(A), w, None, n, **{k: v for k, v in kw.items() if k not in ("l1", "l1_scalar")})
    for b in range(B):
        Ab = (A[b] if A.ndim == 3 else A)[:, :n]
        wa = [[Fraction(float(w[b, k])) * Fraction(float(Ab[k, i])) for i in range(n)] for k in range(m)]
        for i in range(n):
            for j in range(i + 1):
                v = sum(wa[k][i] * wa[k][j] for k in range(m))
                P[b, i, j] = float(v + Fraction(float(Pl2[b, i, j])))
                P[b, j, i] = float(v + Fraction(float(Pl2[b, j, i])))
        if y is not None:
            wy = [Fraction(float(w[b, k])) * Fraction(float(np.asarray(y)[b, k])) for k in range(m)]
            lin = np.full(n, kw.get("l1_scalar", 0.0)) if kw.get("l1") is None else np.asarray(kw["l1"], dtype=float)
            for i in range(n):
                q[b, i] = float(-sum(wa[k][i] * wy[k] for k in range(m)) + Fraction(float(lin[i])))
    return P, q


def error_bounds(A, w, y, n, m, **kw):
    """element-wise bounds (P, q) on |computed - exact| for any float64 evaluation that rounds w*A, sums m products in any order
    with or without fused multiply-adds, forms each L2 term with at most five roundings (two square roots, three products), adds
    three of them and adds the result to the sum:  gamma_(m+8) (|WA|'|WA|) + 8u |L2|,  gamma_(m+8) (|WA|'|Wy|) + 8u |l1|"""
    kw = dict(kw)
    lin = np.full(n, kw.pop("l1_scalar", 0.0)) if kw.get("l1") is None else np.asarray(kw["l1"], dtype=float)
    kw.pop("l1", None)
    # (the magnitudes themselves in float64: their own rounding, a relative gamma_m, is covered by the factor below)
    gram_abs, lin_abs = reference_pq(A, w, y, n, absolute=True)
    both_abs, _ = reference_pq(A, w, None, n, absolute=True, **kw)
    l2_abs = np.maximum(both_abs - gram_abs, 0.0) * (1.0 + 1e-9)
    gram_abs, lin_abs = gram_abs * (1.0 + 1e-9), None if y is None else lin_abs * (1.0 + 1e-9)
    g = gamma(m + 8)
    bp = g * gram_abs + 8 * U * l2_abs
    bq = None if y is None else g * lin_abs + 8 * U * np.abs(lin)[None, :]
    return bp, bq


def toeplitz_penalty(n, ns, first_rows, special=None, ld=None):
    """three [n][ld] penalty matrices whose DRT block (>= ns) is symmetric Toeplitz with the given first rows (each of length
    <= n - ns, zero beyond); `special` (optional, three [n][n] arrays) supplies every entry with an index below ns"""
    ld = n if ld is None else ld
    nd = n - ns
    d = np.abs(np.arange(nd)[:, None] - np.arange(nd)[None, :])
    out = []
    for k in range(3):
        t = np.zeros(max(nd, 1))
        t[:len(first_rows[k])] = first_rows[k]
        m = np.zeros((n, ld))
        if special is not None:
            m[:n, :n] = special[k]
        m[ns:n, ns:n] = t[d] if nd else 0.0
        out.append(m)
    return out


def golden71_case(golden_dir):
    """the float test's small case: response matrix, weights, data vector, penalty matrices, s vectors and rho of the reference's
    own 71 x 91 run (refrun_golden71x91.npz; n = 93 with two special parameters, m = 142), with the product's dfac =
    l2_lambda_0 * derivative_weights and the special diagonals of the padded penalty matrices (1e-6)"""
    import os
    g = np.load(os.path.join(golden_dir, "refrun_golden71x91.npz"), allow_pickle=False)
    n, ns = g["rm"].shape[1], g["rm"].shape[1] - g["m0"].shape[0]
    mk = []
    for k in range(3):
        m = np.zeros((n, n))
        m[np.arange(ns), np.arange(ns)] = 1e-6
        m[ns:, ns:] = g[f"m{k}"]
        mk.append(m)
    return dict(A=np.array(g["rm"]), w=np.array(g["weights"])[None], y=np.array(g["rv"])[None], mk=mk, s=np.array(g["s_vectors"])[None],
                rho=np.array(g["rho_vector"])[None], dfac=tuple(142.0 * np.array([1.5, 1.0, 0.5])), ns=ns)


def worst_ratio(actual, exact, bound):
    """max |actual - exact| / bound over the elements (0 / 0 counts as 0: an element with a zero bound must be exact)"""
    err = np.abs(np.asarray(actual, dtype=np.longdouble) - np.asarray(exact, dtype=np.longdouble)).astype(np.float64)
    if np.any((bound == 0) & (err != 0)):
        return np.inf
    return float(np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)))
