"""Cases, extended-precision reference, exact statements and error bound of the posterior variance / covariance chain -- the
reference of tests/test_gpu_posterior.py, checked on the CPU by tests/test_posterior_util.py.  Imports neither the package under
test nor the oracle; written from the comments of csrc/qp_resident.hpp (factor(), cov_kernel_resident) and csrc/gram.hip
(pack_rows_kernel, rows_outer_kernel).

    var_bi  = s_b * r_i' P_b^-1 r_i          cov_b = s_b * R P_b^-1 R'
    r_i = row i of `rows`, placed at the unknowns col_offset .. col_offset + ncol - 1 and zero elsewhere

Reference: float64 Cholesky (scipy.linalg.cho_factor / cho_solve), then iterative refinement of X = P^-1 R' with the residual
R' - P X and the iterate X in gram_util.extended_dtype() (64-bit significand): O(n^2) extended operations per row, so it serves
n = 4096 with a handful of rows.  The correction of such a refinement cannot fall below ~ kappa_2(P) 2^-64 |X|: the rounding of the
residual (and of X itself) is a perturbation of relative size 2^-64 of P X, and P^-1 magnifies its part along the small
eigenvectors by kappa.  "Converged" is therefore: the last correction is at most 2^-60 kappa_2(P) of the solution (column-wise,
maximum norm) -- an error of the reference of 2^-7 u kappa var, less than a hundredth of the unit of the bound below at every n.
A case that does not get there is refused (RuntimeError).

Bound: |var - exact| <= C_BOUND (n + 16) u kappa_2(P) var, u = 2^-53 -- the forward-error scale of a quadratic form through any
backward-stable Cholesky factor (the explicitly inverted diagonal blocks stay inside it: kappa(L_jj)^2 <= kappa_2(P)); for cov_ij
the same unit with sqrt(var_i var_j).  The constant cannot be derived and is not taken from the kernel: it is 8 times the worst
ratio that `restate` -- a float64 numpy restatement of the kernel's algorithm -- shows against the reference over the whole case
table, rounded up to a power of two (tests/test_posterior_util.py recomputes it).
"""
import functools

import numpy as np

import gram_util as gu

U = gu.U

# 8 x (worst ratio of the float64 restatement over the case table), rounded up to a power of two.  Measured on the CPU:
# restatement 0.0516, plain LAPACK route (cho_solve) 0.0516, both at case a_n1_k1e+01_e16, where kappa = 1 and the unit is smallest
# (0.88 u of error against 17 u); full matrix: restatement 0.0166 (i_n17_eye), LAPACK 0.0168 (i_n17_e40).  8 x 0.0516 = 0.413.
# tests/test_posterior_util.py measures again and asserts C_BOUND / 2 < 8 x worst <= C_BOUND.
C_BOUND = 2.0 ** -1


def unit(n, kappa):
    return (n + 16) * U * kappa


# ---- packed tiles ---------------------------------------------------------------------------------------------------------------
def pack_rows(rows, n, col_offset):
    """the exact packed image of `rows`: [nex][nchp][256]"""
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    neval, ncol = rows.shape
    nex, nc = (neval + 15) // 16, gu.nchp_of(n)
    full = np.zeros((nex * 16, nc * 16))
    full[:neval, col_offset:col_offset + ncol] = rows
    out = np.empty((nex, nc, 256))
    for tr in range(nex):
        for tc in range(nc):
            out[tr, tc] = full[tr * 16 + gu._TI, tc * 16 + gu._TJ]
    return out


def unpack_rows(tiles):
    """[..., nex][nchp][256] -> [..., nex * 16][nchp * 16]"""
    tiles = np.asarray(tiles)
    nex, nc = tiles.shape[-3], tiles.shape[-2]
    full = np.empty(tiles.shape[:-3] + (nex * 16, nc * 16))
    for tr in range(nex):
        for tc in range(nc):
            full[..., (tr * 16 + gu._TI), (tc * 16 + gu._TJ)] = tiles[..., tr, tc, :]
    return full


def full_rows(rows, n, col_offset, shift=0):
    rows = np.atleast_2d(np.asarray(rows, dtype=np.float64))
    out = np.zeros((rows.shape[0], n))
    a = col_offset + shift
    lo, hi = max(a, 0), min(a + rows.shape[1], n)
    out[:, lo:hi] = rows[:, lo - a:hi - a]
    return out


# ---- case builder ---------------------------------------------------------------------------------------------------------------
def spd_matrix(n, kappa, seed):
    """(P = Q diag(lambda) Q', kappa_2): Q from the QR of a seeded Gaussian matrix, lambda log-spaced over [1, kappa]"""
    rng = np.random.default_rng(seed)
    q, _ = np.linalg.qr(rng.standard_normal((n, n)))
    lam = np.logspace(0.0, np.log10(kappa), n) if n > 1 else np.ones(1)
    p = (q * lam) @ q.T
    return gu.mirror_lower(p), float(lam[-1] / lam[0])


def fit_like_matrix(n, seed, ns=2):
    """(A'A + a Toeplitz penalty on the DRT block, kappa_2 by Lanczos on P and on its inverse)"""
    from scipy.linalg import cho_factor, cho_solve
    from scipy.sparse.linalg import LinearOperator, eigsh
    rng = np.random.default_rng(seed)
    m = min(2 * n, 142)
    ns = min(ns, n - 1)
    t = np.linspace(-4.0, 4.0, n - ns)
    f = np.linspace(-5.0, 5.0, m)
    a = np.empty((m, n))
    a[:, :ns] = 1.0 + 0.1 * rng.standard_normal((m, ns))
    a[:, ns:] = np.exp(-0.5 * (f[:, None] - t[None, :]) ** 2) * (1.0 + 0.01 * rng.standard_normal((m, n - ns)))
    special = [np.diag(np.r_[np.full(ns, 1e-3), np.zeros(n - ns)])] * 3
    mk = gu.toeplitz_penalty(n, ns, [[1.0], [2.0, -1.0], [6.0, -4.0, 1.0]], special)
    p = a.T @ a + 1e-2 * mk[0] + 0.3 * mk[1] + 1.0 * mk[2]
    p = gu.mirror_lower(p)
    if n <= 600:
        ev = np.linalg.eigvalsh(p)
        return p, float(ev[-1] / ev[0])
    c = cho_factor(p, lower=True)
    top = eigsh(LinearOperator((n, n), matvec=lambda v: p @ v, dtype=np.float64), k=1, which="LA", tol=1e-4,
                return_eigenvectors=False)[0]
    inv = eigsh(LinearOperator((n, n), matvec=lambda v: cho_solve(c, v, check_finite=False), dtype=np.float64), k=1, which="LA",
                tol=1e-4, return_eigenvectors=False)[0]
    return p, float(top * inv)


def make_rows(kind, neval, ncol, seed):
    """dense Gaussian rows; from four rows on, row 1 has a single non-zero and row 2 is zero ("mixed"); "identity": the
    parameter-covariance route"""
    if kind == "identity":
        return np.eye(ncol)
    rng = np.random.default_rng(seed + 77)
    r = rng.standard_normal((neval, ncol))
    if neval >= 4:
        r[1] = 0.0
        r[1, (seed * 7 + 3) % ncol] = 1.5
        r[2] = 0.0
    return r


def _spec(n, kappa, neval, off=None, ncol=None, rows="mixed", seed=0):
    off = min(2, n - 1) if off is None else off
    return dict(n=n, kappa=kappa, neval=neval, off=off, ncol=n - off if ncol is None else ncol, rows=rows, seed=seed)


@functools.lru_cache(maxsize=None)
def case_table():
    """name -> (group, spec).  Groups as the sections of tests/test_gpu_posterior.py: a sizes, b the LDS / global U switch, c large,
    d pass boundaries of the row wavefronts, e column offsets, i the full matrix."""
    t = {}
    for n in (1, 15, 16, 17, 31, 32, 33, 48, 49, 64, 65, 96, 97, 129, 161):
        for kappa in ((1e1, 1e6, 1e10) if n <= 129 else (1e6,)):
            for neval in (1, 16, 17, 40):
                t[f"a_n{n}_k{kappa:.0e}_e{neval}"] = ("a", _spec(n, kappa, neval, seed=n + neval))
    for n in (497, 512, 513, 528, 529, 545, 700):
        t[f"b_n{n}"] = ("b", _spec(n, 1e6, 40, seed=n))
    for n in (2049, 4096):
        t[f"c_n{n}"] = ("c", _spec(n, "fit", 17, seed=n))
    for n in (33, 161):
        for neval in (24 * 16, 24 * 16 + 1, 48 * 16, 48 * 16 + 1):
            t[f"d_n{n}_e{neval}"] = ("d", _spec(n, 1e6, neval, seed=n + neval))
    for off in (0, 1, 2, 17):
        t[f"e_off{off}_full"] = ("e", _spec(70, 1e1, 17, off=off, seed=off))
        t[f"e_off{off}_part"] = ("e", _spec(70, 1e1, 17, off=off, ncol=70 - off - 19, seed=off + 50))
    for n, kappa in ((17, 1e1), (93, "fit"), (514, 1e6)):
        for neval in (1, 17, 40):
            t[f"i_n{n}_e{neval}"] = ("i", _spec(n, kappa, neval, seed=n + neval))
        if n <= 93:
            t[f"i_n{n}_eye"] = ("i", _spec(n, kappa, n, off=0, rows="identity", seed=n))
    return t


def build_case(spec):
    n = spec["n"]
    if spec["kappa"] == "fit":
        p, kappa = fit_like_matrix(n, spec["seed"])
    else:
        p, kappa = spd_matrix(n, spec["kappa"], spec["seed"])
    rows = make_rows(spec["rows"], spec["neval"], spec["ncol"], spec["seed"])
    return dict(n=n, P=p, kappa=kappa, rows=rows, off=spec["off"], neval=rows.shape[0], ncol=rows.shape[1])


@functools.lru_cache(maxsize=None)
def get_case(name, want_cov=False):
    """(case, reference) of a table entry; built once and shared: treat both as read-only"""
    c = build_case(case_table()[name][1])
    ref = reference(c["P"], full_rows(c["rows"], c["n"], c["off"]), c["kappa"], want_cov)
    for v in list(c.values()) + list(ref.values()):
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c, ref


# ---- reference ------------------------------------------------------------------------------------------------------------------
def reference(P, R, kappa, want_cov=False, max_iter=12):
    """dict(var [neval], cov [neval][neval] or None, corrections: the relative size of every refinement step's correction, iters).
    P [n][n] (the lower triangle counts), R [neval][n] full rows.  Raises RuntimeError when the refinement does not converge."""
    from scipy.linalg import cho_factor, cho_solve
    ext = gu.extended_dtype()
    if ext is None:
        raise RuntimeError("no extended type on this platform")
    P = gu.mirror_lower(np.asarray(P, dtype=np.float64))
    R = np.atleast_2d(np.asarray(R, dtype=np.float64))
    c = cho_factor(P, lower=True)
    pe, be = P.astype(ext), R.T.astype(ext)
    live = np.any(R != 0.0, axis=1)                    # a zero row has the exact answer zero
    xe = cho_solve(c, R.T).astype(ext)
    tol = 2.0 ** -60 * max(kappa, 1.0)
    hist, ok = [], False
    for _ in range(max_iter):
        d = cho_solve(c, (be - pe @ xe).astype(np.float64))
        xe = xe + d.astype(ext)
        rel = np.max(np.abs(d), axis=0)[live] / np.max(np.abs(xe), axis=0)[live].astype(np.float64) if live.any() else np.zeros(1)
        hist.append(float(np.max(rel)))
        if hist[-1] <= tol:
            ok = True
            break
    if not ok:
        raise RuntimeError(f"refinement did not converge: corrections {hist}, wanted {tol:.3g}")
    var = np.sum(be * xe, axis=0)
    return dict(var=var, cov=(be.T @ xe) if want_cov else None, corrections=hist, iters=len(hist), tol=tol)


def lapack_route(P, R, want_cov=False):
    """float64: cho_factor / cho_solve and a dot product"""
    from scipy.linalg import cho_factor, cho_solve
    P = gu.mirror_lower(np.asarray(P, dtype=np.float64))
    x = cho_solve(cho_factor(P, lower=True), R.T)
    return dict(var=np.sum(R.T * x, axis=0), cov=(R @ x) if want_cov else None)


# ---- float64 restatement of the kernel's algorithm --------------------------------------------------------------------------------
MUTANTS = ("panel_tile", "appended_tile_row", "second_half_sum", "col_offset", "upper_triangle")


def restate(P, rows, col_offset, mutant=None, want_cov=False):
    """The chain in float64 numpy as the kernel orders it: P padded by the identity to a multiple of 32, blocked by 32; every diagonal
    block factored and explicitly inverted; panel rows and the appended rows formed by multiplication with that inverse; var = the
    sum of squares of an appended row, cov = Y Y'.  `mutant`: one of MUTANTS, the defects the bound has to see."""
    from scipy.linalg import solve_triangular
    P = np.asarray(P, dtype=np.float64)
    n = P.shape[0]
    NP = (n + 31) // 32 * 32
    A = np.eye(NP)
    A[:n, :n] = gu.mirror_lower(P.T if mutant == "upper_triangle" else P)
    C = np.zeros((np.atleast_2d(rows).shape[0], NP))
    C[:, :n] = full_rows(rows, n, col_offset, shift=1 if mutant == "col_offset" else 0)
    L, Y = np.zeros((NP, NP)), np.zeros_like(C)
    nblk = NP // 32
    hit = nblk // 2                                     # the block column a mutant strikes
    for jb in range(nblk):
        j0, j1 = jb * 32, jb * 32 + 32
        Lr = L[j0:j1, :j0]
        D = A[j0:j1, j0:j1] - Lr @ Lr.T
        Ljj = np.linalg.cholesky(D)
        W = solve_triangular(Ljj, np.eye(32), lower=True)
        L[j0:j1, j0:j1] = Ljj
        if j1 < NP:
            L[j1:, j0:j1] = (A[j1:, j0:j1] - L[j1:, :j0] @ Lr.T) @ W.T
            if mutant == "panel_tile" and jb == min(hit, nblk - 2):
                L[j1:j1 + 16, j0:j0 + 16] = 0.0
        Y[:, j0:j1] = (C[:, j0:j1] - Y[:, :j0] @ Lr.T) @ W.T
        if mutant == "appended_tile_row" and jb == hit:
            Y[:16, j0:j1] = 0.0
    S = Y.copy()
    if mutant == "second_half_sum":
        S[:, hit * 32 + 16:hit * 32 + 32] = 0.0
    return dict(var=np.sum(S * S, axis=1), cov=(S @ S.T) if want_cov else None, Y=Y)


# ---- comparison -----------------------------------------------------------------------------------------------------------------
def var_ratio(var, ref, n, kappa, scale=1.0):
    """worst |var - exact| / ((n + 16) u kappa exact) over the rows (in units of the bound WITHOUT its constant); exact = scale * the
    reference's variance.  A zero row must give zero exactly."""
    exact = np.asarray(ref["var"]) * scale
    return gu.worst_ratio(var, exact, unit(n, kappa) * np.abs(exact).astype(np.float64))


def cov_ratio(cov, ref, n, kappa, scale=1.0):
    sd = np.sqrt(np.abs(np.asarray(ref["var"]) * scale).astype(np.float64))
    return gu.worst_ratio(cov, np.asarray(ref["cov"]) * scale, unit(n, kappa) * sd[:, None] * sd[None, :])
