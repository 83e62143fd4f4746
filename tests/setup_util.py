"""numpy restatement of what runs before the fit loop and after it (csrc/hyper.hip: prep_kernel, prep_prepared_kernel,
init_weights_kernel, row_mask_kernel, weight_method_kernel, llh_kernel and the element-wise kernels) -- the reference of
tests/test_gpu_setup.py, checked on the CPU by tests/test_setup_util.py.  Imports neither the package under test nor the oracle: it is
written from drt1d.py:439-514, 542-566, 612, 648-672, 748-760, 4436-4496, 5825-5896 and qphb.py:521-557, 1347-1377, 1471-1479,
1545-1594, 1644-1648 of the reference.  estimate_weights, with its bound and its `near` set, is hyper_util._weights.

    prep(c, dtype)                  scaling, the variance floor and the constant state
    init_weights(c, dtype, ...)     stages 0..3 of initialize_weights
    weight_rule(c, dtype, ...)      hybrid_weight_factor_method='weight'
    llh(c, dtype, mode, ...)        rss and sum(log w) in the four weight modes
    the element-wise operations     plain float64: every one of them is exact or a correctly rounded product

With the extended type of gram_util.extended_dtype() a function gives the reference value (EXACT: once-rounded exact sums where the
platform has none), with float64 a plain restatement (the one the mutants of test_setup_util.py are made from).  want_bounds=True
adds 'bound': for every floating-point output a first-order bound on |float64 evaluation - exact| in ANY summation order, with or
without fused multiply-adds (a fusion only removes a rounding), times 2 for the second-order terms; and 'exclude'.

The bounds (u = 2^-53, gamma_k = k u / (1 - k u); sqrt and division correctly rounded: u; log: 2 ulp = 4u relative)

  cs, rv      (max - min) / rp_scale and z / cs are single correctly rounded operations on exact inputs: bit for bit.
  var_floor   mean = sum(v) / m: dmean = gamma_(m+1) sum|v| / m;  d_i = v_i - mean: dd_i = dmean + u |d_i|;  s2 = sum d_i^2:
              ds2 = sum (2 |d_i| dd_i + u d_i^2) + gamma_m s2;  floor = (s2 / m) 1e-7: (ds2 / m + 2u s2 / m) 1e-7.
  est_w       hyper_util._weights (estimate_weights without the blend).  Stage 2 takes its floor from the block's own data: where
              s_hat lies under the floor (or within d(s_hat) + d(floor) of it) w = floor^-1/2 moves by w d(floor) / 2 floor on top.
  init w      q = 1 / w^2: rel 2 dw / w + 2u;  bq = 1/2 - alpha + 1: dbq = u |1/2 - alpha| + u |bq|;  D = bq^2 + 2 beta q:
              dD = 2 |bq| dbq + u bq^2 + |2 beta q| (rel q + 2u) + u |D|;  R = sqrt(D): dD / 2R + u R;  N = R - bq: dN = dbq + dR + u |N|
              (bq > 0: N cancels, and the local roundings of R and bq dominate);  sh = N / 2 beta: dN / |2 beta| + 2u |sh|;
              w = sh^-1/2: w (dsh / 2 sh + 2u).  iw_alpha <= 0: a copy, the bound of est_w.
  weight rule sc = sum 1 / w_i^2 over a block of k rows: relative gamma_(k+2);  cws = (sc / k)^-1/2: e_c = gamma_(k+2) / 2 + 3u, ews
              alike;  ratio = sqrt(sqrt(ews / cws)): (e_c + e_e + u) / 4 + 3u / 2;  1 / ratio: u more.  An override is exact.
  llh         y = rm x: dy = gamma_n |rm| |x|.  Weights: mode 0 as est_w with the caller's floor; mode 1 and 3 exact; mode 2 the mean
              of k entries, relative gamma_k + u (the tests choose dyadic est_w, whose sums are exact: bit for bit).  The kernel
              forms rss = A - 2C + D from A = sum (w y)^2, C = sum (w rv)(w y), D = sum (w rv)^2, which nearly cancel for a good fit:
                  drss = gamma_(m+6) (A + 2 |C| + D)                                   (|C| = sum |w rv| |w y|)
                         + sum 2 |w y| (|y| dw + w dy)  +  2 sum [ |w rv| (|y| dw + w dy) + |w y| |rv| dw ]  +  sum 2 |w rv| |rv| dw
              the reference value itself is the residual form sum (w (y - rv))^2.
              sum log w: sum dw_i / w_i + (4u + gamma_m) sum |log w_i|.
The outlier rule sb > |r| is a jump: entries within their bound of it (`near`), and every row whose variance estimate reads such an
entry, are left out of a value comparison; exclusion_share() is capped at 2 % by tests/test_setup_util.py.
"""
import math
from fractions import Fraction

import numpy as np

from gram_util import U, gamma
from hyper_util import EXACT, POISON, _Arith, _weights, reference_dtype      # noqa: F401  (re-exported for the tests)

F = np.float64
ONE = 1.0 + 1e-9
OPTS = dict(rp_scale=14.0, scale_data=1, s_0=(1.0, 2.0, 0.5), rho_0=(1.5, 1.0, 0.25), outlier_p=0.0, iw_alpha=0.0, iw_beta=1.0,
            inductance_scale=1e-5)
DOP_RHO_0 = (3.0, 0.5, 7.0)


# ---- variance floor ---------------------------------------------------------------------------------------------------------------
def var_floor(A, v, ddof=0, want_bound=False):
    """np.var(v) * 1e-7 in A's arithmetic -> value [, bound]"""
    v64 = np.asarray(v, dtype=F)
    m = v64.size
    if not np.all(np.isfinite(v64)):
        return (np.nan, np.nan) if want_bound else np.nan
    if A.exact:
        fr = [Fraction(float(t)) for t in v64]
        mean = sum(fr) / m
        var = float(sum((t - mean) ** 2 for t in fr) / max(m - ddof, 1)) * 1e-7 if m > ddof else np.nan
    else:
        t = A.t
        va = A.a(v64)
        mean = va.sum() / t(m)
        d = va - mean
        var = (d * d).sum() / t(m - ddof) * t(1e-7) if m > ddof else t(np.nan)
    if not want_bound:
        return var
    mean64 = v64.mean()
    d = np.abs(v64 - mean64)
    dmean = gamma(m + 1) * np.abs(v64).sum() / m
    dd = dmean + U * d
    s2 = (d * d).sum()
    ds2 = (2 * d * dd + U * d * d).sum() + gamma(m) * s2
    return var, 2.0 * (ds2 / m + 2 * U * s2 / m) * 1e-7 * ONE


# ---- prep ---------------------------------------------------------------------------------------------------------------------------
def make_prep_case(seed, nf, n, scale_data, prepared=False, m=None):
    """B = 3 members: member 0 has the maximum of Re z in the last entry and the minimum in the first, member 1 the other way round,
    member 2 somewhere inside; the imaginary parts are larger than the real ones, so a range taken over them as well changes cs"""
    rng = np.random.default_rng(seed)
    B = 3
    o = dict(OPTS, scale_data=scale_data)
    if prepared:
        rv = rng.standard_normal((B, m)) * rng.uniform(0.5, 3.0, (B, 1)) + rng.uniform(-2, 2, (B, 1))
        return dict(B=B, nf=0, m=m, n=n, prepared=True, rv=rv, opts=o, dop_rho_0=DOP_RHO_0)
    zr = rng.uniform(2.0, 3.0, (B, nf))
    zr[0, 0], zr[0, nf - 1] = 1.0, 4.0
    zr[1, 0], zr[1, nf - 1] = 4.5, 0.5
    if nf == 1:
        zr[:, 0] = (1.0, 4.5, 2.5)
    zi = -rng.uniform(10.0, 50.0, (B, nf))
    return dict(B=B, nf=nf, m=2 * nf, n=n, prepared=False, z_re=zr, z_im=zi, opts=o)


def prep(c, dtype=F, mutant=None, want_bounds=False):
    A = _Arith(dtype)
    B, m, n, o = c["B"], c["m"], c["n"], c["opts"]
    out = dict(w=np.ones((B, m)), s=np.empty((B, 3, n)), x=np.full((B, n), 1e-6), x_in=np.full((B, n), 1e-6),
               rho=np.tile(np.asarray(o["rho_0"], dtype=F), (B, 1)), xmx=np.ones((B, 3)), active=np.ones(B, dtype=np.int32),
               outer_iters=np.zeros(B, dtype=np.int32), fit_status=np.ones(B, dtype=np.int32), qp_iters_total=np.zeros(B, dtype=np.int32))
    for k in range(3):
        out["s"][:, k, :] = o["s_0"][k]
    if c["prepared"]:
        out["coef_scale"] = np.ones(B)
        out["rv"] = np.array(c["rv"], dtype=F)
        out["dop_rho"] = np.tile(np.asarray(c["dop_rho_0"], dtype=F), (B, 1))
        out["dop_xmx"] = np.ones((B, 3))
    else:
        zr, zi = np.asarray(c["z_re"], dtype=F), np.asarray(c["z_im"], dtype=F)
        src = np.concatenate([zr, zi], axis=1) if mutant == "range_all" else zr
        cs = (src.max(axis=1) - src.min(axis=1)) / F(o["rp_scale"]) if o["scale_data"] else np.ones(B)
        out["coef_scale"] = cs
        with np.errstate(all="ignore"):
            out["rv"] = np.concatenate([zr, zi], axis=1) / cs[:, None]
    vf = [var_floor(A, out["rv"][b], ddof=1 if mutant == "ddof1" else 0, want_bound=True) for b in range(B)]
    out["var_floor"] = np.array([v[0] for v in vf], dtype=A.t)
    if want_bounds:
        out["bound"] = dict(var_floor=np.array([v[1] for v in vf], dtype=F))
    return out


PREP_EXACT = ("coef_scale", "rv", "w", "s", "x", "x_in", "rho", "xmx", "dop_rho", "dop_xmx", "active", "outer_iters", "fit_status",
              "qp_iters_total")


# ---- fit cases: response matrix, variance matrix, x, data with chosen residuals -------------------------------------------------------
INIT_SHAPES = ((2, 2, 2), (33, 5, 5), (64, 16, 16), (142, 93, 94), (513, 129, 130), (1030, 514, 514))


def banded_vmm(rng, m, width=2.0):
    v = np.abs(rng.standard_normal((m, m))) * np.exp(-0.5 * ((np.arange(m)[:, None] - np.arange(m)[None, :]) / width) ** 2)
    return v / v.sum(axis=1, keepdims=True)


def exclude_self(vmm, mutant=None):
    """qphb.py:1644-1648: no point reads its own residual, rows renormalised"""
    d = np.diagonal(vmm)
    out = vmm / (1.0 - (d[None, :] if mutant == "dj" else d[:, None]))
    out[np.diag_indices_from(out)] = 0.0
    return out


def make_fit_case(seed, m, n, ldrm, rm_batched=False, outlier_p=0.0, resid=1e-3, floor_starts=None, huge=None, nc=None, B=3,
                  qp_fail=(1,)):
    """B members; qp_fail: members whose QP broke down.  floor_starts: first rows of runs of nine residuals of 1e-6, far under the
    variance floor (default: one run from row 2, a second from nc + 2 with nc); huge: rows of the LAST member whose residual of 1e11
    drives the weight under 1e-10 (default the last two; they raise that member's floor over every other row).  Both only where m >= 33.  nc: the variance matrix is block diagonal, split at nc."""
    rng = np.random.default_rng(seed)
    rm = np.full(((B,) if rm_batched else ()) + (m, ldrm), 977.0)
    rm[..., :n] = rng.standard_normal(rm[..., :n].shape) / np.sqrt(n)
    x = rng.uniform(0.2, 2.0, (B, n))
    vmm = banded_vmm(rng, m)
    big = m >= 33
    if floor_starts is None and outlier_p > 0:         # (the same underflow next to a run of tiny residuals)
        floor_starts = []
    if floor_starts is None:
        floor_starts = ([2] + ([nc + 2] if nc is not None and nc + 12 <= m else [])) if big else []
        if nc is not None and nc < 12:
            floor_starts = [nc + 2] if big else []
    if huge is None:           # (not with the outlier rule: next to 1e11 an outlier_t underflows to 0, and its sqrt has no bound)
        huge = [m - 2, m - 1] if big and not outlier_p > 0 else []
    noutl = (3 if big else 0) if outlier_p > 0 else 0
    oidx = 14 + 8 * np.arange(noutl)
    for i in oidx:          # an outlier's own residual has little part in its variance estimate
        off = vmm[i].sum() - vmm[i, i]
        vmm[i] *= 0.98 / off
        vmm[i, i] = 0.02
    vmm_cross = vmm.copy()
    if nc is not None:
        vmm[:nc, nc:] = 0.0
        vmm[nc:, :nc] = 0.0
    rv = np.empty((B, m))
    for b in range(B):
        r = resid * rng.standard_normal(m) * rng.uniform(0.5, 1.5, m)
        if outlier_p > 0:       # rows that estimate each other's variance: residuals of one size, so that no outlier_t
            r = resid * rng.uniform(0.7, 1.3, m) * rng.choice([-1.0, 1.0], m)      # underflows to 0, where its sqrt has no bound
        for s0 in floor_starts:
            r[s0:s0 + 9] = 1e-6 * rng.standard_normal(len(r[s0:s0 + 9]))
        r[oidx] = 4.0 * resid * rng.choice([-1.0, 1.0], noutl)
        if b == B - 1:
            r[huge] = 1e11
        rv[b] = (rm[b] if rm_batched else rm)[:, :n] @ x[b] - r
    qs = np.zeros(B, dtype=np.int32)
    qs[[q for q in qp_fail if q < B]] = -1
    est_w = (1.0 / resid) * 10.0 ** rng.uniform(-2, 2, (B, m))
    return dict(seed=seed, B=B, m=m, n=n, rm=rm, x=x, rv=rv, vmm=vmm, vmm_cross=vmm_cross,
                vmm_iw=exclude_self(vmm) if outlier_p > 0 else vmm, var_floor=np.array([np.var(rv[b]) * 1e-7 for b in range(B)]),
                est_w=est_w, qp_status=qs, opts=dict(OPTS, outlier_p=outlier_p), nc=nc, resid=resid)


def _rmb(c, b):
    return np.asarray(c["rm"][b] if c["rm"].ndim == 3 else c["rm"])[:, :c["n"]]


# ---- initial weights ----------------------------------------------------------------------------------------------------------------
_EST = {}


def _estimate(c, dtype, want_bounds):
    """stages 0 and 1 share this: estimate_weights(x, est_w=None) on vmm_iw for every member whose QP held -> per member dict or None"""
    key = (id(c), str(dtype), want_bounds)
    if key not in _EST:
        A = _Arith(dtype)
        _EST[key] = (c, [None if c["qp_status"][b] < 0 else
                         _weights(A, c, b, c["x"][b], c["vmm_iw"], None, c["var_floor"][b], None, want_bounds) for b in range(c["B"])])
    return _EST[key][1]


def weight_scale(A, w, alpha, beta, mutant=None, dw=None):
    """solve_init_weight_scale -> w [, bound]"""
    t = A.t
    w = A.a(w)
    if not alpha > 0.0:
        return (w, dw) if dw is not None else w
    bq = (t(0.5) + t(alpha) + t(1)) if mutant == "b_plus" else (t(0.5) - t(alpha) + t(1))
    q = t(1) / (w * w)
    D = bq * bq + t(2) * t(beta) * q
    R = np.sqrt(D)
    N = -bq + R
    sh = N / (t(2) * t(beta))
    out = t(1) / np.sqrt(sh)
    if dw is None:
        return out
    wf, qf, Df, Rf, Nf, shf, of = (np.asarray(v, dtype=F) for v in (w, q, D, R, N, sh, out))
    bqf = float(bq)
    relq = 2 * dw / wf + 2 * U
    dbq = U * abs(0.5 - alpha) + U * abs(bqf)
    dD = 2 * abs(bqf) * dbq + U * bqf * bqf + np.abs(2 * beta * qf) * (relq + 2 * U) + U * np.abs(Df)
    dR = dD / (2 * Rf) + U * Rf
    dN = dbq + dR + U * np.abs(Nf)
    dsh = dN / abs(2 * beta) + 2 * U * np.abs(shf)
    return out, 2.0 * of * (dsh / (2 * shf) + 2 * U) * ONE


def _weights64(c, b, V, vf, mutant=None, perm=None, fma=False):
    """estimate_weights without outliers and without the blend in plain float64 -- the summation order `perm` (a permutation of the
    columns of both products, None: numpy's own) and, fma=True, every product fused into its addition"""
    rm, x, rv = _rmb(c, b), c["x"][b], c["rv"][b]

    def mv(M, v):
        if perm is None and not fma:
            return M @ v
        p = np.arange(M.shape[1]) if perm is None else perm(M.shape[1])
        s = np.zeros(M.shape[0])
        for j in p:
            s = (np.asarray(M[:, j], dtype=np.longdouble) * np.longdouble(v[j]) + s).astype(F) if fma else s + M[:, j] * v[j]
        return s
    r = mv(rm, x) - rv
    sh = mv(V, r * r)
    if mutant == "floor_after":
        w = np.maximum(1.0 / np.sqrt(sh), vf)
    else:
        w = 1.0 / np.sqrt(np.where(sh < vf, vf, sh))
    return w if mutant == "no_clip" else np.maximum(w, 1e-10)


def init_weights(c, stage, r0=0, r1=0, iw_alpha=0.0, iw_beta=1.0, dtype=F, mutant=None, want_bounds=False, before=None):
    """est_w, w, x, outlier_t, active, fit_status after launch_init_weights(stage, r0, r1).  before: dict of the arrays as they stand
    before the launch (default: poison; est_w of stage 3: c['est_w']).  A float64 mutant evaluation takes the plain path."""
    A = _Arith(dtype)
    t = A.t
    B, m, n = c["B"], c["m"], c["n"]
    before = before or {}
    o = {k: np.array(before.get(k, np.full(shape, POISON)), dtype=t) for k, shape in
         (("est_w", (B, m)), ("w", (B, m)), ("x", (B, n)), ("outlier_t", (B, m)))}
    if "x" not in before:
        o["x"] = np.array(c["x"], dtype=t)
    if stage == 3 and "est_w" not in before:
        o["est_w"] = np.array(c["est_w"], dtype=t)
    o["active"] = np.array(before.get("active", np.ones(B)), dtype=np.int32)
    o["fit_status"] = np.array(before.get("fit_status", np.full(B, -77)), dtype=np.int32)
    bd = {k: np.zeros((B, m)) for k in ("est_w", "w", "outlier_t")}
    bd["x"] = np.zeros((B, n))
    excl = {k: np.zeros((B, m), dtype=bool) for k in ("est_w", "w", "outlier_t")}
    op = c["opts"]["outlier_p"]
    est = _estimate(c, dtype, want_bounds) if stage in (0, 1) and mutant is None else None
    for b in range(B):
        if c["qp_status"][b] < 0:
            o["active"][b], o["fit_status"][b] = 0, -1
            continue
        if stage == 2:
            sl = slice(r0, r1)
            blk = c["rv"][b, sl]
            vf, dvf = var_floor(A, c["rv"][b] if mutant == "floor_whole" else blk, ddof=1 if mutant == "ddof1" else 0, want_bound=True)
            if mutant == "full_v":
                o["est_w"][b, sl] = _weights64(c, b, c["vmm_cross"], float(vf))[sl]
            elif mutant in ("floor_after", "no_clip"):
                sub = dict(c, m=r1 - r0, rm=_rmb(c, b)[sl][None], rv=c["rv"][b:b + 1, sl], x=c["x"][b][None])
                o["est_w"][b, sl] = _weights64(sub, 0, c["vmm_iw"][sl, sl], float(vf), mutant)
            else:
                sub = dict(c, m=r1 - r0, rm=_rmb(c, b)[sl], rv=c["rv"][:, sl], opts=dict(c["opts"], outlier_p=0.0))
                r = _weights(A, sub, b, c["x"][b], c["vmm_iw"][sl, sl], None, vf, None, want_bounds)
                o["est_w"][b, sl] = r["w"]
                if want_bounds:
                    wf = np.asarray(r["w"], dtype=F)
                    # (a floored entry has w = floor^-1/2 exactly in the reference: that is how they are recognised)
                    w_fl = 1.0 / math.sqrt(float(vf)) if float(vf) > 0 else np.inf
                    floored = np.abs(wf - w_fl) <= 1e-6 * w_fl
                    bd["est_w"][b, sl] = r["dw"] + np.where(floored, wf * dvf / (2 * float(vf)) * ONE, 0.0) if float(vf) > 0 else r["dw"]
            continue
        if stage in (0, 1):
            if mutant in ("floor_after", "no_clip", "ddof1"):
                vf = var_floor(A, c["rv"][b], ddof=1) if mutant == "ddof1" else c["var_floor"][b]
                o["est_w"][b] = _weights64(c, b, c["vmm_iw"], float(vf), mutant)
            else:
                r = est[b] if est is not None else _weights(A, c, b, c["x"][b], c["vmm_iw"], None, c["var_floor"][b], None, want_bounds)
                o["est_w"][b] = r["w"]
                if op > 0.0:
                    o["outlier_t"][b] = r["t"]
                if want_bounds:
                    near = r["near"]
                    reads = near | ((np.abs(c["vmm_iw"]) @ near.astype(F)) > 0)
                    bd["est_w"][b], excl["est_w"][b] = r["dw"], reads
                    if op > 0.0:
                        bd["outlier_t"][b], excl["outlier_t"][b] = r["dt"], near
        if stage == 0:
            continue
        res = weight_scale(A, o["est_w"][b], iw_alpha, iw_beta, mutant, dw=bd["est_w"][b] if want_bounds else None)
        if want_bounds:
            o["w"][b], bd["w"][b] = res
            excl["w"][b] = excl["est_w"][b]
        else:
            o["w"][b] = res
        o["x"][b] = 1e-6
    if want_bounds:
        o["bound"], o["exclude"] = bd, excl
    return o


INIT_FLOAT = ("est_w", "w", "x", "outlier_t")
INIT_INT = ("active", "fit_status")


def ratios(got, ref, keys):
    """worst |got - ref| / bound per key (excluded entries left out; a zero bound asks for equality, poison included)"""
    out = {}
    for key in keys:
        g, r = np.asarray(got[key]), ref[key]
        bnd = np.asarray(ref["bound"].get(key, np.zeros(np.shape(r))), dtype=F)
        with np.errstate(invalid="ignore"):
            err = np.abs(np.asarray(g, dtype=np.longdouble) - np.asarray(r, dtype=np.longdouble)).astype(F)
        same_nan = np.isnan(np.asarray(g, dtype=F)) & np.isnan(np.asarray(r, dtype=F))
        err = np.where(same_nan, 0.0, np.where(np.isnan(err), np.inf, err))
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), np.inf))
        ex = ref.get("exclude", {}).get(key)
        if ex is not None:
            q = np.where(ex, 0.0, q)
        out[key] = float(np.max(q)) if np.size(q) else 0.0
    return out


def exclusion_share(ref):
    ex = ref.get("exclude", {})
    return max([float(np.mean(v)) for v in ex.values() if np.size(v)] or [0.0])


# ---- the weight rule ------------------------------------------------------------------------------------------------------------------
def make_rule_case(seed, m, nc, B=3):
    rng = np.random.default_rng(seed)
    ew = 10.0 ** rng.uniform(-10, 6, (B, m))
    ew[:, :nc] *= 10.0 ** rng.uniform(-2, 2, (B, 1))          # the two blocks on different scales
    return dict(seed=seed, B=B, m=m, nc=nc, est_w=ew)


def weight_rule(c, fixed_chrono=0.0, fixed_eis=0.0, dtype=F, mutant=None, want_bounds=False):
    A = _Arith(dtype)
    t = A.t
    B, m, nc = c["B"], c["m"], c["nc"]
    wrow, wfac = np.empty((B, m), dtype=t), np.empty((B, 2), dtype=t)
    bw = np.zeros((B, 2))
    for b in range(B):
        ew = A.a(c["est_w"][b])
        if mutant == "mean_w":
            cws, ews = A.total(ew[:nc]) / t(nc), A.total(ew[nc:]) / t(m - nc)
        else:
            inv = t(1) / (ew * ew)
            cws = t(1) / np.sqrt(t(A.total(inv[:nc])) / t(nc))
            ews = t(1) / np.sqrt(t(A.total(inv[nc:])) / t(m - nc))
        ratio = np.sqrt(ews / cws) if mutant == "half" else np.sqrt(np.sqrt(ews / cws))
        cf, ef = (t(1) / ratio, ratio) if mutant == "swap" else (ratio, t(1) / ratio)
        rel = (gamma(nc + 2) / 2 + 3 * U + gamma(m - nc + 2) / 2 + 3 * U + U) / 4 + 1.5 * U
        bw[b] = 2.0 * float(cf) * rel * ONE, 2.0 * float(ef) * (rel + U) * ONE
        if fixed_chrono > 0.0:
            cf, bw[b, 0] = t(fixed_chrono), 0.0
        if fixed_eis > 0.0:
            ef, bw[b, 1] = t(fixed_eis), 0.0
        wrow[b, :nc], wrow[b, nc:], wfac[b] = cf, ef, (cf, ef)
    out = dict(wrow=wrow, wfac=wfac)
    if want_bounds:
        brow = np.empty((B, m))
        brow[:, :nc], brow[:, nc:] = bw[:, :1], bw[:, 1:]
        out["bound"] = dict(wrow=brow, wfac=bw)
    return out


# ---- rss and sum log w ----------------------------------------------------------------------------------------------------------------
def dyadic_weights(rng, shape):
    """weights k / 1024 with k < 2^20: every partial sum of a few thousand of them is exact, so their mean is one correctly rounded
    division in any summation order"""
    return rng.integers(1, 1 << 20, shape).astype(F) / 1024.0


def make_llh_case(seed, m, n, ldrm, rm_batched, resid, nc=None):
    """resid 1e-3: a good fit, the three sums of the kernel cancel; resid 1: residuals of the data's own size.  No rows at 1e11 here
    (a weight of 1e-10 on a residual of 1e11 is not what the sums are about) -- the floor rows stay."""
    c = make_fit_case(seed, m, n, ldrm, rm_batched, resid=resid, huge=[], qp_fail=())
    rng = np.random.default_rng(seed + 7)
    c["est_w"] = dyadic_weights(rng, (c["B"], m))
    c["nc"] = nc if nc is not None else 0
    c["scalar_w"] = 0.8125
    return c


def llh(c, mode, nc=0, dtype=F, mutant=None, want_bounds=False, weights=None):
    """rss [B], slw [B], w [B][m] (the weights the sums were formed with).  weights: use these instead of forming them (the
    float64 checks of the sums alone)."""
    A = _Arith(dtype)
    t = A.t
    B, m, n = c["B"], c["m"], c["n"]
    rss, slw, W = np.empty(B, dtype=t), np.empty(B, dtype=t), np.empty((B, m), dtype=t)
    brss, bslw, bw = np.zeros(B), np.zeros(B), np.zeros((B, m))
    split = m // 2 if mutant == "split_half" else nc
    for b in range(B):
        rm, x = _rmb(c, b), c["x"][b]
        y = A.a(A.matvec(rm, np.asarray(x, dtype=F)))
        rv = A.a(c["rv"][b])
        dw = np.zeros(m)
        if weights is not None:
            w = A.a(weights[b])
        elif mode == 0:
            r = _weights(A, dict(c, opts=dict(c["opts"], outlier_p=0.0)), b, x, c["vmm"], None, c["var_floor"][b], None, want_bounds)
            w = r["w"]
            if want_bounds:
                dw = r["dw"]
        elif mode == 1:
            w = A.a(c["est_w"][b])
        elif mode == 2:
            # np.mean of float64 weights is a float64: the exact sum, rounded, over the count.  Where the exact sum IS a float64
            # (dyadic_weights) that is one correctly rounded division in any order, else gamma_k + u relative
            ew = np.asarray(c["est_w"][b], dtype=F)
            w = np.zeros(m, dtype=t)
            for sl in (slice(0, split), slice(split, m)):
                k = len(ew[sl])
                if k:
                    tot = math.fsum(ew[sl])
                    w[sl] = t(F(tot) / F(k))
                    if sum(Fraction(float(v)) for v in ew[sl]) != Fraction(tot):
                        dw[sl] = (gamma(k) + U) * abs(tot / k)
        else:
            w = np.full(m, t(c["scalar_w"]))
        W[b] = w
        wy, wr = w * y, w * rv
        res = w * (y - rv)
        if mutant == "plus2c":
            rss[b] = A.total(wy * wy) + t(2) * A.total(wr * wy) + A.total(wr * wr)
        elif A.exact:
            rss[b] = A.dot(np.asarray(res, dtype=F), np.asarray(res, dtype=F))
        else:
            rss[b] = (res * res).sum()
        lw = np.log(w * w) if mutant == "logw2" else np.log(w)
        slw[b] = A.total(lw)
        if want_bounds:
            yf, rvf, wf, wyf, wrf = (np.abs(np.asarray(v, dtype=F)) for v in (y, rv, w, wy, wr))
            dy = gamma(n) * (np.abs(rm) @ np.abs(np.asarray(x, dtype=F))) * ONE
            dwy = yf * dw + wf * dy
            brss[b] = 2.0 * ONE * (gamma(m + 6) * ((wyf * wyf).sum() + 2 * (wrf * wyf).sum() + (wrf * wrf).sum())
                                   + (2 * wyf * dwy).sum() + 2 * (wrf * dwy + wyf * rvf * dw).sum() + (2 * wrf * rvf * dw).sum())
            lf = np.abs(np.asarray(lw, dtype=F))
            bslw[b] = 2.0 * ONE * ((dw / wf).sum() + (4 * U + gamma(m)) * lf.sum())
            bw[b] = dw
    out = dict(rss=rss, slw=slw, w=W)
    if want_bounds:
        out["bound"] = dict(rss=brss, slw=bslw, w=bw)
    return out


def three_sums(c, W, perm=None, fma=False):
    """the kernel's form in plain float64: A - 2C + D, and sum log w, with the weights W as given"""
    B, m = c["B"], c["m"]
    rss, slw = np.empty(B), np.empty(B)
    for b in range(B):
        y = _rmb(c, b) @ c["x"][b]
        w, rv = np.asarray(W[b], dtype=F), c["rv"][b]
        p = np.arange(m) if perm is None else perm(m)
        wy, wr = (w * y)[p], (w * rv)[p]
        if fma:
            a = c2 = d = np.longdouble(0)
            for i in range(m):
                a = F(np.longdouble(wy[i]) * wy[i] + a)
                c2 = F(np.longdouble(wr[i]) * wy[i] + c2)
                d = F(np.longdouble(wr[i]) * wr[i] + d)
            rss[b] = F(np.longdouble(-2.0) * c2 + a) + d
        else:
            rss[b] = (wy * wy).sum() - 2.0 * (wr * wy).sum() + (wr * wr).sum()
        slw[b] = np.log(w)[p].sum()
    return rss, slw


# ---- the element-wise operations (plain float64) --------------------------------------------------------------------------------------
def assemble_rm(a_re, a_im, freq, n, ns, ld, idx_rinf, idx_induc, inductance_scale, before, mutant=None):
    nf = len(freq)
    out = np.array(before, dtype=F).reshape(2 * nf, ld)
    out[:, :n] = 0.0
    out[:nf, ns:n], out[nf:, ns:n] = a_re, a_im
    if idx_rinf >= 0:
        out[:nf, idx_rinf] = 1.0
    if idx_induc >= 0:
        col = 2.0 * 3.141592653589793 * np.asarray(freq, dtype=F)
        out[nf:, idx_induc] = col if mutant == "no_lscale" else col * inductance_scale
    return out


def special_penalty(mats, idx_rinf, idx_induc, pen_r, pen_l):
    out = [np.array(v, dtype=F) for v in mats]
    for v in out:
        if idx_rinf >= 0:
            v[idx_rinf, idx_rinf] = pen_r
        if idx_induc >= 0:
            v[idx_induc, idx_induc] = pen_l
    return out


def make_h(n, ns, nonneg):
    return np.where(np.arange(n) < ns, 0.0, 0.0 if nonneg else 1e5)


def row_mask(B, m, r0, r1):
    i = np.arange(m)
    return np.tile(((i >= r0) & (i < r1)).astype(F), (B, 1))


def scale_rows(w, rows, factor, active, before):
    """(w * factor) * rows, in this order; members that are not active keep what `before` holds"""
    v = np.asarray(w, dtype=F) * F(factor)
    if rows is not None:
        v = v * np.asarray(rows, dtype=F)
    out = np.array(before, dtype=F)
    on = np.ones(len(v), dtype=bool) if active is None else np.asarray(active) != 0
    out[on] = v[on]
    return out


def copy_column(rm, B, col):
    rm = np.asarray(rm)
    return np.array([(rm[b] if rm.ndim == 3 else rm)[:, col] for b in range(B)])


# ---- the case tables ------------------------------------------------------------------------------------------------------------------
PREP_NF = (1, 2, 63, 64, 65, 511, 512, 513, 1030)
PREP_N = (2, 93)
RULE_M = (2, 130, 1030)
RULE_NC = (1, 63, 64, 65, 512)
STAGE2_NC = (1, 31, 64)
LLH_RESID = (1e-3, 1.0)
ROWOP_M = (1, 255, 256, 257, 1030)
ROWOP_N = (1, 257)


def rule_ncs(m):
    return sorted({nc for nc in RULE_NC + (m - 1,) if 0 < nc < m})


def stage2_ncs(m):
    return sorted({nc for nc in STAGE2_NC + (m - 1,) if 0 < nc < m})


def llh_nc(m):
    return max(1, min(31, m - 1))


_CASES = {}


def cached(kind, *key):
    """a case, made once per process: kind 'prep' (nf, n, scale_data) | 'prepared' (m, n) | 'init' (shape index, batched, outlier_p)
    | 'stage2' (shape index, nc) | 'rule' (m, nc) | 'llh' (shape index, batched, resid)"""
    k = (kind,) + key
    if k not in _CASES:
        seed = 4000 + sum((i + 1) * int(1000 * float(v)) for i, v in enumerate(key)) % 100000
        if kind == "prep":
            _CASES[k] = make_prep_case(seed, key[0], key[1], key[2])
        elif kind == "prepared":
            _CASES[k] = make_prep_case(seed, 0, key[1], 0, prepared=True, m=key[0])
        elif kind == "init":
            m, n, ld = INIT_SHAPES[key[0]]
            _CASES[k] = make_fit_case(seed, m, n, ld, rm_batched=bool(key[1]), outlier_p=key[2])
        elif kind == "stage2":
            m, n, ld = INIT_SHAPES[key[0]]
            _CASES[k] = make_fit_case(seed, m, n, ld, rm_batched=bool(key[0] % 2), nc=key[1])
        elif kind == "rule":
            _CASES[k] = make_rule_case(seed, key[0], key[1])
        elif kind == "llh":
            m, n, ld = INIT_SHAPES[key[0]]
            _CASES[k] = make_llh_case(seed, m, n, ld, bool(key[1]), key[2], nc=llh_nc(m))
        else:
            raise KeyError(kind)
    return _CASES[k]


_REFS = {}


def reference(fn, c, *args, **kw):
    """fn(c, *args, dtype=reference_dtype(), want_bounds=True, **kw), computed once per process"""
    k = (fn.__name__, id(c), args, tuple(sorted(kw.items())))
    if k not in _REFS:
        _REFS[k] = (c, fn(c, *args, dtype=reference_dtype(), want_bounds=True, **kw))
    return _REFS[k][1]
