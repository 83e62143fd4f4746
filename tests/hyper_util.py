"""numpy restatement of one hyper-parameter step of the fit loop (csrc/hyper.hip: hyper_kernel with its three product forms) -- the
reference of tests/test_gpu_hyper.py, checked on the CPU by tests/test_hyper_util.py.  Imports neither the package under test nor
the oracle: it is written from qphb.py:320-405 (solve_s, solve_rho), 597-603 (is_converged), 1497-1594 (solve_outlier_t,
outlier_tvt, estimate_weights) and drt1d.py:903-979 (update_scale, the xmx norms, the vz_offset column) of the reference.

    step(c, dtype)    every output of the step for the case `c` (a dict, see make_case) in `dtype` arithmetic; with the
                      extended type of gram_util.extended_dtype() this is the reference value, with float64 a plain
                      restatement (the one the mutants of test_hyper_util.py are made from)
    step(c, ext, want_bounds=True)
                      adds, for every floating-point output, a first-order bound on |float64 evaluation - exact| in ANY summation
                      order, times 2 for the second-order terms ('bound'), and the entries that lie within their bound of a switch
                      point ('exclude')

The bounds (u = 2^-53, gamma_k = k u / (1 - k u); sqrt and division correctly rounded: u; exp: 2 ulp = 4u relative -- ROCm's
own documentation on the build host gives no other figure for the f64 exp of the device library)

  solve_s    gu_ij = (r x_i M_ij x_j + xh_i M1_ij xh_j / (2 sigma^2)) sqrt(s_j), j != i, xh = sign(x) sqrt|x|.  One term takes at
             most 11 roundings in either kernel form (sqrt s, x sqrt s, r x_i, two products; sqrt|x| twice, 2 sigma^2, the
             division, three products) and one addition; the row sum adds nd - 1 of them:
                 db_i = gamma_(nd + 12) sum_j |gu_ij|            dg_i = gamma_12 (|r x_i^2 M_ii| + |xh_i^2 M1_ii / 2 sigma^2| + |beta|)
             u = N / 2g, N = -b + sgn(b) R, R = sqrt(D), D = b^2 + 4 g (alpha - 1).  By the partial derivatives
                 dR = (|b| db + 2 |alpha - 1| dg) / R  +  (u b^2 + 3u |4 g (alpha - 1)| + u |D|) / 2R + u R
                 dN = db + dR + u |N|                            (b > 0: N = R - b cancels, |N| << R, and the LOCAL roundings of R,
                                                                  about 2u b, dominate dN / |N| -- the term the bound exists for)
                 du = dN / |2g| + |N| dg / 2 g^2 + 2u |u|        ds = 2 |u| du + u s
             gmax <= 1e-10:  s = (alpha - 1) / g,  ds = |s| (dg / |g| + 2u).  The replacements NaN -> 1 and <= 0 -> 1e-15 are exact.
  solve_rho  v = sqrt(s) x with the NEW s: dv_i = |x_i| (ds_i / 2 sqrt(s_i) + u sqrt(s_i)) + u |v_i|;  q = v' M v:
                 dq = sum_i dv_i (|M| |v|)_i + sum_j (|v|' |M|)_j dv_j + gamma_(2 nd + 2) |v|' |M| |v|
             rho = a / (q / xmx + a / r0): d(den) = dq / |xmx| + u |q / xmx| + u |a / r0| + u |den|, drho = |rho| (d(den) / |den| + u).
  xmx        x' M x: gamma_(2 nd + 2) |x|' |M| |x|.
  weights    y = rm x: dy = gamma_n |rm| |x|;  r = y - rv: dr = dy + u |r|;  r2 = r^2: 2 |r| dr + u r2;
             sh = V r2: |V| d(r2) + gamma_m |V| r2.  max(sh, var_floor) is continuous: the error passes or vanishes.
             w = 1 / sqrt(sh): w (d(sh) / 2 sh + 2u);  the est_w blend fc = w / (w + e), fe = 1 - fc, fc w + fe e by its partial
             derivatives with one u per operation;  max(., 1e-10) is continuous.
  outliers   sb = sqrt(V r2), pdf(r; scale) = exp(-r^2 / 2 scale^2) / (scale sqrt(2 pi)): relative error of pdf_in
             d(sb) / sb + d(arg) + 4u + 5u with d(arg) = arg (2 dr / |r| + 2 d(sb) / sb + 4u), of pdf_out dr / |r| + 4u 0.5 + 4u + 5u;
             t = 1 - A / (A + C) with A = p pdf_out, C = (1 - p) pdf_in: dt = g (1 - g) (rel A + rel C + 3u) + 3u g + u |t|, g = A / (A + C).
             t = 1 where sb > |r|: a discontinuity (t jumps from 1 - p), entries with | sb - |r| | <= d(sb) + dr are left out.
             s_hat = sqrt(t) V (sqrt(t) r2) + (1 - t) r2 by its partial derivatives as above.
  vz column  (rm x0 [+ vz_entry x_vz]) strength, sign by row: gamma_(n + 3) of the absolute sums.
  scale      rp = area sum |x|: gamma_(nd + 1);  sf = sqrt(rp_scale / rp): e = gamma_(nd + 1) / 2 + 2u relative; everything scaled
             by sf, 1 / sf: e + u on top of its own error;  xmx sqrt(sf): e / 2 + 2u;  var_floor sf^2: 2 e + 2u.
The convergence rule compares max |dx / (x_in + 1e-15)| with xtol and max |dx| with 1e-3 mean(x_in): the cases keep both at
least 1e-6 relative from their thresholds (margins(), asserted by tests/test_hyper_util.py), `gmax` a factor 1e3 from 1e-10.
"""
import math

import numpy as np

from gram_util import U, extended_dtype, gamma, toeplitz_penalty

POISON = -3.0e33           # state a step must not read (and what it must leave where it does not write)
EXACT = "exact"            # dtype for platforms without an extended type: sums of exact products, rounded once (math.fsum)

DEFAULT_OPTS = dict(rp_scale=14.0, derivative_weights=(1.5, 1.0, 0.5), sigma_ds=(1.0, 1000.0, 1000.0), s_alpha=(5.0, 10.0, 25.0),
                    s_0=(1.0, 1.0, 1.0), rho_alpha=(0.15, 0.2, 0.25), rho_0=(1.0, 1.0, 1.0), xtol=1e-2, max_iter=50, scale_data=1,
                    update_scale=0, eff_hp=1, outlier_p=0.0)


def reference_dtype():
    e = extended_dtype()
    return EXACT if e is None else e


# ---- sums in the chosen arithmetic ----------------------------------------------------------------------------------------------
def _split(a):
    c = 134217729.0 * a           # Veltkamp: 2^27 + 1
    hi = c - (c - a)
    return hi, a - hi


def _two_prod(a, b):
    """a * b = p + e exactly (Dekker), float64 arrays of one shape"""
    p = a * b
    ah, al = _split(a)
    bh, bl = _split(b)
    return p, ((ah * bh - p) + ah * bl + al * bh) + al * bl


class _Arith:
    def __init__(self, dtype):
        self.exact = isinstance(dtype, str)
        self.t = np.float64 if self.exact else dtype

    def a(self, v):
        return np.asarray(v, dtype=self.t)

    def rowsum(self, mat):
        """sum over the last axis of a matrix of already formed terms"""
        if self.exact:
            return np.array([math.fsum(r) for r in np.atleast_2d(mat)]).reshape(np.shape(mat)[:-1])
        return mat.sum(axis=-1)

    def matvec(self, M, v):
        if self.exact:
            out = np.empty(M.shape[0])
            for i in range(M.shape[0]):
                p, e = _two_prod(M[i], v)
                out[i] = math.fsum(np.concatenate([p, e]))
            return out
        v = self.a(v)
        if M.dtype == self.t or M.size <= 1 << 20:
            return self.a(M) @ v
        return np.concatenate([self.a(M[i:i + 256]) @ v for i in range(0, M.shape[0], 256)])      # (memory: no extended copy of M)

    def dot(self, a, b):
        return self.matvec(np.atleast_2d(np.asarray(a)), b)[0]

    def total(self, v):
        return math.fsum(v) if self.exact else self.a(v).sum()


# ---- the reach window of the two-rows-per-thread Toeplitz convolution (csrc/hyper.hip) ---------------------------------------------
def window_mask(nd, reach, mutant=None):
    """bool [nd][nd]: the columns the kernel visits for each row -- for the row pair (2p, 2p + 1) the columns [2p - reach,
    2p + 1 + reach] widened to multiples of four and clipped to [0, nd).  reach < 0: all.  Mutants: 'lastcol' drops the last
    column of every window, 'noalign' rounds the upper end DOWN to a multiple of four (aligned, but not widened)."""
    if reach < 0:
        return np.ones((nd, nd), dtype=bool)
    ia = (np.arange(nd) // 2) * 2
    lo = np.where(ia - reach > 0, (ia - reach) & ~3, 0)
    hi = (ia + 2 + reach) & ~3 if mutant == "noalign" else (ia + 2 + reach + 3) & ~3
    hi = np.minimum(hi, nd)
    if mutant == "lastcol":
        hi = hi - 1
    j = np.arange(nd)[None, :]
    return (j >= lo[:, None]) & (j < hi[:, None])


def true_reach(mk, ns, nd):
    r = 0
    for k in range(3):
        nz = np.nonzero(np.asarray(mk[k])[ns, ns:ns + nd])[0]
        if nz.size:
            r = max(r, int(nz.max()))
    return r


# ---- one step ---------------------------------------------------------------------------------------------------------------------
def _opt(c, key):
    return c["opts"].get(key, DEFAULT_OPTS[key])


def _sign(v):
    return np.sign(v)


def _update_block(A, c, k, xd, M, M1, use_g, alpha, s0, sigma, ra, r0, xmx_k, reff, s_old, mask, mutant, want_bounds):
    """solve_s + solve_rho of one order on one block.  Returns dict(s, rho, gmax[, ds, drho, near_gmax])"""
    t = A.t
    nd = xd.size
    xd_, so = A.a(xd), A.a(s_old)
    xh = _sign(xd_) * np.sqrt(np.abs(xd_))
    a1 = t(alpha) - t(1)
    beta = a1 / t(s0)
    sig2 = t(2) * t(sigma) * t(sigma)
    Mt = A.a(M)
    eye = np.eye(nd, dtype=bool)

    def solve(sq):
        t1 = ((t(reff) * xd_)[:, None] * Mt) * xd_[None, :]
        t2 = ((xh[:, None] * A.a(M1)) * xh[None, :]) / sig2 if use_g else np.zeros((nd, nd), dtype=t)
        gam = t1 + t2
        gd = np.diagonal(gam) + beta
        gu = gam * sq[None, :]
        keep = ~eye if mutant != "lag0" else np.ones((nd, nd), dtype=bool)
        if mask is not None:
            keep = keep & mask
        gu = np.where(keep, gu, t(0))
        gmax = float(np.max(np.abs(np.where(~eye, gu, t(0))))) if nd > 1 else 0.0
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            if gmax > 1e-10:
                b = A.a(A.rowsum(gu))
                D = b * b + t(4) * gd * a1
                R = np.sqrt(D)
                N = -b + _sign(b) * R
                uh = N / (t(2) * gd)
                sh = uh * uh
            else:
                b = D = R = N = uh = None
                sh = a1 / gd
        nan = np.isnan(sh)
        sh = np.where(nan, t(1), sh)
        low = sh <= 0
        sh = np.where(low, t(1e-15), sh)
        return dict(s=sh, gmax=gmax, b=b, R=R, N=N, uh=uh, gd=gd, t1=t1, t2=t2, fixed=nan | low, D=D, beta=beta, a1=a1, sq=sq)

    r = solve(np.sqrt(so))
    if mutant == "sqrt_new_s":
        r = solve(np.sqrt(r["s"]))
    sh = r["s"]
    v = np.sqrt(sh) * xd_
    Mv = Mt if mask is None else np.where(mask, Mt, t(0))
    mv = A.matvec(np.asarray(Mv, dtype=np.float64) if A.exact else Mv, np.asarray(v, dtype=np.float64) if A.exact else v)
    q = A.dot(v, mv)
    rb = t(ra) / t(r0)
    den = t(q) / t(xmx_k) + rb
    rho = t(ra) / den
    out = dict(s=sh, rho=rho, gmax=r["gmax"])
    if want_bounds:
        f = np.float64
        one = 1.0 + 1e-9
        sq = np.asarray(r["sq"], dtype=f)
        absgu = (np.abs(np.asarray(r["t1"], dtype=f)) + np.abs(np.asarray(r["t2"], dtype=f))) * sq[None, :]
        absgu[eye] = 0.0
        db = gamma(nd + 12) * absgu.sum(axis=1) * one
        dgv = gamma(12) * (np.abs(np.diagonal(np.asarray(r["t1"], dtype=f))) + np.abs(np.diagonal(np.asarray(r["t2"], dtype=f)))
                           + abs(float(r["beta"]))) * one
        gd = np.asarray(r["gd"], dtype=f)
        a1f = abs(float(r["a1"]))
        with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
            if r["gmax"] > 1e-10:
                b, R, N, uh = (np.asarray(r[key], dtype=f) for key in ("b", "R", "N", "uh"))
                D = np.asarray(r["D"], dtype=f)
                dR = (np.abs(b) * db + 2 * a1f * dgv) / R + (U * b * b + 3 * U * np.abs(4 * gd * a1f) + U * np.abs(D)) / (2 * R) + U * R
                dN = db + dR + U * np.abs(N)
                du = dN / np.abs(2 * gd) + np.abs(N) * dgv / (2 * gd * gd) + 2 * U * np.abs(uh)
                ds = 2 * np.abs(uh) * du + U * np.asarray(sh, dtype=f)
            else:
                ds = np.abs(np.asarray(sh, dtype=f)) * (dgv / np.abs(gd) + 2 * U)
        ds = np.where(r["fixed"], 0.0, ds)
        shf, vf, xf = np.asarray(sh, dtype=f), np.abs(np.asarray(v, dtype=f)), np.abs(np.asarray(xd, dtype=f))
        dv = xf * (ds / (2 * np.sqrt(shf)) + U * np.sqrt(shf)) + U * vf
        absM = np.abs(np.asarray(M, dtype=f))
        Mabsv = absM @ vf
        dq = (dv @ Mabsv + (vf @ absM) @ dv + gamma(2 * nd + 2) * (vf @ Mabsv)) * one
        qx = float(q) / float(xmx_k)
        dden = dq / abs(float(xmx_k)) + U * abs(qx) + U * abs(float(rb)) + U * abs(float(den))
        out["ds"] = 2.0 * ds
        out["drho"] = 2.0 * abs(float(rho)) * (dden / abs(float(den)) + U)
    return out


def _weights(A, c, b, x, V, est_w, var_floor, mutant, want_bounds):
    """estimate_weights for spectrum b -> dict(w, t or None[, dw, dt, near])"""
    t = A.t
    f = np.float64
    m, n = c["m"], c["n"]
    rm = np.asarray(c["rm"][b] if c["rm"].ndim == 3 else c["rm"])[:, :n]
    rv = A.a(c["rv"][b])
    y = A.a(A.matvec(rm, np.asarray(x, dtype=f)))
    r = y - rv
    if mutant == "resid_sign":
        r = rv - y
    r2 = r * r
    op = float(_opt(c, "outlier_p"))
    ex = (lambda a_: np.asarray(a_, dtype=f)) if A.exact else (lambda a_: a_)
    sh0 = A.a(A.matvec(ex(V) if A.exact else A.a(V), ex(r2)))
    out = {}
    tt = None
    if op > 0.0:
        s2pi = np.sqrt(t(2) * t(3.141592653589793))
        ar = np.abs(r) if mutant != "resid_sign" else r
        sb = np.sqrt(sh0)
        with np.errstate(all="ignore"):
            pdf_in = t(1) / (sb * s2pi) * np.exp(t(-0.5) * (r * r) / (sb * sb))
            pdf_out = t(1) / (ar * s2pi) * np.exp(t(-0.5) * (r * r) / (ar * ar))
            Aq, Cq = t(op) * pdf_out, (t(1) - t(op)) * pdf_in
            tt = t(1) - Aq / (Cq + Aq)
        one_ = sb > ar
        tt = np.where(one_, t(1), tt)
        sqt = np.sqrt(tt)
        tmp4 = sqt * r2
        second = A.a(A.matvec(ex(V) if A.exact else A.a(V), ex(tmp4)))
        sh = sqt * second + (t(1) - tt) * r2
    else:
        sh = sh0
    vfl = t(var_floor)
    if mutant == "floor_after_blend":
        she = sh
    else:
        she = np.where(sh < vfl, vfl, sh)
    with np.errstate(all="ignore"):
        wh = t(1) / np.sqrt(she)
    ew = None if est_w is None else A.a(est_w)
    if ew is not None:
        fc = wh / (wh + ew)
        fe = t(1) - fc
        w = fc * wh + fe * ew
    else:
        w = wh
    if mutant == "floor_after_blend":
        w = np.minimum(w, t(1) / np.sqrt(vfl))
    w = np.maximum(w, t(1e-10))
    out["w"], out["t"] = w, tt
    if want_bounds:
        one = 1.0 + 1e-9
        xa = np.abs(np.asarray(x, dtype=f))
        dy = gamma(n) * (np.abs(rm) @ xa) * one
        rf, r2f = np.abs(np.asarray(r, dtype=f)), np.asarray(r2, dtype=f)
        dr = dy + U * rf
        dr2 = 2 * rf * dr + U * r2f
        Va = np.abs(np.asarray(V, dtype=f))
        dsh0 = (Va @ dr2 + gamma(m) * (Va @ r2f)) * one
        near = np.zeros(m, dtype=bool)
        if op > 0.0:
            sbf, shf0 = np.asarray(sb, dtype=f), np.asarray(sh0, dtype=f)
            dsb = dsh0 / (2 * sbf) + U * sbf
            near = np.abs(sbf - rf) <= 2.0 * (dsb + dr)
            arg = 0.5 * r2f / shf0
            darg = arg * (2 * dr / rf + 2 * dsb / sbf + 4 * U)
            rel_in = dsb / sbf + darg + 9 * U
            rel_out = dr / rf + 2 * U + 9 * U
            g = np.asarray(Aq / (Aq + Cq), dtype=f)
            tf = np.asarray(tt, dtype=f)
            dt = g * (1 - g) * (rel_in + rel_out + 3 * U) + 3 * U * g + U * np.abs(tf)
            dt = np.where(one_, 0.0, dt)
            sqf = np.sqrt(tf)
            with np.errstate(all="ignore"):
                dsq = np.where(one_, 0.0, dt / (2 * sqf) + U * sqf)
            t4 = np.asarray(tmp4, dtype=f)
            dt4 = dsq * r2f + sqf * dr2 + U * t4
            secf = np.asarray(second, dtype=f)
            dsec = (Va @ dt4 + gamma(m) * (Va @ t4)) * one
            dsh = (dsq * np.abs(secf) + sqf * dsec + U * np.abs(sqf * secf) + (dt + U * np.abs(1 - tf)) * r2f + np.abs(1 - tf) * dr2
                   + U * np.abs((1 - tf) * r2f) + U * np.abs(np.asarray(sh, dtype=f)))
            out["dt"] = 2.0 * dt
        else:
            dsh = dsh0
        shf = np.asarray(sh, dtype=f)
        dshe = np.where(shf < float(var_floor) - dsh, 0.0, dsh)
        whf = np.asarray(wh, dtype=f)
        dwh = whf * (dshe / (2 * np.asarray(she, dtype=f)) + 2 * U)
        if ew is not None:
            ef, fcf, fef = np.asarray(ew, dtype=f), np.asarray(fc, dtype=f), np.asarray(fe, dtype=f)
            S = whf + ef
            dS = dwh + U * np.abs(S)
            dfc = dwh / np.abs(S) + np.abs(fcf) * dS / np.abs(S) + U * np.abs(fcf)
            dfe = dfc + U * np.abs(fef)
            dw = (dfc * whf + np.abs(fcf) * dwh + U * np.abs(fcf * whf) + dfe * np.abs(ef) + U * np.abs(fef * ef)
                  + U * np.abs(np.asarray(fc * wh + fe * ew, dtype=f)))
        else:
            dw = dwh
        out["dw"] = 2.0 * dw
        out["near"] = near
    return out


def step(c, dtype=np.float64, mutant=None, want_bounds=False):
    """one hyper-parameter step of every spectrum of the case -> dict of arrays [B][...] in `dtype` (EXACT: float64 holding the
    once-rounded values).  want_bounds=True adds 'bound' (dict, same keys, float64) and 'exclude' (dict of bool arrays)."""
    A = _Arith(dtype)
    t = A.t
    f = np.float64
    B, m, n, ns = c["B"], c["m"], c["n"], c["ns"]
    nd = n - ns
    it, cm, min_iter = c["it"], c["continue_mode"], c["min_iter"]
    desc = c.get("desc")
    o = {key: np.array(c[key], dtype=t) for key in ("s", "rho", "xmx", "w", "x_in", "rv", "est_w", "coef_scale", "var_floor")}
    o["dop_rho"] = np.array(c["dop_rho"], dtype=t) if desc else None
    o["dop_xmx"] = np.array(c["dop_xmx"], dtype=t) if desc else None
    op = float(_opt(c, "outlier_p"))
    o["outlier_t"] = np.array(c["outlier_t"], dtype=t)
    vz = desc["vz_index"] if desc else -1
    nmat = B if c["rm"].ndim == 3 else 1
    o["rm_col"] = np.array([np.asarray(c["rm"][b] if c["rm"].ndim == 3 else c["rm"])[:, vz] for b in range(nmat)], dtype=t) if vz >= 0 else None
    o["active"], o["fit_status"], o["outer_iters"] = (np.array(c[key], dtype=np.int64) for key in ("active", "fit_status", "outer_iters"))
    o["n_active"] = int(c.get("n_active", 0))
    o["gmax"] = np.full((B, 2, 3), np.nan)
    o["converged"] = np.zeros(B, dtype=bool)
    o["mrel"], o["mabs"], o["atol"] = np.full(B, np.nan), np.full(B, np.nan), np.full(B, np.nan)
    bd = {key: np.zeros(np.shape(o[key])) for key in o if isinstance(o[key], np.ndarray) and o[key].dtype == t}
    excl = dict(w=np.zeros((B, m), dtype=bool), outlier_t=np.zeros((B, m), dtype=bool))
    mk = [np.asarray(v)[:n, :n] for v in c["mk"]]
    mask = None
    if c["toeplitz"] and c["toep_reach"] >= 0 and mutant in ("lastcol", "noalign"):
        mask = window_mask(nd, c["toep_reach"], mutant)
    dw_ = _opt(c, "derivative_weights")
    eff = bool(_opt(c, "eff_hp"))
    for b in range(B):
        if not c["active"][b]:
            continue
        if c["qp_status"][b] < 0:
            o["active"][b], o["fit_status"][b], o["outer_iters"][b] = 0, -1, it + 1
            continue
        x = np.asarray(c["x"][b], dtype=f)
        xd = x[ns:]
        for k in range(3):
            if not dw_[k] > 0.0:
                continue
            r = _update_block(A, c, k, xd, mk[k][ns:, ns:], mk[1][ns:, ns:], k == 0, _opt(c, "s_alpha")[k], _opt(c, "s_0")[k],
                              _opt(c, "sigma_ds")[k], _opt(c, "rho_alpha")[k], _opt(c, "rho_0")[k],
                              c["xmx"][b, (k + 1) % 3 if mutant == "xmx_order" else k], 1.0 if eff else c["rho"][b, k],
                              c["s"][b, k, ns:], mask, mutant, want_bounds)
            o["s"][b, k, ns:], o["rho"][b, k], o["gmax"][b, 0, k] = r["s"], r["rho"], r["gmax"]
            if want_bounds:
                bd["s"][b, k, ns:], bd["rho"][b, k] = r["ds"], r["drho"]
        if desc and desc["dop_size"] > 0:
            d0, dn = desc["dop_start"], desc["dop_size"]
            for k in range(3):
                if not desc["dop_derivative_weights"][k] > 0.0:
                    continue
                r = _update_block(A, c, k, x[d0:d0 + dn], mk[k][d0:d0 + dn, d0:d0 + dn], mk[1][d0:d0 + dn, d0:d0 + dn], False,
                                  desc["dop_s_alpha"][k], desc["dop_s_0"][k], 1.0, desc["dop_rho_alpha"][k], desc["dop_rho_0"][k],
                                  c["dop_xmx"][b, k], 1.0 if eff else c["dop_rho"][b, k], c["s"][b, k, d0:d0 + dn], None, mutant,
                                  want_bounds)
                o["s"][b, k, d0:d0 + dn], o["dop_rho"][b, k], o["gmax"][b, 1, k] = r["s"], r["rho"], r["gmax"]
                if want_bounds:
                    bd["s"][b, k, d0:d0 + dn], bd["dop_rho"][b, k] = r["ds"], r["drho"]
        if it == 0 and not cm:
            blocks = [("xmx", ns, nd)] + ([("dop_xmx", desc["dop_start"], desc["dop_size"])] if desc and desc["dop_size"] > 0 else [])
            for key, a0, an in blocks:
                xb = x[a0:a0 + an]
                for k in range(3):
                    Mb = mk[k][a0:a0 + an, a0:a0 + an]
                    Mm = Mb if (mask is None or key != "xmx") else np.where(mask, Mb, 0.0)
                    o[key][b, k] = A.dot(xb, A.matvec(Mm, xb) if A.exact else A.a(Mm) @ A.a(xb))
                    if want_bounds:
                        bd[key][b, k] = 2.0 * gamma(2 * an + 2) * (np.abs(xb) @ (np.abs(Mb) @ np.abs(xb))) * (1 + 1e-9)
        # weights (with the response matrix as it stands BEFORE the vz_offset column is rewritten)
        r = _weights(A, c, b, x, c["vmm"], c["est_w"][b], c["var_floor"][b], mutant, want_bounds)
        o["w"][b] = r["w"]
        if op > 0.0:
            o["outlier_t"][b] = r["t"]
        if want_bounds:
            bd["w"][b] = r["dw"]
            excl["w"][b] = r["near"]
            if op > 0.0:
                bd["outlier_t"][b], excl["outlier_t"][b] = r["dt"], r["near"]
        # convergence (qphb.py:597-603 with x_atol = mean(x_in) * 1e-3)
        xin = A.a(c["x_in"][b])
        dlt = A.a(x) - xin
        with np.errstate(all="ignore"):
            mrel = np.max(np.abs(dlt / (xin if mutant == "no_eps" else xin + t(1e-15))))
        mabs = np.max(np.abs(dlt))
        atol = A.total(c["x_in"][b]) / t(n) * t(1e-3)
        conv = bool(mrel <= t(_opt(c, "xtol"))) or bool(mabs <= atol)
        o["converged"][b], o["mrel"][b], o["mabs"][b], o["atol"][b] = conv, float(mrel), float(mabs), float(atol)
        o["x_in"][b] = A.a(x)
        if desc and vz >= 0 and cm != 2:
            x0 = x.copy()
            x0[vz] = 0.0
            x0[desc["vb_start"]:desc["vb_start"] + desc["vb_size"]] = 0.0
            rmb = np.asarray(c["rm"][b] if c["rm"].ndim == 3 else c["rm"])[:, :n]
            pred = A.a(A.matvec(rmb, x0))
            frozen = cm == 1 and c.get("vz_entry") is not None
            add = A.a(c["vz_entry"][b]) * t(x[vz]) if frozen else 0
            pred = pred + add
            sgn = np.where(np.arange(m) < desc["num_chrono"], 1.0, -1.0)
            o["rm_col"][b] = (A.a(sgn) * pred) * A.a(c["vz_strength"])
            if want_bounds:
                mag = np.abs(rmb) @ np.abs(x0) + (np.abs(np.asarray(c["vz_entry"][b]) * x[vz]) if frozen else 0.0)
                bd["rm_col"][b] = 2.0 * gamma(n + 3) * mag * np.abs(c["vz_strength"]) * (1 + 1e-9)
        stop = conv and it + 1 >= min_iter
        max_iter = int(_opt(c, "max_iter"))
        if _opt(c, "update_scale") and _opt(c, "scale_data") and it >= 1 and not stop and it + 1 < max_iter and not cm:
            rp = A.total(np.abs(xd)) * t(c["basis_area"])
            sf = np.sqrt(t(_opt(c, "rp_scale")) / rp)
            e = gamma(nd + 1) / 2 + 2 * U
            sff = float(sf)
            o["x_in"][b] = o["x_in"][b] * sf
            o["rv"][b] = o["rv"][b] * sf
            o["est_w"][b] = o["est_w"][b] / sf
            o["w"][b] = o["w"][b] / sf
            o["xmx"][b] = o["xmx"][b] * np.sqrt(sf)
            o["coef_scale"][b] = o["coef_scale"][b] / sf
            o["var_floor"][b] = o["var_floor"][b] * sf * sf
            if desc and desc["dop_size"] > 0:
                o["dop_xmx"][b] = o["dop_xmx"][b] * np.sqrt(sf)
            if want_bounds:
                a64 = lambda v: np.abs(np.asarray(v, dtype=f))
                bd["x_in"][b] = 2.0 * (e + U) * a64(o["x_in"][b])
                bd["rv"][b] = 2.0 * (e + U) * a64(o["rv"][b])
                bd["est_w"][b] = 2.0 * (e + U) * a64(o["est_w"][b])
                bd["w"][b] = bd["w"][b] / sff + 2.0 * (e + U) * a64(o["w"][b])
                bd["xmx"][b] = 2.0 * (e / 2 + 2 * U) * a64(o["xmx"][b])
                bd["coef_scale"][b] = 2.0 * (e + U) * a64(o["coef_scale"][b])
                bd["var_floor"][b] = 2.0 * (2 * e + 2 * U) * a64(o["var_floor"][b])
                if desc and desc["dop_size"] > 0:
                    bd["dop_xmx"][b] = 2.0 * (e / 2 + 2 * U) * a64(o["dop_xmx"][b])
        o["outer_iters"][b] = it + 1
        if stop:
            o["active"][b], o["fit_status"][b] = 0, 0
        elif it + 1 >= max_iter:
            o["active"][b], o["fit_status"][b] = 0, 1
        if not stop and it + 1 < max_iter:
            o["n_active"] += 1
    if want_bounds:
        o["bound"], o["exclude"] = bd, excl
    return o


FLOAT_KEYS = ("s", "rho", "xmx", "dop_rho", "dop_xmx", "w", "x_in", "outlier_t", "rv", "est_w", "coef_scale", "var_floor", "rm_col")
INT_KEYS = ("active", "fit_status", "outer_iters")


def ratios(got, ref):
    """worst |got - ref| / bound per floating-point output (entries of ref['exclude'] left out; an entry with a zero bound must be
    equal -- poison included -- else inf) -> dict key -> ratio"""
    out = {}
    for key in FLOAT_KEYS:
        if ref.get(key) is None or key not in got or got[key] is None:
            continue
        g, r, bnd = np.asarray(got[key]), ref[key], ref["bound"][key]
        ex = ref["exclude"].get(key)
        with np.errstate(invalid="ignore"):
            err = np.abs(np.asarray(g, dtype=np.longdouble) - np.asarray(r, dtype=np.longdouble)).astype(np.float64)
        err = np.where(np.isnan(err), np.inf, err)
        with np.errstate(divide="ignore", invalid="ignore"):
            q = np.where(err == 0, 0.0, np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), np.inf))
        if ex is not None:
            q = np.where(ex, 0.0, q)
        out[key] = float(np.max(q)) if q.size else 0.0
    return out


def ints_equal(got, ref):
    return all(np.array_equal(np.asarray(got[key]), ref[key]) for key in INT_KEYS) and int(got["n_active"]) == ref["n_active"]


def margins(ref, c):
    """how far the reference sits from every switch point: dict(gmax = min |log10(gmax / 1e-10)| over the blocks that ran,
    conv = min relative distance of mrel from xtol and of mabs from atol, excluded = largest excluded fraction of a spectrum)"""
    g = ref["gmax"][np.isfinite(ref["gmax"]) & (ref["gmax"] > 0)]
    gm = float(np.min(np.abs(np.log10(g / 1e-10)))) if g.size else np.inf
    xtol = _opt(c, "xtol")
    ok = np.isfinite(ref["mrel"])
    cv = np.inf
    if ok.any():
        cv = min(float(np.min(np.abs(ref["mrel"][ok] - xtol) / xtol)),
                 float(np.min(np.abs(ref["mabs"][ok] - ref["atol"][ok]) / np.maximum(np.abs(ref["atol"][ok]), 1e-300))))
    ex = max(float(v.mean(axis=-1).max()) for v in ref["exclude"].values())
    return dict(gmax=gm, conv=cv, excluded=ex)


# ---- the cases (shared by tests/test_hyper_util.py and tests/test_gpu_hyper.py) ----------------------------------------------------
def gaussian_rows(nd, reach, rng):
    """three first rows of Gaussian shape, exactly zero beyond `reach`: derivative orders 0, 1, 2 of a Gaussian Gram matrix"""
    d = np.arange(nd, dtype=float)
    a = 0.35 + 0.1 * rng.random()
    g = np.exp(-(a * d) ** 2)
    rows = [g, g * (1 - 2 * (a * d) ** 2) * 2 * a * a, g * (3 - 12 * (a * d) ** 2 + 4 * (a * d) ** 4) * 4 * a ** 4]
    for r in rows:
        r[min(max(reach, 0), nd - 1) + 1:] = 0.0
        if reach < nd and reach >= 0 and r[min(reach, nd - 1)] == 0.0:
            r[min(reach, nd - 1)] = 1e-3            # the reach is attained exactly
    return rows


def make_case(seed, B, nd, ns, m, toeplitz=True, reach=None, toep_reach=-1, ldm=None, ldrm=None, rm_batched=False, it=1,
              continue_mode=0, min_iter=1, opts=None, x_kind="pos", desc=None, est_kind="mixed", resid=0.05, floor_rows=0,
              outliers=0, huge_rows=0, conv=None, vz_entry=False, n_active=3, chrono_rows=0,
              active=None, qp_status=None):
    """one hook call's inputs.  x_kind: 'pos' | 'zeros' (some rows exactly 0) | 'neg' (mixed signs) | 'tiny' (|x| ~ 1e-9);
    conv: None (far from converged) or (criterion, side) with criterion 'rel' | 'abs' and side 'in' | 'out': x_in placed so that
    exactly that criterion lies 2e-3 relative inside / outside its threshold and the other one fails clearly; ('eps', 'in'): the
    relative criterion holds only because of the 1e-15 in its denominator (one entry of x_in is 1e-15)."""
    rng = np.random.default_rng(seed)
    n = nd + ns
    ldm, ldrm = ldm or n, ldrm or n
    o = dict(DEFAULT_OPTS)
    o.update(opts or {})
    reach_true = (nd - 1) if reach is None else min(reach, nd - 1)
    if toeplitz:
        special = [np.diag(np.concatenate([rng.uniform(0.5, 2.0, ns), np.zeros(nd)])) for _ in range(3)]
        if desc and desc.get("dop_size", 0) > 0:
            for sp in special:
                d0, dn = desc["dop_start"], desc["dop_size"]
                blk = rng.standard_normal((dn, dn))
                sp[d0:d0 + dn, d0:d0 + dn] = blk @ blk.T / dn + np.eye(dn)
        mk = toeplitz_penalty(n, ns, gaussian_rows(nd, reach_true, rng), special, ld=ldm)
    else:
        mk = []
        for _ in range(3):
            blk = rng.standard_normal((n, n))
            full = np.zeros((n, ldm))
            full[:, :n] = (blk + blk.T) / 2 + np.diag(rng.uniform(1.0, 2.0, n))
            mk.append(full)
    for mat in mk:
        mat[:, n:] = 977.0
    rm = np.full(((B,) if rm_batched else ()) + (m, ldrm), 977.0)
    rm[..., :n] = rng.standard_normal(rm[..., :n].shape) / np.sqrt(n)
    x = rng.uniform(0.2, 2.0, (B, n))
    if x_kind == "zeros":
        x[:, ns::3] = 0.0
    elif x_kind == "neg":
        x[:, ns:] *= rng.choice([-1.0, 1.0], (B, nd))
    elif x_kind == "tiny":
        x[:, ns:] = rng.uniform(0.5e-9, 2e-9, (B, nd)) * rng.choice([-1.0, 1.0], (B, nd))
    x_in = x * (1.0 + rng.uniform(0.05, 0.3, (B, n)) * rng.choice([-1.0, 1.0], (B, n)))
    if conv is not None:
        crit, side = conv
        xtol = o["xtol"]
        f = (1 - 2e-3) if side == "in" else (1 + 2e-3)
        if crit == "eps":
            x_in = x / (1.0 + 0.5 * xtol * rng.uniform(0.2, 1.0, (B, n)))
            x_in[:, 0] = 1e-15
            x[:, 0] = 1e-15 + 1.5e-17              # 0.0075 of x_in + 1e-15, 0.015 of x_in
        elif crit == "rel":
            # every |dx / x_in| = xtol * f at most, attained; |dx| well above 1e-3 mean(x_in) since xtol = 1e-2
            x_in = x / (1.0 + xtol * f * rng.uniform(0.2, 1.0, (B, n)))
            x_in[:, n - 1] = x[:, n - 1] / (1.0 + xtol * f)
        else:
            # one entry of x_in is tiny: its relative change is huge, every absolute change is atol * f at most, attained
            x_in = x.copy()
            x_in[:, 0] = 1e-12
            x[:, 0] = 2e-12
            at = x_in.mean(axis=1) * 1e-3
            x_in[:, 1:] = x[:, 1:] + (at * f)[:, None] * rng.uniform(0.1, 0.9, (B, n - 1))
            x_in[:, n - 1] = x[:, n - 1] + at * f
            for _ in range(40):                    # atol depends on x_in itself: a few fixed-point passes
                at = x_in.mean(axis=1) * 1e-3
                x_in[:, n - 1] = x[:, n - 1] + at * f
    vmm = np.abs(rng.standard_normal((m, m))) * np.exp(-0.5 * ((np.arange(m)[:, None] - np.arange(m)[None, :]) / 2.0) ** 2)
    vmm /= vmm.sum(axis=1, keepdims=True)
    oidx = floor_rows + 1 + 8 * np.arange(outliers)            # outlier rows: apart, so that none sits in another's variance window
    assert outliers == 0 or oidx[-1] < m - huge_rows
    for i in oidx:     # an outlier's own residual has little part in its variance estimate
        off = vmm[i].sum() - vmm[i, i]
        vmm[i] *= 0.98 / off
        vmm[i, i] = 0.02
    if chrono_rows:
        vmm[:chrono_rows] = 0.0
        vmm[:chrono_rows, :chrono_rows] = rng.uniform(0.5, 1.5, chrono_rows) / chrono_rows
    rv = np.empty((B, m))
    for b in range(B):
        rmb = (rm[b] if rm_batched else rm)[:, :n]
        scale = np.full(m, resid)
        scale[:floor_rows] = 1e-6                  # residuals far below the variance floor
        r = scale * rng.standard_normal(m) * rng.uniform(0.5, 1.5, m)
        if outliers:
            r[oidx] = 6.0 * resid * rng.choice([-1.0, 1.0], outliers)
        if huge_rows:
            r[m - huge_rows:] = 1e11
        rv[b] = rmb @ x[b] - r
    w_hat = 1.0 / resid
    if est_kind == "large":
        est_w = np.full((B, m), 1e4 * w_hat)
    elif est_kind == "small":
        est_w = np.full((B, m), 1e-4 * w_hat)
    elif est_kind == "floor":
        est_w = np.full((B, m), 1e-12)
    else:
        est_w = w_hat * 10.0 ** rng.uniform(-2, 2, (B, m))
    c = dict(seed=seed, B=B, m=m, n=n, ns=ns, nd=nd, rm=rm, vmm=vmm, mk=mk, toeplitz=bool(toeplitz), toep_reach=toep_reach,
             reach=reach_true if toeplitz else None, x=x, x_in=x_in, s=rng.uniform(0.2, 3.0, (B, 3, n)), rho=rng.uniform(0.5, 2.0, (B, 3)),
             xmx=rng.uniform(0.5, 2.0, (B, 3)), rv=rv, est_w=est_w, w=np.full((B, m), POISON),
             var_floor=np.array([np.var(rv[b]) * 1e-7 for b in range(B)]), coef_scale=rng.uniform(0.5, 2.0, B),
             qp_status=np.array(qp_status if qp_status is not None else np.zeros(B), dtype=np.int32),
             active=np.array(active if active is not None else np.ones(B), dtype=np.int32), fit_status=np.full(B, -77, dtype=np.int32),
             outer_iters=np.full(B, -77, dtype=np.int32), n_active=n_active, outlier_t=np.full((B, m), POISON), opts=o, it=it,
             continue_mode=continue_mode, min_iter=min_iter, basis_area=1.7724538509055159 / 1.2, desc=desc,
             dop_rho=rng.uniform(0.5, 2.0, (B, 3)) if desc else None, dop_xmx=rng.uniform(0.5, 2.0, (B, 3)) if desc else None,
             vz_strength=rng.uniform(0.5, 1.5, m) if desc and desc.get("vz_index", -1) >= 0 else None,
             vz_entry=rng.standard_normal((B, m)) if vz_entry else None)
    return c


def make_desc(**kw):
    d = dict(dop_start=0, dop_size=0, vz_index=-1, vb_start=0, vb_size=0, num_chrono=0, chrono_vmm_uniform=0,
             dop_derivative_weights=(1.0, 0.5, 0.25), dop_s_alpha=(4.0, 6.0, 8.0), dop_rho_alpha=(0.3, 0.4, 0.5), dop_s_0=(1.0, 2.0, 0.5),
             dop_rho_0=(1.0, 0.5, 2.0))
    d.update(kw)
    return d


# name -> (group, keyword arguments of make_case).  The shapes are the smallest at which each mechanism exists; see the opening test
# of tests/test_gpu_hyper.py for the arithmetic that places each on its side of a fold.
TOEP_ND = (1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 1023, 1024, 1025)
GEN_ND = (1, 2, 3, 5, 6, 510, 512, 514, 515)
GEN_M = (1, 2, 3, 4, 5, 31, 32, 33)
FORM_SHAPES = {"form1": (64, 2, 24), "form2": (1500, 2, 2000), "form2_tall": (820, 2, 5760), "form0": (1700, 2, 2000)}


BATCH_B = (1, 15, 16, 17, 31, 32, 33, 70)
BATCH_M = (1, 63, 64, 65, 130)
BATCH_N = (3, 15, 16, 17, 18, 34)


def toep_reaches(nd):
    return sorted({r for r in (0, 1, 2, 3, 4, 5, nd - 2, nd - 1, nd + 7) if r >= 0})


def case_table():
    T = {}
    seed = 1000
    for nd in TOEP_ND:
        for r in toep_reaches(nd):
            seed += 1
            T[f"toep_nd{nd}_r{r}"] = ("toeplitz", dict(seed=seed, B=2 if nd < 100 else 1, nd=nd, ns=2, m=24, reach=r, toep_reach=r, it=0))
    i = 0
    for nd in GEN_ND:
        for ns in (1, 2):
            for pad in (0, 1):
                seed += 1
                m = GEN_M[i % len(GEN_M)]
                i += 3
                T[f"gen_nd{nd}_ns{ns}_pad{pad}_m{m}"] = ("general", dict(seed=seed, B=2 if nd < 100 else 1, nd=nd, ns=ns, m=m, toeplitz=False,
                                                                        ldm=nd + ns + pad, ldrm=nd + ns + (pad if nd % 2 else 0), it=0,
                                                                        x_kind="neg" if i % 2 else "pos"))
    for name, (nd, ns, m) in FORM_SHAPES.items():
        seed += 1
        T[name] = ("forms", dict(seed=seed, B=1, nd=nd, ns=ns, m=m, reach=39, toep_reach=39, it=0))
    small = dict(B=2, nd=37, ns=2, m=24, reach=6, toep_reach=6)
    branches = {
        "zeros": dict(x_kind="zeros"), "neg": dict(x_kind="neg"), "zeros_general": dict(x_kind="zeros", toeplitz=False),
        "neg_general": dict(x_kind="neg", toeplitz=False),
        "tiny": dict(x_kind="tiny", opts=dict(sigma_ds=(1000.0, 1000.0, 1000.0))),
        "tiny_general": dict(x_kind="tiny", toeplitz=False, opts=dict(sigma_ds=(1000.0, 1000.0, 1000.0))),
        "alpha1": dict(x_kind="zeros", opts=dict(s_alpha=(5.0, 1.0, 25.0))),
        "alpha1_general": dict(x_kind="zeros", toeplitz=False, opts=dict(s_alpha=(5.0, 1.0, 25.0))),
        "noeff": dict(opts=dict(eff_hp=0)), "noeff_general": dict(toeplitz=False, opts=dict(eff_hp=0)),
        "order_off": dict(opts=dict(derivative_weights=(1.5, 0.0, 0.5))),
        "dop_2_5": dict(ns=8, it=0, desc=make_desc(dop_start=2, dop_size=5)),
        "dop_1_8": dict(ns=9, it=1, opts=dict(eff_hp=0), desc=make_desc(dop_start=1, dop_size=8, dop_derivative_weights=(1.0, 0.0, 0.25))),
    }
    for name, kw in branches.items():
        seed += 1
        T["s_" + name] = ("solve_s", dict(small, seed=seed, **kw))
    wsmall = dict(B=2, nd=21, ns=2, m=67, reach=5, toep_reach=5)
    weights = {
        "est_large": dict(est_kind="large"), "est_small": dict(est_kind="small"), "floor_rows": dict(floor_rows=9, resid=1e-3),
        "floor_1e10": dict(huge_rows=3, est_kind="floor"),
        "outlier": dict(outliers=4, opts=dict(outlier_p=0.05)), "outlier_floor": dict(outliers=3, floor_rows=5, opts=dict(outlier_p=0.05)),
        "no_outlier": dict(outliers=4),
    }
    for name, kw in weights.items():
        seed += 1
        T["w_" + name] = ("weights", dict(wsmall, seed=seed, **kw))
    for nc in (1, 5, 67):
        seed += 1
        T[f"w_chrono{nc}"] = ("weights", dict(wsmall, seed=seed, chrono_rows=nc, rm_batched=True,
                                              desc=make_desc(num_chrono=nc, chrono_vmm_uniform=1)))
    for m in (31, 32, 33, 65):
        for B in (1, 3):
            seed += 1
            T[f"prod_m{m}_B{B}"] = ("products", dict(seed=seed, B=B, nd=20 + m % 3, ns=2, m=m, reach=4, toep_reach=4))
    for i, B in enumerate(BATCH_B):
        seed += 1
        m, n = BATCH_M[i % len(BATCH_M)], BATCH_N[i % len(BATCH_N)]
        T[f"batch_B{B}_m{m}_n{n}"] = ("batch", dict(seed=seed, B=B, nd=n - 2, ns=2, m=m, reach=3, toep_reach=3, it=1 + i % 2))
    flow = {
        "rel_in": dict(conv=("rel", "in")), "rel_out": dict(conv=("rel", "out")), "abs_in": dict(conv=("abs", "in")),
        "abs_out": dict(conv=("abs", "out")), "eps_in": dict(conv=("eps", "in")), "min_iter": dict(conv=("rel", "in"), min_iter=3), "max_iter": dict(opts=dict(max_iter=2)),
        "max_iter_conv": dict(conv=("abs", "in"), opts=dict(max_iter=2)),
        "it0": dict(it=0), "it1": dict(it=1), "cont1_it0": dict(it=0, continue_mode=1), "cont2_it0": dict(it=0, continue_mode=2),
        "scale": dict(opts=dict(update_scale=1)), "scale_it0": dict(it=0, opts=dict(update_scale=1)),
        "scale_stop": dict(conv=("rel", "in"), opts=dict(update_scale=1)), "scale_last": dict(opts=dict(update_scale=1, max_iter=2)),
        "scale_cont": dict(continue_mode=1, opts=dict(update_scale=1)), "scale_noscale": dict(opts=dict(update_scale=1, scale_data=0)),
        "scale_dop": dict(ns=8, opts=dict(update_scale=1), desc=make_desc(dop_start=2, dop_size=5)),
    }
    flow["inactive"] = dict(B=4, active=(1, 0, 1, 0), qp_status=(0, 0, -1, -1), it=4)
    for name, kw in flow.items():
        seed += 1
        T["f_" + name] = ("flow", dict(small, seed=seed, **kw))
    vzd = dict(vz_index=1, vb_start=2, vb_size=2, num_chrono=10)
    for name, kw in {"vz": dict(), "vz_cont1": dict(continue_mode=1, vz_entry=True), "vz_cont1_plain": dict(continue_mode=1),
                     "vz_cont2": dict(continue_mode=2)}.items():
        seed += 1
        T["f_" + name] = ("flow", dict(small, seed=seed, ns=5, rm_batched=True, desc=make_desc(**vzd), **kw))
    return T


_CASES = {}


def get_case(name):
    """the case and its reference (extended precision, bounds, exclusions), computed once per process"""
    if name not in _CASES:
        group, kw = case_table()[name]
        c = make_case(**kw)
        if name == "s_order_off":
            c["s"][:, 1, :] = POISON
            c["rho"][:, 1] = POISON
        _CASES[name] = (c, step(c, reference_dtype(), want_bounds=True))
    return _CASES[name]
