"""Generators, an extended-precision KKT check and a CPU model of the coneqp kernel's carried product P x -- the reference side of
tests/test_gpu_qp_loop.py, checked on the CPU by tests/test_qp_util.py.  Test infrastructure only: the oracle (oracle/coneqp.py)
is used as it is and does not change.

The kernel (csrc/qp_common.hpp: ipm_solve) is cvxopt's coneqp for  min 1/2 x'Px + q'x  s.t.  -x <= h  with one deliberate departure:
P x is not formed by a pass over P in every iteration but follows the iterate by an O(n) recurrence,

    start point   (P + I) x0 = -q - h              =>  px = (-q - h) - x0
    every step    (P + D) dx = r,  D = diag(di^2)  =>  px += step (r - di^2 dx),    r = the corrector's right-hand side

and two rules send it back to a direct product:

    drift  sum of max|step dx| since the last direct product (start: max|x0|); once drift > kDriftTol max|x|, kDriftTol = 8, the next
           residual is taken from P x itself and drift restarts at max|x|;
    canc   sum of max step (|r| + di^2 |dx|) since the last direct product (start: max(|q + h| + |x0|)); a verdict -- "optimal", or
           the last test at maxiters -- taken on a carried product with kCancUlps eps sqrt(n) canc > 0.05 feastol resx0, kCancUlps = 64,
           eps = 2^-53, is taken again on a direct product.

`carried_model` is oracle.coneqp.coneqp_boxlow with exactly that, each rule switchable, and reports per iteration whether a rule
fired and by what ratio to its threshold.
"""
import math
import os

import numpy as np

from oracle.coneqp import ABSTOL, FEASTOL, MAXITERS, RELTOL, STEP, EXPON, KKTError, _factor, _kkt_solve, coneqp_boxlow

K_DRIFT_TOL = 8.0
K_CANC_ULPS = 64.0
EPS = 2.0 ** -53          # the kernel's constant 1.1102230246251565e-16
LD = np.longdouble


def opts_dict(opts=None):
    """None (defaults), a dict or an object with abstol / reltol / feastol / maxiters attributes -> keyword arguments of the oracle"""
    d = dict(abstol=ABSTOL, reltol=RELTOL, feastol=FEASTOL, maxiters=MAXITERS)
    if opts is None:
        return d
    for k in d:
        if isinstance(opts, dict):
            if k in opts:
                d[k] = opts[k]
        else:
            d[k] = getattr(opts, k)
    d["maxiters"] = int(d["maxiters"])
    return d


# ---- generators (all seeded) ------------------------------------------------------------------------------------------------------
def spd(n, seed=None):
    """the recipe of test_gpu_qp.py::test_qp_random_spd_vs_oracle, one problem: (P, q, h)"""
    rng = np.random.default_rng(n if seed is None else seed)
    M = rng.standard_normal((n + 3, n))
    return M.T @ M + 0.1 * np.eye(n), rng.standard_normal(n) * 3, np.where(rng.random(n) < 0.8, 0.0, 1000.0)


def badly_scaled(n, seed):
    """(M'M) o sqrt(c c') with row / column scales c = 10^U(-6, 6) plus a small ridge, q spanning decades, h = 0 but for one large bound"""
    rng = np.random.default_rng([n, seed, 77])
    M = rng.standard_normal((n + 3, n))
    c = 10.0 ** rng.uniform(-6, 6, n)
    sc = np.sqrt(c)
    P = (M.T @ M) * np.outer(sc, sc)
    P = 0.5 * (P + P.T) + 1e-9 * np.diag(np.diag(P))
    q = rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)
    h = np.zeros(n)
    h[int(rng.integers(n))] = 1000.0
    return P, q, h


def far_start(n, seed=0, bound=1e5):
    """a well-conditioned problem whose constraint vector is `bound` on all unknowns (nonneg off): the start point lies `bound` away
    from the solution and the iterates come down from there -- the case the drift rule was written for"""
    P, q, _ = spd(n, [n, seed, 5])
    return P, q, np.full(n, float(bound))


def late_breakdown(n, seed=0, pjj=-0.01, qj=-0.1):
    """an SPD block plus one decoupled unknown j = n - 1 with P_jj < 0, h = 0: P + I is positive definite (the start point exists),
    and the factorisation breaks down once di_j^2 has come down below -P_jj"""
    rng = np.random.default_rng([n, seed, 9])
    M = rng.standard_normal((n + 2, n - 1))
    P = np.zeros((n, n))
    P[:n - 1, :n - 1] = M.T @ M + 0.1 * np.eye(n - 1)
    P[n - 1, n - 1] = pjj
    q = np.append(rng.standard_normal(n - 1) * 3, qj)
    return P, q, np.zeros(n)


def golden_neg_qp(i):
    """QP i captured from the reference run with nonneg off (tests/golden/refrun_golden71x91_neg.npz): P, q, h, x, iterations"""
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "refrun_golden71x91_neg.npz"), allow_pickle=False)
    return g[f"qp{i}_P"], g[f"qp{i}_q"], g[f"qp{i}_h"], g[f"qp{i}_x"], int(g["qp_iterations"][i])


# ---- the extended-precision check of a returned point ------------------------------------------------------------------------------
def kkt_check(P, q, h, x, s, z, opts=None):
    """In np.longdouble: the true residuals of (x, s, z) as coneqp's stopping test defines them, the gap, the costs, and the rounding
    bound of ONE direct FP64 product P x + q - z relative to resx0 (dres_bound: worst case, (n + 2) eps | |P||x| + |q| + |z| |; dres_typical:
    the same with sqrt(n + 2), the size such an error has when the roundings do not conspire).  `ok` = the verdict "optimal" was earned: dres within 1.05 feastol
    plus that bound (5 % is what the kernel's own rule allows a carried residual to be off), pres within feastol plus a few eps,
    s, z > 0, gap <= abstol or relative gap <= reltol."""
    o = opts_dict(opts)
    P, q, h, x, s, z = (np.asarray(v, dtype=LD) for v in (P, q, h, x, s, z))
    n = q.size
    resx0 = max(LD(1), np.sqrt(q @ q))
    resz0 = max(LD(1), np.sqrt(h @ h))
    px = P @ x
    rx = px + q - z
    rz = s - h - x
    dres = np.sqrt(rx @ rx) / resx0
    pres = np.sqrt(rz @ rz) / resz0
    gap = s @ z
    f0 = LD(0.5) * (x @ (px + q) + x @ q)
    pcost = f0
    dcost = f0 + z @ rz - gap
    relgap = gap / -pcost if pcost < 0 else (gap / dcost if dcost > 0 else None)
    mag = np.abs(P) @ np.abs(x) + np.abs(q) + np.abs(z)
    dres_bound = (n + 2) * LD(2.0 ** -52) * np.sqrt(mag @ mag) / resx0
    # the same product's rounding error as it accumulates in the mean: sqrt(n + 2) terms' worth instead of the worst case's n + 2
    dres_typical = np.sqrt(LD(n + 2)) * LD(2.0 ** -52) * np.sqrt(mag @ mag) / resx0
    pres_bound = 4 * LD(2.0 ** -52) * np.sqrt(np.sum((np.abs(s) + np.abs(h) + np.abs(x)) ** 2)) / resz0
    ok = bool(dres <= LD(1.05) * o["feastol"] + dres_bound and pres <= o["feastol"] + pres_bound and np.all(s > 0) and np.all(z > 0)
              and (gap <= o["abstol"] or (relgap is not None and relgap <= o["reltol"])))
    return dict(dres=float(dres), pres=float(pres), gap=float(gap), pcost=float(pcost), dcost=float(dcost),
                relgap=None if relgap is None else float(relgap), dres_bound=float(dres_bound), dres_typical=float(dres_typical),
                pres_bound=float(pres_bound), ok=ok)


# ---- the kernel's trajectory on the CPU ------------------------------------------------------------------------------------------------
def carried_model(P, q, h, opts=None, drift_rule=True, canc_rule=True):
    """coneqp_boxlow with the kernel's carried P x (module docstring).  Returns the oracle's result keys plus `code` (the kernel's
    status: 0 optimal, 1 maxiters, 2 breakdown after the first iteration), `events`: one dict per pass through the stopping test
    -- it, direct (this pass used a direct product), drift_ratio = drift / (8 max|x|) after the update that follows (None when there
    is none), drift_fired, canc_ratio = 64 eps sqrt(n) canc / (0.05 feastol resx0) at the test, canc_fired, test_ratio = the largest of the
    stopping test's quantities over its threshold (the gap at its easier alternative; conv is test_ratio <= 1) -- and `true_dres`,
    the dual residual of the returned point from a direct product."""
    o = opts_dict(opts)
    abstol, reltol, feastol, maxiters = o["abstol"], o["reltol"], o["feastol"], o["maxiters"]
    P = np.ascontiguousarray(P, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64).ravel()
    h = np.asarray(h, dtype=np.float64).ravel()
    n = q.size
    resx0 = max(1.0, math.sqrt(float(q @ q)))
    resz0 = max(1.0, math.sqrt(float(h @ h)))
    ones = np.ones(n)
    try:
        L = _factor(P, ones)
    except KKTError:
        raise ValueError("Rank(A) < p or Rank([P; A; G]) < n")
    x, z = _kkt_solve(L, ones, -q, h.copy())
    px = (-q - h) - x
    drift = float(np.max(np.abs(x)))
    canc = float(np.max(np.abs(q + h) + np.abs(x)))
    s = -z
    nrms = math.sqrt(float(s @ s))
    ts = float(np.max(-s))
    if ts >= -1e-8 * max(nrms, 1.0):
        s = s + (1.0 + ts)
    nrmz = math.sqrt(float(z @ z))
    tz = float(np.max(-z))
    if tz >= -1e-8 * max(nrmz, 1.0):
        z = z + (1.0 + tz)
    gap = float(s @ z)
    d = di = lmbda = None
    status, code, iters, refresh, events = "unknown", 1, 0, False, []
    pcost = dcost = relgap = pres = dres = None
    while True:
        direct = refresh
        if direct:
            px = P @ x
            refresh = False
            canc = 0.0
        rx = px + q
        f0 = 0.5 * (float(x @ rx) + float(x @ q))
        rx = rx - z
        resx = math.sqrt(float(rx @ rx))
        rz = s - h - x
        resz = math.sqrt(float(rz @ rz))
        pcost = f0
        dcost = f0 + float(z @ rz) - gap
        if pcost < 0.0:
            relgap = gap / -pcost
        elif dcost > 0.0:
            relgap = gap / dcost
        else:
            relgap = None
        pres = resz / resz0
        dres = resx / resx0
        conv = pres <= feastol and dres <= feastol and (gap <= abstol or (relgap is not None and relgap <= reltol))
        canc_ratio = K_CANC_ULPS * EPS * math.sqrt(float(n)) * canc / (0.05 * feastol * resx0)
        gaps = [gap / abstol] + ([relgap / reltol] if relgap is not None else [])
        ev = dict(it=iters, direct=direct, drift_ratio=None, drift_fired=False, canc_ratio=canc_ratio, canc_fired=False,
                  pres=pres, dres=dres, gap=gap, relgap=relgap, conv=conv, test_ratio=max(pres / feastol, dres / feastol, min(gaps)))
        events.append(ev)
        if (conv or iters == maxiters) and not direct and canc_rule and canc_ratio > 1.0:
            ev["canc_fired"] = True
            refresh = True
            continue
        if conv:
            status, code = "optimal", 0
            break
        if iters == maxiters:
            status, code = "unknown", 1
            break
        if iters == 0:
            d = np.sqrt(s / z)
            di = 1.0 / d
            lmbda = np.sqrt(s * z)
        lmbdasq = lmbda * lmbda
        try:
            L = _factor(P, di)
        except KKTError:
            if iters == 0:
                raise ValueError("Rank(A) < p or Rank([P; A; G]) < n")
            status, code = "unknown", 2
            break
        mu = gap / n
        sigma = 0.0
        dsdz_a = None
        for i in (0, 1):
            ds = -dsdz_a - lmbdasq if i == 1 else -lmbdasq
            ds = ds + sigma * mu
            sv = ds / lmbda
            bz = -rz - d * sv
            zz = bz * di
            r = -rx - di * zz                         # the right-hand side of (P + D) dx = r
            dx, dz = _kkt_solve(L, di, -rx, bz)
            ds = sv - dz
            dsdz = float(ds @ dz)
            if i == 0:
                dsdz_a = ds * dz
            ds = ds / lmbda
            dz = dz / lmbda
            t = max(0.0, float(np.max(-ds)), float(np.max(-dz)))
            if t == 0.0:
                step = 1.0
            elif i == 0:
                step = min(1.0, 1.0 / t)
            else:
                step = min(1.0, STEP / t)
            if i == 0:
                sigma = min(1.0, max(0.0, 1.0 - step + dsdz / gap * step ** 2)) ** EXPON
        t_ = (di * di) * dx
        px = px + step * (r - t_)
        m0 = float(np.max(np.abs(step * dx)))
        m2 = float(np.max(step * (np.abs(r) + np.abs(t_))))
        x = x + step * dx
        m1 = float(np.max(np.abs(x)))
        ds = (1.0 + step * ds) * lmbda
        dz = (1.0 + step * dz) * lmbda
        sq_s = np.sqrt(ds)
        sq_z = np.sqrt(dz)
        d = d * sq_s / sq_z
        di = 1.0 / d
        lmbda = sq_s * sq_z
        s = lmbda * d
        z = lmbda * di
        gap = float(lmbda @ lmbda)
        drift += m0
        canc += m2
        ev["drift_ratio"] = drift / (K_DRIFT_TOL * m1) if m1 > 0 else math.inf
        if drift_rule and drift > K_DRIFT_TOL * m1:
            ev["drift_fired"] = True
            refresh = True
            drift = m1
        iters += 1
    t = P @ x + q - z
    return {"x": x, "s": s, "z": z, "status": status, "code": code, "gap": gap, "iterations": iters, "primal objective": pcost,
            "dual objective": dcost, "relative gap": relgap, "primal infeasibility": pres, "dual infeasibility": dres,
            "events": events, "true_dres": math.sqrt(float(t @ t)) / resx0}


def oracle(P, q, h, opts=None, trace=None):
    return coneqp_boxlow(P, q, h, trace=trace, **opts_dict(opts))


def oracle_code(res, opts=None):
    """the kernel's status for an oracle result: 0 optimal, 1 stopped at maxiters, 2 the factorisation broke down after iteration 0"""
    if res["status"] == "optimal":
        return 0
    return 1 if res["iterations"] == opts_dict(opts)["maxiters"] else 2


def sensitivity(P, q, h, opts=None, k=4, seed=0):
    """largest |x' - x| over k oracle runs with P (symmetrically) and q perturbed by relative 1e-13: how far the checker's own x moves
    under an input perturbation of a thousand ulps -- the scale a different but equally valid summation order is judged on"""
    rng = np.random.default_rng([seed, 13])
    x0 = oracle(P, q, h, opts)["x"]
    P = np.asarray(P, dtype=np.float64)
    q = np.asarray(q, dtype=np.float64)
    worst = 0.0
    for _ in range(k):
        E = rng.uniform(-1, 1, P.shape)
        E = 0.5 * (E + E.T)
        x1 = oracle(P * (1.0 + 1e-13 * E), q * (1.0 + 1e-13 * rng.uniform(-1, 1, q.shape)), h, opts)["x"]
        worst = max(worst, float(np.max(np.abs(x1 - x0))))
    return worst


def decisive_margin(P, q, h, opts=None):
    """From the oracle's trace: how far the quantity that decides the last stopping test lies from its threshold at the iteration
    before the last (`before` = largest value / threshold over the tests that still failed, >= 1) and at the last (`after` = largest
    value / threshold over the tests, with the gap test at its easier alternative, <= 1).  Both far from 1 (>= 2 and <= 1 / 2) means
    no equally valid arithmetic can stop one iteration earlier or later."""
    o = opts_dict(opts)
    trace = []
    res = oracle(P, q, h, o, trace=trace)

    def ratios(t):
        g = [t["gap"] / o["abstol"]]
        pc, dc = t["pcost"], t["dcost"]
        rel = t["gap"] / -pc if pc < 0 else (t["gap"] / dc if dc > 0 else None)
        if rel is not None:
            g.append(rel / o["reltol"])
        return max(t["pres"] / o["feastol"], t["dres"] / o["feastol"], min(g))
    after = ratios(trace[-1])
    before = ratios(trace[-2]) if len(trace) >= 2 else math.inf
    return dict(before=before, after=after, iterations=res["iterations"], status=res["status"])


# ---- the inputs the GPU tests rest on (tests/test_qp_util.py pins what makes them usable) -----------------------------------------------
LOOSE = dict(abstol=1e-3, reltol=1e-2, feastol=1e-3, maxiters=100)
TIGHT = dict(abstol=1e-10, reltol=1e-9, feastol=1e-10, maxiters=100)
# far start (h = 1e5 on all unknowns): (n, seed).  Chosen from seeds 0 .. 23 by the CPU model: the drift rule fires with ratio >= 2, the
# oracle's last stopping test is decided by a factor >= 2 on either side, and without the rule x moves by more than 2 x (10 x sensitivity)
# and the true dual residual of the returned point grows more than tenfold.
FAR_INPUTS = [(33, 22), (33, 23), (97, 15), (97, 19)]
# badly scaled, default tolerances: (n, seed).  The cancellation rule fires with ratio >= 2 and the verdict stands on the direct product:
# a trajectory check (in 450 draws the model found no input at the default tolerances whose result the rule changes).
CANC_DEFAULT = [(17, 8), (17, 11), (33, 7), (33, 8), (33, 9), (65, 0), (65, 10)]
# badly scaled, TIGHT tolerances: (n, seed).  In the model the carried residual passes the stopping test by a factor >= 2, the direct
# product the rule asks for fails it by a factor >= 2, and the iteration goes on for one more.  What the carried product is off by is
# rounding noise, so another summation order may find the direct product inside feastol at once; what holds in every form is that the
# returned point's TRUE dual residual is inside feastol -- and without the rule it is not, by a factor >= 2 beyond the allowance of
# tests/test_gpu_qp_loop.py::test_cancellation_rule_retakes_the_verdict.
CANC_TIGHT = [(17, 143), (33, 136)]


def named_input(kind, *key):
    if kind == "far":
        return far_start(*key)
    if kind == "neg":
        return golden_neg_qp(*key)[:3]
    return badly_scaled(*key)
