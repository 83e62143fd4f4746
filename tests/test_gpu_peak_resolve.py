"""GPU: per-peak coefficients, distributions and resistances on the device (csrc/peak_resolve.hip behind
hipdrt_plan_resolve_peaks and hipdrt_plan_integrate_drt) against their numpy statement (hipdrt/models/peaks.py) and against a
run of the reference (tests/golden/refrun_peak_resolve_golden71x91.npz).

1. The kernel alone, through hipdrt_debug_peak_resolve, on integer rows and ln grids of small integers.  Peak and trough indices,
   counts and statuses are equal to the statement's; eps_l / eps_r are equal too (one correctly rounded division and comparisons
   on both sides).  The floats are held to the statement evaluated in np.longdouble within DERIVED bounds (u = 2^-53):
     weights      w = exp(-a), a = (eps y)^2 formed with four roundings (y, the product, the square: (1 + u)^5), so
                  |dw| / w <= 5 u a + 4 u (a device exp within one ulp = 2 u, doubled); x_peaks = x_red * (w_i / sum_k w_k): relative bound bw_i + max_k bw_k + (P + 3) u, plus
                  an absolute 2^-1000 |x_red| / sum for weights in the denormal range
     peak_gammas  |E0| |dx_peaks| + (nb + 8) u sum_j |E0| |x_peaks|  (DESIGN section 12's bound of the MFMA contraction)
     r_coef       area * (sum_j |dx_peaks| + (nb + 8) u sum_j |x_peaks|) + 2 u |r_coef|
     r_peaks      sum_k d_k (|dg_k+1| + |dg_k|) / 2 + (nout + 12) u sum_k |t_k|, t_k = d_k (g_k+1 + g_k) / 2
   Every sum also gets (terms + 8) * 2^-1074: an operation whose result is sub-normal rounds to the spacing 2^-1074, absolutely.
   The worst ratio of a deviation to its bound is printed per test (DESIGN section 14 records them).
2. The chain on a 37-spectrum fit against the statement on downloaded predict_drt_batch rows and coefficients; against the
   reference fixture (indices equal, floats by parity() at 1e-7 of the row's peak); a failed fit; a prepared two-copy plan with
   row_scale; refusals.
"""
import os

import numpy as np
import pytest

from conftest import GOLDEN, parity

from hipdrt.models import peaks, predict

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
TINY = np.longdouble(2.0) ** -1074          # spacing of the sub-normal doubles
FREQ71 = np.logspace(6, -1, 71)
WORST = {}


@pytest.fixture(scope="module")
def ctx():
    from hipdrt import _ffi
    return _ffi.get_context(0)


def ratio(name, got, ref, bound):
    """assert |got - ref| <= bound element by element (NaN exactly where the reference has it); record the worst ratio"""
    got, ref, bound = np.asarray(got, dtype=LD), np.asarray(ref, dtype=LD), np.asarray(bound, dtype=LD)
    assert got.shape == ref.shape, (name, got.shape, ref.shape)
    nan = np.isnan(ref)
    assert np.array_equal(np.isnan(got), nan), name
    if nan.all():
        return
    err = np.abs(got - ref)[~nan]
    bd = np.broadcast_to(bound, ref.shape)[~nan]
    assert (err <= bd).all(), (name, float(np.max(err / np.maximum(bd, LD(1e-4000)))))
    r = float(np.max(np.where(bd > 0, err / np.where(bd > 0, bd, 1), 0))) if err.size else 0.0
    WORST[name] = max(WORST.get(name, 0.0), r)


def reference(f, fxx, pk, x_red, lt, lb, e0, lto, area, eps_kw):
    """the statement in np.longdouble on float64 decisions (indices and length scales are exact on both sides), and the bounds"""
    pk = np.asarray(pk, dtype=np.intp)
    tr = peaks.find_troughs(f, fxx, pk)
    el, er = peaks.peak_epsilons(lt, pk, tr, **eps_kw)
    P, nb = len(pk), len(lb)
    xr = np.asarray(x_red, dtype=LD)
    if P <= 1:
        xp = np.tile(xr, (P, 1))
        dxp = np.zeros((P, nb), dtype=LD)
    else:
        y = np.asarray(lb, dtype=LD)[None, :] - np.asarray(lt, dtype=LD)[pk][:, None]
        eps = np.where(y < 0, np.asarray(el, dtype=LD)[:, None], np.asarray(er, dtype=LD)[:, None])
        a = (eps * y) ** 2
        w = np.exp(-a)
        tot = np.sum(w, axis=0)
        with np.errstate(invalid="ignore", divide="ignore"):
            xp = xr * (w / tot)
            bw = 5 * U * a + 4 * U
            # (a weight that has underflowed carries no relative information: its own term drops out, the sum's stays)
            bsum = np.sum(bw * w, axis=0) / tot
            dxp = np.abs(xp) * (bw + bsum + (P + 3) * U) + np.abs(xr) * LD(2.0) ** -1000 / tot
        # float64 underflow of a whole column: the reference's 0 / 0
        w64 = peaks.peak_weights(lb, np.asarray(lt, dtype=float)[pk], el, er)
        xp = np.where(np.isnan(w64), LD(np.nan), xp)
    out = dict(peak_index=pk, troughs=tr, eps_l=el, eps_r=er, x_peaks=xp, dx_peaks=dxp)
    axp = np.abs(np.nan_to_num(xp))
    out["r_coef"] = np.sum(xp, axis=1) * LD(area)
    out["dr_coef"] = LD(area) * (np.sum(dxp, axis=1) + (nb + 8) * U * np.sum(axp, axis=1)) + 2 * U * np.abs(np.nan_to_num(out["r_coef"])) + \
        (nb + 8) * TINY * max(LD(area), 1)
    if e0 is not None:
        e0 = np.asarray(e0, dtype=LD)
        g = xp @ e0.T
        dg = dxp @ np.abs(e0).T + (nb + 8) * U * (axp @ np.abs(e0).T) + (nb + 8) * TINY
        d = np.diff(np.asarray(lto, dtype=LD))
        t = d * (g[:, 1:] + g[:, :-1]) / 2
        out["peak_gammas"], out["dpeak_gammas"] = g, dg
        out["r_peaks"] = np.sum(t, axis=1)
        out["dr_peaks"] = np.sum(np.abs(d) * (dg[:, 1:] + dg[:, :-1]) / 2, axis=1) + \
            (len(lto) + 12) * U * np.sum(np.abs(np.nan_to_num(d * (np.abs(g[:, 1:]) + np.abs(g[:, :-1])) / 2)), axis=1) + \
            (len(lto) + 8) * TINY * max(1, float(np.max(np.abs(d), initial=0)))
    return out


def compare(tag, out, b, ref, mp, nout):
    P = len(ref["peak_index"])
    assert out["count"][b] == P, (tag, b)
    assert out["peak_index"][b].tolist() == ref["peak_index"].tolist() + [-1] * (mp - P), (tag, b)
    assert out["trough_index"][b].tolist() == ref["troughs"].tolist() + [-1] * (mp - max(P - 1, 0)), (tag, b)
    assert np.array_equal(out["eps_l"][b, :P], ref["eps_l"]) and np.array_equal(out["eps_r"][b, :P], ref["eps_r"]), (tag, b)
    for k in ("eps_l", "eps_r", "r_coef", "x_peaks") + (("r_peaks", "peak_gammas") if nout else ()):
        assert np.isnan(out[k][b, P:]).all(), (tag, b, k, "padding")
    ratio("x_peaks", out["x_peaks"][b, :P], ref["x_peaks"], ref["dx_peaks"])
    ratio("r_coef", out["r_coef"][b, :P], ref["r_coef"], ref["dr_coef"])
    if nout:
        ratio("peak_gammas", out["peak_gammas"][b, :P], ref["peak_gammas"], ref["dpeak_gammas"])
        ratio("r_peaks", out["r_peaks"][b, :P], ref["r_peaks"], ref["dr_peaks"])


def grids(nfind, nb, nout):
    """ln grids of small integers; the basis and output points lie inside the find grid (no column underflows as a whole)"""
    lt = np.arange(nfind, dtype=float)
    lb = np.round(np.linspace(0, nfind - 1, nb))
    lto = np.round(np.linspace(0, nfind - 1, nout)) if nout > 1 else np.array([float(nfind // 2)])[:nout]
    return lt, lb, lto


BASIS_EPS = 0.5


def run_case(ctx, seed, nfind, nb, nout, P, B, copies=1, sign=1, use_keep=True, eps_kw=None, mp=None):
    from hipdrt import _ffi
    rng = np.random.default_rng(seed)
    eps_kw = eps_kw or {}
    mp = mp if mp is not None else min(64, max(P, 1) + (3 if P not in (16, 64) else 0))
    lt, lb, lto = grids(nfind, nb, nout)
    f = rng.integers(-3, 4, (B, nfind)).astype(float)
    fxx = rng.integers(-3, 4, (B, nfind)).astype(float)
    x = rng.integers(-4, 5, (B, copies * nb)).astype(float)
    counts = [P] + [int(c) for c in rng.integers(0, P + 1, B - 1)]
    pks = [np.sort(rng.choice(nfind, c, replace=False)) for c in counts]
    keep = np.zeros((B, nfind), dtype=np.int32)
    idx = np.full((B, mp), -1, dtype=np.int32)
    for b, pk in enumerate(pks):
        keep[b, pk] = 1
        idx[b, :len(pk)] = pk
    opts = _ffi.peak_resolve_opts(sign=sign, max_peaks=mp, **eps_kw)
    src = dict(keep=keep) if use_keep else dict(indices=idx)
    out = ctx.debug_peak_resolve(f, fxx, x, lt, lb, lto if nout else None, basis_eps=BASIS_EPS, copies=copies, opts=opts, **src)
    assert (out["status"] == 0).all()
    e0 = ctx.func_eval_matrix(lb, lto, BASIS_EPS, 0) if nout else None      # (the bits the kernel multiplies with)
    for b in range(B):
        x_red = predict.drt_params(x[b], nb, sign)
        ref = reference(f[b], fxx[b], pks[b], x_red, lt, lb, e0, lto, np.sqrt(np.pi) / BASIS_EPS, eps_kw)
        compare((nfind, nb, nout, P, B), out, b, ref, mp, nout)
    return out


SHAPES = [  # nfind, nb, nout, P, B
    (3, 1, 1, 0, 1), (4, 3, 2, 1, 3), (63, 4, 15, 2, 1), (64, 5, 16, 15, 3), (65, 15, 17, 16, 1), (255, 16, 65, 17, 3),
    (256, 17, 121, 33, 1), (257, 63, 1, 64, 3), (65, 64, 2, 2, 37), (257, 65, 16, 64, 1), (256, 514, 121, 17, 3),
    (64, 3, 65, 33, 1), (4, 3, 0, 3, 1),
]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_kernel_alone_on_integer_rows(ctx, shape):
    nfind, nb, nout, P, B = shape
    run_case(ctx, 1000 + nfind + nb, nfind, nb, nout, P, B, use_keep=(nb % 2 == 1))
    print("worst ratio to the bound so far:", {k: f"{v:.3f}" for k, v in WORST.items()})


@pytest.mark.parametrize("sign", [1, -1, 0])
def test_kernel_alone_two_copies_and_length_scale_options(ctx, sign):
    run_case(ctx, 7 + sign, 65, 17, 17, 5, 3, copies=2, sign=sign)
    run_case(ctx, 17 + sign, 65, 17, 17, 5, 3, copies=2, sign=sign, eps_kw=dict(min_epsilon=0.3, max_epsilon=0.9, epsilon_factor=2.0))
    run_case(ctx, 27 + sign, 65, 17, 17, 5, 3, copies=2, sign=sign, use_keep=False, eps_kw=dict(epsilon_uniform=0.2))


def adversarial():
    """rows (f, fxx, peaks, expected troughs) of 322 samples: the rules a parallel search gets wrong first"""
    n = 322
    rows = []
    base = np.full(n, 5.0)
    # tied minima across lanes 63 | 64 and threads 255 | 256 of the pair [1, 320): the first one wins
    for first in (63, 255):
        f = base.copy(); f[[0, n - 1]] = 0.0
        f[1 + first] = 1.0; f[1 + first + 1] = 1.0
        rows.append((f, np.zeros(n), [1, 320], [1 + first]))
    # ... in the f - fxx branch (f rises monotonically: no local minimum), and in the sign-change branch
    for first in (63, 255):
        f = np.arange(n, dtype=float) + 1.0
        fxx = f.copy(); fxx[1 + first] += 9.0; fxx[1 + first + 1] += 9.0
        rows.append((f, fxx, [1, 320], [1 + first]))
        f = np.where(np.arange(n) < 200, 7.0, -7.0); f[1 + first] = 0.0; f[1 + first + 1] = 0.0
        if first == 63:
            f[1 + 255] = 0.0
        rows.append((f, np.zeros(n), [1, 320], [1 + first]))
    # neighbouring peaks (e = s + 1), peaks at 1 and n - 2, two-pass peaks of opposite sign
    f = np.tile([3.0, 1.0, 2.0, 4.0], n // 4 + 1)[:n]
    rows.append((f, np.zeros(n), [1, 2, 3, 200, 201, n - 2], None))
    f = np.cos(np.arange(n) / 7.0).round(2) * 8
    rows.append((f, -f, [1, 23, 45, 67, n - 2], None))
    return n, rows


def test_adversarial_rows(ctx):
    from hipdrt import _ffi
    n, rows = adversarial()
    lt, lb, lto = grids(n, 33, 17)
    mp = 8
    f = np.array([r[0] for r in rows]); fxx = np.array([r[1] for r in rows])
    idx = np.full((len(rows), mp), -1, dtype=np.int32)
    for b, r in enumerate(rows):
        idx[b, :len(r[2])] = r[2]
    x = np.ones((len(rows), 33))
    out = ctx.debug_peak_resolve(f, fxx, x, lt, lb, lto, basis_eps=BASIS_EPS, indices=idx, opts=_ffi.peak_resolve_opts(max_peaks=mp))
    e0 = ctx.func_eval_matrix(lb, lto, BASIS_EPS, 0)
    for b, (fb, fxxb, pk, expect) in enumerate(rows):
        ref = reference(fb, fxxb, pk, x[b], lt, lb, e0, lto, np.sqrt(np.pi) / BASIS_EPS, {})
        if expect is not None:
            assert ref["troughs"].tolist() == expect, b                      # (the statement itself takes the first one)
        compare("adversarial", out, b, ref, mp, 17)
    # the window source: ties of the curvature's minimum across the same borders, windows sharing their border sample
    fxx = np.full((2, n), 2.0)
    fxx[0, [64, 65, 256, 257, 300]] = [-1, -1, -1, -1, -1]
    fxx[1, [10, 255, 256, 320]] = [-3, -4, -4, -4]
    ws, we = [0, 65, 258], [66, 259, n + 1]
    out = ctx.debug_peak_resolve(np.abs(fxx), fxx, np.ones((2, 33)), lt, lb, None, windows=(ws, we), opts=_ffi.peak_resolve_opts(max_peaks=3),
                                 want=("peak_index", "trough_index", "r_coef"))
    assert out["peak_index"].tolist() == [peaks.window_peaks(fxx[b], ws, we).tolist() for b in range(2)] == [[64, 65, 300], [10, 255, 320]]


def test_position_in_the_batch_does_not_change_the_bits(ctx):
    from hipdrt import _ffi
    rng = np.random.default_rng(5)
    nfind, nb, nout, B, mp = 129, 70, 33, 37, 20
    lt, lb, lto = grids(nfind, nb, nout)
    f, fxx = rng.normal(size=(B, nfind)), rng.normal(size=(B, nfind))
    x = rng.normal(size=(B, nb))
    keep = (rng.random((B, nfind)) < 0.1).astype(np.int32)
    keep[36, :] = 0; keep[36, [3, 9, 40, 41, 100, 127]] = 1
    o = _ffi.peak_resolve_opts(max_peaks=mp)
    many = ctx.debug_peak_resolve(f, fxx, x, lt, lb, lto, basis_eps=BASIS_EPS, keep=keep, opts=o)
    one = ctx.debug_peak_resolve(f[36:], fxx[36:], x[36:], lt, lb, lto, basis_eps=BASIS_EPS, keep=keep[36:], opts=o)
    assert one["count"][0] == 6
    for k, v in one.items():
        if k != "lds_bytes":
            assert np.array_equal(v[0], many[k][36], equal_nan=True), k


def test_overflow_failed_rows_and_refusals(ctx):
    from hipdrt import _ffi
    nfind, nb = 40, 9
    lt, lb, lto = grids(nfind, nb, 5)
    f = np.tile(np.arange(nfind, dtype=float) % 5, (3, 1)); fxx = -f
    x = np.ones((3, nb))
    keep = np.zeros((3, nfind), dtype=np.int32)
    keep[0, [2, 7, 12]] = 1; keep[1, [1, 5, 9, 13, 17]] = 1; keep[2, [3, 30]] = 1
    o = _ffi.peak_resolve_opts(max_peaks=4)
    out = ctx.debug_peak_resolve(f, fxx, x, lt, lb, lto, basis_eps=BASIS_EPS, keep=keep, fit_status=[0, 0, -2], opts=o)
    assert out["status"].tolist() == [0, _ffi.PEAKS_OVERFLOW, -2] and out["count"].tolist() == [3, 5, 0]
    for b in (1, 2):
        assert (out["peak_index"][b] == -1).all() and (out["trough_index"][b] == -1).all()
        for k in ("eps_l", "eps_r", "r_peaks", "r_coef", "x_peaks", "peak_gammas"):
            assert np.isnan(out[k][b]).all(), (b, k)
    assert out["peak_index"][0].tolist() == [2, 7, 12, -1] and np.isfinite(out["peak_gammas"][0, :3]).all()
    # the stated shape fits one workgroup's LDS; two 16-peak tiles of a 1024-point basis do not
    big = np.zeros((1, 512)), np.zeros((1, 512)), np.zeros((1, 1024)), np.arange(512.0), np.arange(1024.0) / 2, np.arange(121.0) * 4
    idx = np.full((1, 16), -1, dtype=np.int32); idx[0, :2] = [100, 300]
    ok = ctx.debug_peak_resolve(*big, basis_eps=BASIS_EPS, indices=idx, opts=_ffi.peak_resolve_opts(max_peaks=16), want=("r_peaks",))
    assert 135 * 1024 < ok["lds_bytes"] <= 160 * 1024 - 256 and ok["count"][0] == 2
    with pytest.raises(_ffi.HipDrtError, match="LDS"):
        ctx.debug_peak_resolve(*big, basis_eps=BASIS_EPS, indices=np.full((1, 17), -1, dtype=np.int32), opts=_ffi.peak_resolve_opts(max_peaks=17))
    assert ctx.last_peak_resolve_lds > 160 * 1024
    for bad, what in (([5, 5, -1, -1], "strictly increasing"), ([7, 5, -1, -1], "strictly increasing"), ([5, 40, -1, -1], "out of range"),
                      ([5, -1, 9, -1], "padding"), ([-2, 5, 9, -1], "out of range")):
        with pytest.raises(_ffi.HipDrtError, match=what):
            ctx.debug_peak_resolve(f[:1], fxx[:1], x[:1], lt, lb, lto, basis_eps=BASIS_EPS, indices=np.array([bad]), opts=o)
    with pytest.raises(_ffi.HipDrtError, match="windows"):
        ctx.debug_peak_resolve(f[:1], fxx[:1], x[:1], lt, lb, lto, basis_eps=BASIS_EPS, windows=([0, 50], [10, 60]), opts=o)
    with pytest.raises(_ffi.HipDrtError, match="sign must be 1"):
        ctx.debug_peak_resolve(f[:1], fxx[:1], x[:1], lt, lb, lto, basis_eps=BASIS_EPS, keep=keep[:1], opts=_ffi.peak_resolve_opts(sign=0, max_peaks=4))
    with pytest.raises(_ffi.HipDrtError, match="max_peaks"):
        ctx.debug_peak_resolve(f[:1], fxx[:1], x[:1], lt, lb, lto, basis_eps=BASIS_EPS, keep=keep[:1], opts=_ffi.peak_resolve_opts(max_peaks=65))
    with pytest.raises(_ffi.HipDrtError, match="non-finite"):
        ctx.debug_peak_resolve(np.full((1, nfind), np.nan), fxx[:1], x[:1], lt, lb, lto, basis_eps=BASIS_EPS, keep=keep[:1], opts=o)
    # two windows that choose their shared border sample: upstream fails on the repeated peak; here a status
    fxx2 = np.full((1, nfind), 1.0); fxx2[0, 10] = -5.0
    out = ctx.debug_peak_resolve(f[:1], fxx2, x[:1], lt, lb, None, windows=([0, 10], [11, nfind + 1]), opts=o, want=("r_coef",))
    assert out["status"].tolist() == [_ffi.PEAKS_UNORDERED] and np.isnan(out["r_coef"]).all()


# ---- the whole chain -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fit37():
    from hipdrt import synth
    from hipdrt.models import DRT
    z = synth.zarc2_batch(FREQ71, 37, first_seed=900)
    drt = DRT(warn=False)
    res = drt.fit_eis_batch(FREQ71, z)
    assert (res["status"] >= 0).all()
    return drt, z, res


def chain_against_statement(ctx, drt, x_red, sign, tau_find, tau_out, find_kw, eps_kw=None):
    """quantify / coef / drts of the batch against the statement on downloaded rows; returns the number of peaks seen"""
    eps_kw = eps_kw or {}
    bt, eps = drt.basis_tau, drt.tau_epsilon
    f = drt.predict_drt_batch(tau=tau_find, order=0, sign=sign)
    fxx = drt.predict_drt_batch(tau=tau_find, order=2, sign=sign)
    _, _, idx, _ = drt.find_peaks_batch(tau=tau_find, sign=sign, return_info=True, **find_kw)
    r_peaks, info = drt.quantify_peaks_batch(tau=tau_out, tau_find_peaks=tau_find, sign=sign, find_peaks_kw=find_kw, return_info=True, **eps_kw)
    x_peaks = drt.estimate_peak_coef_batch(tau=tau_find, sign=sign, **eps_kw, **find_kw)
    gammas = drt.estimate_peak_drts_batch(tau=tau_out, tau_find_peaks=tau_find, sign=sign, find_peaks_kw=find_kw, **eps_kw)
    e0 = ctx.func_eval_matrix(np.log(bt), np.log(tau_out), eps, 0)
    total = 0
    for b in range(len(f)):
        ref = reference(f[b], fxx[b], idx[b], x_red[b], np.log(tau_find), np.log(bt), e0, np.log(tau_out), np.sqrt(np.pi) / eps, eps_kw)
        P = len(idx[b])
        total += P
        assert info["peak_index"][b].tolist() == list(idx[b]) and info["trough_index"][b].tolist() == ref["troughs"].tolist(), b
        assert np.array_equal(info["eps_l"][b], ref["eps_l"]) and np.array_equal(info["eps_r"][b], ref["eps_r"]), b
        assert x_peaks[b].shape == (P, len(bt)) and gammas[b].shape == (P, len(tau_out)) and r_peaks[b].shape == (P,)
        ratio("chain_x_peaks", x_peaks[b], ref["x_peaks"], ref["dx_peaks"])
        ratio("chain_peak_gammas", gammas[b], ref["peak_gammas"], ref["dpeak_gammas"])
        ratio("chain_r_peaks", r_peaks[b], ref["r_peaks"], ref["dr_peaks"])
        ratio("chain_r_coef", info["r_coef"][b], ref["r_coef"], ref["dr_coef"])
    return total


def test_chain_against_the_statement_on_downloaded_rows(ctx, fit37):
    drt, z, res = fit37
    ns = drt._plan.ns
    x_red = res["x"][:, ns:] * res["coefficient_scale"][:, None]
    tau10, tau20 = drt.get_tau_eval(10), drt.get_tau_eval(20)
    assert chain_against_statement(ctx, drt, x_red, 1, tau10, tau20, {}) >= 37
    assert chain_against_statement(ctx, drt, x_red, 1, tau10, tau10, dict(method="prob"), dict(min_epsilon=0.4)) >= 37
    # windows: the trapezoid of the downloaded row, and one resolved peak per window
    row = drt.predict_drt_batch(tau=tau20)
    start, end = peaks.split_windows(tau20, [1e-4, 1e-2])
    got = drt.split_r_p_batch([1e-4, 1e-2])
    want = np.array([peaks.window_integrals(r, np.log(tau20), start, end) for r in row])
    assert got.shape == (37, 3)
    parity("split_r_p", got, want, default=1e-13)               # (sums of <= 81 terms in another order: (nout + 12) u)
    got = drt.integrate_drt_batch(1e-5, 1e-1)
    tau = np.logspace(np.log10(1e-5), np.log10(1e-1), int((np.log10(1e-1) - np.log10(1e-5)) * 10) + 1)
    row = drt.predict_drt_batch(tau=tau)
    parity("integrate_drt", got, [peaks.trapezoid(r, np.log(tau)) for r in row], default=1e-13)
    assert drt.integrate_drt(1e-5, 1e-1, b=4) == got[4] and np.array_equal(drt.split_r_p([1e-4, 1e-2], b=7), drt.split_r_p_batch([1e-4, 1e-2])[7])
    fxx20, f20 = drt.predict_drt_batch(tau=tau20, order=2, sign=1), drt.predict_drt_batch(tau=tau20, sign=1)
    got = drt.split_r_p_batch([1e-4, 1e-2], resolve_peaks=True)
    for b in range(37):
        pk = peaks.window_peaks(fxx20[b], start, end)
        ref = reference(f20[b], fxx20[b], pk, x_red[b], np.log(tau20), np.log(drt.basis_tau), None, None, np.sqrt(np.pi) / drt.tau_epsilon, {})
        ratio("chain_split_resolved", got[b], ref["r_coef"], ref["dr_coef"])
    print("worst ratio to the bound:", {k: f"{v:.3f}" for k, v in WORST.items()})


def test_alone_and_in_a_batch_give_the_same_bits(fit37):
    from hipdrt.models import DRT
    drt, z, res = fit37
    tau20 = drt.get_tau_eval(20)
    many = drt.quantify_peaks_batch(tau=tau20, return_info=True)
    many_g = drt.estimate_peak_drts_batch(tau=tau20)
    one = DRT(warn=False)
    r1 = one.fit_eis_batch(FREQ71, z[36:37])
    assert np.array_equal(r1["x"][0], res["x"][36]), "the fit itself differs between batch sizes: nothing to compare"
    single = one.quantify_peaks_batch(tau=tau20, return_info=True)
    assert np.array_equal(single[0][0], many[0][36]) and len(single[0][0]) >= 1
    for k in ("peak_index", "trough_index", "eps_l", "eps_r", "r_coef"):
        assert np.array_equal(single[1][k][0], many[1][k][36]), k
    assert np.array_equal(one.estimate_peak_drts_batch(tau=tau20)[0], many_g[36])
    assert np.array_equal(one.quantify_peaks(tau=tau20), many[0][36])


FITS = {"plain": (dict(), dict()), "nn": (dict(nonneg=False), dict()), "sneg": (dict(series_neg=True), dict(normalize=False))}


@pytest.mark.parametrize("tag", ["plain", "nn", "sneg"])
def test_fit_against_the_reference_run(tag):
    from hipdrt.models import DRT
    g = np.load(os.path.join(GOLDEN, "refrun_peak_resolve_golden71x91.npz"))
    fit_kw, fkw = FITS[tag]
    drt = DRT()
    drt.fit_eis(g["freq"], g["z"], **fit_kw)
    tau10, tau20 = g[f"{tag}_tau10"], g[f"{tag}_tau20"]
    np.testing.assert_allclose(drt.get_tau_eval(10), tau10, rtol=1e-13)
    x_peaks = drt.estimate_peak_coef(sign=1, **fkw)
    parity("x_peaks", x_peaks, g[f"{tag}_x_peaks"], default=1e-7)
    for k, tau in (("10", tau10), ("20", tau20)):
        r_peaks, info = drt.quantify_peaks_batch(tau=tau, sign=1, find_peaks_kw=dict(fkw), return_info=True)
        assert info["peak_index"][0].tolist() == g[f"{tag}_peak_index"].tolist(), k
        assert info["trough_index"][0].tolist() == g[f"{tag}_trough_index"].tolist(), k
        gam = drt.estimate_peak_drts(tau=tau, sign=1, find_peaks_kw=dict(fkw))
        parity(f"peak_gammas{k}", gam, g[f"{tag}_peak_gammas{k}"], default=1e-7)
        parity(f"r_peaks{k}", r_peaks[0], g[f"{tag}_r_peaks{k}"], default=1e-7)
        assert drt.quantify_peaks(tau=tau, sign=1, find_peaks_kw=dict(fkw)) == list(r_peaks[0])
    parity("split", drt.split_r_p(list(g["tau_splits"])), g[f"{tag}_split"], default=1e-7)
    parity("integral", [drt.integrate_drt(*g["integrate_lim"])], [g[f"{tag}_integral"]], default=1e-7)
    if f"{tag}_split_resolved" in g.files:
        parity("split_resolved", drt.split_r_p(list(g["tau_splits"]), resolve_peaks=True), g[f"{tag}_split_resolved"], default=1e-7)


def test_prepared_two_copy_plan_with_row_scale_against_the_statement(ctx):
    """a series_neg fit runs on a prepared plan at unit scale: the coefficient scale travels as row_scale; signs 0 and -1 are
    checked against the statement only (upstream raises for them in estimate_peak_coef)"""
    from hipdrt import synth
    from hipdrt.models import DRT
    z = synth.zarc2_batch(FREQ71, 1, first_seed=41)
    drt = DRT(warn=False)
    drt.fit_eis(FREQ71, z[0], series_neg=True)
    plan, scales = drt._predict_plan("test")
    assert scales is not None and scales[0] != 1.0
    nb = len(drt.basis_tau)
    x = plan.get("x")[:, plan.ns:] * scales[:, None]
    tau10, tau20 = drt.get_tau_eval(10), drt.get_tau_eval(20)
    for sign in (0, -1, 1):
        n = chain_against_statement(ctx, drt, predict.drt_params(x, nb, sign), sign, tau10, tau20, dict(normalize=False))
        assert n >= 1 or sign == -1
    assert len(drt.quantify_peaks_batch()[0]) >= 1                # sign=None: the net distribution of a series_neg fit


def test_failed_fit_gives_empty_results():
    from hipdrt import synth
    from hipdrt.models import DRT
    z = synth.zarc2_batch(FREQ71, 5, first_seed=300)
    zbad = z.copy()
    zbad[2] = np.nan
    good, bad = DRT(warn=False), DRT(warn=False)
    good.fit_eis_batch(FREQ71, z)
    res = bad.fit_eis_batch(FREQ71, zbad)
    assert res["status"][2] < 0
    a, c = bad.quantify_peaks_batch(return_info=True), good.quantify_peaks_batch(return_info=True)
    assert len(a[0][2]) == 0 and len(a[1]["peak_index"][2]) == 0 and bad.estimate_peak_drts_batch()[2].shape == (0, len(bad.get_tau_eval(10)))
    for b in (0, 1, 3, 4):
        assert np.array_equal(a[0][b], c[0][b]) and len(a[0][b]) >= 1
    out = bad._plan.resolve_peaks(np.log(bad.get_tau_eval(10)), np.log(bad.get_tau_eval(10)))
    assert out["status"][2] < 0 and out["count"][2] == 0 and (out["peak_index"][2] == -1).all() and np.isnan(out["x_peaks"][2]).all()
    assert np.isnan(bad.split_r_p_batch([1e-3])[2]).all() and np.isnan(bad.split_r_p_batch([1e-3], resolve_peaks=True)[2]).all()
    assert np.isnan(bad.integrate_drt_batch(1e-5, 1e-1)[2])


def test_refusals_of_the_chain(fit37):
    from hipdrt import _ffi
    drt = fit37[0]
    tau = drt.get_tau_eval(10)
    for name, value in (("peak_tau", [1e-3]), ("trough_tau", [1e-2]), ("squeeze_factors", [1.0])):
        with pytest.raises(NotImplementedError, match=name):
            drt.estimate_peak_drts_batch(**{name: value})
    with pytest.raises(NotImplementedError, match="peak_tau"):
        drt.estimate_peak_coef(peak_tau=[1e-3])
    with pytest.raises(NotImplementedError, match="x="):
        drt.quantify_peaks_batch(x=np.ones(3))
    with pytest.raises(NotImplementedError, match="distance"):
        drt.estimate_peak_coef_batch(distance=3)
    with pytest.raises(ValueError, match="tau grid"):
        drt.estimate_peak_coef_batch(peak_indices=[3, 9])
    with pytest.raises(_ffi.HipDrtError, match="sign must be 1"):
        drt._plan.resolve_peaks(np.log(tau), np.log(tau), opts=_ffi.peak_resolve_opts(sign=0))
    with pytest.raises(_ffi.HipDrtError, match="strictly increasing"):
        drt._plan.resolve_peaks(np.log(tau), None, peak_indices=np.tile([9, 3] + [-1] * 14, (37, 1)))
    with pytest.raises(_ffi.HipDrtError, match="LDS"):
        drt._plan.resolve_peaks(np.linspace(-20, 5, 12000), None)
    # caller's indices: one row for all spectra; more than 16 peaks widen the slots
    rows = drt.estimate_peak_coef_batch(tau=tau, peak_indices=list(range(2, 2 + 3 * 20, 3)))
    assert all(r.shape == (20, len(drt.basis_tau)) for r in rows)
    # overflow: the call is repeated once with the largest count
    few = drt._plan.resolve_peaks(np.log(tau), None, opts=_ffi.peak_resolve_opts(max_peaks=1), want=("r_coef",))
    assert (few["status"][few["count"] > 1] == _ffi.PEAKS_OVERFLOW).all() and (few["count"] > 1).any()
