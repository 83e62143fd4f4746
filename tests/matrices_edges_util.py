"""Cases, inputs and extended-precision statements for the matrix builders of csrc/matrices.hip at their launch edges
(tests/test_gpu_matrices_edges.py on the device, tests/test_matrices_edges_util.py pins this file on the CPU).

Every operation is stated once in np.longdouble on the float64 inputs exactly as given: the trapezoid rule
sum d_j (f_{j+1} + f_j) / 2 on y = np.linspace(-20, 20, ny) (formed in float64, then widened), np.interp with numpy's
semantics (end clamping, knot shortcut, un-fused evaluation), the penalty closed forms, the row-normalised Gaussians of the
two variance matrices and the basis evaluation matrix.  The phasance columns need a complex erf and 1 / Gamma, which numpy
has in no extended precision: tools/make_phasor_edges_golden.py states them with mpmath and writes
tests/golden/phasor_edges_mp.npz.

Bounds (tests/matrices_edges_bounds.json, "quantity": [measured, bound]): `measured` is the deviation of the float64 oracle
(oracle/drt_oracle.py, or plain numpy where the oracle has no such function) from the extended-precision statement on the
inputs of the GPU cases, as a fraction of the statement's largest entry; bound = 10 x measured, rounded up to the next 1-2-5
step, never below 16 x 2^-52.  No bound comes from a run of the code under test."""
import json
import os

import numpy as np

LD = np.longdouble
HERE = os.path.dirname(os.path.abspath(__file__))
BOUNDS = os.path.join(HERE, "matrices_edges_bounds.json")
PHASOR_GOLDEN = os.path.join(HERE, "golden", "phasor_edges_mp.npz")
FLOOR = 16 * 2.0 ** -52
PI_LD = 4 * np.arctan(LD(1))
EPS_DEFAULT = 4.342944819032518
# 2.0 * PI * F_UNIT_OMEGA == 1.0 exactly in float64: ln(omega) is 0 on any libm, and with nu = 1 the phasance kernel's complex
# erf gets x == 0 (test_matrices_edges_util.py pins it)
F_UNIT_OMEGA = 1.0 / (2.0 * np.pi)


# ---- the launchers' geometry, restated (hipdrt_debug_impedance_interp_form reads the library's own back) ----------------------
LDS_LIMIT = 160 * 1024 - 256             # kLdsLimit
NY_MAX = 6000                            # kNyMax
GRID_DIM_MAX = 65535                     # kGridDimMax


def interp_lds_bytes(ng, rpb):
    """impedance_interp_lds: knots padded to an even count, (value, slope) pairs, ln(omega) of the workgroup's rows"""
    return (6 * (ng + (ng & 1)) + rpb) * 8


def interp_form(B, nf, ntau, ng=2000):
    """impedance_interp_form: threads per row, rows per workgroup, rows a thread steps by, dynamic LDS"""
    tpr = min(((ntau + 1) // 2 + 63) // 64 * 64, 1024)
    while 1024 % tpr:
        tpr += 64
    rpb = 256
    while rpb > 4 and B * ((nf + rpb - 1) // rpb) < 1024:
        rpb //= 2
    while rpb > 4 and interp_lds_bytes(ng, rpb) > LDS_LIMIT:
        rpb //= 2
    return dict(tpr=tpr, rpb=rpb, rp=1024 // tpr, lds=interp_lds_bytes(ng, rpb))


def block_rows(nf, rpb):
    """row counts of the workgroups of one spectrum"""
    return [min(rpb, nf - r0) for r0 in range(0, nf, rpb)]


def two_row_passes(nf, form):
    """passes of `for (; r + rp < rend; r += 2 * rp)` that the thread row tr = 0 of the fullest workgroup makes"""
    rows, rp = max(block_rows(nf, form["rpb"])), form["rp"]
    return len(range(0, max(rows - rp, 0), 2 * rp))


INTERP_NGRID_MAX = max(ng for ng in range(3300, 3500) if interp_lds_bytes(ng, 4) <= LDS_LIMIT)
RESPONSE_NGRID_MAX = LDS_LIMIT // 24      # response_interp_lds: three tables
REF_ROWS, REF_COLS = 4096, 128            # a B = 1 build of at most this size is rpb = 4, tpr = 64: no two-row pass, no column wrap


def toeplitz_grid_z(B):
    return min(B, 64)


def response_rpb(nt, ntau):
    rpb = 32
    while rpb > 1 and ((ntau + 255) // 256) * ((nt + rpb - 1) // rpb) < 1024:
        rpb //= 2
    return rpb


# ---- bounds -----------------------------------------------------------------------------------------------------------------
def step_125(measured):
    """10 x measured, rounded up to the next 1-2-5 step, never below 16 x 2^-52"""
    target = 10.0 * float(measured)
    if target <= FLOOR:
        return FLOOR
    k = int(np.floor(np.log10(target)))
    for m, e in ((1, k), (2, k), (5, k), (1, k + 1)):
        if float(f"{m}e{e}") >= target * (1 - 1e-9):           # 10 x 1e-15 is 1e-14, whatever the product rounds to
            return float(f"{m}e{e}")
    raise AssertionError(measured)


def bounds():
    with open(BOUNDS) as f:
        return json.load(f)


def bound(key):
    return float(bounds()[key][1])


def deviation(actual, ref, scale=None):
    """max |actual - ref| as a fraction of the largest |ref| (or of `scale`), the difference taken in extended precision"""
    actual, ref = np.asarray(actual, dtype=LD), np.asarray(ref, dtype=LD)
    assert actual.shape == ref.shape, (actual.shape, ref.shape)
    sc = float(np.abs(ref).max()) if scale is None else float(scale)
    return float(np.abs(actual - ref).max()) / max(sc, 1e-300)


# ---- extended-precision statements ------------------------------------------------------------------------------------------
def y_nodes(ny):
    return np.linspace(-20, 20, ny).astype(LD)


def trapz(f, y):
    """sum d_j (f_{j+1} + f_j) / 2 along the last axis"""
    d = y[1:] - y[:-1]
    return np.sum(d * (f[..., 1:] + f[..., :-1]) / 2, axis=-1)


def phi(y, eps):
    return np.exp(-(LD(eps) * y) ** 2)


def impedance_trapz(freq, tau, eps, ny):
    """(Z', Z'') [.., nf, ntau] of freq [.., nf]: basis.py:93-95, 565-570"""
    y = y_nodes(ny)
    w = (2 * PI_LD * np.asarray(freq, dtype=LD))[..., :, None, None]
    t = np.asarray(tau, dtype=LD)[:, None]
    den = 1 + np.exp(2 * (y + np.log(w * t)))
    return trapz(phi(y, eps) / den, y), trapz(-phi(y, eps) * np.exp(y) * w * t / den, y)


def impedance_lookup(eps, wt_re, wt_im, ny):
    """generate_impedance_lookup's two tables: omega tau = wt, i.e. 2 pi f = wt and tau = 1"""
    f_re, f_im = np.asarray(wt_re, dtype=LD) / (2 * PI_LD), np.asarray(wt_im, dtype=LD) / (2 * PI_LD)
    return impedance_trapz(f_re, [1.0], eps, ny)[0][:, 0], impedance_trapz(f_im, [1.0], eps, ny)[1][:, 0]


def response_trapz_entry(td_over, eps, ny):
    """int phi(y) (1 - exp(-x / e^y)) dy at x = (t - t_k) / tau"""
    y = y_nodes(ny)
    x = np.asarray(td_over, dtype=LD)[..., None]
    return trapz(phi(y, eps) * (1 - np.exp(-x / np.exp(y))), y)


def response_expdecay_entry(dt, tau, tr, eps, ny):
    """basis.py:619-637: phi(y) (1 - e^{-t/T} + tr / (tr - T) (e^{-t/T} - e^{-t/tr})), T = e^y tau; dt [nt], tau [ntau]"""
    y = y_nodes(ny)
    t = np.asarray(dt, dtype=LD)[:, None, None]
    T = np.exp(y) * np.asarray(tau, dtype=LD)[None, :, None]
    tr = LD(tr)
    eT = np.exp(-t / T)
    return trapz(phi(y, eps) * ((1 - eT) + (tr / (tr - T)) * (eT - np.exp(-t / tr))), y)


def layered_response(times, step_times, step_sizes, entry, ntau, inclusive=False):
    """rows after a step (t > t_k; t >= t_k for the potentiostatic form) hold entry(t - t_k) * size_k, earlier rows 0 exactly;
    entry maps dt [n] to [n, ntau].  Returns (sum over the steps in order, layers)"""
    times = np.asarray(times, dtype=LD)
    lay = []
    for st, sa in zip(step_times, step_sizes):
        after = times >= LD(st) if inclusive else times > LD(st)
        layer = np.zeros((times.size, ntau), dtype=LD)
        if after.any():
            layer[after] = entry(times[after] - LD(st)) * LD(sa)
        lay.append(layer)
    lay = np.array(lay)
    total = np.zeros_like(lay[0])
    for layer in lay:
        total = total + layer
    return total, lay


def response_trapz(times, tau, step_times, step_sizes, eps, ny):
    tau = np.asarray(tau, dtype=LD)
    return layered_response(times, step_times, step_sizes, lambda dt: response_trapz_entry(dt[:, None] / tau[None, :], eps, ny), tau.size)


def response_expdecay(times, tau, step_times, step_sizes, tau_rise, eps, ny):
    times = np.asarray(times, dtype=LD)
    lay = []
    for st, sa, tr in zip(step_times, step_sizes, tau_rise):
        layer = np.zeros((times.size, len(tau)), dtype=LD)
        after = times > LD(st)
        if after.any():
            layer[after] = response_expdecay_entry(times[after] - LD(st), tau, tr, eps, ny) * LD(sa)
        lay.append(layer)
    lay = np.array(lay)
    total = np.zeros_like(lay[0])
    for layer in lay:
        total = total + layer
    return total, lay


def response_pot(times, tau, step_times, step_sizes):
    tau = np.asarray(tau, dtype=LD)
    return layered_response(times, step_times, step_sizes, lambda dt: np.exp(-dt[:, None] / tau[None, :]), tau.size, inclusive=True)


def interp(x, xp, fp):
    """np.interp(x, xp, fp) in extended precision: table ends beyond the knots, the knot's own value on a knot, else
    slope * (x - xp[j]) + fp[j] un-fused"""
    x, xp, fp = np.asarray(x, dtype=LD), np.asarray(xp, dtype=LD), np.asarray(fp, dtype=LD)
    ng = xp.size
    j = np.clip(np.searchsorted(xp, x, side="right") - 1, 0, ng - 2)
    slope = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j])
    out = slope * (x - xp[j]) + fp[j]
    out = np.where(x == xp[j], fp[j], out)
    out = np.where(x >= xp[-1], fp[-1], out)
    return np.where(x < xp[0], fp[0], out)


def impedance_interp(freq, tau, tables):
    """np.interp(ln(omega tau)) on the (Z', Z'') tables; freq [.., nf] -> two [.., nf, ntau]"""
    x = np.log((2 * PI_LD * np.asarray(freq, dtype=LD))[..., :, None] * np.asarray(tau, dtype=LD))
    return interp(x, *tables[0]), interp(x, *tables[1])


def impedance_interp_f64(freq, tau, tables):
    """the oracle's row, construct_impedance_matrix without its Toeplitz detection: np.interp(np.log(w_n * tau))"""
    x = np.log((np.asarray(freq, dtype=float) * 2 * np.pi)[..., :, None] * np.asarray(tau, dtype=float))
    return np.interp(x, *tables[0]), np.interp(x, *tables[1])


def response_interp(times, tau, step_times, step_sizes, table):
    tau = np.asarray(tau, dtype=LD)
    return layered_response(times, step_times, step_sizes, lambda dt: interp(np.log(dt[:, None] / tau[None, :]), *table), tau.size)


def toeplitz_of(c, r):
    """scipy.linalg.toeplitz(c, r): A[i][j] = c[i - j] (i >= j) else r[j - i]"""
    c, r = np.asarray(c), np.asarray(r)
    i, j = np.arange(c.size)[:, None], np.arange(r.size)[None, :]
    return np.where(i >= j, c[np.maximum(i - j, 0)], r[np.maximum(j - i, 0)])


def penalty_matrices(ln_tau, eps, toeplitz, dtype=LD):
    """basis.py:382-395; the Toeplitz form evaluates c[d] = func(x_d, x_0) and mirrors it (mat1d.py:125-209).  dtype=float is
    the plain numpy statement (the oracle's construct_integrated_derivative_matrix picks the form by itself)"""
    x = np.asarray(ln_tau, dtype=dtype)
    eps = dtype(eps)
    n = x.size
    if toeplitz:
        d = np.abs(np.arange(n)[:, None] - np.arange(n)[None, :])
        a = eps * (x[0] - x[d])
    else:
        a = eps * (x[None, :] - x[:, None])
    pi = PI_LD if dtype is LD else np.pi
    rpi, e = np.sqrt(pi / 2), np.exp(-(a ** 2 / 2))
    return rpi / eps * e, -rpi * eps * (a ** 2 - 1) * e, rpi * eps ** 3 * (3 - 6 * a ** 2 + a ** 4) * e


def eis_var(freq, ve, cor, uniform=False):
    lf = np.log(np.asarray(freq, dtype=LD))
    main = np.ones((lf.size, lf.size), dtype=LD) if uniform else np.exp(-(LD(ve) * (lf[:, None] - lf[None, :])) ** 2)
    vmm = np.block([[main, main * LD(cor)], [main * LD(cor), main]])
    return vmm / np.sum(vmm, axis=1)[:, None]


def chrono_var(tt, seg, eps, uniform=False, dtype=LD):
    """Gaussian in transformed time inside a segment [seg[k], seg[k+1]), exact zeros across segments, rows normalised"""
    tt = np.asarray(tt, dtype=dtype)
    if uniform:
        vmm = np.ones((tt.size, tt.size), dtype=dtype)
    else:
        vmm = np.zeros((tt.size, tt.size), dtype=dtype)
        for a, b in zip(seg[:-1], seg[1:]):
            vmm[a:b, a:b] = np.exp(-(dtype(eps) * (tt[a:b, None] - tt[None, a:b])) ** 2)
    return vmm / np.sum(vmm, axis=1)[:, None]


def func_eval(basis, ev, eps, order, dtype=LD):
    """basis.py:488-514, 218-228: phi^(order)(e_i - b_j) of the gaussian basis"""
    y = np.asarray(ev, dtype=dtype)[:, None] - np.asarray(basis, dtype=dtype)[None, :]
    eps = dtype(eps)
    p = np.exp(-(eps * y) ** 2)
    if order == 0:
        return p
    if order == 1:
        return (-2 * eps ** 2 * y) * p
    return (-2 * eps ** 2 + 4 * eps ** 4 * y ** 2) * p


# ---- inputs -----------------------------------------------------------------------------------------------------------------
def rng_of(*key):
    return np.random.default_rng([17, *[int(k) for k in key]])


def tau_grid(ntau):
    return np.logspace(-6, 2, ntau) if ntau > 1 else np.array([1e-3])


def freq_grid(B, nf, key=0, lo=-3, hi=7):
    """per-spectrum frequencies [B, nf], descending; by default ln(omega tau) of tau_grid runs from far below to far above the lookups"""
    f = np.sort(10 ** rng_of(1, B, nf, key).uniform(lo, hi, size=(B, nf)), axis=1)[:, ::-1]
    return np.ascontiguousarray(f)


def default_tables(eps=EPS_DEFAULT):
    """the default 2000-knot lookups (float64 oracle: values of the tables are inputs of the interp build)"""
    from oracle import drt_oracle as orc
    return orc.generate_impedance_lookup(eps)


def jittered_table(ng, lim, key, zero_knot=False):
    """an increasing table visibly off the uniform grid (the arithmetic bin is then off and the search runs)"""
    rng = rng_of(2, ng, key)
    x = np.linspace(-lim, lim, ng)
    if ng > 2:
        x[1:-1] += rng.uniform(-0.45, 0.45, ng - 2) * (x[1] - x[0])
    if zero_knot:
        x[np.argmin(np.abs(x))] = 0.0
        assert np.all(np.diff(x) > 0)
    return x, np.cumsum(rng.standard_normal(ng)) * 0.01 + np.sin(x)


def toeplitz_grids(nf, ntau, offset=2):
    """a log-uniform frequency grid and a tau grid on the same 10 points per decade: omega_i tau_j depends on j - i alone"""
    k = np.arange(max(nf, ntau) + offset)
    freq = 10.0 ** (4 - k[:nf] / 10)
    tau = (1 / (2 * np.pi * freq[0])) * 10.0 ** ((k[:ntau] - offset) / 10)
    return freq, tau


# ---- cases ------------------------------------------------------------------------------------------------------------------
# 1. the general interp build.  (B, nf, ntau): every rows-per-workgroup value; at rpb 8 and 16 the threads-per-row count is chosen
# so that a thread steps by less than the workgroup's rows (rp < rpb), i.e. the two-row loop makes a pass at every rpb >= 8
GEOMETRY_BATCHED = {
    4: [(1, 9, 5)],
    8: [(32, 250, 2), (512, 9, 257)],
    16: [(64, 245, 5), (512, 17, 129)],
    32: [(128, 230, 1)],
    64: [(256, 200, 2)],
    128: [(512, 200, 1)],
    256: [(1024, 1, 5), (512, 300, 2)],
}
GEOMETRY_NTAU = (127, 128, 129, 1023, 1025, 2047, 2048, 2049, 2051)
GEOMETRY_NF = ((1, 1), (3, 3), (4, 1), (5, 3), (6, 1), (37, 4))      # (nf, B) at B <= 4


def geometry_cases():
    out = [(B, nf, ntau) for shapes in GEOMETRY_BATCHED.values() for (B, nf, ntau) in shapes]
    return out + [(B, nf, ntau) for ntau in GEOMETRY_NTAU for (nf, B) in GEOMETRY_NF]


# 2. lookups at the LDS edge: (ngrid, B, nf, ntau)
def lds_edge_cases():
    return [(ng, B, nf, 3) for ng in (3400, INTERP_NGRID_MAX - 1, INTERP_NGRID_MAX) for (B, nf) in ((1, 5), (1024, 1))]


JITTERED_CASES = [(1999, 1024, 1, 3), (1999, 1, 5, 3)]      # the irregular tables at rpb = 256 and at rpb = 4


def jittered_tables(ng):
    """different abscissae for Z' and Z'' (two bin searches), as in the irregular-table test of test_gpu_matrices.py"""
    return jittered_table(ng, 6.2, 0), jittered_table(ng, 12.4, 1)


# 3. the trapezoid family
NY = (2, 3, 64, 65, 66, 129, 1000, 2731, 6000)
TRAPZ_SHAPES = ((1, 1, 1), (3, 15, 1), (1, 16, 3), (3, 17, 3), (1, 33, 1))            # (nf, ntau, B)
TOEPLITZ_TRAPZ_SHAPES = ((1, 1), (5, 3), (3, 5), (4, 4))
LOOKUP_NGRID = (2, 3, 5)
RESPONSE_SHAPES = ((1, 1, 1), (7, 15, 3), (7, 16, 1), (1, 17, 3), (7, 33, 3))          # (nt, ntau, nsteps)


def eps_of(ny):
    """at ny <= 3 the default basis underflows phi at every node but the middle one: a wide basis keeps the case from being zeros"""
    return 0.5 if ny <= 3 else EPS_DEFAULT


def trapz_cases():
    """(ny, nf, ntau, B): every shape at ny = 65, one shape (in turn) at every other ny"""
    out = [(65, *s) for s in TRAPZ_SHAPES]
    return out + [(ny, *TRAPZ_SHAPES[i % len(TRAPZ_SHAPES)]) for i, ny in enumerate(NY) if ny != 65]


def trapz_freq(B, nf, ny):
    return freq_grid(B, nf, ny, lo=-1, hi=4)


def toeplitz_trapz_cases():
    out = [(65, *s) for s in TOEPLITZ_TRAPZ_SHAPES]
    return out + [(ny, *TOEPLITZ_TRAPZ_SHAPES[(i + 1) % 4]) for i, ny in enumerate(NY) if ny != 65]


def response_cases():
    out = [(65, *s) for s in RESPONSE_SHAPES]
    return out + [(ny, *RESPONSE_SHAPES[(i + 2) % len(RESPONSE_SHAPES)]) for i, ny in enumerate(NY) if ny != 65]


def response_inputs(nt, nsteps):
    """dyadic times (t - t_k is exact): one sample before the first step and one exactly at a step time when nt allows"""
    step_times = np.array([0.0, 0.5, 1.0])[:nsteps]
    step_sizes = np.array([1e-3, -2e-3, 1.5e-3])[:nsteps]
    tau_rise = np.array([1.3e-3, 3.1e-3, 2.3e-4])[:nsteps]      # off the tau grids: tau_rise - e^y tau has no exact zero
    times = np.array([1.75]) if nt == 1 else np.array([-0.125, 0.0, 0.015625, 0.25, 0.5, 0.75, 1.75])[:nt]
    return times, step_times, step_sizes, tau_rise


# 4. the Toeplitz interp build: (nf, ntau) and copies B; np_interp through the response build
TOEPLITZ_SHAPES = ((7, 3), (3, 7), (1, 1), (71, 91))
TOEPLITZ_B = (1, 64, 65, 130)
NP_INTERP_NTAU = (255, 256, 257)
NP_INTERP_NT = (1, 2, 33)


RESPONSE_EDGE_NGRID = (6400, RESPONSE_NGRID_MAX)


def np_interp_cases():
    """(ngrid, nt, ntau): the jittered 1999-knot table at every shape, the longest tables the LDS holds at one"""
    return [(1999, nt, ntau) for ntau in NP_INTERP_NTAU for nt in NP_INTERP_NT] + [(ng, 33, 257) for ng in RESPONSE_EDGE_NGRID]


def response_table(ng):
    return jittered_table(ng, 9.0, 2, zero_knot=True)


def np_interp_inputs(nt, ntau):
    """one unit step at 0, tau with an exact 1.0 among them and a time of exactly 1.0: ln(1 / 1) is the table's zero knot on any
    libm; the first and last tau send ln(t / tau) beyond both table ends"""
    tau = np.logspace(-9, 9, ntau)
    tau[ntau // 2] = 1.0
    times = np.array([1.0, 0.37, *np.logspace(-3, 2, 31)])[:nt]
    return times, tau


# 5. variance matrices
EIS_VAR_NF = (1, 2, 127, 128, 129, 300)
CHRONO_VAR = {1: [(0, 1)], 255: [(0, 255), (0, 100, 101, 255)], 256: [(0, 256), (0, 1, 255, 256)],
              257: [(0, 257), (0, 1, 256, 257)], 600: [(0, 600), (0, 256, 257, 600)]}


def chrono_tt(nt):
    return np.cumsum(rng_of(5, nt).uniform(0.05, 0.6, nt))


# 6. penalties, 8. func_eval
PENALTY_N = (1, 2, 255, 256, 257)
PENALTY_EPS = 2.3
FUNC_EVAL_NB, FUNC_EVAL_NE = (63, 64, 65), (3, 4, 5)


def uniform_ln_tau(n):
    return np.linspace(-14.0, 5.0, n) if n > 1 else np.array([-3.0])


# 7. phasance: the inputs tools/make_phasor_edges_golden.py evaluates with mpmath
PHASOR_EPS = (0.5, 2.0, 8.0)
PHASOR_NNU = (1, 63, 64, 65)


def phasor_cases():
    """name -> dict(freq, nu, eps, times, step_times, step_sizes); nu = 0 and nu = 1 among the columns (nnu = 1: nu = 1), the
    frequency 1 / (2 pi) in every case, dyadic times"""
    out = {}
    for ie, eps in enumerate(PHASOR_EPS):
        for iu, nnu in enumerate(PHASOR_NNU):
            nu = np.linspace(-1.0, 1.0, nnu) if nnu > 1 else np.array([1.0])
            if nnu == 64:
                nu[20] = 0.0
            three = (ie + iu) % 2 == 0
            freq = np.array([F_UNIT_OMEGA, 10.0, 0.02]) if three else np.array([F_UNIT_OMEGA])
            times = np.array([-0.125, 0.5, 1.75]) if three else np.array([1.75])
            nsteps = 3 if iu % 2 else 1
            out[f"eps{eps:g}_nnu{nnu}"] = dict(freq=freq, nu=nu, eps=eps, times=times, step_times=np.array([0.0, 0.5, 1.0])[:nsteps],
                                               step_sizes=np.array([1e-3, -2e-3, 1.5e-3])[:nsteps])
    return out


# 9. long dimensions
LONG_NT = 65539


def long_inputs():
    """(times, tau, step_times, step_sizes): one unit step at 0, one tau, more samples than a grid's y dimension holds"""
    return np.linspace(1e-3, 2.0, LONG_NT), np.array([0.7]), [0.0], [1.0]


# ---- the float64 oracle's deviation from the statements: what the bounds table records -----------------------------------------
def measure_bounds():
    """quantity -> deviation of the float64 oracle from the extended-precision statement, on the GPU cases' inputs"""
    from oracle import drt_oracle as orc
    m = {}

    def note(key, got, ref, scale=None):
        m[key] = max(m.get(key, 0.0), deviation(got, ref, scale))

    # interp builds: the general build (default and jittered tables, tables at the LDS edge) and the Toeplitz build
    tables = default_tables()
    for (B, nf, ntau) in [(1, 9, 5), (3, 37, 129), (4, 5, 2051)]:
        freq, tau = freq_grid(B, nf), tau_grid(ntau)
        for got, ref in zip(impedance_interp_f64(freq, tau, tables), impedance_interp(freq, tau, tables)):
            note("interp_general", got, ref)
    for (ng, B, nf, ntau) in lds_edge_cases() + JITTERED_CASES:
        tabs, freq, tau = jittered_tables(ng), freq_grid(B, nf, ng), tau_grid(ntau)
        for got, ref in zip(impedance_interp_f64(freq, tau, tabs), impedance_interp(freq, tau, tabs)):
            note("interp_general", got, ref)
    for (nf, ntau) in TOEPLITZ_SHAPES:
        freq, tau = toeplitz_grids(nf, ntau)
        for got, ref in zip(impedance_interp_f64(freq, tau, tables), impedance_interp(freq, tau, tables)):
            note("interp_toeplitz", got, ref)
    for (ng, nt, ntau) in np_interp_cases():
        table = response_table(ng)
        times, tau = np_interp_inputs(nt, ntau)
        got, _ = orc.construct_response_matrix(tau, times, [0.0], [1.0], 1.0, 'interp', interpolate_grids=table)
        note("response_interp", got, response_interp(times, tau, [0.0], [1.0], table)[0])
    # the trapezoid family
    for ny in NY:
        eps, y = eps_of(ny), np.linspace(-20, 20, ny)
        for ng in LOOKUP_NGRID:
            wt_re, wt_im = np.logspace(-2.7, 2.7, ng), np.logspace(-5.4, 5.4, ng)
            ref = impedance_lookup(eps, wt_re, wt_im, ny)
            note("lookup_trapz", [np.trapezoid(orc.z_re_integrand(y, w, 1, eps), x=y) for w in wt_re], ref[0])
            note("lookup_trapz", [np.trapezoid(orc.z_im_integrand(y, w, 1, eps), x=y) for w in wt_im], ref[1])
            td = np.logspace(-6, 2, ng)
            note("response_lookup", [np.trapezoid(orc.response_integrand(y, 1, t, eps), x=y) for t in td],
                 response_trapz_entry(td, eps, ny))
    for (ny, nf, ntau, B) in trapz_cases():
        eps, y = eps_of(ny), np.linspace(-20, 20, ny)
        freq, tau = trapz_freq(B, nf, ny), tau_grid(ntau)
        ref = impedance_trapz(freq, tau, eps, ny)
        for part, func in enumerate((orc.z_re_integrand, orc.z_im_integrand)):
            got = [[[np.trapezoid(func(y, w, t, eps), x=y) for t in tau] for w in 2 * np.pi * f] for f in freq]
            note("impedance_trapz", got, ref[part])
    for (ny, nf, ntau) in toeplitz_trapz_cases():
        eps, y = eps_of(ny), np.linspace(-20, 20, ny)
        freq, tau = toeplitz_grids(nf, ntau)
        ref = impedance_trapz(freq, tau, eps, ny)
        for part, func in enumerate((orc.z_re_integrand, orc.z_im_integrand)):
            got = [[np.trapezoid(func(y, w, t, eps), x=y) for t in tau] for w in 2 * np.pi * freq]
            note("impedance_trapz", got, ref[part])
    for (ny, nt, ntau, nsteps) in response_cases():
        eps, y = eps_of(ny), np.linspace(-20, 20, ny)
        times, st, sz, tr = response_inputs(nt, nsteps)
        tau = tau_grid(ntau)
        got, lay = orc.construct_response_matrix(tau, times, st, sz, eps, 'trapz', integrate_points=ny)
        ref, ref_lay = response_trapz(times, tau, st, sz, eps, ny)
        note("response_trapz", got, ref, scale=np.abs(ref_lay).max())      # the sum over the steps, against its layers' size
        note("response_trapz", lay, ref_lay)
        ref, ref_lay = response_expdecay(times, tau, st, sz, tr, eps, ny)
        lay = np.zeros(ref_lay.shape)
        for k in range(nsteps):                        # plain numpy: the oracle has no expdecay step model
            for i, t in enumerate(times):
                if t > st[k]:
                    T = np.exp(y)[None, :] * tau[:, None]
                    eT = np.exp(-(t - st[k]) / T)
                    f = orc.phi_gaussian(y, eps) * ((1 - eT) + (tr[k] / (tr[k] - T)) * (eT - np.exp(-(t - st[k]) / tr[k])))
                    lay[k, i] = np.trapezoid(f, x=y, axis=-1) * sz[k]
        note("response_expdecay", lay.sum(axis=0), ref, scale=np.abs(ref_lay).max())
        note("response_expdecay", lay, ref_lay)
        ref, ref_lay = response_pot(times, tau, st, sz)
        lay = pot_f64(times, tau, st, sz)
        note("response_pot", lay.sum(axis=0), ref, scale=np.abs(ref_lay).max())
        note("response_pot", lay, ref_lay)
    times, tau, st, sz = long_inputs()                 # the potentiostatic form over a long record
    note("response_pot", pot_f64(times, tau, st, sz)[0], response_pot(times, tau, st, sz)[0])
    # variance matrices
    for nf in EIS_VAR_NF:
        freq = freq_grid(1, nf, 5)[0]
        for uniform in (False, True):
            got = orc.construct_eis_var_matrix(freq, 0.25, 0.25, 'uniform' if uniform else None)
            note("eis_var", got, eis_var(freq, 0.25, 0.25, uniform))
            note("row_sum", got.sum(axis=1), np.ones(2 * nf))
    for nt, segs in CHRONO_VAR.items():
        tt = chrono_tt(nt)
        for seg in segs:
            got = chrono_var(tt, seg, 0.25, dtype=np.float64)
            note("chrono_var", got, chrono_var(tt, seg, 0.25))
            note("row_sum", got.sum(axis=1), np.ones(nt))
    # penalties (order 2 cancels near its roots: scale eps^3, as order 1 has eps and order 0 1 / eps up to sqrt(pi / 2))
    for n in PENALTY_N:
        x = uniform_ln_tau(n)
        for toeplitz in (True, False):
            ref = penalty_matrices(x, PENALTY_EPS, toeplitz)
            got = penalty_matrices(x, PENALTY_EPS, toeplitz, dtype=np.float64)
            for k in range(3):
                note(f"penalty{k}", got[k], ref[k], scale=penalty_scale(k, PENALTY_EPS))
        for k in range(3 if n > 1 else 0):
            note(f"penalty{k}", orc.construct_integrated_derivative_matrix(x, k, PENALTY_EPS),
                 penalty_matrices(x, PENALTY_EPS, True)[k], scale=penalty_scale(k, PENALTY_EPS))
    for nb in FUNC_EVAL_NB:
        for ne in FUNC_EVAL_NE:
            basis, ev = uniform_ln_tau(nb), np.sort(rng_of(8, nb, ne).uniform(-15, 6, ne))
            for order in range(3):
                note(f"func_eval{order}", func_eval(basis, ev, 1.7, order, dtype=np.float64), func_eval(basis, ev, 1.7, order))
    if os.path.exists(PHASOR_GOLDEN):
        G = np.load(PHASOR_GOLDEN)
        for name, c in phasor_cases().items():
            zm = orc.construct_phasor_z_matrix(c["freq"], c["nu"], c["eps"])
            ref = G[f"{name}.zm_re"] + 1j * G[f"{name}.zm_im"]
            # one bound per case: where the difference of the two erf values cancels (eps = 0.5 away from omega = 1) scipy's erf
            # keeps nine digits, elsewhere fifteen -- one bound for all would hide a complex erf that is wrong at 1e-10
            m[f"phasor_z.{name}"] = float(np.abs(zm - ref).max() / np.abs(ref).max())
            vm, vlay = orc.construct_phasor_v_matrix(c["times"], c["nu"], c["eps"], c["step_times"], c["step_sizes"])
            note(f"phasor_v.{name}", vm, G[f"{name}.vm"], scale=np.abs(G[f"{name}.vlay"]).max())
            note(f"phasor_v.{name}", vlay, G[f"{name}.vlay"])
    return m


def pot_f64(times, tau, step_times, step_sizes):
    """plain numpy (mat1d.py:114-118): exp(-(t - t_k) / tau) size_k from the step on, 0 before; layers [nsteps][nt][ntau]"""
    with np.errstate(over="ignore"):
        return np.array([np.where((times >= s)[:, None], np.exp(-(times - s)[:, None] / np.asarray(tau)[None, :]) * a, 0.0)
                         for s, a in zip(step_times, step_sizes)])


def penalty_scale(order, eps):
    return float(np.sqrt(np.pi / 2)) * (1 / eps, eps, 3 * eps ** 3)[order]


def bounds_table():
    return {k: [float(f"{v:.3e}"), step_125(float(f"{v:.3e}"))] for k, v in sorted(measure_bounds().items())}
