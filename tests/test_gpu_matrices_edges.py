"""The matrix builders of csrc/matrices.hip at their launch edges, through the C-ABI entry points (ctx.*, so that the test and not
mat1d picks the form): every rows-per-workgroup and threads-per-row value of the general interp build and its two-row loop, lookups
at the LDS limit, the trapezoid family from ny = 2 to the accepted maximum, the Toeplitz build's copies, np_interp on irregular
tables, block-stride loops that wrap, and rows beyond what a grid's y dimension holds.

References are the extended-precision statements of tests/matrices_edges_util.py (mpmath for the phasance columns:
tests/golden/phasor_edges_mp.npz), bounds come from tests/matrices_edges_bounds.json -- ten times what the float64 oracle itself
deviates from those statements on the same inputs, never a figure from the device.  Where an entry's arithmetic cannot depend on
the launch the check is bitwise and needs no bound."""
import numpy as np
import pytest

import matrices_edges_util as mu
from conftest import parity_close

pytestmark = pytest.mark.gpu

LD = np.longdouble
TRAPZ, INTERP = 1, 0


@pytest.fixture(scope="module")
def ctx():
    from hipdrt import _ffi
    return _ffi.get_context(0)


@pytest.fixture(scope="module")
def tables():
    return mu.default_tables()


@pytest.fixture(scope="module")
def golden():
    return np.load(mu.PHASOR_GOLDEN)


def check(key, got, ref, scale=None):
    """deviation from the statement as a fraction of its largest entry, at the table's bound for this quantity"""
    return parity_close(f"matrices_edges:{key}", got, np.asarray(ref, dtype=float), mu.bound(key), scale=scale)


def same(a, b):
    return a.shape == b.shape and np.array_equal(a, b)


def refused(ctx_call):
    """the library's own refusal (HIPDRT_E_INVALID, before any launch) -- not a HIP launch error, whose text may say the same words"""
    from hipdrt import _ffi
    with pytest.raises(_ffi.HipDrtError, match=r"hipdrt error -1: invalid argument: "):
        ctx_call()


def reference_build(ctx, freq, tau, lookups):
    """every spectrum's rows built as B = 1 grids of at most REF_ROWS rows and REF_COLS columns: rpb = 4, tpr = 64 -- one row per
    thread and pass, no second row in flight, no column wrap (test_matrices_edges_util.py pins that)"""
    rows = np.ascontiguousarray(np.asarray(freq, dtype=float).reshape(-1))
    re, im = np.empty((rows.size, tau.size)), np.empty((rows.size, tau.size))
    for r0 in range(0, rows.size, mu.REF_ROWS):
        for c0 in range(0, tau.size, mu.REF_COLS):
            a, b = ctx.impedance_matrix(rows[r0:r0 + mu.REF_ROWS], tau[c0:c0 + mu.REF_COLS], 1.0, INTERP, False, lookups)
            re[r0:r0 + mu.REF_ROWS, c0:c0 + mu.REF_COLS], im[r0:r0 + mu.REF_ROWS, c0:c0 + mu.REF_COLS] = a, b
    shape = np.shape(freq) + (tau.size,)
    return re.reshape(shape), im.reshape(shape)


# ---- 1. general interp build: launch geometry, bit for bit ---------------------------------------------------------------------
def test_interp_form_is_the_utils(ctx):
    """the launcher's rule read back: a change of tpr, rpb or the LDS bytes without tests/matrices_edges_util.py fails here"""
    for (B, nf, ntau) in mu.geometry_cases():
        f = mu.interp_form(B, nf, ntau)
        assert ctx.debug_impedance_interp_form(B, nf, ntau, 2000) == (f["tpr"], f["rpb"], f["lds"]), (B, nf, ntau)
    for (ng, B, nf, ntau) in mu.lds_edge_cases() + mu.JITTERED_CASES:
        f = mu.interp_form(B, nf, ntau, ng)
        assert ctx.debug_impedance_interp_form(B, nf, ntau, ng) == (f["tpr"], f["rpb"], f["lds"]), (ng, B)
        assert f["lds"] <= mu.LDS_LIMIT
    # the default tables keep the form they always had
    assert ctx.debug_impedance_interp_form(1, 256, 512, 2000) == (256, 4, 96032)
    assert ctx.debug_impedance_interp_form(4096, 71, 91, 2000) == (64, 256, 98048)
    refused(lambda: ctx.debug_impedance_interp_form(1, 1, 1, mu.INTERP_NGRID_MAX + 1))


def batched_equals_reference(ctx, tables, B, nf, ntau, key=0):
    freq, tau = mu.freq_grid(B, nf, key), mu.tau_grid(ntau)
    re, im = ctx.impedance_matrix(freq, tau, 1.0, INTERP, False, tables)
    ref_re, ref_im = reference_build(ctx, freq, tau, tables)
    assert re.shape == (B, nf, ntau)
    bad = np.argwhere((re != ref_re) | (im != ref_im))
    assert bad.size == 0, f"(B, nf, ntau) = {(B, nf, ntau)}, form {mu.interp_form(B, nf, ntau)}: {len(bad)} entries differ, first (b, row, column) {bad[0]}"
    return freq, tau, re, im


@pytest.mark.parametrize("rpb", sorted(mu.GEOMETRY_BATCHED))
def test_interp_rows_per_block(ctx, tables, rpb):
    """every spectrum of a batched build equals, bit for bit, the build of its own frequencies alone at rpb = 4"""
    for (B, nf, ntau) in mu.GEOMETRY_BATCHED[rpb]:
        assert ctx.debug_impedance_interp_form(B, nf, ntau, 2000)[1] == rpb
        batched_equals_reference(ctx, tables, B, nf, ntau)


@pytest.mark.parametrize("ntau", mu.GEOMETRY_NTAU)
def test_interp_threads_per_row_and_column_wrap(ctx, tables, ntau):
    """tpr 64 .. 1024, the two-row loop at every remainder of a workgroup's rows, the column wrap from ntau = 2049 on: each column
    block equals the same tau values built as a short matrix"""
    for (nf, B) in mu.GEOMETRY_NF:
        batched_equals_reference(ctx, tables, B, nf, ntau)


def test_interp_general_against_the_extended_precision_statement(ctx, tables):
    clamped = 0
    for (B, nf, ntau) in [(1, 9, 5), (3, 37, 129), (4, 5, 2051)]:
        freq, tau = mu.freq_grid(B, nf), mu.tau_grid(ntau)
        got = ctx.impedance_matrix(freq, tau, 1.0, INTERP, False, tables)
        x = np.log(2 * np.pi * freq)[..., None] + np.log(tau)
        for g, ref, (xp, fp) in zip(got, mu.impedance_interp(freq, tau, tables), tables):
            check("interp_general", g, ref)
            g = g.reshape(x.shape)
            below, above = x < xp[0] - 1e-9, x > xp[-1] + 1e-9
            assert np.all(g[below] == fp[0]) and np.all(g[above] == fp[-1])      # table ends: copies
            clamped += min(below.sum(), above.sum())
    assert clamped > 100


# ---- 2. lookups at the LDS edge --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ng,B,nf,ntau", mu.lds_edge_cases() + mu.JITTERED_CASES)
def test_interp_lookups_at_the_lds_edge(ctx, ng, B, nf, ntau):
    """the longest accepted tables build at every batch size (the launcher gives up rows per workgroup for them), irregular knots,
    different abscissae for Z' and Z''; (3400, 1024, 1, 3) asked for 165 248 bytes of LDS before the launcher did that"""
    tabs, freq, tau = mu.jittered_tables(ng), mu.freq_grid(B, nf, ng), mu.tau_grid(ntau)
    got = ctx.impedance_matrix(freq, tau, 1.0, INTERP, False, tabs)
    ref = mu.impedance_interp(freq, tau, tabs)
    ref_re, ref_im = reference_build(ctx, freq, tau, tabs)
    for g, r, r4 in zip(got, ref, (ref_re, ref_im)):
        check("interp_general", g, r)
        assert same(g, r4)
    x = np.log(2 * np.pi * freq)[..., None] + np.log(tau)
    assert (x < tabs[0][0][0] - 1).any() and (x > tabs[0][0][-1] + 1).any()


@pytest.mark.parametrize("B,nf", [(1, 5), (1024, 1)])
def test_interp_lookup_beyond_the_lds_is_refused(ctx, B, nf):
    ng = mu.INTERP_NGRID_MAX + 1
    refused(lambda: ctx.impedance_matrix(mu.freq_grid(B, nf, ng), mu.tau_grid(3), 1.0, INTERP, False, mu.jittered_tables(ng)))


# ---- 4b. np_interp, the searching form, through the response build (and 2: its lookup at the LDS edge) ---------------------------
@pytest.mark.parametrize("ng,nt,ntau", mu.np_interp_cases())
def test_np_interp_on_irregular_tables(ctx, ng, nt, ntau):
    table = mu.response_table(ng)
    times, tau = mu.np_interp_inputs(nt, ntau)
    a, lay = ctx.response_matrix(times, tau, [0.0], [1.0], 1.0, INTERP, table)
    ref, _ = mu.response_interp(times, tau, [0.0], [1.0], table)
    check("response_interp", a, ref)
    assert same(a, lay[0])
    x = np.log(times[:, None] / tau[None, :])
    xp, fp = table
    assert same(a[x < xp[0] - 1e-9], np.full((x < xp[0] - 1e-9).sum(), fp[0])) and (x < xp[0] - 1e-9).any()      # table ends: copies
    assert same(a[x > xp[-1] + 1e-9], np.full((x > xp[-1] + 1e-9).sum(), fp[-1])) and (x > xp[-1] + 1e-9).any()
    assert same(a[x == 0.0], np.full((x == 0.0).sum(), fp[xp == 0.0][0])) and (x == 0.0).any()                    # on a knot: its value


def test_response_lookup_beyond_the_lds_is_refused(ctx):
    times, tau = mu.np_interp_inputs(2, 3)
    refused(lambda: ctx.response_matrix(times, tau, [0.0], [1.0], 1.0, INTERP, mu.response_table(mu.RESPONSE_NGRID_MAX + 1)))


# ---- 3. the trapezoid family -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ny", mu.NY)
def test_trapz_lookups(ctx, ny):
    eps = mu.eps_of(ny)
    for ng in mu.LOOKUP_NGRID:          # ng = 3, 5: the Z' and Z'' wavefronts share a workgroup
        wt_re, wt_im = np.logspace(-2.7, 2.7, ng), np.logspace(-5.4, 5.4, ng)
        ref = mu.impedance_lookup(eps, wt_re, wt_im, ny)
        for g, r in zip(ctx.impedance_lookup(eps, wt_re, wt_im, ny), ref):
            check("lookup_trapz", g, r)
        td = np.logspace(-6, 2, ng)
        check("response_lookup", ctx.response_lookup(eps, td, ny), mu.response_trapz_entry(td, eps, ny))


@pytest.mark.parametrize("ny,nf,ntau,B", mu.trapz_cases())
def test_trapz_general(ctx, ny, nf, ntau, B):
    eps, freq, tau = mu.eps_of(ny), mu.trapz_freq(B, nf, ny), mu.tau_grid(ntau)
    got = ctx.impedance_matrix(freq if B > 1 else freq[0], tau, eps, TRAPZ, False, ny=ny)
    for g, r in zip(got, mu.impedance_trapz(freq if B > 1 else freq[0], tau, eps, ny)):
        check("impedance_trapz", g, r)
    if B > 1:                            # per-spectrum frequencies: each spectrum is its own build
        for b in range(B):
            alone = ctx.impedance_matrix(freq[b], tau, eps, TRAPZ, False, ny=ny)
            assert same(got[0][b], alone[0]) and same(got[1][b], alone[1])


@pytest.mark.parametrize("ny,nf,ntau", mu.toeplitz_trapz_cases())
def test_trapz_toeplitz(ctx, ny, nf, ntau):
    eps = mu.eps_of(ny)
    freq, tau = mu.toeplitz_grids(nf, ntau)
    got = ctx.impedance_matrix(freq, tau, eps, TRAPZ, True, ny=ny)
    full = ctx.impedance_matrix(freq, tau, eps, TRAPZ, False, ny=ny)
    for g, f, r in zip(got, full, mu.impedance_trapz(freq, tau, eps, ny)):
        assert same(g, mu.toeplitz_of(f[:, 0], f[0, :]))          # the arrangement of the general build's first column and row
        check("impedance_trapz", g, mu.toeplitz_of(r[:, 0], r[0, :]))


@pytest.mark.parametrize("ny,nt,ntau,nsteps", mu.response_cases())
def test_trapz_response_and_expdecay(ctx, ny, nt, ntau, nsteps):
    from hipdrt import _ffi
    eps, tau = mu.eps_of(ny), mu.tau_grid(ntau)
    times, st, sz, tr = mu.response_inputs(nt, nsteps)
    zero = ~(times[None, :] > st[:, None])                    # a sample at or before a step: exactly 0 in that layer
    for key, (a, lay), (ref, ref_lay) in (
            ("response_trapz", ctx.response_matrix(times, tau, st, sz, eps, TRAPZ, ny=ny), mu.response_trapz(times, tau, st, sz, eps, ny)),
            ("response_expdecay", ctx.response_matrix_variant(times, tau, st, sz, _ffi.RESPONSE_EXPDECAY, tr, eps, ny),
             mu.response_expdecay(times, tau, st, sz, tr, eps, ny))):
        assert not lay[zero].any() and (nt == 1 or zero.any())
        check(key, lay, ref_lay)
        check(key, a, ref, scale=float(np.abs(ref_lay).max()))
    a, lay = ctx.response_matrix_variant(times, tau, st, sz, _ffi.RESPONSE_POT)
    ref, ref_lay = mu.response_pot(times, tau, st, sz)
    assert same(lay == 0, np.asarray(ref_lay, dtype=float) == 0)              # the step's own sample counts (t >= t_k)
    check("response_pot", lay, ref_lay)
    check("response_pot", a, ref, scale=float(np.abs(ref_lay).max()))


@pytest.mark.parametrize("nt,ntau,nsteps", [(5, 3, 3), (5, 257, 3)])
def test_interp_response_at_the_step_rule(ctx, nt, ntau, nsteps):
    """the interp build with more than one step, a sample before the first step and one exactly on a step (t > t_k: that sample
    belongs to the layer before); 257 columns: one past a 256-column block"""
    table, tau = mu.response_table(1999), mu.tau_grid(ntau)
    times, st, sz, _ = mu.response_inputs(nt, nsteps)
    a, lay = ctx.response_matrix(times, tau, st, sz, 1.0, INTERP, lookup=table)
    ref, ref_lay = mu.response_interp(times, tau, st, sz, table)
    zero = ~(times[None, :] > st[:, None])
    assert zero.any() and (times[None, :] == st[:, None]).any() and not lay[zero].any()
    assert same(lay == 0, np.asarray(ref_lay, dtype=float) == 0)              # and nowhere else
    check("response_interp", lay, ref_lay)
    check("response_interp", a, ref, scale=float(np.abs(ref_lay).max()))


def test_layered_false_agrees_with_layered_true(ctx):
    """the sum is the same matrix whether or not the layers are kept (the shared step loop's null-pointer branch)"""
    from hipdrt import _ffi
    nt, ntau, nsteps = 5, 3, 3
    tau, table = mu.tau_grid(ntau), mu.response_table(1999)
    times, st, sz, tr = mu.response_inputs(nt, nsteps)
    eps = mu.eps_of(65)
    builds = {
        "interp": lambda layered: ctx.response_matrix(times, tau, st, sz, 1.0, INTERP, lookup=table, layered=layered),
        "trapz": lambda layered: ctx.response_matrix(times, tau, st, sz, eps, TRAPZ, ny=65, layered=layered),
        "expdecay": lambda layered: ctx.response_matrix_variant(times, tau, st, sz, _ffi.RESPONSE_EXPDECAY, tr, eps, 65, layered=layered),
        "pot": lambda layered: ctx.response_matrix_variant(times, tau, st, sz, _ffi.RESPONSE_POT, layered=layered),
    }
    for name, build in builds.items():
        (a, lay), (b, none) = build(True), build(False)
        assert none is None and lay.shape == (nsteps, nt, ntau), name
        assert a.any() and same(a, b), name


def test_trapz_points_beyond_the_maximum_are_refused(ctx):
    from hipdrt import _ffi
    ny, one = mu.NY_MAX + 1, np.array([1.0])
    refused(lambda: ctx.impedance_lookup(1.0, [1.0, 2.0], [1.0, 2.0], ny))
    refused(lambda: ctx.response_lookup(1.0, [1.0, 2.0], ny))
    refused(lambda: ctx.impedance_matrix(one, one, 1.0, TRAPZ, False, ny=ny))
    refused(lambda: ctx.impedance_matrix(one, one, 1.0, TRAPZ, True, ny=ny))
    refused(lambda: ctx.response_matrix(one, one, [0.0], [1.0], 1.0, TRAPZ, ny=ny))
    refused(lambda: ctx.response_matrix_variant(one, one, [0.0], [1.0], _ffi.RESPONSE_EXPDECAY, [1e-3], 1.0, ny))
    refused(lambda: ctx.impedance_lookup(1.0, [1.0, 2.0], [1.0, 2.0], 1))


# ---- 4. the Toeplitz interp build ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf,ntau", mu.TOEPLITZ_SHAPES)
def test_toeplitz_interp_copies(ctx, tables, nf, ntau):
    freq, tau = mu.toeplitz_grids(nf, ntau)
    ref = mu.impedance_interp(freq, tau, tables)
    f64 = mu.impedance_interp_f64(freq, tau, tables)
    general = ctx.impedance_matrix(freq, tau, 1.0, INTERP, False, tables)
    first = None
    for B in mu.TOEPLITZ_B:              # 65 and 130: the b += gridDim.z stride makes a second and a third pass
        got = ctx.impedance_matrix(freq, tau, 1.0, INTERP, True, tables, copies=B)
        assert got[0].shape == (B, nf, ntau)
        for part in range(2):
            assert all(same(got[part][b], got[part][0]) for b in range(1, B)), (B, part)
        first = first or (got[0][0].copy(), got[1][0].copy())
        assert same(got[0][0], first[0]) and same(got[1][0], first[1])
    for t, g, r, o in zip(first, general, ref, f64):
        assert same(t, mu.toeplitz_of(t[:, 0], t[0, :]))
        np.testing.assert_allclose(t, o, rtol=1e-12, atol=1e-300)
        check("interp_toeplitz", t, mu.toeplitz_of(r[:, 0], r[0, :]))
        check("interp_general", g, r)
        # the two builds form ln(omega tau) differently (one log of the product, a sum of two logs): each within its own bound of
        # the statement, so within the sum of the two of each other
        parity_close("matrices_edges:toeplitz_vs_general", t, g, mu.bound("interp_toeplitz") + mu.bound("interp_general"))


# ---- 5. variance matrices --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nf", mu.EIS_VAR_NF)
def test_eis_var_matrix(ctx, nf):
    """2 nf = 258 .. 600 columns: the 256-thread row loop wraps"""
    freq = mu.freq_grid(1, nf, 5)[0]
    for uniform in (False, True):
        got = ctx.eis_var_matrix(freq, 0.25, 0.25, uniform)
        check("eis_var", got, mu.eis_var(freq, 0.25, 0.25, uniform))
        check("row_sum", np.sum(got.astype(LD), axis=1).astype(float), np.ones(2 * nf))


@pytest.mark.parametrize("nt", sorted(mu.CHRONO_VAR))
def test_chrono_var_matrix(ctx, nt):
    tt = mu.chrono_tt(nt)
    for seg in mu.CHRONO_VAR[nt]:
        got = ctx.chrono_var_matrix(tt, seg, 0.25)
        ref = mu.chrono_var(tt, seg, 0.25)
        block = np.zeros((nt, nt), bool)
        for a, b in zip(seg[:-1], seg[1:]):
            block[a:b, a:b] = True
        assert not got[~block].any()                                # exact zeros across segments ...
        assert np.all(got[block & np.asarray(ref > 1e-290)] != 0)   # ... and none inside, short of a double's underflow
        check("chrono_var", got, ref)
        check("row_sum", np.sum(got.astype(LD), axis=1).astype(float), np.ones(nt))
    assert same(ctx.chrono_var_matrix(tt, [0, nt], 0.25, uniform=True), np.full((nt, nt), 1.0) / float(nt))


# ---- 6. penalties ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", mu.PENALTY_N)
def test_penalty_matrices(ctx, n):
    x = mu.uniform_ln_tau(n)
    for toeplitz in (True, False):
        got = ctx.penalty_matrices(x, mu.PENALTY_EPS, toeplitz)
        for k, (g, r) in enumerate(zip(got, mu.penalty_matrices(x, mu.PENALTY_EPS, toeplitz))):
            check(f"penalty{k}", g, r, scale=mu.penalty_scale(k, mu.PENALTY_EPS))      # order 2 cancels near its roots: eps^3 scale
            if toeplitz:
                assert same(g, mu.toeplitz_of(g[:, 0], g[:, 0]))


# ---- 7. phasance -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(mu.phasor_cases()))
def test_phasance_columns(ctx, golden, name):
    """Against mpmath at 40 digits, one bound per case.  The comment on the device's complex erf (A&S 7.1.29) says "absolute error
    ~1e-16".  Measured on an MI355X, whole column (prefactor and the difference of two erf values included) as a fraction of the
    largest entry: 1.3e-16 .. 8.4e-16 in the ten cases without cancellation (eps = 2 and 8, and eps = 0.5 at omega = 1 alone, the
    x == 0 branch among them) -- the comment holds; 1.4e-9 and 2.8e-9 in the two eps = 0.5 cases with omega = 0.04 pi and 20 pi,
    where the two erf values are equal to seven digits and scipy's erf loses as much (6.9e-10 and 1.3e-9)."""
    c = {k: golden[f"{name}.{k}"] for k in ("freq", "nu", "times", "step_times", "step_sizes", "zm_re", "zm_im", "vm", "vlay")}
    eps = float(golden[f"{name}.eps"])
    zm = ctx.phasor_z_matrix(c["freq"], c["nu"], eps)
    ref = c["zm_re"] + 1j * c["zm_im"]
    zero = c["nu"] == 0.0
    assert not zm[:, zero].any()                                     # both limits coincide: exactly 0
    one = c["nu"] == 1.0
    assert one.any() and c["freq"][0] == mu.F_UNIT_OMEGA and np.all(zm[0, one].imag != 0)      # x == 0 in cerf, a nonzero result
    sc = float(np.abs(ref).max())
    check(f"phasor_z.{name}", np.stack([zm.real, zm.imag]), np.stack([ref.real, ref.imag]), scale=sc)
    vm, vlay = ctx.phasor_v_matrix(c["times"], c["nu"], eps, c["step_times"], c["step_sizes"])
    assert same(vlay == 0, c["vlay"] == 0)
    check(f"phasor_v.{name}", vlay, c["vlay"])
    check(f"phasor_v.{name}", vm, c["vm"], scale=float(np.abs(c["vlay"]).max()))


# ---- 8. func_eval_matrix ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nb", mu.FUNC_EVAL_NB)
def test_func_eval_matrix_tile_edges(ctx, nb):
    for ne in mu.FUNC_EVAL_NE:
        basis, ev = mu.uniform_ln_tau(nb), np.sort(mu.rng_of(8, nb, ne).uniform(-15, 6, ne))
        for order in range(3):
            check(f"func_eval{order}", ctx.func_eval_matrix(basis, ev, 1.7, order), mu.func_eval(basis, ev, 1.7, order))


# ---- 9. more rows than a grid's y dimension holds ----------------------------------------------------------------------------------
def in_chunks(build, times, rows=30000):
    return np.concatenate([build(times[r0:r0 + rows]) for r0 in range(0, times.size, rows)])


def test_long_records(ctx):
    """65 539 samples: the four response and phasance kernels stride over the rows.  Full output, each row bit for bit what a short
    build of the same samples gives -- the last four rows (beyond 65 535) included"""
    from hipdrt import _ffi
    nt = mu.LONG_NT
    times, tau, st, sz = mu.long_inputs()
    builds = {
        "pot": lambda t: ctx.response_matrix_variant(t, tau, st, sz, _ffi.RESPONSE_POT, layered=False)[0],
        "phasor_v": lambda t: ctx.phasor_v_matrix(t, [0.5], 2.0, st, sz)[0],
        "trapz": lambda t: ctx.response_matrix(t, tau, st, sz, mu.EPS_DEFAULT, TRAPZ, ny=64, layered=False)[0],
    }
    for name, build in builds.items():
        got = build(times)
        assert got.shape == (nt, 1)
        assert same(got, in_chunks(build, times)), name
    check("response_pot", builds["pot"](times), mu.response_pot(times, tau, st, sz)[0])
    # spectra ride on gridDim.y / .z of the general builds: a batch beyond it is refused before any launch
    refused(lambda: ctx.impedance_matrix(np.ones((mu.GRID_DIM_MAX + 1, 1)), [1.0], 1.0, TRAPZ, False, ny=2))
