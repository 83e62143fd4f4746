"""CPU: pins tests/matrices_edges_util.py -- that its case list reaches every launch form and loop path of csrc/matrices.hip
the GPU suite is there for, that each extended-precision statement agrees with the float64 oracle at ordinary sizes, that the
mpmath fixture is what the tool writes, and that the committed bounds table is what the rule gives today."""
import json
import os
import sys

import numpy as np
import pytest

import matrices_edges_util as mu
from oracle import drt_oracle as orc

LD = np.longdouble


def test_longdouble_is_wider_than_double():
    assert np.finfo(LD).eps < 2.0 ** -60, "the statements need an extended-precision long double"


def test_unit_omega_frequency_is_exact():
    """2.0 * PI * f == 1.0 in the kernel's own order of operations, so ln(omega) is exactly 0 on any libm: with nu = 1 the complex
    erf of phasor_z_kernel gets x == 0 and y != 0 (a nonzero result from its x == 0 branch)"""
    f = np.float64(mu.F_UNIT_OMEGA)
    assert 2.0 * 3.141592653589793 * f == 1.0 and np.log(2.0 * 3.141592653589793 * f) == 0.0
    for eps in mu.PHASOR_EPS:
        assert eps * (1.0 - 1.0) + (-0.0 / (2.0 * eps)) == 0.0 and -np.pi / (4.0 * eps) != 0.0
    assert all(c["freq"][0] == f and 1.0 in c["nu"] for c in mu.phasor_cases().values())
    assert all(0.0 in c["nu"] for c in mu.phasor_cases().values() if c["nu"].size > 1)
    assert {c["nu"].size for c in mu.phasor_cases().values()} == {1, 63, 64, 65}
    assert {(c["freq"].size, c["times"].size) for c in mu.phasor_cases().values()} == {(1, 1), (3, 3)}


def test_interp_geometry_reaches_every_form():
    cases = mu.geometry_cases()
    forms = [(mu.interp_form(B, nf, ntau), B, nf, ntau) for (B, nf, ntau) in cases]
    assert {f["rpb"] for f, *_ in forms} == {4, 8, 16, 32, 64, 128, 256}
    assert {f["tpr"] for f, *_ in forms} == {64, 128, 256, 512, 1024}
    for rpb, shapes in mu.GEOMETRY_BATCHED.items():
        assert all(mu.interp_form(*s)["rpb"] == rpb for s in shapes), rpb
        # the two-row loop makes a pass at every rpb >= 8: an `entry(r + rp)` gone wrong shows at each of them
        assert rpb == 4 or any(mu.two_row_passes(s[1], mu.interp_form(*s)) >= 1 for s in shapes), rpb
    assert max(mu.two_row_passes(nf, f) for f, B, nf, ntau in forms) >= 2
    # a workgroup's row count modulo 2 rp: a whole number of passes, a lone last row, one row short of a pass, one beyond
    for rp in (1, 2):
        seen = {rows % (2 * rp) for f, B, nf, ntau in forms if f["rp"] == rp for rows in mu.block_rows(nf, f["rpb"])}
        assert seen >= {0, 1 % (2 * rp), rp, (rp + 1) % (2 * rp)}, (rp, seen)
    assert any(ntau > 2 * 1024 for _, _, _, ntau in forms)                       # the column wrap c += 2 tpr
    assert any(ntau % 2 for _, _, _, ntau in forms) and any(ntau % 2 == 0 for _, _, _, ntau in forms)      # both store forms
    # the reference build never takes any of these paths
    ref = mu.interp_form(1, mu.REF_ROWS, mu.REF_COLS)
    assert (ref["rpb"], ref["tpr"], ref["rp"]) == (4, 64, 16) and mu.two_row_passes(mu.REF_ROWS, ref) == 0
    assert all(mu.interp_form(1, nf, mu.REF_COLS)["rpb"] == 4 for nf in (1, 2, 1000, mu.REF_ROWS))
    # downloads stay small
    assert max(B * nf * ntau * 16 for B, nf, ntau in cases) <= 20e6


def test_lds_edges():
    assert mu.interp_lds_bytes(2000, 256) == 98048 and mu.interp_lds_bytes(2000, 4) == 96032      # the default tables' launch
    assert mu.interp_lds_bytes(3400, 256) == 165248 > mu.LDS_LIMIT >= mu.interp_lds_bytes(3400, 32)
    assert mu.interp_form(1024, 1, 3, 3400)["rpb"] == 32 and mu.interp_form(1024, 1, 3, 2000)["rpb"] == 256
    assert mu.INTERP_NGRID_MAX == 3406 and mu.interp_lds_bytes(3407, 4) > mu.LDS_LIMIT
    assert mu.interp_form(1024, 1, 3, mu.INTERP_NGRID_MAX)["lds"] <= mu.LDS_LIMIT
    assert mu.RESPONSE_NGRID_MAX == 6816 and 3 * 8 * 6817 > mu.LDS_LIMIT
    assert 3 * 8 * mu.NY_MAX <= mu.LDS_LIMIT and 3 * 8 * 2731 > 64 * 1024 >= 3 * 8 * 2730
    assert {B for (_, B, _, _) in mu.lds_edge_cases()} == {1, 1024}
    assert {mu.interp_form(B, nf, ntau, 2000)["rpb"] for (_, B, nf, ntau) in mu.lds_edge_cases()} == {4, 256}
    assert [mu.toeplitz_grid_z(B) for B in mu.TOEPLITZ_B] == [1, 64, 64, 64] and max(mu.TOEPLITZ_B) > 2 * 64
    assert mu.LONG_NT > mu.GRID_DIM_MAX


def test_case_lists_cover_the_issue():
    assert {c[0] for c in mu.trapz_cases()} == set(mu.NY) == {c[0] for c in mu.toeplitz_trapz_cases()} == {c[0] for c in mu.response_cases()}
    assert {c[1:] for c in mu.trapz_cases()} == set(mu.TRAPZ_SHAPES)
    assert {s[1] for s in mu.TRAPZ_SHAPES} == {1, 15, 16, 17, 33} and {s[0] for s in mu.TRAPZ_SHAPES} == {1, 3} == {s[2] for s in mu.TRAPZ_SHAPES}
    assert {c[1:] for c in mu.toeplitz_trapz_cases()} == {(1, 1), (5, 3), (3, 5), (4, 4)}
    assert {s[0] for s in mu.RESPONSE_SHAPES} == {1, 7} and {s[2] for s in mu.RESPONSE_SHAPES} == {1, 3}
    assert {c[1:] for c in mu.response_cases()} == set(mu.RESPONSE_SHAPES)
    times, st, _, _ = mu.response_inputs(7, 3)
    assert times[0] < st[0] and np.isin(times, st).any()
    for nt, segs in mu.CHRONO_VAR.items():
        assert all(s[0] == 0 and s[-1] == nt and np.all(np.diff(s) > 0) for s in segs)
    assert any(1 in np.diff(s) for segs in mu.CHRONO_VAR.values() for s in segs) and 256 in mu.CHRONO_VAR[600][1]
    for nt in mu.NP_INTERP_NT:
        times, tau = mu.np_interp_inputs(nt, 257)
        table = mu.jittered_table(1999, 9.0, 2, zero_knot=True)
        x = np.log(times[:, None] / tau[None, :])
        assert (x == 0.0).any() and 0.0 in table[0] and (x < table[0][0]).any() and (x > table[0][-1]).any()
    assert [mu.response_rpb(nt, 257) for nt in mu.NP_INTERP_NT] == [1, 1, 1] and mu.response_rpb(20000, 257) == 32


# ---- every statement against the oracle at ordinary sizes ------------------------------------------------------------------
def close(got, ref, tol):
    assert mu.deviation(got, ref) <= tol, mu.deviation(got, ref)


def test_statements_equal_the_oracle_at_ordinary_sizes():
    eps = mu.EPS_DEFAULT
    freq, tau = np.logspace(5, -1, 13), np.logspace(-6, 1, 11)
    assert not orc.impedance_matrix_is_toeplitz(freq, tau)
    tables = orc.generate_impedance_lookup(eps, 300, 400)
    wt = np.exp(tables[0][0]), np.exp(tables[1][0])
    for part, got in enumerate(mu.impedance_lookup(eps, wt[0][::37], wt[1][::37], 400)):
        close(tables[part][1][::37], got, 1e-13)
    for part, name in enumerate(("real", "imag")):
        close(orc.construct_impedance_matrix(freq, name, tau, eps, 'trapz', 400), mu.impedance_trapz(freq, tau, eps, 400)[part], 1e-13)
        close(orc.construct_impedance_matrix(freq, name, tau, eps, 'interp', interpolate_grids=tables[part]),
              mu.impedance_interp(freq, tau, tables)[part], 1e-13)
        assert np.array_equal(orc.construct_impedance_matrix(freq, name, tau, eps, 'interp', interpolate_grids=tables[part]),
                              mu.impedance_interp_f64(freq, tau, tables)[part])
    # np.interp's own semantics, bit for bit where no rounding is involved: on the knots, beyond the ends
    xp, fp = mu.jittered_table(41, 3.0, 9)
    x = np.concatenate([xp, [xp[0] - 1, xp[-1] + 1, xp[0], xp[-1]], (xp[1:] + xp[:-1]) / 2])
    got = mu.interp(x, xp, fp)
    assert np.array_equal(got[:45].astype(float), np.interp(x[:45], xp, fp))
    close(np.interp(x, xp, fp), got, 1e-15)
    # the Toeplitz arrangement
    from scipy.linalg import toeplitz
    c, r = np.arange(5.0), np.r_[0.0, -np.arange(1.0, 7.0)]
    assert np.array_equal(mu.toeplitz_of(c, r), toeplitz(c, r))
    for shape in mu.TOEPLITZ_SHAPES + mu.TOEPLITZ_TRAPZ_SHAPES:      # omega_i tau_j depends on j - i alone
        f_t, t_t = mu.toeplitz_grids(*shape)
        x = np.log(2 * np.pi * f_t)[:, None] + np.log(t_t)[None, :]
        assert np.allclose(x[1:, 1:], x[:-1, :-1], rtol=0, atol=1e-12) and np.all(np.diff(f_t) < 0) and np.all(np.diff(t_t) > 0)
    # responses
    times, st, sz, tr = mu.response_inputs(7, 3)
    log_td, v = orc.generate_response_lookup(eps, 200, 400)
    close(v[::29], mu.response_trapz_entry(np.exp(log_td)[::29], eps, 400), 1e-13)
    for got, ref in zip(orc.construct_response_matrix(tau, times, st, sz, eps, 'trapz', 400), mu.response_trapz(times, tau, st, sz, eps, 400)):
        close(got, ref, 1e-13)
        assert np.array_equal(np.asarray(ref == 0), got == 0)
    for got, ref in zip(orc.construct_response_matrix(tau, times, st, sz, eps, 'interp', interpolate_grids=(log_td, v)),
                        mu.response_interp(times, tau, st, sz, (log_td, v))):
        close(got, ref, 1e-12)
    # tau_rise -> 0 is the ideal step; the potentiostatic form includes the step's own sample
    a0 = mu.response_expdecay(times, tau, st, sz, [1e-30] * 3, eps, 400)[0]
    close(a0.astype(float), mu.response_trapz(times, tau, st, sz, eps, 400)[0], 1e-15)
    pot, pot_lay = mu.response_pot(times, tau, st, sz)
    assert np.all(pot_lay[0][times >= st[0], -1] != 0) and not pot_lay[0][times < st[0]].any() and pot_lay[1][4, 0] == LD(sz[1])
    # penalties, variance matrices, basis evaluation
    grid = mu.uniform_ln_tau(57)
    assert orc.is_uniform(grid)
    for k in range(3):
        close(orc.construct_integrated_derivative_matrix(grid, k, 2.3), mu.penalty_matrices(grid, 2.3, True)[k], 1e-14)
        close(mu.penalty_matrices(grid, 2.3, False, dtype=np.float64)[k], mu.penalty_matrices(grid, 2.3, False)[k], 1e-14)
        assert float(np.abs(mu.penalty_matrices(grid, 2.3, True)[k]).max()) == pytest.approx(mu.penalty_scale(k, 2.3), rel=1e-15)
    close(orc.construct_eis_var_matrix(freq, 0.25, 0.25), mu.eis_var(freq, 0.25, 0.25), 1e-14)
    t_c = np.r_[np.linspace(-0.01, 0, 5, endpoint=False), np.logspace(-4, 0, 40), 1 + np.logspace(-4, 0, 40)]
    seg = np.r_[0, orc.get_step_indices_from_step_times(t_c, [0.0, 1.0]), t_c.size]
    close(orc.construct_chrono_var_matrix(t_c, [0.0, 1.0], 0.25), mu.chrono_var(orc.chrono_time_transform(t_c, [0.0, 1.0]), seg, 0.25), 1e-14)
    close(orc.construct_func_eval_matrix(grid, grid[::5] + 0.1, 2.3), mu.func_eval(grid, grid[::5] + 0.1, 2.3, 0), 1e-15)
    h = 1e-4                                               # the derivative orders, by differences of the statement itself
    ev = grid[::5] + 0.1
    d1 = (mu.func_eval(grid, ev + h, 2.3, 0) - mu.func_eval(grid, ev - h, 2.3, 0)) / (2 * LD(h))
    d2 = (mu.func_eval(grid, ev + h, 2.3, 1) - mu.func_eval(grid, ev - h, 2.3, 1)) / (2 * LD(h))
    close(d1, mu.func_eval(grid, ev, 2.3, 1), 1e-7)
    close(d2, mu.func_eval(grid, ev, 2.3, 2), 1e-7)


def test_underflow_is_why_the_scale_is_the_largest_entry():
    """ny = 2 with the default basis: float64 underflows phi to 0 at both nodes where long double keeps 1e-3274 -- a relative
    error of 1 in an entry that is nothing against the matrix; the cases use eps = 0.5 at ny <= 3"""
    assert orc.phi_gaussian(np.array([20.0]), mu.EPS_DEFAULT)[0] == 0.0 and mu.phi(LD(20), mu.EPS_DEFAULT) > 0
    assert all(mu.eps_of(ny) == 0.5 for ny in mu.NY if ny <= 3)
    re, im = mu.impedance_trapz([1.0], [0.1], mu.eps_of(2), 2)
    assert float(abs(re[0, 0])) > 1e-50


# ---- the mpmath fixture -----------------------------------------------------------------------------------------------------
def test_phasor_fixture_holds_the_cases_inputs():
    G = np.load(mu.PHASOR_GOLDEN)
    cases = mu.phasor_cases()
    assert {k.rsplit(".", 1)[0] for k in G.files} == set(cases)
    for name, c in cases.items():
        for key in ("freq", "nu", "times", "step_times", "step_sizes"):
            assert np.array_equal(G[f"{name}.{key}"], c[key]), (name, key)
        assert float(G[f"{name}.eps"]) == c["eps"]
        col0 = np.flatnonzero(c["nu"] == 0.0)
        assert not G[f"{name}.zm_re"][:, col0].any() and not G[f"{name}.zm_im"][:, col0].any() and not G[f"{name}.vlay"][:, :, col0].any()
        assert np.array_equal(G[f"{name}.vlay"] == 0, np.broadcast_to(
            (~(c["times"][None, :] > c["step_times"][:, None]))[:, :, None] | (c["nu"] == 0)[None, None, :] | (c["nu"] == 1)[None, None, :],
            G[f"{name}.vlay"].shape))
    # the x == 0 branch of the device's complex erf: omega = 1, nu = 1 -- a nonzero entry
    assert all(G[f"{name}.zm_im"][0, -1] != 0 for name in cases)
    assert os.path.getsize(mu.PHASOR_GOLDEN) < 200e3


def test_phasor_fixture_is_what_the_tool_writes():
    pytest.importorskip("mpmath")
    sys.path.insert(0, os.path.join(os.path.dirname(mu.HERE), "tools"))
    try:
        import make_phasor_edges_golden as tool
    finally:
        sys.path.pop(0)
    G = np.load(mu.PHASOR_GOLDEN)
    fresh = tool.build()
    assert set(fresh) == set(G.files)
    for key, val in fresh.items():
        assert np.array_equal(G[key], val), key
    # 40 digits are enough: 60 digits round to the same doubles
    name = "eps0.5_nnu65"
    for got, want in zip(tool.evaluate(mu.phasor_cases()[name], digits=60), (G[f"{name}.zm_re"] + 1j * G[f"{name}.zm_im"], G[f"{name}.vm"], G[f"{name}.vlay"])):
        assert np.array_equal(got, want)


# ---- the bounds table -------------------------------------------------------------------------------------------------------
def test_bound_rule():
    assert mu.step_125(0.0) == mu.FLOOR == 16 * 2.0 ** -52 and mu.step_125(3e-16) == mu.FLOOR
    assert mu.step_125(3.6e-16) == 5e-15 and mu.step_125(1e-15) == 1e-14 and mu.step_125(1.01e-15) == 2e-14
    assert mu.step_125(2.1e-15) == 5e-14 and mu.step_125(5.1e-15) == 1e-13


def test_committed_bounds_are_what_the_rule_gives_today():
    """the float64 oracle against the extended-precision statements on the GPU cases' own inputs: the committed table must state
    that measurement (to the digits it keeps; libm may move the last one) and the rule's bound for it"""
    with open(mu.BOUNDS) as f:
        table = json.load(f)
    measured = mu.measure_bounds()
    assert set(table) == set(measured)
    for key, (m, b) in table.items():
        assert b == mu.step_125(m), key
        now = measured[key]
        assert abs(now - m) <= 0.02 * m + 1e-17, (key, now, m)
        assert mu.step_125(now) == b or abs(10 * now - b) <= 0.05 * b, (key, now, b)
