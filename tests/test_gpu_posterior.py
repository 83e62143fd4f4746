"""GPU: the posterior variance and covariance chain alone (hipdrt_debug_posterior: pack_rows_kernel, cov_kernel_resident with the
32-column factorisation OpsResidentT::factor() and its appended tile rows, rows_outer_kernel -- the functions the plan entry points
call, csrc/plan_post.hip) on matrices of known condition, against the extended-precision reference of tests/posterior_util.py.

a. sizes around every tile and block edge;  b. both sides of the LDS / global-U switch at n = 528 / 529;  c. n = 2049 and 4096;
d. the pass boundaries of the row wavefronts (24 tile rows per pass);  e. column offsets, the packed image bit for bit;
f. exact padding invariants;  g. invariances, bit for bit;  h. more than 256 spectra (the chunk loop);  i. the full matrix;
j. breakdown on an indefinite P;  k. the refusals.

Bound (posterior_util): |var - exact| <= C_BOUND (n + 16) u kappa_2(P) var, for cov_ij with sqrt(var_i var_j); nothing in it is
taken from the kernel.  Every numerical check prints its worst deviation / bound.
"""
import numpy as np
import pytest

import gram_util as gu
import posterior_util as pu

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(gu.extended_dtype() is None, reason="no extended type on this platform")]

TABLE = pu.case_table()
U = pu.U


def names(group):
    return [k for k, (g, _) in TABLE.items() if g == group]


@pytest.fixture(scope="module")
def ctx():
    from hipdrt import _ffi
    return _ffi.get_context(0)


def check_var(ctx, name, want=("var", "status"), **kw):
    """the case through the hook (B = 1): status 0, var >= 0 and inside the bound -> (outputs, case, reference, ratio)"""
    c, ref = pu.get_case(name, TABLE[name][0] == "i")
    out = ctx.debug_posterior(c["P"], c["rows"], c["off"], want=want, **kw)
    assert out["status"].tolist() == [0], (name, out["status"])
    var = out["var"][0]
    assert np.all(var >= 0.0), name
    scale = 1.0 if kw.get("scale") is None else float(np.ravel(kw["scale"])[max(kw.get("cov_member", 0), 0)])
    r = pu.var_ratio(var, ref, c["n"], c["kappa"], scale)
    print(f"{name}: n {c['n']} neval {c['neval']} kappa {c['kappa']:.3g}: worst deviation / bound {r / pu.C_BOUND:.2e}")
    assert r <= pu.C_BOUND, (name, r)
    return out, c, ref, r


# ---- a, b, c, d: sizes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", sorted({s["n"] for g, s in TABLE.values() if g == "a"}))
def test_a_sizes_around_tile_and_block_edges(ctx, n):
    worst = max(check_var(ctx, k)[3] for k in names("a") if TABLE[k][1]["n"] == n)
    print(f"group a, n = {n}: worst deviation / bound {worst / pu.C_BOUND:.2e}")


@pytest.mark.parametrize("name", names("b"))
def test_b_lds_and_global_u_forms(ctx, name):
    check_var(ctx, name)


@pytest.mark.parametrize("name", names("c"))
def test_c_large(ctx, name):
    check_var(ctx, name)


@pytest.mark.parametrize("name", names("d"))
def test_d_pass_boundaries_of_the_row_wavefronts(ctx, name):
    check_var(ctx, name)


# ---- e, f: packing and padding, exact ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names("e"))
def test_e_column_offset_and_packed_image(ctx, name):
    out, c, _, _ = check_var(ctx, name, want=("var", "status", "bex"))
    np.testing.assert_array_equal(out["bex"], pu.pack_rows(c["rows"], c["n"], c["off"]))


@pytest.mark.parametrize("name", ["a_n17_k1e+01_e40", "a_n33_k1e+06_e17", "a_n49_k1e+10_e40", "a_n97_k1e+01_e17", "e_off17_part",
                                  "b_n513", "b_n545", "d_n33_e385"])
def test_f_exact_padding_invariants(ctx, name):
    out, c, _, _ = check_var(ctx, name, want=("var", "status", "bex", "tail"))
    n, neval = c["n"], c["neval"]
    np.testing.assert_array_equal(out["bex"], pu.pack_rows(c["rows"], n, c["off"]))
    Y = pu.unpack_rows(out["tail"][0])
    assert Y.shape == ((neval + 15) // 16 * 16, gu.nchp_of(n) * 16)
    # rows beyond neval are zero rows of the packed image, and a zero row stays zero through every product
    np.testing.assert_array_equal(Y[neval:], 0.0)
    # tile columns from 2 ceil(n / 32) on do not exist; the columns from n on multiply the identity padding of P
    np.testing.assert_array_equal(Y[:, n:], 0.0)
    if neval >= 4:                                          # posterior_util.make_rows: row 2 is zero
        assert not c["rows"][2].any()
        np.testing.assert_array_equal(Y[2], 0.0)
        assert out["var"][0, 2] == 0.0
    # var is the float64 sum of the squares of a row of Y, in the kernel's own order: n terms
    ss = np.sum(Y[:neval] ** 2, axis=1)
    assert np.all(np.abs(ss - out["var"][0]) <= 2 * (n + 2) * U * out["var"][0])


# ---- g: invariances, bit for bit ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [40, 161, 600])
def test_g_batch_position_and_form_do_not_change_a_bit(ctx, n):
    Pa, _ = pu.spd_matrix(n, 1e6, 11)
    Px, _ = pu.spd_matrix(n, 1e1, 12)
    Py, _ = pu.spd_matrix(n, 1e10, 13)
    rows = pu.make_rows("mixed", 40, n - 2, 5)
    alone = ctx.debug_posterior(Pa, rows, 2)
    member = ctx.debug_posterior(np.stack([Px, Py, Pa]), rows, 2)
    shared = ctx.debug_posterior(Pa, rows, 2, B=3)
    single = ctx.debug_posterior(np.stack([Px, Py, Pa]), rows, 2, cov_member=2)
    assert alone["status"].tolist() == [0] and member["status"].tolist() == [0, 0, 0] and shared["status"].tolist() == [0, 0, 0]
    np.testing.assert_array_equal(member["var"][2], alone["var"][0])
    for b in range(3):
        np.testing.assert_array_equal(shared["var"][b], alone["var"][0])
    np.testing.assert_array_equal(single["var"], alone["var"])
    assert single["status"].tolist() == [0]
    assert not np.array_equal(member["var"][0], member["var"][2])          # (the members are different problems)


@pytest.mark.parametrize("n", [33, 161])
def test_g_a_row_does_not_depend_on_its_companions_or_its_pass(ctx, n):
    """row wavefronts take 24 tile rows per pass: tile row 24 (rows 384 ..) is the first of the second pass"""
    P, _ = pu.spd_matrix(n, 1e6, 21)
    rng = np.random.default_rng(22)
    r = rng.standard_normal((1, n - 2))
    r40, r389 = rng.standard_normal((40, n - 2)), rng.standard_normal((24 * 16 + 5, n - 2))
    r40[20], r389[386] = r[0], r[0]
    v1 = ctx.debug_posterior(P, r, 2)["var"][0, 0]
    v40 = ctx.debug_posterior(P, r40, 2)["var"][0]
    v389 = ctx.debug_posterior(P, r389, 2)["var"][0]
    assert v1 == v40[20] and v1 == v389[386], (v1, v40[20], v389[386])
    # and the companions of the first 40 rows' tile rows: the same rows in the longer set
    r389b = r389.copy()
    r389b[:40] = r40
    np.testing.assert_array_equal(ctx.debug_posterior(P, r389b, 2)["var"][0, :40], v40)


# ---- h: the chunk loop ------------------------------------------------------------------------------------------------------------
def test_h_more_than_256_spectra(ctx):
    B, n, neval = 300, 5, 3
    built = [pu.spd_matrix(n, 10.0 ** (1 + b % 6), 1000 + b) for b in range(B)]
    P = np.stack([p for p, _ in built])
    rows = np.random.default_rng(31).standard_normal((neval, n))
    out = ctx.debug_posterior(P, rows, 0)
    assert not out["status"].any()
    worst = 0.0
    for b in range(B):
        ref = pu.reference(P[b], rows, built[b][1])
        worst = max(worst, pu.var_ratio(out["var"][b], ref, n, built[b][1]))
    print(f"h: 300 spectra of n = 5: worst deviation / bound {worst / pu.C_BOUND:.2e}")
    assert worst <= pu.C_BOUND
    for b in (255, 256, 299):
        np.testing.assert_array_equal(ctx.debug_posterior(P[b], rows, 0)["var"][0], out["var"][b])


# ---- i: the full matrix -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", names("i"))
def test_i_full_covariance(ctx, name):
    scale = np.array([1.7])
    out, c, ref, _ = check_var(ctx, name, want=("var", "status", "cov"), cov_member=0, scale=scale)
    cov, var, n = out["cov"], out["var"][0], c["n"]
    r = pu.cov_ratio(cov, ref, n, c["kappa"], 1.7)
    print(f"{name}: cov worst deviation / bound {r / pu.C_BOUND:.2e}")
    assert r <= pu.C_BOUND, (name, r)
    np.testing.assert_array_equal(cov, cov.T)
    # both are float64 sums of the same n squares, scaled once
    assert np.all(np.abs(np.diag(cov) - var) <= 2 * (n + 2) * U * var), np.max(np.abs(np.diag(cov) - var) / var)


# ---- j: breakdown -----------------------------------------------------------------------------------------------------------------
def indefinite(P, k):
    """P with its k-th Cholesky pivot turned into -1: the pivots before it depend on the leading block alone and stay"""
    L = np.linalg.cholesky(P)
    Q = P.copy()
    Q[k, k] = np.sum(L[k, :k] ** 2) - 1.0
    return Q


@pytest.mark.parametrize("n", [40, 600])
@pytest.mark.parametrize("where", ["first", "second_half_of_a_block", "last"])
def test_j_breakdown_is_reported_and_stays_with_its_spectrum(ctx, n, where):
    k = {"first": 0, "second_half_of_a_block": 20, "last": n - 1}[where]
    P0, _ = pu.spd_matrix(n, 1e6, 41)
    P1, _ = pu.spd_matrix(n, 1e1, 42)
    P2, _ = pu.spd_matrix(n, 1e6, 43)
    rows = pu.make_rows("mixed", 17, n - 2, 44)
    good = ctx.debug_posterior(np.stack([P0, P1, P2]), rows, 2)
    assert good["status"].tolist() == [0, 0, 0]
    bad = ctx.debug_posterior(np.stack([P0, indefinite(P1, k), P2]), rows, 2)
    assert bad["status"].tolist() == [0, -1, 0]
    assert np.all(np.isnan(bad["var"][1]))
    np.testing.assert_array_equal(bad["var"][[0, 2]], good["var"][[0, 2]])
    one = ctx.debug_posterior(np.stack([P0, indefinite(P1, k), P2]), rows, 2, cov_member=1, want=("var", "status", "cov"))
    assert one["status"].tolist() == [-1] and np.all(np.isnan(one["cov"])) and np.all(np.isnan(one["var"]))


# ---- k: refusals ------------------------------------------------------------------------------------------------------------------
def test_k_refusals(ctx):
    from hipdrt._ffi import HipDrtError
    n = 20
    P, _ = pu.spd_matrix(n, 1e1, 51)
    rows = pu.make_rows("mixed", 5, n - 2, 52)
    nan_p, inf_rows = P.copy(), rows.copy()
    nan_p[7, 3] = np.nan
    inf_rows[4, 0] = np.inf
    calls = dict(
        n_zero=lambda: ctx.debug_posterior(np.zeros((0, 1)), np.ones((1, 1)), 0, n=0),
        n_large=lambda: ctx.debug_posterior(np.eye(4097), np.ones((1, 1)), 0),
        B_zero=lambda: ctx.debug_posterior(P, rows, 2, B=0),
        B_large=lambda: ctx.debug_posterior(P, rows, 2, B=4097),
        neval_zero=lambda: ctx.debug_posterior(P, np.zeros((0, n - 2)), 2),
        offset_negative=lambda: ctx.debug_posterior(P, rows, -1),
        columns_past_n=lambda: ctx.debug_posterior(P, rows, 3),
        ldp_small=lambda: ctx.debug_posterior(np.ascontiguousarray(P[:, :n - 1]), rows, 2),
        cov_member_large=lambda: ctx.debug_posterior(P, rows, 2, B=3, cov_member=3),
        cov_member_negative=lambda: ctx.debug_posterior(P, rows, 2, B=3, cov_member=-2),
        nan_in_p=lambda: ctx.debug_posterior(nan_p, rows, 2),
        inf_in_rows=lambda: ctx.debug_posterior(P, inf_rows, 2),
        nan_scale=lambda: ctx.debug_posterior(P, rows, 2, scale=[np.nan]),
    )
    for what, call in calls.items():
        with pytest.raises(HipDrtError):
            call()
        print("refused:", what)
    # and the same arguments without the defect are served
    assert ctx.debug_posterior(P, rows, 2)["status"].tolist() == [0]
