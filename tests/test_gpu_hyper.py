"""GPU: the hyper-parameter step of the fit loop (csrc/hyper.hip: hyper_kernel -- solve_s, solve_rho, the xmx freeze,
estimate_weights, the convergence rule, the vz_offset column, update_scale -- with the products of estimate_weights inside it, from
premv_kernel, or from batch_products_kernel<0> / <1> on the matrix pipe) in isolation, through the test hook hipdrt_debug_hyper_step
(include/hipdrt_debug.h), which calls launch_hyper exactly as the loop does (csrc/plan_fit.hip: plan_hyper).

The reference is the extended-precision restatement of tests/hyper_util.py, and every tolerance is the forward error bound derived in
its docstring for a float64 evaluation in any summation order (checked from both sides on the CPU, on these very inputs, by
tests/test_hyper_util.py).  An error is recorded in units of its bound: every ratio in tests/_parity_measured.txt must be <= 1.
State the step must not touch is poisoned beforehand and has a zero bound: it must come back bit for bit.  Where the code promises
the same bits on two paths (reach window or all columns; products inside the kernel or from premv_kernel; a spectrum alone or in a
batch; the uniform-chrono shortcut) the comparison is assert_array_equal.
"""
import numpy as np
import pytest

import hyper_util as hu
from conftest import parity_close

pytestmark = pytest.mark.gpu

TABLE = hu.case_table()
LDS_DOUBLES = (160 * 1024 - 256) // 8          # dynamic LDS of one workgroup, in doubles (csrc/hyper_dev.hpp: kLdsLimit)


@pytest.fixture(scope="module")
def ctx():
    from hipdrt import _ffi
    return _ffi.get_context()


def names(group, prefix=""):
    return [n for n, (g, _) in TABLE.items() if g == group and n.startswith(prefix)]


def fit_opts(c):
    from hipdrt import _ffi
    o = _ffi.default_fit_opts()
    for key, v in c["opts"].items():
        if isinstance(v, tuple):
            for k in range(3):
                getattr(o, key)[k] = v[k]
        else:
            setattr(o, key, v)
    return o


def prepared_desc(c):
    from hipdrt import _ffi
    if c["desc"] is None:
        return None
    d = _ffi.PreparedDesc()
    for key, v in c["desc"].items():
        if isinstance(v, tuple):
            for k in range(3):
                getattr(d, key)[k] = v[k]
        else:
            setattr(d, key, v)
    return d


def run(ctx, c, products=0, **over):
    c = dict(c, **over)
    return ctx.debug_hyper_step(c["rm"], c["vmm"], c["mk"], c["x"], c["x_in"], c["s"], c["rho"], c["xmx"], c["rv"], c["est_w"], c["w"],
                                c["var_floor"], c["coef_scale"], fit_opts(c), ns=c["ns"], n=c["n"], toeplitz=c["toeplitz"],
                                toep_reach=c["toep_reach"], qp_status=c["qp_status"], active=c["active"], fit_status=c["fit_status"],
                                outer_iters=c["outer_iters"], n_active=c["n_active"], outlier_t=c["outlier_t"], it=c["it"],
                                continue_mode=c["continue_mode"], min_iter=c["min_iter"], basis_area=c["basis_area"],
                                desc=prepared_desc(c), dop_rho=c["dop_rho"], dop_xmx=c["dop_xmx"], vz_strength=c["vz_strength"],
                                vz_entry=c["vz_entry"], products=products)


def check(label, got, ref):
    """every floating-point output within its bound (recorded in units of the bound), every integer output equal"""
    r = hu.ratios(got, ref)
    for key in hu.INT_KEYS:
        np.testing.assert_array_equal(got[key], ref[key], err_msg=f"{label}: {key}")
    assert got["n_active"] == ref["n_active"], (label, got["n_active"], ref["n_active"])
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    for key, v in r.items():
        if key not in bad:
            parity_close(f"hyper_step:{label.split(':')[0]}:{key}", v, 0.0, 1.0, scale=1.0)
    assert not bad, (label, bad)
    return r


def same_bits(a, b, what):
    for key in hu.FLOAT_KEYS + hu.INT_KEYS:
        if a.get(key) is not None:
            np.testing.assert_array_equal(a[key], b[key], err_msg=f"{what}: {key}")
    assert a["n_active"] == b["n_active"], what


def test_every_shape_lies_on_the_side_of_the_fold_it_is_meant_for(ctx):
    assert LDS_DOUBLES == 20448
    # the three LDS forms: the columns beside the two m-vectors, inside the second one, not in LDS at all
    def doubles(nd, ns, m):
        n, tl, cols = nd + ns, max(m, nd), 3 * (2 * nd - 1)
        return n + 4 * nd + 2 * tl + cols, n + 4 * nd + tl + max(tl, nd + cols), cols
    for name, want in (("form1", 1), ("form2", 2), ("form2_tall", 2), ("form0", 0)):
        nd, ns, m = hu.FORM_SHAPES[name]
        full, compact, cols = doubles(nd, ns, m)
        form, lds = ctx.debug_hyper_form(nd + ns, m, ns, True, False)
        assert form == want, (name, form)
        if want == 1:
            assert full <= LDS_DOUBLES and lds == 8 * full
        elif want == 2:
            assert full > LDS_DOUBLES >= compact and lds == 8 * compact
        else:
            assert compact > LDS_DOUBLES >= full - cols and lds == 8 * (full - cols)
    assert doubles(1500, 2, 2000)[:2] == (20499, 19999) and doubles(1700, 2, 2000)[1] == 22399
    nd, ns, m = hu.FORM_SHAPES["form2"]
    assert m < nd + 3 * (2 * nd - 1)                    # the columns end beyond the m-vector they start in
    nd, ns, m = hu.FORM_SHAPES["form2_tall"]
    assert m > nd + 3 * (2 * nd - 1)                    # ... and here inside it
    assert ctx.debug_hyper_form(66, 24, 2, False, False)[0] == 0 and ctx.debug_hyper_form(66, 24, 2, True, True)[0] == 1
    # the outlier branch keeps two more m-vectors behind the columns and has no compact form
    from hipdrt import _ffi
    with pytest.raises(_ffi.HipDrtError, match="too large for LDS"):
        ctx.debug_hyper_form(1502, 2000, 2, True, True)
    # Toeplitz row sums: two rows and 512 threads, so a second pass of the thread loop from nd = 1025; odd nd has a last row
    # without a partner; windows clipped at 0 (reach >= 2p), at nd (2p + 2 + reach > nd), and not at all (63 .. 65 with reach <= 5)
    assert max(hu.TOEP_ND) > 2 * 512 >= 1024 and {nd % 2 for nd in hu.TOEP_ND} == {0, 1}
    assert all(r in hu.toep_reaches(65) for r in (0, 1, 2, 3, 4, 5, 63, 64, 72))
    # rows_matvec: 16-byte loads when ld and ncol are even and the block starts on 16 bytes -- for a penalty block at (ns, ns) that
    # is ns * ldm + ns even; chunks of 512 columns (514, 515 take a second one; 510, 512 end inside / at the first); four rows per
    # pass (m = 1 .. 5); tail columns clamped to ncol - 2 (ncol = 2: column 0)
    forms = set()
    for name in names("general"):
        kw = TABLE[name][1]
        n = kw["nd"] + kw["ns"]
        vec_pen = kw["ldm"] % 2 == 0 and kw["nd"] % 2 == 0 and (kw["ns"] * kw["ldm"] + kw["ns"]) % 2 == 0
        vec_rm = kw["ldrm"] % 2 == 0 and n % 2 == 0
        vec_v = kw["m"] % 2 == 0
        forms |= {("pen", vec_pen, kw["nd"] > 512), ("rm", vec_rm), ("vmm", vec_v)}
    assert forms >= {("pen", True, False), ("pen", True, True), ("pen", False, False), ("pen", False, True), ("rm", True), ("rm", False),
                     ("vmm", True), ("vmm", False)}
    # batched products: tiles of 32 spectra x 64 rows, slabs of 16 columns
    assert {b - 32 for b in hu.BATCH_B} >= {-1, 0, 1} and {m - 64 for m in hu.BATCH_M} >= {-1, 0, 1} and {n - 16 for n in hu.BATCH_N} >= {-1, 0, 1}


@pytest.mark.parametrize("nd", hu.TOEP_ND)
def test_toeplitz_row_sums_and_reach_window(ctx, nd):
    for name in names("toeplitz", f"toep_nd{nd}_"):
        c, ref = hu.get_case(name)
        got = run(ctx, c)
        check(f"toeplitz:{name}", got, ref)
        # the documented guarantee: restricted to the reach or over all columns, the same bits
        same_bits(got, run(ctx, c, toep_reach=-1), f"{name}: reach window against all columns")
        if c["toep_reach"] != c["reach"]:
            same_bits(got, run(ctx, c, toep_reach=c["reach"]), f"{name}: against the true reach")


@pytest.mark.parametrize("nd", hu.GEN_ND)
def test_general_form_and_rows_matvec(ctx, nd):
    for name in names("general", f"gen_nd{nd}_"):
        c, ref = hu.get_case(name)
        check(f"general:{name}", run(ctx, c), ref)


@pytest.mark.parametrize("name", list(hu.FORM_SHAPES))
def test_three_lds_forms(ctx, name):
    c, ref = hu.get_case(name)
    assert c["it"] == 0                                   # the xmx phase reads the (aliased) columns as well
    got = run(ctx, c)
    check(f"forms:{name}", got, ref)
    if name != "form0":                                   # the fallback is another summation order; the two Toeplitz layouts are not
        same_bits(got, run(ctx, c, toep_reach=-1), f"{name}: reach window against all columns")


@pytest.mark.parametrize("name", names("solve_s"))
def test_solve_s_branches(ctx, name):
    c, ref = hu.get_case(name)
    check(f"solve_s:{name}", run(ctx, c), ref)


@pytest.mark.parametrize("name", names("weights"))
def test_weights(ctx, name):
    c, ref = hu.get_case(name)
    got = run(ctx, c)
    check(f"weights:{name}", got, ref)
    if c["desc"] and c["desc"]["chrono_vmm_uniform"]:
        plain = run(ctx, dict(c, desc=dict(c["desc"], chrono_vmm_uniform=0)))
        same_bits(got, plain, f"{name}: one row for the uniform chrono block against all rows")
        same_bits(got, run(ctx, c, products=1), f"{name}: premv_kernel's shortcut")


@pytest.mark.parametrize("name", names("products"))
def test_products_inside_the_kernel_and_from_premv_kernel_agree_bit_for_bit(ctx, name):
    c, ref = hu.get_case(name)
    got = run(ctx, c, products=0)
    check(f"products:{name}", got, ref)
    same_bits(got, run(ctx, c, products=1), name)
    cb = dict(c, rm=np.repeat(c["rm"][None], c["B"], axis=0))            # one response matrix per spectrum: the same numbers
    same_bits(got, run(ctx, cb, products=1), name + " (rm per spectrum)")


@pytest.mark.parametrize("name", names("batch"))
def test_batched_products_on_the_matrix_pipe(ctx, name):
    c, ref = hu.get_case(name)
    got = run(ctx, c, products=2)
    check(f"batch:{name}", got, ref)
    if c["B"] == 70:
        keys = ("x", "x_in", "s", "rho", "xmx", "rv", "est_w", "w", "var_floor", "coef_scale", "qp_status", "active", "fit_status",
                "outer_iters", "outlier_t")
        for b in (0, 31, 32, 69):
            alone = run(ctx, dict(c, B=1, **{k: c[k][b:b + 1] for k in keys}), products=2)
            for key in hu.FLOAT_KEYS + hu.INT_KEYS:
                if got.get(key) is not None:
                    np.testing.assert_array_equal(alone[key][0], got[key][b], err_msg=f"member {b} alone: {key}")
        # a slab of 32 spectra that are all inactive, next to active ones: nothing of theirs changes, the others do not notice
        act = np.ones(70, dtype=np.int32)
        act[32:64] = 0
        part = run(ctx, dict(c, active=act), products=2)
        on = act != 0
        for key in hu.FLOAT_KEYS + hu.INT_KEYS:
            if got.get(key) is None:
                continue
            np.testing.assert_array_equal(part[key][on], got[key][on], err_msg=key)
            before = act if key == "active" else c[key]
            np.testing.assert_array_equal(part[key][~on], np.asarray(before)[~on], err_msg=f"inactive slab: {key}")
        assert part["n_active"] == c["n_active"] + int(on.sum())


@pytest.mark.parametrize("name", names("flow"))
def test_control_flow_and_state(ctx, name):
    c, ref = hu.get_case(name)
    got = run(ctx, c)
    check(f"flow:{name}", got, ref)
    same_bits(got, run(ctx, c, products=1), f"{name}: premv_kernel (the vz_offset product included)")


def test_inactive_and_failed_spectra_keep_their_poison(ctx):
    c, ref = hu.get_case("f_inactive")
    got = run(ctx, c)
    it = c["it"]
    np.testing.assert_array_equal(got["active"], [got["active"][0], 0, 0, 0])
    np.testing.assert_array_equal(got["fit_status"][1:], [-77, -1, -77])
    np.testing.assert_array_equal(got["outer_iters"], [it + 1, -77, it + 1, -77])
    for key in ("s", "rho", "xmx", "w", "x_in", "rv", "est_w", "coef_scale", "var_floor", "outlier_t"):
        np.testing.assert_array_equal(got[key][1:], c[key][1:], err_msg=key)
    assert (got["w"][0] != hu.POISON).all() and got["n_active"] == c["n_active"] + 1


def test_refusals(ctx):
    from hipdrt import _ffi
    c, _ = hu.get_case("s_neg")
    g, _ = hu.get_case("s_neg_general")
    d, _ = hu.get_case("s_dop_2_5")
    v, _ = hu.get_case("f_vz")

    def refused(match, case, products=0, **over):
        with pytest.raises(_ffi.HipDrtError, match=match):
            run(ctx, case, products=products, **over)

    refused("DRT block", c, ns=c["n"])
    refused("not symmetric Toeplitz", g, toeplitz=True)
    refused("smaller than the reach", c, toep_reach=c["reach"] - 1)
    refused("toep_reach", c, toep_reach=-2)
    refused("shared rm", dict(c, rm=np.repeat(c["rm"][None], c["B"], axis=0)), products=2)
    refused("outlier_p", dict(c, opts=dict(c["opts"], outlier_p=0.05)), products=2)
    refused("outlier_p", dict(c, opts=dict(c["opts"], outlier_p=0.05)), products=1)
    refused("vz_offset", v, products=2)
    refused("special block", dict(d, desc=dict(d["desc"], dop_start=5, dop_size=5)))
    refused("special block", dict(d, desc=dict(d["desc"], dop_start=-1)))
    refused("vz_index", dict(v, desc=dict(v["desc"], vz_index=v["n"])))
    refused("v_baseline", dict(v, desc=dict(v["desc"], vb_start=v["n"] - 1, vb_size=2)))
    refused("num_chrono", dict(v, desc=dict(v["desc"], num_chrono=v["m"] + 1)))
    refused("one response matrix per spectrum", dict(v, rm=v["rm"][0]))
    refused("continue_mode", c, continue_mode=3)
    wide = hu.make_case(seed=5, B=1, nd=4, ns=40, m=8, desc=hu.make_desc(dop_start=0, dop_size=6))
    refused("larger than the DRT block", wide)
    # an LDS overflow is an error of the launcher, and nothing is launched: the general form at nd = 2048 needs 26623 doubles
    n, m = 2050, 24
    big = dict(c, B=1, n=n, m=m, ns=2, toeplitz=False, rm=np.zeros((m, n)), vmm=np.zeros((m, m)), mk=[np.zeros((n, n))] * 3,
               x=np.zeros((1, n)), x_in=np.zeros((1, n)), s=np.ones((1, 3, n)), rho=np.ones((1, 3)), xmx=np.ones((1, 3)), rv=np.zeros((1, m)),
               est_w=np.ones((1, m)), w=np.ones((1, m)), var_floor=np.ones(1), coef_scale=np.ones(1), qp_status=np.zeros(1),
               active=np.ones(1), fit_status=np.zeros(1), outer_iters=np.zeros(1), outlier_t=None)
    assert n + 4 * (n - 2) + 2 * (n - 2) + 3 * (2 * (n - 2) - 1) == 26623 > LDS_DOUBLES
    refused("too large for LDS", big)
