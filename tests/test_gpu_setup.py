"""GPU: what runs before the fit loop and after it (csrc/hyper.hip: prep_kernel, prep_prepared_kernel, row_mask_kernel,
init_weights_kernel, weight_method_kernel, llh_kernel and the element-wise kernels) in isolation, through the test hooks of
csrc/debug_setup.hip (include/hipdrt_debug.h), which call the launchers exactly as the plan does.

The reference is the extended-precision restatement of tests/setup_util.py, and every tolerance is the forward error bound derived in
its docstring for a float64 evaluation in any summation order (checked from both sides on the CPU, on these very inputs, by
tests/test_setup_util.py).  An error is recorded in units of its bound: every ratio in tests/_parity_measured.txt must be <= 1.
What is exact -- cs, rv, the constants, statuses and masks, the element-wise kernels -- is compared with assert_array_equal.  Every
array a launch must not write is poisoned beforehand and must come back bit for bit; on the device each has a border of marker bytes.
"""
import numpy as np
import pytest

import setup_util as su
from conftest import parity_close

pytestmark = pytest.mark.gpu

F = np.float64
P = su.POISON
SHAPES = range(len(su.INIT_SHAPES))


@pytest.fixture(scope="module")
def ctx():
    from hipdrt import _ffi
    return _ffi.get_context()


def fit_opts(o):
    from hipdrt import _ffi
    f = _ffi.default_fit_opts()
    for key, v in o.items():
        if isinstance(v, tuple):
            for k in range(3):
                getattr(f, key)[k] = v[k]
        else:
            setattr(f, key, v)
    return f


def desc_of(m, n, nc=0, dop_rho_0=su.DOP_RHO_0, uniform=0):
    from hipdrt import _ffi
    d = _ffi.PreparedDesc()
    d.m, d.n, d.ns, d.vz_index, d.num_chrono, d.chrono_vmm_uniform = m, n, 0, -1, nc, uniform
    for k in range(3):
        d.dop_rho_0[k] = dop_rho_0[k]
    return d


def poison(*shape, dtype=F):
    return np.full(shape, -77 if dtype == np.int32 else P, dtype=dtype)


def record(label, got, ref, keys):
    r = su.ratios(got, ref, keys)
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    for k, v in r.items():
        print(f"ratio {label}:{k} {v:.3g}")
        if k not in bad:
            parity_close(f"setup:{label}:{k}", v, 0.0, 1.0, scale=1.0)
    assert not bad, (label, bad)


# ---- prep -----------------------------------------------------------------------------------------------------------------------------
PREP_STATE = ("rv", "w", "s", "x", "x_in", "rho", "xmx", "coef_scale", "var_floor", "active", "outer_iters", "fit_status", "qp_iters_total")
UNTOUCHED = ("est_w", "outlier_t")


def prep_state(B, m, n, more=()):
    st = dict(rv=poison(B, m), w=poison(B, m), s=poison(B, 3, n), x=poison(B, n), x_in=poison(B, n), rho=poison(B, 3), xmx=poison(B, 3),
              coef_scale=poison(B), var_floor=poison(B), est_w=poison(B, m), outlier_t=poison(B, m))
    st.update({k: poison(B, dtype=np.int32) for k in ("active", "outer_iters", "fit_status", "qp_iters_total")})
    st.update({k: poison(B, 3) for k in more})
    return st


@pytest.mark.parametrize("nf", su.PREP_NF)
def test_prep_plain(ctx, nf):
    for n in su.PREP_N:
        for sd in (0, 1):
            c = su.cached("prep", nf, n, sd)
            ref = su.reference(su.prep, c)
            B, m = c["B"], c["m"]
            assert c["z_re"][0].argmax() == nf - 1 and c["z_re"][1].argmin() == nf - 1 and c["z_re"][0].argmin() == 0
            assert (np.abs(c["z_im"]) > np.abs(c["z_re"]).max()).all()
            got = ctx.debug_setup("prep", B, m, n, fit_opts(c["opts"]), nf=nf, z_re=c["z_re"], z_im=c["z_im"],
                                  **prep_state(B, m, n, more=("dop_rho", "dop_xmx")))
            for key in su.PREP_EXACT:
                if key in ref:
                    np.testing.assert_array_equal(got[key], ref[key], err_msg=f"nf {nf} n {n} scale_data {sd}: {key}")
            for key in UNTOUCHED + ("dop_rho", "dop_xmx"):
                assert (got[key] == P).all(), key
            record(f"prep:nf{nf}", got, ref, ("var_floor",))
            if nf == 1 and sd:
                assert not np.isfinite(got["rv"]).any()          # a single frequency has no range: the division by 0 of the reference
            # a member alone gives the bits it gives in the batch
            b = 1
            alone = ctx.debug_setup("prep", 1, m, n, fit_opts(c["opts"]), nf=nf, z_re=c["z_re"][b:b + 1], z_im=c["z_im"][b:b + 1],
                                    **prep_state(1, m, n))
            for key in PREP_STATE:
                np.testing.assert_array_equal(alone[key][0], got[key][b], err_msg=key)


@pytest.mark.parametrize("m", su.PREP_NF)
def test_prep_prepared(ctx, m):
    n = 93
    c = su.cached("prepared", m, n)
    ref = su.reference(su.prep, c)
    B = c["B"]
    st = prep_state(B, m, n, more=("dop_rho", "dop_xmx"))
    st["rv"] = c["rv"]
    got = ctx.debug_setup("prep", B, m, n, fit_opts(c["opts"]), desc=desc_of(m, n), **st)
    for key in su.PREP_EXACT:
        np.testing.assert_array_equal(got[key], ref[key], err_msg=key)
    assert (got["coef_scale"] == 1.0).all() and len(set(su.DOP_RHO_0)) == 3
    for key in UNTOUCHED:
        assert (got[key] == P).all(), key
    record(f"prep_prepared:m{m}", got, ref, ("var_floor",))


# ---- initial weights ---------------------------------------------------------------------------------------------------------------------
def init_state(c, stage, est_w=None):
    B, m, n = c["B"], c["m"], c["n"]
    st = dict(x=c["x"], rv=c["rv"], w=poison(B, m), est_w=poison(B, m) if est_w is None else est_w, var_floor=c["var_floor"],
              active=np.ones(B, dtype=np.int32), fit_status=poison(B, dtype=np.int32), outlier_t=poison(B, m),
              x_in=poison(B, n), s=poison(B, 3, n), rho=poison(B, 3), coef_scale=poison(B), outer_iters=poison(B, dtype=np.int32))
    if stage == 2:
        st["var_floor"] = poison(B)          # stage 2 takes the floor from the block's own data
    return st


def run_init(ctx, c, stage, r0=0, r1=0, al=0.0, be=1.0, row_mask=False, members=None):
    sel = slice(None) if members is None else members
    o = fit_opts(dict(c["opts"], iw_alpha=al, iw_beta=be))
    st = {k: v[sel] for k, v in init_state(c, stage, c["est_w"] if stage == 3 else None).items()}
    rm = c["rm"] if c["rm"].ndim == 2 else c["rm"][sel]
    B = len(st["x"])
    return ctx.debug_setup("init_weights", B, c["m"], c["n"], o, rm=rm, vmm=np.full((c["m"], c["m"]), P), vmm_iw=c["vmm_iw"],
                           qp_status=c["qp_status"][sel], stage=stage, r0=r0, r1=r1, row_mask=row_mask, **st), st


def check_init(label, c, got, st, ref, stage, masked=None):
    for key in su.INIT_INT:
        np.testing.assert_array_equal(got[key], ref[key], err_msg=f"{label}: {key}")
    record(label, got, ref, su.INIT_FLOAT)
    fail = c["qp_status"] < 0
    assert fail[1] and not fail[0]
    for key in ("est_w", "w", "x", "outlier_t"):           # a failed QP: nothing but active / fit_status
        np.testing.assert_array_equal(got[key][fail], np.asarray(st[key])[fail], err_msg=f"{label}: failed member, {key}")
    for key in ("rv", "var_floor", "x_in", "s", "rho", "coef_scale", "outer_iters"):
        np.testing.assert_array_equal(got[key], st[key], err_msg=f"{label}: {key} must not be written")


@pytest.mark.parametrize("si", SHAPES)
def test_init_weights_stages(ctx, si):
    m, n, ld = su.INIT_SHAPES[si]
    for batched in (0, 1):
        for op in (0.0, 0.05):
            c = su.cached("init", si, batched, op)
            assert c["rm"].shape[-1] == ld and (c["rm"].ndim == 3) == bool(batched)
            for stage, al in ((0, 0.0), (1, 0.0), (1, 2.0), (1, 0.75), (3, 0.0), (3, 2.0)):
                ref = su.reference(su.init_weights, c, stage, iw_alpha=al, iw_beta=1.5)
                got, st = run_init(ctx, c, stage, al=al, be=1.5)
                check_init(f"init:s{stage}:m{m}", c, got, st, ref, stage)
                if stage == 0:
                    assert (got["w"] == P).all() and (got["x"] == c["x"]).all()
                if stage == 1 and al == 2.0:
                    alone, _ = run_init(ctx, c, stage, al=al, be=1.5, members=slice(2, 3))
                    for key in su.INIT_FLOAT + su.INIT_INT:
                        np.testing.assert_array_equal(alone[key][0], got[key][2], err_msg=f"member 2 alone: {key}")


@pytest.mark.parametrize("si", SHAPES)
def test_init_weights_stage_two_on_a_block_diagonal_v(ctx, si):
    m, n, ld = su.INIT_SHAPES[si]
    for nc in su.stage2_ncs(m):
        c = su.cached("stage2", si, nc)
        for r0, r1 in ((0, nc), (nc, m)):
            ref = su.reference(su.init_weights, c, 2, r0, r1)
            got, st = run_init(ctx, c, 2, r0, r1, row_mask=True)
            np.testing.assert_array_equal(got["w"], su.row_mask(c["B"], m, r0, r1))
            ref = dict(ref, w=su.row_mask(c["B"], m, r0, r1))          # (the mask is written for every member, failed QP or not)
            for key in su.INIT_INT:
                np.testing.assert_array_equal(got[key], ref[key])
            record(f"init:s2:m{m}", got, ref, su.INIT_FLOAT)
            outside = np.ones(m, dtype=bool)
            outside[r0:r1] = False
            assert (got["est_w"][:, outside] == P).all() and (got["est_w"][1] == P).all() and (got["var_floor"] == P).all()


def test_init_weights_refuses_what_lds_cannot_hold(ctx):
    from hipdrt import _ffi
    m, n = 8192, 4096
    assert (n + 2 * m) * 8 > 160 * 1024 - 256
    z = np.zeros((m, m))
    with pytest.raises(_ffi.HipDrtError, match="invalid argument: initialize_weights: 163840 bytes of LDS needed .* 163584 available"):
        ctx.debug_setup("init_weights", 1, m, n, fit_opts({}), rm=z[:, :n], vmm=z, vmm_iw=z, qp_status=np.zeros(1), stage=1,
                        x=np.zeros((1, n)), rv=np.zeros((1, m)), w=np.zeros((1, m)), est_w=np.zeros((1, m)), var_floor=np.ones(1),
                        active=np.ones(1), fit_status=np.zeros(1))


# ---- the weight rule ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", su.RULE_M)
def test_weight_rule(ctx, m):
    for nc in su.rule_ncs(m):
        c = su.cached("rule", m, nc)
        assert c["est_w"].min() < 1e-8 and c["est_w"].max() > 1e4
        for fc, fe in ((0.0, 0.0), (1.75, 0.0), (0.0, 0.4), (1.75, 0.4)):
            ref = su.reference(su.weight_rule, c, fc, fe)
            B = c["B"]
            got = ctx.debug_setup("weight_method", B, m, 2, fit_opts({}), desc=desc_of(m, 2, nc), fixed_chrono=fc, fixed_eis=fe,
                                  est_w=c["est_w"], wrow=poison(B, m), wfac=poison(B, 2), w=poison(B, m))
            record(f"weight_rule:m{m}", got, ref, ("wrow", "wfac"))
            np.testing.assert_array_equal(got["est_w"], c["est_w"])
            assert (got["w"] == P).all()
            np.testing.assert_array_equal(got["wrow"][:, :nc], np.repeat(got["wfac"][:, :1], nc, 1))
            np.testing.assert_array_equal(got["wrow"][:, nc:], np.repeat(got["wfac"][:, 1:], m - nc, 1))


# ---- rss and sum log w -------------------------------------------------------------------------------------------------------------------
def run_llh(ctx, c, mode, nc, prepared, w_out, members=None):
    sel = slice(None) if members is None else members
    m, n = c["m"], c["n"]
    rm = c["rm"] if c["rm"].ndim == 2 else c["rm"][sel]
    st = dict(x=c["x"][sel], rv=c["rv"][sel], est_w=c["est_w"][sel], var_floor=c["var_floor"][sel])
    B = len(st["x"])
    st.update(rss=poison(B), slw=poison(B), w=poison(B, m), active=poison(B, dtype=np.int32))
    if w_out:
        st["w_out"] = poison(B, m)
    got = ctx.debug_setup("llh", B, m, n, fit_opts(c["opts"]), desc=desc_of(m, n, nc) if prepared else None, rm=rm, vmm=c["vmm"],
                          stored=mode, scalar_w=c["scalar_w"], **st)
    for key in ("x", "rv", "est_w", "var_floor", "w", "active"):
        np.testing.assert_array_equal(got[key], st[key], err_msg=f"{key} must not be written")
    return got


@pytest.mark.parametrize("si", SHAPES)
def test_llh_modes(ctx, si):
    m, n, ld = su.INIT_SHAPES[si]
    nc = su.llh_nc(m)
    for batched in (0, 1):
        for resid in su.LLH_RESID:
            c = su.cached("llh", si, batched, resid)
            for mode in range(4):
                plans = [(False, 0), (True, nc)] if mode != 2 else [(False, 0), (True, 0), (True, 1), (True, nc), (True, m)]
                for i, (prepared, k) in enumerate(plans):
                    ref = su.reference(su.llh, c, mode, k)
                    label = f"llh:mode{mode}:m{m}:resid{resid:g}"
                    got = run_llh(ctx, c, mode, k, prepared, w_out=True)
                    record(label, dict(rss=got["rss"], slw=got["slw"], w=got["w_out"]), ref, ("rss", "slw", "w"))
                    if mode:          # stored weights, their domain means and the scalar: the definition, bit for bit
                        np.testing.assert_array_equal(got["w_out"], np.asarray(ref["w"], dtype=F), err_msg=label)
                    if i == 0:
                        bare = run_llh(ctx, c, mode, k, prepared, w_out=False)
                        np.testing.assert_array_equal(bare["rss"], got["rss"])
                        np.testing.assert_array_equal(bare["slw"], got["slw"])
                        alone = run_llh(ctx, c, mode, k, prepared, w_out=True, members=slice(1, 2))
                        for key in ("rss", "slw", "w_out"):
                            np.testing.assert_array_equal(alone[key][0], got[key][1], err_msg=f"member 1 alone: {key}")


def test_llh_refuses_what_lds_cannot_hold(ctx):
    from hipdrt import _ffi
    m, n = 8192, 2
    assert (n + 3 * m) * 8 > 160 * 1024 - 256
    with pytest.raises(_ffi.HipDrtError, match=r"invalid argument: llh_kernel: 196624 bytes of LDS needed .* 163584 available"):
        ctx.debug_setup("llh", 1, m, n, fit_opts({}), rm=np.zeros((m, n)), vmm=np.zeros((m, m)), x=np.zeros((1, n)), rv=np.zeros((1, m)),
                        est_w=np.ones((1, m)), var_floor=np.ones(1), rss=np.zeros(1), slw=np.zeros(1))


# ---- the element-wise kernels -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("m", su.ROWOP_M)
def test_element_wise_kernels(ctx, m):
    rng = np.random.default_rng(900 + m)
    B = 3
    # vmm_exclude_self
    v = su.banded_vmm(rng, m) * 0.9
    np.testing.assert_array_equal(ctx.debug_rowop(0, poison(m, m), in0=v, m=m), su.exclude_self(v))
    # row mask through the initial-weights hook is covered there; scale_rows in every form
    w, rows_s, rows_b = rng.uniform(0.5, 2, (B, m)), rng.uniform(0.5, 2, (1, m)), rng.uniform(0.5, 2, (B, m))
    act = np.array([1, 0, 1], dtype=np.int32)
    for rows, batched in ((None, 0), (rows_s, 0), (rows_b, 1)):
        for active in (None, act):
            ref = su.scale_rows(w, None if rows is None else np.broadcast_to(rows, (B, m)), 1.37, active, poison(B, m))
            np.testing.assert_array_equal(ctx.debug_rowop(4, poison(B, m), in0=w, in1=rows, active=active, B=B, m=m, batched=batched,
                                                          factor=1.37), ref)
            ref = su.scale_rows(w, None if rows is None else np.broadcast_to(rows, (B, m)), 1.37, active, w)          # in place
            np.testing.assert_array_equal(ctx.debug_rowop(4, w, in1=rows, active=active, B=B, m=m, batched=batched, factor=1.37), ref)
    np.testing.assert_array_equal(ctx.debug_rowop(5, w, active=act, B=B, m=m, factor=0.3), su.scale_rows(w, None, 0.3, act, w))
    for n in su.ROWOP_N:
        # copy_column: a shared matrix (stride 0) and one per member (stride m ldrm)
        ld = n + 1
        rmb = rng.standard_normal((B, m, ld))
        for rm, batched in ((rmb[0], 0), (rmb, 1)):
            for col in sorted({0, n - 1}):
                np.testing.assert_array_equal(ctx.debug_rowop(6, poison(B, m), in0=rm, B=B, m=m, ld=ld, col=col, batched=batched),
                                              su.copy_column(rm, B, col))
        # assemble_rm: m rows = 2 nf needs an even m; the odd sizes run as nf = m
        nf = m
        for ns, ir, il in ((0, -1, -1), (1, 0, -1), (2, 0, 1), (2, 1, 0), (3, -1, 2)):
            nn = n + ns
            a_re, a_im, freq = rng.standard_normal((nf, n)), rng.standard_normal((nf, n)), np.logspace(5, -1, nf)
            before = poison(2 * nf, nn + 1)
            got = ctx.debug_rowop(1, before, in0=a_re, in1=a_im, in2=freq, n=nn, ns=ns, nf=nf, ld=nn + 1, idx_rinf=ir, idx_induc=il,
                                  factor=1e-5)
            np.testing.assert_array_equal(got, su.assemble_rm(a_re, a_im, freq, nn, ns, nn + 1, ir, il, 1e-5, before))
    # special_penalty and make_h at n = m
    n = m
    for ir, il in ((-1, -1), (0, -1), (n - 1, 0), (0, n - 1)):
        if ir == il and ir >= 0:
            continue
        mats = [rng.standard_normal((n, n + 1)) for _ in range(3)]
        got = ctx.debug_rowop(2, mats, n=n, ld=n + 1, idx_rinf=ir, idx_induc=il, pen_r=3.5, pen_l=0.25)
        for g, r in zip(got, su.special_penalty(mats, ir, il, 3.5, 0.25)):
            np.testing.assert_array_equal(g, r)
    for ns in sorted({0, 1, n}):
        for nonneg in (0, 1):
            np.testing.assert_array_equal(ctx.debug_rowop(3, poison(n), n=n, ns=ns, nonneg=nonneg), su.make_h(n, ns, nonneg))


# ---- refusals ---------------------------------------------------------------------------------------------------------------------------
def test_hook_refusals(ctx):
    from hipdrt import _ffi
    c = su.cached("init", 1, 0, 0.0)
    B, m, n = c["B"], c["m"], c["n"]
    o = fit_opts(c["opts"])
    base = dict(rm=c["rm"], vmm=c["vmm"], vmm_iw=c["vmm_iw"], qp_status=c["qp_status"], stage=1, **init_state(c, 1))

    def refused(match, hook="init_weights", **over):
        kw = dict(base, **over)
        with pytest.raises(_ffi.HipDrtError, match=match):
            ctx.debug_setup(hook, kw.pop("B", B), kw.pop("m", m), kw.pop("n", n), o, **{k: v for k, v in kw.items() if v is not None})

    refused("NULL pointer", x=None)
    refused("NULL pointer", vmm_iw=None)
    refused("NULL pointer", hook="llh")                                    # no rss, slw
    refused("NULL pointer", hook="prep")                                   # no z_re
    refused("ldrm >= n", rm=c["rm"][:, :n - 1])
    refused("r0 < r1 <= m", stage=2, r0=0, r1=m + 1)
    refused("r0 < r1 <= m", stage=2, r0=3, r1=3)
    refused("r0 < r1 <= m", row_mask=True, r0=-1, r1=2)
    refused("stage", stage=4)
    bad = c["rv"].copy()
    bad[0, 3] = np.nan
    refused("non-finite", rv=bad)
    bad = c["rm"].copy()
    bad[2, 1] = np.inf
    refused("non-finite", rm=bad)
    with pytest.raises(_ffi.HipDrtError, match="0 < num_chrono < m"):
        ctx.debug_setup("weight_method", B, m, n, o, desc=desc_of(m, n, m), est_w=c["est_w"], wrow=poison(B, m), wfac=poison(B, 2))
    with pytest.raises(_ffi.HipDrtError, match="num_chrono"):
        ctx.debug_setup("llh", B, m, n, o, desc=desc_of(m, n, m + 1), rm=c["rm"], vmm=c["vmm"], x=c["x"], rv=c["rv"], est_w=c["est_w"],
                        var_floor=c["var_floor"], rss=poison(B), slw=poison(B))
    with pytest.raises(_ffi.HipDrtError, match="stored"):
        ctx.debug_setup("llh", B, m, n, o, rm=c["rm"], vmm=c["vmm"], x=c["x"], rv=c["rv"], est_w=c["est_w"], var_floor=c["var_floor"],
                        rss=poison(B), slw=poison(B), stored=4)
    with pytest.raises(_ffi.HipDrtError, match="col < ld"):
        ctx.debug_rowop(6, poison(B, m), in0=c["rm"], B=B, m=m, ld=c["rm"].shape[-1], col=c["rm"].shape[-1])
    with pytest.raises(_ffi.HipDrtError, match="in0 = vmm"):
        ctx.debug_rowop(0, poison(m, m), m=m)                                # no input matrix


def test_prepared_plan_refuses_a_v_with_cross_blocks_for_separate_initial_weights(ctx):
    """stage 2 of init_weights_kernel multiplies the whole V: hipdrt_plan_create_prepared must see that the cross blocks are zero"""
    from hipdrt import _ffi
    c = su.cached("stage2", 1, 31)
    m, n = c["m"], c["n"]

    def create(vmm, separately, nc):
        d = desc_of(m, n, nc)
        d.init_weights_separately = separately
        _ffi.PreparedPlan(ctx, d, [np.eye(n)] * 3, vmm, np.zeros(n), np.zeros(n), capacity=2).close()

    create(c["vmm"], 1, 31)                                  # block diagonal
    with pytest.raises(_ffi.HipDrtError, match="zero outside its chrono and impedance blocks"):
        create(c["vmm_cross"], 1, 31)
    only_upper = c["vmm"].copy()
    only_upper[30, 31] = 1e-300
    with pytest.raises(_ffi.HipDrtError, match="zero outside its chrono and impedance blocks"):
        create(only_upper, 1, 31)
    create(c["vmm_cross"], 0, 31)                            # not asked for, or a single block: nothing to refuse
    create(c["vmm_cross"], 1, 0)
    create(c["vmm_cross"], 1, m)
