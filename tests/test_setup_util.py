"""CPU: the numpy reference of tests/test_gpu_setup.py (tests/setup_util.py) is itself checked, on the very inputs the GPU tests use --
(a) its derived bounds hold for a float64 evaluation in other summation orders, with and without fused products; (b) they bite: every
listed mutant leaves its output's bound by a factor 10 at least, on every case it applies to; (c) the float64 restatement agrees with
the oracle within the same bounds; (d) no case leaves more than 2 % of an output's entries out of a value comparison."""
import inspect

import numpy as np
import pytest

import setup_util as su

F = np.float64
SHAPES = range(len(su.INIT_SHAPES))
SMALL = [i for i in SHAPES if su.INIT_SHAPES[i][0] <= 142]
CAP = 0.02


def perm(seed):
    rng = np.random.default_rng(seed)
    return lambda k: rng.permutation(k)


def worst(got, ref, keys):
    return max(su.ratios(got, ref, keys).values())


def shuffled(c, seed):
    """the same case with the columns of rm (and x) and the rows of the data (with the variance matrix) in another order: every sum
    of a float64 evaluation then runs in another order.  -> (case, row permutation)"""
    rng = np.random.default_rng(seed)
    pc, pr = rng.permutation(c["n"]), rng.permutation(c["m"])
    rm = c["rm"][..., :c["n"]]
    d = dict(c, rm=np.ascontiguousarray(rm[..., pr, :][..., pc]), x=c["x"][:, pc], rv=c["rv"][:, pr], est_w=c["est_w"][:, pr])
    for k in ("vmm", "vmm_iw", "vmm_cross"):
        d[k] = np.ascontiguousarray(c[k][pr][:, pr])
    return d, pr


# ---- prep -----------------------------------------------------------------------------------------------------------------------------
def prep_cases():
    for nf in su.PREP_NF:
        for n in su.PREP_N:
            for sd in (0, 1):
                yield su.cached("prep", nf, n, sd)
        yield su.cached("prepared", nf, 93)


def test_prep_floor_bound_holds_and_bites():
    for c in prep_cases():
        ref = su.reference(su.prep, c)
        f64 = su.prep(c)
        for key in su.PREP_EXACT:
            if key in ref:
                np.testing.assert_array_equal(f64[key], ref[key])
        assert worst(f64, ref, ("var_floor",)) <= 1.0
        finite = np.isfinite(np.asarray(ref["var_floor"], dtype=F))
        if c["m"] > 1 and finite.all():
            for seed in range(3):          # another order of the two sums
                p = np.random.default_rng(seed).permutation(c["m"])
                other = np.array([su.var_floor(su._Arith(F), f64["rv"][b][p]) for b in range(c["B"])])
                assert worst(dict(var_floor=other), ref, ("var_floor",)) <= 1.0
            assert su.ratios(su.prep(c, mutant="ddof1"), ref, ("var_floor",))["var_floor"] >= 10.0
        if not c["prepared"] and c["opts"]["scale_data"] and c["nf"] > 1:
            assert not np.array_equal(su.prep(c, mutant="range_all")["coef_scale"], ref["coef_scale"])


# ---- initial weights ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", SHAPES)
def test_init_weights_bounds_hold_bite_and_keep_the_cap(si):
    m = su.INIT_SHAPES[si][0]
    for batched in (0, 1):
        for op in (0.0, 0.05):
            c = su.cached("init", si, batched, op)
            for al in (0.0, 2.0, 0.75):
                ref = su.reference(su.init_weights, c, 1, iw_alpha=al, iw_beta=1.5)
                assert su.exclusion_share(ref) <= CAP
                assert worst(su.init_weights(c, 1, iw_alpha=al, iw_beta=1.5), ref, su.INIT_FLOAT) <= 1.0
                if al > 0:
                    assert su.ratios(su.init_weights(c, 1, iw_alpha=al, iw_beta=1.5, mutant="b_plus"), ref, ("w",))["w"] >= 10.0
            ref = su.reference(su.init_weights, c, 1)
            if op == 0.0:
                d, pr = shuffled(c, 11 + si)
                got = su.init_weights(d, 1)
                back = {k: (np.empty_like(got[k]) if k != "x" else got[k]) for k in su.INIT_FLOAT}
                for k in ("est_w", "w", "outlier_t"):
                    back[k][:, pr] = got[k]
                assert worst(back, ref, ("est_w", "w")) <= 1.0
                live = [b for b in range(c["B"]) if c["qp_status"][b] >= 0]
                orders = [dict(perm=perm(s)) for s in (1, 2)] + ([dict(fma=True), dict(fma=True, perm=perm(3))] if m <= 142 else [])
                for kw in orders:
                    for b in live:
                        w = su._weights64(c, b, c["vmm_iw"], c["var_floor"][b], **kw)
                        assert np.all(np.abs(w - np.asarray(ref["est_w"][b], dtype=F)) <= ref["bound"]["est_w"][b])
                # both branches of the floor and of the clip are taken where the shape has room for them
                if m >= 33:
                    b = live[0]
                    w = np.asarray(ref["est_w"][b], dtype=F)
                    assert np.isclose(w, c["var_floor"][b] ** -0.5, rtol=1e-9).any() and (w < 0.5 * c["var_floor"][b] ** -0.5).any()
                    assert (np.asarray(ref["est_w"][live[-1]], dtype=F) == 1e-10).any() and (w > 1e-10).all()
                    for mutant in ("floor_after", "no_clip", "ddof1"):
                        assert su.ratios(su.init_weights(c, 0, mutant=mutant), ref, ("est_w",))["est_w"] >= 10.0, mutant


@pytest.mark.parametrize("si", SHAPES)
def test_stage_two_bounds_hold_and_bite(si):
    m = su.INIT_SHAPES[si][0]
    for nc in su.stage2_ncs(m):
        c = su.cached("stage2", si, nc)
        assert not c["vmm"][:nc, nc:].any() and not c["vmm"][nc:, :nc].any() and (m < 4 or c["vmm_cross"][:nc, nc:].any())
        for r0, r1 in ((0, nc), (nc, m)):
            ref = su.reference(su.init_weights, c, 2, r0, r1)
            assert su.exclusion_share(ref) <= CAP
            assert worst(su.init_weights(c, 2, r0, r1), ref, su.INIT_FLOAT) <= 1.0
            b = 0
            w = np.asarray(ref["est_w"][b, r0:r1], dtype=F)
            vf = float(su.var_floor(su._Arith(F), c["rv"][b, r0:r1]))
            floored = vf > 0 and np.isclose(w, vf ** -0.5, rtol=1e-9).any()
            bite = lambda mutant: su.ratios(su.init_weights(c, 2, r0, r1, mutant=mutant), ref, ("est_w",))["est_w"]
            if floored:                                    # the floor only shows where an entry lies under it
                assert bite("floor_whole") >= 10.0 and bite("floor_after") >= 10.0
                if r1 - r0 > 1:
                    assert bite("ddof1") >= 10.0
            if m >= 4:
                assert bite("full_v") >= 10.0              # a cross block that is not zero reaches the rows next to the split


# ---- the weight rule ---------------------------------------------------------------------------------------------------------------------
def test_weight_rule_bounds_hold_and_bite():
    for m in su.RULE_M:
        for nc in su.rule_ncs(m):
            c = su.cached("rule", m, nc)
            for fc, fe in ((0.0, 0.0), (1.75, 0.0), (0.0, 0.4), (1.75, 0.4)):
                ref = su.reference(su.weight_rule, c, fc, fe)
                assert worst(su.weight_rule(c, fc, fe), ref, ("wrow", "wfac")) <= 1.0
                for seed in (1, 2):
                    p0, p1 = np.random.default_rng(seed).permutation(nc), nc + np.random.default_rng(seed).permutation(m - nc)
                    d = dict(c, est_w=c["est_w"][:, np.concatenate([p0, p1])])
                    assert worst(su.weight_rule(d, fc, fe), ref, ("wfac",)) <= 1.0
                if fc == 0.0 and fe == 0.0:
                    for mutant in ("mean_w", "half", "swap") if m > 2 else ("half", "swap"):       # (one row: both means are it)
                        assert su.ratios(su.weight_rule(c, mutant=mutant), ref, ("wfac",))["wfac"] >= 10.0, (m, nc, mutant)


# ---- rss and sum log w -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("si", SHAPES)
def test_llh_bounds_hold_for_the_three_sum_form_and_bite(si):
    m = su.INIT_SHAPES[si][0]
    nc = su.llh_nc(m)
    for batched in (0, 1):
        for resid in su.LLH_RESID:
            c = su.cached("llh", si, batched, resid)
            for mode in range(4):
                for k in sorted({0, nc} if mode != 2 else {0, 1, nc, m}):
                    ref = su.reference(su.llh, c, mode, k)
                    f64 = su.llh(c, mode, k)
                    assert worst(f64, ref, ("rss", "slw", "w")) <= 1.0
                    W = np.asarray(ref["w"], dtype=F)
                    for kw in [dict(), dict(perm=perm(1)), dict(perm=perm(2))] + ([dict(fma=True)] if m <= 142 else []):
                        rss, slw = su.three_sums(c, f64["w"], **kw)
                        assert worst(dict(rss=rss, slw=slw), ref, ("rss", "slw")) <= 1.0, (mode, k, kw)
                    bite = lambda mutant: su.ratios(su.llh(c, mode, k, mutant=mutant, weights=None if mutant == "split_half" else W),
                                                    ref, ("rss", "slw", "w"))
                    assert bite("plus2c")["rss"] >= 10.0 and bite("logw2")["slw"] >= 10.0
                    if mode == 2 and 0 < k < m and k != m // 2:
                        assert bite("split_half")["w"] >= 10.0
            if resid == su.LLH_RESID[0] and m >= 33:
                # a good fit: the three sums cancel to a small part of their size (what the bound is there for)
                ref = su.reference(su.llh, c, 1, 0)
                y = np.array([su._rmb(c, b) @ c["x"][b] for b in range(c["B"])])
                a = ((c["est_w"] * y) ** 2).sum(axis=1)
                assert np.all(np.asarray(ref["rss"], dtype=F) < 1e-3 * a)


# ---- the element-wise operations ------------------------------------------------------------------------------------------------------------
def test_element_wise_mutants_change_bits():
    rng = np.random.default_rng(5)
    v = su.banded_vmm(rng, 9)
    assert not np.array_equal(su.exclude_self(v), su.exclude_self(v, "dj"))
    a, f = rng.standard_normal((4, 3)), np.logspace(3, 0, 4)
    kw = dict(n=5, ns=2, ld=6, idx_rinf=0, idx_induc=1, inductance_scale=1e-5, before=np.full((8, 6), su.POISON))
    r = su.assemble_rm(a, -a, f, **kw)
    assert not np.array_equal(r, su.assemble_rm(a, -a, f, mutant="no_lscale", **kw))
    assert (r[:, 5] == su.POISON).all() and (r[:4, 0] == 1).all() and (r[4:, 0] == 0).all() and (r[:4, 1] == 0).all()
    np.testing.assert_array_equal(su.make_h(5, 2, 0), [0, 0, 1e5, 1e5, 1e5])
    np.testing.assert_array_equal(su.make_h(5, 2, 1), np.zeros(5))
    np.testing.assert_array_equal(su.row_mask(2, 5, 1, 3), [[0, 1, 1, 0, 0]] * 2)


# ---- (c) the oracle ---------------------------------------------------------------------------------------------------------------------------
def test_restatement_matches_the_oracle():
    from oracle import drt_oracle as orc
    from scipy.special import loggamma
    src = inspect.getsource(orc.qphb_fit_prepared).splitlines()

    def run_lines(first, count, **names):
        """the oracle's own lines, from the one that starts with `first`, executed on `names`"""
        at = [i for i, line in enumerate(src) if line.strip().startswith(first)]
        assert len(at) == 1, first
        ns = dict(np=np, **names)
        exec("\n".join(line.strip() for line in src[at[0]:at[0] + count]), ns)
        return ns
    for si in SMALL:
        m, n, _ = su.INIT_SHAPES[si]
        for op in (0.0, 0.05):
            c = su.cached("init", si, 0, op)
            ref = su.reference(su.init_weights, c, 1, iw_alpha=2.0, iw_beta=1.5)
            for b in (0, 2):
                # the oracle takes its floor from the data itself: the case's var_floor is np.var(rv) * 1e-7 as well
                w = orc.estimate_weights(c["x"][b], c["rv"][b], c["vmm_iw"], su._rmb(c, b), None, op if op > 0 else None)
                ex = ref["exclude"]["est_w"][b]
                assert np.all((np.abs(w - np.asarray(ref["est_w"][b], dtype=F)) <= ref["bound"]["est_w"][b]) | ex)
                w2 = orc.solve_init_weight_scale(w, 2.0, 1.5)
                assert np.all((np.abs(w2 - np.asarray(ref["w"][b], dtype=F)) <= ref["bound"]["w"][b]) | ex)
            if op > 0:
                got = run_lines("vmm_iw = (vmm", 1, vmm=c["vmm"])["vmm_iw"]
                np.testing.assert_array_equal(got, su.exclude_self(c["vmm"]))
        for resid in su.LLH_RESID:
            c = su.cached("llh", si, 0, resid)
            for mode in (0, 1):
                ref = su.reference(su.llh, c, mode, 0)
                for b in range(c["B"]):
                    w = np.asarray(ref["w"][b], dtype=F)
                    rm, x, rv = su._rmb(c, b), c["x"][b], c["rv"][b]
                    rss = orc.evaluate_rss(x, rm, rv, w)
                    assert abs(rss - float(ref["rss"][b])) <= ref["bound"]["rss"][b]
                    rest = 2 * np.log(1) - (2 - 1 + m / 2) * np.log(1 + 0.5 * rss) + loggamma(2 - 1 + m / 2) - loggamma(2)
                    full = orc.evaluate_llh(x, rm, rv, w)
                    # (the subtraction that isolates sum log w rounds once at the size of its operands)
                    assert abs((full - rest) - float(ref["slw"][b])) <= ref["bound"]["slw"][b] + 4 * su.U * (abs(full) + abs(rest))
    for m in su.RULE_M:
        for nc in su.rule_ncs(m):
            c = su.cached("rule", m, nc)
            ref = su.reference(su.weight_rule, c)
            for b in range(c["B"]):
                rows = run_lines("cws = np.mean", 4, est_weights=c["est_w"][b], nc=nc, rzv=np.zeros(m))["row_factors"]
                assert np.all(np.abs(rows - np.asarray(ref["wrow"][b], dtype=F)) <= ref["bound"]["wrow"][b])
