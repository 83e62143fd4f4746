"""GPU: the coneqp launch in the fit loop's own form and at every exit, through hipdrt_debug_qp (include/hipdrt_debug.h): P as packed tiles
only, an active mask, the dispatch-order table, iters_accum, non-default options, s and z back from the device.  Every call goes through
the hook's borders of marker bytes (in/out arrays, per-problem state blocks and factor scratch, the group kernel's sync words): a write
outside any of them raises.  References and the inputs' preconditions: tests/qp_util.py, pinned on the CPU by tests/test_qp_util.py.

Measured on an MI355X, test_carried_product: largest |x - oracle's x| over the three kernel forms, beside the oracle's sensitivity
(its own movement under a relative 1e-13 perturbation of P and q; the bound is 10 x that) and what a library built with the rule
switched off gave (kDriftTol = 1e30 for far / neg; kCancUlps = 0 changes nothing at the default tolerances):
    input          deviation   sensitivity   rule off            input          deviation   sensitivity
    far (33, 22)   4.3e-14     6.9e-12       1.5e-10  fails      bad (17, 8)    9.3e-10     1.8e-07
    far (33, 23)   1.5e-14     6.8e-12       2.4e-10  fails      bad (17, 11)   4.9e-08     1.0e-07
    far (97, 15)   4.6e-14     1.3e-11       1.3e-09  fails      bad (33, 7)    3.7e-09     1.5e-06
    far (97, 19)   4.8e-13     2.4e-11       1.2e-09  fails      bad (33, 8)    1.3e-09     1.7e-07
    neg QP 0       3.8e-10     1.2e-07       4.5e-06  fails      bad (33, 9)    7.0e-09     5.8e-07
    neg QP 1       7.4e-13     1.3e-10       7.5e-12             bad (65, 0)    5.3e-10     3.9e-07
    neg QP 2       1.1e-12     2.5e-10       1.8e-11             bad (65, 10)   3.3e-09     4.8e-07
The true dual residual of the far-start results equals the model's to two digits (2.4e-13 .. 1.3e-12).
test_cancellation_rule_retakes_the_verdict (tight tolerances), true dual residual of the returned point / allowed / with kCancUlps = 0:
    bad (17, 143)  2.9e-11 (batch forms, 17 iterations), 4.9e-11 (group form, 16)  /  2.2e-10  /  2.0e-09 (batch forms: fails), 4.9e-11 (group)
    bad (33, 136)  1.5e-11 (batch forms, 17 iterations), 5.4e-11 (group form, 17)  /  9.9e-10  /  3.8e-09 (batch forms: fails), 8.6e-10 (group)
"""
import contextlib
import functools

import numpy as np
import pytest

import qp_util as qu

pytestmark = pytest.mark.gpu

B = 9           # odd, and one more than the group kernel's round of eight problems

# kernel forms, each at the smallest shapes at which it still has its structure: name -> (group switch, waves switch, sizes, the form
# the hook must report: workgroups per problem, inverse blocks in global memory, wavefronts)
FORMS = {
    "batch8": (0, 8, (1, 17, 33, 65), lambda n: (0, 0, 8)),
    "fat4": (0, 4, (1, 17, 33, 65), lambda n: (0, 0, 4)),
    "global_u": (0, -1, (529,), lambda n: (0, 1, 8)),
    "group3": (3, -1, (97,), lambda n: (3, 0, 8)),
    "group8": (8, -1, (545,), lambda n: (8, 0, 8)),
}
CASES = [pytest.param(f, n, id=f"{f}-n{n}") for f, (_, _, ns, _) in FORMS.items() for n in ns]
# the forms a small problem can run in (carried-product inputs, n = 17 .. 97): the group switch gives min(3, block rows / 2) members
SMALL_FORMS = {"batch8": (0, 8, lambda n: (0, 0, 8)), "fat4": (0, 4, lambda n: (0, 0, 4)),
               "group": (3, -1, lambda n: (max(1, min(3, ((n + 15) // 16) // 2)), 0, 8))}


@pytest.fixture(scope="module")
def ctx():
    from hipdrt import _ffi
    return _ffi.Context(0)


@contextlib.contextmanager
def switches(ctx, group, waves):
    try:
        ctx.debug_qp_group(group)
        ctx.debug_qp_waves(waves)
        yield
    finally:
        ctx.debug_qp_group(-1)
        ctx.debug_qp_waves(-1)


@contextlib.contextmanager
def form(ctx, name):
    group, waves, _, _ = FORMS[name]
    with switches(ctx, group, waves):
        yield


def assert_form(res, name, n):
    assert tuple(res["form"]) == FORMS[name][3](n), (name, n, res["form"])


def qp_opts(**kw):
    from hipdrt import _ffi
    o = qu.opts_dict(kw)
    return _ffi.QpOpts(o["abstol"], o["reltol"], o["feastol"], o["maxiters"])


@functools.lru_cache(maxsize=None)
def problems(n):
    """B well-conditioned random problems of n unknowns and the oracle's results, computed once"""
    Ps, qs, hs = zip(*[qu.spd(n, [n, b]) for b in range(B)])
    P, q, h = np.stack(Ps), np.stack(qs), np.stack(hs)
    for a in (P, q, h):
        a.setflags(write=False)
    return P, q, h, tuple(qu.oracle(P[b], q[b], h[b]) for b in range(B))


@functools.lru_cache(maxsize=None)
def oracle_at(n, b, key):
    P, q, h, _ = problems(n)
    return qu.oracle(P[b], q[b], h[b], dict(key))


def same_bits(a, b, rows=None, keys=("x", "iterations", "pcost", "status")):
    for k in keys:
        u, v = (a[k], b[k]) if rows is None else (a[k][rows], b[k][rows])
        np.testing.assert_array_equal(u, v, err_msg=k)


def x_close(x, ref):
    """the tolerance of test_gpu_qp.py::test_qp_random_spd_vs_oracle"""
    np.testing.assert_allclose(x, ref, rtol=1e-8, atol=1e-9 * max(1.0, np.abs(ref).max()))


def earned(P, q, h, res, b, ref, opts=None, xtol=None):
    """e: a status-0 result has earned its verdict -- in extended precision the returned (x, s, z) passes coneqp's stopping test (dual
    residual within 1.05 feastol plus the rounding bound of one direct product, primal residual within feastol plus a few eps, s, z > 0,
    gap or relative gap inside its tolerance), and s and z are the oracle's at the tolerance used for x"""
    assert res["status"][b] == 0
    x, s, z = res["x"][b], res["s"][b], res["z"][b]
    k = qu.kkt_check(P, q, h, x, s, z, opts)
    print(f"kkt b={b}: dres {k['dres']:.2e} (+{k['dres_bound']:.1e}) pres {k['pres']:.2e} gap {k['gap']:.2e} relgap {k['relgap']}")
    o = qu.opts_dict(opts)
    assert k["dres"] <= 1.05 * o["feastol"] + k["dres_bound"], k
    assert k["pres"] <= o["feastol"] + k["pres_bound"], k
    assert np.all(s > 0) and np.all(z > 0)
    assert k["gap"] <= o["abstol"] or (k["relgap"] is not None and k["relgap"] <= o["reltol"]), k
    assert k["ok"]
    if ref is not None:
        close = x_close if xtol is None else (lambda a, r: np.testing.assert_allclose(a, r, rtol=0, atol=xtol * np.abs(r).max()))
        close(s, ref["s"])
        close(z, ref["z"])
    return k


# ---- a. the loop's form gives the bits of the stand-alone form ------------------------------------------------------------------
@pytest.mark.parametrize("shared", [False, True], ids=["batched_p", "shared_p"])
@pytest.mark.parametrize("name,n", CASES)
def test_loop_form_equals_the_stand_alone_form(ctx, name, n, shared):
    P, q, h, refs = problems(n)
    Pa, ha = (P[0], h[0]) if shared else (P, h)          # shared: one P with stride 0 (initialize_weights), one h
    with form(ctx, name):
        alone = ctx.qp_batch(Pa, q, ha)
        res = ctx.debug_qp(Pa, q, ha)
    assert_form(res, name, n)
    same_bits(res, alone)
    assert res["iters_accum"].tolist() == res["iterations"].tolist()
    assert res["order"].tolist() == list(range(B))
    for b in range(B):
        ref = refs[b] if not shared else (refs[0] if b == 0 else qu.oracle(P[0], q[b], h[0]))
        assert res["status"][b] == 0 and res["iterations"][b] == ref["iterations"]
        x_close(res["x"][b], ref["x"])
        earned(Pa if shared else P[b], q[b], ha if shared else h[b], res, b, ref)


# ---- b. the active mask ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", CASES)
def test_active_mask(ctx, name, n):
    P, q, h, _ = problems(n)
    active = np.array([0, 1, 1, 1, 0, 1, 1, 1, 0], dtype=np.int32)         # inactive first, in the middle, last
    on, off = active == 1, active == 0
    with form(ctx, name):
        full = ctx.debug_qp(P, q, h)
        one = ctx.debug_qp(P, q, h, active=active, iters_accum=np.full(B, 5))
        two = ctx.debug_qp(P, q, h, active=active, iters_accum=one["iters_accum"])
    for res in (full, one, two):
        assert_form(res, name, n)
    for res in (one, two):
        same_bits(res, full, rows=on)
        assert np.all(res["x"][off] == 7e77) and np.all(res["pcost"][off] == 7e77)
        assert np.all(res["iterations"][off] == -7) and np.all(res["status"][off] == -7)
        assert np.all(np.isnan(res["s"][off])) and np.all(np.isfinite(res["s"][on]))
    it = np.where(on, full["iterations"], 0)
    assert one["iters_accum"].tolist() == (5 + it).tolist()
    assert two["iters_accum"].tolist() == (5 + 2 * it).tolist()           # inactive slots keep what went in


# ---- c. the dispatch order -----------------------------------------------------------------------------------------------------------
def lpt_reference(iters, active=None):
    key = np.asarray(iters, dtype=np.int64).copy()
    if active is not None:
        key[np.asarray(active) == 0] = -1
    return np.lexsort((np.arange(key.size), -key))


@pytest.mark.parametrize("name,n", CASES)
def test_dispatch_order(ctx, name, n):
    P, q, h, refs = problems(n)
    rng = np.random.default_rng(n)
    prev = np.array([r["iterations"] for r in refs], dtype=np.int32)[::-1].copy()      # "the previous solve's counts"
    with form(ctx, name):
        plain = ctx.debug_qp(P, q, h)
        outs = {}
        for tag, order in (("identity", np.arange(B)), ("reversed", np.arange(B)[::-1]), ("random", rng.permutation(B))):
            outs[tag] = ctx.debug_qp(P, q, h, order=order)
            assert outs[tag]["order"].tolist() == list(order)
        outs["lpt"] = ctx.debug_qp(P, q, h, use_lpt=True, iters=prev)
        active = np.array([1, 1, 0, 1, 1, 1, 0, 1, 1], dtype=np.int32)
        masked = ctx.debug_qp(P, q, h, use_lpt=True, iters=prev, active=active)
    assert outs["lpt"]["order"].tolist() == lpt_reference(prev).tolist()
    assert masked["order"].tolist() == lpt_reference(prev, active).tolist()
    for tag, res in outs.items():
        assert_form(res, name, n)
        same_bits(res, plain)               # (the group kernel ignores the table: unchanged as well)
    same_bits(masked, plain, rows=active == 1)
    assert np.all(masked["status"][active == 0] == -7)


@pytest.mark.parametrize("nb", [1, 15, 16, 17, 257, 4096])
def test_lpt_order_kernel(ctx, nb):
    """lpt_order_kernel alone against numpy.lexsort on (index, -key), key -1 for inactive problems: exact"""
    rng = np.random.default_rng(nb)
    some = (rng.random(nb) < 0.7).astype(np.int32)
    cases = [(rng.integers(0, 4, nb), None), (rng.integers(0, 4, nb), some), (np.full(nb, 6), None), (np.full(nb, 6), some),
             (rng.integers(0, 100, nb), np.zeros(nb, dtype=np.int32)), (rng.permutation(nb), None), (np.arange(nb), some),
             (np.zeros(nb, dtype=np.int32), None)]
    for iters, active in cases:
        got = ctx.debug_lpt_order(iters, active)
        np.testing.assert_array_equal(got, lpt_reference(iters, active))


def test_hook_refuses_what_it_cannot_run(ctx):
    from hipdrt import _ffi
    P, q, h, _ = problems(17)
    for order in ([0] * B, list(range(1, B + 1)), [-1] + list(range(1, B))):
        with pytest.raises(_ffi.HipDrtError, match="permutation"):
            ctx.debug_qp(P, q, h, order=order)
    bad = q.copy()
    bad[3, 5] = np.nan
    with pytest.raises(_ffi.HipDrtError, match="non-finite"):
        ctx.debug_qp(P, bad, h)
    with pytest.raises(_ffi.HipDrtError):
        ctx.debug_lpt_order(np.zeros(48 * 1024 // 4 + 1, dtype=np.int32))
    with switches(ctx, 0, -1), pytest.raises(_ffi.HipDrtError):
        ctx.debug_qp(np.eye(2049), np.zeros((1, 2049)), np.zeros(2049))


# ---- d. the exits ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,n", CASES)
def test_exit_at_maxiters(ctx, name, n):
    """maxiters = k < the oracle's count: status 1 after exactly k iterations, x and pcost those of coneqp_boxlow(maxiters=k);
    k = it and it + 1: status 0 after it iterations (cvxopt: converged at the last test counts as optimal)"""
    P, q, h, refs = problems(n)
    its = np.array([r["iterations"] for r in refs])
    it0 = int(its[0])
    with form(ctx, name):
        for k in sorted({0, 1, 3, it0 - 1, it0, it0 + 1}):
            res = ctx.debug_qp(P, q, h, opts=qp_opts(maxiters=k))
            assert_form(res, name, n)
            for b in range(B):
                ref = oracle_at(n, b, (("maxiters", k),))
                want = 1 if k < its[b] else 0
                assert res["status"][b] == want == qu.oracle_code(ref, dict(maxiters=k)), (k, b)
                assert res["iterations"][b] == min(k, its[b]) == ref["iterations"]
                x_close(res["x"][b], ref["x"])
                assert abs(res["pcost"][b] - ref["primal objective"]) <= 1e-9 * abs(ref["primal objective"])
                if want == 0:
                    earned(P[b], q[b], h[b], res, b, ref)
    assert it0 - 1 > 0 and np.all(its > 3)               # every k below it0 was an early exit of problem 0, k <= 3 of every problem


@pytest.mark.parametrize("name,n", CASES)
def test_tolerances_move_the_exit(ctx, name, n):
    P, q, h, refs = problems(n)
    default = np.array([r["iterations"] for r in refs])
    with form(ctx, name):
        for o in (qu.LOOSE, qu.TIGHT):
            res = ctx.debug_qp(P, q, h, opts=qp_opts(**o))
            assert_form(res, name, n)
            want = np.array([oracle_at(n, b, tuple(sorted(o.items())))["iterations"] for b in range(B)])
            assert res["status"].tolist() == [0] * B
            assert res["iterations"].tolist() == want.tolist()
            assert np.all(want != default)
            for b in range(B):
                earned(P[b], q[b], h[b], res, b, None, opts=o)


@pytest.mark.parametrize("name,n", [c for c in CASES if c.values[1] > 1])
def test_late_breakdown_in_a_batch(ctx, name, n):
    """one member whose factorisation breaks down in iteration 2 among ordinary ones: status 2 for it alone, the oracle's count and
    last iterate; the others as in a launch without it"""
    P, q, h, _ = problems(n)
    Pl, ql, hl = qu.late_breakdown(n)
    ref = qu.oracle(Pl, ql, hl)
    at = 4
    P2, q2, h2 = P.copy(), q.copy(), h.copy()
    P2[at], q2[at], h2[at] = Pl, ql, hl
    others = np.arange(B) != at
    with form(ctx, name):
        plain = ctx.debug_qp(P, q, h)
        res = ctx.debug_qp(P2, q2, h2)
    assert_form(res, name, n)
    assert res["status"][at] == 2 and res["iterations"][at] == ref["iterations"] == 2
    x_close(res["x"][at], ref["x"])
    assert res["iters_accum"][at] == 2
    same_bits(res, plain, rows=others, keys=("x", "iterations", "pcost", "status", "s", "z"))


# ---- f. the carried product --------------------------------------------------------------------------------------------------------------
CARRIED = ([("far", k) for k in qu.FAR_INPUTS] + [("neg", (i,)) for i in range(3)] + [("bad", k) for k in qu.CANC_DEFAULT])


@functools.lru_cache(maxsize=None)
def carried_reference(kind, key):
    P, q, h = qu.named_input(kind, *key)
    return P, q, h, qu.oracle(P, q, h), qu.sensitivity(P, q, h), qu.carried_model(P, q, h)


@pytest.mark.parametrize("fname", list(SMALL_FORMS))
@pytest.mark.parametrize("kind,key", [pytest.param(k, key, id=f"{k}-{'-'.join(map(str, key))}") for k, key in CARRIED])
def test_carried_product(ctx, kind, key, fname):
    """Inputs on which the drift rule (far, neg) or the cancellation rule (bad) fires: status and iteration count are the oracle's and x
    lies within max(10 x sensitivity, 1e-12 max|x|) of it -- the reference's own movement under a 1e-13 perturbation of its input sets the
    scale, the factor 10 covers another summation order in the factorisation.  For the far-start inputs the true dual residual of the
    returned point is within ten times the model's as well (without the drift rule the model's grows by a factor 50 to 7000)."""
    P, q, h, ref, sens, model = carried_reference(kind, key)
    n = q.size
    group, waves, want = SMALL_FORMS[fname]
    with switches(ctx, group, waves):
        res = ctx.debug_qp(P, q[None], h)
    assert tuple(res["form"]) == want(n)
    assert res["status"][0] == 0 and ref["status"] == "optimal"
    assert res["iterations"][0] == ref["iterations"]
    peak = np.abs(ref["x"]).max()
    dev, bound = np.abs(res["x"][0] - ref["x"]).max(), max(10 * sens, 1e-12 * peak)
    print(f"carried {kind} {key} {fname}: |x - oracle| {dev:.2e} sensitivity {sens:.2e} bound {bound:.2e} peak {peak:.2e}")
    assert dev <= bound
    k = earned(P, q, h, res, 0, ref, xtol=bound / peak)
    if kind == "far":
        print(f"carried {kind} {key} {fname}: true dres {k['dres']:.2e} model {model['true_dres']:.2e}")
        assert k["dres"] <= 10 * model["true_dres"]


@pytest.mark.parametrize("fname", list(SMALL_FORMS))
@pytest.mark.parametrize("n,seed", qu.CANC_TIGHT)
def test_cancellation_rule_retakes_the_verdict(ctx, n, seed, fname):
    """Tight tolerances on a badly scaled problem: in the CPU model the carried residual passes the stopping test while the direct
    product the rule asks for does not (both by a factor >= 2, tests/test_qp_util.py).  What the carried product is off by is rounding
    noise, so the kernel either finds its own direct product inside feastol and stops where it would without the rule, or goes on for
    one more iteration; either way the point it returns has a TRUE dual residual (extended precision) within 1.05 feastol plus the
    typical rounding of the one direct FP64 product that passed, sqrt(n + 2) eps | |P||x| + |q| + |z| | / resx0.  Without the rule the
    model's point lies a factor 2 to 30 beyond that (pinned in tests/test_qp_util.py)."""
    P, q, h = qu.badly_scaled(n, seed)
    off = qu.carried_model(P, q, h, qu.TIGHT, canc_rule=False)
    group, waves, want = SMALL_FORMS[fname]
    with switches(ctx, group, waves):
        res = ctx.debug_qp(P, q[None], h, opts=qp_opts(**qu.TIGHT))
    assert tuple(res["form"]) == want(n)
    k = earned(P, q, h, res, 0, None, opts=qu.TIGHT)
    allowed = 1.05 * qu.TIGHT["feastol"] + k["dres_typical"]
    print(f"tight {n} {seed} {fname}: iterations {res['iterations'][0]} without the rule {off['iterations']}; true dres {k['dres']:.2e} "
          f"allowed {allowed:.2e}, without the rule {off['true_dres']:.2e}")
    assert res["iterations"][0] in (off["iterations"], off["iterations"] + 1)
    assert k["dres"] <= allowed


# ---- g. the borders at the largest padding ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group,waves,n,want", [(3, -1, 1, (1, 0, 8)), (3, -1, 33, (1, 0, 8)), (0, -1, 545, (0, 1, 8))],
                         ids=["group-n1", "group-n33", "global_u-n545"])
def test_borders_at_the_largest_padding(ctx, group, waves, n, want):
    """n = 1 and n = 33 (padded to 64) in the group kernel, n = 545 (padded to 576) with the inverse blocks in global memory; the batch
    forms run these sizes in every test above"""
    P, q, h, refs = problems(n)
    with switches(ctx, group, waves):
        alone = ctx.qp_batch(P, q, h)
        res = ctx.debug_qp(P, q, h)
    assert tuple(res["form"]) == want
    same_bits(res, alone)
    for b in range(B):
        assert res["iterations"][b] == refs[b]["iterations"]
        x_close(res["x"][b], refs[b]["x"])
        earned(P[b], q[b], h[b], res, b, refs[b])
