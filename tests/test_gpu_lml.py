"""GPU: the log marginal likelihood of a fitted batch on the device (DRT.evaluate_lml / evaluate_lml_batch over
hipdrt_plan_lml_terms; csrc/lml.hip, csrc/qp_resident.hpp: logdet_kernel_resident).

1. the log-determinant kernel alone (hipdrt_debug_logdet) against an extended-precision Cholesky sum, at both LDS forms, the
   32-block edge on both sides and padding of 1 and 31; an indefinite matrix between two good ones; one matrix alone and in a batch;
2. the reference's recorded states (tools/make_lml_golden.py) uploaded to a device fit of the same data: all eight terms and lml,
   the NaN pattern, the update_hypers and weights variants;
3. the live fit end to end against the reference's final value;
4. a batch with a failed member: NaN and a negative status for it, the others bit for bit as when fitted alone;
5. a recorded step equals the upload of that step's state, bit for bit; a step beyond the store is refused;
6. the sums against hipdrt_plan_obs_llh_terms;
7. a call touches nothing of the fit.

Bounds: tests/lml_bounds.json (label -> [measured on an MI355X, bound]); a bound is 10 to 50 times the measured deviation from
the RECORDED reference values, rounded to 1 / 2 / 5 x 10^k and never below 1e-13 (a deviation of a few ulp is no measurement).
Terms: relative to max(1, |recorded|); lml: absolute, over the finite entries.  `kernel:n<n>` is measured against the
extended-precision sum and is all but the prescribed-eigenvalue matrix's: at condition 1e10 any double-precision Cholesky moves
the small eigenvalues by cond x eps of themselves (LAPACK's deviates by 1.5e-9 on the same matrices, the kernel by 4.1e-9 at
most), while the well-conditioned and the graded members agree to 1e-15.  `ref_state` uploads the reference's state and
weights, so only the device's own rm, rv and arithmetic differ; `ref_state_devw` reads the device fit's est_weights, and `e2e` its
whole state, so those carry the fit's own deviation from the reference (tests/parity_bounds.json) into the sums, and the
cancellation in beta = 0.5 (wy2 - fit2 - xox) + 1 carries it, amplified by alpha |W y|^2 / |beta| (up to 4e6 here), into lml."""
import numpy as np
import pytest

import lml_util as U

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from hipdrt import _ffi
    return _ffi.get_context(0)


# ---- 1. the kernel alone -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def kernel_cases():
    """n -> (matrices (3, n, n), their extended-precision log-determinants), formed once"""
    return {}


def case(kernel_cases, n):
    if n not in kernel_cases:
        mats = U.kernel_matrices(n)
        kernel_cases[n] = (mats, np.array([U.longdouble_logdet(a) for a in mats]))
    return kernel_cases[n]


@pytest.mark.parametrize("n", U.KERNEL_N)
def test_logdet_kernel_against_extended_precision(ctx, kernel_cases, n):
    mats, ref = case(kernel_cases, n)
    got, status = ctx.debug_logdet(mats)
    assert status.tolist() == [0, 0, 0]
    U.check(f"kernel:n{n}", got, ref)
    # one matrix alone gives the bits it gives in the batch
    for b in range(3):
        alone, st = ctx.debug_logdet(mats[b:b + 1])
        assert st[0] == 0 and np.array_equal(alone, got[b:b + 1]), (n, b)


def test_logdet_kernel_on_the_fixtures_prior_and_posterior(ctx):
    g = U.load("golden71x91")
    mats = np.stack(U.omega_and_p(g, len(g["lml"]) - 1) + U.omega_and_p(g, 0))
    got, status = ctx.debug_logdet(mats)
    assert not status.any()
    U.check("kernel:n93", got, np.array([U.longdouble_logdet(a) for a in mats]))


@pytest.mark.parametrize("n", (33, 529))
def test_an_indefinite_matrix_between_two_good_ones(ctx, kernel_cases, n):
    mats, _ = case(kernel_cases, n)
    good, _ = ctx.debug_logdet(mats[[0, 2]])
    bad = mats[1].copy()
    bad[n // 2, n // 2] = -1.0                            # a negative diagonal entry: not positive definite
    got, status = ctx.debug_logdet(np.stack([mats[0], bad, mats[2]]))
    assert status.tolist() == [0, -1, 0] and np.isnan(got[1])
    assert np.array_equal(got[[0, 2]], good)


# ---- the fits of the four fixtures, on the device ----------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def fits():
    cache = {}

    def get(name):
        if name not in cache:
            from hipdrt.models import DRT
            g = U.load(name)
            drt = DRT(warn=False, fit_dop=name == "hybrid_dop_s0")
            if name.startswith("hybrid"):
                drt.fit_hybrid(g["times"], g["i_signal"], g["v_signal"], g["freq"], g["z"])
            else:
                drt.fit_eis(g["freq"], g["z"], **(dict(nonneg=False) if name.endswith("_neg") else {}))
            cache[name] = (g, drt)
        return cache[name]
    return get


def state_of(g, i):
    st = dict(x=g["x"][i][None], rho_vector=g["rho_vector"][i][None], s_vectors=g["s_vectors"][i][None])
    if int(g["has_dop"]):
        st["dop_rho_vector"] = g["dop_rho_vector"][i][None]
    return st


def terms_array(terms):
    return np.array([terms[k][0] for k in U.TERMS])


# ---- 2. reference states ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.FIXTURES)
def test_reference_states_on_a_device_fit(fits, name):
    g, drt = fits(name)
    ne = len(g["lml"])
    for label, weights in (("ref_state", g["est_weights"]), ("ref_state_devw", None)):
        got_t, got_l = [], []
        for i in range(ne):
            val, terms = drt.evaluate_lml_batch(state=state_of(g, i), weights=weights, return_terms=True)
            assert terms["status"][0] >= 0
            got_t.append(terms_array(terms)); got_l.append(val[0])
        got_t = np.array(got_t)
        for k, term in enumerate(U.TERMS):
            U.check(f"{label}:{term}", got_t[:, k], g["terms"][:, k])
        U.check(f"{label}:lml", np.array(got_l), g["lml"], absolute=True)          # NaN exactly where the fixture has NaN
    last = state_of(g, ne - 1)
    for tag in U.VARIANTS:
        update, weights = U.variant_kw(g, tag)
        val, terms = drt.evaluate_lml_batch(state=last, weights=g["est_weights"] if weights is None else weights, update_hypers=update,
                                            return_terms=True)
        for k, term in enumerate(U.TERMS):
            U.check(f"ref_state:{term}", terms[term], g[f"terms_{tag}"][k:k + 1])
        U.check("ref_state:lml", val, np.array([float(g[f"lml_{tag}"])]), absolute=True)


# ---- 3. end to end ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", U.FIXTURES)
def test_live_fit_against_the_references_final_value(fits, name):
    g, drt = fits(name)
    batch, terms = drt.evaluate_lml_batch(return_terms=True)
    for k, term in enumerate(U.TERMS):
        U.check(f"e2e:{term}", terms[term], g["terms"][-1:, k])
    U.check("e2e:lml", batch, np.array([float(g["lml_final"])]), absolute=True)
    single = drt.evaluate_lml(b=0)
    assert np.array([single]).tobytes() == batch[:1].tobytes()                 # (the joint fits' final value is NaN: compare bits)
    # upstream's signature with a history entry in upstream's form: member 0 takes the entry's state
    i = 0
    entry = dict(x=g["x"][i], rho_vector=g["rho_vector"][i], s_vectors=list(g["s_vectors"][i]),
                 dop_rho_vector=g["dop_rho_vector"][i] if int(g["has_dop"]) else None)
    via_entry = drt.evaluate_lml(history_entry=entry)
    via_state = drt.evaluate_lml_batch(state=state_of(g, i))[0]
    assert np.array([via_entry]).tobytes() == np.array([via_state]).tobytes() and np.isfinite(via_entry)


# ---- 4. batch rules -------------------------------------------------------------------------------------------------------------------
def test_a_failed_member_is_nan_and_the_others_keep_their_bits():
    """all-NaN data break the QP at its start point (the failing member of tests/test_gpu_predict.py)"""
    from hipdrt import synth
    from hipdrt.models import DRT
    g = U.load("golden71x91")
    freq = g["freq"]
    z = np.stack([g["z"], synth.zarc2_batch(freq, 1, first_seed=300)[0], np.full(len(freq), np.nan + 0j)])
    drt = DRT(warn=False)
    res = drt.fit_eis_batch(freq, z)
    assert res["status"][2] < 0 and (res["status"][:2] >= 0).all()
    val, terms = drt.evaluate_lml_batch(return_terms=True)
    assert np.isnan(val[2]) and terms["status"][2] < 0 and (terms["status"][:2] >= 0).all()
    assert all(np.isnan(terms[k][2]) for k in U.TERMS)
    assert np.isfinite(val[0])
    for b in range(2):
        alone = DRT(warn=False)
        alone.fit_eis_batch(freq, z[b:b + 1])
        v1, t1 = alone.evaluate_lml_batch(return_terms=True)
        assert v1.tobytes() == val[b:b + 1].tobytes(), b
        for k in U.TERMS:
            assert t1[k].tobytes() == terms[k][b:b + 1].tobytes(), (b, k)
    assert np.array([drt.evaluate_lml(b=1)]).tobytes() == val[1:2].tobytes()
    assert np.isnan(drt.evaluate_lml(b=2))


# ---- 5. step source -------------------------------------------------------------------------------------------------------------------
def test_a_recorded_step_equals_the_upload_of_its_state():
    from hipdrt import _ffi, synth
    from hipdrt.models import DRT
    freq = np.logspace(6, -1, 71)
    z = synth.zarc2_batch(freq, 2, first_seed=11)
    drt = DRT(warn=False)
    drt.pfrt_fit_eis_batch(freq, z, factors=np.array([0.5, 1.0, 2.0]))
    plan = drt._plan
    assert plan.pfrt_steps() == 3
    vals = []
    for i in range(3):
        st = plan.pfrt_step_state(i)
        by_step, t_step = drt.evaluate_lml_batch(step=i, return_terms=True)
        by_state, t_state = drt.evaluate_lml_batch(state=dict(x=st["x"], rho_vector=st["rho"], s_vectors=st["s_vectors"]), return_terms=True)
        assert by_step.tobytes() == by_state.tobytes(), i
        for k in U.TERMS:
            assert t_step[k].tobytes() == t_state[k].tobytes(), (i, k)
        vals.append(t_step["xox"])
    assert not np.array_equal(vals[0], vals[2])                              # the steps do differ
    with pytest.raises(_ffi.HipDrtError, match="step out of range"):
        drt.evaluate_lml_batch(step=3)
    with pytest.raises(ValueError, match="exclude each other"):
        drt.evaluate_lml_batch(step=0, state=dict(x=st["x"], rho_vector=st["rho"], s_vectors=st["s_vectors"]))
    # refusals of the entry point itself
    with pytest.raises(_ffi.HipDrtError, match="dop_rho"):
        plan.lml_terms(x=st["x"], rho=st["rho"], s_vectors=st["s_vectors"], dop_rho=np.ones((2, 3)))
    with pytest.raises(_ffi.HipDrtError, match="together"):
        plan.lml_terms(x=st["x"])
    with pytest.raises(_ffi.HipDrtError, match="positive"):
        plan.lml_terms(weights=np.zeros((2, plan.m)))


# ---- 6. consistency with what exists ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("golden71x91", "hybrid_dop_s0"))
def test_sums_agree_with_obs_llh_terms(fits, name):
    """wy2 - 2 cross + fit2 is the residual sum of squares that hipdrt_plan_obs_llh_terms expands the same way from the same
    weights: each of the three sums of m products carries at most m eps of its own magnitude, and all three are bounded by wy2
    up to the fit's residual, so the two agree within 8 m eps wy2.  slw is the same loop over the same weights in the same
    order (thread t takes rows t, t + 512, ...; the same block reduction): bit for bit."""
    _, drt = fits(name)
    plan = drt._plan
    _, t = drt.evaluate_lml_batch(return_terms=True)
    rss, slw = plan.llh_terms(stored=True)
    assert np.all(np.abs((t["wy2"] - 2 * t["cross"] + t["fit2"]) - rss) <= 8 * plan.m * np.finfo(float).eps * t["wy2"])
    assert t["slw"].tobytes() == slw.tobytes()


# ---- 7. nothing of the fit is touched ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("golden71x91", "hybrid_dop_s0"))
def test_a_call_leaves_the_fit_as_it_was(fits, name):
    g, drt = fits(name)
    plan = drt._plan

    def snapshot():
        d = plan.download(s_vectors=True)
        var = drt.estimate_distribution_var_batch()[0] if name == "golden71x91" else plan.param_var(1)[0]
        return [np.asarray(d[k]).tobytes() for k in sorted(d)], plan.p_matrix(0).tobytes(), var.tobytes()
    before = snapshot()
    drt.evaluate_lml_batch()
    drt.evaluate_lml_batch(state=state_of(g, 0), weights=0.5 * g["est_weights"], update_hypers=dict(l2_lambda_0=7.0))
    assert snapshot() == before
