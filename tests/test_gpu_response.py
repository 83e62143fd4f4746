"""GPU: the voltage response of chrono / hybrid fits on the device (hipdrt_plan_predict_response, csrc/predict.hip:
response_assemble_kernel behind the row-application kernel) against its numpy statement hipdrt.models.response and against runs
of the reference.

1. the device chain alone through its hook (hipdrt_debug_response) on synthetic arrays, no fit: every include bit alone and all of
   them, one and two copies of the basis, a failed member, a member alone against the same member in the batch (same bits);
2. fits of the fixtures' measurements against the reference's recorded predictions (tools/make_response_golden.py);
3. a batch of five members with different step sizes against the statement fed every member's own parameters, and against the
   members' single fits (same bits);  4. a member with NaN data;  5. series_neg;  6. the refusals;
7. impedance of a prepared fit (hipdrt_plan_predict_z_model) and distribution of phasances (hipdrt_plan_predict_dop) against the
   reference's run, and against the statement fed the members' own parameters (bound (K + 8) u sum |terms|: one block of K products
   and the same handful of scalar operations);
8. solve_rp fits, single and batch: the post-fit scales and every member's own dop_scale_vector, against the statements fed each
   member's own parameters.

Bound of 1 and 3 (u = 2^-53; nothing is measured from the kernel).  An output element is a sum of K products per step and block
(K = ntau or dop_size, in the MFMA's order), S steps per block, and a handful of scalar operations (the coefficient scale, the
step size, the DOP block's scale vector, the difference of the two copies, the three additions, the vz-offset factor, the baseline's rescaling and dot product):
at most K + S + 8 roundings lie on the path of any term, so |device - exact| <= (K + S + 8) u sum |terms|.  The statement is
evaluated in extended precision (its own error is 2^-11 of that) and also returns the sum of absolute terms.

Bound of 2: the project's parity contract, 1e-7 of each signal's peak magnitude; tests/response_bounds.json records what a GPU run
measured (label -> [measured, bound = 20 x measured rounded up to 1 / 2 / 5 x 10^k, at least 1e-12 and at most 1e-7])."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, parity

pytestmark = pytest.mark.gpu

U = 2.0 ** -53
LD = np.longdouble
BITS = dict(drt=1, ohmic=2, cap=4, dop=8, vz_offset=16, baseline=32)


def include_kw(mask):
    return {f"include_{k}": bool(mask & v) for k, v in BITS.items()}


@pytest.fixture(scope="module")
def ctx():
    from hipdrt import _ffi
    return _ffi.get_context()


# ---- 1. the device chain alone --------------------------------------------------------------------------------------------------------
B0, S0, NT0, NTAU0, NVB0, ND0 = 33, 3, 70, 57, 2, 50          # one past the 32-spectrum tile; 210 stacked rows: no multiple of 64


def synthetic(copies):
    """special block: v_baseline (2), vz_offset, R_inf, C_inv, x_dop (50); then one or two copies of a 57-point basis"""
    rng = np.random.default_rng(11 + copies)
    ns = NVB0 + 3 + ND0
    n = ns + copies * NTAU0
    c = dict(copies=copies, ns=ns, n=n, vb_start=0, vz_index=2, idx_rinf=3, idx_cinv=4, dop_start=5)
    c["X"] = rng.standard_normal((B0, n)) * np.exp(rng.standard_normal((B0, n)))
    c["X"][:, 2] *= 0.05
    t = np.sort(rng.uniform(0.0, 3.0, NT0))
    steps = np.array([0.2, 1.1, 2.0])
    after = (t[None, :] > steps[:, None]).astype(float)              # (S, nt): a layer is zero before its step
    c["U"] = rng.uniform(0.0, 1.0, (S0, NT0, NTAU0)) * after[:, :, None]
    c["Ud"] = rng.standard_normal((S0, NT0, ND0)) * after[:, :, None]
    c["dsv"] = np.exp(rng.standard_normal((B0, ND0)))               # every member its own dop_scale_vector, as under solve_rp
    c["sizes"] = rng.standard_normal((B0, S0)) * 1e-3
    c["cs"], c["rss"] = rng.uniform(0.5, 20.0, B0), rng.uniform(1e-3, 1e-1, B0)
    c["sro"] = rng.standard_normal(B0)
    c["cap_scale"] = 0.37
    c["inf_rv"] = np.cumsum(c["sizes"][:, :, None] * after[None], axis=1)[:, -1]            # (B, nt)
    c["cap_rv"] = np.sum(1e-3 * np.maximum(t[None, :] - steps[:, None], 0.0), axis=0)       # (nt,), shared
    c["strength"] = rng.uniform(0.0, 1.0, NT0)
    c["vb_mat"] = np.stack([np.ones(NT0), t - t[0]], axis=1)
    c["vb_scale"] = np.array([1.0, t[-1] - t[0]])
    return c


def device(ctx, c, mask, rows=slice(None), fit_status=None):
    return ctx.debug_response(c["X"][rows], c["ns"], c["sizes"][rows], c["cs"][rows], U=c["U"], Ud=c["Ud"], dop_start=c["dop_start"],
                              dop_scale_vector=c["dsv"][rows], copies=c["copies"], idx_rinf=c["idx_rinf"], idx_cinv=c["idx_cinv"], vz_index=c["vz_index"],
                              vb_start=c["vb_start"], capacitance_scale=c["cap_scale"], response_signal_scale=c["rss"][rows],
                              scaled_response_offset=c["sro"][rows], inf_rv=c["inf_rv"][rows], cap_rv=c["cap_rv"],
                              vz_strength=c["strength"], vb_mat=c["vb_mat"], v_baseline_scale=c["vb_scale"], fit_status=fit_status,
                              include_mask=mask)


def statement(c, b, mask):
    """(value, sum of absolute terms) of member b in extended precision"""
    from hipdrt.models import response
    ld = lambda a: np.asarray(a, dtype=LD)
    fp = response.fit_parameters(ld(c["X"][b]), c["ns"], LD(c["cs"][b]), idx_rinf=c["idx_rinf"], idx_cinv=c["idx_cinv"],
                                 capacitance_scale=LD(c["cap_scale"]), vz_index=c["vz_index"], vb_start=c["vb_start"],
                                 v_baseline_scale=ld(c["vb_scale"]), scaled_response_offset=LD(c["sro"][b]),
                                 response_signal_scale=LD(c["rss"][b]), dop_start=c["dop_start"], dop_scale_vector=ld(c["dsv"][b]),
                                 with_abs=True)
    return response.predict_response_rows(ld(c["U"]), ld(c["sizes"][b]), fp, u_dop=ld(c["Ud"]), inf_rv=ld(c["inf_rv"][b]),
                                          cap_rv=ld(c["cap_rv"]), vz_strength=ld(c["strength"]), vb_mat=ld(c["vb_mat"]),
                                          return_abs=True, **include_kw(mask))


def assert_bound(label, got, want, mag, k, s):
    bound = (k + s + 8) * U * np.asarray(mag, dtype=float)
    err = np.abs(np.asarray(got, dtype=LD) - want).astype(float)
    worst = float(np.max(err / np.maximum(bound, 1e-300))) if np.any(bound > 0) else 0.0
    print(f"{label}: worst error / bound {worst:.3f}")
    assert np.all(err <= bound), f"{label}: {worst:.2f} x the derived bound"


@pytest.mark.parametrize("copies", [1, 2])
@pytest.mark.parametrize("mask", [1, 2, 4, 8, 16, 32, 63])
def test_chain_alone_against_the_statement(ctx, copies, mask):
    c = synthetic(copies)
    out = device(ctx, c, mask)                     # (raises if the kernel wrote outside out[B][nt])
    assert out.shape == (B0, NT0) and np.isfinite(out).all()
    for b in range(B0):
        want, mag = statement(c, b, mask)
        assert_bound(f"copies {copies} mask {mask} member {b}", out[b], want, mag, max(NTAU0, ND0), S0)
    if mask in (1, 63):
        assert np.abs(out).max() > 0 and not np.array_equal(out, device(ctx, c, mask & ~1))


def test_chain_alone_member_alone_failed_member_and_absent_terms(ctx):
    c = synthetic(2)
    full = device(ctx, c, 63)
    for b in (0, 17, 32):                          # first of a tile, inside one, the member past the 32-spectrum tile
        assert np.array_equal(device(ctx, c, 63, rows=slice(b, b + 1))[0], full[b])
    status = np.zeros(B0, dtype=np.int32)
    status[[5, 32]] = -1
    bad = device(ctx, c, 63, fit_status=status)
    assert np.isnan(bad[[5, 32]]).all() and np.array_equal(np.delete(bad, [5, 32], axis=0), np.delete(full, [5, 32], axis=0))
    # the members' own scale vectors are used: without them (ones) the DOP term alone differs, row by row
    kw = dict(Ud=c["Ud"], dop_start=c["dop_start"], include_mask=8)
    scaled = ctx.debug_response(c["X"], c["ns"], c["sizes"], c["cs"], dop_scale_vector=c["dsv"], **kw)
    plain = ctx.debug_response(c["X"], c["ns"], c["sizes"], c["cs"], **kw)
    shared = ctx.debug_response(c["X"], c["ns"], c["sizes"], c["cs"], dop_scale_vector=np.tile(c["dsv"][0], (B0, 1)), **kw)
    assert np.array_equal(scaled, device(ctx, c, 8)) and np.array_equal(shared[0], scaled[0])
    assert all(not np.array_equal(scaled[b], plain[b]) and not np.array_equal(scaled[b], shared[b]) for b in range(1, B0))
    # a term without its layers or vector is left out, whatever the mask says
    bare = ctx.debug_response(c["X"], c["ns"], c["sizes"], c["cs"], U=c["U"], copies=2, include_mask=63)
    assert np.array_equal(bare, ctx.debug_response(c["X"], c["ns"], c["sizes"], c["cs"], U=c["U"], copies=2, include_mask=1))
    # shared step sizes: the same row for every member
    shared = ctx.debug_response(c["X"], c["ns"], c["sizes"][7], c["cs"], U=c["U"], copies=2, include_mask=1)
    assert np.array_equal(shared[7], bare[7]) and not np.array_equal(shared[8], bare[8])


def test_hook_refuses_what_would_leave_the_arrays(ctx):
    from hipdrt import _ffi
    c = synthetic(1)
    for kw in (dict(idx_rinf=c["n"]), dict(vz_index=c["n"] + 3), dict(dop_start=c["n"] - 10), dict(copies=2), dict(include_mask=128)):
        args = dict(U=c["U"], Ud=c["Ud"], dop_start=c["dop_start"], copies=1, include_mask=63)
        args.update(kw)
        with pytest.raises(_ffi.HipDrtError, match="invalid argument"):
            ctx.debug_response(c["X"], c["ns"], c["sizes"], c["cs"], **args)


# ---- 2. fits of the fixtures' measurements against the reference's run -----------------------------------------------------------------
def measurement(name):
    from hipdrt import synth
    if name == "hybrid_3step":
        return synth.hybrid_measurement(seed=2, n_post=80, extra_steps=((2.0, -2e-3), (3.0, 1e-3))), dict(vz_offset_scale=0.5, vz_offset_eps=2)
    meas = synth.hybrid_measurement(seed=0)
    return (meas[:3] + (None, None) if name == "chrono_s1" else meas), (dict(solve_rp=True) if name.endswith("_solverp") else {})


def ref_parity(label, got, ref, scale=None):
    """conftest.parity against the reference's recorded values: the bound of tests/response_bounds.json, never above the parity
    contract of 1e-7, and 1e-7 for a label not measured yet"""
    with open(os.path.join(ROOT, "tests", "response_bounds.json")) as f:
        entry = json.load(f).get(label)
    return parity(label, got, ref, bound=1e-7 if entry is None else min(1e-7, float(entry[1])), label=label, scale=scale)


@pytest.mark.parametrize("name", ["hybrid_s0", "hybrid_s0_dop", "hybrid_s0_dop_solverp", "hybrid_3step", "chrono_s1"])
def test_fit_against_the_reference_run(name):
    from hipdrt.models import DRT
    g = np.load(os.path.join(GOLDEN, f"refrun_response_predict_{name}.npz"))
    meas, fit_kw = measurement(name)
    drt = DRT(fit_dop="_dop" in name, warn=False)
    if meas[3] is None:
        drt.fit_chrono(*meas[:3], **fit_kw)
    else:
        drt.fit_hybrid(*meas, **fit_kw)
    peak = float(np.abs(g["response_fit"]).max())
    ref_parity(f"{name}.response_fit", drt.predict_response(), g["response_fit"])
    ref_parity(f"{name}.response_off", drt.predict_response(times=g["t_off"]), g["response_off"])
    # the transient without its baseline, which would otherwise hide it: 1e-7 of ITS peak
    ref_parity(f"{name}.response_off_less_baseline", drt.predict_response(times=g["t_off"]) - drt.predict_v_baseline(g["t_off"]),
               g["response_off"] - g["v_baseline_off"])
    for term in ("drt", "ohmic", "dop", "vz_offset"):
        ref_parity(f"{name}.response_off_no_{term}", drt.predict_response(times=g["t_off"], **{f"include_{term}": False}),
                   g[f"response_off_no_{term}"], scale=peak)
    ref_parity(f"{name}.v_baseline_fit", drt.predict_v_baseline(g["t_fit"]), g["v_baseline_fit"])
    ref_parity(f"{name}.v_baseline_off", drt.predict_v_baseline(g["t_off"]), g["v_baseline_off"])
    # the fitted steps given explicitly, and as a signal, are the same request
    base = drt.predict_response(times=g["t_fit"])
    assert np.array_equal(drt.predict_response(times=g["t_fit"], step_times=drt.step_times, step_sizes=drt.step_sizes), base)
    assert np.array_equal(drt.predict_response(), base) and np.array_equal(drt.predict_response_batch()[0], base)
    assert np.array_equal(drt.predict_response(times=g["t_fit"], input_signal=meas[1]), base)         # steps found in the signal
    # a given v_baseline replaces the fitted one (here: none)
    assert np.allclose(drt.predict_response(v_baseline=np.zeros(len(base))), base - drt.predict_v_baseline(g["t_fit"]), rtol=0,
                       atol=4 * U * peak)
    # the measured ohmic response (smooth_inf_response=False) of an ideal signal is the ideal steps: the fitted signal's, and the
    # model signal's of given steps
    for kw in (dict(), dict(times=g["t_fit"], step_times=drt.step_times, step_sizes=drt.step_sizes)):
        assert np.allclose(drt.predict_response(smooth_inf_response=False, **kw), base, rtol=0, atol=8 * U * peak)
    with pytest.raises(ValueError, match="smooth_inf_response=False"):
        drt.predict_response(times=g["t_off"], smooth_inf_response=False)
    # the prediction describes the data it was fitted to (a sanity check of the whole path, not a parity bound)
    assert np.max(np.abs(base - g["v_signal"])) < 2e-3 * peak


# ---- 3. a batch with different step sizes ------------------------------------------------------------------------------------------------
I_STEPS = (1e-3, 0.5e-3, 2e-3, -1e-3, 1.5e-3)


@pytest.fixture(scope="module")
def batch5():
    from hipdrt import synth
    from hipdrt.models import DRT
    meas = [synth.hybrid_measurement(seed=b, jitter=True, i_step=I_STEPS[b]) for b in range(5)]
    drt = DRT(warn=False)
    res = drt.fit_hybrid_batch(meas[0][0], [m[1] for m in meas], [m[2] for m in meas], meas[0][3], [m[4] for m in meas])
    assert (res["status"] >= 0).all()
    return drt, meas, drt.predict_response_batch()


def member_statement(drt, ctx, b, times):
    """the statement fed member b's own parameters and the unit-step layers of the stand-alone builder -> (value, magnitude)"""
    from hipdrt import _ffi
    from hipdrt.matrices import mat1d
    from hipdrt.models import background, response
    preps, fps = drt._last_prepared
    pr, fp = preps[b], fps[b]
    ld = lambda a: np.asarray(a, dtype=LD)
    lut = drt._lookups(ctx)["response"]
    _, u = ctx.response_matrix(times, drt.basis_tau, pr["step_times"], np.ones(len(pr["step_times"])), drt.tau_epsilon,
                               mode=_ffi.MODE_INTERP, lookup=lut, layered=True)
    inf_rv = mat1d.construct_ohmic_response_vector(times, "ideal", pr["step_times"], pr["step_sizes"], None, None, True)
    strength = drt._vz_strength(pr["sample_times"], pr["frequencies"], pr["nonconsec_step_times"], 1, times=times)[0]
    vb_mat = background.get_baseline_matrix(times, 0, normalize=False)
    fpl = {k: ld(v) for k, v in fp.items() if k in ("x", "R_inf", "C_inv", "v_baseline", "vz_offset", "x_dop")}
    u_dop = None
    if pr["dop"]:
        _, u_dop = ctx.phasor_v_matrix(times, drt.basis_nu, drt.nu_epsilon, pr["step_times"], np.ones(len(pr["step_times"])))
    return response.predict_response_rows(ld(u), ld(pr["step_sizes"]), fpl, u_dop=None if u_dop is None else ld(u_dop),
                                          inf_rv=ld(inf_rv), vz_strength=ld(strength), vb_mat=ld(vb_mat), return_abs=True)


def test_batch_members_follow_the_statement_with_their_own_step_sizes(ctx, batch5):
    drt, meas, out = batch5
    times = meas[0][0]
    assert out.shape == (5, len(times))
    sizes = np.array([pr["step_sizes"] for pr in drt._last_prepared[0]])
    assert np.allclose(sizes[:, 0], I_STEPS, rtol=1e-9)                     # (the members' measured step sizes do differ)
    for b in range(5):
        want, mag = member_statement(drt, ctx, b, times)
        assert_bound(f"batch member {b}", out[b], want, mag, len(drt.basis_tau), 1)
        assert np.max(np.abs(out[b] - meas[b][2])) < 2e-3 * np.abs(meas[b][2]).max()
    t_off = np.concatenate([[times[0] - 0.01], 0.05 + np.logspace(-4.5, 2, 45)])
    off = drt.predict_response_batch(times=t_off)
    for b in (1, 3):
        want, mag = member_statement(drt, ctx, b, t_off)
        assert_bound(f"batch member {b} off grid", off[b], want, mag, len(drt.basis_tau), 1)


def test_member_alone_gives_the_same_bits_as_inside_the_batch(batch5):
    from hipdrt.models import DRT
    drt, meas, out = batch5
    for b in (0, 3):
        single = DRT(warn=False)
        fp = single.fit_hybrid(*meas[b])
        assert np.array_equal(fp["x"], drt._last_prepared[1][b]["x"])         # (the fits themselves are the same bits)
        assert np.array_equal(single.predict_response(), out[b])
        assert np.array_equal(single.predict_response(), drt.predict_response(b=b))


# ---- 4. a failed member ---------------------------------------------------------------------------------------------------------------------
def test_failed_member_gives_a_nan_row_and_a_negative_status(batch5):
    from hipdrt.models import DRT
    _, meas, out = batch5
    v = [m[2].copy() for m in meas]
    v[2][:] = np.nan
    bad = DRT(warn=False)
    with np.errstate(all="ignore"):
        res = bad.fit_hybrid_batch(meas[0][0], [m[1] for m in meas], v, meas[0][3], [m[4] for m in meas])
        got = bad.predict_response_batch()
    assert res["status"][2] < 0 and (np.delete(res["status"], 2) >= 0).all()
    assert np.isnan(got[2]).all()
    keep = [0, 1, 3, 4]
    assert np.array_equal(got[keep], out[keep])
    plan = bad._plan
    _, status = plan.predict_response(meas[0][0], bad._last_prepared[0][0]["step_times"], [1e-3], include_mask=2)
    assert status[2] < 0 and (status[keep] >= 0).all()


# ---- 5. series_neg ----------------------------------------------------------------------------------------------------------------------------
def test_series_neg_fit_follows_the_statement(ctx):
    from hipdrt import synth
    from hipdrt.models import DRT
    meas = synth.hybrid_measurement(seed=4)
    drt = DRT(warn=False)
    fp = drt.fit_hybrid(*meas, series_neg=True)
    assert len(fp["x"]) == 2 * len(drt.basis_tau) and np.abs(fp["x"][len(drt.basis_tau):]).max() > 0
    drt._last_prepared = ([drt._prep], [fp])
    try:
        want, mag = member_statement(drt, ctx, 0, meas[0])
    finally:
        drt._last_prepared = None
    out = drt.predict_response()
    assert_bound("series_neg", out, want, mag, len(drt.basis_tau), 1)
    assert np.max(np.abs(out - meas[2])) < 2e-3 * np.abs(meas[2]).max()


# ---- 6. refusals --------------------------------------------------------------------------------------------------------------------------------
def test_refusals(batch5):
    from hipdrt import _ffi, synth
    from hipdrt.models import DRT
    drt, meas, out = batch5
    times = meas[0][0]
    with pytest.raises(NotImplementedError, match="x="):
        drt.predict_response(x=np.ones(3))
    with pytest.raises(NotImplementedError, match="subtract_background"):
        drt.predict_response(subtract_background=False)
    with pytest.raises(NotImplementedError, match="op_mode"):
        drt.predict_response(op_mode="pot")
    with pytest.raises(NotImplementedError, match="x_vb"):
        drt.predict_v_baseline(times, x_vb=np.ones(1))
    nonideal = DRT(warn=False)
    nonideal.__dict__.update(drt.__dict__)
    nonideal.step_model = "expdecay"
    with pytest.raises(NotImplementedError, match="step_model"):
        nonideal.predict_response()
    with pytest.raises(ValueError, match="input_signal OR"):
        drt.predict_response(input_signal=meas[0][1], step_times=[0.05], step_sizes=[1e-3])
    with pytest.raises(ValueError, match="both step_times and step_sizes"):
        drt.predict_response(step_times=[0.05])
    # y_bkg is added as upstream adds it
    assert np.array_equal(drt.predict_response(subtract_background=False, y_bkg=np.ones(len(times))), out[0] + 1.0)
    # an EIS fit has no response
    eis = DRT(warn=False)
    eis.fit_eis(meas[0][3], meas[0][4])
    with pytest.raises(RuntimeError, match="chrono or hybrid"):
        eis.predict_response(times=times)
    # the entry point before the prediction description says what is missing; so does a new upload
    fresh = DRT(warn=False)
    fresh.fit_hybrid(*synth.hybrid_measurement(seed=0))
    st = fresh._prep["step_times"]
    with pytest.raises(_ffi.HipDrtError, match="error -1.*prediction description is missing.*hipdrt_plan_set_predict_desc"):
        fresh._plan.predict_response(times, st, [1e-3], include_mask=2)
    fresh._set_predict_desc(fresh._plan)
    with pytest.raises(_ffi.HipDrtError, match="error -1.*tau basis is missing"):
        fresh._plan.predict_response(times, st, [1e-3], include_mask=2)
    assert fresh.predict_response().shape == times.shape
    with pytest.raises(_ffi.HipDrtError, match="invalid argument"):
        fresh._plan.predict_response(times, st, [1e-3], include_mask=128)
    with pytest.raises(_ffi.HipDrtError, match="basis_tau"):
        fresh._plan.predict_response(times, st, [1e-3], include_mask=1)
    # impedance prediction of a prepared plan is refused as before
    with pytest.raises(NotImplementedError, match="plain EIS"):
        fresh.predict_z_batch()


# ---- 7. impedance of a prepared fit, distribution of phasances ------------------------------------------------------------------------
def fitted(name):
    from hipdrt.models import DRT
    g = np.load(os.path.join(GOLDEN, f"refrun_response_predict_{name}.npz"))
    if name.startswith("golden71"):
        e = np.load(os.path.join(GOLDEN, "ref_test_drt_fit_eis.npz"))
        drt = DRT(fit_dop=name.endswith("_dop"), fit_capacitance=name.endswith("_cap"), warn=False)
        drt.fit_eis(np.asarray(e["freq"], dtype=float), np.asarray(e["z"], dtype=complex))
        return drt, g
    meas, fit_kw = measurement(name)
    drt = DRT(fit_dop="_dop" in name, warn=False)
    drt.fit_hybrid(*meas, **fit_kw)
    return drt, g


@pytest.mark.parametrize("name", ["hybrid_s0", "hybrid_s0_dop", "hybrid_s0_dop_solverp", "hybrid_3step", "golden71_dop", "golden71_cap"])
def test_z_model_against_the_reference_run(name):
    drt, g = fitted(name)
    peak = float(np.abs(g["z_wide"]).max())
    ref_parity(f"{name}.z_fit", drt.predict_z_model_batch()[0], g["z_fit"])
    ref_parity(f"{name}.z_fit_no_vz", drt.predict_z_model_batch(g["freq"], include_vz_offset=False)[0], g["z_fit_no_vz"])
    ref_parity(f"{name}.z_wide", drt.predict_z_model_batch(g["f_wide"])[0], g["z_wide"])
    ref_parity(f"{name}.z_wide_no_vz", drt.predict_z_model_batch(g["f_wide"], include_vz_offset=False)[0], g["z_wide_no_vz"])
    for term in ("drt", "ohmic", "inductance", "cap", "dop"):
        ref_parity(f"{name}.z_wide_no_{term}", drt.predict_z_model_batch(g["f_wide"], **{f"include_{term}": False})[0],
                   g[f"z_wide_no_{term}"], scale=peak)
    # the existing any-grid prediction keeps refusing such a fit
    with pytest.raises(NotImplementedError):
        drt.predict_z_batch()


@pytest.mark.parametrize("name", ["hybrid_s0_dop", "hybrid_s0_dop_solverp", "golden71_dop"])
def test_dop_against_the_reference_run(name):
    drt, g = fitted(name)
    nu, dop = drt.predict_dop(return_nu=True)
    assert np.array_equal(nu, g["dop_nu"])
    peak = float(np.abs(g["dop_no_ideal"]).max())
    ref_parity(f"{name}.dop", dop, g["dop"])
    ref_parity(f"{name}.dop_no_ideal", drt.predict_dop(include_ideal=False), g["dop_no_ideal"])
    ref_parity(f"{name}.dop_less_ideal", dop[np.abs(nu) % 1 != 0], g["dop"][np.abs(nu) % 1 != 0], scale=peak)
    ref_parity(f"{name}.dop_norm", drt.predict_dop(normalize=True), g["dop_norm"])
    nu7, d7 = drt.predict_dop(nu=[0.9, -1.0, 0.0, -0.45, 0.5, 1.0, -0.8], normalize=True, return_nu=True)
    assert np.array_equal(nu7, g["nu7"])
    ref_parity(f"{name}.dop_nu7_norm", d7, g["dop_nu7_norm"])
    assert np.array_equal(drt.predict_dop_batch()[0], dop)
    with pytest.raises(NotImplementedError, match="delta_density"):
        drt.predict_dop(delta_density=True)
    with pytest.raises(NotImplementedError, match="order"):
        drt.predict_dop(order=1)
    with pytest.raises(NotImplementedError, match="x="):
        drt.predict_dop(x=np.ones(3))


def z_statement(drt, ctx, fp, pr, f, **flags):
    from hipdrt import _ffi
    from hipdrt.models import response
    ld = lambda a: np.asarray(a, dtype=LD)
    a_re, a_im = ctx.impedance_matrix(f, drt.basis_tau, drt.tau_epsilon, mode=_ffi.MODE_INTERP, toeplitz=False,
                                      lookups=drt._lookups(ctx)["z"])
    zd = None
    if pr["dop"]:
        zd = ctx.phasor_z_matrix(f, drt.basis_nu, drt.nu_epsilon).astype(np.clongdouble)
    strength = None
    if "vz_offset" in fp:
        strength = drt._vz_strength(pr["sample_times"], pr["frequencies"], pr["nonconsec_step_times"], 1, predict_frequencies=f)[1]
    fpl = {k: (ld(v) if v is not None else None) for k, v in fp.items() if k in ("x", "R_inf", "inductance", "C_inv", "vz_offset", "x_dop")}
    return response.predict_z_model_rows(ld(a_re), ld(a_im), ld(f), fpl, zm_dop=zd, eis_strength=None if strength is None else ld(strength),
                                         return_abs=True, **flags)


def assert_z_bound(label, got, want, mag, k):
    bound = (k + 8) * U * np.asarray(mag, dtype=float)
    err = np.maximum(np.abs(got.real - want.real.astype(LD)), np.abs(got.imag - want.imag.astype(LD))).astype(float)
    worst = float(np.max(err / np.maximum(bound, 1e-300)))
    print(f"{label}: worst error / bound {worst:.3f}")
    assert np.all(err <= bound), f"{label}: {worst:.2f} x the derived bound"


F33 = np.logspace(6.5, -2.5, 33)


def test_z_model_of_a_batch_follows_the_statement_and_single_fits(ctx, batch5):
    from hipdrt.models import DRT
    drt, meas, _ = batch5
    preps, fps = drt._last_prepared
    z = drt.predict_z_model_batch(F33)
    assert z.shape == (5, 33) and np.iscomplexobj(z)
    for b in range(5):
        want, mag = z_statement(drt, ctx, fps[b], preps[b], F33)
        assert_z_bound(f"z member {b}", z[b], want, mag, len(drt.basis_tau))
    for mask_kw in (dict(include_drt=False), dict(include_vz_offset=False), dict(include_ohmic=False, include_inductance=False)):
        want, mag = z_statement(drt, ctx, fps[2], preps[2], F33, **mask_kw)
        assert_z_bound(f"z member 2 {mask_kw}", drt.predict_z_model_batch(F33, **mask_kw)[2], want, mag, len(drt.basis_tau))
    single = DRT(warn=False)
    single.fit_hybrid(*meas[3])
    assert np.array_equal(single.predict_z_model_batch(F33)[0], z[3])
    assert np.array_equal(drt.predict_z_model_batch()[1], drt.predict_z_model_batch(meas[0][3])[1])


def test_z_model_and_dop_of_special_fits(ctx):
    """series_neg (both copies with their signs), a DOP batch with a failed member, and the refusals of the two entry points"""
    from hipdrt import _ffi, synth
    from hipdrt.models import DRT
    meas = synth.hybrid_measurement(seed=4)
    sneg = DRT(warn=False)
    fp = sneg.fit_hybrid(*meas, series_neg=True)
    want, mag = z_statement(sneg, ctx, fp, sneg._prep, F33)
    assert_z_bound("series_neg z", sneg.predict_z_model_batch(F33)[0], want, mag, len(sneg.basis_tau))
    with pytest.raises(RuntimeError, match="fit_dop"):
        sneg.predict_dop()
    # a DOP batch, one member without data
    ms = [synth.hybrid_measurement(seed=b, jitter=True) for b in range(3)]
    z_in = [m[4] for m in ms]
    good, bad = DRT(fit_dop=True, warn=False), DRT(fit_dop=True, warn=False)
    good.fit_hybrid_batch(ms[0][0], [m[1] for m in ms], [m[2] for m in ms], ms[0][3], z_in)
    z_bad = [z_in[0], np.full_like(z_in[1], np.nan), z_in[2]]
    with np.errstate(all="ignore"):
        res = bad.fit_hybrid_batch(ms[0][0], [m[1] for m in ms], [m[2] for m in ms], ms[0][3], z_bad)
        dop, zz = bad.predict_dop_batch(), bad.predict_z_model_batch(F33)
    assert res["status"][1] < 0 and np.isnan(dop[1]).all() and np.isnan(zz[1]).all()
    assert np.array_equal(dop[[0, 2]], good.predict_dop_batch()[[0, 2]]) and np.array_equal(zz[[0, 2]], good.predict_z_model_batch(F33)[[0, 2]])
    preps, fps = good._last_prepared
    for b in (0, 2):
        want, mag = z_statement(good, ctx, fps[b], preps[b], F33)
        assert_z_bound(f"dop batch z member {b}", zz[b], want, mag, len(good.basis_tau))
    # the entry points say what is missing
    fresh = DRT(fit_dop=True, warn=False)
    fresh.fit_hybrid(*ms[0])
    with pytest.raises(_ffi.HipDrtError, match="error -1.*prediction description is missing"):
        fresh._plan.predict_z_model(F33, include_mask=2)
    with pytest.raises(_ffi.HipDrtError, match="error -1.*prediction description is missing"):
        fresh._plan.predict_dop([-1.0, 0.0, 1.0], fresh.basis_nu, fresh.nu_epsilon)
    fresh._set_predict_desc(fresh._plan)
    with pytest.raises(_ffi.HipDrtError, match="ascending"):
        fresh._plan.predict_dop([0.0, -1.0], fresh.basis_nu, fresh.nu_epsilon)
    with pytest.raises(_ffi.HipDrtError, match="error -1.*tau basis is missing"):
        fresh._plan.predict_z_model([1.0, 2.0], include_mask=2)
    assert fresh.predict_z_model_batch(F33).shape == (1, 33)
    with pytest.raises(_ffi.HipDrtError, match="positive"):
        fresh._plan.predict_z_model([1.0, 0.0], include_mask=2)
    # a plain EIS fit has predict_z_batch; its plan is refused by the new entry points
    eis = DRT(warn=False)
    eis.fit_eis(ms[0][3], ms[0][4])
    with pytest.raises(NotImplementedError, match="predict_z_batch"):
        eis.predict_z_model_batch()
    assert eis.predict_z_batch(F33).shape == (1, 33)


# ---- 8. solve_rp: the post-fit scales, and every member's own dop_scale_vector --------------------------------------------------------
def dop_statement(drt, ctx, fp, nu):
    from hipdrt.models import response
    ld = lambda a: np.asarray(a, dtype=LD)
    bm = ctx.func_eval_matrix(drt.basis_nu, nu, drt.nu_epsilon, order=0)
    fpl = {k: ld(v) for k, v in fp.items() if k in ("R_inf", "inductance", "C_inv", "x_dop")}
    return response.predict_dop_rows(ld(bm), nu, fpl, return_abs=True)


def check_member_against_the_statements(label, drt, ctx, b, times, v_out, z_out, nu, dop_out):
    preps, fps = drt._last_prepared if drt._last_prepared else ([drt._prep], [drt.fit_parameters])
    k = max(len(drt.basis_tau), len(drt.basis_nu))
    saved, drt._last_prepared = drt._last_prepared, (preps, fps)
    try:
        want, mag = member_statement(drt, ctx, b, times)
    finally:
        drt._last_prepared = saved
    assert_bound(f"{label} response member {b}", v_out, want, mag, k, 1)
    want, mag = z_statement(drt, ctx, fps[b], preps[b], F33)
    assert_z_bound(f"{label} z member {b}", z_out, want, mag, k)
    want, mag = dop_statement(drt, ctx, fps[b], nu)
    assert_bound(f"{label} dop member {b}", dop_out, want, mag, k, 0)


def test_solve_rp_fits_use_the_post_fit_scales_of_every_member(ctx):
    """solve_rp rescales the data and the DOP columns of every measurement by that measurement's own factors
    (drt1d.py:568-606): coefficient_scale, response_signal_scale, scaled_response_offset and dop_scale_vector all differ from member
    to member and from their pre-fit values.  A single fit and a batch of three, each member against the statements fed ITS OWN
    extracted parameters; a member of the batch against its single fit, bit for bit."""
    from hipdrt import synth
    from hipdrt.models import DRT
    ms = [synth.hybrid_measurement(seed=b, jitter=True, i_step=I_STEPS[b]) for b in range(3)]
    times = ms[0][0]
    single = DRT(fit_dop=True, warn=False)
    single.fit_hybrid(*ms[1], solve_rp=True)
    plainfit = DRT(fit_dop=True, warn=False)
    plainfit.fit_hybrid(*ms[1])
    assert single._prep["coefficient_scale"] != plainfit._prep["coefficient_scale"]           # (the scales did move)
    assert not np.array_equal(single._prep["dop_scale_vector"], plainfit._prep["dop_scale_vector"])
    nu, dop1 = single.predict_dop(return_nu=True)
    v1, z1 = single.predict_response(), single.predict_z_model_batch(F33)[0]
    check_member_against_the_statements("solve_rp single", single, ctx, 0, times, v1, z1, nu, dop1)
    assert np.max(np.abs(v1 - ms[1][2])) < 2e-3 * np.abs(ms[1][2]).max()

    batch = DRT(fit_dop=True, warn=False)
    res = batch.fit_hybrid_batch(times, [m[1] for m in ms], [m[2] for m in ms], ms[0][3], [m[4] for m in ms], solve_rp=True)
    assert (res["status"] >= 0).all()
    dsv = np.array([pr["dop_scale_vector"] for pr in batch._last_prepared[0]])
    assert not np.array_equal(dsv[0], dsv[1]) and not np.array_equal(dsv[0], dsv[2])           # (one vector per member)
    v, z, dop = batch.predict_response_batch(), batch.predict_z_model_batch(F33), batch.predict_dop_batch()
    for b in range(3):
        check_member_against_the_statements("solve_rp batch", batch, ctx, b, times, v[b], z[b], nu, dop[b])
    # with member 0's vector for everybody, members 1 and 2 would miss the bound by orders of magnitude: the DOP rows scale with it
    assert np.abs(dsv[1] / dsv[0] - 1).min() > 1e-6
    assert np.array_equal(res["x_dop"][1], single.fit_parameters["x_dop"])
    assert np.array_equal(v[1], v1) and np.array_equal(z[1], z1) and np.array_equal(dop[1], dop1)
