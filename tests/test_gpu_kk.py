"""GPU: the Kramers-Kronig screen (csrc/kk.hip; hipdrt_plan_kk_screen, hipdrt_debug_kk_stats) and the methods on top of it.

1. the statistics stage alone on the residual vectors of tests/golden/refrun_kk_stats.npz, several per launch, against
   hipdrt.models.kk (which tests/test_host_kk.py holds to the reference's recorded outputs);
2. both stages on a fitted plan against models.kk applied to rm, rv and x downloaded from that plan (isolates the kernel from
   fit parity), and the row factors it leaves for the next fit;
3. kk_test_batch and the single-spectrum kk_test against the reference's recorded run (refrun_kk_test_41.npz), both passes;
4. a fit_eis_batch after kk_test_batch returns the bits of a fresh instance.

The fixtures keep every point at least 0.2 in ln(prob) away from the outlier threshold in every pass (tools/make_kk_golden.py),
so masks, limits and trimmed data are compared exactly."""
import os

import numpy as np
import pytest

from conftest import GOLDEN, parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def stats():
    return np.load(os.path.join(GOLDEN, "refrun_kk_stats.npz"))


@pytest.fixture(scope="module")
def run41():
    return np.load(os.path.join(GOLDEN, "refrun_kk_test_41.npz"))


@pytest.fixture(scope="module")
def ctx():
    from hipdrt import _ffi
    return _ffi.get_context(0)


def host_stats(freq, err, n_iter=2, p_thresh=1e-4, n_sigma=None, fraction=0.6, max_out=2):
    """models.kk on one residual vector -> (mask, std, status, f_lim, i_lim) in the kernel's output conventions"""
    from hipdrt.models import kk
    idx, std = kk.get_outliers(err, n_iter, p_thresh, n_sigma, fraction, return_std=True)
    mask = np.zeros(len(freq), dtype=bool)
    mask[idx] = True
    try:
        f_lim, i_lim = kk.get_limits(freq, idx, max_num_outliers=max_out, return_index=True)
        return mask, std, 0, np.array(f_lim), np.array(i_lim)
    except IndexError:
        return mask, std, 1, np.array([np.nan, np.nan]), np.array([-1, -1])


def check_against_host(label, out, b, host, std_of=None):
    """std_of: the residual vector the device's std is to be checked against when the host's own differs from the device's at
    rounding level (the 1e-12 is for identical inputs)"""
    mask, std, status, f_lim, i_lim = host
    if std_of is not None:
        std = host_stats(np.logspace(1, 0, len(std_of)), std_of)[1]
    assert np.array_equal(out["outlier_mask"][b] != 0, mask), label
    assert int(out["status"][b]) == status, label
    assert out["i_lim"][b].tolist() == i_lim.tolist(), label
    assert np.array_equal(out["f_lim"][b], f_lim, equal_nan=True), label
    print(f"{label}: std device {out['std'][b]!r} host {std!r}")
    assert abs(out["std"][b] - std) <= 1e-12 * abs(std), (label, out["std"][b], std)


def test_statistics_stage_alone(stats, ctx):
    """hipdrt_debug_kk_stats on the fixture's residuals: the cases that share a grid and options go into ONE launch (clean,
    outliers at either end, adjacent ones, the trimming branch, no clean point side by side)"""
    from hipdrt import _ffi
    from hipdrt.models import kk
    names = [str(n) for n in stats["case_names"]]
    groups = {}
    for i in range(len(names)):
        key = (stats[f"c{i}_freq"].tobytes(), stats[f"c{i}_opts"].tobytes())
        groups.setdefault(key, []).append(i)
    assert max(len(g) for g in groups.values()) >= 5
    mixed = 0
    for members in groups.values():
        i0 = members[0]
        freq = stats[f"c{i0}_freq"]
        n_iter, p_thresh, n_sigma, fraction, max_out = stats[f"c{i0}_opts"]
        n_sigma = None if n_sigma <= 0 else float(n_sigma)
        opts = _ffi.kk_opts(n_outlier_iter=int(n_iter), p_thresh=p_thresh, n_sigma=n_sigma, std_sample_fraction=fraction,
                            n_std=kk.std_normal_quantile(0.5 + fraction / 2), max_num_outliers=int(max_out))
        err = np.stack([stats[f"c{i}_err"] for i in members])
        out = ctx.debug_kk_stats(freq, err, opts)
        mixed += len(set(out["status"].tolist())) > 1
        for b, i in enumerate(members):
            check_against_host(names[i], out, b, host_stats(freq, err[b], int(n_iter), p_thresh, n_sigma, fraction, int(max_out)))
            # ... and the reference's recorded values directly
            assert np.array_equal(np.where(out["outlier_mask"][b])[0], stats[f"c{i}_outliers"]), names[i]
            assert int(out["status"][b]) == int(stats[f"c{i}_status"]) and out["i_lim"][b].tolist() == stats[f"c{i}_ilim"].tolist()
    assert mixed >= 1                      # ok and "no clean point" in one launch


def planted(nf, positions, seed, scale=0.2):
    """noise of `scale` percent with large residuals at `positions`; the seed is advanced until every point keeps the fixtures'
    margin of 0.2 in ln(prob) from the threshold in both outlier iterations"""
    from hipdrt.models import kk
    for s in range(seed, seed + 100):
        rng = np.random.default_rng(s)
        err = scale * (rng.standard_normal(nf) + 1j * rng.standard_normal(nf))
        for i, k in enumerate(positions):
            err[k] = 12 * scale * (1, -1, 1j, -1j)[i % 4] * (1 + 0.3 * rng.random())
        mask, ok = np.zeros(nf, dtype=bool), True
        for _ in range(2):
            keep = err[~mask]
            std = kk.robust_std(np.concatenate([keep.real, keep.imag]), 0.6)
            lnp = -np.abs(err) ** 2 / (2 * std * std)
            ok = ok and np.min(np.abs(lnp - np.log(1e-4))) >= 0.2
            mask = lnp < np.log(1e-4)
        if ok:
            return err
    raise AssertionError("no seed with the margin")


@pytest.mark.parametrize("nf", [600, 2048])
def test_statistics_stage_beyond_one_pass_of_the_workgroup(nf, ctx):
    """more frequencies than the workgroup has threads (every loop strides), the largest size that must fit (nf = 2048: a
    4096-point sort), a trimming search over a long window, ascending and descending grids in two launches"""
    from hipdrt import _ffi
    from hipdrt.models import kk
    opts = _ffi.kk_opts(n_std=kk.std_normal_quantile(0.8))           # the host layer's n_std (upstream's tabulated quantile)
    pos = [5, 6, nf // 3, nf // 2, nf // 2 + 7, nf - 40, nf - 2]
    errs = np.stack([planted(nf, pos, 1000), planted(nf, [], 2000), planted(nf, list(range(1, nf, 3)), 3000)])
    for freq in (np.logspace(6, -2, nf), np.logspace(-2, 6, nf)):
        out = ctx.debug_kk_stats(freq, errs, opts)
        for b in range(len(errs)):
            check_against_host(f"nf{nf} vector {b}", out, b, host_stats(freq, errs[b]))
        assert out["status"].tolist() == [0, 0, 1]
        assert out["i_lim"][0].tolist() != [0, nf - 1]              # the window of vector 0 was cut


def test_statistics_stage_refuses_what_it_cannot_hold(ctx):
    from hipdrt import _ffi
    with pytest.raises(_ffi.HipDrtError, match="nf"):
        ctx.debug_kk_stats(np.logspace(6, -2, 5000), np.ones((1, 5000), dtype=complex))
    with pytest.raises(_ffi.HipDrtError, match="ascending or descending"):
        ctx.debug_kk_stats(np.array([3.0, 1.0, 2.0]), np.ones((1, 3), dtype=complex))
    with pytest.raises(_ffi.HipDrtError, match="std_sample_fraction"):
        ctx.debug_kk_stats(np.logspace(3, 0, 4), np.ones((1, 4), dtype=complex), _ffi.kk_opts(std_sample_fraction=1.5, n_std=1.0))


@pytest.fixture(scope="module")
def fitted41(run41):
    """the six spectra of the recorded run, fitted as kk_fit fits them (first pass)"""
    from hipdrt.models import DRT
    freq = run41["freq"]
    z = np.stack([run41[f"s{b}_z"] for b in range(6)])
    drt = DRT(extend_basis_decades=2)
    res = drt.fit_eis_batch(freq, z, nonneg=False, l2_lambda_0=1e-2)
    assert drt._plan.n == 113 and (res["status"] >= 0).all()
    return drt, freq, z


def test_screen_on_a_fitted_plan(fitted41):
    """stage A + B against models.kk on rm, rv, x of the same plan; then the row factors the screen leaves for the next fit"""
    from hipdrt.models import kk
    drt, freq, z = fitted41
    plan, nf = drt._plan, len(freq)
    opts = drt._kk_opts()
    out = plan.kk_screen(opts)
    rm, rv, x, cs = plan.get("rm"), plan.get("rv"), plan.get("x"), plan.get("coef_scale")
    yh = np.einsum("ij,bj->bi", rm, x)
    z_host = (yh[:, :nf] + 1j * yh[:, nf:]) * cs[:, None]
    e_host = kk.normalize_residuals(rv[:, :nf] + 1j * rv[:, nf:], yh[:, :nf] + 1j * yh[:, nf:])
    # summation order over n = 113 terms: ~ n eps = 1e-14 of the prediction, the residual is ~ 1e-3 of it
    parity("residuals", out["residuals"], e_host, default=1e-10)
    parity("z_hat", out["z_hat"], z_host, default=1e-10)
    for b in range(len(z)):
        check_against_host(f"spectrum {b}", out, b, host_stats(freq, e_host[b]), std_of=out["residuals"][b])
    assert (out["status"] == 0).all() and out["outlier_mask"].any()
    with pytest.raises(Exception):
        plan.get("row_factors")                          # no screen has set them yet
    out2 = plan.kk_screen(opts, set_row_factors=True, z_hat=False, residuals=False)
    assert np.array_equal(out2["outlier_mask"], out["outlier_mask"]) and np.array_equal(out2["f_lim"], out["f_lim"])
    rows = plan.get("row_factors")
    expected = np.where(out["outlier_mask"] != 0, 1e-10, 1.0)
    assert np.array_equal(rows, np.hstack([expected, expected]))
    plan.set_weight_factors(1.0)


def test_screen_outputs_are_optional(fitted41):
    drt, freq, z = fitted41
    out = drt._plan.kk_screen(None, z_hat=False, residuals=False)            # NULL options: the library's defaults
    assert "z_hat" not in out and out["outlier_mask"].shape == z.shape and np.isfinite(out["std"]).all()
    zh = drt.predict_z(drt.get_fit_frequencies())
    assert zh.shape == (len(freq),) and np.abs(zh - z[0]).max() < 0.1 * np.abs(z[0]).max()
    with pytest.raises(NotImplementedError, match="fit frequencies"):
        drt.predict_z(freq[:-1])


def check_pass(run41, b, p, freq, z, res, tag):
    """one spectrum of one pass against the recorded run: indices, limits, trimmed data exact; residuals relative to the peak"""
    pre = f"s{b}_p{p}_"
    assert np.array_equal(np.where(res["outlier_mask"])[0], run41[pre + "outliers"]), (tag, b, p)
    assert (res["f_min"], res["f_max"]) == tuple(run41[pre + "flim"]), (tag, b, p)
    assert np.array_equal(freq[res["clean_mask"]], run41[pre + "f_clean"]), (tag, b, p)
    assert np.array_equal(z[res["clean_mask"]], run41[pre + "z_clean"]), (tag, b, p)


def test_kk_test_batch_vs_reference_run(run41):
    """The documented tolerance of a fit-derived quantity is 1e-7 of the peak coefficient; a fraction 1e-7 on x is at most
    1e-7 * 100 / 1e-3 = 1e-2 of a percent-residual peak (the residual is ~ 1e-3 of the prediction).  Asserted relative to the peak
    of the recorded residuals; parity() records what is measured."""
    from hipdrt.models import DRT
    freq = run41["freq"]
    z = np.stack([run41[f"s{b}_z"] for b in range(6)])
    drt = DRT()
    out = drt.kk_test_batch(freq, z)
    assert drt.extend_basis_decades == 1 and len(out["passes"]) == 2 and (out["status"] == 0).all()
    for p, res in enumerate(out["passes"]):
        ref_err = np.stack([run41[f"s{b}_p{p}_err"] for b in range(6)])
        for b in range(6):
            one = {k: res[k][b] for k in ("outlier_mask", "f_min", "f_max", "clean_mask")}
            check_pass(run41, b, p, freq, z[b], one, "batch")
        parity(f"pass{p}.residuals", res["residuals"], ref_err, default=1e-2)
        ref_std = np.array([float(run41[f"s{b}_p{p}_std"]) for b in range(6)])
        print(f"pass {p}: std deviates by at most {np.max(np.abs(res['std'] - ref_std) / ref_std):.2e} (relative; not asserted)")
    assert np.array_equal(out["outlier_mask"], out["passes"][-1]["outlier_mask"])


@pytest.mark.parametrize("b", [1, 2])
def test_single_spectrum_kk_test_vs_reference_run(run41, b):
    from hipdrt.models import DRT
    freq, z = run41["freq"], run41[f"s{b}_z"]
    drt = DRT()
    idx, (f_min, f_max), (f_clean, z_clean) = drt.kk_test(freq, z, show_plot=False)
    pre = f"s{b}_p1_"
    assert np.array_equal(idx, run41[pre + "outliers"])
    assert (f_min, f_max) == tuple(run41[pre + "flim"])
    assert np.array_equal(f_clean, run41[pre + "f_clean"]) and np.array_equal(z_clean, run41[pre + "z_clean"])
    parity("residuals", drt.eval_kk_residuals(), run41[pre + "err"], default=1e-2)
    assert drt.extend_basis_decades == 1 and np.array_equal(drt.get_fit_frequencies(), freq)
    # the first pass alone, through the separate methods
    drt.kk_fit(freq, z)
    first = drt.get_kk_outliers()
    assert np.array_equal(first, run41[f"s{b}_p0_outliers"])
    assert drt.get_kk_limits(first) == tuple(run41[f"s{b}_p0_flim"])
    with pytest.raises(IndexError):
        drt.get_kk_limits(np.arange(0, len(freq), 2))           # an index set of the caller's own: no clean point


def test_fit_after_kk_test_batch_is_unchanged(run41):
    from hipdrt.models import DRT
    freq = run41["freq"]
    z = np.stack([run41[f"s{b}_z"] for b in range(6)])
    used, fresh = DRT(), DRT()
    used.kk_test_batch(freq, z)
    a, c = used.fit_eis_batch(freq, z), fresh.fit_eis_batch(freq, z)
    for key in ("x", "fit_x", "R_inf", "inductance", "weights", "rho", "q_vector", "s_vectors", "coefficient_scale"):
        assert np.array_equal(a[key], c[key]), key
    assert np.array_equal(a["outer_iters"], c["outer_iters"]) and np.array_equal(a["status"], c["status"])
