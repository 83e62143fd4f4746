"""CPU: hipdrt.models.kk -- the numpy statement of the KK screen kernel's statistics stage -- reproduces what the reference's
kk.get_outliers / kk.get_limits returned for the residual vectors and masks of tests/golden/refrun_kk_stats.npz
(tools/make_kk_golden.py), and the host side of DRT.kk_fit / kk_test builds what the reference builds.

Every accepted case keeps every point at least 0.2 in ln(prob) away from the threshold, so masks and limits are compared
exactly; std is a handful of double operations on identical inputs and must agree to 1e-12 relative."""
import os

import numpy as np
import pytest

from conftest import GOLDEN


@pytest.fixture(scope="module")
def stats():
    return np.load(os.path.join(GOLDEN, "refrun_kk_stats.npz"))


def case_opts(d, i):
    n_iter, p_thresh, n_sigma, fraction, max_out = d[f"c{i}_opts"]
    return dict(n_iter=int(n_iter), p_thresh=float(p_thresh), n_sigma=None if n_sigma <= 0 else float(n_sigma),
                std_sample_fraction=float(fraction)), int(max_out)


def test_fixture_covers_the_cases(stats):
    names = [str(n) for n in stats["case_names"]]
    for nf in (3, 7, 41, 64):
        for order in ("asc", "desc"):
            assert f"none_nf{nf}_{order}" in names and f"first_nf{nf}_{order}" in names and f"last_nf{nf}_{order}" in names
    for key in ("adjacent", "trim_mo0", "trim_mo2", "tie_mo1", "n_sigma", "no_clean_point"):
        assert any(n.startswith(key) for n in names), key
    assert any(int(stats[f"c{i}_status"]) == 1 for i in range(len(names)))
    assert all(float(stats[f"c{i}_margin"]) >= 0.2 for i in range(len(names)))


def test_outliers_and_std_match_the_reference(stats):
    from hipdrt.models import kk
    for i, name in enumerate(stats["case_names"]):
        kw, _ = case_opts(stats, i)
        idx, std = kk.get_outliers(stats[f"c{i}_err"], return_std=True, **kw)
        assert np.array_equal(idx, stats[f"c{i}_outliers"]), name
        ref = float(stats[f"c{i}_std"])
        assert abs(std - ref) <= 1e-12 * abs(ref), (name, std, ref)
        assert np.array_equal(kk.get_outliers(stats[f"c{i}_err"], kw["n_iter"], kw["p_thresh"], kw["n_sigma"],
                                              kw["std_sample_fraction"]), idx)          # the reference's positional form


def check_limits(kk, name, freq, outliers, max_out, status, flim, ilim):
    if status == 1:
        with pytest.raises(IndexError):
            kk.get_limits(freq, outliers, max_num_outliers=max_out)
        return
    (f_min, f_max), (i_left, i_right) = kk.get_limits(freq, outliers, max_num_outliers=max_out, return_index=True)
    assert (f_min, f_max) == (flim[0], flim[1]), name
    assert (i_left, i_right) == (int(ilim[0]), int(ilim[1])), name
    assert kk.get_limits(freq, outliers, max_out) == (f_min, f_max)


def test_limits_match_the_reference(stats):
    from hipdrt.models import kk
    for i, name in enumerate(stats["case_names"]):
        _, max_out = case_opts(stats, i)
        check_limits(kk, str(name), stats[f"c{i}_freq"], stats[f"c{i}_outliers"], max_out, int(stats[f"c{i}_status"]),
                     stats[f"c{i}_flim"], stats[f"c{i}_ilim"])
    raised = 0
    for i in range(int(stats["num_masks"])):
        status = int(stats[f"m{i}_status"])
        raised += status
        check_limits(kk, f"mask {i}", stats[f"m{i}_freq"], np.where(stats[f"m{i}_mask"])[0], int(stats[f"m{i}_maxout"]), status,
                     stats[f"m{i}_flim"], stats[f"m{i}_ilim"])
    assert raised >= 1


def test_recorded_kk_test_passes_follow_from_their_residuals():
    """the six spectra of refrun_kk_test_41.npz: outliers, limits and trimmed data of both passes from the recorded residuals"""
    from hipdrt.models import kk
    d = np.load(os.path.join(GOLDEN, "refrun_kk_test_41.npz"))
    freq = d["freq"]
    assert int(d["num_spectra"]) == 6 and len(freq) == 41
    for b in range(6):
        for p in range(int(d["num_passes"])):
            pre = f"s{b}_p{p}_"
            assert float(d[pre + "margin"]) >= 0.2
            idx, std = kk.get_outliers(d[pre + "err"], return_std=True)
            assert np.array_equal(idx, d[pre + "outliers"]), pre
            assert abs(std - float(d[pre + "std"])) <= 1e-12 * float(d[pre + "std"]), pre
            f_min, f_max = kk.get_limits(freq, idx)
            assert (f_min, f_max) == tuple(d[pre + "flim"]), pre
            f_clean, z_clean = kk.trim_data(freq, d[f"s{b}_z"], f_min, f_max)
            assert np.array_equal(f_clean, d[pre + "f_clean"]) and np.array_equal(z_clean, d[pre + "z_clean"]), pre


def test_degenerate_samples_mask_nothing():
    from hipdrt.models import kk
    assert len(kk.get_outliers(np.zeros(5, dtype=complex))) == 0                  # std 0
    assert len(kk.get_outliers(np.array([1 + 1j, np.nan, 2 - 1j]))) == 0          # std not finite
    idx, std = kk.get_outliers(np.array([1 + 2j]), n_iter=0, return_std=True)
    assert len(idx) == 0 and np.isnan(std)
    assert np.isnan(kk.robust_std(np.array([1.0])))


def test_normalize_residuals_and_trim_data():
    from hipdrt.models import kk
    z = np.array([3 + 4j, 1j, -2 + 0j])
    zp = np.array([3 + 3j, 0.5j, -1 + 0j])
    assert np.allclose(kk.normalize_residuals(z, zp), [20j, 50j, -50], rtol=1e-15)
    with pytest.raises(ValueError):
        kk.normalize_residuals(z, zp, norm="real")
    f = np.array([100.0, 10.0, 1.0])
    ft, zt = kk.trim_data(f, z, 1.0, 10.0)
    assert ft.tolist() == [10.0, 1.0] and zt.tolist() == [1j, -2 + 0j]


def test_n_std_is_the_reference_table_value():
    """stats.std_normal_quantile interpolates a cdf table: 0.84162417 for 0.8 (exact quantile 0.84162123); std follows it"""
    from hipdrt.models import kk
    assert abs(kk.std_normal_quantile(0.8) - 0.8416241734049236) < 1e-15
    assert abs(kk.std_normal_quantile(0.8) - 0.8416212335729143) < 1e-5


def test_bad_arguments_raise():
    from hipdrt.models import DRT, kk
    with pytest.raises(ValueError):
        kk.get_outliers(np.ones(4, dtype=complex), p_thresh=1.5)
    with pytest.raises(ValueError):
        kk.get_outliers(np.ones(4, dtype=complex), n_sigma=-1.0)
    with pytest.raises(ValueError):
        kk.get_outliers(np.ones(4, dtype=complex), std_sample_fraction=1.5)
    with pytest.raises(ValueError):
        kk.get_limits(np.logspace(3, 0, 5), [1], max_num_outliers=-1)
    with pytest.raises(IndexError):
        kk.get_limits(np.logspace(3, 0, 5), [0, 2, 4])
    drt = DRT()
    freq = np.logspace(3, 0, 5)
    with pytest.raises(ValueError):
        drt.kk_test_batch(freq, np.ones((2, 4), dtype=complex))              # shape
    with pytest.raises(ValueError):
        drt.kk_test_batch(freq, np.ones((2, 5), dtype=complex), norm="real")
    with pytest.raises(ValueError):
        drt.kk_test_batch(freq, np.ones((2, 5), dtype=complex), n_iter=0)
    with pytest.raises(ValueError):
        drt.kk_test(freq, np.ones(5, dtype=complex), n_iter=0)
    with pytest.raises(NotImplementedError):
        drt.predict_z(freq)                                                  # nothing fitted
    with pytest.raises(NotImplementedError):
        drt.get_kk_outliers()
    with pytest.raises(ValueError):
        drt.eval_kk_residuals(norm="real")


def test_kk_fit_builds_the_weight_factor_vector_and_restores_the_basis_extension(monkeypatch):
    """drt1d.py:1393-1411: extend_basis_decades swapped for the call only; outliers get 1e-10 on their Re and Im rows"""
    from hipdrt.models import DRT
    drt = DRT(extend_basis_decades=1)
    seen = {}

    def fake_fit_eis(frequencies, z, **kw):
        seen.update(kw, extend=drt.extend_basis_decades)

    monkeypatch.setattr(drt, "fit_eis", fake_fit_eis)
    freq = np.logspace(3, 0, 6)
    z = np.ones(6, dtype=complex)
    drt.kk_fit(freq, z)
    assert seen == dict(nonneg=False, l2_lambda_0=1e-2, weight_factor=1, extend=2) and drt.extend_basis_decades == 1
    drt.kk_fit(freq, z, extend_basis_decades=3, outlier_index=np.array([1, 4]), l2_lambda_0=0.5, nonneg=True)
    expected = np.ones(12)
    expected[[1, 4, 7, 10]] = 1e-10
    assert np.array_equal(seen["weight_factor"], expected) and seen["extend"] == 3 and seen["l2_lambda_0"] == 0.5
    assert drt.extend_basis_decades == 1

    def failing(frequencies, z, **kw):
        raise RuntimeError("fit failed")

    monkeypatch.setattr(drt, "fit_eis", failing)
    with pytest.raises(RuntimeError):
        drt.kk_fit(freq, z)
    assert drt.extend_basis_decades == 1


def test_kk_test_warns_about_plotting_and_carries_on(monkeypatch):
    from hipdrt.models import DRT
    drt = DRT()
    freq = np.logspace(3, 0, 6)
    z = np.arange(6) + 1j
    calls = []
    monkeypatch.setattr(drt, "kk_fit", lambda *a, **kw: calls.append(kw.get("outlier_index")))
    monkeypatch.setattr(drt, "get_kk_outliers", lambda **kw: np.array([2]))
    monkeypatch.setattr(drt, "get_kk_limits", lambda idx, max_num_outliers=2: (1.0, 100.0))
    with pytest.warns(UserWarning, match="plotting"):
        idx, lim, (f_clean, z_clean) = drt.kk_test(freq, z)
    assert calls[0] is None and np.array_equal(calls[1], [2]) and len(calls) == 2
    assert idx.tolist() == [2] and lim == (1.0, 100.0)
    assert np.array_equal(f_clean, freq[(freq <= 100.0) & (freq >= 1.0)])
