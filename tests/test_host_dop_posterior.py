"""CPU: the numpy statement of the DOP posterior (hipdrt/models/response.py: dop_cov_rows, dop_band) against runs of the reference
(tests/golden/refrun_dop_posterior_*.npz, written by tools/make_dop_posterior_golden.py: estimate_dop_cov and predict_dop_ci of
hybdrt/models/drt1d.py:3153-3258 on the fits of the refrun_response_predict_* files), and the argument rules of the new post-fit
methods against a recording stand-in for the prepared plan -- no device is touched.

Tolerance of the fixture checks: 1e-9 of each array's largest magnitude.  dop_cov_rows follows upstream's own route (np.linalg.inv,
the two-sided rescaling, E cov E'), so the two differ by the numpy / LAPACK builds of the machine that wrote the fixture and the one
that reads it alone.  Measured where the fixtures were written: 0 on every array of every case (the same build on both sides)."""
import os
import warnings

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

CASES = ("golden71_dop", "hybrid_s0_dop", "hybrid_s0_dop_solverp")
TOL = 1e-9


@pytest.fixture(scope="module", params=CASES)
def fx(request):
    return request.param, np.load(os.path.join(GOLDEN, f"refrun_dop_posterior_{request.param}.npz"))


def close(what, got, want):
    got, want = np.asarray(got, dtype=float), np.asarray(want, dtype=float)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    err = float(np.max(np.abs(got - want))) / float(np.max(np.abs(want)))
    print(f"{what}: deviation {err:.2e} of the largest magnitude")
    assert err <= TOL, (what, err)


def cov_of(g, bm, normalize_by=None):
    from hipdrt.models import response
    return response.dop_cov_rows(g["p_matrix"], int(g["dop_indices"][0]), g["dop_scale_vector"], float(g["coefficient_scale"]), bm,
                                 normalize_by)


def test_fixture_holds_what_the_tests_need(fx):
    name, g = fx
    a, e = g["dop_indices"]
    n = g["p_matrix"].shape[0]
    assert g["p_matrix"].shape == (n, n) and e - a == len(g["dop_scale_vector"]) == len(g["basis_nu"]) == 50
    assert len(g["nu"]) == 1034 and np.all(np.diff(g["nu"]) > 0) and np.all(np.diff(g["nu7"]) > 0)
    assert np.all(g["dop_scale_vector"] > 0) and np.all(np.linalg.eigvalsh(g["p_matrix"]) > 0)
    for order in (0, 1, 2):
        assert g[f"basis_matrix_o{order}"].shape == (1034, 50)
        for norm in (0, 1):
            assert np.all(g[f"var_o{order}_n{norm}"] >= 0) and np.all(g[f"hi_o{order}_n{norm}"] >= g[f"lo_o{order}_n{norm}"])
    assert os.path.getsize(os.path.join(GOLDEN, f"refrun_dop_posterior_{name}.npz")) < 1 << 20


def test_diagonals_and_bands_on_the_long_grid(fx):
    from hipdrt.models import response
    name, g = fx
    for order in (0, 1, 2):
        for norm in (0, 1):
            tag = f"o{order}_n{norm}"
            var = np.diag(cov_of(g, g[f"basis_matrix_o{order}"], g["normalize_by"] if norm else None))
            close(f"{name} var_{tag}", var, g[f"var_{tag}"])
            lo, hi = response.dop_band(g[f"mu_{tag}"], var, (0.025, 0.975))
            close(f"{name} lo_{tag}", lo, g[f"lo_{tag}"])
            close(f"{name} hi_{tag}", hi, g[f"hi_{tag}"])
    var = np.diag(cov_of(g, g["basis_matrix_o0"]))
    lo, hi = response.dop_band(g["mu_o0_n0"], var, tuple(g["q2"]))
    close(f"{name} lo_q2", lo, g["lo_q2"])
    close(f"{name} hi_q2", hi, g["hi_q2"])
    assert not np.allclose(lo, g["lo_o0_n0"])


def test_full_matrices_and_var_floor(fx):
    from hipdrt.matrices import basis
    name, g = fx
    for tag in ("basis", "nu7"):
        grid = g["basis_nu"] if tag == "basis" else g["nu7"]
        bm = basis.construct_func_eval_matrix(g["basis_nu"], grid, "gaussian", epsilon=float(g["nu_epsilon"]), order=0)
        plain, normed = cov_of(g, bm), cov_of(g, bm, g[f"normalize_by_{tag}"])
        close(f"{name} cov_{tag}_n0", plain, g[f"cov_{tag}_n0"])
        close(f"{name} cov_{tag}_n1", normed, g[f"cov_{tag}_n1"])
        # upstream's broadcast: column j is divided by normalize_by[j]^2
        np.testing.assert_allclose(normed, plain / g[f"normalize_by_{tag}"][None, :] ** 2, rtol=1e-15)
        assert not np.allclose(normed, normed.T, rtol=1e-6)
    floor = float(g["var_floor"])
    bm = basis.construct_func_eval_matrix(g["basis_nu"], g["basis_nu"], "gaussian", epsilon=float(g["nu_epsilon"]), order=0)
    cov = cov_of(g, bm)
    var = np.diag(cov).copy()
    assert (var < floor).any() and (var > floor).any()
    var[var < floor] = floor
    np.fill_diagonal(cov, var)
    close(f"{name} cov_basis_floor", cov, g["cov_basis_floor"])


def test_scaling_p_is_the_same_quadratic_form(fx):
    """the identity the device relies on: inv(S P S) = D inv(P) D, S = 1 / D on the DOP block"""
    name, g = fx
    a, e = g["dop_indices"]
    s = np.ones(g["p_matrix"].shape[0])
    s[a:e] = 1.0 / g["dop_scale_vector"]
    M = (g["p_matrix"] * s[:, None]) * s[None, :]
    L = np.linalg.cholesky(M)
    E = np.zeros((1034, len(s)))
    E[:, a:e] = g["basis_matrix_o0"]
    Y = np.linalg.solve(L, E.T)
    var = np.sum(Y * Y, axis=0) * float(g["coefficient_scale"]) ** 2
    err = np.max(np.abs(var - g["var_o0_n0"])) / np.max(g["var_o0_n0"])
    print(f"{name}: Cholesky of S P S against the reference's route: {err:.2e} of the largest variance, kappa_2(P) "
          f"{np.linalg.cond(g['p_matrix']):.3g}")
    assert err < 1e-9


# ---- the argument rules of the post-fit methods, without a device -----------------------------------------------------------------
B, ND, A0 = 3, 50, 4
BASIS_NU = np.linspace(-1, 1, ND + 2)[1:-1]
F71 = np.logspace(5, -2, 71)


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "hybrid-drt_amd", "libhipdrt.so")):
        g.build()
    from hipdrt import _ffi
    _ffi.load_library()
    return _ffi


def make_drt(ffi, dop=True, status=(0, 0, 0)):
    from hipdrt.models import DRT

    class FakePlan(ffi.PreparedPlan):
        def __init__(self):
            self.batch, self.calls, self.status = B, [], np.array(status, dtype=np.int32)

        def set_tau_basis(self, *a):
            pass

        def set_predict_desc(self, *a, **kw):
            self.calls.append(("set_predict_desc", kw))

        def dop_posterior(self, nu, basis_nu, nu_epsilon, **kw):
            self.calls.append(("dop_posterior", dict(kw, nu=np.array(nu))))
            mu = np.arange(1.0, B + 1)[:, None] * (1.0 + np.arange(len(nu)))[None, :]
            band = kw.get("n_sigma") is not None
            var = mu * 4.0 if kw.get("want_var", True) else None
            return mu, (mu - 1 if band else None), (mu + 2 if band else None), var, self.status.copy()

        def dop_cov(self, member, nu, basis_nu, nu_epsilon, **kw):
            self.calls.append(("dop_cov", dict(kw, nu=np.array(nu), member=member)))
            k = np.arange(1.0, len(nu) + 1)
            return np.outer(k, k) + 10.0 * member, int(self.status[member])

    drt = DRT(warn=False)
    drt.basis_tau, drt.basis_nu, drt.nu_epsilon = np.logspace(-7, 2, 91), BASIS_NU, 12.5
    drt.fit_kwargs = dict(nonneg=True, inductance_scale=1e-5, capacitance_scale=1e-3)
    drt.special_qp_params = {'R_inf': {'index': 0}, 'inductance': {'index': 1}}
    members = [dict(coefficient_scale=cs, frequencies=F71, sample_times=None, nonconsec_step_times=None, step_times=None, num_chrono=0,
                    dop=(A0, A0 + ND) if dop else None, dop_scale_vector=np.full(ND, 1.0 + k)) for k, cs in enumerate((2.0, 0.5, 3.0))]
    drt._plan, drt._prep, drt._last_prepared = FakePlan(), members[0], (members, None)
    return drt


def last(drt, name):
    return next(kw for n, kw in reversed(drt._plan.calls) if n == name)


def test_refusals(ffi):
    from hipdrt.models import DRT
    drt = make_drt(ffi)
    methods = (drt.predict_dop_ci_batch, drt.predict_dop_ci, drt.estimate_dop_var_batch, drt.estimate_dop_cov)
    for call in methods:
        with pytest.raises(NotImplementedError, match="delta_density=True is not taken"):
            call(delta_density=True)
        with pytest.raises(ValueError, match="Invalid order 3"):
            call(order=3)
    with pytest.raises(NotImplementedError, match="x= override is not taken"):
        drt.predict_dop_ci(x=np.ones(3))
    with pytest.raises(NotImplementedError, match="p_matrix= override is not taken"):
        drt.estimate_dop_cov(p_matrix=np.eye(3))
    assert not drt._plan.calls
    for unfit in (DRT(warn=False), make_drt(ffi, dop=False)):
        for call in (unfit.predict_dop_ci_batch, unfit.predict_dop_ci, unfit.estimate_dop_var_batch, unfit.estimate_dop_cov):
            with pytest.raises(RuntimeError):
                call()
    with pytest.raises(RuntimeError, match="needs a finished fit with fit_dop=True"):
        make_drt(ffi, dop=False).estimate_dop_cov()


def test_grids_quantiles_and_normalisation(ffi):
    from hipdrt import preprocessing as pp
    from hipdrt.models import predict, response
    drt = make_drt(ffi)
    grid = np.unique(np.concatenate([BASIS_NU, np.linspace(-1, 1, 1001), [-1, 0, 1]]))
    lo, hi, ok, info = drt.predict_dop_ci_batch(return_info=True)
    kw = last(drt, "dop_posterior")
    np.testing.assert_array_equal(kw["nu"], grid)                       # predict_dop's grid for mean AND sigma
    np.testing.assert_array_equal(info["nu"], grid)
    assert kw["n_sigma"] == predict.n_sigma((0.025, 0.975)) and kw["normalize_by"] is None and kw["order"] == 0
    assert kw["include_ideal"] is True and kw["want_var"] is True and ok.tolist() == [True] * 3
    np.testing.assert_array_equal(info["sigma"], np.sqrt(info["mu"] * 4.0))
    np.testing.assert_array_equal(lo, info["mu"] - 1)
    assert kw["nu_basis_area"] == np.sqrt(np.pi) / 12.5
    # the scales every member carries reach the plan before the call
    desc = last(drt, "set_predict_desc")
    np.testing.assert_array_equal(desc["dop_scale_vector"], np.stack([np.full(ND, 1.0 + k) for k in range(B)]))
    # an unsorted grid: both on the sorted one; predict_dop_ci's own normalize_quantiles
    nu7 = np.array([0.9, -1.0, 0.0, -0.45, 0.5, 1.0, -0.8])
    drt.predict_dop_ci_batch(nu=nu7, normalize=True, quantiles=(0.16, 0.84), order=2, include_ideal=False)
    kw = last(drt, "dop_posterior")
    np.testing.assert_array_equal(kw["nu"], np.sort(nu7))
    tau_lim = pp.get_tau_lim(F71, None, None)
    np.testing.assert_array_equal(kw["normalize_by"], response.dop_norm(np.sort(nu7), tau_lim, 12.5, (0.25, 0.75)))
    assert kw["n_sigma"] == predict.n_sigma((0.16, 0.84)) and kw["order"] == 2 and kw["include_ideal"] is False
    assert kw["want_var"] is False
    # the covariance takes basis_nu, as upstream; rows and columns come back in the caller's order
    var, ok = drt.estimate_dop_var_batch()
    np.testing.assert_array_equal(last(drt, "dop_posterior")["nu"], BASIS_NU)
    assert "n_sigma" not in last(drt, "dop_posterior")                  # (no band: the variance alone)
    assert var.shape == (B, ND)
    var7, _ = drt.estimate_dop_var_batch(nu=nu7)
    order = np.argsort(nu7)
    np.testing.assert_array_equal(var7[:, order], 4.0 * np.arange(1.0, B + 1)[:, None] * (1.0 + np.arange(7))[None, :])
    cov = drt.estimate_dop_cov(nu=nu7, b=2)
    k = np.arange(1.0, 8)
    np.testing.assert_array_equal(cov[np.ix_(order, order)], np.outer(k, k) + 20.0)
    assert last(drt, "dop_cov")["member"] == 2
    np.testing.assert_array_equal(drt.estimate_dop_cov().shape, (ND, ND))
    np.testing.assert_array_equal(last(drt, "dop_cov")["nu"], BASIS_NU)


def test_var_floor_and_a_p_that_is_not_positive_definite(ffi):
    drt = make_drt(ffi)
    plain = drt.estimate_dop_cov(nu=[-0.5, 0.0, 0.5])
    floored = drt.estimate_dop_cov(nu=[-0.5, 0.0, 0.5], var_floor=3.0)
    np.testing.assert_array_equal(np.diag(plain), [1.0, 4.0, 9.0])
    np.testing.assert_array_equal(np.diag(floored), [3.0, 4.0, 9.0])
    off = ~np.eye(3, dtype=bool)
    np.testing.assert_array_equal(floored[off], plain[off])
    bad = make_drt(ffi, status=(0, ffi.PREDICT_NOT_PD, 0))
    lo, hi, ok = bad.predict_dop_ci_batch(nu=[0.0, 0.5])
    assert ok.tolist() == [True, False, True]
    assert bad.estimate_dop_var_batch(nu=[0.0])[1].tolist() == [True, False, True]
    with pytest.warns(UserWarning, match="Singular P matrix - could not obtain covariance estimate"):
        assert bad.predict_dop_ci(nu=[0.0, 0.5], b=1) == (None, None)
    with pytest.warns(UserWarning, match="Singular P matrix"):
        assert bad.estimate_dop_cov(nu=[0.0], b=1) is None
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        lo0, hi0 = bad.predict_dop_ci(nu=[0.0, 0.5], b=0)
    np.testing.assert_array_equal(lo0, lo[0])
