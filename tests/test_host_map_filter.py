"""CPU: the map filter's host layers -- the numpy statement hipdrt.filters.ndfilters against the reference's own runs
(tests/golden/refrun_map_filter.npz, every case and recorded intermediate), filter_ndx's refusals, the bookkeeping of
DRTMD.filter_observations / filter_group / get_group_index with a stand-in for the device filter, and the C-ABI declaration."""
import json
import os
import re
import warnings

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

CASES = ["s3x5", "s23_tau_skipped", "s23", "s23_plain", "s23_impute", "s23_adaptive", "s23_adaptive_plain", "s23_wide", "s70",
         "s70_plain", "s70_impute", "s70_adaptive", "v23"]


def load_fixture():
    g = np.load(os.path.join(GOLDEN, "refrun_map_filter.npz"))
    out = {}
    for k in g.files:
        v = g[k]
        out[k] = g[str(v)[1:]] if v.dtype.kind == "U" and str(v).startswith("=") else v      # "=key": stored once under key
    return out


def case_kw(fx, name):
    kw = json.loads(str(fx[f"{name}_kw"]))
    return {k: tuple(v) if isinstance(v, list) else v for k, v in kw.items()}


def deviation(actual, ref):
    actual, ref = np.asarray(actual), np.asarray(ref)
    assert actual.shape == ref.shape
    np.testing.assert_array_equal(np.isnan(actual), np.isnan(ref))
    return float(np.nanmax(np.abs(actual - ref)) / np.nanmax(np.abs(ref)))


def statement_case(fx, name):
    """label -> (numpy statement, reference) for the output and every recorded intermediate of a case"""
    from hipdrt.filters import ndfilters
    from hipdrt.mapping.ndx import filter_ndx_statement
    a, kw = fx[f"{name}_in"], case_kw(fx, name)
    with np.errstate(invalid="ignore", divide="ignore"):
        res = {f"{name}:out": (filter_ndx_statement(a.copy(), 0, **kw), fx[f"{name}_out"])}
        fkw = {k: v for k, v in kw.items() if k in ("sigma", "max_sigma")}
        x, nan = np.nan_to_num(a), np.isnan(a)
        adaptive = kw.get("adaptive", False)
        if kw.get("iterative", True):
            w = ndfilters.iterate_gaussian_weights(x, None, adaptive, 2, 5, dev_rms_size=5, nan_mask=nan, **fkw)
            res[f"{name}:weights"] = (w, fx[f"{name}_weights"])
            if adaptive:
                res[f"{name}:sigmas"] = (np.stack(ndfilters.get_adaptive_sigmas(x, empty=False, weights=w, **fkw)), fx[f"{name}_sigmas"])
        elif adaptive:
            res[f"{name}:sigmas"] = (np.stack(ndfilters.get_adaptive_sigmas(x, weights=(~nan).astype(float), **fkw)), fx[f"{name}_sigmas"])
    return res


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


@pytest.fixture(scope="module")
def bounds():
    with open(os.path.join(ROOT, "tests", "map_filter_bounds.json")) as f:
        return json.load(f)


def test_fixture_holds_the_cases_of_the_issue(fx):
    assert list(fx["cases"]) == CASES
    shapes = {name: fx[f"{name}_in"].shape for name in CASES}
    assert shapes["s3x5"] == (3, 5) and shapes["s23"] == (23, 37) and shapes["s70"] == (70, 130) and shapes["v23"] == (23,)
    assert case_kw(fx, "s23_tau_skipped") == {"sigma": (1, 0)} and case_kw(fx, "s70_adaptive") == {"adaptive": True, "max_sigma": (2, 1)}
    for name in CASES:
        a = fx[f"{name}_in"]
        assert np.isnan(a).any() and (a.ndim == 1 or np.isnan(a).all(axis=1).sum() == 1)      # scattered NaNs, one all-NaN row


@pytest.mark.parametrize("name", CASES)
def test_numpy_statement_matches_the_reference_run(fx, bounds, name):
    for label, (actual, ref) in statement_case(fx, name).items():
        err = deviation(actual, ref)
        print(f"map_filter numpy {label}: measured {err:.2e} bound {bounds['numpy'][label][1]:.1e}")
        assert err <= bounds["numpy"][label][1], (label, err)


def test_bounds_table_covers_both_sections_and_keeps_its_rule(bounds):
    # ("kernels": the adaptive passes of tests/test_gpu_map_kernels.py against ndfilters, under the same rule)
    assert set(bounds) == {"device", "numpy", "kernels"}
    for name in CASES:
        assert f"{name}:out" in bounds["device"] and f"{name}:out" in bounds["numpy"]
    import map_kernels_util
    assert set(bounds["kernels"]) == set(map_kernels_util.ADAPTIVE_CASES)
    for rows in bounds.values():
        for label, (measured, bound) in rows.items():
            assert bound >= 10 * measured and bound >= 5e-15, label
            assert f"{bound:.0e}"[0] in "125" and float(f"{bound:.0e}") == bound, label


def test_correlate_reflects_repeatedly_past_the_axis_length():
    from hipdrt.filters import ndfilters
    a = np.array([1.0, 2.0, 4.0])
    w = np.zeros(15)
    w[0] = 1.0                                  # picks a[i - 7]: d c b a | a b c d | d c b a
    tiled = np.concatenate([a[::-1], a, a[::-1], a, a[::-1], a])              # positions -9 .. 8
    np.testing.assert_array_equal(ndfilters.correlate1d_reflect(a, w), tiled[9 + np.arange(3) - 7])
    assert ndfilters.reflect_index(np.array([-1, -3, -4, 3, 6, 7]), 3).tolist() == [0, 2, 2, 2, 0, 1]


def test_rms_filter_uses_upstreams_formula_for_degenerate_neighbourhoods():
    from hipdrt.filters import ndfilters
    a = np.zeros((5, 6))
    a[2, 3] = 2.0
    r = ndfilters.rms_filter(a, 5, empty=True)
    assert r[2, 3] == 0.0 and r[0, 0] == 0.0                                   # (4/25 - 4/25) * 25/24, clipped
    np.testing.assert_allclose(r[2, 2], np.sqrt(4.0 / 25 * 25 / 24), rtol=1e-15)
    np.testing.assert_array_equal(ndfilters.rms_filter(np.ones(7), 5, empty=True), np.ones(7))


def test_filter_ndx_refuses_what_is_not_built():
    from hipdrt.mapping.ndx import filter_ndx
    a = np.ones((4, 5))
    for kw, word in ((dict(filter_func=lambda x, **k: x), "filter_func"), (dict(by_group=True), "by_group"),
                     (dict(num_group_dims=1), "num_group_dims")):
        kw = dict(dict(num_group_dims=0), **kw)
        with pytest.raises(NotImplementedError, match=word):
            filter_ndx(a, sigma=(1, 0), **kw)
    with pytest.raises(NotImplementedError, match="two dimensions"):
        filter_ndx(np.ones((2, 3, 4)), 0, sigma=1)
    with pytest.raises(ValueError, match="Group imputation"):
        filter_ndx(a, 0, impute_groups=True, by_group=True, sigma=1)


def test_existing_1d_filter_keeps_its_refusal():
    from hipdrt import filters
    with pytest.raises(NotImplementedError, match="only the 1-D, order-0, reflect-mode filter"):
        filters.nonuniform_gaussian_filter1d(np.ones((3, 4)), np.ones((3, 4)))
    for name in ("masked_filter", "iterative_gaussian_filter", "adaptive_gaussian_filter", "get_adaptive_sigmas"):
        assert callable(getattr(filters, name))
    with pytest.raises(NotImplementedError, match="filter_func"):
        filters.masked_filter(np.ones(4), np.ones(4), filter_func=lambda x: x)
    with pytest.raises(NotImplementedError, match="sigmas=None"):
        filters.adaptive_gaussian_filter(np.ones(4))


def test_header_and_ctypes_table_hold_the_symbol():
    from hipdrt import _ffi
    txt = open(os.path.join(ROOT, "include", "hipdrt.h")).read()
    assert re.search(r"\bint\s+hipdrt_map_filter\s*\(", txt) and "ndx.py:261-349" in txt and "_filters.py" in txt
    assert len(_ffi.SIGNATURES["hipdrt_map_filter"]) == 6 and hasattr(_ffi.Context, "map_filter")
    fields = [n for n, _ in _ffi.MapFilterArgs._fields_]
    decl = re.search(r"typedef struct \{\s*int ndim, rows, cols;(.*?)\} hipdrt_map_filter_args;", txt, flags=re.S).group(1)
    decl = re.sub(r"/\*.*?\*/", "", decl, flags=re.S)
    names = re.findall(r"(\w+)(?:\[\d\])?\s*[,;]", decl)
    assert ["ndim", "rows", "cols"] + names == fields


# ---- the store's bookkeeping, with a stand-in for the device filter ---------------------------------------------------------
class _NoDevice:
    pass


@pytest.fixture
def fake_filter(monkeypatch):
    """filter_ndx replaced by a recorder that returns its input plus 100"""
    from hipdrt.mapping import store
    calls = []

    def filter_ndx(ndx, num_group_dims, **kw):
        calls.append((np.array(ndx), num_group_dims, kw))
        return np.asarray(ndx) + 100.0

    monkeypatch.setattr(store, "filter_ndx", filter_ndx)
    return calls


def _store(n=5, nt=7):
    from hipdrt.mapping import store
    md = store.DRTMD(np.logspace(-4, 1, nt), drt=_NoDevice(), psi_dim_names=["T", "p"])
    temps = [30.0, 10.0, 20.0, 10.0, 40.0]
    for k in range(n):
        md.add_observation([temps[k], float(k % 2)], None, None, group_id="a" if k < 4 else "b")
    md.obs_x[:] = np.arange(n)[:, None] * 10.0 + np.arange(nt)[None]
    md.obs_fit_status[:] = True
    md.obs_tau_indices = [(1, 6)] * n
    md.obs_special = {"R_inf": np.arange(n) + 0.5, "vz_offset": np.arange(n) + 0.25, "x_dop": np.arange(n)[:, None] + np.zeros((n, 3)),
                      "v_baseline": np.arange(n)[:, None] * np.ones((n, 2))}
    return md


def test_filter_observations_sorts_excludes_and_scatters(fake_filter):
    md = _store()
    md.obs_fit_status[2] = False                      # unfitted
    md.obs_ignore_flag[4] = True                      # ignored
    md.obs_tau_indices[3] = (2, 7)
    md.filter_observations(np.arange(5), psi_sort_dims=["T", "p"], resolved=False, sigma=(1.5, 0.5), iterative=False)
    order = sorted([0, 1, 3], key=lambda i: (md.obs_psi[i, 0], md.obs_psi[i, 1]))
    assert order == [1, 3, 0]
    x_in, ngd, kw = fake_filter[0]
    assert ngd == 0 and kw == dict(sigma=(1.5, 0.5), iterative=False)
    np.testing.assert_array_equal(x_in, md.obs_x[order, 1:7])                 # truncate=False: the longest window (1, 7)
    np.testing.assert_array_equal(md.obs_x_filt[order, 1:7], md.obs_x[order, 1:7] + 100.0)
    assert not md.obs_x_filt[[2, 4]].any() and not md.obs_x_filt[:, 0].any()
    by_key = {}
    for arr, _, kw in fake_filter[1:]:
        by_key[arr.shape[1:]] = kw
    assert by_key[(3,)] == dict(sigma=(1.5, 0.5), iterative=False)            # x_dop: filtered with kw
    assert by_key[()] == dict(sigma=(1.5,), iterative=False)                  # R_inf: the tau entry of sigma dropped
    assert len(fake_filter) == 3                                              # vz_offset and v_baseline are not filtered
    np.testing.assert_array_equal(md.obs_special_filt["vz_offset"][order], md.obs_special["vz_offset"][order])
    np.testing.assert_array_equal(md.obs_special_filt["v_baseline"][order], md.obs_special["v_baseline"][order])
    np.testing.assert_array_equal(md.obs_special_filt["R_inf"][order], md.obs_special["R_inf"][order] + 100.0)
    assert md.obs_special_filt["R_inf"][[2, 4]].tolist() == [0.0, 0.0] and md.obs_special_filt["x_dop"].shape == (5, 3)


def test_truncate_special_kw_and_scalar_sigma(fake_filter):
    md = _store()
    md.obs_tau_indices[3] = (2, 7)
    md.filter_observations(np.array([0, 3]), truncate=True, resolved=False, special_kw=dict(sigma=(3,)), max_sigma=(2, 1), adaptive=True)
    assert fake_filter[0][0].shape == (2, 4)                                   # the window every observation covers: (2, 6)
    kws = [kw for _, _, kw in fake_filter[1:]]
    assert dict(max_sigma=(2, 1), adaptive=True) in kws and dict(sigma=(3,)) in kws
    fake_filter.clear()
    md.filter_observations(np.array([0, 3]), resolved=False, sigma=2)          # a scalar sigma stays as it is
    assert all(kw == dict(sigma=2) for _, _, kw in fake_filter)


def test_single_and_no_observation_and_resolved(fake_filter):
    md = _store()
    with pytest.warns(UserWarning, match="Only one observation"):
        md.filter_observations(np.array([1]), resolved=False, sigma=(1, 0))
    assert fake_filter == []
    np.testing.assert_array_equal(md.obs_x_filt[1, 1:6], md.obs_x[1, 1:6])
    assert md.obs_x_filt[1, 0] == 0.0 and md.obs_special_filt["R_inf"][1] == md.obs_special["R_inf"][1]
    md.obs_fit_status[:] = False
    with pytest.warns(UserWarning, match="No valid observations"):
        md.filter_observations(np.arange(5), resolved=False, sigma=(1, 0))
    md.obs_fit_status[:] = True
    with pytest.raises(ValueError, match="resolved=False"):
        md.filter_observations(np.arange(5), sigma=(1, 0))
    md.obs_x_resolved, md.obs_special_resolved = md.obs_x * 2.0, {"R_inf": md.obs_special["R_inf"] * 2.0}
    md.filter_observations(np.arange(5), sigma=(1, 0))
    np.testing.assert_array_equal(fake_filter[0][0], md.obs_x[:, 1:6] * 2.0)
    assert set(md.obs_special_filt) >= {"R_inf"} and md.obs_special_filt["R_inf"][0] == md.obs_special["R_inf"][0] * 2.0 + 100.0


def test_filt_tables_grow_with_add_observation_and_group_index(fake_filter):
    md = _store()
    md.filter_observations(np.arange(5), resolved=False, sigma=(1, 0))
    md.add_observation([50.0, 0.0], None, None, group_id="b")
    assert md.obs_x_filt.shape == (6, 7) and md.obs_special_filt["x_dop"].shape == (6, 3) and not md.obs_x_filt[5].any()
    assert md.get_group_index("a").tolist() == [0, 1, 2, 3] and md.get_group_index(["b"]).tolist() == [4, 5]
    assert md.get_group_index("a", psi_sort_dims=["T", "p"]).tolist() == [1, 3, 2, 0]
    assert md.get_group_index(["a", "b"], psi_sort_dims=["T"]).tolist() == [1, 3, 2, 0, 4, 5]          # sorted within groups
    md.obs_ignore_flag[3] = True
    assert md.get_group_index("a", exclude_flagged=True).tolist() == [0, 1, 2]


def test_filter_group_forwards_special_kw_as_given(fake_filter):
    md = _store()
    md.filter_group("a", psi_sort_dims=["T"], resolved=False, sigma=(1, 0))        # upstream's default special_kw={}
    assert fake_filter[0][0].shape == (4, 5)
    assert [kw for arr, _, kw in fake_filter[1:] if arr.ndim == 1] == [{}]          # R_inf: no sigma reaches the special filter
    fake_filter.clear()
    md.filter_group("a", resolved=False, special_kw=None, sigma=(1, 0))
    assert [kw for arr, _, kw in fake_filter[1:] if arr.ndim == 1] == [dict(sigma=(1,))]
