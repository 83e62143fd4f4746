"""Device map filter (csrc/map_filter.hip: hipdrt_map_filter) behind mapping.ndx.filter_ndx, hipdrt.filters and
DRTMD.filter_observations, against the reference's own runs in tests/golden/refrun_map_filter.npz
(tools/make_map_filter_golden.py).  Every figure is max |difference| / max |reference| and is asserted at its bound in
tests/map_filter_bounds.json (measured on the GPU against the fixture; bound = the next 1-2-5 step at least 10 x above)."""
import json
import os

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

pytestmark = pytest.mark.gpu

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
    """max |actual - ref| / max |ref| over the entries the reference fills; the NaN patterns must agree"""
    actual, ref = np.asarray(actual), np.asarray(ref)
    assert actual.shape == ref.shape
    np.testing.assert_array_equal(np.isnan(actual), np.isnan(ref))
    return float(np.nanmax(np.abs(actual - ref)) / np.nanmax(np.abs(ref)))


def check(section, label, actual, ref):
    with open(os.path.join(ROOT, "tests", "map_filter_bounds.json")) as f:
        table = json.load(f)[section]
    err = deviation(actual, ref)
    print(f"map_filter {section} {label}: measured {err:.2e} bound {table[label][1]:.1e}")
    assert err <= table[label][1], (label, err, table[label])


@pytest.fixture(scope="module")
def fx():
    return load_fixture()


def test_fixture_lists_the_cases(fx):
    assert list(fx["cases"]) == CASES


@pytest.mark.parametrize("name", CASES)
def test_filter_ndx_matches_the_reference_run(fx, name):
    from hipdrt.mapping.ndx import filter_ndx
    out = filter_ndx(fx[f"{name}_in"].copy(), 0, **case_kw(fx, name))
    check("device", f"{name}:out", out, fx[f"{name}_out"])


@pytest.mark.parametrize("name", [c for c in CASES if "plain" not in c or "adaptive" in c])
def test_weights_and_sigmas_match_the_recorded_intermediates(fx, name):
    from hipdrt import filters
    kw = case_kw(fx, name)
    kw.pop("impute", None)
    res = filters.filter_array(fx[f"{name}_in"], return_info=True, **kw)
    assert (f"{name}_weights" in fx) == ("weights" in res) and (f"{name}_sigmas" in fx) == ("sigmas" in res)
    if "weights" in res:
        check("device", f"{name}:weights", res["weights"], fx[f"{name}_weights"])
    if "sigmas" in res:
        check("device", f"{name}:sigmas", res["sigmas"], fx[f"{name}_sigmas"])


def test_a_call_repeats_itself_bit_for_bit(fx):
    from hipdrt import filters
    runs = [filters.filter_array(fx["s70_adaptive_in"], return_info=True, **case_kw(fx, "s70_adaptive")) for _ in range(2)]
    for key in ("out", "weights", "sigmas"):
        assert runs[0][key].tobytes() == runs[1][key].tobytes(), key


def test_reexported_filters_compose_like_the_reference_chain(fx):
    """hipdrt.filters' device functions, called the way _filter_ndx_sub calls the reference's (adaptive, not iterative)"""
    from hipdrt import filters
    name = "s23_adaptive_plain"
    a, kw = fx[f"{name}_in"], case_kw(fx, name)
    x, w = np.nan_to_num(a), (~np.isnan(a)).astype(float)
    sigmas = filters.get_adaptive_sigmas(x, weights=w, max_sigma=kw["max_sigma"])
    check("device", f"{name}:sigmas", np.stack(sigmas), fx[f"{name}_sigmas"])
    num = filters.adaptive_gaussian_filter(x * w, sigmas=sigmas, max_sigma=kw["max_sigma"])
    den = filters.adaptive_gaussian_filter(w, sigmas=sigmas, max_sigma=kw["max_sigma"])
    out = num / den
    out[np.isnan(a)] = np.nan
    check("device", f"{name}:out", out, fx[f"{name}_out"])
    plain = case_kw(fx, "s23_plain")
    out = filters.masked_filter(x, w, sigma=plain["sigma"])
    out[np.isnan(a)] = np.nan
    check("device", "s23_plain:out", out, fx["s23_plain_out"])


def test_drtmd_filter_observations_end_to_end():
    """8 small EIS observations fitted on the device, then smoothed across psi: obs_x_filt against the numpy statement on obs_x"""
    from hipdrt import synth
    from hipdrt.mapping import DRTMD
    from hipdrt.mapping.ndx import filter_ndx_statement
    freq = np.logspace(5, 0, 31)
    md = DRTMD(np.logspace(-8, 3, 111), psi_dim_names=["T"], warn=False)
    for k in range(8):
        md.add_observation([300.0 - 5 * k], None, (freq, synth.zarc2_spectrum(freq, 40 + k, jitter=True)))
    md.fit_all()
    assert md.obs_fit_status.all()
    md.filter_observations(np.arange(8), psi_sort_dims=["T"], resolved=False, sigma=(1, 0))
    left, right = md.obs_tau_indices[0]
    order = np.arange(8)[::-1]                                   # ascending T
    ref = filter_ndx_statement(md.obs_x[order, left:right], 0, sigma=(1, 0))
    check("device", "drtmd:obs_x_filt", md.obs_x_filt[order, left:right], ref)
    assert not md.obs_x_filt[:, :left].any() and not md.obs_x_filt[:, right:].any()
    for key, val in md.obs_special.items():
        ref = filter_ndx_statement(val[order], 0, sigma=(1,))
        check("device", "drtmd:special", md.obs_special_filt[key][order], ref)
