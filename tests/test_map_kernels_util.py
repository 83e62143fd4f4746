"""CPU: the references of tests/test_gpu_map_kernels.py pinned without a GPU (tests/map_kernels_util.py).

 - hipdrt.filters.ndfilters equals scipy.ndimage bit for bit at every filter and rank-filter case of the GPU test, the arrays
   shorter than their window and the 1-D ones included;
 - the masks leave no NaN in a masked output, except the one fully masked row;
 - the edge table says what the launcher does: 65536 bytes of LDS at the listed radius, more at the next;
 - a numpy emulation of the device's fixed summation order stays inside both derived reduction bounds at every n;
 - the statement of the probability rows treats the adversarial inputs as the GPU test assumes."""
import numpy as np
import pytest

import map_badness_util
import map_kernels_util as util
from hipdrt.filters import ndfilters


def same(a, b):
    return np.array_equal(a, b, equal_nan=True)


def scipy_masked(ndi, x, mask, sigma):
    with np.errstate(invalid="ignore", divide="ignore"):
        return ndi.gaussian_filter(x * mask, sigma, mode="reflect") / ndi.gaussian_filter(mask, sigma, mode="reflect")


def filter_cases():
    for shape in util.TILE_SHAPES:
        for sigma in util.TILE_SIGMAS:
            yield shape, sigma, None
    yield util.MULTI_PERIOD + (None,)
    for shape, sigma, masked, *_ in util.EDGE_CASES:
        yield shape, sigma, masked


def test_ndfilters_equals_scipy_at_every_filter_case():
    ndi = pytest.importorskip("scipy.ndimage")
    count = masked_with_zeros = 0
    for shape, sigma, masked in filter_cases():
        a = util.filter_input(shape)
        if masked is not True:
            assert same(util.plain_reference(a, sigma), ndi.gaussian_filter(a, sigma, mode="reflect")), (shape, sigma)
        if masked is not False:
            mask = util.filter_mask(shape, sigma)
            ref = util.masked_reference(a, mask, sigma)
            assert same(ref, scipy_masked(ndi, a, mask, sigma)), (shape, sigma)
            assert np.isnan(ref).sum() == 0, (shape, sigma)
            # (a window that is one entry, such as a single row filtered along axis 0, cannot lose that entry: no zeros there)
            zeros = (mask == 0).mean()
            assert zeros < 0.25 and (zeros > 0.02 or masked is None), (shape, sigma, zeros)
            masked_with_zeros += zeros > 0
        count += 1
    assert count == 9 * 3 + 1 + 12 and masked_with_zeros >= 20


def test_fully_masked_row_is_the_only_nan_row():
    ndi = pytest.importorskip("scipy.ndimage")
    x, mask, sigma = util.masked_row_case()
    ref = util.masked_reference(x, mask, sigma)
    assert np.isnan(ref[4]).all() and np.isnan(ref).sum() == ref.shape[1]
    assert same(ref, scipy_masked(ndi, x, mask, sigma))


def test_edge_table_states_the_launchers_lds():
    for shape, sigma, masked, axis, radius, form in util.EDGE_CASES:
        s = util.sigma_seq(sigma, len(shape))[-1 if axis == 1 else 0]
        assert ndfilters.kernel_radius(s) == radius
        assert shape[axis if len(shape) == 2 else 0] < radius                  # the reflection wraps more than once
        need = util.lds_bytes(axis, radius, masked)
        assert (need == util.LDS_BUDGET) if form == "lds" else (need > util.LDS_BUDGET), (shape, sigma, need)
        tabs = util.full_tables(sigma, len(shape))
        assert [None if t is None else len(t) // 2 for t in tabs] == ([radius, None] if axis == 0 else [None, radius])
    assert util.lds_bytes(0, 6, True) <= util.LDS_BUDGET                        # the tile cases run the LDS form
    # the adaptive cases: one operand keeps its window in LDS up to radius 48
    assert util.lds_bytes(0, ndfilters.kernel_radius(6.0), False) <= util.LDS_BUDGET < util.lds_bytes(0, ndfilters.kernel_radius(13.0), False)


@pytest.mark.parametrize("name", util.ADAPTIVE_CASES)
def test_adaptive_case_spans_its_nodes(name):
    a, sigmas, max_sigma = util.adaptive_case(name)
    assert sigmas[0].min() == 0.1 and sigmas[0].max() == max_sigma[0]
    nodes = ndfilters.sigma_nodes(0.1, max_sigma[0])[0]
    assert len(nodes) <= 16 and ndfilters.kernel_radius(nodes[-1]) == int(4 * max_sigma[0] + 0.5)
    out = ndfilters.adaptive_gaussian_filter(a, sigmas=[s.copy() for s in sigmas], max_sigma=max_sigma)
    assert np.isfinite(out).all()


@pytest.mark.parametrize("shape", util.RANK_SHAPES)
def test_ndfilters_rank_filters_equal_scipy(shape):
    ndi = pytest.importorskip("scipy.ndimage")
    a = util.rank_input(shape)
    assert np.isnan(a).sum() == (0 if a.size == 1 else max(1, round(0.03 * a.size)))
    for size in util.RANK_WINDOWS:
        for kind in util.RANK_KINDS:
            if kind == "median":
                ref = ndi.median_filter(a, size=size, mode="reflect")
            elif kind == "iqr":
                ref = ndi.percentile_filter(a, 75, size=size, mode="reflect") - ndi.percentile_filter(a, 25, size=size, mode="reflect")
            else:
                ref = ndi.percentile_filter(a, int(kind[1:]), size=size, mode="reflect")
            got = util.rank_reference(a, kind, size)
            assert map_badness_util.rank_rule_equal(a, kind, size, got, ref), (shape, size, kind)


def test_reduce_geometry():
    assert util.reduce_geometry(1) == (1, 1, 1, 18) and util.reduce_geometry(257) == (2, 1, 1, 18)
    assert util.reduce_geometry(65537) == (257, 1, 2, 19)                       # reduce_final's loop repeats
    assert util.reduce_geometry(262144) == (1024, 1, 4, 21) and util.reduce_geometry(262145) == (1024, 2, 4, 22)
    assert util.reduce_geometry(600001) == (1024, 3, 4, 23)


@pytest.mark.parametrize("n", util.REDUCE_N)
def test_emulated_device_order_stays_inside_the_derived_bounds(n):
    x = util.reduce_data(n)
    assert (x > 0).any() or n < 3
    assert n < 3 or (np.log10(np.abs(x).max() / np.abs(x).min()) > 3 and (x < 0).any())
    mean = util.emulate_mean(x)
    err, bound = abs(mean - util.mean_exact(x)), util.mean_bound(x)
    assert err <= bound, (n, err, bound)
    std = util.emulate_std(x, mean)
    exact = util.std_exact(x, mean)
    serr, sbound = abs(std - exact), util.std_bound(x, exact)
    assert serr <= sbound, (n, serr, sbound)
    print(f"reduce n {n}: mean |error| / bound {err / bound if bound else 0:.3f}, std {serr / sbound if sbound else 0:.3f}")
    if n <= 257:                                                                # the emulation is the plain sum where it must be
        assert util.emulate_sum(np.ones(n)) == n
    const = np.full(256, 0.1)
    assert util.emulate_mean(const) == 0.1 and util.emulate_std(const, 0.1) == 0.0


def test_probability_statement_on_the_adversarial_inputs():
    rng = np.random.default_rng(3)
    fxx, f, vxx, vf = util.integer_rows(rng, 3, 40)
    ext = np.array([[-1, -1], [30, 10], [5, 35]], dtype=np.int32)               # none, crossed, ordinary
    vf[2, 7] = np.nan                                                           # a NaN variance: the clamp leaves the row alone
    f[0], fxx[0] = np.nan, np.nan                                               # a NaN row has no peaks
    ref = util.prob_reference(f, fxx, vf, vxx, ext, 0, 1e-3, 5e-3, True)
    assert same(ref["f_var"][2], vf[2]) and same(ref["f_var"][0], vf[0])
    assert (ref["fxx_var"][2, :5] >= vxx[2, 5]).all() and (ref["fxx_var"][2, 35:] >= vxx[2, 35]).all()
    assert (ref["f_var"][1, :30] >= vf[1, 30]).all() and (ref["f_var"][1, 10:] >= ref["f_var"][1, 10]).all()
    assert np.isnan(ref["pk"][0]).all() and np.isnan(ref["curv"][0]).all()
    assert np.isnan(ref["curv"][2, 7]) and np.isfinite(ref["curv"][2, :7]).all()
    assert (ref["pk"][1] != 0).any()
    unsigned = util.prob_reference(f, fxx, vf, vxx, ext, 0, 1e-3, 5e-3, False)["pk"]
    assert (unsigned[0] == 0).all() and (unsigned[1:][np.isfinite(unsigned[1:])] >= 0).all()
    assert util.ext_rows(rng, 3, 40)[0].tolist() == [-1, -1] and util.ext_rows(rng, 1, 1).tolist() == [[0, 0]]
