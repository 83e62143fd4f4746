"""CPU: the reference of the chain-alone tests of tests/test_gpu_dop_posterior.py (tests/dop_posterior_util.py) is itself checked, on
the very cases the GPU tests use -- the refinement converged; a float64 numpy restatement of the device's route (scale entry by
entry, Cholesky, solve: both posterior_util's restatement of the kernel's blocked algorithm and plain LAPACK) stays inside the bound
on every case; the exact packed image of the scaled P is the packed image of fl(fl(P_ij s_i) s_j), with the padding of an unscaled
image; and defects a scaling kernel can have leave the bound."""
import numpy as np
import pytest

import dop_posterior_util as du
import gram_util as gu
import posterior_util as pu

pytestmark = pytest.mark.skipif(gu.extended_dtype() is None, reason="no extended type on this platform")


@pytest.mark.parametrize("shape", du.SHAPES, ids=lambda s: f"n{s[0]}")
def test_refinement_converged_and_float64_routes_stay_inside_the_bound(shape):
    n, ds, dz = shape
    worst = 0.0
    for neval in du.NEVALS:
        m, rows, refs = du.get_case(n, ds, dz, neval)
        R = pu.full_rows(rows, n, ds)
        for b in range(du.B):
            ref = refs[b]
            assert ref["corrections"][-1] <= ref["tol"] and ref["iters"] <= 12, (shape, neval, b, ref["corrections"])
            M = du.scaled_f64(m["P"][b], m["s"][b])
            for route in (pu.restate(M, rows, ds)["var"], pu.lapack_route(M, R)["var"]):
                assert np.all(route >= 0.0)
                worst = max(worst, du.var_ratio(route, ref, n, m["kappa"][b]))
    kap = du.get_matrices(n, ds, dz)["kappa"]
    print(f"n {n}: kappa_2(SPS) {kap.min():.3g} .. {kap.max():.3g}, bound {du.bound(n, kap.max()):.2e}, "
          f"worst float64 deviation / bound {worst:.2e}")
    assert worst <= 1.0, (shape, worst)


def test_scales_span_four_decades_and_differ_between_members():
    for n, ds, dz in du.SHAPES:
        dsv = du.get_matrices(n, ds, dz)["dsv"]
        assert dsv.shape == (du.B, dz) and np.all(dsv > 0)
        assert not np.array_equal(dsv[0], dsv[1]) and not np.array_equal(dsv[1], dsv[2])
    dsv = du.get_matrices(150, 5, 50)["dsv"]
    assert dsv.min() < 5e-2 and dsv.max() > 2e1, (dsv.min(), dsv.max())


@pytest.mark.parametrize("shape", du.SHAPES, ids=lambda s: f"n{s[0]}")
def test_packed_image_of_the_scaled_p(shape):
    n, ds, dz = shape
    m = du.get_matrices(n, ds, dz)
    P, s = m["P"][1], m["s"][1]
    img = du.scaled_image(P, s)
    plain = gu.pack_tiles(gu.mirror_lower(P), n, fill=0.0)
    full, full0 = gu.unpack_tiles(img, n, fill=0.0), gu.unpack_tiles(plain, n, fill=0.0)
    nt16 = gu.nchp_of(n) * 16
    i, j = np.meshgrid(np.arange(nt16), np.arange(nt16), indexing="ij")
    lower = (j // 16) <= (i // 16)
    inside = lower & (i < n) & (j < n)
    # entry (i, j) of a lower tile: P_ij times s_i, rounded, times s_j, rounded
    se = np.ones(nt16)
    se[:n] = s
    np.testing.assert_array_equal(full[inside], ((full0 * se[:, None]) * se[None, :])[inside])
    # the padding and the tiles above the diagonal are those of the unscaled image; so is every entry outside the DOP rows and columns
    np.testing.assert_array_equal(full[~inside], full0[~inside])
    dop = np.zeros(nt16, dtype=bool)
    dop[ds:ds + dz] = True
    untouched = ~(dop[:, None] | dop[None, :])
    np.testing.assert_array_equal(full[untouched], full0[untouched])
    # the tiles that hold a changed entry are the tiles whose row range or column range meets the block, and no other
    changed = (img != plain).reshape(-1, 256).any(axis=1)
    t0, t1 = ds // 16, (ds + dz - 1) // 16
    nc = gu.nchp_of(n)
    for t in np.nonzero(changed)[0]:
        tr, tc = divmod(int(t), nc)
        assert tc <= tr and (t0 <= tr <= t1 or t0 <= tc <= t1), (tr, tc)
    # dsv = 1 is the identity, bit for bit
    np.testing.assert_array_equal(du.scaled_image(P, np.ones(n)), plain)


@pytest.mark.parametrize("mutant", ["one_sided", "wrong_member", "block_shifted", "dsv_not_inverted"])
def test_defects_of_a_scaling_leave_the_bound(mutant):
    n, ds, dz = 70, 5, 50
    m, rows, refs = du.get_case(n, ds, dz, 17)
    P, s = m["P"][0], m["s"][0]
    if mutant == "one_sided":
        M = gu.mirror_lower(np.tril(P * s[:, None]))
    elif mutant == "wrong_member":
        M = du.scaled_f64(P, m["s"][1])
    elif mutant == "block_shifted":
        M = du.scaled_f64(P, du.scale_vector(n, ds + 1, m["dsv"][0]))
    else:
        M = du.scaled_f64(P, du.scale_vector(n, ds, 1.0 / m["dsv"][0]))
    try:
        var = pu.lapack_route(M, pu.full_rows(rows, n, ds))["var"]
    except np.linalg.LinAlgError:
        return                                          # (not even positive definite: the device reports status -1)
    r = du.var_ratio(var, refs[0], n, m["kappa"][0])
    assert r > 1.0, (mutant, r)
