"""CPU: the numpy reference of tests/test_gpu_gram.py (tests/gram_util.py) is itself checked -- the tile layout against a direct
statement of it, the L2 restatement against the oracle, the derived error bound against plain float64 numpy."""
import numpy as np
import pytest

import gram_util as gu
from conftest import GOLDEN


@pytest.mark.parametrize("n", [1, 5, 16, 17, 32, 33, 93])
def test_pack_unpack_round_trip(n):
    rng = np.random.default_rng(n)
    P = rng.standard_normal((n, n + 3))
    nc = gu.nchp_of(n)
    assert nc % 2 == 0 and nc * 16 >= n > (nc - 2) * 16
    ppk = gu.pack_tiles(P, n)
    assert ppk.shape == (nc * nc * 256,)
    np.testing.assert_array_equal(np.isnan(ppk), ~gu.lower_tile_mask(n))           # tiles above the diagonal: never packed
    full = gu.unpack_tiles(ppk, n)
    tile_r, tile_c = np.arange(nc * 16)[:, None] // 16, np.arange(nc * 16)[None, :] // 16
    want = np.zeros((nc * 16, nc * 16))
    want[:n, :n] = P[:n, :n]
    want[tile_c > tile_r] = np.nan
    np.testing.assert_array_equal(full, want)
    np.testing.assert_array_equal(gu.pack_tiles(np.nan_to_num(full), nc * 16)[gu.lower_tile_mask(n)], ppk[gu.lower_tile_mask(n)])
    # the documented slot rule, element by element: double2 slot h*64 + i*4 + q = columns q + 8h, q + 8h + 4 of row i
    for tr, tc, i, j in [(0, 0, 0, 0), (nc - 1, 0, 15, 15), (nc - 1, nc - 1, 7, 12), (1, 0, 3, 9), (1, 1, 2, 5)]:
        h, q, e = j // 8, j % 4, (j % 8) // 4
        assert j == q + 8 * h + 4 * e
        v = ppk[(tr * nc + tc) * 256 + 2 * (h * 64 + i * 4 + q) + e]
        r, c = tr * 16 + i, tc * 16 + j
        assert v == (P[r, c] if r < n and c < n else 0.0)


@pytest.mark.parametrize("dop", [None, (1, 4)])
def test_l2_restatement_equals_the_oracle(dop):
    from oracle import drt_oracle as orc
    rng = np.random.default_rng(11)
    n, ns = 29, 6
    pen = [rng.standard_normal((n, n)) for _ in range(3)]
    s = rng.uniform(0.1, 4.0, (3, n))
    rho, dop_rho = rng.uniform(0.5, 2.0, 3), rng.uniform(0.5, 2.0, 3)
    hyp = dict(derivative_weights=[1.5, 0.0, 0.5], l2_lambda_0=142.0, dop_l2_lambda_0=7.0, dop_derivative_weights=[0.25, 1.0, 2.0])
    ref = orc.calculate_qp_l2_matrix_dop(hyp, rho, dop_rho, pen, [v.copy() for v in s], ns,
                                         None if dop is None else (dop[0], dop[0] + dop[1]))
    dfac = [hyp['l2_lambda_0'] * d for d in hyp['derivative_weights']]
    dop_dfac = [hyp['dop_l2_lambda_0'] * d for d in hyp['dop_derivative_weights']]
    got = gu.l2_matrix(pen, s, rho, dfac, ns, dop, dop_rho, dop_dfac)
    # the same products in another association (dfac * rho first): a few roundings per element
    np.testing.assert_allclose(got, ref, rtol=8 * gu.U, atol=0)
    assert np.count_nonzero(got) == n * n
    # and with it P and q: against the plain formulas
    A, w, y = rng.standard_normal((13, n)), rng.uniform(0.5, 2, (2, 13)), rng.standard_normal((2, 13))
    P, q = gu.reference_pq(A, w, y, l1_scalar=0.25, mk=pen, s=np.stack([s, 2 * s]), rho=np.stack([rho, rho]), dfac=dfac, ns=ns,
                           dop=dop, dop_rho=np.stack([dop_rho, dop_rho]), dop_dfac=dop_dfac)
    wa = w[0][:, None] * A
    np.testing.assert_allclose(P[0], wa.T @ wa + ref, rtol=1e-13, atol=1e-13)
    np.testing.assert_allclose(q[0], -wa.T @ (w[0] * y[0]) + 0.25, rtol=1e-13, atol=1e-13)
    assert not np.allclose(P[1], P[0])


def test_exact_fallback_agrees_with_the_extended_reference():
    ext = gu.extended_dtype()
    if ext is None:
        pytest.skip("no extended type on this platform: the fallback IS the reference")
    rng = np.random.default_rng(5)
    n, m, ns = 7, 9, 2
    A, w, y = rng.standard_normal((m, n)), rng.uniform(0.5, 2, (1, m)), rng.standard_normal((1, m))
    kw = dict(mk=[rng.standard_normal((n, n)) for _ in range(3)], s=rng.uniform(0.1, 4, (1, 3, n)), rho=rng.uniform(0.5, 2, (1, 3)),
              dfac=(2.0, 1.0, 0.5), ns=ns, l1_scalar=0.5)
    Pe, qe = gu.reference_pq_exact(A, w, y, n, **kw)
    Px, qx = gu.reference_pq(A, w, y, n, dtype=ext, **kw)
    bp, bq = gu.error_bounds(A, w, y, n, m, **kw)
    assert gu.worst_ratio(Pe, Px, bp) < 0.2 and gu.worst_ratio(qe, qx, bq) < 0.2


def test_float64_numpy_meets_the_derived_bound_on_the_golden_case():
    """the bound of the GPU float test, gamma_(m+8) |WA|'|WA| + 8u |L2| (and its q form), holds for plain float64 numpy on the
    71 x 91 inputs -- whatever order BLAS sums in -- so it is a bound a correct kernel can meet; one element off by a relative 1e-11 exceeds it"""
    ext = gu.extended_dtype()
    c = gu.golden71_case(GOLDEN)
    n, m = c["A"].shape[1], c["A"].shape[0]
    if ext is not None:
        assert np.finfo(ext).nmant >= 63
        Px, qx = gu.reference_pq(n=n, dtype=ext, **c)
    else:
        Px, qx = gu.reference_pq_exact(n=n, **c)
    P, q = gu.reference_pq(n=n, **c)
    bp, bq = gu.error_bounds(n=n, m=m, **c)
    assert bp.shape == (1, n, n) and bq.shape == (1, n) and (bp >= 0).all() and (bq > 0).all()      # (exact zeros: R_inf x inductance)
    rp, rq = gu.worst_ratio(P, Px, bp), gu.worst_ratio(q, qx, bq)
    print(f"float64 numpy / bound: P {rp:.3f}  q {rq:.3f}")
    assert rp <= 1.0 and rq <= 1.0
    # the bound is tight enough to notice a wrong value: on the diagonal (no cancellation) it is gamma_(m+8) = 1.7e-14 of the element at most
    assert np.max(np.diagonal(bp[0]) / np.diagonal(np.asarray(Px[0], dtype=np.float64))) <= gu.gamma(m + 8) * (1 + 1e-8)
    bad = P.copy()
    bad[0, 40, 37] *= 1 + 1e-11
    assert gu.worst_ratio(bad, Px, bp) > 1.0
