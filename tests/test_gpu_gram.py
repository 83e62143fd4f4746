"""GPU: the fit loop's Gram and q kernels (csrc/gram.hip: gram_kernel in its four template forms, qvec_kernel; csrc/hyper.hip:
batch_products_kernel<2, true>) in isolation, through the test hook hipdrt_debug_gram_l2 (include/hipdrt_debug.h), which calls
launch_gram_l2 / launch_qvec exactly as the loop does (csrc/plan_fit.hip: outer_iteration).

The reference is the numpy restatement of tests/gram_util.py (checked on the CPU by tests/test_gram_util.py).  Operands are small
integers (and powers of two, and squares under the roots), so every product and every sum is exact in binary64 whatever its
order: the comparisons are assert_array_equal, and a failure names the element -- hence the 64 x 64 tile and the 16 x 16 packed
tile -- that is wrong.  Output buffers are poisoned with NaN beforehand: what the kernels did not write is still NaN afterwards.
One test runs the product's own floating-point magnitudes against an extended-precision reference and a derived bound.
"""
import os

import numpy as np
import pytest

import gram_util as gu
from conftest import GOLDEN

pytestmark = pytest.mark.gpu

PAD = 977.0          # sentinel in the padding columns of A and of the penalty matrices: a kernel that reads them as data shows it


@pytest.fixture(scope="module")
def ctx():
    from hipdrt import _ffi
    return _ffi.get_context()


def make_case(seed, B, m, n, ns=0, lda=None, ldm=None, a_batched=False, reach=3, coupling=True, symmetric=True, dop=None,
              dfac=(2.0, 0.5, 4.0), use_rho=True, l1_vector=True):
    """integer-valued operands of one hook call.  The DRT block (>= ns) of every penalty matrix is symmetric Toeplitz with first
    rows that are non-zero up to distance `reach` exactly; the special block and (coupling=True) the special x DRT entries are
    random, symmetric or not."""
    rng = np.random.default_rng(seed)
    lda, ldm = lda or n, ldm or n
    A = np.full(((B,) if a_batched else ()) + (m, lda), PAD)
    A[..., :n] = rng.integers(-4, 5, A[..., :n].shape)
    nd = n - ns
    reach = min(reach, max(nd - 1, 0))
    first = [np.concatenate([rng.integers(1, 4, reach + 1) * rng.choice([-1, 1], reach + 1), np.zeros(max(nd - reach - 1, 0))])
             for _ in range(3)]
    special = []
    for k in range(3):
        sp = rng.integers(-3, 4, (n, n)).astype(float)
        if symmetric:
            sp = np.tril(sp) + np.tril(sp, -1).T
        if not coupling:
            sp[ns:, :ns] = 0.0
            sp[:ns, ns:] = 0.0
        special.append(sp)
    mk = gu.toeplitz_penalty(n, ns, first, special, ld=ldm)
    for mat in mk:
        mat[:, n:] = PAD
    c = dict(B=B, m=m, n=n, ns=ns, A=A, w=rng.integers(1, 4, (B, m)).astype(float), y=rng.integers(-3, 4, (B, m)).astype(float),
             l1=rng.integers(-5, 6, n).astype(float) if l1_vector else None, l1_scalar=0.0 if l1_vector else 3.0,
             mk=mk, s=rng.choice([1.0, 4.0, 9.0, 16.0], (B, 3, n)), dfac=tuple(dfac), reach=reach, coupling=coupling, symmetric=symmetric,
             rho=2.0 ** rng.integers(-2, 3, (B, 3)) if use_rho else None, dop=dop, dop_rho=None, dop_dfac=(0.0, 0.0, 0.0))
    if use_rho and B > 1:
        c["rho"][:, 0] = 2.0 ** (np.arange(B) % 5 - 2)                # distinct between neighbours: a member reading another's rho shows
    if dop is not None:
        c["dop_dfac"] = (0.25, 8.0, 1.0)
        if use_rho:
            c["dop_rho"] = 2.0 ** rng.integers(-2, 3, (B, 3))
            c["dop_rho"][:, 1] = 2.0 ** (np.arange(B) % 4 - 1)
    return c


def reference(c):
    if "ref" not in c:
        c["ref"] = gu.reference_pq(c["A"], c["w"], c["y"], c["n"], l1=c["l1"], l1_scalar=c["l1_scalar"], mk=c["mk"], s=c["s"],
                                   rho=c["rho"], dfac=c["dfac"], ns=c["ns"], dop=c["dop"], dop_rho=c["dop_rho"], dop_dfac=c["dop_dfac"])
        assert np.abs(c["ref"][0]).max() < 2.0 ** 50                  # exact integers (or dyadic fractions) all the way
    return c["ref"]


def run(ctx, c, rowp=True, ppk=True, q=True, toep=True, toep_maxd=None, sym=None, spec_zero=None, ldp=None, active=None):
    """one hook call on NaN-poisoned outputs -> (P [B][n][ldp] or None, Ppk [B][nchp^2 * 256] or None, q [B][n] or None)"""
    B, n = c["B"], c["n"]
    P = np.full((B, n, ldp or n), np.nan) if rowp else None
    Ppk = np.full((B, gu.nchp_of(n) ** 2 * 256), np.nan) if ppk else None
    qq = np.full((B, n), np.nan) if q else None
    toep = bool(toep and n - c["ns"] >= 1)
    dop = c["dop"] or (0, 0)
    ctx.debug_gram_l2(c["A"], c["w"], y=c["y"] if q else None, l1=c["l1"], l1_scalar=c["l1_scalar"], mk=c["mk"], s=c["s"], rho=c["rho"],
                      dfac=c["dfac"], ns=c["ns"], sym=c["symmetric"] if sym is None else sym, toep=toep,
                      toep_maxd=(c["reach"] if toep_maxd is None else toep_maxd) if toep else -1,
                      spec_zero=(not c["coupling"]) if spec_zero is None else spec_zero, dop_start=dop[0], dop_size=dop[1],
                      dop_rho=c["dop_rho"], dop_dfac=c["dop_dfac"], active=active, n=n, P=P, Ppk=Ppk, q=qq)
    return P, Ppk, qq


def check(ctx, c, out, active=None, pack_p=True):
    """every output of one call against the reference, bit for bit; inactive members keep the poison"""
    P, Ppk, q = out
    n, B = c["n"], c["B"]
    refP, refq = reference(c)
    act = np.ones(B, dtype=bool) if active is None else np.asarray(active, dtype=bool)
    nc = gu.nchp_of(n)
    for b in range(B):
        tag = f"member {b}"
        if not act[b]:
            for arr in (P, Ppk, q):
                assert arr is None or np.isnan(arr[b]).all(), tag + ": an inactive member was written"
            continue
        if P is not None:
            # complete and symmetric: the lower triangle and its mirror, no poison left inside n x n, nothing outside it
            np.testing.assert_array_equal(P[b][:, :n], gu.mirror_lower(refP[b]), err_msg=tag + " row-major P")
            assert np.isnan(P[b][:, n:]).all(), tag + ": padding columns of P written"
        if Ppk is not None:
            full = gu.unpack_tiles(Ppk[b], n)
            tr, tc = np.arange(nc * 16)[:, None] // 16, np.arange(nc * 16)[None, :] // 16
            assert not np.isnan(full[tc <= tr]).any(), tag + ": a lower tile of Ppk is not fully written"
            # strictly lower tiles and the lower halves of diagonal tiles are P; the upper halves of diagonal tiles are computed
            # from their own (i, j), not mirrored
            np.testing.assert_array_equal(full[:n, :n][(tc <= tr)[:n, :n]], refP[b][(tc <= tr)[:n, :n]], err_msg=tag + " Ppk inside n x n")
            pad = (tc <= tr) & ((np.arange(nc * 16)[:, None] >= n) | (np.arange(nc * 16)[None, :] >= n))
            assert (full[pad] == 0.0).all(), tag + ": padding of Ppk is not exactly zero"
            # raw buffer: written tiles as documented, tiles outside the lower grid keep the poison
            np.testing.assert_array_equal(Ppk[b], gu.pack_tiles(refP[b], n), err_msg=tag + " raw Ppk")
        if q is not None:
            np.testing.assert_array_equal(q[b], refq[b], err_msg=tag + " q")
    if pack_p and P is not None and Ppk is not None and c["symmetric"] and act.all():
        # pack_p_kernel's layout is the one the QP tests validate end to end: the Gram kernel's own packing must be its bits.
        # (pack_p_kernel packs the ceil(n / 16) tile rows that hold data and leaves a pure-padding last tile row of the nchp grid
        # alone; the Gram kernel writes its zeros, checked above)
        packed = ctx.debug_pack_p(np.ascontiguousarray(P[:, :, :n]))
        rows_packed = np.repeat(np.arange(nc * nc) // nc < (n + 15) // 16, 256)
        np.testing.assert_array_equal(~np.isnan(packed), np.tile(gu.lower_tile_mask(n) & rows_packed, (B, 1)), err_msg="tiles pack_p wrote")
        np.testing.assert_array_equal(Ppk[:, rows_packed], packed[:, rows_packed], err_msg="Ppk vs pack_p(P)")


# n: the 16-, 32- and 64-element tile edges, nchp against 4 * nt (n = 129: nt = 3 tiles of 64 = 12 sixteens, nchp = 10; pure-padding
# 16-tiles), the plan's sizes.  m: the slab tail (16) and m not a multiple of 4.  Odd n with lda = n takes the scalar fetch, with
# lda = n + 1 the double2 fetch is still off (n odd) -- the product's case; even n with even lda takes double2.
_SHAPES = [(1, 1, 0), (5, 3, 2), (16, 15, 2), (17, 16, 3), (31, 17, 2), (32, 33, 0), (33, 142, 2), (63, 1, 3), (64, 3, 2), (65, 15, 2),
           (93, 142, 2), (96, 16, 0), (97, 17, 3), (127, 33, 2), (128, 15, 2), (129, 16, 3), (514, 17, 2), (527, 3, 3), (528, 33, 2),
           (529, 15, 2), (1078, 17, 2)]


@pytest.mark.parametrize("n,m,ns", _SHAPES)
def test_shapes_and_leading_dimensions(ctx, n, m, ns):
    ns = min(ns, n)
    B = 2 if n <= 529 else 1
    for pad_a in ((0, 1) if n % 2 else (0, 2)) if n <= 529 else (n % 2,):
        c = make_case(1000 + n + pad_a, B, m, n, ns=ns, lda=n + pad_a, ldm=n + (3 if pad_a else 0), reach=min(5, n))
        check(ctx, c, run(ctx, c, ldp=n + (1 if pad_a else 0)))
    if n <= 129:                                       # the loop's own form: packed tiles only
        check(ctx, c, run(ctx, c, rowp=False))


@pytest.mark.parametrize("m", [1, 3, 15, 16, 17, 33, 142])
def test_every_slab_tail_at_a_tile_edge(ctx, m):
    for n, a_batched in ((65, False), (34, True)):
        c = make_case(2000 + m, 3, m, n, ns=2, a_batched=a_batched, lda=n + n % 2)
        check(ctx, c, run(ctx, c))


@pytest.mark.parametrize("B", [1, 3, 16, 17, 32, 33, 70])
def test_batch_sizes_shared_and_per_spectrum_matrices(ctx, B):
    """q over the 32-spectrum slab of batch_products_kernel (shared A) and through qvec_kernel (per-spectrum A); per-spectrum rho
    must not leak between members"""
    for a_batched in (False, True):
        for n, m, l1_vector in ((33, 15, True), (70, 142, False)):
            if a_batched and B > 33 and n == 70:
                continue
            c = make_case(3000 + B, B, m, n, ns=2, a_batched=a_batched, l1_vector=l1_vector)
            check(ctx, c, run(ctx, c, rowp=(n == 33)), pack_p=B <= 17)


def test_active_mask_keeps_the_poison_of_inactive_members(ctx):
    B = 70
    active = np.ones(B, dtype=np.int32)
    active[:32] = 0                                    # a wholly inactive 32-slab
    active[[33, 40, 41, 63]] = 0                       # a partly inactive one
    active[69] = 0
    for a_batched in (False, True):
        c = make_case(4000 + a_batched, B, 17, 33, ns=2, a_batched=a_batched)
        check(ctx, c, run(ctx, c, active=active), active=active)
        check(ctx, c, run(ctx, c, rowp=False, active=active), active=active)
    dopc = make_case(4002, 5, 9, 40, ns=12, dop=(2, 10))
    act5 = np.array([1, 0, 1, 0, 1], dtype=np.int32)
    check(ctx, dopc, run(ctx, dopc, active=act5), active=act5)


def test_qvec_kernel_on_a_large_shared_matrix_equals_the_batched_path(ctx):
    """m * n >= 2^20 with a shared A: launch_qvec takes qvec_kernel (otherwise reached only with per-spectrum matrices); the
    same columns in two halves (m * n / 2 < 2^20) take batch_products_kernel.  Same bits, and the reference's."""
    m, n, B = 2050, 514, 2
    assert m * n >= 1 << 20 > m * (n // 2)
    c = make_case(5000, B, m, n, ns=2, reach=4, use_rho=False)
    P, _, q = run(ctx, c, ppk=False)
    refP, refq = reference(c)
    np.testing.assert_array_equal(q, refq)
    np.testing.assert_array_equal(P, gu.mirror_lower(refP))
    h = n // 2
    for lo, hi in ((0, h), (h, n)):
        w = hi - lo
        qh = np.full((B, w), np.nan)
        ctx.debug_gram_l2(np.ascontiguousarray(c["A"][:, lo:hi]), c["w"], y=c["y"], l1=c["l1"][lo:hi], P=np.full((B, w, w), np.nan), q=qh)
        np.testing.assert_array_equal(qh, q[:, lo:hi])


# reach of the penalties' first rows: the tile-skip shortcut fires at 64 * (ti - tj) - 63 > toep_maxd, i.e. one tile diagonal out at
# reach 0, two out below 65, three out below 129 -- its boundaries and their neighbours, and the full block
@pytest.mark.parametrize("reach", [0, 1, 2, 63, 64, 65, 66, 128, 129, 10 ** 6])
def test_toeplitz_window_and_tile_shortcut(ctx, reach):
    n = 260                                                            # five tile rows: up to four tile diagonals out
    for ns in (0, 2, 3):
        for coupling in ((False,) if ns == 0 else (True, False)):      # spec_zero = 0 with coupling entries, spec_zero = 1 without
            c = make_case(6000 + ns, 2, 17, n, ns=ns, reach=reach, coupling=coupling, ldm=n + (ns % 2))
            assert c["reach"] == (reach if reach < n else n - ns - 1)
            d = np.arange(n - ns)
            assert all((mat[ns, ns + d] != 0).tolist() == (d <= c["reach"]).tolist() for mat in c["mk"])
            outs = [run(ctx, c, rowp=rowp) for rowp in (True, False)]                    # toep_maxd = reach
            outs.append(run(ctx, c, toep_maxd=-1))                                       # reach not known: every tile adds L2
            outs.append(run(ctx, c, toep=False))                                         # dense reads of the same matrices
            for o in outs:
                check(ctx, c, o, pack_p=False)
            check(ctx, c, outs[0])


def test_special_couplings_far_below_the_diagonal(ctx):
    """spec_zero = 0: entries that couple a special parameter with a DRT coefficient far away (row 500, column 0) are in P although
    the tile lies beyond the penalties' reach; spec_zero = 1 (entries zero): the same tiles are skipped, same bits"""
    n, ns = 514, 2
    for coupling in (True, False):
        c = make_case(7000, 1, 9, n, ns=ns, reach=2, coupling=coupling)
        if coupling:
            for k, mat in enumerate(c["mk"]):
                mat[:n, :n][ns:, :ns] = 0.0
                mat[:n, :n][:ns, ns:] = 0.0
                mat[500, 0] = mat[0, 500] = 3.0 + k
                mat[513, 1] = mat[1, 513] = -2.0
            refP, _ = reference(c)
            gram_only, _ = gu.reference_pq(c["A"], c["w"], None, n)
            assert refP[0, 500, 0] != gram_only[0, 500, 0] and refP[0, 513, 1] != gram_only[0, 513, 1]
        for rowp in (True, False):
            check(ctx, c, run(ctx, c, rowp=rowp))
        check(ctx, c, run(ctx, c, toep_maxd=-1), pack_p=False)


def test_unsymmetric_penalties_are_read_as_given_without_sym(ctx):
    """sym = 0: entry (i, j) of the lower triangle uses M_k[i][j] (the special block and the couplings are not symmetric here);
    sym = 1 with symmetric matrices reads the mirror and gives the symmetric case's bits"""
    for n, ns in ((70, 5), (33, 33), (130, 3)):
        c = make_case(8000 + n, 2, 9, n, ns=ns, symmetric=False)
        assert any(not np.array_equal(mat[:n, :n], mat[:n, :n].T) for mat in c["mk"])
        for toep in (True, False):
            check(ctx, c, run(ctx, c, toep=toep))
        cs = make_case(8000 + n, 2, 9, n, ns=ns, symmetric=True)
        a = run(ctx, cs, sym=True)
        b_ = run(ctx, cs, sym=False)
        check(ctx, cs, a)
        for x, y in zip(a, b_):
            np.testing.assert_array_equal(x, y)


def test_an_order_switched_off_and_no_rho(ctx):
    for dfac in ((2.0, 0.0, 4.0), (0.0, 0.0, 1.0), (0.0, 0.0, 0.0)):
        for use_rho in (True, False):
            c = make_case(9000, 2, 9, 70, ns=2, dfac=dfac, use_rho=use_rho)
            for mat, f in zip(c["mk"], dfac):
                if f == 0.0:
                    mat[:] = np.nan                     # an order that is switched off is not read at all (0 * NaN would show)
            check(ctx, c, run(ctx, c))
            check(ctx, c, run(ctx, c, toep=False, rowp=False))


def test_explicit_l2_form_and_no_l2(ctx):
    rng = np.random.default_rng(12)
    B, m, n = 3, 17, 67
    c = make_case(9500, B, m, n, lda=n + 1)
    for l2 in (None, rng.integers(-5, 6, (n, n + 2)).astype(float), rng.integers(-5, 6, (B, n, n)).astype(float)):
        if l2 is not None:
            l2[..., :n] = np.tril(l2[..., :n]) + np.swapaxes(np.tril(l2[..., :n], -1), -1, -2)
        P, Ppk, q = np.full((B, n, n), np.nan), np.full((B, gu.nchp_of(n) ** 2 * 256), np.nan), np.full((B, n), np.nan)
        ctx.debug_gram_l2(c["A"], c["w"], y=c["y"], l1_scalar=2.0, l2=l2, n=n, P=P, Ppk=Ppk, q=q)
        refP, refq = gu.reference_pq(c["A"], c["w"], c["y"], n, l1_scalar=2.0, l2=l2)
        np.testing.assert_array_equal(P, refP)
        np.testing.assert_array_equal(q, refq)
        for b in range(B):
            np.testing.assert_array_equal(Ppk[b], gu.pack_tiles(refP[b], n))


@pytest.mark.parametrize("rowp", [True, False])
def test_dop_block_straddling_a_tile_boundary(ctx, rowp):
    """ns = 2 + 70 with the x_dop block [2, 72) across the first 64-tile boundary: dop_dfac * dop_rho (distinct per spectrum) inside
    the block only, dfac * rho where both indices are DRT coefficients only, special diagonals and every mixed entry unscaled"""
    n, ns, dop = 150, 72, (2, 70)
    for use_rho in (True, False):
        c = make_case(10000, 3, 17, n, ns=ns, dop=dop, use_rho=use_rho, reach=70)
        refP, _ = reference(c)
        plain = dict(c, dop=None)
        plain.pop("ref")
        assert not np.array_equal(reference(plain)[0][:, 2:72, 2:72], refP[:, 2:72, 2:72])     # the block's scale matters here
        np.testing.assert_array_equal(reference(plain)[0][:, :2, :], refP[:, :2, :])
        for toep in (True, False):
            check(ctx, c, run(ctx, c, rowp=rowp, toep=toep))
    edge = make_case(10001, 2, 5, 80, ns=64, dop=(0, 64))                                       # the block IS the first tile
    check(ctx, edge, run(ctx, edge, rowp=rowp))


def test_hook_refuses_what_could_run_out_of_bounds(ctx):
    from hipdrt import _ffi
    c = make_case(11000, 1, 5, 20, ns=4)
    n = 20
    P = np.full((1, n, n), np.nan)
    base = dict(y=c["y"], mk=c["mk"], s=c["s"], rho=c["rho"], dfac=c["dfac"], ns=4, P=P, q=np.full((1, n), np.nan))
    for bad, what in ((dict(ns=21), "ns"), (dict(ns=-1), "ns"), (dict(toep=True, toep_maxd=20), "toep_maxd"),
                      (dict(toep=True, ns=20), "Toeplitz"), (dict(dop_start=2, dop_size=3, dop_rho=c["rho"]), "x_dop"),
                      (dict(dop_start=-1, dop_size=2, dop_rho=c["rho"]), "x_dop"), (dict(dop_start=0, dop_size=2), "dop_rho"),
                      (dict(P=None), "P / Ppk"), (dict(y=c["y"], q=None), "q")):
        with pytest.raises(_ffi.HipDrtError, match=what):
            ctx.debug_gram_l2(c["A"], c["w"], **dict(base, **bad))
    with pytest.raises(_ffi.HipDrtError, match="lda"):
        ctx.debug_gram_l2(c["A"], c["w"], n=21, P=np.full((1, 21, 21), np.nan))
    assert np.isnan(P).all()


def _float_cases():
    """the product's own magnitudes: the reference's 71 x 91 run (matrices from the fixture) and one member of the 256 x 512
    batch (its weights, s vectors and rho from the fixture; response and penalty matrices as the product builds them for that grid)"""
    from hipdrt import _ffi
    from hipdrt.models import DRT
    small = gu.golden71_case(GOLDEN)
    small.update(sym=False, toep=False, toep_maxd=-1)
    yield "golden71x91", small
    g = np.load(os.path.join(GOLDEN, "refrun_c3_member1.npz"), allow_pickle=False)
    drt = DRT(fixed_basis_tau=g["basis_tau"])
    plan = drt._get_plan(g["freq"], _ffi.default_fit_opts(), 1)
    mk = [plan.get(f"m{k}") for k in range(3)]
    ns, n = plan.ns, plan.n
    d = np.arange(n - ns)
    reach = max(int(np.flatnonzero(mat[ns, ns:]).max()) for mat in mk)
    assert all(np.array_equal(mat[ns:, ns:], mat[ns, ns:][np.abs(d[:, None] - d[None, :])]) for mat in mk)      # Toeplitz, bitwise
    y = np.concatenate([g["z"].real, g["z"].imag]) / float(g["coefficient_scale"])
    yield "c3_member1", dict(A=plan.get("rm"), w=np.array(g["weights"])[None], y=y[None], mk=mk, s=np.array(g["s_vectors"])[None],
                             rho=np.array(g["rho_vector"])[None], dfac=tuple(142.0 * np.array([1.5, 1.0, 0.5])), ns=ns,
                             sym=True, toep=True, toep_maxd=reach)


def test_float_magnitudes_against_extended_precision(ctx):
    """Floating point, the product's magnitudes.  Reference: np.longdouble (64-bit significand, asserted) -- or exact rational
    sums where there is none.  Bound, derived and not measured: per element
        |P - P_ref| <= gamma_(m+8) (|WA|'|WA|)_ij + 8u |L2|_ij ,   |q - q_ref| <= gamma_(m+8) (|WA|'|Wy|)_i + 8u |l1_i|
    (gamma_k = k u / (1 - k u), u = 2^-53): w*A rounds once per factor, the m products are summed in some order with or without
    fused multiply-adds, an L2 term is two square roots and three products, three terms are added and the result is added to
    the sum.  Plain float64 numpy is checked against the same bound first.  Packed tiles against the row-major copy: the same
    bits for i >= j; the upper halves of diagonal 16-tiles within the bound ((sqrt(s_i) m) sqrt(s_j) does not commute in
    rounding).  Measured worst ratios to the bound are printed (DESIGN.md section 2 records them)."""
    ext = gu.extended_dtype()
    for name, c in _float_cases():
        flags = {k: c.pop(k) for k in ("sym", "toep", "toep_maxd")}
        m, n = c["A"].shape
        if ext is not None:
            assert np.finfo(ext).nmant >= 63
            Px, qx = gu.reference_pq(n=n, dtype=ext, **c)
        else:
            Px, qx = gu.reference_pq_exact(n=n, **c)
        bp, bq = gu.error_bounds(n=n, m=m, **c)
        Pn, qn = gu.reference_pq(n=n, **c)
        rn = (gu.worst_ratio(Pn, Px, bp), gu.worst_ratio(qn, qx, bq))
        assert max(rn) <= 1.0, (name, rn)
        A = np.zeros((m, n + n % 2))                                   # the product's leading dimension: round_up(n, 2)
        A[:, :n] = c["A"]
        P, Ppk, q = np.full((1, n, n), np.nan), np.full((1, gu.nchp_of(n) ** 2 * 256), np.nan), np.full((1, n), np.nan)
        ctx.debug_gram_l2(A, c["w"], y=c["y"], mk=c["mk"], s=c["s"], rho=c["rho"], dfac=c["dfac"], ns=c["ns"], spec_zero=True, n=n,
                          P=P, Ppk=Ppk, q=q, **flags)
        rp, rq = gu.worst_ratio(P, gu.mirror_lower(np.asarray(Px)), bp), gu.worst_ratio(q, qx, bq)
        full = gu.unpack_tiles(Ppk[0], n)[:n, :n]
        lower = np.tril(np.ones((n, n), dtype=bool))
        diag_upper = ~lower & (np.arange(n)[:, None] // 16 == np.arange(n)[None, :] // 16)
        ru = gu.worst_ratio(full[diag_upper], np.asarray(Px[0])[diag_upper], bp[0][diag_upper])
        print(f"gram float {name}: kernel / bound  P {rp:.3f}  q {rq:.3f}  Ppk upper halves of diagonal tiles {ru:.3f}"
              f"   (numpy float64: P {rn[0]:.3f}  q {rn[1]:.3f})")
        assert rp <= 1.0 and rq <= 1.0 and ru <= 1.0, (name, rp, rq, ru)
        np.testing.assert_array_equal(full[lower], P[0][lower])
        assert not np.isnan(P).any() and not np.isnan(q).any()
