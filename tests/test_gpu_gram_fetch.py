"""GPU: the two slab fetch forms of the Gram kernel (csrc/gram.hip: FORM, chosen once per workgroup in front of the K loop), through
the test hook hipdrt_debug_gram_l2 only.

A workgroup takes the full form -- unconditional 16-byte loads from per-thread row pointers -- when all 64 columns it stages (its
row tile's, and its column tile's off the diagonal) lie inside n, m is a multiple of the 16-row slab, lda and n are even and the
rows are 16-byte aligned; every other workgroup takes the general form with a bounds test per load.  The shapes below put the two
forms, or workgroups of both kinds, side by side:
  n = 64, lda = 64     one full diagonal workgroup; m = 16, 32, 48: one, two and three slabs (the prefetch chain with its first and
                       last slab); m = 15, 17, 33: the same workgroup in the general form (slab tail)
  n = 128              two diagonal workgroups of opposite turn and one off-diagonal workgroup, all full
  n = 130              the product's kind: full tiles and the folded strip with two data columns (fourteen of a thread row's
                       sixteen strip columns are masked)
  n = 190              tiles (0, 0), (1, 0), (1, 1) full, tile row 2 on the edge: both forms in one launch
Integer operands, NaN-poisoned outputs and assert_array_equal are borrowed from tests/test_gpu_gram.py.  Integers cannot see a
changed summation order; the float test can: the same values through the full form (lda = 130) and through the general form with
8-byte loads (lda = 131) must give the same bits.
"""
import numpy as np
import pytest

import gram_util as gu
from conftest import GOLDEN
from test_gpu_gram import check, ctx, make_case, run  # noqa: F401  (ctx: the module-scoped fixture)

pytestmark = pytest.mark.gpu


def full_form(n, m, lda, ti, tj):
    """the kernel's own rule for the workgroup of tile (ti, tj), for arrays that start 16-byte aligned"""
    return (lda % 2 == 0 and n % 2 == 0 and m >= 16 and m % 16 == 0 and 64 * ti + 64 <= n and 64 * tj + 64 <= n)


def test_the_shapes_hold_the_forms_they_are_meant_for():
    assert all(full_form(64, m, 64, 0, 0) for m in (16, 32, 48))
    assert not any(full_form(64, m, 64, 0, 0) for m in (15, 17, 33))
    assert all(full_form(n, 32, n, ti, tj) for n in (128, 130, 190) for ti, tj in ((0, 0), (1, 0), (1, 1)))
    assert not any(full_form(190, 32, 190, 2, tj) for tj in range(3))
    assert full_form(130, 48, 130, 1, 0) and not full_form(130, 48, 131, 1, 0)


@pytest.mark.parametrize("m", [16, 32, 48, 15, 17, 33])
def test_one_diagonal_workgroup_full_and_general(ctx, m):
    c = make_case(30000 + m, 2, m, 64, ns=2, lda=64)
    for rowp in (True, False):
        check(ctx, c, run(ctx, c, rowp=rowp))


@pytest.mark.parametrize("n,ns", [(128, 0), (130, 2), (190, 2)])
def test_full_workgroups_of_both_kinds_and_edge_tiles(ctx, n, ns):
    c = make_case(31000 + n, 2, 32, n, ns=ns, lda=n)
    for rowp in (True, False):
        check(ctx, c, run(ctx, c, rowp=rowp))


def test_per_spectrum_matrices_in_the_full_form(ctx):
    c = make_case(32000, 3, 32, 130, ns=2, lda=130, a_batched=True)
    for rowp in (True, False):
        check(ctx, c, run(ctx, c, rowp=rowp))


def test_inactive_member_keeps_its_poison(ctx):
    active = np.array([1, 0, 1], dtype=np.int32)
    c = make_case(32100, 3, 32, 128, ns=0, lda=128)
    for rowp in (True, False):
        check(ctx, c, run(ctx, c, rowp=rowp, active=active), active=active)


def test_float_operands_the_forms_agree_bit_for_bit(ctx):
    """Random normal A, w in [0.5, 2], s and rho log-uniform over the ranges of the reference's own 71 x 91 run, the product's
    dfac, float Toeplitz penalties.  lda = 130: every workgroup in the full form; lda = 131: every workgroup in the general form
    with 8-byte loads.  Same bits in P, Ppk and q; and the full form's result within gram_util.error_bounds of the
    extended-precision reference, as test_gpu_gram.py's float test has it."""
    n, ns, m, B = 130, 2, 48, 2
    rng = np.random.default_rng(33000)
    g = gu.golden71_case(GOLDEN)
    lo_s, hi_s = np.log(g["s"].min()), np.log(g["s"].max())
    lo_r, hi_r = np.log(g["rho"].min()), np.log(g["rho"].max())
    vals = rng.standard_normal((m, n))
    first = [rng.standard_normal(6) for _ in range(3)]
    special = []
    for k in range(3):
        sp = np.zeros((n, n))
        sp[np.arange(ns), np.arange(ns)] = 1e-6
        special.append(sp)
    c = dict(w=rng.uniform(0.5, 2.0, (B, m)), y=rng.standard_normal((B, m)), mk=gu.toeplitz_penalty(n, ns, first, special),
             s=np.exp(rng.uniform(lo_s, hi_s, (B, 3, n))), rho=np.exp(rng.uniform(lo_r, hi_r, (B, 3))), dfac=g["dfac"], ns=ns)
    outs = []
    for lda in (130, 131):
        A = np.full((m, lda), 977.0)
        A[:, :n] = vals
        P, Ppk, q = np.full((B, n, n), np.nan), np.full((B, gu.nchp_of(n) ** 2 * 256), np.nan), np.full((B, n), np.nan)
        ctx.debug_gram_l2(A, c["w"], y=c["y"], mk=c["mk"], s=c["s"], rho=c["rho"], dfac=c["dfac"], ns=ns, sym=True, toep=True, toep_maxd=5,
                          spec_zero=True, n=n, P=P, Ppk=Ppk, q=q)
        assert not np.isnan(P).any() and not np.isnan(q).any()
        outs.append((P, Ppk, q))
    for a, b, what in zip(outs[0], outs[1], ("P", "Ppk", "q")):
        np.testing.assert_array_equal(a, b, err_msg=what + ": full form (lda = 130) against general form (lda = 131)")
    ext = gu.extended_dtype()
    if ext is not None:
        Px, qx = gu.reference_pq(vals, n=n, dtype=ext, **c)
    else:
        Px, qx = gu.reference_pq_exact(vals, n=n, **c)
    bp, bq = gu.error_bounds(vals, n=n, m=m, **c)
    P, _, q = outs[0]
    rp, rq = gu.worst_ratio(P, gu.mirror_lower(np.asarray(Px)), bp), gu.worst_ratio(q, qx, bq)
    print(f"gram fetch float: kernel / bound  P {rp:.3f}  q {rq:.3f}")
    assert rp <= 1.0 and rq <= 1.0, (rp, rq)
