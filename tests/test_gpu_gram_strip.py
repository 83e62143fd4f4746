"""GPU: the Gram kernel's tile decomposition at the sizes where the last 16-row strip rides on the diagonal tiles (csrc/gram.hip:
nt16 = ceil(n / 16), nt16 % 4 == 1 and nt16 > 1 -- n = 65...80, 129...144, 513...528) and at their neighbours that keep a 64-tile
row for it, through the test hook hipdrt_debug_gram_l2 only.

Everything is borrowed from tests/test_gpu_gram.py: integer operands (every product and sum exact in binary64), NaN-poisoned
outputs, assert_array_equal against the numpy restatement -- a failure names the element, hence the sub-tile and its owner.
What the shapes exercise:
  n = 65 / 80    one diagonal workgroup with four strip sub-tiles and the corner (15 sub-tiles on four wavefronts), one data row
                 resp. a full strip; the packed layout's pure-padding tile row 5 (zeros by plain stores)
  n = 130 / 144  two diagonal workgroups (turns 0 and 2: the short shares alternate), one off-diagonal workgroup, strip sub-tiles
                 (8, 0...7) split between the two diagonal workgroups; n = 130: padding tile row 9
  n = 81, 145    nt16 = 6, 10: no fold, a partial last tile row as before
  n = 514        the product's shape (36 workgroups, padding tile row 33)
"""
import numpy as np
import pytest

from test_gpu_gram import check, ctx, make_case, reference, run  # noqa: F401  (ctx: the module-scoped fixture)

pytestmark = pytest.mark.gpu


def folds(n):
    nt16 = (n + 15) // 16
    return nt16 % 4 == 1 and nt16 > 1


def test_the_shapes_are_on_the_sides_of_the_fold_they_are_meant_for():
    assert [n for n in (64, 65, 80, 81, 128, 129, 130, 144, 145, 514, 527, 528, 529, 1078) if folds(n)] == [65, 80, 129, 130, 144, 514, 527, 528]


@pytest.mark.parametrize("n", [65, 80, 81])
def test_one_diagonal_workgroup_with_strip_and_corner(ctx, n):
    for lda in sorted({n, n + n % 2, n + 1}):          # scalar fetch (odd n or odd lda) and, for even n, the double2 fetch
        c = make_case(20000 + n + lda, 2, 17, n, ns=2, lda=lda)
        for rowp in (True, False):
            check(ctx, c, run(ctx, c, rowp=rowp))


@pytest.mark.parametrize("m", [3, 16, 33])
@pytest.mark.parametrize("n,ns", [(130, 2), (144, 0), (145, 2)])
def test_two_diagonal_workgroups_share_the_strip(ctx, n, ns, m):
    c = make_case(21000 + n + m, 2, m, n, ns=ns, lda=n + n % 2)
    for rowp in (True, False):
        check(ctx, c, run(ctx, c, rowp=rowp))


@pytest.mark.parametrize("lda", [130, 131])
@pytest.mark.parametrize("a_batched", [False, True])
def test_options_operand_forms(ctx, lda, a_batched):
    c = make_case(22000 + lda, 3, 17, 130, ns=2, lda=lda, a_batched=a_batched)
    for rowp in (True, False):
        check(ctx, c, run(ctx, c, rowp=rowp))


def test_options_inactive_member_keeps_its_poison(ctx):
    active = np.array([1, 0, 1], dtype=np.int32)
    c = make_case(22100, 3, 17, 130, ns=2)
    for rowp in (True, False):
        check(ctx, c, run(ctx, c, rowp=rowp, active=active), active=active)


def test_options_unsymmetric_special_entries_without_sym(ctx):
    c = make_case(22200, 2, 9, 130, ns=2, symmetric=False)
    assert any(not np.array_equal(mat[:130, :130], mat[:130, :130].T) for mat in c["mk"])
    assert any(mat[128, 0] != mat[0, 128] for mat in c["mk"])          # in strip sub-tile (8, 0)
    for toep in (True, False):
        for rowp in (True, False):
            check(ctx, c, run(ctx, c, toep=toep, rowp=rowp))


@pytest.mark.parametrize("dfac", [(2.0, 0.0, 4.0), (0.0, 0.5, 0.0)])
def test_options_an_order_switched_off(ctx, dfac):
    c = make_case(22300, 2, 9, 130, ns=2, dfac=dfac)
    for mat, f in zip(c["mk"], dfac):
        if f == 0.0:
            mat[:] = np.nan                                             # not read at all (0 * NaN would show)
    for rowp in (True, False):
        check(ctx, c, run(ctx, c, rowp=rowp))


def test_options_no_rho(ctx):
    c = make_case(22400, 2, 9, 130, ns=2, use_rho=False)
    assert c["rho"] is None
    for rowp in (True, False):
        check(ctx, c, run(ctx, c, rowp=rowp))


# n = 130, ns = 2.  The reach shortcut fires where the smallest difference of a part exceeds toep_maxd: 1 for the off-diagonal
# tile (1, 0) and for the strip part of diagonal tile 1 (rows 128..., columns 64...127), 65 for the strip part of diagonal tile 0
# (columns 0...63) -- so reach 0 | 1 and 64 | 65 are its thresholds; 15, 16, 17 / 63 / 79, 80 the edges of the strip's window of 79
# differences (1...79 and 65...143, cut at the block's size) and of the corner's 31 in the tile's window; 127 the whole block
@pytest.mark.parametrize("reach", [0, 1, 15, 16, 17, 63, 64, 65, 79, 80, 127])
def test_toeplitz_reach_at_the_strip_windows_edges(ctx, reach):
    n, ns = 130, 2
    c = make_case(23000 + reach, 2, 9, n, ns=ns, reach=reach, coupling=False)
    assert c["reach"] == reach
    d = np.arange(n - ns)
    assert all((mat[ns, ns + d] != 0).tolist() == (d <= reach).tolist() for mat in c["mk"])
    for rowp in (True, False):
        check(ctx, c, run(ctx, c, rowp=rowp, toep_maxd=reach, spec_zero=True))
    check(ctx, c, run(ctx, c, toep_maxd=-1, spec_zero=True), pack_p=False)     # reach not known: every part adds L2, same bits


def test_toeplitz_reach_with_coupling_entries_in_the_strip(ctx):
    """spec_zero = 0: strip sub-tile (8, 0) holds the special columns, read through the dense matrices whatever the reach"""
    n, ns = 130, 2
    for reach in (1, 16):
        c = make_case(23500 + reach, 2, 9, n, ns=ns, reach=reach, coupling=True)
        assert any(mat[128, 0] != 0 or mat[129, 1] != 0 for mat in c["mk"])
        for rowp in (True, False):
            check(ctx, c, run(ctx, c, rowp=rowp, toep_maxd=reach, spec_zero=False))


@pytest.mark.parametrize("rowp", [True, False])
@pytest.mark.parametrize("dop,ns", [((120, 8), 128), ((126, 4), 130)])
def test_dop_block_at_the_strip_boundary(ctx, dop, ns, rowp):
    """the x_dop block lies inside the special block [0, ns): rows 120...127 end with the tile (none in the strip), rows 126...129
    cross row 128 -- dop_dfac * dop_rho inside the block only, whichever sub-tile and wavefront an element belongs to"""
    n = 130
    for use_rho in (True, False):
        c = make_case(24000 + dop[0], 3, 17, n, ns=ns, dop=dop, use_rho=use_rho)
        refP, _ = reference(c)
        plain = dict(c, dop=None)
        plain.pop("ref")
        lo, hi = dop[0], dop[0] + dop[1]
        assert not np.array_equal(reference(plain)[0][:, lo:hi, lo:hi], refP[:, lo:hi, lo:hi])
        check(ctx, c, run(ctx, c, rowp=rowp))


def test_the_products_shape_packed_tiles_only(ctx):
    c = make_case(25000, 2, 17, 514, ns=2, lda=514)
    check(ctx, c, run(ctx, c, rowp=False))
