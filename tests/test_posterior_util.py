"""CPU: the reference of tests/test_gpu_posterior.py (tests/posterior_util.py) is itself checked, on the very cases the GPU tests
use -- the refinement converged on every case; the bound holds from above for two float64 routes that sum in different orders (the
numpy restatement of the kernel's algorithm and plain LAPACK), and its constant is 8 times the worst ratio the restatement shows,
rounded up to a power of two; from below, every listed mutant of the restatement leaves the bound on at least one case; the exact
statements (packed image, padding) hold for the restatement."""
import numpy as np
import pytest

import gram_util as gu
import posterior_util as pu

pytestmark = pytest.mark.skipif(gu.extended_dtype() is None, reason="no extended type on this platform")

TABLE = pu.case_table()
GROUPS = sorted({g for g, _ in TABLE.values()})


@pytest.fixture(scope="module")
def measured():
    """name -> dict(restate, lapack[, restate_cov, lapack_cov]): ratios in units of (n + 16) u kappa, over the whole table"""
    out = {}
    for name, (group, _) in TABLE.items():
        cov = group == "i"
        c, ref = pu.get_case(name, cov)
        R = pu.full_rows(c["rows"], c["n"], c["off"])
        rs, lp = pu.restate(c["P"], c["rows"], c["off"], want_cov=cov), pu.lapack_route(c["P"], R, cov)
        m = dict(restate=pu.var_ratio(rs["var"], ref, c["n"], c["kappa"]), lapack=pu.var_ratio(lp["var"], ref, c["n"], c["kappa"]))
        if cov:
            m["restate_cov"] = pu.cov_ratio(rs["cov"], ref, c["n"], c["kappa"])
            m["lapack_cov"] = pu.cov_ratio(lp["cov"], ref, c["n"], c["kappa"])
        out[name] = m
    return out


def test_refinement_converged_on_every_case():
    for name, (group, _) in TABLE.items():
        _, ref = pu.get_case(name, group == "i")
        assert ref["corrections"][-1] <= ref["tol"] and ref["iters"] <= 12, (name, ref["corrections"])
        # the corrections fall until they reach the floor of the extended residual: the first is a float64 solve's error
        assert ref["corrections"][-1] <= ref["corrections"][0], (name, ref["corrections"])


def test_reference_refuses_what_it_cannot_refine():
    """a correction of 2^-60 of the solution is below the floor kappa 2^-64 of an extended residual once kappa is large: asked
    for it (kappa = 1 claimed for a matrix of 1e8), the reference refuses instead of returning what it has"""
    p, _ = pu.spd_matrix(40, 1e8, 3)
    with pytest.raises(RuntimeError, match="did not converge"):
        pu.reference(p, np.ones((1, 40)), 1.0)


def test_bound_holds_for_both_float64_routes_and_its_constant_is_the_measured_one(measured):
    worst = {}
    for name, m in measured.items():
        for k, v in m.items():
            if v > worst.get(k, (0.0, ""))[0]:
                worst[k] = (v, name)
            assert v <= pu.C_BOUND, (name, k, v)
    print("worst ratio / unit:", {k: (f"{v:.3g}", nm) for k, (v, nm) in worst.items()}, "C_BOUND", pu.C_BOUND)
    w = max(worst["restate"][0], worst.get("restate_cov", (0.0, ""))[0])
    assert pu.C_BOUND / 2 < 8 * w <= pu.C_BOUND, (w, pu.C_BOUND)


@pytest.mark.parametrize("mutant", pu.MUTANTS)
def test_every_mutant_leaves_the_bound(mutant):
    caught = []
    for name, (group, spec) in TABLE.items():
        if spec["n"] > 200 or spec["neval"] > 40 or spec["kappa"] != 1e1:
            continue                                        # the sensitive cases: kappa = 10
        c, ref = pu.get_case(name, group == "i")
        P = c["P"]
        if mutant == "upper_triangle":                      # the lower triangle is the matrix; the upper one holds another,
            P = np.tril(P) + 0.5 * np.triu(P, 1)            # (P + diag P) / 2: positive definite as well
        r = pu.var_ratio(pu.restate(P, c["rows"], c["off"], mutant)["var"], ref, c["n"], c["kappa"])
        if r > pu.C_BOUND:
            caught.append(name)
    assert caught, mutant
    print(mutant, "caught on", len(caught), "cases, e.g.", caught[:3])


def test_restatement_reads_the_lower_triangle_only():
    c, _ = pu.get_case("e_off2_full")
    other, _ = pu.spd_matrix(c["n"], 1e1, 999)
    P = np.tril(c["P"]) + np.triu(other, 1)
    a, b = pu.restate(c["P"], c["rows"], c["off"]), pu.restate(P, c["rows"], c["off"])
    np.testing.assert_array_equal(a["var"], b["var"])


def test_packed_image_and_padding_invariants():
    for name in ("e_off17_part", "a_n17_k1e+01_e40", "a_n33_k1e+06_e17"):
        c, _ = pu.get_case(name)
        n, off = c["n"], c["off"]
        bex = pu.pack_rows(c["rows"], n, off)
        nex, nchp = (c["neval"] + 15) // 16, gu.nchp_of(n)
        assert bex.shape == (nex, nchp, 256)
        full = pu.unpack_rows(bex)
        np.testing.assert_array_equal(full[:c["neval"], :n], pu.full_rows(c["rows"], n, off))
        assert not full[c["neval"]:].any() and not full[:, n:].any()
        # the layout is the factor's: one tile of the image is pack_tiles' tile of the same matrix
        sq = np.zeros((nchp * 16, nchp * 16))
        sq[:16] = full[:16]
        np.testing.assert_array_equal(gu.pack_tiles(sq, nchp * 16)[:nchp * 256].reshape(nchp, 256)[0], bex[0, 0])
        # the restatement's Y: rows beyond neval do not exist, columns beyond n are exactly zero, a zero row stays zero
        rs = pu.restate(c["P"], c["rows"], off)
        assert not rs["Y"][:, n:].any()
        if c["neval"] >= 4:
            assert rs["var"][2] == 0.0
