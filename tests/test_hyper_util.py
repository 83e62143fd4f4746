"""CPU: the numpy reference of tests/test_gpu_hyper.py (tests/hyper_util.py) is itself checked, on the very inputs the GPU tests
use -- the derived error bounds from above (the oracle's float64 solve_s / solve_rho / estimate_weights / is_converged, which sum in
another order, and a plain float64 restatement stay inside them), from below (every listed mutant of the restatement leaves them
on at least one case), and the distance of every case from the switch points of the step."""
import numpy as np
import pytest

import hyper_util as hu

TABLE = hu.case_table()
GROUPS = sorted({g for g, _ in TABLE.values()})


def oracle_step(c, b, structure):
    """the DRT-block part of one step by the oracle's float64 functions -> dict(s [3][nd], rho [3], w [m], converged)"""
    from oracle import drt_oracle as orc
    o, ns, n = c["opts"], c["ns"], c["n"]
    x = c["x"][b]
    xd = x[ns:]
    out = dict(s=np.array(c["s"][b][:, ns:]), rho=np.array(c["rho"][b]))
    for k in range(3):
        if not o["derivative_weights"][k] > 0:
            continue
        pm = c["mk"][k][ns:n, ns:n]
        g = 0
        if k == 0:
            xh = np.sign(xd) * np.abs(xd) ** 0.5
            g = (xh[:, None] * c["mk"][1][ns:n, ns:n]) * xh[None, :]
        reff = 1 if o["eff_hp"] else c["rho"][b, k]
        sv = orc.solve_s(pm, xd, c["s"][b, k, ns:], reff, o["s_alpha"][k], (o["s_alpha"][k] - 1) / o["s_0"][k], g, o["sigma_ds"][k],
                         structure)
        sv[sv <= 0] = 1e-15
        out["s"][k] = sv
        out["rho"][k] = orc.solve_rho(pm, xd, sv, o["rho_alpha"][k], o["rho_alpha"][k] / o["rho_0"][k], c["xmx"][b, k])
    rm = (c["rm"][b] if c["rm"].ndim == 3 else c["rm"])[:, :n]
    out["w"] = orc.estimate_weights(x, c["rv"][b], c["vmm"], rm, c["est_w"][b], o["outlier_p"] if o["outlier_p"] > 0 else None)
    out["converged"] = orc.is_converged(c["x_in"][b], x, np.mean(c["x_in"][b]) * 1e-3, o["xtol"])
    return out


@pytest.mark.parametrize("group", GROUPS)
def test_bounds_hold_for_float64_in_another_order_and_cases_keep_their_distance(group):
    worst = {}
    for name, (g, _) in TABLE.items():
        if g != group:
            continue
        c, ref = hu.get_case(name)
        mg = hu.margins(ref, c)
        # switch points: gmax a factor 1e3 from 1e-10, both convergence measures 1e-6 relative from their thresholds, at most 1 % of
        # a spectrum's entries left out of a value comparison
        assert mg["gmax"] >= 3.0 and mg["conv"] >= 1e-6 and mg["excluded"] <= 0.01, (name, mg)
        f64 = hu.step(c, np.float64)
        r = hu.ratios(f64, ref)
        assert max(r.values()) <= 1.0 and hu.ints_equal(f64, ref), (name, r)
        assert np.array_equal(f64["converged"], ref["converged"]), name
        for key, v in r.items():
            worst[key] = max(worst.get(key, 0.0), v)
        ns = c["ns"]
        for b in range(c["B"]):
            if not c["active"][b] or c["qp_status"][b] < 0:
                continue
            for structure in ("fast",) + (("reference",) if c["nd"] <= 100 else ()):
                o = oracle_step(c, b, structure)
                got = dict(s=np.array(ref["s"][b], dtype=float), rho=np.array(ref["rho"][b], dtype=float), w=o["w"])
                got["s"][:, ns:], got["rho"] = o["s"], o["rho"]
                if c["desc"] and c["desc"]["dop_size"] > 0:         # (the oracle's step has no x_dop pass: the DRT block alone)
                    d0, dn = c["desc"]["dop_start"], c["desc"]["dop_size"]
                    got["s"][:, d0:d0 + dn] = np.array(ref["s"][b][:, d0:d0 + dn], dtype=float)
                for key in ("s", "rho", "w"):
                    refv, bnd, ex = ref[key][b], ref["bound"][key][b], ref["exclude"].get(key)
                    if key == "w" and ref["x_in"][b][0] != c["x"][b][0]:      # update_scale ran: the oracle's weights are the unscaled ones
                        continue
                    err = np.abs(np.asarray(got[key], dtype=np.longdouble) - refv).astype(float)
                    ok = (err <= bnd) | (ex[b] if ex is not None else False)
                    assert ok.all(), (name, b, structure, key, float(np.max(err / np.maximum(bnd, 1e-300))))
                assert o["converged"] == bool(ref["converged"][b]), (name, b)
    print(f"{group}: float64 restatement / bound, worst per output: " + "  ".join(f"{k} {v:.3f}" for k, v in worst.items() if v > 0))


# mutant -> the cases it is tried on (all of them small); at least one must leave the bounds
MUTANTS = {
    "lag0": ["toep_nd9_r3", "gen_nd5_ns1_pad0_m5", "s_neg"],
    "lastcol": ["toep_nd9_r3", "toep_nd65_r5", "toep_nd64_r2"],
    "noalign": ["toep_nd9_r3", "toep_nd65_r5", "toep_nd64_r2"],
    "sqrt_new_s": ["toep_nd9_r3", "s_neg_general"],
    "xmx_order": ["toep_nd9_r3", "s_noeff"],
    "resid_sign": ["w_outlier", "w_outlier_floor"],
    "floor_after_blend": ["w_floor_rows", "w_outlier_floor"],
    "no_eps": ["f_eps_in"],
}


@pytest.mark.parametrize("mutant", sorted(MUTANTS))
def test_each_mutant_of_the_float64_restatement_leaves_the_bounds(mutant):
    assert all(n in TABLE for n in MUTANTS[mutant]), [n for n in MUTANTS[mutant] if n not in TABLE]
    caught = []
    for name in MUTANTS[mutant]:
        c, ref = hu.get_case(name)
        good = hu.step(c, np.float64)
        assert max(hu.ratios(good, ref).values()) <= 1.0 and hu.ints_equal(good, ref)
        bad = hu.step(c, np.float64, mutant=mutant)
        r = hu.ratios(bad, ref)
        if max(r.values()) > 1.0 or not hu.ints_equal(bad, ref):
            caught.append((name, max(r.values())))
    print(mutant, caught)
    assert caught, mutant


def test_window_mask_is_the_kernels_column_range():
    for nd in (1, 2, 3, 5, 8, 9, 13, 64, 65):
        for reach in (0, 1, 2, 3, 4, 5, nd - 1, nd + 7):
            mask = hu.window_mask(nd, reach)
            for i in range(nd):
                ia = i - i % 2
                lo = (ia - reach) // 4 * 4 if ia - reach > 0 else 0
                hi = min(-(-(ia + 2 + reach) // 4) * 4, nd)
                assert np.array_equal(np.nonzero(mask[i])[0], np.arange(lo, hi)), (nd, reach, i)
                # it covers everything within the reach of the row: what it leaves out are exact zeros
                assert mask[i, max(i - reach, 0):min(i + reach, nd - 1) + 1].all()
    assert hu.window_mask(7, -1).all()


def test_exact_sum_fallback_agrees_with_the_extended_reference():
    if hu.extended_dtype() is None:
        pytest.skip("no extended type on this platform: the fallback IS the reference")
    for name in ("toep_nd9_r3", "gen_nd5_ns1_pad0_m5", "w_outlier", "f_scale", "f_vz_cont1", "s_dop_2_5"):
        c, ref = hu.get_case(name)
        r = hu.ratios(hu.step(c, hu.EXACT), ref)
        assert max(r.values()) <= 0.5, (name, r)


def test_cases_cover_the_listed_shapes():
    kw = {name: v[1] for name, v in TABLE.items()}
    toep = {(k["nd"], k["toep_reach"]) for n_, k in kw.items() if n_.startswith("toep_")}
    for nd in hu.TOEP_ND:
        assert {r for d, r in toep if d == nd} == set(hu.toep_reaches(nd)) and nd % 2 in (0, 1)
    gen = [k for n_, k in kw.items() if n_.startswith("gen_")]
    assert {k["nd"] for k in gen} == set(hu.GEN_ND) and {k["m"] for k in gen} == set(hu.GEN_M) and {k["ns"] for k in gen} == {1, 2}
    assert {(k["nd"] + k["ns"]) % 2 for k in gen} == {0, 1} and {k["ldm"] - k["nd"] - k["ns"] for k in gen} == {0, 1}
    c, ref = hu.get_case("s_order_off")
    assert (np.asarray(ref["s"][:, 1], dtype=float) == hu.POISON).all() and (np.asarray(ref["rho"][:, 1], dtype=float) == hu.POISON).all()
    # the branches the cases are named for are the ones the reference takes
    assert np.nanmax(hu.get_case("s_tiny")[1]["gmax"]) <= 1e-13 and np.nanmin(hu.get_case("s_neg")[1]["gmax"]) >= 1e-7
    z, zr = hu.get_case("s_zeros")
    assert (np.asarray(zr["s"], dtype=float)[:, :, z["ns"]::3] == 1e-15).all()
    a, ar = hu.get_case("s_alpha1")
    s1 = np.asarray(ar["s"], dtype=float)[:, 1, a["ns"]:]
    assert (s1[:, ::3] == 1.0).all() and (np.delete(s1, np.arange(0, s1.shape[1], 3), axis=1) == 1e-15).all()
    w, wr = hu.get_case("w_floor_1e10")
    assert (np.asarray(wr["w"], dtype=float) == 1e-10).sum() >= 3 * w["B"]
    f, fr = hu.get_case("w_floor_rows")
    sh_low = np.asarray(fr["w"], dtype=float)[:, :5]
    assert sh_low.min() > 0
    o, orf = hu.get_case("w_outlier")
    t = np.asarray(orf["outlier_t"], dtype=float)
    assert (t == 1.0).any() and (t < 0.5).any()
    for name, want in dict(f_rel_in=True, f_rel_out=False, f_abs_in=True, f_abs_out=False, f_eps_in=True, f_it1=False).items():
        assert bool(hu.get_case(name)[1]["converged"].all()) == want and bool(hu.get_case(name)[1]["converged"].any()) == want, name
    for name, scaled in dict(f_scale=True, f_scale_it0=False, f_scale_stop=False, f_scale_last=False, f_scale_cont=False,
                             f_scale_noscale=False, f_scale_dop=True).items():
        c, ref = hu.get_case(name)
        assert bool((np.asarray(ref["rv"], dtype=float) != c["rv"]).any()) == scaled, name
