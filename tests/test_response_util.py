"""CPU: the numpy statement of response prediction (hipdrt/models/response.py) against runs of the reference
(tests/golden/refrun_response_predict_*.npz, written by tools/make_response_golden.py), the generalised vz-offset strength, and the
new symbols in the header and the ctypes table.

The statement sums per step first and then over the steps, as the device does; the reference adds the steps into one matrix and
multiplies once.  Both are float64 evaluations of the same sum of products, so they may differ by twice the rounding bound of one
evaluation: 2 (K + S + 8) 2^-53 sum |terms| per element (K products per row, S steps, a handful of scalar operations), with the sum
of absolute terms taken from the statement itself."""
import os
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT

CASES = ("hybrid_s0", "hybrid_s0_dop", "hybrid_s0_dop_solverp", "hybrid_3step", "chrono_s1")
U = 2.0 ** -53


def load(name):
    return np.load(os.path.join(GOLDEN, f"refrun_response_predict_{name}.npz"))


def params(g):
    """the reference's recorded fit_parameters, as models.response reads them"""
    return {k[3:]: g[k] for k in g.files if k.startswith("fp_")}


def rows_kw(g, tag):
    return dict(u_drt=g[f"u_{tag}"], step_sizes=g["step_sizes"], fp=params(g),
                u_dop=g[f"u_dop_{tag}"] if f"u_dop_{tag}" in g.files else None, inf_rv=g[f"inf_rv_{tag}"],
                cap_rv=g[f"cap_rv_{tag}"], vz_strength=g[f"strength_{tag}"], vb_mat=g[f"vb_mat_{tag}"])


def assert_within(label, got, want, mag, k, s):
    bound = 2 * (k + s + 8) * U * mag
    worst = np.max(np.abs(got - want) / np.maximum(bound, 1e-300))
    assert np.all(np.abs(got - want) <= bound), f"{label}: {worst:.2f} x the rounding bound"


@pytest.mark.parametrize("name", CASES)
@pytest.mark.parametrize("tag", ("fit", "off"))
def test_statement_reproduces_the_reference_run(name, tag):
    from hipdrt.models import response
    g = load(name)
    kw = rows_kw(g, tag)
    s, k = len(g["step_sizes"]), max(len(g["fp_x"]), len(g["fp_x_dop"]) if "fp_x_dop" in g.files else 0)
    got, mag = response.predict_response_rows(**kw, return_abs=True)
    assert np.abs(g[f"response_{tag}"]).max() > 0.05            # (the fixture is a real transient, not zeros)
    assert_within(f"{name} response_{tag}", got, g[f"response_{tag}"], mag, k, s)
    for term in ("drt", "ohmic", "cap", "dop", "vz_offset"):
        got, mag = response.predict_response_rows(**kw, **{f"include_{term}": False}, return_abs=True)
        assert_within(f"{name} response_{tag}_no_{term}", got, g[f"response_{tag}_no_{term}"], mag, k, s)
    vb = response.predict_v_baseline_rows(kw["vb_mat"], kw["fp"])
    assert_within(f"{name} v_baseline_{tag}", vb, g[f"v_baseline_{tag}"], np.abs(kw["vb_mat"]) @ np.abs(kw["fp"]["v_baseline"]), 1, 1)
    # the off-grid times start before the first step (no response there but the baseline) and end past the last sample
    if tag == "off":
        assert g["t_off"][0] < g["step_times"][0] and g["t_off"][-1] > g["t_fit"][-1]
        assert np.array_equal(got[:3], np.zeros(3) + vb[:3])


def test_two_copies_enter_with_their_signs():
    """series_neg: x = [x+ | x-] is applied as [U, -U] (drt1d.py:6112-6113)"""
    from hipdrt.models import response
    g = load("hybrid_3step")
    kw = rows_kw(g, "off")
    x = kw["fp"]["x"]
    rng = np.random.default_rng(3)
    xn = np.abs(rng.standard_normal(len(x))) * 1e-2
    one = response.predict_response_rows(**dict(kw, fp=dict(kw["fp"], x=x - xn)))
    two, mag = response.predict_response_rows(**dict(kw, fp=dict(kw["fp"], x=np.concatenate([x, xn]))), return_abs=True)
    assert_within("two copies", two, one, mag, 2 * len(x), 3)
    with pytest.raises(ValueError, match="coefficients for a basis"):
        response.predict_response_rows(**dict(kw, fp=dict(kw["fp"], x=x[:-1])))


def test_fit_parameters_follow_extract_qphb_parameters():
    """the rescaling of a scaled solution (drt1d.py:6228-6289), on a made-up vector with every special block"""
    from hipdrt.models import response
    x = np.arange(1.0, 13.0)
    fp = response.fit_parameters(x, ns=8, coefficient_scale=2.0, idx_rinf=3, idx_cinv=4, capacitance_scale=0.5, vz_index=2, vb_start=0,
                                 v_baseline_scale=[4.0, 8.0], scaled_response_offset=0.125, response_signal_scale=3.0, dop_start=5,
                                 dop_scale_vector=[1.0, 10.0, 100.0])
    assert np.array_equal(fp["x"], x[8:] * 2.0) and fp["R_inf"] == 8.0 and fp["C_inv"] == 5.0 and fp["vz_offset"] == 3.0
    assert np.array_equal(fp["v_baseline"], [(1.0 / 4.0 - 0.125) * 3.0, (2.0 / 8.0) * 3.0])
    assert np.array_equal(fp["x_dop"], [6.0 * 2.0, 7.0 * 20.0, 8.0 * 200.0])
    bare = response.fit_parameters(x, ns=8, coefficient_scale=2.0)
    assert bare["R_inf"] == 0 and bare["C_inv"] == 0 and "v_baseline" not in bare and "vz_offset" not in bare and "x_dop" not in bare


@pytest.mark.parametrize("name", CASES)
def test_vz_strength_at_off_grid_times_and_frequencies(name):
    """DRT._get_vz_strength_vec (drt1d.py:6173-6226) evaluated away from the fit's own samples, against the fit's overlap limits"""
    from hipdrt.models import response
    g = load(name)
    hybrid = "freq" in g.files
    eps = None if np.isnan(g["vz_offset_eps"]) else float(g["vz_offset_eps"])
    kw = dict(fit_times=g["t_fit"], step_times=g["nonconsec_step_times"], fit_frequencies=g["freq"] if hybrid else None,
              vz_offset_eps=eps)
    for tag in ("fit", "off"):
        cs, _ = response.vz_strength(times=g[f"t_{tag}"], **kw)
        assert np.array_equal(cs, g[f"strength_{tag}"]), (name, tag)
    if hybrid:
        off = g["strength_off"]
        assert off[0] == 0 and off.max() == 1 and 0 < off[-1] < 1         # before the first step, inside the overlap, past it
        for tag, f in (("fit", g["freq"]), ("wide", g["f_wide"])):
            _, es = response.vz_strength(frequencies=f, **kw)
            assert np.array_equal(es, g[f"eis_strength_{tag}"]), (name, tag)
        assert g["eis_strength_wide"].min() < 1
    else:
        assert np.array_equal(g["strength_off"], np.ones(len(g["t_off"])))


def test_the_fit_path_keeps_its_strength_vector():
    """PreparedFitMixin._vz_strength at the fit's own samples is what it was before it took prediction grids"""
    from hipdrt.models import DRT
    g = load("hybrid_3step")
    cs, es = DRT._vz_strength(None, g["t_fit"], g["freq"], g["nonconsec_step_times"], 2)
    assert np.array_equal(cs, g["strength_fit"]) and np.array_equal(es, g["eis_strength_fit"])
    cs, es = DRT._vz_strength(None, g["t_fit"], g["freq"], g["nonconsec_step_times"], 2, times=g["t_off"], predict_frequencies=g["f_wide"])
    assert np.array_equal(cs, g["strength_off"]) and np.array_equal(es, g["eis_strength_wide"])


def test_header_and_ctypes_table_hold_the_new_symbols():
    from hipdrt import _ffi
    release = open(os.path.join(ROOT, "include", "hipdrt.h")).read()
    debug = open(os.path.join(ROOT, "include", "hipdrt_debug.h")).read()
    for name in ("hipdrt_plan_set_predict_desc", "hipdrt_plan_predict_response", "hipdrt_plan_predict_z_model", "hipdrt_plan_predict_dop"):
        assert re.search(rf"\bint\s+{name}\s*\(", release), name
        assert name in _ffi.SIGNATURES
    assert re.search(r"\bint\s+hipdrt_debug_response\s*\(\s*hipdrt_ctx\* ctx", debug) and "hipdrt_debug_response" in _ffi.SIGNATURES
    # the include-mask bits of the header and of the binding agree
    bits = dict(re.findall(r"#define HIPDRT_INCLUDE_([A-Z_]+) (\d+)", release))
    assert {k: int(v) for k, v in bits.items()} == {k[8:]: getattr(_ffi, k) for k in dir(_ffi) if k.startswith("INCLUDE_") and k != "INCLUDE_ALL"}
    assert _ffi.INCLUDE_ALL == sum(int(v) for v in bits.values())
    # struct layouts: one ctypes field per member of the C struct, in order
    for struct, cls in (("hipdrt_predict_desc", _ffi.PredictDesc), ("hipdrt_response_args", _ffi.ResponseArgs),
                        ("hipdrt_z_model_args", _ffi.ZModelArgs)):
        body = re.search(r"typedef struct \{([^}]*)\}\s*" + struct + ";", release).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n for decl in body.split(";") for n in re.findall(r"\*?\s*([a-z_]+)\s*(?:,|$)", decl.strip().split(" ", 1)[-1] if decl.strip() else "")]
        assert names == [f[0] for f in cls._fields_], (struct, names)


# ---- impedance of a prepared fit and distribution of phasances ----------------------------------------------------------------------
Z_CASES = ("hybrid_s0", "hybrid_s0_dop", "hybrid_s0_dop_solverp", "hybrid_3step", "golden71_dop", "golden71_cap")


@pytest.mark.parametrize("name", Z_CASES)
@pytest.mark.parametrize("tag", ("fit", "wide"))
def test_z_statement_reproduces_the_reference_run(name, tag):
    from hipdrt.models import response
    g = load(name)
    fp, f = params(g), g["freq" if tag == "fit" else "f_wide"]
    zm = g[f"zm_{tag}"]
    kw = dict(a_re=zm.real, a_im=zm.imag, frequencies=f, fp=fp, zm_dop=g[f"zm_dop_{tag}"] if f"zm_dop_{tag}" in g.files else None,
              eis_strength=g[f"eis_strength_{tag}"])
    k = max(zm.shape[1], len(fp["x_dop"]) if "x_dop" in fp else 0)

    def check(label, want, **flags):
        got, mag = response.predict_z_model_rows(**kw, **flags, return_abs=True)
        bound = 2 * (k + 8) * U * mag
        assert np.all(np.abs(got.real - want.real) <= bound) and np.all(np.abs(got.imag - want.imag) <= bound), (name, label)
    check("z", g[f"z_{tag}"])
    check("z_no_vz", g[f"z_{tag}_no_vz"], include_vz_offset=False)
    for term in ("drt", "ohmic", "inductance", "cap", "dop"):
        check(f"z_no_{term}", g[f"z_{tag}_no_{term}"], **{f"include_{term}": False})
    if "fp_vz_offset" in g.files and tag == "wide":
        assert not np.array_equal(g["z_wide"], g["z_wide_no_vz"])
    if name == "golden71_cap":
        assert fp["C_inv"] > 0 and not np.array_equal(g[f"z_{tag}"], g[f"z_{tag}_no_cap"])


@pytest.mark.parametrize("name", ("hybrid_s0_dop", "hybrid_s0_dop_solverp", "golden71_dop"))
def test_dop_statement_reproduces_the_reference_run(name):
    from hipdrt.models import response
    g = load(name)
    fp, nu, bm = params(g), g["dop_nu"], g["dop_basis_matrix"]
    assert {-1.0, 0.0, 1.0} <= set(nu.tolist()) and np.all(np.diff(nu) > 0)
    k = bm.shape[1]

    def check(label, got_mag, want):
        got, mag = got_mag
        assert np.all(np.abs(got - want) <= 2 * (k + 8) * U * mag), (name, label)
    check("dop", response.predict_dop_rows(bm, nu, fp, return_abs=True), g["dop"])
    check("dop_no_ideal", response.predict_dop_rows(bm, nu, fp, include_ideal=False, return_abs=True), g["dop_no_ideal"])
    assert g["dop"][nu == 0][0] - g["dop_no_ideal"][nu == 0][0] == pytest.approx(float(fp["R_inf"]), rel=1e-12)
    # get_dop_norm: the default normalize_tau is the measured tau range
    from hipdrt import preprocessing as pp
    hybrid = "t_fit" in g.files
    tau_lim = pp.get_tau_lim(g["freq"], g["t_fit"] if hybrid else None, g["step_times"] if hybrid else None)
    norm = response.dop_norm(nu, tau_lim, float(g["nu_epsilon"]))
    assert np.allclose(norm, g["dop_normalize_by"], rtol=4 * U, atol=0)
    area = float(g["nu_basis_area"])
    assert area == np.sqrt(np.pi) / float(g["nu_epsilon"])
    check("dop_norm", response.predict_dop_rows(bm, nu, fp, normalize_by=norm, nu_basis_area=area, return_abs=True), g["dop_norm"])
    assert np.all(np.diff(g["nu7"]) > 0)                                     # (the reference sorts a given grid)
