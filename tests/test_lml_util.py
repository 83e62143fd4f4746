"""CPU: the numpy statement of the log marginal likelihood (hipdrt/models/lml.py) against the reference's own evaluate_lml runs
(tools/make_lml_golden.py: every history entry of four fits, and three variants of the final state), the extended-precision
log-determinant helper of the GPU kernel test against slogdet, the corner cases of lml_from_terms, the C ABI's new names and
struct layouts, and the argument checks of the DRT methods that need no device.

Bounds: tests/lml_bounds.json, `statement:<term>` -- the largest deviation of the statement from the recorded values over the four
fixtures, relative to max(1, |recorded|) per term and absolute for lml, times 10 to 50, rounded to 1 / 2 / 5 x 10^k, and never below
1e-13 (a deviation of a few ulp is no measurement).  lml amplifies the cancellation in beta = 0.5 (wy2 - fit2 - xox) + 1 by
alpha |W y|^2 / |beta|, up to 4e6 on these fixtures, which is why its bound is orders above the terms'."""
import os
import re
import warnings

import numpy as np
import pytest

import lml_util as U
from conftest import ROOT


@pytest.mark.parametrize("name", U.FIXTURES)
def test_statement_reproduces_every_recorded_term_and_lml(name):
    from hipdrt.models import lml
    g = U.load(name)
    m = len(g["rv"])
    got = np.array([U.statement_terms(g, i)[0] for i in range(len(g["lml"]))])
    assert all(U.statement_terms(g, i)[1] == 0 for i in (0, len(g["lml"]) - 1))
    for k, term in enumerate(U.TERMS):
        U.check(f"statement:{term}", got[:, k], g["terms"][:, k])
    lml_got = lml.lml_from_terms({t: got[:, k] for k, t in enumerate(U.TERMS)}, m)
    U.check("statement:lml", lml_got, g["lml"], absolute=True)
    assert np.isnan(g["lml"]).any() and np.isfinite(g["lml"]).any()
    # upstream's beta decides the NaN pattern with a margin no rounding reaches
    assert np.all(np.abs(g["beta"]) >= 1e-6 * g["terms"][:, U.TERMS.index("wy2")])
    last = len(g["lml"]) - 1
    assert int(g["final_is_last"]) == 1
    for tag in U.VARIANTS:
        update, weights = U.variant_kw(g, tag)
        t, status = U.statement_terms(g, last, update, weights)
        assert status == 0
        for k, term in enumerate(U.TERMS):
            U.check(f"statement:{term}", t[k:k + 1], g[f"terms_{tag}"][k:k + 1])
        U.check("statement:lml", np.array([lml.lml_from_terms(dict(zip(U.TERMS, t)), m)]), np.array([float(g[f"lml_{tag}"])]), absolute=True)


def test_sample_values_of_the_known_answer_fit():
    g = U.load("golden71x91")
    assert abs(float(g["lml_final"]) - 162.108606324) < 1e-8 and abs(float(g["lml_l2x2"]) - 254.783159123) < 1e-8
    assert np.array_equal(g["lml"][-1:], np.array([float(g["lml_final"])]))


def test_qphb_evaluate_lml_is_the_statement_behind_upstreams_signature():
    from hipdrt.models import qphb
    g = U.load("golden71x91")
    i = len(g["lml"]) - 1
    val = qphb.evaluate_lml(g["x"][i], U.penalty_of(g), "integral", U.hypers_of(g), g["l1_lambda_vector"], g["rho_vector"][i], None,
                            g["s_vectors"][i], g["est_weights"], g["rm"], g["rv"], U.special_of(g))
    U.check("statement:lml", np.array([val]), g["lml"][i:i + 1], absolute=True)
    bad = U.penalty_of(g)
    bad["m0"] = -bad["m0"]
    with pytest.raises(ValueError, match="Determinant of .* covariance matrix is negative - not PSD"):
        qphb.evaluate_lml(g["x"][i], bad, "integral", U.hypers_of(g, derivative_weights=np.array([1.0, 0.0, 0.0])), g["l1_lambda_vector"],
                          g["rho_vector"][i], None, g["s_vectors"][i], g["est_weights"], g["rm"], g["rv"], U.special_of(g))


@pytest.mark.parametrize("name", U.FIXTURES)
def test_longdouble_cholesky_logdet_agrees_with_slogdet(name):
    """the reference of the GPU kernel test, on the fixtures' own P and Omega (eigenvalues 3e-6 ... 3e4): slogdet's LU and the
    extended-precision Cholesky sum agree to the double rounding of slogdet, 1e-12 of a log-determinant of several hundred"""
    g = U.load(name)
    for i in (0, len(g["lml"]) - 1):
        for a in U.omega_and_p(g, i):
            sign, ld = np.linalg.slogdet(a)
            assert sign > 0
            assert abs(U.longdouble_logdet(a) - ld) <= 1e-12 * max(1.0, abs(ld))
    with pytest.raises(np.linalg.LinAlgError):
        U.longdouble_logdet(np.array([[1.0, 2.0], [2.0, 1.0]]))


def test_lml_from_terms_nan_and_inf_without_warnings():
    from hipdrt.models import lml
    base = dict(logdet_p=10.0, logdet_prior=4.0, slw=3.0, fit2=1.0, xox=1.0)
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert np.isnan(lml.lml_from_terms(dict(base, wy2=-1.0), 10))            # beta = -0.5
        assert lml.lml_from_terms(dict(base, wy2=0.0), 10) == np.inf             # beta = 0
        assert np.isfinite(lml.lml_from_terms(dict(base, wy2=5.0), 10))
        both = lml.lml_from_terms({k: np.array([v, v]) for k, v in dict(base, wy2=0.0).items()} | {"wy2": np.array([-1.0, 5.0])}, 10)
    assert np.isnan(both[0]) and np.isfinite(both[1])


def struct_members(header, struct):
    body = re.search(r"typedef struct \{([^}]*)\}\s*" + struct + ";", header).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if decl:
            names += [re.sub(r"\[\d+\]", "", n).strip(" *") for n in decl.split(" ", 1 + decl.startswith("const "))[-1].split(",")]
    return names


def test_header_and_ctypes_table_hold_the_new_symbols():
    from hipdrt import _ffi
    release = open(os.path.join(ROOT, "include", "hipdrt.h")).read()
    debug = open(os.path.join(ROOT, "include", "hipdrt_debug.h")).read()
    assert re.search(r"\bint\s+hipdrt_plan_lml_terms\s*\(", release) and re.search(r"\bvoid\s+hipdrt_default_lml_in\s*\(", release)
    assert re.search(r"\bint\s+hipdrt_debug_logdet\s*\(\s*hipdrt_ctx\* ctx", debug)
    for name in ("hipdrt_plan_lml_terms", "hipdrt_default_lml_in", "hipdrt_debug_logdet"):
        assert name in _ffi.SIGNATURES
    assert _ffi._RESTYPES["hipdrt_default_lml_in"] is None
    # struct layouts: one ctypes field per member of the C struct, in order
    for struct, cls in (("hipdrt_lml_in", _ffi.LmlIn), ("hipdrt_lml_out", _ffi.LmlOut)):
        assert struct_members(release, struct) == [f[0] for f in cls._fields_], struct
    assert tuple(f[0] for f in _ffi.LmlOut._fields_[:-1]) == _ffi.LML_TERMS == U.TERMS
    # the header cites the reference lines the feature restates
    assert "drt1d.py:4513-4543" in release and "qphb.py:1279-1344" in release


class _Plan:
    B, m, n = 1, 4, 3


def _unfitted():
    from hipdrt.models import DRT
    drt = DRT.__new__(DRT)
    drt._plan, drt.special_qp_params = _Plan(), {}
    drt.fit_kwargs = dict(l2_lambda_0=142.0, derivative_weights=np.array([1.5, 1.0, 0.5]))
    return drt


def test_update_hypers_with_an_unknown_key_raises():
    drt = _unfitted()
    with pytest.raises(ValueError, match="unknown key"):
        drt.evaluate_lml_batch(update_hypers={"l2_lambda": 3.0})
    with pytest.raises(ValueError, match="exclude each other"):
        drt.evaluate_lml_batch(state={}, step=0)


def test_a_history_entry_without_s_vectors_raises():
    drt = _unfitted()
    entry = dict(x=np.zeros(3), rho_vector=np.ones(3), weights=np.ones(4))          # the form of this project's qphb_history
    with pytest.raises(ValueError, match=r"s_vectors.*step=.*state="):
        drt.evaluate_lml(history_entry=entry)
    with pytest.raises(ValueError, match="s_vectors"):
        drt.evaluate_lml_batch(state=entry)
