"""CPU: the host layer that re-enters the device loop on a finished fit (models/restart.py: the warm restart, the candidate
generators, the PFRT step loop) against a recording stand-in for the device plan, once per plan kind: the plan calls of a
restart in their order with their arguments (the FitOpts struct byte for byte), the row factors of a prepared plan, what is
collected, the refusals, what every candidate step receives, and the PFRT loop with its result.

The library is needed for the defaults of FitOpts only; no device is touched.  Every expected value is written here from the
rules (a step at factor f sets s_0 * f and l2_lambda_0 / f; a missing chrono / eis factor of a restart falls back to the FIT's
chrono factor, for both blocks; a failure in any step of a chain stays), not read back from the code under test.

Fixed inputs: EIS plans with 3 members, n = 2 + 91 unknowns, m = 142 data rows (71 frequencies); prepared plans with 2 joint
measurements of 40 chrono samples and 51 frequencies (m = 40 + 2 * 51 = 142), n = 4 + 91; 3 PFRT factors."""
import os
import types

import numpy as np
import pytest

from conftest import ROOT

B, NS, NB, M = 3, 2, 91, 142
NC, NF, NSP = 40, 51, 4
BASIS = np.logspace(-7, 2, NB)
F71 = np.logspace(5, -2, 71)
FACTORS = [0.5, 1.0, 4.0]
S0_FIT, L2_FIT = np.array([1.0, 2.0, 3.0]), 100.0          # the fit's own s_0 / l2_lambda_0 (not the defaults 1 / 142)


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "hybrid-drt_amd", "libhipdrt.so")):
        g.build()
    from hipdrt import _ffi
    _ffi.load_library()
    return _ffi


def eq(a, b):
    np.testing.assert_array_equal(a, b)


def rows(*shape):
    """member b holds (b + 1) * (1, 2, 3, ...): no two members and no two columns alike"""
    a = np.arange(1, int(np.prod(shape[1:], dtype=int)) + 1, dtype=float).reshape(shape[1:])
    return np.stack([(b + 1) * a for b in range(shape[0])])


class RecPlan:
    """what the restart layer calls on a plan: every method stores its arguments; what comes back depends on the member, the
    column and the number of restarts run so far (``step``), so that no two members, steps or columns are alike"""

    def __init__(self, batch=B, n=NS + NB, ns=NS, dop_size=0, status=None):
        self.B = self.batch = self.capacity = batch
        self.n, self.m, self.ns, self.ntau = n, M, ns, NB
        self.desc = types.SimpleNamespace(dop_size=dop_size)
        self.status_by_step = status or {}
        self.step = 0
        self.calls = []

    def rec(self, name, **kw):
        self.calls.append((name, kw))

    def names(self, start=0):
        return [n for n, _ in self.calls[start:]]

    def all(self, name):
        return [kw for n, kw in self.calls if n == name]

    # what the device holds after `step` restarts
    def x(self, step):
        return rows(self.B, self.n) + 1000.0 * step

    def s_vectors(self, step):
        return rows(self.B, 3, self.n) + 7.0 + 1000.0 * step

    def weights(self, step):
        return rows(self.B, M) / (1 + step) + 0.25

    def coefficient_scale(self, step):
        return np.array([2.0, 0.5, 4.0])[:self.B] + step

    def outer_iters(self, step):
        return (np.array([3, 4, 5])[:self.B] + step).astype(np.int32)

    def status(self, step):
        return np.array(self.status_by_step.get(step, [0] * self.B), dtype=np.int32)

    def llh(self, step):
        return rows(self.B, 1)[:, 0] * 3.0 + step, -rows(self.B, 1)[:, 0] - 10.0 * step         # rss, sum(log w)

    def hist(self, step):
        """2 + step recorded iterates of member 0"""
        r = 2 + step
        h = dict(x=rows(r, self.n) + 0.5 + 1000.0 * step, rho=rows(r, 3) + 1000.0 * step, weights=rows(r, M) + 1000.0 * step,
                 qp_iterations=np.arange(r + 1, dtype=np.int32))
        if self.desc.dop_size > 0:
            h['dop_rho'] = rows(r, 3) + 0.125 + 1000.0 * step
        return h

    def state(self, s_vectors=True, lean=False):
        k = self.step
        out = dict(fit_x=rows(self.B, NB) * 0.5 + k, R_inf=np.arange(self.B) + 0.1 + k, inductance=np.arange(self.B) + 0.2 + k,
                   coefficient_scale=self.coefficient_scale(k), outer_iters=self.outer_iters(k),
                   qp_iters_total=10 * self.outer_iters(k), status=self.status(k))
        if not lean:
            out.update(x=self.x(k), weights=self.weights(k), rho=rows(self.B, 3) + 0.5 + 1000.0 * k, q_vector=-rows(self.B, self.n) - k)
            if s_vectors:
                out['s_vectors'] = self.s_vectors(k)
        return out

    # the plan's interface
    def set_state(self, **kw):
        self.rec('set_state', **kw)

    def set_weight_factors(self, weight_factor=1.0, row_factors=None, late=False):
        self.rec('set_weight_factors', weight_factor=weight_factor, row_factors=row_factors, late=late)

    def record_history(self, b):
        self.rec('record_history', b=b)

    def continue_fit(self, opts, weight_factor=1.0, min_iter=2):
        self.rec('continue_fit', opts=bytes(opts), weight_factor=weight_factor, min_iter=min_iter)
        self.step += 1

    def download(self, s_vectors=False, lean=False):
        self.rec('download', s_vectors=s_vectors, lean=lean)
        return self.state(s_vectors, lean)

    def get(self, which):
        self.rec('get', which=which)
        return {'dop_rho': rows(self.B, 3) + 0.75 + 1000.0 * self.step}[which]

    def history(self):
        self.rec('history')
        return self.hist(self.step)

    def timings(self):
        self.rec('timings')
        return {'total': 1.0 + self.step}, {'total': 10 + self.step}

    def pfrt_begin(self, max_steps):
        self.rec('pfrt_begin', max_steps=max_steps)

    def pfrt_record(self):
        self.rec('pfrt_record')

    def llh_terms(self, stored=False, weights=None):
        self.rec('llh_terms', stored=stored, weights=weights)
        return self.llh(self.step)

    def p_matrix(self, b):
        self.rec('p_matrix', b=b)
        return np.full((self.n, self.n), float(b))


def prep(cf, ef, num_chrono=NC, num_eis=NF):
    return dict(num_chrono=num_chrono, num_eis=num_eis, m=M, chrono_weight_factor=cf, eis_weight_factor=ef)


def block_rows(*pairs, num_chrono=NC):
    """one row per measurement: its chrono factor on the chrono samples, its eis factor on the rest"""
    return np.array([[cf] * num_chrono + [ef] * (M - num_chrono) for cf, ef in pairs])


def make_drt(ffi, preps=None, batch=None, **plan_kw):
    """a DRT that looks fitted, on an EIS plan (preps None) or on a prepared plan holding ``preps``.  A subclass stands in
    for the three device-bound calls of the PFRT entry points: the full fits and _store_single record themselves on the plan"""
    from hipdrt.models import DRT

    class RecPrepared(RecPlan, ffi.PreparedPlan):
        def __init__(self, **kw):
            RecPlan.__init__(self, **kw)

    class StubDRT(DRT):
        def new_plan(self):
            if preps is None:
                self._plan, self._last_batch = RecPlan(batch=batch or B, **plan_kw), batch or B
            else:
                self._plan = RecPrepared(batch=len(preps), n=NSP + NB, ns=NSP, **plan_kw)
            return self._plan

        def fit_eis_batch(self, frequencies, z_batch, **kw):
            plan = self.new_plan()
            plan.rec('fit_eis_batch', frequencies=frequencies, z_batch=z_batch, kw=kw)
            self.fit_kwargs = dict(kw)
            return plan.state()

        def _fit_prepared(self, measurements, fit_kw, history_of=-1, _init_only=False):
            plan = self.new_plan()
            plan.rec('_fit_prepared', measurements=measurements, fit_kw=fit_kw, history_of=history_of)
            self.fit_kwargs = dict(fit_kw, vz_offset=True, chrono_vmm_epsilon=4, chrono_weight_factor=None, eis_weight_factor=None)
            self._prep = self._last_prepared = None
            assert len(measurements) == len(preps)
            return preps, plan.state(), 'hypers', 'kw', 'ckw'

        def _store_single(self, preps_, out, hypers, kw, ckw, fit_type):
            self._plan.rec('_store_single', preps=preps_, out=out, rest=(hypers, kw, ckw), fit_type=fit_type)
            self._prep, self._last_prepared = preps_[0], None

    drt = StubDRT(warn=False)
    drt.new_plan()
    drt.basis_tau, drt.f_fit = BASIS, F71
    drt.fit_kwargs = dict(s_0=S0_FIT, l2_lambda_0=L2_FIT, nonneg=True)
    if preps is not None:
        # as a prepared fit leaves fit_kwargs: its chrono / hybrid keywords among them.  The eis factor GIVEN TO THE FIT is not
        # what a restart falls back to (that is the fit's chrono factor, kept per measurement)
        drt.fit_kwargs.update(vz_offset=True, chrono_vmm_epsilon=4, chrono_weight_factor=None, eis_weight_factor=7.0)
        drt._prep, drt._last_prepared = None, (preps, None)
    return drt


UNEQUAL = [prep(2.0, 0.5), prep(3.0, 0.25)]
EQUAL = [prep(2.0, 0.5), prep(2.0, 0.5)]


def fit_opts(ffi, s_0=S0_FIT, l2_lambda_0=L2_FIT, xtol=1e-2, max_iter=10, **fields):
    """the FitOpts struct of the documented defaults (drt1d.py:102-137, qphb.py:208-255) with the given values"""
    o = ffi.default_fit_opts()
    vec = dict(derivative_weights=(1.5, 1.0, 0.5), sigma_ds=(1, 1000, 1000), s_alpha=(5, 10, 25), s_0=tuple(s_0),
               rho_alpha=(0.15, 0.2, 0.25), rho_0=(1, 1, 1))
    for name, vals in vec.items():
        for k in range(3):
            getattr(o, name)[k] = float(vals[k])
    scalar = dict(rp_scale=14.0, l1_lambda_0=0.0, l2_lambda_0=float(l2_lambda_0), outlier_p=-1.0, iw_alpha=-1.0, iw_beta=-1.0,
                  iw_l1_lambda_0=1e-4, iw_l2_lambda_0=1e-4, ohmic_penalty=1e-6, inductance_penalty=1e-6, inductance_scale=1e-5,
                  eis_vmm_epsilon=0.25, eis_reim_cor=0.25, xtol=float(xtol), max_iter=int(max_iter), nonneg=1, scale_data=1,
                  fit_ohmic=1, fit_inductance=1, eis_error_uniform=0, update_scale=0, eff_hp=1)
    scalar.update(fields)
    for name, val in scalar.items():
        setattr(o, name, val)
    return o


def same_opts(ffi, got, **fields):
    want = fit_opts(ffi, **fields)
    if got != bytes(want):
        g = ffi.FitOpts.from_buffer_copy(got)
        show = lambda v: list(v) if hasattr(v, '__len__') else v          # noqa: E731
        diff = {n: (show(getattr(g, n)), show(getattr(want, n))) for n, _ in ffi.FitOpts._fields_
                if n != 'qp' and show(getattr(g, n)) != show(getattr(want, n))}
        raise AssertionError(f'fit opts differ (got, expected): {diff}')


# ---- one warm restart per kind ----------------------------------------------------------------------------------------------------
def test_restart_on_an_eis_plan(ffi):
    drt = make_drt(ffi)
    plan = drt._plan
    x, rho, s, w = rows(B, NS + NB), rows(B, 3), rows(B, 3, NS + NB), rows(B, M)
    res = drt.continue_from_init(x_init=x, rho_vector=rho, s_vectors=s, weights=w, weight_factor=1.5, xtol=1e-3, max_iter=7,
                                 min_iter=3, dop_rho_vector=rows(B, 3), s_0=S0_FIT * 4, l2_lambda_0=25.0)
    assert plan.names() == ['set_state', 'record_history', 'continue_fit', 'download', 'timings']     # no set_weight_factors
    st, hi, co, do, _ = (kw for _, kw in plan.calls)
    assert sorted(st) == ['rho', 's', 'weights', 'x']               # dop_rho_vector is accepted and dropped
    assert st['x'] is x and st['rho'] is rho and st['s'] is s and st['weights'] is w
    assert hi == dict(b=-1) and do == dict(s_vectors=True, lean=False)
    assert (co['weight_factor'], co['min_iter']) == (1.5, 3)
    same_opts(ffi, co['opts'], s_0=[4.0, 8.0, 12.0], l2_lambda_0=25.0, xtol=1e-3, max_iter=7)
    # collect_staged() of the state after the restart
    assert sorted(res) == sorted(['fit_x', 'R_inf', 'inductance', 'coefficient_scale', 'outer_iters', 'qp_iters_total', 'status',
                                  'x', 'weights', 'rho', 'q_vector', 's_vectors', 'z_sigma_tot', 'basis_tau', 'timings_ms', 'launches'])
    eq(res['x'], plan.x(1))
    sigma = 1.0 / plan.weights(1)
    eq(res['z_sigma_tot'], (sigma[:, :71] + 1j * sigma[:, 71:]) * plan.coefficient_scale(1)[:, None])
    assert res['basis_tau'] is BASIS and res['timings_ms'] == {'total': 2.0} and res['launches'] == {'total': 11}
    # defaults: the state the device holds, the fit's own hyper-parameters, xtol 1e-2, 10 iterations; history on request
    n0 = len(plan.calls)
    res = drt.continue_from_init(history_of=1)
    assert plan.names(n0) == ['set_state', 'record_history', 'continue_fit', 'download', 'timings', 'history']
    assert plan.calls[n0][1] == dict(x=None, rho=None, s=None, weights=None) and plan.calls[n0 + 1][1] == dict(b=1)
    assert (plan.calls[n0 + 2][1]['weight_factor'], plan.calls[n0 + 2][1]['min_iter']) == (1, 2)
    same_opts(ffi, plan.calls[n0 + 2][1]['opts'])
    eq(res['history']['x'], plan.hist(2)['x'])
    # the lean form of a map
    drt.collect_fields = 'map'
    res = drt.continue_from_init()
    assert plan.all('download')[-1] == dict(s_vectors=False, lean=True)
    assert sorted(res) == sorted(['fit_x', 'R_inf', 'inductance', 'coefficient_scale', 'outer_iters', 'qp_iters_total', 'status',
                                  'basis_tau', 'timings_ms', 'launches'])


@pytest.mark.parametrize("dop_size", [0, 50])
def test_restart_on_a_prepared_plan(ffi, dop_size):
    drt = make_drt(ffi, UNEQUAL, dop_size=dop_size)
    plan = drt._plan
    n = NSP + NB
    x, rho, s, w, dr = rows(2, n), rows(2, 3), rows(2, 3, n), rows(2, M), rows(2, 3) + 0.5
    res = drt.continue_from_init(x_init=x, rho_vector=rho, s_vectors=s, weights=w, dop_rho_vector=dr, weight_factor=1.5,
                                 xtol=1e-3, max_iter=7, min_iter=3, chrono_weight_factor=5.0, eis_weight_factor=6.0,
                                 s_0=S0_FIT * 4, l2_lambda_0=25.0, outlier_p=0.05)
    assert plan.names() == ['set_weight_factors', 'set_state', 'record_history', 'continue_fit', 'download'] + \
        (['get'] if dop_size else []) + ['timings']
    wf, st, hi, co, do = (kw for _, kw in plan.calls[:5])
    assert wf['weight_factor'] == 1.0 and wf['late'] is False
    eq(wf['row_factors'], block_rows((5.0, 6.0), (5.0, 6.0)))
    assert sorted(st) == ['dop_rho', 'rho', 's', 'weights', 'x'] and st['dop_rho'] is dr and st['x'] is x and st['s'] is s
    assert hi == dict(b=-1) and do == dict(s_vectors=True, lean=False)
    assert (co['weight_factor'], co['min_iter']) == (1.5, 3)
    # the chrono / hybrid keywords of fit_kwargs and of the call stop at _split_kwargs; the rest makes the struct
    same_opts(ffi, co['opts'], s_0=[4.0, 8.0, 12.0], l2_lambda_0=25.0, xtol=1e-3, max_iter=7, outlier_p=0.05)
    keys = ['x', 'rho', 'weights', 's_vectors', 'q_vector', 'outer_iters', 'qp_iters_total', 'status', 'timings_ms', 'launches']
    assert sorted(res) == sorted(keys + (['dop_rho'] if dop_size else []))
    eq(res['x'], plan.x(1))
    eq(res['s_vectors'], plan.s_vectors(1))
    if dop_size:
        assert plan.all('get') == [dict(which='dop_rho')]
        eq(res['dop_rho'], rows(2, 3) + 0.75 + 1000.0)
    n0 = len(plan.calls)
    res = drt._continue_prepared(history_of=0)                       # the thin name, the defaults
    assert plan.names(n0)[:4] == ['set_weight_factors', 'set_state', 'record_history', 'continue_fit'] and plan.names(n0)[-1] == 'history'
    assert plan.calls[n0 + 1][1] == dict(x=None, rho=None, s=None, weights=None, dop_rho=None) and plan.calls[n0 + 2][1] == dict(b=0)
    same_opts(ffi, plan.calls[n0 + 3][1]['opts'])
    eq(res['history']['x'], plan.hist(2)['x'])
    assert ('dop_rho' in res['history']) == bool(dop_size)


@pytest.mark.parametrize("given,want", [
    ({}, [(2.0, 2.0), (3.0, 3.0)]),                                        # neither: the fit's CHRONO factor on both blocks
    (dict(chrono_weight_factor=5.0), [(5.0, 2.0), (5.0, 3.0)]),
    (dict(eis_weight_factor=6.0), [(2.0, 6.0), (3.0, 6.0)]),
    (dict(chrono_weight_factor=5.0, eis_weight_factor=6.0), [(5.0, 6.0), (5.0, 6.0)]),
    (dict(chrono_weight_factor=1.0, eis_weight_factor=1.0), None)])
def test_row_factors_of_a_prepared_restart(ffi, given, want):
    drt = make_drt(ffi, UNEQUAL)
    drt.continue_from_init(**given)
    got = drt._plan.all('set_weight_factors')
    assert len(got) == 1 and got[0]['weight_factor'] == 1.0
    if want is None:
        assert got[0]['row_factors'] is None
    else:
        eq(got[0]['row_factors'], block_rows(*want))


def test_row_factors_are_one_outside_joint_measurements(ffi):
    for preps in [prep(2.0, 0.5, num_chrono=M, num_eis=0)] * 2, [prep(2.0, 0.5, num_chrono=0, num_eis=71)] * 2:
        drt = make_drt(ffi, preps)
        drt.continue_from_init(chrono_weight_factor=5.0, eis_weight_factor=6.0)
        assert drt._plan.all('set_weight_factors') == [dict(weight_factor=1.0, row_factors=None, late=False)]
    drt = make_drt(ffi, [prep(1.0, 0.5), prep(1.0, 0.25)])          # joint, the fit's chrono factor 1 and nothing given
    drt.continue_from_init()
    assert drt._plan.all('set_weight_factors')[0]['row_factors'] is None
    drt = make_drt(ffi, [prep(1.0, 0.5), prep(3.0, 0.25)])          # one row per measurement, only one of them all ones
    drt.continue_from_init()
    eq(drt._plan.all('set_weight_factors')[0]['row_factors'], block_rows((1.0, 1.0), (3.0, 3.0)))
    drt = make_drt(ffi, UNEQUAL)                                    # a single fit: its own measurement alone
    drt._last_prepared, drt._prep = None, UNEQUAL[1]
    drt.continue_from_init(eis_weight_factor=6.0)
    eq(drt._plan.all('set_weight_factors')[0]['row_factors'], block_rows((3.0, 6.0)))


def test_refusals(ffi):
    from hipdrt.models import DRT
    needs = 'continue_from_init needs a finished qphb fit'
    with pytest.raises(Exception, match=needs):
        DRT().continue_from_init()                                   # no plan
    drt = make_drt(ffi)
    drt._last_batch = None                                           # an EIS plan that was never fitted
    with pytest.raises(Exception, match=needs):
        drt.continue_from_init()
    drt = make_drt(ffi, UNEQUAL)
    drt._last_prepared = drt._prep = None                            # a prepared plan with neither a batch nor a single fit
    with pytest.raises(Exception, match=needs):
        drt.continue_from_init()
    assert drt._plan.calls == []
    # keywords: an EIS plan hands them straight to _make_opts (the chrono / hybrid ones are unknown there), a prepared plan
    # passes them through _split_kwargs first
    drt = make_drt(ffi)
    for bad in ('bogus', 'chrono_weight_factor', 'vz_offset'):
        with pytest.raises(ValueError, match=f'Invalid keyword argument {bad}'):
            drt.continue_from_init(**{bad: 1.0})
    assert drt._plan.calls == []
    drt = make_drt(ffi, UNEQUAL)
    with pytest.raises(NotImplementedError, match='subtract_background=True is not built'):
        drt.continue_from_init(subtract_background=True)
    with pytest.raises(ValueError, match='Invalid error_structure'):
        drt.continue_from_init(chrono_error_structure='bogus')
    with pytest.raises(ValueError, match='Invalid keyword argument bogus'):
        drt.continue_from_init(bogus=1.0)
    assert drt._plan.calls == []


# ---- candidates ---------------------------------------------------------------------------------------------------------------
def single_fit_state(drt, dop=False):
    """what a single fit keeps on the host and the candidate generators re-read before their first restart"""
    n = drt._plan.n
    drt.qphb_history = [dict(x=np.full(n, 1.0)), dict(x=np.arange(n) + 0.5)]
    drt.qphb_params = dict(rho_vector=np.array([1.5, 2.5, 3.5]), weights=np.arange(M) + 2.0,
                           dop_rho_vector=np.array([4.5, 5.5, 6.5]) if dop else None)
    want = dict(x=(np.arange(n) + 0.5)[None, :], rho=np.array([[1.5, 2.5, 3.5]]), weights=(np.arange(M) + 2.0)[None, :])
    if dop:
        want['dop_rho'] = np.array([[4.5, 5.5, 6.5]])
    return want


def state_is(got, want):
    assert sorted(got) == sorted(want)
    for k in want:
        if want[k] is None:
            assert got[k] is None, k
        else:
            eq(got[k], want[k])


def test_candidates_s0_multiplier_above_one_on_a_single_eis_fit(ffi):
    drt = make_drt(ffi, batch=1)
    plan = drt._plan
    base = single_fit_state(drt)
    steps = drt.generate_candidates_s0(4, 3, xtol=1e-3, max_iter=6, history_of=0)
    per_step = ['set_state', 'record_history', 'continue_fit', 'download', 'timings', 'history']
    assert plan.names() == ['download', 'timings'] + per_step * 3          # the baseline s vectors through the collector, once
    assert len(steps) == 3
    for i, (st, co, hi, res) in enumerate(zip(plan.all('set_state'), plan.all('continue_fit'), plan.all('record_history'), steps), 1):
        # every step: the BASELINE s vectors times 4^i; x / rho / weights of the fit for step 1 only, then what the device holds
        state_is(st, dict(base, s=plan.s_vectors(0) * 4.0 ** i) if i == 1 else dict(x=None, rho=None, weights=None, s=plan.s_vectors(0) * 4.0 ** i))
        same_opts(ffi, co['opts'], s_0=S0_FIT * 4.0 ** i, l2_lambda_0=L2_FIT / 4.0 ** i, xtol=1e-3, max_iter=6)
        assert (co['weight_factor'], co['min_iter']) == (1, 2) and hi == dict(b=0)
        eq(res['x'], plan.x(i))
        eq(res['history']['x'], plan.hist(i)['x'])


def test_candidates_s0_multiplier_below_one_on_a_batch(ffi):
    drt = make_drt(ffi)
    plan = drt._plan
    drt.qphb_params, drt.qphb_history = None, None                       # a batch keeps neither: no baseline
    steps = drt.generate_candidates_s0(0.5, 3)
    assert plan.names() == ['download', 'timings'] + ['set_state', 'record_history', 'continue_fit', 'download', 'timings'] * 3
    for i, (st, co, res) in enumerate(zip(plan.all('set_state'), plan.all('continue_fit'), steps), 1):
        # every step: half of the s vectors its predecessor ended with (step 1: of the fit)
        state_is(st, dict(x=None, rho=None, weights=None, s=plan.s_vectors(i - 1) * 0.5))
        same_opts(ffi, co['opts'], s_0=S0_FIT * 0.5 ** i, l2_lambda_0=L2_FIT / 0.5 ** i)
        eq(res['s_vectors'], plan.s_vectors(i))
    assert plan.all('record_history') == [dict(b=-1)] * 3


def test_candidates_s0_on_a_prepared_plan(ffi):
    drt = make_drt(ffi, UNEQUAL[:1], dop_size=50)
    plan = drt._plan
    drt._last_prepared, drt._prep = None, UNEQUAL[0]
    base = single_fit_state(drt, dop=True)
    drt.generate_candidates_s0(4, 3)
    assert plan.names()[:3] == ['download', 'get', 'timings']            # the same collector, of this kind
    for i, (st, wf) in enumerate(zip(plan.all('set_state'), plan.all('set_weight_factors')), 1):
        s = plan.s_vectors(0) * 4.0 ** i
        state_is(st, dict(base, s=s) if i == 1 else dict(x=None, rho=None, weights=None, dop_rho=None, s=s))
        eq(wf['row_factors'], block_rows((2.0, 2.0)))
    for i, co in enumerate(plan.all('continue_fit'), 1):
        same_opts(ffi, co['opts'], s_0=S0_FIT * 4.0 ** i, l2_lambda_0=L2_FIT / 4.0 ** i)


@pytest.mark.parametrize("kind", ["eis", "prepared"])
def test_candidates_weights(ffi, kind):
    drt = make_drt(ffi, batch=1) if kind == 'eis' else make_drt(ffi, UNEQUAL)
    plan = drt._plan
    base = single_fit_state(drt)                 # (two prepared measurements: a batch, whose baseline is the device's state)
    none = dict(x=None, rho=None, weights=None, s=None, **({} if kind == 'eis' else dict(dop_rho=None)))
    steps = drt.generate_candidates_weights(0.5, 3, xtol=1e-3, max_iter=6, history_of=0)
    assert len(steps) == 3 and len(plan.all('set_weight_factors')) == (0 if kind == 'eis' else 3)
    for i, (st, co, res) in enumerate(zip(plan.all('set_state'), plan.all('continue_fit'), steps), 1):
        state_is(st, dict(base, s=None) if (i == 1 and kind == 'eis') else none)
        assert (co['weight_factor'], co['min_iter']) == (0.5 ** i, 2)
        same_opts(ffi, co['opts'], xtol=1e-3, max_iter=6)              # the fit's own s_0 / l2_lambda_0
        eq(res['x'], plan.x(i))
    assert plan.all('record_history') == [dict(b=0)] * 3


# ---- the PFRT loop ------------------------------------------------------------------------------------------------------------
def step_llh(plan, step):
    """qphb.evaluate_llh with marginalised weights (qphb.py:1355-1377) from the plan's two sums, alpha_0 = 2, beta_0 = 1"""
    from scipy.special import loggamma
    rss, slw = plan.llh(step)
    alpha_n = 2 - 1 + M / 2
    return 2 * np.log(1) - alpha_n * np.log(1 + 0.5 * rss) + loggamma(alpha_n) - loggamma(2) + slw


STATUS = {0: [0, 0, 0], 1: [0, -2, 0], 2: [1, 0, 0]}          # member 1 fails at step 2: that stays; else the last verdict


def check_pfrt_result(plan, pr, batch, extra=()):
    assert list(pr) == ['factors', 'step_x', 'step_llh', 'step_iters', 'status'] + list(extra)
    eq(pr['factors'], FACTORS)
    assert pr['step_x'].shape == (3, batch, plan.n) and pr['step_llh'].shape == (3, batch) and pr['step_iters'].shape == (3, batch)
    eq(pr['step_x'], np.stack([plan.x(k) for k in range(3)]))
    np.testing.assert_allclose(pr['step_llh'], np.stack([step_llh(plan, k) for k in range(3)]), rtol=1e-14, atol=0)
    eq(pr['step_iters'], np.stack([plan.outer_iters(k) for k in range(3)]))
    eq(pr['status'], [1, -2, 0][:batch])


def test_pfrt_loop_on_an_eis_plan(ffi):
    drt = make_drt(ffi, status=STATUS)
    z = rows(B, 71) * (1 + 0.5j)
    seen = []

    def after_init(out):
        drt._plan.rec('after_init')
        seen.append(out)
    pr = drt.pfrt_fit_eis_batch(F71, z, factors=FACTORS, max_iter_per_step=6, max_init_iter=15, xtol=1e-3, nonneg=False,
                                after_init=after_init, s_0=S0_FIT, l2_lambda_0=L2_FIT, eis_vmm_epsilon=0.3)
    plan = drt._plan
    restart = ['set_state', 'record_history', 'continue_fit', 'download', 'timings']
    assert plan.names() == ['fit_eis_batch', 'pfrt_begin', 'pfrt_record', 'llh_terms', 'after_init'] + (restart + ['pfrt_record', 'llh_terms']) * 2
    fit = plan.calls[0][1]
    assert fit['frequencies'] is F71 and fit['z_batch'] is z
    assert sorted(fit['kw']) == ['eis_vmm_epsilon', 'l2_lambda_0', 'max_iter', 'nonneg', 's_0', 'xtol']
    eq(fit['kw']['s_0'], S0_FIT * 0.5)
    assert (fit['kw']['l2_lambda_0'], fit['kw']['max_iter'], fit['kw']['nonneg'], fit['kw']['xtol'], fit['kw']['eis_vmm_epsilon']) == \
        (L2_FIT / 0.5, 15, False, 1e-3, 0.3)
    assert plan.all('pfrt_begin') == [dict(max_steps=3)] and len(plan.all('pfrt_record')) == 3
    assert plan.all('llh_terms') == [dict(stored=False, weights=None)] * 3
    assert len(seen) == 1 and sorted(seen[0]) == sorted(plan.state()) and seen[0]['outer_iters'].tolist() == [3, 4, 5]
    for f, st, co in zip(FACTORS[1:], plan.all('set_state'), plan.all('continue_fit')):
        assert st == dict(x=None, rho=None, s=None, weights=None)
        same_opts(ffi, co['opts'], s_0=S0_FIT * f, l2_lambda_0=L2_FIT / f, xtol=1e-3, max_iter=6, nonneg=0, eis_vmm_epsilon=0.3)
        assert (co['weight_factor'], co['min_iter']) == (1, 2)
    assert plan.all('record_history') == [dict(b=-1)] * 2
    assert pr is drt.pfrt_result
    check_pfrt_result(plan, pr, B, extra=['coefficient_scale', 'basis_tau'])
    eq(pr['coefficient_scale'], plan.coefficient_scale(2))            # of the last step
    assert pr['basis_tau'] is BASIS


def test_pfrt_defaults_on_an_eis_plan(ffi):
    """eleven factors over two decades, the default s_0 = 1 and l2_lambda_0 = 142, 20 iterations first and 10 per step"""
    drt = make_drt(ffi)
    pr = drt.pfrt_fit_eis_batch(F71, rows(B, 71) * (1 + 0.5j))
    plan = drt._plan
    factors = np.logspace(-1, 1, 11)
    eq(pr['factors'], factors)
    assert plan.all('pfrt_begin') == [dict(max_steps=11)] and len(plan.all('pfrt_record')) == 11 and pr['step_x'].shape == (11, B, NS + NB)
    kw = plan.calls[0][1]['kw']
    eq(kw['s_0'], np.ones(3) * factors[0])
    assert (kw['l2_lambda_0'], kw['max_iter'], kw['nonneg'], kw['xtol']) == (142 / factors[0], 20, True, 1e-2)
    for f, co in zip(factors[1:], plan.all('continue_fit')):
        same_opts(ffi, co['opts'], s_0=np.ones(3) * f, l2_lambda_0=142 / f, xtol=1e-2, max_iter=10)
    eq(pr['status'], [0, 0, 0])


@pytest.mark.parametrize("nc,nf,fit_type", [(NC, NF, 'qphb_hybrid'), (M, 0, 'qphb_chrono'), (0, 71, 'qphb_eis')])
def test_pfrt_loop_on_a_single_prepared_measurement(ffi, nc, nf, fit_type):
    preps = [prep(2.0, 0.5, num_chrono=nc, num_eis=nf)]
    drt = make_drt(ffi, preps, dop_size=50 if fit_type == 'qphb_hybrid' else 0, status={k: v[:1] for k, v in STATUS.items()})
    meas = [('t', 'i', 'v', 'f', 'z')]

    def after_init(out):
        drt._plan.rec('after_init', out=out)
    fitted = drt._pfrt_prepared(meas, FACTORS, 6, 15, 1e-3, False, dict(s_0=S0_FIT, l2_lambda_0=L2_FIT, outlier_p=0.05), after_init=after_init)
    plan = drt._plan
    dop = ['get'] if plan.desc.dop_size else []
    restart = ['set_weight_factors', 'set_state', 'record_history', 'continue_fit', 'download'] + dop + ['timings', 'history']
    assert plan.names() == ['_fit_prepared', '_store_single', 'pfrt_begin', 'pfrt_record', 'llh_terms', 'history', 'after_init'] + \
        (restart + ['pfrt_record', 'llh_terms']) * 2
    fit = plan.calls[0][1]
    assert fit['measurements'] is meas and fit['history_of'] == 0
    assert sorted(fit['fit_kw']) == ['l2_lambda_0', 'max_iter', 'nonneg', 'outlier_p', 's_0', 'xtol']
    eq(fit['fit_kw']['s_0'], S0_FIT * 0.5)
    assert (fit['fit_kw']['l2_lambda_0'], fit['fit_kw']['max_iter'], fit['fit_kw']['nonneg'], fit['fit_kw']['xtol']) == (L2_FIT / 0.5, 15, False, 1e-3)
    store = plan.calls[1][1]
    assert store['fit_type'] == fit_type and store['preps'] == preps and store['rest'] == ('hypers', 'kw', 'ckw')
    assert fitted[0] == preps and fitted[1] is store['out'] and fitted[2:] == ('hypers', 'kw', 'ckw')
    assert plan.all('after_init')[0]['out'] is fitted[1]
    assert plan.all('pfrt_begin') == [dict(max_steps=3)] and plan.all('record_history') == [dict(b=0)] * 2
    rf = block_rows((2.0, 0.5), num_chrono=nc) if fit_type == 'qphb_hybrid' else None       # the fit's own two factors
    for f, wf, st, co in zip(FACTORS[1:], plan.all('set_weight_factors'), plan.all('set_state'), plan.all('continue_fit')):
        assert wf['weight_factor'] == 1.0
        assert wf['row_factors'] is None if rf is None else np.array_equal(wf['row_factors'], rf)
        assert st == dict(x=None, rho=None, s=None, weights=None, dop_rho=None)
        same_opts(ffi, co['opts'], s_0=S0_FIT * f, l2_lambda_0=L2_FIT / f, xtol=1e-3, max_iter=6, nonneg=0, outlier_p=0.05)
    check_pfrt_result(plan, drt.pfrt_result, 1)
    # every recorded iterate of the first fit (2), of the first restart (3) and of the second (4)
    hists = [plan.hist(k) for k in range(3)]
    assert len(drt.pfrt_history) == 9
    for row, (h, i) in zip(drt.pfrt_history, [(h, i) for h in hists for i in range(len(h['x']))]):
        assert sorted(row) == ['dop_rho_vector', 'rho_vector', 'weights', 'x']
        eq(row['x'], h['x'][i])
        eq(row['rho_vector'], h['rho'][i])
        eq(row['weights'], h['weights'][i])
        if plan.desc.dop_size:
            eq(row['dop_rho_vector'], h['dop_rho'][i])
        else:
            assert row['dop_rho_vector'] is None
    assert drt._last_prepared is None and drt._prep is preps[0]


def test_pfrt_loop_on_a_prepared_batch(ffi):
    drt = make_drt(ffi, EQUAL, status={k: v[:2] for k, v in STATUS.items()})
    drt.pfrt_history = 'untouched'
    t, f = np.arange(NC) * 1.0, np.logspace(4, -1, NF)
    i_b, v_b, z_b = rows(2, NC), rows(2, NC) + 0.5, rows(2, NF) * (1 + 2j)
    pr = drt.pfrt_fit_hybrid_batch(t, i_b, v_b, f, z_b, factors=FACTORS, max_iter_per_step=6, max_init_iter=15, xtol=1e-3,
                                   s_0=S0_FIT, l2_lambda_0=L2_FIT)
    plan = drt._plan
    restart = ['set_weight_factors', 'set_state', 'record_history', 'continue_fit', 'download', 'timings']
    assert plan.names() == ['_fit_prepared', 'pfrt_begin', 'pfrt_record', 'llh_terms'] + (restart + ['pfrt_record', 'llh_terms']) * 2
    fit = plan.calls[0][1]
    assert fit['history_of'] == -1 and len(fit['measurements']) == 2
    for b, m in enumerate(fit['measurements']):
        assert m[0] is t and m[3] is f
        eq(m[1], i_b[b]), eq(m[2], v_b[b]), eq(m[4], z_b[b])
    assert (fit['fit_kw']['max_iter'], fit['fit_kw']['nonneg'], fit['fit_kw']['xtol']) == (15, True, 1e-3)
    assert plan.all('record_history') == [dict(b=-1)] * 2
    for fac, wf, co in zip(FACTORS[1:], plan.all('set_weight_factors'), plan.all('continue_fit')):
        eq(wf['row_factors'], block_rows((2.0, 0.5), (2.0, 0.5)))      # the fit's own common chrono / eis factors
        same_opts(ffi, co['opts'], s_0=S0_FIT * fac, l2_lambda_0=L2_FIT / fac, xtol=1e-3, max_iter=6)
    assert pr is drt.pfrt_result
    check_pfrt_result(plan, pr, 2)
    assert drt._last_prepared[0] is EQUAL and drt._last_prepared[1] is None and len(drt._last_prepared) == 2
    assert drt.pfrt_history == 'untouched'


def test_pfrt_batch_refuses_unequal_factors_at_the_second_step_only(ffi):
    meas = [('t', 'i', 'v', 'f', 'z')] * 2
    drt = make_drt(ffi, UNEQUAL)
    drt._pfrt_prepared(meas, [0.5], 6, 15, 1e-3, True, {})              # one factor: nothing to restart, nothing to refuse
    assert drt._plan.names() == ['_fit_prepared', 'pfrt_begin', 'pfrt_record', 'llh_terms']
    eq(drt.pfrt_result['step_x'], drt._plan.x(0)[None])
    drt = make_drt(ffi, UNEQUAL)
    with pytest.raises(NotImplementedError, match='per-measurement chrono / eis weight factors in a PFRT batch'):
        drt._pfrt_prepared(meas, [0.5, 1.0], 6, 15, 1e-3, True, {})
    assert drt._plan.names() == ['_fit_prepared', 'pfrt_begin', 'pfrt_record', 'llh_terms']    # after the initial fit
    drt = make_drt(ffi, [prep(2.0, 0.5), prep(2.0, 0.25)])              # the eis factors alone differ
    with pytest.raises(NotImplementedError, match='per-measurement chrono / eis weight factors in a PFRT batch'):
        drt._pfrt_prepared(meas, [0.5, 1.0], 6, 15, 1e-3, True, {})


def test_pfrt_entry_points_of_a_single_measurement(ffi):
    drt = make_drt(ffi, UNEQUAL[:1])
    pr = drt.pfrt_fit_hybrid('t', 'i', 'v', 'f', 'z', factors=FACTORS)
    fit = drt._plan.calls[0][1]
    assert fit['measurements'] == [('t', 'i', 'v', 'f', 'z')] and fit['history_of'] == 0
    assert (fit['fit_kw']['max_iter'], fit['fit_kw']['nonneg'], fit['fit_kw']['xtol'], fit['fit_kw']['l2_lambda_0']) == (20, True, 1e-2, 142 / 0.5)
    assert pr is drt.pfrt_result and drt.fit_type == 'qphb_hybrid' and pr['step_x'].shape == (3, 1, NSP + NB)
    for co in drt._plan.all('continue_fit'):
        assert ffi.FitOpts.from_buffer_copy(co['opts']).max_iter == 10
    drt = make_drt(ffi, [prep(1.0, 1.0, num_chrono=M, num_eis=0)])
    pr = drt.pfrt_fit_chrono('t', 'i', 'v', factors=FACTORS, error_structure=None, vmm_epsilon=2)
    fit = drt._plan.calls[0][1]
    assert fit['measurements'] == [('t', 'i', 'v', None, None)]
    assert (fit['fit_kw']['chrono_error_structure'], fit['fit_kw']['chrono_vmm_epsilon']) == (None, 2)
    assert pr is drt.pfrt_result and drt.fit_type == 'qphb_chrono'


def test_each_rule_has_one_home():
    """the restart layer lives in models/restart.py alone"""
    import re
    src = {name: open(os.path.join(ROOT, "hybrid-drt_amd", "models", name + ".py")).read() for name in ('drt1d', 'prepared', 'restart')}
    for fn in ('continue_from_init', '_candidate_baseline', 'generate_candidates_s0', 'generate_candidates_weights',
               'evaluate_step_llh_batch', 'pfrt_fit_eis_batch', '_pfrt_prepared', 'pfrt_fit_hybrid', 'pfrt_fit_chrono',
               'pfrt_fit_hybrid_batch', 'combine_status', 'step_hypers'):
        homes = [name for name, text in src.items() if re.search(rf'^\s*def {fn}\(', text, re.M)]
        assert homes == ['restart'], (fn, homes)
    kk_plan = src['drt1d'].index('def _kk_plan')
    where = [m.start() for m in re.finditer(r'isinstance\(self\._plan, _ffi\.PreparedPlan\)', src['drt1d'])]
    assert len(where) == 1 and 0 < where[0] - kk_plan < 200
