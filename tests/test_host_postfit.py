"""CPU: the host layer of the DRT post-fit methods (prediction, credible bands, peak finding, per-peak DRTs and resistances, PFRT,
covariance estimates) against a recording stand-in for the device plan: what every method hands to the plan (the option
structs byte for byte, row_scale, want, the log grids), the host-side scaling of what comes back, and the table of refusals.

The library is needed for the defaults of the *_opts structs only; no device is touched.  Every expected option struct is
written here from the rules (search = sign for a nonneg fit and a sign other than 0, else 0; the extend_var clamp indices for
every method but 'thresh'; normalize code 0 / 1 by R_p / 2 by absolute R_p), not read back from the code under test.

Fixed inputs: 3 members, a 91-point basis (1e-7 .. 1e2 s), 71 fit frequencies (1e5 .. 1e-2 Hz), fit_kwargs = {'nonneg': True}.
On get_tau_eval(10) (111 points, 1e-8 .. 1e3 s) the measured range 1 / (2 pi f) = 1.59e-6 .. 15.9 s lies nearest to the points
22 and 92, so the clamp indices are (23, 92)."""
import os

import numpy as np
import pytest

from conftest import ROOT

B, NB, NS = 3, 91, 2
BASIS = np.logspace(-7, 2, NB)
F71 = np.logspace(5, -2, 71)
EXT = (23, 92)
SHORT = np.logspace(-9, -7, 21)          # a grid that ends below the measured range: the left clamp index is len(grid)


@pytest.fixture(scope="module")
def ffi():
    import __graft_entry__ as g
    if not os.path.exists(os.path.join(ROOT, "hybrid-drt_amd", "libhipdrt.so")):
        g.build()
    from hipdrt import _ffi
    _ffi.load_library()
    return _ffi


class FakePlan:
    """what the post-fit layer calls on a plan: every method stores its arguments and returns arrays of the right shape"""

    def __init__(self, copies=1, steps=0):
        self.B = self.batch = self.capacity = B
        self.ns, self.n, self.nb = NS, NS + copies * NB, NB
        self.steps = steps
        self.status = np.zeros(B, dtype=np.int32)
        self.count = np.array([2, 1, 0], dtype=np.int32)
        self.calls = []

    def rec(self, name, **kw):
        self.calls.append((name, kw))

    def last(self, name):
        return next(kw for n, kw in reversed(self.calls) if n == name)

    @staticmethod
    def rows(*shape, shift=0.0):
        """member b holds (b + 1) * (1, 2, 3, ...) + shift: no two members and no two columns alike"""
        a = np.arange(1, int(np.prod(shape[1:])) + 1, dtype=float).reshape(shape[1:])
        return np.stack([(b + 1) * a + shift for b in range(shape[0])])

    def set_tau_basis(self, ln_basis_tau, epsilon):
        self.rec('set_tau_basis', ln=np.array(ln_basis_tau), epsilon=epsilon)

    def get(self, which):
        self.rec('get', which=which)
        return self.rows(B, self.n)

    def predict_drt(self, ln_tau_eval, order=0, sign=1, normalize=0, n_sigma=None):
        self.rec('predict_drt', ln=np.array(ln_tau_eval), order=order, sign=sign, normalize=normalize, n_sigma=n_sigma)
        mu = self.rows(B, len(ln_tau_eval))
        lo, hi = (None, None) if n_sigma is None else (mu - 0.5, mu + 0.25)
        return mu, lo, hi, self.status.copy()

    def find_peaks(self, ln_tau_eval, opts, row_scale=None, want=None):
        self.rec('find_peaks', ln=np.array(ln_tau_eval), opts=bytes(opts), row_scale=row_scale, want=want)
        n = len(ln_tau_eval)
        sign = np.zeros((B, n), dtype=np.int32)
        for b in range(B):
            sign[b, [4 + b, 9, 15]] = 1
        keep = sign.copy()
        keep[:, 9] = 0
        f = self.rows(B, n)
        return dict(peak_sign=sign, keep=keep, heights=f, prominences=f + 0.5, probs=f / 1000, left_bases=keep * 2,
                    right_bases=keep * 3, count=keep.sum(axis=1).astype(np.int32), used_prominence=np.ones(B),
                    peak_prob=f + 7, curv_prob=f + 9, status=self.status.copy())

    def resolve_peaks(self, ln_tau_find, ln_tau_out=None, opts=None, find_opts=None, peak_indices=None, windows=None,
                      row_scale=None, want=None):
        self.rec('resolve_peaks', ln_find=np.array(ln_tau_find), ln_out=None if ln_tau_out is None else np.array(ln_tau_out),
                 opts=bytes(opts), find_opts=None if find_opts is None else bytes(find_opts),
                 peak_indices=None if peak_indices is None else np.array(peak_indices), windows=windows, row_scale=row_scale,
                 want=want)
        mp, nout = opts.max_peaks, 0 if ln_tau_out is None else len(ln_tau_out)
        f = self.rows(B, mp)
        idx = np.tile(np.arange(mp, dtype=np.int32), (B, 1))
        return dict(count=self.count.copy(), status=self.status.copy(), peak_index=idx + 10, trough_index=idx + 20, eps_l=f + 1,
                    eps_r=f + 2, r_peaks=f + 3, r_coef=f + 4, x_peaks=self.rows(B, mp, self.nb), peak_gammas=self.rows(B, mp, nout))

    def integrate_drt(self, ln_tau_eval, windows, order=0, sign=1, normalize=0, row_scale=None):
        self.rec('integrate_drt', ln=np.array(ln_tau_eval), windows=windows, order=order, sign=sign, normalize=normalize,
                 row_scale=row_scale)
        return self.rows(B, len(windows[0])), self.status.copy()

    def predict_resistances(self, absolute=False, r_p_only=False):
        self.rec('predict_resistances', absolute=absolute, r_p_only=r_p_only)
        r_p = np.array([1.0, 2.0, 3.0])
        return (r_p, None, None) if r_p_only else (r_p, r_p + 10, r_p + 20)

    def pfrt_steps(self):
        return self.steps

    def step_p_matrix(self, step, b=0):
        self.rec('step_p_matrix', step=step, b=b)
        return np.full((self.n, self.n), float(step + b))

    def predict_pfrt(self, factors, ln_tau_pfrt, ln_tau_out=None, opts=None, want=None):
        self.rec('predict_pfrt', factors=np.array(factors), ln_pfrt=np.array(ln_tau_pfrt),
                 ln_out=None if ln_tau_out is None else np.array(ln_tau_out), opts=bytes(opts), want=want)
        S, npf = len(factors), len(ln_tau_pfrt)
        nout = npf if ln_tau_out is None else len(ln_tau_out)
        return dict(pfrt=self.rows(B, nout), raw_pfrt=self.rows(B, npf, shift=1), step_pfrt=np.stack([self.rows(B, npf, shift=s) for s in range(S)]),
                    post_prob=np.full((S, B), 1.0 / S), status=self.status.copy())

    @staticmethod
    def var_row(b, n):
        """a variance row with no monotone stretch, so that a clamp from either end changes it"""
        return 2.0 + (1 + b) * np.cos(0.37 * np.arange(n))

    def param_var(self, batch):
        self.rec('param_var', batch=batch)
        return self.rows(batch, self.n), np.zeros(batch, dtype=np.int32)

    def distribution_var(self, basis_eval, batch):
        self.rec('distribution_var', bm=np.array(basis_eval), batch=batch)
        return np.stack([self.var_row(b, basis_eval.shape[0]) for b in range(batch)]), np.zeros(batch, dtype=np.int32)

    def param_cov(self, b=0):
        self.rec('param_cov', b=b)
        return np.full((self.n, self.n), 1.0 + b), True

    def distribution_cov(self, basis_eval, b=0):
        self.rec('distribution_cov', bm=np.array(basis_eval), b=b)
        n = basis_eval.shape[0]
        cov = np.full((n, n), 0.125)
        np.fill_diagonal(cov, self.var_row(b, n))
        return cov, True


SCALES = np.array([2.0, 0.5, 2.0])


def make_drt(ffi, prepared=False, copies=1, steps=0, nonneg=True):
    """a DRT that looks fitted: the stand-in plan, the basis, and either the fit frequencies (plain) or the members' prepared
    measurements, whose coefficient scales differ (prepared; f_fit stays empty so that the clamp can only come from them)"""
    from hipdrt.models import DRT
    drt = DRT(warn=False)
    drt.basis_tau, drt.fit_kwargs = BASIS, {'nonneg': nonneg}
    if prepared:
        class FakePrepared(FakePlan, ffi.PreparedPlan):
            def __init__(self, copies, steps):
                FakePlan.__init__(self, copies, steps)

        pa, pb = (dict(coefficient_scale=cs, frequencies=F71, sample_times=None, nonconsec_step_times=None, dop=None)
                  for cs in (2.0, 0.5))
        drt._plan = FakePrepared(copies, steps)
        drt._prep, drt._last_prepared = pa, ([pa, pb, pa], None)
        drt.special_qp_params = {'R_inf': {'index': 0, 'nonneg': True, 'size': 1}, 'inductance': {'index': 1, 'nonneg': True, 'size': 1}}
    else:
        drt._plan, drt._last_batch, drt.f_fit = FakePlan(copies, steps), B, F71
    if steps:
        drt.pfrt_result = {'factors': np.logspace(-1, 1, steps)}
    return drt


@pytest.fixture(params=[False, True], ids=["plain", "prepared"])
def fitted(request, ffi):
    drt = make_drt(ffi, prepared=request.param)
    return drt, drt._plan, (SCALES if request.param else None)


def same_struct(ffi, kind, got, **fields):
    """the bytes of an option struct against the one the literals give, field by field where they differ"""
    make = {'peak': ffi.peak_opts, 'resolve': ffi.peak_resolve_opts, 'pfrt': ffi.pfrt_opts}[kind]
    cls = {'peak': ffi.PeakOpts, 'resolve': ffi.PeakResolveOpts, 'pfrt': ffi.PfrtOpts}[kind]
    want = make(**fields)
    if got != bytes(want):
        g = cls.from_buffer_copy(got)
        diff = {n: (getattr(g, n), getattr(want, n)) for n, _ in cls._fields_ if repr(getattr(g, n)) != repr(getattr(want, n))}
        raise AssertionError(f'{kind} opts differ (got, expected): {diff}')


def same_scale(got, scales):
    if scales is None:
        assert got is None
    else:
        np.testing.assert_array_equal(got, scales)


def eq(a, b):
    np.testing.assert_array_equal(a, b)


def test_grid_and_clamp_indices(ffi, fitted):
    drt, plan, scales = fitted
    tau = drt.get_tau_eval(10)
    assert len(tau) == 111 and len(drt.get_tau_eval(20)) == 221
    np.testing.assert_allclose(tau[[0, -1]], [1e-8, 1e3], rtol=1e-12)
    assert drt._extend_var_indices(tau) == EXT
    assert drt._extend_var_indices(SHORT) == (len(SHORT), len(SHORT) - 1)
    from hipdrt.models import DRT
    assert DRT.series_neg is False and drt.series_neg is False


# ---- prediction ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kw,code,by_rp", [({}, 0, False), (dict(normalize=True), 1, True), (dict(normalize=True, abs_norm=True), 2, True),
                                           (dict(abs_norm=True), 0, False), (dict(normalize_by=2.5), 0, False),
                                           (dict(normalize=True, normalize_by=2.5, abs_norm=True), 0, False)])
def test_predict_drt_batch(fitted, kw, code, by_rp):
    drt, plan, scales = fitted
    got = drt.predict_drt_batch(order=2, **kw)
    c = plan.last('predict_drt')
    assert (c['order'], c['sign'], c['normalize'], c['n_sigma']) == (2, 1, code, None)
    eq(c['ln'], np.log(drt.get_tau_eval(20)))
    mu = plan.rows(B, 221)
    f = None if (scales is None or by_rp) else scales[:, None]
    if 'normalize_by' in kw:
        f = (1.0 if f is None else f) / 2.5
    eq(got, mu if f is None else mu * f)
    if scales is not None:
        s = plan.last('set_tau_basis')
        eq(s['ln'], np.log(BASIS))
        assert s['epsilon'] == drt.tau_epsilon


def test_predict_drt_ci_batch_and_single_forms(fitted):
    from hipdrt.models import predict
    drt, plan, scales = fitted
    tau = drt.get_tau_eval(10)
    lo, hi, ok = drt.predict_drt_ci_batch(tau=tau, quantiles=(0.1, 0.8))
    c = plan.last('predict_drt')
    assert c['n_sigma'] == predict.n_sigma((0.1, 0.8)) and (c['order'], c['sign'], c['normalize']) == (0, 1, 0)
    eq(c['ln'], np.log(tau))
    mu = plan.rows(B, 111)
    f = 1.0 if scales is None else scales[:, None]
    eq(lo, (mu - 0.5) * f)
    eq(hi, (mu + 0.25) * f)
    assert ok.dtype == bool and ok.all()
    eq(drt.predict_drt(tau=tau, b=1), (mu * f)[1])
    lo1, hi1 = drt.predict_drt_ci(tau=tau, b=2, normalize_by=4.0)
    eq(lo1, ((mu - 0.5) * (f / 4.0))[2])
    eq(hi1, ((mu + 0.25) * (f / 4.0))[2])
    plan.status[1] = -3
    with pytest.warns(UserWarning, match='Singular P matrix'):
        assert drt.predict_drt_ci(tau=tau, b=1) == (None, None)
    assert list(drt.predict_drt_ci_batch(tau=tau)[2]) == [True, False, True]


def test_sign_of_one_and_two_copies(ffi):
    one, two = make_drt(ffi), make_drt(ffi, prepared=True, copies=2)
    for sign, s1, s2 in ((None, 1, 0), (1, 1, 1), (-1, 1, -1), (0, 1, 0)):
        one.predict_drt_batch(sign=sign)
        two.predict_drt_batch(sign=sign)
        assert (one._plan.last('predict_drt')['sign'], two._plan.last('predict_drt')['sign']) == (s1, s2)
    with pytest.raises(ValueError, match='Invalid sign 2'):
        one.predict_drt_batch(sign=2)


def test_resistances(fitted):
    drt, plan, scales = fitted
    r_p = np.array([1.0, 2.0, 3.0])
    if scales is None:
        eq(drt.predict_r_p_batch(absolute=True), r_p)
        assert plan.last('predict_resistances') == dict(absolute=True, r_p_only=False)
        eq(drt.predict_r_inf_batch(), r_p + 10)
        eq(drt.predict_r_tot_batch(), r_p + 20)
        assert drt.predict_r_tot(b=2) == 23.0
    else:
        eq(drt.predict_r_p_batch(absolute=True), r_p * scales)
        assert plan.last('predict_resistances') == dict(absolute=True, r_p_only=True)
        r_inf = plan.rows(B, plan.n)[:, 0] * scales
        eq(drt.predict_r_inf_batch(), r_inf)
        eq(drt.predict_r_tot_batch(), r_inf + r_p * scales)
        assert plan.last('get') == dict(which='x')
        assert drt.predict_r_inf(b=1) == float(r_inf[1])
    assert drt.predict_r_p(b=1) == float((r_p if scales is None else r_p * scales)[1])


# ---- peak finding -------------------------------------------------------------------------------------------------------------
DEFAULT_FIND = dict(eval_sign=1, search=1, normalize=1, method='thresh', height=None, prominence=None, prob_thresh=0.25,
                    num_peaks=None, fxx_var_floor=1e-5, ext_left=-1, ext_right=-1)


@pytest.mark.parametrize("kw,fields,scaled", [
    ({}, {}, False),
    (dict(extend_var=False), {}, False),
    (dict(normalize=False, sign=-1, height=0.02, prominence=0.01, num_peaks=3), dict(normalize=0, search=-1, height=0.02, prominence=0.01, num_peaks=3), True),
    (dict(method='prob'), dict(method='prob', ext_left=23, ext_right=92), False),
    (dict(method='prob', extend_var=False, prob_thresh=0.5, fxx_var_floor=1e-3, sign=0), dict(method='prob', search=0, prob_thresh=0.5, fxx_var_floor=1e-3), False),
    (dict(method='prob', normalize=False), dict(method='prob', normalize=0, ext_left=23, ext_right=92), True)])
def test_find_peaks_batch(ffi, fitted, kw, fields, scaled):
    drt, plan, scales = fitted
    tau = drt.get_tau_eval(10)
    got = drt.find_peaks_batch(**kw)
    c = plan.last('find_peaks')
    same_struct(ffi, 'peak', c['opts'], **dict(DEFAULT_FIND, **fields))
    same_scale(c['row_scale'], scales if scaled else None)
    assert c['want'] == ('keep',)
    eq(c['ln'], np.log(tau))
    assert len(got) == B
    for b in range(B):
        eq(got[b], tau[[4 + b, 15]])
    peak_tau, tau_r, idx, info = drt.find_peaks_batch(return_info=True, **kw)
    assert plan.last('find_peaks')['want'] is None
    eq(tau_r, tau)
    f = plan.rows(B, 111)
    for b in range(B):
        eq(peak_tau[b], tau[[4 + b, 15]])
        eq(idx[b], [4 + b, 15])
        cols = sorted([4 + b, 9, 15])
        assert set(info[b]) == {'peak_heights', 'prominences', 'left_bases', 'right_bases'} | ({'probs'} if kw.get('method') == 'prob' else set())
        eq(info[b]['peak_heights'], f[b, cols])
        eq(info[b]['prominences'], f[b, cols] + 0.5)
        eq(info[b]['left_bases'], [2, 0, 2])
        assert info[b]['right_bases'].dtype == np.intp
    one = drt.find_peaks(b=1, **kw)
    eq(one, tau[[5, 15]])
    assert len(drt.find_peaks(b=2, return_info=True, **kw)) == 4


def test_search_follows_nonneg_and_sign(ffi):
    for prepared in (False, True):
        drt = make_drt(ffi, prepared=prepared, nonneg=False)
        for sign in (1, -1, 0):
            drt.find_peaks_batch(sign=sign)
            same_struct(ffi, 'peak', drt._plan.last('find_peaks')['opts'], **dict(DEFAULT_FIND, search=0))
            drt.estimate_peak_coef_batch(sign=sign)
            same_struct(ffi, 'peak', drt._plan.last('resolve_peaks')['find_opts'], **dict(DEFAULT_FIND, search=0))
        drt = make_drt(ffi, prepared=prepared, copies=2)
        for sign, search in ((1, 1), (-1, -1), (0, 0)):
            drt.find_peaks_batch(sign=sign)
            same_struct(ffi, 'peak', drt._plan.last('find_peaks')['opts'], **dict(DEFAULT_FIND, eval_sign=sign, search=search))
            drt.estimate_peak_coef_batch(sign=sign)
            same_struct(ffi, 'peak', drt._plan.last('resolve_peaks')['find_opts'], **dict(DEFAULT_FIND, eval_sign=sign, search=search))
    drt = make_drt(ffi, steps=11, nonneg=False)
    drt.predict_pfrt_batch()
    same_struct(ffi, 'pfrt', drt._plan.last('predict_pfrt')['opts'], **dict(DEFAULT_PFRT, search=0))


@pytest.mark.parametrize("name,which", [('peak_prob_batch', 'peak_prob'), ('curv_prob_batch', 'curv_prob')])
def test_map_probabilities(ffi, fitted, name, which):
    drt, plan, scales = fitted
    f = plan.rows(B, 111) + (7 if which == 'peak_prob' else 9)
    eq(getattr(drt, name)(), f)
    c = plan.last('find_peaks')
    same_struct(ffi, 'peak', c['opts'], **dict(DEFAULT_FIND, method='map', height=1e-3, prominence=5e-3, fxx_var_floor=0.0,
                                               ext_left=23, ext_right=92))
    assert c['want'] == (which,) and c['row_scale'] is None
    eq(c['ln'], np.log(drt.get_tau_eval(10)))
    getattr(drt, name)(tau=drt.get_tau_eval(20), extend_var=False, prominence=0.1, height=0.2, sign=-1, normalize=False)
    c = plan.last('find_peaks')
    same_struct(ffi, 'peak', c['opts'], **dict(DEFAULT_FIND, method='map', height=0.2, prominence=0.1, fxx_var_floor=0.0,
                                               normalize=0, search=-1))
    same_scale(c['row_scale'], scales)
    eq(c['ln'], np.log(drt.get_tau_eval(20)))


# ---- per-peak coefficients, distributions, resistances ---------------------------------------------------------------------------
DEFAULT_RESOLVE = dict(sign=1, max_peaks=16, epsilon_factor=1.25, max_epsilon=1.25, min_epsilon=None, epsilon_uniform=None)


def cut(plan, a):
    return [a[b, :plan.count[b]] for b in range(B)]


def test_estimate_peak_coef_batch(ffi, fitted):
    drt, plan, scales = fitted
    tau = drt.get_tau_eval(10)
    got = drt.estimate_peak_coef_batch()
    c = plan.last('resolve_peaks')
    same_struct(ffi, 'resolve', c['opts'], **DEFAULT_RESOLVE)
    same_struct(ffi, 'peak', c['find_opts'], **DEFAULT_FIND)
    same_scale(c['row_scale'], scales)
    assert c['want'] == ('x_peaks',) and c['ln_out'] is None and c['peak_indices'] is None and c['windows'] is None
    eq(c['ln_find'], np.log(tau))
    for g, w in zip(got, cut(plan, plan.rows(B, 16, NB))):
        eq(g, w)
    assert got[2].shape == (0, NB)
    # find_peaks' keywords ride along; the clamp indices are those of the find grid
    drt.estimate_peak_coef_batch(tau=drt.get_tau_eval(20), method='prob', normalize=False, height=0.3, epsilon_factor=2.0,
                                 max_epsilon=3.0, min_epsilon=0.5, epsilon_uniform=0.75)
    c = plan.last('resolve_peaks')
    same_struct(ffi, 'resolve', c['opts'], sign=1, max_peaks=16, epsilon_factor=2.0, max_epsilon=3.0, min_epsilon=0.5, epsilon_uniform=0.75)
    same_struct(ffi, 'peak', c['find_opts'], **dict(DEFAULT_FIND, method='prob', normalize=0, height=0.3, ext_left=45, ext_right=184))
    same_scale(c['row_scale'], scales)
    eq(c['ln_find'], np.log(drt.get_tau_eval(20)))
    drt.estimate_peak_coef_batch(method='prob', extend_var=False)
    same_struct(ffi, 'peak', plan.last('resolve_peaks')['find_opts'], **dict(DEFAULT_FIND, method='prob'))
    # given indices: one row for all members, or one row per member, -1 padded to max_peaks
    drt.estimate_peak_coef_batch(tau=tau, peak_indices=[40, 5])
    c = plan.last('resolve_peaks')
    assert c['find_opts'] is None and c['peak_indices'].dtype == np.int32 and c['peak_indices'].shape == (B, 16)
    eq(c['peak_indices'][:, :3], [[5, 40, -1]] * B)
    drt.estimate_peak_coef_batch(tau=tau, peak_indices=[[1], [2, 3], list(range(20))])
    c = plan.last('resolve_peaks')
    same_struct(ffi, 'resolve', c['opts'], **dict(DEFAULT_RESOLVE, max_peaks=20))
    eq(c['peak_indices'][1, :3], [2, 3, -1])
    eq(drt.estimate_peak_coef(b=1), plan.rows(B, 16, NB)[1, :1])
    # the resolve family leaves a clamp index beyond the grid to the library's refusal
    drt.estimate_peak_coef_batch(tau=SHORT, method='prob')
    same_struct(ffi, 'peak', plan.last('resolve_peaks')['find_opts'], **dict(DEFAULT_FIND, method='prob', ext_left=21, ext_right=20))


def test_quantify_peaks_and_peak_drts(ffi, fitted):
    drt, plan, scales = fitted
    tau = drt.get_tau_eval(10)
    f = plan.rows(B, 16)
    got = drt.quantify_peaks_batch()
    c = plan.last('resolve_peaks')
    same_struct(ffi, 'resolve', c['opts'], **DEFAULT_RESOLVE)
    same_struct(ffi, 'peak', c['find_opts'], **DEFAULT_FIND)
    same_scale(c['row_scale'], scales)
    assert c['want'] == ('r_peaks',)
    eq(c['ln_find'], np.log(tau))
    eq(c['ln_out'], np.log(tau))
    for g, w in zip(got, cut(plan, f + 3)):
        eq(g, w)
    r, info = drt.quantify_peaks_batch(tau=drt.get_tau_eval(20), tau_find_peaks=tau, sign=1, return_info=True,
                                       find_peaks_kw=dict(method='prob', prominence=0.2))
    c = plan.last('resolve_peaks')
    same_struct(ffi, 'peak', c['find_opts'], **dict(DEFAULT_FIND, method='prob', prominence=0.2, ext_left=23, ext_right=92))
    assert c['want'] == ('r_peaks', 'peak_index', 'trough_index', 'eps_l', 'eps_r', 'r_coef')
    eq(c['ln_out'], np.log(drt.get_tau_eval(20)))
    assert set(info) == {'peak_index', 'trough_index', 'eps_l', 'eps_r', 'r_coef', 'tau_find_peaks'}
    eq(info['tau_find_peaks'], tau)
    assert [len(t) for t in info['trough_index']] == [1, 0, 0] and [len(t) for t in info['peak_index']] == [2, 1, 0]
    eq(info['r_coef'][0], (f + 4)[0, :2])
    assert drt.quantify_peaks(b=0) == list((f + 3)[0, :2])
    got = drt.estimate_peak_drts_batch(ppd=20)
    c = plan.last('resolve_peaks')
    assert c['want'] == ('peak_gammas',)
    eq(c['ln_out'], np.log(drt.get_tau_eval(20)))
    eq(c['ln_find'], np.log(tau))
    for g, w in zip(got, cut(plan, plan.rows(B, 16, 221))):
        eq(g, w)
    eq(drt.estimate_peak_drts(b=0, ppd=20), got[0])


def test_default_peak_sign_of_a_series_neg_fit(ffi):
    drt = make_drt(ffi, prepared=True, copies=2)
    drt.series_neg = True
    drt.quantify_peaks_batch()
    c = drt._plan.last('resolve_peaks')
    same_struct(ffi, 'resolve', c['opts'], **dict(DEFAULT_RESOLVE, sign=0))
    same_struct(ffi, 'peak', c['find_opts'], **dict(DEFAULT_FIND, eval_sign=0, search=0))
    with pytest.raises(ValueError, match='find_peaks runs with the sign of the peak coefficients'):
        drt.quantify_peaks_batch(find_peaks_kw=dict(sign=1))


@pytest.mark.parametrize("kw,code,by_rp", [({}, 0, False), (dict(normalize=True), 1, True), (dict(normalize=True, abs_norm=True), 2, True),
                                           (dict(normalize_by=2.5, order=1), 0, False),
                                           (dict(normalize=True, normalize_by=2.5), 0, False)])
def test_split_r_p_and_integrate_drt(fitted, kw, code, by_rp):
    from hipdrt.models import peaks
    drt, plan, scales = fitted
    splits = [1e-1, 1e-3]
    got = drt.split_r_p_batch(splits, **kw)
    c = plan.last('integrate_drt')
    tau = drt.get_tau_eval(20)
    ws, we = peaks.split_windows(tau, splits)
    eq(c['ln'], np.log(tau))
    eq(c['windows'][0], ws)
    eq(c['windows'][1], we)
    assert len(ws) == 3
    assert (c['order'], c['sign'], c['normalize']) == (kw.get('order', 0), 1, code)
    same_scale(c['row_scale'], None if by_rp else scales)
    out = plan.rows(B, 3)
    eq(got, out / 2.5 if 'normalize_by' in kw else out)
    eq(drt.split_r_p(splits, b=1, **kw), got[1])
    got = drt.integrate_drt_batch(1e-4, 1e0, ppd=10, **kw)
    c = plan.last('integrate_drt')
    eq(c['ln'], np.log(np.logspace(-4, 0, 41)))
    assert c['windows'] == ([0], [41])
    assert (c['order'], c['sign'], c['normalize']) == (kw.get('order', 0), 1, code)
    same_scale(c['row_scale'], None if by_rp else scales)
    out = plan.rows(B, 1)[:, 0]
    eq(got, out / 2.5 if 'normalize_by' in kw else out)
    assert drt.integrate_drt(1e-4, 1e0, b=2, **kw) == float(got[2])


def test_split_r_p_resolved(ffi, fitted):
    from hipdrt.models import peaks
    drt, plan, scales = fitted
    tau = drt.get_tau_eval(10)
    plan.status[1] = -1
    got = drt.split_r_p_batch([1e-2], resolve_peaks=True, tau=tau)
    c = plan.last('resolve_peaks')
    same_struct(ffi, 'resolve', c['opts'], **DEFAULT_RESOLVE)
    ws, we = peaks.split_windows(tau, [1e-2])
    eq(c['windows'][0], ws)
    eq(c['windows'][1], we)
    assert c['find_opts'] is None and c['peak_indices'] is None and c['ln_out'] is None and c['want'] == ('r_coef',)
    same_scale(c['row_scale'], scales)
    eq(c['ln_find'], np.log(tau))
    want = (plan.rows(B, 16) + 4)[:, :2]
    want[1] = np.nan
    eq(got, want)


# ---- PFRT ---------------------------------------------------------------------------------------------------------------------
DEFAULT_PFRT = dict(eval_sign=1, search=1, height=1e-3, prominence=5e-3, prior_mu=-4, prior_sigma=0.5, n_eff_factor=0.5,
                    fxx_var_floor=1e-5, ext_left=23, ext_right=92, smooth=True, smooth_order=2, smooth_epsilon=5, integrate=False,
                    integrate_threshold=1e-6, normalize=True)


def test_predict_pfrt_batch(ffi):
    drt = make_drt(ffi, steps=11)
    plan = drt._plan
    tau = drt.get_tau_eval(10)
    got = drt.predict_pfrt_batch()
    c = plan.last('predict_pfrt')
    same_struct(ffi, 'pfrt', c['opts'], **DEFAULT_PFRT)
    assert c['want'] == ('pfrt',)
    eq(c['factors'], np.logspace(-1, 1, 11))
    eq(c['ln_pfrt'], np.log(tau))
    eq(c['ln_out'], np.log(tau))
    eq(got, plan.rows(B, 111))
    tau_out = drt.get_tau_eval(20)
    got, info = drt.predict_pfrt_batch(tau=tau_out, sign=-1, prior_mu=-3, prior_sigma=0.25, find_peaks_kw=dict(height=0.1),
                                       n_eff_factor=0.75, fxx_var_floor=1e-4, extend_var=False, smooth_kw=dict(order=1, epsilon=3),
                                       integrate=True, integrate_threshold=1e-5, normalize=False, return_info=True)
    c = plan.last('predict_pfrt')
    # (predict_pfrt searches with the sign it evaluates with, which is 1 for a fit with one copy of the basis whatever was asked;
    #  find_peaks searches with the sign it was given)
    same_struct(ffi, 'pfrt', c['opts'], eval_sign=1, search=1, height=0.1, prominence=0, prior_mu=-3, prior_sigma=0.25,
                n_eff_factor=0.75, fxx_var_floor=1e-4, ext_left=-1, ext_right=-1, smooth=True, smooth_order=1, smooth_epsilon=3,
                integrate=True, integrate_threshold=1e-5, normalize=False)
    assert c['want'] is None
    eq(c['ln_out'], np.log(tau_out))
    eq(got, plan.rows(B, 221))
    assert set(info) == {'tau_pfrt', 'raw_pfrt', 'step_pfrt', 'post_prob', 'status'}
    eq(info['raw_pfrt'], plan.rows(B, 111, shift=1))
    eq(drt.pfrt_result['step_pfrt'], info['step_pfrt'])
    # without smoothing the result stays on tau_pfrt
    drt.predict_pfrt_batch(tau=tau_out, tau_pfrt=drt.get_tau_eval(5), smooth=False)
    c = plan.last('predict_pfrt')
    assert c['ln_out'] is None
    eq(c['ln_pfrt'], np.log(drt.get_tau_eval(5)))
    same_struct(ffi, 'pfrt', c['opts'], **dict(DEFAULT_PFRT, smooth=False, ext_left=12, ext_right=46))
    eq(drt.predict_pfrt(b=1), plan.rows(B, 111)[1])
    eq(drt.pfrt_result['raw_pfrt'], plan.rows(B, 111, shift=1)[1])
    assert drt.pfrt_result['step_pfrt'].shape == (11, 111)
    eq(drt.step_p_matrix(3, b=2), np.full((plan.n, plan.n), 5.0))


# ---- covariance estimates -----------------------------------------------------------------------------------------------------
def clamp(v):
    v = v.copy()
    v[:EXT[0]] = np.maximum(v[:EXT[0]], v[EXT[0]])
    v[EXT[1]:] = np.maximum(v[EXT[1]:], v[EXT[1]])
    return v


def test_covariance_estimates(fitted):
    from hipdrt.matrices import basis
    drt, plan, scales = fitted
    s2 = 1.0 if scales is None else scales ** 2
    var, ok = drt.estimate_param_var_batch()
    assert plan.last('param_var') == dict(batch=B) and ok.all()
    eq(var, plan.rows(B, plan.n) * (s2 if scales is None else s2[:, None]))
    tau = drt.get_tau_eval(10)
    bm = basis.construct_func_eval_matrix(np.log(BASIS), np.log(tau), 'gaussian', epsilon=drt.tau_epsilon, order=0)
    raw = np.stack([plan.var_row(b, 111) for b in range(B)])
    var, ok = drt.estimate_distribution_var_batch(tau=tau)
    c = plan.last('distribution_var')
    eq(c['bm'], bm)
    assert c['batch'] == B and ok.all()
    eq(var, raw * (s2 if scales is None else s2[:, None]))
    assert drt.estimate_distribution_var_batch()[0].shape == (B, 221)
    ext, _ = drt.estimate_distribution_var_batch(tau=tau, extend_var=True)
    for b in range(B):
        cs2 = 1.0 if scales is None else scales[b] ** 2
        want = clamp(raw[b] * cs2)
        assert not np.array_equal(want, raw[b] * cs2)
        eq(ext[b], want)
        cov = drt.estimate_distribution_cov(tau=tau, extend_var=True, b=b)
        c = plan.last('distribution_cov')
        eq(c['bm'], bm)
        assert c['b'] == b
        eq(np.diag(cov), want)
        assert cov[0, 1] == 0.125 * cs2
        eq(np.diag(drt.estimate_distribution_cov(tau=tau, b=b)), raw[b] * cs2)
        floor = drt.estimate_distribution_cov(tau=tau, b=b, var_floor=2.5 * cs2)
        eq(np.diag(floor), np.maximum(raw[b] * cs2, 2.5 * cs2))
        eq(drt.estimate_param_cov(b=b), np.full((plan.n, plan.n), 1.0 + b) * cs2)
        assert plan.last('param_cov') == dict(b=b)


# ---- refusals -----------------------------------------------------------------------------------------------------------------
def refuses(exc, match, call, *a, **kw):
    with pytest.raises(exc, match=match) as ei:
        call(*a, **kw)
    assert type(ei.value) is exc, type(ei.value)


def test_no_fit_is_refused():
    from hipdrt.models import DRT
    drt = DRT()
    tau = np.logspace(-8, 3, 111)
    for call, a, kw in [(drt.predict_drt_batch, (), {}), (drt.predict_drt_ci_batch, (), {}), (drt.predict_z_batch, (), {}),
                        (drt.predict_r_p_batch, (), {}), (drt.predict_r_inf_batch, (), {}), (drt.predict_r_tot_batch, (), {}),
                        (drt.predict_drt, (), {}), (drt.predict_drt_ci, (), {}), (drt.predict_r_p, (), {}), (drt.predict_r_inf, (), {}),
                        (drt.predict_r_tot, (), {}), (drt.find_peaks_batch, (), {}), (drt.find_peaks, (), {}),
                        (drt.peak_prob_batch, (), {}), (drt.curv_prob_batch, (), {}), (drt.estimate_peak_coef_batch, (), {}),
                        (drt.estimate_peak_coef, (), {}), (drt.estimate_peak_drts_batch, (), dict(tau=tau)),
                        (drt.estimate_peak_drts, (), dict(tau=tau)), (drt.quantify_peaks_batch, (), dict(tau=tau)),
                        (drt.quantify_peaks, (), dict(tau=tau)), (drt.split_r_p_batch, ([1e-2],), dict(tau=tau)),
                        (drt.split_r_p, ([1e-2],), dict(tau=tau)), (drt.split_r_p_batch, ([1e-2],), dict(tau=tau, resolve_peaks=True)),
                        (drt.integrate_drt_batch, (1e-4, 1.0), {}), (drt.integrate_drt, (1e-4, 1.0), {})]:
        refuses(RuntimeError, 'needs a finished qphb fit', call, *a, **kw)
    refuses(RuntimeError, 'find_peaks needs a finished qphb fit', drt.find_peaks_batch)
    refuses(RuntimeError, 'quantify_peaks needs a finished qphb fit', drt.quantify_peaks_batch, tau=tau)
    for call, a in [(drt.estimate_distribution_var_batch, ()), (drt.estimate_param_var_batch, ()), (drt.estimate_param_cov, ()),
                    (drt.estimate_distribution_cov, ())]:
        refuses(Exception, 'Parameter covariance estimation is only available for qphb fits', call, *a)
    for call, a in [(drt.predict_pfrt_batch, ()), (drt.predict_pfrt, ()), (drt.step_p_matrix, (0,))]:
        refuses(RuntimeError, 'needs a finished PFRT fit', call, *a)
    # the order of the checks: the request is looked at before the fit
    refuses(ValueError, 'Invalid order 3', drt.predict_drt_batch, order=3)
    refuses(ValueError, 'Invalid order 3', drt.integrate_drt_batch, 1e-4, 1.0, order=3)
    refuses(ValueError, 'normalize_by must be positive', drt.split_r_p_batch, [1e-2], tau=tau, normalize_by=0)
    refuses(NotImplementedError, 'x= override', drt.integrate_drt_batch, 1e-4, 1.0, order=3, x=np.ones(3))
    refuses(TypeError, 'integrate_drt: unexpected keyword quantiles', drt.integrate_drt_batch, 1e-4, 1.0, order=3, quantiles=None)
    refuses(ValueError, 'Invalid method map', drt.find_peaks_batch, method='map', p_matrix=np.eye(2))
    refuses(NotImplementedError, 'peak_tau= argument is not taken', drt.estimate_peak_coef_batch, peak_tau=[1.0])


def test_a_prepared_plan_without_a_batch_is_refused(ffi):
    drt = make_drt(ffi, prepared=True)
    drt._plan.batch = 0
    refuses(RuntimeError, 'predict_drt_batch needs a finished qphb fit', drt.predict_drt_batch)
    refuses(RuntimeError, 'find_peaks needs a finished qphb fit', drt.find_peaks_batch)


def test_request_refusals(ffi, fitted):
    drt, plan, scales = fitted
    tau = drt.get_tau_eval(10)
    x = np.ones(3)
    for call, a in [(drt.predict_drt_batch, ()), (drt.predict_drt_ci_batch, ()), (drt.predict_drt, ()), (drt.predict_drt_ci, ()),
                    (drt.predict_r_p, ()), (drt.estimate_peak_coef_batch, ()), (drt.estimate_peak_drts_batch, ()),
                    (drt.quantify_peaks_batch, ()), (drt.integrate_drt_batch, (1e-4, 1.0)), (drt.split_r_p_batch, ([1e-2],))]:
        refuses(NotImplementedError, 'x= override is not taken', call, *a, x=x)
    refuses(NotImplementedError, 'find_peaks: the x= argument is not taken', drt.find_peaks, x=x)
    refuses(NotImplementedError, "quantify_peaks: find_peaks' p_matrix= argument is not taken", drt.quantify_peaks_batch,
            find_peaks_kw=dict(p_matrix=np.eye(2)))
    for call in (drt.predict_drt_ci_batch, drt.predict_drt_ci):
        refuses(NotImplementedError, 'p_matrix= override is not taken', call, p_matrix=np.eye(2))
    refuses(NotImplementedError, 'find_peaks: the p_matrix= override is not taken', drt.find_peaks_batch, p_matrix=np.eye(2))
    for call in (drt.estimate_peak_coef_batch, drt.estimate_peak_drts_batch, drt.quantify_peaks_batch):
        refuses(NotImplementedError, 'the peak_tau= argument is not taken', call, peak_tau=[1.0])
        refuses(NotImplementedError, 'the trough_tau= argument is not taken', call, trough_tau=[1.0])
    for call in (drt.estimate_peak_drts_batch, drt.quantify_peaks_batch, drt.estimate_peak_drts):
        refuses(NotImplementedError, 'the squeeze_factors= argument is not taken', call, squeeze_factors=[1.0])
    for call, a in [(drt.predict_drt_batch, ()), (drt.predict_drt_ci_batch, ()), (drt.predict_drt, ()),
                    (drt.integrate_drt_batch, (1e-4, 1.0)), (drt.split_r_p_batch, ([1e-2],)),
                    (drt.split_r_p_batch, ([1e-2], True))]:
        refuses(ValueError, 'Invalid order 3. Options: 0, 1, 2', call, *a, order=3)
        refuses(ValueError, 'normalize_by must be positive', call, *a, normalize_by=0.0)
        refuses(ValueError, 'normalize_by must be positive', call, *a, normalize_by=-1.0)
    refuses(TypeError, 'split_r_p: unexpected keyword quantiles', drt.split_r_p_batch, [1e-2], quantiles=(0.1, 0.9))
    for method in ('map', 'nope'):
        refuses(ValueError, f'Invalid method {method}. Options:', drt.find_peaks_batch, method=method)
        refuses(ValueError, f'Invalid method {method}. Options:', drt.estimate_peak_coef_batch, method=method)
        refuses(ValueError, f'Invalid method {method}. Options:', drt.quantify_peaks_batch, find_peaks_kw=dict(method=method))
    refuses(NotImplementedError, 'find_peaks: the width= argument is not taken', drt.find_peaks_batch, width=3)
    refuses(NotImplementedError, 'find_peaks: the width= argument is not taken', drt.estimate_peak_coef_batch, width=3)
    refuses(NotImplementedError, 'find_peaks: the width= argument is not taken', drt.estimate_peak_drts_batch, find_peaks_kw=dict(width=3))
    refuses(ValueError, 'If peak_indices are provided, the corresponding tau grid must also be provided',
            drt.estimate_peak_coef_batch, peak_indices=[3, 4])
    refuses(ValueError, 'quantify_peaks: at most 64 peaks per spectrum', drt.quantify_peaks_batch, tau_find_peaks=tau,
            peak_indices=list(range(65)))
    refuses(ValueError, 'peak_indices must be one row, or one row per spectrum', drt.estimate_peak_coef_batch, tau=tau,
            peak_indices=[[1], [2]])
    refuses(NotImplementedError, r'split_r_p\(resolve_peaks=True\): order, normalize and normalize_by are not taken',
            drt.split_r_p_batch, [1e-2], resolve_peaks=True, normalize=True)
    refuses(NotImplementedError, r'split_r_p\(resolve_peaks=True\)', drt.split_r_p, [1e-2], resolve_peaks=True, normalize_by=2.0)
    refuses(NotImplementedError, r'split_r_p\(resolve_peaks=True\)', drt.split_r_p_batch, [1e-2], resolve_peaks=True, order=1)
    # a clamp index beyond the grid: refused here for find_peaks and the map probabilities ('thresh' takes no clamp)
    beyond = 'extend_var: the measured tau range ends at the last point of the evaluation grid'
    refuses(ValueError, beyond, drt.find_peaks_batch, tau=SHORT, method='prob')
    refuses(ValueError, beyond, drt.find_peaks, tau=SHORT, method='prob')
    refuses(ValueError, beyond, drt.peak_prob_batch, tau=SHORT)
    refuses(ValueError, beyond, drt.curv_prob_batch, tau=SHORT)
    assert len(drt.find_peaks_batch(tau=SHORT)) == B and len(drt.find_peaks_batch(tau=SHORT, method='prob', extend_var=False)) == B
    if scales is None:
        refuses(NotImplementedError, 'predict_z_batch: the x= override is not taken', drt.predict_z_batch, x=x)
    else:
        refuses(NotImplementedError, 'predict_z_batch is built for plain EIS plans', drt.predict_z_batch)


def test_predict_pfrt_refusals(ffi):
    drt = make_drt(ffi, steps=11)
    beyond = 'extend_var: the measured tau range ends at the last point of the evaluation grid'
    refuses(ValueError, beyond, drt.predict_pfrt_batch, tau_pfrt=SHORT)
    refuses(ValueError, beyond, drt.predict_pfrt, tau_pfrt=SHORT)
    assert drt.predict_pfrt_batch(tau_pfrt=SHORT, extend_var=False).shape == (B, len(SHORT))
    refuses(NotImplementedError, 'predict_pfrt: the width= condition of scipy.signal.find_peaks is not built', drt.predict_pfrt_batch,
            find_peaks_kw=dict(width=3))
    refuses(TypeError, r"unexpected smooth_kw \['sigma'\]", drt.predict_pfrt_batch, smooth_kw=dict(sigma=1))
    refuses(ValueError, 'Invalid sign 3', drt.predict_pfrt_batch, sign=3)
    drt.pfrt_result['factors'] = np.logspace(-1, 1, 5)
    refuses(ValueError, r"pfrt_result\['factors'\] has 5 entries, the plan recorded 11 steps", drt.predict_pfrt_batch)
    drt._plan.steps = 0
    refuses(RuntimeError, 'predict_pfrt needs a finished PFRT fit', drt.predict_pfrt_batch)
    refuses(RuntimeError, 'step_p_matrix needs a finished PFRT fit', drt.step_p_matrix, 0)
    prep = make_drt(ffi, prepared=True, steps=11)
    refuses(NotImplementedError, 'predict_pfrt is built for plain EIS fits', prep.predict_pfrt_batch)
    refuses(NotImplementedError, 'predict_pfrt is built for plain EIS fits', prep.predict_pfrt)
    eq(prep.step_p_matrix(2, b=1), np.full((prep._plan.n, prep._plan.n), 3.0))
    prep.series_neg = True                  # (both refusals apply to such a fit: the series_neg one comes first)
    refuses(NotImplementedError, 'predict_pfrt: series_neg fits are not taken', prep.predict_pfrt_batch)
    plain = make_drt(ffi, steps=11)
    plain.series_neg = True
    refuses(NotImplementedError, 'predict_pfrt: series_neg fits are not taken', plain.predict_pfrt)
