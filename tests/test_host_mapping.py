"""CPU: the host bookkeeping of the mapping drivers -- mapping.fit_observations in its shared-grid, observation-list and PFRT
forms, max_batch chunks and batches in flight, fit_observations_sharded at world = 1, the packed rows that travel between
ranks, and the DRTMD store on top of the real driver -- with a stand-in DRT whose "device" results are deterministic functions
of each observation's own data (no GPU, no library call).

Every case compares the FULL triple a driver returns: obs_x, every key of obs_special, every key of res, each with its
container type, dtype, shape and values.  Expected values are written from the observations by the rules below, never by
running the drivers a second way.

An observation carries a tag t; its signature is s = t + 0.25, found in the second sample of its spectrum (of its voltage
signal, without a spectrum).  A first sample of -999 marks an observation on which the solver breaks down (status -1): the
stand-in still returns its usual NON-zero rows for it, so a zero in the result was put there by the driver.  What the
stand-in "fits" for a signature s (dyadic numbers throughout: every product below is exact):

    fit_x = s * (1 .. nb)      R_inf = s + 0.5      inductance = s / 8      v_baseline = (s, -2 s)      x_dop = s / 4 * (1 .. 5)
    status = int(4 s) % 3      outer_iters = 3 + int(4 s) % 5               qp_iters_total = 11 + int(4 s) % 7
    llh = -(s + 1) * f         rss = (s * s + 1) * f     var = (s + 2) * (1 .. len(tau)) * f, valid where s < 6

with f = 1 for a plain fit and f = the regularisation factor of the PFRT step the object currently describes.  EIS fits report
R_inf and inductance, joint fits v_baseline too, chrono-only fits v_baseline, R_inf and x_dop.  The supergrid has 13 points;
EIS and joint fits use its points 2 .. 10 as basis (9 points), chrono-only fits the points 3 .. 10 (8 points)."""
import numpy as np
import pytest

SUP = np.logspace(-5, 1, 13)
BASIS = {'eis': SUP[2:11], 'hybrid': SUP[2:11], 'chrono': SUP[3:11]}
SLOTS = {'eis': (2, 11), 'hybrid': (2, 11), 'chrono': (3, 11)}
LAYOUT = {'eis': (('R_inf', 1), ('inductance', 1)),                                   # leading unknowns of a solution vector
          'hybrid': (('v_baseline', 2), ('R_inf', 1), ('inductance', 1)),
          'chrono': (('v_baseline', 2), ('R_inf', 1), ('x_dop', 5))}
FREQ = np.logspace(3, 0, 6)
TIMES = np.arange(5.0)
IND_SCALE = 0.25
TEXT = "Rank(A) < p or Rank([P; A; G]) < n"


def eis(tag, fail=False):
    z = np.full(len(FREQ), (tag + 0.25) * (1 + 0.5j))
    if fail:
        z[0] = -999.0
    return FREQ, z


def chrono(tag, fail=False):
    v = np.full(len(TIMES), tag + 0.25)
    if fail:
        v[0] = -999.0
    return TIMES, np.ones(len(TIMES)), v


def kind_of(meas):
    return 'hybrid' if meas[0] is not None and meas[3] is not None else 'eis' if meas[3] is not None else 'chrono'


def sig(meas):
    return float(meas[4][1].real if meas[3] is not None else meas[2][1])


def failed(meas):
    return bool(meas[4][0].real == -999.0 if meas[3] is not None else meas[2][0] == -999.0)


def special_value(key, s):
    return {'R_inf': s + 0.5, 'inductance': s / 8, 'v_baseline': np.array([s, -2 * s]),
            'x_dop': s / 4 * np.arange(1.0, 6.0)}[key]


def fit_x_of(s, nb):
    return s * np.arange(1.0, nb + 1)


def status_of(meas):
    return -1 if failed(meas) else int(4 * sig(meas)) % 3


def iters_of(s):
    return 3 + int(4 * s) % 5, 11 + int(4 * s) % 7


def llh_rss_of(s, f=1.0):
    return -(s + 1) * f, (s * s + 1) * f


def var_of(s, n, f=1.0):
    return (s + 2) * np.arange(1.0, n + 1) * f, s < 6


def cscale_of(s):
    return 2.0 if int(4 * s) % 2 else 4.0


def solution_vector(meas):
    """the unknowns of one fit in the order of LAYOUT, then the coefficients"""
    kind, s = kind_of(meas), sig(meas)
    lead = [np.atleast_1d(special_value(key, s)) for key, _ in LAYOUT[kind]]
    return np.concatenate(lead + [fit_x_of(s, len(BASIS[kind]))])


class FakePlan:
    def __init__(self, ns):
        self.ns = ns

    def set_subbatches(self, k):
        pass


class FakeDRT:
    """quacks like hipdrt.models.DRT as far as the mapping drivers go; counts what it is asked"""
    inductance_scale = IND_SCALE
    tau_epsilon = None                    # (no lookup tables to share between ranks)

    def __init__(self):
        self.fits, self.llh_calls, self.var_calls, self.predict_calls, self.outlier_calls = [], [], [], [], []
        self.meas, self.f_now = None, 1.0
        self._plan = None
        self.special_qp_params = {}

    # ---- the fits ----------------------------------------------------------------------------------------------------
    def _begin(self, name, meas, kw):
        self.meas, self.f_now = list(meas), 1.0
        kind = kind_of(meas[0])
        assert all(kind_of(m) == kind for m in meas)
        self.fits.append((name, kind, len(meas), dict(kw)))
        pos, self.special_qp_params = 0, {}
        for key, width in LAYOUT[kind]:
            self.special_qp_params[key] = {'index': pos, 'size': width}
            pos += width
        self._plan = FakePlan(pos)
        return kind

    def _counts(self):
        it = np.array([iters_of(sig(m)) for m in self.meas], dtype=np.int64)
        return dict(status=np.array([status_of(m) for m in self.meas], dtype=np.int64), outer_iters=it[:, 0], qp_iters_total=it[:, 1])

    def _fit_out(self, kind):
        s = [sig(m) for m in self.meas]
        out = {key: np.array([special_value(key, v) for v in s]) for key, _ in LAYOUT[kind]}
        out.update(self._counts(), fit_x=np.array([fit_x_of(v, len(BASIS[kind])) for v in s]),
                   x=np.array([solution_vector(m) for m in self.meas]), basis_tau=BASIS[kind].copy())
        return out

    def fit_eis_batch(self, frequencies, z, **kw):
        kind = self._begin('fit_eis_batch', [(None, None, None, np.asarray(frequencies), zb) for zb in np.asarray(z)], kw)
        return dict(self._fit_out(kind), timings_ms={'qp': 1.0}, launches={'qp': 1})

    def _fit_prepared_batch(self, meas, kw):
        kind = self._begin('_fit_prepared_batch', meas, kw)
        out = self._fit_out(kind)
        out['x_scaled'] = 0.5 * out['x']
        return out

    def _steps(self, factors):
        x = np.array([solution_vector(m) for m in self.meas])
        s = np.array([sig(m) for m in self.meas])
        it = np.array([iters_of(v)[0] for v in s], dtype=np.int64)
        return {'factors': np.asarray(factors), 'step_x': np.array([f * x for f in factors]),
                'step_llh': np.array([-(s + 1) * f for f in factors]), 'step_iters': np.array([it + i for i in range(len(factors))]),
                'status': self._counts()['status']}

    def pfrt_fit_eis_batch(self, frequencies, z_batch, factors=None, after_init=None, **kw):
        self._begin('pfrt_fit_eis_batch', [(None, None, None, np.asarray(frequencies), zb) for zb in np.asarray(z_batch)],
                    dict(kw, factors=np.array(factors)))
        self.f_now = factors[0]
        if after_init is not None:
            after_init(self._counts())
        self.f_now = factors[-1]
        self.pfrt_result = dict(self._steps(factors), coefficient_scale=np.array([cscale_of(sig(m)) for m in self.meas]),
                                basis_tau=BASIS['eis'].copy())
        return self.pfrt_result

    def _pfrt_prepared(self, measurements, factors, max_iter_per_step, max_init_iter, xtol, nonneg, kw, after_init=None):
        self.prepared_kw = dict(kw)
        kind = self._begin('_pfrt_prepared', measurements, dict(kw, factors=np.array(factors), max_iter_per_step=max_iter_per_step,
                                                              max_init_iter=max_init_iter, xtol=xtol, nonneg=nonneg))
        self.f_now = factors[0]
        out = dict(self._counts(), weights=[('weights of', sig(m)) for m in self.meas])
        if after_init is not None:
            after_init(out)
        self.f_now = factors[-1]
        self.pfrt_result = self._steps(factors)
        preps = [dict(basis_tau=BASIS[kind].copy(), kind=kind, sig=sig(m)) for m in self.meas]
        return preps, out, {'hypers': 1}, {'kw2': 1}, {'ckw': 1}

    def _extract(self, prep, x, weights, kw, ckw):
        assert weights == ('weights of', prep['sig']) and kw == {'kw2': 1} and ckw == {'ckw': 1}
        cs, pos, fp = cscale_of(prep['sig']), 0, {'vz_offset_eps': None}
        for key, width in LAYOUT[prep['kind']]:
            fp[key] = x[pos] * cs if width == 1 else x[pos:pos + width] * cs
            pos += width
        fp['x'] = x[pos:] * cs
        return fp

    # ---- what the drivers read after a fit ---------------------------------------------------------------------------
    def evaluate_obs_llh_rss_batch(self, llh_kw=None, rss_kw=None):
        self.llh_calls.append((dict(llh_kw), dict(rss_kw)))
        both = np.array([llh_rss_of(sig(m), self.f_now) for m in self.meas])
        return both[:, 0], both[:, 1]

    def estimate_distribution_var_batch(self, tau=None, extend_var=False):
        self.var_calls.append((np.array(tau), extend_var))
        rows = [var_of(sig(m), len(tau), self.f_now) for m in self.meas]
        return np.array([r[0] for r in rows]), np.array([r[1] for r in rows])

    def predict_pfrt_batch(self, return_info=False, **kw):
        self.predict_calls.append(dict(kw))
        tot = np.array([np.full(len(kw['tau_pfrt']), np.nan) if failed(m) else sig(m) * np.arange(1.0, len(kw['tau_pfrt']) + 1)
                        for m in self.meas])
        return tot, {'raw_pfrt': 2 * tot}

    # ---- the outlier pre-filter: every observation loses its last sample(s) --------------------------------------------
    def _split_kwargs(self, fit_kw):
        return {'ckw of': sorted(fit_kw)}, dict(fit_kw)

    def _remove_outliers_batch(self, measurements, fit_kw, ckw):
        self.outlier_calls.append((len(measurements), dict(fit_kw), ckw))
        cleaned, masks = [], []
        for t, i, v, f, z in measurements:
            cm = None if t is None else np.arange(len(t)) < len(t) - 1
            em = None if f is None else np.arange(len(f)) < len(f) - 1
            cleaned.append((None if t is None else t[cm], None if t is None else i[cm], None if t is None else v[cm],
                            None if f is None else f[em], None if f is None else z[em]))
            masks.append((cm, em))
        return cleaned, (None if measurements[0][0] is None else np.array([0.5, 2.5])), masks


# ---- comparing whole results ---------------------------------------------------------------------------------------------
def same(got, want, where='result'):
    """container type, dtype, shape and values of `got` are those of `want`, all the way down"""
    if isinstance(want, BaseException):
        assert type(got) is type(want) and str(got) == str(want), where
    elif isinstance(want, np.ndarray):
        assert type(got) is np.ndarray and got.dtype == want.dtype and got.shape == want.shape, (where, got, want)
        np.testing.assert_array_equal(got, want, err_msg=where)
    elif isinstance(want, dict):
        assert type(got) is type(want) and set(got) == set(want), (where, sorted(got), sorted(want))
        for key in want:
            same(got[key], want[key], f'{where}[{key!r}]')
    elif isinstance(want, (list, tuple)):
        assert type(got) is type(want) and len(got) == len(want), (where, got, want)
        for j, (g, w) in enumerate(zip(got, want)):
            same(g, w, f'{where}[{j}]')
    else:
        assert type(got) is type(want) and got == want, (where, got, want)


def same_triple(got, want):
    assert type(got) is tuple and len(got) == 3
    for g, w, name in zip(got, want, ('obs_x', 'obs_special', 'res')):
        same(g, w, name)


def as_meas(obs):
    c, e = obs
    c, e = c if c is not None else (None, None, None), e if e is not None else (None, None)
    return c[0], c[1], c[2], e[0], e[1]


def errors_of(meas):
    return [ValueError(TEXT) if failed(m) else None for m in meas]


def counts_of(meas):
    it = np.array([iters_of(sig(m)) for m in meas], dtype=np.int64).reshape(-1, 2)
    return dict(status=np.array([status_of(m) for m in meas], dtype=np.int64), outer_iters=it[:, 0], qp_iters_total=it[:, 1])


# ---- shared grid ---------------------------------------------------------------------------------------------------------
def shared_expected(tags, bad, sup, slots, drt_var):
    """what fit_observations(frequencies, z_obs) returns for EIS observations with these tags, `bad` of them failing"""
    meas = [as_meas((None, eis(t, t in bad))) for t in tags]
    num, (left, right) = len(meas), slots
    ok = np.array([not failed(m) for m in meas])
    s = np.array([sig(m) for m in meas])
    raw_x = np.array([fit_x_of(v, 9) for v in s])
    obs_x = np.zeros((num, len(sup)))
    obs_x[:, left:right] = raw_x * ok[:, None]
    special = {'R_inf': (s + 0.5) * ok, 'inductance': s / 8 * ok}
    res = dict(counts_of(meas), fit_x=raw_x, R_inf=s + 0.5, inductance=s / 8, x=np.array([solution_vector(m) for m in meas]),
               basis_tau=BASIS['eis'].copy(), timings_ms={'qp': 1.0}, launches={'qp': 1},
               obs_fit_status=ok, obs_fit_errors=errors_of(meas), obs_llh=-(s + 1) * ok, obs_rss=(s * s + 1) * ok,
               obs_tau_indices=slots)
    if drt_var:
        vok = ok & (s < 6)
        res['obs_drt_var'] = np.array([var_of(v, len(sup))[0] for v in s]) * vok[:, None]
        res['obs_drt_var_ok'] = vok
    return obs_x, special, res


def z_of(tags, bad=()):
    return np.array([eis(t, t in bad)[1] for t in tags])


METRIC = {'normalize': True, 'weights': 'uniform'}


@pytest.mark.parametrize("drt_var", [False, True])
def test_shared_grid_full_triple_with_a_failed_fit_in_the_middle(drt_var):
    from hipdrt.mapping import drtmd
    tags = [1, 2, 3, 6, 7]
    fake = FakeDRT()
    got = drtmd.fit_observations(fake, FREQ, z_of(tags, bad={3}), tau_supergrid=SUP, drt_var=drt_var, ignore_errors=True, nonneg=True)
    same_triple(got, shared_expected(tags, {3}, SUP, (2, 11), drt_var))
    assert not got[0][2].any() and got[2]['obs_fit_status'].tolist() == [True, True, False, True, True]
    assert [f[0] for f in fake.fits] == ['fit_eis_batch'] and fake.fits[0][2:] == (5, {'nonneg': True})
    assert fake.llh_calls == [(METRIC, METRIC)]
    assert len(fake.var_calls) == int(drt_var)
    if drt_var:
        assert got[2]['obs_drt_var_ok'].tolist() == [True, True, False, False, False]
        np.testing.assert_array_equal(fake.var_calls[0][0], SUP)
        assert fake.var_calls[0][1] is True


def test_shared_grid_without_a_supergrid_uses_the_basis_grid():
    from hipdrt.mapping import drtmd
    tags = [5, 1, 4, 2, 3, 7]
    got = drtmd.fit_observations(FakeDRT(), FREQ, z_of(tags), drt_var=True, llh_kw={'normalize': False}, rss_kw={'weights': None})
    same_triple(got, shared_expected(tags, set(), BASIS['eis'], (0, 9), True))


def test_shared_grid_raises_at_the_first_failure_before_the_llh_is_evaluated(capsys):
    from hipdrt.mapping import drtmd
    fake = FakeDRT()
    with pytest.raises(ValueError) as info:
        drtmd.fit_observations(fake, FREQ, z_of([1, 2, 3, 4, 5], bad={3, 5}), tau_supergrid=SUP, drt_var=True)
    assert str(info.value) == TEXT
    assert len(fake.fits) == 1 and fake.llh_calls == [] and fake.var_calls == []
    assert "Error encountered at obs_index 2\n" in capsys.readouterr().out
    keyed = FakeDRT()
    drtmd.fit_observations(keyed, FREQ, z_of([1]), llh_kw={'normalize': False}, rss_kw={'weights': None})
    assert keyed.llh_calls == [({'normalize': False, 'weights': 'uniform'}, {'normalize': True, 'weights': None})]


# ---- observation list ----------------------------------------------------------------------------------------------------
def mixed_list():
    """EIS (0, 3), joint (1, 4, 6; 4 fails) and chrono-only (2, 5) observations, interleaved"""
    return [(None, eis(1)), (chrono(2), eis(2)), (chrono(3), None), (None, eis(4)), (chrono(5), eis(5, fail=True)),
            ((chrono(6)[0], chrono(6)[1], chrono(6)[2]), (None, None)), (chrono(7), eis(7))]


def list_expected(observations, drt_var, group_order=('eis', 'hybrid', 'chrono'), special_order=('R_inf', 'inductance', 'v_baseline', 'x_dop')):
    meas = [as_meas(o) for o in observations]
    num = len(meas)
    kinds = [kind_of(m) for m in meas]
    obs_x = np.zeros((num, 13))
    widths = {'R_inf': (), 'inductance': (), 'v_baseline': (2,), 'x_dop': (5,)}
    present = {key for k in kinds for key, _ in LAYOUT[k]}
    special = {key: np.zeros((num,) + widths[key]) for key in special_order if key in present}
    res = dict(counts_of(meas), obs_llh=np.zeros(num), obs_rss=np.zeros(num), obs_tau_indices=[SLOTS[k] for k in kinds],
               obs_group=np.array([[g for g in group_order if g in kinds].index(k) for k in kinds]),
               obs_fit_status=np.array([not failed(m) for m in meas]), obs_fit_errors=errors_of(meas), groups=[])
    if drt_var:
        res['obs_drt_var'], res['obs_drt_var_ok'] = np.zeros((num, 13)), np.zeros(num, dtype=bool)
    for k, m in enumerate(meas):
        if failed(m):
            continue
        s, (left, right) = sig(m), SLOTS[kinds[k]]
        obs_x[k, left:right] = fit_x_of(s, right - left)
        for key, _ in LAYOUT[kinds[k]]:
            special[key][k] = special_value(key, s)
        res['obs_llh'][k], res['obs_rss'][k] = llh_rss_of(s)
        if drt_var and s < 6:
            res['obs_drt_var'][k], res['obs_drt_var_ok'][k] = var_of(s, 13)[0], True
    for kind in group_order:
        if kind in kinds:
            res['groups'].append(dict(kind=kind, indices=np.array([k for k in range(num) if kinds[k] == kind]),
                                      basis_tau=BASIS[kind].copy(), tau_indices=SLOTS[kind]))
    return obs_x, special, res


@pytest.mark.parametrize("drt_var", [False, True])
def test_list_form_full_triple_three_groups_two_slices(drt_var):
    from hipdrt.mapping import drtmd
    fake = FakeDRT()
    got = drtmd.fit_observations(fake, observations=mixed_list(), tau_supergrid=SUP, drt_var=drt_var, ignore_errors=True, nonneg=True)
    want = list_expected(mixed_list(), drt_var)
    same_triple(got, want)
    assert list(got[1]) == ['R_inf', 'inductance', 'v_baseline', 'x_dop']              # in order of first appearance
    assert not got[1]['x_dop'][[0, 1, 3, 4, 6]].any() and got[1]['x_dop'][[2, 5]].all()    # reported by the chrono group only
    assert not got[1]['v_baseline'][[0, 3, 4]].any() and not got[1]['inductance'][[2, 4, 5]].any()
    assert not got[0][4].any() and got[2]['obs_group'].tolist() == [0, 1, 2, 0, 1, 2, 1]
    assert [(f[0], f[1], f[2], f[3]) for f in fake.fits] == [('fit_eis_batch', 'eis', 2, {'nonneg': True}),
                                                            ('_fit_prepared_batch', 'hybrid', 3, {'nonneg': True}),
                                                            ('_fit_prepared_batch', 'chrono', 2, {'nonneg': True})]
    assert fake.llh_calls == [(METRIC, METRIC)] * 3 and len(fake.var_calls) == 3 * int(drt_var)


def test_list_form_raises_only_after_every_group_was_fitted(capsys):
    from hipdrt.mapping import drtmd
    fake = FakeDRT()
    with pytest.raises(ValueError) as info:
        drtmd.fit_observations(fake, observations=mixed_list(), tau_supergrid=SUP, drt_var=True)
    assert str(info.value) == TEXT
    assert len(fake.fits) == 3 and len(fake.llh_calls) == 3 and len(fake.var_calls) == 3
    assert "Error encountered at obs_index 4\n" in capsys.readouterr().out
    with pytest.raises(ValueError, match="tau_supergrid"):
        drtmd.fit_observations(fake, observations=mixed_list())


def test_list_form_step_times_of_the_prefilter_reach_the_groups_keywords():
    from hipdrt.mapping import drtmd
    fake = FakeDRT()
    obs = [(chrono(2), eis(2)), (None, eis(1)), (chrono(5), eis(5))]
    got = drtmd.fit_observations(fake, observations=obs, tau_supergrid=SUP, ignore_errors=True, nonneg=True, remove_outliers=True,
                                 outlier_p=0.05, outlier_thresh=0.75)
    # the signature sits in the second sample, which the stand-in's filter keeps: same results as without it
    same_triple(got, list_expected(obs, False, group_order=('hybrid', 'eis'), special_order=('v_baseline', 'R_inf', 'inductance')))
    assert [c[0] for c in fake.outlier_calls] == [2, 1]
    assert all(c[1]['remove_outliers'] is True and c[1]['remove_extremes'] is False and c[1]['outlier_p'] == 0.05
               for c in fake.outlier_calls)
    (_, kind0, n0, kw0), (_, kind1, n1, kw1) = fake.fits
    assert (kind0, n0, kind1, n1) == ('hybrid', 2, 'eis', 1)
    assert sorted(kw0) == ['nonneg', 'outlier_p', 'step_sizes', 'step_times']
    np.testing.assert_array_equal(kw0['step_times'], [0.5, 2.5])
    assert kw0['step_sizes'] is None and kw0['outlier_p'] is None and kw1 == {'nonneg': True, 'outlier_p': None}
    assert [len(m[3]) for m in fake.meas] == [5]                       # every observation lost its last sample before the fit


# ---- PFRT ------------------------------------------------------------------------------------------------------------------
FACTORS = np.array([0.5, 1.0, 2.0])


def pfrt_list():
    """an EIS group (0, 2, 3; 2 fails) and a joint group (1, 4)"""
    return [(None, eis(1)), (chrono(2), eis(2)), (None, eis(3, fail=True)), (None, eis(6)), (chrono(7), eis(7))]


def pfrt_expected(observations, factors, drt_var, predict):
    meas = [as_meas(o) for o in observations]
    num, S = len(meas), len(factors)
    kinds = [kind_of(m) for m in meas]
    s = np.array([sig(m) for m in meas])
    ok = np.array([not failed(m) for m in meas])
    obs_x = np.zeros((num, S, 13))
    special = {'R_inf': np.zeros((num, S)), 'inductance': np.zeros((num, S))}
    if 'hybrid' in kinds:
        special['v_baseline'] = np.zeros((num, S, 2))
    it = np.array([iters_of(v)[0] for v in s], dtype=np.int64)
    res = dict(obs_llh=-(s + 1) * factors[0] * ok, obs_rss=(s * s + 1) * factors[0] * ok, obs_tau_indices=[SLOTS[k] for k in kinds],
               obs_group=np.array([('eis', 'hybrid').index(k) for k in kinds]), obs_fit_status=ok, obs_fit_errors=errors_of(meas),
               status=np.array([status_of(m) for m in meas], dtype=np.int64),
               step_llh=np.outer(-(s + 1), factors), step_iters=it[:, None] + np.arange(S)[None, :], pfrt_factors=factors, groups=[])
    for k, m in enumerate(meas):
        if not ok[k]:
            continue
        cs = cscale_of(s[k])
        for i, f in enumerate(factors):
            obs_x[k, i, 2:11] = f * fit_x_of(s[k], 9) * cs
            special['R_inf'][k, i] = f * (s[k] + 0.5) * cs
            # the joint fit's _extract hands the inductance back in data units, the EIS path scales it here
            special['inductance'][k, i] = f * (s[k] / 8) * cs * (IND_SCALE if kinds[k] == 'eis' else 1.0)
            if kinds[k] == 'hybrid':
                special['v_baseline'][k, i] = f * np.array([s[k], -2 * s[k]]) * cs
    if drt_var:
        vok = ok & (s < 6)
        one = np.array([var_of(v, 13, factors[0])[0] for v in s]) * vok[:, None]
        res['obs_drt_var'], res['obs_drt_var_ok'] = np.repeat(one[:, None, :], S, axis=1), vok
    if predict:
        res['obs_pfrt'] = np.array([s[k] * np.arange(1.0, 14.0) if ok[k] and kinds[k] == 'eis' else np.full(13, np.nan) for k in range(num)])
        res['obs_raw_pfrt'] = 2 * res['obs_pfrt']
    for kind in ('eis', 'hybrid'):
        if kind in kinds:
            res['groups'].append(dict(kind=kind, indices=np.array([k for k in range(num) if kinds[k] == kind]),
                                      basis_tau=BASIS[kind].copy(), tau_indices=SLOTS[kind]))
    return obs_x, special, res


@pytest.mark.parametrize("drt_var,predict", [(False, False), (True, False), (True, True)])
def test_pfrt_form_full_triple(drt_var, predict):
    from hipdrt.mapping import drtmd
    fake = FakeDRT()
    got = drtmd.fit_observations(fake, observations=pfrt_list(), tau_supergrid=SUP, fit_type='pfrt', pfrt_factors=FACTORS,
                                 drt_var=drt_var, ignore_errors=True, predict_pfrt_kw={} if predict else None,
                                 nonneg=False, max_iter_per_step=7, max_init_iter=13, xtol=0.125, l2_lambda_0=3.0)
    same_triple(got, pfrt_expected(pfrt_list(), FACTORS, drt_var, predict))
    assert got[0].shape == (5, 3, 13) and got[1]['R_inf'].shape == (5, 3) and got[1]['v_baseline'].shape == (5, 3, 2)
    assert ('obs_pfrt' in got[2]) == predict and not got[0][2].any()
    # the four PFRT controls leave the fit keywords: named arguments of the fit, absent from what the prepared fit gets as `kw`
    (n0, k0, b0, kw0), (n1, k1, b1, kw1) = fake.fits
    assert (n0, k0, b0, n1, k1, b1) == ('pfrt_fit_eis_batch', 'eis', 3, '_pfrt_prepared', 'hybrid', 2)
    for kw in (kw0, kw1):
        np.testing.assert_array_equal(kw.pop('factors'), FACTORS)
        assert kw == dict(nonneg=False, max_iter_per_step=7, max_init_iter=13, xtol=0.125, l2_lambda_0=3.0)
    assert fake.prepared_kw == {'l2_lambda_0': 3.0}
    # llh / rss / variance were taken inside after_init: once per group, while the object described the first step
    assert fake.llh_calls == [(METRIC, METRIC)] * 2 and len(fake.var_calls) == 2 * int(drt_var)
    assert len(fake.predict_calls) == int(predict)
    if predict:
        assert sorted(fake.predict_calls[0]) == ['tau', 'tau_pfrt']
        np.testing.assert_array_equal(fake.predict_calls[0]['tau'], SUP)
        assert np.isnan(got[2]['obs_pfrt'][[1, 2, 4]]).all() and np.isfinite(got[2]['obs_pfrt'][[0, 3]]).all()


def test_pfrt_factors_defaults_and_checks(capsys):
    from hipdrt.mapping import drtmd
    obs = pfrt_list()[:2]
    # `factors=` among the fit keywords wins over pfrt_factors
    got = drtmd.fit_observations_pfrt(FakeDRT(), obs, SUP, pfrt_factors=np.array([4.0, 8.0]), factors=FACTORS)
    same_triple(got, pfrt_expected(obs, FACTORS, False, False))
    # neither given: logspace(-1, 1, 11); the prepared fit then gets its own defaults for the four controls
    fake = FakeDRT()
    got = drtmd.fit_observations_pfrt(fake, obs, SUP, drt_var=True)
    same_triple(got, pfrt_expected(obs, np.logspace(-1, 1, 11), True, False))
    np.testing.assert_array_equal(fake.fits[1][3].pop('factors'), np.logspace(-1, 1, 11))
    assert fake.fits[1][3] == dict(max_iter_per_step=10, max_init_iter=20, xtol=1e-2, nonneg=True) and fake.prepared_kw == {}
    # the shared-grid call form makes a list of EIS observations
    class Gridded(FakeDRT):
        fixed_basis_tau, tau_supergrid = None, SUP
    got = drtmd.fit_observations(Gridded(), FREQ, z_of([1, 3]), fit_type='pfrt', pfrt_factors=FACTORS)
    same_triple(got, pfrt_expected([(None, eis(1)), (None, eis(3))], FACTORS, False, False))
    for bad in ({'tau': SUP[:5]}, {'tau_pfrt': SUP[:5]}, {'tau': SUP, 'tau_pfrt': SUP[:12]}):
        with pytest.raises(ValueError, match="predict_pfrt_kw"):
            drtmd.fit_observations_pfrt(FakeDRT(), obs, SUP, predict_pfrt_kw=bad)
    with pytest.raises(ValueError) as info:
        drtmd.fit_observations_pfrt(FakeDRT(), pfrt_list(), SUP, pfrt_factors=FACTORS)
    assert str(info.value) == TEXT and "Error encountered at obs_index 2\n" in capsys.readouterr().out
    with pytest.raises(ValueError, match="fit_type"):
        drtmd.fit_observations(FakeDRT(), FREQ, z_of([1]), fit_type='nope')


# ---- chunks, batches in flight -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["max_batch", "inflight"])
def test_chunked_map_equals_the_one_batch_map_in_every_returned_object(monkeypatch, how):
    from hipdrt.mapping import drtmd
    tags = [3, 1, 4, 1, 5, 2, 6]
    z = z_of(tags)
    z[5, 0] = -999.0                                               # falls into the last of three chunks (3 + 2 + 2)
    one = drtmd.fit_observations(FakeDRT(), FREQ, z, tau_supergrid=SUP, drt_var=True, ignore_errors=True)
    want = shared_expected(tags, {2}, SUP, (2, 11), True)
    same_triple(one, want)
    fakes = [FakeDRT() for _ in range(3)]
    monkeypatch.setattr(drtmd, "drt_siblings", lambda drt, count: fakes[:count])
    kw = dict(max_batch=3) if how == "max_batch" else dict(inflight=3)
    many = drtmd.fit_observations(fakes[0], FREQ, z, tau_supergrid=SUP, drt_var=True, ignore_errors=True, **kw)
    same_triple(many, want)
    sizes = [f[2] for fake in fakes for f in fake.fits]
    assert sizes == [3, 2, 2] and (len(fakes[1].fits) == 1) == (how == "inflight")
    with pytest.raises(ValueError) as info:
        drtmd.fit_observations(fakes[0], FREQ, z, tau_supergrid=SUP, drt_var=True, **kw)
    assert str(info.value) == TEXT


# ---- the sharded driver at world = 1 ---------------------------------------------------------------------------------------
DOCUMENTED = ('obs_llh', 'obs_rss', 'outer_iters', 'qp_iters_total', 'status', 'obs_tau_indices', 'obs_fit_status', 'obs_fit_errors')


@pytest.mark.parametrize("drt_var", [False, True])
def test_sharded_world_one_shared_grid_equals_the_direct_call(drt_var):
    from hipdrt.mapping import drtmd
    tags = [1, 2, 3, 6, 7]
    z = z_of(tags, bad={3})
    x, special, res = shared_expected(tags, {3}, SUP, (2, 11), drt_var)
    keep = DOCUMENTED + (('obs_drt_var', 'obs_drt_var_ok') if drt_var else ())
    want = (x, special, dict({k: res[k] for k in keep}, obs_tau_indices=[(2, 11)] * 5))
    fake = FakeDRT()
    got = drtmd.fit_observations_sharded(fake, FREQ, z, rank=0, world=1, tau_supergrid=SUP, drt_var=drt_var, ignore_errors=True,
                                         fit=drtmd.fit_observations, nonneg=True)
    same_triple(got, want)
    assert all(type(v) is int for pair in got[2]['obs_tau_indices'] for v in pair)
    assert got[2]['status'].dtype == got[2]['outer_iters'].dtype == got[2]['qp_iters_total'].dtype == np.int64
    assert got[2]['obs_llh'].dtype == got[2]['obs_rss'].dtype == np.float64
    assert fake.fits[0][3] == {'nonneg': True} and getattr(fake, 'collect_fields', None) is None
    for scheme in ('block', 'lpt'):
        same_triple(drtmd.fit_observations_sharded(FakeDRT(), FREQ, z, rank=0, world=1, tau_supergrid=SUP, drt_var=drt_var,
                                                   ignore_errors=True, scheme=scheme, fit=drtmd.fit_observations, nonneg=True), want)
    with pytest.raises(ValueError) as info:              # every rank fits with ignore_errors; the failure raises after the gather
        drtmd.fit_observations_sharded(FakeDRT(), FREQ, z, rank=0, world=1, tau_supergrid=SUP, drt_var=drt_var, fit=drtmd.fit_observations)
    assert str(info.value) == TEXT
    assert drtmd.fit_observations_sharded(FakeDRT(), FREQ, z, rank=1, world=2, tau_supergrid=SUP, drt_var=drt_var, ignore_errors=True,
                                          fit=drtmd.fit_observations) is None          # (no group: the gather is the identity)


@pytest.mark.parametrize("drt_var", [False, True])
def test_sharded_world_one_list_form_equals_the_direct_call(drt_var):
    from hipdrt.mapping import drtmd
    x, special, res = list_expected(mixed_list(), drt_var)
    keep = DOCUMENTED + (('obs_drt_var', 'obs_drt_var_ok') if drt_var else ())
    got = drtmd.fit_observations_sharded(FakeDRT(), observations=mixed_list(), rank=0, world=1, tau_supergrid=SUP, drt_var=drt_var,
                                         ignore_errors=True, fit=drtmd.fit_observations, nonneg=True)
    same_triple(got, (x, special, {k: res[k] for k in keep}))
    assert list(got[1]) == ['v_baseline', 'R_inf', 'inductance', 'x_dop']               # the order of the rows' registry
    assert all(type(v) is int for pair in got[2]['obs_tau_indices'] for v in pair)
    with pytest.raises(ValueError, match="lpt"):
        drtmd.fit_observations_sharded(FakeDRT(), observations=mixed_list(), rank=0, world=1, tau_supergrid=SUP, scheme='lpt')


# ---- the rows that travel between ranks -----------------------------------------------------------------------------------
def block_of(num, nsup, specials, drt_var, slots):
    rng = np.random.default_rng(num + nsup)
    shapes = {'v_baseline': (num, 2), 'vz_offset': (num,), 'R_inf': (num,), 'inductance': (num,), 'C_inv': (num,), 'x_dop': (num, 5)}
    obs_special = {key: rng.standard_normal(shapes[key]) for key in specials}
    res = dict(obs_llh=rng.standard_normal(num), obs_rss=rng.standard_normal(num) ** 2, outer_iters=rng.integers(1, 50, num),
               qp_iters_total=rng.integers(1, 900, num), status=rng.integers(-1, 3, num), obs_tau_indices=slots)
    if drt_var:
        res['obs_drt_var'], res['obs_drt_var_ok'] = rng.standard_normal((num, nsup)) ** 2, rng.integers(0, 2, num).astype(bool)
    return rng.standard_normal((num, nsup)), obs_special, res


def check_unpacked(unpacked, obs_x, obs_special, res, drt_var, slots):
    ux, uspecial, ucols, uti, uvar, uvok = unpacked
    np.testing.assert_array_equal(ux, obs_x)
    assert set(uspecial) == set(obs_special)
    for key, val in obs_special.items():
        np.testing.assert_array_equal(uspecial[key][0], val.reshape(len(obs_x), -1))
        assert uspecial[key][1] == val.ndim
    assert list(ucols) == ['obs_llh', 'obs_rss', 'outer_iters', 'qp_iters_total', 'status']
    for key in ucols:
        np.testing.assert_array_equal(ucols[key], res[key])
    np.testing.assert_array_equal(uti, np.broadcast_to(np.array(slots, dtype=float).reshape(-1, 2), (len(obs_x), 2)))
    if drt_var:
        np.testing.assert_array_equal(uvar, res['obs_drt_var'])
        np.testing.assert_array_equal(uvok, res['obs_drt_var_ok'])
    else:
        assert uvar is None and uvok is None


def test_packed_rows_header_is_the_wire_format_and_round_trips():
    from hipdrt.mapping import drtmd
    # no specials, one (left, right) for the whole block: 4 + 5 + 2 columns under a header of three numbers
    obs_x, obs_special, res = block_of(3, 4, (), False, (1, 4))
    packed = drtmd._pack_rows(obs_x, obs_special, res, False)
    assert packed.shape == (4, 11) and packed.dtype == np.float64
    assert packed[0].tolist() == [4.0, 0.0, 0.0] + [0.0] * 8
    assert packed[1].tolist() == obs_x[0].tolist() + [res[k][0] for k in ('obs_llh', 'obs_rss', 'outer_iters', 'qp_iters_total', 'status')] + [1.0, 4.0]
    check_unpacked(drtmd._unpack_block(packed), obs_x, obs_special, res, False, (1, 4))
    # all six registry specials handed over in another order, at widths 2, 1, 1, 1, 1, 5; variance rows; per-row slots
    order = ('x_dop', 'R_inf', 'C_inv', 'v_baseline', 'inductance', 'vz_offset')
    slots = [(0, 9), (2, 11), (3, 11), (2, 11)]
    obs_x, obs_special, res = block_of(4, 13, order, True, slots)
    packed = drtmd._pack_rows(obs_x, obs_special, res, True)
    assert packed.shape == (5, 13 + 11 + 5 + 2 + 13 + 1)
    assert packed[0].tolist() == [13.0, 1.0, 6.0, 0.0, 2.0, 2.0, 1.0, 1.0, 1.0, 2.0, 1.0, 1.0, 3.0, 1.0, 1.0, 4.0, 1.0, 1.0,
                                  5.0, 5.0, 2.0] + [0.0] * (45 - 21)
    check_unpacked(drtmd._unpack_block(packed), obs_x, obs_special, res, True, slots)
    # rows padded to another rank's wider row unpack to the same
    check_unpacked(drtmd._unpack_block(np.pad(packed, ((0, 0), (0, 7)))), obs_x, obs_special, res, True, slots)
    # a header longer than the rows it describes sets the width; no obs_tau_indices = the whole grid
    obs_x, obs_special, res = block_of(2, 1, order, False, (0, 1))
    del res['obs_tau_indices']
    packed = drtmd._pack_rows(obs_x, obs_special, res, False)
    assert packed.shape == (3, 21) and packed[0, :3].tolist() == [1.0, 0.0, 6.0]
    check_unpacked(drtmd._unpack_block(packed), obs_x, obs_special, res, False, (0, 1))
    # a key whose value is None is not sent; an unknown one is refused
    obs_x, obs_special, res = block_of(3, 4, ('R_inf',), False, (1, 4))
    packed = drtmd._pack_rows(obs_x, dict(obs_special, inductance=None), res, False)
    assert packed[0].tolist() == [4.0, 0.0, 1.0, 2.0, 1.0, 1.0] + [0.0] * 6
    with pytest.raises(NotImplementedError, match="x_new"):
        drtmd._pack_rows(obs_x, dict(obs_special, x_new=np.zeros(3)), res, False)


# ---- the store on top of the real driver -----------------------------------------------------------------------------------
def test_store_on_the_real_driver(capsys):
    from hipdrt.mapping import store
    fake = FakeDRT()
    md = store.DRTMD(SUP, drt=fake, drt_var=True)
    assert md.llh_kw == METRIC and md.rss_kw == METRIC and md.llh_kw is not md.rss_kw
    assert store.DRTMD(SUP, drt=fake, llh_kw={'normalize': False}).llh_kw == {'normalize': False, 'weights': 'uniform'}
    first = [(None, eis(1)), (None, eis(2, fail=True)), (None, eis(3))]
    for k, (c, e) in enumerate(first):
        md.add_observation([k], c, e)
    with pytest.raises(ValueError) as info:                        # the reference's serial loop: 0 is stored, 1 raises, 2 stays unfitted
        md.fit_all()
    assert str(info.value) == TEXT and "Error encountered at obs_index 1\n" in capsys.readouterr().out
    assert md.obs_fit_status.tolist() == [True, False, False] and not md.obs_ignore_flag.any() and md.obs_fit_errors == [None] * 3
    assert md.obs_tau_indices == [(2, 11), None, None] and list(md.obs_special) == ['R_inf', 'inductance']
    assert md.fit_all(ignore_errors=True).tolist() == [1, 2]
    assert md.obs_fit_status.tolist() == [True, False, True] and md.obs_ignore_flag.tolist() == [False, True, False]
    same(md.obs_fit_errors, [None, ValueError(TEXT), None])
    # a special that only a later call reports: zeros for everyone stored before
    later = [(chrono(4), eis(4)), (chrono(5), None)]
    for k, (c, e) in enumerate(later):
        md.add_observation([3 + k], c, e)
    assert md.fit_all().tolist() == [3, 4] and md.last_fit_index.tolist() == [3, 4]
    want_x, want_special, want = list_expected(first + later, True, special_order=('R_inf', 'inductance', 'v_baseline', 'x_dop'))
    same(md.obs_x, want_x)
    same(md.obs_special, want_special)
    assert list(md.obs_special) == ['R_inf', 'inductance', 'v_baseline', 'x_dop']
    same(md.obs_llh, want['obs_llh'])
    same(md.obs_rss, want['obs_rss'])
    same(md.obs_drt_var, want['obs_drt_var'])
    same(md.obs_tau_indices, [(2, 11), None, (2, 11), (2, 11), (3, 11)])
    assert all(type(v) is int for pair in md.obs_tau_indices if pair is not None for v in pair)
    assert all(f[3] == {'nonneg': True} for f in fake.fits) and fake.llh_calls[-1] == (METRIC, METRIC)


def test_store_with_pfrt_shapes():
    from hipdrt.mapping import store
    md = store.DRTMD(SUP, drt=FakeDRT(), fit_type='pfrt', pfrt_factors=FACTORS, drt_var=True)
    for k, (c, e) in enumerate(pfrt_list()):
        md.add_observation([k], c, e)
    assert md.obs_x.shape == (5, 3, 13) and md.obs_drt_var.shape == (5, 3, 13)
    assert md.fit_all(ignore_errors=True).tolist() == [0, 1, 2, 3, 4]
    want_x, want_special, want = pfrt_expected(pfrt_list(), FACTORS, True, False)
    same(md.obs_x, want_x)
    same(md.obs_special, want_special)
    same(md.obs_drt_var, want['obs_drt_var'])
    same(md.obs_llh, want['obs_llh'])
    same(md.obs_tau_indices, [(2, 11), (2, 11), None, (2, 11), (2, 11)])
    assert md.obs_fit_status.tolist() == [True, True, False, True, True] and md.obs_ignore_flag.tolist() == [False, False, True, False, False]
    assert store.DRTMD(SUP, drt=FakeDRT(), fit_type='pfrt').obs_x.shape == (0, 11, 13)
