"""CPU: the host layer of candidate generation (models/restart.py: generate_candidates, generate_candidates_batch, evaluate_bic and
the table readers) against the recording stand-in plan of test_host_restart.py, extended by the calls this layer adds
(score_candidates, the step store's restore / read-back): the order of the restarts and what each receives, what is uploaded to
the scoring call, that a batch call brings nothing down between its steps, how the scores are reordered and ranked, the refusals.

Expected values are written from the rules: weight restarts first with factors 0.5^i from the fit's x / rho / weights, then s_0
restarts with s_0 * 4^i and l2_lambda_0 / 4^i from the same baseline; candidates ordered base history, s_0 iterates, weight
iterates; k = special parameters + 4 peaks; the best candidate per peak count is the first with the largest llh."""
import types

import numpy as np
import pytest

from test_host_restart import B, BASIS, L2_FIT, M, NB, NS, NSP, S0_FIT, block_rows, eq, ffi, make_drt, prep, rows, same_opts  # noqa: F401

from hipdrt.models import candidates, qphb

COUNTS = np.array([2, 4, 4, 3, 6, 2, 3])         # peaks of candidate c: COUNTS[c % 7]


def extend(plan):
    """the calls the candidate layer adds to a plan; scores depend on the candidate, the member and the peak slot"""
    plan.pf_steps, plan.pf_at = 0, []

    def pfrt_begin(self, max_steps):
        self.rec('pfrt_begin', max_steps=max_steps)
        self.pf_steps, self.pf_at = 0, []

    def pfrt_record(self):
        self.rec('pfrt_record')
        self.pf_at.append(self.step)
        self.pf_steps += 1

    def pfrt_restore_s(self, step, factor=1.0):
        self.rec('pfrt_restore_s', step=step, factor=factor)

    def pfrt_step_state(self, step):
        self.rec('pfrt_step_state', step=step)
        return dict(x=self.x(self.pf_at[step]), status=self.status(self.pf_at[step]))

    def set_tau_basis(self, ln_tau, eps):
        self.rec('set_tau_basis', ln_tau=ln_tau, eps=eps)

    def score_candidates(self, x=None, ncand=None, ln_tau_find=None, opts=None, max_peaks=16, want=None):
        self.rec('score_candidates', x=x, ncand=ncand, ln_tau_find=ln_tau_find, opts=opts, max_peaks=max_peaks)
        C = self.pf_steps if x is None else len(x)
        c, b = np.arange(C)[:, None], np.arange(self.B)[None, :]
        count = np.broadcast_to(COUNTS[np.arange(C) % 7][:, None], (C, self.B)).astype(np.int32)
        slot = np.arange(max_peaks)[None, None, :]
        valid = slot < count[:, :, None]
        idx = np.where(valid, 3 + 5 * slot + (c % 3)[:, :, None] + 0 * b[:, :, None], -1).astype(np.int32)
        ht = np.where(valid, 1.0 + ((slot * 7 + c[:, :, None]) % 5) + 0.0 * b[:, :, None], np.nan)
        pr = np.where(valid, 2.0 + ((slot * 3 + c[:, :, None]) % 4) + 0.0 * b[:, :, None], np.nan)
        return dict(rss=30.0 + ((c * 5) % 11) + b, sum_log_w=-100.0 + 2.0 * ((c * 3) % 7) - b, count=count.copy(),
                    peak_index=idx, heights=ht, prominences=pr, status=np.zeros((C, self.B), dtype=np.int32))

    for f in (pfrt_begin, pfrt_record, pfrt_restore_s, pfrt_step_state, set_tau_basis, score_candidates):
        setattr(plan, f.__name__, types.MethodType(f, plan))
    return plan


def single(ffi):
    drt = make_drt(ffi, batch=1)
    plan = extend(drt._plan)
    n = NS + NB
    drt.qphb_history = [dict(x=rows(1, n)[0] * (k + 1) - 0.5, rho_vector=np.ones(3), weights=np.ones(M)) for k in range(2)]
    drt.qphb_params = dict(weights=np.full(M, 0.75), rho_vector=np.array([1.0, 2.0, 3.0]))
    return drt, plan


def expected_llh(c, b=0):
    rss, slw = 30.0 + ((c * 5) % 11) + b, -100.0 + 2.0 * ((c * 3) % 7) - b
    return qphb.marginal_llh(rss, M) + slw


def test_generate_candidates_restarts_uploads_and_ranks(ffi):
    drt, plan = single(ffi)
    n0 = len(plan.calls)
    cd = drt.generate_candidates()
    # weights first (drt1d.py:1660-1664), each pass from the fit's x / rho / weights, histories recorded
    co = plan.all('continue_fit')
    assert [c['weight_factor'] for c in co] == [0.5, 0.25, 0.125, 1, 1]
    for c in co[:3]:
        same_opts(ffi, c['opts'])
    same_opts(ffi, co[3]['opts'], s_0=S0_FIT * 4, l2_lambda_0=L2_FIT / 4)
    same_opts(ffi, co[4]['opts'], s_0=S0_FIT * 16, l2_lambda_0=L2_FIT / 16)
    st = plan.all('set_state')
    for k in (0, 3):
        eq(st[k]['x'], drt.qphb_history[-1]['x'][None])
        eq(st[k]['rho'], [[1.0, 2.0, 3.0]])
        eq(st[k]['weights'], np.full((1, M), 0.75))
    assert st[0]['s'] is None and all(s['x'] is None for s in (st[1], st[2], st[4]))
    eq(st[3]['s'], plan.s_vectors(3) * 4.0)             # the s vectors the weight pass left, scaled
    eq(st[4]['s'], plan.s_vectors(3) * 16.0)
    assert all(h == dict(b=0) for h in plan.all('record_history'))
    # one scoring call, after the last restart: base history, then the s_0 iterates, then the weight iterates
    names = plan.names(n0)
    assert names.count('score_candidates') == 1 and names[-1] == 'score_candidates'
    sc = plan.all('score_candidates')[0]
    x = np.concatenate([[h['x'] for h in drt.qphb_history]] + [plan.hist(k)['x'] for k in (4, 5, 1, 2, 3)])
    assert x.shape == (2 + 6 + 7 + 3 + 4 + 5, NS + NB)
    eq(sc['x'], x[:, None, :])
    eq(sc['ln_tau_find'], np.log(drt.get_tau_eval(10)))
    o = sc['opts']
    assert (o.eval_sign, o.search, o.normalize, o.method, o.ext_left, o.ext_right) == (1, 1, 1, 0, -1, -1)
    assert np.isnan(o.height) and np.isnan(o.prominence) and sc['ncand'] is None and sc['max_peaks'] == 64
    # the result
    C = len(x)
    assert sorted(cd) == sorted(['x', 'peak_tau', 'peak_info', 'num_peaks', 'llh', 'bic', 'history', 'hypers'])
    eq(cd['x'], x)
    eq(cd['num_peaks'], COUNTS[np.arange(C) % 7])
    eq(cd['llh'], expected_llh(np.arange(C)))
    eq(cd['bic'], (NS + 4 * cd['num_peaks']) * np.log(71) - 2 * cd['llh'])
    tau = drt.get_tau_eval(10)
    for c in (0, 4, C - 1):
        k = COUNTS[c % 7]
        eq(cd['peak_tau'][c], tau[3 + 5 * np.arange(k) + c % 3])
        eq(cd['peak_info'][c]['peak_heights'], 1.0 + ((np.arange(k) * 7 + c) % 5))
        eq(cd['peak_info'][c]['prominences'], 2.0 + ((np.arange(k) * 3 + c) % 4))
    assert len(cd['history']) == C and cd['history'][0] is drt.qphb_history[0]
    eq(cd['history'][2]['x'], plan.hist(4)['x'][0])
    assert cd['hypers'][0] is cd['hypers'][1] and sorted(cd['hypers'][0]) == ['l2_lambda_0', 's_0', 'weight_factor']
    assert cd['hypers'][0]['l2_lambda_0'] == L2_FIT and cd['hypers'][0]['s_0'] is S0_FIT and cd['hypers'][0]['weight_factor'] is None
    eq(cd['hypers'][2]['s_0'], S0_FIT * 4)
    assert cd['hypers'][2 + 6]['l2_lambda_0'] == L2_FIT / 16 and cd['hypers'][2 + 13] == dict(weight_factor=0.5)
    assert cd['hypers'][-1] == dict(weight_factor=0.125)
    # ranking: the statement, on these scores
    r = candidates.rank_candidates(cd['num_peaks'], cd['llh'], NS, 71, [i['prominences'] for i in cd['peak_info']],
                                   [i['peak_heights'] for i in cd['peak_info']])
    assert list(drt.best_candidate_dict) == [2, 3, 4, 5, 6] and r['best_keys'] == [2, 3, 4, 5, 6]
    for name in r['best_table']:
        eq(drt.best_candidate_df[name], r['best_table'][name])
        if name != 'model_id':
            eq(drt.candidate_df[name], r['candidate_table'][name])
    for k, i in zip(r['unique_num_peaks'], r['best_indices']):
        e = drt.best_candidate_dict[int(k)]
        assert i == np.where((cd['num_peaks'] == k) & (cd['llh'] == cd['llh'][cd['num_peaks'] == k].max()))[0][0]
        eq(e['x'], x[i])
        assert e['llh'] == cd['llh'][i] and e['bic'] == cd['bic'][i] and e['history'] is cd['history'][i]
    hi_num, order = r['filled'][5]
    assert hi_num == 6
    five, six = drt.best_candidate_dict[5], drt.best_candidate_dict[6]
    eq(five['peak_tau'], six['peak_tau'][order])
    assert len(five['peak_tau']) == 5 and five['llh'] == six['llh'] and five['bic'] == six['bic']
    eq(order, np.argsort(np.minimum(six['peak_info']['prominences'], six['peak_info']['peak_heights']))[::-1][:5])
    # the readers
    bf = drt.evaluate_norm_bayes_factors('continuous')
    eq(bf, np.exp(-0.5 * (r['best_table']['bic'] - r['best_table']['bic'].min())))
    best = drt.get_best_candidate_id('continuous')
    assert best == r['best_table']['model_id'][np.argmin(r['best_table']['bic'])]
    eq(drt.evaluate_norm_bayes_factors('continuous', candidate_id=best), [1.0])
    assert drt.evaluate_norm_bayes_factors('continuous', candidate_id=9, na_val=-1.0) == -1.0
    assert drt.evaluate_bayes_factor(2, 4, 'continuous') == np.exp(-0.5 * (drt.get_candidate(2, 'continuous')['bic'] -
                                                                            drt.get_candidate(4, 'continuous')['bic']))
    assert drt.get_candidate(5, 'continuous') is five and drt.get_candidate_df('continuous') is drt.best_candidate_df
    # include_qphb_history=False, no filling, the llh keywords
    cd2 = drt.generate_candidates(include_qphb_history=False, fill=False, llh_kw=dict(marginalize_weights=False, normalize=True))
    eq(plan.all('score_candidates')[-1]['x'][0, 0], drt.qphb_history[-1]['x'])
    c = np.arange(len(cd2['x']))
    eq(cd2['llh'], (-0.5 * (30.0 + ((c * 5) % 11)) + (-100.0 + 2.0 * ((c * 3) % 7))) / M)
    assert sorted(drt.best_candidate_dict) == sorted(set(cd2['num_peaks'].tolist()))


def test_batch_brings_nothing_down_between_its_steps(ffi):
    drt = make_drt(ffi)
    plan = extend(drt._plan)
    out = drt.generate_candidates_batch()
    names = plan.names()
    first, score = names.index('pfrt_record'), names.index('score_candidates')
    assert names[:first] == ['download', 'timings', 'pfrt_begin'] and plan.all('pfrt_begin') == [dict(max_steps=6)]
    between = names[first:score]
    assert set(between) == {'pfrt_record', 'set_state', 'record_history', 'continue_fit', 'pfrt_restore_s'}
    assert between.count('pfrt_record') == 6 and between.count('continue_fit') == 5
    # weights first, each pass from the fit's state; the s_0 pass takes its s vectors from the step store, on the device
    assert [c['weight_factor'] for c in plan.all('continue_fit')] == [0.5, 0.25, 0.125, 1, 1]
    st = plan.all('set_state')
    for k in (0, 3):
        eq(st[k]['x'], plan.x(0))
        eq(st[k]['weights'], plan.weights(0))
    assert all(s['s'] is None for s in st) and all(s['x'] is None for s in (st[1], st[2], st[4]))
    assert plan.all('pfrt_restore_s') == [dict(step=3, factor=4), dict(step=3, factor=16)]
    assert names.index('pfrt_restore_s') > [i for i, n in enumerate(names) if n == 'pfrt_record'][3]
    same_opts(ffi, plan.all('continue_fit')[4]['opts'], s_0=S0_FIT * 16, l2_lambda_0=L2_FIT / 16)
    assert all(h == dict(b=-1) for h in plan.all('record_history'))
    sc = plan.all('score_candidates')
    assert len(sc) == 1 and sc[0]['x'] is None
    # recorded fit, w1, w2, w3, s1, s2 -> reported fit, s1, s2, w1, w2, w3
    order = np.array([0, 4, 5, 1, 2, 3])
    eq(out['num_peaks'], np.broadcast_to(COUNTS[order][:, None], (6, B)))
    eq(out['llh'], np.stack([expected_llh(order, b) for b in range(B)], axis=1))
    eq(out['x'], np.array([plan.x(k) for k in order]))
    eq(out['bic'], (NS + 4 * out['num_peaks']) * np.log(71) - 2 * out['llh'])
    eq(out['status'], np.zeros(B))
    assert out['hypers'][1]['l2_lambda_0'] == L2_FIT / 4 and out['hypers'][3] == dict(weight_factor=0.5)
    for b in range(B):
        r = candidates.rank_candidates(out['num_peaks'][:, b], out['llh'][:, b], NS, 71,
                                       [p[~np.isnan(p)] for p in out['prominences'][:, b]],
                                       [p[~np.isnan(p)] for p in out['peak_heights'][:, b]])
        assert out['best'][b]['keys'] == r['best_keys'] == [2, 3, 4, 5, 6]
        eq(out['best'][b]['best_indices'], r['best_indices'])
        eq(out['best'][b]['table']['bic'], r['best_table']['bic'])


def test_batch_on_a_prepared_plan_scales_the_baseline_weights_and_fails_members(ffi):
    preps = [dict(prep(2.0, 0.5), coefficient_scale=1.5), dict(prep(3.0, 0.25), coefficient_scale=2.5)]
    drt = make_drt(ffi, preps, dop_size=50, status={2: [0, -1]})
    plan = extend(drt._plan)
    out = drt.generate_candidates_batch(s0_steps=1, weight_steps=2)
    st = plan.all('set_state')
    for k in (0, 2):
        eq(st[k]['weights'], plan.weights(0) * block_rows((2.0, 0.5), (3.0, 0.25)))
        eq(st[k]['dop_rho'], rows(2, 3) + 0.75)
    assert plan.all('pfrt_restore_s') == [dict(step=2, factor=4)]
    assert plan.all('score_candidates')[0]['opts'].normalize == 1
    eq(out['status'], [0, -1])                          # the second weight restart failed for member 1: it stays
    assert out['best'][1] is None and out['best'][0]['keys'] == [2, 3, 4] and np.isnan(out['bic'][:, 1]).all()
    eq(out['bic'][:, 0], (NSP + 4 * out['num_peaks'][:, 0]) * np.log(40 + 51) - 2 * out['llh'][:, 0])


def test_evaluate_bic(ffi):
    """upstream's rule (drt1d.py:4498-4511): llh = evaluate_llh(**llh_kw) of the fitted solution -- the fit's own est_weights
    unless `weights` says otherwise, NOT the candidates' re-estimated weights -- and the peaks of find_peaks(**find_peaks_kw)"""
    drt = make_drt(ffi)
    plan = extend(drt._plan)
    counts = [2, 0, 5]

    def find_peaks(self, ln_tau, opts, row_scale=None, want=None):
        self.rec('find_peaks', ln_tau=ln_tau, opts=opts, want=want)
        keep = np.zeros((self.B, len(ln_tau)), dtype=np.int32)
        for b, k in enumerate(counts):
            keep[b, 3:3 + 2 * k:2] = 1
        return dict(keep=keep, status=np.zeros(self.B, dtype=np.int32))
    plan.find_peaks = types.MethodType(find_peaks, plan)
    bic = drt.evaluate_bic_batch()
    assert plan.names() == ['find_peaks', 'llh_terms'] and plan.all('llh_terms') == [dict(stored=True, weights=None)]
    fp = plan.all('find_peaks')[0]
    eq(fp['ln_tau'], np.log(drt.get_tau_eval(10)))
    assert fp['want'] == ('keep',) and fp['opts'].method == 0 and np.isnan(fp['opts'].prominence)
    rss, slw = plan.llh(0)
    eq(bic, (NS + 4 * np.array(counts)) * np.log(71) - 2 * (qphb.marginal_llh(rss, M) + slw))
    # the keywords of both calls reach them
    bic = drt.evaluate_bic_batch(find_peaks_kw=dict(prominence=0.01, height=0.002, ppd=20, method='prob'), weights='uniform',
                                 alpha_0=3, beta_0=2, normalize=True)
    fp = plan.all('find_peaks')[1]
    eq(fp['ln_tau'], np.log(drt.get_tau_eval(20)))
    assert (fp['opts'].prominence, fp['opts'].height, fp['opts'].method) == (0.01, 0.002, 1)
    assert plan.all('llh_terms')[1] == dict(stored=True, weights='uniform')
    eq(bic, (NS + 4 * np.array(counts)) * np.log(71) - 2 * (qphb.marginal_llh(rss, M, 3, 2) + slw) / M)
    assert drt.evaluate_bic(b=2, marginalize_weights=False) == (NS + 20) * np.log(71) - 2 * (-0.5 * rss[2] + slw[2])
    assert not plan.all('score_candidates')
    with pytest.raises(TypeError, match="gamma_0"):
        drt.evaluate_bic_batch(gamma_0=1)


def test_refusals(ffi):
    drt, plan = single(ffi)
    n0 = len(plan.calls)
    with pytest.raises(NotImplementedError, match="'prob' needs a P matrix per candidate"):
        drt.generate_candidates(find_peaks_kw=dict(method='prob'))
    with pytest.raises(NotImplementedError, match="distance"):
        drt.generate_candidates(find_peaks_kw=dict(distance=3))
    with pytest.raises(TypeError, match="weights"):
        drt.generate_candidates(llh_kw=dict(weights='uniform'))
    with pytest.raises(Exception, match="finished single qphb fit"):
        drt.generate_candidates(b=1)
    assert len(plan.calls) == n0                         # refused before anything reached the plan
    with pytest.raises(ValueError, match="Candidates must be first be generated using generate_candidates"):
        drt.get_candidate(2, 'continuous')
    with pytest.raises(ValueError, match="Candidates must be first be generated"):
        drt.evaluate_norm_bayes_factors('continuous')
    for kind in ('discrete', 'pfrt'):
        with pytest.raises(NotImplementedError, match="discrete element models"):
            drt.get_candidate(2, kind)
        with pytest.raises(NotImplementedError, match="discrete element models"):
            drt.get_candidate_df(kind)
    with pytest.raises(NotImplementedError, match="discrete element models"):
        drt.get_best_candidate_id('discrete')
    with pytest.raises(ValueError, match="Invalid candidate_type other"):
        drt.get_candidate_df('other')
    with pytest.raises(ValueError, match="Invalid candidate_type pfrt"):
        drt.get_best_candidate_id('pfrt')
    drt.generate_candidates()
    with pytest.raises(ValueError, match="No candidate with 9 peaks exists"):
        drt.get_candidate(9, 'continuous')
    with pytest.raises(ValueError, match="Invalid criterion aic"):
        drt.get_best_candidate_id('continuous', 'aic')
    with pytest.raises(NotImplementedError, match="evaluate_lml"):
        drt.evaluate_norm_bayes_factors('continuous', criterion='lml')
    batch = make_drt(ffi)
    extend(batch._plan)
    with pytest.raises(Exception, match="generate_candidates_batch"):
        batch.generate_candidates()
    prepared = make_drt(ffi, [dict(prep(2.0, 0.5), coefficient_scale=1.5)] * 2)
    extend(prepared._plan)
    with pytest.raises(NotImplementedError, match="normalize=False on a prepared plan"):
        prepared.generate_candidates_batch(find_peaks_kw=dict(normalize=False))
