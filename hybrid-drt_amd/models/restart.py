"""Everything of DRT that re-enters the device loop on a finished fit, for both plan kinds (the EIS plan of fit_eis /
fit_eis_batch and the prepared-matrix plan of chrono / joint / DOP fits): the warm restart (DRT._continue_from_init,
drt1d.py:1270-1365), the candidate generators on top of it (1497-1632) and the PFRT step loop (_pfrt_fit_core, 2558-2715).
The flow is written once; where the kinds differ -- the finished-fit check, the keyword split, the row factors and dop_rho of
a prepared plan, what is collected -- the difference is one named piece."""
import numpy as np

from .. import _ffi
from . import candidates, lml, qphb


def combine_status(so_far, step):
    """per-spectrum status of a chain of fits (a full fit and its warm restarts): a failure (< 0: QP breakdown, singular KKT
    system) in ANY step stays -- its iterate went into every later step --, otherwise the last step's verdict (0 converged,
    1 stopped at max_iter)"""
    so_far, step = np.asarray(so_far), np.asarray(step)
    return np.where(step < 0, step, np.where(so_far < 0, so_far, step))


def restart_row_factors(preps, chrono_weight_factor=None, eis_weight_factor=None):
    """the (measurement, data row) factors of a warm restart on a prepared plan, None when every entry is 1: a joint
    measurement's chrono block takes the given chrono factor, its eis block the given eis factor, and a factor that is not
    given falls back to the FIT's chrono factor, for both blocks (drt1d.py:1284-1287); any other measurement takes 1"""
    rows = []
    for pr in preps:
        nc, m = pr['num_chrono'], pr['m']
        if nc > 0 and pr['num_eis'] > 0:
            cf = pr['chrono_weight_factor'] if chrono_weight_factor is None else chrono_weight_factor
            ef = pr['chrono_weight_factor'] if eis_weight_factor is None else eis_weight_factor
        else:
            cf = ef = 1.0
        rows.append(np.concatenate([np.full(nc, float(cf)), np.full(m - nc, float(ef))]))
    rows = np.array(rows)
    return None if np.all(rows == 1.0) else rows


def pfrt_schedule(factors, kw):
    """(factors, step_hypers) of a PFRT run: the regularisation factors (default 11 over two decades) and what step f sets,
    s_0 * f and l2_lambda_0 / f of the given or default hyper-parameters (drt1d.py:2590-2600)"""
    base = qphb.get_default_hypers()
    base.update({k: v for k, v in kw.items() if k in base})
    factors = np.asarray(np.logspace(-1, 1, 11) if factors is None else factors, dtype=float)
    s_0 = np.broadcast_to(np.asarray(base['s_0'], dtype=float), (3,))

    def step_hypers(f):
        return dict(s_0=s_0 * f, l2_lambda_0=base['l2_lambda_0'] / f)
    return factors, step_hypers


def _no_column(criterion):
    """the candidate tables hold bic only, like upstream's continuous tables: 'lml' and 'lml-bic' have nothing to read"""
    return (f"criterion {criterion!r}: the candidate tables have no such column (nor have upstream's continuous tables); "
            "evaluate_lml / evaluate_lml_batch score a fit, not a table of candidates")


class RestartMixin:
    """Methods of DRT that act on the state a finished fit left on the device."""

    # ---- the warm restart ---------------------------------------------------------------------------------------------
    def _restart_preps(self):
        """the finished-fit check of a warm restart: the prepared measurements of the last fit on a prepared plan (batch,
        else single), None on an EIS plan"""
        if isinstance(self._plan, _ffi.PreparedPlan):
            if getattr(self, '_last_prepared', None):
                return self._last_prepared[0]
            if getattr(self, '_prep', None) is not None:
                return [self._prep]
        elif self._plan is not None and self._last_batch is not None:
            return None
        raise Exception('continue_from_init needs a finished qphb fit')

    def _collect_restart(self):
        """the state a fit or a warm restart leaves on the device, as arrays with a leading batch axis: collect_staged() on an
        EIS plan; on a prepared plan the loop's own arrays (scaled units), dop_rho where there is a DOP block, and the timings"""
        plan = self._plan
        if not isinstance(plan, _ffi.PreparedPlan):
            return self.collect_staged()
        out = plan.download(s_vectors=True)
        res = {k: out[k] for k in ('x', 'rho', 'weights', 's_vectors', 'q_vector', 'outer_iters', 'qp_iters_total', 'status')}
        if plan.desc.dop_size > 0:
            res['dop_rho'] = plan.get('dop_rho')
        res['timings_ms'], res['launches'] = plan.timings()
        return res

    def continue_from_init(self, x_init=None, rho_vector=None, s_vectors=None, weights=None, weight_factor=1,
                           xtol=1e-2, max_iter=10, min_iter=2, history_of=-1, dop_rho_vector=None, collect=True, **kw):
        """DRT._continue_from_init for the last fit (EIS, chrono, joint, DOP; single or batch): the outer loop re-entered on
        the device from the given state (arrays with a leading batch axis; None = the state left by the previous call) with
        ``kw`` updating the hyper-parameters (e.g. s_0, l2_lambda_0).  est_weights, xmx / dop_xmx norms and the data scale
        stay as fitted.  A prepared plan also takes ``chrono_weight_factor`` / ``eis_weight_factor`` (restart_row_factors: they
        multiply the weights at the top of every iteration together with ``weight_factor``) and ``dop_rho_vector``, and rewrites
        its vz_offset column after every iteration from a copy of the matrix frozen at entry (1295-1298).  Returns the arrays
        of _collect_restart (outer_iters = iterations of this call), plus ``history`` of member ``history_of`` when that is >= 0;
        ``collect=False`` leaves everything on the device and returns None."""
        preps = self._restart_preps()
        fit_kw = dict(self.fit_kwargs, **kw, xtol=xtol, max_iter=max_iter)
        state = dict(x=x_init, rho=rho_vector, s=s_vectors, weights=weights)
        plan = self._plan
        if preps is None:       # EIS plan: an unknown keyword is _make_opts' ValueError
            opts, _, _ = self._make_opts(fit_kw)
        else:                   # prepared plan: the chrono / hybrid keywords (the two factors among them) stop at _split_kwargs
            opts, _, _ = self._make_opts(self._split_kwargs(fit_kw)[1])
            plan.set_weight_factors(1.0, restart_row_factors(preps, kw.get('chrono_weight_factor'), kw.get('eis_weight_factor')))
            state['dop_rho'] = dop_rho_vector
        plan.set_state(**state)
        plan.record_history(history_of)
        plan.continue_fit(opts, weight_factor=weight_factor, min_iter=min_iter)
        if not collect:
            return None
        res = self._collect_restart()
        if history_of >= 0:
            res['history'] = plan.history()
        return res

    _continue_prepared = continue_from_init         # the name the prepared-plan tests call

    # ---- candidate generators (drt1d.py:1497-1632) ----------------------------------------------------------------------
    def _candidate_baseline(self):
        """What the reference's candidate generators re-read from the finished fit before their first warm restart
        (drt1d.py:1517-1525, 1587-1594): x of the last recorded iterate, rho / dop_rho and the (scaled) weights of
        qphb_params -- NOT the s vectors, which its shallow list copies let earlier warm restarts update in place.  Single
        fits only (a batch fit keeps no per-spectrum qphb_params: its restarts go on from the state on the device)."""
        qp, hist = getattr(self, 'qphb_params', None), getattr(self, 'qphb_history', None)
        if not qp or not hist or self._plan.B != 1 or len(qp['weights']) != self._plan.m:
            return {}
        base = dict(x_init=np.asarray(hist[-1]['x'])[None, :], rho_vector=np.asarray(qp['rho_vector'])[None, :],
                    weights=np.asarray(qp['weights'])[None, :])
        if qp.get('dop_rho_vector') is not None:
            base['dop_rho_vector'] = np.asarray(qp['dop_rho_vector'])[None, :]
        return base

    def generate_candidates_s0(self, multiplier, steps, xtol=1e-2, max_iter=10, history_of=-1):
        """DRT._generate_candidates_s0 (drt1d.py:1497-1565) for the last fit (EIS, chrono or joint; single or batch): step i
        restarts with s_0 * multiplier^i, l2_lambda_0 / multiplier^i and (multiplier > 1) the baseline s vectors
        scaled by multiplier^i; the first step from the fit's x / rho / weights, later ones from their predecessor's.
        Returns the list of per-step result dicts."""
        s_base = self._collect_restart()['s_vectors'].copy()
        s_in = s_base.copy()
        s_0 = np.broadcast_to(np.asarray(self.fit_kwargs['s_0'], dtype=float), (3,)).copy()
        out = []
        start = self._candidate_baseline()
        for i in range(1, steps + 1):
            f = multiplier ** i
            s_in = s_base * f if multiplier > 1 else s_in * multiplier
            res = self.continue_from_init(s_vectors=s_in, xtol=xtol, max_iter=max_iter, history_of=history_of,
                                          s_0=s_0 * f, l2_lambda_0=self.fit_kwargs['l2_lambda_0'] / f, **start)
            start = {}
            s_in = res['s_vectors'].copy()
            out.append(res)
        return out

    def generate_candidates_weights(self, multiplier, steps, xtol=1e-2, max_iter=10, history_of=-1):
        """DRT._generate_candidates_weights (drt1d.py:1567-1632): step i restarts with weight_factor = multiplier^i.
        As in the reference (whose shallow list copy lets iterate_qphb update the stored s vectors in place) every
        step starts from the s vectors the previous step ended with."""
        out = []
        start = self._candidate_baseline()
        for i in range(1, steps + 1):
            out.append(self.continue_from_init(weight_factor=multiplier ** i, xtol=xtol, max_iter=max_iter,
                                               history_of=history_of, **start))
            start = {}
        return out

    # ---- candidate models (drt1d.py:1632-1821, 2383-2500, 4498-4511) ---------------------------------------------------------
    # The device scores the candidates (hipdrt_plan_score_candidates: likelihood sums and peaks of many x per spectrum); the
    # ranking is models/candidates.py.  Each rule of a request is stated once, here.
    def _candidate_llh(self, rss, sum_log_w, llh_kw):
        """DRT.evaluate_llh's keywords (drt1d.py:4457-4496) applied to the device's sums; the weights are the candidate's own
        re-estimate, so ``weights`` is not one of them"""
        kw = dict(llh_kw or {})
        bad = set(kw) - {'marginalize_weights', 'alpha_0', 'beta_0', 'normalize'}
        if bad:
            raise TypeError(f"unexpected keyword(s) {sorted(bad)}")
        m = self._plan.m
        llh = qphb.marginal_llh(rss, m, kw.get('alpha_0', 2), kw.get('beta_0', 1)) if kw.get('marginalize_weights', True) \
            else -0.5 * rss
        llh = llh + sum_log_w
        return llh / m if kw.get('normalize', False) else llh

    def _candidate_peak_request(self, what, find_peaks_kw):
        """(plan, tau, hipdrt_peak_opts) of find_peaks(x=candidate, **find_peaks_kw): method 'thresh' only ('prob' needs a P
        matrix per candidate); a prepared plan runs at unit scale, so its candidates are normalised by their own R_p"""
        kw = dict(find_peaks_kw or {})
        tau, ppd, sign = kw.pop('tau', None), kw.pop('ppd', 10), kw.pop('sign', 1)
        normalize, method = kw.pop('normalize', True), kw.pop('method', 'thresh')
        opt_kw = {k: kw.pop(k) for k in ('height', 'prominence') if k in kw}
        if method != 'thresh':
            raise NotImplementedError(f"{what}: find_peaks method {method!r} needs a P matrix per candidate; only 'thresh' is built")
        for name in kw:
            raise NotImplementedError(f'{what}: the find_peaks argument {name}= is not taken')
        plan, scales = self._predict_plan(what)
        if scales is not None and not normalize:
            raise NotImplementedError(f'{what}: normalize=False on a prepared plan (its rows carry no data scale on the device)')
        tau = np.asarray(self.get_tau_eval(ppd) if tau is None else tau, dtype=float)
        return plan, tau, self._peak_opts(plan, tau, sign, 'thresh', normalize, False, opt_kw)

    def _num_independent_data(self, b=0):
        """DRT.num_independent_data (drt1d.py:72-80): sample times plus frequencies of member ``b``"""
        if isinstance(self._plan, _ffi.PreparedPlan):
            pr = self._members()[b]
            return int(pr['num_chrono'] + pr['num_eis'])
        return len(self.f_fit)

    def _score_candidates(self, plan, x, tau, opts, llh_kw, max_peaks=64):
        """hipdrt_plan_score_candidates (x (C, B, n) uploaded, or None: the recorded steps) with llh (C, B) added"""
        out = plan.score_candidates(x, ln_tau_find=np.log(tau), opts=opts, max_peaks=max_peaks)
        if np.any(out['status'] == _ffi.PEAKS_OVERFLOW):
            raise ValueError(f'a candidate has more than {max_peaks} peaks')
        out['llh'] = self._candidate_llh(out['rss'], out['sum_log_w'], llh_kw)
        return out

    def _rank_member(self, scores, c_order, b, tau, fill, min_fill_num):
        """candidates.rank_candidates for member ``b`` of a scored batch, the candidates taken in the order ``c_order`` ->
        (rank dict, peak_tau list, peak_info list)"""
        idx = scores['peak_index'][c_order, b]
        keep = [row >= 0 for row in idx]
        peak_tau = [tau[row[k]] for row, k in zip(idx, keep)]
        info = [{'peak_heights': scores['heights'][c, b][k], 'prominences': scores['prominences'][c, b][k]}
                for c, k in zip(c_order, keep)]
        rank = candidates.rank_candidates(scores['count'][c_order, b], scores['llh'][c_order, b], self._plan.ns,
                                          self._num_independent_data(b), [i['prominences'] for i in info],
                                          [i['peak_heights'] for i in info], fill=fill, min_fill_num=min_fill_num)
        return rank, peak_tau, info

    @staticmethod
    def _best_dict(rank, entry):
        """best_candidate_dict (drt1d.py:1731-1812): entry(i) of the best candidate per peak count, then the filled counts --
        everything of the richer candidate, its peaks cut to the most prominent j -- sorted by peak count"""
        best = {int(k): entry(i) for k, i in zip(rank['unique_num_peaks'], rank['best_indices'])}
        for j, (hi_num, order) in rank['filled'].items():
            src = best[hi_num]
            best[j] = dict(src, peak_tau=src['peak_tau'][order], peak_info={k: v[order] for k, v in src['peak_info'].items()})
        return {k: best[k] for k in sorted(best)}

    def generate_candidates(self, s0_multiplier=4, s0_steps=2, weight_multiplier=0.5, weight_steps=3,
                            include_qphb_history=True, fill=True, min_fill_num=None, xtol=1e-2, max_iter=10, llh_kw=None,
                            find_peaks_kw=None, b=0):
        """DRT.generate_candidates (drt1d.py:1632-1821) for a single fit (EIS, chrono, joint, DOP): the weight restarts, then the
        s_0 restarts (1660-1664), every recorded iterate a candidate in the order base history, s_0 iterates, weight iterates;
        all of them scored in one device call.  Leaves candidate_dict (x, peak_tau, peak_info, num_peaks, llh, bic, history,
        hypers), candidate_df, best_candidate_dict and best_candidate_df (the tables as dicts of arrays) and returns a copy of
        candidate_dict.  peak_info holds peak_heights and prominences."""
        if b != 0 or self._plan is None or self._plan.B != 1 or not self.qphb_history:
            raise Exception('generate_candidates needs a finished single qphb fit (a batch: generate_candidates_batch)')
        self._restart_preps()
        plan, tau, opts = self._candidate_peak_request('generate_candidates', find_peaks_kw)
        self._candidate_llh(0.0, 0.0, llh_kw)               # (the keyword check comes before the first restart)
        base = list(self.qphb_history) if include_qphb_history else list(self.qphb_history[-1:])
        down = self.generate_candidates_weights(weight_multiplier, weight_steps, xtol=xtol, max_iter=max_iter, history_of=0)
        up = self.generate_candidates_s0(s0_multiplier, s0_steps, xtol=xtol, max_iter=max_iter, history_of=0)

        def iterates(steps, hypers_of):
            hist, hyp = [], []
            for i, res in enumerate(steps, start=1):
                h = res['history']
                hist += [dict(x=h['x'][k], rho_vector=h['rho'][k], weights=h['weights'][k],
                              dop_rho_vector=h['dop_rho'][k] if 'dop_rho' in h else None) for k in range(len(h['x']))]
                hyp += [hypers_of(i)] * len(h['x'])
            return hist, hyp
        s_0 = np.broadcast_to(np.asarray(self.fit_kwargs['s_0'], dtype=float), (3,))
        up_hist, up_hyp = iterates(up, lambda i: {'s_0': s_0 * s0_multiplier ** i,
                                                  'l2_lambda_0': self.fit_kwargs['l2_lambda_0'] / s0_multiplier ** i})
        down_hist, down_hyp = iterates(down, lambda i: {'weight_factor': weight_multiplier ** i})
        default = {k: self.fit_kwargs.get(k) for k in ('weight_factor', 's_0', 'l2_lambda_0')}
        history = base + up_hist + down_hist
        hypers = [default] * len(base) + up_hyp + down_hyp
        x = np.array([h['x'] for h in history])
        scores = self._score_candidates(plan, x[:, None, :], tau, opts, llh_kw)
        rank, peak_tau, info = self._rank_member(scores, np.arange(len(x)), 0, tau, fill, min_fill_num)
        llh, num_peaks = scores['llh'][:, 0], scores['count'][:, 0].astype(int)
        self.candidate_dict = {'x': x, 'peak_tau': peak_tau, 'peak_info': info, 'num_peaks': num_peaks, 'llh': llh,
                               'bic': rank['bic'], 'history': history, 'hypers': hypers}
        self.candidate_df = rank['candidate_table']
        self.best_candidate_dict = self._best_dict(rank, lambda i: {
            'x': x[i], 'llh': llh[i], 'bic': rank['bic'][i], 'peak_tau': peak_tau[i], 'peak_info': info[i],
            'history': history[i], 'hypers': hypers[i]})
        self.best_candidate_df = rank['best_table']
        return self.candidate_dict.copy()

    def generate_candidates_batch(self, s0_multiplier=4, s0_steps=2, weight_multiplier=0.5, weight_steps=3, fill=True,
                                  min_fill_num=None, xtol=1e-2, max_iter=10, llh_kw=None, find_peaks_kw=None):
        """generate_candidates for every spectrum of the last batch.  The candidates are the final state of the fit and of each
        restart, 1 + s0_steps + weight_steps per spectrum, kept in the plan's step store: the fit's x / rho / weights come down
        once before the first restart (both passes start from them), after that nothing crosses to the host until the scores
        do.  Returns dict(x (C, B, n); llh, bic, num_peaks (C, B); peak_index, peak_heights, prominences (C, B, max_peaks),
        -1 / NaN padded; status (B,): a failure in any step stays; tau; hypers: per candidate; best: per spectrum
        dict(table, keys, filled, best_indices) of candidates.rank_candidates, None where a step failed), the candidates
        ordered fit, s_0 steps, weight steps as generate_candidates orders them."""
        self._restart_preps()
        plan, tau, opts = self._candidate_peak_request('generate_candidates_batch', find_peaks_kw)
        self._candidate_llh(0.0, 0.0, llh_kw)
        # what both passes start from (_candidate_baseline, per member): the fit's x / rho and its weights as qphb_params holds
        # them -- on a prepared plan times the fit's chrono / eis factors
        start = self._collect_restart()
        baseline = dict(x_init=start['x'], rho_vector=start['rho'], weights=start['weights'])
        if isinstance(plan, _ffi.PreparedPlan):
            baseline['weights'] = start['weights'] * np.array([np.concatenate([
                np.full(pr['num_chrono'], pr['chrono_weight_factor']), np.full(pr['m'] - pr['num_chrono'], pr['eis_weight_factor'])])
                for pr in self._members()])
        if 'dop_rho' in start:
            baseline['dop_rho_vector'] = start['dop_rho']
        # the plan has ONE step store: the steps of an earlier PFRT fit go, and with them pfrt_result, so that predict_pfrt and
        # step_p_matrix refuse afterwards instead of reading restart states
        self.pfrt_result = None
        plan.pfrt_begin(1 + s0_steps + weight_steps)
        plan.pfrt_record()
        state = dict(baseline)
        for i in range(1, weight_steps + 1):
            self.continue_from_init(weight_factor=weight_multiplier ** i, xtol=xtol, max_iter=max_iter, collect=False, **state)
            state = {}
            plan.pfrt_record()
        s_0 = np.broadcast_to(np.asarray(self.fit_kwargs['s_0'], dtype=float), (3,))
        state = dict(baseline)
        for i in range(1, s0_steps + 1):
            f = s0_multiplier ** i
            # the s vectors the weight restarts ended with, scaled (multiplier > 1), else the predecessor's once more
            plan.pfrt_restore_s(weight_steps if s0_multiplier > 1 else plan.pfrt_steps() - 1, f if s0_multiplier > 1 else s0_multiplier)
            self.continue_from_init(xtol=xtol, max_iter=max_iter, collect=False, s_0=s_0 * f,
                                    l2_lambda_0=self.fit_kwargs['l2_lambda_0'] / f, **state)
            state = {}
            plan.pfrt_record()
        scores = self._score_candidates(plan, None, tau, opts, llh_kw)
        # recorded: fit, weight steps, s_0 steps -> reported: fit, s_0 steps, weight steps
        order = np.r_[0, 1 + weight_steps + np.arange(s0_steps), 1 + np.arange(weight_steps)].astype(int)
        B = plan.B
        recorded = [plan.pfrt_step_state(int(c)) for c in order]
        status = None                                   # a failure in any step stays (combine_status), in run order
        for c in np.argsort(order):
            status = recorded[c]['status'] if status is None else combine_status(status, recorded[c]['status'])
        ranks = [self._rank_member(scores, order, b, tau, fill, min_fill_num)[0] if status[b] >= 0 and
                 np.all(scores['count'][:, b] >= 0) else None for b in range(B)]
        default = {k: self.fit_kwargs.get(k) for k in ('weight_factor', 's_0', 'l2_lambda_0')}
        hypers = [default] + [{'s_0': s_0 * s0_multiplier ** i, 'l2_lambda_0': self.fit_kwargs['l2_lambda_0'] / s0_multiplier ** i}
                              for i in range(1, s0_steps + 1)] + [{'weight_factor': weight_multiplier ** i}
                                                                  for i in range(1, weight_steps + 1)]
        x = np.array([r['x'] for r in recorded])
        bic = np.full(scores['llh'].shape, np.nan)
        for b, r in enumerate(ranks):
            if r is not None:
                bic[:, b] = r['bic']
        self.candidate_batch = dict(
            x=x, llh=scores['llh'][order], bic=bic, num_peaks=scores['count'][order], status=status,
            peak_index=scores['peak_index'][order], peak_heights=scores['heights'][order], prominences=scores['prominences'][order],
            tau=tau, hypers=hypers,
            best=[None if r is None else dict(table=r['best_table'], keys=r['best_keys'], filled=r['filled'],
                                              best_indices=r['best_indices']) for r in ranks])
        return self.candidate_batch

    def evaluate_bic_batch(self, find_peaks_kw=None, **llh_kw):
        """DRT.evaluate_bic (drt1d.py:4498-4511) for every spectrum of the last batch, on the live fit: k ln(n) - 2 llh with
        k = the special parameters + 4 per peak.  As upstream, llh is evaluate_llh(**llh_kw) of the fitted solution -- by default
        under the fit's own est_weights, NOT the re-estimated weights generate_candidates scores its candidates with
        (evaluate_obs_llh_rss_batch: ``weights``, ``marginalize_weights``, ``alpha_0``, ``beta_0``, ``normalize``) -- and the peaks
        are find_peaks_batch(**find_peaks_kw)'s; only the sums and the peak mask come down.  A failed fit has a NaN solution and
        so a NaN llh and BIC."""
        peak_tau = self.find_peaks_batch(**(find_peaks_kw or {}))
        llh, _ = self.evaluate_obs_llh_rss_batch(llh_kw=llh_kw)
        n_data = np.array([self._num_independent_data(b) for b in range(self._plan.B)])
        return candidates.bic(self._plan.ns + 4 * np.array([len(p) for p in peak_tau]), n_data, llh)

    def evaluate_bic(self, b=0, find_peaks_kw=None, **llh_kw):
        """DRT.evaluate_bic of member ``b`` of the last fit"""
        return float(self.evaluate_bic_batch(find_peaks_kw=find_peaks_kw, **llh_kw)[b])

    # ---- the log marginal likelihood (drt1d.py:4513-4543) -------------------------------------------------------------------
    def evaluate_lml_batch(self, weights=None, update_hypers=None, state=None, step=None, alpha_0=1, beta_0=1, return_terms=False):
        """DRT.evaluate_lml (drt1d.py:4513-4543 over qphb.py:1279-1344) for every spectrum of the last batch -> (B,): both
        log-determinants and the sums on the device (hipdrt_plan_lml_terms), upstream's last two lines here (models/lml.py).
        state: dict of batch arrays x (B, n), rho_vector (B, 3), s_vectors (B, 3, n), plus dop_rho_vector (B, 3) for a fit with
        fit_dop -- what upstream takes from a history entry; step: a recorded step of the step store (PFRT steps, candidates);
        neither: the live fit.  weights (B, m) or (m,): None = the fit's est_weights, as upstream.  update_hypers: of the keys of
        a hyper dict, l2_lambda_0, derivative_weights, dop_l2_lambda_0 and dop_derivative_weights reach the formula, the others
        are accepted without effect, as upstream; a key no hyper dict has is a ValueError.  A member whose fit failed, or whose
        P or prior precision is not positive definite, gives NaN (status: the fit's, or PREDICT_NOT_PD); so does a negative
        beta, as upstream.  return_terms: (lml, dict of the eight terms and status)."""
        plan = self._plan
        if plan is None or not plan.B:
            raise ValueError('evaluate_lml needs a finished fit')
        if state is not None and step is not None:
            raise ValueError('state and step exclude each other')
        has_dop = 'x_dop' in (self.special_qp_params or {})
        hypers = None
        if update_hypers:
            hypers = lml.updated_hypers({k: self.fit_kwargs[k] for k in lml.LML_HYPERS if k in self.fit_kwargs}, update_hypers,
                                        known=qphb.get_default_hypers(fit_dop=True))
        kw = {}
        if state is not None:
            x, rho, s, dop_rho = lml.entry_state(state)
            if has_dop and dop_rho is None:
                raise ValueError('state lacks dop_rho_vector: this fit has a DOP block')
            kw = dict(x=x, rho=rho, s_vectors=np.asarray(s, dtype=float), dop_rho=dop_rho if has_dop else None)
        if weights is not None:
            weights = np.broadcast_to(np.asarray(weights, dtype=float), (plan.B, plan.m))
            if not np.all(weights > 0):
                raise ValueError('weights must be positive')
        terms = plan.lml_terms(step=step, weights=weights, hypers=hypers, **kw)
        out = np.asarray(lml.lml_from_terms(terms, plan.m, alpha_0, beta_0), dtype=float)
        out = np.where(terms['status'] < 0, np.nan, out)
        return (out, terms) if return_terms else out

    def evaluate_lml(self, history_entry=None, weights=None, update_hypers=None, b=0):
        """DRT.evaluate_lml of member ``b`` of the last fit, upstream's signature.  history_entry: a dict with x, rho_vector,
        s_vectors (and dop_rho_vector), as upstream's history entries are; this project's own qphb_history entries carry no
        s_vectors and are refused with a pointer to evaluate_lml_batch(step=...) / (state=...).  Where upstream raises
        'Determinant of ... is negative - not PSD', a failed factorisation raises the same text."""
        plan = self._plan
        if plan is None or not plan.B:
            raise ValueError('evaluate_lml needs a finished fit')
        state = None
        if history_entry is not None:
            x, rho, s, dop_rho = lml.entry_state(history_entry)
            live = plan.download(s_vectors=True)                       # the other members keep their own state
            state = dict(x=live['x'].copy(), rho_vector=live['rho'].copy(), s_vectors=live['s_vectors'].copy())
            state['x'][b], state['rho_vector'][b], state['s_vectors'][b] = x, rho, np.asarray(s, dtype=float)
            if 'x_dop' in (self.special_qp_params or {}):
                if dop_rho is None:
                    raise ValueError('history_entry lacks dop_rho_vector: this fit has a DOP block')
                state['dop_rho_vector'] = plan.get('dop_rho').copy()
                state['dop_rho_vector'][b] = dop_rho
        if weights is not None and plan.B > 1:
            w = plan.get('est_weights').copy()
            w[b] = weights
            weights = w
        out, terms = self.evaluate_lml_batch(weights=weights, update_hypers=update_hypers, state=state, return_terms=True)
        if terms['status'][b] == _ffi.PREDICT_NOT_PD:
            which = 'posterior' if np.isnan(terms['logdet_p'][b]) else 'prior'
            raise ValueError(f'Determinant of {which} covariance matrix is negative - not PSD')
        return float(out[b])

    # the tables generate_candidates left (drt1d.py:2383-2500); discrete element models are not built
    def get_candidate_df(self, candidate_type):
        if candidate_type == 'continuous':
            return getattr(self, 'best_candidate_df', None)
        if candidate_type in ('discrete', 'pfrt'):
            raise NotImplementedError(f'candidate_type {candidate_type!r}: discrete element models are not built')
        raise ValueError(f'Invalid candidate_type {candidate_type}')

    def get_candidate(self, candidate_num_peaks, candidate_type):
        if candidate_type in ('discrete', 'pfrt'):
            raise NotImplementedError(f'candidate_type {candidate_type!r}: discrete element models are not built')
        if candidate_type != 'continuous':
            raise ValueError(f"Invalid candidate_type {candidate_type}. Options: 'continuous', 'discrete', 'pfrt'")
        if getattr(self, 'best_candidate_dict', None) is None:
            raise ValueError('Candidates must be first be generated using generate_candidates')
        try:
            return self.best_candidate_dict[candidate_num_peaks]
        except KeyError:
            raise ValueError(f'No candidate with {candidate_num_peaks} peaks exists')

    def evaluate_norm_bayes_factors(self, candidate_type, criterion=None, candidate_id=None, na_val=None):
        df = self.get_candidate_df(candidate_type)
        if df is None:
            raise ValueError('Candidates must be first be generated using generate_candidates')
        criterion = 'bic' if criterion is None else criterion
        if criterion not in df:
            candidates.norm_bayes_factors(np.zeros(1), criterion)        # (an invalid criterion is stats' ValueError)
            raise NotImplementedError(_no_column(criterion))
        bf = candidates.norm_bayes_factors(df[criterion], criterion)
        if candidate_id is None:
            return bf
        index = np.where(df['model_id'] == candidate_id)
        # (upstream tests len() of where's TUPLE, which is never 0, so its na_val is dead and an unknown id gives an empty array;
        # here na_val is returned for an unknown id, as the argument is meant)
        if na_val is not None and len(index[0]) == 0:
            return na_val
        return bf[index]

    def evaluate_bayes_factor(self, candidate_id_1, candidate_id_2, candidate_type='discrete', criterion=None):
        criterion = 'bic' if criterion is None else criterion
        c1, c2 = self.get_candidate(candidate_id_1, candidate_type), self.get_candidate(candidate_id_2, candidate_type)
        if criterion not in c1:
            candidates.bayes_factor(0.0, 0.0, criterion)
            raise NotImplementedError(_no_column(criterion))
        return candidates.bayes_factor(c1[criterion], c2[criterion], criterion)

    def get_best_candidate_id(self, candidate_type, criterion=None):
        if candidate_type == 'discrete':
            raise NotImplementedError("candidate_type 'discrete': discrete element models are not built")
        if candidate_type != 'continuous':
            raise ValueError(f"Invalid candidate_type {candidate_type}. Options: ['discrete', 'continuous']")
        directions = {'bic': -1, 'lml': 1, 'lml-bic': 1}
        if criterion is not None and criterion not in directions:
            raise ValueError(f'Invalid criterion {criterion}. Options: {directions.keys()}')
        criterion = 'bic' if criterion is None else criterion
        df = self.get_candidate_df('continuous')
        if df is None:
            raise ValueError('Candidates must be first be generated using generate_candidates')
        if criterion not in df:
            raise NotImplementedError(_no_column(criterion))
        values = df[criterion] * directions[criterion]
        return df['model_id'][np.argmax(values)]

    # ---- PFRT (drt1d.py:2558-2715) ----------------------------------------------------------------------------------------
    def evaluate_step_llh_batch(self, alpha_0=2, beta_0=1):
        """evaluate_llh(weights=estimate_weights(x), x) (drt1d.py:2618-2622) for the current x of every spectrum of
        the batch: residuals, re-estimated weights and both sums on the device, the two lgamma constants here."""
        rss, slw = self._plan.llh_terms()
        return qphb.marginal_llh(rss, self._plan.m, alpha_0, beta_0) + slw

    def _pfrt_steps(self, factors, step_hypers, out, restart, after_init=None):
        """The PFRT step loop on the plan that holds the full fit at factors[0], whose result dict is ``out``: one
        ``restart(**step_hypers(f))`` per further factor.  Every step's final state stays on the device for predict_pfrt_batch /
        step_p_matrix (hipdrt_plan_pfrt_begin / _record); its step log-likelihood comes from weights re-estimated on the
        current iterate alone.  ``after_init(out)`` runs between the first step's record and the first restart (what DRTMD reads
        from the FIRST step's fit: its P matrix, llh / rss -- mapping).  Leaves pfrt_result {'factors', 'step_x' (S, B, n)
        scaled-space solutions, 'step_llh' (S, B), 'step_iters' (S, B), 'status' (B,)} and returns the last step's result dict."""
        plan = self._plan
        plan.pfrt_begin(len(factors))
        steps, status = [], None
        for i, f in enumerate(factors):
            res = restart(**step_hypers(f)) if i else out
            plan.pfrt_record()
            steps.append((res['x'].copy(), self.evaluate_step_llh_batch(), res['outer_iters'].copy()))
            status = combine_status(status, res['status']) if i else np.array(res['status']).copy()
            if i == 0 and after_init is not None:
                after_init(out)
        step_x, step_llh, step_iters = (np.array(a) for a in zip(*steps))
        self.pfrt_result = {'factors': factors, 'step_x': step_x, 'step_llh': step_llh, 'step_iters': step_iters, 'status': status}
        return res

    def pfrt_fit_eis_batch(self, frequencies, z_batch, factors=None, max_iter_per_step=10, max_init_iter=20,
                           xtol=1e-2, nonneg=True, after_init=None, **kw):
        """DRT.pfrt_fit_eis (drt1d.py:2558-2690) for B spectra at once: a full fit at the first regularisation factor
        (s_0 * f, l2_lambda_0 / f), then one warm restart per further factor on the device.  Returns pfrt_result with
        the last step's 'coefficient_scale' (B,) and 'basis_tau' added."""
        factors, step_hypers = pfrt_schedule(factors, kw)
        out = self.fit_eis_batch(frequencies, z_batch, nonneg=nonneg, max_iter=max_init_iter, xtol=xtol,
                                 **dict(kw, **step_hypers(factors[0])))
        last = self._pfrt_steps(factors, step_hypers, out, after_init=after_init, restart=lambda **hypers:
                                self.continue_from_init(xtol=xtol, max_iter=max_iter_per_step, **hypers))
        self.pfrt_result.update(coefficient_scale=last['coefficient_scale'], basis_tau=last['basis_tau'])
        return self.pfrt_result

    def _pfrt_prepared(self, measurements, factors, max_iter_per_step, max_init_iter, xtol, nonneg, kw, after_init=None):
        """DRT._pfrt_fit_core (drt1d.py:2558-2700) on a prepared plan: the full fit at factors[0], one warm restart per
        further factor with the fit's own chrono / eis weight factors (2660-2668), which all measurements must share.  A
        single measurement is stored as its fit stores it (fit_parameters / qphb_params / qphb_history of the first step)
        and leaves pfrt_history, every recorded iterate of every step.  Returns what _fit_prepared returned."""
        factors, step_hypers = pfrt_schedule(factors, kw)
        single = len(measurements) == 1
        history_of = 0 if single else -1
        fitted = self._fit_prepared(measurements, dict(kw, nonneg=nonneg, max_iter=max_init_iter, xtol=xtol,
                                                       **step_hypers(factors[0])), history_of=history_of)
        preps, out = fitted[0], fitted[1]
        if single:
            self._store_single(*fitted, 'qphb_hybrid' if preps[0]['num_eis'] and preps[0]['num_chrono'] else
                               ('qphb_chrono' if preps[0]['num_chrono'] else 'qphb_eis'))
        else:
            self._last_prepared = (preps, None)
        history = []

        def first(out):
            if single:
                history.append(self._plan.history())
            if after_init is not None:
                after_init(out)

        def restart(**hypers):
            pairs = {(float(pr['chrono_weight_factor']), float(pr['eis_weight_factor'])) for pr in preps}
            if len(pairs) > 1:
                raise NotImplementedError('per-measurement chrono / eis weight factors in a PFRT batch')
            (cf, ef), = pairs
            res = self.continue_from_init(xtol=xtol, max_iter=max_iter_per_step, history_of=history_of,
                                          chrono_weight_factor=cf, eis_weight_factor=ef, **hypers)
            if single:
                history.append(res['history'])
            return res
        self._pfrt_steps(factors, step_hypers, out, restart, after_init=first)
        if single:
            self.pfrt_history = [dict(x=h['x'][i], rho_vector=h['rho'][i], weights=h['weights'][i],
                                      dop_rho_vector=h['dop_rho'][i] if 'dop_rho' in h else None)
                                 for h in history for i in range(len(h['x']))]
        return fitted

    def pfrt_fit_hybrid(self, times, i_signal, v_signal, frequencies, z, factors=None, max_iter_per_step=10,
                        max_init_iter=20, xtol=1e-2, nonneg=True, **kw):
        """DRT.pfrt_fit_hybrid (drt1d.py:2705-2715): leaves fit_parameters / qphb_params of the LAST step's state as a fit
        does, pfrt_result {'factors', 'step_x' (S, 1, n), 'step_llh' (S, 1), 'step_iters' (S, 1)} and pfrt_history."""
        self._pfrt_prepared([(times, i_signal, v_signal, frequencies, z)], factors, max_iter_per_step, max_init_iter, xtol,
                            nonneg, kw)
        self.fit_type = 'qphb_hybrid'
        return self.pfrt_result

    def pfrt_fit_chrono(self, times, i_signal, v_signal, factors=None, max_iter_per_step=10, max_init_iter=20,
                        xtol=1e-2, nonneg=True, error_structure='uniform', vmm_epsilon=4, **kw):
        """DRT.pfrt_fit_chrono (drt1d.py:2699-2703)"""
        self._pfrt_prepared([(times, i_signal, v_signal, None, None)], factors, max_iter_per_step, max_init_iter, xtol,
                            nonneg, dict(kw, chrono_error_structure=error_structure, chrono_vmm_epsilon=vmm_epsilon))
        self.fit_type = 'qphb_chrono'
        return self.pfrt_result

    def pfrt_fit_hybrid_batch(self, times, i_batch, v_batch, frequencies, z_batch, factors=None, max_iter_per_step=10,
                              max_init_iter=20, xtol=1e-2, nonneg=True, **kw):
        """pfrt_fit_hybrid for B joint measurements of one protocol at once (what DRTMD with fit_type='pfrt' loops over,
        drtmd.py:98-100, 1338): step_x (S, B, n), step_llh (S, B), step_iters (S, B)."""
        meas = [(times, i_batch[b], v_batch[b], frequencies, z_batch[b]) for b in range(len(z_batch))]
        fitted = self._pfrt_prepared(meas, factors, max_iter_per_step, max_init_iter, xtol, nonneg, kw)
        self._last_prepared = (fitted[0], None)
        return self.pfrt_result
