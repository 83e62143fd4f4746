"""Everything of DRT that re-enters the device loop on a finished fit, for both plan kinds (the EIS plan of fit_eis /
fit_eis_batch and the prepared-matrix plan of chrono / joint / DOP fits): the warm restart (DRT._continue_from_init,
drt1d.py:1270-1365), the candidate generators on top of it (1497-1632) and the PFRT step loop (_pfrt_fit_core, 2558-2715).
The flow is written once; where the kinds differ -- the finished-fit check, the keyword split, the row factors and dop_rho of
a prepared plan, what is collected -- the difference is one named piece."""
import numpy as np

from .. import _ffi
from . import qphb


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
                           xtol=1e-2, max_iter=10, min_iter=2, history_of=-1, dop_rho_vector=None, **kw):
        """DRT._continue_from_init for the last fit (EIS, chrono, joint, DOP; single or batch): the outer loop re-entered on
        the device from the given state (arrays with a leading batch axis; None = the state left by the previous call) with
        ``kw`` updating the hyper-parameters (e.g. s_0, l2_lambda_0).  est_weights, xmx / dop_xmx norms and the data scale
        stay as fitted.  A prepared plan also takes ``chrono_weight_factor`` / ``eis_weight_factor`` (restart_row_factors: they
        multiply the weights at the top of every iteration together with ``weight_factor``) and ``dop_rho_vector``, and rewrites
        its vz_offset column after every iteration from a copy of the matrix frozen at entry (1295-1298).  Returns the arrays
        of _collect_restart (outer_iters = iterations of this call), plus ``history`` of member ``history_of`` when that is >= 0."""
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
