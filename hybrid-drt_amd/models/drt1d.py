"""Drop-in for the EIS fit path of hybdrt.models.DRT (hybdrt/models/drt1d.py + drtbase.py).

``DRT(**ctor).fit_eis(frequencies, z, **hypers)`` leaves ``fit_parameters``, ``qphb_params``,
``qphb_history`` populated like the reference; ``fit_eis_batch`` is the batched form the reference runs as a
serial loop in DRTMD.fit_observations (hybdrt/mapping/drtmd.py:303-319).  All arithmetic -- lookup tables,
Z'/Z'' and penalty matrices, the QPHB loop -- runs in libhipdrt.so on one MI355X; this module only decides
grids and options and rescales results (host logic mirrored from the reference, cited per method).  The methods that act on a
finished fit (prediction, peaks, PFRT, covariances) are postfit.PostFitMixin; chrono / joint / DOP fits prepared.PreparedFitMixin;
what re-enters the device loop on a finished fit (warm restarts, candidates, the PFRT fits) restart.RestartMixin."""
import warnings

import numpy as np

from .. import _ffi, preprocessing as pp
from ..matrices import mat1d
from ..utils.array import is_uniform
from . import kk, qphb
from .postfit import PostFitMixin
from .prepared import PreparedFitMixin
from .restart import RestartMixin

_FIT_KW_DEFAULTS = dict(  # DRT._qphb_fit_core keyword defaults (drt1d.py:102-137) that the device loop honours
    nonneg=True, scale_data=True, ohmic_penalty=1e-6, inductance_penalty=1e-6, inductance_scale=1e-5,
    capacitance_penalty=1e-6, capacitance_scale=1e-3, update_scale=False,
    penalty_type='integral', eis_error_structure=None, eis_vmm_epsilon=0.25, eis_reim_cor=0.25,
    iw_l1_lambda_0=1e-4, iw_l2_lambda_0=1e-4, eff_hp=True, weight_factor=1, xtol=1e-2, max_iter=50)


class DRT(PreparedFitMixin, PostFitMixin, RestartMixin):
    def __init__(self, fixed_basis_tau=None, tau_supergrid=None, tau_basis_type='gaussian', tau_epsilon=None,
                 basis_tau_ppd=10, extend_basis_decades=1, interpolate_integrals=True, fit_dop=False,
                 fit_inductance=True, fit_ohmic=True, fit_capacitance=False, frequency_precision=10,
                 fixed_basis_nu=None, nu_basis_type='gaussian', nu_epsilon=None, normalize_dop=True,
                 step_model='ideal', chrono_mode='galv',
                 print_diagnostics=False, warn=True, device=0, context=None):
        """DRTBase.__init__ (hybdrt/models/drtbase.py:21-159): epsilon rule and the lookup tables."""
        if tau_basis_type != 'gaussian':
            raise NotImplementedError("only the default gaussian basis is on the hot path")
        if nu_basis_type != 'gaussian' or not normalize_dop:
            raise NotImplementedError("only the default gaussian, normalised distribution of phasances is built")
        if step_model != 'ideal' or chrono_mode != 'galv':
            raise NotImplementedError("only ideal galvanostatic steps are built")
        self.basis_nu = None if fixed_basis_nu is None else np.asarray(fixed_basis_nu, dtype=float)
        self.nu_epsilon = nu_epsilon
        if fixed_basis_tau is not None and tau_supergrid is not None:
            warnings.warn('If fixed_basis_tau is provided, tau_supergrid will be ignored')
        self.fixed_basis_tau = None if fixed_basis_tau is None else np.asarray(fixed_basis_tau, dtype=float)
        self.tau_supergrid = None if tau_supergrid is None else np.asarray(tau_supergrid, dtype=float)
        self.tau_basis_type = tau_basis_type
        self.tau_epsilon = tau_epsilon
        self.extend_basis_decades = extend_basis_decades
        self.fit_inductance, self.fit_ohmic, self.fit_capacitance, self.fit_dop = fit_inductance, fit_ohmic, bool(fit_capacitance), bool(fit_dop)
        self.frequency_precision = frequency_precision
        self.print_diagnostics, self.warn = print_diagnostics, warn
        self.device = device
        self._context = context          # optional private hipdrt context (own HIP stream): lets several
                                         # DRT instances keep batches in flight concurrently on one GPU
        if self.tau_epsilon is None:
            if self.fixed_basis_tau is not None:
                self.tau_epsilon = 1 / np.mean(np.diff(np.log(self.fixed_basis_tau)))
            elif self.tau_supergrid is not None:
                self.tau_epsilon = 1 / np.mean(np.diff(np.log(self.tau_supergrid)))
            elif basis_tau_ppd is not None:
                self.tau_epsilon = pp.get_epsilon_from_ppd(basis_tau_ppd)
        self.integrate_method = 'interp' if interpolate_integrals else 'trapz'
        # lookup abscissae (basis.py:653-657); the ordinates are produced on the device inside the plan
        self._wt_re = np.logspace(-2.7, 2.7, 2000)
        self._wt_im = np.logspace(-5.4, 5.4, 2000)
        self._plan = None
        self._plan_key = None
        self._last_batch = None
        self.basis_tau = None
        self.special_qp_params = {}
        self.fit_parameters = None
        self.qphb_params = None
        self.qphb_history = None
        self.cvx_result = None
        self.fit_kwargs = None
        self.fit_type = None
        self.coefficient_scale = 1.0
        self.impedance_scale = 1.0
        self.inductance_scale = None
        self.f_fit = []

    # ---- plan management (the counterpart of the reference's matrix recalc cache, drtbase.py:1008-1032) ----
    @property
    def interpolate_lookups(self):
        if self._plan is None or self.integrate_method != 'interp':
            return {'z_real': None, 'z_imag': None}
        p = self._plan
        return {'z_real': (p.log_wt_re, p.get('lut_z_re')), 'z_imag': (p.log_wt_im, p.get('lut_z_im'))}

    def _special_params(self):
        """drt1d.py:375-408 / drtbase.py:538-547 for an EIS fit."""
        sp = {}
        if self.fit_ohmic:
            sp['R_inf'] = {'index': len(sp), 'nonneg': True, 'size': 1}
        if self.fit_inductance:
            sp['inductance'] = {'index': len(sp), 'nonneg': True, 'size': 1}
        return sp

    def _get_plan(self, frequencies, opts, capacity):
        if self.fixed_basis_tau is not None:
            basis_tau = self.fixed_basis_tau
        else:
            basis_tau = pp.get_basis_tau(frequencies, None, None, tau_grid=self.tau_supergrid,
                                         extend_decades=self.extend_basis_decades)
        if self.tau_epsilon is None:
            self.tau_epsilon = 1 / np.mean(np.diff(np.log(basis_tau)))
        key = (np.asarray(frequencies).tobytes(), basis_tau.tobytes(), float(self.tau_epsilon), bytes(opts))
        if self._plan is not None and self._plan_key == key and self._plan.capacity >= capacity:
            return self._plan
        if self._plan is not None:
            self._plan.close()
        mode = _ffi.MODE_INTERP if self.integrate_method == 'interp' else _ffi.MODE_TRAPZ
        tpl_a = mat1d.impedance_matrix_is_toeplitz(frequencies, basis_tau, self.frequency_precision)
        tpl_m = is_uniform(np.log(basis_tau))
        ctx = self._context if self._context is not None else _ffi.get_context(self.device)
        self._plan = _ffi.Plan(ctx, frequencies, basis_tau, self.tau_epsilon,
                               wt_re=self._wt_re, wt_im=self._wt_im, mode=mode, toeplitz_a=tpl_a, toeplitz_m=tpl_m,
                               opts=opts, capacity=capacity)
        self._plan_key = key
        self.basis_tau = basis_tau
        sub = getattr(self, 'plan_subbatches', None)      # None: the library's choice (hipdrt_plan_set_subbatches(0))
        if sub is not None:
            self._plan.set_subbatches(sub)
        if getattr(self, '_luts_installed', False) and getattr(self, '_lut_key', None) == float(self.tau_epsilon):
            (_, z_re), (_, z_im) = self._luts['z']          # tables received from another rank (install_lookup_tables)
            self._plan.set_lookup(z_re, z_im)
        return self._plan

    def lookup_tables(self):
        """(z_re, z_im, response) ordinates of the three lookup tables of this instance's epsilon (drtbase.py:138-156),
        built on the device (PreparedFitMixin._lookups)."""
        ctx = self._context if self._context is not None else _ffi.get_context(self.device)
        luts = self._lookups(ctx)
        return luts['z'][0][1], luts['z'][1][1], luts['response'][1]

    def install_lookup_tables(self, z_re, z_im, response):
        """Use tables built elsewhere (rank 0 of a sharded map, mapping.share_lookup_tables) instead of building them:
        prepared-matrix fits read them from here, EIS plans receive them right after they are created."""
        td = np.logspace(-6, 2, 2000)
        self._luts = dict(z=((np.log(self._wt_re), np.asarray(z_re, dtype=float)), (np.log(self._wt_im), np.asarray(z_im, dtype=float))),
                          response=(np.log(td), np.asarray(response, dtype=float)))
        self._lut_key = float(self.tau_epsilon)
        self._luts_installed = True
        if self._plan is not None and hasattr(self._plan, 'set_lookup'):
            self._plan.set_lookup(z_re, z_im)

    def _make_opts(self, fit_kw):
        kw = dict(_FIT_KW_DEFAULTS)
        hypers = qphb.get_default_hypers(bool(fit_kw.get('eff_hp', True)), self.fit_dop, 'gaussian')
        for key, val in fit_kw.items():
            if key in kw:
                kw[key] = val
            elif key in hypers:
                hypers[key] = val
            else:
                raise ValueError(f'Invalid keyword argument {key}')     # drt1d.py:415-419
        if kw['penalty_type'] != 'integral':
            raise NotImplementedError("penalty_type 'discrete' is deprecated in the reference and not built")
        if (hypers['iw_alpha'] is None) != (hypers['iw_beta'] is None):
            raise ValueError('iw_alpha and iw_beta must be given together')
        if kw['eis_error_structure'] not in (None, 'uniform'):
            raise ValueError(f"Invalid eis_error_structure {kw['eis_error_structure']}")
        o = _ffi.default_fit_opts()
        o.rp_scale = float(hypers['rp_scale'])
        for name in ('derivative_weights', 'sigma_ds', 's_alpha', 's_0', 'rho_alpha', 'rho_0'):
            vals = np.broadcast_to(np.asarray(hypers[name], dtype=float), (3,))
            for k in range(3):
                getattr(o, name)[k] = float(vals[k])
        o.l1_lambda_0, o.l2_lambda_0 = float(hypers['l1_lambda_0']), float(hypers['l2_lambda_0'])
        # optional branches of the weight estimation (None <-> -1)
        o.outlier_p = -1.0 if hypers['outlier_p'] is None else float(hypers['outlier_p'])
        o.iw_alpha = -1.0 if hypers['iw_alpha'] is None else float(hypers['iw_alpha'])
        o.iw_beta = -1.0 if hypers['iw_beta'] is None else float(hypers['iw_beta'])
        o.iw_l1_lambda_0, o.iw_l2_lambda_0 = float(kw['iw_l1_lambda_0']), float(kw['iw_l2_lambda_0'])
        o.ohmic_penalty, o.inductance_penalty = float(kw['ohmic_penalty']), float(kw['inductance_penalty'])
        o.inductance_scale = float(kw['inductance_scale'])
        o.eis_vmm_epsilon, o.eis_reim_cor = float(kw['eis_vmm_epsilon']), float(kw['eis_reim_cor'])
        o.xtol, o.max_iter = float(kw['xtol']), int(kw['max_iter'])
        o.nonneg, o.scale_data = int(bool(kw['nonneg'])), int(bool(kw['scale_data']))
        o.fit_ohmic, o.fit_inductance = int(self.fit_ohmic), int(self.fit_inductance)
        o.eis_error_uniform = int(kw['eis_error_structure'] == 'uniform')
        o.update_scale = int(bool(kw['update_scale']))
        o.eff_hp = int(bool(kw['eff_hp']))
        return o, hypers, kw

    # ---- the fits ------------------------------------------------------------------------------------------
    def _qphb_fit_core(self, times, i_signal, v_signal, frequencies, z, **kw):
        """DRT._qphb_fit_core(times, i_signal, v_signal, frequencies, z, **fit_kw) (drt1d.py:102-137), the call
        DRTMD.fit_observation makes as ``drt1d._qphb_fit_core(*chrono_data, *eis_data, **fit_kw)`` (drtmd.py:253): which
        data are None selects the EIS, chrono or joint fit, with the keyword names of _qphb_fit_core itself."""
        has_chrono = times is not None
        has_eis = frequencies is not None
        if not has_chrono and not has_eis:
            raise ValueError('At least one of (times, i_signal, v_signal) and (frequencies, z) must be provided')
        if has_chrono and (i_signal is None or v_signal is None):
            raise ValueError('times, i_signal and v_signal must be provided together')     # utils.validation.check_chrono_data
        if has_eis and z is None:
            raise ValueError('frequencies and z must be provided together')                # utils.validation.check_eis_data
        if not has_chrono:
            return self.fit_eis(frequencies, z, **kw)
        if not has_eis:
            kw = dict(kw)
            for core, own in (('chrono_error_structure', 'error_structure'), ('chrono_vmm_epsilon', 'vmm_epsilon')):
                if core in kw:
                    kw[own] = kw.pop(core)
            for eis_only in ('eis_error_structure', 'eis_vmm_epsilon', 'eis_reim_cor'):
                kw.pop(eis_only, None)
            return self.fit_chrono(times, i_signal, v_signal, **kw)
        return self.fit_hybrid(times, i_signal, v_signal, frequencies, z, **kw)

    def fit_eis(self, frequencies, z, **kw):
        """DRT.fit_eis (drt1d.py:1215-1241) -> _qphb_fit_core (102-1104) for one spectrum."""
        frequencies = np.asarray(frequencies, dtype=float)
        z = np.asarray(z, dtype=complex)
        if len(frequencies) != len(z):
            raise ValueError('Length of frequencies and z must be equal')    # utils/validation.check_eis_data
        kw = dict(kw)
        for old, new in (('error_structure', 'eis_error_structure'), ('vmm_epsilon', 'eis_vmm_epsilon'),
                         ('vmm_reim_cor', 'eis_reim_cor')):     # fit_eis's own keyword names (drt1d.py:1215-1241)
            if old in kw:
                kw[new] = kw.pop(old)
        if self.fit_dop or self.fit_capacitance or kw.get('solve_rp') or kw.get('remove_outliers') \
                or kw.get('remove_extremes') or kw.get('neg_allowed_tau_range') is not None \
                or kw.get('series_neg'):   # prepared-matrix plan
            return self._store_single(*self._fit_prepared([(None, None, None, frequencies, z)], kw, history_of=0),
                                      'qphb_eis')
        res = self._fit(frequencies, z[None, :], kw, history_of=0)
        b = 0
        fp = {'x': res['fit_x'][b], 'R_inf': res['R_inf'][b] if self.fit_ohmic else 0,
              'inductance': res['inductance'][b] if self.fit_inductance else 0, 'C_inv': 0,
              'v_sigma_tot': None, 'v_sigma_res': None, 'z_sigma_tot': res['z_sigma_tot'][b], 'vz_offset_eps': 1,
              'p_matrix': self._plan.p_matrix(b), 'q_vector': res['q_vector'][b]}
        if res['status'][b] < 0:
            raise ValueError("Rank(A) < p or Rank([P; A; G]) < n")          # cvxopt's error at the QP start point
        if res['status'][b] == 1 and self.warn:
            warnings.warn(f"Solution did not converge within {self.fit_kwargs['max_iter']} iterations. "
                          f"This is usually not an issue.")
        self.fit_parameters = fp
        self.coefficient_scale = self.impedance_scale = float(res['coefficient_scale'][b])
        hist = self._plan.history()
        self.qphb_history = [{'x': hist['x'][i], 'rho_vector': hist['rho'][i], 'weights': hist['weights'][i]}
                             for i in range(len(hist['x']))]
        self.qphb_params = {'weights': res['weights'][b], 'true_weights': res['weights'][b],
                            'rho_vector': res['rho'][b], 's_vectors': list(res['s_vectors'][b]),
                            'p_matrix': fp['p_matrix'], 'q_vector': fp['q_vector'], 'rm': self._plan.get('rm'),
                            'vmm': self._plan.get('vmm'), 'num_eis': len(frequencies), 'num_chrono': 0,
                            'qp_iterations': hist['qp_iterations'], 'outer_iterations': int(res['outer_iters'][b]),
                            'est_weights': self._plan.get('est_weights')[b], 'rv': self._plan.get('rv')[b]}
        self.cvx_result = {'x': res['x'][b]}
        self.fit_type = 'qphb_eis'
        return fp

    def fit_eis_batch(self, frequencies, z_batch, **kw):
        """B spectra on one frequency grid, fitted concurrently (the reference's DRTMD loop calls
        _qphb_fit_core once per observation, mapping/drtmd.py:245-319).  Returns a dict of arrays."""
        frequencies = np.asarray(frequencies, dtype=float)
        z_batch = np.asarray(z_batch, dtype=complex)
        if z_batch.ndim != 2 or z_batch.shape[1] != len(frequencies):
            raise ValueError('z_batch must have shape (B, len(frequencies))')
        if self.fit_dop or self.fit_capacitance or kw.get('solve_rp'):
            return self._fit_prepared_batch([(None, None, None, frequencies, zb) for zb in z_batch], kw)
        return self._fit(frequencies, z_batch, kw, history_of=-1)

    # staged form: inputs made resident in HBM once, the fit launched separately (what bench.py times)
    def stage_batch(self, frequencies, z_batch, history_of=-1, **kw):
        frequencies = np.asarray(frequencies, dtype=float)
        z_batch = np.asarray(z_batch, dtype=complex)
        opts, hypers, fkw = self._make_opts(kw)
        plan = self._get_plan(frequencies, opts, z_batch.shape[0])
        self.special_qp_params = self._special_params()
        self.inductance_scale = fkw['inductance_scale']
        self.fit_kwargs = dict(hypers, **fkw)
        self.f_fit = frequencies
        plan.record_history(history_of)
        wf = fkw['weight_factor']
        if np.ndim(wf) > 0:       # vector-valued weight_factor (drt1d.py:889-901): one factor per data row
            plan.set_weight_factors(1.0, np.asarray(wf, dtype=float), late=True)
        else:
            plan.set_weight_factors(wf)
        plan.upload(z_batch)
        self._last_batch = z_batch.shape[0]
        return plan

    def fit_staged(self):
        self._plan.fit()

    def collect_staged(self):
        plan = self._plan
        frequencies = self.f_fit
        if getattr(self, 'collect_fields', None) == 'map':
            # a map keeps, per observation, the distribution, the special parameters, llh / rss and the counts (drtmd.py:245-301):
            # the solution in scaled units, weights, rho, s vectors and q stay on the device (mapping.fit_observations_sharded)
            res = plan.download(lean=True)
        else:
            res = plan.download(s_vectors=True)
            nf = len(frequencies)
            sigma = 1.0 / res['weights']
            res['z_sigma_tot'] = (sigma[:, :nf] + 1j * sigma[:, nf:]) * res['coefficient_scale'][:, None]
        res['basis_tau'] = self.basis_tau
        res['timings_ms'], res['launches'] = plan.timings()
        return res

    def evaluate_obs_llh_rss_batch(self, llh_kw=None, rss_kw=None):
        """(DRT.evaluate_llh(**llh_kw), DRT.evaluate_rss(**rss_kw)) (drt1d.py:4433-4496; x = the last iterate) for every
        spectrum of the last fitted batch -- what DRTMD.fit_observation stores as obs_llh / obs_rss (drtmd.py:259-260).
        Keys as upstream: ``weights`` (None = the fit's est_weights, 'uniform' = per-domain means of them, a scalar),
        ``normalize`` (divide by the number of data rows), and for the likelihood ``marginalize_weights``, ``alpha_0``,
        ``beta_0``.  Residuals and all sums on the device."""
        llh_kw, rss_kw = dict(llh_kw or {}), dict(rss_kw or {})
        bad = (set(llh_kw) - {'weights', 'normalize', 'marginalize_weights', 'alpha_0', 'beta_0', 'subtract_background'}) | \
              (set(rss_kw) - {'weights', 'normalize'})
        if bad:
            raise TypeError(f"unexpected keyword(s) {sorted(bad)}")
        m = self._plan.m
        terms = {}

        def sums(weights):
            key = weights if (weights is None or isinstance(weights, str)) else float(weights)
            if key not in terms:
                terms[key] = self._plan.llh_terms(stored=True, weights=weights)
            return terms[key]

        rss_l, slw = sums(llh_kw.get('weights'))
        alpha_0, beta_0 = llh_kw.get('alpha_0', 2), llh_kw.get('beta_0', 1)
        llh = qphb.marginal_llh(rss_l, m, alpha_0, beta_0) if llh_kw.get('marginalize_weights', True) else -0.5 * rss_l
        llh = llh + slw
        if llh_kw.get('normalize', False):
            llh = llh / m
        rss = sums(rss_kw.get('weights'))[0].copy()
        if rss_kw.get('normalize', False):
            rss /= m
        return llh, rss

    series_neg = False

    def _llh_weights(self, weights):
        """the `weights` argument of evaluate_rss / evaluate_llh (drt1d.py:4434-4443, 4459-4472)"""
        est = self.qphb_params['est_weights']
        if weights is None:
            return est
        if isinstance(weights, str):
            if weights != 'uniform':
                raise ValueError(f"weights must be None, 'uniform', a scalar or an array, got {weights!r}")
            nc = int(self.qphb_params.get('num_chrono', 0) or 0)
            w = np.empty(len(est))
            if nc:
                w[:nc] = np.mean(est[:nc])
            w[nc:] = np.mean(est[nc:])
            return w
        if np.isscalar(weights):
            return np.ones_like(est) * weights
        w = np.asarray(weights, dtype=float)
        if w.shape != est.shape:
            raise ValueError('Expected weights array of shape {}, but received shape {}'.format(est.shape, w.shape))
        return w

    def evaluate_rss(self, weights=None, x=None, normalize=False):
        """drt1d.evaluate_rss (drt1d.py:4433-4455) -> qphb.evaluate_rss (qphb.py:1347-1352)."""
        w = self._llh_weights(weights)
        x = self.qphb_history[-1]['x'] if x is None else x
        rm, rv = self.qphb_params['rm'], self.qphb_params['rv']
        wrm, wrv = w[:, None] * rm, w * rv
        rss = x @ wrm.T @ wrm @ x - 2 * wrv.T @ wrm @ x + wrv.T @ wrv
        return rss / len(rv) if normalize else rss

    def evaluate_llh(self, weights=None, x=None, marginalize_weights=True, alpha_0=2, beta_0=1, normalize=False):
        """drt1d.evaluate_llh (drt1d.py:4457-4496) -> qphb.evaluate_llh (qphb.py:1355-1377)."""
        w = self._llh_weights(weights)
        rss = self.evaluate_rss(w, x)
        llh = qphb.marginal_llh(rss, len(w), alpha_0, beta_0) if marginalize_weights else -0.5 * rss
        llh = llh + np.sum(np.log(w))
        return llh / len(w) if normalize else llh

    def _fit(self, frequencies, z_batch, kw, history_of):
        self.stage_batch(frequencies, z_batch, history_of=history_of, **kw)
        self.fit_staged()
        return self.collect_staged()

    # ---- Kramers-Kronig test (drt1d.py:1370-1491) ------------------------------------------------------------------------
    def get_fit_frequencies(self):
        """DRTBase.get_fit_frequencies for an EIS fit: the frequencies of the last fit"""
        return np.asarray(self.f_fit, dtype=float)

    def _kk_plan(self):
        if self._plan is None or self._last_batch is None or isinstance(self._plan, _ffi.PreparedPlan):
            raise NotImplementedError('the Kramers-Kronig screen needs a finished plain EIS fit (fit_eis / fit_eis_batch '
                                      'without fit_dop, fit_capacitance, solve_rp or outlier removal)')
        return self._plan

    @staticmethod
    def _kk_opts(n_outlier_iter=2, p_thresh=1e-4, n_sigma=None, std_sample_fraction=0.6, max_num_outliers=2):
        if std_sample_fraction > 1 or std_sample_fraction <= 0:
            raise ValueError('sample_fraction must be no greater than 1')              # stats.robust_std
        return _ffi.kk_opts(n_outlier_iter=n_outlier_iter, p_thresh=p_thresh, n_sigma=n_sigma,
                            std_sample_fraction=std_sample_fraction,
                            n_std=kk.std_normal_quantile(0.5 + std_sample_fraction / 2), max_num_outliers=max_num_outliers)

    def predict_z(self, frequencies):
        """DRT.predict_z at the FIT frequencies only: rm @ x of the fitted spectrum, in data units, formed on the device
        (hipdrt_plan_kk_screen).  Any other frequencies raise NotImplementedError."""
        plan = self._kk_plan()
        f = np.asarray(frequencies, dtype=float)
        if f.shape != np.shape(self.f_fit) or not np.array_equal(f, self.f_fit):
            raise NotImplementedError('predict_z is built for the fit frequencies only (get_fit_frequencies())')
        return plan.kk_screen(self._kk_opts(), residuals=False)['z_hat'][0]

    def eval_kk_residuals(self, norm='modulus'):
        """DRT.eval_kk_residuals (drt1d.py:1472-1481): 100 (z - z_hat) / |z| at the fit frequencies, from the device"""
        if norm != 'modulus':
            raise ValueError(f'norm must be "modulus", got {norm!r}')
        return self._kk_plan().kk_screen(self._kk_opts(), z_hat=False)['residuals'][0]

    def get_kk_outliers(self, norm='modulus', n_iter=2, p_thresh=1e-4, n_sigma=None, std_sample_fraction=0.6):
        """DRT.get_kk_outliers (drt1d.py:1483-1486): indices of the outliers of the last fit's residuals, from the device"""
        if norm != 'modulus':
            raise ValueError(f'norm must be "modulus", got {norm!r}')
        self._kk_last = dict(n_outlier_iter=n_iter, p_thresh=p_thresh, n_sigma=n_sigma, std_sample_fraction=std_sample_fraction)
        res = self._kk_plan().kk_screen(self._kk_opts(**self._kk_last), z_hat=False, residuals=False)
        if res['status'][0] < 0:
            raise ValueError('the fit of this spectrum failed: there are no residuals to screen')
        return np.where(res['outlier_mask'][0] != 0)[0]

    def get_kk_limits(self, outlier_index, max_num_outliers=2):
        """DRT.get_kk_limits (drt1d.py:1488-1491): (f_min, f_max) of the clean window.  For the index set get_kk_outliers
        returned for this fit -- what kk_test passes -- the window is the device's; an index set of the caller's own making is
        handed to models.kk.get_limits.  IndexError when no point is clean with clean neighbours, as upstream."""
        plan = self._kk_plan()
        res = plan.kk_screen(self._kk_opts(max_num_outliers=max_num_outliers, **getattr(self, '_kk_last', {})),
                             z_hat=False, residuals=False)
        own = np.where(res['outlier_mask'][0] != 0)[0]
        if not np.array_equal(np.sort(np.asarray(outlier_index, dtype=int)), own):
            return kk.get_limits(self.get_fit_frequencies(), outlier_index, max_num_outliers=max_num_outliers)
        if res['status'][0] == 1:
            raise IndexError('no clean point with clean neighbours: the frequency limits are undefined')
        return float(res['f_lim'][0, 0]), float(res['f_lim'][0, 1])

    @staticmethod
    def _kk_weight_factor(num_freq, outlier_index, outlier_weight=1e-10):
        """the vector-valued weight_factor of kk_fit (drt1d.py:1399-1404): outliers stay in the data with (almost) no weight"""
        weight_factor = np.ones(2 * num_freq)
        outlier_index = np.asarray(outlier_index, dtype=int)
        weight_factor[outlier_index] = outlier_weight
        weight_factor[outlier_index + num_freq] = outlier_weight
        return weight_factor

    def kk_fit(self, frequencies, z, nonneg=False, l2_lambda_0=1e-2, extend_basis_decades=2, outlier_index=None):
        """DRT.kk_fit (drt1d.py:1393-1411): a weakly regularised fit without the sign constraint on a basis extended by
        ``extend_basis_decades`` (the instance's own setting is restored afterwards)."""
        extend_basis_orig = self.extend_basis_decades
        self.extend_basis_decades = extend_basis_decades
        try:
            weight_factor = 1 if outlier_index is None else self._kk_weight_factor(len(frequencies), outlier_index)
            self.fit_eis(frequencies, z, nonneg=nonneg, l2_lambda_0=l2_lambda_0, weight_factor=weight_factor)
            self.z_fit = np.asarray(z, dtype=complex)
        finally:
            self.extend_basis_decades = extend_basis_orig

    def kk_test(self, frequencies, z, nonneg=False, l2_lambda_0=1e-2, extend_basis_decades=2, norm='modulus',
                max_num_outliers=2, p_thresh=1e-4, n_sigma=None, std_sample_fraction=0.6, n_iter=2, n_outlier_iter=2,
                show_plot=True):
        """DRT.kk_test (drt1d.py:1370-1391): n_iter rounds of kk_fit -> outliers -> limits, each fit with the previous round's
        outliers weighted out.  Returns (outlier_index, (f_min, f_max), (f_clean, z_clean))."""
        if n_iter < 1:
            raise ValueError('n_iter must be at least 1')
        frequencies, z = np.asarray(frequencies, dtype=float), np.asarray(z, dtype=complex)
        outlier_index = None
        for _ in range(n_iter):
            self.kk_fit(frequencies, z, nonneg=nonneg, l2_lambda_0=l2_lambda_0, extend_basis_decades=extend_basis_decades,
                        outlier_index=outlier_index)
            outlier_index = self.get_kk_outliers(norm=norm, p_thresh=p_thresh, n_iter=n_outlier_iter, n_sigma=n_sigma,
                                                 std_sample_fraction=std_sample_fraction)
            f_min, f_max = self.get_kk_limits(outlier_index, max_num_outliers=max_num_outliers)
            fz_clean = kk.trim_data(frequencies, z, f_min, f_max)
        if show_plot:
            warnings.warn('plotting is outside this package: kk_test(show_plot=True) returns its results without a figure')
        return outlier_index, (f_min, f_max), fz_clean

    def kk_test_batch(self, frequencies, z_batch, nonneg=False, l2_lambda_0=1e-2, extend_basis_decades=2, norm='modulus',
                      max_num_outliers=2, p_thresh=1e-4, n_sigma=None, std_sample_fraction=0.6, n_iter=2, n_outlier_iter=2):
        """kk_test for B spectra on one frequency grid (a map): the batch is staged once, then n_iter rounds of fit -> screen run
        on one plan.  Every screen but the last writes the next fit's row factors on the device (nothing but the results crosses
        to the host), and the later rounds fit the staged data again without staging anew, which would reset them.  Fits with
        row factors run in one range (hipdrt_plan_set_subbatches), so the second and later fits do not overlap ranges.
        Returns a dict: outlier_mask (B, nf) bool, f_min / f_max (B,), clean_mask (B, nf) bool (the points trim_data keeps),
        residuals (B, nf) complex in percent of |Z|, std (B,), status (B,) (0 ok, 1 no clean point: limits NaN, -1 fit failed),
        z_hat (B, nf) complex -- all of the last round -- and passes, the same entries for every round.  The plan's weight
        factors are cleared afterwards."""
        if norm != 'modulus':
            raise ValueError(f'norm must be "modulus", got {norm!r}')
        if n_iter < 1:
            raise ValueError('n_iter must be at least 1')
        if self.fit_dop or self.fit_capacitance:
            raise NotImplementedError('kk_test_batch is built for plain EIS plans')
        frequencies = np.asarray(frequencies, dtype=float)
        z_batch = np.asarray(z_batch, dtype=complex)
        if z_batch.ndim != 2 or z_batch.shape[1] != len(frequencies):
            raise ValueError('z_batch must have shape (B, len(frequencies))')
        opts = self._kk_opts(n_outlier_iter=n_outlier_iter, p_thresh=p_thresh, n_sigma=n_sigma,
                             std_sample_fraction=std_sample_fraction, max_num_outliers=max_num_outliers)
        extend_basis_orig = self.extend_basis_decades
        self.extend_basis_decades = extend_basis_decades
        plan, passes = None, []
        try:
            plan = self.stage_batch(frequencies, z_batch, nonneg=nonneg, l2_lambda_0=l2_lambda_0)
            for i in range(n_iter):
                plan.fit()
                res = plan.kk_screen(opts, set_row_factors=i < n_iter - 1)
                res['timings_ms'], res['launches'] = plan.timings()
                ok = res['status'] == 0
                f_min, f_max = res['f_lim'][:, 0], res['f_lim'][:, 1]
                with np.errstate(invalid='ignore'):
                    clean = (frequencies[None, :] <= f_max[:, None]) & (frequencies[None, :] >= f_min[:, None]) & ok[:, None]
                passes.append(dict(outlier_mask=res['outlier_mask'] != 0, f_min=f_min, f_max=f_max, clean_mask=clean,
                                   residuals=res['residuals'], std=res['std'], status=res['status'], z_hat=res['z_hat'],
                                   i_lim=res['i_lim'], timings_ms=res['timings_ms']))
        finally:
            self.extend_basis_decades = extend_basis_orig
            if plan is not None:
                plan.set_weight_factors(1.0)
        out = dict(passes[-1])
        out['passes'] = passes
        return out
