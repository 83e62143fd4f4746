"""Drop-in for the EIS fit path of hybdrt.models.DRT (hybdrt/models/drt1d.py + drtbase.py).

``DRT(**ctor).fit_eis(frequencies, z, **hypers)`` leaves ``fit_parameters``, ``qphb_params``,
``qphb_history`` populated like the reference; ``fit_eis_batch`` is the batched form the reference runs as a
serial loop in DRTMD.fit_observations (hybdrt/mapping/drtmd.py:303-319).  All arithmetic -- lookup tables,
Z'/Z'' and penalty matrices, the QPHB loop -- runs in libhipdrt.so on one MI355X; this module only decides
grids and options and rescales results (host logic mirrored from the reference, cited per method)."""
import warnings

import numpy as np

from .. import _ffi, preprocessing as pp
from ..matrices import mat1d
from ..utils.array import is_uniform
from . import kk, peaks, predict, qphb
from .prepared import PreparedFitMixin, combine_status

_FIT_KW_DEFAULTS = dict(  # DRT._qphb_fit_core keyword defaults (drt1d.py:102-137) that the device loop honours
    nonneg=True, scale_data=True, ohmic_penalty=1e-6, inductance_penalty=1e-6, inductance_scale=1e-5,
    capacitance_penalty=1e-6, capacitance_scale=1e-3, update_scale=False,
    penalty_type='integral', eis_error_structure=None, eis_vmm_epsilon=0.25, eis_reim_cor=0.25,
    iw_l1_lambda_0=1e-4, iw_l2_lambda_0=1e-4, eff_hp=True, weight_factor=1, xtol=1e-2, max_iter=50)


class DRT(PreparedFitMixin):
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

    # ---- warm restarts of the device loop (drt1d.py:1270-1365) and the candidate generators on top (1497-1632) ---
    def continue_from_init(self, x_init=None, rho_vector=None, s_vectors=None, weights=None, weight_factor=1,
                           xtol=1e-2, max_iter=10, min_iter=2, history_of=-1, dop_rho_vector=None, **kw):
        """DRT._continue_from_init for the last fitted batch: the outer loop re-entered on the device from the given
        state (arrays with a leading batch axis; None = the state left by the previous call) with ``kw`` updating the
        hyper-parameters (e.g. s_0, l2_lambda_0).  est_weights, xmx norms and the data scale stay as fitted.
        Returns the same dict of arrays as fit_eis_batch (outer_iters = iterations of this call)."""
        if isinstance(self._plan, _ffi.PreparedPlan):         # chrono / joint fits, DOP: the same loop on the prepared plan
            return self._continue_prepared(x_init=x_init, rho_vector=rho_vector, s_vectors=s_vectors, weights=weights,
                                           dop_rho_vector=dop_rho_vector, weight_factor=weight_factor, xtol=xtol, max_iter=max_iter, min_iter=min_iter,
                                           history_of=history_of, **kw)
        if self._plan is None or self._last_batch is None:
            raise Exception('continue_from_init needs a finished qphb fit')
        fit_kw = dict(self.fit_kwargs)
        fit_kw.update(kw)
        fit_kw.update(xtol=xtol, max_iter=max_iter)
        opts, _, _ = self._make_opts(fit_kw)
        plan = self._plan
        plan.set_state(x=x_init, rho=rho_vector, s=s_vectors, weights=weights)
        plan.record_history(history_of)
        plan.continue_fit(opts, weight_factor=weight_factor, min_iter=min_iter)
        res = self.collect_staged()
        if history_of >= 0:
            res['history'] = plan.history()
        return res

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
        base = self._collect_prepared() if isinstance(self._plan, _ffi.PreparedPlan) else self.collect_staged()
        s_base = base['s_vectors'].copy()
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

    def evaluate_obs_llh_rss_batch(self, llh_kw=None, rss_kw=None):
        """(DRT.evaluate_llh(**llh_kw), DRT.evaluate_rss(**rss_kw)) (drt1d.py:4433-4496; x = the last iterate) for every
        spectrum of the last fitted batch -- what DRTMD.fit_observation stores as obs_llh / obs_rss (drtmd.py:259-260).
        Keys as upstream: ``weights`` (None = the fit's est_weights, 'uniform' = per-domain means of them, a scalar),
        ``normalize`` (divide by the number of data rows), and for the likelihood ``marginalize_weights``, ``alpha_0``,
        ``beta_0``.  Residuals and all sums on the device."""
        from scipy.special import loggamma
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
        if llh_kw.get('marginalize_weights', True):
            alpha_n = alpha_0 - 1 + m / 2
            llh = alpha_0 * np.log(beta_0) - alpha_n * np.log(beta_0 + 0.5 * rss_l) + loggamma(alpha_n) - loggamma(alpha_0)
        else:
            llh = -0.5 * rss_l
        llh = llh + slw
        if llh_kw.get('normalize', False):
            llh = llh / m
        rss = sums(rss_kw.get('weights'))[0].copy()
        if rss_kw.get('normalize', False):
            rss /= m
        return llh, rss

    def evaluate_step_llh_batch(self, alpha_0=2, beta_0=1):
        """evaluate_llh(weights=estimate_weights(x), x) (drt1d.py:2618-2622) for the current x of every spectrum of
        the batch: residuals, re-estimated weights and both sums on the device, the two lgamma constants here."""
        from scipy.special import loggamma
        rss, slw = self._plan.llh_terms()
        alpha_n = alpha_0 - 1 + self._plan.m / 2
        beta_n = beta_0 + 0.5 * rss
        return alpha_0 * np.log(beta_0) - alpha_n * np.log(beta_n) + loggamma(alpha_n) - loggamma(alpha_0) + slw

    def pfrt_fit_eis_batch(self, frequencies, z_batch, factors=None, max_iter_per_step=10, max_init_iter=20,
                           xtol=1e-2, nonneg=True, after_init=None, **kw):
        """DRT.pfrt_fit_eis (drt1d.py:2558-2690) for B spectra at once: a full fit at the first regularisation factor
        (s_0 * f, l2_lambda_0 / f), then one warm restart per further factor on the device.  Returns
        {'factors', 'step_x' (S, B, n) scaled-space solutions, 'step_llh' (S, B), 'step_iters' (S, B)}."""
        base = qphb.get_default_hypers(True, False, 'gaussian')
        base.update({k: v for k, v in kw.items() if k in base})
        if factors is None:
            factors = np.logspace(-1, 1, 11)
        s_0 = np.broadcast_to(np.asarray(base['s_0'], dtype=float), (3,))

        def step_hypers(f):
            return dict(s_0=s_0 * f, l2_lambda_0=base['l2_lambda_0'] / f)

        init_kw = dict(kw)
        init_kw.update(step_hypers(factors[0]))
        res = self.fit_eis_batch(frequencies, z_batch, nonneg=nonneg, max_iter=max_init_iter, xtol=xtol, **init_kw)
        # every step's final state stays on the device for predict_pfrt_batch / step_p_matrix (hipdrt_plan_pfrt_begin / _record)
        self._plan.pfrt_begin(len(factors))
        self._plan.pfrt_record()
        step_x, step_llh, step_iters = [res['x'].copy()], [self.evaluate_step_llh_batch()], [res['outer_iters'].copy()]
        status = np.array(res['status']).copy()
        if after_init is not None:          # (what DRTMD reads from the FIRST step's fit: its P matrix, llh / rss -- mapping)
            after_init(res)
        for f in factors[1:]:
            res = self.continue_from_init(xtol=xtol, max_iter=max_iter_per_step, **step_hypers(f))
            self._plan.pfrt_record()
            step_x.append(res['x'].copy())
            step_llh.append(self.evaluate_step_llh_batch())
            step_iters.append(res['outer_iters'].copy())
            status = combine_status(status, res['status'])
        self.pfrt_result = {'factors': np.asarray(factors), 'step_x': np.array(step_x), 'step_llh': np.array(step_llh),
                            'step_iters': np.array(step_iters), 'status': status,
                            'coefficient_scale': res['coefficient_scale'], 'basis_tau': res['basis_tau']}
        return self.pfrt_result

    # ---- the PFRT of a PFRT fit (drt1d.py:2716-2858), over the steps recorded on the device -----------------------------------
    def _pfrt_plan(self, what):
        plan = self._plan
        if plan is None or getattr(self, 'pfrt_result', None) is None or plan.pfrt_steps() == 0:
            raise RuntimeError(f'{what} needs a finished PFRT fit (pfrt_fit_eis_batch, fit_observations(fit_type="pfrt"))')
        return plan

    def step_p_matrix(self, step, b=0):
        """pfrt_result['step_p_mat'][step] of member ``b`` of the last PFRT fit (drt1d.py:2611-2632): calculate_pq with the step's
        final s / rho and the raw weights re-estimated from the step's x, formed on the device (hipdrt_plan_get_step_p_matrix)"""
        return self._pfrt_plan('step_p_matrix').step_p_matrix(step, b)

    def predict_pfrt_batch(self, tau=None, tau_pfrt=None, sign=None, prior_mu=-4, prior_sigma=0.5, find_peaks_kw=None,
                           n_eff_factor=0.5, fxx_var_floor=1e-5, extend_var=True, smooth=True, smooth_kw=None, integrate=False,
                           integrate_threshold=1e-6, normalize=True, return_info=False):
        """DRT.predict_pfrt (drt1d.py:2716-2858) for every spectrum of the last PFRT fit -> (B, len(tau)), on the device over the
        recorded steps (hipdrt_plan_predict_pfrt; models/pfrt.py is the rule in numpy).  tau_pfrt=None is get_tau_eval(10), tau=None
        is tau_pfrt (without smooth the result stays on tau_pfrt, as upstream).  With return_info also a dict with tau_pfrt,
        raw_pfrt (B, n), step_pfrt (S, B, n), post_prob (S, B) and status (B,), the first three also stored into pfrt_result under
        upstream's keys.  Rows of spectra whose fit failed in any step, or whose step P is not positive definite, are NaN.  Of
        find_peaks_kw only height and prominence are built; plain EIS fits only.  select_pfrt_candidates and the discrete-model
        conversion stay with the reference's Python on these arrays."""
        from .. import _ffi
        if self.series_neg:
            raise NotImplementedError('predict_pfrt: series_neg fits are not taken (upstream\'s normalize=True raises for them)')
        if isinstance(self._plan, _ffi.PreparedPlan):
            raise NotImplementedError('predict_pfrt is built for plain EIS fits; a prepared plan records its steps and gives '
                                      'step_p_matrix only')
        plan = self._pfrt_plan('predict_pfrt')
        fkw = dict(find_peaks_kw or {'height': 1e-3, 'prominence': 5e-3})
        for name in fkw:
            if name not in ('height', 'prominence'):
                raise NotImplementedError(f'predict_pfrt: the {name}= condition of scipy.signal.find_peaks is not built '
                                          f'(only height and prominence)')
        skw = dict(smooth_kw or {'order': 2, 'epsilon': 5})
        if set(skw) - {'order', 'epsilon'}:
            raise TypeError(f"unexpected smooth_kw {sorted(set(skw) - {'order', 'epsilon'})}")
        sign = self._drt_sign(plan, sign)
        tau_pfrt = self.get_tau_eval(10) if tau_pfrt is None else np.asarray(tau_pfrt, dtype=float)
        tau_out = tau_pfrt if (tau is None or not smooth) else np.asarray(tau, dtype=float)
        search = sign if (self.fit_kwargs['nonneg'] and sign != 0) else 0
        ext = self._extend_var_indices(tau_pfrt) if extend_var else (-1, -1)
        if ext[0] >= len(tau_pfrt):
            raise ValueError('extend_var: the measured tau range ends at the last point of the evaluation grid')
        opts = _ffi.pfrt_opts(eval_sign=sign, search=search, height=fkw.get('height', 0), prominence=fkw.get('prominence', 0),
                              prior_mu=prior_mu, prior_sigma=prior_sigma, n_eff_factor=n_eff_factor, fxx_var_floor=fxx_var_floor,
                              ext_left=ext[0], ext_right=ext[1], smooth=bool(smooth), smooth_order=skw.get('order', 2),
                              smooth_epsilon=skw.get('epsilon', 5), integrate=bool(integrate),
                              integrate_threshold=integrate_threshold, normalize=bool(normalize))
        factors = np.asarray(self.pfrt_result['factors'], dtype=float)
        if len(factors) != plan.pfrt_steps():
            raise ValueError(f"pfrt_result['factors'] has {len(factors)} entries, the plan recorded {plan.pfrt_steps()} steps")
        out = plan.predict_pfrt(factors, np.log(tau_pfrt), np.log(tau_out) if smooth else None, opts,
                                want=None if return_info else ('pfrt',))
        if not return_info:
            return out['pfrt']
        self.pfrt_result.update(tau_pfrt=tau_pfrt, raw_pfrt=out['raw_pfrt'], step_pfrt=out['step_pfrt'])
        info = dict(tau_pfrt=tau_pfrt, raw_pfrt=out['raw_pfrt'], step_pfrt=out['step_pfrt'], post_prob=out['post_prob'],
                    status=out['status'])
        return out['pfrt'], info

    def predict_pfrt(self, tau=None, tau_pfrt=None, sign=None, prior_mu=-4, prior_sigma=0.5, find_peaks_kw=None, n_eff_factor=0.5,
                     fxx_var_floor=1e-5, extend_var=True, smooth=True, smooth_kw=None, integrate=False, integrate_threshold=1e-6,
                     normalize=True, b=0):
        """DRT.predict_pfrt (drt1d.py:2716-2858) of member ``b`` of the last PFRT fit, from the device; pfrt_result gets tau_pfrt,
        raw_pfrt and step_pfrt of that member, as upstream"""
        tot, info = self.predict_pfrt_batch(tau=tau, tau_pfrt=tau_pfrt, sign=sign, prior_mu=prior_mu, prior_sigma=prior_sigma,
                                            find_peaks_kw=find_peaks_kw, n_eff_factor=n_eff_factor, fxx_var_floor=fxx_var_floor,
                                            extend_var=extend_var, smooth=smooth, smooth_kw=smooth_kw, integrate=integrate,
                                            integrate_threshold=integrate_threshold, normalize=normalize, return_info=True)
        self.pfrt_result.update(raw_pfrt=info['raw_pfrt'][b], step_pfrt=info['step_pfrt'][:, b])
        return tot[b]

    # ---- what DRTMD takes from a finished fit (mapping/drtmd.py:258-279) ----------------------------------------
    def _signed_basis(self, bm, sign):
        """series_neg fits carry 2 ntau coefficients [positive copy | negative copy]: the evaluation rows of
        estimate_distribution_cov's three cases (drt1d.py:3090-3103) as ONE matrix over both copies -- sign=1 the positive
        block, -1 the negative one, 0 their difference (B, -B): B S++ B' + B S-- B' - B (S+- + S-+) B'"""
        if not self.series_neg:
            return bm
        zero = np.zeros_like(bm)
        if sign == 1:
            return np.hstack([bm, zero])
        if sign == -1:
            return np.hstack([zero, bm])
        if sign == 0:
            return np.hstack([bm, -bm])
        raise ValueError('sign must be 1, -1 or 0')

    def estimate_distribution_var_batch(self, tau=None, ppd=20, extend_var=False, sign=1):
        """Diagonal of DRT.estimate_distribution_cov (drt1d.py:3063-3151; order 0, no normalisation) for every
        spectrum of the last fitted batch: diag(B P^-1 B') coefficient_scale^2, computed on the device from the
        Cholesky factor of each final P.  Returns (var (B, len(tau)), ok (B,) bool); ``extend_var`` applies the
        reference's clamp outside the measured tau range (drt1d.py:3126-3143)."""
        from ..matrices import basis
        prepared = isinstance(self._plan, _ffi.PreparedPlan)
        if self._plan is None or (self._last_batch is None and not prepared):
            raise Exception('Parameter covariance estimation is only available for qphb fits')
        if tau is None:
            tau = self.get_tau_eval(ppd)
        tau = np.asarray(tau, dtype=float)
        bm = basis.construct_func_eval_matrix(np.log(self.basis_tau), np.log(tau), self.tau_basis_type,
                                              epsilon=self.tau_epsilon, order=0)
        bm = self._signed_basis(bm, sign)
        if prepared:
            # the device loop of a prepared plan runs at unit scale: estimate_param_cov's coefficient_scale^2 is applied here
            var, status = self._plan.distribution_var(bm, self._plan.batch)
            preps = self._last_prepared[0] if getattr(self, '_last_prepared', None) and \
                len(self._last_prepared[0]) == self._plan.batch else [self._prep]
            var = var * np.array([pr['coefficient_scale'] for pr in preps])[:, None] ** 2
        else:
            var, status = self._plan.distribution_var(bm, self._last_batch)
        if extend_var:
            if prepared:
                pr = preps[0]                       # (the members of a prepared batch share their sampling grids)
                t_left, t_right = pp.get_tau_lim(pr['frequencies'], pr.get('sample_times'), pr.get('nonconsec_step_times'))
            else:
                t_left, t_right = 1 / (2 * np.pi * np.max(self.f_fit)), 1 / (2 * np.pi * np.min(self.f_fit))
            left_index = int(np.argmin(np.abs(tau - t_left))) + 1
            right_index = int(np.argmin(np.abs(tau - t_right)))
            var[:, :left_index] = np.maximum(var[:, :left_index], var[:, left_index][:, None])
            var[:, right_index:] = np.maximum(var[:, right_index:], var[:, right_index][:, None])
        return var, status == 0

    def estimate_param_var_batch(self):
        """np.diag(DRT.estimate_param_cov()) (drt1d.py:4116-4138) for every spectrum of the last fitted batch, from the
        Cholesky factor of each final P on the device.  Returns (var (B, n), ok (B,) bool)."""
        prepared = isinstance(self._plan, _ffi.PreparedPlan)
        if self._plan is None or (self._last_batch is None and not prepared):
            raise Exception('Parameter covariance estimation is only available for qphb fits')
        if prepared:     # the prepared loop runs at unit scale: coefficient_scale^2 of estimate_param_cov applied here
            var, status = self._plan.param_var(self._plan.batch)
            preps = self._last_prepared[0] if getattr(self, '_last_prepared', None) and \
                len(self._last_prepared[0]) == self._plan.batch else [self._prep]
            return var * np.array([pr['coefficient_scale'] for pr in preps])[:, None] ** 2, status == 0
        var, status = self._plan.param_var(self._last_batch)
        return var, status == 0

    def _cov_scale(self, b):
        """(coefficient_scale of fitted measurement b where the device loop ran at unit scale, else 1; its prep or None)"""
        if isinstance(self._plan, _ffi.PreparedPlan):
            preps = self._last_prepared[0] if getattr(self, '_last_prepared', None) and \
                len(self._last_prepared[0]) == self._plan.batch else [self._prep]
            return preps[b]['coefficient_scale'], preps[b]
        return 1.0, None

    def estimate_param_cov(self, b=0):
        """DRT.estimate_param_cov (drt1d.py:4116-4138): inv(P) * coefficient_scale^2 with the DOP block rescaled by
        dop_scale_vector, from the Cholesky factor of the final P on the device (hipdrt_plan_param_cov); ``b`` picks a
        member of the last batch.  None (with upstream's warning) when P is not positive definite."""
        if self._plan is None or (self._last_batch is None and not isinstance(self._plan, _ffi.PreparedPlan)):
            raise Exception('Parameter covariance estimation is only available for qphb fits')
        cov, ok = self._plan.param_cov(b)
        if not ok:
            warnings.warn('Singular P matrix - could not obtain covariance estimate')
            return None
        cs, prep = self._cov_scale(b)
        cov = cov * cs ** 2
        if prep is not None and prep['dop']:
            a, e = prep['dop']
            cov[:, a:e] *= prep['dop_scale_vector'][None, :]
            cov[a:e, :] *= prep['dop_scale_vector'][:, None]
        return cov

    def estimate_distribution_cov(self, tau=None, ppd=20, extend_var=False, var_floor=0.0, b=0, sign=1):
        """DRT.estimate_distribution_cov (drt1d.py:3063-3151; order 0, sign 1, no normalisation): basis_matrix @ x_cov @
        basis_matrix.T of the DRT block, formed on the device (hipdrt_plan_distribution_cov), then upstream's ``extend_var``
        clamp of the diagonal outside the measured tau range (3126-3143) and ``var_floor``."""
        from ..matrices import basis
        if self._plan is None or (self._last_batch is None and not isinstance(self._plan, _ffi.PreparedPlan)):
            raise Exception('Parameter covariance estimation is only available for qphb fits')
        if tau is None:
            tau = self.get_tau_eval(ppd)
        tau = np.asarray(tau, dtype=float)
        bm = basis.construct_func_eval_matrix(np.log(self.basis_tau), np.log(tau), self.tau_basis_type,
                                              epsilon=self.tau_epsilon, order=0)
        cov, ok = self._plan.distribution_cov(self._signed_basis(bm, sign), b)
        if not ok:
            warnings.warn('Singular P matrix - could not obtain covariance estimate')
            return None
        cs, prep = self._cov_scale(b)
        cov = cov * cs ** 2
        if extend_var:
            if prep is not None:
                t_left, t_right = pp.get_tau_lim(prep['frequencies'], prep.get('sample_times'), prep.get('nonconsec_step_times'))
            else:
                t_left, t_right = 1 / (2 * np.pi * np.max(self.f_fit)), 1 / (2 * np.pi * np.min(self.f_fit))
            left_index = int(np.argmin(np.abs(tau - t_left))) + 1
            right_index = int(np.argmin(np.abs(tau - t_right)))
            var = np.diag(cov).copy()
            var[:left_index] = np.maximum(var[:left_index], var[left_index])
            var[right_index:] = np.maximum(var[right_index:], var[right_index])
            cov[np.diag_indices(cov.shape[0])] = var
        if var_floor > 0:
            var = np.diag(cov).copy()
            var[var < var_floor] = var_floor
            np.fill_diagonal(cov, var)
        return cov

    def get_tau_eval(self, ppd):
        """drtbase.get_tau_eval (drtbase.py:263-285): one decade beyond the basis grid on each side."""
        basis_tau = self.basis_tau
        log_min, log_max = np.log10(np.min(basis_tau)) - 1, np.log10(np.max(basis_tau)) + 1
        return np.logspace(log_min, log_max, int((log_max - log_min) * ppd) + 1)

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
        from scipy.special import loggamma
        w = self._llh_weights(weights)
        rss = self.evaluate_rss(w, x)
        if marginalize_weights:
            alpha_n = alpha_0 - 1 + len(w) / 2
            beta_n = beta_0 + 0.5 * rss
            llh = alpha_0 * np.log(beta_0) - alpha_n * np.log(beta_n) + loggamma(alpha_n) - loggamma(alpha_0)
        else:
            llh = -0.5 * rss
        llh = llh + np.sum(np.log(w))
        return llh / len(w) if normalize else llh

    def _fit(self, frequencies, z_batch, kw, history_of):
        self.stage_batch(frequencies, z_batch, history_of=history_of, **kw)
        self.fit_staged()
        return self.collect_staged()

    # ---- model evaluation (drt1d.py:2959-3584), acting on the last fitted batch --------------------------------------------
    def _predict_plan(self, what, x=None, p_matrix=None):
        """(plan, per-member coefficient scales or None) for a prediction.  The x= / p_matrix= overrides of the reference would
        bypass the state on the device and are not taken."""
        if x is not None:
            raise NotImplementedError(f'{what}: the x= override is not taken (predictions use the coefficients on the device)')
        if p_matrix is not None:
            raise NotImplementedError(f'{what}: the p_matrix= override is not taken (the band uses the fit\'s own P on the device)')
        prepared = isinstance(self._plan, _ffi.PreparedPlan)
        if self._plan is None or (self._last_batch is None and not prepared) or (prepared and not self._plan.batch):
            raise RuntimeError(f'{what} needs a finished qphb fit')
        if not prepared:
            return self._plan, None
        # the device loop of a prepared plan runs at unit scale: the coefficient scale is applied here
        preps = self._last_prepared[0] if getattr(self, '_last_prepared', None) and \
            len(self._last_prepared[0]) == self._plan.batch else [self._prep]
        self._plan.set_tau_basis(np.log(self.basis_tau), self.tau_epsilon)
        return self._plan, np.array([pr['coefficient_scale'] for pr in preps], dtype=float)

    def _drt_sign(self, plan, sign):
        two_copies = plan.n - plan.ns == 2 * len(self.basis_tau)
        if sign is None:
            return predict.default_sign(two_copies)              # DRT.default_dist_sign
        if sign not in (-1, 0, 1):
            raise ValueError(f'Invalid sign {sign}. Options: -1, 0, 1')
        return sign if two_copies else 1                         # get_drt_params ignores the sign of a one-copy fit

    def _predict_drt_device(self, what, tau, ppd, order, sign, normalize, normalize_by, abs_norm, quantiles, x=None, p_matrix=None):
        if order not in (0, 1, 2):
            raise ValueError(f'Invalid order {order}. Options: 0, 1, 2')
        if normalize_by is not None and not normalize_by > 0:
            raise ValueError('normalize_by must be positive')
        plan, scales = self._predict_plan(what, x=x, p_matrix=p_matrix)
        sign = self._drt_sign(plan, sign)
        if tau is None:
            tau = self.get_tau_eval(ppd)
        by_rp = bool(normalize) and normalize_by is None
        n_sig = None if quantiles is None else predict.n_sigma(quantiles)
        mu, lo, hi, status = plan.predict_drt(np.log(np.asarray(tau, dtype=float)), order=order, sign=sign,
                                              normalize=(2 if abs_norm else 1) if by_rp else 0, n_sigma=n_sig)
        f = None
        if scales is not None and not by_rp:                     # (a ratio to the spectrum's own R_p carries no scale)
            f = scales[:, None]
        if normalize_by is not None:
            f = (1.0 if f is None else f) / normalize_by
        if f is not None:
            mu = mu * f
            lo, hi = (None, None) if lo is None else (lo * f, hi * f)
        return mu, lo, hi, status

    def predict_drt_batch(self, tau=None, ppd=20, order=0, sign=None, normalize=False, normalize_by=None, abs_norm=False,
                          x=None):
        """DRT.predict_drt (drt1d.py:3040-3061) for every spectrum of the last fitted batch -> (B, len(tau)): the evaluation
        matrix is built and applied to the resident coefficients on the device (hipdrt_plan_predict_drt); nothing is downloaded
        but the result.  order 0, 1, 2; sign=None is the reference's default (0 for series_neg fits, else 1); tau=None is
        get_tau_eval(ppd); normalize divides every spectrum by its own R_p (abs_norm: of |x|), normalize_by by a given positive
        number.  Rows of failed fits are NaN.  A map cut into several device batches (max_batch) predicts for the last batch."""
        return self._predict_drt_device('predict_drt_batch', tau, ppd, order, sign, normalize, normalize_by, abs_norm, None, x=x)[0]

    def predict_drt_ci_batch(self, tau=None, ppd=20, order=0, sign=None, normalize=False, normalize_by=None, abs_norm=False,
                             quantiles=(0.025, 0.975), x=None, p_matrix=None):
        """DRT.predict_drt_ci (drt1d.py:3209-3231) for every spectrum of the last fitted batch -> (lo, hi, ok): mean +/- the
        quantiles' numbers of posterior standard deviations (stats.std_normal_quantile), sigma^2 = diag(E inv(P) E') from the
        Cholesky factor of every final P on the device, fed the device-resident evaluation rows.  ok (B,) bool is False where
        the fit failed or P is not positive definite (rows NaN; the reference returns (None, None)).  Last device batch only."""
        _, lo, hi, status = self._predict_drt_device('predict_drt_ci_batch', tau, ppd, order, sign, normalize, normalize_by,
                                                     abs_norm, quantiles, x=x, p_matrix=p_matrix)
        return lo, hi, status >= 0

    def predict_z_batch(self, frequencies=None, include_drt=True, include_ohmic=True, include_inductance=True, x=None):
        """DRT.predict_z(include_vz_offset=False) (drt1d.py:3500-3542) for every spectrum of the last fitted batch, at ANY
        frequencies -> complex (B, nf); frequencies=None: the fit frequencies.  Z' / Z'' matrices are built on the device at the
        requested frequencies from the plan's own lookup tables (clamped outside them like np.interp), tau grid and integration
        mode, and applied to the resident coefficients (hipdrt_plan_predict_z).  This is the any-grid impedance prediction:
        ``predict_z_batch(f)[b]``; DRT.predict_z itself serves the fit frequencies only.  Plain EIS fits only (no fit_dop,
        fit_capacitance, solve_rp, series_neg, chrono or joint data).  Rows of failed fits are NaN.  Last device batch only."""
        if self.fit_dop:
            raise NotImplementedError('predict_z_batch is built for plain EIS fits, not for fit_dop fits')
        plan, scales = self._predict_plan('predict_z_batch', x=x)
        if scales is not None:
            raise NotImplementedError('predict_z_batch is built for plain EIS plans (fit_eis / fit_eis_batch without '
                                      'fit_dop, fit_capacitance, solve_rp, series_neg or outlier removal)')
        f = self.get_fit_frequencies() if frequencies is None else np.asarray(frequencies, dtype=float)
        return plan.predict_z(f, include_drt=include_drt, include_ohmic=include_ohmic, include_inductance=include_inductance)[0]

    def predict_r_p_batch(self, absolute=False):
        """DRT.predict_r_p (drt1d.py:3552-3571; default sign) of every spectrum of the last fitted batch, summed on the device"""
        plan, scales = self._predict_plan('predict_r_p_batch')
        r_p = plan.predict_resistances(absolute=absolute, r_p_only=scales is not None)[0]
        return r_p if scales is None else r_p * scales

    def _r_inf_prepared(self, scales):
        sp = self.special_qp_params
        if 'R_inf' not in sp:
            return np.zeros(len(scales))
        return self._plan.get('x')[:, sp['R_inf']['index']] * scales

    def predict_r_inf_batch(self):
        """DRT.predict_r_inf (drt1d.py:3573-3581) of every spectrum of the last fitted batch"""
        plan, scales = self._predict_plan('predict_r_inf_batch')
        return plan.predict_resistances()[1] if scales is None else self._r_inf_prepared(scales)

    def predict_r_tot_batch(self):
        """DRT.predict_r_tot (drt1d.py:3583-3584): R_inf + R_p of every spectrum of the last fitted batch"""
        plan, scales = self._predict_plan('predict_r_tot_batch')
        if scales is None:
            return plan.predict_resistances()[2]
        return self._r_inf_prepared(scales) + plan.predict_resistances(r_p_only=True)[0] * scales

    # single-spectrum forms with the reference's signatures; ``b`` picks a member of the last batch
    def predict_drt(self, tau=None, ppd=20, x=None, order=0, sign=1, normalize=False, normalize_by=None, abs_norm=False, b=0):
        """DRT.predict_drt (drt1d.py:3040-3061) of member ``b`` of the last fit, from the device"""
        return self._predict_drt_device('predict_drt', tau, ppd, order, sign, normalize, normalize_by, abs_norm, None, x=x)[0][b]

    def predict_distribution(self, tau=None, ppd=20, x=None, order=0, sign=1, normalize=False, normalize_by=None,
                             abs_norm=False, b=0):
        """DRT.predict_distribution (drt1d.py:3033-3038): the deprecated name of predict_drt"""
        warnings.warn("predict_distribution is deprecated and will be removed in the future. Please use predict_drt instead",
                      DeprecationWarning)
        return self.predict_drt(tau=tau, ppd=ppd, x=x, order=order, sign=sign, normalize=normalize, normalize_by=normalize_by,
                                abs_norm=abs_norm, b=b)

    def predict_drt_ci(self, tau=None, ppd=20, x=None, order=0, sign=1, normalize=False, normalize_by=None,
                       quantiles=(0.025, 0.975), p_matrix=None, b=0):
        """DRT.predict_drt_ci (drt1d.py:3209-3231) of member ``b`` of the last fit: (lo, hi), or (None, None) with upstream's
        warning when P is not positive definite"""
        _, lo, hi, status = self._predict_drt_device('predict_drt_ci', tau, ppd, order, sign, normalize, normalize_by, False,
                                                     quantiles, x=x, p_matrix=p_matrix)
        if status[b] < 0:
            warnings.warn('Singular P matrix - could not obtain covariance estimate')
            return None, None
        return lo[b], hi[b]

    def predict_r_p(self, sign=None, absolute=False, x=None, raw=False, b=0):
        """DRT.predict_r_p (drt1d.py:3552-3571) of member ``b`` of the last fit; the default sign only"""
        plan, _ = self._predict_plan('predict_r_p', x=x)
        if raw or (sign is not None and self._drt_sign(plan, sign) != self._drt_sign(plan, None)):
            raise NotImplementedError('predict_r_p: only the default sign of the fitted coefficients is built')
        return float(self.predict_r_p_batch(absolute=absolute)[b])

    def predict_r_inf(self, b=0):
        """DRT.predict_r_inf (drt1d.py:3573-3581) of member ``b`` of the last fit"""
        return float(self.predict_r_inf_batch()[b])

    def predict_r_tot(self, b=0):
        """DRT.predict_r_tot (drt1d.py:3583-3584) of member ``b`` of the last fit"""
        return float(self.predict_r_tot_batch()[b])

    # ---- peak finding (drt1d.py:3753-3947; mapping/curvature.py, mapping/drtmd.py:1023-1106) on the last fitted batch ------------
    def _extend_var_indices(self, tau):
        """the two clamp indices of estimate_distribution_cov's extend_var (drt1d.py:3125-3135) on the grid tau"""
        if isinstance(self._plan, _ffi.PreparedPlan):
            preps = self._last_prepared[0] if getattr(self, '_last_prepared', None) and \
                len(self._last_prepared[0]) == self._plan.batch else [self._prep]
            pr = preps[0]                           # (the members of a prepared batch share their sampling grids)
            t_left, t_right = pp.get_tau_lim(pr['frequencies'], pr.get('sample_times'), pr.get('nonconsec_step_times'))
        else:
            t_left, t_right = 1 / (2 * np.pi * np.max(self.f_fit)), 1 / (2 * np.pi * np.min(self.f_fit))
        return int(np.argmin(np.abs(tau - t_left))) + 1, int(np.argmin(np.abs(tau - t_right)))

    def _find_peaks_device(self, what, tau, ppd, normalize, sign, method, extend_var, want=None, **opt_kw):
        plan, scales = self._predict_plan(what)
        if tau is None:
            tau = self.get_tau_eval(ppd)
        tau = np.asarray(tau, dtype=float)
        search = sign if (self.fit_kwargs['nonneg'] and sign != 0) else 0
        ext = self._extend_var_indices(tau) if (extend_var and method != 'thresh') else (-1, -1)
        if ext[0] >= len(tau):
            raise ValueError('extend_var: the measured tau range ends at the last point of the evaluation grid')
        opts = _ffi.peak_opts(eval_sign=self._drt_sign(plan, sign), search=search, normalize=1 if normalize else 0, method=method,
                              ext_left=ext[0], ext_right=ext[1], **opt_kw)
        # (a ratio to the spectrum's own R_p carries no scale; otherwise a prepared plan's unit-scale rows take theirs on the device)
        out = plan.find_peaks(np.log(tau), opts, row_scale=None if (normalize or scales is None) else scales, want=want)
        return tau, out

    def find_peaks_batch(self, tau=None, normalize=True, ppd=10, prominence=None, height=None, sign=1, return_info=False,
                         method='thresh', prob_thresh=0.25, p_matrix=None, fxx_var_floor=1e-5, extend_var=True, num_peaks=None,
                         **kw):
        """DRT.find_peaks (drt1d.py:3753-3947) for every spectrum of the last fitted batch, on the device
        (hipdrt_plan_find_peaks; models/peaks.py is the rule in numpy) -> a list of B arrays of peak tau; with return_info
        (peak_tau, tau, peak_indices, peak_info), the last two per-spectrum lists, every info dict with scipy's peak_heights,
        prominences, left_bases, right_bases and for method 'prob' probs (of all peaks that passed height and prominence, as
        upstream).  Only the height and prominence conditions of scipy.signal.find_peaks are built.  Spectra whose fit failed
        (or, for 'prob', whose P is not positive definite) have no peaks.  Last device batch only."""
        if method not in peaks.METHODS:
            raise ValueError(f'Invalid method {method}. Options: {list(peaks.METHODS)}')
        for name in kw:
            raise NotImplementedError(f'find_peaks: the {name}= argument is not taken (of scipy.signal.find_peaks\' conditions '
                                      f'only height and prominence are built; coefficients and P are the fit\'s own, on the device)')
        if p_matrix is not None:
            raise NotImplementedError('find_peaks: the p_matrix= override is not taken (sigma comes from the fit\'s own P on the device)')
        # (only what the caller asked for comes down: the kept mask alone without return_info)
        want = None if return_info else ('keep',)
        tau, out = self._find_peaks_device('find_peaks', tau, ppd, normalize, sign, method, extend_var, want=want, height=height,
                                           prominence=prominence, prob_thresh=prob_thresh, num_peaks=num_peaks,
                                           fxx_var_floor=fxx_var_floor)
        B = out['keep'].shape[0]

        def per_spectrum(mask):
            """(column indices of the set entries, cut points) -> np.split gives one array per spectrum"""
            rows, cols = np.nonzero(mask)
            return cols, np.searchsorted(rows, np.arange(1, B))

        kept, cut = per_spectrum(out['keep'])
        peak_tau = np.split(tau[kept], cut)
        if not return_info:
            return peak_tau
        peak_indices = np.split(kept, cut)
        _, cut = per_spectrum(out['peak_sign'])
        sel = out['peak_sign'] != 0
        cols = {'peak_heights': out['heights'][sel], 'prominences': out['prominences'][sel],
                'left_bases': out['left_bases'][sel].astype(np.intp), 'right_bases': out['right_bases'][sel].astype(np.intp)}
        if method == 'prob':
            cols['probs'] = out['probs'][sel]
        parts = {k: np.split(v, cut) for k, v in cols.items()}
        peak_info = [{k: parts[k][b] for k in parts} for b in range(B)]
        return peak_tau, tau, peak_indices, peak_info

    def find_peaks(self, tau=None, x=None, normalize=True, ppd=10, prominence=None, height=None, sign=1, return_info=False,
                   method='thresh', prob_thresh=0.25, p_matrix=None, fxx_var_floor=1e-5, extend_var=True, num_peaks=None, b=0, **kw):
        """DRT.find_peaks (drt1d.py:3753-3947) of member ``b`` of the last fit, from the device"""
        if x is not None:
            kw = dict(kw, x=x)
        res = self.find_peaks_batch(tau=tau, normalize=normalize, ppd=ppd, prominence=prominence, height=height, sign=sign,
                                    return_info=True, method=method, prob_thresh=prob_thresh, p_matrix=p_matrix,
                                    fxx_var_floor=fxx_var_floor, extend_var=extend_var, num_peaks=num_peaks, **kw)
        if return_info:
            return res[0][b], res[1], res[2][b], res[3][b]
        return res[0][b]

    def _map_probs(self, what, which, tau, extend_var, prominence, height, sign, normalize):
        return self._find_peaks_device(what, tau, 10, normalize, sign, 'map', extend_var, want=(which,), height=height,
                                       prominence=prominence, fxx_var_floor=0.0)[1][which]

    def peak_prob_batch(self, tau=None, extend_var=True, prominence=5e-3, height=1e-3, sign=1, normalize=True):
        """the per-observation core of DRTMD.predict_peak_prob (drtmd.py:1023-1064: curvature.peak_prob_1d times sign(f)) for every
        spectrum of the last fitted batch -> (B, len(tau)); tau=None is get_tau_eval(10).  No psi filtering, no peak_spread_sigma."""
        return self._map_probs('peak_prob_batch', 'peak_prob', tau, extend_var, prominence, height, sign, normalize)

    def curv_prob_batch(self, tau=None, extend_var=True, prominence=5e-3, height=1e-3, sign=1, normalize=True):
        """the per-observation core of DRTMD.predict_curv_prob (drtmd.py:1066-1106) for every spectrum of the last fitted batch ->
        (B, len(tau)): the probability of f > 0 with negative curvature (or the reverse), signed by f"""
        return self._map_probs('curv_prob_batch', 'curv_prob', tau, extend_var, prominence, height, sign, normalize)

    # ---- per-peak coefficients, distributions and resistances (drt1d.py:3586-3620, 3949-4111; hybdrt/peaks.py:92-217) ------------
    def _resolve_device(self, what, tau_out, tau_find, peak_indices, sign, epsilon_factor, max_epsilon, min_epsilon,
                        epsilon_uniform, want, windows=None, find_peaks_kw=None, peak_tau=None, trough_tau=None,
                        squeeze_factors=None, x=None):
        """hipdrt_plan_resolve_peaks with upstream's defaults -> (padded outputs, tau_find).  On overflow the call is repeated
        once with max_peaks = the largest count (at most 64); spectra beyond 64 keep empty rows and a warning is given."""
        for name, v in (('peak_tau', peak_tau), ('trough_tau', trough_tau), ('squeeze_factors', squeeze_factors)):
            if v is not None:
                raise NotImplementedError(f'{what}: the {name}= argument is not taken (off-grid positions and squeezing act on one '
                                          f'spectrum; peaks and troughs live on the find grid)')
        plan, scales = self._predict_plan(what, x=x)
        fkw = dict(find_peaks_kw or {})
        if peak_indices is not None and tau_find is None and windows is None:
            raise ValueError('If peak_indices are provided, the corresponding tau grid must also be provided')
        if tau_find is None:
            tau_find = fkw.pop('tau', None)
        if tau_find is None:
            tau_find = self.get_tau_eval(fkw.pop('ppd', 10))         # find_peaks' own default; estimate_peak_coef's is the same grid
        tau_find = np.asarray(tau_find, dtype=float)
        dsign = self._drt_sign(plan, sign)
        B = plan.B
        src = {}
        if windows is not None:
            src['windows'] = windows
            mp0 = max(16, len(windows[0]))
        elif peak_indices is not None:
            rows = [np.sort(np.asarray(r, dtype=np.int64).ravel()) for r in (peak_indices if np.ndim(peak_indices[0]) else [peak_indices] * B)] \
                if len(peak_indices) else [np.zeros(0, dtype=np.int64)] * B
            if len(rows) != B:
                raise ValueError(f'{what}: peak_indices must be one row, or one row per spectrum of the batch')
            mp0 = max([16] + [len(r) for r in rows])
            if mp0 > 64:
                raise ValueError(f'{what}: at most 64 peaks per spectrum')
        else:
            for name in ('x', 'p_matrix', 'return_info'):
                if fkw.get(name) is not None:
                    raise NotImplementedError(f'{what}: find_peaks\' {name}= argument is not taken')
                fkw.pop(name, None)
            method = fkw.pop('method', 'thresh')
            if method not in peaks.METHODS:
                raise ValueError(f'Invalid method {method}. Options: {list(peaks.METHODS)}')
            normalize, extend_var = fkw.pop('normalize', True), fkw.pop('extend_var', True)
            fsign = fkw.pop('sign', sign)
            if self._drt_sign(plan, fsign) != dsign:
                raise ValueError(f'{what}: find_peaks runs with the sign of the peak coefficients')
            opt_kw = {k: fkw.pop(k) for k in ('height', 'prominence', 'prob_thresh', 'num_peaks', 'fxx_var_floor') if k in fkw}
            for name in fkw:
                raise NotImplementedError(f'find_peaks: the {name}= argument is not taken (of scipy.signal.find_peaks\' conditions '
                                          f'only height and prominence are built)')
            search = sign if (self.fit_kwargs['nonneg'] and sign != 0) else 0
            ext = self._extend_var_indices(tau_find) if (extend_var and method != 'thresh') else (-1, -1)
            src['find_opts'] = _ffi.peak_opts(eval_sign=dsign, search=search, normalize=1 if normalize else 0, method=method,
                                              ext_left=ext[0], ext_right=ext[1], **opt_kw)
            mp0 = 16
        ln_out = None if tau_out is None else np.log(np.asarray(tau_out, dtype=float))

        def call(mp):
            if peak_indices is not None and windows is None:
                idx = np.full((B, mp), -1, dtype=np.int32)
                for b, r in enumerate(rows):
                    idx[b, :len(r)] = r
                src['peak_indices'] = idx
            o = _ffi.peak_resolve_opts(sign=dsign, max_peaks=mp, epsilon_factor=epsilon_factor, max_epsilon=max_epsilon,
                                       min_epsilon=min_epsilon, epsilon_uniform=epsilon_uniform)
            return plan.resolve_peaks(np.log(tau_find), ln_out, opts=o, row_scale=scales, want=want, **src)

        out = call(mp0)
        over = out['status'] == _ffi.PEAKS_OVERFLOW
        if np.any(over):
            out = call(int(min(64, np.max(out['count'][over]))))
            over = out['status'] == _ffi.PEAKS_OVERFLOW
            if np.any(over):
                warnings.warn(f'{what}: {int(np.sum(over))} spectra have more than 64 peaks and get empty results')
        return out, tau_find

    @staticmethod
    def _cut(out, name):
        """per-spectrum list cut from a padded array (empty for spectra without a result)"""
        ok = out['status'] >= 0
        return [out[name][b, :out['count'][b]].copy() if ok[b] else out[name][b, :0].copy() for b in range(len(ok))]

    def estimate_peak_coef_batch(self, tau=None, peak_indices=None, x=None, sign=1, epsilon_factor=1.25, max_epsilon=1.25,
                                 min_epsilon=None, epsilon_uniform=None, peak_tau=None, trough_tau=None, **find_peaks_kw):
        """DRT.estimate_peak_coef (drt1d.py:3949-3972) for every spectrum of the last fitted batch, on the device
        (hipdrt_plan_resolve_peaks; models/peaks.py resolve_peaks_row is the rule in numpy) -> a list of B arrays
        (peaks, len(basis_tau)) in data units.  tau: the find grid (None: find_peaks' own, get_tau_eval(10)); peak_indices: one
        row for all spectra or one row per spectrum, else find_peaks(**find_peaks_kw) on the device.  Spectra whose fit failed
        have no rows.  Last device batch only."""
        out, _ = self._resolve_device('estimate_peak_coef', None, tau, peak_indices, sign, epsilon_factor, max_epsilon, min_epsilon,
                                      epsilon_uniform, ('x_peaks',), find_peaks_kw=find_peaks_kw, peak_tau=peak_tau,
                                      trough_tau=trough_tau, x=x)
        return self._cut(out, 'x_peaks')

    def _default_peak_sign(self, sign):
        return (0 if self.series_neg else 1) if sign is None else sign

    def estimate_peak_drts_batch(self, tau=None, ppd=10, tau_find_peaks=None, peak_indices=None, x=None, sign=None,
                                 epsilon_factor=1.25, max_epsilon=1.25, min_epsilon=None, epsilon_uniform=None,
                                 squeeze_factors=None, find_peaks_kw=None, peak_tau=None, trough_tau=None):
        """DRT.estimate_peak_drts (drt1d.py:3984-4034) for every spectrum of the last fitted batch -> a list of B arrays
        (peaks, len(tau)): every peak's partial distribution on tau (None: get_tau_eval(ppd)), formed on the device from the
        peak coefficients and the order-0 evaluation matrix.  sign=None: 0 for series_neg fits, else 1."""
        if tau is None:
            tau = self.get_tau_eval(ppd)
        out, _ = self._resolve_device('estimate_peak_drts', tau, tau_find_peaks, peak_indices, self._default_peak_sign(sign),
                                      epsilon_factor, max_epsilon, min_epsilon, epsilon_uniform, ('peak_gammas',),
                                      find_peaks_kw=find_peaks_kw, peak_tau=peak_tau, trough_tau=trough_tau,
                                      squeeze_factors=squeeze_factors, x=x)
        return self._cut(out, 'peak_gammas')

    def quantify_peaks_batch(self, tau=None, ppd=10, tau_find_peaks=None, peak_indices=None, x=None, sign=None,
                             epsilon_factor=1.25, max_epsilon=1.25, min_epsilon=None, epsilon_uniform=None, squeeze_factors=None,
                             find_peaks_kw=None, peak_tau=None, trough_tau=None, return_info=False):
        """DRT.quantify_peaks (drt1d.py:4101-4111) for every spectrum of the last fitted batch -> a list of B arrays of peak
        resistances, np.trapezoid of every peak's distribution over ln(tau); only the resistances (and with return_info the
        peak and trough indices, the length scales and r_coef = predict_r_p of every peak's coefficients) come down."""
        if tau is None:
            tau = self.get_tau_eval(ppd)
        want = ('r_peaks',) + (('peak_index', 'trough_index', 'eps_l', 'eps_r', 'r_coef') if return_info else ())
        out, tau_find = self._resolve_device('quantify_peaks', tau, tau_find_peaks, peak_indices, self._default_peak_sign(sign),
                                             epsilon_factor, max_epsilon, min_epsilon, epsilon_uniform, want,
                                             find_peaks_kw=find_peaks_kw, peak_tau=peak_tau, trough_tau=trough_tau,
                                             squeeze_factors=squeeze_factors, x=x)
        r_peaks = self._cut(out, 'r_peaks')
        if not return_info:
            return r_peaks
        info = {k: self._cut(out, k) for k in want[1:]}
        info['trough_index'] = [t[:max(len(t) - 1, 0)] for t in info['trough_index']]
        info['tau_find_peaks'] = tau_find
        return r_peaks, info

    def _window_kw(self, what, predict_kw):
        kw = dict(predict_kw)
        if kw.pop('x', None) is not None:
            raise NotImplementedError(f'{what}: the x= override is not taken (predictions use the coefficients on the device)')
        order, sign = kw.pop('order', 0), kw.pop('sign', 1)
        normalize, normalize_by, abs_norm = kw.pop('normalize', False), kw.pop('normalize_by', None), kw.pop('abs_norm', False)
        for name in kw:
            raise TypeError(f'{what}: unexpected keyword {name}')
        if order not in (0, 1, 2):
            raise ValueError(f'Invalid order {order}. Options: 0, 1, 2')
        if normalize_by is not None and not normalize_by > 0:
            raise ValueError('normalize_by must be positive')
        return order, sign, normalize, normalize_by, abs_norm

    def _integrate_device(self, what, tau, windows, predict_kw):
        order, sign, normalize, normalize_by, abs_norm = self._window_kw(what, predict_kw)
        plan, scales = self._predict_plan(what)
        by_rp = bool(normalize) and normalize_by is None
        out, _ = plan.integrate_drt(np.log(tau), windows, order=order, sign=self._drt_sign(plan, sign),
                                    normalize=(2 if abs_norm else 1) if by_rp else 0,
                                    row_scale=None if (by_rp or scales is None) else scales)
        return out if normalize_by is None else out / normalize_by

    def split_r_p_batch(self, tau_splits, resolve_peaks=False, **predict_kw):
        """DRT.split_r_p (drt1d.py:3596-3620) for every spectrum of the last fitted batch -> (B, len(tau_splits) + 1): the
        trapezoid of predict_drt's row over the windows between the splits, or with resolve_peaks the resistance
        predict_r_p(x = x_peak) of one resolved peak per window (the minimum of the curvature), all on the device"""
        predict_kw = dict(predict_kw)
        tau = predict_kw.pop('tau', None)
        ppd = predict_kw.pop('ppd', 20)
        tau = self.get_tau_eval(ppd) if tau is None else np.asarray(tau, dtype=float)
        windows = peaks.split_windows(tau, tau_splits)
        if not resolve_peaks:
            return self._integrate_device('split_r_p', tau, windows, predict_kw)
        order, sign, normalize, normalize_by, _ = self._window_kw('split_r_p', predict_kw)
        if order != 0 or normalize or normalize_by is not None:
            raise NotImplementedError('split_r_p(resolve_peaks=True): order, normalize and normalize_by are not taken (upstream '
                                      'applies them to the curvature it searches; the peak resistances carry none)')
        out, _ = self._resolve_device('split_r_p', None, tau, None, 1, 1.25, 1.25, None, None, ('r_coef',), windows=windows)
        nwin = len(windows[0])
        res = out['r_coef'][:, :nwin].copy()
        res[out['status'] < 0] = np.nan
        return res

    def integrate_drt_batch(self, tau_min, tau_max, ppd=10, **predict_kw):
        """DRT.integrate_drt (drt1d.py:3590-3594) for every spectrum of the last fitted batch -> (B,)"""
        num_decades = np.log10(tau_max) - np.log10(tau_min)
        tau = np.logspace(np.log10(tau_min), np.log10(tau_max), int(num_decades * ppd) + 1)
        return self._integrate_device('integrate_drt', tau, ([0], [len(tau)]), predict_kw)[:, 0]

    # single-member forms with the reference's signatures; ``b`` picks a member of the last batch
    def estimate_peak_coef(self, tau=None, peak_indices=None, x=None, sign=1, epsilon_factor=1.25, max_epsilon=1.25,
                           min_epsilon=None, epsilon_uniform=None, peak_tau=None, trough_tau=None, b=0, **find_peaks_kw):
        """DRT.estimate_peak_coef (drt1d.py:3949-3972) of member ``b`` of the last fit, from the device"""
        return self.estimate_peak_coef_batch(tau=tau, peak_indices=peak_indices, x=x, sign=sign, epsilon_factor=epsilon_factor,
                                             max_epsilon=max_epsilon, min_epsilon=min_epsilon, epsilon_uniform=epsilon_uniform,
                                             peak_tau=peak_tau, trough_tau=trough_tau, **find_peaks_kw)[b]

    def estimate_peak_drts(self, tau=None, ppd=10, tau_find_peaks=None, peak_indices=None, x=None, sign=None, epsilon_factor=1.25,
                           max_epsilon=1.25, min_epsilon=None, epsilon_uniform=None, squeeze_factors=None, find_peaks_kw=None,
                           peak_tau=None, trough_tau=None, b=0):
        """DRT.estimate_peak_drts (drt1d.py:3984-4034) of member ``b`` of the last fit, from the device"""
        return self.estimate_peak_drts_batch(tau=tau, ppd=ppd, tau_find_peaks=tau_find_peaks, peak_indices=peak_indices, x=x,
                                             sign=sign, epsilon_factor=epsilon_factor, max_epsilon=max_epsilon,
                                             min_epsilon=min_epsilon, epsilon_uniform=epsilon_uniform,
                                             squeeze_factors=squeeze_factors, find_peaks_kw=find_peaks_kw, peak_tau=peak_tau,
                                             trough_tau=trough_tau)[b]

    def quantify_peaks(self, tau=None, ppd=10, b=0, **estimate_peak_drts_kw):
        """DRT.quantify_peaks (drt1d.py:4101-4111) of member ``b`` of the last fit -> a list of peak resistances"""
        return list(self.quantify_peaks_batch(tau=tau, ppd=ppd, **estimate_peak_drts_kw)[b])

    def split_r_p(self, tau_splits, resolve_peaks=False, b=0, **predict_kw):
        """DRT.split_r_p (drt1d.py:3596-3620) of member ``b`` of the last fit"""
        return self.split_r_p_batch(tau_splits, resolve_peaks=resolve_peaks, **predict_kw)[b]

    def integrate_drt(self, tau_min, tau_max, ppd=10, b=0, **predict_kw):
        """DRT.integrate_drt (drt1d.py:3590-3594) of member ``b`` of the last fit"""
        return float(self.integrate_drt_batch(tau_min, tau_max, ppd=ppd, **predict_kw)[b])

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
