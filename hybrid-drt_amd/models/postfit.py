"""The post-fit methods of DRT (hybdrt/models/drt1d.py:2716-4138): model evaluation, peak finding, per-peak distributions and
resistances, the PFRT and the covariance estimates of the last fitted batch.  Everything runs on the device plan the fit left
(_ffi.Plan / PreparedPlan); this module decides grids and options, states each rule of a request once, and rescales results."""
import warnings

import numpy as np

from .. import _ffi, preprocessing as pp
from ..matrices import basis, mat1d
from . import background, peaks, pfrt as pfrt_rule, predict, response


class PostFitMixin:
    # ---- the rules every request shares, each stated once ------------------------------------------------------------------------
    def _members(self):
        """the prepared measurements of the members of the last batch on a prepared plan"""
        return self._last_prepared[0] if getattr(self, '_last_prepared', None) and \
            len(self._last_prepared[0]) == self._plan.batch else [self._prep]

    def _member_scales(self):
        """(B,) coefficient scales of those members: the device loop of a prepared plan runs at unit scale"""
        return np.array([pr['coefficient_scale'] for pr in self._members()], dtype=float)

    def _need_cov_fit(self):
        if self._plan is None or (self._last_batch is None and not isinstance(self._plan, _ffi.PreparedPlan)):
            raise Exception('Parameter covariance estimation is only available for qphb fits')

    def _extend_var_indices(self, tau, b=0):
        """the two clamp indices of estimate_distribution_cov's extend_var (drt1d.py:3125-3135) on the grid tau, from the measured
        tau range of member ``b`` (the members of a prepared batch share their sampling grids)"""
        if isinstance(self._plan, _ffi.PreparedPlan):
            pr = self._members()[b]
            t_left, t_right = pp.get_tau_lim(pr['frequencies'], pr.get('sample_times'), pr.get('nonconsec_step_times'))
        else:
            t_left, t_right = 1 / (2 * np.pi * np.max(self.f_fit)), 1 / (2 * np.pi * np.min(self.f_fit))
        return int(np.argmin(np.abs(tau - t_left))) + 1, int(np.argmin(np.abs(tau - t_right)))

    def _peak_search(self, sign):
        """the sign find_peaks searches with: the given one for a nonneg fit, else both"""
        return sign if (self.fit_kwargs['nonneg'] and sign != 0) else 0

    def _peak_ext(self, tau, extend_var, refuse_beyond=True):
        """the extend_var clamp indices as the peak options carry them, (-1, -1) without the clamp.  An index beyond the grid is
        refused here for find_peaks, the map probabilities and predict_pfrt; the resolve family leaves it to the library."""
        ext = self._extend_var_indices(tau) if extend_var else (-1, -1)
        if refuse_beyond and ext[0] >= len(tau):
            raise ValueError('extend_var: the measured tau range ends at the last point of the evaluation grid')
        return ext

    def _peak_opts(self, plan, tau, sign, method, normalize, extend_var, opt_kw, refuse_beyond=True):
        """hipdrt_peak_opts of a find_peaks request on the grid tau ('thresh' takes no clamp)"""
        search = self._peak_search(sign)
        ext = self._peak_ext(tau, extend_var and method != 'thresh', refuse_beyond)
        return _ffi.peak_opts(eval_sign=self._drt_sign(plan, sign), search=search, normalize=1 if normalize else 0, method=method,
                              ext_left=ext[0], ext_right=ext[1], **opt_kw)

    @staticmethod
    def _drt_request(order, normalize, normalize_by, abs_norm=False):
        """the checks of a predict_drt request -> (whether it divides by R_p, the normalize code of the device call: 0, 1 by R_p,
        2 by absolute R_p)"""
        if order not in (0, 1, 2):
            raise ValueError(f'Invalid order {order}. Options: 0, 1, 2')
        if normalize_by is not None and not normalize_by > 0:
            raise ValueError('normalize_by must be positive')
        by_rp = bool(normalize) and normalize_by is None
        return by_rp, (2 if abs_norm else 1) if by_rp else 0

    def get_tau_eval(self, ppd):
        """drtbase.get_tau_eval (drtbase.py:263-285): one decade beyond the basis grid on each side."""
        basis_tau = self.basis_tau
        log_min, log_max = np.log10(np.min(basis_tau)) - 1, np.log10(np.max(basis_tau)) + 1
        return np.logspace(log_min, log_max, int((log_max - log_min) * ppd) + 1)

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
        scales = self._member_scales()
        self._plan.set_tau_basis(np.log(self.basis_tau), self.tau_epsilon)
        return self._plan, scales

    def _drt_sign(self, plan, sign):
        two_copies = plan.n - plan.ns == 2 * len(self.basis_tau)
        if sign is None:
            return predict.default_sign(two_copies)              # DRT.default_dist_sign
        if sign not in (-1, 0, 1):
            raise ValueError(f'Invalid sign {sign}. Options: -1, 0, 1')
        return sign if two_copies else 1                         # get_drt_params ignores the sign of a one-copy fit

    def _predict_drt_device(self, what, tau, ppd, order, sign, normalize, normalize_by, abs_norm, quantiles, x=None, p_matrix=None):
        by_rp, code = self._drt_request(order, normalize, normalize_by, abs_norm)
        plan, scales = self._predict_plan(what, x=x, p_matrix=p_matrix)
        sign = self._drt_sign(plan, sign)
        if tau is None:
            tau = self.get_tau_eval(ppd)
        n_sig = None if quantiles is None else predict.n_sigma(quantiles)
        mu, lo, hi, status = plan.predict_drt(np.log(np.asarray(tau, dtype=float)), order=order, sign=sign,
                                              normalize=code, n_sigma=n_sig)
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

    # ---- the voltage response of a chrono / hybrid fit (drt1d.py:3363-3474), on the prepared plan of the last fit ---------------
    def _set_predict_desc(self, plan):
        """gives the prepared plan what extract_qphb_parameters needs (hipdrt_plan_set_predict_desc): the meaning of its special
        columns and the members' post-fit scales, as prepared.py keeps them in each prep"""
        members, sp, kw = self._members(), self.special_qp_params, self.fit_kwargs
        p0 = members[0]
        idx = lambda name: sp[name]['index'] if name in sp else -1
        chrono = p0['num_chrono'] > 0
        plan.set_predict_desc(
            idx('R_inf'), idx('inductance'), idx('C_inv'), kw['inductance_scale'], kw['capacitance_scale'],
            [pr['coefficient_scale'] for pr in members],
            # (solve_rp rescales the DOP columns of every member by that member's own factor)
            dop_scale_vector=np.array([pr['dop_scale_vector'] for pr in members]) if p0['dop'] else None,
            v_baseline_scale=p0['v_baseline_scale'] if chrono else None,
            response_signal_scale=[pr['response_signal_scale'] for pr in members] if chrono else None,
            scaled_response_offset=[pr['scaled_response_offset'] for pr in members] if chrono else None)

    def _response_request(self, what, times, input_signal, step_times, step_sizes, op_mode, offset_steps, step_offset_size, x,
                          subtract_background, y_bkg):
        """the checks and defaults of a predict_response request (drt1d.py:3369-3387, 5994-6045) -> (plan, times, step_times,
        step_sizes (S,) or (B, S), the input signal behind a measured ohmic response or None)"""
        if subtract_background is False and y_bkg is None:
            raise NotImplementedError(f'{what}: subtract_background=False without y_bkg is not taken (no chrono background is '
                                      f'fitted here)')
        if (op_mode if op_mode is not None else self.chrono_mode) != 'galv':
            raise NotImplementedError(f"{what}: op_mode='pot' is not taken (galvanostatic prediction only)")
        if self.step_model != 'ideal':
            raise NotImplementedError(f'{what}: step_model={self.step_model!r} is not taken (ideal steps only)')
        plan, scales = self._predict_plan(what, x=x)
        if scales is None or self._members()[0].get('num_chrono', 0) == 0:
            raise RuntimeError(f'{what} needs a finished chrono or hybrid fit (fit_chrono, fit_hybrid, fit_hybrid_batch)')
        members = self._members()
        if input_signal is not None and step_times is not None:
            raise ValueError('Either input_signal OR (step_times and step_sizes) should be provided; '
                             'received input_signal and step_times')
        if step_times is not None and step_sizes is None:
            raise ValueError('If input signal steps are provided, both step_times and step_sizes must be provided; '
                             'received step_times only')
        kw = self.fit_kwargs
        offset_steps = kw['offset_steps'] if offset_steps is None else offset_steps
        step_offset_size = kw['step_offset_size'] if step_offset_size is None else step_offset_size
        times = members[0]['sample_times'] if times is None else np.asarray(times, dtype=float)
        signals = None
        if input_signal is None and step_times is None:
            # the fitted signal: the members of one protocol share their step times, their measured step sizes differ
            step_times = members[0]['step_times']
            if any(not np.array_equal(pr['step_times'], step_times) for pr in members[1:]):
                raise ValueError(f'{what}: the members of the batch do not share their step times; give step_times and step_sizes')
            step_sizes = np.array([pr['step_sizes'] for pr in members])
            signals = [pr['raw_input_signal'] for pr in members]
        elif step_times is None:
            input_signal = np.asarray(input_signal, dtype=float)
            step_times, step_sizes, _ = pp.process_input_signal(times, input_signal, self.step_model, offset_steps, step_offset_size)
            signals = [input_signal] * len(members)
        step_times, step_sizes = np.asarray(step_times, dtype=float), np.asarray(step_sizes, dtype=float)
        if step_sizes.shape not in ((len(step_times),), (len(members), len(step_times))):
            raise ValueError(f'{what}: step_sizes must have one entry per step, or one row of them per member of the batch')
        return plan, times, step_times, step_sizes, signals

    def predict_response_batch(self, times=None, input_signal=None, step_times=None, step_sizes=None, op_mode=None,
                               offset_steps=None, step_offset_size=None, include_dop=True, include_drt=True, include_ohmic=True,
                               include_cap=True, smooth_inf_response=None, x=None, include_vz_offset=True,
                               subtract_background=True, y_bkg=None, v_baseline=None, include_baseline=True):
        """DRT.predict_response (drt1d.py:3363-3464) for every member of the last chrono / hybrid fit, at ANY times -> (B, nt);
        times=None: the fit times, no signal and no steps: the fitted steps with every member's own step sizes.  The unit-step
        response layers (and the phasor layers of a fit_dop fit) are built once for the batch on the device and applied to the
        resident coefficients (hipdrt_plan_predict_response; models/response.py is the rule in numpy); the host forms only the
        O(nt) ohmic and capacitance response vectors, the vz-offset strength at ``times`` and the baseline features.  y_bkg and
        v_baseline, when given, are added as upstream adds them.  Rows of failed fits are NaN.  Ideal steps, galvanostatic;
        last device batch only."""
        what = 'predict_response'
        plan, times, step_times, step_sizes, signals = self._response_request(
            what, times, input_signal, step_times, step_sizes, op_mode, offset_steps, step_offset_size, x, subtract_background, y_bkg)
        members, sp, kw = self._members(), self.special_qp_params, self.fit_kwargs
        p0, B = members[0], len(members)
        smooth = kw['smooth_inf_response'] if smooth_inf_response is None else smooth_inf_response
        rows = step_sizes if step_sizes.ndim == 2 else step_sizes[None, :]
        if not smooth and signals is None:
            # given steps: upstream measures the ohmic response on the model signal of those steps (drt1d.py:6020-6021)
            signals = [pp.generate_model_signal(times, step_times, rows[b if step_sizes.ndim == 2 else 0], None, self.step_model)
                       for b in range(B)]
        if not smooth and len(signals[0]) != len(times):
            raise ValueError(f'{what}: smooth_inf_response=False takes the ohmic response from the input signal, which must be '
                             f'given at the prediction times')
        per_member = lambda fn: np.array([fn(b) for b in range(len(rows))]) if step_sizes.ndim == 2 else fn(0)
        inf_rv = cap_rv = strength = vb_mat = None
        if 'R_inf' in sp and include_ohmic:
            # the ideal steps, or (smooth_inf_response=False) every member's own signal minus its pre-step mean
            inf_of = lambda b: mat1d.construct_ohmic_response_vector(
                times, self.step_model, step_times, rows[b if step_sizes.ndim == 2 else 0], None,
                None if smooth else signals[b], smooth)
            inf_rv = per_member(inf_of) if smooth else np.array([inf_of(b) for b in range(B)])
        if 'C_inv' in sp and include_cap:
            cap_rv = per_member(lambda b: mat1d.construct_capacitance_response_vector(times, self.step_model, step_times,
                                                                                      rows[b], None))
        if 'vz_offset' in sp and include_vz_offset:
            strength = self._vz_strength(p0['sample_times'], p0['frequencies'], p0['nonconsec_step_times'], kw['vz_offset_eps'],
                                         times=times)[0]
        if include_baseline and v_baseline is None:
            vb_mat = background.get_baseline_matrix(times, int(kw['v_baseline_deg']), normalize=False,
                                                    sqrt=bool(kw['v_baseline_sqrt']))
        mask = (_ffi.INCLUDE_DRT * bool(include_drt) | _ffi.INCLUDE_OHMIC * bool(include_ohmic) | _ffi.INCLUDE_CAP * bool(include_cap)
                | _ffi.INCLUDE_DOP * bool(include_dop) | _ffi.INCLUDE_VZ_OFFSET * bool(include_vz_offset)
                | _ffi.INCLUDE_BASELINE * (vb_mat is not None))
        interp = self.integrate_method == 'interp'
        self._set_predict_desc(plan)
        out, _ = plan.predict_response(
            times, step_times, step_sizes, basis_tau=self.basis_tau, mode=_ffi.MODE_INTERP if interp else _ffi.MODE_TRAPZ,
            lookup=self._lookups(plan.ctx)['response'] if interp else None,
            basis_nu=self.basis_nu if p0['dop'] else None, nu_epsilon=self.nu_epsilon if p0['dop'] else 0.0,
            inf_rv=inf_rv, cap_rv=cap_rv, vz_strength=strength, vb_mat=vb_mat, include_mask=mask)
        if v_baseline is not None:
            out = out + np.asarray(v_baseline, dtype=float)
        if not subtract_background:
            if len(times) != len(y_bkg):
                raise ValueError('Length of background does not match length of times')
            out = out + np.asarray(y_bkg, dtype=float)
        return out

    def predict_response(self, times=None, input_signal=None, step_times=None, step_sizes=None, op_mode=None, offset_steps=None,
                         step_offset_size=None, include_dop=True, include_drt=True, include_ohmic=True, include_cap=True,
                         smooth_inf_response=None, x=None, include_vz_offset=True, subtract_background=True, y_bkg=None,
                         v_baseline=None, b=0):
        """DRT.predict_response (drt1d.py:3363-3464) of member ``b`` of the last chrono / hybrid fit, from the device.  The whole
        batch is predicted and downloaded and row ``b`` returned: for many members call predict_response_batch once."""
        return self.predict_response_batch(
            times=times, input_signal=input_signal, step_times=step_times, step_sizes=step_sizes, op_mode=op_mode,
            offset_steps=offset_steps, step_offset_size=step_offset_size, include_dop=include_dop, include_drt=include_drt,
            include_ohmic=include_ohmic, include_cap=include_cap, smooth_inf_response=smooth_inf_response, x=x,
            include_vz_offset=include_vz_offset, subtract_background=subtract_background, y_bkg=y_bkg, v_baseline=v_baseline)[b]

    def predict_v_baseline(self, times, x_vb=None, b=0):
        """DRT.predict_v_baseline (drt1d.py:3466-3473) of member ``b`` of the last chrono / hybrid fit: the baseline term of the
        device prediction alone (of the whole batch, row ``b`` returned)"""
        if x_vb is not None:
            raise NotImplementedError('predict_v_baseline: the x_vb= override is not taken (the coefficients are the fit\'s own, '
                                      'on the device)')
        return self.predict_response_batch(times=times, include_dop=False, include_drt=False, include_ohmic=False,
                                           include_cap=False, include_vz_offset=False)[b]

    # ---- impedance and distribution of phasances of a prepared fit (drt1d.py:3273-3361, 3500-3542) ------------------------------
    def predict_z_model_batch(self, frequencies=None, include_vz_offset=True, include_dop=True, include_drt=True,
                              include_inductance=True, include_ohmic=True, include_cap=True, x=None):
        """DRT.predict_z (drt1d.py:3500-3542) for every member of the last fit on a PREPARED plan -- hybrid, fit_dop,
        fit_capacitance, solve_rp, series_neg and outlier-removal fits -- at ANY frequencies -> complex (B, nf);
        frequencies=None: the fit frequencies.  The impedance matrices and the phasor-Z rows of a DOP block are built on the device
        at the requested frequencies and applied to the resident coefficients; R_inf, the inductance, C_inv and the DOP term are
        added in data units and the result is multiplied by 1 - vz_offset * strength(f) (hipdrt_plan_predict_z_model;
        models/response.py is the rule in numpy).  Every term is switchable as upstream's include_* flags switch it.  Rows of
        failed fits are NaN.  Plain EIS fits have predict_z_batch.  Last device batch only."""
        what = 'predict_z_model_batch'
        plan, scales = self._predict_plan(what, x=x)
        if scales is None:
            raise NotImplementedError(f'{what} is built for fits on a prepared plan (hybrid, fit_dop, fit_capacitance, solve_rp, '
                                      f'series_neg); a plain EIS fit has predict_z_batch')
        p0, sp, kw = self._members()[0], self.special_qp_params, self.fit_kwargs
        if frequencies is None:
            if p0['frequencies'] is None:
                raise ValueError(f'{what}: a chrono fit has no fit frequencies; give frequencies')
            frequencies = p0['frequencies']
        f = np.asarray(frequencies, dtype=float)
        strength = None
        if 'vz_offset' in sp and include_vz_offset:
            strength = self._vz_strength(p0['sample_times'], p0['frequencies'], p0['nonconsec_step_times'], kw['vz_offset_eps'],
                                         predict_frequencies=f)[1]
        mask = (_ffi.INCLUDE_DRT * bool(include_drt) | _ffi.INCLUDE_OHMIC * bool(include_ohmic) | _ffi.INCLUDE_CAP * bool(include_cap)
                | _ffi.INCLUDE_DOP * bool(include_dop) | _ffi.INCLUDE_VZ_OFFSET * bool(include_vz_offset)
                | _ffi.INCLUDE_INDUCTANCE * bool(include_inductance))
        interp = self.integrate_method == 'interp'
        self._set_predict_desc(plan)
        return plan.predict_z_model(f, basis_tau=self.basis_tau, mode=_ffi.MODE_INTERP if interp else _ffi.MODE_TRAPZ,
                                    lookups=self._lookups(plan.ctx)['z'] if interp else None,
                                    basis_nu=self.basis_nu if p0['dop'] else None, nu_epsilon=self.nu_epsilon if p0['dop'] else 0.0,
                                    vz_strength=strength, include_mask=mask)[0]

    def predict_dop_batch(self, nu=None, x=None, normalize=False, normalize_tau=None, order=0, return_nu=False,
                          normalize_quantiles=(0, 1), delta_density=False, include_ideal=True):
        """DRT.predict_dop (drt1d.py:3273-3347) for every member of the last fit_dop fit -> (B, len(nu)), with return_nu
        (nu, dop).  nu=None is upstream's grid: 1001 points on [-1, 1] joined with basis_nu and the ideal elements' -1, 0, 1.  The
        evaluation rows are built on the device and applied to the resident DOP block with the member's dop_scale_vector and coefficient
        scale (hipdrt_plan_predict_dop); normalize divides by get_dop_norm (3349-3361; normalize_tau=None: the measured tau range);
        include_ideal adds R_inf, the inductance and C_inv at nu = 0, 1, -1 as upstream adds them.  Rows of failed fits are NaN."""
        what = 'predict_dop'
        if delta_density:
            raise NotImplementedError(f'{what}: delta_density=True is not taken')
        if order != 0:
            raise NotImplementedError(f'{what}: order={order} is not taken (order 0 only)')
        plan, scales = self._predict_plan(what, x=x)
        p0 = self._members()[0]
        if scales is None or not p0['dop']:
            raise RuntimeError(f'{what} needs a finished fit with fit_dop=True')
        if nu is None:
            nu = np.unique(np.concatenate([self.basis_nu, np.linspace(-1, 1, 1001)]))
            nu = np.unique(np.concatenate([nu, np.array([-1, 0, 1])]))
        else:
            nu = np.sort(np.asarray(nu, dtype=float))
        area = np.sqrt(np.pi) / self.nu_epsilon
        normalize_by = None
        if normalize:
            if normalize_tau is None:
                normalize_tau = pp.get_tau_lim(p0['frequencies'], p0.get('sample_times'), p0.get('step_times'))
            normalize_by = response.dop_norm(nu, normalize_tau, self.nu_epsilon, normalize_quantiles)
        self._set_predict_desc(plan)
        dop = plan.predict_dop(nu, self.basis_nu, self.nu_epsilon, normalize_by=normalize_by, nu_basis_area=area,
                               include_ideal=include_ideal)[0]
        return (nu, dop) if return_nu else dop

    def predict_dop(self, nu=None, x=None, normalize=False, normalize_tau=None, order=0, return_nu=False,
                    normalize_quantiles=(0, 1), delta_density=False, include_ideal=True, b=0):
        """DRT.predict_dop (drt1d.py:3273-3347) of member ``b`` of the last fit_dop fit, from the device (the whole batch is
        predicted, row ``b`` returned)"""
        nu, dop = self.predict_dop_batch(nu=nu, x=x, normalize=normalize, normalize_tau=normalize_tau, order=order, return_nu=True,
                                         normalize_quantiles=normalize_quantiles, delta_density=delta_density,
                                         include_ideal=include_ideal)
        return (nu, dop[b]) if return_nu else dop[b]

    # ---- the posterior of the distribution of phasances (drt1d.py:3153-3198, 3233-3258) on the prepared plan of the last fit --------
    def _dop_grid(self):
        """predict_dop's default grid (drt1d.py:3275-3280)"""
        nu = np.unique(np.concatenate([self.basis_nu, np.linspace(-1, 1, 1001)]))
        return np.unique(np.concatenate([nu, np.array([-1, 0, 1])]))

    def _dop_posterior_request(self, what, nu, default_nu, normalize, normalize_tau, normalize_quantiles, order, delta_density,
                               x=None, p_matrix=None):
        """the checks of a DOP posterior request -> (plan, the ascending grid, the permutation that sorted the caller's nu,
        get_dop_norm's vector on the grid or None, the area of one nu basis function); default_nu() is the grid of nu=None"""
        if delta_density:
            raise NotImplementedError(f'{what}: delta_density=True is not taken')
        if order not in (0, 1, 2):
            raise ValueError(f'Invalid order {order}. Options: 0, 1, 2')
        plan, scales = self._predict_plan(what, x=x, p_matrix=p_matrix)
        p0 = self._members()[0]
        if scales is None or not p0['dop']:
            raise RuntimeError(f'{what} needs a finished fit with fit_dop=True')
        nu = np.asarray(default_nu() if nu is None else nu, dtype=float).ravel()
        perm = np.argsort(nu, kind='stable')
        nu = nu[perm]
        normalize_by = None
        if normalize:
            if normalize_tau is None:
                normalize_tau = pp.get_tau_lim(p0['frequencies'], p0.get('sample_times'), p0.get('step_times'))
            normalize_by = response.dop_norm(nu, normalize_tau, self.nu_epsilon, normalize_quantiles)
        self._set_predict_desc(plan)
        return plan, nu, perm, normalize_by, np.sqrt(np.pi) / self.nu_epsilon

    def predict_dop_ci_batch(self, nu=None, normalize=False, normalize_tau=None, quantiles=(0.025, 0.975), order=0,
                             normalize_quantiles=(0.25, 0.75), delta_density=False, include_ideal=True, return_info=False):
        """DRT.predict_dop_ci (drt1d.py:3233-3258) for every member of the last fit_dop fit -> (lo, hi, ok), each band (B, len(nu)):
        the mean of derivative order 0, 1 or 2 plus the quantiles' numbers of posterior standard deviations, sigma^2 =
        diag(E D inv(P) D E') coefficient_scale^2 / normalize_by^2 with D = diag(dop_scale_vector) of that member (under solve_rp
        every member has its own).  Everything is formed on the device from the resident coefficients and the fit's own final
        P (hipdrt_plan_dop_posterior): one Gram/L2 rebuild and one Cholesky factorisation per member.  ok (B,) bool is False where
        the fit failed or P is not positive definite (rows NaN; upstream returns (None, None)).  return_info adds a dict: nu, mu,
        sigma, status.

        Where upstream is inconsistent: with nu=None its covariance is taken on basis_nu and its mean on predict_dop's
        1034-point grid, so its own predict_dop_ci(nu=None) adds arrays of different lengths; here both use predict_dop's grid.
        An unsorted nu is sorted by upstream for the mean only; here mean and sigma are both on the sorted grid, which is
        info['nu'].  Upstream adds no variance for R_inf, the inductance and C_inv (include_ideal), and neither is any added here.
        normalize_quantiles defaults to upstream's (0.25, 0.75) for this method, not predict_dop's (0, 1).  Last device batch only."""
        what = 'predict_dop_ci'
        plan, nu, _, normalize_by, area = self._dop_posterior_request(
            what, nu, self._dop_grid, normalize, normalize_tau, normalize_quantiles, order, delta_density)
        mu, lo, hi, var, status = plan.dop_posterior(nu, self.basis_nu, self.nu_epsilon, order=order, normalize_by=normalize_by,
                                                     nu_basis_area=area, include_ideal=include_ideal,
                                                     n_sigma=predict.n_sigma(quantiles), want_var=bool(return_info))
        ok = status >= 0
        if return_info:
            return lo, hi, ok, dict(nu=nu, mu=mu, sigma=np.sqrt(var), status=status)
        return lo, hi, ok

    def predict_dop_ci(self, nu=None, x=None, normalize=False, normalize_tau=None, quantiles=(0.025, 0.975), order=0,
                       normalize_quantiles=(0.25, 0.75), delta_density=False, include_ideal=True, b=0):
        """DRT.predict_dop_ci (drt1d.py:3233-3258) of member ``b`` of the last fit_dop fit: (lo, hi) on the sorted grid, or
        (None, None) with upstream's warning when P is not positive definite.  The choices of predict_dop_ci_batch hold."""
        if x is not None:
            raise NotImplementedError('predict_dop_ci: the x= override is not taken (predictions use the coefficients on the device)')
        lo, hi, ok = self.predict_dop_ci_batch(nu=nu, normalize=normalize, normalize_tau=normalize_tau, quantiles=quantiles,
                                               order=order, normalize_quantiles=normalize_quantiles, delta_density=delta_density,
                                               include_ideal=include_ideal)
        if not ok[b]:
            warnings.warn('Singular P matrix - could not obtain covariance estimate')
            return None, None
        return lo[b], hi[b]

    def estimate_dop_var_batch(self, nu=None, normalize=False, normalize_tau=None, normalize_quantiles=(0.25, 0.75), order=0,
                               delta_density=False):
        """np.diag(DRT.estimate_dop_cov(...)) (drt1d.py:3153-3198) for every member of the last fit_dop fit -> (var (B, len(nu)),
        ok (B,) bool), from the device (hipdrt_plan_dop_posterior without a mean or a band).  nu=None is basis_nu, as upstream's
        covariance takes it; the rows come back in the order of the caller's nu."""
        plan, nu, perm, normalize_by, area = self._dop_posterior_request(
            'estimate_dop_var', nu, lambda: self.basis_nu, normalize, normalize_tau, normalize_quantiles, order,
            delta_density)
        _, _, _, var, status = plan.dop_posterior(nu, self.basis_nu, self.nu_epsilon, order=order, normalize_by=normalize_by,
                                                  nu_basis_area=area, include_ideal=False)
        out = np.empty_like(var)
        out[:, perm] = var
        return out, status >= 0

    def estimate_dop_cov(self, nu=None, p_matrix=None, normalize=False, normalize_tau=None, normalize_quantiles=(0.25, 0.75),
                         var_floor=0.0, order=0, delta_density=False, b=0):
        """DRT.estimate_dop_cov (drt1d.py:3153-3198) of member ``b`` of the last fit_dop fit: E x_cov[dop, dop] E' with x_cov =
        estimate_param_cov's inv(P) coefficient_scale^2, rescaled on both sides by dop_scale_vector, formed on the device from
        the Cholesky factor of the scaled P (hipdrt_plan_dop_cov).  nu=None is basis_nu as upstream; rows and columns follow the
        caller's nu.  With normalize upstream divides by get_dop_norm's vector squared as a plain broadcast -- column j by
        normalize_by[j]^2 -- so the matrix is not symmetric; exactly that is kept, and its diagonal is what the band uses.
        var_floor is applied to the returned diagonal on the host, as upstream applies it.  None (with upstream's warning) when
        P is not positive definite."""
        plan, nu, perm, normalize_by, area = self._dop_posterior_request(
            'estimate_dop_cov', nu, lambda: self.basis_nu, normalize, normalize_tau, normalize_quantiles, order,
            delta_density, p_matrix=p_matrix)
        cov, status = plan.dop_cov(b, nu, self.basis_nu, self.nu_epsilon, order=order, normalize_by=normalize_by, nu_basis_area=area)
        if status < 0:
            warnings.warn('Singular P matrix - could not obtain covariance estimate')
            return None
        out = np.empty_like(cov)
        out[np.ix_(perm, perm)] = cov
        if var_floor > 0:
            var = np.diag(out).copy()
            var[var < var_floor] = var_floor
            np.fill_diagonal(out, var)
        return out

    # ---- peak finding (drt1d.py:3753-3947; mapping/curvature.py, mapping/drtmd.py:1023-1106) on the last fitted batch ------------
    def _find_peaks_device(self, what, tau, ppd, normalize, sign, method, extend_var, want=None, **opt_kw):
        plan, scales = self._predict_plan(what)
        if tau is None:
            tau = self.get_tau_eval(ppd)
        tau = np.asarray(tau, dtype=float)
        opts = self._peak_opts(plan, tau, sign, method, normalize, extend_var, opt_kw)
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

    # ---- peak and trough probabilities and find_peaks_byprob (drt1d.py:3655-3750; mapping/surface.py:265-350) --------------------
    def _peak_prob_device(self, what, tau, bayes_cov, want, search='rows', height=None, prominence=None, ranges=None, x=None,
                          p_matrix=None, prob=None):
        """hipdrt_plan_peak_trough_probs on the grid tau (None: get_tau_eval(10)) -> (tau, outputs): f, fx, fxx as predict_drt
        gives them at its defaults (sign 1, not normalised), with bayes_cov the clamp indices of extend_var=True; the ranges
        become index windows here, from the very tau array (peaks.range_windows: tau must be strictly increasing).  Rows of a
        failed fit (with bayes_cov: of a P that is not positive definite) are NaN and carry no peaks.  Last device batch only."""
        if prob is not None:
            raise NotImplementedError(f'{what}: the prob= override is not taken (the probability is formed on the device from the '
                                      f'fit\'s own coefficients and P)')
        plan, scales = self._predict_plan(what, x=x, p_matrix=p_matrix)
        tau = self.get_tau_eval(10) if tau is None else np.asarray(tau, dtype=float)
        windows = None if ranges is None else peaks.range_windows(tau, ranges)
        if windows is not None and not 1 <= len(windows) <= 64:
            raise ValueError(f'{what}: between 1 and 64 peak_tau_ranges')
        ext = self._peak_ext(tau, bool(bayes_cov))
        opts = _ffi.peak_prob_opts(bayes_cov=bayes_cov, ext_left=ext[0], ext_right=ext[1], search=search, height=height,
                                   prominence=prominence)
        return tau, plan.peak_trough_probs(np.log(tau), opts, row_scale=scales, ranges=windows, want=want)

    def predict_peak_trough_probs_batch(self, tau=None, bayes_cov=True):
        """DRT.predict_peak_trough_probs (drt1d.py:3655-3690) for every spectrum of the last fitted batch, on the device
        (hipdrt_plan_peak_trough_probs; models/peaks.py peak_trough_probs_rows is the rule in numpy) -> (pp, tp), each (B, len(tau)).
        bayes_cov: sigma of f, fx and fxx from ONE factorisation of every spectrum's final P, floored per order; else the windowed
        standard deviation of every row."""
        out = self._peak_prob_device('predict_peak_trough_probs', tau, bayes_cov, ('pp', 'tp'))[1]
        return out['pp'], out['tp']

    def predict_peak_prob_batch(self, tau=None, bayes_cov=True):
        """DRT.predict_peak_prob (drt1d.py:3692-3718) for every spectrum of the last fitted batch -> (B, len(tau)): pp * (1 - tp)"""
        return self._peak_prob_device('predict_peak_prob', tau, bayes_cov, ('prob',))[1]['prob']

    def _find_peaks_byprob_device(self, tau, height, prominence, bayes_cov, peak_tau_ranges, return_info, **overrides):
        what = 'find_peaks_byprob'
        if peak_tau_ranges is not None:
            tau, out = self._peak_prob_device(what, tau, bayes_cov, ('range_peaks',), search='ranges', ranges=peak_tau_ranges,
                                              **overrides)
            # (a failed fit has -1 in every slot: no peaks)
            peak_indices = [r[r >= 0].astype(np.intp) for r in out['range_peaks']]
            peak_info = [{} for _ in peak_indices]
        else:
            names = {'heights': 'peak_heights', 'prominences': 'prominences', 'left_bases': 'left_bases', 'right_bases': 'right_bases'}
            want = ('keep',)
            if return_info:
                want += (('heights',) if height is not None else ()) + \
                    (('prominences', 'left_bases', 'right_bases') if prominence is not None else ())
            tau, out = self._peak_prob_device(what, tau, bayes_cov, want, search='thresh', height=height, prominence=prominence,
                                              **overrides)
            B = len(out['status'])
            rows, cols = np.nonzero(out['keep'])
            cut = np.searchsorted(rows, np.arange(1, B))
            peak_indices = np.split(cols, cut)
            sel = out['keep'] != 0
            parts = {names[k]: np.split(out[k][sel].astype(np.intp) if k.endswith('bases') else out[k][sel], cut) for k in want[1:]}
            peak_info = [{k: parts[k][b] for k in parts} for b in range(B)]
        peak_tau = [tau[i] for i in peak_indices]
        return (peak_tau, tau, peak_indices, peak_info) if return_info else peak_tau

    def find_peaks_byprob_batch(self, tau=None, height=None, prominence=None, bayes_cov=True, peak_tau_ranges=None,
                                return_info=False):
        """DRT.find_peaks_byprob (drt1d.py:3720-3750) for every spectrum of the last fitted batch, probability and search on the
        device -> a list of B arrays of peak tau; with return_info (peak_tau, tau, peak_indices, peak_info), the first and the
        last two per-spectrum lists.  With peak_tau_ranges (at most 64) one peak per range (peaks.find_peaks_byrange) and empty
        info dicts; else scipy.signal.find_peaks(prob, height=, prominence=), the info dicts with exactly scipy's keys for the
        conditions given (peak_heights; prominences, left_bases, right_bases)."""
        return self._find_peaks_byprob_device(tau, height, prominence, bayes_cov, peak_tau_ranges, return_info)

    # single-member forms with the reference's signatures; ``b`` picks a member of the last batch
    def predict_peak_trough_probs(self, tau=None, x=None, bayes_cov=True, p_matrix=None, b=0):
        """DRT.predict_peak_trough_probs (drt1d.py:3655-3690) of member ``b`` of the last fit, from the device -> (pp, tp)"""
        out = self._peak_prob_device('predict_peak_trough_probs', tau, bayes_cov, ('pp', 'tp'), x=x, p_matrix=p_matrix)[1]
        return out['pp'][b], out['tp'][b]

    def predict_peak_prob(self, tau=None, x=None, bayes_cov=True, p_matrix=None, b=0):
        """DRT.predict_peak_prob (drt1d.py:3692-3718) of member ``b`` of the last fit, from the device"""
        return self._peak_prob_device('predict_peak_prob', tau, bayes_cov, ('prob',), x=x, p_matrix=p_matrix)[1]['prob'][b]

    def find_peaks_byprob(self, tau=None, x=None, prob=None, height=None, prominence=None, bayes_cov=True, p_matrix=None,
                          peak_tau_ranges=None, return_info=False, b=0):
        """DRT.find_peaks_byprob (drt1d.py:3720-3750) of member ``b`` of the last fit, from the device"""
        res = self._find_peaks_byprob_device(tau, height, prominence, bayes_cov, peak_tau_ranges, True, x=x, p_matrix=p_matrix,
                                             prob=prob)
        return (res[0][b], res[1], res[2][b], res[3][b]) if return_info else res[0][b]

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
            src['find_opts'] = self._peak_opts(plan, tau_find, sign, method, normalize, extend_var, opt_kw, refuse_beyond=False)
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
        return order, sign, normalize, normalize_by, abs_norm

    def _integrate_device(self, what, tau, windows, predict_kw):
        order, sign, normalize, normalize_by, abs_norm = self._window_kw(what, predict_kw)
        by_rp, code = self._drt_request(order, normalize, normalize_by, abs_norm)
        plan, scales = self._predict_plan(what)
        out, _ = plan.integrate_drt(np.log(tau), windows, order=order, sign=self._drt_sign(plan, sign), normalize=code,
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
        self._drt_request(order, normalize, normalize_by)
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

    def _pfrt_chain(self, what, tau_pfrt, sign, prior_mu, prior_sigma, find_peaks_kw, n_eff_factor, fxx_var_floor, extend_var):
        """what predict_pfrt_batch and select_pfrt_candidates_batch ask of the chain up to the raw PFRT, with its refusals ->
        (plan, tau_pfrt, the fields of hipdrt_pfrt_opts the chain reads, factors)"""
        if self.series_neg:
            raise NotImplementedError(f'{what}: series_neg fits are not taken (upstream\'s normalize=True raises for them)')
        if isinstance(self._plan, _ffi.PreparedPlan):
            raise NotImplementedError(f'{what} is built for plain EIS fits; a prepared plan records its steps and gives '
                                      'step_p_matrix only')
        plan = self._pfrt_plan(what)
        fkw = dict(find_peaks_kw or {'height': 1e-3, 'prominence': 5e-3})
        for name in fkw:
            if name not in ('height', 'prominence'):
                raise NotImplementedError(f'{what}: the {name}= condition of scipy.signal.find_peaks is not built '
                                          f'(only height and prominence)')
        sign = self._drt_sign(plan, sign)
        tau_pfrt = self.get_tau_eval(10) if tau_pfrt is None else np.asarray(tau_pfrt, dtype=float)
        search, ext = self._peak_search(sign), self._peak_ext(tau_pfrt, extend_var)
        chain = dict(eval_sign=sign, search=search, height=fkw.get('height', 0), prominence=fkw.get('prominence', 0),
                     prior_mu=prior_mu, prior_sigma=prior_sigma, n_eff_factor=n_eff_factor, fxx_var_floor=fxx_var_floor,
                     ext_left=ext[0], ext_right=ext[1])
        factors = np.asarray(self.pfrt_result['factors'], dtype=float)
        if len(factors) != plan.pfrt_steps():
            raise ValueError(f"pfrt_result['factors'] has {len(factors)} entries, the plan recorded {plan.pfrt_steps()} steps")
        return plan, tau_pfrt, chain, factors

    @staticmethod
    def _pfrt_finish(smooth=True, smooth_kw=None, integrate=False, integrate_threshold=1e-6, normalize=True):
        """the fields of hipdrt_pfrt_opts behind predict_pfrt's last stage (drt1d.py:2840-2858), from its keywords"""
        skw = dict(smooth_kw or {'order': 2, 'epsilon': 5})
        if set(skw) - {'order', 'epsilon'}:
            raise TypeError(f"unexpected smooth_kw {sorted(set(skw) - {'order', 'epsilon'})}")
        return dict(smooth=bool(smooth), smooth_order=skw.get('order', 2), smooth_epsilon=skw.get('epsilon', 5),
                    integrate=bool(integrate), integrate_threshold=integrate_threshold, normalize=bool(normalize))

    def predict_pfrt_batch(self, tau=None, tau_pfrt=None, sign=None, prior_mu=-4, prior_sigma=0.5, find_peaks_kw=None,
                           n_eff_factor=0.5, fxx_var_floor=1e-5, extend_var=True, smooth=True, smooth_kw=None, integrate=False,
                           integrate_threshold=1e-6, normalize=True, return_info=False):
        """DRT.predict_pfrt (drt1d.py:2716-2858) for every spectrum of the last PFRT fit -> (B, len(tau)), on the device over the
        recorded steps (hipdrt_plan_predict_pfrt; models/pfrt.py is the rule in numpy).  tau_pfrt=None is get_tau_eval(10), tau=None
        is tau_pfrt (without smooth the result stays on tau_pfrt, as upstream).  With return_info also a dict with tau_pfrt,
        raw_pfrt (B, n), step_pfrt (S, B, n), post_prob (S, B) and status (B,), the first three also stored into pfrt_result under
        upstream's keys.  Rows of spectra whose fit failed in any step, or whose step P is not positive definite, are NaN.  Of
        find_peaks_kw only height and prominence are built; plain EIS fits only.  select_pfrt_candidates has its own device pass
        (select_pfrt_candidates_batch); the discrete-model conversion stays with the reference's Python on these arrays."""
        finish = self._pfrt_finish(smooth, smooth_kw, integrate, integrate_threshold, normalize)
        plan, tau_pfrt, chain, factors = self._pfrt_chain('predict_pfrt', tau_pfrt, sign, prior_mu, prior_sigma, find_peaks_kw,
                                                          n_eff_factor, fxx_var_floor, extend_var)
        tau_out = tau_pfrt if (tau is None or not smooth) else np.asarray(tau, dtype=float)
        opts = _ffi.pfrt_opts(**finish, **chain)
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

    # ---- DRT.select_pfrt_candidates (drt1d.py:2860-2865 over hybdrt/models/pfrt.py:164-213) on the device ----------------------
    def select_pfrt_candidates_batch(self, start_thresh=0.99, end_thresh=0.01, peak_thresh=1e-6, max_peaks=16, return_info=False,
                                     tau_pfrt=None, sign=None, prior_mu=-4, prior_sigma=0.5, find_peaks_kw=None, n_eff_factor=0.5,
                                     fxx_var_floor=1e-5, extend_var=True, pfrt_kw=None):
        """DRT.select_pfrt_candidates for every spectrum of the last PFRT fit, in one device pass over the recorded steps
        (hipdrt_plan_pfrt_select; models/pfrt.py select_compact is the rule in numpy) -> a list of B pairs (target_peak_indices,
        step_indices) in upstream's form: candidate j is the set of the first + j + 1 most probable peaks of the raw PFRT (indices
        into tau_pfrt) and the recorded step whose own PFRT matches it best.  Entry b is None where member b has no answer: a
        negative status (a failed fit, a step P that is not positive definite), _ffi.PFRT_NO_PEAK (nothing at or above
        peak_thresh; upstream raises) or _ffi.PFRT_TOO_MANY_PEAKS (more ranges than max_peaks).  The fit's own non-negative
        statuses are live, as in predict_pfrt_batch: 1, a step that ended at its iteration limit, is how PFRT steps usually
        end.  Peaks of equal area rank the higher index first; np.argmax picks the step, so the first NaN (an all-zero shifted
        row) wins.  tau_pfrt ... extend_var are predict_pfrt_batch's keywords for the chain up to the raw PFRT, with the same
        refusals.
        Without return_info only the compact arrays and the status come down (a few numbers per spectrum; none of the rows),
        and pfrt_result stays as it is.  With return_info also a dict with the compact arrays (num_peaks, ranked_index,
        magnitude, first, num_candidates, step_index, match_quality), raw_pfrt, step_pfrt, post_prob, tau_pfrt and status;
        tau_pfrt, raw_pfrt and step_pfrt are then stored into pfrt_result, as predict_pfrt_batch does with return_info.
        pfrt_kw (with return_info; a dict of predict_pfrt_batch's tau, smooth, smooth_kw, integrate, integrate_threshold,
        normalize; may be empty): the dict also holds 'pfrt', that method's result from the same pass, the same bits."""
        plan, tau_pfrt, chain, factors = self._pfrt_chain('select_pfrt_candidates', tau_pfrt, sign, prior_mu, prior_sigma,
                                                          find_peaks_kw, n_eff_factor, fxx_var_floor, extend_var)
        want, finish, ln_tau_out = _ffi.PFRT_SELECT_COMPACT, {}, None
        if return_info:
            want = want + _ffi.PFRT_SELECT_ROWS[:3]
            if pfrt_kw is not None:
                fkw = dict(pfrt_kw)
                tau = fkw.pop('tau', None)
                finish = self._pfrt_finish(**fkw)
                want = want + ('pfrt',)
                if tau is not None and finish['smooth']:
                    ln_tau_out = np.log(np.asarray(tau, dtype=float))
        elif pfrt_kw is not None:
            raise ValueError('select_pfrt_candidates_batch: pfrt_kw goes with return_info=True')
        out = plan.pfrt_select(factors, np.log(tau_pfrt), _ffi.pfrt_opts(**finish, **chain),
                               _ffi.pfrt_select_opts(start_thresh, end_thresh, peak_thresh, max_peaks), want=want,
                               ln_tau_out=ln_tau_out)
        no_answer = (out['status'] < 0) | np.isin(out['status'], (_ffi.PFRT_NO_PEAK, _ffi.PFRT_TOO_MANY_PEAKS))
        pairs = [None if no_answer[b] else pfrt_rule.candidates_from_compact({k: out[k][b] for k in _ffi.PFRT_SELECT_COMPACT})
                 for b in range(len(no_answer))]
        if not return_info:
            return pairs
        self.pfrt_result.update(tau_pfrt=tau_pfrt, raw_pfrt=out['raw_pfrt'], step_pfrt=out['step_pfrt'])
        return pairs, dict(out, tau_pfrt=tau_pfrt)

    def select_pfrt_candidates(self, start_thresh=0.99, end_thresh=0.01, peak_thresh=1e-6, b=0):
        """DRT.select_pfrt_candidates (drt1d.py:2860-2865) of member ``b`` of the last PFRT fit, from the device ->
        (target_peak_indices, step_indices).  Upstream reads pfrt_result here and writes nothing to it; neither does this, and
        no row comes down.  ValueError where the raw PFRT has nothing at or above peak_thresh (upstream fails there inside
        find_contiguous_ranges)."""
        plan, tau_pfrt, chain, factors = self._pfrt_chain('select_pfrt_candidates', None, None, -4, 0.5, None, 0.5, 1e-5, True)
        out = plan.pfrt_select(factors, np.log(tau_pfrt), _ffi.pfrt_opts(**chain),
                               _ffi.pfrt_select_opts(start_thresh, end_thresh, peak_thresh), want=_ffi.PFRT_SELECT_COMPACT)
        status = int(out['status'][b])
        if status == _ffi.PFRT_NO_PEAK:
            raise ValueError(f'select_pfrt_candidates: no value of the raw PFRT at or above peak_thresh={peak_thresh}')
        if status < 0 or status == _ffi.PFRT_TOO_MANY_PEAKS:
            raise RuntimeError(f'select_pfrt_candidates: member {b} has status {status}')
        return pfrt_rule.candidates_from_compact({k: out[k][b] for k in _ffi.PFRT_SELECT_COMPACT})

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

    def _cov_rows(self, tau, ppd, sign, order=0):
        """(tau as an array, the evaluation rows (order 0 unless asked otherwise) of a covariance estimate on it)"""
        tau = np.asarray(self.get_tau_eval(ppd) if tau is None else tau, dtype=float)
        bm = basis.construct_func_eval_matrix(np.log(self.basis_tau), np.log(tau), self.tau_basis_type, epsilon=self.tau_epsilon, order=order)
        return tau, self._signed_basis(bm, sign)

    def estimate_distribution_var_batch(self, tau=None, ppd=20, extend_var=False, sign=1, order=0):
        """Diagonal of DRT.estimate_distribution_cov (drt1d.py:3063-3151; no normalisation) for every
        spectrum of the last fitted batch: diag(B P^-1 B') coefficient_scale^2, computed on the device from the
        Cholesky factor of each final P.  Returns (var (B, len(tau)), ok (B,) bool); ``extend_var`` applies the
        reference's clamp outside the measured tau range (drt1d.py:3126-3143).  ``order``: the derivative of the basis the rows
        evaluate (0: the DRT; 2: its curvature, the fxx variance of DRTMD.predict_drt_var, hybdrt/mapping/drtmd.py:980-991)."""
        self._need_cov_fit()
        prepared = isinstance(self._plan, _ffi.PreparedPlan)
        tau, bm = self._cov_rows(tau, ppd, sign, order)
        var, status = self._plan.distribution_var(bm, self._plan.batch if prepared else self._last_batch)
        if prepared:     # the device loop of a prepared plan runs at unit scale: estimate_param_cov's coefficient_scale^2 is applied here
            var = var * self._member_scales()[:, None] ** 2
        if extend_var:
            left_index, right_index = self._extend_var_indices(tau)
            var[:, :left_index] = np.maximum(var[:, :left_index], var[:, left_index][:, None])
            var[:, right_index:] = np.maximum(var[:, right_index:], var[:, right_index][:, None])
        return var, status == 0

    def estimate_param_var_batch(self):
        """np.diag(DRT.estimate_param_cov()) (drt1d.py:4116-4138) for every spectrum of the last fitted batch, from the
        Cholesky factor of each final P on the device.  Returns (var (B, n), ok (B,) bool)."""
        self._need_cov_fit()
        prepared = isinstance(self._plan, _ffi.PreparedPlan)
        var, status = self._plan.param_var(self._plan.batch if prepared else self._last_batch)
        if prepared:     # the prepared loop runs at unit scale: coefficient_scale^2 of estimate_param_cov applied here
            var = var * self._member_scales()[:, None] ** 2
        return var, status == 0

    def _cov_scale(self, b):
        """(coefficient_scale of fitted measurement b where the device loop ran at unit scale, else 1; its prep or None)"""
        if isinstance(self._plan, _ffi.PreparedPlan):
            prep = self._members()[b]
            return prep['coefficient_scale'], prep
        return 1.0, None

    def estimate_param_cov(self, b=0):
        """DRT.estimate_param_cov (drt1d.py:4116-4138): inv(P) * coefficient_scale^2 with the DOP block rescaled by
        dop_scale_vector, from the Cholesky factor of the final P on the device (hipdrt_plan_param_cov); ``b`` picks a
        member of the last batch.  None (with upstream's warning) when P is not positive definite."""
        self._need_cov_fit()
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
        self._need_cov_fit()
        tau, bm = self._cov_rows(tau, ppd, sign)
        cov, ok = self._plan.distribution_cov(bm, b)
        if not ok:
            warnings.warn('Singular P matrix - could not obtain covariance estimate')
            return None
        cs, prep = self._cov_scale(b)
        cov = cov * cs ** 2
        if extend_var:
            left_index, right_index = self._extend_var_indices(tau, b)
            var = np.diag(cov).copy()
            var[:left_index] = np.maximum(var[:left_index], var[left_index])
            var[right_index:] = np.maximum(var[right_index:], var[right_index])
            cov[np.diag_indices(cov.shape[0])] = var
        if var_floor > 0:
            var = np.diag(cov).copy()
            var[var < var_floor] = var_floor
            np.fill_diagonal(cov, var)
        return cov
