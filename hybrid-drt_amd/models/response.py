"""Model evaluation of a chrono, hybrid or DOP fit in numpy: DRT.predict_response and predict_v_baseline
(hybdrt/models/drt1d.py:3363-3474), predict_z with every term of a prepared fit (3500-3542) and predict_dop (3273-3361), with the
parameter rescaling of extract_qphb_parameters (6228-6289) and the vz-offset strength of _get_vz_strength_vec (6173-6226), written
as functions of host arrays.

Like ``models/predict.py`` for the DRT and impedance predictions of a plain EIS fit, this module is the specification of the device
path (``response_assemble_kernel``, ``z_model_assemble_kernel`` and ``dop_assemble_kernel`` of ``csrc/predict.hip`` behind
``hipdrt_plan_predict_response``, ``hipdrt_plan_predict_z_model`` and ``hipdrt_plan_predict_dop``): CPU tests hold it to runs of the
reference, GPU tests hold the device to it.  It makes no device call; a fitted ``DRT`` does not use it.  It sums as the device
does: every step's layer is applied to the coefficients first, then the steps are added in ascending order with their sizes.
"""
import numpy as np

from .. import preprocessing as pp


def vz_strength(times=None, frequencies=None, fit_times=None, step_times=None, fit_frequencies=None, vz_offset_eps=1):
    """DRT._get_vz_strength_vec (drt1d.py:6173-6226) at any ``times`` / ``frequencies`` against the overlap limits of the FIT's
    times, (non-consecutive) step times and frequencies -> (chrono strength or None, eis strength or None): 1 where the two data
    sets overlap in time scale, a Gaussian decay in log time scale away from the overlap, 0 before the first step.  Without both
    data sets, or without vz_offset_eps, the strengths are 1."""
    if fit_times is None or fit_frequencies is None or vz_offset_eps is None:
        return (None if times is None else np.ones(len(times)),
                None if frequencies is None else np.ones(len(frequencies)))
    rbf = lambda y, eps: np.exp(-(eps * y) ** 2)
    fit_deltas = pp.get_time_since_step(fit_times, step_times, prestep_value=-1)
    chrono_tau_min = np.min(fit_deltas[fit_deltas > 0])
    eis_tau_max = np.max(1 / (2 * np.pi * np.asarray(fit_frequencies)))
    cs = es = None
    if times is not None:
        deltas = pp.get_time_since_step(times, step_times, prestep_value=-1)
        cs = np.ones(len(deltas))
        far = deltas >= eis_tau_max
        cs[far] = rbf(np.log(deltas[far] / eis_tau_max), vz_offset_eps)
        cs[deltas == -1] = 0
    if frequencies is not None:
        f_inv = 1 / (2 * np.pi * np.asarray(frequencies))
        es = np.ones(len(f_inv))
        fast = f_inv <= chrono_tau_min
        es[fast] = rbf(np.log(f_inv[fast] / chrono_tau_min), vz_offset_eps)
    return cs, es


def fit_parameters(x, ns, coefficient_scale, idx_rinf=-1, idx_cinv=-1, capacitance_scale=1.0, vz_index=-1, vb_start=0,
                   v_baseline_scale=None, scaled_response_offset=0.0, response_signal_scale=1.0, dop_start=0,
                   dop_scale_vector=None, idx_induc=-1, inductance_scale=1.0, with_abs=False):
    """DRT.extract_qphb_parameters (drt1d.py:6228-6289) of one scaled solution ``x``: the entries predict_response reads, in data
    units.  The baseline coefficients lose their column normalisation, the first one the scaled offset, then all take the
    response scale; the DOP block takes dop_scale_vector * coefficient_scale.  ``with_abs`` adds 'v_baseline_abs', the magnitudes the
    baseline coefficients are formed from (what a rounding-error bound of the baseline term is stated against).  This is the one
    statement of the rule on the host: PreparedFitMixin._extract fills fit_parameters through it."""
    x = np.asarray(x)                # (any float type: the GPU tests evaluate this module in extended precision)
    cs = coefficient_scale
    fp = {'x': x[ns:] * cs, 'R_inf': x[idx_rinf] * cs if idx_rinf >= 0 else 0,
          'inductance': x[idx_induc] * (cs * inductance_scale) if idx_induc >= 0 else 0,
          'C_inv': x[idx_cinv] * (cs * capacitance_scale) if idx_cinv >= 0 else 0}
    if v_baseline_scale is not None and len(v_baseline_scale):
        vbx = x[vb_start:vb_start + len(v_baseline_scale)] * (1.0 / np.asarray(v_baseline_scale))
        vbx[0] -= scaled_response_offset
        fp['v_baseline'] = vbx * response_signal_scale
        if with_abs:
            mag = np.abs(x[vb_start:vb_start + len(v_baseline_scale)] * (1.0 / np.asarray(v_baseline_scale)))
            mag[0] += np.abs(scaled_response_offset)
            fp['v_baseline_abs'] = mag * np.abs(response_signal_scale)
    if vz_index >= 0:
        fp['vz_offset'] = x[vz_index]
    if dop_scale_vector is not None and len(dop_scale_vector):
        fp['x_dop'] = x[dop_start:dop_start + len(dop_scale_vector)] * (np.asarray(dop_scale_vector) * cs)
    return fp


def predict_v_baseline_rows(vb_mat, fp):
    """DRT.predict_v_baseline (drt1d.py:3466-3473): vb_mat @ v_baseline, zero for a fit without a baseline"""
    if 'v_baseline' not in fp or vb_mat is None:
        return 0.0
    return np.asarray(vb_mat) @ np.asarray(fp['v_baseline'])


def predict_response_rows(u_drt, step_sizes, fp, u_dop=None, inf_rv=None, cap_rv=None, vz_strength=None, vb_mat=None,
                          include_drt=True, include_ohmic=True, include_cap=True, include_dop=True, include_vz_offset=True,
                          include_baseline=True, return_abs=False):
    """DRT.predict_response (drt1d.py:3363-3464) of one member from its parameters ``fp`` in data units (fit_parameters) -> (nt,).

    u_drt (S, nt, ntau) and u_dop (S, nt, n_nu) are the unit-step layers of mat1d.construct_response_matrix and
    phasance.construct_phasor_v_matrix (their ``layered`` output for step sizes 1); step_sizes (S,).  fp['x'] holds one copy of the
    basis, or two (series_neg: the second copy enters with a minus sign, rm = [rm, -rm], drt1d.py:6112-6113).  A term whose
    layers or vector is None is left out, as is one switched off.  ``return_abs`` also returns the same expression over the
    absolute values of every product: the magnitude a rounding-error bound of the device result is stated against."""
    sizes = np.asarray(step_sizes)
    nt = next(np.shape(a)[-2 if np.ndim(a) == 3 else 0] for a in (u_drt, u_dop, inf_rv, cap_rv, vz_strength, vb_mat) if a is not None)
    dtype = np.result_type(sizes.dtype, np.float64)
    v, mag = np.zeros(nt, dtype), np.zeros(nt, dtype)

    def layers(u, x):
        acc, acc_abs = np.zeros(nt, dtype), np.zeros(nt, dtype)
        for s in range(len(sizes)):
            acc = acc + sizes[s] * (u[s] @ x)
            acc_abs = acc_abs + np.abs(sizes[s]) * (np.abs(u[s]) @ np.abs(x))
        return acc, acc_abs

    if include_drt and u_drt is not None:
        u = np.asarray(u_drt)
        x, ntau = np.asarray(fp['x']), u.shape[2]
        if len(x) == 2 * ntau:
            u = np.concatenate([u, -u], axis=2)
        elif len(x) != ntau:
            raise ValueError(f'x holds {len(x)} coefficients for a basis of {ntau}')
        t, t_abs = layers(u, x)
        v, mag = v + t, mag + t_abs
    if include_dop and u_dop is not None and fp.get('x_dop') is not None:
        t, t_abs = layers(np.asarray(u_dop), np.asarray(fp['x_dop']))
        v, mag = v + t, mag + t_abs
    if include_ohmic and inf_rv is not None:
        v, mag = v + np.asarray(inf_rv) * fp.get('R_inf', 0), mag + np.abs(np.asarray(inf_rv) * fp.get('R_inf', 0))
    if include_cap and cap_rv is not None:
        v, mag = v + fp.get('C_inv', 0) * np.asarray(cap_rv), mag + np.abs(fp.get('C_inv', 0) * np.asarray(cap_rv))
    if include_vz_offset and vz_strength is not None:
        v = v * (1 + fp.get('vz_offset', 0) * np.asarray(vz_strength))
        mag = mag * (1 + np.abs(fp.get('vz_offset', 0) * np.asarray(vz_strength)))
    if include_baseline and vb_mat is not None and 'v_baseline' in fp:
        v = v + predict_v_baseline_rows(vb_mat, fp)
        mag = mag + np.abs(np.asarray(vb_mat)) @ np.asarray(fp.get('v_baseline_abs', np.abs(fp['v_baseline'])))
    return (v, mag) if return_abs else v


def predict_z_model_rows(a_re, a_im, frequencies, fp, zm_dop=None, eis_strength=None, include_drt=True, include_ohmic=True,
                         include_inductance=True, include_cap=True, include_dop=True, include_vz_offset=True, return_abs=False):
    """DRT.predict_z (drt1d.py:3500-3542) of one member from its parameters ``fp`` in data units -> complex (nf,).

    a_re, a_im (nf, ntau): the impedance matrices at ``frequencies`` (mat1d.construct_impedance_matrix); fp['x'] holds one copy of
    the basis or two (series_neg: zm = [zm, -zm], drt1d.py:6168-6169); zm_dop (nf, n_nu) complex: phasance.construct_phasor_z_matrix;
    eis_strength (nf,): the eis half of vz_strength, None leaves the vz-offset factor out.  ``return_abs`` also returns the sum of
    the absolute values of every product, real and imaginary parts taken together."""
    frequencies = np.asarray(frequencies)
    ctype = np.result_type(frequencies.dtype, np.complex128)
    z, mag = np.zeros(len(frequencies), dtype=ctype), np.zeros(len(frequencies), dtype=frequencies.dtype)
    if include_drt and a_re is not None:
        x, ntau = np.asarray(fp['x']), np.shape(a_re)[1]
        zm = np.asarray(a_re) + 1j * np.asarray(a_im)
        if len(x) == 2 * ntau:
            zm = np.hstack((zm, -zm))
        elif len(x) != ntau:
            raise ValueError(f'x holds {len(x)} coefficients for a basis of {ntau}')
        z, mag = z + zm @ x, mag + (np.abs(zm.real) + np.abs(zm.imag)) @ np.abs(x)
    if include_ohmic:
        z, mag = z + fp.get('R_inf', 0), mag + np.abs(fp.get('R_inf', 0))
    if include_inductance:
        t = fp.get('inductance', 0) * 2j * np.pi * frequencies
        z, mag = z + t, mag + np.abs(t.imag)
    if include_cap:
        t = fp.get('C_inv', 0) * (2j * np.pi * frequencies) ** -1
        z, mag = z + t, mag + np.abs(t.imag)
    if include_dop and zm_dop is not None and fp.get('x_dop') is not None:
        zd, xd = np.asarray(zm_dop), np.asarray(fp['x_dop'])
        z, mag = z + zd @ xd, mag + (np.abs(zd.real) + np.abs(zd.imag)) @ np.abs(xd)
    if include_vz_offset and eis_strength is not None:
        z = z * (1 - fp.get('vz_offset', 0) * np.asarray(eis_strength))
        mag = mag * (1 + np.abs(fp.get('vz_offset', 0) * np.asarray(eis_strength)))
    return (z, mag) if return_abs else z


def dop_norm(nu, normalize_tau, nu_epsilon, normalize_quantiles=(0, 1)):
    """DRT.get_dop_norm (drt1d.py:3349-3361) with normalize=True: phasance.phasor_scale_vector(nu, normalize_tau, quantiles) over
    the area of one Gaussian nu basis function, sqrt(pi) / nu_epsilon"""
    from ..matrices import phasance
    return phasance.phasor_scale_vector(nu, np.array(normalize_tau), normalize_quantiles) / (np.sqrt(np.pi) / nu_epsilon)


def predict_dop_rows(basis_matrix, nu, fp, normalize_by=None, nu_basis_area=1.0, include_ideal=True, return_abs=False):
    """DRT.predict_dop (drt1d.py:3273-3347; order 0, no delta_density) of one member -> (len(nu),): basis_matrix (len(nu), n_nu) =
    basis.construct_func_eval_matrix(basis_nu, nu, 'gaussian', nu_epsilon) applied to fp['x_dop'], divided by normalize_by (dop_norm;
    None: not normalised), plus the ideal elements where nu is exactly 0 (R_inf), 1 (inductance) and -1 (C_inv) -- delta functions,
    so with normalisation they are divided by normalize_by * nu_basis_area instead"""
    nu, xd = np.asarray(nu), np.asarray(fp['x_dop'])
    dop, mag = np.asarray(basis_matrix) @ xd, np.abs(np.asarray(basis_matrix)) @ np.abs(xd)
    if normalize_by is not None:
        dop, mag = dop / normalize_by, mag / normalize_by
    if include_ideal:
        for at, key in ((0, 'R_inf'), (1, 'inductance'), (-1, 'C_inv')):
            idx = np.where(nu == at)
            e = fp.get(key, 0)
            if normalize_by is not None:
                e = e / (np.asarray(normalize_by)[idx] * nu_basis_area)
            dop[idx] += e
            mag[idx] += np.abs(e)
    return (dop, mag) if return_abs else dop


def dop_cov_rows(p_matrix, dop_start, dop_scale_vector, coefficient_scale, basis_matrix, normalize_by=None):
    """DRT.estimate_dop_cov (drt1d.py:3153-3198; no delta_density, var_floor left to the caller) of one member -> (nn, nn), by
    upstream's route: np.linalg.inv of the fit's P, the two-sided rescaling of its DOP block by dop_scale_vector and the factor
    coefficient_scale^2 of estimate_param_cov (4126-4133), then basis_matrix @ x_cov[dop, dop] @ basis_matrix.T with basis_matrix
    (nn, dop_size) = basis.construct_func_eval_matrix(basis_nu, nu, 'gaussian', nu_epsilon, order).  normalize_by (nn,) is
    get_dop_norm's vector (dop_norm; None: not normalised): upstream divides by its square as a plain broadcast, so column j is
    divided by normalize_by[j]^2 and the matrix is no longer symmetric; the diagonal is what the band uses.  A singular P raises
    np.linalg.LinAlgError (upstream warns and returns None).  The device forms the same quantity from the Cholesky factor of
    S P S, S = diag(1 / dop_scale_vector) on the DOP block (scale_p_kernel, csrc/predict.hip)."""
    p_inv = np.linalg.inv(np.asarray(p_matrix, dtype=float))
    dsv = np.asarray(dop_scale_vector, dtype=float)
    a, e = int(dop_start), int(dop_start) + len(dsv)
    dop_scale_mat = np.tile(dsv, (len(p_inv), 1))
    p_inv[:, a:e] *= dop_scale_mat
    p_inv[a:e, :] *= dop_scale_mat.T
    x_cov = (p_inv * coefficient_scale ** 2)[a:e, a:e]
    bm = np.asarray(basis_matrix, dtype=float)
    cov = bm @ x_cov @ bm.T
    if normalize_by is not None:
        cov = cov / np.asarray(normalize_by, dtype=float) ** 2
    return cov


def dop_band(mu, var, quantiles=(0.025, 0.975)):
    """DRT.predict_dop_ci (drt1d.py:3233-3258) from the mean and the diagonal of dop_cov_rows: (mu + s_lo sigma, mu + s_hi sigma),
    sigma = var ** 0.5, s the quantiles' numbers of standard deviations (stats.std_normal_quantile)"""
    from . import predict
    s_lo, s_hi = predict.n_sigma(quantiles)
    mu, sigma = np.asarray(mu, dtype=float), np.asarray(var, dtype=float) ** 0.5
    return mu + s_lo * sigma, mu + s_hi * sigma
