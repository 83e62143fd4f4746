"""Model evaluation of a finished fit in numpy: the prediction methods of hybdrt.models.DRT (hybdrt/models/drt1d.py:2965-3061
predict_drt, 3209-3231 predict_drt_ci, 3500-3542 predict_z, 3552-3584 predict_r_p / predict_r_inf / predict_r_tot) written as
functions of the fitted coefficients.

Like ``models/kk.py`` for ``csrc/kk.hip``, this module is the specification of the device path (``csrc/predict.hip`` behind
``hipdrt_plan_predict_drt``, ``hipdrt_plan_predict_z`` and ``hipdrt_plan_predict_resistances``): CPU tests hold it to runs of
the reference, GPU tests hold the device to it.  It makes no device call; a fitted ``DRT`` does not use it -- its predictions
are formed on the device from the coefficients that are resident there.

All coefficients here are in data units (``fit_parameters['x']`` = solution * coefficient_scale, R_inf, inductance).
"""
import numpy as np

from . import kk


def eval_matrix(basis_tau, tau, epsilon, order=0):
    """basis.construct_func_eval_matrix(ln basis_tau, ln tau, 'gaussian', epsilon, order) (hybdrt/matrices/basis.py:488-514 with
    218-228): E[i, j] = phi^(order)(ln tau_i - ln basis_tau_j), phi(y) = exp(-(epsilon y)^2)"""
    if order not in (0, 1, 2):
        raise ValueError(f'Invalid order {order}. Options: 0, 1, 2')
    y = np.log(np.asarray(tau, dtype=float))[:, None] - np.log(np.asarray(basis_tau, dtype=float))[None, :]
    phi = np.exp(-(epsilon * y) ** 2)
    if order == 0:
        return phi
    if order == 1:
        return -2 * epsilon ** 2 * y * phi
    return (-2 * epsilon ** 2 + 4 * epsilon ** 4 * y ** 2) * phi


def default_sign(series_neg):
    """DRT.default_dist_sign (drt1d.py:2989-2994): the net distribution of a series_neg fit, else the distribution itself"""
    return 0 if series_neg else 1


def drt_params(x, num_basis, sign=1):
    """DRT.get_drt_params (drt1d.py:2965-2987): a series_neg fit carries [positive copy | negative copy]; sign 1 -> +x+,
    -1 -> -x-, 0 -> x+ - x-.  A fit with one copy returns x whatever the sign, as upstream."""
    x = np.asarray(x, dtype=float)
    if x.shape[-1] == num_basis:
        return x
    if x.shape[-1] != 2 * num_basis:
        raise ValueError(f'x holds {x.shape[-1]} coefficients for a basis of {num_basis}')
    if sign == 1:
        return x[..., :num_basis]
    if sign == -1:
        return -x[..., num_basis:]
    if sign == 0:
        return x[..., :num_basis] - x[..., num_basis:]
    raise ValueError(f'Invalid sign {sign}. Options: -1, 0, 1')


def basis_area(epsilon):
    """basis.get_basis_func_area for the gaussian basis: sqrt(pi) / epsilon"""
    return np.sqrt(np.pi) / epsilon


def r_p(x, epsilon, absolute=False):
    """DRT.predict_r_p (drt1d.py:3552-3571) of signed coefficients x (drt_params): the polarisation resistance"""
    x = np.asarray(x, dtype=float)
    return (np.sum(np.abs(x), axis=-1) if absolute else np.sum(x, axis=-1)) * basis_area(epsilon)


def r_tot(x, r_inf, epsilon):
    """DRT.predict_r_tot (drt1d.py:3583-3584): R_inf + R_p"""
    return r_inf + r_p(x, epsilon)


def drt(x, basis_tau, tau, epsilon, order=0, sign=1, normalize=False, normalize_by=None, abs_norm=False):
    """DRT.predict_drt (drt1d.py:3040-3061): gamma^(order)(tau) = E x / norm, norm = R_p of the same signed coefficients with
    ``normalize`` (get_drt_norm, 3020-3031), ``normalize_by`` when given, else 1"""
    xs = drt_params(x, len(basis_tau), sign)
    if normalize_by is None:
        normalize_by = r_p(xs, epsilon, absolute=abs_norm) if normalize else 1
    return eval_matrix(basis_tau, tau, epsilon, order) @ xs / normalize_by


def n_sigma(quantiles=(0.025, 0.975)):
    """(s_lo, s_hi): the numbers of standard deviations of the two quantiles, through the reference's tabulated quantile
    function (stats.std_normal_quantile, restated in models.kk)"""
    q_lo, q_hi = quantiles
    return kk.std_normal_quantile(q_lo), kk.std_normal_quantile(q_hi)


def band(mu, sigma, quantiles=(0.025, 0.975)):
    """DRT.predict_drt_ci (drt1d.py:3209-3231) from the mean and the posterior standard deviation: mu + s sigma per quantile"""
    s_lo, s_hi = n_sigma(quantiles)
    mu, sigma = np.asarray(mu, dtype=float), np.asarray(sigma, dtype=float)
    return mu + s_lo * sigma, mu + s_hi * sigma


def impedance(a_re, a_im, x, r_inf, inductance, frequencies, include_drt=True, include_ohmic=True, include_inductance=True):
    """DRT.predict_z(include_vz_offset=False) (drt1d.py:3500-3542) of a plain EIS fit: (A' + j A'') x + R_inf + j 2 pi f L with
    A', A'' the impedance matrices at ``frequencies`` (mat1d.construct_impedance_matrix) and every term switchable"""
    frequencies = np.asarray(frequencies, dtype=float)
    z = np.zeros(len(frequencies), dtype=complex)
    if include_drt:
        z += (np.asarray(a_re) + 1j * np.asarray(a_im)) @ np.asarray(x, dtype=float)
    if include_ohmic:
        z += r_inf
    if include_inductance:
        z += inductance * 2j * np.pi * frequencies
    return z
