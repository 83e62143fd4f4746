"""Plan and PreparedPlan: the fit loop of a batch on the device and its post-fit entry points."""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .abi import *            # noqa: F401,F403 (the constants and structures)
from .abi import _check, _f64, _i32, _p, _pi, _vp, load_library
from .args import Bound, pfrt_select_bound, resolve_bound
from .opts import (_index_windows, _kk_outputs, _peak_out_args, _peak_outputs, _peak_prob_out_args, _peak_prob_outputs, _resolve_out_struct, _resolve_outputs, default_fit_opts, peak_opts,
                   peak_resolve_opts, pfrt_opts, pfrt_select_opts)


class Plan:
    """hipdrt_plan: shared matrices + work space for `capacity` spectra on one frequency / tau grid."""

    def __init__(self, ctx: Context, freq, tau, epsilon, wt_re=None, wt_im=None, mode=MODE_INTERP,
                 toeplitz_a=False, toeplitz_m=False, opts: FitOpts | None = None, capacity=1, ny=1000):
        self._lib = load_library()
        self.ctx = ctx
        freq, tau = _f64(freq), _f64(tau)
        self.freq, self.tau = freq, tau
        if mode == MODE_INTERP:
            wt_re, wt_im = _f64(wt_re), _f64(wt_im)
            lre, lim = np.log(wt_re), np.log(wt_im)
            ng = wt_re.size
        else:
            wt_re = wt_im = lre = lim = None
            ng = 0
        self.log_wt_re, self.log_wt_im = lre, lim
        self.opts = opts if opts is not None else default_fit_opts()
        h = _vp()
        _check(self._lib.hipdrt_plan_create(ctx._h, _p(freq), freq.size, _p(tau), tau.size, float(epsilon), int(mode),
                                            int(bool(toeplitz_a)), int(bool(toeplitz_m)), ng, int(ny), _p(wt_re),
                                            _p(wt_im), _p(lre), _p(lim), C.byref(self.opts), int(capacity),
                                            C.byref(h)))
        self._h = h
        if os.environ.get("HIPDRT_SUBBATCHES"):           # tools / A-B runs
            self.set_subbatches(int(os.environ["HIPDRT_SUBBATCHES"]))
        n, m, ns = C.c_int(), C.c_int(), C.c_int()
        _check(self._lib.hipdrt_plan_dims(self._h, C.byref(n), C.byref(m), C.byref(ns)))
        self.n, self.m, self.ns = n.value, m.value, ns.value
        self.nf, self.ntau, self.ngrid = freq.size, tau.size, ng
        self.capacity = int(capacity)
        self.B = 0

    def close(self):
        if getattr(self, "_h", None):
            self._lib.hipdrt_plan_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def get(self, which):
        shapes = {"lut_z_re": (self.ngrid,), "lut_z_im": (self.ngrid,), "a_re": (self.nf, self.ntau),
                  "a_im": (self.nf, self.ntau), "rm": (self.m, self.n), "m0": (self.n, self.n),
                  "m1": (self.n, self.n), "m2": (self.n, self.n), "vmm": (self.m, self.m), "h": (self.n,),
                  "est_weights": (self.batch, self.m), "rv": (self.batch, self.m), "xmx": (self.batch, 3),
                  "outlier_t": (self.batch, self.m), "row_factors": (self.batch, self.m), "x": (self.batch, self.n),
                  "coef_scale": (self.batch,), "var_floor": (self.batch,)}
        out = np.empty(shapes[which])
        _check(self._lib.hipdrt_plan_get(self._h, which.encode(), _p(out), out.size))
        return out

    def set_lookup(self, z_re, z_im):
        z_re, z_im = _f64(z_re), _f64(z_im)
        _check(self._lib.hipdrt_plan_set_lookup(self._h, _p(z_re), _p(z_im)))

    batch = 0      # spectra of the last upload

    def upload(self, z):
        z = np.asarray(z)
        if z.ndim == 1:
            z = z[None, :]
        z_re, z_im = _f64(z.real), _f64(z.imag)
        _check(self._lib.hipdrt_plan_upload(self._h, z.shape[0], _p(z_re), _p(z_im)))
        self.batch = z.shape[0]
        self.B = z.shape[0]

    def fit(self):
        _check(self._lib.hipdrt_plan_fit(self._h))

    def set_subbatches(self, k):
        """ranges the staged batch is fitted in, side by side inside one fit() call (hipdrt_plan_set_subbatches): 0 = the
        library chooses from the batch size (default; env HIPDRT_SUBBATCHES overrides at plan creation), 1 = one launch sequence"""
        _check(self._lib.hipdrt_plan_set_subbatches(self._h, int(k)))

    def llh_terms(self, stored=False, weights=None):
        """(rss, sum(log w)) per spectrum; stored=False: weights re-estimated from the current x (PFRT steps),
        stored=True: the `weights` argument of DRT.evaluate_rss() / evaluate_llh(): None = the fit's own est_weights,
        'uniform' = per-domain means of them (DRTMD's default), a positive scalar = that weight for every row."""
        rss, slw = np.empty(self.batch), np.empty(self.batch)
        if not stored:
            _check(self._lib.hipdrt_plan_llh_terms(self._h, _p(rss), _p(slw)))
        elif weights is None:
            _check(self._lib.hipdrt_plan_obs_llh_terms(self._h, _p(rss), _p(slw)))
        elif isinstance(weights, str):
            if weights != 'uniform':
                raise ValueError(f"weights must be None, 'uniform' or a scalar, got {weights!r}")
            _check(self._lib.hipdrt_plan_obs_llh_terms_w(self._h, 2, 1.0, _p(rss), _p(slw)))
        else:
            _check(self._lib.hipdrt_plan_obs_llh_terms_w(self._h, 3, float(weights), _p(rss), _p(slw)))
        return rss, slw

    def lml_terms(self, x=None, rho=None, s_vectors=None, dop_rho=None, step=None, weights=None, hypers=None, want=None):
        """hipdrt_plan_lml_terms for the fitted batch: the eight terms of DRT.evaluate_lml per spectrum -> dict of logdet_p,
        logdet_prior, wy2, fit2, cross, slw, xox, l1x and status, each (B,).  State: x (B, n), rho (B, 3), s_vectors (B, 3, n) and,
        for a plan with a DOP block, dop_rho (B, 3) together; or step = a recorded step; or neither: the live fit.  weights (B, m):
        None = the fit's est_weights.  hypers: None = the plan's own, else a dict with l2_lambda_0, derivative_weights and, for a
        DOP plan, dop_l2_lambda_0, dop_derivative_weights.  want: the terms to form and download (None: all); status always comes."""
        B, n, m = self.B, self.n, self.m
        lib = self._lib
        b = Bound(LmlIn())
        i = b.c
        lib.hipdrt_default_lml_in(C.byref(i))
        i.step = -1 if step is None else int(step)
        if step is not None and i.step < 0:
            raise ValueError("step must be >= 0")
        b.array("x", x, (B, n)); b.array("rho", rho, (B, 3)); b.array("s", s_vectors, (B, 3, n)); b.array("dop_rho", dop_rho, (B, 3))
        b.array("weights", weights, (B, m))
        if hypers is not None:
            i.override_hypers = 1
            i.l2_lambda_0 = float(hypers["l2_lambda_0"])
            for k, v in enumerate(np.broadcast_to(np.asarray(hypers["derivative_weights"], dtype=float), (3,))):
                i.derivative_weights[k] = float(v)
            if hypers.get("dop_l2_lambda_0") is not None:
                i.dop_l2_lambda_0 = float(hypers["dop_l2_lambda_0"])
                for k, v in enumerate(np.broadcast_to(np.asarray(hypers["dop_derivative_weights"], dtype=float), (3,))):
                    i.dop_derivative_weights[k] = float(v)
        out = {k: np.full(B, 7e77) for k in LML_TERMS if want is None or k in want}
        out["status"] = np.full(B, -77, dtype=np.int32)
        u = LmlOut()
        for k in LML_TERMS:
            setattr(u, k, _p(out.get(k)))
        u.status = _pi(out["status"])
        _check(lib.hipdrt_plan_lml_terms(self._h, C.byref(i), C.byref(u)))
        return out

    def set_state(self, x=None, rho=None, s=None, weights=None, dop_rho=None):
        arrs = [None if a is None else _f64(a) for a in (x, rho, s, weights)]
        _check(self._lib.hipdrt_plan_set_state(self._h, *[None if a is None else _p(a) for a in arrs]))
        if dop_rho is not None:
            _check(self._lib.hipdrt_plan_set_state_dop(self._h, _p(_f64(dop_rho))))

    def continue_fit(self, opts, weight_factor=1.0, min_iter=2):
        _check(self._lib.hipdrt_plan_continue(self._h, C.byref(opts), float(weight_factor), int(min_iter)))

    def set_weight_factors(self, weight_factor=1.0, row_factors=None, late=False):
        """weight_factor / chrono- and EIS-row factors of _qphb_fit_core; row_factors (m,) or (capacity, m); late=True: the
        rows are a vector-valued weight_factor (applied from the second iteration on)"""
        rf = None if row_factors is None else _f64(row_factors)
        if rf is not None and rf.ndim == 2 and rf.shape[0] < self.capacity:     # the C side reads capacity rows
            rf = _f64(np.vstack([rf, np.ones((self.capacity - rf.shape[0], rf.shape[1]))]))
        _check(self._lib.hipdrt_plan_set_weight_factors(self._h, float(weight_factor), _p(rf),
                                                        int(rf is not None and rf.ndim == 2) | (2 if late else 0)))

    def kk_screen(self, opts: KkOpts | None = None, set_row_factors=False, z_hat=True, residuals=True):
        """hipdrt_plan_kk_screen: prediction at the fit frequencies, residuals in percent of |Z|, outlier mask and clean window
        of every spectrum of the fitted batch, on the device.  Returns dict(z_hat (B, nf) complex, residuals (B, nf) complex,
        std (B,), outlier_mask (B, nf) int32, f_lim (B, 2) = f_min, f_max, i_lim (B, 2), status (B,)); z_hat / residuals are
        left out on request.  set_row_factors: the next fit's row factors (outlier_weight on the rows of masked frequencies)
        are written on the device and the plan is left as set_weight_factors(1.0, rows, late=True) would leave it."""
        B, nf = self.B, self.nf
        out = _kk_outputs(B, nf)
        zr, zi = (np.empty((B, nf)), np.empty((B, nf))) if z_hat else (None, None)
        er, ei = (np.empty((B, nf)), np.empty((B, nf))) if residuals else (None, None)
        _check(self._lib.hipdrt_plan_kk_screen(self._h, C.byref(opts) if opts is not None else None, int(bool(set_row_factors)),
                                               _p(zr), _p(zi), _p(er), _p(ei), _p(out["std"]), _pi(out["outlier_mask"]),
                                               _p(out["f_lim"]), _pi(out["i_lim"]), _pi(out["status"])))
        if z_hat:
            out["z_hat"] = zr + 1j * zi
        if residuals:
            out["residuals"] = er + 1j * ei
        return out

    def set_tau_basis(self, ln_basis_tau, epsilon):
        """prepared plans: the tau basis the DRT block stands on (hipdrt_plan_set_tau_basis), needed by predict_drt"""
        ln_tau = _f64(ln_basis_tau)
        _check(self._lib.hipdrt_plan_set_tau_basis(self._h, _p(ln_tau), ln_tau.size, float(epsilon)))
        self._basis_nb = ln_tau.size

    def basis_size(self):
        """points of the tau basis the DRT block stands on (a prepared plan: what set_tau_basis gave)"""
        return getattr(self, '_basis_nb', None) or self.ntau

    def predict_drt(self, ln_tau_eval, order=0, sign=1, normalize=0, n_sigma=None):
        """hipdrt_plan_predict_drt for the fitted batch: mu (B, neval) = scale_b E x_b on the device; normalize 0 / 1 (by R_p) /
        2 (by absolute R_p); n_sigma = (s_lo, s_hi) adds the band.  Returns (mu, lo, hi, status) with lo = hi = None without
        n_sigma; status (B,): the fit's status, or PREDICT_NOT_PD."""
        ev = _f64(ln_tau_eval).ravel()
        B = self.B
        mu = np.empty((B, ev.size))
        lo, hi = (np.empty((B, ev.size)), np.empty((B, ev.size))) if n_sigma is not None else (None, None)
        s_lo, s_hi = (0.0, 0.0) if n_sigma is None else (float(n_sigma[0]), float(n_sigma[1]))
        status = np.empty(B, dtype=np.int32)
        _check(self._lib.hipdrt_plan_predict_drt(self._h, _p(ev), ev.size, int(order), int(sign), int(normalize), s_lo, s_hi,
                                                 _p(mu), _p(lo), _p(hi), _pi(status)))
        return mu, lo, hi, status

    def find_peaks(self, ln_tau_eval, opts: PeakOpts, row_scale=None, want=None):
        """hipdrt_plan_find_peaks for the fitted batch -> dict of dense (B, neval) rows peak_sign, keep, heights, prominences,
        probs, left_bases, right_bases (and peak_prob, curv_prob for method 2), count (B,), used_prominence (B,), status (B,).
        row_scale (B,): per-spectrum factor on the coefficient scale (prepared plans, normalize = 0).  want: the names to
        download (None: all); status always comes."""
        ev = _f64(ln_tau_eval).ravel()
        out = _peak_outputs(self.B, ev.size, opts.method, want)
        out["status"] = np.empty(self.B, dtype=np.int32)
        rs = None if row_scale is None else _f64(row_scale)
        if rs is not None and rs.shape != (self.B,):
            raise ValueError("row_scale must have shape (B,)")
        _check(self._lib.hipdrt_plan_find_peaks(self._h, _p(ev), ev.size, C.byref(opts), _p(rs), *_peak_out_args(out),
                                                _pi(out["status"])))
        return out

    def peak_trough_probs(self, ln_tau_eval, opts: PeakProbOpts, row_scale=None, ranges=None, want=None):
        """hipdrt_plan_peak_trough_probs for the fitted batch -> dict of mu (3, B, neval) = f, fx, fxx (only when `want` names
        it), pp, tp, prob (B, neval), sigma (3, B, neval) and, by opts.search, 1: the dense (B, neval) rows keep, heights, prominences, left_bases, right_bases and count (B,); 2:
        range_peaks (B, nranges) for ranges = (nranges, 2) index windows [lo, hi] of the grid; status (B,) always.  row_scale
        (B,): per-spectrum factor on the coefficient scale (prepared plans).  want: the names to download (None: all)."""
        ev = _f64(ln_tau_eval).ravel()
        lo, hi = _index_windows(ranges)
        nr = 0 if lo is None else lo.size
        out = _peak_prob_outputs(self.B, ev.size, opts.search, nr, want)
        if want is not None and "mu" in want:
            out["mu"] = np.full((3, self.B, ev.size), np.nan)
        out["status"] = np.empty(self.B, dtype=np.int32)
        rs = None if row_scale is None else _f64(row_scale)
        if rs is not None and rs.shape != (self.B,):
            raise ValueError("row_scale must have shape (B,)")
        _check(self._lib.hipdrt_plan_peak_trough_probs(self._h, _p(ev), ev.size, C.byref(opts), _p(rs), nr, _pi(lo), _pi(hi),
                                                       _p(out.get("mu")), *_peak_prob_out_args(out), _pi(out["status"])))
        return out

    def resolve_peaks(self, ln_tau_find, ln_tau_out=None, opts: PeakResolveOpts | None = None, find_opts: PeakOpts | None = None,
                      peak_indices=None, windows=None, row_scale=None, want=None):
        """hipdrt_plan_resolve_peaks for the fitted batch -> dict of the padded outputs count (B,), status (B,), peak_index,
        trough_index, eps_l, eps_r, r_peaks, r_coef (B, max_peaks), x_peaks (B, max_peaks, nb), peak_gammas (B, max_peaks,
        nout); absent slots hold -1 / NaN.  Peak source: peak_indices (B, max_peaks) -1 padded, or windows = (start, end), else
        find_peaks with find_opts.  want: the names to form and download (None: all)."""
        opts = opts if opts is not None else peak_resolve_opts()
        b = Bound(PeakResolveIn())
        i = b.c
        lt = b.array("ln_tau_find", np.ravel(ln_tau_find))
        lo = b.array("ln_tau_out", None if ln_tau_out is None else np.ravel(ln_tau_out))
        i.nfind, i.nout = lt.size, 0 if lo is None else lo.size
        if peak_indices is not None:
            i.source = PEAKS_FROM_INDICES
            b.array("peak_indices", peak_indices, (self.B, opts.max_peaks), np.int32)
        elif windows is not None:
            i.source = PEAKS_FROM_WINDOWS
            i.nwin = b.array("win_start", np.ravel(windows[0]), None, np.int32).size
            b.array("win_end", np.ravel(windows[1]), None, np.int32)
        else:
            i.source, i.peak_opts = PEAKS_FROM_FIND, C.pointer(b.hold(find_opts if find_opts is not None else peak_opts()))
        b.array("row_scale", row_scale, (self.B,))
        out = _resolve_outputs(self.B, opts.max_peaks, self.basis_size(), i.nout, want)
        u = _resolve_out_struct(out)
        _check(self._lib.hipdrt_plan_resolve_peaks(self._h, C.byref(i), C.byref(opts), C.byref(u)))
        return out

    def score_candidates(self, x=None, ncand=None, ln_tau_find=None, opts: PeakOpts | None = None, max_peaks=16, want=None):
        """hipdrt_plan_score_candidates for the fitted batch: x (C, B, n) scaled candidate vectors to upload, or None for every
        recorded step of the step store; ncand (B,) candidates per spectrum (None: all); ln_tau_find: the grid of the peak
        search (None: likelihood sums only) -> dict of rss, sum_log_w, count, status (C, B), peak_index, heights, prominences
        (C, B, max_peaks); absent slots hold -1 / NaN.  want: the names to form and download (None: all); status always comes."""
        B, n = self.B, self.n
        b = Bound(CandidatesIn())
        i = b.c
        if x is None:
            Cn = self.pfrt_steps()
            i.source, i.C = CANDIDATES_FROM_STEPS, 0
        else:
            xa = b.array("x", x)
            if xa.ndim != 3 or xa.shape[1:] != (B, n):
                raise ValueError("x must have shape (C, B, n)")
            Cn = xa.shape[0]
            i.source, i.C = CANDIDATES_FROM_HOST, Cn
        b.array("ncand", ncand, (B,), np.int32)
        lt = b.array("ln_tau_find", None if ln_tau_find is None else np.ravel(ln_tau_find))
        i.peak_opts = C.pointer(b.hold(opts if opts is not None else peak_opts()))
        i.nfind, i.max_peaks = 0 if lt is None else lt.size, int(max_peaks)
        mp = int(max_peaks) or 16
        shapes = dict(rss=(Cn, B), sum_log_w=(Cn, B), count=(Cn, B), peak_index=(Cn, B, mp), heights=(Cn, B, mp),
                      prominences=(Cn, B, mp), status=(Cn, B))
        out = {}
        for k, shape in shapes.items():
            if (want is not None and k not in want and k != "status") or (lt is None and k in CANDIDATE_OUTPUTS[2:6]):
                continue
            out[k] = np.full(shape, -77, dtype=np.int32) if k in ("count", "peak_index", "status") else np.full(shape, 7e77)
        u = CandidatesOut()
        for k in CANDIDATE_OUTPUTS:
            a = out.get(k)
            setattr(u, k, None if a is None else (_pi(a) if a.dtype == np.int32 else _p(a)))
        _check(self._lib.hipdrt_plan_score_candidates(self._h, C.byref(i), C.byref(u)))
        return out

    def integrate_drt(self, ln_tau_eval, windows, order=0, sign=1, normalize=0, row_scale=None):
        """hipdrt_plan_integrate_drt: the trapezoid of predict_drt's row over every window (start, end) -> ((B, nwin), status)"""
        ev = _f64(ln_tau_eval).ravel()
        ws, we = _i32(windows[0]).ravel(), _i32(windows[1]).ravel()
        rs = None if row_scale is None else _f64(row_scale)
        if rs is not None and rs.shape != (self.B,):
            raise ValueError("row_scale must have shape (B,)")
        out = np.empty((self.B, ws.size))
        status = np.empty(self.B, dtype=np.int32)
        _check(self._lib.hipdrt_plan_integrate_drt(self._h, _p(ev), ev.size, int(order), int(sign), int(normalize), _p(rs), _pi(ws),
                                                   _pi(we), ws.size, _p(out), _pi(status)))
        return out, status

    def predict_z(self, frequencies, include_drt=True, include_ohmic=True, include_inductance=True):
        """hipdrt_plan_predict_z: complex (B, nf) impedance of the fitted batch at any frequencies, and the status (B,)"""
        f = _f64(frequencies).ravel()
        B = self.B
        zr, zi = np.empty((B, f.size)), np.empty((B, f.size))
        status = np.empty(B, dtype=np.int32)
        mask = int(bool(include_drt)) | (int(bool(include_ohmic)) << 1) | (int(bool(include_inductance)) << 2)
        _check(self._lib.hipdrt_plan_predict_z(self._h, _p(f), f.size, mask, _p(zr), _p(zi), _pi(status)))
        return zr + 1j * zi, status

    def predict_resistances(self, absolute=False, r_p_only=False):
        """hipdrt_plan_predict_resistances: (r_p, r_inf, r_tot), each (B,); r_p_only (prepared plans): (r_p, None, None)"""
        B = self.B
        r_p = np.empty(B)
        r_inf, r_tot = (None, None) if r_p_only else (np.empty(B), np.empty(B))
        _check(self._lib.hipdrt_plan_predict_resistances(self._h, _p(r_p), _p(r_inf), _p(r_tot), int(bool(absolute))))
        return r_p, r_inf, r_tot

    def pfrt_begin(self, max_steps):
        """size and empty the PFRT step store (hipdrt_plan_pfrt_begin)"""
        _check(self._lib.hipdrt_plan_pfrt_begin(self._h, int(max_steps)))

    def pfrt_record(self):
        """append the state the last fit / warm restart left to the PFRT step store (hipdrt_plan_pfrt_record)"""
        _check(self._lib.hipdrt_plan_pfrt_record(self._h))

    def pfrt_restore_s(self, step, factor=1.0):
        """the live s vectors become factor times those step `step` recorded, on the device (hipdrt_plan_pfrt_restore_s)"""
        _check(self._lib.hipdrt_plan_pfrt_restore_s(self._h, int(step), float(factor)))

    def pfrt_steps(self):
        n = C.c_int()
        _check(self._lib.hipdrt_plan_pfrt_steps(self._h, C.byref(n)))
        return n.value

    def pfrt_step_state(self, step):
        """what step `step` recorded -> dict(x (B, n), rho (B, 3), s_vectors (B, 3, n), rss (B,), sum_log_w (B,), status (B,))"""
        B, n = self.B, self.n
        out = dict(x=np.empty((B, n)), rho=np.empty((B, 3)), s_vectors=np.empty((B, 3, n)), rss=np.empty(B), sum_log_w=np.empty(B),
                   status=np.empty(B, dtype=np.int32))
        _check(self._lib.hipdrt_plan_pfrt_get_step(self._h, int(step), _p(out["x"]), _p(out["rho"]), _p(out["s_vectors"]),
                                                   _p(out["rss"]), _p(out["sum_log_w"]), _pi(out["status"])))
        return out

    def step_p_matrix(self, step, b=0):
        """pfrt_result['step_p_mat'][step] of spectrum b (hipdrt_plan_get_step_p_matrix)"""
        out = np.empty((self.n, self.n))
        _check(self._lib.hipdrt_plan_get_step_p_matrix(self._h, int(step), int(b), _p(out)))
        return out

    def predict_pfrt(self, factors, ln_tau_pfrt, ln_tau_out=None, opts: PfrtOpts | None = None, want=None):
        """hipdrt_plan_predict_pfrt over the recorded steps -> dict(pfrt (B, nout), raw_pfrt (B, np), step_pfrt (S, B, np),
        post_prob (S, B), status (B,)); want: the names to form and download (None: all); status always comes"""
        fac, ltp = _f64(factors).ravel(), _f64(ln_tau_pfrt).ravel()
        lto = None if ln_tau_out is None else _f64(ln_tau_out).ravel()
        S, B, npf = fac.size, self.B, ltp.size
        if S != self.pfrt_steps():
            raise ValueError(f"factors has {S} entries, the plan has recorded {self.pfrt_steps()} PFRT steps")
        nout = npf if lto is None else lto.size
        opts = opts if opts is not None else pfrt_opts()
        shapes = dict(pfrt=(B, nout), raw_pfrt=(B, npf), step_pfrt=(S, B, npf), post_prob=(S, B))
        out = {k: np.full(shape, 7e77) for k, shape in shapes.items() if want is None or k in want}
        out["status"] = np.empty(B, dtype=np.int32)
        g = out.get
        _check(self._lib.hipdrt_plan_predict_pfrt(self._h, _p(fac), _p(ltp), npf, _p(lto), nout, C.byref(opts), _p(g("pfrt")),
                                                  _p(g("raw_pfrt")), _p(g("step_pfrt")), _p(g("post_prob")), _pi(out["status"])))
        return out

    def pfrt_select(self, factors, ln_tau_pfrt, opts: PfrtOpts | None = None, sel: PfrtSelectOpts | None = None, want=None,
                    ln_tau_out=None):
        """hipdrt_plan_pfrt_select over the recorded steps -> dict of the compact form (num_peaks, first, num_candidates (B,);
        ranked_index, step_index, magnitude, match_quality (B, max_peaks); unused slots -1 / NaN), raw_pfrt (B, np), step_pfrt
        (S, B, np), post_prob (S, B) and status (B,); want: the names to form and download (None: all of these); status always
        comes.  'pfrt' in want: also the finished PFRT (B, nout) of the same pass, as predict_pfrt gives it for opts, on
        ln_tau_out (None: the tau_pfrt grid)."""
        fac, ltp = _f64(factors).ravel(), _f64(ln_tau_pfrt).ravel()
        S = fac.size
        if S != self.pfrt_steps():
            raise ValueError(f"factors has {S} entries, the plan has recorded {self.pfrt_steps()} PFRT steps")
        opts = opts if opts is not None else pfrt_opts()
        sel = sel if sel is not None else pfrt_select_opts()
        lto = None
        if want is not None and "pfrt" in want:
            lto = ltp if ln_tau_out is None else _f64(ln_tau_out).ravel()
            sel.ln_tau_out, sel.neval_out = _p(lto), lto.size
        b, out = pfrt_select_bound(self.B, S, ltp.size, sel.max_peaks, want, nout=0 if lto is None else lto.size)
        out["status"] = np.empty(self.B, dtype=np.int32)
        _check(self._lib.hipdrt_plan_pfrt_select(self._h, _p(fac), _p(ltp), ltp.size, C.byref(opts), C.byref(sel), C.byref(b.c),
                                                 _pi(out["status"])))
        return out

    def set_init_h(self, h_init):
        h = None if h_init is None else _f64(h_init)
        _check(self._lib.hipdrt_plan_set_init_h(self._h, _p(h)))

    def record_history(self, b):
        _check(self._lib.hipdrt_plan_record_history(self._h, int(b)))

    def download(self, s_vectors=False, lean=False):
        """results of the staged spectra; ``lean``: only what a map records per observation (fit_x, R_inf, inductance, the
        coefficient scale, iteration counts, status) -- 4 kB instead of 29 kB per spectrum at 256 x 512"""
        B, n, m = self.B, self.n, self.m
        out = dict(fit_x=np.empty((B, self.ntau)), R_inf=np.empty(B), inductance=np.empty(B), coefficient_scale=np.empty(B),
                   outer_iters=np.empty(B, dtype=np.int32), qp_iters_total=np.empty(B, dtype=np.int32),
                   status=np.empty(B, dtype=np.int32))
        if not lean:
            out.update(x=np.empty((B, n)), weights=np.empty((B, m)), rho=np.empty((B, 3)), q_vector=np.empty((B, n)))
        sv = np.empty((B, 3, n)) if (s_vectors and not lean) else None
        opt = lambda key: _p(out[key]) if key in out else None          # noqa: E731 (NULL = not wanted, include/hipdrt.h)
        _check(self._lib.hipdrt_plan_download(self._h, opt("x"), _p(out["fit_x"]), _p(out["R_inf"]),
                                              _p(out["inductance"]), opt("weights"), _p(out["coefficient_scale"]),
                                              opt("rho"), _p(sv) if sv is not None else None, opt("q_vector"),
                                              _pi(out["outer_iters"]), _pi(out["qp_iters_total"]), _pi(out["status"])))
        if sv is not None:
            out["s_vectors"] = sv
        return out

    def p_matrix(self, b):
        out = np.empty((self.n, self.n))
        _check(self._lib.hipdrt_plan_get_p_matrix(self._h, int(b), _p(out)))
        return out

    def distribution_var(self, basis_eval, batch):
        """diag(B P^-1 B') cs^2 for every fitted spectrum; basis_eval (neval, ntau)."""
        basis_eval = _f64(basis_eval)
        out = np.empty((int(batch), basis_eval.shape[0]))
        status = np.empty(int(batch), dtype=np.int32)
        _check(self._lib.hipdrt_plan_distribution_var(self._h, _p(basis_eval), basis_eval.shape[0], _p(out), _pi(status)))
        return out, status

    def param_cov(self, b=0):
        """inv(P_b) cs_b^2 (n, n) of fitted spectrum b, and whether P_b was positive definite"""
        out = np.empty((self.n, self.n))
        status = C.c_int()
        _check(self._lib.hipdrt_plan_param_cov(self._h, int(b), _p(out), C.byref(status)))
        return out, status.value == 0

    def distribution_cov(self, basis_eval, b=0):
        """basis_eval inv(P_b)[DRT block] basis_eval' cs_b^2 (neval, neval) of fitted spectrum b"""
        basis_eval = _f64(basis_eval)
        out = np.empty((basis_eval.shape[0], basis_eval.shape[0]))
        status = C.c_int()
        _check(self._lib.hipdrt_plan_distribution_cov(self._h, int(b), _p(basis_eval), basis_eval.shape[0], _p(out),
                                                      C.byref(status)))
        return out, status.value == 0

    def param_var(self, batch):
        out = np.empty((int(batch), self.n))
        status = np.empty(int(batch), dtype=np.int32)
        _check(self._lib.hipdrt_plan_param_var(self._h, _p(out), _pi(status)))
        return out, status

    def history(self):
        cap = int(self.opts.max_iter)
        hx, hr, hw = np.empty((cap, self.n)), np.empty((cap, 3)), np.empty((cap, self.m))
        qi = np.empty(cap + 1, dtype=np.int32)
        rows = C.c_int()
        _check(self._lib.hipdrt_plan_get_history(self._h, _p(hx), _p(hr), _p(hw), _pi(qi), cap, C.byref(rows)))
        r = rows.value
        return dict(x=hx[:r], rho=hr[:r], weights=hw[:r], qp_iterations=qi[:r + 1])

    def timings(self):
        t = (C.c_float * 5)()
        l = (C.c_int * 5)()
        _check(self._lib.hipdrt_plan_timings(self._h, t, l))
        names = ("total", "gram", "qp", "hyper", "other")
        return {k: float(t[i]) for i, k in enumerate(names)}, {k: int(l[i]) for i, k in enumerate(names)}


class PreparedPlan(Plan):
    """hipdrt_plan_create_prepared: the device loop on caller-prepared matrices (any data type; optional x_dop block
    and vz_offset column).  `desc` is a PreparedDesc, penalty = [m0, m1, m2] (n, n), vmm (m, m), h / l1 (n,)."""

    def __init__(self, ctx: Context, desc: PreparedDesc, penalty, vmm, h, l1, vz_strength=None,
                 opts: FitOpts | None = None, capacity=1):
        self._lib = load_library()
        self.ctx = ctx
        self.desc = desc
        self.opts = opts if opts is not None else default_fit_opts()
        mk = [_f64(a) for a in penalty]
        vmm, h, l1 = _f64(vmm), _f64(h), _f64(l1)
        vzs = None if vz_strength is None else _f64(vz_strength)
        hnd = _vp()
        _check(self._lib.hipdrt_plan_create_prepared(ctx._h, C.byref(desc), _p(mk[0]), _p(mk[1]), _p(mk[2]), _p(vmm),
                                                     _p(h), _p(l1), _p(vzs), C.byref(self.opts), int(capacity),
                                                     C.byref(hnd)))
        self._h = hnd
        self.n, self.m, self.ns = desc.n, desc.m, desc.ns
        self.nf, self.ntau, self.ngrid = 0, desc.n - desc.ns, 0
        self.capacity = int(capacity)
        self.B = 0
        self.rm_batched = False

    def upload(self, rzm, rzv):
        """rzm (m, n) shared or (B, m, n) per measurement; rzv (B, m)"""
        rzm, rzv = _f64(rzm), _f64(rzv)
        if rzv.ndim == 1:
            rzv = rzv[None, :]
        batched = rzm.ndim == 3
        _check(self._lib.hipdrt_plan_upload_prepared(self._h, rzv.shape[0], int(batched), _p(rzm), _p(rzv)))
        self.batch = self.B = rzv.shape[0]
        self.rm_batched = batched

    def iterate(self, x_in=None, s_vectors=None, rho=None, dop_rho=None, weights=None, est_weights=None,
                xmx_norms=None, dop_xmx_norms=None):
        """hipdrt_plan_iterate: one qphb.iterate_qphb on every staged measurement; arrays are (B, ...) or None to keep
        what the device holds.  Returns dict(converged, qp_status, qp_iters, primal_objective), each (B,)."""
        B, n, m = self.batch, self.n, self.m
        st = Bound(IterateState())
        for name, arr, shape in (("x_in", x_in, (B, n)), ("s_vectors", s_vectors, (B, 3, n)), ("rho", rho, (B, 3)),
                                 ("dop_rho", dop_rho, (B, 3)), ("weights", weights, (B, m)), ("est_weights", est_weights, (B, m)),
                                 ("xmx_norms", xmx_norms, (B, 3)), ("dop_xmx_norms", dop_xmx_norms, (B, 3))):
            st.array(name, arr, shape)
        conv, status, iters = (np.empty(B, dtype=np.int32) for _ in range(3))
        pobj = np.empty(B)
        _check(self._lib.hipdrt_plan_iterate(self._h, C.byref(st.c), _pi(conv), _pi(status), _pi(iters), _p(pobj)))
        return dict(converged=conv.astype(bool), qp_status=status, qp_iters=iters, primal_objective=pobj)

    def set_predict_desc(self, idx_rinf, idx_induc, idx_cinv, inductance_scale, capacitance_scale, coefficient_scale,
                         dop_scale_vector=None, v_baseline_scale=None, response_signal_scale=None, scaled_response_offset=None):
        """hipdrt_plan_set_predict_desc: what the special columns mean and the post-fit scales of the fitted batch (per member:
        coefficient_scale, response_signal_scale, scaled_response_offset, each (B,); dop_scale_vector (dop_size,) shared or (B, dop_size))"""
        b = Bound(PredictDesc())
        d = b.c
        d.idx_rinf, d.idx_induc, d.idx_cinv = int(idx_rinf), int(idx_induc), int(idx_cinv)
        d.inductance_scale, d.capacitance_scale = float(inductance_scale), float(capacitance_scale)
        if dop_scale_vector is not None and np.ndim(dop_scale_vector) == 2:
            if np.shape(dop_scale_vector) != (self.batch, self.desc.dop_size):
                raise ValueError(f"dop_scale_vector: expected shape {(self.batch, self.desc.dop_size)} or {(self.desc.dop_size,)}")
            d.dop_scale_batched = 1
        for name, v, size in (("dop_scale_vector", dop_scale_vector, self.desc.dop_size * (self.batch if d.dop_scale_batched else 1)),
                              ("v_baseline_scale", v_baseline_scale, self.desc.vb_size), ("coefficient_scale", coefficient_scale, self.batch),
                              ("response_signal_scale", response_signal_scale, self.batch),
                              ("scaled_response_offset", scaled_response_offset, self.batch)):
            if v is not None and np.size(v) != size:
                raise ValueError(f"{name}: expected {size} values, got {np.size(v)}")
            b.array(name, v)
        _check(self._lib.hipdrt_plan_set_predict_desc(self._h, C.byref(d)))

    def predict_response(self, times, step_times, step_sizes, basis_tau=None, mode=MODE_TRAPZ, ny=1000, lookup=None,
                         basis_nu=None, nu_epsilon=0.0, inf_rv=None, cap_rv=None, vz_strength=None, vb_mat=None,
                         include_mask=INCLUDE_ALL):
        """hipdrt_plan_predict_response: (B, nt) voltage response of the fitted batch at any times, and the status (B,).
        step_sizes (S,) or (B, S); inf_rv / cap_rv (nt,) or (B, nt); lookup = (log_td, v) for MODE_INTERP; vb_mat (nt, vb_size)."""
        b = Bound(ResponseArgs())
        a, arr, B = b.c, b.array, self.batch
        t = arr('times', np.ravel(times))
        st = arr('step_times', np.ravel(step_times))
        a.nt, a.nsteps = t.size, st.size
        sz = arr('step_sizes', step_sizes, [(st.size,), (B, st.size)])
        a.sizes_batched = int(sz.ndim == 2)
        # (without set_tau_basis the library refuses before it reads the basis)
        arr('basis_tau', basis_tau, [(self._basis_nb,)] if getattr(self, '_basis_nb', None) else None)
        a.mode, a.ny = int(mode), int(ny)
        if lookup is not None:
            ltd, v = arr('log_td', lookup[0]), arr('v', lookup[1])
            a.ngrid = ltd.size
        arr('basis_nu', basis_nu, [(self.desc.dop_size,)])
        a.nu_epsilon = float(nu_epsilon)
        for name, v in (('inf_rv', inf_rv), ('cap_rv', cap_rv)):
            v = arr(name, v, [(t.size,), (B, t.size)])
            if v is not None:
                setattr(a, name[:3] + '_batched', int(v.ndim == 2))
        arr('vz_strength', vz_strength, [(t.size,)])
        arr('vb_mat', vb_mat, [(t.size, self.desc.vb_size)])
        a.include_mask = int(include_mask)
        out = np.empty((B, t.size))
        status = np.empty(B, dtype=np.int32)
        _check(self._lib.hipdrt_plan_predict_response(self._h, C.byref(a), _p(out), _pi(status)))
        return out, status

    def predict_z_model(self, frequencies, basis_tau=None, mode=MODE_TRAPZ, ny=1000, lookups=None, basis_nu=None, nu_epsilon=0.0,
                        vz_strength=None, include_mask=INCLUDE_ALL):
        """hipdrt_plan_predict_z_model: complex (B, nf) impedance of the fitted batch of a prepared plan at any frequencies, and
        the status (B,).  lookups = ((log_wt_re, z_re), (log_wt_im, z_im)) for MODE_INTERP; vz_strength (nf,) or None."""
        b = Bound(ZModelArgs())
        a, arr = b.c, b.array
        f = arr('freq', np.ravel(frequencies))
        a.nf = f.size
        arr('basis_tau', basis_tau, (self._basis_nb,) if getattr(self, '_basis_nb', None) else None)
        a.mode, a.ny = int(mode), int(ny)
        if lookups is not None:
            (lwr, zr), (lwi, zi) = lookups
            lwr = arr('log_wt_re', lwr)
            a.ngrid = lwr.size
            for name, v in (('z_re', zr), ('log_wt_im', lwi), ('z_im', zi)):
                arr(name, v, (lwr.size,))
        arr('basis_nu', basis_nu, (self.desc.dop_size,))
        a.nu_epsilon = float(nu_epsilon)
        arr('vz_strength', vz_strength, (f.size,))
        a.include_mask = int(include_mask)
        B = self.batch
        zr, zi = np.empty((B, f.size)), np.empty((B, f.size))
        status = np.empty(B, dtype=np.int32)
        _check(self._lib.hipdrt_plan_predict_z_model(self._h, C.byref(a), _p(zr), _p(zi), _pi(status)))
        return zr + 1j * zi, status

    def predict_dop(self, nu, basis_nu, nu_epsilon, normalize_by=None, nu_basis_area=1.0, include_ideal=True):
        """hipdrt_plan_predict_dop: (B, len(nu)) distribution of phasances of the fitted batch on the ascending grid nu, and the
        status (B,); normalize_by (len(nu),) divides it (get_dop_norm), None leaves it as it is"""
        nu, bn = _f64(nu).ravel(), _f64(basis_nu).ravel()
        if bn.size != self.desc.dop_size:
            raise ValueError(f"basis_nu: expected {self.desc.dop_size} points, got {bn.size}")
        nb = None if normalize_by is None else _f64(normalize_by).ravel()
        if nb is not None and nb.size != nu.size:
            raise ValueError("normalize_by must have one entry per point of nu")
        B = self.batch
        out = np.empty((B, nu.size))
        status = np.empty(B, dtype=np.int32)
        _check(self._lib.hipdrt_plan_predict_dop(self._h, _p(nu), nu.size, _p(bn), float(nu_epsilon), _p(nb), float(nu_basis_area),
                                                 int(bool(include_ideal)), _p(out), _pi(status)))
        return out, status

    def _dop_args(self, nu, basis_nu, nu_epsilon, order, normalize_by, nu_basis_area, include_ideal=True, n_sigma=None):
        """a Bound hipdrt_dop_args"""
        b = Bound(DopArgs())
        a, arr = b.c, b.array
        nu = arr('nu', np.ravel(nu))
        a.nn = nu.size
        arr('basis_nu', np.ravel(basis_nu), (self.desc.dop_size,))
        arr('normalize_by', None if normalize_by is None else np.ravel(normalize_by), (nu.size,))
        a.nu_epsilon, a.order, a.nu_basis_area, a.include_ideal = float(nu_epsilon), int(order), float(nu_basis_area), int(bool(include_ideal))
        if n_sigma is not None:
            a.s_lo, a.s_hi = float(n_sigma[0]), float(n_sigma[1])
        return b

    def dop_posterior(self, nu, basis_nu, nu_epsilon, order=0, normalize_by=None, nu_basis_area=1.0, include_ideal=True,
                      n_sigma=None, want_var=True):
        """hipdrt_plan_dop_posterior: (mu, lo, hi, var, status) of the distribution of phasances of the fitted batch on the
        ascending grid nu, each (B, len(nu)); n_sigma = (s_lo, s_hi) or None (lo, hi None); want_var False: var None.  Without
        a band and a variance nothing is factorised."""
        b = self._dop_args(nu, basis_nu, nu_epsilon, order, normalize_by, nu_basis_area, include_ideal, n_sigma)
        B, nn = self.batch, b.c.nn
        mu = np.empty((B, nn))
        lo, hi = (np.empty((B, nn)), np.empty((B, nn))) if n_sigma is not None else (None, None)
        var = np.empty((B, nn)) if want_var else None
        status = np.empty(B, dtype=np.int32)
        _check(self._lib.hipdrt_plan_dop_posterior(self._h, C.byref(b.c), _p(mu), _p(lo), _p(hi), _p(var), _pi(status)))
        return mu, lo, hi, var, status

    def dop_cov(self, member, nu, basis_nu, nu_epsilon, order=0, normalize_by=None, nu_basis_area=1.0):
        """hipdrt_plan_dop_cov: (cov (len(nu), len(nu)), status) of member `member`; cov is NaN when status < 0"""
        b = self._dop_args(nu, basis_nu, nu_epsilon, order, normalize_by, nu_basis_area)
        out = np.empty((b.c.nn, b.c.nn))
        status = C.c_int(0)
        _check(self._lib.hipdrt_plan_dop_cov(self._h, int(member), C.byref(b.c), _p(out), C.byref(status)))
        return out, int(status.value)

    def resolve_group(self, args):
        """hipdrt_plan_resolve_group: the coupled QPs of DRTMD.resolve_group over members of the fitted batch, assembled from the final
        P and q on the device and solved there.  args: mapping.resolve.resolve_args' description -> dict of x (one (nr, nc_k) array
        per batch), iterations (nb,), status (nb,).  tau_filter_sigma / special_filter_sigma > 0: NotImplementedError."""
        b, nc, off = resolve_bound(args, self.B)
        nb, nr = b.c.nb, b.c.nr
        x = np.full(off[-1], 7e77)
        iters, status = np.full(nb, -7, dtype=np.int32), np.full(nb, -7, dtype=np.int32)
        _check(self._lib.hipdrt_plan_resolve_group(self._h, C.byref(b.c), _p(x), _pi(iters), _pi(status)), {E_UNSUPPORTED: NotImplementedError})
        return dict(x=[x[off[k]:off[k + 1]].reshape(nr, nc[k]) for k in range(nb)], iterations=iters, status=status)

    def get(self, which):
        B = self.batch
        shapes = {"m0": (self.n, self.n), "m1": (self.n, self.n), "m2": (self.n, self.n), "vmm": (self.m, self.m),
                  "h": (self.n,), "est_weights": (B, self.m), "rv": (B, self.m), "xmx": (B, 3), "dop_rho": (B, 3),
                  "dop_xmx": (B, 3), "hist_dop_rho": (int(self.opts.max_iter), 3), "outlier_t": (B, self.m),
                  "weight_factors": (B, 2), "x": (B, self.n), "var_floor": (B,),
                  "rzm": (B, self.m, self.n) if self.rm_batched else (self.m, self.n)}
        out = np.empty(shapes[which])
        _check(self._lib.hipdrt_plan_get(self._h, which.encode(), _p(out), out.size))
        return out

    def history(self):
        h = super().history()
        if self.desc.dop_size > 0:
            h["dop_rho"] = self.get("hist_dop_rho")[:len(h["x"])]
        return h
