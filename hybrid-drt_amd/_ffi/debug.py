"""DebugHooks: the debug_* test hooks of include/hipdrt_debug.h and the profile readers, mixed into Context."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .abi import *            # noqa: F401,F403 (the constants and structures)
from .abi import _check, _dp, _f64, _i32, _p, _pi
from .args import Bound, pfrt_select_bound, resolve_bound
from .opts import (_index_windows, _kk_outputs, _peak_out_args, _peak_outputs, _peak_prob_out_args, _peak_prob_outputs,
                   _resolve_out_struct, _resolve_outputs, peak_opts, peak_prob_opts, peak_resolve_opts, pfrt_opts, pfrt_select_opts)


class DebugHooks:
    """what only tests/ and tools/ call on a Context; uses self._lib and self._h alone"""

    def debug_map_filter_stats(self):
        """tools: (kernel launches, full-array reads + writes, device ms) of this context's last map_filter"""
        st = (C.c_double * 3)()
        _check(self._lib.hipdrt_debug_map_filter_stats(self._h, st))
        return int(st[0]), int(st[1]), float(st[2])

    def debug_map_badness_ms(self):
        """tools: device ms of this context's last map_badness"""
        ms = C.c_double()
        _check(self._lib.hipdrt_debug_map_badness_ms(self._h, C.cast(C.byref(ms), _dp)))
        return float(ms.value)

    def debug_qp_group(self, members):
        """tests / diagnostics: force the workgroups per problem of this context's coneqp launches sized from now on
        (hipdrt_debug_qp_group, include/hipdrt_debug.h)"""
        _check(self._lib.hipdrt_debug_qp_group(self._h, int(members)))
        self._qp_group_override = int(members)          # (remembered for callers that switch it temporarily: mapping._one_kernel)

    def debug_qp_waves(self, waves):
        """tests / tools: 4 = this context's batch coneqp launches (n <= 528) use the fat four-wavefront kernel, 8 = the
        eight-wavefront one, -1 = the library's choice (hipdrt_debug_qp_waves, include/hipdrt_debug.h)"""
        _check(self._lib.hipdrt_debug_qp_waves(self._h, int(waves)))

    def debug_stream_pool(self):
        """tests: (streams, holders, running) of the library's own streams on this context's device
        (hipdrt_debug_stream_pool, include/hipdrt_debug.h)"""
        size = C.c_int(0)
        _check(self._lib.hipdrt_debug_stream_pool(self._h, 0, None, None, None, C.byref(size)))
        n = size.value
        st, ho, ru = (C.c_void_p * n)(), (C.c_int * n)(), (C.c_int * n)()
        _check(self._lib.hipdrt_debug_stream_pool(self._h, n, st, ho, ru, C.byref(size)))
        return [st[i] for i in range(n)], [ho[i] for i in range(n)], [ru[i] for i in range(n)]

    def debug_exact_zero_shortcuts(self, on):
        """tests: with on = False this context's fits visit the penalty matrices' exact zeros as well (same bits, slower)
        (hipdrt_debug_exact_zero_shortcuts, include/hipdrt_debug.h)"""
        _check(self._lib.hipdrt_debug_exact_zero_shortcuts(self._h, int(bool(on))))

    def debug_gram_l2(self, A, w, y=None, l1=None, l1_scalar=0.0, l2=None, mk=None, s=None, rho=None, dfac=(0.0, 0.0, 0.0),
                      ns=0, sym=False, toep=False, toep_maxd=-1, spec_zero=False, dop_start=0, dop_size=0, dop_rho=None,
                      dop_dfac=(0.0, 0.0, 0.0), active=None, n=None, P=None, Ppk=None, q=None):
        """tests: the fit loop's Gram / q launchers on host arrays (hipdrt_debug_gram_l2, include/hipdrt_debug.h).
        A [m][lda] (shared) or [B][m][lda], w [B][m], y [B][m] or None (no q); `n` = the number of unknowns when A's rows are
        padded (lda = A.shape[-1] > n).  Either l2 ([n][ldl2] or [B][n][ldl2]) or the hyper-parameter form mk (three [n][ldm]
        matrices) + s [B][3][n] (+ rho [B][3]); see GramL2 in csrc/common.hpp for the rest.  P [B][n][ldp], Ppk [B][nchp^2 * 256]
        and q [B][n] are float64 C-contiguous arrays the CALLER fills beforehand (poison): they are uploaded, the kernels
        run, and they are overwritten in place with what the device holds afterwards.  P=None runs the kernel form without the
        row-major copy.  Returns (P, Ppk, q)."""
        b = Bound(DebugGramArgs())
        a = b.c
        A, w = b.array("A", A), b.array("w", w)
        B, m = w.shape
        a.B, a.m, a.lda = B, m, A.shape[-1]
        a.n = n = A.shape[-1] if n is None else int(n)
        a.a_batched = int(A.ndim == 3)
        if A.shape[-2] != m or (A.ndim == 3 and A.shape[0] != B):
            raise ValueError("A does not match w")
        b.array("y", y, (B, m))
        b.array("l1", l1, (n,))
        a.l1_scalar = float(l1_scalar)
        if s is not None:
            if mk is None or len(mk) != 3 or l2 is not None:
                raise ValueError("hyper-parameter form: three penalty matrices and no explicit l2")
            mk = [_f64(v) for v in mk]
            a.ldm = mk[0].shape[-1]
            if any(v.shape != (n, a.ldm) for v in mk):
                raise ValueError("mk: three [n][ldm] matrices")
            for k in range(3):
                a.mk[k] = _p(b.hold(mk[k]))
            b.array("s", s, (B, 3, n))
            b.array("rho", rho, (B, 3))
            b.array("dop_rho", dop_rho, (B, 3))
        elif l2 is not None:
            l2 = _f64(l2)
            a.l2_batched, a.ldl2 = int(l2.ndim == 3), l2.shape[-1]
            b.array("l2", l2, (B, n, a.ldl2) if l2.ndim == 3 else (n, a.ldl2))
        for k in range(3):
            a.dfac[k], a.dop_dfac[k] = float(dfac[k]), float(dop_dfac[k])
        a.ns, a.sym, a.toep, a.toep_maxd, a.spec_zero = int(ns), int(bool(sym)), int(bool(toep)), int(toep_maxd), int(bool(spec_zero))
        a.dop_start, a.dop_size = int(dop_start), int(dop_size)
        b.array("active", active, (B,), np.int32)
        if P is not None:
            a.ldp = P.shape[-1]
            b.output("P", P, (B, n, a.ldp))
        nchp = (n + 31) // 32 * 2
        b.output("Ppk", Ppk, (B, nchp * nchp * 256))
        b.output("q", q, (B, n))
        _check(self._lib.hipdrt_debug_gram_l2(self._h, C.byref(a)))
        return P, Ppk, q

    def debug_hyper_form(self, n, m, ns, toeplitz=True, outlier=False):
        """tests: (form, lds_bytes) of the LDS layout launch_hyper picks -- 1: Toeplitz columns beside the two m-vectors, 2: inside
        the second one, 0: the general row-streaming form; raises when none fits (hipdrt_debug_hyper_form, include/hipdrt_debug.h)"""
        form, lds = C.c_int(-1), C.c_longlong(0)
        _check(self._lib.hipdrt_debug_hyper_form(self._h, int(n), int(m), int(ns), int(bool(toeplitz)), int(bool(outlier)),
                                                 C.byref(form), C.byref(lds)))
        return form.value, lds.value

    def debug_impedance_interp_form(self, B, nf, ntau, ngrid):
        """tests: (tpr, rpb, lds_bytes) of the general interp build's launch -- threads per row, rows per workgroup, dynamic LDS;
        raises for an ngrid the entry points refuse (hipdrt_debug_impedance_interp_form, include/hipdrt_debug.h)"""
        tpr, rpb, lds = C.c_int(-1), C.c_int(-1), C.c_longlong(0)
        _check(self._lib.hipdrt_debug_impedance_interp_form(self._h, int(B), int(nf), int(ntau), int(ngrid), C.byref(tpr),
                                                            C.byref(rpb), C.byref(lds)))
        return tpr.value, rpb.value, lds.value

    def debug_hyper_step(self, rm, vmm, mk, x, x_in, s, rho, xmx, rv, est_w, w, var_floor, coef_scale, opts: FitOpts, ns=0, n=None,
                         toeplitz=False, toep_reach=-1, qp_status=None, active=None, fit_status=None, outer_iters=None, n_active=0,
                         outlier_t=None, it=0, continue_mode=0, min_iter=1, basis_area=1.0, desc: PreparedDesc | None = None,
                         dop_rho=None, dop_xmx=None, vz_strength=None, vz_entry=None, products=0):
        """tests: one hyper-parameter step (launch_hyper as it is) on host arrays (hipdrt_debug_hyper_step, include/hipdrt_debug.h).
        rm [m][ldrm] (shared) or [B][m][ldrm], vmm [m][m], mk three [n][ldm]; `n` = the number of unknowns when the rows of rm are
        padded.  x [B][n] is the QP's result; the other per-spectrum arrays are the state BEFORE the step (poison where the step is
        to write without reading).  Nothing passed in is modified.  Returns a dict of the state AFTER the step: s, rho, xmx, dop_rho,
        dop_xmx, w, x_in, outlier_t, active, fit_status, outer_iters, n_active, rv, est_w, coef_scale, var_floor, rm_col."""
        b = Bound(DebugHyperArgs())
        a = b.c
        rm, vmm, x = b.array("rm", rm), b.array("vmm", vmm), b.array("x", x)
        B = x.shape[0]
        m = vmm.shape[0]
        a.B, a.m, a.ldrm = B, m, rm.shape[-1]
        a.n = n = x.shape[1] if n is None else int(n)
        a.ns, a.rm_batched = int(ns), int(rm.ndim == 3)
        if rm.shape[-2] != m or (rm.ndim == 3 and rm.shape[0] != B) or vmm.shape != (m, m) or x.shape != (B, n):
            raise ValueError("rm, vmm and x do not match")
        mk = [_f64(v) for v in mk]
        if len(mk) != 3 or any(v.shape != (n, mk[0].shape[-1]) for v in mk):
            raise ValueError("mk: three [n][ldm] matrices")
        a.ldm = mk[0].shape[-1]
        for k in range(3):
            a.mk[k] = _p(b.hold(mk[k]))
        a.toeplitz, a.toep_reach = int(bool(toeplitz)), int(toep_reach)
        b.array("qp_status", np.zeros(B) if qp_status is None else qp_status, (B,), np.int32)
        a.opts = C.pointer(opts)
        a.it, a.continue_mode, a.min_iter, a.basis_area = int(it), int(continue_mode), int(min_iter), float(basis_area)
        a.products = int(products)
        # the state the step reads and writes: (field, value, shape[, dtype]); all but outlier_t are required
        states = [("x_in", x_in, (B, n)), ("s", s, (B, 3, n)), ("rho", rho, (B, 3)), ("xmx", xmx, (B, 3)), ("rv", rv, (B, m)),
                  ("est_w", est_w, (B, m)), ("w", w, (B, m)), ("var_floor", var_floor, (B,)), ("coef_scale", coef_scale, (B,)),
                  ("active", np.ones(B) if active is None else active, (B,), np.int32),
                  ("fit_status", np.full(B, -77) if fit_status is None else fit_status, (B,), np.int32),
                  ("outer_iters", np.full(B, -77) if outer_iters is None else outer_iters, (B,), np.int32),
                  ("n_active", [n_active], (1,), np.int32), ("outlier_t", outlier_t, (B, m))]
        if desc is not None:
            a.desc = C.pointer(desc)
            states += [("dop_rho", dop_rho, (B, 3)), ("dop_xmx", dop_xmx, (B, 3))]
            if desc.vz_index >= 0:
                b.array("vz_strength", _f64(vz_strength), (m,))
                rows = B if rm.ndim == 3 else 1
                states.append(("rm_col", np.full((rows, m), np.nan), (rows, m)))
        b.array("vz_entry", vz_entry, (B, m))
        out = {}
        for name, v, *shape_dtype in states:
            if v is not None:
                out[name] = b.array(name, v, *shape_dtype, copy=True)            # a copy: the caller's array stays as it is
            elif name != "outlier_t":
                raise ValueError(f"{name} is required")
        _check(self._lib.hipdrt_debug_hyper_step(self._h, C.byref(a)))
        out["n_active"] = int(out["n_active"][0])
        return out

    _SETUP_F64 = dict(rv="Bm", w="Bm", est_w="Bm", x="Bn", x_in="Bn", s="B3n", rho="B3", xmx="B3", dop_rho="B3", dop_xmx="B3",
                      coef_scale="B", var_floor="B", outlier_t="Bm", wrow="Bm", wfac="B2", rss="B", slw="B", w_out="Bm")
    _SETUP_I32 = ("active", "outer_iters", "fit_status", "qp_iters_total")

    def debug_setup(self, hook, B, m, n, opts: FitOpts, desc: PreparedDesc | None = None, nf=0, z_re=None, z_im=None, rm=None,
                    vmm=None, vmm_iw=None, qp_status=None, stage=0, r0=0, r1=0, row_mask=False, fixed_chrono=0.0, fixed_eis=0.0,
                    stored=0, scalar_w=1.0, **state):
        """tests: one of the setup hooks of include/hipdrt_debug.h -- hook = 'prep' | 'init_weights' | 'weight_method' | 'llh' -- on
        host arrays.  rm (m, ldrm) shared or (B, m, ldrm); vmm, vmm_iw (m, m).  `state`: the per-spectrum arrays by their names in
        hipdrt_debug_setup_args, as they are BEFORE the launch (poison where a kernel is to write without reading); they are copied,
        and the copies come back in a dict as the device holds them AFTER it.  Raises when a kernel wrote outside an array."""
        b = Bound(DebugSetupArgs())
        a = b.c
        a.B, a.nf, a.m, a.n = int(B), int(nf), int(m), int(n)
        a.opts = C.pointer(b.hold(opts))
        if desc is not None:
            a.desc = C.pointer(b.hold(desc))
        b.array("z_re", z_re, (B, nf)), b.array("z_im", z_im, (B, nf))
        rm = b.array("rm", rm, [(m, rm.shape[-1]), (B, m, rm.shape[-1])] if rm is not None else None)
        a.ldrm, a.rm_batched = (rm.shape[-1], int(rm.ndim == 3)) if rm is not None else (n, 0)
        b.array("vmm", vmm, (m, m)), b.array("vmm_iw", vmm_iw, (m, m))
        b.array("qp_status", qp_status, (B,), np.int32)
        a.stage, a.r0, a.r1, a.row_mask = int(stage), int(r0), int(r1), int(bool(row_mask))
        a.fixed_chrono, a.fixed_eis, a.stored, a.scalar_w = float(fixed_chrono), float(fixed_eis), int(stored), float(scalar_w)
        dims = dict(B=(B,), Bm=(B, m), Bn=(B, n), B3n=(B, 3, n), B3=(B, 3), B2=(B, 2))
        out = {}
        for name, v in state.items():
            if name in self._SETUP_I32:
                out[name] = b.array(name, v, (B,), np.int32, copy=True)
            elif name in self._SETUP_F64:
                out[name] = b.array(name, v, dims[self._SETUP_F64[name]], copy=True)
            else:
                raise ValueError(f"unknown state array {name}")
        _check(getattr(self._lib, "hipdrt_debug_" + hook)(self._h, C.byref(a)))
        return out

    def debug_rowop(self, op, out, in0=None, in1=None, in2=None, active=None, B=0, m=0, n=0, ns=0, nf=0, ld=0, col=0, idx_rinf=-1,
                    idx_induc=-1, nonneg=0, batched=False, factor=1.0, pen_r=0.0, pen_l=0.0):
        """tests: one element-wise launcher of csrc/hyper.hip on host arrays (hipdrt_debug_rowop, include/hipdrt_debug.h; `op` as
        numbered there).  out: one array, or the three matrices of op 2, as they are BEFORE the launch; copies come back as the device
        holds them AFTER it (one array, or a list of three).  Raises when a kernel wrote outside an array."""
        b = Bound(DebugRowopArgs())
        a = b.c
        a.op, a.B, a.m, a.n, a.ns, a.nf, a.ld, a.col = int(op), int(B), int(m), int(n), int(ns), int(nf), int(ld), int(col)
        a.idx_rinf, a.idx_induc, a.nonneg, a.batched = int(idx_rinf), int(idx_induc), int(nonneg), int(bool(batched))
        a.factor, a.pen_r, a.pen_l = float(factor), float(pen_r), float(pen_l)
        b.array("in0", in0), b.array("in1", in1), b.array("in2", in2), b.array("active", active, None, np.int32)
        outs = list(out) if isinstance(out, (list, tuple)) else [out]
        res = [b.array(f"out{k}", v, copy=True) for k, v in enumerate(outs)]
        _check(self._lib.hipdrt_debug_rowop(self._h, C.byref(a)))
        return res if isinstance(out, (list, tuple)) else res[0]

    def debug_kk_stats(self, freq, err, opts: KkOpts | None = None):
        """tests: the statistics stage of the KK screen kernel on host residuals err (B, nf) complex
        (hipdrt_debug_kk_stats, include/hipdrt_debug.h) -> dict(std, outlier_mask, f_lim, i_lim, status)"""
        freq = _f64(freq)
        err = np.atleast_2d(np.asarray(err, dtype=complex))
        if err.shape[1] != freq.size:
            raise ValueError("err must have shape (B, len(freq))")
        e_re, e_im = _f64(err.real), _f64(err.imag)
        out = _kk_outputs(err.shape[0], freq.size)
        _check(self._lib.hipdrt_debug_kk_stats(self._h, err.shape[0], freq.size, _p(freq), _p(e_re), _p(e_im),
                                               C.byref(opts) if opts is not None else None, _p(out["std"]),
                                               _pi(out["outlier_mask"]), _p(out["f_lim"]), _pi(out["i_lim"]),
                                               _pi(out["status"])))
        return out

    def debug_apply_rows(self, X, E, col_offset=0, scale=None):
        """tests: the row-application kernel of the predictions on host arrays (hipdrt_debug_apply_rows, include/hipdrt_debug.h):
        out[b, i] = scale[b] * sum_j E[i, j] X[b, col_offset + j]; X (B, ldx), E (r, K).  Raises when the kernel wrote outside
        its B x r block of the padded device output."""
        X, E = _f64(X), _f64(E)
        B, ldx = X.shape
        r, K = E.shape
        sc = None if scale is None else _f64(scale)
        if sc is not None and sc.shape != (B,):
            raise ValueError("scale must have shape (B,)")
        out = np.empty((B, r))
        _check(self._lib.hipdrt_debug_apply_rows(self._h, B, K, ldx, int(col_offset), _p(X), r, _p(E), _p(sc), _p(out)))
        return out

    def debug_response(self, X, ns, step_sizes, coefficient_scale, U=None, Ud=None, dop_start=0, copies=1, idx_rinf=-1,
                       idx_cinv=-1, vz_index=-1, vb_start=0, capacitance_scale=1.0, response_signal_scale=None,
                       scaled_response_offset=None, inf_rv=None, cap_rv=None, vz_strength=None, vb_mat=None,
                       v_baseline_scale=None, fit_status=None, include_mask=INCLUDE_ALL, nt=None, dop_scale_vector=None):
        """tests: the device chain of hipdrt_plan_predict_response behind its layer builders, on host arrays
        (hipdrt_debug_response, include/hipdrt_debug.h) -> (B, nt).  X (B, n); U (S, nt, ntau) unit-step layers; Ud (S, nt, dop_size)
        unit phasor layers, dop_scale_vector (B, dop_size) or None; step_sizes (S,) or (B, S); inf_rv / cap_rv (nt,) or (B, nt).  Raises when the kernel
        wrote outside its output."""
        b = Bound(DebugResponseArgs())
        a = b.c
        X = b.array('X', X)
        sz = b.array('step_sizes', step_sizes)
        U, Ud = b.array('U', U), b.array('Ud', Ud)
        a.B, a.n = X.shape
        a.S = sz.shape[-1]
        a.sizes_batched = int(sz.ndim == 2)
        layers = U if U is not None else Ud
        a.nt = int(nt) if layers is None else layers.shape[1]
        a.ntau = U.shape[2] if U is not None else 1
        a.copies, a.ns = int(copies), int(ns)
        a.dop_start, a.dop_size = int(dop_start), (Ud.shape[2] if Ud is not None else 0)
        b.array('dop_scale_vector', dop_scale_vector, (a.B, a.dop_size))
        for name, v in (('coefficient_scale', coefficient_scale), ('response_signal_scale', response_signal_scale),
                        ('scaled_response_offset', scaled_response_offset)):
            b.array(name, v, (a.B,))
        a.idx_rinf, a.idx_cinv, a.vz_index, a.vb_start = int(idx_rinf), int(idx_cinv), int(vz_index), int(vb_start)
        a.capacitance_scale = float(capacitance_scale)
        for name, v in (('inf_rv', inf_rv), ('cap_rv', cap_rv)):
            v = b.array(name, v, [(a.nt,), (a.B, a.nt)])
            if v is not None:
                setattr(a, name[:3] + '_batched', int(v.ndim == 2))
        b.array('vz_strength', vz_strength, (a.nt,))
        vb, vbs = b.array('vb_mat', vb_mat), b.array('v_baseline_scale', v_baseline_scale)
        a.vb_size = 0 if vb is None else vb.shape[1]
        if vb is not None and (vb.shape[0] != a.nt or vbs is None or vbs.shape != (a.vb_size,)):
            raise ValueError("vb_mat must have shape (nt, vb_size) and v_baseline_scale (vb_size,)")
        for name, v in (('U', U), ('Ud', Ud)):
            if v is not None and v.shape[:2] != (a.S, a.nt):
                raise ValueError(f"{name} must have shape (S, nt, columns)")
        b.array('fit_status', fit_status, (a.B,), np.int32)
        a.include_mask = int(include_mask)
        out = b.array('out', np.empty((a.B, a.nt)))
        _check(self._lib.hipdrt_debug_response(self._h, C.byref(a)))
        return out

    def debug_find_peaks(self, fxx, f=None, var_fxx=None, var_f=None, opts: PeakOpts | None = None):
        """tests: peaks_kernel on host rows (B, neval) (hipdrt_debug_find_peaks, include/hipdrt_debug.h) -> dict(peak_sign, keep,
        heights, prominences, probs, left_bases, right_bases, count, used_prominence[, peak_prob, curv_prob]).  Raises when the
        kernel wrote outside an output."""
        rows = [None if r is None else np.atleast_2d(_f64(r)) for r in (fxx, f, var_fxx, var_f)]
        B, n = rows[0].shape
        if any(r is not None and r.shape != (B, n) for r in rows):
            raise ValueError("all rows must have the shape of fxx")
        opts = opts if opts is not None else peak_opts()
        out = _peak_outputs(B, n, opts.method)
        _check(self._lib.hipdrt_debug_find_peaks(self._h, B, n, *[_p(r) for r in rows], C.byref(opts), *_peak_out_args(out)))
        return out

    def debug_peak_trough_probs(self, f=None, fx=None, fxx=None, var_f=None, var_fx=None, var_fxx=None, prob_in=None,
                                opts: PeakProbOpts | None = None, ranges=None, want=None):
        """tests: peak_trough_prob_kernel on host rows (B, neval) (hipdrt_debug_peak_trough_probs, include/hipdrt_debug.h) ->
        dict as Plan.peak_trough_probs without status.  prob_in: the search alone on that row (no pp, tp, sigma); ranges:
        (nranges, 2) index windows of search 2.  Raises when the kernel wrote outside an output."""
        rows = [None if r is None else np.atleast_2d(_f64(r)) for r in (f, fx, fxx, var_f, var_fx, var_fxx, prob_in)]
        first = next((r for r in rows if r is not None), None)
        if first is None:
            raise ValueError("the three mean rows, or prob_in")
        B, n = first.shape
        if any(r is not None and r.shape != (B, n) for r in rows):
            raise ValueError("all rows must have one shape")
        opts = opts if opts is not None else peak_prob_opts()
        lo, hi = _index_windows(ranges)
        nr = 0 if lo is None else lo.size
        out = _peak_prob_outputs(B, n, opts.search, nr, want, given_prob=prob_in is not None)
        _check(self._lib.hipdrt_debug_peak_trough_probs(self._h, B, n, *[_p(r) for r in rows], C.byref(opts), nr, _pi(lo), _pi(hi),
                                                        *_peak_prob_out_args(out)))
        return out

    def debug_peak_resolve(self, f, fxx, x, ln_tau_find, ln_basis, ln_tau_out=None, basis_eps=1.0, keep=None, indices=None,
                           windows=None, copies=1, fit_status=None, opts: PeakResolveOpts | None = None, want=None):
        """tests: peak_resolve_kernel on host arrays (hipdrt_debug_peak_resolve, include/hipdrt_debug.h): rows f, fxx (B, nfind),
        x (B, copies * nb) in data units, the peak source keep (B, nfind) / indices (B, max_peaks) / windows (start, end) ->
        dict of the padded outputs of hipdrt_plan_resolve_peaks plus lds_bytes.  Raises when the kernel wrote outside an output."""
        f, fxx, x = np.atleast_2d(_f64(f)), np.atleast_2d(_f64(fxx)), np.atleast_2d(_f64(x))
        lt, lb = _f64(ln_tau_find).ravel(), _f64(ln_basis).ravel()
        lo = None if ln_tau_out is None else _f64(ln_tau_out).ravel()
        B, nfind = f.shape
        nb, nout = lb.size, 0 if lo is None else lo.size
        if fxx.shape != f.shape or lt.size != nfind or x.shape != (B, copies * nb):
            raise ValueError("shapes: f, fxx (B, nfind); x (B, copies * nb)")
        opts = opts if opts is not None else peak_resolve_opts()
        b = Bound(DebugPeakResolveArgs())
        a = b.c
        a.B, a.nfind, a.nb, a.nout, a.copies, a.basis_eps = B, nfind, nb, nout, int(copies), float(basis_eps)
        for name, v in (("f", f), ("fxx", fxx), ("x", x), ("ln_tau_find", lt), ("ln_basis", lb), ("ln_tau_out", lo)):
            b.array(name, v)
        if keep is not None:
            a.source = PEAKS_FROM_FIND
            b.array("keep", np.atleast_2d(_i32(keep)), f.shape, np.int32)
        elif indices is not None:
            a.source = PEAKS_FROM_INDICES
            b.array("indices", np.atleast_2d(_i32(indices)), (B, opts.max_peaks), np.int32)
        else:
            a.source = PEAKS_FROM_WINDOWS
            a.nwin = b.array("win_start", np.ravel(windows[0]), None, np.int32).size
            b.array("win_end", np.ravel(windows[1]), None, np.int32)
        b.array("fit_status", fit_status, None, np.int32)
        a.opts = C.pointer(opts)
        out = _resolve_outputs(B, opts.max_peaks, nb, nout, want)
        a.out = _resolve_out_struct(out)
        lds = C.c_longlong(-1)
        a.lds_bytes = C.pointer(lds)
        try:
            _check(self._lib.hipdrt_debug_peak_resolve(self._h, C.byref(a)))
        finally:
            self.last_peak_resolve_lds = int(lds.value)
        out["lds_bytes"] = int(lds.value)
        return out

    def debug_pfrt_step(self, peak_sign, heights, prominences, f, var_f, var_fxx, var_floor=1e-5, ext_left=-1, ext_right=-1):
        """tests: pfrt_step_kernel on host rows (B, neval) (hipdrt_debug_pfrt_step, include/hipdrt_debug.h) -> (B, neval).  Raises
        when the kernel wrote outside its output."""
        sg = np.atleast_2d(_i32(peak_sign))
        rows = [np.atleast_2d(_f64(r)) for r in (heights, prominences, f, var_f, var_fxx)]
        B, n = sg.shape
        if any(r.shape != (B, n) for r in rows):
            raise ValueError("all rows must have the shape of peak_sign")
        out = np.full((B, n), 7e77)
        _check(self._lib.hipdrt_debug_pfrt_step(self._h, B, n, _pi(sg), *[_p(r) for r in rows], float(var_floor), int(ext_left),
                                                int(ext_right), _p(out)))
        return out

    def debug_pfrt_combine(self, step_pfrt, rss, sum_log_w, factors, m, ln_tau_pfrt, ln_tau_out=None, opts: PfrtOpts | None = None):
        """tests: pfrt_combine_kernel on host arrays (hipdrt_debug_pfrt_combine): step_pfrt (S, B, np), rss and sum_log_w (S, B),
        factors (S,) -> dict(pfrt (B, nout), raw_pfrt (B, np), post_prob (S, B)).  Raises when the kernel wrote outside an output."""
        sp, rss, slw, fac = _f64(step_pfrt), _f64(rss), _f64(sum_log_w), _f64(factors).ravel()
        S, B, npf = sp.shape
        if rss.shape != (S, B) or slw.shape != (S, B) or fac.size != S:
            raise ValueError("shapes: step_pfrt (S, B, np); rss, sum_log_w (S, B); factors (S,)")
        opts = opts if opts is not None else pfrt_opts()
        ltp = _f64(ln_tau_pfrt).ravel()
        lto = None if ln_tau_out is None else _f64(ln_tau_out).ravel()
        nout = npf if lto is None else lto.size
        if ltp.size != npf:
            raise ValueError("ln_tau_pfrt must have np points")
        out = dict(pfrt=np.full((B, nout), 7e77), raw_pfrt=np.full((B, npf), 7e77), post_prob=np.full((S, B), 7e77))
        _check(self._lib.hipdrt_debug_pfrt_combine(self._h, B, S, npf, nout, _p(sp), _p(rss), _p(slw), _p(fac), int(m), C.byref(opts),
                                                   _p(ltp), _p(lto), _p(out["pfrt"]), _p(out["raw_pfrt"]), _p(out["post_prob"])))
        return out

    def debug_pfrt_select(self, raw_pfrt, step_pfrt, rss, sum_log_w, m, sel: PfrtSelectOpts | None = None):
        """tests: pfrt_select_kernel on host arrays (hipdrt_debug_pfrt_select): raw_pfrt (B, np), step_pfrt (S, B, np), rss and
        sum_log_w (S, B) -> dict of the compact form (see Plan.pfrt_select) and status (B,).  Raises when the kernel wrote outside
        an output."""
        raw, sp, rss, slw = _f64(raw_pfrt), _f64(step_pfrt), _f64(rss), _f64(sum_log_w)
        if sp.ndim != 3 or raw.shape != sp.shape[1:] or rss.shape != sp.shape[:2] or slw.shape != sp.shape[:2]:
            raise ValueError("shapes: raw_pfrt (B, np); step_pfrt (S, B, np); rss, sum_log_w (S, B)")
        S, B, npf = sp.shape
        sel = sel if sel is not None else pfrt_select_opts()
        b, out = pfrt_select_bound(B, S, npf, sel.max_peaks, rows=False)
        out["status"] = np.full(B, -77, dtype=np.int32)
        _check(self._lib.hipdrt_debug_pfrt_select(self._h, B, S, npf, _p(raw), _p(sp), _p(rss), _p(slw), int(m), C.byref(sel),
                                                  C.byref(b.c), _pi(out["status"])))
        return out

    def debug_candidate_llh(self, x, rm, rv, vmm, var_floor):
        """tests: the likelihood kernels of csrc/candidates.hip on host arrays (hipdrt_debug_candidate_llh): x (C, B, n), rm (m, n)
        or (B, m, n), rv (B, m), vmm (m, m), var_floor (B,) -> (rss, sum_log_w), each (C, B).  Raises when a kernel wrote outside
        an output."""
        x, rm, rv, vmm, vf = _f64(x), _f64(rm), _f64(rv), _f64(vmm), _f64(var_floor).ravel()
        Cn, B, n = x.shape
        m = rv.shape[1]
        if rm.shape not in ((m, n), (B, m, n)) or rv.shape != (B, m) or vmm.shape != (m, m) or vf.shape != (B,):
            raise ValueError("shapes: x (C, B, n); rm (m, n) or (B, m, n); rv (B, m); vmm (m, m); var_floor (B,)")
        rss, slw = np.full((Cn, B), 7e77), np.full((Cn, B), 7e77)
        _check(self._lib.hipdrt_debug_candidate_llh(self._h, Cn, B, m, n, _p(rm), int(rm.ndim == 3), _p(rv), _p(vmm), _p(vf), _p(x),
                                                    _p(rss), _p(slw)))
        return rss, slw

    def debug_dop_posterior(self, P, rows, dop_start, dop_scale_vector, col_offset=None, B=None, scale=None, cov_member=-1, n=None,
                            dop_size=None, want=("var", "status")):
        """tests: the posterior chain behind the per-member congruence scaling of the packed P (hipdrt_debug_dop_posterior,
        include/hipdrt_debug.h).  Arguments and outputs as debug_posterior; dop_scale_vector (dop_size,) shared or (B, dop_size);
        col_offset=None places the rows at dop_start.  One more output may be named in `want`: ppk (nb, nchp * nchp * 256), the
        packed image of every member's P after the scaling."""
        P, rows = _f64(P), np.atleast_2d(_f64(rows))
        dsv = _f64(dop_scale_vector)
        batched = P.ndim == 3
        B = (P.shape[0] if batched else (dsv.shape[0] if dsv.ndim == 2 else 1)) if B is None else int(B)
        n = P.shape[-2] if n is None else int(n)
        nd = dsv.shape[-1] if dop_size is None else int(dop_size)
        if P.ndim not in (2, 3) or P.shape[-2] != n or (batched and P.shape[0] != B):
            raise ValueError("P: (n, ldp) or (B, n, ldp)")
        if dsv.ndim not in (1, 2) or (dsv.ndim == 2 and dsv.shape[0] != B) or dsv.shape[-1] != max(nd, 0):
            raise ValueError("dop_scale_vector: (dop_size,) or (B, dop_size)")
        neval, ncol = rows.shape
        sc = None if scale is None else _f64(scale).ravel()
        if sc is not None and sc.size != B:
            raise ValueError("scale: (B,)")
        nb = 1 if cov_member >= 0 else max(B, 0)
        nex, nchp = max((neval + 15) // 16, 0), (max(n, 0) + 31) // 32 * 2
        shapes = dict(var=(nb, neval), status=(nb,), cov=(neval, neval), bex=(nex, nchp, 256), tail=(nb, nex, nchp, 256),
                      ppk=(nb, nchp * nchp * 256))
        out = {k: (np.full(shapes[k], -7, dtype=np.int32) if k == "status" else np.full(shapes[k], 7e77)) for k in want}
        d = DebugDopPosteriorArgs()
        a = d.post
        a.B, a.n, a.P, a.p_batched, a.ldp = B, n, _p(P), int(batched), P.shape[-1]
        a.rows, a.neval, a.ncol, a.scale, a.cov_member = _p(rows), neval, ncol, _p(sc), int(cov_member)
        a.col_offset = int(dop_start if col_offset is None else col_offset)
        d.dop_start, d.dop_size, d.dop_scale_vector, d.dop_scale_batched = int(dop_start), nd, _p(dsv), int(dsv.ndim == 2)
        for k in want:
            setattr(d if k == "ppk" else a, k, _pi(out[k]) if k == "status" else _p(out[k]))
        _check(self._lib.hipdrt_debug_dop_posterior(self._h, C.byref(d)))
        return out

    def debug_posterior(self, P, rows, col_offset=0, B=None, scale=None, cov_member=-1, n=None, want=("var", "status")):
        """tests: the posterior variance and covariance chain on host arrays (hipdrt_debug_posterior, include/hipdrt_debug.h):
        P (n, ldp) shared by B spectra or (B, n, ldp), rows (neval, ncol) at unknowns col_offset.., scale (B,) or None ->
        dict of the outputs named in `want`: var (nb, neval), status (nb,), cov (neval, neval), bex (nex, nchp, 256),
        tail (nb, nex, nchp, 256); nb = B, or 1 with cov_member >= 0.  Raises when a kernel wrote outside an output or outside a
        spectrum's factor scratch."""
        P, rows = _f64(P), np.atleast_2d(_f64(rows))
        batched = P.ndim == 3
        B = (P.shape[0] if batched else 1) if B is None else int(B)
        n = P.shape[-2] if n is None else int(n)
        if P.ndim not in (2, 3) or P.shape[-2] != n or (batched and P.shape[0] != B):
            raise ValueError("P: (n, ldp) or (B, n, ldp)")
        neval, ncol = rows.shape
        sc = None if scale is None else _f64(scale).ravel()
        if sc is not None and sc.size != B:
            raise ValueError("scale: (B,)")
        nb = 1 if cov_member >= 0 else max(B, 0)
        nex, nchp = max((neval + 15) // 16, 0), (max(n, 0) + 31) // 32 * 2
        shapes = dict(var=(nb, neval), status=(nb,), cov=(neval, neval), bex=(nex, nchp, 256), tail=(nb, nex, nchp, 256))
        out = {k: (np.full(shapes[k], -7, dtype=np.int32) if k == "status" else np.full(shapes[k], 7e77)) for k in want}
        a = DebugPosteriorArgs()
        a.B, a.n, a.P, a.p_batched, a.ldp = B, n, _p(P), int(batched), P.shape[-1]
        a.rows, a.neval, a.ncol, a.col_offset, a.scale, a.cov_member = _p(rows), neval, ncol, int(col_offset), _p(sc), int(cov_member)
        for k in want:
            setattr(a, k, _pi(out[k]) if k == "status" else _p(out[k]))
        _check(self._lib.hipdrt_debug_posterior(self._h, C.byref(a)))
        return out

    def debug_qp(self, P, q, h, opts: QpOpts | None = None, active=None, order=None, use_lpt=False, x=None, iters=None, pcost=None,
                 status=None, iters_accum=None):
        """tests: launch_qp in the fit loop's form on host arrays (hipdrt_debug_qp, include/hipdrt_debug.h): P (n, ldp) shared or
        (B, n, ldp), q (B, n), h (n,) or (B, n).  x, iters, pcost, status, iters_accum are what the in/out arrays hold before the launch
        (sentinels by default; they are copied, not changed) -> dict with x, iterations, pcost, status, iters_accum, s, z (NaN rows
        for inactive problems), order (the table the kernel used), form (G, inverse blocks in global memory, wavefronts).  Raises when
        a kernel wrote outside an array, a problem's state block or factor scratch, or the sync words."""
        P, q, h = _f64(P), np.atleast_2d(_f64(q)), _f64(h)
        B, n = q.shape
        if P.ndim not in (2, 3) or P.shape[-2] != n or (P.ndim == 3 and P.shape[0] != B) or h.shape not in ((n,), (B, n)):
            raise ValueError("P: (n, ldp) or (B, n, ldp); q: (B, n); h: (n,) or (B, n)")

        def inout(v, shape, dtype, fill):
            out = np.full(shape, fill, dtype=dtype)
            if v is not None:
                out[...] = v
            return out
        out = dict(x=inout(x, (B, n), np.float64, 7e77), iterations=inout(iters, B, np.int32, -7), pcost=inout(pcost, B, np.float64, 7e77),
                   status=inout(status, B, np.int32, -7), iters_accum=inout(iters_accum, B, np.int32, 0),
                   s=np.full((B, n), np.nan), z=np.full((B, n), np.nan), order=np.full(B, -7, dtype=np.int32),
                   form=np.full(3, -7, dtype=np.int32))
        act = None if active is None else _i32(active).ravel()
        order_in = None if order is None else _i32(order).ravel()
        if (act is not None and act.size != B) or (order_in is not None and order_in.size != B):
            raise ValueError("active, order: (B,)")
        a = DebugQpArgs()
        a.B, a.n, a.P, a.p_batched, a.ldp, a.q, a.h, a.h_batched = B, n, _p(P), int(P.ndim == 3), P.shape[-1], _p(q), _p(h), int(h.ndim == 2)
        a.opts = C.pointer(opts) if opts is not None else None
        a.active, a.order, a.use_lpt, a.form = _pi(act), _pi(order_in), int(bool(use_lpt)), _pi(out["form"])
        a.x, a.iters, a.pcost, a.status, a.iters_accum = (_p(out["x"]), _pi(out["iterations"]), _p(out["pcost"]), _pi(out["status"]),
                                                          _pi(out["iters_accum"]))
        a.s, a.z, a.order_out = _p(out["s"]), _p(out["z"]), _pi(out["order"])
        _check(self._lib.hipdrt_debug_qp(self._h, C.byref(a)))
        return out

    def debug_lpt_order(self, iters, active=None):
        """tests: lpt_order_kernel alone (hipdrt_debug_lpt_order, include/hipdrt_debug.h) -> order (B,), -7 where the kernel wrote nothing"""
        iters = _i32(iters).ravel()
        act = None if active is None else _i32(active).ravel()
        order = np.full(iters.size, -7, dtype=np.int32)
        _check(self._lib.hipdrt_debug_lpt_order(self._h, iters.size, _pi(iters), _pi(act), _pi(order)))
        return order

    def debug_map_gaussian(self, a, tables, masked=False):
        """tests: plain_gaussian_device / masked_gaussian_device (csrc/map_filter.hip) on a 2-D host array
        (hipdrt_debug_map_gaussian, include/hipdrt_debug.h); tables: one full symmetric table per axis, None skips the axis;
        masked: the NaNs of `a` are the mask.  Entries no kernel wrote come back as -7e77."""
        a = _f64(a)
        if a.ndim != 2 or len(tables) != 2:
            raise ValueError("a 2-D array and one table (or None) per axis")
        tabs = Bound((FilterTable * 2)())
        for slot, full in zip(tabs.c, tables):
            tabs.table(slot, full)
        out = np.full(a.shape, -7.0e77)
        _check(self._lib.hipdrt_debug_map_gaussian(self._h, _p(a), a.shape[0], a.shape[1], tabs.c, int(bool(masked)), _p(out)))
        return out

    def debug_map_reduce(self, x, mode):
        """tests: the fixed-order reductions of csrc/map_filter.hip alone (hipdrt_debug_map_reduce) on a host vector ->
        mode 0: (mean, 0), 1: (np.std, the mean it was taken about), 2: (min, max)"""
        x = _f64(x).ravel()
        out = np.full(2, -7.0e77)
        _check(self._lib.hipdrt_debug_map_reduce(self._h, _p(x), x.size, int(mode), _p(out)))
        return float(out[0]), float(out[1])

    def debug_map_prob(self, f, fxx, f_var, fxx_var, ext=None, clamp_first=False, search=1, height=1e-3, prominence=5e-3,
                       sign_now=True, want=("pk", "curv", "f_var", "fxx_var")):
        """tests: clamp_kernel and / or map_prob_kernel (csrc/map_predict.hip) as stage 3 of hipdrt_map_predict launches them, on
        host rows (rows, n) (hipdrt_debug_map_prob, include/hipdrt_debug.h) -> dict of the rows in `want`; entries no kernel wrote
        come back as -7e77.  A grid beyond what LDS holds raises NotImplementedError, as Context.map_predict does."""
        names = ("pk", "curv", "f_var", "fxx_var")
        unknown = [w for w in want if w not in names]
        if unknown:
            raise ValueError(f"unknown outputs {unknown}")
        f_var, fxx_var = _f64(f_var), _f64(fxx_var)
        shape = f_var.shape
        f, fxx = (None if r is None else _f64(r) for r in (f, fxx))
        if len(shape) != 2 or any(r is not None and r.shape != shape for r in (f, fxx, fxx_var)):
            raise ValueError("f, fxx, f_var, fxx_var: 2-D arrays of one shape (rows, n)")
        if ext is not None:
            ext = np.ascontiguousarray(ext, dtype=np.int32)
            if ext.shape != (shape[0], 2):
                raise ValueError("ext: (rows, 2)")
        res = {w: np.full(shape, -7.0e77) for w in names if w in want}
        _check(self._lib.hipdrt_debug_map_prob(self._h, shape[0], shape[1], _p(f), _p(fxx), _p(f_var), _p(fxx_var), _pi(ext),
                                               int(bool(clamp_first)), int(search), float(height), float(prominence),
                                               int(bool(sign_now)), *[_p(res.get(w)) for w in names]), {E_UNSUPPORTED: NotImplementedError})
        return res

    def debug_candidate_form(self, form):
        """tests: how candidate scoring on this context keeps rm x between its two products: 0 LDS, 1 scratch, -1 automatic"""
        _check(self._lib.hipdrt_debug_candidate_form(self._h, int(form)))

    def debug_last_predict_ms(self):
        """tools: kernel time in ms of the last predict_drt / predict_z of a plan of this context -> (mean or impedance, with band)"""
        ms = (C.c_float * 2)()
        _check(self._lib.hipdrt_debug_last_predict_ms(self._h, ms))
        return float(ms[0]), float(ms[1])

    def debug_pack_p(self, P, n=None):
        """tests: launch_pack_p on row-major symmetric P [B][n][ldp] -> Ppk [B][nchp^2 * 256]; slots the kernel does not write
        come back as NaN (hipdrt_debug_pack_p, include/hipdrt_debug.h)"""
        P = _f64(P)
        B, rows, ldp = P.shape
        n = rows if n is None else int(n)
        if rows != n:
            raise ValueError("P: [B][n][ldp]")
        nchp = (n + 31) // 32 * 2
        Ppk = np.full((B, nchp * nchp * 256), np.nan)
        _check(self._lib.hipdrt_debug_pack_p(self._h, B, n, _p(P), ldp, _p(Ppk)))
        return Ppk

    def debug_logdet(self, P):
        """tests: the log-determinant kernel of Plan.lml_terms alone on symmetric matrices P (B, n, n) (hipdrt_debug_logdet,
        include/hipdrt_debug.h) -> (logdet (B,), status (B,)): 2 sum log L_ii, or NaN and -1 where P is not positive definite"""
        P = _f64(P)
        if P.ndim != 3 or P.shape[1] != P.shape[2]:
            raise ValueError("P: [B][n][n]")
        B, n = P.shape[:2]
        logdet, status = np.full(B, 7e77), np.full(B, -77, dtype=np.int32)
        _check(self._lib.hipdrt_debug_logdet(self._h, B, n, _p(P), _p(logdet), _pi(status)))
        return logdet, status

    def debug_resolve_assemble(self, args, p_list, q_list):
        """tests: the assembly kernels of Plan.resolve_group alone (hipdrt_debug_resolve_assemble, include/hipdrt_debug.h) on host
        arrays: args as mapping.resolve.resolve_args gives it (h is not read), member b's own P (n_b, n_b) and q (n_b,) -> one
        (P_k, q_k) per batch, P_k dense and symmetric from the lower tiles the kernel wrote.  Raises when a kernel wrote outside an
        array or left a padding entry of a tile non-zero."""
        if len(p_list) != len(q_list):
            raise ValueError("one q per P")
        b, nc, off = resolve_bound(args, len(p_list))
        nb, nr = b.c.nb, b.c.nr
        for m, (p, v, (left, right)) in enumerate(zip(p_list, q_list, np.asarray(args["tau_indices"]).reshape(-1, 2))):
            n = b.c.num_remove + b.c.so + int(right) - int(left)          # the hook reads this many rows, whatever it is handed
            if np.shape(p) != (n, n) or np.shape(v) != (n,):
                raise ValueError(f"member {m}: P ({n}, {n}) and q ({n},) for its tau range, got {np.shape(p)} and {np.shape(v)}")
        P = np.concatenate([_f64(p).ravel() for p in p_list])
        q = np.concatenate([_f64(v).ravel() for v in q_list])
        p_out = np.full(int(sum((nr * v) ** 2 for v in nc)), 7e77)
        q_out = np.full(off[-1], 7e77)
        _check(self._lib.hipdrt_debug_resolve_assemble(self._h, C.byref(b.c), len(p_list), _p(P), _p(q), _p(p_out), _p(q_out)),
               {E_UNSUPPORTED: NotImplementedError})
        poff = np.concatenate([[0], np.cumsum([(nr * v) ** 2 for v in nc])]).astype(int)
        return [(p_out[poff[k]:poff[k + 1]].reshape(nr * nc[k], nr * nc[k]), q_out[off[k]:off[k + 1]]) for k in range(nb)]

    def qp_profile(self, reset=True):
        buf = (C.c_ulonglong * 64)()        # 0..47 the QP kernel's phases, 48..63 hyper_kernel's (PROFILE=1 builds)
        _check(self._lib.hipdrt_qp_profile(self._h, buf, 64, int(reset)))
        return [int(v) for v in buf]

    def qp_timeline(self):
        """PROFILE builds: s_memtime stamps [wavefront 8][super column 16][stamp 8] of workgroup 0's last factorisation
        (csrc/qp_common.hpp, g_qp_tl); zeros otherwise"""
        n = 64 + 8 * 16 * 8
        buf = (C.c_ulonglong * n)()
        _check(self._lib.hipdrt_qp_profile(self._h, buf, n, 0))
        return np.array(buf[64:], dtype=np.uint64).reshape(8, 16, 8)

    def qp_timeline_mean(self, reset=True):
        """PROFILE builds: the same stamps as mean cycles since the start of the factorisation, over all factorisations of
        workgroup 0 since the last reset -> (array [8][16][8], number of factorisations)"""
        nt = 8 * 16 * 8
        n = 64 + 2 * nt + 1
        buf = (C.c_ulonglong * n)()
        _check(self._lib.hipdrt_qp_profile(self._h, buf, n, int(reset)))
        cnt = int(buf[64 + 2 * nt])
        return np.array(buf[64 + nt:64 + 2 * nt], dtype=np.float64).reshape(8, 16, 8) / max(cnt, 1), cnt
