"""Context: one hipdrt_ctx and the product's operators on it; the process-wide contexts."""
from __future__ import annotations

import ctypes as C

import numpy as np

from .abi import *            # noqa: F401,F403 (the constants and structures)
from .abi import HipDrtError, _check, _f64, _p, _pi, _vp, load_library
from .args import Bound
from .debug import DebugHooks
from .opts import default_fit_opts


class Context(DebugHooks):
    """One hipdrt_ctx (device + stream)."""

    def __init__(self, device: int = 0):
        self._lib = load_library()
        h = _vp()
        _check(self._lib.hipdrt_create(int(device), C.byref(h)))
        self._h = h
        self.device = int(device)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.hipdrt_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def stream(self):
        return self._lib.hipdrt_stream(self._h)

    def synchronize(self):
        _check(self._lib.hipdrt_synchronize(self._h))

    def plan_bytes_per_spectrum(self, nf, ntau, ns):
        """device bytes one staged spectrum costs an EIS plan of this shape (hipdrt_plan_bytes_per_spectrum)"""
        out = C.c_longlong(0)
        _check(self._lib.hipdrt_plan_bytes_per_spectrum(int(nf), int(ntau), int(ns), C.byref(out)))
        return out.value

    def device_info(self):
        buf = C.create_string_buffer(64)
        ncu = C.c_int()
        hbm = C.c_longlong()
        _check(self._lib.hipdrt_device_info(self._h, buf, 64, C.byref(ncu), C.byref(hbm)))
        return dict(arch=buf.value.decode(), num_cu=ncu.value, hbm_bytes=hbm.value)

    # ---- L1 ------------------------------------------------------------------------------------------
    def impedance_lookup(self, epsilon, wt_re, wt_im, ny=1000):
        wt_re, wt_im = _f64(wt_re), _f64(wt_im)
        z_re, z_im = np.empty_like(wt_re), np.empty_like(wt_im)
        _check(self._lib.hipdrt_impedance_lookup(self._h, float(epsilon), wt_re.size, int(ny), _p(wt_re), _p(wt_im),
                                                 _p(z_re), _p(z_im)))
        return z_re, z_im

    def impedance_matrix(self, freq, tau, epsilon, mode=MODE_INTERP, toeplitz=False, lookups=None, ny=1000, copies=None):
        """freq [nf] -> (nf, ntau) pair; freq [B][nf] (per-spectrum grids) -> (B, nf, ntau); copies = B with a shared freq [nf]:
        the B identical matrices a batch on one grid gets, (B, nf, ntau)"""
        freq, tau = _f64(freq), _f64(tau)
        batched = freq.ndim == 2
        if copies is not None and batched:
            raise ValueError("copies goes with one shared frequency grid")
        B = freq.shape[0] if batched else (1 if copies is None else int(copies))
        nf = freq.shape[-1]
        if lookups is not None:
            (lre, zre), (lim, zim) = lookups
            lre, zre, lim, zim = _f64(lre), _f64(zre), _f64(lim), _f64(zim)
            ng = lre.size
        else:
            lre = zre = lim = zim = None
            ng = 0
        a_re = np.empty((B, nf, tau.size))
        a_im = np.empty((B, nf, tau.size))
        _check(self._lib.hipdrt_impedance_matrix(self._h, B, int(batched), _p(freq), nf, _p(tau), tau.size, int(mode),
                                                 int(bool(toeplitz)), float(epsilon), ng, _p(lre), _p(zre), _p(lim),
                                                 _p(zim), int(ny), _p(a_re), _p(a_im)))
        if not batched and copies is None:
            return a_re[0], a_im[0]
        return a_re, a_im

    def impedance_matrix_timed(self, freq, tau, epsilon, dev_re, dev_im, mode=MODE_INTERP, toeplitz=False,
                               lookups=None, ny=1000, repeat=1):
        """Device-resident build (dev_re/dev_im: integer device pointers); returns elapsed ms of `repeat` launches."""
        freq, tau = _f64(freq), _f64(tau)
        batched = freq.ndim == 2
        B = freq.shape[0] if batched else 1
        nf = freq.shape[-1]
        (lre, zre), (lim, zim) = lookups if lookups is not None else ((None, None), (None, None))
        arrs = [None if a is None else _f64(a) for a in (lre, zre, lim, zim)]
        ng = 0 if arrs[0] is None else arrs[0].size
        ms = C.c_float()
        _check(self._lib.hipdrt_impedance_matrix_dev(self._h, B, int(batched), _p(freq), nf, _p(tau), tau.size,
                                                     int(mode), int(bool(toeplitz)), float(epsilon), ng, _p(arrs[0]),
                                                     _p(arrs[1]), _p(arrs[2]), _p(arrs[3]), int(ny), _vp(dev_re),
                                                     _vp(dev_im), int(repeat), C.byref(ms)))
        return ms.value

    def phasor_z_matrix(self, freq, nu, nu_epsilon):
        freq, nu = _f64(freq), _f64(nu)
        zr, zi = np.empty((freq.size, nu.size)), np.empty((freq.size, nu.size))
        _check(self._lib.hipdrt_phasor_z_matrix(self._h, _p(freq), freq.size, _p(nu), nu.size, float(nu_epsilon), _p(zr),
                                                _p(zi)))
        return zr + 1j * zi

    def phasor_v_matrix(self, times, nu, nu_epsilon, step_times, step_sizes):
        times, nu, st, sa = _f64(times), _f64(nu), _f64(step_times), _f64(step_sizes)
        rm = np.empty((times.size, nu.size))
        lay = np.empty((st.size, times.size, nu.size))
        _check(self._lib.hipdrt_phasor_v_matrix(self._h, _p(times), times.size, _p(nu), nu.size, float(nu_epsilon), _p(st),
                                                _p(sa), st.size, _p(rm), _p(lay)))
        return rm, lay

    def chrono_var_matrix(self, tt, seg, vmm_epsilon, uniform=False):
        tt = _f64(tt)
        seg = np.ascontiguousarray(seg, dtype=np.int32)
        out = np.empty((tt.size, tt.size))
        _check(self._lib.hipdrt_chrono_var_matrix(self._h, _p(tt), tt.size, _pi(seg), seg.size - 1, float(vmm_epsilon),
                                                  int(bool(uniform)), _p(out)))
        return out

    def response_lookup(self, epsilon, td, ny=1000):
        td = _f64(td)
        v = np.empty_like(td)
        _check(self._lib.hipdrt_response_lookup(self._h, float(epsilon), td.size, int(ny), _p(td), _p(v)))
        return v

    def response_matrix(self, times, tau, step_times, step_sizes, epsilon, mode=MODE_INTERP, lookup=None, ny=1000,
                        layered=True):
        times, tau, st, sa = _f64(times), _f64(tau), _f64(step_times), _f64(step_sizes)
        if st.size != sa.size:
            raise ValueError("step_times and step_sizes must have the same length")
        a = np.empty((times.size, tau.size))
        lay = np.empty((st.size, times.size, tau.size)) if layered else None
        if lookup is not None:
            log_td, v = _f64(lookup[0]), _f64(lookup[1])
            ng, plt, pv = log_td.size, _p(log_td), _p(v)
        else:
            ng, plt, pv = 0, None, None
        _check(self._lib.hipdrt_response_matrix(self._h, _p(times), times.size, _p(tau), tau.size, _p(st), _p(sa), st.size,
                                                int(mode), float(epsilon), ng, plt, pv, int(ny), _p(a),
                                                _p(lay) if layered else None))
        return a, lay

    def response_matrix_variant(self, times, tau, step_times, step_sizes, variant, tau_rise=None, epsilon=1.0, ny=1000,
                                layered=True):
        """the potentiostatic (RESPONSE_POT) and the expdecay-step (RESPONSE_EXPDECAY, trapz) forms of construct_response_matrix"""
        times, tau, st, sa = _f64(times), _f64(tau), _f64(step_times), _f64(step_sizes)
        if st.size != sa.size:
            raise ValueError("step_times and step_sizes must have the same length")
        tr = None
        if tau_rise is not None:
            tr = _f64(tau_rise)
            if tr.size != st.size:
                raise ValueError("tau_rise needs one entry per step")
        a = np.empty((times.size, tau.size))
        lay = np.empty((st.size, times.size, tau.size)) if layered else None
        _check(self._lib.hipdrt_response_matrix_variant(self._h, _p(times), times.size, _p(tau), tau.size, _p(st), _p(sa),
                                                        _p(tr) if tr is not None else None, st.size, int(variant), float(epsilon),
                                                        int(ny), _p(a), _p(lay) if layered else None))
        return a, lay

    def nonuniform_gaussian_filter1d(self, y, sigma, seg, filtered, nodes, node_delta, weights, woff, radius):
        """segment-wise blended Gaussian filter; see hipdrt.filters.nonuniform_gaussian_filter1d for the set-up"""
        y, sigma, nodes, node_delta, weights = _f64(y), _f64(sigma), _f64(nodes), _f64(node_delta), _f64(weights)
        seg, filtered, woff, radius = (np.ascontiguousarray(a, dtype=np.int32) for a in (seg, filtered, woff, radius))
        out = np.empty_like(y)
        _check(self._lib.hipdrt_nonuniform_gaussian_filter1d(self._h, _p(y), y.size, _p(sigma), _pi(seg), seg.size - 1,
                                                             _pi(filtered), _p(nodes), nodes.shape[1], _p(node_delta),
                                                             _p(weights), weights.size, _pi(woff), _pi(radius), _p(out)))
        return out

    def map_filter(self, a, args: MapFilterArgs, want_weights=False, want_sigmas=False):
        """hipdrt_map_filter on a 1-D or 2-D array (NaN = missing); `args` comes filled but for the shape (hipdrt.filters builds
        it).  Returns dict(out=, weights=, sigmas=) with the entries the call produces."""
        a = _f64(a)
        if a.ndim not in (1, 2):
            raise ValueError("a 1-D or 2-D array")
        args.ndim, args.rows, args.cols = a.ndim, a.shape[0], (a.shape[1] if a.ndim == 2 else 1)
        res = {}
        if args.op == MAP_FILTER:
            res["out"] = np.empty_like(a)
            if want_weights:
                res["weights"] = np.empty_like(a)
        if want_sigmas or args.op == MAP_SIGMAS:
            res["sigmas"] = np.empty((a.ndim,) + a.shape)
        _check(self._lib.hipdrt_map_filter(self._h, C.byref(args), _p(a), _p(res.get("out")), _p(res.get("weights")),
                                           _p(res.get("sigmas"))))
        return res

    def rank_filter(self, a, size, rank_lo, rank_hi=None):
        """hipdrt_rank_filter on a 2-D array: rank rank_lo of every size[0] x size[1] window, or (rank_hi given) the difference
        rank_hi - rank_lo of the same window.  A window of more than 49 entries raises NotImplementedError."""
        a = _f64(a)
        if a.ndim != 2:
            raise ValueError("a 2-D array")
        out = np.empty_like(a)
        _check(self._lib.hipdrt_rank_filter(self._h, _p(a), a.shape[0], a.shape[1], int(size[0]), int(size[1]),
                                            RANK_ONE if rank_hi is None else RANK_DIFF, int(rank_lo),
                                            int(rank_lo if rank_hi is None else rank_hi), _p(out)), {E_UNSUPPORTED: NotImplementedError})
        return out

    def percentiles(self, a, q, by_row=False):
        """hipdrt_percentiles: np.nanpercentile(a, q) over the whole array (out[nq]) or by row of a 2-D one (out[rows, nq]);
        an entry Q_NANMEDIAN of q asks for np.nanmedian"""
        a = _f64(a)
        q = _f64(np.atleast_1d(q))
        rows, cols = (a.shape if (by_row and a.ndim == 2) else (1, a.size))
        out = np.empty((rows, q.size) if by_row else q.size)
        _check(self._lib.hipdrt_percentiles(self._h, _p(a), rows, cols, int(bool(by_row)), _p(q), q.size, _p(out)))
        return out

    def map_badness(self, a, args: MapBadnessArgs, scale_src=None, want_flags=False, want_filt=False):
        """hipdrt_map_badness on a 2-D array; `args` comes filled but for the shape (hipdrt.mapping.nddata builds it).  Returns
        dict(rss=, flags=, filt=); ValueError when x_std contains NaNs, as the reference raises it."""
        a = _f64(a)
        if a.ndim != 2:
            raise ValueError("a 2-D array")
        args.rows, args.cols = a.shape
        if scale_src is not None:
            scale_src = _f64(scale_src)
            if scale_src.shape != a.shape:
                raise ValueError("scale_src must have the shape of a")
        res = {}
        if args.score:
            res["rss"] = np.empty(a.shape[0])
        if want_flags:
            res["flags"] = np.empty(a.shape, dtype=np.uint8)
        if want_filt:
            res["filt"] = np.empty_like(a)
        flags = res["flags"].ctypes.data_as(C.POINTER(C.c_ubyte)) if want_flags else None
        _check(self._lib.hipdrt_map_badness(self._h, C.byref(args), _p(a), _p(scale_src), _p(res.get("rss")), flags, _p(res.get("filt"))),
               {E_NUMERIC: ValueError})
        if want_flags:
            res["flags"] = res["flags"].astype(bool)
        return res

    def map_predict(self, x, ln_tau_sup, ln_tau_eval=None, epsilon=1.0, basis_area=1.0, normalize=False, filter_tables=None,
                    f_var=None, fxx_var=None, var_stored=False, ext=None, search=1, height=1e-3, prominence=5e-3, spread_table=None,
                    spread_factor=1.0, want=("x",)):
        """hipdrt_map_predict on the rows x (rows, nsup) of a map (hipdrt.mapping.predict states it in numpy).  filter_tables: None
        or one full symmetric table per axis (psi, tau; None skips the axis); f_var / fxx_var (rows, neval): the caller's variances,
        or with var_stored the raw stored ones, which take the clamp ext (rows, 2) and the filter; spread_table: the full tau table of
        peak_spread_sigma.  want: any of x, f, fxx, f_var, fxx_var, peak_prob, curv_prob -> dict.  An evaluation grid beyond what
        LDS holds raises NotImplementedError."""
        names = ("x", "f", "fxx", "f_var", "fxx_var", "peak_prob", "curv_prob")
        unknown = [w for w in want if w not in names]
        if unknown:
            raise ValueError(f"unknown outputs {unknown}")
        x = _f64(x)
        if x.ndim != 2:
            raise ValueError("x: a 2-D array (rows, nsup)")
        b = Bound(MapPredictArgs())
        a = b.c
        a.rows, a.nsup = x.shape
        lts = _f64(ln_tau_sup).ravel()
        if lts.size != x.shape[1]:
            raise ValueError("ln_tau_sup must have one entry per column of x")
        lte = _f64(ln_tau_eval).ravel() if ln_tau_eval is not None else lts
        a.neval, a.ln_tau_sup, a.ln_tau_eval = lte.size, _p(lts), _p(lte)
        a.epsilon, a.basis_area, a.normalize = float(epsilon), float(basis_area), int(bool(normalize))
        tabs = list(filter_tables) if filter_tables is not None else [None, None]
        if len(tabs) != 2:
            raise ValueError("filter_tables: one table per axis (psi, tau)")
        for slot, full in zip(a.x_filter, tabs):
            b.table(slot, full)
        b.table(a.spread, spread_table)
        a.spread_factor = float(spread_factor)
        shape = (x.shape[0], lte.size)
        if (f_var is None) != (fxx_var is None):
            raise ValueError("f_var and fxx_var: both or none")
        b.array("f_var", f_var, shape)
        b.array("fxx_var", fxx_var, shape)
        a.var_stored = int(f_var is not None and bool(var_stored))
        b.array("ext", ext, (x.shape[0], 2), np.int32)
        a.search, a.height, a.prominence = int(search), float(height), float(prominence)
        res = {w: np.empty(x.shape if w == "x" else shape) for w in names if w in want}
        _check(self._lib.hipdrt_map_predict(self._h, C.byref(a), _p(x), *[_p(res.get(w)) for w in names]), {E_UNSUPPORTED: NotImplementedError})
        return res

    def penalty_matrices(self, ln_tau, epsilon, toeplitz):
        ln_tau = _f64(ln_tau)
        n = ln_tau.size
        out = [np.empty((n, n)) for _ in range(3)]
        _check(self._lib.hipdrt_penalty_matrices(self._h, _p(ln_tau), n, float(epsilon), int(bool(toeplitz)),
                                                 _p(out[0]), _p(out[1]), _p(out[2])))
        return out

    def eis_var_matrix(self, freq, vmm_epsilon=0.25, reim_cor=0.25, uniform=False):
        freq = _f64(freq)
        vmm = np.empty((2 * freq.size, 2 * freq.size))
        _check(self._lib.hipdrt_eis_var_matrix(self._h, _p(freq), freq.size, float(vmm_epsilon), float(reim_cor),
                                               int(bool(uniform)), _p(vmm)))
        return vmm

    # ---- L2 ------------------------------------------------------------------------------------------
    def qp_batch(self, P, q, h, opts: QpOpts | None = None):
        P, q, h = _f64(P), _f64(q), _f64(h)
        if q.ndim == 1:
            q = q[None, :]
        B, n = q.shape
        p_batched = P.ndim == 3
        h_batched = h.ndim == 2
        x = np.empty((B, n))
        iters = np.empty(B, dtype=np.int32)
        pcost = np.empty(B)
        status = np.empty(B, dtype=np.int32)
        _check(self._lib.hipdrt_qp_batch(self._h, B, n, int(p_batched), _p(P), _p(q), int(h_batched), _p(h),
                                         C.byref(opts) if opts is not None else None, _p(x), _pi(iters), _p(pcost),
                                         _pi(status)))
        return dict(x=x, iterations=iters, pcost=pcost, status=status)

    def fit_eis_batch(self, freq, z, tau, epsilon, wt_re, wt_im, toeplitz_a=False, toeplitz_m=False, opts=None,
                      ny=1000):
        """the one-shot C entry point hipdrt_fit_eis_batch (interp mode): plan create, upload, fit, download, destroy"""
        freq, tau, wt_re, wt_im = _f64(freq), _f64(tau), _f64(wt_re), _f64(wt_im)
        z = np.atleast_2d(np.asarray(z))
        z_re, z_im = _f64(z.real), _f64(z.imag)
        lre, lim = np.log(wt_re), np.log(wt_im)
        opts = opts if opts is not None else default_fit_opts()
        B, nf, ntau = z.shape[0], freq.size, tau.size
        n = ntau + int(opts.fit_ohmic) + int(opts.fit_inductance)
        out = {"x": np.empty((B, n)), "fit_x": np.empty((B, ntau)), "R_inf": np.empty(B), "inductance": np.empty(B),
               "weights": np.empty((B, 2 * nf)), "coefficient_scale": np.empty(B), "rho": np.empty((B, 3)),
               "q_vector": np.empty((B, n)), "outer_iters": np.empty(B, dtype=np.int32),
               "status": np.empty(B, dtype=np.int32)}
        _check(self._lib.hipdrt_fit_eis_batch(self._h, B, _p(freq), nf, _p(z_re), _p(z_im), _p(tau), ntau, float(epsilon),
                                              MODE_INTERP, int(bool(toeplitz_a)), int(bool(toeplitz_m)), wt_re.size,
                                              int(ny), _p(wt_re), _p(wt_im), _p(lre), _p(lim), C.byref(opts),
                                              _p(out["x"]), _p(out["fit_x"]), _p(out["R_inf"]), _p(out["inductance"]),
                                              _p(out["weights"]), _p(out["coefficient_scale"]), _p(out["rho"]),
                                              _p(out["q_vector"]), _pi(out["outer_iters"]), _pi(out["status"])))
        return out

    def device_alloc(self, nbytes):
        """device memory as an integer pointer (hipdrt_device_alloc): for the *_dev entry points; free with device_free"""
        ptr = _vp()
        _check(self._lib.hipdrt_device_alloc(self._h, int(nbytes), C.byref(ptr)))
        return ptr.value

    def device_free(self, ptr):
        _check(self._lib.hipdrt_device_free(self._h, _vp(ptr)))

    def device_synchronize(self):
        """hipDeviceSynchronize on this context's device (every stream, every context of the process on that GPU)"""
        _check(self._lib.hipdrt_device_synchronize(self._h))

    def func_eval_matrix(self, basis_grid, eval_grid, epsilon, order=0):
        """hipdrt_func_eval_matrix: E[i, j] = phi^(order)(eval_i - basis_j; epsilon) of the gaussian basis, orders 0-2, on the
        device (natural-log grids) -> (len(eval_grid), len(basis_grid))"""
        basis_grid, eval_grid = _f64(basis_grid).ravel(), _f64(eval_grid).ravel()
        out = np.empty((eval_grid.size, basis_grid.size))
        _check(self._lib.hipdrt_func_eval_matrix(self._h, _p(basis_grid), basis_grid.size, _p(eval_grid), eval_grid.size,
                                                 float(epsilon), int(order), _p(out)))
        return out

    def weighted_gram(self, A, w, b, l2=None, l1=None):
        A, w, b = _f64(A), _f64(w), _f64(b)
        if w.ndim == 1:
            w, b = w[None, :], b[None, :]
        B, m = w.shape
        n = A.shape[1]
        l2a = None if l2 is None else _f64(l2)
        l1a = None if l1 is None else _f64(l1)
        P = np.empty((B, n, n))
        q = np.empty((B, n))
        _check(self._lib.hipdrt_weighted_gram(self._h, B, m, n, _p(A), _p(w), _p(b),
                                              int(l2a is not None and l2a.ndim == 3), _p(l2a), _p(l1a), _p(P), _p(q)))
        return P, q


_default_ctx = {}


def device_usable(device: int = 0) -> bool:
    """can this process open gfx950 device `device`? (no exception, and nothing is created on the device -- not even a stream:
    streams are dealt to the hardware queues in the order they are made; mapping.dist picks its default backend with this)"""
    try:
        lib = load_library()
    except HipDrtError:
        return False
    return lib.hipdrt_device_probe(int(device)) == 0


def get_context(device: int = 0) -> Context:
    """Process-wide context per device (created on first use)."""
    if device not in _default_ctx:
        _default_ctx[device] = Context(device)
    return _default_ctx[device]
