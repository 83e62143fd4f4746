"""Device-backed map filters (csrc/map_filter.hip, hipdrt_map_filter) with the reference's names and signatures
(hybdrt/filters/_filters.py: masked_filter 149-175, iterative_gaussian_filter 235-256, get_adaptive_sigmas 416-435,
adaptive_gaussian_filter 451-475).  The kernel tables -- Gaussian, empty Gaussian, order-2 Gaussian, box, and the node tables of
a sigma field -- are built here in numpy exactly as scipy / _scifilters.py build them (filters/ndfilters.py); the device gets
their centre and right half.  What the device path does not cover raises NotImplementedError naming the option; there is no
numpy fall-back (ndfilters is the statement to read the device against, not a second path)."""
import numpy as np

from .. import _ffi
from . import ndfilters

MIN_SIGMA = 0.25            # nonuniform_gaussian_filter1d's min_sigma: the adaptive chain never passes another


def _per_axis(value, ndim, what):
    if np.ndim(value) == 0:
        return [float(value)] * ndim
    value = [float(v) for v in value]
    if len(value) != ndim:
        raise RuntimeError(f"{what} must have one entry per axis")
    return value


def _refuse(kw, adaptive):
    """the keywords of scipy's gaussian_filter / the adaptive chain that the device path has one setting of"""
    kw = dict(kw)
    if kw.pop('mode', 'reflect') != 'reflect':
        raise NotImplementedError("mode: only the 'reflect' boundary is built")
    kw.pop('cval', None)
    if np.any(np.asarray(kw.pop('order', 0)) != 0):
        raise NotImplementedError("order: only order 0 is built")
    for name in ('curv_func', 'curv_kw', 'radius', 'output'):
        if kw.pop(name, None) is not None:
            raise NotImplementedError(f"{name} is not built on the device")
    truncate = float(kw.pop('truncate', 4.0))
    if adaptive and truncate != 4.0:
        raise NotImplementedError("truncate: the adaptive chain is built for truncate=4 (the reference smooths |curv| with scipy's default)")
    return kw, truncate


class _Args(_ffi.Bound):
    """hipdrt_map_filter_args with its defaults (every table skipped) and the numpy tables its pointers refer to"""

    def __init__(self, ndim):
        super().__init__(_ffi.MapFilterArgs())
        self.ndim = ndim
        self.error = None
        a = self.c
        for tabs in (a.gauss, a.empty_gauss, a.box, a.pre_gauss, a.pre_empty, [a.curv]):
            for t in tabs:
                self.table(t, None)
        a.iter, a.nstd, a.box_size = 2, 5.0, 5

    def gaussians(self, slots, empty_slots, sigma, truncate):
        for l, s in enumerate(sigma):
            if s > 1e-15:
                r = ndfilters.kernel_radius(s, truncate)
                self.table(slots[l], ndfilters.gaussian_kernel1d(s, 0, r))
                self.table(empty_slots[l], ndfilters.gaussian_kernel1d(s, 0, r, empty=True))

    def sigma(self, kw):
        kw, truncate = _refuse(kw, False)
        if 'sigma' not in kw:
            raise TypeError("the Gaussian filter needs sigma=")
        sigma = _per_axis(kw.pop('sigma'), self.ndim, 'sigma')
        if kw:
            raise TypeError(f"unexpected filter keywords {sorted(kw)}")
        self.gaussians(self.c.gauss, self.c.empty_gauss, sigma, truncate)

    def adaptive(self, kw, sigmas_in=None):
        """the keywords of get_adaptive_sigmas / adaptive_gaussian_filter"""
        kw, truncate = _refuse(kw, True)
        a = self.c
        a.adaptive = 1
        max_sigma = _per_axis(kw.pop('max_sigma', 1.0), self.ndim, 'max_sigma')
        k_factor = _per_axis(kw.pop('k_factor', 1.0), self.ndim, 'k_factor')
        presmooth = kw.pop('presmooth_sigma', None)
        presmooth = max_sigma if presmooth is None else _per_axis(presmooth, self.ndim, 'presmooth_sigma')
        node_factor = float(kw.pop('sigma_node_factor', 1.5))
        if kw:
            raise TypeError(f"unexpected filter keywords {sorted(kw)}")
        for l in range(self.ndim):
            a.max_sigma[l], a.k_factor[l] = max_sigma[l], k_factor[l]
        if sigmas_in is None:
            self.gaussians(a.pre_gauss, a.pre_empty, presmooth, truncate)
            r = ndfilters.kernel_radius(1, truncate)
            self.table(a.curv, ndfilters.gaussian_kernel1d(1, 2, r))
        else:
            self.array("sigmas_in", np.stack([np.broadcast_to(np.asarray(x, dtype=np.float64), sigmas_in[0].shape) for x in sigmas_in]))

        def node_tables(user, axis, empty, smin, smax, out):
            try:
                nodes, delta, floor, _ = ndfilters.sigma_nodes(smin, smax, node_factor, MIN_SIGMA)
                if len(nodes) > _ffi.MAP_FILTER_MAX_NODES:
                    raise ValueError(f"{len(nodes)} sigma nodes: more than {_ffi.MAP_FILTER_MAX_NODES}")
                t = out.contents
                t.count, t.node_delta, t.floor = len(nodes), float(delta), float(floor)
                for k, node in enumerate(nodes):
                    t.node[k] = float(node)
                    if node < MIN_SIGMA and not empty:
                        self.table((t, k), None)    # below the minimum effective width: the node returns its input
                        continue
                    s = MIN_SIGMA if node < MIN_SIGMA else float(node)
                    r = ndfilters.kernel_radius(s, truncate)
                    self.table((t, k), ndfilters.gaussian_kernel1d(s, 0, r, empty=bool(empty)))
                return 0
            except Exception as e:             # noqa: BLE001 (no exception may cross the C frames)
                self.error = e
                return 1

        self.callback = _ffi.NODE_TABLE_FN(node_tables)
        a.nodes = self.callback

    def iterative(self, iter, nstd, dev_rms_size):
        a = self.c
        if int(dev_rms_size) != dev_rms_size or dev_rms_size < 3 or dev_rms_size % 2 != 1:
            raise NotImplementedError("dev_rms_size: the device's box filter takes an odd size >= 3")
        a.iterative, a.iter, a.nstd, a.box_size = 1, int(iter), float(nstd), int(dev_rms_size)
        for l in range(self.ndim):
            self.table(a.box[l], np.ones(int(dev_rms_size)))

    def weights(self, w, shape):
        self.array("init_weights", np.broadcast_to(np.asarray(w, dtype=np.float64), shape))

    def run(self, a, device, **want):
        try:
            return _ffi.get_context(device).map_filter(a, self.c, **want)
        except _ffi.HipDrtError:
            if self.error is not None:
                raise self.error
            raise


def _array(a):
    a = np.asarray(a, dtype=np.float64)
    if a.ndim not in (1, 2):
        raise NotImplementedError("more than two dimensions: the device filters take 1-D and 2-D arrays")
    return a


def filter_array(a, iterative=True, adaptive=False, mask_nans=True, device=0, return_info=False, **filter_kw):
    """_filter_ndx_sub (hybdrt/mapping/ndx.py:302-349) with filter_func=None on an array with NaN for a missing entry: every
    entry of the result is filled.  return_info: also the final weights (iterative) and sigma fields (adaptive)."""
    a = _array(a)
    args = _Args(a.ndim)
    args.c.op, args.c.mask_nans = _ffi.MAP_FILTER, int(bool(mask_nans))
    if iterative:
        it = {k: filter_kw.pop(k) for k in ('iter', 'nstd', 'dev_rms_size') if k in filter_kw}
        args.iterative(it.get('iter', 2), it.get('nstd', 5), it.get('dev_rms_size', 5))
    if adaptive:
        args.adaptive(filter_kw)
    else:
        args.sigma(filter_kw)
    res = args.run(a, device, want_weights=bool(return_info and iterative), want_sigmas=bool(return_info and adaptive))
    return res if return_info else res["out"]


def masked_filter(a, mask, filter_func=None, device=0, **filter_kw):
    """_filters.masked_filter with the default filter_func (gaussian_filter): f(a mask) / f(mask) in one fused pass per axis"""
    if filter_func is not None:
        raise NotImplementedError("filter_func: the device's masked filter is the Gaussian one (filter_func=None)")
    a = _array(a)
    args = _Args(a.ndim)
    args.c.op = _ffi.MAP_FILTER
    args.sigma(filter_kw)
    args.weights(np.asarray(mask).astype(float), a.shape)
    return args.run(a, device)["out"]


def iterative_gaussian_filter(a, adaptive=False, iter=2, nstd=5, dev_rms_size=5, nan_mask=None, fill_nans=False, device=0,
                              **filter_kw):
    """_filters.iterative_gaussian_filter; entries under nan_mask must be zero-filled, as filter_ndx passes them"""
    a = _array(a)
    if nan_mask is not None:
        nan_mask = np.asarray(nan_mask, dtype=bool)
        if np.any(np.nan_to_num(a[nan_mask]) != 0):
            raise NotImplementedError("nan_mask: the device path takes zero-filled entries under the mask")
        a = np.where(nan_mask, np.nan, a)
    out = filter_array(a, True, adaptive, nan_mask is not None, device, iter=iter, nstd=nstd, dev_rms_size=dev_rms_size, **filter_kw)
    if nan_mask is not None and not fill_nans:
        out[nan_mask] = np.nan
    return out


def get_adaptive_sigmas(a, presmooth_sigma=None, empty=False, weights=None, curv_func=None, curv_kw=None, k_factor=1.0,
                        max_sigma=1.0, mode='reflect', cval=0.0, truncate=4.0, device=0):
    """_filters.get_adaptive_sigmas: the list of per-axis sigma fields"""
    a = _array(a)
    args = _Args(a.ndim)
    args.c.op, args.c.empty = _ffi.MAP_SIGMAS, int(bool(empty))
    args.adaptive(dict(presmooth_sigma=presmooth_sigma, curv_func=curv_func, curv_kw=curv_kw, k_factor=k_factor, max_sigma=max_sigma,
                       mode=mode, cval=cval, truncate=truncate))
    if weights is not None:
        args.weights(weights, a.shape)
    return list(args.run(a, device)["sigmas"])


def adaptive_gaussian_filter(a, sigmas=None, presmooth_sigma=None, empty=False, curv_func=None, curv_kw=None, k_factor=1,
                             max_sigma=5, mode='reflect', cval=0.0, truncate=4, order=0, sigma_node_factor=1.5, device=0):
    """_filters.adaptive_gaussian_filter with the sigma fields given (as every caller in the reference's filter chain gives them)"""
    if sigmas is None or any(s is None for s in sigmas):
        raise NotImplementedError("sigmas=None: compute the fields with get_adaptive_sigmas and pass them")
    a = _array(a)
    args = _Args(a.ndim)
    args.c.op, args.c.empty = _ffi.MAP_FILTER, int(bool(empty))
    args.adaptive(dict(presmooth_sigma=presmooth_sigma, curv_func=curv_func, curv_kw=curv_kw, k_factor=k_factor, max_sigma=max_sigma,
                       mode=mode, cval=cval, truncate=truncate, order=order, sigma_node_factor=sigma_node_factor),
                  sigmas_in=[np.broadcast_to(np.asarray(s, dtype=np.float64), a.shape) for s in sigmas])
    return args.run(a, device)["out"]
