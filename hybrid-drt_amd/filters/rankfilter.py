"""Device-backed rank filters (csrc/map_rank.hip, hipdrt_rank_filter) with scipy.ndimage's names and signatures: median_filter,
percentile_filter, and hybdrt/filters/_filters.py:43-46 iqr_filter, whose two percentiles come from one pass over the window.
2-D input and size= only; what is not built raises NotImplementedError naming the argument, and there is no numpy fall-back
(filters/ndfilters.py states the same filters in numpy to read the device against)."""
from .. import _ffi
from . import ndfilters


def _run(input, size, footprint, output, mode, origin, device, rank_lo, rank_hi=None):
    a, size = ndfilters._check_rank_args(input, size, footprint, output, mode, origin)
    n = size[0] * size[1]
    if n > ndfilters.RANK_MAX_WINDOW:
        raise NotImplementedError(f"size: windows of more than {ndfilters.RANK_MAX_WINDOW} entries are not built")
    return _ffi.get_context(device).rank_filter(a, size, rank_lo(n), None if rank_hi is None else rank_hi(n))


def median_filter(input, size=None, footprint=None, output=None, mode="reflect", cval=0.0, origin=0, device=0):
    return _run(input, size, footprint, output, mode, origin, device, lambda n: n // 2)


def percentile_filter(input, percentile, size=None, footprint=None, output=None, mode="reflect", cval=0.0, origin=0, device=0):
    return _run(input, size, footprint, output, mode, origin, device, lambda n: ndfilters.percentile_rank(n, percentile))


def iqr_filter(a, size, footprint=None, output=None, mode="reflect", cval=0.0, origin=0, device=0):
    return _run(a, size, footprint, output, mode, origin, device, lambda n: ndfilters.percentile_rank(n, 25),
                lambda n: ndfilters.percentile_rank(n, 75))
