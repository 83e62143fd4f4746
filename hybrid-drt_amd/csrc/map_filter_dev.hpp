// The piece of map_filter.hip that other translation units run on device buffers.
#pragma once
#include "plan.hpp"

namespace hipdrt {

// masked_filter(nan_to_num(a), ~isnan(a), gaussian_filter, sigma=) (hybdrt/filters/_filters.py:149-175) on a device array
// a[R * C]: the fused pair f(a w) / f(w) per axis with the caller's half tables tabs[0 .. 1] (host memory; radius < 0 skips the
// axis).  `out` may not alias `a`.  Synchronises the stream before it returns.
int masked_gaussian_device(hipStream_t st, const double* a, int R, int C, const hipdrt_filter_table* tabs, double* out);

// scipy.ndimage.gaussian_filter(a, sigma, mode='reflect') (apply_filter, hybdrt/filters/_filters.py:506-518) on a device array
// a[R * C]: the plain correlation per axis, axis 0 first, with the same half tables (radius < 0 skips the axis; both skipped: a
// copy).  No mask: a NaN spreads over its window.  `out` may not alias `a`.  Synchronises the stream before it returns.
int plain_gaussian_device(hipStream_t st, const double* a, int R, int C, const hipdrt_filter_table* tabs, double* out);

}  // namespace hipdrt
