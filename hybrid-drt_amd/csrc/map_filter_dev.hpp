// The piece of map_filter.hip that other translation units run on device buffers.
#pragma once
#include "plan.hpp"

namespace hipdrt {

// masked_filter(nan_to_num(a), ~isnan(a), gaussian_filter, sigma=) (hybdrt/filters/_filters.py:149-175) on a device array
// a[R * C]: the fused pair f(a w) / f(w) per axis with the caller's half tables tabs[0 .. 1] (host memory; radius < 0 skips the
// axis).  `out` may not alias `a`.  Synchronises the stream before it returns.
int masked_gaussian_device(hipStream_t st, const double* a, int R, int C, const hipdrt_filter_table* tabs, double* out);

}  // namespace hipdrt
