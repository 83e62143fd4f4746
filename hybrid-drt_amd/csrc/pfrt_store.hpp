// Layout of the PFRT step store of a plan (hipdrt_plan_pfrt_begin / _record, include/hipdrt.h): where step `step` of each buffer
// starts and how many elements each buffer holds.  Plain host arithmetic without a HIP type in it, so that the stand-alone host
// program tests/c/pfrt_store_host.cpp can drive it under a sanitizer with memcpy in place of the device copies.
#pragma once
#include <cstddef>

namespace hipdrt {

struct PfrtStoreLayout {
    size_t capacity, n;                                   // spectra the plan was made for, unknowns per spectrum
    size_t slot(int step) const { return (size_t)step * capacity; }
    // first element of step `step`: x [S][capacity][n], s [S][capacity][3][n], rho and dop_rho [S][capacity][3], and the per-spectrum
    // scalars rss, sum_log_w, status [S][capacity]
    size_t x(int step) const { return slot(step) * n; }
    size_t s(int step) const { return slot(step) * 3 * n; }
    size_t rho(int step) const { return slot(step) * 3; }
    size_t scalar(int step) const { return slot(step); }
    // elements of each buffer for max_steps steps
    size_t x_elems(int max_steps) const { return x(max_steps); }
    size_t s_elems(int max_steps) const { return s(max_steps); }
    size_t rho_elems(int max_steps) const { return rho(max_steps); }
    size_t scalar_elems(int max_steps) const { return scalar(max_steps); }
};

// bytes per spectrum of the capacity for `steps` steps: x, s, rho, dop_rho, rss and sum_log_w as doubles, the status as an int
inline long long pfrt_store_bytes_per_spectrum(int n, int steps) {
    return (long long)steps * ((4LL * n + 8) * (long long)sizeof(double) + (long long)sizeof(int));
}

}  // namespace hipdrt
