// The device pieces of the peak rule that more than one kernel file runs: peaks.hip (a fitted batch) and map_predict.hip (the rows of
// a map).  scipy.signal.find_peaks(v, height=, prominence=) restated as peaks.hip's head describes it; every decision is a comparison
// of staged values, so the result does not depend on which thread takes which plateau start.  Include from files compiled with
// -ffp-contract=off only: thresholds and probabilities round as written.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>

namespace hipdrt {

static constexpr int PKT = 256;
static constexpr double PK_SQRT2 = 1.4142135623730951;      // 2 ** 0.5

// numpy's sign, maximum and minimum (NaN goes through)
__device__ __forceinline__ double np_sign(double x) { return x > 0.0 ? 1.0 : (x < 0.0 ? -1.0 : (x == 0.0 ? 0.0 : x)); }
__device__ __forceinline__ double np_max(double a, double c) { return (a != a) ? a : ((c != c) ? c : (a > c ? a : c)); }
__device__ __forceinline__ double np_min(double a, double c) { return (a != a) ? a : ((c != c) ? c : (a < c ? a : c)); }
// 1 - Phi(0; mu, sigma)
__device__ __forceinline__ double upper_prob(double mu, double sigma) { return 1.0 - 0.5 * erfc(mu / (sigma * PK_SQRT2)); }

// one search pass on v = -s * fxx: peaks that pass height, the f test (two: s * f[p] > 0) and prominence are entered at their index
__device__ __forceinline__ void peaks_pass(const double* __restrict__ fxx, const double* __restrict__ f, int n, int s, bool two,
                                           double height, double prominence, int* __restrict__ sgn, double* __restrict__ prom,
                                           int* __restrict__ lb, int* __restrict__ rb) {
    auto V = [&](int i) { return s > 0 ? -fxx[i] : fxx[i]; };
    for (int i = 1 + (int)threadIdx.x; i < n - 1; i += PKT) {
        const double vi = V(i);
        if (!(V(i - 1) < vi)) continue;
        int e = i + 1;
        while (e < n - 1 && V(e) == vi) ++e;               // e <= n - 1
        if (!(V(e) < vi)) continue;
        const int p = (i + e - 1) / 2;
        if (!(vi >= height)) continue;
        if (two && !((s > 0 ? f[p] : -f[p]) > 0.0)) continue;
        double lmin = vi, rmin = vi;
        int lbi = p, rbi = p;
        for (int j = p; j >= 0; --j) {
            const double vj = V(j);
            if (!(vj <= vi)) break;
            if (vj < lmin) { lmin = vj; lbi = j; }
        }
        for (int j = p; j < n; ++j) {
            const double vj = V(j);
            if (!(vj <= vi)) break;
            if (vj < rmin) { rmin = vj; rbi = j; }
        }
        const double pr = vi - (lmin > rmin ? lmin : rmin);
        if (!(pr >= prominence)) continue;
        sgn[p] = s; prom[p] = pr; lb[p] = lbi; rb[p] = rbi;
    }
}

}  // namespace hipdrt
