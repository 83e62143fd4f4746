// The row arithmetic that more than one kernel file of the DRT chain runs (peaks.hip, peak_prob.hip, pfrt.hip, peak_resolve.hip,
// map_predict.hip): numpy's sign / maximum / minimum, the variance scaling, extend_var's clamp, the map probabilities and the peak
// rule.  scipy.signal.find_peaks(v, height=, prominence=) restated as peaks.hip's head describes it; every decision is a comparison
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

// e' inv(P) e as drt_band_kernel scales it: times cs^2, then over norm^2, each only where its vector is given
__device__ __forceinline__ double var_scaled(double v, const double* cs, double c2, const double* norm, double n2) {
    if (cs) v = v * c2;
    if (norm) v = v / n2;
    return v;
}

// extend_var's clamp (drt1d.py:3123-3140) from the row's values at the two bounds (0 where the index is -1): the left part first,
// so the right bound may already be a clamped value.  What follows it (a floor, the root) is the kernel's.
// (Not the map clamp, clamp_row of map_predict.hip: that leaves a row with a NaN alone and reads the right bound after the left side wrote.)
struct ExtClamp {
    int li, ri;
    double vl, vr;
    __device__ __forceinline__ double apply(double x, int i) const {
        if (li >= 0 && i < li) x = np_max(x, vl);
        if (ri >= 0 && i >= ri) x = np_max(x, vr);
        return x;
    }
};
__device__ __forceinline__ ExtClamp ext_clamp(int li, int ri, double vl, double vr) {
    if (li >= 0 && ri >= 0 && ri < li) vr = np_max(vr, vl);
    return {li, ri, vl, vr};
}

// the map probabilities of one sample (method 2 of peaks.hip, map_prob_kernel): curvature.peak_prob_1d's value at a found peak of
// prominence prom and height h (curvature.py:46-53), and DRTMD.predict_curv_prob (drtmd.py:1097-1104) with sf = sign(f)
__device__ __forceinline__ double map_peak_prob(double prom, double h, double f, double vxx, double vf) {
    return np_min(upper_prob(np_min(prom, h), sqrt(vxx)), upper_prob(fabs(f), sqrt(vf)));
}
__device__ __forceinline__ double map_curv_prob(double f, double fxx, double sf, double vf, double vxx) {
    double fp = upper_prob(-np_sign(fxx) * f, sqrt(vf));
    double cp = upper_prob(-sf * fxx, sqrt(vxx));
    fp = 2.0 * np_max(fp - 0.5, 0.0);
    cp = 2.0 * np_max(cp - 0.5, 0.0);
    return np_min(fp, cp) * sf;
}

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
