// Peak and trough probabilities of a fitted batch and the peak search on their product, one 256-thread workgroup per spectrum,
// rows in LDS:
//
//   DRT.predict_peak_trough_probs   hybdrt/models/drt1d.py:3655-3690
//   DRT.predict_peak_prob           drt1d.py:3692-3718: pp * (1 - tp)
//   DRT.find_peaks_byprob           drt1d.py:3720-3750
//   surface.peak_prob / trough_prob hybdrt/mapping/surface.py:265-350 (constrain_sign=False)
//   filters.std_filter              hybdrt/filters/_filters.py:29-40 over masked_filter (149-175), mask = ones
//   peaks.find_peaks_byrange        hybdrt/peaks.py:423-441
//
// With Phi(z) = erfc(-z / sqrt 2) / 2 (scipy.stats.norm.cdf) and sgn = np.sign:
//
//   fxx_prob = 1 - Phi(sgn(f) fxx / sxx)                                  surface.py:298
//   fx_prob  = Phi((5 sx - fx) / sx) - Phi((-5 sx - fx) / sx)             surface.py:301, 340
//   f_prob   = 1 - Phi((sf - |f|) / sf)                                   surface.py:304
//   pp = f_prob * fx_prob * fxx_prob                                      surface.py:306
//   tp = fx_prob * (1 - Phi(-sgn(f) fxx / sxx))                           surface.py:346-349
//   prob = pp * (1 - tp)                                                  drt1d.py:3718
//
// sigma, bayes_cov (drt1d.py:3670-3680): the root of e' inv(P) e cs^2 after extend_var's clamp (3123-3140), then for every order
// the floor np.median(s) - 1.5 * (np.percentile(s, 75) - np.percentile(s, 25)) from the sorted row (hyper_dev.hpp's bitonic
// network, padded with +inf): numpy's 'linear' percentile at the virtual index q (n - 1) with _lerp's two branches, the median
// as the mean of the two middle samples for even n.  sigma without bayes_cov (surface.py:272-291): the windowed standard
// deviation -- the mean over std_size samples with 'reflect' indices (period 2 n, any n >= 1), then the mean of the squared
// deviations from THAT row over the same window, negatives set to 0, the root -- plus std_baseline * np.std(row); the terms of a
// window are added in ascending offset, np.std's sums run per thread over i = tid, tid + 256, ... and then through blk_sum's fixed
// tree.  No reduction depends on anything but neval: a spectrum gives the same bits alone, in any batch and at any position.
//
// The search (search 1) is peaks_pass of peaks_dev.hpp on prob, a NaN threshold switching that condition off; search 2 gives
// np.argmax of the row with everything outside [lo, hi] set to zero, per window -- one wavefront per window, every lane keeping
// the first largest sample of its stride, the lanes merged by value and then by lower index.  Every decision compares staged LDS
// values.  Results are staged in LDS and written once, dense, by the loop at the end: that loop (i < neval, offset b * neval + i),
// the per-window loop (r < nranges) and the count are the only global stores.  Compiled with -ffp-contract=off.
//
// LDS rows of one spectrum (doubles): m0 m1 m2 the means f, fx, fxx -- once prob exists m0 holds the prominences, m1 pp, m2 tp;
// s0 s1 s2 the variances, then sigma in place; w[p2] the sort buffer (or the windowed mean), then prob.  ints: sgn, lb, rb.
#include <cmath>

#include "hyper_dev.hpp"
#include "peaks_dev.hpp"

namespace hipdrt {

static constexpr int PP_MAX_RANGES = 64;

__device__ __forceinline__ double pp_phi(double z) { return 0.5 * erfc(-z / PK_SQRT2); }
// scipy's 'reflect' (d c b a | a b c d | d c b a) for any distance
__device__ __forceinline__ int pp_reflect(int j, int n) {
    const int p = 2 * n;
    int m = j % p;
    if (m < 0) m += p;
    return m < n ? m : p - 1 - m;
}
// np.percentile(v, 100 q) of the ascending row v[n], method 'linear' (numpy's _lerp)
__device__ __forceinline__ double pp_quantile(const double* v, int n, double q) {
    const double vi = (double)(n - 1) * q;
    const int lo = (int)floor(vi);
    const int hi = lo + 1 < n ? lo + 1 : n - 1;
    const double t = vi - (double)lo, a = v[lo], c = v[hi], d = c - a;
    return t >= 0.5 ? c - d * (1.0 - t) : a + d * t;
}
// np.argmax's order: a NaN beats every number, then the larger value, then the lower index
__device__ __forceinline__ bool pp_before(double v, int i, double w, int j) {
    const bool vn = v != v, wn = w != w;
    if (vn != wn) return vn;
    if (!vn && v != w) return v > w;
    return i < j;
}

// grid = B
__global__ __launch_bounds__(PKT) void peak_trough_prob_kernel(PeakProbArgs a) {
    extern __shared__ double sm[];
    __shared__ double red[PKT / 64];
    __shared__ int rpk[PP_MAX_RANGES];
    const int b = blockIdx.x, tid = threadIdx.x, n = a.neval, p2 = a.p2;
    const bool bayes = a.o.bayes_cov != 0, have_prob = a.prob_in != nullptr;
    const PeakProbLds L = peak_prob_lds(sm, n, p2);
    double *m0 = L.m0, *m1 = L.m1, *m2 = L.m2, *s0 = L.s0, *w = L.w;
    int *sgn = L.sgn, *lb = L.lb, *rb = L.rb;
    const size_t row = (size_t)b * n, bn = (size_t)gridDim.x * n;

    const bool dead = (a.fit_status && a.fit_status[b] < 0) || (bayes && a.var_status && a.var_status[b] != 0);
    if (dead) {                                          // a failed fit, or sigma asked of a P that is not positive definite
        for (int i = tid; i < n; i += PKT) {
            const size_t o = row + i;
            if (a.pp) a.pp[o] = NAN;
            if (a.tp) a.tp[o] = NAN;
            if (a.prob) a.prob[o] = NAN;
            if (a.sigma) for (int k = 0; k < 3; ++k) a.sigma[k * bn + o] = NAN;
            if (a.keep) a.keep[o] = 0;
            if (a.heights) a.heights[o] = NAN;
            if (a.prominences) a.prominences[o] = NAN;
            if (a.left_bases) a.left_bases[o] = -1;
            if (a.right_bases) a.right_bases[o] = -1;
        }
        if (a.range_peaks) for (int r = tid; r < a.nranges; r += PKT) a.range_peaks[(size_t)b * a.nranges + r] = -1;
        if (tid == 0 && a.count) a.count[b] = 0;
        return;
    }

    if (have_prob) {
        for (int i = tid; i < n; i += PKT) w[i] = a.prob_in[row + i];
    } else {
        // ---- stage the rows; the variances scaled as peaks_kernel scales them ----
        const double* mu[3] = {a.f, a.fx, a.fxx};
        const double* var[3] = {a.var_f, a.var_fx, a.var_fxx};
        double c2 = 1.0;
        if (bayes && a.cs) c2 = a.cs[b] * a.cs[b];
        for (int i = tid; i < n; i += PKT)
            for (int k = 0; k < 3; ++k) {
                m0[k * n + i] = mu[k][row + i];
                if (bayes) s0[k * n + i] = var_scaled(var[k][(size_t)b * a.ldv + i], a.cs, c2, nullptr, 1.0);
            }
        __syncthreads();
        if (bayes) {
            // extend_var's clamp, then the root
            const int li = a.o.ext_left, ri = a.o.ext_right;
            for (int k = 0; k < 3; ++k) {
                double* v = s0 + k * n;
                const ExtClamp c = ext_clamp(li, ri, li >= 0 ? v[li] : 0.0, ri >= 0 ? v[ri] : 0.0);
                __syncthreads();
                for (int i = tid; i < n; i += PKT) v[i] = sqrt(c.apply(v[i], i));
                __syncthreads();
                if (!a.o.sigma_floor) continue;
                // the floor (drt1d.py:3676-3679) from the order statistics of the sorted row
                for (int i = tid; i < p2; i += PKT) w[i] = i < n ? v[i] : INFINITY;
                __syncthreads();
                lds_sort<PKT>(w, p2);
                const double med = (n & 1) ? w[n / 2] : (w[n / 2 - 1] + w[n / 2]) / 2.0;
                const double fl = med - 1.5 * (pp_quantile(w, n, 0.75) - pp_quantile(w, n, 0.25));
                for (int i = tid; i < n; i += PKT) if (v[i] < fl) v[i] = fl;
                __syncthreads();                         // (w is read above by every thread before the next order fills it)
            }
        } else {
            // std_filter(row, std_size, mask = ones) + std_baseline * np.std(row)  (surface.py:272-291; _filters.py:29-40)
            const int h = a.o.std_size / 2;
            const double size = (double)a.o.std_size;
            for (int k = 0; k < 3; ++k) {
                const double* r = m0 + k * n;
                double* s = s0 + k * n;
                double sum = 0.0;
                for (int i = tid; i < n; i += PKT) sum += r[i];
                sum = blk_sum<PKT>(sum, red);
                const double mean = sum / (double)n;
                double d = 0.0;
                for (int i = tid; i < n; i += PKT) { const double t = fabs(r[i] - mean); d += t * t; }
                d = blk_sum<PKT>(d, red);
                const double base = a.o.std_baseline * sqrt(d / (double)n);
                for (int i = tid; i < n; i += PKT) {
                    double t = 0.0;
                    for (int j = -h; j <= h; ++j) t += r[pp_reflect(i + j, n)];
                    w[i] = t / size;
                }
                __syncthreads();
                for (int i = tid; i < n; i += PKT) {
                    double t = 0.0;
                    for (int j = -h; j <= h; ++j) {
                        const int q = pp_reflect(i + j, n);
                        const double e = r[q] - w[q];
                        t += e * e;
                    }
                    t = t / size;
                    if (t < 0.0) t = 0.0;
                    s[i] = sqrt(t) + base;
                }
                __syncthreads();                         // (w is overwritten by the next row)
            }
        }
    }
    __syncthreads();

    // ---- the probabilities, elementwise; pp and tp take the place of fx and fxx ----
    if (!have_prob) {
        const double *sf = s0, *sx = s0 + n, *sxx = s0 + 2 * (size_t)n;
        for (int i = tid; i < n; i += PKT) {
            const double f = m0[i], fx = m1[i], fxx = m2[i], sg = np_sign(f);
            const double fxx_prob = 1.0 - pp_phi(sg * fxx / sxx[i]);
            const double fx_prob = pp_phi((5.0 * sx[i] - fx) / sx[i]) - pp_phi((-5.0 * sx[i] - fx) / sx[i]);
            const double f_prob = 1.0 - pp_phi((sf[i] - fabs(f)) / sf[i]);
            const double pp = f_prob * fx_prob * fxx_prob;
            const double tp = fx_prob * (1.0 - pp_phi(-sg * fxx / sxx[i]));
            m1[i] = pp; m2[i] = tp; w[i] = pp * (1.0 - tp);
        }
    }
    for (int i = tid; i < n; i += PKT) { m0[i] = 0.0; sgn[i] = 0; lb[i] = -1; rb[i] = -1; }
    __syncthreads();

    // ---- the search: scipy.signal.find_peaks on prob (drt1d.py:3744), or np.argmax of the masked row per window (peaks.py:423-441) ----
    const double* prob = w;
    double* prom = m0;
    if (a.o.search == 1) {
        const double height = a.o.height != a.o.height ? -INFINITY : a.o.height;
        const double prominence = a.o.prominence != a.o.prominence ? -INFINITY : a.o.prominence;
        peaks_pass(prob, nullptr, n, -1, false, height, prominence, sgn, prom, lb, rb);
    } else if (a.o.search == 2) {
        const int lane = tid & 63;
        for (int r = tid >> 6; r < a.nranges; r += PKT / 64) {
            const int lo = a.range_lo[r], hi = a.range_hi[r];
            // g = 0 outside [lo, hi]: its first sample stands for all of them
            const int out0 = lo > 0 ? 0 : (hi + 1 < n ? hi + 1 : -1);
            double bv = -INFINITY;
            int bi = n;
            for (int i = lo + lane; i <= hi; i += 64)
                if (pp_before(prob[i], i, bv, bi)) { bv = prob[i]; bi = i; }
            if (lane == 0 && out0 >= 0 && pp_before(0.0, out0, bv, bi)) { bv = 0.0; bi = out0; }
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) {
                const double ov = __shfl_xor(bv, off, 64);
                const int oi = __shfl_xor(bi, off, 64);
                if (pp_before(ov, oi, bv, bi)) { bv = ov; bi = oi; }
            }
            if (lane == 0) rpk[r] = bi;
        }
    }
    __syncthreads();

    // ---- the dense rows: the only global stores of the kernel besides the windows' peaks and the count ----
    double kept = 0.0;
    for (int i = tid; i < n; i += PKT) {
        const size_t o = row + i;
        const int kp = sgn[i] != 0 ? 1 : 0;
        kept += (double)kp;
        if (a.pp) a.pp[o] = m1[i];
        if (a.tp) a.tp[o] = m2[i];
        if (a.prob) a.prob[o] = prob[i];
        if (a.sigma) for (int k = 0; k < 3; ++k) a.sigma[k * bn + o] = s0[k * n + i];
        if (a.keep) a.keep[o] = kp;
        if (a.heights) a.heights[o] = kp ? prob[i] : 0.0;
        if (a.prominences) a.prominences[o] = prom[i];
        if (a.left_bases) a.left_bases[o] = lb[i];
        if (a.right_bases) a.right_bases[o] = rb[i];
    }
    if (a.range_peaks) for (int r = tid; r < a.nranges; r += PKT) a.range_peaks[(size_t)b * a.nranges + r] = rpk[r];
    kept = blk_sum<PKT>(kept, red);
    if (tid == 0 && a.count) a.count[b] = (int)kept;
}

size_t peak_prob_lds_bytes(int neval) { return peak_prob_lds(nullptr, neval, next_pow2(neval)).bytes; }

int peak_prob_check(const hipdrt_peak_prob_opts& o, int neval, int nranges, const int* range_lo, const int* range_hi) {
    HIPDRT_REQUIRE(neval >= 1, "neval >= 1");
    HIPDRT_REQUIRE(o.std_size >= 3 && (o.std_size & 1) == 1, "std_size must be odd and at least 3");
    HIPDRT_REQUIRE(std::isfinite(o.std_baseline) && o.std_baseline >= 0.0, "std_baseline must be finite and not negative");
    HIPDRT_REQUIRE(o.search >= 0 && o.search <= 2, "search must be 0 (rows only), 1 (height and prominence) or 2 (ranges)");
    HIPDRT_REQUIRE(!std::isinf(o.height) && !std::isinf(o.prominence), "height and prominence: finite, or NaN for none");
    HIPDRT_REQUIRE(o.ext_left >= -1 && o.ext_left < neval && o.ext_right >= -1 && o.ext_right < neval,
                   "ext_left and ext_right: an index of the evaluation grid, or -1");
    HIPDRT_REQUIRE(nranges >= 0 && nranges <= PP_MAX_RANGES, "0 <= nranges <= 64");
    HIPDRT_REQUIRE(o.search != 2 || (nranges >= 1 && range_lo && range_hi), "search 2 needs the ranges");
    if (o.search == 2)
        for (int r = 0; r < nranges; ++r)
            HIPDRT_REQUIRE(range_lo[r] >= 0 && range_hi[r] < neval && range_lo[r] <= range_hi[r] + 1,
                           "ranges: 0 <= lo, hi < neval, lo <= hi + 1 (lo = hi + 1: an empty window)");
    return lds_check(peak_prob_lds_bytes(neval), "peak_trough_probs", "neval");
}

int launch_peak_prob(hipStream_t s, PeakProbArgs a, int B) {
    HIPDRT_REQUIRE(B >= 1, "peak_trough_probs: B >= 1");
    HIPDRT_REQUIRE(a.prob_in || (a.f && a.fx && a.fxx), "peak_trough_probs: the three mean rows");
    HIPDRT_REQUIRE(a.prob_in || !a.o.bayes_cov || (a.var_f && a.var_fx && a.var_fxx), "peak_trough_probs: bayes_cov needs the three variance rows");
    HIPDRT_REQUIRE(!a.prob_in || !(a.pp || a.tp || a.sigma), "peak_trough_probs: a given prob row has no pp, tp or sigma");
    if (a.o.search != 2) a.nranges = 0;
    a.p2 = next_pow2(a.neval);
    const size_t lds = peak_prob_lds_bytes(a.neval);
    HIPDRT_REQUIRE(lds <= kLdsLimit, "peak_trough_probs: neval too large for one workgroup's LDS");
    if (int rc = set_lds(reinterpret_cast<const void*>(peak_trough_prob_kernel), lds, "peak_trough_prob_kernel")) return rc;
    hipLaunchKernelGGL(peak_trough_prob_kernel, dim3(B), dim3(PKT), lds, s, a);
    return 0;
}

}  // namespace hipdrt
