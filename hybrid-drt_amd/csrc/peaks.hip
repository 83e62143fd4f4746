// Peak finding on the curvature rows of a fitted batch, one 256-thread workgroup per spectrum, rows in LDS:
//
//   DRT.find_peaks                 hybdrt/models/drt1d.py:3753-3947 (method 'thresh' and 'prob', num_peaks)
//   curvature.peak_prob_1d         hybdrt/mapping/curvature.py:12-58, times sign(f) (hybdrt/mapping/drtmd.py:1064)
//   DRTMD.predict_curv_prob        drtmd.py:1097-1104, elementwise
//
// scipy.signal.find_peaks(v, height=, prominence=) is restated: a local maximum is the middle (i + a - 1) / 2 of a plateau
// [i, a) that rises at its left edge and falls at its right one, never the first or last sample; the prominence walks outwards
// from the peak while v <= v[p], keeps the FIRST lowest sample on each side (the one nearest the peak) as the base, and is
// v[p] - max(left minimum, right minimum).  hipdrt/models/peaks.py is the same arithmetic in numpy.
//
// Every plateau start is taken by one thread, which walks its plateau, applies the height (and, in a two-pass search, the f)
// test, walks out for the bases and applies the prominence test: all of it reads LDS only and every decision is a comparison of
// staged values, so the result does not depend on which thread takes which start.  The automatic threshold of 'thresh' is
// np.std: the mean, then the mean squared deviation, each summed per thread over i = tid, tid + 256, ... and then across the
// workgroup in one fixed tree -- the order depends on neval alone, never on B or on the spectrum's position.  Results go to
// LDS rows and are written once, dense, by the loop at the end of the kernel: that loop (i < neval, offset b * neval + i) and the
// two per-spectrum scalars are the only global stores.  Compiled with -ffp-contract=off: thresholds and probabilities round as
// written.
#include <cmath>

#include "hyper_dev.hpp"
#include "peaks_dev.hpp"

namespace hipdrt {

// grid = B
__global__ __launch_bounds__(PKT) void peaks_kernel(PeakArgs a) {
    extern __shared__ double sm[];
    __shared__ double red[PKT / 64];
    const int b = blockIdx.x, tid = threadIdx.x, n = a.neval, method = a.o.method;
    const PeaksLds l = peaks_lds(sm, n, a.p2, method, a.f != nullptr, a.o.num_peaks);
    double *fxx = l.fxx, *prom = l.prom, *f = l.frow, *vxx = l.vxx, *prob = l.prob, *vf = l.vf, *srt = l.srt;
    int *sgn = l.sgn, *lb = l.lb, *rb = l.rb;
    const size_t row = (size_t)b * n;

    const bool dead = (a.fit_status && a.fit_status[b] < 0) || (l.var && a.var_status && a.var_status[b] != 0);
    if (dead) {                                          // a failed fit, or sigma asked of a P that is not positive definite
        for (int i = tid; i < n; i += PKT) {
            const size_t o = row + i;
            if (a.peak_sign) a.peak_sign[o] = 0;
            if (a.keep) a.keep[o] = 0;
            if (a.heights) a.heights[o] = NAN;
            if (a.prominences) a.prominences[o] = NAN;
            if (a.probs) a.probs[o] = NAN;
            if (a.left_bases) a.left_bases[o] = -1;
            if (a.right_bases) a.right_bases[o] = -1;
            if (a.peak_prob) a.peak_prob[o] = NAN;
            if (a.curv_prob) a.curv_prob[o] = NAN;
        }
        if (tid == 0) {
            if (a.count) a.count[b] = 0;
            if (a.used_prominence) a.used_prominence[b] = NAN;
        }
        return;
    }

    // ---- stage the rows; the variances scaled as drt_band_kernel scales them ----
    double c2 = 1.0, n2 = 1.0;
    if (l.var) {
        if (a.cs) c2 = a.cs[b] * a.cs[b];
        if (a.norm) n2 = a.norm[b] * a.norm[b];
    }
    for (int i = tid; i < n; i += PKT) {
        fxx[i] = a.fxx[row + i];
        if (l.f) f[i] = a.f[row + i];
        if (l.var) vxx[i] = var_scaled(a.var_fxx[(size_t)b * a.ldv + i], a.cs, c2, a.norm, n2);
        if (l.varf) vf[i] = var_scaled(a.var_f[(size_t)b * a.ldv + i], a.cs, c2, a.norm, n2);
        prom[i] = 0.0; sgn[i] = 0; lb[i] = -1; rb[i] = -1;
        if (l.var) prob[i] = 0.0;
    }
    __syncthreads();
    // extend_var's clamp, then the floor (of the curvature's variance only)
    if (l.var) {
        const int li = a.o.ext_left, ri = a.o.ext_right;
        const double floor_v = a.o.fxx_var_floor;
        for (int k = 0; k < (l.varf ? 2 : 1); ++k) {
            double* v = k ? vf : vxx;
            const ExtClamp c = ext_clamp(li, ri, li >= 0 ? v[li] : 0.0, ri >= 0 ? v[ri] : 0.0);
            __syncthreads();
            for (int i = tid; i < n; i += PKT) {
                double x = c.apply(v[i], i);
                if (k == 0 && floor_v > 0.0 && x < floor_v) x = floor_v;
                v[i] = x;
            }
            __syncthreads();
        }
    }

    // ---- thresholds (drt1d.py:3846-3858) ----
    double prominence = a.o.prominence, height = a.o.height;
    if (height != height) height = method == 0 ? 0.0 : 1e-3;
    if (prominence != prominence) {
        if (method == 0) {
            double s = 0.0, c = 0.0;
            for (int i = tid; i < n; i += PKT) if (!isinf(fxx[i])) { s += fxx[i]; c += 1.0; }
            s = blk_sum<PKT>(s, red);
            c = blk_sum<PKT>(c, red);
            const double mean = s / c;
            double d = 0.0;
            for (int i = tid; i < n; i += PKT) if (!isinf(fxx[i])) { const double t = fabs(fxx[i] - mean); d += t * t; }
            d = blk_sum<PKT>(d, red);
            prominence = 0.05 * sqrt(d / c) + 5e-3;
        } else {
            prominence = 5e-3;
        }
    }

    // ---- the search (drt1d.py:3886-3913): one pass, or the passes -1 and +1 with the f test ----
    if (a.o.search != 0) {
        peaks_pass(fxx, f, n, a.o.search, false, height, prominence, sgn, prom, lb, rb);
    } else {
        peaks_pass(fxx, f, n, -1, true, height, prominence, sgn, prom, lb, rb);
        peaks_pass(fxx, f, n, 1, true, height, prominence, sgn, prom, lb, rb);   // (a maximum of fxx is no maximum of -fxx)
    }
    __syncthreads();

    // ---- probabilities (drt1d.py:3915-3941; curvature.py:46-53) ----
    double thresh = a.o.prob_thresh;
    if (l.var) {
        for (int i = tid; i < n; i += PKT) {
            if (sgn[i] == 0) continue;
            const double h = sgn[i] > 0 ? -fxx[i] : fxx[i];
            if (method == 1) prob[i] = 1.0 - erfc(np_min(prom[i], h) / (sqrt(vxx[i]) * PK_SQRT2));
            else prob[i] = map_peak_prob(prom[i], h, f[i], vxx[i], vf[i]);
        }
        __syncthreads();
        if (l.sort) {
            // the min(num_peaks, count)-th largest probability; two passes can put peaks on neighbouring samples, so every sample has a slot
            double c = 0.0;
            for (int i = tid; i < a.p2; i += PKT) {
                const bool pk = i < n && sgn[i] != 0;
                srt[i] = pk ? prob[i] : -INFINITY;
                if (pk) c += 1.0;
            }
            c = blk_sum<PKT>(c, red);                    // (ends with a barrier: srt is complete)
            lds_sort<PKT>(srt, a.p2);
            const int cnt = (int)c, k = a.o.num_peaks < cnt ? a.o.num_peaks : cnt;
            if (cnt > 0) thresh = srt[a.p2 - k];
        }
    }

    // ---- the dense rows: the only global stores of the kernel besides the two scalars below ----
    double kept = 0.0;
    for (int i = tid; i < n; i += PKT) {
        const size_t o = row + i;
        const int s = sgn[i];
        const int kp = s != 0 && (method != 1 || prob[i] >= thresh) ? 1 : 0;
        kept += (double)kp;
        if (a.peak_sign) a.peak_sign[o] = s;
        if (a.keep) a.keep[o] = kp;
        if (a.heights) a.heights[o] = s == 0 ? 0.0 : (s > 0 ? -fxx[i] : fxx[i]);
        if (a.prominences) a.prominences[o] = prom[i];
        if (a.probs) a.probs[o] = l.var ? prob[i] : 0.0;
        if (a.left_bases) a.left_bases[o] = lb[i];
        if (a.right_bases) a.right_bases[o] = rb[i];
        if (method == 2) {
            const double sf = np_sign(f[i]);
            if (a.peak_prob) a.peak_prob[o] = prob[i] * sf;
            if (a.curv_prob) a.curv_prob[o] = map_curv_prob(f[i], fxx[i], sf, vf[i], vxx[i]);
        }
    }
    kept = blk_sum<PKT>(kept, red);
    if (tid == 0) {
        if (a.count) a.count[b] = (int)kept;
        if (a.used_prominence) a.used_prominence[b] = prominence;
    }
}

size_t peaks_lds_bytes(int neval, int method, int need_f, int num_peaks) {
    return peaks_lds(nullptr, neval, next_pow2(neval), method, need_f, num_peaks).bytes;
}

int peak_check_opts(const hipdrt_peak_opts& o, int neval) {
    HIPDRT_REQUIRE(neval >= 1, "neval >= 1");
    HIPDRT_REQUIRE(o.search >= -1 && o.search <= 1, "search must be 1, -1 or 0 (two passes)");
    HIPDRT_REQUIRE(o.method >= 0 && o.method <= 2, "method must be 0 (thresh), 1 (prob) or 2 (map probabilities)");
    HIPDRT_REQUIRE(!std::isinf(o.height) && !std::isinf(o.prominence), "height and prominence: finite, or NaN for automatic");
    HIPDRT_REQUIRE(std::isfinite(o.prob_thresh), "prob_thresh must be finite");
    HIPDRT_REQUIRE(o.num_peaks >= 0, "num_peaks >= 0 (0: off)");
    HIPDRT_REQUIRE(std::isfinite(o.fxx_var_floor), "fxx_var_floor must be finite");
    HIPDRT_REQUIRE(o.ext_left >= -1 && o.ext_left < neval && o.ext_right >= -1 && o.ext_right < neval,
                   "ext_left and ext_right: an index of the evaluation grid, or -1");
    return HIPDRT_OK;
}

int launch_peaks(hipStream_t s, PeakArgs a, int B) {
    if (int rc = peak_check_opts(a.o, a.neval)) return rc;
    HIPDRT_REQUIRE(B >= 1 && a.fxx, "peaks: B >= 1 and the curvature rows");
    HIPDRT_REQUIRE(a.f || (a.o.search != 0 && a.o.method != 2), "peaks: a two-pass search and the map probabilities need the f rows");
    HIPDRT_REQUIRE(a.o.method == 0 || a.var_fxx, "peaks: methods 1 and 2 need the curvature's variance");
    HIPDRT_REQUIRE(a.o.method != 2 || a.var_f, "peaks: method 2 needs the variance of f");
    if (a.o.search != 0 && a.o.method != 2) a.f = nullptr;      // not read: not staged
    a.p2 = next_pow2(a.neval);
    const size_t lds = peaks_lds_bytes(a.neval, a.o.method, a.f != nullptr, a.o.num_peaks);
    if (int rc = lds_check(lds, "peaks", "neval, method")) return rc;
    if (int rc = set_lds(reinterpret_cast<const void*>(peaks_kernel), lds, "peaks_kernel")) return rc;
    hipLaunchKernelGGL(peaks_kernel, dim3(B), dim3(PKT), lds, s, a);
    return 0;
}

// out[b] = x[b] * y[b]: a caller's per-spectrum factor on top of the plan's coefficient scale
__global__ void scale_mul_kernel(int B, const double* __restrict__ x, const double* __restrict__ y, double* __restrict__ out) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b < B) out[b] = x[b] * y[b];
}
void launch_scale_mul(hipStream_t s, int B, const double* x, const double* y, double* out) {
    hipLaunchKernelGGL(scale_mul_kernel, dim3((B + 255) / 256), dim3(256), 0, s, B, x, y, out);
}

}  // namespace hipdrt
