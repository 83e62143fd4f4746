// Kramers-Kronig screening of the fitted batch (one 512-thread workgroup per spectrum), the step between the two fits of
// DRT.kk_test (hybdrt/models/drt1d.py:1370-1391) and after the second:
//
//   stage A   predict_z at the fit frequencies and kk.normalize_residuals(norm="modulus")     hybdrt/models/kk.py:9-19,
//             drt1d.py:1472-1481
//   stage B   kk.get_outliers (kk.py:21-53; stats.robust_std, hybdrt/utils/stats.py:124-134, with numpy's 'linear' percentile;
//             stats.outer_cdf_chi2 for k = 2 in closed form) and kk.get_limits (kk.py:56-123)
//   rows      the next kk_fit's vector-valued weight_factor (drt1d.py:1399-1404), written into the plan's row-factor buffer
//
// Stage B also runs alone on supplied residuals (hipdrt_debug_kk_stats).  hipdrt/models/kk.py is the same arithmetic in numpy.
#include "hyper_dev.hpp"

namespace hipdrt {

// np.percentile(method='linear') on the first N entries of the sorted array: virtual index q / 100 * (N - 1), numpy's _lerp
__device__ __forceinline__ double lds_percentile(const double* __restrict__ v, int N, double q) {
    const double vi = q / 100.0 * (double)(N - 1);
    int lo = (int)floor(vi);
    lo = lo < 0 ? 0 : (lo > N - 1 ? N - 1 : lo);
    const int hi = lo + 1 > N - 1 ? N - 1 : lo + 1;
    const double t = vi - (double)lo, a = v[lo], c = v[hi], d = c - a;
    return t >= 0.5 ? c - d * (1.0 - t) : a + d * t;
}

// stage A: yh = rm_b x_b, residuals in percent of |Z| into er / ei (LDS), optional global copies
__device__ __forceinline__ void kk_residuals(const FitState& st, const KkArgs& a, int b, double* __restrict__ xs,
                                             double* __restrict__ yh, double* __restrict__ er, double* __restrict__ ei) {
    const int tid = threadIdx.x, n = st.n, m = st.m, nf = a.nf;
    for (int i = tid; i < n; i += HT) xs[i] = st.x[(size_t)b * n + i];
    __syncthreads();
    rows_matvec(st.rm + (size_t)b * st.rm_stride, st.ldrm, m, n, xs, yh);
    __syncthreads();
    const double* rv = st.rv + (size_t)b * m;
    const double cs = st.coef_scale[b];
    for (int k = tid; k < nf; k += HT) {
        const double zr = rv[k], zi = rv[nf + k];
        const double mod = hypot(zr, zi);
        const double e_r = 100.0 * (zr - yh[k]) / mod, e_i = 100.0 * (zi - yh[nf + k]) / mod;
        er[k] = e_r; ei[k] = e_i;
        const size_t o = (size_t)b * nf + k;
        if (a.z_re) a.z_re[o] = cs * yh[k];
        if (a.z_im) a.z_im[o] = cs * yh[nf + k];
        if (a.e_re) a.e_re[o] = e_r;
        if (a.e_im) a.e_im[o] = e_i;
    }
    __syncthreads();
}

// stage B: outlier mask from er / ei, then the clean window.  srt: [p2] doubles (p2 = the power of two >= 2 nf, so that it also
// holds three int vectors of nf entries for the window rule), mask: [nf] ints.
__device__ __forceinline__ void kk_stats(const KkArgs& a, int b, const double* __restrict__ er, const double* __restrict__ ei,
                                         double* __restrict__ srt, int* __restrict__ mask, double* __restrict__ red) {
    __shared__ double sh_std;
    const int tid = threadIdx.x, nf = a.nf, p2 = a.p2;
    const hipdrt_kk_opts& o = a.o;
    for (int k = tid; k < nf; k += HT) mask[k] = 0;
    if (tid == 0) sh_std = NAN;
    __syncthreads();
    for (int it = 0; it < o.n_outlier_iter; ++it) {
        // the unmasked Re and Im values, masked ones and the padding as +inf: sorted, the first N entries are the sample
        double nm = 0.0, bad = 0.0;
        for (int k = tid; k < nf; k += HT) {
            const bool mk = mask[k] != 0;
            srt[2 * k] = mk ? INFINITY : er[k];
            srt[2 * k + 1] = mk ? INFINITY : ei[k];
            if (mk) nm += 1.0;
            else if (!(isfinite(er[k]) && isfinite(ei[k]))) bad += 1.0;
        }
        for (int i = 2 * nf + tid; i < p2; i += HT) srt[i] = INFINITY;
        nm = blk_sum(nm, red);
        bad = blk_sum(bad, red);                   // (ends with a barrier: srt is complete)
        lds_sort(srt, p2);
        const int N = 2 * (nf - (int)nm);
        if (tid == 0) {
            double sd = NAN;
            if (N >= 2 && bad == 0.0) {
                const double q_lo = lds_percentile(srt, N, 50.0 - 100.0 * o.std_sample_fraction / 2.0);
                const double q_hi = lds_percentile(srt, N, 50.0 + 100.0 * o.std_sample_fraction / 2.0);
                sd = (q_hi - q_lo) / (2.0 * o.n_std);
            }
            sh_std = sd;
        }
        __syncthreads();
        const double sd = sh_std;
        const bool ok = isfinite(sd) && sd > 0.0;          // otherwise the reference compares against NaN: nothing is masked
        for (int k = tid; k < nf; k += HT) {
            const double e2 = er[k] * er[k] + ei[k] * ei[k];
            bool out = false;
            if (ok) out = o.n_sigma > 0.0 ? sqrt(e2) > o.n_sigma * sd : exp(-e2 / (2.0 * sd * sd)) < o.p_thresh;
            mask[k] = out ? 1 : 0;
        }
        __syncthreads();
    }
    const double sd_out = sh_std;
    for (int k = tid; k < nf; k += HT) if (a.mask) a.mask[(size_t)b * nf + k] = mask[k];
    if (a.wrow) {
        double* wr = a.wrow + (size_t)b * 2 * nf;
        for (int k = tid; k < nf; k += HT) { const double f = mask[k] ? o.outlier_weight : 1.0; wr[k] = f; wr[nf + k] = f; }
    }

    // ---- the clean window (kk.get_limits), positions j in descending-frequency order ----
    int* oj = reinterpret_cast<int*>(srt);     // o[j]
    int* sa = oj + nf;                         // inclusive running sums of o (two buffers for the scan)
    int* sb = sa + nf;
    const int desc = a.desc;
    for (int j = tid; j < nf; j += HT) { const int v = mask[desc ? j : nf - 1 - j]; oj[j] = v; sa[j] = v; }
    __syncthreads();
    for (int off = 1; off < nf; off <<= 1) {
        for (int j = tid; j < nf; j += HT) sb[j] = sa[j] + (j >= off ? sa[j - off] : 0);
        __syncthreads();
        int* t = sa; sa = sb; sb = t;
    }
    const int* S = sa;
    auto clean = [&](int j) { return oj[j > 0 ? j - 1 : 0] + oj[j] + oj[j + 1 < nf ? j + 1 : nf - 1] == 0; };
    // first / last clean position at or after / before a bound (nf / -1: none)
    auto first_clean_from = [&](int from) {
        double v = (double)nf;
        for (int j = tid; j < nf; j += HT) if (j >= from && clean(j)) v = fmin(v, (double)j);
        return (int)blk_min(v, red);
    };
    auto last_clean_upto = [&](int upto) {
        double v = -1.0;
        for (int j = tid; j < nf; j += HT) if (j <= upto && clean(j)) v = fmax(v, (double)j);
        return (int)blk_max(v, red);
    };
    int i_left = first_clean_from(0), i_right = last_clean_upto(nf - 1);
    int status = 0;
    if (i_left >= nf) {
        status = 1; i_left = i_right = -1;             // the reference raises IndexError
    } else {
        const int inside = i_right > i_left ? S[i_right - 1] - (i_left > 0 ? S[i_left - 1] : 0) : 0;
        if (inside > o.max_num_outliers) {
            // fl[l] = S[i_left + l] - base, fr[r] = S[i_right] - S[i_right - r - 1]: both non-decreasing, so for every r the
            // smallest admissible l is found by bisection; smallest r + l wins, ties to the smallest r
            const int need = inside - o.max_num_outliers, L = i_right - i_left + 1;
            const int base = i_left > 0 ? S[i_left - 1] : 0;
            double best = 4.0 * (double)nf * (double)nf;
            for (int r = tid; r < L; r += HT) {
                const int below = i_right - r - 1;
                const int want = need - (S[i_right] - (below >= 0 ? S[below] : 0));
                int lo = 0, hi = L - 1;                  // fl[L - 1] >= inside >= need: an admissible l exists
                while (lo < hi) {
                    const int mid = (lo + hi) >> 1;
                    if (S[i_left + mid] - base >= want) hi = mid; else lo = mid + 1;
                }
                best = fmin(best, (double)(r + lo) * (double)(2 * nf) + (double)r);
            }
            best = blk_min(best, red);
            const int sum = (int)(best / (double)(2 * nf)), r = (int)(best - (double)sum * (double)(2 * nf));
            i_left += sum - r;
            i_right -= r;
        }
        const bool move_l = oj[i_left] != 0, move_r = oj[i_right] != 0;       // (uniform: every thread reads the same entries)
        if (move_l) i_left = first_clean_from(i_left);
        if (move_r) i_right = last_clean_upto(i_right);
        // (cannot happen: the outer clean points bracket both bounds -- kept so that no index leaves [0, nf) whatever the input)
        if (i_left >= nf || i_right < 0) { status = 1; i_left = i_right = -1; }
    }
    if (tid == 0) {
        if (a.std) a.std[b] = sd_out;
        if (a.status) a.status[b] = status;
        if (a.i_lim) { a.i_lim[2 * b] = i_left; a.i_lim[2 * b + 1] = i_right; }
        if (a.f_lim) {
            a.f_lim[2 * b] = status ? NAN : a.freq[desc ? i_right : nf - 1 - i_right];          // f_min
            a.f_lim[2 * b + 1] = status ? NAN : a.freq[desc ? i_left : nf - 1 - i_left];        // f_max
        }
    }
}

// grid = B.  stage_a != 0: residuals from the plan's state (st), else from a.in_re / a.in_im.
__global__ __launch_bounds__(HT) void kk_kernel(FitState st, KkArgs a, int stage_a) {
    extern __shared__ double sm[];
    __shared__ double red[HNW];
    const int b = blockIdx.x, tid = threadIdx.x, nf = a.nf;
    const KkLds L = kk_lds(sm, nf, a.p2, st.n, stage_a);
    double *er = L.er, *ei = L.ei, *srt = L.srt, *xs = L.xs, *yh = L.yh;
    int* mask = L.mask;
    if (stage_a) {
        if (st.fit_status[b] < 0) {              // the fit of this spectrum failed: nothing to screen
            for (int k = tid; k < nf; k += HT) {
                const size_t o = (size_t)b * nf + k;
                if (a.z_re) a.z_re[o] = NAN;
                if (a.z_im) a.z_im[o] = NAN;
                if (a.e_re) a.e_re[o] = NAN;
                if (a.e_im) a.e_im[o] = NAN;
                if (a.mask) a.mask[o] = 0;
                if (a.wrow) { a.wrow[(size_t)b * 2 * nf + k] = 1.0; a.wrow[(size_t)b * 2 * nf + nf + k] = 1.0; }
            }
            if (tid == 0) {
                if (a.std) a.std[b] = NAN;
                if (a.status) a.status[b] = -1;
                if (a.i_lim) { a.i_lim[2 * b] = -1; a.i_lim[2 * b + 1] = -1; }
                if (a.f_lim) { a.f_lim[2 * b] = NAN; a.f_lim[2 * b + 1] = NAN; }
            }
            return;
        }
        kk_residuals(st, a, b, xs, yh, er, ei);
    } else {
        for (int k = tid; k < nf; k += HT) { er[k] = a.in_re[(size_t)b * nf + k]; ei[k] = a.in_im[(size_t)b * nf + k]; }
        __syncthreads();
    }
    kk_stats(a, b, er, ei, srt, mask, red);
}

size_t kk_lds_bytes(int nf, int n, int stage_a) { return kk_lds(nullptr, nf, kk_p2(nf), n, stage_a).bytes; }

int launch_kk(hipStream_t s, const FitState* st, KkArgs a, int B) {
    const int stage_a = st != nullptr;
    a.p2 = kk_p2(a.nf);
    if (a.nf < 1 || (stage_a && st->m != 2 * a.nf)) { set_error("invalid argument: KK screen: m must be 2 nf"); return HIPDRT_E_INVALID; }
    const size_t lds = kk_lds_bytes(a.nf, stage_a ? st->n : 0, stage_a);
    if (lds > kLdsLimit) {
        set_error("invalid argument: KK screen: " + std::to_string(lds) + " bytes of LDS needed (nf, n), " + std::to_string(kLdsLimit) + " available");
        return HIPDRT_E_INVALID;
    }
    if (int rc = set_lds(reinterpret_cast<const void*>(kk_kernel), lds, "kk_kernel")) return rc;
    FitState none{};
    hipLaunchKernelGGL(kk_kernel, dim3(B), dim3(HT), lds, s, stage_a ? *st : none, a, stage_a);
    return 0;
}

}  // namespace hipdrt
