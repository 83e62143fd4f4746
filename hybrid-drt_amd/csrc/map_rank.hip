// hipdrt_rank_filter, hipdrt_percentiles, hipdrt_map_badness (include/hipdrt.h): the order statistics behind the reference's
// quality control of a map (hybdrt/mapping/nddata.py: impute_nans 135-149, flag_outliers 152-175, flag_bad_obs 178-295;
// DRTMD.score_group_data_badness / score_group_fit_badness, hybdrt/mapping/drtmd.py:642-783), stated in numpy in
// hipdrt/filters/ndfilters.py (rank filters) and hipdrt/mapping/nddata.py (the chains).
//
//   rank_kernel<SR, SC>  scipy.ndimage's rank filters on the 'reflect' boundary: a 16 x 64 tile with its halo in LDS, up to three
//                        ranks of the same window in one pass (the median, and the pair behind iqr_filter as their difference).
//                        A window without a NaN is selected by a branch-free rank count (element i has rank
//                        #{j: w_j < w_i or w_j == w_i, j < i}); the instantiations for the chain's sizes hold the window in
//                        registers, the generic one (<0, 0>, any window up to 49 entries) reads it from the tile.  A window with
//                        a NaN goes through scipy's Hoare quickselect on a per-thread buffer in LDS, in scipy's element order,
//                        so that the result is scipy's (NaN compares false everywhere, so "where the NaN ends up" is a
//                        property of that very algorithm).  Ranks 0 and size - 1 of a NaN window are NaN (numpy's min / max).
//   select kernels       exact k-th smallest non-NaN values of every row, or of the whole array, by radix select over
//                        order-preserving 64-bit keys, eight bits a pass, integer histograms only: nothing depends on the
//                        launch geometry or on the order of the atomics.  A segment of up to SEL_BLOCK_LEN entries is selected
//                        by one workgroup in one launch (histograms in LDS); longer ones by many workgroups with the histograms
//                        in global memory.  numpy's 'linear' percentile and nanmedian's mean of the middle pair are formed from
//                        the two neighbouring order statistics.
//   chain kernels        the element-wise and per-row passes of flag_outliers, the 5 % rule and flag_bad_obs.
// Compiled with -ffp-contract=off: every product and sum rounds as numpy's does.
#include <cfloat>
#include <cmath>
#include <vector>

#include "map_filter_dev.hpp"

namespace hipdrt {
namespace {

// ---- rank filter -----------------------------------------------------------------------------------------------------------
constexpr int RANK_MAX_WINDOW = 49;        // (the tile, RT_R x RT_C outputs, is lds_layout.hpp's)

struct RankArgs {
    const double* in;
    const double* fill;          // device scalar that replaces a NaN as the tile is loaded (null: NaNs stay)
    double *out_rank, *out_diff; // rank_m of the window; rank_hi - rank_lo of the same window (either may be null)
    int R, C, sr, sc;
    int rank_m, rank_lo, rank_hi;
};

__device__ __forceinline__ int reflect_rank(int i, int n) {
    if (i < 0) i = -i - 1;
    if (i >= n) { i %= 2 * n; if (i >= n) i = 2 * n - 1 - i; }
    return i;
}

// scipy's NI_Select on buf[0 .. n-1] (entry k of this thread at sel[k * 256]).  The clamps never bind (Hoare's invariant keeps
// i and j inside [lo, hi]); they and the round count only bound the loops.
__device__ double ni_select(double* sel, int n, int rank) {
    int lo = 0, hi = n - 1;
    for (int round = 0; round < n && lo < hi; ++round) {
        const double x = sel[lo * 256];
        int i = lo - 1, j = hi + 1;
        for (;;) {
            do { --j; } while (j > lo && sel[j * 256] > x);
            do { ++i; } while (i < hi && sel[i * 256] < x);
            if (i >= j) break;
            const double t = sel[i * 256]; sel[i * 256] = sel[j * 256]; sel[j * 256] = t;
        }
        const int k = j - lo + 1;
        if (rank < k) hi = j;
        else { lo = j + 1; rank -= k; }
    }
    return sel[(lo < n ? lo : n - 1) * 256];
}

template <int SR, int SC>
__global__ __launch_bounds__(256) void rank_kernel(RankArgs a) {
    extern __shared__ double sm[];
    const int tid = threadIdx.x;
    const int sr = SR ? SR : a.sr, sc = SC ? SC : a.sc, n = sr * sc;
    const int r0 = blockIdx.x * RT_R, c0 = blockIdx.y * RT_C;
    const int WR = RT_R + sr - 1, WC = RT_C + sc - 1, WN = WR * WC;
    const RankLds L = rank_lds(sm, sr, sc);
    double* lds = L.win;
    double* sel = L.sel + tid;
    const double fill = a.fill ? *a.fill : 0.0;
    for (int e = tid; e < WN; e += 256) {
        const int gr = reflect_rank(r0 - sr / 2 + e / WC, a.R), gc = reflect_rank(c0 - sc / 2 + e % WC, a.C);
        double v = a.in[(size_t)gr * a.C + gc];
        if (a.fill && v != v) v = fill;
        lds[e] = v;
    }
    __syncthreads();
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    for (int e = tid; e < RT_R * RT_C; e += 256) {
        const int lr = e / RT_C, lc = e % RT_C, gr = r0 + lr, gc = c0 + lc;
        if (gr >= a.R || gc >= a.C) continue;
        const double* win = lds + lr * WC + lc;
        double vm = 0.0, vlo = 0.0, vhi = 0.0;
        bool nan = false;
        if constexpr (SR > 0) {
            constexpr int N = SR * SC;
            double w[N];
#pragma unroll
            for (int i = 0; i < SR; ++i)
#pragma unroll
                for (int j = 0; j < SC; ++j) w[i * SC + j] = win[i * WC + j];
#pragma unroll
            for (int i = 0; i < N; ++i) nan |= w[i] != w[i];
            if (!nan) {
#pragma unroll
                for (int i = 0; i < N; ++i) {
                    int c = 0;
#pragma unroll
                    for (int j = 0; j < N; ++j) c += (w[j] < w[i]) | ((j < i) & (w[j] == w[i]));
                    vm = c == a.rank_m ? w[i] : vm;
                    vlo = c == a.rank_lo ? w[i] : vlo;
                    vhi = c == a.rank_hi ? w[i] : vhi;
                }
            }
        } else {
            for (int k = 0; k < n; ++k) { const double v = win[(k / sc) * WC + k % sc]; nan |= v != v; }
            if (!nan) {
                for (int i = 0; i < n; ++i) {
                    const double wi = win[(i / sc) * WC + i % sc];
                    int c = 0;
                    for (int j = 0; j < n; ++j) {
                        const double wj = win[(j / sc) * WC + j % sc];
                        c += (wj < wi) | ((j < i) & (wj == wi));
                    }
                    vm = c == a.rank_m ? wi : vm;
                    vlo = c == a.rank_lo ? wi : vlo;
                    vhi = c == a.rank_hi ? wi : vhi;
                }
            }
        }
        if (nan) {
            // every rank selects from a fresh copy of the window, rows outer (scipy's filter buffer)
            auto select = [&](int rank) {
                if (rank <= 0 || rank >= n - 1) return qnan;
                for (int k = 0; k < n; ++k) sel[k * 256] = win[(k / sc) * WC + k % sc];
                return ni_select(sel, n, rank);
            };
            if (a.out_rank) vm = select(a.rank_m);
            if (a.out_diff) { vlo = select(a.rank_lo); vhi = select(a.rank_hi); }
        }
        const size_t gi = (size_t)gr * a.C + gc;
        if (a.out_rank) a.out_rank[gi] = vm;
        if (a.out_diff) a.out_diff[gi] = vhi - vlo;
    }
}

size_t rank_lds_bytes(int sr, int sc) { return rank_lds(nullptr, sr, sc).bytes; }

template <int SR, int SC>
int launch_rank(hipStream_t st, const RankArgs& a) {
    const size_t bytes = rank_lds_bytes(a.sr, a.sc);
    TRY(set_lds((const void*)rank_kernel<SR, SC>, bytes, "rank_kernel"));
    const dim3 grid((a.R + RT_R - 1) / RT_R, (a.C + RT_C - 1) / RT_C);
    hipLaunchKernelGGL((rank_kernel<SR, SC>), grid, dim3(256), bytes, st, a);
    LAUNCH_OK();
    return HIPDRT_OK;
}

int check_window(int R, int C, int sr, int sc) {
    HIPDRT_REQUIRE(R >= 1 && C >= 1 && (long long)R * C < (1LL << 30), "rows, cols >= 1, rows * cols < 2^30");
    HIPDRT_REQUIRE((C + RT_C - 1) / RT_C <= 65535, "at most 65535 * 64 entries along a row");
    HIPDRT_REQUIRE(sr >= 1 && sc >= 1, "window sizes >= 1");
    if ((long long)sr * sc > RANK_MAX_WINDOW) {
        set_error("rank filter: windows of more than 49 entries are not built");
        return HIPDRT_E_UNSUPPORTED;
    }
    return HIPDRT_OK;
}

// in -> out_rank (rank_m) and / or out_diff (rank_hi - rank_lo), NaNs replaced by *fill on the way in when fill is given
int rank_filter_device(hipStream_t st, const double* in, const double* fill, int R, int C, int sr, int sc, int rank_m, int rank_lo,
                       int rank_hi, double* out_rank, double* out_diff) {
    TRY(check_window(R, C, sr, sc));
    const int n = sr * sc;
    HIPDRT_REQUIRE(!out_rank || (rank_m >= 0 && rank_m < n), "0 <= rank < size");
    HIPDRT_REQUIRE(!out_diff || (rank_lo >= 0 && rank_lo < n && rank_hi >= 0 && rank_hi < n), "0 <= rank < size");
    RankArgs a{in, fill, out_rank, out_diff, R, C, sr, sc, out_rank ? rank_m : -1, out_diff ? rank_lo : -1, out_diff ? rank_hi : -1};
    if (sr == 3 && sc == 1) return launch_rank<3, 1>(st, a);
    if (sr == 5 && sc == 1) return launch_rank<5, 1>(st, a);
    if (sr == 3 && sc == 3) return launch_rank<3, 3>(st, a);
    if (sr == 5 && sc == 3) return launch_rank<5, 3>(st, a);
    return launch_rank<0, 0>(st, a);
}

// ---- order statistics ------------------------------------------------------------------------------------------------------
constexpr int SEL_MAXQ = 4, SEL_T = 2 * SEL_MAXQ;
constexpr size_t SEL_BLOCK_LEN = 16384;     // longest segment one workgroup selects on its own
constexpr int SEL_MAX_CHUNKS = 1024;

struct SelTarget { unsigned long long prefix; unsigned int rank, pad; };
struct SelQ { int nq; double q[SEL_MAXQ]; };        // fractions in [0, 1]; < 0: nanmedian's rule

__device__ __forceinline__ unsigned long long sel_key(double v) {
    const unsigned long long u = v == 0.0 ? 0ull : (unsigned long long)__double_as_longlong(v);      // -0 and +0: one key
    return (u >> 63) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ double sel_value(unsigned long long k) {
    return __longlong_as_double((long long)((k >> 63) ? (k ^ 0x8000000000000000ull) : ~k));
}

// the two order statistics around numpy's virtual index (n - 1) q, and the weight of the upper one
__device__ void sel_setup(unsigned int n, const SelQ& q, SelTarget* tg, double* tfrac) {
    for (int k = 0; k < q.nq; ++k) {
        unsigned int lo = 0, hi = 0;
        double t = 0.0;
        if (n > 0) {
            if (q.q[k] < 0.0) { lo = (n - 1) / 2; hi = n / 2; }
            else {
                const double v = (double)(n - 1) * q.q[k];
                lo = (unsigned int)floor(v);
                if (lo > n - 1) lo = n - 1;
                hi = lo + 1 < n ? lo + 1 : n - 1;
                t = v - (double)lo;
            }
        }
        tg[2 * k] = SelTarget{0ull, lo, 0u};
        tg[2 * k + 1] = SelTarget{0ull, hi, 0u};
        tfrac[k] = t;
    }
}

__device__ void sel_pick(const unsigned int* hist, SelTarget& t) {
    unsigned int cum = 0;
    int d = 0;
    for (; d < 255; ++d) {
        const unsigned int c = hist[d];
        if (cum + c > t.rank) break;
        cum += c;
    }
    t.prefix = (t.prefix << 8) | (unsigned long long)d;
    t.rank -= cum;
}

__device__ double sel_finish(unsigned int n, double q, double t, const SelTarget& lo, const SelTarget& hi) {
    if (n == 0) return __longlong_as_double(0x7ff8000000000000LL);
    const double a = sel_value(lo.prefix), b = sel_value(hi.prefix);
    if (q < 0.0) return (a + b) / 2.0;
    const double d = b - a;
    double r = a + d * t;
    if (t >= 0.5) r = b - d * (1.0 - t);
    return r;
}

// one workgroup per segment: count, eight histogram passes in LDS, the interpolation
__global__ __launch_bounds__(256) void sel_block_kernel(const double* __restrict__ a, unsigned int len, SelQ q,
                                                        double* __restrict__ out) {
    __shared__ unsigned int hist[SEL_T * 256];
    __shared__ SelTarget tg[SEL_T];
    __shared__ double tfrac[SEL_MAXQ];
    __shared__ unsigned int count;
    const int tid = threadIdx.x, T = 2 * q.nq;
    const double* x = a + (size_t)blockIdx.x * len;
    if (tid == 0) count = 0;
    __syncthreads();
    unsigned int mine = 0;
    for (unsigned int i = tid; i < len; i += 256) mine += x[i] == x[i];
    atomicAdd(&count, mine);
    __syncthreads();
    if (tid == 0) sel_setup(count, q, tg, tfrac);
    for (int shift = 56; shift >= 0; shift -= 8) {
        for (int k = tid; k < T * 256; k += 256) hist[k] = 0;
        __syncthreads();
        for (unsigned int i = tid; i < len; i += 256) {
            const double v = x[i];
            if (v != v) continue;
            const unsigned long long key = sel_key(v);
            const unsigned long long top = shift == 56 ? 0ull : key >> (shift + 8);
            const unsigned int digit = (unsigned int)(key >> shift) & 255u;
            for (int t = 0; t < T; ++t)
                if (top == tg[t].prefix) atomicAdd(&hist[t * 256 + digit], 1u);
        }
        __syncthreads();
        if (tid < T) sel_pick(hist + tid * 256, tg[tid]);
        __syncthreads();
    }
    if (tid < q.nq) out[(size_t)blockIdx.x * q.nq + tid] = sel_finish(count, q.q[tid], tfrac[tid], tg[2 * tid], tg[2 * tid + 1]);
}

// many workgroups per segment: grid (segments, chunks)
__global__ __launch_bounds__(256) void sel_count_kernel(const double* __restrict__ a, size_t len, unsigned int* __restrict__ cnt) {
    __shared__ unsigned int count;
    const int tid = threadIdx.x;
    const double* x = a + (size_t)blockIdx.x * len;
    if (tid == 0) count = 0;
    __syncthreads();
    unsigned int mine = 0;
    for (size_t i = (size_t)blockIdx.y * 256 + tid; i < len; i += (size_t)gridDim.y * 256) mine += x[i] == x[i];
    atomicAdd(&count, mine);
    __syncthreads();
    if (tid == 0 && count) atomicAdd(&cnt[blockIdx.x], count);
}

__global__ void sel_setup_kernel(const unsigned int* __restrict__ cnt, int nseg, SelQ q, SelTarget* __restrict__ tg,
                                 double* __restrict__ tfrac) {
    const int s = blockIdx.x * blockDim.x + threadIdx.x;
    if (s < nseg) sel_setup(cnt[s], q, tg + (size_t)s * 2 * q.nq, tfrac + (size_t)s * q.nq);
}

__global__ __launch_bounds__(256) void sel_hist_kernel(const double* __restrict__ a, size_t len, int T, int shift,
                                                       const SelTarget* __restrict__ tg_all, unsigned int* __restrict__ hist_all) {
    __shared__ unsigned int hist[SEL_T * 256];
    __shared__ unsigned long long prefix[SEL_T];
    const int tid = threadIdx.x;
    const double* x = a + (size_t)blockIdx.x * len;
    for (int k = tid; k < T * 256; k += 256) hist[k] = 0;
    if (tid < T) prefix[tid] = tg_all[(size_t)blockIdx.x * T + tid].prefix;
    __syncthreads();
    for (size_t i = (size_t)blockIdx.y * 256 + tid; i < len; i += (size_t)gridDim.y * 256) {
        const double v = x[i];
        if (v != v) continue;
        const unsigned long long key = sel_key(v);
        const unsigned long long top = shift == 56 ? 0ull : key >> (shift + 8);
        const unsigned int digit = (unsigned int)(key >> shift) & 255u;
        for (int t = 0; t < T; ++t)
            if (top == prefix[t]) atomicAdd(&hist[t * 256 + digit], 1u);
    }
    __syncthreads();
    unsigned int* g = hist_all + (size_t)blockIdx.x * T * 256;
    for (int k = tid; k < T * 256; k += 256)
        if (hist[k]) atomicAdd(&g[k], hist[k]);
}

__global__ void sel_pick_kernel(const unsigned int* __restrict__ hist_all, size_t ntargets, SelTarget* __restrict__ tg) {
    const size_t k = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k < ntargets) sel_pick(hist_all + k * 256, tg[k]);
}

__global__ void sel_finish_kernel(const unsigned int* __restrict__ cnt, int nseg, SelQ q, const SelTarget* __restrict__ tg,
                                  const double* __restrict__ tfrac, double* __restrict__ out) {
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nseg * q.nq) return;
    const int s = k / q.nq, j = k % q.nq;
    const SelTarget* t = tg + (size_t)s * 2 * q.nq;
    out[k] = sel_finish(cnt[s], q.q[j], tfrac[k], t[2 * j], t[2 * j + 1]);
}

// percentiles q[0 .. nq) (per cent; HIPDRT_Q_NANMEDIAN: nanmedian) of the non-NaN values of each of nseg segments of len entries
int percentiles_device(hipStream_t st, const double* a, int nseg, size_t len, const double* q_percent, int nq, double* out) {
    HIPDRT_REQUIRE(nseg >= 1 && len >= 1 && (long long)nseg * (long long)len < (1LL << 30), "rows, cols >= 1, rows * cols < 2^30");
    HIPDRT_REQUIRE(nq >= 1 && nq <= SEL_MAXQ, "1 .. 4 percentiles a call");
    SelQ q{};
    q.nq = nq;
    for (int k = 0; k < nq; ++k) {
        const double p = q_percent[k];
        HIPDRT_REQUIRE(p == HIPDRT_Q_NANMEDIAN || (p >= 0.0 && p <= 100.0), "percentiles in [0, 100]");
        q.q[k] = p == HIPDRT_Q_NANMEDIAN ? -1.0 : p / 100.0;
    }
    if (len <= SEL_BLOCK_LEN) {
        hipLaunchKernelGGL(sel_block_kernel, dim3(nseg), dim3(256), 0, st, a, (unsigned int)len, q, out);
        LAUNCH_OK();
        return HIPDRT_OK;
    }
    const int T = 2 * nq;
    const int chunks = (int)std::min<size_t>(SEL_MAX_CHUNKS, (len + 4095) / 4096);
    const size_t ntargets = (size_t)nseg * T;
    DevBuf cnt, tg, tfrac, hist;
    HIPDRT_CHECK(cnt.alloc(nseg * sizeof(unsigned int)));
    HIPDRT_CHECK(tg.alloc(ntargets * sizeof(SelTarget)));
    HIPDRT_CHECK(tfrac.alloc((size_t)nseg * nq * sizeof(double)));
    HIPDRT_CHECK(hist.alloc(ntargets * 256 * sizeof(unsigned int)));
    HIPDRT_CHECK(hipMemsetAsync(cnt.p, 0, nseg * sizeof(unsigned int), st));
    hipLaunchKernelGGL(sel_count_kernel, dim3(nseg, chunks), dim3(256), 0, st, a, len, cnt.as<unsigned int>());
    hipLaunchKernelGGL(sel_setup_kernel, dim3((nseg + 255) / 256), dim3(256), 0, st, cnt.as<unsigned int>(), nseg, q, tg.as<SelTarget>(),
                       tfrac.d());
    LAUNCH_OK();
    for (int shift = 56; shift >= 0; shift -= 8) {
        HIPDRT_CHECK(hipMemsetAsync(hist.p, 0, ntargets * 256 * sizeof(unsigned int), st));
        hipLaunchKernelGGL(sel_hist_kernel, dim3(nseg, chunks), dim3(256), 0, st, a, len, T, shift, tg.as<SelTarget>(),
                           hist.as<unsigned int>());
        hipLaunchKernelGGL(sel_pick_kernel, dim3((unsigned int)((ntargets + 255) / 256)), dim3(256), 0, st, hist.as<unsigned int>(),
                           ntargets, tg.as<SelTarget>());
        LAUNCH_OK();
    }
    hipLaunchKernelGGL(sel_finish_kernel, dim3((nseg * nq + 255) / 256), dim3(256), 0, st, cnt.as<unsigned int>(), nseg, q,
                       tg.as<SelTarget>(), tfrac.d(), out);
    LAUNCH_OK();
    HIPDRT_CHECK(hipStreamSynchronize(st));          // the work buffers go out of scope
    return HIPDRT_OK;
}

// ---- the element-wise and per-row passes of the chains ------------------------------------------------------------------------
__device__ __forceinline__ double nan_to_num(double v) {
    if (v != v) return 0.0;
    if (isinf(v)) return v > 0 ? DBL_MAX : -DBL_MAX;
    return v;
}

// drtmd.py:675-679: (v - 0.5 (v_hi + v_lo)) / (i_hi - i_lo) with the rows' 2 % and 98 % nanpercentiles (pa, ps: [rows][2])
__global__ __launch_bounds__(256) void scale_kernel(double* __restrict__ a, size_t n, int C, const double* __restrict__ pa,
                                                    const double* __restrict__ ps) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const size_t r = i / C;
    const double mid = 0.5 * (pa[2 * r + 1] + pa[2 * r]), range = ps[2 * r + 1] - ps[2 * r];
    a[i] = (a[i] - mid) / range;
}

__global__ __launch_bounds__(256) void nan_to_num_kernel(const double* __restrict__ in, size_t n, double* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = nan_to_num(in[i]);
}

// impute_nans' last step: y_filt = y where y is a number, the masked Gaussian elsewhere (in place, in `filt`)
__global__ __launch_bounds__(256) void impute_kernel(const double* __restrict__ y, size_t n, double* __restrict__ filt) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n && y[i] == y[i]) filt[i] = y[i];
}

// flag_outliers 164-175 with preprocessing.outlier_prob (860-876) and stats.pdf_normal; q: the 25 % and 75 % percentiles of
// nan_to_num(y_filt) behind stats.robust_std
__global__ __launch_bounds__(256) void outlier_kernel(const double* __restrict__ y, const double* __restrict__ mu,
                                                      const double* __restrict__ iqr, const double* __restrict__ q, size_t n,
                                                      double two_nstd, double fsc, double p_prior, double thresh, double sqrt2pi,
                                                      unsigned char* __restrict__ flag) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double rs = n < 2 ? __longlong_as_double(0x7ff8000000000000LL) : (q[1] - q[0]) / two_nstd;
    double s_in = iqr[i] / 1.349;
    s_in = s_in + fsc * rs;
    s_in = s_in + 1e-8;
    const double d = y[i] - mu[i], dev = fabs(d);
    const double s_out = dev + 1e-8;
    const double num = -0.5 * (d * d);
    const double pdf_in = 1.0 / (s_in * sqrt2pi) * exp(num / (s_in * s_in));
    const double pdf_out = 1.0 / (s_out * sqrt2pi) * exp(num / (s_out * s_out));
    double p = p_prior * pdf_out / ((1.0 - p_prior) * pdf_in + p_prior * pdf_out);
    if (dev <= s_in) p = 0.0;
    p = nan_to_num(p);
    flag[i] = p > thresh;
}

// drtmd.py:699-707: a row with fewer than min_count flagged entries has them set to NaN.  One workgroup per row.
__global__ __launch_bounds__(256) void flag_rule_kernel(double* __restrict__ a, const unsigned char* __restrict__ flag, int C,
                                                        int min_count) {
    __shared__ unsigned int count;
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * C;
    if (tid == 0) count = 0;
    __syncthreads();
    unsigned int mine = 0;
    for (int c = tid; c < C; c += 256) mine += flag[base + c];
    if (mine) atomicAdd(&count, mine);
    __syncthreads();
    if ((int)count >= min_count) return;
    const double qnan = __longlong_as_double(0x7ff8000000000000LL);
    for (int c = tid; c < C; c += 256)
        if (flag[base + c]) a[base + c] = qnan;
}

// flag_bad_obs 197-210: x_std = iqr / 1.349 + 0.1 robust_std, resid = nan_to_num((raw - filt) / x_std), rss = sum resid^2 / C.
// One workgroup per row; thread t sums its columns t, t + 256, ... in order, then a binary tree over the threads.
__global__ __launch_bounds__(256) void rss_kernel(const double* __restrict__ raw, const double* __restrict__ filt,
                                                  const double* __restrict__ iqr, const double* __restrict__ q, size_t nvalid_min,
                                                  const unsigned int* __restrict__ nvalid, double two_nstd, int C,
                                                  double* __restrict__ rss, unsigned int* __restrict__ nan_std) {
    __shared__ double s[256];
    const int tid = threadIdx.x;
    const size_t base = (size_t)blockIdx.x * C;
    const double rs = *nvalid < nvalid_min ? __longlong_as_double(0x7ff8000000000000LL) : (q[1] - q[0]) / two_nstd;
    double acc = 0.0;
    bool bad = false;
    for (int c = tid; c < C; c += 256) {
        double x_std = iqr[base + c] / 1.349;
        x_std = x_std + 0.1 * rs;
        bad |= x_std != x_std;
        const double r = nan_to_num((raw[base + c] - filt[base + c]) / x_std);
        acc += r * r;
    }
    if (bad) atomicOr(nan_std, 1u);
    s[tid] = acc;
    for (int h = 128; h >= 1; h >>= 1) {
        __syncthreads();
        if (tid < h) s[tid] = s[tid] + s[tid + h];
    }
    if (tid == 0) rss[blockIdx.x] = s[0] / (double)C;
}

__global__ __launch_bounds__(256) void count_valid_kernel(const double* __restrict__ a, size_t n, unsigned int* __restrict__ cnt) {
    __shared__ unsigned int count;
    if (threadIdx.x == 0) count = 0;
    __syncthreads();
    unsigned int mine = 0;
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256) mine += a[i] == a[i];
    if (mine) atomicAdd(&count, mine);
    __syncthreads();
    if (threadIdx.x == 0 && count) atomicAdd(cnt, count);
}

}  // namespace
}  // namespace hipdrt

using namespace hipdrt;

extern "C" int hipdrt_rank_filter(hipdrt_ctx* ctx, const double* a, int rows, int cols, int size_r, int size_c, int op, int rank_lo,
                                  int rank_hi, double* out) try {
    HIPDRT_REQUIRE(ctx && a && out, "NULL pointer");
    HIPDRT_REQUIRE(op == HIPDRT_RANK_ONE || op == HIPDRT_RANK_DIFF, "op");
    TRY(check_window(rows, cols, size_r, size_c));
    hipStream_t st; TRY(enter(ctx, &st));
    const size_t bytes = (size_t)rows * cols * sizeof(double);
    DevBuf in, res;
    TRY(upload(in, a, bytes, st));
    HIPDRT_CHECK(res.alloc(bytes));
    const bool one = op == HIPDRT_RANK_ONE;
    TRY(rank_filter_device(st, in.d(), nullptr, rows, cols, size_r, size_c, rank_lo, rank_lo, rank_hi, one ? res.d() : nullptr,
                           one ? nullptr : res.d()));
    HIPDRT_CHECK(hipMemcpyAsync(out, res.p, bytes, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

extern "C" int hipdrt_percentiles(hipdrt_ctx* ctx, const double* a, int rows, int cols, int by_row, const double* q, int nq,
                                  double* out) try {
    HIPDRT_REQUIRE(ctx && a && q && out, "NULL pointer");
    HIPDRT_REQUIRE(rows >= 1 && cols >= 1 && (long long)rows * cols < (1LL << 30), "rows, cols >= 1, rows * cols < 2^30");
    hipStream_t st; TRY(enter(ctx, &st));
    const size_t n = (size_t)rows * cols;
    const int nseg = by_row ? rows : 1;
    DevBuf in, res;
    TRY(upload(in, a, n * sizeof(double), st));
    HIPDRT_CHECK(res.alloc((size_t)nseg * std::max(nq, 1) * sizeof(double)));
    TRY(percentiles_device(st, in.d(), nseg, by_row ? (size_t)cols : n, q, nq, res.d()));
    HIPDRT_CHECK(hipMemcpyAsync(out, res.p, (size_t)nseg * nq * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

extern "C" int hipdrt_map_badness(hipdrt_ctx* ctx, const hipdrt_map_badness_args* g, const double* a, const double* scale_src,
                                  double* rss_out, unsigned char* flags_out, double* filt_out) try {
    HIPDRT_REQUIRE(ctx && g && a && (rss_out || !g->score), "NULL pointer");
    HIPDRT_REQUIRE(g->score || (g->flag_outliers && flags_out), "score = 0 is the flag chain alone: flag_outliers = 1 and flags_out");
    const int R = g->rows, C = g->cols;
    TRY(check_window(R, C, g->median_size[0], g->median_size[1]));
    TRY(check_window(R, C, g->std_size[0], g->std_size[1]));
    if (g->flag_outliers) TRY(check_window(R, C, g->flag_size[0], g->flag_size[1]));
    HIPDRT_REQUIRE(!g->scale || scale_src, "scale = 1 needs scale_src");
    HIPDRT_REQUIRE(!flags_out || g->flag_outliers, "flags_out goes with flag_outliers = 1");
    HIPDRT_REQUIRE(g->n_std > 0, "n_std > 0");
    hipStream_t st; TRY(enter(ctx, &st));
    const size_t n = (size_t)R * C, bytes = n * sizeof(double);
    const dim3 ew((unsigned int)((n + 255) / 256)), tb(256);
    const double two_nstd = 2 * g->n_std;
    auto window_rank = [](const int* size, double pct) { return (int)((double)(size[0] * size[1]) * pct / 100.0); };
    DevBuf x, src, filt, iqr, tmp, scal, flag, cnt, rss;
    TRY(upload(x, a, bytes, st));
    for (DevBuf* b : {&filt, &iqr, &tmp}) HIPDRT_CHECK(b->alloc(bytes));
    HIPDRT_CHECK(scal.alloc(((size_t)4 * R + 8) * sizeof(double)));
    HIPDRT_CHECK(cnt.alloc(2 * sizeof(unsigned int)));
    HIPDRT_CHECK(rss.alloc((size_t)R * sizeof(double)));
    HIPDRT_CHECK(hipMemsetAsync(cnt.p, 0, 2 * sizeof(unsigned int), st));
    double* const glob = scal.d() + (size_t)4 * R;     // [0, 1]: 25 / 75 % of the flag chain; [2]: nanmedian, [3, 4]: 25 / 75 % of filt
    hipEvent_t ev0, ev1;
    HIPDRT_CHECK(hipEventCreate(&ev0)); HIPDRT_CHECK(hipEventCreate(&ev1));
    struct EventGuard { hipEvent_t a, b; ~EventGuard() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } guard{ev0, ev1};
    if (g->scale) TRY(upload(src, scale_src, bytes, st));
    HIPDRT_CHECK(hipEventRecord(ev0, st));

    if (g->scale) {
        const double q[2] = {2.0, 98.0};
        TRY(percentiles_device(st, x.d(), R, C, q, 2, scal.d()));
        TRY(percentiles_device(st, src.d(), R, C, q, 2, scal.d() + (size_t)2 * R));
        hipLaunchKernelGGL(scale_kernel, ew, tb, 0, st, x.d(), n, C, scal.d(), scal.d() + (size_t)2 * R);
        LAUNCH_OK();
    }
    if (g->flag_outliers) {
        // impute_nans leaves an array without NaNs as it is, so with impute = 1 the masked Gaussian runs unconditionally
        HIPDRT_CHECK(flag.alloc(n));
        if (g->impute) {
            TRY(masked_gaussian_device(st, x.d(), R, C, g->impute_gauss, filt.d()));
            hipLaunchKernelGGL(impute_kernel, ew, tb, 0, st, x.d(), n, filt.d());
        } else {
            HIPDRT_CHECK(hipMemcpyAsync(filt.p, x.p, bytes, hipMemcpyDeviceToDevice, st));
        }
        hipLaunchKernelGGL(nan_to_num_kernel, ew, tb, 0, st, filt.d(), n, tmp.d());
        LAUNCH_OK();
        const double q[2] = {25.0, 75.0};
        TRY(percentiles_device(st, tmp.d(), 1, n, q, 2, glob));
        const int nw = g->flag_size[0] * g->flag_size[1];
        TRY(rank_filter_device(st, filt.d(), nullptr, R, C, g->flag_size[0], g->flag_size[1], nw / 2, window_rank(g->flag_size, 25.0),
                               window_rank(g->flag_size, 75.0), tmp.d(), iqr.d()));
        hipLaunchKernelGGL(outlier_kernel, ew, tb, 0, st, x.d(), tmp.d(), iqr.d(), glob, n, two_nstd, g->full_std_contribution,
                           g->p_prior, g->thresh, std::sqrt(2 * M_PI), flag.as<unsigned char>());
        LAUNCH_OK();
        if (!g->score) {
            HIPDRT_CHECK(hipMemcpyAsync(flags_out, flag.p, n, hipMemcpyDeviceToHost, st));
            HIPDRT_CHECK(hipStreamSynchronize(st));
            return HIPDRT_OK;
        }
        hipLaunchKernelGGL(flag_rule_kernel, dim3(R), tb, 0, st, x.d(), flag.as<unsigned char>(), C, (int)(C * 0.05));
        LAUNCH_OK();
    }
    // the median-filtered array, then flag_bad_obs(robust_std=True) against it
    const int nm = g->median_size[0] * g->median_size[1];
    if (g->filt_in) HIPDRT_CHECK(hipMemcpyAsync(filt.p, g->filt_in, bytes, hipMemcpyHostToDevice, st));
    else TRY(rank_filter_device(st, x.d(), nullptr, R, C, g->median_size[0], g->median_size[1], nm / 2, 0, 0, filt.d(), nullptr));
    const double q3[3] = {HIPDRT_Q_NANMEDIAN, 25.0, 75.0};
    TRY(percentiles_device(st, filt.d(), 1, n, q3, 3, glob + 2));
    hipLaunchKernelGGL(count_valid_kernel, dim3((unsigned int)std::min<size_t>(1024, (n + 255) / 256)), tb, 0, st, filt.d(), n,
                       cnt.as<unsigned int>());
    TRY(rank_filter_device(st, filt.d(), glob + 2, R, C, g->std_size[0], g->std_size[1], 0, window_rank(g->std_size, 25.0),
                           window_rank(g->std_size, 75.0), nullptr, iqr.d()));
    hipLaunchKernelGGL(rss_kernel, dim3(R), tb, 0, st, x.d(), filt.d(), iqr.d(), glob + 3, (size_t)2, cnt.as<unsigned int>(), two_nstd,
                       C, rss.d(), cnt.as<unsigned int>() + 1);
    LAUNCH_OK();
    HIPDRT_CHECK(hipEventRecord(ev1, st));
    unsigned int host_cnt[2] = {0, 0};
    HIPDRT_CHECK(hipMemcpyAsync(host_cnt, cnt.p, sizeof(host_cnt), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(rss_out, rss.p, (size_t)R * sizeof(double), hipMemcpyDeviceToHost, st));
    if (flags_out) HIPDRT_CHECK(hipMemcpyAsync(flags_out, flag.p, n, hipMemcpyDeviceToHost, st));
    if (filt_out) HIPDRT_CHECK(hipMemcpyAsync(filt_out, filt.p, bytes, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    float ms = 0.f;
    HIPDRT_CHECK(hipEventElapsedTime(&ms, ev0, ev1));
    ctx->map_badness_ms = ms;
    if (host_cnt[1]) {
        set_error("x_std contains nans!");
        return HIPDRT_E_NUMERIC;
    }
    return HIPDRT_OK;
} HIPDRT_CATCH

extern "C" int hipdrt_debug_map_badness_ms(hipdrt_ctx* ctx, double* ms) try {
    HIPDRT_REQUIRE(ctx && ms, "NULL pointer");
    *ms = ctx->map_badness_ms;
    return HIPDRT_OK;
} HIPDRT_CATCH
