// Scoring many candidate solutions of every spectrum of a fitted batch (DRT.generate_candidates, hybdrt/models/drt1d.py:1632-1821):
// the two likelihood sums of DRT.evaluate_llh(weights=estimate_weights(x), x) (drt1d.py:4457-4496, qphb.py:1347-1377) for C
// candidates x per spectrum, defined as llh_kernel (hyper.hip) with stored = 0 defines them for one x,
//
//     yh = rm_b x,  r = yh - rv_b,  s = vmm r^2 floored at var_floor[b],  w = max(s^-1/2, 1e-10),
//     rss = sum (w yh)^2 - 2 sum (w rv)(w yh) + sum (w rv)^2,   sum_log_w = sum log w,
//
// and the compaction of peaks_kernel's dense rows into per-candidate peak lists.  hipdrt/models/candidates.py
// (candidate_llh_terms) is the same arithmetic in numpy.
//
// Layout.  llh_kernel reads rm (m x n) and vmm (m x m) once per x.  Here a 256-thread workgroup (4 wavefronts) owns 16
// candidates of ONE spectrum, so both matrix-vector products become 16-row matrix products on v_mfma_f64_16x16x4_f64 and every
// tile of rm and of vmm is read once per 16 candidates.  Both products run through cand_pass: per 64-wide slab of k the 16 x 64
// operand rows (x, then r^2) and 64 matrix rows (16 per wavefront) are staged through LDS, k-contiguous with leading dimension 68
// as in predict.hip (every bank pair is hit exactly twice per 64 lanes, the minimum for 8-byte words).  MFMA operands as there:
// A[l & 15][l >> 4] = operand rows (rows = candidates), B[l >> 4][l & 15] = matrix rows; C/D: col = lane & 15 (matrix row),
// row = (lane >> 4) + 4 reg (candidate).  The 16 x m tile yh = X rm' is formed first and kept -- in LDS (16 rows of
// round_up(m, 32) + 4 doubles), or, when that does not fit beside the staging slabs (m > 896; configuration 5 has m = 5120), in a
// scratch buffer of C B m doubles between two launches of the same code.  r^2 is re-formed from yh and rv as the second
// product's operand is staged.
//
// Order of summation.  Every element of either product has ONE accumulator that receives its k-blocks of four in ascending
// order from k = 0.  The four sums of a candidate run over the matrix rows i: wavefront w takes the tiles w, w + 4, ... in
// ascending order into one partial per lane (i mod 16), the 16 lanes are combined by one xor tree (1, 2, 4, 8), the four
// wavefronts in ascending order.  All of that is a function of (m, n) alone: a candidate gives the same bits alone and inside
// any C, a spectrum the same bits alone and inside a batch, and both forms of keeping yh the same bits (the values that reach the
// MFMAs and the epilogue are the same doubles either way).  Tails in C, m and n are staged as zeros; rows past the spectrum's
// candidate count are never stored.  Compiled with -ffp-contract=off: the epilogue rounds as written.
#include <cmath>

#include "common.hpp"

namespace hipdrt {

typedef double v4d __attribute__((ext_vector_type(4)));

static constexpr int CT = 16, CK = 64, CLD = 68, CW = 4;       // candidates per workgroup, k slab, slab leading dimension, wavefronts
// static LDS of cand_llh_kernel: the two staging slabs and the reduction table
static constexpr size_t kCandStaticLds = ((size_t)CT * CLD + (size_t)CW * 16 * CLD + (size_t)CW * CT * 4) * sizeof(double);
// LDS of a gfx950 CU available to one workgroup, static part included -- not kLdsLimit, which bounds the dynamic part alone
static constexpr size_t kCandLdsTotal = 160 * 1024;

static __host__ __device__ inline int cand_ldy(int m) { return (m + 31) / 32 * 32 + 4; }
static inline size_t cand_dyn_lds(int m) { return (size_t)CT * cand_ldy(m) * sizeof(double); }

bool cand_llh_fits_lds(int m) { return cand_dyn_lds(m) + kCandStaticLds + 512 <= kCandLdsTotal; }

// acc(candidate, matrix row) = sum_k A(candidate, k) M[row][k] for all rows of M [nrow][ldM] (K columns read): loadA(cl, k) gives
// the operand of local candidate cl (0 where it has none), epi(tile, acc) receives the finished 16 x 16 tile of rows 16 tile ..
// (element reg of the lane: candidate (lane >> 4) + 4 reg, row 16 tile + (lane & 15)).  Every wavefront makes the same number of
// trips, so the barriers are uniform; a wavefront whose tile lies past nrow multiplies zeros.
template <class LoadA, class Epi>
__device__ __forceinline__ void cand_pass(int nrow, int K, const double* __restrict__ M, long long ldM, LoadA loadA, Epi epi,
                                          double* __restrict__ sA, double* __restrict__ sM) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int srow = tid >> 4, skc = tid & 15;                 // staging map: 16 lanes along k (128 contiguous bytes per row)
    const int ntile = (nrow + 15) / 16;
    // slab k0 + CK is fetched (global or LDS -> registers) while slab k0 is multiplied out of LDS; tails come in as zeros
    double va[CK / 16], vm[CW * (CK / 16)];
    auto fetch = [&](int t0, int k0) {
#pragma unroll
        for (int j = 0; j < CK / 16; ++j) va[j] = loadA(srow, k0 + skc + 16 * j);
#pragma unroll
        for (int rr = 0; rr < CW; ++rr) {
            const int i = (t0 + rr) * 16 + srow;
#pragma unroll
            for (int j = 0; j < CK / 16; ++j) {
                const int k = k0 + skc + 16 * j;
                vm[rr * (CK / 16) + j] = (i < nrow && k < K) ? M[(size_t)i * ldM + k] : 0.0;
            }
        }
    };
    __syncthreads();                                           // what loadA reads (the previous pass's tile in LDS) is complete
    for (int t0 = 0; t0 < ntile; t0 += CW) {
        v4d acc = (v4d){0.0, 0.0, 0.0, 0.0};
        fetch(t0, 0);
        for (int k0 = 0; k0 < K; k0 += CK) {
            __syncthreads();                                   // previous slab fully consumed
#pragma unroll
            for (int j = 0; j < CK / 16; ++j) sA[srow * CLD + skc + 16 * j] = va[j];
#pragma unroll
            for (int rr = 0; rr < CW; ++rr)
#pragma unroll
                for (int j = 0; j < CK / 16; ++j) sM[(rr * 16 + srow) * CLD + skc + 16 * j] = vm[rr * (CK / 16) + j];
            __syncthreads();
            if (k0 + CK < K) fetch(t0, k0 + CK);
            const int left = K - k0;
            const int kend = left >= CK ? CK : (left + 3) & ~3; // whole blocks of four; the zeros past K are staged above
            for (int kk = 0; kk < kend; kk += 4) {
                const int kr = kk + (lane >> 4);
                const double av = sA[(lane & 15) * CLD + kr];
                const double ev = sM[(wv * 16 + (lane & 15)) * CLD + kr];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(av, ev, acc, 0, 0, 0);
            }
        }
        epi(t0 + wv, acc);
    }
}

// grid (ceil(C / 16), B).  FORM 0: both products, yh in LDS; 1: the first product, yh to a.scratch; 2: the second product and the
// sums, yh from a.scratch.
template <int FORM>
__global__ __launch_bounds__(256) void cand_llh_kernel(CandLlhArgs a) {
    extern __shared__ double dyn[];
    __shared__ double sA[CT * CLD];
    __shared__ double sM[CW * 16 * CLD];
    __shared__ double red[CW * CT * 4];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b = blockIdx.y, c0 = blockIdx.x * CT, m = a.m, n = a.n;
    const int slots = a.C - c0 < CT ? a.C - c0 : CT;            // output slots of this workgroup
    int nc = a.ncand ? a.ncand[b] : a.C;
    if (a.fit_status && a.fit_status[b] < 0) nc = 0;
    const int rows = nc - c0 < CT ? nc - c0 : CT;               // candidates of this workgroup (<= 0: none)
    if (rows <= 0) {
        if (FORM != 1 && tid < slots) { a.rss[(size_t)(c0 + tid) * a.B + b] = NAN; a.slw[(size_t)(c0 + tid) * a.B + b] = NAN; }
        return;
    }
    // yh of local candidate cl, row i: Y[cl * ystride + i]
    double* Y = FORM == 0 ? dyn : a.scratch + ((size_t)c0 * a.B + b) * m;
    const size_t ystride = FORM == 0 ? (size_t)cand_ldy(m) : (size_t)a.B * m;
    const double* rv = a.rv + (size_t)b * m;

    if (FORM != 2) {
        const double* x = a.x + (size_t)c0 * a.x_cstride + (size_t)b * a.x_bstride;
        cand_pass(m, n, a.rm + (size_t)b * a.rm_stride, a.ldrm,
                  [&](int cl, int k) { return (cl < rows && k < n) ? x[(size_t)cl * a.x_cstride + k] : 0.0; },
                  [&](int tile, const v4d& acc) {
                      const int i = tile * 16 + (lane & 15);
                      if (i >= m) return;
#pragma unroll
                      for (int reg = 0; reg < 4; ++reg) {
                          const int cl = (lane >> 4) + 4 * reg;
                          if (cl < rows) Y[cl * ystride + i] = acc[reg];
                      }
                  },
                  sA, sM);
    }
    if (FORM == 1) return;

    double pa[4] = {0.0, 0.0, 0.0, 0.0}, pc[4] = {0.0, 0.0, 0.0, 0.0}, pd[4] = {0.0, 0.0, 0.0, 0.0}, pl[4] = {0.0, 0.0, 0.0, 0.0};
    const double vf = a.var_floor[b];
    cand_pass(m, m, a.vmm, m,
              [&](int cl, int k) {
                  if (!(cl < rows && k < m)) return 0.0;
                  const double r = Y[cl * ystride + k] - rv[k];
                  return r * r;
              },
              [&](int tile, const v4d& acc) {
                  const int i = tile * 16 + (lane & 15);
                  if (i >= m) return;
                  const double rvi = rv[i];
#pragma unroll
                  for (int reg = 0; reg < 4; ++reg) {
                      const int cl = (lane >> 4) + 4 * reg;
                      if (cl >= rows) continue;
                      double v = acc[reg];
                      if (v < vf) v = vf;
                      const double w = fmax(1.0 / sqrt(v), 1e-10);
                      const double wy = w * Y[cl * ystride + i], wr = w * rvi;
                      pa[reg] += wy * wy; pc[reg] += wr * wy; pd[reg] += wr * wr; pl[reg] += log(w);
                  }
              },
              sA, sM);
    // the 16 lanes of a candidate (one xor tree), then the four wavefronts in ascending order
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
            pa[reg] += __shfl_xor(pa[reg], o); pc[reg] += __shfl_xor(pc[reg], o);
            pd[reg] += __shfl_xor(pd[reg], o); pl[reg] += __shfl_xor(pl[reg], o);
        }
        if ((lane & 15) == 0) {
            double* r = red + ((size_t)wv * CT + (lane >> 4) + 4 * reg) * 4;
            r[0] = pa[reg]; r[1] = pc[reg]; r[2] = pd[reg]; r[3] = pl[reg];
        }
    }
    __syncthreads();
    if (tid < slots) {
        double s[4] = {NAN, NAN, NAN, NAN};
        if (tid < rows) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                double t = 0.0;
#pragma unroll
                for (int w = 0; w < CW; ++w) t += red[((size_t)w * CT + tid) * 4 + q];
                s[q] = t;
            }
        }
        const size_t o = (size_t)(c0 + tid) * a.B + b;
        const bool dead = tid >= rows || (a.slot_status && a.slot_status[o] < 0);     // (a failed step's x was multiplied, not stored)
        a.rss[o] = dead ? NAN : s[0] - 2.0 * s[1] + s[2];
        a.slw[o] = dead ? NAN : s[3];
    }
}

size_t cand_llh_scratch_doubles(int C, int B, int m) { return (size_t)C * B * m; }

int launch_cand_llh(hipStream_t st, const CandLlhArgs& a, int form) {
    HIPDRT_REQUIRE(a.C >= 1 && a.B >= 1 && a.B <= 65535 && a.m >= 1 && a.n >= 1, "candidates: C, m, n >= 1 and 1 <= B <= 65535");
    HIPDRT_REQUIRE(a.x && a.rm && a.rv && a.vmm && a.var_floor && a.rss && a.slw, "candidates: NULL pointer");
    HIPDRT_REQUIRE(form == 0 || form == 1, "candidates: form must be 0 (yh in LDS) or 1 (yh through scratch)");
    const dim3 grid((a.C + CT - 1) / CT, a.B), block(256);
    if (form == 0) {
        HIPDRT_REQUIRE(cand_llh_fits_lds(a.m), "candidates: 16 rows of m doubles do not fit in LDS; use the scratch form");
        const size_t dyn = cand_dyn_lds(a.m);
        if (int rc = set_lds(reinterpret_cast<const void*>(cand_llh_kernel<0>), dyn, "cand_llh_kernel")) return rc;
        hipLaunchKernelGGL(cand_llh_kernel<0>, grid, block, dyn, st, a);
    } else {
        HIPDRT_REQUIRE(a.scratch, "candidates: the scratch form needs its buffer");
        hipLaunchKernelGGL(cand_llh_kernel<1>, grid, block, 0, st, a);
        hipLaunchKernelGGL(cand_llh_kernel<2>, grid, block, 0, st, a);
    }
    return HIPDRT_OK;
}

// peaks_kernel's dense rows of one candidate of every spectrum -> that candidate's compact lists: one thread per spectrum walks
// its keep row in ascending order.  status[b] < 0 (failed fit, slot past the spectrum's candidate count): count -1, empty rows.
// More peaks than max_peaks: the true count, HIPDRT_PEAKS_OVERFLOW and empty rows, as hipdrt_plan_resolve_peaks reports it.
__global__ void cand_compact_kernel(CandPeakArgs a) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= a.B) return;
    const int mp = a.max_peaks, st = a.slot_status[b];
    const size_t row = (size_t)b * a.neval, o = (size_t)b * mp;
    int k = 0;
    if (st >= 0) for (int i = 0; i < a.neval; ++i) k += a.keep[row + i] != 0;
    const bool fill = st >= 0 && k <= mp;
    int j = 0;
    if (fill)
        for (int i = 0; i < a.neval && j < mp; ++i) {
            if (!a.keep[row + i]) continue;
            if (a.peak_index) a.peak_index[o + j] = i;
            if (a.heights) a.heights[o + j] = a.dense_heights[row + i];
            if (a.prominences) a.prominences[o + j] = a.dense_prominences[row + i];
            ++j;
        }
    for (; j < mp; ++j) {
        if (a.peak_index) a.peak_index[o + j] = -1;
        if (a.heights) a.heights[o + j] = NAN;
        if (a.prominences) a.prominences[o + j] = NAN;
    }
    if (a.count) a.count[b] = st >= 0 ? k : -1;
    if (a.status) a.status[b] = st < 0 ? st : (k > mp ? HIPDRT_PEAKS_OVERFLOW : st);
}

void launch_cand_compact(hipStream_t st, const CandPeakArgs& a) {
    hipLaunchKernelGGL(cand_compact_kernel, dim3((a.B + 63) / 64), dim3(64), 0, st, a);
}

}  // namespace hipdrt
