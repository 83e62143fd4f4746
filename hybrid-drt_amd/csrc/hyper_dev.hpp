// Device helpers shared by the one-workgroup-per-spectrum kernels (hyper.hip, kk.hip, peaks.hip, peak_resolve.hip): 512-thread workgroups (peaks.hip,
// peak_resolve.hip: 256, through the template argument), wavefront and block reductions, the bitonic sort, and the row-slab matrix-vector product.
#pragma once
#include "common.hpp"

namespace hipdrt {

static constexpr int HT = 512;
static constexpr int HNW = HT / 64;

// DPP moves of a double (two dwords); ctrl: quad_perm 0x00-0xFF, row_ror:n = 0x120 + n
template <int CTRL>
__device__ __forceinline__ double dpp_mov(double v) {
    const int lo = __double2loint(v), hi = __double2hiint(v);
    return __hiloint2double(__builtin_amdgcn_update_dpp(0, hi, CTRL, 0xF, 0xF, true),
                            __builtin_amdgcn_update_dpp(0, lo, CTRL, 0xF, 0xF, true));
}
__device__ __forceinline__ double lane_bcast(double v, int lane) {
    return __hiloint2double(__builtin_amdgcn_readlane(__double2hiint(v), lane),
                            __builtin_amdgcn_readlane(__double2loint(v), lane));
}
// wavefront sum, every lane gets the total: quad permutes and row rotations (VALU speed) inside the 16-lane rows,
// v_readlane across the four rows -- no LDS crossbar traffic
__device__ __forceinline__ double hw_sum(double v) {
    v += dpp_mov<0xB1>(v);          // lane ^ 1
    v += dpp_mov<0x4E>(v);          // lane ^ 2
    v += dpp_mov<0x124>(v);         // row_ror:4
    v += dpp_mov<0x128>(v);         // row_ror:8
    return (lane_bcast(v, 0) + lane_bcast(v, 16)) + (lane_bcast(v, 32) + lane_bcast(v, 48));
}
__device__ __forceinline__ double hw_max(double v) {
    v = fmax(v, dpp_mov<0xB1>(v));
    v = fmax(v, dpp_mov<0x4E>(v));
    v = fmax(v, dpp_mov<0x124>(v));
    v = fmax(v, dpp_mov<0x128>(v));
    return fmax(fmax(lane_bcast(v, 0), lane_bcast(v, 16)), fmax(lane_bcast(v, 32), lane_bcast(v, 48)));
}
__device__ __forceinline__ double hw_min(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v = fmin(v, __shfl_xor(v, off, 64));
    return v;
}

// block-wide reductions over NT threads; red = LDS [NT / 64]; two syncs so `red` is immediately reusable
template <int NT = HT>
__device__ __forceinline__ double blk_sum(double v, double* red) {
    v = hw_sum(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = 0.0;
#pragma unroll
    for (int w = 0; w < NT / 64; ++w) t += red[w];
    return t;
}
__device__ __forceinline__ double blk_max(double v, double* red) {
    v = hw_max(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = red[0];
#pragma unroll
    for (int w = 1; w < HNW; ++w) t = fmax(t, red[w]);
    return t;
}
__device__ __forceinline__ double blk_min(double v, double* red) {
    v = hw_min(v);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    double t = red[0];
#pragma unroll
    for (int w = 1; w < HNW; ++w) t = fmin(t, red[w]);
    return t;
}

// ascending bitonic network over p2 (a power of two, lds_layout.hpp: next_pow2) doubles in LDS, NT threads
template <int NT = HT>
__device__ __forceinline__ void lds_sort(double* __restrict__ v, int p2) {
    for (int k = 2; k <= p2; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int i = threadIdx.x; i < p2; i += NT) {
                const int l = i ^ j;
                if (l > i) {
                    const double a = v[i], c = v[l];
                    const bool up = (i & k) == 0;
                    if (up ? (a > c) : (a < c)) { v[i] = c; v[l] = a; }
                }
            }
            __syncthreads();
        }
    }
}

// y[i] = sum_j M[i][j] * v[j] for the rows owned by this wavefront; v in LDS; result to LDS out.  Four rows per
// pass with 16-byte loads, MV_UC column chunks of 128 requested before the first product: 4 * MV_UC independent loads
// in flight per lane (one L2 round trip per 512 columns instead of one per chunk; more would not fit 128 VGPRs).  Columns past the end are
// loaded from a clamped address and left out of the sum, so the per-lane order of additions is the plain loop's.
static constexpr int MV_UC = 4;
__device__ __forceinline__ void rows_matvec(const double* __restrict__ M, int ld, int nrow, int ncol,
                                            const double* __restrict__ v, double* __restrict__ out) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    if (((ld | ncol) & 1) == 0 && (reinterpret_cast<size_t>(M) & 15) == 0) {
        for (int i0 = 4 * wv; i0 < nrow; i0 += 4 * HNW) {
            const double* r0 = M + (size_t)i0 * ld;
            const double* r1 = M + (size_t)(i0 + 1 < nrow ? i0 + 1 : i0) * ld;
            const double* r2 = M + (size_t)(i0 + 2 < nrow ? i0 + 2 : i0) * ld;
            const double* r3 = M + (size_t)(i0 + 3 < nrow ? i0 + 3 : i0) * ld;
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
            for (int base = 0; base < ncol; base += 128 * MV_UC) {
                const int jb = base + 2 * lane;
                double2 a0[MV_UC], a1[MV_UC], a2[MV_UC], a3[MV_UC];
#pragma unroll
                for (int c = 0; c < MV_UC; ++c) {
                    if (base + 128 * c >= ncol) break;               // the whole chunk lies past the end (uniform)
                    const int j = jb + 128 * c, jj = j < ncol ? j : ncol - 2;
                    a0[c] = *reinterpret_cast<const double2*>(r0 + jj);
                    a1[c] = *reinterpret_cast<const double2*>(r1 + jj);
                    a2[c] = *reinterpret_cast<const double2*>(r2 + jj);
                    a3[c] = *reinterpret_cast<const double2*>(r3 + jj);
                }
#pragma unroll
                for (int c = 0; c < MV_UC; ++c) {
                    const int j = jb + 128 * c;
                    if (j < ncol) {
                        const double vx = v[j], vy = v[j + 1];
                        s0 += a0[c].x * vx + a0[c].y * vy;
                        s1 += a1[c].x * vx + a1[c].y * vy;
                        s2 += a2[c].x * vx + a2[c].y * vy;
                        s3 += a3[c].x * vx + a3[c].y * vy;
                    }
                }
            }
            s0 = hw_sum(s0); s1 = hw_sum(s1); s2 = hw_sum(s2); s3 = hw_sum(s3);
            if (lane == 0) {
                out[i0] = s0;
                if (i0 + 1 < nrow) out[i0 + 1] = s1;
                if (i0 + 2 < nrow) out[i0 + 2] = s2;
                if (i0 + 3 < nrow) out[i0 + 3] = s3;
            }
        }
        return;
    }
    for (int i = wv; i < nrow; i += HNW) {
        const double* row = M + (size_t)i * ld;
        double s = 0.0;
        for (int j = lane; j < ncol; j += 64) s += row[j] * v[j];
        s = hw_sum(s);
        if (lane == 0) out[i] = s;
    }
}

}  // namespace hipdrt
