// Kernel-matrix builders for gfx950 (compiled with -ffp-contract=off so that the interpolation
// arithmetic rounds exactly like numpy's un-fused slope*(x-xp[j])+fp[j]).
//
//  lookup_kernel          basis.generate_impedance_lookup        hybdrt/matrices/basis.py:648-669
//  impedance_*_kernel     mat1d.construct_impedance_matrix        hybdrt/matrices/mat1d.py:212-374
//  response_lookup_kernel basis.generate_response_lookup          hybdrt/matrices/basis.py:672-689, 616-618
//  response_interp_kernel, response_trapz_kernel<EXPDECAY>, step_column_kernel<PotColumn>
//                         mat1d.construct_response_matrix         hybdrt/matrices/mat1d.py:16-122
//  penalty_kernel         mat1d.construct_integrated_derivative_matrix  mat1d.py:125-209, basis.py:382-395
//  eis_vmm_kernel         mat1d.construct_eis_var_matrix          mat1d.py:493-515
//  phasor_z_kernel / step_column_kernel<PhasorVColumn>  phasance.construct_phasor_z_matrix / _v_matrix   hybdrt/matrices/phasance.py:108-144
//  chrono_vmm_kernel      mat1d.construct_chrono_var_matrix       mat1d.py:457-490 (transformed times: utils/chrono.py:5-44)
//
// Layout: every matrix row-major float64.  The interp build is HBM-write bound (2*nf*ntau*8 B per
// frequency grid); the lookup tables (3 arrays x 2 parts x ngrid x 8 B = 96 kB at ngrid=2000) are staged
// once per workgroup into LDS, each thread produces two adjacent tau columns of both parts and stores them
// as 16-byte vectors, so a wavefront writes 1 KiB contiguous per store instruction.
#include "common.hpp"

namespace hipdrt {

// Threads of a workgroup, one constant per kernel family: the kernel's launch bound, its index arithmetic and its launcher's dim3
// all read it here.
constexpr int kEntryBlock = 256;                       // one thread per entry or column
constexpr int kWaveBlock = 256;                        // one wavefront per entry (the trapezoid kernels) ...
constexpr int kWaves = kWaveBlock / 64;                // ... so this many entries per pass of a block,
constexpr int kWaveCols = 4 * kWaves;                  // and this many consecutive columns per block of a matrix build
constexpr int kRowBlock = 256;                         // one block per row of a variance matrix
constexpr int kPhasorBlock = 64;                       // one thread per nu column (erf-heavy: few columns, many rows)
constexpr int kInterpBlock = 1024;                     // impedance_interp_kernel
static inline int blocks_of(int n, int per_block) { return (n + per_block - 1) / per_block; }

constexpr double kPi = 3.141592653589793;
__device__ __forceinline__ double omega(double f) { return f * 2.0 * kPi; }

// entry of a lookup / column q of a matrix block that this wavefront owns
__device__ __forceinline__ int wave_entry() { return blockIdx.x * kWaves + (threadIdx.x >> 6); }
__device__ __forceinline__ int wave_column(int q) { return blockIdx.x * kWaveCols + q * kWaves + (threadIdx.x >> 6); }

// ---------------------------------------------------------------------------------------------------------
// integrands (basis.py:93-95, 565-570) evaluated for one y; lw = log(w*t), wt = w*t
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void integrand(double phi, double ey, double y, double lw, double w, double t,
                                          double& fre, double& fim) {
    const double den = 1.0 + exp(2.0 * (y + lw));
    fre = phi / den;
    fim = (((-phi) * ey) * w) * t / den;
}

__device__ __forceinline__ double wave_sum(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
    return v;
}

// One wavefront integrates one (w, t) pair with the ny-point trapezoid rule of np.trapezoid:
// sum_j d_j * (f_{j+1} + f_j) / 2 on y = linspace(-20, 20, ny).  Y: the LDS tables [ny] of stage_y_tables.
__device__ __forceinline__ void trapz_pair(const YTablesLds& Y, int ny, double w, double t, double& zre, double& zim) {
    const double *ys = Y.ys, *phis = Y.phis, *eys = Y.eys;
    const int lane = threadIdx.x & 63;
    const double lw = log(w * t);
    double sre = 0.0, sim = 0.0;
    for (int j = lane; j < ny - 1; j += 64) {
        double f0r, f0i, f1r, f1i;
        integrand(phis[j], eys[j], ys[j], lw, w, t, f0r, f0i);
        integrand(phis[j + 1], eys[j + 1], ys[j + 1], lw, w, t, f1r, f1i);
        const double d = ys[j + 1] - ys[j];
        sre += d * (f1r + f0r) / 2.0;
        sim += d * (f1i + f0i) / 2.0;
    }
    zre = wave_sum(sre);
    zim = wave_sum(sim);
}

// the prologue of every trapezoid kernel: y = np.linspace(-20, 20, ny), phi(y) and e^y in the block's dynamic LDS, filled and visible
__device__ __forceinline__ YTablesLds stage_y_tables(double* sm, int ny, double eps) {
    const YTablesLds Y = y_tables_lds(sm, ny);
    const double step = 40.0 / (double)(ny - 1);
    for (int j = threadIdx.x; j < ny; j += blockDim.x) {
        double y = (double)j * step + (-20.0);
        if (j == ny - 1) y = 20.0;
        Y.ys[j] = y;
        const double ey2 = eps * y;
        Y.phis[j] = exp(-(ey2 * ey2));
        Y.eys[j] = exp(y);
    }
    __syncthreads();
    return Y;
}

// grid: ceil(2*ngrid / kWaves) blocks; wave g handles table entry g (re for g < ngrid, else im)
__global__ __launch_bounds__(kWaveBlock) void lookup_kernel(double eps, int ngrid, int ny, const double* __restrict__ wt_re,
                                                     const double* __restrict__ wt_im, double* __restrict__ z_re,
                                                     double* __restrict__ z_im) {
    extern __shared__ double sm[];
    const YTablesLds Y = stage_y_tables(sm, ny, eps);
    const int g = wave_entry();
    if (g >= 2 * ngrid) return;
    const bool im = g >= ngrid;
    const int i = im ? g - ngrid : g;
    const double wt = im ? wt_im[i] : wt_re[i];
    double zr, zi;
    trapz_pair(Y, ny, wt, 1.0, zr, zi);
    if ((threadIdx.x & 63) == 0) {
        if (im) z_im[i] = zi; else z_re[i] = zr;
    }
}

__global__ __launch_bounds__(kEntryBlock) void slopes_kernel(int ngrid, const double* __restrict__ xp, const double* __restrict__ fp,
                              double* __restrict__ slopes) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j < ngrid - 1) slopes[j] = (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]);
    else if (j == ngrid - 1) slopes[j] = 0.0;
}

// np.interp(x, xp, fp) with numpy's semantics (end clamping, exact-knot shortcut, un-fused evaluation).
// xp is log(logspace(..)), i.e. uniform to ~1e-15, so the bin is found arithmetically and then verified
// against the true knots (result identical to numpy's binary search).
__device__ __forceinline__ double np_interp(double x, const double* xp, const double* fp, const double* sl,
                                            int ng, double x0, double inv_dx) {
    if (x > xp[ng - 1]) return fp[ng - 1];
    if (x < xp[0]) return fp[0];
    int j = (int)((x - x0) * inv_dx);
    j = j < 0 ? 0 : (j > ng - 1 ? ng - 1 : j);
    while (j > 0 && xp[j] > x) --j;
    while (j < ng - 1 && xp[j + 1] <= x) ++j;
    if (j == ng - 1) return fp[j];
    const double xj = xp[j];
    if (xj == x) return fp[j];
    return sl[j] * (x - xj) + fp[j];
}

// ln(2 pi f) per (grid, frequency) and ln(tau): the general build evaluates ln(omega tau) as their sum (one add
// per entry instead of one FP64 log; differs from log(omega*tau) by <= 2 ulp of the abscissa, i.e. ~1e-16
// relative in the interpolated value, and not at all in the clamped regions).
__global__ __launch_bounds__(kEntryBlock) void log_grid_kernel(int count_f, const double* __restrict__ freq, int ntau, const double* __restrict__ tau,
                                double* __restrict__ lw, double* __restrict__ lt) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i < count_f) lw[i] = log(omega(freq[i]));
    if (i < ntau) lt[i] = log(tau[i]);
}

// LDS image of one lookup for the general build: knots x[ng] and (value, slope) pairs fs[ng], so an interpolation is one
// 16-byte pair of knots (ds_read2_b64) plus one 16-byte (f, s) read instead of four to six dependent 8-byte reads
struct LutFS {
    const double* x;
    const double2* fs;
    double x_lo, x_hi, f_lo, f_hi, x0, inv_dx;
    int ng;
};

__device__ __forceinline__ LutFS stage_lut_fs(double* sm_x, double2* sm_fs, const double* __restrict__ xp,
                                              const double* __restrict__ fp, const double* __restrict__ sl, int ng) {
    for (int i = threadIdx.x; i < ng; i += blockDim.x) {
        sm_x[i] = xp[i];
        sm_fs[i] = make_double2(fp[i], sl[i]);
    }
    return LutFS{sm_x, sm_fs, xp[0], xp[ng - 1], fp[0], fp[ng - 1], xp[0], (double)(ng - 1) / (xp[ng - 1] - xp[0]), ng};
}

// Two np.interp evaluations on one table, written so that their LDS reads are independent and issue together.  bins2:
// arithmetic bin (the knots are log(logspace(..)), uniform to ~1e-15), checked against the true knots; the search only runs
// for a lane that sits on a rounding edge, so the result is numpy's for any increasing grid.  eval2: value from (f, s).
struct Bins2 { int ja, jb; double a0, b0; };

__device__ __forceinline__ Bins2 bins2(const LutFS& T, double xa, double xb) {
    int ja = (int)((xa - T.x0) * T.inv_dx), jb = (int)((xb - T.x0) * T.inv_dx);
    ja = min(max(ja, 0), T.ng - 2);
    jb = min(max(jb, 0), T.ng - 2);
    double a0 = T.x[ja], a1 = T.x[ja + 1], b0 = T.x[jb], b1 = T.x[jb + 1];
    if (__builtin_expect((a0 > xa) | (a1 <= xa) | (b0 > xb) | (b1 <= xb), 0)) {
        while (ja > 0 && T.x[ja] > xa) --ja;
        while (ja < T.ng - 2 && T.x[ja + 1] <= xa) ++ja;
        while (jb > 0 && T.x[jb] > xb) --jb;
        while (jb < T.ng - 2 && T.x[jb + 1] <= xb) ++jb;
        a0 = T.x[ja];
        b0 = T.x[jb];
    }
    return Bins2{ja, jb, a0, b0};
}

__device__ __forceinline__ void eval2(const LutFS& T, const Bins2& k, double xa, double xb, double& va, double& vb) {
    const double2 fa = T.fs[k.ja], fb = T.fs[k.jb];
    const double la = (k.a0 == xa) ? fa.x : fa.y * (xa - k.a0) + fa.x;
    const double lb = (k.b0 == xb) ? fb.x : fb.y * (xb - k.b0) + fb.x;
    va = xa >= T.x_hi ? T.f_hi : (xa < T.x_lo ? T.f_lo : la);
    vb = xb >= T.x_hi ? T.f_hi : (xb < T.x_lo ? T.f_lo : lb);
}

// INTERP, general (non-Toeplitz) build.  grid = (row chunks, B), 1024 threads: the 96 kB of tables are staged
// once per workgroup and amortised over `rows_per_block` rows; thread (tr, tc) walks rows tr, tr+RP, ... and owns
// two adjacent tau columns, so a wavefront stores 1 KiB contiguous per matrix per row.
__global__ __launch_bounds__(kInterpBlock) void impedance_interp_kernel(
    int freq_batched, const double* __restrict__ lw, int nf, const double* __restrict__ lt, int ntau, int ng,
    const double* __restrict__ lut6, int rows_per_block, int tpr, double* __restrict__ a_re,
    double* __restrict__ a_im) {
    extern __shared__ double sm[];
    static_assert(sizeof(LdsPair) == sizeof(double2) && alignof(LdsPair) == alignof(double2), "the layout's pair is a double2");
    const ImpedanceInterpLds L = impedance_interp_lds(sm, ng, rows_per_block);
    const LutPart<const double> Gr = lut_part(lut6, ng, 0);
    const LutFS Tr = stage_lut_fs(L.x_re, reinterpret_cast<double2*>(L.fs_re), Gr.x, Gr.f, Gr.slope, ng);
    const LutPart<const double> Gi = lut_part(lut6, ng, 1);      // formed here, behind the first staging loop, as it always was
    const LutFS Ti = stage_lut_fs(L.x_im, reinterpret_cast<double2*>(L.fs_im), Gi.x, Gi.f, Gi.slope, ng);
    const int b = blockIdx.y;
    const double* lwb = lw + (freq_batched ? (size_t)b * nf : 0);
    const int row0 = blockIdx.x * rows_per_block;
    const int rend = min(row0 + rows_per_block, nf);
    // ln(omega) of this workgroup's rows: an LDS read per row instead of a global load in front of every dependent chain
    double* slw = L.slw;
    for (int i = threadIdx.x; i < rend - row0; i += blockDim.x) slw[i] = lwb[row0 + i];
    // Z' and Z'' tabulated on the same abscissae (generate_impedance_lookup gives both one grid): one bin search serves both
    int mine = 1;
    for (int i = threadIdx.x; i < ng; i += blockDim.x) mine &= (Gr.x[i] == Gi.x[i]);
    const bool same_x = __syncthreads_and(mine) != 0;
    const int tc = threadIdx.x % tpr, tr = threadIdx.x / tpr, rp = blockDim.x / tpr;
    const bool even = (ntau & 1) == 0;
    typedef double v2d_t __attribute__((ext_vector_type(2)));
    for (int c = 2 * tc; c < ntau; c += 2 * tpr) {
        const bool two = (c + 1 < ntau);
        const double t0 = lt[c], t1 = two ? lt[c + 1] : lt[c];
        auto entry = [&](int r) {
            const double w = slw[r - row0];
            const double xa = w + t0, xb = w + t1;
            double re0, re1, im0, im1;
            Bins2 k = bins2(Tr, xa, xb);
            eval2(Tr, k, xa, xb, re0, re1);
            if (!same_x) k = bins2(Ti, xa, xb);
            eval2(Ti, k, xa, xb, im0, im1);
            const size_t o = ((size_t)b * nf + r) * ntau + c;
            if (two) {
                if (even) {
                    // written once, read later by another kernel: non-temporal 16-byte stores (plain stores measured
                    // 2-4 % slower; with the interpolation replaced by constants this mapping writes 5.0-5.9 TB/s)
                    const v2d_t vre = {re0, re1}, vim = {im0, im1};
                    __builtin_nontemporal_store(vre, reinterpret_cast<v2d_t*>(a_re + o));
                    __builtin_nontemporal_store(vim, reinterpret_cast<v2d_t*>(a_im + o));
                } else {
                    a_re[o] = re0; a_re[o + 1] = re1;
                    a_im[o] = im0; a_im[o + 1] = im1;
                }
            } else {
                a_re[o] = re0;
                a_im[o] = im0;
            }
        };
        int r = row0 + tr;
        for (; r + rp < rend; r += 2 * rp) { entry(r); entry(r + rp); }      // two rows in flight per pass
        if (r < rend) entry(r);
    }
}

// first column c[nf] (omega_n * tau_0) and first row r[ntau] (omega_0 * tau_m) of the Toeplitz shortcut
// (mat1d.py:353-360).  cr = {c_re[nf], r_re[ntau], c_im[nf], r_im[ntau]}.
// INTERP: one thread per entry; TRAPZ: one wavefront per entry.
__device__ __forceinline__ void toeplitz_pair(int i, const double* freq, int nf, const double* tau, double& w, double& t) {
    if (i < nf) { w = omega(freq[i]); t = tau[0]; }
    else { w = omega(freq[0]); t = tau[i - nf]; }
}

__global__ __launch_bounds__(kEntryBlock) void toeplitz_cr_interp_kernel(const double* __restrict__ freq, int nf, const double* __restrict__ tau,
                                          int ntau, int ng, const double* __restrict__ lut6, double* __restrict__ cr) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= nf + ntau) return;
    const LutPart<const double> Gr = lut_part(lut6, ng, 0), Gi = lut_part(lut6, ng, 1);
    const double idr = (double)(ng - 1) / (Gr.x[ng - 1] - Gr.x[0]);
    const double idi = (double)(ng - 1) / (Gi.x[ng - 1] - Gi.x[0]);
    double w, t;
    toeplitz_pair(i, freq, nf, tau, w, t);
    const double x = log(w * t);
    cr[i] = np_interp(x, Gr.x, Gr.f, Gr.slope, ng, Gr.x[0], idr);
    cr[nf + ntau + i] = np_interp(x, Gi.x, Gi.f, Gi.slope, ng, Gi.x[0], idi);
}

__global__ __launch_bounds__(kWaveBlock) void toeplitz_cr_trapz_kernel(const double* __restrict__ freq, int nf,
                                                                       const double* __restrict__ tau, int ntau, double eps,
                                                                       int ny, double* __restrict__ cr) {
    extern __shared__ double sm[];
    const YTablesLds Y = stage_y_tables(sm, ny, eps);
    const int i = wave_entry();
    if (i >= nf + ntau) return;
    double w, t, zr, zi;
    toeplitz_pair(i, freq, nf, tau, w, t);
    trapz_pair(Y, ny, w, t, zr, zi);
    if ((threadIdx.x & 63) == 0) { cr[i] = zr; cr[nf + ntau + i] = zi; }
}

// scipy.linalg.toeplitz(c, r): A[i][j] = c[i-j] (i >= j) else r[j-i]
__global__ __launch_bounds__(kEntryBlock) void toeplitz_fill_kernel(int B, int nf, int ntau, const double* __restrict__ cr, double* __restrict__ a_re,
                                     double* __restrict__ a_im) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    if (j >= ntau) return;
    const double* c_re = cr; const double* r_re = cr + nf;
    const double* c_im = cr + nf + ntau; const double* r_im = c_im + nf;
    for (int i = blockIdx.y; i < nf; i += gridDim.y) {
        const double vr = (i >= j) ? c_re[i - j] : r_re[j - i];
        const double vi = (i >= j) ? c_im[i - j] : r_im[j - i];
        for (int b = blockIdx.z; b < B; b += gridDim.z) {
            const size_t o = ((size_t)b * nf + i) * ntau + j;
            a_re[o] = vr;
            a_im[o] = vi;
        }
    }
}

// TRAPZ, general: one wavefront per matrix entry, kWaveCols consecutive tau columns per block.
__global__ __launch_bounds__(kWaveBlock) void impedance_trapz_kernel(int freq_batched, const double* __restrict__ freq, int nf,
                                                                     const double* __restrict__ tau, int ntau, double eps, int ny,
                                                                     double* __restrict__ a_re, double* __restrict__ a_im) {
    extern __shared__ double sm[];
    const YTablesLds Y = stage_y_tables(sm, ny, eps);
    const int b = blockIdx.z;
    const double* fr = freq + (freq_batched ? (size_t)b * nf : 0);
    for (int r = blockIdx.y; r < nf; r += gridDim.y) {
        const double w = omega(fr[r]);
        for (int q = 0; q < kWaveCols / kWaves; ++q) {
            const int c = wave_column(q);
            if (c >= ntau) continue;
            double zr, zi;
            trapz_pair(Y, ny, w, tau[c], zr, zi);
            if ((threadIdx.x & 63) == 0) {
                const size_t o = ((size_t)b * nf + r) * ntau + c;
                a_re[o] = zr;
                a_im[o] = zi;
            }
        }
    }
}

// ---------------------------------------------------------------------------------------------------------
// penalty matrices: orders 0..2 in one pass.  out matrices have leading dimension ld and the DRT block
// starts at (pad, pad) (pad = number of special parameters in the plan; 0 for the stand-alone API).
// ---------------------------------------------------------------------------------------------------------
__device__ __forceinline__ void penalty_funcs(double x_n, double x_m, double eps, double& f0, double& f1, double& f2) {
    const double a = eps * (x_m - x_n);
    const double a2 = a * a;
    const double e = exp(-(a2 / 2.0));
    const double rpi = sqrt(kPi / 2.0);
    f0 = rpi * (1.0 / eps) * e;
    f1 = (-rpi) * eps * (-1.0 + a2) * e;
    f2 = rpi * (eps * eps * eps) * (3.0 - 6.0 * a2 + a2 * a2) * e;
}

__global__ __launch_bounds__(kEntryBlock) void penalty_kernel(const double* __restrict__ ln_tau, int n, double eps, int toeplitz,
                               double* __restrict__ m0, double* __restrict__ m1, double* __restrict__ m2, int ld,
                               int pad) {
    const int j = blockIdx.x * blockDim.x + threadIdx.x;
    const int i = blockIdx.y;
    if (j >= n) return;
    double f0, f1, f2;
    if (toeplitz) {
        const int dd = i > j ? i - j : j - i;
        penalty_funcs(ln_tau[dd], ln_tau[0], eps, f0, f1, f2);   // c[d] = func(x_d, x_0)
    } else {
        penalty_funcs(ln_tau[i], ln_tau[j], eps, f0, f1, f2);
    }
    const size_t o = (size_t)(i + pad) * ld + (j + pad);
    m0[o] = f0;
    m1[o] = f1;
    m2[o] = f2;
}

// ---------------------------------------------------------------------------------------------------------
// Time response of the Gaussian basis to ideal galvanostatic steps (chrono / hybrid fits)
// ---------------------------------------------------------------------------------------------------------
// integrand (basis.py:616-618): phi(y) * (1 - exp(-t / (tau * e^y))); one wavefront integrates one (t, tau) pair
__device__ __forceinline__ double trapz_response(const YTablesLds& Y, int ny, double tau, double t) {
    const double *ys = Y.ys, *phis = Y.phis, *eys = Y.eys;
    double s = 0.0;
    for (int j = threadIdx.x & 63; j < ny - 1; j += 64) {
        const double f0 = phis[j] * (1.0 - exp(-t / (tau * eys[j])));
        const double f1 = phis[j + 1] * (1.0 - exp(-t / (tau * eys[j + 1])));
        const double d = ys[j + 1] - ys[j];
        s += d * (f1 + f0) / 2.0;
    }
    return wave_sum(s);
}

// expdecay step model (basis.py:619-637): the current rises as 1 - exp(-t / tau_rise); integrand
//   phi(y) * (1 - e^{-t/T} + tau_rise / (tau_rise - T) * (e^{-t/T} - e^{-t/tau_rise})),  T = e^y tau
__device__ __forceinline__ double trapz_response_expdecay(const YTablesLds& Y, int ny, double tau, double t, double tr) {
    const double *ys = Y.ys, *phis = Y.phis, *eys = Y.eys;
    const double etr = exp(-t / tr);
    auto f = [&](int j) {
        const double T = eys[j] * tau;
        const double eT = exp(-t / T);
        return phis[j] * ((1.0 - eT) + (tr / (tr - T)) * (eT - etr));
    };
    double s = 0.0;
    for (int j = threadIdx.x & 63; j < ny - 1; j += 64) {
        const double d = ys[j + 1] - ys[j];
        s += d * (f(j + 1) + f(j)) / 2.0;
    }
    return wave_sum(s);
}

// v[i] = trapz over y of the integrand at t/tau = td[i]; grid: ceil(ngrid / kWaves) blocks
__global__ __launch_bounds__(kWaveBlock) void response_lookup_kernel(double eps, int ngrid, int ny,
                                                                     const double* __restrict__ td, double* __restrict__ v) {
    extern __shared__ double sm[];
    const YTablesLds Y = stage_y_tables(sm, ny, eps);
    const int g = wave_entry();
    if (g >= ngrid) return;
    const double r = trapz_response(Y, ny, 1.0, td[g]);
    if ((threadIdx.x & 63) == 0) v[g] = r;
}

// The sum over steps that every response matrix is: layer k is 0 up to step k and entry(t - t_k, k) * size_k after it, a = the sum
// of the layers in step order, the layers kept where `layered` is given.  col: tau of the DRT builds, nu of the phasance build.
struct StepArgs {
    const double* times; int nt;
    const double* col; int ncol;
    const double* step_times; const double* step_sizes; int nsteps;
    double* a;                 // [nt][ncol]
    double* layered;           // [nsteps][nt][ncol] or null
};
// entry (r, c).  INCLUSIVE: the step's own sample belongs to it (t >= t_k, the potentiostatic form), otherwise t > t_k.  Every
// thread that shares the entry calls (a wavefront's lanes take part in entry()'s reduction); `writer` is the one that stores.
template <bool INCLUSIVE, class Entry>
__device__ __forceinline__ void step_sum(const StepArgs& s, int r, int c, bool writer, Entry entry) {
    const double t = s.times[r];
    double acc = 0.0;
    for (int k = 0; k < s.nsteps; ++k) {
        const double st = s.step_times[k];
        double val = 0.0;
        if (INCLUSIVE ? t >= st : t > st) val = entry(t - st, k) * s.step_sizes[k];
        if (s.layered && writer) s.layered[((size_t)k * s.nt + r) * s.ncol + c] = val;
        acc += val;
    }
    if (writer) s.a[(size_t)r * s.ncol + c] = acc;
}

// interp mode: entry = np.interp(ln((t - t_k)/tau), log_td, v).  lut3 = {log_td, v, slope}[ngrid] staged in LDS; block =
// kEntryBlock columns x rpb rows.
__global__ __launch_bounds__(kEntryBlock) void response_interp_kernel(StepArgs s, int ngrid, const double* __restrict__ lut3, int rpb) {
    extern __shared__ double sm[];
    const ResponseInterpLds L = response_interp_lds(sm, ngrid);
    for (int i = threadIdx.x; i < (int)lut_doubles(ngrid, 1); i += blockDim.x) L.xp[i] = lut3[i];      // the layout is lut3's own
    __syncthreads();
    const double* xp = L.xp; const double* fp = L.fp; const double* sl = L.sl;
    const double x0 = xp[0], inv_dx = (double)(ngrid - 1) / (xp[ngrid - 1] - xp[0]);
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= s.ncol) return;
    const double tc = s.col[c];
    const int r1 = min(s.nt, (int)(blockIdx.y + 1) * rpb);
    for (int r = blockIdx.y * rpb; r < r1; ++r)
        step_sum<false>(s, r, c, true, [&](double dt, int) { return np_interp(log(dt / tc), xp, fp, sl, ngrid, x0, inv_dx); });
}

// trapz mode and the expdecay step model (tau_rise[k] per step): one wavefront per entry, an ny-point trapezoid per step; grid
// (ceil(ntau / kWaveCols), rows)
template <bool EXPDECAY>
__global__ __launch_bounds__(kWaveBlock) void response_trapz_kernel(StepArgs s, const double* __restrict__ tau_rise, double eps, int ny) {
    extern __shared__ double sm[];
    const YTablesLds Y = stage_y_tables(sm, ny, eps);
    const bool writer = (threadIdx.x & 63) == 0;
    for (int r = blockIdx.y; r < s.nt; r += gridDim.y) {      // a long record has more rows than a grid has y
        for (int q = 0; q < kWaveCols / kWaves; ++q) {
            const int c = wave_column(q);
            if (c >= s.ncol) continue;
            step_sum<false>(s, r, c, writer, [&](double dt, int k) {
                if constexpr (EXPDECAY) return trapz_response_expdecay(Y, ny, s.col[c], dt, tau_rise[k]);
                else return trapz_response(Y, ny, s.col[c], dt);
            });
        }
    }
}

// One thread per column, rows strided over gridDim.y.  Column: kBlock threads per block, the step rule, and of(value of the
// column) -> what the column needs once, callable as entry(dt).
template <class Column>
__global__ __launch_bounds__(Column::kBlock) void step_column_kernel(StepArgs s, Column col) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= s.ncol) return;
    const auto entry = col.of(s.col[c]);
    for (int r = blockIdx.y; r < s.nt; r += gridDim.y)
        step_sum<Column::kInclusive>(s, r, c, true, [&](double dt, int) { return entry(dt); });
}

// potentiostatic form (mat1d.py:114-118): the basis is a delta function, the current after a voltage step decays as
// exp(-(t - t_k) / tau) from the step on (unit_step: t >= t_k); rows before the step are 0 (the reference's nan_to_num)
struct PotColumn {
    static constexpr int kBlock = kEntryBlock;
    static constexpr bool kInclusive = true;
    struct Entry {
        double tc;
        __device__ __forceinline__ double operator()(double dt) const { return exp(-dt / tc); }
    };
    __device__ __forceinline__ Entry of(double tau) const { return Entry{tau}; }
};

// ---------------------------------------------------------------------------------------------------------
// EIS variance-estimation matrix: one kRowBlock-thread block per row of the (2nf x 2nf) matrix
// ---------------------------------------------------------------------------------------------------------
// row / its sum (s: this thread's part of the sum, red: one double per wavefront of the block)
__device__ __forceinline__ void normalise_row(double* row, int len, double s, double* red) {
    static_assert(kRowBlock / 64 == 4, "the sum below adds four wavefronts' parts");
    s = wave_sum(s);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
    __syncthreads();
    const double tot = (red[0] + red[1]) + (red[2] + red[3]);
    for (int j = threadIdx.x; j < len; j += blockDim.x) row[j] /= tot;
}

__global__ __launch_bounds__(kRowBlock) void eis_vmm_kernel(const double* __restrict__ freq, int nf, double ve, double cor,
                                                            int uniform, double* __restrict__ vmm) {
    __shared__ double red[kRowBlock / 64];
    const int i = blockIdx.x;          // row in [0, 2nf)
    const int ih = i >= nf ? i - nf : i;
    const int m = 2 * nf;
    const double lfi = log(freq[ih]);
    double s = 0.0;
    for (int j = threadIdx.x; j < m; j += blockDim.x) {
        const int jh = j >= nf ? j - nf : j;
        double v = 1.0;
        if (!uniform) {
            const double dd = ve * (lfi - log(freq[jh]));
            v = exp(-(dd * dd));
        }
        if ((i >= nf) != (j >= nf)) v = v * cor;
        vmm[(size_t)i * m + j] = v;
        s += v;
    }
    normalise_row(vmm + (size_t)i * m, m, s, red);
}

// Chrono variance-estimation matrix: one block per row.  tt = transformed sample times, seg[nseg+1] =
// sample index bounds of the step segments (no correlation across segments), rows normalised to sum 1.
__global__ __launch_bounds__(kRowBlock) void chrono_vmm_kernel(const double* __restrict__ tt, int nt,
                                                               const int* __restrict__ seg, int nseg, double eps, int uniform,
                                                               double* __restrict__ vmm) {
    __shared__ double red[kRowBlock / 64];
    const int i = blockIdx.x;
    int a = 0, b = nt;
    if (!uniform) {
        for (int k = 0; k < nseg; ++k)
            if (i >= seg[k] && i < seg[k + 1]) { a = seg[k]; b = seg[k + 1]; }
    }
    const double ti = tt[i];
    double s = 0.0;
    for (int j = threadIdx.x; j < nt; j += blockDim.x) {
        double v = 0.0;
        if (uniform) v = 1.0;
        else if (j >= a && j < b) { const double dd = eps * (ti - tt[j]); v = exp(-(dd * dd)); }
        vmm[(size_t)i * nt + j] = v;
        s += v;
    }
    normalise_row(vmm + (size_t)i * nt, nt, s, red);
}

// ---------------------------------------------------------------------------------------------------------
// Distribution of phasances (gaussian nu basis, normalize=False)
// ---------------------------------------------------------------------------------------------------------
// erf(x + i y) by Abramowitz & Stegun 7.1.29 (|y| <= ~1: here y = -pi / (4 eps)); absolute error ~1e-16
__device__ __forceinline__ void cerf(double x, double y, double& re, double& im) {
    const double PI = kPi;
    const double ex2 = exp(-x * x);
    re = erf(x);
    const double s = sin(x * y), xy2 = 2.0 * x * y;
    const double c2 = cos(xy2), s2 = sin(xy2);
    if (x != 0.0) { re += ex2 * 2.0 * s * s / (2.0 * PI * x); im = ex2 * s2 / (2.0 * PI * x); }
    else im = ex2 * y / PI;
    double sre = 0.0, sim = 0.0;
    for (int n = 1; n <= 32; ++n) {
        const double dn = (double)n;
        const double en = exp(-0.25 * dn * dn) / (dn * dn + 4.0 * x * x);
        const double ch = cosh(dn * y), sh = sinh(dn * y);
        sre += en * (2.0 * x - 2.0 * x * ch * c2 + dn * sh * s2);
        sim += en * (2.0 * x * ch * s2 + dn * sh * c2);
    }
    re += 2.0 / PI * ex2 * sre;
    im += 2.0 / PI * ex2 * sim;
}

// zm[r][c] = F(b) - F(a),  F(nu) = sqrt(pi)/2 (j w)^nu_m / eps * (j w)^(ln(j w) / 4 eps^2) * erf(eps (nu - nu_m) - ln(j w) / 2 eps),
// (a, b) = (min(0, sgn nu_m), max(0, sgn nu_m))   (phasance.py:19-33, 62-82)
__global__ __launch_bounds__(kPhasorBlock) void phasor_z_kernel(const double* __restrict__ freq, int nf, const double* __restrict__ nu,
                                                                int nnu, double eps, double* __restrict__ zre, double* __restrict__ zim) {
    const int c = blockIdx.x * blockDim.x + threadIdx.x;
    if (c >= nnu) return;
    const double PI = kPi;
    const double num = nu[c];
    const double sg = (num > 0.0) ? 1.0 : ((num < 0.0) ? -1.0 : 0.0);
    const double a = fmin(0.0, sg), b = fmax(0.0, sg);
    for (int r = blockIdx.y; r < nf; r += gridDim.y) {
        const double lw = log(2.0 * PI * freq[r]);      // (2 pi) f as the reference forms it here, not omega()'s (2 f) pi
        // prefactor exp(nu_m L + L^2 / (4 eps^2)), L = ln(j w) = lw + j pi/2
        const double q = 1.0 / (4.0 * eps * eps);
        const double e_re = num * lw + (lw * lw - 0.25 * PI * PI) * q;
        const double e_im = num * 0.5 * PI + PI * lw * q;
        const double mag = 0.5 * sqrt(PI) / eps * exp(e_re);
        const double p_re = mag * cos(e_im), p_im = mag * sin(e_im);
        const double y = -PI / (4.0 * eps), xoff = -lw / (2.0 * eps);
        double br, bi, ar, ai;
        cerf(eps * (b - num) + xoff, y, br, bi);
        cerf(eps * (a - num) + xoff, y, ar, ai);
        const double dr = br - ar, di = bi - ai;
        zre[(size_t)r * nnu + c] = p_re * dr - p_im * di;
        zim[(size_t)r * nnu + c] = p_re * di + p_im * dr;
    }
}

// rm_layered[k][r][c] = size_k (G(b) - G(a)) for t_r > t_k, G(nu) = sqrt(pi)/2 dt^-nu_m / Gamma(1 - nu_m) / eps *
// dt^(ln dt / 4 eps^2) * erf(eps (nu - nu_m) + ln dt / 2 eps), dt = t_r - t_k; rm = sum over k  (phasance.py:38-52, 121-144)
struct PhasorVColumn {
    static constexpr int kBlock = kPhasorBlock;
    static constexpr bool kInclusive = false;
    double eps;
    struct Entry {
        double eps, num, a, b, gin;      // gin = 1 / Gamma(1 - nu_m), once per column
        __device__ __forceinline__ double operator()(double dt) const {
            const double ldt = log(dt);
            const double pre = 0.5 * sqrt(kPi) * (exp(-num * ldt) * gin) / eps * exp(ldt * ldt / (4.0 * eps * eps));
            const double xo = ldt / (2.0 * eps);
            return pre * erf(eps * (b - num) + xo) - pre * erf(eps * (a - num) + xo);
        }
    };
    __device__ __forceinline__ Entry of(double num) const {
        const double sg = (num > 0.0) ? 1.0 : ((num < 0.0) ? -1.0 : 0.0);
        return Entry{eps, num, fmin(0.0, sg), fmax(0.0, sg), 1.0 / tgamma(1.0 - num)};
    }
};

// ---------------------------------------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------------------------------------
// rows on gridDim.y: as many as a grid has, the kernels stride over the rest
static inline int grid_rows(int rows) { return rows < kGridDimMax ? rows : kGridDimMax; }
static inline size_t y_bytes(int ny) { return y_tables_lds(nullptr, ny).bytes; }

void launch_lookup(hipStream_t st, double eps, int ngrid, int ny, const double* wt_re, const double* wt_im,
                   double* z_re, double* z_im) {
    hipLaunchKernelGGL(lookup_kernel, dim3(blocks_of(2 * ngrid, kWaves)), dim3(kWaveBlock), y_bytes(ny), st, eps, ngrid, ny, wt_re,
                       wt_im, z_re, z_im);
}

void launch_lut_slopes(hipStream_t st, double* base, int ngrid, int ntables) {
    for (int k = 0; k < ntables; ++k) {
        const LutPart<double> T = lut_part(base, ngrid, k);
        hipLaunchKernelGGL(slopes_kernel, dim3(blocks_of(ngrid, kEntryBlock)), dim3(kEntryBlock), 0, st, ngrid, T.x, T.f, T.slope);
    }
}

// What launch_impedance_matrix keeps in its scratch.  Toeplitz: the first column and row of both parts, cr = {c_re[nf], r_re[ntau],
// c_im[nf], r_im[ntau]}.  General interp: ln(omega) of every frequency row, then ln(tau).  General trapz: nothing.
static inline size_t freq_rows(int B, int freq_batched, int nf) { return (size_t)(freq_batched ? B : 1) * nf; }
size_t impedance_scratch_doubles(int B, int freq_batched, int nf, int ntau, int mode, int toeplitz) {
    if (toeplitz) return 2 * ((size_t)nf + ntau);
    return mode == HIPDRT_MODE_INTERP ? freq_rows(B, freq_batched, nf) + ntau : 0;
}

void launch_impedance_matrix(hipStream_t st, int B, int freq_batched, const double* freq, int nf, const double* tau,
                             int ntau, int mode, int toeplitz, double eps, int ngrid, const double* lut6, int ny,
                             double* a_re, double* a_im, double* scratch) {
    if (toeplitz) {
        const int tot = nf + ntau;
        if (mode == HIPDRT_MODE_INTERP)
            hipLaunchKernelGGL(toeplitz_cr_interp_kernel, dim3(blocks_of(tot, kEntryBlock)), dim3(kEntryBlock), 0, st, freq, nf, tau,
                               ntau, ngrid, lut6, scratch);
        else
            hipLaunchKernelGGL(toeplitz_cr_trapz_kernel, dim3(blocks_of(tot, kWaves)), dim3(kWaveBlock), y_bytes(ny), st,
                               freq, nf, tau, ntau, eps, ny, scratch);
        const int zb = B < 64 ? B : 64;
        hipLaunchKernelGGL(toeplitz_fill_kernel, dim3(blocks_of(ntau, kEntryBlock), grid_rows(nf), zb), dim3(kEntryBlock), 0, st, B,
                           nf, ntau, scratch, a_re, a_im);
        return;
    }
    if (mode == HIPDRT_MODE_INTERP) {
        const int count_f = (int)freq_rows(B, freq_batched, nf);
        double *lw = scratch, *lt = scratch + count_f;
        const int cnt = count_f > ntau ? count_f : ntau;
        hipLaunchKernelGGL(log_grid_kernel, dim3(blocks_of(cnt, kEntryBlock)), dim3(kEntryBlock), 0, st, count_f, freq, ntau, tau, lw, lt);
        int tpr, rpb;
        size_t lds;
        impedance_interp_form(B, nf, ntau, ngrid, &tpr, &rpb, &lds);
        hipLaunchKernelGGL(impedance_interp_kernel, dim3(blocks_of(nf, rpb), B), dim3(kInterpBlock), lds, st,
                           freq_batched, lw, nf, lt, ntau, ngrid, lut6, rpb, tpr, a_re, a_im);
    } else {
        hipLaunchKernelGGL(impedance_trapz_kernel, dim3(blocks_of(ntau, kWaveCols), grid_rows(nf), B), dim3(kWaveBlock), y_bytes(ny),
                           st, freq_batched, freq, nf, tau, ntau, eps, ny, a_re, a_im);
    }
}

void impedance_interp_form(int B, int nf, int ntau, int ngrid, int* tpr_out, int* rpb_out, size_t* lds_bytes) {
    int tpr = ((ntau + 1) / 2 + 63) / 64 * 64;           // threads per row (two columns each)
    if (tpr > kInterpBlock) tpr = kInterpBlock;
    while (kInterpBlock % tpr) tpr += 64;                 // 64,128,256,512,1024
    int rpb = kInterpMaxRows;
    while (rpb > kInterpMinRows && (long long)B * ((nf + rpb - 1) / rpb) < 1024) rpb /= 2;   // enough workgroups for 256 CUs
    // a long table leaves fewer rows' ln(omega) beside it: every ngrid the entry points accept fits at kInterpMinRows
    while (rpb > kInterpMinRows && impedance_interp_lds(nullptr, ngrid, rpb).bytes > kLdsLimit) rpb /= 2;
    *tpr_out = tpr;
    *rpb_out = rpb;
    *lds_bytes = impedance_interp_lds(nullptr, ngrid, rpb).bytes;
}

void launch_phasor_z(hipStream_t st, const double* freq, int nf, const double* nu, int nnu, double eps, double* zre,
                     double* zim) {
    hipLaunchKernelGGL(phasor_z_kernel, dim3(blocks_of(nnu, kPhasorBlock), grid_rows(nf)), dim3(kPhasorBlock), 0, st, freq, nf, nu,
                       nnu, eps, zre, zim);
}

template <class Column>
static void launch_step_columns(hipStream_t st, const StepArgs& s, Column col) {
    hipLaunchKernelGGL(step_column_kernel<Column>, dim3(blocks_of(s.ncol, Column::kBlock), grid_rows(s.nt)), dim3(Column::kBlock), 0,
                       st, s, col);
}

void launch_phasor_v(hipStream_t st, const double* times, int nt, const double* nu, int nnu, double eps,
                     const double* step_times, const double* step_sizes, int nsteps, double* rm, double* layered) {
    launch_step_columns(st, StepArgs{times, nt, nu, nnu, step_times, step_sizes, nsteps, rm, layered}, PhasorVColumn{eps});
}

void launch_chrono_vmm(hipStream_t st, const double* tt, int nt, const int* seg, int nseg, double eps, int uniform,
                       double* vmm) {
    hipLaunchKernelGGL(chrono_vmm_kernel, dim3(nt), dim3(kRowBlock), 0, st, tt, nt, seg, nseg, eps, uniform, vmm);
}

void launch_response_lookup(hipStream_t st, double eps, int ngrid, int ny, const double* td, double* v) {
    hipLaunchKernelGGL(response_lookup_kernel, dim3(blocks_of(ngrid, kWaves)), dim3(kWaveBlock), y_bytes(ny), st, eps, ngrid, ny,
                       td, v);
}

template <bool EXPDECAY>
static void launch_response_trapz(hipStream_t st, const StepArgs& s, const double* tau_rise, double eps, int ny) {
    hipLaunchKernelGGL(response_trapz_kernel<EXPDECAY>, dim3(blocks_of(s.ncol, kWaveCols), grid_rows(s.nt)), dim3(kWaveBlock),
                       y_bytes(ny), st, s, tau_rise, eps, ny);
}

void launch_response_matrix(hipStream_t st, const double* times, int nt, const double* tau, int ntau,
                            const double* step_times, const double* step_sizes, int nsteps, int mode, double eps,
                            int ngrid, const double* lut3, int ny, double* a, double* layered) {
    const StepArgs s{times, nt, tau, ntau, step_times, step_sizes, nsteps, a, layered};
    if (mode == HIPDRT_MODE_INTERP) {
        const int bx = blocks_of(ntau, kEntryBlock);
        int rpb = 32;
        while (rpb > 1 && (long long)bx * blocks_of(nt, rpb) < 1024) rpb /= 2;
        hipLaunchKernelGGL(response_interp_kernel, dim3(bx, blocks_of(nt, rpb)), dim3(kEntryBlock),
                           response_interp_lds(nullptr, ngrid).bytes, st, s, ngrid, lut3, rpb);
    } else {
        launch_response_trapz<false>(st, s, nullptr, eps, ny);
    }
}

void launch_response_variant(hipStream_t st, const double* times, int nt, const double* tau, int ntau,
                             const double* step_times, const double* step_sizes, const double* tau_rise, int nsteps,
                             int variant, double eps, int ny, double* a, double* layered) {
    const StepArgs s{times, nt, tau, ntau, step_times, step_sizes, nsteps, a, layered};
    if (variant == HIPDRT_RESPONSE_POT) launch_step_columns(st, s, PotColumn{});
    else launch_response_trapz<true>(st, s, tau_rise, eps, ny);
}

void launch_penalty(hipStream_t st, const double* ln_tau, int n, double eps, int toeplitz, double* m0, double* m1,
                    double* m2, int ld, int pad) {
    hipLaunchKernelGGL(penalty_kernel, dim3(blocks_of(n, kEntryBlock), n), dim3(kEntryBlock), 0, st, ln_tau, n, eps, toeplitz, m0,
                       m1, m2, ld, pad);
}

void launch_eis_vmm(hipStream_t st, const double* freq, int nf, double vmm_eps, double reim_cor, int uniform,
                    double* vmm) {
    hipLaunchKernelGGL(eis_vmm_kernel, dim3(2 * nf), dim3(kRowBlock), 0, st, freq, nf, vmm_eps, reim_cor, uniform, vmm);
}

// ---------------------------------------------------------------------------------------------------------
// filters.nonuniform_gaussian_filter1d (hybdrt/filters/_filters.py:261-343), order 0, mode 'reflect', empty=False: the
// anti-aliasing filter of the chrono down-sampling (preprocessing.filter_chrono_signal, 507-572).  Every sample has its own
// sigma; the reference evaluates scipy's gaussian_filter1d at log-spaced sigma nodes and blends the node outputs with
// triangular weights in log sigma.  Here one thread per sample evaluates only the (at most two) nodes that carry weight,
// with scipy's symmetric correlation order  y[i] w0 + sum_j (y[i-j] + y[i+j]) w_j  and its 'reflect' boundary
// (d c b a | a b c d | d c b a).  weights[woff[k] + j], j = 0..radius[k], are the normalised kernel halves (host: numpy,
// exactly as scipy builds them); a node with radius < 0 returns the input (sigma below min_sigma).
// seg[s], seg[s+1] bound the step segments: the reference filters every segment separately.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void nonuniform_gauss_kernel(const double* __restrict__ y, int n,
                                                               const double* __restrict__ sigma,
                                                               const int* __restrict__ seg_of, const int* __restrict__ seg,
                                                               const double* __restrict__ nodes, int K,
                                                               const double* __restrict__ node_delta,
                                                               const double* __restrict__ weights,
                                                               const int* __restrict__ woff, const int* __restrict__ radius,
                                                               double* __restrict__ out) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int s = seg_of[i];
    if (s < 0) { out[i] = y[i]; return; }                 // segment without filtering (all sigma zero)
    const int a = seg[s], len = seg[s + 1] - a, li = i - a;
    const double sg = sigma[i];
    const int kb = s * K;                                  // nodes are per segment
    double acc = 0.0;
    for (int k = 0; k < K; ++k) {
        const double node = nodes[kb + k];
        if (!(node > 0.0)) continue;                       // unused slot
        double nw = fabs(log(sg / node)) / node_delta[s];
        if (nw >= 1.0) nw = 1.0;
        nw = 1.0 - nw;
        if (nw == 0.0) continue;                           // exact zero: adds nothing in the reference either
        double v;
        const int r = radius[kb + k];
        if (r < 0) {
            v = y[i];
        } else {
            const double* w = weights + woff[kb + k];
            v = y[i] * w[0];
            for (int j = 1; j <= r; ++j) {
                int lo = li - j, hi = li + j;
                // scipy 'reflect': period 2 len, mirrored about the half-sample edges
                if (lo < 0) { lo = -lo - 1; if (lo >= len) { lo %= 2 * len; if (lo >= len) lo = 2 * len - 1 - lo; } }
                if (hi >= len) { hi %= 2 * len; if (hi >= len) hi = 2 * len - 1 - hi; }
                v += (y[a + lo] + y[a + hi]) * w[j];
            }
        }
        acc += v * nw;
    }
    out[i] = acc;
}

void launch_nonuniform_gauss(hipStream_t st, const double* y, int n, const double* sigma, const int* seg_of, const int* seg,
                             const double* nodes, int K, const double* node_delta, const double* weights, const int* woff,
                             const int* radius, double* out) {
    hipLaunchKernelGGL(nonuniform_gauss_kernel, dim3((n + 255) / 256), dim3(256), 0, st, y, n, sigma, seg_of, seg, nodes, K,
                       node_delta, weights, woff, radius, out);
}

// ---------------------------------------------------------------------------------------------------------
// basis.construct_func_eval_matrix (hybdrt/matrices/basis.py:488-514) with get_basis_func_derivative (218-228), gaussian basis:
// out[i * ld + j] = fac * phi^(order)(e_i - b_j), evaluated in numpy's order of operations -- y = e - b, (eps y)^2, exp, then
// ((-2 eps^2) y) phi or ((-2 eps^2) + (4 eps^4) y^2) phi with the two constants formed on the host as Python forms them.
// ---------------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void func_eval_kernel(const double* __restrict__ basis, int nb, const double* __restrict__ ev,
                                                        int ne, double eps, int order, double c1, double c2, double fac,
                                                        double* __restrict__ out, int ld) {
    const int j = blockIdx.x * 64 + (threadIdx.x & 63), i = blockIdx.y * 4 + (threadIdx.x >> 6);
    if (i >= ne || j >= nb) return;
    const double y = ev[i] - basis[j];
    const double ey = eps * y;
    const double phi = exp(-(ey * ey));
    double v = phi;
    if (order == 1) v = (c1 * y) * phi;
    else if (order == 2) v = (c1 + c2 * (y * y)) * phi;
    out[(size_t)i * ld + j] = fac * v;
}

void launch_func_eval(hipStream_t st, const double* basis, int nb, const double* ev, int ne, double eps, int order, double c1,
                      double c2, double fac, double* out, int ld) {
    hipLaunchKernelGGL(func_eval_kernel, dim3((nb + 63) / 64, (ne + 3) / 4), dim3(256), 0, st, basis, nb, ev, ne, eps, order, c1,
                       c2, fac, out, ld);
}

}  // namespace hipdrt
