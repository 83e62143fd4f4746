// Model evaluation for a fitted batch (hybdrt/models/drt1d.py:2965-3061 predict_drt, 3209-3231 predict_drt_ci, 3500-3542
// predict_z, 3552-3584 the resistances): every prediction is "rows of an evaluation matrix applied to each spectrum's x",
//
//     Y[b][i] = scale_b * sum_j E[i][j] * x[b][col_offset + j]            (a B x r x K product, x resident on the device)
//
// followed by a per-element epilogue (credible band, impedance assembly; for a prepared plan the voltage response, the impedance
// with every special term, the distribution of phasances and its posterior: hipdrt/models/response.py).  FP64 only (SURVEY.md
// fact 4); the contraction runs on v_mfma_f64_16x16x4_f64.  hipdrt/models/predict.py is the same arithmetic in numpy.
//
// Layout.  A 256-thread workgroup (4 wavefronts) owns 32 spectra x 64 evaluation rows.  Per 64-wide slab of k it stages
// x[32][64] and E[64][64] through LDS (both k-contiguous, leading dimension 68: the operand reads below then hit every bank
// pair exactly twice per 64 lanes, the minimum for 8-byte words).  Wavefront w owns evaluation rows 16 w .. 16 w + 15 and two
// accumulators (spectra 0-15 and 16-31), so the two MFMA chains of a wavefront are independent.  MFMA operands: A[l & 15][l >> 4] =
// x (rows = spectra), B[l >> 4][l & 15] = E' (columns = evaluation rows); C/D: col = lane & 15, row = (lane >> 4) + 4 reg.
//
// Accumulation order.  Every output element has ONE accumulator and receives its k-blocks of four in ascending order, from k = 0,
// whatever the batch size and wherever the spectrum sits in the batch or the tile (no split-K, no atomics; the MFMA's internal
// order over its four k is a property of the instruction).  So a spectrum predicted alone and the same spectrum inside a batch
// give the same bits.  Tails in B, r and K are staged as zeros; nothing outside the arrays is read, nothing outside
// out[B][r] is written.  x + col_offset need not be 16-byte aligned: the slab is fetched with 8-byte loads.
#include "common.hpp"

namespace hipdrt {

typedef double v4d __attribute__((ext_vector_type(4)));

constexpr int PB = 32, PR = 64, PK = 64, PLD = 68;

__global__ __launch_bounds__(256) void apply_rows_kernel(int B, int K, const double* __restrict__ X, long long ldx,
                                                         int col_offset, int r, const double* __restrict__ E, int lde,
                                                         const double* __restrict__ scale, const int* __restrict__ fit_status,
                                                         double* __restrict__ out, long long ldo) {
    __shared__ double sX[PB * PLD];
    __shared__ double sE[PR * PLD];
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int b0 = blockIdx.x * PB, i0 = blockIdx.y * PR;
    const int srow = tid >> 4, skc = tid & 15;                  // staging map: 16 lanes along k (128 contiguous bytes per row)
    const bool live = i0 + wv * 16 < r;                         // (a wavefront whose 16 evaluation rows are all padding only stages)
    v4d acc0 = (v4d){0.0, 0.0, 0.0, 0.0}, acc1 = (v4d){0.0, 0.0, 0.0, 0.0};
    // slab k0 + PK is fetched (global -> registers) while slab k0 is multiplied out of LDS; tails come in as zeros
    double vx[(PB / 16) * (PK / 16)], ve[(PR / 16) * (PK / 16)];
    auto fetch = [&](int k0) {
#pragma unroll
        for (int rr = 0; rr < PB / 16; ++rr) {
            const int b = b0 + srow + 16 * rr;
#pragma unroll
            for (int j = 0; j < PK / 16; ++j) {
                const int k = k0 + skc + 16 * j;
                vx[rr * (PK / 16) + j] = (b < B && k < K) ? X[(size_t)b * ldx + col_offset + k] : 0.0;
            }
        }
#pragma unroll
        for (int rr = 0; rr < PR / 16; ++rr) {
            const int i = i0 + srow + 16 * rr;
#pragma unroll
            for (int j = 0; j < PK / 16; ++j) {
                const int k = k0 + skc + 16 * j;
                ve[rr * (PK / 16) + j] = (i < r && k < K) ? E[(size_t)i * lde + k] : 0.0;
            }
        }
    };
    fetch(0);
    for (int k0 = 0; k0 < K; k0 += PK) {
        __syncthreads();                                        // previous slab fully consumed
#pragma unroll
        for (int rr = 0; rr < PB / 16; ++rr)
#pragma unroll
            for (int j = 0; j < PK / 16; ++j) sX[(srow + 16 * rr) * PLD + skc + 16 * j] = vx[rr * (PK / 16) + j];
#pragma unroll
        for (int rr = 0; rr < PR / 16; ++rr)
#pragma unroll
            for (int j = 0; j < PK / 16; ++j) sE[(srow + 16 * rr) * PLD + skc + 16 * j] = ve[rr * (PK / 16) + j];
        __syncthreads();
        if (k0 + PK < K) fetch(k0 + PK);
        if (live) {
            const int left = K - k0;
            const int kend = left >= PK ? PK : (left + 3) & ~3;  // whole blocks of four; the zeros past K are staged above
            for (int kk = 0; kk < kend; kk += 4) {
                const int kr = kk + (lane >> 4);
                const double a0 = sX[(lane & 15) * PLD + kr];
                const double a1 = sX[(16 + (lane & 15)) * PLD + kr];
                const double e = sE[(wv * 16 + (lane & 15)) * PLD + kr];
                acc0 = __builtin_amdgcn_mfma_f64_16x16x4f64(a0, e, acc0, 0, 0, 0);
                acc1 = __builtin_amdgcn_mfma_f64_16x16x4f64(a1, e, acc1, 0, 0, 0);
            }
        }
    }
    const int i = i0 + wv * 16 + (lane & 15);
    if (!live || i >= r) return;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const v4d acc = h ? acc1 : acc0;
#pragma unroll
        for (int reg = 0; reg < 4; ++reg) {
            const int b = b0 + 16 * h + (lane >> 4) + 4 * reg;
            if (b >= B) continue;
            double v = acc[reg];
            if (scale) v = scale[b] * v;
            if (fit_status && fit_status[b] < 0) v = NAN;
            out[(size_t)b * ldo + i] = v;
        }
    }
}

void launch_apply_rows(hipStream_t st, int B, int K, const double* X, long long ldx, int col_offset, int r, const double* E,
                       int lde, const double* scale, const int* fit_status, double* out, long long ldo) {
    hipLaunchKernelGGL(apply_rows_kernel, dim3((B + PB - 1) / PB, (r + PR - 1) / PR), dim3(256), 0, st, B, K, X, ldx, col_offset,
                       r, E, lde, scale, fit_status, out, ldo);
}

// Signed coefficient sums of every spectrum's DRT block (get_drt_params, drt1d.py:2965-2987, inside predict_r_p, 3552-3571):
// one wavefront per spectrum, a fixed lane-strided order and a fixed shuffle tree, so the sums do not depend on the batch either.
// sum_x[b] = sum_j s_j, sum_abs[b] = sum_j |s_j| with s = x+ (sign 1), -x- (sign -1), x+ - x- (sign 0); copies = 1: s = x.
__global__ __launch_bounds__(64) void drt_sums_kernel(int B, const double* __restrict__ X, long long ldx, int col_offset, int nb,
                                                      int copies, int sign, double* __restrict__ sum_x,
                                                      double* __restrict__ sum_abs) {
    const int b = blockIdx.x, lane = threadIdx.x;
    const double* x = X + (size_t)b * ldx + col_offset;
    double s = 0.0, a = 0.0;
    for (int j = lane; j < nb; j += 64) {
        double v;
        if (copies == 1 || sign == 1) v = x[j];
        else if (sign == -1) v = -x[nb + j];
        else v = x[j] - x[nb + j];
        s += v; a += fabs(v);
    }
    for (int o = 32; o > 0; o >>= 1) { s += __shfl_down(s, o); a += __shfl_down(a, o); }
    if (lane == 0) { sum_x[b] = s; sum_abs[b] = a; }
}

void launch_drt_sums(hipStream_t st, int B, const double* X, long long ldx, int col_offset, int nb, int copies, int sign,
                     double* sum_x, double* sum_abs) {
    hipLaunchKernelGGL(drt_sums_kernel, dim3(B), dim3(64), 0, st, B, X, ldx, col_offset, nb, copies, sign, sum_x, sum_abs);
}

// Per-spectrum scalars from the sums: r_p = (sum * area) * cs (predict_r_p in data units), and the factor predict_drt applies to
// E x: cs, or cs / r_p with normalize (get_drt_norm, drt1d.py:3020-3031; abs_norm takes sum |x|).  Any output may be null.
__global__ void drt_scalars_kernel(int B, const double* __restrict__ sum_x, const double* __restrict__ sum_abs,
                                   const double* __restrict__ cs, double area, int normalize, int absolute,
                                   const double* __restrict__ X, long long ldx, int idx_rinf, double* __restrict__ r_p,
                                   double* __restrict__ r_inf, double* __restrict__ r_tot, double* __restrict__ norm,
                                   double* __restrict__ scale) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double c = cs[b];
    const double rp = ((absolute ? sum_abs[b] : sum_x[b]) * area) * c;
    const double rp_signed = (sum_x[b] * area) * c;
    const double ri = idx_rinf >= 0 ? X[(size_t)b * ldx + idx_rinf] * c : 0.0;
    if (r_p) r_p[b] = rp;
    if (r_inf) r_inf[b] = ri;
    if (r_tot) r_tot[b] = ri + rp_signed;                      // predict_r_tot adds predict_r_p() with its defaults
    if (norm) norm[b] = normalize ? rp : 1.0;
    if (scale) scale[b] = normalize ? c / rp : c;
}

void launch_drt_scalars(hipStream_t st, int B, const double* sum_x, const double* sum_abs, const double* cs, double area,
                        int normalize, int absolute, const double* X, long long ldx, int idx_rinf, double* r_p, double* r_inf,
                        double* r_tot, double* norm, double* scale) {
    hipLaunchKernelGGL(drt_scalars_kernel, dim3((B + 255) / 256), dim3(256), 0, st, B, sum_x, sum_abs, cs, area, normalize,
                       absolute, X, ldx, idx_rinf, r_p, r_inf, r_tot, norm, scale);
}

// predict_drt_ci (drt1d.py:3209-3231): sigma = sqrt(diag(E cov E') / norm^2) with cov = inv(P) cs^2 (estimate_param_cov,
// 4116-4138), lo = mu + s_lo sigma, hi = mu + s_hi sigma.  var[b][i] = e_i' inv(P_b) e_i comes from the variance kernel
// (qp_resident.hpp: cov_kernel_resident); a P that is not positive definite (var_status != 0) or a failed fit gives NaN rows.
__global__ void drt_band_kernel(int B, int r, const double* __restrict__ mu, const double* __restrict__ var, long long ldv,
                                const double* __restrict__ cs, const double* __restrict__ norm, double s_lo, double s_hi,
                                const int* __restrict__ var_status, const int* __restrict__ fit_status, double* __restrict__ lo,
                                double* __restrict__ hi) {
    const int i = blockIdx.y * blockDim.x + threadIdx.x, b = blockIdx.x;
    if (i >= r) return;
    const size_t o = (size_t)b * r + i;
    double l = NAN, h = NAN;
    if (var_status[b] == 0 && fit_status[b] >= 0) {
        double v = var[(size_t)b * ldv + i] * (cs[b] * cs[b]);
        if (norm) v = v / (norm[b] * norm[b]);
        const double sg = sqrt(v), m = mu[o];
        l = m + s_lo * sg;
        h = m + s_hi * sg;
    }
    if (lo) lo[o] = l;
    if (hi) hi[o] = h;
}

void launch_drt_band(hipStream_t st, int B, int r, const double* mu, const double* var, long long ldv, const double* cs,
                     const double* norm, double s_lo, double s_hi, const int* var_status, const int* fit_status, double* lo,
                     double* hi) {
    hipLaunchKernelGGL(drt_band_kernel, dim3(B, (r + 255) / 256), dim3(256), 0, st, B, r, mu, var, ldv, cs, norm, s_lo, s_hi,
                       var_status, fit_status, lo, hi);
}

// predict_z (drt1d.py:3500-3542) from y[b] = cs_b [A'; A''] x_b: Z = y' + j y'' + R_inf + j 2 pi f L in data units, every term
// switchable (mask bit 0 DRT, 1 ohmic, 2 inductance).  R_inf and L are rescaled like extract_qphb_parameters (6228-6289); the
// inductive term is formed as numpy forms `induc * 2j * np.pi * frequencies`.  y may be null when the DRT term is off.
__global__ void z_assemble_kernel(int B, int nf, const double* __restrict__ y, const double* __restrict__ X, long long ldx,
                                  int idx_rinf, int idx_induc, const double* __restrict__ cs, double inductance_scale,
                                  const double* __restrict__ freq, int mask, const int* __restrict__ fit_status,
                                  double* __restrict__ z_re, double* __restrict__ z_im) {
    const int i = blockIdx.y * blockDim.x + threadIdx.x, b = blockIdx.x;
    if (i >= nf) return;
    const double c = cs[b];
    double re = 0.0, im = 0.0;
    if (mask & 1) { re = y[(size_t)b * 2 * nf + i]; im = y[(size_t)b * 2 * nf + nf + i]; }
    if ((mask & 2) && idx_rinf >= 0) re += X[(size_t)b * ldx + idx_rinf] * c;
    if ((mask & 4) && idx_induc >= 0) {
        const double induc = X[(size_t)b * ldx + idx_induc] * (c * inductance_scale);
        im += ((induc * 2.0) * 3.141592653589793) * freq[i];
    }
    if (fit_status[b] < 0) { re = NAN; im = NAN; }
    z_re[(size_t)b * nf + i] = re;
    z_im[(size_t)b * nf + i] = im;
}

void launch_z_assemble(hipStream_t st, int B, int nf, const double* y, const double* X, long long ldx, int idx_rinf,
                       int idx_induc, const double* cs, double inductance_scale, const double* freq, int mask,
                       const int* fit_status, double* z_re, double* z_im) {
    hipLaunchKernelGGL(z_assemble_kernel, dim3(B, (nf + 255) / 256), dim3(256), 0, st, B, nf, y, X, ldx, idx_rinf, idx_induc, cs,
                       inductance_scale, freq, mask, fit_status, z_re, z_im);
}

// predict_response (drt1d.py:3363-3464) of every member from T = cs U x, the unit-step layers applied to the resident solution
// (entry s * nt + i of row b): threads run along i, so T, the response vectors and out are read and written with unit stride.
//   v = sum_s size[b][s] (T[b][s][i] - Tn[b][s][i])        one accumulator, s ascending: the same bits alone and in a batch
//     + sum_s size[b][s] Td[b][s][i]
//     + inf_rv[i] r_inf + c_inv cap_rv[i]
//   v *= 1 + vz_offset strength[i];  v += vb_mat[i] . v_baseline
// r_inf, c_inv and v_baseline in data units as extract_qphb_parameters forms them (6228-6289): the baseline coefficients lose their
// column normalisation, the first one the scaled offset, then all take the response scale.  A failed fit gives a NaN row.
__global__ __launch_bounds__(256) void response_assemble_kernel(int B, ResponseArgs a) {
    const int i = blockIdx.y * blockDim.x + threadIdx.x, b = blockIdx.x;
    if (i >= a.nt || b >= B) return;
    const double* sz = a.sizes + (a.sizes_batched ? (size_t)b * a.S : 0);
    const double* x = a.X + (size_t)b * a.ldx;
    const double c = a.cs[b];
    double v = 0.0;
    if ((a.mask & HIPDRT_INCLUDE_DRT) && a.T) {
        const double* t = a.T + (size_t)b * a.ldt + i;
        const double* tn = a.Tn ? a.Tn + (size_t)b * a.ldt + i : nullptr;
        double acc = 0.0;
        for (int s = 0; s < a.S; ++s) {
            double ts = t[(size_t)s * a.nt];
            if (tn) ts = ts - tn[(size_t)s * a.nt];
            acc += sz[s] * ts;
        }
        v += acc;
    }
    if ((a.mask & HIPDRT_INCLUDE_DOP) && a.Td) {
        const double* t = a.Td + (size_t)b * a.ldt + i;
        double acc = 0.0;
        for (int s = 0; s < a.S; ++s) acc += sz[s] * t[(size_t)s * a.nt];
        v += acc;
    }
    if ((a.mask & HIPDRT_INCLUDE_OHMIC) && a.idx_rinf >= 0 && a.inf_rv)
        v += a.inf_rv[(a.inf_batched ? (size_t)b * a.nt : 0) + i] * (x[a.idx_rinf] * c);
    if ((a.mask & HIPDRT_INCLUDE_CAP) && a.idx_cinv >= 0 && a.cap_rv)
        v += (x[a.idx_cinv] * (c * a.capacitance_scale)) * a.cap_rv[(a.cap_batched ? (size_t)b * a.nt : 0) + i];
    if ((a.mask & HIPDRT_INCLUDE_VZ_OFFSET) && a.vz_index >= 0 && a.strength) v *= 1.0 + x[a.vz_index] * a.strength[i];
    if ((a.mask & HIPDRT_INCLUDE_BASELINE) && a.vb_size > 0 && a.vb_mat) {
        double acc = 0.0;
        for (int k = 0; k < a.vb_size; ++k) {
            double coef = x[a.vb_start + k] * (1.0 / a.vb_scale[k]);
            if (k == 0 && a.sro) coef -= a.sro[b];
            acc += a.vb_mat[(size_t)i * a.vb_size + k] * (coef * a.rss[b]);
        }
        v += acc;
    }
    if (a.fit_status && a.fit_status[b] < 0) v = NAN;
    a.out[(size_t)b * a.nt + i] = v;
}

void launch_response_assemble(hipStream_t st, int B, const ResponseArgs& a) {
    hipLaunchKernelGGL(response_assemble_kernel, dim3(B, (a.nt + 255) / 256), dim3(256), 0, st, B, a);
}

// predict_z (drt1d.py:3500-3542) of every member of a prepared plan from Y = cs [A'; A''] x (row b: nf real parts, then nf
// imaginary parts; Yn the negative copy of a series_neg block, Yd the phasor-Z rows of a DOP block):
//   Z = (Y - Yn) + Yd + R_inf + j 2 pi f L + C_inv / (j 2 pi f),   Z *= 1 - vz_offset eis_strength[f]
// every term switchable, the ideal elements rescaled like extract_qphb_parameters (6228-6289) and formed as numpy forms
// `induc * 2j * np.pi * frequencies` and `c_inv * (2j * np.pi * frequencies) ** -1`.  A failed fit gives a NaN row.
__global__ __launch_bounds__(256) void z_model_assemble_kernel(int B, ZModelArgs a) {
    const int i = blockIdx.y * blockDim.x + threadIdx.x, b = blockIdx.x;
    if (i >= a.nf || b >= B) return;
    const double* x = a.X + (size_t)b * a.ldx;
    const double c = a.cs[b];
    const size_t o = (size_t)b * 2 * a.nf + i;
    double re = 0.0, im = 0.0;
    if ((a.mask & HIPDRT_INCLUDE_DRT) && a.Y) {
        re = a.Y[o]; im = a.Y[o + a.nf];
        if (a.Yn) { re = re - a.Yn[o]; im = im - a.Yn[o + a.nf]; }
    }
    if ((a.mask & HIPDRT_INCLUDE_OHMIC) && a.idx_rinf >= 0) re += x[a.idx_rinf] * c;
    if ((a.mask & HIPDRT_INCLUDE_INDUCTANCE) && a.idx_induc >= 0) {
        const double induc = x[a.idx_induc] * (c * a.inductance_scale);
        im += ((induc * 2.0) * 3.141592653589793) * a.freq[i];
    }
    if ((a.mask & HIPDRT_INCLUDE_CAP) && a.idx_cinv >= 0)
        im += (x[a.idx_cinv] * (c * a.capacitance_scale)) * -(1.0 / (6.283185307179586 * a.freq[i]));
    if ((a.mask & HIPDRT_INCLUDE_DOP) && a.Yd) { re += a.Yd[o]; im += a.Yd[o + a.nf]; }
    if ((a.mask & HIPDRT_INCLUDE_VZ_OFFSET) && a.vz_index >= 0 && a.strength) {
        const double f = 1.0 - x[a.vz_index] * a.strength[i];
        re *= f; im *= f;
    }
    if (a.fit_status && a.fit_status[b] < 0) { re = NAN; im = NAN; }
    a.z_re[(size_t)b * a.nf + i] = re;
    a.z_im[(size_t)b * a.nf + i] = im;
}

void launch_z_model_assemble(hipStream_t st, int B, const ZModelArgs& a) {
    hipLaunchKernelGGL(z_model_assemble_kernel, dim3(B, (a.nf + 255) / 256), dim3(256), 0, st, B, a);
}

// predict_dop (drt1d.py:3273-3347) of every member from dop[b][i] = cs E (dop_scale_vector x_dop), in place: the division by
// get_dop_norm's vector (null: none), then the ideal elements at nu = 0, 1, -1 -- R_inf, inductance and C_inv in data units, each
// divided by norm[i] * basis_area when normalised (they are delta functions: the basis-function area does not scale them).
__global__ __launch_bounds__(256) void dop_assemble_kernel(int B, DopArgs a) {
    const int i = blockIdx.y * blockDim.x + threadIdx.x, b = blockIdx.x;
    if (i >= a.nn || b >= B) return;
    const double* x = a.X + (size_t)b * a.ldx;
    const double c = a.cs[b], nu = a.nu[i];
    double v = a.dop[(size_t)b * a.nn + i];
    if (a.norm) v = v / a.norm[i];
    if (a.include_ideal && (nu == 0.0 || nu == 1.0 || nu == -1.0)) {
        double e = 0.0;
        if (nu == 0.0) e = a.idx_rinf >= 0 ? x[a.idx_rinf] * c : 0.0;
        else if (nu == 1.0) e = a.idx_induc >= 0 ? x[a.idx_induc] * (c * a.inductance_scale) : 0.0;
        else e = a.idx_cinv >= 0 ? x[a.idx_cinv] * (c * a.capacitance_scale) : 0.0;
        if (a.norm) e = e / (a.norm[i] * a.basis_area);
        v += e;
    }
    if (a.fit_status && a.fit_status[b] < 0) v = NAN;
    a.dop[(size_t)b * a.nn + i] = v;
}

void launch_dop_assemble(hipStream_t st, int B, const DopArgs& a) {
    hipLaunchKernelGGL(dop_assemble_kernel, dim3(B, (a.nn + 255) / 256), dim3(256), 0, st, B, a);
}

// out[b][j] = X[b][col + j] * v[b][j]: the DOP block of every member times that member's own dop_scale_vector (solve_rp rescales
// it per member), the operand the DOP rows are applied to
__global__ void scale_block_kernel(int B, int nd, const double* __restrict__ X, long long ldx, int col, const double* __restrict__ v,
                                   double* __restrict__ out) {
    const int j = blockIdx.y * blockDim.x + threadIdx.x, b = blockIdx.x;
    if (j < nd && b < B) out[(size_t)b * nd + j] = X[(size_t)b * ldx + col + j] * v[(size_t)b * nd + j];
}

void launch_scale_block(hipStream_t st, int B, int nd, const double* X, long long ldx, int col, const double* v, double* out) {
    hipLaunchKernelGGL(scale_block_kernel, dim3(B, (nd + 255) / 256), dim3(256), 0, st, B, nd, X, ldx, col, v, out);
}

// ---- the posterior of the distribution of phasances (drt1d.py:3153-3198 estimate_dop_cov, 3233-3258 predict_dop_ci) -----------------
// estimate_param_cov (4126-4133) rescales inv(P) by D = diag(dop_scale_vector) on both sides of its DOP block, and under solve_rp D
// differs from member to member.  The variance kernel takes one shared set of packed rows, so the members' scales go into P instead:
// with S = diag(s), s = 1 / dop_scale_vector on the DOP unknowns and 1 elsewhere, inv(S P S) = D inv(P) D, and the shared rows E
// over the DOP columns give e' D inv(P)[dop, dop] D e from the chain that serves the DRT band.
//
// s is formed once per member, by one correctly rounded division per entry, so every tile of a member sees the same bits.
__global__ void dop_recip_kernel(int B, int nd, const double* __restrict__ dsv, long long dsv_stride, double* __restrict__ sinv) {
    const int j = blockIdx.y * blockDim.x + threadIdx.x, b = blockIdx.x;
    if (j >= nd || b >= B) return;
    const double d = dsv[(size_t)b * dsv_stride + j];
    sinv[(size_t)b * nd + j] = (d > 0.0 && d < INFINITY) ? 1.0 / d : 1.0;
}

void launch_dop_recip(hipStream_t st, int B, int nd, const double* dsv, long long dsv_stride, double* sinv) {
    hipLaunchKernelGGL(dop_recip_kernel, dim3(B, (nd + 255) / 256), dim3(256), 0, st, B, nd, dsv, dsv_stride, sinv);
}

// Entry (i, j) of every lower tile becomes (P_ij s_i) s_j, in that order: two roundings, the same for a member alone and inside a
// batch.  One wavefront per tile in pack_p_kernel's lane map (gram.hip): lane l holds row l & 15 and, as two double2, the columns
// q, q + 4 and q + 8, q + 12 with q = l >> 4 -- 16-byte loads and stores.  Only the tiles whose row range or column range meets the
// DOP block are visited: workgroup (k, y) takes tile row t = t0 + y up to its diagonal tile (k <= t) and tile column t below the
// band (k > t1; the tiles (k, t) with t < k <= t1 belong to row k), so each of them is visited once.  Only entries with i or j in
// the block are written: the zeros beyond n, the identity padding and the tiles above the diagonal stay as they were.
__global__ __launch_bounds__(64) void scale_p_kernel(int nt, int t0, int t1, int dop_start, int dop_size,
                                                     const double* __restrict__ sinv, long long sinv_stride,
                                                     double* __restrict__ Ppk, long long ppk_stride, int nchp) {
    const int b = blockIdx.x / nt, k = blockIdx.x % nt, t = t0 + blockIdx.y, lane = threadIdx.x;
    int tr, tc;
    if (k <= t) { tr = t; tc = k; }
    else if (k > t1) { tr = k; tc = t; }
    else return;
    const double* s = sinv + (size_t)b * sinv_stride;
    double2* tile = reinterpret_cast<double2*>(Ppk + (size_t)b * ppk_stride + ((size_t)tr * nchp + tc) * 256);
    const int i = tr * 16 + (lane & 15) - dop_start, j0 = tc * 16 + (lane >> 4) - dop_start;
    const bool ri = i >= 0 && i < dop_size;
    const double si = ri ? s[i] : 1.0;
    const int fo = (lane & 15) * 4 + (lane >> 4);
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int ja = j0 + 8 * h, jb = ja + 4;
        const bool ca = ja >= 0 && ja < dop_size, cb = jb >= 0 && jb < dop_size;
        if (!(ri || ca || cb)) continue;
        double2 v = tile[64 * h + fo];
        if (ri) { v.x = v.x * si; v.y = v.y * si; }
        if (ca) v.x = v.x * s[ja];
        if (cb) v.y = v.y * s[jb];
        tile[64 * h + fo] = v;
    }
}

void launch_scale_p(hipStream_t st, int B, int n, int dop_start, int dop_size, const double* sinv, long long sinv_stride,
                    double* Ppk, long long ppk_stride) {
    const int nt = (n + 15) / 16, t0 = dop_start / 16, t1 = (dop_start + dop_size - 1) / 16;
    hipLaunchKernelGGL(scale_p_kernel, dim3((unsigned)B * nt, t1 - t0 + 1), dim3(64), 0, st, nt, t0, t1, dop_start, dop_size, sinv,
                       sinv_stride, Ppk, ppk_stride, qp_nchp(n));
}

// predict_dop_ci's band on the mean that dop_assemble_kernel left (ideal elements included: upstream adds no variance for them):
// estimate_dop_cov divides the covariance by get_dop_norm's vector squared, so sigma = sqrt(var cs^2) / norm[i].
__global__ void dop_band_kernel(int B, int nn, const double* __restrict__ mu, const double* __restrict__ var, long long ldv,
                                const double* __restrict__ cs, const double* __restrict__ norm, double s_lo, double s_hi,
                                const int* __restrict__ var_status, const int* __restrict__ fit_status, double* __restrict__ lo,
                                double* __restrict__ hi, double* __restrict__ var_out) {
    const int i = blockIdx.y * blockDim.x + threadIdx.x, b = blockIdx.x;
    if (i >= nn || b >= B) return;
    const size_t o = (size_t)b * nn + i;
    double l = NAN, h = NAN, vo = NAN;
    if (var_status[b] == 0 && fit_status[b] >= 0) {
        const double v = var[(size_t)b * ldv + i] * (cs[b] * cs[b]);
        double sg = sqrt(v);
        vo = v;
        if (norm) { sg = sg / norm[i]; vo = v / (norm[i] * norm[i]); }
        const double m = mu[o];
        l = m + s_lo * sg;
        h = m + s_hi * sg;
    }
    if (lo) lo[o] = l;
    if (hi) hi[o] = h;
    if (var_out) var_out[o] = vo;
}

void launch_dop_band(hipStream_t st, int B, int nn, const double* mu, const double* var, long long ldv, const double* cs,
                     const double* norm, double s_lo, double s_hi, const int* var_status, const int* fit_status, double* lo,
                     double* hi, double* var_out) {
    hipLaunchKernelGGL(dop_band_kernel, dim3(B, (nn + 255) / 256), dim3(256), 0, st, B, nn, mu, var, ldv, cs, norm, s_lo, s_hi,
                       var_status, fit_status, lo, hi, var_out);
}

}  // namespace hipdrt
