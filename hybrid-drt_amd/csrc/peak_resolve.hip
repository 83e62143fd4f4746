// Per-peak coefficients, distributions and resistances of a fitted batch, one 256-thread workgroup per spectrum:
//
//   peaks.find_troughs                          hybdrt/peaks.py:92-136
//   peaks.estimate_peak_weight_distributions    hybdrt/peaks.py:139-217
//   DRT.estimate_peak_coef / estimate_peak_drts / quantify_peaks      hybdrt/models/drt1d.py:3949-4111
//   DRT.split_r_p / integrate_drt               drt1d.py:3586-3620
//
// hipdrt/models/peaks.py (find_troughs, peak_epsilons, peak_weights, resolve_peaks_row, window_integrals) is the same rule in
// numpy.  All quantities are in data units: x_red = get_drt_params(cs_b * x_b, sign).
//
// Order of work.  f and fxx of the find grid are staged in LDS.  The peak list is compacted in ascending order from the keep row
// of peaks_kernel (the rank of a kept sample is the number of kept samples below it: contiguous chunks per thread and one
// scan of the 256 counts), or read from the caller's index row, or found per window (i + argmin fxx[i:j]).  One wavefront per neighbouring
// pair of peaks then finds the trough: every argmin / argmax is a reduction over (value, index) pairs in which the smaller index
// wins a tie, within a lane (ascending scan, strict comparison) and across lanes (butterfly), so the result is numpy's first
// extremum whichever lane holds which sample.  The inverse length scales follow.  Every thread then owns the basis columns
// j = tid, tid + 256, ...: it writes w[i][j] = exp(-(eps y)^2) into the LDS operand xw, sums over the peaks in ascending order,
// and rescales in place to x_peaks[i][j] = x_red[j] * (w[i][j] / sum), the order upstream rounds in.  x and ln(basis tau) are read
// once from global memory; no sum vector is held.  r_coef is one block reduction per peak (per-thread partial sums over
// j = tid, tid + 256, ..., then blk_sum<256>'s tree).
//
// peak_gammas = x_peaks E0' runs on v_mfma_f64_16x16x4_f64 with predict.hip's layout: A[l & 15][l >> 4] = 16 peaks x 4 k from xw,
// B[l >> 4][l & 15] = E0' (4 k x 16 output points) read from the shared E0[nout][nb] in global memory (one matrix per call, L2
// resident), C/D col = lane & 15 (output point), row = (lane >> 4) + 4 reg (peak).  Wavefront w owns the output tiles w, w + 4, ...
// of every 16-peak tile that holds a peak.  Every output element has ONE accumulator and takes its k-blocks of four in ascending
// order from k = 0: no split-K, no atomics, so a spectrum alone and the same spectrum in a batch give the same bits.  Tails: the
// columns nb .. of xw and rows of absent peaks are zeros, E0 past nb or nout is loaded as zero.
//
// Leading dimension of xw: ld = the smallest value >= nb rounded up to 4 with ld % 32 == 4 (1028 for nb = 1024).  The operand
// read of a k-block takes 16 rows x 4 consecutive doubles; with 64 banks of 4 bytes a row's four doubles cover 8 banks and rows
// are 2 ld = 8 (mod 64) banks apart, so rows 0-7 tile the 64 banks exactly once and rows 8-15 a second time: every bank twice
// per 64 lanes, the minimum for 8-byte words (predict.hip's 68 is the same residue).  The weight phase writes consecutive doubles
// from consecutive lanes, conflict free for any ld.
//
// The accumulators of one peak tile go to an LDS row block gam[16][ldg]; the trapezoid (quantify_peaks) and the dense stores of
// peak_gammas read it.  The trapezoid of a peak is summed by 16 threads, thread t taking the terms k = t, t + 16, ... in ascending
// order, then a fixed xor tree over the 16: the order depends on nout alone.
//
// Stores: vector stores only, dense and padded -- absent peaks get NaN / -1; nothing outside [B][max_peaks][.] is written, and an
// output left NULL is never formed in global memory.  Compiled with -ffp-contract=off: every product and sum rounds as written.
#include <cmath>

#include "hyper_dev.hpp"
#include "peaks_dev.hpp"

namespace hipdrt {

static constexpr int RT = 256;
static constexpr int RNW = RT / 64;
typedef double v4d __attribute__((ext_vector_type(4)));

// (value, index) reductions over one wavefront; the smaller index wins a tie; every lane gets the result
struct ValIdx { double v; int i; };
template <bool MAX>
__device__ __forceinline__ ValIdx wave_arg(ValIdx a) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) {
        const double ov = __shfl_xor(a.v, off, 64);
        const int oi = __shfl_xor(a.i, off, 64);
        const bool better = oi >= 0 && (a.i < 0 || (MAX ? ov > a.v : ov < a.v) || (ov == a.v && oi < a.i));
        if (better) { a.v = ov; a.i = oi; }
    }
    return a;
}
// first extremum of g(i) over [s, e): lanes scan i = s + lane, s + lane + 64, ... in ascending order with a strict comparison
template <bool MAX, class G>
__device__ __forceinline__ ValIdx wave_arg_range(int s, int e, G g) {
    ValIdx a{0.0, -1};
    for (int i = s + (int)(threadIdx.x & 63); i < e; i += 64) {
        const double v = g(i);
        if (a.i < 0 || (MAX ? v > a.v : v < a.v)) { a.v = v; a.i = i; }
    }
    return wave_arg<MAX>(a);
}

static_assert(RT == PR_THREADS, "the layout's scan row has one int per thread");
size_t peak_resolve_lds_bytes(int nfind, int nb, int nout, int max_peaks) {
    return peak_resolve_lds(nullptr, nfind, peak_resolve_ld(nb), pr_ldg(nout), nout, max_peaks).bytes;
}

// grid = B
__global__ __launch_bounds__(RT) void peak_resolve_kernel(PeakResolveArgs a) {
    extern __shared__ double sm[];
    __shared__ double red[RNW];
    __shared__ int s_cnt;
    const int b = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n = a.nfind, nb = a.nb, nout = a.nout, mp = a.max_peaks, ld = a.ld, ldg = pr_ldg(nout);
    const PeakResolveLds L = peak_resolve_lds(sm, n, ld, ldg, nout, mp);
    double *f = L.f, *fxx = L.fxx, *xw = L.xw, *gam = L.gam, *epsl = L.epsl, *epsr = L.epsr, *rco = L.rco, *rpk = L.rpk;
    int *pk = L.pk, *tr = L.tr, *scan = L.scan;

    // padded rows of one spectrum: NaN floats and -1 ints from peak slot `from` on
    auto pad_rows = [&](int from) {
        for (int i = from + tid; i < mp; i += RT) {
            const size_t o = (size_t)b * mp + i;
            if (a.peak_index) a.peak_index[o] = -1;
            if (a.trough_index) a.trough_index[o] = -1;
            if (a.eps_l) a.eps_l[o] = NAN;
            if (a.eps_r) a.eps_r[o] = NAN;
            if (a.r_peaks) a.r_peaks[o] = NAN;
            if (a.r_coef) a.r_coef[o] = NAN;
        }
        if (a.x_peaks)
            for (size_t i = (size_t)from * nb + tid; i < (size_t)mp * nb; i += RT) a.x_peaks[(size_t)b * mp * nb + i] = NAN;
        if (a.peak_gammas)
            for (size_t i = (size_t)from * nout + tid; i < (size_t)mp * nout; i += RT) a.peak_gammas[(size_t)b * mp * nout + i] = NAN;
    };

    const int fs = a.fit_status ? a.fit_status[b] : 0;
    if (fs < 0) {                                       // a failed fit: count 0 and empty rows, as peaks_kernel gives
        pad_rows(0);
        if (tid == 0) {
            if (a.count) a.count[b] = 0;
            if (a.status) a.status[b] = fs;
        }
        return;
    }

    // ---- stage the rows ----
    const size_t row = (size_t)b * n;
    for (int i = tid; i < n; i += RT) { f[i] = a.f[row + i]; fxx[i] = a.fxx[row + i]; }
    for (int i = tid; i < mp; i += RT) { pk[i] = -1; tr[i] = -1; }
    __syncthreads();

    // ---- the peak list, ascending ----
    int P = 0, st = 0;
    if (a.source == 0) {
        const int chunk = (n + RT - 1) / RT, i0 = tid * chunk, i1 = (i0 + chunk < n) ? i0 + chunk : n;
        const int* keep = a.keep + row;
        int c = 0;
        for (int i = i0; i < i1; ++i) c += keep[i] != 0;
        scan[tid] = c;
        __syncthreads();
        for (int off = 1; off < RT; off <<= 1) {         // inclusive scan
            const int v = tid >= off ? scan[tid - off] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        P = scan[RT - 1];
        if (P <= mp) {
            int r = scan[tid] - c;
            for (int i = i0; i < i1; ++i) if (keep[i] != 0) pk[r++] = i;
        } else {
            st = HIPDRT_PEAKS_OVERFLOW;
        }
    } else if (a.source == 1) {
        const int* idx = a.indices + (size_t)b * mp;
        int c = 0;
        for (int i = tid; i < mp; i += RT) { const int v = idx[i]; pk[i] = v; c += v >= 0; }
        P = (int)blk_sum<RT>((double)c, red);
    } else {
        // one peak per window: i + argmin(fxx[i:j]); a window's end is clipped to the grid as numpy clips a slice
        for (int k = wv; k < a.nwin; k += RNW) {
            const int s = a.win_start[k], e = a.win_end[k] < n ? a.win_end[k] : n;
            const ValIdx m = wave_arg_range<false>(s, e, [&](int i) { return fxx[i]; });
            if (lane == 0) pk[k] = m.i;
        }
        P = a.nwin;
        __syncthreads();
        if (tid == 0) {                                  // two windows share their border sample: upstream fails on a repeated peak
            int ok = 1;
            for (int k = 0; k < P; ++k) ok &= pk[k] >= 0 && (k + 1 >= P || pk[k] < pk[k + 1]);
            s_cnt = ok;
        }
        __syncthreads();
        if (!s_cnt) st = HIPDRT_PEAKS_UNORDERED;
    }
    __syncthreads();
    if (st != 0) {
        pad_rows(0);
        if (tid == 0) {
            if (a.count) a.count[b] = P;
            if (a.status) a.status[b] = st;
        }
        return;
    }

    // ---- troughs (peaks.py:108-134): one wavefront per neighbouring pair ----
    for (int q = wv; q + 1 < P; q += RNW) {
        const int s = pk[q], e = pk[q + 1];
        const double ls = np_sign(f[s]), rs = np_sign(f[e]);
        int t;
        if (ls == rs) {
            const ValIdx m = wave_arg_range<false>(s, e, [&](int i) { return ls * f[i]; });
            const double vs = ls * f[s], ve = ls * f[e];
            if (m.v < (ve < vs ? ve : vs)) {
                t = m.i;
            } else {
                const ValIdx x = wave_arg_range<true>(s, e, [&](int i) { return ls * (-(f[i] - fxx[i])); });
                t = x.i;
                if (t == s) t = (s + e + 2 * t) / 4;
            }
        } else {
            t = wave_arg_range<false>(s, e, [&](int i) { return fabs(f[i]); }).i;
        }
        if (lane == 0) tr[q] = t;
    }
    __syncthreads();

    // ---- inverse length scales (peaks.py:164-199) ----
    const hipdrt_peak_resolve_opts& o = a.o;
    for (int i = tid; i < P; i += RT) {
        double el, er;
        if (o.epsilon_uniform == o.epsilon_uniform) {
            el = er = o.epsilon_uniform;
        } else {
            const double lp = a.lt[pk[i]];
            const double prev = i == 0 ? a.lt[0] : a.lt[tr[i - 1]];
            const double next = i == P - 1 ? a.lt[n - 1] : a.lt[tr[i]];
            el = o.epsilon_factor / (lp - prev);
            er = o.epsilon_factor / (next - lp);
            if (o.max_epsilon < el) el = o.max_epsilon;          // min(el, max_epsilon)
            if (o.max_epsilon < er) er = o.max_epsilon;
            if (o.min_epsilon == o.min_epsilon) {
                if (o.min_epsilon > el) el = o.min_epsilon;      // max(el, min_epsilon)
                if (o.min_epsilon > er) er = o.min_epsilon;
            }
        }
        epsl[i] = el; epsr[i] = er;
    }
    __syncthreads();

    // ---- weights and x_peaks into the operand xw[Pt * 16][ld]; rows of absent peaks and the columns past nb are zeros ----
    const int live_tiles = (P + 15) / 16, rows = live_tiles * 16;
    const int kpad = (nb + 3) & ~3;
    const double* x = a.X + (size_t)b * a.ldx + a.col_offset;
    const double cs = a.cs ? a.cs[b] : 1.0;
    for (int j = tid; j < kpad; j += RT) {
        if (j >= nb) {
            for (int i = 0; i < rows; ++i) xw[(size_t)i * ld + j] = 0.0;
            continue;
        }
        // get_drt_params on the coefficients in data units: the copies are scaled first, then combined, as upstream rounds
        double xr;
        if (a.copies == 1 || o.sign == 1) xr = x[j] * cs;
        else if (o.sign == -1) xr = -(x[nb + j] * cs);
        else xr = x[j] * cs - x[nb + j] * cs;
        if (P <= 1) {
            if (P == 1) xw[j] = xr * 1.0;
        } else {
            const double lbj = a.lb[j];
            double sum = 0.0;
            for (int i = 0; i < P; ++i) {
                const double y = lbj - a.lt[pk[i]];
                const double ey = (y < 0.0 ? epsl[i] : epsr[i]) * y;
                const double w = exp(-(ey * ey));
                xw[(size_t)i * ld + j] = w;
                sum = sum + w;
            }
            for (int i = 0; i < P; ++i) xw[(size_t)i * ld + j] = xr * (xw[(size_t)i * ld + j] / sum);
        }
        for (int i = P; i < rows; ++i) xw[(size_t)i * ld + j] = 0.0;
    }
    __syncthreads();

    // ---- r_coef = predict_r_p(x = x_peak): sum_j x_peaks[i][j] * basis area ----
    for (int i = 0; i < P; ++i) {
        double s = 0.0;
        for (int j = tid; j < nb; j += RT) s += xw[(size_t)i * ld + j];
        s = blk_sum<RT>(s, red);
        if (tid == 0) rco[i] = s * a.basis_area;
    }

    // ---- x_peaks rows, dense ----
    if (a.x_peaks) {
        double* xp = a.x_peaks + (size_t)b * mp * nb;
        for (int i = 0; i < P; ++i)
            for (int j = tid; j < nb; j += RT) xp[(size_t)i * nb + j] = xw[(size_t)i * ld + j];
    }

    // ---- peak_gammas = x_peaks E0' on the matrix pipe, tile by tile of 16 peaks; r_peaks from the LDS rows ----
    if (nout > 0) {
        const int otiles = (nout + 15) / 16;
        for (int pt = 0; pt < live_tiles; ++pt) {
            for (int ot = wv; ot < otiles; ot += RNW) {
                v4d acc = (v4d){0.0, 0.0, 0.0, 0.0};
                const int oc = ot * 16 + (lane & 15);
                const double* arow = xw + (size_t)(pt * 16 + (lane & 15)) * ld + (lane >> 4);
                const bool oin = oc < nout;
                const double* erow = a.E0 + (size_t)(oin ? oc : 0) * nb + (lane >> 4);
                // whole k-blocks: four blocks' loads issued together (a padding column reads row 0 and is zeroed after the load)
                const int kfull = nb & ~3;
                int k0 = 0;
                for (; k0 + 16 <= kfull; k0 += 16) {
                    double e0 = erow[k0], e1 = erow[k0 + 4], e2 = erow[k0 + 8], e3 = erow[k0 + 12];
                    if (!oin) { e0 = 0.0; e1 = 0.0; e2 = 0.0; e3 = 0.0; }
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(arow[k0], e0, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(arow[k0 + 4], e1, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(arow[k0 + 8], e2, acc, 0, 0, 0);
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(arow[k0 + 12], e3, acc, 0, 0, 0);
                }
                for (; k0 < kfull; k0 += 4) {
                    double e0 = erow[k0];
                    if (!oin) e0 = 0.0;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(arow[k0], e0, acc, 0, 0, 0);
                }
                if (kfull < kpad) {                      // the last, partial block: E0 past nb comes in as zero
                    const double e0 = (oin && kfull + (lane >> 4) < nb) ? erow[kfull] : 0.0;
                    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(arow[kfull], e0, acc, 0, 0, 0);
                }
#pragma unroll
                for (int reg = 0; reg < 4; ++reg) gam[((lane >> 4) + 4 * reg) * ldg + ot * 16 + (lane & 15)] = acc[reg];
            }
            __syncthreads();
            const int np = (P - pt * 16) < 16 ? (P - pt * 16) : 16;
            if (a.peak_gammas) {
                double* g = a.peak_gammas + ((size_t)b * mp + pt * 16) * nout;
                for (int i = 0; i < np; ++i)
                    for (int k = tid; k < nout; k += RT) g[(size_t)i * nout + k] = gam[i * ldg + k];
            }
            {   // np.trapezoid(gamma, x = ln tau): 16 threads per peak
                const int pi = tid >> 4, t = tid & 15;
                double s = 0.0;
                for (int k = t; k + 1 < nout; k += 16)
                    s += ((a.lto[k + 1] - a.lto[k]) * (gam[pi * ldg + k + 1] + gam[pi * ldg + k])) / 2.0;
#pragma unroll
                for (int off = 8; off > 0; off >>= 1) s += __shfl_xor(s, off, 16);
                if (t == 0 && pi < np) rpk[pt * 16 + pi] = s;
            }
            __syncthreads();
        }
    }
    __syncthreads();

    // ---- the per-peak scalars, dense and padded ----
    for (int i = tid; i < P; i += RT) {
        const size_t oo = (size_t)b * mp + i;
        if (a.peak_index) a.peak_index[oo] = pk[i];
        if (a.trough_index) a.trough_index[oo] = i + 1 < P ? tr[i] : -1;
        if (a.eps_l) a.eps_l[oo] = epsl[i];
        if (a.eps_r) a.eps_r[oo] = epsr[i];
        if (a.r_peaks) a.r_peaks[oo] = nout > 0 ? rpk[i] : NAN;
        if (a.r_coef) a.r_coef[oo] = rco[i];
    }
    pad_rows(P);
    if (tid == 0) {
        if (a.count) a.count[b] = P;
        if (a.status) a.status[b] = fs;
    }
}

int peak_resolve_check_opts(const hipdrt_peak_resolve_opts& o) {
    HIPDRT_REQUIRE(o.sign >= -1 && o.sign <= 1, "sign must be 1, -1 or 0");
    HIPDRT_REQUIRE(o.max_peaks >= 1 && o.max_peaks <= 64, "1 <= max_peaks <= 64");
    HIPDRT_REQUIRE(std::isfinite(o.epsilon_factor) && std::isfinite(o.max_epsilon), "epsilon_factor and max_epsilon must be finite");
    HIPDRT_REQUIRE(!std::isinf(o.min_epsilon) && !std::isinf(o.epsilon_uniform), "min_epsilon and epsilon_uniform: finite, or NaN for none");
    return HIPDRT_OK;
}

int launch_peak_resolve(hipStream_t s, PeakResolveArgs a, int B) {
    if (int rc = peak_resolve_check_opts(a.o)) return rc;
    HIPDRT_REQUIRE(B >= 1 && a.nfind >= 1 && a.nb >= 1 && a.nout >= 0, "peak_resolve: B, nfind, nb >= 1");
    HIPDRT_REQUIRE(a.f && a.fxx && a.X && a.lt && a.lb, "peak_resolve: the rows, the coefficients and both ln grids");
    HIPDRT_REQUIRE(a.source >= 0 && a.source <= 2, "peak_resolve: source must be 0 (keep rows), 1 (indices) or 2 (windows)");
    HIPDRT_REQUIRE(a.source != 0 || a.keep, "peak_resolve: source 0 needs the keep rows");
    HIPDRT_REQUIRE(a.source != 1 || a.indices, "peak_resolve: source 1 needs the index rows");
    HIPDRT_REQUIRE(a.source != 2 || (a.win_start && a.win_end && a.nwin >= 1 && a.nwin <= a.o.max_peaks),
                   "peak_resolve: source 2 needs 1 .. max_peaks windows");
    HIPDRT_REQUIRE(a.nout == 0 || (a.E0 && a.lto), "peak_resolve: an output grid needs its evaluation matrix and its ln grid");
    HIPDRT_REQUIRE(a.copies == 1 || a.copies == 2, "peak_resolve: one or two copies of the basis");
    HIPDRT_REQUIRE(a.copies == 2 || a.o.sign == 1, "sign must be 1 unless the DRT block holds a positive and a negative copy");
    a.max_peaks = a.o.max_peaks;
    a.ld = peak_resolve_ld(a.nb);
    const size_t lds = peak_resolve_lds_bytes(a.nfind, a.nb, a.nout, a.max_peaks);
    if (int rc = lds_check(lds, "peak_resolve", "nfind, nb, nout, max_peaks")) return rc;
    if (int rc = set_lds(reinterpret_cast<const void*>(peak_resolve_kernel), lds, "peak_resolve_kernel")) return rc;
    hipLaunchKernelGGL(peak_resolve_kernel, dim3(B), dim3(RT), lds, s, a);
    return 0;
}

// split_r_p without resolve_peaks and integrate_drt: out[b][k] = np.trapezoid(mu[b][i:j], x = ln_tau[i:j]) over the windows
// [start_k, min(end_k, n)).  One wavefront per (spectrum, window): lane l takes the terms i + l, i + l + 64, ... in ascending order,
// then hw_sum's tree -- the order depends on the window alone.  Rows of failed fits are NaN already.
__global__ __launch_bounds__(64) void window_trapz_kernel(int n, int nwin, const double* __restrict__ mu,
                                                          const double* __restrict__ lt, const int* __restrict__ win_start,
                                                          const int* __restrict__ win_end, double* __restrict__ out) {
    const int b = blockIdx.x, k = blockIdx.y, lane = threadIdx.x;
    const int s = win_start[k], e = win_end[k] < n ? win_end[k] : n;
    const double* y = mu + (size_t)b * n;
    double acc = 0.0;
    for (int i = s + lane; i + 1 < e; i += 64) acc += ((lt[i + 1] - lt[i]) * (y[i + 1] + y[i])) / 2.0;
    acc = hw_sum(acc);
    if (lane == 0) out[(size_t)b * nwin + k] = acc;
}

void launch_window_trapz(hipStream_t s, int B, int n, int nwin, const double* mu, const double* lt, const int* win_start,
                         const int* win_end, double* out) {
    hipLaunchKernelGGL(window_trapz_kernel, dim3(B, nwin), dim3(64), 0, s, n, nwin, mu, lt, win_start, win_end, out);
}

}  // namespace hipdrt
