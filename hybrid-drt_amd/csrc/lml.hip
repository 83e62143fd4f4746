// The log marginal likelihood (evidence) of a fitted batch, DRT.evaluate_lml (hybdrt/models/drt1d.py:4513-4543 over
// qphb.evaluate_lml, hybdrt/models/qphb.py:1279-1344):
//     Omega = calculate_qp_l2_matrix(...)                         (qphb.py:53-120)
//     P     = Omega + (W rm)'(W rm)                                (calculate_pq, qphb.py:1154-1183)
//     beta  = 0.5 (|W y|^2 - |W rm x|^2 - x' Omega x) + beta_0 ,  alpha = m / 2 + alpha_0
//     lml   = 0.5 (logdet Omega - logdet P) + sum log w + lgamma(alpha) - lgamma(alpha_0) + alpha_0 ln beta_0 - alpha ln beta
// This file: the kernel of the sums.  The entry point hipdrt_plan_lml_terms (plan_post.hip) forms the packed image of P (launch_gram_l2),
// reduces it to its log-determinant (qp_resident.hpp: logdet_kernel_resident), forms Omega's image in the same place -- the same
// launch with an all-zero weight vector, so that the Gram part adds exact zeros -- and reduces that.  The combination of the eight
// numbers into lml is host arithmetic (hipdrt/models/lml.py: lml_from_terms).
#include "hyper_dev.hpp"

namespace hipdrt {

// grid = B.  Every reduction in the order of llh_kernel (hyper.hip): thread t takes rows t, t + 512, ..., then blk_sum -- a
// spectrum's bits depend neither on the batch size nor on its neighbours, and slw is llh_kernel's sum_log_w bit for bit.
// xox walks the lower triangle of every M_k, which is the triangle launch_gram_l2 reads and mirrors and the factorisation
// references: x' Omega x = sum_k sum_i v_i (2 sum_{j < i} f_ij M_k[i][j] v_j + f_ii M_k[i][i] v_i) with v = sqrt(s_k) x and f the block
// factor of calculate_qp_l2_matrix (dfac_k rho_k on the DRT block, dop_dfac_k dop_rho_k on the DOP block, 1 elsewhere).
__global__ __launch_bounds__(HT) void lml_sums_kernel(LmlSumsArgs a) {
    extern __shared__ double sm[];
    __shared__ double red[HNW];
    const int b = blockIdx.x, tid = threadIdx.x, n = a.n, m = a.m;
    const int lane = tid & 63, wv = tid >> 6;
    if (a.fit_status && a.fit_status[b] < 0) {
        if (tid == 0) {
            const double nan = __builtin_nan("");
            if (a.wy2) a.wy2[b] = nan;
            if (a.fit2) a.fit2[b] = nan;
            if (a.cross) a.cross[b] = nan;
            if (a.slw) a.slw[b] = nan;
            if (a.xox) a.xox[b] = nan;
            if (a.l1x) a.l1x[b] = nan;
        }
        return;
    }
    const LmlLds L = lml_lds(sm, n, m);
    double *xs = L.xs, *vs = L.vs, *yh = L.yh;
    for (int i = tid; i < n; i += HT) xs[i] = a.x[(size_t)b * n + i];
    __syncthreads();
    rows_matvec(a.rm + (size_t)b * a.rm_stride, a.ldrm, m, n, xs, yh);
    __syncthreads();
    const double* rv = a.rv + (size_t)b * m;
    const double* wb = a.w + (size_t)b * m;
    double s_y = 0.0, s_r = 0.0, s_c = 0.0, s_l = 0.0;
    for (int i = tid; i < m; i += HT) {
        const double w = wb[i];
        const double wr = w * yh[i], wy = w * rv[i];
        s_y += wy * wy; s_r += wr * wr; s_c += wr * wy; s_l += log(w);
    }
    s_y = blk_sum(s_y, red); s_r = blk_sum(s_r, red); s_c = blk_sum(s_c, red); s_l = blk_sum(s_l, red);
    double s_1 = 0.0;
    if (a.l1)
        for (int i = tid; i < n; i += HT) s_1 += a.l1[i] * xs[i];
    s_1 = blk_sum(s_1, red);

    const GramL2& g = a.g;
    const bool dop = g.dop_size > 0;
    const int dop_lo = dop ? g.dop_start : 0, dop_hi = dop ? g.dop_start + g.dop_size : 0;
    double acc = 0.0;                    // this wavefront's rows, every lane the same value
    for (int k = 0; k < 3; ++k) {
        if (!(g.dfac[k] > 0.0)) continue;
        const double fac = g.dfac[k] * g.rho[(size_t)b * 3 + k];
        const double fac2 = dop ? g.dop_dfac[k] * g.dop_rho[(size_t)b * 3 + k] : 0.0;
        const double* sk = g.s + ((size_t)b * 3 + k) * n;
        __syncthreads();                 // the previous order's vs has been read
        for (int i = tid; i < n; i += HT) vs[i] = sqrt(sk[i]) * xs[i];
        __syncthreads();
        const double* M = g.mk[k];
        for (int i = wv; i < n; i += HNW) {
            const double* row = M + (size_t)i * g.ldm;
            const bool i_drt = i >= g.ns, i_dop = dop && i >= dop_lo && i < dop_hi;
            double t = 0.0;
            for (int j = lane; j < i; j += 64) {
                double mv = row[j];
                if (i_drt && j >= g.ns) mv *= fac;
                else if (i_dop && j >= dop_lo && j < dop_hi) mv *= fac2;
                t += mv * vs[j];
            }
            t = hw_sum(t);
            double md = row[i];
            if (i_drt) md *= fac;
            else if (i_dop) md *= fac2;
            acc += vs[i] * (2.0 * t + md * vs[i]);
        }
    }
    __syncthreads();
    if (lane == 0) red[wv] = acc;
    __syncthreads();
    if (tid == 0) {
        double xox = 0.0;
#pragma unroll
        for (int w = 0; w < HNW; ++w) xox += red[w];
        if (a.wy2) a.wy2[b] = s_y;
        if (a.fit2) a.fit2[b] = s_r;
        if (a.cross) a.cross[b] = s_c;
        if (a.slw) a.slw[b] = s_l;
        if (a.xox) a.xox[b] = xox;
        if (a.l1x) a.l1x[b] = s_1;
    }
}

size_t lml_sums_lds_bytes(int n, int m) { return lml_lds(nullptr, n, m).bytes; }

int launch_lml_sums(hipStream_t st, const LmlSumsArgs& a, int B) {
    const size_t lds = lml_sums_lds_bytes(a.n, a.m);
    if (int rc = lds_check(lds, "lml sums", "n, m")) return rc;
    if (int rc = set_lds(reinterpret_cast<const void*>(lml_sums_kernel), lds, "lml_sums_kernel")) return rc;
    hipLaunchKernelGGL(lml_sums_kernel, dim3(B), dim3(HT), lds, st, a);
    return HIPDRT_OK;
}

}  // namespace hipdrt
