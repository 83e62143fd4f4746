// hipdrt_map_predict (include/hipdrt.h): the prediction block of a DRTMD map (hybdrt/mapping/drtmd.py:788-1106) on the rows of a
// store -- predict_x 815-833, predict_drt 848-851, the map clamp of predict_drt_cov 993-1008 and the filter of predict_drt_var
// 1017-1019, predict_peak_prob 1023-1064 (curvature.peak_prob_1d, hybdrt/mapping/curvature.py:12-58) and predict_curv_prob
// 1066-1106.  hipdrt/mapping/predict.py is the same arithmetic in numpy.
//
// Stages, all on device buffers between one upload and one download:
//   1  row sums of |x| (drt_sums_kernel of predict.hip: one wavefront per row, fixed lane-strided order and shuffle tree), the
//      division x / (sum|x| area) by element, then the plain 'reflect' Gaussian along psi and / or tau (plain_gaussian_device of
//      map_filter.hip: one accumulator per output element, symmetric order)
//   2  the order-0 and order-2 evaluation matrices (the kernel behind hipdrt_func_eval_matrix) and f = x E0', fxx = x E2' through
//      launch_apply_rows (predict.hip): one accumulator per element, k ascending -- a row predicted alone and the same row inside a
//      map give the same bits
//   3  map_prob_kernel: one 256-thread workgroup per map row; f, fxx and the two variance rows staged in LDS (consecutive threads
//      take consecutive 8-byte words: every bank pair is hit once per 32 lanes), the map clamp, the peak search of peaks_dev.hpp,
//      min(prominence, height) and the two upper-tail probabilities; it writes the unsigned peak row and the curv_prob row.  When
//      the variances are also filtered the clamp runs in clamp_kernel before the filter and map_prob_kernel skips it.
//   4  peak_spread_sigma: the tau-only Gaussian of the peak rows through the same plain pass, then one elementwise kernel for the
//      factor and sign(f); without it that product is done where the row is written.
// No atomics; nothing depends on where a row sits in the launch except through the psi filter's window.  Compiled with
// -ffp-contract=off: every product and sum rounds as numpy's does.
#include <cmath>
#include <cstring>

#include "debug_guard.hpp"
#include "map_filter_dev.hpp"
#include "peaks_dev.hpp"

namespace hipdrt {
namespace {

// x[b][j] /= sum_abs[b] * area (predict_r_p(absolute=True), then x / rp[:, None]: drtmd.py:816-817)
__global__ __launch_bounds__(256) void normalize_kernel(int rows, int nsup, const double* __restrict__ sum_abs, double area,
                                                        double* __restrict__ x) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (size_t)rows * nsup) return;
    const double rp = sum_abs[i / nsup] * area;
    x[i] = x[i] / rp;
}

// the map clamp of one row v[0 .. n) (global memory or LDS), by the whole workgroup: the left side first, then the right one, which
// may then read a value the left side raised; a row that holds a NaN is left alone.  Ends with a barrier.
__device__ __forceinline__ void clamp_row(double* v, int n, int li, int ri) {
    int bad = 0;
    for (int i = threadIdx.x; i < n; i += PKT) bad |= v[i] != v[i];
    if (__syncthreads_or(bad) || li < 0) return;
    const double vl = v[li];
    __syncthreads();
    for (int i = threadIdx.x; i < li; i += PKT) v[i] = np_max(v[i], vl);
    __syncthreads();
    const double vr = v[ri];
    __syncthreads();
    for (int i = ri + (int)threadIdx.x; i < n; i += PKT) v[i] = np_max(v[i], vr);
    __syncthreads();
}

// grid = (rows, 2): in place on the stored f_var (y = 0) and fxx_var (y = 1) rows
__global__ __launch_bounds__(PKT) void clamp_kernel(int n, double* __restrict__ vf, double* __restrict__ vxx,
                                                    const int* __restrict__ ext) {
    const int b = blockIdx.x;
    clamp_row((blockIdx.y ? vxx : vf) + (size_t)b * n, n, ext[2 * b], ext[2 * b + 1]);
}

struct MapProbArgs {
    int n;
    const double *f, *fxx, *vf, *vxx;
    const int* ext;                     // non-null: the clamp runs here
    int search;
    double height, prominence;
    int sign_now;                       // 1: the peak row leaves as pk * sign(f) (no spread follows)
    double *pk, *curv, *vf_out, *vxx_out;
};

// grid = rows
__global__ __launch_bounds__(PKT) void map_prob_kernel(MapProbArgs a) {
    extern __shared__ double sm[];
    const int b = blockIdx.x, tid = threadIdx.x, n = a.n;
    const MapProbLds L = map_prob_lds(sm, n);
    double *f = L.f, *fxx = L.fxx, *vf = L.vf, *vxx = L.vxx, *prom = L.prom;
    int *sgn = L.sgn, *lb = L.lb, *rb = L.rb;
    const size_t row = (size_t)b * n;
    for (int i = tid; i < n; i += PKT) {
        f[i] = a.f[row + i]; fxx[i] = a.fxx[row + i]; vf[i] = a.vf[row + i]; vxx[i] = a.vxx[row + i];
        prom[i] = 0.0; sgn[i] = 0; lb[i] = -1; rb[i] = -1;
    }
    __syncthreads();
    if (a.ext) {
        clamp_row(vf, n, a.ext[2 * b], a.ext[2 * b + 1]);
        clamp_row(vxx, n, a.ext[2 * b], a.ext[2 * b + 1]);
    }
    if (a.pk) {
        // curvature.py:15-41: one pass, or the passes -1 and +1 with the f test (a maximum of fxx is no maximum of -fxx)
        if (a.search != 0) {
            peaks_pass(fxx, f, n, a.search, false, a.height, a.prominence, sgn, prom, lb, rb);
        } else {
            peaks_pass(fxx, f, n, -1, true, a.height, a.prominence, sgn, prom, lb, rb);
            peaks_pass(fxx, f, n, 1, true, a.height, a.prominence, sgn, prom, lb, rb);
        }
        __syncthreads();
    }
    // the dense rows: the only global stores of the kernel
    for (int i = tid; i < n; i += PKT) {
        const size_t o = row + i;
        const double sf = np_sign(f[i]);
        if (a.vf_out) a.vf_out[o] = vf[i];
        if (a.vxx_out) a.vxx_out[o] = vxx[i];
        if (a.pk) {
            double p = 0.0;
            if (sgn[i] != 0) p = map_peak_prob(prom[i], sgn[i] > 0 ? -fxx[i] : fxx[i], f[i], vxx[i], vf[i]);
            a.pk[o] = a.sign_now ? p * sf : p;
        }
        if (a.curv) a.curv[o] = map_curv_prob(f[i], fxx[i], sf, vf[i], vxx[i]);
    }
}

// out = (pk * factor) * sign(f) (drtmd.py:1062-1064)
__global__ __launch_bounds__(256) void spread_sign_kernel(size_t n, const double* __restrict__ pk, double factor,
                                                          const double* __restrict__ f, double* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) out[i] = (pk[i] * factor) * np_sign(f[i]);
}

// ---- stage 3's launches, shared by hipdrt_map_predict and its test hook hipdrt_debug_map_prob ----
// what map_prob_kernel stages for rows of n points; HIPDRT_E_UNSUPPORTED with the limit in the message when LDS does not hold it
int map_prob_lds_check(int n, size_t* lds) {
    *lds = map_prob_lds(nullptr, n).bytes;
    if (*lds > kLdsLimit) {
        const size_t per_point = map_prob_lds(nullptr, 1).bytes;
        set_error("unsupported: map_predict stages " + std::to_string(per_point) + " bytes per evaluation point in LDS: neval <= " +
                  std::to_string(kLdsLimit / per_point) + ", got " + std::to_string(n));
        return HIPDRT_E_UNSUPPORTED;
    }
    return HIPDRT_OK;
}
// the clamp in a kernel of its own, in place on the stored rows
int launch_clamp(hipStream_t st, int rows, int n, double* vf, double* vxx, const int* ext) {
    hipLaunchKernelGGL(clamp_kernel, dim3(rows, 2), dim3(PKT), 0, st, n, vf, vxx, ext);
    LAUNCH_OK();
    return HIPDRT_OK;
}
int launch_map_prob(hipStream_t st, int rows, const MapProbArgs& a) {
    size_t lds;
    TRY(map_prob_lds_check(a.n, &lds));
    TRY(set_lds(reinterpret_cast<const void*>(map_prob_kernel), lds, "map_prob_kernel"));
    hipLaunchKernelGGL(map_prob_kernel, dim3(rows), dim3(PKT), lds, st, a);
    LAUNCH_OK();
    return HIPDRT_OK;
}
// ext: rows pairs of indices of the n-point grid, or (-1, -1)
int check_ext(const int* ext, int rows, int n) {
    for (int b = 0; b < rows; ++b) {
        const int li = ext[2 * b], ri = ext[2 * b + 1];
        HIPDRT_REQUIRE((li == -1 && ri == -1) || (li >= 0 && li < n && ri >= 0 && ri < n),
                       "ext: a pair of indices of the evaluation grid, or (-1, -1)");
    }
    return HIPDRT_OK;
}

}  // namespace
}  // namespace hipdrt

using namespace hipdrt;

extern "C" int hipdrt_map_predict(hipdrt_ctx* ctx, const hipdrt_map_predict_args* g, const double* x, double* x_out, double* f,
                                  double* fxx, double* f_var_out, double* fxx_var_out, double* peak_prob, double* curv_prob) try {
    HIPDRT_REQUIRE(ctx && g && x, "NULL pointer");
    const int rows = g->rows, nsup = g->nsup, neval = g->neval;
    HIPDRT_REQUIRE(rows >= 1 && nsup >= 1, "rows, nsup >= 1");
    HIPDRT_REQUIRE((long long)rows * nsup < (1LL << 30), "rows * nsup < 2^30");
    const bool want_var = f_var_out || fxx_var_out, want_prob = peak_prob || curv_prob;
    const bool want_rows = f || fxx || want_prob;           // (the variances alone need neither grid nor matrices)
    const bool have_var = g->f_var && g->fxx_var;
    HIPDRT_REQUIRE(!g->f_var == !g->fxx_var, "f_var and fxx_var: both or none");
    HIPDRT_REQUIRE(have_var || !(want_var || want_prob), "the variances and the probabilities need f_var and fxx_var");
    if (want_rows || want_var) {
        HIPDRT_REQUIRE(neval >= 1, "neval >= 1");
        HIPDRT_REQUIRE((long long)rows * neval < (1LL << 30), "rows * neval < 2^30");
    }
    if (want_rows) {
        HIPDRT_REQUIRE(g->ln_tau_sup && g->ln_tau_eval, "both grids");
        HIPDRT_REQUIRE(std::isfinite(g->epsilon) && g->epsilon > 0, "epsilon > 0");
    }
    HIPDRT_REQUIRE(!g->normalize || (std::isfinite(g->basis_area) && g->basis_area > 0), "basis_area > 0");
    if (peak_prob) {
        HIPDRT_REQUIRE(g->search >= -1 && g->search <= 1, "search must be 1, -1 or 0 (two passes)");
        HIPDRT_REQUIRE(std::isfinite(g->height) && std::isfinite(g->prominence), "height and prominence must be finite");
        HIPDRT_REQUIRE(g->spread.radius < 0 || (g->spread.w && std::isfinite(g->spread_factor)), "the spread table and its factor");
    }
    const bool stored = have_var && g->var_stored != 0;
    if (stored && g->ext && (want_var || want_prob)) TRY(check_ext(g->ext, rows, neval));
    size_t lds;
    if (want_prob) TRY(map_prob_lds_check(neval, &lds));
    hipStream_t st; TRY(enter(ctx, &st));

    // ---- 1: x ----
    const size_t nx = (size_t)rows * nsup, ne = (size_t)rows * (want_rows || want_var ? neval : 0);
    DevBuf dx, dxf, dsum, dabs;
    TRY(upload(dx, x, nx * sizeof(double), st));
    if (g->normalize) {
        HIPDRT_CHECK(dsum.alloc(rows * sizeof(double))); HIPDRT_CHECK(dabs.alloc(rows * sizeof(double)));
        launch_drt_sums(st, rows, dx.d(), nsup, 0, nsup, 1, 1, dsum.d(), dabs.d());
        hipLaunchKernelGGL(normalize_kernel, dim3((nx + 255) / 256), dim3(256), 0, st, rows, nsup, dabs.d(), g->basis_area, dx.d());
        LAUNCH_OK();
    }
    const bool filt = g->x_filter[0].radius >= 0 || g->x_filter[1].radius >= 0;
    const double* xf = dx.d();
    if (filt) {
        HIPDRT_CHECK(dxf.alloc(nx * sizeof(double)));
        TRY(plain_gaussian_device(st, dx.d(), rows, nsup, g->x_filter, dxf.d()));
        xf = dxf.d();
    }

    // ---- 2: f, fxx ----
    DevBuf dls, dle, dE0, dE2, df, dfxx, dvf, dvxx, dvf2, dvxx2, dext, dpk, dpk2, dpeak, dcurv;
    const double *vf = nullptr, *vxx = nullptr;
    if (want_rows) {
        TRY(upload(dls, g->ln_tau_sup, (size_t)nsup * sizeof(double), st));
        TRY(upload(dle, g->ln_tau_eval, (size_t)neval * sizeof(double), st));
        HIPDRT_CHECK(dE0.alloc((size_t)neval * nsup * sizeof(double))); HIPDRT_CHECK(dE2.alloc((size_t)neval * nsup * sizeof(double)));
        TRY(func_eval_dev(st, dls.d(), nsup, dle.d(), neval, g->epsilon, 0, 1.0, dE0.d(), nsup));
        TRY(func_eval_dev(st, dls.d(), nsup, dle.d(), neval, g->epsilon, 2, 1.0, dE2.d(), nsup));
        HIPDRT_CHECK(df.alloc(ne * sizeof(double))); HIPDRT_CHECK(dfxx.alloc(ne * sizeof(double)));
        launch_apply_rows(st, rows, nsup, xf, nsup, 0, neval, dE0.d(), nsup, nullptr, nullptr, df.d(), neval);
        launch_apply_rows(st, rows, nsup, xf, nsup, 0, neval, dE2.d(), nsup, nullptr, nullptr, dfxx.d(), neval);
        LAUNCH_OK();
    }

    // ---- 3: variances and probabilities ----
    const bool clamp = stored && g->ext != nullptr;
    if (want_var || want_prob) {
        TRY(upload(dvf, g->f_var, ne * sizeof(double), st));
        TRY(upload(dvxx, g->fxx_var, ne * sizeof(double), st));
        vf = dvf.d(); vxx = dvxx.d();
        if (clamp) TRY(upload(dext, g->ext, (size_t)rows * 2 * sizeof(int), st));
        const bool clamp_first = stored && (filt || !want_prob);     // the clamp in a kernel of its own, then the filter
        if (clamp_first && clamp) TRY(launch_clamp(st, rows, neval, dvf.d(), dvxx.d(), dext.i()));
        if (stored && filt) {
            HIPDRT_CHECK(dvf2.alloc(ne * sizeof(double))); HIPDRT_CHECK(dvxx2.alloc(ne * sizeof(double)));
            TRY(plain_gaussian_device(st, dvf.d(), rows, neval, g->x_filter, dvf2.d()));
            TRY(plain_gaussian_device(st, dvxx.d(), rows, neval, g->x_filter, dvxx2.d()));
            vf = dvf2.d(); vxx = dvxx2.d();
        }
        const bool spread = peak_prob && g->spread.radius >= 0;
        MapProbArgs a{};
        a.n = neval; a.f = df.d(); a.fxx = dfxx.d(); a.vf = vf; a.vxx = vxx;
        a.ext = clamp && !clamp_first ? dext.i() : nullptr;
        a.search = g->search; a.height = g->height; a.prominence = g->prominence; a.sign_now = spread ? 0 : 1;
        if (peak_prob) {
            HIPDRT_CHECK(dpeak.alloc(ne * sizeof(double)));
            if (spread) { HIPDRT_CHECK(dpk.alloc(ne * sizeof(double))); HIPDRT_CHECK(dpk2.alloc(ne * sizeof(double))); }
            a.pk = spread ? dpk.d() : dpeak.d();
        }
        if (curv_prob) { HIPDRT_CHECK(dcurv.alloc(ne * sizeof(double))); a.curv = dcurv.d(); }
        if (a.ext) {                                     // the clamped rows leave through the kernel
            HIPDRT_CHECK(dvf2.alloc(ne * sizeof(double))); HIPDRT_CHECK(dvxx2.alloc(ne * sizeof(double)));
            a.vf_out = dvf2.d(); a.vxx_out = dvxx2.d();
            vf = dvf2.d(); vxx = dvxx2.d();
        }
        if (a.pk || a.curv) TRY(launch_map_prob(st, rows, a));
        // ---- 4: spread and sign ----
        if (spread) {
            hipdrt_filter_table tabs[2] = {{nullptr, -1}, g->spread};
            TRY(plain_gaussian_device(st, dpk.d(), rows, neval, tabs, dpk2.d()));
            hipLaunchKernelGGL(spread_sign_kernel, dim3((ne + 255) / 256), dim3(256), 0, st, ne, dpk2.d(), g->spread_factor, df.d(),
                               dpeak.d());
            LAUNCH_OK();
        }
    }

    // ---- the download ----
    auto back = [&](double* host, const double* dev, size_t count) -> int {
        if (host) HIPDRT_CHECK(hipMemcpyAsync(host, dev, count * sizeof(double), hipMemcpyDeviceToHost, st));
        return HIPDRT_OK;
    };
    TRY(back(x_out, xf, nx));
    TRY(back(f, df.d(), ne));
    TRY(back(fxx, dfxx.d(), ne));
    TRY(back(f_var_out, vf, ne));
    TRY(back(fxx_var_out, vxx, ne));
    TRY(back(peak_prob, dpeak.d(), ne));
    TRY(back(curv_prob, dcurv.d(), ne));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

// test hook (include/hipdrt_debug.h): stage 3 alone -- clamp_kernel and / or map_prob_kernel through the launchers the entry point
// uses, on host rows; every in and out array between borders of marker bytes
extern "C" int hipdrt_debug_map_prob(hipdrt_ctx* ctx, int rows, int n, const double* f, const double* fxx, const double* vf,
                                     const double* vxx, const int* ext, int clamp_first, int search, double height,
                                     double prominence, int sign_now, double* pk, double* curv, double* vf_out,
                                     double* vxx_out) try {
    HIPDRT_REQUIRE(ctx && vf && vxx, "NULL pointer");
    HIPDRT_REQUIRE(rows >= 1 && n >= 1 && (long long)rows * n < (1LL << 30), "rows, n >= 1, rows * n < 2^30");
    const bool prob = pk || curv;
    HIPDRT_REQUIRE(!prob || (f && fxx), "the probabilities need the f and fxx rows");
    HIPDRT_REQUIRE(prob || (clamp_first && ext), "nothing to launch: no probability row and no clamp kernel");
    HIPDRT_REQUIRE(!clamp_first || ext, "clamp_first needs ext");
    HIPDRT_REQUIRE(search >= -1 && search <= 1, "search must be 1, -1 or 0 (two passes)");
    HIPDRT_REQUIRE(std::isfinite(height) && std::isfinite(prominence), "height and prominence must be finite");
    if (ext) TRY(check_ext(ext, rows, n));
    size_t lds;
    if (prob) TRY(map_prob_lds_check(n, &lds));
    hipStream_t st; TRY(enter(ctx, &st));
    const size_t bn = (size_t)rows * n;
    MapProbArgs a{};
    a.n = n; a.search = search; a.height = height; a.prominence = prominence; a.sign_now = sign_now ? 1 : 0;
    GuardedOuts g;
    TRY(g.in("f", f, bn, a.f, st)); TRY(g.in("fxx", fxx, bn, a.fxx, st));
    // the variance rows are in/out when the clamp kernel runs first: it works in place, as on the entry point's uploaded rows
    Guarded gvf, gvxx;
    TRY(gvf.up_in("vf", vf, bn * sizeof(double), st)); TRY(gvxx.up_in("vxx", vxx, bn * sizeof(double), st));
    a.vf = gvf.dd(); a.vxx = gvxx.dd();
    const int* dext = nullptr;
    TRY(g.in("ext", ext, (size_t)rows * 2, dext, st));
    if (clamp_first) TRY(launch_clamp(st, rows, n, gvf.dd(), gvxx.dd(), dext));
    else a.ext = dext;
    TRY(g.want("pk", pk, bn, a.pk, st)); TRY(g.want("curv", curv, bn, a.curv, st));
    if (!clamp_first) { TRY(g.want("vf_out", vf_out, bn, a.vf_out, st)); TRY(g.want("vxx_out", vxx_out, bn, a.vxx_out, st)); }
    if (prob) TRY(launch_map_prob(st, rows, a));
    TRY(gvf.fetch(st)); TRY(gvxx.fetch(st));
    TRY(g.back(st));
    TRY(gvf.check()); TRY(gvxx.check());
    if (clamp_first && vf_out) std::memcpy(vf_out, gvf.data(), bn * sizeof(double));
    if (clamp_first && vxx_out) std::memcpy(vxx_out, gvxx.data(), bn * sizeof(double));
    return HIPDRT_OK;
} HIPDRT_CATCH
