// hipdrt_map_filter (include/hipdrt.h): mapping.ndx.filter_ndx without groups on one (rows, cols) array -- the iterative,
// optionally curvature-adaptive Gaussian filter of hybdrt/filters/_filters.py, stated in numpy in hipdrt/filters/ndfilters.py.
//
// The whole chain is separable stencils, element-wise maps and global reductions over arrays that stay on the device:
//   filter_pass_kernel   one 1-D correlation along axis 0 or 1 with scipy's 'reflect' boundary and symmetric summation order
//                        y[i] w0 + sum_{j = r .. 1} (y[i - j] + y[i + j]) w_j, for one operand or for the pair of a masked filter
//                        (a w, w share table and index arithmetic); the first pass of a filter forms its operands as it loads
//                        (`pre`), the last one applies the epilogue (`post`: the division of masked_filter, a - f(a w) / f(w),
//                        rms_filter's tail, the curvature normalisation, the sigma formula).  With a sigma field it is
//                        nonuniform_gaussian_filter1d: every element evaluates only the nodes that carry weight.
//   reduce kernels       mean, then sum of squared deviations (np.std), or min / max, in a fixed order
//   weight_kernel        exp(-(dev / (nstd dev_rms + 0.1 std(dev)))^6), weights[nan] = 0
// The drivers (iterate_gaussian_weights, iterative_gaussian_filter, get_adaptive_sigmas) are host code below that sequences the
// launches on the context's stream.  Compiled with -ffp-contract=off: every product and sum rounds as numpy's does.
#include <cfloat>
#include <cmath>
#include <memory>

#include "debug_guard.hpp"
#include "map_filter_dev.hpp"
#include "plan.hpp"

namespace hipdrt {
namespace {

constexpr int TILE_C = 64;           // columns of a tile: consecutive threads take consecutive columns in either axis
constexpr int TILE_R0 = 32;          // rows of an axis-0 tile (a strip of 64 columns with its row halo in LDS)
constexpr int TILE_R1 = 4;           // rows of an axis-1 tile (64 columns of 4 rows with their column halo)
constexpr size_t LDS_BUDGET = 65536; // a window that does not fit is read through the caches instead (same sums, same order)

enum Pre { PRE_NONE = 0, PRE_MUL, PRE_MULSQ, PRE_ABSDIV };
enum Post { POST_NONE = 0, POST_DIV, POST_RMSDIV, POST_DEV, POST_SIGMA, POST_CURVNORM };

struct NodeArgs {
    int K;
    double node[HIPDRT_MAP_FILTER_MAX_NODES];
    double node_delta, floor;
    int radius[HIPDRT_MAP_FILTER_MAX_NODES];
    int woff[HIPDRT_MAP_FILTER_MAX_NODES];
    const double* w;
};

struct PassArgs {
    const double *in0, *in1;   // in1 null: one operand
    double *out0, *out1;       // out1 null unless post == POST_NONE with two operands
    int R, C, axis;
    int pre, post;
    double div;                // every sum is divided by this (the box filter's size; 1 otherwise)
    const double *e0, *e1;     // POST_RMSDIV: dev and w of the first pass; POST_DEV: a; POST_CURVNORM: a_smooth
    const double* sp;          // device scalar: PRE_ABSDIV |in0 / *sp|, POST_CURVNORM a0 / (|e0| + *sp)
    double p0, p1;             // POST_RMSDIV: n, n / (n - 1); POST_SIGMA: k_factor, c
    const double* w;           // table w[0 .. r] (sigma == null)
    int r;
    const double* sigma;       // non-null: nonuniform filter with the nodes of NodeArgs
    int tile_r, rstage, lds;   // rows per tile, staged halo radius (>= every radius used), 1: window staged in LDS
};

__device__ __forceinline__ int reflect_index(int i, int n) {
    // scipy 'reflect' (d c b a | a b c d | d c b a): period 2 n, mirrored about the half-sample edges, any distance
    if (i < 0) i = -i - 1;
    if (i >= n) { i %= 2 * n; if (i >= n) i = 2 * n - 1 - i; }
    return i;
}

__device__ __forceinline__ void load_pair(const PassArgs& a, int gr, int gc, double& v0, double& v1) {
    const size_t i = (size_t)gr * a.C + gc;
    double p = a.in0[i], q = a.in1 ? a.in1[i] : 0.0;
    switch (a.pre) {
        case PRE_MUL: p = p * q; break;
        case PRE_MULSQ: p = p * q; p = p * p; q = q * q; break;
        case PRE_ABSDIV: p = fabs(p / *a.sp); break;
        default: break;
    }
    v0 = p; v1 = q;
}

__global__ __launch_bounds__(256) void filter_pass_kernel(PassArgs a, NodeArgs nd) {
    extern __shared__ double lds[];
    const int tid = threadIdx.x;
    const int r0 = blockIdx.x * a.tile_r, c0 = blockIdx.y * TILE_C;
    const int hr = a.axis == 0 ? a.rstage : 0, hc = a.axis == 1 ? a.rstage : 0;
    const int WR = a.tile_r + 2 * hr, WC = TILE_C + 2 * hc, WN = WR * WC;
    const bool two = a.in1 != nullptr;
    if (a.lds) {
        for (int e = tid; e < WN; e += 256) {
            int gr = r0 - hr + e / WC, gc = c0 - hc + e % WC;
            bool valid;
            if (a.axis == 0) { gr = reflect_index(gr, a.R); valid = gc < a.C; }
            else { gc = reflect_index(gc, a.C); valid = gr < a.R; }
            double v0 = 0.0, v1 = 0.0;
            if (valid) load_pair(a, gr, gc, v0, v1);
            lds[e] = v0;
            if (two) lds[WN + e] = v1;
        }
        __syncthreads();
    }
    for (int e = tid; e < a.tile_r * TILE_C; e += 256) {
        const int lr = e / TILE_C, lc = e % TILE_C, gr = r0 + lr, gc = c0 + lc;
        if (gr >= a.R || gc >= a.C) continue;
        const size_t gi = (size_t)gr * a.C + gc;
        // the operands at offset j along the axis
        auto at = [&](int j, double& v0, double& v1) {
            if (a.lds) {
                const int k = (lr + hr + (a.axis == 0 ? j : 0)) * WC + lc + hc + (a.axis == 1 ? j : 0);
                v0 = lds[k];
                v1 = two ? lds[WN + k] : 0.0;
            } else if (a.axis == 0) {
                load_pair(a, reflect_index(gr + j, a.R), gc, v0, v1);
            } else {
                load_pair(a, gr, reflect_index(gc + j, a.C), v0, v1);
            }
        };
        double c0v, c1v;
        at(0, c0v, c1v);
        auto corr = [&](const double* __restrict__ w, int r, double& s0, double& s1) {
            s0 = c0v * w[0];
            s1 = c1v * w[0];
            for (int j = r; j >= 1; --j) {
                double l0, l1, h0, h1;
                at(-j, l0, l1);
                at(j, h0, h1);
                s0 += (l0 + h0) * w[j];
                s1 += (l1 + h1) * w[j];
            }
        };
        double a0, a1;
        if (a.sigma) {
            double sg = fmax(a.sigma[gi], 1e-8);
            if (sg < nd.floor) sg = nd.floor;
            a0 = 0.0; a1 = 0.0;
            for (int k = 0; k < nd.K; ++k) {
                double nw = fabs(log(sg / nd.node[k])) / nd.node_delta;
                if (nw >= 1.0) nw = 1.0;
                nw = 1.0 - nw;
                if (nw == 0.0) continue;               // exact zero: adds nothing in the reference either
                double v0 = c0v, v1 = c1v;
                if (nd.radius[k] >= 0) corr(nd.w + nd.woff[k], nd.radius[k], v0, v1);
                a0 += v0 * nw;
                a1 += v1 * nw;
            }
        } else {
            corr(a.w, a.r, a0, a1);
        }
        if (a.div != 1.0) { a0 = a0 / a.div; a1 = a1 / a.div; }
        switch (a.post) {
            case POST_DIV: a.out0[gi] = a0 / a1; break;
            case POST_DEV: a.out0[gi] = a.e0[gi] - a0 / a1; break;
            case POST_RMSDIV: {
                // rms_filter(..., empty=True): a2_mean -= a2 / n; a2_mean *= n / (n - 1); clip at 0; sqrt
                double x0 = a.e0[gi] * a.e1[gi], x1 = a.e1[gi];
                x0 = x0 * x0; x1 = x1 * x1;
                double m0 = (a0 - x0 / a.p0) * a.p1, m1 = (a1 - x1 / a.p0) * a.p1;
                if (m0 < 0.0) m0 = 0.0;
                if (m1 < 0.0) m1 = 0.0;
                a.out0[gi] = sqrt(m0) / sqrt(m1);
                break;
            }
            case POST_SIGMA: a.out0[gi] = sqrt(a.p0 / (fabs(a0) + a.p1)); break;
            case POST_CURVNORM: a.out0[gi] = a0 / (fabs(a.e0[gi]) + *a.sp); break;
            default:
                a.out0[gi] = a0;
                if (a.out1) a.out1[gi] = a1;
                break;
        }
    }
}

// x = nan_to_num(a), w = (init or 1) with 0 at the NaNs (mask_nans); otherwise x = a, w = init or 1
__global__ __launch_bounds__(256) void prep_kernel(const double* __restrict__ a, size_t n, int mask_nans,
                                                   const double* __restrict__ init, double* __restrict__ x,
                                                   double* __restrict__ w) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    double v = a[i], wt = init ? init[i] : 1.0;
    if (mask_nans) {
        if (isnan(v)) { v = 0.0; wt = 0.0; }
        else if (isinf(v)) v = v > 0 ? DBL_MAX : -DBL_MAX;
    }
    x[i] = v;
    w[i] = wt;
}

__global__ __launch_bounds__(256) void weight_kernel(const double* __restrict__ dev, const double* __restrict__ rms,
                                                     const double* __restrict__ std_dev, double nstd,
                                                     const double* __restrict__ a, int mask_nans, size_t n,
                                                     double* __restrict__ w) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const double t = dev[i] / (nstd * rms[i] + 0.1 * *std_dev);
    double v = exp(-pow(t, 6.0));
    if (mask_nans && isnan(a[i])) v = 0.0;
    w[i] = v;
}

__global__ __launch_bounds__(256) void fill_kernel(double* __restrict__ x, size_t n, double v) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) x[i] = v;
}

// fixed-order reductions: block b sums its grid-strided elements thread by thread, then a binary tree over the 256 threads;
// reduce_final does the same over the partials.  mode 0: sum x; 1: sum (x - *mean)^2; 2: min and max (partial[b], partial[G + b])
enum { RED_SUM = 0, RED_SQDEV, RED_MINMAX };
__device__ __forceinline__ void block_tree(double* s0, double* s1, int tid, int mode) {
    for (int h = 128; h >= 1; h >>= 1) {
        __syncthreads();
        if (tid < h) {
            if (mode == RED_MINMAX) { s0[tid] = fmin(s0[tid], s0[tid + h]); s1[tid] = fmax(s1[tid], s1[tid + h]); }
            else s0[tid] = s0[tid] + s0[tid + h];
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(256) void reduce_partial(const double* __restrict__ x, size_t n, int mode,
                                                      const double* __restrict__ mean, double* __restrict__ partial) {
    __shared__ double s0[256], s1[256];
    const int tid = threadIdx.x;
    const size_t stride = (size_t)gridDim.x * 256;
    double v0 = mode == RED_MINMAX ? INFINITY : 0.0, v1 = -INFINITY;
    const double mu = mode == RED_SQDEV ? *mean : 0.0;
    for (size_t i = (size_t)blockIdx.x * 256 + tid; i < n; i += stride) {
        const double v = x[i];
        if (mode == RED_SUM) v0 += v;
        else if (mode == RED_SQDEV) { const double d = v - mu; v0 += d * d; }
        else { v0 = fmin(v0, v); v1 = fmax(v1, v); }
    }
    s0[tid] = v0; s1[tid] = v1;
    block_tree(s0, s1, tid, mode);
    if (tid == 0) { partial[blockIdx.x] = s0[0]; if (mode == RED_MINMAX) partial[gridDim.x + blockIdx.x] = s1[0]; }
}

// out[0] = mean (mode 0), sqrt(sum / n) (mode 1: np.std), or out[0], out[1] = min, max (mode 2)
__global__ __launch_bounds__(256) void reduce_final(const double* __restrict__ partial, int G, size_t n, int mode,
                                                    double* __restrict__ out) {
    __shared__ double s0[256], s1[256];
    const int tid = threadIdx.x;
    double v0 = mode == RED_MINMAX ? INFINITY : 0.0, v1 = -INFINITY;
    for (int i = tid; i < G; i += 256) {
        if (mode == RED_MINMAX) { v0 = fmin(v0, partial[i]); v1 = fmax(v1, partial[G + i]); }
        else v0 += partial[i];
    }
    s0[tid] = v0; s1[tid] = v1;
    block_tree(s0, s1, tid, mode);
    if (tid == 0) {
        if (mode == RED_SUM) out[0] = s0[0] / (double)n;
        else if (mode == RED_SQDEV) out[0] = sqrt(s0[0] / (double)n);
        else { out[0] = s0[0]; out[1] = s1[0]; }
    }
}

struct Tab {                      // a half table on the device
    DevBuf buf;
    int r = -1;
};

struct Step {                     // one pass of a separable filter: a table, or the nodes of a sigma field
    int axis;                     // physical axis
    const Tab* tab = nullptr;
    const double* sigma = nullptr;
    NodeArgs nd{};
    int rmax = 0;
    double div = 1.0;
};

struct MapFilter {
    hipStream_t st;
    const hipdrt_map_filter_args* g;
    int R, C, nax;                // physical shape (a 1-D array is one row) and number of logical axes
    int phys[2];                  // physical axis of logical axis l
    size_t n, bytes;
    DevBuf raw, x, w, t0, t1, u0, u1, dev, rms, smooth, curv, sig[2], scal, partial, winit;
    Tab gauss[2], egauss[2], box[2], pgauss[2], pempty[2], curvtab, ident;
    std::vector<std::unique_ptr<DevBuf>> node_bufs;
    static constexpr int G = 1024;
    long long launches = 0, arrays = 0;           // hipdrt_debug_map_filter_stats
    void count(int kernels, int array_moves) { launches += kernels; arrays += array_moves; }

    int upload_tab(Tab& t, const hipdrt_filter_table& h) {
        t.r = h.radius;
        if (h.radius < 0) return HIPDRT_OK;
        HIPDRT_REQUIRE(h.w, "a filter table with radius >= 0 needs its weights");
        return upload(t.buf, h.w, (size_t)(h.radius + 1) * sizeof(double), st);
    }

    int pass(const Step& s, const double* in0, const double* in1, int pre, double* out0, double* out1, int post,
             const double* e0, const double* e1, const double* sp, double p0, double p1) {
        PassArgs a{};
        a.in0 = in0; a.in1 = in1; a.out0 = out0; a.out1 = out1;
        a.R = R; a.C = C; a.axis = s.axis; a.pre = pre; a.post = post; a.div = s.div;
        a.e0 = e0; a.e1 = e1; a.sp = sp; a.p0 = p0; a.p1 = p1;
        a.sigma = s.sigma;
        if (!s.sigma) { a.w = s.tab->buf.d(); a.r = s.tab->r; }
        a.rstage = s.sigma ? s.rmax : s.tab->r;
        a.tile_r = s.axis == 0 ? TILE_R0 : TILE_R1;
        const size_t wr = a.tile_r + (s.axis == 0 ? 2 * (size_t)a.rstage : 0), wc = TILE_C + (s.axis == 1 ? 2 * (size_t)a.rstage : 0);
        const size_t lds_bytes = wr * wc * sizeof(double) * (in1 ? 2 : 1);
        a.lds = lds_bytes <= LDS_BUDGET;
        const dim3 grid((R + a.tile_r - 1) / a.tile_r, (C + TILE_C - 1) / TILE_C);
        hipLaunchKernelGGL(filter_pass_kernel, grid, dim3(256), a.lds ? lds_bytes : 0, st, a, s.nd);
        count(1, 1 + (in1 ? 1 : 0) + (s.sigma ? 1 : 0) + (post == POST_RMSDIV ? 2 : (post == POST_DEV || post == POST_CURVNORM) ? 1 : 0)
                     + 1 + (out1 ? 1 : 0));
        LAUNCH_OK();
        return HIPDRT_OK;
    }

    // a separable filter: the steps in order, `pre` on the first one's loads, `post` on the last one's results.  No step: the
    // identity table, so that pre and post still apply.  Intermediates go through (u0, u1) and (t0, t1) in turn.
    int run(std::vector<Step> steps, const double* in0, const double* in1, int pre, double* out0, double* out1, int post,
            const double* e0 = nullptr, const double* e1 = nullptr, const double* sp = nullptr, double p0 = 0, double p1 = 0) {
        if (steps.empty()) { Step s; s.axis = 1; s.tab = &ident; steps.push_back(s); }
        const double *c0 = in0, *c1 = in1;
        for (size_t k = 0; k < steps.size(); ++k) {
            const bool first = k == 0, last = k + 1 == steps.size();
            double* o0 = last ? out0 : (k % 2 ? t0.d() : u0.d());
            double* o1 = last ? out1 : (in1 ? (k % 2 ? t1.d() : u1.d()) : nullptr);
            TRY(pass(steps[k], c0, c1, first ? pre : PRE_NONE, o0, o1, last ? post : POST_NONE, e0, e1, sp, p0, p1));
            c0 = o0; c1 = o1;
        }
        return HIPDRT_OK;
    }

    std::vector<Step> table_steps(const Tab* tabs, double div = 1.0) {
        std::vector<Step> v;
        for (int l = 0; l < nax; ++l)
            if (tabs[l].r >= 0) { Step s; s.axis = phys[l]; s.tab = &tabs[l]; s.div = div; v.push_back(s); }
        return v;
    }

    int reduce(const double* xs, int mode, const double* mean, double* out) {
        const int blocks = (int)std::min<size_t>(G, (n + 255) / 256);
        hipLaunchKernelGGL(reduce_partial, dim3(blocks), dim3(256), 0, st, xs, n, mode, mean, partial.d());
        hipLaunchKernelGGL(reduce_final, dim3(1), dim3(256), 0, st, partial.d(), blocks, n, mode, out);
        count(2, 1);
        LAUNCH_OK();
        return HIPDRT_OK;
    }
    // np.std into scal[slot] (scal[slot + 1] holds the mean)
    int std_of(const double* xs, int slot) {
        TRY(reduce(xs, RED_SUM, nullptr, scal.d() + slot + 1));
        return reduce(xs, RED_SQDEV, scal.d() + slot + 1, scal.d() + slot);
    }
    int read_scal(int slot, int count, double* host) {
        HIPDRT_CHECK(hipMemcpyAsync(host, scal.d() + slot, count * sizeof(double), hipMemcpyDeviceToHost, st));
        HIPDRT_CHECK(hipStreamSynchronize(st));
        return HIPDRT_OK;
    }

    // the steps of adaptive_gaussian_filter(sigmas=sig, empty=): per axis with max_sigma > 0 and max(sigma) > 0, the node tables
    // the caller builds from the extremes of the field
    int node_steps(int empty, std::vector<Step>& v) {
        for (int l = 0; l < nax; ++l) {
            if (!(g->max_sigma[l] > 0)) continue;
            TRY(reduce(sig[l].d(), RED_MINMAX, nullptr, scal.d() + 4));
            double mm[2];
            TRY(read_scal(4, 2, mm));
            if (!(mm[1] > 0)) continue;
            hipdrt_node_tables nt{};
            HIPDRT_REQUIRE(g->nodes(g->user, l, empty, std::max(mm[0], 1e-8), std::max(mm[1], 1e-8), &nt) == 0, "the node-table callback failed");
            HIPDRT_REQUIRE(nt.count >= 1 && nt.count <= HIPDRT_MAP_FILTER_MAX_NODES, "1 .. 16 sigma nodes");
            Step s; s.axis = phys[l]; s.sigma = sig[l].d();
            s.nd.K = nt.count; s.nd.node_delta = nt.node_delta; s.nd.floor = nt.floor;
            std::vector<double> pool;
            for (int k = 0; k < nt.count; ++k) {
                s.nd.node[k] = nt.node[k]; s.nd.radius[k] = nt.radius[k]; s.nd.woff[k] = (int)pool.size();
                if (nt.radius[k] < 0) continue;
                HIPDRT_REQUIRE(nt.w[k], "a node with radius >= 0 needs its table");
                pool.insert(pool.end(), nt.w[k], nt.w[k] + nt.radius[k] + 1);
                s.rmax = std::max(s.rmax, nt.radius[k]);
            }
            if (pool.empty()) pool.push_back(1.0);
            node_bufs.emplace_back(new DevBuf());
            TRY(upload(*node_bufs.back(), pool.data(), pool.size() * sizeof(double), st));
            HIPDRT_CHECK(hipStreamSynchronize(st));      // `pool` goes out of scope
            s.nd.w = node_bufs.back()->d();
            v.push_back(s);
        }
        return HIPDRT_OK;
    }

    // get_adaptive_sigmas(x, empty=, weights=wt): sig[l] for every logical axis
    int sigmas(int empty, const double* wt) {
        const Tab* pre = empty ? pempty : pgauss;
        bool any_pre = false;
        for (int l = 0; l < nax; ++l) any_pre |= pre[l].r >= 0;
        const double* sm = x.d();
        if (any_pre) {                   // np.max(presmooth_sigma) > 0
            if (wt) TRY(run(table_steps(pre), x.d(), wt, PRE_MUL, smooth.d(), nullptr, POST_DIV));
            else TRY(run(table_steps(pre), x.d(), nullptr, PRE_NONE, smooth.d(), nullptr, POST_NONE));
            sm = smooth.d();
        }
        bool std_done = false;
        for (int l = 0; l < nax; ++l) {
            if (!(g->max_sigma[l] > 0)) { HIPDRT_CHECK(hipMemsetAsync(sig[l].p, 0, bytes, st)); count(1, 1); continue; }
            if (!std_done) { TRY(std_of(sm, 0)); std_done = true; }
            Step cs; cs.axis = phys[l]; cs.tab = &curvtab;
            TRY(run({cs}, sm, nullptr, PRE_NONE, curv.d(), nullptr, POST_CURVNORM, sm, nullptr, scal.d() + 0));
            TRY(std_of(curv.d(), 2));
            double sc;
            TRY(read_scal(2, 1, &sc));
            if (sc == 0.0) {
                hipLaunchKernelGGL(fill_kernel, dim3((n + 255) / 256), dim3(256), 0, st, sig[l].d(), n, g->max_sigma[l]);
                count(1, 1);
                LAUNCH_OK();
                continue;
            }
            const double k = g->k_factor[l], c = k / (g->max_sigma[l] * g->max_sigma[l]);
            TRY(run(table_steps(pgauss), curv.d(), nullptr, PRE_ABSDIV, sig[l].d(), nullptr, POST_SIGMA, nullptr, nullptr,
                    scal.d() + 2, k, c));
        }
        return HIPDRT_OK;
    }

    // masked (wt != null) or plain filter of x into out0 with the final or the empty tables / nodes; post: POST_DIV or POST_DEV
    int smooth_x(int empty, const double* wt, double* out0, int post) {
        std::vector<Step> steps;
        if (g->adaptive) TRY(node_steps(empty, steps));
        else steps = table_steps(empty ? egauss : gauss);
        if (wt) return run(steps, x.d(), wt, PRE_MUL, out0, nullptr, post, x.d());
        return run(steps, x.d(), nullptr, PRE_NONE, out0, nullptr, POST_NONE);
    }

    int iterate_weights() {
        const double nbox = std::pow((double)g->box_size, (double)nax);
        for (int it = 0; it < g->iter; ++it) {
            if (g->adaptive) TRY(sigmas(1, w.d()));
            TRY(smooth_x(1, w.d(), dev.d(), POST_DEV));
            TRY(run(table_steps(box, (double)g->box_size), dev.d(), w.d(), PRE_MULSQ, rms.d(), nullptr, POST_RMSDIV, dev.d(), w.d(),
                    nullptr, nbox, nbox / (nbox - 1.0)));
            TRY(std_of(dev.d(), 0));
            hipLaunchKernelGGL(weight_kernel, dim3((n + 255) / 256), dim3(256), 0, st, dev.d(), rms.d(), scal.d() + 0, g->nstd,
                               raw.d(), g->mask_nans, n, w.d());
            count(1, 4);
            LAUNCH_OK();
        }
        return HIPDRT_OK;
    }
};

}  // namespace

// map_filter_dev.hpp: masked_filter(nan_to_num(a), ~isnan(a), gaussian_filter) on device buffers -- prep_kernel and the fused
// masked passes above, for impute_nans of the badness chain (map_rank.hip)
int masked_gaussian_device(hipStream_t st, const double* a, int R, int C, const hipdrt_filter_table* tabs, double* out) {
    MapFilter m;
    m.st = st; m.g = nullptr;
    m.R = R; m.C = C; m.nax = 2; m.phys[0] = 0; m.phys[1] = 1;
    HIPDRT_REQUIRE((C + TILE_C - 1) / TILE_C <= 65535, "at most 65535 * 64 entries along a row");
    m.n = (size_t)R * C; m.bytes = m.n * sizeof(double);
    for (DevBuf* b : {&m.x, &m.w, &m.t0, &m.t1, &m.u0, &m.u1}) HIPDRT_CHECK(b->alloc(m.bytes));
    const double one = 1.0;
    TRY(upload(m.ident.buf, &one, sizeof(double), st)); m.ident.r = 0;
    for (int l = 0; l < 2; ++l) TRY(m.upload_tab(m.gauss[l], tabs[l]));
    hipLaunchKernelGGL(prep_kernel, dim3((m.n + 255) / 256), dim3(256), 0, st, a, m.n, 1, (const double*)nullptr, m.x.d(), m.w.d());
    LAUNCH_OK();
    TRY(m.run(m.table_steps(m.gauss), m.x.d(), m.w.d(), PRE_MUL, out, nullptr, POST_DIV));
    HIPDRT_CHECK(hipStreamSynchronize(st));          // the work buffers and `one` go out of scope
    return HIPDRT_OK;
}

// map_filter_dev.hpp: scipy.ndimage.gaussian_filter(a, sigma, mode='reflect') on device buffers -- the same passes without a mask: a
// NaN spreads over the window that holds it, as scipy spreads it.  Every output element is one accumulator summed in the symmetric
// order of filter_pass_kernel, whatever the shape of the launch.
int plain_gaussian_device(hipStream_t st, const double* a, int R, int C, const hipdrt_filter_table* tabs, double* out) {
    MapFilter m;
    m.st = st; m.g = nullptr;
    m.R = R; m.C = C; m.nax = 2; m.phys[0] = 0; m.phys[1] = 1;
    HIPDRT_REQUIRE(R >= 1 && C >= 1 && a != out, "plain filter: rows, cols >= 1 and distinct buffers");
    HIPDRT_REQUIRE((C + TILE_C - 1) / TILE_C <= 65535, "at most 65535 * 64 entries along a row");
    m.n = (size_t)R * C; m.bytes = m.n * sizeof(double);
    const double one = 1.0;
    TRY(upload(m.ident.buf, &one, sizeof(double), st)); m.ident.r = 0;
    for (int l = 0; l < 2; ++l) TRY(m.upload_tab(m.gauss[l], tabs[l]));
    if (m.gauss[0].r >= 0 && m.gauss[1].r >= 0) HIPDRT_CHECK(m.u0.alloc(m.bytes));      // the intermediate of two passes
    TRY(m.run(m.table_steps(m.gauss), a, nullptr, PRE_NONE, out, nullptr, POST_NONE));
    HIPDRT_CHECK(hipStreamSynchronize(st));          // the work buffers and `one` go out of scope
    return HIPDRT_OK;
}

}  // namespace hipdrt

using namespace hipdrt;

extern "C" int hipdrt_map_filter(hipdrt_ctx* ctx, const hipdrt_map_filter_args* g, const double* a, double* out,
                                 double* weights_out, double* sigmas_out) try {
    HIPDRT_REQUIRE(ctx && g && a, "NULL pointer");
    HIPDRT_REQUIRE(g->ndim == 1 || g->ndim == 2, "ndim 1 or 2");
    HIPDRT_REQUIRE(g->rows >= 1 && g->cols >= 1 && (g->ndim == 2 || g->cols == 1), "rows, cols >= 1; cols == 1 with ndim == 1");
    HIPDRT_REQUIRE((long long)g->rows * g->cols < (1LL << 30), "rows * cols < 2^30");
    HIPDRT_REQUIRE(g->op == HIPDRT_MAP_FILTER || g->op == HIPDRT_MAP_SIGMAS, "op");
    const bool filter = g->op == HIPDRT_MAP_FILTER;
    HIPDRT_REQUIRE(!filter || out, "NULL pointer");
    HIPDRT_REQUIRE(filter || (g->adaptive && sigmas_out), "HIPDRT_MAP_SIGMAS needs adaptive = 1 and sigmas_out");
    HIPDRT_REQUIRE(!g->adaptive || g->nodes || !filter, "adaptive = 1 needs the node-table callback");
    HIPDRT_REQUIRE(!g->sigmas_in || (filter && g->adaptive && !g->iterative), "sigmas_in goes with a non-iterative adaptive filter");
    HIPDRT_REQUIRE(!(filter && g->iterative) || (g->iter >= 0 && g->box_size >= 3 && g->box_size % 2 == 1), "iter >= 0, odd box_size >= 3");
    hipStream_t st; TRY(enter(ctx, &st));

    MapFilter m;
    m.st = st; m.g = g;
    if (g->ndim == 1) { m.R = 1; m.C = g->rows; m.nax = 1; m.phys[0] = 1; m.phys[1] = 1; }
    else { m.R = g->rows; m.C = g->cols; m.nax = 2; m.phys[0] = 0; m.phys[1] = 1; }
    HIPDRT_REQUIRE((m.C + TILE_C - 1) / TILE_C <= 65535, "at most 65535 * 64 entries along a row");
    m.n = (size_t)m.R * m.C; m.bytes = m.n * sizeof(double);
    TRY(upload(m.raw, a, m.bytes, st));
    for (DevBuf* b : {&m.x, &m.w, &m.t0, &m.t1, &m.u0, &m.u1, &m.dev}) HIPDRT_CHECK(b->alloc(m.bytes));
    HIPDRT_CHECK(m.scal.alloc(8 * sizeof(double)));
    HIPDRT_CHECK(m.partial.alloc(2 * MapFilter::G * sizeof(double)));
    const double one = 1.0;
    TRY(upload(m.ident.buf, &one, sizeof(double), st)); m.ident.r = 0;
    for (int l = 0; l < m.nax; ++l) {
        if (g->adaptive && !g->sigmas_in) { TRY(m.upload_tab(m.pgauss[l], g->pre_gauss[l])); TRY(m.upload_tab(m.pempty[l], g->pre_empty[l])); }

        else if (filter) { TRY(m.upload_tab(m.gauss[l], g->gauss[l])); TRY(m.upload_tab(m.egauss[l], g->empty_gauss[l])); }
        if (filter && g->iterative) {
            TRY(m.upload_tab(m.box[l], g->box[l]));
            HIPDRT_REQUIRE(m.box[l].r == g->box_size / 2, "box radius == box_size / 2");
        }
    }
    if (g->adaptive) {
        if (!g->sigmas_in) {
            TRY(m.upload_tab(m.curvtab, g->curv));
            HIPDRT_REQUIRE(m.curvtab.r >= 0, "the order-2 table");
        }
        for (DevBuf* b : {&m.smooth, &m.curv, &m.sig[0], &m.sig[1]}) HIPDRT_CHECK(b->alloc(m.bytes));
    }
    if (filter && g->iterative) HIPDRT_CHECK(m.rms.alloc(m.bytes));
    if (g->init_weights) TRY(upload(m.winit, g->init_weights, m.bytes, st));
    hipEvent_t ev0, ev1;
    HIPDRT_CHECK(hipEventCreate(&ev0)); HIPDRT_CHECK(hipEventCreate(&ev1));
    struct EventGuard { hipEvent_t a, b; ~EventGuard() { (void)hipEventDestroy(a); (void)hipEventDestroy(b); } } guard{ev0, ev1};
    HIPDRT_CHECK(hipEventRecord(ev0, st));
    m.count(1, 3 + (g->init_weights ? 1 : 0));
    hipLaunchKernelGGL(prep_kernel, dim3((m.n + 255) / 256), dim3(256), 0, st, m.raw.d(), m.n, g->mask_nans,
                       g->init_weights ? m.winit.d() : nullptr, m.x.d(), m.w.d());
    LAUNCH_OK();
    // weights of the masked forms: the NaN mask, the caller's mask, or (iterative) the iterated weights; none: plain filters
    const bool masked = g->mask_nans || g->init_weights || (filter && g->iterative);
    const double* wt = masked ? m.w.d() : nullptr;

    if (!filter) {
        TRY(m.sigmas(g->empty, wt));
        HIPDRT_CHECK(hipEventRecord(ev1, st));
    } else {
        if (g->iterative) TRY(m.iterate_weights());
        if (g->sigmas_in) {
            for (int l = 0; l < m.nax; ++l)
                HIPDRT_CHECK(hipMemcpyAsync(m.sig[l].p, g->sigmas_in + (size_t)l * m.n, m.bytes, hipMemcpyHostToDevice, st));
        } else if (g->adaptive) {
            TRY(m.sigmas(0, wt));
        }
        TRY(m.smooth_x(g->sigmas_in ? g->empty : 0, wt, m.dev.d(), POST_DIV));
        HIPDRT_CHECK(hipEventRecord(ev1, st));
        HIPDRT_CHECK(hipMemcpyAsync(out, m.dev.p, m.bytes, hipMemcpyDeviceToHost, st));
        if (weights_out) HIPDRT_CHECK(hipMemcpyAsync(weights_out, m.w.p, m.bytes, hipMemcpyDeviceToHost, st));
    }
    if (sigmas_out && g->adaptive)
        for (int l = 0; l < m.nax; ++l)
            HIPDRT_CHECK(hipMemcpyAsync(sigmas_out + (size_t)l * m.n, m.sig[l].p, m.bytes, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    float ms = 0.f;
    HIPDRT_CHECK(hipEventElapsedTime(&ms, ev0, ev1));
    ctx->map_filter_stats[0] = (double)m.launches; ctx->map_filter_stats[1] = (double)m.arrays; ctx->map_filter_stats[2] = ms;
    return HIPDRT_OK;
} HIPDRT_CATCH

extern "C" int hipdrt_debug_map_filter_stats(hipdrt_ctx* ctx, double* stats) try {
    HIPDRT_REQUIRE(ctx && stats, "NULL pointer");
    for (int k = 0; k < 3; ++k) stats[k] = ctx->map_filter_stats[k];
    return HIPDRT_OK;
} HIPDRT_CATCH

// test hook (include/hipdrt_debug.h): plain_gaussian_device / masked_gaussian_device as map_rank.hip and map_predict.hip call them,
// on a host array; input and output between borders of marker bytes
extern "C" int hipdrt_debug_map_gaussian(hipdrt_ctx* ctx, const double* a, int R, int C, const hipdrt_filter_table* tabs, int masked,
                                         double* out) try {
    HIPDRT_REQUIRE(ctx && a && tabs && out, "NULL pointer");
    HIPDRT_REQUIRE(R >= 1 && C >= 1 && (long long)R * C < (1LL << 30), "rows, cols >= 1, rows * cols < 2^30");
    HIPDRT_REQUIRE(masked == 0 || masked == 1, "masked: 0 or 1");
    for (int l = 0; l < 2; ++l)
        HIPDRT_REQUIRE(tabs[l].radius < 0 || (tabs[l].w && tabs[l].radius < (1 << 20)), "a table with 0 <= radius < 2^20 needs its weights");
    hipStream_t st; TRY(enter(ctx, &st));
    const size_t n = (size_t)R * C;
    GuardedOuts g;
    const double* din = nullptr;
    double* dout = nullptr;
    TRY(g.in("a", a, n, din, st));
    TRY(g.want("out", out, n, dout, st));
    TRY(masked ? masked_gaussian_device(st, din, R, C, tabs, dout) : plain_gaussian_device(st, din, R, C, tabs, dout));
    return g.back(st);
} HIPDRT_CATCH

// test hook (include/hipdrt_debug.h): MapFilter::reduce / std_of alone on a host vector; x, the partials and the scalars between
// borders of marker bytes
extern "C" int hipdrt_debug_map_reduce(hipdrt_ctx* ctx, const double* x, long long n, int mode, double* out) try {
    HIPDRT_REQUIRE(ctx && x && out, "NULL pointer");
    HIPDRT_REQUIRE(n >= 1 && n < (1LL << 30), "1 <= n < 2^30");
    HIPDRT_REQUIRE(mode >= 0 && mode <= 2, "mode: 0 (mean), 1 (std and mean), 2 (min and max)");
    hipStream_t st; TRY(enter(ctx, &st));
    MapFilter m;
    m.st = st; m.g = nullptr;
    m.R = 1; m.C = (int)n; m.nax = 1; m.phys[0] = 1; m.phys[1] = 1;
    m.n = (size_t)n; m.bytes = m.n * sizeof(double);
    Guarded gx, gpart, gscal;
    std::vector<double> hscal(8, 0.0);
    TRY(gx.up_in("x", x, m.bytes, st));
    TRY(gpart.up_in("partial", nullptr, 2 * MapFilter::G * sizeof(double), st));
    TRY(gscal.up("scal", hscal.data(), hscal.size() * sizeof(double), st));
    m.partial.alias(gpart.buf, Guarded::G, gpart.bytes);
    m.scal.alias(gscal.buf, Guarded::G, gscal.bytes);
    if (mode == 0) TRY(m.reduce(gx.dd(), RED_SUM, nullptr, m.scal.d() + 1));
    else if (mode == 1) TRY(m.std_of(gx.dd(), 0));
    else TRY(m.reduce(gx.dd(), RED_MINMAX, nullptr, m.scal.d() + 4));
    for (Guarded* g : {&gx, &gpart, &gscal}) TRY(g->fetch(st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    for (Guarded* g : {&gx, &gpart, &gscal}) TRY(g->check());
    if (mode == 0) { out[0] = hscal[1]; out[1] = 0.0; }
    else if (mode == 1) { out[0] = hscal[0]; out[1] = hscal[1]; }
    else { out[0] = hscal[4]; out[1] = hscal[5]; }
    return HIPDRT_OK;
} HIPDRT_CATCH
