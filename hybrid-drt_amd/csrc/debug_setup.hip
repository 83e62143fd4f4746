// Test hooks of include/hipdrt_debug.h for what runs before the fit loop and after it (csrc/hyper.hip): launch_prep, launch_row_mask +
// launch_init_weights, launch_weight_method, launch_llh and the element-wise launchers, each run as it is on host arrays.  Every
// extent a kernel derives an address from is checked here: the kernels themselves trust their caller.  Every array a kernel may write
// sits between two borders of marker bytes (debug_guard.hpp).
#include <cmath>

#include "debug_guard.hpp"
#include "plan.hpp"

namespace {

using namespace hipdrt;

int finite_rows(const double* row, size_t count, const char* what) {
    if (row)
        for (size_t i = 0; i < count; ++i)
            if (!std::isfinite(row[i])) { set_error(std::string("invalid argument: non-finite input row (") + what + ")"); return HIPDRT_E_INVALID; }
    return HIPDRT_OK;
}

// what the four FitState hooks share: sizes checked, the state arrays that are given uploaded between borders, the matrices uploaded
struct SetupRun {
    const hipdrt_debug_setup_args* a;
    hipStream_t st = nullptr;
    FitState fs{};
    GuardedOuts g;
    DevBuf drm, dvmm, dvmm_iw, dzr, dzi, dqs;

    int sizes() const {
        HIPDRT_REQUIRE(a->B >= 1 && a->B <= 4096 && a->m >= 1 && a->m <= 8192 && a->n >= 1 && a->n <= 4096,
                       "1 <= B <= 4096, 1 <= m <= 8192, 1 <= n <= 4096");
        HIPDRT_REQUIRE(a->opts, "NULL pointer (opts)");
        HIPDRT_REQUIRE(!a->desc || (a->desc->num_chrono >= 0 && a->desc->num_chrono <= a->m), "0 <= num_chrono <= m");
        return HIPDRT_OK;
    }
    int matrices(bool want_rm, bool want_vmm, bool want_iw) {
        const int m = a->m;
        if (want_rm) {
            HIPDRT_REQUIRE(a->rm, "NULL pointer (rm)");
            HIPDRT_REQUIRE(a->ldrm >= a->n, "ldrm >= n");
            const size_t cnt = (size_t)(a->rm_batched ? a->B : 1) * m * a->ldrm;
            TRY(finite_rows(a->rm, cnt, "rm"));
            TRY(upload(drm, a->rm, cnt * sizeof(double), st));
            fs.rm = drm.d(); fs.rm_rw = drm.d();
        }
        if (want_vmm) {
            HIPDRT_REQUIRE(a->vmm, "NULL pointer (vmm)");
            TRY(finite_rows(a->vmm, (size_t)m * m, "vmm"));
            TRY(upload(dvmm, a->vmm, (size_t)m * m * sizeof(double), st));
            fs.vmm = dvmm.d();
        }
        if (want_iw) {
            HIPDRT_REQUIRE(a->vmm_iw, "NULL pointer (vmm_iw)");
            TRY(finite_rows(a->vmm_iw, (size_t)m * m, "vmm_iw"));
            TRY(upload(dvmm_iw, a->vmm_iw, (size_t)m * m * sizeof(double), st));
            fs.vmm_iw = dvmm_iw.d();
        }
        return HIPDRT_OK;
    }
    int begin(hipdrt_ctx* ctx) {
        TRY(enter(ctx, &st));
        fs = debug_fit_state(a->nf, a->m, a->n, 0, a->ldrm, a->n, a->rm_batched != 0, *a->opts, a->desc);
        const size_t B = (size_t)a->B, bm = B * a->m, bn = B * a->n;
        TRY(g.want("rv", a->rv, bm, fs.rv, st)); TRY(g.want("w", a->w, bm, fs.w, st)); TRY(g.want("est_w", a->est_w, bm, fs.est_w, st));
        TRY(g.want("x", a->x, bn, fs.x, st)); TRY(g.want("x_in", a->x_in, bn, fs.x_in, st)); TRY(g.want("s", a->s, 3 * bn, fs.s, st));
        TRY(g.want("rho", a->rho, 3 * B, fs.rho, st)); TRY(g.want("xmx", a->xmx, 3 * B, fs.xmx, st));
        TRY(g.want("dop_rho", a->dop_rho, 3 * B, fs.dop_rho, st)); TRY(g.want("dop_xmx", a->dop_xmx, 3 * B, fs.dop_xmx, st));
        TRY(g.want("coef_scale", a->coef_scale, B, fs.coef_scale, st)); TRY(g.want("var_floor", a->var_floor, B, fs.var_floor, st));
        TRY(g.want("active", a->active, B, fs.active, st)); TRY(g.want("outer_iters", a->outer_iters, B, fs.outer_iters, st));
        TRY(g.want("fit_status", a->fit_status, B, fs.fit_status, st));
        TRY(g.want("qp_iters_total", a->qp_iters_total, B, fs.qp_iters_total, st));
        TRY(g.want("outlier_t", a->outlier_t, bm, fs.outlier_t, st));
        if (a->qp_status) { TRY(upload(dqs, a->qp_status, B * sizeof(int), st)); fs.qp_status = dqs.i(); }
        return HIPDRT_OK;
    }
    int end() {
        LAUNCH_OK();
        return g.back(st);
    }
};

}  // namespace

extern "C" {

int hipdrt_debug_prep(hipdrt_ctx* ctx, const hipdrt_debug_setup_args* a) try {
    HIPDRT_REQUIRE(ctx && a, "NULL pointer");
    SetupRun r{a};
    TRY(r.sizes());
    const size_t B = (size_t)a->B;
    HIPDRT_REQUIRE(a->rv && a->w && a->s && a->x && a->x_in && a->rho && a->xmx && a->coef_scale && a->var_floor && a->active &&
                   a->outer_iters && a->fit_status && a->qp_iters_total,
                   "NULL pointer: prep writes rv, w, s, x, x_in, rho, xmx, coef_scale, var_floor, active, outer_iters, fit_status, qp_iters_total");
    if (a->desc) {
        HIPDRT_REQUIRE(a->dop_rho && a->dop_xmx, "NULL pointer: a prepared prep writes dop_rho and dop_xmx");
        TRY(finite_rows(a->rv, B * a->m, "rv"));
    } else {
        HIPDRT_REQUIRE(a->z_re && a->z_im, "NULL pointer (z_re, z_im)");
        HIPDRT_REQUIRE(a->nf >= 1 && a->m == 2 * a->nf, "a plain plan has m = 2 nf rows, nf >= 1");
        TRY(finite_rows(a->z_re, B * a->nf, "z_re")); TRY(finite_rows(a->z_im, B * a->nf, "z_im"));
    }
    TRY(r.begin(ctx));
    if (!a->desc) {
        TRY(upload(r.dzr, a->z_re, B * a->nf * sizeof(double), r.st)); TRY(upload(r.dzi, a->z_im, B * a->nf * sizeof(double), r.st));
        r.fs.z_re = r.dzr.d(); r.fs.z_im = r.dzi.d();
    }
    TRY(launch_prep(r.st, r.fs, a->B));
    return r.end();
} HIPDRT_CATCH

int hipdrt_debug_init_weights(hipdrt_ctx* ctx, const hipdrt_debug_setup_args* a) try {
    HIPDRT_REQUIRE(ctx && a, "NULL pointer");
    SetupRun r{a};
    TRY(r.sizes());
    const size_t B = (size_t)a->B;
    HIPDRT_REQUIRE(a->qp_status && a->x && a->rv && a->w && a->est_w && a->var_floor && a->active && a->fit_status,
                   "NULL pointer: init_weights needs qp_status, x, rv, w, est_w, var_floor, active, fit_status");
    HIPDRT_REQUIRE(a->stage >= 0 && a->stage <= 3, "stage 0, 1, 2 or 3");
    if (a->stage == 2 || a->row_mask) HIPDRT_REQUIRE(a->r0 >= 0 && a->r0 < a->r1 && a->r1 <= a->m, "0 <= r0 < r1 <= m");
    HIPDRT_REQUIRE(!(a->stage == 2 && a->opts->outlier_p > 0.0), "init_weights_separately with outlier_p is not built");
    TRY(finite_rows(a->x, B * a->n, "x")); TRY(finite_rows(a->rv, B * a->m, "rv"));
    if (a->stage == 3) TRY(finite_rows(a->est_w, B * a->m, "est_w"));
    if (a->stage < 2) TRY(finite_rows(a->var_floor, B, "var_floor"));
    TRY(r.begin(ctx));
    TRY(r.matrices(true, true, true));
    if (a->row_mask) launch_row_mask(r.st, a->B, a->m, a->r0, a->r1, r.fs.w);
    TRY(launch_init_weights(r.st, r.fs, a->B, a->stage, a->r0, a->r1));
    return r.end();
} HIPDRT_CATCH

int hipdrt_debug_weight_method(hipdrt_ctx* ctx, const hipdrt_debug_setup_args* a) try {
    HIPDRT_REQUIRE(ctx && a, "NULL pointer");
    SetupRun r{a};
    TRY(r.sizes());
    HIPDRT_REQUIRE(a->desc && a->est_w && a->wrow && a->wfac, "NULL pointer: the weight rule needs desc, est_w, wrow, wfac");
    HIPDRT_REQUIRE(a->desc->num_chrono > 0 && a->desc->num_chrono < a->m, "the weight rule needs 0 < num_chrono < m");
    HIPDRT_REQUIRE(std::isfinite(a->fixed_chrono) && std::isfinite(a->fixed_eis), "non-finite fixed factor");
    TRY(finite_rows(a->est_w, (size_t)a->B * a->m, "est_w"));
    TRY(r.begin(ctx));
    double *wrow = nullptr, *wfac = nullptr;
    TRY(r.g.want("wrow", a->wrow, (size_t)a->B * a->m, wrow, r.st)); TRY(r.g.want("wfac", a->wfac, (size_t)a->B * 2, wfac, r.st));
    launch_weight_method(r.st, r.fs, a->B, a->fixed_chrono, a->fixed_eis, wrow, wfac);
    return r.end();
} HIPDRT_CATCH

int hipdrt_debug_llh(hipdrt_ctx* ctx, const hipdrt_debug_setup_args* a) try {
    HIPDRT_REQUIRE(ctx && a, "NULL pointer");
    SetupRun r{a};
    TRY(r.sizes());
    const size_t B = (size_t)a->B;
    HIPDRT_REQUIRE(a->x && a->rv && a->est_w && a->var_floor && a->rss && a->slw, "NULL pointer: llh needs x, rv, est_w, var_floor, rss, slw");
    HIPDRT_REQUIRE(a->stored >= 0 && a->stored <= 3 && std::isfinite(a->scalar_w), "stored 0..3, a finite scalar_w");
    TRY(finite_rows(a->x, B * a->n, "x")); TRY(finite_rows(a->rv, B * a->m, "rv"));
    if (a->stored == 1 || a->stored == 2) TRY(finite_rows(a->est_w, B * a->m, "est_w"));
    if (a->stored == 0) TRY(finite_rows(a->var_floor, B, "var_floor"));
    TRY(r.begin(ctx));
    TRY(r.matrices(true, true, false));
    r.fs.vmm_iw = r.fs.vmm;
    double *rss = nullptr, *slw = nullptr, *w_out = nullptr;
    TRY(r.g.want("rss", a->rss, B, rss, r.st)); TRY(r.g.want("slw", a->slw, B, slw, r.st));
    TRY(r.g.want("w_out", a->w_out, B * a->m, w_out, r.st));
    TRY(launch_llh(r.st, r.fs, a->B, rss, slw, a->stored, a->scalar_w, w_out));
    return r.end();
} HIPDRT_CATCH

int hipdrt_debug_rowop(hipdrt_ctx* ctx, const hipdrt_debug_rowop_args* a) try {
    HIPDRT_REQUIRE(ctx && a, "NULL pointer");
    HIPDRT_REQUIRE(a->op >= 0 && a->op <= 6, "op 0..6");
    const int B = a->B, m = a->m, n = a->n, ns = a->ns, nf = a->nf, ld = a->ld;
    const size_t D = sizeof(double);
    HIPDRT_REQUIRE(a->out0, "NULL pointer (out0)");
    HIPDRT_REQUIRE(std::isfinite(a->factor) && std::isfinite(a->pen_r) && std::isfinite(a->pen_l), "non-finite scalar");
    // sizes first, so that nothing is uploaded for a call that is refused
    switch (a->op) {
    case 0:
        HIPDRT_REQUIRE(m >= 1 && m <= 8192 && a->in0, "vmm_exclude_self: 1 <= m <= 8192, in0 = vmm");
        TRY(finite_rows(a->in0, (size_t)m * m, "vmm"));
        break;
    case 1:
        HIPDRT_REQUIRE(nf >= 1 && 2 * nf <= 8192 && n >= 1 && n <= 4096 && ns >= 0 && ns < n && ld >= n, "assemble_rm: 1 <= 2 nf <= 8192, 0 <= ns < n <= 4096, ld >= n");
        HIPDRT_REQUIRE(a->in0 && a->in1 && a->in2, "assemble_rm: a_re, a_im, freq");
        HIPDRT_REQUIRE(a->idx_rinf >= -1 && a->idx_rinf < ns && a->idx_induc >= -1 && a->idx_induc < ns, "assemble_rm: special indices in [-1, ns)");
        TRY(finite_rows(a->in0, (size_t)nf * (n - ns), "a_re")); TRY(finite_rows(a->in1, (size_t)nf * (n - ns), "a_im"));
        TRY(finite_rows(a->in2, (size_t)nf, "freq"));
        break;
    case 2:
        HIPDRT_REQUIRE(n >= 1 && n <= 4096 && ld >= n && a->out1 && a->out2, "special_penalty: 1 <= n <= 4096, ld >= n, three matrices");
        HIPDRT_REQUIRE(a->idx_rinf >= -1 && a->idx_rinf < n && a->idx_induc >= -1 && a->idx_induc < n, "special_penalty: special indices in [-1, n)");
        break;
    case 3:
        HIPDRT_REQUIRE(n >= 1 && n <= 4096 && ns >= 0 && ns <= n, "make_h: 1 <= n <= 4096, 0 <= ns <= n");
        break;
    case 4: case 5:
        HIPDRT_REQUIRE(B >= 1 && B <= 4096 && m >= 1 && m <= 3 * 8192, "scale_rows: 1 <= B <= 4096, 1 <= m <= 24576");
        HIPDRT_REQUIRE(a->op == 4 || a->active, "scale_weights: active");
        TRY(finite_rows(a->in0, a->op == 4 ? (size_t)B * m : 0, "w"));
        TRY(finite_rows(a->op == 4 ? a->in1 : nullptr, (size_t)(a->batched ? B : 1) * m, "rows"));
        break;
    default:
        HIPDRT_REQUIRE(B >= 1 && B <= 4096 && m >= 1 && m <= 8192 && ld >= 1 && a->col >= 0 && a->col < ld && a->in0,
                       "copy_column: 1 <= B <= 4096, 1 <= m <= 8192, 0 <= col < ld, in0 = rm");
        TRY(finite_rows(a->in0, (size_t)(a->batched ? B : 1) * m * ld, "rm"));
    }
    hipStream_t st; TRY(enter(ctx, &st));
    GuardedOuts g;
    DevBuf d0, d1, d2, dact;
    double *o0 = nullptr, *o1 = nullptr, *o2 = nullptr;
    if (a->active && (a->op == 4 || a->op == 5)) TRY(upload(dact, a->active, (size_t)B * sizeof(int), st));
    switch (a->op) {
    case 0:
        TRY(upload(d0, a->in0, (size_t)m * m * D, st));
        TRY(g.want("out", a->out0, (size_t)m * m, o0, st));
        launch_vmm_exclude_self(st, d0.d(), m, o0);
        break;
    case 1: {
        hipdrt_fit_opts o; hipdrt_default_fit_opts(&o);
        o.inductance_scale = a->factor;
        FitState fs = debug_fit_state(nf, 2 * nf, n, ns, ld, n, false, o, nullptr);
        TRY(upload(d0, a->in0, (size_t)nf * (n - ns) * D, st)); TRY(upload(d1, a->in1, (size_t)nf * (n - ns) * D, st));
        TRY(upload(d2, a->in2, (size_t)nf * D, st));
        TRY(g.want("rm", a->out0, (size_t)2 * nf * ld, o0, st));
        launch_assemble_rm(st, fs, d0.d(), d1.d(), d2.d(), o0, a->idx_rinf, a->idx_induc);
        break;
    }
    case 2:
        TRY(g.want("m0", a->out0, (size_t)n * ld, o0, st)); TRY(g.want("m1", a->out1, (size_t)n * ld, o1, st));
        TRY(g.want("m2", a->out2, (size_t)n * ld, o2, st));
        launch_special_penalty(st, o0, o1, o2, ld, a->idx_rinf, a->idx_induc, a->pen_r, a->pen_l);
        break;
    case 3:
        TRY(g.want("h", a->out0, (size_t)n, o0, st));
        launch_make_h(st, o0, n, ns, a->nonneg);
        break;
    case 4:
        if (a->in0) TRY(upload(d0, a->in0, (size_t)B * m * D, st));
        if (a->in1) TRY(upload(d1, a->in1, (size_t)(a->batched ? B : 1) * m * D, st));
        TRY(g.want("out", a->out0, (size_t)B * m, o0, st));
        launch_scale_rows(st, B, m, a->in0 ? d0.d() : o0, a->in1 ? d1.d() : nullptr, a->batched ? 1 : 0, a->factor,
                          a->active ? dact.i() : nullptr, o0);
        break;
    case 5: {
        hipdrt_fit_opts o; hipdrt_default_fit_opts(&o);
        FitState fs = debug_fit_state(0, m, 1, 0, 1, 1, false, o, nullptr);
        TRY(g.want("w", a->out0, (size_t)B * m, o0, st));
        fs.w = o0; fs.active = dact.i();
        launch_scale_weights(st, fs, B, a->factor);
        break;
    }
    default:
        TRY(upload(d0, a->in0, (size_t)(a->batched ? B : 1) * m * ld * D, st));
        TRY(g.want("out", a->out0, (size_t)B * m, o0, st));
        launch_copy_column(st, B, m, d0.d(), a->batched ? (long long)m * ld : 0, ld, a->col, o0);
    }
    LAUNCH_OK();
    return g.back(st);
} HIPDRT_CATCH

}  // extern "C"
