// Test and diagnostic hooks of include/hipdrt_debug.h: context switches, and single launchers run on host arrays exactly as
// the fit loop runs them.  (hipdrt_debug_stream_pool sits with the pool in api.hip; hipdrt_debug_map_gaussian, _map_reduce and
// _map_prob sit in map_filter.hip and map_predict.hip, next to kernels no other file can name; the hooks of the launchers that run
// before the fit loop and after it sit in debug_setup.hip.  debug_guard.hpp holds the bordered device arrays all of them use.)
#include <cmath>
#include <cstring>

#include "debug_guard.hpp"
#include "plan.hpp"

// what the row hooks ask of every input row they upload (a null row: not read)
static int require_finite(const double* row, size_t count) {
    if (row) for (size_t i = 0; i < count; ++i) HIPDRT_REQUIRE(std::isfinite(row[i]), "non-finite input row");
    return HIPDRT_OK;
}

extern "C" {

int hipdrt_debug_qp_group(hipdrt_ctx* ctx, int members) try {
    HIPDRT_REQUIRE(ctx, "NULL pointer");
    ctx->qp_force_group = members;
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_debug_qp_waves(hipdrt_ctx* ctx, int waves) try {
    HIPDRT_REQUIRE(ctx, "NULL pointer");
    HIPDRT_REQUIRE(waves == -1 || waves == 4 || waves == 8, "waves: 4, 8 or -1");
    ctx->qp_waves = waves;
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_debug_exact_zero_shortcuts(hipdrt_ctx* ctx, int on) try {
    HIPDRT_REQUIRE(ctx, "NULL pointer");
    ctx->zero_shortcuts = on ? 1 : 0;
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_debug_qp_occupancy(hipdrt_ctx* ctx, int threads, int n) try {
    if (!ctx || hipSetDevice(ctx->device) != hipSuccess) return -1;
    return qp_occupancy(threads, n);
} HIPDRT_CATCH

int hipdrt_qp_profile(hipdrt_ctx* ctx, unsigned long long* cycles, int n, int reset) try {
    HIPDRT_REQUIRE(ctx && cycles, "NULL pointer");
    TRY(enter(ctx));
    HIPDRT_CHECK(hipStreamSynchronize(ctx->stream));
    return qp_profile_read(cycles, n, reset) < 0 ? HIPDRT_E_HIP : HIPDRT_OK;
} HIPDRT_CATCH

// test hook (include/hipdrt_debug.h): launch_gram_l2 / launch_qvec exactly as the fit loop calls them, on host arrays.  Every
// extent a kernel derives an address from is checked here: the kernels themselves trust their caller.
int hipdrt_debug_gram_l2(hipdrt_ctx* ctx, const hipdrt_debug_gram_args* a) try {
    HIPDRT_REQUIRE(ctx && a && a->A && a->w, "NULL pointer");
    const int B = a->B, m = a->m, n = a->n;
    HIPDRT_REQUIRE(B >= 1 && B <= 4096 && m >= 1 && m <= 8192 && n >= 1 && n <= 4096, "1 <= B <= 4096, 1 <= m <= 8192, 1 <= n <= 4096");
    HIPDRT_REQUIRE(a->lda >= n, "lda >= n");
    HIPDRT_REQUIRE(a->P || a->Ppk, "at least one of P / Ppk");
    HIPDRT_REQUIRE(!a->P || a->ldp >= n, "ldp >= n");
    HIPDRT_REQUIRE(!a->y || a->q, "y without q");
    const bool hyper = a->s != nullptr;
    if (hyper) {
        HIPDRT_REQUIRE(a->mk[0] && a->mk[1] && a->mk[2], "hyper-parameter form: three penalty matrices");
        HIPDRT_REQUIRE(a->ldm >= n, "ldm >= n");
        HIPDRT_REQUIRE(a->ns >= 0 && a->ns <= n, "0 <= ns <= n");
        HIPDRT_REQUIRE(a->dop_size >= 0 && (a->dop_size == 0 || (a->dop_start >= 0 && a->dop_start + a->dop_size <= a->ns)),
                       "x_dop block outside the special block [0, ns)");
        HIPDRT_REQUIRE(a->dop_size == 0 || !a->rho || a->dop_rho, "dop_rho missing");
        HIPDRT_REQUIRE(a->toep_maxd >= -1 && a->toep_maxd < n, "-1 <= toep_maxd < n");
        HIPDRT_REQUIRE(!a->toep || n - a->ns >= 1, "Toeplitz form needs a DRT block (n - ns >= 1)");
    } else if (a->l2) {
        HIPDRT_REQUIRE(a->ldl2 >= n, "ldl2 >= n");
    }
    hipStream_t st; TRY(enter(ctx, &st));
    const size_t D = sizeof(double);
    const size_t ppk = qp_ppk_doubles(n);
    DevBuf dA, dw, dy, dl1, dl2, dmk[3], ds, drho, ddrho, dact, dP, dPpk, dq;
    TRY(upload(dA, a->A, (size_t)(a->a_batched ? B : 1) * m * a->lda * D, st));
    TRY(upload(dw, a->w, (size_t)B * m * D, st));
    if (a->y) TRY(upload(dy, a->y, (size_t)B * m * D, st));
    if (a->l1) TRY(upload(dl1, a->l1, (size_t)n * D, st));
    if (a->active) TRY(upload(dact, a->active, (size_t)B * sizeof(int), st));
    GramL2 g{};
    if (hyper) {
        for (int k = 0; k < 3; ++k) {
            TRY(upload(dmk[k], a->mk[k], (size_t)n * a->ldm * D, st));
            g.mk[k] = dmk[k].d(); g.dfac[k] = a->dfac[k]; g.dop_dfac[k] = a->dop_dfac[k];
        }
        TRY(upload(ds, a->s, (size_t)B * 3 * n * D, st));
        if (a->rho) TRY(upload(drho, a->rho, (size_t)B * 3 * D, st));
        if (a->rho && a->dop_size > 0) TRY(upload(ddrho, a->dop_rho, (size_t)B * 3 * D, st));
        g.ldm = a->ldm; g.s = ds.d(); g.rho = a->rho ? drho.d() : nullptr; g.use_rho = a->rho ? 1 : 0;
        g.ns = a->ns; g.sym = a->sym ? 1 : 0; g.toep = a->toep ? 1 : 0; g.toep_maxd = a->toep_maxd; g.spec_zero = a->spec_zero ? 1 : 0;
        g.dop_start = a->dop_start; g.dop_size = a->dop_size; g.dop_rho = ddrho.d();
    } else if (a->l2) {
        TRY(upload(dl2, a->l2, (size_t)(a->l2_batched ? B : 1) * n * a->ldl2 * D, st));
        g.l2 = dl2.d(); g.l2_stride = a->l2_batched ? (long long)n * a->ldl2 : 0; g.ldl2 = a->ldl2;
    }
    if (a->P) TRY(upload(dP, a->P, (size_t)B * n * a->ldp * D, st));
    if (a->Ppk) TRY(upload(dPpk, a->Ppk, (size_t)B * ppk * D, st));
    if (a->y) TRY(upload(dq, a->q, (size_t)B * n * D, st));
    PqArgs pq{};
    pq.B = B; pq.m = m; pq.n = n; pq.A = dA.d(); pq.lda = a->lda; pq.a_stride = a->a_batched ? (long long)m * a->lda : 0;
    pq.w = dw.d(); pq.active = a->active ? dact.i() : nullptr;
    pq.P = a->P ? dP.d() : nullptr; pq.ldp = a->ldp; pq.p_stride = (long long)n * a->ldp;
    pq.Ppk = a->Ppk ? dPpk.d() : nullptr; pq.ppk_stride = (long long)ppk;
    pq.y = dy.d(); pq.l1 = a->l1 ? dl1.d() : nullptr; pq.l1_scalar = a->l1_scalar; pq.q = dq.d();
    launch_gram_l2(st, pq, g);
    LAUNCH_OK();
    if (a->y) {
        launch_qvec(st, pq);
        LAUNCH_OK();
    }
    if (a->P) HIPDRT_CHECK(hipMemcpyAsync(a->P, dP.p, (size_t)B * n * a->ldp * D, hipMemcpyDeviceToHost, st));
    if (a->Ppk) HIPDRT_CHECK(hipMemcpyAsync(a->Ppk, dPpk.p, (size_t)B * ppk * D, hipMemcpyDeviceToHost, st));
    if (a->y) HIPDRT_CHECK(hipMemcpyAsync(a->q, dq.p, (size_t)B * n * D, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_debug_pack_p(hipdrt_ctx* ctx, int B, int n, const double* P, int ldp, double* Ppk) try {
    HIPDRT_REQUIRE(ctx && P && Ppk, "NULL pointer");
    HIPDRT_REQUIRE(B >= 1 && B <= 4096 && n >= 1 && n <= 4096 && ldp >= n, "1 <= B <= 4096, 1 <= n <= 4096, ldp >= n");
    hipStream_t st; TRY(enter(ctx, &st));
    const size_t ppk = qp_ppk_doubles(n);
    DevBuf dP, dPpk;
    TRY(upload(dP, P, (size_t)B * n * ldp * sizeof(double), st));
    TRY(upload(dPpk, Ppk, (size_t)B * ppk * sizeof(double), st));
    launch_pack_p(st, B, n, dP.d(), ldp, dPpk.d());
    LAUNCH_OK();
    HIPDRT_CHECK(hipMemcpyAsync(Ppk, dPpk.p, (size_t)B * ppk * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_debug_logdet(hipdrt_ctx* ctx, int B, int n, const double* P, double* logdet, int* status) try {
    HIPDRT_REQUIRE(ctx && P && logdet && status, "NULL pointer");
    HIPDRT_REQUIRE(B >= 1 && B <= 4096 && n >= 1 && n <= 4096, "1 <= B <= 4096, 1 <= n <= 4096");
    hipStream_t st; TRY(enter(ctx, &st));
    const size_t ppk = qp_ppk_doubles(n);
    DevBuf dP, dPpk, scratch, dld, dst;
    TRY(upload(dP, P, (size_t)B * n * n * sizeof(double), st));
    // (tiles above the diagonal and tile rows of pure padding are neither written by the packing nor read by the factorisation)
    HIPDRT_CHECK(dPpk.alloc((size_t)B * ppk * sizeof(double)));
    HIPDRT_CHECK(hipMemsetAsync(dPpk.p, 0, (size_t)B * ppk * sizeof(double), st));
    HIPDRT_CHECK(dld.alloc((size_t)B * sizeof(double))); HIPDRT_CHECK(dst.alloc((size_t)B * sizeof(int)));
    launch_pack_p(st, B, n, dP.d(), n, dPpk.d());
    LAUNCH_OK();
    TRY(logdet_dev(st, B, n, dPpk.d(), (long long)ppk, scratch, dld.d(), dst.i()));
    LAUNCH_OK();
    HIPDRT_CHECK(hipMemcpyAsync(logdet, dld.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(status, dst.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

// test hook (include/hipdrt_debug.h): launch_hyper as the fit loop calls it, on host arrays.  Every extent a kernel derives an
// address from is checked here.  In/out arrays live on the device between two borders of marker bytes (Guarded).
int hipdrt_debug_hyper_form(hipdrt_ctx* ctx, int n, int m, int ns, int toeplitz, int outlier, int* form, long long* lds_bytes) try {
    HIPDRT_REQUIRE(ctx && form && lds_bytes, "NULL pointer");
    HIPDRT_REQUIRE(m >= 1 && m <= 8192 && n >= 1 && n <= 4096 && ns >= 0 && ns < n, "1 <= m <= 8192, 0 <= ns < n <= 4096");
    size_t lds = 0;
    const bool ok = hyper_lds_form(n, m, ns, toeplitz ? 1 : 0, outlier != 0, form, &lds);
    *lds_bytes = (long long)lds;
    if (!ok) { set_error("hyper-parameter kernel: problem too large for LDS (m, n)"); return HIPDRT_E_INVALID; }
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_debug_impedance_interp_form(hipdrt_ctx* ctx, int B, int nf, int ntau, int ngrid, int* tpr, int* rpb,
                                       long long* lds_bytes) try {
    HIPDRT_REQUIRE(ctx && tpr && rpb && lds_bytes, "NULL pointer");
    HIPDRT_REQUIRE(B >= 1 && B <= kGridDimMax && nf >= 1 && ntau >= 1, "1 <= B <= 65535, nf, ntau >= 1");
    HIPDRT_REQUIRE(impedance_ngrid_ok(ngrid), "interp needs lookups with ngrid >= 2 that one workgroup's LDS holds (2 <= ngrid <= 3406)");
    size_t lds = 0;
    impedance_interp_form(B, nf, ntau, ngrid, tpr, rpb, &lds);
    *lds_bytes = (long long)lds;
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_debug_hyper_step(hipdrt_ctx* ctx, const hipdrt_debug_hyper_args* a) try {
    HIPDRT_REQUIRE(ctx && a, "NULL pointer");
    const int B = a->B, m = a->m, n = a->n, ns = a->ns, nd = n - ns;
    HIPDRT_REQUIRE(B >= 1 && B <= 4096 && m >= 1 && m <= 8192 && n >= 1 && n <= 4096, "1 <= B <= 4096, 1 <= m <= 8192, 1 <= n <= 4096");
    HIPDRT_REQUIRE(ns >= 0 && nd >= 1, "0 <= ns < n: the step needs a DRT block");
    HIPDRT_REQUIRE(a->ldrm >= n && a->ldm >= n, "ldrm >= n, ldm >= n");
    HIPDRT_REQUIRE(a->rm && a->vmm && a->mk[0] && a->mk[1] && a->mk[2] && a->opts, "rm, vmm, three penalty matrices, opts");
    HIPDRT_REQUIRE(a->x && a->x_in && a->s && a->rho && a->xmx && a->rv && a->est_w && a->w && a->var_floor && a->coef_scale,
                   "per-spectrum state: x, x_in, s, rho, xmx, rv, est_w, w, var_floor, coef_scale");
    HIPDRT_REQUIRE(a->qp_status && a->active && a->fit_status && a->outer_iters && a->n_active, "qp_status, active, fit_status, outer_iters, n_active");
    HIPDRT_REQUIRE(a->continue_mode >= 0 && a->continue_mode <= 2 && a->it >= 0, "continue_mode 0, 1 or 2; it >= 0");
    HIPDRT_REQUIRE(a->products >= 0 && a->products <= 2, "products 0, 1 or 2");
    HIPDRT_REQUIRE(a->toep_reach >= -1, "toep_reach >= -1");
    const bool outl = a->opts->outlier_p > 0.0;
    const bool prep = a->desc != nullptr;
    hipdrt_prepared_desc desc{};
    desc.vz_index = -1;
    if (prep) {
        desc = *a->desc;
        HIPDRT_REQUIRE(a->dop_rho && a->dop_xmx, "a prepared step needs dop_rho and dop_xmx");
        HIPDRT_REQUIRE(desc.dop_size >= 0 && (desc.dop_size == 0 || (desc.dop_start >= 0 && desc.dop_start + desc.dop_size <= ns)),
                       "x_dop block outside the special block [0, ns)");
        HIPDRT_REQUIRE(desc.dop_size <= nd, "x_dop block larger than the DRT block (the kernel's LDS vectors hold n - ns entries)");
        HIPDRT_REQUIRE(desc.vz_index >= -1 && desc.vz_index < n, "-1 <= vz_index < n");
        HIPDRT_REQUIRE(desc.vb_start >= 0 && desc.vb_size >= 0 && desc.vb_start + desc.vb_size <= n, "v_baseline columns outside [0, n)");
        HIPDRT_REQUIRE(desc.num_chrono >= 0 && desc.num_chrono <= m, "0 <= num_chrono <= m");
        if (desc.vz_index >= 0) {
            HIPDRT_REQUIRE(a->vz_strength && a->rm_col, "vz_offset column: vz_strength and rm_col");
            HIPDRT_REQUIRE(a->rm_batched || B == 1, "vz_offset column: one response matrix per spectrum");
        }
        desc.m = m; desc.n = n; desc.ns = ns; desc.toeplitz_m = a->toeplitz ? 1 : 0;
    }
    const bool vz = prep && desc.vz_index >= 0;
    HIPDRT_REQUIRE(!a->vz_entry || vz, "vz_entry without a vz_offset column");
    if (a->products == 1) HIPDRT_REQUIRE(!outl, "products = 1: outlier_p <= 0");
    if (a->products == 2) HIPDRT_REQUIRE(!a->rm_batched && !outl && !vz, "products = 2: a shared rm, no vz_offset column, outlier_p <= 0");
    // the Toeplitz claim and the reach, on the host
    if (a->toeplitz) {
        int reach = 0;
        for (int k = 0; k < 3; ++k) {
            const double* blk = a->mk[k] + (size_t)ns * a->ldm + ns;
            for (int i = 0; i < nd; ++i)
                for (int j = 0; j < nd; ++j) {
                    const int d = i > j ? i - j : j - i;
                    const double v = blk[(size_t)i * a->ldm + j];
                    HIPDRT_REQUIRE(v == blk[d] || (v != v && blk[d] != blk[d]), "toeplitz = 1, but a DRT block is not symmetric Toeplitz");
                }
            for (int d = nd - 1; d > reach; --d)
                if (blk[d] != 0.0) { reach = d; break; }
        }
        HIPDRT_REQUIRE(a->toep_reach < 0 || a->toep_reach >= reach, "toep_reach is smaller than the reach of the penalty blocks");
    }
    int form = 0;
    size_t lds = 0;
    if (!hyper_lds_form(n, m, ns, a->toeplitz ? 1 : 0, outl, &form, &lds)) {
        set_error("hyper-parameter kernel: problem too large for LDS (m, n)");
        return HIPDRT_E_INVALID;
    }
    hipStream_t st; TRY(enter(ctx, &st));
    const size_t D = sizeof(double), I = sizeof(int);
    const size_t nrm = (size_t)(a->rm_batched ? B : 1) * m * a->ldrm;
    DevBuf dvmm, dmk[3], dx, dqs, dvs, dve, dpremv;
    std::vector<double> rm_copy(a->rm, a->rm + nrm);
    const size_t bn = (size_t)B * n, bm = (size_t)B * m, b3 = (size_t)B * 3;
    FitState fs = debug_fit_state(0, m, n, ns, a->ldrm, a->ldm, a->rm_batched != 0, *a->opts, prep ? &desc : nullptr);
    GuardedOuts g;
    TRY(g.want("rm", rm_copy.data(), nrm, fs.rm_rw, st));
    TRY(upload(dvmm, a->vmm, (size_t)m * m * D, st));
    for (int k = 0; k < 3; ++k) TRY(upload(dmk[k], a->mk[k], (size_t)n * a->ldm * D, st));
    TRY(upload(dx, a->x, bn * D, st));
    TRY(upload(dqs, a->qp_status, (size_t)B * I, st));
    if (vz) TRY(upload(dvs, a->vz_strength, (size_t)m * D, st));
    if (a->vz_entry) TRY(upload(dve, a->vz_entry, bm * D, st));
    TRY(g.want("x_in", a->x_in, bn, fs.x_in, st)); TRY(g.want("s", a->s, 3 * bn, fs.s, st));
    TRY(g.want("rho", a->rho, b3, fs.rho, st)); TRY(g.want("xmx", a->xmx, b3, fs.xmx, st));
    TRY(g.want("rv", a->rv, bm, fs.rv, st)); TRY(g.want("est_w", a->est_w, bm, fs.est_w, st)); TRY(g.want("w", a->w, bm, fs.w, st));
    TRY(g.want("var_floor", a->var_floor, B, fs.var_floor, st)); TRY(g.want("coef_scale", a->coef_scale, B, fs.coef_scale, st));
    TRY(g.want("active", a->active, B, fs.active, st)); TRY(g.want("fit_status", a->fit_status, B, fs.fit_status, st));
    TRY(g.want("outer_iters", a->outer_iters, B, fs.outer_iters, st)); TRY(g.want("n_active", a->n_active, 1, fs.n_active, st));
    TRY(g.want("outlier_t", a->outlier_t, bm, fs.outlier_t, st));
    TRY(g.want("dop_rho", prep ? a->dop_rho : nullptr, b3, fs.dop_rho, st)); TRY(g.want("dop_xmx", prep ? a->dop_xmx : nullptr, b3, fs.dop_xmx, st));
    fs.toeplitz_m = a->toeplitz ? 1 : 0; fs.toep_reach = a->toeplitz ? a->toep_reach : -1;
    fs.continue_mode = a->continue_mode; fs.min_iter = a->min_iter; fs.basis_area = a->basis_area;
    fs.desc = desc;          // (not a prepared step: vz_index -1, the rest zero, as before)
    fs.rm = fs.rm_rw;
    fs.vz_strength = vz ? dvs.d() : nullptr; fs.vz_entry = a->vz_entry ? dve.d() : nullptr;
    fs.vmm = dvmm.d(); fs.vmm_iw = dvmm.d();
    for (int k = 0; k < 3; ++k) fs.mk[k] = dmk[k].d();
    fs.x = dx.d(); fs.qp_status = dqs.i();
    if (a->products) {
        HIPDRT_CHECK(dpremv.alloc(3 * (size_t)B * m * D));
        HIPDRT_CHECK(hipMemsetAsync(dpremv.p, 0xFF, 3 * (size_t)B * m * D, st));       // NaN where no product kernel wrote
        fs.premv = dpremv.d();
        fs.premv_batched = a->products == 2 ? 1 : 0;
    }
    TRY(launch_hyper(st, fs, B, a->it));
    LAUNCH_OK();
    TRY(g.back(st));
    // the response matrix: nothing but the vz_offset column may differ from what was uploaded
    const int nmat = a->rm_batched ? B : 1;
    for (int b = 0; b < nmat; ++b)
        for (int i = 0; i < m; ++i) {
            const size_t row = ((size_t)b * m + i) * a->ldrm;
            for (int j = 0; j < a->ldrm; ++j) {
                if (vz && j == desc.vz_index) { a->rm_col[(size_t)b * m + i] = rm_copy[row + j]; continue; }
                if (std::memcmp(&rm_copy[row + j], &a->rm[row + j], D) != 0) {
                    set_error("hyper step changed rm outside the vz_offset column (row " + std::to_string(i) + ", column " + std::to_string(j) + ")");
                    return HIPDRT_E_NUMERIC;
                }
            }
        }
    return HIPDRT_OK;
} HIPDRT_CATCH

// test hook (include/hipdrt_debug.h): stage B of kk_kernel as it is, on host residuals
int hipdrt_debug_kk_stats(hipdrt_ctx* ctx, int B, int nf, const double* freq, const double* err_re, const double* err_im,
                          const hipdrt_kk_opts* opts, double* std_out, int* outlier_mask, double* f_lim, int* i_lim,
                          int* status) try {
    HIPDRT_REQUIRE(ctx && freq && err_re && err_im, "NULL pointer");
    HIPDRT_REQUIRE(B >= 1 && B <= 65535 && nf >= 1 && nf <= 4096, "1 <= B <= 65535, 1 <= nf <= 4096");
    const int order = freq_monotone(freq, nf);
    HIPDRT_REQUIRE(order != 0, "the frequency grid must be strictly ascending or descending");
    hipdrt_kk_opts o = opts_or(opts, hipdrt_default_kk_opts);
    TRY(kk_check_opts(o));
    HIPDRT_REQUIRE(kk_lds_bytes(nf, 0, 0) <= kLdsLimit, "KK statistics: nf too large for one workgroup's LDS");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf dfreq, dre, dim;
    TRY(upload(dfreq, freq, (size_t)nf * sizeof(double), st));
    TRY(upload(dre, err_re, (size_t)B * nf * sizeof(double), st));
    TRY(upload(dim, err_im, (size_t)B * nf * sizeof(double), st));
    KkArgs a{};
    a.nf = nf; a.desc = order > 0 ? 1 : 0; a.freq = dfreq.d(); a.o = o; a.in_re = dre.d(); a.in_im = dim.d();
    DevOuts outs;
    TRY(outs.want(std_out, (size_t)B, a.std)); TRY(outs.want(outlier_mask, (size_t)B * nf, a.mask));
    TRY(outs.want(f_lim, (size_t)B * 2, a.f_lim)); TRY(outs.want(i_lim, (size_t)B * 2, a.i_lim)); TRY(outs.want(status, (size_t)B, a.status));
    TRY(launch_kk(st, nullptr, a, B));
    LAUNCH_OK();
    TRY(outs.back(st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

// test hook (include/hipdrt_debug.h): apply_rows_kernel as it is, on host arrays.  The device output carries one extra row and
// five extra columns filled with a marker; a marker that changed means the kernel wrote outside its B x r block.
int hipdrt_debug_apply_rows(hipdrt_ctx* ctx, int B, int K, int ldx, int col_offset, const double* X, int r, const double* E,
                            const double* scale, double* out) try {
    HIPDRT_REQUIRE(ctx && X && E && out, "NULL pointer");
    HIPDRT_REQUIRE(B >= 1 && K >= 1 && r >= 1 && col_offset >= 0, "B, K, r >= 1, col_offset >= 0");
    HIPDRT_REQUIRE(ldx >= col_offset + K, "ldx >= col_offset + K");
    hipStream_t st; TRY(enter(ctx, &st));
    const int ldo = r + 5, rows = B + 1;
    const double marker = -7.0e77;
    DevBuf dx, de, ds, dout;
    TRY(upload(dx, X, (size_t)B * ldx * sizeof(double), st));
    TRY(upload(de, E, (size_t)r * K * sizeof(double), st));
    if (scale) TRY(upload(ds, scale, (size_t)B * sizeof(double), st));
    std::vector<double> ho((size_t)rows * ldo, marker);
    TRY(upload(dout, ho.data(), ho.size() * sizeof(double), st));
    launch_apply_rows(st, B, K, dx.d(), ldx, col_offset, r, de.d(), K, scale ? ds.d() : nullptr, nullptr, dout.d(), ldo);
    LAUNCH_OK();
    HIPDRT_CHECK(hipMemcpyAsync(ho.data(), dout.p, ho.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    for (int b = 0; b < rows; ++b)
        for (int i = 0; i < ldo; ++i) {
            const double v = ho[(size_t)b * ldo + i];
            if (b < B && i < r) out[(size_t)b * r + i] = v;
            else if (!(v == marker)) {
                set_error("apply_rows wrote outside its B x r block (row " + std::to_string(b) + ", column " + std::to_string(i) + ")");
                return HIPDRT_E_NUMERIC;
            }
        }
    return HIPDRT_OK;
} HIPDRT_CATCH

// test hook (include/hipdrt_debug.h): peaks_kernel as it is, on host rows.  Every output sits between two borders of marker bytes.
int hipdrt_debug_find_peaks(hipdrt_ctx* ctx, int B, int neval, const double* fxx, const double* f, const double* var_fxx,
                            const double* var_f, const hipdrt_peak_opts* opts, int* peak_sign, int* keep, double* heights,
                            double* prominences, double* probs, int* left_bases, int* right_bases, int* count,
                            double* used_prominence, double* peak_prob, double* curv_prob) try {
    HIPDRT_REQUIRE(ctx && fxx, "NULL pointer");
    HIPDRT_REQUIRE(B >= 1 && B <= 65535 && neval >= 1 && neval <= (1 << 20), "1 <= B <= 65535, 1 <= neval <= 2^20");
    hipdrt_peak_opts o = opts_or(opts, hipdrt_peak_opts_default);
    TRY(peak_check_opts(o, neval));
    const bool need_f = o.search == 0 || o.method == 2;
    HIPDRT_REQUIRE(!need_f || f, "a two-pass search and the map probabilities need the f rows");
    HIPDRT_REQUIRE(o.method == 0 || var_fxx, "methods 1 and 2 need var_fxx");
    HIPDRT_REQUIRE(o.method != 2 || var_f, "method 2 needs var_f");
    HIPDRT_REQUIRE(peaks_lds_bytes(neval, o.method, need_f, o.num_peaks) <= kLdsLimit,
                   "find_peaks: neval too large for one workgroup's LDS");
    const size_t bn = (size_t)B * neval;
    const double* rows[4] = {fxx, need_f ? f : nullptr, o.method >= 1 ? var_fxx : nullptr, o.method == 2 ? var_f : nullptr};
    for (const double* r : rows) TRY(require_finite(r, bn));
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf din[4];
    for (int k = 0; k < 4; ++k) if (rows[k]) TRY(upload(din[k], rows[k], bn * sizeof(double), st));
    PeakArgs a{};
    a.neval = neval; a.o = o; a.fxx = din[0].d(); a.f = din[1].d(); a.var_fxx = din[2].d(); a.var_f = din[3].d(); a.ldv = neval;
    GuardedOuts outs;
    TRY(outs.want("peak_sign", peak_sign, bn, a.peak_sign, st)); TRY(outs.want("keep", keep, bn, a.keep, st));
    TRY(outs.want("heights", heights, bn, a.heights, st)); TRY(outs.want("prominences", prominences, bn, a.prominences, st));
    TRY(outs.want("probs", probs, bn, a.probs, st));
    TRY(outs.want("left_bases", left_bases, bn, a.left_bases, st)); TRY(outs.want("right_bases", right_bases, bn, a.right_bases, st));
    TRY(outs.want("count", count, (size_t)B, a.count, st)); TRY(outs.want("used_prominence", used_prominence, (size_t)B, a.used_prominence, st));
    TRY(outs.want("peak_prob", o.method == 2 ? peak_prob : nullptr, bn, a.peak_prob, st));
    TRY(outs.want("curv_prob", o.method == 2 ? curv_prob : nullptr, bn, a.curv_prob, st));
    TRY(launch_peaks(st, a, B));
    LAUNCH_OK();
    return outs.back(st);
} HIPDRT_CATCH

// test hook (include/hipdrt_debug.h): peak_trough_prob_kernel as it is, on host rows.  Every output sits between two borders of marker bytes.
int hipdrt_debug_peak_trough_probs(hipdrt_ctx* ctx, int B, int neval, const double* f, const double* fx, const double* fxx,
                                   const double* var_f, const double* var_fx, const double* var_fxx, const double* prob_in,
                                   const hipdrt_peak_prob_opts* opts, int nranges, const int* range_lo, const int* range_hi,
                                   double* pp, double* tp, double* prob, double* sigma, int* keep, double* heights,
                                   double* prominences, int* left_bases, int* right_bases, int* count, int* range_peaks) try {
    HIPDRT_REQUIRE(ctx, "NULL pointer");
    HIPDRT_REQUIRE(B >= 1 && B <= 65535 && neval >= 1 && neval <= (1 << 20), "1 <= B <= 65535, 1 <= neval <= 2^20");
    hipdrt_peak_prob_opts o = opts_or(opts, hipdrt_peak_prob_opts_default);
    TRY(peak_prob_check(o, neval, nranges, range_lo, range_hi));
    const bool bayes = o.bayes_cov != 0;
    HIPDRT_REQUIRE(prob_in || (f && fx && fxx), "the three mean rows, or prob_in");
    HIPDRT_REQUIRE(prob_in || !bayes || (var_f && var_fx && var_fxx), "bayes_cov needs the three variance rows");
    HIPDRT_REQUIRE(!prob_in || !(pp || tp || sigma), "a given prob row has no pp, tp or sigma");
    const size_t bn = (size_t)B * neval;
    const double* rows[7] = {prob_in, prob_in ? nullptr : f, prob_in ? nullptr : fx, prob_in ? nullptr : fxx,
                             prob_in || !bayes ? nullptr : var_f, prob_in || !bayes ? nullptr : var_fx,
                             prob_in || !bayes ? nullptr : var_fxx};
    for (const double* r : rows) TRY(require_finite(r, bn));
    if (o.search != 2) nranges = 0;
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf din[7], dlo, dhi;
    for (int k = 0; k < 7; ++k) if (rows[k]) TRY(upload(din[k], rows[k], bn * sizeof(double), st));
    if (nranges > 0) {
        TRY(upload(dlo, range_lo, (size_t)nranges * sizeof(int), st)); TRY(upload(dhi, range_hi, (size_t)nranges * sizeof(int), st));
    }
    PeakProbArgs a{};
    a.neval = neval; a.nranges = nranges; a.o = o; a.prob_in = din[0].d(); a.f = din[1].d(); a.fx = din[2].d(); a.fxx = din[3].d();
    a.var_f = din[4].d(); a.var_fx = din[5].d(); a.var_fxx = din[6].d(); a.ldv = neval; a.range_lo = dlo.i(); a.range_hi = dhi.i();
    GuardedOuts outs;
    TRY(outs.want("pp", pp, bn, a.pp, st)); TRY(outs.want("tp", tp, bn, a.tp, st)); TRY(outs.want("prob", prob, bn, a.prob, st));
    TRY(outs.want("sigma", sigma, 3 * bn, a.sigma, st)); TRY(outs.want("keep", keep, bn, a.keep, st));
    TRY(outs.want("heights", heights, bn, a.heights, st)); TRY(outs.want("prominences", prominences, bn, a.prominences, st));
    TRY(outs.want("left_bases", left_bases, bn, a.left_bases, st)); TRY(outs.want("right_bases", right_bases, bn, a.right_bases, st));
    TRY(outs.want("count", count, (size_t)B, a.count, st));
    TRY(outs.want("range_peaks", nranges > 0 ? range_peaks : nullptr, (size_t)B * nranges, a.range_peaks, st));
    TRY(launch_peak_prob(st, a, B));
    LAUNCH_OK();
    return outs.back(st);
} HIPDRT_CATCH

// test hooks (include/hipdrt_debug.h): the two kernels of pfrt.hip as they are, on host arrays; outputs between borders of marker bytes
int hipdrt_debug_pfrt_step(hipdrt_ctx* ctx, int B, int neval, const int* peak_sign, const double* heights, const double* prominences,
                           const double* f, const double* var_f, const double* var_fxx, double var_floor, int ext_left,
                           int ext_right, double* out) try {
    HIPDRT_REQUIRE(ctx && peak_sign && heights && prominences && f && var_f && var_fxx && out, "NULL pointer");
    HIPDRT_REQUIRE(B >= 1 && B <= 65535 && neval >= 1 && neval <= (1 << 20), "1 <= B <= 65535, 1 <= neval <= 2^20");
    const size_t bn = (size_t)B * neval;
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf dsg, din[5];
    const double* rows[5] = {heights, prominences, f, var_f, var_fxx};
    TRY(upload(dsg, peak_sign, bn * sizeof(int), st));
    for (int k = 0; k < 5; ++k) TRY(upload(din[k], rows[k], bn * sizeof(double), st));
    Guarded g;
    TRY(g.up("out", out, bn * sizeof(double), st));
    PfrtStepArgs a{};
    a.neval = neval; a.floor = var_floor; a.ext_left = ext_left; a.ext_right = ext_right; a.peak_sign = dsg.i();
    a.heights = din[0].d(); a.prominences = din[1].d(); a.f = din[2].d(); a.var_f = din[3].d(); a.var_fxx = din[4].d();
    a.ldv = neval; a.out = g.dd();
    TRY(launch_pfrt_step(st, a, B));
    LAUNCH_OK();
    TRY(g.fetch(st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return g.check();
} HIPDRT_CATCH

int hipdrt_debug_pfrt_combine(hipdrt_ctx* ctx, int B, int S, int neval_pfrt, int neval_out, const double* step_pfrt,
                              const double* rss, const double* sum_log_w, const double* factors, int m,
                              const hipdrt_pfrt_opts* opts, const double* ln_tau_pfrt, const double* ln_tau_out, double* pfrt,
                              double* raw_pfrt, double* post_prob) try {
    HIPDRT_REQUIRE(ctx && step_pfrt && rss && sum_log_w && factors && ln_tau_pfrt, "NULL pointer");
    HIPDRT_REQUIRE(B >= 1 && B <= 65535 && m >= 1, "1 <= B <= 65535, m >= 1");
    hipdrt_pfrt_opts o = opts_or(opts, hipdrt_pfrt_opts_default);
    // every check comes before the first launch (and the first upload)
    TRY(pfrt_check(o, S, neval_pfrt, neval_out));
    HIPDRT_REQUIRE(!o.smooth || ln_tau_out, "smoothing needs the output grid");
    for (int i = 0; i < S; ++i) HIPDRT_REQUIRE(factors[i] > 0.0 && std::isfinite(factors[i]), "factors must be positive and finite");
    const int np = neval_pfrt, nout = neval_out;
    std::vector<double> lnf(S);
    for (int i = 0; i < S; ++i) lnf[i] = std::log(factors[i]);
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf dstep, drss, dslw, dlnf, dltp, dlto;
    TRY(upload(dstep, step_pfrt, (size_t)S * B * np * sizeof(double), st));
    TRY(upload(drss, rss, (size_t)S * B * sizeof(double), st)); TRY(upload(dslw, sum_log_w, (size_t)S * B * sizeof(double), st));
    TRY(upload(dlnf, lnf.data(), (size_t)S * sizeof(double), st));
    TRY(upload(dltp, ln_tau_pfrt, (size_t)np * sizeof(double), st));
    if (o.smooth) TRY(upload(dlto, ln_tau_out, (size_t)nout * sizeof(double), st));
    PfrtCombineArgs a = pfrt_combine_args(o, m);
    a.S = S; a.np = np; a.nout = nout; a.ld_step = (long long)B * np; a.ld_sum = B;
    a.step_pfrt = dstep.d(); a.rss = drss.d(); a.slw = dslw.d(); a.ln_factors = dlnf.d();
    a.ltp = dltp.d(); a.lto = dlto.d();
    GuardedOuts outs;
    TRY(outs.want("pfrt", pfrt, (size_t)B * nout, a.pfrt, st)); TRY(outs.want("raw_pfrt", raw_pfrt, (size_t)B * np, a.raw, st));
    TRY(outs.want("post_prob", post_prob, (size_t)S * B, a.post, st));
    TRY(launch_pfrt_combine(st, a, B));
    LAUNCH_OK();
    return outs.back(st);
} HIPDRT_CATCH

int hipdrt_debug_pfrt_select(hipdrt_ctx* ctx, int B, int S, int neval_pfrt, const double* raw_pfrt, const double* step_pfrt,
                             const double* rss, const double* sum_log_w, int m, const hipdrt_pfrt_select_opts* sel,
                             hipdrt_pfrt_select_out* out, int* status) try {
    HIPDRT_REQUIRE(ctx && raw_pfrt && step_pfrt && rss && sum_log_w && out && status, "NULL pointer");
    HIPDRT_REQUIRE(B >= 1 && B <= 65535 && m >= 1, "1 <= B <= 65535, m >= 1");
    const hipdrt_pfrt_select_opts so = opts_or(sel, hipdrt_pfrt_select_opts_default);
    // every check comes before the first launch (and the first upload)
    HIPDRT_REQUIRE(S >= 1 && S <= 1024, "1 <= steps <= 1024");
    HIPDRT_REQUIRE(neval_pfrt >= 1 && neval_pfrt <= 2048, "pfrt_select: at most 2048 points on the tau_pfrt grid");
    TRY(pfrt_select_check(so));
    const int np = neval_pfrt, mp = so.max_peaks;
    const size_t bn = (size_t)B * np, bm = (size_t)B * mp;
    TRY(require_finite(raw_pfrt, bn)); TRY(require_finite(step_pfrt, (size_t)S * bn));
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf draw, dstep, drss, dslw;
    TRY(upload(draw, raw_pfrt, bn * sizeof(double), st)); TRY(upload(dstep, step_pfrt, (size_t)S * bn * sizeof(double), st));
    TRY(upload(drss, rss, (size_t)S * B * sizeof(double), st)); TRY(upload(dslw, sum_log_w, (size_t)S * B * sizeof(double), st));
    PfrtSelectArgs a{};
    a.S = S; a.np = np; a.max_peaks = mp; a.ld_step = (long long)bn; a.ld_sum = B;
    a.raw = draw.d(); a.step_pfrt = dstep.d(); a.rss = drss.d(); a.slw = dslw.d();
    pfrt_llh_consts(m, &a.c, &a.alpha_n, &a.beta_0);
    a.start_thresh = so.start_thresh; a.end_thresh = so.end_thresh; a.peak_thresh = so.peak_thresh;
    GuardedOuts outs;
    TRY(outs.want("num_peaks", out->num_peaks, (size_t)B, a.num_peaks, st)); TRY(outs.want("ranked_index", out->ranked_index, bm, a.ranked_index, st));
    TRY(outs.want("first", out->first, (size_t)B, a.first, st)); TRY(outs.want("num_candidates", out->num_candidates, (size_t)B, a.num_candidates, st));
    TRY(outs.want("step_index", out->step_index, bm, a.step_index, st)); TRY(outs.want("magnitude", out->magnitude, bm, a.magnitude, st));
    TRY(outs.want("match_quality", out->match_quality, bm, a.match_quality, st)); TRY(outs.want("status", status, (size_t)B, a.status, st));
    TRY(launch_pfrt_select(st, a, B));
    LAUNCH_OK();
    return outs.back(st);
} HIPDRT_CATCH

// test hook (include/hipdrt_debug.h): response_chain (plan_response.hip) as it is, on host arrays; out between borders of marker bytes
int hipdrt_debug_response(hipdrt_ctx* ctx, const hipdrt_debug_response_args* q) try {
    HIPDRT_REQUIRE(ctx && q && q->X && q->step_sizes && q->coefficient_scale && q->out, "NULL pointer");
    const int B = q->B, S = q->S, nt = q->nt, ntau = q->ntau, n = q->n, ns = q->ns, nd = q->dop_size, nvb = q->vb_size;
    HIPDRT_REQUIRE(B >= 1 && B <= 65535 && S >= 1 && nt >= 1 && nt <= 65535 && ntau >= 1 && n >= 1, "1 <= B, nt <= 65535; S, ntau, n >= 1");
    HIPDRT_REQUIRE((long long)S * nt <= (1 << 22) - 64, "S * nt < 2^22");
    HIPDRT_REQUIRE(q->copies == 1 || q->copies == 2, "copies: 1 or 2");
    HIPDRT_REQUIRE(ns >= 0 && (long long)ns + (long long)q->copies * ntau <= n, "the DRT block must lie inside [0, n)");
    HIPDRT_REQUIRE(nd >= 0 && q->dop_start >= 0 && (long long)q->dop_start + nd <= n, "the DOP block must lie inside [0, n)");
    HIPDRT_REQUIRE(nvb >= 0 && q->vb_start >= 0 && (long long)q->vb_start + nvb <= n, "the baseline block must lie inside [0, n)");
    for (int idx : {q->idx_rinf, q->idx_cinv, q->vz_index}) HIPDRT_REQUIRE(idx >= -1 && idx < n, "special indices: -1 or inside [0, n)");
    HIPDRT_REQUIRE(q->include_mask >= 0 && q->include_mask < 128, "include_mask: HIPDRT_INCLUDE_* bits");
    HIPDRT_REQUIRE(nvb == 0 || !q->vb_mat || (q->v_baseline_scale && q->response_signal_scale),
                   "a baseline term needs v_baseline_scale and response_signal_scale");
    hipStream_t st; TRY(enter(ctx, &st));
    const size_t tb = (size_t)nt * sizeof(double), bb = (size_t)B * sizeof(double);
    DevBuf dx, du, dud, ddsv, dxd, dsz, dcs, drss, dsro, dinf, dcap, dstr, dvb, dvs, dfs, t, tn, td;
    TRY(upload(dx, q->X, (size_t)B * n * sizeof(double), st));
    if (q->U) TRY(upload(du, q->U, (size_t)S * ntau * tb, st));
    const bool dop = q->Ud && nd > 0;
    if (dop) {
        TRY(upload(dud, q->Ud, (size_t)S * nd * tb, st));
        std::vector<double> ones((size_t)B * nd, 1.0);
        TRY(upload(ddsv, q->dop_scale_vector ? q->dop_scale_vector : ones.data(), ones.size() * sizeof(double), st));
        HIPDRT_CHECK(hipStreamSynchronize(st));       // (ones leaves scope)
        HIPDRT_CHECK(dxd.alloc(ones.size() * sizeof(double)));
    }
    TRY(upload(dsz, q->step_sizes, (size_t)(q->sizes_batched ? B : 1) * S * sizeof(double), st));
    TRY(upload(dcs, q->coefficient_scale, bb, st));
    ResponseArgs a{};
    a.S = S; a.nt = nt; a.mask = q->include_mask; a.sizes = dsz.d(); a.sizes_batched = q->sizes_batched != 0;
    a.X = dx.d(); a.ldx = n; a.cs = dcs.d();
    if (q->response_signal_scale) { TRY(upload(drss, q->response_signal_scale, bb, st)); a.rss = drss.d(); }
    if (q->scaled_response_offset) { TRY(upload(dsro, q->scaled_response_offset, bb, st)); a.sro = dsro.d(); }
    a.idx_rinf = q->idx_rinf; a.idx_cinv = q->idx_cinv; a.vz_index = q->vz_index; a.vb_start = q->vb_start; a.vb_size = nvb;
    a.capacitance_scale = q->capacitance_scale;
    if (q->inf_rv) { TRY(upload(dinf, q->inf_rv, (q->inf_batched ? B : 1) * tb, st)); a.inf_rv = dinf.d(); a.inf_batched = q->inf_batched != 0; }
    if (q->cap_rv) { TRY(upload(dcap, q->cap_rv, (q->cap_batched ? B : 1) * tb, st)); a.cap_rv = dcap.d(); a.cap_batched = q->cap_batched != 0; }
    if (q->vz_strength) { TRY(upload(dstr, q->vz_strength, tb, st)); a.strength = dstr.d(); }
    if (q->vb_mat && nvb > 0) {
        TRY(upload(dvb, q->vb_mat, tb * nvb, st)); a.vb_mat = dvb.d();
        TRY(upload(dvs, q->v_baseline_scale, (size_t)nvb * sizeof(double), st)); a.vb_scale = dvs.d();
    }
    if (q->fit_status) { TRY(upload(dfs, q->fit_status, (size_t)B * sizeof(int), st)); a.fit_status = dfs.i(); }
    Guarded g;
    TRY(g.up("out", q->out, (size_t)B * tb, st));
    a.out = g.dd();
    if (dop) launch_scale_block(st, B, nd, dx.d(), n, q->dop_start, ddsv.d(), dxd.d());
    TRY(response_chain(st, B, ntau, q->copies, ns, q->U ? du.d() : nullptr, dop ? dud.d() : nullptr, dop ? dxd.d() : nullptr, nd,
                       a, t, tn, td));
    TRY(g.fetch(st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return g.check();
} HIPDRT_CATCH

// test hook (include/hipdrt_debug.h): peak_resolve_kernel as it is, on host arrays.  Every output sits between two borders of marker bytes.
int hipdrt_debug_peak_resolve(hipdrt_ctx* ctx, const hipdrt_debug_peak_resolve_args* q) try {
    HIPDRT_REQUIRE(ctx && q && q->f && q->fxx && q->x && q->ln_tau_find && q->ln_basis, "NULL pointer");
    const int B = q->B, nfind = q->nfind, nb = q->nb, nout = q->nout;
    HIPDRT_REQUIRE(B >= 1 && B <= 65535 && nfind >= 1 && nfind <= (1 << 20) && nb >= 1 && nb <= (1 << 20) && nout >= 0 && nout <= (1 << 20),
                   "1 <= B <= 65535, 1 <= nfind, nb <= 2^20, 0 <= nout <= 2^20");
    HIPDRT_REQUIRE(q->copies == 1 || q->copies == 2, "copies must be 1 or 2");
    HIPDRT_REQUIRE(nout == 0 || (q->ln_tau_out && q->basis_eps > 0.0 && std::isfinite(q->basis_eps)), "an output grid needs ln_tau_out and basis_eps > 0");
    hipdrt_peak_resolve_opts o = opts_or(q->opts, hipdrt_peak_resolve_opts_default);
    TRY(peak_resolve_check_opts(o));
    const int mp = o.max_peaks;
    HIPDRT_REQUIRE(q->copies == 2 || o.sign == 1, "sign must be 1 unless the DRT block holds a positive and a negative copy");
    const size_t lds = peak_resolve_lds_bytes(nfind, nb, nout, mp);
    if (q->lds_bytes) *q->lds_bytes = (long long)lds;
    HIPDRT_REQUIRE(q->source != 0 || q->keep, "source 0 needs the keep rows");
    TRY(peak_resolve_check_source(q->source, q->indices, B, mp, q->win_start, q->win_end, q->nwin, nfind));
    const size_t bn = (size_t)B * nfind, bx = (size_t)B * q->copies * nb;
    TRY(require_finite(q->f, bn)); TRY(require_finite(q->fxx, bn));
    for (size_t i = 0; i < bx; ++i) HIPDRT_REQUIRE(std::isfinite(q->x[i]), "non-finite coefficients");
    for (int i = 0; i < nfind; ++i) HIPDRT_REQUIRE(std::isfinite(q->ln_tau_find[i]), "non-finite find grid");
    for (int i = 0; i < nb; ++i) HIPDRT_REQUIRE(std::isfinite(q->ln_basis[i]), "non-finite basis grid");
    for (int i = 0; i < nout; ++i) HIPDRT_REQUIRE(std::isfinite(q->ln_tau_out[i]), "non-finite output grid");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf df, dfxx, dkeep, didx, dws, dwe, dx, dlt, dlb, dlo, dE0, dfs;
    TRY(upload(df, q->f, bn * sizeof(double), st)); TRY(upload(dfxx, q->fxx, bn * sizeof(double), st));
    TRY(upload(dx, q->x, bx * sizeof(double), st));
    TRY(upload(dlt, q->ln_tau_find, (size_t)nfind * sizeof(double), st)); TRY(upload(dlb, q->ln_basis, (size_t)nb * sizeof(double), st));
    PeakResolveArgs a{};
    a.nfind = nfind; a.nb = nb; a.nout = nout; a.source = q->source; a.nwin = q->nwin; a.copies = q->copies; a.o = o;
    a.f = df.d(); a.fxx = dfxx.d(); a.X = dx.d(); a.ldx = (long long)q->copies * nb; a.col_offset = 0; a.cs = nullptr;
    a.lt = dlt.d(); a.lb = dlb.d();
    if (q->source == 0) { TRY(upload(dkeep, q->keep, bn * sizeof(int), st)); a.keep = dkeep.i(); }
    if (q->source == 1) { TRY(upload(didx, q->indices, (size_t)B * mp * sizeof(int), st)); a.indices = didx.i(); }
    if (q->source == 2) {
        TRY(upload(dws, q->win_start, (size_t)q->nwin * sizeof(int), st)); TRY(upload(dwe, q->win_end, (size_t)q->nwin * sizeof(int), st));
        a.win_start = dws.i(); a.win_end = dwe.i();
    }
    if (q->fit_status) { TRY(upload(dfs, q->fit_status, (size_t)B * sizeof(int), st)); a.fit_status = dfs.i(); }
    if (nout > 0) {
        TRY(upload(dlo, q->ln_tau_out, (size_t)nout * sizeof(double), st));
        HIPDRT_CHECK(dE0.alloc((size_t)nout * nb * sizeof(double)));
        TRY(func_eval_dev(st, dlb.d(), nb, dlo.d(), nout, q->basis_eps, 0, 1.0, dE0.d(), nb));
        a.E0 = dE0.d(); a.lto = dlo.d();
        a.basis_area = basis_area(q->basis_eps);
    } else {
        a.basis_area = q->basis_eps > 0.0 ? basis_area(q->basis_eps) : 1.0;
    }
    const size_t bm = (size_t)B * mp;
    const hipdrt_peak_resolve_out& u = q->out;
    GuardedOuts outs;
    TRY(outs.want("count", u.count, (size_t)B, a.count, st)); TRY(outs.want("status", u.status, (size_t)B, a.status, st));
    TRY(outs.want("peak_index", u.peak_index, bm, a.peak_index, st)); TRY(outs.want("trough_index", u.trough_index, bm, a.trough_index, st));
    TRY(outs.want("eps_l", u.eps_l, bm, a.eps_l, st)); TRY(outs.want("eps_r", u.eps_r, bm, a.eps_r, st));
    TRY(outs.want("r_peaks", u.r_peaks, bm, a.r_peaks, st)); TRY(outs.want("r_coef", u.r_coef, bm, a.r_coef, st));
    TRY(outs.want("x_peaks", u.x_peaks, bm * nb, a.x_peaks, st));
    TRY(outs.want("peak_gammas", nout > 0 ? u.peak_gammas : nullptr, bm * nout, a.peak_gammas, st));
    TRY(launch_peak_resolve(st, a, B));
    LAUNCH_OK();
    return outs.back(st);
} HIPDRT_CATCH

// test hooks (include/hipdrt_debug.h): the likelihood kernels of candidates.hip as they are, on host arrays; outputs between borders
// of marker bytes
int hipdrt_debug_candidate_llh(hipdrt_ctx* ctx, int C, int B, int m, int n, const double* rm, int rm_batched, const double* rv,
                               const double* vmm, const double* var_floor, const double* x, double* rss, double* sum_log_w) try {
    HIPDRT_REQUIRE(ctx && rm && rv && vmm && var_floor && x && rss && sum_log_w, "NULL pointer");
    HIPDRT_REQUIRE(C >= 1 && C <= 4096 && B >= 1 && B <= 65535 && m >= 1 && m <= 16384 && n >= 1 && n <= 16384,
                   "1 <= C <= 4096, 1 <= B <= 65535, 1 <= m, n <= 16384");
    const int form = cand_llh_form(ctx, m);
    HIPDRT_REQUIRE(form == 1 || cand_llh_fits_lds(m), "candidates: 16 rows of m doubles do not fit in LDS; use the scratch form");
    hipStream_t st; TRY(enter(ctx, &st));
    const size_t D = sizeof(double), cb = (size_t)C * B;
    DevBuf drm, drv, dvmm, dvf, dx, dscr;
    TRY(upload(drm, rm, (size_t)(rm_batched ? B : 1) * m * n * D, st)); TRY(upload(drv, rv, (size_t)B * m * D, st));
    TRY(upload(dvmm, vmm, (size_t)m * m * D, st)); TRY(upload(dvf, var_floor, (size_t)B * D, st));
    TRY(upload(dx, x, cb * n * D, st));
    if (form == 1) HIPDRT_CHECK(dscr.alloc(cand_llh_scratch_doubles(C, B, m) * D));
    CandLlhArgs a{};
    a.C = C; a.B = B; a.m = m; a.n = n; a.x = dx.d(); a.x_cstride = (long long)B * n; a.x_bstride = n;
    a.rm = drm.d(); a.ldrm = n; a.rm_stride = rm_batched ? (long long)m * n : 0; a.rv = drv.d(); a.vmm = dvmm.d();
    a.var_floor = dvf.d(); a.scratch = dscr.d();
    GuardedOuts outs;
    TRY(outs.want("rss", rss, cb, a.rss, st)); TRY(outs.want("sum_log_w", sum_log_w, cb, a.slw, st));
    TRY(launch_cand_llh(st, a, form));
    LAUNCH_OK();
    return outs.back(st);
} HIPDRT_CATCH

int hipdrt_debug_candidate_form(hipdrt_ctx* ctx, int form) try {
    HIPDRT_REQUIRE(ctx, "NULL pointer");
    HIPDRT_REQUIRE(form >= -1 && form <= 1, "form must be -1 (automatic), 0 (LDS) or 1 (scratch)");
    ctx->cand_form = form;
    return HIPDRT_OK;
} HIPDRT_CATCH

// test hook (include/hipdrt_debug.h): the posterior chain of plan_post.hip -- posterior_var_dev and posterior_cov_dev, the functions
// the plan entry points call -- on a P and rows of the caller's.  Every device output sits between borders of marker bytes, and so
// does every spectrum's factor scratch.
// d: the DOP form (hipdrt_debug_dop_posterior), null: the chain as it is
static int debug_posterior_run(hipdrt_ctx* ctx, const hipdrt_debug_posterior_args* a, const hipdrt_debug_dop_posterior_args* d) {
    HIPDRT_REQUIRE(ctx && a && a->P && a->rows, "NULL pointer");
    const int B = a->B, n = a->n, neval = a->neval, ncol = a->ncol, off = a->col_offset, ldp = a->ldp, cm = a->cov_member;
    HIPDRT_REQUIRE(n >= 1 && n <= 4096 && B >= 1 && B <= 4096, "1 <= n <= 4096, 1 <= B <= 4096");
    HIPDRT_REQUIRE(neval >= 1 && neval <= 65536, "1 <= neval <= 65536");
    HIPDRT_REQUIRE(ncol >= 1 && off >= 0 && off <= n && ncol <= n - off, "the rows' columns must lie inside [0, n)");
    HIPDRT_REQUIRE(ldp >= n, "ldp >= n");
    HIPDRT_REQUIRE(cm >= -1 && cm < B, "cov_member: -1 or a spectrum index");
    HIPDRT_REQUIRE(!a->cov || cm >= 0, "cov needs cov_member");
    HIPDRT_REQUIRE(!a->tail || cm >= 0 || B <= 256, "tail: the spectra of one chunk only (B <= 256)");
    const int pb = a->p_batched ? B : 1;
    for (int b = 0; b < pb; ++b)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) HIPDRT_REQUIRE(std::isfinite(a->P[((size_t)b * n + i) * ldp + j]), "non-finite P");
    for (size_t i = 0; i < (size_t)neval * ncol; ++i) HIPDRT_REQUIRE(std::isfinite(a->rows[i]), "non-finite rows");
    if (a->scale) for (int b = 0; b < B; ++b) HIPDRT_REQUIRE(std::isfinite(a->scale[b]), "non-finite scale");
    const int nd = d ? d->dop_size : 0;
    if (d) {
        HIPDRT_REQUIRE(d->dop_scale_vector, "NULL pointer");
        HIPDRT_REQUIRE(nd >= 1 && d->dop_start >= 0 && d->dop_start <= n && nd <= n - d->dop_start, "the DOP block must lie inside [0, n) and hold a column");
        for (size_t k = 0; k < (size_t)(d->dop_scale_batched ? B : 1) * nd; ++k)
            HIPDRT_REQUIRE(d->dop_scale_vector[k] > 0.0 && std::isfinite(d->dop_scale_vector[k]), "dop_scale_vector must be finite and positive");
    }
    hipStream_t st; TRY(enter(ctx, &st));
    const size_t D = sizeof(double), ppk = qp_ppk_doubles(n), G = Guarded::G / D;
    const int nex = (neval + 15) / 16, nchp = qp_nchp(n);
    const bool single = cm >= 0;
    const int nb = single ? 1 : B, first = single ? cm : 0;
    // P -> packed tiles as the stand-alone QP entry point packs it (lower triangle); tiles the kernel does not write stay zero
    DevBuf dP, dPpk, drows, scratch;
    TRY(upload(dP, a->P, (size_t)pb * n * ldp * D, st));
    // (the DOP form: every member has an image of its own, between borders; a shared P is packed into each)
    const int ni = d ? B : pb;
    const bool own = d || a->p_batched;
    Guarded gpk;
    double* images = nullptr;
    if (d) {
        TRY(gpk.up("ppk", nullptr, (size_t)ni * ppk * D, st));
        images = gpk.dd();
    } else {
        HIPDRT_CHECK(dPpk.alloc((size_t)ni * ppk * D));
        images = dPpk.d();
    }
    HIPDRT_CHECK(hipMemsetAsync(images, 0, (size_t)ni * ppk * D, st));
    if (d && !a->p_batched) for (int b = 0; b < B; ++b) launch_pack_p(st, 1, n, dP.d(), ldp, images + (size_t)b * ppk);
    else launch_pack_p(st, pb, n, dP.d(), ldp, images);
    LAUNCH_OK();
    DevBuf ddsv, dsinv;
    if (d) {
        // 1 / dop_scale_vector of every member, then S P S on the images the chain will read: all of them, or member cm's alone in
        // the single-member form (strides 0, its own scale row)
        TRY(upload(ddsv, d->dop_scale_vector, (size_t)(d->dop_scale_batched ? B : 1) * nd * D, st));
        HIPDRT_CHECK(dsinv.alloc((size_t)B * nd * D));
        launch_dop_recip(st, B, nd, ddsv.d(), d->dop_scale_batched ? nd : 0, dsinv.d());
        launch_scale_p(st, nb, n, d->dop_start, nd, dsinv.d() + (size_t)first * nd, single ? 0 : nd, images + (size_t)first * ppk,
                       single ? 0 : (long long)ppk);
        LAUNCH_OK();
    }
    TRY(upload(drows, a->rows, (size_t)neval * ncol * D, st));
    std::vector<double> hvar((size_t)nb * nex * 16, 0.0), hbex((size_t)nex * nchp * 256, 0.0), hcov;
    std::vector<int> hstat(nb, 0);
    PosteriorChain c{};
    c.nb = nb; c.n = n; c.ppk = images + (own ? (size_t)first * ppk : 0); c.pstr = (own && !single) ? (long long)ppk : 0;
    c.single = single; c.rows = drows.d(); c.neval = neval; c.ncol = ncol; c.col_offset = off; c.guard = G;
    GuardedOuts outs;
    double* dcov = nullptr;
    TRY(outs.want("var", hvar.data(), hvar.size(), c.var, st));
    TRY(outs.want("status", hstat.data(), hstat.size(), c.status, st));
    TRY(outs.want("bex", hbex.data(), hbex.size(), c.bex, st));
    if (a->cov) { hcov.assign((size_t)neval * neval, 0.0); TRY(outs.want("cov", hcov.data(), hcov.size(), dcov, st)); }
    TRY(posterior_var_dev(st, c, scratch));
    int bad = 0;
    if (a->cov) {
        HIPDRT_CHECK(hipMemcpyAsync(&bad, c.status, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPDRT_CHECK(hipStreamSynchronize(st));
        if (!bad) { posterior_cov_dev(st, scratch.d() + G, n, neval, a->scale ? a->scale[cm] : 1.0, dcov); LAUNCH_OK(); }
    }
    // the factor scratch: its borders, then the rows left behind every factor
    const size_t lsz = dist_var_scratch_doubles(n, nex), nch = (size_t)nchp, tl = (size_t)nex * nch * 256;
    const int chunk = nb < 256 ? nb : 256;
    std::vector<double> hs(scratch.bytes / D);
    HIPDRT_CHECK(hipMemcpyAsync(hs.data(), scratch.p, scratch.bytes, hipMemcpyDeviceToHost, st));
    TRY(outs.back(st));
    const unsigned char* raw = reinterpret_cast<const unsigned char*>(hs.data());
    for (int k = 0; k <= chunk; ++k)
        for (size_t i = 0; i < Guarded::G; ++i)
            if (raw[(size_t)k * (lsz + G) * D + i] != Guarded::MARK) {
                set_error("the kernel under test wrote outside a spectrum's factor scratch");
                return HIPDRT_E_NUMERIC;
            }
    if (a->var) posterior_var_host(hvar.data(), nb, neval, a->scale ? a->scale + first : nullptr, a->var);
    if (a->status) std::memcpy(a->status, hstat.data(), (size_t)nb * sizeof(int));
    if (a->bex) std::memcpy(a->bex, hbex.data(), hbex.size() * D);
    if (a->cov) for (size_t i = 0; i < hcov.size(); ++i) a->cov[i] = bad ? __builtin_nan("") : hcov[i];
    if (a->tail)
        for (int k = 0; k < nb; ++k) std::memcpy(a->tail + (size_t)k * tl, hs.data() + G + (size_t)k * (lsz + G) + nch * nch * 256, tl * D);
    if (d) {
        TRY(gpk.fetch(st));
        HIPDRT_CHECK(hipStreamSynchronize(st));
        TRY(gpk.check());
        if (d->ppk) std::memcpy(d->ppk, gpk.data() + (size_t)first * ppk * D, (size_t)nb * ppk * D);
    }
    return HIPDRT_OK;
}

int hipdrt_debug_posterior(hipdrt_ctx* ctx, const hipdrt_debug_posterior_args* a) try {
    return debug_posterior_run(ctx, a, nullptr);
} HIPDRT_CATCH

// test hook (include/hipdrt_debug.h): the same chain behind launch_scale_p, as plan_quadratic_forms_dev runs it for the DOP posterior
int hipdrt_debug_dop_posterior(hipdrt_ctx* ctx, const hipdrt_debug_dop_posterior_args* a) try {
    HIPDRT_REQUIRE(a, "NULL pointer");
    return debug_posterior_run(ctx, &a->post, a);
} HIPDRT_CATCH

// test hook (include/hipdrt_debug.h): lpt_order_kernel alone
int hipdrt_debug_lpt_order(hipdrt_ctx* ctx, int B, const int* iters, const int* active, int* order) try {
    HIPDRT_REQUIRE(ctx && iters && order, "NULL pointer");
    HIPDRT_REQUIRE(B >= 1 && (size_t)B * sizeof(int) <= 48 * 1024, "B >= 1, B * sizeof(int) <= 48 KiB (the fit loop's own condition)");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf dit, dact;
    TRY(upload(dit, iters, (size_t)B * sizeof(int), st));
    if (active) TRY(upload(dact, active, (size_t)B * sizeof(int), st));
    Guarded g;
    TRY(g.up("order", order, (size_t)B * sizeof(int), st));
    launch_lpt_order(st, B, dit.i(), active ? dact.i() : nullptr, reinterpret_cast<int*>(g.dd()));
    LAUNCH_OK();
    TRY(g.fetch(st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return g.check();
} HIPDRT_CATCH

// test hook (include/hipdrt_debug.h): launch_qp as the fit loop calls it (loop_qp_args, plan_fit.hip), on host arrays.  Every in/out
// array, every problem's state block and factor scratch and the group kernel's sync words sit between borders of marker bytes.
int hipdrt_debug_qp(hipdrt_ctx* ctx, const hipdrt_debug_qp_args* a) try {
    HIPDRT_REQUIRE(ctx && a && a->P && a->q && a->h && a->x && a->status, "NULL pointer");
    const int B = a->B, n = a->n, ldp = a->ldp;
    HIPDRT_REQUIRE(n >= 1 && n <= 4096 && B >= 1 && B <= 4096, "1 <= n <= 4096, 1 <= B <= 4096");
    HIPDRT_REQUIRE(ldp >= n, "ldp >= n");
    HIPDRT_REQUIRE(!(a->order && a->use_lpt), "order and use_lpt exclude each other");
    HIPDRT_REQUIRE(!a->use_lpt || a->iters, "use_lpt ranks the uploaded iters");
    const int G = qp_group_size(B, n, ctx->qp_force_group);
    HIPDRT_REQUIRE(G >= 0, "n not supported");
    HIPDRT_REQUIRE(!(ctx->qp_force_group == 0 && n > 2048), "n > 2048 needs the group kernel, and this context forces the batch kernel");
    const int pb = a->p_batched ? B : 1, hb = a->h_batched ? B : 1;
    for (int b = 0; b < pb; ++b)
        for (int i = 0; i < n; ++i)
            for (int j = 0; j < n; ++j) HIPDRT_REQUIRE(std::isfinite(a->P[((size_t)b * n + i) * ldp + j]), "non-finite P");
    for (size_t i = 0; i < (size_t)B * n; ++i) HIPDRT_REQUIRE(std::isfinite(a->q[i]), "non-finite q");
    for (size_t i = 0; i < (size_t)hb * n; ++i) HIPDRT_REQUIRE(std::isfinite(a->h[i]), "non-finite h");
    if (a->order) {
        std::vector<char> seen((size_t)B, 0);
        for (int i = 0; i < B; ++i) {
            const int o = a->order[i];
            HIPDRT_REQUIRE(o >= 0 && o < B && !seen[(size_t)o], "order must be a permutation of 0 .. B - 1");
            seen[(size_t)o] = 1;
        }
    }
    hipStream_t st; TRY(enter(ctx, &st));
    const size_t D = sizeof(double), ppk = qp_ppk_doubles(n);
    const int Gm = G > 1 ? G : 1;
    const bool gu = G == 0 && qp_scratch_doubles(n, 0) > ppk;       // the scratch holds more than the factor's tiles: the inverse blocks
    if (a->form) { a->form[0] = G; a->form[1] = gu ? 1 : 0; a->form[2] = (G == 0 && !gu && ctx->qp_waves == 4) ? 4 : 8; }
    // P -> packed tiles (lower triangle); the kernel never sees the row-major copy
    DevBuf dP, dPpk, dq, dh, dact;
    TRY(upload(dP, a->P, (size_t)pb * n * ldp * D, st));
    HIPDRT_CHECK(dPpk.alloc((size_t)pb * ppk * D));
    HIPDRT_CHECK(hipMemsetAsync(dPpk.p, 0, dPpk.bytes, st));
    launch_pack_p(st, pb, n, dP.d(), ldp, dPpk.d());
    LAUNCH_OK();
    TRY(upload(dq, a->q, (size_t)B * n * D, st));
    TRY(upload(dh, a->h, (size_t)hb * n * D, st));
    if (a->active) TRY(upload(dact, a->active, (size_t)B * sizeof(int), st));
    QpArgs qa{};
    qa.B = B; qa.n = n; qa.ldp = ldp; qa.q = dq.d(); qa.h = dh.d(); qa.h_stride = a->h_batched ? n : 0;
    qa.P = nullptr; qa.p_stride = (long long)n * ldp; qa.active = a->active ? dact.i() : nullptr;
    qa.Ppk = dPpk.d(); qa.ppk_stride = a->p_batched ? (long long)ppk : 0; qa.nchp = qp_nchp(n);
    qa.opts = a->opts ? *a->opts : default_qp_opts();
    qa.G = G; qa.waves = ctx->qp_waves;
    GuardedOuts g;
    TRY(g.want("x", a->x, (size_t)B * n, qa.x, st)); TRY(g.want("iters", a->iters, (size_t)B, qa.iters, st));
    TRY(g.want("pcost", a->pcost, (size_t)B, qa.pcost, st)); TRY(g.want("status", a->status, (size_t)B, qa.status, st));
    TRY(g.want("iters_accum", a->iters_accum, (size_t)B, qa.iters_accum, st));
    std::vector<int> horder;
    int* dorder = nullptr;
    if (a->order || a->use_lpt) {
        horder.assign((size_t)B, -1);
        if (a->order) std::memcpy(horder.data(), a->order, (size_t)B * sizeof(int));
        TRY(g.want("order", horder.data(), (size_t)B, dorder, st));
        if (a->use_lpt) { launch_lpt_order(st, B, qa.iters, qa.active, dorder); LAUNCH_OK(); }     // as outer_iteration does
        qa.order = dorder;
    }
    std::vector<int> hsync;
    if (G >= 1) {
        hsync.assign((size_t)B * qp_gsync_ints(), 0);
        TRY(g.want("the sync words", hsync.data(), hsync.size(), qa.gsync, st));
    }
    GuardedBlocks L, S;
    TRY(L.alloc(qp_scratch_doubles(n, G), (size_t)B, st));
    TRY(S.alloc(qp_state_doubles(n), (size_t)B * Gm, st));
    qa.L = L.first(); qa.ldl = (int)qp_scratch_ld(n); qa.l_stride = (long long)L.stride();
    qa.state = S.first(); qa.state_ld = qp_state_ld(n); qa.state_stride = (long long)S.stride();
    TRY(launch_qp(st, qa));
    LAUNCH_OK();
    std::vector<double> hs(S.buf.bytes / D);
    HIPDRT_CHECK(hipMemcpyAsync(hs.data(), S.buf.p, S.buf.bytes, hipMemcpyDeviceToHost, st));
    TRY(g.back(st));
    TRY(L.check("a problem's factor scratch", st));
    TRY(S.check("a problem's state block", st));
    if (a->order_out)
        for (int i = 0; i < B; ++i) a->order_out[i] = qa.order ? horder[(size_t)i] : i;
    // s and z: state vectors 2 and 1 of the leader's copy, slot b * max(G, 1) -- or slot b when the launcher fell back to one member
    // per problem (qp.hip: launch_qp); the leader's copy is the one whose vector 0 is the x that came back
    if (a->s || a->z)
        for (int b = 0; b < B; ++b) {
            if (a->active && !a->active[b]) continue;
            const int sld = qp_state_ld(n);
            const double* blk = nullptr;
            for (size_t slot : {(size_t)b * Gm, (size_t)b}) {
                const double* c = hs.data() + GuardedBlocks::GD + slot * S.stride();
                if (std::memcmp(c, a->x + (size_t)b * n, (size_t)n * D) == 0) { blk = c; break; }
            }
            if (!blk) { set_error("the leader's state block does not hold the x that came back"); return HIPDRT_E_NUMERIC; }
            if (a->s) std::memcpy(a->s + (size_t)b * n, blk + (size_t)2 * sld, (size_t)n * D);
            if (a->z) std::memcpy(a->z + (size_t)b * n, blk + (size_t)1 * sld, (size_t)n * D);
        }
    return HIPDRT_OK;
} HIPDRT_CATCH

// tools hook: kernel time of the last hipdrt_plan_predict_drt or hipdrt_plan_predict_z on this context
int hipdrt_debug_last_predict_ms(hipdrt_ctx* ctx, float* ms) try {
    HIPDRT_REQUIRE(ctx && ms, "NULL pointer");
    ms[0] = ctx->predict_ms[0]; ms[1] = ctx->predict_ms[1];
    return HIPDRT_OK;
} HIPDRT_CATCH

}  // extern "C"
