// What reads a finished fit of a plan (include/hipdrt.h): log-likelihood terms, the posterior covariance and variance,
// Kramers-Kronig screening (csrc/kk.hip), model evaluation (csrc/predict.hip), peak finding (csrc/peaks.hip) and per-peak
// resolution (csrc/peak_resolve.hip).
#include <cmath>
#include <cstring>

#include "plan.hpp"

namespace hipdrt {
int kk_check_opts(const hipdrt_kk_opts& o) {
    HIPDRT_REQUIRE(o.n_outlier_iter >= 0 && o.n_outlier_iter <= 100, "0 <= n_outlier_iter <= 100");
    HIPDRT_REQUIRE(o.n_sigma > 0.0 || (o.p_thresh > 0.0 && o.p_thresh < 1.0), "0 < p_thresh < 1");
    HIPDRT_REQUIRE(o.std_sample_fraction > 0.0 && o.std_sample_fraction <= 1.0, "0 < std_sample_fraction <= 1");
    HIPDRT_REQUIRE(o.n_std > 0.0 && std::isfinite(o.n_std), "n_std > 0");
    HIPDRT_REQUIRE(o.max_num_outliers >= 0, "max_num_outliers >= 0");
    HIPDRT_REQUIRE(o.outlier_weight > 0.0 && std::isfinite(o.outlier_weight), "outlier_weight > 0");
    return HIPDRT_OK;
}

int peak_resolve_check_source(int source, const int* indices, int B, int max_peaks, const int* win_start, const int* win_end,
                              int nwin, int nfind) {
    HIPDRT_REQUIRE(source >= 0 && source <= 2, "source must be 0 (find_peaks), 1 (indices) or 2 (windows)");
    if (source == 1) {
        HIPDRT_REQUIRE(indices, "source 1 needs peak_indices");
        for (int b = 0; b < B; ++b) {
            int prev = -1;
            bool ended = false;
            for (int i = 0; i < max_peaks; ++i) {
                const int v = indices[(size_t)b * max_peaks + i];
                if (v == -1) { ended = true; continue; }
                HIPDRT_REQUIRE(!ended, "peak_indices: -1 only as padding at the end of a row");
                HIPDRT_REQUIRE(v >= 0 && v < nfind, "peak_indices out of range of the find grid");
                HIPDRT_REQUIRE(v > prev, "peak_indices must be strictly increasing within a spectrum");
                prev = v;
            }
        }
    } else if (source == 2) {
        HIPDRT_REQUIRE(win_start && win_end, "source 2 needs win_start and win_end");
        HIPDRT_REQUIRE(nwin >= 1 && nwin <= max_peaks, "1 <= nwin <= max_peaks");
        for (int k = 0; k < nwin; ++k) {
            HIPDRT_REQUIRE(win_start[k] >= 0 && win_start[k] < nfind && win_end[k] > win_start[k] && win_end[k] <= nfind + 1,
                           "windows: 0 <= start < end <= nfind + 1, start < nfind");
            HIPDRT_REQUIRE(k == 0 || (win_start[k] >= win_start[k - 1] && win_end[k] >= win_end[k - 1]), "windows must be ascending");
        }
    }
    return HIPDRT_OK;
}
}  // namespace hipdrt

extern "C" {

static int plan_llh_terms(hipdrt_plan* p, double* rss, double* sum_log_w, int stored, double scalar_w = 1.0);

int hipdrt_plan_llh_terms(hipdrt_plan* p, double* rss, double* sum_log_w) { return plan_llh_terms(p, rss, sum_log_w, 0); }

int hipdrt_plan_obs_llh_terms(hipdrt_plan* p, double* rss, double* sum_log_w) { return plan_llh_terms(p, rss, sum_log_w, 1); }

int hipdrt_plan_obs_llh_terms_w(hipdrt_plan* p, int weights_mode, double scalar_weight, double* rss, double* sum_log_w) try {
    HIPDRT_REQUIRE(weights_mode == HIPDRT_LLH_W_EST || weights_mode == HIPDRT_LLH_W_UNIFORM || weights_mode == HIPDRT_LLH_W_SCALAR,
                   "weights_mode");
    HIPDRT_REQUIRE(weights_mode != HIPDRT_LLH_W_SCALAR || scalar_weight > 0.0, "scalar weight must be positive");
    return plan_llh_terms(p, rss, sum_log_w, weights_mode, scalar_weight);
} HIPDRT_CATCH

static int plan_llh_terms(hipdrt_plan* p, double* rss, double* sum_log_w, int stored, double scalar_w) {
    HIPDRT_REQUIRE(p && rss && sum_log_w, "NULL pointer");
    HIPDRT_REQUIRE(p->B >= 1, "no fitted batch in the plan");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const size_t bb = (size_t)p->B * sizeof(double);
    DevBuf d1, d2;
    HIPDRT_CHECK(d1.alloc(bb)); HIPDRT_CHECK(d2.alloc(bb));
    TRY(launch_llh(st, p->state(), p->B, d1.d(), d2.d(), stored, scalar_w));
    LAUNCH_OK();
    HIPDRT_CHECK(hipMemcpyAsync(rss, d1.p, bb, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(sum_log_w, d2.p, bb, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
}

// What the posterior entry points call "the final P": calculate_pq with the final weights / s / rho (drt1d.py:1006), from
// calculate_pq's scaled_weights -- w_eff whenever the plan has weight factors.  b >= 0: s, rho, dop_rho and the weights of
// spectrum b alone.
struct FinalP { GramL2 g; const double* w; };
// Where a posterior computation reads the fitted state from: the plan's live buffers (what the last fit or warm restart left), or
// one recorded step of the PFRT store with the raw re-estimated weights of that step (step_source).  All [B]-major with the
// strides of the live buffers.
struct PostSource { const double *x, *s, *rho, *dop_rho, *w; const int* fit_status; };
static PostSource live_source(const hipdrt_plan* p) {
    return {p->x.d(), p->s.d(), p->rho.d(), p->dop_rho.d(), p->has_weight_factors() ? p->w_eff.d() : p->w.d(), p->fit_status.i()};
}
static PostSource step_source(const hipdrt_plan* p, int step, const double* w, const int* fit_status) {
    const PfrtStoreLayout L = p->pf_layout();
    return {p->pf_x.d() + L.x(step), p->pf_s.d() + L.s(step), p->pf_rho.d() + L.rho(step),
            p->pf_dop_rho.p ? p->pf_dop_rho.d() + L.rho(step) : nullptr, w, fit_status};
}
static FinalP plan_final_p(const hipdrt_plan* p, int b, const PostSource& src) {
    FinalP f{plan_l2(p, p->opts.l2_lambda_0, p->opts.derivative_weights, p->prepared ? p->desc.dop_l2_lambda_0 : 0.0), src.w};
    f.g.s = src.s; f.g.rho = src.rho;
    if (f.g.dop_size > 0) f.g.dop_rho = src.dop_rho;
    if (b >= 0) {
        f.g.s += (size_t)b * 3 * p->n; f.g.rho += (size_t)b * 3;
        if (f.g.dop_size > 0) f.g.dop_rho += (size_t)b * 3;
        f.w += (size_t)b * p->m;
    }
    return f;
}

int hipdrt_plan_get_p_matrix(hipdrt_plan* p, int b, double* out) try {
    HIPDRT_REQUIRE(p && out, "NULL pointer");
    HIPDRT_REQUIRE(b >= 0 && b < p->B, "spectrum index out of range");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const int n = p->n, m = p->m;
    const FinalP f = plan_final_p(p, b, live_source(p));
    launch_gram_l2(st, 1, m, n, p->rm.d() + (size_t)b * p->rm_stride, p->ldrm, f.w, f.g, p->Ptmp.d(), p->ldp, 0, nullptr);
    LAUNCH_OK();
    return copy_strided(out, p->Ptmp.d(), n, n, p->ldp, st);
} HIPDRT_CATCH

// rows_dev[neval][ncol] in device memory (it sits at columns col_offset.. of the unknown vector, zero elsewhere) ->
// dout[B][nex * 16] = rows_i' P_b^-1 rows_i (not yet scaled by cs_b^2), dstat[B]
static int plan_quadratic_forms_dev(hipdrt_plan* p, const PostSource& src, const double* rows_dev, int neval, int ncol,
                                    int col_offset, DevBuf& dout, DevBuf& dstat) {
    HIPDRT_REQUIRE(p->B > 0, "no fitted batch in the plan");
    HIPDRT_REQUIRE(neval >= 1, "neval >= 1");
    HIPDRT_REQUIRE(p->n <= 4096, "posterior variance: n <= 4096");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const int n = p->n, m = p->m, B = p->B;
    const int nex = (neval + 15) / 16, nchp = qp_nchp(n);
    // final P of every spectrum, packed tiles only
    const FinalP f = plan_final_p(p, -1, src);
    launch_gram_l2(st, B, m, n, p->rm.d(), p->ldrm, f.w, f.g, nullptr, p->ldp, 0, nullptr, p->Ppk.d(),
                   (long long)qp_ppk_doubles(n), nchp, p->rm_stride);
    LAUNCH_OK();
    // evaluation rows -> packed tiles, shifted past the special-parameter slots
    DevBuf bex, scratch;
    HIPDRT_CHECK(bex.alloc((size_t)nex * nchp * 256 * sizeof(double)));
    launch_pack_rows(st, neval, ncol, col_offset, rows_dev, ncol, nex, bex.d(), nchp);
    LAUNCH_OK();
    const int chunk = B < 256 ? B : 256;
    const size_t lsz = dist_var_scratch_doubles(n, nex);
    HIPDRT_CHECK(scratch.alloc((size_t)chunk * lsz * sizeof(double)));
    HIPDRT_CHECK(dout.alloc((size_t)B * nex * 16 * sizeof(double)));
    HIPDRT_CHECK(dstat.alloc((size_t)B * sizeof(int)));
    for (int b0 = 0; b0 < B; b0 += chunk) {
        const int nb = (B - b0) < chunk ? (B - b0) : chunk;
        TRY(launch_dist_var(st, nb, n, p->Ppk.d() + (size_t)b0 * qp_ppk_doubles(n), (long long)qp_ppk_doubles(n), bex.d(),
                            nex, scratch.d(), (long long)lsz, dout.d() + (size_t)b0 * nex * 16, (long long)nex * 16,
                            dstat.i() + b0));
    }
    HIPDRT_CHECK(hipStreamSynchronize(st));      // bex and scratch are released on return
    return HIPDRT_OK;
}

// out[b][i] = rows_i' P_b^-1 rows_i * cs_b^2 for the fitted batch, host rows in, host results out
static int plan_quadratic_forms(hipdrt_plan* p, const double* basis_eval, int neval, int ncol, int col_offset, double* out,
                                int* status) {
    HIPDRT_REQUIRE(p->B > 0, "no fitted batch in the plan");
    HIPDRT_REQUIRE(neval >= 1, "neval >= 1");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const int B = p->B, nex = (neval + 15) / 16;
    DevBuf dbe, dout, dstat;
    TRY(upload(dbe, basis_eval, (size_t)neval * ncol * sizeof(double), st));
    TRY(plan_quadratic_forms_dev(p, live_source(p), dbe.d(), neval, ncol, col_offset, dout, dstat));
    std::vector<double> hv((size_t)B * nex * 16), cs(B);
    std::vector<int> hs(B);
    HIPDRT_CHECK(hipMemcpyAsync(hv.data(), dout.p, hv.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(cs.data(), p->coef_scale.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(hs.data(), dstat.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    // estimate_param_cov scales the inverse by coefficient_scale^2 (drt1d.py:4133)
    for (int b = 0; b < B; ++b) {
        const double c2 = cs[b] * cs[b];
        for (int i = 0; i < neval; ++i) out[(size_t)b * neval + i] = hv[((size_t)b * nex) * 16 + i] * c2;
        if (status) status[b] = hs[b];
    }
    return HIPDRT_OK;
}

// out[neval][neval] = rows P_b^-1 rows' * cs_b^2 for ONE fitted spectrum: the variance kernel leaves Y = rows L^-T behind the
// factor (one more panel of the same factorisation), rows_outer_kernel forms Y Y'
static int plan_full_cov(hipdrt_plan* p, int b, const double* rows, int neval, int ncol, int col_offset, double* out, int* status) {
    HIPDRT_REQUIRE(p->B > 0, "no fitted batch in the plan");
    HIPDRT_REQUIRE(b >= 0 && b < p->B, "spectrum index out of range");
    HIPDRT_REQUIRE(neval >= 1, "neval >= 1");
    HIPDRT_REQUIRE(p->n <= 4096, "posterior covariance: n <= 4096");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const int n = p->n, m = p->m;
    const int nex = (neval + 15) / 16, nchp = qp_nchp(n), nch = round_up(n, 32) / 16;
    // final P of this spectrum, packed tiles, into its own slot of Ppk
    const FinalP f = plan_final_p(p, b, live_source(p));
    double* ppk = p->Ppk.d() + (size_t)b * qp_ppk_doubles(n);
    launch_gram_l2(st, 1, m, n, p->rm.d() + (size_t)b * p->rm_stride, p->ldrm, f.w, f.g, nullptr, p->ldp, 0, nullptr, ppk, 0,
                   nchp, 0);
    LAUNCH_OK();
    DevBuf dbe, bex, scratch, dvar, dstat, dcov;
    TRY(upload(dbe, rows, (size_t)neval * ncol * sizeof(double), st));
    HIPDRT_CHECK(bex.alloc((size_t)nex * nchp * 256 * sizeof(double)));
    launch_pack_rows(st, neval, ncol, col_offset, dbe.d(), ncol, nex, bex.d(), nchp);
    LAUNCH_OK();
    HIPDRT_CHECK(scratch.alloc(dist_var_scratch_doubles(n, nex) * sizeof(double)));
    HIPDRT_CHECK(dvar.alloc((size_t)nex * 16 * sizeof(double)));
    HIPDRT_CHECK(dstat.alloc(sizeof(int)));
    HIPDRT_CHECK(dcov.alloc((size_t)neval * neval * sizeof(double)));
    TRY(launch_dist_var(st, 1, n, ppk, 0, bex.d(), nex, scratch.d(), 0, dvar.d(), 0, dstat.i()));
    double cs = 1.0;
    int hs = 0;
    HIPDRT_CHECK(hipMemcpyAsync(&cs, p->coef_scale.d() + b, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(&hs, dstat.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    if (status) *status = hs;
    if (hs != 0) {                               // P not positive definite (np.linalg.inv would still return something; the
        for (size_t i = 0; i < (size_t)neval * neval; ++i) out[i] = __builtin_nan("");      // reference warns and returns None)
        return HIPDRT_OK;
    }
    // Y = rows L^-T sits in tile rows nch .. nch + nex - 1 of the scratch; only the first ceil(n / 16) tile columns are non-zero
    launch_rows_outer(st, scratch.d() + (size_t)nch * nch * 256, nch, nch, nex, neval, cs * cs, dcov.d(), neval);
    LAUNCH_OK();
    HIPDRT_CHECK(hipMemcpyAsync(out, dcov.p, (size_t)neval * neval * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
}

int hipdrt_plan_distribution_cov(hipdrt_plan* p, int b, const double* basis_eval, int neval, double* out, int* status) try {
    HIPDRT_REQUIRE(p && basis_eval && out, "NULL pointer");
    return plan_full_cov(p, b, basis_eval, neval, p->ntau, p->ns, out, status);
} HIPDRT_CATCH

int hipdrt_plan_param_cov(hipdrt_plan* p, int b, double* out, int* status) try {
    HIPDRT_REQUIRE(p && out, "NULL pointer");
    const int n = p->n;
    std::vector<double> eye((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) eye[(size_t)i * n + i] = 1.0;
    return plan_full_cov(p, b, eye.data(), n, n, 0, out, status);
} HIPDRT_CATCH

int hipdrt_plan_distribution_var(hipdrt_plan* p, const double* basis_eval, int neval, double* out, int* status) try {
    HIPDRT_REQUIRE(p && basis_eval && out, "NULL pointer");
    return plan_quadratic_forms(p, basis_eval, neval, p->ntau, p->ns, out, status);
} HIPDRT_CATCH

int hipdrt_plan_param_var(hipdrt_plan* p, double* out, int* status) try {
    HIPDRT_REQUIRE(p && out, "NULL pointer");
    const int n = p->n;
    std::vector<double> eye((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) eye[(size_t)i * n + i] = 1.0;
    return plan_quadratic_forms(p, eye.data(), n, n, 0, out, status);
} HIPDRT_CATCH

// ---- Kramers-Kronig screening (csrc/kk.hip) ---------------------------------------------------------------------------------
void hipdrt_default_kk_opts(hipdrt_kk_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->n_outlier_iter = 2; o->p_thresh = 1e-4; o->n_sigma = -1.0; o->std_sample_fraction = 0.6;
    o->n_std = 0.8416212335729143; o->max_num_outliers = 2; o->outlier_weight = 1e-10;
}

int hipdrt_plan_kk_screen(hipdrt_plan* p, const hipdrt_kk_opts* opts, int set_row_factors, double* z_hat_re, double* z_hat_im,
                          double* err_re, double* err_im, double* std_out, int* outlier_mask, double* f_lim, int* i_lim,
                          int* status) try {
    HIPDRT_REQUIRE(p, "plan is NULL");
    HIPDRT_REQUIRE(p->B >= 1 && p->prepped, "no fitted batch in the plan");
    // every check comes before the first launch and the first change of the plan
    HIPDRT_REQUIRE(!p->prepared, "the KK screen is built for plain EIS plans (hipdrt_plan_create)");
    HIPDRT_REQUIRE(p->nf >= 1 && p->m == 2 * p->nf, "the KK screen needs EIS-only data (m = 2 nf)");
    HIPDRT_REQUIRE(p->freq_order != 0, "the KK screen needs a strictly ascending or descending frequency grid");
    hipdrt_kk_opts o;
    if (opts) o = *opts; else hipdrt_default_kk_opts(&o);
    TRY(kk_check_opts(o));
    HIPDRT_REQUIRE(kk_lds_bytes(p->nf, p->n, 1) <= 160 * 1024 - 256, "KK screen: nf and n too large for one workgroup's LDS");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const int B = p->B, nf = p->nf, m = p->m;
    KkArgs a{};
    a.nf = nf; a.desc = p->freq_order > 0 ? 1 : 0; a.freq = p->freq.d(); a.o = o;
    KkOut out;
    TRY(out.alloc(a, B, nf, z_hat_re, z_hat_im, err_re, err_im, std_out, outlier_mask, f_lim, i_lim, status));
    if (set_row_factors) {
        const size_t need = (size_t)p->capacity * m * sizeof(double);
        if (p->wrow.bytes < need || !p->wrow_batched) {
            // (rows past the staged batch are never read by a fit of this batch; ones all the same)
            std::vector<double> ones((size_t)p->capacity * m, 1.0);
            TRY(upload(p->wrow, ones.data(), need, st));
            HIPDRT_CHECK(hipStreamSynchronize(st));
        }
        if (!p->w_eff.p) HIPDRT_CHECK(p->w_eff.alloc(need));
        a.wrow = p->wrow.d();
    }
    const FitState fs = p->state();
    TRY(launch_kk(st, &fs, a, B));
    LAUNCH_OK();
    if (set_row_factors) { p->weight_factor = 1.0; p->wrow_batched = 1; p->wrow_late = 1; }
    TRY(KkOut::back(z_hat_re, out.zr, st)); TRY(KkOut::back(z_hat_im, out.zi, st));
    TRY(KkOut::back(err_re, out.er, st)); TRY(KkOut::back(err_im, out.ei, st));
    TRY(KkOut::back(std_out, out.sd, st)); TRY(KkOut::back(outlier_mask, out.mask, st));
    TRY(KkOut::back(f_lim, out.flim, st)); TRY(KkOut::back(i_lim, out.ilim, st)); TRY(KkOut::back(status, out.status, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

// ---- model evaluation for the fitted batch (csrc/predict.hip) ----------------------------------------------------------------
int hipdrt_plan_set_tau_basis(hipdrt_plan* p, const double* ln_basis_tau, int nb, double epsilon) try {
    HIPDRT_REQUIRE(p && ln_basis_tau, "NULL pointer");
    HIPDRT_REQUIRE(p->prepared, "a plan made by hipdrt_plan_create holds its tau basis already");
    const int width = p->n - p->ns;
    HIPDRT_REQUIRE(nb >= 1 && (width == nb || width == 2 * nb), "the DRT block must hold one or two copies of the basis");
    HIPDRT_REQUIRE(epsilon > 0.0 && std::isfinite(epsilon), "epsilon > 0");
    TRY(enter(p->ctx));
    TRY(upload(p->basis_ln_tau, ln_basis_tau, (size_t)nb * sizeof(double), p->ctx->stream));
    HIPDRT_CHECK(hipStreamSynchronize(p->ctx->stream));
    p->basis_nb = nb; p->basis_eps = epsilon;
    return HIPDRT_OK;
} HIPDRT_CATCH

// kernel time of the last prediction on a context (hipdrt_debug_last_predict_ms): HIP events around the launches
struct PredictTimer {
    hipdrt_ctx* ctx; hipStream_t st; hipEvent_t e[3] = {nullptr, nullptr, nullptr}; int n = 0;
    PredictTimer(hipdrt_ctx* c, hipStream_t s) : ctx(c), st(s) { mark(); }
    void mark() { if (n < 3 && hipEventCreate(&e[n]) == hipSuccess) { (void)hipEventRecord(e[n], st); ++n; } }
    // (destroyed after the stream has been synchronised) [0] up to the second mark, [1] up to the last one
    ~PredictTimer() {
        float a = 0.f, b = 0.f;
        if (n >= 2 && hipEventElapsedTime(&a, e[0], e[1]) == hipSuccess && hipEventElapsedTime(&b, e[0], e[n - 1]) == hipSuccess) {
            ctx->predict_ms[0] = a; ctx->predict_ms[1] = b;
        }
        for (int i = 0; i < n; ++i) (void)hipEventDestroy(e[i]);
        (void)hipGetLastError();
    }
};

// the tau basis a prediction evaluates: the plan's own grid, or what hipdrt_plan_set_tau_basis gave a prepared plan
struct PredictBasis { const double* ln_tau; int nb, copies; double eps; };
static int predict_basis(const hipdrt_plan* p, PredictBasis& pb) {
    HIPDRT_REQUIRE(p->B >= 1 && p->prepped, "no fitted batch in the plan");
    if (p->prepared) {
        HIPDRT_REQUIRE(p->basis_nb > 0, "a prepared plan needs hipdrt_plan_set_tau_basis before a DRT prediction");
        pb = {p->basis_ln_tau.d(), p->basis_nb, (p->n - p->ns) / p->basis_nb, p->basis_eps};
    } else {
        pb = {p->ln_tau.d(), p->ntau, 1, p->eps};
    }
    return HIPDRT_OK;
}

// What a DRT prediction leaves on the device (hipdrt_plan_predict_drt, hipdrt_plan_find_peaks): for every order asked for the
// signed evaluation rows and the mean rows of the batch, the normalisation scalars, and (want_var) e' inv(P_b) e of all rows from
// one factorisation per spectrum, not yet scaled.
struct DrtRows {
    DevBuf dE, dsum, dabs, dnorm, dscale, dcs, dmu, dvar, dvstat;      // dE and dmu are allocated by the caller
    const double* scale = nullptr;       // [B] the factor the mean rows carry
    const double* cs = nullptr;          // [B] the coefficient scale behind it (times row_scale)
    const double* norm = nullptr;        // [B] R_p, or null without normalisation
    int neval = 0, B = 0, norders = 0;
    double* mu(int k) const { return dmu.d() + (size_t)k * B * neval; }                 // [B][neval] of orders[k]
    const double* var(int k) const { return dvar.d() + (size_t)k * neval; }             // row stride ldv()
    long long ldv() const { return (long long)((norders * neval + 15) / 16) * 16; }
};
// orders[norders] (norders 1 or 2): rows k * neval .. of dE and slab k of dmu belong to orders[k].  dev: ln(tau_eval) on the
// device.  row_scale: host [B] or null.  The timer is marked once, after the mean rows.
// have_E: dE already holds the evaluation rows (a second call on the same grid, orders and sign).
static int plan_drt_rows_dev(hipdrt_plan* p, const PostSource& src, const PredictBasis& pb, int neval, const int* orders,
                             int norders, int sign, int normalize, const double* row_scale, bool want_var, hipStream_t st,
                             DevBuf& dev, DrtRows& R, PredictTimer& tm, bool have_E = false) {
    const int B = p->B, n = p->n, ns = p->ns, width = n - ns, nb = pb.nb;
    R.neval = neval; R.B = B; R.norders = norders;
    // E[neval][width]: the signed evaluation rows over the whole DRT block (+E | 0), (0 | -E) or (+E | -E)
    if (!have_E && pb.copies == 2 && sign != 0) HIPDRT_CHECK(hipMemsetAsync(R.dE.p, 0, R.dE.bytes, st));
    for (int k = 0; k < norders && !have_E; ++k) {
        double* E = R.dE.d() + (size_t)k * neval * width;
        if (sign != -1) TRY(func_eval_dev(st, pb.ln_tau, nb, dev.d(), neval, pb.eps, orders[k], 1.0, E, width));
        if (pb.copies == 2 && sign != 1) TRY(func_eval_dev(st, pb.ln_tau, nb, dev.d(), neval, pb.eps, orders[k], -1.0, E + nb, width));
    }
    R.cs = p->coef_scale.d();
    if (row_scale) {
        DevBuf drs;
        TRY(upload(drs, row_scale, (size_t)B * sizeof(double), st));
        HIPDRT_CHECK(R.dcs.alloc((size_t)B * sizeof(double)));
        launch_scale_mul(st, B, p->coef_scale.d(), drs.d(), R.dcs.d());
        LAUNCH_OK();
        HIPDRT_CHECK(hipStreamSynchronize(st));      // drs is released on return
        R.cs = R.dcs.d();
    }
    R.scale = R.cs;
    if (normalize) {
        HIPDRT_CHECK(R.dsum.alloc((size_t)B * sizeof(double))); HIPDRT_CHECK(R.dabs.alloc((size_t)B * sizeof(double)));
        HIPDRT_CHECK(R.dnorm.alloc((size_t)B * sizeof(double))); HIPDRT_CHECK(R.dscale.alloc((size_t)B * sizeof(double)));
        launch_drt_sums(st, B, src.x, n, ns, nb, pb.copies, sign, R.dsum.d(), R.dabs.d());
        launch_drt_scalars(st, B, R.dsum.d(), R.dabs.d(), R.cs, 1.7724538509055159 / pb.eps, 1, normalize == 2,
                           src.x, n, -1, nullptr, nullptr, nullptr, R.dnorm.d(), R.dscale.d());
        LAUNCH_OK();
        R.scale = R.dscale.d();
        R.norm = R.dnorm.d();
    }
    for (int k = 0; k < norders; ++k) {
        launch_apply_rows(st, B, width, src.x, n, ns, neval, R.dE.d() + (size_t)k * neval * width, width, R.scale,
                          src.fit_status, R.mu(k), neval);
        LAUNCH_OK();
    }
    tm.mark();
    // sigma^2 = diag(E inv(P) E') from the variance path, fed the evaluation rows where they are (both orders as one row block)
    if (want_var) TRY(plan_quadratic_forms_dev(p, src, R.dE.d(), norders * neval, width, ns, R.dvar, R.dvstat));
    return HIPDRT_OK;
}

int hipdrt_plan_predict_drt(hipdrt_plan* p, const double* ln_tau_eval, int neval, int order, int sign, int normalize, double s_lo,
                            double s_hi, double* mu, double* lo, double* hi, int* status) try {
    HIPDRT_REQUIRE(p && ln_tau_eval && mu, "NULL pointer");
    PredictBasis pb;
    TRY(predict_basis(p, pb));
    HIPDRT_REQUIRE(neval >= 1, "neval >= 1");
    HIPDRT_REQUIRE(order >= 0 && order <= 2, "order must be 0, 1 or 2");
    HIPDRT_REQUIRE(sign == 1 || (pb.copies == 2 && (sign == 0 || sign == -1)),
                   "sign must be 1, or 1, -1 or 0 when the DRT block holds a positive and a negative copy");
    HIPDRT_REQUIRE(normalize >= 0 && normalize <= 2, "normalize must be 0, 1 (by R_p) or 2 (by absolute R_p)");
    const bool band = lo || hi;
    HIPDRT_REQUIRE(!band || (std::isfinite(s_lo) && std::isfinite(s_hi)), "s_lo and s_hi must be finite");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const int B = p->B, width = p->n - p->ns;
    DevBuf dev, dlo, dhi;
    DrtRows R;
    TRY(upload(dev, ln_tau_eval, (size_t)neval * sizeof(double), st));
    HIPDRT_CHECK(R.dE.alloc((size_t)neval * width * sizeof(double)));
    HIPDRT_CHECK(R.dmu.alloc((size_t)B * neval * sizeof(double)));
    PredictTimer tm(p->ctx, st);
    TRY(plan_drt_rows_dev(p, live_source(p), pb, neval, &order, 1, sign, normalize, nullptr, band, st, dev, R, tm));
    std::vector<int> hs(B), hv;
    if (band) {
        if (lo) HIPDRT_CHECK(dlo.alloc((size_t)B * neval * sizeof(double)));
        if (hi) HIPDRT_CHECK(dhi.alloc((size_t)B * neval * sizeof(double)));
        launch_drt_band(st, B, neval, R.mu(0), R.dvar.d(), R.ldv(), p->coef_scale.d(), R.norm, s_lo, s_hi, R.dvstat.i(),
                        p->fit_status.i(), dlo.d(), dhi.d());
        LAUNCH_OK();
        tm.mark();
        if (lo) HIPDRT_CHECK(hipMemcpyAsync(lo, dlo.p, dlo.bytes, hipMemcpyDeviceToHost, st));
        if (hi) HIPDRT_CHECK(hipMemcpyAsync(hi, dhi.p, dhi.bytes, hipMemcpyDeviceToHost, st));
        hv.resize(B);
        HIPDRT_CHECK(hipMemcpyAsync(hv.data(), R.dvstat.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    }
    HIPDRT_CHECK(hipMemcpyAsync(mu, R.dmu.p, R.dmu.bytes, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(hs.data(), p->fit_status.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    if (status)
        for (int b = 0; b < B; ++b) status[b] = (hs[b] >= 0 && band && hv[b] != 0) ? HIPDRT_PREDICT_NOT_PD : hs[b];
    return HIPDRT_OK;
} HIPDRT_CATCH

// ---- peak finding for the fitted batch (csrc/peaks.hip) ------------------------------------------------------------------------
void hipdrt_peak_opts_default(hipdrt_peak_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->eval_sign = 1; o->search = 1; o->normalize = 1; o->method = 0;
    o->height = __builtin_nan(""); o->prominence = __builtin_nan("");
    o->prob_thresh = 0.25; o->num_peaks = 0; o->fxx_var_floor = 1e-5; o->ext_left = -1; o->ext_right = -1;
}

int hipdrt_plan_find_peaks(hipdrt_plan* p, const double* ln_tau_eval, int neval, const hipdrt_peak_opts* opts,
                           const double* row_scale, int* peak_sign, int* keep, double* heights, double* prominences, double* probs,
                           int* left_bases, int* right_bases, int* count, double* used_prominence, double* peak_prob,
                           double* curv_prob, int* status) try {
    HIPDRT_REQUIRE(p && ln_tau_eval, "NULL pointer");
    PredictBasis pb;
    TRY(predict_basis(p, pb));
    hipdrt_peak_opts o;
    if (opts) o = *opts; else hipdrt_peak_opts_default(&o);
    // every check comes before the first launch
    TRY(peak_check_opts(o, neval));
    const int sign = o.eval_sign, normalize = o.normalize;
    HIPDRT_REQUIRE(sign == 1 || (pb.copies == 2 && (sign == 0 || sign == -1)),
                   "eval_sign must be 1, or 1, -1 or 0 when the DRT block holds a positive and a negative copy");
    HIPDRT_REQUIRE(normalize >= 0 && normalize <= 2, "normalize must be 0, 1 (by R_p) or 2 (by absolute R_p)");
    HIPDRT_REQUIRE(!row_scale || normalize == 0, "row_scale goes with normalize = 0 (a ratio to the spectrum's own R_p carries no scale)");
    const int B = p->B, width = p->n - p->ns;
    if (row_scale) for (int b = 0; b < B; ++b) HIPDRT_REQUIRE(row_scale[b] > 0.0 && std::isfinite(row_scale[b]), "row_scale must be positive and finite");
    const bool need_f = o.search == 0 || o.method == 2, need_var = o.method >= 1;
    const int orders[2] = {2, 0}, norders = need_f ? 2 : 1;
    PeakArgs a{};
    a.neval = neval; a.o = o;
    HIPDRT_REQUIRE(peaks_lds_bytes(neval, o.method, need_f, o.num_peaks) <= 160 * 1024 - 256,
                   "find_peaks: neval too large for one workgroup's LDS");
    hipStream_t st; TRY(enter(p->ctx, &st));
    DevBuf dev;
    DrtRows R;
    TRY(upload(dev, ln_tau_eval, (size_t)neval * sizeof(double), st));
    HIPDRT_CHECK(R.dE.alloc((size_t)norders * neval * width * sizeof(double)));
    HIPDRT_CHECK(R.dmu.alloc((size_t)norders * B * neval * sizeof(double)));
    const size_t bn = (size_t)B * neval;
    DevBuf dsg, dkp, dht, dpr, dpb, dlb, drb, dct, dup, dpp, dcp;
    if (peak_sign) { HIPDRT_CHECK(dsg.alloc(bn * sizeof(int))); a.peak_sign = dsg.i(); }
    if (keep) { HIPDRT_CHECK(dkp.alloc(bn * sizeof(int))); a.keep = dkp.i(); }
    if (heights) { HIPDRT_CHECK(dht.alloc(bn * sizeof(double))); a.heights = dht.d(); }
    if (prominences) { HIPDRT_CHECK(dpr.alloc(bn * sizeof(double))); a.prominences = dpr.d(); }
    if (probs) { HIPDRT_CHECK(dpb.alloc(bn * sizeof(double))); a.probs = dpb.d(); }
    if (left_bases) { HIPDRT_CHECK(dlb.alloc(bn * sizeof(int))); a.left_bases = dlb.i(); }
    if (right_bases) { HIPDRT_CHECK(drb.alloc(bn * sizeof(int))); a.right_bases = drb.i(); }
    if (count) { HIPDRT_CHECK(dct.alloc((size_t)B * sizeof(int))); a.count = dct.i(); }
    if (used_prominence) { HIPDRT_CHECK(dup.alloc((size_t)B * sizeof(double))); a.used_prominence = dup.d(); }
    if (peak_prob && o.method == 2) { HIPDRT_CHECK(dpp.alloc(bn * sizeof(double))); a.peak_prob = dpp.d(); }
    if (curv_prob && o.method == 2) { HIPDRT_CHECK(dcp.alloc(bn * sizeof(double))); a.curv_prob = dcp.d(); }
    PredictTimer tm(p->ctx, st);
    TRY(plan_drt_rows_dev(p, live_source(p), pb, neval, orders, norders, sign, normalize, row_scale, need_var, st, dev, R, tm));
    a.fxx = R.mu(0);
    a.f = need_f ? R.mu(1) : nullptr;
    if (need_var) {
        a.var_fxx = R.var(0); a.var_f = o.method == 2 ? R.var(1) : nullptr; a.ldv = R.ldv();
        a.cs = R.cs; a.norm = R.norm; a.var_status = R.dvstat.i();
    }
    a.fit_status = p->fit_status.i();
    TRY(launch_peaks(st, a, B));
    LAUNCH_OK();
    tm.mark();
    // (KkOut::back: copy a device output to the host when both exist)
    TRY(KkOut::back(peak_sign, dsg, st)); TRY(KkOut::back(keep, dkp, st)); TRY(KkOut::back(heights, dht, st));
    TRY(KkOut::back(prominences, dpr, st)); TRY(KkOut::back(probs, dpb, st)); TRY(KkOut::back(left_bases, dlb, st));
    TRY(KkOut::back(right_bases, drb, st)); TRY(KkOut::back(count, dct, st)); TRY(KkOut::back(used_prominence, dup, st));
    TRY(KkOut::back(peak_prob, dpp, st)); TRY(KkOut::back(curv_prob, dcp, st));
    std::vector<int> hs(B), hv(B, 0);
    HIPDRT_CHECK(hipMemcpyAsync(hs.data(), p->fit_status.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    if (need_var) HIPDRT_CHECK(hipMemcpyAsync(hv.data(), R.dvstat.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    if (status)
        for (int b = 0; b < B; ++b) status[b] = (hs[b] >= 0 && need_var && hv[b] != 0) ? HIPDRT_PREDICT_NOT_PD : hs[b];
    return HIPDRT_OK;
} HIPDRT_CATCH

// ---- per-peak coefficients, distributions and resistances (csrc/peak_resolve.hip) ----------------------------------------------
void hipdrt_peak_resolve_opts_default(hipdrt_peak_resolve_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->sign = 1; o->max_peaks = 16; o->epsilon_factor = 1.25; o->max_epsilon = 1.25;
    o->min_epsilon = __builtin_nan(""); o->epsilon_uniform = __builtin_nan("");
}

int hipdrt_plan_resolve_peaks(hipdrt_plan* p, const hipdrt_peak_resolve_in* in, const hipdrt_peak_resolve_opts* opts,
                              hipdrt_peak_resolve_out* out) try {
    HIPDRT_REQUIRE(p && in && out && in->ln_tau_find, "NULL pointer");
    PredictBasis pb;
    TRY(predict_basis(p, pb));
    hipdrt_peak_resolve_opts o;
    if (opts) o = *opts; else hipdrt_peak_resolve_opts_default(&o);
    // every check comes before the first launch
    TRY(peak_resolve_check_opts(o));
    const int B = p->B, n = p->n, ns = p->ns, width = n - ns, nfind = in->nfind, mp = o.max_peaks;
    const bool want_out = out->r_peaks || out->peak_gammas;
    const int nout = want_out ? in->nout : 0;
    HIPDRT_REQUIRE(nfind >= 1, "nfind >= 1");
    HIPDRT_REQUIRE(!want_out || (in->ln_tau_out && in->nout >= 1), "r_peaks and peak_gammas need the output grid");
    HIPDRT_REQUIRE(o.sign == 1 || (pb.copies == 2 && (o.sign == 0 || o.sign == -1)),
                   "sign must be 1, or 1, -1 or 0 when the DRT block holds a positive and a negative copy");
    TRY(peak_resolve_check_source(in->source, in->peak_indices, B, mp, in->win_start, in->win_end, in->nwin, nfind));
    const double* row_scale = in->row_scale;
    if (row_scale) for (int b = 0; b < B; ++b) HIPDRT_REQUIRE(row_scale[b] > 0.0 && std::isfinite(row_scale[b]), "row_scale must be positive and finite");
    hipdrt_peak_opts po;
    if (in->peak_opts) po = *in->peak_opts; else hipdrt_peak_opts_default(&po);
    const bool find = in->source == HIPDRT_PEAKS_FROM_FIND;
    bool need_var = false;
    if (find) {
        TRY(peak_check_opts(po, nfind));
        HIPDRT_REQUIRE(po.eval_sign == o.sign, "peak_opts.eval_sign must equal opts.sign (estimate_peak_coef hands its sign to find_peaks)");
        HIPDRT_REQUIRE(po.method == 0 || po.method == 1, "peak_opts.method must be 0 (thresh) or 1 (prob)");
        HIPDRT_REQUIRE(po.normalize >= 0 && po.normalize <= 2, "normalize must be 0, 1 (by R_p) or 2 (by absolute R_p)");
        HIPDRT_REQUIRE(peaks_lds_bytes(nfind, po.method, 1, po.num_peaks) <= 160 * 1024 - 256,
                       "find_peaks: nfind too large for one workgroup's LDS");
        need_var = po.method >= 1;
    }
    {
        const size_t lds = peak_resolve_lds_bytes(nfind, pb.nb, nout, mp);
        if (lds > 160 * 1024 - 256) {
            set_error("invalid argument: resolve_peaks: " + std::to_string(lds) + " bytes of LDS needed (nfind, nb, nout, max_peaks), " +
                      std::to_string(160 * 1024 - 256) + " available");
            return HIPDRT_E_INVALID;
        }
    }
    hipStream_t st; TRY(enter(p->ctx, &st));
    const int orders[2] = {2, 0};
    const int normalize = find ? po.normalize : 0;
    DevBuf dev, dout_grid, dE0, dkeep, dmu2, didx, dws, dwe;
    DrtRows R;
    TRY(upload(dev, in->ln_tau_find, (size_t)nfind * sizeof(double), st));
    HIPDRT_CHECK(R.dE.alloc((size_t)2 * nfind * width * sizeof(double)));
    HIPDRT_CHECK(R.dmu.alloc((size_t)2 * B * nfind * sizeof(double)));
    PeakResolveArgs a{};
    a.nfind = nfind; a.nb = pb.nb; a.nout = nout; a.source = in->source; a.nwin = in->nwin; a.copies = pb.copies; a.o = o;
    if (in->source == HIPDRT_PEAKS_FROM_INDICES) { TRY(upload(didx, in->peak_indices, (size_t)B * mp * sizeof(int), st)); a.indices = didx.i(); }
    if (in->source == HIPDRT_PEAKS_FROM_WINDOWS) {
        TRY(upload(dws, in->win_start, (size_t)in->nwin * sizeof(int), st)); TRY(upload(dwe, in->win_end, (size_t)in->nwin * sizeof(int), st));
        a.win_start = dws.i(); a.win_end = dwe.i();
    }
    if (nout > 0) {
        TRY(upload(dout_grid, in->ln_tau_out, (size_t)nout * sizeof(double), st));
        HIPDRT_CHECK(dE0.alloc((size_t)nout * pb.nb * sizeof(double)));
    }
    const size_t bm = (size_t)B * mp;
    DevBuf dct, dpi, dti, del, der, drp, drc, dxp, dpg, dst;
    HIPDRT_CHECK(dct.alloc((size_t)B * sizeof(int))); a.count = dct.i();
    HIPDRT_CHECK(dst.alloc((size_t)B * sizeof(int))); a.status = dst.i();
    if (out->peak_index) { HIPDRT_CHECK(dpi.alloc(bm * sizeof(int))); a.peak_index = dpi.i(); }
    if (out->trough_index) { HIPDRT_CHECK(dti.alloc(bm * sizeof(int))); a.trough_index = dti.i(); }
    if (out->eps_l) { HIPDRT_CHECK(del.alloc(bm * sizeof(double))); a.eps_l = del.d(); }
    if (out->eps_r) { HIPDRT_CHECK(der.alloc(bm * sizeof(double))); a.eps_r = der.d(); }
    if (out->r_peaks) { HIPDRT_CHECK(drp.alloc(bm * sizeof(double))); a.r_peaks = drp.d(); }
    if (out->r_coef) { HIPDRT_CHECK(drc.alloc(bm * sizeof(double))); a.r_coef = drc.d(); }
    if (out->x_peaks) { HIPDRT_CHECK(dxp.alloc(bm * pb.nb * sizeof(double))); a.x_peaks = dxp.d(); }
    if (out->peak_gammas) { HIPDRT_CHECK(dpg.alloc(bm * nout * sizeof(double))); a.peak_gammas = dpg.d(); }
    PredictTimer tm(p->ctx, st);
    TRY(plan_drt_rows_dev(p, live_source(p), pb, nfind, orders, 2, o.sign, normalize, row_scale, need_var, st, dev, R, tm));
    a.fxx = R.mu(0); a.f = R.mu(1);
    if (find) {
        HIPDRT_CHECK(dkeep.alloc((size_t)B * nfind * sizeof(int)));
        PeakArgs pa{};
        pa.neval = nfind; pa.o = po; pa.fxx = R.mu(0); pa.f = R.mu(1); pa.keep = dkeep.i(); pa.fit_status = p->fit_status.i();
        if (need_var) {
            pa.var_fxx = R.var(0); pa.ldv = R.ldv(); pa.cs = R.cs; pa.norm = R.norm; pa.var_status = R.dvstat.i();
        }
        TRY(launch_peaks(st, pa, B));
        LAUNCH_OK();
        a.keep = dkeep.i();
        if (normalize) {
            // estimate_peak_coef evaluates f and fxx without normalisation whatever find_peaks used: the same evaluation rows
            // applied once more at the coefficient scale alone -- the bits of hipdrt_plan_predict_drt(normalize = 0)
            HIPDRT_CHECK(dmu2.alloc((size_t)2 * B * nfind * sizeof(double)));
            for (int k = 0; k < 2; ++k) {
                launch_apply_rows(st, B, width, p->x.d(), n, ns, nfind, R.dE.d() + (size_t)k * nfind * width, width, R.cs,
                                  p->fit_status.i(), dmu2.d() + (size_t)k * B * nfind, nfind);
                LAUNCH_OK();
            }
            a.fxx = dmu2.d(); a.f = dmu2.d() + (size_t)B * nfind;
        }
    }
    if (nout > 0) {
        TRY(func_eval_dev(st, pb.ln_tau, pb.nb, dout_grid.d(), nout, pb.eps, 0, 1.0, dE0.d(), pb.nb));
        a.E0 = dE0.d(); a.lto = dout_grid.d();
    }
    a.X = p->x.d(); a.ldx = n; a.col_offset = ns; a.cs = R.cs;
    a.lt = dev.d(); a.lb = pb.ln_tau; a.basis_area = 1.7724538509055159 / pb.eps;
    a.fit_status = p->fit_status.i();
    TRY(launch_peak_resolve(st, a, B));
    LAUNCH_OK();
    tm.mark();
    TRY(KkOut::back(out->count, dct, st)); TRY(KkOut::back(out->peak_index, dpi, st)); TRY(KkOut::back(out->trough_index, dti, st));
    TRY(KkOut::back(out->eps_l, del, st)); TRY(KkOut::back(out->eps_r, der, st)); TRY(KkOut::back(out->r_peaks, drp, st));
    TRY(KkOut::back(out->r_coef, drc, st)); TRY(KkOut::back(out->x_peaks, dxp, st)); TRY(KkOut::back(out->peak_gammas, dpg, st));
    std::vector<int> hs(B), hv(B, 0);
    HIPDRT_CHECK(hipMemcpyAsync(hs.data(), dst.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    if (need_var) HIPDRT_CHECK(hipMemcpyAsync(hv.data(), R.dvstat.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    bool unordered = false;
    for (int b = 0; b < B; ++b) {
        if (hs[b] >= 0 && need_var && hv[b] != 0) hs[b] = HIPDRT_PREDICT_NOT_PD;
        unordered = unordered || hs[b] == HIPDRT_PEAKS_UNORDERED;
        if (out->status) out->status[b] = hs[b];
    }
    if (unordered) {
        set_error("invalid argument: resolve_peaks: the window peaks of a spectrum are not strictly increasing (two windows chose "
                  "their shared border sample); see status");
        return HIPDRT_E_INVALID;
    }
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_integrate_drt(hipdrt_plan* p, const double* ln_tau_eval, int neval, int order, int sign, int normalize,
                              const double* row_scale, const int* win_start, const int* win_end, int nwin, double* out,
                              int* status) try {
    HIPDRT_REQUIRE(p && ln_tau_eval && win_start && win_end && out, "NULL pointer");
    PredictBasis pb;
    TRY(predict_basis(p, pb));
    HIPDRT_REQUIRE(neval >= 1, "neval >= 1");
    HIPDRT_REQUIRE(order >= 0 && order <= 2, "order must be 0, 1 or 2");
    HIPDRT_REQUIRE(sign == 1 || (pb.copies == 2 && (sign == 0 || sign == -1)),
                   "sign must be 1, or 1, -1 or 0 when the DRT block holds a positive and a negative copy");
    HIPDRT_REQUIRE(normalize >= 0 && normalize <= 2, "normalize must be 0, 1 (by R_p) or 2 (by absolute R_p)");
    HIPDRT_REQUIRE(!row_scale || normalize == 0, "row_scale goes with normalize = 0 (a ratio to the spectrum's own R_p carries no scale)");
    HIPDRT_REQUIRE(nwin >= 1 && nwin <= 65535, "1 <= nwin <= 65535");
    TRY(peak_resolve_check_source(2, nullptr, 0, nwin, win_start, win_end, nwin, neval));
    const int B = p->B, width = p->n - p->ns;
    if (row_scale) for (int b = 0; b < B; ++b) HIPDRT_REQUIRE(row_scale[b] > 0.0 && std::isfinite(row_scale[b]), "row_scale must be positive and finite");
    hipStream_t st; TRY(enter(p->ctx, &st));
    DevBuf dev, dws, dwe, dres;
    DrtRows R;
    TRY(upload(dev, ln_tau_eval, (size_t)neval * sizeof(double), st));
    TRY(upload(dws, win_start, (size_t)nwin * sizeof(int), st)); TRY(upload(dwe, win_end, (size_t)nwin * sizeof(int), st));
    HIPDRT_CHECK(R.dE.alloc((size_t)neval * width * sizeof(double)));
    HIPDRT_CHECK(R.dmu.alloc((size_t)B * neval * sizeof(double)));
    HIPDRT_CHECK(dres.alloc((size_t)B * nwin * sizeof(double)));
    PredictTimer tm(p->ctx, st);
    TRY(plan_drt_rows_dev(p, live_source(p), pb, neval, &order, 1, sign, normalize, row_scale, false, st, dev, R, tm));
    launch_window_trapz(st, B, neval, nwin, R.mu(0), dev.d(), dws.i(), dwe.i(), dres.d());
    LAUNCH_OK();
    tm.mark();
    HIPDRT_CHECK(hipMemcpyAsync(out, dres.p, (size_t)B * nwin * sizeof(double), hipMemcpyDeviceToHost, st));
    if (status) HIPDRT_CHECK(hipMemcpyAsync(status, p->fit_status.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_predict_z(hipdrt_plan* p, const double* freq, int nf, int include_mask, double* z_re, double* z_im,
                          int* status) try {
    HIPDRT_REQUIRE(p && freq && z_re && z_im, "NULL pointer");
    if (p->prepared) {
        set_error("not supported: impedance prediction is built for plain EIS plans (hipdrt_plan_create); a prepared plan holds "
                  "neither lookup tables nor a tau grid");
        return HIPDRT_E_UNSUPPORTED;
    }
    HIPDRT_REQUIRE(p->B >= 1 && p->prepped, "no fitted batch in the plan");
    HIPDRT_REQUIRE(nf >= 1, "nf >= 1");
    HIPDRT_REQUIRE(include_mask >= 0 && include_mask <= 7, "include_mask: bit 0 DRT, bit 1 ohmic, bit 2 inductance");
    for (int i = 0; i < nf; ++i) HIPDRT_REQUIRE(freq[i] > 0.0 && std::isfinite(freq[i]), "frequencies must be positive and finite");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const int B = p->B, n = p->n, ntau = p->ntau;
    DevBuf dfreq, dA, cr, dy, dzr, dzi;
    TRY(upload(dfreq, freq, (size_t)nf * sizeof(double), st));
    HIPDRT_CHECK(dzr.alloc((size_t)B * nf * sizeof(double))); HIPDRT_CHECK(dzi.alloc((size_t)B * nf * sizeof(double)));
    if (include_mask & 1) {
        HIPDRT_CHECK(dA.alloc((size_t)2 * nf * ntau * sizeof(double)));
        HIPDRT_CHECK(cr.alloc(((size_t)nf + 2 * (size_t)(nf + ntau)) * sizeof(double)));
        HIPDRT_CHECK(dy.alloc((size_t)B * 2 * nf * sizeof(double)));
    }
    PredictTimer tm(p->ctx, st);
    if (include_mask & 1) {
        // [A'; A''] at the requested frequencies from the plan's own tables, tau grid and integration mode (no Toeplitz shortcut:
        // every entry is evaluated where it stands), then both parts as the two row blocks of one product
        launch_impedance_matrix(st, 1, 0, dfreq.d(), nf, p->tau.d(), ntau, p->mode, 0, p->eps, p->ngrid, p->lut6.d(), p->ny,
                                dA.d(), dA.d() + (size_t)nf * ntau, cr.d());
        LAUNCH_OK();
        launch_apply_rows(st, B, ntau, p->x.d(), n, p->ns, 2 * nf, dA.d(), ntau, p->coef_scale.d(), nullptr, dy.d(), 2 * nf);
        LAUNCH_OK();
    }
    launch_z_assemble(st, B, nf, dy.d(), p->x.d(), n, p->idx_rinf, p->idx_induc, p->coef_scale.d(), p->opts.inductance_scale,
                      dfreq.d(), include_mask, p->fit_status.i(), dzr.d(), dzi.d());
    LAUNCH_OK();
    tm.mark();
    HIPDRT_CHECK(hipMemcpyAsync(z_re, dzr.p, dzr.bytes, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(z_im, dzi.p, dzi.bytes, hipMemcpyDeviceToHost, st));
    if (status) HIPDRT_CHECK(hipMemcpyAsync(status, p->fit_status.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_predict_resistances(hipdrt_plan* p, double* r_p, double* r_inf, double* r_tot, int abs_norm) try {
    HIPDRT_REQUIRE(p, "plan is NULL");
    PredictBasis pb;
    TRY(predict_basis(p, pb));
    if (p->prepared && (r_inf || r_tot)) {
        set_error("not supported: a prepared plan does not know which special parameter is R_inf (pass NULL for r_inf and r_tot)");
        return HIPDRT_E_UNSUPPORTED;
    }
    hipStream_t st; TRY(enter(p->ctx, &st));
    const int B = p->B, n = p->n;
    DevBuf dsum, dabs, drp, dri, drt;
    for (DevBuf* d : {&dsum, &dabs, &drp, &dri, &drt}) HIPDRT_CHECK(d->alloc((size_t)B * sizeof(double)));
    // predict_r_p's default sign: the net distribution of a two-copy block, else the block itself
    launch_drt_sums(st, B, p->x.d(), n, p->ns, pb.nb, pb.copies, pb.copies == 2 ? 0 : 1, dsum.d(), dabs.d());
    launch_drt_scalars(st, B, dsum.d(), dabs.d(), p->coef_scale.d(), 1.7724538509055159 / pb.eps, 0, abs_norm != 0, p->x.d(), n,
                       p->idx_rinf, drp.d(), dri.d(), drt.d(), nullptr, nullptr);
    LAUNCH_OK();
    if (r_p) HIPDRT_CHECK(hipMemcpyAsync(r_p, drp.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
    if (r_inf) HIPDRT_CHECK(hipMemcpyAsync(r_inf, dri.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
    if (r_tot) HIPDRT_CHECK(hipMemcpyAsync(r_tot, drt.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

// ---- the probability function of relaxation times of a PFRT fit (csrc/pfrt.hip) -------------------------------------------------
void hipdrt_pfrt_opts_default(hipdrt_pfrt_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->eval_sign = 1; o->search = 1; o->height = 1e-3; o->prominence = 5e-3;
    o->prior_mu = -4.0; o->prior_sigma = 0.5; o->n_eff_factor = 0.5; o->fxx_var_floor = 1e-5; o->ext_left = -1; o->ext_right = -1;
    o->smooth = 1; o->smooth_order = 2.0; o->smooth_epsilon = 5.0; o->integrate = 0; o->integrate_threshold = 1e-6; o->normalize = 1;
}

// the raw weights estimate_weights(x, rv, vmm, rm) of one recorded step into dw [B][m] (the sums go to scratch)
static int step_weights(hipdrt_plan* p, int step, hipStream_t st, DevBuf& dw, DevBuf& dscratch) {
    const size_t B = (size_t)p->B;
    if (dw.bytes < B * p->m * sizeof(double)) HIPDRT_CHECK(dw.alloc(B * p->m * sizeof(double)));
    if (dscratch.bytes < 2 * B * sizeof(double)) HIPDRT_CHECK(dscratch.alloc(2 * B * sizeof(double)));
    FitState fs = p->state();
    fs.x = p->pf_x.d() + p->pf_layout().x(step);
    TRY(launch_llh(st, fs, p->B, dscratch.d(), dscratch.d() + B, 0, 1.0, dw.d()));
    LAUNCH_OK();
    return HIPDRT_OK;
}

int hipdrt_plan_get_step_p_matrix(hipdrt_plan* p, int step, int b, double* out) try {
    HIPDRT_REQUIRE(p && out, "NULL pointer");
    HIPDRT_REQUIRE(p->B >= 1 && p->prepped, "no fitted batch in the plan");
    HIPDRT_REQUIRE(step >= 0 && step < p->pf_steps, "step out of range of the recorded PFRT steps");
    HIPDRT_REQUIRE(b >= 0 && b < p->B, "spectrum index out of range");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const int n = p->n, m = p->m;
    DevBuf dw, dscratch;
    TRY(step_weights(p, step, st, dw, dscratch));
    const FinalP f = plan_final_p(p, b, step_source(p, step, dw.d(), nullptr));
    launch_gram_l2(st, 1, m, n, p->rm.d() + (size_t)b * p->rm_stride, p->ldrm, f.w, f.g, p->Ptmp.d(), p->ldp, 0, nullptr);
    LAUNCH_OK();
    return copy_strided(out, p->Ptmp.d(), n, n, p->ldp, st);      // (synchronises: dw may go)
} HIPDRT_CATCH

int hipdrt_plan_pfrt_get_step(hipdrt_plan* p, int step, double* x, double* rho, double* s, double* rss, double* sum_log_w,
                              int* status) try {
    HIPDRT_REQUIRE(p, "plan is NULL");
    HIPDRT_REQUIRE(step >= 0 && step < p->pf_steps, "step out of range of the recorded PFRT steps");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const PfrtStoreLayout L = p->pf_layout();
    const size_t B = (size_t)p->B, n = (size_t)p->n, D = sizeof(double);
    if (x) HIPDRT_CHECK(hipMemcpyAsync(x, p->pf_x.d() + L.x(step), B * n * D, hipMemcpyDeviceToHost, st));
    if (rho) HIPDRT_CHECK(hipMemcpyAsync(rho, p->pf_rho.d() + L.rho(step), B * 3 * D, hipMemcpyDeviceToHost, st));
    if (s) HIPDRT_CHECK(hipMemcpyAsync(s, p->pf_s.d() + L.s(step), B * 3 * n * D, hipMemcpyDeviceToHost, st));
    if (rss) HIPDRT_CHECK(hipMemcpyAsync(rss, p->pf_rss.d() + L.scalar(step), B * D, hipMemcpyDeviceToHost, st));
    if (sum_log_w) HIPDRT_CHECK(hipMemcpyAsync(sum_log_w, p->pf_slw.d() + L.scalar(step), B * D, hipMemcpyDeviceToHost, st));
    if (status) HIPDRT_CHECK(hipMemcpyAsync(status, p->pf_status.i() + L.scalar(step), B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_predict_pfrt(hipdrt_plan* p, const double* factors, const double* ln_tau_pfrt, int neval_pfrt,
                             const double* ln_tau_out, int neval_out, const hipdrt_pfrt_opts* opts, double* pfrt, double* raw_pfrt,
                             double* step_pfrt, double* post_prob, int* status) try {
    HIPDRT_REQUIRE(p && factors && ln_tau_pfrt, "NULL pointer");
    if (p->prepared) {
        set_error("not supported: predict_pfrt is built for plain EIS plans (hipdrt_plan_create); a prepared plan records its steps "
                  "and gives their P matrices only");
        return HIPDRT_E_UNSUPPORTED;
    }
    PredictBasis pb;
    TRY(predict_basis(p, pb));
    hipdrt_pfrt_opts o;
    if (opts) o = *opts; else hipdrt_pfrt_opts_default(&o);
    const int S = p->pf_steps, B = p->B, np = neval_pfrt, nout = neval_out, width = p->n - p->ns;
    // every check comes before the first launch
    HIPDRT_REQUIRE(S >= 1, "no recorded PFRT steps in the plan (hipdrt_plan_pfrt_begin / _record around the fit's steps)");
    TRY(pfrt_check(o, S, np, nout));
    HIPDRT_REQUIRE(!o.smooth || ln_tau_out, "smoothing needs the output grid");
    HIPDRT_REQUIRE(o.eval_sign == 1, "eval_sign must be 1 (the DRT block of a plain EIS plan holds one copy of the basis)");
    for (int i = 0; i < S; ++i) HIPDRT_REQUIRE(factors[i] > 0.0 && std::isfinite(factors[i]), "factors must be positive and finite");
    hipdrt_peak_opts po;
    hipdrt_peak_opts_default(&po);
    po.eval_sign = 1; po.search = o.search; po.normalize = 1; po.method = 0; po.height = o.height; po.prominence = o.prominence;
    TRY(peak_check_opts(po, np));
    HIPDRT_REQUIRE(peaks_lds_bytes(np, 0, 1, 0) <= 160 * 1024 - 256, "predict_pfrt: neval_pfrt too large for one workgroup's LDS");
    hipStream_t st; TRY(enter(p->ctx, &st));

    // a spectrum whose fit failed in any step is dead in every step
    std::vector<int> hs((size_t)S * B), comb(B, 0), hbad(B, 0);
    for (int i = 0; i < S; ++i)
        HIPDRT_CHECK(hipMemcpyAsync(hs.data() + (size_t)i * B, p->pf_status.i() + p->pf_layout().scalar(i), (size_t)B * sizeof(int),
                                    hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < S; ++i) {
            const int v = hs[(size_t)i * B + b];
            if (comb[b] >= 0 && (v < 0 || v > comb[b])) comb[b] = v;
        }
    std::vector<double> lnf(S);
    for (int i = 0; i < S; ++i) lnf[i] = std::log(factors[i]);

    const size_t bn = (size_t)B * np;
    DevBuf dev, dout_grid, dfs, dbad, dlnf, dw, dscratch, dnorm0, dsg, dht, dpr, dstep, dpf, draw, dpost;
    DevBuf dE;
    TRY(upload(dev, ln_tau_pfrt, (size_t)np * sizeof(double), st));
    if (o.smooth) TRY(upload(dout_grid, ln_tau_out, (size_t)nout * sizeof(double), st));
    TRY(upload(dfs, comb.data(), (size_t)B * sizeof(int), st));
    TRY(upload(dlnf, lnf.data(), (size_t)S * sizeof(double), st));
    HIPDRT_CHECK(dbad.alloc((size_t)B * sizeof(int)));
    HIPDRT_CHECK(hipMemsetAsync(dbad.p, 0, (size_t)B * sizeof(int), st));
    HIPDRT_CHECK(dnorm0.alloc((size_t)B * sizeof(double)));
    HIPDRT_CHECK(dsg.alloc(bn * sizeof(int))); HIPDRT_CHECK(dht.alloc(bn * sizeof(double))); HIPDRT_CHECK(dpr.alloc(bn * sizeof(double)));
    HIPDRT_CHECK(dstep.alloc((size_t)S * bn * sizeof(double)));
    HIPDRT_CHECK(dE.alloc((size_t)2 * np * width * sizeof(double)));
    HIPDRT_CHECK(hipStreamSynchronize(st));          // (the host vectors above may go out of use)
    const int orders[2] = {2, 0};
    PredictTimer tm(p->ctx, st);
    for (int i = 0; i < S; ++i) {
        // step P = calculate_pq with the step's s / rho and the raw re-estimated weights (drt1d.py:2611-2632)
        TRY(step_weights(p, i, st, dw, dscratch));
        const PostSource src = step_source(p, i, dw.d(), dfs.i());
        // f and fxx normalised by the R_p of the step's own x; sigma^2 of both orders from one factorisation of the step P
        DrtRows R;
        R.dE.alias(dE, 0, dE.bytes);
        HIPDRT_CHECK(R.dmu.alloc((size_t)2 * bn * sizeof(double)));
        TRY(plan_drt_rows_dev(p, src, pb, np, orders, 2, 1, 1, nullptr, true, st, dev, R, tm, i > 0));
        // ... but every step's variances are divided by the squared R_p of the FIRST step (estimate_distribution_cov takes
        // get_drt_norm() of fit_parameters, which the warm restarts never update: drt1d.py:3081)
        if (i == 0) HIPDRT_CHECK(hipMemcpyAsync(dnorm0.p, R.dnorm.p, (size_t)B * sizeof(double), hipMemcpyDeviceToDevice, st));
        PeakArgs pa{};
        pa.neval = np; pa.o = po; pa.fxx = R.mu(0); pa.f = R.mu(1); pa.fit_status = dfs.i();
        pa.peak_sign = dsg.i(); pa.heights = dht.d(); pa.prominences = dpr.d();
        TRY(launch_peaks(st, pa, B));
        LAUNCH_OK();
        PfrtStepArgs sa{};
        sa.neval = np; sa.floor = o.fxx_var_floor; sa.ext_left = o.ext_left; sa.ext_right = o.ext_right;
        sa.peak_sign = dsg.i(); sa.heights = dht.d(); sa.prominences = dpr.d(); sa.f = R.mu(1);
        sa.var_fxx = R.var(0); sa.var_f = R.var(1); sa.ldv = R.ldv(); sa.cs = R.cs; sa.norm = dnorm0.d();
        sa.fit_status = dfs.i(); sa.var_status = R.dvstat.i(); sa.out = dstep.d() + (size_t)i * bn; sa.bad = dbad.i();
        TRY(launch_pfrt_step(st, sa, B));
        LAUNCH_OK();
        HIPDRT_CHECK(hipStreamSynchronize(st));      // R's buffers are released at the end of the iteration
    }
    PfrtCombineArgs ca{};
    ca.S = S; ca.np = np; ca.nout = nout; ca.ld_step = (long long)bn; ca.ld_sum = p->capacity;
    ca.step_pfrt = dstep.d(); ca.rss = p->pf_rss.d(); ca.slw = p->pf_slw.d(); ca.ln_factors = dlnf.d();
    pfrt_llh_consts(p->m, &ca.c, &ca.alpha_n, &ca.beta_0);
    ca.prior_mu = o.prior_mu; ca.prior_sigma = o.prior_sigma; ca.n_eff = o.n_eff_factor;
    ca.smooth = o.smooth != 0; ca.smooth_order = o.smooth_order; ca.smooth_eps = o.smooth_epsilon;
    ca.integrate = o.integrate != 0; ca.thr = o.integrate_threshold; ca.normalize = o.normalize != 0;
    ca.ltp = dev.d(); ca.lto = dout_grid.d(); ca.fit_status = dfs.i(); ca.bad = dbad.i();
    if (pfrt) { HIPDRT_CHECK(dpf.alloc((size_t)B * nout * sizeof(double))); ca.pfrt = dpf.d(); }
    if (raw_pfrt) { HIPDRT_CHECK(draw.alloc(bn * sizeof(double))); ca.raw = draw.d(); }
    if (post_prob) { HIPDRT_CHECK(dpost.alloc((size_t)S * B * sizeof(double))); ca.post = dpost.d(); }
    TRY(launch_pfrt_combine(st, ca, B));
    LAUNCH_OK();
    tm.mark();
    TRY(KkOut::back(pfrt, dpf, st)); TRY(KkOut::back(raw_pfrt, draw, st)); TRY(KkOut::back(post_prob, dpost, st));
    TRY(KkOut::back(step_pfrt, dstep, st));
    HIPDRT_CHECK(hipMemcpyAsync(hbad.data(), dbad.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    if (status)
        for (int b = 0; b < B; ++b) status[b] = (comb[b] >= 0 && hbad[b] != 0) ? HIPDRT_PREDICT_NOT_PD : comb[b];
    return HIPDRT_OK;
} HIPDRT_CATCH

}  // extern "C"
