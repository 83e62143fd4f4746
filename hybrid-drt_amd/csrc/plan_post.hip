// What reads a finished fit of a plan (include/hipdrt.h) apart from the DRT chain of plan_drt.hip: log-likelihood terms, the
// final P, the posterior covariance and variance, the terms of the log marginal likelihood (csrc/lml.hip), Kramers-Kronig screening
// (csrc/kk.hip), impedance and resistances (csrc/predict.hip).
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

PostSource live_source(const hipdrt_plan* p) {
    return {p->x.d(), p->s.d(), p->rho.d(), p->dop_rho.d(), p->has_weight_factors() ? p->w_eff.d() : p->w.d(), p->fit_status.i()};
}
PostSource step_source(const hipdrt_plan* p, int step, const double* w, const int* fit_status) {
    const PfrtStoreLayout L = p->pf_layout();
    return {p->pf_x.d() + L.x(step), p->pf_s.d() + L.s(step), p->pf_rho.d() + L.rho(step),
            p->pf_dop_rho.p ? p->pf_dop_rho.d() + L.rho(step) : nullptr, w, fit_status};
}
FinalP plan_final_p(const hipdrt_plan* p, int b, const PostSource& src) {
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
int plan_final_p_to_host(hipdrt_plan* p, hipStream_t st, int b, const FinalP& f, double* out) {
    PqArgs pq = p->pq_one(b, f.w);
    pq.P = p->Ptmp.d(); pq.Ppk = nullptr;
    launch_gram_l2(st, pq, f.g);
    LAUNCH_OK();
    return copy_strided(out, p->Ptmp.d(), p->n, p->n, p->ldp, st);
}

int plan_quadratic_forms_dev(hipdrt_plan* p, const PostSource& src, int b, const double* rows_dev, int neval, int ncol,
                             int col_offset, DevBuf& scratch, DevBuf& dout, DevBuf& dstat, const double* dop_sinv) {
    HIPDRT_REQUIRE(p->B > 0, "no fitted batch in the plan");
    HIPDRT_REQUIRE(b >= -1 && b < p->B, "spectrum index out of range");
    HIPDRT_REQUIRE(neval >= 1, "neval >= 1");
    HIPDRT_REQUIRE(p->n <= 4096, "posterior variance: n <= 4096");
    HIPDRT_REQUIRE(!dop_sinv || (p->prepared && p->desc.dop_size > 0), "internal: a DOP scaling for a plan without a DOP block");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const bool one = b >= 0;
    const int n = p->n, nb = one ? 1 : p->B;
    const int nex = (neval + 15) / 16, nchp = qp_nchp(n);
    // final P, packed tiles only: of every spectrum, active or not, or of spectrum b into its own slot of Ppk (all strides 0)
    const FinalP f = plan_final_p(p, b, src);
    PqArgs pq = one ? p->pq_one(b, f.w) : p->pq(f.w);
    pq.active = nullptr;
    launch_gram_l2(st, pq, f.g);
    LAUNCH_OK();
    if (dop_sinv) {
        const int nd = p->desc.dop_size;
        launch_scale_p(st, nb, n, p->desc.dop_start, nd, dop_sinv + (one ? (size_t)b * nd : 0), one ? 0 : nd, pq.Ppk, pq.ppk_stride);
        LAUNCH_OK();
    }
    DevBuf bex;
    HIPDRT_CHECK(bex.alloc((size_t)nex * nchp * 256 * sizeof(double)));
    HIPDRT_CHECK(dout.alloc((size_t)nb * nex * 16 * sizeof(double)));
    HIPDRT_CHECK(dstat.alloc((size_t)nb * sizeof(int)));
    TRY(posterior_var_dev(st, {nb, n, pq.Ppk, pq.ppk_stride, one, rows_dev, neval, ncol, col_offset, bex.d(), dout.d(), dstat.i()}, scratch));
    HIPDRT_CHECK(hipStreamSynchronize(st));      // bex is released on return
    return HIPDRT_OK;
}

int posterior_var_dev(hipStream_t st, const PosteriorChain& c, DevBuf& scratch) {
    const int n = c.n, nb = c.nb, nex = c.nex(), nchp = qp_nchp(n);
    const long long lsz = (long long)(dist_var_scratch_doubles(n, nex) + c.guard);
    // evaluation rows -> packed tiles, shifted past the special-parameter slots
    launch_pack_rows(st, c.neval, c.ncol, c.col_offset, c.rows, c.ncol, nex, c.bex, nchp);
    LAUNCH_OK();
    const int chunk = nb < 256 ? nb : 256;
    HIPDRT_CHECK(scratch.alloc(((size_t)chunk * lsz + c.guard) * sizeof(double)));
    if (c.guard) HIPDRT_CHECK(hipMemsetAsync(scratch.p, 0xA5, scratch.bytes, st));
    for (int b0 = 0; b0 < nb; b0 += chunk) {
        const int nc = (nb - b0) < chunk ? (nb - b0) : chunk;
        TRY(launch_dist_var(st, nc, n, c.ppk + (size_t)b0 * c.pstr, c.pstr, c.bex, nex, scratch.d() + c.guard, c.single ? 0 : lsz,
                            c.var + (size_t)b0 * nex * 16, c.single ? 0 : (long long)nex * 16, c.status + b0));
    }
    return HIPDRT_OK;
}

int logdet_dev(hipStream_t st, int nb, int n, const double* ppk, long long pstr, DevBuf& scratch, double* logdet, int* status) {
    const long long lsz = (long long)dist_var_scratch_doubles(n, 0);
    const int chunk = nb < 256 ? nb : 256;
    if (scratch.bytes < (size_t)chunk * lsz * sizeof(double)) HIPDRT_CHECK(scratch.alloc((size_t)chunk * lsz * sizeof(double)));
    for (int b0 = 0; b0 < nb; b0 += chunk) {
        const int nc = (nb - b0) < chunk ? (nb - b0) : chunk;
        TRY(launch_logdet(st, nc, n, ppk + (size_t)b0 * pstr, pstr, scratch.d(), lsz, logdet + b0, status + b0));
    }
    return HIPDRT_OK;
}

void posterior_cov_dev(hipStream_t st, const double* scratch_b, int n, int neval, double scale, double* dcov) {
    // Y = rows L^-T sits in tile rows nch .. nch + nex - 1 of the scratch; only the first ceil(n / 16) tile columns are non-zero
    const int nex = (neval + 15) / 16, nch = qp_nchp(n);
    launch_rows_outer(st, scratch_b + (size_t)nch * nch * 256, nch, nch, nex, neval, scale, dcov, neval);
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
    PredictTimer tm(p->ctx, st);                    // (hipdrt_debug_last_predict_ms: the launch alone)
    TRY(launch_llh(st, p->state(), p->B, d1.d(), d2.d(), stored, scalar_w));
    LAUNCH_OK();
    tm.mark();
    HIPDRT_CHECK(hipMemcpyAsync(rss, d1.p, bb, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(sum_log_w, d2.p, bb, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
}

int hipdrt_plan_get_p_matrix(hipdrt_plan* p, int b, double* out) try {
    HIPDRT_REQUIRE(p && out, "NULL pointer");
    HIPDRT_REQUIRE(b >= 0 && b < p->B, "spectrum index out of range");
    hipStream_t st; TRY(enter(p->ctx, &st));
    return plan_final_p_to_host(p, st, b, plan_final_p(p, b, live_source(p)), out);
} HIPDRT_CATCH

// out[b][i] = rows_i' P_b^-1 rows_i * cs_b^2 for the fitted batch, host rows in, host results out
static int plan_quadratic_forms(hipdrt_plan* p, const double* basis_eval, int neval, int ncol, int col_offset, double* out,
                                int* status) {
    HIPDRT_REQUIRE(p->B > 0, "no fitted batch in the plan");
    HIPDRT_REQUIRE(neval >= 1, "neval >= 1");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const int B = p->B, nex = (neval + 15) / 16;
    DevBuf dbe, scratch, dout, dstat;
    TRY(upload(dbe, basis_eval, (size_t)neval * ncol * sizeof(double), st));
    TRY(plan_quadratic_forms_dev(p, live_source(p), -1, dbe.d(), neval, ncol, col_offset, scratch, dout, dstat));
    std::vector<double> hv((size_t)B * nex * 16), cs(B);
    std::vector<int> hs(B);
    HIPDRT_CHECK(hipMemcpyAsync(hv.data(), dout.p, hv.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(cs.data(), p->coef_scale.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(hs.data(), dstat.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    // estimate_param_cov scales the inverse by coefficient_scale^2 (drt1d.py:4133)
    for (int b = 0; b < B; ++b) cs[b] *= cs[b];
    posterior_var_host(hv.data(), B, neval, cs.data(), out);
    if (status) std::memcpy(status, hs.data(), (size_t)B * sizeof(int));
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
    DevBuf dbe, scratch, dvar, dstat, dcov;
    TRY(upload(dbe, rows, (size_t)neval * ncol * sizeof(double), st));
    TRY(plan_quadratic_forms_dev(p, live_source(p), b, dbe.d(), neval, ncol, col_offset, scratch, dvar, dstat));
    HIPDRT_CHECK(dcov.alloc((size_t)neval * neval * sizeof(double)));
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
    posterior_cov_dev(st, scratch.d(), p->n, neval, cs * cs, dcov.d());
    LAUNCH_OK();
    HIPDRT_CHECK(hipMemcpyAsync(out, dcov.p, (size_t)neval * neval * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
}

static std::vector<double> host_identity(int n) {          // the rows of the parameter covariance and variance
    std::vector<double> eye((size_t)n * n, 0.0);
    for (int i = 0; i < n; ++i) eye[(size_t)i * n + i] = 1.0;
    return eye;
}

int hipdrt_plan_distribution_cov(hipdrt_plan* p, int b, const double* basis_eval, int neval, double* out, int* status) try {
    HIPDRT_REQUIRE(p && basis_eval && out, "NULL pointer");
    return plan_full_cov(p, b, basis_eval, neval, p->ntau, p->ns, out, status);
} HIPDRT_CATCH

int hipdrt_plan_param_cov(hipdrt_plan* p, int b, double* out, int* status) try {
    HIPDRT_REQUIRE(p && out, "NULL pointer");
    const int n = p->n;
    return plan_full_cov(p, b, host_identity(n).data(), n, n, 0, out, status);
} HIPDRT_CATCH

int hipdrt_plan_distribution_var(hipdrt_plan* p, const double* basis_eval, int neval, double* out, int* status) try {
    HIPDRT_REQUIRE(p && basis_eval && out, "NULL pointer");
    return plan_quadratic_forms(p, basis_eval, neval, p->ntau, p->ns, out, status);
} HIPDRT_CATCH

int hipdrt_plan_param_var(hipdrt_plan* p, double* out, int* status) try {
    HIPDRT_REQUIRE(p && out, "NULL pointer");
    const int n = p->n;
    return plan_quadratic_forms(p, host_identity(n).data(), n, n, 0, out, status);
} HIPDRT_CATCH

// ---- the log marginal likelihood (csrc/lml.hip, qp_resident.hpp: logdet_kernel_resident) ---------------------------------------
void hipdrt_default_lml_in(hipdrt_lml_in* in) {
    if (!in) return;
    std::memset(in, 0, sizeof(*in));
    in->step = -1;
    // get_default_hypers (qphb.py:208-255); read only with override_hypers
    in->l2_lambda_0 = 142.0; in->dop_l2_lambda_0 = 10.0;
    const double dw[3] = {1.5, 1.0, 0.5}, ddw[3] = {0.5, 1.0, 0.5};
    for (int k = 0; k < 3; ++k) { in->derivative_weights[k] = dw[k]; in->dop_derivative_weights[k] = ddw[k]; }
}

int hipdrt_plan_lml_terms(hipdrt_plan* p, const hipdrt_lml_in* in_, hipdrt_lml_out* out) try {
    HIPDRT_REQUIRE(p && out, "NULL pointer");
    const hipdrt_lml_in in = opts_or(in_, hipdrt_default_lml_in);
    HIPDRT_REQUIRE(p->B >= 1 && p->prepped, "no fitted batch in the plan");
    HIPDRT_REQUIRE(p->n <= 4096, "log marginal likelihood: n <= 4096");
    const int B = p->B, n = p->n, m = p->m;
    const bool dop = p->prepared && p->desc.dop_size > 0;
    const bool uploaded = in.x || in.rho || in.s || in.dop_rho;
    // every check comes before the first launch
    if (uploaded) {
        HIPDRT_REQUIRE(in.x && in.rho && in.s, "an uploaded state needs x, rho and s together");
        HIPDRT_REQUIRE(in.step < 0, "an uploaded state and a recorded step exclude each other");
        HIPDRT_REQUIRE(dop == (in.dop_rho != nullptr), "dop_rho is required exactly when the plan has a DOP block");
    }
    HIPDRT_REQUIRE(in.step < p->pf_steps, "step out of range of the recorded steps");
    if (in.weights)
        for (size_t i = 0; i < (size_t)B * m; ++i)
            HIPDRT_REQUIRE(in.weights[i] > 0.0 && std::isfinite(in.weights[i]), "weights must be positive and finite");
    double l2 = p->opts.l2_lambda_0, dop_l2 = dop ? p->desc.dop_l2_lambda_0 : 0.0, dw[3], ddw[3];
    for (int k = 0; k < 3; ++k) { dw[k] = p->opts.derivative_weights[k]; ddw[k] = dop ? p->desc.dop_derivative_weights[k] : 0.0; }
    if (in.override_hypers) {
        l2 = in.l2_lambda_0; dop_l2 = in.dop_l2_lambda_0;
        for (int k = 0; k < 3; ++k) { dw[k] = in.derivative_weights[k]; ddw[k] = in.dop_derivative_weights[k]; }
        HIPDRT_REQUIRE(std::isfinite(l2) && (!dop || std::isfinite(dop_l2)), "hyper override: l2_lambda_0 and dop_l2_lambda_0 must be finite");
        for (int k = 0; k < 3; ++k)
            HIPDRT_REQUIRE(std::isfinite(dw[k]) && (!dop || std::isfinite(ddw[k])), "hyper override: derivative weights must be finite");
    }
    TRY(lds_check(lml_sums_lds_bytes(n, m), "lml sums", "n, m"));
    hipStream_t st; TRY(enter(p->ctx, &st));

    const size_t D = sizeof(double);
    DevBuf dx, drho, ds, ddop, dwt, dzero, scratch, dst;
    PostSource src = live_source(p);
    if (uploaded) {
        TRY(upload(dx, in.x, (size_t)B * n * D, st)); TRY(upload(drho, in.rho, (size_t)B * 3 * D, st));
        TRY(upload(ds, in.s, (size_t)B * 3 * n * D, st));
        if (dop) TRY(upload(ddop, in.dop_rho, (size_t)B * 3 * D, st));
        src = PostSource{dx.d(), ds.d(), drho.d(), dop ? ddop.d() : nullptr, nullptr, p->fit_status.i()};
    } else if (in.step >= 0) {
        src = step_source(p, in.step, nullptr, p->pf_status.i() + p->pf_layout().scalar(in.step));
    }
    // upstream's default is qphb_params['est_weights'], never the scaled weights of the last calculate_pq
    if (in.weights) TRY(upload(dwt, in.weights, (size_t)B * m * D, st));
    src.w = in.weights ? dwt.d() : p->est_w.d();
    HIPDRT_CHECK(dzero.alloc((size_t)B * m * D));
    HIPDRT_CHECK(hipMemsetAsync(dzero.p, 0, (size_t)B * m * D, st));
    HIPDRT_CHECK(dst.alloc((size_t)2 * B * sizeof(int)));

    GramL2 g = plan_l2(p, l2, dw, dop_l2, ddw);
    g.s = src.s; g.rho = src.rho;
    if (g.dop_size > 0) g.dop_rho = src.dop_rho;

    LmlSumsArgs sa{};
    sa.m = m; sa.n = n; sa.ldrm = p->ldrm; sa.rm = p->rm.d(); sa.rm_stride = p->rm_stride; sa.rv = p->rv.d(); sa.w = src.w;
    sa.x = src.x; sa.g = g; sa.l1 = p->l1.d(); sa.fit_status = src.fit_status;
    double *dlp = nullptr, *dlo = nullptr;
    DevOuts outs;
    TRY(outs.want(out->logdet_p, B, dlp, true)); TRY(outs.want(out->logdet_prior, B, dlo, true));
    TRY(outs.want(out->wy2, B, sa.wy2)); TRY(outs.want(out->fit2, B, sa.fit2)); TRY(outs.want(out->cross, B, sa.cross));
    TRY(outs.want(out->slw, B, sa.slw)); TRY(outs.want(out->xox, B, sa.xox)); TRY(outs.want(out->l1x, B, sa.l1x));

    PredictTimer tm(p->ctx, st);
    // P, packed tiles only, of every member whether still active or not; then Omega into the same place
    PqArgs pq = p->pq(src.w);
    pq.active = nullptr;
    launch_gram_l2(st, pq, g);
    LAUNCH_OK();
    TRY(logdet_dev(st, B, n, pq.Ppk, pq.ppk_stride, scratch, dlp, dst.i()));
    pq.w = dzero.d();
    launch_gram_l2(st, pq, g);
    LAUNCH_OK();
    TRY(logdet_dev(st, B, n, pq.Ppk, pq.ppk_stride, scratch, dlo, dst.i() + B));
    TRY(launch_lml_sums(st, sa, B));
    LAUNCH_OK();
    tm.mark();

    std::vector<int> hfit(B), hdet(2 * (size_t)B), hstat(B);
    HIPDRT_CHECK(hipMemcpyAsync(hfit.data(), src.fit_status, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(hdet.data(), dst.p, (size_t)2 * B * sizeof(int), hipMemcpyDeviceToHost, st));
    TRY(outs.back(st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    for (int b = 0; b < B; ++b) hdet[b] = (hdet[b] != 0 || hdet[(size_t)B + b] != 0) ? -1 : 0;
    merge_status(B, hfit.data(), hdet.data(), hstat.data());
    // a member whose fit failed: every row NaN (the sums are, by the kernel; the determinants of whatever its state held are not)
    for (int b = 0; b < B; ++b)
        if (hfit[b] < 0) {
            if (out->logdet_p) out->logdet_p[b] = __builtin_nan("");
            if (out->logdet_prior) out->logdet_prior[b] = __builtin_nan("");
        }
    if (out->status) std::memcpy(out->status, hstat.data(), (size_t)B * sizeof(int));
    return HIPDRT_OK;
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
    hipdrt_kk_opts o = opts_or(opts, hipdrt_default_kk_opts);
    TRY(kk_check_opts(o));
    HIPDRT_REQUIRE(kk_lds_bytes(p->nf, p->n, 1) <= kLdsLimit, "KK screen: nf and n too large for one workgroup's LDS");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const int B = p->B, nf = p->nf, m = p->m;
    KkArgs a{};
    a.nf = nf; a.desc = p->freq_order > 0 ? 1 : 0; a.freq = p->freq.d(); a.o = o;
    const size_t bn = (size_t)B * nf;
    DevOuts outs;
    TRY(outs.want(z_hat_re, bn, a.z_re)); TRY(outs.want(z_hat_im, bn, a.z_im));
    TRY(outs.want(err_re, bn, a.e_re)); TRY(outs.want(err_im, bn, a.e_im));
    TRY(outs.want(std_out, B, a.std)); TRY(outs.want(outlier_mask, bn, a.mask)); TRY(outs.want(f_lim, 2 * B, a.f_lim));
    TRY(outs.want(i_lim, 2 * B, a.i_lim)); TRY(outs.want(status, B, a.status));
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
    TRY(outs.back(st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

// ---- the tau basis of a prepared plan, impedance and resistances (csrc/predict.hip) ----------------------------------------------
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
        HIPDRT_CHECK(cr.alloc(impedance_scratch_doubles(1, 0, nf, ntau, p->mode, 0) * sizeof(double)));
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
    launch_drt_scalars(st, B, dsum.d(), dabs.d(), p->coef_scale.d(), basis_area(pb.eps), 0, abs_norm != 0, p->x.d(), n,
                       p->idx_rinf, drp.d(), dri.d(), drt.d(), nullptr, nullptr);
    LAUNCH_OK();
    if (r_p) HIPDRT_CHECK(hipMemcpyAsync(r_p, drp.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
    if (r_inf) HIPDRT_CHECK(hipMemcpyAsync(r_inf, dri.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
    if (r_tot) HIPDRT_CHECK(hipMemcpyAsync(r_tot, drt.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

}  // extern "C"
