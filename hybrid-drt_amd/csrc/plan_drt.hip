// The DRT chain on a finished fit of a plan (include/hipdrt.h): the evaluation rows of the batch and their variances (DrtRows),
// and what is built on them -- DRT prediction and window integrals (csrc/predict.hip), peak finding (csrc/peaks.hip), the peak
// and trough probabilities (csrc/peak_prob.hip), per-peak resolution (csrc/peak_resolve.hip) and the PFRT over the recorded
// steps of a PFRT fit (csrc/pfrt.hip).  The fitted state, the
// final P and the variance path come from plan_post.hip (plan.hpp).
#include <cmath>
#include <cstring>
#include <optional>

#include "plan.hpp"

namespace hipdrt {
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

int predict_basis(const hipdrt_plan* p, PredictBasis& pb) {
    HIPDRT_REQUIRE(p->B >= 1 && p->prepped, "no fitted batch in the plan");
    if (p->prepared) {
        HIPDRT_REQUIRE(p->basis_nb > 0, "a prepared plan needs hipdrt_plan_set_tau_basis before a DRT prediction");
        pb = {p->basis_ln_tau.d(), p->basis_nb, (p->n - p->ns) / p->basis_nb, p->basis_eps};
    } else {
        pb = {p->ln_tau.d(), p->ntau, 1, p->eps};
    }
    return HIPDRT_OK;
}

PfrtCombineArgs pfrt_combine_args(const hipdrt_pfrt_opts& o, int m) {
    PfrtCombineArgs a{};
    pfrt_llh_consts(m, &a.c, &a.alpha_n, &a.beta_0);
    a.prior_mu = o.prior_mu; a.prior_sigma = o.prior_sigma; a.n_eff = o.n_eff_factor;
    a.smooth = o.smooth != 0; a.smooth_order = o.smooth_order; a.smooth_eps = o.smooth_epsilon;
    a.integrate = o.integrate != 0; a.thr = o.integrate_threshold; a.normalize = o.normalize != 0;
    return a;
}
}  // namespace hipdrt

// what every DRT request checks of its sign (under the name the caller gives it) and of normalize against row_scale (host [B],
// or null); the entries of row_scale are checked by drt_check_row_scale, where each caller's order of refusals has them
static int drt_check_request(const PredictBasis& pb, int sign, int normalize, const double* row_scale, const char* sign_name) {
    HIPDRT_REQUIRE(sign == 1 || (pb.copies == 2 && (sign == 0 || sign == -1)),
                   std::string(sign_name) + " must be 1, or 1, -1 or 0 when the DRT block holds a positive and a negative copy");
    HIPDRT_REQUIRE(normalize >= 0 && normalize <= 2, "normalize must be 0, 1 (by R_p) or 2 (by absolute R_p)");
    HIPDRT_REQUIRE(!row_scale || normalize == 0, "row_scale goes with normalize = 0 (a ratio to the spectrum's own R_p carries no scale)");
    return HIPDRT_OK;
}
static int drt_check_row_scale(const double* row_scale, int B) {
    if (row_scale) for (int b = 0; b < B; ++b) HIPDRT_REQUIRE(row_scale[b] > 0.0 && std::isfinite(row_scale[b]), "row_scale must be positive and finite");
    return HIPDRT_OK;
}

// What a DRT prediction leaves on the device (hipdrt_plan_predict_drt, hipdrt_plan_find_peaks, hipdrt_plan_peak_trough_probs): for every order asked for the
// signed evaluation rows and the mean rows of the batch, the normalisation scalars, and (want_var) e' inv(P_b) e of all rows from
// one factorisation per spectrum, not yet scaled.
struct DrtRows {
    DevBuf dgrid, dE, dsum, dabs, dnorm, dscale, dcs, dmu, dvar, dvstat;
    const double* grid = nullptr;        // [neval] ln(tau_eval) on the device
    const double* scale = nullptr;       // [B] the factor the mean rows carry
    const double* cs = nullptr;          // [B] the coefficient scale behind it (times row_scale)
    const double* norm = nullptr;        // [B] R_p, or null without normalisation
    int neval = 0, B = 0, norders = 0;
    double* mu(int k) const { return dmu.d() + (size_t)k * B * neval; }                 // [B][neval] of orders[k]
    const double* var(int k) const { return dvar.d() + (size_t)k * neval; }             // row stride ldv()
    long long ldv() const { return (long long)((norders * neval + 15) / 16) * 16; }
    // the grid uploaded, dE [norders * neval][width] and dmu [norders][B][neval] allocated
    int begin(const hipdrt_plan* p, const double* ln_tau_host, int neval_, int norders_, hipStream_t st) {
        TRY(upload(dgrid, ln_tau_host, (size_t)neval_ * sizeof(double), st));
        HIPDRT_CHECK(dE.alloc((size_t)norders_ * neval_ * (p->n - p->ns) * sizeof(double)));
        return begin_mu(p, dgrid.d(), neval_, norders_);
    }
    // ... on a device grid and a dE that the caller keeps across the calls of a loop
    int begin(const hipdrt_plan* p, const double* grid_dev, const DevBuf& dE_kept, int neval_, int norders_) {
        dE.alias(dE_kept, 0, dE_kept.bytes);
        return begin_mu(p, grid_dev, neval_, norders_);
    }
    int begin_mu(const hipdrt_plan* p, const double* grid_dev, int neval_, int norders_) {
        grid = grid_dev; neval = neval_; B = p->B; norders = norders_;
        HIPDRT_CHECK(dmu.alloc((size_t)norders * B * neval * sizeof(double)));
        return HIPDRT_OK;
    }
};
// orders[R.norders] (any number of them): rows k * neval .. of dE and slab k of dmu belong to orders[k].  row_scale: host [B] or
// null.  The timer is marked once, after the mean rows.
// have_E: dE already holds the evaluation rows (a second call on the same grid, orders and sign).
static int plan_drt_rows_dev(hipdrt_plan* p, const PostSource& src, const PredictBasis& pb, const int* orders, int sign,
                             int normalize, const double* row_scale, bool want_var, hipStream_t st, DrtRows& R, PredictTimer& tm,
                             bool have_E = false) {
    const int B = p->B, n = p->n, ns = p->ns, width = n - ns, nb = pb.nb, neval = R.neval, norders = R.norders;
    // E[neval][width]: the signed evaluation rows over the whole DRT block (+E | 0), (0 | -E) or (+E | -E)
    if (!have_E && pb.copies == 2 && sign != 0) HIPDRT_CHECK(hipMemsetAsync(R.dE.p, 0, R.dE.bytes, st));
    for (int k = 0; k < norders && !have_E; ++k) {
        double* E = R.dE.d() + (size_t)k * neval * width;
        if (sign != -1) TRY(func_eval_dev(st, pb.ln_tau, nb, R.grid, neval, pb.eps, orders[k], 1.0, E, width));
        if (pb.copies == 2 && sign != 1) TRY(func_eval_dev(st, pb.ln_tau, nb, R.grid, neval, pb.eps, orders[k], -1.0, E + nb, width));
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
        // (a DrtRows that is used again on the same stream keeps its buffers: the candidates of hipdrt_plan_score_candidates)
        for (DevBuf* d : {&R.dsum, &R.dabs, &R.dnorm, &R.dscale})
            if (d->bytes < (size_t)B * sizeof(double)) HIPDRT_CHECK(d->alloc((size_t)B * sizeof(double)));
        launch_drt_sums(st, B, src.x, n, ns, nb, pb.copies, sign, R.dsum.d(), R.dabs.d());
        launch_drt_scalars(st, B, R.dsum.d(), R.dabs.d(), R.cs, basis_area(pb.eps), 1, normalize == 2,
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
    // sigma^2 = diag(E inv(P) E') from the variance path, fed the evaluation rows where they are (all orders as one row block)
    DevBuf scratch;
    if (want_var) TRY(plan_quadratic_forms_dev(p, src, -1, R.dE.d(), norders * neval, width, ns, scratch, R.dvar, R.dvstat));
    return HIPDRT_OK;
}
// The end of an entry point on R: the per-spectrum status on the device (the fit's, or a kernel's built on it) and, have_var, the
// variance path's come back, the stream is synchronised, and merge_status of the two goes to status_out (host [B] or null) and to
// *merged.
static int drt_status_back(const DrtRows& R, const int* fit_status_dev, bool have_var, hipStream_t st, int* status_out,
                           std::vector<int>* merged = nullptr) {
    std::vector<int> hs(R.B), hv(R.B, 0);
    HIPDRT_CHECK(hipMemcpyAsync(hs.data(), fit_status_dev, hs.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    if (have_var) HIPDRT_CHECK(hipMemcpyAsync(hv.data(), R.dvstat.p, hv.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    merge_status(R.B, hs.data(), have_var ? hv.data() : nullptr, hs.data());
    if (status_out) std::memcpy(status_out, hs.data(), hs.size() * sizeof(int));
    if (merged) merged->swap(hs);
    return HIPDRT_OK;
}

// the rows launch_peaks reads, from a DrtRows of orders {2, 0}: fxx, f (need_f) and, for need_var, the variances with their scaling
static void peak_args_rows(PeakArgs& a, const DrtRows& R, const hipdrt_peak_opts& o, bool need_f, bool need_var,
                           const int* fit_status) {
    a.neval = R.neval; a.o = o; a.fxx = R.mu(0); a.f = need_f ? R.mu(1) : nullptr; a.fit_status = fit_status;
    if (need_var) {
        a.var_fxx = R.var(0); a.var_f = o.method == 2 ? R.var(1) : nullptr; a.ldv = R.ldv();
        a.cs = R.cs; a.norm = R.norm; a.var_status = R.dvstat.i();
    }
}

extern "C" {

int hipdrt_plan_predict_drt(hipdrt_plan* p, const double* ln_tau_eval, int neval, int order, int sign, int normalize, double s_lo,
                            double s_hi, double* mu, double* lo, double* hi, int* status) try {
    HIPDRT_REQUIRE(p && ln_tau_eval && mu, "NULL pointer");
    PredictBasis pb;
    TRY(predict_basis(p, pb));
    HIPDRT_REQUIRE(neval >= 1, "neval >= 1");
    HIPDRT_REQUIRE(order >= 0 && order <= 2, "order must be 0, 1 or 2");
    TRY(drt_check_request(pb, sign, normalize, nullptr, "sign"));
    const bool band = lo || hi;
    HIPDRT_REQUIRE(!band || (std::isfinite(s_lo) && std::isfinite(s_hi)), "s_lo and s_hi must be finite");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const int B = p->B;
    DrtRows R;
    TRY(R.begin(p, ln_tau_eval, neval, 1, st));
    PredictTimer tm(p->ctx, st);
    TRY(plan_drt_rows_dev(p, live_source(p), pb, &order, sign, normalize, nullptr, band, st, R, tm));
    DevOuts outs;
    double *dlo = nullptr, *dhi = nullptr;
    if (band) {
        TRY(outs.want(lo, (size_t)B * neval, dlo)); TRY(outs.want(hi, (size_t)B * neval, dhi));
        launch_drt_band(st, B, neval, R.mu(0), R.dvar.d(), R.ldv(), p->coef_scale.d(), R.norm, s_lo, s_hi, R.dvstat.i(),
                        p->fit_status.i(), dlo, dhi);
        LAUNCH_OK();
        tm.mark();
        TRY(outs.back(st));
    }
    HIPDRT_CHECK(hipMemcpyAsync(mu, R.dmu.p, R.dmu.bytes, hipMemcpyDeviceToHost, st));
    return drt_status_back(R, p->fit_status.i(), band, st, status);
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
    hipdrt_peak_opts o = opts_or(opts, hipdrt_peak_opts_default);
    // every check comes before the first launch
    TRY(peak_check_opts(o, neval));
    const int sign = o.eval_sign, normalize = o.normalize;
    const int B = p->B;
    TRY(drt_check_request(pb, sign, normalize, row_scale, "eval_sign"));
    TRY(drt_check_row_scale(row_scale, B));
    const bool need_f = o.search == 0 || o.method == 2, need_var = o.method >= 1;
    const int orders[2] = {2, 0}, norders = need_f ? 2 : 1;
    HIPDRT_REQUIRE(peaks_lds_bytes(neval, o.method, need_f, o.num_peaks) <= kLdsLimit,
                   "find_peaks: neval too large for one workgroup's LDS");
    hipStream_t st; TRY(enter(p->ctx, &st));
    DrtRows R;
    TRY(R.begin(p, ln_tau_eval, neval, norders, st));
    const size_t bn = (size_t)B * neval;
    PeakArgs a{};
    DevOuts outs;
    TRY(outs.want(peak_sign, bn, a.peak_sign)); TRY(outs.want(keep, bn, a.keep)); TRY(outs.want(heights, bn, a.heights));
    TRY(outs.want(prominences, bn, a.prominences)); TRY(outs.want(probs, bn, a.probs)); TRY(outs.want(left_bases, bn, a.left_bases));
    TRY(outs.want(right_bases, bn, a.right_bases)); TRY(outs.want(count, B, a.count)); TRY(outs.want(used_prominence, B, a.used_prominence));
    TRY(outs.want(o.method == 2 ? peak_prob : nullptr, bn, a.peak_prob)); TRY(outs.want(o.method == 2 ? curv_prob : nullptr, bn, a.curv_prob));
    PredictTimer tm(p->ctx, st);
    TRY(plan_drt_rows_dev(p, live_source(p), pb, orders, sign, normalize, row_scale, need_var, st, R, tm));
    peak_args_rows(a, R, o, need_f, need_var, p->fit_status.i());
    TRY(launch_peaks(st, a, B));
    LAUNCH_OK();
    tm.mark();
    TRY(outs.back(st));
    return drt_status_back(R, p->fit_status.i(), need_var, st, status);
} HIPDRT_CATCH

// ---- peak and trough probabilities of the fitted batch (csrc/peak_prob.hip) ------------------------------------------------------
void hipdrt_peak_prob_opts_default(hipdrt_peak_prob_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->bayes_cov = 1; o->std_size = 5; o->std_baseline = 0.1; o->sigma_floor = 1; o->ext_left = -1; o->ext_right = -1;
    o->search = 0; o->height = __builtin_nan(""); o->prominence = __builtin_nan("");
}

int hipdrt_plan_peak_trough_probs(hipdrt_plan* p, const double* ln_tau_eval, int neval, const hipdrt_peak_prob_opts* opts,
                                  const double* row_scale, int nranges, const int* range_lo, const int* range_hi, double* mu,
                                  double* pp, double* tp, double* prob, double* sigma, int* keep, double* heights,
                                  double* prominences, int* left_bases, int* right_bases, int* count, int* range_peaks,
                                  int* status) try {
    HIPDRT_REQUIRE(p && ln_tau_eval, "NULL pointer");
    PredictBasis pb;
    TRY(predict_basis(p, pb));
    hipdrt_peak_prob_opts o = opts_or(opts, hipdrt_peak_prob_opts_default);
    // every check comes before the first launch
    TRY(peak_prob_check(o, neval, nranges, range_lo, range_hi));
    const int B = p->B;
    // predict_drt(tau, order=k) at its defaults (drt1d.py:3667): sign 1, not normalised
    TRY(drt_check_request(pb, 1, 0, row_scale, "sign"));
    TRY(drt_check_row_scale(row_scale, B));
    const bool need_var = o.bayes_cov != 0;
    const int orders[3] = {0, 1, 2};
    if (o.search != 2) nranges = 0;
    hipStream_t st; TRY(enter(p->ctx, &st));
    DevBuf dlo, dhi;
    DrtRows R;
    TRY(R.begin(p, ln_tau_eval, neval, 3, st));
    if (nranges > 0) {
        TRY(upload(dlo, range_lo, (size_t)nranges * sizeof(int), st)); TRY(upload(dhi, range_hi, (size_t)nranges * sizeof(int), st));
    }
    const size_t bn = (size_t)B * neval;
    PeakProbArgs a{};
    DevOuts outs;
    TRY(outs.want(pp, bn, a.pp)); TRY(outs.want(tp, bn, a.tp)); TRY(outs.want(prob, bn, a.prob)); TRY(outs.want(sigma, 3 * bn, a.sigma));
    TRY(outs.want(keep, bn, a.keep)); TRY(outs.want(heights, bn, a.heights)); TRY(outs.want(prominences, bn, a.prominences));
    TRY(outs.want(left_bases, bn, a.left_bases)); TRY(outs.want(right_bases, bn, a.right_bases)); TRY(outs.want(count, B, a.count));
    TRY(outs.want(nranges > 0 ? range_peaks : nullptr, (size_t)B * nranges, a.range_peaks));
    PredictTimer tm(p->ctx, st);
    // one factorisation per spectrum, fed the rows of all three orders
    TRY(plan_drt_rows_dev(p, live_source(p), pb, orders, 1, 0, row_scale, need_var, st, R, tm));
    a.neval = neval; a.nranges = nranges; a.o = o; a.f = R.mu(0); a.fx = R.mu(1); a.fxx = R.mu(2);
    a.fit_status = p->fit_status.i(); a.range_lo = dlo.i(); a.range_hi = dhi.i();
    if (need_var) {
        a.var_f = R.var(0); a.var_fx = R.var(1); a.var_fxx = R.var(2); a.ldv = R.ldv(); a.cs = R.cs; a.var_status = R.dvstat.i();
    }
    TRY(launch_peak_prob(st, a, B));
    LAUNCH_OK();
    tm.mark();
    TRY(outs.back(st));
    if (mu) HIPDRT_CHECK(hipMemcpyAsync(mu, R.dmu.p, R.dmu.bytes, hipMemcpyDeviceToHost, st));
    return drt_status_back(R, p->fit_status.i(), need_var, st, status);
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
    hipdrt_peak_resolve_opts o = opts_or(opts, hipdrt_peak_resolve_opts_default);
    // every check comes before the first launch
    TRY(peak_resolve_check_opts(o));
    const int B = p->B, n = p->n, ns = p->ns, width = n - ns, nfind = in->nfind, mp = o.max_peaks;
    const bool want_out = out->r_peaks || out->peak_gammas;
    const int nout = want_out ? in->nout : 0;
    HIPDRT_REQUIRE(nfind >= 1, "nfind >= 1");
    HIPDRT_REQUIRE(!want_out || (in->ln_tau_out && in->nout >= 1), "r_peaks and peak_gammas need the output grid");
    TRY(drt_check_request(pb, o.sign, 0, in->row_scale, "sign"));
    TRY(peak_resolve_check_source(in->source, in->peak_indices, B, mp, in->win_start, in->win_end, in->nwin, nfind));
    TRY(drt_check_row_scale(in->row_scale, B));
    hipdrt_peak_opts po = opts_or(in->peak_opts, hipdrt_peak_opts_default);
    const bool find = in->source == HIPDRT_PEAKS_FROM_FIND;
    bool need_var = false;
    if (find) {
        TRY(peak_check_opts(po, nfind));
        HIPDRT_REQUIRE(po.eval_sign == o.sign, "peak_opts.eval_sign must equal opts.sign (estimate_peak_coef hands its sign to find_peaks)");
        HIPDRT_REQUIRE(po.method == 0 || po.method == 1, "peak_opts.method must be 0 (thresh) or 1 (prob)");
        HIPDRT_REQUIRE(po.normalize >= 0 && po.normalize <= 2, "normalize must be 0, 1 (by R_p) or 2 (by absolute R_p)");
        HIPDRT_REQUIRE(peaks_lds_bytes(nfind, po.method, 1, po.num_peaks) <= kLdsLimit,
                       "find_peaks: nfind too large for one workgroup's LDS");
        need_var = po.method >= 1;
    }
    TRY(lds_check(peak_resolve_lds_bytes(nfind, pb.nb, nout, mp), "resolve_peaks", "nfind, nb, nout, max_peaks"));
    hipStream_t st; TRY(enter(p->ctx, &st));
    const int orders[2] = {2, 0};
    const int normalize = find ? po.normalize : 0;
    DevBuf dout_grid, dE0, dkeep, dmu2, didx, dws, dwe, dst;
    DrtRows R;
    TRY(R.begin(p, in->ln_tau_find, nfind, 2, st));
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
    // (count and status: the kernel writes them whatever the caller asked for; the status is merged on the host below)
    HIPDRT_CHECK(dst.alloc((size_t)B * sizeof(int))); a.status = dst.i();
    DevOuts outs;
    TRY(outs.want(out->count, B, a.count, true)); TRY(outs.want(out->peak_index, bm, a.peak_index)); TRY(outs.want(out->trough_index, bm, a.trough_index));
    TRY(outs.want(out->eps_l, bm, a.eps_l)); TRY(outs.want(out->eps_r, bm, a.eps_r)); TRY(outs.want(out->r_peaks, bm, a.r_peaks));
    TRY(outs.want(out->r_coef, bm, a.r_coef)); TRY(outs.want(out->x_peaks, bm * pb.nb, a.x_peaks)); TRY(outs.want(out->peak_gammas, bm * nout, a.peak_gammas));
    PredictTimer tm(p->ctx, st);
    TRY(plan_drt_rows_dev(p, live_source(p), pb, orders, o.sign, normalize, in->row_scale, need_var, st, R, tm));
    a.fxx = R.mu(0); a.f = R.mu(1);
    if (find) {
        HIPDRT_CHECK(dkeep.alloc((size_t)B * nfind * sizeof(int)));
        PeakArgs pa{};
        peak_args_rows(pa, R, po, true, need_var, p->fit_status.i());
        pa.keep = dkeep.i();
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
    a.lt = R.grid; a.lb = pb.ln_tau; a.basis_area = basis_area(pb.eps);
    a.fit_status = p->fit_status.i();
    TRY(launch_peak_resolve(st, a, B));
    LAUNCH_OK();
    tm.mark();
    TRY(outs.back(st));
    std::vector<int> hs;
    TRY(drt_status_back(R, dst.i(), need_var, st, out->status, &hs));
    bool unordered = false;
    for (int b = 0; b < B; ++b) unordered = unordered || hs[b] == HIPDRT_PEAKS_UNORDERED;
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
    TRY(drt_check_request(pb, sign, normalize, row_scale, "sign"));
    HIPDRT_REQUIRE(nwin >= 1 && nwin <= 65535, "1 <= nwin <= 65535");
    TRY(peak_resolve_check_source(2, nullptr, 0, nwin, win_start, win_end, nwin, neval));
    const int B = p->B;
    TRY(drt_check_row_scale(row_scale, B));
    hipStream_t st; TRY(enter(p->ctx, &st));
    DevBuf dws, dwe, dres;
    DrtRows R;
    TRY(R.begin(p, ln_tau_eval, neval, 1, st));
    TRY(upload(dws, win_start, (size_t)nwin * sizeof(int), st)); TRY(upload(dwe, win_end, (size_t)nwin * sizeof(int), st));
    HIPDRT_CHECK(dres.alloc((size_t)B * nwin * sizeof(double)));
    PredictTimer tm(p->ctx, st);
    TRY(plan_drt_rows_dev(p, live_source(p), pb, &order, sign, normalize, row_scale, false, st, R, tm));
    launch_window_trapz(st, B, neval, nwin, R.mu(0), R.grid, dws.i(), dwe.i(), dres.d());
    LAUNCH_OK();
    tm.mark();
    HIPDRT_CHECK(hipMemcpyAsync(out, dres.p, (size_t)B * nwin * sizeof(double), hipMemcpyDeviceToHost, st));
    if (status) HIPDRT_CHECK(hipMemcpyAsync(status, p->fit_status.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
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
    DevBuf dw, dscratch;
    TRY(step_weights(p, step, st, dw, dscratch));
    // (synchronises: dw may go)
    return plan_final_p_to_host(p, st, b, plan_final_p(p, b, step_source(p, step, dw.d(), nullptr)), out);
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

// What hipdrt_plan_predict_pfrt and hipdrt_plan_pfrt_select share.  pfrt_request: every check of the plan, the factors and the
// options (o already holds the caller's or the defaults; np, nout the two grids), before the first launch.  pfrt_steps_dev: the
// loop over the recorded steps -- the step weights, the rows, one factorisation per step, launch_peaks and launch_pfrt_step --
// which leaves the steps' rows and the status vectors on the device.
struct PfrtSteps {
    DevBuf dev, dfs, dbad, dlnf, dstep;      // ln(tau_pfrt) [np], merged fit status [B], variance flag [B], ln(factors) [S], [S][B][np]
    std::vector<int> comb;                   // host image of dfs: a spectrum whose fit failed in any step is dead in every step
    size_t bn = 0;                           // B * np
    std::optional<PredictTimer> tm;          // started before the first step; the caller marks it after its last launch
};
static int pfrt_request(hipdrt_plan* p, const double* factors, const double* ln_tau_pfrt, const hipdrt_pfrt_opts& o, int np,
                        int nout, PredictBasis& pb, hipdrt_peak_opts& po) {
    HIPDRT_REQUIRE(p && factors && ln_tau_pfrt, "NULL pointer");
    if (p->prepared) {
        set_error("not supported: predict_pfrt is built for plain EIS plans (hipdrt_plan_create); a prepared plan records its steps "
                  "and gives their P matrices only");
        return HIPDRT_E_UNSUPPORTED;
    }
    TRY(predict_basis(p, pb));
    const int S = p->pf_steps;
    HIPDRT_REQUIRE(S >= 1, "no recorded PFRT steps in the plan (hipdrt_plan_pfrt_begin / _record around the fit's steps)");
    TRY(pfrt_check(o, S, np, nout));
    HIPDRT_REQUIRE(o.eval_sign == 1, "eval_sign must be 1 (the DRT block of a plain EIS plan holds one copy of the basis)");
    for (int i = 0; i < S; ++i) HIPDRT_REQUIRE(factors[i] > 0.0 && std::isfinite(factors[i]), "factors must be positive and finite");
    hipdrt_peak_opts_default(&po);
    po.eval_sign = 1; po.search = o.search; po.normalize = 1; po.method = 0; po.height = o.height; po.prominence = o.prominence;
    TRY(peak_check_opts(po, np));
    HIPDRT_REQUIRE(peaks_lds_bytes(np, 0, 1, 0) <= kLdsLimit, "predict_pfrt: neval_pfrt too large for one workgroup's LDS");
    return HIPDRT_OK;
}
static int pfrt_steps_dev(hipdrt_plan* p, const PredictBasis& pb, const hipdrt_pfrt_opts& o, const hipdrt_peak_opts& po,
                          const double* factors, const double* ln_tau_pfrt, int np, hipStream_t st, PfrtSteps& W) {
    const int S = p->pf_steps, B = p->B, width = p->n - p->ns;
    std::vector<int> hs((size_t)S * B);
    W.comb.assign(B, 0);
    for (int i = 0; i < S; ++i)
        HIPDRT_CHECK(hipMemcpyAsync(hs.data() + (size_t)i * B, p->pf_status.i() + p->pf_layout().scalar(i), (size_t)B * sizeof(int),
                                    hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    for (int b = 0; b < B; ++b)
        for (int i = 0; i < S; ++i) {
            const int v = hs[(size_t)i * B + b];
            if (W.comb[b] >= 0 && (v < 0 || v > W.comb[b])) W.comb[b] = v;
        }
    std::vector<double> lnf(S);
    for (int i = 0; i < S; ++i) lnf[i] = std::log(factors[i]);

    const size_t bn = W.bn = (size_t)B * np;
    DevBuf dw, dscratch, dnorm0, dsg, dht, dpr, dE;
    TRY(upload(W.dev, ln_tau_pfrt, (size_t)np * sizeof(double), st));
    TRY(upload(W.dfs, W.comb.data(), (size_t)B * sizeof(int), st));
    TRY(upload(W.dlnf, lnf.data(), (size_t)S * sizeof(double), st));
    HIPDRT_CHECK(W.dbad.alloc((size_t)B * sizeof(int)));
    HIPDRT_CHECK(hipMemsetAsync(W.dbad.p, 0, (size_t)B * sizeof(int), st));
    HIPDRT_CHECK(dnorm0.alloc((size_t)B * sizeof(double)));
    HIPDRT_CHECK(dsg.alloc(bn * sizeof(int))); HIPDRT_CHECK(dht.alloc(bn * sizeof(double))); HIPDRT_CHECK(dpr.alloc(bn * sizeof(double)));
    HIPDRT_CHECK(W.dstep.alloc((size_t)S * bn * sizeof(double)));
    HIPDRT_CHECK(dE.alloc((size_t)2 * np * width * sizeof(double)));
    HIPDRT_CHECK(hipStreamSynchronize(st));          // (the host vectors above may go out of use)
    const int orders[2] = {2, 0};
    PredictTimer& tm = W.tm.emplace(p->ctx, st);
    for (int i = 0; i < S; ++i) {
        // step P = calculate_pq with the step's s / rho and the raw re-estimated weights (drt1d.py:2611-2632)
        TRY(step_weights(p, i, st, dw, dscratch));
        const PostSource src = step_source(p, i, dw.d(), W.dfs.i());
        // f and fxx normalised by the R_p of the step's own x; sigma^2 of both orders from one factorisation of the step P
        DrtRows R;
        TRY(R.begin(p, W.dev.d(), dE, np, 2));
        TRY(plan_drt_rows_dev(p, src, pb, orders, 1, 1, nullptr, true, st, R, tm, i > 0));
        // ... but every step's variances are divided by the squared R_p of the FIRST step (estimate_distribution_cov takes
        // get_drt_norm() of fit_parameters, which the warm restarts never update: drt1d.py:3081)
        if (i == 0) HIPDRT_CHECK(hipMemcpyAsync(dnorm0.p, R.dnorm.p, (size_t)B * sizeof(double), hipMemcpyDeviceToDevice, st));
        PeakArgs pa{};
        peak_args_rows(pa, R, po, true, false, W.dfs.i());
        pa.peak_sign = dsg.i(); pa.heights = dht.d(); pa.prominences = dpr.d();
        TRY(launch_peaks(st, pa, B));
        LAUNCH_OK();
        PfrtStepArgs sa{};
        sa.neval = np; sa.floor = o.fxx_var_floor; sa.ext_left = o.ext_left; sa.ext_right = o.ext_right;
        sa.peak_sign = dsg.i(); sa.heights = dht.d(); sa.prominences = dpr.d(); sa.f = R.mu(1);
        sa.var_fxx = R.var(0); sa.var_f = R.var(1); sa.ldv = R.ldv(); sa.cs = R.cs; sa.norm = dnorm0.d();
        sa.fit_status = W.dfs.i(); sa.var_status = R.dvstat.i(); sa.out = W.dstep.d() + (size_t)i * bn; sa.bad = W.dbad.i();
        TRY(launch_pfrt_step(st, sa, B));
        LAUNCH_OK();
        HIPDRT_CHECK(hipStreamSynchronize(st));      // R's buffers are released at the end of the iteration
    }
    return HIPDRT_OK;
}
// the combination of the steps W holds; sizes, the output grid and the output pointers are the caller's
static PfrtCombineArgs pfrt_combine_of(const hipdrt_plan* p, const hipdrt_pfrt_opts& o, const PfrtSteps& W, int np, int nout) {
    PfrtCombineArgs ca = pfrt_combine_args(o, p->m);
    ca.S = p->pf_steps; ca.np = np; ca.nout = nout; ca.ld_step = (long long)W.bn; ca.ld_sum = p->capacity;
    ca.step_pfrt = W.dstep.d(); ca.rss = p->pf_rss.d(); ca.slw = p->pf_slw.d(); ca.ln_factors = W.dlnf.d();
    ca.ltp = W.dev.d(); ca.fit_status = W.dfs.i(); ca.bad = W.dbad.i();
    return ca;
}

int hipdrt_plan_predict_pfrt(hipdrt_plan* p, const double* factors, const double* ln_tau_pfrt, int neval_pfrt,
                             const double* ln_tau_out, int neval_out, const hipdrt_pfrt_opts* opts, double* pfrt, double* raw_pfrt,
                             double* step_pfrt, double* post_prob, int* status) try {
    const hipdrt_pfrt_opts o = opts_or(opts, hipdrt_pfrt_opts_default);
    const int np = neval_pfrt, nout = neval_out;
    PredictBasis pb;
    hipdrt_peak_opts po;
    // every check comes before the first launch
    TRY(pfrt_request(p, factors, ln_tau_pfrt, o, np, nout, pb, po));
    HIPDRT_REQUIRE(!o.smooth || ln_tau_out, "smoothing needs the output grid");
    const int S = p->pf_steps, B = p->B;
    hipStream_t st; TRY(enter(p->ctx, &st));
    DevBuf dout_grid;
    if (o.smooth) TRY(upload(dout_grid, ln_tau_out, (size_t)nout * sizeof(double), st));
    PfrtSteps W;
    TRY(pfrt_steps_dev(p, pb, o, po, factors, ln_tau_pfrt, np, st, W));
    PfrtCombineArgs ca = pfrt_combine_of(p, o, W, np, nout);
    ca.lto = dout_grid.d();
    DevOuts outs;
    TRY(outs.want(pfrt, (size_t)B * nout, ca.pfrt)); TRY(outs.want(raw_pfrt, W.bn, ca.raw)); TRY(outs.want(post_prob, (size_t)S * B, ca.post));
    TRY(launch_pfrt_combine(st, ca, B));
    LAUNCH_OK();
    W.tm->mark();
    TRY(outs.back(st));
    // (the steps' rows are formed whatever the caller asked for: the combination reads them)
    if (step_pfrt) HIPDRT_CHECK(hipMemcpyAsync(step_pfrt, W.dstep.p, W.dstep.bytes, hipMemcpyDeviceToHost, st));
    std::vector<int> hbad(B, 0);
    HIPDRT_CHECK(hipMemcpyAsync(hbad.data(), W.dbad.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    if (status) merge_status(B, W.comb.data(), hbad.data(), status);
    return HIPDRT_OK;
} HIPDRT_CATCH

// ---- DRT.select_pfrt_candidates on the device (pfrt_select_kernel, csrc/pfrt.hip) -------------------------------------------------
void hipdrt_pfrt_select_opts_default(hipdrt_pfrt_select_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->start_thresh = 0.99; o->end_thresh = 0.01; o->peak_thresh = 1e-6; o->max_peaks = 16;
}

int hipdrt_plan_pfrt_select(hipdrt_plan* p, const double* factors, const double* ln_tau_pfrt, int neval_pfrt,
                            const hipdrt_pfrt_opts* opts, const hipdrt_pfrt_select_opts* sel, hipdrt_pfrt_select_out* out,
                            int* status) try {
    HIPDRT_REQUIRE(out, "NULL pointer");
    const hipdrt_pfrt_opts of = opts_or(opts, hipdrt_pfrt_opts_default);      // as given: the finished row out->pfrt
    hipdrt_pfrt_opts o = of;
    o.smooth = 0; o.integrate = 0; o.normalize = 0;          // upstream selects on the raw PFRT
    const hipdrt_pfrt_select_opts so = opts_or(sel, hipdrt_pfrt_select_opts_default);
    const int np = neval_pfrt, nout = so.neval_out;
    PredictBasis pb;
    hipdrt_peak_opts po;
    // every check comes before the first launch
    TRY(pfrt_request(p, factors, ln_tau_pfrt, o, np, np, pb, po));
    TRY(pfrt_select_check(so));
    if (out->pfrt) {
        TRY(pfrt_check(of, p->pf_steps, np, nout));
        HIPDRT_REQUIRE(!of.smooth || so.ln_tau_out, "smoothing needs the output grid");
    }
    const int S = p->pf_steps, B = p->B, mp = so.max_peaks;
    hipStream_t st; TRY(enter(p->ctx, &st));
    PfrtSteps W;
    TRY(pfrt_steps_dev(p, pb, o, po, factors, ln_tau_pfrt, np, st, W));
    PfrtCombineArgs ca = pfrt_combine_of(p, o, W, np, np);
    DevOuts outs;
    TRY(outs.want(out->raw_pfrt, W.bn, ca.raw, true)); TRY(outs.want(out->post_prob, (size_t)S * B, ca.post));
    TRY(launch_pfrt_combine(st, ca, B));
    LAUNCH_OK();
    PfrtSelectArgs sa{};
    sa.S = S; sa.np = np; sa.max_peaks = mp; sa.ld_step = ca.ld_step; sa.ld_sum = ca.ld_sum;
    sa.raw = ca.raw; sa.step_pfrt = ca.step_pfrt; sa.rss = ca.rss; sa.slw = ca.slw;
    sa.c = ca.c; sa.alpha_n = ca.alpha_n; sa.beta_0 = ca.beta_0;
    sa.start_thresh = so.start_thresh; sa.end_thresh = so.end_thresh; sa.peak_thresh = so.peak_thresh;
    sa.fit_status = W.dfs.i(); sa.bad = W.dbad.i();
    const size_t bm = (size_t)B * mp;
    int* dsel = nullptr;
    TRY(outs.want(out->num_peaks, (size_t)B, sa.num_peaks)); TRY(outs.want(out->ranked_index, bm, sa.ranked_index));
    TRY(outs.want(out->first, (size_t)B, sa.first)); TRY(outs.want(out->num_candidates, (size_t)B, sa.num_candidates));
    TRY(outs.want(out->step_index, bm, sa.step_index)); TRY(outs.want(out->magnitude, bm, sa.magnitude));
    TRY(outs.want(out->match_quality, bm, sa.match_quality));
    std::vector<int> hsel(B, 0), hbad(B, 0);
    TRY(outs.want(hsel.data(), (size_t)B, dsel));
    sa.status = dsel;
    TRY(launch_pfrt_select(st, sa, B));
    LAUNCH_OK();
    // the finished row: the combination once more with the caller's smoothing, integration and normalisation
    DevBuf dout_grid;
    if (out->pfrt) {
        if (of.smooth) TRY(upload(dout_grid, so.ln_tau_out, (size_t)nout * sizeof(double), st));
        PfrtCombineArgs cf = pfrt_combine_of(p, of, W, np, nout);
        cf.lto = dout_grid.d();
        TRY(outs.want(out->pfrt, (size_t)B * nout, cf.pfrt));
        TRY(launch_pfrt_combine(st, cf, B));
        LAUNCH_OK();
    }
    W.tm->mark();
    TRY(outs.back(st));
    if (out->step_pfrt) HIPDRT_CHECK(hipMemcpyAsync(out->step_pfrt, W.dstep.p, W.dstep.bytes, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(hbad.data(), W.dbad.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    if (status) {
        merge_status(B, W.comb.data(), hbad.data(), status);
        // a live row's own outcome (no peak, too many peaks) goes before a non-negative fit status
        for (int b = 0; b < B; ++b) if (status[b] >= 0 && hsel[b] != 0) status[b] = hsel[b];
    }
    return HIPDRT_OK;
} HIPDRT_CATCH

// ---- candidate models of the fitted batch (csrc/candidates.hip) -------------------------------------------------------------------
int hipdrt_plan_score_candidates(hipdrt_plan* p, const hipdrt_candidates_in* in, hipdrt_candidates_out* out) try {
    HIPDRT_REQUIRE(p && in && out, "NULL pointer");
    HIPDRT_REQUIRE(p->B >= 1 && p->prepped, "no fitted batch in the plan");
    // every check comes before the first launch
    const bool steps = in->source == HIPDRT_CANDIDATES_FROM_STEPS;
    HIPDRT_REQUIRE(steps || in->source == HIPDRT_CANDIDATES_FROM_HOST, "source must be 0 (recorded steps) or 1 (host array)");
    const int B = p->B, n = p->n, m = p->m, width = n - p->ns;
    int C = in->C;
    if (steps) {
        HIPDRT_REQUIRE(p->pf_steps >= 1, "no recorded steps in the plan (hipdrt_plan_pfrt_begin / _record around the fit's steps)");
        HIPDRT_REQUIRE(C == 0 || C == p->pf_steps, "C must be 0 or the number of recorded steps");
        C = p->pf_steps;
    } else {
        HIPDRT_REQUIRE(in->x, "source 1 needs x");
        HIPDRT_REQUIRE(C >= 1 && C <= 4096, "1 <= C <= 4096");
    }
    HIPDRT_REQUIRE(B <= 65535, "candidates: at most 65535 spectra per call");
    if (in->ncand) for (int b = 0; b < B; ++b) HIPDRT_REQUIRE(in->ncand[b] >= 0 && in->ncand[b] <= C, "ncand: 0 <= ncand[b] <= C");
    const bool want_llh = out->rss || out->sum_log_w;
    const bool want_peaks = out->count || out->peak_index || out->heights || out->prominences;
    const int nfind = in->nfind, mp = in->max_peaks == 0 ? 16 : in->max_peaks;
    hipdrt_peak_opts o = opts_or(in->peak_opts, hipdrt_peak_opts_default);
    PredictBasis pb{};
    if (want_peaks) {
        HIPDRT_REQUIRE(in->ln_tau_find && nfind >= 1, "the peak outputs need the find grid");
        HIPDRT_REQUIRE(mp >= 1 && mp <= 64, "1 <= max_peaks <= 64");
        TRY(predict_basis(p, pb));
        TRY(peak_check_opts(o, nfind));
        HIPDRT_REQUIRE(o.method == 0, "method must be 0 ('thresh'): 'prob' needs a P matrix per candidate");
        TRY(drt_check_request(pb, o.eval_sign, o.normalize, nullptr, "eval_sign"));
        HIPDRT_REQUIRE(peaks_lds_bytes(nfind, 0, o.search == 0, 0) <= kLdsLimit, "find_peaks: nfind too large for one workgroup's LDS");
    }
    const int form = cand_llh_form(p->ctx, m);
    HIPDRT_REQUIRE(!want_llh || form == 1 || cand_llh_fits_lds(m), "candidates: 16 rows of m doubles do not fit in LDS; use the scratch form");
    hipStream_t st; TRY(enter(p->ctx, &st));

    // status of every slot: the live fit's status where that is negative; else HIPDRT_CANDIDATE_ABSENT at or past ncand[b]; else
    // the live status (uploaded candidates) or the status recorded with the step -- a step that failed for a spectrum is no
    // candidate of it, whatever later steps did
    std::vector<int> hs(B), slot((size_t)C * B);
    HIPDRT_CHECK(hipMemcpyAsync(hs.data(), p->fit_status.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    if (steps)
        for (int c = 0; c < C; ++c)
            HIPDRT_CHECK(hipMemcpyAsync(slot.data() + (size_t)c * B, p->pf_status.i() + p->pf_layout().scalar(c), (size_t)B * sizeof(int),
                                        hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    for (int c = 0; c < C; ++c)
        for (int b = 0; b < B; ++b) {
            int& v = slot[(size_t)c * B + b];
            if (hs[b] < 0) v = hs[b];
            else if (in->ncand && c >= in->ncand[b]) v = HIPDRT_CANDIDATE_ABSENT;
            else if (!steps) v = hs[b];
        }

    DevBuf dx, dnc, dslot, dscr;
    const double* x = nullptr;
    long long cstride = 0;
    if (steps) {
        x = p->pf_x.d(); cstride = (long long)p->pf_layout().x(1);
    } else {
        TRY(upload(dx, in->x, (size_t)C * B * n * sizeof(double), st));
        x = dx.d(); cstride = (long long)B * n;
    }
    if (in->ncand) TRY(upload(dnc, in->ncand, (size_t)B * sizeof(int), st));
    TRY(upload(dslot, slot.data(), slot.size() * sizeof(int), st));
    const size_t cb = (size_t)C * B;
    DevOuts outs;
    CandLlhArgs la{};
    TRY(outs.want(out->rss, cb, la.rss, want_llh)); TRY(outs.want(out->sum_log_w, cb, la.slw, want_llh));
    int *d_count = nullptr, *d_index = nullptr, *d_status = nullptr;
    double *d_heights = nullptr, *d_prom = nullptr;
    TRY(outs.want(out->count, cb, d_count)); TRY(outs.want(out->peak_index, cb * mp, d_index));
    TRY(outs.want(out->heights, cb * mp, d_heights)); TRY(outs.want(out->prominences, cb * mp, d_prom));
    TRY(outs.want(want_peaks ? out->status : nullptr, cb, d_status));
    PredictTimer tm(p->ctx, st);
    if (want_llh) {
        if (form == 1) HIPDRT_CHECK(dscr.alloc(cand_llh_scratch_doubles(C, B, m) * sizeof(double)));
        la.C = C; la.B = B; la.m = m; la.n = n; la.x = x; la.x_cstride = cstride; la.x_bstride = n;
        la.rm = p->rm.d(); la.ldrm = p->ldrm; la.rm_stride = p->rm_stride; la.rv = p->rv.d(); la.vmm = p->vmm.d();
        la.var_floor = p->var_floor.d(); la.ncand = in->ncand ? dnc.i() : nullptr; la.fit_status = p->fit_status.i();
        la.slot_status = dslot.i(); la.scratch = dscr.d();
        TRY(launch_cand_llh(st, la, form));
        LAUNCH_OK();
    }
    if (want_peaks) {
        const bool need_f = o.search == 0;
        const int orders[2] = {2, 0}, norders = need_f ? 2 : 1;
        const size_t bn = (size_t)B * nfind;
        DevBuf dev, dE, dkeep, dht, dpr;
        TRY(upload(dev, in->ln_tau_find, (size_t)nfind * sizeof(double), st));
        HIPDRT_CHECK(dE.alloc((size_t)norders * nfind * width * sizeof(double)));
        HIPDRT_CHECK(dkeep.alloc(bn * sizeof(int))); HIPDRT_CHECK(dht.alloc(bn * sizeof(double))); HIPDRT_CHECK(dpr.alloc(bn * sizeof(double)));
        // one set of row buffers for all candidates: the launches of candidate c + 1 follow those of candidate c on the stream
        DrtRows R;
        TRY(R.begin(p, dev.d(), dE, nfind, norders));
        for (int c = 0; c < C; ++c) {
            // the rows of candidate c of every spectrum, normalised by the R_p of the candidate's own x; a slot without a
            // candidate is a dead spectrum to every kernel of the chain
            const int* sl = dslot.i() + (size_t)c * B;
            const PostSource src{x + (size_t)c * cstride, nullptr, nullptr, nullptr, nullptr, sl};
            TRY(plan_drt_rows_dev(p, src, pb, orders, o.eval_sign, o.normalize, nullptr, false, st, R, tm, c > 0));
            PeakArgs pa{};
            peak_args_rows(pa, R, o, need_f, false, sl);
            pa.keep = dkeep.i(); pa.heights = dht.d(); pa.prominences = dpr.d();
            TRY(launch_peaks(st, pa, B));
            LAUNCH_OK();
            CandPeakArgs ca{};
            ca.B = B; ca.neval = nfind; ca.max_peaks = mp; ca.keep = dkeep.i(); ca.dense_heights = dht.d(); ca.dense_prominences = dpr.d();
            ca.slot_status = sl;
            ca.count = d_count ? d_count + (size_t)c * B : nullptr; ca.status = d_status ? d_status + (size_t)c * B : nullptr;
            ca.peak_index = d_index ? d_index + (size_t)c * B * mp : nullptr;
            ca.heights = d_heights ? d_heights + (size_t)c * B * mp : nullptr;
            ca.prominences = d_prom ? d_prom + (size_t)c * B * mp : nullptr;
            launch_cand_compact(st, ca);
            LAUNCH_OK();
        }
        tm.mark();
        TRY(outs.back(st));
        HIPDRT_CHECK(hipStreamSynchronize(st));          // (the row buffers are released at the end of this block)
    } else {
        tm.mark();
        TRY(outs.back(st));
        HIPDRT_CHECK(hipStreamSynchronize(st));
    }
    if (out->status && !want_peaks) std::memcpy(out->status, slot.data(), cb * sizeof(int));
    return HIPDRT_OK;
} HIPDRT_CATCH

}  // extern "C"
