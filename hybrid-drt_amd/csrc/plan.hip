// The plan (include/hipdrt.h): creation, upload and the setters, what is read back from it (matrices, results, history, timings),
// and the one-call hipdrt_fit_eis_batch.  Its device fit loop is plan_fit.hip, what reads a finished fit plan_post.hip and plan_drt.hip.
#include <cmath>
#include <cstring>

#include "plan.hpp"

// ---- the buffers a plan holds once per staged spectrum, sized by its capacity --------------------------------------------
// plan_alloc_batch allocates them, make_view cuts a sub-batch range's windows out of them, hipdrt_plan_bytes_per_spectrum adds
// them up for the map driver.  Buffers that only some plans use (outlier_t, w_eff, wrow, wfac, dop_rho, dop_xmx, vz_entry, the
// history) stay outside the table and are never windowed: a plan which may use a buffer outside the table fits as one range
// (subbatch_count).
struct SpecDims { size_t n, m, nf; int qp_G; };
struct PerSpectrumBuf {
    DevBuf hipdrt_plan::*buf;
    size_t (*bytes)(const SpecDims&);      // per spectrum
    bool lazy;                             // allocated where it is first needed, not by plan_alloc_batch
};
static const PerSpectrumBuf kPerSpectrum[] = {
    {&hipdrt_plan::z_re, [](const SpecDims& d) { return d.nf * sizeof(double); }},
    {&hipdrt_plan::z_im, [](const SpecDims& d) { return d.nf * sizeof(double); }},
    {&hipdrt_plan::rv, [](const SpecDims& d) { return d.m * sizeof(double); }},
    {&hipdrt_plan::w, [](const SpecDims& d) { return d.m * sizeof(double); }},
    {&hipdrt_plan::est_w, [](const SpecDims& d) { return d.m * sizeof(double); }},
    {&hipdrt_plan::x, [](const SpecDims& d) { return d.n * sizeof(double); }},
    {&hipdrt_plan::x_in, [](const SpecDims& d) { return d.n * sizeof(double); }},
    {&hipdrt_plan::q, [](const SpecDims& d) { return d.n * sizeof(double); }},
    {&hipdrt_plan::s, [](const SpecDims& d) { return 3 * d.n * sizeof(double); }},
    {&hipdrt_plan::rho, [](const SpecDims&) { return 3 * sizeof(double); }},
    {&hipdrt_plan::xmx, [](const SpecDims&) { return 3 * sizeof(double); }},
    {&hipdrt_plan::coef_scale, [](const SpecDims&) { return sizeof(double); }},
    {&hipdrt_plan::var_floor, [](const SpecDims&) { return sizeof(double); }},
    {&hipdrt_plan::pcost, [](const SpecDims&) { return sizeof(double); }},
    {&hipdrt_plan::active, [](const SpecDims&) { return sizeof(int); }},
    {&hipdrt_plan::outer_iters, [](const SpecDims&) { return sizeof(int); }},
    {&hipdrt_plan::fit_status, [](const SpecDims&) { return sizeof(int); }},
    {&hipdrt_plan::qp_iters_total, [](const SpecDims&) { return sizeof(int); }},
    {&hipdrt_plan::qp_status, [](const SpecDims&) { return sizeof(int); }},
    {&hipdrt_plan::qp_iters, [](const SpecDims&) { return sizeof(int); }},
    {&hipdrt_plan::L, [](const SpecDims& d) { return qp_scratch_doubles((int)d.n, d.qp_G) * sizeof(double); }},
    {&hipdrt_plan::qpstate, [](const SpecDims& d) { return (d.qp_G > 1 ? d.qp_G : 1) * qp_state_doubles((int)d.n) * sizeof(double); }},
    {&hipdrt_plan::gsync, [](const SpecDims&) { return qp_gsync_ints() * sizeof(int); }},
    {&hipdrt_plan::Ppk, [](const SpecDims& d) { return qp_ppk_doubles((int)d.n) * sizeof(double); }},
    {&hipdrt_plan::order, [](const SpecDims&) { return sizeof(int); }},
    // [3][capacity][m], a range's window its own [3][nb][m]: plan_hyper's batched products, allocated by plan_hyper / hipdrt_plan_fit
    {&hipdrt_plan::premv, [](const SpecDims& d) { return 3 * d.m * sizeof(double); }, true},
};

// (prepared plans have no frequency grid: nf = 0, the impedance buffers keep one entry per spectrum)
static SpecDims spec_dims(const hipdrt_plan* p) {
    return {(size_t)p->n, (size_t)p->m, (size_t)(p->nf > 0 ? p->nf : 1), p->qp_G};
}

namespace hipdrt {
// one range of a plan's staged batch as a plan of its own: spectra [b0, b0 + nb), counter `idx` of n_active_sub
int make_view(hipdrt_plan* p, hipdrt_subfit& sf, int idx, int b0, int nb) {
    hipdrt_plan& v = sf.view;
    // the parent's context and its settings, but a context of its own: no plans to count, no pool slot held (its stream is
    // borrowed per fit: hipdrt_plan_fit)
    sf.ctx = *p->ctx;
    sf.ctx.plans = 0; sf.ctx.released = false; sf.ctx.pool_idx = -1;
    v.ctx = &sf.ctx;
    static_cast<PlanShape&>(v) = *p;          // dimensions, flags, options: all of it, whatever is added to it later
    v.capacity = nb; v.B = nb; v.subbatches = 1;
    // shared, read-only in the loop
    auto whole = [](DevBuf& d, const DevBuf& s_) { d.alias(s_, 0, s_.bytes); };
    whole(v.freq, p->freq); whole(v.tau, p->tau); whole(v.ln_tau, p->ln_tau); whole(v.wt_re, p->wt_re); whole(v.wt_im, p->wt_im);
    whole(v.lut6, p->lut6); whole(v.a_re, p->a_re); whole(v.a_im, p->a_im); whole(v.cr, p->cr); whole(v.rm, p->rm);
    for (int k = 0; k < 3; ++k) whole(v.mk[k], p->mk[k]);
    whole(v.vmm, p->vmm); whole(v.h, p->h); whole(v.l1, p->l1); whole(v.h_init, p->h_init); whole(v.vmm_base, p->vmm_base);
    whole(v.Ptmp, p->Ptmp);
    // per spectrum: this range's window of every buffer of the table
    const SpecDims d = spec_dims(p);
    for (const PerSpectrumBuf& e : kPerSpectrum) {
        const size_t per = e.bytes(d);
        (v.*e.buf).alias(p->*e.buf, (size_t)b0 * per, (size_t)nb * per);
    }
    v.n_active.alias(p->n_active_sub, (size_t)idx * sizeof(int), sizeof(int));
    return HIPDRT_OK;
}

// history buffers for `rows` outer iterations (grown when a later call asks for more than the first one did)
int plan_hist_reserve(hipdrt_plan* p, int rows) {
    if (rows < 1) rows = 1;
    if (p->hist_b >= 0 && p->hist_cap < rows) {
        p->hist_cap = rows;
        HIPDRT_CHECK(p->hist_x.alloc((size_t)p->hist_cap * p->n * sizeof(double)));
        HIPDRT_CHECK(p->hist_w.alloc((size_t)p->hist_cap * p->m * sizeof(double)));
        HIPDRT_CHECK(p->hist_rho.alloc((size_t)p->hist_cap * 3 * sizeof(double)));
        HIPDRT_CHECK(p->hist_qp.alloc((size_t)(p->hist_cap + 1) * sizeof(int)));
        HIPDRT_CHECK(p->hist_dop_rho.alloc((size_t)p->hist_cap * 3 * sizeof(double)));
    }
    return HIPDRT_OK;
}
}  // namespace hipdrt

extern "C" {

void hipdrt_default_fit_opts(hipdrt_fit_opts* o) {
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->rp_scale = 14;
    const double dw[3] = {1.5, 1.0, 0.5}, sd[3] = {1, 1000, 1000}, sa[3] = {5, 10, 25}, ra[3] = {0.15, 0.2, 0.25};
    for (int k = 0; k < 3; ++k) {
        o->derivative_weights[k] = dw[k]; o->sigma_ds[k] = sd[k]; o->s_alpha[k] = sa[k]; o->s_0[k] = 1.0;
        o->rho_alpha[k] = ra[k]; o->rho_0[k] = 1.0;
    }
    o->l1_lambda_0 = 0; o->l2_lambda_0 = 142;
    o->iw_l1_lambda_0 = 1e-4; o->iw_l2_lambda_0 = 1e-4;
    o->ohmic_penalty = 1e-6; o->inductance_penalty = 1e-6; o->inductance_scale = 1e-5;
    o->eis_vmm_epsilon = 0.25; o->eis_reim_cor = 0.25;
    o->xtol = 1e-2; o->max_iter = 50; o->nonneg = 1; o->scale_data = 1; o->fit_ohmic = 1; o->fit_inductance = 1;
    o->update_scale = 0; o->eff_hp = 1;
    o->eis_error_uniform = 0;
    o->outlier_p = -1.0; o->iw_alpha = -1.0; o->iw_beta = -1.0;
    o->qp = default_qp_opts();
}

static int plan_build_matrices(hipdrt_plan* p, bool build_lookup) {
    hipStream_t st = p->ctx->stream;
    if (p->mode == HIPDRT_MODE_INTERP && build_lookup) {
        launch_lookup(st, p->eps, p->ngrid, p->ny, p->wt_re.d(), p->wt_im.d(), lut_part(p->lut6.d(), p->ngrid, 0).f,
                      lut_part(p->lut6.d(), p->ngrid, 1).f);
        LAUNCH_OK();
    }
    if (p->mode == HIPDRT_MODE_INTERP) launch_lut_slopes(st, p->lut6.d(), p->ngrid, 2);
    launch_impedance_matrix(st, 1, 0, p->freq.d(), p->nf, p->tau.d(), p->ntau, p->mode, p->toeplitz_a, p->eps, p->ngrid,
                            p->lut6.d(), p->ny, p->a_re.d(), p->a_im.d(), p->cr.d());
    LAUNCH_OK();
    FitState fs = p->state();
    launch_assemble_rm(st, fs, p->a_re.d(), p->a_im.d(), p->freq.d(), p->rm.d(), p->idx_rinf, p->idx_induc);
    LAUNCH_OK();
    return 0;
}

// work space for `capacity` spectra
static int plan_alloc_batch(hipdrt_plan* p) {
    const size_t cap = (size_t)p->capacity;
    const int n = p->n, m = p->m;
    p->qp_G = qp_group_size(p->capacity, n, p->ctx->qp_force_group);
    HIPDRT_REQUIRE(p->qp_G >= 0, "n too large for the QP kernels");
    const SpecDims d = spec_dims(p);
    for (const PerSpectrumBuf& e : kPerSpectrum)
        if (!e.lazy) HIPDRT_CHECK((p->*e.buf).alloc(cap * e.bytes(d)));
    HIPDRT_CHECK(p->n_active.alloc(sizeof(int)));
    HIPDRT_CHECK(p->Ptmp.alloc((size_t)n * p->ldp * sizeof(double)));
    if (p->opts.outlier_p > 0.0) {
        HIPDRT_CHECK(p->vmm_base.alloc((size_t)m * m * sizeof(double)));
        HIPDRT_CHECK(p->outlier_t.alloc(cap * m * sizeof(double)));
    }
    HIPDRT_CHECK(p->hist_rows.alloc(sizeof(int)));
    return 0;
}

// Reach of the penalty matrices on a log-uniform grid: the largest distance from the diagonal at which the first row of the DRT
// block of any order is not exactly zero (Gaussian basis: e^(-a^2 / 2) underflows ~39 grid points out at 10 points per decade,
// whatever the matrix size).  The Gram kernel's L2 epilogue skips tiles that lie wholly beyond it.  Once per plan.
static int plan_toep_reach(hipdrt_plan* p) {
    p->toep_maxd = -1;
    if (!p->toeplitz_m) return HIPDRT_OK;
    const int nd = p->n - p->ns;
    std::vector<double> row(nd);
    int reach = 0;
    for (int k = 0; k < 3; ++k) {
        HIPDRT_CHECK(hipMemcpy(row.data(), p->mk[k].d() + (size_t)p->ns * p->ldm + p->ns, (size_t)nd * sizeof(double), hipMemcpyDeviceToHost));
        for (int d = nd - 1; d > reach; --d)
            if (row[d] != 0.0) { reach = d; break; }
    }
    p->toep_maxd = reach;
    // the columns of the special parameters below the special block, and their rows to the right of it
    p->spec_zero = 1;
    if (p->ns > 0) {
        std::vector<double> cols((size_t)nd * p->ns), rows((size_t)p->ns * nd);
        for (int k = 0; k < 3 && p->spec_zero; ++k) {
            HIPDRT_CHECK(hipMemcpy2D(cols.data(), (size_t)p->ns * sizeof(double), p->mk[k].d() + (size_t)p->ns * p->ldm,
                                     (size_t)p->ldm * sizeof(double), (size_t)p->ns * sizeof(double), nd, hipMemcpyDeviceToHost));
            HIPDRT_CHECK(hipMemcpy2D(rows.data(), (size_t)nd * sizeof(double), p->mk[k].d() + p->ns, (size_t)p->ldm * sizeof(double),
                                     (size_t)nd * sizeof(double), p->ns, hipMemcpyDeviceToHost));
            for (double v : cols) if (v != 0.0) { p->spec_zero = 0; break; }
            for (double v : rows) if (v != 0.0) { p->spec_zero = 0; break; }
        }
    }
    return HIPDRT_OK;
}

int hipdrt_plan_create(hipdrt_ctx* ctx, const double* freq, int nf, const double* tau, int ntau, double epsilon,
                       int mode, int toeplitz_a, int toeplitz_m, int ngrid, int ny, const double* wt_re,
                       const double* wt_im, const double* log_wt_re, const double* log_wt_im,
                       const hipdrt_fit_opts* opts, int capacity, hipdrt_plan** out) try {
    HIPDRT_REQUIRE(ctx && freq && tau && out, "NULL pointer");
    HIPDRT_REQUIRE(nf >= 2 && ntau >= 2 && capacity >= 1, "nf, ntau >= 2, capacity >= 1");
    HIPDRT_REQUIRE(mode == HIPDRT_MODE_INTERP || mode == HIPDRT_MODE_TRAPZ, "mode");
    if (mode == HIPDRT_MODE_INTERP)
        HIPDRT_REQUIRE(wt_re && wt_im && log_wt_re && log_wt_im && impedance_ngrid_ok(ngrid), "interp lookups");
    HIPDRT_REQUIRE(ny_ok(ny), "2 <= ny <= 6000");
    hipStream_t st; TRY(enter(ctx, &st));
    std::unique_ptr<hipdrt_plan> p(new hipdrt_plan());
    p->ctx = ctx;
    p->opts = opts_or(opts, hipdrt_default_fit_opts);
    p->nf = nf; p->ntau = ntau; p->eps = epsilon; p->mode = mode; p->ngrid = ngrid; p->ny = ny;
    p->toeplitz_a = toeplitz_a; p->toeplitz_m = toeplitz_m; p->capacity = capacity;
    // special parameters in registration order (drt1d.py:383-388): R_inf, then inductance
    int ns = 0;
    if (p->opts.fit_ohmic) p->idx_rinf = ns++;
    if (p->opts.fit_inductance) p->idx_induc = ns++;
    p->ns = ns; p->n = ns + ntau; p->m = 2 * nf;
    const int n = p->n, m = p->m;
    HIPDRT_REQUIRE(n <= 4096, "ns + ntau <= 4096");
    p->ldrm = round_up(n, 2); p->ldm = round_up(n, 2); p->ldp = round_up(n, 2); p->ldl = (int)qp_scratch_ld(n);

    std::vector<double> ln_tau(ntau);
    for (int i = 0; i < ntau; ++i) ln_tau[i] = std::log(tau[i]);
    TRY(upload(p->freq, freq, (size_t)nf * sizeof(double), st));
    TRY(upload(p->tau, tau, (size_t)ntau * sizeof(double), st));
    p->freq_order = freq_monotone(freq, nf);
    const size_t gb = (size_t)(ngrid > 0 ? ngrid : 1) * sizeof(double);
    if (mode == HIPDRT_MODE_INTERP) {
        TRY(upload(p->wt_re, wt_re, gb, st)); TRY(upload(p->wt_im, wt_im, gb, st));
        TRY(stage_lut(st, p->lut6, ngrid, 2, 0, log_wt_re, nullptr));
        TRY(stage_lut(st, p->lut6, ngrid, 2, 1, log_wt_im, nullptr));
    }
    HIPDRT_CHECK(p->a_re.alloc((size_t)nf * ntau * sizeof(double)));
    HIPDRT_CHECK(p->a_im.alloc((size_t)nf * ntau * sizeof(double)));
    HIPDRT_CHECK(p->cr.alloc(impedance_scratch_doubles(1, 0, nf, ntau, mode, toeplitz_a) * sizeof(double)));
    HIPDRT_CHECK(p->rm.alloc((size_t)m * p->ldrm * sizeof(double)));
    HIPDRT_CHECK(hipMemsetAsync(p->rm.p, 0, p->rm.bytes, st));
    for (int k = 0; k < 3; ++k) {
        HIPDRT_CHECK(p->mk[k].alloc((size_t)n * p->ldm * sizeof(double)));
        HIPDRT_CHECK(hipMemsetAsync(p->mk[k].p, 0, p->mk[k].bytes, st));
    }
    HIPDRT_CHECK(p->vmm.alloc((size_t)m * m * sizeof(double)));
    HIPDRT_CHECK(p->h.alloc((size_t)n * sizeof(double)));
    // l1_lambda_vector: 0 on specials, l1_lambda_0 on DRT coefficients (drt1d.py:552-553)
    std::vector<double> l1(n, 0.0);
    for (int i = ns; i < n; ++i) l1[i] = p->opts.l1_lambda_0;
    TRY(upload(p->l1, l1.data(), (size_t)n * sizeof(double), st));
    // ln(tau) on the host: np.log(self.basis_tau) (drt1d.py:5694)
    TRY(upload(p->ln_tau, ln_tau.data(), (size_t)ntau * sizeof(double), st));
    HIPDRT_CHECK(hipStreamSynchronize(st));   // host vectors above go out of scope

    TRY(plan_alloc_batch(p.get()));

    // shared matrices on the device
    TRY(plan_build_matrices(p.get(), true));
    launch_penalty(st, p->ln_tau.d(), ntau, epsilon, toeplitz_m, p->mk[0].d(), p->mk[1].d(), p->mk[2].d(), p->ldm, ns);
    launch_special_penalty(st, p->mk[0].d(), p->mk[1].d(), p->mk[2].d(), p->ldm, p->idx_rinf, p->idx_induc,
                           p->opts.ohmic_penalty, p->opts.inductance_penalty);
    launch_eis_vmm(st, p->freq.d(), nf, p->opts.eis_vmm_epsilon, p->opts.eis_reim_cor, p->opts.eis_error_uniform,
                   p->vmm.d());
    if (p->vmm_base.p) launch_vmm_exclude_self(st, p->vmm.d(), m, p->vmm_base.d());
    launch_make_h(st, p->h.d(), n, ns, p->opts.nonneg);
    LAUNCH_OK();
    HIPDRT_CHECK(hipStreamSynchronize(st));
    TRY(plan_toep_reach(p.get()));
    { std::lock_guard<std::mutex> lk(g_life); ++ctx->plans; }
    *out = p.release();
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_create_prepared(hipdrt_ctx* ctx, const hipdrt_prepared_desc* d, const double* m0, const double* m1,
                                const double* m2, const double* vmm, const double* h, const double* l1,
                                const double* vz_strength, const hipdrt_fit_opts* opts, int capacity, hipdrt_plan** out) try {
    HIPDRT_REQUIRE(ctx && d && m0 && m1 && m2 && vmm && h && l1 && out, "NULL pointer");
    HIPDRT_REQUIRE(d->m >= 2 && d->n >= 2 && d->ns >= 0 && d->ns < d->n && capacity >= 1, "m, n >= 2, 0 <= ns < n, capacity >= 1");
    HIPDRT_REQUIRE(d->n <= 4096, "n <= 4096");
    HIPDRT_REQUIRE(d->dop_size >= 0 && (d->dop_size == 0 || (d->dop_start >= 0 && d->dop_start + d->dop_size <= d->ns)),
                   "the x_dop block must lie inside the special parameters");
    HIPDRT_REQUIRE(d->dop_size <= d->n - d->ns, "x_dop block larger than the DRT block");
    HIPDRT_REQUIRE(d->vz_index < d->ns && (d->vz_index < 0 || vz_strength), "vz_offset column / strength vector");
    HIPDRT_REQUIRE(d->vb_size >= 0 && d->vb_start >= 0 && d->vb_start + d->vb_size <= d->ns, "v_baseline columns");
    HIPDRT_REQUIRE(d->num_chrono >= 0 && d->num_chrono <= d->m, "num_chrono");
    HIPDRT_REQUIRE(!(opts && opts->update_scale) || d->basis_area > 0.0, "update_scale needs desc.basis_area");
    if (d->init_weights_separately && d->num_chrono > 0 && d->num_chrono < d->m) {
        // stage 2 of init_weights_kernel multiplies the whole of V by the residuals of all rows where the reference takes
        // vmm[sl, sl] (drt1d.py:648-672): the two agree only while no chrono row reads an impedance residual, or the reverse
        const int nc = d->num_chrono;
        for (int i = 0; i < d->m; ++i) {
            const int j0 = i < nc ? nc : 0, j1 = i < nc ? d->m : nc;
            for (int j = j0; j < j1; ++j)
                HIPDRT_REQUIRE(vmm[(size_t)i * d->m + j] == 0.0,
                               "init_weights_separately: vmm must be zero outside its chrono and impedance blocks");
        }
    }
    hipStream_t st; TRY(enter(ctx, &st));
    std::unique_ptr<hipdrt_plan> p(new hipdrt_plan());
    p->ctx = ctx;
    p->opts = opts_or(opts, hipdrt_default_fit_opts);
    p->prepared = 1; p->desc = *d;
    p->n = d->n; p->m = d->m; p->ns = d->ns; p->ntau = d->n - d->ns; p->nf = 0; p->toeplitz_m = d->toeplitz_m;
    p->capacity = capacity;
    const int n = p->n, m = p->m;
    p->ldrm = round_up(n, 2); p->ldm = round_up(n, 2); p->ldp = round_up(n, 2); p->ldl = (int)qp_scratch_ld(n);
    const double* mk[3] = {m0, m1, m2};
    for (int k = 0; k < 3; ++k) {
        HIPDRT_CHECK(p->mk[k].alloc((size_t)n * p->ldm * sizeof(double)));
        HIPDRT_CHECK(hipMemsetAsync(p->mk[k].p, 0, p->mk[k].bytes, st));
        HIPDRT_CHECK(hipMemcpy2DAsync(p->mk[k].p, (size_t)p->ldm * sizeof(double), mk[k], (size_t)n * sizeof(double),
                                      (size_t)n * sizeof(double), n, hipMemcpyHostToDevice, st));
    }
    TRY(upload(p->vmm, vmm, (size_t)m * m * sizeof(double), st));
    TRY(upload(p->h, h, (size_t)n * sizeof(double), st));
    TRY(upload(p->l1, l1, (size_t)n * sizeof(double), st));
    if (vz_strength) TRY(upload(p->vz_strength, vz_strength, (size_t)m * sizeof(double), st));
    TRY(plan_alloc_batch(p.get()));
    if (p->vmm_base.p) launch_vmm_exclude_self(st, p->vmm.d(), m, p->vmm_base.d());     // outlier_p: qphb.py:1644-1648
    HIPDRT_CHECK(p->dop_rho.alloc((size_t)capacity * 3 * sizeof(double)));
    HIPDRT_CHECK(p->dop_xmx.alloc((size_t)capacity * 3 * sizeof(double)));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    TRY(plan_toep_reach(p.get()));
    { std::lock_guard<std::mutex> lk(g_life); ++ctx->plans; }
    *out = p.release();
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_upload_prepared(hipdrt_plan* p, int B, int rm_batched, const double* rzm, const double* rzv) try {
    HIPDRT_REQUIRE(p && rzm && rzv, "NULL pointer");
    HIPDRT_REQUIRE(p->prepared, "not a prepared plan");
    HIPDRT_REQUIRE(B >= 1 && B <= p->capacity, "1 <= B <= capacity");
    HIPDRT_REQUIRE(rm_batched || p->desc.vz_index < 0, "a vz_offset column needs one response matrix per measurement");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const int n = p->n, m = p->m;
    const size_t nmat = rm_batched ? (size_t)B : 1;
    const size_t need = nmat * m * p->ldrm * sizeof(double);
    if (p->rm.bytes < need) HIPDRT_CHECK(p->rm.alloc(need));
    HIPDRT_CHECK(hipMemsetAsync(p->rm.p, 0, need, st));
    HIPDRT_CHECK(hipMemcpy2DAsync(p->rm.p, (size_t)p->ldrm * sizeof(double), rzm, (size_t)n * sizeof(double),
                                  (size_t)n * sizeof(double), nmat * m, hipMemcpyHostToDevice, st));
    HIPDRT_CHECK(hipMemcpyAsync(p->rv.p, rzv, (size_t)B * m * sizeof(double), hipMemcpyHostToDevice, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    p->rm_stride = rm_batched ? (long long)m * p->ldrm : 0;
    p->B = B;
    p->prepped = 0;
    p->pf_steps = 0;            // (recorded PFRT steps belong to the batch they were fitted on)
    p->pd_set = 0;              // (so do the post-fit scales of the prediction description)
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_set_weight_factors(hipdrt_plan* p, double weight_factor, const double* row_factors, int batched) try {
    HIPDRT_REQUIRE(p, "plan is NULL");
    HIPDRT_REQUIRE(weight_factor > 0.0, "weight_factor > 0");
    hipStream_t st; TRY(enter(p->ctx, &st));
    p->weight_factor = weight_factor;
    p->wrow_batched = (batched & 1) ? 1 : 0;
    p->wrow_late = (batched & 2) ? 1 : 0;
    if (row_factors) {
        const size_t cnt = ((batched & 1) ? (size_t)p->capacity : 1) * p->m;   // bit 1 (late) does not make it per spectrum
        TRY(upload(p->wrow, row_factors, cnt * sizeof(double), st));
    } else {
        p->wrow.release();
    }
    if (p->has_weight_factors() && !p->w_eff.p) HIPDRT_CHECK(p->w_eff.alloc((size_t)p->capacity * p->m * sizeof(double)));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_set_init_h(hipdrt_plan* p, const double* h_init) try {
    HIPDRT_REQUIRE(p, "plan is NULL");
    TRY(enter(p->ctx));
    if (!h_init) { p->h_init.release(); return HIPDRT_OK; }
    TRY(upload(p->h_init, h_init, (size_t)p->n * sizeof(double), p->ctx->stream));
    HIPDRT_CHECK(hipStreamSynchronize(p->ctx->stream));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_destroy(hipdrt_plan* plan) try {
    if (!plan) return HIPDRT_OK;
    std::lock_guard<std::mutex> lk(g_life);
    hipdrt_ctx* ctx = plan->ctx;
    (void)hipSetDevice(ctx->device);
    delete plan;
    if (--ctx->plans == 0 && ctx->released) free_ctx(ctx);
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_dims(hipdrt_plan* plan, int* n, int* m, int* ns) try {
    HIPDRT_REQUIRE(plan, "plan is NULL");
    if (n) *n = plan->n;
    if (m) *m = plan->m;
    if (ns) *ns = plan->ns;
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_get(hipdrt_plan* p, const char* which, double* out, long long count) try {
    HIPDRT_REQUIRE(p && which && out, "NULL pointer");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const std::string w = which;
    const double* src = nullptr; int rows = 0, cols = 0, ld = 0;
    if (w == "lut_z_re") { src = lut_part(p->lut6.d(), p->ngrid, 0).f; rows = 1; cols = ld = p->ngrid; }
    else if (w == "lut_z_im") { src = lut_part(p->lut6.d(), p->ngrid, 1).f; rows = 1; cols = ld = p->ngrid; }
    else if (w == "a_re") { src = p->a_re.d(); rows = p->nf; cols = ld = p->ntau; }
    else if (w == "a_im") { src = p->a_im.d(); rows = p->nf; cols = ld = p->ntau; }
    else if (w == "rm") { src = p->rm.d(); rows = p->m; cols = p->n; ld = p->ldrm; }
    else if (w == "m0" || w == "m1" || w == "m2") { src = p->mk[w[1] - '0'].d(); rows = cols = p->n; ld = p->ldm; }
    else if (w == "vmm") { src = p->vmm.d(); rows = cols = ld = p->m; }
    else if (w == "h") { src = p->h.d(); rows = 1; cols = ld = p->n; }
    else if (w == "est_weights") { src = p->est_w.d(); rows = p->B; cols = ld = p->m; }   // per spectrum of the last batch
    else if (w == "rv") { src = p->rv.d(); rows = p->B; cols = ld = p->m; }
    else if (w == "xmx") { src = p->xmx.d(); rows = p->B; cols = ld = 3; }
    else if (w == "outlier_t" && p->outlier_t.p) { src = p->outlier_t.d(); rows = p->B; cols = ld = p->m; }
    else if (w == "weight_factors" && p->wfac.p) { src = p->wfac.d(); rows = p->B; cols = ld = 2; }
    else if (w == "row_factors" && p->wrow.p && p->wrow_batched) { src = p->wrow.d(); rows = p->B; cols = ld = p->m; }   // [B][m]
    else if (w == "x") { src = p->x.d(); rows = p->B; cols = ld = p->n; }
    else if (w == "coef_scale") { src = p->coef_scale.d(); rows = p->B; cols = ld = 1; }
    else if (w == "var_floor") { src = p->var_floor.d(); rows = p->B; cols = ld = 1; }
    else if (w == "dop_rho" && p->prepared) { src = p->dop_rho.d(); rows = p->B; cols = ld = 3; }
    else if (w == "dop_xmx" && p->prepared) { src = p->dop_xmx.d(); rows = p->B; cols = ld = 3; }
    else if (w == "rzm") { src = p->rm.d(); rows = (p->rm_stride ? p->B : 1) * p->m; cols = p->n; ld = p->ldrm; }
    else if (w == "hist_dop_rho" && p->prepared && p->hist_b >= 0) { src = p->hist_dop_rho.d(); rows = p->hist_cap; cols = ld = 3; }
    else { set_error("unknown matrix name: " + w); return HIPDRT_E_INVALID; }
    HIPDRT_REQUIRE(src != nullptr, "matrix not available in this mode");
    HIPDRT_REQUIRE(count == (long long)rows * cols, "count does not match the matrix size");
    return copy_strided(out, src, rows, cols, ld, st);
} HIPDRT_CATCH

int hipdrt_plan_set_lookup(hipdrt_plan* p, const double* z_re, const double* z_im) try {
    HIPDRT_REQUIRE(p && z_re && z_im, "NULL pointer");
    HIPDRT_REQUIRE(p->mode == HIPDRT_MODE_INTERP, "plan is not in interp mode");
    hipStream_t st; TRY(enter(p->ctx, &st));
    TRY(stage_lut(st, p->lut6, p->ngrid, 2, 0, nullptr, z_re));
    TRY(stage_lut(st, p->lut6, p->ngrid, 2, 1, nullptr, z_im));
    TRY(plan_build_matrices(p, false));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_upload(hipdrt_plan* p, int B, const double* z_re, const double* z_im) try {
    HIPDRT_REQUIRE(p && z_re && z_im, "NULL pointer");
    HIPDRT_REQUIRE(!p->prepared, "prepared plans take hipdrt_plan_upload_prepared");
    HIPDRT_REQUIRE(B >= 1 && B <= p->capacity, "1 <= B <= capacity");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const size_t bytes = (size_t)B * p->nf * sizeof(double);
    HIPDRT_CHECK(hipMemcpyAsync(p->z_re.p, z_re, bytes, hipMemcpyHostToDevice, st));
    HIPDRT_CHECK(hipMemcpyAsync(p->z_im.p, z_im, bytes, hipMemcpyHostToDevice, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    p->B = B;
    p->pf_steps = 0;            // (recorded PFRT steps belong to the batch they were fitted on)
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_set_state(hipdrt_plan* p, const double* x, const double* rho, const double* s, const double* weights) try {
    HIPDRT_REQUIRE(p, "plan is NULL");
    HIPDRT_REQUIRE(p->B >= 1, "no fitted batch in the plan");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const size_t B = p->B, n = p->n, m = p->m;
    if (x) {
        HIPDRT_CHECK(hipMemcpyAsync(p->x.p, x, B * n * sizeof(double), hipMemcpyHostToDevice, st));
        HIPDRT_CHECK(hipMemcpyAsync(p->x_in.p, x, B * n * sizeof(double), hipMemcpyHostToDevice, st));
    }
    if (rho) HIPDRT_CHECK(hipMemcpyAsync(p->rho.p, rho, B * 3 * sizeof(double), hipMemcpyHostToDevice, st));
    if (s) HIPDRT_CHECK(hipMemcpyAsync(p->s.p, s, B * 3 * n * sizeof(double), hipMemcpyHostToDevice, st));
    if (weights) HIPDRT_CHECK(hipMemcpyAsync(p->w.p, weights, B * m * sizeof(double), hipMemcpyHostToDevice, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_set_state_dop(hipdrt_plan* p, const double* dop_rho) try {
    HIPDRT_REQUIRE(p && dop_rho, "NULL pointer");
    HIPDRT_REQUIRE(p->prepared && p->desc.dop_size > 0, "the plan has no distribution of phasances");
    HIPDRT_REQUIRE(p->B >= 1, "no fitted batch in the plan");
    TRY(enter(p->ctx));
    HIPDRT_CHECK(hipMemcpyAsync(p->dop_rho.p, dop_rho, (size_t)p->B * 3 * sizeof(double), hipMemcpyHostToDevice, p->ctx->stream));
    HIPDRT_CHECK(hipStreamSynchronize(p->ctx->stream));
    return HIPDRT_OK;
} HIPDRT_CATCH

// device bytes one more staged spectrum costs an EIS plan (the per-spectrum buffers plan_alloc_batch and hipdrt_plan_fit size
// by the capacity, batch coneqp kernel): what a map driver divides the device's memory by before it forms its batches
int hipdrt_plan_bytes_per_spectrum(int nf, int ntau, int ns, long long* bytes) try {
    HIPDRT_REQUIRE(bytes && nf >= 1 && ntau >= 1 && ns >= 0, "arguments");
    const SpecDims d{(size_t)ntau + ns, 2 * (size_t)nf, (size_t)nf, 0};
    size_t b = 0;
    for (const PerSpectrumBuf& e : kPerSpectrum) b += e.bytes(d);
    *bytes = (long long)b;
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_set_subbatches(hipdrt_plan* p, int k) try {
    HIPDRT_REQUIRE(p, "plan is NULL");
    HIPDRT_REQUIRE(k >= 0 && k <= 16, "0 (automatic) <= k <= 16");
    p->subbatches = k;
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_record_history(hipdrt_plan* p, int b) try {
    HIPDRT_REQUIRE(p, "plan is NULL");
    TRY(enter(p->ctx));
    p->hist_b = b;
    return plan_hist_reserve(p, p->opts.max_iter);
} HIPDRT_CATCH

int hipdrt_plan_get_history(hipdrt_plan* p, double* hist_x, double* hist_rho, double* hist_w, int* qp_iters,
                            int max_rows, int* rows) try {
    HIPDRT_REQUIRE(p && rows, "NULL pointer");
    HIPDRT_REQUIRE(p->hist_b >= 0 && p->hist_cap > 0, "history recording was not enabled");
    TRY(enter(p->ctx));
    int r = 0;
    HIPDRT_CHECK(hipMemcpy(&r, p->hist_rows.p, sizeof(int), hipMemcpyDeviceToHost));
    if (r > max_rows) r = max_rows;
    *rows = r;
    if (hist_x) HIPDRT_CHECK(hipMemcpy(hist_x, p->hist_x.p, (size_t)r * p->n * sizeof(double), hipMemcpyDeviceToHost));
    if (hist_w) HIPDRT_CHECK(hipMemcpy(hist_w, p->hist_w.p, (size_t)r * p->m * sizeof(double), hipMemcpyDeviceToHost));
    if (hist_rho) HIPDRT_CHECK(hipMemcpy(hist_rho, p->hist_rho.p, (size_t)r * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (qp_iters) HIPDRT_CHECK(hipMemcpy(qp_iters, p->hist_qp.p, (size_t)(r + 1) * sizeof(int), hipMemcpyDeviceToHost));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_timings(hipdrt_plan* p, float* t, int* launches) try {
    HIPDRT_REQUIRE(p, "plan is NULL");
    if (t) std::memcpy(t, p->t_ms, sizeof(p->t_ms));
    if (launches) std::memcpy(launches, p->launches, sizeof(p->launches));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_download(hipdrt_plan* p, double* x, double* fit_x, double* r_inf, double* induc, double* weights,
                         double* coef_scale, double* rho, double* s_vectors, double* q_vector, int* outer_iters,
                         int* qp_iters_total, int* status) try {
    HIPDRT_REQUIRE(p, "plan is NULL");
    HIPDRT_REQUIRE(p->B >= 1, "nothing fitted");
    TRY(enter(p->ctx));
    const int B = p->B, n = p->n, m = p->m, ns = p->ns, ntau = p->ntau;
    std::vector<double> hx((size_t)B * n), hcs(B);
    HIPDRT_CHECK(hipMemcpy(hx.data(), p->x.p, hx.size() * sizeof(double), hipMemcpyDeviceToHost));
    HIPDRT_CHECK(hipMemcpy(hcs.data(), p->coef_scale.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost));
    if (x) std::memcpy(x, hx.data(), hx.size() * sizeof(double));
    if (coef_scale) std::memcpy(coef_scale, hcs.data(), (size_t)B * sizeof(double));
    // extract_qphb_parameters (drt1d.py:6228-6289)
    for (int b = 0; b < B; ++b) {
        const double cs = hcs[b];
        const double* xb = hx.data() + (size_t)b * n;
        if (fit_x) for (int i = 0; i < ntau; ++i) fit_x[(size_t)b * ntau + i] = xb[ns + i] * cs;
        if (r_inf) r_inf[b] = p->idx_rinf >= 0 ? xb[p->idx_rinf] * cs : 0.0;
        if (induc) induc[b] = p->idx_induc >= 0 ? xb[p->idx_induc] * (cs * p->opts.inductance_scale) : 0.0;
    }
    if (weights) HIPDRT_CHECK(hipMemcpy(weights, p->w.p, (size_t)B * m * sizeof(double), hipMemcpyDeviceToHost));
    if (rho) HIPDRT_CHECK(hipMemcpy(rho, p->rho.p, (size_t)B * 3 * sizeof(double), hipMemcpyDeviceToHost));
    if (s_vectors) HIPDRT_CHECK(hipMemcpy(s_vectors, p->s.p, (size_t)B * 3 * n * sizeof(double), hipMemcpyDeviceToHost));
    if (q_vector) HIPDRT_CHECK(hipMemcpy(q_vector, p->q.p, (size_t)B * n * sizeof(double), hipMemcpyDeviceToHost));
    if (outer_iters) HIPDRT_CHECK(hipMemcpy(outer_iters, p->outer_iters.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
    if (qp_iters_total) HIPDRT_CHECK(hipMemcpy(qp_iters_total, p->qp_iters_total.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
    if (status) HIPDRT_CHECK(hipMemcpy(status, p->fit_status.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_fit_eis_batch(hipdrt_ctx* ctx, int B, const double* freq, int nf, const double* z_re, const double* z_im,
                         const double* tau, int ntau, double epsilon, int mode, int toeplitz_a, int toeplitz_m,
                         int ngrid, int ny, const double* wt_re, const double* wt_im, const double* log_wt_re,
                         const double* log_wt_im, const hipdrt_fit_opts* opts, double* x, double* fit_x, double* r_inf,
                         double* induc, double* weights, double* coef_scale, double* rho, double* q_vector,
                         int* outer_iters, int* status) try {
    hipdrt_plan* p = nullptr;
    TRY(hipdrt_plan_create(ctx, freq, nf, tau, ntau, epsilon, mode, toeplitz_a, toeplitz_m, ngrid, ny, wt_re, wt_im,
                           log_wt_re, log_wt_im, opts, B, &p));
    int rc = hipdrt_plan_upload(p, B, z_re, z_im);
    if (!rc) rc = hipdrt_plan_fit(p);
    if (!rc) rc = hipdrt_plan_download(p, x, fit_x, r_inf, induc, weights, coef_scale, rho, nullptr, q_vector,
                                       outer_iters, nullptr, status);
    hipdrt_plan_destroy(p);
    return rc;
} HIPDRT_CATCH

}  // extern "C"
