// Model evaluation of a prepared plan (include/hipdrt.h): the prediction description that tells the plan what its special columns
// mean, and the voltage response of every member of its fitted batch (DRT.predict_response, hybdrt/models/drt1d.py:3363-3464) from
// unit-step layers built once for the batch (csrc/matrices.hip), the row-application kernel and response_assemble_kernel
// (csrc/predict.hip); its impedance with every special term, its distribution of phasances (DRT.predict_dop, 3273-3347) and the
// posterior of that distribution (DRT.estimate_dop_cov, 3153-3198; DRT.predict_dop_ci, 3233-3258).
#include <cmath>

#include "plan.hpp"

namespace hipdrt {
int response_chain(hipStream_t st, int B, int ntau, int copies, int ns, const double* U, const double* Ud, const double* Xd,
                   int dop_size, ResponseArgs a, DevBuf& t, DevBuf& tn, DevBuf& td) {
    const int r = a.S * a.nt;
    const size_t tb = (size_t)B * r * sizeof(double);
    a.ldt = r; a.T = a.Tn = a.Td = nullptr;
    if ((a.mask & HIPDRT_INCLUDE_DRT) && U) {
        HIPDRT_CHECK(t.alloc(tb));
        launch_apply_rows(st, B, ntau, a.X, a.ldx, ns, r, U, ntau, a.cs, nullptr, t.d(), r);
        LAUNCH_OK();
        a.T = t.d();
        if (copies == 2) {
            HIPDRT_CHECK(tn.alloc(tb));
            launch_apply_rows(st, B, ntau, a.X, a.ldx, ns + ntau, r, U, ntau, a.cs, nullptr, tn.d(), r);
            LAUNCH_OK();
            a.Tn = tn.d();
        }
    }
    if ((a.mask & HIPDRT_INCLUDE_DOP) && Ud && Xd && dop_size > 0) {
        HIPDRT_CHECK(td.alloc(tb));
        launch_apply_rows(st, B, dop_size, Xd, dop_size, 0, r, Ud, dop_size, a.cs, nullptr, td.d(), r);
        LAUNCH_OK();
        a.Td = td.d();
    }
    launch_response_assemble(st, B, a);
    LAUNCH_OK();
    return HIPDRT_OK;
}

// ---- the distribution of phasances: what hipdrt_plan_predict_dop and the two posterior entry points share --------------------------
// The grids of a request on the device, the evaluation rows dE [nn][dop_size], the scaled DOP blocks dxd [B][dop_size] and the mean
// rows dmu [B][nn]
struct DopRequest {
    DevBuf dnu, dbn, dnorm, dE, dxd, dmu;
    int nn = 0;
    int begin(const hipdrt_plan* p, const double* nu, int nn_, const double* basis_nu, const double* normalize_by, hipStream_t st) {
        const int nd = p->desc.dop_size;
        nn = nn_;
        TRY(upload(dnu, nu, (size_t)nn * sizeof(double), st));
        TRY(upload(dbn, basis_nu, (size_t)nd * sizeof(double), st));
        if (normalize_by) TRY(upload(dnorm, normalize_by, (size_t)nn * sizeof(double), st));
        HIPDRT_CHECK(dE.alloc((size_t)nn * nd * sizeof(double)));
        HIPDRT_CHECK(dmu.alloc((size_t)p->B * nn * sizeof(double)));
        HIPDRT_CHECK(dxd.alloc((size_t)p->B * nd * sizeof(double)));
        return HIPDRT_OK;
    }
};
// predict_dop (drt1d.py:3273-3347) at derivative order `order` into R.dmu: the rows E, every member's DOP block times its own
// dop_scale_vector, their product times the coefficient scale, then normalisation and ideal elements (dop_assemble_kernel); R.dnorm
// decides whether it is normalised
static int dop_mean_dev(hipdrt_plan* p, hipStream_t st, DopRequest& R, double nu_epsilon, int order, double nu_basis_area,
                        int include_ideal) {
    const int B = p->B, n = p->n, nd = p->desc.dop_size, nn = R.nn;
    TRY(func_eval_dev(st, R.dbn.d(), nd, R.dnu.d(), nn, nu_epsilon, order, 1.0, R.dE.d(), nd));
    launch_scale_block(st, B, nd, p->x.d(), n, p->desc.dop_start, p->pd_dop_scale.d(), R.dxd.d());
    launch_apply_rows(st, B, nd, R.dxd.d(), nd, 0, nn, R.dE.d(), nd, p->pd_cs.d(), nullptr, R.dmu.d(), nn);
    LAUNCH_OK();
    DopArgs a{};
    a.nn = nn; a.include_ideal = include_ideal != 0; a.dop = R.dmu.d(); a.nu = R.dnu.d(); a.norm = R.dnorm.p ? R.dnorm.d() : nullptr;
    a.basis_area = nu_basis_area; a.X = p->x.d(); a.ldx = n; a.cs = p->pd_cs.d();
    a.idx_rinf = p->pd_idx_rinf; a.idx_induc = p->pd_idx_induc; a.idx_cinv = p->pd_idx_cinv;
    a.inductance_scale = p->pd_inductance_scale; a.capacitance_scale = p->pd_capacitance_scale; a.fit_status = p->fit_status.i();
    launch_dop_assemble(st, B, a);
    LAUNCH_OK();
    return HIPDRT_OK;
}
// what the posterior entry points refuse before anything is launched
static int dop_check_request(const hipdrt_plan* p, const hipdrt_dop_args* q) {
    HIPDRT_REQUIRE(p->prepared && p->desc.dop_size > 0, "the DOP posterior needs a prepared plan with a DOP block");
    HIPDRT_REQUIRE(p->B >= 1 && p->prepped, "no fitted batch in the plan");
    HIPDRT_REQUIRE(p->pd_set, "the prediction description is missing: call hipdrt_plan_set_predict_desc after the fit");
    HIPDRT_REQUIRE(p->n <= 4096, "the DOP posterior: n <= 4096");
    HIPDRT_REQUIRE(q->nu && q->basis_nu, "NULL pointer");
    HIPDRT_REQUIRE(q->nn >= 1 && q->nn <= 65536, "1 <= nn <= 65536");
    HIPDRT_REQUIRE(q->order >= 0 && q->order <= 2, "order must be 0, 1 or 2");
    HIPDRT_REQUIRE(q->nu_epsilon > 0.0 && std::isfinite(q->nu_epsilon), "nu_epsilon > 0");
    for (int i = 0; i < q->nn; ++i)
        HIPDRT_REQUIRE(std::isfinite(q->nu[i]) && (i == 0 || q->nu[i] >= q->nu[i - 1]), "nu must be finite and ascending");
    for (int j = 0; j < p->desc.dop_size; ++j) HIPDRT_REQUIRE(std::isfinite(q->basis_nu[j]), "basis_nu must be finite");
    if (q->normalize_by) {
        HIPDRT_REQUIRE(q->nu_basis_area > 0.0 && std::isfinite(q->nu_basis_area), "nu_basis_area > 0");
        for (int i = 0; i < q->nn; ++i)
            HIPDRT_REQUIRE(q->normalize_by[i] > 0.0 && std::isfinite(q->normalize_by[i]), "normalize_by must be positive and finite");
    }
    return HIPDRT_OK;
}
// ... and of the dop_scale_vector of members b0 .. b0 + nb - 1 as hipdrt_plan_set_predict_desc left it on the device: 1 / it scales P.
// (That of a member whose fit failed is not looked at: its data may not have been finite, and its rows are NaN anyway.)
static int dop_check_scales(const hipdrt_plan* p, hipStream_t st, int b0, int nb) {
    const int nd = p->desc.dop_size;
    std::vector<double> dsv((size_t)nb * nd);
    std::vector<int> fit(nb);
    HIPDRT_CHECK(hipMemcpyAsync(dsv.data(), p->pd_dop_scale.d() + (size_t)b0 * nd, dsv.size() * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(fit.data(), p->fit_status.i() + b0, (size_t)nb * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    for (int b = 0; b < nb; ++b)
        for (int j = 0; j < nd && fit[b] >= 0; ++j)
            HIPDRT_REQUIRE(dsv[(size_t)b * nd + j] > 0.0 && std::isfinite(dsv[(size_t)b * nd + j]),
                           "dop_scale_vector must be finite and positive");
    return HIPDRT_OK;
}
}  // namespace hipdrt

extern "C" {

int hipdrt_plan_set_predict_desc(hipdrt_plan* p, const hipdrt_predict_desc* d) try {
    HIPDRT_REQUIRE(p && d, "NULL pointer");
    HIPDRT_REQUIRE(p->prepared, "the prediction description belongs to a prepared plan (hipdrt_plan_create_prepared)");
    HIPDRT_REQUIRE(p->B >= 1 && p->prepped, "no fitted batch in the plan");
    const int B = p->B, ns = p->ns, nd = p->desc.dop_size, nvb = p->desc.vb_size;
    for (int idx : {d->idx_rinf, d->idx_induc, d->idx_cinv})
        HIPDRT_REQUIRE(idx >= -1 && idx < ns, "idx_rinf, idx_induc and idx_cinv lie inside the special block, or are -1");
    HIPDRT_REQUIRE(d->idx_induc < 0 || std::isfinite(d->inductance_scale), "inductance_scale must be finite");
    HIPDRT_REQUIRE(d->idx_cinv < 0 || std::isfinite(d->capacitance_scale), "capacitance_scale must be finite");
    HIPDRT_REQUIRE(d->coefficient_scale, "coefficient_scale [B] is required");
    HIPDRT_REQUIRE(nd == 0 || d->dop_scale_vector, "the plan has a DOP block: dop_scale_vector [dop_size] or [B][dop_size] is required");
    HIPDRT_REQUIRE(nvb == 0 || (d->v_baseline_scale && d->response_signal_scale),
                   "the plan has a v_baseline block: v_baseline_scale [vb_size] and response_signal_scale [B] are required");
    // (the per-member scales are not checked: those of a member whose data were not finite are not, and its row is NaN anyway)
    // (nor is a per-member dop_scale_vector)
    if (!d->dop_scale_batched)
        for (int k = 0; k < nd; ++k) HIPDRT_REQUIRE(std::isfinite(d->dop_scale_vector[k]), "dop_scale_vector must be finite");
    for (int k = 0; k < nvb; ++k)
        HIPDRT_REQUIRE(std::isfinite(d->v_baseline_scale[k]) && d->v_baseline_scale[k] != 0.0, "v_baseline_scale must be finite and non-zero");
    hipStream_t st; TRY(enter(p->ctx, &st));
    p->pd_set = 0;
    const size_t bb = (size_t)B * sizeof(double);
    TRY(upload(p->pd_cs, d->coefficient_scale, bb, st));
    std::vector<double> zeros(B, 0.0), ones(B, 1.0);
    TRY(upload(p->pd_rss, d->response_signal_scale ? d->response_signal_scale : ones.data(), bb, st));
    TRY(upload(p->pd_sro, d->scaled_response_offset ? d->scaled_response_offset : zeros.data(), bb, st));
    std::vector<double> dsv;
    if (nd > 0) {                                // held per member: a shared vector is repeated
        dsv.resize((size_t)B * nd);
        for (int b = 0; b < B; ++b)
            for (int k = 0; k < nd; ++k) dsv[(size_t)b * nd + k] = d->dop_scale_vector[(d->dop_scale_batched ? (size_t)b * nd : 0) + k];
        TRY(upload(p->pd_dop_scale, dsv.data(), dsv.size() * sizeof(double), st));
    }
    if (nvb > 0) TRY(upload(p->pd_vb_scale, d->v_baseline_scale, (size_t)nvb * sizeof(double), st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    p->pd_idx_rinf = d->idx_rinf; p->pd_idx_induc = d->idx_induc; p->pd_idx_cinv = d->idx_cinv;
    p->pd_inductance_scale = d->inductance_scale; p->pd_capacitance_scale = d->capacitance_scale;
    p->pd_set = 1;
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_predict_response(hipdrt_plan* p, const hipdrt_response_args* q, double* out, int* status) try {
    HIPDRT_REQUIRE(p && q && out, "NULL pointer");
    HIPDRT_REQUIRE(p->prepared, "response prediction is built for prepared plans (hipdrt_plan_create_prepared)");
    HIPDRT_REQUIRE(p->B >= 1 && p->prepped, "no fitted batch in the plan");
    HIPDRT_REQUIRE(p->pd_set, "the prediction description is missing: call hipdrt_plan_set_predict_desc after the fit");
    HIPDRT_REQUIRE(p->basis_nb >= 1, "the tau basis is missing: call hipdrt_plan_set_tau_basis");
    const int B = p->B, n = p->n, ns = p->ns, ntau = p->basis_nb, copies = (n - ns) / ntau;
    const int nt = q->nt, S = q->nsteps, mask = q->include_mask, nd = p->desc.dop_size, nvb = p->desc.vb_size;
    HIPDRT_REQUIRE(mask >= 0 && mask < 128, "include_mask: HIPDRT_INCLUDE_* bits");
    HIPDRT_REQUIRE(q->times && nt >= 1 && nt <= 65535, "times: 1 <= nt <= 65535");
    HIPDRT_REQUIRE(q->step_times && q->step_sizes && S >= 1, "step_times, step_sizes: nsteps >= 1");
    HIPDRT_REQUIRE((long long)S * nt <= (1 << 22) - 64, "nsteps * nt < 2^22");
    for (int i = 0; i < nt; ++i) HIPDRT_REQUIRE(std::isfinite(q->times[i]), "times must be finite");
    for (int s = 0; s < S; ++s) HIPDRT_REQUIRE(std::isfinite(q->step_times[s]), "step_times must be finite");
    for (size_t k = 0; k < (size_t)(q->sizes_batched ? B : 1) * S; ++k)
        HIPDRT_REQUIRE(std::isfinite(q->step_sizes[k]), "step_sizes must be finite");
    const bool want_drt = (mask & HIPDRT_INCLUDE_DRT) != 0, want_dop = (mask & HIPDRT_INCLUDE_DOP) && nd > 0;
    if (want_drt) {
        HIPDRT_REQUIRE(q->basis_tau, "the DRT term needs basis_tau");
        for (int j = 0; j < ntau; ++j) HIPDRT_REQUIRE(q->basis_tau[j] > 0.0 && std::isfinite(q->basis_tau[j]), "basis_tau must be positive and finite");
        HIPDRT_REQUIRE(q->mode == HIPDRT_MODE_INTERP || q->mode == HIPDRT_MODE_TRAPZ, "mode must be INTERP or TRAPZ");
        if (q->mode == HIPDRT_MODE_INTERP) {
            HIPDRT_REQUIRE(q->log_td && q->v && q->ngrid >= 2, "the response lookup table must be provided for mode INTERP");
            HIPDRT_REQUIRE(response_ngrid_ok(q->ngrid), "lookup too long for LDS staging");
        } else {
            HIPDRT_REQUIRE(ny_ok(q->ny), "2 <= ny <= 6000");
        }
    }
    if (want_dop) HIPDRT_REQUIRE(q->basis_nu && q->nu_epsilon > 0.0 && std::isfinite(q->nu_epsilon), "the DOP term needs basis_nu [dop_size] and nu_epsilon > 0");
    if ((mask & HIPDRT_INCLUDE_BASELINE) && nvb > 0) HIPDRT_REQUIRE(q->vb_mat, "the baseline term needs vb_mat [nt][vb_size]");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const size_t tb = (size_t)nt * sizeof(double);
    DevBuf dt, dst, dsz, dones, dtau, lut3, dsum, dU, dnu, dUd, dxd, dinf, dcap, dstr, dvb, dout, t, tn, td;
    TRY(upload(dt, q->times, tb, st));
    TRY(upload(dst, q->step_times, (size_t)S * sizeof(double), st));
    TRY(upload(dsz, q->step_sizes, (size_t)(q->sizes_batched ? B : 1) * S * sizeof(double), st));
    std::vector<double> ones(S, 1.0);
    TRY(upload(dones, ones.data(), (size_t)S * sizeof(double), st));
    ResponseArgs a{};
    a.S = S; a.nt = nt; a.mask = mask; a.sizes = dsz.d(); a.sizes_batched = q->sizes_batched != 0;
    a.X = p->x.d(); a.ldx = n; a.cs = p->pd_cs.d(); a.rss = p->pd_rss.d(); a.sro = p->pd_sro.d();
    a.idx_rinf = p->pd_idx_rinf; a.idx_cinv = p->pd_idx_cinv; a.vz_index = p->desc.vz_index;
    a.vb_start = p->desc.vb_start; a.vb_size = nvb; a.capacitance_scale = p->pd_capacitance_scale;
    a.vb_scale = p->pd_vb_scale.d(); a.fit_status = p->fit_status.i();
    if (q->inf_rv) { TRY(upload(dinf, q->inf_rv, (q->inf_batched ? B : 1) * tb, st)); a.inf_rv = dinf.d(); a.inf_batched = q->inf_batched != 0; }
    if (q->cap_rv) { TRY(upload(dcap, q->cap_rv, (q->cap_batched ? B : 1) * tb, st)); a.cap_rv = dcap.d(); a.cap_batched = q->cap_batched != 0; }
    if (q->vz_strength) { TRY(upload(dstr, q->vz_strength, tb, st)); a.strength = dstr.d(); }
    if (q->vb_mat && nvb > 0) { TRY(upload(dvb, q->vb_mat, tb * nvb, st)); a.vb_mat = dvb.d(); }
    HIPDRT_CHECK(dout.alloc((size_t)B * tb));
    a.out = dout.d();
    if (want_drt) {
        TRY(upload(dtau, q->basis_tau, (size_t)ntau * sizeof(double), st));
        if (q->mode == HIPDRT_MODE_INTERP) TRY(stage_lut(st, lut3, q->ngrid, 1, 0, q->log_td, q->v));
        HIPDRT_CHECK(dsum.alloc(tb * ntau));
        HIPDRT_CHECK(dU.alloc(tb * ntau * S));
    }
    if (want_dop) {
        TRY(upload(dnu, q->basis_nu, (size_t)nd * sizeof(double), st));
        if (dsum.bytes < tb * nd) HIPDRT_CHECK(dsum.alloc(tb * (nd > ntau ? nd : ntau)));
        HIPDRT_CHECK(dUd.alloc(tb * nd * S));
        HIPDRT_CHECK(dxd.alloc((size_t)B * nd * sizeof(double)));
    }
    PredictTimer tm(p->ctx, st);
    if (want_drt) {
        // the unit-step layers, once for the batch: the members' step sizes enter in the assembly
        if (q->mode == HIPDRT_MODE_INTERP) launch_lut_slopes(st, lut3.d(), q->ngrid, 1);
        launch_response_matrix(st, dt.d(), nt, dtau.d(), ntau, dst.d(), dones.d(), S, q->mode, p->basis_eps, q->ngrid, lut3.d(),
                               q->ny, dsum.d(), dU.d());
        LAUNCH_OK();
    }
    if (want_dop) {
        launch_phasor_v(st, dt.d(), nt, dnu.d(), nd, q->nu_epsilon, dst.d(), dones.d(), S, dsum.d(), dUd.d());
        launch_scale_block(st, B, nd, p->x.d(), n, p->desc.dop_start, p->pd_dop_scale.d(), dxd.d());
        LAUNCH_OK();
    }
    TRY(response_chain(st, B, ntau, copies, ns, want_drt ? dU.d() : nullptr, want_dop ? dUd.d() : nullptr, want_dop ? dxd.d() : nullptr, nd,
                       a, t, tn, td));
    tm.mark();
    HIPDRT_CHECK(hipMemcpyAsync(out, dout.p, (size_t)B * tb, hipMemcpyDeviceToHost, st));
    if (status) HIPDRT_CHECK(hipMemcpyAsync(status, p->fit_status.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_predict_z_model(hipdrt_plan* p, const hipdrt_z_model_args* q, double* z_re, double* z_im, int* status) try {
    HIPDRT_REQUIRE(p && q && z_re && z_im, "NULL pointer");
    HIPDRT_REQUIRE(p->prepared, "hipdrt_plan_predict_z_model is built for prepared plans; a plain EIS plan has hipdrt_plan_predict_z");
    HIPDRT_REQUIRE(p->B >= 1 && p->prepped, "no fitted batch in the plan");
    HIPDRT_REQUIRE(p->pd_set, "the prediction description is missing: call hipdrt_plan_set_predict_desc after the fit");
    HIPDRT_REQUIRE(p->basis_nb >= 1, "the tau basis is missing: call hipdrt_plan_set_tau_basis");
    const int B = p->B, n = p->n, ns = p->ns, ntau = p->basis_nb, copies = (n - ns) / ntau;
    const int nf = q->nf, mask = q->include_mask, nd = p->desc.dop_size;
    HIPDRT_REQUIRE(mask >= 0 && mask < 128, "include_mask: HIPDRT_INCLUDE_* bits");
    HIPDRT_REQUIRE(q->freq && nf >= 1 && nf <= 65535, "freq: 1 <= nf <= 65535");
    for (int i = 0; i < nf; ++i) HIPDRT_REQUIRE(q->freq[i] > 0.0 && std::isfinite(q->freq[i]), "frequencies must be positive and finite");
    const bool want_drt = (mask & HIPDRT_INCLUDE_DRT) != 0, want_dop = (mask & HIPDRT_INCLUDE_DOP) && nd > 0;
    if (want_drt) {
        HIPDRT_REQUIRE(q->basis_tau, "the DRT term needs basis_tau");
        for (int j = 0; j < ntau; ++j) HIPDRT_REQUIRE(q->basis_tau[j] > 0.0 && std::isfinite(q->basis_tau[j]), "basis_tau must be positive and finite");
    }
    if (want_dop) HIPDRT_REQUIRE(q->basis_nu && q->nu_epsilon > 0.0 && std::isfinite(q->nu_epsilon), "the DOP term needs basis_nu [dop_size] and nu_epsilon > 0");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const size_t fb = (size_t)nf * sizeof(double);
    DevBuf dfreq, dA, dnu, dZd, dxd, dstr, dy, dyn, dyd, dzr, dzi;
    TRY(upload(dfreq, q->freq, fb, st));
    if (q->vz_strength) TRY(upload(dstr, q->vz_strength, fb, st));
    HIPDRT_CHECK(dzr.alloc((size_t)B * fb)); HIPDRT_CHECK(dzi.alloc((size_t)B * fb));
    ZModelArgs a{};
    a.nf = nf; a.mask = mask; a.X = p->x.d(); a.ldx = n; a.cs = p->pd_cs.d();
    a.idx_rinf = p->pd_idx_rinf; a.idx_induc = p->pd_idx_induc; a.idx_cinv = p->pd_idx_cinv; a.vz_index = p->desc.vz_index;
    a.inductance_scale = p->pd_inductance_scale; a.capacitance_scale = p->pd_capacitance_scale;
    a.freq = dfreq.d(); a.strength = q->vz_strength ? dstr.d() : nullptr; a.fit_status = p->fit_status.i();
    a.z_re = dzr.d(); a.z_im = dzi.d();
    if (want_drt) {
        HIPDRT_CHECK(dA.alloc(2 * fb * ntau));
        HIPDRT_CHECK(dy.alloc((size_t)B * 2 * fb));
        if (copies == 2) HIPDRT_CHECK(dyn.alloc((size_t)B * 2 * fb));
    }
    if (want_dop) {
        TRY(upload(dnu, q->basis_nu, (size_t)nd * sizeof(double), st));
        HIPDRT_CHECK(dZd.alloc(2 * fb * nd));
        HIPDRT_CHECK(dyd.alloc((size_t)B * 2 * fb));
        HIPDRT_CHECK(dxd.alloc((size_t)B * nd * sizeof(double)));
    }
    PredictTimer tm(p->ctx, st);
    if (want_drt)
        // [A'; A''] at the requested frequencies, every entry evaluated where it stands (the checks of the lookup tables are
        // hipdrt_impedance_matrix_dev's, as is the upload of the grids and tables: inside the timed span), both parts as the two
        // row blocks of one product per copy
        TRY(hipdrt_impedance_matrix_dev(p->ctx, 1, 0, q->freq, nf, q->basis_tau, ntau, q->mode, 0, p->basis_eps, q->ngrid,
                                        q->log_wt_re, q->z_re, q->log_wt_im, q->z_im, q->ny, dA.d(), dA.d() + (size_t)nf * ntau, 1,
                                        nullptr));
    if (want_drt) {
        launch_apply_rows(st, B, ntau, p->x.d(), n, ns, 2 * nf, dA.d(), ntau, a.cs, nullptr, dy.d(), 2 * nf);
        a.Y = dy.d();
        if (copies == 2) {
            launch_apply_rows(st, B, ntau, p->x.d(), n, ns + ntau, 2 * nf, dA.d(), ntau, a.cs, nullptr, dyn.d(), 2 * nf);
            a.Yn = dyn.d();
        }
        LAUNCH_OK();
    }
    if (want_dop) {
        launch_phasor_z(st, dfreq.d(), nf, dnu.d(), nd, q->nu_epsilon, dZd.d(), dZd.d() + (size_t)nf * nd);
        launch_scale_block(st, B, nd, p->x.d(), n, p->desc.dop_start, p->pd_dop_scale.d(), dxd.d());
        launch_apply_rows(st, B, nd, dxd.d(), nd, 0, 2 * nf, dZd.d(), nd, a.cs, nullptr, dyd.d(), 2 * nf);
        LAUNCH_OK();
        a.Yd = dyd.d();
    }
    launch_z_model_assemble(st, B, a);
    LAUNCH_OK();
    tm.mark();
    HIPDRT_CHECK(hipMemcpyAsync(z_re, dzr.p, (size_t)B * fb, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(z_im, dzi.p, (size_t)B * fb, hipMemcpyDeviceToHost, st));
    if (status) HIPDRT_CHECK(hipMemcpyAsync(status, p->fit_status.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_predict_dop(hipdrt_plan* p, const double* nu, int nn, const double* basis_nu, double nu_epsilon,
                            const double* normalize_by, double nu_basis_area, int include_ideal, double* out, int* status) try {
    HIPDRT_REQUIRE(p && nu && basis_nu && out, "NULL pointer");
    HIPDRT_REQUIRE(p->prepared && p->desc.dop_size > 0, "hipdrt_plan_predict_dop needs a prepared plan with a DOP block");
    HIPDRT_REQUIRE(p->B >= 1 && p->prepped, "no fitted batch in the plan");
    HIPDRT_REQUIRE(p->pd_set, "the prediction description is missing: call hipdrt_plan_set_predict_desc after the fit");
    HIPDRT_REQUIRE(nn >= 1 && nn <= (1 << 22) - 64, "1 <= nn < 2^22");
    HIPDRT_REQUIRE(nu_epsilon > 0.0 && std::isfinite(nu_epsilon), "nu_epsilon > 0");
    for (int i = 0; i < nn; ++i) HIPDRT_REQUIRE(std::isfinite(nu[i]) && (i == 0 || nu[i] >= nu[i - 1]), "nu must be finite and ascending");
    if (normalize_by) {
        HIPDRT_REQUIRE(nu_basis_area > 0.0 && std::isfinite(nu_basis_area), "nu_basis_area > 0");
        for (int i = 0; i < nn; ++i) HIPDRT_REQUIRE(normalize_by[i] > 0.0 && std::isfinite(normalize_by[i]), "normalize_by must be positive and finite");
    }
    hipStream_t st; TRY(enter(p->ctx, &st));
    DopRequest R;
    TRY(R.begin(p, nu, nn, basis_nu, normalize_by, st));
    PredictTimer tm(p->ctx, st);
    TRY(dop_mean_dev(p, st, R, nu_epsilon, 0, nu_basis_area, include_ideal));
    tm.mark();
    HIPDRT_CHECK(hipMemcpyAsync(out, R.dmu.p, R.dmu.bytes, hipMemcpyDeviceToHost, st));
    if (status) HIPDRT_CHECK(hipMemcpyAsync(status, p->fit_status.p, (size_t)p->B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

// DRT.predict_dop_ci (drt1d.py:3233-3258) and the diagonal of DRT.estimate_dop_cov (3153-3198) of every member: the mean chain above
// at order k, then one Gram/L2 rebuild, the congruence scaling by every member's own 1 / dop_scale_vector and one factorisation per
// member (plan_quadratic_forms_dev), then dop_band_kernel
int hipdrt_plan_dop_posterior(hipdrt_plan* p, const hipdrt_dop_args* q, double* mu, double* lo, double* hi, double* var,
                              int* status) try {
    HIPDRT_REQUIRE(p && q, "NULL pointer");
    TRY(dop_check_request(p, q));
    const bool band = lo || hi || var;
    HIPDRT_REQUIRE(!(lo || hi) || (std::isfinite(q->s_lo) && std::isfinite(q->s_hi)), "s_lo and s_hi must be finite");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const int B = p->B, nn = q->nn, nd = p->desc.dop_size;
    if (band) TRY(dop_check_scales(p, st, 0, B));
    DopRequest R;
    TRY(R.begin(p, q->nu, nn, q->basis_nu, q->normalize_by, st));
    DevBuf dsinv, scratch, dvar, dvstat;
    if (band) HIPDRT_CHECK(dsinv.alloc((size_t)B * nd * sizeof(double)));
    PredictTimer tm(p->ctx, st);
    TRY(dop_mean_dev(p, st, R, q->nu_epsilon, q->order, q->nu_basis_area, q->include_ideal));
    tm.mark();
    DevOuts outs;
    if (band) {
        launch_dop_recip(st, B, nd, p->pd_dop_scale.d(), nd, dsinv.d());
        LAUNCH_OK();
        TRY(plan_quadratic_forms_dev(p, live_source(p), -1, R.dE.d(), nn, nd, p->desc.dop_start, scratch, dvar, dvstat, dsinv.d()));
        double *dlo = nullptr, *dhi = nullptr, *dvo = nullptr;
        TRY(outs.want(lo, (size_t)B * nn, dlo)); TRY(outs.want(hi, (size_t)B * nn, dhi)); TRY(outs.want(var, (size_t)B * nn, dvo));
        launch_dop_band(st, B, nn, R.dmu.d(), dvar.d(), (long long)((nn + 15) / 16) * 16, p->pd_cs.d(),
                        q->normalize_by ? R.dnorm.d() : nullptr, q->s_lo, q->s_hi, dvstat.i(), p->fit_status.i(), dlo, dhi, dvo);
        LAUNCH_OK();
        tm.mark();
        TRY(outs.back(st));
    }
    if (mu) HIPDRT_CHECK(hipMemcpyAsync(mu, R.dmu.p, R.dmu.bytes, hipMemcpyDeviceToHost, st));
    std::vector<int> hs(B), hv(B, 0);
    HIPDRT_CHECK(hipMemcpyAsync(hs.data(), p->fit_status.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    if (band) HIPDRT_CHECK(hipMemcpyAsync(hv.data(), dvstat.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    if (status) merge_status(B, hs.data(), band ? hv.data() : nullptr, status);
    return HIPDRT_OK;
} HIPDRT_CATCH

// DRT.estimate_dop_cov (drt1d.py:3153-3198) of member b: plan_full_cov's route (plan_post.hip) on the scaled image of that member's P
// in the single-member form -- the factorisation leaves Y = E L^-T behind the factor, rows_outer_kernel forms Y Y' cs_b^2 -- then
// upstream's broadcast division of column j by normalize_by[j]^2 on the host
int hipdrt_plan_dop_cov(hipdrt_plan* p, int b, const hipdrt_dop_args* q, double* out, int* status) try {
    HIPDRT_REQUIRE(p && q && out, "NULL pointer");
    TRY(dop_check_request(p, q));
    HIPDRT_REQUIRE(b >= 0 && b < p->B, "spectrum index out of range");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const int B = p->B, nn = q->nn, nd = p->desc.dop_size;
    const size_t cells = (size_t)nn * nn;
    TRY(dop_check_scales(p, st, b, 1));
    DopRequest R;
    TRY(R.begin(p, q->nu, nn, q->basis_nu, nullptr, st));
    DevBuf dsinv, scratch, dvar, dvstat, dcov;
    HIPDRT_CHECK(dsinv.alloc((size_t)B * nd * sizeof(double)));
    HIPDRT_CHECK(dcov.alloc(cells * sizeof(double)));
    TRY(func_eval_dev(st, R.dbn.d(), nd, R.dnu.d(), nn, q->nu_epsilon, q->order, 1.0, R.dE.d(), nd));
    launch_dop_recip(st, B, nd, p->pd_dop_scale.d(), nd, dsinv.d());
    LAUNCH_OK();
    TRY(plan_quadratic_forms_dev(p, live_source(p), b, R.dE.d(), nn, nd, p->desc.dop_start, scratch, dvar, dvstat, dsinv.d()));
    double cs = 1.0;
    int hv = 0, hf = 0;
    HIPDRT_CHECK(hipMemcpyAsync(&cs, p->pd_cs.d() + b, sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(&hv, dvstat.p, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(&hf, p->fit_status.i() + b, sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    int merged = 0;
    merge_status(1, &hf, &hv, &merged);
    if (status) *status = merged;
    if (merged < 0) {                            // (the reference warns and returns None)
        for (size_t i = 0; i < cells; ++i) out[i] = __builtin_nan("");
        return HIPDRT_OK;
    }
    posterior_cov_dev(st, scratch.d(), p->n, nn, cs * cs, dcov.d());
    LAUNCH_OK();
    HIPDRT_CHECK(hipMemcpyAsync(out, dcov.p, cells * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    if (q->normalize_by)
        for (int i = 0; i < nn; ++i)
            for (int j = 0; j < nn; ++j) out[(size_t)i * nn + j] /= q->normalize_by[j] * q->normalize_by[j];
    return HIPDRT_OK;
} HIPDRT_CATCH

}  // extern "C"
