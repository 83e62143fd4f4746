// Stand-alone operators of the C-ABI (include/hipdrt.h): host arrays in, one launch sequence on the context's stream, host
// arrays out.
#include <cmath>

#include "plan.hpp"

namespace hipdrt {
hipdrt_qp_opts default_qp_opts() { return hipdrt_qp_opts{1e-7, 1e-6, 1e-7, 100}; }

int func_eval_dev(hipStream_t st, const double* basis_dev, int nb, const double* ev_dev, int ne, double eps, int order, double fac,
                  double* out_dev, int ld) {
    // the two constants as Python forms them in basis.get_basis_func_derivative: -2 * epsilon ** 2 and 4 * epsilon ** 4
    const double c1 = -2.0 * std::pow(eps, 2.0), c2 = 4.0 * std::pow(eps, 4.0);
    launch_func_eval(st, basis_dev, nb, ev_dev, ne, eps, order, c1, c2, fac, out_dev, ld);
    LAUNCH_OK();
    return HIPDRT_OK;
}
}  // namespace hipdrt

// the tail of every entry point: the outputs on their way to the host, and the stream drained
static int back_and_wait(const DevOuts& outs, hipStream_t st) {
    TRY(outs.back(st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
}

// the device copies of what every step-response builder reads (col: the tau or nu grid; tau_rise only where the model has one)
struct StepInputs {
    DevBuf times, col, step_times, step_sizes, tau_rise;
    int upload_all(hipStream_t st, const double* t, int nt, const double* c, int ncol, const double* stt, const double* sz, int nsteps,
                   const double* rise = nullptr) {
        TRY(upload(times, t, (size_t)nt * sizeof(double), st));
        TRY(upload(col, c, (size_t)ncol * sizeof(double), st));
        TRY(upload(step_times, stt, (size_t)nsteps * sizeof(double), st));
        TRY(upload(step_sizes, sz, (size_t)nsteps * sizeof(double), st));
        if (rise) TRY(upload(tau_rise, rise, (size_t)nsteps * sizeof(double), st));
        return HIPDRT_OK;
    }
};

extern "C" {

int hipdrt_impedance_lookup(hipdrt_ctx* ctx, double epsilon, int ngrid, int ny, const double* wt_re,
                            const double* wt_im, double* z_re, double* z_im) try {
    HIPDRT_REQUIRE(ctx && wt_re && wt_im && z_re && z_im, "NULL pointer");
    HIPDRT_REQUIRE(ngrid >= 2 && ny_ok(ny), "ngrid >= 2, 2 <= ny <= 6000");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf dwr, dwi;
    DevOuts outs;
    double *dzr = nullptr, *dzi = nullptr;
    const size_t gb = (size_t)ngrid * sizeof(double);
    TRY(upload(dwr, wt_re, gb, st)); TRY(upload(dwi, wt_im, gb, st));
    TRY(outs.want(z_re, (size_t)ngrid, dzr)); TRY(outs.want(z_im, (size_t)ngrid, dzi));
    launch_lookup(st, epsilon, ngrid, ny, dwr.d(), dwi.d(), dzr, dzi);
    LAUNCH_OK();
    return back_and_wait(outs, st);
} HIPDRT_CATCH

int hipdrt_phasor_z_matrix(hipdrt_ctx* ctx, const double* freq, int nf, const double* basis_nu, int n_nu, double nu_epsilon,
                           double* zm_re, double* zm_im) try {
    HIPDRT_REQUIRE(ctx && freq && basis_nu && zm_re && zm_im, "NULL pointer");
    HIPDRT_REQUIRE(nf >= 1 && n_nu >= 1 && nu_epsilon > 0.0, "nf, n_nu >= 1, nu_epsilon > 0");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf df, dn;
    DevOuts outs;
    double *dr = nullptr, *di = nullptr;
    TRY(upload(df, freq, (size_t)nf * sizeof(double), st));
    TRY(upload(dn, basis_nu, (size_t)n_nu * sizeof(double), st));
    TRY(outs.want(zm_re, (size_t)nf * n_nu, dr)); TRY(outs.want(zm_im, (size_t)nf * n_nu, di));
    launch_phasor_z(st, df.d(), nf, dn.d(), n_nu, nu_epsilon, dr, di);
    LAUNCH_OK();
    return back_and_wait(outs, st);
} HIPDRT_CATCH

int hipdrt_phasor_v_matrix(hipdrt_ctx* ctx, const double* times, int nt, const double* basis_nu, int n_nu, double nu_epsilon,
                           const double* step_times, const double* step_sizes, int nsteps, double* rm, double* layered) try {
    HIPDRT_REQUIRE(ctx && times && basis_nu && step_times && step_sizes && rm, "NULL pointer");
    HIPDRT_REQUIRE(nt >= 1 && n_nu >= 1 && nsteps >= 1 && nu_epsilon > 0.0, "nt, n_nu, nsteps >= 1, nu_epsilon > 0");
    hipStream_t st; TRY(enter(ctx, &st));
    StepInputs in;
    DevOuts outs;
    double *dr = nullptr, *dl = nullptr;
    TRY(in.upload_all(st, times, nt, basis_nu, n_nu, step_times, step_sizes, nsteps));
    TRY(outs.want(rm, (size_t)nt * n_nu, dr)); TRY(outs.want(layered, (size_t)nt * n_nu * nsteps, dl));
    launch_phasor_v(st, in.times.d(), nt, in.col.d(), n_nu, nu_epsilon, in.step_times.d(), in.step_sizes.d(), nsteps, dr, dl);
    LAUNCH_OK();
    return back_and_wait(outs, st);
} HIPDRT_CATCH

int hipdrt_chrono_var_matrix(hipdrt_ctx* ctx, const double* tt, int nt, const int* seg, int nseg, double vmm_epsilon,
                             int uniform, double* vmm) try {
    HIPDRT_REQUIRE(ctx && tt && seg && vmm, "NULL pointer");
    HIPDRT_REQUIRE(nt >= 1 && nseg >= 1, "nt >= 1, nseg >= 1");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf dtt, dseg;
    DevOuts outs;
    double* dv = nullptr;
    TRY(upload(dtt, tt, (size_t)nt * sizeof(double), st));
    TRY(upload(dseg, seg, (size_t)(nseg + 1) * sizeof(int), st));
    TRY(outs.want(vmm, (size_t)nt * nt, dv));
    launch_chrono_vmm(st, dtt.d(), nt, dseg.i(), nseg, vmm_epsilon, uniform, dv);
    LAUNCH_OK();
    return back_and_wait(outs, st);
} HIPDRT_CATCH

int hipdrt_response_lookup(hipdrt_ctx* ctx, double epsilon, int ngrid, int ny, const double* td, double* v) try {
    HIPDRT_REQUIRE(ctx && td && v, "NULL pointer");
    HIPDRT_REQUIRE(ngrid >= 2 && ny_ok(ny), "ngrid >= 2, 2 <= ny <= 6000");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf dtd;
    DevOuts outs;
    double* dv = nullptr;
    TRY(upload(dtd, td, (size_t)ngrid * sizeof(double), st));
    TRY(outs.want(v, (size_t)ngrid, dv));
    launch_response_lookup(st, epsilon, ngrid, ny, dtd.d(), dv);
    LAUNCH_OK();
    return back_and_wait(outs, st);
} HIPDRT_CATCH

int hipdrt_response_matrix(hipdrt_ctx* ctx, const double* times, int nt, const double* tau, int ntau,
                           const double* step_times, const double* step_sizes, int nsteps, int mode, double epsilon,
                           int ngrid, const double* log_td, const double* v, int ny, double* a, double* layered) try {
    HIPDRT_REQUIRE(ctx && times && tau && step_times && step_sizes && a, "NULL pointer");
    HIPDRT_REQUIRE(nt >= 1 && ntau >= 1 && nsteps >= 1, "nt, ntau, nsteps >= 1");
    HIPDRT_REQUIRE(mode == HIPDRT_MODE_INTERP || mode == HIPDRT_MODE_TRAPZ, "mode must be INTERP or TRAPZ");
    if (mode == HIPDRT_MODE_INTERP) {
        HIPDRT_REQUIRE(log_td && v && ngrid >= 2, "interpolate_grids must be provided for integrate_method 'interp'");
        HIPDRT_REQUIRE(response_ngrid_ok(ngrid), "lookup too long for LDS staging");
    } else {
        HIPDRT_REQUIRE(ny_ok(ny), "2 <= ny <= 6000");
    }
    hipStream_t st; TRY(enter(ctx, &st));
    StepInputs in;
    DevBuf lut3;
    DevOuts outs;
    double *da = nullptr, *dl = nullptr;
    TRY(in.upload_all(st, times, nt, tau, ntau, step_times, step_sizes, nsteps));
    if (mode == HIPDRT_MODE_INTERP) {
        TRY(stage_lut(st, lut3, ngrid, 1, 0, log_td, v));
        launch_lut_slopes(st, lut3.d(), ngrid, 1);
    }
    TRY(outs.want(a, (size_t)nt * ntau, da)); TRY(outs.want(layered, (size_t)nt * ntau * nsteps, dl));
    launch_response_matrix(st, in.times.d(), nt, in.col.d(), ntau, in.step_times.d(), in.step_sizes.d(), nsteps, mode, epsilon,
                           ngrid, lut3.d(), ny, da, dl);
    LAUNCH_OK();
    return back_and_wait(outs, st);
} HIPDRT_CATCH

int hipdrt_response_matrix_variant(hipdrt_ctx* ctx, const double* times, int nt, const double* tau, int ntau,
                                   const double* step_times, const double* step_sizes, const double* tau_rise, int nsteps,
                                   int variant, double epsilon, int ny, double* a, double* layered) try {
    HIPDRT_REQUIRE(ctx && times && tau && step_times && step_sizes && a, "NULL pointer");
    HIPDRT_REQUIRE(nt >= 1 && ntau >= 1 && nsteps >= 1, "nt, ntau, nsteps >= 1");
    HIPDRT_REQUIRE(variant == HIPDRT_RESPONSE_POT || variant == HIPDRT_RESPONSE_EXPDECAY, "variant must be POT or EXPDECAY");
    if (variant == HIPDRT_RESPONSE_EXPDECAY) {
        HIPDRT_REQUIRE(tau_rise, "the expdecay step model needs tau_rise");
        HIPDRT_REQUIRE(ny_ok(ny), "2 <= ny <= 6000");
    }
    hipStream_t st; TRY(enter(ctx, &st));
    StepInputs in;
    DevOuts outs;
    double *da = nullptr, *dl = nullptr;
    TRY(in.upload_all(st, times, nt, tau, ntau, step_times, step_sizes, nsteps,
                      variant == HIPDRT_RESPONSE_EXPDECAY ? tau_rise : nullptr));
    TRY(outs.want(a, (size_t)nt * ntau, da)); TRY(outs.want(layered, (size_t)nt * ntau * nsteps, dl));
    launch_response_variant(st, in.times.d(), nt, in.col.d(), ntau, in.step_times.d(), in.step_sizes.d(), in.tau_rise.d(), nsteps,
                            variant, epsilon, ny, da, dl);
    LAUNCH_OK();
    return back_and_wait(outs, st);
} HIPDRT_CATCH

// the body of both impedance entry points.  to_host: a_re / a_im are host arrays (device twins here, copied back), else device memory
static int impedance_matrix_common(hipdrt_ctx* ctx, int B, int freq_batched, const double* freq, int nf,
                                   const double* tau, int ntau, int mode, int toeplitz, double epsilon, int ngrid,
                                   const double* log_wt_re, const double* z_re, const double* log_wt_im,
                                   const double* z_im, int ny, double* a_re, double* a_im, bool to_host, int repeat,
                                   float* elapsed_ms) {
    HIPDRT_REQUIRE(ctx && freq && tau && a_re && a_im, "NULL pointer");
    HIPDRT_REQUIRE(B >= 1 && nf >= 1 && ntau >= 1, "B, nf, ntau >= 1");
    HIPDRT_REQUIRE(mode == HIPDRT_MODE_INTERP || mode == HIPDRT_MODE_TRAPZ, "mode");
    HIPDRT_REQUIRE(!(toeplitz && freq_batched), "Toeplitz shortcut needs one shared frequency grid");
    HIPDRT_REQUIRE(toeplitz || B <= kGridDimMax, "B <= 65535 spectra in one general build");
    if (mode == HIPDRT_MODE_INTERP)
        HIPDRT_REQUIRE(log_wt_re && z_re && log_wt_im && z_im && impedance_ngrid_ok(ngrid),
                       "interp needs lookups with ngrid >= 2 that one workgroup's LDS holds (2 <= ngrid <= 3406)");
    else HIPDRT_REQUIRE(ny_ok(ny), "2 <= ny <= 6000");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf dfreq, dtau, lut6, scratch;
    DevOuts outs;
    double *dre = a_re, *dim = a_im;
    if (to_host) { TRY(outs.want(a_re, (size_t)B * nf * ntau, dre)); TRY(outs.want(a_im, (size_t)B * nf * ntau, dim)); }
    TRY(upload(dfreq, freq, (size_t)(freq_batched ? B : 1) * nf * sizeof(double), st));
    TRY(upload(dtau, tau, (size_t)ntau * sizeof(double), st));
    if (mode == HIPDRT_MODE_INTERP) {
        TRY(stage_lut(st, lut6, ngrid, 2, 0, log_wt_re, z_re));
        TRY(stage_lut(st, lut6, ngrid, 2, 1, log_wt_im, z_im));
        launch_lut_slopes(st, lut6.d(), ngrid, 2);
        LAUNCH_OK();
    }
    HIPDRT_CHECK(scratch.alloc(impedance_scratch_doubles(B, freq_batched, nf, ntau, mode, toeplitz) * sizeof(double)));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (elapsed_ms) { HIPDRT_CHECK(hipEventCreate(&e0)); HIPDRT_CHECK(hipEventCreate(&e1)); HIPDRT_CHECK(hipEventRecord(e0, st)); }
    for (int r = 0; r < (repeat < 1 ? 1 : repeat); ++r)
        launch_impedance_matrix(st, B, freq_batched, dfreq.d(), nf, dtau.d(), ntau, mode, toeplitz, epsilon, ngrid,
                                lut6.d(), ny, dre, dim, scratch.d());
    LAUNCH_OK();
    if (elapsed_ms) { HIPDRT_CHECK(hipEventRecord(e1, st)); }
    TRY(back_and_wait(outs, st));
    if (elapsed_ms) {
        HIPDRT_CHECK(hipEventElapsedTime(elapsed_ms, e0, e1));
        (void)hipEventDestroy(e0); (void)hipEventDestroy(e1);
    }
    return HIPDRT_OK;
}

int hipdrt_impedance_matrix_dev(hipdrt_ctx* ctx, int B, int freq_batched, const double* freq, int nf,
                                const double* tau, int ntau, int mode, int toeplitz, double epsilon, int ngrid,
                                const double* log_wt_re, const double* z_re, const double* log_wt_im,
                                const double* z_im, int ny, void* a_re_dev, void* a_im_dev, int repeat,
                                float* elapsed_ms) try {
    return impedance_matrix_common(ctx, B, freq_batched, freq, nf, tau, ntau, mode, toeplitz, epsilon, ngrid,
                                   log_wt_re, z_re, log_wt_im, z_im, ny, (double*)a_re_dev, (double*)a_im_dev, false, repeat,
                                   elapsed_ms);
} HIPDRT_CATCH

int hipdrt_impedance_matrix(hipdrt_ctx* ctx, int B, int freq_batched, const double* freq, int nf, const double* tau,
                            int ntau, int mode, int toeplitz, double epsilon, int ngrid, const double* log_wt_re,
                            const double* z_re, const double* log_wt_im, const double* z_im, int ny, double* a_re,
                            double* a_im) try {
    return impedance_matrix_common(ctx, B, freq_batched, freq, nf, tau, ntau, mode, toeplitz, epsilon, ngrid, log_wt_re,
                                   z_re, log_wt_im, z_im, ny, a_re, a_im, true, 1, nullptr);
} HIPDRT_CATCH

int hipdrt_nonuniform_gaussian_filter1d(hipdrt_ctx* ctx, const double* y, int n, const double* sigma, const int* seg, int nseg,
                                        const int* filtered, const double* nodes, int K, const double* node_delta,
                                        const double* weights, long long nweights, const int* woff, const int* radius,
                                        double* out) try {
    HIPDRT_REQUIRE(ctx && y && sigma && seg && filtered && nodes && node_delta && weights && woff && radius && out, "NULL pointer");
    HIPDRT_REQUIRE(n >= 1 && nseg >= 1 && K >= 1 && nweights >= 1, "n, nseg, K, nweights >= 1");
    hipStream_t st; TRY(enter(ctx, &st));
    // sample -> segment map (or -1 for an unfiltered segment)
    std::vector<int> seg_of(n, -1);
    for (int s_ = 0; s_ < nseg; ++s_) {
        HIPDRT_REQUIRE(seg[s_] >= 0 && seg[s_] <= seg[s_ + 1] && seg[s_ + 1] <= n, "segment bounds");
        if (filtered[s_]) for (int i = seg[s_]; i < seg[s_ + 1]; ++i) seg_of[i] = s_;
    }
    DevBuf dy, dsg, dso, dseg, dnodes, dnd, dw, dwo, drad;
    DevOuts outs;
    double* dout = nullptr;
    TRY(upload(dy, y, (size_t)n * sizeof(double), st));
    TRY(upload(dsg, sigma, (size_t)n * sizeof(double), st));
    TRY(upload(dso, seg_of.data(), (size_t)n * sizeof(int), st));
    TRY(upload(dseg, seg, (size_t)(nseg + 1) * sizeof(int), st));
    TRY(upload(dnodes, nodes, (size_t)nseg * K * sizeof(double), st));
    TRY(upload(dnd, node_delta, (size_t)nseg * sizeof(double), st));
    TRY(upload(dw, weights, (size_t)nweights * sizeof(double), st));
    TRY(upload(dwo, woff, (size_t)nseg * K * sizeof(int), st));
    TRY(upload(drad, radius, (size_t)nseg * K * sizeof(int), st));
    TRY(outs.want(out, (size_t)n, dout));
    launch_nonuniform_gauss(st, dy.d(), n, dsg.d(), dso.i(), dseg.i(), dnodes.d(), K, dnd.d(), dw.d(), dwo.i(), drad.i(), dout);
    LAUNCH_OK();
    return back_and_wait(outs, st);
} HIPDRT_CATCH

int hipdrt_penalty_matrices(hipdrt_ctx* ctx, const double* ln_tau, int n, double epsilon, int toeplitz, double* m0,
                            double* m1, double* m2) try {
    HIPDRT_REQUIRE(ctx && ln_tau && m0 && m1 && m2, "NULL pointer");
    HIPDRT_REQUIRE(n >= 1, "n >= 1");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf dl;
    DevOuts outs;
    double *d0 = nullptr, *d1 = nullptr, *d2 = nullptr;
    TRY(upload(dl, ln_tau, (size_t)n * sizeof(double), st));
    TRY(outs.want(m0, (size_t)n * n, d0)); TRY(outs.want(m1, (size_t)n * n, d1)); TRY(outs.want(m2, (size_t)n * n, d2));
    launch_penalty(st, dl.d(), n, epsilon, toeplitz, d0, d1, d2, n, 0);
    LAUNCH_OK();
    return back_and_wait(outs, st);
} HIPDRT_CATCH

int hipdrt_eis_var_matrix(hipdrt_ctx* ctx, const double* freq, int nf, double vmm_epsilon, double reim_cor,
                          int uniform, double* vmm) try {
    HIPDRT_REQUIRE(ctx && freq && vmm, "NULL pointer");
    HIPDRT_REQUIRE(nf >= 1, "nf >= 1");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf df;
    DevOuts outs;
    double* dv = nullptr;
    TRY(upload(df, freq, (size_t)nf * sizeof(double), st));
    TRY(outs.want(vmm, (size_t)4 * nf * nf, dv));
    launch_eis_vmm(st, df.d(), nf, vmm_epsilon, reim_cor, uniform, dv);
    LAUNCH_OK();
    return back_and_wait(outs, st);
} HIPDRT_CATCH

int hipdrt_qp_batch(hipdrt_ctx* ctx, int B, int n, int p_batched, const double* P, const double* q, int h_batched,
                    const double* h, const hipdrt_qp_opts* opts, double* x, int* iters, double* pcost, int* status) try {
    HIPDRT_REQUIRE(ctx && P && q && h && x && status, "NULL pointer");
    HIPDRT_REQUIRE(B >= 1 && n >= 1 && n <= 4096, "B >= 1, 1 <= n <= 4096");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf dP, dq, dh, dL, dstate, dPpk, dgs;
    DevOuts outs;
    const int ldl = (int)qp_scratch_ld(n);
    const int G = qp_group_size(B, n, ctx->qp_force_group);           // 0: one workgroup per problem; >= 1: that many workgroups per problem
    // device copy of P with an even leading dimension (16-byte row-pair loads in the kernels), pad column zeroed
    const int ldp = round_up(n, 2);
    const size_t nmat = (size_t)(p_batched ? B : 1);
    HIPDRT_CHECK(dP.alloc(nmat * n * ldp * sizeof(double)));
    if (ldp != n) HIPDRT_CHECK(hipMemsetAsync(dP.p, 0, dP.bytes, st));
    HIPDRT_CHECK(hipMemcpy2DAsync(dP.p, (size_t)ldp * sizeof(double), P, (size_t)n * sizeof(double),
                                  (size_t)n * sizeof(double), nmat * n, hipMemcpyHostToDevice, st));
    TRY(upload(dq, q, (size_t)B * n * sizeof(double), st));
    TRY(upload(dh, h, (size_t)(h_batched ? B : 1) * n * sizeof(double), st));
    HIPDRT_CHECK(dL.alloc((size_t)B * qp_scratch_doubles(n, G) * sizeof(double)));
    QpArgs a{};
    // the kernel writes iteration counts and costs whether or not the caller wants them back
    TRY(outs.want(x, (size_t)B * n, a.x)); TRY(outs.want(iters, (size_t)B, a.iters, true));
    TRY(outs.want(pcost, (size_t)B, a.pcost, true)); TRY(outs.want(status, (size_t)B, a.status));
    a.B = B; a.n = n; a.P = dP.d(); a.p_stride = p_batched ? (long long)n * ldp : 0; a.ldp = ldp;
    a.q = dq.d(); a.h = dh.d(); a.h_stride = h_batched ? n : 0;
    a.L = dL.d(); a.ldl = ldl; a.l_stride = (long long)qp_scratch_doubles(n, G);
    a.active = nullptr; a.iters_accum = nullptr;
    a.G = G;
    a.waves = ctx->qp_waves;
    if (G >= 1) {
        HIPDRT_CHECK(dgs.alloc((size_t)B * qp_gsync_ints() * sizeof(int)));
        a.gsync = dgs.i();
    }
    HIPDRT_CHECK(dPpk.alloc(nmat * qp_ppk_doubles(n) * sizeof(double)));
    launch_pack_p(st, (int)nmat, n, dP.d(), ldp, dPpk.d());
    a.Ppk = dPpk.d(); a.ppk_stride = p_batched ? (long long)qp_ppk_doubles(n) : 0; a.nchp = qp_nchp(n);
    HIPDRT_CHECK(dstate.alloc((size_t)B * (G > 1 ? G : 1) * qp_state_doubles(n) * sizeof(double)));
    a.state = dstate.d(); a.state_ld = qp_state_ld(n); a.state_stride = (long long)qp_state_doubles(n);
    a.opts = opts ? *opts : default_qp_opts();
    TRY(launch_qp(st, a));
    return back_and_wait(outs, st);
} HIPDRT_CATCH

int hipdrt_weighted_gram(hipdrt_ctx* ctx, int B, int m, int n, const double* A, const double* w, const double* b,
                         int l2_batched, const double* l2, const double* l1, double* P, double* q) try {
    HIPDRT_REQUIRE(ctx && A && w && b && P && q, "NULL pointer");
    HIPDRT_REQUIRE(B >= 1 && m >= 1 && n >= 1, "B, m, n >= 1");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf dA, dw, db, dl2, dl1;
    DevOuts outs;
    TRY(upload(dA, A, (size_t)m * n * sizeof(double), st));
    TRY(upload(dw, w, (size_t)B * m * sizeof(double), st));
    TRY(upload(db, b, (size_t)B * m * sizeof(double), st));
    if (l2) TRY(upload(dl2, l2, (size_t)(l2_batched ? B : 1) * n * n * sizeof(double), st));
    if (l1) TRY(upload(dl1, l1, (size_t)n * sizeof(double), st));
    // one shared A, every problem, row-major P only; L2 as given (none: l2 = NULL)
    PqArgs pq{};
    TRY(outs.want(P, (size_t)B * n * n, pq.P)); TRY(outs.want(q, (size_t)B * n, pq.q));
    pq.B = B; pq.m = m; pq.n = n; pq.A = dA.d(); pq.lda = n; pq.w = dw.d();
    pq.ldp = n; pq.p_stride = (long long)n * n;
    pq.y = db.d(); pq.l1 = l1 ? dl1.d() : nullptr;
    GramL2 g{};
    g.l2 = l2 ? dl2.d() : nullptr; g.l2_stride = l2_batched ? (long long)n * n : 0; g.ldl2 = n;
    launch_gram_l2(st, pq, g);
    launch_qvec(st, pq);
    LAUNCH_OK();
    return back_and_wait(outs, st);
} HIPDRT_CATCH

int hipdrt_func_eval_matrix(hipdrt_ctx* ctx, const double* basis_grid, int nb, const double* eval_grid, int ne, double epsilon,
                            int order, double* out) try {
    HIPDRT_REQUIRE(ctx && basis_grid && eval_grid && out, "NULL pointer");
    HIPDRT_REQUIRE(nb >= 1 && ne >= 1, "nb, ne >= 1");
    HIPDRT_REQUIRE(order >= 0 && order <= 2, "order must be 0, 1 or 2");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf db, de;
    DevOuts outs;
    double* dout = nullptr;
    TRY(upload(db, basis_grid, (size_t)nb * sizeof(double), st));
    TRY(upload(de, eval_grid, (size_t)ne * sizeof(double), st));
    TRY(outs.want(out, (size_t)ne * nb, dout));
    TRY(func_eval_dev(st, db.d(), nb, de.d(), ne, epsilon, order, 1.0, dout, nb));
    return back_and_wait(outs, st);
} HIPDRT_CATCH

}  // extern "C"
