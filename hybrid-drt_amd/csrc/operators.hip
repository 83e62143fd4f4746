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

extern "C" {

int hipdrt_impedance_lookup(hipdrt_ctx* ctx, double epsilon, int ngrid, int ny, const double* wt_re,
                            const double* wt_im, double* z_re, double* z_im) try {
    HIPDRT_REQUIRE(ctx && wt_re && wt_im && z_re && z_im, "NULL pointer");
    HIPDRT_REQUIRE(ngrid >= 2 && ny_ok(ny), "ngrid >= 2, 2 <= ny <= 6000");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf dwr, dwi, dzr, dzi;
    const size_t gb = (size_t)ngrid * sizeof(double);
    TRY(upload(dwr, wt_re, gb, st)); TRY(upload(dwi, wt_im, gb, st));
    HIPDRT_CHECK(dzr.alloc(gb)); HIPDRT_CHECK(dzi.alloc(gb));
    launch_lookup(st, epsilon, ngrid, ny, dwr.d(), dwi.d(), dzr.d(), dzi.d());
    LAUNCH_OK();
    HIPDRT_CHECK(hipMemcpyAsync(z_re, dzr.p, gb, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(z_im, dzi.p, gb, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_phasor_z_matrix(hipdrt_ctx* ctx, const double* freq, int nf, const double* basis_nu, int n_nu, double nu_epsilon,
                           double* zm_re, double* zm_im) try {
    HIPDRT_REQUIRE(ctx && freq && basis_nu && zm_re && zm_im, "NULL pointer");
    HIPDRT_REQUIRE(nf >= 1 && n_nu >= 1 && nu_epsilon > 0.0, "nf, n_nu >= 1, nu_epsilon > 0");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf df, dn, dr, di;
    TRY(upload(df, freq, (size_t)nf * sizeof(double), st));
    TRY(upload(dn, basis_nu, (size_t)n_nu * sizeof(double), st));
    const size_t ob = (size_t)nf * n_nu * sizeof(double);
    HIPDRT_CHECK(dr.alloc(ob)); HIPDRT_CHECK(di.alloc(ob));
    launch_phasor_z(st, df.d(), nf, dn.d(), n_nu, nu_epsilon, dr.d(), di.d());
    LAUNCH_OK();
    HIPDRT_CHECK(hipMemcpyAsync(zm_re, dr.p, ob, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(zm_im, di.p, ob, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_phasor_v_matrix(hipdrt_ctx* ctx, const double* times, int nt, const double* basis_nu, int n_nu, double nu_epsilon,
                           const double* step_times, const double* step_sizes, int nsteps, double* rm, double* layered) try {
    HIPDRT_REQUIRE(ctx && times && basis_nu && step_times && step_sizes && rm, "NULL pointer");
    HIPDRT_REQUIRE(nt >= 1 && n_nu >= 1 && nsteps >= 1 && nu_epsilon > 0.0, "nt, n_nu, nsteps >= 1, nu_epsilon > 0");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf dt, dn, ds, da, dr, dl;
    TRY(upload(dt, times, (size_t)nt * sizeof(double), st));
    TRY(upload(dn, basis_nu, (size_t)n_nu * sizeof(double), st));
    TRY(upload(ds, step_times, (size_t)nsteps * sizeof(double), st));
    TRY(upload(da, step_sizes, (size_t)nsteps * sizeof(double), st));
    const size_t ob = (size_t)nt * n_nu * sizeof(double);
    HIPDRT_CHECK(dr.alloc(ob));
    if (layered) HIPDRT_CHECK(dl.alloc(ob * nsteps));
    launch_phasor_v(st, dt.d(), nt, dn.d(), n_nu, nu_epsilon, ds.d(), da.d(), nsteps, dr.d(), layered ? dl.d() : nullptr);
    LAUNCH_OK();
    HIPDRT_CHECK(hipMemcpyAsync(rm, dr.p, ob, hipMemcpyDeviceToHost, st));
    if (layered) HIPDRT_CHECK(hipMemcpyAsync(layered, dl.p, ob * nsteps, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_chrono_var_matrix(hipdrt_ctx* ctx, const double* tt, int nt, const int* seg, int nseg, double vmm_epsilon,
                             int uniform, double* vmm) try {
    HIPDRT_REQUIRE(ctx && tt && seg && vmm, "NULL pointer");
    HIPDRT_REQUIRE(nt >= 1 && nseg >= 1, "nt >= 1, nseg >= 1");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf dtt, dseg, dv;
    TRY(upload(dtt, tt, (size_t)nt * sizeof(double), st));
    TRY(upload(dseg, seg, (size_t)(nseg + 1) * sizeof(int), st));
    HIPDRT_CHECK(dv.alloc((size_t)nt * nt * sizeof(double)));
    launch_chrono_vmm(st, dtt.d(), nt, dseg.i(), nseg, vmm_epsilon, uniform, dv.d());
    LAUNCH_OK();
    HIPDRT_CHECK(hipMemcpyAsync(vmm, dv.p, (size_t)nt * nt * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_response_lookup(hipdrt_ctx* ctx, double epsilon, int ngrid, int ny, const double* td, double* v) try {
    HIPDRT_REQUIRE(ctx && td && v, "NULL pointer");
    HIPDRT_REQUIRE(ngrid >= 2 && ny_ok(ny), "ngrid >= 2, 2 <= ny <= 6000");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf dtd, dv;
    const size_t gb = (size_t)ngrid * sizeof(double);
    TRY(upload(dtd, td, gb, st));
    HIPDRT_CHECK(dv.alloc(gb));
    launch_response_lookup(st, epsilon, ngrid, ny, dtd.d(), dv.d());
    LAUNCH_OK();
    HIPDRT_CHECK(hipMemcpyAsync(v, dv.p, gb, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
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
    DevBuf dt, dtau, dst, dsa, lut3, da, dl;
    TRY(upload(dt, times, (size_t)nt * sizeof(double), st));
    TRY(upload(dtau, tau, (size_t)ntau * sizeof(double), st));
    TRY(upload(dst, step_times, (size_t)nsteps * sizeof(double), st));
    TRY(upload(dsa, step_sizes, (size_t)nsteps * sizeof(double), st));
    if (mode == HIPDRT_MODE_INTERP) {
        const size_t gb = (size_t)ngrid * sizeof(double);
        HIPDRT_CHECK(lut3.alloc(3 * gb));
        HIPDRT_CHECK(hipMemcpyAsync(lut3.d(), log_td, gb, hipMemcpyHostToDevice, st));
        HIPDRT_CHECK(hipMemcpyAsync(lut3.d() + ngrid, v, gb, hipMemcpyHostToDevice, st));
        launch_lookup_slopes(st, ngrid, lut3.d(), lut3.d() + ngrid, lut3.d() + 2 * (size_t)ngrid);
    }
    const size_t ab = (size_t)nt * ntau * sizeof(double);
    HIPDRT_CHECK(da.alloc(ab));
    if (layered) HIPDRT_CHECK(dl.alloc(ab * nsteps));
    launch_response_matrix(st, dt.d(), nt, dtau.d(), ntau, dst.d(), dsa.d(), nsteps, mode, epsilon, ngrid, lut3.d(), ny,
                           da.d(), layered ? dl.d() : nullptr);
    LAUNCH_OK();
    HIPDRT_CHECK(hipMemcpyAsync(a, da.p, ab, hipMemcpyDeviceToHost, st));
    if (layered) HIPDRT_CHECK(hipMemcpyAsync(layered, dl.p, ab * nsteps, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
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
    DevBuf dt, dtau, dst, dsa, dtr, da, dl;
    TRY(upload(dt, times, (size_t)nt * sizeof(double), st));
    TRY(upload(dtau, tau, (size_t)ntau * sizeof(double), st));
    TRY(upload(dst, step_times, (size_t)nsteps * sizeof(double), st));
    TRY(upload(dsa, step_sizes, (size_t)nsteps * sizeof(double), st));
    if (variant == HIPDRT_RESPONSE_EXPDECAY) TRY(upload(dtr, tau_rise, (size_t)nsteps * sizeof(double), st));
    const size_t ab = (size_t)nt * ntau * sizeof(double);
    HIPDRT_CHECK(da.alloc(ab));
    if (layered) HIPDRT_CHECK(dl.alloc(ab * nsteps));
    launch_response_variant(st, dt.d(), nt, dtau.d(), ntau, dst.d(), dsa.d(), dtr.d(), nsteps, variant, epsilon, ny, da.d(),
                            layered ? dl.d() : nullptr);
    LAUNCH_OK();
    HIPDRT_CHECK(hipMemcpyAsync(a, da.p, ab, hipMemcpyDeviceToHost, st));
    if (layered) HIPDRT_CHECK(hipMemcpyAsync(layered, dl.p, ab * nsteps, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

// lut6 = {log_wt_re, z_re, slope_re, log_wt_im, z_im, slope_im}
static int build_lut6(hipStream_t st, DevBuf& lut6, int ngrid, const double* log_wt_re, const double* z_re,
                      const double* log_wt_im, const double* z_im, bool z_on_device) {
    const size_t gb = (size_t)ngrid * sizeof(double);
    if (!lut6.p) HIPDRT_CHECK(lut6.alloc(6 * gb));
    double* base = lut6.d();
    const hipMemcpyKind zk = z_on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    HIPDRT_CHECK(hipMemcpyAsync(base, log_wt_re, gb, hipMemcpyHostToDevice, st));
    HIPDRT_CHECK(hipMemcpyAsync(base + 3 * (size_t)ngrid, log_wt_im, gb, hipMemcpyHostToDevice, st));
    if (z_re) HIPDRT_CHECK(hipMemcpyAsync(base + ngrid, z_re, gb, zk, st));
    if (z_im) HIPDRT_CHECK(hipMemcpyAsync(base + 4 * (size_t)ngrid, z_im, gb, zk, st));
    launch_lookup_slopes(st, ngrid, base, base + ngrid, base + 2 * (size_t)ngrid);
    launch_lookup_slopes(st, ngrid, base + 3 * (size_t)ngrid, base + 4 * (size_t)ngrid, base + 5 * (size_t)ngrid);
    LAUNCH_OK();
    return 0;
}

static int impedance_matrix_common(hipdrt_ctx* ctx, int B, int freq_batched, const double* freq, int nf,
                                   const double* tau, int ntau, int mode, int toeplitz, double epsilon, int ngrid,
                                   const double* log_wt_re, const double* z_re, const double* log_wt_im,
                                   const double* z_im, int ny, double* a_re_dev, double* a_im_dev, int repeat,
                                   float* elapsed_ms) {
    HIPDRT_REQUIRE(ctx && freq && tau && a_re_dev && a_im_dev, "NULL pointer");
    HIPDRT_REQUIRE(B >= 1 && nf >= 1 && ntau >= 1, "B, nf, ntau >= 1");
    HIPDRT_REQUIRE(mode == HIPDRT_MODE_INTERP || mode == HIPDRT_MODE_TRAPZ, "mode");
    HIPDRT_REQUIRE(!(toeplitz && freq_batched), "Toeplitz shortcut needs one shared frequency grid");
    HIPDRT_REQUIRE(toeplitz || B <= kGridDimMax, "B <= 65535 spectra in one general build");
    if (mode == HIPDRT_MODE_INTERP)
        HIPDRT_REQUIRE(log_wt_re && z_re && log_wt_im && z_im && impedance_ngrid_ok(ngrid),
                       "interp needs lookups with ngrid >= 2 that one workgroup's LDS holds (2 <= ngrid <= 3406)");
    else HIPDRT_REQUIRE(ny_ok(ny), "2 <= ny <= 6000");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf dfreq, dtau, lut6, cr;
    TRY(upload(dfreq, freq, (size_t)(freq_batched ? B : 1) * nf * sizeof(double), st));
    TRY(upload(dtau, tau, (size_t)ntau * sizeof(double), st));
    if (mode == HIPDRT_MODE_INTERP) TRY(build_lut6(st, lut6, ngrid, log_wt_re, z_re, log_wt_im, z_im, false));
    HIPDRT_CHECK(cr.alloc(((size_t)(freq_batched ? B : 1) * nf + 2 * (size_t)(nf + ntau)) * sizeof(double)));
    hipEvent_t e0 = nullptr, e1 = nullptr;
    if (elapsed_ms) { HIPDRT_CHECK(hipEventCreate(&e0)); HIPDRT_CHECK(hipEventCreate(&e1)); HIPDRT_CHECK(hipEventRecord(e0, st)); }
    for (int r = 0; r < (repeat < 1 ? 1 : repeat); ++r)
        launch_impedance_matrix(st, B, freq_batched, dfreq.d(), nf, dtau.d(), ntau, mode, toeplitz, epsilon, ngrid,
                                lut6.d(), ny, a_re_dev, a_im_dev, cr.d());
    LAUNCH_OK();
    if (elapsed_ms) { HIPDRT_CHECK(hipEventRecord(e1, st)); }
    HIPDRT_CHECK(hipStreamSynchronize(st));
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
                                   log_wt_re, z_re, log_wt_im, z_im, ny, (double*)a_re_dev, (double*)a_im_dev, repeat,
                                   elapsed_ms);
} HIPDRT_CATCH

int hipdrt_impedance_matrix(hipdrt_ctx* ctx, int B, int freq_batched, const double* freq, int nf, const double* tau,
                            int ntau, int mode, int toeplitz, double epsilon, int ngrid, const double* log_wt_re,
                            const double* z_re, const double* log_wt_im, const double* z_im, int ny, double* a_re,
                            double* a_im) try {
    HIPDRT_REQUIRE(ctx && a_re && a_im, "NULL pointer");
    HIPDRT_REQUIRE(B >= 1 && nf >= 1 && ntau >= 1, "B, nf, ntau >= 1");
    TRY(enter(ctx));
    DevBuf dre, dim;
    const size_t bytes = (size_t)B * nf * ntau * sizeof(double);
    HIPDRT_CHECK(dre.alloc(bytes)); HIPDRT_CHECK(dim.alloc(bytes));
    TRY(impedance_matrix_common(ctx, B, freq_batched, freq, nf, tau, ntau, mode, toeplitz, epsilon, ngrid, log_wt_re,
                                z_re, log_wt_im, z_im, ny, dre.d(), dim.d(), 1, nullptr));
    HIPDRT_CHECK(hipMemcpy(a_re, dre.p, bytes, hipMemcpyDeviceToHost));
    HIPDRT_CHECK(hipMemcpy(a_im, dim.p, bytes, hipMemcpyDeviceToHost));
    return HIPDRT_OK;
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
    DevBuf dy, dsg, dso, dseg, dnodes, dnd, dw, dwo, drad, dout;
    TRY(upload(dy, y, (size_t)n * sizeof(double), st));
    TRY(upload(dsg, sigma, (size_t)n * sizeof(double), st));
    TRY(upload(dso, seg_of.data(), (size_t)n * sizeof(int), st));
    TRY(upload(dseg, seg, (size_t)(nseg + 1) * sizeof(int), st));
    TRY(upload(dnodes, nodes, (size_t)nseg * K * sizeof(double), st));
    TRY(upload(dnd, node_delta, (size_t)nseg * sizeof(double), st));
    TRY(upload(dw, weights, (size_t)nweights * sizeof(double), st));
    TRY(upload(dwo, woff, (size_t)nseg * K * sizeof(int), st));
    TRY(upload(drad, radius, (size_t)nseg * K * sizeof(int), st));
    HIPDRT_CHECK(dout.alloc((size_t)n * sizeof(double)));
    launch_nonuniform_gauss(st, dy.d(), n, dsg.d(), dso.i(), dseg.i(), dnodes.d(), K, dnd.d(), dw.d(), dwo.i(), drad.i(),
                            dout.d());
    LAUNCH_OK();
    HIPDRT_CHECK(hipMemcpyAsync(out, dout.p, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_penalty_matrices(hipdrt_ctx* ctx, const double* ln_tau, int n, double epsilon, int toeplitz, double* m0,
                            double* m1, double* m2) try {
    HIPDRT_REQUIRE(ctx && ln_tau && m0 && m1 && m2, "NULL pointer");
    HIPDRT_REQUIRE(n >= 1, "n >= 1");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf dl, d0, d1, d2;
    const size_t bytes = (size_t)n * n * sizeof(double);
    TRY(upload(dl, ln_tau, (size_t)n * sizeof(double), st));
    HIPDRT_CHECK(d0.alloc(bytes)); HIPDRT_CHECK(d1.alloc(bytes)); HIPDRT_CHECK(d2.alloc(bytes));
    launch_penalty(st, dl.d(), n, epsilon, toeplitz, d0.d(), d1.d(), d2.d(), n, 0);
    LAUNCH_OK();
    HIPDRT_CHECK(hipMemcpyAsync(m0, d0.p, bytes, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(m1, d1.p, bytes, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(m2, d2.p, bytes, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_eis_var_matrix(hipdrt_ctx* ctx, const double* freq, int nf, double vmm_epsilon, double reim_cor,
                          int uniform, double* vmm) try {
    HIPDRT_REQUIRE(ctx && freq && vmm, "NULL pointer");
    HIPDRT_REQUIRE(nf >= 1, "nf >= 1");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf df, dv;
    const size_t bytes = (size_t)4 * nf * nf * sizeof(double);
    TRY(upload(df, freq, (size_t)nf * sizeof(double), st));
    HIPDRT_CHECK(dv.alloc(bytes));
    launch_eis_vmm(st, df.d(), nf, vmm_epsilon, reim_cor, uniform, dv.d());
    LAUNCH_OK();
    HIPDRT_CHECK(hipMemcpyAsync(vmm, dv.p, bytes, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_qp_batch(hipdrt_ctx* ctx, int B, int n, int p_batched, const double* P, const double* q, int h_batched,
                    const double* h, const hipdrt_qp_opts* opts, double* x, int* iters, double* pcost, int* status) try {
    HIPDRT_REQUIRE(ctx && P && q && h && x && status, "NULL pointer");
    HIPDRT_REQUIRE(B >= 1 && n >= 1 && n <= 4096, "B >= 1, 1 <= n <= 4096");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf dP, dq, dh, dL, dx, dit, dpc, dst, dstate, dPpk, dgs;
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
    HIPDRT_CHECK(dx.alloc((size_t)B * n * sizeof(double)));
    HIPDRT_CHECK(dit.alloc((size_t)B * sizeof(int)));
    HIPDRT_CHECK(dpc.alloc((size_t)B * sizeof(double)));
    HIPDRT_CHECK(dst.alloc((size_t)B * sizeof(int)));
    QpArgs a{};
    a.B = B; a.n = n; a.P = dP.d(); a.p_stride = p_batched ? (long long)n * ldp : 0; a.ldp = ldp;
    a.q = dq.d(); a.h = dh.d(); a.h_stride = h_batched ? n : 0;
    a.L = dL.d(); a.ldl = ldl; a.l_stride = (long long)qp_scratch_doubles(n, G);
    a.x = dx.d(); a.iters = dit.i(); a.pcost = dpc.d(); a.status = dst.i();
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
    HIPDRT_CHECK(hipMemcpyAsync(x, dx.p, (size_t)B * n * sizeof(double), hipMemcpyDeviceToHost, st));
    if (iters) HIPDRT_CHECK(hipMemcpyAsync(iters, dit.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    if (pcost) HIPDRT_CHECK(hipMemcpyAsync(pcost, dpc.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(status, dst.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_weighted_gram(hipdrt_ctx* ctx, int B, int m, int n, const double* A, const double* w, const double* b,
                         int l2_batched, const double* l2, const double* l1, double* P, double* q) try {
    HIPDRT_REQUIRE(ctx && A && w && b && P && q, "NULL pointer");
    HIPDRT_REQUIRE(B >= 1 && m >= 1 && n >= 1, "B, m, n >= 1");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf dA, dw, db, dl2, dl1, dP, dq;
    TRY(upload(dA, A, (size_t)m * n * sizeof(double), st));
    TRY(upload(dw, w, (size_t)B * m * sizeof(double), st));
    TRY(upload(db, b, (size_t)B * m * sizeof(double), st));
    if (l2) TRY(upload(dl2, l2, (size_t)(l2_batched ? B : 1) * n * n * sizeof(double), st));
    if (l1) TRY(upload(dl1, l1, (size_t)n * sizeof(double), st));
    HIPDRT_CHECK(dP.alloc((size_t)B * n * n * sizeof(double)));
    HIPDRT_CHECK(dq.alloc((size_t)B * n * sizeof(double)));
    // one shared A, every problem, row-major P only; L2 as given (none: l2 = NULL)
    PqArgs pq{};
    pq.B = B; pq.m = m; pq.n = n; pq.A = dA.d(); pq.lda = n; pq.w = dw.d();
    pq.P = dP.d(); pq.ldp = n; pq.p_stride = (long long)n * n;
    pq.y = db.d(); pq.l1 = l1 ? dl1.d() : nullptr; pq.q = dq.d();
    GramL2 g{};
    g.l2 = l2 ? dl2.d() : nullptr; g.l2_stride = l2_batched ? (long long)n * n : 0; g.ldl2 = n;
    launch_gram_l2(st, pq, g);
    launch_qvec(st, pq);
    LAUNCH_OK();
    HIPDRT_CHECK(hipMemcpyAsync(P, dP.p, (size_t)B * n * n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(q, dq.p, (size_t)B * n * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_func_eval_matrix(hipdrt_ctx* ctx, const double* basis_grid, int nb, const double* eval_grid, int ne, double epsilon,
                            int order, double* out) try {
    HIPDRT_REQUIRE(ctx && basis_grid && eval_grid && out, "NULL pointer");
    HIPDRT_REQUIRE(nb >= 1 && ne >= 1, "nb, ne >= 1");
    HIPDRT_REQUIRE(order >= 0 && order <= 2, "order must be 0, 1 or 2");
    hipStream_t st; TRY(enter(ctx, &st));
    DevBuf db, de, dout;
    TRY(upload(db, basis_grid, (size_t)nb * sizeof(double), st));
    TRY(upload(de, eval_grid, (size_t)ne * sizeof(double), st));
    HIPDRT_CHECK(dout.alloc((size_t)ne * nb * sizeof(double)));
    TRY(func_eval_dev(st, db.d(), nb, de.d(), ne, epsilon, order, 1.0, dout.d(), nb));
    HIPDRT_CHECK(hipMemcpyAsync(out, dout.p, (size_t)ne * nb * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

}  // extern "C"
