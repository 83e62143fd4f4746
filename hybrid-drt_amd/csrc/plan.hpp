// Internal declarations shared by the host-side translation units of the C-ABI (api.hip, operators.hip, debug.hip, plan.hip,
// plan_fit.hip, plan_post.hip, plan_drt.hip): the plan itself, the entry points' error handling, the table of an entry point's
// optional outputs, and the few functions that cross those files.  Never included by a kernel file: what those see is common.hpp.
#pragma once
#include <memory>
#include <mutex>
#include <new>
#include <stdexcept>

#include "common.hpp"
#include "pfrt_store.hpp"

using namespace hipdrt;

#define TRY(expr) do { int _rc = (expr); if (_rc) return _rc; } while (0)
#define LAUNCH_OK() HIPDRT_CHECK(hipGetLastError())

// No exception may cross the C ABI: every entry point is a function-try-block.  (Host-side std::vector buffers -- an
// n x n identity of 134 MB at n = 4096, download staging, the Toeplitz reach scan of plan creation -- can throw std::bad_alloc.)
#define HIPDRT_CATCH                                                                                              \
    catch (const std::bad_alloc&) { hipdrt::set_error("out of host memory"); return HIPDRT_E_HIP; }                \
    catch (const std::exception& e) { hipdrt::set_error(std::string("internal error: ") + e.what()); return HIPDRT_E_HIP; } \
    catch (...) { hipdrt::set_error("internal error"); return HIPDRT_E_HIP; }

// every entry point that touches the device starts here: the context's device current, no sticky error left over from an
// earlier call, and (when asked for) the context's stream
inline int enter(hipdrt_ctx* ctx, hipStream_t* st = nullptr) {
    HIPDRT_CHECK(hipSetDevice(ctx->device)); (void)hipGetLastError();
    if (st) *st = ctx->stream;
    return HIPDRT_OK;
}

// an entry point's options: the caller's, or the defaults of the public initialiser
template <class O>
O opts_or(const O* given, void (*dflt)(O*)) {
    O o;
    if (given) o = *given; else dflt(&o);
    return o;
}

inline int upload(DevBuf& buf, const void* src, size_t bytes, hipStream_t st) {
    HIPDRT_CHECK(buf.alloc(bytes));
    if (src) HIPDRT_CHECK(hipMemcpyAsync(buf.p, src, bytes, hipMemcpyHostToDevice, st));
    return 0;
}

inline int copy_strided(double* out, const double* dev, int rows, int cols, int ld, hipStream_t st) {
    HIPDRT_CHECK(hipMemcpy2DAsync(out, (size_t)cols * sizeof(double), dev, (size_t)ld * sizeof(double),
                                  (size_t)cols * sizeof(double), rows, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return 0;
}

// The device twins of the optional host outputs of one entry point.  One want() per output, in the order of the argument list;
// one back() after the launch queues every copy to the host in that order.  (A fixed array: a DevBuf must not move.)
struct DevOuts {
    static constexpr int MAX = 12;         // hipdrt_plan_find_peaks has 11
    DevBuf buf[MAX];
    void* host[MAX] = {};
    int n = 0;
    // `count` elements of T on the device for the host array h, and the kernel argument that points at them; a null h does
    // nothing and leaves the field null, unless the kernel needs the array whatever the caller asked for (force)
    template <class T>
    int want(T* h, size_t count, T*& field, bool force = false) {
        if (!h && !force) return HIPDRT_OK;
        HIPDRT_REQUIRE(n < MAX, "internal: more optional outputs than DevOuts holds");
        HIPDRT_CHECK(buf[n].alloc(count * sizeof(T)));
        field = buf[n].as<T>(); host[n++] = h;
        return HIPDRT_OK;
    }
    int back(hipStream_t st) const {
        for (int i = 0; i < n; ++i)
            if (host[i]) HIPDRT_CHECK(hipMemcpyAsync(host[i], buf[i].p, buf[i].bytes, hipMemcpyDeviceToHost, st));
        return HIPDRT_OK;
    }
};

// +1: strictly descending, -1: strictly ascending, 0: neither
inline int freq_monotone(const double* f, int nf) {
    if (nf < 2) return 1;
    const int dir = f[0] > f[1] ? 1 : -1;
    for (int i = 0; i + 1 < nf; ++i)
        if (!(dir > 0 ? f[i] > f[i + 1] : f[i] < f[i + 1])) return 0;
    return dir;
}

namespace hipdrt {
// ---- api.hip: the library's own streams (StreamPool) and the life cycle of contexts -----------------------------------------
// k streams for the ranges of one fit, the least busy first (more ranges than streams: they repeat), and their return
void pool_borrow(int device, int k, int* idx, hipStream_t* st);
void pool_return(int device, int k, const int* idx);
int pool_size(int device);
struct LoopOnContextStream {       // RAII: "a device loop runs on this context's stream" for the ranges of other fits to avoid
    hipdrt_ctx* c;
    explicit LoopOnContextStream(hipdrt_ctx* c_);
    ~LoopOnContextStream();
};
extern std::mutex g_life;          // context / plan creation and destruction (any thread, e.g. a garbage collector's)
void free_ctx(hipdrt_ctx* ctx);    // (under g_life) a released context whose last plan is gone

// ---- operators.hip --------------------------------------------------------------------------------------------------------
hipdrt_qp_opts default_qp_opts();
// out_dev[i * ld + j] = fac * phi^(order)(ev_i - basis_j) (launch_func_eval with the two constants as Python forms them)
int func_eval_dev(hipStream_t st, const double* basis_dev, int nb, const double* ev_dev, int ne, double eps, int order,
                  double fac, double* out_dev, int ld);
}  // namespace hipdrt

// ---- the plan ---------------------------------------------------------------------------------------------------------------
// What a sub-batch view shares with its parent, copied whole (plan.hip: make_view): dimensions and leading dimensions, mode and
// structure flags, options.  A scalar that every range of a fit must see the same belongs HERE, not beside it in hipdrt_plan.
struct PlanShape {
    int nf = 0, ntau = 0, n = 0, m = 0, ns = 0, ngrid = 0, ny = 0, mode = 0, toeplitz_a = 0, toeplitz_m = 0;
    int idx_rinf = -1, idx_induc = -1;
    int ldrm = 0, ldm = 0, ldp = 0, ldl = 0;
    double eps = 0;
    hipdrt_fit_opts opts{};
    int toep_maxd = -1;     // reach of the Toeplitz penalty blocks in grid points (plan_toep_reach), -1 = not determined
    int spec_zero = 0;      // the special-parameter rows / columns of the penalty matrices are zero outside the special block
    int qp_G = 0;           // workgroups per QP when the plan is full (qp_group_size at its capacity): 0 = the batch kernel
};

struct hipdrt_plan : PlanShape {
    hipdrt_ctx* ctx = nullptr;
    int freq_order = 0;        // +1: the frequency grid is strictly descending, -1: strictly ascending, 0: neither (kk_screen refuses)
    int capacity = 0, B = 0;
    // prepared-matrix plans (hipdrt_plan_create_prepared)
    int prepared = 0;
    int prepped = 0;           // launch_prep has run on the staged batch (hipdrt_plan_iterate runs it once)
    hipdrt_prepared_desc desc{};
    long long rm_stride = 0;
    DevBuf vz_strength, dop_rho, dop_xmx, hist_dop_rho, outlier_t, vz_entry;
    // weight factors (hipdrt_plan_set_weight_factors): w_eff = w * row factor * weight_factor is what the QP sees
    double weight_factor = 1.0;
    int wrow_batched = 0;
    int wrow_late = 0;      // row factors are a vector-valued weight_factor: applied from the second iteration on only
    DevBuf wrow, w_eff, h_init, wfac;
    bool has_weight_factors() const { return weight_factor != 1.0 || wrow.p != nullptr; }
    // shared
    DevBuf freq, tau, ln_tau, wt_re, wt_im, lut6, a_re, a_im, cr, rm, mk[3], vmm, h, l1;
    // per spectrum
    DevBuf z_re, z_im, rv, w, est_w, x, x_in, q, s, rho, xmx, coef_scale, var_floor;
    DevBuf active, outer_iters, fit_status, qp_iters_total, qp_status, qp_iters, n_active, pcost;
    DevBuf premv;          // [3][capacity][m]: hyper-parameter step of few, large fits (hyper.hip, premv_kernel)
    DevBuf L, Ptmp, qpstate, Ppk, order, vmm_base, gsync;
    // tau basis of a prepared plan (hipdrt_plan_set_tau_basis): ln(basis_tau) [basis_nb] and its epsilon, for hipdrt_plan_predict_drt
    DevBuf basis_ln_tau;
    int basis_nb = 0;
    double basis_eps = 0;
    // prediction description of a prepared plan (hipdrt_plan_set_predict_desc): what its special columns mean and the post-fit
    // scales of the staged batch -- dop_scale_vector [B][dop_size] (solve_rp rescales it per member), v_baseline_scale [vb_size]; coefficient scale, response signal
    // scale and scaled response offset [B]
    int pd_set = 0, pd_idx_rinf = -1, pd_idx_induc = -1, pd_idx_cinv = -1;
    double pd_inductance_scale = 0, pd_capacitance_scale = 0;
    DevBuf pd_dop_scale, pd_vb_scale, pd_cs, pd_rss, pd_sro;
    // The kernel is chosen per fit from the number of spectra actually staged: a plan sized for a thousand spectra that is
    // handed one or a handful runs them on several workgroups each, inside the scratch it already has.
    void qp_layout(int B, QpArgs& qa) const {
        int G = qp_group_size(B, n, ctx ? ctx->qp_force_group : -1);
        const size_t have_l = L.bytes / sizeof(double), have_s = qpstate.bytes / sizeof(double);
        if (G >= 1 && G != qp_G) {
            const bool fits = gsync.p && (size_t)B * qp_scratch_doubles(n, G) <= have_l &&
                              (size_t)B * G * qp_state_doubles(n) <= have_s && (size_t)B * qp_gsync_ints() * sizeof(int) <= gsync.bytes;
            if (!fits) G = qp_G;
        } else if (G < 1) {
            G = qp_G;            // (a plan created for few spectra keeps its group layout when it is full)
        }
        qa.G = G; qa.gsync = gsync.i(); qa.l_stride = (long long)qp_scratch_doubles(n, G);
        qa.waves = ctx ? ctx->qp_waves : -1;
    }
    // The plan's own operands of the weighted normal equations, for the weights `wq` [B][m]: every staged spectrum that is
    // still active, its P as packed tiles in its slot of Ppk, its q from rv and the plan's l1 vector.  A call site states only
    // what differs.
    PqArgs pq(const double* wq) const {
        PqArgs a{};
        a.B = B; a.m = m; a.n = n; a.A = rm.d(); a.lda = ldrm; a.a_stride = rm_stride; a.w = wq; a.active = active.i();
        a.P = nullptr; a.ldp = ldp; a.p_stride = (long long)n * ldp; a.Ppk = Ppk.d(); a.ppk_stride = (long long)qp_ppk_doubles(n);
        a.y = rv.d(); a.l1 = l1.d(); a.l1_scalar = 0.0; a.q = q.d();
        return a;
    }
    // ... of spectrum b alone, `wb` [m] being that spectrum's weights: one problem on its own response matrix and its own slot
    // of Ppk, every stride 0, whether it is still active or not (P only: y and q stay the batch's)
    PqArgs pq_one(int b, const double* wb) const {
        PqArgs a = pq(wb);
        a.B = 1; a.A += (size_t)b * rm_stride; a.Ppk += (size_t)b * qp_ppk_doubles(n);
        a.a_stride = a.p_stride = a.ppk_stride = 0; a.active = nullptr;
        return a;
    }
    // history
    int hist_b = -1, hist_cap = 0;
    DevBuf hist_x, hist_w, hist_rho, hist_qp, hist_rows;
    // PFRT step store (hipdrt_plan_pfrt_begin / _record): the state every step of a PFRT fit ended with, sized for the plan's capacity
    // -- x [S][capacity][n], rho and dop_rho [S][capacity][3], s [S][capacity][3][n], the two likelihood sums and the fit status
    // [S][capacity] -- and how many steps are in it
    int pf_max = 0, pf_steps = 0;
    DevBuf pf_x, pf_rho, pf_dop_rho, pf_s, pf_rss, pf_slw, pf_status;
    hipdrt::PfrtStoreLayout pf_layout() const { return {(size_t)capacity, (size_t)n}; }
    // timings of the last fit
    float t_ms[5] = {0, 0, 0, 0, 0};
    int launches[5] = {0, 0, 0, 0, 0};
    // sub-batches of one fit (hipdrt_plan_set_subbatches): the staged spectra split into `k` contiguous ranges, every range
    // fitted by the same device loop on its own stream, all inside ONE hipdrt_plan_fit call and the plan's own buffers
    int subbatches = 0;                                   // 0 = automatic (subbatch_count), >= 1 fixed
    std::vector<std::unique_ptr<struct hipdrt_subfit>> subs;
    DevBuf n_active_sub;                                  // one "still active" counter per sub-batch
    hipdrt_plan() = default;
    ~hipdrt_plan();

    FitState state() const {
        FitState st{};
        st.nf = nf; st.m = m; st.n = n; st.ns = ns; st.ldrm = ldrm; st.ldm = ldm; st.toeplitz_m = toeplitz_m;
        st.toep_reach = (toeplitz_m && !(ctx && !ctx->zero_shortcuts)) ? toep_maxd : -1;
        st.opts = opts; st.continue_mode = 0; st.min_iter = 1;
        st.basis_area = prepared ? desc.basis_area : (eps > 0 ? hipdrt::basis_area(eps) : 0.0);
        st.prepared = prepared; st.desc = desc; st.rm_stride = rm_stride; st.rm_rw = rm.d();
        st.vz_strength = vz_strength.d(); st.vz_entry = nullptr; st.dop_rho = dop_rho.d(); st.dop_xmx = dop_xmx.d();
        st.hist_dop_rho = hist_dop_rho.d(); st.outlier_t = outlier_t.d();
        st.rm = rm.d(); st.vmm = vmm.d(); st.vmm_iw = vmm_base.p ? vmm_base.d() : vmm.d();
        for (int k = 0; k < 3; ++k) st.mk[k] = mk[k].d();
        st.z_re = z_re.d(); st.z_im = z_im.d();
        st.rv = rv.d(); st.w = w.d(); st.est_w = est_w.d();
        st.x = x.d(); st.x_in = x_in.d(); st.s = s.d(); st.rho = rho.d(); st.xmx = xmx.d();
        st.coef_scale = coef_scale.d(); st.var_floor = var_floor.d();
        st.active = active.i(); st.outer_iters = outer_iters.i(); st.fit_status = fit_status.i();
        st.qp_iters_total = qp_iters_total.i(); st.qp_status = qp_status.i(); st.qp_iters = qp_iters.i();
        st.n_active = n_active.i();
        st.hist_b = hist_b; st.hist_cap = hist_cap;
        st.hist_x = hist_x.d(); st.hist_w = hist_w.d(); st.hist_rho = hist_rho.d();
        st.hist_qp = hist_qp.i(); st.hist_rows = hist_rows.i();
        st.premv = nullptr; st.premv_batched = 0;
        return st;
    }
};

// one sub-batch of a plan: a plan object whose buffers are windows into the parent's, with a stream of its own
struct hipdrt_subfit {
    hipdrt_ctx ctx;
    hipdrt_plan view;
    int rc = 0;
    std::string err;
    // (ctx.stream is borrowed from the library's pool for the duration of one fit: hipdrt_plan_fit)
};
inline hipdrt_plan::~hipdrt_plan() = default;

namespace hipdrt {
// plan.hip: one range of a plan's staged batch as a plan of its own; history buffers for `rows` outer iterations
int make_view(hipdrt_plan* p, hipdrt_subfit& sf, int idx, int b0, int nb);
int plan_hist_reserve(hipdrt_plan* p, int rows);
// plan_fit.hip: L2 part of P in hyper-parameter form for the plan's current state
// (dop_derivative_weights null: the plan's own)
GramL2 plan_l2(const hipdrt_plan* p, double l2_lambda_0, const double* derivative_weights, double dop_l2_lambda_0,
               const double* dop_derivative_weights = nullptr);

// ---- Kramers-Kronig screening: plan_post.hip (hipdrt_plan_kk_screen) and its stage-B test hook in debug.hip --------------------
int kk_check_opts(const hipdrt_kk_opts& o);

// ---- plan_post.hip: the fitted state and its final P, for the posterior entry points there and the DRT chain of plan_drt.hip ------
// Where a posterior computation reads the fitted state from: the plan's live buffers (what the last fit or warm restart left), or
// one recorded step of the PFRT store with the raw re-estimated weights of that step (step_source).  All [B]-major with the
// strides of the live buffers.
struct PostSource { const double *x, *s, *rho, *dop_rho, *w; const int* fit_status; };
PostSource live_source(const hipdrt_plan* p);
PostSource step_source(const hipdrt_plan* p, int step, const double* w, const int* fit_status);
// What the posterior entry points call "the final P": calculate_pq with the final weights / s / rho (drt1d.py:1006), from
// calculate_pq's scaled_weights -- w_eff whenever the plan has weight factors.  b >= 0: s, rho, dop_rho and the weights of
// spectrum b alone.
struct FinalP { GramL2 g; const double* w; };
FinalP plan_final_p(const hipdrt_plan* p, int b, const PostSource& src);
// out[n][n] (host) = the final P `f` of spectrum b, formed row-major in Ptmp without a packed copy; synchronises the stream
int plan_final_p_to_host(hipdrt_plan* p, hipStream_t st, int b, const FinalP& f, double* out);
// rows_dev[neval][ncol] in device memory (it sits at columns col_offset.. of the unknown vector, zero elsewhere) ->
// dout[nb][nex * 16] = rows_i' P^-1 rows_i (not yet scaled by cs^2) and dstat[nb], of spectrum b alone (nb = 1) or, b = -1, of
// the batch (nb = B).  The caller owns the scratch: Y = rows L^-T of the last factorisation stays in it.
// dop_sinv (null: P as it is): every member's image of P is scaled to S_b P_b S_b on the plan's DOP block first (launch_scale_p), so
// that the forms are rows_i' D_b P_b^-1 D_b rows_i with D_b = diag(dop_scale_vector_b); dop_sinv [B][dop_size] on the device, 1 / D of
// EVERY member of the batch, whatever b.  The image is rebuilt for every call: nothing of the fit is touched.
int plan_quadratic_forms_dev(hipdrt_plan* p, const PostSource& src, int b, const double* rows_dev, int neval, int ncol,
                             int col_offset, DevBuf& scratch, DevBuf& dout, DevBuf& dstat, const double* dop_sinv = nullptr);
// status[b] = the fit's status fit[b], or HIPDRT_PREDICT_NOT_PD where the fit is good and the variance factorisation failed
// (var[b] != 0; var null: no variances were formed).  status may be fit itself.
inline void merge_status(int B, const int* fit, const int* var, int* status) {
    for (int b = 0; b < B; ++b) status[b] = (fit[b] >= 0 && var && var[b] != 0) ? HIPDRT_PREDICT_NOT_PD : fit[b];
}
// The device chain behind that, from packed P and device rows on -- what plan_quadratic_forms_dev runs once it has built P, and
// what hipdrt_debug_posterior runs on a P of the caller's: rows -> packed tiles (bex), then cov_kernel_resident over the spectra in
// chunks of at most 256 (one factor scratch per spectrum of a chunk).  `single`: the single-spectrum form (nb = 1, every stride 0).
// Spectrum k of a chunk has its scratch at scratch + guard + k * (dist_var_scratch_doubles + guard) doubles; with guard > 0 (the
// hook) the whole buffer is filled with the bytes 0xA5 first, so that what lies between the spectra's scratch shows a stray write.
struct PosteriorChain {
    int nb, n;
    const double* ppk; long long pstr;          // packed final P; pstr 0: one P for every spectrum
    bool single;
    const double* rows; int neval, ncol, col_offset;
    double* bex;                                // [nex][nchp][256]
    double* var; int* status;                   // [nb][16 nex], [nb]
    size_t guard = 0;
    int nex() const { return (neval + 15) / 16; }
};
int posterior_var_dev(hipStream_t st, const PosteriorChain& c, DevBuf& scratch);
// logdet[nb], status[nb] (device) of nb packed matrices, through launch_logdet in chunks of at most 256 with one factor scratch per
// matrix of a chunk; `scratch` is grown when it is too small and otherwise reused, so that a second call costs no allocation
int logdet_dev(hipStream_t st, int nb, int n, const double* ppk, long long pstr, DevBuf& scratch, double* logdet, int* status);
// scale * Y Y' of the rows Y = rows L^-T that the chain left behind ONE spectrum's factor (scratch_b: that spectrum's scratch)
// -> dcov[neval][neval] on the device
void posterior_cov_dev(hipStream_t st, const double* scratch_b, int n, int neval, double scale, double* dcov);
// host side of the variances: out[nb][neval] from the device's [nb][16 nex], times scale[b] (scale NULL: 1)
inline void posterior_var_host(const double* var, int nb, int neval, const double* scale, double* out) {
    const int nex = (neval + 15) / 16;
    for (int b = 0; b < nb; ++b)
        for (int i = 0; i < neval; ++i) out[(size_t)b * neval + i] = var[((size_t)b * nex) * 16 + i] * (scale ? scale[b] : 1.0);
}
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

// ---- plan_response.hip: the voltage response of a prepared plan's batch, and its test hook in debug.hip ---------------------------
// Everything on the device: X [B][ldx] scaled solutions with the DRT block at column ns (copies = 2: positive copy, negative copy),
// U [S nt][ntau] unit-step layers, Ud [S nt][dop_size] unit phasor layers applied to Xd [B][dop_size], every member's DOP block times
// its own dop_scale_vector (launch_scale_block; Ud or Xd null: no DOP term).  a carries sizes, scales, vectors, mask and out; T / Tn /
// Td / ldt are set here from the three scratch buffers, which the caller keeps until the stream has been synchronised.
int response_chain(hipStream_t st, int B, int ntau, int copies, int ns, const double* U, const double* Ud, const double* Xd,
                   int dop_size, ResponseArgs a, DevBuf& t, DevBuf& tn, DevBuf& td);

// ---- plan_drt.hip: the DRT chain (prediction, peaks, per-peak resolution, PFRT) and the test hooks of its kernels in debug.hip ----
// the tau basis a prediction evaluates: the plan's own grid, or what hipdrt_plan_set_tau_basis gave a prepared plan
struct PredictBasis { const double* ln_tau; int nb, copies; double eps; };
int predict_basis(const hipdrt_plan* p, PredictBasis& pb);
// host checks of the caller's peak source: index rows [B][max_peaks] in range, strictly increasing, -1 only as padding at the
// end; windows 0 <= start < min(end, nfind), starts and ends ascending
int peak_resolve_check_source(int source, const int* indices, int B, int max_peaks, const int* win_start, const int* win_end,
                              int nwin, int nfind);
// what launch_pfrt_combine takes from the options and the number of data rows m; sizes, strides and pointers are the caller's
PfrtCombineArgs pfrt_combine_args(const hipdrt_pfrt_opts& o, int m);
}  // namespace hipdrt

