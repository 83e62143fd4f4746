// Internal declarations shared by the HIP translation units of libhipdrt.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <string>
#include <vector>

#include "../../include/hipdrt.h"
#include "../../include/hipdrt_debug.h"
#include "lds_layout.hpp"

namespace hipdrt {

void set_error(const std::string& msg);

#define HIPDRT_CHECK(expr)                                                                     \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) {                                                                \
            hipdrt::set_error(std::string(#expr) + ": " + hipGetErrorString(_e) + " (" +       \
                              __FILE__ + ":" + std::to_string(__LINE__) + ")");                \
            return HIPDRT_E_HIP;                                                               \
        }                                                                                      \
    } while (0)

#define HIPDRT_REQUIRE(cond, msg)                                                              \
    do {                                                                                       \
        if (!(cond)) {                                                                         \
            hipdrt::set_error(std::string("invalid argument: ") + msg);                        \
            return HIPDRT_E_INVALID;                                                           \
        }                                                                                      \
    } while (0)

// RAII device buffer (freed on destruction; the ctx/plan own these)
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    bool own = true;          // false: a window into another buffer (sub-batch views of a plan), never freed here
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    ~DevBuf() { release(); }
    void release() {
        if (p && own) (void)hipFree(p);
        p = nullptr;
        bytes = 0;
        own = true;
    }
    hipError_t alloc(size_t n) {
        release();
        if (n == 0) n = 8;
        hipError_t e = hipMalloc(&p, n);
        if (e == hipSuccess) bytes = n;
        return e;
    }
    // window [offset, offset + n) of `src` (nothing when src is empty)
    void alias(const DevBuf& src, size_t offset, size_t n) {
        release();
        if (!src.p) return;
        p = static_cast<char*>(src.p) + offset;
        bytes = n;
        own = false;
    }
    template <class T>
    T* as() const { return static_cast<T*>(p); }
    double* d() const { return static_cast<double*>(p); }
    int* i() const { return static_cast<int*>(p); }
};

inline int round_up(int v, int m) { return (v + m - 1) / m * m; }

// raise kernel f's dynamic-LDS limit to `bytes` (`what` names the kernel in the error message)
inline int set_lds_limit(const void* f, size_t bytes, const char* what) {
    const hipError_t e = hipFuncSetAttribute(f, hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) { set_error(std::string("hipFuncSetAttribute(") + what + "): " + hipGetErrorString(e)); return HIPDRT_E_HIP; }
    return HIPDRT_OK;
}
// the tail of a launcher with dynamic LDS: the attribute is raised only above the 64 KiB a kernel may have without it (the launchers
// of matrices.hip do without it: their kernels launch at up to kLdsLimit all the same, tests/test_gpu_matrices_edges.py)
inline int set_lds(const void* f, size_t bytes, const char* what) {
    return bytes <= 64 * 1024 ? 0 : set_lds_limit(f, bytes, what);
}

// per-workgroup LDS of a gfx950 CU, less the static part; and the refusal of a launch that needs more (dims: the sizes that decide it)
static constexpr size_t kLdsLimit = 160 * 1024 - 256;
inline int lds_check(size_t bytes, const char* who, const char* dims) {
    if (bytes <= kLdsLimit) return HIPDRT_OK;
    set_error(std::string("invalid argument: ") + who + ": " + std::to_string(bytes) + " bytes of LDS needed (" + dims + "), " +
              std::to_string(kLdsLimit) + " available");
    return HIPDRT_E_INVALID;
}

// What the matrix builders (matrices.hip) accept, each from the layout its kernel stages in LDS: trapezoid points (the interface's
// 6000, which the y tables must hold), knots of the impedance lookups (at the fewest rows a workgroup of the general build takes --
// launch_impedance_matrix gives up rows for a long table, so that an accepted table builds at every batch size) and knots of the
// response lookup.  kGridDimMax: what a launch may put on gridDim.y or .z -- the kernels stride over rows, a longer batch is refused.
static constexpr int kNyMax = 6000;
static constexpr int kInterpMinRows = 4, kInterpMaxRows = 256;
static constexpr int kGridDimMax = 65535;
inline bool ny_ok(int ny) { return ny >= 2 && ny <= kNyMax && y_tables_lds(nullptr, ny).bytes <= kLdsLimit; }
inline bool impedance_ngrid_ok(int ngrid) {
    return ngrid >= 2 && ngrid <= (1 << 20) && impedance_interp_lds(nullptr, ngrid, kInterpMinRows).bytes <= kLdsLimit;
}
inline bool response_ngrid_ok(int ngrid) {
    return ngrid >= 2 && ngrid <= (1 << 20) && response_interp_lds(nullptr, ngrid).bytes <= kLdsLimit;
}

// A lookup buffer holds `ntables` tables back to back, each {x, f, slope}[ngrid]: lut6 = the impedance lookups {ln(omega tau), Z',
// slope} then {ln(omega tau), Z'', slope}, lut3 = the response lookup {ln(t / tau), v, slope}.  Table k of buffer `base`:
template <class T>
struct LutPart { T *x, *f, *slope; };
template <class T>
HIPDRT_HD __forceinline__ LutPart<T> lut_part(T* base, int ngrid, int k) {
    // ngrid <= 2^20 (impedance_ngrid_ok, response_ngrid_ok): int offsets, each formed on its own as the kernels always formed them
    return LutPart<T>{base + 3 * k * ngrid, base + (3 * k + 1) * ngrid, base + (3 * k + 2) * ngrid};
}
HIPDRT_HD inline size_t lut_doubles(int ngrid, int ntables) { return (size_t)3 * ngrid * ntables; }
// host side of table k: the buffer allocated on first use, then the host's abscissae and values copied in, each where given; the
// slopes follow from launch_lut_slopes
inline int stage_lut(hipStream_t st, DevBuf& lut, int ngrid, int ntables, int k, const double* x, const double* f) {
    if (!lut.p) HIPDRT_CHECK(lut.alloc(lut_doubles(ngrid, ntables) * sizeof(double)));
    const LutPart<double> T = lut_part(lut.d(), ngrid, k);
    const size_t gb = (size_t)ngrid * sizeof(double);
    if (x) HIPDRT_CHECK(hipMemcpyAsync(T.x, x, gb, hipMemcpyHostToDevice, st));
    if (f) HIPDRT_CHECK(hipMemcpyAsync(T.f, f, gb, hipMemcpyHostToDevice, st));
    return HIPDRT_OK;
}

// area of one tau basis function: sqrt(pi) / epsilon
inline double basis_area(double eps) { return 1.7724538509055159 / eps; }

}  // namespace hipdrt

struct hipdrt_ctx {
    int device = 0;
    hipStream_t stream = nullptr;      // one of the library's own streams (api.hip: StreamPool), held for the context's lifetime
    int pool_idx = -1;
    int num_cu = 0;
    size_t hbm_bytes = 0;
    std::string arch;
    // lifetime: plans refer to their context, and a garbage collector may release the two in either order -- a released
    // context lives on until its last plan is destroyed
    int plans = 0;
    bool released = false;
    // hipdrt_debug_qp_group (include/hipdrt_debug.h; tests): workgroups per problem of this context's coneqp launches,
    // -1 = the library chooses
    int qp_force_group = -1;
    // hipdrt_debug_exact_zero_shortcuts (tests): 0 = the Gram epilogue and the hyper kernel visit the penalty matrices' exact
    // zeros as well (no reach restriction, no tile skip)
    int zero_shortcuts = 1;
    // hipdrt_debug_qp_waves (tests, tools): wavefronts per workgroup of this context's batch coneqp launches at n <= 528 --
    // 4 = the fat form, 8 = eight wavefronts, -1 = the library chooses.  Initialised from HIPDRT_QP_WAVES when the context is made.
    int qp_waves = -1;
    // hipdrt_debug_candidate_form (tests): how this context's candidate scoring keeps yh = X rm' between its two products --
    // 0 = in LDS, 1 = through the scratch buffer, -1 = the library chooses (LDS where 16 rows of m fit)
    int cand_form = -1;
    // hipdrt_debug_last_predict_ms (tools): kernel time of the last prediction, ms -- [0] up to the mean / the impedance, [1] band included
    float predict_ms[2] = {0.f, 0.f};
    // hipdrt_debug_map_filter_stats (tools): launches, full-array reads + writes and device ms of the last hipdrt_map_filter
    double map_filter_stats[3] = {0.0, 0.0, 0.0};
    double map_badness_ms = 0.0;      // hipdrt_debug_map_badness_ms (tools): device ms of the last hipdrt_map_badness
};

// ---- launchers implemented in the .hip files (all asynchronous on `st`) ---------------------------------
namespace hipdrt {

// api.hip: the library's own streams (one per hardware queue) exist from here on
void ensure_stream_pool(int device);

// matrices.hip
void launch_lookup(hipStream_t st, double eps, int ngrid, int ny, const double* wt_re, const double* wt_im,
                   double* z_re, double* z_im);
// slope[j] = (f[j + 1] - f[j]) / (x[j + 1] - x[j]) of the first `ntables` tables of a lookup buffer (lut_part)
void launch_lut_slopes(hipStream_t st, double* base, int ngrid, int ntables);
// lut6: the two impedance lookups (lut_part), device; scratch: impedance_scratch_doubles(...) doubles of the same arguments
void launch_impedance_matrix(hipStream_t st, int B, int freq_batched, const double* freq, int nf, const double* tau,
                             int ntau, int mode, int toeplitz, double eps, int ngrid, const double* lut6, int ny,
                             double* a_re, double* a_im, double* scratch);
size_t impedance_scratch_doubles(int B, int freq_batched, int nf, int ntau, int mode, int toeplitz);
// the general interp build's launch form: threads per row, rows per workgroup and dynamic LDS (launch_impedance_matrix and
// hipdrt_debug_impedance_interp_form both ask here)
void impedance_interp_form(int B, int nf, int ntau, int ngrid, int* tpr, int* rpb, size_t* lds_bytes);
void launch_phasor_z(hipStream_t st, const double* freq, int nf, const double* nu, int nnu, double eps, double* zre,
                     double* zim);
void launch_phasor_v(hipStream_t st, const double* times, int nt, const double* nu, int nnu, double eps,
                     const double* step_times, const double* step_sizes, int nsteps, double* rm, double* layered);
void launch_chrono_vmm(hipStream_t st, const double* tt, int nt, const int* seg, int nseg, double eps, int uniform,
                       double* vmm);
void launch_response_lookup(hipStream_t st, double eps, int ngrid, int ny, const double* td, double* v);
void launch_response_matrix(hipStream_t st, const double* times, int nt, const double* tau, int ntau,
                            const double* step_times, const double* step_sizes, int nsteps, int mode, double eps,
                            int ngrid, const double* lut3, int ny, double* a, double* layered);
void launch_response_variant(hipStream_t st, const double* times, int nt, const double* tau, int ntau,
                             const double* step_times, const double* step_sizes, const double* tau_rise, int nsteps,
                             int variant, double eps, int ny, double* a, double* layered);
void launch_nonuniform_gauss(hipStream_t st, const double* y, int n, const double* sigma, const int* seg_of, const int* seg,
                             const double* nodes, int K, const double* node_delta, const double* weights, const int* woff,
                             const int* radius, double* out);
void launch_penalty(hipStream_t st, const double* ln_tau, int n, double eps, int toeplitz, double* m0, double* m1,
                    double* m2, int ld, int pad);
void launch_eis_vmm(hipStream_t st, const double* freq, int nf, double vmm_eps, double reim_cor, int uniform,
                    double* vmm);

// gram.hip
struct GramL2 {
    // explicit L2 (stand-alone API) ...
    const double* l2;
    long long l2_stride;
    int ldl2;
    // ... or hyper-parameter form (fit loop)
    const double* mk[3];   // padded penalty matrices [n][ldm]
    int ldm;
    const double* s;       // [B][3][n]
    const double* rho;     // [B][3]
    double dfac[3];        // l2_lambda_0 * derivative_weight[k]   (0 => order skipped)
    int ns;
    int use_rho;
    int sym;               // penalty matrices are bitwise symmetric (Toeplitz build): read them along rows
    int toep;              // the DRT block (indices >= ns) of every mk is symmetric Toeplitz: mk[i][j] = mk[ns][ns + |i - j|]
    int toep_maxd;         // largest |i - j| at which any order's first row is non-zero (-1: not known): the Gaussian penalties
                           // underflow to exactly 0 a few dozen grid points off the diagonal, so a tile further out adds exact zeros
    int spec_zero;         // every penalty entry that couples a special parameter with a DRT coefficient is exactly zero
    // x_dop block (qphb.py:92-100): entries with both indices in [dop_start, dop_start + dop_size) are scaled by
    // dop_dfac[k] * dop_rho[b][k] instead
    int dop_start, dop_size;
    const double* dop_rho; // [B][3]
    double dop_dfac[3];    // dop_l2_lambda_0 * dop_derivative_weight[k]
};
// The weighted normal equations of B problems (all pointers device memory): P_b = A_b' diag(w_b^2) A_b + L2_b for
// launch_gram_l2, which reads the first two blocks, and q_b = -A_b' diag(w_b^2) y_b + l1 for launch_qvec, which reads the first
// and the last.  A launcher ignores the block it does not read.
struct PqArgs {
    int B, m, n;          // problems, rows and columns of A
    const double* A;      // [B or 1][m][lda]
    int lda;
    long long a_stride;   // doubles between the matrices of consecutive problems (0 = one shared matrix)
    const double* w;      // [B][m]
    const int* active;    // [B] or null: problems with active[b] == 0 are left as they are
    // P: at least one of the two copies
    double* P;            // [B][n][ldp] row-major, or null
    int ldp;
    long long p_stride;   // doubles between consecutive problems' P
    double* Ppk;          // [B][nchp][nchp][256] lower 16 x 16 tiles in the QP factor's layout (nchp = qp_nchp(n)), or null
    long long ppk_stride; // doubles between consecutive problems' Ppk (qp_ppk_doubles(n) when they are packed one behind the other)
    // q
    const double* y;      // [B][m]
    const double* l1;     // [n] shared by all problems, or null: l1_scalar in every entry
    double l1_scalar;
    double* q;            // [B][n]
};
inline int qp_nchp(int n) { return round_up(n, 32) / 16; }
inline size_t qp_ppk_doubles(int n) { return (size_t)qp_nchp(n) * qp_nchp(n) * 256; }
void launch_gram_l2(hipStream_t st, const PqArgs& a, const GramL2& g);
void launch_qvec(hipStream_t st, const PqArgs& a);
void launch_qvec_batched(hipStream_t s, const PqArgs& a);     // hyper.hip: the shared-matrix form of launch_qvec
// row-major symmetric P [B][n][ldp] -> accumulator-native lower tiles Ppk [B][qp_ppk_doubles(n)]
void launch_pack_p(hipStream_t st, int B, int n, const double* P, int ldp, double* Ppk);

// hyper.hip: device-resident state of a batched fit (passed by value to the kernels)
struct FitState {
    int nf, m, n, ns, ldrm, ldm;
    int toeplitz_m;        // penalty blocks are symmetric Toeplitz (uniform ln-tau grid): first column suffices
    int toep_reach;        // ... and exactly zero beyond this distance from the diagonal in every order (-1: not known)
    int continue_mode;     // 1: warm restart (_continue_from_init): xmx norms stay frozen, no rescaling;
                           // 2: a bare iterate_qphb (hipdrt_plan_iterate): as 1 and no vz_offset column rewrite
    int min_iter;          // a spectrum may only stop once it has done this many outer iterations (fit: 1)
    double basis_area;     // area of one tau basis function (sqrt(pi) / epsilon): predict_r_p of update_scale
    hipdrt_fit_opts opts;
    // prepared-matrix plans (hipdrt_plan_create_prepared): any data type, optional x_dop block and vz_offset column
    int prepared;
    hipdrt_prepared_desc desc;
    long long rm_stride;   // doubles between the response matrices of consecutive spectra (0 = shared)
    double* rm_rw;         // == rm when the matrices are per spectrum (the vz_offset column is rewritten every iteration)
    const double* vz_strength;   // [m]
    const double* vz_entry;      // [B][m] or null: warm restarts (continue_mode 1) predict the vz_offset column from a matrix whose
                                 // offset column is frozen as it stood when the restart began (drt1d.py:1295-1298), not zero
    double *dop_rho, *dop_xmx;   // [B][3]
    double* outlier_t;           // [B][m] or null: 1 - posterior outlier probability of the last estimate_weights (outlier_p set)
    double* hist_dop_rho;
    // shared (plan) matrices
    const double* rm;      // [m][ldrm]  stacked [Re; Im] response matrix incl. special columns
    const double* vmm;     // [m][m]
    const double* vmm_iw;  // [m][m]  variance matrix of initialize_weights (self-excluded rows when outlier_p is set)
    const double* mk[3];   // [n][ldm]   padded penalty matrices
    // per-spectrum
    const double *z_re, *z_im;   // [B][nf]
    double *rv, *w, *est_w;      // [B][m]
    double *x, *x_in;            // [B][n]
    double* s;                   // [B][3][n]
    double *rho, *xmx;           // [B][3]
    double *coef_scale, *var_floor;   // [B]
    int *active, *outer_iters, *fit_status, *qp_iters_total, *qp_status, *qp_iters;   // [B]
    int* n_active;               // [1]
    // few, large fits: the three matrix-vector products of an outer iteration (rm @ x, vmm @ resid^2, rm @ x for the
    // vz_offset column) computed by a many-workgroup kernel before hyper_kernel, which then only reads them ([3][B][m], or null)
    double* premv;
    int premv_batched;     // premv is filled by batch_products_kernel (many fits sharing rm and vmm: two products on the matrix pipe)
    // optional history of one spectrum
    int hist_b, hist_cap;
    double *hist_x, *hist_w, *hist_rho;
    int *hist_qp, *hist_rows;
};
size_t hyper_lds_bytes(int n, int m, int ns);
bool hyper_lds_form(int n, int m, int ns, int toeplitz, bool outlier, int* form, size_t* lds_bytes);
int launch_prep(hipStream_t s, const FitState& st, int B);
// stage 0: weights from the first overfit only (outlier branch); stage 1: final est_weights -> init weights, x reset
// stage 2: est_weights of rows [r0, r1) only (init_weights_separately); stage 3: final step only
int launch_init_weights(hipStream_t s, const FitState& st, int B, int stage, int r0 = 0, int r1 = 0);
void launch_row_mask(hipStream_t s, int B, int m, int r0, int r1, double* w);
void launch_weight_method(hipStream_t s, const FitState& st, int B, double fixed_chrono, double fixed_eis, double* wrow,
                          double* wfac);
void launch_vmm_exclude_self(hipStream_t s, const double* vmm, int m, double* out);
int launch_hyper(hipStream_t s, const FitState& st, int B, int it);
int device_cus();      // compute units of the current device (qp.hip)
void launch_scale_weights(hipStream_t s, const FitState& st, int B, double factor);
void launch_scale_rows(hipStream_t s, int B, int m, const double* w, const double* rows, int batched, double factor,
                       const int* active, double* out);
void launch_copy_column(hipStream_t s, int B, int m, const double* rm, long long rm_stride, int ldrm, int col, double* out);
// w_out ([B][m] or null): the weights the sums were formed with
int launch_llh(hipStream_t s, const FitState& st, int B, double* rss, double* slw, int stored = 0, double scalar_w = 1.0,
               double* w_out = nullptr);
void launch_assemble_rm(hipStream_t s, const FitState& st, const double* a_re, const double* a_im, const double* freq,
                        double* rm, int idx_rinf, int idx_induc);
void launch_special_penalty(hipStream_t s, double* m0, double* m1, double* m2, int ld, int idx_rinf, int idx_induc,
                            double pen_r, double pen_l);
void launch_make_h(hipStream_t s, double* h, int n, int ns, int nonneg);

// kk.hip: Kramers-Kronig screening, one workgroup per spectrum (all pointers device memory; an output may be null)
struct KkArgs {
    int nf, p2;                   // frequencies; power of two >= 2 nf (set by launch_kk)
    int desc;                     // 1: freq is descending, 0: ascending
    const double* freq;           // [nf]
    hipdrt_kk_opts o;
    const double *in_re, *in_im;  // [B][nf] residuals for the stage-B-only launch
    double *z_re, *z_im;          // [B][nf] prediction in data units
    double *e_re, *e_im;          // [B][nf] residuals, percent of |Z|
    double* std;                  // [B]
    int* mask;                    // [B][nf]
    double* f_lim;                // [B][2] f_min, f_max
    int* i_lim;                   // [B][2] positions in descending-frequency order
    int* status;                  // [B]
    double* wrow;                 // [B][2 nf] or null: row factors of the next fit
};
size_t kk_lds_bytes(int nf, int n, int stage_a);
// st != null: both stages on the plan's state; null: stage B alone on a.in_re / a.in_im.  HIPDRT_E_INVALID when LDS cannot hold the shape.
int launch_kk(hipStream_t s, const FitState* st, KkArgs a, int B);

// matrices.hip: out[i * ld + j] = fac * phi^(order)(ev_i - basis_j), c1 = -2 eps^2, c2 = 4 eps^4 (formed by the caller)
void launch_func_eval(hipStream_t st, const double* basis, int nb, const double* ev, int ne, double eps, int order, double c1,
                      double c2, double fac, double* out, int ld);

// predict.hip: model evaluation for the fitted batch (all pointers device memory)
// out[b * ldo + i] = scale[b] * sum_j E[i * lde + j] * X[b * ldx + col_offset + j]; scale may be null (1), fit_status may be null
// (otherwise rows with a negative status become NaN)
void launch_apply_rows(hipStream_t st, int B, int K, const double* X, long long ldx, int col_offset, int r, const double* E,
                       int lde, const double* scale, const int* fit_status, double* out, long long ldo);
void launch_drt_sums(hipStream_t st, int B, const double* X, long long ldx, int col_offset, int nb, int copies, int sign,
                     double* sum_x, double* sum_abs);
void launch_drt_scalars(hipStream_t st, int B, const double* sum_x, const double* sum_abs, const double* cs, double area,
                        int normalize, int absolute, const double* X, long long ldx, int idx_rinf, double* r_p, double* r_inf,
                        double* r_tot, double* norm, double* scale);
void launch_drt_band(hipStream_t st, int B, int r, const double* mu, const double* var, long long ldv, const double* cs,
                     const double* norm, double s_lo, double s_hi, const int* var_status, const int* fit_status, double* lo,
                     double* hi);
void launch_z_assemble(hipStream_t st, int B, int nf, const double* y, const double* X, long long ldx, int idx_rinf,
                       int idx_induc, const double* cs, double inductance_scale, const double* freq, int mask,
                       const int* fit_status, double* z_re, double* z_im);
// response_assemble_kernel (predict.hip): the voltage response of every member from the step-wise products T = cs U x.  All
// pointers are device memory; a null T / Tn / Td / vector leaves its term out.
struct ResponseArgs {
    int S, nt, mask;                       // steps, prediction times, HIPDRT_INCLUDE_* bits
    const double *T, *Tn, *Td;             // [B][ldt], entry s * nt + i: DRT block (positive copy), negative copy, DOP block
    long long ldt;
    const double* sizes; int sizes_batched;    // [S] or [B][S]
    const double* X; long long ldx;        // the scaled solutions
    const double *cs, *rss, *sro;          // [B] coefficient scale, response signal scale, scaled response offset (null: 0)
    int idx_rinf, idx_cinv, vz_index, vb_start, vb_size;
    double capacitance_scale;
    const double* inf_rv; int inf_batched;     // [nt] or [B][nt]
    const double* cap_rv; int cap_batched;
    const double *strength, *vb_mat, *vb_scale;    // [nt], [nt][vb_size], [vb_size]
    const int* fit_status;
    double* out;                           // [B][nt]
};
void launch_response_assemble(hipStream_t st, int B, const ResponseArgs& a);
// z_model_assemble_kernel (predict.hip): the impedance of every member of a prepared plan from Y = cs [A'; A''] x
struct ZModelArgs {
    int nf, mask;                          // HIPDRT_INCLUDE_* bits
    const double *Y, *Yn, *Yd;             // [B][2 nf]: DRT block (positive copy), negative copy, DOP block; null: term left out
    const double* X; long long ldx;
    const double* cs;
    int idx_rinf, idx_induc, idx_cinv, vz_index;
    double inductance_scale, capacitance_scale;
    const double *freq, *strength;         // [nf]; strength null: no vz-offset factor
    const int* fit_status;
    double *z_re, *z_im;                   // [B][nf]
};
void launch_z_model_assemble(hipStream_t st, int B, const ZModelArgs& a);
// dop_assemble_kernel (predict.hip): normalisation and ideal elements of the distribution of phasances, in place
struct DopArgs {
    int nn, include_ideal;
    double* dop;                           // [B][nn]
    const double *nu, *norm;               // [nn]; norm null: not normalised
    double basis_area;
    const double* X; long long ldx;
    const double* cs;
    int idx_rinf, idx_induc, idx_cinv;
    double inductance_scale, capacitance_scale;
    const int* fit_status;
};
void launch_dop_assemble(hipStream_t st, int B, const DopArgs& a);
// out[b][j] = X[b][col + j] * v[b][j], out and v [B][nd]: every member's DOP block times its own dop_scale_vector
void launch_scale_block(hipStream_t st, int B, int nd, const double* X, long long ldx, int col, const double* v, double* out);
// The posterior of the distribution of phasances (predict.hip).  sinv[b][j] = 1.0 / dsv[b][j] (dsv_stride 0: one shared vector; an
// entry that is not finite and positive gives 1: the caller has refused it, or the member's rows are NaN anyway)
void launch_dop_recip(hipStream_t st, int B, int nd, const double* dsv, long long dsv_stride, double* sinv);
// scale_p_kernel: the congruence S_b P_b S_b on the packed lower tiles Ppk [B][nchp][nchp][256] in place, S_b = diag(s) with
// s = sinv[b] on the unknowns dop_start .. dop_start + dop_size - 1 and 1 elsewhere.  B = 1 with both strides 0: one member's image
// and that member's own row of sinv.
void launch_scale_p(hipStream_t st, int B, int n, int dop_start, int dop_size, const double* sinv, long long sinv_stride,
                    double* Ppk, long long ppk_stride);
// dop_band_kernel: lo, hi [B][nn] = mu + s sigma, sigma = sqrt(var cs^2) / norm[i], and var_out [B][nn] = var cs^2 / norm[i]^2 in
// data units (norm null: 1; each output may be null); NaN where var_status != 0 or fit_status < 0
void launch_dop_band(hipStream_t st, int B, int nn, const double* mu, const double* var, long long ldv, const double* cs,
                     const double* norm, double s_lo, double s_hi, const int* var_status, const int* fit_status, double* lo,
                     double* hi, double* var_out);

// peaks.hip: peak finding on evaluated rows, one workgroup per spectrum (all pointers device memory; an output may be null)
struct PeakArgs {
    int neval, p2;                       // p2: power of two >= neval (set by launch_peaks)
    hipdrt_peak_opts o;
    const double *fxx, *f;               // [B][neval]; f may be null unless search = 0 or method = 2
    const double *var_fxx, *var_f;       // [B][ldv] e' inv(P) e (methods 1, 2 / method 2), scaled by cs^2 / norm^2 while staged
    long long ldv;
    const double *cs, *norm;             // [B] or null (1)
    const int *fit_status, *var_status;  // [B] or null: a negative fit status / a non-zero variance status empties the spectrum
    int *peak_sign, *keep;               // [B][neval]
    double *heights, *prominences, *probs;
    int *left_bases, *right_bases;
    int* count;                          // [B]
    double* used_prominence;             // [B]
    double *peak_prob, *curv_prob;       // [B][neval], method 2
};
int peak_check_opts(const hipdrt_peak_opts& o, int neval);
size_t peaks_lds_bytes(int neval, int method, int need_f, int num_peaks);    // need_f: search = 0 or method = 2
// HIPDRT_E_INVALID when the options are out of range, a row the mode reads is missing, or LDS cannot hold the rows; nothing is launched then
int launch_peaks(hipStream_t s, PeakArgs a, int B);
void launch_scale_mul(hipStream_t s, int B, const double* x, const double* y, double* out);

// peak_prob.hip: peak and trough probabilities of evaluated rows and the search on their product, one workgroup per spectrum
// (all pointers device memory; an output may be null)
struct PeakProbArgs {
    int neval, p2, nranges;              // p2: power of two >= neval (set by launch_peak_prob); nranges counts for search 2 only
    hipdrt_peak_prob_opts o;
    const double *f, *fx, *fxx;          // [B][neval] orders 0, 1, 2
    const double *var_f, *var_fx, *var_fxx;   // [B][ldv] e' inv(P) e (bayes_cov), scaled by cs^2 while staged
    long long ldv;
    const double* cs;                    // [B] or null (1)
    const double* prob_in;               // [B][neval] or null: the search runs on this row, nothing else is read or formed
    const int *fit_status, *var_status;  // [B] or null: a negative fit status / a non-zero variance status empties the spectrum
    const int *range_lo, *range_hi;      // [nranges] index windows [lo, hi] of search 2
    double *pp, *tp, *prob;              // [B][neval]
    double* sigma;                       // [3][B][neval]
    int* keep;                           // [B][neval]
    double *heights, *prominences;
    int *left_bases, *right_bases;
    int* count;                          // [B]
    int* range_peaks;                    // [B][nranges]
};
size_t peak_prob_lds_bytes(int neval);
// the options, the windows and the LDS need of neval: HIPDRT_E_INVALID for what the kernel cannot take
int peak_prob_check(const hipdrt_peak_prob_opts& o, int neval, int nranges, const int* range_lo, const int* range_hi);
int launch_peak_prob(hipStream_t s, PeakProbArgs a, int B);

// peak_resolve.hip: per-peak coefficients, distributions and resistances, one workgroup per spectrum (all pointers device memory;
// an output may be null)
struct PeakResolveArgs {
    int nfind, nb, nout, max_peaks, ld;  // max_peaks and ld (leading dimension of the LDS operand) are set by the launcher
    int source;                          // 0: the keep rows of peaks_kernel, 1: index rows, 2: one peak per window (argmin fxx)
    int nwin, copies;                    // copies of the basis in the DRT block (1, or 2: x+ | x-)
    hipdrt_peak_resolve_opts o;
    const double *f, *fxx;               // [B][nfind] unnormalised rows on the find grid
    const int* keep;                     // [B][nfind]
    const int* indices;                  // [B][max_peaks], -1 padded, strictly increasing
    const int *win_start, *win_end;      // [nwin] windows [start, end) of the find grid (end may pass it by one)
    const double* X;                     // [B][ldx] the unknowns; the DRT block starts at col_offset
    long long ldx;
    int col_offset;
    const double* cs;                    // [B] coefficient scale, or null (1)
    const double *lt, *lb, *lto;         // ln of the find grid [nfind], of the basis grid [nb], of the output grid [nout]
    const double* E0;                    // [nout][nb] order-0 evaluation matrix of the output grid
    double basis_area;                   // sqrt(pi) / epsilon of the basis
    const int* fit_status;               // [B] or null
    int *count, *status;                 // [B]
    int *peak_index, *trough_index;      // [B][max_peaks]
    double *eps_l, *eps_r, *r_peaks, *r_coef;   // [B][max_peaks]
    double* x_peaks;                     // [B][max_peaks][nb]
    double* peak_gammas;                 // [B][max_peaks][nout]
};
int peak_resolve_check_opts(const hipdrt_peak_resolve_opts& o);
size_t peak_resolve_lds_bytes(int nfind, int nb, int nout, int max_peaks);
// HIPDRT_E_INVALID, before any launch, when an option is out of range, an input the source needs is missing, or LDS cannot hold the shape
int launch_peak_resolve(hipStream_t s, PeakResolveArgs a, int B);
// out[b][k] = trapezoid of mu[b][start_k : end_k] over ln_tau (windows clipped to the grid)
void launch_window_trapz(hipStream_t s, int B, int n, int nwin, const double* mu, const double* lt, const int* win_start,
                         const int* win_end, double* out);

// pfrt.hip: the probability function of relaxation times on evaluated rows, one workgroup per spectrum (all pointers device memory)
struct PfrtStepArgs {
    int neval;
    double floor;                        // lower bound of both variances (<= 0: none)
    int ext_left, ext_right;             // extend_var's clamp indices, -1 = off
    const int* peak_sign;                // [B][neval] of peaks_kernel (method 0)
    const double *heights, *prominences; // [B][neval] of peaks_kernel
    const double* f;                     // [B][neval]
    const double *var_f, *var_fxx;       // [B][ldv] e' inv(P) e, scaled by cs^2 / norm^2 as they are read
    long long ldv;
    const double *cs, *norm;             // [B] or null (1)
    const int *fit_status, *var_status;  // [B] or null: a negative fit status / a non-zero variance status gives a NaN row
    double* out;                         // [B][neval]
    int* bad;                            // [B] or null: set to 1 where var_status is non-zero
};
int launch_pfrt_step(hipStream_t s, const PfrtStepArgs& a, int B);
struct PfrtCombineArgs {
    int S, np, nout;                     // steps, points of tau_pfrt, points of the output grid (== np without smoothing)
    long long ld_step, ld_sum;           // doubles between consecutive steps of step_pfrt (B * np) and of rss / slw
    const double* step_pfrt;             // [S][B][np]
    const double *rss, *slw;             // [S][ld_sum] the two likelihood sums of every step (launch_llh, stored = 0)
    const double* ln_factors;            // [S]
    double c, alpha_n, beta_0;           // llh = (c - alpha_n ln(beta_0 + rss / 2)) + slw
    double prior_mu, prior_sigma, n_eff;
    int smooth;
    double smooth_order, smooth_eps;
    int integrate;
    double thr;
    int normalize;
    const double *ltp, *lto;             // ln(tau_pfrt) [np], ln(tau_out) [nout] (read with smooth only)
    const int *fit_status, *bad;         // [B] or null: a negative status / a non-zero flag gives NaN rows
    double *pfrt, *raw, *post;           // [B][nout], [B][np], [S][B]; any may be null
};
size_t pfrt_combine_lds_bytes(int S, int np, int nout);
// every check of hipdrt_plan_predict_pfrt's options and grids (HIPDRT_E_INVALID: more than 2048 points on a grid, ...)
int pfrt_check(const hipdrt_pfrt_opts& o, int S, int np, int nout);
int launch_pfrt_combine(hipStream_t s, const PfrtCombineArgs& a, int B);
// c, alpha_n and beta_0 of PfrtCombineArgs for m data rows (evaluate_llh's defaults alpha_0 = 2, beta_0 = 1)
void pfrt_llh_consts(int m, double* c, double* alpha_n, double* beta_0);
// pfrt_select_kernel: pfrt.select_candidates (hybdrt/models/pfrt.py:164-213) on the raw PFRT and the steps' rows of every spectrum
struct PfrtSelectArgs {
    int S, np, max_peaks;
    long long ld_step, ld_sum;           // as PfrtCombineArgs
    const double* raw;                   // [B][np]
    const double* step_pfrt;             // [S][B][np]
    const double *rss, *slw;             // [S][ld_sum]
    double c, alpha_n, beta_0;           // llh = (c - alpha_n ln(beta_0 + rss / 2)) + slw
    double start_thresh, end_thresh, peak_thresh;
    const int *fit_status, *bad;         // [B] or null: a negative status / a non-zero flag leaves every slot unused
    int *num_peaks, *first, *num_candidates;       // [B] each; any output may be null
    int *ranked_index, *step_index;      // [B][max_peaks]: unused slots hold -1
    double *magnitude, *match_quality;   // [B][max_peaks]: unused slots hold NaN
    int* status;                         // [B]: 0, HIPDRT_PFRT_NO_PEAK or HIPDRT_PFRT_TOO_MANY_PEAKS (required)
};
// the limits of hipdrt_plan_pfrt_select beyond pfrt_check's: thresholds that are numbers, 1 <= max_peaks <= 64
int pfrt_select_check(const hipdrt_pfrt_select_opts& o);
int launch_pfrt_select(hipStream_t s, const PfrtSelectArgs& a, int B);

// candidates.hip: the likelihood sums of C candidate solutions per spectrum, 16 candidates of a spectrum per workgroup on the
// matrix pipe, and the compaction of peaks_kernel's dense rows (all pointers device memory)
struct CandLlhArgs {
    int C, B, m, n;
    const double* x;                     // candidate (c, b): x + c * x_cstride + b * x_bstride, n doubles
    long long x_cstride, x_bstride;
    const double* rm; int ldrm; long long rm_stride;   // [m][ldrm]; doubles between consecutive spectra (0 = shared)
    const double* rv;                    // [B][m]
    const double* vmm;                   // [m][m]
    const double* var_floor;             // [B]
    const int* ncand;                    // [B] or null (C): slots at or past it get NaN
    const int* fit_status;               // [B] or null: a negative status gives NaN in every slot
    const int* slot_status;              // [C][B] or null: a negative entry gives NaN in that slot (a recorded step that failed)
    double *rss, *slw;                   // [C][B]
    double* scratch;                     // form 1: cand_llh_scratch_doubles(C, B, m) doubles
};
bool cand_llh_fits_lds(int m);           // 16 rows of rm x fit in LDS beside the staging slabs (form 0)
size_t cand_llh_scratch_doubles(int C, int B, int m);
// form 0: yh = X rm' stays in LDS; 1: it goes through a.scratch between two launches.  Same bits either way.
int launch_cand_llh(hipStream_t st, const CandLlhArgs& a, int form);
inline int cand_llh_form(const hipdrt_ctx* ctx, int m) { return ctx->cand_form >= 0 ? ctx->cand_form : (cand_llh_fits_lds(m) ? 0 : 1); }
struct CandPeakArgs {
    int B, neval, max_peaks;
    const int* keep;                                     // [B][neval] of peaks_kernel
    const double *dense_heights, *dense_prominences;     // [B][neval] of peaks_kernel (read only where the list is asked for)
    const int* slot_status;                              // [B]: negative = no candidate in this slot
    int* count;                                          // [B]; any output may be null
    int* peak_index;                                     // [B][max_peaks], -1 padded
    double *heights, *prominences;                       // [B][max_peaks], NaN padded
    int* status;                                         // [B]
};
void launch_cand_compact(hipStream_t st, const CandPeakArgs& a);

// lml.hip: the sums of the log marginal likelihood (qphb.py:1279-1344), one workgroup per spectrum (all pointers device memory; an
// output may be null).  With r = rm_b x_b: wy2 = |w y|^2, fit2 = |w r|^2, cross = sum w^2 r y, slw = sum log w, xox = x' Omega x
// for the Omega that launch_gram_l2 forms from `g` (the lower triangle of every M_k, mirrored), l1x = l1' x.
struct LmlSumsArgs {
    int m, n, ldrm;
    const double* rm; long long rm_stride;   // [m][ldrm]; doubles between consecutive spectra (0 = shared)
    const double *rv, *w;                    // [B][m]
    const double* x;                         // [B][n]
    GramL2 g;                                // mk, ldm, s, rho, dfac, ns and the DOP block; l2 is not read
    const double* l1;                        // [n] or null (l1x = 0)
    const int* fit_status;                   // [B] or null: a negative status gives NaN in every sum
    double *wy2, *fit2, *cross, *slw, *xox, *l1x;   // [B]
};
size_t lml_sums_lds_bytes(int n, int m);
int launch_lml_sums(hipStream_t st, const LmlSumsArgs& a, int B);

// qp.hip
struct QpArgs {
    int B, n;
    const double* P;      // [B or 1][n][ldp]
    long long p_stride;   // 0 if shared
    int ldp;
    const double* Ppk;    // optional [B or 1][nchp][nchp][256]: P in accumulator-native 16x16 tiles (lower tiles)
    long long ppk_stride; // 0 if shared
    int nchp;
    const double* q;      // [B][n]
    const double* h;      // [B or 1][n]
    long long h_stride;
    double* L;            // scratch [B][n_pad][ldl]
    int ldl;
    long long l_stride;
    double* x;            // [B][n] out
    int* iters;           // [B] out (may be null)
    double* pcost;        // [B] out (may be null)
    int* status;          // [B] out
    const int* active;    // [B] or null: skip problems with active[b]==0
    const int* order = nullptr;   // [B] or null: workgroup i solves problem order[i] (longest-first dispatch)
    int* iters_accum;     // [B] or null: += iterations
    double* state;        // scratch [B * max(G, 1)][17][state_ld] for the IPM iterates (one copy per member of a group)
    int state_ld;
    long long state_stride;
    hipdrt_qp_opts opts;
    // G >= 1: the group kernel (qp_group.hpp), every problem on G co-resident workgroups (qp_group_size picks G when the
    // buffers are sized); 0: the batch kernel, one workgroup per problem
    int G = 0;
    int* gsync = nullptr; // [B][qp_gsync_ints()] global sync words of the groups (zeroed by the launcher)
    int redo_aborted = 0; // group kernel: only the problems whose status is HIPDRT_QP_ABORTED (second pass of launch_qp)
    int waves = 0;        // batch kernel, n <= 528: 4 = the fat form (four wavefronts x 512 registers), anything else = eight wavefronts
};
int launch_qp(hipStream_t st, const QpArgs& a);
// workgroups per problem for a launch of B problems of n unknowns: 0 = batch kernel (one workgroup per problem, n <= 2048),
// >= 1 = group kernel with that many members (few problems, or n > 2048); -1 = n not supported
// (`force`: the context's hipdrt_debug_qp_group setting, -1 = automatic)
int qp_group_size(int B, int n, int force = -1);
size_t qp_gsync_ints();
// posterior variance on an evaluation grid (qp_resident.hpp: cov_kernel_resident); Bex = evaluation rows as packed tiles
int launch_dist_var(hipStream_t st, int B, int n, const double* Ppk, long long ppk_stride, const double* Bex, int nex,
                    double* L, long long l_stride, double* out, long long out_stride, int* status);
size_t dist_var_scratch_doubles(int n, int nex);
// logdet[b] = 2 sum log diag chol(M_b) of B packed matrices, status[b] = -1 and NaN where M_b is not positive definite
// (qp_resident.hpp: logdet_kernel_resident); L: dist_var_scratch_doubles(n, 0) doubles of scratch per matrix
int launch_logdet(hipStream_t st, int B, int n, const double* Ppk, long long ppk_stride, double* L, long long l_stride,
                  double* logdet, int* status);
void launch_rows_outer(hipStream_t st, const double* Y, int nch, int ncol, int nex, int nrow, double scale, double* out, int ld);
void launch_pack_rows(hipStream_t st, int nrow, int ncol, int col_offset, const double* M, int ldm, int ntile_rows,
                      double* tiles, int nchp);
// order[] = problem indices sorted by descending iteration count of the previous solve (inactive ones last)
void launch_lpt_order(hipStream_t st, int B, const int* iters, const int* active, int* order);
size_t qp_scratch_ld(int n);
size_t qp_scratch_doubles(int n, int G = 0);
inline int qp_state_ld(int n) { return round_up(n, 32) + 32; }
inline size_t qp_state_doubles(int n) { return (size_t)17 * qp_state_ld(n); }
int qp_profile_read(unsigned long long* out, int n, int reset);
int hyper_profile_read(unsigned long long* out, int n, int reset);   // slots 48.. of hipdrt_qp_profile (hyper.hip)
int qp_occupancy(int threads, int n);

}  // namespace hipdrt
