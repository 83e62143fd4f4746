/* hipdrt_debug.h -- diagnostic and test hooks of libhipdrt.so.
 *
 * NOT part of the drop-in boundary (include/hipdrt.h): nothing here replaces a reference interface, and the Python host
 * layer's product path never calls these.  They exist for tests/ (kernel-choice independence of the results) and tools/
 * (in-kernel phase counters of a PROFILE build, occupancy queries).  Every hook takes a context: there is no process-wide
 * switch.  The kernels of the fit loop each have a hook that runs their launcher as it is on host arrays: hipdrt_debug_gram_l2
 * (Gram, q), hipdrt_debug_hyper_step (the hyper-parameter step in its three product forms), hipdrt_debug_kk_stats,
 * hipdrt_debug_apply_rows, hipdrt_debug_find_peaks, hipdrt_debug_peak_trough_probs, hipdrt_debug_peak_resolve,
 * hipdrt_debug_response; so have the kernels that read
 * a finished fit: hipdrt_debug_pfrt_step / _combine, hipdrt_debug_candidate_llh, and hipdrt_debug_posterior (the posterior variance and
 * covariance chain: packed rows, the 32-column factorisation with appended tile rows, the outer product).  The interior-point QP has
 * hipdrt_debug_qp (launch_qp in the fit loop's form: packed P only, active mask, dispatch order, iters_accum; s and z come back) and
 * hipdrt_debug_lpt_order (the dispatch-order kernel alone).  The map kernels have hipdrt_debug_map_gaussian (the separable filter
 * passes in their LDS and uncached forms), hipdrt_debug_map_reduce (the fixed-order mean, std and min / max) and hipdrt_debug_map_prob
 * (the clamp and probability kernels of a map's rows, fed f and fxx directly); the rank filters are reached through their entry point.
 * The assembly kernels of hipdrt_plan_resolve_group have hipdrt_debug_resolve_assemble (members of their own sizes in, dense P_k out).
 * What runs before the loop and after it has hipdrt_debug_prep, hipdrt_debug_init_weights, hipdrt_debug_weight_method, hipdrt_debug_llh
 * and hipdrt_debug_rowop (the element-wise launchers), csrc/debug_setup.hip.
 */
#ifndef HIPDRT_DEBUG_H
#define HIPDRT_DEBUG_H

#include "hipdrt.h"

#ifdef __cplusplus
extern "C" {
#endif

/* diagnostic: in-kernel phase cycle counters of qp_kernel (workgroup 0 only), non-zero only in a build with
 * -DHIPDRT_QP_PROFILE (make PROFILE=1); slots documented in csrc/qp.hip.  Never used in timed runs.        */
int hipdrt_qp_profile(hipdrt_ctx* ctx, unsigned long long* cycles, int n, int reset);
/* diagnostic: workgroups per CU the runtime reports for the coneqp kernel of n unknowns (threads = 512)          */
int hipdrt_debug_qp_occupancy(hipdrt_ctx* ctx, int threads, int n);
/* diagnostic (tests): workgroups per problem of THIS CONTEXT's coneqp launches sized from now on (plans created on it,
 * hipdrt_qp_batch calls through it; other contexts are not affected) -- members >= 1 forces the group kernel
 * with (at most) that many members for every problem size, 0 forces the one-workgroup batch kernel (n <= 2048), -1 gives the
 * choice back to the library (few problems of n > 528, or n > 2048 -> group kernel).  The group kernel's results do not
 * depend on the group size (bit for bit); batch and group kernel differ by rounding (the batch kernel fuses the forward
 * substitution into the factorisation: another summation order), same iteration counts.                                */
int hipdrt_debug_qp_group(hipdrt_ctx* ctx, int members);
/* diagnostic (tests, tools): wavefronts per workgroup of THIS CONTEXT's batch coneqp launches at n <= 528 -- 4 = the fat form
 * (four wavefronts, one per SIMD, 512 registers each), 8 = eight wavefronts with 256 registers, -1 = the library's choice.
 * A context starts from the environment variable HIPDRT_QP_WAVES (4 | 8) when it is set.  Both kernels run the same arithmetic
 * in the same order: the results are the same bits (tests/test_gpu_qp.py).                                             */
int hipdrt_debug_qp_waves(hipdrt_ctx* ctx, int waves);
/* diagnostic (tests): on = 0 makes THIS CONTEXT's fits visit the exact zeros of the penalty matrices as well -- the Gram
 * epilogue adds the L2 part to every tile and the hyper kernel's Toeplitz convolutions run over all columns instead of the
 * penalties' reach (csrc/gram.hip, csrc/hyper.hip).  The results are the same bits either way; tests/test_gpu_fit.py checks it. */
int hipdrt_debug_exact_zero_shortcuts(hipdrt_ctx* ctx, int on);
/* diagnostic (tests): the library's own streams on the context's device (hipdrt.h: hipdrt_stream) -- how many there are
 * (return value through *size), and for the first min(*size, cap) of them the hipStream_t, the number of contexts holding it and
 * the number of device loops running on it right now.  Any of the three arrays may be NULL.                               */
int hipdrt_debug_stream_pool(hipdrt_ctx* ctx, int cap, void** streams, int* holders, int* running, int* size);

/* test hook (tests/test_gpu_gram.py): the fit loop's Gram and q launchers on host arrays, in every form the loop, the posterior
 * entry points and the stand-alone API run them -- P_b = (W_b A_b)'(W_b A_b) + L2_b and q_b = -(W_b A_b)'(W_b y_b) + l1 (csrc/gram.hip).
 * All arrays are host memory, row-major; a NULL pointer means "absent".                                                     */
typedef struct hipdrt_debug_gram_args {
    int B, m, n;
    const double* A;        /* [a_batched ? B : 1][m][lda], lda >= n                                                    */
    int a_batched, lda;
    const double* w;        /* [B][m]                                                                                   */
    const double* y;        /* [B][m] or NULL: no q                                                                     */
    const double* l1;       /* [n] or NULL: l1_scalar                                                                   */
    double l1_scalar;
    /* explicit L2 (used when s is NULL; may be NULL as well: no L2 term) ...                                           */
    const double* l2;       /* [l2_batched ? B : 1][n][ldl2], ldl2 >= n                                                 */
    int l2_batched, ldl2;
    /* ... or the hyper-parameter form, selected by s != NULL (fields as GramL2, csrc/common.hpp)                       */
    const double* mk[3];    /* each [n][ldm], ldm >= n                                                                  */
    int ldm;
    const double* s;        /* [B][3][n]                                                                                */
    const double* rho;      /* [B][3] or NULL: use_rho = 0 (dop_rho is then not used either)                            */
    double dfac[3];
    int ns, sym, toep, toep_maxd, spec_zero;
    int dop_start, dop_size;       /* dop_size > 0: the block lies inside [0, ns)                                       */
    const double* dop_rho;  /* [B][3], required when dop_size > 0 and rho is given                                      */
    double dop_dfac[3];
    const int* active;      /* [B] or NULL                                                                              */
    /* in/out: the host contents are uploaded first, so what comes back differs from them only where a kernel wrote     */
    double* P;              /* [B][n][ldp], ldp >= n, or NULL: the kernel form without the row-major copy               */
    int ldp;
    double* Ppk;            /* [B][nchp * nchp * 256] with nchp = round_up(n, 32) / 16, or NULL                         */
    double* q;              /* [B][n] (with y)                                                                          */
} hipdrt_debug_gram_args;
/* uploads, calls launch_gram_l2 and (with y) launch_qvec as they are, downloads.  Refuses every combination that could make a
 * kernel read or write out of bounds.                                                                                   */
int hipdrt_debug_gram_l2(hipdrt_ctx* ctx, const hipdrt_debug_gram_args* a);
/* test hook: launch_pack_p -- row-major symmetric P [B][n][ldp] (host) -> Ppk [B][nchp * nchp * 256] (host, in/out as above) */
int hipdrt_debug_pack_p(hipdrt_ctx* ctx, int B, int n, const double* P, int ldp, double* Ppk);
/* test hook (tests/test_gpu_lml.py): the log-determinant kernel of hipdrt_plan_lml_terms alone -- launch_pack_p, then launch_logdet in
 * that entry's chunks -- on B row-major symmetric matrices P [B][n][n] (host; the lower triangle is read).  logdet [B] = 2 sum ln L_ii
 * of the Cholesky factor, status [B] = 0; a matrix that is not positive definite gives NaN and -1.  1 <= B <= 4096, 1 <= n <= 4096. */
int hipdrt_debug_logdet(hipdrt_ctx* ctx, int B, int n, const double* P, double* logdet, int* status);

/* test hook (tests/test_gpu_hyper.py): one hyper-parameter step -- launch_hyper (csrc/hyper.hip) as it is: hyper_kernel, with the
 * products of estimate_weights inside it, from premv_kernel or from batch_products_kernel<0> / <1> -- on host arrays.  The hook
 * fills a FitState (csrc/common.hpp) from this struct.  Arrays are host memory, row-major.  The per-spectrum arrays are in/out:
 * their host contents are uploaded, so what comes back differs from them only where a kernel wrote.  On the device every one of
 * them has a border of marker bytes on either side; HIPDRT_E_NUMERIC when a border changed, or when any entry of a per-spectrum rm
 * other than the vz_offset column did.                                                                                        */
typedef struct hipdrt_debug_hyper_args {
    int B, m, n, ns, ldrm, ldm;    /* ns < n: there is a DRT block; ldrm, ldm >= n                                             */
    const double* rm;       /* [rm_batched ? B : 1][m][ldrm]                                                                */
    int rm_batched;
    const double* vmm;      /* [m][m]                                                                                       */
    const double* mk[3];    /* each [n][ldm]                                                                                */
    int toeplitz;           /* 1: the DRT blocks are symmetric Toeplitz (verified on the host, refused when they are not)      */
    int toep_reach;         /* -1, or a distance beyond which every DRT block is exactly zero (refused when it is too small)   */
    const double* x;        /* [B][n] the QP's result                                                                       */
    double* x_in;           /* [B][n]                                                                                       */
    double* s;              /* [B][3][n]                                                                                    */
    double *rho, *xmx;      /* [B][3]                                                                                       */
    double *rv, *est_w, *w; /* [B][m]                                                                                       */
    double *var_floor, *coef_scale;        /* [B]                                                                          */
    const int* qp_status;   /* [B]                                                                                          */
    int *active, *fit_status, *outer_iters;   /* [B]                                                                       */
    int* n_active;          /* [1]: incremented by every spectrum that goes on                                              */
    double* outlier_t;      /* [B][m] or NULL                                                                               */
    const hipdrt_fit_opts* opts;
    int it, continue_mode, min_iter;       /* continue_mode 0, 1 or 2 (FitState)                                           */
    double basis_area;
    const hipdrt_prepared_desc* desc;      /* or NULL: not a prepared plan.  Used: ns-independent fields dop_*, vz_index, vb_*,
                                              num_chrono, chrono_vmm_uniform                                                */
    double *dop_rho, *dop_xmx;             /* [B][3], required with desc                                                    */
    const double* vz_strength;             /* [m], required when desc->vz_index >= 0                                        */
    const double* vz_entry;                /* [B][m] or NULL                                                                */
    double* rm_col;         /* out [rm_batched ? B : 1][m]: column vz_index of rm after the step (desc->vz_index >= 0)        */
    int products;           /* 0: inside hyper_kernel, 1: premv_kernel, 2: batch_products_kernel (needs a shared rm, no vz
                               column and outlier_p <= 0, as the fit loop's own choice does)                                */
} hipdrt_debug_hyper_args;
/* Refuses every combination that could make a kernel read or write out of bounds, and a problem no LDS form holds (nothing is
 * launched then).                                                                                                           */
int hipdrt_debug_hyper_step(hipdrt_ctx* ctx, const hipdrt_debug_hyper_args* a);
/* test hook: the LDS form launch_hyper picks for a problem -- *form 1: Toeplitz columns beside the two m-vectors, 2: inside the
 * second m-vector, 0: the general row-streaming form -- and its dynamic LDS in bytes; HIPDRT_E_INVALID when none fits.        */
int hipdrt_debug_hyper_form(hipdrt_ctx* ctx, int n, int m, int ns, int toeplitz, int outlier, int* form, long long* lds_bytes);
/* test hook (tests/test_gpu_matrices_edges.py): the launch form of the general interp build of hipdrt_impedance_matrix for B
 * spectra of nf frequencies, ntau columns and lookups of ngrid knots -- threads per matrix row, rows per workgroup and dynamic LDS
 * in bytes; HIPDRT_E_INVALID for an ngrid the entry points refuse.  Nothing is launched.                                      */
int hipdrt_debug_impedance_interp_form(hipdrt_ctx* ctx, int B, int nf, int ntau, int ngrid, int* tpr, int* rpb,
                                       long long* lds_bytes);

/* test hook (tests/test_gpu_kk.py): the statistics stage of hipdrt_plan_kk_screen's kernel as it is, on host residuals --
 * freq [nf] strictly ascending or descending, err_re / err_im [B][nf]; out (any may be NULL): std [B], outlier_mask [B][nf],
 * f_lim [B][2], i_lim [B][2], status [B] as documented there.  Refuses sizes the kernel's LDS cannot hold.                  */
int hipdrt_debug_kk_stats(hipdrt_ctx* ctx, int B, int nf, const double* freq, const double* err_re, const double* err_im,
                          const hipdrt_kk_opts* opts, double* std, int* outlier_mask, double* f_lim, int* i_lim, int* status);

/* test hook (tests/test_gpu_predict.py): the row-application kernel of the prediction entry points (csrc/predict.hip) as it is,
 * on host arrays: out[b][i] = scale[b] * sum_j E[i][j] X[b][col_offset + j]; X [B][ldx] with ldx >= col_offset + K, E [r][K],
 * scale [B] or NULL (1), out [B][r].  The device output is allocated one row and five columns larger and filled with a marker:
 * HIPDRT_E_NUMERIC when the kernel changed anything outside its B x r block.                                                */
int hipdrt_debug_apply_rows(hipdrt_ctx* ctx, int B, int K, int ldx, int col_offset, const double* X, int r, const double* E,
                            const double* scale, double* out);

/* test hook (tests/test_gpu_peaks.py): peaks_kernel (csrc/peaks.hip) as it is, on host rows -- fxx [B][neval]; f [B][neval]
 * (needed by search = 0 and method 2, else may be NULL); var_fxx [B][neval] (methods 1, 2) and var_f [B][neval] (method 2): the
 * variances before extend_var's clamp and the floor, which the kernel applies.  eval_sign and normalize of the options are not
 * used.  Outputs as hipdrt_plan_find_peaks, any may be NULL.  Non-finite input rows are refused.  Every device output has a
 * border of marker bytes on either side: HIPDRT_E_NUMERIC when the kernel changed one.  HIPDRT_E_INVALID, and nothing is
 * launched, when the rows do not fit one workgroup's LDS.                                                                      */
int hipdrt_debug_find_peaks(hipdrt_ctx* ctx, int B, int neval, const double* fxx, const double* f, const double* var_fxx,
                            const double* var_f, const hipdrt_peak_opts* opts, int* peak_sign, int* keep, double* heights,
                            double* prominences, double* probs, int* left_bases, int* right_bases, int* count,
                            double* used_prominence, double* peak_prob, double* curv_prob);

/* test hook (tests/test_gpu_peak_prob.py): peak_trough_prob_kernel (csrc/peak_prob.hip) as it is, on host rows -- f, fx, fxx
 * [B][neval]; var_f, var_fx, var_fxx [B][neval] (bayes_cov = 1; NULL with bayes_cov = 0): the variances before extend_var's
 * clamp, the root and the floor, which the kernel applies.  prob_in [B][neval] non-NULL skips the probability stage and runs the
 * search on the caller's row: the other input rows are then not read, and pp, tp and sigma must be NULL.  Ranges and outputs as
 * hipdrt_plan_peak_trough_probs, any output may be NULL.  Non-finite input rows are refused.  Every device output has a border of
 * marker bytes on either side: HIPDRT_E_NUMERIC when the kernel changed one.  HIPDRT_E_INVALID, and nothing is launched, for what
 * the entry point refuses.                                                                                                     */
int hipdrt_debug_peak_trough_probs(hipdrt_ctx* ctx, int B, int neval, const double* f, const double* fx, const double* fxx,
                                   const double* var_f, const double* var_fx, const double* var_fxx, const double* prob_in,
                                   const hipdrt_peak_prob_opts* opts, int nranges, const int* range_lo, const int* range_hi,
                                   double* pp, double* tp, double* prob, double* sigma, int* keep, double* heights,
                                   double* prominences, int* left_bases, int* right_bases, int* count, int* range_peaks);

/* test hook (tests/test_gpu_peak_resolve.py): peak_resolve_kernel (csrc/peak_resolve.hip) as it is, on host arrays -- f, fxx
 * [B][nfind]; keep [B][nfind] (source 0) or indices [B][max_peaks] (source 1) or windows (source 2); x [B][copies * nb] the DRT
 * block in data units; ln_tau_find [nfind], ln_basis [nb], ln_tau_out [nout] (nout may be 0); E0 [nout][nb] is built by the
 * library (hipdrt_func_eval_matrix's kernel, order 0, basis_eps).  fit_status [B] may be NULL.  Outputs as
 * hipdrt_plan_resolve_peaks, any may be NULL.  Non-finite input rows are refused, as are indices and windows out of range or not
 * strictly increasing.  Every device output has a border of marker bytes on either side: HIPDRT_E_NUMERIC when the kernel changed
 * one.  HIPDRT_E_INVALID, and nothing is launched, when the shape does not fit one workgroup's LDS; lds_bytes (may be NULL) gets
 * the need in every case.                                                                                                        */
typedef struct {
    int B, nfind, nb, nout, copies, source, nwin;
    const double *f, *fxx;
    const int *keep, *indices, *win_start, *win_end;
    const double* x;
    const double *ln_tau_find, *ln_basis, *ln_tau_out;
    double basis_eps;
    const int* fit_status;
    const hipdrt_peak_resolve_opts* opts;
    hipdrt_peak_resolve_out out;
    long long* lds_bytes;
} hipdrt_debug_peak_resolve_args;
int hipdrt_debug_peak_resolve(hipdrt_ctx* ctx, const hipdrt_debug_peak_resolve_args* a);

/* test hooks (tests/test_gpu_pfrt.py): the two kernels of csrc/pfrt.hip as they are, on host arrays.
 * pfrt_step: peak_sign, heights, prominences (what peaks_kernel writes), f, var_f, var_fxx, all [B][neval]; the variances before
 * extend_var's clamp (ext_left, ext_right; -1 = off) and the floor, which the kernel applies; out [B][neval].
 * pfrt_combine: step_pfrt [S][B][neval_pfrt], rss and sum_log_w [S][B], factors [S], m the number of data rows behind the sums;
 * the options' prior, n_eff_factor, smooth, integrate and normalize fields are used; ln_tau_out may be NULL without smooth;
 * pfrt [B][neval_out], raw_pfrt [B][neval_pfrt], post_prob [S][B], any may be NULL.  Every device output has a border of marker
 * bytes on either side: HIPDRT_E_NUMERIC when a kernel changed one.  HIPDRT_E_INVALID, and nothing is launched, for a grid of more
 * than 2048 points.                                                                                                            */
int hipdrt_debug_pfrt_step(hipdrt_ctx* ctx, int B, int neval, const int* peak_sign, const double* heights, const double* prominences,
                           const double* f, const double* var_f, const double* var_fxx, double var_floor, int ext_left,
                           int ext_right, double* out);
int hipdrt_debug_pfrt_combine(hipdrt_ctx* ctx, int B, int S, int neval_pfrt, int neval_out, const double* step_pfrt,
                              const double* rss, const double* sum_log_w, const double* factors, int m,
                              const hipdrt_pfrt_opts* opts, const double* ln_tau_pfrt, const double* ln_tau_out, double* pfrt,
                              double* raw_pfrt, double* post_prob);
/* test hook (tests/test_gpu_pfrt_select.py): pfrt_select_kernel of csrc/pfrt.hip as it is, on host arrays: raw_pfrt [B][neval_pfrt],
 * step_pfrt [S][B][neval_pfrt], rss and sum_log_w [S][B], m the number of data rows behind the sums.  out: the compact form of
 * hipdrt_plan_pfrt_select (its raw_pfrt, step_pfrt, post_prob and pfrt are not written, sel's output grid is not read); status [B]: 0, HIPDRT_PFRT_NO_PEAK or
 * HIPDRT_PFRT_TOO_MANY_PEAKS.  Every device output has a border of marker bytes: HIPDRT_E_NUMERIC when the kernel wrote outside.   */
int hipdrt_debug_pfrt_select(hipdrt_ctx* ctx, int B, int S, int neval_pfrt, const double* raw_pfrt, const double* step_pfrt,
                             const double* rss, const double* sum_log_w, int m, const hipdrt_pfrt_select_opts* sel,
                             hipdrt_pfrt_select_out* out, int* status);

/* test hook (tests/test_gpu_response.py): the device chain of hipdrt_plan_predict_response behind its layer builders -- the DOP
 * blocks times their scale vectors, the row-application kernel on the S nt stacked rows of U (both copies of a two-copy block) and
 * of Ud, then response_assemble_kernel (csrc/predict.hip) -- on host arrays, no fit needed.  The assembly kernel is reached through
 * the products it reads (T = cs U x is formed by the hook, as the entry point forms it); it cannot be fed a T of the caller's.
 * X [B][n] scaled solutions, DRT block at column ns; U [S][nt][ntau] unit-step layers or NULL; Ud [S][nt][dop_size] unit phasor layers
 * or NULL; dop_scale_vector [B][dop_size] per member, or NULL (1); the other fields as hipdrt_predict_desc and hipdrt_response_args
 * name them (NULL leaves a term out).  out [B][nt] sits between two borders of marker bytes: HIPDRT_E_NUMERIC when the kernel
 * changed one.  Every index and block is checked against n before anything is launched.                                         */
typedef struct {
    int B, S, nt, ntau, copies, ns, n;
    const double *X, *U, *Ud;
    int dop_start, dop_size;
    const double* dop_scale_vector;
    const double* step_sizes; int sizes_batched;
    const double *coefficient_scale, *response_signal_scale, *scaled_response_offset;      /* [B]; the last two may be NULL */
    int idx_rinf, idx_cinv, vz_index, vb_start, vb_size;
    double capacitance_scale;
    const double* inf_rv; int inf_batched;
    const double* cap_rv; int cap_batched;
    const double *vz_strength, *vb_mat, *v_baseline_scale;
    const int* fit_status;      /* [B] or NULL */
    int include_mask;
    double* out;
} hipdrt_debug_response_args;
int hipdrt_debug_response(hipdrt_ctx* ctx, const hipdrt_debug_response_args* a);

/* test hooks (tests/test_gpu_candidates.py): the likelihood kernels of csrc/candidates.hip alone, on host arrays, no plan needed.
 * x [C][B][n]; rm [m][n] (rm_batched = 0) or [B][m][n]; rv [B][m]; vmm [m][m]; var_floor [B]; rss, sum_log_w [C][B] out, each
 * between two borders of marker bytes (HIPDRT_E_NUMERIC when a kernel changed one).  hipdrt_debug_candidate_form fixes how this
 * context's candidate scoring -- this hook and hipdrt_plan_score_candidates on its plans -- keeps rm x between its two products:
 * 0 in LDS (HIPDRT_E_INVALID at the call when 16 rows of m do not fit), 1 through the scratch buffer, -1 the library chooses.    */
int hipdrt_debug_candidate_llh(hipdrt_ctx* ctx, int C, int B, int m, int n, const double* rm, int rm_batched, const double* rv,
                               const double* vmm, const double* var_floor, const double* x, double* rss, double* sum_log_w);
int hipdrt_debug_candidate_form(hipdrt_ctx* ctx, int form);

/* test hook (tests/test_gpu_posterior.py): the posterior variance and covariance chain behind the plan entry points
 * (hipdrt_plan_distribution_var / _cov, _param_var / _cov, the credible bands; csrc/plan_post.hip) from the packed final P on, with a P
 * of the caller's: pack_rows_kernel, cov_kernel_resident over the spectra in chunks of 256, rows_outer_kernel.  The entry points and the
 * hook call the same two functions (posterior_var_dev, posterior_cov_dev).  Host arrays, row-major:
 *   P [p_batched ? B : 1][n][ldp], symmetric positive definite; only the lower triangle is read (launch_pack_p packs it);
 *   rows [neval][ncol]: row i sits at unknowns col_offset .. col_offset + ncol - 1 and is zero elsewhere; scale [B] or NULL (1);
 *   cov_member -1: the batched form over all B spectra.  cov_member = b: spectrum b alone in the single-spectrum form (every stride
 *   0, as the covariance entry points run it); var, status and tail then hold that one spectrum.
 * out, any may be NULL, nb = B or 1:  var [nb][neval] = scale_b * rows_i' P_b^-1 rows_i (NaN where status is -1);  status [nb] 0, or -1:
 * P_b is not positive definite;  cov [neval][neval] = scale_b * rows P_b^-1 rows' (cov_member >= 0; all NaN when status is -1, and the
 * call still returns HIPDRT_OK);  bex [nex][nchp][256] the packed rows, nex = ceil(neval / 16), nchp = round_up(n, 32) / 16;
 * tail [nb][nex][nchp][256] the tile rows nchp .. nchp + nex - 1 behind each factor, rows L^-T, which rows_outer_kernel reads
 * (B <= 256 in the batched form: later chunks reuse the scratch).
 * Every device output has a border of marker bytes on either side, and so has every spectrum's factor scratch (with the inverse
 * diagonal blocks behind it for n > 528): HIPDRT_E_NUMERIC when a kernel changed one.  HIPDRT_E_INVALID, and nothing is launched, for
 * n or B outside 1..4096, neval < 1, col_offset < 0, col_offset + ncol > n, ldp < n, cov_member out of range, or non-finite input.   */
typedef struct hipdrt_debug_posterior_args {
    int B, n;
    const double* P; int p_batched, ldp;
    const double* rows; int neval, ncol, col_offset;
    const double* scale;
    int cov_member;
    double* var; int* status; double* cov; double* bex; double* tail;
} hipdrt_debug_posterior_args;
int hipdrt_debug_posterior(hipdrt_ctx* ctx, const hipdrt_debug_posterior_args* a);
/* test hook (tests/test_gpu_dop_posterior.py): the same chain with the per-member congruence scaling of the packed P in front of it,
 * as hipdrt_plan_dop_posterior / hipdrt_plan_dop_cov run it (scale_p_kernel between the packing of P and posterior_var_dev):
 * entry (i, j) of every lower tile of member b is multiplied by s_i, then by s_j, with s = 1.0 / dop_scale_vector_b on the unknowns
 * dop_start .. dop_start + dop_size - 1 and 1 elsewhere, so that var = rows_i' (S P S)^-1 rows_i.
 *   post: hipdrt_debug_posterior's arguments, read as there (every member has its own image of P, a shared P is packed B times);
 *   dop_scale_vector [dop_size], or [B][dop_size] when dop_scale_batched != 0.
 * One more optional output: ppk [nb][nchp][nchp][256], the packed image after the scaling (tiles the kernels do not write are zero),
 * of all B members or, with cov_member >= 0, of that member.  Borders and HIPDRT_E_NUMERIC as hipdrt_debug_posterior.
 * HIPDRT_E_INVALID, and nothing is launched, for its refusals, dop_size < 1, a block outside [0, n), or a dop_scale_vector entry
 * that is not finite and positive.                                                                                                */
typedef struct hipdrt_debug_dop_posterior_args {
    hipdrt_debug_posterior_args post;
    int dop_start, dop_size;
    const double* dop_scale_vector; int dop_scale_batched;
    double* ppk;
} hipdrt_debug_dop_posterior_args;
int hipdrt_debug_dop_posterior(hipdrt_ctx* ctx, const hipdrt_debug_dop_posterior_args* a);

/* test hook (tests/test_gpu_qp_loop.py): launch_qp (csrc/qp.hip) as it is, on host arrays, with its arguments filled the way the fit
 * loop fills them (loop_qp_args, csrc/plan_fit.hip) -- a form hipdrt_qp_batch cannot produce: P reaches the kernel as packed tiles only
 * (launch_pack_p; one shared copy with stride 0 when p_batched = 0), with an active mask, a dispatch-order table and iters_accum.
 * The kernel is chosen from this context's switches (hipdrt_debug_qp_group, hipdrt_debug_qp_waves) as every launch of the context is.
 *   P [p_batched ? B : 1][n][ldp] (lower triangle read), q [B][n], h [h_batched ? B : 1][n]; opts NULL = the defaults;
 *   active [B] or NULL; order [B] or NULL: workgroup i solves problem order[i], must be a permutation of 0 .. B - 1;
 *   use_lpt != 0 (excludes order, needs iters): the hook runs lpt_order_kernel on the uploaded iters and active, as the fit loop does
 *   in front of every coneqp launch, and hands its table to the kernel;
 *   form [3] out or NULL: {workgroups per problem G (0 = the batch kernel), inverse diagonal blocks in global memory 0 / 1, wavefronts
 *   per workgroup}: what the launch was sized for.
 * In/out, host contents uploaded first, so an entry no kernel wrote comes back as it went in: x [B][n], status [B]; iters [B], pcost [B],
 * iters_accum [B] (each may be NULL).  Out, any may be NULL: s, z [B][n], state vectors 2 and 1 of the leader's copy of the iterates
 * (slot b * max(G, 1); rows of inactive problems are left alone); order_out [B] the table the kernel used (the identity without one).
 * On the device every in/out array, the order table, every problem's state block (17 vectors x state_ld, one per member), every
 * problem's factor scratch (qp_scratch_doubles) and the group kernel's sync words sit between borders of marker bytes:
 * HIPDRT_E_NUMERIC when a border changed, or when the leader's state does not hold the x that came back.  HIPDRT_E_INVALID, and
 * nothing is launched, for n or B outside 1..4096, ldp < n, non-finite input, an order that is no permutation, or n > 2048 with the
 * batch kernel forced.                                                                                                             */
typedef struct hipdrt_debug_qp_args {
    int B, n;
    const double* P; int p_batched, ldp;
    const double* q;
    const double* h; int h_batched;
    const hipdrt_qp_opts* opts;
    const int* active;
    const int* order;
    int use_lpt;
    int* form;
    double* x; int* iters; double* pcost; int* status; int* iters_accum;
    double* s; double* z; int* order_out;
} hipdrt_debug_qp_args;
int hipdrt_debug_qp(hipdrt_ctx* ctx, const hipdrt_debug_qp_args* a);
/* test hook: lpt_order_kernel alone -- order [B] (in/out, between borders of marker bytes) = the problems by descending iters, inactive
 * ones (active [B], may be NULL) last, ties in index order.  HIPDRT_E_INVALID when B * sizeof(int) exceeds 48 KiB, the fit loop's own
 * condition for using the table.                                                                                                 */
int hipdrt_debug_lpt_order(hipdrt_ctx* ctx, int B, const int* iters, const int* active, int* order);

/* tools hook (tools/bench_predict.py, tools/bench_peaks.py, tools/bench_response.py, tools/bench_candidates.py): kernel time in ms
 * of the last hipdrt_plan_llh_terms / _obs_llh_terms(_w) (ms[0] = ms[1]: its one launch), hipdrt_plan_score_candidates (ms[1]: all
 * launches),
 * hipdrt_plan_predict_drt / hipdrt_plan_predict_z / hipdrt_plan_find_peaks (ms[0]: the mean rows, ms[1]: all launches, peaks_kernel
 * included), hipdrt_plan_predict_response / _z_model / _dop (ms[0] = ms[1]: all launches; _z_model with the upload of its grids and
 * tables) or hipdrt_plan_dop_posterior (ms[0]: the mean rows, ms[1]: with the Gram/L2 rebuild, the scaling, the factorisations and the
 * band) of a plan of this context, by HIP
 * events around its launches (allocations and copies excluded): ms[0] up to the mean (predict_z: the whole prediction), ms[1] with
 * the credible band's factorisation included (equal to ms[0] without a band).                                                    */
int hipdrt_debug_last_predict_ms(hipdrt_ctx* ctx, float* ms);

/* Tools (tools/probe_map_filter.py): what the last hipdrt_map_filter of this context did between its upload and its download --
 * stats[0] kernel launches, stats[1] full-array reads plus writes those kernels make (in arrays of rows * cols doubles, counted
 * by the driver as it launches), stats[2] device time in ms by HIP events around them (the scalar read-backs and the node-table
 * callbacks of the adaptive path included).                                                                                    */
int hipdrt_debug_map_filter_stats(hipdrt_ctx* ctx, double* stats);

/* Tools (tools/probe_map_badness.py): device time in ms, by HIP events between the upload and the download, of this context's
 * last hipdrt_map_badness (its internal synchronisations included).                                                             */
int hipdrt_debug_map_badness_ms(hipdrt_ctx* ctx, double* ms);

/* test hooks (tests/test_gpu_map_kernels.py): the launchers of the map kernels alone, on host arrays.  On the device every in and out
 * array sits between two borders of marker bytes: HIPDRT_E_NUMERIC when a kernel changed one.  HIPDRT_E_INVALID, and nothing is
 * launched, for arguments that could make a kernel read or write out of bounds.
 *
 * map_gaussian: plain_gaussian_device (masked = 0: scipy's gaussian_filter, a NaN spreads over its window) or masked_gaussian_device
 * (masked = 1: masked_filter(nan_to_num(a), ~isnan(a), gaussian_filter)) of csrc/map_filter.hip, the two functions csrc/map_rank.hip
 * and csrc/map_predict.hip call and the same filter_pass_kernel launches as hipdrt_map_filter's -- a [R][C] row-major, tabs[2] the
 * half tables of axis 0 and 1 (radius < 0 skips the axis), out [R][C].
 *
 * map_reduce: the fixed-order reductions of csrc/map_filter.hip (MapFilter::reduce, std_of: reduce_partial + reduce_final) on x [n],
 * 1 <= n < 2^30 -- mode 0: out[0] = mean, out[1] = 0;  mode 1: out[0] = np.std(x), out[1] = the mean it was taken about;
 * mode 2: out[0], out[1] = min, max.  The partial sums and the scalar slots are bordered as well.
 *
 * map_prob: stage 3 of hipdrt_map_predict (csrc/map_predict.hip) through the entry point's own launchers -- with clamp_first
 * clamp_kernel in place on the variance rows, then (pk or curv given) map_prob_kernel without ext; without clamp_first map_prob_kernel
 * alone, with the clamp inside it when ext is given; the dynamic-LDS limit is raised as the entry point raises it.  f, fxx, vf, vxx
 * [rows][n] (f and fxx may be NULL when neither pk nor curv is asked for; non-finite values are allowed); ext [rows][2] or NULL: pairs
 * of indices of the grid, or (-1, -1); search 1, -1 or 0; sign_now as MapProbArgs.  Out, any may be NULL: pk, curv [rows][n];
 * vf_out, vxx_out [rows][n] the variance rows as the probabilities saw them.  HIPDRT_E_UNSUPPORTED with the entry point's message
 * when n exceeds what LDS holds; HIPDRT_E_INVALID for an ext pair outside the grid, and when there is nothing to launch.          */
int hipdrt_debug_map_gaussian(hipdrt_ctx* ctx, const double* a, int R, int C, const hipdrt_filter_table* tabs, int masked,
                              double* out);
int hipdrt_debug_map_reduce(hipdrt_ctx* ctx, const double* x, long long n, int mode, double* out);
int hipdrt_debug_map_prob(hipdrt_ctx* ctx, int rows, int n, const double* f, const double* fxx, const double* vf, const double* vxx,
                          const int* ext, int clamp_first, int search, double height, double prominence, int sign_now, double* pk,
                          double* curv, double* vf_out, double* vxx_out);

/* test hook (tests/test_gpu_store_resolve.py): the assembly kernels of hipdrt_plan_resolve_group (csrc/resolve.hip) alone, on host
 * arrays -- args as there (h is not read), B members of their own sizes n_b = num_remove + so + right_b - left_b:
 *   P: member b's row-major n_b x n_b matrix, member after member; q: its n_b entries, member after member.
 * Out: P_out, batch k's dense (nr nc_k) square matrix, batch after batch, unpacked from the lower tiles the kernel wrote (the upper
 * triangle is the mirror image, as the QP reads it); q_out, batch k's nr nc_k entries, batch after batch.  The packed image, q and
 * every input sit between borders of marker bytes: HIPDRT_E_NUMERIC when a kernel changed one, when a padding entry of a tile is not
 * zero, or when a diagonal tile is not symmetric.  HIPDRT_E_INVALID / HIPDRT_E_UNSUPPORTED, and nothing is launched, as the entry point. */
int hipdrt_debug_resolve_assemble(hipdrt_ctx* ctx, const hipdrt_resolve_args* args, int B, const double* P, const double* q,
                                  double* P_out, double* q_out);

/* test hooks (tests/test_gpu_setup.py, csrc/debug_setup.hip): what runs before the fit loop and after it -- launch_prep,
 * launch_row_mask + launch_init_weights, launch_weight_method and launch_llh (csrc/hyper.hip) as they are, on host arrays, with a
 * FitState filled as hipdrt_plan::state() fills it (hist_b = -1).  One structure serves the four hooks; each names below what it
 * needs, and refuses a NULL among those.  Arrays are host memory, row-major.  Every per-spectrum array that is given is in/out: its host
 * contents are uploaded between two borders of marker bytes, the launcher runs, and it is overwritten with what the device holds
 * afterwards, so it differs from what went in only where a kernel wrote.  HIPDRT_E_NUMERIC when a border changed.  Non-finite
 * entries of z, rm, vmm, vmm_iw, x, rv, est_w and var_floor are refused where the hook's kernels read them.
 * Limits: 1 <= B <= 4096, 1 <= m <= 8192, 1 <= n <= 4096, ldrm >= n, 0 <= num_chrono <= m.                                        */
typedef struct hipdrt_debug_setup_args {
    int B, nf, m, n, ldrm;
    const hipdrt_fit_opts* opts;
    const hipdrt_prepared_desc* desc;      /* or NULL: a plain plan.  Used: num_chrono, chrono_vmm_uniform, dop_rho_0             */
    const double *z_re, *z_im;             /* [B][nf]: prep of a plain plan (m = 2 nf)                                            */
    const double* rm;                      /* [rm_batched ? B : 1][m][ldrm]                                                       */
    int rm_batched;
    const double *vmm, *vmm_iw;            /* [m][m] each: two uploads, so a read of the wrong one shows                          */
    const int* qp_status;                  /* [B]                                                                                 */
    double *rv, *w, *est_w;                /* [B][m]                                                                              */
    double *x, *x_in;                      /* [B][n]                                                                              */
    double* s;                             /* [B][3][n]                                                                           */
    double *rho, *xmx, *dop_rho, *dop_xmx; /* [B][3]                                                                              */
    double *coef_scale, *var_floor;        /* [B]                                                                                 */
    int *active, *outer_iters, *fit_status, *qp_iters_total;      /* [B]                                                          */
    double* outlier_t;                     /* [B][m] or NULL                                                                      */
    int stage, r0, r1, row_mask;           /* init_weights: stage 0..3; 0 <= r0 < r1 <= m (stage 2, row_mask)                     */
    double fixed_chrono, fixed_eis;        /* weight rule: > 0 overrides                                                          */
    double *wrow, *wfac;                   /* weight rule out: [B][m], [B][2]                                                     */
    int stored;                            /* llh: weight mode 0..3                                                               */
    double scalar_w;
    double *rss, *slw;                     /* llh out: [B] each                                                                   */
    double* w_out;                         /* llh out: [B][m] or NULL                                                             */
} hipdrt_debug_setup_args;
/* launch_prep.  Plain (desc NULL): z_re, z_im, nf >= 1, m == 2 nf.  Prepared: rv (read), dop_rho, dop_xmx.  Both: rv, w, s, x, x_in,
 * rho, xmx, coef_scale, var_floor, active, outer_iters, fit_status, qp_iters_total.                                              */
int hipdrt_debug_prep(hipdrt_ctx* ctx, const hipdrt_debug_setup_args* a);
/* row_mask != 0: launch_row_mask(r0, r1) on w first; then launch_init_weights(stage, r0, r1).  Needs rm, vmm, vmm_iw, qp_status, x,
 * rv, w, est_w, var_floor, active, fit_status.  HIPDRT_E_INVALID, and nothing launched, when (n, m) do not fit one workgroup's LDS. */
int hipdrt_debug_init_weights(hipdrt_ctx* ctx, const hipdrt_debug_setup_args* a);
/* launch_weight_method: needs desc with 0 < num_chrono < m (the condition under which the fit launches it), est_w, wrow, wfac.    */
int hipdrt_debug_weight_method(hipdrt_ctx* ctx, const hipdrt_debug_setup_args* a);
/* launch_llh(stored, scalar_w, w_out): needs rm, vmm, x, rv, est_w, var_floor, rss, slw.  HIPDRT_E_INVALID, and nothing launched,
 * when n + 3 m doubles do not fit one workgroup's LDS.                                                                            */
int hipdrt_debug_llh(hipdrt_ctx* ctx, const hipdrt_debug_setup_args* a);

/* test hook: the element-wise launchers of csrc/hyper.hip, one per call, chosen by `op`.  in0..in2 are read, out0..out2 are in/out
 * between marker borders as above.  Non-finite inputs are refused.
 *   0 launch_vmm_exclude_self   in0 vmm [m][m] -> out0 [m][m]
 *   1 launch_assemble_rm        in0 a_re, in1 a_im [nf][n - ns], in2 freq [nf]; idx_rinf, idx_induc in [-1, ns); factor = the
 *                               inductance scale -> out0 rm [2 nf][ld], ld >= n (m is not read: the rows are 2 nf)
 *   2 launch_special_penalty    out0..out2 the three [n][ld] matrices; idx_rinf, idx_induc in [-1, n); pen_r, pen_l
 *   3 launch_make_h             n, ns, nonneg -> out0 [n]
 *   4 launch_scale_rows         in0 w [B][m], or NULL: in place on out0; in1 rows [batched ? B : 1][m] or NULL; active [B] or NULL;
 *                               factor -> out0 [B][m]
 *   5 launch_scale_weights      out0 w [B][m] in place; active [B]; factor
 *   6 launch_copy_column        in0 rm [batched ? B : 1][m][ld], 0 <= col < ld -> out0 [B][m]                                      */
typedef struct hipdrt_debug_rowop_args {
    int op, B, m, n, ns, nf, ld, col, idx_rinf, idx_induc, nonneg, batched;
    double factor, pen_r, pen_l;
    const double *in0, *in1, *in2;
    const int* active;
    double *out0, *out1, *out2;
} hipdrt_debug_rowop_args;
int hipdrt_debug_rowop(hipdrt_ctx* ctx, const hipdrt_debug_rowop_args* a);

#ifdef __cplusplus
}
#endif

#endif /* HIPDRT_DEBUG_H */
