/* hipdrt.h -- C-ABI of libhipdrt.so, the MI355X (gfx950) implementation of hybrid-drt's hot path.
 *
 * The reference (jdhuang-csm/hybrid-drt) is pure Python; it has no FFI of its own.  The entry points below
 * are what a ctypes binding for the hot path replaces, each citing the reference interface it stands for
 * (paths relative to the reference root).  Conventions:
 *   - plain C: opaque handles, pointers and sizes only; no C++/torch types;
 *   - every array is row-major contiguous float64 (int32 for counters/status) unless stated otherwise;
 *   - "host" pointers are caller-owned host memory, the library does the H2D/D2H copies;
 *     "_dev" entry points take device pointers and neither copy nor synchronise more than documented;
 *   - every function returns 0 on success, <0 on error (HIPDRT_E_*); hipdrt_last_error() gives the text;
 *     nothing throws, nothing falls back to the CPU: without a gfx950 device hipdrt_create fails;
 *   - one hipdrt_ctx per (process, device); a ctx is not re-entrant, distinct ctxs are independent.
 */
#ifndef HIPDRT_H
#define HIPDRT_H

#ifdef __cplusplus
extern "C" {
#endif

#define HIPDRT_OK 0
#define HIPDRT_E_INVALID (-1)   /* bad argument                                         */
#define HIPDRT_E_HIP (-2)       /* HIP runtime error (text in hipdrt_last_error)         */
#define HIPDRT_E_NODEVICE (-3)  /* no usable gfx950 device                              */
#define HIPDRT_E_NUMERIC (-4)   /* numerical breakdown for the whole call               */
#define HIPDRT_E_UNSUPPORTED (-5) /* the call is not built for this kind of plan         */

/* per-problem status codes written to status[] arrays */
#define HIPDRT_QP_OPTIMAL 0     /* coneqp stopping test met                                        */
#define HIPDRT_QP_MAXITER 1     /* maxiters reached (cvxopt status 'unknown')                      */
#define HIPDRT_QP_SINGULAR_LATE 2 /* Cholesky breakdown after iteration 0: cvxopt returns current x */
#define HIPDRT_QP_SINGULAR (-1) /* breakdown at the start point: cvxopt raises ValueError          */
#define HIPDRT_QP_ABORTED (-2)  /* internal to the several-workgroups-per-problem kernel: the workgroups of this problem were
                                   not placed on one XCD; the launcher repeats such a problem on one workgroup before it
                                   returns, so a caller sees this only if that repeat could not run     */

#define HIPDRT_MODE_INTERP 0    /* integrate_method='interp' (drtbase.py:155)  */
#define HIPDRT_MODE_TRAPZ 1     /* integrate_method='trapz'  (drtbase.py:159)  */

typedef struct hipdrt_ctx hipdrt_ctx;
typedef struct hipdrt_plan hipdrt_plan;
typedef struct hipdrt_comm hipdrt_comm;

/* ---- context -------------------------------------------------------------------------------------- */
int hipdrt_create(int device, hipdrt_ctx** out);
int hipdrt_destroy(hipdrt_ctx* ctx);   /* with plans still alive on it the context is freed by the last hipdrt_plan_destroy */
const char* hipdrt_last_error(void);
/* HIP stream the ctx launches on (so callers can record events / order other work): returns hipStream_t.
 * The stream is one of the library's own (created once per device, one per hardware queue beside the null stream's:
 * GPU_MAX_HW_QUEUES - 1, i.e. 3 by default and 7 under the host layer's default of 8; HIPDRT_STREAM_POOL=<n> overrides) and is
 * held by the context for its lifetime; contexts beyond that count share streams (their work is then ordered with each other's,
 * never wrong).  The ranges of a sub-batched hipdrt_plan_fit borrow the least busy of these streams for the duration of the call. */
void* hipdrt_stream(hipdrt_ctx* ctx);
int hipdrt_synchronize(hipdrt_ctx* ctx);
/* name of the device architecture, e.g. "gfx950" */
int hipdrt_device_info(hipdrt_ctx* ctx, char* arch, int arch_len, int* num_cu, long long* hbm_bytes);

/* ---- L1 kernel matrices --------------------------------------------------------------------------- */

/* basis.generate_impedance_lookup (hybdrt/matrices/basis.py:648-669), Gaussian basis.
 * in : wt_re[ngrid], wt_im[ngrid]  the omega*tau abscissae (np.logspace(-2.7,2.7,ngrid) / (-5.4,5.4))
 * out: z_re[ngrid], z_im[ngrid]    ny-point trapezoid integrals over y = linspace(-20,20,ny)          */
int hipdrt_impedance_lookup(hipdrt_ctx* ctx, double epsilon, int ngrid, int ny,
                            const double* wt_re, const double* wt_im, double* z_re, double* z_im);

/* mat1d.construct_impedance_matrix (hybdrt/matrices/mat1d.py:212-374), both parts in one call,
 * batched over B frequency grids.
 * freq[B or 1][nf] (freq_batched selects), tau[ntau]; mode INTERP uses the lookups (log_wt_*, z_* of
 * length ngrid, np.interp semantics incl. end clamping); mode TRAPZ integrates ny points.
 * toeplitz != 0 reproduces the reference's Toeplitz shortcut (mat1d.py:353-360): first column/row are
 * evaluated and scattered (the caller decides with the reference's rule, it requires B-independent grids).
 * out: a_re[B][nf][ntau], a_im[B][nf][ntau]                                                          */
int hipdrt_impedance_matrix(hipdrt_ctx* ctx, int B, int freq_batched, const double* freq, int nf,
                            const double* tau, int ntau, int mode, int toeplitz, double epsilon,
                            int ngrid, const double* log_wt_re, const double* z_re,
                            const double* log_wt_im, const double* z_im, int ny,
                            double* a_re, double* a_im);
/* same, outputs stay on the device (a_re_dev/a_im_dev are device pointers); used by bench.py to time the
 * build with HIP events without the D2H copy.  elapsed_ms (may be NULL) = kernel time over `repeat` launches */
int hipdrt_impedance_matrix_dev(hipdrt_ctx* ctx, int B, int freq_batched, const double* freq, int nf,
                                const double* tau, int ntau, int mode, int toeplitz, double epsilon,
                                int ngrid, const double* log_wt_re, const double* z_re,
                                const double* log_wt_im, const double* z_im, int ny,
                                void* a_re_dev, void* a_im_dev, int repeat, float* elapsed_ms);

/* phasance.construct_phasor_z_matrix (hybdrt/matrices/phasance.py:108-118), nu_basis_type='gaussian', normalize=False:
 * the distribution-of-phasances impedance columns.  out: zm_re, zm_im [nf][n_nu] (real and imaginary part).           */
int hipdrt_phasor_z_matrix(hipdrt_ctx* ctx, const double* freq, int nf, const double* basis_nu, int n_nu,
                           double nu_epsilon, double* zm_re, double* zm_im);
/* phasance.construct_phasor_v_matrix (phasance.py:121-144), gaussian nu basis, galvanostatic ideal steps.
 * out: rm[nt][n_nu] = sum over steps; layered[nsteps][nt][n_nu] (may be NULL)                                        */
int hipdrt_phasor_v_matrix(hipdrt_ctx* ctx, const double* times, int nt, const double* basis_nu, int n_nu,
                           double nu_epsilon, const double* step_times, const double* step_sizes, int nsteps,
                           double* rm, double* layered);

/* mat1d.construct_chrono_var_matrix (hybdrt/matrices/mat1d.py:457-490).  tt[nt] = the samples' transformed times
 * (utils/chrono.py:5-44 fwd_transform), seg[nseg+1] = sample-index bounds of the step segments
 * ([0, step indices..., nt], preprocessing.py:161-178); uniform != 0 -> error_structure='uniform' (ones / nt).
 * out: vmm[nt][nt], Gaussian in transformed time inside a segment, zero across segments, rows normalised.   */
int hipdrt_chrono_var_matrix(hipdrt_ctx* ctx, const double* tt, int nt, const int* seg, int nseg,
                             double vmm_epsilon, int uniform, double* vmm);

/* basis.generate_response_lookup (hybdrt/matrices/basis.py:672-689; integrand basis.py:616-618), Gaussian basis,
 * galvanostatic ideal step.
 * in : td[ngrid]   the (t - t_step)/tau abscissae (np.logspace(-6, 2, ngrid))
 * out: v[ngrid]    ny-point trapezoid integrals over y = linspace(-20,20,ny)                            */
int hipdrt_response_lookup(hipdrt_ctx* ctx, double epsilon, int ngrid, int ny, const double* td, double* v);

/* mat1d.construct_response_matrix (hybdrt/matrices/mat1d.py:16-122) for basis_type='gaussian', op_mode='galv',
 * step_model='ideal'.  times[nt], tau[ntau], step_times/step_sizes[nsteps]; mode INTERP uses the lookup
 * (log_td, v of length ngrid, np.interp semantics incl. end clamping), mode TRAPZ integrates ny points.
 * out: a[nt][ntau] = sum over steps; layered[nsteps][nt][ntau] per step (may be NULL)                   */
int hipdrt_response_matrix(hipdrt_ctx* ctx, const double* times, int nt, const double* tau, int ntau,
                           const double* step_times, const double* step_sizes, int nsteps, int mode,
                           double epsilon, int ngrid, const double* log_td, const double* v, int ny,
                           double* a, double* layered);

/* The non-default forms of mat1d.construct_response_matrix (hybdrt/matrices/mat1d.py:96-118), Gaussian basis:
 *   HIPDRT_RESPONSE_POT       op_mode='pot' (mat1d.py:114-118): exp(-(t - t_k) / tau) * unit_step(t, t_k) * size_k, rows before a
 *                             step 0 (tau_rise, epsilon, ny unused)
 *   HIPDRT_RESPONSE_EXPDECAY  op_mode='galv', step_model='expdecay', integrate_method='trapz' (integrand basis.py:619-637):
 *                             tau_rise[nsteps] = rise time of every step, ny-point trapezoid over y = linspace(-20, 20, ny)
 * same outputs as hipdrt_response_matrix                                                                    */
#define HIPDRT_RESPONSE_POT 0
#define HIPDRT_RESPONSE_EXPDECAY 1
int hipdrt_response_matrix_variant(hipdrt_ctx* ctx, const double* times, int nt, const double* tau, int ntau,
                                   const double* step_times, const double* step_sizes, const double* tau_rise, int nsteps,
                                   int variant, double epsilon, int ny, double* a, double* layered);

/* filters.nonuniform_gaussian_filter1d (hybdrt/filters/_filters.py:261-343; order 0, mode 'reflect', empty=False) applied
 * segment by segment: the anti-aliasing filter of the chrono down-sampling (preprocessing.filter_chrono_signal, 507-572,
 * called by downsample_data, 423-432).  y[n], sigma[n] (per-sample filter widths in samples, already capped);
 * seg[nseg+1] sample-index bounds of the step segments; per segment s its log-spaced sigma nodes nodes[s*K .. s*K+K)
 * (0 = unused slot), node_delta[nseg] = log spacing of the nodes, radius[s*K+k] = int(4 sigma + 0.5) or -1 for a node
 * below min_sigma (output = input), weights[woff[s*K+k] + j], j = 0..radius, the normalised Gaussian kernel halves
 * (scipy.ndimage._filters._gaussian_kernel1d); filtered[s] = 0 skips a segment (all widths zero).  out[n].
 * The caller (hipdrt.filters / hipdrt.preprocessing) derives nodes and kernels exactly as the reference does. */
int hipdrt_nonuniform_gaussian_filter1d(hipdrt_ctx* ctx, const double* y, int n, const double* sigma, const int* seg,
                                        int nseg, const int* filtered, const double* nodes, int K,
                                        const double* node_delta, const double* weights, long long nweights,
                                        const int* woff, const int* radius, double* out);

/* mapping.ndx.filter_ndx without groups (hybdrt/mapping/ndx.py:261-349, _filter_ndx_sub 302-349) on one (rows, cols) array --
 * the smoothing of a fitted map across psi and tau (DRTMD.filter_observations, hybdrt/mapping/drtmd.py:561-635): the
 * outlier-robust iterative Gaussian filter (hybdrt/filters/_filters.py: masked_filter 149-175, iterate_gaussian_weights
 * 183-232, iterative_gaussian_filter 235-256; rms_filter 8-26), optionally with curvature-adaptive widths
 * (nonuniform_gaussian_filter1d 261-345, get_adaptive_sigma1d 363-413, adaptive_gaussian_filter 451-475), on the 'reflect'
 * boundary of scipy.ndimage.  `a` is uploaded once and `out` downloaded once; in between only the scalars the host needs come
 * back (std of the curvature, min / max of a sigma field).
 *
 * Every table is built by the caller as scipy / _scifilters.py build it and is given as its centre and right half (all are
 * symmetric): w[0 .. radius].  radius < 0 skips the axis (sigma <= 1e-15, as gaussian_filter does).  Axis 0 runs along the rows
 * (stride cols), axis 1 along a row; ndim == 1 takes cols == 1 and axis 0 only. */
typedef struct {
    const double* w;
    int radius;
} hipdrt_filter_table;

#define HIPDRT_MAP_FILTER_MAX_NODES 16
/* the sigma nodes of one nonuniform_gaussian_filter1d call (_filters.py:264-295): node[k] ascending, node_delta their log
 * spacing, floor the value smaller sigmas are raised to (0: none); w[k][0 .. radius[k]] the node's table (Gaussian, or empty
 * Gaussian at max(node, min_sigma)), radius[k] < 0: the node returns its input (empty=False below min_sigma) */
typedef struct {
    int count;
    double node[HIPDRT_MAP_FILTER_MAX_NODES];
    double node_delta, floor;
    int radius[HIPDRT_MAP_FILTER_MAX_NODES];
    const double* w[HIPDRT_MAP_FILTER_MAX_NODES];
} hipdrt_node_tables;
/* called by hipdrt_map_filter, on the calling thread, once the extremes of a sigma field (after the floor at 1e-8) are known;
 * the tables must stay valid until hipdrt_map_filter returns.  Non-zero return: hipdrt_map_filter fails with HIPDRT_E_INVALID. */
typedef int (*hipdrt_node_table_fn)(void* user, int axis, int empty, double sigma_min, double sigma_max, hipdrt_node_tables* out);

#define HIPDRT_MAP_FILTER 0   /* the filtered array */
#define HIPDRT_MAP_SIGMAS 1   /* get_adaptive_sigmas(a, empty=, weights=init_weights) only: sigmas_out, nothing else */
typedef struct {
    int ndim, rows, cols;
    int op;                       /* HIPDRT_MAP_FILTER / HIPDRT_MAP_SIGMAS */
    int iterative, adaptive;      /* _filter_ndx_sub's switches */
    int mask_nans;                /* 1: NaN entries are zero-filled and carry weight 0; 0: `a` is filtered as it stands */
    int empty;                    /* HIPDRT_MAP_SIGMAS: get_adaptive_sigmas' empty=; with sigmas_in: adaptive_gaussian_filter's */
    int iter;                     /* iterate_gaussian_weights: passes (2) */
    double nstd;                  /* ... and nstd (5) */
    int box_size;                 /* dev_rms_size (5; odd) */
    const double* init_weights;   /* optional [rows * cols]: the mask of a non-iterative masked filter (masked_filter's mask) */
    const double* sigmas_in;      /* optional [ndim][rows * cols], adaptive = 1, iterative = 0: adaptive_gaussian_filter(a,
                                   * sigmas=, empty=) with these fields instead of get_adaptive_sigmas' */
    hipdrt_filter_table gauss[2], empty_gauss[2];   /* adaptive = 0: order-0 Gaussian and empty Gaussian of sigma[axis] */
    hipdrt_filter_table box[2];                     /* iterative: ones, radius box_size / 2, per axis */
    hipdrt_filter_table pre_gauss[2], pre_empty[2]; /* adaptive = 1: the same pair for presmooth_sigma[axis] ... */
    hipdrt_filter_table curv;                       /* ... and the order-2 Gaussian of curv_sigma = 1 */
    double k_factor[2], max_sigma[2];
    hipdrt_node_table_fn nodes;   /* adaptive = 1 */
    void* user;
} hipdrt_map_filter_args;
/* a[rows * cols] row-major, NaN = missing.  out[rows * cols]: every entry filled (fill_nans=True; the caller restores NaNs per
 * impute / impute_groups).  weights_out (optional, iterative): the final weights of iterate_gaussian_weights.  sigmas_out
 * (optional, adaptive): [ndim][rows * cols], the sigma fields of the last get_adaptive_sigmas.  Sums behind np.std run in a
 * fixed order: a call repeats itself bit for bit. */
int hipdrt_map_filter(hipdrt_ctx* ctx, const hipdrt_map_filter_args* args, const double* a, double* out, double* weights_out,
                      double* sigmas_out);

/* scipy.ndimage.median_filter / percentile_filter with size=(size_r, size_c), mode='reflect', origin 0, on a[rows * cols]
 * row-major, and hybdrt/filters/_filters.py:43-46 iqr_filter as the difference of two ranks of the same window.  The window of
 * an entry starts size // 2 before it on either axis; rank r is entry r of the sorted window (the median: size_r size_c / 2; a
 * percentile p: (int)(size_r size_c p / 100.0)).  A window that holds a NaN returns what scipy's quickselect returns on it
 * (NaN compares false), for 0 < rank < size - 1; at ranks 0 and size - 1 such a window gives NaN.  Windows of more than 49
 * entries: HIPDRT_E_UNSUPPORTED. */
#define HIPDRT_RANK_ONE 0    /* out = rank rank_lo                */
#define HIPDRT_RANK_DIFF 1   /* out = rank rank_hi - rank rank_lo */
int hipdrt_rank_filter(hipdrt_ctx* ctx, const double* a, int rows, int cols, int size_r, int size_c, int op, int rank_lo,
                       int rank_hi, double* out);

/* np.nanpercentile(a, q, axis=1) (by_row != 0: out[rows][nq]) or np.nanpercentile(a, q) (by_row == 0: out[nq]) with numpy's
 * 'linear' rule -- virtual index (n - 1) q / 100 among the n non-NaN values, a + (b - a) t between its neighbours, b - (b - a)
 * (1 - t) where t >= 0.5 -- as DRTMD.score_group_data_badness (hybdrt/mapping/drtmd.py:675-678) and stats.robust_std
 * (hybdrt/utils/stats.py:124-134) use it.  q[k] == HIPDRT_Q_NANMEDIAN: np.nanmedian's rule, the mean of the middle pair
 * (nddata.py:194).  Exact selection with integer histograms: the result does not depend on the launch.  -0 and +0 compare equal;
 * a segment without a number gives NaN.  1 <= nq <= 4. */
#define HIPDRT_Q_NANMEDIAN (-1.0)
int hipdrt_percentiles(hipdrt_ctx* ctx, const double* a, int rows, int cols, int by_row, const double* q, int nq, double* out);

/* The badness score of the rows of one array (hybdrt/mapping/drtmd.py: score_group_data_badness 642-735 for one of its two
 * arrays, score_group_fit_badness 737-747 and 783), between one upload and one download:
 *   scale            a <- (a - 0.5 (hi + lo)) / (range of scale_src) by row, the 2 % and 98 % nanpercentiles (drtmd.py:675-679)
 *   flag_outliers    nddata.flag_outliers(a, flag_size, thresh, p_prior, full_std_contribution) (nddata.py:152-175, with
 *                    impute_nans 135-149 through impute_gauss and preprocessing.outlier_prob, preprocessing.py:860-876); then a
 *                    row with fewer than (int)(0.05 cols) flagged entries has them set to NaN (drtmd.py:699-707)
 *   always           filt = median_filter(a, median_size); rss = flag_bad_obs(a, filt, std_size, return_rss=True,
 *                    robust_std=True) (nddata.py:178-211)
 * n_std is stats.std_normal_quantile(0.75), the denominator constant of robust_std.  HIPDRT_E_NUMERIC with the reference's
 * message when x_std contains NaNs (nddata.py:205-206); rss_out is filled all the same. */
typedef struct {
    int rows, cols;
    int scale, flag_outliers;
    int flag_size[2], median_size[2], std_size[2];
    double thresh, p_prior, full_std_contribution;
    double n_std;
    int impute;                            /* flag_outliers' impute= (its default, and what drtmd.py:695-696 runs, is 1) */
    hipdrt_filter_table impute_gauss[2];   /* impute: the Gaussian of impute_nans (sigma 0.5) per axis */
    int score;                             /* 1: the whole chain; 0: stop after flag_outliers (flags_out only, no 5 % rule) */
    const double* filt_in;                 /* optional [rows * cols]: flag_bad_obs against this array instead of the median
                                            * filter of a (nddata.flag_bad_obs with the caller's x_filt) */
} hipdrt_map_badness_args;
/* a[rows * cols]; scale_src[rows * cols] (scale = 1); rss_out[rows] (score = 1); flags_out[rows * cols] (optional, flag_outliers = 1): the
 * outlier flags; filt_out[rows * cols] (optional): the median-filtered array */
int hipdrt_map_badness(hipdrt_ctx* ctx, const hipdrt_map_badness_args* args, const double* a, const double* scale_src,
                       double* rss_out, unsigned char* flags_out, double* filt_out);

/* The prediction block of a DRTMD map (hybdrt/mapping/drtmd.py: predict_x 815-833, predict_drt 848-851, the clamp of
 * predict_drt_cov 993-1008 and the filter of predict_drt_var 1017-1019 on rows that already are diag(B x_cov B'),
 * predict_peak_prob 1023-1064 with curvature.peak_prob_1d (hybdrt/mapping/curvature.py:12-58), predict_curv_prob 1066-1106) on
 * the rows x[rows][nsup] of a map, between one upload and one download:
 *   x        normalize: x / (sum_j |x_j| basis_area) by row, first; then x_filter -- scipy.ndimage.gaussian_filter with 'reflect'
 *            along psi (axis 0, the rows) and / or tau (axis 1), a plain correlation: a NaN row spreads to its neighbours
 *   f, fxx   x E0', x E2' with the order-0 and order-2 evaluation matrices of hipdrt_func_eval_matrix
 *   f_var, fxx_var   var_stored = 0: used as given.  var_stored = 1 (stored raw variances): the map clamp with the row's ext = (li,
 *            ri) -- v[:li] = max(v[:li], v[li]), then v[ri:] = max(v[ri:], v[ri]); li < 0 or a NaN in the row: left alone -- and
 *            then x_filter
 *   peaks    search = 1 / -1: one pass on -search fxx; 0: the passes -1 and +1, each keeping peaks with pass * f > 0.  The
 *            probability at a peak is min(P(min(prominence, height) > 0), P(|f| > 0)), zero elsewhere; spread.radius >= 0: that row
 *            correlated along tau with the spread table, times spread_factor; then times sign(f)
 * Sums run in a fixed order per output element and without atomics: a row's results depend on its position in the map only
 * through the psi filter's window.  A row of x that is all NaN gives NaN rows.  neval is limited by the LDS the four staged rows of
 * a map row take (52 bytes per evaluation point): HIPDRT_E_UNSUPPORTED beyond that, with the limit in the message. */
typedef struct {
    int rows, nsup, neval;
    const double* ln_tau_sup;           /* [nsup] natural log of the supergrid  */
    const double* ln_tau_eval;          /* [neval] natural log of the evaluation grid */
    double epsilon, basis_area;
    int normalize;
    hipdrt_filter_table x_filter[2];    /* psi axis, tau axis; radius < 0 skips */
    const double* f_var;                /* optional [rows][neval]; both or none */
    const double* fxx_var;
    int var_stored;
    const int* ext;                     /* var_stored = 1: optional [rows][2], (li, ri) on the evaluation grid or (-1, -1) */
    int search;
    double height, prominence;
    hipdrt_filter_table spread;         /* radius < 0: no spread */
    double spread_factor;
} hipdrt_map_predict_args;
/* every output is optional: x_out[rows][nsup] the normalised and filtered x; f, fxx [rows][neval]; f_var_out, fxx_var_out
 * [rows][neval] the variances as they enter the square root; peak_prob, curv_prob [rows][neval] (both need the variances) */
int hipdrt_map_predict(hipdrt_ctx* ctx, const hipdrt_map_predict_args* args, const double* x, double* x_out, double* f,
                       double* fxx, double* f_var_out, double* fxx_var_out, double* peak_prob, double* curv_prob);

/* mat1d.construct_integrated_derivative_matrix (hybdrt/matrices/mat1d.py:125-209), orders 0,1,2 of the
 * Gaussian basis (closed forms basis.py:382-395).  toeplitz != 0: first column scattered (mat1d.py:158-168).
 * out: m0, m1, m2 each [n][n]                                                                        */
int hipdrt_penalty_matrices(hipdrt_ctx* ctx, const double* ln_tau, int n, double epsilon, int toeplitz,
                            double* m0, double* m1, double* m2);

/* mat1d.construct_eis_var_matrix (hybdrt/matrices/mat1d.py:493-515): out vmm[2nf][2nf], rows normalised.
 * uniform != 0 is error_structure='uniform'.                                                         */
int hipdrt_eis_var_matrix(hipdrt_ctx* ctx, const double* freq, int nf, double vmm_epsilon, double reim_cor,
                          int uniform, double* vmm);

/* ---- L2 QP ------------------------------------------------------------------------------------------ */

typedef struct {
    double abstol, reltol, feastol; /* cvxopt.solvers.options defaults 1e-7, 1e-6, 1e-7 */
    int maxiters;                   /* 100 */
} hipdrt_qp_opts;

/* cvxopt.solvers.qp(P, q, G=-I, h) as called from qphb.solve_convex_opt (hybdrt/models/qphb.py:512-519):
 * B independent problems min 1/2 x'Px + q'x s.t. -x <= h, solved with coneqp's trajectory.
 * P[B or 1][n][n] (p_batched selects; only the lower triangle is read), q[B][n], h[B or 1][n].
 * out: x[B][n], iters[B], pcost[B] ('primal objective'), status[B]
 * n <= 4096.  Many problems: one workgroup each (n <= 2048).  Few problems (B <= #CUs / 16, n > 256) or n > 2048: every
 * problem on up to 32 co-resident workgroups of one XCD; same iteration counts, x equal to rounding.   */
int hipdrt_qp_batch(hipdrt_ctx* ctx, int B, int n, int p_batched, const double* P, const double* q,
                    int h_batched, const double* h, const hipdrt_qp_opts* opts,
                    double* x, int* iters, double* pcost, int* status);

/* (diagnostic entry points -- kernel phase counters, occupancy, forcing a kernel choice -- are declared in hipdrt_debug.h:
 * they are not part of the drop-in boundary and nothing in the host layer's product path calls them)                          */

/* P = (W A)'(W A) + L2, q = -(W A)'(W b) + l1 of qphb.solve_convex_opt (qphb.py:465-466) for B weight
 * vectors over one shared A[m][n]:  w[B][m], b[B][m], l2[B or 1][n][n], l1[n] -> P[B][n][n], q[B][n]   */
int hipdrt_weighted_gram(hipdrt_ctx* ctx, int B, int m, int n, const double* A, const double* w,
                         const double* b, int l2_batched, const double* l2, const double* l1,
                         double* P, double* q);

/* ---- L3/L4 batched fit ------------------------------------------------------------------------------ */

typedef struct {
    /* qphb.get_default_hypers (hybdrt/models/qphb.py:208-255), eff_hp=True */
    double rp_scale;                 /* 14 */
    double derivative_weights[3];    /* 1.5, 1.0, 0.5 */
    double sigma_ds[3];              /* 1, 1000, 1000 */
    double l1_lambda_0;              /* 0 */
    double l2_lambda_0;              /* 142 */
    double s_alpha[3];               /* 5, 10, 25 */
    double s_0[3];                   /* 1, 1, 1 */
    double rho_alpha[3];             /* 0.15, 0.2, 0.25 */
    double rho_0[3];                 /* 1, 1, 1 */
    /* DRT._qphb_fit_core keyword defaults (hybdrt/models/drt1d.py:102-137) */
    double iw_l1_lambda_0, iw_l2_lambda_0;   /* 1e-4, 1e-4 */
    double ohmic_penalty, inductance_penalty; /* 1e-6, 1e-6 */
    double inductance_scale;         /* 1e-5 */
    double eis_vmm_epsilon, eis_reim_cor;    /* 0.25, 0.25 */
    double xtol;                     /* 1e-2 */
    int max_iter;                    /* 50 */
    int nonneg;                      /* 1 */
    int scale_data;                  /* 1 */
    int fit_ohmic, fit_inductance;   /* 1, 1 */
    int eis_error_uniform;           /* 0 (eis_error_structure=None) */
    int update_scale;                /* 0; 1: re-scale the data every iteration from the second on (drt1d.py:903-927) */
    int eff_hp;                      /* 1; 0: solve_s sees rho_k instead of 1 (qphb.py:747-750; other default alphas) */
    /* optional branches of the weight estimation; <= 0 means None (the reference defaults) */
    double outlier_p;                /* prior outlier probability, qphb.py:1497-1553, 1629-1656 */
    double iw_alpha, iw_beta;        /* prior on the initial weights, qphb.py:1471-1479, 1679 */
    hipdrt_qp_opts qp;
} hipdrt_fit_opts;

void hipdrt_default_fit_opts(hipdrt_fit_opts* o);

/* A plan = everything that does not depend on the measured impedances: lookups (DRTBase.__init__,
 * hybdrt/models/drtbase.py:138-156), Z'/Z'' (DRT._prep_impedance_fit_matrix, drt1d.py:5625-5657), penalty
 * matrices (_prep_penalty_matrices, 5673-5734), the stacked [Re;Im] response matrix and padded M_k
 * (_format_qp_matrices, 5736-5963), the variance-estimation matrix (drt1d.py:622-636), all built on the
 * device, plus work space for `capacity` spectra.  All spectra of a plan share freq[nf] and tau[ntau]
 * (the DRTMD case: mapping/drtmd.py:245-319 with one DRT instance and its recalc cache).
 * toeplitz_a / toeplitz_m carry the reference's Toeplitz decisions (host logic); wt_* are the lookup
 * abscissae and log_wt_* = np.log(wt_*) (both computed by the caller exactly as basis.py:655-669 does). */
int hipdrt_plan_create(hipdrt_ctx* ctx, const double* freq, int nf, const double* tau, int ntau,
                       double epsilon, int mode, int toeplitz_a, int toeplitz_m, int ngrid, int ny,
                       const double* wt_re, const double* wt_im, const double* log_wt_re,
                       const double* log_wt_im, const hipdrt_fit_opts* opts, int capacity,
                       hipdrt_plan** out);
int hipdrt_plan_destroy(hipdrt_plan* plan);
/* dimensions: n = ns + ntau unknowns, m = 2 nf rows, ns special parameters */
int hipdrt_plan_dims(hipdrt_plan* plan, int* n, int* m, int* ns);
/* copy a shared matrix of the plan back to the host: which = "lut_z_re","lut_z_im" [ngrid],
 * "a_re","a_im" [nf][ntau], "rm" [m][n], "m0","m1","m2" [n][n] (padded), "vmm" [m][m]; of the staged batch:
 * "rv" [B][m] scaled data, "x" [B][n] current solution, "coef_scale" [B], "var_floor" [B] (the variance floor of the weight
 * re-estimate), "row_factors" [B][m] (batched row factors only) */
int hipdrt_plan_get(hipdrt_plan* plan, const char* which, double* out, long long count);
/* replace the plan's lookup tables with externally supplied ones (multi-GPU: rank 0 builds them, RCCL
 * broadcasts, the other ranks install them) and rebuild the dependent matrices            */
int hipdrt_plan_set_lookup(hipdrt_plan* plan, const double* z_re, const double* z_im);

/* stage B <= capacity spectra (z_re[B][nf], z_im[B][nf], host) into the plan's device buffers */
int hipdrt_plan_upload(hipdrt_plan* plan, int B, const double* z_re, const double* z_im);
/* DRT._qphb_fit_core (drt1d.py:102-1104) for the staged spectra, entirely on the device: scale_data,
 * initialize_weights (qphb.py:1609-1681), the iterate_qphb loop (qphb.py:606-972) with per-spectrum
 * convergence masks, calculate_pq's q (qphb.py:1154-1183).  Asynchronous on the ctx stream except for one
 * 4-byte "all converged" read-back per outer iteration.                                                */
int hipdrt_plan_fit(hipdrt_plan* plan);
/* How many contiguous ranges ("sub-batches") hipdrt_plan_fit cuts the staged spectra into: every range runs the same device
 * loop on a stream of its own, side by side, inside the one call and the plan's own buffers -- what DRTMD's serial loop over
 * observations (hybdrt/mapping/drtmd.py:303-319) becomes when the tail of one range's launches is filled by the others'.
 * k = 0 (default): chosen from the batch size -- 1 below 600 spectra, 2 from 600 on, 4 from 1000 on (capped at the number of the
 * library's own streams, see hipdrt_stream: 3 under the runtime's default of 4 hardware queues; profiles/r06_subbatch_sweep.txt); the
 * ranges run on those streams, picked per fit by activity and compute pipe, so the choice no longer depends on what else the process
 * has created (profiles/r06_trace_queue_placement.txt).  k >= 1: that many (capped so that a range keeps >= 64 spectra).  A caller
 * that keeps four or more plans fitting at the same time (own contexts, own threads) should set k = 1 on each: the command processor
 * has four compute pipes, and launch sequences beyond four take turns (4 plans x 2 ranges: 1900 fits/s against 2372 for 4 x 1 at
 * 1250 spectra, profiles/r06_inflight_ranges.txt).  Plans with prepared matrices, a recorded history, weight factors or outlier_p
 * fit in one range.
 * Per-spectrum results do not depend on k (every kernel of the loop works per spectrum).                                    */
int hipdrt_plan_set_subbatches(hipdrt_plan* plan, int k);
/* device bytes ONE staged spectrum costs an EIS plan of this shape (nf frequencies, ntau basis points, ns special parameters):
 * 4.9 MB at 256 x 512 -- the factor and P in tile order are the bulk.  A map driver sizes its batches with it
 * (mapping.fit_observations cuts a map that would not fit 80 % of the device's memory into consecutive batches).             */
int hipdrt_plan_bytes_per_spectrum(int nf, int ntau, int ns, long long* bytes);
/* results for the B staged spectra (any pointer may be NULL):
 * x[B][n] QP solution in scaled units, fit_x[B][ntau] / r_inf[B] / induc[B] rescaled like
 * extract_qphb_parameters (drt1d.py:6228-6289), weights[B][m] (1/sigma, scaled units),
 * coef_scale[B], rho[B][3], s_vectors[B][3][n], q_vector[B][n], outer_iters[B], qp_iters_total[B],
 * status[B] (0 converged, 1 max_iter reached, <0 failed)                                              */
int hipdrt_plan_download(hipdrt_plan* plan, double* x, double* fit_x, double* r_inf, double* induc,
                         double* weights, double* coef_scale, double* rho, double* s_vectors,
                         double* q_vector, int* outer_iters, int* qp_iters_total, int* status);
/* final P (calculate_pq) of spectrum b: p[n][n].  After hipdrt_plan_fit: the matrix calculate_pq builds from the fit's final
 * state (true_weights x chrono / eis row factors, drt1d.py:990-1006).  After hipdrt_plan_continue (upstream's
 * _continue_from_init returns its history only and leaves fit_parameters alone): the same construction on the state the
 * restart ended with -- its last s / rho and the last re-estimated weights times the factors the restart's QPs saw (row
 * factors x weight_factor), q_vector of hipdrt_plan_download to match.  The posterior entry points below use this P.     */
int hipdrt_plan_get_p_matrix(hipdrt_plan* plan, int b, double* p);
/* Posterior variance of the fitted distribution on an evaluation grid: the diagonal of
 * DRT.estimate_distribution_cov (hybdrt/models/drt1d.py:3063-3151 with estimate_param_cov, 4116-4138; order 0, no
 * normalisation), i.e. what DRTMD.fit_observation stores as obs_drt_var (hybdrt/mapping/drtmd.py:278-279) before its
 * extend_var post-processing.  basis_eval[neval][ntau] = basis.construct_func_eval_matrix(ln basis_tau, ln tau_eval).
 * For every fitted spectrum: final P (calculate_pq state), P = L L' on the device, out[b][i] = |L^-1 b_i|^2 * cs_b^2.
 * status[b] (may be NULL): 0 ok, -1 P not positive definite (the reference's LinAlgError -> None).  n <= 4096. */
int hipdrt_plan_distribution_var(hipdrt_plan* plan, const double* basis_eval, int neval, double* out, int* status);
/* same machinery with the identity as evaluation rows: out[b][i] = diag(inv(P_b))_i * cs_b^2, the parameter variances
 * np.diag(DRT.estimate_param_cov()) (hybdrt/models/drt1d.py:4116-4138) of every fitted spectrum.  n <= 4096.          */
int hipdrt_plan_param_var(hipdrt_plan* plan, double* out, int* status);
/* The FULL matrices, for one fitted spectrum b: out[n][n] = inv(P_b) * cs_b^2 = DRT.estimate_param_cov() (drt1d.py:4116-4138;
 * the DOP rescaling of 4126-4130 is the caller's: it needs dop_scale_vector) -- what DRTMD's PFRT post-processing takes per
 * step (hybdrt/mapping/drtmd.py:934-941) -- and out[neval][neval] = basis_eval inv(P_b)[DRT block] basis_eval' * cs_b^2 =
 * DRT.estimate_distribution_cov (drt1d.py:3063-3151; order 0, no normalisation, before extend_var).  Same factorisation as
 * the variances: the evaluation rows ride along as extra panel rows and come out as rows L^-T, one more product gives
 * rows L^-T L^-1 rows'.  *status (may be NULL): 0 ok, -1 P not positive definite (out is then NaN).  n <= 4096.            */
int hipdrt_plan_param_cov(hipdrt_plan* plan, int b, double* out, int* status);
int hipdrt_plan_distribution_cov(hipdrt_plan* plan, int b, const double* basis_eval, int neval, double* out, int* status);

/* per-outer-iteration history of spectrum b recorded when record_history was enabled before the fit:
 * hist_x[iters][n], hist_rho[iters][3], hist_w[iters][m], qp_iters[iters+1]                            */
int hipdrt_plan_record_history(hipdrt_plan* plan, int b_or_minus1);
int hipdrt_plan_get_history(hipdrt_plan* plan, double* hist_x, double* hist_rho, double* hist_w,
                            int* qp_iters, int max_rows, int* rows);
/* Ingredients of DRT.evaluate_llh(weights=qphb.estimate_weights(x, rv, vmm, rm), x=x) (hybdrt/models/drt1d.py:4457-4496,
 * qphb.py:1347-1377) for the current x of every spectrum, as the PFRT driver evaluates it after each step
 * (drt1d.py:2618-2622): out rss[B] = weighted residual sum of squares, sum_log_w[B] = sum(log(weights)).
 * llh = a0 ln b0 - an ln(b0 + rss/2) + lgamma(an) - lgamma(a0) + sum_log_w with an = a0 - 1 + m/2.                 */
int hipdrt_plan_llh_terms(hipdrt_plan* plan, double* rss, double* sum_log_w);
/* The same two sums with the fit's own est_weights (qphb_params['est_weights']) as the weights: DRT.evaluate_rss() and
 * DRT.evaluate_llh() with their default arguments (hybdrt/models/drt1d.py:4433-4496), which DRTMD.fit_observation
 * records for every observation as obs_rss / obs_llh (hybdrt/mapping/drtmd.py:259-260).                              */
int hipdrt_plan_obs_llh_terms(hipdrt_plan* plan, double* rss, double* sum_log_w);
/* The same two sums for the other forms of the `weights` argument of DRT.evaluate_rss / evaluate_llh
 * (hybdrt/models/drt1d.py:4434-4443, 4459-4472): HIPDRT_LLH_W_EST = None (the fit's est_weights, as above),
 * HIPDRT_LLH_W_UNIFORM = "uniform" (within each domain -- chrono rows, impedance rows -- every weight is the mean of that
 * domain's est_weights: DRTMD's default llh_kw / rss_kw, hybdrt/mapping/drtmd.py:129-131), HIPDRT_LLH_W_SCALAR = one scalar
 * weight for every row.  `normalize=True` (division by the number of rows) is left to the caller.                     */
#define HIPDRT_LLH_W_EST 1
#define HIPDRT_LLH_W_UNIFORM 2
#define HIPDRT_LLH_W_SCALAR 3
int hipdrt_plan_obs_llh_terms_w(hipdrt_plan* plan, int weights_mode, double scalar_weight, double* rss, double* sum_log_w);

/* Overwrite parts of the fitted batch's state on the device (NULL = keep): x[B][n] (also becomes the previous iterate),
 * rho[B][3], s[B][3][n], weights[B][m].  The inputs of drt1d._continue_from_init (x_init, rho_vector, s_vectors, weights). */
int hipdrt_plan_set_state(hipdrt_plan* plan, const double* x, const double* rho, const double* s, const double* weights);
/* ... and dop_rho[B][3] of a prepared plan with a distribution of phasances (dop_rho_vector of _continue_from_init) */
int hipdrt_plan_set_state_dop(hipdrt_plan* plan, const double* dop_rho);

/* drt1d._continue_from_init (hybdrt/models/drt1d.py:1270-1365), any data type: re-enter the outer loop from the state on the
 * device with updated hyper-parameters (opts: s_0, l2_lambda_0, ..., xtol, max_iter), at least min_iter iterations;
 * every iteration first multiplies the weights by weight_factor -- and, on prepared plans, by the plan's row factors (the
 * chrono / eis weight factors, 1314-1316: hipdrt_plan_set_weight_factors(plan, 1, rows, batched) beforehand).  est_weights,
 * xmx / dop_xmx norms and the data scale are kept.  Joint fits: the vz_offset column of every measurement's matrix is
 * rewritten after each iteration as in the fit, but from a copy whose offset column is frozen as this call found it
 * (1295-1298, 1353-1357) -- the reference's behaviour, so a chain of warm restarts reproduces pfrt_fit_hybrid (2558-2715).
 * Results through hipdrt_plan_download / _get_history as after hipdrt_plan_fit (outer_iters = iterations of this call).
 * Used by the candidate generators (drt1d.py:1497-1632) and PFRT (2558-2715, DRTMD fit_type='pfrt': drtmd.py:98-100, 1338).
 * opts->outlier_p > 0 (any plan; it may differ from the fit's): estimate_weights forms outlier_t and T V T anew from every
 * iterate (qphb.py:1545-1594) -- the outlier_t / outlier_tvt a caller hands _continue_from_init are never read (1300-1304).  */
int hipdrt_plan_continue(hipdrt_plan* plan, const hipdrt_fit_opts* opts, double weight_factor, int min_iter);

/* ---- prepared-matrix plans: the same device loop for any data type (config-5 family) -----------------------------
 * DRT._qphb_fit_core (hybdrt/models/drt1d.py:551-1006) is data-type agnostic once _prep_for_fit / _format_qp_matrices
 * (5439-5558, 5736-5963) have produced the stacked matrix rzm, the data vector rzv, the padded penalty matrices and the
 * stacked variance-estimation matrix.  A prepared plan takes exactly those (built by the caller from the stand-alone
 * builders above) and runs initialize_weights + the iterate_qphb loop on the device, including
 *   - the x_dop hyper-parameter pass (hybdrt/models/qphb.py:822-933) and the DOP block of the L2 matrix (qphb.py:92-100),
 *   - the per-iteration rewrite of the vz_offset column of a hybrid fit (drt1d.py:973-979).
 * Weight factors are 1 (hybrid_weight_factor_method=None, drt1d.py:785-787).                                          */
typedef struct {
    int m, n, ns;              /* rows of rzm, unknowns, special (non-DRT) unknowns ahead of the DRT block            */
    int dop_start, dop_size;   /* the x_dop block inside the specials (dop_size 0: none)                              */
    int vz_index;              /* column of vz_offset (-1: none)                                                      */
    int vb_start, vb_size;     /* v_baseline columns: excluded from the vz prediction (drt1d.py:507-511)              */
    int num_chrono;            /* rows [0, num_chrono) are chrono samples, the rest [Re; Im] impedance rows           */
    int toeplitz_m;            /* DRT block of the penalty matrices is symmetric Toeplitz (uniform ln tau)            */
    int chrono_vmm_uniform;    /* chrono block of vmm is the 'uniform' error structure (all rows equal): one row is read */
    double basis_area;         /* area of one tau basis function, sqrt(pi)/epsilon for the Gaussian basis (update_scale) */
    int init_weights_separately; /* 1: initialize_weights once per data block (chrono rows, impedance rows), each QP seeing
                                  only its block and each block with its own variance floor (drt1d.py:648-672)         */
    int weight_method;         /* 1: hybrid_weight_factor_method='weight' -- row factors from the blocks' weight scales
                                  after initialize_weights (drt1d.py:748-760); fixed_*_factor > 0 overrides one of them;
                                  the factors used are returned by hipdrt_plan_get("weight_factors") [B][2] = chrono, eis */
    double fixed_chrono_factor, fixed_eis_factor;
    double dop_l2_lambda_0;                                       /* qphb.py:243-253 */
    double dop_derivative_weights[3], dop_s_alpha[3], dop_rho_alpha[3], dop_s_0[3], dop_rho_0[3];
} hipdrt_prepared_desc;
/* m0,m1,m2 [n][n] padded penalty matrices; vmm [m][m]; h [n] (make_h_constraint, qphb.py:521-557); l1 [n]
 * (l1_lambda_vector, drt1d.py:552-556); vz_strength [m] (drt1d.py:514-519; NULL when vz_index < 0).
 * opts: the fit options (scale_data / rp_scale / fit_ohmic / fit_inductance / eis_* are ignored: the caller prepared
 * the data).                                                                                                         */
int hipdrt_plan_create_prepared(hipdrt_ctx* ctx, const hipdrt_prepared_desc* desc, const double* m0, const double* m1,
                                const double* m2, const double* vmm, const double* h, const double* l1,
                                const double* vz_strength, const hipdrt_fit_opts* opts, int capacity,
                                hipdrt_plan** out);
/* stage B measurements: rzm [B][m][n] (rm_batched != 0) or one shared [m][n]; rzv [B][m].  A vz_offset column needs
 * per-measurement matrices.  Then hipdrt_plan_fit; results through hipdrt_plan_download (x, weights, rho, s_vectors,
 * q_vector, iteration counts, status; pass NULL for fit_x / r_inf / induc), hipdrt_plan_get_p_matrix and
 * hipdrt_plan_get ("dop_rho" [B][3], "xmx", "dop_xmx" [B][3], "est_weights", "rzm" [B or 1][m][n] = final matrix;
 * with outlier_p set also "outlier_t" [B][m], qphb.py:1497-1520, of the last weight estimation -- with max_iter = 0 that
 * is initialize_weights', which is what remove_outliers thresholds, drt1d.py:817-833).                                  */
int hipdrt_plan_upload_prepared(hipdrt_plan* plan, int B, int rm_batched, const double* rzm, const double* rzv);

/* One qphb.iterate_qphb (hybdrt/models/qphb.py:606-972) on every staged measurement of a prepared plan -- the body of
 * _qphb_fit_core's loop as the reference exposes it: solve the QP built from (weights, s_vectors, rho_vector, dop_rho_vector),
 * update s_vectors / rho_vector (733-817) and the DOP pair (822-933) from the new x with the given xmx norms, re-estimate the
 * weights against est_weights (936), and test is_converged(x_in, x) (967-970).  A NULL member keeps the value on the device
 * (defaults after hipdrt_plan_upload_prepared: x 1e-6, s = s_0, rho = rho_0, weights = est_weights... = 1, norms 1; after
 * hipdrt_plan_fit: the fit's), so repeated calls with in = NULL continue from their own results.  Not included: what
 * _qphb_fit_core does around the call (xmx norms of the first iteration, update_scale, the vz_offset column, weight factors).
 * Results through hipdrt_plan_download (x, weights, rho, s_vectors) and hipdrt_plan_get("dop_rho"); the optional
 * outputs [B]: is_converged, and of the QP its status (HIPDRT_QP_*), iteration count and 'primal objective'. */
typedef struct {
    const double* x_in;           /* [B][n]    */
    const double* s_vectors;      /* [B][3][n] */
    const double* rho;            /* [B][3]    */
    const double* dop_rho;        /* [B][3]    */
    const double* weights;        /* [B][m]    */
    const double* est_weights;    /* [B][m]    */
    const double* xmx_norms;      /* [B][3]    */
    const double* dop_xmx_norms;  /* [B][3]    */
} hipdrt_iterate_state;
int hipdrt_plan_iterate(hipdrt_plan* plan, const hipdrt_iterate_state* in, int* converged, int* qp_status, int* qp_iters,
                        double* primal_objective);

/* Weight factors of _qphb_fit_core (hybdrt/models/drt1d.py:887-901, 990-1000): every outer iteration solves its QP with
 * weights * row_factors (chrono_weight_factor on the chrono rows, eis_weight_factor on the impedance rows; NULL = 1),
 * from the second iteration on also * weight_factor; estimate_weights keeps working on the unscaled weights.  After the
 * fit hipdrt_plan_download returns weights * weight_factor ("true_weights"); q_vector / p_matrix / the posterior
 * variances use those times the row factors ("scaled weights").  row_factors: [m], or [capacity][m] when batched != 0.
 * Applies to every later hipdrt_plan_fit of the plan (any plan kind); (1.0, NULL) switches it off.  batched bit 1 (value
 * 2): the row factors are a vector-valued weight_factor (kk_fit, drt1d.py:1393-1411) -- applied from the second iteration
 * on only and folded into the returned weights.                                                                        */
int hipdrt_plan_set_weight_factors(hipdrt_plan* plan, double weight_factor, const double* row_factors, int batched);
/* Constraint vector of the initialize_weights QP when it differs from the loop's (neg_allowed_tau_range: the loop allows
 * negative coefficients only inside a tau window, initialize_weights everywhere; hybdrt/models/drt1d.py:467, 657-660 vs
 * 944, hybdrt/models/qphb.py:521-557).  h_init[n]; NULL restores the plan's single h.                                   */
int hipdrt_plan_set_init_h(hipdrt_plan* plan, const double* h_init);

/* ---- Kramers-Kronig screening of the fitted batch ---------------------------------------------------------------------
 * Options of DRT.kk_test's screening step (hybdrt/models/drt1d.py:1370-1391): n_outlier_iter / p_thresh / n_sigma /
 * std_sample_fraction are the arguments of kk.get_outliers (hybdrt/models/kk.py:21-53), max_num_outliers that of kk.get_limits
 * (kk.py:56-123), outlier_weight the row factor kk_fit gives an outlier (drt1d.py:1403-1404).  n_std is the standard-normal
 * quantile of 0.5 + std_sample_fraction / 2 (stats.robust_std, hybdrt/utils/stats.py:124-134), supplied by the caller.      */
typedef struct {
    int n_outlier_iter;           /* 2 */
    double p_thresh;              /* 1e-4 */
    double n_sigma;               /* -1; <= 0 means None: the chi-squared test with p_thresh, else |e| > n_sigma * std */
    double std_sample_fraction;   /* 0.6 */
    double n_std;                 /* 0.8416212335729143 */
    int max_num_outliers;         /* 2 */
    double outlier_weight;        /* 1e-10 */
} hipdrt_kk_opts;
void hipdrt_default_kk_opts(hipdrt_kk_opts* o);
/* DRT.eval_kk_residuals + get_kk_outliers + get_kk_limits (drt1d.py:1472-1491) for every spectrum of the fitted batch, on the
 * device, one workgroup per spectrum: the prediction at the fit frequencies yh = rm x (predict_z, in data units:
 * z_hat = coef_scale * yh), residuals e = 100 (z - z_hat) / |z| (kk.normalize_residuals, norm="modulus", kk.py:9-19), the outlier
 * mask of kk.get_outliers -- robust std from numpy's linear percentiles 50 -/+ 100 fraction / 2 of the unmasked Re and Im
 * residuals, then exp(-|e|^2 / (2 std^2)) < p_thresh (= 1 - chi2.cdf(|e|^2, 2, scale=std^2)) or |e| > n_sigma std, n_outlier_iter
 * times; fewer than two values left, or a std that is zero or not finite, masks nothing -- and the clean window of kk.get_limits.
 * Plain EIS plans (hipdrt_plan_create) whose frequency grid is strictly ascending or descending; anything else, or a shape whose
 * residuals, sort buffer, x and prediction do not fit one workgroup's LDS (nf <= 2048 with n <= 4096 fits), is HIPDRT_E_INVALID
 * before any launch.
 * out (host; any may be NULL): z_hat_re, z_hat_im [B][nf]; err_re, err_im [B][nf] percent of |Z|; std [B] of the last outlier
 * iteration; outlier_mask [B][nf]; f_lim [B][2] = f_min, f_max; i_lim [B][2] = i_left, i_right, positions in descending-frequency
 * order; status [B]: 0 ok, 1 no clean point (the reference raises IndexError; limits NaN, indices -1), -1 the spectrum's fit
 * failed (outputs NaN, mask empty, row factors 1).
 * set_row_factors != 0: the next fit's row factors are written on the device into the plan's batched row-factor buffer -- rows k and
 * nf + k get outlier_weight for masked k and 1 elsewhere (drt1d.py:1399-1404) -- and the plan is left as
 * hipdrt_plan_set_weight_factors(plan, 1.0, rows, 3) would leave it.  Fits with row factors run in one range
 * (hipdrt_plan_set_subbatches).                                                                                              */
int hipdrt_plan_kk_screen(hipdrt_plan* plan, const hipdrt_kk_opts* opts, int set_row_factors,
                          double* z_hat_re, double* z_hat_im, double* err_re, double* err_im,
                          double* std, int* outlier_mask, double* f_lim, int* i_lim, int* status);

/* ---- model evaluation: what a user does first with a finished fit ---------------------------------------------------------
 * basis.construct_func_eval_matrix (hybdrt/matrices/basis.py:488-514) with get_basis_func_derivative (218-228), gaussian basis:
 * out[ne][nb], out[i][j] = phi^(order)(eval_grid[i] - basis_grid[j]; epsilon) for natural-log grids; order 0: exp(-(eps y)^2),
 * 1: -2 eps^2 y phi, 2: (-2 eps^2 + 4 eps^4 y^2) phi, evaluated in numpy's order of operations.                              */
int hipdrt_func_eval_matrix(hipdrt_ctx* ctx, const double* basis_grid, int nb, const double* eval_grid, int ne, double epsilon,
                            int order, double* out);
/* A prepared plan holds no tau grid: give it ln(basis_tau)[nb] and the basis epsilon before hipdrt_plan_predict_drt /
 * hipdrt_plan_predict_resistances.  Its DRT block (n - ns columns) must hold one copy of the basis, or two (series_neg: positive
 * copy, then negative copy; drt1d.py:2961-2963).  Plans made by hipdrt_plan_create know their basis: the call is refused there. */
int hipdrt_plan_set_tau_basis(hipdrt_plan* plan, const double* ln_basis_tau, int nb, double epsilon);
/* per-spectrum status of hipdrt_plan_predict_drt when the band was asked for and P is not positive definite (the reference's
 * LinAlgError -> (None, None), drt1d.py:3229-3231): mu is valid, lo and hi are NaN                                             */
#define HIPDRT_PREDICT_NOT_PD (-3)
/* DRT.predict_drt (hybdrt/models/drt1d.py:3040-3061) and DRT.predict_drt_ci (3209-3231) for every spectrum of the fitted batch:
 * mu[b][i] = scale_b * sum_j E[i][j] x_b[j] with E the evaluation matrix above at ln_tau_eval[neval], x_b the DRT block of the
 * solution on the device, scale_b the coefficient scale -- divided by that spectrum's own R_p (normalize = 1; 2: by R_p of |x|,
 * abs_norm; get_drt_norm, 3020-3031).  sign is get_drt_params' (2965-2987): 1 = +x+, -1 = -x-, 0 = x+ - x-; a one-copy block takes
 * 1 only.  lo, hi (may be NULL: then nothing is factorised) = mu + s_lo sigma, mu + s_hi sigma with
 * sigma^2 = diag(E inv(P) E') scale_b^2 (estimate_distribution_cov, 3063-3151, before extend_var) from the same Cholesky kernel
 * as hipdrt_plan_distribution_var, fed the device-resident E; s_lo, s_hi are the caller's numbers of standard deviations
 * (stats.std_normal_quantile of the quantiles).  mu, lo, hi: [B][neval].  status[B] (may be NULL): the fit's status (0, 1; < 0
 * failed: the row is NaN), or HIPDRT_PREDICT_NOT_PD.  Plain and prepared plans; a prepared plan runs at unit scale
 * (coefficient scale 1: the caller rescales) and needs hipdrt_plan_set_tau_basis.  Every output element is accumulated in one
 * fixed order that depends neither on B nor on the spectrum's position: alone or in a batch, a spectrum gives the same bits.   */
int hipdrt_plan_predict_drt(hipdrt_plan* plan, const double* ln_tau_eval, int neval, int order, int sign, int normalize,
                            double s_lo, double s_hi, double* mu, double* lo, double* hi, int* status);
/* DRT.predict_z (drt1d.py:3500-3542; include_vz_offset / include_dop / include_cap do not apply to a plain EIS fit) at ANY
 * frequencies freq[nf]: Z = cs (A' x + j A'' x) + R_inf + j 2 pi f L in data units, A', A'' built on the device at freq from the
 * plan's own lookup tables, tau grid and integration mode (mat1d.construct_impedance_matrix, hybdrt/matrices/mat1d.py:212-374,
 * with np.interp's clamp outside the tables, 353-372).  include_mask: bit 0 the DRT term, bit 1 R_inf, bit 2 the inductance
 * (include_drt / include_ohmic / include_inductance).  z_re, z_im [B][nf]; status[B] (may be NULL) the fit's status, rows of a
 * failed fit are NaN.  Plain EIS plans only: a prepared plan returns HIPDRT_E_UNSUPPORTED.                                      */
int hipdrt_plan_predict_z(hipdrt_plan* plan, const double* freq, int nf, int include_mask, double* z_re, double* z_im,
                          int* status);
/* DRT.predict_r_p (drt1d.py:3552-3571; abs_norm != 0: absolute=True), predict_r_inf (3573-3581) and predict_r_tot (3583-3584) of
 * every fitted spectrum, in data units; each output [B], any may be NULL.  A prepared plan gives r_p only (unit scale;
 * HIPDRT_E_UNSUPPORTED when r_inf or r_tot is asked for).                                                                       */
int hipdrt_plan_predict_resistances(hipdrt_plan* plan, double* r_p, double* r_inf, double* r_tot, int abs_norm);

/* ---- model evaluation of a prepared plan: voltage response, impedance and distribution of phasances ---------------------------
 * A prepared plan runs at unit scale and does not know what its special columns mean; hipdrt_prepared_desc gives it dop_start /
 * dop_size, vz_index and vb_start / vb_size.  This is the rest of what DRT.extract_qphb_parameters (hybdrt/models/drt1d.py:
 * 6228-6289) needs to turn the scaled solution into data units, given AFTER a fit (the per-member scales change under solve_rp and
 * update_scale; they must be the post-fit values).  Arrays are copied; a NULL array is allowed where its block is absent.        */
typedef struct {
    int idx_rinf, idx_induc, idx_cinv;         /* columns of R_inf, inductance and C_inv (-1: none)                              */
    double inductance_scale, capacitance_scale;
    const double* dop_scale_vector;            /* [dop_size], or [B][dop_size] when dop_scale_batched != 0: solve_rp rescales the
                                                  DOP columns of every member by that member's own factor (drt1d.py:596-606)     */
    int dop_scale_batched;
    const double* v_baseline_scale;            /* [vb_size]: the column normalisation of the baseline block                     */
    const double* coefficient_scale;           /* [B]                                                                           */
    const double* response_signal_scale;       /* [B] (NULL: a plan without chrono rows)                                        */
    const double* scaled_response_offset;      /* [B] (NULL: 0)                                                                 */
} hipdrt_predict_desc;
/* B = the fitted batch.  HIPDRT_E_INVALID for a plan that is not prepared or holds no fitted batch, for an index outside the
 * special block, a shared scale that is not finite, or a missing array of a block the plan has.  Holds until the next upload.           */
int hipdrt_plan_set_predict_desc(hipdrt_plan* plan, const hipdrt_predict_desc* desc);

/* terms of hipdrt_plan_predict_response (include_drt / include_ohmic / include_cap / include_dop / include_vz_offset of
 * DRT.predict_response, and its v_baseline)                                                                                    */
#define HIPDRT_INCLUDE_DRT 1
#define HIPDRT_INCLUDE_OHMIC 2
#define HIPDRT_INCLUDE_CAP 4
#define HIPDRT_INCLUDE_DOP 8
#define HIPDRT_INCLUDE_VZ_OFFSET 16
#define HIPDRT_INCLUDE_BASELINE 32
#define HIPDRT_INCLUDE_INDUCTANCE 64   /* hipdrt_plan_predict_z_model only: ideal steps induce nothing, the response ignores it */
typedef struct {
    const double* times; int nt;               /* prediction times, any                                                         */
    const double* step_times; int nsteps;      /* [S] shared by the batch                                                       */
    const double* step_sizes; int sizes_batched;   /* [S], or [B][S] when sizes_batched != 0                                    */
    const double* basis_tau;                   /* [nb of hipdrt_plan_set_tau_basis]: the tau basis itself (not its logarithm)    */
    int mode, ny;                              /* HIPDRT_MODE_INTERP / _TRAPZ and the trapezoid's points, as hipdrt_response_matrix */
    int ngrid; const double *log_td, *v;       /* the response lookup table (INTERP)                                            */
    const double* basis_nu; double nu_epsilon; /* [dop_size], needed when the DOP term is on and the plan has a DOP block        */
    const double* inf_rv; int inf_batched;     /* ohmic response vector [nt] or [B][nt] (mat1d.construct_ohmic_response_vector)  */
    const double* cap_rv; int cap_batched;     /* capacitance response vector [nt] or [B][nt]                                   */
    const double* vz_strength;                 /* [nt] chrono strength of the vz offset at `times` (drt1d.py:6173-6226)          */
    const double* vb_mat;                      /* [nt][vb_size] background.get_baseline_matrix(times, normalize=False)           */
    int include_mask;                          /* HIPDRT_INCLUDE_* bits                                                        */
} hipdrt_response_args;
/* DRT.predict_response (drt1d.py:3363-3464; ideal steps, galvanostatic, background subtracted) for every member of the fitted
 * batch of a prepared plan, at any times: out[b][i] in data units.  The unit-step layers U[S][nt][ntau] (and the phasor-V layers
 * of a DOP block, applied to every member's DOP block times its own dop_scale_vector) are built once for the batch by the kernels of
 * hipdrt_response_matrix / hipdrt_phasor_v_matrix; their S nt stacked rows are applied to every member's resident x by the kernel
 * of hipdrt_plan_predict_drt (both copies of a series_neg block); response_assemble_kernel then forms, per (b, i),
 *   ( sum_s size[b][s] T_drt[b][s][i] + sum_s size[b][s] T_dop[b][s][i] + r_inf inf_rv[i] + c_inv cap_rv[i] )
 *   * (1 + vz_offset_b strength[i]) + vb_mat[i] . v_baseline_b
 * with the sums over s ascending in one accumulator, so a member gives the same bits alone and inside a batch.  No per-member
 * [B][nt][ntau] matrix is formed.  A term whose bit is off, or whose block or vector is absent (NULL), is left out.  status[B] (may
 * be NULL): the fit's status; the row of a failed fit is NaN.  Needs hipdrt_plan_set_tau_basis and hipdrt_plan_set_predict_desc
 * (HIPDRT_E_INVALID says which is missing).                                                                                     */
int hipdrt_plan_predict_response(hipdrt_plan* plan, const hipdrt_response_args* args, double* out, int* status);

typedef struct {
    const double* freq; int nf;                /* prediction frequencies, any (positive)                                         */
    const double* basis_tau;                   /* [nb of hipdrt_plan_set_tau_basis]                                              */
    int mode, ny;                              /* as hipdrt_impedance_matrix                                                     */
    int ngrid; const double *log_wt_re, *z_re, *log_wt_im, *z_im;   /* the impedance lookup tables (INTERP)                      */
    const double* basis_nu; double nu_epsilon; /* [dop_size], needed when the DOP term is on and the plan has a DOP block        */
    const double* vz_strength;                 /* [nf] eis strength of the vz offset at `freq` (drt1d.py:6173-6226), or NULL     */
    int include_mask;                          /* HIPDRT_INCLUDE_DRT, _OHMIC, _CAP, _DOP, _VZ_OFFSET, _INDUCTANCE                */
} hipdrt_z_model_args;
/* DRT.predict_z (drt1d.py:3500-3542) for every member of the fitted batch of a PREPARED plan (hybrid, fit_dop, fit_capacitance,
 * solve_rp, series_neg fits), at any frequencies: [A'; A''] (mat1d.construct_impedance_matrix, no Toeplitz shortcut) and the
 * phasor-Z rows of a DOP block (phasance.construct_phasor_z_matrix; applied to x_dop times the member's dop_scale_vector) are built at freq
 * and applied to the resident x by the kernel of hipdrt_plan_predict_drt; z_model_assemble_kernel adds R_inf, j 2 pi f L,
 * C_inv / (j 2 pi f) and the DOP term in data units and multiplies by 1 - vz_offset strength[f].  z_re, z_im [B][nf]; status[B]
 * (may be NULL) the fit's status, rows of a failed fit are NaN.  Needs hipdrt_plan_set_tau_basis and
 * hipdrt_plan_set_predict_desc.  hipdrt_plan_predict_z is unchanged: it serves plain EIS plans and refuses prepared ones.        */
int hipdrt_plan_predict_z_model(hipdrt_plan* plan, const hipdrt_z_model_args* args, double* z_re, double* z_im, int* status);

/* DRT.predict_dop (drt1d.py:3273-3347; order 0, no delta_density) for every member of the fitted batch of a prepared plan with a
 * DOP block: out[b][i] = cs_b sum_j E[i][j] dop_scale_vector_b[j] x_b[dop_start + j] with E = hipdrt_func_eval_matrix(basis_nu, nu,
 * nu_epsilon), divided by normalize_by[i] (get_dop_norm, 3349-3361: the caller's vector, NULL = not normalised); include_ideal != 0
 * adds R_inf at nu = 0, the inductance at nu = 1 and C_inv at nu = -1 as upstream adds them (divided by normalize_by[i] *
 * nu_basis_area when normalised).  nu [nn] in ascending order; out [B][nn]; status[B] may be NULL; a failed fit gives a NaN row.
 * Needs hipdrt_plan_set_predict_desc.                                                                                            */
int hipdrt_plan_predict_dop(hipdrt_plan* plan, const double* nu, int nn, const double* basis_nu, double nu_epsilon,
                            const double* normalize_by, double nu_basis_area, int include_ideal, double* out, int* status);

typedef struct {
    const double* nu; int nn;                  /* evaluation grid, finite and ascending                                          */
    const double* basis_nu; double nu_epsilon; /* [dop_size] the DOP basis grid and its Gaussian epsilon                         */
    int order;                                 /* 0, 1, 2: the derivative of the basis that the rows evaluate                    */
    const double* normalize_by;                /* [nn] get_dop_norm's vector, or NULL: not normalised                            */
    double nu_basis_area;                      /* area of one basis function (read with normalize_by only)                       */
    int include_ideal;                         /* R_inf, inductance and C_inv added to the mean at nu = 0, 1, -1                 */
    double s_lo, s_hi;                         /* numbers of standard deviations of the band (stats.std_normal_quantile)         */
} hipdrt_dop_args;
/* DRT.predict_dop_ci (drt1d.py:3233-3258) and the diagonal of DRT.estimate_dop_cov (3153-3198) for every member of the fitted batch
 * of a prepared plan with a DOP block, at derivative order 0, 1 or 2.  mu is hipdrt_plan_predict_dop's chain fed the order-k rows
 * E = hipdrt_func_eval_matrix(basis_nu, nu, nu_epsilon, order) (order 0: the bits of hipdrt_plan_predict_dop).  The variance is
 *   var[b][i] = e_i' D_b inv(P_b)[dop, dop] D_b e_i cs_b^2 / normalize_by[i]^2,   D_b = diag(dop_scale_vector_b)
 * (estimate_param_cov's two-sided rescaling, 4126-4133): the packed image of every member's final P is scaled by 1 / dop_scale_vector_b
 * on its DOP rows and columns (inv(S P S) = D inv(P) D), and the shared rows, placed over the DOP columns, go through the Cholesky
 * kernel of hipdrt_plan_distribution_var: one Gram/L2 rebuild and one factorisation per member.  lo, hi = mu + s_lo sigma,
 * mu + s_hi sigma with sigma = sqrt(var cs^2) / normalize_by; upstream adds no variance for the ideal elements, nor is any added here.
 * mu, lo, hi, var: [B][nn], each may be NULL; with lo, hi and var all NULL nothing is factorised.  status [B] (may be NULL): the
 * fit's status (< 0: NaN rows), or HIPDRT_PREDICT_NOT_PD when a variance was asked for and P is not positive definite (lo, hi, var
 * NaN, mu valid).  Needs hipdrt_plan_set_predict_desc.  HIPDRT_E_INVALID for a plan without a DOP block, nu not ascending, order
 * outside 0..2, n > 4096, or a dop_scale_vector entry of a member with a good fit that is not finite and positive.               */
int hipdrt_plan_dop_posterior(hipdrt_plan* plan, const hipdrt_dop_args* args, double* mu, double* lo, double* hi, double* var,
                              int* status);
/* DRT.estimate_dop_cov (drt1d.py:3153-3198; var_floor is the caller's) of member b: out [nn][nn] =
 * E D_b inv(P_b)[dop, dop] D_b E' cs_b^2, column j divided by normalize_by[j]^2 as upstream's broadcast divides it (the matrix is
 * then not symmetric), from the same scaled image of P in the single-member form and rows_outer_kernel, as
 * hipdrt_plan_distribution_cov.  include_ideal, s_lo and s_hi are not read.  *status (may be NULL): the fit's status, or
 * HIPDRT_PREDICT_NOT_PD; out is NaN for either.  The refusals of hipdrt_plan_dop_posterior, and b outside the batch.                */
int hipdrt_plan_dop_cov(hipdrt_plan* plan, int b, const hipdrt_dop_args* args, double* out, int* status);

/* ---- peak finding for the fitted batch ---------------------------------------------------------------------------------------
 * Options of DRT.find_peaks (hybdrt/models/drt1d.py:3753-3947) and of the map's peak probabilities (curvature.peak_prob_1d,
 * hybdrt/mapping/curvature.py:12-58; DRTMD.predict_curv_prob, hybdrt/mapping/drtmd.py:1097-1104).                              */
typedef struct {
    int eval_sign;         /* 1; get_drt_params' sign of the evaluated rows (as hipdrt_plan_predict_drt's sign)                 */
    int search;            /* 1; +1 / -1: one scipy.signal.find_peaks pass on -search * fxx; 0: the passes -1 and +1, each keeping
                              the peaks with pass * f[p] > 0 (upstream: search = sign if nonneg and sign != 0, else 0)           */
    int normalize;         /* 1; 0, 1 (by R_p) or 2 (by absolute R_p), as hipdrt_plan_predict_drt's normalize                   */
    int method;            /* 0; 0 'thresh', 1 'prob', 2 the map probabilities (peak_prob and curv_prob rows)                   */
    double height;         /* NaN = automatic: 0 for method 0, else 1e-3                                                        */
    double prominence;     /* NaN = automatic: 0.05 np.std(fxx) + 5e-3 for method 0, else 5e-3                                  */
    double prob_thresh;    /* 0.25; method 1 keeps peaks with 1 - erfc(min(prominence, height) / (sigma sqrt 2)) >= prob_thresh  */
    int num_peaks;         /* 0 = off; method 1: the threshold becomes the min(num_peaks, count)-th largest probability        */
    double fxx_var_floor;  /* 1e-5; lower bound of the curvature's variance (methods 1 and 2; <= 0: none)                        */
    int ext_left;          /* -1 = off; extend_var (drt1d.py:3123-3140): var[:ext_left] = max(var[:ext_left], var[ext_left])     */
    int ext_right;         /* -1 = off; var[ext_right:] = max(var[ext_right:], var[ext_right])                                  */
} hipdrt_peak_opts;
void hipdrt_peak_opts_default(hipdrt_peak_opts* o);
/* Peaks of every spectrum of the fitted batch on the evaluation grid ln_tau_eval[neval], found on the device: the rows fxx (order
 * 2) and, where the options need it, f (order 0) are evaluated as hipdrt_plan_predict_drt evaluates them (same kernels, same
 * bits), for methods 1 and 2 sigma^2 = diag(E inv(P) E') scale_b^2 / norm_b^2 comes from ONE factorisation per spectrum fed both
 * orders' rows, then extend_var's clamp and the floor; one workgroup per spectrum then applies the rule (csrc/peaks.hip;
 * hipdrt/models/peaks.py is its numpy statement).  row_scale[B] (may be NULL) multiplies every spectrum's coefficient scale when
 * normalize = 0: a prepared plan runs at unit scale and its caller knows the scales; the thresholds are absolute, so here the
 * scale cannot be applied afterwards.
 * out (host; any may be NULL), all dense on the grid: peak_sign [B][neval] 0, or the pass (+1 / -1) of a peak that passed height,
 * prominence and the f test; keep [B][neval] 0 / 1 (= peak_sign != 0 unless method 1 filters by probability); heights,
 * prominences, probs [B][neval], zero where there is no peak (probs: method 1 the peak probability, 2 the unsigned peak_prob_1d
 * value); left_bases, right_bases [B][neval], -1 where there is no peak; count [B] peaks kept; used_prominence [B]; peak_prob,
 * curv_prob [B][neval] (method 2 only, else left untouched); status [B]: the fit's status, or HIPDRT_PREDICT_NOT_PD where sigma is
 * needed and P is not positive definite.  A spectrum with a negative status has count 0, empty integer rows and NaN float rows.
 * HIPDRT_E_INVALID, before any launch, for options out of range and for a neval whose rows do not fit one workgroup's LDS
 * (neval <= 2048 fits in every mode).  Plain and prepared plans (hipdrt_plan_set_tau_basis first).  The result of a spectrum
 * depends neither on B nor on its position in the batch.                                                                        */
int hipdrt_plan_find_peaks(hipdrt_plan* plan, const double* ln_tau_eval, int neval, const hipdrt_peak_opts* opts,
                           const double* row_scale, int* peak_sign, int* keep, double* heights, double* prominences, double* probs,
                           int* left_bases, int* right_bases, int* count, double* used_prominence, double* peak_prob,
                           double* curv_prob, int* status);

/* ---- peak and trough probabilities of the fitted batch and the peak search on them -------------------------------------------
 * Options of DRT.predict_peak_trough_probs / predict_peak_prob / find_peaks_byprob (hybdrt/models/drt1d.py:3655-3750) over
 * surface.peak_prob / trough_prob (hybdrt/mapping/surface.py:265-350, constrain_sign=False).                                   */
typedef struct {
    int bayes_cov;         /* 1; 1: sigma of every order from the fit's own P (drt1d.py:3670-3680), 0: the windowed standard
                              deviation of the row itself (surface.py:272-291; no factorisation, no clamp, no floor)            */
    int std_size;          /* 5; odd, >= 3: window of filters.std_filter (bayes_cov = 0)                                         */
    double std_baseline;   /* 0.1; times np.std(row), added to the filtered sigma (bayes_cov = 0)                                */
    int sigma_floor;       /* 1; bayes_cov = 1: sigma[sigma < floor] = floor with floor = np.median(sigma) - 1.5 * (np.percentile(
                              sigma, 75) - np.percentile(sigma, 25)) per order (drt1d.py:3676-3679); 0: no floor                */
    int ext_left;          /* -1 = off; extend_var (drt1d.py:3123-3140): var[:ext_left] = max(var[:ext_left], var[ext_left])     */
    int ext_right;         /* -1 = off; var[ext_right:] = max(var[ext_right:], var[ext_right])                                  */
    int search;            /* 0; 0: the rows only, 1: scipy.signal.find_peaks(prob, height, prominence) (drt1d.py:3744),
                              2: peaks.find_peaks_byrange (hybdrt/peaks.py:423-441) on the index windows given                  */
    double height;         /* NaN = no height condition (upstream's None)                                                       */
    double prominence;     /* NaN = no prominence condition                                                                     */
} hipdrt_peak_prob_opts;
void hipdrt_peak_prob_opts_default(hipdrt_peak_prob_opts* o);
/* pp, tp and prob = pp (1 - tp) of every spectrum of the fitted batch on the evaluation grid ln_tau_eval[neval], on the device.
 * The rows f, fx, fxx (orders 0, 1, 2; sign 1, not normalised, as upstream's predict_drt defaults) are evaluated as
 * hipdrt_plan_predict_drt evaluates them (same kernels, same bits); with bayes_cov sigma^2 = diag(E inv(P) E') scale_b^2 of all
 * three orders comes from ONE factorisation per spectrum fed the three orders' rows, then extend_var's clamp, the root and the
 * floor.  One workgroup per spectrum then forms, with Phi = scipy.stats.norm.cdf and sgn = np.sign,
 *   pp = (1 - Phi((s_f - |f|) / s_f)) (Phi((5 s_x - fx) / s_x) - Phi((-5 s_x - fx) / s_x)) (1 - Phi(sgn(f) fxx / s_xx)),
 *   tp = (Phi((5 s_x - fx) / s_x) - Phi((-5 s_x - fx) / s_x)) (1 - Phi(-sgn(f) fxx / s_xx))
 * and runs the search (csrc/peak_prob.hip; hipdrt/models/peaks.py peak_trough_probs_rows, find_peaks_byprob_row and
 * find_peaks_byrange are its numpy statement).  row_scale[B] (may be NULL) multiplies every spectrum's coefficient scale: a
 * prepared plan runs at unit scale and its caller knows the scales (bayes_cov = 0 adds a baseline to sigma, so the scale cannot
 * be applied afterwards).  range_lo, range_hi [nranges] (search 2; nranges <= 64): index windows [lo, hi] of the grid, lo = hi + 1
 * an empty one; the peak of a window is np.argmax of prob with every sample outside it set to zero (the first maximum; index 0
 * when nothing inside is positive and the window does not start at 0).
 * out (host; any may be NULL): mu [3][B][neval] the rows f, fx, fxx (the bits of hipdrt_plan_predict_drt; NaN rows for a failed
 * fit); pp, tp, prob [B][neval]; sigma [3][B][neval] of orders 0, 1, 2 as they enter the formulas; with
 * search 1, dense on the grid as hipdrt_plan_find_peaks writes them: keep [B][neval] 0 / 1, heights, prominences [B][neval] zero
 * where there is no peak, left_bases, right_bases [B][neval] -1 where there is none, count [B] (search 0, 2: no peaks);
 * range_peaks [B][nranges] (search 2 only, else left untouched); status [B]: the fit's status, or HIPDRT_PREDICT_NOT_PD where
 * bayes_cov needs sigma and P is not positive definite (upstream fails there).  A spectrum with a negative status has count 0,
 * empty integer rows, NaN float rows and -1 range peaks.  HIPDRT_E_INVALID, before any launch: options out of range, a window
 * outside the grid, nranges > 64, a neval whose rows do not fit one workgroup's LDS (neval <= 2048 fits).  Plain and prepared
 * plans (hipdrt_plan_set_tau_basis first).  The result of a spectrum depends neither on B nor on its position in the batch.    */
int hipdrt_plan_peak_trough_probs(hipdrt_plan* plan, const double* ln_tau_eval, int neval, const hipdrt_peak_prob_opts* opts,
                                  const double* row_scale, int nranges, const int* range_lo, const int* range_hi, double* mu,
                                  double* pp, double* tp, double* prob, double* sigma, int* keep, double* heights,
                                  double* prominences, int* left_bases, int* right_bases, int* count, int* range_peaks,
                                  int* status);

/* ---- per-peak coefficients, distributions and resistances of the fitted batch ------------------------------------------------
 * Options of DRT.estimate_peak_coef / estimate_peak_drts / quantify_peaks (hybdrt/models/drt1d.py:3949-4111) over
 * peaks.find_troughs and peaks.estimate_peak_weight_distributions (hybdrt/peaks.py:92-217).                                    */
typedef struct {
    int sign;                /* 1; get_drt_params' sign of the coefficients and rows (1, or 1 / -1 / 0 for a two-copy block)      */
    int max_peaks;           /* 16; 1 .. 64: peak slots per spectrum in every output                                             */
    double epsilon_factor;   /* 1.25; eps = min(epsilon_factor / distance to the neighbouring trough in ln tau, max_epsilon)      */
    double max_epsilon;      /* 1.25                                                                                             */
    double min_epsilon;      /* NaN = none; lower bound of eps                                                                   */
    double epsilon_uniform;  /* NaN = per peak; one inverse length scale for every peak and side                                 */
} hipdrt_peak_resolve_opts;
void hipdrt_peak_resolve_opts_default(hipdrt_peak_resolve_opts* o);
/* per-spectrum statuses of hipdrt_plan_resolve_peaks: more peaks than max_peaks (count holds the true number, the rows are empty);
 * the window peaks of source 2 are not strictly increasing (two windows chose their shared border sample: upstream fails there) */
#define HIPDRT_PEAKS_OVERFLOW (-4)
#define HIPDRT_PEAKS_UNORDERED (-5)
#define HIPDRT_PEAKS_FROM_FIND 0      /* the kept peaks of find_peaks with peak_opts                                             */
#define HIPDRT_PEAKS_FROM_INDICES 1   /* peak_indices [B][max_peaks], -1 padded                                                   */
#define HIPDRT_PEAKS_FROM_WINDOWS 2   /* split_r_p(resolve_peaks=True): i + argmin(fxx[i:j]) of every window                      */
typedef struct {
    int source;                       /* HIPDRT_PEAKS_FROM_*                                                                     */
    const hipdrt_peak_opts* peak_opts;/* source 0: find_peaks' options (NULL: defaults); eval_sign must equal opts.sign           */
    const int* peak_indices;          /* source 1: [B][max_peaks] into the find grid, strictly increasing, -1 padded at the end   */
    const int *win_start, *win_end;   /* source 2: [nwin] windows [start, end) of the find grid; end may pass the grid by one     */
    int nwin;
    const double* ln_tau_find;        /* [nfind] the grid the peaks and troughs live on                                          */
    int nfind;
    const double* ln_tau_out;         /* [nout] grid of peak_gammas / r_peaks; NULL with nout = 0 when neither is asked for       */
    int nout;
    const double* row_scale;          /* [B] or NULL: multiplies every spectrum's coefficient scale (prepared plans)              */
} hipdrt_peak_resolve_in;
typedef struct {                      /* host arrays, any may be NULL (it is then never formed); padded: -1 / NaN in absent slots */
    int* count;                       /* [B] peaks of the spectrum                                                               */
    int* peak_index;                  /* [B][max_peaks]                                                                          */
    int* trough_index;                /* [B][max_peaks] count - 1 troughs                                                        */
    double *eps_l, *eps_r;            /* [B][max_peaks] inverse length scales left and right of every peak                       */
    double* r_peaks;                  /* [B][max_peaks] quantify_peaks: np.trapezoid(peak_gammas, x = ln tau_out)                 */
    double* r_coef;                   /* [B][max_peaks] predict_r_p(x = x_peak) = sqrt(pi) / eps_basis * sum_j x_peaks[i][j]      */
    double* x_peaks;                  /* [B][max_peaks][nb] estimate_peak_coef                                                   */
    double* peak_gammas;              /* [B][max_peaks][nout] estimate_peak_drts                                                 */
    int* status;                      /* [B] the fit's status, HIPDRT_PREDICT_NOT_PD (source 0, method 1), HIPDRT_PEAKS_*        */
} hipdrt_peak_resolve_out;
/* DRT.estimate_peak_coef (drt1d.py:3949-3972), estimate_peak_drts (3984-4034), quantify_peaks (4101-4111) and the resolve_peaks
 * branch of split_r_p (3610-3616) for every spectrum of the fitted batch, on the device.  The rows f (order 0) and fxx (order 2)
 * on the find grid are evaluated as hipdrt_plan_predict_drt(normalize = 0) evaluates them (same kernels, same bits); source 0
 * first runs hipdrt_plan_find_peaks' kernel on the rows with peak_opts' normalisation and takes its keep rows where they lie.
 * One workgroup per spectrum then finds the troughs (hybdrt/peaks.py:92-136), the inverse length scales (164-199), the
 * normalised weights (201-213), x_peaks = x_red * w in data units, peak_gammas = x_peaks E0' with E0 the order-0 matrix of
 * hipdrt_func_eval_matrix on the output grid, and both resistances (csrc/peak_resolve.hip; hipdrt/models/peaks.py
 * resolve_peaks_row is its numpy statement).  A basis point so far from every peak that all its weights underflow gives 0 / 0 =
 * NaN, as upstream.  HIPDRT_E_INVALID, before any launch: options out of range, a sign other than 1 on a one-copy block, indices
 * or windows out of range or not strictly increasing, a shape whose rows do not fit one workgroup's LDS (nb = 1024 with 16
 * peaks, nfind = 512 and nout = 121 fits); after the launch: a spectrum with HIPDRT_PEAKS_UNORDERED (the outputs are valid for
 * the other spectra).  Plain and prepared plans (hipdrt_plan_set_tau_basis first; unit scale times row_scale).  The result of a
 * spectrum depends neither on B nor on its position in the batch.                                                              */
int hipdrt_plan_resolve_peaks(hipdrt_plan* plan, const hipdrt_peak_resolve_in* in, const hipdrt_peak_resolve_opts* opts,
                              hipdrt_peak_resolve_out* out);
/* DRT.integrate_drt (drt1d.py:3590-3594) and split_r_p without resolve_peaks (3596-3620): out[b][k] = np.trapezoid of
 * predict_drt's row (order, sign, normalize as hipdrt_plan_predict_drt; row_scale [B] or NULL, normalize = 0 only) over the
 * windows [win_start[k], win_end[k]) of ln_tau_eval[neval]; an end may pass the grid by one (numpy clips the slice).
 * out [B][nwin]; status [B] (may be NULL) the fit's status, rows of failed fits are NaN.                                        */
int hipdrt_plan_integrate_drt(hipdrt_plan* plan, const double* ln_tau_eval, int neval, int order, int sign, int normalize,
                              const double* row_scale, const int* win_start, const int* win_end, int nwin, double* out,
                              int* status);

/* ---- the probability function of relaxation times (PFRT) of a PFRT fit ----------------------------------------------------------
 * DRT.pfrt_fit_eis (hybdrt/models/drt1d.py:2558-2698) is a fit at the first regularisation factor followed by one warm restart
 * per further factor; DRT.predict_pfrt (2716-2858) turns the S solutions into the PFRT.  The plan keeps what that needs in a step
 * store: hipdrt_plan_pfrt_begin sizes it for max_steps steps of the plan's capacity (x, s, rho [, dop_rho], the two likelihood sums
 * and the status of every spectrum: hipdrt_plan_pfrt_bytes_per_spectrum bytes each) and empties it; hipdrt_plan_pfrt_record, called
 * after hipdrt_plan_fit and after every hipdrt_plan_continue, appends the state that call left (device-to-device copies) and the
 * sums of hipdrt_plan_llh_terms; hipdrt_plan_pfrt_steps gives the count.  Staging a new batch empties the store.  Plain and
 * prepared plans.  A failed allocation is HIPDRT_E_HIP and leaves the plan usable with an empty store.                          */
int hipdrt_plan_pfrt_bytes_per_spectrum(int n, int steps, long long* bytes);
int hipdrt_plan_pfrt_begin(hipdrt_plan* plan, int max_steps);
int hipdrt_plan_pfrt_record(hipdrt_plan* plan);
int hipdrt_plan_pfrt_steps(hipdrt_plan* plan, int* steps);
/* the live s vectors of every staged spectrum become factor times the s vectors step `step` recorded (on the device): the start
 * of DRT._generate_candidates_s0's restarts, "the baseline s vectors scaled by multiplier^i" (drt1d.py:1534-1537), when the
 * baseline is a recorded step and nothing is to cross to the host                                                               */
int hipdrt_plan_pfrt_restore_s(hipdrt_plan* plan, int step, double factor);
/* what step `step` recorded, for the staged spectra: x [B][n], rho [B][3], s [B][3][n], rss [B], sum_log_w [B], status [B]; any
 * may be NULL                                                                                                                  */
int hipdrt_plan_pfrt_get_step(hipdrt_plan* plan, int step, double* x, double* rho, double* s, double* rss, double* sum_log_w,
                              int* status);
/* pfrt_result['step_p_mat'][step] of spectrum b, p[n][n]: calculate_pq with the step's final s / rho and the RAW weights
 * estimate_weights(x, rv, vmm, rm) of the step's x (drt1d.py:2611-2632) -- not hipdrt_plan_get_p_matrix's matrix, which carries
 * the loop's blended weights times the weight factors, and only for the last state.  Also what DRTMD reads per factor
 * (hybdrt/mapping/drtmd.py:934-941).  Plain and prepared plans.                                                                */
int hipdrt_plan_get_step_p_matrix(hipdrt_plan* plan, int step, int b, double* p);
typedef struct {
    int eval_sign;              /* 1; get_drt_params' sign of the evaluated rows (a plain EIS plan takes 1 only)                 */
    int search;                 /* 1; as hipdrt_peak_opts.search: sign if nonneg and sign != 0, else 0 (two passes)              */
    double height;              /* 1e-3; find_peaks_kw                                                                          */
    double prominence;          /* 5e-3                                                                                         */
    double prior_mu;            /* -4; log-normal prior on ln(factor)                                                           */
    double prior_sigma;         /* 0.5                                                                                          */
    double n_eff_factor;        /* 0.5; exponent on the normalised posterior                                                    */
    double fxx_var_floor;       /* 1e-5; lower bound of BOTH variances (upstream hands it to both estimate_distribution_cov calls) */
    int ext_left;               /* -1 = off; extend_var's clamp indices on the tau_pfrt grid, as hipdrt_peak_opts                */
    int ext_right;
    int smooth;                 /* 1; multiply by exp(-(epsilon |ln tau_out - ln tau_pfrt|)^(2 order))                           */
    double smooth_order;        /* 2                                                                                            */
    double smooth_epsilon;      /* 5                                                                                            */
    int integrate;              /* 0; pfrt.integrate_peaks: every contiguous range >= integrate_threshold becomes its trapezoid
                                   area (one sample beyond either end included) at the range's maximum; a range that starts at
                                   index 0 gets 0, as upstream's empty slice does                                               */
    double integrate_threshold; /* 1e-6                                                                                         */
    int normalize;              /* 1; divide by the row's maximum (an all-zero row becomes NaN, as upstream)                     */
} hipdrt_pfrt_opts;
void hipdrt_pfrt_opts_default(hipdrt_pfrt_opts* o);
/* DRT.predict_pfrt for every spectrum of the fitted batch over the S recorded steps, on the device.  factors [S] (S must be the
 * recorded step count); ln_tau_pfrt [neval_pfrt] the peak-finding grid; ln_tau_out [neval_out] the grid of the smoothed result
 * (without smooth: neval_out == neval_pfrt and ln_tau_out is not read).  Per step: the step P of the whole batch, one
 * factorisation per spectrum fed the order-2 and order-0 evaluation rows, f and fxx normalised by the R_p of the step's own x,
 * both variances divided by the squared R_p of the FIRST step (as upstream, whose estimate_distribution_cov normalises by
 * fit_parameters), extend_var's clamp and the floor, scipy's peak rule (peaks_kernel, method 0), and at every peak
 * min(1 - erfc(|f| / (sigma_f sqrt 2)), 1 - erfc(min(prominence, height) / (sigma_fxx sqrt 2))).  Then once: posterior weights of
 * the steps from the recorded likelihood sums and the prior, the weighted sum, smoothing, integration, normalisation.
 * out (host; any may be NULL): pfrt [B][neval_out], raw_pfrt [B][neval_pfrt], step_pfrt [S][B][neval_pfrt], post_prob [S][B],
 * status [B]: the fit's status (negative when any step failed), or HIPDRT_PREDICT_NOT_PD when a step P is not positive definite;
 * the rows of such a spectrum are NaN.  HIPDRT_E_INVALID before any launch: no recorded steps, options out of range, more than
 * 2048 points on either grid.  HIPDRT_E_UNSUPPORTED for a prepared plan.  Callable repeatedly after one fit.  The result of a
 * spectrum depends neither on B nor on its position.                                                                            */
int hipdrt_plan_predict_pfrt(hipdrt_plan* plan, const double* factors, const double* ln_tau_pfrt, int neval_pfrt,
                             const double* ln_tau_out, int neval_out, const hipdrt_pfrt_opts* opts, double* pfrt, double* raw_pfrt,
                             double* step_pfrt, double* post_prob, int* status);

/* DRT.select_pfrt_candidates (hybdrt/models/drt1d.py:2860-2865 over hybdrt/models/pfrt.py:164-213) for every spectrum of the
 * fitted batch, on the device: the chain of hipdrt_plan_predict_pfrt up to raw_pfrt (opts as there; upstream selects on the raw
 * PFRT, so its smooth, integrate and normalize fields act on the optional finished row `pfrt` alone), then per spectrum the
 * contiguous ranges of raw_pfrt >= peak_thresh, their peaks ranked by integrated area (equal areas: the higher index first),
 * every step's row shifted onto those peaks (an entry at ti moves to the peak of the range with start <= ti <= end, end being
 * the exclusive end; of several entries that land on one peak the one from the highest index stays), and for each growing set
 * of best peaks the step with the largest corrcoef(target, shifted row) * step likelihood, by np.argmax's rule (the first
 * maximum; the first NaN, which an all-zero row gives, beats everything).  The first target holds the peaks whose magnitude
 * (area / largest area) reaches start_thresh (at least one); targets grow by one peak until the next magnitude is below
 * end_thresh; the full set is never a target, so K peaks give at most K - 1 candidates.
 * out (host; any may be NULL), the compact form: num_peaks [B] = K; ranked_index, magnitude [B][max_peaks]; first [B], the
 * prefix length minus one of the first target; num_candidates [B]; step_index, match_quality [B][max_peaks] -- candidate j has
 * target ranked_index[0 .. first + j] and step step_index[j], match_quality[j] is the winning value.  Unused slots hold -1 and
 * NaN.  raw_pfrt, step_pfrt, post_prob: as hipdrt_plan_predict_pfrt.  pfrt [B][neval_out]: the finished PFRT of the same pass,
 * the bits hipdrt_plan_predict_pfrt gives for the same opts and grids (sel->ln_tau_out, sel->neval_out; without smooth
 * neval_out == neval_pfrt and the grid is not read); it costs one more launch of the combination, no second pass over the steps.
 * status [B]: the fit's or the variance path's status as in hipdrt_plan_predict_pfrt.  A negative one leaves every slot unused
 * and the three counts -1; 0 and 1, a step that ended at its iteration limit, are live fits.  A live fit has
 * HIPDRT_PFRT_NO_PEAK for a row with nothing at or above peak_thresh (num_peaks 0, upstream raises there) and
 * HIPDRT_PFRT_TOO_MANY_PEAKS for more ranges than max_peaks (num_peaks holds their number, nothing is ranked).
 * HIPDRT_E_INVALID before any launch: as hipdrt_plan_predict_pfrt (the smoothing options and the output grid only when pfrt is
 * asked for), max_peaks outside 1 ... 64, a threshold that is NaN.  HIPDRT_E_UNSUPPORTED for a prepared plan.  The result of a
 * spectrum depends neither on B nor on its position.                                                                            */
#define HIPDRT_PFRT_NO_PEAK 16
#define HIPDRT_PFRT_TOO_MANY_PEAKS 17
typedef struct {
    double start_thresh;        /* 0.99                                                                                        */
    double end_thresh;          /* 0.01                                                                                        */
    double peak_thresh;         /* 1e-6                                                                                        */
    int max_peaks;              /* 16; 1 ... 64                                                                                 */
    const double* ln_tau_out;   /* NULL; [neval_out] the grid of out->pfrt (read with out->pfrt and opts->smooth only)          */
    int neval_out;              /* 0; points of out->pfrt                                                                       */
} hipdrt_pfrt_select_opts;
void hipdrt_pfrt_select_opts_default(hipdrt_pfrt_select_opts* o);
typedef struct {
    int* num_peaks;             /* [B]                                                                                          */
    int* ranked_index;          /* [B][max_peaks]                                                                               */
    int* first;                 /* [B]                                                                                          */
    int* num_candidates;        /* [B]                                                                                          */
    int* step_index;            /* [B][max_peaks]                                                                               */
    double* magnitude;          /* [B][max_peaks]                                                                               */
    double* match_quality;      /* [B][max_peaks]                                                                               */
    double* raw_pfrt;           /* [B][neval_pfrt]                                                                              */
    double* step_pfrt;          /* [S][B][neval_pfrt]                                                                           */
    double* post_prob;          /* [S][B]                                                                                       */
    double* pfrt;               /* [B][sel->neval_out]                                                                          */
} hipdrt_pfrt_select_out;
int hipdrt_plan_pfrt_select(hipdrt_plan* plan, const double* factors, const double* ln_tau_pfrt, int neval_pfrt,
                            const hipdrt_pfrt_opts* opts, const hipdrt_pfrt_select_opts* sel, hipdrt_pfrt_select_out* out,
                            int* status);

/* ---- candidate models of the fitted batch, scored on the device -----------------------------------------------------------------
 * What DRT.generate_candidates (hybdrt/models/drt1d.py:1632-1821) computes per candidate before it ranks them (1690-1729): the
 * log-likelihood under weights re-estimated from the candidate alone (evaluate_llh(weights=None, x=x), 4457-4496 over
 * qphb.py:1347-1377) and the peaks of find_peaks(x=x) (3753-3947 over predict_drt(x=x, normalize=True), 3020-3061) -- for C
 * candidates of every spectrum in one call.  The ranking itself (BIC, best per number of peaks, filling, Bayes factors) is host
 * arithmetic on these outputs: hipdrt/models/candidates.py.                                                                      */
#define HIPDRT_CANDIDATES_FROM_STEPS 0   /* every recorded step of the plan's step store (hipdrt_plan_pfrt_begin / _record)      */
#define HIPDRT_CANDIDATES_FROM_HOST 1    /* x [C][B][n] in scaled units, uploaded by the call                                    */
#define HIPDRT_CANDIDATE_ABSENT (-6)     /* status of a slot at or past the spectrum's ncand                                     */
typedef struct {
    int source;                       /* HIPDRT_CANDIDATES_FROM_*                                                                */
    int C;                            /* FROM_HOST: candidates per spectrum; FROM_STEPS: 0, or the recorded step count            */
    const double* x;                  /* FROM_HOST: [C][B][n], the unknown vectors as the fit holds them (scaled units)           */
    const int* ncand;                 /* [B] candidates of each spectrum, 0 .. C; NULL: all C                                     */
    const double* ln_tau_find;        /* [nfind] the grid peaks are found on; NULL with nfind = 0: no peak search                 */
    int nfind;
    const hipdrt_peak_opts* peak_opts;/* NULL: defaults; method must be 0 ('thresh': 'prob' needs a P matrix per candidate)       */
    int max_peaks;                    /* 0 = 16; 1 .. 64 peak slots per candidate                                                 */
} hipdrt_candidates_in;
typedef struct {                      /* host arrays, any may be NULL; [C][B] leading                                            */
    double *rss, *sum_log_w;          /* [C][B] the sums of hipdrt_plan_llh_terms for the candidate's x                           */
    int* count;                       /* [C][B] peaks of the candidate (the true number even beyond max_peaks)                    */
    int* peak_index;                  /* [C][B][max_peaks] positions on the find grid, ascending, -1 padded                       */
    double *heights, *prominences;    /* [C][B][max_peaks] of those peaks, NaN padded                                            */
    int* status;                      /* [C][B] the fit's (FROM_STEPS: the step's) status, HIPDRT_CANDIDATE_ABSENT, HIPDRT_PEAKS_OVERFLOW */
} hipdrt_candidates_out;
/* Likelihood sums (csrc/candidates.hip): r = rm_b x - rv_b, s = vmm r^2 floored at the spectrum's variance floor, w = max(s^-1/2,
 * 1e-10), rss = |w r|^2 expanded as hipdrt_plan_llh_terms expands it, sum_log_w = sum log w.  A spectrum's candidates are taken 16
 * at a time on the FP64 matrix pipe, so rm and vmm are read once per 16 candidates rather than once per candidate; where 16 rows of
 * m do not fit in LDS (m > 896) rm x passes through a scratch buffer of C B m doubles, with the same bits.  Peaks: per candidate
 * the curvature row (and f where the options need it) of the candidate's x on the find grid, normalised by the R_p of that x, by
 * the kernels of hipdrt_plan_find_peaks; then that entry's peak rule (method 0) and a compaction of its dense rows.
 * A failed fit gives NaN / -1 in every slot of the spectrum and its negative status; so does a slot at or past ncand[b], with
 * HIPDRT_CANDIDATE_ABSENT, and (FROM_STEPS) a step whose recorded status is negative for the spectrum, with that status, whatever
 * later steps did.  The status of a valid slot is the live fit's (FROM_HOST) or the one recorded with the step (FROM_STEPS).  More than max_peaks peaks: the true count, HIPDRT_PEAKS_OVERFLOW and empty rows.  HIPDRT_E_INVALID
 * before any launch: no fitted batch, no recorded steps (FROM_STEPS), C out of range, ncand out of range, options out of range,
 * method other than 0, a find grid whose rows do not fit one workgroup's LDS.  The call reads the plan's matrices, data and
 * statuses and writes nothing the fit or a later call reads.  Plain and prepared plans (hipdrt_plan_set_tau_basis first for
 * peaks).  The result of a candidate depends neither on C or B nor on its position among the candidates or in the batch.         */
int hipdrt_plan_score_candidates(hipdrt_plan* plan, const hipdrt_candidates_in* in, hipdrt_candidates_out* out);

/* ---- log marginal likelihood (evidence) of the fitted batch -----------------------------------------------------------------------
 * The ingredients of DRT.evaluate_lml (hybdrt/models/drt1d.py:4513-4543 over qphb.evaluate_lml, hybdrt/models/qphb.py:1279-1344)
 * for every spectrum of the fitted batch.  With Omega = calculate_qp_l2_matrix(...) (qphb.py:53-120, special diagonal included),
 * P = Omega + (W rm)'(W rm) (calculate_pq, qphb.py:1154-1183), y = rv and r = rm x:
 *     logdet_p = ln det P, logdet_prior = ln det Omega, wy2 = |W y|^2, fit2 = |W r|^2, cross = sum w^2 r y, slw = sum ln w,
 *     xox = x' Omega x, l1x = l1' x
 * from which upstream's last lines follow on the host (hipdrt/models/lml.py: lml_from_terms):
 *     beta = 0.5 (wy2 - fit2 - xox) + beta_0,  alpha = m / 2 + alpha_0,
 *     lml  = 0.5 (logdet_prior - logdet_p) + slw + lgamma(alpha) - lgamma(alpha_0) + alpha_0 ln beta_0 - alpha ln beta
 * (cross and l1x are not in the LML: wy2 - 2 cross + fit2 is the residual sum of squares, and with xox they give x'Px and q'x).
 * State: the live fit (step < 0, no arrays), recorded step `step` of the step store (hipdrt_plan_pfrt_begin / _record), or the
 * uploaded arrays x, rho, s (and dop_rho exactly when the plan has a DOP block).  Weights: NULL = the fit's own est_weights, which
 * is upstream's default -- never the scaled weights the fit's last P was formed with, nor the row factors of a KK pass.
 * A determinant is 2 sum ln L_ii of the Cholesky factor (csrc/qp_resident.hpp: logdet_kernel_resident); P's packed image is formed,
 * reduced, and Omega's image then formed in the same place.                                                                          */
typedef struct {
    int step;                         /* >= 0: that recorded step's x, rho, s, dop_rho; -1: the live fit or the arrays below          */
    const double* x;                  /* [B][n] scaled unknowns; x, rho and s come together or not at all                             */
    const double* rho;                /* [B][3]                                                                                       */
    const double* s;                  /* [B][3][n]                                                                                    */
    const double* dop_rho;            /* [B][3]; with the arrays above, required exactly when the plan has a DOP block                */
    const double* weights;            /* [B][m], every entry > 0; NULL: the plan's est_weights                                        */
    int override_hypers;              /* 0: the plan's own hyper-parameters; 1: the four below (update_hypers)                        */
    double l2_lambda_0;
    double derivative_weights[3];     /* a weight of 0 skips that order                                                               */
    double dop_l2_lambda_0;           /* read only when the plan has a DOP block, as the next                                         */
    double dop_derivative_weights[3];
} hipdrt_lml_in;
typedef struct {                      /* host arrays [B], any may be NULL                                                             */
    double *logdet_p, *logdet_prior;  /* NaN where that factorisation failed                                                          */
    double *wy2, *fit2, *cross, *slw, *xox, *l1x;
    int* status;                      /* the fit's (a recorded step: the step's) status where negative: every row of that member is
                                         NaN; else HIPDRT_PREDICT_NOT_PD where either matrix is not positive definite; else that status */
} hipdrt_lml_out;
/* step -1, no arrays, no override; the hyper fields hold get_default_hypers' values (qphb.py:208-255)                                */
void hipdrt_default_lml_in(hipdrt_lml_in* in);
/* in NULL: the defaults.  HIPDRT_E_INVALID before any launch: no fitted batch, n > 4096, a step outside the store, a step together
 * with arrays, arrays without x, rho or s, dop_rho missing or superfluous, a weight that is not positive and finite, an override that
 * is not finite, m and n beyond one workgroup's LDS.  The last device batch only.  The call rebuilds the packed image of P, which
 * every outer iteration of a fit rebuilds too, and writes nothing else that the fit or a later call reads.  Plain and prepared
 * plans; a vz_offset column is taken as the fit left it.  A spectrum's result depends neither on B nor on its position.              */
int hipdrt_plan_lml_terms(hipdrt_plan* plan, const hipdrt_lml_in* in, hipdrt_lml_out* out);

/* ---- coherent re-optimisation of neighbouring observations, assembled on the device --------------------------------------------------
 * DRTMD.resolve_observations / resolve_group (hybdrt/mapping/drtmd.py:432-559) over resolve.resolve_observations
 * (hybdrt/mapping/resolve.py:176-341) for the members of a fitted PREPARED batch: every coupled batch k takes the nr consecutive
 * members first[k] .. first[k] + nr - 1; their final P (what hipdrt_plan_get_p_matrix returns) and q never leave the device.  With
 * nc_k = so + match[k][1] - match[k][0] unknowns per member, P_k (nr nc_k square) and q_k are written in the form the coneqp
 * launchers read (lower 16 x 16 tiles):
 *     block (i, i)   member i's P without its leading num_remove data-dependent unknowns (v_baseline, vz_offset; get_offset_pq,
 *                    resolve.py:11-64), its tau range tau_indices[b] moved into match[k] (resize_pq's four cases, resolve.py:67-134;
 *                    zero where the member has no basis function), plus param_scale[c] * my[i][i] * lambda_psi on the diagonal;
 *     block (i, j)   the diagonal matrix param_scale[c] * my[i][j] * lambda_psi;
 *     q_k block i    q_trim + x_remove_i @ P_i[:num_remove, num_remove:], resized alike.
 * Products and the single add round as numpy's (no fused multiply-add); q's short sum runs in index order.  All batches of one size
 * are then solved in one coneqp launch, with the kernel choice and default options of hipdrt_qp_batch for that many problems of that
 * size.                                                                                                                              */
typedef struct {
    int nb, nr;                       /* coupled batches; members of every batch (>= 1)                                               */
    int num_remove, so;               /* leading unknowns dropped from every member; special unknowns kept behind them                */
    double lambda_psi;
    double tau_filter_sigma, special_filter_sigma;   /* > 0 makes P dense across blocks: HIPDRT_E_UNSUPPORTED                         */
    const int* first;                 /* [nb] first member of batch k                                                                 */
    const int* match;                 /* [nb][2] the batch's common tau range (left, right) on the supergrid                          */
    const int* tau_indices;           /* [B][2] every member's own range; right - left = n - num_remove - so                          */
    const double* my;                 /* [nb][nr][nr] coupling across the members of a batch (exactly symmetric)                      */
    const double* param_scale;        /* nc_k entries for batch k, batch after batch                                                  */
    const double* x_remove;           /* [B][num_remove] fitted values of the dropped unknowns; NULL with num_remove = 0              */
    const double* h;                  /* nr * nc_k entries for batch k, batch after batch (the QP's bound; read by the solve only)    */
} hipdrt_resolve_args;
/* x_out: batch k's nr * nc_k unknowns, batch after batch; iters_out (may be NULL) and status_out [nb]: as hipdrt_qp_batch returns them.
 * HIPDRT_E_INVALID before any launch: a plan that is not prepared or holds no fitted batch, a member outside the batch, a range that
 * is empty or does not match n, nr * nc_k > 4096, nb > 65535.  HIPDRT_E_UNSUPPORTED for either filter sigma > 0 (the caller assembles
 * those on the host and uses hipdrt_qp_batch).  Reads the fitted state only: the plan can be fitted, read or resolved again.          */
int hipdrt_plan_resolve_group(hipdrt_plan* plan, const hipdrt_resolve_args* args, double* x_out, int* iters_out, int* status_out);

/* kernel-time breakdown of the last hipdrt_plan_fit in ms (HIP events on the ctx stream):
 * t[0]=total, t[1]=gram, t[2]=qp, t[3]=hyper, t[4]=setup/other; launches[5] same order                 */
int hipdrt_plan_timings(hipdrt_plan* plan, float* t, int* launches);

/* one-shot convenience: create plan, upload, fit, download, destroy */
int hipdrt_fit_eis_batch(hipdrt_ctx* ctx, int B, const double* freq, int nf, const double* z_re,
                         const double* z_im, const double* tau, int ntau, double epsilon, int mode,
                         int toeplitz_a, int toeplitz_m, int ngrid, int ny, const double* wt_re,
                         const double* wt_im, const double* log_wt_re, const double* log_wt_im,
                         const hipdrt_fit_opts* opts, double* x, double* fit_x,
                         double* r_inf, double* induc, double* weights, double* coef_scale, double* rho,
                         double* q_vector, int* outer_iters, int* status);

/* ---- one map over the GPUs of a node: RCCL behind the C ABI -------------------------------------------------------------
 * The reference fits the observations of a map one after the other in ONE process (DRTMD.fit_observations,
 * hybdrt/mapping/drtmd.py:303-319); they share only the lookup tables, the tau supergrid and cached matrices (245-301).  Here a
 * map is sharded over one process per GPU; the two exchanges that needs are a broadcast of rank 0's lookup tables and ONE gather
 * of the per-observation result rows.  librccl.so is loaded on first use.  Rendezvous: rank 0 calls hipdrt_comm_unique_id and
 * gets its 128 bytes to the other ranks by any out-of-band channel (hybrid-drt_amd/mapping/dist.py: a file next to
 * MASTER_PORT); every rank then calls hipdrt_comm_create with the same bytes (collective: returns when all `world` ranks did). */
#define HIPDRT_COMM_ID_BYTES 128
int hipdrt_comm_unique_id(char* id128);
int hipdrt_comm_create(int device, int rank, int world, const char* id128, hipdrt_comm** out);
int hipdrt_comm_destroy(hipdrt_comm* comm);
int hipdrt_comm_info(hipdrt_comm* comm, int* rank, int* world, int* device);
/* device buffers in, device buffers out.  broadcast: `count` doubles of `root` to everyone, in place.  gather: every rank
 * sends `count` doubles, `root` receives world x count (rank r's block at r * count; dev_recv may be NULL elsewhere) -- a
 * true gather, one ncclSend per rank and `world` ncclRecv on the root inside one group.  Both return when the data is there. */
int hipdrt_comm_broadcast_dev(hipdrt_comm* comm, double* dev_buf, long long count, int root);
int hipdrt_comm_gather_dev(hipdrt_comm* comm, const double* dev_send, long long count, double* dev_recv, int root);
/* the same for host arrays (numpy in, numpy out), staged through the communicator's own device buffers */
int hipdrt_comm_broadcast(hipdrt_comm* comm, double* host_buf, long long count, int root);
int hipdrt_comm_gather(hipdrt_comm* comm, const double* host_send, long long count, double* host_recv, int root);
/* max over the ranks of *value, in every rank (a benchmark's "slowest rank" time); value == NULL: a plain barrier */
int hipdrt_comm_allreduce_max(hipdrt_comm* comm, double* value);
int hipdrt_comm_barrier(hipdrt_comm* comm);
/* device memory for callers that keep matrices resident (hipdrt_impedance_matrix_dev and the *_dev collectives take it) */
int hipdrt_device_alloc(hipdrt_ctx* ctx, long long bytes, void** out);
int hipdrt_device_free(hipdrt_ctx* ctx, void* ptr);
/* hipDeviceSynchronize on the context's device: every stream drained (a benchmark brackets its timed region with it)       */
int hipdrt_device_synchronize(hipdrt_ctx* ctx);
/* 0 when device `device` exists and is a gfx950 part (HIPDRT_E_NODEVICE otherwise); creates nothing on the device                */
int hipdrt_device_probe(int device);

#ifdef __cplusplus
}
#endif
#endif /* HIPDRT_H */
