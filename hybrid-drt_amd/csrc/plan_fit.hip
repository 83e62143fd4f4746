// The device fit loop of a plan (include/hipdrt.h): DRT._qphb_fit_core (hybdrt/models/drt1d.py:102-1104, EIS branch) for the
// staged batch, its side-by-side ranges, warm restarts and the single iterate_qphb pass.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <functional>
#include <thread>

#include "plan.hpp"

namespace hipdrt {
// L2 part of P in hyper-parameter form (calculate_qp_l2_matrix, qphb.py:53-120) for the plan's current state
GramL2 plan_l2(const hipdrt_plan* p, double l2_lambda_0, const double* derivative_weights, double dop_l2_lambda_0,
               const double* dop_derivative_weights) {
    GramL2 g{};
    g.l2 = nullptr; g.ldm = p->ldm; g.ns = p->ns; g.use_rho = 1;
    g.sym = p->prepared ? 0 : p->toeplitz_m;      // caller-supplied matrices are not assumed bitwise symmetric
    g.toep = p->toeplitz_m;                       // log-uniform tau grid (the hyper kernel relies on the same structure)
    g.toep_maxd = (p->toeplitz_m && !(p->ctx && !p->ctx->zero_shortcuts)) ? p->toep_maxd : -1;
    g.spec_zero = p->spec_zero;
    for (int k = 0; k < 3; ++k) { g.mk[k] = p->mk[k].d(); g.dfac[k] = l2_lambda_0 * derivative_weights[k]; }
    g.s = p->s.d(); g.rho = p->rho.d();
    if (p->prepared && p->desc.dop_size > 0) {
        g.dop_start = p->desc.dop_start; g.dop_size = p->desc.dop_size; g.dop_rho = p->dop_rho.d();
        const double* ddw = dop_derivative_weights ? dop_derivative_weights : p->desc.dop_derivative_weights;
        for (int k = 0; k < 3; ++k) g.dop_dfac[k] = dop_l2_lambda_0 * ddw[k];
    }
    return g;
}
}  // namespace hipdrt

extern "C" {

// hyper-parameter step of one outer iteration.  Few fits with large matrices: their matrix-vector products are spread over
// many workgroups first (premv_kernel), else the one workgroup per fit of hyper_kernel would stream them through one CU each.
static int plan_hyper(hipdrt_plan* p, hipStream_t st, const FitState& fs_in, int B, int it) {
    FitState fs = fs_in;
    const size_t premv_need = 3 * (size_t)(p->capacity > B ? p->capacity : B) * p->m * sizeof(double);
    // (the options of THIS loop decide -- a warm restart may switch outlier_p on or off against the plan's fit)
    const bool outl = fs_in.opts.outlier_p > 0.0;
    const bool spread = B * 8 <= device_cus() && (size_t)p->m * p->n >= ((size_t)1 << 20) && !outl;
    // one response matrix and one variance matrix for the whole batch (every EIS plan, prepared plans without a vz_offset
    // column): rm @ x and vmm @ resid^2 of all spectra as two batched products (hyper.hip: batch_products_kernel) -- for any
    // batch size, so that a spectrum's bits do not depend on whether it is fitted alone or among a thousand
    const bool batched = !spread && p->rm_stride == 0 && !outl && !(p->prepared && p->desc.vz_index >= 0);
    if (spread || batched) {
        if (p->premv.bytes < premv_need) HIPDRT_CHECK(p->premv.alloc(premv_need));     // (a sub-batch view: a window of the parent's)
        fs.premv = p->premv.d();
        fs.premv_batched = batched;
    }
    return launch_hyper(st, fs, B, it);
}

namespace {
struct PhaseTimer {
    hipStream_t st;
    std::vector<hipEvent_t> ev;
    std::vector<int> cat;
    explicit PhaseTimer(hipStream_t s) : st(s) {}
    ~PhaseTimer() { for (auto e : ev) (void)hipEventDestroy(e); }
    void mark(int category) {   // closes the previous phase, opens `category` (-1 = end)
        hipEvent_t e;
        if (hipEventCreate(&e) != hipSuccess) return;
        (void)hipEventRecord(e, st);
        ev.push_back(e);
        cat.push_back(category);
    }
    void collect(float* t_ms, int* launches) {
        for (int i = 0; i < 5; ++i) { t_ms[i] = 0; launches[i] = 0; }
        for (size_t i = 0; i + 1 < ev.size(); ++i) {
            float ms = 0;
            if (hipEventElapsedTime(&ms, ev[i], ev[i + 1]) == hipSuccess && cat[i] >= 1 && cat[i] <= 4) {
                t_ms[cat[i]] += ms; launches[cat[i]] += 1;
            }
        }
        if (ev.size() >= 2) { float ms = 0; (void)hipEventElapsedTime(&ms, ev.front(), ev.back()); t_ms[0] = ms; launches[0] = 1; }
    }
};
}  // namespace

// QP arguments of the loop, all but P and the active mask (pq_qp_step takes those from the normal equations it forms): the
// plan's solution, scratch and counters, the loop's constraint vector
static QpArgs loop_qp_args(hipdrt_plan* p, const hipdrt_qp_opts& qpo) {
    const int n = p->n;
    QpArgs qa{};
    qa.B = p->B; qa.n = n; qa.q = p->q.d(); qa.h = p->h.d(); qa.h_stride = 0;
    qa.L = p->L.d(); qa.ldl = p->ldl;
    p->qp_layout(p->B, qa);
    qa.x = p->x.d(); qa.iters = p->qp_iters.i(); qa.pcost = p->pcost.d(); qa.status = p->qp_status.i();
    qa.iters_accum = p->qp_iters_total.i(); qa.opts = qpo;
    qa.state = p->qpstate.d(); qa.state_ld = qp_state_ld(n); qa.state_stride = (long long)qp_state_doubles(n);
    return qa;
}

// The step every QP of the fit consists of: P and q of the normal equations `pq` (phase 1, opened by the caller), then the QP
// `qa` on them (phase 2; workgroups dispatched longest first when an `order` buffer is given); the phase of what follows (3) is
// opened on return.  `one_p`: every problem has the same P (a shared response matrix, weights and hyper-parameters that do not
// differ between the spectra) -- it is formed once and every QP reads that copy.
static int pq_qp_step(hipStream_t st, PhaseTimer& tm, const PqArgs& pq, const GramL2& g, QpArgs qa, bool one_p,
                      int* order = nullptr) {
    PqArgs gp = pq;
    if (one_p) { gp.B = 1; gp.p_stride = gp.ppk_stride = 0; }
    launch_gram_l2(st, gp, g);
    launch_qvec(st, pq);
    LAUNCH_OK();
    tm.mark(2);
    // the QP reads P where and as the Gram launch has written it, and leaves out the spectra that launch left out
    qa.P = gp.P; qa.ldp = gp.ldp; qa.p_stride = gp.p_stride;
    qa.Ppk = gp.Ppk; qa.ppk_stride = gp.ppk_stride; qa.nchp = gp.Ppk ? qp_nchp(gp.n) : 0;
    qa.active = pq.active;
    if (order && pq.B * sizeof(int) <= 48 * 1024) {     // dispatch order from the previous QP's iteration counts
        launch_lpt_order(st, pq.B, qa.iters, qa.active, order);
        qa.order = order;
    }
    TRY(launch_qp(st, qa));
    tm.mark(3);
    return HIPDRT_OK;
}

// One outer iteration of the staged batch on the weights `wq` the QP sees: pq_qp_step on the plan's own operands, one P per
// spectrum, then the hyper-parameter step (phase 3)
static int outer_iteration(hipdrt_plan* p, hipStream_t st, PhaseTimer& tm, const FitState& fs, const GramL2& g, const QpArgs& qa,
                           const double* wq, int* order, int it) {
    TRY(pq_qp_step(st, tm, p->pq(wq), g, qa, false, order));
    TRY(plan_hyper(p, st, fs, p->B, it));
    LAUNCH_OK();
    return HIPDRT_OK;
}

// The outer loop (drt1d.py:877-988) with the options of `fs`: until no spectrum is active, at most max_iter iterations.
// `weights(it)` applies the caller's weight scaling of iteration `it` and returns the weights the QP sees.
static int outer_loop(hipdrt_plan* p, hipStream_t st, PhaseTimer& tm, const FitState& fs,
                      const std::function<const double*(int)>& weights) {
    const GramL2 g = plan_l2(p, fs.opts.l2_lambda_0, fs.opts.derivative_weights, p->prepared ? p->desc.dop_l2_lambda_0 : 0.0);
    const QpArgs qa = loop_qp_args(p, fs.opts.qp);
    for (int it = 0; it < fs.opts.max_iter; ++it) {
        tm.mark(1);
        HIPDRT_CHECK(hipMemsetAsync(p->n_active.p, 0, sizeof(int), st));
        TRY(outer_iteration(p, st, tm, fs, g, qa, weights(it), p->order.i(), it));
        int n_active = 0;
        HIPDRT_CHECK(hipMemcpyAsync(&n_active, p->n_active.p, sizeof(int), hipMemcpyDeviceToHost, st));
        HIPDRT_CHECK(hipStreamSynchronize(st));
        if (n_active == 0) break;
    }
    return HIPDRT_OK;
}

// calculate_pq's q with the final weights `wfin` (qphb.py:1154-1183), then the phase record of the call
static int outer_finish(hipdrt_plan* p, hipStream_t st, PhaseTimer& tm, const double* wfin) {
    PqArgs pq = p->pq(wfin);
    pq.active = nullptr;       // every spectrum, stopped or not
    launch_qvec(st, pq);
    LAUNCH_OK();
    tm.mark(-1);
    HIPDRT_CHECK(hipStreamSynchronize(st));
    tm.collect(p->t_ms, p->launches);
    return HIPDRT_OK;
}

// the whole fit of the plan's staged spectra on the plan's stream (hipdrt_plan_fit; also run per sub-batch view)
static int plan_fit_one(hipdrt_plan* p) {
    HIPDRT_REQUIRE(p, "plan is NULL");
    HIPDRT_REQUIRE(p->B >= 1, "no spectra staged (call hipdrt_plan_upload)");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const int B = p->B, m = p->m;
    FitState fs = p->state();
    PhaseTimer tm(st);
    tm.mark(4);
    if (p->hist_b >= 0) HIPDRT_CHECK(hipMemsetAsync(p->hist_rows.p, 0, sizeof(int), st));
    launch_prep(st, fs, B);
    LAUNCH_OK();
    p->prepped = 1;

    // initialize_weights runs with iw_l2_lambda_0 and the DOP / DRT ratio kept (drt1d.py:640-646)
    const double dop_l2 = p->prepared ? p->desc.dop_l2_lambda_0 : 0.0;
    const GramL2 g = plan_l2(p, p->opts.iw_l2_lambda_0, p->opts.derivative_weights,
                             dop_l2 / p->opts.l2_lambda_0 * p->opts.iw_l2_lambda_0);
    // initialize_weights' QPs: the loop's arguments with initialize_weights' own constraint vector, on the plan's normal
    // equations with every spectrum taking part and a scalar l1
    QpArgs qa = loop_qp_args(p, p->opts.qp);
    if (p->h_init.p) qa.h = p->h_init.d();
    PqArgs iw = p->pq(p->w.d());
    iw.active = nullptr; iw.l1 = nullptr; iw.l1_scalar = p->opts.iw_l1_lambda_0;
    // with the weights launch_prep and launch_row_mask leave (the same for every spectrum, like s = s_0 and rho = rho_0) P
    // differs between the spectra only where their response matrices do, and only q otherwise
    const bool one_p = p->rm_stride == 0;

    // ---- initialize_weights (qphb.py:1609-1681): one un-weighted, weakly penalised QP --------------------------------------
    tm.mark(1);
    const int nc = p->prepared ? p->desc.num_chrono : 0;
    const bool separately = p->prepared && p->desc.init_weights_separately && nc > 0 && nc < m;
    HIPDRT_REQUIRE(!(separately && p->opts.outlier_p > 0.0), "init_weights_separately with outlier_p is not built");
    if (separately) {
        // drt1d.py:648-672: initialize_weights once for the chrono rows and once for the impedance rows.  A QP that sees
        // only one block = unit weights on its rows and zero on the others (the zero rows add exact zeros to P and q)
        const int bounds[3] = {0, nc, m};
        for (int blk = 0; blk < 2; ++blk) {
            tm.mark(1);
            launch_row_mask(st, B, m, bounds[blk], bounds[blk + 1], p->w.d());
            TRY(pq_qp_step(st, tm, iw, g, qa, one_p));
            TRY(launch_init_weights(st, fs, B, 2, bounds[blk], bounds[blk + 1]));
            LAUNCH_OK();
        }
        TRY(launch_init_weights(st, fs, B, 3));
        LAUNCH_OK();
    } else {
        TRY(pq_qp_step(st, tm, iw, g, qa, one_p));
        if (p->opts.outlier_p > 0.0) {
            // qphb.py:1629-1656: weights from the first overfit with outlier down-weighting (variance matrix without each
            // point's own residual), a second ridge QP weighted by them (every spectrum its own P now), weights again
            TRY(launch_init_weights(st, fs, B, 0));
            LAUNCH_OK();
            tm.mark(1);
            PqArgs ow = iw; ow.w = p->est_w.d();
            TRY(pq_qp_step(st, tm, ow, g, qa, false));
        }
        TRY(launch_init_weights(st, fs, B, 1));
        LAUNCH_OK();
    }
    if (p->prepared && p->desc.weight_method == 1 && nc > 0 && nc < m) {
        // hybrid_weight_factor_method='weight' (drt1d.py:748-760): per-measurement row factors from the initial weights
        if (!p->w_eff.p) HIPDRT_CHECK(p->w_eff.alloc((size_t)p->capacity * m * sizeof(double)));
        if (p->wrow.bytes < (size_t)p->capacity * m * sizeof(double)) HIPDRT_CHECK(p->wrow.alloc((size_t)p->capacity * m * sizeof(double)));
        if (!p->wfac.p) HIPDRT_CHECK(p->wfac.alloc((size_t)p->capacity * 2 * sizeof(double)));
        p->wrow_batched = 1;
        launch_weight_method(st, fs, B, p->desc.fixed_chrono_factor, p->desc.fixed_eis_factor, p->wrow.d(), p->wfac.d());
        LAUNCH_OK();
    }

    // ---- outer loop (drt1d.py:877-988) ----------------------------------------------------------------------
    TRY(outer_loop(p, st, tm, fs, [&](int it) {
        if (!p->has_weight_factors()) return p->w.d();
        // drt1d.py:889-901: row factors every iteration, weight_factor from the second
        launch_scale_rows(st, B, m, p->w.d(), (p->wrow_late && it == 0) ? nullptr : p->wrow.d(), p->wrow_batched,
                          it > 0 ? p->weight_factor : 1.0, p->active.i(), p->w_eff.d());
        return p->w_eff.d();
    }));
    // ---- calculate_pq's q with the final weights (qphb.py:1154-1183) ---------------------------------------
    tm.mark(4);
    const double* wfin = p->w.d();
    if (p->has_weight_factors()) {
        // drt1d.py:990-1000: weights *= weight_factor (these are `true_weights`); calculate_pq sees them times the row factors
        if (p->wrow_late) {      // vector weight_factor: part of the weights themselves, no separate "scaled" weights
            launch_scale_rows(st, B, m, p->w.d(), p->wrow.d(), p->wrow_batched, p->weight_factor, nullptr, p->w.d());
            launch_scale_rows(st, B, m, p->w.d(), nullptr, 0, 1.0, nullptr, p->w_eff.d());
        } else {
            launch_scale_rows(st, B, m, p->w.d(), nullptr, 0, p->weight_factor, nullptr, p->w.d());
            launch_scale_rows(st, B, m, p->w.d(), p->wrow.d(), p->wrow_batched, 1.0, nullptr, p->w_eff.d());
        }
        wfin = p->w_eff.d();
    }
    return outer_finish(p, st, tm, wfin);
}

// ---- sub-batches ---------------------------------------------------------------------------------------------------------
// Spectra finish after 4 ... 50 outer iterations, so the tail of ONE batch's launch sequence leaves most CUs idle, and between
// two kernels of a sequence the device waits for the host's "anyone still active?" read-back.  Several sequences side by side
// fill both gaps.  bench.py / mapping.fit_observations(inflight=k) do that with k plans (k x the memory, k host threads of the
// caller); here the SAME effect comes from inside one plan: its staged batch is cut into contiguous ranges, every range is
// fitted by plan_fit_one on a view whose buffers are windows into the plan's own (nothing is allocated per range but a
// stream and a 4-byte counter), each on its own stream and worker thread, and the call returns when all are done.  Every
// kernel of the loop works per spectrum (reductions included), so a spectrum's result does not depend on which range it is in:
// bit-identical to the un-split fit as long as both use the same coneqp kernel (ranges of more than #CUs / 16 spectra).
static int subbatch_count(const hipdrt_plan* p) {
    if (p->prepared || p->hist_b >= 0 || p->has_weight_factors() || p->opts.outlier_p > 0.0 || p->qp_G != 0) return 1;
    // measured on one MI355X (profiles/r04_subbatch_sweep.txt): ranges below ~300 spectra lose to launch-wave quantisation
    // (fits/s with k = 1 / 2 / 3 / 4 ranges: 1024 spectra 1902 / 2110 / 2106 / 1660, 1250: 2001 / 2205 / 2219 / 1796, 2500: 2229 / 2375 / 2408 / 2104).
    // Round 5: TWO ranges from 600 spectra on, never three.  The kernel trace says why k = 3 and k = 4 lose (tools/trace_ranges.sh,
    // profiles/r05w_trace_ranges_1250.txt): the runtime maps streams onto 4 hardware queues by default, the ranges' streams landed
    // on TWO of them -- with k = 3 one queue carries two ranges' launch sequences one behind the other (102 coneqp launches
    // against 51 on the other queue), with k = 4 two each, and never more than two coneqp launches run at a time.  With
    // GPU_MAX_HW_QUEUES=8 in the process environment every range has its own queue and k = 2 / 3 / 4 measure 2285 / 2281 / 2330
    // at 1250 spectra (profiles/r05x_ab_hw_queues.txt) -- the library cannot set that for its host (it is read when the HIP
    // runtime starts), so it keeps the choice that is right with either setting.
    // Round 6: the ranges run on the library's own streams, picked per fit by activity and compute pipe (api.hip: StreamPool), so every
    // range has a queue and a pipe to itself whatever else the process has created (profiles/r06_trace_queue_placement.txt: 2254 ...
    // 2324 fits/s in all placements tried, against 1778 with two ranges on one queue and 2205 with two on one pipe), and FOUR ranges
    // from 1000 spectra on are the best cut (profiles/r06_subbatch_sweep.txt, k = 1 / 2 / 3 / 4 / 6: 1024 spectra 2048 / 2262 / 2261 /
    // 2320 / 2214, 1250: 2150 / 2368 / 2351 / 2422 / 2317, 2500: 2392 / 2556 / 2587 / 2600 / 2524; six lose: four pipes) -- as many
    // as the pool has streams: three under the runtime's default of 4 hardware queues, four with GPU_MAX_HW_QUEUES >= 5 (the host
    // layer's loader exports 8 unless its caller has set the variable).
    const int k_auto = p->B >= 1000 ? std::min(4, pool_size(p->ctx->device)) : (p->B >= 600 ? 2 : 1);
    int k = p->subbatches >= 1 ? std::min(p->subbatches, std::max(1, p->B / 64)) : k_auto;
    // the promise is "the bits of the un-split fit": the whole batch AND the smallest range must choose the batch coneqp kernel as
    // the views will see it (qp_layout runs qp_group_size on the view's own count with the context's current override, which may
    // have been set after the plan was allocated) -- otherwise fewer ranges, down to one
    const int force = p->ctx ? p->ctx->qp_force_group : -1;
    if (qp_group_size(p->B, p->n, force) != 0) return 1;
    while (k > 1 && qp_group_size(p->B / k, p->n, force) != 0) --k;
    return k;
}

int hipdrt_plan_fit(hipdrt_plan* p) try {
    HIPDRT_REQUIRE(p, "plan is NULL");
    HIPDRT_REQUIRE(p->B >= 1, "no spectra staged (call hipdrt_plan_upload)");
    const int k = subbatch_count(p);
    if (k <= 1) {
        LoopOnContextStream busy(p->ctx);
        return plan_fit_one(p);
    }
    TRY(enter(p->ctx));
    HIPDRT_CHECK(hipStreamSynchronize(p->ctx->stream));       // whatever staged the batch is done
    if (p->n_active_sub.bytes < (size_t)k * sizeof(int)) HIPDRT_CHECK(p->n_active_sub.alloc(16 * sizeof(int)));
    if (p->premv.bytes < 3 * (size_t)p->capacity * p->m * sizeof(double))      // the ranges' products buffers are windows of this one
        HIPDRT_CHECK(p->premv.alloc(3 * (size_t)p->capacity * p->m * sizeof(double)));
    while ((int)p->subs.size() < k) p->subs.emplace_back(new hipdrt_subfit());
    const int B = p->B;
    for (int i = 0; i < k; ++i) {
        const int b0 = (int)((long long)B * i / k), b1 = (int)((long long)B * (i + 1) / k);
        TRY(make_view(p, *p->subs[i], i, b0, b1 - b0));
    }
    // the ranges' streams: borrowed from the library's pool for this fit, the least busy ones (the context's own may be among
    // them: it is idle until the ranges are done)
    struct Borrowed {
        int device, k; int idx[16]; hipStream_t st[16];
        Borrowed(int device_, int k_) : device(device_), k(k_) { pool_borrow(device, k, idx, st); }
        ~Borrowed() { pool_return(device, k, idx); }
    } streams(p->ctx->device, k);
    for (int i = 0; i < k; ++i) p->subs[i]->ctx.stream = streams.st[i];
    const auto t0 = std::chrono::steady_clock::now();
    // no exception may cross the C ABI, and a joinable std::thread must not be destroyed: ranges whose worker thread cannot
    // be created (std::system_error) are fitted right here, on the caller's thread, after the started ones were joined
    std::vector<std::thread> workers;
    workers.reserve(k);
    int started = 0;
    for (int i = 0; i < k; ++i) {
        hipdrt_subfit* sf = p->subs[i].get();
        sf->rc = HIPDRT_OK;
        try {
            workers.emplace_back([sf] {
                sf->rc = plan_fit_one(&sf->view);
                if (sf->rc) sf->err = hipdrt_last_error();
            });
            ++started;
        } catch (...) {
            break;
        }
    }
    for (auto& w : workers) w.join();
    for (int i = started; i < k; ++i) {
        hipdrt_subfit* sf = p->subs[i].get();
        sf->rc = plan_fit_one(&sf->view);
        if (sf->rc) sf->err = hipdrt_last_error();
    }
    const float wall_ms = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    for (int i = 0; i < 5; ++i) { p->t_ms[i] = 0; p->launches[i] = 0; }
    for (int i = 0; i < k; ++i) {
        hipdrt_subfit* sf = p->subs[i].get();
        if (sf->rc) { set_error("sub-batch " + std::to_string(i) + ": " + sf->err); return sf->rc; }
        // phase times are HIP-event intervals on streams that share the GPU: summed over the ranges they exceed the wall time
        for (int c = 1; c < 5; ++c) { p->t_ms[c] += sf->view.t_ms[c]; p->launches[c] += sf->view.launches[c]; }
    }
    p->t_ms[0] = wall_ms; p->launches[0] = 1;
    p->prepped = 1;
    return HIPDRT_OK;
} HIPDRT_CATCH

// every spectrum takes part again (warm restart, hipdrt_plan_iterate).  The stream is idle on return: `ones`, and whatever host
// arrays the caller has queued for upload before, may go.
static int reactivate_all(hipdrt_plan* p, hipStream_t st) {
    std::vector<int> ones(p->B, 1);
    HIPDRT_CHECK(hipMemcpyAsync(p->active.p, ones.data(), (size_t)p->B * sizeof(int), hipMemcpyHostToDevice, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
}

// drt1d._continue_from_init (hybdrt/models/drt1d.py:1270-1365) for the fitted batch: the same outer loop re-entered from
// the state on the device (x, s, rho [, dop_rho], weights; est_weights, xmx / dop_xmx norms and data scale stay) with updated
// hyper-parameters.  Any data type: on prepared plans (chrono / joint fits, DOP) the plan's row factors -- chrono / eis weight
// factors, hipdrt_plan_set_weight_factors -- multiply the weights at the top of every iteration together with `weight_factor`
// (1314-1318), the DOP pass runs as in the fit, and the vz_offset column is rewritten after every iteration from a matrix
// whose offset column is FROZEN as this call found it (1295-1298, 1353-1357: the reference copies rm at entry, zeroing the
// baseline columns only; the fit itself copied while the column was still zero).  The plan's scalar weight_factor is not used.
int hipdrt_plan_continue(hipdrt_plan* p, const hipdrt_fit_opts* opts, double weight_factor, int min_iter) try {
    HIPDRT_REQUIRE(p && opts, "NULL pointer");
    HIPDRT_REQUIRE(p->B >= 1, "no fitted batch in the plan");
    HIPDRT_REQUIRE(opts->max_iter >= 1 && min_iter >= 1, "max_iter, min_iter >= 1");
    LoopOnContextStream busy(p->ctx);
    // rejected calls must leave the finished fit as it is: every check comes before the first write
    HIPDRT_REQUIRE(p->prepared || !p->has_weight_factors(),
                   "warm restarts take their weight_factor argument; clear the plan's weight factors");
    HIPDRT_REQUIRE(!(p->wrow.p && p->wrow_late), "a vector-valued weight_factor belongs to the fit, not to its warm restarts");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const int B = p->B, m = p->m;
    TRY(plan_hist_reserve(p, opts->max_iter));
    // the row factors may be new with this call (hipdrt_plan_set_weight_factors after the fit): the buffer of the scaled final
    // weights is filled behind the loop, below
    const bool rowfac = p->prepared && p->wrow.p;
    if (rowfac && !p->w_eff.p) HIPDRT_CHECK(p->w_eff.alloc((size_t)p->capacity * m * sizeof(double)));
    // outlier_p (qphb.py:1545-1594: estimate_weights forms outlier_t and the T V T matrix anew from every iterate, what
    // _continue_from_init is handed is never read, drt1d.py:1300-1304): only the record of 1 - outlier probability needs room
    if (opts->outlier_p > 0.0 && !p->outlier_t.p) HIPDRT_CHECK(p->outlier_t.alloc((size_t)p->capacity * m * sizeof(double)));
    FitState fs = p->state();
    fs.opts = *opts; fs.continue_mode = 1; fs.min_iter = min_iter;
    if (p->prepared && p->desc.vz_index >= 0) {
        if (!p->vz_entry.p) HIPDRT_CHECK(p->vz_entry.alloc((size_t)p->capacity * m * sizeof(double)));
        launch_copy_column(st, B, m, p->rm.d(), p->rm_stride, p->ldrm, p->desc.vz_index, p->vz_entry.d());
        LAUNCH_OK();
        fs.vz_entry = p->vz_entry.d();
    }
    PhaseTimer tm(st);
    tm.mark(4);
    if (p->hist_b >= 0) HIPDRT_CHECK(hipMemsetAsync(p->hist_rows.p, 0, sizeof(int), st));
    TRY(reactivate_all(p, st));
    HIPDRT_CHECK(hipMemsetAsync(p->qp_iters_total.p, 0, (size_t)B * sizeof(int), st));      // QP iteration totals restart
    TRY(outer_loop(p, st, tm, fs, [&](int) {
        // in place, like the reference's `weights[:num_chrono] *= ...; weights = weights * weight_factor`: the hyper step
        // replaces the weights with a fresh estimate afterwards
        if (p->prepared && p->wrow.p)
            launch_scale_rows(st, B, m, p->w.d(), p->wrow.d(), p->wrow_batched, weight_factor, p->active.i(), p->w.d());
        else if (weight_factor != 1.0) launch_scale_weights(st, fs, B, weight_factor);
        return p->w.d();
    }));
    tm.mark(4);
    // What the posterior entry points call "the final P" (hipdrt_plan_p_matrix, _param_cov, _distribution_cov, _param_var read
    // w_eff whenever the plan has weight factors): the weights this restart ended with -- the last iteration's fresh estimate --
    // times the factors its QPs saw, i.e. the matrix the NEXT iteration would have solved with, and q to match.  (The fit
    // leaves true_weights x row factors there, drt1d.py:990-1006; left alone, w_eff would still hold the FIRST fit's scaled
    // weights, or nothing at all when the factors came with this call.)
    const double* wfin = p->w.d();
    if (rowfac) {
        launch_scale_rows(st, B, m, p->w.d(), p->wrow.d(), p->wrow_batched, weight_factor, nullptr, p->w_eff.d());
        wfin = p->w_eff.d();
    }
    return outer_finish(p, st, tm, wfin);
} HIPDRT_CATCH

// qphb.iterate_qphb (hybdrt/models/qphb.py:606-972) for every staged measurement of a prepared plan: the QP on
// (weights, s_vectors, rho) as given, then the s / rho / DOP hyper-parameter pass, estimate_weights and is_converged
// against x_in.  What _qphb_fit_core does around the call (xmx norms of the first iteration, data rescaling, the
// vz_offset column; drt1d.py:903-979) is not part of it.
int hipdrt_plan_iterate(hipdrt_plan* p, const hipdrt_iterate_state* in, int* converged, int* qp_status, int* qp_iters,
                        double* primal_objective) try {
    HIPDRT_REQUIRE(p, "plan is NULL");
    HIPDRT_REQUIRE(p->prepared, "hipdrt_plan_iterate works on prepared plans (the caller's rm, rv as iterate_qphb takes them)");
    HIPDRT_REQUIRE(p->B >= 1, "no measurements staged (call hipdrt_plan_upload_prepared)");
    HIPDRT_REQUIRE(!p->has_weight_factors(), "weight factors belong to _qphb_fit_core, not to iterate_qphb");
    hipStream_t st; TRY(enter(p->ctx, &st));
    const int B = p->B, n = p->n, m = p->m;
    FitState fs = p->state();
    fs.continue_mode = 2; fs.min_iter = 1;
    fs.opts.max_iter = 2;                      // never "stopped at max_iter": fit_status 0 <=> converged
    if (!p->prepped) {                         // variance floor of estimate_weights + default state (qphb.py:1569)
        launch_prep(st, fs, B);
        LAUNCH_OK();
        p->prepped = 1;
    }
    if (in) {
        const size_t b = (size_t)B;
        struct { const double* src; void* dst; size_t cnt; } cp[] = {
            {in->x_in, p->x_in.p, b * n}, {in->x_in, p->x.p, b * n}, {in->s_vectors, p->s.p, b * 3 * n},
            {in->rho, p->rho.p, b * 3}, {in->dop_rho, p->dop_rho.p, b * 3}, {in->weights, p->w.p, b * m},
            {in->est_weights, p->est_w.p, b * m}, {in->xmx_norms, p->xmx.p, b * 3},
            {in->dop_xmx_norms, p->dop_xmx.p, b * 3}};
        for (auto& c : cp)
            if (c.src) HIPDRT_CHECK(hipMemcpyAsync(c.dst, c.src, c.cnt * sizeof(double), hipMemcpyHostToDevice, st));
    }
    PhaseTimer tm(st);
    tm.mark(4);
    TRY(reactivate_all(p, st));                    // (the caller's arrays may go once this returns)
    HIPDRT_CHECK(hipMemsetAsync(p->n_active.p, 0, sizeof(int), st));
    const GramL2 g = plan_l2(p, p->opts.l2_lambda_0, p->opts.derivative_weights, p->desc.dop_l2_lambda_0);
    const QpArgs qa = loop_qp_args(p, p->opts.qp);
    tm.mark(1);
    TRY(outer_iteration(p, st, tm, fs, g, qa, p->w.d(), nullptr, 0));      // (no dispatch order)
    tm.mark(-1);
    std::vector<int> act(B);
    HIPDRT_CHECK(hipMemcpyAsync(act.data(), p->active.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    if (qp_status) HIPDRT_CHECK(hipMemcpyAsync(qp_status, p->qp_status.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    if (qp_iters) HIPDRT_CHECK(hipMemcpyAsync(qp_iters, p->qp_iters.p, (size_t)B * sizeof(int), hipMemcpyDeviceToHost, st));
    if (primal_objective)
        HIPDRT_CHECK(hipMemcpyAsync(primal_objective, p->pcost.p, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    if (converged) for (int b = 0; b < B; ++b) converged[b] = act[b] == 0;
    tm.collect(p->t_ms, p->launches);
    return HIPDRT_OK;
} HIPDRT_CATCH

// ---- PFRT step store (include/hipdrt.h) ---------------------------------------------------------------------------------------
int hipdrt_plan_pfrt_bytes_per_spectrum(int n, int steps, long long* bytes) try {
    HIPDRT_REQUIRE(bytes && n >= 1 && steps >= 1, "n, steps >= 1");
    *bytes = pfrt_store_bytes_per_spectrum(n, steps);
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_pfrt_begin(hipdrt_plan* p, int max_steps) try {
    HIPDRT_REQUIRE(p, "plan is NULL");
    HIPDRT_REQUIRE(max_steps >= 1 && max_steps <= 1024, "1 <= max_steps <= 1024");
    TRY(enter(p->ctx));
    p->pf_steps = 0;
    if (max_steps <= p->pf_max) return HIPDRT_OK;
    const PfrtStoreLayout L = p->pf_layout();
    const size_t D = sizeof(double);
    const bool dop = p->prepared && p->desc.dop_size > 0;
    struct { DevBuf* buf; size_t bytes; } want[] = {
        {&p->pf_x, L.x_elems(max_steps) * D}, {&p->pf_rho, L.rho_elems(max_steps) * D}, {&p->pf_s, L.s_elems(max_steps) * D},
        {&p->pf_rss, L.scalar_elems(max_steps) * D}, {&p->pf_slw, L.scalar_elems(max_steps) * D},
        {&p->pf_status, L.scalar_elems(max_steps) * sizeof(int)}, {&p->pf_dop_rho, dop ? L.rho_elems(max_steps) * D : 0}};
    p->pf_max = 0;
    for (auto& w : want) {
        if (w.bytes == 0) continue;
        const hipError_t e = w.buf->alloc(w.bytes);
        if (e != hipSuccess) {
            // the plan itself is untouched: the store is simply empty again
            for (auto& v : want) v.buf->release();
            (void)hipGetLastError();
            set_error(std::string("PFRT step store: ") + hipGetErrorString(e));
            return HIPDRT_E_HIP;
        }
    }
    p->pf_max = max_steps;
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_pfrt_record(hipdrt_plan* p) try {
    HIPDRT_REQUIRE(p, "plan is NULL");
    HIPDRT_REQUIRE(p->B >= 1 && p->prepped, "no fitted batch in the plan");
    HIPDRT_REQUIRE(p->pf_max >= 1, "hipdrt_plan_pfrt_begin has not been called");
    HIPDRT_REQUIRE(p->pf_steps < p->pf_max, "the PFRT step store is full");
    // (hipdrt_plan_fit and hipdrt_plan_continue return with every range joined and the plan's stream idle)
    hipStream_t st; TRY(enter(p->ctx, &st));
    const PfrtStoreLayout L = p->pf_layout();
    const size_t B = (size_t)p->B, n = (size_t)p->n, D = sizeof(double);
    const int step = p->pf_steps;
    const auto d2d = [&](DevBuf& dst, size_t off, const DevBuf& src, size_t bytes) {
        return hipMemcpyAsync(static_cast<char*>(dst.p) + off, src.p, bytes, hipMemcpyDeviceToDevice, st);
    };
    HIPDRT_CHECK(d2d(p->pf_x, L.x(step) * D, p->x, B * n * D));
    HIPDRT_CHECK(d2d(p->pf_rho, L.rho(step) * D, p->rho, B * 3 * D));
    HIPDRT_CHECK(d2d(p->pf_s, L.s(step) * D, p->s, B * 3 * n * D));
    HIPDRT_CHECK(d2d(p->pf_status, L.scalar(step) * sizeof(int), p->fit_status, B * sizeof(int)));
    if (p->pf_dop_rho.p) HIPDRT_CHECK(d2d(p->pf_dop_rho, L.rho(step) * D, p->dop_rho, B * 3 * D));
    TRY(launch_llh(st, p->state(), p->B, p->pf_rss.d() + L.scalar(step), p->pf_slw.d() + L.scalar(step), 0));
    LAUNCH_OK();
    HIPDRT_CHECK(hipStreamSynchronize(st));
    p->pf_steps += 1;
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_pfrt_restore_s(hipdrt_plan* p, int step, double factor) try {
    HIPDRT_REQUIRE(p, "plan is NULL");
    HIPDRT_REQUIRE(p->B >= 1 && p->prepped, "no fitted batch in the plan");
    HIPDRT_REQUIRE(step >= 0 && step < p->pf_steps, "step out of range of the recorded PFRT steps");
    HIPDRT_REQUIRE(factor > 0.0 && std::isfinite(factor), "factor must be positive and finite");
    hipStream_t st; TRY(enter(p->ctx, &st));
    launch_scale_rows(st, p->B, 3 * p->n, p->pf_s.d() + p->pf_layout().s(step), nullptr, 0, factor, nullptr, p->s.d());
    LAUNCH_OK();
    HIPDRT_CHECK(hipStreamSynchronize(st));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_plan_pfrt_steps(hipdrt_plan* p, int* steps) try {
    HIPDRT_REQUIRE(p && steps, "NULL pointer");
    *steps = p->pf_steps;
    return HIPDRT_OK;
} HIPDRT_CATCH

}  // extern "C"
