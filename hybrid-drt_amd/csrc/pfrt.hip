// The probability function of relaxation times of a fitted batch, DRT.predict_pfrt (hybdrt/models/drt1d.py:2716-2858), on rows
// that are already evaluated; hipdrt/models/pfrt.py is the same arithmetic in numpy.
//
//   pfrt_step_kernel      one regularisation step: at every peak that peaks_kernel (method 0, explicit height and prominence)
//                         found, the credibility min(P(|f| > 0), P(curvature peak)) with both two-sided probabilities
//                         1 - erfc(mu / (sigma sqrt 2)) (drt1d.py:2811-2829); sigma^2 is e' inv(P) e scaled as drt_band_kernel
//                         scales it, then extend_var's clamp and the floor -- on BOTH variance rows (2772-2786)
//   pfrt_combine_kernel   the posterior weights of the steps (2730-2749), the weighted sum (2831-2834), the smoothing matrix
//                         (2840-2848, formed on the fly), the contiguous-range integration (hybdrt/models/pfrt.py:22-46) and the
//                         normalisation by the row's maximum
//   pfrt_select_kernel    DRT.select_pfrt_candidates (drt1d.py:2860-2865 over hybdrt/models/pfrt.py:49-213) on the raw PFRT: the
//                         ranges and their ranking by area, every step row shifted onto the ranges' peaks, its correlation with
//                         the growing sets of best peaks times the step likelihood, and the best step of every set
//
// One 256-thread workgroup per spectrum.  Every sum runs in one fixed order (over the steps ascending, over the grid ascending), so
// a spectrum's result depends neither on B nor on its position.  Each kernel's global stores are its dense output rows (offset
// b * n + i with i < n) and one scalar per spectrum.  Compiled with -ffp-contract=off: the probabilities round as written.
#include <cmath>

#include "hyper_dev.hpp"
#include "peaks_dev.hpp"

namespace hipdrt {

static constexpr double PF_LOG_2PI = 1.8378770664093453;    // np.log(2 * np.pi)

// grid = B
__global__ __launch_bounds__(PKT) void pfrt_step_kernel(PfrtStepArgs a) {
    const int b = blockIdx.x, tid = threadIdx.x, n = a.neval;
    const size_t row = (size_t)b * n;
    const bool no_var = a.var_status && a.var_status[b] != 0;
    if ((a.fit_status && a.fit_status[b] < 0) || no_var) {     // a failed fit, or a step P that is not positive definite
        for (int i = tid; i < n; i += PKT) a.out[row + i] = NAN;
        if (tid == 0 && a.bad && no_var) a.bad[b] = 1;
        return;
    }
    double c2 = 1.0, n2 = 1.0;
    if (a.cs) c2 = a.cs[b] * a.cs[b];
    if (a.norm) n2 = a.norm[b] * a.norm[b];
    auto scaled = [&](const double* var, int i) { return var_scaled(var[(size_t)b * a.ldv + i], a.cs, c2, a.norm, n2); };
    // extend_var's bounds, from the scaled rows in global memory
    const int li = a.ext_left, ri = a.ext_right;
    ExtClamp c[2];
    for (int k = 0; k < 2; ++k) {
        const double* var = k ? a.var_fxx : a.var_f;
        c[k] = ext_clamp(li, ri, li >= 0 ? scaled(var, li) : 0.0, ri >= 0 ? scaled(var, ri) : 0.0);
    }
    for (int i = tid; i < n; i += PKT) {
        double p = 0.0;
        if (a.peak_sign[row + i] != 0) {
            double v[2];
            for (int k = 0; k < 2; ++k) {
                double x = c[k].apply(scaled(k ? a.var_fxx : a.var_f, i), i);
                if (a.floor > 0.0 && x < a.floor) x = a.floor;
                v[k] = x;
            }
            const double mp = np_min(a.prominences[row + i], a.heights[row + i]);
            const double f_prob = 1.0 - erfc(fabs(a.f[row + i]) / (sqrt(v[0]) * PK_SQRT2));
            const double fxx_prob = 1.0 - erfc(mp / (sqrt(v[1]) * PK_SQRT2));
            p = np_min(f_prob, fxx_prob);
        }
        a.out[row + i] = p;
    }
}

int launch_pfrt_step(hipStream_t s, const PfrtStepArgs& a, int B) {
    HIPDRT_REQUIRE(B >= 1 && a.neval >= 1, "pfrt_step: B, neval >= 1");
    HIPDRT_REQUIRE(a.peak_sign && a.heights && a.prominences && a.f && a.var_f && a.var_fxx && a.out, "pfrt_step: NULL row");
    HIPDRT_REQUIRE(std::isfinite(a.floor), "fxx_var_floor must be finite");
    HIPDRT_REQUIRE(a.ext_left >= -1 && a.ext_left < a.neval && a.ext_right >= -1 && a.ext_right < a.neval,
                   "ext_left and ext_right: an index of the evaluation grid, or -1");
    hipLaunchKernelGGL(pfrt_step_kernel, dim3(B), dim3(PKT), 0, s, a);
    return HIPDRT_OK;
}

// evaluate_llh(marginalize_weights=True) of one step from its two recorded sums (pfrt_llh_consts gives c, alpha_n, beta_0)
__device__ inline double pf_step_llh(double c, double alpha_n, double beta_0, double rss, double slw) {
    return (c - alpha_n * log(beta_0 + 0.5 * rss)) + slw;
}

// pfrt.get_peak_ranges / identify_peaks / integrate_peaks (hybdrt/models/pfrt.py:8-46) for the range of v >= thr that starts at k
// (false: none starts there): its exclusive end, its first maximum, and np.trapezoid(v[start - 1:end + 1]) with unit spacing
struct PfRange { int end, peak; double area; };
__device__ inline bool pf_range_at(const double* v, int n, double thr, int k, PfRange& r) {
    if (!(v[k] >= thr) || (k > 0 && v[k - 1] >= thr)) return false;
    int e = k, pk = k;
    while (e < n && v[e] >= thr) { if (v[e] > v[pk]) pk = e; ++e; }
    // np.trapezoid(pf[start - 1:end + 1]): empty (or one sample) for a range that starts at index 0
    double ar = 0.0;
    if (k > 0) {
        const int hi = e + 1 < n ? e + 1 : n;
        for (int i = k - 1; i + 1 < hi; ++i) ar += (v[i + 1] + v[i]) / 2.0;
    }
    r.end = e; r.peak = pk; r.area = ar;
    return true;
}

size_t pfrt_combine_lds_bytes(int S, int np, int nout) { return pfrt_combine_lds(nullptr, S, np, nout).bytes; }

// grid = B
__global__ __launch_bounds__(PKT) void pfrt_combine_kernel(PfrtCombineArgs a) {
    extern __shared__ double sm[];
    __shared__ double red[PKT];
    const int b = blockIdx.x, B = gridDim.x, tid = threadIdx.x, S = a.S, np = a.np, nout = a.nout;
    const PfrtCombineLds L = pfrt_combine_lds(sm, S, np, nout);
    double *acc = L.acc, *ltp = L.ltp, *lto = L.lto, *v = L.v, *res = L.res, *post = L.post;

    if ((a.fit_status && a.fit_status[b] < 0) || (a.bad && a.bad[b] != 0)) {
        for (int k = tid; k < nout; k += PKT) if (a.pfrt) a.pfrt[(size_t)b * nout + k] = NAN;
        for (int j = tid; j < np; j += PKT) if (a.raw) a.raw[(size_t)b * np + j] = NAN;
        for (int i = tid; i < S; i += PKT) if (a.post) a.post[(size_t)i * B + b] = NAN;
        return;
    }
    for (int j = tid; j < np; j += PKT) ltp[j] = a.ltp[j];
    for (int k = tid; k < nout; k += PKT) lto[k] = a.smooth ? a.lto[k] : 0.0;

    // ---- posterior weights of the steps (drt1d.py:2730-2749) ----
    for (int i = tid; i < S; i += PKT) {
        const size_t o = (size_t)i * a.ld_sum + b;
        const double llh = pf_step_llh(a.c, a.alpha_n, a.beta_0, a.rss[o], a.slw[o]);
        const double z = (a.ln_factors[i] - a.prior_mu) / a.prior_sigma;
        post[i] = -0.5 * (PF_LOG_2PI + 2.0 * log(a.prior_sigma) + z * z) + llh;
    }
    __syncthreads();
    double mx = post[0];
    for (int i = 1; i < S; ++i) mx = np_max(mx, post[i]);
    __syncthreads();
    for (int i = tid; i < S; i += PKT) post[i] = exp((post[i] - mx) * a.n_eff);
    __syncthreads();
    double area = post[0];
    if (S > 1) {
        area = 0.0;
        for (int i = 0; i + 1 < S; ++i) area += ((a.ln_factors[i + 1] - a.ln_factors[i]) * (post[i + 1] + post[i])) / 2.0;
    }
    __syncthreads();
    for (int i = tid; i < S; i += PKT) post[i] = post[i] / area;
    __syncthreads();
    double psum = 0.0;
    for (int i = 0; i < S; ++i) psum += post[i];

    // ---- the weighted sum over the steps, ascending ----
    for (int j = tid; j < np; j += PKT) {
        double t = 0.0;
        for (int i = 0; i < S; ++i) t += post[i] * a.step_pfrt[(size_t)i * a.ld_step + (size_t)b * np + j];
        acc[j] = t / psum;
    }
    __syncthreads();

    // ---- smoothing: row k of exp(-(eps |ln tau_out_k - ln tau_pfrt_j|)^(2 order)) times the accumulator (zeros add nothing) ----
    if (a.smooth) {
        const double ex = 2.0 * a.smooth_order;
        for (int k = tid; k < nout; k += PKT) {
            double t = 0.0;
            for (int j = 0; j < np; ++j) {
                const double r = acc[j];
                if (r != 0.0) t += exp(-pow(a.smooth_eps * fabs(lto[k] - ltp[j]), ex)) * r;
            }
            v[k] = t;
        }
    } else {
        for (int k = tid; k < nout; k += PKT) v[k] = acc[k];
    }
    __syncthreads();

    // ---- integrate_peaks (models/pfrt.py:22-46): every contiguous range of v >= threshold becomes one value at its maximum ----
    if (a.integrate) {
        const double thr = a.thr;
        for (int k = tid; k < nout; k += PKT) res[k] = 0.0;
        __syncthreads();
        for (int k = tid; k < nout; k += PKT) {
            PfRange r;
            if (pf_range_at(v, nout, thr, k, r)) res[r.peak] = r.area;
        }
        __syncthreads();
        for (int k = tid; k < nout; k += PKT) v[k] = res[k];
        __syncthreads();
    }

    // ---- tot / np.max(tot): an all-zero row gives NaN, as upstream ----
    if (a.normalize) {
        double m = -INFINITY;
        for (int k = tid; k < nout; k += PKT) m = np_max(m, v[k]);
        red[tid] = m;
        __syncthreads();
        for (int w = PKT / 2; w > 0; w >>= 1) {
            if (tid < w) red[tid] = np_max(red[tid], red[tid + w]);
            __syncthreads();
        }
        m = red[0];
        for (int k = tid; k < nout; k += PKT) v[k] = v[k] / m;      // (every thread scales the entries it wrote or copied itself)
    }

    // ---- the dense rows: the only global stores ----
    for (int k = tid; k < nout; k += PKT) if (a.pfrt) a.pfrt[(size_t)b * nout + k] = v[k];
    for (int j = tid; j < np; j += PKT) if (a.raw) a.raw[(size_t)b * np + j] = acc[j];
    for (int i = tid; i < S; i += PKT) if (a.post) a.post[(size_t)i * B + b] = post[i];
}

// grid = B.  DRT.select_pfrt_candidates: pfrt.select_candidates (hybdrt/models/pfrt.py:164-213) on the raw PFRT of the spectrum.
// hipdrt/models/pfrt.py (select_compact) is the same rule in numpy, sum for sum.  The per-range and per-candidate work sits on the
// first max_peaks threads; every sum over the grid runs in ascending order on one thread.
__global__ __launch_bounds__(PKT) void pfrt_select_kernel(PfrtSelectArgs a) {
    extern __shared__ double sm[];
    const int b = blockIdx.x, tid = threadIdx.x, S = a.S, np = a.np, mp = a.max_peaks;
    const PfrtSelectLds L = pfrt_select_lds(sm, np, mp);
    const size_t slot = (size_t)b * mp;
    // what a spectrum without an answer leaves: every slot unused, the three counts as given
    auto leave = [&](int num_peaks, int num_candidates, int status) {
        for (int k = tid; k < mp; k += PKT) {
            if (a.ranked_index) a.ranked_index[slot + k] = -1;
            if (a.step_index) a.step_index[slot + k] = -1;
            if (a.magnitude) a.magnitude[slot + k] = NAN;
            if (a.match_quality) a.match_quality[slot + k] = NAN;
        }
        if (tid == 0) {
            if (a.num_peaks) a.num_peaks[b] = num_peaks;
            if (a.first) a.first[b] = -1;
            if (a.num_candidates) a.num_candidates[b] = num_candidates;
            a.status[b] = status;
        }
    };
    if ((a.fit_status && a.fit_status[b] < 0) || (a.bad && a.bad[b] != 0)) { leave(-1, -1, 0); return; }

    // ---- the ranges of raw >= peak_thresh in ascending order (get_peak_ranges), their peaks and areas ----
    const double thr = a.peak_thresh;
    for (int k = tid; k < np; k += PKT) L.raw[k] = a.raw[(size_t)b * np + k];
    __syncthreads();
    for (int k = tid; k < np; k += PKT) {
        L.rank_at[k] = (L.raw[k] >= thr && !(k > 0 && L.raw[k - 1] >= thr)) ? 1 : 0;      // (a range starts here)
        L.rng[k] = -1;
    }
    if (tid < mp) L.order[tid] = 0;
    __syncthreads();
    if (tid == 0) {
        int cnt = 0;
        for (int k = 0; k < np; ++k)
            if (L.rank_at[k]) { if (cnt < mp) L.start[cnt] = k; ++cnt; }
        L.counts[0] = cnt;
    }
    __syncthreads();
    const int K = L.counts[0];
    if (K == 0) { leave(0, 0, HIPDRT_PFRT_NO_PEAK); return; }
    if (K > mp) { leave(K, 0, HIPDRT_PFRT_TOO_MANY_PEAKS); return; }
    for (int k = tid; k < np; k += PKT) L.rank_at[k] = 0x7fffffff;
    if (tid < K) {
        PfRange r;
        pf_range_at(L.raw, np, thr, L.start[tid], r);
        L.end[tid] = r.end; L.peak[tid] = r.peak; L.area[tid] = r.area;
        // shift_candidate_pfrt's test start <= ti <= end takes the point one past the range with it; the next range starts later
        const int last = r.end < np ? r.end : np - 1;
        for (int ti = L.start[tid]; ti <= last; ++ti) L.rng[ti] = tid;
    }
    __syncthreads();

    // ---- rank_peaks: descending area, of equal areas the higher index first; magnitudes relative to the largest ----
    if (tid < K) {
        int rank = 0;
        for (int q = 0; q < K; ++q) rank += (L.area[q] > L.area[tid] || (L.area[q] == L.area[tid] && q > tid)) ? 1 : 0;
        L.order[rank] = tid;
        L.rank_at[L.peak[tid]] = rank;
    }
    __syncthreads();
    if (tid < K) L.mag[tid] = L.area[L.order[tid]] / L.area[L.order[0]];
    __syncthreads();
    if (tid == 0) {
        int first = 0;
        for (int k = 0; k < K; ++k) if (L.mag[k] >= a.start_thresh) first = k;
        int inc = first, nc = 0;
        while (inc < K - 1) {                    // upstream's loop: K peaks give at most K - 1 targets
            ++nc; ++inc;
            if (L.mag[inc] < a.end_thresh) break;
        }
        L.counts[1] = first; L.counts[2] = nc;
    }
    __syncthreads();
    const int first = L.counts[1], nc = L.counts[2];

    // ---- candidate j = tid: the target has ones at the first + j + 1 best peaks; its mean and centred sum of squares ----
    const int ones = first + tid + 1;
    const double mt = (double)ones / (double)np, fac = 1.0 / (double)(np - 1);
    double best = 0.0, stt = 0.0;
    int best_step = 0;
    if (tid < nc)
        for (int i = 0; i < np; ++i) {
            const double dt = (L.rank_at[i] < ones ? 1.0 : 0.0) - mt;
            stt += dt * dt;
        }
    for (int s = 0; s < S && nc > 0; ++s) {
        for (int k = tid; k < np; k += PKT) L.row[k] = a.step_pfrt[(size_t)s * a.ld_step + (size_t)b * np + k];
        __syncthreads();
        // shift_candidate_pfrt: what ends at point k.  Outside every range an entry stays; inside, the entries of the range move to
        // its peak, where the one from the highest index is left
        for (int k = tid; k < np; k += PKT) {
            const int r = L.rng[k];
            double v = 0.0;
            if (r < 0) {
                if (L.row[k] > 0.0) v = L.row[k];
            } else if (k == L.peak[r]) {
                const int last = L.end[r] < np ? L.end[r] : np - 1;
                for (int ti = last; ti >= L.start[r]; --ti)
                    if (L.row[ti] > 0.0) { v = L.row[ti]; break; }
            }
            L.sh[k] = v;
        }
        __syncthreads();
        if (tid < nc) {
            // np.corrcoef: both rows centred, the sums of products ascending, each times 1 / (np - 1), then the two divisions
            double mc = 0.0;
            for (int i = 0; i < np; ++i) mc += L.sh[i];
            mc = mc / (double)np;
            double scc = 0.0, stc = 0.0;
            for (int i = 0; i < np; ++i) {
                const double dt = (L.rank_at[i] < ones ? 1.0 : 0.0) - mt, dc = L.sh[i] - mc;
                scc += dc * dc;
                stc += dt * dc;
            }
            double r = ((stc * fac) / sqrt(stt * fac)) / sqrt(scc * fac);
            if (r > 1.0) r = 1.0;
            if (r < -1.0) r = -1.0;
            const size_t o = (size_t)s * a.ld_sum + b;
            const double mq = r * pf_step_llh(a.c, a.alpha_n, a.beta_0, a.rss[o], a.slw[o]);
            // np.argmax: the first maximum, and the first NaN beats everything
            if (s == 0 || (!isnan(best) && (isnan(mq) || mq > best))) { best = mq; best_step = s; }
        }
    }
    if (tid < nc) { L.best[tid] = best; L.best_step[tid] = best_step; }
    __syncthreads();

    // ---- the compact result: the only global stores ----
    for (int k = tid; k < mp; k += PKT) {
        if (a.ranked_index) a.ranked_index[slot + k] = k < K ? L.peak[L.order[k]] : -1;
        if (a.magnitude) a.magnitude[slot + k] = k < K ? L.mag[k] : NAN;
        if (a.step_index) a.step_index[slot + k] = k < nc ? L.best_step[k] : -1;
        if (a.match_quality) a.match_quality[slot + k] = k < nc ? L.best[k] : NAN;
    }
    if (tid == 0) {
        if (a.num_peaks) a.num_peaks[b] = K;
        if (a.first) a.first[b] = first;
        if (a.num_candidates) a.num_candidates[b] = nc;
        a.status[b] = 0;
    }
}

int pfrt_select_check(const hipdrt_pfrt_select_opts& o) {
    HIPDRT_REQUIRE(o.max_peaks >= 1 && o.max_peaks <= PFS_MAX_PEAKS, "pfrt_select: 1 <= max_peaks <= 64");
    HIPDRT_REQUIRE(!std::isnan(o.start_thresh) && !std::isnan(o.end_thresh) && !std::isnan(o.peak_thresh),
                   "pfrt_select: start_thresh, end_thresh and peak_thresh must be numbers");
    return HIPDRT_OK;
}

int launch_pfrt_select(hipStream_t s, const PfrtSelectArgs& a, int B) {
    HIPDRT_REQUIRE(B >= 1 && a.S >= 1 && a.S <= 1024, "pfrt_select: B >= 1, 1 <= steps <= 1024");
    HIPDRT_REQUIRE(a.np >= 1 && a.np <= 2048, "pfrt_select: at most 2048 points on the tau_pfrt grid");
    HIPDRT_REQUIRE(a.max_peaks >= 1 && a.max_peaks <= PFS_MAX_PEAKS, "pfrt_select: 1 <= max_peaks <= 64");
    HIPDRT_REQUIRE(a.raw && a.step_pfrt && a.rss && a.slw && a.status, "pfrt_select: NULL input");
    const size_t lds = pfrt_select_lds(nullptr, a.np, a.max_peaks).bytes;
    if (int rc = lds_check(lds, "pfrt_select_kernel", "neval_pfrt, max_peaks")) return rc;
    if (int rc = set_lds(reinterpret_cast<const void*>(pfrt_select_kernel), lds, "pfrt_select_kernel")) return rc;
    hipLaunchKernelGGL(pfrt_select_kernel, dim3(B), dim3(PKT), lds, s, a);
    return HIPDRT_OK;
}

// the constants of evaluate_llh(marginalize_weights=True, alpha_0=2, beta_0=1) for m data rows (drt1d.py:4457-4496):
// llh = (c - alpha_n ln(beta_0 + rss / 2)) + sum(log w)
void pfrt_llh_consts(int m, double* c, double* alpha_n, double* beta_0) {
    const double a0 = 2.0, b0 = 1.0, an = a0 - 1.0 + 0.5 * (double)m;
    *c = a0 * std::log(b0) + std::lgamma(an) - std::lgamma(a0);
    *alpha_n = an; *beta_0 = b0;
}

int pfrt_check(const hipdrt_pfrt_opts& o, int S, int np, int nout) {
    HIPDRT_REQUIRE(S >= 1 && S <= 1024, "1 <= steps <= 1024");
    HIPDRT_REQUIRE(np >= 1 && nout >= 1, "neval_pfrt, neval_out >= 1");
    HIPDRT_REQUIRE(np <= 2048 && nout <= 2048, "predict_pfrt: at most 2048 points on either grid");
    HIPDRT_REQUIRE(o.smooth || nout == np, "without smoothing the PFRT stays on the tau_pfrt grid: neval_out == neval_pfrt");
    HIPDRT_REQUIRE(o.search >= -1 && o.search <= 1, "search must be 1, -1 or 0 (two passes)");
    HIPDRT_REQUIRE(std::isfinite(o.height) && std::isfinite(o.prominence), "height and prominence must be finite");
    HIPDRT_REQUIRE(std::isfinite(o.prior_mu) && o.prior_sigma > 0.0 && std::isfinite(o.prior_sigma), "prior_mu finite, prior_sigma > 0");
    HIPDRT_REQUIRE(std::isfinite(o.n_eff_factor), "n_eff_factor must be finite");
    HIPDRT_REQUIRE(std::isfinite(o.fxx_var_floor), "fxx_var_floor must be finite");
    HIPDRT_REQUIRE(o.ext_left >= -1 && o.ext_left < np && o.ext_right >= -1 && o.ext_right < np,
                   "ext_left and ext_right: an index of the tau_pfrt grid, or -1");
    HIPDRT_REQUIRE(!o.smooth || (o.smooth_order > 0.0 && std::isfinite(o.smooth_order) && o.smooth_epsilon > 0.0 &&
                                 std::isfinite(o.smooth_epsilon)), "smooth_order, smooth_epsilon > 0");
    HIPDRT_REQUIRE(!o.integrate || std::isfinite(o.integrate_threshold), "integrate_threshold must be finite");
    return HIPDRT_OK;
}

int launch_pfrt_combine(hipStream_t s, const PfrtCombineArgs& a, int B) {
    HIPDRT_REQUIRE(B >= 1 && a.S >= 1 && a.S <= 1024, "pfrt_combine: B >= 1, 1 <= steps <= 1024");
    HIPDRT_REQUIRE(a.np >= 1 && a.nout >= 1 && a.np <= 2048 && a.nout <= 2048, "pfrt_combine: 1 ... 2048 points on either grid");
    HIPDRT_REQUIRE(a.smooth || a.nout == a.np, "pfrt_combine: without smoothing neval_out == neval_pfrt");
    HIPDRT_REQUIRE(a.step_pfrt && a.rss && a.slw && a.ln_factors && a.ltp && (a.lto || !a.smooth), "pfrt_combine: NULL input");
    const size_t lds = pfrt_combine_lds_bytes(a.S, a.np, a.nout);
    if (int rc = set_lds(reinterpret_cast<const void*>(pfrt_combine_kernel), lds, "pfrt_combine_kernel")) return rc;
    hipLaunchKernelGGL(pfrt_combine_kernel, dim3(B), dim3(PKT), lds, s, a);
    return HIPDRT_OK;
}

}  // namespace hipdrt
