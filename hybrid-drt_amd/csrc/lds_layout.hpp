// Dynamic-LDS layouts of the one-workgroup-per-spectrum kernels, each stated once: the kernel calls its layout function with the
// base of its `extern __shared__` array and uses the region pointers, the launcher calls the same function with a null base and
// requests `.bytes`.  Plain arithmetic without a HIP type in it, so that the stand-alone host program tests/c/lds_layout_host.cpp can
// carve a heap buffer of exactly `.bytes` with every layout under a sanitizer.
//
// A new kernel adds: a struct of its region pointers plus `bytes`, and a function that takes the regions off an LdsCarver in
// order.  Shapes come in as the ints the kernel already has; padded lengths (p2, ld, ldg) are computed once by the launcher with
// the helpers below and reach the kernel through its argument struct.
#pragma once
#include <cstddef>

#if defined(__HIPCC__)
#define HIPDRT_HD __host__ __device__
#else
#define HIPDRT_HD
#endif

namespace hipdrt {

// A base and a running byte offset.  take<T>(count) rounds the offset up to alignof(T), returns that position and advances by count
// elements; count == 0 returns the current position (an absent region aliases its successor).  The base of a dynamic LDS segment is
// 16-byte aligned, so an offset that is a multiple of alignof(T) is an aligned pointer.
#if defined(__HIP_DEVICE_COMPILE__)
// an LDS address has 32 bits: the kernel forms its offsets in int arithmetic, as the hand-written prologues did (with 64-bit offsets
// hyper_kernel, which sits at exactly 128 VGPRs, spills two of them)
typedef int lds_size_t;
#else
typedef size_t lds_size_t;
#endif
struct LdsCarver {
    char* base;
    lds_size_t off = 0;
    template <class T>
    HIPDRT_HD T* take(lds_size_t count) {
        off = (off + alignof(T) - 1) & ~(lds_size_t)(alignof(T) - 1);
        const lds_size_t at = off;
        off += count * (lds_size_t)sizeof(T);
#if defined(__HIP_DEVICE_COMPILE__)
        return reinterpret_cast<T*>(base + at);
#else
        return base ? reinterpret_cast<T*>(base + at) : nullptr;      // null base: the sizing pass, only `off` matters
#endif
    }
};
HIPDRT_HD inline LdsCarver lds_carver(void* base) { return LdsCarver{static_cast<char*>(base)}; }
// entry i of region p, for a declared overlay (null in the sizing pass)
template <class T>
HIPDRT_HD inline T* lds_at(T* p, lds_size_t i) {
#if defined(__HIP_DEVICE_COMPILE__)
    return p + i;
#else
    return p ? p + i : nullptr;
#endif
}

// ---- padded lengths the layouts are given ----
// the length lds_sort needs for n values: the next power of two, at least 2
HIPDRT_HD inline int next_pow2(int n) {
    int p2 = 2;
    while (p2 < n) p2 <<= 1;
    return p2;
}
// kk_kernel sorts the 2 nf residuals of a spectrum
HIPDRT_HD inline int kk_p2(int nf) { return next_pow2(2 * nf); }
// peak_resolve_kernel: leading dimension of the xw rows (a multiple of 4 that is 4 mod 32) and of the gamma rows
HIPDRT_HD inline int peak_resolve_ld(int nb) {
    int ld = (nb + 3) & ~3;
    while (ld % 32 != 4) ld += 4;
    return ld;
}
HIPDRT_HD inline int pr_ldg(int nout) {
    int l = (nout + 15) & ~15;
    if (l % 32 == 0) l += 16;      // rows 32 banks apart: the four accumulator rows a wavefront writes at once alternate halves
    return l;
}

// ---- hyper.hip ----
// hyper_kernel's forms (hyper_lds_form decides which one a problem gets; FitState::toeplitz_m carries 0, 1 or 2 to the kernel):
//   HYPER_ROWS     the general row-streaming form.  A problem that is not Toeplitz to begin with still gets the column slot of
//                  HYPER_BESIDE, unused -- a quirk of long standing that the byte counts hipdrt_debug_hyper_form reports include
//   HYPER_BESIDE   the mirrored Toeplitz columns [3][2 nd - 1] behind the two m-vectors
//   HYPER_INSIDE   the columns inside the second m-vector (large joint fits), see below
//   HYPER_DEMOTED  host side only: a Toeplitz problem for which neither column form fits runs as HYPER_ROWS without the slot (the
//                  kernel sees form 0 and, there being no outlier vectors in a demoted problem, touches nothing behind tmp2)
enum { HYPER_ROWS = 0, HYPER_BESIDE = 1, HYPER_INSIDE = 2, HYPER_DEMOTED = 3 };
struct HyperLds {
    double *xs, *bsum, *gdia, *sq, *xh;      // x [n]; then [nd] each (nd = n - ns)
    double *tmp, *tmp2;                      // [max(m, nd)] each (tmp2 longer in HYPER_INSIDE)
    double *ctp;                             // [3][2 nd - 1]
    double *tmp3;                            // [2][m], outlier_p > 0 only
    size_t bytes;
};
HIPDRT_HD inline HyperLds hyper_lds(void* sm, int n, int m, int ns, int form, bool outlier) {
    const int nd = n - ns, tl = m > nd ? m : nd, cols = 3 * (2 * nd - 1);
    LdsCarver c = lds_carver(sm);
    HyperLds l;
    l.xs = c.take<double>(n);
    l.bsum = c.take<double>(nd);
    l.gdia = c.take<double>(nd);
    l.sq = c.take<double>(nd);
    l.xh = c.take<double>(nd);
    l.tmp = c.take<double>(tl);
    // the one overlay, HYPER_INSIDE: the columns start behind the nd entries of tmp2 that the Toeplitz phases use and overlap
    // tmp2[nd ..) on purpose -- the weights phase, which needs all m entries of tmp2, comes after the last use of the columns.  tmp2
    // is then max(tl, nd + cols) long (its tail is taken separately, so that the kernel sees the columns at tmp2 + nd or at
    // tmp2 + tl and nothing else), and no slot follows it
    const bool inside = form == HYPER_INSIDE;
    l.tmp2 = c.take<double>(tl);
    c.take<double>(inside || form == HYPER_DEMOTED ? 0 : cols);
    c.take<double>(inside && nd + cols > tl ? nd + cols - tl : 0);
    l.ctp = lds_at(l.tmp2, inside ? nd : tl);      // the slot just taken, or nd entries into tmp2
    l.tmp3 = c.take<double>(outlier ? 2 * m : 0);
    l.bytes = c.off;
    return l;
}

// init_weights_kernel: x [n], two row vectors [m], two more only for the outlier branch
struct InitWeightsLds { double *xs, *tmp, *tmp2, *tmp3, *tmp4; size_t bytes; };
HIPDRT_HD inline InitWeightsLds init_weights_lds(void* sm, int n, int m, bool outlier) {
    LdsCarver c = lds_carver(sm);
    InitWeightsLds l;
    l.xs = c.take<double>((size_t)n);
    l.tmp = c.take<double>((size_t)m);
    l.tmp2 = c.take<double>((size_t)m);
    l.tmp3 = c.take<double>(outlier ? (size_t)m : 0);
    l.tmp4 = c.take<double>(outlier ? (size_t)m : 0);
    l.bytes = c.off;
    return l;
}

// llh_kernel: x [n]; rm @ x, residual^2, vmm @ residual^2 [m each]
struct LlhLds { double *xs, *yh, *r2, *sh; size_t bytes; };
HIPDRT_HD inline LlhLds llh_lds(void* sm, int n, int m) {
    LdsCarver c = lds_carver(sm);
    LlhLds l;
    l.xs = c.take<double>((size_t)n);
    l.yh = c.take<double>((size_t)m);
    l.r2 = c.take<double>((size_t)m);
    l.sh = c.take<double>((size_t)m);
    l.bytes = c.off;
    return l;
}

// ---- lml.hip ----
// lml_sums_kernel: x [n], sqrt(s_k) x of the order at hand [n], rm @ x [m]
struct LmlLds { double *xs, *vs, *yh; size_t bytes; };
HIPDRT_HD inline LmlLds lml_lds(void* sm, int n, int m) {
    LdsCarver c = lds_carver(sm);
    LmlLds l;
    l.xs = c.take<double>((size_t)n);
    l.vs = c.take<double>((size_t)n);
    l.yh = c.take<double>((size_t)m);
    l.bytes = c.off;
    return l;
}

// ---- kk.hip ----
// kk_kernel: residuals [nf each], the sort buffer [p2 = kk_p2(nf)], the mask [nf ints; the doubles behind it start on the next
// even count], and for stage A x [n] and the prediction [m = 2 nf]
struct KkLds { double *er, *ei, *srt; int* mask; double *xs, *yh; size_t bytes; };
HIPDRT_HD inline KkLds kk_lds(void* sm, int nf, int p2, int n, int stage_a) {
    LdsCarver c = lds_carver(sm);
    KkLds l;
    l.er = c.take<double>((size_t)nf);
    l.ei = c.take<double>((size_t)nf);
    l.srt = c.take<double>((size_t)p2);
    l.mask = c.take<int>((size_t)nf);
    l.xs = c.take<double>(stage_a ? (size_t)n : 0);
    l.yh = c.take<double>(stage_a ? 2 * (size_t)nf : 0);
    l.bytes = c.off;
    return l;
}

// ---- peaks.hip ----
// peaks_kernel: rows of one spectrum -- doubles fxx, prom, [f], [vxx, prob], [vf], [srt p2]; ints sgn, lb, rb.  The flags say which
// of the optional rows exist (need_f: search = 0 or method = 2); an absent row has length zero
struct PeaksLds {
    int f, var, varf, sort;
    double *fxx, *prom, *frow, *vxx, *prob, *vf, *srt;
    int *sgn, *lb, *rb;
    size_t bytes;
};
HIPDRT_HD inline PeaksLds peaks_lds(void* sm, int neval, int p2, int method, int need_f, int num_peaks) {
    const size_t n = (size_t)neval;
    LdsCarver c = lds_carver(sm);
    PeaksLds l;
    l.f = need_f; l.var = method >= 1; l.varf = method == 2; l.sort = method == 1 && num_peaks > 0;
    l.fxx = c.take<double>(n);
    l.prom = c.take<double>(n);
    l.frow = c.take<double>(l.f ? n : 0);
    l.vxx = c.take<double>(l.var ? n : 0);
    l.prob = c.take<double>(l.var ? n : 0);
    l.vf = c.take<double>(l.varf ? n : 0);
    l.srt = c.take<double>(l.sort ? (size_t)p2 : 0);
    l.sgn = c.take<int>(n);
    l.lb = c.take<int>(n);
    l.rb = c.take<int>(n);
    l.bytes = c.off;
    return l;
}

// ---- peak_prob.hip ----
// peak_trough_prob_kernel: the three mean rows [n each], the three sigma rows [3 n], the work / sort row [p2]; ints sgn, lb, rb
struct PeakProbLds { double *m0, *m1, *m2, *s0, *w; int *sgn, *lb, *rb; size_t bytes; };
HIPDRT_HD inline PeakProbLds peak_prob_lds(void* sm, int neval, int p2) {
    const size_t n = (size_t)neval;
    LdsCarver c = lds_carver(sm);
    PeakProbLds l;
    l.m0 = c.take<double>(n);
    l.m1 = c.take<double>(n);
    l.m2 = c.take<double>(n);
    l.s0 = c.take<double>(3 * n);
    l.w = c.take<double>((size_t)p2);
    l.sgn = c.take<int>(n);
    l.lb = c.take<int>(n);
    l.rb = c.take<int>(n);
    l.bytes = c.off;
    return l;
}

// ---- peak_resolve.hip ----
// peak_resolve_kernel: doubles f, fxx [nfind], xw [Pt * 16][ld] (Pt tiles of 16 peaks), gam [16][ldg] (nout > 0), eps_l, eps_r,
// rco, rpk [max_peaks each]; ints pk, tr [max_peaks], scan [one per thread]
static constexpr int PR_THREADS = 256;
struct PeakResolveLds { double *f, *fxx, *xw, *gam, *epsl, *epsr, *rco, *rpk; int *pk, *tr, *scan; size_t bytes; };
HIPDRT_HD inline PeakResolveLds peak_resolve_lds(void* sm, int nfind, int ld, int ldg, int nout, int max_peaks) {
    const size_t n = (size_t)nfind, mp = (size_t)max_peaks, ptiles = (mp + 15) / 16;
    LdsCarver c = lds_carver(sm);
    PeakResolveLds l;
    l.f = c.take<double>(n);
    l.fxx = c.take<double>(n);
    l.xw = c.take<double>(ptiles * 16 * (size_t)ld);
    l.gam = c.take<double>(nout > 0 ? 16 * (size_t)ldg : 0);
    l.epsl = c.take<double>(mp);
    l.epsr = c.take<double>(mp);
    l.rco = c.take<double>(mp);
    l.rpk = c.take<double>(mp);
    l.pk = c.take<int>(mp);
    l.tr = c.take<int>(mp);
    l.scan = c.take<int>((size_t)PR_THREADS);
    l.bytes = c.off;
    return l;
}

// ---- pfrt.hip ----
// pfrt_combine_kernel: the accumulator and ln(tau_pfrt) [np], ln(tau_out), the smoothed row and the integrated row [nout], the
// steps' posterior weights [S]
struct PfrtCombineLds { double *acc, *ltp, *lto, *v, *res, *post; size_t bytes; };
HIPDRT_HD inline PfrtCombineLds pfrt_combine_lds(void* sm, int S, int np, int nout) {
    LdsCarver c = lds_carver(sm);
    PfrtCombineLds l;
    l.acc = c.take<double>((size_t)np);
    l.ltp = c.take<double>((size_t)np);
    l.lto = c.take<double>((size_t)nout);
    l.v = c.take<double>((size_t)nout);
    l.res = c.take<double>((size_t)nout);
    l.post = c.take<double>((size_t)S);
    l.bytes = c.off;
    return l;
}

// pfrt_select_kernel: the raw PFRT, one step row and its shifted image [np each]; per range its area, its magnitude and the
// running best match_quality [max_peaks each]; ints: per grid point the range it belongs to (its end included) and rank_at [np
// each] -- rank_at first holds the flag "a range starts here" for the count of the ranges, and from then on the rank of the peak
// that sits at the point (INT_MAX: none); per range start, end, peak, rank -> range and the running best step [max_peaks each],
// and the counts {ranges, first, candidates}
static constexpr int PFS_MAX_PEAKS = 64;
struct PfrtSelectLds {
    double *raw, *row, *sh, *area, *mag, *best;
    int *rng, *rank_at, *start, *end, *peak, *order, *best_step, *counts;
    size_t bytes;
};
HIPDRT_HD inline PfrtSelectLds pfrt_select_lds(void* sm, int np, int max_peaks) {
    const size_t n = (size_t)np, mp = (size_t)max_peaks;
    LdsCarver c = lds_carver(sm);
    PfrtSelectLds l;
    l.raw = c.take<double>(n);
    l.row = c.take<double>(n);
    l.sh = c.take<double>(n);
    l.area = c.take<double>(mp);
    l.mag = c.take<double>(mp);
    l.best = c.take<double>(mp);
    l.rng = c.take<int>(n);
    l.rank_at = c.take<int>(n);
    l.start = c.take<int>(mp);
    l.end = c.take<int>(mp);
    l.peak = c.take<int>(mp);
    l.order = c.take<int>(mp);
    l.best_step = c.take<int>(mp);
    l.counts = c.take<int>(4);
    l.bytes = c.off;
    return l;
}

// ---- map_predict.hip ----
// map_prob_kernel: five double rows and three int rows of n evaluation points
struct MapProbLds { double *f, *fxx, *vf, *vxx, *prom; int *sgn, *lb, *rb; size_t bytes; };
HIPDRT_HD inline MapProbLds map_prob_lds(void* sm, int n_) {
    const size_t n = (size_t)(n_ > 0 ? n_ : 0);
    LdsCarver c = lds_carver(sm);
    MapProbLds l;
    l.f = c.take<double>(n);
    l.fxx = c.take<double>(n);
    l.vf = c.take<double>(n);
    l.vxx = c.take<double>(n);
    l.prom = c.take<double>(n);
    l.sgn = c.take<int>(n);
    l.lb = c.take<int>(n);
    l.rb = c.take<int>(n);
    l.bytes = c.off;
    return l;
}

// ---- map_rank.hip ----
// rank_kernel (256 threads): the window of a tile of RT_R x RT_C outputs, and per thread a selection buffer of the sr * sc window
// entries (entry k of thread t at sel[k * 256 + t])
constexpr int RT_R = 16, RT_C = 64;        // outputs of a tile: 4 per thread
struct RankLds { double *win, *sel; size_t bytes; };
HIPDRT_HD inline RankLds rank_lds(void* sm, int sr, int sc) {
    LdsCarver c = lds_carver(sm);
    RankLds l;
    l.win = c.take<double>((size_t)(RT_R + sr - 1) * (RT_C + sc - 1));
    l.sel = c.take<double>((size_t)256 * sr * sc);
    l.bytes = c.off;
    return l;
}

// ---- matrices.hip ----
// the trapezoid kernels' y tables (stage_y_tables): ys, phis, eys [ny each]
struct YTablesLds { double *ys, *phis, *eys; size_t bytes; };
HIPDRT_HD inline YTablesLds y_tables_lds(void* sm, int ny) {
    LdsCarver c = lds_carver(sm);
    YTablesLds l;
    l.ys = c.take<double>((size_t)ny);
    l.phis = c.take<double>((size_t)ny);
    l.eys = c.take<double>((size_t)ny);
    l.bytes = c.off;
    return l;
}
// impedance_interp_kernel: the knots of the Z' and Z'' lookups [npad each, npad = ng rounded up to even], their (value, slope)
// pairs [ng each, 16 bytes a pair], and ln(omega) of the workgroup's rows [rpb].  The rows start 6 npad doubles in, as if the
// pairs were padded like the knots: for odd ng two doubles behind the pairs are unused.
struct alignas(16) LdsPair { double v, s; };
struct ImpedanceInterpLds { double *x_re, *x_im; LdsPair *fs_re, *fs_im; double *pad, *slw; size_t bytes; };
HIPDRT_HD inline ImpedanceInterpLds impedance_interp_lds(void* sm, int ng, int rpb) {
    const size_t npad = (size_t)(ng + (ng & 1));
    LdsCarver c = lds_carver(sm);
    ImpedanceInterpLds l;
    l.x_re = c.take<double>(npad);
    l.x_im = c.take<double>(npad);
    l.fs_re = c.take<LdsPair>((size_t)ng);
    l.fs_im = c.take<LdsPair>((size_t)ng);
    l.pad = c.take<double>(4 * (npad - (size_t)ng));
    l.slw = c.take<double>((size_t)rpb);
    l.bytes = c.off;
    return l;
}
// response_interp_kernel: the response lookup {log_td, v, slope} [ng each], an image of lut3
struct ResponseInterpLds { double *xp, *fp, *sl; size_t bytes; };
HIPDRT_HD inline ResponseInterpLds response_interp_lds(void* sm, int ng) {
    LdsCarver c = lds_carver(sm);
    ResponseInterpLds l;
    l.xp = c.take<double>((size_t)ng);
    l.fp = c.take<double>((size_t)ng);
    l.sl = c.take<double>((size_t)ng);
    l.bytes = c.off;
    return l;
}

}  // namespace hipdrt
