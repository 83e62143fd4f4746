// Stand-alone host program (its own main, no GPU, no Python): every dynamic-LDS layout of csrc/lds_layout.hpp carved out of a heap
// buffer of exactly the `.bytes` its launcher requests.  Meant to be compiled with -fsanitize=address,undefined
// (tests/test_lds_layout_host.py does): a region that reaches past the request is a heap overflow the sanitizer reports when the
// region is filled, an overlap nobody declared shows as a wrong tag in the read-back, and `.bytes` is compared with the value the
// hand-written sums gave before the layouts existed.  Exit status 0 = all checks passed.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "lds_layout.hpp"

using namespace hipdrt;

static int failures = 0;
static const char* current = "";
#define EXPECT(cond, ...)                                            \
    do {                                                             \
        if (!(cond)) {                                               \
            ++failures;                                              \
            std::printf("FAIL %s: %s -- ", current, #cond);          \
            std::printf(__VA_ARGS__);                                \
            std::printf("\n");                                       \
        }                                                            \
    } while (0)

struct Region {
    const char* name;
    void* p;
    size_t elem, count, align;
    bool overlay;      // lies inside another region on purpose: bounds only, filled last
};
#define R(L, member, count) Region{#member, (void*)(L).member, sizeof(*(L).member), (size_t)(count), alignof(decltype(*(L).member)), false}
#define OVERLAY(L, member, count) Region{#member, (void*)(L).member, sizeof(*(L).member), (size_t)(count), alignof(decltype(*(L).member)), true}

// carve(base) -> the layout struct; regions(L) -> its regions in carving order, with the lengths the kernel uses
template <class Carve, class Regions>
static void run(const char* what, size_t pinned, Carve carve, Regions regions) {
    current = what;
    const size_t bytes = carve(nullptr).bytes;
    EXPECT(bytes == pinned, "%zu bytes, %zu pinned", bytes, pinned);
    void* buf = nullptr;
    if (posix_memalign(&buf, 16, bytes) != 0 || !buf) { EXPECT(false, "allocation of %zu bytes", bytes); return; }
    char* const b0 = static_cast<char*>(buf);
    const auto L = carve(buf);
    EXPECT(L.bytes == bytes, "%zu bytes with a base, %zu without", (size_t)L.bytes, bytes);
    const std::vector<Region> rs = regions(L);
    // aligned, inside the buffer, each plain region where the one before it ends (rounded up to its alignment), the last one
    // ending at `bytes`
    size_t end = 0;
    for (const Region& r : rs) {
        const size_t at = (size_t)(static_cast<char*>(r.p) - b0), len = r.elem * r.count;
        EXPECT((uintptr_t)r.p % r.align == 0, "%s is not aligned to %zu", r.name, r.align);
        EXPECT(at <= bytes && len <= bytes - at, "%s [%zu, %zu) leaves the %zu bytes", r.name, at, at + len, bytes);
        if (r.overlay) continue;
        const size_t want = (end + r.align - 1) / r.align * r.align;
        EXPECT(at == want, "%s starts at %zu, the region before it ends at %zu", r.name, at, end);
        end = at + len;
    }
    EXPECT(end == bytes, "the last region ends at %zu of %zu bytes", end, bytes);
    // every plain region filled over its full extent with its own tag, then all of them read back
    for (size_t i = 0; i < rs.size(); ++i)
        if (!rs[i].overlay) std::memset(rs[i].p, (int)(i + 1), rs[i].elem * rs[i].count);
    for (size_t i = 0; i < rs.size(); ++i) {
        if (rs[i].overlay) continue;
        const unsigned char* p = static_cast<const unsigned char*>(rs[i].p);
        size_t bad = 0;
        for (size_t k = 0; k < rs[i].elem * rs[i].count; ++k) bad += p[k] != (unsigned char)(i + 1);
        EXPECT(bad == 0, "%zu bytes of %s carry another region's tag", bad, rs[i].name);
    }
    for (const Region& r : rs)
        if (r.overlay) std::memset(r.p, 0xEE, r.elem * r.count);
    std::free(buf);
}

static void hyper(const char* what, int n, int m, int ns, int form, bool outlier, size_t pinned) {
    const size_t nd = (size_t)(n - ns), tl = (size_t)m > nd ? (size_t)m : nd, cols = 3 * (2 * nd - 1);
    run(what, pinned, [&](void* b) { return hyper_lds(b, n, m, ns, form, outlier); },
        [&](const HyperLds& L) {
            std::vector<Region> r = {R(L, xs, n), R(L, bsum, nd), R(L, gdia, nd), R(L, sq, nd), R(L, xh, nd), R(L, tmp, tl)};
            if (form == HYPER_INSIDE) {
                // the declared overlay: the columns start at tmp2 + nd and end inside the (possibly lengthened) second vector
                const size_t second = tl > nd + cols ? tl : nd + cols;
                r.push_back(R(L, tmp2, second));
                r.push_back(OVERLAY(L, ctp, cols));
                EXPECT(L.ctp == L.tmp2 + nd, "the columns start %td doubles into tmp2, not %zu", L.ctp - L.tmp2, nd);
                EXPECT(nd + cols <= second, "the columns end past tmp2");
            } else {
                r.push_back(R(L, tmp2, tl));
                r.push_back(R(L, ctp, form == HYPER_DEMOTED ? 0 : cols));
            }
            r.push_back(R(L, tmp3, outlier ? 2 * (size_t)m : 0));
            return r;
        });
}

static void init_weights(int n, int m, bool outlier, size_t pinned) {
    run("init_weights", pinned, [&](void* b) { return init_weights_lds(b, n, m, outlier); },
        [&](const InitWeightsLds& L) {
            const size_t o = outlier ? m : 0;
            return std::vector<Region>{R(L, xs, n), R(L, tmp, m), R(L, tmp2, m), R(L, tmp3, o), R(L, tmp4, o)};
        });
}

static void llh(int n, int m, size_t pinned) {
    run("llh", pinned, [&](void* b) { return llh_lds(b, n, m); },
        [&](const LlhLds& L) { return std::vector<Region>{R(L, xs, n), R(L, yh, m), R(L, r2, m), R(L, sh, m)}; });
}

static void kk(int nf, int n, int stage_a, size_t pinned) {
    run("kk", pinned, [&](void* b) { return kk_lds(b, nf, kk_p2(nf), n, stage_a); },
        [&](const KkLds& L) {
            return std::vector<Region>{R(L, er, nf), R(L, ei, nf), R(L, srt, kk_p2(nf)), R(L, mask, nf), R(L, xs, stage_a ? n : 0),
                                       R(L, yh, stage_a ? 2 * nf : 0)};
        });
}

static void peaks(int neval, int method, int need_f, int num_peaks, size_t pinned) {
    const int p2 = next_pow2(neval);
    run("peaks", pinned, [&](void* b) { return peaks_lds(b, neval, p2, method, need_f, num_peaks); },
        [&](const PeaksLds& L) {
            const size_t n = neval;
            EXPECT(L.f == need_f && L.var == (method >= 1) && L.varf == (method == 2) && L.sort == (method == 1 && num_peaks > 0),
                   "flags %d %d %d %d", L.f, L.var, L.varf, L.sort);
            // an absent row has length zero and starts where its successor does
            return std::vector<Region>{R(L, fxx, n), R(L, prom, n), R(L, frow, need_f ? n : 0), R(L, vxx, method >= 1 ? n : 0),
                                       R(L, prob, method >= 1 ? n : 0), R(L, vf, method == 2 ? n : 0),
                                       R(L, srt, method == 1 && num_peaks > 0 ? p2 : 0), R(L, sgn, n), R(L, lb, n), R(L, rb, n)};
        });
}

static void peak_prob(int neval, size_t pinned) {
    const int p2 = next_pow2(neval);
    run("peak_prob", pinned, [&](void* b) { return peak_prob_lds(b, neval, p2); },
        [&](const PeakProbLds& L) {
            const size_t n = neval;
            return std::vector<Region>{R(L, m0, n), R(L, m1, n), R(L, m2, n), R(L, s0, 3 * n), R(L, w, p2), R(L, sgn, n), R(L, lb, n),
                                       R(L, rb, n)};
        });
}

static void peak_resolve(int nfind, int nb, int nout, int mp, size_t pinned, int want_ldg = -1) {
    const int ld = peak_resolve_ld(nb), ldg = pr_ldg(nout);
    current = "peak_resolve";
    EXPECT(ld >= nb && ld % 32 == 4, "ld = %d for nb = %d", ld, nb);
    if (want_ldg >= 0) EXPECT(ldg == want_ldg, "ldg = %d for nout = %d, %d expected", ldg, nout, want_ldg);
    run("peak_resolve", pinned, [&](void* b) { return peak_resolve_lds(b, nfind, ld, ldg, nout, mp); },
        [&](const PeakResolveLds& L) {
            const size_t pt = ((size_t)mp + 15) / 16;
            return std::vector<Region>{R(L, f, nfind), R(L, fxx, nfind), R(L, xw, pt * 16 * ld), R(L, gam, nout > 0 ? 16 * ldg : 0),
                                       R(L, epsl, mp), R(L, epsr, mp), R(L, rco, mp), R(L, rpk, mp), R(L, pk, mp), R(L, tr, mp),
                                       R(L, scan, PR_THREADS)};
        });
}

static void pfrt_combine(int S, int np, int nout, size_t pinned) {
    run("pfrt_combine", pinned, [&](void* b) { return pfrt_combine_lds(b, S, np, nout); },
        [&](const PfrtCombineLds& L) {
            return std::vector<Region>{R(L, acc, np), R(L, ltp, np), R(L, lto, nout), R(L, v, nout), R(L, res, nout), R(L, post, S)};
        });
}

static void map_prob(int n, size_t pinned) {
    run("map_prob", pinned, [&](void* b) { return map_prob_lds(b, n); },
        [&](const MapProbLds& L) {
            return std::vector<Region>{R(L, f, n), R(L, fxx, n), R(L, vf, n), R(L, vxx, n), R(L, prom, n), R(L, sgn, n), R(L, lb, n),
                                       R(L, rb, n)};
        });
}

static void rank(int sr, int sc, size_t pinned) {
    run("rank", pinned, [&](void* b) { return rank_lds(b, sr, sc); },
        [&](const RankLds& L) {
            return std::vector<Region>{R(L, win, (size_t)(RT_R + sr - 1) * (RT_C + sc - 1)), R(L, sel, (size_t)256 * sr * sc)};
        });
}

static void y_tables(int ny) {
    run("y_tables", 3 * (size_t)ny * 8, [&](void* b) { return y_tables_lds(b, ny); },
        [&](const YTablesLds& L) { return std::vector<Region>{R(L, ys, ny), R(L, phis, ny), R(L, eys, ny)}; });
}

static void impedance_interp(int ng, int rpb) {
    // what the launch argument was: (6 * (ngrid + (ngrid & 1)) + rpb) doubles
    const size_t npad = (size_t)(ng + (ng & 1));
    run("impedance_interp", (6 * npad + (size_t)rpb) * 8, [&](void* b) { return impedance_interp_lds(b, ng, rpb); },
        [&](const ImpedanceInterpLds& L) {
            EXPECT((char*)L.slw - (char*)L.x_re == (ptrdiff_t)(6 * npad * 8), "the rows start 6 npad doubles in");
            EXPECT(L.fs_im == L.fs_re + ng, "the Z'' pairs follow the Z' pairs");
            return std::vector<Region>{R(L, x_re, npad), R(L, x_im, npad), R(L, fs_re, ng), R(L, fs_im, ng), R(L, pad, 4 * (npad - ng)),
                                       R(L, slw, rpb)};
        });
}

static void response_interp(int ng) {
    run("response_interp", 3 * (size_t)ng * 8, [&](void* b) { return response_interp_lds(b, ng); },
        [&](const ResponseInterpLds& L) { return std::vector<Region>{R(L, xp, ng), R(L, fp, ng), R(L, sl, ng)}; });
}

int main() {
    // hyper_kernel: (n, m, ns) in the form hyper_lds_form gives a (toeplitz, outlier) problem of that shape
    hyper("hyper form 1", 66, 24, 2, HYPER_BESIDE, false, 6648);
    hyper("hyper form 0, not Toeplitz: slot kept", 66, 24, 2, HYPER_ROWS, false, 6648);
    hyper("hyper form 1, outlier", 66, 24, 2, HYPER_BESIDE, true, 7032);
    hyper("hyper form 2", 1502, 2000, 2, HYPER_INSIDE, false, 159992);
    hyper("hyper form 2, columns end inside the m-vector", 822, 5760, 2, HYPER_INSIDE, false, 124976);
    hyper("hyper form 0, demoted", 1702, 2000, 2, HYPER_DEMOTED, false, 100016);
    hyper("hyper form 1, outlier, refused", 1502, 2000, 2, HYPER_BESIDE, true, 195992);
    hyper("hyper nd = 1", 3, 1, 2, HYPER_BESIDE, false, 96);
    init_weights(66, 24, false, 912);
    init_weights(66, 24, true, 1296);
    llh(66, 24, 1104);
    llh(1078, 5120, 131504);
    kk(1, 0, 0, 40);
    kk(7, 0, 0, 272);
    kk(12, 66, 1, 1216);
    kk(13, 66, 1, 1256);      // odd nf: the mask padding
    kk(4096, 0, 0, 147456);
    peaks(1, 0, 0, 0, 28);
    peaks(91, 0, 1, 0, 3276);
    peaks(91, 1, 0, 3, 5028);
    peaks(91, 1, 0, 0, 4004);
    peaks(91, 2, 1, 0, 5460);
    peaks(257, 1, 1, 5, 17460);
    peak_prob(1, 76);
    peak_prob(3, 212);
    peak_prob(91, 6484);
    peak_prob(257, 19516);
    peak_resolve(1, 1, 0, 1, 1592);
    peak_resolve(91, 71, 0, 16, 15920);
    peak_resolve(91, 71, 91, 17, 43096);
    peak_resolve(91, 71, 32, 3, 21544, 48);      // ldg bumped from 32 to 48
    peak_resolve(1000, 1024, 0, 16, 149248);
    pfrt_combine(1, 1, 1, 48);
    pfrt_combine(5, 91, 71, 3200);
    map_prob(1, 52);
    map_prob(1260, 65520);
    map_prob(1261, 65572);
    map_prob(3145, 163540);      // the last that fits
    map_prob(3146, 163592);      // the first refused
    rank(1, 1, 10240);
    rank(3, 3, 27936);
    rank(5, 7, 82880);
    y_tables(1);
    y_tables(1000);
    impedance_interp(2000, 256);
    impedance_interp(1001, 4);
    impedance_interp(3406, 4);
    response_interp(2000);
    response_interp(6816);
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("lds layouts ok\n");
    return 0;
}
