// Coherent re-optimisation of neighbouring observations (hybdrt/mapping/resolve.py:176-341 under DRTMD.resolve_group,
// hybdrt/mapping/drtmd.py:432-559): the coupled QPs of a fitted prepared batch, assembled where the members' final P and q already
// are.  resolve_p_kernel writes every coupled P_k straight into the lower 16 x 16 tiles the coneqp launchers read (pack_p_kernel's
// layout, gram.hip), resolve_q_kernel the q_k; hipdrt_plan_resolve_group then solves all batches of one size in one launch_qp.
// Built with -ffp-contract=off: param_scale * my * lambda_psi, the one add onto a member's entry and q's short sum round as numpy's.
#include <cmath>
#include <cstring>

#include "debug_guard.hpp"
#include "plan.hpp"

namespace hipdrt {
namespace {

// where a member's P and q lie (doubles from the kernels' P and q pointers) and which slots of the supergrid its DRT block covers
struct ResolveMember { long long p_off, q_off; int ld, left, right, pad; };
// one coupled batch: its outputs (doubles from Ppk and qk), its param_scale row, its first member, the left end of its common
// range and its unknowns per member
struct ResolveBatch { long long ppk_off, q_off, ps_off; int first, mleft, nc, pad; };
struct ResolveAsm {
    int nr, num_remove, so;
    double lambda_psi;
    const ResolveMember* mem;
    const ResolveBatch* bat;
    const double *P, *q;          // the members' matrices and vectors
    const double* my;             // [nb][nr][nr]
    const double* ps;             // param_scale rows, ResolveBatch::ps_off
    const double* xrm;            // [B][num_remove]
    double *Ppk, *qk;
};

// column c of a batch's member block -> that member's own unknown, or -1 where the member has no basis function there (resize_pq:
// the special unknowns keep their place, the DRT block is shifted by the distance between the two left ends and cut at either end)
__device__ __forceinline__ int resolve_src(const ResolveAsm& a, const ResolveMember& m, int mleft, int c) {
    if (c < a.so) return a.num_remove + c;
    const int s = c - a.so + mleft - m.left;
    return (s >= 0 && s < m.right - m.left) ? a.num_remove + a.so + s : -1;
}

// grid (ceil(nchp / 4), nchp, nb) for the largest batch: one workgroup per 64-column strip of one tile row, one wavefront per tile;
// every lower tile of the padded image is written, the padding with zeros
__global__ __launch_bounds__(256) void resolve_p_kernel(ResolveAsm a) {
    const ResolveBatch bt = a.bat[blockIdx.z];
    const int nc = bt.nc, nr = a.nr, n = nr * nc, nchp = ((n + 31) / 32) * 2;
    const int tr = blockIdx.y, tc = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (tr >= nchp || tc > tr) return;
    const double* my = a.my + (size_t)blockIdx.z * nr * nr;
    const double* ps = a.ps + bt.ps_off;
    double vals[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        int i = tr * 16 + (lane & 15), j = tc * 16 + (lane >> 4) + 4 * r;
        if (i < j) { const int t = i; i = j; j = t; }          // a diagonal tile: the mirror image of its lower half
        double v = 0.0;
        if (i < n) {
            const int bi = i / nc, ci = i - bi * nc, bj = j / nc, cj = j - bj * nc;
            if (ci == cj) v = (ps[ci] * my[bi * nr + bj]) * a.lambda_psi;
            if (bi == bj) {
                const ResolveMember m = a.mem[bt.first + bi];
                const int si = resolve_src(a, m, bt.mleft, ci), sj = resolve_src(a, m, bt.mleft, cj);
                v = v + ((si >= 0 && sj >= 0) ? a.P[m.p_off + (size_t)si * m.ld + sj] : 0.0);
            }
        }
        vals[r] = v;
    }
    double2* tile = reinterpret_cast<double2*>(a.Ppk + bt.ppk_off + ((size_t)tr * nchp + tc) * 256);
    const int fo = (lane & 15) * 4 + (lane >> 4);
    tile[fo] = make_double2(vals[0], vals[1]);
    tile[64 + fo] = make_double2(vals[2], vals[3]);
}

// grid (ceil(n / 256), nb) for the largest batch
__global__ __launch_bounds__(256) void resolve_q_kernel(ResolveAsm a) {
    const ResolveBatch bt = a.bat[blockIdx.y];
    const int nc = bt.nc, n = a.nr * nc, g = blockIdx.x * 256 + threadIdx.x;
    if (g >= n) return;
    const int bi = g / nc, ci = g - bi * nc;
    const ResolveMember m = a.mem[bt.first + bi];
    const int s = resolve_src(a, m, bt.mleft, ci);
    double v = 0.0;
    if (s >= 0) {
        const double* x = a.xrm + (size_t)(bt.first + bi) * a.num_remove;
        double acc = 0.0;
        for (int k = 0; k < a.num_remove; ++k) acc += x[k] * a.P[m.p_off + (size_t)k * m.ld + s];
        v = a.q[m.q_off + s] + acc;
    }
    a.qk[bt.q_off + g] = v;
}

// The host's account of one call: the batches in the order of their outputs -- all of one size behind each other, sizes in order of
// first appearance -- and where each lies.
struct ResolveSizeGroup { int nc, count; size_t first_slot; };
struct ResolveLayout {
    std::vector<ResolveBatch> bat;              // in the caller's order
    std::vector<ResolveSizeGroup> groups;
    std::vector<size_t> x_user;                 // doubles before batch k in the caller's x_out / q_out / h
    size_t ppk_total = 0, q_total = 0, ps_total = 0;
    int n_max = 0;
};

// every check of the description; member_n(b) = the unknowns of member b
template <class F>
int resolve_layout(const hipdrt_resolve_args& r, int B, F member_n, ResolveLayout& L) {
    HIPDRT_REQUIRE(r.nb >= 1 && r.nb <= kGridDimMax, "1 <= nb <= 65535");
    HIPDRT_REQUIRE(r.nr >= 1 && r.nr <= B, "1 <= nr <= members");
    HIPDRT_REQUIRE(r.num_remove >= 0 && r.so >= 0, "num_remove, so >= 0");
    HIPDRT_REQUIRE(r.first && r.match && r.tau_indices && r.my && r.param_scale, "NULL pointer in the description");
    HIPDRT_REQUIRE(r.num_remove == 0 || r.x_remove, "x_remove is NULL");
    HIPDRT_REQUIRE(std::isfinite(r.lambda_psi), "lambda_psi must be finite");
    if (r.tau_filter_sigma > 0.0 || r.special_filter_sigma > 0.0) {
        set_error("not supported: tau_filter_sigma / special_filter_sigma > 0 couple every unknown of a batch with every other; "
                  "assemble those problems on the host and solve them with hipdrt_qp_batch");
        return HIPDRT_E_UNSUPPORTED;
    }
    for (int b = 0; b < B; ++b) {
        const int left = r.tau_indices[2 * b], right = r.tau_indices[2 * b + 1];
        HIPDRT_REQUIRE(left >= 0 && right > left, "a member's tau range is empty or negative");
        HIPDRT_REQUIRE((long long)r.num_remove + r.so + (right - left) == member_n(b), "a member's tau range does not match its unknowns");
    }
    L.bat.resize((size_t)r.nb);
    L.x_user.resize((size_t)r.nb);
    size_t xoff = 0, psoff = 0;
    for (int k = 0; k < r.nb; ++k) {
        const int first = r.first[k], ml = r.match[2 * k], mr = r.match[2 * k + 1];
        HIPDRT_REQUIRE(first >= 0 && first <= B - r.nr, "a batch reaches outside the members");
        HIPDRT_REQUIRE(ml >= 0 && mr > ml, "a batch's common tau range is empty or negative");
        const long long nc = (long long)r.so + (mr - ml);
        HIPDRT_REQUIRE(nc * r.nr <= 4096, "nr * nc <= 4096 unknowns per coupled problem");
        ResolveBatch& bt = L.bat[(size_t)k];
        bt = ResolveBatch{};
        bt.first = first; bt.mleft = ml; bt.nc = (int)nc; bt.ps_off = (long long)psoff;
        L.x_user[(size_t)k] = xoff;
        xoff += (size_t)nc * r.nr; psoff += (size_t)nc;
        size_t g = 0;
        while (g < L.groups.size() && L.groups[g].nc != (int)nc) ++g;
        if (g == L.groups.size()) L.groups.push_back({(int)nc, 0, 0});
        ++L.groups[g].count;
        if ((int)nc * r.nr > L.n_max) L.n_max = (int)nc * r.nr;
    }
    L.ps_total = psoff;
    // outputs: the batches of a size one behind the other, at the strides launch_qp takes
    size_t slot = 0;
    std::vector<size_t> ppk_at(L.groups.size()), q_at(L.groups.size());
    std::vector<int> seen(L.groups.size(), 0);
    for (size_t g = 0; g < L.groups.size(); ++g) {
        const int n = L.groups[g].nc * r.nr;
        L.groups[g].first_slot = slot; slot += (size_t)L.groups[g].count;
        ppk_at[g] = L.ppk_total; q_at[g] = L.q_total;
        L.ppk_total += (size_t)L.groups[g].count * qp_ppk_doubles(n);
        L.q_total += (size_t)L.groups[g].count * n;
    }
    for (int k = 0; k < r.nb; ++k) {
        ResolveBatch& bt = L.bat[(size_t)k];
        size_t g = 0;
        while (L.groups[g].nc != bt.nc) ++g;
        const int n = bt.nc * r.nr;
        bt.ppk_off = (long long)(ppk_at[g] + (size_t)seen[g] * qp_ppk_doubles(n));
        bt.q_off = (long long)(q_at[g] + (size_t)seen[g] * n);
        ++seen[g];
    }
    return HIPDRT_OK;
}

void launch_resolve_assemble(hipStream_t st, const ResolveAsm& a, int nb, int n_max) {
    const int nchp = qp_nchp(n_max);
    hipLaunchKernelGGL(resolve_p_kernel, dim3((nchp + 3) / 4, nchp, nb), dim3(256), 0, st, a);
    hipLaunchKernelGGL(resolve_q_kernel, dim3((n_max + 255) / 256, nb), dim3(256), 0, st, a);
}

}  // namespace
}  // namespace hipdrt

extern "C" int hipdrt_plan_resolve_group(hipdrt_plan* p, const hipdrt_resolve_args* r, double* x_out, int* iters_out,
                                         int* status_out) try {
    HIPDRT_REQUIRE(p && r && x_out && status_out, "NULL pointer");
    HIPDRT_REQUIRE(p->prepared, "resolve takes the members of a prepared plan (hipdrt_plan_create_prepared): an EIS fit has no "
                                "v_baseline / vz_offset to eliminate");
    HIPDRT_REQUIRE(p->B >= 1 && p->prepped, "no fitted batch in the plan");
    HIPDRT_REQUIRE(r->h, "h is NULL");
    // every check comes before the first launch
    const int B = p->B, n = p->n, ldp = p->ldp;
    ResolveLayout L;
    TRY(resolve_layout(*r, B, [n](int) { return n; }, L));
    hipdrt_ctx* ctx = p->ctx;
    std::vector<int> Gs(L.groups.size());
    for (size_t g = 0; g < L.groups.size(); ++g) {
        const int nk = L.groups[g].nc * r->nr;
        Gs[g] = qp_group_size(L.groups[g].count, nk, ctx->qp_force_group);
        HIPDRT_REQUIRE(Gs[g] >= 0, "a coupled problem's size is not supported by the coneqp kernels");
        HIPDRT_REQUIRE(!(ctx->qp_force_group == 0 && nk > 2048), "n > 2048 needs the group kernel, and this context forces the batch kernel");
    }
    hipStream_t st; TRY(enter(ctx, &st));
    const size_t D = sizeof(double);

    // the members' final P, row-major, one launch for the batch (what hipdrt_plan_get_p_matrix forms member by member)
    DevBuf dPm;
    HIPDRT_CHECK(dPm.alloc((size_t)B * n * ldp * D));
    const FinalP f = plan_final_p(p, -1, live_source(p));
    PqArgs pq = p->pq(f.w);
    pq.active = nullptr; pq.P = dPm.d(); pq.Ppk = nullptr;
    launch_gram_l2(st, pq, f.g);
    LAUNCH_OK();

    std::vector<ResolveMember> mem((size_t)B);
    for (int b = 0; b < B; ++b)
        mem[(size_t)b] = ResolveMember{(long long)b * n * ldp, (long long)b * n, ldp, r->tau_indices[2 * b], r->tau_indices[2 * b + 1], 0};
    DevBuf dmem, dbat, dmy, dps, dxr, dh, dPpk, dq, dx, dit, dpc, dstat;
    TRY(upload(dmem, mem.data(), mem.size() * sizeof(ResolveMember), st));
    TRY(upload(dbat, L.bat.data(), L.bat.size() * sizeof(ResolveBatch), st));
    TRY(upload(dmy, r->my, (size_t)r->nb * r->nr * r->nr * D, st));
    TRY(upload(dps, r->param_scale, L.ps_total * D, st));
    if (r->num_remove > 0) TRY(upload(dxr, r->x_remove, (size_t)B * r->num_remove * D, st));
    HIPDRT_CHECK(dPpk.alloc(L.ppk_total * D));
    HIPDRT_CHECK(dq.alloc(L.q_total * D));
    // h in the order of the outputs
    std::vector<double> hh(L.q_total);
    for (int k = 0; k < r->nb; ++k)
        std::memcpy(hh.data() + L.bat[(size_t)k].q_off, r->h + L.x_user[(size_t)k], (size_t)L.bat[(size_t)k].nc * r->nr * D);
    TRY(upload(dh, hh.data(), hh.size() * D, st));
    HIPDRT_CHECK(dx.alloc(L.q_total * D));
    HIPDRT_CHECK(dit.alloc((size_t)r->nb * sizeof(int)));
    HIPDRT_CHECK(dpc.alloc((size_t)r->nb * D));
    HIPDRT_CHECK(dstat.alloc((size_t)r->nb * sizeof(int)));

    ResolveAsm a{};
    a.nr = r->nr; a.num_remove = r->num_remove; a.so = r->so; a.lambda_psi = r->lambda_psi;
    a.mem = dmem.as<ResolveMember>(); a.bat = dbat.as<ResolveBatch>();
    a.P = dPm.d(); a.q = p->q.d(); a.my = dmy.d(); a.ps = dps.d(); a.xrm = dxr.d();
    a.Ppk = dPpk.d(); a.qk = dq.d();
    launch_resolve_assemble(st, a, r->nb, L.n_max);
    LAUNCH_OK();

    // one coneqp launch per size, as hipdrt_qp_batch sets it up for that many problems of that size
    size_t ppk_at = 0, q_at = 0;
    for (size_t g = 0; g < L.groups.size(); ++g) {
        const int nbg = L.groups[g].count, nk = L.groups[g].nc * r->nr, G = Gs[g];
        DevBuf dL, dstate, dgs;
        HIPDRT_CHECK(dL.alloc((size_t)nbg * qp_scratch_doubles(nk, G) * D));
        HIPDRT_CHECK(dstate.alloc((size_t)nbg * (G > 1 ? G : 1) * qp_state_doubles(nk) * D));
        QpArgs qa{};
        qa.B = nbg; qa.n = nk; qa.P = nullptr; qa.ldp = round_up(nk, 2); qa.p_stride = (long long)nk * qa.ldp;
        qa.Ppk = dPpk.d() + ppk_at; qa.ppk_stride = (long long)qp_ppk_doubles(nk); qa.nchp = qp_nchp(nk);
        qa.q = dq.d() + q_at; qa.h = dh.d() + q_at; qa.h_stride = nk;
        qa.L = dL.d(); qa.ldl = (int)qp_scratch_ld(nk); qa.l_stride = (long long)qp_scratch_doubles(nk, G);
        qa.x = dx.d() + q_at; qa.iters = dit.i() + L.groups[g].first_slot; qa.pcost = dpc.d() + L.groups[g].first_slot;
        qa.status = dstat.i() + L.groups[g].first_slot;
        qa.active = nullptr; qa.iters_accum = nullptr;
        qa.G = G; qa.waves = ctx->qp_waves;
        if (G >= 1) {
            HIPDRT_CHECK(dgs.alloc((size_t)nbg * qp_gsync_ints() * sizeof(int)));
            qa.gsync = dgs.i();
        }
        qa.state = dstate.d(); qa.state_ld = qp_state_ld(nk); qa.state_stride = (long long)qp_state_doubles(nk);
        qa.opts = default_qp_opts();
        TRY(launch_qp(st, qa));
        LAUNCH_OK();
        HIPDRT_CHECK(hipStreamSynchronize(st));      // this size's scratch is released here
        ppk_at += (size_t)nbg * qp_ppk_doubles(nk); q_at += (size_t)nbg * nk;
    }

    std::vector<double> hx(L.q_total);
    std::vector<int> hit((size_t)r->nb), hst((size_t)r->nb);
    HIPDRT_CHECK(hipMemcpyAsync(hx.data(), dx.p, hx.size() * D, hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(hit.data(), dit.p, hit.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipMemcpyAsync(hst.data(), dstat.p, hst.size() * sizeof(int), hipMemcpyDeviceToHost, st));
    HIPDRT_CHECK(hipStreamSynchronize(st));
    // back into the caller's order
    std::vector<int> seen(L.groups.size(), 0);
    for (int k = 0; k < r->nb; ++k) {
        const ResolveBatch& bt = L.bat[(size_t)k];
        size_t g = 0;
        while (L.groups[g].nc != bt.nc) ++g;
        const size_t slot = L.groups[g].first_slot + (size_t)seen[g]++;
        std::memcpy(x_out + L.x_user[(size_t)k], hx.data() + bt.q_off, (size_t)bt.nc * r->nr * D);
        if (iters_out) iters_out[k] = hit[slot];
        status_out[k] = hst[slot];
    }
    return HIPDRT_OK;
} HIPDRT_CATCH

extern "C" int hipdrt_debug_resolve_assemble(hipdrt_ctx* ctx, const hipdrt_resolve_args* r, int B, const double* P, const double* q,
                                             double* P_out, double* q_out) try {
    HIPDRT_REQUIRE(ctx && r && P && q && P_out && q_out, "NULL pointer");
    HIPDRT_REQUIRE(B >= 1 && B <= 4096, "1 <= B <= 4096");
    HIPDRT_REQUIRE(r->tau_indices, "NULL pointer in the description");
    // the members' sizes follow from their ranges; resolve_layout checks the ranges themselves
    std::vector<ResolveMember> mem((size_t)B);
    size_t ptot = 0, qtot = 0;
    for (int b = 0; b < B; ++b) {
        const long long w = (long long)r->tau_indices[2 * b + 1] - r->tau_indices[2 * b];
        HIPDRT_REQUIRE(w >= 1 && w <= 4096 && r->num_remove >= 0 && r->so >= 0 && (long long)r->num_remove + r->so + w <= 8192,
                       "a member's tau range is empty or too long");
        const int nbm = r->num_remove + r->so + (int)w;
        mem[(size_t)b] = ResolveMember{(long long)ptot, (long long)qtot, nbm, r->tau_indices[2 * b], r->tau_indices[2 * b + 1], 0};
        ptot += (size_t)nbm * nbm; qtot += (size_t)nbm;
    }
    ResolveLayout L;
    TRY(resolve_layout(*r, B, [&mem](int b) { return mem[(size_t)b].ld; }, L));
    for (size_t i = 0; i < ptot; ++i) HIPDRT_REQUIRE(std::isfinite(P[i]), "non-finite P");
    for (size_t i = 0; i < qtot; ++i) HIPDRT_REQUIRE(std::isfinite(q[i]), "non-finite q");
    hipStream_t st; TRY(enter(ctx, &st));
    const size_t D = sizeof(double);
    GuardedOuts g;
    ResolveAsm a{};
    a.nr = r->nr; a.num_remove = r->num_remove; a.so = r->so; a.lambda_psi = r->lambda_psi;
    const double dummy = 0.0;
    TRY(g.in("the member table", mem.data(), mem.size(), a.mem, st));
    TRY(g.in("the batch table", L.bat.data(), L.bat.size(), a.bat, st));
    TRY(g.in("P", P, ptot, a.P, st));
    TRY(g.in("q", q, qtot, a.q, st));
    TRY(g.in("my", r->my, (size_t)r->nb * r->nr * r->nr, a.my, st));
    TRY(g.in("param_scale", r->param_scale, L.ps_total, a.ps, st));
    TRY(g.in("x_remove", r->num_remove > 0 ? r->x_remove : &dummy, r->num_remove > 0 ? (size_t)B * r->num_remove : 1, a.xrm, st));
    std::vector<double> hppk(L.ppk_total, 7e77), hq(L.q_total, 7e77);
    TRY(g.want("the packed image of P", hppk.data(), hppk.size(), a.Ppk, st));
    TRY(g.want("q_k", hq.data(), hq.size(), a.qk, st));
    launch_resolve_assemble(st, a, r->nb, L.n_max);
    LAUNCH_OK();
    TRY(g.back(st));
    // lower tiles -> dense, in the caller's order of batches
    auto at = [](int i, int j) { return 2 * ((j >> 3) * 64 + i * 4 + (j & 3)) + ((j >> 2) & 1); };     // (row, column) inside a tile
    size_t pout = 0;
    for (int k = 0; k < r->nb; ++k) {
        const ResolveBatch& bt = L.bat[(size_t)k];
        const int n = bt.nc * r->nr, nchp = qp_nchp(n);
        const double* img = hppk.data() + bt.ppk_off;
        double* out = P_out + pout;
        for (int tr = 0; tr < nchp; ++tr)
            for (int tc = 0; tc <= tr; ++tc) {
                const double* tile = img + ((size_t)tr * nchp + tc) * 256;
                for (int i = 0; i < 16; ++i)
                    for (int j = 0; j < 16; ++j) {
                        const int gi = tr * 16 + i, gj = tc * 16 + j;
                        const double v = tile[at(i, j)];
                        if (gi >= n || gj >= n) {
                            if (!(v == 0.0)) { set_error("a padding entry of the packed image is not zero"); return HIPDRT_E_NUMERIC; }
                        } else if (gi >= gj) {
                            out[(size_t)gi * n + gj] = v; out[(size_t)gj * n + gi] = v;
                        } else if (std::memcmp(&v, &tile[at(j, i)], D) != 0) {
                            set_error("a diagonal tile of the packed image is not symmetric"); return HIPDRT_E_NUMERIC;
                        }
                    }
            }
        std::memcpy(q_out + L.x_user[(size_t)k], hq.data() + bt.q_off, (size_t)n * D);
        pout += (size_t)n * n;
    }
    return HIPDRT_OK;
} HIPDRT_CATCH
