// Weighted normal equations of qphb.solve_convex_opt (hybdrt/models/qphb.py:465-466) and the L2 assembly of
// qphb.calculate_qp_l2_matrix (qphb.py:53-120), batched over spectra that share one response matrix A:
//
//     P_b = (W_b A)' (W_b A) + L2_b ,   L2_b = sum_k S_bk^1/2 (M_k o scale_bk) S_bk^1/2
//     q_b = -(W_b A)' (W_b y_b) + l1
//
// FP64 only.  The contraction runs on v_mfma_f64_16x16x4_f64: a 256-thread workgroup
// (4 wavefronts; who owns which 16x16 sub-tile: "Tile decomposition" below) owns a 64x64 tile of the lower triangle
// of P_b, stages 16-row slabs of A (already multiplied by w_b) through LDS and mirrors the tile into the upper
// triangle on store.  The reference forms
// L2 with two dense n^3 products per derivative order; here it is the O(n^2) elementwise epilogue of the tile.
#include "common.hpp"
#include <type_traits>

namespace hipdrt {

typedef double v4d __attribute__((ext_vector_type(4)));

static constexpr int GT = 64;        // tile edge
static constexpr int GK = 16;        // K slab
static constexpr int GLD = 80;       // LDS row stride in doubles (k-rows land 32 banks apart: conflict-free b64 reads)


// Tile decomposition.  The lower triangle is cut into 64 x 64 tiles, one workgroup each, and every tile into 16 x 16 sub-tiles, one
// MFMA accumulator each.  Whoever owns a sub-tile gives it the same MFMA sequence (k ascending, the same operands), so the deal
// below does not move a bit of P.
//   off-diagonal workgroup: wavefront wv owns the 32 x 32 quadrant (wv >> 1, wv & 1), four sub-tiles that share their operands.
//   diagonal workgroup: its 10 lower sub-tiles are dealt round-robin over the four wavefronts (the quadrant deal gives 3 / 0 / 4 / 3),
//     the turn starting at wavefront 0 or 2 with the parity of the tile, so that the short shares even out over a spectrum.
//   the strip: with nt16 = ceil(n / 16) sub-tile rows and nt16 % 4 == 1 (n = 514: 512 tau + R_inf + L, nt16 = 33) the last sub-tile
//     row R gets no 64-tile row of its own -- nine workgroups that would fetch full slabs for an eighth of a tile's MFMAs.  Diagonal
//     workgroup t takes the sub-tiles (R, 4t ... 4t+3) instead: their column operand is the slab it has staged anyway, their row
//     operand -- columns 16R ... 16R+15 of A -- is staged into the columns 64 ... 79 of sI that the row stride leaves free (one
//     double per thread, in a vj register a diagonal tile does not use).  The last diagonal workgroup also takes the corner (R, R).
//     That is 14 (15) sub-tiles, at most four per wavefront; at n = 514 36 workgroups instead of 45 and 140 / 141 sub-tiles per
//     wavefront index and spectrum instead of 153 / 128 / 144 / 136.
__host__ __device__ inline bool gram_strip_folds(int n) { const int nt16 = (n + 15) >> 4; return (nt16 & 3) == 1 && nt16 > 1; }

struct GramSub { int r, c; };
__host__ __device__ constexpr GramSub gram_diag_sub(int e) {
    const int r = e >= 10 ? 4 : e >= 6 ? 3 : e >= 3 ? 2 : e >= 1 ? 1 : 0;
    return GramSub{r, e >= 14 ? 4 : e >= 10 ? e - 10 : e - r * (r + 1) / 2};
}

// one slab of a diagonal workgroup for the wavefront whose turn is TURN: sl = the lane's (k row, column) base in the slab
template <int TURN>
__device__ __forceinline__ void gram_diag_slab(const double* sl, v4d (&acc)[4], int needm) {
#pragma unroll
    for (int kk = 0; kk < GK; kk += 4) {
        double x[5];
#pragma unroll
        for (int c = 0; c < 5; ++c) x[c] = sl[kk * GLD + c * 16];  // (the reads no sub-tile of this turn uses fall away)
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            const GramSub sub = gram_diag_sub(TURN + 4 * s);
            if (needm & (1 << s)) acc[s] = __builtin_amdgcn_mfma_f64_16x16x4f64(x[sub.c], x[sub.r], acc[s], 0, 0, 0);
        }
    }
}

// ROWP: also write the row-major copy P (stand-alone entry points); the fit loop reads the packed tiles only
template <bool DOP, bool ROWP>
__global__ __launch_bounds__(256, 5) void gram_kernel(int m, int n, const double* __restrict__ A, int lda,
                                                   const double* __restrict__ w, GramL2 g, double* __restrict__ P,
                                                   int ldp, long long p_stride, const int* __restrict__ active,
                                                   int ntile, double* __restrict__ Ppk, long long ppk_stride, int nchp,
                                                   long long a_stride) {
    const int b = blockIdx.y;
    if (active && !active[b]) return;
    A += (size_t)b * a_stride;
    // decode lower-triangular tile index -> (ti >= tj)
    int t = blockIdx.x, ti = 0;
    while (t >= ti + 1) { t -= ti + 1; ++ti; }
    const int tj = t;
    const int i0 = ti * GT, j0 = tj * GT;
    const bool diag = (ti == tj);
    const int nt16 = (n + 15) >> 4;
    const bool strip = diag && gram_strip_folds(n);         // this workgroup carries four sub-tiles of the strip ...
    const int s0 = (nt16 - 1) * 16;                          // ... whose first row this is
    const bool last = strip && i0 + GT == s0;                // ... and the corner

    __shared__ double sI[GK * GLD];
    __shared__ double sJ[GK * GLD];

    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    const double* wb = w + (size_t)b * m;
    double* Pk = Ppk ? Ppk + (size_t)b * ppk_stride : nullptr;

    // Sub-tile e of a diagonal workgroup, row-major over its lower sub-tiles, then the strip's four, then the corner:
    // e = 0 ... 9 -> (r, c) with c <= r <= 3, 10 ... 13 -> (4, e - 10), 14 -> (4, 4), row / column 4 being the strip's.
    // Wavefront wv owns e = turn + 4 s, s = 0 ... 3, as far as they exist (nown) and hold data to multiply (nneed: the rest
    // is padding of the packed layout, written as zeros).
    int nown = 0, needm = 0;                                 // needm: bit s = sub-tile turn + 4 s is multiplied
    const int turn = (wv + 2 * (ti & 1)) & 3;
    if (diag) {
        const int rows_all = (Pk && nchp > nt16 ? nchp : nt16) - 4 * ti, rows_data = nt16 - 4 * ti;
        const int nr = rows_all < 4 ? rows_all : 4, nd = rows_data < 4 ? rows_data : 4;
        nown = nr * (nr + 1) / 2 + (strip ? 4 : 0) + (last ? 1 : 0);
        const int nneed = strip ? nown : nd * (nd + 1) / 2;
#pragma unroll
        for (int s = 0; s < 4; ++s) needm |= (turn + 4 * s < nneed) << s;
    }
    // the quadrant of an off-diagonal workgroup: sub-tile s = 2 a + c is (2 (wv >> 1) + a, 2 (wv & 1) + c) of the tile
    const int qr = 4 * ti + 2 * (wv >> 1), qc = 4 * tj + 2 * (wv & 1);
    const bool need00 = qr < nt16 && qc < nt16, need01 = qr < nt16 && qc + 1 < nt16;
    const bool need10 = qr + 1 < nt16 && qc < nt16, need11 = qr + 1 < nt16 && qc + 1 < nt16;

    v4d acc[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) acc[s] = (v4d){0.0, 0.0, 0.0, 0.0};

    // staging map: thread -> (k = tid/16, 4 consecutive columns); the strip: (k = tid/16, column tid%16).  How a slab is fetched is
    // decided here, once per workgroup, and compiled into the K loop as FORM (a choice made inside the loop is a join at which
    // the compiler waits for every load in flight -- a memory round trip per slab in front of the MFMAs):
    //   FORM 0, full: every staged column lies inside n (the strip's 16 apart), m is a multiple of the slab and the rows are
    //     16-byte aligned -- every workgroup of the plan's matrices.  Unconditional 16-byte loads from two per-thread pointers that
    //     advance a slab at a time; the strip's operand is read from a column clamped into the row and masked when it is used.
    //   FORM 1, general with 16-byte loads (even lda and n, aligned rows), FORM 2, general with 8-byte loads: edge tiles, slab
    //     tails, odd sizes; every load under its own bounds test.
    const int sk = tid >> 4, sc = (tid & 15) * 4;
    const bool vec2 = ((lda | n) & 1) == 0 && (reinterpret_cast<size_t>(A) & 15) == 0;
    const bool full = vec2 && m >= GK && (m & (GK - 1)) == 0 && i0 + GT <= n && (diag || j0 + GT <= n);
    const bool smask = strip && s0 + (tid & 15) < n;         // the strip's column of this thread holds data
    // slab k0+GK is fetched (global -> registers) while slab k0 is multiplied out of LDS; the products with w are formed only
    // when the slab is written to LDS, so the loads are waited for at the head of the next slab and nowhere else
    double vi[4], vj[4], wkr = 0.0;
    const double *pI = nullptr, *pJ = nullptr;               // FORM 0: the thread's columns in the row of the slab to fetch next
    // (DIAG, TURN, FORM are the workgroup's `diag`, the wavefront's `turn` and the fetch form as types: the K loop is compiled
    // once per kind, each with the registers it needs)
    auto fetch = [&](auto DIAG, auto FORM, int k0) {
        constexpr bool D = decltype(DIAG)::value;
        constexpr int F = decltype(FORM)::value;
        if constexpr (F == 0) {
            wkr = wb[k0 + sk];
            const double2 t0 = *reinterpret_cast<const double2*>(pI), t1 = *reinterpret_cast<const double2*>(pI + 2);
            vi[0] = t0.x; vi[1] = t0.y; vi[2] = t1.x; vi[3] = t1.y;
            if constexpr (!D) {
                const double2 u0 = *reinterpret_cast<const double2*>(pJ), u1 = *reinterpret_cast<const double2*>(pJ + 2);
                vj[0] = u0.x; vj[1] = u0.y; vj[2] = u1.x; vj[3] = u1.y;
            } else if (strip) {
                vj[0] = *pJ;
            }
            pI += (size_t)GK * lda;
            pJ += (size_t)GK * lda;
        } else {
            const int k = k0 + sk;
#pragma unroll
            for (int e = 0; e < 4; ++e) { vi[e] = 0.0; vj[e] = 0.0; }
            wkr = 0.0;
            if (k < m) {
                wkr = wb[k];
                const double* row = A + (size_t)k * lda;
                if constexpr (F == 1) {
#pragma unroll
                    for (int e = 0; e < 4; e += 2) {
                        const int ci = i0 + sc + e, cj = j0 + sc + e;
                        if (ci < n) { const double2 t = *reinterpret_cast<const double2*>(row + ci); vi[e] = t.x; vi[e + 1] = t.y; }
                        if (!D && cj < n) { const double2 t = *reinterpret_cast<const double2*>(row + cj); vj[e] = t.x; vj[e + 1] = t.y; }
                    }
                } else {
#pragma unroll
                    for (int e = 0; e < 4; ++e) {
                        const int ci = i0 + sc + e, cj = j0 + sc + e;
                        if (ci < n) vi[e] = row[ci];
                        if (!D && cj < n) vj[e] = row[cj];
                    }
                }
                if (D && smask) vj[0] = row[s0 + (tid & 15)];
            }
        }
    };
    // 16x16 sub-tiles that are pure padding (beyond n) or lie above the diagonal (the epilogue takes those elements
    // from the mirror) are not multiplied at all
    auto kloop = [&](auto DIAG, auto TURN, auto FORM) {
        constexpr bool D = decltype(DIAG)::value;
        constexpr bool FULL = decltype(FORM)::value == 0;
        if constexpr (FULL) {
            pI = A + (size_t)sk * lda + i0 + sc;
            pJ = A + (size_t)sk * lda + (D ? (smask ? s0 + (tid & 15) : n - 1) : j0 + sc);
        }
        fetch(DIAG, FORM, 0);
        for (int k0 = 0; k0 < m; k0 += GK) {
            __syncthreads();   // previous slab fully consumed
            *reinterpret_cast<double2*>(&sI[sk * GLD + sc]) = make_double2(wkr * vi[0], wkr * vi[1]);
            *reinterpret_cast<double2*>(&sI[sk * GLD + sc + 2]) = make_double2(wkr * vi[2], wkr * vi[3]);
            if (!D) {
                *reinterpret_cast<double2*>(&sJ[sk * GLD + sc]) = make_double2(wkr * vj[0], wkr * vj[1]);
                *reinterpret_cast<double2*>(&sJ[sk * GLD + sc + 2]) = make_double2(wkr * vj[2], wkr * vj[3]);
            } else if (strip) {
                sI[sk * GLD + GT + (tid & 15)] = wkr * (FULL && !smask ? 0.0 : vj[0]);
            }
            __syncthreads();
            if (k0 + GK < m) fetch(DIAG, FORM, k0 + GK);
            if (!D) {
                const int wi = (wv >> 1) * 32, wj = (wv & 1) * 32;     // four sub-tiles from four operand reads
#pragma unroll
                for (int kk = 0; kk < GK; kk += 4) {
                    const int kr = kk + (lane >> 4);
                    double a0 = sI[kr * GLD + wi + (lane & 15)];
                    double a1 = sI[kr * GLD + wi + 16 + (lane & 15)];
                    double b0 = sJ[kr * GLD + wj + (lane & 15)];
                    double b1 = sJ[kr * GLD + wj + 16 + (lane & 15)];
                    // (a full workgroup has no padding sub-tile)
                    if (FULL || need00) acc[0] = __builtin_amdgcn_mfma_f64_16x16x4f64(b0, a0, acc[0], 0, 0, 0);
                    if (FULL || need01) acc[1] = __builtin_amdgcn_mfma_f64_16x16x4f64(b1, a0, acc[1], 0, 0, 0);
                    if (FULL || need10) acc[2] = __builtin_amdgcn_mfma_f64_16x16x4f64(b0, a1, acc[2], 0, 0, 0);
                    if (FULL || need11) acc[3] = __builtin_amdgcn_mfma_f64_16x16x4f64(b1, a1, acc[3], 0, 0, 0);
                }
            } else {
                // any wavefront reads any 16 columns of the slab (the strip's are columns 64 ... 79); one loop per turn, so
                // that every operand address is the lane's base plus a constant
                const double* sl = sI + (lane >> 4) * GLD + (lane & 15);
                gram_diag_slab<decltype(TURN)::value>(sl, acc, needm);
            }
        }
    };
    auto kform = [&](auto DIAG, auto TURN) {
        if (full) kloop(DIAG, TURN, std::integral_constant<int, 0>{});
        else if (vec2) kloop(DIAG, TURN, std::integral_constant<int, 1>{});
        else kloop(DIAG, TURN, std::integral_constant<int, 2>{});
    };
    if (!diag) kform(std::false_type{}, std::integral_constant<int, 0>{});
    else if (turn == 0) kform(std::true_type{}, std::integral_constant<int, 0>{});
    else if (turn == 1) kform(std::true_type{}, std::integral_constant<int, 1>{});
    else if (turn == 2) kform(std::true_type{}, std::integral_constant<int, 2>{});
    else kform(std::true_type{}, std::integral_constant<int, 3>{});

    // sqrt(s_k) of the tile's rows / columns once per workgroup (the L2 epilogue needs them per element); they take
    // over the slab buffers, so the kernel needs 20 kB of LDS and eight workgroups fit a CU
    double* sqI = sI;                                                // [3][GT]
    double* sqJ = sJ;                                                // [3][GT]
    // On a log-uniform tau grid the DRT block of every penalty matrix is symmetric Toeplitz, M_k[i][j] = t_k[|i - j|]
    // with t_k = its first row: the tile needs the 127 differences around i0 - j0 only, staged behind the sqrt tables,
    // and no dense matrix is read in the epilogue (three 2 MB matrices per spectrum and outer iteration otherwise).
    constexpr int TW = 2 * GT;                                      // window slots per order (127 used)
    double* tw = sI + 3 * GT;                                        // [3][TW]
    const int dbase = i0 - j0 - (GT - 1);                           // difference of window slot 0
    // the strip's tables, in the sJ region a diagonal tile leaves free: sqrt(s_k) of its 16 rows and a window of its own for the
    // 79 differences 16R + r - (j0 + c) (the corner's differences -15 ... 15 are in the tile's window)
    constexpr int SW = GT + 16;
    double* sqS = sJ + 3 * GT;                                       // [3][16]
    double* tws = sJ + 4 * GT;                                       // [3][SW]
    const int dbase_s = s0 - j0 - (GT - 1);
    double fac[3] = {0, 0, 0};
    // Tiles of the DRT block that lie wholly beyond the reach of the penalty matrices -- every |i - j| of the tile larger than the
    // last non-zero entry of the Toeplitz first rows -- would add (sqrt(s_i) * 0) * sqrt(s_j) = 0 to every element: no tables,
    // no epilogue arithmetic, the same bits (21 of the 36 tiles of a 514 x 514 matrix lie two or more tile diagonals out; the 6
    // of them that touch the special-parameter columns qualify when those columns of the penalty matrices are zero outside the
    // special block, which the plan checks once).  The strip part of a diagonal tile is judged by its own differences (at
    // n = 514 it is within reach of the last diagonal tiles only).
    const bool reach_known = !DOP && g.toep && g.toep_maxd >= 0 && (j0 >= g.ns || g.spec_zero);
    const bool l2on = g.s && !(reach_known && i0 >= g.ns && dbase > g.toep_maxd);
    const bool l2on_s = strip && g.s && !(reach_known && s0 >= g.ns && dbase_s > g.toep_maxd);
    if (l2on) {
#pragma unroll
        for (int k = 0; k < 3; ++k) fac[k] = g.dfac[k] * (g.use_rho ? g.rho[(size_t)b * 3 + k] : 1.0);
        __syncthreads();   // last slab consumed
        const double* sb_ = g.s + (size_t)b * 3 * n;
        for (int e = tid; e < 3 * GT; e += 256) {
            const int k = e / GT, c = e % GT;
            sqI[e] = (i0 + c < n) ? sqrt(sb_[k * n + i0 + c]) : 0.0;
            sqJ[e] = (j0 + c < n) ? sqrt(sb_[k * n + j0 + c]) : 0.0;
        }
        if (strip && tid < 3 * 16) {
            const int k = tid >> 4, c = tid & 15;
            sqS[tid] = (s0 + c < n) ? sqrt(sb_[k * n + s0 + c]) : 0.0;
        }
        if (g.toep) {
            // (the window holds M_k[|i - j|] * fac[k]: the product the epilogue used to form per element)
            const int nd = n - g.ns;                                // size of the DRT block
            for (int e = tid; e < 3 * TW; e += 256) {
                const int k = e / TW, sl = e % TW;
                int dd = dbase + sl;
                dd = dd < 0 ? -dd : dd;
                tw[e] = (g.dfac[k] > 0.0 && dd < nd) ? g.mk[k][(size_t)g.ns * g.ldm + g.ns + dd] * fac[k] : 0.0;
            }
            if (l2on_s && tid < 3 * SW) {
                const int k = tid / SW, dd = dbase_s + tid % SW;    // > 0
                tws[tid] = (g.dfac[k] > 0.0 && dd < nd) ? g.mk[k][(size_t)g.ns * g.ldm + g.ns + dd] * fac[k] : 0.0;
            }
        }
        __syncthreads();
    }
    // epilogue: + L2, store lower tile and its mirror.  With the swapped operands the accumulator of lane l, register
    // r is element (row = l&15, column = (l>>4) + 4r) of the sub-tile.
    double* Pb = (ROWP && P) ? P + (size_t)b * p_stride : nullptr;   // row-major copy is optional (the resident QP kernel reads Ppk)
    double dfac2[3] = {0, 0, 0};
    if (l2on) {
        if (DOP) {
#pragma unroll
            for (int k = 0; k < 3; ++k) dfac2[k] = g.dop_dfac[k] * (g.use_rho ? g.dop_rho[(size_t)b * 3 + k] : 1.0);
        }
    }
    const int dop_lo = DOP ? g.dop_start : 0, dop_hi = DOP ? g.dop_start + g.dop_size : 0;
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        // one owned sub-tile (r16, c16): tables of the tile or of the strip, everything else keyed on the absolute (i, j)
        int r16 = qr + (s >> 1), c16 = qc + (s & 1);
        bool srow = false, scol = false;
        if (diag) {
            const int e = turn + 4 * s;
            if (e >= nown) continue;
            const GramSub sub = gram_diag_sub(e);
            srow = sub.r == 4;
            scol = sub.c == 4;
            r16 = srow ? nt16 - 1 : 4 * ti + sub.r;
            c16 = scol ? nt16 - 1 : 4 * ti + sub.c;
        }
        const bool sw = srow && !scol;                               // a strip sub-tile left of the corner
        const bool on = sw ? l2on_s : l2on;
        const double* sqr = srow ? sqS - s0 : sqI - i0;              // [k * rstr + i]
        const double* sqc = scol ? sqS - s0 : sqJ - j0;              // [k * cstr + j]
        const int rstr = srow ? 16 : GT, cstr = scol ? 16 : GT;
        const double* win = sw ? tws - dbase_s : tw - dbase;         // [k * wstr + (i - j)]
        const int wstr = sw ? SW : TW;
        double vals[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int i = r16 * 16 + (lane & 15);
            const int j = c16 * 16 + (lane >> 4) + 4 * r;
            double v = 0.0;
            if (i < n && j < n) {
                v = acc[s][r];
                if (on) {
                    double l2 = 0.0;
#pragma unroll
                    for (int k = 0; k < 3; ++k) {
                        if (g.dfac[k] > 0.0) {
                            // (i, j) = (lane&15, lane>>4 + 4r): reading the mirror element keeps the wave's
                            // addresses contiguous when the matrices are bitwise symmetric
                            double mv;
                            if (g.toep && i >= g.ns && j >= g.ns) {
                                mv = win[k * wstr + (i - j)];
                            } else {
                                mv = g.sym ? g.mk[k][(size_t)j * g.ldm + i] : g.mk[k][(size_t)i * g.ldm + j];
                                if (i >= g.ns && j >= g.ns) mv *= fac[k];
                                else if (DOP && i >= dop_lo && i < dop_hi && j >= dop_lo && j < dop_hi) mv *= dfac2[k];
                            }
                            l2 += (sqr[k * rstr + i] * mv) * sqc[k * cstr + j];
                        }
                    }
                    v += l2;
                } else if (!g.s && g.l2) {
                    v += g.l2[(size_t)b * g.l2_stride + (size_t)i * g.ldl2 + j];
                }
                if (ROWP && Pb && j <= i) {                // upper part of a diagonal sub-tile comes from the mirror
                    Pb[(size_t)i * ldp + j] = v;
                    if (i != j) Pb[(size_t)j * ldp + i] = v;
                }
            }
            vals[r] = v;
        }
        // second copy for the Cholesky in the factor's tile layout (qp_resident.hpp): double2 h*64 + i*4 + q holds
        // columns q + 8h, q + 8h + 4 of row i -- two 16-byte stores per lane, 2 KB contiguous per tile
        if (Pk && r16 < nchp && c16 < nchp && r16 >= c16) {
            double2* tile = reinterpret_cast<double2*>(Pk + ((size_t)r16 * nchp + c16) * 256);
            const int fo = (lane & 15) * 4 + (lane >> 4);
            tile[fo] = make_double2(vals[0], vals[1]);
            tile[64 + fo] = make_double2(vals[2], vals[3]);
        }
    }
    // the packed layout's pure-padding tile rows below the strip (n = 514: tile row 33 of nchp = 34), which a 64-tile row of
    // the strip's own would have covered: zeros, beneath this workgroup's columns
    if (Pk && strip) {
        const int pe = nchp < nt16 + 3 ? nchp : nt16 + 3;
        for (int pr = nt16; pr < pe; ++pr) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int pc = h ? nt16 - 1 + wv : 4 * ti + wv;
                if (h && !(last && pc <= pr)) continue;
                double2* tile = reinterpret_cast<double2*>(Pk + ((size_t)pr * nchp + pc) * 256);
                tile[lane] = make_double2(0.0, 0.0);
                tile[64 + lane] = make_double2(0.0, 0.0);
            }
        }
    }
}

// row-major symmetric P -> lower tiles in the factor's tile layout; one wavefront per tile, grid (tiles, B)
__global__ __launch_bounds__(64) void pack_p_kernel(int n, const double* __restrict__ P, int ldp, long long p_stride,
                                                    double* __restrict__ Ppk, long long ppk_stride, int nchp) {
    int t = blockIdx.x, tr = 0;
    while (t >= tr + 1) { t -= tr + 1; ++tr; }
    const int tc = t, b = blockIdx.y, lane = threadIdx.x;
    const double* Pb = P + (size_t)b * p_stride;
    double vals[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = tr * 16 + (lane & 15), j = tc * 16 + (lane >> 4) + 4 * r;
        double v = 0.0;
        if (i < n && j < n) v = (i >= j) ? Pb[(size_t)i * ldp + j] : Pb[(size_t)j * ldp + i];   // lower triangle only
        vals[r] = v;
    }
    double2* tile = reinterpret_cast<double2*>(Ppk + (size_t)b * ppk_stride + ((size_t)tr * nchp + tc) * 256);
    const int fo = (lane & 15) * 4 + (lane >> 4);
    tile[fo] = make_double2(vals[0], vals[1]);
    tile[64 + fo] = make_double2(vals[2], vals[3]);
}

// q_b[i] = -sum_k (w_k A_ki)(w_k y_k) + l1_i ; grid (ceil(n/256), B)
__global__ __launch_bounds__(256) void qvec_kernel(int m, int n, const double* __restrict__ A, int lda,
                                                   const double* __restrict__ w, const double* __restrict__ y,
                                                   const double* __restrict__ l1, double l1_scalar,
                                                   double* __restrict__ q, const int* __restrict__ active,
                                                   long long a_stride) {
    const int b = blockIdx.y;
    if (active && !active[b]) return;
    A += (size_t)b * a_stride;
    __shared__ double sw[256], swy[256];
    const int i = blockIdx.x * 256 + threadIdx.x;
    const double* wb = w + (size_t)b * m;
    const double* yb = y + (size_t)b * m;
    double acc = 0.0;
    for (int k0 = 0; k0 < m; k0 += 256) {
        __syncthreads();
        const int kk = k0 + threadIdx.x;
        if (kk < m) { const double wk = wb[kk]; sw[threadIdx.x] = wk; swy[threadIdx.x] = wk * yb[kk]; }
        __syncthreads();
        const int lim = (m - k0) < 256 ? (m - k0) : 256;
        if (i < n) {
            for (int k = 0; k < lim; ++k) acc += (sw[k] * A[(size_t)(k0 + k) * lda + i]) * swy[k];
        }
    }
    if (i < n) q[(size_t)b * n + i] = -acc + (l1 ? l1[i] : l1_scalar);
}

// row-major M[nrow][ncol] -> tiles [ntile_rows][nchp][256] in the factor's tile layout, columns shifted right by
// col_offset (the special-parameter slots), zero padding elsewhere; one wavefront per tile
__global__ __launch_bounds__(64) void pack_rows_kernel(int nrow, int ncol, int col_offset, const double* __restrict__ M,
                                                       int ldm, double* __restrict__ tiles, int nchp) {
    const int tr = blockIdx.y, tc = blockIdx.x, lane = threadIdx.x;
    double vals[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int i = tr * 16 + (lane & 15), j = tc * 16 + (lane >> 4) + 4 * r - col_offset;
        vals[r] = (i < nrow && j >= 0 && j < ncol) ? M[(size_t)i * ldm + j] : 0.0;
    }
    double2* tile = reinterpret_cast<double2*>(tiles + ((size_t)tr * nchp + tc) * 256);
    const int fo = (lane & 15) * 4 + (lane >> 4);
    tile[fo] = make_double2(vals[0], vals[1]);
    tile[64 + fo] = make_double2(vals[2], vals[3]);
}

void launch_pack_rows(hipStream_t st, int nrow, int ncol, int col_offset, const double* M, int ldm, int ntile_rows,
                      double* tiles, int nchp) {
    hipLaunchKernelGGL(pack_rows_kernel, dim3(nchp, ntile_rows), dim3(64), 0, st, nrow, ncol, col_offset, M, ldm, tiles,
                       nchp);
}

// out = scale * Y Y' for the rows Y of `nex` tile rows (tile-packed, `nch` tiles per tile row, the first `ncol` tile columns
// count): the full posterior covariance from the rows B L^-T that the variance kernel leaves behind the factor.  One 16 x 16
// tile of the (symmetric) result per workgroup, lower tiles computed and mirrored; chunks in ascending order (fixed sums).
__global__ __launch_bounds__(256) void rows_outer_kernel(const double* __restrict__ Y, int nch, int ncol, int nrow, double scale,
                                                         double* __restrict__ out, int ld) {
    const int ti = blockIdx.y, tj = blockIdx.x;
    if (tj > ti) return;
    __shared__ double A[256], Bt[256];
    const int t = threadIdx.x, i = t >> 4, j = t & 15;
    auto at = [](int r, int k) { return 2 * ((k >> 3) * 64 + r * 4 + (k & 3)) + ((k >> 2) & 1); };   // (row, column) inside a tile
    double acc = 0.0;
    for (int c = 0; c < ncol; ++c) {
        A[t] = Y[((size_t)ti * nch + c) * 256 + t];
        Bt[t] = Y[((size_t)tj * nch + c) * 256 + t];
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 16; ++k) acc += A[at(i, k)] * Bt[at(j, k)];
        __syncthreads();
    }
    const int r = ti * 16 + i, cc = tj * 16 + j;
    if (r < nrow && cc < nrow) {
        out[(size_t)r * ld + cc] = acc * scale;
        out[(size_t)cc * ld + r] = acc * scale;
    }
}

void launch_rows_outer(hipStream_t st, const double* Y, int nch, int ncol, int nex, int nrow, double scale, double* out, int ld) {
    hipLaunchKernelGGL(rows_outer_kernel, dim3(nex, nex), dim3(256), 0, st, Y, nch, ncol, nrow, scale, out, ld);
}

void launch_pack_p(hipStream_t st, int B, int n, const double* P, int ldp, double* Ppk) {
    const int nt = (n + 15) / 16;
    hipLaunchKernelGGL(pack_p_kernel, dim3(nt * (nt + 1) / 2, B), dim3(64), 0, st, n, P, ldp, (long long)n * ldp, Ppk,
                       (long long)qp_ppk_doubles(n), qp_nchp(n));
}

void launch_gram_l2(hipStream_t st, const PqArgs& a, const GramL2& g) {
    // tile rows: the last sub-tile row rides on the diagonal tiles when it would be a 64-tile row's only one
    const int nt = gram_strip_folds(a.n) ? ((a.n + 15) / 16) / 4 : (a.n + GT - 1) / GT;
    const int ntile = nt * (nt + 1) / 2;
    const int nchp = a.Ppk ? qp_nchp(a.n) : 0;
    const bool dop = g.s && g.dop_size > 0;
#define HIPDRT_GRAM(D, R) hipLaunchKernelGGL((gram_kernel<D, R>), dim3(ntile, a.B), dim3(256), 0, st, a.m, a.n, a.A, a.lda, a.w, \
                                             g, a.P, a.ldp, a.p_stride, a.active, ntile, a.Ppk, a.ppk_stride, nchp, a.a_stride)
    if (a.P) { if (dop) HIPDRT_GRAM(true, true); else HIPDRT_GRAM(false, true); }
    else { if (dop) HIPDRT_GRAM(true, false); else HIPDRT_GRAM(false, false); }
#undef HIPDRT_GRAM
}

void launch_qvec(hipStream_t st, const PqArgs& a) {
    // one matrix for the whole batch: a matrix product with a shared operand (hyper.hip: batch_products_kernel), whatever the
    // batch size -- a fit's bits do not depend on how many are fitted beside it; few fits with very large matrices keep the
    // vector kernel (a handful of workgroups would stream all of A)
    if (a.a_stride == 0 && (size_t)a.m * a.n < ((size_t)1 << 20)) {
        launch_qvec_batched(st, a);
        return;
    }
    hipLaunchKernelGGL(qvec_kernel, dim3((a.n + 255) / 256, a.B), dim3(256), 0, st, a.m, a.n, a.A, a.lda, a.w, a.y, a.l1,
                       a.l1_scalar, a.q, a.active, a.a_stride);
}

}  // namespace hipdrt
