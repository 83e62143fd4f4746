// Device arrays between borders of marker bytes, for the test hooks of include/hipdrt_debug.h (debug.hip, and the hooks that sit
// next to kernels no other file can name: map_filter.hip, map_predict.hip).  A hook uploads every in and out array of the
// launcher under test through these, launches, fetches and checks: a border that changed is HIPDRT_E_NUMERIC.
#pragma once
#include <cstring>

#include "plan.hpp"

namespace hipdrt {

struct Guarded {
    static constexpr size_t G = 128;           // border bytes on either side
    static constexpr unsigned char MARK = 0xA5;
    DevBuf buf;
    void* host = nullptr;
    size_t bytes = 0;
    const char* name = "";
    std::vector<unsigned char> stage;
    int up(const char* what, void* h, size_t nbytes, hipStream_t st) {
        name = what; host = h; bytes = nbytes;
        stage.assign(nbytes + 2 * G, MARK);
        if (h) std::memcpy(stage.data() + G, h, nbytes);
        HIPDRT_CHECK(buf.alloc(stage.size()));
        HIPDRT_CHECK(hipMemcpyAsync(buf.p, stage.data(), stage.size(), hipMemcpyHostToDevice, st));
        return 0;
    }
    // an array the kernels only read (or one the hook hands back itself, from data()): uploaded, never copied back by check()
    int up_in(const char* what, const void* h, size_t nbytes, hipStream_t st) {
        TRY(up(what, const_cast<void*>(h), nbytes, st));
        host = nullptr;
        return 0;
    }
    double* dd() const { return reinterpret_cast<double*>(static_cast<unsigned char*>(buf.p) + G); }
    const unsigned char* data() const { return stage.data() + G; }       // what fetch() brought back
    int fetch(hipStream_t st) { HIPDRT_CHECK(hipMemcpyAsync(stage.data(), buf.p, stage.size(), hipMemcpyDeviceToHost, st)); return 0; }
    int check() {
        for (size_t i = 0; i < G; ++i)
            if (stage[i] != MARK || stage[G + bytes + i] != MARK) {
                set_error(std::string("the kernel under test wrote outside ") + name);
                return HIPDRT_E_NUMERIC;
            }
        if (host) std::memcpy(host, stage.data() + G, bytes);
        return 0;
    }
};
// The guarded outputs of one hook, as DevOuts (plan.hpp) holds the plain ones of an entry point: one want() per output, one
// back() after the launch that fetches every array and then checks every border.
struct GuardedOuts {
    static constexpr int MAX = 24;         // hipdrt_debug_hyper_step has 17, the setup hooks (debug_setup.hip) up to 22
    Guarded g[MAX];
    int n = 0;
    template <class T>
    int want(const char* name, T* host, size_t count, T*& field, hipStream_t st) {
        if (!host) return 0;
        HIPDRT_REQUIRE(n < MAX, "internal: more outputs than GuardedOuts holds");
        TRY(g[n].up(name, host, count * sizeof(T), st));
        field = reinterpret_cast<T*>(g[n++].dd());
        return 0;
    }
    // an input: bordered and checked like the outputs, never copied back
    template <class T>
    int in(const char* name, const T* host, size_t count, const T*& field, hipStream_t st) {
        if (!host) return 0;
        HIPDRT_REQUIRE(n < MAX, "internal: more arrays than GuardedOuts holds");
        TRY(g[n].up_in(name, host, count * sizeof(T), st));
        field = reinterpret_cast<const T*>(g[n++].dd());
        return 0;
    }
    int back(hipStream_t st) {
        for (int i = 0; i < n; ++i) TRY(g[i].fetch(st));
        HIPDRT_CHECK(hipStreamSynchronize(st));
        for (int i = 0; i < n; ++i) TRY(g[i].check());
        return 0;
    }
};
// `count` blocks of `blk` doubles, each between two borders of marker bytes: [border][block 0][border][block 1] ... [border].  The
// kernels take the distance between blocks as a stride, so the borders need nothing from them.
struct GuardedBlocks {
    static constexpr size_t GD = Guarded::G / sizeof(double);
    DevBuf buf;
    size_t blk = 0, count = 0;
    int alloc(size_t block_doubles, size_t blocks, hipStream_t st) {
        blk = block_doubles; count = blocks;
        HIPDRT_CHECK(buf.alloc((count + 1) * stride() * sizeof(double)));
        HIPDRT_CHECK(hipMemsetAsync(buf.p, Guarded::MARK, buf.bytes, st));
        return 0;
    }
    size_t stride() const { return blk + GD; }
    double* first() const { return buf.d() + GD; }
    // the count + 1 borders alone come back (the blocks may be tens of megabytes)
    int check(const char* what, hipStream_t st) {
        std::vector<unsigned char> h((count + 1) * Guarded::G);
        HIPDRT_CHECK(hipMemcpy2DAsync(h.data(), Guarded::G, buf.p, stride() * sizeof(double), Guarded::G, count + 1,
                                      hipMemcpyDeviceToHost, st));
        HIPDRT_CHECK(hipStreamSynchronize(st));
        for (size_t i = 0; i < h.size(); ++i)
            if (h[i] != Guarded::MARK) {
                set_error(std::string("the kernel under test wrote outside ") + what + " (border " + std::to_string(i / Guarded::G) + ")");
                return HIPDRT_E_NUMERIC;
            }
        return 0;
    }
};

// The fields of a FitState that are not arrays, as hipdrt_plan::state() fills them for a problem of these sizes: what
// hipdrt_debug_hyper_step and the setup hooks (debug_setup.hip) share.  desc null: not a prepared plan.  No history, no product scratch.
inline FitState debug_fit_state(int nf, int m, int n, int ns, int ldrm, int ldm, bool rm_batched, const hipdrt_fit_opts& opts,
                                const hipdrt_prepared_desc* desc) {
    FitState fs{};
    fs.nf = nf; fs.m = m; fs.n = n; fs.ns = ns; fs.ldrm = ldrm; fs.ldm = ldm;
    fs.toeplitz_m = 0; fs.toep_reach = -1; fs.continue_mode = 0; fs.min_iter = 1; fs.opts = opts;
    fs.prepared = desc ? 1 : 0;
    if (desc) fs.desc = *desc; else fs.desc.vz_index = -1;
    fs.rm_stride = rm_batched ? (long long)m * ldrm : 0;
    fs.hist_b = -1; fs.hist_cap = 0;
    fs.premv = nullptr; fs.premv_batched = 0;
    return fs;
}

}  // namespace hipdrt
