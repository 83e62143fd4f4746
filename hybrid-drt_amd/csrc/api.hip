// C-ABI of libhipdrt.so (include/hipdrt.h): the error string, the library's own streams and the life cycle of a context.
// The rest of the ABI: operators.hip (stand-alone operators), plan.hip (the plan), plan_fit.hip (its device fit loop),
// plan_post.hip and plan_drt.hip (what reads a finished fit), debug.hip (include/hipdrt_debug.h).
#include <algorithm>
#include <cstdlib>
#include <cstring>

#include "plan.hpp"

namespace hipdrt {
static thread_local std::string g_err;
void set_error(const std::string& msg) { g_err = msg; }
}  // namespace hipdrt

extern "C" {

const char* hipdrt_last_error(void) { return g_err.c_str(); }

// what the environment promises about the runtime's hardware-queue count (read when the runtime started; 4 when unset)
static int hw_queues_hint() {
    static const int q = [] { const char* e = std::getenv("GPU_MAX_HW_QUEUES"); const int v = e ? std::atoi(e) : 4; return v > 0 ? std::min(v, 32) : 4; }();
    return q;
}

// ---- the library's own streams ------------------------------------------------------------------------------------------
// The HIP runtime maps streams onto at most GPU_MAX_HW_QUEUES hardware queues (4 unless the environment says otherwise), and two
// launch sequences on ONE queue run one behind the other.  Its rule, read off rocprofv3's queue ids (tools/queue_map_probe.sh,
// profiles/r06_queue_map.txt): queue 1 belongs to the null stream; a new stream gets a NEW queue while fewer than the maximum
// exist, afterwards the LAST queue among those with the fewest streams -- counting idle streams like busy ones.  So the stream that
// fills the pool and the one created right after it share a queue, and any two streams created one pool's length apart do:
//   * four ranges of one plan behind three or five other (idle!) streams land on three queues, two of them back to back:
//     1778 fits/s instead of 2304 (tools/trace_queue_placement.sh, profiles/r06_trace_queue_placement.txt);
//   * two plans in flight whose contexts were created seven streams apart share queue 8: 1730 instead of 2266
//     (profiles/r06_trace_plans_placement.txt);
//   * the "wrapped" placements of profiles/r06_hw_queue_placement.txt (-4 %) and round 5's "three and four ranges flip between
//     fast and slow".
// The library therefore creates its streams ONCE per device -- as many as queues are left beside the null stream's, each on a
// queue of its own when nothing else has created streams before -- and hands them out itself, by ACTIVITY: a context holds one
// for its lifetime (the one with the fewest holders), the ranges of a fit borrow the ones with the fewest device loops running
// for the duration of that fit.  Idle contexts and idle plans no longer push active ones onto shared queues.
// HIPDRT_STREAM_POOL=<n> sets the count (1 ... 32).
extern "C++" {
namespace {
struct StreamPool {
    std::mutex mu;
    std::vector<hipStream_t> st;
    std::vector<int> holders, running;
};

StreamPool* stream_pool(int device) {
    static std::mutex mu;
    static std::vector<std::pair<int, StreamPool*>> pools;         // (never freed: the streams live as long as the process)
    std::lock_guard<std::mutex> lock(mu);
    for (auto& pr : pools) if (pr.first == device) return pr.second;
    int n = std::max(2, hw_queues_hint() - 1);
    if (const char* e = std::getenv("HIPDRT_STREAM_POOL")) { const int v = std::atoi(e); if (v >= 1 && v <= 32) n = v; }
    auto* pl = new StreamPool();
    int before = 0;
    (void)hipGetDevice(&before);
    (void)hipSetDevice(device);
    for (int i = 0; i < n; ++i) {
        hipStream_t st = nullptr;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { (void)hipGetLastError(); break; }
        pl->st.push_back(st);
    }
    (void)hipSetDevice(before);
    pl->holders.assign(pl->st.size(), 0);
    pl->running.assign(pl->st.size(), 0);
    pools.emplace_back(device, pl);
    return pl;
}

// Streams whose queues sit on the same compute pipe of the command processor take turns at dispatching: queues are dealt to
// the four pipes in creation order, so pool streams i and i + 4 are such a pair, and four ranges on queues of pipes 1, 2, 3, 1
// measure 2205 fits/s where pipes 0 ... 3 measure 2300 (profiles/r06_trace_queue_placement.txt, second half: every placement the
// trace shows as "four queues" but slow has two ranges one pipe apart).
constexpr int kPipes = 4;

// the stream for one more device loop: none running on it, the fewest loops running on its pipe, the fewest holders, the lowest index
int pool_pick(const StreamPool& pl) {
    int on_pipe[kPipes] = {0, 0, 0, 0};
    for (int i = 0; i < (int)pl.st.size(); ++i) on_pipe[i % kPipes] += pl.running[i];
    auto better = [&](int a, int b) {
        if (pl.running[a] != pl.running[b]) return pl.running[a] < pl.running[b];
        if (on_pipe[a % kPipes] != on_pipe[b % kPipes]) return on_pipe[a % kPipes] < on_pipe[b % kPipes];
        return pl.holders[a] < pl.holders[b];
    };
    int best = 0;
    for (int i = 1; i < (int)pl.st.size(); ++i) if (better(i, best)) best = i;
    return best;
}

// a context's stream for its lifetime
bool pool_hold(hipdrt_ctx* c) {
    StreamPool* pl = stream_pool(c->device);
    if (pl->st.empty()) return false;
    std::lock_guard<std::mutex> lock(pl->mu);
    int best = 0;
    for (int i = 1; i < (int)pl->st.size(); ++i) if (pl->holders[i] < pl->holders[best]) best = i;
    ++pl->holders[best];
    c->stream = pl->st[best];
    c->pool_idx = best;
    return true;
}
void pool_drop(hipdrt_ctx* c) {
    if (c->pool_idx < 0) return;
    StreamPool* pl = stream_pool(c->device);
    std::lock_guard<std::mutex> lock(pl->mu);
    --pl->holders[c->pool_idx];
    c->pool_idx = -1; c->stream = nullptr;
}
// a device loop starts / ends on stream `idx` (a fit on the context's own stream)
void pool_running(int device, int idx, int delta) {
    if (idx < 0) return;
    StreamPool* pl = stream_pool(device);
    std::lock_guard<std::mutex> lock(pl->mu);
    pl->running[idx] += delta;
}
}  // namespace

namespace hipdrt {
// k streams for the ranges of one fit, the least busy first (more ranges than streams: they repeat)
void pool_borrow(int device, int k, int* idx, hipStream_t* st) {
    StreamPool* pl = stream_pool(device);
    std::lock_guard<std::mutex> lock(pl->mu);
    for (int i = 0; i < k; ++i) {
        idx[i] = pool_pick(*pl);
        ++pl->running[idx[i]];
        st[i] = pl->st[idx[i]];
    }
}
int pool_size(int device) { return (int)stream_pool(device)->st.size(); }
void pool_return(int device, int k, const int* idx) {
    StreamPool* pl = stream_pool(device);
    std::lock_guard<std::mutex> lock(pl->mu);
    for (int i = 0; i < k; ++i) --pl->running[idx[i]];
}
LoopOnContextStream::LoopOnContextStream(hipdrt_ctx* c_) : c(c_) { pool_running(c->device, c->pool_idx, +1); }
LoopOnContextStream::~LoopOnContextStream() { pool_running(c->device, c->pool_idx, -1); }
// (comm.hip: a communicator made before the first context must not take one of the queues the pool would get)
void ensure_stream_pool(int device) { (void)stream_pool(device); }
}  // namespace hipdrt
}

int hipdrt_create(int device, hipdrt_ctx** out) try {
    HIPDRT_REQUIRE(out != nullptr, "out is NULL");
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count <= 0) {
        set_error("no HIP device visible (libhipdrt has no CPU fallback)");
        return HIPDRT_E_NODEVICE;
    }
    HIPDRT_REQUIRE(device >= 0 && device < count, "device index out of range");
    HIPDRT_CHECK(hipSetDevice(device)); (void)hipGetLastError();
    hipDeviceProp_t prop;
    HIPDRT_CHECK(hipGetDeviceProperties(&prop, device));
    std::string arch = prop.gcnArchName;
    if (arch.rfind("gfx950", 0) != 0) {
        set_error("device " + std::to_string(device) + " is " + arch + "; libhipdrt is built for gfx950 only");
        return HIPDRT_E_NODEVICE;
    }
    auto* c = new hipdrt_ctx();
    c->device = device;
    c->num_cu = prop.multiProcessorCount;
    c->hbm_bytes = prop.totalGlobalMem;
    c->arch = arch.substr(0, arch.find(':'));
    if (const char* wv = std::getenv("HIPDRT_QP_WAVES")) {        // (tools/: A/B of the two batch coneqp kernels without a code change)
        const int w = std::atoi(wv);
        if (w == 4 || w == 8) c->qp_waves = w;
    }
    if (!pool_hold(c)) { delete c; set_error("no HIP stream could be created on device " + std::to_string(device)); return HIPDRT_E_HIP; }
    *out = c;
    return HIPDRT_OK;
} HIPDRT_CATCH

extern "C++" {
namespace hipdrt {
std::mutex g_life;                 // context / plan creation and destruction (any thread, e.g. a garbage collector's)

void free_ctx(hipdrt_ctx* ctx) {
    pool_drop(ctx);                    // (the stream itself belongs to the library's pool and lives on)
    delete ctx;
}
}  // namespace hipdrt
}

int hipdrt_destroy(hipdrt_ctx* ctx) try {
    if (!ctx) return HIPDRT_OK;
    std::lock_guard<std::mutex> lk(g_life);
    if (ctx->plans > 0) { ctx->released = true; return HIPDRT_OK; }     // the last plan's destruction frees it
    free_ctx(ctx);
    return HIPDRT_OK;
} HIPDRT_CATCH

void* hipdrt_stream(hipdrt_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int hipdrt_synchronize(hipdrt_ctx* ctx) try {
    HIPDRT_REQUIRE(ctx, "ctx is NULL");
    HIPDRT_CHECK(hipStreamSynchronize(ctx->stream));
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_device_info(hipdrt_ctx* ctx, char* arch, int arch_len, int* num_cu, long long* hbm_bytes) try {
    HIPDRT_REQUIRE(ctx, "ctx is NULL");
    if (arch && arch_len > 0) { std::strncpy(arch, ctx->arch.c_str(), arch_len - 1); arch[arch_len - 1] = 0; }
    if (num_cu) *num_cu = ctx->num_cu;
    if (hbm_bytes) *hbm_bytes = (long long)ctx->hbm_bytes;
    return HIPDRT_OK;
} HIPDRT_CATCH

int hipdrt_debug_stream_pool(hipdrt_ctx* ctx, int cap, void** streams, int* holders, int* running, int* size) try {
    HIPDRT_REQUIRE(ctx && size && cap >= 0, "NULL pointer");
    StreamPool* pl = stream_pool(ctx->device);
    std::lock_guard<std::mutex> lock(pl->mu);
    *size = (int)pl->st.size();
    for (int i = 0; i < std::min(cap, *size); ++i) {
        if (streams) streams[i] = pl->st[i];
        if (holders) holders[i] = pl->holders[i];
        if (running) running[i] = pl->running[i];
    }
    return HIPDRT_OK;
} HIPDRT_CATCH

}  // extern "C"
