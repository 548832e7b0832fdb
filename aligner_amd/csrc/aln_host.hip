// aln_host.hip -- host side of the C ABI declared in include/aligner_hip.h.
//
// The reference's callers own host buffers (Vec<T> per sequence, statistics/mod.rs:255-286; simple/mod.rs:35-40) and get
// owned results back, so the entry points take HOST pointers and everything between them and the kernels lives here:
//
//   plan      per chunk of pairs: validation of the lengths, routing (batch kernel / single-pair kernel), LPT order of the
//             device work queue, layout of the direction, string and tag regions            (chunk_plan)
//   pool      every context owns a few SLOTS: device buffers (grow-only), a stream, pinned staging for the small tables --
//             nothing is hipMalloc'ed per call once the pool is warm                         (Slot, slot_ensure)
//   pipeline  aln_align_batch cuts the batch into chunks of ~1e10 cells in the CALLER's pair order, so that a chunk's
//             residues, summaries and aligned strings are contiguous spans of the caller's buffers: one H2D and two D2H
//             copies per chunk, straight from / into the caller's memory (no bounce, no per-pair memcpy; the runtime moves
//             pageable memory at the link rate, profiles/r02_host_link.txt).  Chunk i+1 is staged and chunk i-1 is fetched
//             (by a second host thread) while chunk i fills; chunks run on different slots = different streams, so the
//             tail of one fill, the traceback behind it and the head of the next fill overlap on the device, and the
//             directions of a chunk only live until its traceback is done (4 x ~2.5 GB instead of 35 GB for C5).
//   staged    aln_batch_* keeps ONE chunk = the whole batch resident in a private slot (inputs in HBM before the timed
//             region: what bench.py's headline measures) -- same plan, same launches.
//
// One context per process per GPU; multi-GPU runs are one process per GPU (the Python driver shards pairs across ranks and
// gathers the 48-byte summaries with RCCL through torch.distributed).  There is NO CPU implementation of the DP here: if the
// device or the kernels are unavailable every entry point fails with ALN_ERR_DEVICE.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cmath>
#include <condition_variable>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <deque>
#include <memory>
#include <mutex>
#include <new>
#include <numeric>
#include <string>
#include <chrono>
#include <thread>
#include <vector>

#include "aln_device.h"
#include "aln_launch.h"
#include "aln_loop_rules.h"
#include "aln_plan_rules.h"
#include "aln_scheme_rules.h"
#include "aln_seqset_rules.h"
#include "aln_best_rules.h"
#include "aln_search_rules.h"
#include "aln_shuffle_rules.h"
#include "aln_signif_rules.h"
#include "aln_report_rules.h"
#include "aln_cluster_rules.h"
#include "aln_prefilter_rules.h"
#include "../../include/aligner_hip_prefilter.h"
#include "aln_wordjoin_rules.h"
#include "aln_strand_rules.h"
#include "../../include/aligner_hip_wordjoin.h"
#include "aln_seedjoin_rules.h"
#include "../../include/aligner_hip_seedjoin.h"
#include "aln_seedchain_rules.h"

#define ALN_TIMING_SLOTS 256u
// HIP multiplexes streams onto 4 hardware queues by default (GPU_MAX_HW_QUEUES): with more slots than that two chunks share a
// queue and wait for each other (measured: 6 slots 67 ms, 4 slots 57 ms for the C5 batch)
#define ALN_POOL_SLOTS 4

static thread_local std::string g_err;

// HIP multiplexes the streams of a process onto GPU_MAX_HW_QUEUES hardware queues (default 4).  A pipelined batch call keeps
// four streams busy at once; when other streams of the process (a framework's, a staged batch's) are mapped onto the same
// queues, two chunks end up in one queue and wait for each other (C5: 52 ms -> 60-63 ms; eight queues remove that,
// profiles/r02_e2e_chunking.txt).  The library does NOT touch the environment (it did in r02: a constructor that called setenv in
// someone else's process): a host that runs other streams beside batch calls exports GPU_MAX_HW_QUEUES=8 itself before the HIP
// runtime initialises -- bench.py and the test harness do ("Environment").

static int fail(hipError_t e, const char *what)
{
    char buf[256];
    snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    g_err = buf;
    return e == hipErrorOutOfMemory ? ALN_ERR_OOM : ALN_ERR_DEVICE;
}
#define HIPCHK(call)                                         \
    do {                                                     \
        hipError_t e_ = (call);                              \
        if (e_ != hipSuccess) return fail(e_, #call);        \
    } while (0)

static double wall_ms(const std::chrono::steady_clock::time_point &t0)
{
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
}

// what the last call on a resident handle (scan, pair set, sequence set) took and moved: aln_*_stats
struct CallStats {
    double ms[4] = {0, 0, 0, 0};      // three kernel times, as the family's header comment names them, and the call's wall time
    uint64_t bytes[2] = {0, 0};       // host -> device, device -> host
};
static void stats_reset(CallStats &s) { s = CallStats(); }
static int stats_get(const CallStats *s, double *ms, uint64_t *bytes)
{
    if (!s) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (ms) for (int i = 0; i < 4; ++i) ms[i] = s->ms[i];
    if (bytes) { bytes[0] = s->bytes[0]; bytes[1] = s->bytes[1]; }
    return ALN_OK;
}

// ---------------------------------------------------------------- grow-only buffers
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};
static int dev_ensure(DevBuf &b, size_t bytes, bool slack)
{
    bytes = std::max<size_t>(bytes, 256);
    if (b.cap >= bytes) return ALN_OK;
    if (b.p) { (void)hipFree(b.p); b.p = nullptr; b.cap = 0; }
    size_t want = slack ? bytes + bytes / 8 : bytes;
    hipError_t e = hipMalloc(&b.p, want);
    if (e != hipSuccess && want != bytes) { want = bytes; e = hipMalloc(&b.p, want); }
    if (e != hipSuccess) { b.p = nullptr; return fail(e, "hipMalloc"); }
    b.cap = want;
    return ALN_OK;
}
static void dev_free(DevBuf &b)
{
    if (b.p) (void)hipFree(b.p);
    b.p = nullptr; b.cap = 0;
}
// the tile buffer of an ordered selection (aln_select.h): `tiles` offsets (the wider words first: aligned), then as many counts
template <class Off> static int tiles_ensure(DevBuf &b, uint64_t tiles, uint32_t **tile_count, Off **tile_off)
{
    const int st = dev_ensure(b, (sizeof(Off) + 4) * tiles, false);
    if (st != ALN_OK) return st;
    *tile_off = b.as<Off>();
    *tile_count = reinterpret_cast<uint32_t *>(*tile_off + tiles);
    return ALN_OK;
}
struct PinBuf {
    void *p = nullptr;
    size_t cap = 0;
    template <class T> T *as() const { return reinterpret_cast<T *>(p); }
};
static int pin_ensure(PinBuf &b, size_t bytes)
{
    bytes = std::max<size_t>(bytes, 4096);
    if (b.cap >= bytes) return ALN_OK;
    if (b.p) { (void)hipHostFree(b.p); b.p = nullptr; b.cap = 0; }
    const size_t want = bytes + bytes / 4;
    hipError_t e = hipHostMalloc(&b.p, want, hipHostMallocDefault);
    if (e != hipSuccess) { b.p = nullptr; return fail(e, "hipHostMalloc"); }
    b.cap = want;
    return ALN_OK;
}
static void pin_free(PinBuf &b)
{
    if (b.p) (void)hipHostFree(b.p);
    b.p = nullptr; b.cap = 0;
}

// ---------------------------------------------------------------- a slot: everything one chunk needs on the device
struct Slot {
    bool pooled = true;       // pool slots keep some slack when they grow; a staged batch's private slot is sized exactly
    DevBuf seqs, descs, order, counter, walked, dirs, results, tb, tags, scratch, matrix, pwm_words, hmat;
    DevBuf granules, advice1, cand, ctrl, tbmap, unpack, repair, coop;
    DevBuf shuffle;           // shuffle calls (aln_shuffle_*): pair table | f of every copy | first failed copy per pair
    PinBuf h_meta;            // descs + order + matrix + pwm words (small, truly asynchronous H2D)
    PinBuf h_in, h_out;       // fallback staging: sequences gathered from scattered offsets / strings for a foreign tb layout
    hipStream_t stream = nullptr;
    hipStream_t tb_stream = nullptr;                 // in-kernel overlapped traceback (staged batches)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_done = nullptr, ev_fill = nullptr;
    uint32_t epoch = 0;
    bool walked_clean = false;
    // fast batch kernels: the boundary rows in `scratch` hold tagged granules (aln_coop_tag); the tag's salt counts this slot's
    // launches, and the rows are cleared whenever the buffer is new or the salt's 10 bits wrap
    uint32_t salt = 0;
    bool scratch_clean = false;
};

// one GPU of a context: its properties and its slot pool
struct DevCtx {
    int device = 0;
    int cus = 0;
    size_t hbm = 0;
    char name[128] = {0};
    std::mutex mu;                                   // guards the pool
    std::condition_variable cv;
    Slot *slots[ALN_POOL_SLOTS] = {nullptr};
    bool busy[ALN_POOL_SLOTS] = {false};
};

// A context spans one or more GPUs of this process (aln_create: one; aln_create_multi: a list).  Single calls go to the
// devices in turn; a batch call is cut into chunks that the devices take from a common queue.
struct aln_ctx {
    std::vector<DevCtx *> devs;
    std::atomic<uint32_t> turn{0};
    DevCtx *next_device() { return devs[turn.fetch_add(1, std::memory_order_relaxed) % devs.size()]; }
};

static int slot_init(Slot &s)
{
    if (!s.stream) HIPCHK(hipStreamCreateWithFlags(&s.stream, hipStreamNonBlocking));
    if (!s.ev_done) HIPCHK(hipEventCreateWithFlags(&s.ev_done, hipEventDisableTiming));
    if (!s.ev_fill) HIPCHK(hipEventCreateWithFlags(&s.ev_fill, hipEventDisableTiming));
    return ALN_OK;
}
static void slot_destroy(Slot *s)
{
    if (!s) return;
    DevBuf *d[] = {&s->seqs, &s->descs, &s->order, &s->counter, &s->walked, &s->dirs, &s->results, &s->tb, &s->tags, &s->scratch,
                   &s->matrix, &s->pwm_words, &s->hmat, &s->granules, &s->advice1, &s->cand, &s->ctrl, &s->tbmap, &s->unpack, &s->repair, &s->coop,
                   &s->shuffle};
    for (DevBuf *b : d) dev_free(*b);
    pin_free(s->h_meta); pin_free(s->h_in); pin_free(s->h_out);
    if (s->ev_fork) (void)hipEventDestroy(s->ev_fork);
    if (s->ev_join) (void)hipEventDestroy(s->ev_join);
    if (s->ev_done) (void)hipEventDestroy(s->ev_done);
    if (s->ev_fill) (void)hipEventDestroy(s->ev_fill);
    if (s->tb_stream) (void)hipStreamDestroy(s->tb_stream);
    if (s->stream) (void)hipStreamDestroy(s->stream);
    delete s;
}

// takes between 1 and `want` free pool slots (blocks while none is free); concurrent callers share the pool
static int pool_lease(DevCtx *ctx, int want, Slot **out)
{
    std::unique_lock<std::mutex> lk(ctx->mu);
    int got = 0;
    for (;;) {
        for (int i = 0; i < ALN_POOL_SLOTS && got < want; ++i)
            if (!ctx->busy[i]) {
                if (!ctx->slots[i]) ctx->slots[i] = new Slot();
                ctx->busy[i] = true;
                out[got++] = ctx->slots[i];
            }
        if (got) return got;
        ctx->cv.wait(lk);
    }
}
static void pool_release(DevCtx *ctx, Slot **slots, int n)
{
    {
        std::lock_guard<std::mutex> lk(ctx->mu);
        for (int k = 0; k < n; ++k)
            for (int i = 0; i < ALN_POOL_SLOTS; ++i)
                if (ctx->slots[i] == slots[k]) ctx->busy[i] = false;
    }
    ctx->cv.notify_all();
}

extern "C" const char *aln_last_error(void) { return g_err.c_str(); }
extern "C" int aln_abi_version(void) { return ALN_ABI_VERSION; }

// aln_create's warm-up: what a first call used to pay for (26-31 ms for a first 1000 x 1000 pair against 0.4 ms for the second;
// aligner-cli aligns ONE pair per process, aligner-cli/main.rs:41-53).  Per device: the code objects are loaded (one per kernel
// translation unit, aln_warm_*), and one synthetic 1000 x 1000 pair goes through aln_align_pair -- pool slot 0 with its stream,
// events and staging, the buffers of the single-pair route at the size of the usual pair, the first launch of every kernel on
// that route.  ALN_NO_WARMUP=1 leaves all of it to the first call as before.  A failure here is not an error of aln_create: the
// first real call meets the same condition and reports it.
static void warm_context(aln_ctx *c)
{
    if (getenv("ALN_NO_WARMUP")) return;
    const uint32_t L = 1000;
    std::vector<uint8_t> q(L), t(L);
    uint32_t x = 12345u;
    for (uint32_t i = 0; i < L; ++i) {
        x = x * 1664525u + 1013904223u; q[i] = (uint8_t)((x >> 16) % 20u);
        x = x * 1664525u + 1013904223u; t[i] = (i % 3u) ? q[i] : (uint8_t)((x >> 16) % 20u);
    }
    std::vector<double> mat(20 * 20);
    for (int i = 0; i < 20; ++i) for (int j = 0; j < 20; ++j) mat[i * 20 + j] = i == j ? 5.0 : -2.0;
    aln_params p;
    memset(&p, 0, sizeof p);
    p.semantics = ALN_CORE_LOCAL; p.del = 11.0; p.ext = 2.0;
    p.matrix = mat.data(); p.rows = 20; p.cols = 20; p.row_stride = 20;
    p.outputs = ALN_OUT_SCORE | ALN_OUT_TRACEBACK;
    std::vector<uint8_t> qa(2 * L + 2), ta(2 * L + 2);
    for (size_t d = 0; d < c->devs.size(); ++d) {
        if (hipSetDevice(c->devs[d]->device) != hipSuccess) continue;
        (void)aln_warm_single(); (void)aln_warm_tb(); (void)aln_warm_generic();
        (void)aln_warm_fast_cl(); (void)aln_warm_fast_cl_solo(); (void)aln_warm_fast_rest(); (void)aln_warm_fast_rest_solo();
        (void)aln_warm_best(); (void)aln_warm_search(); (void)aln_warm_profile(); (void)aln_warm_msa(); (void)aln_warm_cigar(); (void)aln_warm_wordjoin(); (void)aln_warm_seedjoin(); (void)aln_warm_seedchain();
        aln_pair_result r;
        (void)aln_align_pair(c, &p, q.data(), L, t.data(), L, &r, qa.data(), ta.data(), nullptr, nullptr);   // devices in turn
    }
    c->turn.store(0);
    (void)hipGetLastError();
    g_err.clear();
}

extern "C" aln_ctx *aln_create_multi(int n_devices, const int *device_ids, int *status)
{
    int st = ALN_OK;
    aln_ctx *c = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) {
        g_err = e != hipSuccess ? std::string("hipGetDeviceCount: ") + hipGetErrorString(e) : "no HIP device visible";
        st = ALN_ERR_DEVICE;
    } else if (n_devices < 0 || n_devices > 64 || (n_devices > 0 && !device_ids)) {
        g_err = "bad device list";
        st = ALN_ERR_INVALID_ARGUMENT;
    } else {
        std::vector<int> ids;
        if (n_devices == 0) for (int i = 0; i < ndev; ++i) ids.push_back(i);          // every visible device
        else ids.assign(device_ids, device_ids + n_devices);
        c = new aln_ctx();
        for (int id : ids) {
            if (id < 0 || id >= ndev) { g_err = "device id out of range"; st = ALN_ERR_INVALID_ARGUMENT; break; }
            hipDeviceProp_t prop;
            if ((e = hipSetDevice(id)) != hipSuccess || (e = hipGetDeviceProperties(&prop, id)) != hipSuccess) {
                st = fail(e, "hipSetDevice/hipGetDeviceProperties");
                break;
            }
            DevCtx *d = new DevCtx();
            d->device = id;
            d->cus = prop.multiProcessorCount;
            d->hbm = prop.totalGlobalMem;
            snprintf(d->name, sizeof d->name, "%s (%s)", prop.name, prop.gcnArchName);
            c->devs.push_back(d);
        }
        if (st != ALN_OK) {
            for (DevCtx *d : c->devs) delete d;
            delete c;
            c = nullptr;
        }
    }
    if (c) warm_context(c);
    if (status) *status = st;
    return c;
}

extern "C" aln_ctx *aln_create(int device_id, int *status) { return aln_create_multi(1, &device_id, status); }

extern "C" void aln_destroy(aln_ctx *ctx)
{
    if (!ctx) return;
    for (DevCtx *d : ctx->devs) {
        (void)hipSetDevice(d->device);
        for (Slot *s : d->slots) slot_destroy(s);
        delete d;
    }
    delete ctx;
}

extern "C" int aln_device_count(const aln_ctx *ctx) { return ctx ? (int)ctx->devs.size() : 0; }

extern "C" int aln_device_info(aln_ctx *ctx, int *cus, size_t *hbm, char *name, size_t cap)
{
    if (!ctx) return ALN_ERR_INVALID_ARGUMENT;
    const DevCtx *d = ctx->devs[0];
    if (cus) *cus = d->cus;
    if (hbm) *hbm = d->hbm;
    if (name && cap) { strncpy(name, d->name, cap - 1); name[cap - 1] = 0; }
    return ALN_OK;
}

// ---------------------------------------------------------------- per call: arguments of perform_alignment, analysed once
struct Call {
    aln_params p{};
    bool pwm = false, core = false;
    uint32_t rows = 0, cols = 0;
    std::vector<double> md;           // the matrix, compact row-major
    bool all_int = false;
    double maxabs = 0, smin = 0, smax = 0;
    uint32_t outs = 0;
    bool store_dirs = true, want_tb = true, want_h = false;
    bool is_int = true, fast = false; // decided from the whole batch (the longest pair), the same for every chunk
    double unscale = 1.0;             // dyadic schemes on the integer kernels: scores come back multiplied by this (2^-k), see call_init
    int semantics = 0;                // what the kernels run (PWM runs as CORE_LOCAL with position-specific scoring)
    const double *pair_matrices = nullptr;   // aln_pairset_run: DEVICE array, one rows x cols matrix per pair of the call (lean f64 kernel only)
};

static int call_init(Call &c, const aln_params *p, const uint64_t *q_len, const uint64_t *t_len, size_t n, bool want_h)
{
    if (!p) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (p->semantics < ALN_CORE_GLOBAL || p->semantics > ALN_PWM_LOCAL) { g_err = "bad semantics"; return ALN_ERR_INVALID_ARGUMENT; }
    c.p = *p;
    c.pwm = p->semantics == ALN_PWM_LOCAL;
    c.core = p->semantics == ALN_CORE_GLOBAL || p->semantics == ALN_CORE_LOCAL || c.pwm;
    c.semantics = c.pwm ? ALN_CORE_LOCAL : p->semantics;       // same recurrence and tie rules; only the score lookup differs
    // simple/mod.rs:49-51 / :175-177
    if (c.core && p->heuristics_present) return ALN_ERR_UNNECESSARY_ARGUMENT;
    if (!p->matrix || p->rows == 0 || p->cols == 0) { g_err = "matrix missing"; return ALN_ERR_INVALID_ARGUMENT; }
    if (c.pwm && p->rows != 4) return ALN_ERR_MATRIX_SHAPE;                    // pwm/mod.rs:40-42
    // the matrix lives in LDS: 32 KiB next to the query profiles; a position-weight matrix (no profiles in LDS) may be
    // 4 x 2000 wide (62.5 KiB as f64)
    if (!aln_matrix_fits(c.pwm, p->rows, p->cols)) {
        g_err = c.pwm ? "position-weight matrix larger than 8000 entries (4 x 2000)" : "substitution matrix larger than 4096 entries";
        return ALN_ERR_UNSUPPORTED;
    }
    if (n > 0xFFFFFFF0ull) { g_err = "too many pairs"; return ALN_ERR_UNSUPPORTED; }
    c.rows = p->rows; c.cols = p->cols;
    const int64_t rs = p->row_stride ? p->row_stride : (int64_t)c.cols;
    c.md.resize((size_t)c.rows * c.cols);
    for (uint32_t r = 0; r < c.rows; ++r)
        for (uint32_t k = 0; k < c.cols; ++k) c.md[(size_t)r * c.cols + k] = p->matrix[(int64_t)r * rs + k];
    AlnScheme sch = aln_scheme_scan(c.core, p->del, p->ext, c.md.data(), c.md.size());
    c.all_int = sch.all_int;
    if (!c.core && !c.all_int) { g_err = "legacy semantics are i32: del and matrix must be integral"; return ALN_ERR_INVALID_ARGUMENT; }
    if (!c.core && p->force_f64) { g_err = "legacy semantics have no f64 form"; return ALN_ERR_UNSUPPORTED; }
    c.outs = p->outputs ? p->outputs : (ALN_OUT_SCORE | ALN_OUT_TRACEBACK);
    c.store_dirs = (c.outs & (ALN_OUT_TRACEBACK | ALN_OUT_DIRECTIONS)) != 0;
    c.want_tb = (c.outs & ALN_OUT_TRACEBACK) != 0;
    c.want_h = want_h;
    uint64_t max_span = 0;
    for (size_t i = 0; i < n; ++i) {
        if (q_len[i] > 0x7FFFFFF0ull || t_len[i] > 0x7FFFFFF0ull) { g_err = "sequence too long"; return ALN_ERR_UNSUPPORTED; }
        const uint64_t N = c.pwm ? c.cols : q_len[i], M = t_len[i];
        if (N && M) max_span = std::max(max_span, N + M + 2);
    }
    // Dyadic schemes: when every penalty and score is a multiple of 2^-k (BLOSUM62 in half-bits, del 11.5 ...), the scheme times 2^k
    // is an integer scheme with the same maxima, the same ties and the same zeros -- in the reference's f64 every H is an exact
    // multiple of 2^-k, two candidates differ by 0 or by >= 2^-k > f64::EPSILON, and H == 0 means the same -- so the integer kernels
    // fill it (three times the f64 kernels' rate) and the two scores of every summary are scaled back, exactly, by one small kernel
    // behind the traceback.  Not with the H output (the dump is what the kernels computed), not when f64 is asked for.
    // ALN_NO_DYADIC=1: off.  The classification itself (bounds included) is aln_scheme_rules.h.
    aln_scheme_dyadic(sch, c.core, p->force_f64, want_h, getenv("ALN_NO_DYADIC") != nullptr, p->del, p->ext, c.md.data(), c.md.size(),
                      max_span);
    if (sch.scale != 1.0) {
        for (double &v : c.md) v *= sch.scale;
        c.p.del *= sch.scale; c.p.ext *= sch.scale;
        c.unscale = 1.0 / sch.scale;
    }
    // integer kernels are exact iff every value is integral and |H| cannot leave i32; fast integer kernels: keys are
    // 4*H + tag in i32, the profile holds 4*s - 2 as int8, and S + four waves' profiles (cols x 512 B each) have to fit the 64 KiB
    // of LDS a workgroup gets without an opt-in
    aln_scheme_route(sch, c.pwm, c.rows, c.cols, max_span, p->force_f64, want_h, p->force_serial, p->force_generic, ALN_FULL_R);
    c.all_int = sch.all_int;
    c.maxabs = sch.maxabs; c.smin = sch.smin; c.smax = sch.smax;
    c.is_int = sch.is_int;
    if (!c.core && !c.is_int) { g_err = "legacy scores overflow i32 for these lengths"; return ALN_ERR_UNSUPPORTED; }
    c.fast = sch.fast;
    return ALN_OK;
}

// ---------------------------------------------------------------- per chunk: descriptors, routing, layout (aln_plan_rules.h)
// the facts of a call that the plan reads
static AlnPlanCall plan_call(const Call &c)
{
    AlnPlanCall pc;
    pc.pwm = c.pwm; pc.fast = c.fast; pc.is_int = c.is_int;
    pc.want_h = c.want_h; pc.want_tb = c.want_tb; pc.store_dirs = c.store_dirs;
    pc.semantics = c.semantics;
    pc.hazard = c.semantics == ALN_CORE_LOCAL && c.p.del != c.p.ext;
    pc.force_serial = c.p.force_serial != 0;
    pc.pair_matrices = c.pair_matrices != nullptr;
    pc.rows = c.rows; pc.cols = c.cols;
    return pc;
}

// The plan's settings (AlnPlanKnobs), read from the environment at every plan -- tests change them inside one process -- but for two:
// ALN_COOP_LEAN (unset = aln_coop_lean_plan decides, 0 = the cooperative build wherever a chunk could share, 1 = the lean build
// there.  Unlike ALN_NO_COOP -- no cooperative passes at all, which also routes large pairs as if nothing could be shared -- it only
// picks the kernel build: routing, grid, claim runs and two pairs per wave are decided as without it) and
// ALN_TRACE_PLAN (=1: one stderr line per chunk that could share -- which build it runs, and the figures that decided it, "aln plan:"
// -- and one per planned chunk that names its route, "aln route:": pairs of the batch kernel, of the single-pair route, of the
// one-workgroup route, two pairs per wave, overlapped traceback, shared passes, kernel family) are read once per process.
static bool trace_plan()
{
    static const bool v = getenv("ALN_TRACE_PLAN") != nullptr;
    return v;
}
static AlnPlanKnobs plan_knobs()
{
    static const int coop_lean = [] { const char *e = getenv("ALN_COOP_LEAN"); return e ? (atoi(e) != 0 ? 1 : 0) : -1; }();
    auto flag = [](const char *name) { return getenv(name) != nullptr; };
    auto num = [](const char *name) { AlnKnob k; if (const char *e = getenv(name)) { k.set = true; k.v = atoi(e); } return k; };
    AlnPlanKnobs kn;
    kn.coop_lean = coop_lean;
    kn.trace_plan = trace_plan();
    kn.single_r = num("ALN_SINGLE_R");
    kn.no_single = flag("ALN_NO_SINGLE");
    kn.no_coop = flag("ALN_NO_COOP");
    kn.big_to_single = num("ALN_BIG_TO_SINGLE");
    kn.no_wgpipe = flag("ALN_NO_WGPIPE");
    kn.wg_r = num("ALN_WG_R");
    kn.tb_overlap = num("ALN_TB_OVERLAP");
    kn.tb_overlap_any = flag("ALN_TB_OVERLAP_ANY");
    if (const char *e = getenv("ALN_COOP_TAIL")) { kn.coop_tail.set = true; kn.coop_tail.v = (long long)strtoull(e, nullptr, 10); }
    kn.chain_wgs = num("ALN_CHAIN_WGS");
    kn.fill_wgs = num("ALN_FILL_WGS");
    kn.no_duo = flag("ALN_NO_DUO");
    if (const char *e = getenv("ALN_CHUNK_CELLS")) { kn.chunk_cells_set = true; kn.chunk_cells = atof(e); }
    return kn;
}

// allow_overlap: the chunk has the device to itself (a single-chunk call, a staged batch).  many_chunks: one of more than four
// chunks of a pipelined call.
static int chunk_plan(const DevCtx *ctx, const Call &c, const uint64_t *q_off, const uint64_t *q_len, const uint64_t *t_off,
                      const uint64_t *t_len, size_t first, size_t n, bool allow_overlap, Chunk &k, bool many_chunks = false)
{
    const AlnPlanKnobs kn = plan_knobs();
    AlnShareTrace tr;
    aln_plan_chunk((uint32_t)ctx->cus, plan_call(c), kn, q_off, q_len, t_off, t_len, first, n, allow_overlap, many_chunks, k, &tr);
    if (kn.trace_plan) {
        const AlnLeanPlan &lp = tr.lp;
        if (tr.could_share)
            fprintf(stderr, "aln plan: pairs %zu waves %llu resident %llu tail %llu share %.4g tail_cost %llu max_cost %llu build %s\n", k.n_small,
                    (unsigned long long)lp.waves, (unsigned long long)lp.resident, (unsigned long long)lp.tail, lp.share,
                    (unsigned long long)aln_pair_cost(k.descs[k.order[lp.tail]]), (unsigned long long)aln_pair_cost(k.descs[k.order[0]]), lp.lean ? "lean" : "coop");
        // for every planned chunk: which route serves it (a score pass brings no flags word back)
        fprintf(stderr, "aln route: pairs %zu small %zu single %zu wg %zu duo %d overlap %d share %s kernels %s\n", n, k.n_small,
                k.single_pairs.size(), k.wg_pairs.size(), k.duo_qo ? 1 : 0, k.overlap ? 1 : 0, k.coop ? "coop" : k.coop_lean ? "lean" : "none",
                c.fast ? "fast" : c.is_int ? "int" : "f64");
    }
    return ALN_OK;
}

// A planned chunk whose residues are resident: pair i's lie at qo[i] / to[i] of one device buffer of seq_span bytes, which is there
// already and must not grow.  The descriptors (the device's, and the host's copy that the launches of pairs routed off the batch
// kernel read) carry those offsets, and nothing is staged.
static void chunk_resident(Chunk &k, const uint64_t *qo, const uint64_t *to, size_t n, uint64_t seq_span)
{
    for (size_t i = 0; i < n; ++i) { k.descs[i].q_off = qo[i]; k.descs[i].t_off = to[i]; }
    k.seq_direct = true; k.seq_lo = 0; k.seq_span = seq_span;
}

// device buffers of a slot for this chunk (grow-only; nothing happens once the pool is warm)
// small_meta (window scans): the descriptors and the queue are built on the device, so the pinned staging holds the matrix only
static int slot_ensure(Slot &s, const Call &c, const Chunk &k, const AlnPlanBounds *need = nullptr, bool small_meta = false)
{
    int st;
    const bool sl = s.pooled;
#define ENS(buf, bytes) if ((st = dev_ensure(s.buf, (bytes), sl)) != ALN_OK) return st
    if (need) {
        ENS(seqs, need->seq_span + 64);
        ENS(descs, need->n * sizeof(PairDesc));
        ENS(order, need->n * sizeof(uint32_t));
        ENS(results, need->n * sizeof(aln_pair_result));
        ENS(dirs, need->dir_bytes);
        ENS(tb, need->tb_bytes);
        ENS(tags, need->tag_bytes);
        ENS(scratch, need->scratch);
        if (need->coop) ENS(coop, need->coop);
    }
    ENS(seqs, k.seq_span + 64);
    ENS(descs, k.n * sizeof(PairDesc));
    ENS(order, k.n * sizeof(uint32_t));
    ENS(counter, k.counter_bytes);
    if (k.coop) ENS(coop, k.coop_bytes);
    if (k.overlap) {
        const size_t before = s.walked.cap;
        ENS(walked, 4ull * k.n);
        if (s.walked.cap != before) s.walked_clean = false;
        if (!s.tb_stream) HIPCHK(hipStreamCreateWithFlags(&s.tb_stream, hipStreamNonBlocking));
        if (!s.ev_fork) HIPCHK(hipEventCreateWithFlags(&s.ev_fork, hipEventDisableTiming));
        if (!s.ev_join) HIPCHK(hipEventCreateWithFlags(&s.ev_join, hipEventDisableTiming));
    }
    ENS(dirs, k.dir_bytes);
    ENS(results, k.n * sizeof(aln_pair_result));
    ENS(tb, k.tb_bytes);
    ENS(tags, k.tag_bytes);
    {
        const size_t before = s.scratch.cap;
        const void *before_p = s.scratch.p;
        ENS(scratch, std::max<uint64_t>((uint64_t)k.grid * 4 * k.scratch_stride, k.wg_pairs.empty() ? 0 : ((uint64_t)k.max_len + 66) * 8));
        if (s.scratch.cap != before || s.scratch.p != before_p) s.scratch_clean = false;
    }
    if (!k.wg_pairs.empty()) ENS(tbmap, k.tbmap_entries * 16);
    ENS(matrix, (uint64_t)c.rows * c.cols * (c.is_int ? 4 : 8));
    if (c.pwm && c.fast) ENS(pwm_words, (uint64_t)c.cols * 4);
    if (c.want_h) ENS(hmat, k.hmat_elems * (c.is_int ? 4 : 8));
    if (!k.single_pairs.empty()) {
        ENS(granules, k.granule_bytes);
        ENS(advice1, 2ull * single_advice_bytes(k.single_max_n));
        ENS(cand, 16ull * (k.single_max_n + 64));
        ENS(ctrl, 256);
        ENS(tbmap, k.tbmap_entries * 16);
        // localized repair of the single-pair route: up to 8 strips' scratch granule rows, checkpoints, candidates
        ENS(repair, 8ull * (k.granule_stride_max * 4 + 18 * 64 * 4 + 32) + 256);
    }
#undef ENS
    // pinned staging of the small tables: descs | order | matrix | pwm words
    const size_t meta = (small_meta ? 0 : std::max<size_t>(k.n, need ? need->n : 0) * (sizeof(PairDesc) + 4)) + (size_t)c.rows * c.cols * 8 + (size_t)c.cols * 4 + 256;
    if ((st = pin_ensure(s.h_meta, meta)) != ALN_OK) return st;
    if (!small_meta && !k.seq_direct && (st = pin_ensure(s.h_in, k.seq_span + 64)) != ALN_OK) return st;
    return slot_init(s);
}

// H2D of the call's matrix (and of the PWM column words of the fast kernels) through pinned staging at `m`
static int upload_matrix(Slot &s, const Call &c, uint8_t *m, hipStream_t st)
{
    size_t o = 0;
    const size_t nm = c.md.size();
    if (nm == 0) return ALN_OK;        // per-pair matrices (aln_pairset_run): the call has none of its own
    if (c.is_int) {
        int32_t *mi = reinterpret_cast<int32_t *>(m + o);
        for (size_t i = 0; i < nm; ++i) mi[i] = (int32_t)c.md[i];
        HIPCHK(hipMemcpyAsync(s.matrix.p, mi, nm * 4, hipMemcpyHostToDevice, st));
    } else {
        memcpy(m + o, c.md.data(), nm * 8);
        HIPCHK(hipMemcpyAsync(s.matrix.p, m + o, nm * 8, hipMemcpyHostToDevice, st));
    }
    o += nm * 8;
    if (c.pwm && c.fast) {
        uint32_t *words = reinterpret_cast<uint32_t *>(m + o);
        for (uint32_t x = 0; x < c.cols; ++x) {
            uint32_t wv = 0;
            for (uint32_t r = 0; r < 4; ++r) wv |= ((uint32_t)(int32_t)(4 * (int32_t)c.md[(size_t)r * c.cols + x] - 2) & 0xffu) << (8 * r);
            words[x] = wv;
        }
        HIPCHK(hipMemcpyAsync(s.pwm_words.p, words, (size_t)c.cols * 4, hipMemcpyHostToDevice, st));
    }
    return ALN_OK;
}

// H2D of one chunk on the slot's stream.  The residues come straight out of the caller's buffer (one span); the small tables
// go through pinned memory.  Returns when the copies are queued (the span copy of pageable memory is staged by the runtime).
static int slot_upload(Slot &s, const Call &c, const Chunk &k, const uint8_t *seqs, const uint64_t *q_off, const uint64_t *q_len,
                       const uint64_t *t_off, const uint64_t *t_len, hipStream_t st, bool staged = false, bool seqs_there = false)
{
    uint8_t *m = s.h_meta.as<uint8_t>();
    size_t o = 0;
    if (k.n) {
        memcpy(m + o, k.descs.data(), k.n * sizeof(PairDesc));
        HIPCHK(hipMemcpyAsync(s.descs.p, m + o, k.n * sizeof(PairDesc), hipMemcpyHostToDevice, st));
        o += k.n * sizeof(PairDesc);
        if (!k.order.empty()) {
            memcpy(m + o, k.order.data(), k.order.size() * 4);
            HIPCHK(hipMemcpyAsync(s.order.p, m + o, k.order.size() * 4, hipMemcpyHostToDevice, st));
        }
        o += k.n * 4;
    }
    o = (o + 15) & ~(size_t)15;
    int e = upload_matrix(s, c, m + o, st);
    if (e != ALN_OK) return e;
    if (k.seq_span && !seqs_there) {
        if (k.seq_direct) {
            HIPCHK(hipMemcpyAsync(s.seqs.p, seqs + k.seq_lo, k.seq_span, hipMemcpyHostToDevice, st));
        } else {
            uint8_t *h = s.h_in.as<uint8_t>();
            for (size_t i = 0; i < k.n && !staged; ++i) {     // staged: the caller has filled h_in already (aln_align_pair)
                const size_t g = k.first + i;
                if (!c.pwm && q_len[g]) memcpy(h + k.descs[i].q_off, seqs + q_off[g], q_len[g]);
                if (t_len[g]) memcpy(h + k.descs[i].t_off, seqs + t_off[g], t_len[g]);
            }
            HIPCHK(hipMemcpyAsync(s.seqs.p, h, k.seq_span, hipMemcpyHostToDevice, st));
        }
    }
    return ALN_OK;
}

// All kernels of one chunk, asynchronous on `st`: validation of the residue codes, fill (+ exact re-fills), traceback.
// ev (optional): three timing events (fill start, fill end, traceback end).
// fill_after (optional): an event the fill has to wait for (pipelined calls: the fill of the chunk two before, see below).
static int slot_launch(DevCtx *ctx, Slot &s, const Call &c, const Chunk &k, hipStream_t st, hipEvent_t *ev, uint32_t *fill_launches,
                       hipEvent_t fill_after = nullptr)
{
    if (fill_launches) *fill_launches = 0;
    if (k.n == 0) return ALN_OK;
    if (k.n_small) HIPCHK(hipMemsetAsync(s.counter.p, 0, k.counter_bytes, st));     // the batch kernel's work queue
    if (k.n_small && k.coop) HIPCHK(hipMemsetAsync(s.coop.p, 0, k.coop_bytes, st)); // counters, claim words (zero = nothing to claim), records
    if (k.n_small && c.fast) {
        s.salt = (s.salt + 1u) & 0x3ffu;
        if (!s.scratch_clean || s.salt == 0u) { HIPCHK(hipMemsetAsync(s.scratch.p, 0, s.scratch.cap, st)); s.scratch_clean = true; }
    }
    // residue codes outside the matrix: the batch fill kernels check the pairs they take; the single-pair route reads the status
    // from the descriptor, so its pairs are checked by a kernel of their own in front
    if (!k.single_pairs.empty())
        aln_launch_validate(s.seqs.as<uint8_t>(), s.descs.as<PairDesc>(), (uint32_t)k.n, c.rows, c.cols, c.pwm ? 1 : 0, st);
    FillArgs fa{};
    fa.seqs = s.seqs.as<uint8_t>(); fa.descs = s.descs.as<PairDesc>(); fa.order = s.order.as<uint32_t>(); fa.n_pairs = (uint32_t)k.n_small;
    fa.counter = s.counter.as<uint32_t>(); fa.dirs = s.dirs.as<uint8_t>(); fa.results = s.results.as<aln_pair_result>();
    fa.scratch = s.scratch.as<uint8_t>(); fa.scratch_stride = k.scratch_stride; fa.max_len = k.max_len; fa.zrow_bytes = k.zrow_bytes;
    fa.cascade_rows = k.cascade_rows;
    fa.matrix = s.matrix.p; fa.rows = c.rows; fa.cols = c.cols; fa.prof_stride = k.prof_stride;
    fa.del = c.p.del; fa.ext = c.p.ext; fa.semantics = c.semantics;
    fa.max_passes = c.p.max_passes; fa.force_serial = c.p.force_serial;
    fa.no_repair = getenv("ALN_NO_REPAIR") ? 1u : 0u;
    fa.f64_old = getenv("ALN_F64_OLD") ? 1u : 0u;
    if (c.pair_matrices) { fa.matrix = c.pair_matrices + k.first * ((size_t)c.rows * c.cols); fa.pair_matrices = 1u; fa.f64_old = 0u; }
    fa.max_cells = k.max_cells;
    fa.store_dirs = c.store_dirs ? 1u : 0u;
    fa.pwm = c.pwm ? 1u : 0u;
    fa.pwm_words = s.pwm_words.as<uint32_t>();
    fa.hmat = c.want_h ? s.hmat.p : nullptr; fa.blank = c.p.blank_code;
    fa.n_descs = (uint32_t)k.n;
    // ALN_BACK_WAVES=1 (experiment, off): the youngest wave of every SIMD takes its pairs from the back of the queue (next_pair2).
    // Measured on the 8-way shard of C5: fill 6.47-6.61 ms with it, 6.25 without -- the short pairs it moves to the slow waves are
    // what filled the gaps at the end; r02 had seen the same with a queue in two segments.
    { const char *e = getenv("ALN_BACK_WAVES"); fa.back_waves = (e && atoi(e) && k.grid == (uint32_t)ctx->cus * 3u && k.n_small >= 2ull * k.grid * 4u) ? 1u : 0u; }
    fa.coop = k.coop ? s.coop.as<uint32_t>() : nullptr; fa.coop_waves = k.grid * 4u; fa.coop_tail = k.coop_tail; fa.salt = s.salt;
    { const char *e = getenv("ALN_COOP_LINGER"); fa.coop_linger = e ? (uint32_t)atoi(e) : (k.coop_linger ? 1u : 0u); }
    { const char *e = getenv("ALN_COOP_DEBUG"); fa.coop_debug = e ? (uint32_t)atoi(e) : 0u; }
    { const char *e = getenv("ALN_FAIR"); fa.fair = e ? (uint32_t)atoi(e) : 0u; }
    { const char *e = getenv("ALN_CK_LAST"); fa.ck_last = (e && atoi(e) == 512) ? 512u : ALN_CK_LAST; }
    fa.duo_qo = k.duo_qo;
    // runs of queue positions per atomic: only where pairs are many, short and alike (one strip, <= 2^18 cells), nothing is shared
    // and the queue is not two-ended; about 1.6 runs per wave or more, so that the last round stays as even as with single pairs
    fa.claim = 1;
    if (c.fast && !k.coop && !k.coop_lean && !fa.back_waves && k.max_cells <= (1ull << 18) && k.n_small != 0) {
        // (queue units per resident wave; two pairs per wave: a unit is two pairs)
        const double per_wave = (double)(k.duo_qo ? (k.n_small + 1) / 2 : k.n_small) / ((double)std::min(k.grid, (uint32_t)ctx->cus * 3u) * 4.0);
        // (measured: C3, 3.3 pairs per wave: runs of 2 fill 0.232 -> 0.204 ms, runs of 3 / 4 0.218 / 0.222 -- the last round gets uneven;
        // 100 000 PWM windows, 32 per wave: runs of 4 cost 4 % -- with many pairs per wave the waves drift apart by themselves)
        fa.claim = (per_wave >= 3.2 && per_wave < 12.0) ? 2u : 1u;
    }
    if (const char *e = getenv("ALN_CLAIM")) fa.claim = (uint32_t)std::max(1, std::min(8, atoi(e)));
    if (fill_after) HIPCHK(hipStreamWaitEvent(st, fill_after, 0));
    if (ev) HIPCHK(hipEventRecord(ev[0], st));
    uint32_t launches = 0;
    TraceArgs ta{};
    ta.seqs = s.seqs.as<uint8_t>(); ta.descs = s.descs.as<PairDesc>(); ta.n_pairs = (uint32_t)k.n; ta.dirs = s.dirs.as<uint8_t>();
    ta.results = s.results.as<aln_pair_result>(); ta.tb = s.tb.as<uint8_t>(); ta.tags = s.tags.as<uint8_t>();
    ta.semantics = c.semantics; ta.blank = c.p.blank_code; ta.pwm = c.pwm ? 1 : 0;
    const bool overlap = k.overlap;
    if (overlap) {
        if (!s.walked_clean) { HIPCHK(hipMemsetAsync(s.walked.p, 0, s.walked.cap, st)); s.walked_clean = true; s.epoch = 0; }
        fa.doneq = s.counter.as<uint32_t>() + 64;
        ta.walked = s.walked.as<uint32_t>(); ta.epoch = ++s.epoch; ta.n_order = (uint32_t)k.n_small;
        ta.doneq = s.counter.as<uint32_t>() + 64; ta.head = s.counter.as<uint32_t>() + 2; ta.wait_ticks = 50000000ull;   // 0.5 s
        if (const char *w = getenv("ALN_TB_WAIT_US")) ta.wait_ticks = 100ull * strtoull(w, nullptr, 10);   // testing: 0 = give up at once
        HIPCHK(hipEventRecord(s.ev_fork, st));                                // after the memsets, before the fill
    }
    if (k.n_small) {
        aln_launch_fill(&fa, c.is_int ? 1 : 0, c.fast ? 1 : 0, k.grid, k.lds_bytes, st);
        HIPCHK(hipGetLastError());
        launches = 1;
    }
    if (overlap) {                                                            // submitted after the fill, runs beside it
        HIPCHK(hipStreamWaitEvent(s.tb_stream, s.ev_fork, 0));
        aln_launch_traceback_overlap(&ta, k.tb_waves, s.tb_stream);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(s.ev_join, s.tb_stream));
    }
    for (size_t j = 0; j < k.single_pairs.size(); ++j) {
        const PairDesc &d = k.descs[k.single_pairs[j]];
        SingleArgs sa{};
        sa.seqs = s.seqs.as<uint8_t>(); sa.descs = s.descs.as<PairDesc>(); sa.pair = k.single_pairs[j]; sa.dirs = s.dirs.as<uint8_t>();
        sa.results = s.results.as<aln_pair_result>(); sa.granules = s.granules.as<uint32_t>();
        sa.gstride = ((uint64_t)d.N + 64 + 63) & ~63ull;
        sa.advice = s.advice1.as<uint8_t>(); sa.zrow = s.advice1.as<uint8_t>() + single_advice_bytes(k.single_max_n);
        sa.cand = s.cand.as<int32_t>(); sa.ctrl = s.ctrl.as<uint32_t>(); sa.matrix = s.matrix.p;
        sa.rows = c.rows; sa.cols = c.cols; sa.del = c.p.del; sa.ext = c.p.ext;
        sa.semantics = c.semantics; sa.R = k.single_r[j];
        sa.ns = (d.M + 64 * sa.R - 1) / (64 * sa.R);
        sa.hazard = (sa.semantics == ALN_CORE_LOCAL && sa.del != sa.ext && d.N >= 2) ? 1u : 0u;
        sa.store_dirs = c.store_dirs ? 1u : 0u;
        { const char *td = getenv("ALN_TEST_DROP_STRIP"); sa.test_drop = td ? (uint32_t)atoi(td) : 0u; }
        if (getenv("ALN_TEST_FAIL_REPAIR")) sa.test_drop = 0xffffffffu;      // the repair run is declared failed (tests)
        sa.max_passes = sa.hazard ? std::min<uint32_t>(c.p.max_passes ? c.p.max_passes : 4u, 12u) : 1u;
        // Localized repair (hazard pairs): when pass 0's advice is wrong in leading columns only, the first rep_S strips re-run
        // their leading columns (strip s up to step rep_K + 64 (rep_S - 1 - s)) instead of the whole pipeline running again.
        sa.rep_S = 0; sa.rep_K = 0; sa.mode = 0;
        {
            const uint32_t S = sa.R >= 2 ? 4u : 8u, K = 256u;
            if (sa.hazard && !getenv("ALN_NO_SINGLE_REPAIR") && sa.R <= 2 && sa.ns > S && d.N >= K + 64u * S + 128u) { sa.rep_S = S; sa.rep_K = K; }
            uint8_t *rb = s.repair.as<uint8_t>();
            sa.rgranules = reinterpret_cast<uint32_t *>(rb);
            sa.ckpt = reinterpret_cast<int *>(rb + 8ull * k.granule_stride_max * 4);
            sa.rcand = reinterpret_cast<int32_t *>(rb + 8ull * k.granule_stride_max * 4 + 8ull * 18 * 64 * 4);
        }
        aln_launch_single_init(&sa, (uint32_t)single_advice_bytes(d.N), st);
        // the granule rows must read "not yet produced" before a pass: one memset here, later passes are zeroed by the
        // finalize kernel that arms them
        HIPCHK(hipMemsetAsync(s.granules.p, 0, (size_t)sa.ns * sa.gstride * 4, st));
        for (uint32_t pass = 0; pass < sa.max_passes; ++pass) {
            sa.pass = pass;
            aln_launch_single(&sa, d.N, pass + 1 == sa.max_passes ? 1 : 0, st);
            launches++;
            if (pass == 0 && sa.rep_S) aln_launch_single_repair(&sa, d.N, st);      // exits at once unless pass 0 armed it
        }
        HIPCHK(hipGetLastError());
    }
    for (size_t j = 0; j < k.wg_pairs.size(); ++j) {
        const PairDesc &d = k.descs[k.wg_pairs[j]];
        WgArgs wa{};
        wa.seqs = s.seqs.as<uint8_t>(); wa.descs = s.descs.as<PairDesc>(); wa.pair = k.wg_pairs[j]; wa.dirs = s.dirs.as<uint8_t>();
        wa.results = s.results.as<aln_pair_result>(); wa.matrix = s.matrix.p; wa.rows = c.rows; wa.cols = c.cols;
        wa.del = c.p.del; wa.ext = c.p.ext; wa.semantics = c.semantics; wa.R = k.wg_r[j]; wa.ns = (d.M + 64 * wa.R - 1) / (64 * wa.R);
        wa.max_passes = c.p.max_passes; wa.store_dirs = c.store_dirs ? 1u : 0u; wa.scratch = s.scratch.as<uint8_t>();
        wa.hmat = c.want_h ? s.hmat.p : nullptr;
        wa.pwm = c.pwm ? 1u : 0u;
        aln_launch_wgpipe(&wa, c.is_int ? 1 : 0, aln_wg_lds_bytes(c.rows, c.cols, c.is_int ? 4u : 8u, wa.ns, d.N), st);
        launches++;
        HIPCHK(hipGetLastError());
    }
    if (ev) HIPCHK(hipEventRecord(ev[1], st));
    if (s.ev_fill) HIPCHK(hipEventRecord(s.ev_fill, st));
    if (c.want_tb && c.store_dirs) {
        if (overlap) HIPCHK(hipStreamWaitEvent(st, s.ev_join, 0));
        // every pair except those in the uniform-R layout (handled below); pairs the single-pair route hands to the strict-order
        // kernel (row-major layout) are walked by these two as well
        const bool batch_tb = k.n_small != 0 || c.semantics == ALN_CORE_LOCAL || !k.wg_pairs.empty();
        if (batch_tb) {
            // few pairs: one WAVE per pair, its lanes fetching the direction quads ahead of the path (tb_walk_pair_wave: the walk of
            // 256 pairs of 4200 x 4200 3.7 -> ~1 ms); many pairs: one lane per pair, 64 walks in flight per wave.  ALN_TB_WAVE=0 / 1
            // forces one or the other.
            // (up to 4095 pairs when they are long: 3000 C5 pairs host to host 5.27 -> 4.56 ms, 3072 pairs of 4200 x 4200 27.8 -> 26.3;
            // from 4096 pairs on the walks of such batches run beside the fill)
            bool wave_walk = k.n <= 2048 || (k.n < 4096 && k.max_len >= 1024);
            if (const char *e = getenv("ALN_TB_WAVE")) wave_walk = atoi(e) != 0;
            if (wave_walk) aln_launch_traceback_wave(&ta, st);
            else aln_launch_traceback(&ta, st);
        }
        for (size_t j = 0; j < k.single_pairs.size(); ++j) {
            const PairDesc &d = k.descs[k.single_pairs[j]];
            TraceSingleArgs tsa{};
            tsa.seqs = s.seqs.as<uint8_t>(); tsa.descs = s.descs.as<PairDesc>(); tsa.pair = k.single_pairs[j]; tsa.dirs = s.dirs.as<uint8_t>();
            tsa.results = s.results.as<aln_pair_result>(); tsa.tb = s.tb.as<uint8_t>(); tsa.tags = s.tags.as<uint8_t>();
            tsa.semantics = c.semantics;
            tsa.R = k.single_r[j]; tsa.ns = (d.M + 64 * tsa.R - 1) / (64 * tsa.R);
            tsa.map = s.tbmap.as<uint4>(); tsa.seg = s.tbmap.as<uint4>() + (uint64_t)tsa.ns * (d.N + 1);
            aln_launch_traceback_single(&tsa, d.N, st);
            aln_launch_traceback_expand_single(&ta, tsa.pair, st);
        }
        for (size_t j = 0; j < k.wg_pairs.size(); ++j) {      // the same parallel traceback for the pairs one workgroup filled
            const PairDesc &d = k.descs[k.wg_pairs[j]];
            TraceSingleArgs tsa{};
            tsa.seqs = s.seqs.as<uint8_t>(); tsa.descs = s.descs.as<PairDesc>(); tsa.pair = k.wg_pairs[j]; tsa.dirs = s.dirs.as<uint8_t>();
            tsa.results = s.results.as<aln_pair_result>(); tsa.tb = s.tb.as<uint8_t>(); tsa.tags = s.tags.as<uint8_t>();
            tsa.semantics = c.semantics;
            tsa.R = k.wg_r[j]; tsa.ns = (d.M + 64 * tsa.R - 1) / (64 * tsa.R);
            tsa.map = s.tbmap.as<uint4>(); tsa.seg = s.tbmap.as<uint4>() + (uint64_t)tsa.ns * (d.N + 1);
            tsa.pwm = c.pwm ? 1u : 0u;
            aln_launch_traceback_single(&tsa, d.N, st);
            aln_launch_traceback_expand_single(&ta, tsa.pair, st);
        }
        if (batch_tb) aln_launch_traceback_expand(&ta, st);
        HIPCHK(hipGetLastError());
    }
    if (c.unscale != 1.0) { aln_launch_scale_results(s.results.as<aln_pair_result>(), (uint32_t)k.n, c.unscale, st); HIPCHK(hipGetLastError()); }
    if (ev) HIPCHK(hipEventRecord(ev[2], st));
    if (fill_launches) *fill_launches = launches;
    return ALN_OK;
}

// diagnostics (ALN_COOP_STATS): the control words of the cooperative passes after a run
static void coop_stats_slot(Slot &s, const Chunk &k)
{
    if (k.coop && getenv("ALN_COOP_STATS")) {
        uint32_t w[256] = {0};
        if (hipMemcpy(w, s.coop.p, sizeof w, hipMemcpyDeviceToHost) == hipSuccess) {
            if (w[14]) {
                fprintf(stderr, "coop: %u strips left rows without their tag; the first: N %u, strip %u of %u, R %u, own %u, open %u; columns (tag found):", w[14], w[16], (w[15] >> 4), w[17] >> 8,
                        w[15] & 15u, w[17] & 1u, (w[17] >> 1) & 1u);
                for (int i = 0; i < 40 && w[128 + i]; ++i) fprintf(stderr, " %u(%#x)", w[128 + i], w[192 + i]);
                fprintf(stderr, "\n");
            }
            fprintf(stderr, "coop: urgent passes %u, unclaimed strips now %d urgent %d lazy, finished %u, strips helped %u, scans %u, aborted passes %u, spins waiting for strips to finish %u; "
                    "strips that gave up waiting for the row above %u, owners that gave up waiting for a strip %u, bottom-row records not found %u, pair granules not found %u\n",
                    w[ALN_COOP_ULOGW], (int)w[ALN_COOP_UOPEN], (int)w[ALN_COOP_LOPEN], w[ALN_COOP_FINISHED], w[ALN_COOP_HELPED], w[ALN_COOP_SCANS], w[ALN_COOP_ABORTS], w[9],
                    w[10], w[11], w[12], w[13]);
        }
    }
}
// ALN_TRACE_TB=1 (read once): one stderr line per chunk whose results are down -- how the parallel traceback crossed the strips of the
// last pair of the chunk that went through aln_launch_traceback_single ("aln tb:": the chunk's pair index, rows per lane, strips, and
// per strip the class aln_tb_single_chain_kernel left in seg[s].w: 0 not visited, 1 the end cell's own strip, 2 by its exit-map entry,
// 3 entered outside the band, 4 inside the band but the map's walk had given up).  Unset: no copy, no synchronisation.
static bool trace_tb()
{
    static const bool v = getenv("ALN_TRACE_TB") != nullptr;
    return v;
}
static void trace_tb_slot(Slot &s, const Call &c, const Chunk &k)
{
    if (!trace_tb() || !(c.want_tb && c.store_dirs) || (k.single_pairs.empty() && k.wg_pairs.empty())) return;
    const bool wg = !k.wg_pairs.empty();                       // launched after the single-pair route's pairs (slot_launch)
    const uint32_t pair = wg ? k.wg_pairs.back() : k.single_pairs.back(), R = wg ? k.wg_r.back() : k.single_r.back();
    const PairDesc &d = k.descs[pair];
    const uint32_t ns = (d.M + 64 * R - 1) / (64 * R);
    std::vector<uint32_t> seg(4 * (size_t)ns);
    if (hipMemcpy(seg.data(), s.tbmap.as<uint4>() + (uint64_t)ns * (d.N + 1), seg.size() * 4, hipMemcpyDeviceToHost) != hipSuccess) return;
    std::string digits(ns, '0');
    for (uint32_t i = 0; i < ns; ++i) digits[i] = (char)('0' + (seg[4 * (size_t)i + 3] < 10u ? seg[4 * (size_t)i + 3] : 9u));
    fprintf(stderr, "aln tb: pair %u R %u strips %u classes %s\n", pair, R, ns, digits.c_str());
}
// D2H of one chunk on `st`, then a stream sync: summaries into results[first ..], strings into tb_buf.  When the caller's
// tb_off is the documented cumulative layout the chunk's strings are ONE span of tb_buf and are copied there directly;
// any other layout goes through pinned staging and one memcpy per string.
static int slot_download(Slot &s, const Call &c, const Chunk &k, hipStream_t st, aln_pair_result *results, uint8_t *tb_buf,
                         const uint64_t *tb_off)
{
    if (k.n == 0) return ALN_OK;
    HIPCHK(hipMemcpyAsync(results + k.first, s.results.p, k.n * sizeof(aln_pair_result), hipMemcpyDeviceToHost, st));
    const bool want = tb_buf && tb_off && c.store_dirs && c.want_tb && k.tb_bytes;
    bool direct = want;
    if (want) {
        const uint64_t base = tb_off[k.first];
        for (size_t i = 0; i < k.n && direct; ++i) direct = tb_off[k.first + i] - base == k.descs[i].tb_off && tb_off[k.first + i] >= base;
        if (direct) HIPCHK(hipMemcpyAsync(tb_buf + base, s.tb.p, k.tb_bytes, hipMemcpyDeviceToHost, st));
        else {
            int e = pin_ensure(s.h_out, k.tb_bytes);
            if (e != ALN_OK) return e;
            HIPCHK(hipMemcpyAsync(s.h_out.p, s.tb.p, k.tb_bytes, hipMemcpyDeviceToHost, st));
        }
    }
    HIPCHK(hipStreamSynchronize(st));
    coop_stats_slot(s, k);
    trace_tb_slot(s, c, k);
    if (want && !direct) {
        const uint8_t *h = s.h_out.as<uint8_t>();
        for (size_t i = 0; i < k.n; ++i) {
            const PairDesc &d = k.descs[i];
            const aln_pair_result &r = results[k.first + i];
            if (r.status != ALN_OK) continue;
            const uint64_t cap = (uint64_t)d.N + d.M + 2;
            uint8_t *dst = tb_buf + tb_off[k.first + i];
            if (c.pwm) {   // u32 column numbers, then the residue string
                memcpy(dst, h + d.tb_off, 4ull * r.aln_len);
                memcpy(dst + 4 * cap, h + d.tb_off + 4 * cap, r.aln_len);
            } else {
                memcpy(dst, h + d.tb_off, r.aln_len);
                memcpy(dst + cap, h + d.tb_off + cap, r.aln_len);
            }
        }
    }
    return ALN_OK;
}

// ---------------------------------------------------------------- chunking of a batch call (aln_make_chunks, aln_plan_rules.h)
// The chunking aln_align_batch would use for these lengths on a context of n_devices GPUs: pure host arithmetic (no device is
// touched), exported so that the sharding can be inspected and tested anywhere.  Returns the number of chunks; writes up to
// `cap` (first pair, pair count) entries.
extern "C" size_t aln_plan_chunks(const aln_params *params, const uint64_t *q_len, const uint64_t *t_len, size_t n_pairs,
                                  int n_devices, uint64_t *first, uint64_t *count, size_t cap)
{
    if (!params || (n_pairs && (!q_len || !t_len)) || n_devices < 1) return 0;
    Call c;
    if (call_init(c, params, q_len, t_len, n_pairs, false) != ALN_OK) {      // lengths only (no matrix): planned as for the fast kernels
        c = Call();
        c.pwm = params->semantics == ALN_PWM_LOCAL;
        c.cols = params->cols;
        c.fast = true;
    }
    std::vector<std::pair<size_t, size_t>> ranges;
    if (n_pairs) aln_make_chunks(plan_call(c), plan_knobs(), q_len, t_len, n_pairs, (size_t)n_devices, ranges);
    for (size_t i = 0; i < ranges.size() && i < cap; ++i) {
        if (first) first[i] = ranges[i].first;
        if (count) count[i] = ranges[i].second;
    }
    return ranges.size();
}

// everything a pipelined call shares between its threads
struct BatchJob {
    const Call *c;
    const uint8_t *seqs;
    const uint64_t *q_off, *q_len, *t_off, *t_len;
    aln_pair_result *results;
    uint8_t *tb_buf;
    const uint64_t *tb_off;
    const std::vector<std::pair<size_t, size_t>> *ranges;
    AlnPlanBounds need;            // upper bounds over the chunks: every slot is sized once (aln_plan_bounds)
    std::atomic<size_t> next{0};       // the chunk queue: devices take the next range when they have a free slot
    std::atomic<int> failed{0};
    std::mutex mu;
    int status = ALN_OK;
    std::string err;
    void fail_with(int st, const std::string &e)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (status == ALN_OK) { status = st; err = e; }
        failed.store(1);
    }
};

// One device's share of a pipelined call: this thread takes chunks from the job's queue, plans, uploads and launches them; a
// second thread waits for each chunk's kernels and copies its results back; a slot is reused once its chunk has been fetched.
static void device_pipeline(DevCtx *dev, BatchJob &job)
{
    if (hipSetDevice(dev->device) != hipSuccess) { job.fail_with(ALN_ERR_DEVICE, "hipSetDevice failed"); return; }
    const Call &c = *job.c;
    const size_t nc = job.ranges->size();
    Slot *slots[ALN_POOL_SLOTS];
    const int ns = pool_lease(dev, ALN_POOL_SLOTS, slots);
    struct Release { DevCtx *c; Slot **s; int n; ~Release() { pool_release(c, s, n); } } rel{dev, slots, ns};
    struct Shared {
        std::mutex mu;
        std::condition_variable cv;
        std::deque<std::pair<size_t, int>> ready;      // (local chunk number, slot) launched, to be fetched, in order
        std::vector<char> slot_free;
        bool done_issuing = false;
    } sh;
    sh.slot_free.assign(ns, 1);
    static thread_local std::vector<Chunk> plans_tl;   // (kept from call to call: see Chunk::reset)
    if (plans_tl.size() < (size_t)ns) plans_tl.resize(ns);
    std::vector<Chunk> &plans = plans_tl;              // the plan of the chunk each slot holds
    size_t depth = 3;
    if (const char *e = getenv("ALN_FILL_DEPTH")) depth = std::max(1, atoi(e));
    std::thread fetcher([&] {
        (void)hipSetDevice(dev->device);
        for (;;) {
            int si;
            {
                std::unique_lock<std::mutex> lk(sh.mu);
                sh.cv.wait(lk, [&] { return !sh.ready.empty() || sh.done_issuing; });
                if (sh.ready.empty()) return;
                si = sh.ready.front().second;
                sh.ready.pop_front();
            }
            Slot &s = *slots[si];
            const int e = slot_download(s, c, plans[si], s.stream, job.results, job.tb_buf, job.tb_off);
            if (e != ALN_OK) job.fail_with(e, g_err);
            {
                std::lock_guard<std::mutex> lk(sh.mu);
                sh.slot_free[si] = 1;
            }
            sh.cv.notify_all();
        }
    });
    int st = ALN_OK;
    for (size_t li = 0; st == ALN_OK && !job.failed.load(); ++li) {
        const int si = (int)(li % (size_t)ns);
        {   // the slot's previous chunk must have been fetched before its plan and buffers are reused
            std::unique_lock<std::mutex> lk(sh.mu);
            sh.cv.wait(lk, [&] { return sh.slot_free[si] != 0; });
        }
        const size_t ci = job.next.fetch_add(1);
        if (ci >= nc) break;
        Chunk &k = plans[si];
        k.reset();
        Slot &s = *slots[si];
        // the first chunk of this pipeline: nothing runs yet, so its residues go up on a helper thread while it is planned (as in a
        // one-chunk call); every later chunk is planned and uploaded while the chunks before it fill
        std::thread copier;
        hipError_t copy_err = hipSuccess;
        AlnSeqSpan span;
        bool early = false;
        if (li == 0 && !getenv("ALN_NO_EARLY_UPLOAD")) {
            const size_t f0 = (*job.ranges)[ci].first, f1 = f0 + (*job.ranges)[ci].second;
            for (size_t i = f0; i < f1; ++i) span.add_pair(c.pwm, job.q_off[i], job.q_len[i], job.t_off[i], job.t_len[i]);
            early = span.direct() && span.extent() >= (4u << 20) && span.extent() <= job.need.seq_span;
            if (early) {
                if ((st = slot_init(s)) != ALN_OK || (st = dev_ensure(s.seqs, job.need.seq_span + 64, s.pooled)) != ALN_OK) break;
                copier = std::thread([&] {
                    copy_err = hipSetDevice(dev->device);
                    if (copy_err == hipSuccess) copy_err = hipMemcpyAsync(s.seqs.p, job.seqs + span.lo, span.extent(), hipMemcpyHostToDevice, s.stream);
                });
            }
        }
        struct Join { std::thread &t; ~Join() { if (t.joinable()) t.join(); } } join{copier};
        // (walk waves beside the LAST chunk's own fill, as a staged batch has them, were measured: 53.7 ms against 52.0 without)
        st = chunk_plan(dev, c, job.q_off, job.q_len, job.t_off, job.t_len, (*job.ranges)[ci].first, (*job.ranges)[ci].second, false, k, nc > 4);
        if (st != ALN_OK) break;
        if ((st = slot_ensure(s, c, k, &job.need)) != ALN_OK) break;
        if (copier.joinable()) copier.join();
        if (copy_err != hipSuccess) { st = fail(copy_err, "hipMemcpyAsync(residues)"); break; }
        const bool seqs_there = early && k.seq_direct && k.seq_lo == span.lo && k.seq_span == span.extent();
        if ((st = slot_upload(s, c, k, job.seqs, job.q_off, job.q_len, job.t_off, job.t_len, s.stream, false, seqs_there)) != ALN_OK) break;
        // At most `depth` fills share the chip: chunk i's fill waits for the fill of chunk i - depth.  With every slot's fill
        // started at once the chunks run in lockstep -- they share the chip equally, reach their tails together (a chunk's
        // largest pairs take as long as the whole chunk), then all walk and copy while nothing fills.  Fewer at a time stay
        // staggered: the oldest is in its tail while the younger ones fill the waves it leaves free (C5, 16 chunks: depth
        // 1: 83 ms, 2: 53.7, 3: 52.6, 4 = every slot: 56.5).
        hipEvent_t after = (li >= depth && ns > (int)depth) ? slots[(li - depth) % (size_t)ns]->ev_fill : nullptr;
        if ((st = slot_launch(dev, s, c, k, s.stream, nullptr, nullptr, after)) != ALN_OK) break;
        {
            std::lock_guard<std::mutex> lk(sh.mu);
            sh.slot_free[si] = 0;
            sh.ready.emplace_back(li, si);
        }
        sh.cv.notify_all();
    }
    if (st != ALN_OK) job.fail_with(st, g_err);
    {
        std::lock_guard<std::mutex> lk(sh.mu);
        sh.done_issuing = true;
    }
    sh.cv.notify_all();
    fetcher.join();
    for (int i = 0; i < ns; ++i) (void)hipStreamSynchronize(slots[i]->stream);
}

extern "C" int aln_align_batch(aln_ctx *ctx, const aln_params *params, const uint8_t *seqs, const uint64_t *q_off,
                               const uint64_t *q_len, const uint64_t *t_off, const uint64_t *t_len, size_t n_pairs,
                               aln_pair_result *results, uint8_t *tb_buf, const uint64_t *tb_off)
{
    if (!ctx || !params || (n_pairs && (!seqs || !q_off || !q_len || !t_off || !t_len || !results))) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    Call c;
    int st = call_init(c, params, q_len, t_len, n_pairs, false);
    if (st != ALN_OK) return st;
    if (n_pairs == 0) return ALN_OK;
    std::vector<std::pair<size_t, size_t>> ranges;
    aln_make_chunks(plan_call(c), plan_knobs(), q_len, t_len, n_pairs, ctx->devs.size(), ranges, 12.0 * (double)ctx->devs[0]->cus);
    const size_t nc = ranges.size();

    if (nc == 1) {                                   // one chunk: everything on the caller's thread, on the next device in turn
        DevCtx *dev = ctx->next_device();
        HIPCHK(hipSetDevice(dev->device));
        Slot *sl[1];
        pool_lease(dev, 1, sl);
        struct Release { DevCtx *c; Slot **s; ~Release() { pool_release(c, s, 1); } } rel{dev, sl};
        static thread_local Chunk k_tl;              // (kept from call to call: see Chunk::reset)
        Chunk &k = k_tl;
        k.reset();
        Slot &s = *sl[0];
        // ALN_TRACE_CALL=1: where the wall clock of a one-chunk call goes (stderr)
        const bool trace = getenv("ALN_TRACE_CALL") != nullptr;
        auto now = [] { return std::chrono::steady_clock::now(); };
        auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        const auto t0 = now();
        // The residues do not wait for the plan: where they lie is a min / max over the offsets (AlnSeqSpan, as the plan's),
        // and copying pageable memory keeps the calling thread busy for its whole length (0.55 ms for the 27 MB of 12 500 C5 pairs,
        // beside 0.7 ms of planning) -- a helper thread copies while this one plans.
        AlnSeqSpan span;
        for (size_t i = 0; i < n_pairs; ++i) span.add_pair(c.pwm, q_off[i], q_len[i], t_off[i], t_len[i]);
        const uint64_t lo = span.lo, hi = span.hi;
        const bool early = span.direct() && span.extent() >= (4u << 20) && !getenv("ALN_NO_EARLY_UPLOAD");
        std::thread copier;
        hipError_t copy_err = hipSuccess;
        if (early) {
            if ((st = slot_init(s)) != ALN_OK || (st = dev_ensure(s.seqs, hi - lo + 64, s.pooled)) != ALN_OK) return st;
            copier = std::thread([&] {
                copy_err = hipSetDevice(dev->device);
                if (copy_err == hipSuccess) copy_err = hipMemcpyAsync(s.seqs.p, seqs + lo, hi - lo, hipMemcpyHostToDevice, s.stream);
            });
        }
        struct Join { std::thread &t; ~Join() { if (t.joinable()) t.join(); } } join{copier};
        if ((st = chunk_plan(dev, c, q_off, q_len, t_off, t_len, 0, n_pairs, true, k)) != ALN_OK) return st;
        const auto t1 = now();
        if ((st = slot_ensure(s, c, k)) != ALN_OK) return st;        // (the residue buffer has its size already: it is not moved)
        const auto t2 = now();
        if (copier.joinable()) copier.join();
        if (copy_err != hipSuccess) return fail(copy_err, "hipMemcpyAsync(residues)");
        const bool seqs_there = early && k.seq_direct && k.seq_lo == lo && k.seq_span == hi - lo;
        if ((st = slot_upload(s, c, k, seqs, q_off, q_len, t_off, t_len, s.stream, false, seqs_there)) != ALN_OK) return st;
        const auto t3 = now();
        if ((st = slot_launch(dev, s, c, k, s.stream, nullptr, nullptr)) != ALN_OK) { (void)hipStreamSynchronize(s.stream); return st; }
        const auto t4 = now();
        if (trace) (void)hipStreamSynchronize(s.stream);
        const auto t5 = now();
        st = slot_download(s, c, k, s.stream, results, tb_buf, tb_off);
        if (trace) fprintf(stderr, "aln_align_batch (one chunk, %zu pairs): plan %.3f ensure %.3f upload %.3f launch %.3f kernels %.3f download %.3f ms\n",
                           n_pairs, ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, t4), ms(t4, t5), ms(t5, now()));
        return st;
    }

    BatchJob job;
    job.c = &c; job.seqs = seqs; job.q_off = q_off; job.q_len = q_len; job.t_off = t_off; job.t_len = t_len;
    job.results = results; job.tb_buf = tb_buf; job.tb_off = tb_off; job.ranges = &ranges;
    {   // upper bounds over the chunks: every slot is sized once, before the pipeline runs
        int max_cus = 0;
        for (const DevCtx *d : ctx->devs) max_cus = std::max(max_cus, d->cus);
        const AlnPlanCall pc = plan_call(c);
        for (const auto &r : ranges) job.need.raise(aln_plan_bounds((uint32_t)max_cus, pc, q_off, q_len, t_off, t_len, r.first, r.second));
    }
    // ---- the devices of the context take the chunks from one queue; device 0's pipeline runs on the caller's thread
    const size_t nd = std::min(ctx->devs.size(), nc);
    std::vector<std::thread> others;
    for (size_t d = 1; d < nd; ++d) others.emplace_back([&, d] { device_pipeline(ctx->devs[d], job); });
    device_pipeline(ctx->devs[0], job);
    for (auto &t : others) t.join();
    if (job.status != ALN_OK) { g_err = job.err; return job.status; }
    return ALN_OK;
}

// ---------------------------------------------------------------- staged batch: one chunk resident in a private slot
struct aln_batch {
    DevCtx *ctx = nullptr;           // a staged batch lives on ONE device: the context's first
    Call call;
    Chunk k;
    Slot *slot = nullptr;
    hipStream_t last_stream = nullptr;
    // timing ring: one event triple per run (fill start, fill end, traceback end), recorded on the launch stream
    bool timing = false;
    std::vector<hipEvent_t> ev;
    uint32_t ev_runs = 0;
    uint32_t fill_launches = 0;
};

static void batch_free(aln_batch *b)
{
    if (!b) return;
    (void)hipSetDevice(b->ctx->device);
    for (auto &e : b->ev) if (e) (void)hipEventDestroy(e);
    slot_destroy(b->slot);
    delete b;
}

extern "C" void aln_batch_destroy(aln_batch *b) { batch_free(b); }

extern "C" aln_batch *aln_batch_create(aln_ctx *ctx, const aln_params *params, const uint8_t *seqs,
                                       const uint64_t *q_off, const uint64_t *q_len, const uint64_t *t_off,
                                       const uint64_t *t_len, size_t n_pairs, int *status)
{
    int st = ALN_OK;
    aln_batch *b = nullptr;
    if (!ctx || !params || (n_pairs && (!seqs || !q_off || !q_len || !t_off || !t_len))) { g_err = "null argument"; st = ALN_ERR_INVALID_ARGUMENT; }
    else {
        b = new aln_batch();
        b->ctx = ctx->devs[0];
        hipError_t e = hipSetDevice(b->ctx->device);
        if (e != hipSuccess) st = fail(e, "hipSetDevice");
        if (st == ALN_OK) st = call_init(b->call, params, q_len, t_len, n_pairs, false);
        if (st == ALN_OK) st = chunk_plan(b->ctx, b->call, q_off, q_len, t_off, t_len, 0, n_pairs, true, b->k);
        if (st == ALN_OK) {
            b->slot = new Slot();
            b->slot->pooled = false;
            st = slot_ensure(*b->slot, b->call, b->k);
        }
        if (st == ALN_OK) st = slot_upload(*b->slot, b->call, b->k, seqs, q_off, q_len, t_off, t_len, b->slot->stream);
        if (st == ALN_OK) {
            e = hipMemsetAsync(b->slot->results.p, 0, std::max<size_t>(n_pairs * sizeof(aln_pair_result), 1), b->slot->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(b->slot->stream);
            if (e != hipSuccess) st = fail(e, "stage");
        }
        if (st != ALN_OK) { batch_free(b); b = nullptr; }
    }
    if (status) *status = st;
    return b;
}

extern "C" void aln_batch_enable_timing(aln_batch *b, int on)
{
    if (!b) return;
    b->timing = on != 0;
    b->ev_runs = 0;
    if (b->timing && b->ev.empty()) {
        (void)hipSetDevice(b->ctx->device);
        b->ev.resize(3 * ALN_TIMING_SLOTS, nullptr);
        for (auto &e : b->ev) (void)hipEventCreate(&e);
    }
}

extern "C" int aln_batch_run(aln_batch *b, void *stream)
{
    if (!b) return ALN_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(b->ctx->device));
    hipStream_t s = stream ? (hipStream_t)stream : b->slot->stream;
    b->last_stream = s;
    hipEvent_t *ev = b->timing ? &b->ev[3 * (b->ev_runs % ALN_TIMING_SLOTS)] : nullptr;
    int st = slot_launch(b->ctx, *b->slot, b->call, b->k, s, ev, &b->fill_launches);
    if (st == ALN_OK && ev) b->ev_runs++;
    return st;
}

static void coop_stats(aln_batch *b) { coop_stats_slot(*b->slot, b->k); }

extern "C" int aln_batch_sync(aln_batch *b)
{
    if (!b) return ALN_ERR_INVALID_ARGUMENT;
    HIPCHK(hipSetDevice(b->ctx->device));
    HIPCHK(hipStreamSynchronize(b->last_stream ? b->last_stream : b->slot->stream));
    coop_stats(b);
    return ALN_OK;
}

extern "C" int aln_batch_timing(aln_batch *b, double *fill_ms, double *tb_ms, uint32_t *fill_launches)
{
    if (!b || !b->timing || b->ev.empty() || b->ev_runs == 0) return ALN_ERR_INVALID_ARGUMENT;
    // mean over the runs recorded since aln_batch_enable_timing (at most the last ALN_TIMING_SLOTS)
    const uint32_t runs = std::min<uint32_t>(b->ev_runs, ALN_TIMING_SLOTS);
    double fs = 0, ts = 0;
    for (uint32_t r = 0; r < runs; ++r) {
        hipEvent_t *ev = &b->ev[3 * r];
        float f = 0, t = 0;
        HIPCHK(hipEventSynchronize(ev[2]));
        HIPCHK(hipEventElapsedTime(&f, ev[0], ev[1]));
        HIPCHK(hipEventElapsedTime(&t, ev[1], ev[2]));
        fs += f; ts += t;
    }
    coop_stats(b);
    if (fill_ms) *fill_ms = fs / runs;
    if (tb_ms) *tb_ms = ts / runs;
    if (fill_launches) *fill_launches = b->fill_launches;
    return ALN_OK;
}

extern "C" int aln_batch_fetch(aln_batch *b, aln_pair_result *results, uint8_t *tb_buf, const uint64_t *tb_off)
{
    if (!b || !results) return ALN_ERR_INVALID_ARGUMENT;
    int st = aln_batch_sync(b);
    if (st != ALN_OK) return st;
    return slot_download(*b->slot, b->call, b->k, b->slot->stream, results, tb_buf, tb_off);
}

extern "C" uint64_t aln_batch_cells(const aln_batch *b) { return b ? b->k.cells : 0; }
extern "C" size_t aln_batch_size(const aln_batch *b) { return b ? b->k.n : 0; }
extern "C" void *aln_batch_results_device(aln_batch *b) { return b ? b->slot->results.p : nullptr; }
extern "C" uint64_t aln_batch_direction_bytes(const aln_batch *b)
{
    if (!b) return 0;
    uint64_t total = 0;
    for (const PairDesc &d : b->k.descs) total += aln_pair_stored_dir_bytes(d);
    return total;
}

// ---------------------------------------------------------------- one pair, blocking
extern "C" int aln_align_pair(aln_ctx *ctx, const aln_params *params, const uint8_t *query, size_t N,
                              const uint8_t *target, size_t M, aln_pair_result *out, uint8_t *q_aln, uint8_t *t_aln,
                              uint8_t *directions, double *h_matrix)
{
    if (!ctx || !params || !out) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    const bool pwm = params->semantics == ALN_PWM_LOCAL;
    if (pwm) { N = params->cols; query = nullptr; }          // the columns are the PWM positions (pwm/mod.rs:44-46)
    const size_t nq = pwm ? 0 : N;
    aln_params p = *params;
    p.outputs = (params->outputs ? params->outputs : (ALN_OUT_SCORE | ALN_OUT_TRACEBACK));
    if (q_aln && t_aln) p.outputs |= ALN_OUT_TRACEBACK;
    if (directions) p.outputs |= ALN_OUT_DIRECTIONS;
    const uint64_t qo = 0, ql = N, to = nq, tl = M;
    Call c;
    int st = call_init(c, &p, &ql, &tl, 1, h_matrix != nullptr);
    if (st != ALN_OK) { memset(out, 0, sizeof *out); out->status = st; return st; }
    DevCtx *dev = ctx->next_device();                        // concurrent callers spread over the context's devices
    HIPCHK(hipSetDevice(dev->device));
    Slot *sl[1];
    pool_lease(dev, 1, sl);
    struct Release { DevCtx *c; Slot **s; ~Release() { pool_release(c, s, 1); } } rel{dev, sl};
    Slot &s = *sl[0];
    Chunk k;
    // (allow_overlap = true: a pair that misses the single-pair route -- more than ~77 000 columns -- opens its first pass for other waves
    // like a one-pair batch call does: 200 000 x 5000 ran on ONE wave at 1.8 GCUPS before, the reference's only limit being memory,
    // simple/mod.rs:53-57)
    if ((st = chunk_plan(dev, c, &qo, &ql, &to, &tl, 0, 1, true, k)) != ALN_OK) return st;
    k.seq_direct = false;                                    // query and target are two caller buffers: gathered into staging
    k.seq_span = nq + M;
    k.descs[0].q_off = 0; k.descs[0].t_off = nq;
    if ((st = slot_ensure(s, c, k)) != ALN_OK) return st;
    {   // the gather of slot_upload, from two pointers
        uint8_t *h = s.h_in.as<uint8_t>();
        if (nq) memcpy(h, query, nq);
        if (M) memcpy(h + nq, target, M);
    }
    if ((st = slot_upload(s, c, k, nullptr, &qo, &ql, &to, &tl, s.stream, true)) != ALN_OK) return st;
    if ((st = slot_launch(dev, s, c, k, s.stream, nullptr, nullptr)) != ALN_OK) { (void)hipStreamSynchronize(s.stream); return st; }
    const size_t cap = N + M + 2;
    const uint64_t cells = (uint64_t)(N + 1) * (M + 1);
    const bool ok_shape = k.descs[0].status == ALN_OK;
    if (directions && ok_shape) {
        if ((st = dev_ensure(s.unpack, cells, true)) != ALN_OK) return st;
        aln_launch_unpack(s.dirs.as<uint8_t>(), s.descs.as<PairDesc>(), 0, c.semantics, s.unpack.as<uint8_t>(), cells, s.stream);
    }
    // summary + strings: the strings of one pair are fetched through pinned staging and handed out as two buffers
    HIPCHK(hipMemcpyAsync(out, s.results.p, sizeof *out, hipMemcpyDeviceToHost, s.stream));
    const bool want_tb = q_aln && t_aln && c.want_tb && k.tb_bytes;
    if (want_tb) {
        if ((st = pin_ensure(s.h_out, k.tb_bytes)) != ALN_OK) return st;
        HIPCHK(hipMemcpyAsync(s.h_out.p, s.tb.p, k.tb_bytes, hipMemcpyDeviceToHost, s.stream));
    }
    HIPCHK(hipStreamSynchronize(s.stream));
    trace_tb_slot(s, c, k);
    if (out->status == ALN_OK && ok_shape) {
        if (want_tb) {
            const uint8_t *h = s.h_out.as<uint8_t>();
            if (pwm) {
                memcpy(q_aln, h, 4ull * out->aln_len);          // uint32 PWM column numbers
                memcpy(t_aln, h + 4 * cap, out->aln_len);
            } else {
                memcpy(q_aln, h, out->aln_len);
                memcpy(t_aln, h + cap, out->aln_len);
            }
        }
        if (directions) HIPCHK(hipMemcpy(directions, s.unpack.p, cells, hipMemcpyDeviceToHost));
        if (h_matrix) {
            if (c.is_int) {
                std::vector<int32_t> hi(cells);
                HIPCHK(hipMemcpy(hi.data(), s.hmat.p, cells * 4, hipMemcpyDeviceToHost));
                for (uint64_t i = 0; i < cells; ++i) h_matrix[i] = (double)hi[i];
            } else {
                HIPCHK(hipMemcpy(h_matrix, s.hmat.p, cells * 8, hipMemcpyDeviceToHost));
            }
        }
    }
    return out->status;
}

// ---------------------------------------------------------------- window scan: one chromosome resident in HBM
// The repeat search (latent-repeat-search, engine/calc.rs:19-147) aligns one PWM against every window j = first + k * step of a
// chromosome, rows seq[j .. min(j + width, len)), again and again.  A scan uploads the residues once; a pass is a geometry, not
// arrays: the descriptors are expanded on the device (aln_scan.hip) and handed to the same fill / traceback launches as a staged
// batch (slot_launch), planned by the same chunk_plan from the window lengths -- once per geometry and kind of call, then kept.
// A select pass tests z on the device, compacts the hits in window order and re-fills only those with directions, all on one
// stream; what comes back is the hit count, the hits' summaries and strings.
// A held pass (aln_scan_hits) is a select pass that keeps all of that on the device: the count alone comes back, the hit buffers
// are sized for it (no capacity, no second fill), and the caller then asks for the hit list (window, f), for the sum of the
// frequency matrices of a list of hits (aln_scan_freq_kernel: u32 counters, exact in any order) or for the strings of a list.

// the re-fill of a select pass has room for at least this many hits: a chunk of <= 4 pairs would take the one-workgroup route,
// whose plan reads the pairs' shapes on the host
#define ALN_SCAN_MIN_SLOTS 8u

struct ScanPlan {
    std::vector<uint64_t> key;
    Chunk k;
    uint64_t dir_stride = 0, tb_stride = 0, tag_stride = 0;
};

// Plans are shared by every scan of the process: the starting values' shuffled copy, the cycles and the reverse pass of a record
// (same length, same geometry) use one plan per kind of call.  Least recently used first.
static std::mutex g_scan_plans_mu;
static std::vector<std::shared_ptr<ScanPlan>> g_scan_plans;

// (ms of the last pass: fill, selection, hit re-fill + walk (kernel time), download (wall))
struct aln_scan : CallStats {
    DevCtx *ctx = nullptr;            // one device: the context's first (as a staged batch)
    Slot *slot = nullptr;             // private slot; slot->seqs holds the forward strand at 0 and, once needed, the reversed one at len
    uint64_t len = 0;
    bool rev_ready = false;
    DevBuf fbuf, tiles, idx, misc;    // f of every window; tile counts + offsets; hit indices; [0] hit count, [1] failed-status flag
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    // held hits (aln_scan_hits): hit h's window in idx[h], its summary in slot->results[h], its descriptor in slot->descs[h], its
    // strings in slot->tb at h * held_stride -- until the next pass on this scan
    bool held = false;
    uint64_t held_count = 0, held_stride = 0;
    uint32_t held_cols = 0, held_blank = 0;
    DevBuf held_f, keep, freq, packed;   // f of every hit; an uploaded list; u32 counters | f64 matrix; a list's summaries | strings
};

static uint64_t scan_windows(uint64_t len, const aln_scan_geometry *g)
{
    return g->first < len ? (len - 1 - g->first) / g->step + 1 : 0;
}

extern "C" size_t aln_scan_windows(const aln_scan *sc, const aln_scan_geometry *g)
{
    if (!sc || !g || g->step == 0) return 0;
    return (size_t)scan_windows(sc->len, g);
}

extern "C" void aln_scan_destroy(aln_scan *sc)
{
    if (!sc) return;
    (void)hipSetDevice(sc->ctx->device);
    for (hipEvent_t e : sc->ev) if (e) (void)hipEventDestroy(e);
    dev_free(sc->fbuf); dev_free(sc->tiles); dev_free(sc->idx); dev_free(sc->misc);
    dev_free(sc->held_f); dev_free(sc->keep); dev_free(sc->freq); dev_free(sc->packed);
    slot_destroy(sc->slot);
    delete sc;
}

extern "C" aln_scan *aln_scan_create(aln_ctx *ctx, const uint8_t *seq, size_t len, int *status)
{
    int st = ALN_OK;
    aln_scan *sc = nullptr;
    if (!ctx || (len && !seq)) { g_err = "null argument"; st = ALN_ERR_INVALID_ARGUMENT; }
    else if ((uint64_t)len > 0x7FFFFFF0ull) { g_err = "sequence too long"; st = ALN_ERR_UNSUPPORTED; }
    else {
        // residue codes: a PWM has 4 rows (pwm/mod.rs:40-42), so every code must be below 4 -- checked once here instead of per pass
        for (size_t i = 0; i < len; ++i)
            if (seq[i] >= 4) { g_err = "residue code outside the position-weight matrix"; st = ALN_ERR_CODE_OUT_OF_RANGE; break; }
    }
    if (st == ALN_OK) {
        sc = new aln_scan();
        sc->ctx = ctx->devs[0];
        sc->len = len;
        sc->slot = new Slot();
        sc->slot->pooled = false;
        hipError_t e = hipSetDevice(sc->ctx->device);
        if (e != hipSuccess) st = fail(e, "hipSetDevice");
        // both strands' room at once: the buffer never moves afterwards (slot_ensure asks for at most len + 64)
        if (st == ALN_OK) st = dev_ensure(sc->slot->seqs, 2 * (uint64_t)len + 256, false);
        if (st == ALN_OK) st = dev_ensure(sc->misc, 256, false);
        if (st == ALN_OK) st = slot_init(*sc->slot);
        for (int i = 0; i < 4 && st == ALN_OK; ++i) { e = hipEventCreate(&sc->ev[i]); if (e != hipSuccess) st = fail(e, "hipEventCreate"); }
        if (st == ALN_OK && len) {
            e = hipMemcpyAsync(sc->slot->seqs.p, seq, len, hipMemcpyHostToDevice, sc->slot->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(sc->slot->stream);
            if (e != hipSuccess) st = fail(e, "upload");
        }
        if (st != ALN_OK) { aln_scan_destroy(sc); sc = nullptr; }
    }
    if (status) *status = st;
    return sc;
}

// the plan of n windows of geometry g (hits == 0), or of a re-fill with `hits` slots of the geometry's widest window
// (the strand does not enter the plan: the descriptors' offsets are the device's business)
static int scan_plan(aln_scan *sc, const Call &c, const aln_scan_geometry *g, uint64_t n, uint64_t hits, std::shared_ptr<ScanPlan> &out)
{
    const uint64_t wmax = std::min<uint64_t>(g->width, sc->len);
    std::vector<uint64_t> key = {(uint64_t)sc->ctx->device, sc->len, n, g->first, g->step, g->width, hits, c.cols, (uint64_t)c.is_int,
                                 (uint64_t)c.fast, (uint64_t)c.store_dirs, (uint64_t)c.want_tb, (uint64_t)c.semantics,
                                 (uint64_t)(c.p.del != c.p.ext), (uint64_t)c.p.force_serial, (uint64_t)c.p.force_generic,
                                 (uint64_t)c.p.max_passes};
    {
        std::lock_guard<std::mutex> lk(g_scan_plans_mu);
        for (size_t i = 0; i < g_scan_plans.size(); ++i)
            if (g_scan_plans[i]->key == key) {
                out = g_scan_plans[i];
                g_scan_plans.erase(g_scan_plans.begin() + (ptrdiff_t)i);
                g_scan_plans.push_back(out);
                return ALN_OK;
            }
    }
    std::shared_ptr<ScanPlan> plp = std::make_shared<ScanPlan>();
    ScanPlan &pl = *plp;
    pl.key = key;
    const uint64_t m = hits ? hits : n;
    int st;
    {
        std::vector<uint64_t> q_off(m, 0), q_len(m, c.cols), t_off(m), t_len(m);
        for (uint64_t k = 0; k < m; ++k) {
            if (hits) { t_off[k] = 0; t_len[k] = wmax; continue; }
            const uint64_t j = g->first + k * g->step;
            t_off[k] = j;
            t_len[k] = std::min<uint64_t>(g->width, sc->len - j);
        }
        st = chunk_plan(sc->ctx, c, q_off.data(), q_len.data(), t_off.data(), t_len.data(), 0, m, true, pl.k);
    }
    if (st != ALN_OK) return st;
    if (hits) {
        // every slot gets the room of the largest window of the geometry (the last windows are shorter)
        uint64_t dmax = aln_dir_bytes(c.cols, (uint32_t)wmax);
        for (uint64_t k = n; k-- > 0;) {
            const uint64_t j = g->first + k * g->step;
            if (sc->len - j >= g->width) break;
            dmax = std::max<uint64_t>(dmax, aln_dir_bytes(c.cols, (uint32_t)(sc->len - j)));
        }
        const uint64_t cap = (uint64_t)c.cols + wmax + 2;
        pl.dir_stride = (dmax + 255) & ~255ull;
        pl.tb_stride = aln_tb_bytes(true, cap);
        pl.tag_stride = aln_tag_bytes(cap);
        pl.k.dir_bytes = hits * pl.dir_stride; pl.k.tb_bytes = hits * pl.tb_stride; pl.k.tag_bytes = hits * pl.tag_stride;
    }
    // The device writes the descriptors, and the queue as the window order.  Windows routed elsewhere (<= 4 windows, real-valued
    // PWM: the one-workgroup route takes the long ones) leave the batch kernel a queue of the others only: the plan's own queue is
    // uploaded over the identity then (scan_fill), and the host keeps the descriptors those launches read.
    if (pl.k.single_pairs.empty() && pl.k.wg_pairs.empty()) {
        pl.k.descs.clear(); pl.k.descs.shrink_to_fit();
        pl.k.order.clear(); pl.k.order.shrink_to_fit();
    }
    {
        std::lock_guard<std::mutex> lk(g_scan_plans_mu);
        if (g_scan_plans.size() >= 8) g_scan_plans.erase(g_scan_plans.begin());
        g_scan_plans.push_back(plp);
    }
    out = plp;
    return ALN_OK;
}

static int scan_call(aln_scan *sc, const aln_params *params, const aln_scan_geometry *g, uint32_t outputs, Call &c)
{
    if (!sc || !params || !g) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (params->semantics != ALN_PWM_LOCAL) { g_err = "a window scan aligns a position-weight matrix (ALN_PWM_LOCAL) only"; return ALN_ERR_UNSUPPORTED; }
    if (g->step == 0 || g->width == 0) { g_err = "geometry: step and width must be positive"; return ALN_ERR_INVALID_ARGUMENT; }
    if (scan_windows(sc->len, g) > 0xFFFFFFF0ull) { g_err = "too many windows"; return ALN_ERR_UNSUPPORTED; }
    aln_params p = *params;
    p.outputs = outputs;
    const uint64_t q1 = 0, t1 = std::min<uint64_t>(g->width, sc->len);      // the widest window decides the kernels (call_init)
    int st = call_init(c, &p, &q1, &t1, 1, false);
    if (st != ALN_OK) return st;
    HIPCHK(hipSetDevice(sc->ctx->device));
    Slot &s = *sc->slot;
    if (g->reverse && !sc->rev_ready && sc->len) {
        aln_scan_launch_reverse(s.seqs.as<uint8_t>(), sc->len, s.stream);
        HIPCHK(hipGetLastError());
        sc->rev_ready = true;
    }
    return ALN_OK;
}

// fill every window of g (score only) into the slot's results; f of every window into fbuf, a failed status into misc[1]
static int scan_fill(aln_scan *sc, const Call &c, const aln_scan_geometry *g, const ScanPlan *pl, uint64_t n)
{
    Slot &s = *sc->slot;
    hipStream_t st = s.stream;
    aln_scan_launch_expand(s.descs.as<PairDesc>(), s.order.as<uint32_t>(), n, g->first, g->step, g->width, sc->len, g->reverse ? sc->len : 0,
                           c.cols, st);
    HIPCHK(hipGetLastError());
    if (pl->k.n_small != n && pl->k.n_small)               // some windows take another route: the batch kernel's queue is the plan's
        HIPCHK(hipMemcpyAsync(s.order.p, pl->k.order.data(), 4 * pl->k.n_small, hipMemcpyHostToDevice, st));
    int e = slot_launch(sc->ctx, s, c, pl->k, st, nullptr, nullptr);
    if (e != ALN_OK) return e;
    HIPCHK(hipMemsetAsync(sc->misc.p, 0, 8, st));
    aln_scan_launch_f(s.results.as<aln_pair_result>(), sc->fbuf.as<double>(), n, sc->misc.as<int32_t>() + 1, st);
    HIPCHK(hipGetLastError());
    return ALN_OK;
}

static double ev_ms(hipEvent_t a, hipEvent_t b)
{
    float v = 0;
    return hipEventElapsedTime(&v, a, b) == hipSuccess ? (double)v : 0.0;
}

extern "C" int aln_scan_score(aln_scan *sc, const aln_params *params, const aln_scan_geometry *g, double *f)
{
    Call c;
    int st = scan_call(sc, params, g, ALN_OUT_SCORE, c);
    if (st != ALN_OK) return st;
    const uint64_t n = scan_windows(sc->len, g);
    if (n && !f) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    sc->held = false;
    stats_reset(*sc);
    if (n == 0) return ALN_OK;
    Slot &s = *sc->slot;
    std::shared_ptr<ScanPlan> pl;
    if ((st = scan_plan(sc, c, g, n, 0, pl)) != ALN_OK) return st;
    if ((st = slot_ensure(s, c, pl->k, nullptr, true)) != ALN_OK) return st;
    if ((st = dev_ensure(sc->fbuf, 8 * n, false)) != ALN_OK) return st;
    HIPCHK(hipEventRecord(sc->ev[0], s.stream));
    if ((st = upload_matrix(s, c, s.h_meta.as<uint8_t>(), s.stream)) != ALN_OK) return st;
    if ((st = scan_fill(sc, c, g, pl.get(), n)) != ALN_OK) { (void)hipStreamSynchronize(s.stream); return st; }
    HIPCHK(hipEventRecord(sc->ev[1], s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
    const auto t0 = std::chrono::steady_clock::now();
    int32_t misc[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(f, sc->fbuf.p, 8 * n, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipMemcpyAsync(misc, sc->misc.p, 8, hipMemcpyDeviceToHost, s.stream));
    HIPCHK(hipStreamSynchronize(s.stream));
    sc->ms[0] = ev_ms(sc->ev[0], sc->ev[1]);
    sc->ms[3] = wall_ms(t0);
    sc->bytes[0] = c.md.size() * (c.is_int ? 4 : 8) + (c.pwm && c.fast ? 4ull * c.cols : 0);
    sc->bytes[1] = 8 * n + 8;
    if (misc[1] != ALN_OK) { g_err = "a window failed"; return misc[1]; }
    return ALN_OK;
}

extern "C" int aln_scan_select(aln_scan *sc, const aln_params *params, const aln_scan_geometry *g, double mean, double sd, double z_min,
                               size_t cap, uint64_t *count, uint32_t *indices, aln_pair_result *results, uint8_t *tb_buf)
{
    Call c, ct;
    int st = scan_call(sc, params, g, ALN_OUT_SCORE, c);
    if (st != ALN_OK) return st;
    if (!count || (cap && (!indices || !results))) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (cap > 0xFFFFFFF0ull) { g_err = "capacity too large"; return ALN_ERR_UNSUPPORTED; }
    aln_params pt = *params;
    pt.outputs = ALN_OUT_SCORE | ALN_OUT_TRACEBACK;
    const uint64_t q1 = 0, t1 = std::min<uint64_t>(g->width, sc->len);
    if ((st = call_init(ct, &pt, &q1, &t1, 1, false)) != ALN_OK) return st;
    *count = 0;
    sc->held = false;
    stats_reset(*sc);
    const uint64_t n = scan_windows(sc->len, g);
    if (n == 0) return ALN_OK;
    Slot &s = *sc->slot;
    const uint64_t slots = std::max<uint64_t>(std::min<uint64_t>(cap, n), ALN_SCAN_MIN_SLOTS);
    std::shared_ptr<ScanPlan> pl, ph;
    if ((st = scan_plan(sc, c, g, n, 0, pl)) != ALN_OK) return st;
    if ((st = scan_plan(sc, ct, g, n, slots, ph)) != ALN_OK) return st;
    // every buffer is sized before anything is queued: a buffer that grew later would be freed under a running kernel
    if ((st = slot_ensure(s, c, pl->k, nullptr, true)) != ALN_OK) return st;
    if ((st = slot_ensure(s, ct, ph->k, nullptr, true)) != ALN_OK) return st;
    uint32_t *tile_count, *tile_off;
    if ((st = dev_ensure(sc->fbuf, 8 * n, false)) != ALN_OK) return st;
    if ((st = tiles_ensure(sc->tiles, aln_scan_tiles(n), &tile_count, &tile_off)) != ALN_OK) return st;
    if ((st = dev_ensure(sc->idx, 4 * slots, false)) != ALN_OK) return st;
    hipStream_t q = s.stream;
    HIPCHK(hipEventRecord(sc->ev[0], q));
    if ((st = upload_matrix(s, c, s.h_meta.as<uint8_t>(), q)) != ALN_OK) return st;
    if ((st = scan_fill(sc, c, g, pl.get(), n)) != ALN_OK) { (void)hipStreamSynchronize(q); return st; }
    HIPCHK(hipEventRecord(sc->ev[1], q));
    uint32_t *misc = sc->misc.as<uint32_t>();
    aln_scan_launch_select(s.results.as<aln_pair_result>(), n, mean, sd, z_min, tile_count, tile_off, misc, sc->idx.as<uint32_t>(), (uint32_t)slots, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(sc->ev[2], q));
    aln_scan_launch_hits(s.descs.as<PairDesc>(), s.order.as<uint32_t>(), (uint32_t)slots, sc->idx.as<uint32_t>(), misc, (uint32_t)slots,
                         g->first, g->step, g->width, sc->len, g->reverse ? sc->len : 0, c.cols, ph->dir_stride, ph->tb_stride, ph->tag_stride, q);
    HIPCHK(hipGetLastError());
    if ((st = slot_launch(sc->ctx, s, ct, ph->k, q, nullptr, nullptr)) != ALN_OK) { (void)hipStreamSynchronize(q); return st; }
    HIPCHK(hipEventRecord(sc->ev[3], q));
    HIPCHK(hipStreamSynchronize(q));
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t hm[2] = {0, 0};
    HIPCHK(hipMemcpy(hm, misc, 8, hipMemcpyDeviceToHost));
    *count = hm[0];
    const uint64_t got = std::min<uint64_t>(hm[0], cap);
    if (got) {
        HIPCHK(hipMemcpyAsync(indices, sc->idx.p, 4 * got, hipMemcpyDeviceToHost, q));
        HIPCHK(hipMemcpyAsync(results, s.results.p, sizeof(aln_pair_result) * got, hipMemcpyDeviceToHost, q));
        if (tb_buf) HIPCHK(hipMemcpyAsync(tb_buf, s.tb.p, ph->tb_stride * got, hipMemcpyDeviceToHost, q));
        HIPCHK(hipStreamSynchronize(q));
    }
    sc->ms[0] = ev_ms(sc->ev[0], sc->ev[1]);
    sc->ms[1] = ev_ms(sc->ev[1], sc->ev[2]);
    sc->ms[2] = ev_ms(sc->ev[2], sc->ev[3]);
    sc->ms[3] = wall_ms(t0);
    sc->bytes[0] = c.md.size() * (c.is_int ? 4 : 8) + (c.pwm && c.fast ? 4ull * c.cols : 0);
    sc->bytes[1] = 8 + got * (4 + sizeof(aln_pair_result) + (tb_buf ? ph->tb_stride : 0));
    if (hm[1] != ALN_OK) { g_err = "a window failed"; return (int)hm[1]; }
    if (hm[0] > cap) { g_err = "more windows passed than the capacity holds"; return ALN_ERR_CAPACITY; }
    return ALN_OK;
}

// ---- held pass: fill, z test and compaction as aln_scan_select; the count is read where the pass waits anyway, the hit buffers are
// sized for it, and every hit is re-filled with directions and walked.  Nothing but the count comes back.
extern "C" int aln_scan_hits(aln_scan *sc, const aln_params *params, const aln_scan_geometry *g, double mean, double sd, double z_min,
                             uint64_t *count)
{
    Call c, ct;
    int st = scan_call(sc, params, g, ALN_OUT_SCORE, c);
    if (st != ALN_OK) return st;
    if (!count) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    aln_params pt = *params;
    pt.outputs = ALN_OUT_SCORE | ALN_OUT_TRACEBACK;
    const uint64_t q1 = 0, t1 = std::min<uint64_t>(g->width, sc->len);
    if ((st = call_init(ct, &pt, &q1, &t1, 1, false)) != ALN_OK) return st;
    *count = 0;
    sc->held = false;
    stats_reset(*sc);
    sc->held_count = 0;
    sc->held_cols = c.cols;
    sc->held_blank = ct.p.blank_code;
    sc->held_stride = aln_scan_string_stride(sc, c.cols, g);
    const uint64_t n = scan_windows(sc->len, g);
    if (n == 0) { sc->held = true; return ALN_OK; }
    Slot &s = *sc->slot;
    std::shared_ptr<ScanPlan> pl, ph;
    if ((st = scan_plan(sc, c, g, n, 0, pl)) != ALN_OK) return st;
    if ((st = slot_ensure(s, c, pl->k, nullptr, true)) != ALN_OK) return st;
    uint32_t *tile_count, *tile_off;
    if ((st = dev_ensure(sc->fbuf, 8 * n, false)) != ALN_OK) return st;
    if ((st = tiles_ensure(sc->tiles, aln_scan_tiles(n), &tile_count, &tile_off)) != ALN_OK) return st;
    if ((st = dev_ensure(sc->idx, 4 * n, false)) != ALN_OK) return st;           // every window may pass: 4 bytes each
    hipStream_t q = s.stream;
    HIPCHK(hipEventRecord(sc->ev[0], q));
    if ((st = upload_matrix(s, c, s.h_meta.as<uint8_t>(), q)) != ALN_OK) return st;
    if ((st = scan_fill(sc, c, g, pl.get(), n)) != ALN_OK) { (void)hipStreamSynchronize(q); return st; }
    HIPCHK(hipEventRecord(sc->ev[1], q));
    uint32_t *misc = sc->misc.as<uint32_t>();
    aln_scan_launch_select(s.results.as<aln_pair_result>(), n, mean, sd, z_min, tile_count, tile_off, misc, sc->idx.as<uint32_t>(), (uint32_t)n, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(sc->ev[2], q));
    uint32_t hm[2] = {0, 0};
    HIPCHK(hipMemcpyAsync(hm, misc, 8, hipMemcpyDeviceToHost, q));
    HIPCHK(hipStreamSynchronize(q));
    sc->ms[0] = ev_ms(sc->ev[0], sc->ev[1]);
    sc->ms[1] = ev_ms(sc->ev[1], sc->ev[2]);
    sc->bytes[0] = c.md.size() * (c.is_int ? 4 : 8) + (c.pwm && c.fast ? 4ull * c.cols : 0);
    sc->bytes[1] = 8;
    if (hm[1] != ALN_OK) { g_err = "a window failed"; return (int)hm[1]; }
    const uint64_t hits = hm[0];
    if (hits) {
        // the stream is idle: the hit buffers may grow now.  The matrix is the fill's; it goes up again if its buffer moved.
        const uint64_t slots = std::max<uint64_t>(hits, ALN_SCAN_MIN_SLOTS);
        const void *m0 = s.matrix.p, *w0 = s.pwm_words.p;
        if ((st = scan_plan(sc, ct, g, n, slots, ph)) != ALN_OK) return st;
        st = slot_ensure(s, ct, ph->k, nullptr, true);
        if (st == ALN_OK) st = dev_ensure(sc->held_f, 8 * hits, false);
        if (st != ALN_OK) return st;                                 // ALN_ERR_OOM if the memory cannot be had; nothing is held
        if (s.matrix.p != m0 || s.pwm_words.p != w0)
            if ((st = upload_matrix(s, c, s.h_meta.as<uint8_t>(), q)) != ALN_OK) return st;
        HIPCHK(hipEventRecord(sc->ev[2], q));
        aln_scan_launch_hits(s.descs.as<PairDesc>(), s.order.as<uint32_t>(), (uint32_t)slots, sc->idx.as<uint32_t>(), misc, (uint32_t)slots,
                             g->first, g->step, g->width, sc->len, g->reverse ? sc->len : 0, c.cols, ph->dir_stride, ph->tb_stride,
                             ph->tag_stride, q);
        HIPCHK(hipGetLastError());
        if ((st = slot_launch(sc->ctx, s, ct, ph->k, q, nullptr, nullptr)) != ALN_OK) { (void)hipStreamSynchronize(q); return st; }
        aln_scan_launch_held_f(s.results.as<aln_pair_result>(), sc->held_f.as<double>(), (uint32_t)hits, q);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(sc->ev[3], q));
        HIPCHK(hipStreamSynchronize(q));
        sc->ms[2] = ev_ms(sc->ev[2], sc->ev[3]);
        sc->held_stride = ph->tb_stride;
    }
    sc->held_count = hits;
    sc->held = true;
    *count = hits;
    return ALN_OK;
}

static int held_check(aln_scan *sc, const void *keep, uint64_t n_keep)
{
    if (!sc) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (!sc->held) { g_err = "no held hits: aln_scan_hits has not run, or another pass has replaced them"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n_keep && !keep) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n_keep > 0x7FFFFFF0ull) { g_err = "list too long"; return ALN_ERR_INVALID_ARGUMENT; }
    const uint32_t *k = reinterpret_cast<const uint32_t *>(keep);
    for (uint64_t i = 0; i < n_keep; ++i)
        if (k[i] >= sc->held_count) { g_err = "a listed position is beyond the held hits"; return ALN_ERR_INVALID_ARGUMENT; }
    HIPCHK(hipSetDevice(sc->ctx->device));
    stats_reset(*sc);
    return ALN_OK;
}

static void held_done(aln_scan *sc, const std::chrono::steady_clock::time_point &t0, uint64_t up, uint64_t down)
{
    sc->ms[3] = wall_ms(t0);
    sc->bytes[0] = up; sc->bytes[1] = down;
}

extern "C" int aln_scan_held_list(aln_scan *sc, uint64_t first, uint64_t n, uint32_t *indices, double *f)
{
    int st = held_check(sc, nullptr, 0);
    if (st != ALN_OK) return st;
    if (first > sc->held_count || n > sc->held_count - first) { g_err = "range beyond the held hits"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n && (!indices || !f)) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    const auto t0 = std::chrono::steady_clock::now();
    if (n) {
        hipStream_t q = sc->slot->stream;
        HIPCHK(hipMemcpyAsync(indices, sc->idx.as<uint32_t>() + first, 4 * n, hipMemcpyDeviceToHost, q));
        HIPCHK(hipMemcpyAsync(f, sc->held_f.as<double>() + first, 8 * n, hipMemcpyDeviceToHost, q));
        HIPCHK(hipStreamSynchronize(q));
    }
    held_done(sc, t0, 0, 12 * n);
    return ALN_OK;
}

extern "C" int aln_scan_held_frequencies(aln_scan *sc, const uint32_t *keep, uint64_t n_keep, double *counts)
{
    int st = held_check(sc, keep, n_keep);
    if (st != ALN_OK) return st;
    if (!counts) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    const uint64_t cells = 4ull * sc->held_cols;
    if ((st = dev_ensure(sc->keep, 4 * n_keep, false)) != ALN_OK) return st;
    if ((st = dev_ensure(sc->freq, 16 * cells, false)) != ALN_OK) return st;     // u32 counters, then (8-byte aligned) the f64 matrix
    const auto t0 = std::chrono::steady_clock::now();
    Slot &s = *sc->slot;
    hipStream_t q = s.stream;
    double *out = reinterpret_cast<double *>(sc->freq.as<uint8_t>() + 8 * cells);
    HIPCHK(hipEventRecord(sc->ev[2], q));
    if (n_keep) HIPCHK(hipMemcpyAsync(sc->keep.p, keep, 4 * n_keep, hipMemcpyHostToDevice, q));
    aln_scan_launch_freq(s.descs.as<PairDesc>(), s.results.as<aln_pair_result>(), s.tb.as<uint8_t>(), sc->keep.as<uint32_t>(), (uint32_t)n_keep,
                         (uint32_t)sc->held_count, sc->held_cols, sc->held_blank, sc->freq.as<uint32_t>(), out, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(sc->ev[3], q));
    HIPCHK(hipMemcpyAsync(counts, out, 8 * cells, hipMemcpyDeviceToHost, q));
    HIPCHK(hipStreamSynchronize(q));
    sc->ms[2] = ev_ms(sc->ev[2], sc->ev[3]);
    held_done(sc, t0, 4 * n_keep, 8 * cells);
    return ALN_OK;
}

extern "C" int aln_scan_held_strings(aln_scan *sc, const uint32_t *keep, uint64_t n_keep, aln_pair_result *results, uint8_t *tb_buf)
{
    int st = held_check(sc, keep, n_keep);
    if (st != ALN_OK) return st;
    if (n_keep && (!results || !tb_buf)) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    const auto t0 = std::chrono::steady_clock::now();
    if (n_keep) {
        const uint64_t stride = sc->held_stride, res_bytes = (sizeof(aln_pair_result) * n_keep + 255) & ~255ull;
        if ((st = dev_ensure(sc->keep, 4 * n_keep, false)) != ALN_OK) return st;
        if ((st = dev_ensure(sc->packed, res_bytes + stride * n_keep, false)) != ALN_OK) return st;
        Slot &s = *sc->slot;
        hipStream_t q = s.stream;
        aln_pair_result *pres = sc->packed.as<aln_pair_result>();
        uint8_t *ptb = sc->packed.as<uint8_t>() + res_bytes;
        HIPCHK(hipEventRecord(sc->ev[2], q));
        HIPCHK(hipMemcpyAsync(sc->keep.p, keep, 4 * n_keep, hipMemcpyHostToDevice, q));
        aln_scan_launch_gather(s.results.as<aln_pair_result>(), s.tb.as<uint8_t>(), sc->keep.as<uint32_t>(), (uint32_t)n_keep,
                               (uint32_t)sc->held_count, stride, pres, ptb, q);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(sc->ev[3], q));
        HIPCHK(hipMemcpyAsync(results, pres, sizeof(aln_pair_result) * n_keep, hipMemcpyDeviceToHost, q));
        HIPCHK(hipMemcpyAsync(tb_buf, ptb, stride * n_keep, hipMemcpyDeviceToHost, q));
        HIPCHK(hipStreamSynchronize(q));
        sc->ms[2] = ev_ms(sc->ev[2], sc->ev[3]);
    }
    held_done(sc, t0, 4 * n_keep, n_keep * (sizeof(aln_pair_result) + sc->held_stride));
    return ALN_OK;
}

extern "C" uint64_t aln_scan_string_stride(const aln_scan *sc, uint32_t cols, const aln_scan_geometry *g)
{
    if (!sc || !g) return 0;
    const uint64_t cap = (uint64_t)cols + std::min<uint64_t>(g->width, sc->len) + 2;
    return (5 * cap + 3) & ~3ull;
}

extern "C" int aln_scan_stats(const aln_scan *sc, double *ms, uint64_t *bytes)
{
    return stats_get(sc, ms, bytes);
}

// ---------------------------------------------------------------- shuffled copies: calculate_p_value's batch on the device
// calculate_p_value (statistics/mod.rs:240-320) aligns a query against 4 999 trimmed and shuffled copies of its target.  A shuffle
// call uploads every pair's query and original target once; per chunk of whole pairs the copies are drawn on the device
// (aln_shuffle.hip: one thread per copy), expanded into descriptors there, filled score only by the same launches a batch call
// makes (slot_launch, planned by chunk_plan from the copies' lengths, which the host computes with aln_shuffle_rules.h), and
// their f gathered into one array: 8 bytes per copy and 4 per pair come back.  Every chunk is queued on one stream behind the
// one before it; the host waits once, at the end.

#define ALN_SHUFFLE_MAX_COPIES (1u << 20)          // per pair
#define ALN_SHUFFLE_CHUNK_COPIES (1ull << 22)      // per chunk: the pair limit of a chunk of aln_align_batch
#define ALN_SHUFFLE_CHUNK_BYTES (1ull << 30)       // shuffled residues per chunk

#include "aln_arena_rules.h"      // align256, and the arenas of the calls on a sequence set

// A body of queued work: a lambda whose HIPCHKs and checks return on the first thing that goes wrong.  Any way out of it but ALN_OK
// waits for the stream before the caller sees the status, so nothing queued still reads or writes the call's buffers by then.
template <class Body> static int run_queued(hipStream_t q, Body &&body)
{
    const int st = body();
    if (st != ALN_OK) (void)hipStreamSynchronize(q);
    return st;
}

static int shuffle_check(aln_ctx *ctx, const aln_shuffle_spec *sp, const uint8_t *seqs, const uint64_t *t_off, const uint64_t *t_len, size_t n)
{
    if (!ctx || !sp || (n && (!seqs || !t_off || !t_len))) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (sp->per_pair == 0 || sp->per_pair > ALN_SHUFFLE_MAX_COPIES) { g_err = "per_pair must be 1 .. 2^20"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n > 0xFFFFFFF0ull) { g_err = "too many pairs"; return ALN_ERR_UNSUPPORTED; }
    for (size_t i = 0; i < n; ++i) {
        if (t_len[i] > 0x7FFFFFF0ull) { g_err = "sequence too long"; return ALN_ERR_UNSUPPORTED; }
        // statistics/mod.rs:312-314 slices target[..len - lock]: a trim draw longer than the target panics there
        if (t_len[i] < sp->max_trim) { g_err = "a target is shorter than max_trim"; return ALN_ERR_INVALID_ARGUMENT; }
    }
    return ALN_OK;
}

// what a shuffle call uploads: one span of the caller's buffer, or -- offsets scattered far beyond what the pairs use -- the ranges
// packed back to back; and the pair table with every pair's offsets in those bytes and its copies' place in the shuffled region
struct ShuffleStage {
    std::vector<ShufflePair> pairs;
    bool direct = true;
    uint64_t lo = 0, bytes = 0;       // direct: seqs[lo .. lo + bytes)
    std::vector<uint8_t> packed;
};

static void shuffle_stage(const uint8_t *seqs, const uint64_t *q_off, const uint64_t *q_len, const uint64_t *t_off, const uint64_t *t_len,
                          size_t n, uint32_t per_pair, ShuffleStage &g)
{
    AlnSeqSpan span;
    for (size_t i = 0; i < n; ++i) { if (q_len) span.add(q_off[i], q_len[i]); span.add(t_off[i], t_len[i]); }
    const uint64_t lo = span.empty() ? 0 : span.lo, sum = span.sum;
    g.direct = span.direct();
    g.lo = lo;
    g.pairs.resize(n);
    if (!g.direct && seqs) g.packed.resize(sum);       // (no host residues: the caller copies the ranges on the device)
    uint64_t pos = 0, out = 0;
    for (size_t i = 0; i < n; ++i) {
        ShufflePair &P = g.pairs[i];
        P.q_len = q_len ? (uint32_t)q_len[i] : 0u;
        P.t_len = (uint32_t)t_len[i];
        if (g.direct) {
            P.q_off = P.q_len ? q_off[i] - lo : 0;
            P.t_off = P.t_len ? t_off[i] - lo : 0;
        } else {
            P.q_off = pos;
            if (P.q_len && seqs) memcpy(g.packed.data() + pos, seqs + q_off[i], P.q_len);
            pos += P.q_len;
            P.t_off = pos;
            if (P.t_len && seqs) memcpy(g.packed.data() + pos, seqs + t_off[i], P.t_len);
            pos += P.t_len;
        }
        P.out_off = out;
        out += (uint64_t)per_pair * P.t_len;
    }
    g.bytes = g.direct ? span.extent() : pos;
}

// chunks of whole pairs: at most ALN_SHUFFLE_CHUNK_COPIES copies and ALN_SHUFFLE_CHUNK_BYTES shuffled residues (a single pair may
// exceed the latter), and -- cells given -- cut once they reach `target` cells, as aln_make_chunks cuts
static void shuffle_chunks(const ShuffleStage &g, uint32_t per_pair, const std::vector<double> *cells, double target,
                           std::vector<std::pair<size_t, size_t>> &out)
{
    out.clear();
    const size_t n = g.pairs.size();
    size_t first = 0;
    double acc = 0;
    uint64_t copies = 0, bytes = 0;
    for (size_t i = 0; i < n; ++i) {
        const uint64_t b = (uint64_t)per_pair * g.pairs[i].t_len;
        if (i > first && (copies + per_pair > ALN_SHUFFLE_CHUNK_COPIES || bytes + b > ALN_SHUFFLE_CHUNK_BYTES)) {
            out.emplace_back(first, i - first);
            first = i; acc = 0; copies = 0; bytes = 0;
        }
        copies += per_pair; bytes += b;
        if (cells && (acc += (*cells)[i]) >= target) {
            out.emplace_back(first, i + 1 - first);
            first = i + 1; acc = 0; copies = 0; bytes = 0;
        }
    }
    if (first < n) out.emplace_back(first, n - first);
}

// LDS bytes per thread of the shuffle kernel for pairs [p0, p0 + np): the longest target that fits ALN_SHUFFLE_LDS_MAX, 16-aligned
static uint32_t shuffle_lds_slot(const ShuffleStage &g, size_t p0, size_t np)
{
    uint32_t m = 0;
    for (size_t i = p0; i < p0 + np; ++i)
        if (g.pairs[i].t_len <= ALN_SHUFFLE_LDS_MAX) m = std::max(m, g.pairs[i].t_len);
    return (m + 15u) & ~15u;
}

static uint64_t chunk_region_bytes(const ShuffleStage &g, uint32_t per_pair, size_t p0, size_t np)
{
    uint64_t b = 0;
    for (size_t i = p0; i < p0 + np; ++i) b += (uint64_t)per_pair * g.pairs[i].t_len;
    return b;
}

// H2D of the staged residues (at 0 of the slot's residue buffer) and of the pair table (at 0 of its shuffle buffer)
static int shuffle_upload(Slot &s, const ShuffleStage &g, const uint8_t *seqs, hipStream_t st)
{
    if (g.bytes) HIPCHK(hipMemcpyAsync(s.seqs.p, g.direct ? seqs + g.lo : g.packed.data(), g.bytes, hipMemcpyHostToDevice, st));
    if (!g.pairs.empty()) HIPCHK(hipMemcpyAsync(s.shuffle.p, g.pairs.data(), g.pairs.size() * sizeof(ShufflePair), hipMemcpyHostToDevice, st));
    return ALN_OK;
}

// ---- what a call that scores shuffled copies plans before anything is queued (aln_shuffle_scores, aln_seqset_held_significance):
// the copies' lengths, the call's analysis, the staged pair table, the chunks of whole pairs and every chunk's plan
struct ShuffleJob {
    Call c;
    ShuffleStage g;
    std::vector<std::pair<size_t, size_t>> ranges;
    std::vector<Chunk> plans;
    uint64_t region = 0;              // the shuffled copies of a chunk lie behind the staged residues
    uint64_t region_max = 0, seq_need = 0, copies_max = 0;
};

// stream (optional): pair i's stream index is stream[i], not spec->pair_base + i.  seqs: the caller's residues, or null when they
// are resident on the device at the same offsets (the caller then copies them there: ShuffleStage says where).  lens (optional):
// n * per_pair entries, written; without it the lengths are drawn again where a chunk is planned (a trim is one SplitMix64 draw),
// so nothing on the host grows with n * per_pair beyond one chunk's tables.  n == 0: only the checks of call_init.
static int shuffle_job_plan(const DevCtx *dev, const aln_params *params, const aln_shuffle_spec *spec, const uint64_t *stream,
                            const uint8_t *seqs, const uint64_t *q_off, const uint64_t *q_len, const uint64_t *t_off, const uint64_t *t_len,
                            size_t n_pairs, uint32_t *lens, ShuffleJob &job)
{
    const uint32_t per = spec->per_pair;
    // every copy's length: the plan needs them, the caller gets them; the longest copy of each pair decides the routes as in
    // aln_align_batch over the copies (call_init)
    std::vector<uint64_t> lmax(n_pairs, 0);
    std::vector<double> cells(n_pairs, 0.0);
    for (size_t i = 0; i < n_pairs; ++i) {
        uint64_t sum = 0;
        const uint64_t id = stream ? stream[i] : spec->pair_base + i;
        for (uint32_t s = 0; s < per; ++s) {
            const uint32_t L = (uint32_t)t_len[i] - aln_shuffle_trim_of(spec->seed, id, s, spec->max_trim);
            if (lens) lens[(uint64_t)i * per + s] = L;
            lmax[i] = std::max<uint64_t>(lmax[i], L);
            sum += L;
        }
        cells[i] = (double)q_len[i] * (double)sum;
    }
    aln_params p = *params;
    p.outputs = ALN_OUT_SCORE;
    Call &c = job.c;
    int st;
    if ((st = call_init(c, &p, q_len, lmax.data(), n_pairs, false)) != ALN_OK) return st;
    if (n_pairs == 0) return ALN_OK;

    ShuffleStage &g = job.g;
    shuffle_stage(seqs, q_off, q_len, t_off, t_len, n_pairs, per, g);
    shuffle_chunks(g, per, &cells, aln_chunk_cells_override(plan_knobs(), aln_shuffle_chunk_target(c.fast)), job.ranges);
    job.region = align256(g.bytes);
    // the plans of every chunk first: the copies' lengths and offsets in the residue buffer, routed and laid out by chunk_plan
    job.plans.resize(job.ranges.size());
    std::vector<uint64_t> qo, ql, to, tl;
    for (size_t j = 0; j < job.ranges.size(); ++j) {
        const size_t p0 = job.ranges[j].first, np = job.ranges[j].second;
        const uint64_t m = (uint64_t)np * per, out_base = g.pairs[p0].out_off;
        qo.resize(m); ql.resize(m); to.resize(m); tl.resize(m);
        for (size_t i = p0; i < p0 + np; ++i) {
            const ShufflePair &P = g.pairs[i];
            const uint64_t id = stream ? stream[i] : spec->pair_base + i;
            for (uint32_t s = 0; s < per; ++s) {
                const uint64_t k = (uint64_t)(i - p0) * per + s;
                qo[k] = P.q_off; ql[k] = P.q_len;
                to[k] = job.region + (P.out_off - out_base) + (uint64_t)s * P.t_len;
                tl[k] = lens ? lens[(uint64_t)i * per + s] : P.t_len - aln_shuffle_trim_of(spec->seed, id, s, spec->max_trim);
            }
        }
        Chunk &k = job.plans[j];
        if ((st = chunk_plan(dev, c, qo.data(), ql.data(), to.data(), tl.data(), 0, m, true, k)) != ALN_OK) return st;
        // the descriptors are the device's (aln_shuffle_expand_kernel); the host keeps them, and the queue, only for the launches of
        // copies routed elsewhere (scan_plan does the same)
        if (k.single_pairs.empty() && k.wg_pairs.empty()) {
            k.descs.clear(); k.descs.shrink_to_fit();
            k.order.clear(); k.order.shrink_to_fit();
        }
        job.region_max = std::max(job.region_max, chunk_region_bytes(g, per, p0, np));
        job.seq_need = std::max(job.seq_need, k.seq_span);
        job.copies_max = std::max(job.copies_max, m);
    }
    if (trace_plan()) fprintf(stderr, "aln shuffle: pairs %zu copies %u chunks %zu\n", n_pairs, per, job.ranges.size());
    return ALN_OK;
}

// the slot's buffers for every chunk of the job, sized before anything is queued (a buffer that grew later would be freed under a
// running kernel); the shuffle buffer is the caller's to size
static int shuffle_job_ensure(Slot &s, const ShuffleJob &job)
{
    int st;
    if ((st = dev_ensure(s.seqs, std::max(job.region + job.region_max, job.seq_need) + 64, s.pooled)) != ALN_OK) return st;
    for (const Chunk &k : job.plans)
        if ((st = slot_ensure(s, job.c, k, nullptr, true)) != ALN_OK) return st;
    return ALN_OK;
}

// chunk j on the slot's stream: its copies drawn, expanded into descriptors and filled; their summaries are in s.results afterwards
// (stream order).  pairs_d / stream_d: the pair table and the optional stream table on the device.
static int shuffle_job_chunk(DevCtx *dev, Slot &s, const ShuffleJob &job, size_t j, const aln_shuffle_spec *spec, const ShufflePair *pairs_d,
                             const uint64_t *stream_d, uint64_t *up)
{
    hipStream_t q = s.stream;
    const size_t p0 = job.ranges[j].first, np = job.ranges[j].second;
    const uint32_t per = spec->per_pair;
    const uint64_t m = (uint64_t)np * per, out_base = job.g.pairs[p0].out_off, region = job.region;
    const Chunk &k = job.plans[j];
    const uint32_t lds = shuffle_lds_slot(job.g, p0, np);
    if (stream_d) {
        aln_shuffle_launch_table(s.seqs.as<uint8_t>(), s.seqs.as<uint8_t>() + region, pairs_d, (uint32_t)p0, m, per, spec->seed, stream_d,
                                 spec->max_trim, out_base, lds, q);
        aln_shuffle_launch_expand_table(s.descs.as<PairDesc>(), s.order.as<uint32_t>(), pairs_d, (uint32_t)p0, m, per, spec->seed, stream_d,
                                        spec->max_trim, region, out_base, q);
    } else {
        aln_shuffle_launch(s.seqs.as<uint8_t>(), s.seqs.as<uint8_t>() + region, pairs_d, (uint32_t)p0, m, per, spec->seed, spec->pair_base,
                           spec->max_trim, out_base, lds, q);
        aln_shuffle_launch_expand(s.descs.as<PairDesc>(), s.order.as<uint32_t>(), pairs_d, (uint32_t)p0, m, per, spec->seed, spec->pair_base,
                                  spec->max_trim, region, out_base, q);
    }
    HIPCHK(hipGetLastError());
    if (k.n_small != k.n && k.n_small) {             // some copies take another route: the batch kernel's queue is the plan's
        HIPCHK(hipMemcpyAsync(s.order.p, k.order.data(), 4 * k.n_small, hipMemcpyHostToDevice, q));
        if (up) *up += 4 * k.n_small;
    }
    int st;
    if ((st = slot_launch(dev, s, job.c, k, q, nullptr, nullptr)) != ALN_OK) { (void)hipStreamSynchronize(q); return st; }
    return ALN_OK;
}

extern "C" int aln_shuffle_scores(aln_ctx *ctx, const aln_params *params, const aln_shuffle_spec *spec, const uint8_t *seqs,
                                  const uint64_t *q_off, const uint64_t *q_len, const uint64_t *t_off, const uint64_t *t_len,
                                  size_t n_pairs, double *f, uint32_t *lengths, int32_t *status)
{
    int st = shuffle_check(ctx, spec, seqs, t_off, t_len, n_pairs);
    if (st != ALN_OK) return st;
    if (!params || (n_pairs && (!q_off || !q_len || !f))) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (params->semantics == ALN_PWM_LOCAL) { g_err = "shuffled copies are aligned with the substitution-matrix semantics only"; return ALN_ERR_UNSUPPORTED; }
    const uint32_t per = spec->per_pair;
    const uint64_t total = (uint64_t)n_pairs * per;
    std::vector<uint32_t> own_lens;
    uint32_t *lens = lengths;
    if (!lens) { own_lens.resize(total); lens = own_lens.data(); }
    DevCtx *dev = ctx->devs[0];
    ShuffleJob job;
    if ((st = shuffle_job_plan(dev, params, spec, nullptr, seqs, q_off, q_len, t_off, t_len, n_pairs, lens, job)) != ALN_OK) return st;
    if (n_pairs == 0) return ALN_OK;
    const Call &c = job.c;
    const ShuffleStage &g = job.g;
    HIPCHK(hipSetDevice(dev->device));
    Slot *sl[1];
    pool_lease(dev, 1, sl);
    struct Release { DevCtx *c; Slot **s; ~Release() { pool_release(c, s, 1); } } rel{dev, sl};
    Slot &s = *sl[0];
    if ((st = shuffle_job_ensure(s, job)) != ALN_OK) return st;
    const uint64_t f_off = align256(sizeof(ShufflePair) * n_pairs), first_off = align256(f_off + 8 * total);
    if ((st = dev_ensure(s.shuffle, first_off + 4ull * n_pairs, s.pooled)) != ALN_OK) return st;
    const ShufflePair *pairs_d = s.shuffle.as<ShufflePair>();
    double *f_d = reinterpret_cast<double *>(s.shuffle.as<uint8_t>() + f_off);
    uint32_t *first_d = reinterpret_cast<uint32_t *>(s.shuffle.as<uint8_t>() + first_off);
    hipStream_t q = s.stream;
    if ((st = shuffle_upload(s, g, seqs, q)) != ALN_OK) return st;
    HIPCHK(hipMemsetAsync(first_d, 0xff, 4ull * n_pairs, q));
    if ((st = upload_matrix(s, c, s.h_meta.as<uint8_t>(), q)) != ALN_OK) return st;
    for (size_t j = 0; j < job.ranges.size(); ++j) {
        const size_t p0 = job.ranges[j].first, np = job.ranges[j].second;
        if ((st = shuffle_job_chunk(dev, s, job, j, spec, pairs_d, nullptr, nullptr)) != ALN_OK) return st;
        aln_shuffle_launch_gather(s.results.as<aln_pair_result>(), f_d + (uint64_t)p0 * per, (uint64_t)np * per, per, first_d + p0, q);
        HIPCHK(hipGetLastError());
    }
    std::vector<uint32_t> first(n_pairs);
    HIPCHK(hipMemcpyAsync(f, f_d, 8 * total, hipMemcpyDeviceToHost, q));
    HIPCHK(hipMemcpyAsync(first.data(), first_d, 4ull * n_pairs, hipMemcpyDeviceToHost, q));
    HIPCHK(hipStreamSynchronize(q));
    int bad = ALN_OK;
    for (size_t i = 0; i < n_pairs; ++i) {
        const int32_t v = first[i] == 0xffffffffu ? ALN_OK : (int32_t)(first[i] & 0xffu);
        if (status) status[i] = v;
        if (bad == ALN_OK && v != ALN_OK) bad = v;
    }
    if (!status && bad != ALN_OK) { g_err = "a pair failed"; return bad; }
    return ALN_OK;
}

extern "C" int aln_shuffle_targets(aln_ctx *ctx, const aln_shuffle_spec *spec, const uint8_t *seqs, const uint64_t *t_off,
                                   const uint64_t *t_len, size_t n_pairs, uint8_t *out, const uint64_t *out_off)
{
    int st = shuffle_check(ctx, spec, seqs, t_off, t_len, n_pairs);
    if (st != ALN_OK) return st;
    if (n_pairs && (!out || !out_off)) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n_pairs == 0) return ALN_OK;
    const uint32_t per = spec->per_pair;
    ShuffleStage g;
    shuffle_stage(seqs, nullptr, nullptr, t_off, t_len, n_pairs, per, g);
    std::vector<std::pair<size_t, size_t>> ranges;
    shuffle_chunks(g, per, nullptr, 0.0, ranges);
    uint64_t region_max = 0;
    for (const auto &r : ranges) region_max = std::max(region_max, chunk_region_bytes(g, per, r.first, r.second));
    const uint64_t region = align256(g.bytes);
    DevCtx *dev = ctx->devs[0];
    HIPCHK(hipSetDevice(dev->device));
    Slot *sl[1];
    pool_lease(dev, 1, sl);
    struct Release { DevCtx *c; Slot **s; ~Release() { pool_release(c, s, 1); } } rel{dev, sl};
    Slot &s = *sl[0];
    if ((st = dev_ensure(s.seqs, region + region_max + 64, s.pooled)) != ALN_OK) return st;
    if ((st = dev_ensure(s.shuffle, sizeof(ShufflePair) * n_pairs, s.pooled)) != ALN_OK) return st;
    if ((st = slot_init(s)) != ALN_OK) return st;
    hipStream_t q = s.stream;
    if ((st = shuffle_upload(s, g, seqs, q)) != ALN_OK) return st;
    uint8_t *region_d = s.seqs.as<uint8_t>() + region;
    for (const auto &r : ranges) {
        const size_t p0 = r.first, np = r.second;
        const uint64_t out_base = g.pairs[p0].out_off, bytes = chunk_region_bytes(g, per, p0, np);
        HIPCHK(hipMemsetAsync(region_d, 0, bytes, q));     // the bytes of a slot beyond its copy's length read 0
        aln_shuffle_launch(s.seqs.as<uint8_t>(), region_d, s.shuffle.as<ShufflePair>(), (uint32_t)p0, (uint64_t)np * per, per, spec->seed,
                           spec->pair_base, spec->max_trim, out_base, shuffle_lds_slot(g, p0, np), q);
        HIPCHK(hipGetLastError());
        // the caller's layout: one copy when its offsets are this chunk's, one per pair otherwise
        bool span = true;
        for (size_t i = p0; i < p0 + np && span; ++i) span = out_off[i] >= out_off[p0] && out_off[i] - out_off[p0] == g.pairs[i].out_off - out_base;
        if (span) {
            if (bytes) HIPCHK(hipMemcpyAsync(out + out_off[p0], region_d, bytes, hipMemcpyDeviceToHost, q));
        } else {
            for (size_t i = p0; i < p0 + np; ++i)
                if (g.pairs[i].t_len)
                    HIPCHK(hipMemcpyAsync(out + out_off[i], region_d + (g.pairs[i].out_off - out_base), (uint64_t)per * g.pairs[i].t_len,
                                          hipMemcpyDeviceToHost, q));
        }
    }
    HIPCHK(hipStreamSynchronize(q));
    return ALN_OK;
}

// ---------------------------------------------------------------- the held store of a pair set and of a sequence set
// What a pair set's last run and a sequence set's held pass leave on the device: entry k's summary in res[k] and its strings in tb at
// info_h[k].tb_off (HeldEntry).  The triple (info, res, tb) is what aln_pairset_launch_freq, the transform, aln_report_launch and the
// loop's step read.  (A scan's held hits are PairDesc entries at a uniform stride in its slot: aln_scan_held_*.)
struct HeldStore {
    size_t n = 0;                     // entries
    std::vector<HeldEntry> info_h;    // host copy of the table
    DevBuf res, tb, info;
    DevBuf list, out_off, packed_res, packed_tb;      // a fetch: the listed entries, their packed offsets, what goes down
};

static void held_free(HeldStore &h)
{
    DevBuf *d[] = {&h.res, &h.tb, &h.info, &h.list, &h.out_off, &h.packed_res, &h.packed_tb};
    for (DevBuf *b : d) dev_free(*b);
}
static void held_clear(HeldStore &h) { h.n = 0; h.info_h.clear(); }
// what every reader of a store takes: the triple on the device
struct HeldView { const HeldEntry *info; const aln_pair_result *res; const uint8_t *tb; };
static HeldView held_view(const HeldStore &h) { return HeldView{h.info.as<HeldEntry>(), h.res.as<aln_pair_result>(), h.tb.as<uint8_t>()}; }

// kernel times and uploaded bytes of a re-fill, added to: each family reports them its own way (a pair set fill and traceback, a
// sequence set both as one interval, fill start to traceback end: not their sum, which counts the event between them twice)
struct RefillStats { double fill_ms = 0, tb_ms = 0, both_ms = 0; uint64_t bytes_up = 0; };

// The listed pairs as a batch of their own over resident residues (pair k's at qo[k] / to[k] of s.seqs, whose seq_span bytes are
// there already and must not grow): the fill with directions and the traceback, chunk after chunk on the one slot, summaries and
// strings kept in `h`.  The stream is idle on entry and on every way out; on a failure nothing is held.
static int held_refill(HeldStore &h, DevCtx *ctx, Slot &s, const Call &c, const std::vector<uint64_t> &qo, const std::vector<uint64_t> &ql,
                       const std::vector<uint64_t> &to, const std::vector<uint64_t> &tl, uint64_t seq_span, hipEvent_t *ev, RefillStats &acc)
{
    hipStream_t q = s.stream;
    const size_t pairs = ql.size();
    h.n = 0;
    h.info_h.assign(pairs, HeldEntry{});
    uint64_t tb_total = 0;
    for (size_t k = 0; k < pairs; ++k) {
        h.info_h[k].N = (uint32_t)ql[k]; h.info_h[k].M = (uint32_t)tl[k]; h.info_h[k].tb_off = tb_total;
        tb_total += 2ull * (ql[k] + tl[k] + 2);      // the chunks' own layout (chunk_plan), chunk after chunk
    }
    std::vector<std::pair<size_t, size_t>> ranges;
    aln_make_chunks(plan_call(c), plan_knobs(), ql.data(), tl.data(), pairs, 1, ranges);
    Chunk k;
    bool timed = false;
    auto collect = [&]() {
        if (timed) { acc.fill_ms += ev_ms(ev[0], ev[1]); acc.tb_ms += ev_ms(ev[1], ev[2]); acc.both_ms += ev_ms(ev[0], ev[2]); timed = false; }
    };
    int st = ALN_OK;
    st = run_queued(q, [&]() -> int {
        // the store, sized for exactly this count; nothing is held if the memory cannot be had
        if ((st = dev_ensure(h.res, sizeof(aln_pair_result) * pairs, false)) != ALN_OK) return st;
        if ((st = dev_ensure(h.tb, tb_total, false)) != ALN_OK) return st;
        if ((st = dev_ensure(h.info, sizeof(HeldEntry) * pairs, false)) != ALN_OK) return st;
        HIPCHK(hipMemcpyAsync(h.info.p, h.info_h.data(), sizeof(HeldEntry) * pairs, hipMemcpyHostToDevice, q));
        acc.bytes_up += sizeof(HeldEntry) * pairs;
        // the plan of chunk j + 1 is made while chunk j runs; its tables go through the slot's pinned staging, so they wait for chunk j
        for (size_t j = 0; j < ranges.size(); ++j) {
            const size_t first = ranges[j].first, n = ranges[j].second;
            k.reset();
            if ((st = chunk_plan(ctx, c, qo.data(), ql.data(), to.data(), tl.data(), first, n, ranges.size() == 1, k, ranges.size() > 4)) != ALN_OK) return st;
            chunk_resident(k, qo.data() + first, to.data() + first, n, seq_span);
            HIPCHK(hipStreamSynchronize(q));
            collect();
            if ((st = slot_ensure(s, c, k)) != ALN_OK) return st;
            if ((st = slot_upload(s, c, k, nullptr, qo.data(), ql.data(), to.data(), tl.data(), q, false, true)) != ALN_OK) return st;
            // (4 bytes per pair for the queue, as reported since the first resident run: the queue uploaded leaves out the pairs that
            // are routed off the batch kernel, so fewer bytes may move)
            acc.bytes_up += n * (sizeof(PairDesc) + 4);
            if ((st = slot_launch(ctx, s, c, k, q, ev, nullptr)) != ALN_OK) return st;
            timed = true;
            HIPCHK(hipMemcpyAsync(h.res.as<aln_pair_result>() + first, s.results.p, n * sizeof(aln_pair_result), hipMemcpyDeviceToDevice, q));
            if (k.tb_bytes) HIPCHK(hipMemcpyAsync(h.tb.as<uint8_t>() + h.info_h[first].tb_off, s.tb.p, k.tb_bytes, hipMemcpyDeviceToDevice, q));
        }
        HIPCHK(hipStreamSynchronize(q));
        return ALN_OK;
    });
    if (st != ALN_OK) return st;
    collect();
    h.n = pairs;
    return ALN_OK;
}

// Summaries and both strings of the listed entries: packed on the device (aln_held_gather_kernel) for one download in the documented
// cumulative layout, from which the caller's own offsets are served.  An entry's whole capacity goes to the caller in either layout:
// zeros beyond aln_len, and zeros for a failed entry.  stats: ms[2], ms[3] and bytes of the fetch.
static int held_fetch_strings(HeldStore &h, hipStream_t q, hipEvent_t *ev, const uint32_t *entries, size_t n, aln_pair_result *results,
                              uint8_t *tb_buf, const uint64_t *tb_off, CallStats &stats)
{
    std::vector<uint64_t> off(n);
    uint64_t total = 0;
    for (size_t k = 0; k < n; ++k) { off[k] = total; total += 2ull * ((uint64_t)h.info_h[entries[k]].N + h.info_h[entries[k]].M + 2); }
    const bool want = tb_buf != nullptr;
    bool direct = want;
    for (size_t k = 0; k < n && direct; ++k) direct = tb_off[k] >= tb_off[0] && tb_off[k] - tb_off[0] == off[k];
    int st;
    if ((st = dev_ensure(h.list, 4ull * n, false)) != ALN_OK) return st;
    if ((st = dev_ensure(h.out_off, 8ull * n, false)) != ALN_OK) return st;
    if ((st = dev_ensure(h.packed_res, sizeof(aln_pair_result) * n, false)) != ALN_OK) return st;
    if (want && (st = dev_ensure(h.packed_tb, total, false)) != ALN_OK) return st;
    const auto t0 = std::chrono::steady_clock::now();
    // (the summaries land in a buffer of the call's own first: an error on the way leaves the caller's array as it was)
    std::vector<aln_pair_result> res(n);
    std::vector<uint8_t> bounce;
    st = run_queued(q, [&]() -> int {
        HIPCHK(hipMemcpyAsync(h.list.p, entries, 4ull * n, hipMemcpyHostToDevice, q));
        HIPCHK(hipMemcpyAsync(h.out_off.p, off.data(), 8ull * n, hipMemcpyHostToDevice, q));
        HIPCHK(hipEventRecord(ev[0], q));
        // (the kernel writes aln_len bytes per string: whatever else the packed span holds goes to the caller as zeros, not as what
        // an earlier fetch left there)
        if (want) HIPCHK(hipMemsetAsync(h.packed_tb.p, 0, total, q));
        const HeldView v = held_view(h);
        aln_held_launch_gather(v.info, v.res, v.tb, h.list.as<uint32_t>(), h.out_off.as<uint64_t>(), (uint32_t)n, (uint32_t)h.n,
                               h.packed_res.as<aln_pair_result>(), want ? h.packed_tb.as<uint8_t>() : nullptr, q);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ev[1], q));
        HIPCHK(hipMemcpyAsync(res.data(), h.packed_res.p, sizeof(aln_pair_result) * n, hipMemcpyDeviceToHost, q));
        if (want) {
            if (direct) HIPCHK(hipMemcpyAsync(tb_buf + tb_off[0], h.packed_tb.p, total, hipMemcpyDeviceToHost, q));
            else { bounce.resize(total); HIPCHK(hipMemcpyAsync(bounce.data(), h.packed_tb.p, total, hipMemcpyDeviceToHost, q)); }
        }
        HIPCHK(hipStreamSynchronize(q));
        return ALN_OK;
    });
    if (st != ALN_OK) return st;
    memcpy(results, res.data(), sizeof(aln_pair_result) * n);
    if (want && !direct)                             // an entry's whole capacity, as the direct copy
        for (size_t k = 0; k < n; ++k) {
            const uint64_t cap = (uint64_t)h.info_h[entries[k]].N + h.info_h[entries[k]].M + 2;
            memcpy(tb_buf + tb_off[k], bounce.data() + off[k], 2 * cap);
        }
    stats.ms[2] = ev_ms(ev[0], ev[1]);
    stats.ms[3] = wall_ms(t0);
    stats.bytes[0] = 12ull * n; stats.bytes[1] = sizeof(aln_pair_result) * n + (want ? total : 0);
    return ALN_OK;
}

// ---------------------------------------------------------------- resident pair set (aln_pairset_*, include/aligner_hip.h)
// The loop of HeuristicAligner (heuristic/mod.rs:36-78) for many pairs in lock step: the residues stay in HBM, every run aligns the
// listed pairs under a matrix of their own (aln_fill_f64_kernel<SEM, true>: the lean f64 strip, the matrix staged per wave), and the
// walked strings stay on the device, where the frequency matrices the next iteration needs are counted.

struct aln_seqset;
static void seqset_derived_gone(aln_seqset *ss);

// (ms: last run: fill kernels, traceback kernels; last fetch: its kernels; last call: wall time of its copies)
struct aln_pairset : CallStats {
    DevCtx *ctx = nullptr;            // one device: the context's first (as a staged batch)
    Slot *slot = nullptr;             // private slot; slot->seqs holds every pair's residues, packed in pair order
    // a pair set over a block of a sequence set (aln_pairset_create_from_set): slot->seqs is the set's residue buffer, borrowed -- never
    // grown and never freed here
    aln_seqset *owner = nullptr;
    uint64_t residues = 0;            // bytes of residues in slot->seqs
    size_t n = 0;
    std::vector<uint64_t> q_off, q_len, t_off, t_len;      // offsets into slot->seqs
    // held state of the last run: entry k = pair active[k]
    bool held = false;
    HeldStore held_store;
    uint32_t rows = 0, cols = 0, blank = 0;
    std::vector<int64_t> entry_of;    // pair -> held entry, -1: not in the last run
    DevBuf matrices, counts;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // 0 .. 2: a run's launches; 4, 5: transform / pick kernels
    // the heuristic loop's resident state (aln_pairset_heuristics): every pair's parameters and one matrix per pair
    bool heur = false;
    uint32_t h_rows = 0, h_cols = 0;
    DevBuf h_freq, h_kd, h_r2, store, shared, h_list, h_entry, h_status, picked;
    std::vector<char> written;        // pair -> its store entry holds a matrix
    // the loop's own state (aln_pairset_loop_begin / loop_step): best f per pair and the going list on the device -- going[cur] is the
    // list, going[cur ^ 1] where the next one is compacted -- and the host's copy of the list, from which the chunks are planned
    bool loop = false;
    int cur = 0;
    DevBuf best, going[2], cls, l_tiles, l_count, cand_pair, cand_entry, fin_pair, fin_cause, fin_res;
    std::vector<uint32_t> going_h;
};

extern "C" void aln_pairset_destroy(aln_pairset *ps)
{
    if (!ps) return;
    (void)hipSetDevice(ps->ctx->device);
    if (ps->slot && ps->slot->stream) (void)hipStreamSynchronize(ps->slot->stream);
    for (hipEvent_t e : ps->ev) if (e) (void)hipEventDestroy(e);
    held_free(ps->held_store);
    DevBuf *d[] = {&ps->matrices, &ps->counts, &ps->h_freq, &ps->h_kd, &ps->h_r2, &ps->store, &ps->shared, &ps->h_list, &ps->h_entry, &ps->h_status, &ps->picked,
                   &ps->best, &ps->going[0], &ps->going[1], &ps->cls, &ps->l_tiles, &ps->l_count, &ps->cand_pair, &ps->cand_entry, &ps->fin_pair,
                   &ps->fin_cause, &ps->fin_res};
    for (DevBuf *b : d) dev_free(*b);
    if (ps->owner && ps->slot) ps->slot->seqs = DevBuf{};           // borrowed: the set's to free
    slot_destroy(ps->slot);
    if (ps->owner) seqset_derived_gone(ps->owner);
    delete ps;
}

extern "C" aln_pairset *aln_pairset_create(aln_ctx *ctx, const uint8_t *seqs, const uint64_t *q_off, const uint64_t *q_len,
                                           const uint64_t *t_off, const uint64_t *t_len, size_t n_pairs, int *status)
{
    int st = ALN_OK;
    aln_pairset *ps = nullptr;
    uint64_t total = 0;
    if (!ctx || (n_pairs && (!q_off || !q_len || !t_off || !t_len))) { g_err = "null argument"; st = ALN_ERR_INVALID_ARGUMENT; }
    else if (n_pairs > 0xFFFFFFF0ull) { g_err = "too many pairs"; st = ALN_ERR_UNSUPPORTED; }
    else {
        for (size_t i = 0; i < n_pairs && st == ALN_OK; ++i) {
            if (q_len[i] > 0x7FFFFFF0ull || t_len[i] > 0x7FFFFFF0ull) { g_err = "sequence too long"; st = ALN_ERR_UNSUPPORTED; }
            total += q_len[i] + t_len[i];
        }
        if (st == ALN_OK && total && !seqs) { g_err = "null argument"; st = ALN_ERR_INVALID_ARGUMENT; }
    }
    if (st == ALN_OK) {
        ps = new aln_pairset();
        ps->ctx = ctx->devs[0];
        ps->n = n_pairs;
        ps->residues = total;
        ps->slot = new Slot();
        ps->slot->pooled = false;
        ps->q_off.resize(n_pairs); ps->t_off.resize(n_pairs);
        ps->q_len.assign(q_len, q_len + n_pairs); ps->t_len.assign(t_len, t_len + n_pairs);
        ps->entry_of.assign(n_pairs, -1);
        // the residues, packed in pair order (query, then target): the buffer never moves afterwards
        std::vector<uint8_t> packed(total);
        uint64_t pos = 0;
        for (size_t i = 0; i < n_pairs; ++i) {
            ps->q_off[i] = pos; if (q_len[i]) memcpy(packed.data() + pos, seqs + q_off[i], q_len[i]); pos += q_len[i];
            ps->t_off[i] = pos; if (t_len[i]) memcpy(packed.data() + pos, seqs + t_off[i], t_len[i]); pos += t_len[i];
        }
        hipError_t e = hipSetDevice(ps->ctx->device);
        if (e != hipSuccess) st = fail(e, "hipSetDevice");
        if (st == ALN_OK) st = dev_ensure(ps->slot->seqs, total + 256, false);
        if (st == ALN_OK) st = slot_init(*ps->slot);
        for (int i = 0; i < 6 && st == ALN_OK; ++i) { e = hipEventCreate(&ps->ev[i]); if (e != hipSuccess) st = fail(e, "hipEventCreate"); }
        if (st == ALN_OK && total) {
            e = hipMemcpyAsync(ps->slot->seqs.p, packed.data(), total, hipMemcpyHostToDevice, ps->slot->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ps->slot->stream);
            if (e != hipSuccess) st = fail(e, "upload");
        }
        ps->bytes[0] = total;
        if (st != ALN_OK) { aln_pairset_destroy(ps); ps = nullptr; }
    }
    if (status) *status = st;
    return ps;
}

// the checks of a run that need no device
static int pairset_check_run(const aln_pairset *ps, const aln_params *p, const double *matrices, const uint32_t *active, size_t n_active,
                             const aln_pair_result *results, bool stored = false, bool loop = false)
{
    if (!p) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (p->semantics < ALN_CORE_GLOBAL || p->semantics > ALN_PWM_LOCAL) { g_err = "bad semantics"; return ALN_ERR_INVALID_ARGUMENT; }
    if (p->semantics != ALN_CORE_GLOBAL && p->semantics != ALN_CORE_LOCAL) { g_err = "a pair set runs the core semantics only"; return ALN_ERR_UNSUPPORTED; }
    if (p->heuristics_present) return ALN_ERR_UNNECESSARY_ARGUMENT;
    if (!ps) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (p->matrix) { g_err = "a pair set takes its matrices per pair: params->matrix must be null"; return ALN_ERR_INVALID_ARGUMENT; }
    if (p->rows == 0 || p->cols == 0 || (uint64_t)p->rows * p->cols > ALN_PAIRSET_MAX_ENTRIES) {
        g_err = "per-pair matrices hold 1 .. 1024 entries";
        return ALN_ERR_INVALID_ARGUMENT;
    }
    if (n_active && ((!stored && !matrices) || !active || (!results && !loop))) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (stored && !ps->heur) { g_err = "no heuristics set"; return ALN_ERR_INVALID_ARGUMENT; }
    if (stored && (p->rows != ps->h_rows || p->cols != ps->h_cols)) { g_err = "the shape differs from the store's"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n_active > ps->n) { g_err = "more active entries than pairs"; return ALN_ERR_INVALID_ARGUMENT; }
    std::vector<char> seen(ps->n, 0);
    for (size_t k = 0; k < n_active; ++k) {
        if (active[k] >= ps->n || seen[active[k]]) { g_err = "active: an entry is out of range or listed twice"; return ALN_ERR_INVALID_ARGUMENT; }
        if (stored && !ps->written[active[k]]) { g_err = "active: a pair's store entry was never written"; return ALN_ERR_INVALID_ARGUMENT; }
        seen[active[k]] = 1;
    }
    return ALN_OK;
}

// aln_pairset_run (matrices from the host) and aln_pairset_run_stored (matrices == nullptr: entry k scored by store[active[k]]).
// dev_list (aln_pairset_loop_step): `active` as it already lies on the device -- the list is not uploaded, and the summaries stay there
static int pairset_run(aln_pairset *ps, const aln_params *params, const double *matrices, const uint32_t *active, size_t n_active,
                       aln_pair_result *results, bool stored, const uint32_t *dev_list = nullptr)
{
    int st = pairset_check_run(ps, params, matrices, active, n_active, results, stored, dev_list != nullptr);
    if (st != ALN_OK) return st;
    HIPCHK(hipSetDevice(ps->ctx->device));
    Slot &s = *ps->slot;
    hipStream_t q = s.stream;
    HIPCHK(hipStreamSynchronize(q));
    ps->held = false;
    held_clear(ps->held_store);
    std::fill(ps->entry_of.begin(), ps->entry_of.end(), (int64_t)-1);
    stats_reset(*ps);
    if (n_active == 0) { ps->held = true; ps->rows = params->rows; ps->cols = params->cols; ps->blank = params->blank_code; return ALN_OK; }

    Call c;
    c.p = *params;
    c.p.outputs = ALN_OUT_SCORE | ALN_OUT_TRACEBACK;
    c.core = true;
    c.semantics = params->semantics;
    c.rows = params->rows; c.cols = params->cols;
    c.outs = c.p.outputs;
    c.is_int = false; c.fast = false; c.all_int = false;
    const size_t e = (size_t)c.rows * c.cols;

    std::vector<uint64_t> qo(n_active), ql(n_active), to(n_active), tl(n_active);
    for (size_t k = 0; k < n_active; ++k) {
        const uint32_t i = active[k];
        qo[k] = ps->q_off[i]; ql[k] = ps->q_len[i]; to[k] = ps->t_off[i]; tl[k] = ps->t_len[i];
    }
    if ((st = dev_ensure(ps->matrices, 8ull * e * n_active, false)) != ALN_OK) return st;
    c.pair_matrices = ps->matrices.as<double>();
    const auto t0 = std::chrono::steady_clock::now();
    RefillStats acc;
    if (stored) {
        // the listed store entries, gathered on the device into the compact array the fill reads
        if (!dev_list) {
            if ((st = dev_ensure(ps->h_list, 4ull * n_active, false)) != ALN_OK) return st;
            HIPCHK(hipMemcpyAsync(ps->h_list.p, active, 4ull * n_active, hipMemcpyHostToDevice, q));
        }
        HIPCHK(hipEventRecord(ps->ev[4], q));
        aln_pairset_launch_pick(ps->store.as<double>(), dev_list ? dev_list : ps->h_list.as<uint32_t>(), (uint32_t)n_active, (uint32_t)e,
                                ps->matrices.as<double>(), q);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ps->ev[5], q));
        acc.bytes_up = dev_list ? 0 : 4ull * n_active;
    } else {
        HIPCHK(hipMemcpyAsync(ps->matrices.p, matrices, 8ull * e * n_active, hipMemcpyHostToDevice, q));
        acc.bytes_up = 8ull * e * n_active;
    }
    // (the slot's own residues, or the owner's buffer, where pairs share sequences: neither may grow)
    if ((st = held_refill(ps->held_store, ps->ctx, s, c, qo, ql, to, tl, ps->residues, ps->ev, acc)) != ALN_OK) return st;
    ps->ms[0] = acc.fill_ms; ps->ms[1] = acc.tb_ms;
    ps->bytes[0] = acc.bytes_up;
    if (results) {
        HIPCHK(hipMemcpyAsync(results, ps->held_store.res.p, sizeof(aln_pair_result) * n_active, hipMemcpyDeviceToHost, q));
        HIPCHK(hipStreamSynchronize(q));
    }
    if (stored) ps->ms[2] = ev_ms(ps->ev[4], ps->ev[5]);
    ps->ms[3] = wall_ms(t0);
    ps->bytes[1] = results ? sizeof(aln_pair_result) * n_active : 0;
    for (size_t kk = 0; kk < n_active; ++kk) ps->entry_of[active[kk]] = (int64_t)kk;
    ps->rows = c.rows; ps->cols = c.cols; ps->blank = params->blank_code;
    ps->held = true;
    return ALN_OK;
}

extern "C" int aln_pairset_run(aln_pairset *ps, const aln_params *params, const double *matrices, const uint32_t *active, size_t n_active,
                               aln_pair_result *results)
{
    return pairset_run(ps, params, matrices, active, n_active, results, false);
}

extern "C" int aln_pairset_run_stored(aln_pairset *ps, const aln_params *params, const uint32_t *active, size_t n_active,
                                      aln_pair_result *results)
{
    return pairset_run(ps, params, nullptr, active, n_active, results, true);
}

// ---- the heuristic loop's matrices, re-estimated and kept on the device
extern "C" int aln_pairset_heuristics(aln_pairset *ps, uint32_t rows, uint32_t cols, const double *frequencies, const double *kd,
                                      const double *r_squared)
{
    if (!ps) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (rows == 0 || cols == 0 || (uint64_t)rows * cols > ALN_PAIRSET_MAX_ENTRIES) {
        g_err = "per-pair matrices hold 1 .. 1024 entries";
        return ALN_ERR_INVALID_ARGUMENT;
    }
    if (ps->n && (!frequencies || !kd || !r_squared)) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    HIPCHK(hipSetDevice(ps->ctx->device));
    hipStream_t q = ps->slot->stream;
    HIPCHK(hipStreamSynchronize(q));
    const uint64_t e = (uint64_t)rows * cols;
    // new buffers first: a failure leaves the old parameters and the old store as they were
    DevBuf nb[4];
    const size_t want[4] = {8ull * rows * ps->n, 8ull * ps->n, 8ull * ps->n, 8ull * e * ps->n};
    for (int i = 0; i < 4; ++i) {
        const int st = dev_ensure(nb[i], want[i], false);
        if (st != ALN_OK) {
            for (DevBuf &b : nb) dev_free(b);
            (void)hipGetLastError();
            return st == ALN_ERR_OOM ? ALN_ERR_OOM : st;
        }
    }
    const auto t0 = std::chrono::steady_clock::now();
    hipError_t err = hipSuccess;
    if (ps->n) {
        err = hipMemcpyAsync(nb[0].p, frequencies, want[0], hipMemcpyHostToDevice, q);
        if (err == hipSuccess) err = hipMemcpyAsync(nb[1].p, kd, want[1], hipMemcpyHostToDevice, q);
        if (err == hipSuccess) err = hipMemcpyAsync(nb[2].p, r_squared, want[2], hipMemcpyHostToDevice, q);
        if (err == hipSuccess) err = hipMemsetAsync(nb[3].p, 0, want[3], q);
        if (err == hipSuccess) err = hipStreamSynchronize(q);
    }
    if (err != hipSuccess) { for (DevBuf &b : nb) dev_free(b); return fail(err, "upload"); }
    DevBuf *old[4] = {&ps->h_freq, &ps->h_kd, &ps->h_r2, &ps->store};
    for (int i = 0; i < 4; ++i) { dev_free(*old[i]); *old[i] = nb[i]; }
    ps->written.assign(ps->n, 0);
    ps->h_rows = rows; ps->h_cols = cols;
    ps->heur = true;
    ps->loop = false;                    // the store is new: a loop begins again with aln_pairset_loop_begin
    ps->going_h.clear();
    ps->ms[2] = 0;
    ps->ms[3] = wall_ms(t0);
    ps->bytes[0] = want[0] + want[1] + want[2]; ps->bytes[1] = 0;
    return ALN_OK;
}

extern "C" int aln_pairset_reestimate(aln_pairset *ps, const double *shared_matrix, const uint32_t *which, size_t n, int32_t *status)
{
    if (!ps) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (!ps->heur) { g_err = "no heuristics set"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n && (!which || !status)) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n > ps->n) { g_err = "more listed entries than pairs"; return ALN_ERR_INVALID_ARGUMENT; }
    if (!shared_matrix) {
        if (!ps->held) { g_err = "no held run"; return ALN_ERR_INVALID_ARGUMENT; }
        if (n && (ps->rows != ps->h_rows || ps->cols != ps->h_cols)) { g_err = "the held run's shape differs from the store's"; return ALN_ERR_INVALID_ARGUMENT; }
    }
    std::vector<char> seen(ps->n, 0);
    std::vector<uint32_t> entries(shared_matrix ? 0 : n);
    for (size_t k = 0; k < n; ++k) {
        if (which[k] >= ps->n || seen[which[k]]) { g_err = "which: an entry is out of range or listed twice"; return ALN_ERR_INVALID_ARGUMENT; }
        seen[which[k]] = 1;
        if (!shared_matrix) {
            if (ps->entry_of[which[k]] < 0) { g_err = "a listed pair was not in the last run"; return ALN_ERR_INVALID_ARGUMENT; }
            entries[k] = (uint32_t)ps->entry_of[which[k]];
        }
    }
    if (n == 0) return ALN_OK;
    HIPCHK(hipSetDevice(ps->ctx->device));
    hipStream_t q = ps->slot->stream;
    const uint64_t e = (uint64_t)ps->h_rows * ps->h_cols;
    int st;
    if ((st = dev_ensure(ps->h_list, 4ull * n, false)) != ALN_OK) return st;
    if ((st = dev_ensure(ps->h_status, 4ull * n, false)) != ALN_OK) return st;
    if (shared_matrix) { if ((st = dev_ensure(ps->shared, 8ull * e, false)) != ALN_OK) return st; }
    else if ((st = dev_ensure(ps->h_entry, 4ull * n, false)) != ALN_OK) return st;
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipMemcpyAsync(ps->h_list.p, which, 4ull * n, hipMemcpyHostToDevice, q));
    if (shared_matrix) HIPCHK(hipMemcpyAsync(ps->shared.p, shared_matrix, 8ull * e, hipMemcpyHostToDevice, q));
    else HIPCHK(hipMemcpyAsync(ps->h_entry.p, entries.data(), 4ull * n, hipMemcpyHostToDevice, q));
    PairsetTransformArgs a{};
    a.shared = shared_matrix ? ps->shared.as<double>() : nullptr;
    a.own = nullptr;
    a.held = ps->held_store.info.as<HeldEntry>(); a.res = ps->held_store.res.as<aln_pair_result>(); a.tb = ps->held_store.tb.as<uint8_t>();
    a.entry = ps->h_entry.as<uint32_t>();
    a.par = a.dst_index = ps->h_list.as<uint32_t>();
    a.freq = ps->h_freq.as<double>(); a.kd = ps->h_kd.as<double>(); a.r2 = ps->h_r2.as<double>();
    a.dst = ps->store.as<double>();
    a.status = ps->h_status.as<int32_t>();
    a.n_list = (uint32_t)n; a.n_held = (uint32_t)ps->held_store.n; a.rows = ps->h_rows; a.cols = ps->h_cols; a.blank = ps->blank;
    HIPCHK(hipEventRecord(ps->ev[4], q));
    if (aln_pairset_launch_transform(&a, q) != 0) { g_err = "per-pair matrices hold 1 .. 1024 entries"; return ALN_ERR_INVALID_ARGUMENT; }
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ps->ev[5], q));
    HIPCHK(hipMemcpyAsync(status, ps->h_status.p, 4ull * n, hipMemcpyDeviceToHost, q));
    HIPCHK(hipStreamSynchronize(q));
    for (size_t k = 0; k < n; ++k) if (status[k] == 0) ps->written[which[k]] = 1;
    ps->ms[2] = ev_ms(ps->ev[4], ps->ev[5]);
    ps->ms[3] = wall_ms(t0);
    ps->bytes[0] = (shared_matrix ? 4ull * n + 8ull * e : 8ull * n); ps->bytes[1] = 4ull * n;
    return ALN_OK;
}

extern "C" int aln_pairset_matrices(aln_pairset *ps, const uint32_t *which, size_t n, double *out)
{
    if (!ps) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (!ps->heur) { g_err = "no heuristics set"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n && (!which || !out)) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    for (size_t k = 0; k < n; ++k)
        if (which[k] >= ps->n || !ps->written[which[k]]) { g_err = "which: a pair is out of range or its store entry was never written"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n == 0) return ALN_OK;
    if (n > 0xFFFFFFF0ull) { g_err = "too many entries"; return ALN_ERR_INVALID_ARGUMENT; }
    HIPCHK(hipSetDevice(ps->ctx->device));
    hipStream_t q = ps->slot->stream;
    const uint64_t e = (uint64_t)ps->h_rows * ps->h_cols;
    int st;
    if ((st = dev_ensure(ps->h_list, 4ull * n, false)) != ALN_OK) return st;
    if ((st = dev_ensure(ps->picked, 8ull * e * n, false)) != ALN_OK) return st;
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipMemcpyAsync(ps->h_list.p, which, 4ull * n, hipMemcpyHostToDevice, q));
    HIPCHK(hipEventRecord(ps->ev[4], q));
    aln_pairset_launch_pick(ps->store.as<double>(), ps->h_list.as<uint32_t>(), (uint32_t)n, (uint32_t)e, ps->picked.as<double>(), q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ps->ev[5], q));
    HIPCHK(hipMemcpyAsync(out, ps->picked.p, 8ull * e * n, hipMemcpyDeviceToHost, q));
    HIPCHK(hipStreamSynchronize(q));
    ps->ms[2] = ev_ms(ps->ev[4], ps->ev[5]);
    ps->ms[3] = wall_ms(t0);
    ps->bytes[0] = 4ull * n; ps->bytes[1] = 8ull * e * n;
    return ALN_OK;
}

// transform_matrix for n matrices on the device (the context's first): aln_transform_matrices with aln_pairset_transform_kernel
extern "C" int aln_transform_matrices_device(aln_ctx *ctx, size_t n, uint32_t rows, uint32_t cols, const double *matrices_in,
                                             const double *frequencies, const double *kd, const double *r_squared, double *matrices_out,
                                             int32_t *status)
{
    if (!ctx) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n == 0) return ALN_OK;
    if (!matrices_in || !frequencies || !kd || !r_squared || !matrices_out || !status || rows == 0 || cols == 0 ||
        (uint64_t)rows * cols > ALN_PAIRSET_MAX_ENTRIES) {
        g_err = "null argument, or a matrix outside 1 .. 1024 entries";
        return ALN_ERR_INVALID_ARGUMENT;
    }
    HIPCHK(hipSetDevice(ctx->devs[0]->device));
    const size_t e = (size_t)rows * cols;
    const size_t step = std::max<size_t>(1, std::min<size_t>(n, (256ull << 20) / (8 * e)));      // at most 256 MiB of matrices at a time
    DevBuf m, fr, k, r, stt;
    std::vector<double> back(step * e);
    int st = ALN_OK;
    auto body = [&]() -> int {
        int s2;
        if ((s2 = dev_ensure(m, 8 * e * step, false)) != ALN_OK || (s2 = dev_ensure(fr, 8ull * rows * step, false)) != ALN_OK ||
            (s2 = dev_ensure(k, 8 * step, false)) != ALN_OK || (s2 = dev_ensure(r, 8 * step, false)) != ALN_OK ||
            (s2 = dev_ensure(stt, 4 * step, false)) != ALN_OK)
            return s2;
        for (size_t first = 0; first < n; first += step) {
            const size_t c = std::min(step, n - first);
            HIPCHK(hipMemcpy(m.p, matrices_in + first * e, 8 * e * c, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(fr.p, frequencies + first * rows, 8ull * rows * c, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(k.p, kd + first, 8 * c, hipMemcpyHostToDevice));
            HIPCHK(hipMemcpy(r.p, r_squared + first, 8 * c, hipMemcpyHostToDevice));
            PairsetTransformArgs a{};
            a.own = m.as<double>();
            a.freq = fr.as<double>(); a.kd = k.as<double>(); a.r2 = r.as<double>();
            a.dst = m.as<double>();                                  // in place: a wave holds its source in LDS before it writes
            a.status = stt.as<int32_t>();
            a.n_list = (uint32_t)c; a.rows = rows; a.cols = cols;
            if (aln_pairset_launch_transform(&a, nullptr) != 0) { g_err = "a matrix outside 1 .. 1024 entries"; return ALN_ERR_INVALID_ARGUMENT; }
            HIPCHK(hipGetLastError());
            HIPCHK(hipMemcpy(status + first, stt.p, 4 * c, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(back.data(), m.p, 8 * e * c, hipMemcpyDeviceToHost));
            for (size_t i = 0; i < c; ++i)                           // a matrix without a root is left as it was
                if (status[first + i] == 0) memcpy(matrices_out + (first + i) * e, back.data() + i * e, 8 * e);
        }
        return ALN_OK;
    };
    st = body();
    DevBuf *d[] = {&m, &fr, &k, &r, &stt};
    for (DevBuf *b : d) dev_free(*b);
    return st;
}

// `which` -> held entries; INVALID_ARGUMENT for a pair that was not in the last run
static int pairset_list(aln_pairset *ps, const uint32_t *which, size_t n, std::vector<uint32_t> &entries)
{
    if (!ps) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (!ps->held) { g_err = "no held run"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n && !which) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    entries.resize(n);
    for (size_t k = 0; k < n; ++k) {
        if (which[k] >= ps->n || ps->entry_of[which[k]] < 0) { g_err = "a listed pair was not in the last run"; return ALN_ERR_INVALID_ARGUMENT; }
        entries[k] = (uint32_t)ps->entry_of[which[k]];
    }
    return ALN_OK;
}

extern "C" int aln_pairset_frequencies(aln_pairset *ps, const uint32_t *which, size_t n, uint32_t *counts)
{
    std::vector<uint32_t> entries;
    int st = pairset_list(ps, which, n, entries);
    if (st != ALN_OK) return st;
    if (n && !counts) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n == 0) return ALN_OK;
    HIPCHK(hipSetDevice(ps->ctx->device));
    hipStream_t q = ps->slot->stream;
    const uint64_t cells = (uint64_t)ps->rows * ps->cols;
    if ((st = dev_ensure(ps->held_store.list, 4ull * n, false)) != ALN_OK) return st;
    if ((st = dev_ensure(ps->counts, 4ull * cells * n, false)) != ALN_OK) return st;
    const auto t0 = std::chrono::steady_clock::now();
    HIPCHK(hipMemcpyAsync(ps->held_store.list.p, entries.data(), 4ull * n, hipMemcpyHostToDevice, q));
    HIPCHK(hipEventRecord(ps->ev[0], q));
    aln_pairset_launch_freq(ps->held_store.info.as<HeldEntry>(), ps->held_store.res.as<aln_pair_result>(), ps->held_store.tb.as<uint8_t>(), ps->held_store.list.as<uint32_t>(),
                            (uint32_t)n, (uint32_t)ps->held_store.n, ps->rows, ps->cols, ps->blank, ps->counts.as<uint32_t>(), q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ps->ev[1], q));
    HIPCHK(hipMemcpyAsync(counts, ps->counts.p, 4ull * cells * n, hipMemcpyDeviceToHost, q));
    HIPCHK(hipStreamSynchronize(q));
    ps->ms[2] = ev_ms(ps->ev[0], ps->ev[1]);
    ps->ms[3] = wall_ms(t0);
    ps->bytes[0] = 4ull * n; ps->bytes[1] = 4ull * cells * n;
    return ALN_OK;
}

extern "C" int aln_pairset_strings(aln_pairset *ps, const uint32_t *which, size_t n, aln_pair_result *results, uint8_t *tb_buf,
                                   const uint64_t *tb_off)
{
    std::vector<uint32_t> entries;
    int st = pairset_list(ps, which, n, entries);
    if (st != ALN_OK) return st;
    if (n && (!results || (tb_buf && !tb_off))) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n == 0) return ALN_OK;
    HIPCHK(hipSetDevice(ps->ctx->device));
    return held_fetch_strings(ps->held_store, ps->slot->stream, ps->ev, entries.data(), n, results, tb_buf, tb_off, *ps);
}

extern "C" int aln_pairset_stats(const aln_pairset *ps, double *ms, uint64_t *bytes)
{
    return stats_get(ps, ms, bytes);
}

// ---------------------------------------------------------------- resident sequence set (aln_seqset_*, include/aligner_hip.h)
// The request path of the reference (generate_pairs, dispatcher/handlers.rs:253-264: every pair i < j of a FASTA; blast_p_value_cmp
// and calc: rows of one sequence table): S sequences stay in HBM and a call names a block of the S x S grid.  A call is cut into chunks
// of consecutive pair numbers by the cell bounds of aln_align_batch (and 2^22 pairs).  The host derives a chunk's lengths from
// aln_seqset_rules.h for chunk_plan -- routing, grid and scratch are the batch's -- while the chunk before it runs; the descriptors
// themselves are expanded on the device (aln_seqset.hip), the staged batch's launches (slot_launch) fill them, and what a chunk leaves
// is gathered there: f and status (score), or the pairs at or above a threshold, compacted in pair order (hits).  A held pass then
// plans the re-fill of the hits from their list (the routes and the direction layout depend on every hit's shape, so this plan is the
// host's, as in aln_pairset_run), runs it chunk by chunk and keeps summaries and strings on the device.
// the per-row selection of aln_seqset_best, as a pass carries it from chunk to chunk
struct BestPass { uint32_t slots; uint32_t flags; double f_min; };

#define ALN_SEQSET_CHUNK_PAIRS (1ull << 22)        // per chunk: the pair limit of a chunk of aln_align_batch

// the host's copy of a set's candidate list: pair numbers of `block`, ascending, with their sequence numbers and shared counts (a seed
// join: seeds, and the diagonals beside them).  live: there is a list; has_chain: a chain filter made it, and the kept entries' chain
// records are resident (chain_rec)
struct CandList {
    bool live = false, has_diag = false, has_chain = false;
    aln_seqset_block block = {0, 0, 0, 0, 0, 0};
    std::vector<uint64_t> pair;
    std::vector<uint32_t> qs, ts, shared;
    std::vector<int32_t> diag;
    void clear()
    {
        live = has_diag = has_chain = false;
        pair.clear(); qs.clear(); ts.clear(); shared.clear(); diag.clear();
    }
};

struct aln_seqset : CallStats {
    DevCtx *ctx = nullptr;            // one device: the context's first (as a staged batch)
    Slot *slot = nullptr;             // private slot; slot->seqs holds every sequence once, packed in set order
    size_t n = 0;
    uint64_t total = 0;               // residues
    std::vector<uint64_t> off;        // into slot->seqs
    std::vector<uint32_t> len;
    DevBuf d_off, d_len;              // the same tables on the device (the expansion reads them)
    // a chunk's gathered output: f | status; tile counts | offsets; the chunk's hits (pair number, f); [0] hit count, [2..3] first failure
    DevBuf fbuf, stbuf, tiles, hit_k, hit_f, misc;
    // misc: ALN_SEQSET_MISC_WORDS counter words; which call family owns which word is aln_seqset_rules.h's ALN_SEQSET_MISC_*
    PinBuf h_out;                     // a chunk's f | status | misc on their way to the caller
    // held hits (aln_seqset_hits): the list lives on the host (it is what the re-fill was planned from); hit h is entry h of the
    // store -- until the next pass on this set
    bool held = false;
    std::vector<uint64_t> hit_pair;
    std::vector<double> hit_score;
    std::vector<uint32_t> hit_q, hit_t;
    HeldStore held_store;
    aln_seqset_block held_block = {0, 0, 0, 0, 0, 0};   // the block of the held pass (aln_seqset_held_cluster: its ranges are the nodes)
    // aln_seqset_best: a chunk's piece lists (key | target | count per piece) and the rows' running lists (aln_best.hip)
    DevBuf cand_key, cand_t, cand_n, run_key, run_t, run_n;
    DevBuf row_first;                 // aln_seqset_candidate_best: where every row of the block starts in the candidate list (aln_search.hip)
    // aln_seqset_held_report / _filter: the scheme's bit table, the reports (of a list, or of all held hits), the kept positions | records
    DevBuf rep_bits, reports, rep_pos, rep_out;
    DevBuf cluster;                   // aln_seqset_held_cluster: the call's tables, one arena
    DevBuf profile;                   // aln_seqset_held_profiles: the call's tables and its output, one arena
    uint8_t held_blank = 0;           // the blank code of the held pass (aln_seqset_held_profiles without params)
    // aln_seqset_held_msa_plan / _fill: the plan's tables and the fill's tables and output, an arena each; the passes that replaced the
    // held hits so far, and what the host keeps of the last plan (valid: there is one)
    DevBuf msa, msa_out;
    uint64_t held_passes = 0;
    struct MsaPlan {
        bool valid = false;
        uint64_t passes = 0, n = 0, held = 0, n_centers = 0, n_ins = 0, bytes = 0, total_rows = 0;
        uint32_t blank = 0;
        std::vector<uint64_t> byte_off, row_off;
    } msa_plan;
    // aln_seqset_held_cigar_plan / _fill: the plan's tables (the listed positions, the records, the offsets) and the fill's words, an
    // arena each, and what the host keeps of the last plan
    DevBuf cigar, cigar_out;
    struct CigarPlan {
        bool valid = false;
        bool stranded = false;        // a plan of aln_seqset_held_strand_cigar_plan: cigar_rev marks the listed hits on a mirrored target
        uint64_t passes = 0, n = 0, held = 0, total_ops = 0;
        uint32_t flags = 0, blank = 0;
    } cigar_plan;
    // aln_seqset_create_stranded (aln_strand_rules.h): the caller's records, 0 for a plain set -- n is twice that, records strand_n + i
    // the mirrors; the byte table the mirror kernel read; a stranded plan's marks, one byte per listed hit
    uint64_t strand_n = 0;
    DevBuf strand_map, cigar_rev;
    // the k-mer prefilter (aln_prefilter_rules.h).  The index: one bitmap row of kmer_stride elements and one word count per
    // sequence, resident until the next aln_seqset_kmer_index (kmer_k == 0: none built)
    uint32_t kmer_k = 0, kmer_alphabet = 0, kmer_stride = 0;
    DevBuf kmer_bits, kmer_n;
    // the candidate list of aln_seqset_prefilter or of a join: the block's pair numbers resident (cand_k) and the whole list on the
    // host (cands: the later passes are planned from this copy).  Separate from the held hits: until the next index, prefilter,
    // join, destroy
    CandList cands;
    DevBuf cand_k, pf_shared, pf_keep, pf_out;      // pf_*: a sharing chunk's shared | keep flags | compacted shared
    // the sorted word index (aln_wordjoin_rules.h): the distinct (word, sequence) keys ascending and the word count per sequence,
    // resident until the next aln_seqset_word_index (word_k == 0: none built); beside the bitmap index, not in its place.  wj_*: what
    // a join plans with (where each entry's piece starts | its length | its offset in a chunk | the occurrences per query row) and a
    // chunk's pair numbers before and after the sort, with the sort's own storage
    uint32_t word_k = 0, word_alphabet = 0;
    uint64_t word_entries = 0;
    DevBuf word_e, word_n, wj_first, wj_len, wj_off, wj_occ, wj_a, wj_b, wj_temp;
    // the positional word index (aln_seedjoin_rules.h): every occurrence's key and position, ascending by (word, sequence),
    // resident until the next aln_seqset_seed_index (seed_k == 0: none built); beside the other two indexes.  A seed join plans and
    // sorts in the word join's wj_* buffers and brings sj_diag, a chunk's compacted diagonals
    uint32_t seed_k = 0, seed_alphabet = 0;
    uint64_t seed_entries = 0;
    DevBuf seed_key, seed_pos, sj_diag;
    // the seed chains (aln_seedchain_rules.h).  ch_*: a call's tables -- the listed entries' records (q | t), their anchors (A | what
    // is chained | the 64-bit offsets), their chain records, a run's anchors | states, a filter's kept places; chain_rec: the chain
    // records of the entries a filter kept, resident while cands.has_chain
    DevBuf ch_q, ch_t, ch_seeds, ch_chained, ch_off, ch_rec, ch_anchor, ch_state, ch_pos, chain_rec;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};      // 0 .. 2: a chunk's launches; 4, 5: the best selection
    // pair sets made by aln_pairset_create_from_set read the residue buffer: a destroy with some of them alive releases everything
    // else, moves the buffer here and leaves the rest to the last of them
    size_t derived = 0;
    bool destroyed = false;
    DevBuf residues;
};

// a derived pair set is gone (aln_pairset_destroy)
static void seqset_derived_gone(aln_seqset *ss)
{
    if (ss->derived) --ss->derived;
    if (ss->destroyed && ss->derived == 0) {
        (void)hipSetDevice(ss->ctx->device);
        dev_free(ss->residues);
        delete ss;
    }
}

extern "C" void aln_seqset_destroy(aln_seqset *ss)
{
    if (!ss || ss->destroyed) return;
    (void)hipSetDevice(ss->ctx->device);
    if (ss->slot && ss->slot->stream) (void)hipStreamSynchronize(ss->slot->stream);
    for (hipEvent_t &e : ss->ev) if (e) { (void)hipEventDestroy(e); e = nullptr; }
    held_free(ss->held_store);
    DevBuf *d[] = {&ss->d_off, &ss->d_len, &ss->fbuf, &ss->stbuf, &ss->tiles, &ss->hit_k, &ss->hit_f, &ss->misc, &ss->cand_key, &ss->cand_t, &ss->cand_n,
                   &ss->run_key, &ss->run_t, &ss->run_n, &ss->rep_bits, &ss->reports, &ss->rep_pos, &ss->rep_out, &ss->cluster, &ss->kmer_bits, &ss->kmer_n,
                   &ss->cand_k, &ss->pf_shared, &ss->pf_keep, &ss->pf_out, &ss->row_first, &ss->profile, &ss->msa, &ss->msa_out, &ss->cigar,
                   &ss->cigar_out, &ss->strand_map, &ss->cigar_rev, &ss->word_e, &ss->word_n, &ss->wj_first, &ss->wj_len, &ss->wj_off, &ss->wj_occ, &ss->wj_a, &ss->wj_b, &ss->wj_temp, &ss->seed_key, &ss->seed_pos, &ss->sj_diag,
                   &ss->ch_q, &ss->ch_t, &ss->ch_seeds, &ss->ch_chained, &ss->ch_off, &ss->ch_rec, &ss->ch_anchor, &ss->ch_state, &ss->ch_pos, &ss->chain_rec};
    for (DevBuf *b : d) dev_free(*b);
    pin_free(ss->h_out);
    if (ss->derived && ss->slot) { ss->residues = ss->slot->seqs; ss->slot->seqs = DevBuf{}; }
    slot_destroy(ss->slot);
    ss->slot = nullptr;
    if (ss->derived) { ss->destroyed = true; ss->held = false; ss->cands.clear(); ss->kmer_k = 0; ss->word_k = 0; ss->seed_k = 0; return; }      // the residues go with the last derived pair set
    delete ss;
}

// map: null for a plain set (aln_seqset_create); else the set is stranded (aln_seqset_create_stranded, aln_strand_rules.h): the n_seqs
// records go up as they do for a plain set and the mirror kernel writes n_seqs more behind them
static aln_seqset *seqset_create(aln_ctx *ctx, const uint8_t *seqs, const uint64_t *off, const uint64_t *len, size_t n_seqs, const uint8_t *map,
                                 bool stranded, int *status)
{
    int st = ALN_OK;
    aln_seqset *ss = nullptr;
    uint64_t total = 0;
    if (!ctx || (n_seqs && (!off || !len)) || (stranded && !map)) { g_err = "null argument"; st = ALN_ERR_INVALID_ARGUMENT; }
    else if (stranded && !aln_strand_count_ok(n_seqs)) { g_err = "a stranded sequence set holds fewer than 2^31 records: twice as many are resident"; st = ALN_ERR_INVALID_ARGUMENT; }
    else if ((uint64_t)n_seqs >= (1ull << 32)) { g_err = "a sequence set holds fewer than 2^32 sequences"; st = ALN_ERR_INVALID_ARGUMENT; }
    else {
        for (size_t i = 0; i < n_seqs && st == ALN_OK; ++i) {
            if (len[i] > 0x7FFFFFF0ull) { g_err = "sequence too long"; st = ALN_ERR_UNSUPPORTED; }
            total += len[i];
        }
        if (st == ALN_OK && total && !seqs) { g_err = "null argument"; st = ALN_ERR_INVALID_ARGUMENT; }
    }
    if (st == ALN_OK) {
        ss = new aln_seqset();
        ss->ctx = ctx->devs[0];
        const size_t resident = stranded ? 2 * n_seqs : n_seqs;
        ss->n = resident;
        ss->total = stranded ? 2 * total : total;
        ss->strand_n = stranded ? n_seqs : 0;
        ss->slot = new Slot();
        ss->slot->pooled = false;
        ss->off.resize(resident); ss->len.resize(resident);
        // every sequence once, packed in set order: the buffer never moves afterwards
        std::vector<uint8_t> packed(total);
        uint64_t pos = 0;
        for (size_t i = 0; i < n_seqs; ++i) {
            ss->off[i] = pos; ss->len[i] = (uint32_t)len[i];
            if (len[i]) memcpy(packed.data() + pos, seqs + off[i], len[i]);
            pos += len[i];
        }
        for (size_t i = 0; stranded && i < n_seqs; ++i) { ss->off[n_seqs + i] = aln_strand_mirror_off(total, ss->off[i]); ss->len[n_seqs + i] = ss->len[i]; }
        hipError_t e = hipSetDevice(ss->ctx->device);
        if (e != hipSuccess) st = fail(e, "hipSetDevice");
        if (st == ALN_OK) st = dev_ensure(ss->slot->seqs, stranded ? aln_strand_buffer_bytes(total) : total + 256, false);
        if (st == ALN_OK) st = dev_ensure(ss->d_off, 8ull * resident, false);
        if (st == ALN_OK) st = dev_ensure(ss->d_len, 4ull * resident, false);
        if (st == ALN_OK && stranded) st = dev_ensure(ss->strand_map, 256, false);
        if (st == ALN_OK) st = dev_ensure(ss->misc, 4 * ALN_SEQSET_MISC_WORDS, false);
        if (st == ALN_OK) st = slot_init(*ss->slot);
        for (int i = 0; i < 6 && st == ALN_OK; ++i) { e = hipEventCreate(&ss->ev[i]); if (e != hipSuccess) st = fail(e, "hipEventCreate"); }
        if (st == ALN_OK) {
            hipStream_t q = ss->slot->stream;
            e = hipSuccess;
            if (total) e = hipMemcpyAsync(ss->slot->seqs.p, packed.data(), total, hipMemcpyHostToDevice, q);
            if (e == hipSuccess && n_seqs) e = hipMemcpyAsync(ss->d_off.p, ss->off.data(), 8ull * resident, hipMemcpyHostToDevice, q);
            if (e == hipSuccess && n_seqs) e = hipMemcpyAsync(ss->d_len.p, ss->len.data(), 4ull * resident, hipMemcpyHostToDevice, q);
            if (e == hipSuccess && stranded) {        // the mirrors: behind the uploads on the set's stream
                const auto t0 = std::chrono::steady_clock::now();
                e = hipMemcpyAsync(ss->strand_map.p, map, 256, hipMemcpyHostToDevice, q);
                if (e == hipSuccess) e = hipEventRecord(ss->ev[0], q);
                if (e == hipSuccess) {
                    aln_strand_launch_mirror(ss->slot->seqs.as<uint8_t>(), ss->d_off.as<uint64_t>(), ss->d_len.as<uint32_t>(), n_seqs, total,
                                             ss->strand_map.as<uint8_t>(), q);
                    e = hipGetLastError();
                }
                if (e == hipSuccess) e = hipEventRecord(ss->ev[1], q);
                if (e == hipSuccess) e = hipStreamSynchronize(q);
                if (e == hipSuccess) { ss->ms[2] = ev_ms(ss->ev[0], ss->ev[1]); ss->ms[3] = wall_ms(t0); }
            }
            if (e == hipSuccess) e = hipStreamSynchronize(q);
            if (e != hipSuccess) st = fail(e, "upload");
        }
        ss->bytes[0] = total + 12ull * resident + (stranded ? 256u : 0u);
        if (st != ALN_OK) { aln_seqset_destroy(ss); ss = nullptr; }
    }
    if (status) *status = st;
    return ss;
}

extern "C" aln_seqset *aln_seqset_create(aln_ctx *ctx, const uint8_t *seqs, const uint64_t *off, const uint64_t *len, size_t n_seqs, int *status)
{
    return seqset_create(ctx, seqs, off, len, n_seqs, nullptr, false, status);
}

extern "C" aln_seqset *aln_seqset_create_stranded(aln_ctx *ctx, const uint8_t *seqs, const uint64_t *off, const uint64_t *len, size_t n_seqs,
                                                  const uint8_t map[256], int *status)
{
    return seqset_create(ctx, seqs, off, len, n_seqs, map, true, status);
}

extern "C" uint64_t aln_seqset_strand_records(const aln_seqset *ss)
{
    return ss ? ss->strand_n : 0;
}

// Resident records first .. first + count - 1 as they lie in the residue buffer, record first + k to out + out_off[k]
extern "C" int aln_seqset_strand_residues(aln_seqset *ss, uint64_t first, uint64_t count, const uint64_t *out_off, uint8_t *out)
{
    if (!ss || (count && !out_off)) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (ss->destroyed || !ss->slot) { g_err = "the set was destroyed"; return ALN_ERR_INVALID_ARGUMENT; }
    if (first > ss->n || count > ss->n - first) { g_err = "a record beyond the set"; return ALN_ERR_INVALID_ARGUMENT; }
    uint64_t bytes = 0;
    for (uint64_t k = 0; k < count; ++k) bytes += ss->len[first + k];
    if (bytes && !out) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    HIPCHK(hipSetDevice(ss->ctx->device));
    hipStream_t q = ss->slot->stream;
    const auto t0 = std::chrono::steady_clock::now();
    const int st = run_queued(q, [&]() -> int {
        for (uint64_t k = 0; k < count; ++k) {
            const uint64_t i = first + k;
            if (ss->len[i]) HIPCHK(hipMemcpyAsync(out + out_off[k], ss->slot->seqs.as<uint8_t>() + ss->off[i], ss->len[i], hipMemcpyDeviceToHost, q));
        }
        HIPCHK(hipStreamSynchronize(q));
        return ALN_OK;
    });
    if (st != ALN_OK) return st;
    ss->ms[2] = 0.0; ss->ms[3] = wall_ms(t0);
    ss->bytes[0] = 0; ss->bytes[1] = bytes;
    return ALN_OK;
}

extern "C" uint64_t aln_seqset_pairs(const aln_seqset *ss, const aln_seqset_block *b)
{
    if (!ss || !b) return 0;
    return aln_seqset_block_pairs(ss->n, *b);
}

// the checks of a pass that need no device, and the call's analysis: the longest pair of the block decides the kernels, as the longest
// pair of a batch does (call_init)
static int seqset_call(aln_seqset *ss, const aln_params *params, const aln_seqset_block *b, uint32_t outputs, Call &c)
{
    if (!ss || !params || !b) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (params->semantics == ALN_PWM_LOCAL) { g_err = "a sequence set aligns with the substitution-matrix semantics only"; return ALN_ERR_UNSUPPORTED; }
    if (aln_seqset_block_pairs(ss->n, *b) == 0) { g_err = "block: a range beyond the set, unequal ranges of an upper block, a reserved word, or no pairs"; return ALN_ERR_INVALID_ARGUMENT; }
    uint64_t q1 = 0, t1 = 0;
    if (b->upper) {                                   // i < j: the two longest sequences of the square
        for (uint64_t i = b->q_first; i < b->q_first + b->q_count; ++i) {
            const uint64_t L = ss->len[i];
            if (L > q1) { t1 = q1; q1 = L; } else if (L > t1) t1 = L;
        }
    } else {
        for (uint64_t i = b->q_first; i < b->q_first + b->q_count; ++i) q1 = std::max<uint64_t>(q1, ss->len[i]);
        for (uint64_t i = b->t_first; i < b->t_first + b->t_count; ++i) t1 = std::max<uint64_t>(t1, ss->len[i]);
    }
    aln_params p = *params;
    p.outputs = outputs;
    return call_init(c, &p, &q1, &t1, 1, false);
}

static int seqset_cand_check(aln_seqset *ss)
{
    if (!ss) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (!ss->cands.live) { g_err = "no candidate list: aln_seqset_prefilter has not run, or a new k-mer index has replaced it"; return ALN_ERR_INVALID_ARGUMENT; }
    return ALN_OK;
}

// What a pass runs over: every pair of a block in the block's order (position k is pair k), or the set's candidate list (position h
// is the list's entry h, a pair of the prefilter's block).  A block is walked, by one aln_seqset_unrank and aln_seqset_next after
// it: it may hold far more pairs than a host table should, so nothing is kept per pair beyond what a caller asks for at a time.
struct PairSource {
    aln_seqset *ss;
    bool list;
    const aln_seqset_block *b;        // the block the pair numbers belong to (a list: the prefilter's, once check() has passed)
    uint64_t at = ~0ull, cq = 0, ct = 0;      // the walk: the next position (none before the first seek) and, of a block, its pair

    // what a source refuses before the call's own checks: a list that does not exist
    int check()
    {
        if (!list) return ALN_OK;
        const int st = seqset_cand_check(ss);
        if (st == ALN_OK) b = &ss->cands.block;
        return st;
    }
    uint64_t positions() const { return list ? ss->cands.pair.size() : aln_seqset_block_pairs(ss->n, *b); }
    // cells of all positions together (as a double, like aln_make_chunks): a block's out of the length sums
    double cells() const
    {
        if (list) {
            double sum = 0;
            for (size_t h = 0; h < ss->cands.pair.size(); ++h) sum += (double)ss->len[ss->cands.qs[h]] * (double)ss->len[ss->cands.ts[h]];
            return sum;
        }
        double sq = 0, st = 0, s2 = 0;
        for (uint64_t i = b->q_first; i < b->q_first + b->q_count; ++i) { sq += (double)ss->len[i]; s2 += (double)ss->len[i] * (double)ss->len[i]; }
        if (b->upper) return (sq * sq - s2) / 2.0;
        for (uint64_t i = b->t_first; i < b->t_first + b->t_count; ++i) st += (double)ss->len[i];
        return sq * st;
    }
    void seek(uint64_t k)             // k < positions()
    {
        at = k;
        if (!list) aln_seqset_unrank(*b, k, &cq, &ct);
    }
    // the sequence numbers of position `at`, and on to the next
    void step(uint64_t *q, uint64_t *t)
    {
        if (list) { *q = ss->cands.qs[at]; *t = ss->cands.ts[at]; }
        else { *q = cq; *t = ct; aln_seqset_next(*b, &cq, &ct); }
        ++at;
    }
    // the sequence numbers of positions k0 .. k0 + n - 1 (no seek where the walk stands at k0 already: chunk after chunk)
    void window(uint64_t k0, uint64_t n, std::vector<uint32_t> &q, std::vector<uint32_t> &t)
    {
        if (at != k0) seek(k0);
        q.resize(n); t.resize(n);
        for (uint64_t i = 0; i < n; ++i) {
            uint64_t sq, st;
            step(&sq, &st);
            q[i] = (uint32_t)sq; t[i] = (uint32_t)st;
        }
    }
};

// the cells a chunk of a pass aims at (total cells over `pairs` pairs, one device); *forced: ALN_CHUNK_CELLS said so.  Where the
// chunks are cut is aln_seqset_cut's rule (aln_seqset_rules.h)
static double seqset_chunk_target(const Call &c, double total, uint64_t pairs, bool *forced)
{
    return aln_chunk_cells_override(plan_knobs(), aln_chunk_target(c.fast, total, pairs, 1, 3072.0), forced);
}

// what a chunk of n pairs needs of the set's buffers (the stream is idle: they may grow)
static int seqset_chunk_ensure(aln_seqset *ss, const Call &c, const Chunk &k, uint64_t n, bool want_out, bool select, uint32_t **tile_count,
                               uint32_t **tile_off)
{
    int st;
    if ((st = slot_ensure(*ss->slot, c, k, nullptr, true)) != ALN_OK) return st;
    if ((st = dev_ensure(ss->fbuf, 8 * n, false)) != ALN_OK) return st;
    if ((st = dev_ensure(ss->stbuf, 4 * n, false)) != ALN_OK) return st;
    if ((st = pin_ensure(ss->h_out, 256 + (want_out ? 12 * n : 0))) != ALN_OK) return st;
    if (select) {
        if ((st = tiles_ensure(ss->tiles, aln_seqset_tiles(n), tile_count, tile_off)) != ALN_OK) return st;
        if ((st = dev_ensure(ss->hit_k, 8 * n, false)) != ALN_OK) return st;
        if ((st = dev_ensure(ss->hit_f, 8 * n, false)) != ALN_OK) return st;
    }
    return ALN_OK;
}

// One pass over a source: its positions cut into chunks (aln_seqset_cut, by the cell bounds of aln_make_chunks and the pair limit of a
// chunk), every chunk expanded, filled and gathered on the set's stream.  f / status (optional): the caller's arrays, by position.
// select: the POSITIONS of the chunk's pairs with status ALN_OK and f >= f_min are appended to ss->hit_pair (of a list, the caller
// turns them into pair numbers), their f to hit_score.  *first_bad: the status of the first failed pair, ALN_OK if none failed.
// best: the chunk's f / status go through the piece and merge kernels (a block: aln_best.hip; a list: aln_search.hip, with
// ss->row_first filled by the caller) into the rows' running lists (ss->run_*, zeroed by the caller).
static int seqset_pass_chunks(aln_seqset *ss, const Call &c, PairSource &src, double *f, int32_t *status, bool select, double f_min, int *first_bad,
                              Chunk *plans, const BestPass *best)
{
    Slot &s = *ss->slot;
    hipStream_t q = s.stream;
    std::vector<uint64_t> counts;
    if (const uint64_t positions = src.positions()) {
        const double total = src.cells();
        bool forced = false;
        const double target = seqset_chunk_target(c, total, positions, &forced);
        src.seek(0);
        aln_seqset_cut([&]() { uint64_t sq, sx; src.step(&sq, &sx); return (double)ss->len[sq] * (double)ss->len[sx]; }, positions, total, target,
                       forced, ALN_SEQSET_CHUNK_PAIRS, counts);
    }
    const bool want_out = f != nullptr || status != nullptr;
    std::vector<uint32_t> qs, ts;                  // one chunk's tables: its sequence numbers, then what chunk_plan reads
    std::vector<uint64_t> qo, ql, to, tl;
    // what the chunk in flight leaves behind, collected where the pass waits for it anyway
    uint64_t prev_k0 = 0, prev_n = 0;
    bool timed = false;
    int st = ALN_OK;
    auto collect = [&]() -> int {
        if (timed && best) ss->ms[2] += ev_ms(ss->ev[4], ss->ev[5]);
        if (timed) { ss->ms[0] += ev_ms(ss->ev[0], ss->ev[1]); timed = false; }
        if (!prev_n) return ALN_OK;
        const uint8_t *h = ss->h_out.as<uint8_t>();
        const uint64_t *misc = reinterpret_cast<const uint64_t *>(h);
        if (f) memcpy(f + prev_k0, h + 256, 8 * prev_n);
        if (status) memcpy(status + prev_k0, h + 256 + 8 * prev_n, 4 * prev_n);
        if (*first_bad == ALN_OK && misc[1] != 0) *first_bad = (int)(misc[1] & 0xffu);
        const uint64_t got = (uint32_t)misc[0];
        if (select && got) {
            const size_t at = ss->hit_pair.size();
            ss->hit_pair.resize(at + got); ss->hit_score.resize(at + got);
            HIPCHK(hipMemcpy(ss->hit_pair.data() + at, ss->hit_k.p, 8 * got, hipMemcpyDeviceToHost));
            HIPCHK(hipMemcpy(ss->hit_score.data() + at, ss->hit_f.p, 8 * got, hipMemcpyDeviceToHost));
            ss->bytes[1] += 16 * got;
        }
        prev_n = 0;
        return ALN_OK;
    };
    uint64_t k0 = 0;
    for (size_t j = 0; j < counts.size(); ++j) {
        const uint64_t n = counts[j];
        Chunk &k = plans[j & 1];
        src.window(k0, n, qs, ts);
        qo.resize(n); ql.resize(n); to.resize(n); tl.resize(n);
        for (uint64_t i = 0; i < n; ++i) { qo[i] = ss->off[qs[i]]; ql[i] = ss->len[qs[i]]; to[i] = ss->off[ts[i]]; tl[i] = ss->len[ts[i]]; }
        k.reset();
        if ((st = chunk_plan(ss->ctx, c, qo.data(), ql.data(), to.data(), tl.data(), 0, n, counts.size() == 1, k, counts.size() > 4)) != ALN_OK) break;
        chunk_resident(k, qo.data(), to.data(), n, ss->total);          // the set's own buffer
        bool identity = k.n_small == n;
        for (uint64_t i = 0; i < n && identity; ++i) identity = k.order[i] == (uint32_t)i;
        HIPCHK(hipStreamSynchronize(q));
        if ((st = collect()) != ALN_OK) break;
        // the stream is idle: buffers may grow now
        uint32_t *tile_count = nullptr, *tile_off = nullptr;
        if ((st = seqset_chunk_ensure(ss, c, k, n, want_out, select, &tile_count, &tile_off)) != ALN_OK) break;
        if (best && src.list) {                        // the chunk's sorted pieces, by chunk position
            if ((st = dev_ensure(ss->cand_key, 8 * n, false)) != ALN_OK) break;
            if ((st = dev_ensure(ss->cand_t, 4 * n, false)) != ALN_OK) break;
        } else if (best) {                             // a list of `slots` per piece of a row
            const uint64_t pieces = aln_best_chunk_geometry(k0, n, src.b->t_count).pieces;
            if ((st = dev_ensure(ss->cand_key, 8 * pieces * best->slots, false)) != ALN_OK) break;
            if ((st = dev_ensure(ss->cand_t, 4 * pieces * best->slots, false)) != ALN_OK) break;
            if ((st = dev_ensure(ss->cand_n, 4 * pieces, false)) != ALN_OK) break;
        }
        if (j == 0) {
            if ((st = upload_matrix(s, c, s.h_meta.as<uint8_t>(), q)) != ALN_OK) break;
            ss->bytes[0] += c.md.size() * (c.is_int ? 4 : 8);
        }
        HIPCHK(hipMemsetAsync(ss->misc.p, 0, 16, q));
        if (src.list)
            aln_prefilter_launch_expand_list(s.descs.as<PairDesc>(), s.order.as<uint32_t>(), n, ss->cand_k.as<uint64_t>() + k0, src.b, ss->d_off.as<uint64_t>(),
                                             ss->d_len.as<uint32_t>(), q);
        else
            aln_seqset_launch_expand(s.descs.as<PairDesc>(), s.order.as<uint32_t>(), n, k0, src.b, ss->d_off.as<uint64_t>(), ss->d_len.as<uint32_t>(), q);
        HIPCHK(hipGetLastError());
        if (!identity && k.n_small) {                  // the plan's queue: longest pairs first, without the pairs routed elsewhere
            HIPCHK(hipMemcpyAsync(s.order.p, k.order.data(), 4 * k.n_small, hipMemcpyHostToDevice, q));
            ss->bytes[0] += 4 * k.n_small;
        }
        if ((st = slot_launch(ss->ctx, s, c, k, q, ss->ev, nullptr)) != ALN_OK) break;
        timed = true;
        aln_seqset_launch_gather(s.results.as<aln_pair_result>(), ss->fbuf.as<double>(), ss->stbuf.as<int32_t>(), n,
                                 reinterpret_cast<unsigned long long *>(ss->misc.as<uint8_t>() + 8), q);
        HIPCHK(hipGetLastError());
        if (select) {
            aln_seqset_launch_select(s.results.as<aln_pair_result>(), n, k0, f_min, tile_count, tile_off, ss->misc.as<uint32_t>(), ss->hit_k.as<uint64_t>(), ss->hit_f.as<double>(), q);
            HIPCHK(hipGetLastError());
        }
        if (best) {
            HIPCHK(hipEventRecord(ss->ev[4], q));
            if (src.list) {                            // the rows the chunk's candidates lie in
                const uint64_t t_count = src.b->t_count;
                const uint64_t row0 = aln_search_row(ss->cands.pair[k0], t_count), row1 = aln_search_row(ss->cands.pair[k0 + n - 1], t_count);
                aln_search_launch_chunk(ss->cand_k.as<uint64_t>(), ss->row_first.as<uint32_t>(), ss->fbuf.as<double>(), ss->stbuf.as<int32_t>(), k0, n, row0,
                                        row1 - row0 + 1, src.b, best->f_min, best->flags, best->slots, ss->cand_key.as<uint64_t>(),
                                        ss->cand_t.as<uint32_t>(), ss->run_key.as<uint64_t>(), ss->run_t.as<uint32_t>(), ss->run_n.as<uint32_t>(), q);
            } else
                aln_best_launch_chunk(ss->fbuf.as<double>(), ss->stbuf.as<int32_t>(), n, k0, src.b, best->f_min, best->flags, best->slots,
                                      ss->cand_key.as<uint64_t>(), ss->cand_t.as<uint32_t>(), ss->cand_n.as<uint32_t>(), ss->run_key.as<uint64_t>(),
                                      ss->run_t.as<uint32_t>(), ss->run_n.as<uint32_t>(), q);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(ss->ev[5], q));
        }
        uint8_t *h = ss->h_out.as<uint8_t>();
        HIPCHK(hipMemcpyAsync(h, ss->misc.p, 16, hipMemcpyDeviceToHost, q));
        ss->bytes[1] += 16;
        if (f) { HIPCHK(hipMemcpyAsync(h + 256, ss->fbuf.p, 8 * n, hipMemcpyDeviceToHost, q)); ss->bytes[1] += 8 * n; }
        if (status) { HIPCHK(hipMemcpyAsync(h + 256 + 8 * n, ss->stbuf.p, 4 * n, hipMemcpyDeviceToHost, q)); ss->bytes[1] += 4 * n; }
        prev_k0 = k0; prev_n = n;
        k0 += n;
    }
    if (st != ALN_OK) { (void)hipStreamSynchronize(q); return st; }
    HIPCHK(hipStreamSynchronize(q));
    return collect();
}

// (every way out of a failed pass waits for the stream: queued work reads the plans' queues and writes the pinned staging)
static int seqset_pass(aln_seqset *ss, const Call &c, PairSource &src, double *f, int32_t *status, bool select, double f_min, int *first_bad,
                       const BestPass *best = nullptr)
{
    Chunk plans[2];                    // chunk j's queue may still be on its way while chunk j + 1 is planned
    const int st = seqset_pass_chunks(ss, c, src, f, status, select, f_min, first_bad, plans, best);
    if (st != ALN_OK) (void)hipStreamSynchronize(ss->slot->stream);
    return st;
}

static void seqset_begin(aln_seqset *ss)
{
    ss->held = false;
    ++ss->held_passes;                // (a plan of aln_seqset_held_msa_plan / _cigar_plan is a plan of the held hits it saw)
    ss->hit_pair.clear(); ss->hit_score.clear(); ss->hit_q.clear(); ss->hit_t.clear();
    held_clear(ss->held_store);
    stats_reset(*ss);
}

// The stats of a call that went well, as held_done writes a scan's: its kernels (ev[0] to ev[1], or the sum over its chunks), its wall
// time, the bytes up and down.  Only on success: a refusal or an error leaves the stats of the call before in place.
static void seqset_done(aln_seqset *ss, const std::chrono::steady_clock::time_point &t0, uint64_t up, uint64_t down, double kernel_ms)
{
    ss->ms[2] = kernel_ms;
    ss->ms[3] = wall_ms(t0);
    ss->bytes[0] = up; ss->bytes[1] = down;
}
static void seqset_done(aln_seqset *ss, const std::chrono::steady_clock::time_point &t0, uint64_t up, uint64_t down)
{
    seqset_done(ss, t0, up, down, ev_ms(ss->ev[0], ss->ev[1]));
}

// f and status of every position of a source (aln_seqset_score, aln_seqset_candidate_scores)
static int seqset_run_score(PairSource src, const aln_params *params, double *f, int32_t *status)
{
    aln_seqset *ss = src.ss;
    int st = src.check();
    if (st != ALN_OK) return st;
    Call c;
    if ((st = seqset_call(ss, params, src.b, ALN_OUT_SCORE, c)) != ALN_OK) return st;
    if (!f) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    HIPCHK(hipSetDevice(ss->ctx->device));
    HIPCHK(hipStreamSynchronize(ss->slot->stream));
    seqset_begin(ss);
    const auto t0 = std::chrono::steady_clock::now();
    int bad = ALN_OK;
    st = seqset_pass(ss, c, src, f, status, false, 0.0, &bad);
    ss->ms[3] = wall_ms(t0);
    if (st != ALN_OK) return st;
    if (!status && bad != ALN_OK) { g_err = "a pair failed"; return bad; }
    return ALN_OK;
}

// Holds the ascending pair list in ss->hit_pair / hit_score (what a selection left there): the re-fill with directions, the listed
// pairs as a batch of their own over the resident residues (held_refill), summaries and strings kept in the set's store.  On a
// failure nothing is held (the caller clears the list).
static int seqset_hold_list(aln_seqset *ss, const Call &ct, const aln_seqset_block *b)
{
    const size_t hits = ss->hit_pair.size();
    if (hits > 0xFFFFFFF0ull) { g_err = "too many hits"; return ALN_ERR_UNSUPPORTED; }
    ss->held_blank = ct.p.blank_code;
    if (!hits) return ALN_OK;
    std::vector<uint64_t> qo(hits), ql(hits), to(hits), tl(hits);
    ss->hit_q.resize(hits); ss->hit_t.resize(hits);
    for (size_t h = 0; h < hits; ++h) {
        uint64_t sq, tq;
        aln_seqset_unrank(*b, ss->hit_pair[h], &sq, &tq);
        ss->hit_q[h] = (uint32_t)sq; ss->hit_t[h] = (uint32_t)tq;
        qo[h] = ss->off[sq]; ql[h] = ss->len[sq]; to[h] = ss->off[tq]; tl[h] = ss->len[tq];
    }
    RefillStats acc;
    const int st = held_refill(ss->held_store, ss->ctx, *ss->slot, ct, qo, ql, to, tl, ss->total, ss->ev, acc);
    ss->ms[1] += acc.both_ms;
    ss->bytes[0] += acc.bytes_up;
    return st;
}

// The positions of a source at or above a threshold, held (aln_seqset_hits, aln_seqset_candidate_hits): the held state after a
// list is exactly what a block pass would hold for those pairs.
static int seqset_run_hits(PairSource src, const aln_params *params, double f_min, uint64_t *count)
{
    aln_seqset *ss = src.ss;
    int st = src.check();
    if (st != ALN_OK) return st;
    Call c, ct;
    const aln_seqset_block *b = src.b;
    if ((st = seqset_call(ss, params, b, ALN_OUT_SCORE, c)) != ALN_OK) return st;
    if (!count) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if ((st = seqset_call(ss, params, b, ALN_OUT_SCORE | ALN_OUT_TRACEBACK, ct)) != ALN_OK) return st;
    HIPCHK(hipSetDevice(ss->ctx->device));
    HIPCHK(hipStreamSynchronize(ss->slot->stream));
    seqset_begin(ss);
    *count = 0;
    const auto t0 = std::chrono::steady_clock::now();
    int bad = ALN_OK;
    if ((st = seqset_pass(ss, c, src, nullptr, nullptr, true, f_min, &bad)) != ALN_OK) { seqset_begin(ss); return st; }
    // the selection numbered a list's candidates by list position: the held list speaks of pairs of the block
    if (src.list)
        for (uint64_t &p : ss->hit_pair) {
            if (p >= ss->cands.pair.size()) { g_err = "the selection's list leaves the candidate list"; seqset_begin(ss); return ALN_ERR_DEVICE; }
            p = ss->cands.pair[p];
        }
    if ((st = seqset_hold_list(ss, ct, b)) != ALN_OK) { seqset_begin(ss); return st; }
    ss->ms[3] = wall_ms(t0);
    ss->held = true;
    ss->held_block = *b;
    *count = ss->hit_pair.size();
    return ALN_OK;
}

// The finish of a per-row selection (aln_seqset_best, aln_seqset_candidate_best): the rows' counts -> offsets and the total, then
// (sized for exactly the total) the ascending pair list of block b in ss->hit_pair / hit_score.  On a failure the caller waits for
// the stream and clears the list.
static int seqset_best_finish(aln_seqset *ss, const aln_seqset_block *b, uint32_t slots, uint32_t *tile_count, uint64_t *tile_off, uint64_t *out_total)
{
    hipStream_t q = ss->slot->stream;
    const uint64_t rows = b->q_count;
    uint64_t *d_total = reinterpret_cast<uint64_t *>(ss->misc.as<uint8_t>() + 32);
    uint64_t total = 0;
    HIPCHK(hipEventRecord(ss->ev[4], q));
    aln_best_launch_count(ss->run_n.as<uint32_t>(), rows, tile_count, tile_off, d_total, q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(&total, d_total, 8, hipMemcpyDeviceToHost, q));
    HIPCHK(hipStreamSynchronize(q));
    ss->bytes[1] += 8;
    if (total > 0xFFFFFFF0ull) { g_err = "too many hits"; return ALN_ERR_UNSUPPORTED; }
    if (total) {
        int e = dev_ensure(ss->hit_k, 8 * total, false);
        if (e == ALN_OK) e = dev_ensure(ss->hit_f, 8 * total, false);
        if (e != ALN_OK) return e;
        aln_best_launch_emit(ss->run_key.as<uint64_t>(), ss->run_t.as<uint32_t>(), ss->run_n.as<uint32_t>(), rows, slots, b, tile_off, total,
                             ss->hit_k.as<uint64_t>(), ss->hit_f.as<double>(), q);
        HIPCHK(hipGetLastError());
    }
    HIPCHK(hipEventRecord(ss->ev[5], q));
    ss->hit_pair.resize(total); ss->hit_score.resize(total);
    if (total) {
        HIPCHK(hipMemcpyAsync(ss->hit_pair.data(), ss->hit_k.p, 8 * total, hipMemcpyDeviceToHost, q));
        HIPCHK(hipMemcpyAsync(ss->hit_score.data(), ss->hit_f.p, 8 * total, hipMemcpyDeviceToHost, q));
        ss->bytes[1] += 16 * total;
    }
    HIPCHK(hipStreamSynchronize(q));
    ss->ms[2] += ev_ms(ss->ev[4], ss->ev[5]);
    // the host indexes its tables with this list: pairs of the block, ascending
    const uint64_t pairs = aln_seqset_block_pairs(ss->n, *b);
    for (uint64_t h = 0; h < total; ++h)
        if (ss->hit_pair[h] >= pairs || (h && ss->hit_pair[h] <= ss->hit_pair[h - 1])) { g_err = "the selection's list is not an ascending list of the block's pairs"; return ALN_ERR_DEVICE; }
    *out_total = total;
    return ALN_OK;
}

// The k best targets per query row of a source (aln_seqset_best, aln_seqset_candidate_best): the pass of hits with the per-row
// selection of aln_best.hip (a list: of aln_search.hip, which finds a row's candidates through row_first) in place of the
// threshold's, then the rows' lists as one ascending pair list, held like the hits.
static int seqset_run_best(PairSource src, const aln_params *params, uint32_t k, double f_min, uint32_t flags, uint64_t *count)
{
    aln_seqset *ss = src.ss;
    int st = src.check();
    if (st != ALN_OK) return st;
    Call c, ct;
    const aln_seqset_block *b = src.b;
    if ((st = seqset_call(ss, params, b, ALN_OUT_SCORE, c)) != ALN_OK) return st;
    if (!count) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (k < 1u || k > ALN_SEQSET_BEST_MAX) { g_err = "k must lie in 1 .. ALN_SEQSET_BEST_MAX"; return ALN_ERR_INVALID_ARGUMENT; }
    if (flags & ~ALN_BEST_SKIP_SELF) { g_err = "unknown flag bits"; return ALN_ERR_INVALID_ARGUMENT; }
    if (b->upper) { g_err = "the k best per query are defined on a rectangle: a pair of an upper block belongs to both of its sequences"; return ALN_ERR_UNSUPPORTED; }
    if ((st = seqset_call(ss, params, b, ALN_OUT_SCORE | ALN_OUT_TRACEBACK, ct)) != ALN_OK) return st;
    HIPCHK(hipSetDevice(ss->ctx->device));
    hipStream_t q = ss->slot->stream;
    HIPCHK(hipStreamSynchronize(q));
    seqset_begin(ss);
    if (src.list) *count = 0;          // (a block's best leaves *count alone unless it succeeds, as it always has)
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t rows = b->q_count, listed = src.list ? src.positions() : 0;
    BestPass best;
    best.slots = aln_best_slots(k, b->t_count); best.flags = flags; best.f_min = f_min;
    // the rows' running lists and, for a list, their places in it, for this call
    st = dev_ensure(ss->run_key, 8 * rows * best.slots, false);
    if (st == ALN_OK) st = dev_ensure(ss->run_t, 4 * rows * best.slots, false);
    if (st == ALN_OK) st = dev_ensure(ss->run_n, 4 * rows, false);
    if (st == ALN_OK && src.list) st = dev_ensure(ss->row_first, 4 * (rows + 1), false);
    uint32_t *tile_count;
    uint64_t *tile_off;
    if (st == ALN_OK) st = tiles_ensure(ss->tiles, aln_best_tiles(rows), &tile_count, &tile_off);
    if (st != ALN_OK) return st;
    HIPCHK(hipMemsetAsync(ss->run_n.p, 0, 4 * rows, q));
    if (listed) {
        HIPCHK(hipEventRecord(ss->ev[4], q));
        aln_search_launch_rows(ss->cand_k.as<uint64_t>(), listed, rows, b->t_count, ss->row_first.as<uint32_t>(), q);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ss->ev[5], q));
        HIPCHK(hipStreamSynchronize(q));
        ss->ms[2] += ev_ms(ss->ev[4], ss->ev[5]);
    }
    int bad = ALN_OK;
    if ((st = seqset_pass(ss, c, src, nullptr, nullptr, false, 0.0, &bad, &best)) != ALN_OK) { seqset_begin(ss); return st; }
    uint64_t total = 0;
    st = seqset_best_finish(ss, b, best.slots, tile_count, tile_off, &total);
    if (st == ALN_OK) st = seqset_hold_list(ss, ct, b);
    if (st != ALN_OK) { (void)hipStreamSynchronize(q); seqset_begin(ss); return st; }
    ss->ms[3] = wall_ms(t0);
    ss->held = true;
    ss->held_block = *b;
    *count = total;
    return ALN_OK;
}

// The one way through the C boundary for every call below that allocates host memory: what cannot be had is ALN_ERR_OOM, not an
// exception, and with a device behind the handle (`live`) everything queued has finished before the caller hears of it.
#define ALN_GUARDED(live, call)                                                                   \
    try {                                                                                         \
        return call;                                                                              \
    } catch (const std::bad_alloc &) {                                                            \
        if (live) (void)hipDeviceSynchronize();                                                   \
        g_err = "out of host memory";                                                             \
        return ALN_ERR_OOM;                                                                       \
    }
static bool seqset_live(const aln_seqset *ss) { return ss && ss->slot && ss->slot->stream; }

extern "C" int aln_seqset_score(aln_seqset *ss, const aln_params *params, const aln_seqset_block *b, double *f, int32_t *status)
{
    ALN_GUARDED(seqset_live(ss), seqset_run_score(PairSource{ss, false, b}, params, f, status))
}

extern "C" int aln_seqset_hits(aln_seqset *ss, const aln_params *params, const aln_seqset_block *b, double f_min, uint64_t *count)
{
    ALN_GUARDED(seqset_live(ss), seqset_run_hits(PairSource{ss, false, b}, params, f_min, count))
}

extern "C" int aln_seqset_best(aln_seqset *ss, const aln_params *params, const aln_seqset_block *b, uint32_t k, double f_min, uint32_t flags,
                               uint64_t *count)
{
    ALN_GUARDED(seqset_live(ss), seqset_run_best(PairSource{ss, false, b}, params, k, f_min, flags, count))
}

// ---------------------------------------------------------------- the k-mer prefilter (include/aligner_hip_prefilter.h)
// Words first, the dynamic programme on the candidates only.  The index and the candidate list are state of their own beside the held
// hits; the candidate passes are the passes of score, hits and best over a PairSource that names the list: their chunks are runs of
// consecutive list positions.
static void seqset_drop_candidates(aln_seqset *ss) { ss->cands.clear(); }

// the refusals that every route to the candidate list words alike
static const char *const CAND_SPEC_WORDS = "the spec's flags and reserved word must be 0";
static const char *const CAND_BLOCK = "block: a range beyond the set, unequal ranges of an upper block, a reserved word, or no pairs";

static int seqset_kmer_index(aln_seqset *ss, uint32_t k, uint32_t alphabet, uint32_t *n_words)
{
    if (!ss) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    const uint32_t bits = aln_prefilter_bits(k, alphabet);
    if (!bits) { g_err = "k must lie in 1 .. 8, the alphabet size be at least 1 and alphabet^k at most 2^18"; return ALN_ERR_INVALID_ARGUMENT; }
    HIPCHK(hipSetDevice(ss->ctx->device));
    hipStream_t q = ss->slot->stream;
    HIPCHK(hipStreamSynchronize(q));
    const auto t0 = std::chrono::steady_clock::now();
    const uint32_t elements = aln_prefilter_elements(bits), stride = aln_prefilter_stride(bits);
    // the new table first: a failure leaves the old index and the candidate list as they were
    DevBuf table, counts;
    int st = dev_ensure(table, 4ull * stride * ss->n, false);
    if (st == ALN_OK) st = dev_ensure(counts, 4ull * ss->n, false);
    std::vector<uint32_t> counts_h(n_words ? ss->n : 0);
    if (st == ALN_OK) st = run_queued(q, [&]() -> int {
        HIPCHK(hipEventRecord(ss->ev[0], q));
        aln_prefilter_launch_index(ss->slot->seqs.as<uint8_t>(), ss->d_off.as<uint64_t>(), ss->d_len.as<uint32_t>(), ss->n, k, alphabet, elements,
                                   stride, table.as<uint32_t>(), counts.as<uint32_t>(), q);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ss->ev[1], q));
        if (n_words && ss->n) HIPCHK(hipMemcpyAsync(counts_h.data(), counts.p, 4ull * ss->n, hipMemcpyDeviceToHost, q));
        HIPCHK(hipStreamSynchronize(q));
        return ALN_OK;
    });
    if (st != ALN_OK) { dev_free(table); dev_free(counts); return st; }
    dev_free(ss->kmer_bits); dev_free(ss->kmer_n);
    ss->kmer_bits = table; ss->kmer_n = counts;
    ss->kmer_k = k; ss->kmer_alphabet = alphabet; ss->kmer_stride = stride;
    seqset_drop_candidates(ss);
    if (n_words && ss->n) memcpy(n_words, counts_h.data(), 4ull * ss->n);
    seqset_done(ss, t0, 0, n_words ? 4ull * ss->n : 0);
    return ALN_OK;
}

// room for `entries` pair numbers in the resident list, the first `used` of them kept (the stream is idle)
static int seqset_cand_room(aln_seqset *ss, uint64_t used, uint64_t entries)
{
    if (ss->cand_k.cap >= 8 * entries) return ALN_OK;
    DevBuf bigger;
    const int st = dev_ensure(bigger, std::max<uint64_t>(8 * entries, used ? 2 * ss->cand_k.cap : 0), false);
    if (st != ALN_OK) return st;
    if (used) {
        const hipError_t e = hipMemcpy(bigger.p, ss->cand_k.p, 8 * used, hipMemcpyDeviceToDevice);
        if (e != hipSuccess) { dev_free(bigger); return fail(e, "hipMemcpy"); }
    }
    dev_free(ss->cand_k);
    ss->cand_k = bigger;
    return ALN_OK;
}

// What the three routes to the candidate list (prefilter, word join, seed join) do alike.
// A chunk's `got` kept pairs, compacted behind the `total` that are there, come down with their shared counts (pf_out), 12 bytes per
// pair: at most `room` of them (`more` says so), and the host indexes its tables with this list, so it must be pairs
// k_lo .. k_end - 1 of the block, ascending (the stream is idle)
static int seqset_cand_append(aln_seqset *ss, uint64_t total, uint64_t got, uint64_t room, const char *more, uint64_t k_lo, uint64_t k_end,
                              uint64_t *down)
{
    if (got > room) { g_err = more; return ALN_ERR_DEVICE; }
    if (total + got > 0xFFFFFFF0ull) { g_err = "too many candidates"; return ALN_ERR_UNSUPPORTED; }
    *down += 12ull * got;
    if (!got) return ALN_OK;
    ss->cands.pair.resize(total + got); ss->cands.shared.resize(total + got);
    HIPCHK(hipMemcpy(ss->cands.pair.data() + total, ss->cand_k.as<uint64_t>() + total, 8ull * got, hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(ss->cands.shared.data() + total, ss->pf_out.p, 4ull * got, hipMemcpyDeviceToHost));
    for (uint64_t i = total; i < total + got; ++i)
        if (ss->cands.pair[i] < k_lo || ss->cands.pair[i] >= k_end || (i > total && ss->cands.pair[i] <= ss->cands.pair[i - 1])) { g_err = "the candidate list is not an ascending list of the chunk's pairs"; return ALN_ERR_DEVICE; }
    return ALN_OK;
}

// the list is complete: its sequence numbers, and the state the candidate calls read
static void seqset_cand_finish(aln_seqset *ss, const aln_seqset_block *b, uint64_t total, uint64_t *count)
{
    ss->cands.qs.resize(total); ss->cands.ts.resize(total);
    for (uint64_t i = 0; i < total; ++i) {
        uint64_t sq, tq;
        aln_seqset_unrank(*b, ss->cands.pair[i], &sq, &tq);
        ss->cands.qs[i] = (uint32_t)sq; ss->cands.ts[i] = (uint32_t)tq;
    }
    ss->cands.live = true;
    ss->cands.block = *b;
    *count = total;
}

// the query rows of a join cut into chunks: cut(first) gives the rows of the chunk that starts at row `first`, 0 if that row alone is
// above the cap (ALN_ERR_CAPACITY with `over`); a run of rows without anything to expand is no chunk
template <class Cut> static int seqset_cut_rows(const std::vector<uint64_t> &per_row, Cut cut, const char *over, std::vector<uint64_t> &chunk_first,
                                                std::vector<uint64_t> &chunk_rows, std::vector<uint64_t> &chunk_sum)
{
    for (uint64_t first = 0; first < per_row.size();) {
        const uint64_t n = cut(first);
        if (!n) { g_err = over; return ALN_ERR_CAPACITY; }
        uint64_t sum = 0;
        for (uint64_t r = first; r < first + n; ++r) sum += per_row[r];
        if (sum) { chunk_first.push_back(first); chunk_rows.push_back(n); chunk_sum.push_back(sum); }
        first += n;
    }
    return ALN_OK;
}

static int seqset_prefilter(aln_seqset *ss, const aln_prefilter_spec *sp, const aln_seqset_block *b, uint64_t *count)
{
    if (!ss || !sp || !b || !count) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (!aln_prefilter_bits(sp->k, sp->alphabet)) { g_err = "k must lie in 1 .. 8, the alphabet size be at least 1 and alphabet^k at most 2^18"; return ALN_ERR_INVALID_ARGUMENT; }
    if (!ss->kmer_k || sp->k != ss->kmer_k || sp->alphabet != ss->kmer_alphabet) { g_err = "no k-mer index of this k and alphabet: aln_seqset_kmer_index builds it"; return ALN_ERR_INVALID_ARGUMENT; }
    if (sp->min_per_1024 > ALN_PREFILTER_MAX_PER_1024) { g_err = "min_per_1024 must lie in 0 .. 1024"; return ALN_ERR_INVALID_ARGUMENT; }
    if (sp->flags != 0u || sp->reserved != 0u) { g_err = CAND_SPEC_WORDS; return ALN_ERR_INVALID_ARGUMENT; }
    if (sp->chunk_pairs > ALN_PREFILTER_CHUNK_PAIRS) { g_err = "chunk_pairs must lie in 0 .. 2^22"; return ALN_ERR_INVALID_ARGUMENT; }
    const uint64_t pairs = aln_seqset_block_pairs(ss->n, *b);
    if (pairs == 0) { g_err = CAND_BLOCK; return ALN_ERR_INVALID_ARGUMENT; }
    HIPCHK(hipSetDevice(ss->ctx->device));
    hipStream_t q = ss->slot->stream;
    HIPCHK(hipStreamSynchronize(q));
    const auto t0 = std::chrono::steady_clock::now();
    seqset_drop_candidates(ss);
    const uint64_t per = sp->chunk_pairs ? sp->chunk_pairs : ALN_PREFILTER_CHUNK_PAIRS;
    const uint64_t t_end = b->t_first + b->t_count;
    uint64_t total = 0, down = 0;
    double kernels = 0;
    const int st = run_queued(q, [&]() -> int {
        int st;
        for (uint64_t k0 = 0; k0 < pairs; k0 += per) {
            const uint64_t n = std::min(per, pairs - k0);
            // the chunk's pairs lie in query rows q_lo .. q_hi; its targets in t_lo .. (one row: exactly its own)
            uint64_t q_lo, t_a, q_hi, t_b;
            aln_seqset_unrank(*b, k0, &q_lo, &t_a);
            aln_seqset_unrank(*b, k0 + n - 1, &q_hi, &t_b);
            const uint64_t t_lo = q_lo == q_hi ? t_a : (b->upper ? q_lo + 1 : b->t_first);
            const uint64_t t_count = q_lo == q_hi ? n : t_end - t_lo;
            if (!aln_prefilter_share_blocks(q_hi - q_lo + 1, t_count)) { g_err = "a sharing chunk of more tiles than a grid holds"; return ALN_ERR_UNSUPPORTED; }
            uint32_t *tile_count = nullptr, *tile_off = nullptr;
            if ((st = dev_ensure(ss->pf_shared, 4 * n, false)) != ALN_OK) return st;
            if ((st = dev_ensure(ss->pf_keep, n, false)) != ALN_OK) return st;
            if ((st = dev_ensure(ss->pf_out, 4 * n, false)) != ALN_OK) return st;
            if ((st = tiles_ensure(ss->tiles, aln_seqset_tiles(n), &tile_count, &tile_off)) != ALN_OK) return st;
            if ((st = seqset_cand_room(ss, total, total + n)) != ALN_OK) return st;
            uint32_t *d_count = ss->misc.as<uint32_t>() + ALN_SEQSET_MISC_COMPACT;
            HIPCHK(hipEventRecord(ss->ev[0], q));
            aln_prefilter_launch_share(ss->kmer_bits.as<uint32_t>(), ss->kmer_n.as<uint32_t>(), ss->kmer_stride, b, k0, n, q_lo, q_hi - q_lo + 1, t_lo,
                                       t_count, sp->min_shared, sp->min_per_1024, ss->pf_shared.as<uint32_t>(), ss->pf_keep.as<uint8_t>(), q);
            HIPCHK(hipGetLastError());
            aln_prefilter_launch_compact(ss->pf_keep.as<uint8_t>(), ss->pf_shared.as<uint32_t>(), n, k0, tile_count, tile_off, d_count, n,
                                         ss->cand_k.as<uint64_t>() + total, ss->pf_out.as<uint32_t>(), q);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(ss->ev[1], q));
            uint32_t got = 0;
            HIPCHK(hipMemcpyAsync(&got, d_count, 4, hipMemcpyDeviceToHost, q));
            HIPCHK(hipStreamSynchronize(q));
            kernels += ev_ms(ss->ev[0], ss->ev[1]);
            down += 8;
            if ((st = seqset_cand_append(ss, total, got, n, "the compaction kept more pairs than the chunk holds", k0, k0 + n, &down)) != ALN_OK) return st;
            total += got;
        }
        return ALN_OK;
    });
    if (st != ALN_OK) { seqset_drop_candidates(ss); return st; }
    seqset_cand_finish(ss, b, total, count);
    seqset_done(ss, t0, 0, down, kernels);          // 12 bytes per candidate and the 8 of a chunk's count
    return ALN_OK;
}

extern "C" int aln_seqset_kmer_index(aln_seqset *ss, uint32_t k, uint32_t alphabet, uint32_t *n_words)
{
    ALN_GUARDED(seqset_live(ss), seqset_kmer_index(ss, k, alphabet, n_words))
}

extern "C" int aln_seqset_prefilter(aln_seqset *ss, const aln_prefilter_spec *spec, const aln_seqset_block *b, uint64_t *count)
{
    ALN_GUARDED(seqset_live(ss), seqset_prefilter(ss, spec, b, count))
}

extern "C" int aln_seqset_candidates(aln_seqset *ss, uint64_t first, uint64_t n, uint64_t *pair_index, uint32_t *q_seq, uint32_t *t_seq,
                                     uint32_t *shared)
{
    int st = seqset_cand_check(ss);
    if (st != ALN_OK) return st;
    const uint64_t have = ss->cands.pair.size();
    if (first > have || n > have - first) { g_err = "range beyond the candidate list"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n && (!pair_index || !q_seq || !t_seq || !shared)) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    for (uint64_t i = 0; i < n; ++i) {
        pair_index[i] = ss->cands.pair[first + i]; q_seq[i] = ss->cands.qs[first + i]; t_seq[i] = ss->cands.ts[first + i];
        shared[i] = ss->cands.shared[first + i];
    }
    return ALN_OK;                       // (no byte moves and no kernel runs: the stats stay as they are)
}

extern "C" int aln_seqset_candidate_scores(aln_seqset *ss, const aln_params *params, double *f, int32_t *status)
{
    ALN_GUARDED(seqset_live(ss), seqset_run_score(PairSource{ss, true, nullptr}, params, f, status))
}

extern "C" int aln_seqset_candidate_hits(aln_seqset *ss, const aln_params *params, double f_min, uint64_t *count)
{
    ALN_GUARDED(seqset_live(ss), seqset_run_hits(PairSource{ss, true, nullptr}, params, f_min, count))
}

extern "C" int aln_seqset_candidate_best(aln_seqset *ss, const aln_params *params, uint32_t k, double f_min, uint32_t flags, uint64_t *count)
{
    ALN_GUARDED(seqset_live(ss), seqset_run_best(PairSource{ss, true, nullptr}, params, k, f_min, flags, count))
}

// ---------------------------------------------------------------- the posting-list routes: the sorted word index and its join
// (include/aligner_hip_wordjoin.h), the positional word index and the seed join (include/aligner_hip_seedjoin.h)
// The prefilter's candidate list by two more roads.  The word index holds every (word, sequence) once, sorted, and its join names the
// pairs by the posting lists; the seed index keeps every occurrence with its position, and its join judges a pair by the most seeds
// it has within one band of diagonals.  What either leaves behind is the candidate state above (`shared` holds seeds after a seed
// join, the diagonals lie beside it), so the candidate passes, aln_seqset_candidates and the held calls know no difference.
static const char *const WORDJOIN_RANGE = "k must lie in 1 .. 8, the alphabet size be at least 1 and alphabet^k at most 2^32";
static const char *const SEEDJOIN_RANGE = "k must lie in 1 .. 16, the alphabet size be at least 1 and alphabet^k at most 2^32";

// ---- both index builds: the key of every residue position, sorted by (word, seq); then the word index keeps the distinct keys and
// n(s), the seed index (seed) every occurrence with its position.  *entries: how many it holds
static int seqset_posting_index(aln_seqset *ss, uint32_t k, uint32_t alphabet, uint64_t words, bool seed, uint32_t *n_words, uint32_t *entries)
{
    HIPCHK(hipSetDevice(ss->ctx->device));
    hipStream_t q = ss->slot->stream;
    HIPCHK(hipStreamSynchronize(q));
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t total = ss->total;
    uint32_t seq_end, word_end;
    aln_wordjoin_sort_bits(words, ss->n, &seq_end, &word_end);
    // everything new first: a failure leaves the old index and the candidate list as they were.  a | b: the keys before | after a
    // pass of the sort, pos_*: their positions; keep: the resident list; aux: n(s), or the resident positions
    DevBuf a, b, pos_a, pos_b, temp, keep, aux;
    std::vector<uint32_t> counts_h(n_words ? ss->n : 0);
    uint32_t got = 0;
    uint32_t *d_count = ss->misc.as<uint32_t>() + (seed ? ALN_SEQSET_MISC_SEED : ALN_SEQSET_MISC_WORD) + ALN_JOIN_MISC_KEPT;
    auto pass = [&](uint32_t begin, uint32_t end) -> int {      // a -> b over bits begin .. end - 1, then the names change places
        if (seed) HIPCHK((hipError_t)aln_seedjoin_launch_sort_pairs(temp.p, temp.cap, a.as<uint64_t>(), b.as<uint64_t>(), pos_a.as<uint32_t>(), pos_b.as<uint32_t>(), total, begin, end, q));
        else HIPCHK((hipError_t)aln_wordjoin_launch_sort(temp.p, temp.cap, a.as<uint64_t>(), b.as<uint64_t>(), total, begin, end, q));
        std::swap(a, b); std::swap(pos_a, pos_b);
        return ALN_OK;
    };
    const int st = run_queued(q, [&]() -> int {
        int st;
        size_t temp_bytes = 0;
        uint32_t *tile_count = nullptr, *tile_off = nullptr;
        if (seed) HIPCHK((hipError_t)aln_seedjoin_sort_pairs_temp_bytes(total, &temp_bytes));
        else HIPCHK((hipError_t)aln_wordjoin_sort_temp_bytes(total, &temp_bytes));
        if ((st = dev_ensure(a, 8 * total, false)) != ALN_OK) return st;
        if ((st = dev_ensure(b, 8 * total, false)) != ALN_OK) return st;
        if (seed && (st = dev_ensure(pos_a, 4 * total, false)) != ALN_OK) return st;
        if (seed && (st = dev_ensure(pos_b, 4 * total, false)) != ALN_OK) return st;
        if ((st = dev_ensure(temp, temp_bytes, false)) != ALN_OK) return st;
        if (!seed && (st = dev_ensure(aux, 4ull * ss->n, false)) != ALN_OK) return st;
        if (!seed && (st = tiles_ensure(ss->tiles, aln_seqset_tiles(total), &tile_count, &tile_off)) != ALN_OK) return st;
        HIPCHK(hipEventRecord(ss->ev[0], q));
        if (seed) {
            HIPCHK(hipMemsetAsync(d_count, 0, 4, q));
            aln_seedjoin_launch_keys(ss->slot->seqs.as<uint8_t>(), ss->d_off.as<uint64_t>(), ss->d_len.as<uint32_t>(), ss->n, total, k, alphabet,
                                     a.as<uint64_t>(), pos_a.as<uint32_t>(), q);
        } else {
            HIPCHK(hipMemsetAsync(aux.p, 0, std::max<size_t>(4ull * ss->n, 4), q));
            aln_wordjoin_launch_keys(ss->slot->seqs.as<uint8_t>(), ss->d_off.as<uint64_t>(), ss->d_len.as<uint32_t>(), ss->n, total, k, alphabet,
                                     a.as<uint64_t>(), q);
        }
        HIPCHK(hipGetLastError());
        // the sequence's bits, then the word's.  A full word field is sorted as the whole key in one pass (what the launcher asks of a
        // range that ends at bit 64): the bits between the fields are zero in every word's key, so the order is that of the two passes
        if (word_end == 64u) st = pass(0, 64);
        else if ((st = pass(0, seq_end)) == ALN_OK) st = pass(32, word_end);
        if (st != ALN_OK) return st;
        // a is sorted: the occurrences are the keys in front of the all-ones keys; the entries are the distinct ones, compacted into b
        if (!seed) aln_wordjoin_launch_distinct(a.as<uint64_t>(), total, tile_count, tile_off, d_count, total, b.as<uint64_t>(), ss->n, aux.as<uint32_t>(), q);
        else if (total) aln_seedjoin_launch_count(a.as<uint64_t>(), total, d_count, q);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ss->ev[1], q));
        HIPCHK(hipMemcpyAsync(&got, d_count, 4, hipMemcpyDeviceToHost, q));
        if (n_words && ss->n) HIPCHK(hipMemcpyAsync(counts_h.data(), aux.p, 4ull * ss->n, hipMemcpyDeviceToHost, q));
        HIPCHK(hipStreamSynchronize(q));
        if (got > total) {
            g_err = seed ? "the seed index holds more occurrences than the set has windows" : "the word index holds more entries than the set has windows";
            return ALN_ERR_DEVICE;
        }
        // the resident list at its own size; the sort's buffers go
        if ((st = dev_ensure(keep, 8ull * got, false)) != ALN_OK) return st;
        if (seed && (st = dev_ensure(aux, 4ull * got, false)) != ALN_OK) return st;
        if (got) HIPCHK(hipMemcpy(keep.p, seed ? a.p : b.p, 8ull * got, hipMemcpyDeviceToDevice));
        if (seed && got) HIPCHK(hipMemcpy(aux.p, pos_a.p, 4ull * got, hipMemcpyDeviceToDevice));
        return ALN_OK;
    });
    for (DevBuf *d : {&a, &b, &pos_a, &pos_b, &temp}) dev_free(*d);
    if (st != ALN_OK) { dev_free(keep); dev_free(aux); return st; }
    DevBuf &list = seed ? ss->seed_key : ss->word_e, &beside = seed ? ss->seed_pos : ss->word_n;
    dev_free(list); dev_free(beside);
    list = keep; beside = aux;
    (seed ? ss->seed_k : ss->word_k) = k; (seed ? ss->seed_alphabet : ss->word_alphabet) = alphabet; (seed ? ss->seed_entries : ss->word_entries) = got;
    seqset_drop_candidates(ss);
    if (n_words && ss->n) memcpy(n_words, counts_h.data(), 4ull * ss->n);
    *entries = got;
    seqset_done(ss, t0, 0, 4 + (n_words ? 4ull * ss->n : 0));
    return ALN_OK;
}

static int seqset_word_index(aln_seqset *ss, uint32_t k, uint32_t alphabet, uint32_t *n_words)
{
    if (!ss) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    const uint64_t words = aln_wordjoin_words(k, alphabet);
    if (!words) { g_err = WORDJOIN_RANGE; return ALN_ERR_INVALID_ARGUMENT; }
    if (ss->total > 0x7FFFFFFFull) { g_err = "a word index holds fewer than 2^31 residue positions"; return ALN_ERR_UNSUPPORTED; }
    uint32_t entries;
    return seqset_posting_index(ss, k, alphabet, words, false, n_words, &entries);
}

static int seqset_seed_index(aln_seqset *ss, uint32_t k, uint32_t alphabet, uint64_t *occurrences)
{
    if (!ss) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    const uint64_t words = aln_seedjoin_words(k, alphabet);
    if (!words) { g_err = SEEDJOIN_RANGE; return ALN_ERR_INVALID_ARGUMENT; }
    if (ss->total > 0x7FFFFFFFull) { g_err = "a seed index holds fewer than 2^31 residue positions"; return ALN_ERR_UNSUPPORTED; }
    uint32_t entries;
    const int st = seqset_posting_index(ss, k, alphabet, words, true, nullptr, &entries);
    if (st == ALN_OK && occurrences) *occurrences = entries;
    return st;
}

// ---- both joins over an index of n keys.  A Route names the index, its block of the set's counter words (misc: a chunk zeroes and
// reads WORDS of them; the plan's PLAN_WORDS lie behind those and come down into plan_h) and its messages, and adds:
//   plan(q)                      the plan launch into wj_first / wj_len / wj_occ
//   cut(per_row, first)          the rows of the chunk that starts at row `first`; 0: that row alone is above the cap (OVER)
//   ensure(k)                    the chunk's buffers beside wj_a / wj_b / wj_temp
//   queue(q, k, tiles, out_k)    expand -> sort -> append, between the chunk's two events
//   sound(h, k)                  what else must hold of the chunk's counter words h
//   take(h, k, at, got, down)    what comes down per kept pair beside the 12 bytes of seqset_cand_append
struct JoinChunk { uint64_t m, q_lo, q_rows, k_lo, k_end, room; };      // m occurrences; the rows; their pairs; the most it can keep

template <class Route> static int seqset_join(aln_seqset *ss, const aln_seqset_block *b, Route &r, uint64_t *chunks, uint64_t *count)
{
    HIPCHK(hipSetDevice(ss->ctx->device));
    hipStream_t q = ss->slot->stream;
    HIPCHK(hipStreamSynchronize(q));
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t rows = b->q_count;
    uint64_t total = 0, down = 0;
    double kernels = 0;
    int st;
    // ---- the plan: nothing of the set's state is touched before the rows are cut
    std::vector<uint64_t> per_row(rows, 0), chunk_first, chunk_rows, chunk_sum;
    st = run_queued(q, [&]() -> int {
        if ((st = dev_ensure(ss->wj_first, 4 * r.n, false)) != ALN_OK) return st;
        if ((st = dev_ensure(ss->wj_len, 4 * r.n, false)) != ALN_OK) return st;
        if ((st = dev_ensure(ss->wj_off, 4 * r.n, false)) != ALN_OK) return st;
        if ((st = dev_ensure(ss->wj_occ, 8 * rows, false)) != ALN_OK) return st;
        HIPCHK(hipEventRecord(ss->ev[0], q));
        HIPCHK(hipMemsetAsync(ss->wj_occ.p, 0, 8 * rows, q));
        if ((st = r.plan(q)) != ALN_OK) return st;
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ss->ev[1], q));
        HIPCHK(hipMemcpyAsync(per_row.data(), ss->wj_occ.p, 8 * rows, hipMemcpyDeviceToHost, q));
        if constexpr (Route::PLAN_WORDS != 0) HIPCHK(hipMemcpyAsync(r.plan_h, r.misc + Route::WORDS, 4 * Route::PLAN_WORDS, hipMemcpyDeviceToHost, q));
        HIPCHK(hipStreamSynchronize(q));
        kernels += ev_ms(ss->ev[0], ss->ev[1]);
        down += 8 * rows + 4 * Route::PLAN_WORDS;
        return seqset_cut_rows(per_row, [&](uint64_t first) { return r.cut(per_row.data(), first); }, Route::OVER, chunk_first, chunk_rows, chunk_sum);
    });
    if (st != ALN_OK) return st;
    seqset_drop_candidates(ss);
    st = run_queued(q, [&]() -> int {
        if ((st = seqset_cand_room(ss, 0, 1)) != ALN_OK) return st;      // (an empty list is resident too, as the prefilter's is)
        for (size_t c = 0; c < chunk_first.size(); ++c) {
            // the chunk's pairs: the pair numbers of its rows
            const uint64_t first = chunk_first[c], end = first + chunk_rows[c];
            const uint64_t k_lo = b->upper ? aln_seqset_row_start(rows, first) : first * b->t_count;
            const uint64_t k_end = b->upper ? aln_seqset_row_start(rows, end) : end * b->t_count;
            const JoinChunk k = {chunk_sum[c], b->q_first + first, chunk_rows[c], k_lo, k_end, std::min(chunk_sum[c], k_end - k_lo)};
            size_t temp_bytes = 0;
            HIPCHK((hipError_t)aln_wordjoin_sort_temp_bytes(k.m, &temp_bytes));
            uint32_t *tile_count = nullptr, *tile_off = nullptr;
            if ((st = dev_ensure(ss->wj_a, 8 * k.m, false)) != ALN_OK) return st;
            if ((st = dev_ensure(ss->wj_b, 8 * k.m, false)) != ALN_OK) return st;
            if ((st = dev_ensure(ss->wj_temp, temp_bytes, false)) != ALN_OK) return st;
            if ((st = r.ensure(k)) != ALN_OK) return st;
            if ((st = tiles_ensure(ss->tiles, std::max(aln_seqset_tiles(r.n), aln_seqset_tiles(k.m)), &tile_count, &tile_off)) != ALN_OK) return st;
            if ((st = seqset_cand_room(ss, total, total + k.room)) != ALN_OK) return st;
            HIPCHK(hipEventRecord(ss->ev[0], q));
            HIPCHK(hipMemsetAsync(r.misc, 0, 4 * Route::WORDS, q));
            aln_wordjoin_launch_offsets(r.keys, ss->wj_len.as<uint32_t>(), r.n, k.q_lo, k.q_rows, tile_count, tile_off, r.misc + ALN_JOIN_MISC_SCANNED,
                                        ss->wj_off.as<uint32_t>(), q);
            HIPCHK(hipGetLastError());
            if ((st = r.queue(q, k, tile_count, tile_off, ss->cand_k.as<uint64_t>() + total)) != ALN_OK) return st;
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(ss->ev[1], q));
            uint32_t h[Route::WORDS] = {};
            HIPCHK(hipMemcpyAsync(h, r.misc, 4 * Route::WORDS, hipMemcpyDeviceToHost, q));
            HIPCHK(hipStreamSynchronize(q));
            kernels += ev_ms(ss->ev[0], ss->ev[1]);
            down += 4 * Route::WORDS;
            const uint64_t got = h[ALN_JOIN_MISC_KEPT];
            if (h[ALN_JOIN_MISC_SCANNED] != k.m) { g_err = Route::SCANNED; return ALN_ERR_DEVICE; }
            if (h[ALN_JOIN_MISC_NO_PAIR]) { g_err = Route::NO_PAIR; return ALN_ERR_DEVICE; }
            const char *const more = "the join kept more pairs than the chunk's rows hold";
            if (!r.sound(h, k)) { g_err = more; return ALN_ERR_DEVICE; }
            if ((st = seqset_cand_append(ss, total, got, k.room, more, k.k_lo, k.k_end, &down)) != ALN_OK) return st;
            if ((st = r.take(h, k, total, got, &down)) != ALN_OK) return st;
            total += got;
        }
        return ALN_OK;
    });
    if (st != ALN_OK) { seqset_drop_candidates(ss); return st; }
    seqset_cand_finish(ss, b, total, count);
    *chunks = chunk_first.size();
    seqset_done(ss, t0, 0, down, kernels);
    return ALN_OK;
}

// bytes down: 8 per query row, 12 per chunk and 12 per candidate
struct WordJoinRoute {
    aln_seqset *ss;
    const aln_wordjoin_spec *sp;
    const aln_seqset_block *b;
    uint64_t pairs, cap, n = ss->word_entries;
    const uint64_t *keys = ss->word_e.as<uint64_t>();
    uint32_t *misc = ss->misc.as<uint32_t>() + ALN_SEQSET_MISC_WORD;
    static constexpr uint32_t WORDS = ALN_SEQSET_MISC_WORD_WORDS, PLAN_WORDS = 0;
    static constexpr const char *OVER = "one query row of the block has more occurrences than chunk_occurrences allows";
    static constexpr const char *SCANNED = "a chunk's occurrences differ from the plan's", *NO_PAIR = "an occurrence of the join names no pair of the block";
    int plan(hipStream_t q)
    {
        aln_wordjoin_launch_plan(keys, n, b, ss->wj_first.as<uint32_t>(), ss->wj_len.as<uint32_t>(), ss->wj_occ.as<uint64_t>(), q);
        return ALN_OK;
    }
    uint64_t cut(const uint64_t *occ, uint64_t first) const { return aln_wordjoin_cut(occ, b->q_count, first, cap); }
    int ensure(const JoinChunk &k)
    {
        int st;
        if ((st = dev_ensure(ss->pf_shared, 4 * k.m, false)) != ALN_OK || (st = dev_ensure(ss->pf_keep, k.m, false)) != ALN_OK) return st;
        return dev_ensure(ss->pf_out, 4 * k.room, false);
    }
    int queue(hipStream_t q, const JoinChunk &k, uint32_t *tile_count, uint32_t *tile_off, uint64_t *out_k)
    {
        aln_wordjoin_launch_expand(keys, ss->wj_first.as<uint32_t>(), ss->wj_len.as<uint32_t>(), ss->wj_off.as<uint32_t>(), n, k.m, b, pairs, k.q_lo,
                                   k.q_rows, ss->wj_a.as<uint64_t>(), misc + ALN_JOIN_MISC_NO_PAIR, q);
        HIPCHK(hipGetLastError());
        const uint32_t pair_bits = std::max<uint32_t>(aln_wordjoin_bits_needed(pairs), 1u);
        HIPCHK((hipError_t)aln_wordjoin_launch_sort(ss->wj_temp.p, ss->wj_temp.cap, ss->wj_a.as<uint64_t>(), ss->wj_b.as<uint64_t>(), k.m, 0, pair_bits, q));
        aln_wordjoin_launch_append(ss->wj_b.as<uint64_t>(), k.m, b, pairs, ss->word_n.as<uint32_t>(), ss->n, sp->min_shared, sp->min_per_1024,
                                   ss->pf_shared.as<uint32_t>(), ss->pf_keep.as<uint8_t>(), tile_count, tile_off, misc + ALN_JOIN_MISC_KEPT, k.room, out_k,
                                   ss->pf_out.as<uint32_t>(), q);
        return ALN_OK;
    }
    bool sound(const uint32_t *, const JoinChunk &) const { return true; }
    int take(const uint32_t *, const JoinChunk &, uint64_t, uint64_t, uint64_t *) { return ALN_OK; }
};

static int seqset_word_join(aln_seqset *ss, const aln_wordjoin_spec *sp, const aln_seqset_block *b, uint64_t *count)
{
    if (!ss || !sp || !b || !count) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (!aln_wordjoin_words(sp->k, sp->alphabet)) { g_err = WORDJOIN_RANGE; return ALN_ERR_INVALID_ARGUMENT; }
    if (!ss->word_k || sp->k != ss->word_k || sp->alphabet != ss->word_alphabet) { g_err = "no word index of this k and alphabet: aln_seqset_word_index builds it"; return ALN_ERR_INVALID_ARGUMENT; }
    if (sp->min_shared == 0u) { g_err = "min_shared must be at least 1: a join sees only the pairs that share a word"; return ALN_ERR_INVALID_ARGUMENT; }
    if (sp->min_per_1024 > ALN_PREFILTER_MAX_PER_1024) { g_err = "min_per_1024 must lie in 0 .. 1024"; return ALN_ERR_INVALID_ARGUMENT; }
    if (sp->flags != 0u || sp->reserved != 0u) { g_err = CAND_SPEC_WORDS; return ALN_ERR_INVALID_ARGUMENT; }
    if (sp->chunk_occurrences > ALN_WORDJOIN_MAX_CHUNK_OCCURRENCES) { g_err = "chunk_occurrences must lie in 0 .. 2^26"; return ALN_ERR_INVALID_ARGUMENT; }
    const uint64_t pairs = aln_seqset_block_pairs(ss->n, *b);
    if (pairs == 0) { g_err = CAND_BLOCK; return ALN_ERR_INVALID_ARGUMENT; }
    WordJoinRoute r{ss, sp, b, pairs, sp->chunk_occurrences ? sp->chunk_occurrences : ALN_WORDJOIN_CHUNK_OCCURRENCES};
    uint64_t chunks;
    return seqset_join(ss, b, r, &chunks, count);
}

// bytes down: 8 per query row and 4, 16 per chunk and 16 per candidate
struct SeedJoinRoute {
    aln_seqset *ss;
    const aln_seedjoin_spec *sp;
    const aln_seqset_block *b;
    uint64_t cap, n = ss->seed_entries;
    const uint64_t *keys = ss->seed_key.as<uint64_t>();
    uint32_t *misc = ss->misc.as<uint32_t>() + ALN_SEQSET_MISC_SEED;
    uint32_t plan_h[1] = {0};                          // the words max_occ dropped
    uint64_t seeds_all = 0, pairs_seen = 0;
    static constexpr uint32_t WORDS = ALN_SEQSET_MISC_SEED_WORDS - 1u, PLAN_WORDS = 1;
    static constexpr const char *OVER = "one query row of the block has more seeds than chunk_seeds allows: max_occ drops the words that occur too often";
    static constexpr const char *SCANNED = "a chunk's seeds differ from the plan's", *NO_PAIR = "a seed of the join names no pair of the block";
    int plan(hipStream_t q)
    {
        HIPCHK(hipMemsetAsync(misc, 0, 4 * ALN_SEQSET_MISC_SEED_WORDS, q));
        aln_seedjoin_launch_plan(keys, n, b, sp->max_occ, ss->wj_first.as<uint32_t>(), ss->wj_len.as<uint32_t>(), ss->wj_occ.as<uint64_t>(),
                                 misc + ALN_JOIN_MISC_DROPPED, q);
        return ALN_OK;
    }
    uint64_t cut(const uint64_t *seeds, uint64_t first) const { return aln_seedjoin_cut(seeds, *b, first, cap); }
    int ensure(const JoinChunk &k)
    {
        const int st = dev_ensure(ss->pf_out, 4 * k.room, false);
        return st != ALN_OK ? st : dev_ensure(ss->sj_diag, 4 * k.room, false);
    }
    int queue(hipStream_t q, const JoinChunk &k, uint32_t *tile_count, uint32_t *tile_off, uint64_t *out_k)
    {
        // the chunk's pairs are at most 2^32 (aln_seedjoin_cut): their number in the chunk fits the key's high half
        aln_seedjoin_launch_expand(keys, ss->seed_pos.as<uint32_t>(), ss->wj_first.as<uint32_t>(), ss->wj_len.as<uint32_t>(), ss->wj_off.as<uint32_t>(), n,
                                   k.m, b, k.k_lo, k.k_end, k.q_lo, k.q_rows, ss->wj_a.as<uint64_t>(), misc + ALN_JOIN_MISC_NO_PAIR, q);
        HIPCHK(hipGetLastError());
        const uint32_t key_bits = 32u + std::max<uint32_t>(aln_wordjoin_bits_needed(k.k_end - k.k_lo), 1u);
        HIPCHK((hipError_t)aln_wordjoin_launch_sort(ss->wj_temp.p, ss->wj_temp.cap, ss->wj_a.as<uint64_t>(), ss->wj_b.as<uint64_t>(), k.m, 0, key_bits, q));
        // the unsorted keys have been read: their buffer holds the pairs' slots now
        HIPCHK(hipMemsetAsync(ss->wj_a.p, 0, 8 * k.m, q));
        aln_seedjoin_launch_append(ss->wj_b.as<uint64_t>(), k.m, k.k_lo, k.k_end - k.k_lo, sp->band, sp->min_seeds, ss->wj_a.as<uint64_t>(),
                                   misc + ALN_JOIN_MISC_NO_PAIR, tile_count, tile_off, misc + ALN_JOIN_MISC_PAIRS_SEEN, misc + ALN_JOIN_MISC_KEPT, k.room,
                                   out_k, ss->pf_out.as<uint32_t>(), ss->sj_diag.as<int32_t>(), q);
        return ALN_OK;
    }
    bool sound(const uint32_t *h, const JoinChunk &k) const { return h[ALN_JOIN_MISC_KEPT] <= h[ALN_JOIN_MISC_PAIRS_SEEN] && h[ALN_JOIN_MISC_PAIRS_SEEN] <= k.room; }
    int take(const uint32_t *h, const JoinChunk &k, uint64_t at, uint64_t got, uint64_t *down)      // the diagonals beside the list
    {
        if (got) {
            ss->cands.diag.resize(at + got);
            HIPCHK(hipMemcpy(ss->cands.diag.data() + at, ss->sj_diag.p, 4ull * got, hipMemcpyDeviceToHost));
        }
        *down += 4ull * got;
        seeds_all += k.m;
        pairs_seen += h[ALN_JOIN_MISC_PAIRS_SEEN];
        return ALN_OK;
    }
};

static int seqset_seed_join(aln_seqset *ss, const aln_seedjoin_spec *sp, const aln_seqset_block *b, aln_seedjoin_summary *summary, uint64_t *count)
{
    if (!ss || !sp || !b || !count) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (!aln_seedjoin_words(sp->k, sp->alphabet)) { g_err = SEEDJOIN_RANGE; return ALN_ERR_INVALID_ARGUMENT; }
    if (!ss->seed_k || sp->k != ss->seed_k || sp->alphabet != ss->seed_alphabet) { g_err = "no seed index of this k and alphabet: aln_seqset_seed_index builds it"; return ALN_ERR_INVALID_ARGUMENT; }
    if (sp->min_seeds == 0u) { g_err = "min_seeds must be at least 1: a join sees only the pairs that have a seed"; return ALN_ERR_INVALID_ARGUMENT; }
    if (sp->band > ALN_SEEDJOIN_MAX_BAND) { g_err = "band must lie in 0 .. 2^31 - 1"; return ALN_ERR_INVALID_ARGUMENT; }
    if (sp->flags != 0u || sp->reserved != 0u) { g_err = CAND_SPEC_WORDS; return ALN_ERR_INVALID_ARGUMENT; }
    if (sp->chunk_seeds > ALN_SEEDJOIN_MAX_CHUNK_SEEDS) { g_err = "chunk_seeds must lie in 0 .. 2^26"; return ALN_ERR_INVALID_ARGUMENT; }
    if (aln_seqset_block_pairs(ss->n, *b) == 0) { g_err = CAND_BLOCK; return ALN_ERR_INVALID_ARGUMENT; }
    SeedJoinRoute r{ss, sp, b, sp->chunk_seeds ? sp->chunk_seeds : ALN_SEEDJOIN_CHUNK_SEEDS};
    uint64_t chunks;
    const int st = seqset_join(ss, b, r, &chunks, count);
    if (st != ALN_OK) return st;
    ss->cands.has_diag = true;
    if (summary) { summary->seeds = r.seeds_all; summary->pairs_with_seed = r.pairs_seen; summary->words_dropped = r.plan_h[0]; summary->chunks = chunks; }
    return ALN_OK;
}

extern "C" int aln_seqset_word_index(aln_seqset *ss, uint32_t k, uint32_t alphabet, uint32_t *n_words)
{
    ALN_GUARDED(seqset_live(ss), seqset_word_index(ss, k, alphabet, n_words))
}

extern "C" int aln_seqset_word_join(aln_seqset *ss, const aln_wordjoin_spec *spec, const aln_seqset_block *b, uint64_t *count)
{
    ALN_GUARDED(seqset_live(ss), seqset_word_join(ss, spec, b, count))
}

extern "C" int aln_seqset_seed_index(aln_seqset *ss, uint32_t k, uint32_t alphabet, uint64_t *occurrences)
{
    ALN_GUARDED(seqset_live(ss), seqset_seed_index(ss, k, alphabet, occurrences))
}

extern "C" int aln_seqset_seed_join(aln_seqset *ss, const aln_seedjoin_spec *spec, const aln_seqset_block *b, aln_seedjoin_summary *summary,
                                    uint64_t *count)
{
    ALN_GUARDED(seqset_live(ss), seqset_seed_join(ss, spec, b, summary, count))
}

extern "C" int aln_seqset_candidate_diags(aln_seqset *ss, uint64_t first, uint64_t n, int32_t *diag)
{
    const int st = seqset_cand_check(ss);
    if (st != ALN_OK) return st;
    if (!ss->cands.has_diag) { g_err = "the candidate list has no diagonals: aln_seqset_seed_join makes the lists that have"; return ALN_ERR_INVALID_ARGUMENT; }
    const uint64_t have = ss->cands.diag.size();
    if (first > have || n > have - first) { g_err = "range beyond the candidate list"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n && !diag) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    for (uint64_t i = 0; i < n; ++i) diag[i] = ss->cands.diag[first + i];
    return ALN_OK;                       // (no byte moves and no kernel runs: the stats stay as they are)
}

// ---------------------------------------------------------------- seed chains (include/aligner_hip_seedchain.h)
// The colinear chain over ALL seeds of every listed candidate, from the seed index alone: count the anchors per candidate, cut the
// list into runs of whole candidates of at most chunk_anchors, expand and chain run by run.  The records of a call lie in ch_rec; a
// filter compacts the list by them into a new pair-number buffer and a new record buffer and changes places only when all is there.
static const char *const SEEDCHAIN_REFUSALS[] = {
    "", "max_gap must lie in 1 .. 2^31 - 1", "max_skew must lie in 0 .. 2^31 - 1", "gap_scale must lie in 0 .. 255",
    "max_pair_seeds must lie in 0 .. 2^20", "chunk_anchors must lie in 0 .. 2^26", "the spec's flags and reserved words must be 0",
    "max_pair_seeds (0: 2^16) may not exceed chunk_anchors (0: 2^24): a pair that is chained must fit one chunk"};
#define ALN_SEEDCHAIN_CHUNK_CANDIDATES (1ull << 22)      // per run: what one launch takes a block each of

static int seqset_chain_check(aln_seqset *ss, const aln_seedchain_spec *sp)
{
    if (!aln_seedjoin_words(sp->k, sp->alphabet)) { g_err = SEEDJOIN_RANGE; return ALN_ERR_INVALID_ARGUMENT; }
    if (!ss->seed_k || sp->k != ss->seed_k || sp->alphabet != ss->seed_alphabet) { g_err = "no seed index of this k and alphabet: aln_seqset_seed_index builds it"; return ALN_ERR_INVALID_ARGUMENT; }
    const uint32_t why = aln_seedchain_spec_refusal(*sp);
    if (why) { g_err = SEEDCHAIN_REFUSALS[why]; return ALN_ERR_INVALID_ARGUMENT; }
    return seqset_cand_check(ss);
}

struct ChainRun {
    aln_seedchain_summary sum = {0, 0, 0, 0};
    uint64_t up = 0, down = 0;
    double kernels = 0;
};

// the chain records of entries first .. first + n - 1 of the list into ss->ch_rec (n >= 1; the stream is idle before and after).
// Nothing of the set's state but the ch_* tables is touched
static int seqset_chain_run(aln_seqset *ss, const aln_seedchain_spec *sp, uint64_t first, uint64_t n, ChainRun *run)
{
    hipStream_t q = ss->slot->stream;
    uint32_t *misc = ss->misc.as<uint32_t>() + ALN_SEQSET_MISC_CHAIN;
    const uint64_t cap = aln_seedchain_chunk_anchors(*sp);
    const aln_seedchain_index x = {ss->slot->seqs.as<uint8_t>(), ss->d_off.as<uint64_t>(), ss->d_len.as<uint32_t>(), ss->n, ss->total,
                                   ss->seed_key.as<uint64_t>(), ss->seed_pos.as<uint32_t>(), ss->seed_entries};
    std::vector<uint32_t> seeds_h(n), chained_h(n);
    std::vector<uint64_t> per(n), run_first, run_count, run_base, run_sum;
    return run_queued(q, [&]() -> int {
        int st;
        for (DevBuf *d : {&ss->ch_q, &ss->ch_t, &ss->ch_seeds, &ss->ch_chained})
            if ((st = dev_ensure(*d, 4 * n, false)) != ALN_OK) return st;
        if ((st = dev_ensure(ss->ch_off, 8 * n, false)) != ALN_OK) return st;
        if ((st = dev_ensure(ss->ch_rec, sizeof(aln_chain_record) * n, false)) != ALN_OK) return st;
        HIPCHK(hipMemcpyAsync(ss->ch_q.p, ss->cands.qs.data() + first, 4 * n, hipMemcpyHostToDevice, q));
        HIPCHK(hipMemcpyAsync(ss->ch_t.p, ss->cands.ts.data() + first, 4 * n, hipMemcpyHostToDevice, q));
        run->up += 8 * n;
        HIPCHK(hipEventRecord(ss->ev[0], q));
        HIPCHK(hipMemsetAsync(misc, 0, 4 * ALN_SEQSET_MISC_CHAIN_WORDS, q));
        aln_seedchain_launch_count(&x, sp, ss->ch_q.as<uint32_t>(), ss->ch_t.as<uint32_t>(), n, ss->ch_seeds.as<uint32_t>(), ss->ch_chained.as<uint32_t>(),
                                   ss->ch_off.as<uint64_t>(), reinterpret_cast<uint64_t *>(misc + ALN_CHAIN_MISC_TOTAL), ss->ch_rec.as<aln_chain_record>(),
                                   misc + ALN_CHAIN_MISC_ERRORS, q);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ss->ev[1], q));
        uint32_t h[ALN_SEQSET_MISC_CHAIN_WORDS] = {};
        HIPCHK(hipMemcpyAsync(seeds_h.data(), ss->ch_seeds.p, 4 * n, hipMemcpyDeviceToHost, q));
        HIPCHK(hipMemcpyAsync(chained_h.data(), ss->ch_chained.p, 4 * n, hipMemcpyDeviceToHost, q));
        HIPCHK(hipMemcpyAsync(h, misc, sizeof h, hipMemcpyDeviceToHost, q));
        HIPCHK(hipStreamSynchronize(q));
        run->kernels += ev_ms(ss->ev[0], ss->ev[1]);
        run->down += 8 * n + sizeof h;
        if (h[ALN_CHAIN_MISC_ERRORS]) { g_err = "a listed candidate names no record of the set"; return ALN_ERR_DEVICE; }
        const uint32_t pair_cap = aln_seedchain_pair_seeds(*sp);
        uint64_t total = 0;
        for (uint64_t c = 0; c < n; ++c) {
            if (chained_h[c] != aln_seedchain_chained(seeds_h[c], pair_cap)) { g_err = "a candidate chains other anchors than the rule gives it"; return ALN_ERR_DEVICE; }
            per[c] = chained_h[c];
            total += per[c];
            run->sum.with_anchor += seeds_h[c] != 0u;
            run->sum.overflowed += seeds_h[c] > pair_cap;
        }
        if (total != ((uint64_t)h[ALN_CHAIN_MISC_TOTAL + 1] << 32 | h[ALN_CHAIN_MISC_TOTAL])) { g_err = "the anchors' offsets differ from their counts"; return ALN_ERR_DEVICE; }
        // the runs of whole candidates: decided before anything is expanded
        uint64_t most = 0, base = 0;
        for (uint64_t c = 0; c < n;) {
            uint64_t m = aln_wordjoin_cut(per.data(), n, c, cap), sum = 0;
            if (!m) { g_err = "one candidate has more anchors than chunk_anchors allows"; return ALN_ERR_CAPACITY; }
            m = std::min<uint64_t>(m, ALN_SEEDCHAIN_CHUNK_CANDIDATES);
            for (uint64_t r = c; r < c + m; ++r) sum += per[r];
            if (sum) { run_first.push_back(c); run_count.push_back(m); run_base.push_back(base); run_sum.push_back(sum); most = std::max(most, sum); }
            base += sum;
            c += m;
        }
        if (!most) return ALN_OK;
        if ((st = dev_ensure(ss->ch_anchor, 8 * most, false)) != ALN_OK) return st;
        if ((st = dev_ensure(ss->ch_state, sizeof(aln_seedchain_state) * most, false)) != ALN_OK) return st;
        HIPCHK(hipEventRecord(ss->ev[0], q));
        for (size_t r = 0; r < run_first.size(); ++r) {
            aln_seedchain_launch_chunk(&x, sp, ss->ch_q.as<uint32_t>(), ss->ch_t.as<uint32_t>(), run_first[r], run_count[r], ss->ch_seeds.as<uint32_t>(),
                                       ss->ch_chained.as<uint32_t>(), ss->ch_off.as<uint64_t>(), run_base[r], run_sum[r], ss->ch_anchor.as<uint64_t>(),
                                       ss->ch_state.p, ss->ch_rec.as<aln_chain_record>(), misc + ALN_CHAIN_MISC_ERRORS, q);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(ss->ev[1], q));
        HIPCHK(hipMemcpyAsync(h, misc, 4, hipMemcpyDeviceToHost, q));
        HIPCHK(hipStreamSynchronize(q));
        run->kernels += ev_ms(ss->ev[0], ss->ev[1]);
        run->down += 4;
        if (h[ALN_CHAIN_MISC_ERRORS]) { g_err = "the anchors of a candidate differ from their count, or do not ascend"; return ALN_ERR_DEVICE; }
        run->sum.anchors = total;
        run->sum.chunks = run_first.size();
        return ALN_OK;
    });
}

static int seqset_candidate_chains(aln_seqset *ss, const aln_seedchain_spec *sp, uint64_t first, uint64_t n, aln_chain_record *records,
                                   aln_seedchain_summary *summary)
{
    if (!ss || !sp) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    int st = seqset_chain_check(ss, sp);
    if (st != ALN_OK) return st;
    const uint64_t have = ss->cands.pair.size();
    if (first > have || n > have - first) { g_err = "range beyond the candidate list"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n && !records) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    HIPCHK(hipSetDevice(ss->ctx->device));
    hipStream_t q = ss->slot->stream;
    HIPCHK(hipStreamSynchronize(q));
    const auto t0 = std::chrono::steady_clock::now();
    ChainRun run;
    if (n) {
        if ((st = seqset_chain_run(ss, sp, first, n, &run)) != ALN_OK) return st;
        HIPCHK(hipMemcpy(records, ss->ch_rec.p, sizeof(aln_chain_record) * n, hipMemcpyDeviceToHost));
        run.down += sizeof(aln_chain_record) * n;
    }
    if (summary) *summary = run.sum;
    seqset_done(ss, t0, run.up, run.down, run.kernels);
    return ALN_OK;
}

// a device buffer that goes with its scope: what a filter allocates before it knows that everything else can be had
struct ScopedDev {
    DevBuf b;
    ~ScopedDev() { dev_free(b); }
};

static int seqset_candidate_chain_filter(aln_seqset *ss, const aln_seedchain_spec *sp, int32_t min_score, uint32_t min_span,
                                         aln_seedchain_summary *summary, uint64_t *count)
{
    if (!ss || !sp || !count) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    int st = seqset_chain_check(ss, sp);
    if (st != ALN_OK) return st;
    HIPCHK(hipSetDevice(ss->ctx->device));
    hipStream_t q = ss->slot->stream;
    HIPCHK(hipStreamSynchronize(q));
    const auto t0 = std::chrono::steady_clock::now();
    const uint64_t n = ss->cands.pair.size();
    ChainRun run;
    ScopedDev new_k, new_rec;                          // everything new first: a failure leaves the list as it was
    CandList kept;
    uint32_t got = 0;
    if ((st = dev_ensure(new_k.b, 8 * std::max<uint64_t>(n, 1), false)) != ALN_OK) return st;
    if ((st = dev_ensure(new_rec.b, sizeof(aln_chain_record) * std::max<uint64_t>(n, 1), false)) != ALN_OK) return st;
    if (n) {
        if ((st = seqset_chain_run(ss, sp, 0, n, &run)) != ALN_OK) return st;
        std::vector<uint32_t> pos;
        st = run_queued(q, [&]() -> int {
            int st;
            uint32_t *tile_count = nullptr, *tile_off = nullptr, *d_count = ss->misc.as<uint32_t>() + ALN_SEQSET_MISC_CHAIN + ALN_CHAIN_MISC_KEPT;
            if ((st = dev_ensure(ss->ch_pos, 4 * n, false)) != ALN_OK) return st;
            if ((st = tiles_ensure(ss->tiles, aln_seqset_tiles(n), &tile_count, &tile_off)) != ALN_OK) return st;
            HIPCHK(hipEventRecord(ss->ev[0], q));
            aln_seedchain_launch_filter(ss->ch_rec.as<aln_chain_record>(), ss->cand_k.as<uint64_t>(), n, min_score, min_span, tile_count, tile_off, d_count, n,
                                        ss->ch_pos.as<uint32_t>(), new_k.b.as<uint64_t>(), new_rec.b.as<aln_chain_record>(), q);
            HIPCHK(hipGetLastError());
            HIPCHK(hipEventRecord(ss->ev[1], q));
            HIPCHK(hipMemcpyAsync(&got, d_count, 4, hipMemcpyDeviceToHost, q));
            HIPCHK(hipStreamSynchronize(q));
            run.kernels += ev_ms(ss->ev[0], ss->ev[1]);
            if (got > n) { g_err = "the filter kept more entries than the list holds"; return ALN_ERR_DEVICE; }
            pos.resize(got);
            if (got) HIPCHK(hipMemcpy(pos.data(), ss->ch_pos.p, 4ull * got, hipMemcpyDeviceToHost));
            run.down += 4 + 4ull * got;
            return ALN_OK;
        });
        if (st != ALN_OK) return st;
        // the kept entries of the host's copy, by their places: ascending places of the list
        kept.pair.resize(got); kept.qs.resize(got); kept.ts.resize(got); kept.shared.resize(got);
        if (ss->cands.has_diag) kept.diag.resize(got);
        for (uint64_t o = 0; o < got; ++o) {
            const uint64_t c = pos[o];
            if (c >= n || (o && c <= pos[o - 1])) { g_err = "the kept places are not an ascending list of the list's places"; return ALN_ERR_DEVICE; }
            kept.pair[o] = ss->cands.pair[c]; kept.qs[o] = ss->cands.qs[c]; kept.ts[o] = ss->cands.ts[c]; kept.shared[o] = ss->cands.shared[c];
            if (ss->cands.has_diag) kept.diag[o] = ss->cands.diag[c];
        }
    }
    // all is there: the list, the resident pair numbers and the resident records change places
    ss->cands.pair.swap(kept.pair); ss->cands.qs.swap(kept.qs); ss->cands.ts.swap(kept.ts); ss->cands.shared.swap(kept.shared); ss->cands.diag.swap(kept.diag);
    ss->cands.has_chain = true;
    std::swap(ss->cand_k, new_k.b);
    std::swap(ss->chain_rec, new_rec.b);
    if (summary) *summary = run.sum;
    *count = got;
    seqset_done(ss, t0, run.up, run.down, run.kernels);
    return ALN_OK;
}

static int seqset_candidate_chain_records(aln_seqset *ss, uint64_t first, uint64_t n, aln_chain_record *records)
{
    const int st = seqset_cand_check(ss);
    if (st != ALN_OK) return st;
    if (!ss->cands.has_chain) { g_err = "the candidate list holds no chain records: aln_seqset_candidate_chain_filter makes the lists that do"; return ALN_ERR_INVALID_ARGUMENT; }
    const uint64_t have = ss->cands.pair.size();
    if (first > have || n > have - first) { g_err = "range beyond the candidate list"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n && !records) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (!n) return ALN_OK;
    HIPCHK(hipSetDevice(ss->ctx->device));
    HIPCHK(hipStreamSynchronize(ss->slot->stream));
    HIPCHK(hipMemcpy(records, ss->chain_rec.as<aln_chain_record>() + first, sizeof(aln_chain_record) * n, hipMemcpyDeviceToHost));
    return ALN_OK;                       // (no kernel runs: the stats stay the filter's, as aln_seqset_candidates leaves them the join's)
}

extern "C" int aln_seqset_candidate_chains(aln_seqset *ss, const aln_seedchain_spec *spec, uint64_t first, uint64_t n, aln_chain_record *records,
                                           aln_seedchain_summary *summary)
{
    ALN_GUARDED(seqset_live(ss), seqset_candidate_chains(ss, spec, first, n, records, summary))
}

extern "C" int aln_seqset_candidate_chain_filter(aln_seqset *ss, const aln_seedchain_spec *spec, int32_t min_score, uint32_t min_span,
                                                 aln_seedchain_summary *summary, uint64_t *count)
{
    ALN_GUARDED(seqset_live(ss), seqset_candidate_chain_filter(ss, spec, min_score, min_span, summary, count))
}

extern "C" int aln_seqset_candidate_chain_records(aln_seqset *ss, uint64_t first, uint64_t n, aln_chain_record *records)
{
    ALN_GUARDED(seqset_live(ss), seqset_candidate_chain_records(ss, first, n, records))
}

static int seqset_held_check(aln_seqset *ss)
{
    if (!ss) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (!ss->held) { g_err = "no held hits: aln_seqset_hits has not run, or another pass has replaced them"; return ALN_ERR_INVALID_ARGUMENT; }
    return ALN_OK;
}

// A list of held positions: no longer than the caller's own limit, every entry a held hit.  `each` sees every position once it is known
// to be one, in list order, so that a caller's own per-hit refusal keeps its place among these.  The length alone is a check of its
// own for the plans whose refusals that need no set come first.
static int held_length_check(uint64_t n, uint64_t limit)
{
    if (n > limit) { g_err = "list too long"; return ALN_ERR_INVALID_ARGUMENT; }
    return ALN_OK;
}
template <class Each> static int held_list_check(const uint32_t *list, uint64_t n, uint64_t held, uint64_t limit, Each &&each)
{
    int st = held_length_check(n, limit);
    for (uint64_t k = 0; k < n && st == ALN_OK; ++k) {
        if (list[k] >= held) { g_err = "a listed position is beyond the held hits"; return ALN_ERR_INVALID_ARGUMENT; }
        st = each(list[k]);
    }
    return st;
}
static int held_list_check(const uint32_t *list, uint64_t n, uint64_t held, uint64_t limit)
{
    return held_list_check(list, n, held, limit, [](uint32_t) { return (int)ALN_OK; });
}

extern "C" int aln_seqset_held_list(aln_seqset *ss, uint64_t first, uint64_t n, uint64_t *pair_index, uint32_t *q_seq, uint32_t *t_seq, double *f)
{
    int st = seqset_held_check(ss);
    if (st != ALN_OK) return st;
    const uint64_t held = ss->hit_pair.size();
    if (first > held || n > held - first) { g_err = "range beyond the held hits"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n && (!pair_index || !q_seq || !t_seq || !f)) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    // (the list is the host's: the re-fill was planned from it)
    for (uint64_t i = 0; i < n; ++i) {
        pair_index[i] = ss->hit_pair[first + i]; q_seq[i] = ss->hit_q[first + i]; t_seq[i] = ss->hit_t[first + i]; f[i] = ss->hit_score[first + i];
    }
    return ALN_OK;                       // (no byte moves and no kernel runs: the stats of the pass stay as they are)
}

static int seqset_held_strings(aln_seqset *ss, const uint32_t *keep, uint64_t n, aln_pair_result *results, uint8_t *tb_buf, const uint64_t *tb_off)
{
    int st = seqset_held_check(ss);
    if (st != ALN_OK) return st;
    if (n && (!keep || !results || (tb_buf && !tb_off))) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if ((st = held_list_check(keep, n, ss->hit_pair.size(), 0x7FFFFFF0ull)) != ALN_OK) return st;
    if (n == 0) return ALN_OK;
    HIPCHK(hipSetDevice(ss->ctx->device));
    return held_fetch_strings(ss->held_store, ss->slot->stream, ss->ev, keep, n, results, tb_buf, tb_off, *ss);
}

extern "C" int aln_seqset_held_strings(aln_seqset *ss, const uint32_t *keep, uint64_t n, aln_pair_result *results, uint8_t *tb_buf,
                                       const uint64_t *tb_off)
{
    ALN_GUARDED(seqset_live(ss), seqset_held_strings(ss, keep, n, results, tb_buf, tb_off))
}

// Significance of held hits: the listed hits as the pairs of a shuffle job (shuffle_job_plan: the planning, chunking, routing and
// launches of aln_shuffle_scores) whose residues are the set's own.  The fill kernels take one residue base per launch and the set's
// buffer must not grow or move (derived pair sets borrow it), so the job runs on a pool slot like any shuffle call and the listed
// hits' queries and originals are copied device to device into that slot's residue buffer, in front of the shuffled region -- one
// span of the set's buffer, or the ranges one by one when the hits lie far apart.  The held buffers and the set's own slot are not
// touched.  Per chunk the copies' summaries are reduced to records (aln_signif.hip) in place of the gather of aln_shuffle_scores.
static int seqset_held_significance(aln_seqset *ss, const aln_params *params, const aln_shuffle_spec *spec, const uint32_t *keep,
                                    uint64_t n_keep, aln_signif_record *records, double *f, uint32_t *lengths)
{
    int st = seqset_held_check(ss);
    if (st != ALN_OK) return st;
    if (!params || !spec || (n_keep && (!keep || !records))) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (spec->per_pair == 0 || spec->per_pair > ALN_SHUFFLE_MAX_COPIES) { g_err = "per_pair must be 1 .. 2^20"; return ALN_ERR_INVALID_ARGUMENT; }
    st = held_list_check(keep, n_keep, ss->hit_pair.size(), 0xFFFFFFF0ull, [&](uint32_t h) -> int {
        if (ss->len[ss->hit_t[h]] < spec->max_trim) { g_err = "a listed hit's target is shorter than max_trim"; return ALN_ERR_INVALID_ARGUMENT; }
        return ALN_OK;
    });
    if (st != ALN_OK) return st;
    if (params->semantics == ALN_PWM_LOCAL) { g_err = "shuffled copies are aligned with the substitution-matrix semantics only"; return ALN_ERR_UNSUPPORTED; }
    const size_t n = (size_t)n_keep;
    const uint32_t per = spec->per_pair;
    const uint64_t total = (uint64_t)n * per;
    // the listed hits as pairs: where they lie in the set's buffer, their streams (the pair number in the block of the held pass), their f
    std::vector<uint64_t> q_off(n), q_len(n), t_off(n), t_len(n), stream(n);
    std::vector<double> f_hit(n);
    for (size_t k = 0; k < n; ++k) {
        const uint32_t h = keep[k], sq = ss->hit_q[h], tq = ss->hit_t[h];
        q_off[k] = ss->off[sq]; q_len[k] = ss->len[sq]; t_off[k] = ss->off[tq]; t_len[k] = ss->len[tq];
        stream[k] = spec->pair_base + ss->hit_pair[h];
        f_hit[k] = ss->hit_score[h];
    }
    // (no table of every copy's length: the plan draws the trims per chunk, and the caller's array is written at the end, once
    // nothing can fail the call any more)
    DevCtx *dev = ss->ctx;
    ShuffleJob job;
    if ((st = shuffle_job_plan(dev, params, spec, stream.data(), nullptr, q_off.data(), q_len.data(), t_off.data(), t_len.data(), n, nullptr, job)) != ALN_OK) return st;
    if (n == 0) return ALN_OK;
    const Call &c = job.c;
    const ShuffleStage &g = job.g;
    HIPCHK(hipSetDevice(dev->device));
    HIPCHK(hipStreamSynchronize(ss->slot->stream));      // the held pass is complete; its residues are read-only from here
    const auto t0 = std::chrono::steady_clock::now();
    Slot *sl[1];
    pool_lease(dev, 1, sl);
    struct Release { DevCtx *c; Slot **s; ~Release() { pool_release(c, s, 1); } } rel{dev, sl};
    Slot &s = *sl[0];
    if ((st = shuffle_job_ensure(s, job)) != ALN_OK) return st;
    // pair table | stream table | held f | records | the f of one chunk's copies: nothing here grows with n * per_pair
    const uint64_t stream_off = align256(sizeof(ShufflePair) * n), hit_off = align256(stream_off + 8ull * n),
                   rec_off = align256(hit_off + 8ull * n), f_off = align256(rec_off + sizeof(aln_signif_record) * n);
    if ((st = dev_ensure(s.shuffle, f_off + (f ? 8 * job.copies_max : 0), s.pooled)) != ALN_OK) return st;
    uint8_t *base = s.shuffle.as<uint8_t>();
    const ShufflePair *pairs_d = s.shuffle.as<ShufflePair>();
    const uint64_t *stream_d = reinterpret_cast<const uint64_t *>(base + stream_off);
    const double *hit_d = reinterpret_cast<const double *>(base + hit_off);
    aln_signif_record *rec_d = reinterpret_cast<aln_signif_record *>(base + rec_off);
    double *f_d = f ? reinterpret_cast<double *>(base + f_off) : nullptr;
    hipStream_t q = s.stream;
    uint64_t up = 0;
    const uint8_t *set_seqs = ss->slot->seqs.as<uint8_t>();
    std::vector<aln_signif_record> rec(n);
    st = run_queued(q, [&]() -> int {
        if (g.direct) {
            if (g.bytes) HIPCHK(hipMemcpyAsync(s.seqs.p, set_seqs + g.lo, g.bytes, hipMemcpyDeviceToDevice, q));
        } else {
            for (size_t k = 0; k < n; ++k) {
                const ShufflePair &P = g.pairs[k];
                if (P.q_len) HIPCHK(hipMemcpyAsync(s.seqs.as<uint8_t>() + P.q_off, set_seqs + q_off[k], P.q_len, hipMemcpyDeviceToDevice, q));
                if (P.t_len) HIPCHK(hipMemcpyAsync(s.seqs.as<uint8_t>() + P.t_off, set_seqs + t_off[k], P.t_len, hipMemcpyDeviceToDevice, q));
            }
        }
        HIPCHK(hipMemcpyAsync(base, g.pairs.data(), sizeof(ShufflePair) * n, hipMemcpyHostToDevice, q));
        HIPCHK(hipMemcpyAsync(base + stream_off, stream.data(), 8ull * n, hipMemcpyHostToDevice, q));
        HIPCHK(hipMemcpyAsync(base + hit_off, f_hit.data(), 8ull * n, hipMemcpyHostToDevice, q));
        up += (sizeof(ShufflePair) + 16) * n;
        int e = upload_matrix(s, c, s.h_meta.as<uint8_t>(), q);
        if (e != ALN_OK) return e;
        up += c.md.size() * (c.is_int ? 4 : 8);
        HIPCHK(hipEventRecord(ss->ev[0], q));
        for (size_t j = 0; j < job.ranges.size(); ++j) {
            const size_t p0 = job.ranges[j].first, np = job.ranges[j].second;
            if ((e = shuffle_job_chunk(dev, s, job, j, spec, pairs_d, stream_d, &up)) != ALN_OK) return e;
            aln_signif_launch_reduce(s.results.as<aln_pair_result>(), hit_d + p0, (uint32_t)np, per, rec_d + p0, f_d, q);
            HIPCHK(hipGetLastError());
            // (stream order: the next chunk's reduce writes the buffer after this copy has read it)
            if (f) HIPCHK(hipMemcpyAsync(f + (uint64_t)p0 * per, f_d, 8ull * np * per, hipMemcpyDeviceToHost, q));
        }
        HIPCHK(hipEventRecord(ss->ev[1], q));
        // (the records land in a buffer of the call's own first: an error on the way leaves the caller's array as it was)
        HIPCHK(hipMemcpyAsync(rec.data(), rec_d, sizeof(aln_signif_record) * n, hipMemcpyDeviceToHost, q));
        HIPCHK(hipStreamSynchronize(q));
        return ALN_OK;
    });
    if (st != ALN_OK) return st;
    memcpy(records, rec.data(), sizeof(aln_signif_record) * n);
    if (lengths)
        for (size_t k = 0; k < n; ++k)
            for (uint32_t c = 0; c < per; ++c)
                lengths[(uint64_t)k * per + c] = (uint32_t)t_len[k] - aln_shuffle_trim_of(spec->seed, stream[k], c, spec->max_trim);
    seqset_done(ss, t0, up, sizeof(aln_signif_record) * n + (f ? 8 * total : 0));
    return ALN_OK;
}

// (host memory that cannot be had -- the tables of a chunk of 2^22 copies, the listed hits' own -- is ALN_ERR_OOM, not an exception
// through the C boundary)
extern "C" int aln_seqset_held_significance(aln_seqset *ss, const aln_params *params, const aln_shuffle_spec *spec, const uint32_t *keep,
                                            uint64_t n_keep, aln_signif_record *records, double *f, uint32_t *lengths)
{
    ALN_GUARDED(seqset_live(ss), seqset_held_significance(ss, params, spec, keep, n_keep, records, f, lengths))
}

// ---- reports of held hits: the columns of the held strings classed and counted on the device (aln_report.hip, aln_report_rules.h).
// What both calls check before anything moves, and the scheme's bit table; neither call writes the held store's entries.
static int seqset_report_check(aln_seqset *ss, const aln_params *params, uint32_t flags, std::vector<uint32_t> &bits)
{
    int st = seqset_held_check(ss);
    if (st != ALN_OK) return st;
    if (!params || !params->matrix) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (flags & ~ALN_REPORT_SKIP_SEED) { g_err = "unknown flag bits"; return ALN_ERR_INVALID_ARGUMENT; }
    if (params->semantics == ALN_PWM_LOCAL) { g_err = "a report classes the columns of a substitution-matrix alignment"; return ALN_ERR_UNSUPPORTED; }
    const uint64_t entries = (uint64_t)params->rows * params->cols;
    if (entries == 0) { g_err = "an empty matrix"; return ALN_ERR_INVALID_ARGUMENT; }
    if (entries > ALN_REPORT_MAX_BITS) { g_err = "rows * cols beyond 8192"; return ALN_ERR_UNSUPPORTED; }
    bits.resize(aln_report_words(params->rows, params->cols));
    aln_report_table(params->matrix, params->rows, params->cols, params->row_stride, bits.data());
    return ALN_OK;
}

// The steps of a call that has the held hits reported under a scheme, each once.  The check of a call whose filter is optional (with
// one: params, flags and the bit table; without: only that hits are held) and of the filter's reserved word -- two checks, because a
// caller's own refusals may stand between them; room for the table and n reports; the table's upload, which belongs before ev[0];
// the launch over the listed hits, or with no list over all held hits, which belongs after it.
static int seqset_filter_check(aln_seqset *ss, const aln_params *params, uint32_t flags, const aln_hit_filter *filter, std::vector<uint32_t> &bits)
{
    return filter ? seqset_report_check(ss, params, flags, bits) : seqset_held_check(ss);
}
static int filter_reserved_check(const aln_hit_filter *filter)
{
    if (filter && filter->reserved != 0) { g_err = "the filter's reserved word must be 0"; return ALN_ERR_INVALID_ARGUMENT; }
    return ALN_OK;
}
static int seqset_reports_ensure(aln_seqset *ss, const std::vector<uint32_t> &bits, uint64_t n)
{
    const int st = dev_ensure(ss->rep_bits, 4ull * bits.size(), false);
    return st != ALN_OK ? st : dev_ensure(ss->reports, sizeof(aln_hit_report) * n, false);
}
static int seqset_bits_upload(aln_seqset *ss, const std::vector<uint32_t> &bits, hipStream_t q)
{
    HIPCHK(hipMemcpyAsync(ss->rep_bits.p, bits.data(), 4ull * bits.size(), hipMemcpyHostToDevice, q));
    return ALN_OK;
}
static int seqset_report_queue(aln_seqset *ss, const aln_params *params, uint32_t flags, const uint32_t *list_d, uint64_t n, hipStream_t q)
{
    const HeldView v = held_view(ss->held_store);
    aln_report_launch(v.info, v.res, v.tb, list_d, (uint32_t)n, (uint32_t)ss->hit_pair.size(), ss->rep_bits.as<uint32_t>(), params->rows, params->cols,
                      params->blank_code, flags, ss->reports.as<aln_hit_report>(), q);
    HIPCHK(hipGetLastError());
    return ALN_OK;
}
static int seqset_report_all(aln_seqset *ss, const aln_params *params, uint32_t flags, hipStream_t q)
{
    return seqset_report_queue(ss, params, flags, nullptr, ss->hit_pair.size(), q);
}
// What cluster, profiles and the MSA plan send up of the held hits before ev[0]: the endpoints from the host's held list and, with a
// filter (bits: its table, else null), the table; nothing when nothing is held.  And the bytes of that.
static int seqset_endpoints_upload(aln_seqset *ss, uint32_t *d_q, uint32_t *d_t, const std::vector<uint32_t> *bits, hipStream_t q)
{
    const uint64_t held = ss->hit_pair.size();
    if (!held) return ALN_OK;
    HIPCHK(hipMemcpyAsync(d_q, ss->hit_q.data(), 4 * held, hipMemcpyHostToDevice, q));
    HIPCHK(hipMemcpyAsync(d_t, ss->hit_t.data(), 4 * held, hipMemcpyHostToDevice, q));
    return bits ? seqset_bits_upload(ss, *bits, q) : ALN_OK;
}
static uint64_t seqset_endpoints_bytes(const aln_seqset *ss, const std::vector<uint32_t> *bits)
{
    const uint64_t held = ss->hit_pair.size();
    return 8ull * held + (bits && held ? 4ull * bits->size() : 0);
}

static int seqset_held_report(aln_seqset *ss, const aln_params *params, uint32_t flags, const uint32_t *keep, uint64_t n,
                              aln_hit_report *reports)
{
    std::vector<uint32_t> bits;
    int st = seqset_report_check(ss, params, flags, bits);
    if (st != ALN_OK) return st;
    if (n && (!keep || !reports)) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if ((st = held_list_check(keep, n, ss->hit_pair.size(), 0x7FFFFFF0ull)) != ALN_OK) return st;
    if (n == 0) return ALN_OK;
    HIPCHK(hipSetDevice(ss->ctx->device));
    hipStream_t q = ss->slot->stream;
    if ((st = dev_ensure(ss->held_store.list, 4ull * n, false)) != ALN_OK) return st;
    if ((st = seqset_reports_ensure(ss, bits, n)) != ALN_OK) return st;
    const auto t0 = std::chrono::steady_clock::now();
    // (the records land in a buffer of the call's own first: an error on the way leaves the caller's array as it was)
    std::vector<aln_hit_report> rep(n);
    st = run_queued(q, [&]() -> int {
        int e;
        HIPCHK(hipMemcpyAsync(ss->held_store.list.p, keep, 4ull * n, hipMemcpyHostToDevice, q));
        if ((e = seqset_bits_upload(ss, bits, q)) != ALN_OK) return e;
        HIPCHK(hipEventRecord(ss->ev[0], q));
        if ((e = seqset_report_queue(ss, params, flags, ss->held_store.list.as<uint32_t>(), n, q)) != ALN_OK) return e;
        HIPCHK(hipEventRecord(ss->ev[1], q));
        HIPCHK(hipMemcpyAsync(rep.data(), ss->reports.p, sizeof(aln_hit_report) * n, hipMemcpyDeviceToHost, q));
        HIPCHK(hipStreamSynchronize(q));
        return ALN_OK;
    });
    if (st != ALN_OK) return st;
    memcpy(reports, rep.data(), sizeof(aln_hit_report) * n);
    seqset_done(ss, t0, 4ull * n + 4ull * bits.size(), sizeof(aln_hit_report) * n);
    return ALN_OK;
}

static int seqset_held_filter(aln_seqset *ss, const aln_params *params, uint32_t flags, const aln_hit_filter *filter, uint32_t *positions,
                              aln_hit_report *reports, uint64_t capacity, uint64_t *count)
{
    std::vector<uint32_t> bits;
    int st = seqset_report_check(ss, params, flags, bits);
    if (st != ALN_OK) return st;
    if (!filter || !count || (capacity && !positions)) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if ((st = filter_reserved_check(filter)) != ALN_OK) return st;
    const uint64_t held = ss->hit_pair.size();        // (<= 0xFFFFFFF0: seqset_hold_list)
    if (held == 0) { *count = 0; return ALN_OK; }
    const uint64_t room = std::min<uint64_t>(capacity, held);
    HIPCHK(hipSetDevice(ss->ctx->device));
    hipStream_t q = ss->slot->stream;
    uint32_t *tile_count, *tile_off;
    if ((st = tiles_ensure(ss->tiles, aln_seqset_tiles(held), &tile_count, &tile_off)) != ALN_OK) return st;
    if ((st = seqset_reports_ensure(ss, bits, held)) != ALN_OK) return st;
    if ((st = dev_ensure(ss->rep_pos, 4ull * room, false)) != ALN_OK) return st;
    if (reports && (st = dev_ensure(ss->rep_out, sizeof(aln_hit_report) * room, false)) != ALN_OK) return st;
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t *d_count = ss->misc.as<uint32_t>() + ALN_SEQSET_MISC_COMPACT;
    uint32_t kept = 0;
    uint64_t wrote = 0;
    std::vector<uint32_t> pos;
    std::vector<aln_hit_report> rep;
    st = run_queued(q, [&]() -> int {
        int e;
        if ((e = seqset_bits_upload(ss, bits, q)) != ALN_OK) return e;
        HIPCHK(hipEventRecord(ss->ev[0], q));
        if ((e = seqset_report_all(ss, params, flags, q)) != ALN_OK) return e;
        aln_report_launch_filter(ss->reports.as<aln_hit_report>(), held_view(ss->held_store).info, (uint32_t)held, filter, tile_count, tile_off,
                                 d_count, room, ss->rep_pos.as<uint32_t>(), reports ? ss->rep_out.as<aln_hit_report>() : nullptr, q);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ss->ev[1], q));
        HIPCHK(hipMemcpyAsync(&kept, d_count, 4, hipMemcpyDeviceToHost, q));
        HIPCHK(hipStreamSynchronize(q));
        if (kept > held) { g_err = "the selection kept more entries than are held"; return ALN_ERR_DEVICE; }
        wrote = std::min<uint64_t>(kept, room);
        // (the kept land in buffers of the call's own first: an error on the way leaves the caller's arrays as they were)
        pos.resize(wrote);
        if (reports) rep.resize(wrote);
        if (wrote) {
            HIPCHK(hipMemcpyAsync(pos.data(), ss->rep_pos.p, 4ull * wrote, hipMemcpyDeviceToHost, q));
            if (reports) HIPCHK(hipMemcpyAsync(rep.data(), ss->rep_out.p, sizeof(aln_hit_report) * wrote, hipMemcpyDeviceToHost, q));
            HIPCHK(hipStreamSynchronize(q));
        }
        return ALN_OK;
    });
    if (st != ALN_OK) return st;
    if (wrote) {
        memcpy(positions, pos.data(), 4ull * wrote);
        if (reports) memcpy(reports, rep.data(), sizeof(aln_hit_report) * wrote);
    }
    *count = kept;
    // (the 4-byte count aside: what comes down per kept hit)
    seqset_done(ss, t0, 4ull * bits.size(), wrote * (4ull + (reports ? sizeof(aln_hit_report) : 0)));
    return ALN_OK;
}

extern "C" int aln_seqset_held_report(aln_seqset *ss, const aln_params *params, uint32_t flags, const uint32_t *keep, uint64_t n_keep,
                                      aln_hit_report *reports)
{
    ALN_GUARDED(seqset_live(ss), seqset_held_report(ss, params, flags, keep, n_keep, reports))
}

extern "C" int aln_seqset_held_filter(aln_seqset *ss, const aln_params *params, uint32_t flags, const aln_hit_filter *filter,
                                      uint32_t *positions, aln_hit_report *reports, uint64_t capacity, uint64_t *count)
{
    ALN_GUARDED(seqset_live(ss), seqset_held_filter(ss, params, flags, filter, positions, reports, capacity, count))
}

extern "C" int aln_seqset_stats(const aln_seqset *ss, double *ms, uint64_t *bytes)
{
    return stats_get(ss, ms, bytes);
}

// ---------------------------------------------------------------- clusters of an edge list (aln_cluster.hip, aln_cluster_rules.h)
// What the kernels take of one call's arena (cluster_carve, aln_arena_rules.h).  len: the arena's own table, the set's, or null.
static ClusterArgs cluster_args(const ClusterBufs &b, uint32_t mode, uint64_t n, uint64_t m, const aln_cluster_nodes &nodes, const uint32_t *len)
{
    ClusterArgs a = ClusterArgs();
    a.nodes = nodes; a.n = n; a.m = m; a.mode = mode;
    a.len = len; a.ea = b.ea; a.eb = b.eb;
    a.label = b.label; a.aux0 = b.aux0; a.aux1 = b.aux1; a.aux2 = b.aux2; a.key = b.key; a.size = b.size; a.cedges = b.cedges; a.misc = b.misc;
    return a;
}

// The rounds and the finish, on a stream whose earlier work (the endpoints' upload, the held edges) is queued already.  The host reads
// one 4-byte word per round: components the changed word, greedy the undecided count.  Labels, the first `room` records and the
// summary land in the call's own host buffers.  On an error the caller waits for the stream.
static int cluster_core(hipStream_t q, const ClusterArgs &a, const ClusterBufs &b, uint64_t room, std::vector<uint32_t> &label_h,
                        std::vector<aln_cluster_record> &rec_h, aln_cluster_summary &sum, uint64_t *down)
{
    const uint64_t nodes = aln_cluster_node_count(a.nodes);
    const uint64_t bound = a.n + 2;
    uint32_t rounds = 0, word = 0;
    HIPCHK(hipMemsetAsync(a.misc, 0, 64, q));
    aln_cluster_launch_init(&a, q);
    HIPCHK(hipGetLastError());
    if (a.mode == ALN_CLUSTER_COMPONENTS) {
        for (word = a.m ? 1u : 0u; word;) {
            if (rounds >= bound) { g_err = "components: the rounds did not settle within n_nodes + 2"; return ALN_ERR_DEVICE; }
            HIPCHK(hipMemsetAsync(a.misc, 0, 4, q));
            aln_cluster_launch_hook(&a, q);
            aln_cluster_launch_compress(&a, q);
            HIPCHK(hipGetLastError());
            ++rounds;
            HIPCHK(hipMemcpyAsync(&word, a.misc, 4, hipMemcpyDeviceToHost, q));
            HIPCHK(hipStreamSynchronize(q));
        }
    } else {
        for (word = nodes ? 1u : 0u; word;) {
            if (rounds >= bound) { g_err = "greedy: the rounds did not settle within n_nodes + 2"; return ALN_ERR_DEVICE; }
            HIPCHK(hipMemsetAsync(a.misc, 0, 4, q));
            aln_cluster_launch_greedy_round(&a, q);
            HIPCHK(hipGetLastError());
            ++rounds;
            HIPCHK(hipMemcpyAsync(&word, a.misc, 4, hipMemcpyDeviceToHost, q));
            HIPCHK(hipStreamSynchronize(q));
        }
        aln_cluster_launch_greedy_assign(&a, q);
        HIPCHK(hipGetLastError());
    }
    aln_cluster_launch_finish(&a, b.tile_count, b.tile_off, a.misc + 1, room, b.rec, q);
    HIPCHK(hipGetLastError());
    uint32_t misc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    HIPCHK(hipMemcpyAsync(misc, a.misc, 32, hipMemcpyDeviceToHost, q));
    HIPCHK(hipStreamSynchronize(q));
    const uint64_t clusters = misc[1];
    if (clusters > nodes) { g_err = "the cluster list holds more clusters than there are nodes"; return ALN_ERR_DEVICE; }
    const uint64_t wrote = std::min<uint64_t>(clusters, room);
    label_h.resize(a.n);
    rec_h.resize(wrote);
    HIPCHK(hipMemcpyAsync(label_h.data(), a.label, 4 * a.n, hipMemcpyDeviceToHost, q));
    if (wrote) HIPCHK(hipMemcpyAsync(rec_h.data(), b.rec, sizeof(aln_cluster_record) * wrote, hipMemcpyDeviceToHost, q));
    HIPCHK(hipStreamSynchronize(q));
    memset(&sum, 0, sizeof sum);
    sum.nodes = nodes;
    sum.clusters = clusters;
    memcpy(&sum.edges, misc + 2, 8);
    memcpy(&sum.self_edges, misc + 4, 8);
    memcpy(&sum.singletons, misc + 6, 8);
    sum.rounds = rounds;
    if (down) *down = 4 * a.n + sizeof(aln_cluster_record) * wrote + 32 + 4ull * rounds;
    return ALN_OK;
}

static int cluster_edges(aln_ctx *ctx, uint32_t mode, uint64_t n_nodes, const uint32_t *node_len, const uint32_t *edge_a, const uint32_t *edge_b,
                         uint64_t n_edges, uint32_t *label, aln_cluster_record *clusters, uint64_t capacity, aln_cluster_summary *summary)
{
    if (mode != ALN_CLUSTER_COMPONENTS && mode != ALN_CLUSTER_GREEDY) { g_err = "unknown cluster mode"; return ALN_ERR_INVALID_ARGUMENT; }
    if (!ctx || !summary) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n_nodes > ALN_CLUSTER_MAX || n_edges > ALN_CLUSTER_MAX) { g_err = "more than 0xFFFFFFF0 nodes or edges"; return ALN_ERR_INVALID_ARGUMENT; }
    if ((n_nodes && !label) || (n_edges && (!edge_a || !edge_b)) || (capacity && !clusters)) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    for (uint64_t k = 0; k < n_edges; ++k)
        if (edge_a[k] >= n_nodes || edge_b[k] >= n_nodes) { g_err = "an edge's endpoint is not a node"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n_nodes == 0) { memset(summary, 0, sizeof *summary); return ALN_OK; }
    const uint64_t room = std::min<uint64_t>(capacity, n_nodes);
    DevCtx *dev = ctx->devs[0];
    HIPCHK(hipSetDevice(dev->device));
    Slot *sl[1];
    pool_lease(dev, 1, sl);
    struct Release { DevCtx *c; Slot **s; ~Release() { pool_release(c, s, 1); } } rel{dev, sl};
    Slot &s = *sl[0];
    int st;
    if ((st = slot_init(s)) != ALN_OK) return st;
    // (the slot's shuffle table is a call's scratch: nothing outlives the call that wrote it)
    const uint64_t tiles = aln_cluster_tiles(n_nodes);
    if ((st = dev_ensure(s.shuffle, cluster_carve(nullptr, mode, n_nodes, n_edges, room, tiles, node_len != nullptr, nullptr), s.pooled)) != ALN_OK) return st;
    ClusterBufs b;
    cluster_carve(s.shuffle.as<uint8_t>(), mode, n_nodes, n_edges, room, tiles, node_len != nullptr, &b);
    const ClusterArgs a = cluster_args(b, mode, n_nodes, n_edges, aln_cluster_nodes_all(n_nodes), b.len);
    hipStream_t q = s.stream;
    std::vector<uint32_t> label_h;
    std::vector<aln_cluster_record> rec_h;
    aln_cluster_summary sum;
    st = run_queued(q, [&]() -> int {
        if (n_edges) {
            HIPCHK(hipMemcpyAsync(b.ea, edge_a, 4 * n_edges, hipMemcpyHostToDevice, q));
            HIPCHK(hipMemcpyAsync(b.eb, edge_b, 4 * n_edges, hipMemcpyHostToDevice, q));
        }
        if (node_len) HIPCHK(hipMemcpyAsync(b.len, node_len, 4 * n_nodes, hipMemcpyHostToDevice, q));
        return cluster_core(q, a, b, room, label_h, rec_h, sum, nullptr);
    });
    if (st != ALN_OK) return st;
    // (everything landed in buffers of the call's own first: an error on the way left the caller's arrays as they were)
    memcpy(label, label_h.data(), 4 * n_nodes);
    if (!rec_h.empty()) memcpy(clusters, rec_h.data(), sizeof(aln_cluster_record) * rec_h.size());
    *summary = sum;
    return ALN_OK;
}

// The sequences of a set grouped by its held hits.  The endpoints go up from the host's held list (8 bytes per held hit: the list is
// the host's, as the re-fill was planned from it); with a filter the reports of ALL held hits are written into the set's report
// buffer as held_filter writes them, and a kernel drops the edges the rule does not keep.  The held store is only read.
static int seqset_held_cluster(aln_seqset *ss, const aln_params *params, uint32_t flags, const aln_hit_filter *filter, uint32_t mode,
                               uint32_t *label, aln_cluster_record *clusters, uint64_t capacity, aln_cluster_summary *summary)
{
    std::vector<uint32_t> bits;
    int st = seqset_filter_check(ss, params, flags, filter, bits);
    if (st != ALN_OK) return st;
    if ((st = filter_reserved_check(filter)) != ALN_OK) return st;
    if (mode != ALN_CLUSTER_COMPONENTS && mode != ALN_CLUSTER_GREEDY) { g_err = "unknown cluster mode"; return ALN_ERR_INVALID_ARGUMENT; }
    if (!summary || (ss->n && !label) || (capacity && !clusters)) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    const uint64_t n = ss->n, held = ss->hit_pair.size();      // (n < 2^32 - 16 is checked below; held <= 0xFFFFFFF0: seqset_hold_list)
    if (n > ALN_CLUSTER_MAX) { g_err = "more than 0xFFFFFFF0 sequences"; return ALN_ERR_UNSUPPORTED; }
    const uint64_t room = std::min<uint64_t>(capacity, n);
    HIPCHK(hipSetDevice(ss->ctx->device));
    hipStream_t q = ss->slot->stream;
    const uint64_t tiles = aln_cluster_tiles(n);
    if ((st = dev_ensure(ss->cluster, cluster_carve(nullptr, mode, n, held, room, tiles, false, nullptr), false)) != ALN_OK) return st;
    if (filter && held && (st = seqset_reports_ensure(ss, bits, held)) != ALN_OK) return st;
    ClusterBufs b;
    cluster_carve(ss->cluster.as<uint8_t>(), mode, n, held, room, tiles, false, &b);
    const ClusterArgs a = cluster_args(b, mode, n, held, aln_cluster_nodes_of_block(ss->held_block), ss->d_len.as<uint32_t>());
    const std::vector<uint32_t> *up_bits = filter ? &bits : nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint32_t> label_h;
    std::vector<aln_cluster_record> rec_h;
    aln_cluster_summary sum;
    uint64_t down = 0;
    st = run_queued(q, [&]() -> int {
        int e;
        if ((e = seqset_endpoints_upload(ss, b.ea, b.eb, up_bits, q)) != ALN_OK) return e;
        HIPCHK(hipEventRecord(ss->ev[0], q));
        if (held) {
            if (filter && (e = seqset_report_all(ss, params, flags, q)) != ALN_OK) return e;
            const HeldView v = held_view(ss->held_store);
            aln_cluster_launch_held_edges(v.res, ss->reports.as<aln_hit_report>(), v.info, filter, held, b.ea, b.eb, q);
            HIPCHK(hipGetLastError());
        }
        if ((e = cluster_core(q, a, b, room, label_h, rec_h, sum, &down)) != ALN_OK) return e;
        HIPCHK(hipEventRecord(ss->ev[1], q));
        HIPCHK(hipStreamSynchronize(q));
        return ALN_OK;
    });
    if (st != ALN_OK) return st;
    if (n) memcpy(label, label_h.data(), 4 * n);
    if (!rec_h.empty()) memcpy(clusters, rec_h.data(), sizeof(aln_cluster_record) * rec_h.size());
    *summary = sum;
    seqset_done(ss, t0, seqset_endpoints_bytes(ss, up_bits), down);
    return ALN_OK;
}

extern "C" int aln_cluster_edges(aln_ctx *ctx, uint32_t mode, uint64_t n_nodes, const uint32_t *node_len, const uint32_t *edge_a,
                                 const uint32_t *edge_b, uint64_t n_edges, uint32_t *label, aln_cluster_record *clusters, uint64_t capacity,
                                 aln_cluster_summary *summary)
{
    ALN_GUARDED(ctx != nullptr, cluster_edges(ctx, mode, n_nodes, node_len, edge_a, edge_b, n_edges, label, clusters, capacity, summary))
}

extern "C" int aln_seqset_held_cluster(aln_seqset *ss, const aln_params *params, uint32_t flags, const aln_hit_filter *filter, uint32_t mode,
                                       uint32_t *label, aln_cluster_record *clusters, uint64_t capacity, aln_cluster_summary *summary)
{
    ALN_GUARDED(seqset_live(ss), seqset_held_cluster(ss, params, flags, filter, mode, label, clusters, capacity, summary))
}

// ---------------------------------------------------------------- profiles of a set's families (aln_profile.hip, aln_profile_rules.h)
// What profiles and the MSA plan do alike around their own kernels, on the pieces their arenas share (FamilyBufs, aln_arena_rules.h).
// Up, before ev[0]: the endpoints and the filter's table, the labels, the centres and their offsets -- and the bytes of that.
static int family_upload(aln_seqset *ss, const FamilyBufs &b, const std::vector<uint32_t> *bits, const uint32_t *label, const uint32_t *centers,
                         uint64_t n_centers, const uint64_t *off, hipStream_t q)
{
    const int st = seqset_endpoints_upload(ss, b.hit_q, b.hit_t, bits, q);
    if (st != ALN_OK) return st;
    if (ss->n) HIPCHK(hipMemcpyAsync(b.label, label, 4 * ss->n, hipMemcpyHostToDevice, q));
    if (n_centers) {
        HIPCHK(hipMemcpyAsync(b.centers, centers, 4 * n_centers, hipMemcpyHostToDevice, q));
        HIPCHK(hipMemcpyAsync(b.off, off, 8 * n_centers, hipMemcpyHostToDevice, q));
    }
    return ALN_OK;
}
static uint64_t family_upload_bytes(const aln_seqset *ss, const std::vector<uint32_t> *bits, uint64_t n_centers)
{
    return seqset_endpoints_bytes(ss, bits) + 4ull * ss->n + 12ull * n_centers;
}
// After ev[0]: the counters zero, no sequence a centre yet, the records (of either kind: rec_bytes in all) zero.
static int family_clear(const aln_seqset *ss, const FamilyBufs &b, void *rec, size_t rec_bytes, hipStream_t q)
{
    HIPCHK(hipMemsetAsync(b.misc, 0, 8 * ALN_PROFILE_MISC_WORDS, q));
    if (ss->n) HIPCHK(hipMemsetAsync(b.slot_of, 0xFF, 4 * ss->n, q));
    if (rec_bytes) HIPCHK(hipMemsetAsync(rec, 0, rec_bytes, q));
    return ALN_OK;
}
// The counters both summaries report (a 64-bit counter saturates into a 32-bit field); the rest of the summary is zero.
static uint32_t sat32(unsigned long long v) { return (uint32_t)std::min<unsigned long long>(v, 0xFFFFFFFFull); }
template <class Summary> static void family_summary(Summary *summary, uint64_t held, const unsigned long long *misc)
{
    memset(summary, 0, sizeof *summary);
    summary->held = held;
    summary->contributing = misc[ALN_PROFILE_COUNTS];
    summary->self_pairs = sat32(misc[ALN_PROFILE_SELF]);
    summary->between_members = sat32(misc[ALN_PROFILE_BETWEEN]);
    summary->unlisted = sat32(misc[ALN_PROFILE_UNLISTED]);
    summary->overflow = sat32(misc[ALN_PROFILE_MISC_OVERFLOW]);
}

// what both calls check of the centres and n_codes
static int profile_layout_check(const aln_seqset *ss, const uint32_t *centers, uint64_t n_centers, uint32_t n_codes)
{
    if (!ss) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (ss->destroyed) { g_err = "the set was destroyed"; return ALN_ERR_INVALID_ARGUMENT; }
    if (!aln_profile_codes_ok(n_codes)) { g_err = "n_codes must lie in 1 .. 64"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n_centers && !centers) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n_centers > ss->n || !aln_profile_centers_ok(centers, n_centers, ss->n)) {
        g_err = "the centres must be strictly ascending sequence numbers of the set";
        return ALN_ERR_INVALID_ARGUMENT;
    }
    return ALN_OK;
}

extern "C" int aln_seqset_profile_elements(const aln_seqset *ss, const uint32_t *centers, uint64_t n_centers, uint32_t n_codes, uint64_t *total)
{
    int st = profile_layout_check(ss, centers, n_centers, n_codes);
    if (st != ALN_OK) return st;
    if (!total) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    *total = aln_profile_layout(ss->len.data(), centers, n_centers, n_codes, nullptr);
    return ALN_OK;
}

// The held hits' columns counted into the profiles of the listed centres.  Up go the endpoints from the host's held list (as the
// cluster call uploads them), the labels, the centres and their offsets; with a filter the reports of ALL held hits are written into
// the set's report buffer as held_filter writes them.  The held store is only read; the output lives in the call's own arena.
static int seqset_held_profiles(aln_seqset *ss, const aln_params *params, uint32_t flags, const aln_hit_filter *filter, const uint32_t *label,
                                const uint32_t *centers, uint64_t n_centers, uint32_t n_codes, uint32_t *out, uint64_t capacity,
                                aln_profile_record *records, aln_profile_summary *summary)
{
    if (!ss) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if ((params != nullptr) != (filter != nullptr)) { g_err = "params and filter come together: the filter's reports are classed under params"; return ALN_ERR_INVALID_ARGUMENT; }
    std::vector<uint32_t> bits;
    int st = seqset_filter_check(ss, params, flags, filter, bits);
    if (st != ALN_OK) return st;
    if (flags & ~ALN_PROFILE_SKIP_SEED) { g_err = "unknown flag bits"; return ALN_ERR_INVALID_ARGUMENT; }
    if ((st = filter_reserved_check(filter)) != ALN_OK) return st;
    if ((st = profile_layout_check(ss, centers, n_centers, n_codes)) != ALN_OK) return st;
    const uint64_t n = ss->n, held = ss->hit_pair.size();      // (n < 2^32: aln_seqset_create; held <= 0xFFFFFFF0: seqset_hold_list)
    if (!summary || (n && !label) || (n_centers && !records)) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    std::vector<uint64_t> off(n_centers);
    const uint64_t total = aln_profile_layout(ss->len.data(), centers, n_centers, n_codes, off.data());
    if (capacity < total) { g_err = "capacity_elements is below aln_seqset_profile_elements"; return ALN_ERR_INVALID_ARGUMENT; }
    if (total && !out) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (total > (1ull << 40)) { g_err = "more than 2^40 profile elements"; return ALN_ERR_UNSUPPORTED; }
    HIPCHK(hipSetDevice(ss->ctx->device));
    hipStream_t q = ss->slot->stream;
    if ((st = dev_ensure(ss->profile, profile_carve(nullptr, n, held, n_centers, total, nullptr), false)) != ALN_OK) return st;
    if (filter && held && (st = seqset_reports_ensure(ss, bits, held)) != ALN_OK) return st;
    ProfileBufs b;
    profile_carve(ss->profile.as<uint8_t>(), n, held, n_centers, total, &b);
    const HeldView v = held_view(ss->held_store);
    const std::vector<uint32_t> *up_bits = filter ? &bits : nullptr;
    ProfileArgs a;
    memset(&a, 0, sizeof a);
    a.held = v.info; a.res = v.res; a.tb = v.tb;
    a.rep = filter && held ? ss->reports.as<aln_hit_report>() : nullptr;
    if (filter) a.filter = *filter;
    a.hit_q = b.hit_q; a.hit_t = b.hit_t; a.label = b.label; a.len = ss->d_len.as<uint32_t>(); a.slot_of = b.slot_of; a.off = b.off;
    a.n_held = (uint32_t)held; a.n_seqs = (uint32_t)n; a.n_centers = (uint32_t)n_centers; a.n_codes = n_codes;
    a.blank = params ? params->blank_code : ss->held_blank;
    a.flags = flags;
    a.out = b.out; a.rec = b.rec; a.misc = b.misc;
    const auto t0 = std::chrono::steady_clock::now();
    // (everything lands in buffers of the call's own first: an error on the way leaves the caller's arrays as they were)
    std::vector<uint32_t> out_h(total);
    std::vector<aln_profile_record> rec_h(n_centers);
    unsigned long long misc[ALN_PROFILE_MISC_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    st = run_queued(q, [&]() -> int {
        int e;
        if ((e = family_upload(ss, b, up_bits, label, centers, n_centers, off.data(), q)) != ALN_OK) return e;
        HIPCHK(hipEventRecord(ss->ev[0], q));
        if ((e = family_clear(ss, b, b.rec, sizeof(aln_profile_record) * n_centers, q)) != ALN_OK) return e;
        if (total) HIPCHK(hipMemsetAsync(b.out, 0, 4 * total, q));
        aln_profile_launch_slots(b.centers, (uint32_t)n_centers, (uint32_t)n, b.slot_of, b.rec, q);
        HIPCHK(hipGetLastError());
        if (held) {
            if (filter && (e = seqset_report_all(ss, params, flags, q)) != ALN_OK) return e;
            aln_profile_launch(&a, q);
            HIPCHK(hipGetLastError());
        }
        HIPCHK(hipEventRecord(ss->ev[1], q));
        HIPCHK(hipMemcpyAsync(misc, b.misc, 8 * ALN_PROFILE_MISC_WORDS, hipMemcpyDeviceToHost, q));
        if (n_centers) HIPCHK(hipMemcpyAsync(rec_h.data(), b.rec, sizeof(aln_profile_record) * n_centers, hipMemcpyDeviceToHost, q));
        if (total) HIPCHK(hipMemcpyAsync(out_h.data(), b.out, 4 * total, hipMemcpyDeviceToHost, q));
        HIPCHK(hipStreamSynchronize(q));
        return ALN_OK;
    });
    if (st != ALN_OK) return st;
    if (total) memcpy(out, out_h.data(), 4 * total);
    if (n_centers) memcpy(records, rec_h.data(), sizeof(aln_profile_record) * n_centers);
    family_summary(summary, held, misc);
    summary->elements = total;
    seqset_done(ss, t0, family_upload_bytes(ss, up_bits, n_centers), 4ull * total + sizeof(aln_profile_record) * n_centers + 8ull * ALN_PROFILE_MISC_WORDS);
    return ALN_OK;
}

extern "C" int aln_seqset_held_profiles(aln_seqset *ss, const aln_params *params, uint32_t flags, const aln_hit_filter *filter, const uint32_t *label,
                                        const uint32_t *centers, uint64_t n_centers, uint32_t n_codes, uint32_t *out, uint64_t capacity,
                                        aln_profile_record *records, aln_profile_summary *summary)
{
    ALN_GUARDED(seqset_live(ss), seqset_held_profiles(ss, params, flags, filter, label, centers, n_centers, n_codes, out, capacity, records, summary))
}

// ---------------------------------------------------------------- family alignments of a set (aln_msa.hip, aln_msa_rules.h)
// what both calls hand the kernels of the plan's arena
static void msa_args(const aln_seqset *ss, const MsaPlanBufs &b, uint64_t n, uint64_t held, uint64_t n_centers, uint64_t n_ins, uint32_t blank, MsaArgs *a)
{
    memset(a, 0, sizeof *a);
    const HeldView v = held_view(ss->held_store);
    a->held = v.info; a->res = v.res; a->tb = v.tb;
    a->hit_q = b.hit_q; a->hit_t = b.hit_t; a->label = b.label; a->len = ss->d_len.as<uint32_t>(); a->slot_of = b.slot_of; a->ins_off = b.off;
    a->n_ins = n_ins;
    a->n_held = (uint32_t)held; a->n_seqs = (uint32_t)n; a->n_centers = (uint32_t)n_centers; a->blank = blank;
    a->ins = b.ins; a->col = b.col; a->mark = b.mark; a->rec = b.rec; a->misc = b.misc;
    a->seqs = ss->slot->seqs.as<uint8_t>(); a->seq_off = ss->d_off.as<uint64_t>();
}

// Who contributes, the inserts and the columns of every listed centre.  Up go what the profile call uploads (the offsets are those of
// the centres' ins / col tables); down come the records and the counters.  The held store is only read.  A refusal leaves the plan
// before it as it was; once the tables are being rewritten there is no plan until this one has gone well.
static int seqset_held_msa_plan(aln_seqset *ss, const aln_params *params, uint32_t flags, const aln_hit_filter *filter, const uint32_t *label,
                                const uint32_t *centers, uint64_t n_centers, aln_msa_record *records, aln_msa_summary *summary)
{
    // (what needs no set comes first)
    if (flags != 0) { g_err = "flags must be 0: the seed column is never part of a family alignment"; return ALN_ERR_INVALID_ARGUMENT; }
    if ((params != nullptr) != (filter != nullptr)) { g_err = "params and filter come together: the filter's reports are classed under params"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n_centers && !centers) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (!aln_profile_centers_ok(centers, n_centers, 1ull << 32)) {
        g_err = "the centres must be strictly ascending sequence numbers of the set";
        return ALN_ERR_INVALID_ARGUMENT;
    }
    if (!ss) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    std::vector<uint32_t> bits;
    int st = seqset_filter_check(ss, params, ALN_REPORT_SKIP_SEED, filter, bits);
    if (st != ALN_OK) return st;
    if ((st = filter_reserved_check(filter)) != ALN_OK) return st;
    if (ss->destroyed) { g_err = "the set was destroyed"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n_centers > ss->n || !aln_profile_centers_ok(centers, n_centers, ss->n)) {
        g_err = "the centres must be strictly ascending sequence numbers of the set";
        return ALN_ERR_INVALID_ARGUMENT;
    }
    const uint64_t n = ss->n, held = ss->hit_pair.size();      // (n < 2^32: aln_seqset_create; held <= 0xFFFFFFF0: seqset_hold_list)
    if (!summary || (n && !label) || (n_centers && !records)) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    std::vector<uint64_t> ins_off(n_centers);
    uint64_t n_ins = 0;
    for (uint64_t i = 0; i < n_centers; ++i) { ins_off[i] = n_ins; n_ins += (uint64_t)ss->len[centers[i]] + 1ull; }
    if (n_ins > (1ull << 38)) { g_err = "more than 2^38 centre positions"; return ALN_ERR_UNSUPPORTED; }
    HIPCHK(hipSetDevice(ss->ctx->device));
    hipStream_t q = ss->slot->stream;
    // (growing the arena drops the tables of the plan before: it is given up here, before anything else moves)
    if (ss->msa.cap < msa_plan_carve(nullptr, n, held, n_centers, n_ins, nullptr)) ss->msa_plan.valid = false;
    if ((st = dev_ensure(ss->msa, msa_plan_carve(nullptr, n, held, n_centers, n_ins, nullptr), false)) != ALN_OK) return st;
    if (filter && held && (st = seqset_reports_ensure(ss, bits, held)) != ALN_OK) return st;
    ss->msa_plan.valid = false;           // (the tables are rewritten from here on)
    MsaPlanBufs b;
    msa_plan_carve(ss->msa.as<uint8_t>(), n, held, n_centers, n_ins, &b);
    const uint32_t blank = params ? params->blank_code : ss->held_blank;
    MsaArgs a;
    msa_args(ss, b, n, held, n_centers, n_ins, blank, &a);
    a.rep = filter && held ? ss->reports.as<aln_hit_report>() : nullptr;
    if (filter) a.filter = *filter;
    const std::vector<uint32_t> *up_bits = filter ? &bits : nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<aln_msa_record> rec_h(n_centers);
    unsigned long long misc[ALN_MSA_MISC_WORDS] = {0, 0, 0, 0, 0, 0, 0, 0};
    st = run_queued(q, [&]() -> int {
        int e;
        if ((e = family_upload(ss, b, up_bits, label, centers, n_centers, ins_off.data(), q)) != ALN_OK) return e;
        HIPCHK(hipEventRecord(ss->ev[0], q));
        if ((e = family_clear(ss, b, b.rec, sizeof(aln_msa_record) * n_centers, q)) != ALN_OK) return e;
        if (n_ins) HIPCHK(hipMemsetAsync(b.ins, 0, 4 * n_ins, q));
        if (held && filter && (e = seqset_report_all(ss, params, ALN_REPORT_SKIP_SEED, q)) != ALN_OK) return e;
        aln_msa_launch_plan(&a, b.centers, b.slot_of, q);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ss->ev[1], q));
        HIPCHK(hipMemcpyAsync(misc, b.misc, 8 * ALN_MSA_MISC_WORDS, hipMemcpyDeviceToHost, q));
        if (n_centers) HIPCHK(hipMemcpyAsync(rec_h.data(), b.rec, sizeof(aln_msa_record) * n_centers, hipMemcpyDeviceToHost, q));
        HIPCHK(hipStreamSynchronize(q));
        return ALN_OK;
    });
    if (st != ALN_OK) return st;
    if (misc[ALN_MSA_MISC_TOO_WIDE]) { g_err = "a family's width does not fit 32 bits"; return ALN_ERR_UNSUPPORTED; }
    aln_seqset::MsaPlan plan;
    plan.byte_off.resize(n_centers); plan.row_off.resize(n_centers);
    if (!aln_msa_offsets(rec_h.data(), n_centers, plan.byte_off.data(), plan.row_off.data(), &plan.bytes, &plan.total_rows) || plan.bytes > (1ull << 46)) {
        g_err = "the family alignments take more than 2^46 bytes";
        return ALN_ERR_UNSUPPORTED;
    }
    plan.valid = true; plan.passes = ss->held_passes; plan.n = n; plan.held = held; plan.n_centers = n_centers; plan.n_ins = n_ins; plan.blank = blank;
    ss->msa_plan = std::move(plan);
    if (n_centers) memcpy(records, rec_h.data(), sizeof(aln_msa_record) * n_centers);
    family_summary(summary, held, misc);
    summary->bytes = ss->msa_plan.bytes;
    summary->total_rows = ss->msa_plan.total_rows;
    seqset_done(ss, t0, family_upload_bytes(ss, up_bits, n_centers), sizeof(aln_msa_record) * n_centers + 8ull * ALN_MSA_MISC_WORDS);
    return ALN_OK;
}

// The matrices and row lists of the last plan.  Nothing is decided again: the marks, the inserts and the columns are the plan's, resident.
static int seqset_held_msa_fill(aln_seqset *ss, uint8_t *out, uint64_t capacity_bytes, uint32_t *row_hit, uint64_t capacity_rows)
{
    int st = seqset_held_check(ss);
    if (st != ALN_OK) return st;
    const aln_seqset::MsaPlan &plan = ss->msa_plan;
    if (!plan.valid) { g_err = "no plan: aln_seqset_held_msa_plan has not run on this set"; return ALN_ERR_INVALID_ARGUMENT; }
    if (plan.passes != ss->held_passes || plan.held != ss->hit_pair.size() || plan.n != ss->n) {
        g_err = "the plan is of held hits that another pass has replaced";
        return ALN_ERR_INVALID_ARGUMENT;
    }
    if (capacity_bytes < plan.bytes || capacity_rows < plan.total_rows) { g_err = "a capacity is below the plan's totals"; return ALN_ERR_INVALID_ARGUMENT; }
    if ((plan.bytes && !out) || (plan.total_rows && !row_hit)) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    const uint64_t n = plan.n, held = plan.held, n_centers = plan.n_centers;
    HIPCHK(hipSetDevice(ss->ctx->device));
    hipStream_t q = ss->slot->stream;
    if ((st = dev_ensure(ss->msa_out, msa_fill_carve(nullptr, held, n_centers, plan.bytes, plan.total_rows, nullptr), false)) != ALN_OK) return st;
    MsaPlanBufs b;
    msa_plan_carve(ss->msa.as<uint8_t>(), n, held, n_centers, plan.n_ins, &b);
    MsaFillBufs f;
    msa_fill_carve(ss->msa_out.as<uint8_t>(), held, n_centers, plan.bytes, plan.total_rows, &f);
    MsaArgs a;
    msa_args(ss, b, n, held, n_centers, plan.n_ins, plan.blank, &a);
    a.byte_off = f.byte_off; a.row_off = f.row_off; a.taken = f.taken; a.list = f.list; a.hit_row = f.hit_row; a.row_hit = f.row_hit; a.out = f.out;
    a.bytes = plan.bytes; a.total_rows = plan.total_rows;
    const auto t0 = std::chrono::steady_clock::now();
    st = run_queued(q, [&]() -> int {
        if (n_centers) {
            HIPCHK(hipMemcpyAsync(f.byte_off, plan.byte_off.data(), 8 * n_centers, hipMemcpyHostToDevice, q));
            HIPCHK(hipMemcpyAsync(f.row_off, plan.row_off.data(), 8 * n_centers, hipMemcpyHostToDevice, q));
        }
        HIPCHK(hipEventRecord(ss->ev[0], q));
        if (n_centers) HIPCHK(hipMemsetAsync(f.taken, 0, 4 * n_centers, q));
        if (plan.total_rows) HIPCHK(hipMemsetAsync(f.list, 0xFF, 4 * plan.total_rows, q));
        if (plan.total_rows) HIPCHK(hipMemsetAsync(f.row_hit, 0xFF, 4 * plan.total_rows, q));
        if (plan.bytes) HIPCHK(hipMemsetAsync(f.out, (int)plan.blank, plan.bytes, q));
        aln_msa_launch_fill(&a, q);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ss->ev[1], q));
        if (plan.bytes) HIPCHK(hipMemcpyAsync(out, f.out, plan.bytes, hipMemcpyDeviceToHost, q));
        if (plan.total_rows) HIPCHK(hipMemcpyAsync(row_hit, f.row_hit, 4 * plan.total_rows, hipMemcpyDeviceToHost, q));
        HIPCHK(hipStreamSynchronize(q));
        return ALN_OK;
    });
    if (st != ALN_OK) return st;
    seqset_done(ss, t0, 16ull * n_centers, plan.bytes + 4ull * plan.total_rows);
    return ALN_OK;
}

extern "C" int aln_seqset_held_msa_plan(aln_seqset *ss, const aln_params *params, uint32_t flags, const aln_hit_filter *filter, const uint32_t *label,
                                        const uint32_t *centers, uint64_t n_centers, aln_msa_record *records, aln_msa_summary *summary)
{
    ALN_GUARDED(seqset_live(ss), seqset_held_msa_plan(ss, params, flags, filter, label, centers, n_centers, records, summary))
}

extern "C" int aln_seqset_held_msa_fill(aln_seqset *ss, uint8_t *out, uint64_t capacity_bytes, uint32_t *row_hit, uint64_t capacity_rows)
{
    ALN_GUARDED(seqset_live(ss), seqset_held_msa_fill(ss, out, capacity_bytes, row_hit, capacity_rows))
}

// ---------------------------------------------------------------- CIGARs of a set's held hits (aln_cigar.hip, aln_cigar_rules.h)
// what both calls hand the kernels of the plan's arena
static void cigar_args(const aln_seqset *ss, const CigarBufs &b, uint64_t n, uint64_t held, uint32_t flags, uint32_t blank, CigarArgs *a)
{
    memset(a, 0, sizeof *a);
    const HeldView v = held_view(ss->held_store);
    a->held = v.info; a->res = v.res; a->tb = v.tb;
    a->list = b.list; a->n_list = (uint32_t)n; a->n_held = (uint32_t)held; a->blank = blank; a->flags = flags; a->tiles = aln_cigar_tiles(n);
    a->rec = b.rec; a->off = b.off; a->tile_sum = b.tile_sum; a->tile_off = b.tile_off; a->misc = b.misc;
}

// Every listed hit counted and classed, the offsets of their words.  Up go the listed positions; down come the records and the
// counters.  The held store is only read.  A refusal leaves the plan before it as it was; once the tables are being rewritten there is
// no plan until this one has gone well.
// stranded: the plan of aln_seqset_held_strand_cigar_plan (aln_strand_rules.h) -- the same kernels and tables; the listed hits on a
// mirrored target are marked for the fill, one byte each, and the caller's records get their coordinates on the original records
static int seqset_held_cigar_plan(aln_seqset *ss, uint32_t flags, const uint32_t *which, uint64_t n, aln_cigar_record *records,
                                  aln_cigar_summary *summary, bool stranded = false, aln_strand_record *strands = nullptr)
{
    // (what needs no set comes first)
    if (!aln_cigar_flags_ok(flags)) { g_err = "unknown flag bits"; return ALN_ERR_INVALID_ARGUMENT; }
    if (!summary || (n && (!which || !records || (stranded && !strands)))) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    int st = held_length_check(n, 0x7FFFFFF0ull);
    if (st != ALN_OK) return st;
    if ((st = seqset_held_check(ss)) != ALN_OK) return st;
    if (ss->destroyed) { g_err = "the set was destroyed"; return ALN_ERR_INVALID_ARGUMENT; }
    if (stranded && !ss->strand_n) { g_err = "not a stranded set: aln_seqset_create_stranded made none of its records"; return ALN_ERR_INVALID_ARGUMENT; }
    const uint64_t held = ss->hit_pair.size();        // (<= 0xFFFFFFF0: seqset_hold_list)
    if ((st = held_list_check(which, n, held, 0x7FFFFFF0ull)) != ALN_OK) return st;
    uint64_t longest = 0;
    for (uint64_t i = 0; i < ss->n; ++i) longest = std::max<uint64_t>(longest, ss->len[i]);
    if (!aln_cigar_supported(longest)) { g_err = "a run must fit 28 bits: some N + M + 2 of the set reaches 2^28"; return ALN_ERR_UNSUPPORTED; }
    HIPCHK(hipSetDevice(ss->ctx->device));
    hipStream_t q = ss->slot->stream;
    // (growing the arena drops the tables of the plan before: it is given up here, before anything else moves)
    if (ss->cigar.cap < cigar_carve(nullptr, n, nullptr)) ss->cigar_plan.valid = false;
    if ((st = dev_ensure(ss->cigar, cigar_carve(nullptr, n, nullptr), false)) != ALN_OK) return st;
    ss->cigar_plan.valid = false;         // (the tables are rewritten from here on)
    std::vector<uint8_t> rev_h;
    std::vector<aln_strand_record> strand_h;
    if (stranded) {
        if ((st = dev_ensure(ss->cigar_rev, std::max<uint64_t>(n, 1), false)) != ALN_OK) return st;
        rev_h.resize(n); strand_h.resize(n);
        for (uint64_t k = 0; k < n; ++k) {
            strand_h[k] = aln_strand_classify(ss->hit_q[which[k]], ss->hit_t[which[k]], (uint32_t)ss->strand_n);
            rev_h[k] = strand_h[k].t_mirror;
        }
    }
    CigarBufs b;
    cigar_carve(ss->cigar.as<uint8_t>(), n, &b);
    const uint32_t blank = ss->held_blank;
    CigarArgs a;
    cigar_args(ss, b, n, held, flags, blank, &a);
    const auto t0 = std::chrono::steady_clock::now();
    // (the records land in a buffer of the call's own first: an error on the way leaves the caller's array as it was)
    std::vector<aln_cigar_record> rec_h(n);
    unsigned long long misc[ALN_CIGAR_MISC_WORDS] = {0, 0, 0, 0};
    st = run_queued(q, [&]() -> int {
        if (n) HIPCHK(hipMemcpyAsync(b.list, which, 4 * n, hipMemcpyHostToDevice, q));
        if (n && stranded) HIPCHK(hipMemcpyAsync(ss->cigar_rev.p, rev_h.data(), n, hipMemcpyHostToDevice, q));
        HIPCHK(hipEventRecord(ss->ev[0], q));
        HIPCHK(hipMemsetAsync(b.misc, 0, 8 * ALN_CIGAR_MISC_WORDS, q));
        aln_cigar_launch_plan(&a, q);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ss->ev[1], q));
        HIPCHK(hipMemcpyAsync(misc, b.misc, 8 * ALN_CIGAR_MISC_WORDS, hipMemcpyDeviceToHost, q));
        if (n) HIPCHK(hipMemcpyAsync(rec_h.data(), b.rec, sizeof(aln_cigar_record) * n, hipMemcpyDeviceToHost, q));
        HIPCHK(hipStreamSynchronize(q));
        return ALN_OK;
    });
    if (st != ALN_OK) return st;
    aln_seqset::CigarPlan plan;
    plan.valid = true; plan.passes = ss->held_passes; plan.n = n; plan.held = held; plan.total_ops = misc[ALN_CIGAR_MISC_TOTAL];
    plan.flags = flags; plan.blank = blank; plan.stranded = stranded;
    ss->cigar_plan = plan;
    for (uint64_t k = 0; stranded && k < n; ++k)      // (the device keeps the plain records: the fill's clips are decided from them)
        rec_h[k] = aln_strand_record_of(rec_h[k], strand_h[k], ss->len[ss->hit_q[which[k]]], ss->len[ss->hit_t[which[k]]]);
    if (n) memcpy(records, rec_h.data(), sizeof(aln_cigar_record) * n);
    if (n && stranded) memcpy(strands, strand_h.data(), sizeof(aln_strand_record) * n);
    memset(summary, 0, sizeof *summary);
    summary->held = held;
    summary->listed = n;
    summary->total_ops = plan.total_ops;
    summary->failed = sat32(misc[ALN_CIGAR_MISC_FAILED]);
    summary->padded = sat32(misc[ALN_CIGAR_MISC_PADDED]);
    summary->overflow = sat32(misc[ALN_CIGAR_MISC_OVERFLOW]);
    seqset_done(ss, t0, (stranded ? 5ull : 4ull) * n, sizeof(aln_cigar_record) * n + 8ull * ALN_CIGAR_MISC_WORDS);
    return ALN_OK;
}

// The words of the last plan, and its offsets when asked for.  Nothing is decided again: the listed positions, the records and the
// offsets are the plan's, resident.
static int seqset_held_cigar_fill(aln_seqset *ss, uint32_t *ops, uint64_t capacity_ops, uint64_t *offsets, uint64_t capacity_offsets,
                                  bool stranded = false)
{
    int st = seqset_held_check(ss);
    if (st != ALN_OK) return st;
    const aln_seqset::CigarPlan plan = ss->cigar_plan;
    if (!plan.valid) { g_err = "no plan: aln_seqset_held_cigar_plan has not run on this set"; return ALN_ERR_INVALID_ARGUMENT; }
    if (plan.stranded != stranded) { g_err = "no plan of this family: the set's last plan is the other's (plain or stranded)"; return ALN_ERR_INVALID_ARGUMENT; }
    if (plan.passes != ss->held_passes || plan.held != ss->hit_pair.size()) {
        g_err = "the plan is of held hits that another pass has replaced";
        return ALN_ERR_INVALID_ARGUMENT;
    }
    if (capacity_ops < plan.total_ops || (offsets && capacity_offsets < plan.n + 1)) { g_err = "a capacity is below the plan's totals"; return ALN_ERR_INVALID_ARGUMENT; }
    if (plan.total_ops && !ops) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    HIPCHK(hipSetDevice(ss->ctx->device));
    hipStream_t q = ss->slot->stream;
    if ((st = dev_ensure(ss->cigar_out, 4ull * std::max<uint64_t>(plan.total_ops, 1), false)) != ALN_OK) return st;
    CigarBufs b;
    cigar_carve(ss->cigar.as<uint8_t>(), plan.n, &b);
    CigarArgs a;
    cigar_args(ss, b, plan.n, plan.held, plan.flags, plan.blank, &a);
    a.ops = ss->cigar_out.as<uint32_t>();
    a.total = plan.total_ops;
    a.rev = plan.stranded ? ss->cigar_rev.as<uint8_t>() : nullptr;
    const auto t0 = std::chrono::steady_clock::now();
    st = run_queued(q, [&]() -> int {
        HIPCHK(hipEventRecord(ss->ev[0], q));
        if (plan.total_ops) HIPCHK(hipMemsetAsync(a.ops, 0, 4 * plan.total_ops, q));
        aln_cigar_launch_fill(&a, q);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ss->ev[1], q));
        if (plan.total_ops) HIPCHK(hipMemcpyAsync(ops, a.ops, 4 * plan.total_ops, hipMemcpyDeviceToHost, q));
        if (offsets) HIPCHK(hipMemcpyAsync(offsets, b.off, 8 * (plan.n + 1), hipMemcpyDeviceToHost, q));
        HIPCHK(hipStreamSynchronize(q));
        return ALN_OK;
    });
    if (st != ALN_OK) return st;
    seqset_done(ss, t0, 0, 4ull * plan.total_ops + (offsets ? 8ull * (plan.n + 1) : 0));
    return ALN_OK;
}

extern "C" int aln_seqset_held_cigar_plan(aln_seqset *ss, uint32_t flags, const uint32_t *which, uint64_t n, aln_cigar_record *records,
                                          aln_cigar_summary *summary)
{
    ALN_GUARDED(seqset_live(ss), seqset_held_cigar_plan(ss, flags, which, n, records, summary))
}

extern "C" int aln_seqset_held_cigar_fill(aln_seqset *ss, uint32_t *ops, uint64_t capacity_ops, uint64_t *offsets, uint64_t capacity_offsets)
{
    ALN_GUARDED(seqset_live(ss), seqset_held_cigar_fill(ss, ops, capacity_ops, offsets, capacity_offsets))
}

extern "C" int aln_seqset_held_strand_cigar_plan(aln_seqset *ss, uint32_t flags, const uint32_t *which, uint64_t n, aln_cigar_record *records,
                                                 aln_strand_record *strands, aln_cigar_summary *summary)
{
    ALN_GUARDED(seqset_live(ss), seqset_held_cigar_plan(ss, flags, which, n, records, summary, true, strands))
}

extern "C" int aln_seqset_held_strand_cigar_fill(aln_seqset *ss, uint32_t *ops, uint64_t capacity_ops, uint64_t *offsets, uint64_t capacity_offsets)
{
    ALN_GUARDED(seqset_live(ss), seqset_held_cigar_fill(ss, ops, capacity_ops, offsets, capacity_offsets, true))
}

// ---------------------------------------------------------------- a pair set over a block of a sequence set, and the loop's step
// Pairs first .. first + n_pairs - 1 of the block as a pair set that reads the set's own residue buffer: the host tables come from one
// walk over the block (aln_seqset_window), nothing is uploaded.
extern "C" aln_pairset *aln_pairset_create_from_set(aln_seqset *ss, const aln_seqset_block *b, uint64_t first, uint64_t n_pairs, int *status)
{
    int st = ALN_OK;
    aln_pairset *ps = nullptr;
    uint64_t pairs = 0;
    if (!ss || !b) { g_err = "null argument"; st = ALN_ERR_INVALID_ARGUMENT; }
    else if (ss->destroyed) { g_err = "the set was destroyed"; st = ALN_ERR_INVALID_ARGUMENT; }
    else if ((pairs = aln_seqset_block_pairs(ss->n, *b)) == 0) {
        g_err = "block: a range beyond the set, unequal ranges of an upper block, a reserved word, or no pairs";
        st = ALN_ERR_INVALID_ARGUMENT;
    }
    else if (first > pairs || n_pairs > pairs - first) { g_err = "first + n_pairs is beyond the block's pairs"; st = ALN_ERR_INVALID_ARGUMENT; }
    else if (n_pairs > 0xFFFFFFF0ull) { g_err = "too many pairs"; st = ALN_ERR_UNSUPPORTED; }
    if (st == ALN_OK) {
        ps = new aln_pairset();
        ps->ctx = ss->ctx;
        ps->n = (size_t)n_pairs;
        ps->slot = new Slot();
        ps->slot->pooled = false;
        ps->q_off.resize(n_pairs); ps->t_off.resize(n_pairs); ps->q_len.resize(n_pairs); ps->t_len.resize(n_pairs);
        ps->entry_of.assign(n_pairs, -1);
        std::vector<uint64_t> sq(n_pairs), tq(n_pairs);
        aln_seqset_window(*b, first, n_pairs, sq.data(), tq.data());
        for (uint64_t i = 0; i < n_pairs; ++i) {
            ps->q_off[i] = ss->off[sq[i]]; ps->q_len[i] = ss->len[sq[i]];
            ps->t_off[i] = ss->off[tq[i]]; ps->t_len[i] = ss->len[tq[i]];
        }
        hipError_t e = hipSetDevice(ps->ctx->device);
        if (e != hipSuccess) st = fail(e, "hipSetDevice");
        if (st == ALN_OK) st = slot_init(*ps->slot);
        for (int i = 0; i < 6 && st == ALN_OK; ++i) { e = hipEventCreate(&ps->ev[i]); if (e != hipSuccess) st = fail(e, "hipEventCreate"); }
        if (st != ALN_OK) { aln_pairset_destroy(ps); ps = nullptr; }      // (no owner yet: the set's count is untouched)
        else {
            ps->slot->seqs = ss->slot->seqs;       // borrowed: uploaded and waited for by aln_seqset_create, read-only since
            ps->residues = ss->total;
            ps->owner = ss;
            ++ss->derived;
        }
    }
    if (status) *status = st;
    return ps;
}

// best = 0, store[i] = transform(shared_matrix, pair i's parameters), the going list = the pairs with a root, ascending
extern "C" int aln_pairset_loop_begin(aln_pairset *ps, const double *shared_matrix, int32_t *status)
{
    if (!ps) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (!ps->heur) { g_err = "no heuristics set"; return ALN_ERR_INVALID_ARGUMENT; }
    if (!shared_matrix || (ps->n && !status)) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    HIPCHK(hipSetDevice(ps->ctx->device));
    hipStream_t q = ps->slot->stream;
    HIPCHK(hipStreamSynchronize(q));
    const uint32_t n = (uint32_t)ps->n;
    const uint64_t e = (uint64_t)ps->h_rows * ps->h_cols;
    uint32_t *tile_count, *tile_off;
    int st;
    if ((st = dev_ensure(ps->best, 8ull * n, false)) != ALN_OK) return st;
    if ((st = dev_ensure(ps->going[0], 4ull * n, false)) != ALN_OK) return st;
    if ((st = dev_ensure(ps->going[1], 4ull * n, false)) != ALN_OK) return st;
    if ((st = dev_ensure(ps->cls, 4ull * n, false)) != ALN_OK) return st;
    if ((st = tiles_ensure(ps->l_tiles, aln_loop_tiles(n), &tile_count, &tile_off)) != ALN_OK) return st;
    if ((st = dev_ensure(ps->l_count, 256, false)) != ALN_OK) return st;
    if ((st = dev_ensure(ps->h_status, 4ull * n, false)) != ALN_OK) return st;
    if ((st = dev_ensure(ps->shared, 8ull * e, false)) != ALN_OK) return st;
    ps->loop = false;
    ps->going_h.clear();
    ps->cur = 0;
    ps->ms[2] = 0;
    ps->bytes[0] = ps->bytes[1] = 0;
    const auto t0 = std::chrono::steady_clock::now();
    if (n) {
        HIPCHK(hipMemsetAsync(ps->best.p, 0, 8ull * n, q));                     // +0.0
        HIPCHK(hipMemcpyAsync(ps->shared.p, shared_matrix, 8ull * e, hipMemcpyHostToDevice, q));
        PairsetTransformArgs a{};
        a.shared = ps->shared.as<double>();
        a.freq = ps->h_freq.as<double>(); a.kd = ps->h_kd.as<double>(); a.r2 = ps->h_r2.as<double>();
        a.dst = ps->store.as<double>();                                        // listed entry k is pair k: no tables
        a.status = ps->h_status.as<int32_t>();
        a.n_list = n; a.rows = ps->h_rows; a.cols = ps->h_cols;       // (no held strings are read: blank stays 0)
        HIPCHK(hipEventRecord(ps->ev[4], q));
        if (aln_pairset_launch_transform(&a, q) != 0) { g_err = "per-pair matrices hold 1 .. 1024 entries"; return ALN_ERR_INVALID_ARGUMENT; }
        HIPCHK(hipGetLastError());
        aln_loop_launch_settle(nullptr, ps->h_status.as<int32_t>(), n, ps->cls.as<uint32_t>(), q);
        aln_loop_launch_select(ps->cls.as<uint32_t>(), n, 1u, nullptr, nullptr, tile_count, tile_off, ps->l_count.as<uint32_t>(), ps->going[0].as<uint32_t>(), nullptr, nullptr, q);
        HIPCHK(hipGetLastError());
        HIPCHK(hipEventRecord(ps->ev[5], q));
        HIPCHK(hipMemcpyAsync(status, ps->h_status.p, 4ull * n, hipMemcpyDeviceToHost, q));
        HIPCHK(hipStreamSynchronize(q));
        for (uint32_t i = 0; i < n; ++i)
            if (status[i] == 0) { ps->written[i] = 1; ps->going_h.push_back(i); }
        ps->ms[2] = ev_ms(ps->ev[4], ps->ev[5]);
        ps->bytes[0] = 8ull * e; ps->bytes[1] = 4ull * n;
    }
    ps->ms[3] = wall_ms(t0);
    ps->loop = true;
    return ALN_OK;
}

// One iteration for every going pair: aln_pairset_run_stored on the going list as it lies on the device, then classification,
// re-estimation and the two ordered compactions there; the finished pairs' numbers, causes and summaries come back.
extern "C" int aln_pairset_loop_step(aln_pairset *ps, const aln_params *params, uint32_t *finished, uint32_t *cause,
                                     aln_pair_result *finished_results, uint32_t *counts)
{
    if (!params) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    const size_t n = ps ? ps->going_h.size() : 0;
    // the run's own checks (nothing is touched if one fails); the list is the library's own
    int st = pairset_check_run(ps, params, nullptr, ps ? ps->going_h.data() : nullptr, n, nullptr, true, true);
    if (st != ALN_OK) return st;
    if (!ps->loop) { g_err = "no loop: aln_pairset_loop_begin has not run, or aln_pairset_heuristics has replaced the store"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n && (!finished || !cause || !finished_results || !counts)) { g_err = "null argument"; return ALN_ERR_INVALID_ARGUMENT; }
    if (n == 0) {
        if (counts) counts[0] = counts[1] = counts[2] = counts[3] = 0;
        return ALN_OK;
    }
    HIPCHK(hipSetDevice(ps->ctx->device));
    hipStream_t q = ps->slot->stream;
    HIPCHK(hipStreamSynchronize(q));
    const uint32_t n32 = (uint32_t)n;
    uint32_t *tile_count, *tile_off;
    // every buffer of the step before the run: a failure leaves the loop's state as it was
    if ((st = tiles_ensure(ps->l_tiles, aln_loop_tiles(n32), &tile_count, &tile_off)) != ALN_OK) return st;
    if ((st = dev_ensure(ps->cand_pair, 4ull * n, false)) != ALN_OK) return st;
    if ((st = dev_ensure(ps->cand_entry, 4ull * n, false)) != ALN_OK) return st;
    if ((st = dev_ensure(ps->fin_pair, 4ull * n, false)) != ALN_OK) return st;
    if ((st = dev_ensure(ps->fin_cause, 4ull * n, false)) != ALN_OK) return st;
    if ((st = dev_ensure(ps->fin_res, sizeof(aln_pair_result) * n, false)) != ALN_OK) return st;
    const auto t0 = std::chrono::steady_clock::now();
    uint32_t *going = ps->going[ps->cur].as<uint32_t>(), *next = ps->going[ps->cur ^ 1].as<uint32_t>();
    if ((st = pairset_run(ps, params, nullptr, ps->going_h.data(), n, nullptr, true, going)) != ALN_OK) return st;
    const double pick_ms = ps->ms[2];
    uint32_t *cls = ps->cls.as<uint32_t>();
    uint32_t *cnt = ps->l_count.as<uint32_t>();
    const aln_pair_result *res = ps->held_store.res.as<aln_pair_result>();
    HIPCHK(hipEventRecord(ps->ev[4], q));
    aln_loop_launch_classify(res, going, n32, ps->best.as<double>(), cls, q);
    aln_loop_launch_select(cls, n32, 0u, going, nullptr, tile_count, tile_off, cnt, ps->cand_pair.as<uint32_t>(), ps->cand_entry.as<uint32_t>(),
                           nullptr, q);
    HIPCHK(hipGetLastError());
    uint32_t improved = 0;
    HIPCHK(hipMemcpyAsync(&improved, cnt, 4, hipMemcpyDeviceToHost, q));
    HIPCHK(hipStreamSynchronize(q));                                          // the transform's grid is its count
    if (improved > n32) { g_err = "loop: the device's count is out of range"; return ALN_ERR_DEVICE; }
    if (improved) {
        PairsetTransformArgs a{};
        a.held = ps->held_store.info.as<HeldEntry>(); a.res = res; a.tb = ps->held_store.tb.as<uint8_t>();
        a.entry = ps->cand_entry.as<uint32_t>();
        a.par = a.dst_index = ps->cand_pair.as<uint32_t>();
        a.freq = ps->h_freq.as<double>(); a.kd = ps->h_kd.as<double>(); a.r2 = ps->h_r2.as<double>();
        a.dst = ps->store.as<double>();
        a.status = ps->h_status.as<int32_t>();
        a.n_list = improved; a.n_held = n32; a.rows = ps->h_rows; a.cols = ps->h_cols; a.blank = ps->blank;
        if (aln_pairset_launch_transform(&a, q) != 0) { g_err = "per-pair matrices hold 1 .. 1024 entries"; return ALN_ERR_INVALID_ARGUMENT; }
        aln_loop_launch_settle(ps->cand_entry.as<uint32_t>(), ps->h_status.as<int32_t>(), improved, cls, q);
        HIPCHK(hipGetLastError());
    }
    aln_loop_launch_select(cls, n32, 1u, going, nullptr, tile_count, tile_off, cnt + 1, next, nullptr, nullptr, q);
    aln_loop_launch_select(cls, n32, 2u, going, res, tile_count, tile_off, cnt + 2, ps->fin_pair.as<uint32_t>(), ps->fin_cause.as<uint32_t>(),
                           ps->fin_res.as<aln_pair_result>(), q);
    HIPCHK(hipGetLastError());
    HIPCHK(hipEventRecord(ps->ev[5], q));
    uint32_t got[2] = {0, 0};                                                 // going on, finished
    HIPCHK(hipMemcpyAsync(got, cnt + 1, 8, hipMemcpyDeviceToHost, q));
    HIPCHK(hipStreamSynchronize(q));
    const uint32_t more = got[0], fin = got[1];
    if ((uint64_t)more + fin != n) { g_err = "loop: the device's lists do not add up to the going list"; return ALN_ERR_DEVICE; }
    if (fin) {
        HIPCHK(hipMemcpyAsync(finished, ps->fin_pair.p, 4ull * fin, hipMemcpyDeviceToHost, q));
        HIPCHK(hipMemcpyAsync(cause, ps->fin_cause.p, 4ull * fin, hipMemcpyDeviceToHost, q));
        HIPCHK(hipMemcpyAsync(finished_results, ps->fin_res.p, sizeof(aln_pair_result) * fin, hipMemcpyDeviceToHost, q));
        HIPCHK(hipStreamSynchronize(q));
    }
    // the host's copy of the next list: the going list less the finished pairs (both ascending in going order)
    uint32_t done = 0;
    {
        size_t w = 0, f = 0;
        for (size_t k = 0; k < n; ++k) {
            if (f < fin && finished[f] == ps->going_h[k]) { if (cause[f] == ALN_LOOP_CAUSE_DONE) ++done; ++f; }
            else ps->going_h[w++] = ps->going_h[k];
        }
        if (f != fin || w != more) { ps->loop = false; g_err = "loop: the finished list is not a sublist of the going list"; return ALN_ERR_DEVICE; }
        ps->going_h.resize(w);
    }
    ps->cur ^= 1;
    counts[0] = n32; counts[1] = done; counts[2] = fin - done; counts[3] = more;
    ps->ms[2] = pick_ms + ev_ms(ps->ev[4], ps->ev[5]);
    ps->ms[3] = wall_ms(t0);
    ps->bytes[1] += 12ull + (4ull + 4ull + sizeof(aln_pair_result)) * fin;
    return ALN_OK;
}
