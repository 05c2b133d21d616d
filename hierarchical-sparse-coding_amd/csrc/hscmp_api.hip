// hscmp_api.hip -- host side of libhscmp.so (C ABI declared in include/hscmp.h).
//
// Owns the GPU-resident dictionary and the per-batch workspace (table-free state, event lists),
// translates the reference's keyword arguments (hsc/modeling.py:1053) into kernel parameters and
// queues prepare -> initial correlation -> greedy loop on one HIP stream.  No CPU compute path:
// every entry point either runs the HIP kernels or fails with an error code.
#include "../../include/hscmp.h"

#include "hscmp_kernels.h"
#include "hscmp_mfma.h"
#include "hscmp_bound.h"
#include "hscmp_sparse.h"
#include "hscmp_rp.h"
#include "hscmp_rp_sparse.h"
#include "hscmp_wide.h"
#include "hscmp_locomp.h"
#include "hscmp_epilogue.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <algorithm>
#include <vector>

using namespace hscmp;

// The environment knobs (field x is HSCMP_X): tests and diagnostics force a path with them, every path
// bit-identical.  read_knobs is the only reader of the environment: each entry point takes one snapshot when it is called and
// passes it down, and an encode keeps its snapshot in its plan, so hscmp_continue resumes with it.  The snapshot also arms
// HSCMP_ALLOC_FAIL_AT for the call (DevBuf::alloc counts from it), so every entry point that allocates takes one.
struct Knobs {
    bool no_dict_lists, no_row_lists, no_rowbits, no_pairing, force_gathered, force_generic;     // set or not
    bool init_only, exact_init, exact_recorr, locomp_no_mfma, no_sorted_prepare, no_lazy_clear;
    int rp, mfma_quad, sparse_packed, wide;     // 0 / 1 forces the choice; -1: not set, chosen by the shape
    int locomp_pack;                      // at most this many signals per workgroup; 0: not set, by the batch size
    int slot_hash_min, locomp_group_cap, locomp_ahead, sorted_prepare_min, lds_pad;     // the value, or the default
    int epi_lds_keys;                     // the value if a power of two in 64..kEpiLdsKeys, else kEpiLdsKeys
    bool epi_lds_keys_set;                // ... set at all, valid or not (the epilogue's LDS floor is then 8 KB instead of 64 KB)
    int alloc_fail_at;                    // tests: the n-th device allocation of the call fails as on a full card; 0: not set
};

// One device allocation, owned: freed by the destructor, handed on by move.  Every hipMalloc / hipFree of the engine is in here.
// A buffer that queued kernels may still read is freed by replace(), grow() and the destructor alike: waiting for the stream
// first is the caller's part.  Knows nothing of contexts or messages: the callers turn the hipError_t into a status.
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;           // bytes
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), cap(o.cap) { o.p = nullptr; o.cap = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept { std::swap(p, o.p); std::swap(cap, o.cap); o.release(); return *this; }
    ~DevBuf() { release(); }
    template <typename T> T* as() const { return (T*)p; }
    bool holds(size_t bytes) const { return p && cap >= bytes; }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    // Holds at least `bytes` afterwards, contents lost.  Too small: freed FIRST, then exactly `bytes` allocated (the residual
    // buffer is gigabytes: old and new together would not fit); a failure leaves the buffer empty.
    hipError_t replace(size_t bytes)
    {
        if (holds(bytes)) return hipSuccess;
        release();
        const hipError_t e = alloc(&p, bytes);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    // Holds at least `bytes` afterwards, 1/8 more allocated than asked.  `keep`: the old contents are copied over.  The old
    // buffer is freed last: a failure leaves it untouched.  *failed_bytes: the size of an allocation that failed.
    hipError_t grow(size_t bytes, bool keep, size_t* failed_bytes)
    {
        if (holds(bytes)) return hipSuccess;
        DevBuf fresh;
        const size_t want = bytes + bytes / 8 + 256;
        hipError_t e = alloc(&fresh.p, want);
        if (e != hipSuccess) { *failed_bytes = want; return e; }
        fresh.cap = want;
        if (keep && p && (e = hipMemcpy(fresh.p, p, cap, hipMemcpyDeviceToDevice)) != hipSuccess) return e;
        *this = std::move(fresh);
        return hipSuccess;
    }
    // HSCMP_ALLOC_FAIL_AT (tests): read_knobs arms it for the calling thread's entry point; the n-th allocation behind it answers
    // what hipMalloc answers on a full card, and HIP is not called
    static inline thread_local int fail_at = 0, count = 0;
    static hipError_t alloc(void** out, size_t bytes)
    {
        return fail_at > 0 && ++count == fail_at ? hipErrorOutOfMemory : hipMalloc(out, bytes);
    }
};

static Knobs read_knobs()
{
    Knobs k;
    const char* v;
    k.no_dict_lists = getenv("HSCMP_NO_DICT_LISTS"); k.no_row_lists = getenv("HSCMP_NO_ROW_LISTS"); k.no_rowbits = getenv("HSCMP_NO_ROWBITS");
    k.no_pairing = getenv("HSCMP_NO_PAIRING"); k.force_gathered = getenv("HSCMP_FORCE_GATHERED"); k.force_generic = getenv("HSCMP_FORCE_GENERIC");
    k.init_only = getenv("HSCMP_INIT_ONLY"); k.exact_init = getenv("HSCMP_EXACT_INIT"); k.exact_recorr = getenv("HSCMP_EXACT_RECORR"); k.locomp_no_mfma = getenv("HSCMP_LOCOMP_NO_MFMA");
    k.no_sorted_prepare = getenv("HSCMP_NO_SORTED_PREPARE"); k.no_lazy_clear = getenv("HSCMP_NO_LAZY_CLEAR");
    k.rp = (v = getenv("HSCMP_RP")) ? atoi(v) != 0 : -1;
    k.mfma_quad = (v = getenv("HSCMP_MFMA_QUAD")) ? atoi(v) != 0 : -1;
    k.sparse_packed = (v = getenv("HSCMP_SPARSE_PACKED")) ? atoi(v) != 0 : -1;
    k.wide = (v = getenv("HSCMP_WIDE")) ? atoi(v) != 0 : -1;
    k.locomp_pack = (v = getenv("HSCMP_LOCOMP_PACK")) ? std::max(1, atoi(v)) : 0;     // (0 and below pack like 1)
    k.slot_hash_min = (v = getenv("HSCMP_SLOT_HASH_MIN")) ? std::max(0, atoi(v)) : kSlotHashMin;
    k.locomp_group_cap = (v = getenv("HSCMP_LOCOMP_GROUP_CAP")) ? std::min(4096, std::max(2, atoi(v))) : kLocompGroupCap;
    k.locomp_ahead = (v = getenv("HSCMP_LOCOMP_AHEAD")) ? atoi(v) & 7 : 7;
    k.sorted_prepare_min = (v = getenv("HSCMP_SORTED_PREPARE_MIN")) ? atoi(v) : 2048;
    k.lds_pad = (v = getenv("HSCMP_LDS_PAD")) ? atoi(v) : 0;
    k.epi_lds_keys_set = (v = getenv("HSCMP_EPI_LDS_KEYS"));
    const int n = v ? atoi(v) : 0;
    k.epi_lds_keys = n >= 64 && n <= kEpiLdsKeys && (n & (n - 1)) == 0 ? n : kEpiLdsKeys;
    k.alloc_fail_at = (v = getenv("HSCMP_ALLOC_FAIL_AT")) ? atoi(v) : 0;
    DevBuf::fail_at = k.alloc_fail_at; DevBuf::count = 0;
    return k;
}

constexpr int kWideStepsPerPoll = 4;
constexpr int kWideMaxBatch = 16;         // default dispatch: at most this many signals

// The wide loop's shape rule, host arithmetic only (plan_encode and hscmp_wide_plan go by it): can these parameters run it --
// float32, one feature, blocked rounds of at most kWideMaxSel candidates, a width RpMfma is built for, none of the options that
// keep today's loops, and the control workgroup's LDS within kLdsLoop -- and does the default dispatch choose it.
struct WideShape { bool can = false, by_default = false; size_t control_lds = 0; };
static WideShape wide_shape(const DevParams& P, bool f32, bool has_w, bool ragged, bool locomp)
{
    WideShape ws;
    if (!f32 || ragged || locomp || !wide_params_ok(P)) return ws;
    MfmaArgs A{};
    A.G = mfma_groups(P.K); A.S4 = mfma_chunks(P.W); A.has_w = has_w ? 1 : 0;
    const int rc = dispatch_chunks<false>(A.S4, has_w, [&](auto s4c, auto hw) {
        ws.control_lds = wide_control_lds<RpMfma<decltype(s4c)::value, decltype(hw)::value>>(P, A);
        return 0;
    });
    ws.can = rc == 0 && ws.control_lds <= kLdsLoop;
    // Default: the encodes that nothing but the one-atom-at-a-time loop runs today (more candidates per round than the
    // round-parallel workgroup holds) while the batch leaves most of the chip idle; one round per call (a stopCondition
    // callback) keeps today's loop.  Bounds: DESIGN.md section 22.
    ws.by_default = ws.can && P.maxsel > RpMfma<2, false>::kMaxSel && P.B <= kWideMaxBatch && P.max_rounds <= 0;
    return ws;
}

// The kernels of one encode, chosen once by plan_encode before anything is queued: run_encode queues them (launch_init,
// launch_loop) and hscmp_continue resumes the batch with the same loop and the same knobs.
struct EncodePlan {
    enum Init { kInitMfma, kInitBound, kInitSparse, kInitOwn, kInitGeneric };
    enum Loop { kLoopMfma, kLoopSparse, kLoopGeneric, kLoopLocomp, kLoopLocompSparse, kLoopLocompMfma, kLoopWide };
    Init init = kInitGeneric;
    Loop loop = kLoopGeneric;
    bool rp = false;          // the round-parallel form of the loop (hscmp_rp.h, hscmp_rp_sparse.h)
    int group = 1;            // signals per workgroup of the loop
    bool packed = false;      // the four-workgroups-per-CU build of the sparse loop
    bool f64 = false;
    bool dict_lists = false;  // the dictionary has per-atom lists ("dictlist" kernels; "sparse" / "gathered" without)
    bool row_lists = false;   // per-row feature lists of the input's non-zero cells (the level chaining or the init writes them)
    bool kept_lists = false;  // ... and the loop keeps them current: it enters every cell it writes
    bool init_only = false;   // HSCMP_INIT_ONLY (tests): stop behind the initial correlation
    bool bound_loop = false;  // the four-signal loop re-correlates as upper bounds (MfmaRecorr BOUND)
    bool ragged = false;      // signals of different lengths: the RAGGED instances of the loops read each signal's geometry
    bool multi = false;       // a dictionary per signal out of a set: the MULTI instances of the generic pair read it through dict_of
    bool rules = false;       // stop rules per signal: a ragged batch whose RAGGED instances read ws.rules too
    Knobs knobs{};            // the encode's snapshot: the launches read pairing, row bitmaps and LDS pad from it
};

// The dictionary and everything derived from it: replaced as a whole by hscmp_set_dictionary (dtype < 0: none set).
struct Dictionary {
    int K = 0, W = 0, F = 0, dtype = -1;
    int G = 0;                // 0: one dictionary (hscmp_set_dictionary); >= 1: a set of G (hscmp_set_dictionaries): D, Dc and w hold G of
                              // them at strides K*W*F, K*W*F and K, none of the images below is built, and only
                              // hscmp_encode_batch_multi encodes with it
    DevBuf D;
    DevBuf w;                 // empty when no weights
    DevBuf Dfrag;             // MFMA fragment-ordered copy (F == 1)
    DevBuf Bimg;              // bf16 image of the bound passes (f32, F == 1, dictionary inside its model: hscmp_bound.h)
    float bound_cmax = 0.0f;            // >= max_k ||d_k|| |w_k|
    DevBuf Dt;                // [W][F][K] transposed copy for the sparsity-aware kernels (F > 1)
    DevBuf Dc;                // [K][F][W] chain-ordered copy for the dense chains (F > 1)
    DevBuf nzptr, nzwf, nzval;          // CSR of the dictionary's non-zeros per atom, chain order (sparse level dictionaries)
    int dict_nnz = 0;
    DevBuf fptr, fkw, fval;             // the same non-zeros grouped by feature
};

// The buffers of a batch, each grown on its own by ensure_workspace_g (replace: freed, then allocated), hscmp_grow_events aside.
struct Workspace {
    DevBuf x;                 // staging for host inputs
    DevBuf resid, best_c, best_k, ev_t, ev_k, ev_c, slot_t, slot_k, slot_a, sel_t, sel_k, sel_c, stats, energy, edge, scratch;
    DevBuf rowflag;           // [B][T] non-zero input rows handed over by the level chaining
    DevBuf rl_cnt, rl_f;      // per-row feature lists of the residual's possibly non-zero cells (sparse dictionaries)
    DevBuf hkey, hval;        // slot hash table [B][hmask+1]
    DevBuf head;              // [B][T] slot chains by position (round-parallel loop)
    DevBuf lgram;             // [B][kLgramDoubles] LoCOMP: Gram matrices beyond the LDS copy
    DevBuf geom;              // [B][kGeomWords] of a ragged batch
    DevBuf dict_of;           // [B] the dictionary of every signal (hscmp_encode_batch_multi)
    DevBuf rules;             // [B] SignalRule of a batch with stop rules per signal (hscmp_encode_batch_rules)
    DevBuf wide;              // control blocks and candidate arrays of the wide loop (hscmp_wide.h: wide_scratch_bytes)
};

// Workspace arena of the entry points outside the batch encode (grow-only, lives as long as the context): the hierarchical
// epilogue's buffers, then those of the row-level entry points and the device-resident table
enum { kArenaEpiRep, kArenaEpiOffsets, kArenaEpiN, kArenaEpiColptr, kArenaEpiIndices, kArenaEpiData, kArenaEpiOut, kArenaEpiKeys,
       kArenaRowA, kArenaRowB, kArenaRowC, kArenaRowD, kArenaTable, kArenaTabRes, kArenaTabW, kArenaEpiEnergy, kArenaLoad, kArenaSlots };

// The batch state and what it rests on (include/hscmp.h, "What a failed call leaves behind"):
//  - a call that may replace the dictionary or a workspace buffer first drops what depends on it (drop_batch), in front of its
//    first allocation; a failed hscmp_set_dictionary leaves no dictionary, a failed encode no batch, and every entry point
//    answers either with HSCMP_ERR_STATE before it queues anything;
//  - have_batch, ragged, geom, rules, P, plan, B / T / cap / maxsel, last and last_x_dev are written together (commit_batch), after the
//    last launch of the encode has been queued without error;
//  - listed_rows, rowflag_valid and rl_filled describe buffer contents, not the batch: they follow the writes to those buffers.
struct hscmp_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;
    std::string err;
    std::string variant = "none";
    Dictionary dict;
    Workspace ws;
    DevBuf arena[kArenaSlots];
    bool rl_filled = false;   // the lists of the current input were written by the level chaining
    // rows of ws.resid (x F float64) that a chained encode left behind with every possibly non-zero cell named by
    // ws.rl_cnt / ws.rl_f: the next chained encode clears those cells instead of the whole buffer (0: clear everything)
    int64_t listed_rows = 0;
    int listed_F = 0;
    bool rowflag_valid = false;
    // the batch
    int B = 0, T = 0, cap = 0, maxsel = 0;
    bool have_batch = false;
    // the batch was handed over by hscmp_load_level, not encoded: only slot_t / slot_k / slot_a, stats and (with signals) x belong
    // to it.  What resumes or reads an encode's state answers HSCMP_ERR_STATE (NEED_ENCODED)
    bool loaded = false;
    DevParams P{};
    // ragged batch (hscmp_encode_batch_ragged): per signal {length, block size, block count} on the host and in ws.geom, until the
    // next encode of any kind; the batch's P.T is the longest length and every per-signal array keeps that stride
    bool ragged = false;
    std::vector<int> geom;
    // stop rules per signal (hscmp_encode_batch_rules): the table on the host and in ws.rules, from the encode's drop_batch until the
    // next one (hscmp_continue resumes with it); empty: the rules of P apply to every signal
    std::vector<SignalRule> rules;
    hscmp_params last{};
    hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
    bool timed = false;
    bool timed_loop_only = false;   // the last timed launch was a hscmp_continue (no prepare / initial correlation)
    int method = 0;                 // hscmp_set_method: 0 = greedy pursuit (modeling.py:1053), 1 = LoCOMP (:1267)
    EncodePlan plan;                // the kernels of the last encode (hscmp_continue resumes its loop)
    int wide_steps = 0, wide_polls = 0, wide_worked = 0;     // the last wide loop: steps queued, times the control blocks were read, (signal, step) pairs that found work
    const void* last_x_dev = nullptr;   // device address of the signals of the last encode (hscmp_hierarchy_epilogue reads them)
    // device-resident inner-product table of LoCOMP (hscmp_table_*): [T][K] in slot kArenaTable, its residual in kArenaTabRes
    int tab_T = 0;
};

// In front of the first allocation of a call that replaces workspace buffers (dictionary: or the dictionary, which a resident
// table and the listed rows belong to as well).
static void drop_batch(hscmp_ctx* ctx, bool dictionary = false)
{
    ctx->have_batch = false; ctx->loaded = false; ctx->ragged = false; ctx->geom.clear(); ctx->rules.clear();
    if (dictionary) { ctx->tab_T = 0; ctx->listed_rows = 0; }
}

static thread_local std::string g_err;

static int fail(hscmp_ctx* ctx, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    if (ctx) ctx->err = buf; else g_err = buf;
    return code;
}

// A context that holds a set of dictionaries (hscmp_set_dictionaries) encodes through hscmp_encode_batch_multi alone: every other
// entry point that reads the dictionary answers this before it queues anything.
#define NOT_A_SET(ctx, who)                                                                     \
    if ((ctx)->dict.G > 0)                                                                      \
        return fail(ctx, HSCMP_ERR_STATE, "%s: the context holds a set of %d dictionaries (hscmp_set_dictionaries): only hscmp_encode_batch_multi encodes with it", who, (ctx)->dict.G);

#define HIP_TRY(ctx, expr)                                                                      \
    do {                                                                                        \
        hipError_t e__ = (expr);                                                                \
        if (e__ != hipSuccess)                                                                  \
            return fail(ctx, HSCMP_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), __FILE__, __LINE__); \
    } while (0)

static size_t esize(int dtype) { return dtype == HSCMP_F64 ? 8 : 4; }

static int alloc_failed(hscmp_ctx* ctx, size_t bytes, hipError_t e)
{
    return fail(ctx, HSCMP_ERR_ALLOC, "hipMalloc(%zu bytes) failed: %s", bytes, hipGetErrorString(e));
}

// Arena slot i holds at least `bytes` afterwards.  Grow-only: a call that fits reuses the buffer (no hipMalloc in the
// steady state of any entry point); a call that does not fit waits for the stream (kernels may still read the old
// buffer) and grows the slot (DevBuf::grow).  `keep`: the old contents are copied over.
static int epi_buffer(hscmp_ctx* ctx, int i, size_t bytes, bool keep = false)
{
    if (ctx->arena[i].holds(bytes)) return HSCMP_OK;
    hipError_t e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return fail(ctx, HSCMP_ERR_HIP, "hipStreamSynchronize failed: %s", hipGetErrorString(e));
    size_t failed_bytes = 0;
    if ((e = ctx->arena[i].grow(bytes, keep, &failed_bytes)) == hipSuccess) return HSCMP_OK;
    return failed_bytes ? alloc_failed(ctx, failed_bytes, e) : fail(ctx, HSCMP_ERR_HIP, "hipMemcpy failed: %s", hipGetErrorString(e));
}

extern "C" int hscmp_version(void) { return HSCMP_VERSION; }

extern "C" const char* hscmp_last_error(hscmp_ctx* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

extern "C" int hscmp_create(hscmp_ctx** out, int device_id)
{
    if (!out) return fail(nullptr, HSCMP_ERR_INVALID, "hscmp_create: out is NULL");
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0)
        return fail(nullptr, HSCMP_ERR_NO_DEVICE, "hscmp_create: no HIP device visible (%s)", hipGetErrorString(e));
    if (device_id < 0 || device_id >= n)
        return fail(nullptr, HSCMP_ERR_INVALID, "hscmp_create: device %d out of range (%d devices)", device_id, n);
    hscmp_ctx* ctx = new hscmp_ctx();
    ctx->device = device_id;
    e = hipSetDevice(device_id);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking);
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipEventCreate(&ctx->ev[i]);
    if (e != hipSuccess) {
        int rc = fail(nullptr, HSCMP_ERR_HIP, "hscmp_create: %s", hipGetErrorString(e));
        delete ctx;
        return rc;
    }
    ctx->stream = ctx->own_stream;
    *out = ctx;
    return HSCMP_OK;
}

extern "C" void hscmp_destroy(hscmp_ctx* ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (int i = 0; i < 4; ++i) if (ctx->ev[i]) (void)hipEventDestroy(ctx->ev[i]);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;               // (the buffers free themselves)
}

extern "C" int hscmp_set_method(hscmp_ctx* ctx, int method)
{
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, "hscmp_set_method: ctx is NULL");
    if (method != HSCMP_METHOD_CMP && method != HSCMP_METHOD_LOCOMP) return fail(ctx, HSCMP_ERR_INVALID, "hscmp_set_method: unknown method %d", method);
    ctx->method = method;
    return HSCMP_OK;
}

extern "C" int hscmp_set_stream(hscmp_ctx* ctx, void* hip_stream)
{
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, "hscmp_set_stream: ctx is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->stream = hip_stream ? (hipStream_t)hip_stream : ctx->own_stream;
    return HSCMP_OK;
}

extern "C" int hscmp_synchronize(hscmp_ctx* ctx)
{
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, "hscmp_synchronize: ctx is NULL");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return HSCMP_OK;
}

// A dictionary buffer of its own: `bytes` from the host, in a fresh allocation of at least `room` bytes (lists may be empty).
static int upload(hscmp_ctx* ctx, DevBuf& buf, const void* src, size_t bytes, size_t room = 0)
{
    const hipError_t e = buf.replace(std::max(bytes, room));
    if (e != hipSuccess) return alloc_failed(ctx, std::max(bytes, room), e);
    HIP_TRY(ctx, hipMemcpy(buf.p, src, bytes, hipMemcpyHostToDevice));
    return HSCMP_OK;
}

extern "C" int hscmp_set_dictionary(hscmp_ctx* ctx, const void* D, int K, int W, int F, hscmp_dtype dtype, const void* weights)
{
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, "hscmp_set_dictionary: ctx is NULL");
    if (!D || K <= 0 || W <= 0 || F <= 0) return fail(ctx, HSCMP_ERR_INVALID, "hscmp_set_dictionary: bad shape K=%d W=%d F=%d", K, W, F);
    if (dtype != HSCMP_F32 && dtype != HSCMP_F64) return fail(ctx, HSCMP_ERR_INVALID, "hscmp_set_dictionary: bad dtype %d", (int)dtype);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const Knobs kn = read_knobs();
    // the old dictionary goes before the new one is allocated (the two need not fit side by side), and with it the batch and
    // the resident table that were computed with it; the new one is built aside and moved in whole, so a failure on the way
    // leaves "no dictionary set"
    drop_batch(ctx, true);
    ctx->dict = Dictionary{};
    Dictionary d;
    d.K = K; d.W = W; d.F = F; d.dtype = dtype;
    const size_t es = esize(dtype);
    const size_t nD = (size_t)K * W * F * es;
    int rc;
    if ((rc = upload(ctx, d.D, D, nD))) return rc;
    // weights that are all exactly 1 select like no weights at all (|c * 1| == |c| bit for bit; the level-0 weights of the
    // hierarchical encoder, modeling.py:1448-1450 with no singletons): the unweighted kernels are the cheaper instances
    if (weights) {
        bool all_one = true;
        for (int k = 0; k < K && all_one; ++k)
            all_one = dtype == HSCMP_F32 ? ((const float*)weights)[k] == 1.0f : ((const double*)weights)[k] == 1.0;
        if (all_one) weights = nullptr;
    }
    if (weights && (rc = upload(ctx, d.w, weights, (size_t)K * es))) return rc;
    if (F > 1) {
        // Dt[w][f][k] = D[k][w][f]: atom index contiguous, for the gathered-window kernels
        std::vector<char> dt(nD);
        for (int k = 0; k < K; ++k)
            for (int w = 0; w < W; ++w)
                for (int f = 0; f < F; ++f)
                    memcpy(&dt[(((size_t)w * F + f) * K + k) * es], (const char*)D + (((size_t)k * W + w) * F + f) * es, es);
        if ((rc = upload(ctx, d.Dt, dt.data(), nD))) return rc;
        // Dc[k][f][w] = D[k][w][f]: consecutive addresses along the pinned chain (f outer, w inner)
        for (int k = 0; k < K; ++k)
            for (int w = 0; w < W; ++w)
                for (int f = 0; f < F; ++f)
                    memcpy(&dt[(((size_t)k * F + f) * W + w) * es], (const char*)D + (((size_t)k * W + w) * F + f) * es, es);
        if ((rc = upload(ctx, d.Dc, dt.data(), nD))) return rc;
        // per-atom list of non-zeros in chain order (f outer, w inner), kept when the dictionary is sparse
        // (level dictionaries built from decompositions + singletons, hsc/dataset.py:137-194, 826-860)
        if (W <= 32767 && F <= 65535 && !kn.no_dict_lists) {
            std::vector<int> ptr(K + 1, 0), wf;
            std::vector<char> val;
            const size_t limit = (size_t)kDictListMaxPerAtom * K;
            bool sparse = true;
            for (int k = 0; k < K && sparse; ++k) {
                for (int f = 0; f < F && sparse; ++f)
                    for (int w = 0; w < W; ++w) {
                        const char* src = (const char*)D + (((size_t)k * W + w) * F + f) * es;
                        const bool nz = dtype == HSCMP_F32 ? (*(const float*)src != 0.0f) : (*(const double*)src != 0.0);
                        if (!nz) continue;
                        if (wf.size() >= limit) { sparse = false; break; }
                        wf.push_back((w << 16) | f);
                        val.insert(val.end(), src, src + es);
                    }
                ptr[k + 1] = (int)wf.size();
            }
            if (sparse) {
                if ((rc = upload(ctx, d.nzptr, ptr.data(), (K + 1) * sizeof(int)))) return rc;
                if ((rc = upload(ctx, d.nzwf, wf.data(), wf.size() * sizeof(int), sizeof(int)))) return rc;
                if ((rc = upload(ctx, d.nzval, val.data(), val.size(), es))) return rc;
                // grouped by feature: counting sort of the per-atom lists
                if (K <= 65535) {
                    const size_t nnz = wf.size();
                    d.dict_nnz = (int)nnz;
                    std::vector<int> fp(F + 1, 0), kw(nnz);
                    std::vector<char> fv(std::max<size_t>(es, nnz * es));
                    for (size_t e = 0; e < nnz; ++e) fp[(wf[e] & 0xffff) + 1] += 1;
                    for (int f = 0; f < F; ++f) fp[f + 1] += fp[f];
                    std::vector<int> cur(fp.begin(), fp.end() - 1);
                    for (int k = 0; k < K; ++k)
                        for (int e = ptr[k]; e < ptr[k + 1]; ++e) {
                            const int o = cur[wf[e] & 0xffff]++;
                            kw[o] = (int)(((unsigned)k << 16) | (unsigned)(wf[e] >> 16));
                            memcpy(&fv[(size_t)o * es], &val[(size_t)e * es], es);
                        }
                    if ((rc = upload(ctx, d.fptr, fp.data(), (F + 1) * sizeof(int)))) return rc;
                    if ((rc = upload(ctx, d.fkw, kw.data(), nnz * sizeof(int), sizeof(int)))) return rc;
                    if ((rc = upload(ctx, d.fval, fv.data(), fv.size()))) return rc;
                }
            }
        }
    }
    // MFMA operand image of the dictionary (f32 only): built once, reused by every encode
    if (dtype == HSCMP_F32 && mfma_supported<float>(K, W, F)) {
        std::vector<float> frag;
        mfma_build_dict_image((const float*)D, K, W, F, frag);
        if ((rc = upload(ctx, d.Dfrag, frag.data(), frag.size() * sizeof(float)))) return rc;
        // the bound pass of the initial correlation (hscmp_bound.h): bf16 images no larger than the float32 one, and a
        // dictionary and weights inside the error model; otherwise every encode runs the exact initial correlation
        std::vector<unsigned short> bimg;
        float cmax = 0.0f;
        if ((size_t)2 * mfma_groups(K) * bound_steps(W) * 1024 <= TileF32::kMaxImageBytes &&
            bound_build_dict_image((const float*)D, (const float*)weights, K, W, bimg, cmax)) {
            if ((rc = upload(ctx, d.Bimg, bimg.data(), bimg.size() * sizeof(unsigned short)))) return rc;
            d.bound_cmax = cmax;
        }
    } else if (dtype == HSCMP_F64 && mfma_supported<double>(K, W, F)) {
        std::vector<double> frag;
        mfma_build_dict_image_f64((const double*)D, K, W, frag);
        if ((rc = upload(ctx, d.Dfrag, frag.data(), frag.size() * sizeof(double)))) return rc;
    }
    ctx->dict = std::move(d);
    return HSCMP_OK;
}

// A set of G dictionaries of one shape: what the generic kernels read -- D, the chain-ordered copy Dc
// (F > 1) and the weights -- dictionary after dictionary at a fixed stride, and none of the images of hscmp_set_dictionary.
extern "C" int hscmp_set_dictionaries(hscmp_ctx* ctx, const void* D, int G, int K, int W, int F, hscmp_dtype dtype, const void* weights)
{
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, "hscmp_set_dictionaries: ctx is NULL");
    if (!D || G <= 0 || K <= 0 || W <= 0 || F <= 0)
        return fail(ctx, HSCMP_ERR_INVALID, "hscmp_set_dictionaries: bad shape G=%d K=%d W=%d F=%d", G, K, W, F);
    if (dtype != HSCMP_F32 && dtype != HSCMP_F64) return fail(ctx, HSCMP_ERR_INVALID, "hscmp_set_dictionaries: bad dtype %d", (int)dtype);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    (void)read_knobs();                         // (arms HSCMP_ALLOC_FAIL_AT)
    // as hscmp_set_dictionary: the old dictionary, the batch and the table first; the set is built aside and moved in whole
    drop_batch(ctx, true);
    ctx->dict = Dictionary{};
    Dictionary d;
    d.K = K; d.W = W; d.F = F; d.dtype = dtype; d.G = G;
    const size_t es = esize(dtype), n1 = (size_t)K * W * F, nD = (size_t)G * n1 * es;
    int rc;
    if ((rc = upload(ctx, d.D, D, nD))) return rc;
    // all-ones weights count as no weights only when EVERY dictionary's are: one weighted dictionary makes the set weighted
    // (|c * 1| == |c| bit for bit, so the all-ones dictionaries of a weighted set select as they would alone)
    if (weights) {
        bool all_one = true;
        for (size_t i = 0; i < (size_t)G * K && all_one; ++i)
            all_one = dtype == HSCMP_F32 ? ((const float*)weights)[i] == 1.0f : ((const double*)weights)[i] == 1.0;
        if (all_one) weights = nullptr;
    }
    if (weights && (rc = upload(ctx, d.w, weights, (size_t)G * K * es))) return rc;
    if (F > 1) {
        // Dc[g][k][f][w] = D[g][k][w][f]: consecutive addresses along the pinned chain (f outer, w inner)
        std::vector<char> dc(nD);
        for (size_t gk = 0; gk < (size_t)G * K; ++gk)
            for (int w = 0; w < W; ++w)
                for (int f = 0; f < F; ++f)
                    memcpy(&dc[((gk * F + f) * W + w) * es], (const char*)D + ((gk * W + w) * F + f) * es, es);
        if ((rc = upload(ctx, d.Dc, dc.data(), nD))) return rc;
    }
    ctx->dict = std::move(d);
    return HSCMP_OK;
}

// geometry given explicitly (the row-level selection runs on a caller's table of any K, W: the context's dictionary is
// not involved and is not touched)
static int make_params_g(hscmp_ctx* ctx, const Knobs& kn, int K, int W, int F, int B, int T, const hscmp_params* p, DevParams* out)
{
    DevParams P{};
    P.B = B; P.T = T; P.K = K; P.W = W; P.F = F;
    P.off = (W - 1) / 2;
    set_segments(P, kMaxSeg);
    if (p->nb_blocks == 1) { P.blocked = 0; P.bs = 0; P.nbk = 0; P.maxsel = 1; }
    else {
        // modeling.py:908-918
        int bs;
        if (p->nb_blocks < 0) bs = 4 * W;
        else if (p->nb_blocks > 1) bs = (int)std::floor((double)T / (double)p->nb_blocks);
        else return fail(ctx, HSCMP_ERR_INVALID, "nb_blocks must be 1, > 1 or -1 ('auto'), got %d", p->nb_blocks);
        if (bs % 2 == 1) bs += 1;
        if (bs <= 0) return fail(ctx, HSCMP_ERR_INVALID, "nbBlocks=%d gives an empty block for T=%d", p->nb_blocks, T);
        P.blocked = 1; P.bs = bs; P.nbk = (int)std::ceil((double)T / (double)bs); P.maxsel = P.nbk + 1;
    }
    P.l0 = p->nb_nonzero_coefs < 0 ? -1 : p->nb_nonzero_coefs;
    P.has_snr = !std::isnan(p->tolerance_snr);
    P.has_scale = !std::isnan(p->tolerance_residual_scale);
    P.has_thres = !std::isnan(p->null_coeff_thres);
    P.snr_ratio = P.has_snr ? std::pow(10.0, p->tolerance_snr / 10.0) : 0.0;
    P.tol_scale = P.has_scale ? p->tolerance_residual_scale : 0.0;
    P.thres = P.has_thres ? p->null_coeff_thres : 0.0;
    P.eps = p->eps;
    if (p->max_events <= 0) return fail(ctx, HSCMP_ERR_INVALID, "max_events must be > 0");
    P.cap = p->max_events;
    P.hmask = slot_hash_mask(P.cap);
    P.hash_min = kn.slot_hash_min;
    if (ctx && ctx->method == HSCMP_METHOD_LOCOMP) P.hash_min = INT_MAX;        // (its atom body scans the slot list for the neighbourhood anyway)
    P.max_rounds = p->max_rounds;
    P.lg_cap = kn.locomp_group_cap;
    P.lc_ahead = kn.locomp_ahead;     // (default 7) bit 0: selections of a round side by side; bit 1: a group's rows re-correlated one wave per quarter (sparse policy);
                                      // bit 2: the rows of a batch of selections re-correlated behind its last one, one wave per selection
    *out = P;
    return HSCMP_OK;
}

static int make_params(hscmp_ctx* ctx, const Knobs& kn, int B, int T, const hscmp_params* p, DevParams* out)
{
    return make_params_g(ctx, kn, ctx->dict.K, ctx->dict.W, ctx->dict.F, B, T, p, out);
}

// Per-row feature lists: multi-feature inputs with a sparse dictionary (the per-atom lists tell which cells an
// atom touches).
constexpr int kRowListCap = 8;
static bool use_row_lists(const hscmp_ctx* ctx, const Knobs& kn)
{
    return ctx->dict.F > 1 && ctx->dict.nzptr.p != nullptr && !kn.no_row_lists;
}

// Workgroups per signal of the sparse initial correlation: enough to fill the chip at small batches.
static int sparse_init_split(int B, int T, int W)
{
    const int nblocks = (T + 2 * W - 2) / (2 * W - 1);
    return std::max(1, std::min(nblocks, (2048 + B - 1) / B));
}

// Every workspace buffer holds what a batch of shape P needs afterwards (0 bytes: not needed, left as it is).  A buffer that is too
// small is replaced, after one wait for the stream (the previous batch's kernels may still read it): on HSCMP_ERR_ALLOC some
// buffers are gone, which is why the callers drop the batch first.  geom_bytes: the per-signal geometry of a ragged batch;
// rules_bytes: its table of stop rules per signal.
// (element size and feature layout given explicitly: see make_params_g)
static int ensure_workspace_g(hscmp_ctx* ctx, const DevParams& P, bool need_x, size_t es, bool multi_feature, bool row_lists, size_t geom_bytes = 0,
                              size_t rules_bytes = 0)
{
    const size_t B = P.B, TF = (size_t)P.T * P.F, T = P.T, cap = P.cap, ms = P.maxsel;
    const bool locomp = ctx->method == HSCMP_METHOD_LOCOMP;
    Workspace& w = ctx->ws;
    const struct { DevBuf& buf; size_t bytes; } want[] = {
        {w.x, need_x ? B * TF * es : 0}, {w.resid, B * TF * es}, {w.best_c, B * T * es}, {w.best_k, B * T * sizeof(int)},
        {w.ev_t, B * cap * 4}, {w.ev_k, B * cap * 4}, {w.ev_c, B * cap * es},
        {w.slot_t, B * cap * 4}, {w.slot_k, B * cap * 4}, {w.slot_a, B * cap * 8},
        {w.sel_t, B * 2 * ms * 4}, {w.sel_k, B * 2 * ms * 4}, {w.sel_c, B * 2 * ms * es},
        {w.stats, B * ST_COUNT * sizeof(int)}, {w.energy, B * 2 * es}, {w.edge, B * kEdgeWords * sizeof(unsigned long long)},
        {w.scratch, multi_feature ? B * (size_t)sparse_init_split(P.B, P.T, P.W) * (2 * P.W - 1) * P.K * es : 0},
        {w.rowflag, multi_feature ? B * T : 0},
        {w.rl_cnt, row_lists ? B * T * sizeof(int) : 0}, {w.rl_f, row_lists ? B * T * kRowListCap * sizeof(int) : 0},
        {w.hkey, B * ((size_t)P.hmask + 1) * sizeof(unsigned long long)}, {w.hval, B * ((size_t)P.hmask + 1) * sizeof(int)},
        {w.head, (P.blocked || locomp) ? B * T * sizeof(int) : 0},
        {w.lgram, locomp ? B * lgram_doubles(P.lg_cap) * sizeof(double) : 0},
        {w.geom, geom_bytes}, {w.rules, rules_bytes},
        // every shape the wide loop could take, whatever HSCMP_WIDE and the batch size will make plan_encode choose behind this
        // call (52 bytes per block of a round: wide_scratch_bytes)
        {w.wide, es == 4 && !multi_feature && !locomp && geom_bytes == 0 && wide_params_ok(P) ? wide_scratch_bytes(P.B, P.maxsel) : 0},
    };
    bool stream_idle = false;
    for (const auto& b : want) {
        if (b.bytes == 0 || b.buf.holds(b.bytes)) continue;
        if (!stream_idle) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); stream_idle = true; }
        ctx->listed_rows = 0;                   // (a fresh buffer knows nothing of the previous batch)
        const hipError_t e = b.buf.replace(b.bytes);
        if (e != hipSuccess) return alloc_failed(ctx, b.bytes, e);
        // the event and slot lists are fetched whole (hscmp_fetch_events, hscmp_fetch_slots): what lies behind a signal's last entry
        // is zero, not whatever the allocation held before
        for (DevBuf* l : {&w.ev_t, &w.ev_k, &w.ev_c, &w.slot_t, &w.slot_k, &w.slot_a})
            if (l == &b.buf) HIP_TRY(ctx, hipMemsetAsync(b.buf.p, 0, b.bytes, ctx->stream));
    }
    return HSCMP_OK;
}
static int ensure_workspace(hscmp_ctx* ctx, const DevParams& P, bool need_x, bool row_lists, size_t geom_bytes = 0, size_t rules_bytes = 0)
{
    return ensure_workspace_g(ctx, P, need_x, esize(ctx->dict.dtype), ctx->dict.F > 1, row_lists, geom_bytes, rules_bytes);
}

// ragged, multi: of the batch being encoded or resumed (its plan says so), not of the one the context may still hold
template <typename R> static State<R> make_state(hscmp_ctx* c, bool ragged, bool multi = false)
{
    State<R> S;
    S.D = c->dict.D.as<const R>(); S.weights = c->dict.w.as<const R>();
    S.Dc = c->dict.Dc.p ? c->dict.Dc.as<const R>() : c->dict.D.as<const R>();
    S.residual = c->ws.resid.as<R>(); S.best_c = c->ws.best_c.as<R>(); S.best_k = c->ws.best_k.as<int>();
    S.ev_t = c->ws.ev_t.as<int>(); S.ev_k = c->ws.ev_k.as<int>(); S.ev_c = c->ws.ev_c.as<R>();
    S.slot_t = c->ws.slot_t.as<int>(); S.slot_k = c->ws.slot_k.as<int>(); S.slot_a = c->ws.slot_a.as<double>();
    S.hkey = c->ws.hkey.as<unsigned long long>(); S.hval = c->ws.hval.as<int>(); S.head = c->ws.head.as<int>(); S.lgram = c->ws.lgram.as<double>();
    S.sel_t = c->ws.sel_t.as<int>(); S.sel_k = c->ws.sel_k.as<int>(); S.sel_c = c->ws.sel_c.as<R>();
    S.stats = c->ws.stats.as<int>(); S.energy = c->ws.energy.as<R>(); S.edge = c->ws.edge.as<unsigned long long>();
    S.geom = ragged ? c->ws.geom.as<int>() : nullptr;
    S.dict_of = multi ? c->ws.dict_of.as<int>() : nullptr;
    S.rules = ragged && !c->rules.empty() ? c->ws.rules.p : nullptr;      // (the context's table is this batch's: drop_batch clears it)
    return S;
}

template <typename R> static SparseArgs<R> sparse_args(hscmp_ctx* ctx, const EncodePlan& plan, int T, bool packed = false)
{
    SparseArgs<R> A;
    A.Dt = ctx->dict.Dt.as<const R>(); A.scratch = ctx->ws.scratch.as<R>();
    A.rowflag = (T <= kRowBitsMaxT && !plan.knobs.no_rowbits) ? ctx->ws.rowflag.as<unsigned char>() : nullptr;
    A.rowflag_filled = ctx->rowflag_valid ? 1 : 0;
    A.nzptr = ctx->dict.nzptr.as<int>(); A.nzwf = ctx->dict.nzwf.as<int>(); A.nzval = ctx->dict.nzval.as<const R>();
    A.fptr = plan.knobs.no_pairing ? nullptr : ctx->dict.fptr.as<int>(); A.fkw = ctx->dict.fkw.as<int>(); A.fval = ctx->dict.fval.as<const R>();
    A.nnz = ctx->dict.dict_nnz; A.wts = ctx->dict.w.as<const R>();
    A.caps = sparse_caps(ctx->dict.W, packed);
    A.rl_cnt = plan.row_lists ? ctx->ws.rl_cnt.as<int>() : nullptr; A.rl_f = ctx->ws.rl_f.as<int>(); A.rl_cap = kRowListCap; A.rl_filled = ctx->rl_filled ? 1 : 0;
    A.Ts = T;
    return A;
}

template <typename Pol> static size_t policy_lds_bytes(const DevParams& P0, const typename Pol::Args& A)
{
    DevParams P = P0;
    set_segments(P, Pol::kMaxSegments);
    return Pol::total_lds_bytes(P, A);
}

// The loop of policy Pol (iterate_kernel), `signals_per_wg` signals per workgroup.  dry: only tell whether its LDS fits (kLdsLoop),
// queue nothing.  0: launched (or fits); -1: it cannot run this shape.
template <typename R, typename Pol, bool RAGGED = false, bool MULTI = false>
static int launch_policy(hscmp_ctx* ctx, const DevParams& P0, const typename Pol::Args& A, int signals_per_wg, bool dry)
{
    DevParams P = P0;
    set_segments(P, Pol::kMaxSegments);
    return launch_tile_kernel(iterate_kernel<R, Pol, RAGGED, MULTI>, dim3((P.B + signals_per_wg - 1) / signals_per_wg), dim3(signals_per_wg * kThreads),
                              Pol::total_lds_bytes(P, A), kLdsLoop, 0, dry, ctx->stream, P, make_state<R>(ctx, RAGGED, MULTI), A);
}

// LoCOMP with the re-correlations on the matrix cores (LocompMfma: single-feature float32 with a dictionary image), `group`
// signals per workgroup around one image.  -1: no such form for this shape.
template <int S4C, bool HAS_W> static int launch_locomp_mfma_t(hscmp_ctx* ctx, const DevParams& P, const MfmaArgs& A, int group, bool dry)
{
    switch (group) {
    case 4: return launch_policy<float, LocompMfma<S4C, HAS_W, 4>>(ctx, P, A, 4, dry);
    case 2: return launch_policy<float, LocompMfma<S4C, HAS_W, 2>>(ctx, P, A, 2, dry);
    default: return launch_policy<float, LocompMfma<S4C, HAS_W, 1>>(ctx, P, A, 1, dry);
    }
}
static int launch_locomp_mfma(hscmp_ctx* ctx, const DevParams& P, int group, bool dry)
{
    MfmaArgs A;
    A.dimg = ctx->dict.Dfrag.as<const float>(); A.G = mfma_groups(P.K); A.S4 = mfma_chunks(P.W); A.has_w = ctx->dict.w.p != nullptr ? 1 : 0;
    return dispatch_chunks<false>(A.S4, A.has_w != 0, [&](auto s4c, auto hw) {
        return launch_locomp_mfma_t<decltype(s4c)::value, decltype(hw)::value>(ctx, P, A, group, dry);
    });
}

// The one place that chooses the kernels of an encode: every knob that selects a kernel is looked at here, and every LDS-fit
// check runs here.  row_lists: the encode keeps per-row feature lists where its kernels can use them (use_row_lists).
// min_T: the shortest signal (a ragged batch, `ragged`; P.T otherwise).
template <typename R> static EncodePlan plan_encode(hscmp_ctx* ctx, const Knobs& kn, const DevParams& P, bool row_lists, int min_T, bool ragged = false)
{
    EncodePlan plan;
    plan.knobs = kn;
    plan.ragged = ragged;
    plan.f64 = sizeof(R) == 8;
    plan.dict_lists = ctx->dict.nzptr.p != nullptr;
    const State<R> S = make_state<R>(ctx, ragged);
    const R* dimg = ctx->dict.Dfrag.as<const R>();
    const int cus = mfma_device_cus();
    const bool locomp = ctx->method == HSCMP_METHOD_LOCOMP;      // (its loop keeps coefficient + atom per position: no score-only state)
    // Round-parallel loops for blocked rounds (HSCMP_RP=0/1 forces the choice; tests run both, the results are bit-identical).
    // Measured at the config-4 shape (profiles/r03_*): the level loops gain at every batch size (1024 signals: 28.9 -> 14.5 ms);
    // on the matrix cores the four-signal loop catches up once every CU holds four signals (1024: 117.2 vs 117.6 ms; 512: 66.0
    // vs 60.7 ms).
    const bool rp_level = P.blocked && kn.rp != 0;
    const bool rp_mfma = P.blocked && (kn.rp >= 0 ? kn.rp != 0 : P.B <= 3 * cus);
    // Sparsity-aware kernels for multi-feature inputs (hierarchical levels >= 1).  The loop only with a sparse dictionary
    // (measured: for dense single-feature windows the dense chain is 3x faster; subtracting dense atoms fills the residual, the
    // windows then overflow the gathered lists and the dense LDS-staged chain of GenericRecorr is several times faster -- a k-means
    // dictionary with ~150 of 528 non-zeros per atom: 1.3 ms vs 0.37 ms per atom).  ((f << 16) | row keys: W <= 16384, F <= 32767)
    const bool sparse_shape = ctx->dict.F > 1 && ctx->dict.Dt.p != nullptr && ctx->dict.W <= 16384 && ctx->dict.F <= 32767;
    const bool sparse_loop = sparse_shape && (ctx->dict.nzptr.p != nullptr || kn.force_gathered);
    plan.row_lists = row_lists && sparse_loop;

    // The matrix-core kernels come as a pair: the score-only state the initial correlation leaves is what the MFMA loop reads (the
    // generic / sparse kernels keep coefficient + atom instead).  The score-only path assumes single-bounce reflection at the
    // edges (T >= 3W-2; in a ragged batch every signal's: the shortest one decides).  Four signals per workgroup pay off once a CU would otherwise hold more than two signals in turn
    // (B > 2 x CUs); HSCMP_MFMA_QUAD=0/1 forces the choice (tests run both; the results are bit-identical).
    bool mf = false;
    if (!locomp && !kn.force_generic && dimg && min_T >= 3 * ctx->dict.W - 2 && mfma_launch_corr_init<R>(ctx->stream, P, S, dimg, true) == 0) {
        const bool quad = kn.mfma_quad >= 0 ? kn.mfma_quad != 0 : sizeof(R) == 4 && P.B > 2 * cus;
        if (quad && mfma_launch_iterate<R>(ctx->stream, P, S, dimg, 4, kn.lds_pad, true) == 0) plan.group = 4;
        mf = plan.group == 4 || mfma_launch_iterate<R>(ctx->stream, P, S, dimg, 1, kn.lds_pad, true) == 0;
    }
    if (mf) {
        plan.init = EncodePlan::kInitMfma;
        plan.loop = EncodePlan::kLoopMfma;
        plan.init_only = kn.init_only;
        if constexpr (sizeof(R) == 4) {
            // float32 single-arg-max encodes: the initial correlation as upper bounds on the bf16 matrix cores, refined by the loop
            // where a selection needs it (hscmp_bound.h).  HSCMP_EXACT_INIT=1: the exact pass everywhere.
            if (!P.blocked && !P.select_only && ctx->dict.Bimg.p && !kn.exact_init &&
                bound_launch_corr_init(ctx->stream, P, S, dimg, ctx->dict.Bimg.as<unsigned short>(), ctx->dict.bound_cmax, true) == 0)
                plan.init = EncodePlan::kInitBound;
            // ... and the four-signal loop re-correlates as upper bounds too, on the bf16 matrix cores (HSCMP_EXACT_RECORR=1: the
            // exact re-correlation behind the bound pass; HSCMP_EXACT_INIT=1 keeps both exact)
            if (plan.init == EncodePlan::kInitBound && plan.group == 4 && !kn.exact_recorr &&
                mfma_launch_iterate<R>(ctx->stream, P, S, dimg, 4, kn.lds_pad, true, ctx->dict.Bimg.as<unsigned short>(), ctx->dict.bound_cmax) == 0)
                plan.bound_loop = true;
            plan.rp = rp_mfma && rp_mfma_launch(ctx->stream, P, S, dimg, true) == 0;
            // The wide loop (hscmp_wide.h): a round's atoms over the whole chip, for few long signals.
            // HSCMP_WIDE=1 forces it wherever it can run, 0 forbids it.  Unset, it takes the encodes that nothing but the
            // one-atom-at-a-time loop runs today -- more candidates per round than the round-parallel workgroup holds -- while
            // the batch leaves most of the chip idle (kWideMaxBatch); a set HSCMP_RP or HSCMP_MFMA_QUAD keeps what it selects.
            const WideShape wsh = wide_shape(P, true, S.weights != nullptr, ragged, locomp);
            if (wsh.can && ctx->ws.wide.holds(wide_scratch_bytes(P.B, P.maxsel)) &&
                (kn.wide == 1 || (kn.wide < 0 && kn.rp < 0 && kn.mfma_quad < 0 && !plan.rp && wsh.by_default)) &&
                wide_launch(ctx->stream, P, S, dimg, ctx->ws.wide.as<char>(), kWideDry) == 0) {
                plan.loop = EncodePlan::kLoopWide;
                plan.rp = false; plan.group = 1; plan.bound_loop = false;
            }
        }
        return plan;
    }
    // (a dense single-feature signal is cheaper through the dense generic kernel)
    if (sparse_shape && P.T <= 262144) plan.init = EncodePlan::kInitSparse;
    if (locomp) {
        // LoCOMP on the matrix cores: its loop kernel starts with the initial correlation (LocompMfma::prologue).  Signals per
        // workgroup: as many as it takes to put the whole batch on the chip at once -- two or four around one dictionary image,
        // their tiles sharing the CU's matrix pipe (HSCMP_LOCOMP_PACK = 1 / 2 / 4 overrides).  The sparse form when its staged
        // dictionary lists fit (else the dense form runs).
        const int pack = kn.locomp_pack > 0 ? kn.locomp_pack : P.B > 2 * cus ? 4 : P.B > cus ? 2 : 1;
        if (sparse_loop && launch_policy<R, LocompSparse<R>>(ctx, P, sparse_args<R>(ctx, plan, P.T), 1, true) == 0) {
            plan.loop = EncodePlan::kLoopLocompSparse;
            plan.kept_lists = plan.row_lists;
        } else if (sizeof(R) == 4 && ctx->dict.F == 1 && dimg && !kn.locomp_no_mfma) {
            for (int g : {4, 2, 1})
                if ((pack >= g || g == 1) && launch_locomp_mfma(ctx, P, g, true) == 0) {
                    plan.init = EncodePlan::kInitOwn; plan.loop = EncodePlan::kLoopLocompMfma; plan.group = g;
                    break;
                }
        }
        if (plan.loop == EncodePlan::kLoopGeneric) plan.loop = EncodePlan::kLoopLocomp;
        return plan;
    }
    if (sparse_loop) {
        plan.loop = EncodePlan::kLoopSparse;
        plan.kept_lists = plan.row_lists;
        // small batches of blocked rounds: the round-parallel level loop (hscmp_rp_sparse.h), one wave per atom of the round
        if constexpr (sizeof(R) == 8) plan.rp = rp_level && rp_sparse_launch<R>(ctx->stream, P, S, sparse_args<R>(ctx, plan, P.T), true) == 0;
        // more signals than two per CU: the four-workgroups-per-CU form of the loop (see SparseRecorr) when its LDS fits
        if (!plan.rp)
            plan.packed = kn.sparse_packed >= 0 ? kn.sparse_packed != 0
                                                : P.B > 2 * cus && policy_lds_bytes<SparseRecorr<R, true>>(P, sparse_args<R>(ctx, plan, P.T, true)) <= (size_t)40 * 1024;
    }
    return plan;
}

// What hscmp_last_variant reports: "<init>_init+<loop>_loop_<dtype>" and the loop's form.
static std::string variant_of(const EncodePlan& plan)
{
    const bool bound = plan.init == EncodePlan::kInitBound;
    if (plan.init_only) return bound ? "bound_init" : "mfma_init";
    static const char* const inits[] = {"mfma", "mfma", "sparse", "own", "generic"};
    static const char* const loops[] = {"mfma", "gathered", "generic", "locomp", "locomp_dictlist", "locomp_mfma", "mfma"};
    const char* init = plan.init == EncodePlan::kInitSparse && plan.dict_lists ? "dictlist" : inits[plan.init];
    const char* loop = plan.loop == EncodePlan::kLoopSparse && plan.dict_lists ? "dictlist" : loops[plan.loop];
    std::string v = std::string(init) + "_init+" + loop + "_loop_" + (plan.f64 ? "f64" : "f32") + (bound ? "_bound" : "");
    if (plan.loop == EncodePlan::kLoopWide) v += "_wide";
    else if (plan.rp) v += "_rp";
    else if (plan.loop == EncodePlan::kLoopMfma && plan.group > 1) v += "_x" + std::to_string(plan.group);
    if (plan.ragged) v += "_ragged";
    if (plan.rules) v += "_rules";
    if (plan.multi) v += "_multi";
    return v;
}

// Queue the initial correlation of the plan (behind the prepare), and first the per-row lists of the input's non-zero cells
// where the loop uses them and the level chaining has not written them while it scattered.
template <typename R> static int launch_init(hscmp_ctx* ctx, const EncodePlan& plan, const DevParams& P, const void* x_dev)
{
    const State<R> S = make_state<R>(ctx, plan.ragged);
    const R* dimg = ctx->dict.Dfrag.as<const R>();
    if (plan.row_lists && !ctx->rl_filled) {
        HIP_TRY(ctx, hipMemsetAsync(ctx->ws.rl_cnt.as<int>(), 0, (size_t)P.B * P.T * sizeof(int), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(ctx->ws.rl_f.as<int>(), 0xff, (size_t)P.B * P.T * kRowListCap * sizeof(int), ctx->stream));
        const int split = std::max(1, std::min(256, 4096 / P.B));
        hipLaunchKernelGGL((build_row_lists_kernel<R>), dim3(P.B, split), dim3(kThreads), 0, ctx->stream, (const R*)x_dev, P.T, P.F,
                           ctx->ws.rl_cnt.as<int>(), ctx->ws.rl_f.as<int>(), kRowListCap, S.geom);
    }
    int rc = 0;
    switch (plan.init) {
    case EncodePlan::kInitMfma: rc = mfma_launch_corr_init<R>(ctx->stream, P, S, dimg); break;
    case EncodePlan::kInitBound:
        if constexpr (sizeof(R) == 4) rc = bound_launch_corr_init(ctx->stream, P, S, dimg, ctx->dict.Bimg.as<unsigned short>(), ctx->dict.bound_cmax);
        break;
    case EncodePlan::kInitSparse: {
        const SparseArgs<R> A = sparse_args<R>(ctx, plan, P.T);
        const size_t lds = sparse_lds_bytes<R>(A.caps) + staged_dict_bytes(P, A) + (size_t)((P.T + 31) / 32) * sizeof(unsigned);
        auto kern = plan.ragged ? corr_init_sparse_kernel<R, true> : corr_init_sparse_kernel<R, false>;
        HIP_TRY(ctx, set_dyn_lds((const void*)kern, lds));
        hipLaunchKernelGGL(kern, dim3(P.B, sparse_init_split(P.B, P.T, P.W)), dim3(kThreads), lds, ctx->stream, P, S, A);
        break;
    }
    case EncodePlan::kInitOwn: break;
    case EncodePlan::kInitGeneric:
        if (plan.multi)
            hipLaunchKernelGGL((corr_init_generic_kernel<R, false, true>), dim3((P.T + kThreads - 1) / kThreads, P.B), dim3(kThreads), 0, ctx->stream,
                               P, make_state<R>(ctx, false, true), ctx->ws.resid.as<const R>(), P.off, P.T, (R*)nullptr);
        else
            hipLaunchKernelGGL((corr_init_generic_kernel<R, false>), dim3((P.T + kThreads - 1) / kThreads, P.B), dim3(kThreads), 0, ctx->stream,
                               P, S, ctx->ws.resid.as<const R>(), P.off, P.T, (R*)nullptr);
        break;
    }
    if (rc != 0) return fail(ctx, HSCMP_ERR_HIP, "the initial correlation of %s could not be launched", variant_of(plan).c_str());
    return HSCMP_OK;
}

// The wide loop (hscmp_wide.h): the start of the call, then steps of four launches -- control, subtract, re-correlate, candidates --
// queued kWideStepsPerPoll at a time; behind each batch of steps the control blocks are read (one small copy; the stream is
// waited for), until every signal has stopped or run its max_rounds.  Steps queued past that point find no work.
static int wide_loop(hscmp_ctx* ctx, const EncodePlan& plan, const DevParams& P)
{
    const State<float> S = make_state<float>(ctx, false);
    const float* dimg = ctx->dict.Dfrag.as<const float>();
    char* wbuf = ctx->ws.wide.as<char>();
    if (!ctx->ws.wide.holds(wide_scratch_bytes(P.B, P.maxsel)))
        return fail(ctx, HSCMP_ERR_STATE, "the loop of %s has no workspace", variant_of(plan).c_str());
    HIP_TRY(ctx, hipMemsetAsync(S.head, 0xff, (size_t)P.B * P.T * sizeof(int), ctx->stream));
    if (wide_launch(ctx->stream, P, S, dimg, wbuf, kWideBegin) != 0)
        return fail(ctx, HSCMP_ERR_HIP, "the loop of %s could not be launched", variant_of(plan).c_str());
    std::vector<int> ctl((size_t)P.B * WC_COUNT);
    ctx->wide_steps = 0; ctx->wide_polls = 0; ctx->wide_worked = 0;
    for (;;) {
        for (int s = 0; s < kWideStepsPerPoll; ++s)
            if (wide_launch(ctx->stream, P, S, dimg, wbuf, kWideStep) != 0)
                return fail(ctx, HSCMP_ERR_HIP, "the loop of %s could not be launched", variant_of(plan).c_str());
        ctx->wide_steps += kWideStepsPerPoll; ctx->wide_polls += 1;
        HIP_TRY(ctx, hipGetLastError());
        HIP_TRY(ctx, hipMemcpyAsync(ctl.data(), wbuf, ctl.size() * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        bool done = true;
        int worked = 0;
        for (int b = 0; b < P.B; ++b) { done = done && ctl[(size_t)b * WC_COUNT + WC_DONE] != 0; worked += ctl[(size_t)b * WC_COUNT + WC_STEPS]; }
        // (every step of a running signal applies atoms or ends a round: a batch of steps without any is a fault, not a wait)
        if (!done && worked == ctx->wide_worked)
            return fail(ctx, HSCMP_ERR_HIP, "the loop of %s made no progress in %d steps", variant_of(plan).c_str(), kWideStepsPerPoll);
        ctx->wide_worked = worked;
        if (done) break;
    }
    return HSCMP_OK;
}

// Queue the loop of the plan: run_encode behind the initial correlation, hscmp_continue on the state an earlier launch left.
template <typename R> static int launch_loop(hscmp_ctx* ctx, const EncodePlan& plan, const DevParams& P)
{
    const R* dimg = ctx->dict.Dfrag.as<const R>();
    int rc = -1;
    switch (plan.loop) {
    case EncodePlan::kLoopMfma:
        if constexpr (sizeof(R) == 4)
            if (plan.rp) { rc = rp_mfma_launch(ctx->stream, P, make_state<float>(ctx, plan.ragged), dimg); break; }
        rc = mfma_launch_iterate<R>(ctx->stream, P, make_state<R>(ctx, plan.ragged), dimg, plan.group, plan.knobs.lds_pad, false,
                                    plan.bound_loop ? ctx->dict.Bimg.as<unsigned short>() : nullptr, ctx->dict.bound_cmax);
        break;
    case EncodePlan::kLoopSparse:
        if constexpr (sizeof(R) == 8)
            if (plan.rp) { rc = rp_sparse_launch<R>(ctx->stream, P, make_state<R>(ctx, plan.ragged), sparse_args<R>(ctx, plan, P.T), false); break; }
        if (plan.ragged)
            rc = plan.packed ? launch_policy<R, SparseRecorr<R, true, true>, true>(ctx, P, sparse_args<R>(ctx, plan, P.T, true), 1, false)
                             : launch_policy<R, SparseRecorr<R, false, true>, true>(ctx, P, sparse_args<R>(ctx, plan, P.T), 1, false);
        else
            rc = plan.packed ? launch_policy<R, SparseRecorr<R, true>>(ctx, P, sparse_args<R>(ctx, plan, P.T, true), 1, false)
                             : launch_policy<R, SparseRecorr<R, false>>(ctx, P, sparse_args<R>(ctx, plan, P.T), 1, false);
        break;
    case EncodePlan::kLoopGeneric:
        rc = plan.multi    ? launch_policy<R, GenericRecorr<R>, false, true>(ctx, P, {}, 1, false)
             : plan.ragged ? launch_policy<R, GenericRecorr<R>, true>(ctx, P, {}, 1, false)
                           : launch_policy<R, GenericRecorr<R>>(ctx, P, {}, 1, false);
        break;
    case EncodePlan::kLoopLocomp:
        rc = plan.multi ? launch_policy<R, LocompRecorr<R>, false, true>(ctx, P, {}, 1, false) : launch_policy<R, LocompRecorr<R>>(ctx, P, {}, 1, false);
        break;
    case EncodePlan::kLoopLocompSparse: rc = launch_policy<R, LocompSparse<R>>(ctx, P, sparse_args<R>(ctx, plan, P.T), 1, false); break;
    case EncodePlan::kLoopLocompMfma:
        if constexpr (sizeof(R) == 4) rc = launch_locomp_mfma(ctx, P, plan.group, false);
        break;
    case EncodePlan::kLoopWide:
        if constexpr (sizeof(R) == 4) return wide_loop(ctx, plan, P);
        break;
    }
    if (rc != 0) return fail(ctx, HSCMP_ERR_HIP, "the loop of %s could not be launched", variant_of(plan).c_str());
    return HSCMP_OK;
}

// Slots of the previous level an input was scattered from (level chaining): the input then already sits in the
// residual buffer and prepare only needs the energy.
struct ChainSource { const int* slot_t; const int* slot_k; const double* slot_a; const int* stats; int cap, first, has_min; double minc; bool lists; int max_slots; };

// The batch an encode has just queued becomes the context's: everything hscmp_continue, the fetches and the epilogue go by, at once.
static void commit_batch(hscmp_ctx* ctx, const EncodePlan& plan, const DevParams& P, const hscmp_params& params, const void* x_dev, std::vector<int>&& geom)
{
    ctx->P = P; ctx->P.bound_init = plan.init == EncodePlan::kInitBound ? 1 : 0;     // (the loop read it: hscmp_continue resumes on the same state)
    ctx->plan = plan; ctx->last = params; ctx->B = P.B; ctx->T = P.T; ctx->cap = P.cap; ctx->maxsel = P.maxsel;
    ctx->last_x_dev = x_dev;
    ctx->ragged = plan.ragged; ctx->geom = std::move(geom);
    ctx->have_batch = true;
}

template <typename R>
static int run_encode(hscmp_ctx* ctx, const EncodePlan& plan, const DevParams& P, const void* x_dev, const ChainSource* chain = nullptr)
{
    State<R> S = make_state<R>(ctx, plan.ragged);
    HIP_TRY(ctx, hipEventRecord(ctx->ev[0], ctx->stream));
    if (chain) {
        // long slot lists: counting sort in LDS when a word per slot fits (cell index / 256 and slot number in 32 bits)
        int ibits = 1;
        while ((1 << ibits) < std::max(2, chain->max_slots)) ++ibits;
        const long long cells256 = ((long long)P.T * P.F + 255) >> 8;
        const size_t lds = (size_t)std::max(1, chain->max_slots) * sizeof(unsigned);
        const bool sorted = chain->max_slots > plan.knobs.sorted_prepare_min && lds <= (size_t)150 * 1024 && ibits < 31 &&
                            cells256 < (1ll << (32 - ibits)) && !plan.knobs.no_sorted_prepare &&
                            set_dyn_lds((const void*)prepare_from_slots_sorted_kernel<R>, lds) == hipSuccess;
        if (sorted)
            hipLaunchKernelGGL((prepare_from_slots_sorted_kernel<R>), dim3(P.B), dim3(kThreads), lds, ctx->stream, P, S, chain->slot_t, chain->slot_k,
                               chain->slot_a, chain->stats, chain->cap, chain->first, chain->has_min, chain->minc, ibits);
        else
            hipLaunchKernelGGL((prepare_from_slots_kernel<R>), dim3(P.B), dim3(kThreads), 0, ctx->stream, P, S, chain->slot_t, chain->slot_k,
                               chain->slot_a, chain->stats, chain->cap, chain->first, chain->has_min, chain->minc,
                               chain->lists ? ctx->ws.rl_cnt.as<int>() : nullptr, ctx->ws.rl_f.as<int>(), kRowListCap);
    } else
        hipLaunchKernelGGL((prepare_kernel<R>), dim3(P.B), dim3(kThreads), 0, ctx->stream, P, S, (const R*)x_dev);
    HIP_TRY(ctx, hipEventRecord(ctx->ev[1], ctx->stream));
    int rc = launch_init<R>(ctx, plan, P, x_dev);
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(ctx->ev[2], ctx->stream));
    if (!plan.init_only) {          // (HSCMP_INIT_ONLY: best_c / best_k of the initial correlation through hscmp_get_device_view)
        DevParams PL = P;
        PL.bound_init = plan.init == EncodePlan::kInitBound ? 1 : 0;
        if ((rc = launch_loop<R>(ctx, plan, PL))) return rc;
    }
    HIP_TRY(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
    HIP_TRY(ctx, hipGetLastError());
    ctx->timed = true; ctx->timed_loop_only = false;
    ctx->variant = variant_of(plan);
    return HSCMP_OK;
}

// Per-signal geometry of a ragged batch, checked before anything is queued: {T_b, bs_b, nbk_b} per signal with the block size
// of modeling.py:908-918 on the signal's own length; P.maxsel grows to the largest block count.  *min_T: the shortest length.
static int ragged_geometry(hscmp_ctx* ctx, const char* who, int B, int T, const int32_t* lengths, const hscmp_params* p, DevParams& P,
                           std::vector<int>& geom, int* min_T)
{
    geom.assign((size_t)B * kGeomWords, 0);
    *min_T = T;
    for (int b = 0; b < B; ++b) {
        const int Tb = lengths[b];
        if (Tb < ctx->dict.W || Tb > T)
            return fail(ctx, HSCMP_ERR_INVALID, "%s: signal %d has length %d outside [W=%d, T=%d]", who, b, Tb, ctx->dict.W, T);
        int bs = 0, nbk = 0;
        if (P.blocked) {
            bs = p->nb_blocks < 0 ? 4 * ctx->dict.W : (int)std::floor((double)Tb / (double)p->nb_blocks);
            if (bs % 2 == 1) bs += 1;
            if (bs <= 0) return fail(ctx, HSCMP_ERR_INVALID, "%s: signal %d: nbBlocks=%d gives an empty block for its length %d", who, b, p->nb_blocks, Tb);
            nbk = (int)std::ceil((double)Tb / (double)bs);
            P.maxsel = std::max(P.maxsel, nbk + 1);
        }
        geom[(size_t)b * kGeomWords + 0] = Tb;
        geom[(size_t)b * kGeomWords + 1] = bs;
        geom[(size_t)b * kGeomWords + 2] = nbk;
        *min_T = std::min(*min_T, Tb);
    }
    return HSCMP_OK;
}

// lengths: NULL for a uniform batch, else host int32 [B] (hscmp_encode_batch_ragged*); rules: NULL, or the [B] table of a ragged
// batch with stop rules per signal (hscmp_encode_batch_rules*: params then says which rules exist, the table their values)
static int encode_common(hscmp_ctx* ctx, const void* x, bool host, int B, int T, const hscmp_params* params, const int32_t* lengths = nullptr,
                         const char* who = "hscmp_encode_batch", std::vector<SignalRule>* rules = nullptr)
{
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, "%s: ctx is NULL", who);
    if (ctx->dict.dtype < 0) return fail(ctx, HSCMP_ERR_STATE, "%s: no dictionary set", who);
    NOT_A_SET(ctx, who);
    if (!x || !params || B <= 0 || T <= 0) return fail(ctx, HSCMP_ERR_INVALID, "%s: bad arguments (B=%d T=%d)", who, B, T);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const Knobs kn = read_knobs();
    DevParams P;
    int rc = make_params(ctx, kn, B, T, params, &P);
    if (rc) return rc;
    int min_T = T;
    std::vector<int> geom;
    if (lengths && (rc = ragged_geometry(ctx, who, B, T, lengths, params, P, geom, &min_T))) return rc;
    const bool row_lists = use_row_lists(ctx, kn);
    drop_batch(ctx);
    if (rules) ctx->rules = std::move(*rules);      // (from here on make_state hands the table to the RAGGED instances)
    if ((rc = ensure_workspace(ctx, P, host, row_lists, geom.size() * sizeof(int), ctx->rules.size() * sizeof(SignalRule)))) return rc;
    EncodePlan plan = ctx->dict.dtype == HSCMP_F32 ? plan_encode<float>(ctx, kn, P, row_lists, min_T, lengths != nullptr)
                                                   : plan_encode<double>(ctx, kn, P, row_lists, min_T, lengths != nullptr);
    plan.rules = !ctx->rules.empty();
    // (every CMP plan has its ragged form, DESIGN.md sections 15 and 21; the LoCOMP loops have none -- encode_ragged refuses them first)
    if (plan.ragged && plan.loop != EncodePlan::kLoopMfma && plan.loop != EncodePlan::kLoopGeneric && plan.loop != EncodePlan::kLoopSparse)
        return fail(ctx, HSCMP_ERR_UNSUPPORTED, "%s: %s has no ragged form (the LoCOMP loops)", who, variant_of(plan).c_str());
    if (lengths) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // (the previous batch's kernels may still read the old geometry)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->ws.geom.p, geom.data(), geom.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        if (plan.rules)     // (behind the same wait; the context keeps the host table, so the upload may still read it)
            HIP_TRY(ctx, hipMemcpyAsync(ctx->ws.rules.p, ctx->rules.data(), ctx->rules.size() * sizeof(SignalRule), hipMemcpyHostToDevice, ctx->stream));
    }
    const void* xd = x;
    if (host) {
        HIP_TRY(ctx, hipMemcpyAsync(ctx->ws.x.p, x, (size_t)B * T * ctx->dict.F * esize(ctx->dict.dtype), hipMemcpyHostToDevice, ctx->stream));
        xd = ctx->ws.x.p;
    }
    ctx->listed_rows = 0;                       // the residual buffer is overwritten with a dense input
    rc = ctx->dict.dtype == HSCMP_F32 ? run_encode<float>(ctx, plan, P, xd) : run_encode<double>(ctx, plan, P, xd);
    if (rc) return rc;
    commit_batch(ctx, plan, P, *params, xd, std::move(geom));      // (geom keeps its storage: the upload above may still read it)
    if (host) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return HSCMP_OK;
}

extern "C" int hscmp_encode_batch(hscmp_ctx* ctx, const void* x, int B, int T, const hscmp_params* params)
{
    return encode_common(ctx, x, true, B, T, params);
}

extern "C" int hscmp_encode_batch_device(hscmp_ctx* ctx, const void* x_dev, int B, int T, const hscmp_params* params)
{
    return encode_common(ctx, x_dev, false, B, T, params);
}

// A batch encoded with a dictionary per signal out of the context's set: the generic pair alone -- prepare,
// the generic initial correlation and the generic loop (CMP) or the dense LoCOMP loop, in their MULTI instances -- so there is
// nothing to choose and the plan is written down here.  Signal b comes out as hscmp_encode_batch would return it alone on a context
// whose dictionary is dictionary dict_of[b].
template <typename R> static int multi_loop_fits(hscmp_ctx* ctx, const EncodePlan& plan, const DevParams& P)
{
    return plan.loop == EncodePlan::kLoopLocomp ? launch_policy<R, LocompRecorr<R>, false, true>(ctx, P, {}, 1, true)
                                                : launch_policy<R, GenericRecorr<R>, false, true>(ctx, P, {}, 1, true);
}

extern "C" int hscmp_encode_batch_multi(hscmp_ctx* ctx, const void* x, int B, int T, const int32_t* dict_of, const hscmp_params* params)
{
    const char* who = "hscmp_encode_batch_multi";
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, "%s: ctx is NULL", who);
    if (ctx->dict.dtype < 0) return fail(ctx, HSCMP_ERR_STATE, "%s: no dictionary set", who);
    if (ctx->dict.G <= 0)
        return fail(ctx, HSCMP_ERR_STATE, "%s: the context holds one dictionary (hscmp_set_dictionary), not a set (hscmp_set_dictionaries)", who);
    if (!x || !params || !dict_of || B <= 0 || T <= 0) return fail(ctx, HSCMP_ERR_INVALID, "%s: bad arguments (B=%d T=%d)", who, B, T);
    for (int b = 0; b < B; ++b)
        if (dict_of[b] < 0 || dict_of[b] >= ctx->dict.G)
            return fail(ctx, HSCMP_ERR_INVALID, "%s: signal %d asks for dictionary %d outside [0, G=%d)", who, b, (int)dict_of[b], ctx->dict.G);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const Knobs kn = read_knobs();
    DevParams P;
    int rc = make_params(ctx, kn, B, T, params, &P);
    if (rc) return rc;
    const bool f64 = ctx->dict.dtype == HSCMP_F64;
    EncodePlan plan;
    plan.knobs = kn;
    plan.f64 = f64;
    plan.multi = true;
    plan.init = EncodePlan::kInitGeneric;
    plan.loop = ctx->method == HSCMP_METHOD_LOCOMP ? EncodePlan::kLoopLocomp : EncodePlan::kLoopGeneric;
    if ((f64 ? multi_loop_fits<double>(ctx, plan, P) : multi_loop_fits<float>(ctx, plan, P)) != 0)
        return fail(ctx, HSCMP_ERR_UNSUPPORTED, "%s: the loop of %s does not fit this shape", who, variant_of(plan).c_str());
    drop_batch(ctx);
    // (no sparsity-aware kernel runs: none of their buffers is asked for)
    if ((rc = ensure_workspace_g(ctx, P, true, esize(ctx->dict.dtype), false, false))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));         // (the previous batch's kernels may still read the old dict_of)
    const size_t dbytes = (size_t)B * sizeof(int);
    const hipError_t e = ctx->ws.dict_of.replace(dbytes);
    if (e != hipSuccess) return alloc_failed(ctx, dbytes, e);
    HIP_TRY(ctx, hipMemcpy(ctx->ws.dict_of.p, dict_of, dbytes, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpyAsync(ctx->ws.x.p, x, (size_t)B * T * ctx->dict.F * esize(ctx->dict.dtype), hipMemcpyHostToDevice, ctx->stream));
    ctx->listed_rows = 0;                       // the residual buffer is overwritten with a dense input
    rc = f64 ? run_encode<double>(ctx, plan, P, ctx->ws.x.p) : run_encode<float>(ctx, plan, P, ctx->ws.x.p);
    if (rc) return rc;
    commit_batch(ctx, plan, P, *params, ctx->ws.x.p, std::vector<int>());     // (plan.multi and ws.dict_of stay: hscmp_continue resumes with them)
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return HSCMP_OK;
}

static int encode_ragged(hscmp_ctx* ctx, const void* x, bool host, int B, int T, const int32_t* lengths, const hscmp_params* params, const char* who)
{
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, "%s: ctx is NULL", who);
    NOT_A_SET(ctx, who);
    if (B < 1) return fail(ctx, HSCMP_ERR_INVALID, "%s: B=%d, at least one signal is needed", who, B);
    if (!lengths) return fail(ctx, HSCMP_ERR_INVALID, "%s: lengths is NULL", who);
    if (ctx->method == HSCMP_METHOD_LOCOMP) return fail(ctx, HSCMP_ERR_UNSUPPORTED, "%s: the LoCOMP loop has no ragged form", who);
    return encode_common(ctx, x, host, B, T, params, lengths, who);
}

extern "C" int hscmp_encode_batch_ragged(hscmp_ctx* ctx, const void* x, int B, int T, const int32_t* lengths, const hscmp_params* params)
{
    return encode_ragged(ctx, x, true, B, T, lengths, params, "hscmp_encode_batch_ragged");
}

extern "C" int hscmp_encode_batch_ragged_device(hscmp_ctx* ctx, const void* x_dev, int B, int T, const int32_t* lengths, const hscmp_params* params)
{
    return encode_ragged(ctx, x_dev, false, B, T, lengths, params, "hscmp_encode_batch_ragged_device");
}

// The two refusals every call with a rules table starts with.  plain: the call that encodes the same batch without a table.
static int rules_refused(hscmp_ctx* ctx, const char* who, const char* plain, const hscmp_signal_rules* rules)
{
    if (!rules || (!rules->nb_nonzero_coefs && !rules->tolerance_snr && !rules->tolerance_residual_scale))
        return fail(ctx, HSCMP_ERR_INVALID, "%s: no rule has an array: use %s", who, plain);
    if (ctx->method == HSCMP_METHOD_LOCOMP) return fail(ctx, HSCMP_ERR_UNSUPPORTED, "%s: the LoCOMP loop has no per-signal stop rules", who);
    return HSCMP_OK;
}

// The [B] table of a rules batch from the caller's arrays (entry b: signal b of the batch being encoded), and in `pe` the params
// that say which rules exist: the one place that owns the table's expressions and the messages about its values.
static int rules_table(hscmp_ctx* ctx, const char* who, int B, const hscmp_signal_rules* rules, hscmp_params& pe, std::vector<SignalRule>& table)
{
    // (the rules without an array: make_params_g's expressions on the scalars)
    const SignalRule scalars{std::isnan(pe.tolerance_snr) ? 0.0 : std::pow(10.0, pe.tolerance_snr / 10.0),
                             std::isnan(pe.tolerance_residual_scale) ? 0.0 : pe.tolerance_residual_scale,
                             pe.nb_nonzero_coefs < 0 ? -1 : pe.nb_nonzero_coefs, 0};
    table.assign((size_t)B, scalars);
    if (rules->nb_nonzero_coefs) {
        pe.nb_nonzero_coefs = 0;        // (present; P.l0 becomes the largest, which no kernel reads behind signal_params)
        for (int b = 0; b < B; ++b) {
            const int32_t l0 = rules->nb_nonzero_coefs[b];
            if (l0 < 0) return fail(ctx, HSCMP_ERR_INVALID, "%s: signal %d: nb_nonzero_coefs is %d, it must be >= 0", who, b, (int)l0);
            table[(size_t)b].l0 = l0;
            pe.nb_nonzero_coefs = std::max(pe.nb_nonzero_coefs, l0);
        }
    }
    if (rules->tolerance_snr) {
        for (int b = 0; b < B; ++b) {
            const double v = rules->tolerance_snr[b];
            if (std::isnan(v) || v < 0.0) return fail(ctx, HSCMP_ERR_INVALID, "%s: signal %d: tolerance_snr is %g, it must be >= 0", who, b, v);
            table[(size_t)b].snr_ratio = std::pow(10.0, v / 10.0);          // (make_params_g's expression: the same bits)
        }
        pe.tolerance_snr = rules->tolerance_snr[0];
    }
    if (rules->tolerance_residual_scale) {
        for (int b = 0; b < B; ++b) {
            const double v = rules->tolerance_residual_scale[b];
            if (std::isnan(v) || v < 0.0)
                return fail(ctx, HSCMP_ERR_INVALID, "%s: signal %d: tolerance_residual_scale is %g, it must be >= 0", who, b, v);
            table[(size_t)b].tol_scale = v;
        }
        pe.tolerance_residual_scale = rules->tolerance_residual_scale[0];
    }
    return HSCMP_OK;
}

// Stop rules per signal: a ragged batch (a uniform one: every length T) plus a [B] table of the rules' values.
// A rule with an array exists for every signal and its scalar in `params` is not read; a rule without one stays what `params`
// says, for every signal.  Everything is checked before anything is queued, so a refusal leaves the previous batch as it was.
static int encode_rules(hscmp_ctx* ctx, const void* x, bool host, int B, int T, const int32_t* lengths, const hscmp_signal_rules* rules,
                        const hscmp_params* params, const char* who)
{
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, "%s: ctx is NULL", who);
    NOT_A_SET(ctx, who);
    int rc = rules_refused(ctx, who, "hscmp_encode_batch_ragged", rules);
    if (rc) return rc;
    if (B < 1 || T < 1 || !params) return fail(ctx, HSCMP_ERR_INVALID, "%s: bad arguments (B=%d T=%d)", who, B, T);
    hscmp_params pe = *params;
    std::vector<SignalRule> table;
    if ((rc = rules_table(ctx, who, B, rules, pe, table))) return rc;
    const std::vector<int32_t> all_T(lengths ? (size_t)0 : (size_t)B, T);
    rc = encode_common(ctx, x, host, B, T, &pe, lengths ? lengths : all_T.data(), who, &table);
    if (rc && !ctx->have_batch) ctx->rules.clear();     // (a refusal in front of drop_batch leaves the previous batch and ITS table)
    return rc;
}

extern "C" int hscmp_encode_batch_rules(hscmp_ctx* ctx, const void* x, int B, int T, const int32_t* lengths, const hscmp_signal_rules* rules,
                                        const hscmp_params* params)
{
    return encode_rules(ctx, x, true, B, T, lengths, rules, params, "hscmp_encode_batch_rules");
}

extern "C" int hscmp_encode_batch_rules_device(hscmp_ctx* ctx, const void* x_dev, int B, int T, const int32_t* lengths, const hscmp_signal_rules* rules,
                                               const hscmp_params* params)
{
    return encode_rules(ctx, x_dev, false, B, T, lengths, rules, params, "hscmp_encode_batch_rules_device");
}

// rules: NULL, or the caller's table for signals [first, first + count) of prev (hscmp_encode_batch_from_level_rules): the level is
// then encoded as a ragged batch with the table, as encode_rules encodes a level 0 -- a uniform prev with every length T.
static int from_level_common(hscmp_ctx* ctx, hscmp_ctx* prev, int first, int count, double min_coefficients, const hscmp_signal_rules* rules,
                             bool with_rules, const hscmp_params* params_in, const char* who)
{
    if (!ctx || !prev) return fail(ctx, HSCMP_ERR_INVALID, "%s: NULL context", who);
    NOT_A_SET(ctx, who);
    if (prev->dict.G > 0) return fail(ctx, HSCMP_ERR_STATE, "%s: the previous level holds a set of dictionaries (hscmp_set_dictionaries)", who);
    if (ctx->dict.dtype != HSCMP_F64) return fail(ctx, HSCMP_ERR_STATE, "%s: the level dictionary must be float64", who);
    if (!prev->have_batch) return fail(ctx, HSCMP_ERR_STATE, "%s: the previous level has no results", who);
    if (ctx->device != prev->device) return fail(ctx, HSCMP_ERR_INVALID, "%s: contexts on different GPUs", who);
    if (ctx->dict.F != prev->dict.K) return fail(ctx, HSCMP_ERR_INVALID, "%s: F=%d of this level != K=%d of the previous one", who, ctx->dict.F, prev->dict.K);
    if (!params_in || first < 0 || count <= 0 || first + count > prev->B) return fail(ctx, HSCMP_ERR_INVALID, "%s: bad signal range", who);
    int rc;
    hscmp_params pe = *params_in;               // (with a table: which rules exist, as encode_rules hands them to encode_common)
    const hscmp_params* const params = &pe;
    std::vector<SignalRule> table;
    if (with_rules) {
        if ((rc = rules_refused(ctx, who, "hscmp_encode_batch_from_level", rules))) return rc;
        if ((rc = rules_table(ctx, who, count, rules, pe, table))) return rc;
    }
    const bool ragged = prev->ragged || with_rules;
    if (ragged && ctx->method == HSCMP_METHOD_LOCOMP)
        return fail(ctx, HSCMP_ERR_UNSUPPORTED, "%s: the previous level holds a ragged batch, and the LoCOMP loop has no ragged form", who);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(prev->stream));           // the previous level's results are final
    const int T = prev->T;
    const Knobs kn = read_knobs();
    DevParams P;
    if ((rc = make_params(ctx, kn, count, T, params, &P))) return rc;
    // a ragged previous level: the lengths are its signals', the block geometry this level's (its W and nbBlocks); a uniform one
    // under a table: every length T
    int min_T = T;
    std::vector<int> geom;
    if (ragged) {
        std::vector<int32_t> lens((size_t)count, T);
        for (int i = 0; prev->ragged && i < count; ++i) lens[(size_t)i] = prev->geom[(size_t)(first + i) * kGeomWords];
        if ((rc = ragged_geometry(ctx, who, count, T, lens.data(), params, P, geom, &min_T))) return rc;
    }
    const bool row_lists = use_row_lists(ctx, kn);
    drop_batch(ctx);                            // (this level's batch; prev is only read)
    ctx->rules = std::move(table);              // (empty without a table; from here on make_state hands it to the RAGGED instances)
    // no input buffer: the slots are scattered straight into the residual
    if ((rc = ensure_workspace(ctx, P, false, row_lists, geom.size() * sizeof(int), ctx->rules.size() * sizeof(SignalRule)))) return rc;
    EncodePlan plan = plan_encode<double>(ctx, kn, P, row_lists, min_T, ragged);
    plan.rules = !ctx->rules.empty();
    if (ragged) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));     // (the previous batch's kernels may still read the old geometry)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->ws.geom.p, geom.data(), geom.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream));
        if (plan.rules)     // (behind the same wait; the context keeps the host table, so the upload may still read it)
            HIP_TRY(ctx, hipMemcpyAsync(ctx->ws.rules.p, ctx->rules.data(), ctx->rules.size() * sizeof(SignalRule), hipMemcpyHostToDevice, ctx->stream));
    }
    const bool lists = plan.row_lists;          // (the scatter writes them)
    const size_t bytes = (size_t)count * T * ctx->dict.F * sizeof(double);
    if (ctx->listed_rows > 0 && ctx->listed_F == ctx->dict.F && !kn.no_lazy_clear) {
        // the buffer still holds the previous chained batch; its lists say where
        hipLaunchKernelGGL((clear_listed_cells_kernel<double>), dim3((unsigned)((ctx->listed_rows + kThreads - 1) / kThreads)), dim3(kThreads), 0, ctx->stream,
                           ctx->ws.resid.as<double>(), ctx->listed_rows, ctx->dict.F, ctx->ws.rl_cnt.as<int>(), ctx->ws.rl_f.as<int>(), kRowListCap);
        const size_t covered = (size_t)ctx->listed_rows * ctx->dict.F * sizeof(double);
        if (bytes > covered) HIP_TRY(ctx, hipMemsetAsync(ctx->ws.resid.as<char>() + covered, 0, bytes - covered, ctx->stream));
    } else {
        HIP_TRY(ctx, hipMemsetAsync(ctx->ws.resid.p, 0, bytes, ctx->stream));
    }
    ctx->listed_rows = 0;
    HIP_TRY(ctx, hipMemsetAsync(ctx->ws.rowflag.as<unsigned char>(), 0, (size_t)count * T, ctx->stream));
    if (lists) {
        HIP_TRY(ctx, hipMemsetAsync(ctx->ws.rl_cnt.as<int>(), 0, (size_t)count * T * sizeof(int), ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(ctx->ws.rl_f.as<int>(), 0xff, (size_t)count * T * kRowListCap * sizeof(int), ctx->stream));
    }
    const int has_min = !std::isnan(min_coefficients);
    hipLaunchKernelGGL((scatter_slots_kernel<double>), dim3(count), dim3(kThreads), 0, ctx->stream, ctx->ws.resid.as<double>(), T, ctx->dict.F,
                       prev->ws.slot_t.as<int>(), prev->ws.slot_k.as<int>(), prev->ws.slot_a.as<double>(), prev->ws.stats.as<int>(), prev->cap, first, has_min,
                       has_min ? min_coefficients : 0.0, ctx->ws.rowflag.as<unsigned char>(), lists ? ctx->ws.rl_cnt.as<int>() : nullptr, ctx->ws.rl_f.as<int>(), kRowListCap);
    ctx->rowflag_valid = true;                  // the sparse initial correlation skips its scan of the dense input
    ctx->rl_filled = lists;
    // (the longest slot list of the range sizes the LDS of the energy kernel: the previous level's counters are final)
    int max_slots = 0;
    {
        std::vector<int> pst((size_t)count * ST_COUNT);
        HIP_TRY(ctx, hipMemcpy(pst.data(), prev->ws.stats.as<int>() + (size_t)first * ST_COUNT, pst.size() * sizeof(int), hipMemcpyDeviceToHost));
        for (int i = 0; i < count; ++i) max_slots = std::max(max_slots, pst[(size_t)i * ST_COUNT + ST_SLOTS]);
    }
    const ChainSource chain{prev->ws.slot_t.as<int>(), prev->ws.slot_k.as<int>(), prev->ws.slot_a.as<double>(), prev->ws.stats.as<int>(), prev->cap, first, has_min,
                            has_min ? min_coefficients : 0.0, lists, max_slots};
    rc = run_encode<double>(ctx, plan, P, ctx->ws.resid.p, &chain);
    ctx->rowflag_valid = false; ctx->rl_filled = false;
    if (rc) return rc;
    commit_batch(ctx, plan, P, *params, nullptr, std::move(geom));      // (no input of its own on the device: the slots were scattered)
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    // (only now: a failed launch leaves the buffer in an unknown state, and so does any other writer -- see the resets)
    if (plan.kept_lists) { ctx->listed_rows = (int64_t)count * T; ctx->listed_F = ctx->dict.F; }
    return HSCMP_OK;
}

extern "C" int hscmp_encode_batch_from_level(hscmp_ctx* ctx, hscmp_ctx* prev, int first, int count, double min_coefficients,
                                             const hscmp_params* params)
{
    return from_level_common(ctx, prev, first, count, min_coefficients, nullptr, false, params, "hscmp_encode_batch_from_level");
}

extern "C" int hscmp_encode_batch_from_level_rules(hscmp_ctx* ctx, hscmp_ctx* prev, int first, int count, double min_coefficients,
                                                   const hscmp_signal_rules* rules, const hscmp_params* params)
{
    const int rc = from_level_common(ctx, prev, first, count, min_coefficients, rules, true, params, "hscmp_encode_batch_from_level_rules");
    if (rc && ctx && !ctx->have_batch) ctx->rules.clear();      // (a failure behind drop_batch: no batch, so no table either)
    return rc;
}

// hscmp_load_level: the validation pass reads only the staged entries, so a rejected entry is known before anything of the
// context changes; the buffers of the batch are replaced behind it, as an encode replaces them.
// lengths: NULL for a uniform batch, else host int32 [B] (hscmp_load_level_ragged): an entry's row must lie below its signal's length
static int load_level_common(hscmp_ctx* ctx, const void* x, int B, int T, const int32_t* lengths, const int64_t* offsets, const int32_t* rows,
                             const int32_t* cols, const double* data, const char* who)
{
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, "%s: ctx is NULL", who);
    if (ctx->dict.dtype < 0) return fail(ctx, HSCMP_ERR_STATE, "%s: no dictionary set", who);
    NOT_A_SET(ctx, who);
    if (B <= 0 || T <= 0 || !offsets) return fail(ctx, HSCMP_ERR_INVALID, "%s: bad arguments (B=%d T=%d)", who, B, T);
    if (lengths)
        for (int b = 0; b < B; ++b)
            if (lengths[b] < 1 || lengths[b] > T) return fail(ctx, HSCMP_ERR_INVALID, "%s: signal %d has length %d outside [1, T=%d]", who, b, (int)lengths[b], T);
    if (offsets[0] != 0) return fail(ctx, HSCMP_ERR_INVALID, "%s: offsets[0] is %lld, not 0", who, (long long)offsets[0]);
    long long longest = 0;
    for (int b = 0; b < B; ++b) {
        if (offsets[b + 1] < offsets[b]) return fail(ctx, HSCMP_ERR_INVALID, "%s: signal %d: offsets decrease", who, b);
        longest = std::max<long long>(longest, offsets[b + 1] - offsets[b]);
    }
    const long long n = offsets[B];
    if (longest > (long long)T * ctx->dict.K || longest >= (1ll << 30))
        return fail(ctx, HSCMP_ERR_INVALID, "%s: a list of %lld entries is longer than T x K = %d x %d distinct slots (or 2^30)", who, longest, T, ctx->dict.K);
    if (n > 0 && (!rows || !cols || !data)) return fail(ctx, HSCMP_ERR_INVALID, "%s: %lld entries without their arrays", who, n);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    (void)read_knobs();                         // (arms HSCMP_ALLOC_FAIL_AT)
    const int cap = (int)std::max(1ll, longest), K = ctx->dict.K, F = ctx->dict.F;
    // staging, one arena slot: flag record, offsets, values, rows, columns (each 16-byte aligned)
    const auto pad = [](size_t v) { return (v + 15) / 16 * 16; };
    const size_t o_off = 16, o_data = o_off + pad((size_t)(B + 1) * 8), o_rows = o_data + pad((size_t)n * 8), o_cols = o_rows + pad((size_t)n * 4),
                 o_len = o_cols + pad((size_t)n * 4), total = o_len + pad(lengths ? (size_t)B * 4 : 0);
    int rc = epi_buffer(ctx, kArenaLoad, total);
    if (rc) { if (rc == HSCMP_ERR_ALLOC) drop_batch(ctx); return rc; }     // (out of memory: no batch, like every other entry)
    char* const stage = ctx->arena[kArenaLoad].as<char>();
    unsigned long long* const d_flag = (unsigned long long*)stage;
    const long long* const d_off = (const long long*)(stage + o_off);
    const double* const d_data = (const double*)(stage + o_data);
    const int* const d_rows = (const int*)(stage + o_rows);
    const int* const d_cols = (const int*)(stage + o_cols);
    const int* const d_len = lengths ? (const int*)(stage + o_len) : nullptr;
    const unsigned grid = (unsigned)((std::max<long long>(n, B) + kThreads - 1) / kThreads);
    HIP_TRY(ctx, hipMemsetAsync(d_flag, 0xff, sizeof(unsigned long long), ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(stage + o_off, offsets, (size_t)(B + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
    if (n > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(stage + o_data, data, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(stage + o_rows, rows, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(stage + o_cols, cols, (size_t)n * 4, hipMemcpyHostToDevice, ctx->stream));
        if (lengths) HIP_TRY(ctx, hipMemcpyAsync(stage + o_len, lengths, (size_t)B * 4, hipMemcpyHostToDevice, ctx->stream));
        hipLaunchKernelGGL((load_level_kernel<false>), dim3(grid), dim3(kThreads), 0, ctx->stream, d_off, d_rows, d_cols, d_data, n, B, T, K, cap,
                           (int*)nullptr, (int*)nullptr, (double*)nullptr, (int*)nullptr, d_flag, d_len);
        HIP_TRY(ctx, hipGetLastError());
        unsigned long long flag = 0;
        HIP_TRY(ctx, hipMemcpyAsync(&flag, d_flag, sizeof(flag), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        if (flag != ~0ull) {
            static const char* const why[] = {"", "row outside [0, T)", "column outside [0, K)", "value zero or not finite",
                                              "(column, row) not above the entry before it"};
            const long long i = (long long)(flag >> 3);
            const int reason = (int)(flag & 7);
            int b = 0;
            while (b + 1 < B && offsets[b + 1] <= i) ++b;
            if (lengths)
                return fail(ctx, HSCMP_ERR_INVALID, "%s: signal %d, entry %lld (row %d, column %d; T_b=%d K=%d): %s", who, b, i - (long long)offsets[b],
                            (int)rows[i], (int)cols[i], (int)lengths[b], K, reason == kLoadBadRow ? "row outside [0, T_b)" : why[reason >= 1 && reason <= 4 ? reason : 0]);
            return fail(ctx, HSCMP_ERR_INVALID, "%s: signal %d, entry %lld (row %d, column %d; T=%d K=%d): %s", who, b, i - (long long)offsets[b],
                        (int)rows[i], (int)cols[i], T, K, why[reason >= 1 && reason <= 4 ? reason : 0]);
        }
    }
    // from here on as an encode: the batch goes first, then its buffers are replaced
    drop_batch(ctx);
    Workspace& w = ctx->ws;
    const size_t xbytes = x ? (size_t)B * T * F * esize(ctx->dict.dtype) : 0;
    const struct { DevBuf& buf; size_t bytes; } want[] = {
        {w.slot_t, (size_t)B * cap * 4}, {w.slot_k, (size_t)B * cap * 4}, {w.slot_a, (size_t)B * cap * 8}, {w.stats, (size_t)B * ST_COUNT * sizeof(int)}, {w.x, xbytes}};
    bool stream_idle = false;
    for (const auto& b : want) {
        if (b.bytes == 0 || b.buf.holds(b.bytes)) continue;
        if (!stream_idle) { HIP_TRY(ctx, hipStreamSynchronize(ctx->stream)); stream_idle = true; }
        const hipError_t e = b.buf.replace(b.bytes);
        if (e != hipSuccess) return alloc_failed(ctx, b.bytes, e);
    }
    // (the lists are fetched whole: zero behind every signal's last entry)
    HIP_TRY(ctx, hipMemsetAsync(w.slot_t.p, 0, (size_t)B * cap * 4, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(w.slot_k.p, 0, (size_t)B * cap * 4, ctx->stream));
    HIP_TRY(ctx, hipMemsetAsync(w.slot_a.p, 0, (size_t)B * cap * 8, ctx->stream));
    if (x) HIP_TRY(ctx, hipMemcpyAsync(w.x.p, x, xbytes, hipMemcpyHostToDevice, ctx->stream));
    hipLaunchKernelGGL((load_level_kernel<true>), dim3(grid), dim3(kThreads), 0, ctx->stream, d_off, d_rows, d_cols, d_data, n, B, T, K, cap,
                       w.slot_t.as<int>(), w.slot_k.as<int>(), w.slot_a.as<double>(), w.stats.as<int>(), d_flag, (const int*)nullptr);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    ctx->B = B; ctx->T = T; ctx->cap = cap; ctx->maxsel = 0;
    ctx->P = DevParams{}; ctx->plan = EncodePlan{}; ctx->last = hscmp_params{};
    ctx->last_x_dev = x ? w.x.p : nullptr;
    ctx->timed = false;
    ctx->variant = "loaded";
    // a ragged batch: the geometry holds the lengths only (the block geometry belongs to an encode: the level above computes its own)
    ctx->ragged = lengths != nullptr;
    ctx->geom.clear();
    if (lengths) {
        ctx->geom.assign((size_t)B * kGeomWords, 0);
        for (int b = 0; b < B; ++b) ctx->geom[(size_t)b * kGeomWords] = lengths[b];
    }
    ctx->loaded = true; ctx->have_batch = true;
    return HSCMP_OK;
}

extern "C" int hscmp_load_level(hscmp_ctx* ctx, const void* x, int B, int T, const int64_t* offsets, const int32_t* rows, const int32_t* cols,
                                const double* data)
{
    return load_level_common(ctx, x, B, T, nullptr, offsets, rows, cols, data, "hscmp_load_level");
}

extern "C" int hscmp_load_level_ragged(hscmp_ctx* ctx, const void* x, int B, int T, const int32_t* lengths, const int64_t* offsets, const int32_t* rows,
                                       const int32_t* cols, const double* data)
{
    if (ctx && !lengths) return fail(ctx, HSCMP_ERR_INVALID, "hscmp_load_level_ragged: lengths is NULL");
    return load_level_common(ctx, x, B, T, lengths, offsets, rows, cols, data, "hscmp_load_level_ragged");
}

// What only an encode leaves behind (its loop state, events, residual, energies)
#define NOT_LOADED(ctx, name)                                                                   \
    if (ctx->loaded) return fail(ctx, HSCMP_ERR_STATE, name ": the batch was loaded (hscmp_load_level), not encoded: it has slots and counters only");

extern "C" int hscmp_continue(hscmp_ctx* ctx, int max_rounds)
{
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, "hscmp_continue: ctx is NULL");
    if (!ctx->have_batch) return fail(ctx, HSCMP_ERR_STATE, "hscmp_continue: no batch encoded");
    NOT_LOADED(ctx, "hscmp_continue");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    DevParams P = ctx->P;
    P.max_rounds = max_rounds;
    HIP_TRY(ctx, hipEventRecord(ctx->ev[2], ctx->stream));       // hscmp_last_kernel_ms: [2] = this launch, [0] = [1] = 0
    ctx->timed_loop_only = true;
    // the loop the encode chose: the one that understands the state it left
    const int rc = ctx->plan.f64 ? launch_loop<double>(ctx, ctx->plan, P) : launch_loop<float>(ctx, ctx->plan, P);
    if (rc) return rc;
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipEventRecord(ctx->ev[3], ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return HSCMP_OK;
}

extern "C" int hscmp_grow_events(hscmp_ctx* ctx, int new_max_events)
{
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, "hscmp_grow_events: ctx is NULL");
    if (!ctx->have_batch) return fail(ctx, HSCMP_ERR_STATE, "hscmp_grow_events: no batch encoded");
    NOT_LOADED(ctx, "hscmp_grow_events");
    if (new_max_events <= ctx->cap) return fail(ctx, HSCMP_ERR_INVALID, "hscmp_grow_events: %d is not above the current capacity %d", new_max_events, ctx->cap);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    (void)read_knobs();
    const size_t es = esize(ctx->dict.dtype), B = (size_t)ctx->B, oc = (size_t)ctx->cap, nc = (size_t)new_max_events;
    // the slot hash table follows the capacity; the loop rebuilds its contents from the slot list on the next launch
    const unsigned hmask = slot_hash_mask(new_max_events);
    Workspace& w = ctx->ws;
    DevBuf* const bufs[8] = {&w.ev_t, &w.ev_k, &w.ev_c, &w.slot_t, &w.slot_k, &w.slot_a, &w.hkey, &w.hval};     // six lists, then the table
    const size_t elem[6] = {4, 4, es, 4, 4, 8}, H = (size_t)hmask + 1;
    const size_t bytes[8] = {B * nc * elem[0], B * nc * elem[1], B * nc * elem[2], B * nc * elem[3], B * nc * elem[4], B * nc * elem[5],
                             B * H * sizeof(unsigned long long), B * H * sizeof(int)};
    // every new buffer first; the context changes only when all of them exist (a failed call leaves the batch as it was)
    DevBuf fresh[8];
    hipError_t e = hipSuccess;
    size_t failed_bytes = 0;
    for (int i = 0; i < 8 && e == hipSuccess; ++i)
        if ((i < 6 || !bufs[i]->holds(bytes[i])) && (e = fresh[i].replace(bytes[i])) != hipSuccess) failed_bytes = bytes[i];
    for (int i = 0; i < 6 && e == hipSuccess; ++i) e = hipMemset(fresh[i].p, 0, bytes[i]);      // (the new tail of every list: see ensure_workspace_g)
    for (int i = 0; i < 6 && e == hipSuccess; ++i)
        e = hipMemcpy2D(fresh[i].p, nc * elem[i], bufs[i]->p, oc * elem[i], oc * elem[i], B, hipMemcpyDeviceToDevice);
    std::vector<int> stats(B * ST_COUNT);
    if (e == hipSuccess) e = hipMemcpy(stats.data(), w.stats.p, stats.size() * sizeof(int), hipMemcpyDeviceToHost);
    if (e == hipSuccess) {
        for (size_t b = 0; b < B; ++b)
            if (stats[b * ST_COUNT + ST_STOP] == STOP_CAPACITY) stats[b * ST_COUNT + ST_STOP] = STOP_RUNNING;
        e = hipMemcpy(w.stats.p, stats.data(), stats.size() * sizeof(int), hipMemcpyHostToDevice);
    }
    if (e != hipSuccess)        // (the fresh buffers free themselves)
        return fail(ctx, failed_bytes ? HSCMP_ERR_ALLOC : HSCMP_ERR_HIP, "hscmp_grow_events: %s (%zu bytes)", hipGetErrorString(e), failed_bytes);
    for (int i = 0; i < 8; ++i) if (fresh[i].p) *bufs[i] = std::move(fresh[i]);
    ctx->cap = new_max_events; ctx->P.cap = new_max_events; ctx->P.hmask = hmask; ctx->last.max_events = new_max_events;
    return HSCMP_OK;
}

extern "C" int hscmp_stop_signal(hscmp_ctx* ctx, int b)
{
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, "hscmp_stop_signal: ctx is NULL");
    if (!ctx->have_batch || b < 0 || b >= ctx->B) return fail(ctx, HSCMP_ERR_STATE, "hscmp_stop_signal: bad signal index %d", b);
    NOT_LOADED(ctx, "hscmp_stop_signal");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int v = STOP_CALLBACK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    int cur = 0;
    HIP_TRY(ctx, hipMemcpy(&cur, ctx->ws.stats.as<int>() + (size_t)b * ST_COUNT + ST_STOP, sizeof(int), hipMemcpyDeviceToHost));
    if (cur == STOP_RUNNING)
        HIP_TRY(ctx, hipMemcpy(ctx->ws.stats.as<int>() + (size_t)b * ST_COUNT + ST_STOP, &v, sizeof(int), hipMemcpyHostToDevice));
    return HSCMP_OK;
}

static int fetch(hscmp_ctx* ctx, void* dst, const void* src, size_t bytes)
{
    if (!dst) return HSCMP_OK;
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    return HSCMP_OK;
}

#define NEED_BATCH(ctx, name)                                                                   \
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, name ": ctx is NULL");                    \
    if (!ctx->have_batch) return fail(ctx, HSCMP_ERR_STATE, name ": no batch encoded");         \
    HIP_TRY(ctx, hipSetDevice(ctx->device));

extern "C" int hscmp_fetch_events(hscmp_ctx* ctx, int32_t* ev_t, int32_t* ev_k, void* ev_c)
{
    NEED_BATCH(ctx, "hscmp_fetch_events");
    NOT_LOADED(ctx, "hscmp_fetch_events");
    const size_t n = (size_t)ctx->B * ctx->cap;
    int rc;
    if ((rc = fetch(ctx, ev_t, ctx->ws.ev_t.as<int>(), n * 4))) return rc;
    if ((rc = fetch(ctx, ev_k, ctx->ws.ev_k.as<int>(), n * 4))) return rc;
    if ((rc = fetch(ctx, ev_c, ctx->ws.ev_c.p, n * esize(ctx->dict.dtype)))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return HSCMP_OK;
}

extern "C" int hscmp_fetch_slots(hscmp_ctx* ctx, int32_t* slot_t, int32_t* slot_k, double* slot_acc)
{
    NEED_BATCH(ctx, "hscmp_fetch_slots");
    const size_t n = (size_t)ctx->B * ctx->cap;
    int rc;
    if ((rc = fetch(ctx, slot_t, ctx->ws.slot_t.as<int>(), n * 4))) return rc;
    if ((rc = fetch(ctx, slot_k, ctx->ws.slot_k.as<int>(), n * 4))) return rc;
    if ((rc = fetch(ctx, slot_acc, ctx->ws.slot_a.as<double>(), n * 8))) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return HSCMP_OK;
}

extern "C" int hscmp_fetch_stats(hscmp_ctx* ctx, int32_t* stats)
{
    NEED_BATCH(ctx, "hscmp_fetch_stats");
    int rc = fetch(ctx, stats, ctx->ws.stats.as<int>(), (size_t)ctx->B * ST_COUNT * sizeof(int));
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return HSCMP_OK;
}

extern "C" int hscmp_fetch_residual(hscmp_ctx* ctx, void* residual)
{
    NEED_BATCH(ctx, "hscmp_fetch_residual");
    NOT_LOADED(ctx, "hscmp_fetch_residual");
    int rc = fetch(ctx, residual, ctx->ws.resid.p, (size_t)ctx->B * ctx->T * ctx->dict.F * esize(ctx->dict.dtype));
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return HSCMP_OK;
}

extern "C" int hscmp_fetch_energies(hscmp_ctx* ctx, double* energies)
{
    NEED_BATCH(ctx, "hscmp_fetch_energies");
    NOT_LOADED(ctx, "hscmp_fetch_energies");
    if (!energies) return HSCMP_OK;
    const size_t n = (size_t)ctx->B * 2;
    if (ctx->dict.dtype == HSCMP_F64) {
        int rc = fetch(ctx, energies, ctx->ws.energy.p, n * 8);
        if (rc) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    } else {
        std::vector<float> tmp(n);
        int rc = fetch(ctx, tmp.data(), ctx->ws.energy.p, n * 4);
        if (rc) return rc;
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        for (size_t i = 0; i < n; ++i) energies[i] = (double)tmp[i];
    }
    return HSCMP_OK;
}

extern "C" int hscmp_get_device_view(hscmp_ctx* ctx, hscmp_device_view* v)
{
    NEED_BATCH(ctx, "hscmp_get_device_view");
    NOT_LOADED(ctx, "hscmp_get_device_view");
    if (!v) return fail(ctx, HSCMP_ERR_INVALID, "hscmp_get_device_view: view is NULL");
    v->B = ctx->B; v->T = ctx->T; v->F = ctx->dict.F; v->K = ctx->dict.K; v->W = ctx->dict.W; v->max_events = ctx->cap;
    v->dtype = ctx->dict.dtype; v->reserved = 0;
    v->ev_t = ctx->ws.ev_t.as<int>(); v->ev_k = ctx->ws.ev_k.as<int>(); v->ev_c = ctx->ws.ev_c.p; v->stats = ctx->ws.stats.as<int>();
    v->residual = ctx->ws.resid.p; v->energies = ctx->ws.energy.p; v->best_c = ctx->ws.best_c.p; v->best_k = ctx->ws.best_k.as<int>();
    return HSCMP_OK;
}

extern "C" int hscmp_last_kernel_ms(hscmp_ctx* ctx, float* out4)
{
    if (!ctx || !out4) return fail(ctx, HSCMP_ERR_INVALID, "hscmp_last_kernel_ms: NULL argument");
    if (!ctx->timed) return fail(ctx, HSCMP_ERR_STATE, "hscmp_last_kernel_ms: nothing timed yet");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipEventSynchronize(ctx->ev[3]));
    out4[0] = out4[1] = out4[3] = 0.f;
    for (int i = ctx->timed_loop_only ? 2 : 0; i < 3; ++i) HIP_TRY(ctx, hipEventElapsedTime(&out4[i], ctx->ev[i], ctx->ev[i + 1]));
    return HSCMP_OK;
}

extern "C" int hscmp_mem_info(hscmp_ctx* ctx, uint64_t* free_bytes, uint64_t* total_bytes)
{
    if (!ctx || !free_bytes || !total_bytes) return fail(ctx, HSCMP_ERR_INVALID, "hscmp_mem_info: NULL argument");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    size_t f = 0, t = 0;
    HIP_TRY(ctx, hipMemGetInfo(&f, &t));
    *free_bytes = f; *total_bytes = t;
    return HSCMP_OK;
}

extern "C" const char* hscmp_last_variant(hscmp_ctx* ctx) { return ctx ? ctx->variant.c_str() : ""; }

extern "C" int hscmp_copy_from_device(hscmp_ctx* ctx, const void* src_dev, uint64_t nbytes, void* dst_host)
{
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, "hscmp_copy_from_device: ctx is NULL");
    if (!src_dev || !dst_host) return fail(ctx, HSCMP_ERR_INVALID, "hscmp_copy_from_device: NULL argument");
    if (nbytes == 0) return HSCMP_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipMemcpyAsync(dst_host, src_dev, (size_t)nbytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return HSCMP_OK;
}

// modeling.py:149-188 convolve1d on the GPU: full table out [Tout][K]
template <typename R> static void launch_convolve(hscmp_ctx* ctx, const R* dx, int T, int same, int Tout, R* dout)
{
    DevParams P{};
    P.B = 1; P.T = T; P.K = ctx->dict.K; P.W = ctx->dict.W; P.F = ctx->dict.F; P.off = (ctx->dict.W - 1) / 2;
    State<R> S{};
    S.D = ctx->dict.D.as<const R>(); S.weights = nullptr;
    S.Dc = ctx->dict.Dc.p ? ctx->dict.Dc.as<const R>() : ctx->dict.D.as<const R>();
    dim3 grid((Tout + kThreads - 1) / kThreads, 1);
    hipLaunchKernelGGL((corr_init_generic_kernel<R, true>), grid, dim3(kThreads), 0, ctx->stream, P, S, dx, same ? P.off : 0, Tout, dout);
}

template <typename R> static int run_convolve(hscmp_ctx* ctx, const void* x, int T, int same, void* out)
{
    const int K = ctx->dict.K, W = ctx->dict.W, F = ctx->dict.F;
    const int Tout = same ? T : T - W + 1;
    if (Tout <= 0) return fail(ctx, HSCMP_ERR_INVALID, "hscmp_convolve1d: T=%d shorter than the filters (W=%d)", T, W);
    int rc;
    if ((rc = epi_buffer(ctx, kArenaRowA, (size_t)T * F * sizeof(R))) != HSCMP_OK) return rc;
    if ((rc = epi_buffer(ctx, kArenaRowB, (size_t)Tout * K * sizeof(R))) != HSCMP_OK) return rc;
    R* dx = ctx->arena[kArenaRowA].as<R>(); R* dout = ctx->arena[kArenaRowB].as<R>();
    HIP_TRY(ctx, hipMemcpyAsync(dx, x, (size_t)T * F * sizeof(R), hipMemcpyHostToDevice, ctx->stream));
    launch_convolve<R>(ctx, dx, T, same, Tout, dout);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out, dout, (size_t)Tout * K * sizeof(R), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return HSCMP_OK;
}

extern "C" int hscmp_convolve1d(hscmp_ctx* ctx, const void* x, int T, int same, void* out)
{
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, "hscmp_convolve1d: ctx is NULL");
    if (ctx->dict.dtype < 0) return fail(ctx, HSCMP_ERR_STATE, "hscmp_convolve1d: no dictionary set");
    NOT_A_SET(ctx, "hscmp_convolve1d");
    if (!x || !out || T <= 0) return fail(ctx, HSCMP_ERR_INVALID, "hscmp_convolve1d: bad arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    (void)read_knobs();
    return ctx->dict.dtype == HSCMP_F32 ? run_convolve<float>(ctx, x, T, same, out) : run_convolve<double>(ctx, x, T, same, out);
}

// modeling.py:454-460: per-window best (position, atom, coefficient) of the k-means learner
template <typename R>
static int run_assign(hscmp_ctx* ctx, const void* windows, int N, int L, int32_t* out_t, int32_t* out_k, void* out_c)
{
    const int K = ctx->dict.K, W = ctx->dict.W, F = ctx->dict.F;
    const size_t wbytes = (size_t)N * L * F * sizeof(R);
    int rc;
    if ((rc = epi_buffer(ctx, kArenaRowA, wbytes)) != HSCMP_OK) return rc;
    if ((rc = epi_buffer(ctx, kArenaRowB, (size_t)N * sizeof(int))) != HSCMP_OK) return rc;
    if ((rc = epi_buffer(ctx, kArenaRowC, (size_t)N * sizeof(int))) != HSCMP_OK) return rc;
    if ((rc = epi_buffer(ctx, kArenaRowD, (size_t)N * sizeof(R))) != HSCMP_OK) return rc;
    R* dwin = ctx->arena[kArenaRowA].as<R>(); int* dt = ctx->arena[kArenaRowB].as<int>(); int* dk = ctx->arena[kArenaRowC].as<int>(); R* dc = ctx->arena[kArenaRowD].as<R>();
    HIP_TRY(ctx, hipMemcpyAsync(dwin, windows, wbytes, hipMemcpyHostToDevice, ctx->stream));
    const int lds_elems = (size_t)L * F * sizeof(R) <= 32768 ? L * F : 0;
    hipLaunchKernelGGL((assign_windows_kernel<R>), dim3(N), dim3(kThreads), (size_t)lds_elems * sizeof(R), ctx->stream,
                       (const R*)dwin, L, K, W, F, ctx->dict.D.as<const R>(), lds_elems, dt, dk, dc);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(out_t, dt, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(out_k, dk, (size_t)N * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    if (out_c) HIP_TRY(ctx, hipMemcpyAsync(out_c, dc, (size_t)N * sizeof(R), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return HSCMP_OK;
}

extern "C" int hscmp_assign_windows(hscmp_ctx* ctx, const void* windows, int N, int L, int32_t* out_t, int32_t* out_k, void* out_c)
{
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, "hscmp_assign_windows: ctx is NULL");
    if (ctx->dict.dtype < 0) return fail(ctx, HSCMP_ERR_STATE, "hscmp_assign_windows: no dictionary set");
    NOT_A_SET(ctx, "hscmp_assign_windows");
    if (!windows || !out_t || !out_k || N <= 0) return fail(ctx, HSCMP_ERR_INVALID, "hscmp_assign_windows: bad arguments");
    if (L < ctx->dict.W) return fail(ctx, HSCMP_ERR_INVALID, "hscmp_assign_windows: windows of %d samples are shorter than the filters (W=%d)", L, ctx->dict.W);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    (void)read_knobs();
    return ctx->dict.dtype == HSCMP_F32 ? run_assign<float>(ctx, windows, N, L, out_t, out_k, out_c)
                                   : run_assign<double>(ctx, windows, N, L, out_t, out_k, out_c);
}

// ---- host-side synthesis (modeling.py:226-263 reconstructSignal, sparse branch) ------------------------------
// signal[t - (W-1)/2 + w][f] += c * D[k][w][f] for every event (t, k, c), in the order given, clipped at the borders
// (utils.py:103-131): the reference's sequential overlap-add, float64 accumulation.  Plain host code (no GPU work):
// it is the epilogue of the hierarchical encoder (modeling.py:1596-1611) and releases the Python interpreter lock
// while it runs, so a batch can be post-processed on all cores.
extern "C" int hscmp_host_overlap_add(double* signal, int64_t T, int Fd, const int64_t* rows, const int64_t* cols, const double* data,
                                      int64_t n, const void* D, int W, int dict_is_f32)
{
    if (!signal || !D || (n > 0 && (!rows || !cols || !data)) || T <= 0 || Fd <= 0 || W <= 0) return HSCMP_ERR_INVALID;
    const int64_t lead = (W - 1) / 2, atom = (int64_t)W * Fd;
    for (int64_t i = 0; i < n; ++i) {
        const double c = data[i];
        if (c == 0.0) continue;
        const int64_t p0 = rows[i] - lead;
        const int64_t w0 = p0 < 0 ? -p0 : 0, w1 = p0 + W > T ? T - p0 : W;
        double* dst = signal + (p0 + w0) * Fd;
        if (dict_is_f32) {
            const float* src = (const float*)D + cols[i] * atom + w0 * Fd;
            for (int64_t e = 0; e < (w1 - w0) * Fd; ++e) dst[e] += c * (double)src[e];
        } else {
            const double* src = (const double*)D + cols[i] * atom + w0 * Fd;
            for (int64_t e = 0; e < (w1 - w0) * Fd; ++e) dst[e] += c * src[e];
        }
    }
    return HSCMP_OK;
}

// Host-side CSC assembly of one signal's coefficient slots (modeling.py:1171-1181): drop zeros and |a| < min_coefficients
// (NaN: no clip), order by (atom, position).  indptr [K+1], indices / data [n] (first indptr[K] entries used).
// Slots are distinct (t, k) pairs, so there is nothing to sum.  Plain host code.
extern "C" int hscmp_host_slots_to_csc(const int32_t* slot_t, const int32_t* slot_k, const double* slot_a, int64_t n, int K,
                                       double min_coefficients, int32_t* indptr, int32_t* indices, double* data)
{
    if (n < 0 || K <= 0 || !indptr || (n > 0 && (!slot_t || !slot_k || !slot_a || !indices || !data))) return HSCMP_ERR_INVALID;
    const bool clip = !std::isnan(min_coefficients);
    std::vector<int64_t> keep;
    keep.reserve((size_t)n);
    for (int k = 0; k <= K; ++k) indptr[k] = 0;
    for (int64_t i = 0; i < n; ++i) {
        const double a = slot_a[i];
        if (a == 0.0 || (clip && !(std::fabs(a) >= min_coefficients))) continue;
        if (slot_k[i] < 0 || slot_k[i] >= K) return HSCMP_ERR_INVALID;
        keep.push_back(i);
        indptr[slot_k[i] + 1] += 1;
    }
    for (int k = 0; k < K; ++k) indptr[k + 1] += indptr[k];
    std::vector<int32_t> cur(indptr, indptr + K);
    for (int64_t i : keep) {                       // counting sort by atom ...
        const int32_t o = cur[slot_k[i]]++;
        indices[o] = slot_t[i]; data[o] = slot_a[i];
    }
    for (int k = 0; k < K; ++k) {                  // ... then by position inside each column (short runs: insertion sort)
        const int32_t b0 = indptr[k], b1 = indptr[k + 1];
        if (b1 - b0 > 64) {
            std::vector<std::pair<int32_t, double>> col((size_t)(b1 - b0));
            for (int32_t j = b0; j < b1; ++j) col[(size_t)(j - b0)] = {indices[j], data[j]};
            std::sort(col.begin(), col.end(), [](const std::pair<int32_t, double>& x, const std::pair<int32_t, double>& y) { return x.first < y.first; });
            for (int32_t j = b0; j < b1; ++j) { indices[j] = col[(size_t)(j - b0)].first; data[j] = col[(size_t)(j - b0)].second; }
        } else {
            for (int32_t j = b0 + 1; j < b1; ++j) {
                const int32_t ti = indices[j]; const double av = data[j];
                int32_t q = j;
                while (q > b0 && indices[q - 1] > ti) { indices[q] = indices[q - 1]; data[q] = data[q - 1]; --q; }
                indices[q] = ti; data[q] = av;
            }
        }
    }
    return HSCMP_OK;
}

// ---- epilogue of the hierarchical encoder on the device (hscmp_epilogue.h) -----------------------------------------

extern "C" int hscmp_hierarchy_epilogue(hscmp_ctx* last, hscmp_ctx* level0, int first, const hscmp_epilogue_level* levels, int nlevels,
                                        double min_coefficients, const int64_t* offsets, int32_t* out_n, int32_t* out_colptr,
                                        int32_t* out_indices, double* out_data, void* out_events, double* out_residual,
                                        double* out_residual_energy)
{
    if (!last || !level0) return fail(last, HSCMP_ERR_INVALID, "hscmp_hierarchy_epilogue: NULL context");
    NOT_A_SET(last, "hscmp_hierarchy_epilogue");
    if (level0->dict.G > 0) return fail(last, HSCMP_ERR_STATE, "hscmp_hierarchy_epilogue: level 0 holds a set of dictionaries (hscmp_set_dictionaries)");
    if (!last->have_batch || !level0->have_batch) return fail(last, HSCMP_ERR_STATE, "hscmp_hierarchy_epilogue: no batch encoded");
    NOT_LOADED(last, "hscmp_hierarchy_epilogue (last level)");
    if (last->device != level0->device) return fail(last, HSCMP_ERR_INVALID, "hscmp_hierarchy_epilogue: contexts on different GPUs");
    if (!levels || nlevels < 1 || nlevels > kEpiMaxLevels || !offsets || !out_n || !out_colptr || !out_indices || !out_data)
        return fail(last, HSCMP_ERR_INVALID, "hscmp_hierarchy_epilogue: bad arguments");
    const int count = last->B, T = last->T, Fd = level0->dict.F, Ktot = last->dict.K;
    if (first < 0 || first + count > level0->B || level0->T != T) return fail(last, HSCMP_ERR_INVALID, "hscmp_hierarchy_epilogue: signal range / length mismatch");
    // ragged batches: the last level's lengths are level 0's, rows [first, first + count)
    const bool ragged = last->ragged;
    if (ragged != level0->ragged) return fail(last, HSCMP_ERR_INVALID, "hscmp_hierarchy_epilogue: one of the two levels holds a ragged batch, the other a uniform one");
    std::vector<int> lens;
    if (ragged) {
        lens.resize((size_t)count);
        for (int b = 0; b < count; ++b) {
            lens[(size_t)b] = last->geom[(size_t)b * kGeomWords];
            const int l0 = level0->geom[(size_t)(first + b) * kGeomWords];
            if (l0 != lens[(size_t)b])
                return fail(last, HSCMP_ERR_INVALID, "hscmp_hierarchy_epilogue: signal %d has length %d at the last level, %d at level 0 (signal %d)", b, lens[(size_t)b], l0, first + b);
        }
    }
    if (!level0->last_x_dev) return fail(last, HSCMP_ERR_STATE, "hscmp_hierarchy_epilogue: the level-0 input is not on the device any more");
    if (Ktot >= (1 << kEpiColBits) || T >= (1 << kEpiTBits) || last->cap >= (1 << kEpiIdxBits))
        return fail(last, HSCMP_ERR_UNSUPPORTED, "hscmp_hierarchy_epilogue: shape outside the key layout (K < 2^20, T < 2^24, list < 2^20)");
    HIP_TRY(last, hipSetDevice(last->device));
    HIP_TRY(last, hipStreamSynchronize(level0->stream));
    HIP_TRY(last, hipStreamSynchronize(last->stream));
    const Knobs kn = read_knobs();
    const long long total = offsets[count];
    EpiArgs A{};
    A.nlevels = nlevels; A.Ktot = Ktot; A.T = T; A.Fd = Fd;
    A.has_min = !std::isnan(min_coefficients); A.minc = A.has_min ? min_coefficients : 0.0;
    // representations: one device buffer, level after level
    size_t rep_bytes = 0;
    for (int l = 0; l < nlevels; ++l) {
        const hscmp_epilogue_level& d = levels[l];
        if (d.col1 > d.col0 && (!d.rep || d.scale <= 0 || d.col1 > Ktot || d.col0 < 0)) return fail(last, HSCMP_ERR_INVALID, "hscmp_hierarchy_epilogue: bad level %d", l);
        rep_bytes += ((size_t)std::max(0, d.col1) * std::max(0, d.scale) * Fd * (d.rep_is_f32 ? 4 : 8) + 15) / 16 * 16;
    }
    int rc;
    if ((rc = epi_buffer(last, kArenaEpiRep, std::max<size_t>(16, rep_bytes)))) return rc;
    size_t ro = 0;
    for (int l = 0; l < nlevels; ++l) {
        const hscmp_epilogue_level& d = levels[l];
        EpiLevel& L = A.lv[l];
        L.col0 = d.col0; L.col1 = d.col1; L.scale = d.scale; L.lead = (d.scale - 1) / 2; L.rep_f32 = d.rep_is_f32; L.rep = nullptr;
        if (d.col1 <= d.col0) continue;
        const size_t nb = (size_t)d.col1 * d.scale * Fd * (d.rep_is_f32 ? 4 : 8);       // rows [0, col1): indexed by the column number
        L.rep = last->arena[kArenaEpiRep].as<char>() + ro;
        HIP_TRY(last, hipMemcpyAsync(last->arena[kArenaEpiRep].as<char>() + ro, d.rep, nb, hipMemcpyHostToDevice, last->stream));
        ro += (nb + 15) / 16 * 16;
        A.max_back = std::max(A.max_back, d.scale - 1 - L.lead);
        A.max_fwd = std::max(A.max_fwd, L.lead);
    }
    int nmax = 2;
    while (nmax < last->cap) nmax <<= 1;
    const int lds_keys = kn.epi_lds_keys;                        // (HSCMP_EPI_LDS_KEYS: tests force the chunked sort at small sizes)
    const size_t nres = out_residual ? (size_t)count * T * Fd * sizeof(double) : 0;
    const size_t nev = out_events ? (size_t)total * 16 : 0;      // (a multiple of 16: the residual behind the events stays aligned)
    // by arena slot, kArenaEpiOffsets .. kArenaEpiKeys (kArenaEpiOut: the events, then the residual)
    const size_t off_bytes = (size_t)(count + 1) * sizeof(long long);      // (a ragged batch: the lengths ride behind the offsets)
    const size_t sizes[8] = {0, off_bytes + (ragged ? (size_t)count * sizeof(int) : 0), (size_t)count * sizeof(int), (size_t)count * (Ktot + 1) * sizeof(int),
                             std::max<size_t>(16, (size_t)total * sizeof(int)), std::max<size_t>(16, (size_t)total * sizeof(double)),
                             std::max<size_t>(16, nev + nres),
                             (size_t)count * nmax * sizeof(unsigned long long)};       // (the t-sorted keys move there while the LDS holds residual tiles)
    for (int i = kArenaEpiOffsets; i <= kArenaEpiKeys; ++i) if (sizes[i] && (rc = epi_buffer(last, i, sizes[i]))) return rc;
    DevBuf* const arena = last->arena;
    HIP_TRY(last, hipMemcpyAsync(arena[kArenaEpiOffsets].p, offsets, off_bytes, hipMemcpyHostToDevice, last->stream));
    if (ragged) {
        HIP_TRY(last, hipMemcpyAsync(arena[kArenaEpiOffsets].as<char>() + off_bytes, lens.data(), (size_t)count * sizeof(int), hipMemcpyHostToDevice, last->stream));
        A.lens = (const int*)(arena[kArenaEpiOffsets].as<char>() + off_bytes);
    }
    A.slot_t = last->ws.slot_t.as<int>(); A.slot_k = last->ws.slot_k.as<int>(); A.slot_a = last->ws.slot_a.as<double>(); A.stats = last->ws.stats.as<int>(); A.cap = last->cap;
    A.offsets = arena[kArenaEpiOffsets].as<const long long>(); A.out_n = arena[kArenaEpiN].as<int>(); A.out_colptr = arena[kArenaEpiColptr].as<int>();
    A.out_indices = arena[kArenaEpiIndices].as<int>(); A.out_data = arena[kArenaEpiData].as<double>();
    A.out_events = out_events ? arena[kArenaEpiOut].as<int>() : nullptr;
    A.out_residual = out_residual ? (double*)(arena[kArenaEpiOut].as<char>() + nev) : nullptr;
    A.scratch = arena[kArenaEpiKeys].as<unsigned long long>(); A.scratch_n = nmax;
    if (out_residual_energy) {
        if ((rc = epi_buffer(last, kArenaEpiEnergy, (size_t)count * sizeof(double)))) return rc;
        A.out_energy = last->arena[kArenaEpiEnergy].as<double>();
    }
    const size_t lds = std::max<size_t>((size_t)std::min(nmax, lds_keys) * sizeof(unsigned long long), kn.epi_lds_keys_set ? 8192 : 65536);
    A.lds_keys = std::min(nmax, lds_keys); A.lds_bytes = (int)lds;
    const size_t xoff = (size_t)first * T * Fd * esize(level0->dict.dtype);
    if (level0->dict.dtype == HSCMP_F32) {
        auto kern = hier_epilogue_kernel<float>;
        HIP_TRY(last, set_dyn_lds((const void*)kern, lds));
        hipLaunchKernelGGL(kern, dim3(count), dim3(kEpiThreads), lds, last->stream, A, (const float*)((const char*)level0->last_x_dev + xoff));
    } else {
        auto kern = hier_epilogue_kernel<double>;
        HIP_TRY(last, set_dyn_lds((const void*)kern, lds));
        hipLaunchKernelGGL(kern, dim3(count), dim3(kEpiThreads), lds, last->stream, A, (const double*)((const char*)level0->last_x_dev + xoff));
    }
    HIP_TRY(last, hipGetLastError());
    HIP_TRY(last, hipMemcpyAsync(out_n, A.out_n, sizes[kArenaEpiN], hipMemcpyDeviceToHost, last->stream));
    HIP_TRY(last, hipMemcpyAsync(out_colptr, A.out_colptr, sizes[kArenaEpiColptr], hipMemcpyDeviceToHost, last->stream));
    if (total > 0) {
        HIP_TRY(last, hipMemcpyAsync(out_indices, A.out_indices, (size_t)total * sizeof(int), hipMemcpyDeviceToHost, last->stream));
        HIP_TRY(last, hipMemcpyAsync(out_data, A.out_data, (size_t)total * sizeof(double), hipMemcpyDeviceToHost, last->stream));
        if (out_events) HIP_TRY(last, hipMemcpyAsync(out_events, A.out_events, (size_t)total * 16, hipMemcpyDeviceToHost, last->stream));
    }
    if (out_residual) HIP_TRY(last, hipMemcpyAsync(out_residual, A.out_residual, nres, hipMemcpyDeviceToHost, last->stream));
    if (out_residual_energy) HIP_TRY(last, hipMemcpyAsync(out_residual_energy, A.out_energy, (size_t)count * sizeof(double), hipMemcpyDeviceToHost, last->stream));
    HIP_TRY(last, hipStreamSynchronize(last->stream));
    return HSCMP_OK;
}

#ifdef HSCMP_DBG_STAMPS
extern "C" int hscmp_debug_blocks(unsigned long long* out, int n)
{
    return hipMemcpyFromSymbol(out, HIP_SYMBOL(hscmp::g_blk), (size_t)n * 3 * sizeof(unsigned long long)) == hipSuccess ? 0 : -1;
}
// diagnostic build only
extern "C" int hscmp_debug_counters(unsigned long long* out16, int reset)
{
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(hscmp::g_cnt), 16 * sizeof(unsigned long long)) != hipSuccess) return -1;
    if (reset) { unsigned long long z[16] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(hscmp::g_cnt), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
}

extern "C" int hscmp_debug_stamps(unsigned long long* out16, int reset)
{
    if (hipMemcpyFromSymbol(out16, HIP_SYMBOL(hscmp::g_stamps), 64 * sizeof(unsigned long long)) != hipSuccess) return -1;      // (64 entries)
    if (reset) { unsigned long long z[64] = {0}; if (hipMemcpyToSymbol(HIP_SYMBOL(hscmp::g_stamps), z, sizeof(z)) != hipSuccess) return -1; }
    return 0;
}
#endif

// ---- row-level entry points (modeling.py:899-982 and :1018-1051) -------------------------------------
// One selection (modeling.py:899-982) on a table that is ON THE DEVICE: d_ip [T][K], d_w [K] or null.  Uses the batch
// workspace of the context (a batch held by the context is gone afterwards) but none of its dictionary state.
template <typename R>
static int select_on_device(hscmp_ctx* ctx, const Knobs& kn, const R* d_ip, const R* d_w, int T, int K, int W, int nb_blocks, int offset, double thres,
                            int32_t* out_t, int32_t* out_k, void* out_c, int max_out, int32_t* n_out, const char* who)
{
    hscmp_params hp{};
    hp.nb_nonzero_coefs = -1; hp.nb_blocks = nb_blocks; hp.tolerance_snr = NAN; hp.tolerance_residual_scale = NAN;
    hp.null_coeff_thres = thres; hp.eps = 0.0; hp.max_events = 1; hp.max_rounds = 1;
    DevParams P;
    int rc = make_params_g(ctx, kn, K, W, 1, 1, T, &hp, &P);               // only T, K, W matter for the selection
    if (rc != HSCMP_OK) return rc;
    drop_batch(ctx);
    if ((rc = ensure_workspace_g(ctx, P, false, sizeof(R), false, false)) != HSCMP_OK) return rc;
    ctx->listed_rows = 0;
    State<R> S = make_state<R>(ctx, false);
    S.D = nullptr; S.Dc = nullptr; S.weights = d_w;
    hipLaunchKernelGGL((table_to_best_kernel<R>), dim3((T + kThreads - 1) / kThreads), dim3(kThreads), 0, ctx->stream,
                       d_ip, T, K, d_w, S.best_c, S.best_k);
    int st[ST_COUNT] = {0};
    st[ST_OFFSET] = offset ? 1 : 0;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->ws.stats.as<int>(), st, sizeof(st), hipMemcpyHostToDevice, ctx->stream));
    P.select_only = 1; P.has_snr = 0; P.has_scale = 0;
    set_segments(P, GenericRecorr<R>::kMaxSegments);
    const size_t lds = ((sizeof(typename GenericRecorr<R>::Shared) + 15) / 16) * 16 + GenericRecorr<R>::extra_lds_bytes(P);
    auto kern = iterate_kernel<R, GenericRecorr<R>>;
    HIP_TRY(ctx, set_dyn_lds((const void*)kern, lds));
    hipLaunchKernelGGL(kern, dim3(1), dim3(kThreads), lds, ctx->stream, P, S, typename GenericRecorr<R>::Args{});
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(st, ctx->ws.stats.as<int>(), sizeof(st), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const int n = st[ST_EVENTS];
    *n_out = n;
    if (n > max_out) return fail(ctx, HSCMP_ERR_INVALID, "%s: %d atoms selected, room for %d", who, n, max_out);
    if (n > 0) {                                                        // the ordered list lives in the second half of the selection scratch
        HIP_TRY(ctx, hipMemcpyAsync(out_t, ctx->ws.sel_t.as<int>() + P.maxsel, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(out_k, ctx->ws.sel_k.as<int>() + P.maxsel, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(out_c, ctx->ws.sel_c.as<R>() + P.maxsel, (size_t)n * sizeof(R), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    }
    return HSCMP_OK;
}

template <typename R> static int upload_weights(hscmp_ctx* ctx, const void* weights, int K, const R** d_w)
{
    *d_w = nullptr;
    if (!weights) return HSCMP_OK;
    int rc = epi_buffer(ctx, kArenaTabW, (size_t)K * sizeof(R));
    if (rc != HSCMP_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->arena[kArenaTabW].p, weights, (size_t)K * sizeof(R), hipMemcpyHostToDevice, ctx->stream));
    *d_w = ctx->arena[kArenaTabW].as<const R>();
    return HSCMP_OK;
}

template <typename R>
static int run_select(hscmp_ctx* ctx, const Knobs& kn, const void* ip, int T, int K, int W, int nb_blocks, int offset, double thres,
                      const void* weights, int32_t* out_t, int32_t* out_k, void* out_c, int max_out, int32_t* n_out)
{
    int rc = epi_buffer(ctx, kArenaRowA, (size_t)T * K * sizeof(R));
    if (rc != HSCMP_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->arena[kArenaRowA].p, ip, (size_t)T * K * sizeof(R), hipMemcpyHostToDevice, ctx->stream));
    const R* d_w;
    if ((rc = upload_weights<R>(ctx, weights, K, &d_w)) != HSCMP_OK) return rc;
    return select_on_device<R>(ctx, kn, ctx->arena[kArenaRowA].as<const R>(), d_w, T, K, W, nb_blocks, offset, thres, out_t, out_k, out_c, max_out, n_out,
                               "hscmp_select_best_atoms");
}

extern "C" int hscmp_select_best_atoms(hscmp_ctx* ctx, const void* ip, int T, int K, int W, hscmp_dtype dtype, int nb_blocks,
                                       int offset, double null_coeff_thres, const void* weights,
                                       int32_t* out_t, int32_t* out_k, void* out_c, int max_out, int32_t* n_out)
{
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, "hscmp_select_best_atoms: ctx is NULL");
    if (!ip || !out_t || !out_k || !out_c || !n_out || T <= 0 || K <= 0 || W <= 0)
        return fail(ctx, HSCMP_ERR_INVALID, "hscmp_select_best_atoms: bad arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const Knobs kn = read_knobs();
    return dtype == HSCMP_F32
        ? run_select<float>(ctx, kn, ip, T, K, W, nb_blocks, offset, null_coeff_thres, weights, out_t, out_k, out_c, max_out, n_out)
        : run_select<double>(ctx, kn, ip, T, K, W, nb_blocks, offset, null_coeff_thres, weights, out_t, out_k, out_c, max_out, n_out);
}

template <typename R> static void launch_update_rows(hscmp_ctx* ctx, const R* d_r, int T, int p, R* d_rows, R* d_table)
{
    const int K = ctx->dict.K, W = ctx->dict.W, nrows = 2 * W - 1;
    DevParams P{};
    P.B = 1; P.T = T; P.K = K; P.W = W; P.F = ctx->dict.F; P.off = (W - 1) / 2;
    const int grid = (nrows * K + kThreads - 1) / kThreads;
    hipLaunchKernelGGL((update_rows_kernel<R>), dim3(grid), dim3(kThreads), 0, ctx->stream, P, d_r, ctx->dict.D.as<const R>(), p, d_rows, d_table);
}

template <typename R> static int run_update_rows(hscmp_ctx* ctx, void* ip, const void* residual, int T, int p)
{
    const int K = ctx->dict.K, W = ctx->dict.W, F = ctx->dict.F, nrows = 2 * W - 1;
    int rc;
    if ((rc = epi_buffer(ctx, kArenaRowA, (size_t)T * F * sizeof(R))) != HSCMP_OK) return rc;
    if ((rc = epi_buffer(ctx, kArenaRowB, (size_t)nrows * K * sizeof(R))) != HSCMP_OK) return rc;
    R* d_r = ctx->arena[kArenaRowA].as<R>(); R* d_out = ctx->arena[kArenaRowB].as<R>();
    std::vector<R> rows((size_t)nrows * K);
    HIP_TRY(ctx, hipMemcpyAsync(d_r, residual, (size_t)T * F * sizeof(R), hipMemcpyHostToDevice, ctx->stream));
    launch_update_rows<R>(ctx, d_r, T, p, d_out, nullptr);
    HIP_TRY(ctx, hipGetLastError());
    HIP_TRY(ctx, hipMemcpyAsync(rows.data(), d_out, rows.size() * sizeof(R), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    R* tab = (R*)ip;
    for (int row = 0; row < nrows; ++row) {               // overlapReplace clipping (utils.py:133-161)
        const int t = p - (W - 1) + row;
        if (t >= 0 && t < T) memcpy(tab + (size_t)t * K, rows.data() + (size_t)row * K, (size_t)K * sizeof(R));
    }
    return HSCMP_OK;
}

extern "C" int hscmp_update_inner_products(hscmp_ctx* ctx, void* ip, const void* residual, int T, int p)
{
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, "hscmp_update_inner_products: ctx is NULL");
    if (ctx->dict.dtype < 0) return fail(ctx, HSCMP_ERR_STATE, "hscmp_update_inner_products: no dictionary set");
    NOT_A_SET(ctx, "hscmp_update_inner_products");
    if (!ip || !residual || T <= 0) return fail(ctx, HSCMP_ERR_INVALID, "hscmp_update_inner_products: bad arguments");
    if (p < 0 || p >= T) return fail(ctx, HSCMP_ERR_INVALID, "hscmp_update_inner_products: atom centre %d outside the signal [0, %d)", p, T);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    (void)read_knobs();
    return ctx->dict.dtype == HSCMP_F32 ? run_update_rows<float>(ctx, ip, residual, T, p) : run_update_rows<double>(ctx, ip, residual, T, p);
}

// ---- LoCOMP's table on the device (hsc/modeling.py:1267-1425) -----------------------------------------------------------
// The reference keeps innerProducts[T][K] and the residual as host arrays and edits both around every selected atom.
// Here both live in the context's arena: open = :1293 (innerProducts = convolve1d(residual, D, 'same')), select =
// _selectBestAtoms (:899-982) on the resident table, update = the caller's new residual samples + _updateInnerProducts
// (:1018-1051) for every atom of the re-fitted group, in place.  Per iteration the host moves O(W) samples, not T*K.
// Multi-feature tables (hierarchical levels >= 1) are built row by row from the non-zero cells of each row's window
// (table_rows_sparse_kernel); single-feature inputs are dense and keep the dense kernels.
static bool table_rows_are_sparse(const hscmp_ctx* ctx) { return ctx->dict.F > 1 && ctx->dict.W <= 32767 && ctx->dict.F <= 65535; }
constexpr int kTableRowCap = 1024;             // listed non-zeros per row window (12 KB of LDS in float64); more: dense chain
template <typename R> static void launch_table_rows_sparse(hscmp_ctx* ctx, const R* d_r, int T, int row0, int nrows, int p, R* d_table)
{
    DevParams P{};
    P.B = 1; P.T = T; P.K = ctx->dict.K; P.W = ctx->dict.W; P.F = ctx->dict.F; P.off = (ctx->dict.W - 1) / 2;
    hipLaunchKernelGGL((table_rows_sparse_kernel<R>), dim3(nrows), dim3(kThreads), (size_t)kTableRowCap * (sizeof(R) + 4), ctx->stream,
                       P, d_r, ctx->dict.D.as<const R>(), row0, p, d_table, kTableRowCap);
}

template <typename R> static int run_table_open(hscmp_ctx* ctx, const void* x, int T)
{
    const int K = ctx->dict.K, F = ctx->dict.F;
    int rc;
    if ((rc = epi_buffer(ctx, kArenaTabRes, (size_t)T * F * sizeof(R))) != HSCMP_OK) return rc;
    if ((rc = epi_buffer(ctx, kArenaTable, (size_t)T * K * sizeof(R))) != HSCMP_OK) return rc;
    HIP_TRY(ctx, hipMemcpyAsync(ctx->arena[kArenaTabRes].p, x, (size_t)T * F * sizeof(R), hipMemcpyHostToDevice, ctx->stream));
    // the caller's buffer may be reused as soon as this returns (as hscmp_table_update promises): wait for the upload (not through
    // ev[]: those are the batch-timing events hscmp_last_kernel_ms reads)
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (table_rows_are_sparse(ctx)) launch_table_rows_sparse<R>(ctx, ctx->arena[kArenaTabRes].as<const R>(), T, 0, T, -1, ctx->arena[kArenaTable].as<R>());
    else launch_convolve<R>(ctx, ctx->arena[kArenaTabRes].as<const R>(), T, 1, T, ctx->arena[kArenaTable].as<R>());
    HIP_TRY(ctx, hipGetLastError());
    ctx->tab_T = T;
    return HSCMP_OK;
}

extern "C" int hscmp_table_open(hscmp_ctx* ctx, const void* x, int T)
{
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, "hscmp_table_open: ctx is NULL");
    if (ctx->dict.dtype < 0) return fail(ctx, HSCMP_ERR_STATE, "hscmp_table_open: no dictionary set");
    NOT_A_SET(ctx, "hscmp_table_open");
    if (!x || T <= 0) return fail(ctx, HSCMP_ERR_INVALID, "hscmp_table_open: bad arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    (void)read_knobs();
    ctx->tab_T = 0;
    return ctx->dict.dtype == HSCMP_F32 ? run_table_open<float>(ctx, x, T) : run_table_open<double>(ctx, x, T);
}

extern "C" int hscmp_table_select(hscmp_ctx* ctx, int nb_blocks, int offset, double null_coeff_thres, const void* weights,
                                  int32_t* out_t, int32_t* out_k, void* out_c, int max_out, int32_t* n_out)
{
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, "hscmp_table_select: ctx is NULL");
    NOT_A_SET(ctx, "hscmp_table_select");
    if (ctx->tab_T <= 0) return fail(ctx, HSCMP_ERR_STATE, "hscmp_table_select: no table open (hscmp_table_open)");
    if (!out_t || !out_k || !out_c || !n_out) return fail(ctx, HSCMP_ERR_INVALID, "hscmp_table_select: bad arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const Knobs kn = read_knobs();
    int rc;
    if (ctx->dict.dtype == HSCMP_F32) {
        const float* d_w;
        if ((rc = upload_weights<float>(ctx, weights, ctx->dict.K, &d_w)) != HSCMP_OK) return rc;
        return select_on_device<float>(ctx, kn, ctx->arena[kArenaTable].as<const float>(), d_w, ctx->tab_T, ctx->dict.K, ctx->dict.W, nb_blocks, offset, null_coeff_thres,
                                       out_t, out_k, out_c, max_out, n_out, "hscmp_table_select");
    }
    const double* d_w;
    if ((rc = upload_weights<double>(ctx, weights, ctx->dict.K, &d_w)) != HSCMP_OK) return rc;
    return select_on_device<double>(ctx, kn, ctx->arena[kArenaTable].as<const double>(), d_w, ctx->tab_T, ctx->dict.K, ctx->dict.W, nb_blocks, offset, null_coeff_thres,
                                    out_t, out_k, out_c, max_out, n_out, "hscmp_table_select");
}

extern "C" int hscmp_table_update(hscmp_ctx* ctx, const void* residual_samples, int start, int count, const int32_t* centres, int ncentres)
{
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, "hscmp_table_update: ctx is NULL");
    NOT_A_SET(ctx, "hscmp_table_update");
    if (ctx->tab_T <= 0) return fail(ctx, HSCMP_ERR_STATE, "hscmp_table_update: no table open (hscmp_table_open)");
    const int T = ctx->tab_T;
    if (count < 0 || start < 0 || start + count > T || (count > 0 && !residual_samples) || ncentres < 0 || (ncentres > 0 && !centres))
        return fail(ctx, HSCMP_ERR_INVALID, "hscmp_table_update: bad arguments (start=%d count=%d T=%d)", start, count, T);
    for (int i = 0; i < ncentres; ++i)
        if (centres[i] < 0 || centres[i] >= T) return fail(ctx, HSCMP_ERR_INVALID, "hscmp_table_update: atom centre %d outside the signal [0, %d)", centres[i], T);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t es = esize(ctx->dict.dtype), row = (size_t)ctx->dict.F * es;
    if (count > 0)
        HIP_TRY(ctx, hipMemcpyAsync(ctx->arena[kArenaTabRes].as<char>() + (size_t)start * row, residual_samples, (size_t)count * row, hipMemcpyHostToDevice, ctx->stream));
    const bool sparse_rows_form = table_rows_are_sparse(ctx);
    for (int i = 0; i < ncentres; ++i) {
        if (sparse_rows_form) {
            if (ctx->dict.dtype == HSCMP_F32) launch_table_rows_sparse<float>(ctx, ctx->arena[kArenaTabRes].as<const float>(), T, 0, 2 * ctx->dict.W - 1, centres[i], ctx->arena[kArenaTable].as<float>());
            else launch_table_rows_sparse<double>(ctx, ctx->arena[kArenaTabRes].as<const double>(), T, 0, 2 * ctx->dict.W - 1, centres[i], ctx->arena[kArenaTable].as<double>());
        } else if (ctx->dict.dtype == HSCMP_F32) launch_update_rows<float>(ctx, ctx->arena[kArenaTabRes].as<const float>(), T, centres[i], nullptr, ctx->arena[kArenaTable].as<float>());
        else launch_update_rows<double>(ctx, ctx->arena[kArenaTabRes].as<const double>(), T, centres[i], nullptr, ctx->arena[kArenaTable].as<double>());
    }
    HIP_TRY(ctx, hipGetLastError());
    // the host buffer may be reused as soon as this returns
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return HSCMP_OK;
}

extern "C" int hscmp_table_read(hscmp_ctx* ctx, void* out_table, void* out_residual)
{
    if (!ctx) return fail(nullptr, HSCMP_ERR_INVALID, "hscmp_table_read: ctx is NULL");
    NOT_A_SET(ctx, "hscmp_table_read");
    if (ctx->tab_T <= 0) return fail(ctx, HSCMP_ERR_STATE, "hscmp_table_read: no table open (hscmp_table_open)");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const size_t es = esize(ctx->dict.dtype);
    if (out_table) HIP_TRY(ctx, hipMemcpyAsync(out_table, ctx->arena[kArenaTable].p, (size_t)ctx->tab_T * ctx->dict.K * es, hipMemcpyDeviceToHost, ctx->stream));
    if (out_residual) HIP_TRY(ctx, hipMemcpyAsync(out_residual, ctx->arena[kArenaTabRes].p, (size_t)ctx->tab_T * ctx->dict.F * es, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return HSCMP_OK;
}

extern "C" int hscmp_wide_plan(int K, int W, int F, hscmp_dtype dtype, int has_weights, int B, int T, const hscmp_params* params, int32_t* out4)
{
    if (!params || !out4 || K <= 0 || W <= 0 || F <= 0 || B <= 0 || T <= 0) return fail(nullptr, HSCMP_ERR_INVALID, "hscmp_wide_plan: bad arguments");
    if (dtype != HSCMP_F32 && dtype != HSCMP_F64) return fail(nullptr, HSCMP_ERR_INVALID, "hscmp_wide_plan: bad dtype %d", (int)dtype);
    Knobs kn{};
    kn.slot_hash_min = kSlotHashMin; kn.locomp_group_cap = kLocompGroupCap; kn.locomp_ahead = 7;
    DevParams P;
    const int rc = make_params_g(nullptr, kn, K, W, F, B, T, params, &P);
    if (rc) return rc;
    const WideShape ws = wide_shape(P, dtype == HSCMP_F32, has_weights != 0, false, false);
    out4[0] = ws.can ? 1 : 0; out4[1] = ws.by_default ? 1 : 0; out4[2] = P.maxsel; out4[3] = (int32_t)ws.control_lds;
    return HSCMP_OK;
}

extern "C" int hscmp_wide_counters(hscmp_ctx* ctx, int32_t* out4)
{
    if (!ctx || !out4) return fail(ctx, HSCMP_ERR_INVALID, "hscmp_wide_counters: NULL argument");
    const bool wide = ctx->have_batch && ctx->plan.loop == EncodePlan::kLoopWide;
    out4[0] = wide ? ctx->wide_steps : 0; out4[1] = wide ? ctx->wide_polls : 0; out4[2] = wide ? ctx->wide_worked : 0; out4[3] = wide ? ctx->B : 0;
    return HSCMP_OK;
}
