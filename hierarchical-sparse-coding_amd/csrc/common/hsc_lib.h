// hsc_lib.h -- the host shell of the satellite libraries (libhscnmf.so, libhscksvd.so, libhsckmeans.so): error state,
// context create / destroy, grow-only device buffers and the event-timing readback.  DESIGN.md section 10.
//
// Each library includes it once, from its one source file; everything here has internal linkage, so no library
// exports more than its extern "C" entry points.  A library context (`struct HSC_HIDDEN <lib>_ctx : hsc::CtxBase`,
// hidden so that its out-of-line destructor is not exported either) adds its own `hipEvent_t ev[N]` (the events
// create makes) and its device memory, which its destructor frees.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <string>

#define HSC_HIDDEN __attribute__((visibility("hidden")))

namespace {
namespace hsc {

// the status values every satellite header repeats (each library static_asserts its own against these)
enum { OK = 0, ERR_INVALID = -1, ERR_NO_DEVICE = -2, ERR_HIP = -3, ERR_UNSUPPORTED = -5, ERR_ALLOC = -6 };

thread_local std::string g_err;    // the last error of a call without a context (create, ctx = NULL)

struct CtxBase {
    int device = 0;
    hipStream_t stream = nullptr;
    std::string err;
};

__attribute__((format(printf, 3, 4))) int fail(CtxBase* ctx, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    (ctx ? ctx->err : g_err) = buf;
    return code;
}

const char* last_error(const CtxBase* ctx) { return ctx ? ctx->err.c_str() : g_err.c_str(); }

// syncs and frees the stream and events; `delete` then runs the context's destructor, which frees its device memory
template <typename C>
void destroy(C* ctx)
{
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    for (hipEvent_t ev : ctx->ev) if (ev) (void)hipEventDestroy(ev);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

// device count and range, then a non-blocking stream and the context's events; `fn` ("hscnmf_create") heads the messages
template <typename C>
int create(C** out, int device_id, const char* fn)
{
    if (!out) return fail(nullptr, ERR_INVALID, "%s: out is NULL", fn);
    *out = nullptr;
    int n = 0;
    hipError_t e = hipGetDeviceCount(&n);
    if (e != hipSuccess || n <= 0) return fail(nullptr, ERR_NO_DEVICE, "%s: no HIP device visible (%s)", fn, hipGetErrorString(e));
    if (device_id < 0 || device_id >= n)
        return fail(nullptr, ERR_INVALID, "%s: device %d out of range (%d devices)", fn, device_id, n);
    C* ctx = new C();
    ctx->device = device_id;
    e = hipSetDevice(device_id);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking);
    for (hipEvent_t& ev : ctx->ev) if (e == hipSuccess) e = hipEventCreate(&ev);
    if (e != hipSuccess) {
        int rc = fail(nullptr, ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
        destroy(ctx);
        return rc;
    }
    *out = ctx;
    return OK;
}

// a HIP call that fails returns ERR_HIP from the enclosing function, `ctx` naming its context
#define HSC_TRY(expr)                                                                                         \
    do {                                                                                                      \
        hipError_t e_ = (expr);                                                                               \
        if (e_ != hipSuccess) return hsc::fail(ctx, hsc::ERR_HIP, "%s: %s", #expr, hipGetErrorString(e_));    \
    } while (0)

// adds the milliseconds between the context's events i and i + 1 to ms[i], i < n (the events have completed)
template <typename C>
int add_times(C* ctx, int n, double* ms)
{
    for (int i = 0; i < n; ++i) {
        float t = 0.f;
        HSC_TRY(hipEventElapsedTime(&t, ctx->ev[i], ctx->ev[i + 1]));
        ms[i] += t;
    }
    return OK;
}

// N device buffers, each grown to the largest size asked of it and kept until the context goes
template <int N>
struct Buffers {
    void* p[N] = {};
    size_t cap[N] = {};

    ~Buffers() { for (void* q : p) if (q) (void)hipFree(q); }
    void* operator[](int i) const { return p[i]; }

    // buffer i of at least bytes[i] for every i; `fn` names the entry point in the ERR_ALLOC message
    int ensure(CtxBase* ctx, const size_t (&bytes)[N], const char* fn)
    {
        for (int i = 0; i < N; ++i) {
            const size_t want = std::max<size_t>(bytes[i], 256);
            if (cap[i] >= want) continue;
            if (p[i]) (void)hipFree(p[i]);
            p[i] = nullptr;
            cap[i] = 0;
            hipError_t e = hipMalloc(&p[i], want);
            if (e != hipSuccess)
                return fail(ctx, ERR_ALLOC, "%s: hipMalloc of %zu bytes failed (%s)", fn, bytes[i], hipGetErrorString(e));
            cap[i] = want;
        }
        return OK;
    }
};

}  // namespace hsc
}  // namespace
