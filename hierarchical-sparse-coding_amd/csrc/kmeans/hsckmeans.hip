// hsckmeans.hip -- libhsckmeans.so: one iteration of the convolutional k-means learner (hsc/modeling.py:454-503)
// for a batch of learners on gfx950, C ABI in include/hsckmeans.h.  DESIGN.md section 14.
//
// The signals and window starts are uploaded once (hsckmeans_set_data); a step uploads the dictionaries and runs:
//   1. assign_kernel: the 'valid' correlation of every 2W-sample window with every atom on the matrix cores
//      (v_mfma_f64_16x16x4_f64 / v_mfma_f32_16x16x4_f32, both bit-exact k-ordered fma chains).  The product is
//      Dimg [16 atoms][q] x im2col(window) [q][16 columns], q = f * W + w in the pinned order of
//      hscmp_assign_windows (f outer, w inner), so every output is the same chain from +0 as that kernel's.
//      A workgroup takes WPB windows (their W+1 positions laid end to end: the columns), stages them in LDS
//      feature-major in chunks of features, and streams the dictionary image in k-steps from global memory.
//      The flat arg-max of |c| (lowest o = t * K + k among equals) goes through two LDS atomics per window:
//      the largest score's bits, then the smallest o holding it.
//   2. norm_kernel: ||patch|| of every window's matched patch, numpy's pairwise summation of the squares.
//   3. member_kernel: one wave per centroid lists its members in ascending window order (ballot + popcount).
//   4. sum_kernel: one thread per (centroid, element) sums patch / ||patch|| over the members in list order.
// Compiled with -ffp-contract=off: no product is fused into a sum outside the explicit MFMA chains.
#include "../../../include/hsckmeans.h"
#include "../common/hsc_lib.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int kThreads = 256;           // assign_kernel: 4 waves
constexpr int kTilesPerWave = 4;        // column tiles of 16 per wave: WPB * (W + 1) <= 4 * 4 * 16 columns
constexpr int kMaxWPB = 64;
constexpr int kMaxW = 255;              // W + 1 positions must fit the 256 columns of one workgroup
constexpr size_t kStageBytes = 48 * 1024;     // staged window features per workgroup

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

template <typename R> struct Mfma;
template <> struct Mfma<float> {
    typedef f32x4 acc_t;
    __device__ static acc_t step(float a, float b, acc_t c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }
    __device__ static int row(int lane, int r) { return 4 * (lane >> 4) + r; }           // standard C/D map
    __device__ static unsigned long long bits(float v) { return (unsigned long long)__float_as_uint(v); }
};
template <> struct Mfma<double> {
    typedef f64x4 acc_t;
    __device__ static acc_t step(double a, double b, acc_t c) { return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0); }
    __device__ static int row(int lane, int r) { return (lane >> 4) + 4 * r; }           // the f64 form's own map
    __device__ static unsigned long long bits(double v) { return (unsigned long long)__double_as_longlong(v); }
};

struct AssignArgs {
    int T, F, N, W, K, G, Sp, Q, P, WPB, CT, FC, SC, want;
    const int* starts;      // [B][N]
    const int* mode;        // [B]
    int* out_t;             // [B][N]
    int* out_k;             // [B][N]
};

// grid = (ceil(N / WPB), B), block = kThreads; dynamic LDS: WPB * FC * 2W elements of R
template <typename X, typename R>
__global__ __launch_bounds__(kThreads) void assign_kernel(const X* __restrict__ x, const R* __restrict__ img, AssignArgs a)
{
    typedef Mfma<R> M;
    typedef typename M::acc_t acc_t;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    R* win = reinterpret_cast<R*>(smem);
    __shared__ unsigned long long s_max[kMaxWPB];
    __shared__ int s_o[kMaxWPB];

    const int b = blockIdx.y;
    if (a.mode[b] != a.want) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, kk = lane >> 4, j = lane & 15;
    const int W = a.W, F = a.F, K = a.K, L2 = 2 * W;
    const int n0 = blockIdx.x * a.WPB, nwin = min(a.WPB, a.N - n0);
    const X* xb = x + (size_t)b * a.T * F;
    const int* sb = a.starts + (size_t)b * a.N + n0;
    if (tid < kMaxWPB) {
        s_max[tid] = 0ull;
        s_o[tid] = INT_MAX;
    }

    int lbase[kTilesPerWave], lnw[kTilesPerWave], lt[kTilesPerWave];
    bool lvalid[kTilesPerWave];
    R best[kTilesPerWave];
    int bo[kTilesPerWave];
#pragma unroll
    for (int i = 0; i < kTilesPerWave; ++i) {
        const int ct = wave + 4 * i, col = ct * 16 + j;
        int nw = col / a.P, t = col - nw * a.P;
        lvalid[i] = ct < a.CT && nw < nwin;
        if (!lvalid[i]) nw = t = 0;                       // a staged window: read, never reported
        lnw[i] = nw;
        lt[i] = t;
        lbase[i] = nw * a.FC * L2 + t;
        best[i] = (R)-1;
        bo[i] = INT_MAX;
    }

    for (int g = 0; g < a.G; ++g) {
        acc_t acc[kTilesPerWave];
#pragma unroll
        for (int i = 0; i < kTilesPerWave; ++i) acc[i] = acc_t{0, 0, 0, 0};
        const R* ip = img + ((size_t)b * a.G + g) * a.Sp * 64 + lane;
        for (int s0 = 0; s0 < a.Sp; s0 += a.SC) {
            const int s1 = min(a.Sp, s0 + a.SC);
            const int f_lo = min(F - 1, (4 * s0) / W), f_hi = min(F - 1, (4 * s1 - 1) / W), nf = f_hi - f_lo + 1;
            __syncthreads();
            for (int e = tid; e < nwin * L2 * nf; e += kThreads) {     // win[nw][fc][tt] = x[start + tt][f_lo + fc]
                const int fc = e % nf, r = e / nf, tt = r % L2, nw = r / L2;
                win[(nw * a.FC + fc) * L2 + tt] = (R)xb[(size_t)(sb[nw] + tt) * F + f_lo + fc];
            }
            __syncthreads();
            int q = 4 * s0 + kk, f = q / W, w = q - f * W;
            for (int s = s0; s < s1; ++s) {
                const R av = ip[(size_t)s * 64];
                const bool live = q < a.Q;                      // contraction padded to a multiple of 4 with zeros
                const int off = (f - f_lo) * L2 + w;
#pragma unroll
                for (int i = 0; i < kTilesPerWave; ++i)
                    if (wave + 4 * i < a.CT) {
                        const R bv = live ? win[lbase[i] + off] : (R)0;
                        acc[i] = M::step(av, bv, acc[i]);
                    }
                q += 4;
                w += 4;
                while (w >= W) {
                    w -= W;
                    ++f;
                }
            }
        }
#pragma unroll
        for (int i = 0; i < kTilesPerWave; ++i)
            if (lvalid[i])
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int k = 16 * g + M::row(lane, r);
                    if (k >= K) continue;
                    const R sc = fabs(acc[i][r]);
                    const int o = lt[i] * K + k;
                    if (sc > best[i] || (sc == best[i] && o < bo[i])) {    // NaN: never taken
                        best[i] = sc;
                        bo[i] = o;
                    }
                }
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kTilesPerWave; ++i)
        if (lvalid[i] && bo[i] != INT_MAX) atomicMax(&s_max[lnw[i]], M::bits(best[i]));    // scores >= 0: bits order
    __syncthreads();
#pragma unroll
    for (int i = 0; i < kTilesPerWave; ++i)
        if (lvalid[i] && bo[i] != INT_MAX && M::bits(best[i]) == s_max[lnw[i]]) atomicMin(&s_o[lnw[i]], bo[i]);
    __syncthreads();
    if (tid < nwin) {
        const int o = s_o[tid] == INT_MAX ? 0 : s_o[tid];
        a.out_t[(size_t)b * a.N + n0 + tid] = o / K;
        a.out_k[(size_t)b * a.N + n0 + tid] = o % K;
    }
}

// numpy's pairwise summation (PW_BLOCKSIZE 128, unroll 8) of the squares of p[0 .. n)
template <typename X>
__device__ X pairwise_leaf(const X* __restrict__ p, int n)
{
    if (n < 8) {
        X res = (X)0;
        for (int i = 0; i < n; ++i) res = res + p[i] * p[i];
        return res;
    }
    X r[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) r[u] = p[u] * p[u];
    int i = 8;
    for (; i < n - (n % 8); i += 8)
#pragma unroll
        for (int u = 0; u < 8; ++u) r[u] = r[u] + p[i + u] * p[i + u];
    X res = ((r[0] + r[1]) + (r[2] + r[3])) + ((r[4] + r[5]) + (r[6] + r[7]));
    for (; i < n; ++i) res = res + p[i] * p[i];
    return res;
}

template <typename X>
__device__ X pairwise_sumsq(const X* __restrict__ p, int n)
{
    // post-order walk of numpy's split tree: op 0 = evaluate [off, off + len), op 1 = add the top two values
    int st_off[64], st_len[64];
    unsigned char st_op[64];
    X val[32];
    int sp = 0, nv = 0;
    st_off[sp] = 0; st_len[sp] = n; st_op[sp] = 0; ++sp;
    while (sp > 0) {
        --sp;
        const int off = st_off[sp], len = st_len[sp];
        if (st_op[sp] == 1) {
            const X rhs = val[--nv];
            const X lhs = val[--nv];
            val[nv++] = lhs + rhs;
        } else if (len <= 128) {
            val[nv++] = pairwise_leaf(p + off, len);
        } else {
            int n2 = len / 2;
            n2 -= n2 % 8;
            st_op[sp] = 1; ++sp;
            st_off[sp] = off + n2; st_len[sp] = len - n2; st_op[sp] = 0; ++sp;
            st_off[sp] = off; st_len[sp] = n2; st_op[sp] = 0; ++sp;
        }
    }
    return val[0];
}

// grid = (ceil(N / 256), B): norm[b][n] and the patch offset pofs[b][n] = (start + t) * F
template <typename X>
__global__ __launch_bounds__(256) void norm_kernel(const X* __restrict__ x, int T, int F, int N, int W, const int* __restrict__ starts,
                                                   const int* __restrict__ mode, const int* __restrict__ at,
                                                   X* __restrict__ norm, int* __restrict__ pofs)
{
    const int b = blockIdx.y, n = blockIdx.x * 256 + threadIdx.x;
    if (mode[b] == HSCKMEANS_SKIP || n >= N) return;
    const size_t i = (size_t)b * N + n;
    const int po = (starts[i] + at[i]) * F;
    const X ss = pairwise_sumsq(x + (size_t)b * T * F + po, W * F);
    const X nr = sqrt(ss);
    norm[i] = nr > (X)0 ? nr : (X)1;                   // normalize(): np.where(norms > 0, norms, 1)
    pofs[i] = po;
}

// grid = (K, B), block = one wave: members of centroid c in ascending window order
__global__ __launch_bounds__(64) void member_kernel(int N, int K, const int* __restrict__ mode, const int* __restrict__ ak,
                                                    int* __restrict__ members, int* __restrict__ count, int* __restrict__ nonzero)
{
    const int c = blockIdx.x, b = blockIdx.y, lane = threadIdx.x;
    if (mode[b] == HSCKMEANS_SKIP) return;
    const int* kb = ak + (size_t)b * N;
    int* list = members + ((size_t)b * K + c) * N;
    int cnt = 0;
    for (int c0 = 0; c0 < N; c0 += 64) {
        const int n = c0 + lane;
        const bool in = n < N && kb[n] == c;
        const unsigned long long mask = __ballot(in);
        if (in) list[cnt + __popcll(mask & ((1ull << lane) - 1ull))] = n;
        cnt += __popcll(mask);
    }
    if (lane == 0) {
        count[(size_t)b * K + c] = cnt;
        nonzero[(size_t)b * K + c] = cnt - (kb[0] == c ? 1 : 0) > 0 ? 1 : 0;
    }
}

// grid = (ceil(K * W * F / 256), B): S[b][c][e] = sum over the members, in list order, of patch / ||patch||
template <typename X>
__global__ __launch_bounds__(256) void sum_kernel(const X* __restrict__ x, int T, int F, int N, int W, int K, const int* __restrict__ mode,
                                                  const int* __restrict__ members, const int* __restrict__ count,
                                                  const X* __restrict__ norm, const int* __restrict__ pofs, X* __restrict__ S)
{
    const int b = blockIdx.y, Q = W * F;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (mode[b] == HSCKMEANS_SKIP || e >= K * Q) return;
    const int c = e / Q, el = e - c * Q;
    const int m = count[(size_t)b * K + c];
    const int* list = members + ((size_t)b * K + c) * N;
    const X* xb = x + (size_t)b * T * F + el;
    const X* nb = norm + (size_t)b * N;
    const int* pb = pofs + (size_t)b * N;
    X acc = (X)0;
    if (m > 0) {
        const int n = list[0];
        acc = xb[pb[n]] / nb[n];
    }
    int i = 1;
    constexpr int U = 16;                              // loads in flight ahead of the sequential adds
    for (; i + U <= m; i += U) {
        X v[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int n = list[i + u];
            v[u] = xb[pb[n]] / nb[n];
        }
#pragma unroll
        for (int u = 0; u < U; ++u) acc = acc + v[u];
    }
    for (; i < m; ++i) {
        const int n = list[i];
        acc = acc + xb[pb[n]] / nb[n];
    }
    S[(size_t)b * K * Q + e] = acc;
}

}  // namespace

static_assert(HSCKMEANS_OK == hsc::OK && HSCKMEANS_ERR_INVALID == hsc::ERR_INVALID && HSCKMEANS_ERR_NO_DEVICE == hsc::ERR_NO_DEVICE &&
              HSCKMEANS_ERR_HIP == hsc::ERR_HIP && HSCKMEANS_ERR_UNSUPPORTED == hsc::ERR_UNSUPPORTED &&
              HSCKMEANS_ERR_ALLOC == hsc::ERR_ALLOC, "include/hsckmeans.h and common/hsc_lib.h disagree on a status");

struct HSC_HIDDEN hsckmeans_ctx : hsc::CtxBase {
    hipEvent_t ev[5] = {};
    // data (set_data)
    int dtype = -1, B = 0, T = 0, F = 0, N = 0, W = 0;
    void* d_x = nullptr;
    int* d_starts = nullptr;
    // step buffers (grown, never shrunk)
    enum { kImg32, kImg64, kMode, kT, kK, kNorm, kPofs, kMembers, kCount, kNonzero, kSums, kBufs };
    hsc::Buffers<kBufs> buf;
    std::vector<float> img32;
    std::vector<double> img64;

    ~hsckmeans_ctx()
    {
        if (d_x) (void)hipFree(d_x);
        if (d_starts) (void)hipFree(d_starts);
    }
};

using hsc::fail;

extern "C" int hsckmeans_version(void) { return 1; }

extern "C" const char* hsckmeans_last_error(hsckmeans_ctx* ctx) { return hsc::last_error(ctx); }

extern "C" int hsckmeans_create(hsckmeans_ctx** out, int device_id) { return hsc::create(out, device_id, "hsckmeans_create"); }

extern "C" void hsckmeans_destroy(hsckmeans_ctx* ctx) { hsc::destroy(ctx); }

extern "C" int hsckmeans_set_data(hsckmeans_ctx* ctx, const void* x, int dtype, int B, int T, int F, const int64_t* starts,
                                  int N, int W)
{
    if (!ctx) return fail(nullptr, HSCKMEANS_ERR_INVALID, "hsckmeans_set_data: ctx is NULL");
    if (!x || !starts) return fail(ctx, HSCKMEANS_ERR_INVALID, "hsckmeans_set_data: x or starts is NULL");
    if (dtype != HSCKMEANS_F32 && dtype != HSCKMEANS_F64) return fail(ctx, HSCKMEANS_ERR_INVALID, "hsckmeans_set_data: bad dtype %d", dtype);
    if (B < 1 || T < 1 || F < 1 || N < 1 || W < 1)
        return fail(ctx, HSCKMEANS_ERR_INVALID, "hsckmeans_set_data: bad shape B = %d, T = %d, F = %d, N = %d, W = %d", B, T, F, N, W);
    if (W > kMaxW) return fail(ctx, HSCKMEANS_ERR_UNSUPPORTED, "hsckmeans_set_data: W = %d exceeds the limit of %d", W, kMaxW);
    if (2 * W >= T) return fail(ctx, HSCKMEANS_ERR_INVALID, "hsckmeans_set_data: windows of 2W = %d samples need T > %d (T = %d)", 2 * W, 2 * W, T);
    if ((int64_t)T * F > INT_MAX) return fail(ctx, HSCKMEANS_ERR_UNSUPPORTED, "hsckmeans_set_data: T * F = %lld exceeds 2^31 - 1", (long long)T * F);
    std::vector<int> s32((size_t)B * N);
    for (size_t i = 0; i < s32.size(); ++i) {
        if (starts[i] < 0 || starts[i] > T - 2 * W)
            return fail(ctx, HSCKMEANS_ERR_INVALID, "hsckmeans_set_data: start %lld of window %zu is outside [0, %d]", (long long)starts[i], i, T - 2 * W);
        s32[i] = (int)starts[i];
    }
    HSC_TRY(hipSetDevice(ctx->device));
    HSC_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->d_x) (void)hipFree(ctx->d_x);
    if (ctx->d_starts) (void)hipFree(ctx->d_starts);
    ctx->d_x = nullptr;
    ctx->d_starts = nullptr;
    ctx->dtype = -1;
    const size_t bx = (size_t)B * T * F * (dtype == HSCKMEANS_F32 ? 4 : 8), bs = s32.size() * sizeof(int);
    hipError_t e = hipMalloc(&ctx->d_x, bx);
    if (e == hipSuccess) e = hipMalloc((void**)&ctx->d_starts, bs);
    if (e != hipSuccess) return fail(ctx, HSCKMEANS_ERR_ALLOC, "hsckmeans_set_data: hipMalloc failed (%s)", hipGetErrorString(e));
    HSC_TRY(hipMemcpyAsync(ctx->d_x, x, bx, hipMemcpyHostToDevice, ctx->stream));
    HSC_TRY(hipMemcpyAsync(ctx->d_starts, s32.data(), bs, hipMemcpyHostToDevice, ctx->stream));
    HSC_TRY(hipStreamSynchronize(ctx->stream));
    ctx->dtype = dtype;
    ctx->B = B; ctx->T = T; ctx->F = F; ctx->N = N; ctx->W = W;
    return HSCKMEANS_OK;
}

template <typename X, typename R>
static int launch_assign(hsckmeans_ctx* ctx, const void* img, const AssignArgs& args, int WPB, size_t lds)
{
    dim3 grid((ctx->N + WPB - 1) / WPB, ctx->B);
    hipLaunchKernelGGL((assign_kernel<X, R>), grid, dim3(kThreads), lds, ctx->stream, (const X*)ctx->d_x, (const R*)img, args);
    HSC_TRY(hipGetLastError());
    return HSCKMEANS_OK;
}

template <typename X>
static int launch_centroids(hsckmeans_ctx* ctx, int K)
{
    const int B = ctx->B, N = ctx->N, Q = ctx->W * ctx->F;
    const int* mode = (const int*)ctx->buf[hsckmeans_ctx::kMode];
    const int* at = (const int*)ctx->buf[hsckmeans_ctx::kT];
    const int* ak = (const int*)ctx->buf[hsckmeans_ctx::kK];
    X* norm = (X*)ctx->buf[hsckmeans_ctx::kNorm];
    int* pofs = (int*)ctx->buf[hsckmeans_ctx::kPofs];
    int* members = (int*)ctx->buf[hsckmeans_ctx::kMembers];
    int* count = (int*)ctx->buf[hsckmeans_ctx::kCount];
    int* nonzero = (int*)ctx->buf[hsckmeans_ctx::kNonzero];
    hipLaunchKernelGGL((norm_kernel<X>), dim3((N + 255) / 256, B), dim3(256), 0, ctx->stream, (const X*)ctx->d_x, ctx->T, ctx->F, N,
                       ctx->W, ctx->d_starts, mode, at, norm, pofs);
    HSC_TRY(hipGetLastError());
    hipLaunchKernelGGL(member_kernel, dim3(K, B), dim3(64), 0, ctx->stream, N, K, mode, ak, members, count, nonzero);
    HSC_TRY(hipGetLastError());
    hipLaunchKernelGGL((sum_kernel<X>), dim3((unsigned)(((size_t)K * Q + 255) / 256), B), dim3(256), 0, ctx->stream, (const X*)ctx->d_x,
                       ctx->T, ctx->F, N, ctx->W, K, mode, members, count, norm, pofs, (X*)ctx->buf[hsckmeans_ctx::kSums]);
    HSC_TRY(hipGetLastError());
    return HSCKMEANS_OK;
}

extern "C" int hsckmeans_step(hsckmeans_ctx* ctx, const double* D, int K, const int32_t* mode, int32_t* out_t, int32_t* out_k,
                              int32_t* out_count, int32_t* out_nonzero, void* out_sums, double* timing_ms)
{
    if (!ctx) return fail(nullptr, HSCKMEANS_ERR_INVALID, "hsckmeans_step: ctx is NULL");
    if (ctx->dtype < 0) return fail(ctx, HSCKMEANS_ERR_STATE, "hsckmeans_step: no data set");
    if (!D || !mode || !out_t || !out_k || !out_count || !out_nonzero || !out_sums)
        return fail(ctx, HSCKMEANS_ERR_INVALID, "hsckmeans_step: NULL argument");
    const int B = ctx->B, N = ctx->N, W = ctx->W, F = ctx->F, Q = W * F;
    if (K < 1) return fail(ctx, HSCKMEANS_ERR_INVALID, "hsckmeans_step: K = %d", K);
    if ((int64_t)K * Q > INT_MAX / 2 || (int64_t)K * N > INT_MAX / 2)
        return fail(ctx, HSCKMEANS_ERR_UNSUPPORTED, "hsckmeans_step: K = %d is too large for this shape", K);
    bool any32 = false, any64 = false;
    for (int b = 0; b < B; ++b) {
        if (mode[b] < HSCKMEANS_SKIP || mode[b] > HSCKMEANS_ASSIGN_F64)
            return fail(ctx, HSCKMEANS_ERR_INVALID, "hsckmeans_step: bad mode %d of learner %d", mode[b], b);
        if (mode[b] == HSCKMEANS_ASSIGN_F32 && ctx->dtype == HSCKMEANS_F64)
            return fail(ctx, HSCKMEANS_ERR_INVALID, "hsckmeans_step: learner %d: float64 data needs a float64 assignment", b);
        any32 |= mode[b] == HSCKMEANS_ASSIGN_F32;
        any64 |= mode[b] == HSCKMEANS_ASSIGN_F64;
    }
    if (timing_ms)
        for (int i = 0; i < HSCKMEANS_TIMES; ++i) timing_ms[i] = 0.0;
    if (!any32 && !any64) return HSCKMEANS_OK;

    // dictionary images: img[b][g][s][lane] = D[b][16g + (lane & 15)][w][f], q = 4s + (lane >> 4) = f * W + w
    const int G = (K + 15) / 16, Sp = (Q + 3) / 4;
    const size_t per = (size_t)G * Sp * 64;
    if (any32) ctx->img32.assign(per * B, 0.0f);
    if (any64) ctx->img64.assign(per * B, 0.0);
    for (int b = 0; b < B; ++b) {
        if (mode[b] == HSCKMEANS_SKIP) continue;
        const double* Db = D + (size_t)b * K * Q;
        for (int g = 0; g < G; ++g)
            for (int s = 0; s < Sp; ++s)
                for (int l = 0; l < 64; ++l) {
                    const int k = 16 * g + (l & 15), q = 4 * s + (l >> 4);
                    if (k >= K || q >= Q) continue;
                    const int f = q / W, w = q - f * W;
                    const double v = Db[(size_t)k * Q + w * F + f];
                    const size_t o = per * b + ((size_t)g * Sp + s) * 64 + l;
                    if (mode[b] == HSCKMEANS_ASSIGN_F32) ctx->img32[o] = (float)v;
                    else ctx->img64[o] = v;
                }
    }

    HSC_TRY(hipSetDevice(ctx->device));
    const size_t xs = ctx->dtype == HSCKMEANS_F32 ? 4 : 8;
    const size_t bytes[hsckmeans_ctx::kBufs] = {
        any32 ? per * B * 4 : 0, any64 ? per * B * 8 : 0, (size_t)B * sizeof(int), (size_t)B * N * sizeof(int),
        (size_t)B * N * sizeof(int), (size_t)B * N * xs, (size_t)B * N * sizeof(int), (size_t)B * K * N * sizeof(int),
        (size_t)B * K * sizeof(int), (size_t)B * K * sizeof(int), (size_t)B * K * Q * xs};
    if (int rc = ctx->buf.ensure(ctx, bytes, "hsckmeans_step")) return rc;
    hipStream_t st = ctx->stream;
    HSC_TRY(hipEventRecord(ctx->ev[0], st));
    if (any32) HSC_TRY(hipMemcpyAsync(ctx->buf[hsckmeans_ctx::kImg32], ctx->img32.data(), per * B * 4, hipMemcpyHostToDevice, st));
    if (any64) HSC_TRY(hipMemcpyAsync(ctx->buf[hsckmeans_ctx::kImg64], ctx->img64.data(), per * B * 8, hipMemcpyHostToDevice, st));
    HSC_TRY(hipMemcpyAsync(ctx->buf[hsckmeans_ctx::kMode], mode, (size_t)B * sizeof(int), hipMemcpyHostToDevice, st));
    HSC_TRY(hipEventRecord(ctx->ev[1], st));

    // launch shape: WPB windows per workgroup so that their columns fit 16 tiles; features staged FC at a time
    const int P = W + 1;
    const int WPB = std::max(1, std::min(kMaxWPB, (4 * kTilesPerWave * 16) / P));
    const int CT = (WPB * P + 15) / 16;
    int rc;
    for (int pass = 0; pass < 2; ++pass) {
        const bool f64 = pass == 1;
        if (!(f64 ? any64 : any32)) continue;
        const size_t rs = f64 ? 8 : 4;
        int FC = (int)std::max<size_t>(1, kStageBytes / ((size_t)WPB * 2 * W * rs));
        FC = std::min(FC, F);
        int SC = FC == F ? Sp : ((FC - 1) * W + 1) / 4;
        if (SC < 1) {                                  // W < 3 with a single staged feature: stage two
            FC = std::min(F, 2);
            SC = FC == F ? Sp : ((FC - 1) * W + 1) / 4;
            if (SC < 1) return fail(ctx, HSCKMEANS_ERR_UNSUPPORTED, "hsckmeans_step: W = %d, F = %d cannot be staged", W, F);
        }
        AssignArgs args;
        args.T = ctx->T; args.F = F; args.N = N; args.W = W; args.K = K; args.G = G; args.Sp = Sp; args.Q = Q; args.P = P;
        args.WPB = WPB; args.CT = CT; args.FC = FC; args.SC = SC;
        args.want = f64 ? HSCKMEANS_ASSIGN_F64 : HSCKMEANS_ASSIGN_F32;
        args.starts = ctx->d_starts;
        args.mode = (const int*)ctx->buf[hsckmeans_ctx::kMode];
        args.out_t = (int*)ctx->buf[hsckmeans_ctx::kT];
        args.out_k = (int*)ctx->buf[hsckmeans_ctx::kK];
        const size_t lds = (size_t)WPB * FC * 2 * W * rs;
        if (!f64) rc = launch_assign<float, float>(ctx, ctx->buf[hsckmeans_ctx::kImg32], args, WPB, lds);
        else if (ctx->dtype == HSCKMEANS_F32) rc = launch_assign<float, double>(ctx, ctx->buf[hsckmeans_ctx::kImg64], args, WPB, lds);
        else rc = launch_assign<double, double>(ctx, ctx->buf[hsckmeans_ctx::kImg64], args, WPB, lds);
        if (rc != HSCKMEANS_OK) return rc;
    }
    HSC_TRY(hipEventRecord(ctx->ev[2], st));
    rc = ctx->dtype == HSCKMEANS_F32 ? launch_centroids<float>(ctx, K) : launch_centroids<double>(ctx, K);
    if (rc != HSCKMEANS_OK) return rc;
    HSC_TRY(hipEventRecord(ctx->ev[3], st));
    HSC_TRY(hipMemcpyAsync(out_t, ctx->buf[hsckmeans_ctx::kT], (size_t)B * N * sizeof(int), hipMemcpyDeviceToHost, st));
    HSC_TRY(hipMemcpyAsync(out_k, ctx->buf[hsckmeans_ctx::kK], (size_t)B * N * sizeof(int), hipMemcpyDeviceToHost, st));
    HSC_TRY(hipMemcpyAsync(out_count, ctx->buf[hsckmeans_ctx::kCount], (size_t)B * K * sizeof(int), hipMemcpyDeviceToHost, st));
    HSC_TRY(hipMemcpyAsync(out_nonzero, ctx->buf[hsckmeans_ctx::kNonzero], (size_t)B * K * sizeof(int), hipMemcpyDeviceToHost, st));
    HSC_TRY(hipMemcpyAsync(out_sums, ctx->buf[hsckmeans_ctx::kSums], (size_t)B * K * Q * xs, hipMemcpyDeviceToHost, st));
    HSC_TRY(hipEventRecord(ctx->ev[4], st));
    HSC_TRY(hipStreamSynchronize(st));
    if (timing_ms && (rc = hsc::add_times(ctx, HSCKMEANS_TIMES, timing_ms)) != HSCKMEANS_OK) return rc;     // (zeroed above)
    return HSCKMEANS_OK;
}
