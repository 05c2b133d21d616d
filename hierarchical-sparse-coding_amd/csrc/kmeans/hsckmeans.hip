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
// Steps 3 and 4 are centroid plan 1.  Plan 2 (wide) returns the same bits from a stable partition
// of the windows by centroid (hist_kernel, scan_kernel, place_kernel: one [N] index array with K + 1 offsets) and
// wide_sum_kernel: one workgroup per (centroid, tile of 256 elements) that stages its members' rows, divided by their
// norms, through a double-buffered LDS ring and adds them in list order, one lane per element.
// hsckmeans_set_corpus stacks signals of different lengths as one learner's data [rows][F]: every kernel reads it as
// B = 1, T = rows, with window starts that are stacked rows.  hsckmeans_set_corpus_sparse takes the stack as CSR and
// holds the window stack [N * 2W][F] instead: gather_kernel builds every window's dense block from the entries the
// windows cover, and the step's kernels read it with window n at row n * 2W.
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

// ---- plan 2: the wide centroid half ----------------------------------------------------------------------------------
constexpr int kChunk = HSCKMEANS_WIDE_CHUNK_WINDOWS;     // windows per chunk: 4 waves x 4 segments of 64
constexpr int kRing = HSCKMEANS_WIDE_RING_ROWS;          // kRing * 256 elements per ring half
constexpr int kSumThreads = 1024;                        // wide_sum_kernel: 16 waves stage, the first tw lanes add
constexpr int kLoads = kRing * 256 / kSumThreads;        // elements per thread and batch
constexpr int kWideMaxK = HSCKMEANS_WIDE_MAX_K;
static_assert(kChunk == 4 * 4 * 64, "place_kernel: 4 waves, 4 segments of 64 windows each");

// an assignment is in [0, K) by construction; clamped so that no LDS or list index can leave its array
__device__ inline int centroid_of(const int* __restrict__ kb, int n, int K) { return min(max(kb[n], 0), K - 1); }

// grid = (chunks, B), block = 256; dynamic LDS: K ints.  hist[b][c][chunk] = windows of the chunk assigned to c
__global__ __launch_bounds__(256) void hist_kernel(int N, int K, int C, const int* __restrict__ mode, const int* __restrict__ ak,
                                                   int* __restrict__ hist)
{
    extern __shared__ int s_h[];
    const int ch = blockIdx.x, b = blockIdx.y, tid = threadIdx.x;
    if (mode[b] == HSCKMEANS_SKIP) return;
    for (int c = tid; c < K; c += 256) s_h[c] = 0;
    __syncthreads();
    const int* kb = ak + (size_t)b * N;
    const int n1 = min(N, (ch + 1) * kChunk);
    for (int n = ch * kChunk + tid; n < n1; n += 256) atomicAdd(&s_h[centroid_of(kb, n, K)], 1);
    __syncthreads();
    for (int c = tid; c < K; c += 256) hist[((size_t)b * K + c) * C + ch] = s_h[c];
}

// grid = B, block = 256: the exclusive scan of hist[b] in (centroid, chunk) order, in place: where in the index array
// the chunk's members of c begin.  Then offsets [K + 1], count and nonzero.
__global__ __launch_bounds__(256) void scan_kernel(int N, int K, int C, const int* __restrict__ mode, const int* __restrict__ ak,
                                                   int* __restrict__ hist, int* __restrict__ offsets, int* __restrict__ count,
                                                   int* __restrict__ nonzero)
{
    __shared__ int s_tot[256];
    const int b = blockIdx.x, tid = threadIdx.x;
    if (mode[b] == HSCKMEANS_SKIP) return;
    int* h = hist + (size_t)b * K * C;
    const int L = K * C, per = (L + 255) / 256, i0 = min(L, tid * per), i1 = min(L, i0 + per);
    int tot = 0;
    for (int i = i0; i < i1; ++i) tot += h[i];
    s_tot[tid] = tot;
    __syncthreads();
    int run = 0;
    for (int j = 0; j < tid; ++j) run += s_tot[j];
    for (int i = i0; i < i1; ++i) {
        const int v = h[i];
        h[i] = run;
        run += v;
    }
    __syncthreads();
    const int first = centroid_of(ak + (size_t)b * N, 0, K);
    for (int c = tid; c < K; c += 256) {
        const int lo = h[(size_t)c * C], hi = c + 1 < K ? h[(size_t)(c + 1) * C] : N;
        offsets[(size_t)b * (K + 1) + c] = lo;
        count[(size_t)b * K + c] = hi - lo;
        nonzero[(size_t)b * K + c] = hi - lo - (first == c ? 1 : 0) > 0 ? 1 : 0;
    }
    if (tid == 0) offsets[(size_t)b * (K + 1) + K] = N;
}

// grid = (chunks, B), block = 256; dynamic LDS: 4 * K ints.  Wave w of the chunk takes its windows [256 w, 256 w + 256)
// in segments of 64; its cursors start behind the chunk's earlier waves.  A window's place is its centroid's cursor plus
// its rank among the segment's lanes of the same centroid (ballot + popcount): ascending window order in every list.
// Writes the window index and, in list order, its patch offset and norm.
template <typename X>
__global__ __launch_bounds__(256) void place_kernel(int N, int K, int C, const int* __restrict__ mode, const int* __restrict__ ak,
                                                    const int* __restrict__ hist, const X* __restrict__ norm, const int* __restrict__ pofs,
                                                    int* __restrict__ index, int* __restrict__ lpofs, X* __restrict__ lnorm)
{
    extern __shared__ int s_cur[];                     // [4][K]
    const int ch = blockIdx.x, b = blockIdx.y, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    if (mode[b] == HSCKMEANS_SKIP) return;
    for (int i = tid; i < 4 * K; i += 256) s_cur[i] = 0;
    __syncthreads();
    const int* kb = ak + (size_t)b * N;
    const int w0 = ch * kChunk + wave * 256;
    int myk[4];
#pragma unroll
    for (int sg = 0; sg < 4; ++sg) {
        const int n = w0 + sg * 64 + lane;
        myk[sg] = n < N ? centroid_of(kb, n, K) : -1;
        if (n < N) atomicAdd(&s_cur[wave * K + myk[sg]], 1);
    }
    __syncthreads();
    for (int c = tid; c < K; c += 256) {               // counts of the waves -> where each wave's members of c begin
        int run = hist[((size_t)b * K + c) * C + ch];
#pragma unroll
        for (int w = 0; w < 4; ++w) {
            const int v = s_cur[w * K + c];
            s_cur[w * K + c] = run;
            run += v;
        }
    }
    __syncthreads();
    const size_t nb = (size_t)b * N;
#pragma unroll
    for (int sg = 0; sg < 4; ++sg) {
        const int n = w0 + sg * 64 + lane, k = myk[sg];
        unsigned long long rem = __ballot(k >= 0);
        int pos = -1;
        while (rem) {                                  // one round per centroid present in the segment
            const int src = __ffsll((long long)rem) - 1;
            const int kk = __shfl(k, src);
            const bool mine = k == kk;
            const unsigned long long mask = __ballot(mine);
            int base = 0;
            if (lane == src) base = atomicAdd(&s_cur[wave * K + kk], __popcll(mask));
            base = __shfl(base, src);
            if (mine) pos = base + __popcll(mask & ((1ull << lane) - 1ull));
            rem &= ~mask;
        }
        if (k >= 0 && pos >= 0 && pos < N) {
            index[nb + pos] = n;
            lpofs[nb + pos] = pofs[nb + n];
            lnorm[nb + pos] = norm[nb + n];
        }
    }
}

// grid = (ceil(Q / 256), K, B), block = kSumThreads: S[b][c][e0 .. e0 + tw) = the members' x[pofs + e] / norm added in list
// order from the first member's row.  The tile's rows lie in the ring at a pitch tp = tw rounded up to a power of two;
// a batch is RB = kRing * 256 / tp rows.  All 1024 threads load a batch (thread tid holds column tid % tp of the rows
// tid / tp + u * 1024 / tp, u < kLoads: coalesced along the elements), divide and store it to one half of the ring
// while lanes 0 .. tw - 1 add the other half: a member costs its adder lane one LDS read and one add, and the loads and
// divisions of a row are spread over four times as many lanes as add it.  The rows are loaded two batches ahead of the adds (two register sets, the loop
// unrolled by two), the patch offsets three.  Every load is issued unconditionally from a clamped (valid) row and
// column, so a batch's loads are all in flight together; only the store to the ring is predicated.
template <typename X>
__global__ __launch_bounds__(kSumThreads) void wide_sum_kernel(const X* __restrict__ x, int T, int F, int N, int Q, int K, const int* __restrict__ mode,
                                                       const int* __restrict__ offsets, const int* __restrict__ lpofs,
                                                       const X* __restrict__ lnorm, X* __restrict__ S)
{
    __shared__ X ring[2][kRing * 256];
    const int c = blockIdx.y, b = blockIdx.z, tid = threadIdx.x;
    if (mode[b] == HSCKMEANS_SKIP) return;
    const int e0 = blockIdx.x * 256, tw = min(256, Q - e0);
    const int o0 = offsets[(size_t)b * (K + 1) + c], m = offsets[(size_t)b * (K + 1) + c + 1] - o0;
    X* out = S + ((size_t)b * K + c) * Q + e0;
    if (m <= 0) {
        if (tid < tw) out[tid] = (X)0;
        return;
    }
    const int sh = tw > 1 ? 32 - __clz(tw - 1) : 0, tp = 1 << sh;         // tw <= tp <= 256
    const int RB = (kRing * 256) >> sh, nbatch = (m + RB - 1) / RB;
    const int r0 = tid >> sh, rstep = kSumThreads >> sh, col = tid & (tp - 1), colc = min(col, tw - 1);
    const int* lp = lpofs + (size_t)b * N + o0;
    const X* ln = lnorm + (size_t)b * N + o0;
    const X* xb = x + (size_t)b * T * F + e0 + colc;
    int po[kLoads];
    X va[kLoads], vb[kLoads], nr[kLoads];
    // the loads of batch jb (clamped to the last batch: valid rows, loaded again, never stored)
    auto rows_of = [&](int jb) { return min(RB, m - min(jb, nbatch - 1) * RB); };
    auto row_of = [&](int jb, int u) { return min(jb, nbatch - 1) * RB + min(r0 + u * rstep, rows_of(jb) - 1); };
    auto load_offsets = [&](int jb) {
#pragma unroll
        for (int u = 0; u < kLoads; ++u) po[u] = lp[row_of(jb, u)];
    };
    auto load_rows = [&](X (&v)[kLoads]) {
#pragma unroll
        for (int u = 0; u < kLoads; ++u) v[u] = xb[po[u]];
    };
    auto load_norms = [&](int jb) {
#pragma unroll
        for (int u = 0; u < kLoads; ++u) nr[u] = ln[row_of(jb, u)];
    };
    auto store_rows = [&](int jb, const X (&v)[kLoads]) {
        const int rows = rows_of(jb);
#pragma unroll
        for (int u = 0; u < kLoads; ++u)
            if (r0 + u * rstep < rows && col < tw) ring[jb & 1][tid + kSumThreads * u] = v[u] / nr[u];
    };
    load_offsets(0);                                   // batch 0 into ring[0]; batch 1 in flight, the offsets of batch 2
    load_rows(vb);
    load_norms(0);
    load_offsets(1);
    load_rows(va);
    load_offsets(2);
    store_rows(0, vb);
    __syncthreads();
    X acc = (X)0;
    // batch j is added from its half of the ring while batch j + 1 (`cur`, loaded an iteration ago) is divided and
    // stored to the other half and batch j + 2 (`nxt`) is loaded; the offsets run one batch further ahead
    auto body = [&](int j, const X (&cur)[kLoads], X (&nxt)[kLoads]) {
        const int rows = rows_of(j);
        load_rows(nxt);
        load_norms(j + 1);
        load_offsets(j + 3);
        if (tid < tw) {
            const X* r = ring[j & 1] + tid;
            int i = 0;
            if (j == 0) {
                acc = r[0];
                i = 1;
            }
            if (i + 8 <= rows) {                       // the next eight rows are read while these eight are added
                X t[8];
#pragma unroll
                for (int q = 0; q < 8; ++q) t[q] = r[(i + q) << sh];
                for (; i + 16 <= rows; i += 8) {
                    X nx[8];
#pragma unroll
                    for (int q = 0; q < 8; ++q) nx[q] = r[(i + 8 + q) << sh];
#pragma unroll
                    for (int q = 0; q < 8; ++q) acc = acc + t[q];
#pragma unroll
                    for (int q = 0; q < 8; ++q) t[q] = nx[q];
                }
#pragma unroll
                for (int q = 0; q < 8; ++q) acc = acc + t[q];
                i += 8;
            }
            for (; i < rows; ++i) acc = acc + r[i << sh];
        }
        if (j + 1 < nbatch) store_rows(j + 1, cur);
        __syncthreads();
    };
    for (int j = 0; j < nbatch; j += 2) {
        body(j, va, vb);
        if (j + 1 < nbatch) body(j + 1, vb, va);
    }
    if (tid < tw) out[tid] = acc;
}

}  // namespace

static_assert(HSCKMEANS_OK == hsc::OK && HSCKMEANS_ERR_INVALID == hsc::ERR_INVALID && HSCKMEANS_ERR_NO_DEVICE == hsc::ERR_NO_DEVICE &&
              HSCKMEANS_ERR_HIP == hsc::ERR_HIP && HSCKMEANS_ERR_UNSUPPORTED == hsc::ERR_UNSUPPORTED &&
              HSCKMEANS_ERR_ALLOC == hsc::ERR_ALLOC, "include/hsckmeans.h and common/hsc_lib.h disagree on a status");

struct HSC_HIDDEN hsckmeans_ctx : hsc::CtxBase {
    hipEvent_t ev[5] = {};
    // data (set_data)
    int dtype = -1, B = 0, T = 0, F = 0, N = 0, W = 0;    // a corpus: B = 1 learner, T = the rows of the stack
    int plan = HSCKMEANS_PLAN_AUTO;
    void* d_x = nullptr;
    int* d_starts = nullptr;
    // step buffers (grown, never shrunk); kMembers belongs to plan 1, kHist .. kLNorm to plan 2
    enum { kImg32, kImg64, kMode, kT, kK, kNorm, kPofs, kMembers, kCount, kNonzero, kSums, kHist, kOffsets, kIndex, kLPofs, kLNorm, kBufs };
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

static int upload(hsckmeans_ctx* ctx, const void* x, int dtype, int B, int T, int F, const std::vector<int>& s32, int N, int W, const char* fn);

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
    return upload(ctx, x, dtype, B, T, F, s32, N, W, "hsckmeans_set_data");
}

// the signal rules of a corpus: row_offsets ascend from 0 and every signal is longer than 2W; `fn` heads the messages
static int check_corpus_signals(hsckmeans_ctx* ctx, const char* fn, int B, const int64_t* row_offsets, int W)
{
    if (row_offsets[0] != 0) return fail(ctx, HSCKMEANS_ERR_INVALID, "%s: row_offsets[0] = %lld, must be 0", fn, (long long)row_offsets[0]);
    for (int b = 0; b < B; ++b) {
        const int64_t len = row_offsets[b + 1] - row_offsets[b];
        if (len < 0) return fail(ctx, HSCKMEANS_ERR_INVALID, "%s: row_offsets descend at signal %d (%lld after %lld)", fn, b,
                                 (long long)row_offsets[b + 1], (long long)row_offsets[b]);
        if (len <= 2 * W)
            return fail(ctx, HSCKMEANS_ERR_INVALID, "%s: signal %d has %lld samples, windows of 2W = %d samples need more than %d", fn, b,
                        (long long)len, 2 * W, 2 * W);
    }
    return HSCKMEANS_OK;
}

// the window rule of a corpus: every window lies inside one signal
static int check_corpus_windows(hsckmeans_ctx* ctx, const char* fn, int B, const int64_t* row_offsets, const int64_t* starts, int N, int W)
{
    const int64_t rows = row_offsets[B];
    for (int n = 0; n < N; ++n) {
        const int64_t st = starts[n];
        if (st < 0 || st >= rows) return fail(ctx, HSCKMEANS_ERR_INVALID, "%s: start %lld of window %d is outside the stack of %lld rows", fn, (long long)st, n, (long long)rows);
        const int b = (int)(std::upper_bound(row_offsets, row_offsets + B + 1, st) - row_offsets) - 1;     // row_offsets[b] <= st
        if (st + 2 * W > row_offsets[b + 1])
            return fail(ctx, HSCKMEANS_ERR_INVALID, "%s: window %d (rows %lld .. %lld) crosses the end of signal %d at row %lld", fn, n,
                        (long long)st, (long long)(st + 2 * W), b, (long long)row_offsets[b + 1]);
    }
    return HSCKMEANS_OK;
}

extern "C" int hsckmeans_set_corpus(hsckmeans_ctx* ctx, const void* x, int dtype, int B, const int64_t* row_offsets, int F,
                                    const int64_t* starts, int N, int W)
{
    const char* fn = "hsckmeans_set_corpus";
    if (!ctx) return fail(nullptr, HSCKMEANS_ERR_INVALID, "hsckmeans_set_corpus: ctx is NULL");
    if (!x || !row_offsets || !starts) return fail(ctx, HSCKMEANS_ERR_INVALID, "hsckmeans_set_corpus: x, row_offsets or starts is NULL");
    if (dtype != HSCKMEANS_F32 && dtype != HSCKMEANS_F64) return fail(ctx, HSCKMEANS_ERR_INVALID, "hsckmeans_set_corpus: bad dtype %d", dtype);
    if (B < 1 || F < 1 || N < 1 || W < 1)
        return fail(ctx, HSCKMEANS_ERR_INVALID, "hsckmeans_set_corpus: bad shape B = %d, F = %d, N = %d, W = %d", B, F, N, W);
    if (W > kMaxW) return fail(ctx, HSCKMEANS_ERR_UNSUPPORTED, "hsckmeans_set_corpus: W = %d exceeds the limit of %d", W, kMaxW);
    if (int rc = check_corpus_signals(ctx, fn, B, row_offsets, W)) return rc;
    const int64_t rows = row_offsets[B];
    if (rows > INT_MAX / F) return fail(ctx, HSCKMEANS_ERR_UNSUPPORTED, "hsckmeans_set_corpus: the stack of %lld x %d elements exceeds 2^31 - 1", (long long)rows, F);
    if (int rc = check_corpus_windows(ctx, fn, B, row_offsets, starts, N, W)) return rc;
    std::vector<int> s32((size_t)N);
    for (int n = 0; n < N; ++n) s32[n] = (int)starts[n];
    return upload(ctx, x, dtype, 1, (int)rows, F, s32, N, W, fn);
}

namespace {

// The covered part of a CSR corpus, as the host packs it for gather_kernel: the rows that some window covers, laid end
// to end in ascending row order (`crow` rows), with their entries.
//   rowptr [crow + 1]  entries of packed row i: rowptr[i] .. rowptr[i + 1] of cols / vals
//   wrow   [N]         the packed row of window n's first row; its 2W rows follow it (a window lies in one run of rows)
struct SparseArgs {
    const int* rowptr;
    const int* cols;
    const int* wrow;
    int N, L2, F, R, chunks;       // L2 = 2W rows per window, cut into `chunks` pieces of R rows: one piece per wave
};

// grid = ceil(N * chunks / 4), block = 256: wave u of the grid builds rows [c * R, c * R + R) of window n = u / chunks,
// c = u % chunks, in the window stack out [N * L2][F].  The piece is one contiguous span of the stack: the wave zeroes it
// with 16-byte stores (single elements up to the first and after the last aligned address), then writes the rows'
// entries at (row, column), one entry per lane and trip, the row found by bisection of the piece's row pointers.
// The zero of a cell and its entry may come from different lanes, in different store instructions of the SAME wave, and
// nothing but their order of issue puts the entry last: this rests on the hardware performing one wave's vector stores
// to one address in the order the wave issued them (so on gfx950; the wavefront-scope fence below emits no instruction,
// it only keeps the compiler from reordering).  No other wave writes the span.  Zeroing and entries split across waves,
// or a target that may reorder a wave's stores, would need a real barrier or a second kernel here.
template <typename X>
__global__ __launch_bounds__(256) void gather_kernel(const X* __restrict__ vals, X* __restrict__ out, SparseArgs a)
{
    typedef X vec_t __attribute__((ext_vector_type(16 / sizeof(X))));
    constexpr int V = 16 / sizeof(X);
    const int lane = threadIdx.x & 63;
    const long long u = (long long)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (u >= (long long)a.N * a.chunks) return;
    const int n = (int)(u / a.chunks), c = (int)(u - (long long)n * a.chunks);
    const int r0 = c * a.R, r1 = min(a.L2, r0 + a.R);
    const size_t lo = ((size_t)n * a.L2 + r0) * a.F, len = (size_t)(r1 - r0) * a.F;      // elements of the stack
    X* span = out + lo;
    const size_t head = min(len, (size_t)((V - lo % V) % V)), nvec = (len - head) / V, tail0 = head + nvec * V;
    if ((size_t)lane < head) span[lane] = (X)0;
    vec_t* vp = reinterpret_cast<vec_t*>(span + head);
    const vec_t zero = {};
    for (size_t i = lane; i < nvec; i += 64) vp[i] = zero;
    if (tail0 + lane < len) span[tail0 + lane] = (X)0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");         // the zeroes before the entries: same wave, stores in issue order
    const int* rp = a.rowptr + a.wrow[n] + r0;                    // rp[0 .. r1 - r0]: the piece's row pointers
    const int nr = r1 - r0, e1 = rp[nr];
    for (int e = rp[0] + lane; e < e1; e += 64) {
        int ra = 0, rb = nr - 1;                                   // the last row r with rp[r] <= e
        while (ra < rb) {
            const int m = (ra + rb + 1) >> 1;
            if (rp[m] <= e) ra = m;
            else rb = m - 1;
        }
        span[(size_t)ra * a.F + a.cols[e]] = vals[e];
    }
}

}  // namespace

extern "C" int hsckmeans_set_corpus_sparse(hsckmeans_ctx* ctx, int dtype, int B, const int64_t* row_offsets, int F,
                                           const int64_t* indptr, const int32_t* indices, const void* data,
                                           const int64_t* starts, int N, int W)
{
    const char* fn = "hsckmeans_set_corpus_sparse";
    if (!ctx) return fail(nullptr, HSCKMEANS_ERR_INVALID, "hsckmeans_set_corpus_sparse: ctx is NULL");
    if (!row_offsets || !indptr || !starts) return fail(ctx, HSCKMEANS_ERR_INVALID, "%s: row_offsets, indptr or starts is NULL", fn);
    if (dtype != HSCKMEANS_F32 && dtype != HSCKMEANS_F64) return fail(ctx, HSCKMEANS_ERR_INVALID, "%s: bad dtype %d", fn, dtype);
    if (B < 1 || F < 1 || N < 1 || W < 1) return fail(ctx, HSCKMEANS_ERR_INVALID, "%s: bad shape B = %d, F = %d, N = %d, W = %d", fn, B, F, N, W);
    if (W > kMaxW) return fail(ctx, HSCKMEANS_ERR_UNSUPPORTED, "%s: W = %d exceeds the limit of %d", fn, W, kMaxW);
    if (int rc = check_corpus_signals(ctx, fn, B, row_offsets, W)) return rc;
    const int64_t rows = row_offsets[B];
    const int L2 = 2 * W;
    if ((int64_t)N * L2 > INT_MAX / F)
        return fail(ctx, HSCKMEANS_ERR_UNSUPPORTED, "%s: the window stack of %lld x %d elements exceeds 2^31 - 1", fn, (long long)N * L2, F);
    if (int rc = check_corpus_windows(ctx, fn, B, row_offsets, starts, N, W)) return rc;
    // CSR validity, row by row (the whole corpus: the host learner cuts its patches from rows no window covers)
    if (indptr[0] != 0) return fail(ctx, HSCKMEANS_ERR_INVALID, "%s: indptr[0] = %lld, must be 0", fn, (long long)indptr[0]);
    for (int64_t r = 0; r < rows; ++r) {
        if (indptr[r + 1] < indptr[r])
            return fail(ctx, HSCKMEANS_ERR_INVALID, "%s: indptr descends at row %lld (%lld after %lld)", fn, (long long)r,
                        (long long)indptr[r + 1], (long long)indptr[r]);
        if (indptr[r + 1] > INT_MAX)
            return fail(ctx, HSCKMEANS_ERR_INVALID, "%s: indptr exceeds 2^31 - 1 entries at row %lld", fn, (long long)r);
    }
    if (rows > 0 && indptr[rows] > 0 && (!indices || !data)) return fail(ctx, HSCKMEANS_ERR_INVALID, "%s: indices or data is NULL", fn);
    for (int64_t r = 0; r < rows; ++r)
        for (int64_t e = indptr[r]; e < indptr[r + 1]; ++e) {
            if (indices[e] < 0 || indices[e] >= F)
                return fail(ctx, HSCKMEANS_ERR_INVALID, "%s: column %d of row %lld is outside [0, %d)", fn, (int)indices[e], (long long)r, F);
            if (e > indptr[r] && indices[e] <= indices[e - 1])
                return fail(ctx, HSCKMEANS_ERR_INVALID, "%s: the columns of row %lld do not ascend (%d after %d)", fn, (long long)r,
                            (int)indices[e], (int)indices[e - 1]);
        }

    // pack the covered rows: the windows in start order, their row intervals merged into runs
    std::vector<int> order((size_t)N);
    for (int n = 0; n < N; ++n) order[n] = n;
    std::sort(order.begin(), order.end(), [&](int p, int q) { return starts[p] < starts[q]; });
    std::vector<int> wrow((size_t)N), rowptr;
    std::vector<int64_t> run_lo, run_hi;           // the runs of covered rows [lo, hi), ascending and disjoint
    int64_t crow = 0;
    for (int i = 0; i < N; ++i) {
        const int64_t st = starts[order[i]];
        if (run_hi.empty() || st > run_hi.back()) {
            if (!run_hi.empty()) crow += run_hi.back() - run_lo.back();
            run_lo.push_back(st);
            run_hi.push_back(st + L2);
        } else {
            run_hi.back() = std::max(run_hi.back(), st + L2);
        }
        wrow[order[i]] = (int)(crow + (st - run_lo.back()));          // crow < N * L2 <= 2^31 - 1
    }
    crow += run_hi.back() - run_lo.back();
    int64_t cent = 0;
    for (size_t j = 0; j < run_lo.size(); ++j) cent += indptr[run_hi[j]] - indptr[run_lo[j]];
    const size_t xs = dtype == HSCKMEANS_F32 ? 4 : 8;
    rowptr.reserve((size_t)crow + 1);
    std::vector<int> cols((size_t)cent);
    std::vector<unsigned char> vals((size_t)cent * xs);
    int64_t pos = 0;
    for (size_t j = 0; j < run_lo.size(); ++j) {
        const int64_t e0 = indptr[run_lo[j]], ne = indptr[run_hi[j]] - e0;
        for (int64_t r = run_lo[j]; r < run_hi[j]; ++r) rowptr.push_back((int)(pos + indptr[r] - e0));
        if (ne > 0) {
            std::memcpy(cols.data() + pos, indices + e0, (size_t)ne * sizeof(int));
            std::memcpy(vals.data() + (size_t)pos * xs, (const char*)data + (size_t)e0 * xs, (size_t)ne * xs);
        }
        pos += ne;
    }
    rowptr.push_back((int)pos);
    std::vector<int> s32((size_t)N);
    for (int n = 0; n < N; ++n) s32[n] = n * L2;

    // the window stack: allocated, never uploaded; the context holds no data if anything below fails
    HSC_TRY(hipSetDevice(ctx->device));
    HSC_TRY(hipStreamSynchronize(ctx->stream));
    if (ctx->d_x) (void)hipFree(ctx->d_x);
    if (ctx->d_starts) (void)hipFree(ctx->d_starts);
    ctx->d_x = nullptr;
    ctx->d_starts = nullptr;
    ctx->dtype = -1;
    const size_t bytes[4] = {rowptr.size() * sizeof(int), std::max<size_t>(cols.size(), 1) * sizeof(int), std::max<size_t>(vals.size(), xs),
                             wrow.size() * sizeof(int)};
    const void* src[4] = {rowptr.data(), cols.data(), vals.data(), wrow.data()};
    const size_t copy[4] = {bytes[0], cols.size() * sizeof(int), vals.size(), bytes[3]};
    void* d[4] = {};
    hipError_t e = hipMalloc(&ctx->d_x, (size_t)N * L2 * F * xs);
    if (e == hipSuccess) e = hipMalloc((void**)&ctx->d_starts, s32.size() * sizeof(int));
    for (int i = 0; i < 4 && e == hipSuccess; ++i) e = hipMalloc(&d[i], bytes[i]);
    auto release = [&]() { for (void* q : d) if (q) (void)hipFree(q); };
    if (e != hipSuccess) {
        release();
        return fail(ctx, HSCKMEANS_ERR_ALLOC, "%s: hipMalloc failed (%s)", fn, hipGetErrorString(e));
    }
    e = hipMemcpyAsync(ctx->d_starts, s32.data(), s32.size() * sizeof(int), hipMemcpyHostToDevice, ctx->stream);
    for (int i = 0; i < 4 && e == hipSuccess; ++i)
        if (copy[i] > 0) e = hipMemcpyAsync(d[i], src[i], copy[i], hipMemcpyHostToDevice, ctx->stream);
    if (e == hipSuccess) {
        // rows per wave: as many pieces as a window has spans of 4 KiB (four 16-byte stores per lane), begun ones included,
        // then the rows shared evenly among them, so that no wave is launched for a tail of a few rows
        SparseArgs a;
        a.rowptr = (const int*)d[0]; a.cols = (const int*)d[1]; a.wrow = (const int*)d[3];
        a.N = N; a.L2 = L2; a.F = F;
        const int r4k = (int)std::min<size_t>((size_t)L2, std::max<size_t>(1, (4096 + F * xs - 1) / (F * xs)));
        const int pieces = (L2 + r4k - 1) / r4k;
        a.R = (L2 + pieces - 1) / pieces;
        a.chunks = (L2 + a.R - 1) / a.R;
        const unsigned grid = (unsigned)(((size_t)N * a.chunks + 3) / 4);      // N * chunks <= N * 2W <= 2^31 - 1
        if (dtype == HSCKMEANS_F32) hipLaunchKernelGGL((gather_kernel<float>), dim3(grid), dim3(256), 0, ctx->stream, (const float*)d[2], (float*)ctx->d_x, a);
        else hipLaunchKernelGGL((gather_kernel<double>), dim3(grid), dim3(256), 0, ctx->stream, (const double*)d[2], (double*)ctx->d_x, a);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    release();
    if (e != hipSuccess) return fail(ctx, HSCKMEANS_ERR_HIP, "%s: %s", fn, hipGetErrorString(e));
    ctx->dtype = dtype;
    ctx->B = 1; ctx->T = N * L2; ctx->F = F; ctx->N = N; ctx->W = W;
    return HSCKMEANS_OK;
}

extern "C" int hsckmeans_set_plan(hsckmeans_ctx* ctx, int plan)
{
    if (!ctx) return fail(nullptr, HSCKMEANS_ERR_INVALID, "hsckmeans_set_plan: ctx is NULL");
    if (plan != HSCKMEANS_PLAN_AUTO && plan != HSCKMEANS_PLAN_LISTS && plan != HSCKMEANS_PLAN_WIDE)
        return fail(ctx, HSCKMEANS_ERR_INVALID, "hsckmeans_set_plan: plan = %d is not 0 (auto), 1 (lists) or 2 (wide)", plan);
    ctx->plan = plan;
    return HSCKMEANS_OK;
}

// the checked data of set_data / set_corpus to the device; the context holds no data if this fails
static int upload(hsckmeans_ctx* ctx, const void* x, int dtype, int B, int T, int F, const std::vector<int>& s32, int N, int W, const char* fn)
{
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
    if (e != hipSuccess) return fail(ctx, HSCKMEANS_ERR_ALLOC, "%s: hipMalloc failed (%s)", fn, hipGetErrorString(e));
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
static int launch_centroids(hsckmeans_ctx* ctx, int K, int plan)
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
    if (plan == HSCKMEANS_PLAN_WIDE) {
        const int C = (N + kChunk - 1) / kChunk;
        int* hist = (int*)ctx->buf[hsckmeans_ctx::kHist];
        int* offsets = (int*)ctx->buf[hsckmeans_ctx::kOffsets];
        int* index = (int*)ctx->buf[hsckmeans_ctx::kIndex];
        int* lpofs = (int*)ctx->buf[hsckmeans_ctx::kLPofs];
        X* lnorm = (X*)ctx->buf[hsckmeans_ctx::kLNorm];
        hipLaunchKernelGGL(hist_kernel, dim3(C, B), dim3(256), (size_t)K * sizeof(int), ctx->stream, N, K, C, mode, ak, hist);
        HSC_TRY(hipGetLastError());
        hipLaunchKernelGGL(scan_kernel, dim3(B), dim3(256), 0, ctx->stream, N, K, C, mode, ak, hist, offsets, count, nonzero);
        HSC_TRY(hipGetLastError());
        hipLaunchKernelGGL((place_kernel<X>), dim3(C, B), dim3(256), (size_t)4 * K * sizeof(int), ctx->stream, N, K, C, mode, ak,
                           (const int*)hist, (const X*)norm, (const int*)pofs, index, lpofs, lnorm);
        HSC_TRY(hipGetLastError());
        hipLaunchKernelGGL((wide_sum_kernel<X>), dim3((Q + 255) / 256, K, B), dim3(kSumThreads), 0, ctx->stream, (const X*)ctx->d_x, ctx->T, ctx->F,
                           N, Q, K, mode, (const int*)offsets, (const int*)lpofs, (const X*)lnorm, (X*)ctx->buf[hsckmeans_ctx::kSums]);
        HSC_TRY(hipGetLastError());
        return HSCKMEANS_OK;
    }
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
    // plan 1's [K][N] table is indexed in int; auto leaves it there, and from HSCKMEANS_WIDE_FROM_WINDOWS windows on
    const bool lists_fit = (int64_t)K * N <= INT_MAX / 2;
    int plan = ctx->plan;
    if (plan == HSCKMEANS_PLAN_AUTO)
        plan = K <= kWideMaxK && (N >= HSCKMEANS_WIDE_FROM_WINDOWS || !lists_fit) ? HSCKMEANS_PLAN_WIDE : HSCKMEANS_PLAN_LISTS;
    if ((int64_t)K * Q > INT_MAX / 2 || (plan == HSCKMEANS_PLAN_LISTS && !lists_fit))
        return fail(ctx, HSCKMEANS_ERR_UNSUPPORTED, "hsckmeans_step: K = %d is too large for this shape", K);
    if (plan == HSCKMEANS_PLAN_WIDE && K > kWideMaxK)
        return fail(ctx, HSCKMEANS_ERR_UNSUPPORTED, "hsckmeans_step: the wide plan takes K <= %d (K = %d)", kWideMaxK, K);
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
    const size_t xs = ctx->dtype == HSCKMEANS_F32 ? 4 : 8, chunks = ((size_t)N + kChunk - 1) / kChunk;
    const bool wide = plan == HSCKMEANS_PLAN_WIDE;
    const size_t bytes[hsckmeans_ctx::kBufs] = {
        any32 ? per * B * 4 : 0, any64 ? per * B * 8 : 0, (size_t)B * sizeof(int), (size_t)B * N * sizeof(int),
        (size_t)B * N * sizeof(int), (size_t)B * N * xs, (size_t)B * N * sizeof(int), wide ? 0 : (size_t)B * K * N * sizeof(int),
        (size_t)B * K * sizeof(int), (size_t)B * K * sizeof(int), (size_t)B * K * Q * xs,
        wide ? (size_t)B * K * chunks * sizeof(int) : 0, wide ? (size_t)B * (K + 1) * sizeof(int) : 0, wide ? (size_t)B * N * sizeof(int) : 0,
        wide ? (size_t)B * N * sizeof(int) : 0, wide ? (size_t)B * N * xs : 0};
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
    rc = ctx->dtype == HSCKMEANS_F32 ? launch_centroids<float>(ctx, K, plan) : launch_centroids<double>(ctx, K, plan);
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
