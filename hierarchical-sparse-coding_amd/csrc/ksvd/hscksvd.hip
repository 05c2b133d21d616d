// hscksvd.hip -- libhscksvd.so: the dictionary update of the convolutional K-SVD learner (hsc/modeling.py:591-633)
// on gfx950, C ABI in include/hscksvd.h.  DESIGN.md section 13.
//
// A call works on P >= 1 problems of one (K, W, F), and one host driver (run_update) checks, lays out, uploads, launches and
// downloads them.  Problem p has its own dictionary, column pointers, occurrence pointers and stats at stride p, its own
// entries (rows, values, occurrence ids and spans, the ids relative to its first entry) from entry_off[p] on and its own
// patch scratch from patch_off[p] on.  Its coefficient matrix is the vertical stack of its signals' [T_b][K] matrices;
// every occurrence carries the stacked rows [lo, hi) of its own signal, and nothing of another signal enters its patch.
//   hscksvd_update:         P = 1, one signal [0, T)
//   hscksvd_update_corpus:  P = 1, B signals from row_offsets
//   hscksvd_update_batch:   P = B, one signal [0, T) each
// The atoms of a problem depend on each other in order (atom k reads the new atoms and coefficients of every k' < k).
// Two plans run the same device functions, so they return the same bits:
//   plan 1: ONE launch of ksvd_sweep_kernel, workgroup p of 1024 threads on problem p; the atoms run one after the other
//           inside the kernel, separated by workgroup barriers, and never wait for the host.  Nothing is shared between
//           two workgroups.
//   plan 2 (P = 1): per atom, in stream order, ksvd_gather_kernel and ksvd_gram_kernel on grids over the occurrences /
//           the Gram entries (and ksvd_centre_kernel for the PCA branch), then ksvd_tail_kernel on one workgroup.  No
//           kernel waits for another workgroup: the order of the atoms is the order of the launches.
// Per atom k with m occurrences:
//   1. gather: one wave per patch (plan 1: wave w builds the patches i = w, w + 16, ...).  Lane l < W*F owns sample
//      (s, f) = (l / F, l % F) at stacked row tau = g_i - (W-1)/2 + s, live when lo <= tau < hi.  For every other
//      column j the lanes binary-search column j's rows for the entries of [max(g_i - (W-1), lo), min(g_i + W, hi))
//      (lane j % 64 searches column j), then the wave walks those entries in CSC order (column ascending, row
//      ascending) and adds c * D[j][tau - g_e + (W-1)/2][f] for the taps that hit: the host overlap-add's sum, term
//      by term.  The patches go to a global scratch [m][W*F].
//   2. (PCA branch, m >= 2) centre the patches per component.
//   3. Gram matrix G = sum_i P_i P_i^T (one thread per entry, i ascending) into LDS (plan 2: through global memory).
//   4. cyclic Jacobi with the round-robin parallel ordering: per round n/2 disjoint rotations, G <- J^T G J and
//      V <- V J (V transposed in LDS), until a sweep rotates nothing.
//   5. thread 0 picks the top eigenvector, applies the zero / tie / sign rules of include/hscksvd.h, the workgroup
//      writes D[k] and the new coefficients c_i = P_i . u.
// Compiled with -ffp-contract=off: no product is fused into a sum, which step 1 relies on.
#include "../../../include/hscksvd.h"
#include "../common/hsc_lib.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int kThreads = 1024;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxN = HSCKSVD_MAX_ATOM_SIZE;
constexpr int kMaxSweeps = 40;
constexpr int kStats = HSCKSVD_ATOM_STATS;

struct SweepArgs {
    int K, W, F, use_pca;
    double* D;                 // [K][W*F], updated in place
    const int* indptr;         // [K+1]
    const int* rows;           // [nnz]
    double* vals;              // [nnz], updated in place
    const int* occ;            // entry ids of every atom's occurrences, atom after atom
    const int* occ_ptr;        // [K+1]
    const int2* occ_span;      // per occurrence: the stacked rows [lo, hi) of its signal
    double* P;                 // scratch [max m][W*F]
    double* G;                 // plan 2: the Gram matrix [n2][n2] on its way to the tail kernel
    double* stats;             // [K][kStats]
};

// first position in rows[b, e) whose value is >= v (rows ascending)
__device__ __forceinline__ int lower_bound(const int* rows, int b, int e, int v)
{
    while (b < e) {
        const int mid = b + ((e - b) >> 1);
        if (rows[mid] < v) b = mid + 1;
        else e = mid;
    }
    return b;
}

// round-robin (circle) ordering of n2 (even) indices: pair i of round r
__device__ __forceinline__ void rr_pair(int n2, int r, int i, int& p, int& q)
{
    const int L = n2 - 1;
    int a, b;
    if (i == 0) {
        a = L;
        b = r;
    } else {
        a = (r + i) % L;
        b = (r - i + L) % L;
    }
    p = min(a, b);
    q = max(a, b);
}

// what the Jacobi tail keeps in LDS (66 KB at W*F = 64)
struct TailLds {
    double G[kMaxN][kMaxN + 1];     // +1: the column step walks a column
    double Vt[kMaxN][kMaxN];        // Vt[j] = eigenvector estimate j
    double u[kMaxN];
    double rot_c[kMaxN / 2], rot_s[kMaxN / 2];
    int rot_p[kMaxN / 2], rot_q[kMaxN / 2];
    int rotated;
};

// ---- 1. patch i of atom k (one wave)
__device__ __forceinline__ void gather_patch(const SweepArgs& a, int k, int o0, int i, int lane)
{
    const int K = a.K, W = a.W, F = a.F, n = W * F, lead = (W - 1) / 2;
    const int g = a.rows[a.occ[o0 + i]];
    const int2 span = a.occ_span[o0 + i];
    const int s = lane / F, f = lane - s * F;
    const long long tau = (long long)g - lead + s;
    const bool live = lane < n && tau >= span.x && tau < span.y;
    double acc = 0.0;
    for (int cb = 0; cb < K; cb += 64) {
        const int j = cb + lane;
        int lo = 0, hi = 0;
        if (j < K && j != k) {
            const int b = a.indptr[j], e = a.indptr[j + 1];
            lo = lower_bound(a.rows, b, e, max(g - (W - 1), span.x));
            hi = lower_bound(a.rows, lo, e, min(g, span.y - W) + W);
        }
        const int nc = min(64, K - cb);
        for (int jj = 0; jj < nc; ++jj) {
            const int l0 = __shfl(lo, jj), h0 = __shfl(hi, jj);
            const double* Dj = a.D + (size_t)(cb + jj) * n;
            for (int e = l0; e < h0; ++e) {
                const double c = a.vals[e];
                if (c == 0.0) continue;                       // reconstructSignal skips c == 0
                const int tap = g - a.rows[e] + s;            // tau - (g_e - lead)
                if (live && tap >= 0 && tap < W) {
                    const double term = c * Dj[tap * F + f];
                    acc = acc + term;
                }
            }
        }
    }
    if (lane < n) a.P[(size_t)i * n + lane] = live ? acc : 0.0;
}

// ---- 2. centring (the reference's pca: data -= data.mean(axis=0)); one workgroup, `mean` [n] in LDS
__device__ __forceinline__ void centre_patches(double* P, int m, int n, double* mean, int tid, int threads)
{
    if (tid < n) {
        double sum = 0.0;
        for (int i = 0; i < m; ++i) sum = sum + P[(size_t)i * n + tid];
        mean[tid] = sum / (double)m;
    }
    __syncthreads();
    for (int i = tid >> 6; i < m; i += threads >> 6)                     // a wave per patch
        if ((tid & 63) < n) P[(size_t)i * n + (tid & 63)] = P[(size_t)i * n + (tid & 63)] - mean[tid & 63];
    __syncthreads();
}

// ---- 3. entry x of the Gram matrix [n2][n2] (rows and columns >= n: the padding of an odd n)
__device__ __forceinline__ double gram_entry(const double* P, int m, int n, int n2, int x)
{
    const int r = x / n2, c = x - r * n2;
    double g = 0.0;
    if (r < n && c < n)
        for (int i = 0; i < m; ++i) g = g + P[(size_t)i * n + r] * P[(size_t)i * n + c];
    return g;
}

// ---- 3. - 5. of atom k on one workgroup of kThreads: the Gram matrix (kGramGiven: read from a.G), Jacobi, the rules,
// D[k] and the new coefficients.  The patches (centred where the branch asks for it) are in a.P.
template <bool kGramGiven>
__device__ __forceinline__ void atom_tail(const SweepArgs& a, int k, int o0, int m, TailLds& lds, int tid)
{
    auto& G = lds.G;
    auto& Vt = lds.Vt;
    auto& u = lds.u;
    auto& rot_c = lds.rot_c;
    auto& rot_s = lds.rot_s;
    auto& rot_p = lds.rot_p;
    auto& rot_q = lds.rot_q;
    int& rotated = lds.rotated;
    const int n = a.W * a.F;
    const int n2 = n + (n & 1);
    const int half = n2 / 2;
    const bool pca = a.use_pca != 0;
    double* st = a.stats + (size_t)k * kStats;

    double lambda1 = 0.0, lambda2 = 0.0;
    int sweeps = 0;
    if (m == 1) {
        // ---- rank one: u = P / |P|
        if (tid == 0) {
            double ss = 0.0;
            for (int x = 0; x < n; ++x) ss = ss + a.P[x] * a.P[x];
            const double nrm = sqrt(ss);
            lambda1 = ss;
            if (nrm > 0.0) {
                for (int x = 0; x < n; ++x) u[x] = a.P[x] / nrm;
            } else {
                for (int x = 0; x < n; ++x) u[x] = (!pca && x == 0) ? 1.0 : 0.0;   // e_0 / normalize's 0
            }
            rotated = (nrm > 0.0 && !pca) ? 1 : 0;                          // orient by the sign rule?
        }
    } else {
        // ---- 3. Gram matrix, V = I
        for (int x = tid; x < n2 * n2; x += kThreads) {
            const int r = x / n2, c = x - r * n2;
            G[r][c] = kGramGiven ? a.G[x] : gram_entry(a.P, m, n, n2, x);
            Vt[r][c] = r == c ? 1.0 : 0.0;
        }
        __syncthreads();

        // ---- 4. Jacobi
        for (sweeps = 0; sweeps < kMaxSweeps;) {
            if (tid == 0) rotated = 0;
            __syncthreads();
            for (int r = 0; r < n2 - 1; ++r) {
                if (tid < half) {
                    int p, q;
                    rr_pair(n2, r, tid, p, q);
                    const double app = G[p][p], aqq = G[q][q], apq = G[p][q];
                    double c = 1.0, s = 0.0;
                    if (apq != 0.0 && fabs(apq) > 2.220446049250313e-16 * sqrt(fabs(app) * fabs(aqq))) {
                        const double theta = (aqq - app) / (2.0 * apq);
                        const double t = fabs(theta) > 1e150 ? 0.5 / theta
                                                             : copysign(1.0, theta) / (fabs(theta) + sqrt(theta * theta + 1.0));
                        c = 1.0 / sqrt(t * t + 1.0);
                        s = t * c;
                        rotated = 1;
                    }
                    rot_p[tid] = p;
                    rot_q[tid] = q;
                    rot_c[tid] = c;
                    rot_s[tid] = s;
                }
                __syncthreads();
                // G <- G J, V <- V J
                for (int x = tid; x < half * n2; x += kThreads) {
                    const int pi = x / n2, row = x - pi * n2;
                    const double s = rot_s[pi];
                    if (s == 0.0) continue;
                    const int p = rot_p[pi], q = rot_q[pi];
                    const double c = rot_c[pi];
                    const double gp = G[row][p], gq = G[row][q];
                    G[row][p] = c * gp - s * gq;
                    G[row][q] = s * gp + c * gq;
                    const double vp = Vt[p][row], vq = Vt[q][row];
                    Vt[p][row] = c * vp - s * vq;
                    Vt[q][row] = s * vp + c * vq;
                }
                __syncthreads();
                // G <- J^T G, the annihilated pair set to 0
                for (int x = tid; x < half * n2; x += kThreads) {
                    const int pi = x / n2, col = x - pi * n2;
                    const double s = rot_s[pi];
                    if (s == 0.0) continue;
                    const int p = rot_p[pi], q = rot_q[pi];
                    const double c = rot_c[pi];
                    const double gp = G[p][col], gq = G[q][col];
                    G[p][col] = col == q ? 0.0 : c * gp - s * gq;
                    G[q][col] = col == p ? 0.0 : s * gp + c * gq;
                }
                __syncthreads();
            }
            ++sweeps;
            const int any = rotated;
            __syncthreads();
            if (!any) break;
        }

        // ---- 5. the top eigenvector
        if (tid == 0) {
            int top = pca ? n - 1 : 0;
            lambda1 = G[top][top];
            for (int x = 0; x < n; ++x) {
                const double l = G[x][x];
                if (pca ? l >= lambda1 : l > lambda1) {
                    lambda1 = l;
                    top = x;
                }
            }
            lambda2 = -INFINITY;
            for (int x = 0; x < n; ++x)
                if (x != top && G[x][x] > lambda2) lambda2 = G[x][x];
            if (n == 1) lambda2 = 0.0;
            if (lambda1 > 0.0) {
                for (int x = 0; x < n; ++x) u[x] = Vt[top][x];
                rotated = 1;
            } else {                                                        // zero Gram / covariance
                for (int x = 0; x < n; ++x) u[x] = x == (pca ? n - 1 : 0) ? 1.0 : 0.0;
                rotated = 0;
            }
            if (pca) {
                lambda1 = lambda1 / (double)(m - 1);
                lambda2 = lambda2 / (double)(m - 1);
            }
        }
    }
    // sign rule (thread 0; `rotated` says whether u's sign is free)
    if (tid == 0) {
        if (rotated) {
            const double* d = a.D + (size_t)k * n;
            double dot = 0.0;
            for (int x = 0; x < n; ++x) dot = dot + u[x] * d[x];
            bool flip = dot < 0.0;
            if (dot == 0.0) {
                for (int x = 0; x < n; ++x)
                    if (u[x] != 0.0) {
                        flip = u[x] < 0.0;
                        break;
                    }
            }
            if (flip)
                for (int x = 0; x < n; ++x) u[x] = -u[x];
        }
        st[HSCKSVD_STAT_OCCURRENCES] = (double)m;
        st[HSCKSVD_STAT_LAMBDA1] = lambda1;
        st[HSCKSVD_STAT_LAMBDA2] = lambda2;
        st[HSCKSVD_STAT_SWEEPS] = (double)sweeps;
    }
    __syncthreads();

    // ---- the new atom and its coefficients
    if (tid < n) a.D[(size_t)k * n + tid] = u[tid];
    for (int i = tid; i < m; i += kThreads) {
        const double* p = a.P + (size_t)i * n;
        double c = 0.0;
        for (int x = 0; x < n; ++x) c = c + p[x] * u[x];
        a.vals[a.occ[o0 + i]] = c;
    }
    __syncthreads();
}

// ---- plan 1: all atoms of one problem, one after the other, on the calling workgroup
__device__ __forceinline__ void sweep_atoms(const SweepArgs& a, TailLds& lds)
{
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int n = a.W * a.F;
    for (int k = 0; k < a.K; ++k) {
        const int o0 = a.occ_ptr[k], m = a.occ_ptr[k + 1] - o0;
        if (m == 0) {
            if (tid < kStats) a.stats[(size_t)k * kStats + tid] = 0.0;
            continue;
        }
        for (int i = wave; i < m; i += kWaves) gather_patch(a, k, o0, i, lane);
        __syncthreads();
        if (a.use_pca && m >= 2) centre_patches(a.P, m, n, lds.u, tid, kThreads);
        atom_tail<false>(a, k, o0, m, lds, tid);
    }
}

// Workgroup p runs plan 1 on problem p.  `a` describes problem 0; problem p's dictionary, column pointers, occurrence pointers
// and stats lie p strides behind, its entries (rows, values, occurrence ids and spans: all relative to its first entry)
// entry_off[p] behind, its patches patch_off[p] patches behind.  Nothing is shared between two workgroups.
__global__ __launch_bounds__(kThreads) void ksvd_sweep_kernel(SweepArgs a, const long long* __restrict__ entry_off,
                                                              const long long* __restrict__ patch_off)
{
    __shared__ TailLds lds;
    const int p = blockIdx.x, n = a.W * a.F;
    const long long e0 = entry_off[p];
    a.D += (size_t)p * a.K * n;
    a.indptr += (size_t)p * (a.K + 1);
    a.occ_ptr += (size_t)p * (a.K + 1);
    a.stats += (size_t)p * a.K * kStats;
    a.rows += e0;
    a.vals += e0;
    a.occ += e0;
    a.occ_span += e0;
    a.P += (size_t)patch_off[p] * n;
    sweep_atoms(a, lds);
}

// ---- plan 2: the phases of ONE atom as kernels of their own (the stats of an atom without occurrences are zeroed by the host)
constexpr int kGridThreads = 256;

__global__ __launch_bounds__(kGridThreads) void ksvd_gather_kernel(SweepArgs a, int k)
{
    const int o0 = a.occ_ptr[k], m = a.occ_ptr[k + 1] - o0;
    const int i = blockIdx.x * (kGridThreads / 64) + (threadIdx.x >> 6);
    if (i < m) gather_patch(a, k, o0, i, threadIdx.x & 63);
}

__global__ __launch_bounds__(kThreads) void ksvd_centre_kernel(SweepArgs a, int k)
{
    __shared__ double mean[kMaxN];
    centre_patches(a.P, a.occ_ptr[k + 1] - a.occ_ptr[k], a.W * a.F, mean, threadIdx.x, kThreads);
}

__global__ __launch_bounds__(kGridThreads) void ksvd_gram_kernel(SweepArgs a, int k)
{
    const int n = a.W * a.F, n2 = n + (n & 1);
    const int x = blockIdx.x * kGridThreads + threadIdx.x;
    if (x < n2 * n2) a.G[x] = gram_entry(a.P, a.occ_ptr[k + 1] - a.occ_ptr[k], n, n2, x);
}

__global__ __launch_bounds__(kThreads) void ksvd_tail_kernel(SweepArgs a, int k)
{
    __shared__ TailLds lds;
    const int o0 = a.occ_ptr[k];
    atom_tail<true>(a, k, o0, a.occ_ptr[k + 1] - o0, lds, threadIdx.x);
}

}  // namespace

static_assert(HSCKSVD_OK == hsc::OK && HSCKSVD_ERR_INVALID == hsc::ERR_INVALID && HSCKSVD_ERR_NO_DEVICE == hsc::ERR_NO_DEVICE &&
              HSCKSVD_ERR_HIP == hsc::ERR_HIP && HSCKSVD_ERR_UNSUPPORTED == hsc::ERR_UNSUPPORTED && HSCKSVD_ERR_ALLOC == hsc::ERR_ALLOC,
              "include/hscksvd.h and common/hsc_lib.h disagree on a status");

struct HSC_HIDDEN hscksvd_ctx : hsc::CtxBase {
    hipEvent_t ev[4] = {};
    hsc::Buffers<10> buf;              // D, indptr, rows, vals, occ, occ_ptr + stats, P, occ_span, G, entry_off + patch_off
};

using hsc::fail;

extern "C" int hscksvd_version(void) { return 1; }

extern "C" const char* hscksvd_last_error(hscksvd_ctx* ctx) { return hsc::last_error(ctx); }

extern "C" int hscksvd_create(hscksvd_ctx** out, int device_id) { return hsc::create(out, device_id, "hscksvd_create"); }

extern "C" void hscksvd_destroy(hscksvd_ctx* ctx) { hsc::destroy(ctx); }

namespace {

enum { kPlanAuto = 0, kPlanOne = 1, kPlanWide = 2 };

// The sweep behind the three entry points (`fn` heads the messages) over P problems of one (K, W, F).  Problem p has its own
// dictionary, indptr [K+1] and stats [K][kStats] at stride p, and its entries (indices, data) from entry_offsets[p] on.  `batch`
// (hscksvd_update_batch): entry_offsets [P+1] is the caller's argument, checked here, and the messages name the problem;
// otherwise P = 1 and the entries are [0, indptr[K]).  The rows of every problem are the stack of S signals, signal s the rows
// [row_offsets[s], row_offsets[s + 1]).  Plans 0 and 2 take P = 1 only.
int run_update(hscksvd_ctx* ctx, const char* fn, bool batch, int P, const int64_t* entry_offsets, int S, const int32_t* row_offsets,
               int K, int W, int F, double* D, const int32_t* indptr, const int32_t* indices, double* data, int use_pca, int plan,
               double* out_atom_stats, double* timing_ms)
{
    if (W * F > kMaxN) return fail(ctx, HSCKSVD_ERR_UNSUPPORTED, "%s: W * F = %d exceeds the limit of %d", fn, W * F, kMaxN);
    if (use_pca && F != 1) return fail(ctx, HSCKSVD_ERR_UNSUPPORTED, "%s: the PCA branch needs F = 1 (got F = %d)", fn, F);
    const bool no_entries = !indices || !data;
    if (batch) {
        if (!D || !indptr || !entry_offsets) return fail(ctx, HSCKSVD_ERR_INVALID, "%s: D, indptr or entry_offsets is NULL", fn);
        if (entry_offsets[0] != 0) return fail(ctx, HSCKSVD_ERR_INVALID, "%s: entry_offsets[0] = %lld, expected 0", fn, (long long)entry_offsets[0]);
        for (int p = 0; p < P; ++p)
            if (entry_offsets[p + 1] < entry_offsets[p]) return fail(ctx, HSCKSVD_ERR_INVALID, "%s: entry_offsets decreases at problem %d", fn, p);
        if (entry_offsets[P] >= (1ll << 31))
            return fail(ctx, HSCKSVD_ERR_UNSUPPORTED, "%s: %lld stored entries in all, the limit is 2^31 - 1", fn, (long long)entry_offsets[P]);
        if (entry_offsets[P] > 0 && no_entries) return fail(ctx, HSCKSVD_ERR_INVALID, "%s: indices or data is NULL", fn);
    } else if (!D || !indptr) {
        return fail(ctx, HSCKSVD_ERR_INVALID, "%s: D or indptr is NULL", fn);
    }
    const int n = W * F, n2 = n + (n & 1), T = row_offsets[S];
    char name[32] = "";
    auto who = [&](int p) {                                             // "problem p: " in the batch's messages
        if (batch) snprintf(name, sizeof(name), "problem %d: ", p);
        return name;
    };

    // Per problem the checks of its columns and rows and, in the same walk, its occurrences: column k's entries whose value is
    // not 0.0 (they keep their values until atom k's turn), each with the rows of its signal.  They lie at the problem's own
    // place in the entry arrays, their ids relative to its first entry; its patches get the room of its most frequent atom.
    std::vector<int> occ_ptr((size_t)P * (K + 1), 0), occ;
    std::vector<int2> occ_span;
    std::vector<long long> off(2 * (size_t)P);                          // entry_off [P], then patch_off [P]
    long long nnz = 0, patches = 0, occurrences = 0;
    int widest = 0;
    for (int p = 0; p < P; ++p) {
        const int32_t* ip = indptr + (size_t)p * (K + 1);
        if (ip[0] != 0) return fail(ctx, HSCKSVD_ERR_INVALID, "%s: %sindptr[0] = %d, expected 0", fn, who(p), ip[0]);
        for (int k = 0; k < K; ++k)
            if (ip[k + 1] < ip[k]) return fail(ctx, HSCKSVD_ERR_INVALID, "%s: %sindptr decreases at column %d", fn, who(p), k);
        const long long e0 = batch ? entry_offsets[p] : 0, count = batch ? entry_offsets[p + 1] - e0 : ip[K];
        if (ip[K] != count)
            return fail(ctx, HSCKSVD_ERR_INVALID, "%s: %sindptr[K] = %d, but entry_offsets gives it %lld entries", fn, who(p), ip[K], count);
        if (count > 0 && no_entries) return fail(ctx, HSCKSVD_ERR_INVALID, "%s: indices or data is NULL", fn);
        const int32_t* idx = indices + e0;
        const double* val = data + e0;
        int* op = occ_ptr.data() + (size_t)p * (K + 1);
        int max_m = 0;
        occ.resize((size_t)e0, 0);
        occ_span.resize((size_t)e0, make_int2(0, 0));
        for (int k = 0; k < K; ++k) {
            for (int e = ip[k]; e < ip[k + 1]; ++e) {
                if (idx[e] < 0 || idx[e] >= T)
                    return fail(ctx, HSCKSVD_ERR_INVALID, "%s: %srow %d of entry %d is outside [0, %d)", fn, who(p), idx[e], e, T);
                if (e > ip[k] && idx[e] <= idx[e - 1])
                    return fail(ctx, HSCKSVD_ERR_INVALID, "%s: %sthe rows of column %d are not strictly ascending", fn, who(p), k);
                if (val[e] != 0.0) {
                    const int32_t* hi = std::upper_bound(row_offsets, row_offsets + S + 1, idx[e]);
                    occ.push_back(e);
                    occ_span.push_back(make_int2(hi[-1], hi[0]));
                }
            }
            op[k + 1] = (int)(occ.size() - (size_t)e0);
            max_m = std::max(max_m, op[k + 1] - op[k]);
        }
        off[p] = e0;
        off[(size_t)P + p] = patches;
        patches += max_m;
        occurrences += op[K];
        widest = std::max(widest, max_m);
        nnz = e0 + count;
    }
    occ.resize((size_t)nnz, 0);
    occ_span.resize((size_t)nnz, make_int2(0, 0));
    std::vector<double> stats((size_t)P * K * kStats, 0.0);
    if (timing_ms) timing_ms[0] = timing_ms[1] = timing_ms[2] = 0.0;
    if (occurrences == 0) {
        if (out_atom_stats) std::memcpy(out_atom_stats, stats.data(), stats.size() * sizeof(double));
        return HSCKSVD_OK;                                              // no atom of any problem occurs: nothing changes
    }
    if (plan == kPlanAuto) plan = widest >= HSCKSVD_WIDE_FROM_OCCURRENCES ? kPlanWide : kPlanOne;

    HSC_TRY(hipSetDevice(ctx->device));
    const size_t bD = (size_t)P * K * n * sizeof(double), bI = (size_t)P * (K + 1) * sizeof(int), bR = (size_t)nnz * sizeof(int),
                 bV = (size_t)nnz * sizeof(double), bS = (size_t)P * K * kStats * sizeof(double),
                 bP = (size_t)patches * n * sizeof(double), bB = (size_t)nnz * sizeof(int2), bG = (size_t)n2 * n2 * sizeof(double),
                 bF = off.size() * sizeof(long long);
    const size_t bytes[10] = {bD, bI, bR, bV, bR, bI + bS + 16, bP, bB, bG, bF};
    if (int rc = ctx->buf.ensure(ctx, bytes, fn)) return rc;
    SweepArgs args;
    args.K = K;
    args.W = W;
    args.F = F;
    args.use_pca = use_pca ? 1 : 0;
    args.D = (double*)ctx->buf[0];
    args.indptr = (const int*)ctx->buf[1];
    args.rows = (const int*)ctx->buf[2];
    args.vals = (double*)ctx->buf[3];
    args.occ = (const int*)ctx->buf[4];
    args.occ_ptr = (const int*)ctx->buf[5];
    args.stats = (double*)((char*)ctx->buf[5] + (bI + 15) / 16 * 16);
    args.P = (double*)ctx->buf[6];
    args.occ_span = (const int2*)ctx->buf[7];
    args.G = (double*)ctx->buf[8];
    const long long* d_off = (const long long*)ctx->buf[9];
    hipStream_t st = ctx->stream;
    HSC_TRY(hipEventRecord(ctx->ev[0], st));
    HSC_TRY(hipMemcpyAsync(ctx->buf[0], D, bD, hipMemcpyHostToDevice, st));
    HSC_TRY(hipMemcpyAsync(ctx->buf[1], indptr, bI, hipMemcpyHostToDevice, st));
    HSC_TRY(hipMemcpyAsync(ctx->buf[2], indices, bR, hipMemcpyHostToDevice, st));
    HSC_TRY(hipMemcpyAsync(ctx->buf[3], data, bV, hipMemcpyHostToDevice, st));
    HSC_TRY(hipMemcpyAsync(ctx->buf[4], occ.data(), bR, hipMemcpyHostToDevice, st));
    HSC_TRY(hipMemcpyAsync(ctx->buf[5], occ_ptr.data(), bI, hipMemcpyHostToDevice, st));
    HSC_TRY(hipMemcpyAsync(ctx->buf[7], occ_span.data(), bB, hipMemcpyHostToDevice, st));
    HSC_TRY(hipMemcpyAsync(ctx->buf[9], off.data(), bF, hipMemcpyHostToDevice, st));
    HSC_TRY(hipEventRecord(ctx->ev[1], st));
    if (plan == kPlanOne) {
        hipLaunchKernelGGL(ksvd_sweep_kernel, dim3(P), dim3(kThreads), 0, st, args, d_off, d_off + P);
    } else {                                                            // (P = 1: `args` is the problem)
        HSC_TRY(hipMemsetAsync(args.stats, 0, bS, st));
        const int waves = kGridThreads / 64;
        for (int k = 0; k < K; ++k) {
            const int m = occ_ptr[k + 1] - occ_ptr[k];
            if (m == 0) continue;
            hipLaunchKernelGGL(ksvd_gather_kernel, dim3((m + waves - 1) / waves), dim3(kGridThreads), 0, st, args, k);
            if (use_pca && m >= 2) hipLaunchKernelGGL(ksvd_centre_kernel, dim3(1), dim3(kThreads), 0, st, args, k);
            if (m >= 2)
                hipLaunchKernelGGL(ksvd_gram_kernel, dim3((n2 * n2 + kGridThreads - 1) / kGridThreads), dim3(kGridThreads), 0, st, args, k);
            hipLaunchKernelGGL(ksvd_tail_kernel, dim3(1), dim3(kThreads), 0, st, args, k);
        }
    }
    HSC_TRY(hipGetLastError());
    HSC_TRY(hipEventRecord(ctx->ev[2], st));
    HSC_TRY(hipMemcpyAsync(D, ctx->buf[0], bD, hipMemcpyDeviceToHost, st));
    HSC_TRY(hipMemcpyAsync(data, ctx->buf[3], bV, hipMemcpyDeviceToHost, st));
    HSC_TRY(hipMemcpyAsync(stats.data(), args.stats, bS, hipMemcpyDeviceToHost, st));
    HSC_TRY(hipEventRecord(ctx->ev[3], st));
    HSC_TRY(hipStreamSynchronize(st));
    if (timing_ms)
        if (int rc = hsc::add_times(ctx, 3, timing_ms)) return rc;          // (zeroed above)
    if (out_atom_stats) std::memcpy(out_atom_stats, stats.data(), stats.size() * sizeof(double));
    return HSCKSVD_OK;
}

}  // namespace

extern "C" int hscksvd_update(hscksvd_ctx* ctx, int T, int K, int W, int F, double* D, const int32_t* indptr,
                              const int32_t* indices, double* data, int use_pca, double* out_atom_stats, double* timing_ms)
{
    if (!ctx) return fail(nullptr, HSCKSVD_ERR_INVALID, "hscksvd_update: ctx is NULL");
    if (T < 1 || K < 1 || W < 1 || F < 1)
        return fail(ctx, HSCKSVD_ERR_INVALID, "hscksvd_update: bad shape T = %d, K = %d, W = %d, F = %d", T, K, W, F);
    const int32_t row_offsets[2] = {0, T};
    return run_update(ctx, "hscksvd_update", false, 1, nullptr, 1, row_offsets, K, W, F, D, indptr, indices, data, use_pca,
                      kPlanOne, out_atom_stats, timing_ms);
}

extern "C" int hscksvd_update_batch(hscksvd_ctx* ctx, int B, int T, int K, int W, int F, double* D, const int64_t* entry_offsets,
                                    const int32_t* indptr, const int32_t* indices, double* data, int use_pca, double* out_atom_stats,
                                    double* timing_ms)
{
    const char* fn = "hscksvd_update_batch";
    if (!ctx) return fail(nullptr, HSCKSVD_ERR_INVALID, "%s: ctx is NULL", fn);
    if (B < 1 || T < 1 || K < 1 || W < 1 || F < 1)
        return fail(ctx, HSCKSVD_ERR_INVALID, "%s: bad shape B = %d, T = %d, K = %d, W = %d, F = %d", fn, B, T, K, W, F);
    const int32_t row_offsets[2] = {0, T};
    return run_update(ctx, fn, true, B, entry_offsets, 1, row_offsets, K, W, F, D, indptr, indices, data, use_pca, kPlanOne,
                      out_atom_stats, timing_ms);
}

extern "C" int hscksvd_update_corpus(hscksvd_ctx* ctx, int B, const int32_t* row_offsets, int K, int W, int F, double* D,
                                     const int32_t* indptr, const int32_t* indices, double* data, int use_pca, int plan,
                                     double* out_atom_stats, double* timing_ms)
{
    const char* fn = "hscksvd_update_corpus";
    if (!ctx) return fail(nullptr, HSCKSVD_ERR_INVALID, "%s: ctx is NULL", fn);
    if (B < 1 || K < 1 || W < 1 || F < 1)
        return fail(ctx, HSCKSVD_ERR_INVALID, "%s: bad shape B = %d, K = %d, W = %d, F = %d", fn, B, K, W, F);
    if (!row_offsets) return fail(ctx, HSCKSVD_ERR_INVALID, "%s: row_offsets is NULL", fn);
    if (row_offsets[0] != 0) return fail(ctx, HSCKSVD_ERR_INVALID, "%s: row_offsets[0] = %d, expected 0", fn, row_offsets[0]);
    for (int b = 0; b < B; ++b) {
        if (row_offsets[b + 1] < row_offsets[b]) return fail(ctx, HSCKSVD_ERR_INVALID, "%s: row_offsets decreases at signal %d", fn, b);
        if (row_offsets[b + 1] == row_offsets[b]) return fail(ctx, HSCKSVD_ERR_INVALID, "%s: signal %d is empty", fn, b);
    }
    if (plan != kPlanAuto && plan != kPlanOne && plan != kPlanWide)
        return fail(ctx, HSCKSVD_ERR_UNSUPPORTED, "%s: unknown plan %d (0 auto, 1 one workgroup, 2 wide)", fn, plan);
    return run_update(ctx, fn, false, 1, nullptr, B, row_offsets, K, W, F, D, indptr, indices, data, use_pca, plan, out_atom_stats,
                      timing_ms);
}

