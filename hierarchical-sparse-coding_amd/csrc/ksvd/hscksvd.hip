// hscksvd.hip -- libhscksvd.so: the dictionary update of the convolutional K-SVD learner (hsc/modeling.py:591-633)
// on gfx950, C ABI in include/hscksvd.h.  DESIGN.md section 13.
//
// One sweep is ONE launch of ksvd_sweep_kernel on ONE workgroup of 1024 threads: the atoms depend on each other in
// order (atom k reads the new atoms and coefficients of every k' < k), so they run one after the other inside the
// kernel, separated by workgroup barriers, and never wait for the host.  Per atom k with m occurrences:
//   1. gather: wave w builds the patches i = w, w + 16, ...  Lane l < W*F owns sample (s, f) = (l / F, l % F) at
//      time tau = t_i - (W-1)/2 + s.  For every other column j the lanes binary-search column j's rows for the
//      entries within W-1 of t_i (lane j % 64 searches column j), then the wave walks those entries in CSC order
//      (column ascending, row ascending) and adds c * D[j][tau - t_e + (W-1)/2][f] for the taps that hit: the host
//      overlap-add's sum, term by term.  The patches go to a global scratch [m][W*F].
//   2. (PCA branch, m >= 2) centre the patches per component.
//   3. Gram matrix G = sum_i P_i P_i^T (one thread per entry, i ascending) into LDS.
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
    int T, K, W, F, use_pca;
    double* D;                 // [K][W*F], updated in place
    const int* indptr;         // [K+1]
    const int* rows;           // [nnz]
    double* vals;              // [nnz], updated in place
    const int* occ;            // entry ids of every atom's occurrences, atom after atom
    const int* occ_ptr;        // [K+1]
    double* P;                 // scratch [max m][W*F]
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

__global__ __launch_bounds__(kThreads) void ksvd_sweep_kernel(SweepArgs a)
{
    __shared__ double G[kMaxN][kMaxN + 1];     // +1: the column step walks a column
    __shared__ double Vt[kMaxN][kMaxN];        // Vt[j] = eigenvector estimate j
    __shared__ double u[kMaxN];
    __shared__ double rot_c[kMaxN / 2], rot_s[kMaxN / 2];
    __shared__ int rot_p[kMaxN / 2], rot_q[kMaxN / 2];
    __shared__ int rotated;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int T = a.T, K = a.K, W = a.W, F = a.F, n = W * F, lead = (W - 1) / 2;
    const int n2 = n + (n & 1);
    const int half = n2 / 2;

    for (int k = 0; k < K; ++k) {
        const int o0 = a.occ_ptr[k], m = a.occ_ptr[k + 1] - o0;
        double* st = a.stats + (size_t)k * kStats;
        if (m == 0) {
            if (tid < kStats) st[tid] = 0.0;
            continue;
        }
        const bool pca = a.use_pca != 0;

        // ---- 1. patches
        for (int i = wave; i < m; i += kWaves) {
            const int ti = a.rows[a.occ[o0 + i]];
            const int s = lane / F, f = lane - s * F;
            const int tau = ti - lead + s;
            const bool live = lane < n && tau >= 0 && tau < T;
            double acc = 0.0;
            for (int cb = 0; cb < K; cb += 64) {
                const int j = cb + lane;
                int lo = 0, hi = 0;
                if (j < K && j != k) {
                    const int b = a.indptr[j], e = a.indptr[j + 1];
                    lo = lower_bound(a.rows, b, e, ti - (W - 1));
                    hi = lower_bound(a.rows, lo, e, ti + W);
                }
                const int nc = min(64, K - cb);
                for (int jj = 0; jj < nc; ++jj) {
                    const int l0 = __shfl(lo, jj), h0 = __shfl(hi, jj);
                    const double* Dj = a.D + (size_t)(cb + jj) * n;
                    for (int e = l0; e < h0; ++e) {
                        const double c = a.vals[e];
                        if (c == 0.0) continue;                       // reconstructSignal skips c == 0
                        const int tap = tau - (a.rows[e] - lead);
                        if (live && tap >= 0 && tap < W) {
                            const double term = c * Dj[tap * F + f];
                            acc = acc + term;
                        }
                    }
                }
            }
            if (lane < n) a.P[(size_t)i * n + lane] = live ? acc : 0.0;
        }
        __syncthreads();

        // ---- 2. centring (the reference's pca: data -= data.mean(axis=0))
        if (pca && m >= 2) {
            if (tid < n) {
                double sum = 0.0;
                for (int i = 0; i < m; ++i) sum = sum + a.P[(size_t)i * n + tid];
                const double mean = sum / (double)m;
                for (int i = 0; i < m; ++i) a.P[(size_t)i * n + tid] = a.P[(size_t)i * n + tid] - mean;
            }
            __syncthreads();
        }

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
                double g = 0.0;
                if (r < n && c < n)
                    for (int i = 0; i < m; ++i) g = g + a.P[(size_t)i * n + r] * a.P[(size_t)i * n + c];
                G[r][c] = g;
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
}

}  // namespace

static_assert(HSCKSVD_OK == hsc::OK && HSCKSVD_ERR_INVALID == hsc::ERR_INVALID && HSCKSVD_ERR_NO_DEVICE == hsc::ERR_NO_DEVICE &&
              HSCKSVD_ERR_HIP == hsc::ERR_HIP && HSCKSVD_ERR_UNSUPPORTED == hsc::ERR_UNSUPPORTED && HSCKSVD_ERR_ALLOC == hsc::ERR_ALLOC,
              "include/hscksvd.h and common/hsc_lib.h disagree on a status");

struct HSC_HIDDEN hscksvd_ctx : hsc::CtxBase {
    hipEvent_t ev[4] = {};
    hsc::Buffers<7> buf;               // D, indptr, rows, vals, occ, occ_ptr + stats, P
};

using hsc::fail;

extern "C" int hscksvd_version(void) { return 1; }

extern "C" const char* hscksvd_last_error(hscksvd_ctx* ctx) { return hsc::last_error(ctx); }

extern "C" int hscksvd_create(hscksvd_ctx** out, int device_id) { return hsc::create(out, device_id, "hscksvd_create"); }

extern "C" void hscksvd_destroy(hscksvd_ctx* ctx) { hsc::destroy(ctx); }

extern "C" int hscksvd_update(hscksvd_ctx* ctx, int T, int K, int W, int F, double* D, const int32_t* indptr,
                              const int32_t* indices, double* data, int use_pca, double* out_atom_stats, double* timing_ms)
{
    if (!ctx) return fail(nullptr, HSCKSVD_ERR_INVALID, "hscksvd_update: ctx is NULL");
    if (T < 1 || K < 1 || W < 1 || F < 1)
        return fail(ctx, HSCKSVD_ERR_INVALID, "hscksvd_update: bad shape T = %d, K = %d, W = %d, F = %d", T, K, W, F);
    if (W * F > kMaxN)
        return fail(ctx, HSCKSVD_ERR_UNSUPPORTED, "hscksvd_update: W * F = %d exceeds the limit of %d", W * F, kMaxN);
    if (use_pca && F != 1)
        return fail(ctx, HSCKSVD_ERR_UNSUPPORTED, "hscksvd_update: the PCA branch needs F = 1 (got F = %d)", F);
    if (!D || !indptr) return fail(ctx, HSCKSVD_ERR_INVALID, "hscksvd_update: D or indptr is NULL");
    if (indptr[0] != 0) return fail(ctx, HSCKSVD_ERR_INVALID, "hscksvd_update: indptr[0] = %d, expected 0", indptr[0]);
    for (int k = 0; k < K; ++k)
        if (indptr[k + 1] < indptr[k])
            return fail(ctx, HSCKSVD_ERR_INVALID, "hscksvd_update: indptr decreases at column %d", k);
    const int nnz = indptr[K];
    if (nnz > 0 && (!indices || !data)) return fail(ctx, HSCKSVD_ERR_INVALID, "hscksvd_update: indices or data is NULL");
    for (int k = 0; k < K; ++k)
        for (int e = indptr[k]; e < indptr[k + 1]; ++e) {
            if (indices[e] < 0 || indices[e] >= T)
                return fail(ctx, HSCKSVD_ERR_INVALID, "hscksvd_update: row %d of entry %d is outside [0, %d)", indices[e], e, T);
            if (e > indptr[k] && indices[e] <= indices[e - 1])
                return fail(ctx, HSCKSVD_ERR_INVALID, "hscksvd_update: the rows of column %d are not strictly ascending", k);
        }
    const int n = W * F;

    // occurrences: column k's entries whose value is not 0.0 (they keep their values until atom k's turn)
    std::vector<int> occ_ptr((size_t)K + 1, 0), occ;
    occ.reserve(nnz);
    int max_m = 0;
    for (int k = 0; k < K; ++k) {
        for (int e = indptr[k]; e < indptr[k + 1]; ++e)
            if (data[e] != 0.0) occ.push_back(e);
        occ_ptr[k + 1] = (int)occ.size();
        max_m = std::max(max_m, occ_ptr[k + 1] - occ_ptr[k]);
    }
    std::vector<double> stats((size_t)K * kStats, 0.0);
    if (timing_ms) timing_ms[0] = timing_ms[1] = timing_ms[2] = 0.0;
    if (occ.empty()) {
        if (out_atom_stats) std::memcpy(out_atom_stats, stats.data(), stats.size() * sizeof(double));
        return HSCKSVD_OK;                                              // no atom occurs: nothing changes
    }

    HSC_TRY(hipSetDevice(ctx->device));
    const size_t bD = (size_t)K * n * sizeof(double), bI = (size_t)(K + 1) * sizeof(int),
                 bR = (size_t)nnz * sizeof(int), bV = (size_t)nnz * sizeof(double), bO = occ.size() * sizeof(int),
                 bS = (size_t)K * kStats * sizeof(double), bP = (size_t)max_m * n * sizeof(double);
    const size_t bytes[7] = {bD, bI, bR, bV, bO, bI + bS + 16, bP};
    if (int rc = ctx->buf.ensure(ctx, bytes, "hscksvd_update")) return rc;
    int* d_occ_ptr = (int*)ctx->buf[5];
    double* d_stats = (double*)((char*)ctx->buf[5] + (bI + 15) / 16 * 16);
    hipStream_t st = ctx->stream;
    HSC_TRY(hipEventRecord(ctx->ev[0], st));
    HSC_TRY(hipMemcpyAsync(ctx->buf[0], D, bD, hipMemcpyHostToDevice, st));
    HSC_TRY(hipMemcpyAsync(ctx->buf[1], indptr, bI, hipMemcpyHostToDevice, st));
    HSC_TRY(hipMemcpyAsync(ctx->buf[2], indices, bR, hipMemcpyHostToDevice, st));
    HSC_TRY(hipMemcpyAsync(ctx->buf[3], data, bV, hipMemcpyHostToDevice, st));
    HSC_TRY(hipMemcpyAsync(ctx->buf[4], occ.data(), bO, hipMemcpyHostToDevice, st));
    HSC_TRY(hipMemcpyAsync(d_occ_ptr, occ_ptr.data(), bI, hipMemcpyHostToDevice, st));
    HSC_TRY(hipEventRecord(ctx->ev[1], st));
    SweepArgs args;
    args.T = T;
    args.K = K;
    args.W = W;
    args.F = F;
    args.use_pca = use_pca ? 1 : 0;
    args.D = (double*)ctx->buf[0];
    args.indptr = (const int*)ctx->buf[1];
    args.rows = (const int*)ctx->buf[2];
    args.vals = (double*)ctx->buf[3];
    args.occ = (const int*)ctx->buf[4];
    args.occ_ptr = d_occ_ptr;
    args.P = (double*)ctx->buf[6];
    args.stats = d_stats;
    hipLaunchKernelGGL(ksvd_sweep_kernel, dim3(1), dim3(kThreads), 0, st, args);
    HSC_TRY(hipGetLastError());
    HSC_TRY(hipEventRecord(ctx->ev[2], st));
    HSC_TRY(hipMemcpyAsync(D, ctx->buf[0], bD, hipMemcpyDeviceToHost, st));
    HSC_TRY(hipMemcpyAsync(data, ctx->buf[3], bV, hipMemcpyDeviceToHost, st));
    HSC_TRY(hipMemcpyAsync(stats.data(), d_stats, bS, hipMemcpyDeviceToHost, st));
    HSC_TRY(hipEventRecord(ctx->ev[3], st));
    HSC_TRY(hipStreamSynchronize(st));
    if (timing_ms)
        if (int rc = hsc::add_times(ctx, 3, timing_ms)) return rc;          // (zeroed above)
    if (out_atom_stats) std::memcpy(out_atom_stats, stats.data(), stats.size() * sizeof(double));
    return HSCKSVD_OK;
}
