// hscnmf.hip -- libhscnmf.so: convolutional NMF coefficients (hsc/modeling.py:662-747) on gfx950, C ABI in
// include/hscnmf.h.  DESIGN.md section 10.
//
// Per signal, A [L = T-W+1 rows][K] (rows past T-W never reach a reconstruction and are not kept).  One
// multiplicative step t is one launch of nmf_step_kernel; a workgroup owns kRows rows s of A and
//   1. forms P[r][j*F+f] = sum_k A[r][k] D[k][j][f] on the matrix cores for the rows r it needs (its own rows
//      shifted by t, plus a halo of W-1 rows before them: recomputed, never exchanged),
//   2. sums the diagonals recon[n][f] = sum_j P[n-j][j*F+f] (j ascending),
//   3. R = x / |recon|, U[s][k] = (sum_f D[k][t][f] R[s+t][f]) / (sum_f D[k][t][f]), A'[s][k] = A[s][k] * U[s][k],
// reading A from one buffer of a ping-pong pair and writing the other.  After the W steps of an iteration
// nmf_residual_kernel reconstructs once more (residual, per-tile max|r| and sum r^2) and nmf_decide_kernel takes
// the reference's stop decision per signal on the device; a finished signal's workgroups return at once.
// Every kernel that works on a tile is a template on a geometry (Uniform, Ragged<one flag per signal?>): where the tile's
// signal lies, its lengths, its stop flag and its dictionary.  hscnmf_learn (the dictionary learner) adds, per iteration,
// the ratio, partial and update kernels of section 12; hscnmf_learn_corpus (one dictionary from many signals of different
// lengths) runs the ragged geometry with one flag and sums the update over the signals, section 18;
// hscnmf_compute_ragged runs the coder over the ragged geometry with a flag per signal, in chunks of whole signals,
// section 23.  On the host the entry points share one argument ladder (check_args), one owner of a call's device memory
// (DeviceBuffers), the step launches and the stop poll; the two coders share their chunk (Coder::chunk).
#include "../../../include/hscnmf.h"
#include "../common/hsc_lib.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

namespace {

constexpr int kThreads = 256;                 // four waves
constexpr int kRows = 128;                    // A rows (and reconstructed samples) per workgroup
constexpr int kLdsBytes = 64 * 1024;          // P slab + reconstruction tile

typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef double f64x2 __attribute__((ext_vector_type(2)));
typedef double f64x4 __attribute__((ext_vector_type(4)));

template <typename T> struct Tile;
// v_mfma_f32_32x32x2_f32: A lane l = row l&31, k l>>5; B k l>>5, col l&31; C col l&31, row (r&3)+8(r>>2)+4(l>>5)
template <> struct Tile<float> { static constexpr int RB = 32, CB = 32; };
// v_mfma_f64_16x16x4_f64: A lane l = row l&15, k l>>4; B k l>>4, col l&15; C col l&15, row (l>>4)+4r
template <> struct Tile<double> { static constexpr int RB = 16, CB = 16; };

// One RB x CB block of P = A . D (rows r0.., columns c0..), written to LDS out[row][col] (row stride ldo).
// A rows outside [0, L) are the reference's zero padding.  The k order inside the MFMA chain is fixed
// (eight k per load group), so a block's value does not depend on anything but its inputs.
__device__ __forceinline__ void p_block(const float* __restrict__ A, int L, int K, const float* __restrict__ D, int NW,
                                        int r0, int c0, float* out, int ldo)
{
    const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const int r = r0 + i, c = c0 + i;
    const bool vr = r >= 0 && r < L, vc = c < NW;
    const float* ar = A + (size_t)(vr ? r : 0) * K;
    f32x16 acc = {};
    if ((K & 7) == 0) {
        for (int k0 = 0; k0 < K; k0 += 8) {
            const int kb = k0 + 4 * h;
            const f32x4 a = vr ? *reinterpret_cast<const f32x4*>(ar + kb) : f32x4{0.f, 0.f, 0.f, 0.f};
            float b[4];
#pragma unroll
            for (int q = 0; q < 4; ++q) b[q] = vc ? D[(size_t)(kb + q) * NW + c] : 0.f;
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[0], b[0], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[1], b[1], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[2], b[2], acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a[3], b[3], acc, 0, 0, 0);
        }
    } else {
        for (int k0 = 0; k0 < K; k0 += 8) {
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int k = k0 + 4 * h + q;
                const float a = (vr && k < K) ? ar[k] : 0.f;
                const float b = (vc && k < K) ? D[(size_t)k * NW + c] : 0.f;
                acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, b, acc, 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 16; ++e) out[((e & 3) + 8 * (e >> 2) + 4 * h) * ldo + i] = acc[e];
}

__device__ __forceinline__ void p_block(const double* __restrict__ A, int L, int K, const double* __restrict__ D, int NW,
                                        int r0, int c0, double* out, int ldo)
{
    const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const int r = r0 + i, c = c0 + i;
    const bool vr = r >= 0 && r < L, vc = c < NW;
    const double* ar = A + (size_t)(vr ? r : 0) * K;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    if ((K & 7) == 0) {
        for (int k0 = 0; k0 < K; k0 += 8) {
            const int kb = k0 + 2 * g;
            const f64x2 a = vr ? *reinterpret_cast<const f64x2*>(ar + kb) : f64x2{0.0, 0.0};
            const double b0 = vc ? D[(size_t)kb * NW + c] : 0.0;
            const double b1 = vc ? D[(size_t)(kb + 1) * NW + c] : 0.0;
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[0], b0, acc, 0, 0, 0);
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[1], b1, acc, 0, 0, 0);
        }
    } else {
        for (int k0 = 0; k0 < K; k0 += 8) {
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                const int k = k0 + 2 * g + q;
                const double a = (vr && k < K) ? ar[k] : 0.0;
                const double b = (vc && k < K) ? D[(size_t)k * NW + c] : 0.0;
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, acc, 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) out[(g + 4 * e) * ldo + i] = acc[e];
}

// rec[nl][f] = sum_j sum_k A[nbase+nl-j][k] D[k][j][f] for nl in [0, kRows): P rows nbase-(W-1) .. nbase+kRows-1
// (PR of them, a multiple of RB), column blocks `slab` at a time through the LDS slab Pl.
template <typename T>
__device__ void tile_recon(const T* __restrict__ A, int L, int K, const T* __restrict__ D, int W, int F, int nbase,
                           int PR, int slab, T* rec, T* Pl)
{
    constexpr int RB = Tile<T>::RB, CB = Tile<T>::CB;
    const int NW = W * F, ncb = (NW + CB - 1) / CB, nrb = PR / RB, ldo = slab * CB;
    const int wave = threadIdx.x >> 6, rbase = nbase - (W - 1);
    for (int e = threadIdx.x; e < kRows * F; e += kThreads) rec[e] = T(0);
    for (int cb0 = 0; cb0 < ncb; cb0 += slab) {
        const int nb = min(slab, ncb - cb0);
        for (int it = wave; it < nrb * nb; it += kThreads / 64) {
            const int rb = it % nrb, cbi = it / nrb;
            p_block(A, L, K, D, NW, rbase + rb * RB, (cb0 + cbi) * CB, Pl + (size_t)rb * RB * ldo + cbi * CB, ldo);
        }
        __syncthreads();
        const int c_lo = cb0 * CB, c_hi = min((cb0 + nb) * CB, NW);
        for (int e = threadIdx.x; e < kRows * F; e += kThreads) {
            const int nl = e / F, f = e - nl * F;
            T acc = rec[e];
            for (int c = c_lo + ((f - c_lo % F) + F) % F; c < c_hi; c += F) {
                const int j = c / F;
                acc = acc + Pl[(size_t)(nl + W - 1 - j) * ldo + (c - c_lo)];
            }
            rec[e] = acc;
        }
        __syncthreads();
    }
}

// Where a workgroup's signal and tile lie, and what belongs to the signal.  Uniform: B signals of one length, the signal
// on blockIdx.y and the tile on blockIdx.x, a stop flag per signal and a dictionary per signal dstride values apart
// (hscnmf_compute: 0, one dictionary for the batch; hscnmf_learn: K*W*F).
struct Uniform {
    int L, Tn;
    size_t dstride;
    __device__ int signal() const { return blockIdx.y; }
    __device__ int tile() const { return blockIdx.x; }
    __device__ int flag(int b) const { return b; }
    __device__ int rows(int) const { return L; }
    __device__ int samples(int) const { return Tn; }
    __device__ size_t row0(int b) const { return (size_t)b * L; }           // first coefficient row of signal b
    __device__ size_t sample0(int b) const { return (size_t)b * Tn; }       // first sample of signal b
    __device__ size_t dict0(int b) const { return (size_t)b * dstride; }    // first value of signal b's dictionary
    __device__ size_t slot(int b) const { return (size_t)b * gridDim.x + blockIdx.x; }   // the workgroup's partials
    __device__ size_t part0(int b) const { return (size_t)b * ((Tn + kRows - 1) / kRows); }   // signal b's first sample tile
};

// one signal of a corpus: its first sample and coefficient row in the stacks, its first row tile and sample tile in the
// flat tile tables (a signal's tiles are consecutive and ascending), its length and its L = T - W + 1
struct SignalInfo {
    long long x0, a0, rt0, st0;
    int T, L;
};

// Ragged: signals of different lengths stacked without padding, a 1-D grid with one (signal, tile) pair per workgroup, one
// dictionary, and one stop flag for the corpus (hscnmf_learn_corpus) or one per signal (hscnmf_compute_ragged).
template <bool PerSignal>
struct Ragged {
    const SignalInfo* __restrict__ sig;
    const int2* __restrict__ tiles;                                         // (signal, tile) of workgroup blockIdx.x
    __device__ int signal() const { return tiles[blockIdx.x].x; }
    __device__ int tile() const { return tiles[blockIdx.x].y; }
    __device__ int flag(int b) const { return PerSignal ? b : 0; }
    __device__ int rows(int b) const { return sig[b].L; }
    __device__ int samples(int b) const { return sig[b].T; }
    __device__ size_t row0(int b) const { return (size_t)sig[b].a0; }
    __device__ size_t sample0(int b) const { return (size_t)sig[b].x0; }
    __device__ size_t dict0(int) const { return 0; }
    __device__ size_t slot(int) const { return blockIdx.x; }
    __device__ size_t part0(int b) const { return (size_t)sig[b].st0; }
};

template <typename T, typename G>
__global__ __launch_bounds__(kThreads) void nmf_step_kernel(const T* __restrict__ Ain, T* __restrict__ Aout,
                                                            const T* __restrict__ X, const T* __restrict__ D,
                                                            const int* __restrict__ done, G g, int K, int W, int F, int t,
                                                            int PR, int slab)
{
    const int b = g.signal();
    const int L = g.rows(b), Tn = g.samples(b);       // (named before the flag: the table's address loads beside the tiles')
    if (done[g.flag(b)]) return;
    D += g.dict0(b);
    extern __shared__ __align__(16) unsigned char smem[];
    T* rec = reinterpret_cast<T*>(smem);
    T* Pl = rec + kRows * F;
    const int s0 = g.tile() * kRows;
    const T* A = Ain + g.row0(b) * K;
    const int nbase = s0 + t;                                        // R[s+t] for the own rows s
    tile_recon(A, L, K, D, W, F, nbase, PR, slab, rec, Pl);
    for (int e = threadIdx.x; e < kRows * F; e += kThreads) {
        const int nl = e / F, f = e - nl * F, n = nbase + nl;
        rec[e] = n < Tn ? X[(g.sample0(b) + n) * F + f] / fabs(rec[e]) : T(0);
    }
    __syncthreads();
    const int rows = min(kRows, L - s0);
    T* Ao = Aout + g.row0(b) * K;
    for (int e = threadIdx.x; e < rows * K; e += kThreads) {
        const int sl = e / K, k = e - sl * K;
        const T* d = D + ((size_t)k * W + t) * F;
        T num = T(0), den = T(0);
        for (int f = 0; f < F; ++f) {
            num = num + d[f] * rec[sl * F + f];
            den = den + d[f];
        }
        const T u = num / den;
        const size_t o = (size_t)(s0 + sl) * K + k;
        Ao[o] = A[o] * u;
    }
}

template <typename T, typename G>
__global__ __launch_bounds__(kThreads) void nmf_residual_kernel(const T* __restrict__ Abuf, const T* __restrict__ X,
                                                                const T* __restrict__ D, const int* __restrict__ done,
                                                                T* __restrict__ resid, double* __restrict__ part, G g, int K,
                                                                int W, int F, int PR, int slab)
{
    const int b = g.signal();
    const int L = g.rows(b), Tn = g.samples(b);       // (named before the flag: the table's address loads beside the tiles')
    if (done[g.flag(b)]) return;
    D += g.dict0(b);
    extern __shared__ __align__(16) unsigned char smem[];
    T* rec = reinterpret_cast<T*>(smem);
    T* Pl = rec + kRows * F;
    const int n0 = g.tile() * kRows;
    tile_recon(Abuf + g.row0(b) * K, L, K, D, W, F, n0, PR, slab, rec, Pl);
    double mx = 0.0, ss = 0.0;
    for (int e = threadIdx.x; e < kRows * F; e += kThreads) {
        const int n = n0 + e / F;
        if (n >= Tn) break;
        const size_t o = (g.sample0(b) + n0) * F + e;
        const T r = X[o] - rec[e];
        resid[o] = r;
        const double rd = (double)r;
        mx = fmax(mx, fabs(rd));
        ss = ss + rd * rd;
    }
    double* red = reinterpret_cast<double*>(Pl);                     // (the slab is free again)
    red[threadIdx.x] = mx;
    red[kThreads + threadIdx.x] = ss;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            red[threadIdx.x] = fmax(red[threadIdx.x], red[threadIdx.x + w]);
            red[kThreads + threadIdx.x] = red[kThreads + threadIdx.x] + red[kThreads + threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        part[g.slot(b) * 2] = red[0];
        part[g.slot(b) * 2 + 1] = red[kThreads];
    }
}

// A signal's max|r| and sum r^2 from its ntiles sample-tile partials pb, by a workgroup of 64 threads: the threads stride
// the tiles, then the tree; thread 0 hands the two to `then(max, sum)`.
template <typename Then>
__device__ __forceinline__ void signal_reduce(const double* __restrict__ pb, int ntiles, Then then)
{
    __shared__ double smx[64], sss[64];
    double mx = 0.0, ss = 0.0;
    for (int i = threadIdx.x; i < ntiles; i += 64) {
        mx = fmax(mx, pb[(size_t)i * 2]);
        ss = ss + pb[(size_t)i * 2 + 1];
    }
    smx[threadIdx.x] = mx;
    sss[threadIdx.x] = ss;
    __syncthreads();
    for (int w = 32; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
            smx[threadIdx.x] = fmax(smx[threadIdx.x], smx[threadIdx.x + w]);
            sss[threadIdx.x] = sss[threadIdx.x] + sss[threadIdx.x + w];
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) then(smx[0], sss[0]);
}

// the stop rules of hsc/modeling.py:729-740, in that order, after it1 iterations
__device__ __forceinline__ int stop_code(int it1, double residual_scale, double snr, const hscnmf_params& p)
{
    int code = HSCNMF_STOP_RUNNING;
    if (it1 >= p.max_iterations) code = HSCNMF_STOP_MAX_ITERATIONS;
    else if (p.has_residual_scale && residual_scale <= p.tolerance_residual_scale) code = HSCNMF_STOP_RESIDUAL_SCALE;
    else if (p.has_snr && snr >= p.tolerance_snr) code = HSCNMF_STOP_SNR;
    return code;
}

// one workgroup (64 threads) per signal with a stop flag of its own: the signal's statistics and its stop decision
template <typename G>
__global__ __launch_bounds__(64) void nmf_decide_kernel(const double* __restrict__ part, G g,
                                                        const double* __restrict__ energy, int* __restrict__ done,
                                                        int* __restrict__ iters, int* __restrict__ stop,
                                                        double* __restrict__ snr, double* __restrict__ rscale,
                                                        int it1, hscnmf_params p)
{
    const int b = blockIdx.x;
    if (done[b]) return;
    signal_reduce(part + g.part0(b) * 2, (g.samples(b) + kRows - 1) / kRows, [&](double rs, double ss) {
        const double s = 10.0 * log10(energy[b] / ss);
        const int code = stop_code(it1, rs, s, p);
        iters[b] = it1;
        snr[b] = s;
        rscale[b] = rs;
        stop[b] = code;
        if (code != HSCNMF_STOP_RUNNING) done[b] = 1;
    });
}

// ---- the dictionary update of the learner (hsc/modeling.py:383-395), DESIGN.md section 12 ----------------------------

// R[n][f] = X[n][f] / |recon[n][f]| for the samples n0 .. n0+kRows-1 of the tile (the updated A, the old D)
template <typename T, typename G>
__global__ __launch_bounds__(kThreads) void nmf_ratio_kernel(const T* __restrict__ Abuf, const T* __restrict__ X,
                                                             const T* __restrict__ D, const int* __restrict__ done,
                                                             T* __restrict__ R, G g, int K, int W, int F, int PR, int slab)
{
    const int b = g.signal();
    const int L = g.rows(b), Tn = g.samples(b);       // (named before the flag: the table's address loads beside the tiles')
    if (done[g.flag(b)]) return;
    extern __shared__ __align__(16) unsigned char smem[];
    T* rec = reinterpret_cast<T*>(smem);
    T* Pl = rec + kRows * F;
    const int n0 = g.tile() * kRows;
    tile_recon(Abuf + g.row0(b) * K, L, K, D + g.dict0(b), W, F, n0, PR, slab, rec, Pl);
    for (int e = threadIdx.x; e < kRows * F; e += kThreads) {
        const int n = n0 + e / F;
        if (n >= Tn) break;
        const size_t o = (g.sample0(b) + n0) * F + e;
        R[o] = X[o] / fabs(rec[e]);
    }
}

// One RB x CB block of C[k][c] = sum_{sl < rows} A[s0+sl][k] Rl[sl*F + c] (c = t*F+f: the Hankel matrix of the R tile,
// Rl[(sl+t)*F+f] = Rl[sl*F+c]).  MFMA A operand: k across lanes (A is [L][K], so a half-wave loads 32 consecutive
// values); B operand from LDS.  The reduction runs over sl in ascending pairs (f32) / quads (f64): fixed order.
__device__ __forceinline__ void dpart_block(const float* __restrict__ A, int rows, int K, const float* Rl, int F, int NW,
                                            int k0, int c0, float* __restrict__ out, int ld)
{
    const int lane = threadIdx.x & 63, i = lane & 31, h = lane >> 5;
    const int k = k0 + i, c = c0 + i;
    const bool vk = k < K, vc = c < NW;
    f32x16 acc = {};
    for (int s2 = 0; s2 < rows; s2 += 2) {
        const int sl = s2 + h;
        const bool vs = sl < rows;
        const float a = (vk && vs) ? A[(size_t)sl * K + k] : 0.f;
        const float r = (vc && vs) ? Rl[sl * F + c] : 0.f;
        acc = __builtin_amdgcn_mfma_f32_32x32x2f32(a, r, acc, 0, 0, 0);
    }
    if (!vc) return;
#pragma unroll
    for (int e = 0; e < 16; ++e) {
        const int kr = k0 + (e & 3) + 8 * (e >> 2) + 4 * h;
        if (kr < K) out[(size_t)kr * ld + c] = acc[e];
    }
}

__device__ __forceinline__ void dpart_block(const double* __restrict__ A, int rows, int K, const double* Rl, int F, int NW,
                                            int k0, int c0, double* __restrict__ out, int ld)
{
    const int lane = threadIdx.x & 63, i = lane & 15, g = lane >> 4;
    const int k = k0 + i, c = c0 + i;
    const bool vk = k < K, vc = c < NW;
    f64x4 acc = {0.0, 0.0, 0.0, 0.0};
    for (int s4 = 0; s4 < rows; s4 += 4) {
        const int sl = s4 + g;
        const bool vs = sl < rows;
        const double a = (vk && vs) ? A[(size_t)sl * K + k] : 0.0;
        const double r = (vc && vs) ? Rl[sl * F + c] : 0.0;
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a, r, acc, 0, 0, 0);
    }
    if (!vc) return;
#pragma unroll
    for (int e = 0; e < 4; ++e) {
        const int kr = k0 + g + 4 * e;
        if (kr < K) out[(size_t)kr * ld + c] = acc[e];
    }
}

// Partials of one row tile (s0 .. s0+kRows-1, rows < L only): part[slot][k][c] = sum_s A[s][k] R[s+t][f]
// (c = t*F+f < NW) and part[slot][k][NW] = sum_s A[s][k] (ascending s), for the update kernel to sum; slot: the
// signal's tiles in ascending order, signal after signal.
template <typename T, typename G>
__global__ __launch_bounds__(kThreads) void nmf_dpart_kernel(const T* __restrict__ Abuf, const T* __restrict__ R,
                                                             const int* __restrict__ done, T* __restrict__ part, G g, int K,
                                                             int W, int F)
{
    constexpr int RB = Tile<T>::RB, CB = Tile<T>::CB;
    const int b = g.signal();
    const int L = g.rows(b), Tn = g.samples(b);       // (named before the flag: the table's address loads beside the tiles')
    if (done[g.flag(b)]) return;
    extern __shared__ __align__(16) unsigned char smem[];
    T* Rl = reinterpret_cast<T*>(smem);                              // R samples s0 .. s0+kRows+W-2 (0 past T)
    const int s0 = g.tile() * kRows, NW = W * F, ld = NW + 1, nr = (kRows + W - 1) * F;
    const T* Rb = R + (g.sample0(b) + s0) * F;
    for (int e = threadIdx.x; e < nr; e += kThreads) Rl[e] = s0 + e / F < Tn ? Rb[e] : T(0);
    __syncthreads();
    const int rows = min(kRows, L - s0);
    const T* A = Abuf + (g.row0(b) + s0) * K;
    T* out = part + g.slot(b) * K * ld;
    for (int k = threadIdx.x; k < K; k += kThreads) {
        T acc = T(0);
        for (int sl = 0; sl < rows; ++sl) acc = acc + A[(size_t)sl * K + k];
        out[(size_t)k * ld + NW] = acc;
    }
    const int nkb = (K + RB - 1) / RB, ncb = (NW + CB - 1) / CB;
    for (int it = threadIdx.x >> 6; it < nkb * ncb; it += kThreads / 64)
        dpart_block(A, rows, K, Rl, F, NW, (it % nkb) * RB, (it / nkb) * CB, out, ld);
}

// One workgroup per (atom k, learner b): N and den summed over the tiles in ascending order, D[k] *= N / den, then
// D[k] /= ||D[k]|| when the norm is > 0 (hsc/utils.py:67-74).  IEEE division and sqrt; no atomics.  The corpus learner is
// the grid [K, 1] over nmf_dsum_kernel's sums: one learner whose "tiles" are the signals, in ascending order.
template <typename T>
__global__ __launch_bounds__(kThreads) void nmf_dupdate_kernel(const T* __restrict__ part, int ntiles,
                                                               const int* __restrict__ done, T* __restrict__ D, int K, int NW)
{
    const int k = blockIdx.x, b = blockIdx.y;
    if (done[b]) return;
    extern __shared__ __align__(16) unsigned char smem[];
    T* red = reinterpret_cast<T*>(smem);                             // [kThreads] sums of squares, then [NW + 1] sums
    T* sum = red + kThreads;
    const int ld = NW + 1;
    const size_t tstride = (size_t)K * ld;
    const T* p = part + (size_t)b * ntiles * tstride + (size_t)k * ld;
    for (int c = threadIdx.x; c < ld; c += kThreads) {
        T acc = T(0);
        for (int i = 0; i < ntiles; ++i) acc = acc + p[(size_t)i * tstride + c];
        sum[c] = acc;
    }
    __syncthreads();
    T* d = D + ((size_t)b * K + k) * NW;
    const T den = sum[NW];
    T ss = T(0);
    for (int c = threadIdx.x; c < NW; c += kThreads) {
        const T v = d[c] * (sum[c] / den);
        sum[c] = v;
        ss = ss + v * v;
    }
    red[threadIdx.x] = ss;
    __syncthreads();
    for (int w = kThreads / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) red[threadIdx.x] = red[threadIdx.x] + red[threadIdx.x + w];
        __syncthreads();
    }
    const T nrm = sqrt(red[0]);
    for (int c = threadIdx.x; c < NW; c += kThreads) d[c] = nrm > T(0) ? sum[c] / nrm : sum[c];
}

// ---- one dictionary for a corpus (hscnmf_learn_corpus), DESIGN.md section 18 -----------------------------------------

// First level of the corpus update: S[b][k][c] = the sum of signal b's tile partials in ascending tile order, c <= NW
// (nmf_dupdate_kernel's sum, kept per signal).  The partials of a tile are [K][NW + 1] values in a row, so a workgroup
// takes kThreads consecutive ones of them: nchunk workgroups per signal, signal after signal on a 1-D grid.
template <typename T>
__global__ __launch_bounds__(kThreads) void nmf_dsum_kernel(const T* __restrict__ part, const SignalInfo* __restrict__ sig,
                                                            const int* __restrict__ done, T* __restrict__ S,
                                                            unsigned nchunk, size_t tstride)
{
    if (done[0]) return;
    const unsigned b = blockIdx.x / nchunk;
    const size_t e = (size_t)(blockIdx.x - b * nchunk) * kThreads + threadIdx.x;
    if (e >= tstride) return;
    const int ntiles = (sig[b].L + kRows - 1) / kRows;
    const T* p = part + (size_t)sig[b].rt0 * tstride + e;
    T acc = T(0);
    for (int i = 0; i < ntiles; ++i) acc = acc + p[(size_t)i * tstride];
    S[(size_t)b * tstride + e] = acc;
}

// one workgroup (64 threads) per signal: max|r| and sum r^2 of the signal as nmf_decide_kernel forms them, and the
// signal's own SNR and residual scale
__global__ __launch_bounds__(64) void nmf_signal_stats_kernel(const double* __restrict__ part,
                                                              const SignalInfo* __restrict__ sig,
                                                              const double* __restrict__ energy, const int* __restrict__ done,
                                                              double* __restrict__ sigmx, double* __restrict__ sigss,
                                                              double* __restrict__ snr, double* __restrict__ rscale)
{
    const int b = blockIdx.x;
    if (done[0]) return;
    signal_reduce(part + (size_t)sig[b].st0 * 2, (sig[b].T + kRows - 1) / kRows, [&](double mx, double ss) {
        sigmx[b] = mx;
        sigss[b] = ss;
        snr[b] = 10.0 * log10(energy[b] / ss);
        rscale[b] = mx;
    });
}

// One workgroup: the signals' statistics combined in ascending signal order (staged through LDS kThreads at a time, summed
// by one thread), then the stop rules on the corpus.  state: done, iterations, stop; out: snr, scale.
__global__ __launch_bounds__(kThreads) void nmf_decide_corpus_kernel(const double* __restrict__ sigmx,
                                                                     const double* __restrict__ sigss,
                                                                     const double* __restrict__ energy, int B,
                                                                     int* __restrict__ state, double* __restrict__ out,
                                                                     int it1, hscnmf_params p)
{
    if (state[0]) return;
    __shared__ double lmx[kThreads], lss[kThreads], len[kThreads];
    double mx = 0.0, ss = 0.0, en = 0.0;
    for (int b0 = 0; b0 < B; b0 += kThreads) {
        const int n = min(kThreads, B - b0);
        if ((int)threadIdx.x < n) {
            lmx[threadIdx.x] = sigmx[b0 + threadIdx.x];
            lss[threadIdx.x] = sigss[b0 + threadIdx.x];
            len[threadIdx.x] = energy[b0 + threadIdx.x];
        }
        __syncthreads();
        if (threadIdx.x == 0)
            for (int i = 0; i < n; ++i) {
                mx = fmax(mx, lmx[i]);
                ss = ss + lss[i];
                en = en + len[i];
            }
        __syncthreads();
    }
    if (threadIdx.x == 0) {
        const double s = 10.0 * log10(en / ss);
        const int code = stop_code(it1, mx, s, p);
        state[1] = it1;
        state[2] = code;
        out[0] = s;
        out[1] = mx;
        if (code != HSCNMF_STOP_RUNNING) state[0] = 1;
    }
}

}  // namespace

static_assert(HSCNMF_OK == hsc::OK && HSCNMF_ERR_INVALID == hsc::ERR_INVALID && HSCNMF_ERR_NO_DEVICE == hsc::ERR_NO_DEVICE &&
              HSCNMF_ERR_HIP == hsc::ERR_HIP && HSCNMF_ERR_UNSUPPORTED == hsc::ERR_UNSUPPORTED && HSCNMF_ERR_ALLOC == hsc::ERR_ALLOC,
              "include/hscnmf.h and common/hsc_lib.h disagree on a status");

struct HSC_HIDDEN hscnmf_ctx : hsc::CtxBase {
    hipEvent_t ev[4] = {};
};

using hsc::fail;

extern "C" int hscnmf_version(void) { return 2; }

extern "C" const char* hscnmf_last_error(hscnmf_ctx* ctx) { return hsc::last_error(ctx); }

extern "C" int hscnmf_create(hscnmf_ctx** out, int device_id) { return hsc::create(out, device_id, "hscnmf_create"); }

extern "C" void hscnmf_destroy(hscnmf_ctx* ctx) { hsc::destroy(ctx); }

// LDS layout of one workgroup: reconstruction tile [kRows][F], then the P slab [PR][slab * CB] (also the
// residual kernel's reduction scratch, 2 * kThreads doubles)
template <typename T>
static bool lds_plan(int W, int F, int& PR, int& slab, size_t& bytes)
{
    constexpr int RB = Tile<T>::RB, CB = Tile<T>::CB;
    PR = (kRows + W - 1 + RB - 1) / RB * RB;
    const size_t rec = (size_t)kRows * F * sizeof(T), col = (size_t)PR * CB * sizeof(T);
    if (rec + col > (size_t)kLdsBytes) return false;
    const int ncb = (W * F + CB - 1) / CB;
    slab = std::max(1, std::min(ncb, (int)(((size_t)kLdsBytes - rec) / col)));
    bytes = rec + std::max(col * slab, (size_t)2 * kThreads * sizeof(double));
    return bytes <= (size_t)kLdsBytes;
}

namespace {

constexpr int kMaxCorpusSignals = 1 << 22;
// HIP refuses a launch with gridDim.x * blockDim.x >= 2^32: with workgroups of kThreads = 256 a 1-D grid has at most
// 2^24 - 1 workgroups.  The sample tiles (the row tiles are no more) and nmf_dsum_kernel's B * nchunk lie on such grids.
constexpr long long kMaxCorpusGrid = (1LL << 32) / kThreads - 1;

// what the launches of a call share: the shape, lds_plan's answer and the LDS of nmf_dpart_kernel and nmf_dupdate_kernel
struct Plan {
    int K, W, F, PR, slab;
    size_t lds, lds_part, lds_upd;
};

// the calls check_args serves: hscnmf_compute, hscnmf_learn, hscnmf_learn_corpus, and hscnmf_compute_ragged with its plan
enum class Call { Coder, Learner, CorpusLearner, RaggedCoder };

// The argument checks of the five entry points (after their own NULL checks), in one ladder; nothing is allocated before
// them.  lengths: B of them, or the one length of a uniform batch (Coder, Learner).  params: where max_iterations is
// checked here (NULL: not here).  Two refusals have a place of their own per kind of call.  Fills in `pl`.
int check_args(hsc::CtxBase* ctx, const char* fn, Call call, int dtype, const int64_t* lengths, int B, int F, int K, int W,
               const hscnmf_params* params, Plan& pl)
{
    const bool uniform = call == Call::Coder || call == Call::Learner, learner = call == Call::Learner || call == Call::CorpusLearner;
    const bool bad_iterations = params && params->max_iterations < 1;
    auto no_iterations = [&] { return fail(ctx, HSCNMF_ERR_INVALID, "%s: max_iterations = %d", fn, params->max_iterations); };
    auto no_lds = [&] {
        return fail(ctx, HSCNMF_ERR_UNSUPPORTED, "%s: W = %d, F = %d needs more than %d bytes of LDS per workgroup", fn, W, F, kLdsBytes);
    };
    if (!lengths) return fail(ctx, HSCNMF_ERR_INVALID, "%s: NULL argument", fn);
    if (dtype != HSCNMF_F32 && dtype != HSCNMF_F64) return fail(ctx, HSCNMF_ERR_INVALID, "%s: unknown dtype %d", fn, dtype);
    if (B < 1 || K < 1 || F < 1) return fail(ctx, HSCNMF_ERR_INVALID, "%s: B = %d, K = %d, F = %d", fn, B, K, F);
    if (W < 2) return fail(ctx, HSCNMF_ERR_INVALID, "%s: filter width %d (the reference needs W >= 2)", fn, W);
    if (bad_iterations && call == Call::CorpusLearner) return no_iterations();      // a corpus: before its lengths
    if (uniform && lengths[0] < W)
        return fail(ctx, HSCNMF_ERR_INVALID, "%s: signal length %d is shorter than the filter width %d", fn, (int)lengths[0], W);
    for (int b = 0; !uniform && b < B; ++b)
        if (lengths[b] < W)
            return fail(ctx, HSCNMF_ERR_INVALID, "%s: signal %d: length %lld is shorter than the filter width %d", fn, b,
                        (long long)lengths[b], W);
    if (bad_iterations) return no_iterations();                                     // a uniform batch: after its length
    if (call == Call::CorpusLearner && B > kMaxCorpusSignals)
        return fail(ctx, HSCNMF_ERR_UNSUPPORTED, "%s: %d signals (at most %d)", fn, B, kMaxCorpusSignals);
    const int64_t max_lk = ((int64_t)1 << 31) / 8;
    if ((int64_t)W * F > (1 << 24) || (learner && K > 65535) || (uniform && (lengths[0] - W + 1) * K > max_lk))
        return fail(ctx, HSCNMF_ERR_UNSUPPORTED, "%s: shape out of range", fn);
    const size_t item = dtype == HSCNMF_F32 ? sizeof(float) : sizeof(double);
    pl = Plan{K, W, F, 0, 0, 0, (size_t)(kRows + W - 1) * F * item, (size_t)(kThreads + W * F + 1) * item};
    bool fits = dtype == HSCNMF_F32 ? lds_plan<float>(W, F, pl.PR, pl.slab, pl.lds) : lds_plan<double>(W, F, pl.PR, pl.slab, pl.lds);
    if (learner) fits = fits && pl.lds_part <= (size_t)kLdsBytes && pl.lds_upd <= (size_t)kLdsBytes;
    if (!fits && call == Call::RaggedCoder) return no_lds();                        // the ragged coder: before the signals' shapes
    for (int b = 0; !uniform && b < B; ++b)
        if ((lengths[b] - W + 1) * K > max_lk || (call == Call::RaggedCoder && (lengths[b] + kRows - 1) / kRows > kMaxCorpusGrid))
            return fail(ctx, HSCNMF_ERR_UNSUPPORTED, "%s: signal %d: shape out of range", fn, b);
    return fits ? hsc::OK : no_lds();                                               // the others: after them
}

// the device memory of one call, freed (after a stream sync) when the call returns; `fn` names the entry point in the
// ERR_ALLOC message.  Host memory that an asynchronous copy of the call touches is declared before it.
struct DeviceBuffers {
    hscnmf_ctx* ctx;
    const char* fn;
    std::vector<void*> ptrs;
    DeviceBuffers(hscnmf_ctx* c, const char* f) : ctx(c), fn(f) {}
    ~DeviceBuffers()
    {
        (void)hipStreamSynchronize(ctx->stream);
        for (void* q : ptrs) (void)hipFree(q);
    }
    template <typename U> int get(U** out, size_t bytes)
    {
        void* q = nullptr;
        hipError_t e = hipMalloc(&q, std::max<size_t>(bytes, 256));
        if (e != hipSuccess)
            return fail(ctx, HSCNMF_ERR_ALLOC, "%s: hipMalloc of %zu bytes failed (%s)", fn, bytes, hipGetErrorString(e));
        ptrs.push_back(q);
        *out = static_cast<U*>(q);
        return hsc::OK;
    }
};

// the device pointers of a chunk of n signals with a stop flag each: the coefficient pair, x, the residual (the learners'
// R before it), the dictionaries, the residual partials, stat = [3][n] energy, SNR, residual scale and state = [3][n]
// done, iterations, stop
template <typename T>
struct Dev {
    T *A[2], *X, *R, *D;
    double *part, *stat;
    int* state;
};

// where a call's per-signal results go on the host
struct Stats {
    int32_t *iters, *stop;
    double *snr, *rscale;
};

// a host-to-device copy of `bytes`; with spitch, `rows` rows of `bytes` that lie spitch bytes apart on the host
struct Upload {
    void* dst = nullptr;
    const void* src = nullptr;
    size_t bytes = 0, spitch = 0, rows = 0;
};

// between events 0 and 1: the copies (those of no bytes skipped) and the call's stop state (`zeroed` bytes at `state`) zeroed
int upload(hscnmf_ctx* ctx, std::initializer_list<Upload> ups, void* state, size_t zeroed)
{
    hipStream_t st = ctx->stream;
    HSC_TRY(hipEventRecord(ctx->ev[0], st));
    for (const Upload& u : ups) {
        if (!u.bytes) continue;
        if (u.spitch) HSC_TRY(hipMemcpy2DAsync(u.dst, u.bytes, u.src, u.spitch, u.bytes, u.rows, hipMemcpyHostToDevice, st));
        else HSC_TRY(hipMemcpyAsync(u.dst, u.src, u.bytes, hipMemcpyHostToDevice, st));
    }
    HSC_TRY(hipMemsetAsync(state, 0, zeroed, st));
    HSC_TRY(hipEventRecord(ctx->ev[1], st));
    return hsc::OK;
}

// the W steps of iteration `it` over the row tiles; the updated coefficients end in A[((it + 1) * W) & 1]
template <typename T, typename G>
void launch_steps(hipStream_t st, const G& g, dim3 grid, const Plan& pl, T* const* A, const T* X, const T* D, const int* done,
                  int it)
{
    for (int t = 0; t < pl.W; ++t) {
        const int s = it * pl.W + t;
        hipLaunchKernelGGL((nmf_step_kernel<T, G>), grid, dim3(kThreads), pl.lds, st, A[s & 1], A[(s + 1) & 1], X, D, done, g, pl.K,
                           pl.W, pl.F, t, pl.PR, pl.slab);
    }
}

// the residual of iteration `it` over the sample tiles (with the dictionary as it is now), then the n signals' decisions
template <typename T, typename G>
void launch_residual_decide(hipStream_t st, const G& g, dim3 grid, const Plan& pl, const Dev<T>& d, int n, int it,
                            const hscnmf_params& p)
{
    hipLaunchKernelGGL((nmf_residual_kernel<T, G>), grid, dim3(kThreads), pl.lds, st, d.A[((it + 1) * pl.W) & 1], d.X, d.D, d.state,
                       d.R, d.part, g, pl.K, pl.W, pl.F, pl.PR, pl.slab);
    hipLaunchKernelGGL(nmf_decide_kernel<G>, dim3(n), dim3(64), 0, st, d.part, g, d.stat, d.state, d.state + n,
                       d.state + 2 * (size_t)n, d.stat + n, d.stat + 2 * (size_t)n, it + 1, p);
}

// after iteration `it`: 1 when all n flags at `done` are set, else 0 (or a negative status).  The flags are read once per
// iteration, only with a tolerance and another iteration to go.
int all_stopped(hscnmf_ctx* ctx, const hscnmf_params& p, int it, const int* done, int n, std::vector<int>& hdone)
{
    if (!(p.has_residual_scale || p.has_snr) || it + 1 >= p.max_iterations) return 0;
    hdone.resize((size_t)n);
    HSC_TRY(hipMemcpyAsync(hdone.data(), done, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, ctx->stream));
    HSC_TRY(hipStreamSynchronize(ctx->stream));
    return std::all_of(hdone.begin(), hdone.end(), [](int v) { return v != 0; }) ? 1 : 0;
}

// event 2 (the iterations end), then the n signals' iterations, stop reasons, SNR and residual scales to `out` from `first`
template <typename T>
int download_stats(hscnmf_ctx* ctx, const Dev<T>& d, int first, int n, const Stats& out)
{
    hipStream_t st = ctx->stream;
    HSC_TRY(hipEventRecord(ctx->ev[2], st));
    HSC_TRY(hipMemcpyAsync(out.iters + first, d.state + n, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    HSC_TRY(hipMemcpyAsync(out.stop + first, d.state + 2 * (size_t)n, (size_t)n * sizeof(int), hipMemcpyDeviceToHost, st));
    HSC_TRY(hipMemcpyAsync(out.snr + first, d.stat + n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    HSC_TRY(hipMemcpyAsync(out.rscale + first, d.stat + 2 * (size_t)n, (size_t)n * sizeof(double), hipMemcpyDeviceToHost, st));
    return hsc::OK;
}

// the first signal of c0 .. c0 + nb - 1 without a result (its iteration count outside [1, it]), or -1
int no_result(const int32_t* iters, int c0, int nb, int it)
{
    for (int b = c0; b < c0 + nb; ++b)
        if (iters[b] < 1 || iters[b] > it) return b;
    return -1;
}

// once event 3 has completed: a chunk's upload, iteration and download times and the `it` iterations it ran, added to
// tm (timing_ms of include/hscnmf.h)
int add_chunk_times(hscnmf_ctx* ctx, double* tm, int it)
{
    if (int rc = hsc::add_times(ctx, 3, tm)) return rc;
    tm[3] += 1;
    tm[4] += it;
    return hsc::OK;
}

// The chunk size Bc of hscnmf_compute and hscnmf_learn and the chunk's buffers.  Per signal: the A pair, X, R, the stop
// state and (learn) its dsz dictionary values and psz partial values in PD.
template <typename T>
int uniform_alloc(DeviceBuffers& buf, const hscnmf_params& p, const Plan& pl, int B, int Tn, size_t dsz, size_t psz, Dev<T>& d,
                  T** PD, int& Bc)
{
    hscnmf_ctx* ctx = buf.ctx;
    const size_t L = Tn - pl.W + 1, ntt = (Tn + kRows - 1) / kRows, K = pl.K, F = pl.F;
    HSC_TRY(hipSetDevice(ctx->device));
    size_t freeb = 0, totalb = 0;
    HSC_TRY(hipMemGetInfo(&freeb, &totalb));
    const size_t per = (2 * L * K + 2 * (size_t)Tn * F + dsz + psz) * sizeof(T) + ntt * 2 * sizeof(double) + 3 * sizeof(double) +
                       3 * sizeof(int);
    const size_t budget = p.memory_budget ? (size_t)p.memory_budget : freeb / 10 * 6;
    Bc = (int)std::max<size_t>(1, std::min<size_t>({(size_t)B, budget / per, (size_t)65535}));
    const size_t n = Bc;
    if (int rc = buf.get(&d.A[0], n * L * K * sizeof(T))) return rc;
    if (int rc = buf.get(&d.A[1], n * L * K * sizeof(T))) return rc;
    if (int rc = buf.get(&d.X, n * Tn * F * sizeof(T))) return rc;
    if (int rc = buf.get(&d.R, n * Tn * F * sizeof(T))) return rc;
    if (int rc = buf.get(&d.D, (dsz ? n * dsz : K * pl.W * F) * sizeof(T))) return rc;
    if (psz) if (int rc = buf.get(PD, n * psz * sizeof(T))) return rc;
    if (int rc = buf.get(&d.part, n * ntt * 2 * sizeof(double))) return rc;
    if (int rc = buf.get(&d.stat, n * 3 * sizeof(double))) return rc;
    return buf.get(&d.state, n * 3 * sizeof(int));
}

// What hscnmf_compute and hscnmf_compute_ragged share: the host side of the call, the timings summed over its chunks and
// the chunk itself.
template <typename T>
struct Coder {
    hscnmf_ctx* ctx;
    const char* fn;
    const hscnmf_params& p;
    const Plan& pl;
    const T* x;
    const double* energy;
    T *coef, *resid;
    Stats out;
    std::vector<int> hdone;
    double tm[5];

    // One chunk: the signals first .. first + nb - 1 of the call, described by sig[0 .. nb) (T, L, and x0 / a0: the first
    // sample / coefficient row in the chunk's stacks), their samples stacked in x, resid and coef from sample hx0 on.
    // Upload (x, a_init as the caller lays it out, the energies, the caller's tables), per iteration the W steps on
    // `grow`, the residual and the decisions on `gsmp`, the once-per-iteration poll; then the statistics, the residual
    // and every signal's coefficients, centred in its T rows.
    template <typename G>
    int chunk(const G& grow, dim3 rgrid, const G& gsmp, dim3 sgrid, const Dev<T>& d, int first, int nb, const SignalInfo* sig,
              size_t hx0, const Upload& a_init, const Upload& table0 = Upload{}, const Upload& table1 = Upload{})
    {
        const int K = pl.K, W = pl.W, F = pl.F, off = (W - 1) / 2;
        const size_t xbytes = (size_t)(sig[nb - 1].x0 + sig[nb - 1].T) * F * sizeof(T);
        hipStream_t st = ctx->stream;
        if (int rc = upload(ctx, {Upload{d.X, x + hx0 * F, xbytes}, a_init, Upload{d.stat, energy + first, (size_t)nb * sizeof(double)},
                                  table0, table1}, d.state, (size_t)nb * 3 * sizeof(int)))
            return rc;
        int it = 0;
        for (; it < p.max_iterations; ++it) {
            launch_steps(st, grow, rgrid, pl, d.A, d.X, d.D, d.state, it);
            launch_residual_decide(st, gsmp, sgrid, pl, d, nb, it, p);
            HSC_TRY(hipGetLastError());
            const int stopped = all_stopped(ctx, p, it, d.state, nb, hdone);
            if (stopped < 0) return stopped;
            if (stopped) { ++it; break; }
        }
        if (int rc = download_stats(ctx, d, first, nb, out)) return rc;
        HSC_TRY(hipMemcpyAsync(resid + hx0 * F, d.R, xbytes, hipMemcpyDeviceToHost, st));
        HSC_TRY(hipStreamSynchronize(st));
        const int bad = no_result(out.iters, first, nb, it);
        if (bad >= 0) return fail(ctx, HSCNMF_ERR_INVALID, "%s: signal %d has no result", fn, bad);
        for (int b = 0; b < nb; ++b) {
            // a signal that stopped after n iterations holds its coefficients in buffer (n * W) mod 2
            const int n = out.iters[first + b], Tb = sig[b].T, Lb = sig[b].L;
            T* dst = coef + (hx0 + (size_t)sig[b].x0) * K;
            std::memset(dst, 0, (size_t)off * K * sizeof(T));
            std::memset(dst + (size_t)(off + Lb) * K, 0, (size_t)(Tb - off - Lb) * K * sizeof(T));
            HSC_TRY(hipMemcpyAsync(dst + (size_t)off * K, d.A[((size_t)n * W) & 1] + (size_t)sig[b].a0 * K, (size_t)Lb * K * sizeof(T),
                                   hipMemcpyDeviceToHost, st));
        }
        HSC_TRY(hipEventRecord(ctx->ev[3], st));
        HSC_TRY(hipStreamSynchronize(st));
        return add_chunk_times(ctx, tm, it);
    }
};

}  // namespace

// hscnmf_compute: chunks of Bc signals of one length on the uniform geometry, a_init [B][T][K] uploaded as its rows 0 .. L-1
template <typename T>
static int compute_t(hscnmf_ctx* ctx, const Plan& pl, const T* x, int B, int Tn, const T* D, const T* a_init, const double* energy,
                     const hscnmf_params& p, T* coef, T* resid, const Stats& out, double* timing)
{
    const int K = pl.K, W = pl.W, F = pl.F, L = Tn - W + 1, ntl = (L + kRows - 1) / kRows, ntt = (Tn + kRows - 1) / kRows;
    std::vector<SignalInfo> sig;
    Coder<T> c{ctx, "hscnmf_compute", p, pl, x, energy, coef, resid, out, {}, {0, 0, 0, 0, 0}};
    DeviceBuffers buf(ctx, c.fn);
    Dev<T> d;
    int Bc = 0;
    if (int rc = uniform_alloc<T>(buf, p, pl, B, Tn, 0, 0, d, nullptr, Bc)) return rc;
    HSC_TRY(hipMemcpyAsync(d.D, D, (size_t)K * W * F * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    for (int b = 0; b < Bc; ++b) sig.push_back(SignalInfo{(long long)b * Tn, (long long)b * L, 0, 0, Tn, L});
    const Uniform g{L, Tn, 0};
    for (int c0 = 0; c0 < B; c0 += Bc) {
        const int nb = std::min(Bc, B - c0);
        const Upload a{d.A[0], a_init + (size_t)c0 * Tn * K, (size_t)L * K * sizeof(T), (size_t)Tn * K * sizeof(T), (size_t)nb};
        if (int rc = c.chunk(g, dim3(ntl, nb), g, dim3(ntt, nb), d, c0, nb, sig.data(), (size_t)c0 * Tn, a)) return rc;
    }
    if (timing) std::memcpy(timing, c.tm, sizeof(c.tm));
    return HSCNMF_OK;
}

extern "C" int hscnmf_compute(hscnmf_ctx* ctx, int dtype, const void* x, int B, int T, int F, const void* D, int K, int W,
                              const void* a_init, const double* energy, const hscnmf_params* params, void* coefficients,
                              void* residual, int32_t* iterations, int32_t* stop, double* snr, double* residual_scale,
                              double* timing_ms)
{
    const char* fn = "hscnmf_compute";
    if (!ctx) return fail(nullptr, HSCNMF_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!x || !D || !a_init || !energy || !params || !coefficients || !residual || !iterations || !stop || !snr || !residual_scale)
        return fail(ctx, HSCNMF_ERR_INVALID, "%s: NULL argument", fn);
    const int64_t length = T;
    const Stats out{iterations, stop, snr, residual_scale};
    Plan pl;
    if (int rc = check_args(ctx, fn, Call::Coder, dtype, &length, B, F, K, W, params, pl)) return rc;
    if (dtype == HSCNMF_F32)
        return compute_t<float>(ctx, pl, (const float*)x, B, T, (const float*)D, (const float*)a_init, energy, *params,
                                (float*)coefficients, (float*)residual, out, timing_ms);
    return compute_t<double>(ctx, pl, (const double*)x, B, T, (const double*)D, (const double*)a_init, energy, *params,
                             (double*)coefficients, (double*)residual, out, timing_ms);
}

// The learner (hsc/modeling.py:330-417): per chunk of learners, each iteration is the W steps, R = X/|recon| (updated A,
// old D) into the residual buffer, the tile partials, the dictionary update, then the residual and the stop decision with
// the new D.  Every learner owns its D ([B][K][W][F], stride K*W*F); a finished learner's D stays as it was.
template <typename T>
static int learn_t(hscnmf_ctx* ctx, const Plan& pl, const T* x, int B, int Tn, const T* D_init, const T* a_init,
                   const double* energy, const hscnmf_params& p, T* D_out, const Stats& out, double* timing)
{
    const int K = pl.K, W = pl.W, F = pl.F, L = Tn - W + 1, ntl = (L + kRows - 1) / kRows, ntt = (Tn + kRows - 1) / kRows, NW = W * F;
    const size_t dsz = (size_t)K * NW, psz = (size_t)ntl * K * (NW + 1);
    std::vector<int> hdone;
    double tm[5] = {0, 0, 0, 0, 0};
    DeviceBuffers buf(ctx, "hscnmf_learn");
    Dev<T> d;
    T* dPD = nullptr;
    int Bc = 0;
    if (int rc = uniform_alloc(buf, p, pl, B, Tn, dsz, psz, d, &dPD, Bc)) return rc;
    const Uniform g{L, Tn, dsz};
    hipStream_t st = ctx->stream;
    for (int c0 = 0; c0 < B; c0 += Bc) {
        const int nb = std::min(Bc, B - c0);
        const Upload a{d.A[0], a_init + (size_t)c0 * Tn * K, (size_t)L * K * sizeof(T), (size_t)Tn * K * sizeof(T), (size_t)nb};
        if (int rc = upload(ctx, {Upload{d.X, x + (size_t)c0 * Tn * F, (size_t)nb * Tn * F * sizeof(T)}, a,
                                  Upload{d.D, D_init + (size_t)c0 * dsz, (size_t)nb * dsz * sizeof(T)},
                                  Upload{d.stat, energy + c0, (size_t)nb * sizeof(double)}}, d.state, (size_t)nb * 3 * sizeof(int)))
            return rc;
        int it = 0;
        for (; it < p.max_iterations; ++it) {
            launch_steps(st, g, dim3(ntl, nb), pl, d.A, d.X, d.D, d.state, it);
            const T* dAn = d.A[((it + 1) * W) & 1];
            hipLaunchKernelGGL((nmf_ratio_kernel<T, Uniform>), dim3(ntt, nb), dim3(kThreads), pl.lds, st, dAn, d.X, d.D, d.state, d.R, g,
                               K, W, F, pl.PR, pl.slab);
            hipLaunchKernelGGL((nmf_dpart_kernel<T, Uniform>), dim3(ntl, nb), dim3(kThreads), pl.lds_part, st, dAn, d.R, d.state, dPD, g,
                               K, W, F);
            hipLaunchKernelGGL(nmf_dupdate_kernel<T>, dim3(K, nb), dim3(kThreads), pl.lds_upd, st, dPD, ntl, d.state, d.D, K, NW);
            launch_residual_decide(st, g, dim3(ntt, nb), pl, d, nb, it, p);
            HSC_TRY(hipGetLastError());
            const int stopped = all_stopped(ctx, p, it, d.state, nb, hdone);
            if (stopped < 0) return stopped;
            if (stopped) { ++it; break; }
        }
        if (int rc = download_stats(ctx, d, c0, nb, out)) return rc;
        HSC_TRY(hipMemcpyAsync(D_out + (size_t)c0 * dsz, d.D, (size_t)nb * dsz * sizeof(T), hipMemcpyDeviceToHost, st));
        HSC_TRY(hipEventRecord(ctx->ev[3], st));
        HSC_TRY(hipStreamSynchronize(st));
        const int bad = no_result(out.iters, c0, nb, it);
        if (bad >= 0) return fail(ctx, HSCNMF_ERR_INVALID, "hscnmf_learn: learner %d has no result", bad);
        if (int rc = add_chunk_times(ctx, tm, it)) return rc;
    }
    if (timing) std::memcpy(timing, tm, sizeof(tm));
    return HSCNMF_OK;
}

extern "C" int hscnmf_learn(hscnmf_ctx* ctx, int dtype, const void* x, int B, int T, int F, const void* D_init, int K, int W,
                            const void* a_init, const double* energy, const hscnmf_params* params, void* D_out,
                            int32_t* iterations, int32_t* stop, double* snr, double* residual_scale, double* timing_ms)
{
    const char* fn = "hscnmf_learn";
    if (!ctx) return fail(nullptr, HSCNMF_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!x || !D_init || !a_init || !energy || !params || !D_out || !iterations || !stop || !snr || !residual_scale)
        return fail(ctx, HSCNMF_ERR_INVALID, "%s: NULL argument", fn);
    const int64_t length = T;
    const Stats out{iterations, stop, snr, residual_scale};
    Plan pl;
    if (int rc = check_args(ctx, fn, Call::Learner, dtype, &length, B, F, K, W, params, pl)) return rc;
    if (dtype == HSCNMF_F32)
        return learn_t<float>(ctx, pl, (const float*)x, B, T, (const float*)D_init, (const float*)a_init, energy, *params,
                              (float*)D_out, out, timing_ms);
    return learn_t<double>(ctx, pl, (const double*)x, B, T, (const double*)D_init, (const double*)a_init, energy, *params,
                           (double*)D_out, out, timing_ms);
}

// ---- hscnmf_learn_corpus: one dictionary from B signals of different lengths, DESIGN.md section 18 --------------------

// As learn_t with ONE dictionary and the ragged geometry: per iteration the W steps, R = X/|recon|, the tile partials,
// their sums per signal (nmf_dsum_kernel) and over the signals (nmf_dupdate_kernel), the residual with the new D, the
// signals' statistics and the corpus decision.  No synchronisation inside an iteration; the whole corpus is resident.
template <typename T>
static int learn_corpus_t(hscnmf_ctx* ctx, const Plan& pl, const T* x, const int64_t* lengths, int B, const T* D_init,
                          const T* a_init, const double* energy, const hscnmf_params& p, T* D_out, const Stats& out,
                          double* sig_snr, double* sig_rscale, double* timing)
{
    const int K = pl.K, W = pl.W, F = pl.F, NW = W * F, ld = NW + 1;
    const size_t dsz = (size_t)K * NW, tstride = (size_t)K * ld;
    // the per-signal table and the flat tile tables
    std::vector<SignalInfo> sig((size_t)B);
    long long rows = 0, arows = 0, nrt = 0, nst = 0;
    for (int b = 0; b < B; ++b) {
        const long long Tb = lengths[b], Lb = Tb - W + 1;
        sig[b] = SignalInfo{rows, arows, nrt, nst, (int)Tb, (int)Lb};
        rows += Tb;
        arows += Lb;
        nrt += (Lb + kRows - 1) / kRows;
        nst += (Tb + kRows - 1) / kRows;
    }
    const size_t nchunk = (tstride + kThreads - 1) / kThreads;
    if (nst > kMaxCorpusGrid || (long long)B * (long long)nchunk > kMaxCorpusGrid)
        return fail(ctx, HSCNMF_ERR_UNSUPPORTED, "hscnmf_learn_corpus: %lld tiles of %d samples, B * ceil(K * (W * F + 1) / %d) = %lld "
                    "(each at most %lld: a 1-D grid of workgroups of %d threads)", nst, kRows, kThreads,
                    (long long)B * (long long)nchunk, kMaxCorpusGrid, kThreads);
    std::vector<int2> rtiles((size_t)nrt), stiles((size_t)nst);
    for (int b = 0; b < B; ++b) {
        const int nr = (sig[b].L + kRows - 1) / kRows, ns = (sig[b].T + kRows - 1) / kRows;
        for (int i = 0; i < nr; ++i) rtiles[(size_t)sig[b].rt0 + i] = make_int2(b, i);
        for (int i = 0; i < ns; ++i) stiles[(size_t)sig[b].st0 + i] = make_int2(b, i);
    }
    // the bytes of the call, before the first allocation (each buffer rounded up as hipMalloc hands it out)
    const size_t sizes[] = {
        (size_t)arows * K * sizeof(T), (size_t)arows * K * sizeof(T),            // the A pair
        (size_t)rows * F * sizeof(T), (size_t)rows * F * sizeof(T),              // X, R
        dsz * sizeof(T), (size_t)nrt * tstride * sizeof(T), (size_t)B * tstride * sizeof(T),   // D, the tile partials, S
        (size_t)nst * 2 * sizeof(double), (size_t)B * 5 * sizeof(double),        // residual partials; energy, max, sum, snr, scale
        (size_t)B * sizeof(SignalInfo), (size_t)(nrt + nst) * sizeof(int2),      // the tables
        3 * sizeof(int) + 2 * sizeof(double)};                                   // the corpus state
    size_t need = 0;
    for (size_t v : sizes) need += (std::max<size_t>(v, 256) + 255) / 256 * 256;
    HSC_TRY(hipSetDevice(ctx->device));
    size_t freeb = 0, totalb = 0;
    HSC_TRY(hipMemGetInfo(&freeb, &totalb));
    const size_t budget = p.memory_budget ? (size_t)p.memory_budget : freeb / 10 * 6;
    if (need > budget)
        return fail(ctx, HSCNMF_ERR_ALLOC, "hscnmf_learn_corpus: the corpus needs %zu bytes of device memory, the budget is %zu bytes "
                    "(a corpus is resident as a whole: there is no chunking)", need, budget);
    std::vector<int> hdone;
    int hstate[3] = {0, 0, 0};
    double hout[2] = {0.0, 0.0};
    DeviceBuffers buf(ctx, "hscnmf_learn_corpus");
    void* at[std::size(sizes)];
    for (size_t i = 0; i < std::size(sizes); ++i)
        if (int rc = buf.get(&at[i], sizes[i])) return rc;
    T *dA[2] = {(T*)at[0], (T*)at[1]}, *dX = (T*)at[2], *dR = (T*)at[3], *dD = (T*)at[4], *dPD = (T*)at[5], *dS = (T*)at[6];
    double *dPart = (double*)at[7], *dStat = (double*)at[8], *dOut = (double*)at[11];
    SignalInfo* dSig = (SignalInfo*)at[9];
    int2* dTiles = (int2*)at[10];
    int* dState = reinterpret_cast<int*>(dOut + 2);
    double *dEn = dStat, *dMx = dStat + B, *dSs = dStat + 2 * (size_t)B, *dSnr = dStat + 3 * (size_t)B, *dRs = dStat + 4 * (size_t)B;
    using G = Ragged<false>;
    const G grow{dSig, dTiles}, gsmp{dSig, dTiles + nrt};
    const dim3 rgrid((unsigned)nrt), sgrid((unsigned)nst);

    hipStream_t st = ctx->stream;
    if (int rc = upload(ctx, {Upload{dX, x, sizes[2]}, Upload{dA[0], a_init, sizes[0]}, Upload{dD, D_init, sizes[4]},
                              Upload{dEn, energy, (size_t)B * sizeof(double)}, Upload{dSig, sig.data(), sizes[9]},
                              Upload{dTiles, rtiles.data(), (size_t)nrt * sizeof(int2)},
                              Upload{dTiles + nrt, stiles.data(), (size_t)nst * sizeof(int2)}}, dOut, sizes[11]))
        return rc;
    int it = 0;
    for (; it < p.max_iterations; ++it) {
        launch_steps(st, grow, rgrid, pl, dA, dX, dD, dState, it);
        const T* dAn = dA[((it + 1) * W) & 1];
        hipLaunchKernelGGL((nmf_ratio_kernel<T, G>), sgrid, dim3(kThreads), pl.lds, st, dAn, dX, dD, dState, dR, gsmp, K, W, F, pl.PR,
                           pl.slab);
        hipLaunchKernelGGL((nmf_dpart_kernel<T, G>), rgrid, dim3(kThreads), pl.lds_part, st, dAn, dR, dState, dPD, grow, K, W, F);
        hipLaunchKernelGGL(nmf_dsum_kernel<T>, dim3((unsigned)((size_t)B * nchunk)), dim3(kThreads), 0, st, dPD, dSig, dState, dS,
                           (unsigned)nchunk, tstride);
        hipLaunchKernelGGL(nmf_dupdate_kernel<T>, dim3(K, 1), dim3(kThreads), pl.lds_upd, st, dS, B, dState, dD, K, NW);
        hipLaunchKernelGGL((nmf_residual_kernel<T, G>), sgrid, dim3(kThreads), pl.lds, st, dAn, dX, dD, dState, dR, dPart, gsmp, K, W,
                           F, pl.PR, pl.slab);
        hipLaunchKernelGGL(nmf_signal_stats_kernel, dim3(B), dim3(64), 0, st, dPart, dSig, dEn, dState, dMx, dSs, dSnr, dRs);
        hipLaunchKernelGGL(nmf_decide_corpus_kernel, dim3(1), dim3(kThreads), 0, st, dMx, dSs, dEn, B, dState, dOut, it + 1, p);
        HSC_TRY(hipGetLastError());
        const int stopped = all_stopped(ctx, p, it, dState, 1, hdone);
        if (stopped < 0) return stopped;
        if (stopped) { ++it; break; }
    }
    HSC_TRY(hipEventRecord(ctx->ev[2], st));
    HSC_TRY(hipMemcpyAsync(hstate, dState, sizeof(hstate), hipMemcpyDeviceToHost, st));
    HSC_TRY(hipMemcpyAsync(hout, dOut, sizeof(hout), hipMemcpyDeviceToHost, st));
    HSC_TRY(hipMemcpyAsync(sig_snr, dSnr, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
    HSC_TRY(hipMemcpyAsync(sig_rscale, dRs, (size_t)B * sizeof(double), hipMemcpyDeviceToHost, st));
    HSC_TRY(hipMemcpyAsync(D_out, dD, dsz * sizeof(T), hipMemcpyDeviceToHost, st));
    HSC_TRY(hipEventRecord(ctx->ev[3], st));
    HSC_TRY(hipStreamSynchronize(st));
    if (hstate[1] != it) return fail(ctx, HSCNMF_ERR_INVALID, "hscnmf_learn_corpus: the corpus has no result");
    *out.iters = hstate[1];
    *out.stop = hstate[2];
    *out.snr = hout[0];
    *out.rscale = hout[1];
    double tm[5] = {0, 0, 0, 0, 0};
    if (int rc = add_chunk_times(ctx, tm, it)) return rc;
    if (timing) std::memcpy(timing, tm, sizeof(tm));
    return HSCNMF_OK;
}

extern "C" int hscnmf_learn_corpus(hscnmf_ctx* ctx, int dtype, const void* x, const int64_t* lengths, int B, int F,
                                   const void* D_init, int K, int W, const void* a_init, const double* energy,
                                   const hscnmf_params* params, void* D_out, int32_t* iterations, int32_t* stop, double* snr,
                                   double* residual_scale, double* signal_snr, double* signal_residual_scale, double* timing_ms)
{
    const char* fn = "hscnmf_learn_corpus";
    if (!ctx) return fail(nullptr, HSCNMF_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!x || !lengths || !D_init || !a_init || !energy || !params || !D_out || !iterations || !stop || !snr || !residual_scale ||
        !signal_snr || !signal_residual_scale)
        return fail(ctx, HSCNMF_ERR_INVALID, "%s: NULL argument", fn);
    const Stats out{iterations, stop, snr, residual_scale};
    Plan pl;
    if (int rc = check_args(ctx, fn, Call::CorpusLearner, dtype, lengths, B, F, K, W, params, pl)) return rc;
    if (dtype == HSCNMF_F32)
        return learn_corpus_t<float>(ctx, pl, (const float*)x, lengths, B, (const float*)D_init, (const float*)a_init, energy,
                                     *params, (float*)D_out, out, signal_snr, signal_residual_scale, timing_ms);
    return learn_corpus_t<double>(ctx, pl, (const double*)x, lengths, B, (const double*)D_init, (const double*)a_init, energy,
                                  *params, (double*)D_out, out, signal_snr, signal_residual_scale, timing_ms);
}

// ---- hscnmf_compute_ragged: the coder over B signals of different lengths, DESIGN.md section 23 ----------------------

namespace {

// a chunk: the signals first .. first + count - 1, their samples, coefficient rows, row tiles and sample tiles, and the
// device bytes they need
struct RaggedChunk {
    int first, count;
    long long rows, arows, nrt, nst;
    size_t bytes;
};

// The device buffers of a chunk, in the order they lie in the chunk's one allocation: the A pair, X, R, the residual
// partials, (energy, snr, scale), (done, iterations, stop), the signal table, the two tile tables.  Each is rounded up to
// 256 bytes (and is at least that); returns their sum.
constexpr int kRaggedBuffers = 9;
size_t ragged_sizes(size_t item, long long rows, long long arows, long long nrt, long long nst, long long nb, int F, int K,
                    size_t (&s)[kRaggedBuffers])
{
    s[0] = s[1] = (size_t)arows * K * item;
    s[2] = s[3] = (size_t)rows * F * item;
    s[4] = (size_t)nst * 2 * sizeof(double);
    s[5] = (size_t)nb * 3 * sizeof(double);
    s[6] = (size_t)nb * 3 * sizeof(int);
    s[7] = (size_t)nb * sizeof(SignalInfo);
    s[8] = (size_t)(nrt + nst) * sizeof(int2);
    size_t total = 0;
    for (size_t& v : s) {
        v = (std::max<size_t>(v, 256) + 255) / 256 * 256;
        total += v;
    }
    return total;
}

// Consecutive signals into chunks: a chunk takes signals while its bytes stay within `budget`, its sample tiles within
// kMaxCorpusGrid and its signals within kMaxCorpusSignals, and always takes at least one.
void ragged_chunks(size_t item, const int64_t* lengths, int B, int F, int K, int W, size_t budget, std::vector<RaggedChunk>& out)
{
    size_t s[kRaggedBuffers];
    out.clear();
    for (int b = 0; b < B;) {
        RaggedChunk c{b, 0, 0, 0, 0, 0, 0};
        for (; b < B; ++b) {
            const long long Tb = lengths[b], Lb = Tb - W + 1;
            const long long rows = c.rows + Tb, arows = c.arows + Lb;
            const long long nrt = c.nrt + (Lb + kRows - 1) / kRows, nst = c.nst + (Tb + kRows - 1) / kRows;
            const size_t bytes = ragged_sizes(item, rows, arows, nrt, nst, c.count + 1, F, K, s);
            if (c.count > 0 && (bytes > budget || nst > kMaxCorpusGrid || c.count + 1 > kMaxCorpusSignals)) break;
            c = RaggedChunk{c.first, c.count + 1, rows, arows, nrt, nst, bytes};
        }
        out.push_back(c);
    }
}

}  // namespace

extern "C" int hscnmf_ragged_plan(int dtype, const int64_t* lengths, int B, int F, int K, int W, uint64_t budget_bytes,
                                  int32_t* chunk_first, int32_t* n_chunks, uint64_t* max_chunk_bytes)
{
    const char* fn = "hscnmf_ragged_plan";
    if (!n_chunks || !max_chunk_bytes) return fail(nullptr, HSCNMF_ERR_INVALID, "%s: NULL argument", fn);
    Plan pl;
    if (int rc = check_args(nullptr, fn, Call::RaggedCoder, dtype, lengths, B, F, K, W, nullptr, pl)) return rc;
    if (budget_bytes < 1) return fail(nullptr, HSCNMF_ERR_INVALID, "%s: budget_bytes is 0", fn);
    std::vector<RaggedChunk> chunks;
    ragged_chunks(dtype == HSCNMF_F32 ? sizeof(float) : sizeof(double), lengths, B, F, K, W, (size_t)budget_bytes, chunks);
    uint64_t most = 0;
    for (size_t i = 0; i < chunks.size(); ++i) {
        if (chunk_first) chunk_first[i] = chunks[i].first;
        most = std::max<uint64_t>(most, chunks[i].bytes);
    }
    if (chunk_first) chunk_first[chunks.size()] = B;
    *n_chunks = (int32_t)chunks.size();
    *max_chunk_bytes = most;
    return HSCNMF_OK;
}

// hscnmf_compute_ragged: chunks of whole signals (ragged_chunks) on the ragged geometry with a stop flag per signal.  One
// allocation holds the largest chunk; D is uploaded once.  The launches and their order per signal are compute_t's.
template <typename T>
static int compute_ragged_t(hscnmf_ctx* ctx, const Plan& pl, const T* x, const int64_t* lengths, int B, const T* D,
                            const T* a_init, const double* energy, const hscnmf_params& p, T* coef, T* resid, const Stats& out,
                            double* timing)
{
    const int K = pl.K, W = pl.W, F = pl.F;
    HSC_TRY(hipSetDevice(ctx->device));
    size_t freeb = 0, totalb = 0;
    HSC_TRY(hipMemGetInfo(&freeb, &totalb));
    const size_t budget = p.memory_budget ? (size_t)p.memory_budget : std::max<size_t>(freeb / 10 * 6, 1);
    std::vector<RaggedChunk> chunks;
    ragged_chunks(sizeof(T), lengths, B, F, K, W, budget, chunks);
    size_t arena = 0;
    for (const RaggedChunk& c : chunks) arena = std::max(arena, c.bytes);
    std::vector<SignalInfo> sig;
    std::vector<int2> tiles;
    Coder<T> coder{ctx, "hscnmf_compute_ragged", p, pl, x, energy, coef, resid, out, {}, {0, 0, 0, 0, 0}};
    DeviceBuffers buf(ctx, coder.fn);
    unsigned char* base = nullptr;
    T* dD = nullptr;
    if (int rc = buf.get(&base, arena)) return rc;
    if (int rc = buf.get(&dD, (size_t)K * W * F * sizeof(T))) return rc;
    HSC_TRY(hipMemcpyAsync(dD, D, (size_t)K * W * F * sizeof(T), hipMemcpyHostToDevice, ctx->stream));
    long long x0 = 0, a0 = 0;                                        // the chunk's first sample and coefficient row in the stacks
    for (const RaggedChunk& c : chunks) {
        const int nb = c.count;
        size_t s[kRaggedBuffers];
        ragged_sizes(sizeof(T), c.rows, c.arows, c.nrt, c.nst, nb, F, K, s);
        unsigned char* q = base;
        void* at[kRaggedBuffers];
        for (int i = 0; i < kRaggedBuffers; ++i) {
            at[i] = q;
            q += s[i];
        }
        const Dev<T> d{{(T*)at[0], (T*)at[1]}, (T*)at[2], (T*)at[3], dD, (double*)at[4], (double*)at[5], (int*)at[6]};
        SignalInfo* dSig = (SignalInfo*)at[7];
        int2* dTiles = (int2*)at[8];
        // the chunk's tables, with offsets into the chunk's own stacks
        sig.resize((size_t)nb);
        tiles.resize((size_t)(c.nrt + c.nst));
        long long rows = 0, arows = 0, nrt = 0, nst = 0;
        for (int b = 0; b < nb; ++b) {
            const long long Tb = lengths[c.first + b], Lb = Tb - W + 1;
            const long long nr = (Lb + kRows - 1) / kRows, ns = (Tb + kRows - 1) / kRows;
            sig[b] = SignalInfo{rows, arows, nrt, nst, (int)Tb, (int)Lb};
            for (long long i = 0; i < nr; ++i) tiles[(size_t)(nrt + i)] = make_int2(b, (int)i);
            for (long long i = 0; i < ns; ++i) tiles[(size_t)(c.nrt + nst + i)] = make_int2(b, (int)i);
            rows += Tb;
            arows += Lb;
            nrt += nr;
            nst += ns;
        }
        const Ragged<true> grow{dSig, dTiles}, gsmp{dSig, dTiles + c.nrt};
        if (int rc = coder.chunk(grow, dim3((unsigned)c.nrt), gsmp, dim3((unsigned)c.nst), d, c.first, nb, sig.data(), (size_t)x0,
                                 Upload{d.A[0], a_init + (size_t)a0 * K, (size_t)c.arows * K * sizeof(T)},
                                 Upload{dSig, sig.data(), (size_t)nb * sizeof(SignalInfo)},
                                 Upload{dTiles, tiles.data(), tiles.size() * sizeof(int2)}))
            return rc;
        x0 += c.rows;
        a0 += c.arows;
    }
    if (timing) std::memcpy(timing, coder.tm, sizeof(coder.tm));
    return HSCNMF_OK;
}

extern "C" int hscnmf_compute_ragged(hscnmf_ctx* ctx, int dtype, const void* x, const int64_t* lengths, int B, int F,
                                     const void* D, int K, int W, const void* a_init, const double* energy,
                                     const hscnmf_params* params, void* coefficients, void* residual, int32_t* iterations,
                                     int32_t* stop, double* snr, double* residual_scale, double* timing_ms)
{
    const char* fn = "hscnmf_compute_ragged";
    if (!ctx) return fail(nullptr, HSCNMF_ERR_INVALID, "%s: ctx is NULL", fn);
    if (!x || !lengths || !D || !a_init || !energy || !params || !coefficients || !residual || !iterations || !stop || !snr ||
        !residual_scale)
        return fail(ctx, HSCNMF_ERR_INVALID, "%s: NULL argument", fn);
    if (params->max_iterations < 1) return fail(ctx, HSCNMF_ERR_INVALID, "%s: max_iterations = %d", fn, params->max_iterations);
    const Stats out{iterations, stop, snr, residual_scale};
    Plan pl;
    if (int rc = check_args(ctx, fn, Call::RaggedCoder, dtype, lengths, B, F, K, W, nullptr, pl)) return rc;
    if (dtype == HSCNMF_F32)
        return compute_ragged_t<float>(ctx, pl, (const float*)x, lengths, B, (const float*)D, (const float*)a_init, energy,
                                       *params, (float*)coefficients, (float*)residual, out, timing_ms);
    return compute_ragged_t<double>(ctx, pl, (const double*)x, lengths, B, (const double*)D, (const double*)a_init, energy,
                                    *params, (double*)coefficients, (double*)residual, out, timing_ms);
}
