// hscmp_bound.h -- the initial correlation as certified UPPER BOUNDS on the bf16 matrix cores (float32, F == 1).
//
// What the greedy loop needs from the initial correlation is the per-position score max_k |c[t,k] * w_k| of
// DESIGN.md section 2, but only for positions that can win a selection.  This pass writes an upper bound
// ub[t] >= score[t] into best_c and best_k[t] = -1 ("bound, not a score"); the loop computes the exact score
// of such a position the first time it wins a selection (MfmaRecorr::refine).  Outputs
// stay bit-identical: the arg-max over bounds and exact scores, refined until the winner is exact, is the
// arg-max over exact scores with the same tie rule.
//
// The products: every float32 operand v is rounded to bf16, vh = rn(v), and the bound pass of the initial correlation and the
// loop's tile sum ONE product xh dh per tap on v_mfma_f32_32x32x16_bf16: 4 MFMAs of 32 cycles per 32 x 32 tile and atom group at
// W = 64, where the float32 form takes 32 of 64 cycles.  The slack is 2^-7 of ||x_win|| cmax; what the loop pays for it is a
// refine of a position that outranks the exact winner by less than the slack, and a winner that more often holds its exact score
// from an earlier selection's refine (the cache of committed refines keeps that refine's (k, c) for it), both measured in
// DESIGN.md section 11.
//
// ---- derivation of the error constant kBoundEps1 ------------------------------------------------------------------
// u = 2^-8 (bf16 round to nearest), u' = 2^-23 (one accumulation step of the matrix core, ANY order and ANY rounding
// direction), u'' = 2^-24 (float32 round to nearest), n = 16 * SB <= 64 products per output, W <= 16 * SB <= 64 taps.
// For x (signal) and d (atom): |x - xh| <= u|x|, |xh| <= (1+u)|x|, and the same for d.  The tile sees xh and dh only.
// (1) dropped terms: x d - xh dh = xh (d - dh) + (x - xh) d, so per tap
//       |dropped| <= u ((1+u) + 1) |x||d| = u (2 + u) |x||d| = 7.82776e-3 |x||d|.
// (2) the matrix core: each bf16 product is exact in float32 (8 x 8 significant bits; the input ranges below keep every
//       product normal), the sum of n products with relative error <= u' per step in any order is off by at most
//       gamma_n(u') sum|products| (gamma_64 = 64 u' / (1 - 64 u') = 7.6295e-6), and
//       sum|xh dh| <= (1+u)^2 |x||d| = 1.007828 |x||d|  ->  7.6892e-6 |x||d|.
//     A partial sum that cancels below 2^-126 may be flushed to zero: at most n 2^-126 |w_k| < 2^-88 absolute,
//     covered by kBoundAbs.
// (3) the score is NOT the exact real sum but the pinned float32 fmaf chain over the W taps:
//       |chain - sum| <= gamma_W(u'') sum|x||d| <= 64 2^-24 / (1 - 64 2^-24) = 3.8147e-6 per |x||d|.
//   Together, per atom:  |chain_k - acc_k| <= eps_1 sum_w |x_w||d_kw| <= eps_1 ||x_win||_2 ||d_k||_2   (Cauchy-Schwarz)
//       eps_1 = 7.82776e-3 + 7.6892e-6 + 3.8147e-6 = 7.83926e-3  (= 2^-6.995).
// (4) the bound's own arithmetic.  score_k = rn(|chain_k w_k|) <= (1+u'')|chain_k||w_k|, and the tile's
//     v_k = rn(acc_k w_k) >= (1-u'')|acc_k w_k|, so
//       score <= (1+u'')/(1-u'') max_k v_k + (1+u'') eps_1 ||x_win|| max_k ||d_k|| |w_k|.
//     The tile forms ub = fmaf(M, 1 + 2^-20, rn(rn(kBoundEps1 * rn(sqrt(ss))) * cmax) + 2^-80), with M = max_k v_k,
//     cmax >= max_k ||d_k|| |w_k| rounded up on the host, and ss the float32 sum of xh^2 over the 16 SB taps of the window:
//     |x| <= |xh| / (1-u) tap by tap, so ||x_win|| <= ||xh_win|| / (1-u) and
//       score <= (1+u'')/(1-u'') max_k v_k + (1+u'') eps_1 / (1-u) ||xh_win|| cmax,   (1+u'') eps_1 / (1-u) = 7.87001e-3.
//     kBoundEps1 = 2^-7 (1 + 2^-6) = 7.93457e-3 is 1.0082 times that.  The margin of 0.82 % is there for the roundings of
//     rn(rn(kBoundEps1 * rn(sqrt(ss))) * cmax) + 2^-80 and of ss itself (at most 64 fmaf, a sqrt good to 2 ulp, three more
//     roundings: together below a factor 1 - 2^-17 = 1 - 0.0008 %), a thousand times over; it is not needed for anything
//     else, and the constant is not tuned on data (tests/test_bound_one_product.py puts it against the pinned chain).
//     M's factor 1 + 2^-20 after the final rounding still exceeds (1+u'')/(1-u'') = 1 + 2^-23.
//     xh = 0 only where x = 0 (|x| >= 2^-60 in the model), so ss == 0 still means an all-zero window: an exact 0.
//
// Inputs outside the model run the exact float32 tile (same kernel, same result as corr_init_mfma_kernel):
//   a chunk (with its halo) that holds a sample that is not finite, or a non-zero |x| outside [2^-60, 2^60];
//   a dictionary (or weights) with a non-zero magnitude outside [2^-30, 2^30] does not get a bf16 image at all
//   (hscmp_set_dictionary), and the encode runs corr_init_mfma_kernel.
// tools/bf16_bound_probe.hip checks assumption (2) on the hardware (profiles/r05_bf16_probe.txt).
//
// The four-signal loop (MfmaRecorr with BOUND) re-correlates the rows around an applied atom with the same tile
// (bound_tile<SB, HAS_W>, hscmp_mfma.h) over its reflect-padded window: the derivation above holds unchanged whenever
// every sample the tile reads is inside the model, and a tile whose window holds one outside it (a wave-wide vote, every
// atom) runs the exact float32 tile on the loop's float32 image (mfma_tile_score_small).  Split, epilogue and constants have one definition.
// The assumptions of the derivation, one by one, for the loop's caller:
//   * n <= 64 products per output, W <= 64 taps: the tile runs SB <= 4 k-steps of 16 taps; past W the image holds zeros, whose
//     products are exact zeros, and the window norm over 16 SB >= W samples is only larger than the one the derivation needs.
//   * xh = rn(x) of the very samples the pinned chain reads: window_split rounds the float32 value it writes to the window
//     (the reflected copy near a signal end included, one rounding, bf16_rn_bits), and the refine reads that window again through
//     edge_window_value -- the invariant that makes the refined score the row's score (MfmaRecorr::refine) whatever the tile.
//   * dh = rn(d) of the float32 tap the chain uses: Bimg is rn(d) of the dictionary the float32 image holds, element by
//     element (bound_build_dict_image, mfma_build_dict_image), so tile and chain speak of the same d.
//   * every product normal, no sample outside [2^-60, 2^60] or not finite: the vote in front of the tile, over every sample
//     the tile reads (taps past W included); dictionary and weights were checked on the host (bound_build_dict_image).
//   * xh = 0 only where x = 0: by the same vote, so the ss == 0 return is an exact 0 and the rule "sc == 0 -> hint 0" stands.
//   * cmax: the one A.cmax of bound_build_dict_image, as in the bound pass.
// Nothing in (1)-(4) depends on the padding rule or on who calls the tile, and kBoundEps1 is the slack here too.
#pragma once

#include "hscmp_mfma.h"

#include <cmath>
#include <cstring>

namespace hscmp {

// k-steps of 16 taps for the filter width (the bound pass is built for SB = 1, 2, 4: the float32 chunk counts 2, 4, 8)
inline int bound_steps(int W) { return (W + 15) / 16; }

// host: the bf16 image Bimg[g][s][lane][8], every entry rounded to nearest even: element j of lane l in (group g,
// k-step s) is D[32g + (l&31)][16s + 8(l>>5) + j] -- the A-operand map of v_mfma_f32_32x32x16_bf16; zero padded.  Also
// cmax >= max_k ||d_k|| |w_k| (rounded up).  Returns false when the dictionary or the weights lie outside the model.
inline bool bound_build_dict_image(const float* D, const float* wts, int K, int W, std::vector<unsigned short>& out, float& cmax)
{
    const int G = mfma_groups(K), SB = bound_steps(W);
    out.assign((size_t)G * SB * 64 * 8, 0);
    double cm = 0.0;
    auto in_model = [](double a) { return std::isfinite(a) && (a == 0.0 || (std::fabs(a) >= kBoundDMin && std::fabs(a) <= kBoundDMax)); };
    for (int k = 0; k < K; ++k) {
        double n2 = 0.0;
        for (int w = 0; w < W; ++w) {
            const double v = D[(size_t)k * W + w];
            if (!in_model(v)) return false;
            n2 += v * v;
        }
        const double wk = wts ? (double)wts[k] : 1.0;
        if (!in_model(wk)) return false;
        cm = std::max(cm, std::sqrt(n2) * std::fabs(wk));
    }
    for (int g = 0; g < G; ++g)
        for (int s = 0; s < SB; ++s)
            for (int lane = 0; lane < 64; ++lane)
                for (int j = 0; j < 8; ++j) {
                    const int k = 32 * g + (lane & 31), w = 16 * s + 8 * (lane >> 5) + j;
                    if (k >= K || w >= W) continue;
                    const float v = D[(size_t)k * W + w];
                    unsigned short hi, lo;
                    bf16_split(v, hi, lo);
                    out[(((size_t)g * SB + s) * 64 + lane) * 8 + j] = hi;
                }
    cm *= 1.0 + 0x1p-30;                                        // (the double sum and sqrt: relative error < 2^-45)
    float f = (float)cm;
    if ((double)f < cm) f = std::nextafter(f, INFINITY);
    cmax = f;
    return true;
}


// ------------------------------------------------------------------------------------------------
// The bound pass: the persistent grid of corr_init_mfma_kernel over (signal, 2048-position chunk) items, the tile of
// bound_tile<SB, HAS_W>.
// LDS: [bf16 image (Bimg)][weights 32*G][chunk: every sample rounded to bf16, or the float32 chunk of a chunk
// outside the model].
// A chunk outside the model (see the header) runs mfma_tile_score on the float32 image in global
// memory (L2-resident): the exact score and group hint, bit for bit what corr_init_mfma_kernel writes.
// A position whose bound came out as an exact 0 (all-zero window) gets the hint 0 like the exact tile: it is exact.
// ------------------------------------------------------------------------------------------------
template <int SB> __host__ __device__ constexpr int bound_chunk_samples() { return kMfmaChunk + 16 * SB + 32; }

template <int SB, bool HAS_W>
__global__ __launch_bounds__(kThreads) void corr_bound_kernel(DevParams P, State<float> S, MfmaArgs A,
                                                              const unsigned short* __restrict__ bimg, float cmax)
{
    constexpr int S4C = 2 * SB;
    constexpr int nx = bound_chunk_samples<SB>();       // chunk + 16 SB taps + the last tile's lane offset (even)
    static_assert(nx <= kMfmaChunkLoads * kThreads, "staging registers");
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int G = A.G;
    const int nimg = G * SB * 64;                       // 16-byte fragments of the image
    bf16x8* bh = reinterpret_cast<bf16x8*>(smem);
    float* wts = reinterpret_cast<float*>(bh + nimg);
    char* xbuf = reinterpret_cast<char*>(wts + 32 * G);
    unsigned short* xh = reinterpret_cast<unsigned short*>(xbuf);
    float* xs = reinterpret_cast<float*>(xbuf);         // (same bytes: a chunk is staged in one form or the other)
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int T = P.T;
    const int cps = (T + kMfmaChunk - 1) / kMfmaChunk;
    const int nitems = cps * P.B;

    lds_copy16(bh, bimg, nimg * 16);
    if (HAS_W) for (int i = tid; i < 32 * G; i += kThreads) wts[i] = i < P.K ? S.weights[i] : 0.0f;

    float xr[kMfmaChunkLoads];
    auto fetch = [&](int item) {                        // zero padding of 'same' (:159-164), as corr_init_mfma_kernel
        const int b = item / cps, c0 = (item % cps) * kMfmaChunk;
        const float* x = S.residual + (int64_t)b * T;
#pragma unroll
        for (int u = 0; u < kMfmaChunkLoads; ++u) {
            const int i = u * kThreads + tid;
            const int g = c0 - P.off + i;
            xr[u] = (i < nx && g >= 0 && g < T) ? x[g] : 0.0f;
        }
    };

    int item = blockIdx.x;
    if (item < nitems) fetch(item);
    for (; item < nitems; item += gridDim.x) {
        bool out = false;
#pragma unroll
        for (int u = 0; u < kMfmaChunkLoads; ++u) out |= bound_sample_out(xr[u]);
        const bool exact = __syncthreads_or(out) != 0;  // (also: every tile of the previous chunk has read the buffer)
#pragma unroll
        for (int u = 0; u < kMfmaChunkLoads; ++u) {
            const int i = u * kThreads + tid;
            if (i < nx) {
                if (exact) xs[i] = xr[u];
                else xh[i] = (unsigned short)(bf16_rn_bits(__float_as_uint(xr[u])) >> 16);
            }
        }
        __syncthreads();
        const int next = item + gridDim.x;
        if (next < nitems) fetch(next);                 // in flight while this chunk is computed
        const int b = item / cps, c0 = (item % cps) * kMfmaChunk;
        const int Tb = signal_length(P, S, b);          // (ragged batches: rows from Tb on are dead and not computed)
        const int npos = min(kMfmaChunk, Tb - c0);
        const int ntiles = (npos + 31) / 32;
        for (int q = wv; q < ntiles; q += kWaves) {
            float sc;
            int grp;
            if (exact) sc = mfma_tile_score<S4C, HAS_W>(A.dimg, xs + 32 * q, wts, G, S4C, lane, grp);
            else {
                sc = bound_tile<SB, HAS_W>(bh, xh + 32 * q, wts, G, lane, cmax);
                grp = sc == 0.0f ? 0 : -1;              // an exact 0 is a score (hint 0, as the exact tile); else a bound
            }
            const int t = c0 + 32 * q + lane;
            if (lane < 32 && t < Tb) {
                S.best_c[(int64_t)b * T + t] = sc;
                S.best_k[(int64_t)b * T + t] = grp;
            }
        }
    }
}

// LDS bytes of the bound pass: the image, the weights, the chunk as float32 (the exact tile's form, the larger one)
inline size_t bound_lds_bytes(int G, int SB)
{
    return (size_t)G * SB * 1024 + (size_t)32 * G * 4 + (size_t)(kMfmaChunk + 16 * SB + 32) * 4;
}

template <int SB, bool HAS_W>
static int bound_launch_t(hipStream_t stream, const DevParams& P, const State<float>& S, const MfmaArgs& A,
                          const unsigned short* bimg, float cmax, bool dry)
{
    const size_t lds = bound_lds_bytes(A.G, SB);
    auto kern = corr_bound_kernel<SB, HAS_W>;
    const int64_t nitems = (int64_t)((P.T + kMfmaChunk - 1) / kMfmaChunk) * P.B;
    return launch_tile_kernel(kern, persistent_grid((const void*)kern, lds, nitems, dry), dim3(kThreads), lds, kLdsDevice, 0, dry, stream, P, S, A,
                              bimg, cmax);
}

// The bound pass for this shape, or -1 when it does not cover it (the caller then runs the exact corr_init):
// the float32 chunk counts 2, 4, 8 of the compile-time MFMA kernels (W in 9..16, 25..32, 57..64).
inline int bound_launch_corr_init(hipStream_t stream, const DevParams& P, const State<float>& S, const float* dimg,
                                  const unsigned short* bimg, float cmax, bool dry = false)
{
    const MfmaArgs A = mfma_args<float>(P, S, dimg);
    return dispatch_chunks<false>(A.S4, A.has_w != 0, [&](auto s4c, auto hw) {
        return bound_launch_t<decltype(s4c)::value / 2, decltype(hw)::value>(stream, P, S, A, bimg, cmax, dry);
    });
}

}  // namespace hscmp
