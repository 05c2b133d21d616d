// hscmp_wide.h -- the wide loop: ONE signal's blocked round spread over the whole chip.
//
// iterate_rp_kernel (hscmp_rp.h) runs a blocked round as phases over all its atoms, but inside one 1024-thread workgroup: a
// signal of 10^5 .. 10^7 samples with nbBlocks='auto' has hundreds to thousands of atoms per round (more than that kernel's
// 512 candidates) and one CU of 256 at work.  Here the same phases run as plain kernel launches in stream order:
//   candidates   grid over blocks x signals   P1: block arg-max, (k, c), local energies, slot-chain lookup -> global arrays
//   control      one workgroup per signal     P2 filters + |c| order, the group walk, P3 prefix, P6 round bookkeeping;
//                                             atoms at a signal end and rounds without spacing are applied here, alone
//   subtract     grid over the apply list     P4: one wave per atom
//   recorrelate  grid over (atom, 32 rows)    P5: the matrix-core tile from the final residual
// A workgroup never waits for another one: what one launch leaves in global memory the next launch reads (a dependent kernel
// boundary is 1.5 .. 1.9 us; a grid barrier would strand a workgroup whenever the grid is not resident).  Every kernel reads
// the signal's control block and returns at once when the signal has no work for it, so the host queues a fixed sequence of
// launches a few times, then reads the control blocks (wide_loop in hscmp_api.hip).
// The per-atom pieces are RpMfma's, the prefix is rp_wave_prefix, the groups are those of iterate_rp_kernel: the state the
// loop leaves is that loop's, bit for bit (tests/test_gpu_wide.py).
#pragma once

#include "hscmp_rp.h"

#include <algorithm>

namespace hscmp {

constexpr int kWideMaxSel = 16384;       // candidates of a round the control workgroup sorts in LDS (8 bytes each, padded to 2^n)

// control block of a signal, in global memory between the launches
enum { WC_DONE = 0,      // nothing more to do in this call: the signal has stopped, or ran its max_rounds
       WC_MID = 1,       // inside a round (0: at a round start -- the candidates kernel has work)
       WC_POS = 2,       // first atom of ord[] that has not been applied
       WC_N = 3, WC_SPACED = 4, WC_NEDGE = 5,      // the round: atoms, pairwise >= W apart, atoms at a signal end
       WC_ALO = 6, WC_AHI = 7,                     // ord[ALO, AHI): the group the grid applies in this step
       WC_ROUNDS_RUN = 8,                          // rounds of this call (max_rounds)
       WC_STEPS = 9,                               // control launches that found work (diagnostics)
       WC_COUNT = 16 };

// per-signal arrays of the round in global memory: RpShared's candidate fields, the filter lists and the order
struct WideView {
    int* ctl;
    double* c_acc;
    int* c_t; int* c_k; int* c_found; int* c_flag; int* c_head;
    float* c_c; float* c_eb; float* c_ea;
    int* ord; int* la; int* lb;
};
constexpr size_t kWideBytesPerCand = sizeof(double) + 11 * sizeof(int);
inline __host__ __device__ size_t wide_scratch_bytes(int B, int maxsel)
{
    return (size_t)B * (WC_COUNT * sizeof(int) + (size_t)maxsel * kWideBytesPerCand);
}
__device__ __forceinline__ WideView wide_view(char* buf, int B, int maxsel, int b)
{
    WideView V;
    V.ctl = reinterpret_cast<int*>(buf) + (size_t)b * WC_COUNT;             // the control blocks first, contiguous: one copy reads them
    char* p = buf + (size_t)B * WC_COUNT * sizeof(int) + (size_t)b * maxsel * kWideBytesPerCand;
    V.c_acc = reinterpret_cast<double*>(p);
    int* q = reinterpret_cast<int*>(V.c_acc + maxsel);
    V.c_t = q; V.c_k = q + maxsel; V.c_found = q + 2 * (size_t)maxsel; V.c_flag = q + 3 * (size_t)maxsel; V.c_head = q + 4 * (size_t)maxsel;
    V.c_c = reinterpret_cast<float*>(q + 5 * (size_t)maxsel); V.c_eb = V.c_c + maxsel; V.c_ea = V.c_c + 2 * (size_t)maxsel;
    V.ord = q + 8 * (size_t)maxsel; V.la = q + 9 * (size_t)maxsel; V.lb = q + 10 * (size_t)maxsel;
    return V;
}

// what rp_wave_prefix and rp_compact go by (RpShared), the candidate fields as views of the global arrays
struct WideShared {
    int* c_t; int* c_k; float* c_c; float* c_eb; float* c_ea; int* c_found; double* c_acc; int* c_flag; int* c_head; int* ord;
    int wtot[kRpWaves];
    int converged, stop, napply, gend;
    int n, spaced, nedge, full;
    int nnz, ndup, rounds, iters, nev, nslots, offset;
    float e_sig, e_res;
};

template <typename R> __device__ __forceinline__ Sig<R> wide_sig(const DevParams& P, const State<R>& S, int b)
{
    Sig<R> G;
    G.r = S.residual + (int64_t)b * P.T * P.F;
    G.bc = S.best_c + (int64_t)b * P.T;
    G.bk = S.best_k + (int64_t)b * P.T;
    G.ev_t = S.ev_t + (int64_t)b * P.cap; G.ev_k = S.ev_k + (int64_t)b * P.cap; G.ev_c = S.ev_c + (int64_t)b * P.cap;
    G.slot_t = S.slot_t + (int64_t)b * P.cap; G.slot_k = S.slot_k + (int64_t)b * P.cap; G.slot_a = S.slot_a + (int64_t)b * P.cap;
    G.hkey = S.hkey + (int64_t)b * ((int64_t)P.hmask + 1); G.hval = S.hval + (int64_t)b * ((int64_t)P.hmask + 1);
    G.head = S.head + (int64_t)b * P.T;
    G.sel_t = nullptr; G.sel_k = nullptr; G.sel_c = nullptr;
    G.lgram = nullptr;
    return G;
}

// pow2 >= n (at least 64): entries of the control workgroup's sort
inline __host__ __device__ int wide_sort_entries(int n)
{
    int m = 64;
    while (m < n) m <<= 1;
    return m;
}

// ---- start of a call (hscmp_encode_batch*, hscmp_continue): the slot chains from the slot list (head[] is -1 everywhere), the control block.
//      grid = B, block = kRpThreads
template <typename R> __global__ __launch_bounds__(kRpThreads) void wide_begin_kernel(DevParams P, State<R> S, char* wbuf)
{
    const int b = blockIdx.x, tid = threadIdx.x;
    const WideView V = wide_view(wbuf, P.B, P.maxsel, b);
    const int* stats = S.stats + (int64_t)b * ST_COUNT;
    const Sig<R> G = wide_sig(P, S, b);
    const int ns = stats[ST_SLOTS];
    for (int i = tid; i < ns; i += kRpThreads)
        hval_store(G.hval + i, __hip_atomic_exchange(G.head + G.slot_t[i], i, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT));
    if (tid < WC_COUNT) V.ctl[tid] = (tid == WC_DONE && stats[ST_STOP] != STOP_RUNNING) ? 1 : 0;
}

// ---- P1: the candidates of a round.  grid = (workgroups, B), block = kRpThreads.  Blocks of up to 256 positions: one wave per
//      block; longer ones: the workgroup scans one block, a slice per wave, and wave 0 takes the best of the slices (same tie rule:
//      the larger score, then the lower position).
template <typename Pol>
__global__ __launch_bounds__(kRpThreads) void wide_candidates_kernel(DevParams P, State<float> S, typename Pol::Args A, char* wbuf)
{
    using R = float;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.y;
    const WideView V = wide_view(wbuf, P.B, P.maxsel, b);
    if (V.ctl[WC_DONE] || V.ctl[WC_MID]) return;                   // (uniform)
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const int T = P.T;
    const int off = S.stats[(int64_t)b * ST_COUNT + ST_OFFSET];
    const int nb = P.nbk + (off ? 1 : 0);
    const int pad0 = off ? P.bs / 2 : 0;
    const bool per_wave = P.bs <= 256;
    const int first = per_wave ? blockIdx.x * kRpWaves : blockIdx.x;
    if (first >= nb) return;                                       // (uniform; before anything is staged)
    __shared__ float part_s[kRpWaves];
    __shared__ int part_i[kRpWaves];
    const Sig<R> G = wide_sig(P, S, b);
    Pol::prologue(P, S, G, A, smem, b);                            // (ends with a workgroup barrier)
    const R* wts = Pol::weights(P, S, A, smem);
    const int stride = per_wave ? gridDim.x * kRpWaves : gridDim.x;
    for (int j0 = first; j0 < nb; j0 += stride) {                  // (uniform)
        const int j = per_wave ? j0 + wv : j0;
        const int w0 = j * P.bs - pad0;
        const int lo = w0 < 0 ? 0 : w0;
        const int hi = min(T, w0 + P.bs);
        Cand<R> win; win.s = (R)-1; win.i = INT_MAX;
        if (per_wave) {
            if (j < nb && lo < hi) win = rp_range_argmax4<true>(G, wts, lo, hi, lane);
        } else {
            const int len = hi - lo, per = (len + kRpWaves - 1) / kRpWaves;
            const int s0 = min(hi, lo + wv * per), s1 = min(hi, s0 + per);
            if (s0 < s1) win = wave_range_argmax<true>(G, wts, s0, s1, lane);
            __syncthreads();                                       // (the previous block's partial results have been read)
            if (lane == 0) { part_s[wv] = win.s; part_i[wv] = win.i; }
            __syncthreads();
            win.s = (R)-1; win.i = INT_MAX;
            for (int q = 0; q < kRpWaves; ++q) {                   // slices in ascending position
                Cand<R> o; o.s = part_s[q]; o.i = part_i[q];
                if (better(o, win)) win = o;
            }
        }
        if (j >= nb || (!per_wave && wv != 0)) continue;           // (wave-uniform)
        bool valid = (lo < hi) && win.i != INT_MAX;                // :940-942 range test
        if (valid && win.s == (R)0 && w0 < 0) valid = false;       // arg-max on a leading padded row
        int wk = 0, flag = 0, found = -1, head = -1;
        R wc = (R)0, eb = (R)0, ea = (R)0;
        double acc = 0.0;
        if (valid) {                                               // wave-uniform
            head = hval_load(G.head + win.i);
            Pol::candidate(P, S, G, A, smem, win.i, lane, wv, wk, wc, eb, ea, flag);
            found = head;
            while (found >= 0 && G.slot_k[found] != wk) found = hval_load(G.hval + found);      // (uniform)
            if (found >= 0) acc = G.slot_a[found];
        }
        if (lane == 0) {
            V.c_t[j] = valid ? win.i : -1; V.c_k[j] = wk; V.c_c[j] = wc; V.c_eb[j] = eb; V.c_ea[j] = ea;
            V.c_found[j] = found; V.c_acc[j] = acc; V.c_flag[j] = flag; V.c_head[j] = head;
        }
    }
}

// stable compaction of the indices [0, count) over the workgroup, 1024 at a time (rp_compact): dst gets value(i) of every kept i
template <typename KeepF, typename ValF>
__device__ __forceinline__ int wide_compact(WideShared& sh, int count, int* dst, KeepF keep, ValF value)
{
    int total = 0;
    for (int base = 0; base < count; base += kRpThreads) {         // (uniform)
        const int i = base + (int)threadIdx.x;
        const bool k = i < count && keep(i);
        total += rp_compact(sh, k, k ? value(i) : 0, dst + total);
    }
    return total;
}

// ---- P2 over the candidate arrays (rp_block_select for any number of blocks): index lists in global memory, the |c| order by
//      a bitonic sort of (|c| bits, list index + 1) words in LDS -- descending, the later entry first among equals (:960-962)
__device__ __forceinline__ void wide_select(const DevParams& P, WideShared& sh, const WideView& V, unsigned long long* keys, int nb)
{
    const int tid = threadIdx.x, T = P.T, W = P.W, F = P.F;
    const bool has_thres = P.has_thres != 0;
    const double thres = P.thres;
    int* la = V.la; int* lb = V.lb;
    bool spaced = true;
    // :946-948 drop null coefficients (and invalid blocks)
    int n = wide_compact(sh, nb, la, [&](int i) { return V.c_t[i] >= 0 && (!has_thres || fabs((double)V.c_c[i]) > thres); }, [&](int i) { return i; });
    // :951-957 interference filter vs the unfiltered predecessor; skipped when no gap qualifies
    if (n > 1) {
        auto gap = [&](int i) { return i >= 1 && (V.c_t[la[i]] - V.c_t[la[i - 1]] >= W); };
        int any = 0;
        for (int i = tid; i < n; i += kRpThreads) any |= gap(i) ? 1 : 0;
        if (__syncthreads_or(any)) {
            n = wide_compact(sh, n, lb, [&](int i) { return i == 0 || gap(i); }, [&](int i) { return la[i]; });
            int* tmp = la; la = lb; lb = tmp;
        } else {
            spaced = false;
        }
    }
    // :960-962 argsort(|c|)[::-1]
    const int m = wide_sort_entries(n);
    for (int i = tid; i < m; i += kRpThreads)
        keys[i] = i < n ? ((unsigned long long)__float_as_uint(fabsf(V.c_c[la[i]])) << 32) | (unsigned)(i + 1) : 0ull;
    __syncthreads();
    for (int k = 2; k <= m; k <<= 1)
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int p = tid; p < (m >> 1); p += kRpThreads) {
                const int i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), x = i | j;
                const unsigned long long a = keys[i], c = keys[x];
                const bool desc = (i & k) == 0;
                if (desc ? a < c : a > c) { keys[i] = c; keys[x] = a; }
            }
            __syncthreads();
        }
    for (int i = tid; i < n; i += kRpThreads) lb[i] = la[(int)(unsigned)keys[i] - 1];
    __syncthreads();
    { int* tmp = la; la = lb; lb = tmp; }
    // :1090-1099 weak-atom filter: the window of the filter is the atom's clipped support, its energy c_eb
    if (P.has_snr && n > 1) {
        const float tol_energy = sh.e_sig / (float)P.snr_ratio;
        const double thr = (double)tol_energy / (double)((int64_t)T * F);
        n = wide_compact(sh, n, lb, [&](int i) {
                const int me = la[i];
                int s, e, es;
                const int len = centered_span(T, W, V.c_t[me], s, e, es);
                const float mean = V.c_eb[me] / (float)((int64_t)len * F);
                return (double)mean >= thr;
            }, [&](int i) { return la[i]; });
        int* tmp = la; la = lb; lb = tmp;
    }
    if (tid == 0) sh.nedge = 0;
    __syncthreads();
    int edge = 0;
    for (int i = tid; i < n; i += kRpThreads) {
        const int me = la[i];
        V.ord[i] = me;
        edge += (V.c_flag[me] & RPF_INTERIOR) ? 0 : 1;
    }
    if (edge) atomicAdd(&sh.nedge, edge);
    if (tid == 0) { sh.n = n; sh.spaced = spaced ? 1 : 0; }
    __syncthreads();
}

// ---- control: P2 at a round start, then the groups of the round as iterate_rp_kernel forms them, until one goes to the grid
//      or the round ends.  grid = B, block = kRpThreads.  LDS: [WideShared][sort keys][policy LDS]
template <typename Pol>
__global__ __launch_bounds__(kRpThreads) void wide_control_kernel(DevParams P, State<float> S, typename Pol::Args A, char* wbuf, int key_entries)
{
    using R = float;
    extern __shared__ __attribute__((aligned(16))) char smem[];
    WideShared& sh = *reinterpret_cast<WideShared*>(smem);
    unsigned long long* keys = reinterpret_cast<unsigned long long*>(smem + ((sizeof(WideShared) + 15) / 16) * 16);
    char* plds = reinterpret_cast<char*>(keys + key_entries);
    const int b = blockIdx.x;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const WideView V = wide_view(wbuf, P.B, P.maxsel, b);
    int* stats = S.stats + (int64_t)b * ST_COUNT;
    if (V.ctl[WC_DONE]) {                                           // (uniform) nothing of this signal is applied again
        if (tid == 0) { V.ctl[WC_ALO] = 0; V.ctl[WC_AHI] = 0; }
        return;
    }
    const Sig<R> G = wide_sig(P, S, b);
    const bool mid = V.ctl[WC_MID] != 0;
    if (tid == 0) {
        sh.c_t = V.c_t; sh.c_k = V.c_k; sh.c_c = V.c_c; sh.c_eb = V.c_eb; sh.c_ea = V.c_ea; sh.c_found = V.c_found; sh.c_acc = V.c_acc;
        sh.c_flag = V.c_flag; sh.c_head = V.c_head; sh.ord = V.ord;
        sh.nnz = stats[ST_NNZ]; sh.ndup = stats[ST_DUP]; sh.rounds = stats[ST_ROUNDS]; sh.iters = stats[ST_ITERS];
        sh.nev = stats[ST_EVENTS]; sh.nslots = stats[ST_SLOTS]; sh.offset = stats[ST_OFFSET];
        sh.converged = 0; sh.stop = STOP_RUNNING; sh.napply = 0; sh.gend = 0; sh.full = 0;
        sh.n = V.ctl[WC_N]; sh.spaced = V.ctl[WC_SPACED]; sh.nedge = V.ctl[WC_NEDGE];
        sh.e_sig = S.energy[2 * b + 0]; sh.e_res = S.energy[2 * b + 1];
    }
    __syncthreads();
    int pos = mid ? V.ctl[WC_POS] : 0;
    if (!mid) {
        wide_select(P, sh, V, keys, P.nbk + (sh.offset ? 1 : 0));   // (ends with a barrier)
        // A round whose atoms do not all fit the event list is not started: the state then is exactly that of a round
        // boundary, and hscmp_grow_events + hscmp_continue resume bit for bit.
        if (sh.nev + sh.n > P.cap) {
            if (tid == 0) { stats[ST_STOP] = STOP_CAPACITY; V.ctl[WC_DONE] = 1; V.ctl[WC_ALO] = 0; V.ctl[WC_AHI] = 0; V.ctl[WC_STEPS] += 1; }
            return;
        }
    }
    const int n = sh.n;
    const bool own_atoms = !sh.spaced || sh.nedge > 0;              // some atoms of the round are applied here
    if (own_atoms) Pol::prologue(P, S, G, A, plds, b);              // dictionary image, weights, edge record (ends with a barrier)
    bool handed = false;
    while (pos < n) {                                               // (uniform)
        RpPending pend; pend.on = 0;
        R pend_c = (R)0;
        bool own = false;
        if (wv == 0) {
            int gend;
            if (!sh.spaced) {
                // overlapping atoms: one at a time, energies as of its turn
                gend = pos + 1; own = true;
                if (pos > 0) {
                    const int me = V.ord[pos];
                    R eb, ea;
                    Pol::energies(P, S, G, A, plds, V.c_t[me], V.c_k[me], V.c_c[me], lane, wv, eb, ea);
                    if (lane == 0) { V.c_eb[me] = eb; V.c_ea[me] = ea; }
                    __threadfence_block();
                    __builtin_amdgcn_wave_barrier();
                }
            } else if (sh.nedge == 0) {
                gend = n;
            } else if (!(V.c_flag[V.ord[pos]] & RPF_INTERIOR)) {
                gend = pos + 1; own = true;                         // an atom at a signal end: alone
            } else {
                gend = pos + 1;
                while (gend < n && (V.c_flag[V.ord[gend]] & RPF_INTERIOR)) ++gend;
            }
            rp_wave_prefix<R>(P, sh, G, pos, gend, lane, pend, pend_c);   // (-> sh.napply, sh.gend, sh.converged / sh.stop)
            if (lane == 0) sh.full = own ? 1 : 0;                   // (the group's kind, for the other waves)
        }
        __syncthreads();
        if (wv == 0) rp_store_pending<R>(P, G, pend, pend_c);
        own = sh.full != 0;
        const int aend = sh.napply, gend = sh.gend;
        if (!own) {                                                 // interior atoms: the grid applies ord[pos, aend)
            if (tid == 0) { V.ctl[WC_ALO] = pos; V.ctl[WC_AHI] = aend; }
            handed = true;
            pos = gend;
            break;
        }
        // one atom, here: subtraction, then its rows from the final residual
        const int me = V.ord[pos];
        const int p = V.c_t[me], k = V.c_k[me], flag = V.c_flag[me];
        const R c = V.c_c[me];
        if (wv == 0 && aend > pos) Pol::subtract(P, S, G, A, plds, p, k, c, lane, wv);
        __syncthreads();
        if (aend > pos) {
            const int upa = Pol::units_per_atom(P);
            for (int q = wv; q < upa; q += kRpWaves) Pol::recorrelate(P, S, G, A, plds, p, k, q, (flag & RPF_INTERIOR) != 0, lane, wv);
        }
        __syncthreads();
        if (aend > pos && !(flag & RPF_INTERIOR) && tid == 0) Pol::after_atom(P, A, plds, p);
        __syncthreads();
        if (sh.converged) break;
        pos = gend;
    }
    const bool round_over = sh.converged || pos >= n;
    if (own_atoms) Pol::epilogue(P, S, A, plds, b);
    if (tid == 0) {
        if (!handed) { V.ctl[WC_ALO] = 0; V.ctl[WC_AHI] = 0; }
        if (round_over) {
            if (n == 0) { sh.converged = 1; if (sh.stop == STOP_RUNNING) sh.stop = STOP_EMPTY; }     // :1150-1153
            sh.rounds += 1;
            sh.offset = !sh.offset;
            const int run = V.ctl[WC_ROUNDS_RUN] + 1;
            V.ctl[WC_ROUNDS_RUN] = run;
            V.ctl[WC_MID] = 0;
            if (sh.converged || (P.max_rounds > 0 && run >= P.max_rounds)) V.ctl[WC_DONE] = 1;
        } else {
            V.ctl[WC_MID] = 1;
        }
        V.ctl[WC_POS] = pos; V.ctl[WC_N] = n; V.ctl[WC_SPACED] = sh.spaced; V.ctl[WC_NEDGE] = sh.nedge;
        V.ctl[WC_STEPS] += 1;
        stats[ST_NNZ] = sh.nnz; stats[ST_DUP] = sh.ndup; stats[ST_ROUNDS] = sh.rounds; stats[ST_STOP] = sh.stop;
        stats[ST_ITERS] = sh.iters; stats[ST_EVENTS] = sh.nev; stats[ST_SLOTS] = sh.nslots; stats[ST_OFFSET] = sh.offset;
        S.energy[2 * b + 1] = sh.e_res;
    }
}

// ---- P4 on the grid: ord[ALO, AHI), one wave per atom.  The body of RpMfma::subtract (hscmp_rp.h) for INTERIOR atoms: the even-W
//      quirk at p == T-1-W makes an atom non-interior (RpMfma::is_interior), so no edge record is read or written; the taps come
//      straight from the dictionary image in global memory (one atom's W words: staging the image would cost more).
//      grid = (workgroups, B), block = kRpThreads
template <typename Pol>
__global__ __launch_bounds__(kRpThreads) void wide_subtract_kernel(DevParams P, State<float> S, typename Pol::Args A, char* wbuf)
{
    const int b = blockIdx.y;
    const WideView V = wide_view(wbuf, P.B, P.maxsel, b);
    const int alo = V.ctl[WC_ALO], ahi = V.ctl[WC_AHI];
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    float* r = S.residual + (int64_t)b * P.T;
    for (int i = alo + blockIdx.x * kRpWaves + wv; i < ahi; i += gridDim.x * kRpWaves) {      // (wave-uniform)
        const int me = V.ord[i];
        const int p = V.c_t[me], k = V.c_k[me];
        int s, e, es;
        const int len = centered_span(P.T, P.W, p, s, e, es);
        const float nc = -V.c_c[me];
        float v[2] = {0.0f, 0.0f};
#pragma unroll
        for (int u = 0; u < 2; ++u) if (lane + 64 * u < len) v[u] = r[s + lane + 64 * u];
#pragma unroll
        for (int u = 0; u < 2; ++u) {
            const int q = lane + 64 * u;
            if (q < len) {
                const float prod = nc * A.dimg[dimg_index(k, es + q, A.S4)];      // -c*D[k] rounded, then += (utils.py:120,129)
                r[s + q] = v[u] + prod;
            }
        }
    }
}

// ---- P5 on the grid: the (atom, 32-row tile) units of ord[ALO, AHI), one wave per unit, around the dictionary image in LDS.
//      grid = (workgroups, B), block = kRpThreads
template <typename Pol>
__global__ __launch_bounds__(kRpThreads) void wide_recorrelate_kernel(DevParams P, State<float> S, typename Pol::Args A, char* wbuf)
{
    extern __shared__ __attribute__((aligned(16))) char smem[];
    const int b = blockIdx.y;
    const WideView V = wide_view(wbuf, P.B, P.maxsel, b);
    const int alo = V.ctl[WC_ALO], ahi = V.ctl[WC_AHI];
    const int upa = Pol::units_per_atom(P);
    const int nu = (ahi - alo) * upa;
    if ((int)blockIdx.x * kRpWaves >= nu) return;                   // (uniform; before anything is staged)
    const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    const Sig<float> G = wide_sig(P, S, b);
    Pol::prologue(P, S, G, A, smem, b);                             // (ends with a workgroup barrier)
    for (int u = blockIdx.x * kRpWaves + wv; u < nu; u += gridDim.x * kRpWaves) {      // (wave-uniform)
        const int a = u / upa, q = u - a * upa;
        const int me = V.ord[alo + a];
        Pol::recorrelate(P, S, G, A, smem, V.c_t[me], V.c_k[me], q, true, lane, wv);
    }
}

// host-side dispatch -----------------------------------------------------------------------------
// LDS of the control workgroup: its block, the sort keys, the policy's strips and image
template <typename Pol> inline size_t wide_control_lds(const DevParams& P, const typename Pol::Args& A)
{
    return ((sizeof(WideShared) + 15) / 16) * 16 + (size_t)wide_sort_entries(P.maxsel) * sizeof(unsigned long long) + Pol::policy_lds_bytes(A);
}

// can the wide loop run these parameters at all (float32, F = 1, the compile-time widths of RpMfma)
inline bool wide_params_ok(const DevParams& P)
{
    return rp_params_ok(P, kWideMaxSel) && P.F == 1 && P.T >= 3 * P.W - 2;
}

// workgroups per signal of the three grid kernels
// (each workgroup of the candidates and re-correlate kernels stages the dictionary image once and strides over its units: at most
//  two workgroups per CU -- a round of up to 8192 units keeps one unit per wave, the latency-optimal split; a larger one shares the staging)
inline int wide_grid_cap() { return 2 * mfma_device_cus(); }
inline int wide_candidate_groups(const DevParams& P) { return P.bs <= 256 ? std::min(wide_grid_cap(), (P.maxsel + kRpWaves - 1) / kRpWaves) : P.maxsel; }
inline int wide_subtract_groups(const DevParams& P) { return std::min(1024, (P.maxsel + kRpWaves - 1) / kRpWaves); }
inline int wide_recorrelate_groups(const DevParams& P)
{
    const int upa = (2 * P.W - 1 + 31) / 32;
    return std::min(wide_grid_cap(), (P.maxsel * upa + kRpWaves - 1) / kRpWaves);
}

enum WideLaunch { kWideDry, kWideBegin, kWideStep };

template <int S4C, bool HAS_W>
static int wide_launch_t(hipStream_t stream, const DevParams& P, const State<float>& S, const MfmaArgs& A, char* wbuf, WideLaunch what)
{
    using Pol = RpMfma<S4C, HAS_W>;
    const size_t plds = Pol::policy_lds_bytes(A), clds = wide_control_lds<Pol>(P, A);
    const bool dry = what == kWideDry;
    const dim3 block(kRpThreads);
    if (dry || what == kWideBegin) {
        if (!dry) hipLaunchKernelGGL((wide_begin_kernel<float>), dim3(P.B), block, 0, stream, P, S, wbuf);
        if (launch_tile_kernel(wide_candidates_kernel<Pol>, dim3(wide_candidate_groups(P), P.B), block, plds, kLdsLoop, 0, dry, stream, P, S, A, wbuf)) return -1;
        if (!dry) return 0;
    }
    const int entries = wide_sort_entries(P.maxsel);
    if (launch_tile_kernel(wide_control_kernel<Pol>, dim3(P.B), block, clds, kLdsLoop, 0, dry, stream, P, S, A, wbuf, entries)) return -1;
    if (!dry) hipLaunchKernelGGL((wide_subtract_kernel<Pol>), dim3(wide_subtract_groups(P), P.B), block, 0, stream, P, S, A, wbuf);
    if (launch_tile_kernel(wide_recorrelate_kernel<Pol>, dim3(wide_recorrelate_groups(P), P.B), block, plds, kLdsLoop, 0, dry, stream, P, S, A, wbuf)) return -1;
    if (!dry && launch_tile_kernel(wide_candidates_kernel<Pol>, dim3(wide_candidate_groups(P), P.B), block, plds, kLdsLoop, 0, false, stream, P, S, A, wbuf)) return -1;
    return 0;
}

// kWideDry: 0 when the shape has a wide form whose LDS fits; kWideBegin: the start of a call (slot chains, control blocks, the
// first round's candidates; head[] must be -1 everywhere); kWideStep: control, subtract, re-correlate, candidates.  -1: no such form.
inline int wide_launch(hipStream_t stream, const DevParams& P, const State<float>& S, const float* dimg, char* wbuf, WideLaunch what)
{
    if (!wide_params_ok(P)) return -1;
    const MfmaArgs A = mfma_args<float>(P, S, dimg);
    return dispatch_chunks<false>(A.S4, A.has_w != 0, [&](auto s4c, auto hw) {
        return wide_launch_t<decltype(s4c)::value, decltype(hw)::value>(stream, P, S, A, wbuf, what);
    });
}

}  // namespace hscmp
