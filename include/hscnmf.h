/* hscnmf.h -- C ABI of libhscnmf.so: batched convolutional NMF coefficients (the reference's
 * ConvolutionalNMF.computeCoefficients, hsc/modeling.py:662-747) and the convolutional NMF dictionary
 * learner (ConvolutionalDictionaryLearner(algorithm='nmf'), hsc/modeling.py:330-417), for one signal per dictionary
 * (hscnmf_learn) or one dictionary over a corpus of signals (hscnmf_learn_corpus), and the coefficients of a corpus of
 * signals of different lengths in one call (hscnmf_compute_ragged), on MI355X / gfx950.
 *
 * One context per host thread (contexts are not thread safe).  Every entry point returns
 * HSCNMF_OK (0) or a negative status; hscnmf_last_error() describes the last failure.
 * There is no CPU path: without a visible HIP device hscnmf_create fails.
 */
#ifndef HSCNMF_H
#define HSCNMF_H

#include <stdint.h>

#include "hscnmf_plan.h"

#ifdef __cplusplus
extern "C" {
#endif

enum {
    HSCNMF_OK = 0,
    HSCNMF_ERR_INVALID = -1,
    HSCNMF_ERR_NO_DEVICE = -2,
    HSCNMF_ERR_HIP = -3,
    HSCNMF_ERR_UNSUPPORTED = -5,
    HSCNMF_ERR_ALLOC = -6
};

enum { HSCNMF_F32 = 0, HSCNMF_F64 = 1 };

/* per-signal stop reasons (hsc/modeling.py:729-740, checked in this order) */
enum { HSCNMF_STOP_RUNNING = 0, HSCNMF_STOP_MAX_ITERATIONS = 1, HSCNMF_STOP_RESIDUAL_SCALE = 2, HSCNMF_STOP_SNR = 3 };

typedef struct hscnmf_ctx hscnmf_ctx;

typedef struct {
    int32_t max_iterations;           /* >= 1 (the reference's nbMaxIterations=None stops after the first iteration) */
    int32_t has_residual_scale;       /* toleranceResidualScale is not None */
    int32_t has_snr;                  /* toleranceSnr is not None */
    int32_t reserved;
    double tolerance_residual_scale;
    double tolerance_snr;
    uint64_t memory_budget;           /* device bytes for one chunk of signals (learners; whole signals of different
                                         lengths in hscnmf_compute_ragged), for the whole corpus in hscnmf_learn_corpus;
                                         0: 60% of the free memory */
} hscnmf_params;

int hscnmf_version(void);                          /* 2: hscnmf_learn (hscnmf_learn_corpus, hscnmf_compute_ragged and
                                                      hscnmf_ragged_plan were added without a new version) */
int hscnmf_create(hscnmf_ctx** out, int device_id);
void hscnmf_destroy(hscnmf_ctx* ctx);
const char* hscnmf_last_error(hscnmf_ctx* ctx);   /* ctx may be NULL (errors of hscnmf_create) */

/* Runs the multiplicative updates for B signals sharing one dictionary.  All pointers are host memory, C order:
 *   x       [B][T][F]   signals
 *   D       [K][W][F]   dictionary
 *   a_init  [B][T][K]   initial coefficients (only rows 0 .. T-W are read: the others never reach a reconstruction)
 *   energy  [B]         sum of squares of each signal (float64)
 * outputs:
 *   coefficients [B][T][K]  the reference's coefficientsCentered: rows W'..W'+T-W hold the coefficients, W' = (W-1)/2,
 *                           the other rows are set to zero
 *   residual     [B][T][F]  x minus the reconstruction of the last iteration
 *   iterations   [B] int32, stop [B] int32 (HSCNMF_STOP_*), snr [B] float64, residual_scale [B] float64
 *   timing_ms    [5] float64 (may be NULL): upload, iterations, download (ms from HIP events, summed over chunks),
 *                number of chunks, number of iterations run (summed over chunks)
 * Requires W >= 2 and T >= W.  A failed device allocation answers HSCNMF_ERR_ALLOC, here as in every other entry point,
 * the message naming the entry point and the bytes; the call's device memory is freed when it returns. */
int hscnmf_compute(hscnmf_ctx* ctx, int dtype, const void* x, int B, int T, int F, const void* D, int K, int W,
                   const void* a_init, const double* energy, const hscnmf_params* params,
                   void* coefficients, void* residual, int32_t* iterations, int32_t* stop, double* snr,
                   double* residual_scale, double* timing_ms);

/* Trains B independent dictionaries, one per signal (the reference's _train_nmf).  One iteration is the W multiplicative
 * steps of hscnmf_compute (each learner with its own D), then the dictionary update D *= N / den with
 * N[k][t][f] = sum_s A[s][k] R[s+t][f], den[k] = sum_s A[s][k] (s < T-W+1, R = x / |recon| of the updated A and the
 * old D), each atom divided by its l2 norm when that is > 0, then the residual with the new D and the stop rules of
 * hscnmf_compute.  All pointers are host memory, C order:
 *   x       [B][T][F]     signals
 *   D_init  [B][K][W][F]  initial dictionaries
 *   a_init  [B][T][K]     initial coefficients (only rows 0 .. T-W are read)
 *   energy  [B]           sum of squares of each signal (float64)
 * outputs:
 *   D_out   [B][K][W][F]  the learnt dictionaries (a learner's D is frozen from the iteration at which it stops)
 *   iterations, stop, snr, residual_scale, timing_ms: as for hscnmf_compute (the residual of the last iteration)
 * Requires W >= 2 and T >= W.  Learners are independent: a learner's result depends only on its own inputs. */
int hscnmf_learn(hscnmf_ctx* ctx, int dtype, const void* x, int B, int T, int F, const void* D_init, int K, int W,
                 const void* a_init, const double* energy, const hscnmf_params* params, void* D_out,
                 int32_t* iterations, int32_t* stop, double* snr, double* residual_scale, double* timing_ms);

/* Trains ONE dictionary from a corpus of B signals of different lengths.  One iteration: for every signal the W
 * multiplicative steps of hscnmf_compute against the shared D and R_b = x_b / |recon(A_b, D)|; then D *= N / den with
 * N[k][t][f] = sum_b sum_{s < L_b} A_b[s][k] R_b[s+t][f], den[k] = sum_b sum_{s < L_b} A_b[s][k] (L_b = T_b-W+1), each
 * atom divided by its l2 norm when that is > 0; then the residuals with the new D and the stop rules of hscnmf_compute
 * on the corpus: residual scale max_b max|r_b|, SNR 10 log10(sum_b energy_b / sum_b sum r_b^2).
 * Order of every floating-point sum (no atomics): within a signal exactly hscnmf_learn's (tiles of 128 rows in
 * ascending order for N and den, its strided partials and tree for the residual sums), then the signals in ascending
 * order.  A corpus of one signal gives hscnmf_learn's result on that signal bit for bit.
 * All pointers are host memory, C order:
 *   x        [rows][F]      the signals stacked without padding, rows = sum_b T_b
 *   lengths  [B] int64      T_b
 *   D_init   [K][W][F]      the one initial dictionary
 *   a_init   [sum_b L_b][K] the signals' initial coefficients stacked (rows 0 .. T_b-W of each signal only)
 *   energy   [B]            sum of squares of each signal (float64)
 * outputs:
 *   D_out    [K][W][F]      the learnt dictionary
 *   iterations, stop, snr, residual_scale: one value each, for the corpus
 *   signal_snr, signal_residual_scale [B] float64: the same statistics of each signal at the last iteration
 *   timing_ms [5] float64 (may be NULL): upload, iterations, download, 1, number of iterations run
 * Requires W >= 2, B >= 1 and every T_b >= W.  Limits, answered with HSCNMF_ERR_UNSUPPORTED before anything is allocated:
 * B <= 4 194 304; sum_b ceil(T_b / 128) <= 2^24 - 1 tiles of 128 samples over all signals (at most 2^31 - 128 samples);
 * B * ceil(K * (W*F + 1) / 256) <= 2^24 - 1; per signal and for K, W, F the limits of hscnmf_learn.  (Signals and tiles
 * lie on 1-D grids of 256-thread workgroups, which HIP launches only below 2^32 threads in all; the offsets into the
 * stacks are 64-bit on the device.)
 * The whole corpus is resident for the call: the bytes needed are worked out before the first allocation, and a corpus
 * that needs more than params->memory_budget (0: 60% of the free memory) fails with HSCNMF_ERR_ALLOC, the message naming
 * both numbers, with nothing allocated.  There is no chunking: an iteration needs every signal. */
int hscnmf_learn_corpus(hscnmf_ctx* ctx, int dtype, const void* x, const int64_t* lengths, int B, int F, const void* D_init,
                        int K, int W, const void* a_init, const double* energy, const hscnmf_params* params, void* D_out,
                        int32_t* iterations, int32_t* stop, double* snr, double* residual_scale, double* signal_snr,
                        double* signal_residual_scale, double* timing_ms);

/* hscnmf_compute for B signals of different lengths sharing one dictionary.  With L_b = T_b-W+1 and W' = (W-1)/2, all
 * pointers host memory, C order:
 *   x        [rows][F]      the signals stacked without padding, rows = sum_b T_b
 *   lengths  [B] int64      T_b
 *   D        [K][W][F]      the one dictionary
 *   a_init   [sum_b L_b][K] the signals' initial coefficients stacked (rows 0 .. T_b-W of each signal only)
 *   energy   [B]            sum of squares of each signal (float64)
 * outputs:
 *   coefficients [rows][K]  per signal the reference's coefficientsCentered: rows W' .. W'+L_b-1 of the signal's own block
 *                           hold its coefficients, its other rows are set to zero
 *   residual     [rows][F]
 *   iterations, stop, snr, residual_scale [B]; timing_ms [5] (may be NULL): as for hscnmf_compute, summed over chunks
 * Signal b gets, bit for bit, what hscnmf_compute gives it as a batch of one on x_b and its rows of a_init: coefficients,
 * residual, iteration count, stop reason, SNR and residual scale, whatever the other signals are, whatever their order
 * and wherever the chunk boundaries fall.  Every signal has its own stop state; the workgroups of a stopped signal return
 * at its flag.
 * Chunks: a chunk is a run of consecutive signals whose device bytes (the coefficient pair, x, the residual, the residual
 * partials, the per-signal state and the tile tables; D is uploaded once beside them) stay within params->memory_budget
 * (0: 60% of the free memory), whose tiles of 128 samples number at most 2^24 - 1 and whose signals at most 4 194 304; a
 * chunk always holds at least one signal.  hscnmf_ragged_plan (hscnmf_plan.h) gives the chunks of a budget.
 * Refused before anything is allocated, the message naming the signal where there is one: HSCNMF_ERR_INVALID for a NULL
 * argument, an unknown dtype, B, K or F < 1, W < 2, max_iterations < 1 or a T_b < W; HSCNMF_ERR_UNSUPPORTED for a W, F
 * whose workgroup does not fit the LDS, W*F > 2^24, or a signal with L_b * K > 2^28 or more than 2^24 - 1 tiles.  A failed
 * allocation (HSCNMF_ERR_ALLOC) leaves nothing allocated. */
int hscnmf_compute_ragged(hscnmf_ctx* ctx, int dtype, const void* x, const int64_t* lengths, int B, int F,
                          const void* D, int K, int W, const void* a_init, const double* energy,
                          const hscnmf_params* params, void* coefficients, void* residual,
                          int32_t* iterations, int32_t* stop, double* snr, double* residual_scale, double* timing_ms);

/* hscnmf_ragged_plan, the chunks hscnmf_compute_ragged forms under a budget (host arithmetic, no context), is declared
 * in hscnmf_plan.h, which this header includes: the entry points declared here all take a context. */

#ifdef __cplusplus
}
#endif

#endif /* HSCNMF_H */
