/* hscnmf.h -- C ABI of libhscnmf.so: batched convolutional NMF coefficients (the reference's
 * ConvolutionalNMF.computeCoefficients, hsc/modeling.py:662-747) and the convolutional NMF dictionary
 * learner (ConvolutionalDictionaryLearner(algorithm='nmf'), hsc/modeling.py:330-417) on MI355X / gfx950.
 *
 * One context per host thread (contexts are not thread safe).  Every entry point returns
 * HSCNMF_OK (0) or a negative status; hscnmf_last_error() describes the last failure.
 * There is no CPU path: without a visible HIP device hscnmf_create fails.
 */
#ifndef HSCNMF_H
#define HSCNMF_H

#include <stdint.h>

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
    uint64_t memory_budget;           /* device bytes for one chunk of signals (learners); 0: 60% of the free memory */
} hscnmf_params;

int hscnmf_version(void);                          /* 2: hscnmf_learn */
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
 * Requires W >= 2 and T >= W. */
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

#ifdef __cplusplus
}
#endif

#endif /* HSCNMF_H */
