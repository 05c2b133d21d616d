/* hsckmeans.h -- C ABI of libhsckmeans.so: one iteration of the convolutional k-means learner
 * (ConvolutionalDictionaryLearner(algorithm='kmean'), hsc/modeling.py:420-524) on MI355X / gfx950, for a batch
 * of independent learners.  DESIGN.md section 14.
 *
 * One context per host thread (contexts are not thread safe).  Every entry point returns HSCKMEANS_OK (0) or a
 * negative status; hsckmeans_last_error() describes the last failure.  There is no CPU path: without a visible
 * HIP device hsckmeans_create fails.
 */
#ifndef HSCKMEANS_H
#define HSCKMEANS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    HSCKMEANS_OK = 0,
    HSCKMEANS_ERR_INVALID = -1,
    HSCKMEANS_ERR_NO_DEVICE = -2,
    HSCKMEANS_ERR_HIP = -3,
    HSCKMEANS_ERR_STATE = -4,
    HSCKMEANS_ERR_UNSUPPORTED = -5,
    HSCKMEANS_ERR_ALLOC = -6
};

enum { HSCKMEANS_F32 = 0, HSCKMEANS_F64 = 1 };

/* mode[b] of hsckmeans_step: skip learner b, or assign it in float32 / float64 */
enum { HSCKMEANS_SKIP = 0, HSCKMEANS_ASSIGN_F32 = 1, HSCKMEANS_ASSIGN_F64 = 2 };

/* timing_ms of hsckmeans_step (HIP events) */
enum {
    HSCKMEANS_TIME_UPLOAD = 0,     /* dictionary images and modes to the device */
    HSCKMEANS_TIME_ASSIGN = 1,     /* the assignment kernels */
    HSCKMEANS_TIME_CENTROIDS = 2,  /* norms, membership lists and centroid sums */
    HSCKMEANS_TIME_DOWNLOAD = 3,   /* results to the host */
    HSCKMEANS_TIMES = 4
};

typedef struct hsckmeans_ctx hsckmeans_ctx;

int hsckmeans_version(void);                           /* 1 */
int hsckmeans_create(hsckmeans_ctx** out, int device_id);
void hsckmeans_destroy(hsckmeans_ctx* ctx);
const char* hsckmeans_last_error(hsckmeans_ctx* ctx);  /* ctx may be NULL (errors of hsckmeans_create) */

/* Upload the data of B learners once:
 *   x      [B][T][F]  the signals, float32 or float64 (dtype HSCKMEANS_F32 / _F64), host memory, C order
 *   starts [B][N]     window starts, 0 <= starts < T - 2W + 1: window n of learner b is x[b][starts[b][n] : +2W]
 * The windows are read in place on the device in every later step. */
int hsckmeans_set_data(hsckmeans_ctx* ctx, const void* x, int dtype, int B, int T, int F, const int64_t* starts,
                       int N, int W);

/* One iteration for every learner b with mode[b] != HSCKMEANS_SKIP (their rows of the outputs are undefined).
 *   D       [B][K][W][F] float64, host memory: the current dictionaries.  A learner assigned in float32 must hold
 *           float32 values (they are narrowed exactly); float64 data needs HSCKMEANS_ASSIGN_F64.
 * Outputs, host memory:
 *   out_t, out_k [B][N]  the flat arg-max o = t * K + k of |c| over positions t = 0 .. W and atoms, c the
 *                        'valid' correlation of the window with atom k at t, one fma chain from +0 over
 *                        q = f * W + w (f outer, w inner) in the assignment dtype; the lowest o wins ties, and a
 *                        window whose scores are all NaN goes to (0, 0)
 *   out_count    [B][K]  members of every centroid
 *   out_nonzero  [B][K]  1 when some member has window index > 0 (the reference's np.any(members)), else 0
 *   out_sums     [B][K][W*F], the data's dtype: sum over the members, in ascending window order, starting from
 *                        the first member's row, of patch / ||patch|| (patch = x[b][start + t : +W], its squared
 *                        norm numpy's pairwise sum of the W*F squares, a zero norm divides by 1); 0 for no member
 *   timing_ms    [HSCKMEANS_TIMES] (may be NULL) */
int hsckmeans_step(hsckmeans_ctx* ctx, const double* D, int K, const int32_t* mode, int32_t* out_t, int32_t* out_k,
                   int32_t* out_count, int32_t* out_nonzero, void* out_sums, double* timing_ms);

#ifdef __cplusplus
}
#endif

#endif /* HSCKMEANS_H */
