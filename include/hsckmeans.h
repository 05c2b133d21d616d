/* hsckmeans.h -- C ABI of libhsckmeans.so: one iteration of the convolutional k-means learner
 * (ConvolutionalDictionaryLearner(algorithm='kmean'), hsc/modeling.py:420-524) on MI355X / gfx950, for a batch
 * of independent learners (hsckmeans_set_data), or for one learner over a corpus of signals of different lengths
 * (hsckmeans_set_corpus, or hsckmeans_set_corpus_sparse for signals given as CSR).  DESIGN.md sections 14, 17 and 19.
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
    HSCKMEANS_TIME_CENTROIDS = 2,  /* norms, membership and centroid sums */
    HSCKMEANS_TIME_DOWNLOAD = 3,   /* results to the host */
    HSCKMEANS_TIMES = 4
};

/* The centroid half of a step (membership and sums) has two plans with the same bits in every output:
 *   1  one wave per centroid lists its members in a [K][N] table; one thread per (centroid, element) sums them;
 *   2  wide: a stable partition of the windows by centroid into one [N] index array with K + 1 offsets (per-chunk
 *      histograms, an ordered scan over (centroid, chunk), placement in window order), then one workgroup per
 *      (centroid, tile of up to 256 elements) that stages its members' normalised rows through a double-buffered LDS
 *      ring and adds them in list order.  Needs K <= HSCKMEANS_WIDE_MAX_K.
 *   0  auto (the default): plan 2 from HSCKMEANS_WIDE_FROM_WINDOWS windows on (and wherever plan 1's table would
 *      exceed its index range), if K allows it; else plan 1. */
enum { HSCKMEANS_PLAN_AUTO = 0, HSCKMEANS_PLAN_LISTS = 1, HSCKMEANS_PLAN_WIDE = 2 };
enum {
    HSCKMEANS_WIDE_CHUNK_WINDOWS = 1024,  /* windows per chunk of the partition (one workgroup of 4 waves, 256 windows each) */
    HSCKMEANS_WIDE_RING_ROWS = 16,        /* rows of a full 256-element tile per half of the LDS ring; a narrower tile of
                                             tw elements lies at the pitch tp = tw rounded up to a power of two and
                                             stages 16 * 256 / tp rows per half */
    HSCKMEANS_WIDE_MAX_K = 1024,          /* the placement keeps 4 x K cursors in LDS */
    HSCKMEANS_WIDE_FROM_WINDOWS = 1000    /* auto: measured, DESIGN.md section 17 */
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

/* Upload a corpus: B signals of different lengths stacked without padding, for ONE learner whose windows each lie
 * inside one signal.  Replaces the data of an earlier hsckmeans_set_data / _set_corpus (and the other way round).
 *   x           [row_offsets[B]][F]  the stacked signals, dtype as above
 *   row_offsets [B + 1]              ascending from 0: signal b is rows row_offsets[b] .. row_offsets[b + 1]
 *   starts      [N]                  stacked rows: window n is x[starts[n] : +2W]
 * Checked on the host before any allocation or read of x: every signal is longer than 2W and every window lies inside
 * one signal (row_offsets[b] <= start, start + 2W <= row_offsets[b + 1]), else HSCKMEANS_ERR_INVALID naming the signal
 * or window; more than 2^31 - 1 elements in the stack: HSCKMEANS_ERR_UNSUPPORTED.  Afterwards the context holds one
 * learner: hsckmeans_step takes D [1][K][W][F] and mode [1] and returns [1][N] / [1][K] outputs. */
int hsckmeans_set_corpus(hsckmeans_ctx* ctx, const void* x, int dtype, int B, const int64_t* row_offsets, int F,
                         const int64_t* starts, int N, int W);

/* Upload a sparse corpus: the stacked signals of hsckmeans_set_corpus given as CSR, for representations that are a
 * handful of non-zeros per thousand rows.  Replaces the data of an earlier hsckmeans_set_data /
 * _set_corpus / _set_corpus_sparse (and the other way round).
 *   row_offsets [B + 1]              as above: signal b is rows row_offsets[b] .. row_offsets[b + 1] of the stack
 *   indptr      [rows + 1]           rows = row_offsets[B]; row r holds the entries indptr[r] .. indptr[r + 1]
 *   indices     [indptr[rows]]       columns, strictly ascending within a row, in [0, F)
 *   data        [indptr[rows]]       the entries' values, dtype as above (a stored zero is a zero)
 *   starts      [N]                  stacked rows: window n is the dense rows starts[n] .. starts[n] + 2W
 * The context afterwards holds ONE learner whose data is the window stack [N * 2W][F]: block n is the dense form of
 * window n's rows, built on the device from the entries the windows cover (only those are uploaded), and the device
 * start of window n is n * 2W.  hsckmeans_step then runs as after hsckmeans_set_corpus with these starts; out_t stays
 * relative to the window.  Device memory is proportional to N * 2W * F plus the covered entries, never to rows * F.
 * Checked on the host before any allocation or read of data: the rules of hsckmeans_set_corpus for the signals and
 * windows; indptr[0] = 0, indptr non-decreasing, indptr[rows] <= 2^31 - 1, every row's columns ascending and in range,
 * else HSCKMEANS_ERR_INVALID naming the row; N * 2W * F > 2^31 - 1: HSCKMEANS_ERR_UNSUPPORTED.  There is no limit on
 * rows * F. */
int hsckmeans_set_corpus_sparse(hsckmeans_ctx* ctx, int dtype, int B, const int64_t* row_offsets, int F,
                                const int64_t* indptr, const int32_t* indices, const void* data,
                                const int64_t* starts, int N, int W);

/* The centroid plan of the later steps: HSCKMEANS_PLAN_AUTO, _LISTS or _WIDE (anything else: HSCKMEANS_ERR_INVALID).
 * Kept across hsckmeans_set_data / _set_corpus.  A step under plan 2 with K > HSCKMEANS_WIDE_MAX_K is refused. */
int hsckmeans_set_plan(hsckmeans_ctx* ctx, int plan);

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
