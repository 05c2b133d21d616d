/* hscksvd.h -- C ABI of libhscksvd.so: the dictionary-update stage of the convolutional K-SVD learner
 * (ConvolutionalDictionaryLearner(algorithm='ksvd'), hsc/modeling.py:528-641) on MI355X / gfx950.
 * DESIGN.md section 13.
 *
 * One context per host thread (contexts are not thread safe).  Every entry point returns
 * HSCKSVD_OK (0) or a negative status; hscksvd_last_error() describes the last failure.
 * There is no CPU path: without a visible HIP device hscksvd_create fails.
 */
#ifndef HSCKSVD_H
#define HSCKSVD_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
    HSCKSVD_OK = 0,
    HSCKSVD_ERR_INVALID = -1,
    HSCKSVD_ERR_NO_DEVICE = -2,
    HSCKSVD_ERR_HIP = -3,
    HSCKSVD_ERR_UNSUPPORTED = -5,
    HSCKSVD_ERR_ALLOC = -6
};

enum { HSCKSVD_MAX_ATOM_SIZE = 64 };   /* W * F */
enum { HSCKSVD_WIDE_FROM_OCCURRENCES = 64 };   /* hscksvd_update_corpus, plan 0: wide when some atom occurs this often */

/* per-atom record of hscksvd_update's out_atom_stats */
enum {
    HSCKSVD_STAT_OCCURRENCES = 0,      /* n_k: the non-zero coefficients of atom k when its turn came (0: skipped) */
    HSCKSVD_STAT_LAMBDA1 = 1,          /* largest eigenvalue of the decomposed matrix (see below) */
    HSCKSVD_STAT_LAMBDA2 = 2,          /* second largest (0 when n_k = 1) */
    HSCKSVD_STAT_SWEEPS = 3,           /* Jacobi sweeps run (0: no eigensolver needed) */
    HSCKSVD_ATOM_STATS = 4
};

typedef struct hscksvd_ctx hscksvd_ctx;

int hscksvd_version(void);                         /* 1 */
int hscksvd_create(hscksvd_ctx** out, int device_id);
void hscksvd_destroy(hscksvd_ctx* ctx);
const char* hscksvd_last_error(hscksvd_ctx* ctx);  /* ctx may be NULL (errors of hscksvd_create) */

/* One sweep of the K-SVD dictionary update over the atoms k = 0 .. K-1, in order: atom k sees the new atoms
 * and coefficients of every k' < k.  All pointers are host memory, C order, float64:
 *   D        [K][W][F]  in: the dictionary the coefficients were computed with; out: the updated dictionary
 *   indptr   [K+1]      CSC column pointers of the [T][K] coefficient matrix (indptr[0] = 0)
 *   indices  [nnz]      rows (times) of the stored entries, strictly ascending within each column, in [0, T)
 *   data     [nnz]      in: the coefficients; out: the occurrences of every updated atom hold their new values
 *   use_pca  0: the reference's SVD branch; 1: its PCA branch (requires F = 1)
 *   out_atom_stats [K][HSCKSVD_ATOM_STATS] (may be NULL)
 *   timing_ms      [3] (may be NULL): upload, sweep kernel, download (HIP events)
 *
 * Atom k with occurrences t_1 < ... < t_m (the rows of column k whose value is not 0.0; none: D[k] is kept):
 *   P_i = the W*F samples [t_i - (W-1)/2, t_i - (W-1)/2 + W) of the reconstruction of every OTHER atom's non-zero
 *         coefficient (the reference's `error`), 0 outside [0, T).  Each sample is summed from 0.0 in CSC order
 *         (column, then row), each term the rounded product c * D[k'][tap][f]: bit for bit the host overlap-add.
 *   SVD branch: G = sum_i P_i P_i^T, u = its top eigenvector, D[k] = u, c_i = P_i . u.
 *   PCA branch, m >= 2: the P_i are centred per component first (mean over the occurrences), G is their Gram
 *         matrix and c_i = centred P_i . u; the stats report G / (m - 1) (the covariance's eigenvalues).
 *   m = 1 (both branches): u = P_1 / |P_1|, c_1 = P_1 . u.
 * Rules LAPACK leaves open, fixed here:
 *   zero Gram matrix (every P_i zero), SVD branch: u = e_0, coefficients 0 (what scipy.linalg.svd returns);
 *   zero covariance, PCA branch: u = e_{W*F-1} (the last of eigh's tied maxima), coefficients 0;
 *   zero window, PCA branch with m = 1: u = 0 (normalize's rule), coefficient 0;
 *   sign: otherwise (an eigenvector, or P_1 / |P_1| in the SVD branch) u is oriented so that u . D_old[k] >= 0,
 *         and when that product is exactly 0 so that u's first non-zero entry is positive.
 *   ties: the first (SVD branch) / last (PCA branch) index of the largest eigenvalue.
 * The eigenvectors come from a cyclic parallel-ordered Jacobi method in float64; every sum runs in a fixed order
 * without atomics, so two calls on the same input return the same bits. */
int hscksvd_update(hscksvd_ctx* ctx, int T, int K, int W, int F, double* D, const int32_t* indptr,
                   const int32_t* indices, double* data, int use_pca, double* out_atom_stats, double* timing_ms);

/* The same sweep for ONE dictionary over a corpus of B signals of lengths T_0 .. T_{B-1}.  The
 * coefficient matrix is the vertical stack [sum T_b][K] of the per-signal matrices, in CSC; row g of the stack belongs
 * to signal b when row_offsets[b] <= g < row_offsets[b+1].
 *   row_offsets [B+1]  row_offsets[0] = 0, strictly ascending (no empty signal); row_offsets[B] = sum T_b, the row count
 *                      of the stack (int32: a stack of 2^31 rows or more cannot be passed)
 *   indices     [nnz]  stacked rows, strictly ascending within each column, in [0, sum T_b)
 *   plan        0: plan 2 when some atom has HSCKSVD_WIDE_FROM_OCCURRENCES occurrences or more, else plan 1;
 *               1: one workgroup walks all atoms (hscksvd_update's kernel); 2: wide, per atom a grid over its
 *               occurrences, a grid over the Gram entries and one workgroup for the eigenvectors, in stream order.
 *               Every plan returns the same bits.
 *   D, indptr, data, use_pca, out_atom_stats, timing_ms as in hscksvd_update.
 * The update is hscksvd_update's, with these differences:
 *   occurrences: the non-zero entries of column k of the stack in ascending stacked row (signal after signal, time
 *         ascending within a signal); every sum over the occurrences runs in that order.
 *   patches: P_i of an occurrence in signal b is the reconstruction of every other atom's non-zero coefficients OF
 *         SIGNAL b ONLY over [t_i - (W-1)/2, +W), 0 outside [0, T_b) of that signal: an atom's span is clipped at its
 *         own signal's ends and never contributes to a sample of another signal.  Each sample is summed from 0.0 in
 *         CSC order of the stack (column, then stacked row), rounded products, no FMA.
 * Two anchors follow: with B = 1 the result is bit for bit hscksvd_update's; and when every stored entry's span lies
 * inside its signal ((W-1)/2 <= t <= T_b - W + (W-1)/2) it is bit for bit hscksvd_update's on the plain stack, T = sum T_b. */
int hscksvd_update_corpus(hscksvd_ctx* ctx, int B, const int32_t* row_offsets, int K, int W, int F, double* D,
                          const int32_t* indptr, const int32_t* indices, double* data, int use_pca, int plan,
                          double* out_atom_stats, double* timing_ms);

/* B independent sweeps in ONE launch: B dictionaries of one shape, each with the coefficient matrix
 * [T][K] of its own signal.  Problem b is
 *   hscksvd_update(T, K, W, F, D[b], indptr[b], indices + entry_offsets[b], data + entry_offsets[b], use_pca, ...)
 * bit for bit -- D, data and stats -- and inherits every rule fixed above (sign, ties, the zero Gram matrix, m = 1, the PCA
 * branch) and the limits with their messages (W * F <= HSCKSVD_MAX_ATOM_SIZE, PCA needs F = 1).
 *   D             [B][K][W][F]  in / out
 *   entry_offsets [B+1]         entry_offsets[0] = 0, non-decreasing: problem b's stored entries are
 *                               [entry_offsets[b], entry_offsets[b+1]) of indices / data
 *   indptr        [B][K+1]      CSC column pointers of problem b, RELATIVE to its first entry (indptr[b][0] = 0,
 *                               indptr[b][K] = entry_offsets[b+1] - entry_offsets[b])
 *   indices, data               the problems' entries one after the other; rows in [0, T), strictly ascending per column
 *   out_atom_stats [B][K][HSCKSVD_ATOM_STATS] (may be NULL); timing_ms [3] (may be NULL): upload, the launch, download
 * One workgroup per problem runs the one-workgroup sweep (plan 1) over its own scratch: the grid is B, nothing is shared
 * between two problems, there are no atomics and every sum runs in the single sweep's order.  A problem without a stored
 * non-zero entry keeps its dictionary (stats 0).  All entries together must stay below 2^31. */
int hscksvd_update_batch(hscksvd_ctx* ctx, int B, int T, int K, int W, int F, double* D, const int64_t* entry_offsets,
                         const int32_t* indptr, const int32_t* indices, double* data, int use_pca, double* out_atom_stats,
                         double* timing_ms);

#ifdef __cplusplus
}
#endif

#endif /* HSCKSVD_H */
