/* hscnmf_plan.h -- the context-free part of the C ABI of libhscnmf.so: host arithmetic that needs neither a context nor a
 * device.  include/hscnmf.h includes this header; its status values (HSCNMF_OK, HSCNMF_ERR_*) and dtype codes are those of
 * hscnmf.h.  An error of a call declared here is read with hscnmf_last_error(NULL).
 */
#ifndef HSCNMF_PLAN_H
#define HSCNMF_PLAN_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The chunks hscnmf_compute_ragged forms under a budget of budget_bytes (> 0) per chunk: host arithmetic only, no
 * context and no device.  chunk_first [B+1] int32 (may be NULL): chunk c
 * is the signals chunk_first[c] .. chunk_first[c+1]-1, chunk_first[*n_chunks] = B; *max_chunk_bytes: the device bytes of
 * the largest chunk, which is the one allocation of the call beside D (a signal that alone exceeds the budget still gets a
 * chunk of its own).  The same argument checks and refusals as hscnmf_compute_ragged. */
int hscnmf_ragged_plan(int dtype, const int64_t* lengths, int B, int F, int K, int W, uint64_t budget_bytes,
                       int32_t* chunk_first, int32_t* n_chunks, uint64_t* max_chunk_bytes);

#ifdef __cplusplus
}
#endif

#endif /* HSCNMF_PLAN_H */
