/* windgnn_sched.h -- schedule queries of libwindgnn_hip.so: how the library cuts work that it may cut in more than one way.
 * Host-only (no launch, no device pointer); nothing here changes a result.  Conventions are those of windgnn.h.
 */
#ifndef WINDGNN_SCHED_H
#define WINDGNN_SCHED_H

#include "windgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The split-K factors of the two GRU weight-gradient products (dW_ih | db_ih = dGI^T [g | 1], dW_hh | db_hh = dGH^T [Hprev | 1])
 * as the workspace layout of `d` fixes them: every consumer -- the GEMMs in either launch form (WGNN_OPT_TN_MERGED), the
 * partial regions of the workspace, the finish launches, the row-block entry points -- reads these two numbers.
 *   sk_ih, sk_hh          K chunks per output tile of each product
 *   kchunk_ih, kchunk_hh  rows of B*T per chunk (fp16-plane modes: a multiple of 32, the kernels' K step)
 *   merged                1: both products are plane-GEMM tiles and one launch runs them, workgroup w taking work item w of
 *                         dW_ih and then work item w of dW_hh (fp16-plane modes on the register-resident recurrence,
 *                         H <= 127; WGNN_OPT_TN_MERGED = 1); 0: one launch per product
 *   workgroups            fp16-plane modes: merged -- workgroups of that launch, the longer of the two item lists; else the
 *                         workgroups of the two launches together; 0 in exact fp32
 * Each product is split for at most 256 workgroups (one per CU of an MI355X) and chunks of at least 64 rows.  The answer is a
 * function of `d` and `state` alone -- not of the device, not of an option: the chunks fix the order of the fp32 sums, so a
 * run repeats bit for bit wherever it runs.  state != 0: the layout of the state stash. */
typedef struct wgnn_tn_split_info {
  int32_t sk_ih, sk_hh, kchunk_ih, kchunk_hh, merged, workgroups;
} wgnn_tn_split_info;
int wgnn_tn_split(const wgnn_dims* d, int state, wgnn_tn_split_info* out);

#ifdef __cplusplus
}
#endif
#endif /* WINDGNN_SCHED_H */
