/* windgnn_optim.h — optimiser-side additions to the C ABI of libwindgnn_hip.so: clipping the step's gradient by its global
 * L2 norm inside the training-step tail.
 *
 * Where the reference's users would call torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) between
 * loss.backward() and optimizer.step() (src/main.py:79-80), the tail of windgnn.h (wgnn_finish: reduce the deferred partial
 * sums + Adam + the W_ih images, one launch) leaves no room: the final gradient is consumed in the launch that produces it.
 * The pair below splits that tail around the norm, on the device, with no host synchronisation:
 *
 *   one rank        wgnn_bwd_mse_part(.., 7 | 8 | WGNN_BWD_DEFER), wgnn_finish_norm(6), wgnn_finish_clipped
 *   data parallel   .., wgnn_finish(6, NULL), all-reduce of the bucket, wgnn_finish_norm(0), wgnn_finish_clipped
 *                   (the summed bucket is the same on every rank and the norm is deterministic, so every rank derives the
 *                   same coefficient: no extra collective)
 *
 * Conventions are those of windgnn.h (device pointers owned by the caller, asynchronous on `stream`, negative wgnn_status on
 * failure).  `clip` is one more caller-kept device buffer of wgnn_clip_bytes() bytes, 256-byte aligned; it may be dirty before
 * wgnn_finish_norm, which writes every byte that it or the following wgnn_finish_clipped reads; no byte outside
 * [clip, clip + wgnn_clip_bytes) is touched.  The workspace layout and wgnn_workspace_bytes are unchanged.
 */
#ifndef WINDGNN_OPTIM_H
#define WINDGNN_OPTIM_H

#include "windgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WGNN_OPTIM_VERSION 1
int wgnn_optim_version(void);

/* Bytes of `clip`: two result floats, private padding and one partial sum of squares per workgroup of the widest
 * wgnn_finish_norm launch.  Depends on dims only; 0 for dims wgnn_workspace_bytes refuses. */
size_t wgnn_clip_bytes(const wgnn_dims* d);

/* The reduce half of the tail, and the norm.  Reduces the deferred partials named by `which` (0, 2, 4 or 6: wgnn_finish's
 * reduce bits) into `g` -- exactly what wgnn_finish(d, p, g, which, NULL, ..) writes, bit for bit, on the same workspace and
 * under the same ordering rules -- and, over all 8 tensors (those just reduced, from the values the launch writes; the others
 * as they stand in g; which = 0 is a pure pass over g):
 *     total = sqrt(sum g^2)          coef = min(1, max_norm / (total + 1e-6))
 * i.e. clip_grad_norm_ with norm_type = 2, its clamp to 1 included.  ((float*)clip)[0] = total, [1] = coef; the rest of clip
 * is private.  Two launches: the reduction, which leaves one fp32 partial sum of squares per workgroup in clip, and a
 * one-workgroup pass that adds those in fp64.  Every sum has a fixed order (no floating-point atomics): the same inputs give
 * the same total, bit for bit, on every run and on every rank.
 * max_norm > 0; +inf is allowed (coef = 1: the call only measures).  max_norm <= 0 or NaN, or any other `which`:
 * WGNN_ERR_SHAPE.  NULL g, clip or workspace: WGNN_ERR_NULL.  A non-finite total sets WGNN_STATUS_GRAD_NONFINITE in the
 * status block; coef then follows the formula as torch evaluates it (NaN for a NaN total, 0 for an infinite one). */
int wgnn_finish_norm(const wgnn_dims* d, const wgnn_grads* g, int which /* 0, 2, 4 or 6 */, float max_norm, void* clip,
                     void* workspace, size_t workspace_bytes, void* stream);

/* wgnn_finish(d, p, g, 0, adam, ..) with every gradient element entering Adam as g * coef (one fp32 rounding), coef read
 * from `clip` on the device: torch.optim.Adam on all 8 parameters and the refresh of p->prepared, one launch.
 * `g` is NOT rewritten: unlike torch's in-place clip_grad_norm_ it keeps the unclipped gradient; clip[0] and clip[1] are there
 * for callers that want the clipped values.  With coef == 1 the parameters, moments and images equal wgnn_finish(0, adam)'s
 * bit for bit.  Reads only what the preceding wgnn_finish_norm wrote to clip. */
int wgnn_finish_clipped(const wgnn_dims* d, const wgnn_params* p, const wgnn_grads* g, const wgnn_adam* adam, const void* clip,
                        void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WINDGNN_OPTIM_H */
