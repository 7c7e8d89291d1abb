/* windgnn_series_train.h -- training on the sliding windows of one series: the MSE loss fused into the recurrences of
 * windgnn_series.h, as wgnn_fwd_loss / wgnn_bwd_mse_part(part | 8) fuse it into the materialised exact-fp32 step.
 *
 * A label row depends on the hour alone, exactly as a row of the input projection does: with
 *
 *     Ls [ls_rows][H]           hour-major, ls_rows >= (n-1)*stride + T          (windgnn_amd.series.series_labels' Ls)
 *
 * the label of window w at step t is row w*stride + t of Ls, and the recurrence kernels read it there, beside the GI row they
 * load anyway.  No window-major label tensor L [n][T][H], no dY [n][T][H] and no pass over Y exist:
 *
 *     wgnn_series_fwd_loss      Y and the stash of wgnn_series_fwd, bit for bit (the statistics do not enter h), plus per
 *                               workgroup of 16 windows the sum and the maximum of (h - label)^2 resp. |h - label| in loss_buf
 *     wgnn_series_bwd_mse       BPTT forms dY = 2 (Y - label) grad_scale / (n T H) from the h_prev it loads anyway; its first
 *                               workgroup sums the partial sums in a fixed order into loss[0] = mean((Y - label)^2) over all
 *                               n T H elements (NOT weighted by grad_scale: wgnn_bwd_mse_part's convention); the rest is
 *                               wgnn_series_bwd.  The result equals wgnn_mse_loss_grad on the materialised labels followed by
 *                               wgnn_series_bwd; `grads` holds final values on return (stream-ordered).
 *
 * windgnn_series.h, its stash layout and WGNN_SERIES_VERSION are unchanged: the statistics live in a small caller-owned buffer,
 *
 *     loss_buf                  wgnn_series_loss_bytes(sd) = 4 * (2 * ceil(n/16) + 4) bytes, 4-byte aligned: ceil(n/16) sums,
 *                               ceil(n/16) maxima, a tag word written by wgnn_series_fwd_loss, three spare words.
 *
 * A loss_buf whose tag is not wgnn_series_fwd_loss's (never written, or overwritten) behaves as a stash without statistics does
 * in wgnn_bwd_mse_part: loss[0] = NaN and WGNN_STATUS_NO_LOSS_STATS is set in a status block -- here the one of the workspace's
 * window-major half, WGNN_STATUS_BYTES at byte wgnn_series_status_offset(sd) of the workspace (the block at byte 0 belongs to the
 * hour-major half; kernels only OR into either, so the caller zeroes both once).  A C caller that reads a non-zero word there
 * treats it as WGNN_ERR_RANGE; the gradients of such a call are not to be used.  Only C callers read this block: the Python
 * layer (series_backward_mse_raw, TrainStep.step_series) always passes the loss_buf its own forward has just written, so it
 * cannot reach the state, and its check_range_status reads the block at byte 0 alone.
 *
 * Scope, conventions, alignment and the validation order are those of windgnn_series.h (version 1: exact fp32, fp32 I/O, dense
 * adjacency with S <= 64, F = 13, H <= 128; everything else WGNN_ERR_UNSUPPORTED before any launch).  In addition: NULL Ls,
 * loss_buf or loss: WGNN_ERR_NULL; ls_rows < (n-1)*stride + T, ls_rows*H >= 2^31, or a grad_scale that is not finite or not > 0:
 * WGNN_ERR_SHAPE.  Not here: deferred partial sums (WGNN_BWD_DEFER), the fp16-plane modes, CSR, carried state.
 */
#ifndef WINDGNN_SERIES_TRAIN_H
#define WINDGNN_SERIES_TRAIN_H

#include "windgnn_series.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WGNN_SERIES_TRAIN_VERSION 1
int wgnn_series_train_version(void);

/* Bytes of loss_buf (the partial pairs, the tag and the spare words); 0 for dims the entry points below refuse.  Depends on n
 * alone among accepted dims. */
size_t wgnn_series_loss_bytes(const wgnn_series_dims* sd);

/* Byte offset in the workspace of the status block that wgnn_series_bwd_mse ORs WGNN_STATUS_NO_LOSS_STATS into; 0 for refused
 * dims (for accepted ones it is >= WGNN_STATUS_BYTES). */
size_t wgnn_series_status_offset(const wgnn_series_dims* sd);

/* wgnn_series_fwd with the labels: Y [n][T][H], the stash (nullable, as there) and the statistics into loss_buf.
 * Errors as wgnn_series_fwd, plus those in the head comment. */
int wgnn_series_fwd_loss(const wgnn_series_dims* sd, const float* A, const float* Xs, const wgnn_params* p, const float* Ls,
                         int64_t ls_rows, float* Y, void* stash, void* loss_buf, void* workspace, size_t workspace_bytes,
                         void* stream);

/* grads (all 8, overwritten) = the gradients of grad_scale * mean((Y - labels)^2); loss[0] = that mean, unweighted.  Y, stash,
 * loss_buf: as wgnn_series_fwd_loss left them for the same sd, A, Xs, p, Ls.  Errors as wgnn_series_bwd, plus those in the head
 * comment. */
int wgnn_series_bwd_mse(const wgnn_series_dims* sd, const float* A, const float* Xs, const wgnn_params* p, const float* Y,
                        const float* Ls, int64_t ls_rows, float grad_scale, const void* stash, const void* loss_buf, float* loss,
                        const wgnn_grads* grads, void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WINDGNN_SERIES_TRAIN_H */
