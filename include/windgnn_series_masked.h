/* windgnn_series_masked.h -- series training and evaluation through MISSING LABELS: a NaN in the label series Ls means "no label
 * here".  It contributes nothing to the loss, nothing to any gradient and nothing to the statistics; the mean is taken over the
 * labels that exist.  Inputs are the caller's business: build Xs from the filled table and Ls from the unfilled one.
 *
 * With M = { (w, t, c) : Ls[row(w) + t][c] is not NaN } and m = |M| (an infinite label is a label; a window listed twice counts
 * twice), row(w) = w*stride or clamp(starts[w], 0, rows - T):
 *
 *     wgnn_series_fwd_loss_masked   Y and the stash of wgnn_series_fwd_loss, bit for bit; per workgroup of 16 windows the sum of
 *                                   (h - label)^2 and the maximum of |h - label| over M only (a missing entry is selected away,
 *                                   never multiplied by 0), and the exact integer count of the workgroup's entries in M
 *     wgnn_series_bwd_mse_masked    BPTT forms dY = 2 grad_scale (Y - label) / m on M and exactly +0 elsewhere; loss[0] = (the
 *                                   partial sums, added in wgnn_series_bwd_mse's fixed order) / m.  Every BPTT workgroup adds the
 *                                   ceil(n/16) counts itself before its loop (integer addition has no order), and forms
 *                                   1.0f / (float)m and 2.0f * grad_scale / (float)m with IEEE division, as the host does for
 *                                   wgnn_series_bwd_mse: with no NaN among the rows read, loss and all 8 gradients equal
 *                                   wgnn_series_fwd_loss + wgnn_series_bwd_mse bit for bit.
 *
 * m = 0 (every label read is missing): loss[0] = NaN, dY = 0 everywhere, so all 8 gradients are exactly zero, and
 * WGNN_STATUS_NO_LABELS is ORed into the window-major half's status block (byte wgnn_series_status_offset(sd) resp.
 * wgnn_series_at_status_offset(sd) of the workspace, where WGNN_STATUS_NO_LOSS_STATS goes).
 *
 * One pair of entry points serves both row mappings:
 *     sd->stride >= 1, starts == NULL    windgnn_series_train.h's strided windows
 *     sd->stride == 0, starts != NULL    windgnn_series_at.h's table, with its device check (WGNN_STATUS_WINDOW_START) and clamp
 * stride >= 1 with a table: WGNN_ERR_SHAPE; stride == 0 without one: WGNN_ERR_NULL.  Scope, validation order, error codes,
 * workspace and stash sizes are those of the unmasked entry points of the same row mapping (wgnn_series_workspace_bytes /
 * wgnn_series_stash_bytes, or their _at forms).  Only loss_buf differs:
 *
 *     loss_buf    wgnn_series_masked_loss_bytes(sd) = 4 * (3 * ceil(n/16) + 4) bytes, 4-byte aligned:
 *                 float  [ceil(n/16)]  sums | float [ceil(n/16)] maxima | float tag | 3 spare words | uint32 [ceil(n/16)] counts
 *                 (wgnn_series_loss_bytes' layout with the counts appended)
 *
 * The tag is a second value: wgnn_series_bwd_mse_masked on a loss_buf that wgnn_series_fwd_loss_masked did not write (an
 * unmasked forward's, or none), and wgnn_series_bwd_mse on a masked forward's, give loss[0] = NaN and
 * WGNN_STATUS_NO_LOSS_STATS, as windgnn_series_train.h describes; the masked backward then takes m = 0 (dY = 0) without setting
 * WGNN_STATUS_NO_LABELS.
 *
 * wgnn_eval_accum_series is wgnn_eval_accum (windgnn_eval.h) with the truth of window b read from a label series:
 * row (starts ? clamp(starts[b], 0, ls_rows - T) : b*stride) + T - 1 of Ls [ls_rows][H] instead of row T - 1 of labels[b].  The
 * table is in the caller's order (any order; it is only looked up).  With skip_missing != 0 a NaN truth adds nothing to its
 * column: the column's count row `n` is not incremented and abs_err (if given) receives NaN there, so the header's `n` row holds
 * per-column counts and a column with no truth at all has n = 0 and NaN figures.  The accumulator is wgnn_eval_bytes(H), one
 * owner per column, a fixed order, no atomics.  With skip_missing = 0 the header equals wgnn_eval_accum's on the gathered labels
 * bit for bit.  NULL pred, Ls or acc, or stride == 0 without a table: WGNN_ERR_NULL; B, T, H < 1, stride < 0, stride >= 1 with a
 * table, ls_rows < T, ls_rows < (B-1)*stride + T, ls_rows*H >= 2^31: WGNN_ERR_SHAPE.
 *
 * Not here: masked labels in the materialised entry points and the fp16-plane modes, other losses, masks on inputs, weights
 * other than present / absent, and the exchange of counts between the ranks of a process group.
 */
#ifndef WINDGNN_SERIES_MASKED_H
#define WINDGNN_SERIES_MASKED_H

#include "windgnn_series_at.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WGNN_SERIES_MASKED_VERSION 1
int wgnn_series_masked_version(void);

/* Status bit (the window-major half's status block): wgnn_series_bwd_mse_masked found no label at all (m = 0). */
#define WGNN_STATUS_NO_LABELS 32u

/* Bytes of the masked loss_buf (layout above); 0 for dims the entry points below refuse.  stride = 0 selects the table's dims. */
size_t wgnn_series_masked_loss_bytes(const wgnn_series_dims* sd);

int wgnn_series_fwd_loss_masked(const wgnn_series_dims* sd, const float* A, const float* Xs, const int32_t* starts,
                                const wgnn_params* p, const float* Ls, int64_t ls_rows, float* Y, void* stash, void* loss_buf,
                                void* workspace, size_t workspace_bytes, void* stream);
int wgnn_series_bwd_mse_masked(const wgnn_series_dims* sd, const float* A, const float* Xs, const int32_t* starts,
                               const wgnn_params* p, const float* Y, const float* Ls, int64_t ls_rows, float grad_scale,
                               const void* stash, const void* loss_buf, float* loss, const wgnn_grads* grads, void* workspace,
                               size_t workspace_bytes, void* stream);

/* pred [B][H] de-normalised, Ls [ls_rows][H] normalised; starts [B] int32 on the device or NULL; acc, abs_err as wgnn_eval_accum. */
int wgnn_eval_accum_series(const float* pred, const float* Ls, int64_t ls_rows, const int32_t* starts, int32_t stride, int32_t B,
                           int32_t T, int32_t H, float wind_min, float wind_max, int32_t skip_missing, void* acc, float* abs_err,
                           void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WINDGNN_SERIES_MASKED_H */
