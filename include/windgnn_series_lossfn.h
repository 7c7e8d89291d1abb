/* windgnn_series_lossfn.h -- series training on a LOSS SPEC: the mean square, the mean absolute error or the Huber loss, counted
 * from a warm-up step of every window onward, with or without missing labels.  The recurrences form the loss and dY from the h
 * they hold, as windgnn_series_train.h describes: no dY tensor exists, and the GCN, the projection, the fold and the GEMMs are
 * the ones of the other series entry points.
 *
 * A spec is wgnn_lossfn {kind, delta, t_from, masked}.  With row(w) = w*stride or clamp(starts[w], 0, rows - T),
 * r = Y[w][t][c] - Ls[row(w) + t][c],
 *
 *     M = { (w, t, c) : t >= t_from, and (masked == 0 or the label is not NaN) },   m = |M|
 *
 *     kind                 rho(r)                                                    d rho / d r
 *     WGNN_LOSS_MSE   0    r^2                                                       2 r
 *     WGNN_LOSS_L1    1    |r|                                                       sign(r), sign(0) = 0          (torch.sign)
 *     WGNN_LOSS_HUBER 2    0.5 r^2 if |r| <= delta, else delta (|r| - 0.5 delta)     clamp(r, -delta, delta)       (nn.HuberLoss)
 *
 *     wgnn_series_fwd_lossfn    Y and the stash of wgnn_series_fwd_loss, bit for bit; per workgroup of 16 windows the sum of rho
 *                               and the maximum of |r| over M, and the exact integer count of the workgroup's entries in M.  An
 *                               entry outside M is selected away, never multiplied by 0: a NaN label with masked = 1, and any
 *                               label at t < t_from, reaches no arithmetic whose result is kept.
 *     wgnn_series_bwd_lossfn    BPTT forms dY = grad_scale rho'(r) / m on M and exactly +0 elsewhere (it still runs every step: the
 *                               gradient flows back through the warm-up steps); loss[0] = (the partial sums, added in
 *                               wgnn_series_bwd_mse's fixed order) / m.
 *
 * t_from = 0 counts every step; t_from = T - 1 is last-step-only training.  Windows overlap, so "from step t_from on" is not a
 * NaN mask over Ls: row tau of Ls is step 20 of one window and step 1 of another.
 *
 * masked = 0: a NaN label at t >= t_from poisons the loss, as in wgnn_series_fwd_loss (loud on purpose); m = n (T - t_from) H is
 * known on the host, which forms 1.0f / (float)m and the dY factor (2.0f grad_scale / (float)m for MSE, grad_scale / (float)m
 * for L1 and Huber) with IEEE division.  masked = 1: every BPTT workgroup adds the counts itself and forms the same two
 * expressions on the device, as wgnn_series_bwd_mse_masked does.  So with {MSE, any delta, 0, 0} Y, the loss and all 8
 * gradients equal wgnn_series_fwd_loss + wgnn_series_bwd_mse (or their _at forms) bit for bit, and with {MSE, any delta, 0, 1}
 * the masked pair, with or without NaN.
 *
 * m = 0 (masked = 1 only): loss[0] = NaN, all 8 gradients exactly zero, WGNN_STATUS_NO_LABELS in the window-major half's status
 * block (windgnn_series_masked.h).
 *
 * One pair serves both row mappings, as the masked pair does: sd->stride >= 1 with starts == NULL, or sd->stride == 0 with the
 * table, its device check and its clamp.  Scope, validation order, error codes, workspace and stash sizes are the masked
 * pair's; loss_buf has the masked layout (wgnn_series_lossfn_bytes = wgnn_series_masked_loss_bytes: the counts are always
 * there).  Then the spec: fn == NULL: WGNN_ERR_NULL; kind outside 0..2, masked outside 0..1, t_from < 0 or >= T, Huber with a
 * delta that is not finite or <= 0: WGNN_ERR_SHAPE (delta is ignored for MSE and L1).  All of it before any HIP call.
 *
 * Pairing.  The forward writes a third tag value and the spec into the three spare words of loss_buf: kind | masked << 8, the
 * bits of delta (0 unless Huber), t_from.  wgnn_series_bwd_lossfn with another spec than its forward's, or on a loss_buf this
 * forward did not write, gives loss[0] = NaN, WGNN_STATUS_NO_LOSS_STATS and dY = 0 (all 8 gradients zero);
 * wgnn_series_bwd_mse and wgnn_series_bwd_mse_masked refuse this forward's loss_buf the same way.
 *
 * Not here: the materialised entry points and the fp16-plane modes, autograd (forward_series plus any torch loss works there),
 * per-element or per-station weights, quantile losses, masks on inputs, and the exchange of label counts between the ranks of
 * a process group.
 */
#ifndef WINDGNN_SERIES_LOSSFN_H
#define WINDGNN_SERIES_LOSSFN_H

#include "windgnn_series_masked.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WGNN_SERIES_LOSSFN_VERSION 1
int wgnn_series_lossfn_version(void);

#define WGNN_LOSS_MSE 0
#define WGNN_LOSS_L1 1
#define WGNN_LOSS_HUBER 2

typedef struct { int32_t kind; float delta; int32_t t_from; int32_t masked; } wgnn_lossfn;

/* Bytes of loss_buf: wgnn_series_masked_loss_bytes(sd); 0 for dims the entry points below refuse. */
size_t wgnn_series_lossfn_bytes(const wgnn_series_dims* sd);

int wgnn_series_fwd_lossfn(const wgnn_series_dims* sd, const float* A, const float* Xs, const int32_t* starts,
                           const wgnn_params* p, const float* Ls, int64_t ls_rows, const wgnn_lossfn* fn, float* Y, void* stash,
                           void* loss_buf, void* workspace, size_t workspace_bytes, void* stream);
int wgnn_series_bwd_lossfn(const wgnn_series_dims* sd, const float* A, const float* Xs, const int32_t* starts,
                           const wgnn_params* p, const float* Y, const float* Ls, int64_t ls_rows, float grad_scale,
                           const wgnn_lossfn* fn, const void* stash, const void* loss_buf, float* loss, const wgnn_grads* grads,
                           void* workspace, size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WINDGNN_SERIES_LOSSFN_H */
