/* windgnn_series_at.h -- series mode on windows that start at a TABLE of rows, not only at w*stride: a series with outages
 * (the windows that lie wholly inside a clean segment), a train / validation split at window level, shuffled mini-batches.
 *
 * With
 *
 *     starts [n]                int32 on the device, non-decreasing, 0 <= starts[w] <= rows - T
 *
 * window w = 0 .. n-1 covers rows starts[w] .. starts[w] + T - 1 of Xs [rows][S][13] (and of Ls, in the loss pair) and starts
 * from h = 0.  The results are those of windgnn.h on the materialised windows X[w][t] = Xs[starts[w] + t]: Y [n][T][H] and the 8
 * gradients summed over the listed windows.  Duplicates are legal (a window listed twice counts twice), and n may exceed
 * rows - T + 1.  The recurrence and its BPTT are the only readers of the table besides the fold,
 *
 *     dGIs[tau] = sum over { w : tau - T < starts[w] <= tau } of dGI[w][tau - starts[w]]
 *
 * whose windows are, the table being non-decreasing, the contiguous index range [lower_bound(starts, tau - T + 1),
 * upper_bound(starts, tau)): found by binary search, summed in ascending w in fp32 with plain loads and one store (no atomics,
 * the gradients repeat bit for bit).  With starts[w] = w*stride every result equals the strided entry point's bit for bit.
 * Everything else -- the front end on all `rows` rows, the weight-gradient products, dg, the GCN backward -- is windgnn_series.h's
 * and does not look at the table: the front end's cost is that of the series passed, whatever the table lists.
 *
 * The dims are wgnn_series_dims with stride = 0, meaning "table" (the strided entry points keep refusing stride < 1); workspace,
 * stash and loss_buf are sized by the queries below and depend on rows, T, n, S, H alone, never on the table's values.
 *
 * The table is checked on the device: every entry point below first launches one thread per window that ORs
 * WGNN_STATUS_WINDOW_START into the status word at byte 0 of the workspace if starts[w] < 0, starts[w] > rows - T or
 * starts[w] < starts[w-1].  The kernels clamp every start into [0, rows - T] and the fold skips a term whose row lies outside its
 * window, so such a call still returns WGNN_OK and reads and writes only what a valid call would, but its outputs hold
 * unspecified values: a caller that reads a non-zero status word treats it as WGNN_ERR_RANGE.
 *
 * Scope, conventions, alignment and the validation order are those of windgnn_series.h / windgnn_series_train.h (version 1: exact
 * fp32, fp32 I/O, dense adjacency with S <= 64, F = 13, H <= 128; everything else WGNN_ERR_UNSUPPORTED before any launch).
 * stride != 0, T > rows, n < 1 or an element count past the limits: WGNN_ERR_SHAPE.  NULL starts: WGNN_ERR_NULL.  The loss pair
 * requires ls_rows >= rows (a clamped start may read any window of the series) and ls_rows*H < 2^31.
 */
#ifndef WINDGNN_SERIES_AT_H
#define WINDGNN_SERIES_AT_H

#include "windgnn_series_train.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WGNN_SERIES_AT_VERSION 1
int wgnn_series_at_version(void);

/* Status bit (word 0 of the workspace): a window start outside [0, rows - T], or a table that decreases. */
#define WGNN_STATUS_WINDOW_START 16u

/* Sizes for dims with stride = 0; 0 for dims the entry points below refuse.  The status offset is that of
 * wgnn_series_status_offset (the window-major half's block, WGNN_STATUS_NO_LOSS_STATS). */
size_t wgnn_series_at_workspace_bytes(const wgnn_series_dims* sd);
size_t wgnn_series_at_stash_bytes(const wgnn_series_dims* sd);
size_t wgnn_series_at_loss_bytes(const wgnn_series_dims* sd);
size_t wgnn_series_at_status_offset(const wgnn_series_dims* sd);

/* wgnn_series_fwd / _fwd_last / _bwd with the table: the same arguments, `starts` after Xs. */
int wgnn_series_fwd_at(const wgnn_series_dims* sd, const float* A, const float* Xs, const int32_t* starts, const wgnn_params* p,
                       float* Y, void* stash, void* workspace, size_t workspace_bytes, void* stream);
int wgnn_series_fwd_last_at(const wgnn_series_dims* sd, const float* A, const float* Xs, const int32_t* starts,
                            const wgnn_params* p, float wind_min, float wind_max, float* last, void* workspace,
                            size_t workspace_bytes, void* stream);
int wgnn_series_bwd_at(const wgnn_series_dims* sd, const float* A, const float* Xs, const int32_t* starts, const wgnn_params* p,
                       const float* Y, const float* dY, const void* stash, const wgnn_grads* grads, void* workspace,
                       size_t workspace_bytes, void* stream);

/* wgnn_series_fwd_loss / wgnn_series_bwd_mse with the table: the label of window w at step t is row starts[w] + t of Ls. */
int wgnn_series_fwd_loss_at(const wgnn_series_dims* sd, const float* A, const float* Xs, const int32_t* starts,
                            const wgnn_params* p, const float* Ls, int64_t ls_rows, float* Y, void* stash, void* loss_buf,
                            void* workspace, size_t workspace_bytes, void* stream);
int wgnn_series_bwd_mse_at(const wgnn_series_dims* sd, const float* A, const float* Xs, const int32_t* starts,
                           const wgnn_params* p, const float* Y, const float* Ls, int64_t ls_rows, float grad_scale,
                           const void* stash, const void* loss_buf, float* loss, const wgnn_grads* grads, void* workspace,
                           size_t workspace_bytes, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WINDGNN_SERIES_AT_H */
