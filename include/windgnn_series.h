/* windgnn_series.h — series mode: a second way into the model of windgnn.h, for windows that are overlapping slices of ONE
 * hourly series.
 *
 * windgnn.h takes materialised windows X [B][T][S][13].  Windows cut from real data overlap: at stride 1 every hour of the
 * series sits in up to T windows, and everything that depends on the hour alone -- both graph convolutions and the GRU's
 * input projection GI_t = [g_t | 1] [W_ih | b_ih]^T -- is then computed and stored T times.  Here the input is the series
 * itself,
 *
 *     Xs [rows][S][13]          window w = 0 .. n-1 covers rows w*stride .. w*stride + T - 1,   (n-1)*stride + T <= rows
 *
 * every window starts from h = 0, and the results are exactly those of wgnn_fwd / wgnn_bwd on X[w][t] = Xs[w*stride + t]:
 * Y [n][T][H] and the 8 parameter gradients summed over all windows.  The front end (GCN, projection) runs once per hour on
 * `rows` rows; only the recurrence, its BPTT and the dW_hh product are per window.  In the backward the hour-major half needs
 * only
 *
 *     dGIs[tau] = sum over { w : w*stride <= tau < w*stride + T } of dGI[w][tau - w*stride]        (the fold)
 *     dW_ih | db_ih = dGIs^T [g_s | 1],     dg_s = dGIs W_ih,     the GCN backward on (Xs, g_s, dg_s)
 *
 * The fold sums in ascending w, in fp32, with plain loads and stores (no atomics): the gradients repeat bit for bit.
 *
 * Scope of version 1: exact fp32 (WGNN_MATH_F32) with fp32 I/O, a dense adjacency with S <= 64, F = 13, H <= 128.  Every other
 * combination windgnn.h knows (fp16-plane math modes, CSR, wider GRUs, 16-bit I/O) is refused with WGNN_ERR_UNSUPPORTED before
 * any launch: materialise the windows (wgnn_make_windows) and use windgnn.h for those.  There is no carried state and no
 * fused loss / optimiser tail here; `grads` holds final values when wgnn_series_bwd returns (stream-ordered).
 *
 * Conventions are those of windgnn.h: device pointers owned by the caller, asynchronous on `stream`, negative wgnn_status on
 * failure, every argument validated before any HIP call, workspace / stash 256-byte aligned, the status block in the first
 * WGNN_STATUS_BYTES of the workspace.  wgnn_params.prepared is honoured as in wgnn_fwd / wgnn_bwd (it depends on S and H only).
 *
 * The stash (wgnn_series_stash_bytes), with A64(x) = x rounded up to 64 floats, Ip = 32*ceil((13 S + 1)/32), Gp = 32*ceil(3H/32),
 * hq = 16*ceil((H + 1)/16), holds in this order, in floats:
 *     A64(rows * Ip)                                   g_s: conv2's output of every hour, with its ones column
 *     A64(rows * Gp)                                   GI_s
 *     A64(ceil(n/16) * T * ceil(H/16) * 1024)          the recurrence's gate records (window-major)
 *     A64(big ? n * T * hq : 0)                        the [h_{t-1} | 1] rows of the large dW_hh product (window-major);
 *                                                      big = n*T >= 4096 and Ip <= 512 and Gp <= 512
 * i.e. the two regions wgnn_stash_bytes sizes with B*T rows of S*13 and 3H floats are sized with `rows` rows here.  The
 * workspace holds no window-major copy of Xs, g or GI either: its window-major regions are dGI [n*T][Gp], the n third of dGH
 * (or dGH whole below 4096 rows) and the split-K partial sums of dW_hh.
 */
#ifndef WINDGNN_SERIES_H
#define WINDGNN_SERIES_H

#include "windgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WGNN_SERIES_VERSION 1
int wgnn_series_version(void);

typedef struct wgnn_series_dims {
  int32_t rows;        /* hours in the series */
  int32_t T;           /* window length */
  int32_t stride;      /* hours between the starts of consecutive windows, >= 1 (may exceed T: the rows between are unused) */
  int32_t n;           /* windows, (n-1)*stride + T <= rows */
  int32_t S, F, H;     /* as wgnn_dims: stations, 13, GRU hidden width */
  int32_t math;        /* WGNN_MATH_F32 */
  int32_t adj_format;  /* WGNN_ADJ_DENSE */
  int32_t nnz;         /* unused (0) */
  int32_t io;          /* WGNN_IO_F32 */
} wgnn_series_dims;

/* Bytes of workspace (forward and backward alike) and of the stash; 0 for dims the entry points below refuse. */
size_t wgnn_series_workspace_bytes(const wgnn_series_dims* sd);
size_t wgnn_series_stash_bytes(const wgnn_series_dims* sd);

/* Y [n][T][H] = the model on every window.  stash (nullable: inference) receives what wgnn_series_bwd needs.
 * NULL sd, A, Xs, p (or one of its 8 tensors), Y or workspace: WGNN_ERR_NULL.  rows, T, stride, n, S or H < 1, F != 13,
 * (n-1)*stride + T > rows, or an element count past the limits of windgnn.h: WGNN_ERR_SHAPE.  Outside the scope above:
 * WGNN_ERR_UNSUPPORTED.  workspace_bytes below wgnn_series_workspace_bytes: WGNN_ERR_WORKSPACE. */
int wgnn_series_fwd(const wgnn_series_dims* sd, const float* A, const float* Xs, const wgnn_params* p, float* Y, void* stash,
                    void* workspace, size_t workspace_bytes, void* stream);

/* The rolling backtest: last [n][H] = Y[w][T-1][:] * (wind_max - wind_min) + wind_min, one forecast per window, without
 * writing Y (what wgnn_fwd_last gives on the materialised windows: the last_only form of wgnn_series_fwd's recurrence).
 * Errors as wgnn_series_fwd. */
int wgnn_series_fwd_last(const wgnn_series_dims* sd, const float* A, const float* Xs, const wgnn_params* p, float wind_min,
                         float wind_max, float* last, void* workspace, size_t workspace_bytes, void* stream);

/* grads (all 8, overwritten) = the gradients of sum(Y * dY) over all windows.  Y, stash: as wgnn_series_fwd left them for the
 * same sd, A, Xs and p; dY [n][T][H].  Errors as wgnn_series_fwd, with NULL Y, dY, stash, grads (or one of its 8): WGNN_ERR_NULL. */
int wgnn_series_bwd(const wgnn_series_dims* sd, const float* A, const float* Xs, const wgnn_params* p, const float* Y,
                    const float* dY, const void* stash, const wgnn_grads* grads, void* workspace, size_t workspace_bytes,
                    void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WINDGNN_SERIES_H */
