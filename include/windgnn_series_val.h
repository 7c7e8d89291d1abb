/* windgnn_series_val.h -- series VALIDATION: the loss of a spec {kind, delta, t_from, masked} (windgnn_series_lossfn.h) on windows
 * the model is not training on, forward-only, accumulated on the device over several calls, ending in wgnn_keep_best
 * (windgnn_best.h) and a patience counter.  No Y, no stash, no gate records, no [Hprev | 1] rows and no backward exist.
 *
 *   once            wgnn_val_init
 *   per pass        wgnn_val_begin, wgnn_series_val on every table or segment of the hold-out,
 *                   wgnn_keep_best on (const float*)((char*)val + 28), wgnn_val_close(val, best)
 *   when wanted     read the record's public words (the reference's `if patience > 10: break` is stale > 10)
 *
 * wgnn_series_val runs, in this order, the front end of wgnn_series_fwd on the `rows` rows, the recurrence instance of
 * wgnn_series_fwd_lossfn with last_only = 1 and neither gate records nor [Hprev | 1] rows, and series_val_finish_kernel:
 *
 *     last     [n][H], nullable: Y[w][T-1][:] * (wind_max - wind_min) + wind_min, what wgnn_series_fwd_last gives, bit for bit
 *              (NULL: the rows go to the workspace; the recurrence stores through the pointer unconditionally)
 *     loss     float[1], nullable: the bits wgnn_series_fwd_lossfn + wgnn_series_bwd_lossfn write into loss[0] for the same
 *              inputs and spec -- the per-workgroup partial sums added in BPTT's fixed order (per-thread strided sum, xor tree
 *              over the lanes, the 8 waves ascending), times 1.0f / (float)m with IEEE division.  m is the sum of the forward's
 *              exact integer counts for both values of `masked`; with masked = 0 that sum is n (T - t_from) H, the integer the
 *              training pair forms on the host.  m = 0 (masked = 1 only): NaN and WGNN_STATUS_NO_LABELS.
 *     val      the record below, nullable: this call's partial sums (in fp64, ascending workgroup order, one thread), counts and
 *              maxima are added to it and mean, loss, max_abs and calls are rewritten.  Deterministic: two identical passes give
 *              the same bits.  Calls cut at multiples of 16 windows add the same partial sums as one call, in the same order.
 *
 * A NaN label with masked = 0 poisons the call's loss and the record's sum (loud on purpose, as in training).  loss and val both
 * NULL: WGNN_ERR_NULL (nothing to report).  The finish kernel checks the tag and the spec words of the statistics as the
 * backward does: statistics that are not this spec's forward's give a NaN loss, a NaN record sum and WGNN_STATUS_NO_LOSS_STATS.
 * Status bits (WGNN_STATUS_WINDOW_START, WGNN_STATUS_NO_LABELS, WGNN_STATUS_NO_LOSS_STATS) are ORed into the status word at
 * byte 0 of the workspace: this workspace has no window-major half.
 *
 * Row mappings are wgnn_series_fwd_lossfn's: sd->stride >= 1 with starts == NULL, or sd->stride == 0 with the table, its device
 * check and its clamp; stride >= 1 with a table: WGNN_ERR_SHAPE; stride == 0 without one: WGNN_ERR_NULL.  Scope (exact fp32,
 * fp32 I/O, dense adjacency with S <= 64, F = 13, H <= 128), the order of validation and the error codes are the masked pair's,
 * with the spec last, all before any HIP call: NULL loss and val; the dims; the two forms mixed; NULL sd, A, Xs, p (or one of its
 * 8 tensors), Ls, workspace, fn's table; a val that is not 256-byte aligned (WGNN_ERR_SHAPE); ls_rows; workspace_bytes; the spec.
 *
 * The workspace: wgnn_series_val_workspace_bytes(sd) covers the front end on `rows` rows without a stash, GI_s, the statistics
 * (wgnn_series_lossfn_bytes(sd)) and n * H floats for the last rows when the caller passes none.  It holds no window-major
 * region of n * T rows.
 *
 * `val`, the record, is one more caller-kept device buffer of wgnn_val_bytes() bytes, 256-byte aligned.  Its first bytes are
 * PUBLIC:
 *     offset  0  double   sum        sum of rho over the open pass
 *     offset  8  uint64   count      m over the open pass
 *     offset 16  double   mean       sum / count, NaN while count = 0
 *     offset 24  float    max_abs    the largest |r| of the open pass
 *     offset 28  float    loss       (float)mean: the word wgnn_keep_best is pointed at
 *     offset 32  int64    calls      wgnn_series_val calls in the open pass
 *     offset 40  int64    passes     closed passes
 *     offset 48  int64    stale      closed passes since the last one that won
 * Everything behind them is private.  No byte outside [val, val + wgnn_val_bytes()) is written through it.
 *
 * Under a process group nothing is exchanged: every rank validates the same tables, gets the same bits and takes the same
 * decision.  Not here: the materialised path, the fp16-plane modes, a hold-out sharded over ranks, per-station or per-horizon
 * breakdowns (windgnn_eval.h gives those), a recurrence instance that writes no last rows at all.
 */
#ifndef WINDGNN_SERIES_VAL_H
#define WINDGNN_SERIES_VAL_H

#include "windgnn_best.h"
#include "windgnn_series_lossfn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WGNN_SERIES_VAL_VERSION 1
int wgnn_series_val_version(void);

/* Bytes of the record: a multiple of 256. */
size_t wgnn_val_bytes(void);

/* Writes every byte of the record (it may be dirty): sum, count, max_abs, calls, passes and stale 0, mean and loss NaN.  One small
 * launch.  NULL val: WGNN_ERR_NULL. */
int wgnn_val_init(void* val, void* stream);

/* Opens a pass: sum, count, max_abs and calls 0, mean and loss NaN; passes and stale stay.  NULL val: WGNN_ERR_NULL. */
int wgnn_val_begin(void* val, void* stream);

/* Bytes of workspace of wgnn_series_val (above); 0 for dims it refuses.  stride = 0 selects the table's dims. */
size_t wgnn_series_val_workspace_bytes(const wgnn_series_dims* sd);

int wgnn_series_val(const wgnn_series_dims* sd, const float* A, const float* Xs, const int32_t* starts, const wgnn_params* p,
                    const float* Ls, int64_t ls_rows, const wgnn_lossfn* fn, float wind_min, float wind_max, float* last,
                    float* loss, void* val, void* workspace, size_t workspace_bytes, void* stream);

/* Ends the pass: passes += 1.  best (nullable): a record of windgnn_best.h on which the caller has just run wgnn_keep_best with
 * the loss word of val; stale = (the public int32 `improved` at its offset 32) ? 0 : stale + 1.  best == NULL: stale is left
 * alone.  NULL val: WGNN_ERR_NULL. */
int wgnn_val_close(void* val, const void* best, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WINDGNN_SERIES_VAL_H */
