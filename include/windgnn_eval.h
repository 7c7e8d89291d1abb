/* windgnn_eval.h — evaluation-side additions to the C ABI of libwindgnn_hip.so: the statistics of the reference's test loop
 * (src/main.py:100-157) accumulated on the device, window batch by window batch, with no host synchronisation.
 *
 * The reference keeps three Python lists of every prediction, truth and absolute error (one .detach().cpu().numpy() per
 * window) and, after the loop, forms four figures per station and horizon: RMSE, MAE, and the mean and the (population)
 * standard deviation of the "accuracy" 1 - |err| / truth.  All four are functions of five plain sums per column, so the
 * pair below keeps those sums on the device, in fp64, and turns them into the figures in one small launch at the end:
 *
 *   per batch    wgnn_fwd_last (or wgnn_predict_last), wgnn_eval_accum
 *   at the end   [data parallel: one SUM all-reduce of the 5*H doubles of the header] wgnn_eval_stats
 *
 * Conventions are those of windgnn.h (device pointers owned by the caller, asynchronous on `stream`, negative wgnn_status on
 * failure, arguments validated before any HIP call).  H = 3S columns: column k*S + s is station s at horizon +(k+1) h.
 *
 * `acc`, the accumulator, is one more caller-kept device buffer of wgnn_eval_bytes(H) bytes, 256-byte aligned.  An all-zero
 * buffer is the empty accumulator; reset is the caller's hipMemsetAsync.  It begins with a PUBLIC header of five fp64 rows
 * of length H, in this order:
 *     n        windows seen
 *     Σe²      e = truth - pred
 *     Σ|e|
 *     Σa       a = 1 - |e| / truth
 *     Σa²
 * Plain sums on purpose: two accumulators are merged by adding their headers.  Everything behind the header is private
 * scratch (it may be dirty; every byte of it that a call reads, that call has written).  No byte outside
 * [acc, acc + wgnn_eval_bytes(H)) and the stated extents of abs_err / out is touched.
 */
#ifndef WINDGNN_EVAL_H
#define WINDGNN_EVAL_H

#include "windgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WGNN_EVAL_VERSION 1
int wgnn_eval_version(void);

/* Bytes of `acc`: the 5*H doubles of the header plus the private per-slice partial sums of the widest wgnn_eval_accum launch,
 * rounded up to 256.  Depends on H only; 0 for H < 1. */
size_t wgnn_eval_bytes(int32_t H);

/* Adds one batch of windows to `acc`.  pred [B][H] fp32, de-normalised: what wgnn_fwd_last / wgnn_predict_last write.
 * labels [B][T][H] fp32, normalised (the loader's batch_y); only row T-1 of every window is read.  For every window b and
 * column c, in fp64 throughout (the reference's wind_min / wind_max are float64, so src/main.py:103-105 promotes):
 *     truth = (double)labels[b][T-1][c] * ((double)wind_max - (double)wind_min) + (double)wind_min
 *     e     = truth - (double)pred[b][c]
 *     a     = 1 - |e| / truth
 * and 1, e², |e|, a, a² are added to the five header rows of column c.  abs_err (nullable) [B][H] fp32 receives (float)|e|:
 * the rows of the reference's box plots.  The division is IEEE (no fast-math, no contraction): a zero truth makes that column's
 * Σa and Σa² non-finite exactly as numpy's would, and leaves every other column untouched.
 * Deterministic: every column has one owner per launch and every sum a fixed order (no floating-point atomics); the same
 * calls on the same acc give the same bytes.  One launch for small B; for many windows on few columns the windows are sliced
 * over workgroups into private fp64 partials that a second launch folds in slice order (wgnn_finish_norm's shape).
 * NULL pred, labels or acc: WGNN_ERR_NULL.  B, T or H < 1: WGNN_ERR_SHAPE. */
int wgnn_eval_accum(const float* pred, const float* labels, int32_t B, int32_t T, int32_t H, float wind_min, float wind_max,
                    void* acc, float* abs_err, void* stream);

/* out [H][4] fp32, per column: sqrt(Σe²/n), Σ|e|/n, Σa/n, sqrt(max(Σa²/n - (Σa/n)², 0)) -- RMSE, MAE, the mean and the
 * population standard deviation (np.std) of the accuracy; formed in fp64 and rounded once.  n = 0 gives NaN in all four; a NaN
 * variance stays NaN.  Reads the header of acc only (a merged copy of 5*H doubles will do).  One small launch.
 * NULL acc or out: WGNN_ERR_NULL.  H < 1: WGNN_ERR_SHAPE. */
int wgnn_eval_stats(const void* acc, int32_t H, float* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WINDGNN_EVAL_H */
