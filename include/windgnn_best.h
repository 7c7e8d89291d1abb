/* windgnn_best.h — checkpoint-side additions to the C ABI of libwindgnn_hip.so: the reference's "keep the best model" rule
 * (src/main.py:83-86) applied on the device, with no host synchronisation.
 *
 *     if loss.item() < best_loss:
 *         torch.save(model.state_dict(), PATH)
 *         best_loss = loss.item()
 *
 * needs float(loss) -- a full device synchronisation -- and a host-driven copy of the parameters on every step.  The pair
 * below keeps best_loss in a small device record and the saved state_dict in a second, caller-owned set of the 8 tensors:
 *
 *   once          wgnn_best_init
 *   per step      .., wgnn_finish (the optimiser step), wgnn_keep_best(loss word, p, best_p, step)
 *   when wanted   read the record's public words / copy best_p out (the only host reads)
 *
 * Order, as in the reference: the loss of the forward BEFORE the update decides, and the parameters AFTER optimizer.step() are
 * what is kept (src/main.py:66-86), so the call follows the optimiser's launch on the same stream.  Under data parallel the
 * loss word is the all-reduced big-batch mean on every rank: every rank takes the same decision without another collective.
 *
 * Conventions are those of windgnn.h (device pointers owned by the caller, asynchronous on `stream`, negative wgnn_status on
 * refusal, arguments validated before any launch).
 *
 * `best`, the record, is one more caller-kept device buffer of wgnn_best_bytes() bytes, 256-byte aligned.  Its first bytes are
 * PUBLIC:
 *     offset  0  double   best_loss      the threshold, then the smallest winning loss
 *     offset  8  int64    best_step      `step` of the last winning call; -1: none yet
 *     offset 16  int64    calls          wgnn_keep_best calls since wgnn_best_init
 *     offset 24  int64    improvements   winning calls among them
 *     offset 32  int32    improved       1 if the last call won, else 0
 * Everything behind them is private.  No byte outside [best, best + wgnn_best_bytes()) and the 8 tensors of best_p is
 * written.
 */
#ifndef WINDGNN_BEST_H
#define WINDGNN_BEST_H

#include "windgnn.h"

#ifdef __cplusplus
extern "C" {
#endif

#define WGNN_BEST_VERSION 1
int wgnn_best_version(void);

/* Bytes of the record: a multiple of 256. */
size_t wgnn_best_bytes(void);

/* Writes every byte of the record (it may be dirty): best_loss = threshold, best_step = -1, the counters and the flag 0.
 * threshold: the reference's best_loss = 0.03 (src/main.py:60); +inf = the first finite loss wins.  One small launch.
 * NULL best: WGNN_ERR_NULL.  A NaN threshold: WGNN_ERR_SHAPE. */
int wgnn_best_init(void* best, double threshold, void* stream);

/* The rule: if (double)*loss < best_loss, copy the 8 tensors of p into the 8 tensors of best_p, then best_loss = (double)*loss
 * and best_step = step.  The comparison is fp64 against the fp64 record, as Python's `loss.item() < 0.03` is: a loss equal to
 * float32(0.03) = 0.029999999329... wins against the threshold 0.03, which an fp32 comparison would deny.  A NaN loss never
 * wins.  When the loss does not win, no byte of best_p is written.  calls, improvements and improved follow either way.
 * Tensor sizes come from d (F*F, F, F*F, F, 3H*S*F, 3H*H, 3H, 3H floats, the state_dict order of wgnn_params); p->prepared
 * and best_p->prepared are ignored.  Tensors need the alignment of a float only, and source and destination may sit at
 * different offsets inside 16 bytes (the copy then moves single floats).
 * Two launches: one thread decides and rewrites the record; the copy, one launch for all 8 tensors with a grid sized to the
 * chip, reads the published flag, and a workgroup that finds it 0 returns after that one word.
 * NULL d, loss, p, best_p or best, or an empty tensor slot in p or best_p: WGNN_ERR_NULL.  Dims that wgnn_workspace_bytes
 * refuses, step < 0, or a tensor of best_p that overlaps a tensor of p: WGNN_ERR_SHAPE. */
int wgnn_keep_best(const wgnn_dims* d, const float* loss, const wgnn_params* p, const wgnn_params* best_p, int64_t step,
                   void* best, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* WINDGNN_BEST_H */
