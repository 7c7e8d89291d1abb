"""Host-side mirror of the reference's training-loop body (src/main.py:64-80) on flat buffers:
forward -> MSE + backward (wgnn_bwd_mse_part) -> (data-parallel all-reduce) -> Adam, every op a C-ABI call.

Data parallel: windows are independent, so each rank runs its own shard of
windows; the 8 gradients live in ONE flat fp32 bucket (167 440 floats at S=34).  Per step the bucket is summed by ONE
all-reduce of [loss | conv gradients | GRU gradients] (0.67 MB) between the reduce-only wgnn_finish(6) and the optimiser's
wgnn_finish(0, adam).  (Round 3 measured the alternative it replaced -- two all-reduces, the GRU gradients' one started
asynchronously after the weight-gradient GEMMs and overlapped with the dg GEMM + GCN backward -- on a one-rank group, where the
collectives themselves cost nothing: +65 us per 632 us step for its cross-stream dependencies and extra launches against +10 us
for this form; `overlap_collectives=True` still selects it.)  dY is pre-scaled by n_local / n_global (= 1 / world_size for
equal shards) so the summed bucket equals the gradient of the big-batch mean loss, and the returned loss is the big-batch mean
loss on every rank.  The collectives themselves live in distributed.BucketExchange (every rank issues every collective on
every step).

Schedules: how the backward's parts, the collectives and the optimiser's launches of a step are ordered -- one rank, one
bucket, two collectives (`overlap_collectives`), blocked (`grad_blocks`) -- is written once, in TrainStep._run_schedule.  A step
kind hands it what it enqueues: the plain and the carried-state step their deferred backward parts (_Deferred), the empty-shard
and the series step a bucket that is final already (_FINAL), for which the same orderings reduce to the collectives and Adam.

The loss a step returns is a 0-dim VIEW of the bucket's header (no clone launch per step): read it (float(loss)) or
`.clone()` it before the next step -- a list of kept losses would all show the latest value.

A rank whose shard is EMPTY (fewer windows than ranks) still issues every collective of the step, in every schedule: it
contributes a zero bucket and runs the optimiser's launch(es) on the summed gradient, so no rank is left waiting in an all-reduce.

Blocked exchange (`grad_blocks`, opt-in, for buckets of GB: BASELINE configs[4] has 9.66 GB): the weight-gradient GEMMs run
per row block of w_ih, then of w_hh (wgnn_bwd_rows), and each block's all-reduce starts as soon as its rows are final, so the
exchange runs under the remaining blocks' GEMMs and under part 2; the tail [loss | conv | b_ih | b_hh] follows part 2, and
Adam runs per block (wgnn_finish_rows) once the tail -- which holds the biases every block's Adam reads -- and the block have
arrived.  HAZARD: part 2 (dg = dGI W_ih, through the staged W_ih^T image) reads the OLD weights, and wgnn_finish_rows
rewrites W_ih and its images in place: every block's Adam must be enqueued after part 2.  One enqueued earlier gives a wrong
dg -- and wrong conv gradients -- without any error (tests/test_gpu_grad_blocks.py shows the difference).  With one rank the
blocked step is the one-bucket step bit for bit.

A step that RAISES (a refused launch, a failed collective) leaves the optimiser state undefined: `steps` counts completed
steps only, but in the two-collective form the GRU tensors and their moments may already have been stepped when a later
launch of the same step fails, and a retry would then apply the same bias-correction step number to them twice.  Do not
retry a failed step on the same TrainStep: rebuild it from a checkpoint of the parameters (state_dict) instead.

Clipping (`max_grad_norm`, opt-in): where the reference loop would call torch.nn.utils.clip_grad_norm_ between loss.backward()
and optimizer.step(), the optimiser's wgnn_finish becomes wgnn_finish_norm + wgnn_finish_clipped (include/windgnn_optim.h): the
global L2 norm of the 8 gradients and min(1, max_grad_norm / (norm + 1e-6)) are formed on the device, and Adam reads
g * coefficient.  One rank: the norm is taken in the launch that reduces the deferred partial sums.  Data parallel: after the
all-reduce, over the summed bucket -- which is the same on every rank, and the norm's summation order is fixed, so every rank
derives the same coefficient without another collective.  The bucket keeps the UNCLIPPED gradient (torch clips .grad in place);
`grad_norm` and `clip_coef` are views of the device values, overwritten by the next step like the loss.

Best model (`keep_best`, opt-in): the reference keeps the parameters of its best step, src/main.py:83-86
(`if loss.item() < best_loss: torch.save(model.state_dict(), PATH); best_loss = loss.item()`), which costs a device
synchronisation and a host-driven copy per step.  With keep_best set every successful step ends with wgnn_keep_best
(include/windgnn_best.h): the comparison (fp64, as Python's), best_loss / best_step and the copy of the 8 tensors into a second
flat buffer all happen on the device.  The order is the reference's: the loss of the forward BEFORE the update decides, and the
parameters AFTER optimizer.step() are what is kept (src/main.py:66-86), so the call follows the optimiser's launches of every
schedule and carries step = `steps` after the increment.  Under data parallel the loss word is the all-reduced big-batch mean
on every rank, so every rank takes the same decision without another collective.  `best_loss`, `best_step` and `improved`
are views of the device record; best_state_dict() / restore_best() read the snapshot.

Checkpoints: state_dict() / load_state_dict() carry what a TrainStep owns besides the parameters -- the Adam moments and step
count in torch.optim.Adam's own layout (so a run can move between torch.optim.Adam on the drop-in module and TrainStep), the
best record and snapshot, and the carried GRU state.  The parameters travel through model.state_dict() as before.

Series mode (step_series / forward_backward_series; include/windgnn_series_train.h): the same step on the sliding windows of ONE
hourly series, without materialising windows, labels or dY.  The label of window w at step t is row w * stride + t of the label
series Ls (series.series_labels' first result), which the recurrence kernels read beside the GI row: wgnn_series_fwd_loss leaves
the MSE partial sums in a small buffer, wgnn_series_bwd_mse forms dY inside BPTT, finalises the loss into the bucket's header
word and leaves FINAL gradients in the bucket (series mode does not defer its partial sums), so the schedule runs on _FINAL:
its tail is one wgnn_finish(0, adam) that only steps Adam and refreshes the W_ih images.  With a process group the one
all-reduce sits between the backward and that tail.  Exact fp32, a dense adjacency, the one-bucket schedules; the rest is refused with the alternative.

Validation (validate_series; include/windgnn_series_val.h): the loss of step_series' spec on windows the model is not training
on, forward-only (wgnn_series_val: no Y, no stash, no backward) and accumulated over calls in a device record.  With
TrainStep(keep_best=..., best_on="validation") no training step decides on the best model; a closed validation pass does --
wgnn_keep_best on the record's loss word, then wgnn_val_close, which keeps the patience counter `val_stale`.  Nothing is
exchanged under a process group: every rank validates the same tables and takes the same decision.  No host read anywhere.
validate is the same pass on materialised windows, for what series mode refuses (the fp16-plane modes, 16-bit I/O, a CSR
adjacency, the wide-GRU path, the reference's own test_loader): the stash-less forward, the loss terms in fp64 torch operations on
the device (functional.validation_terms) and the record's public words updated by functional.val_add.

Loss specs on materialised windows (step / forward_backward with loss= / huber_delta= / loss_from= / missing_labels=): the loss
validate scores, trained on, in every math mode, adjacency format, I/O type and width.  At the defaults the step is the fused MSE
step above, call for call.  Any other spec: the forward runs without labels (wgnn_fwd), functional.loss_spec_grad forms the loss
(into the bucket's header word) and dY from Y and L with torch's own fused loss kernels, and the backward takes that dY through
wgnn_bwd_part (wgnn_bwd_state_part with carry_state) with its parts deferred -- the route the carried-state step has always
taken with wgnn_mse_loss_grad's dY -- so every schedule, clipping, keep_best and the checkpoints see it unchanged.  No kernel
and no entry point of the library is added; the price is one pass over Y and L that the fused step does not have.  With fp16 /
bf16 windows such a step runs on fp32 copies of X and L (_spec_forward), so that the loss is formed from the unrounded Y.
`loss_count` is the step's count of labels.  Under a process group missing_labels=True is refused (the ranks' label counts
would have to be exchanged); the other specs count the same (T - loss_from) * H entries per window on every rank.

Accumulation (accumulate / accumulate_series / apply / discard): one optimiser step that sees several calls -- several series
tensors, materialised and series windows mixed, or k calls per all-reduce under data parallel (DistributedDataParallel's no_sync).
accumulate* is forward_backward* (a FINAL bucket at grad_scale 1) followed by one fused multiply-add of the bucket, header
included, onto a second buffer of its size, weighted by the call's count of labels over the first call's (accumulate.py); apply
scales the sum back into the bucket -- which is then the bucket of one call on the union of the windows, loss word included --
and runs the tail every step runs on a final bucket (_run_schedule(d, _FINAL, gs), _end_step): one all-reduce under a process
group, one wgnn_finish(0, adam) or the clipped pair, keep_best on the accumulated loss.  No kernel and no entry point of the
library is added: the add and the scale are plain torch on the current stream, without a host read.  accumulate* issues no
collective.  A TrainStep that never calls them is the object it was, launch for launch.

Frozen parameter groups (trainable= / set_trainable): "gru" trains the four GRU tensors under frozen convolutions (a trained model
moved to another station network: transfer.adopt_convs), "conv" the four conv tensors under a frozen GRU, "all" -- the default -- is
every schedule above, launch for launch.  wgnn_bwd*_part already splits the backward (include/windgnn.h: part 1 BPTT, part 4 the
weight-gradient GEMMs = the GRU gradients, part 2 the dg GEMM + GCN backward = the conv gradients; 4 and 2 read only what 1 wrote) and
wgnn_finish(WGNN_FINISH_ADAM_GRU | _CONV) steps one group alone, so a step with a frozen group enqueues part 1 and the trained
group's part only, the reduce-only wgnn_finish of that part, (the one all-reduce of the whole bucket,) and the optimiser's launch
of that group: the frozen group's part is never launched and its slots of the bucket keep the zeros set_trainable wrote.  Series
mode has no parts: its backward runs whole and the frozen slots are zeroed after it.  Adam keeps torch.optim.Adam's rule that a
tensor without a gradient does not advance its step: `steps` counts optimiser steps, _sat_out how many of them each group was
frozen for, and a group's bias-correction step is the difference + 1; "all" with unequal counts issues one optimiser launch per
group.  No kernel and no entry point of the library is added."""
from __future__ import annotations

import collections

import torch

from . import _lib
from .accumulate import Accumulation
from .distributed import HEADER, LOSS_SLOT, BucketExchange, grad_block_plan
from .functional import (PARAM_ORDER, _forward_setup, _require_gpu, best_bytes, best_init, best_word, bwd_rows, check_range_status,
                         clip_buffer, clip_bytes, finish_clipped, finish_norm, finish_rows, finish_step,
                         gcn_gru_backward_mse_raw, gcn_gru_backward_raw, gcn_gru_forward_last_raw, gcn_gru_forward_raw,
                         gcn_gru_state_backward_raw, gcn_gru_state_forward_raw, keep_best_args, keep_best_launch, loss_spec_grad,
                         mse_loss_grad, prepared_weights,
                         refresh_prepared, rows_align, val_add, val_begin, val_buffer, val_close, val_init, val_word,
                         validation_spec, validation_terms)
from .modules import GCN_GRU
from .series import (_compact_arg, _no_stride_with_starts, _starts_table, compacted_starts, loss_spec, n_series_windows,
                     series_backward_mse_raw, series_forward_loss_raw, series_val_raw, val_spec)

AUTO_GRAD_BLOCKS = 8                # grad_blocks="auto": row blocks per GRU weight ...
AUTO_BLOCK_BYTES = 64 << 20         # ... from a gradient bucket of this size (smaller ones are latency-bound: one bucket)


_ROWS = {"ih": _lib.ROWS_IH, "hh": _lib.ROWS_HH}          # GradBlock.tensor -> `which` of wgnn_bwd_rows / wgnn_finish_rows

# trainable=: the group that trains -> (the part of the backward whose products are its gradients, which is also the reduce bit
# of wgnn_finish for them; the `which` of its optimiser step; the group that is frozen meanwhile)
TRAINABLE = ("all", "gru", "conv")
_GROUP = {"gru": (4, _lib.FINISH_ADAM_GRU, "conv"), "conv": (2, _lib.FINISH_ADAM_CONV, "gru")}


class _Deferred:
    """The backward of a step as its schedule enqueues it (TrainStep._run_schedule): parts of the backward with their
    split-K partial sums left deferred, the reduce-only wgnn_finish of those, and the blocked exchange's weight gradients per
    row block.  `parts(mask)` is the step kind's own: it enqueues the parts in `mask` (1 BPTT, 2 dg + GCN, 4 weight gradients)
    with WGNN_BWD_DEFER through its entry point (wgnn_bwd_mse_part or wgnn_bwd_state_part)."""
    pending = 6                     # what the optimiser's wgnn_finish still has to reduce when nothing else did: parts 2 | 4

    def __init__(self, tr, d, parts, Y, stash):
        self.tr, self.d, self.parts, self.Y, self.stash = tr, d, parts, Y, stash

    def reduce(self, which):
        finish_step(self.d, self.tr.p_views, self.tr.g_views, which, device=self.tr.device)

    def rows(self, b):
        bwd_rows(self.d, self.Y, self.stash, self.tr.g_views, _ROWS[b.tensor], b.row0, b.rows, self.tr.device)


class _Final:
    """The same for a bucket that is final before the schedule starts -- an empty shard's zeros, series mode's
    wgnn_series_bwd_mse (which reduces its own partial sums): nothing to enqueue and nothing to reduce."""
    pending = 0

    def parts(self, mask):
        pass

    def reduce(self, which):
        pass

    def rows(self, b):
        pass


_FINAL = _Final()


class TrainStep:
    # A step with a frozen group leaves the split-K partial sums of its one part deferred (WGNN_BWD_DEFER) and reduces them
    # with a reduce-only wgnn_finish, as the one-bucket schedule does; False: the part reduces its own.  Both are legal
    # (include/windgnn.h) and give the same bits; profiles/r23_finetune_cost.txt has the two timings behind the choice.
    FROZEN_DEFER = True

    def __init__(self, model: GCN_GRU, lr: float = 1e-3, betas=(0.9, 0.999), eps: float = 1e-8,
                 process_group=None, check_every: int = 100, overlap_collectives: bool = False, direct_rccl=None,
                 rccl_loader=None, carry_state: bool = False, grad_blocks=None, max_grad_norm=None, keep_best=None,
                 best_on: str = "train", trainable: str = "all"):
        """carry_state: truncated BPTT over consecutive chunks -- each step starts the recurrence from the h_n of the previous
        step (detached; zeros on the first step and after reset_state()), so a model trained on chunks of a long series
        learns the carried-state regime StreamingForecaster(window=None) serves.  The batch size must stay the same
        between resets; fp32 I/O only.

        grad_blocks (with a process group): None = the schedules above; an int k = the blocked exchange, the wider of w_ih
        and w_hh cut into up to k row blocks (multiples of wgnn_bwd_rows_align), the other into about as large ones
        (distributed.grad_block_plan), each block's all-reduce started as soon as its weight-gradient GEMM is done (module
        docstring); "auto" = k = AUTO_GRAD_BLOCKS when the bucket reaches
        AUTO_BLOCK_BYTES and the shape has the row-range entry points, else None.  Not with carry_state,
        overlap_collectives or direct_rccl.

        max_grad_norm: None = no clipping (the schedules above, launch for launch); a value > 0 = clip the step's gradient
        by its global L2 norm as torch.nn.utils.clip_grad_norm_(parameters, max_grad_norm) would before the optimiser step
        (module docstring); float("inf") = measure only (`grad_norm`), nothing is scaled.  Not with overlap_collectives or
        the blocked exchange, which step tensors before the whole bucket has arrived.

        keep_best: None = off (no buffer, no launch: the schedules above, launch for launch); True = keep the parameters of
        the step with the smallest loss so far (threshold +inf: the first finite loss wins); a float = keep them only once
        the loss falls below it (0.03 is the reference's initial best_loss, src/main.py:60).  As in the reference the loss
        of the forward BEFORE the update decides and the parameters AFTER the optimiser step are kept (module docstring).
        Every schedule takes it, the empty-shard step included.

        best_on (with keep_best): "train" = the rule above, launch for launch; "validation" = no step decides -- a CLOSED
        validation pass does (validate_series or validate): its held-out loss is compared, and the parameters at that moment are kept.

        trainable: "all" = every schedule above, launch for launch; "gru" = the four GRU tensors train and the four conv tensors
        are frozen; "conv" = the mirror image (set_trainable has the contract).  Under a process group every rank must hold
        the same value: nothing checks it, and no collective is added for it."""
        if not getattr(model, "fused", True):
            raise RuntimeError("windgnn_amd: TrainStep drives the fused hot path, i.e. the reference model's own widths "
                               "(input_dim = hidden_dim = 13, src/main.py:41); a GCN_GRU of other widths trains through "
                               "autograd (loss.backward() + torch.optim.Adam, as src/main.py:66-80 does)")
        self.model = model
        self.params = list(model.hot_path_parameters())
        sizes = [p.numel() for p in self.params]
        dev = self.params[0].device
        self.flat_p = torch.cat([p.detach().reshape(-1) for p in self.params]).contiguous()
        self.group = process_group
        self.world = 1
        if process_group is not None or (torch.distributed.is_available() and torch.distributed.is_initialized()):
            self.world = torch.distributed.get_world_size(process_group)
        # an explicitly passed group runs the collective path even with one rank (the all-reduces execute)
        self.collective = self.world > 1 or process_group is not None
        self.plan = self._grad_block_plan(grad_blocks, sizes, carry_state, overlap_collectives, direct_rccl)
        if max_grad_norm is not None:
            max_grad_norm = float(max_grad_norm)
            if not max_grad_norm > 0.0:                   # (NaN fails the comparison)
                raise ValueError("windgnn_amd: max_grad_norm must be > 0 (float('inf') = measure only) or None, got %r"
                                 % (max_grad_norm,))
            if overlap_collectives or self.plan is not None:
                raise RuntimeError("windgnn_amd: TrainStep(max_grad_norm=%r) with %s: that schedule steps %s before the "
                                   "whole gradient bucket has arrived, and the global norm needs all of it; clipping runs "
                                   "with the one-bucket schedules only"
                                   % (max_grad_norm, "overlap_collectives=True" if overlap_collectives
                                      else "grad_blocks=%r" % (grad_blocks,),
                                      "the GRU tensors" if overlap_collectives else "row blocks"))
        self.max_grad_norm = max_grad_norm
        self.overlap_collectives = overlap_collectives
        # completed optimiser steps that each group sat out frozen: a group's own count, which is Adam's bias-correction
        # step number for it less one, is `steps` minus this (torch.optim.Adam: no gradient, no step)
        self._sat_out = {"gru": 0, "conv": 0}
        self.trainable = self._trainable_arg("TrainStep(trainable=%r)" % (trainable,), trainable)
        if keep_best is False:                          # off, as a user means it (not the threshold 0.0)
            keep_best = None
        if keep_best is not None:
            keep_best = float("inf") if keep_best is True else float(keep_best)
            if keep_best != keep_best:
                raise ValueError("windgnn_amd: keep_best must be None, True or a loss threshold, got NaN")
        self.keep_best = keep_best
        if best_on not in ("train", "validation"):
            raise ValueError("windgnn_amd: TrainStep(best_on=%r): 'train' (the loss of every step decides) or 'validation' (the "
                             "loss of every closed validate_series pass does)" % (best_on,))
        if best_on == "validation" and keep_best is None:
            raise ValueError("windgnn_amd: TrainStep(best_on='validation') needs keep_best (True, or a loss threshold): without it "
                             "there is no record and no snapshot for a validation pass to decide on")
        self.best_on = best_on
        self._val, self._val_open, self._val_best_call = None, False, None     # the validation record: made by the first pass
        self._clip = None               # wgnn_finish_norm's buffer: sized at the first clipped step (wgnn_clip_bytes needs its dims)
        # gradient bucket with a 4-float header (16-byte aligned bucket): header[3] = the step's loss, so that the loss
        # rides in the conv-gradient all-reduce (the conv gradients are the first 364 floats of the bucket).  The blocked
        # exchange lays it out as its plan says: [header | conv | b_ih | b_hh | w_ih | w_hh]
        if self.plan is None:
            self._gbuf = torch.zeros(self.flat_p.numel() + HEADER, dtype=torch.float32, device=dev)
            g_split = self._gbuf[HEADER:].split(sizes)
        else:
            self._gbuf = torch.zeros(self.plan.numel, dtype=torch.float32, device=dev)
            g_split = [self._gbuf[o:o + n] for o, n in self.plan.slots]
        self.flat_g = self._gbuf[HEADER:]
        self._loss = self._gbuf[LOSS_SLOT]
        self.exp_avg = torch.zeros_like(self.flat_p)
        self.exp_avg_sq = torch.zeros_like(self.flat_p)
        self.p_views, self.g_views = [], []
        for p, pv, gv in zip(self.params, self.flat_p.split(sizes), g_split):
            p.data = pv.view_as(p)              # parameters become views of the flat bucket
            p.grad = gv.view_as(p)
            self.p_views.append(p.data)
            self.g_views.append(p.grad)
        self.m_views = [t.view_as(p) for t, p in zip(self.exp_avg.split(sizes), self.params)]
        self.v_views = [t.view_as(p) for t, p in zip(self.exp_avg_sq.split(sizes), self.params)]
        # the staged images of W_ih (wgnn_params.prepared): built once, then kept current by wgnn_finish's Adam; rebuilt
        # when someone else wrote the parameters (load_state_dict, p.data.copy_, ...: torch's version counter tells)
        self._prepared, self._prepared_version = None, None
        self.n_conv = sum(sizes[:4])
        self.lr, self.betas, self.eps = lr, betas, eps
        self.steps = 0
        # keep_best: the snapshot (one more flat buffer, the 8 tensors at flat_p's offsets) and the device record
        self._best = self._best_p = self._best_views = self._best_dims = self._best_call = None
        if keep_best is not None:
            self._best_p = torch.zeros_like(self.flat_p)
            self._best_views = [t.view_as(p) for t, p in zip(self._best_p.split(sizes), self.params)]
            self._best = torch.zeros(best_bytes(), dtype=torch.uint8, device=dev)
            # sizes the 8 tensors for wgnn_keep_best (S, H and F only: B, T, the adjacency and the math mode do not enter)
            self._best_dims = _lib.Dims(1, 1, self.params[4].shape[1] // 13, 13, self.params[5].shape[1], _lib.MATH_F32,
                                        _lib.ADJ_CSR, 1, _lib.IO_F32)
            self._reset_best(keep_best)
            # the call's arguments but the step number: the views never move, so they are checked and marshalled once
            self._best_call = keep_best_args(self._best_dims, self._loss, self.p_views, self._best_views, self._best)
        # direct_rccl: None = only if WGNN_RCCL_DIRECT=1 (opt-in: distributed.DirectRccl); the two-collective form overlaps
        # through torch.distributed's own stream by design and never takes it
        self.exchange = None
        if self.collective:
            self.exchange = BucketExchange(self._gbuf, self.n_conv, process_group,
                                           False if ((overlap_collectives or self.plan is not None) and direct_rccl is None)
                                           else direct_rccl, rccl_loader)
        self.check_every = check_every          # f16x3 / f16: read the library's range-status word every N steps
        self.device = dev
        # carried state: two [B, H] buffers (h0 of this step, h_n into the other: they may not alias), swapped per step
        self.carry_state = carry_state
        self._hbuf, self._hcur, self._has_state = None, 0, False
        self._count = None              # loss_count: made by the first step on a loss spec
        # accumulate / accumulate_series: the accumulator (one more buffer of the bucket's size, made by the first call and
        # reused), what the open accumulation's calls must share, the tail's dims and this rank's windows so far
        self._acc, self._acc_spec, self._acc_d, self._acc_windows = None, None, None, 0

    def _grad_block_plan(self, grad_blocks, sizes, carry_state, overlap_collectives, direct_rccl):
        """The blocked exchange's plan (distributed.grad_block_plan), or None for the one-bucket schedules."""
        if grad_blocks is None:
            return None
        if isinstance(grad_blocks, str) and grad_blocks != "auto":
            raise ValueError("windgnn_amd: grad_blocks must be None, an int >= 1 or 'auto', got %r" % (grad_blocks,))
        why = None
        if not self.collective:
            why = "it needs a process group (it blocks the gradient all-reduce)"
        elif carry_state:
            why = "the carried-state step (carry_state=True) keeps the one-bucket schedule"
        elif overlap_collectives:
            why = "overlap_collectives=True is another schedule of the same collectives"
        elif direct_rccl:
            why = "direct_rccl enqueues the all-reduce on the compute stream, so nothing could overlap it"
        if why is not None:
            raise RuntimeError("windgnn_amd: TrainStep(grad_blocks=%r): %s" % (grad_blocks, why))
        S, H = self.params[4].shape[1] // 13, self.params[5].shape[1]
        math = self.model.math
        align = rows_align(_lib.Dims(1, 1, S, 13, H, math, _lib.ADJ_CSR, 1, _lib.IO_F32))
        if grad_blocks == "auto":
            if align == 0 or 4 * sum(sizes) < AUTO_BLOCK_BYTES:
                return None
            grad_blocks = AUTO_GRAD_BLOCKS
        elif align == 0:
            raise RuntimeError("windgnn_amd: TrainStep(grad_blocks=%r): the row-range weight gradients (wgnn_bwd_rows) "
                               "need the wide-GRU path (H > 127 in f16x3 / f16x3g, H > 128 in f32; not the f16 mode), got "
                               "H = %d, math = %d" % (grad_blocks, H, math))
        return grad_block_plan(S, H, grad_blocks, align)

    def _trainable_arg(self, who, group):
        """trainable= of the constructor and set_trainable: the group, or the refusal by name, before any launch."""
        if group not in TRAINABLE:
            raise ValueError("windgnn_amd: %s: trainable is 'all', 'gru' (the four GRU tensors train, the convolutions are frozen) "
                             "or 'conv' (the four conv tensors train, the GRU is frozen), got %r" % (who, group))
        why = None
        if group == "all":
            pass
        elif self.max_grad_norm is not None:
            why = ("max_grad_norm=%r: wgnn_finish_clipped steps all eight tensors, and the norm over one group is not built"
                   % (self.max_grad_norm,))
        elif self.overlap_collectives:
            why = ("overlap_collectives=True: that schedule interleaves the backward parts and the optimiser steps of both "
                   "groups; a frozen group runs on the one-bucket schedule")
        elif self.plan is not None:
            why = ("grad_blocks: the blocked exchange interleaves the GRU tensors' row blocks with the conv tensors' part of the "
                   "backward; a frozen group runs on the one-bucket schedule")
        if why is not None:
            raise RuntimeError("windgnn_amd: %s with %s" % (who, why))
        return group

    def set_trainable(self, group):
        """Which tensors the following steps train: "all", "gru" (gru.weight_ih_l0, weight_hh_l0, bias_ih_l0, bias_hh_l0; the
        four conv tensors are frozen) or "conv" (conv1 / conv2 weight and bias; the four GRU tensors are frozen).  Between
        steps, e.g. a "gru" phase on a new station network followed by a few steps on "all".

        A frozen tensor keeps the bits of its parameter and of both Adam moments under every call that takes a step, its slice
        of the keep_best snapshot is a copy of those same bits, and its gradient view reads +0: this call zeroes the newly
        frozen slots of the bucket once (one torch op on the current stream), and the steps that follow never write there.
        On materialised windows (step, forward_backward, loss specs, carry_state) the part of the backward whose only
        products are the frozen group's gradients is not launched: "gru" runs parts 1 and 4 of wgnn_bwd*_part (never the dg
        GEMM and the GCN backward), "conv" parts 1 and 2 (never the weight-gradient GEMMs); the optimiser's launch is
        wgnn_finish(WGNN_FINISH_ADAM_GRU) or (.._CONV) alone.  Series mode (step_series, forward_backward_series) has no parts:
        its backward runs whole, the frozen slots are zeroed after it and only the trained group is stepped -- it saves no
        backward time.  Under a process group the one all-reduce still covers the whole bucket (zeros in the frozen slots);
        every rank must hold the same group, which is the caller's contract -- no collective checks it.

        torch.optim.Adam's rule holds: a tensor without a gradient does not advance its `step`.  Each group keeps its own count
        of steps taken, and its bias correction uses that count: after two steps on "gru", a step on "all" steps the conv tensors
        at 1 and the GRU tensors at 3 (two launches, one per group, while the counts differ; the one launch when they agree).
        `steps` stays the number of optimiser steps taken.

        Refused, naming the reason: an unknown group (ValueError); while an accumulation or a validation pass is open; and,
        for a group other than "all", max_grad_norm, overlap_collectives, grad_blocks (as the constructor refuses them) --
        accumulate / accumulate_series / apply are refused while a group is frozen."""
        who = "TrainStep.set_trainable(%r)" % (group,)
        group = self._trainable_arg(who, group)
        self._bucket_is_free("set_trainable")
        if self._val_open:
            raise RuntimeError("windgnn_amd: %s while a validation pass is open (validate*(..., more=True)): the pass scores one "
                               "model, and a best_on='validation' decision belongs to the group that trained it; close it with a "
                               "call with more=False first" % who)
        newly = group != "all" and group != self.trainable
        self.trainable = group
        if newly:
            self._frozen_grads().zero_()

    def _defer(self):
        """WGNN_BWD_DEFER for the parts a schedule enqueues: always, but for a frozen group under FROZEN_DEFER = False."""
        return _lib.BWD_DEFER if self.trainable == "all" or self.FROZEN_DEFER else 0

    def _parts(self):
        """The `part` of a backward that is enqueued whole (forward_backward): 7, or without the frozen group's part."""
        return 7 if self.trainable == "all" else 1 | _GROUP[self.trainable][0]

    def _frozen_grads(self):
        """The frozen group's slots of the gradient bucket (one-bucket layout: [header | conv | GRU])."""
        conv = self._gbuf[HEADER:HEADER + self.n_conv]
        return conv if self.trainable == "gru" else self._gbuf[HEADER + self.n_conv:]

    def _param_version(self):
        """torch's in-place version counters of the parameters: load_state_dict / optimiser-free edits through the
        nn.Parameters or the flat buffer bump them; the library's own kernels do not."""
        return (self.flat_p._version,) + tuple(p._version for p in self.params)

    def refresh(self):
        """Call after writing parameters in a way torch does not count (p.data.copy_(...), raw pointers): the staged
        W_ih images are rebuilt on the next step."""
        self._prepared_version = None

    def _images(self, d):
        if self._prepared is None:
            self._prepared = prepared_weights(d, self.p_views, self.device)
        else:
            refresh_prepared(d, self.p_views, self._prepared)
        self._prepared_version = self._param_version()

    def _group_count(self, group):
        """Completed optimiser steps of one group ("gru" / "conv")."""
        return self.steps - self._sat_out[group]

    def _adam(self, group=None):
        # the step being taken: self.steps counts COMPLETED steps (a step that raises does not advance Adam's bias correction);
        # group: "gru" / "conv" = that group's own count, None = both groups', which are then equal
        done = self._group_count(group or "gru")
        return dict(exp_avg=self.m_views, exp_avg_sq=self.v_views, step=done + 1, lr=self.lr, beta1=self.betas[0],
                    beta2=self.betas[1], eps=self.eps)

    def _tail(self, d, which, pre):
        """The optimiser's end of a step: reduce the deferred partial sums `which` (0: the bucket is final) and step Adam --
        ONE wgnn_finish, or with max_grad_norm wgnn_finish_norm (the same reduction + the norm) and wgnn_finish_clipped.
        Where the two groups do not step together -- one is frozen, or both train at different counts -- the reduce-only
        wgnn_finish comes first (WGNN_FINISH_ADAM_GRU / _CONV take no reduce bit), then one wgnn_finish per stepped group,
        each with its own step number."""
        if self.trainable == "all" and self._sat_out["gru"] == self._sat_out["conv"]:
            if self.max_grad_norm is None:
                finish_step(d, self.p_views, self.g_views, which, self._adam(), pre, self.device)
                return
            if self._clip is None or self._clip.numel() * 4 < clip_bytes(d):
                self._clip = clip_buffer(d, self.device)
            finish_norm(d, self.g_views, which, self.max_grad_norm, self._clip, self.device)
            finish_clipped(d, self.p_views, self.g_views, self._adam(), self._clip, pre, self.device)
            return
        if self.max_grad_norm is not None:      # (a checkpoint's counts: set_trainable itself refuses max_grad_norm)
            raise RuntimeError("windgnn_amd: TrainStep(max_grad_norm=%r) with the GRU tensors at optimiser step %d and the conv "
                               "tensors at %d: wgnn_finish_clipped steps all eight tensors with one step number; clipping over "
                               "groups at different counts is not built"
                               % (self.max_grad_norm, self._group_count("gru"), self._group_count("conv")))
        if which:
            finish_step(d, self.p_views, self.g_views, which, device=self.device)
        for group in ("gru", "conv") if self.trainable == "all" else (self.trainable,):
            finish_step(d, self.p_views, self.g_views, _GROUP[group][1], self._adam(group), pre, self.device)

    def _clip_word(self, slot, name):
        if self._clip is None:
            raise RuntimeError("windgnn_amd: TrainStep.%s is written by a step with max_grad_norm set (float('inf') measures "
                               "without clipping); %s" % (name, "no such step has run yet" if self.max_grad_norm is not None
                                                          else "this TrainStep has max_grad_norm=None"))
        return self._clip[slot]

    @property
    def grad_norm(self):
        """The L2 norm of the last step's (summed, unclipped) gradient: a 0-dim VIEW of the device value, overwritten by the
        next step -- float() or .clone() it to keep it, as with the returned loss."""
        return self._clip_word(_lib.CLIP_TOTAL, "grad_norm")

    @property
    def clip_coef(self):
        """min(1, max_grad_norm / (grad_norm + 1e-6)) of the last step, the factor its gradient entered Adam with: a 0-dim
        VIEW, overwritten by the next step."""
        return self._clip_word(_lib.CLIP_COEF, "clip_coef")

    @property
    def loss_count(self):
        """The labels the last step on a loss spec counted (windows x steps from loss_from on x outputs, less the missing
        labels): a 0-dim int64 VIEW of the device value, overwritten by the next such step."""
        if self._count is None:
            raise RuntimeError("windgnn_amd: TrainStep.loss_count is written by a step on a loss spec (step / forward_backward "
                               "with loss=, loss_from= or missing_labels= off their defaults); no such step has run yet")
        return self._count

    def _reset_best(self, threshold, words=None):
        """wgnn_best_init for `threshold`; `words`: public words to set after that (a checkpoint's)."""
        best_init(self._best, threshold)
        for name, value in (words or {}).items():
            best_word(self._best, name).copy_(torch.as_tensor(value).reshape(()))

    def _keep_best(self):
        if self._best_call is not None and self.best_on == "train":      # ("validation": a closed pass decides, not a step)
            keep_best_launch(self._best_call, self.steps)

    def _best_word(self, name):
        if self._best is None:
            raise RuntimeError("windgnn_amd: TrainStep.%s is kept by a step with keep_best set (True, or a loss threshold); "
                               "this TrainStep has keep_best=None" % name)
        return best_word(self._best, name)

    @property
    def best_loss(self):
        """The smallest loss that won so far (the threshold until one did): a 0-dim fp64 VIEW of the device record."""
        return self._best_word("best_loss")

    @property
    def best_step(self):
        """`steps` at the end of the step whose parameters are kept; -1: none yet.  A 0-dim int64 VIEW of the device record
        (one read per epoch serves the reference's patience counter)."""
        return self._best_word("best_step")

    @property
    def improved(self):
        """1 if the last step's loss won, else 0: a 0-dim int32 VIEW of the device record, overwritten by the next step."""
        return self._best_word("improved")

    def best_state_dict(self):
        """The kept parameters under the reference's eight keys in its order (clones: torch.save(tr.best_state_dict(), PATH)
        writes what the reference's load_state_dict(torch.load(PATH)) takes), or None while nothing was kept.  One host
        read (best_step): not for the per-step path."""
        if int(self._best_word("best_step")) < 0:
            return None
        return collections.OrderedDict((k, v.clone()) for k, v in zip(PARAM_ORDER, self._best_views))

    def restore_best(self):
        """Copy the kept parameters over the model's (moments and step count stay); the staged W_ih images are rebuilt on
        the next step.  Raises if nothing was kept."""
        if int(self._best_word("best_step")) < 0:
            raise RuntimeError("windgnn_amd: TrainStep.restore_best(): no step has beaten the threshold %r yet" % self.keep_best)
        self.flat_p.copy_(self._best_p)
        self.refresh()

    def state_dict(self):
        """What this step owns besides the parameters, as clones on its device:
        "optimizer": torch.optim.Adam(model.parameters(), lr, betas, eps).state_dict()'s layout (state[i] = {step, exp_avg,
        exp_avg_sq} for i in 0..7, one param group; hot_path_parameters() is in model.parameters() order);
        "steps"; "trainable", only once a group has been frozen -- now, or for some earlier step (state[i]["step"] is each tensor's
        own group's count, and `steps`, which counts every optimiser step, may then exceed both); "best": None or the record's public words plus the snapshot under the reference's keys; "carry": the
        carried [B, H] state or None; and, only once validate_series has run, "val": the public words of the validation record
        (the last closed pass, `passes`, `stale`; an open pass raises).  The parameters are model.state_dict()'s."""
        self._bucket_is_free("state_dict()")
        opt = torch.optim.Adam(self.params, lr=self.lr, betas=tuple(self.betas), eps=self.eps).state_dict()
        # (each tensor at its own group's count -- torch.optim.Adam's own layout after a run with a frozen group)
        opt["state"] = {i: {"step": torch.tensor(float(self._group_count("conv" if i < 4 else "gru"))), "exp_avg": m.clone(),
                            "exp_avg_sq": v.clone()}
                        for i, (m, v) in enumerate(zip(self.m_views, self.v_views))}
        best = None
        if self._best is not None:
            best = {name: best_word(self._best, name).clone() for name in _lib.BEST_WORDS}
            best.update((k, v.clone()) for k, v in zip(PARAM_ORDER, self._best_views))
        out = {"optimizer": opt, "steps": self.steps, "best": best, "carry": self.state}
        if self.trainable != "all" or any(self._sat_out.values()):
            # only once a group has been frozen: else the keys it has always had.  With the key, `steps` may exceed the Adam
            # counts (one step on "gru", one on "conv", one on "all": steps = 3, every tensor at 2)
            out["trainable"] = self.trainable
        if self._val is not None:       # "val": only once validate_series has made a record (else the four keys above)
            if self._val_open:
                raise RuntimeError("windgnn_amd: TrainStep.state_dict(): a validation pass is open (validate_series(..., more=True)); "
                                   "passes are not checkpointed mid-way: close it with a call with more=False first")
            out["val"] = {name: val_word(self._val, name).clone() for name in _lib.VAL_WORDS}
        return out

    def load_state_dict(self, sd):
        """Takes state_dict()'s output or a bare torch.optim.Adam state dict (the `step` values must agree within the four conv
        tensors and within the four GRU tensors; the two groups may differ, as after a phase with a frozen group; an empty
        `state` is step 0; from a bare dict `steps` becomes the larger count).  "trainable" is restored, "all" where the key is
        absent.  Moments are written into the existing flat buffers, lr / betas / eps restored, and from the full
        form the best record + snapshot, the carried state and, when the checkpoint has one, the validation record ("val":
        val_passes, val_stale and the last closed pass).  Load the parameters with model.load_state_dict."""
        self._bucket_is_free("load_state_dict()")
        full = "param_groups" not in sd
        opt = sd["optimizer"] if full else sd
        groups = opt["param_groups"]
        if len(groups) != 1 or len(groups[0]["params"]) != 8:
            raise ValueError("windgnn_amd: TrainStep.load_state_dict: expected one Adam param group of 8 parameters, got %s"
                             % [len(g["params"]) for g in groups])
        grp = groups[0]
        if grp.get("weight_decay", 0) != 0 or grp.get("amsgrad", False) or grp.get("maximize", False):
            raise ValueError("windgnn_amd: TrainStep runs plain Adam (weight_decay = 0, amsgrad = maximize = False), got "
                             "weight_decay=%r amsgrad=%r maximize=%r"
                             % (grp.get("weight_decay"), grp.get("amsgrad"), grp.get("maximize")))
        state = opt["state"]
        steps, have, done = 0, [], {"conv": 0, "gru": 0}
        if len(state):
            # torch.optim.Adam makes a tensor's state at its first gradient: a run on one group alone has the state of that group only
            have = sorted(state)
            if have not in (list(range(8)), list(range(4)), list(range(4, 8))):
                raise ValueError("windgnn_amd: TrainStep.load_state_dict: Adam state for parameters %s, expected 0..7 (or the "
                                 "conv tensors 0..3 / the GRU tensors 4..7 alone)" % have)
            counts = {i: int(round(float(state[i]["step"]))) for i in have}
            for name, idx in (("conv", range(4)), ("gru", range(4, 8))):
                mine = [counts[i] for i in idx if i in counts]
                if len(set(mine)) > 1:
                    raise ValueError("windgnn_amd: TrainStep.load_state_dict: the Adam `step` values disagree inside a group "
                                     "(%s): TrainStep steps the four conv tensors together and the four GRU tensors together"
                                     % {PARAM_ORDER[i]: c for i, c in counts.items()})
                done[name] = mine[0] if mine else 0
            steps = max(done.values())
            for i in have:
                for name, views in (("exp_avg", self.m_views), ("exp_avg_sq", self.v_views)):
                    if tuple(state[i][name].shape) != tuple(views[i].shape):
                        raise ValueError("windgnn_amd: TrainStep.load_state_dict: %s of %s is %s, expected %s"
                                         % (name, PARAM_ORDER[i], tuple(state[i][name].shape), tuple(views[i].shape)))
        group = sd.get("trainable", "all") if full else "all"
        self._trainable_arg("TrainStep.load_state_dict: trainable=%r" % (group,), group)
        apart = group != "all" or done["gru"] != done["conv"]
        if apart and self.max_grad_norm is not None:
            raise RuntimeError("windgnn_amd: TrainStep.load_state_dict: the GRU tensors are at optimiser step %d and the conv "
                               "tensors at %d, and this TrainStep has max_grad_norm=%r: wgnn_finish_clipped steps all eight "
                               "tensors with one step number" % (done["gru"], done["conv"], self.max_grad_norm))
        # (`steps` counts every optimiser step: the groups' own counts are no larger, and equal to it in a checkpoint without
        # "trainable", which is written only while no group has ever sat a step out)
        exact = not apart and "trainable" not in sd
        if full and len(state) and (int(sd["steps"]) != steps if exact else int(sd["steps"]) < steps):
            raise ValueError("windgnn_amd: TrainStep.load_state_dict: steps = %r but the Adam state is at step %d"
                             % (sd["steps"], steps))
        best, carry = (sd.get("best"), sd.get("carry")) if full else (None, None)
        if best is not None:
            if self._best is None:
                raise RuntimeError("windgnn_amd: TrainStep.load_state_dict: the checkpoint carries a best record, but this "
                                   "TrainStep has keep_best=None")
            missing = [k for k in list(_lib.BEST_WORDS) + list(PARAM_ORDER) if k not in best]
            if missing:
                raise ValueError("windgnn_amd: TrainStep.load_state_dict: the best record lacks %s" % ", ".join(missing))
            if float(best["best_loss"]) != float(best["best_loss"]):
                raise ValueError("windgnn_amd: TrainStep.load_state_dict: the best record's best_loss is NaN")
            for key, view in zip(PARAM_ORDER, self._best_views):
                if tuple(best[key].shape) != tuple(view.shape):
                    raise ValueError("windgnn_amd: TrainStep.load_state_dict: best %s is %s, expected %s"
                                     % (key, tuple(best[key].shape), tuple(view.shape)))
        val = sd.get("val") if full else None
        if val is not None:
            missing = [k for k in _lib.VAL_WORDS if k not in val]
            if missing:
                raise ValueError("windgnn_amd: TrainStep.load_state_dict: the validation record lacks %s" % ", ".join(missing))
        if carry is not None:
            H = self.p_views[5].shape[1]
            if not self.carry_state:
                raise RuntimeError("windgnn_amd: TrainStep.load_state_dict: the checkpoint carries a GRU state, but this "
                                   "TrainStep has carry_state=False")
            if carry.dim() != 2 or carry.shape[1] != H:
                raise ValueError("windgnn_amd: TrainStep.load_state_dict: carry is %s, expected [B, %d]" % (tuple(carry.shape), H))
        # everything checked: write
        if len(have) < 8:
            self.exp_avg.zero_()
            self.exp_avg_sq.zero_()
        for i in have:
            self.m_views[i].copy_(state[i]["exp_avg"])
            self.v_views[i].copy_(state[i]["exp_avg_sq"])
        self.steps = int(sd["steps"]) if full else steps
        self._sat_out = {g: self.steps - done[g] if len(state) else 0 for g in ("gru", "conv")}
        if group != self.trainable:
            self.trainable = group
            if group != "all":
                self._frozen_grads().zero_()
        self.lr, self.betas, self.eps = grp["lr"], tuple(grp["betas"]), grp["eps"]
        if self._best is not None and full:
            if best is None:
                self._reset_best(self.keep_best)
            else:
                self._reset_best(float(best["best_loss"]), {name: best[name] for name in _lib.BEST_WORDS})
                for key, view in zip(PARAM_ORDER, self._best_views):
                    view.copy_(best[key])
        if full and val is not None:
            if self._val is None:
                self._val = val_buffer(self.device)
            else:
                val_init(self._val)
            for name in _lib.VAL_WORDS:
                val_word(self._val, name).copy_(torch.as_tensor(val[name]).reshape(()))
            self._val_open = False
        if full and self.carry_state:
            if carry is None:
                self._has_state = False
            else:
                if self._hbuf is None or self._hbuf.shape[1] != carry.shape[0]:
                    self._hbuf = torch.zeros(2, carry.shape[0], carry.shape[1], dtype=torch.float32, device=self.device)
                self._hbuf[self._hcur].copy_(carry)
                self._has_state = True

    def _ensure_images(self, dims):
        """Build or rebuild the staged W_ih images if someone else wrote the parameters since they were last current.
        dims: () -> the Dims that size them (S, H and the math mode only), asked for only then."""
        if self._prepared_version != self._param_version():
            self._images(dims())

    def _run_schedule(self, d, bwd, gs):
        """The backward, the exchange and the optimiser of one step, in the order of this TrainStep's schedule (module
        docstring) -- the ONE place that orders them.  bwd: what the step kind enqueues (_Deferred), or _FINAL for a bucket
        that is final already; gs: this shard's weight, which the exchange scales the loss word with."""
        pre, ex = self._prepared, self.exchange
        if self.trainable != "all":
            # A frozen group (set_trainable): BPTT and the one part whose products are the trained group's gradients -- 4 for
            # "gru", 2 for "conv"; the other part is never enqueued, so the frozen slots of the bucket keep their zeros -- then
            # the one-rank or the one-bucket tail on that group alone.
            part = _GROUP[self.trainable][0]
            pending = bwd.pending & part if self.FROZEN_DEFER else 0       # (not deferred: the part reduces its own sums)
            bwd.parts(1)
            bwd.parts(part)
            if self.collective:
                if pending:
                    bwd.reduce(part)
                ex.all_reduce_all(gs)       # the whole bucket, as ever: zeros in the frozen slots, the loss word in the header
                self._tail(d, 0, pre)
            else:
                self._tail(d, pending, pre)
        elif self.plan is not None:
            # Blocked: part 1, then per row block its weight-gradient GEMM + reduction and the start of its all-reduce, then
            # part 2 under the last blocks' collectives, the tail's all-reduce and the blocked Adam.
            bwd.parts(1)
            works = []
            for b in self.plan.blocks:
                bwd.rows(b)
                works.append(ex.start_block(b))
            # HAZARD: part 2 reads W_ih through its W_ih^T image, and the blocks' Adam (_blocked_adam, the only place that
            # enqueues wgnn_finish_rows) rewrites both in place.  Part 2 is enqueued here, after every block's GEMM and before
            # ANY block's Adam; a wgnn_finish_rows above this line gives a wrong dg (and wrong conv gradients) with no error.
            bwd.parts(2)
            bwd.reduce(2)
            self._blocked_adam(d, works, ex.start_tail(self.plan, gs), pre)    # loss: the big-batch mean
        elif not self.collective:
            # One rank: BPTT, then the dg GEMM + GCN backward, and the weight-gradient GEMMs LAST, so that wgnn_finish reads
            # their split-K partial sums (115 MB at B = 4096) while they still sit in the Infinity Cache; deferring them
            # across the dg GEMM and the GCN backward (0.8 GB of traffic) had them come back from HBM (finish 35 us)
            for part in (1, 2, 4):         # (the order 1, 4, 2 measured the same, 672-680 us either way: round 3)
                bwd.parts(part)
            self._tail(d, bwd.pending, pre)                                                    # src/main.py:79 tail + :80
        elif not self.overlap_collectives:
            # the single-rank schedule, with ONE all-reduce of [loss | conv | GRU gradients] between the reduce-only finish and
            # the optimiser's: one collective, one stream dependency each way per step
            for part in (1, 2, 4):
                bwd.parts(part)
            bwd.reduce(6)
            ex.all_reduce_all(gs)           # loss: sum of the weighted shard means = the big-batch mean
            self._tail(d, 0, pre)                                                              # src/main.py:80
        else:
            # Overlap: the GRU gradients (99.8 % of the bucket) are final after parts 1|4 of the backward, so
            # their all-reduce runs on RCCL's stream while part 2 (dg GEMM + GCN backward, ~30 % of the
            # step) still computes; the 364 conv gradients and the loss follow in a second, tiny all-reduce.
            bwd.parts(1 | 4)
            bwd.reduce(4)
            work = ex.start_gru()
            bwd.parts(2)
            bwd.reduce(2)
            # the conv gradients' (tiny, latency-bound) all-reduce runs under the GRU tensors' optimiser step
            wconv = ex.start_conv(gs)       # loss: sum of the weighted shard means = the big-batch mean
            work.wait()
            finish_step(d, self.p_views, self.g_views, _lib.FINISH_ADAM_GRU, self._adam("gru"), pre, self.device)   # src/main.py:80
            wconv.wait()
            finish_step(d, self.p_views, self.g_views, _lib.FINISH_ADAM_CONV, self._adam("conv"), pre, self.device)

    def _blocked_adam(self, d, works, wtail, pre):
        """The optimiser half of the blocked step: Adam per row block once its all-reduce (and the tail's) has arrived, then
        the conv tensors.  Every wgnn_finish_rows rewrites W_ih and its images in place, so this runs after part 2 of the
        backward (the HAZARD in _run_schedule)."""
        wtail.wait()                    # b_ih / b_hh ride in the tail, and every block's Adam steps its rows' biases
        adam = self._adam("gru")        # (each group at its own count: they differ only after a phase with a frozen group)
        for b, work in zip(self.plan.blocks, works):
            work.wait()
            finish_rows(d, self.p_views, self.g_views, _ROWS[b.tensor], b.row0, b.rows, adam, pre, self.device)
        finish_step(d, self.p_views, self.g_views, _lib.FINISH_ADAM_CONV, self._adam("conv"), pre, self.device)

    def _end_step(self, check=True):
        """What follows the optimiser's launches of every schedule: the count, keep_best, the periodic check()."""
        self.steps += 1                         # only a step whose launches were all accepted counts
        if self.trainable != "all":
            self._sat_out[_GROUP[self.trainable][2]] += 1      # (the frozen group took no step: its own count stays)
        self._keep_best()                       # src/main.py:83-86
        if check and self.check_every and self.steps % self.check_every == 0 and (
                self.model.math != _lib.MATH_F32 or (self.exchange is not None and self.exchange.direct is not None)):
            self.check()

    def _empty_shard_step(self, A, X, n_global):
        """This rank has no windows in this step: zero bucket, the same collectives as every other rank, the optimiser's
        launch(es) on the summed gradient.  Returns (big-batch mean loss, empty Y)."""
        if not self.collective:
            raise RuntimeError("windgnn_amd: TrainStep.step needs at least one window (got a batch of %s)" % (tuple(X.shape),))
        _, d, _, _ = _forward_setup(A, X, self.p_views, self.model.math, B=1)   # sizes the finish launch (B-independent)
        self._ensure_images(lambda: d)
        gs = self.exchange.shard_weight(0, n_global)                   # 0.0; the count collective, if any, is issued
        self._gbuf.zero_()
        self._run_schedule(d, _FINAL, gs)
        self._end_step(check=False)             # no host read on this path: the next step with windows checks
        return self._loss, torch.empty(0, d.T, d.H, dtype=X.dtype, device=X.device)

    def _step_spec(self, who, X, L, loss, huber_delta, loss_from, missing_labels):
        """loss= / huber_delta= / loss_from= / missing_labels= of step / forward_backward, refused here by name before any
        launch: None at the defaults, which are the calls the two methods have always made, else (kind, delta, first counted
        step, missing_labels, L as [B, T, H])."""
        if loss == "mse" and loss_from == 0 and not missing_labels:
            return None
        who = "windgnn_amd: TrainStep." + who
        H = self.p_views[5].shape[1]
        if X.dim() != 4 or X.shape[3] != 13 or X.shape[2] * 13 != self.p_views[4].shape[1]:
            raise RuntimeError("%s: X must be [B, T, S = %d, 13], got %s" % (who, self.p_views[4].shape[1] // 13, tuple(X.shape)))
        B, T = X.shape[0], X.shape[1]
        kind, delta, t0 = validation_spec(loss, huber_delta, loss_from, T, who)
        if missing_labels and self.collective:
            raise RuntimeError("%s with missing_labels=True under a process group: the mean is over the labels that exist, so the "
                               "ranks' label counts would have to be exchanged before the backward, which is out of scope; train "
                               "on one device, or drop the windows that touch a gap and pass missing_labels=False" % who)
        if B == 0:                      # an empty shard: the keywords are checked, and the step is the one it was
            return kind, delta, t0, bool(missing_labels), L
        Lw = L.unsqueeze(0) if L.dim() == 2 else L
        if tuple(Lw.shape) != (B, T, H):
            raise ValueError("%s: L must be X's windows x H = [%d, %d, %d] ([T, H] is taken at B = 1), got %s"
                             % (who, B, T, H, tuple(L.shape)))
        if L.dtype not in (torch.float32, X.dtype):
            raise ValueError("%s: L must be float32 or X's dtype %s, got %s" % (who, X.dtype, L.dtype))
        return kind, delta, t0, bool(missing_labels), Lw

    def _spec_loss(self, who, Y, spec, gs):
        """The loss of `spec` into the bucket's header word (the unweighted shard mean: the exchange weights it), the count
        into loss_count, and dY weighted by gs."""
        kind, delta, t0, missing, Lw = spec
        _, dY, count = loss_spec_grad(Y, Lw, kind, delta, t0, missing, grad_scale=gs, loss_out=self._loss,
                                      who="windgnn_amd: TrainStep." + who)
        if self._count is None:
            self._count = torch.zeros((), dtype=torch.int64, device=count.device)
        self._count.copy_(count)
        return dY

    def _spec_forward(self, A, X, spec):
        """The forward of a step on a loss spec, without labels: (X as the kernels read it, Y in fp32, stash, d, spec).  With
        fp16 / bf16 X the Y that wgnn_fwd returns is rounded to that type, and a loss formed from it would carry the rounding
        (2^-9 at |y| near 1 in bf16) into every residual, where the fused MSE step reads the unrounded state: such a step
        therefore runs on an fp32 copy of X and of the labels (exact conversions), which gives the same hidden state
        unrounded; the caller gets Y rounded once to X's type, as the 16-bit forward gives it."""
        if X.dtype != torch.float32:
            _forward_setup(A, X, self.p_views, self.model.math)      # what refuses 16-bit I/O (math "f32") still does, unconverted
            kind, delta, t0, missing, Lw = spec
            X, spec = X.to(torch.float32), (kind, delta, t0, missing, Lw.to(torch.float32))
        Y, stash, d = self._forward(A, X, None)
        return X, Y, stash, d, spec

    def forward_backward(self, A, X, L, *, loss="mse", huber_delta=1.0, loss_from=0, missing_labels=False):
        """src/main.py:66,72,79: returns (loss, Y); gradients land in the flat bucket (no optimiser step).  `loss` is a
        view of the bucket's header word (see the module docstring).  loss, huber_delta, loss_from, missing_labels: as in
        step."""
        self._bucket_is_free("forward_backward")
        return self._forward_backward(A, X, L, loss, huber_delta, loss_from, missing_labels)[:2]

    def _forward_backward(self, A, X, L, loss, huber_delta, loss_from, missing_labels, admit=None):
        """forward_backward's calls: (loss, Y, the call's dims, its counted labels -- a host integer, with missing_labels the
        device scalar loss_count).  admit(windows, T, loss_from): accumulate's own refusals, after those of the keywords and
        before any launch."""
        X, L = X.contiguous(), L.contiguous()
        spec = self._step_spec("forward_backward", X, L, loss, huber_delta, loss_from, missing_labels)
        if admit is not None:
            admit(X.shape[0], X.shape[1] if X.dim() == 4 else None, spec[2] if spec is not None else 0)
        if spec is not None:
            Xf, Y, stash, d, spec = self._spec_forward(A, X, spec)
            dY = self._spec_loss("forward_backward", Y, spec, 1.0)
            gcn_gru_backward_raw(d, A, Xf, self.p_views, Y, dY, stash, self.g_views, part=self._parts(), prepared=self._prepared)
            count = self._count if spec[3] else Y.shape[0] * (Y.shape[1] - spec[2]) * Y.shape[2]
            return self._loss, Y.to(X.dtype), d, count
        Y, stash, d = self._forward(A, X, L)
        loss = self._loss
        gcn_gru_backward_mse_raw(d, A, X, self.p_views, Y, L, stash, self.g_views, loss, 1.0, part=self._parts() | 8,
                                 prepared=self._prepared)
        return loss, Y, d, Y.numel()

    def _series_refusals(self, A, series, seq_len, stride, missing_labels=False):
        """What step_series / forward_backward_series refuse, each before any launch and with the alternative."""
        windows = ("materialise the windows and labels (windgnn_amd.data.make_windows(feat, seq_len, starts=...)) and call "
                   "TrainStep.step(A, X, L) on them")
        why = None
        if missing_labels and self.collective:
            why = ("missing_labels=True under a process group: the mean is over the labels that exist, so the ranks' label counts "
                   "would have to be exchanged before the backward, which is out of scope; train on one device, or drop the "
                   "windows that touch a gap (series.segment_starts) and pass missing_labels=False")
        elif self.carry_state:
            why = ("carry_state=True: every window of series mode starts from h = 0; for truncated BPTT over consecutive chunks "
                   + windows)
        elif self.plan is not None:
            why = "grad_blocks: the blocked exchange needs the row-range weight gradients (wgnn_bwd_rows); " + windows
        elif self.overlap_collectives:
            why = ("overlap_collectives=True: series mode runs the one-bucket schedule (one all-reduce after the backward); build "
                   "the TrainStep with overlap_collectives=False, or " + windows)
        elif self.model.math != _lib.MATH_F32:
            why = "math != 'f32': series mode is exact fp32 only; build the model with math='f32', or " + windows
        elif hasattr(A, "blob"):
            why = "a CsrAdjacency: series mode takes a dense adjacency (S <= 64); pass the dense matrix, or " + windows
        elif not getattr(self.model, "fused", False):
            why = "a model of other widths than the reference's 13 / 13: train it through autograd (loss.backward())"
        if why is not None:
            raise RuntimeError("windgnn_amd: TrainStep.step_series with " + why)
        if series.dim() != 3 or series.shape[2] != 13:
            raise RuntimeError("windgnn_amd: TrainStep.step_series: series must be [rows, S, 13], got %s" % (tuple(series.shape),))
        if int(seq_len) < 1 or int(stride) < 1:
            raise ValueError("windgnn_amd: TrainStep.step_series: seq_len and stride must be >= 1, got %r and %r"
                             % (seq_len, stride))

    def _series_forward(self, A, series, Ls, seq_len, stride, n, starts=None, **masked):
        """The W_ih images, then wgnn_series_fwd_loss: (Y, stash, loss_buf, sd, d); d = the B-independent dims of the
        tail, as in _empty_shard_step.  starts: the sorted device table instead of (stride, n) -- wgnn_series_fwd_loss_at."""
        _require_gpu(series, Ls, *self.p_views)      # before the images: nothing is launched on host memory
        S, H = series.shape[1], self.p_views[5].shape[1]
        d = _lib.Dims(1, seq_len, S, 13, H, _lib.MATH_F32, _lib.ADJ_DENSE, 0, _lib.IO_F32)
        self._ensure_images(lambda: d)
        if starts is not None:
            Y, stash, loss_buf, sd, _ = series_forward_loss_raw(A, series, Ls, seq_len, None, self.p_views, _lib.MATH_F32,
                                                                prepared=self._prepared, starts=starts, **masked)
            return Y, stash, loss_buf, sd, d
        Y, stash, loss_buf, sd = series_forward_loss_raw(A, series, Ls, seq_len, stride, self.p_views, _lib.MATH_F32,
                                                         n_windows=n, prepared=self._prepared, **masked)
        return Y, stash, loss_buf, sd, d

    def _series_table(self, series, Ls, seq_len, stride, n_windows, starts, who="step_series", compact=False):
        """starts= of step_series / forward_backward_series: (series, Ls, sorted device table, inverse or None, n) with the label
        series checked -- a window may start at any row, so Ls needs a row for every row of the series.  compact=
        (series.compacted_starts): the series and the label series come back as their covered rows and the table points into
        them; Ls is then checked first, since its rows are gathered."""
        _no_stride_with_starts("windgnn_amd: TrainStep." + who, stride, starts, n_windows)
        H = self.p_views[5].shape[1]

        def labels_fit():
            if Ls.dim() != 2 or Ls.shape[1] != H or Ls.shape[0] < series.shape[0]:
                raise RuntimeError("windgnn_amd: TrainStep." + who + ": with starts= the label series Ls must be [rows >= the "
                                   "series' %d, H = %d] (series_labels(feat, ...)[0] of a feat 3 rows longer than the series), "
                                   "got %s" % (series.shape[0], H, tuple(Ls.shape)))
        if compact is not False:
            labels_fit()
        series_c, Ls_c, table, inverse = compacted_starts(starts, series, Ls, seq_len, "windgnn_amd: TrainStep." + who, compact,
                                                          forward_only=who == "validate_series")
        if table.numel() > 0:
            labels_fit()
        return series_c, Ls_c, table, inverse, table.numel()

    def _series_count(self, series, Ls, seq_len, stride, n_windows, who="step_series"):
        """The window count of this call, with n_windows and Ls checked against it."""
        fit = n_series_windows(series.shape[0], seq_len, stride)
        n = fit if n_windows is None else int(n_windows)
        if n < 0 or n > fit:
            raise RuntimeError("windgnn_amd: TrainStep." + who + ": n_windows = %d, but a series of %d rows holds %d windows of "
                               "%d rows at stride %d" % (n, series.shape[0], fit, seq_len, stride))
        need = (n - 1) * stride + seq_len
        H = self.p_views[5].shape[1]
        if n > 0 and (Ls.dim() != 2 or Ls.shape[1] != H or Ls.shape[0] < need):
            raise RuntimeError("windgnn_amd: TrainStep." + who + ": the label series Ls must be [rows >= (n - 1) * stride + "
                               "seq_len = %d, H = %d] (series_labels(feat, seq_len, stride, n_windows)[0]; its window view L is "
                               "for TrainStep.step on materialised windows), got %s" % (need, H, tuple(Ls.shape)))
        return n

    def _series_loss(self, who, seq_len, missing_labels, loss, huber_delta, loss_from):
        """loss= / huber_delta= / loss_from= of step_series / forward_backward_series, refused here by name before any launch:
        the keywords for (series_forward_loss_raw, series_backward_mse_raw) -- none at the defaults, which are the calls the
        two methods have always made."""
        if loss_spec(loss, huber_delta, loss_from, seq_len, missing_labels, "windgnn_amd: TrainStep." + who) is None:
            return {}, {}
        rest = {"huber_delta": float(huber_delta), "loss_from": int(loss_from)}
        return dict(rest, loss=loss), dict(rest, loss_kind=loss)

    def forward_backward_series(self, A, series, Ls, seq_len, stride=None, n_windows=None, starts=None, missing_labels=False,
                                loss="mse", huber_delta=1.0, loss_from=0, compact=False):
        """forward_backward on the first n_windows sliding windows of `series` [rows, S, 13] with the label series Ls
        [>= (n - 1) * stride + seq_len, H]: returns (loss, Y [n, seq_len, H]); the gradients land in the flat bucket, final (no
        optimiser step).  `loss` is a view of the bucket's header word.  starts, missing_labels, loss, huber_delta, loss_from,
        compact: as in step_series."""
        self._bucket_is_free("forward_backward_series")
        return self._forward_backward_series(A, series, Ls, seq_len, stride, n_windows, starts, missing_labels, loss,
                                             huber_delta, loss_from, compact=compact)[:2]

    def _forward_backward_series(self, A, series, Ls, seq_len, stride, n_windows, starts, missing_labels, loss, huber_delta,
                                 loss_from, admit=None, compact=False, who="forward_backward_series"):
        """forward_backward_series' calls: (loss, Y, the tail's dims, the call's counted labels -- a host integer, with
        missing_labels the sum of the integer counts the masked forward leaves in loss_buf, a device scalar).  admit: as in
        _forward_backward."""
        seq_len, table, inverse = int(seq_len), None, None
        self._series_refusals(A, series, seq_len, 1 if stride is None else int(stride), missing_labels)
        fn_f, fn_b = self._series_loss("forward_backward_series", seq_len, missing_labels, loss, huber_delta, loss_from)
        _compact_arg("windgnn_amd: TrainStep." + who, compact, starts, stride)
        series, Ls = series.contiguous(), Ls.contiguous()
        if starts is not None:
            series, Ls, table, inverse, n = self._series_table(series, Ls, seq_len, stride, n_windows, starts, compact=compact)
        else:
            stride = 1 if stride is None else int(stride)
            n = self._series_count(series, Ls, seq_len, stride, n_windows)
        if n == 0:
            raise RuntimeError("windgnn_amd: TrainStep.forward_backward_series needs at least one window (a series of %d rows, "
                               "seq_len %d, n_windows %r)" % (series.shape[0], seq_len, n_windows))
        if admit is not None:
            admit(n, seq_len, int(loss_from))
        at = {} if table is None else {"starts": table}     # (the strided call is the call it has always been)
        masked = {"missing_labels": True} if missing_labels else {}     # (and so is the call without the flag)
        Y, stash, loss_buf, sd, d = self._series_forward(A, series, Ls, seq_len, stride, n, table, **masked, **fn_f)
        series_backward_mse_raw(sd, A, series, self.p_views, Y, Ls, stash, loss_buf, self.g_views, self._loss, 1.0,
                                prepared=self._prepared, **at, **masked, **fn_b)
        if self.trainable != "all":     # (wgnn_series_bwd* has no parts: the backward ran whole)
            self._frozen_grads().zero_()
        if admit is None:               # (forward_backward_series: the call it has always been, launch for launch)
            count = None
        elif missing_labels:            # include/windgnn_series_masked.h: sums | maxima | tag + 3 words | uint32 counts
            nb = -(-n // 16)
            count = loss_buf[2 * nb + 4:3 * nb + 4].view(torch.int32).sum()
        else:
            count = n * (seq_len - int(loss_from)) * Y.shape[2]
        return self._loss, (Y if inverse is None else Y.index_select(0, inverse)), d, count

    def step_series(self, A, series, Ls, seq_len, stride=None, n_windows=None, n_global=None, starts=None,
                    missing_labels=False, loss="mse", huber_delta=1.0, loss_from=0, compact=False):
        """One optimiser step on the first `n_windows` (default: all that fit) sliding windows of this rank's `series`
        [rows, S, 13]: window w covers rows w * stride .. w * stride + seq_len - 1 and starts from h = 0, as step() on the
        materialised windows would.  Ls [>= (n - 1) * stride + seq_len, H]: the label SERIES (series_labels(feat, seq_len,
        stride, n_windows)[0]), read at the rows the windows cover; no window-major labels and no dY exist.  `n_global`: as in
        step().  Returns (loss, Y [n, seq_len, H]); the loss is the same 0-dim VIEW of the bucket's header word.  Under a
        process group every rank passes its own sub-series (the caller's slicing: consecutive ranks' rows overlap by
        seq_len - stride); a rank with no window takes the empty-shard step.  stride defaults to 1.
        starts (instead of stride / n_windows): the step runs on exactly the windows that begin at these rows of `series` -- a list
        or tensor in any order, duplicates allowed (series.segment_starts for a series with outages, a hold-out, one block of a
        shuffled epoch).  The loss and the gradients are over the listed windows, the window count is the table's length (an
        empty table: the empty-shard step), Y comes back in the table's order, and Ls needs a row for every row of `series`.
        With compact=False the graph convolutions and the input projection run on every row of `series`, whatever the table
        lists.  compact=True: they run on the hours some window covers alone -- series.compact_table maps every covered hour to
        its rank among them, the rows are gathered (series, Ls) and the same calls run on the shorter series with the table of
        ranks; the window count, the counted labels and the shard weight are those of compact=False, Y, the loss and the
        gradients agree with it to rounding (the weight-gradient sums are grouped over another row count, and a front layout
        on the other side of 4096 rows takes the other GEMM instance).  A host table is compacted on the host to exactly the covered hours; a
        device table on the device, without a host read, to min(rows, n * seq_len) rows -- compact=<int> promises that the
        table covers at most that many hours and sizes the compacted series by it (a table that covers more is reported like a
        bad device table).  compact="auto": compact where it is measured to pay -- a host table that covers at most
        series.COMPACT_AUTO_THETA of the rows; not a device table, and not validate_series ("Covered hours
        only", has the numbers).  Only with starts=.
        missing_labels=True (include/windgnn_series_masked.h): a NaN in Ls means "no label" -- it adds nothing to the loss or to
        any gradient, and the mean is over the labels that exist (build `series` from the filled table, Ls from the unfilled
        one).  With no label at all the loss is NaN and the gradients are zero.  Refused under a process group.
        loss="mse" | "l1" | "huber" (include/windgnn_series_lossfn.h): the mean over the counted entries of (Y - L)^2, |Y - L| or
        nn.HuberLoss(delta=huber_delta); loss_from=t counts steps t .. seq_len - 1 of every window alone (seq_len - 1: the last
        step, what the reference evaluates), while the gradient still flows back through the warm-up steps.  Both work with
        missing_labels, and under a process group without it (every window counts the same number of entries on every rank).
        The returned loss, keep_best, max_grad_norm and checkpoints see that loss; with the defaults the step is the one it was."""
        self._bucket_is_free("step_series")
        seq_len, table, inverse = int(seq_len), None, None
        self._series_refusals(A, series, seq_len, 1 if stride is None else int(stride), missing_labels)
        fn_f, fn_b = self._series_loss("step_series", seq_len, missing_labels, loss, huber_delta, loss_from)
        _compact_arg("windgnn_amd: TrainStep.step_series", compact, starts, stride)
        series, Ls = series.contiguous(), Ls.contiguous()
        if starts is not None:
            series, Ls, table, inverse, n = self._series_table(series, Ls, seq_len, stride, n_windows, starts, compact=compact)
        else:
            stride = 1 if stride is None else int(stride)
            n = self._series_count(series, Ls, seq_len, stride, n_windows)
        if n == 0:
            return self._empty_shard_step(A, series.new_empty((0, seq_len) + tuple(series.shape[1:])), n_global)
        gs = self.exchange.shard_weight(n, n_global) if self.collective else 1.0
        at = {} if table is None else {"starts": table}     # (the strided call is the call it has always been)
        masked = {"missing_labels": True} if missing_labels else {}     # (and so is the call without the flag)
        Y, stash, loss_buf, sd, d = self._series_forward(A, series, Ls, seq_len, stride, n, table, **masked, **fn_f)
        series_backward_mse_raw(sd, A, series, self.p_views, Y, Ls, stash, loss_buf, self.g_views, self._loss, gs,
                                prepared=self._prepared, **at, **masked, **fn_b)
        if self.trainable != "all":     # (wgnn_series_bwd* has no parts: the backward ran whole; series mode saves no time)
            self._frozen_grads().zero_()
        self._run_schedule(d, _FINAL, gs)       # the bucket is final: (the all-reduce,) Adam and the W_ih images
        self._end_step()
        return self._loss, (Y if inverse is None else Y.index_select(0, inverse))

    def validate_series(self, A, series, Ls, seq_len, stride=None, n_windows=None, starts=None, missing_labels=False,
                        loss="mse", huber_delta=1.0, loss_from=0, more=False, evaluator=None, compact=False):
        """The loss of step_series' spec on windows the model is NOT training on (include/windgnn_series_val.h): the model's
        current parameters, forward-only -- no Y, no stash, no backward -- and no change to the optimiser, the gradient bucket or
        `steps`.  A, series, Ls, seq_len, stride / n_windows or starts (any order, duplicates allowed; series.segment_starts gives
        a hold-out at window level), missing_labels, loss, huber_delta, loss_from, compact: as in step_series.  A pass accumulates over
        calls: more=True leaves it open for the next table or segment of the hold-out, more=False (the default) closes it.  The
        return value is the pass's mean loss so far, a 0-dim fp32 VIEW of the device record (`val_loss`), overwritten by the
        next call.  Closing: with TrainStep(keep_best=..., best_on="validation") wgnn_keep_best runs on that loss word with the
        current parameters and step = `steps` (best_loss / best_step / best_state_dict() then speak of validation passes), then
        wgnn_val_close counts the pass in `val_passes` and keeps `val_stale`, the closed passes since the last one that won --
        the reference's `if patience > 10: break` is `int(tr.val_stale) > 10`, one host read per epoch.  With best_on="train"
        a pass touches neither the best record nor val_stale.
        evaluator=ev (evaluate.Evaluator): the same forward's last rows, de-normalised with ev's wind_min / wind_max, go to ev's
        accumulator as ev.update_series would put them there (skip_missing = missing_labels): the loss the model is trained on
        and the reference's RMSE / MAE / accuracy from one forward.
        Nothing synchronises with the host.  Under a process group nothing is exchanged: every rank must validate the SAME tables;
        each then gets the same bits and takes the same decision.  A hold-out sharded over the ranks is out of scope.
        Exact fp32, a dense adjacency, S <= 64, H <= 128: the rest is refused as step_series refuses it, before any launch."""
        seq_len, table, inverse = int(seq_len), None, None
        self._validate_refusals(A, series, seq_len, 1 if stride is None else int(stride))
        val_spec(loss, huber_delta, loss_from, seq_len, missing_labels, "windgnn_amd: TrainStep.validate_series")
        if evaluator is not None and (getattr(evaluator, "H", None) != self.p_views[5].shape[1]):
            raise ValueError("windgnn_amd: TrainStep.validate_series: evaluator= must be an evaluate.Evaluator of this model's %d "
                             "outputs, got %r" % (self.p_views[5].shape[1], evaluator))
        _compact_arg("windgnn_amd: TrainStep.validate_series", compact, starts, stride)
        series, Ls = series.contiguous(), Ls.contiguous()
        full, Ls_full = series, Ls           # (the evaluator looks its truths up at the caller's starts)
        if starts is not None:
            series, Ls, table, inverse, n = self._series_table(series, Ls, seq_len, stride, n_windows, starts, "validate_series",
                                                               compact)
        else:
            stride = 1 if stride is None else int(stride)
            n = self._series_count(series, Ls, seq_len, stride, n_windows, "validate_series")
        if n == 0:
            raise RuntimeError("windgnn_amd: TrainStep.validate_series needs at least one window (a series of %d rows, seq_len %d, "
                               "n_windows %r, starts %s)" % (series.shape[0], seq_len, n_windows,
                                                             "empty" if starts is not None else None))
        _require_gpu(series, Ls, *self.p_views)      # before the images and the record: nothing is launched on host memory
        S, H = series.shape[1], self.p_views[5].shape[1]
        self._ensure_images(lambda: _lib.Dims(1, seq_len, S, 13, H, _lib.MATH_F32, _lib.ADJ_DENSE, 0, _lib.IO_F32))
        if self._val is None:
            self._val = val_buffer(self.device)
        if not self._val_open:
            val_begin(self._val)
            self._val_open = True
        last = torch.empty(n, H, dtype=torch.float32, device=series.device) if evaluator is not None else None
        wmin, wmax = (evaluator.wind_min, evaluator.wind_max) if evaluator is not None else (0.0, 1.0)
        series_val_raw(A, series, self.p_views, Ls, seq_len, stride=None if table is not None else stride,
                       n_windows=None if table is not None else n, prepared=self._prepared, loss=loss, huber_delta=huber_delta,
                       loss_from=loss_from, missing_labels=missing_labels, starts=table, last=last, val=self._val,
                       wind_min=wmin, wind_max=wmax)
        if evaluator is not None:
            self._feed_evaluator(evaluator, last, inverse, full, Ls_full, seq_len, stride, starts, missing_labels)
        if not more:
            self._close_validation()
        return val_word(self._val, "loss")

    def validate(self, A, X, L, missing_labels=False, loss="mse", huber_delta=1.0, loss_from=0, more=False, evaluator=None):
        """validate_series' pass on MATERIALISED windows, for everything GCN_GRU.forward accepts: X [B, T, S, 13] and L [B, T, H]
        ([T, H] or [1, T, H] at B = 1, as the reference's test_loader yields them; fp32 or X's dtype), any math mode, fp32 / fp16 /
        bf16 I/O (X's dtype), a dense adjacency or a CsrAdjacency, any H.  The forward is the stash-less one model(A, X) runs
        under torch.no_grad() -- the same call on the current parameters (and the current W_ih images, when they are current),
        hence the same Y bits -- from h = 0 also with carry_state=True; it changes nothing of the optimiser, the gradient bucket,
        `steps`, the images or the carried state, and it does not read the range-status word (check() does).  The loss terms
        are functional.validation_terms' (fp64, torch operations on the device) and functional.val_add puts them into the same
        record wgnn_series_val writes: missing_labels, loss, huber_delta, loss_from, more, the closing (wgnn_keep_best under
        best_on="validation", wgnn_val_close, `val_stale`) and the returned 0-dim VIEW `val_loss` are validate_series'; calls of
        both kinds may share a pass.
        loss_from = T - 1 with fp32 X: wgnn_fwd_last with (wind_min, wind_max) = (0, 1) -- y * 1 + 0 is exact -- so the
        register-resident recurrences never write the other T - 1 rows; the terms are the full route's.
        evaluator=ev: the last rows of the same forward, de-normalised by wgnn_predict_last with ev's wind_min / wind_max, go to
        ev's accumulator through wgnn_eval_accum as ev.update(X, L) would put them there.  Not with missing_labels=True:
        wgnn_eval_accum has no skip.
        Nothing synchronises with the host.  Under a process group nothing is exchanged: every rank validates the SAME windows."""
        from .data import predict_last
        from .evaluate import eval_accum
        who = "windgnn_amd: TrainStep.validate"
        H = self.p_views[5].shape[1]
        if X.dim() != 4 or X.shape[0] < 1 or X.shape[3] != 13 or X.shape[2] * 13 != self.p_views[4].shape[1]:
            raise RuntimeError("%s: X must be [B >= 1, T, S = %d, 13], got %s" % (who, self.p_views[4].shape[1] // 13, tuple(X.shape)))
        B, T = X.shape[0], X.shape[1]
        kind, delta, t0 = validation_spec(loss, huber_delta, loss_from, T, who)
        Lw = L.unsqueeze(0) if L.dim() == 2 else L
        if tuple(Lw.shape) != (B, T, H):
            raise ValueError("%s: L must be X's windows x H = [%d, %d, %d] ([T, H] is taken at B = 1), got %s"
                             % (who, B, T, H, tuple(L.shape)))
        if L.dtype not in (torch.float32, X.dtype):
            raise ValueError("%s: L must be float32 or X's dtype %s, got %s" % (who, X.dtype, L.dtype))
        if evaluator is not None:
            if getattr(evaluator, "H", None) != H:
                raise ValueError("%s: evaluator= must be an evaluate.Evaluator of this model's %d outputs, got %r" % (who, H, evaluator))
            if missing_labels:
                raise ValueError("%s: evaluator= with missing_labels=True: wgnn_eval_accum has no skip, so a NaN truth would poison "
                                 "its column; feed the evaluator from the series (validate_series(..., missing_labels=True, "
                                 "evaluator=ev) or ev.update_series(..., skip_missing=True)), or call ev.update on the windows "
                                 "whose last label exists" % who)
        _require_gpu(X, Lw, io_ok=True)      # before the record and any launch: nothing runs on host memory
        _require_gpu(*self.p_views)
        X = X.contiguous()
        # the images as they are: used when current, never built or refreshed here (the library stages its own otherwise)
        pre = self._prepared if self._prepared is not None and self._prepared_version == self._param_version() else None
        if t0 == T - 1 and X.dtype == torch.float32:
            Y = gcn_gru_forward_last_raw(A, X, self.p_views, self.model.math, prepared=pre).view(B, 1, H)
            s, m, a = validation_terms(Y, Lw[:, T - 1:], kind, delta, 0, missing_labels)
        else:
            Y, _, _ = gcn_gru_forward_raw(A, X, self.p_views, self.model.math, want_stash=False, prepared=pre)
            s, m, a = validation_terms(Y, Lw, kind, delta, t0, missing_labels)
        if self._val is None:
            self._val = val_buffer(self.device)
        if not self._val_open:
            val_begin(self._val)
            self._val_open = True
        val_add(self._val, s, m, a)
        if evaluator is not None:
            f32 = Y.dtype == torch.float32 and Lw.dtype == torch.float32
            pred = predict_last(Y if f32 else Y[:, -1:].float(), evaluator.wind_min, evaluator.wind_max)
            err = torch.empty_like(pred) if evaluator.keep_errors else None
            eval_accum(pred, (Lw if f32 else Lw[:, -1:].float()).contiguous(), evaluator.wind_min, evaluator.wind_max,
                       evaluator._acc(), err)
            if err is not None:
                evaluator._errors.append(err)
        if not more:
            self._close_validation()
        return val_word(self._val, "loss")

    def _validate_refusals(self, A, series, seq_len, stride):
        """What validate_series refuses, each before any launch and with the alternative: step_series' scope without what
        belongs to the optimiser's schedule (a pass takes no step, so carry_state, grad_blocks and overlap_collectives do not
        enter) and without the process-group refusal of missing labels (nothing is exchanged: every rank counts its own)."""
        windows = ("materialise the windows and labels (windgnn_amd.data.make_windows(feat, seq_len, starts=...)), run "
                   "GCN_GRU.forward on them under torch.no_grad() and form the loss with torch")
        why = None
        if self.model.math != _lib.MATH_F32:
            why = "math != 'f32': series mode is exact fp32 only; build the model with math='f32', or " + windows
        elif hasattr(A, "blob"):
            why = "a CsrAdjacency: series mode takes a dense adjacency (S <= 64); pass the dense matrix, or " + windows
        elif not getattr(self.model, "fused", False):
            why = "a model of other widths than the reference's 13 / 13: " + windows
        if why is not None:
            raise RuntimeError("windgnn_amd: TrainStep.validate_series with " + why)
        if series.dim() != 3 or series.shape[2] != 13:
            raise RuntimeError("windgnn_amd: TrainStep.validate_series: series must be [rows, S, 13], got %s" % (tuple(series.shape),))
        if int(seq_len) < 1 or int(stride) < 1:
            raise ValueError("windgnn_amd: TrainStep.validate_series: seq_len and stride must be >= 1, got %r and %r"
                             % (seq_len, stride))

    def _feed_evaluator(self, ev, last, inverse, series, Ls, seq_len, stride, starts, missing_labels):
        """The pass's last rows into ev's accumulator, in the caller's order against the caller's table, as
        Evaluator.update_series does it (the accumulator adds in row order: the same order gives the same bits)."""
        from .evaluate import eval_accum_series
        pred = last if inverse is None else last.index_select(0, inverse)
        table = None
        if starts is not None:
            table = _starts_table(starts, series.shape[0], seq_len, series.device, "windgnn_amd: TrainStep.validate_series",
                                  ordered=False)
        err = torch.empty_like(pred) if ev.keep_errors else None
        eval_accum_series(pred, Ls, seq_len, ev.wind_min, ev.wind_max, ev._acc(), None if starts is not None else stride, table,
                          bool(missing_labels), err)
        if err is not None:
            ev._errors.append(err)

    def _close_validation(self):
        """The end of a pass: with best_on="validation" wgnn_keep_best on the record's loss word (the current parameters,
        step = `steps`), then wgnn_val_close, which reads the decision that call has just published."""
        decides = self.best_on == "validation"
        if decides:
            if self._val_best_call is None:      # (the record and the views never move: marshalled once)
                self._val_best_call = keep_best_args(self._best_dims, val_word(self._val, "loss"), self.p_views, self._best_views,
                                                     self._best)
            keep_best_launch(self._val_best_call, self.steps)
        val_close(self._val, self._best if decides else None)
        self._val_open = False

    def _val_word(self, name, word):
        """A public word of the validation record, which the first validate_series or validate call makes."""
        if self._val is None:
            raise RuntimeError("windgnn_amd: TrainStep.%s is kept by validate_series (include/windgnn_series_val.h); no "
                               "validation call has run on this TrainStep yet" % name)
        return val_word(self._val, word)

    @property
    def val_loss(self):
        """The mean held-out loss of the open pass so far, or of the last closed one (NaN before its first call and when it
        counted no label): a 0-dim fp32 VIEW of the device record, overwritten by the next validate_series call."""
        return self._val_word("val_loss", "loss")

    @property
    def val_count(self):
        """The entries that pass counted (windows x steps from loss_from on x outputs, less the missing labels): 0-dim int64 VIEW."""
        return self._val_word("val_count", "count")

    @property
    def val_passes(self):
        """Closed validation passes: a 0-dim int64 VIEW of the device record."""
        return self._val_word("val_passes", "passes")

    @property
    def val_stale(self):
        """Closed passes since the last one whose loss won under best_on="validation" (0 right after a win): a 0-dim int64 VIEW;
        `int(tr.val_stale) > 10` is the reference's patience test, one host read per epoch."""
        return self._val_word("val_stale", "stale")

    def _forward(self, A, X, L):
        # the first call sizes and builds the images from the dims of this batch (they depend on S, H, math only)
        self._ensure_images(lambda: _forward_setup(A, X, self.p_views, self.model.math)[1])
        return gcn_gru_forward_raw(A, X, self.p_views, self.model.math, want_stash=True, labels=L, prepared=self._prepared)

    @property
    def state(self):
        """A copy of the state the next carry_state step starts from ([B, H] fp32), or None (zeros: no step since the
        last reset)."""
        return self._hbuf[self._hcur].clone() if self._has_state else None

    def reset_state(self):
        """The next carry_state step starts from zeros (e.g. at the start of a new series / epoch)."""
        self._has_state = False

    def _state_forward(self, A, X, L):
        """Forward from the carried state (carry_state=True): returns Y, stash, d and leaves h_n in the other buffer."""
        if X.dtype != torch.float32:
            raise RuntimeError("windgnn_amd: TrainStep(carry_state=True) takes fp32 attr_matrix / labels (the loss pass, "
                               "wgnn_mse_loss_grad, reads fp32), got %s" % X.dtype)
        B, H = X.shape[0], self.p_views[5].shape[1]
        if self._hbuf is None or self._hbuf.shape[1] != B:
            if self._has_state:
                raise RuntimeError("windgnn_amd: TrainStep(carry_state=True): the batch changed from %d to %d windows while "
                                   "a state is carried; call reset_state() first" % (self._hbuf.shape[1], B))
            self._hbuf = torch.zeros(2, B, H, dtype=torch.float32, device=self.device)
        self._ensure_images(lambda: _forward_setup(A, X, self.p_views, self.model.math)[1])
        h0 = self._hbuf[self._hcur] if self._has_state else None
        Y, _, stash, d = gcn_gru_state_forward_raw(A, X, self.p_views, self.model.math, h0, self._hbuf[1 - self._hcur],
                                                   prepared=self._prepared)
        return Y, stash, d

    def _state_step(self, A, X, L, gs, spec=None):
        """The carry_state=True step: the loss and dY from wgnn_mse_loss_grad (into the bucket's loss slot) -- on a loss spec
        from functional.loss_spec_grad -- and the backward through wgnn_bwd_state_part (dh_n = 0, no dh0: the carried state is
        detached)."""
        Y, stash, d = self._state_forward(A, X, L)
        if spec is not None:
            dY = self._spec_loss("step", Y, spec, gs)
        else:
            _, dY = mse_loss_grad(Y, L, gs, loss=self._loss)    # the unweighted shard mean: the exchange weights it

        def parts(mask):
            gcn_gru_state_backward_raw(d, A, X, self.p_views, Y, dY, None, stash, self.g_views, part=mask | self._defer(),
                                       prepared=self._prepared)
        self._run_schedule(d, _Deferred(self, d, parts, Y, stash), gs)
        self._hcur, self._has_state = 1 - self._hcur, True     # h_n of this step is the next step's h0
        return Y

    def _plain_step(self, A, X, L, gs):
        """The step from h = 0: wgnn_fwd_loss, then wgnn_bwd_mse_part, whose part 1 also finalises the loss (bit 8)."""
        Y, stash, d = self._forward(A, X, L)

        def parts(mask):
            gcn_gru_backward_mse_raw(d, A, X, self.p_views, Y, L, stash, self.g_views, self._loss, gs,
                                     part=mask | (mask & 1) << 3 | self._defer(), prepared=self._prepared)
        self._run_schedule(d, _Deferred(self, d, parts, Y, stash), gs)
        return Y

    def _spec_step(self, A, X, L, gs, spec):
        """The step from h = 0 on a loss spec: wgnn_fwd (no labels), the loss and dY from functional.loss_spec_grad, then
        wgnn_bwd_part on that dY, its parts deferred as the carried-state step's are."""
        Xf, Y, stash, d, spec = self._spec_forward(A, X, spec)
        dY = self._spec_loss("step", Y, spec, gs)

        def parts(mask):
            gcn_gru_backward_raw(d, A, Xf, self.p_views, Y, dY, stash, self.g_views, part=mask | self._defer(),
                                 prepared=self._prepared)
        self._run_schedule(d, _Deferred(self, d, parts, Y, stash), gs)
        return Y.to(X.dtype)

    def step(self, A, X, L, n_global=None, *, loss="mse", huber_delta=1.0, loss_from=0, missing_labels=False):
        """One optimiser step on this rank's windows (src/main.py:66-80).  `n_global`: windows of ALL ranks in this step,
        when the caller knows it (a fixed global batch); None = the exchange all-reduces the count on every step (a host
        sync).  Launch-sized tail: ONE wgnn_finish (reduce the deferred partial sums + Adam + next step's W_ih images);
        with a process group two of them around the one all-reduce.  The returned loss is a VIEW of the gradient bucket's
        header word, overwritten by the next step (module docstring): float() or .clone() it to keep it.
        loss="mse" | "l1" | "huber", huber_delta, loss_from=t, missing_labels: the loss validate scores (the definitions of
        include/windgnn_series_lossfn.h, which step_series' docstring restates), in every math mode, on a dense or CSR
        adjacency, any H, fp32 / fp16 / bf16 I/O, with or without carry_state, in every schedule.  At the defaults the step is
        the one it was.  Otherwise the loss and dY come from functional.loss_spec_grad on the forward's Y (module docstring); L
        is [B, T, H] ([T, H] at B = 1), fp32 or X's dtype; `loss_count` holds the labels counted; with no label at all the
        loss is NaN and the gradients are zero.  missing_labels=True is refused under a process group."""
        self._bucket_is_free("step")
        X, L = X.contiguous(), L.contiguous()   # a strided batch slice is copied here, never read as if dense
        spec = self._step_spec("step", X, L, loss, huber_delta, loss_from, missing_labels)
        if X.shape[0] == 0:
            return self._empty_shard_step(A, X, n_global)
        gs = self.exchange.shard_weight(X.shape[0], n_global) if self.collective else 1.0
        if spec is None:
            Y = (self._state_step if self.carry_state else self._plain_step)(A, X, L, gs)
        else:
            Y = (self._state_step if self.carry_state else self._spec_step)(A, X, L, gs, spec)
        self._end_step()
        return self._loss, Y

    # ---- gradients accumulated over several calls, one optimiser step (accumulate.py has the arithmetic) ----------------------

    @property
    def accumulated(self):
        """The calls in the open accumulation (a host int; 0: none is open)."""
        return self._acc.calls if self._acc is not None else 0

    @property
    def accumulated_count(self):
        """The labels the open accumulation has counted so far: a 0-dim int64 VIEW of the device value."""
        if self._acc is None:
            raise RuntimeError("windgnn_amd: TrainStep.accumulated_count is kept by accumulate / accumulate_series; no such call "
                               "has run on this TrainStep yet")
        return self._acc.count

    def _bucket_is_free(self, who):
        """step / step_series / forward_backward* / state_dict() / load_state_dict() while an accumulation is open."""
        if self.accumulated:
            raise RuntimeError("windgnn_amd: TrainStep.%s while an accumulation is open (%d call%s since the last apply() / "
                               "discard()): it writes or reads the gradient bucket and the step count that the accumulation owns "
                               "until its optimiser step; finish it with apply(), or drop it with discard(), first"
                               % (who, self.accumulated, "" if self.accumulated == 1 else "s"))

    def _no_frozen_group(self, who):
        if self.trainable != "all":
            raise RuntimeError("%s with trainable=%r: accumulation under a frozen group is not built (the accumulator adds whole "
                               "buckets, and its calls would have to share the group); take one step() per batch, or "
                               "set_trainable('all') first" % (who, self.trainable))

    def _accumulate_refusals(self, who, loss, huber_delta):
        """What accumulate / accumulate_series refuse on top of forward_backward*'s own refusals; returns the admit callback
        of _forward_backward*, which holds those that need the call's shape."""
        who = "windgnn_amd: TrainStep." + who
        self._no_frozen_group(who)
        one_bucket = ("an accumulation is final only at apply(), whose exchange and optimiser run on the one-bucket schedule; build "
                      "the TrainStep without it, or take one step() per batch")
        if self.plan is not None:
            raise RuntimeError("%s with grad_blocks: the blocked exchange steps row blocks of the GRU weights before the whole "
                               "bucket exists; %s" % (who, one_bucket))
        if self.overlap_collectives:
            raise RuntimeError("%s with overlap_collectives=True: that schedule steps the GRU tensors before the whole bucket "
                               "exists; %s" % (who, one_bucket))
        if self.carry_state:
            raise RuntimeError("%s with carry_state=True: that would be truncated BPTT with one optimiser step per k chunks, a "
                               "follow-up that is not built; take one step() per chunk, or build the TrainStep with "
                               "carry_state=False (every window starts from h = 0)" % who)

        def admit(windows, T, t_from):
            kind = self._loss_kind(loss, huber_delta)
            if windows == 0:
                raise RuntimeError("%s needs at least one window; a rank without windows skips the call and still calls apply() "
                                   "(the empty-shard form of the step)" % who)
            if self._acc_spec is None:
                return
            if kind != self._acc_spec[0]:
                was = "loss=%r" % self._acc_spec[0][0] + ("" if self._acc_spec[0][1] is None
                                                          else ", huber_delta=%r" % self._acc_spec[0][1])
                raise RuntimeError("%s: loss=%r, huber_delta=%r, but the open accumulation holds calls on %s: their sum would no "
                                   "longer be one loss; apply() or discard() first, or pass the same loss (huber_delta counts "
                                   "with loss='huber' only)" % (who, loss, huber_delta, was))
            if self.collective and (T, t_from) != self._acc_spec[1]:
                raise RuntimeError("%s under a process group: this call has (T, loss_from) = (%r, %r), the open accumulation's "
                                   "calls (%r, %r); a rank's weight in the exchange is its share of the WINDOWS, which is its share "
                                   "of the labels only while every window counts the same number of steps; apply() first, or "
                                   "accumulate calls of one (T, loss_from)" % ((who, T, t_from) + self._acc_spec[1]))
        return admit

    @staticmethod
    def _loss_kind(loss, huber_delta):
        """What the calls of one accumulation share of the loss (huber_delta counts with loss="huber" only)."""
        return loss, float(huber_delta) if loss == "huber" else None

    def _accumulate(self, kind, out, windows, T, t_from):
        """The add onto the accumulator after a forward_backward*: the last thing a call does, so a call that raises anywhere
        before leaves the accumulation as it was."""
        loss, Y, d, count = out
        if self._acc is None:
            self._acc = Accumulation(self._gbuf)
        self._acc.add(self._gbuf, count)
        if self._acc_spec is None:
            self._acc_spec, self._acc_windows = (kind, (T, t_from)), 0
        self._acc_d, self._acc_windows = d, self._acc_windows + windows
        return loss.clone(), Y          # (a clone: the header word is the next call's)

    def accumulate(self, A, X, L, *, loss="mse", huber_delta=1.0, loss_from=0, missing_labels=False):
        """forward_backward(A, X, L, ...) followed by an add onto the accumulator: no optimiser step, no collective.  apply()
        then takes ONE optimiser step on everything accumulated since the last apply() / discard(), exactly the step of one
        call on the union of the windows: the gradient of the mean loss over all counted labels of all calls (a call's weight is
        its count of labels -- with missing_labels the labels that exist, a device scalar -- not its windows).  Calls of this
        kind and accumulate_series may alternate; they must share loss / huber_delta.  Returns (this call's own loss as a
        0-dim clone, Y).  Refused: grad_blocks, overlap_collectives and carry_state (by name), and what forward_backward
        refuses; while an accumulation is open, step / step_series / forward_backward* / state_dict() / load_state_dict()."""
        admit = self._accumulate_refusals("accumulate", loss, huber_delta)
        out = self._forward_backward(A, X, L, loss, huber_delta, loss_from, missing_labels, admit)
        return self._accumulate(self._loss_kind(loss, huber_delta), out, X.shape[0], X.shape[1], int(loss_from))

    def accumulate_series(self, A, series, Ls, seq_len, stride=None, n_windows=None, starts=None, missing_labels=False,
                          loss="mse", huber_delta=1.0, loss_from=0, compact=False):
        """accumulate on the sliding windows of one series: forward_backward_series(...) followed by the same add (several
        series tensors -- sites, years, folds -- in one optimiser step; two seq_len on one rank).  compact: as in step_series,
        per call.  Returns (this call's own loss as a 0-dim clone, Y)."""
        admit = self._accumulate_refusals("accumulate_series", loss, huber_delta)
        out = self._forward_backward_series(A, series, Ls, seq_len, stride, n_windows, starts, missing_labels, loss,
                                            huber_delta, loss_from, admit, compact, "accumulate_series")
        return self._accumulate(self._loss_kind(loss, huber_delta), out, out[1].shape[0], int(seq_len), int(loss_from))

    def _tail_dims(self):
        """Dims for the optimiser's launch of a rank that has never run a forward: S, H and the math mode size it, as they
        size wgnn_keep_best's (B, T and the adjacency do not enter)."""
        return _lib.Dims(1, 1, self.params[4].shape[1] // 13, 13, self.params[5].shape[1], self.model.math, _lib.ADJ_CSR, 1,
                         _lib.IO_F32)

    def apply(self, n_global=None):
        """ONE optimiser step on everything accumulated since the last apply() / discard(): the bucket and the loss word become
        those of one call on the union (accumulate.py), then the tail of every step -- under a process group one all-reduce
        of the whole bucket, then wgnn_finish(0, adam) (wgnn_finish_norm + wgnn_finish_clipped with max_grad_norm), keep_best on
        the accumulated loss, `steps` + 1, the periodic check().  Returns the loss, the same 0-dim VIEW step() returns.
        n_global (process group): the windows of ALL ranks and ALL calls of this accumulation; None = the count collective, as
        in step().  A rank that accumulated nothing still calls apply(): zero bucket, weight 0, the same collectives.  On one
        rank apply() with nothing accumulated is refused.  An apply() that raises counts nothing and leaves the accumulation
        open; as after a step that raised, rebuild from a checkpoint rather than retry (discard() first: state_dict() is
        refused while it is open)."""
        self._no_frozen_group("windgnn_amd: TrainStep.apply()")
        n = self.accumulated
        if n == 0:
            if not self.collective:
                raise RuntimeError("windgnn_amd: TrainStep.apply(): nothing was accumulated since the last apply() / discard(); "
                                   "call accumulate() or accumulate_series() first (only under a process group does a rank "
                                   "without windows call apply() alone: it joins the collectives with a zero bucket)")
            d = self._acc_d if self._acc_d is not None else self._tail_dims()
            self._ensure_images(lambda: d)
            gs = self.exchange.shard_weight(0, n_global)               # 0.0; the count collective, if any, is issued
            self._gbuf.zero_()
        else:
            d = self._acc_d
            gs = self.exchange.shard_weight(self._acc_windows, n_global) if self.collective else 1.0
            self._acc.write(self._gbuf, LOSS_SLOT, gs)
        self._run_schedule(d, _FINAL, gs)       # the bucket is final: (the all-reduce,) Adam and the W_ih images
        self._end_step(check=n > 0)             # (an empty rank reads nothing from the device, as in _empty_shard_step)
        self.discard()
        return self._loss

    def discard(self):
        """Drop the open accumulation: parameters, moments, `steps` and the best record are untouched, nothing is launched
        (the next accumulation's first call overwrites the accumulator)."""
        if self._acc is not None:
            self._acc.reset()
        self._acc_spec, self._acc_windows = None, 0

    def close(self):
        """Release the step's own RCCL communicator, if it has one (before torch.distributed.destroy_process_group).
        Also runs from `with TrainStep(...) as tr:` and, as a last resort, from __del__."""
        ex = getattr(self, "exchange", None)
        if ex is not None and ex.direct is not None:
            ex.direct.close()
            ex.direct = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:           # interpreter shutdown: the library may be gone already
            pass

    def check(self):
        """Raise if a kernel of the fp16-plane modes reported a value outside fp16's range (one 4-byte read), or if the
        step's own RCCL communicator reported an asynchronous error (ncclCommGetAsyncError)."""
        if self.exchange is not None and self.exchange.direct is not None:
            self.exchange.direct.check()
        if self.model.math != _lib.MATH_F32:
            check_range_status(self.device)
