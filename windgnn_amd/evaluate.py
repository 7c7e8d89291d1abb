"""The reference's test loop and its statistics (src/main.py:100-162) on the device: include/windgnn_eval.h behind an
`Evaluator` that never synchronises with the host until its figures are asked for.

    ev = Evaluator(model, adj, wind_min, wind_max)
    for batch_x, batch_y in test_loader:          # src/main.py:101
        pred = ev.update(batch_x, batch_y)        # forward_last + wgnn_eval_accum on the current stream
    r = ev.compute()                              # r.stats [3,S,4]: horizon, station, RMSE | MAE | accuracy mean | accuracy std
    one, two, three = ev.frames(stations)         # the reference's three DataFrames (one_hour.csv, ...)
"""
from __future__ import annotations

import ctypes as C
from typing import NamedTuple, Optional

import torch

from . import _lib
from .data import forward_last
from .functional import _ptr, _require_contiguous, _require_gpu, _require_scratch_aligned, _stream

COL_LABELS = ["RMSE", "MAE", "Average Accuracy", "Accuracy Deviation"]     # src/main.py:159


def eval_bytes(H: int) -> int:
    """wgnn_eval_bytes(H): bytes of the accumulator for H = 3S columns; 0 for H < 1."""
    return int(_lib.load().wgnn_eval_bytes(int(H)))


def eval_buffer(H: int, device) -> torch.Tensor:
    """A fresh, EMPTY accumulator (all zeros) as an fp64 tensor: [:5*H].view(5, H) is the public header, rows _lib.EVAL_ROWS
    (n, Σe², Σ|e|, Σa, Σa²); the rest is private to the library."""
    nbytes = eval_bytes(H)
    if nbytes == 0:
        _lib.check(-2, "wgnn_eval_bytes(%d)" % H)
    return torch.zeros(nbytes // 8, dtype=torch.float64, device=device)


def _acc_ptr(acc: torch.Tensor, H: int, need: int):
    if not acc.is_cuda or acc.dtype != torch.float64:
        raise RuntimeError("windgnn_amd: the evaluation accumulator is a float64 tensor on the GPU (eval_buffer), got %s on %s. "
                           "There is no CPU fallback." % (acc.dtype, acc.device))
    _require_contiguous(acc=acc)
    _require_scratch_aligned(acc=acc)
    if acc.numel() * 8 < need:
        raise RuntimeError("windgnn_amd: acc holds %d bytes, H = %d needs %d" % (acc.numel() * 8, H, need))
    return _ptr(acc)


def eval_accum(pred: torch.Tensor, labels: torch.Tensor, wind_min: float, wind_max: float, acc: torch.Tensor,
               abs_err: Optional[torch.Tensor] = None) -> None:
    """wgnn_eval_accum: add the windows of pred [B,H] (de-normalised) / labels [B,T,H] (normalised; row T-1 is read) to `acc`;
    abs_err [B,H] (optional) receives |truth - pred| as fp32."""
    lib = _lib.load()
    _require_gpu(pred, labels)
    _require_contiguous(pred=pred, labels=labels, abs_err=abs_err)
    if pred.dim() != 2 or labels.dim() != 3 or labels.shape[0] != pred.shape[0] or labels.shape[2] != pred.shape[1]:
        raise RuntimeError("windgnn_amd: eval_accum wants pred [B,H] and labels [B,T,H], got %s and %s"
                           % (tuple(pred.shape), tuple(labels.shape)))
    B, T, H = labels.shape
    if abs_err is not None:
        _require_gpu(abs_err)
        if tuple(abs_err.shape) != (B, H):
            raise RuntimeError("windgnn_amd: abs_err must be [%d,%d], got %s" % (B, H, tuple(abs_err.shape)))
    ap = _acc_ptr(acc, H, eval_bytes(H))
    _lib.check(lib.wgnn_eval_accum(_ptr(pred), _ptr(labels), B, T, H, float(wind_min), float(wind_max), ap, _ptr(abs_err),
                                   _stream()), "wgnn_eval_accum")


def eval_accum_series(pred: torch.Tensor, Ls: torch.Tensor, seq_len: int, wind_min: float, wind_max: float, acc: torch.Tensor,
                      stride: Optional[int] = 1, starts: Optional[torch.Tensor] = None, skip_missing: bool = False,
                      abs_err: Optional[torch.Tensor] = None) -> None:
    """wgnn_eval_accum_series: eval_accum with the truth of window b read at row b*stride + seq_len - 1 of the label SERIES
    Ls [ls_rows, H] (series.series_labels' first result) -- or, with `starts` (a contiguous int32 device tensor [B] in pred's
    order, stride None), at row starts[b] + seq_len - 1.  No [B, T, H] label tensor exists.  skip_missing: a NaN truth adds
    nothing to its column, whose count (header row n) is not incremented; abs_err gets NaN there."""
    lib = _lib.load()
    _require_gpu(pred, Ls)
    _require_contiguous(pred=pred, Ls=Ls, abs_err=abs_err, starts=starts)
    if pred.dim() != 2 or Ls.dim() != 2 or Ls.shape[1] != pred.shape[1]:
        raise RuntimeError("windgnn_amd: eval_accum_series wants pred [B,H] and Ls [ls_rows,H], got %s and %s"
                           % (tuple(pred.shape), tuple(Ls.shape)))
    B, H = pred.shape
    if starts is not None:
        if stride not in (None, 0):
            raise ValueError("eval_accum_series: pass stride= or starts=, not both (got stride=%r with a table of starts)" % (stride,))
        if not starts.is_cuda:
            raise RuntimeError("windgnn_amd runs on an MI355X (HIP) only: the table of starts is a %s tensor" % starts.device)
        if starts.dtype != torch.int32 or tuple(starts.shape) != (B,):
            raise ValueError("eval_accum_series: starts must be an int32 tensor of B = %d entries, got %s %s"
                             % (B, starts.dtype, tuple(starts.shape)))
        stride = 0
    elif stride is None or int(stride) < 1:
        raise ValueError("eval_accum_series: stride must be >= 1 without a table of starts, got %r" % (stride,))
    if abs_err is not None:
        _require_gpu(abs_err)
        if tuple(abs_err.shape) != (B, H):
            raise RuntimeError("windgnn_amd: abs_err must be [%d,%d], got %s" % (B, H, tuple(abs_err.shape)))
    ap = _acc_ptr(acc, H, eval_bytes(H))
    _lib.check(lib.wgnn_eval_accum_series(_ptr(pred), _ptr(Ls), Ls.shape[0], _ptr(starts), int(stride), B, int(seq_len), H,
                                          float(wind_min), float(wind_max), 1 if skip_missing else 0, ap, _ptr(abs_err),
                                          _stream()), "wgnn_eval_accum_series")


def eval_stats(acc: torch.Tensor, H: int, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """wgnn_eval_stats: [H,4] fp32 (RMSE, MAE, accuracy mean, accuracy std per column) from the header of `acc` -- an
    accumulator, or any fp64 tensor that starts with 5*H header doubles (a merged copy)."""
    lib = _lib.load()
    ap = _acc_ptr(acc, H, 5 * 8 * H)
    if out is None:
        out = torch.empty(H, 4, dtype=torch.float32, device=acc.device)
    _require_gpu(out)
    _require_contiguous(out=out)
    if out.numel() != 4 * H:
        raise RuntimeError("windgnn_amd: out must hold [%d,4] floats, got %s" % (H, tuple(out.shape)))
    _lib.check(lib.wgnn_eval_stats(ap, H, _ptr(out), _stream()), "wgnn_eval_stats")
    return out


def stats_frames(stats, stations):
    """The reference's one_hour / two_hour / three_hour DataFrames (src/main.py:159-162) from stats [3,S,4]: columns
    RMSE, MAE, Average Accuracy, Accuracy Deviation; index = stations.  `.to_csv("one_hour.csv")` as main.py:235."""
    import pandas as pd                                 # only here: the rest of the package does not need it
    a = torch.as_tensor(stats).detach().cpu().numpy()
    stations = list(stations)
    if a.ndim != 3 or a.shape[0] != 3 or a.shape[2] != 4 or a.shape[1] != len(stations):
        raise ValueError("stats_frames wants stats [3, %d, 4] for %d stations, got %s" % (len(stations), len(stations), a.shape))
    return tuple(pd.DataFrame(a[k], columns=COL_LABELS, index=stations) for k in range(3))


class EvalResult(NamedTuple):
    stats: torch.Tensor            # [3,S,4] fp32: horizon, station, (RMSE, MAE, accuracy mean, accuracy std)
    count: torch.Tensor            # 0-dim int64: windows accumulated (over all ranks with a process group).  Counts are kept PER
                                   # COLUMN (header[0]); this is column 0's.  The columns differ only after update_series(...,
                                   # skip_missing=True), where a NaN truth is not counted: read header[0] there
    mse_normalised: torch.Tensor   # [3] fp64: Σe² / (n S (wind_max - wind_min)²) per horizon, the training loss's units
    header: torch.Tensor           # [5,H] fp64: the sums the figures came from (merged over the ranks)


class Evaluator:
    """Device-side replacement of src/main.py:100-162.  Nothing synchronises with the host before the caller reads a result."""

    def __init__(self, model, adj, wind_min: float, wind_max: float, keep_errors: bool = False, process_group=None):
        self.model, self.adj = model, adj
        self.wind_min, self.wind_max = float(wind_min), float(wind_max)
        self.keep_errors = bool(keep_errors)
        self.process_group = process_group
        self.H = int(model.gru.hidden_size)
        if self.H % 3 != 0:
            raise ValueError("Evaluator: the model's %d outputs are not 3 horizons x S stations" % self.H)
        self.S = self.H // 3
        self.device = next(model.parameters()).device
        self.acc = None                                  # allocated by the first update / compute: an all-zero buffer is empty
        self._errors = []

    def _acc(self) -> torch.Tensor:
        if self.acc is None:
            self.acc = eval_buffer(self.H, self.device)
        return self.acc

    def update(self, batch_x: torch.Tensor, batch_y: torch.Tensor) -> torch.Tensor:
        """forward_last(model, adj, batch_x) followed by wgnn_eval_accum against batch_y ([T,3S], [1,T,3S] or [B,T,3S]); returns
        forward_last's tensor ([B,3S]; [3S] at B = 1).  A batch of no windows (an empty shard) is a no-op."""
        labels = batch_y.unsqueeze(0) if batch_y.dim() == 2 else batch_y
        if batch_x.shape[0] == 0:
            return torch.empty(0, self.H, dtype=torch.float32, device=batch_x.device)
        pred = forward_last(self.model, self.adj, batch_x, self.wind_min, self.wind_max)
        p2 = pred.reshape(-1, self.H)                    # (a view: forward_last's tensor is contiguous)
        err = torch.empty_like(p2) if self.keep_errors else None
        eval_accum(p2, labels.contiguous(), self.wind_min, self.wind_max, self._acc(), err)
        if err is not None:
            self._errors.append(err)
        return pred

    def update_series(self, series: torch.Tensor, Ls: torch.Tensor, seq_len: int, stride: Optional[int] = None, n_windows=None,
                      starts=None, skip_missing: bool = False, compact=False) -> torch.Tensor:
        """The rolling backtest on ONE series: series.forward_last_series(model, adj, series, seq_len, ...) followed by
        wgnn_eval_accum_series against the label series Ls [ls_rows, 3S] (series.series_labels' first result: the truth of a
        window that starts at row s is row s + seq_len - 1).  Returns the [n, 3S] forecasts in the caller's order (starts= in any
        order, duplicates allowed; otherwise stride, default 1, and n_windows).  No [n, T, 3S] label tensor is built and nothing
        synchronises with the host.  skip_missing=True: a NaN in Ls is "no truth here" -- that station and horizon is left out of
        this window's sums and of its column's count, so the counts differ per column (compute().header[0]; compute().count is
        column 0's); a column that never saw a truth has count 0 and NaN figures.  compact (with starts= only): the forecasts'
        front end on the covered hours alone, as in TrainStep.step_series; the truths are still looked up in Ls at the
        caller's starts."""
        from .series import _no_stride_with_starts, _starts_table, forward_last_series
        _no_stride_with_starts("Evaluator.update_series", stride, starts, n_windows)
        seq_len = int(seq_len)
        pred = forward_last_series(self.model, self.adj, series, seq_len, self.wind_min, self.wind_max, stride, n_windows, starts,
                                   **({} if compact is False else {"compact": compact}))
        table = None
        if starts is not None:      # in the caller's order, as the rows of pred are (the kernel only looks the table up)
            table = _starts_table(starts, series.shape[0], seq_len, series.device, "Evaluator.update_series", ordered=False)
        step = None if starts is not None else int(1 if stride is None else stride)
        need = series.shape[0] if starts is not None else (pred.shape[0] - 1) * step + seq_len
        if Ls.dim() != 2 or Ls.shape[1] != self.H or Ls.shape[0] < need:
            raise RuntimeError("windgnn_amd: Evaluator.update_series: the label series Ls must be [rows >= %d, H = %d], got %s"
                               % (need, self.H, tuple(Ls.shape)))
        err = torch.empty_like(pred) if self.keep_errors else None
        eval_accum_series(pred, Ls.contiguous(), seq_len, self.wind_min, self.wind_max, self._acc(), step, table, skip_missing,
                          err)
        if err is not None:
            self._errors.append(err)
        return pred

    def errors(self) -> torch.Tensor:
        """[N,3S] fp32: |truth - pred| of every window seen, in order (keep_errors=True); the rows of the reference's box plots."""
        if not self.keep_errors:
            raise RuntimeError("Evaluator(keep_errors=False) kept no error rows")
        if not self._errors:
            return torch.empty(0, self.H, dtype=torch.float32, device=self.device)
        return torch.cat(self._errors, dim=0)

    def compute(self) -> EvalResult:
        """The figures of everything accumulated so far.  With a process group: a SUM all-reduce of a COPY of the header (every
        rank calls this, a rank that saw no window included); the local accumulator stays as it is."""
        H = self.H
        header = self._acc()[:5 * H]
        if self.process_group is not None:
            import torch.distributed as dist
            header = header.clone()
            dist.all_reduce(header, group=self.process_group)
        stats = eval_stats(header, H).view(3, self.S, 4)
        rows = header.view(5, 3, self.S)
        wrange = float(torch.tensor(self.wind_max, dtype=torch.float32)) - float(torch.tensor(self.wind_min, dtype=torch.float32))
        mse = rows[1].sum(dim=1) / (rows[0].sum(dim=1) * (wrange * wrange))
        return EvalResult(stats, header[0].to(torch.int64), mse, header.view(5, H))

    def frames(self, stations):
        """(one_hour, two_hour, three_hour) pandas DataFrames with the reference's columns and index (src/main.py:159-162)."""
        return stats_frames(self.compute().stats, stations)

    def reset(self) -> None:
        if self.acc is not None:
            self.acc.zero_()
        self._errors = []
