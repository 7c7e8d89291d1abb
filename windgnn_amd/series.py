"""Series mode (include/windgnn_series.h): the model on every sliding window of ONE hourly series, without building the
windows.

Window w = 0 .. n-1 covers rows w*stride .. w*stride + T - 1 of `series` [rows, S, 13] and starts from h = 0; the results are
those of GCN_GRU.forward on the materialised windows (make_windows(starts=...)).  What depends on the hour alone -- both graph
convolutions and the GRU's input projection -- runs once per hour instead of once per window and hour.

Exact fp32 with a dense adjacency (S <= 64) and H <= 128 only; everything else raises and names the materialised path."""
from __future__ import annotations

import ctypes as C
from typing import List, Sequence, Tuple

import torch

from . import _lib
from .functional import (_adj, _flat_grads, _params_struct, _ptr, _require_contiguous, _require_gpu, _stash_ptr, _stream,
                         _workspace)

_MATERIALISED = ("materialise the windows (windgnn_amd.data.make_windows(feat, seq_len, starts=...)) and call "
                 "GCN_GRU.forward / forward_last on them instead")


def n_series_windows(rows: int, seq_len: int, stride: int = 1) -> int:
    """Windows of seq_len rows, `stride` rows apart, that fit into a series of `rows` rows (0 if none does)."""
    if seq_len < 1 or stride < 1:
        raise ValueError("n_series_windows: seq_len and stride must be >= 1, got %d and %d" % (seq_len, stride))
    return 0 if rows < seq_len else (rows - seq_len) // stride + 1


def series_coverage(rows: int, seq_len: int, stride: int, n: int) -> List[Tuple[int, int]]:
    """Per series row tau the inclusive range (w_lo, w_hi) of the windows that cover it -- w*stride <= tau < w*stride +
    seq_len, 0 <= w < n -- in the closed form the fold kernel of the backward uses; w_lo > w_hi: no window covers the row
    (a gap when stride > seq_len, or a spare trailing row) and its gate gradient is zero.  Plain Python, no device."""
    if n < 1 or stride < 1 or seq_len < 1 or (n - 1) * stride + seq_len > rows:
        raise ValueError("series_coverage: %d windows of %d rows, %d apart, do not fit into %d rows" % (n, seq_len, stride, rows))
    out = []
    for tau in range(rows):
        w_hi = min(tau // stride, n - 1)
        w_lo = (tau - seq_len) // stride + 1 if tau >= seq_len else 0
        out.append((w_lo, w_hi))
    return out


def _series_setup(A, series, seq_len: int, stride: int, params: Sequence[torch.Tensor], math: int, n_windows=None):
    """Everything a series call checks and sizes before it launches: (adjacency, dims, workspace, workspace bytes)."""
    if hasattr(A, "blob"):
        raise RuntimeError("windgnn_amd: series mode takes a dense adjacency (S <= 64), not a CsrAdjacency: " + _MATERIALISED)
    if math != _lib.MATH_F32:
        raise RuntimeError("windgnn_amd: series mode runs in exact fp32 (math='f32') only, not in the fp16-plane modes "
                           "(f16x3 / f16x3g / f16): " + _MATERIALISED)
    _require_gpu(series)
    _require_gpu(*params)
    _require_contiguous(series=series, params=params)
    if series.dim() != 3:
        raise RuntimeError("windgnn_amd: series must be [rows, S, 13], got %s" % (tuple(series.shape),))
    rows, S, F = series.shape
    fit = n_series_windows(rows, seq_len, stride)
    if fit < 1:
        raise RuntimeError("windgnn_amd: no window of %d rows fits into a series of %d rows" % (seq_len, rows))
    n = fit if n_windows is None else int(n_windows)
    if n < 1 or n > fit:
        raise RuntimeError("windgnn_amd: n_windows = %d, but a series of %d rows holds 1 .. %d windows of %d rows at stride %d"
                           % (n, rows, fit, seq_len, stride))
    A, fmt, nnz = _adj(A, S)
    H = params[5].shape[1]
    sd = _lib.SeriesDims(rows, seq_len, stride, n, S, F, H, math, fmt, nnz, _lib.IO_F32)
    ws, ws_bytes = _workspace(sd, series.device,
                              refused="wgnn_series_workspace_bytes(rows=%d,T=%d,stride=%d,n=%d,S=%d,F=%d,H=%d) [%s]"
                              % (rows, seq_len, stride, n, S, F, H, _MATERIALISED))
    return A, sd, ws, ws_bytes


def series_forward_raw(A, series, seq_len, stride, params, math=_lib.MATH_F32, want_stash=True, n_windows=None):
    """Y [n, T, H], stash, dims = wgnn_series_fwd(...).  n_windows: the first that many windows (default: all that fit)."""
    lib = _lib.load()
    A, sd, ws, ws_bytes = _series_setup(A, series, seq_len, stride, params, math, n_windows)
    stash = (torch.empty(lib.wgnn_series_stash_bytes(C.byref(sd)), dtype=torch.uint8, device=series.device)
             if want_stash else None)
    Y = torch.empty(sd.n, sd.T, sd.H, dtype=torch.float32, device=series.device)
    ps = _params_struct(_lib.Params, params)
    rc = lib.wgnn_series_fwd(C.byref(sd), _ptr(A), _ptr(series), C.byref(ps), _ptr(Y), _stash_ptr(stash), _ptr(ws), ws_bytes,
                             _stream())
    _lib.check(rc, "wgnn_series_fwd")
    return Y, stash, sd


def series_backward_raw(sd, A, series, params, Y, dY, stash, grads: Sequence[torch.Tensor]) -> None:
    """wgnn_series_bwd: the 8 gradients of sum(Y * dY), summed over all windows, into `grads` (overwritten)."""
    lib = _lib.load()
    _require_contiguous(series=series, Y=Y, dY=dY, adj_matrix=A, grads=grads, params=params)
    ws, ws_bytes = _workspace(sd, series.device)
    ps = _params_struct(_lib.Params, params)
    gs = _params_struct(_lib.Grads, grads)
    rc = lib.wgnn_series_bwd(C.byref(sd), _ptr(A), _ptr(series), C.byref(ps), _ptr(Y), _ptr(dY), _stash_ptr(stash), C.byref(gs),
                             _ptr(ws), ws_bytes, _stream())
    _lib.check(rc, "wgnn_series_bwd")


def _check_label_series(Ls, sd) -> None:
    """Ls as series_labels returns it: contiguous [rows, H] fp32 on the GPU with a row for every hour a window covers."""
    need = (sd.n - 1) * sd.stride + sd.T
    if Ls.dim() != 2 or Ls.shape[1] != sd.H or Ls.shape[0] < need:
        raise RuntimeError("windgnn_amd: the label series Ls must be [rows >= (n - 1) * stride + seq_len = %d, H = %d] (what "
                           "series_labels(feat, seq_len, stride, n_windows)[0] returns; its window view L is not needed), got %s"
                           % (need, sd.H, tuple(Ls.shape)))
    _require_gpu(Ls)
    _require_contiguous(Ls=Ls)


def series_forward_loss_raw(A, series, Ls, seq_len, stride, params, math=_lib.MATH_F32, n_windows=None, prepared=None):
    """Y [n, T, H], stash, loss_buf, dims = wgnn_series_fwd_loss(...): series_forward_raw with the MSE statistics of (Y - labels)
    left in loss_buf for series_backward_mse_raw.  Ls [rows - 3, H]: the label SERIES (series_labels' first result); window w,
    step t reads its row w * stride + t."""
    lib = _lib.load()
    A, sd, ws, ws_bytes = _series_setup(A, series, seq_len, stride, params, math, n_windows)
    _check_label_series(Ls, sd)
    stash = torch.empty(lib.wgnn_series_stash_bytes(C.byref(sd)), dtype=torch.uint8, device=series.device)
    loss_buf = torch.empty(lib.wgnn_series_loss_bytes(C.byref(sd)) // 4, dtype=torch.float32, device=series.device)
    Y = torch.empty(sd.n, sd.T, sd.H, dtype=torch.float32, device=series.device)
    ps = _params_struct(_lib.Params, params, prepared)
    rc = lib.wgnn_series_fwd_loss(C.byref(sd), _ptr(A), _ptr(series), C.byref(ps), _ptr(Ls), Ls.shape[0], _ptr(Y),
                                  _stash_ptr(stash), _ptr(loss_buf), _ptr(ws), ws_bytes, _stream())
    _lib.check(rc, "wgnn_series_fwd_loss")
    return Y, stash, loss_buf, sd


def series_backward_mse_raw(sd, A, series, params, Y, Ls, stash, loss_buf, grads: Sequence[torch.Tensor], loss: torch.Tensor,
                            grad_scale: float = 1.0, prepared=None) -> None:
    """wgnn_series_bwd_mse: the 8 gradients of grad_scale * mean((Y - labels)^2) into `grads` (overwritten, final) and the
    unweighted mean into `loss` (a 0-dim fp32 device tensor), without a dY tensor.  Y, stash, loss_buf: as
    series_forward_loss_raw returned them for the same inputs."""
    lib = _lib.load()
    _check_label_series(Ls, sd)
    _require_gpu(loss, loss_buf)
    _require_contiguous(series=series, Y=Y, adj_matrix=A, loss_buf=loss_buf, grads=grads, params=params)
    if loss_buf.numel() * 4 < lib.wgnn_series_loss_bytes(C.byref(sd)):
        raise RuntimeError("windgnn_amd: loss_buf holds %d bytes, wgnn_series_loss_bytes says %d"
                           % (loss_buf.numel() * 4, lib.wgnn_series_loss_bytes(C.byref(sd))))
    ws, ws_bytes = _workspace(sd, series.device)
    ps = _params_struct(_lib.Params, params, prepared)
    gs = _params_struct(_lib.Grads, grads)
    rc = lib.wgnn_series_bwd_mse(C.byref(sd), _ptr(A), _ptr(series), C.byref(ps), _ptr(Y), _ptr(Ls), Ls.shape[0],
                                 float(grad_scale), _stash_ptr(stash), _ptr(loss_buf), _ptr(loss), C.byref(gs), _ptr(ws), ws_bytes,
                                 _stream())
    _lib.check(rc, "wgnn_series_bwd_mse")


class SeriesFunction(torch.autograd.Function):
    """Y [n, T, H] = GCN_GRU on every window of the series.  Gradients flow to the 8 parameters only, as in GCNGRUFunction."""

    @staticmethod
    def forward(ctx, A, series, seq_len, stride, n_windows, math, *params):
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[0]:
            raise RuntimeError("windgnn_amd: series mode gives gradients for the 8 parameters only; a series / adj_matrix "
                               "with requires_grad=True is not supported (detach it)")
        series = series.contiguous()
        params = tuple(p.contiguous() for p in params)
        need = any(ctx.needs_input_grad[6:])
        Y, stash, sd = series_forward_raw(A, series, seq_len, stride, params, math, want_stash=need, n_windows=n_windows)
        ctx.sd = sd
        ctx.save_for_backward(_adj(A)[0], series, Y, stash, *params)
        return Y

    @staticmethod
    def backward(ctx, dY):
        A, series, Y, stash, *params = ctx.saved_tensors
        if stash is None:
            raise RuntimeError("windgnn_amd: backward called but the forward ran without a stash")
        grads = _flat_grads(params, series.device)
        series_backward_raw(ctx.sd, A, series, params, Y, dY.float().contiguous(), stash, grads)
        return (None, None, None, None, None, None, *grads)


def gcn_gru_series(A, series, seq_len: int, stride: int, params, math=_lib.MATH_F32, n_windows=None):
    """Y [n, seq_len, H] for the first n = n_windows (default: all n_series_windows(rows, seq_len, stride)) windows of series
    [rows, S, 13]."""
    return SeriesFunction.apply(A, series, int(seq_len), int(stride), n_windows, math, *params)


def _require_fused(model, who: str) -> None:
    if not getattr(model, "fused", False):
        raise RuntimeError("%s: series mode is built for the reference model's 13 / 13 widths only (got input_dim / "
                           "hidden_dim = %d / %d): %s" % (who, model.conv1.weight.shape[0], model.conv1.weight.shape[1],
                                                          _MATERIALISED))


def forward_last_series(model, adj_matrix, series: torch.Tensor, seq_len: int, wind_min: float, wind_max: float,
                        stride: int = 1, n_windows=None) -> torch.Tensor:
    """The rolling backtest: [n, 3S] de-normalised forecasts, one per window, each from its own zero-state seq_len-hour
    window (wgnn_series_fwd_last; no Y is written).  The rows are what forward_last gives on the materialised windows and feed
    evaluate.eval_accum as they are."""
    lib = _lib.load()
    _require_fused(model, "forward_last_series")
    params = [p.detach().contiguous() for p in model.hot_path_parameters()]
    series = series.contiguous()
    A, sd, ws, ws_bytes = _series_setup(adj_matrix, series, int(seq_len), int(stride), params, model.math, n_windows)
    out = torch.empty(sd.n, sd.H, dtype=torch.float32, device=series.device)
    ps = _params_struct(_lib.Params, params)
    rc = lib.wgnn_series_fwd_last(C.byref(sd), _ptr(A), _ptr(series), C.byref(ps), float(wind_min), float(wind_max), _ptr(out),
                                  _ptr(ws), ws_bytes, _stream())
    _lib.check(rc, "wgnn_series_fwd_last")
    return out


def series_labels(feat: torch.Tensor, seq_len: int, stride: int = 1, n_windows: int = None):
    """(Ls, L): the labels of series mode.  A label row depends on the hour alone, Ls[tau] = [y[tau+1] | y[tau+2] | y[tau+3]]
    with y = feat[:, :, LABEL_FEATURE] (src/step4_sequence_preparer.py:14-19), so Ls [rows - 3, 3S] is built once and
    L [n, seq_len, 3S] is a VIEW of it (unfold: no copy), window-major like forward_series's output.  n = n_windows, or every
    window of seq_len rows that fits into feat (make_windows' count at stride = seq_len).  Works on any device.
    Raises where the last window's +3 h label does not fit into feat -- e.g. train on forward_series(adj, feat[:-3], ...) with
    series_labels(feat, ..., n_windows=n_series_windows(len(feat) - 3, seq_len, stride))."""
    from .data import LABEL_FEATURE
    if feat.dim() != 3:
        raise RuntimeError("windgnn_amd.series_labels: feat must be [rows, S, 13], got %s" % (tuple(feat.shape),))
    rows = feat.shape[0]
    n = n_series_windows(rows, seq_len, stride) if n_windows is None else int(n_windows)
    if n < 1 or (n - 1) * stride + seq_len + 3 > rows:
        raise RuntimeError("windgnn_amd.series_labels: the last of the %d windows of %d rows (stride %d) ends at row %d and "
                           "its +3 h label needs row %d, but feat has %d rows: ask for fewer windows (n_windows) or pass a "
                           "longer feat" % (n, seq_len, stride, (n - 1) * stride + seq_len - 1,
                                            (n - 1) * stride + seq_len + 2, rows))
    y = feat[:, :, LABEL_FEATURE]
    Ls = torch.cat([y[1:rows - 2], y[2:rows - 1], y[3:rows]], dim=1)          # [rows - 3, 3S]
    return Ls, Ls.unfold(0, seq_len, stride)[:n].permute(0, 2, 1)
