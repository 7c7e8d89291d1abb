"""Hourly forecasting with a carried GRU state: one new hour of readings advances the model by one GRU step
(wgnn_fwd_state, T = 1: one kernel launch in the common configuration) instead of re-running the window's prefix.

The reference forecasts from non-overlapping windows (src/step4_sequence_preparer.py:10-13) whose recurrence starts
from zeros (src/step6_gcn_gru_combined_model.py:23); row t of a window's output is the +1/+2/+3 h forecast made from hours
0..t of that window.  StreamingForecaster reproduces exactly those rows, hour by hour: its state resets every `window`
pushes (window=None carries it indefinitely)."""
from __future__ import annotations

from typing import Optional

import torch

from . import _lib
from .data import predict_last
from .functional import _require_gpu, check_range_status, gcn_gru_state


class StreamingForecaster:
    """StreamingForecaster(model, adj, wind_min, wind_max, n_streams=1, window=168)

    model: a GCN_GRU with the reference's 13 / 13 widths (its parameters are read at every push, so training it in
    between is seen); adj: its adjacency (dense [S,S] or graph.CsrAdjacency) on the GPU; n_streams: independent series
    (stations / sites) served together, each with its own state.  push(x_t) takes one hour, [n_streams,S,13] (or [S,13]
    for one stream), and returns the de-normalised forecast [n_streams, 3S]: columns [0:S] +1 h, [S:2S] +2 h, [2S:3S]
    +3 h (data.predict_last).  Inference only: no autograd."""

    def __init__(self, model, adj, wind_min: float, wind_max: float, n_streams: int = 1, window: Optional[int] = 168):
        if not getattr(model, "fused", False):
            raise RuntimeError("StreamingForecaster: the model must be a GCN_GRU with the reference's 13 / 13 widths")
        if n_streams < 1 or (window is not None and window < 1):
            raise RuntimeError("StreamingForecaster: n_streams and window must be >= 1 (got %d, %s)" % (n_streams, window))
        self.model, self.adj = model, adj
        self.wind_min, self.wind_max = float(wind_min), float(wind_max)
        self.n_streams, self.window = n_streams, window
        dev = model.gru.weight_hh_l0.device
        _require_gpu(model.gru.weight_hh_l0)
        H = model.gru.hidden_size
        # h0 and h_n of one call may not share memory: the state lives in two buffers used alternately
        self._h = [torch.zeros(n_streams, H, dtype=torch.float32, device=dev) for _ in range(2)]
        self._cur = 0
        self._count = 0            # pushes since the last reset

    def reset(self) -> None:
        """Start every stream from h = 0 again (the start of a reference window)."""
        self._count = 0

    @property
    def state(self) -> torch.Tensor:
        """The current hidden state [n_streams, H] (a copy; zeros right after a reset)."""
        if self._count == 0:
            return torch.zeros_like(self._h[self._cur])
        return self._h[self._cur].clone()

    @property
    def hours(self) -> int:
        """Hours pushed since the last (automatic or explicit) reset."""
        return self._count

    def push(self, x_t: torch.Tensor) -> torch.Tensor:
        if self.window is not None and self._count == self.window:
            self._count = 0                           # the next reference window starts here
        S = self.model.gru.input_size // 13
        if x_t.dim() == 2:
            x_t = x_t.unsqueeze(0)
        if tuple(x_t.shape) != (self.n_streams, S, 13):
            raise RuntimeError("StreamingForecaster.push: expected [%d, %d, 13] (or [%d, 13] for one stream), got %s"
                               % (self.n_streams, S, S, tuple(x_t.shape)))
        X = x_t.reshape(self.n_streams, 1, S, 13).contiguous()
        params = [p.detach() for p in self.model.hot_path_parameters()]
        h0 = self._h[self._cur] if self._count > 0 else None
        h_n = self._h[1 - self._cur]
        gcn_gru_state(self.adj, X, params, self.model.math, h0=h0, want_y=False, h_n=h_n)
        if self.model.validate and self.model.math != _lib.MATH_F32:
            check_range_status(h_n.device)
        self._cur = 1 - self._cur
        self._count += 1
        return predict_last(h_n.unsqueeze(1), self.wind_min, self.wind_max)   # T = 1: h_n is the output row
