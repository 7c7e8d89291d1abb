"""Drop-in nn.Modules with the reference's names, constructor arguments, forward signatures and
state_dict keys, backed by the HIP library.

  GraphConvLayer(input_dim, output_dim)                         src/step5_gcn_layer_model.py:5-23
  GCN_GRU(input_dim, hidden_dim, output_dim, gru_input,
          gru_hidden_dim).forward(adj_matrix, attr_matrix)      src/step6_gcn_gru_combined_model.py:6-27
"""
from __future__ import annotations

import math

import torch
import torch.nn as nn

from . import _lib
from .functional import GraphConvFunction, GRUFunction, check_range_status, gcn_gru, gcn_gru_state, gcn_gru_with_state

NUM_FEATURES = 13   # hard-coded in the reference: src/step6_gcn_gru_combined_model.py:16


class GraphConvLayer(nn.Module):
    """The reference's constructor domain (src/step5_gcn_layer_model.py:6-10): any input_dim -> output_dim.  13 -> 13, the only
    widths its model builds (src/main.py:41), run the MFMA kernels of gcn.hip; other widths, over a dense adjacency of S <= 64, exact-fp32
    kernels of their own (up to 64 features gcn_any.hip, wider layers the tiled fp32-MFMA kernels of gcn_wide.hip); more than 64
    stations over a dense adjacency, or other widths than 13 -> 13 over a CSR one, raise at the first forward."""

    def __init__(self, input_dim, output_dim):
        super().__init__()
        self.weight = nn.Parameter(torch.randn(input_dim, output_dim))   # step5:8-9
        self.bias = nn.Parameter(torch.zeros(output_dim))                # step5:10

    def forward(self, adj_matrix, attr_matrix):
        return GraphConvFunction.apply(adj_matrix, attr_matrix, self.weight, self.bias)


class _GRUParams(nn.Module):
    """Holds the four nn.GRU tensors under the reference's names (weight_ih_l0 ...), with
    nn.GRU's U(-1/sqrt(H), 1/sqrt(H)) initialisation."""

    def __init__(self, input_size, hidden_size):
        super().__init__()
        self.input_size, self.hidden_size = input_size, hidden_size
        k = 1.0 / math.sqrt(hidden_size)
        self.weight_ih_l0 = nn.Parameter(torch.empty(3 * hidden_size, input_size).uniform_(-k, k))
        self.weight_hh_l0 = nn.Parameter(torch.empty(3 * hidden_size, hidden_size).uniform_(-k, k))
        self.bias_ih_l0 = nn.Parameter(torch.empty(3 * hidden_size).uniform_(-k, k))
        self.bias_hh_l0 = nn.Parameter(torch.empty(3 * hidden_size).uniform_(-k, k))


class GCN_GRU(nn.Module):
    """forward(adj_matrix [S,S], attr_matrix [1,T,S,13]) -> [T, gru_hidden_dim], exactly the
    reference's contract.  Extensions: attr_matrix [B,T,S,13] with B > 1 returns [B,T,H] (B independent windows,
    h0 = 0 each); a float16 / bfloat16 attr_matrix (math "f16x3" or "f16" only) is read as such and the output comes
    back in the same type (16-bit I/O, BASELINE's 16-bit configuration) -- parameters and gradients stay fp32."""

    def __init__(self, input_dim, hidden_dim, output_dim, gru_input, gru_hidden_dim, math="f32", validate=True):
        super().__init__()
        # validate: in the fp16-plane modes read the library's range-status word after every forward (one 4-byte
        # device-to-host copy) and raise instead of returning inf/NaN-derived values; TrainStep checks every N steps
        self.validate = validate
        # The reference's forward flattens conv2's output with a hard-coded 13 (step6:16): output_dim != 13 fails there at the
        # first call (its .view), here at construction.  input_dim / hidden_dim are free (step6:9-10); at 13 / 13 -- the model
        # src/main.py:41 builds -- the whole forward / backward is the fused hot path, at other widths it is two general
        # GraphConvLayers + the recurrent half alone (wgnn_gru_fwd / wgnn_gru_bwd), in exact fp32.
        if output_dim != NUM_FEATURES:
            raise RuntimeError("GCN_GRU: output_dim must be 13: forward() flattens conv2's output as num_stations * 13 "
                               "(src/step6_gcn_gru_combined_model.py:16,20); got output_dim = %d" % output_dim)
        self.fused = input_dim == NUM_FEATURES and hidden_dim == NUM_FEATURES
        if not self.fused and math != "f32":
            raise RuntimeError("GCN_GRU(input_dim=%d, hidden_dim=%d): widths other than 13 run in exact fp32 only "
                               "(math='f32'), got math=%r" % (input_dim, hidden_dim, math))
        self.conv1 = GraphConvLayer(input_dim, hidden_dim)
        self.conv2 = GraphConvLayer(hidden_dim, output_dim)
        self.gru = _GRUParams(gru_input, gru_hidden_dim)
        self.math = {"f32": _lib.MATH_F32, "f16x3": _lib.MATH_F16X3, "f16": _lib.MATH_F16, "f16x3g": _lib.MATH_F16X3G}[math]

    def hot_path_parameters(self):
        return (self.conv1.weight, self.conv1.bias, self.conv2.weight, self.conv2.bias,
                self.gru.weight_ih_l0, self.gru.weight_hh_l0, self.gru.bias_ih_l0, self.gru.bias_hh_l0)

    def forward(self, adj_matrix, attr_matrix):
        if attr_matrix.dim() != 4:
            raise RuntimeError("GCN_GRU.forward: attr_matrix must be [B, T, S, 13], got %s" % (tuple(attr_matrix.shape),))
        B, T, S, F = attr_matrix.shape
        flat = S * NUM_FEATURES
        if not self.fused:
            if flat != self.gru.input_size:
                raise RuntimeError("shape '[%d, %d, %d]' is invalid for input of size %d"
                                   % (B, T, self.gru.input_size, B * T * flat))
            hidden1 = self.conv1(adj_matrix, attr_matrix)                               # step6:17
            hidden2 = self.conv2(adj_matrix, hidden1).view(B, T, flat)                  # step6:20
            out = GRUFunction.apply(hidden2, S, self.gru.weight_ih_l0, self.gru.weight_hh_l0, self.gru.bias_ih_l0,
                                    self.gru.bias_hh_l0)                                 # step6:23
            return out.squeeze(0)                                                        # step6:26
        if F != NUM_FEATURES or flat != self.gru.input_size:
            # mirrors the reference's .view(1, num_seq, flat) failure (step6:20)
            raise RuntimeError("shape '[%d, %d, %d]' is invalid for input of size %d"
                               % (B, T, self.gru.input_size, attr_matrix.numel()))
        out = gcn_gru(adj_matrix, attr_matrix, self.hot_path_parameters(), self.math)
        if self.validate and self.math != _lib.MATH_F32:
            check_range_status(out.device)
        return out.squeeze(0)            # step6:26

    def forward_series(self, adj_matrix, series, seq_len, stride=None, n_windows=None, starts=None, compact=False):
        """[n, seq_len, gru_hidden_dim]: forward() on every window of `series` [rows, S, 13] -- window w covers rows
        w*stride .. w*stride + seq_len - 1, n = n_windows or (rows - seq_len) // stride + 1, h0 = 0 each -- without building them:
        the graph convolutions and the input projection run once per hour (windgnn_amd/series.py).  Differentiable in the
        parameters.  The reference model's 13 / 13 widths in exact fp32 with a dense adjacency only; raises otherwise.
        stride defaults to 1.  starts (instead of stride / n_windows): a list or tensor of window start rows in ANY order,
        duplicates allowed (series.segment_starts: the windows inside clean segments; a hold-out; a shuffled mini-batch); row i
        of the result is the window at starts[i].  The table is sorted on the device without a synchronisation, and the
        parameter gradients do not depend on its order.  A host table is checked before the upload (ValueError); a device
        table by the kernel (check_range_status).  compact (with starts= only; False | True | "auto" | an int bound on the covered
        hours, as in TrainStep.step_series): the graph convolutions and the input projection run on the hours some window
        covers alone -- the gather of those rows sits outside the autograd function, and the series takes no gradient."""
        from .series import _compact_arg, _no_stride_with_starts, _require_fused, compacted_starts, gcn_gru_series
        _require_fused(self, "GCN_GRU.forward_series")
        if series.dim() != 3 or series.shape[2] != NUM_FEATURES or series.shape[1] * NUM_FEATURES != self.gru.input_size:
            raise RuntimeError("GCN_GRU.forward_series: series must be [rows, %d, 13], got %s"
                               % (self.gru.input_size // NUM_FEATURES, tuple(series.shape)))
        _no_stride_with_starts("GCN_GRU.forward_series", stride, starts, n_windows)
        _compact_arg("GCN_GRU.forward_series", compact, starts, stride)
        if starts is None:
            return gcn_gru_series(adj_matrix, series, seq_len, 1 if stride is None else stride, self.hot_path_parameters(),
                                  self.math, n_windows)
        series, _, table, inverse = compacted_starts(starts, series, None, int(seq_len), "GCN_GRU.forward_series", compact)
        Y = gcn_gru_series(adj_matrix, series, seq_len, None, self.hot_path_parameters(), self.math, starts=table)
        return Y if inverse is None else Y.index_select(0, inverse)

    def forward_state(self, adj_matrix, attr_matrix, hx=None):
        """(out, h_n) with nn.GRU(batch_first=True)'s state convention: hx / h_n are [1, B, H] (hx may also be [B, H]; None =
        zeros, i.e. exactly forward()); out is what forward() returns.  Inference only: no autograd graph is built, so with
        grad mode on and a parameter or hx requiring grad it raises instead of dropping the gradients.  h_n is the unrounded
        fp32 state also with a 16-bit attr_matrix."""
        if torch.is_grad_enabled() and (any(p.requires_grad for p in self.hot_path_parameters()) or
                                        (hx is not None and hx.requires_grad)):
            raise RuntimeError("GCN_GRU.forward_state is inference only (no gradients flow through the carried state): "
                               "call it under torch.no_grad() (or torch.inference_mode()), or train through "
                               "GCN_GRU.forward_with_state")
        hx = self._check_state("forward_state", attr_matrix, hx)
        h0 = hx.detach().contiguous() if hx is not None else None
        params = [p.detach().contiguous() for p in self.hot_path_parameters()]
        out, h_n = gcn_gru_state(adj_matrix, attr_matrix.contiguous(), params, self.math, h0=h0)
        if self.validate and self.math != _lib.MATH_F32:
            check_range_status(out.device)
        return out.squeeze(0), h_n.unsqueeze(0)

    def _check_state(self, who, attr_matrix, hx):
        """hx as [B, H] (or None) after the checks both carried-state methods make."""
        if not self.fused:
            raise RuntimeError("GCN_GRU.%s: carried state is built for the reference model's 13 / 13 widths only "
                               "(got input_dim / hidden_dim = %d / %d)" % (who, self.conv1.weight.shape[0],
                                                                           self.conv1.weight.shape[1]))
        if attr_matrix.dim() != 4:
            raise RuntimeError("GCN_GRU.%s: attr_matrix must be [B, T, S, 13], got %s" % (who, tuple(attr_matrix.shape)))
        B, T, S, F = attr_matrix.shape
        if F != NUM_FEATURES or S * NUM_FEATURES != self.gru.input_size:
            raise RuntimeError("shape '[%d, %d, %d]' is invalid for input of size %d"
                               % (B, T, self.gru.input_size, attr_matrix.numel()))
        H = self.gru.hidden_size
        if hx is None:
            return None
        if tuple(hx.shape) == (1, B, H):
            hx = hx[0]
        if tuple(hx.shape) != (B, H):
            raise RuntimeError("GCN_GRU.%s: hx must be [1, B, H] or [B, H] = [1, %d, %d], got %s"
                               % (who, B, H, tuple(hx.shape)))
        if hx.dtype != torch.float32 or hx.device != attr_matrix.device:
            raise RuntimeError("GCN_GRU.%s: hx must be float32 on %s, got %s on %s"
                               % (who, attr_matrix.device, hx.dtype, hx.device))
        return hx

    def forward_with_state(self, adj_matrix, attr_matrix, hx=None):
        """(out, h_n) with nn.GRU(batch_first=True)'s full state semantics, training included: hx / h_n are [1, B, H] (hx may
        also be [B, H]; None = zeros).  Gradients flow to the parameters and to hx, and a loss may use out, h_n or both
        (truncated BPTT: feed h_n.detach() as the next chunk's hx).  With no gradient to record it is forward_state (the same
        kernels, the one-launch hourly step included).  h_n is the unrounded fp32 state also with a 16-bit attr_matrix."""
        if not (torch.is_grad_enabled() and (any(p.requires_grad for p in self.hot_path_parameters()) or
                                             (hx is not None and hx.requires_grad))):
            return self.forward_state(adj_matrix, attr_matrix, hx)
        h0 = self._check_state("forward_with_state", attr_matrix, hx)
        out, h_n = gcn_gru_with_state(adj_matrix, attr_matrix, self.hot_path_parameters(), self.math, h0)
        if self.validate and self.math != _lib.MATH_F32:
            check_range_status(out.device)
        return out.squeeze(0), h_n.unsqueeze(0)
