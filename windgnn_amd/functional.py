"""torch.autograd bindings over the C ABI.  PyTorch is plumbing here: device memory, streams and
the autograd graph; all arithmetic of the path runs in libwindgnn_hip.so."""
from __future__ import annotations

import ctypes as C
from typing import Sequence

import torch

from . import _lib

PARAM_ORDER = ("conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias",
               "gru.weight_ih_l0", "gru.weight_hh_l0", "gru.bias_ih_l0", "gru.bias_hh_l0")


_IO_OF = {torch.float32: _lib.IO_F32, torch.float16: _lib.IO_F16, torch.bfloat16: _lib.IO_BF16}


def _require_gpu(*tensors: torch.Tensor, io_ok: bool = False) -> None:
    """io_ok: the tensor is one of the "on the wire" tensors (X, Y, labels), which may also be fp16 / bf16 (wgnn_io)."""
    for t in tensors:
        if not t.is_cuda:
            raise RuntimeError(
                "windgnn_amd runs on an MI355X (HIP) only: got a %s tensor. There is no CPU fallback; "
                "use the oracle under oracle/ for CPU checks." % t.device)
        if t.dtype != torch.float32 and not (io_ok and t.dtype in _IO_OF):
            raise RuntimeError("windgnn_amd: expected float32 tensors, got %s" % t.dtype)


def _require_contiguous(**named: torch.Tensor) -> None:
    """The C ABI reads dense row-major memory from data_ptr(): a strided view (e.g. a batch slice X[::2], a transposed
    label tensor) would be read as if it were dense.  The raw entry points refuse it; callers own the .contiguous().
    A list of tensors (params=..., grads=...) is checked tensor by tensor; the message names the one, as params[3]."""
    for name, t in named.items():
        is_list = isinstance(t, (list, tuple))
        for i, q in enumerate(t if is_list else (t,)):
            if q is not None and not q.is_contiguous():
                raise RuntimeError("windgnn_amd: %s must be contiguous (got shape %s with strides %s): call .contiguous() "
                                   "on it first"
                                   % ("%s[%d]" % (name, i) if is_list else name, tuple(q.shape), tuple(q.stride())))


SCRATCH_ALIGN = 256        # workspace, stash, state stash and `prepared` (include/windgnn.h, "Alignment")


def _require_scratch_aligned(**named: torch.Tensor) -> None:
    """Tensors need the alignment of their element only, which every torch view has.  The stash and the `prepared` images are
    read by LDS-DMA and 16-byte vector loads at offsets laid out in 256-byte steps from their base: a buffer that starts
    anywhere else (a slice of a larger allocation) is refused here, not read.  Fresh torch allocations qualify."""
    for name, t in named.items():
        if t is not None and t.data_ptr() % SCRATCH_ALIGN != 0:
            raise RuntimeError("windgnn_amd: %s must start on a %d-byte boundary (its data_ptr() is %d bytes past one): "
                               "allocate it on its own (torch.empty) instead of slicing a larger buffer"
                               % (name, SCRATCH_ALIGN, t.data_ptr() % SCRATCH_ALIGN))


def _ptr(t):
    return C.c_void_p(t.data_ptr()) if t is not None else C.c_void_p(0)


def _stash_ptr(stash):
    _require_scratch_aligned(stash=stash)
    return _ptr(stash)


def _scratch(device, nbytes: int):
    """(pointer, bytes) of plain scratch for the entry points that have no status block (wgnn_mse_loss_grad,
    wgnn_gcn_layer_*_bwd): the shared workspace past its first 256 bytes."""
    ws = _Workspace.get(device, nbytes + _lib.STATUS_BYTES)
    return C.c_void_p(ws.data_ptr() + _lib.STATUS_BYTES), ws.numel() - _lib.STATUS_BYTES


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _adj(A, S=None):
    """(device tensor to pass, adj_format, nnz) for a dense [S,S] tensor or a graph.CsrAdjacency.  `S` = the station
    count of the features it will multiply: the kernels locate rowptr / col / val inside the CSR buffer from S and
    nnz alone and the C ABI cannot look into device memory, so a buffer built for another graph is refused HERE."""
    if hasattr(A, "blob"):                                    # CsrAdjacency
        if A.blob.dtype != torch.int32 or A.blob.dim() != 1 or not A.blob.is_contiguous():
            raise RuntimeError("windgnn_amd: the CSR adjacency buffer must be a contiguous 1-D int32 tensor, got %s %s"
                               % (A.blob.dtype, tuple(A.blob.shape)))
        if A.blob.numel() != 2 * (A.S + 1) + 4 * A.nnz:
            raise RuntimeError("windgnn_amd: CSR adjacency buffer has %d words, expected 2*(S+1) + 4*nnz = %d "
                               "(S=%d, nnz=%d)" % (A.blob.numel(), 2 * (A.S + 1) + 4 * A.nnz, A.S, A.nnz))
        if S is not None and A.S != S:
            raise RuntimeError("windgnn_amd: CSR adjacency of %d stations does not match %d stations" % (A.S, S))
        if not A.blob.is_cuda:
            raise RuntimeError("windgnn_amd: the CSR adjacency is on %s; call .to(device) first (no CPU fallback)"
                               % A.blob.device)
        return A.blob, _lib.ADJ_CSR, A.nnz
    _require_gpu(A)
    if S is not None and tuple(A.shape) != (S, S):
        raise RuntimeError("windgnn_amd: adjacency %s does not match %d stations" % (tuple(A.shape), S))
    return A.contiguous(), _lib.ADJ_DENSE, 0


def _params_struct(cls, tensors: Sequence[torch.Tensor], prepared: torch.Tensor = None):
    s = cls()
    for (name, _), t in zip(cls._fields_, tensors):
        setattr(s, name, t.data_ptr())
    if prepared is not None:
        _require_scratch_aligned(prepared=prepared)
        s.prepared = prepared.data_ptr()      # wgnn_params.prepared: caller-kept images of W_ih
    return s


class _Workspace:
    """Per-device grow-only scratch, so the steady state does no allocation.  Allocated zeroed: its first 256 bytes
    are the library's sticky status block (include/windgnn.h), which kernels only OR into."""
    _bufs = {}

    @classmethod
    def get(cls, device, nbytes: int) -> torch.Tensor:
        key = (device.index, torch.cuda.current_stream(device).cuda_stream)
        buf = cls._bufs.get(key)
        nbytes = max(nbytes, _lib.STATUS_BYTES)
        if buf is None or buf.numel() < nbytes:
            status = buf[:_lib.STATUS_BYTES].clone() if buf is not None else None
            buf = torch.zeros(nbytes, dtype=torch.uint8, device=device)
            if status is not None:
                buf[:_lib.STATUS_BYTES] = status            # a pending report survives the re-allocation
            cls._bufs[key] = buf
        return buf


_WORKSPACE_BYTES = {_lib.Dims: "wgnn_workspace_bytes", _lib.SeriesDims: "wgnn_series_workspace_bytes"}


def _workspace(d, device, refused=None, query=None):
    """(workspace, bytes to pass) of the dims struct `d` (wgnn_dims or wgnn_series_dims) on `device`: one size query of the
    library per call, then this stream's shared buffer, grown if need be.  The library sizes nothing (0) for dims it refuses:
    with `refused` (the call, for the message) that is raised here with its reason; without, the entry point reports it.
    query: another size query of the same dims (wgnn_series_val_workspace_bytes, which serves both row mappings)."""
    if query is None:
        query = _WORKSPACE_BYTES[type(d)]
        if isinstance(d, _lib.SeriesDims) and d.stride == 0:       # a table of starts: include/windgnn_series_at.h
            query = "wgnn_series_at_workspace_bytes"
    ws_bytes = getattr(_lib.load(), query)(C.byref(d))
    if ws_bytes == 0 and refused is not None:
        _lib.check(-5 if d.F == 13 else -2, refused)
    return _Workspace.get(device, ws_bytes), ws_bytes


def _grads_device(grads, device):
    """The device of the finish_* / bwd_rows family, which take no input tensor: the caller's, else the gradients'."""
    return device if device is not None else grads[0].device


def _gru_struct(cls, tensors):
    """wgnn_params / wgnn_grads of the GRU-only entry points (wgnn_gru_fwd / wgnn_gru_bwd): the four GRU slots from
    (w_ih, w_hh, b_ih, b_hh), the conv slots NULL."""
    s = cls()
    s.w_ih, s.w_hh, s.b_ih, s.b_hh = (q.data_ptr() for q in tensors)
    return s


def _flat_grads(params, device):
    """Gradients for `params` as views, shaped like them, of ONE new fp32 buffer (one allocation per autograd backward)."""
    sizes = [p.numel() for p in params]
    flat = torch.empty(sum(sizes), dtype=torch.float32, device=device)
    return [g.view_as(p) for g, p in zip(flat.split(sizes), params)]


_STATUS_TEXT = {1: "a graph-convolution pre-activation left fp16's range (|x| > 65504) or was NaN",
                2: "a GRU weight or bias lies outside fp16's range",
                4: "a gradient came out inf / NaN",
                8: "wgnn_bwd_mse_part(part | 8) ran on a stash whose last forward was not wgnn_fwd_loss: the loss is NaN "
                   "and the gradients are not to be used",
                16: "a table of window starts (series mode, starts=) holds an entry outside [0, rows - seq_len] or is not "
                    "non-decreasing: the results of that call are not to be used",
                32: "a validation call (wgnn_series_val, missing_labels=True) found no label at all on its windows: its loss is "
                    "NaN"}
_STATUS_FP16_BITS = 1 | 2      # the reports that come from fp16's range: only they get the advice about the math modes


def check_range_status(device=None) -> None:
    """Read the status word of this process's workspaces on `device` (one 4-byte device-to-host copy each, so a
    synchronisation) and raise if a kernel of the fp16-plane math modes (f16x3 / f16) reported a value it cannot
    represent.  The reference's fp32 path has no such limit; the answer is never silently inf/NaN/0."""
    for (index, _), buf in list(_Workspace._bufs.items()):
        if device is not None and torch.device(device).index not in (None, index):
            continue
        word = int(buf[:4].view(torch.int32).item())
        if word:
            buf[:4].zero_()
            what = "; ".join(t for b, t in _STATUS_TEXT.items() if word & b)
            advice = (" The f16x3 / f16 math modes hold activations and weights as fp16 planes: normalise the inputs (the "
                      "reference min-max-normalises every feature to [0, 1]) or use math='f32'."
                      if word & _STATUS_FP16_BITS else "")
            raise RuntimeError("windgnn_amd: %s (status %d: %s).%s" % (_lib.load().wgnn_strerror(-7).decode(), word, what, advice))


def _forward_setup(A, X, params: Sequence[torch.Tensor], math, labels=None, h0=None, h_n=None, B=None):
    """What every forward checks and sizes before it launches anything: X [B,T,S,F] and the params on the GPU and contiguous
    (labels: contiguous too; h0 / h_n: [B, H] fp32 on X's device), the adjacency resolved for S stations (_adj), the Dims
    (X's dtype is the I/O type: Y comes back in it) and the workspace.  B: Dims for another batch size (sizes that do not
    depend on it).  Returns (adjacency to pass, d, workspace, workspace bytes)."""
    _require_gpu(X, io_ok=True)
    _require_gpu(*params)
    _require_contiguous(X=X, labels=labels, params=params)
    if X.dim() != 4:
        raise RuntimeError("windgnn_amd: X must be [B, T, S, 13], got %s" % (tuple(X.shape),))
    BX, T, S, F = X.shape
    B = BX if B is None else B
    A, fmt, nnz = _adj(A, S)
    H = params[5].shape[1]
    for name, t in (("h0", h0), ("h_n", h_n)):
        if t is None:
            continue
        _require_gpu(t)
        _require_contiguous(**{name: t})
        if tuple(t.shape) != (B, H) or t.device != X.device:
            raise RuntimeError("windgnn_amd: %s must be [B, H] = [%d, %d] float32 on %s, got %s on %s"
                               % (name, B, H, X.device, tuple(t.shape), t.device))
    d = _lib.Dims(B, T, S, F, H, math, fmt, nnz, _IO_OF[X.dtype])
    ws, ws_bytes = _workspace(d, X.device, refused="wgnn_workspace_bytes(B=%d,T=%d,S=%d,F=%d,H=%d,math=%d,io=%s)"
                              % (B, T, S, F, H, math, X.dtype))
    return A, d, ws, ws_bytes


def gcn_gru_forward_raw(A, X, params: Sequence[torch.Tensor], math=_lib.MATH_F32, want_stash=True, labels=None,
                        prepared=None, stash=None):
    """Y[B,T,H], stash = wgnn_fwd(...).  X is [B,T,S,F].  labels [B,T,H]: wgnn_fwd_loss (the MSE statistics of
    (Y - labels) are left in the stash for gcn_gru_backward_mse_raw(..., part | 8)).  stash: a caller's buffer of
    wgnn_stash_bytes bytes (uint8, on X's device) instead of a new one."""
    lib = _lib.load()
    A, d, ws, ws_bytes = _forward_setup(A, X, params, math, labels=labels)
    B, T, H = d.B, d.T, d.H
    if stash is not None:
        if not want_stash or stash.dtype != torch.uint8 or stash.device != X.device or stash.numel() < lib.wgnn_stash_bytes(C.byref(d)):
            raise RuntimeError("windgnn_amd: stash must be a uint8 buffer of wgnn_stash_bytes = %d bytes on %s"
                               % (lib.wgnn_stash_bytes(C.byref(d)), X.device))
    elif want_stash:
        stash = torch.empty(lib.wgnn_stash_bytes(C.byref(d)), dtype=torch.uint8, device=X.device)
    Y = torch.empty(B, T, H, dtype=X.dtype, device=X.device)
    ps = _params_struct(_lib.Params, params, prepared)
    if labels is not None:
        _require_gpu(labels, io_ok=True)
        if labels.dtype != X.dtype:
            raise RuntimeError("windgnn_amd: labels are %s but X is %s (one I/O type per call)" % (labels.dtype, X.dtype))
        if labels.numel() != Y.numel() or not want_stash:
            raise RuntimeError("windgnn_amd: wgnn_fwd_loss needs a stash and labels of Y's size, got %s vs %s"
                               % (tuple(labels.shape), tuple(Y.shape)))
        rc = lib.wgnn_fwd_loss(C.byref(d), _ptr(A), _ptr(X), C.byref(ps), _ptr(labels), _ptr(Y),
                               _stash_ptr(stash), _ptr(ws), ws_bytes, _stream())
        _lib.check(rc, "wgnn_fwd_loss")
        return Y, stash, d
    rc = lib.wgnn_fwd(C.byref(d), _ptr(A), _ptr(X), C.byref(ps), _ptr(Y), _stash_ptr(stash), _ptr(ws), ws_bytes, _stream())
    _lib.check(rc, "wgnn_fwd")
    return Y, stash, d


def gcn_gru_forward_last_raw(A, X, params: Sequence[torch.Tensor], math=_lib.MATH_F32, wind_min: float = 0.0,
                             wind_max: float = 1.0, prepared=None):
    """last [B, H] fp32 = wgnn_fwd_last(...): Y[:, T - 1] * (wind_max - wind_min) + wind_min of gcn_gru_forward_raw's stash-less
    forward, where the register-resident recurrences never write the other T - 1 rows.  fp32 X only.  With (0, 1), the
    defaults, the read-out y * 1 + 0 is exact: the rows are Y's own."""
    lib = _lib.load()
    _require_gpu(X)
    A, d, ws, ws_bytes = _forward_setup(A, X, params, math)
    last = torch.empty(d.B, d.H, dtype=torch.float32, device=X.device)
    ps = _params_struct(_lib.Params, params, prepared)
    rc = lib.wgnn_fwd_last(C.byref(d), _ptr(A), _ptr(X), C.byref(ps), float(wind_min), float(wind_max), _ptr(last), _ptr(ws),
                           ws_bytes, _stream())
    _lib.check(rc, "wgnn_fwd_last")
    return last


def gcn_gru_state(A, X, params: Sequence[torch.Tensor], math=_lib.MATH_F32, h0=None, want_y=True, h_n=None):
    """(Y or None, h_n) = wgnn_fwd_state(...): the forward from the initial state h0 [B,H] (None = zeros, exactly wgnn_fwd's
    recurrence), returning the unrounded fp32 last state h_n [B,H] as nn.GRU does.  No autograd (inference only).  X is
    [B,T,S,F]; Y comes back in X's dtype.  h_n: optional caller buffer [B,H] fp32 (it must not share memory with h0).
    T == 1 with a dense A (S <= 64), fp32 X, H <= 128 and B <= _lib.STEP_MAX_B is ONE kernel launch."""
    lib = _lib.load()
    A, d, ws, ws_bytes = _forward_setup(A, X, params, math, h0=h0, h_n=h_n)
    B, T, H = d.B, d.T, d.H
    Y = torch.empty(B, T, H, dtype=X.dtype, device=X.device) if want_y else None
    if h_n is None:
        h_n = torch.empty(B, H, dtype=torch.float32, device=X.device)
    ps = _params_struct(_lib.Params, params)
    rc = lib.wgnn_fwd_state(C.byref(d), _ptr(A), _ptr(X), C.byref(ps), _ptr(h0), _ptr(Y), _ptr(h_n), _ptr(ws), ws_bytes,
                            _stream())
    _lib.check(rc, "wgnn_fwd_state")
    return Y, h_n


def gcn_gru_backward_raw(d, A, X, params, Y, dY, stash, grads: Sequence[torch.Tensor], part: int = 7, stream=None,
                         prepared=None):
    """part bit mask (wgnn_bwd_part): 1 = BPTT recurrence, 4 = GRU weight-gradient GEMMs, 2 = dg + GCN backward.
    prepared: the caller-kept images of W_ih (wgnn_params.prepared), which part 2 then reads instead of staging its own."""
    lib = _lib.load()
    _require_contiguous(X=X, Y=Y, dY=dY, grads=grads, params=params)
    A = getattr(A, "blob", A)              # CsrAdjacency -> its device buffer (d.adj_format says which it is)
    _require_contiguous(adj_matrix=A)
    ws, ws_bytes = _workspace(d, X.device)
    ps = _params_struct(_lib.Params, params, prepared)
    gs = _params_struct(_lib.Grads, grads)
    rc = lib.wgnn_bwd_part(C.byref(d), _ptr(A), _ptr(X), C.byref(ps), _ptr(Y), _ptr(dY), _stash_ptr(stash), C.byref(gs),
                           _ptr(ws), ws_bytes, _stream() if stream is None else C.c_void_p(stream.cuda_stream), part)
    _lib.check(rc, "wgnn_bwd_part(%d)" % part)


def gcn_gru_backward_mse_raw(d, A, X, params, Y, L, stash, grads: Sequence[torch.Tensor], loss: torch.Tensor,
                             grad_scale: float = 1.0, part: int = 7, prepared=None):
    """wgnn_bwd_mse_part: the backward of grad_scale * mean((Y - L)^2) with the loss call folded in (src/main.py:72,79);
    `loss` (0-dim device tensor) receives mean((Y - L)^2) from the call that has part bit 1."""
    lib = _lib.load()
    _require_gpu(L, io_ok=True)
    if L.dtype != Y.dtype:
        raise RuntimeError("windgnn_amd: labels are %s but Y is %s (one I/O type per call)" % (L.dtype, Y.dtype))
    if L.numel() != Y.numel():
        raise RuntimeError("windgnn_amd: MSE operands differ in size: %s vs %s" % (tuple(Y.shape), tuple(L.shape)))
    _require_contiguous(X=X, Y=Y, labels=L, grads=grads, params=params)
    A = getattr(A, "blob", A)
    _require_contiguous(adj_matrix=A)
    ws, ws_bytes = _workspace(d, X.device)
    ps = _params_struct(_lib.Params, params, prepared)
    gs = _params_struct(_lib.Grads, grads)
    rc = lib.wgnn_bwd_mse_part(C.byref(d), _ptr(A), _ptr(X), C.byref(ps), _ptr(Y), _ptr(L), grad_scale,
                               _ptr(loss), _stash_ptr(stash), C.byref(gs), _ptr(ws), ws_bytes, _stream(), part)
    _lib.check(rc, "wgnn_bwd_mse_part(%d)" % part)


def prepared_weights(d, params, device):
    """A fresh `prepared` buffer (wgnn_params.prepared) holding the staged images of params' W_ih / b_ih, or None when
    this configuration has none (wgnn_prepared_bytes == 0)."""
    lib = _lib.load()
    nbytes = lib.wgnn_prepared_bytes(C.byref(d))
    if nbytes == 0:
        return None
    buf = torch.empty(nbytes, dtype=torch.uint8, device=device)
    refresh_prepared(d, params, buf)
    return buf


def refresh_prepared(d, params, prepared) -> None:
    """wgnn_prepare_weights: rebuild the images after the caller changed W_ih / b_ih itself (load_state_dict, ...)."""
    lib = _lib.load()
    ws = _Workspace.get(prepared.device, _lib.STATUS_BYTES)
    ps = _params_struct(_lib.Params, params, prepared)
    _lib.check(lib.wgnn_prepare_weights(C.byref(d), C.byref(ps), _ptr(ws), ws.numel(), _stream()), "wgnn_prepare_weights")


def _adam_struct(adam):
    ad = _lib.Adam()
    ad.exp_avg = _params_struct(_lib.Grads, adam["exp_avg"])
    ad.exp_avg_sq = _params_struct(_lib.Grads, adam["exp_avg_sq"])
    ad.step, ad.lr, ad.beta1, ad.beta2, ad.eps = adam["step"], adam["lr"], adam["beta1"], adam["beta2"], adam["eps"]
    return ad


def finish_step(d, params, grads, which: int, adam=None, prepared=None, device=None) -> None:
    """wgnn_finish: reduce the deferred partial sums of the backward parts in `which` (4: GRU, 2: conv) into `grads` and,
    with adam = dict(exp_avg=[8 tensors], exp_avg_sq=[8 tensors], step, lr, beta1, beta2, eps), apply Adam to `params`
    in place (and refresh `prepared`) -- one launch.  `which` = _lib.FINISH_ADAM_GRU / FINISH_ADAM_CONV (with adam, no
    reduce bit): the optimiser step of that tensor family only."""
    lib = _lib.load()
    ws, ws_bytes = _workspace(d, _grads_device(grads, device))
    ps = _params_struct(_lib.Params, params, prepared)
    gs = _params_struct(_lib.Grads, grads)
    ad = _adam_struct(adam) if adam is not None else None
    rc = lib.wgnn_finish(C.byref(d), C.byref(ps), C.byref(gs), which, C.byref(ad) if ad is not None else None, _ptr(ws),
                         ws_bytes, _stream())
    _lib.check(rc, "wgnn_finish(%d%s)" % (which, ", adam" if adam is not None else ""))


_CLIP_BYTES = {}           # wgnn_clip_bytes per dims (it depends on nothing else): one library call per shape, not per step


def clip_bytes(d) -> int:
    """wgnn_clip_bytes(d): bytes of the `clip` buffer of finish_norm / finish_clipped; 0 = dims the library refuses."""
    key = bytes(d)
    if key not in _CLIP_BYTES:
        _CLIP_BYTES[key] = int(_lib.load().wgnn_clip_bytes(C.byref(d)))
    return _CLIP_BYTES[key]


def clip_buffer(d, device) -> torch.Tensor:
    """A fresh `clip` buffer (fp32, clip_bytes(d) bytes) for finish_norm / finish_clipped: [_lib.CLIP_TOTAL] the gradient's
    L2 norm, [_lib.CLIP_COEF] the clip coefficient, the rest private to the library."""
    nbytes = clip_bytes(d)
    if nbytes == 0:
        _lib.check(-2, "wgnn_clip_bytes")
    return torch.empty(nbytes // 4, dtype=torch.float32, device=device)


def _clip_ptr(d, clip):
    _require_gpu(clip)
    _require_contiguous(clip=clip)
    _require_scratch_aligned(clip=clip)
    need = clip_bytes(d)
    if need == 0 or clip.numel() * 4 < need:
        raise RuntimeError("windgnn_amd: clip holds %d bytes, wgnn_clip_bytes says %d (0 = dims the library refuses)"
                           % (clip.numel() * 4, need))
    return _ptr(clip)


def finish_norm(d, grads, which: int, max_norm: float, clip, device=None) -> None:
    """wgnn_finish_norm: reduce the deferred partial sums named by `which` (0, 2, 4 or 6) into `grads` exactly as
    finish_step(d, .., which) does, and leave the L2 norm of all 8 gradients in clip[_lib.CLIP_TOTAL] and
    min(1, max_norm / (norm + 1e-6)) in clip[_lib.CLIP_COEF] (torch.nn.utils.clip_grad_norm_'s coefficient) -- on the device,
    deterministic, no host synchronisation.  max_norm > 0; float("inf") only measures.  clip: clip_buffer(d, device)."""
    lib = _lib.load()
    cp = _clip_ptr(d, clip)
    ws, ws_bytes = _workspace(d, _grads_device(grads, device))
    gs = _params_struct(_lib.Grads, grads)
    rc = lib.wgnn_finish_norm(C.byref(d), C.byref(gs), which, float(max_norm), cp, _ptr(ws), ws_bytes, _stream())
    _lib.check(rc, "wgnn_finish_norm(%d, max_norm=%r)" % (which, max_norm))


def finish_clipped(d, params, grads, adam, clip, prepared=None, device=None) -> None:
    """wgnn_finish_clipped: finish_step(d, params, grads, 0, adam, prepared) with every gradient element entering Adam times
    clip[_lib.CLIP_COEF], as the preceding finish_norm left it -- one launch.  `grads` is NOT rewritten (torch's
    clip_grad_norm_ scales .grad in place; here it keeps the unclipped gradient, and clip holds the norm and the factor)."""
    lib = _lib.load()
    cp = _clip_ptr(d, clip)
    ws, ws_bytes = _workspace(d, _grads_device(grads, device))
    ps = _params_struct(_lib.Params, params, prepared)
    gs = _params_struct(_lib.Grads, grads)
    ad = _adam_struct(adam)
    rc = lib.wgnn_finish_clipped(C.byref(d), C.byref(ps), C.byref(gs), C.byref(ad), cp, _ptr(ws), ws_bytes, _stream())
    _lib.check(rc, "wgnn_finish_clipped")


def best_bytes() -> int:
    """wgnn_best_bytes(): bytes of the record of best_init / keep_best (include/windgnn_best.h)."""
    return int(_lib.load().wgnn_best_bytes())


def best_word(record: torch.Tensor, name: str) -> torch.Tensor:
    """A 0-dim VIEW of one public word of a best record (uint8 [best_bytes()]): _lib.BEST_WORDS names them."""
    off, dtype = _lib.BEST_WORDS[name]
    dtype = getattr(torch, dtype)
    return record[off:off + torch.empty((), dtype=dtype).element_size()].view(dtype)[0]


def _record_ptr(record):
    if not record.is_cuda:
        raise RuntimeError("windgnn_amd runs on an MI355X (HIP) only: the best record is on %s. There is no CPU fallback."
                           % record.device)
    _require_contiguous(best=record)
    _require_scratch_aligned(best=record)
    if record.dtype != torch.uint8 or record.numel() < best_bytes():
        raise RuntimeError("windgnn_amd: the best record must be a uint8 tensor of wgnn_best_bytes() = %d bytes, got %s %s"
                           % (best_bytes(), record.dtype, tuple(record.shape)))
    return _ptr(record)


def best_init(record: torch.Tensor, threshold: float) -> None:
    """wgnn_best_init: every byte of `record` (uint8 [best_bytes()], it may be dirty) written: best_loss = threshold
    (float("inf"): the first finite loss wins), best_step = -1, counters 0."""
    _lib.check(_lib.load().wgnn_best_init(_record_ptr(record), float(threshold), _stream()), "wgnn_best_init(%r)" % threshold)


def keep_best_args(d, loss: torch.Tensor, params, best_params, record: torch.Tensor):
    """Everything of a keep_best call but the step number, validated and marshalled once (a caller whose tensors never move --
    TrainStep -- pays the checks and the two wgnn_params structs at construction, not per step): pass it to keep_best_launch."""
    _require_gpu(loss, *params, *best_params)
    _require_contiguous(params=params, best_params=best_params)
    for i, (q, b) in enumerate(zip(params, best_params)):
        if q.numel() != b.numel():
            raise RuntimeError("windgnn_amd: best_params[%d] has %d elements, params[%d] has %d" % (i, b.numel(), i, q.numel()))
    ps = _params_struct(_lib.Params, params)
    bs = _params_struct(_lib.Params, best_params)
    return (_lib.load().wgnn_keep_best, C.byref(d), _ptr(loss), C.byref(ps), C.byref(bs), _record_ptr(record),
            (d, ps, bs, loss, list(params), list(best_params), record))       # the last entry keeps the memory alive


def keep_best_launch(args, step: int) -> None:
    fn, d, loss, ps, bs, rec, _ = args
    _lib.check(fn(d, loss, ps, bs, int(step), rec, _stream()), "wgnn_keep_best(step=%d)" % step)


def keep_best(d, loss: torch.Tensor, params, best_params, step: int, record: torch.Tensor) -> None:
    """wgnn_keep_best: the reference's rule (src/main.py:83-86) on the device -- if float64(loss) < record.best_loss, the 8
    tensors `params` are copied into `best_params` and best_loss / best_step = loss / `step`; no host synchronisation."""
    keep_best_launch(keep_best_args(d, loss, params, best_params, record), step)


def val_bytes() -> int:
    """wgnn_val_bytes(): bytes of the record of a validation pass (include/windgnn_series_val.h)."""
    return int(_lib.load().wgnn_val_bytes())


def val_word(record: torch.Tensor, name: str) -> torch.Tensor:
    """A 0-dim VIEW of one public word of a validation record (uint8 [val_bytes()]): _lib.VAL_WORDS names them."""
    off, dtype = _lib.VAL_WORDS[name]
    dtype = getattr(torch, dtype)
    return record[off:off + torch.empty((), dtype=dtype).element_size()].view(dtype)[0]


def _val_ptr(record):
    if not record.is_cuda:
        raise RuntimeError("windgnn_amd runs on an MI355X (HIP) only: the validation record is on %s. There is no CPU fallback."
                           % record.device)
    _require_contiguous(val=record)
    _require_scratch_aligned(val=record)
    if record.dtype != torch.uint8 or record.numel() < val_bytes():
        raise RuntimeError("windgnn_amd: the validation record must be a uint8 tensor of wgnn_val_bytes() = %d bytes, got %s %s"
                           % (val_bytes(), record.dtype, tuple(record.shape)))
    return _ptr(record)


def val_init(record: torch.Tensor) -> None:
    """wgnn_val_init: every byte of `record` (it may be dirty) written; sums, counts, passes and stale 0, mean and loss NaN."""
    _lib.check(_lib.load().wgnn_val_init(_val_ptr(record), _stream()), "wgnn_val_init")


def val_buffer(device) -> torch.Tensor:
    """A fresh, initialised validation record on `device` (uint8 [val_bytes()]); val_word reads its public words."""
    record = torch.empty(val_bytes(), dtype=torch.uint8, device=device)
    val_init(record)
    return record


def val_begin(record: torch.Tensor) -> None:
    """wgnn_val_begin: opens a pass (sum, count, mean, max_abs, loss and calls reset; passes and stale kept)."""
    _lib.check(_lib.load().wgnn_val_begin(_val_ptr(record), _stream()), "wgnn_val_begin")


def val_close(record: torch.Tensor, best: torch.Tensor = None) -> None:
    """wgnn_val_close: passes += 1 and, with the best record that wgnn_keep_best has just decided on from this record's loss
    word, stale = 0 if it won, else stale + 1."""
    _lib.check(_lib.load().wgnn_val_close(_val_ptr(record), _record_ptr(best) if best is not None else C.c_void_p(0), _stream()),
               "wgnn_val_close")


VALIDATION_KINDS = ("mse", "l1", "huber")
VALIDATION_CHUNK_BYTES = 64 << 20       # the cap on ONE fp64 temporary of validation_terms (it keeps two alive at most)


def validation_spec(loss, huber_delta, loss_from, T, who="windgnn_amd: validation_terms"):
    """loss= / huber_delta= / loss_from= of a validation or a training step on materialised windows of T steps (the caller's
    name goes into `who`), refused by the argument's name:
    (kind, delta, first counted step)."""
    import math as _math
    if loss not in VALIDATION_KINDS:
        raise ValueError("%s: loss=%r: the losses formed here are 'mse', 'l1' or 'huber'; any other loss works on "
                         "GCN_GRU.forward's output with torch" % (who, loss))
    t_from = int(loss_from)
    if t_from != loss_from or not 0 <= t_from < int(T):
        raise ValueError("%s: loss_from=%r must be a step of the window, an integer in [0, T = %d): 0 counts every step, "
                         "T - 1 the last alone" % (who, loss_from, int(T)))
    delta = float(huber_delta)
    if loss == "huber" and not (_math.isfinite(delta) and delta > 0.0):
        raise ValueError("%s: huber_delta=%r must be finite and > 0 (nn.HuberLoss's delta); loss='l1' is the limit of a small "
                         "one and loss='mse' twice that of a large one" % (who, huber_delta))
    return loss, delta, t_from


def validation_chunk_windows(B: int, T: int, H: int, cap_bytes: int = VALIDATION_CHUNK_BYTES) -> int:
    """Windows per chunk of validation_terms' reduction: as many whole windows of T counted steps as keep one fp64 temporary
    (T * H * 8 bytes per window) under the cap, one at least -- a function of the shape alone."""
    return max(1, min(int(B), int(cap_bytes) // (int(T) * int(H) * 8)))


def validation_terms(Y: torch.Tensor, L: torch.Tensor, loss: str = "mse", huber_delta: float = 1.0, loss_from: int = 0,
                     missing_labels: bool = False):
    """What a validation call adds to the record, from Y and L [B, T, H] (fp32, fp16 or bf16; CPU tensors work as well), in
    plain torch and fp64 throughout: with r = Y.double() - L.double() and the counted set
    M = {(b, t, c): t >= loss_from and (not missing_labels or L[b, t, c] is not NaN)},

        s = sum over M of rho(r)     rho = r^2 ("mse"), |r| ("l1"), nn.HuberLoss(delta=huber_delta) ("huber")
        m = |M|                      a 0-dim int64 tensor on Y's device (no host read)
        a = max over M of |r|        0 for an empty M

    returned as (s, m, a), 0-dim.  The steps before loss_from are sliced away and a missing label's residual is replaced by 0
    with torch.where before anything is formed from it (rho(0) = 0 = |0| exactly): nothing outside M reaches s or a, NaN or
    not.  With missing_labels=False a NaN label is counted and poisons s and a.
    Two levels, both fixed by the shape alone: chunks of validation_chunk_windows whole windows, each summed by
    torch.sum in fp64, and the chunks' sums added in ascending order; equal shapes therefore sum in the same order."""
    kind, delta, t0 = validation_spec(loss, huber_delta, loss_from, Y.shape[1] if Y.dim() == 3 else 1)
    if Y.dim() != 3 or tuple(Y.shape) != tuple(L.shape):
        raise ValueError("windgnn_amd: validation_terms wants Y and L of one shape [B, T, H], got %s and %s"
                         % (tuple(Y.shape), tuple(L.shape)))
    B, T, H = Y.shape
    s = a = None
    m = None if missing_labels else B * (T - t0) * H
    step = validation_chunk_windows(B, T - t0, H, VALIDATION_CHUNK_BYTES)
    for b0 in range(0, B, step):
        Lc = L[b0:b0 + step, t0:]
        r = Y[b0:b0 + step, t0:].to(torch.float64)
        r -= Lc                                            # (type promotion: L enters as its exact fp64 value)
        if missing_labels:
            on = ~torch.isnan(Lc)
            r = torch.where(on, r, torch.zeros((), dtype=torch.float64, device=r.device))
            mk = on.sum()
            m = mk if m is None else m + mk
        ak = torch.linalg.vector_norm(r, ord=float("inf"))      # max |r| (NaN if any)
        if kind == "mse":
            rho = r.square_()
        elif kind == "l1":
            rho = r.abs_()
        else:
            rho = torch.nn.functional.huber_loss(r, torch.zeros((), dtype=torch.float64, device=r.device).expand_as(r),
                                                 reduction="none", delta=delta)
        sk = rho.sum()
        s, a = (sk, ak) if s is None else (s + sk, torch.maximum(a, ak))
    if not torch.is_tensor(m):
        m = torch.full((), m, dtype=torch.int64, device=Y.device)
    return s, m, a


def val_add(record: torch.Tensor, s: torch.Tensor, m, a: torch.Tensor) -> None:
    """What one validation call does to the public words of a validation record (include/windgnn_series_val.h), in torch
    operations on val_word's views, in stream order and without a host read (a CPU buffer works as well):
    sum += s; count += m; max_abs = max(max_abs, float32(a)); mean = sum / count (NaN while count = 0); loss = float32(mean);
    calls += 1.  No other byte of the record is written."""
    w = {name: val_word(record, name) for name in ("sum", "count", "mean", "max_abs", "loss", "calls")}
    w["sum"] += s
    w["count"] += m
    torch.maximum(w["max_abs"], a.to(torch.float32), out=w["max_abs"])
    torch.div(w["sum"], w["count"], out=w["mean"])          # (0.0 / 0 = NaN; a NaN sum stays NaN)
    w["loss"].copy_(w["mean"])
    w["calls"] += 1


_SPEC_DTYPES = (torch.float32, torch.float16, torch.bfloat16)


def loss_spec_grad(Y: torch.Tensor, L: torch.Tensor, loss: str = "mse", huber_delta: float = 1.0, loss_from: int = 0,
                   missing_labels: bool = False, grad_scale: float = 1.0, loss_out: torch.Tensor = None,
                   who: str = "windgnn_amd: loss_spec_grad"):
    """(loss, dY, count) of a loss spec on materialised windows: Y and L [B, T, H] (fp32, fp16 or bf16; L fp32 or Y's dtype; CPU
    tensors work as well), in plain torch on the current stream, without a host read.  With r = Y - L over the counted set
    M = {(b, t, c): t >= loss_from and (not missing_labels or L[b, t, c] is not NaN)} and m = |M| (the definitions of
    include/windgnn_series_lossfn.h):

        loss  = sum over M of rho(r) / m                 rho = r^2 ("mse"), |r| ("l1"), nn.HuberLoss(delta=huber_delta) ("huber")
        dY    = grad_scale * rho'(r) / m on M, exactly 0 elsewhere        fp32 [B, T, H], contiguous
        count = m                                        a 0-dim int64 tensor on Y's device

    The counted steps are strided views (a 16-bit one is upcast to fp32 once); a missing label is replaced by Y's own value
    with torch.where, so its residual is exactly 0 and rho(0) = rho'(0) = 0 for all three kinds: nothing is multiplied by a
    mask.  The sum is torch's own loss with reduction="sum" (F.mse_loss / F.huber_loss: on the device two kernels, the elementwise
    rho and its sum, not one fused reduction; "l1": the 1-norm of r, which is formed once, the abs inside the reduction) and dY on the counted steps ONE fused elementwise kernel (aten mse_loss_backward / huber_loss_backward with
    the coefficient grad_scale / m as a 0-dim device tensor; "l1": sign(r) times it), written into dY's view; only
    dY[:, :loss_from] is zero-filled.  m = 0 (possible
    with missing_labels alone): the loss is NaN (0 / 0), dY all zero, count 0 -- the coefficient is selected with torch.where,
    not a branch.  Without missing_labels a NaN label is counted and poisons the loss, as it does mse_loss_grad's.
    loss_out: an optional 0-dim fp32 tensor (a view is fine) that receives the loss instead of a new one.
    The keywords are refused by the argument's name (validation_spec, under `who`).
    Limit: a non-finite Y at a missing label gives a NaN residual (NaN - NaN); the GRU's output is finite unless the
    parameters are not."""
    kind, delta, t0 = validation_spec(loss, huber_delta, loss_from, Y.shape[1] if Y.dim() == 3 else 1, who)
    if Y.dim() != 3 or tuple(Y.shape) != tuple(L.shape):
        raise ValueError("%s wants Y and L of one shape [B, T, H], got %s and %s" % (who, tuple(Y.shape), tuple(L.shape)))
    if Y.dtype not in _SPEC_DTYPES or L.dtype not in (torch.float32, Y.dtype):
        raise ValueError("%s: Y must be float32, float16 or bfloat16 and L float32 or Y's dtype, got %s and %s"
                         % (who, Y.dtype, L.dtype))
    if L.device != Y.device:
        raise ValueError("%s: Y is on %s but L on %s" % (who, Y.device, L.device))
    if loss_out is not None and (loss_out.dim() != 0 or loss_out.dtype != torch.float32 or loss_out.device != Y.device):
        raise ValueError("%s: loss_out must be a 0-dim float32 tensor on %s, got %s %s on %s"
                         % (who, Y.device, tuple(loss_out.shape), loss_out.dtype, loss_out.device))
    B, T, H = Y.shape
    Ys, Ls = Y[:, t0:].to(torch.float32), L[:, t0:].to(torch.float32)       # (fp32: the views themselves, no copy)
    if missing_labels:
        miss = torch.isnan(Ls)
        Ls = torch.where(miss, Ys, Ls)
        count = (~miss).sum()
        coef = torch.where(count > 0, torch.full((), float(grad_scale), dtype=torch.float64, device=Y.device) / count,
                           0.0).to(torch.float32)
    else:
        n = B * (T - t0) * H
        count = torch.full((), n, dtype=torch.int64, device=Y.device)
        coef = torch.full((), float(grad_scale) / n, dtype=torch.float32, device=Y.device)
    dY = torch.empty(B, T, H, dtype=torch.float32, device=Y.device)
    if t0:
        dY[:, :t0].zero_()
    dv = dY[:, t0:]
    if kind == "mse":
        s = torch.nn.functional.mse_loss(Ys, Ls, reduction="sum")
        torch.ops.aten.mse_loss_backward.grad_input(coef, Ys, Ls, 2, grad_input=dv)             # 2 = Reduction::Sum
    elif kind == "l1":
        r = Ys - Ls                                            # formed once, for the sum and for the sign
        s = torch.linalg.vector_norm(r, ord=1)                 # sum |r|: the abs is taken inside the reduction
        torch.mul(torch.sign(r), coef, out=dv)
    else:
        s = torch.nn.functional.huber_loss(Ys, Ls, reduction="sum", delta=delta)
        torch.ops.aten.huber_loss_backward.out(coef, Ys, Ls, 2, delta, grad_input=dv)
    if loss_out is None:
        loss_out = torch.empty((), dtype=torch.float32, device=Y.device)
    torch.div(s, count, out=loss_out)                          # (0.0 / 0 = NaN; a NaN sum stays NaN)
    return loss_out, dY, count


def rows_align(d) -> int:
    """wgnn_bwd_rows_align: the row alignment of a range of wgnn_bwd_rows / wgnn_finish_rows; 0 = not offered for this shape."""
    return int(_lib.load().wgnn_bwd_rows_align(C.byref(d)))


def bwd_rows(d, Y, stash, grads, which: int, row0: int, rows: int, device=None) -> None:
    """wgnn_bwd_rows: part 4 of the backward (weight-gradient GEMMs + their reduction) for gate rows [row0, row0 + rows) of
    the pair `which` (_lib.ROWS_IH: w_ih / b_ih, _lib.ROWS_HH: w_hh / b_hh), after part 1 on the same workspace."""
    lib = _lib.load()
    ws, ws_bytes = _workspace(d, _grads_device(grads, device))
    gs = _params_struct(_lib.Grads, grads)
    rc = lib.wgnn_bwd_rows(C.byref(d), _ptr(Y), _stash_ptr(stash), C.byref(gs), which, row0, rows, _ptr(ws), ws_bytes, _stream())
    _lib.check(rc, "wgnn_bwd_rows(%d, %d, %d)" % (which, row0, rows))


def finish_rows(d, params, grads, which: int, row0: int, rows: int, adam, prepared=None, device=None) -> None:
    """wgnn_finish_rows: Adam (adam: as finish_step) on rows [row0, row0 + rows) of the pair `which`, and the parts of
    `prepared` those rows own."""
    lib = _lib.load()
    ws = _Workspace.get(_grads_device(grads, device), _lib.STATUS_BYTES)
    ps = _params_struct(_lib.Params, params, prepared)
    gs = _params_struct(_lib.Grads, grads)
    ad = _adam_struct(adam)
    rc = lib.wgnn_finish_rows(C.byref(d), C.byref(ps), C.byref(gs), which, row0, rows, C.byref(ad), _ptr(ws), ws.numel(),
                              _stream())
    _lib.check(rc, "wgnn_finish_rows(%d, %d, %d)" % (which, row0, rows))


class GCNGRUFunction(torch.autograd.Function):
    """Y = GCN_GRU(A, X; 8 params).  Gradients flow to the parameters only: the reference's
    adjacency and inputs do not require grad (src/main.py:26, src/step4_sequence_preparer.py:58)."""

    @staticmethod
    def forward(ctx, A, X, math, *params):
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[0]:
            # the reference's autograd would propagate into attr_matrix / adj_matrix; this path has no dX / dA
            # (neither requires grad in the reference loop) and must not drop a requested gradient silently
            raise RuntimeError("windgnn_amd: GCN_GRU gives gradients for its 8 parameters only; attr_matrix / "
                               "adj_matrix with requires_grad=True are not supported (detach them, or stack "
                               "GraphConvLayer modules, which do return dX)")
        X = X.contiguous()
        params = tuple(p.contiguous() for p in params)
        need = any(ctx.needs_input_grad[3:])
        Y, stash, d = gcn_gru_forward_raw(A, X, params, math, want_stash=need)
        ctx.d = d
        ctx.save_for_backward(_adj(A)[0], X, Y, stash, *params)   # dense [S,S] or the CSR blob; d.adj_format says which
        return Y

    @staticmethod
    def backward(ctx, dY):
        A, X, Y, stash, *params = ctx.saved_tensors
        if stash is None:
            raise RuntimeError("windgnn_amd: backward called but the forward ran without a stash")
        grads = _flat_grads(params, X.device)
        gcn_gru_backward_raw(ctx.d, A, X, params, Y, dY.float().contiguous(), stash, grads)   # dY is always fp32
        return (None, None, None, *grads)


def gcn_gru(A, X, params, math=_lib.MATH_F32):
    return GCNGRUFunction.apply(A, X, math, *params)


def gcn_gru_state_forward_raw(A, X, params: Sequence[torch.Tensor], math=_lib.MATH_F32, h0=None, h_n=None, prepared=None):
    """Y, h_n, stash, d = wgnn_fwd_state_stash(...): the training forward from h0 [B,H] fp32 (None = zeros), with the state
    stash the backward (gcn_gru_state_backward_raw) needs; h_n [B,H] fp32 is the unrounded last state (a new tensor unless
    a caller buffer is given; it must not share memory with h0)."""
    lib = _lib.load()
    A, d, ws, ws_bytes = _forward_setup(A, X, params, math, h0=h0, h_n=h_n)
    B, T, H = d.B, d.T, d.H
    stash = torch.empty(lib.wgnn_state_stash_bytes(C.byref(d)), dtype=torch.uint8, device=X.device)
    Y = torch.empty(B, T, H, dtype=X.dtype, device=X.device)
    if h_n is None:
        h_n = torch.empty(B, H, dtype=torch.float32, device=X.device)
    ps = _params_struct(_lib.Params, params, prepared)
    rc = lib.wgnn_fwd_state_stash(C.byref(d), _ptr(A), _ptr(X), C.byref(ps), _ptr(h0), _ptr(Y), _ptr(h_n), _stash_ptr(stash),
                                  _ptr(ws), ws_bytes, _stream())
    _lib.check(rc, "wgnn_fwd_state_stash")
    return Y, h_n, stash, d


def gcn_gru_state_backward_raw(d, A, X, params, Y, dY, dh_n, stash, grads: Sequence[torch.Tensor], dh0=None,
                               part: int = 7, stream=None, prepared=None):
    """wgnn_bwd_state_part: the gradients of sum(Y dY) + sum(h_n dh_n) (dh_n None = zeros) into `grads`, and dh0 [B,H]
    (None = not computed) w.r.t. the h0 recorded in the state stash.  Parts as gcn_gru_backward_raw."""
    lib = _lib.load()
    _require_contiguous(X=X, Y=Y, dY=dY, dh_n=dh_n, dh0=dh0, grads=grads, params=params)
    for name, t in (("dh_n", dh_n), ("dh0", dh0)):
        if t is not None and (tuple(t.shape) != (d.B, d.H) or t.dtype != torch.float32 or t.device != X.device):
            raise RuntimeError("windgnn_amd: %s must be [B, H] = [%d, %d] float32 on %s, got %s %s on %s"
                               % (name, d.B, d.H, X.device, tuple(t.shape), t.dtype, t.device))
    A = getattr(A, "blob", A)
    _require_contiguous(adj_matrix=A)
    ws, ws_bytes = _workspace(d, X.device)
    ps = _params_struct(_lib.Params, params, prepared)
    gs = _params_struct(_lib.Grads, grads)
    rc = lib.wgnn_bwd_state_part(C.byref(d), _ptr(A), _ptr(X), C.byref(ps), _ptr(Y), _ptr(dY), _ptr(dh_n), _stash_ptr(stash),
                                 C.byref(gs), _ptr(dh0), _ptr(ws), ws_bytes,
                                 _stream() if stream is None else C.c_void_p(stream.cuda_stream), part)
    _lib.check(rc, "wgnn_bwd_state_part(%d)" % part)


class GCNGRUStateFunction(torch.autograd.Function):
    """(Y, h_n) = GCN_GRU(A, X, h0; 8 params), nn.GRU's forward(input, hx) -> (output, h_n).  Differentiable in the 8
    parameters and in h0; a loss may depend on Y, on h_n or on both (truncated BPTT over chunks of a long series).
    h0 None: zeros.  Like GCNGRUFunction, no gradient for X or A."""

    @staticmethod
    def forward(ctx, A, X, math, h0, *params):
        if ctx.needs_input_grad[1] or ctx.needs_input_grad[0]:
            raise RuntimeError("windgnn_amd: GCN_GRU gives gradients for its 8 parameters and the initial state only; "
                               "attr_matrix / adj_matrix with requires_grad=True are not supported (detach them)")
        ctx.set_materialize_grads(False)
        X = X.contiguous()
        params = tuple(p.contiguous() for p in params)
        h0c = h0.detach().contiguous() if h0 is not None else None
        Y, h_n, stash, d = gcn_gru_state_forward_raw(A, X, params, math, h0c)
        ctx.d = d
        ctx.has_h0 = h0 is not None
        ctx.save_for_backward(_adj(A)[0], X, Y, stash, *params)
        return Y, h_n

    @staticmethod
    def backward(ctx, dY, dh_n):
        A, X, Y, stash, *params = ctx.saved_tensors
        if dY is None:                     # a loss on h_n alone
            dY = torch.zeros(Y.shape, dtype=torch.float32, device=Y.device)
        grads = _flat_grads(params, X.device)
        want_dh0 = ctx.has_h0 and ctx.needs_input_grad[3]
        dh0 = torch.empty(ctx.d.B, ctx.d.H, dtype=torch.float32, device=X.device) if want_dh0 else None
        gcn_gru_state_backward_raw(ctx.d, A, X, params, Y, dY.float().contiguous(),
                                   dh_n.float().contiguous() if dh_n is not None else None, stash, grads, dh0)
        return (None, None, None, dh0, *grads)


def gcn_gru_with_state(A, X, params, math=_lib.MATH_F32, h0=None):
    """(Y [B,T,H], h_n [B,H]) from the initial state h0 [B,H] fp32 (None = zeros), differentiable in the 8 parameters and h0."""
    return GCNGRUStateFunction.apply(A, X, math, h0, *params)


class GraphConvFunction(torch.autograd.Function):
    """out = relu(A X W + b) for X [..., S, F_in], W [F_in, F_out] (src/step5_gcn_layer_model.py:13-23).  Dense adjacency (S <= 64):
    any widths, exact fp32 -- 13 -> 13, the reference model's own, on the MFMA kernels of gcn.hip, other widths up to 64 on
    gcn_any.hip, wider ones on the tiled fp32-MFMA kernels of gcn_wide.hip; CSR adjacency: 13 -> 13 only."""

    @staticmethod
    def forward(ctx, A, X, W, b):
        lib = _lib.load()
        _require_gpu(X, W, b)
        X, W, b = X.contiguous(), W.contiguous(), b.contiguous()
        S, F = X.shape[-2], X.shape[-1]
        if W.dim() != 2 or W.shape[0] != F or b.shape != (W.shape[1],):
            # the reference's torch.matmul(adj_attr, self.weight) would fail the same way (step5:18)
            raise RuntimeError("GraphConvLayer: attr_matrix has %d features but the weight is %s and the bias %s"
                               % (F, tuple(W.shape), tuple(b.shape)))
        Fo = W.shape[1]
        A, fmt, nnz = _adj(A, S)
        nt = X.numel() // (S * F)
        out = torch.empty(*X.shape[:-1], Fo, dtype=X.dtype, device=X.device)
        if fmt == _lib.ADJ_CSR:
            if (F, Fo) != (13, 13):
                raise RuntimeError("windgnn_amd: a GraphConvLayer over a CSR adjacency is built for the reference's 13 -> 13 "
                                   "layers only (got %d -> %d); other widths need a dense adjacency (S <= 64)" % (F, Fo))
            rc = lib.wgnn_gcn_layer_csr_fwd(nt, S, F, nnz, _ptr(A), _ptr(X), _ptr(W), _ptr(b), _ptr(out), _stream())
        else:
            rc = lib.wgnn_gcn_layer_fwd(nt, S, F, Fo, _ptr(A), _ptr(X), _ptr(W), _ptr(b), _ptr(out), _stream())
        _lib.check(rc, "wgnn_gcn_layer_fwd(S=%d, %d -> %d%s)"
                   % (S, F, Fo, ": a dense adjacency holds at most 64 stations, every width" if fmt != _lib.ADJ_CSR and S > 64 else ""))
        ctx.save_for_backward(A, X, W, out)
        ctx.dims = (nt, S, F, Fo, fmt, nnz)
        return out

    @staticmethod
    def backward(ctx, dout):
        lib = _lib.load()
        A, X, W, out = ctx.saved_tensors
        nt, S, F, Fo, fmt, nnz = ctx.dims
        dout = dout.contiguous()
        dW = torch.empty_like(W)
        db = torch.empty(Fo, dtype=torch.float32, device=X.device)
        dX = torch.empty_like(X) if ctx.needs_input_grad[1] else None
        if fmt == _lib.ADJ_CSR:
            nbytes = lib.wgnn_gcn_layer_csr_workspace_bytes(nt, S, F)
            wsp, _ = _scratch(X.device, nbytes)
            rc = lib.wgnn_gcn_layer_csr_bwd(nt, S, F, nnz, _ptr(A), _ptr(X), _ptr(W), _ptr(out), _ptr(dout), _ptr(dW),
                                            _ptr(db), _ptr(dX), wsp, nbytes, _stream())
            _lib.check(rc, "wgnn_gcn_layer_csr_bwd")
            return None, dX, dW, db
        nbytes = lib.wgnn_gcn_layer_workspace_bytes(nt, S, F, Fo)
        wsp, _ = _scratch(X.device, nbytes)
        rc = lib.wgnn_gcn_layer_bwd(nt, S, F, Fo, _ptr(A), _ptr(X), _ptr(W), _ptr(out), _ptr(dout), _ptr(dW), _ptr(db),
                                    _ptr(dX), wsp, nbytes, _stream())
        _lib.check(rc, "wgnn_gcn_layer_bwd")
        return None, dX, dW, db


class GRUFunction(torch.autograd.Function):
    """Y [B,T,H] = nn.GRU(I, H, batch_first=True)(g [B,T,I]) with h0 = 0 (src/step6_gcn_gru_combined_model.py:23), through
    wgnn_gru_fwd / wgnn_gru_bwd: gradients for g and the four GRU tensors.  What GCN_GRU runs behind two GraphConvLayers when its
    input_dim / hidden_dim are not the reference model's 13 (exact fp32; I must be S * 13: step6:16)."""

    @staticmethod
    def forward(ctx, g, S, w_ih, w_hh, b_ih, b_hh):
        lib = _lib.load()
        _require_gpu(g, w_ih, w_hh, b_ih, b_hh)
        g = g.contiguous()
        params = [p.contiguous() for p in (w_ih, w_hh, b_ih, b_hh)]
        B, T, I = g.shape
        H = w_hh.shape[1]
        d = _lib.Dims(B, T, S, 13, H, _lib.MATH_F32, _lib.ADJ_DENSE, 0, _lib.IO_F32)
        call = "wgnn_gru_fwd(B=%d,T=%d,S=%d,I=%d,H=%d)" % (B, T, S, I, H)
        if I != S * 13:
            _lib.check(-2, call)
        ws, ws_bytes = _workspace(d, g.device, refused=call)
        need = any(ctx.needs_input_grad)
        stash = torch.empty(lib.wgnn_stash_bytes(C.byref(d)), dtype=torch.uint8, device=g.device) if need else None
        Y = torch.empty(B, T, H, dtype=torch.float32, device=g.device)
        ps = _gru_struct(_lib.Params, params)
        _lib.check(lib.wgnn_gru_fwd(C.byref(d), _ptr(g), C.byref(ps), _ptr(Y), _stash_ptr(stash), _ptr(ws), ws_bytes, _stream()),
                   "wgnn_gru_fwd")
        ctx.d = d
        ctx.save_for_backward(g, Y, stash, *params)
        return Y

    @staticmethod
    def backward(ctx, dY):
        lib = _lib.load()
        g, Y, stash, *params = ctx.saved_tensors
        grads = [torch.empty_like(q) for q in params]
        dg = torch.empty_like(g)
        ws, ws_bytes = _workspace(ctx.d, g.device)
        ps, gs = _gru_struct(_lib.Params, params), _gru_struct(_lib.Grads, grads)
        _lib.check(lib.wgnn_gru_bwd(C.byref(ctx.d), _ptr(g), C.byref(ps), _ptr(Y), _ptr(dY.float().contiguous()),
                                    _stash_ptr(stash), C.byref(gs), _ptr(dg), _ptr(ws), ws_bytes, _stream()), "wgnn_gru_bwd")
        return (dg, None, *grads)


def mse_loss_grad(Y, L, grad_scale: float = 1.0, want_grad=True, loss=None):
    """loss (0-dim tensor on device) and dY for nn.MSELoss()(Y, L) (src/main.py:49,72).  loss: optional 0-dim fp32 device
    tensor (a view is fine) that receives it instead of a new one."""
    lib = _lib.load()
    _require_gpu(Y, L)
    Y, L = Y.contiguous(), L.contiguous()
    if Y.numel() != L.numel():
        raise RuntimeError("windgnn_amd: MSE operands differ in size: %s vs %s" % (tuple(Y.shape), tuple(L.shape)))
    dY = torch.empty_like(Y) if want_grad else None
    if loss is None:
        loss = torch.empty((), dtype=torch.float32, device=Y.device)
    wsp, wsn = _scratch(Y.device, 4096)
    rc = lib.wgnn_mse_loss_grad(_ptr(Y), _ptr(L), Y.numel(), grad_scale, _ptr(dY), _ptr(loss), wsp, wsn, _stream())
    _lib.check(rc, "wgnn_mse_loss_grad")
    return loss, dY


def adam_step_(param, grad, exp_avg, exp_avg_sq, step, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8):
    lib = _lib.load()
    _require_gpu(param, grad, exp_avg, exp_avg_sq)
    rc = lib.wgnn_adam_step(_ptr(param), _ptr(grad), _ptr(exp_avg), _ptr(exp_avg_sq), param.numel(), step, lr, beta1,
                            beta2, eps, _stream())
    _lib.check(rc, "wgnn_adam_step")
