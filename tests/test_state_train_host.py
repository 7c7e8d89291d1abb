"""Host-side checks of the carried-state training entry points (no GPU): argument validation of wgnn_state_stash_bytes,
wgnn_fwd_state_stash and wgnn_bwd_state_part before any launch, the state stash's size, GCN_GRU.forward_with_state's
checks and TrainStep(carry_state=True)'s batch check."""
import ctypes

import pytest
import torch

from windgnn_amd import _lib as L


def _lib():
    return L.load()


def _dims(B=4, T=24, S=34, H=102, math=0, fmt=0, nnz=0, io=0):
    return L.Dims(B, T, S, 13, H, math, fmt, nnz, io)


def _params(fill=0x1000):
    p = L.Params()
    for i, n in enumerate(L._SLOTS):
        setattr(p, n, fill + 0x100000 * (i + 1))
    return p


def _grads(fill=0x9000000):
    g = L.Grads()
    for i, n in enumerate(L._SLOTS):
        setattr(g, n, fill + 0x100000 * (i + 1))
    return g


def test_state_stash_covers_the_plain_stash():
    lib = _lib()
    for B in (1, 3, 5, 16, 200, 800, 4096):
        for T in (1, 2, 24):
            for H, math, fmt, nnz, S in ((102, 0, 0, 0, 34), (102, 1, 0, 0, 34), (102, 2, 0, 0, 34), (102, 3, 0, 0, 34),
                                         (200, 0, 0, 0, 7), (200, 1, 0, 0, 7), (102, 1, 1, 1600, 200)):
                d = _dims(B, T, S, H, math, fmt, nnz)
                plain, state = lib.wgnn_stash_bytes(ctypes.byref(d)), lib.wgnn_state_stash_bytes(ctypes.byref(d))
                assert plain > 0 and state >= plain + 4 * B * H, (B, T, H, math, fmt)
    assert lib.wgnn_state_stash_bytes(ctypes.byref(_dims(B=0))) == 0


def test_stash_bytes_unchanged():
    """wgnn_stash_bytes is the plain forward's: the state stash did not grow it (bench.py's shape, exact and split modes)."""
    lib = _lib()
    d32, d16 = _dims(B=4096, math=0), _dims(B=4096, math=1)
    a, b = lib.wgnn_stash_bytes(ctypes.byref(d32)), lib.wgnn_stash_bytes(ctypes.byref(d16))
    assert a < lib.wgnn_state_stash_bytes(ctypes.byref(d32)) and b < lib.wgnn_state_stash_bytes(ctypes.byref(d16))


def test_entry_points_refuse_before_any_launch():
    lib = _lib()
    d = _dims()
    p, g = _params(), _grads()
    ws = lib.wgnn_workspace_bytes(ctypes.byref(d))
    V = ctypes.c_void_p
    A, X, Y, hn, stash, w = V(0x10), V(0x20000), V(0x4000000), V(0x8000000), V(0xA000000), V(0xE000000)
    f = lib.wgnn_fwd_state_stash
    assert f(None, A, X, ctypes.byref(p), None, Y, hn, stash, w, ws, None) == -1
    assert f(ctypes.byref(d), A, X, ctypes.byref(p), None, None, hn, stash, w, ws, None) == -1      # Y is required
    assert f(ctypes.byref(d), A, X, ctypes.byref(p), None, Y, hn, None, w, ws, None) == -1          # so is the stash
    assert f(ctypes.byref(d), A, X, ctypes.byref(L.Params()), None, Y, hn, stash, w, ws, None) == -1
    assert f(ctypes.byref(_dims(B=0)), A, X, ctypes.byref(p), None, Y, hn, stash, w, ws, None) == -2
    assert f(ctypes.byref(d), A, X, ctypes.byref(p), Y, Y, hn, stash, w, ws, None) == -5            # h0 overlaps Y
    assert f(ctypes.byref(d), A, X, ctypes.byref(p), hn, Y, hn, stash, w, ws, None) == -5           # h0 is h_n
    assert f(ctypes.byref(d), A, X, ctypes.byref(p), None, Y, V(Y.value + 64), stash, w, ws, None) == -5
    assert f(ctypes.byref(d), A, X, ctypes.byref(p), None, Y, hn, stash, w, 16, None) == -4
    b = lib.wgnn_bwd_state_part
    dY, dhn, dh0 = V(0x20000000), V(0x30000000), V(0x31000000)
    assert b(None, A, X, ctypes.byref(p), Y, dY, dhn, stash, ctypes.byref(g), dh0, w, ws, None, 7) == -1
    assert b(ctypes.byref(d), A, X, ctypes.byref(p), Y, None, dhn, stash, ctypes.byref(g), dh0, w, ws, None, 7) == -1
    assert b(ctypes.byref(d), A, X, ctypes.byref(p), Y, dY, dhn, None, ctypes.byref(g), dh0, w, ws, None, 7) == -1
    assert b(ctypes.byref(d), A, X, ctypes.byref(p), Y, dY, dhn, stash, None, dh0, w, ws, None, 7) == -1
    assert b(ctypes.byref(d), A, X, ctypes.byref(p), Y, dY, dhn, stash, ctypes.byref(g), dh0, w, ws, None, 0) == -2
    assert b(ctypes.byref(d), A, X, ctypes.byref(p), Y, dY, dhn, stash, ctypes.byref(g), dh0, w, ws, None, 8) == -2
    assert b(ctypes.byref(d), A, X, ctypes.byref(p), Y, dY, dhn, stash, ctypes.byref(g), dhn, w, ws, None, 7) == -5
    assert b(ctypes.byref(d), A, X, ctypes.byref(p), Y, dY, dhn, stash, ctypes.byref(g), dY, w, ws, None, 7) == -5
    assert b(ctypes.byref(d), A, X, ctypes.byref(p), Y, dY, dhn, stash, ctypes.byref(g), stash, w, ws, None, 7) == -5
    assert b(ctypes.byref(d), A, X, ctypes.byref(p), Y, dY, dhn, stash, ctypes.byref(g), dh0, w, 16, None, 7) == -4
    assert b(ctypes.byref(_dims(H=0)), A, X, ctypes.byref(p), Y, dY, dhn, stash, ctypes.byref(g), dh0, w, ws, None, 7) == -2


def _model(**kw):
    from windgnn_amd import GCN_GRU
    return GCN_GRU(13, 13, 13, 34 * 13, 102, **kw)


def test_forward_with_state_refuses_bad_arguments():
    m = _model()
    A, X = torch.rand(34, 34), torch.rand(2, 3, 34, 13)
    with pytest.raises(RuntimeError, match="hx must be"):
        m.forward_with_state(A, X, torch.zeros(2, 2, 102))
    with pytest.raises(RuntimeError, match="hx must be"):
        m.forward_with_state(A, X, torch.zeros(1, 2, 102, dtype=torch.float64))
    with pytest.raises(RuntimeError, match="attr_matrix must be"):
        m.forward_with_state(A, X[0], None)
    with pytest.raises(RuntimeError, match="MI355X"):         # CPU tensors: no fallback
        m.forward_with_state(A, X, torch.zeros(1, 2, 102, requires_grad=True))
    wide = __import__("windgnn_amd").GCN_GRU(13, 16, 13, 34 * 16, 102)
    with pytest.raises(RuntimeError, match="13 / 13 widths"):
        wide.forward_with_state(A, X, None)


def test_trainstep_carry_state_refuses_a_changed_batch():
    from windgnn_amd.trainer import TrainStep
    tr = TrainStep(_model(), carry_state=True)
    assert tr.state is None
    tr._hbuf, tr._has_state = torch.zeros(2, 4, 102), True      # as after a step with B = 4
    with pytest.raises(RuntimeError, match="batch changed from 4 to 5"):
        tr.step(torch.rand(34, 34), torch.rand(5, 3, 34, 13), torch.rand(5, 3, 102))
    with pytest.raises(RuntimeError, match="fp32"):
        tr.step(torch.rand(34, 34), torch.rand(4, 3, 34, 13, dtype=torch.float16), torch.rand(4, 3, 102))
    tr.reset_state()
    assert tr.state is None
