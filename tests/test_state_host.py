"""CPU-side checks of the carried-state entry point (wgnn_fwd_state) and its Python layers: export, argument validation
before any launch, and the inference-only guard of GCN_GRU.forward_state.  No GPU needed."""
import ctypes as C

import pytest
import torch

from conftest import ROOT  # noqa: F401  (puts the repository on sys.path)


def _lib():
    from windgnn_amd import _lib as L
    from windgnn_amd import build
    build.build(verbose=False)
    return L, L.load()


def _dims(L, B=2, T=3, S=4, F=13, H=12, math=0, adj=0, nnz=0, io=0):
    return L.Dims(B, T, S, F, H, math, adj, nnz, io)


def test_fwd_state_is_exported_with_its_prototype():
    L, lib = _lib()
    assert "wgnn_fwd_state" in L.EXPORTS
    assert hasattr(lib, "wgnn_fwd_state")
    res, args = L.EXPORTS["wgnn_fwd_state"]
    assert res is C.c_int and len(args) == 10


def _fake_call(lib, L, d, Y=1 << 24, hn=1 << 28, h0=0, ws=1 << 40, ws_bytes=1 << 40):
    # non-NULL fake device pointers: every call below must be refused on the host before anything is launched
    p = L.Params(*([4096] * 8), None)
    return lib.wgnn_fwd_state(C.byref(d), C.c_void_p(8192), C.c_void_p(1 << 20), C.byref(p), C.c_void_p(h0),
                              C.c_void_p(Y), C.c_void_p(hn), C.c_void_p(ws), ws_bytes, None)


def test_fwd_state_null_and_shape_errors_match_wgnn_fwd():
    L, lib = _lib()
    d = _dims(L)
    assert _fake_call(lib, L, d, Y=0, hn=0) == -1                          # WGNN_ERR_NULL: neither output
    for bad in (_dims(L, B=0), _dims(L, T=0), _dims(L, F=12), _dims(L, H=0)):
        assert _fake_call(lib, L, bad) == -2                                # WGNN_ERR_SHAPE, as wgnn_fwd
        p = L.Params(*([4096] * 8), None)
        assert lib.wgnn_fwd(C.byref(bad), C.c_void_p(8192), C.c_void_p(1 << 20), C.byref(p), C.c_void_p(1), None,
                            C.c_void_p(1 << 40), 1 << 40, None) == -2
    for bad in (_dims(L, S=65), _dims(L, math=0, io=1)):                   # dense S > 64; 16-bit I/O in exact fp32
        assert _fake_call(lib, L, bad) == -5                                # WGNN_ERR_UNSUPPORTED, as wgnn_fwd
        p = L.Params(*([4096] * 8), None)
        assert lib.wgnn_fwd(C.byref(bad), C.c_void_p(8192), C.c_void_p(1 << 20), C.byref(p), C.c_void_p(1), None,
                            C.c_void_p(1 << 40), 1 << 40, None) == -5
    assert _fake_call(lib, L, _dims(L, math=7)) == -3                      # WGNN_ERR_DTYPE
    assert _fake_call(lib, L, d, ws_bytes=16) == -4                        # WGNN_ERR_WORKSPACE


def test_fwd_state_refuses_overlapping_state_buffers():
    L, lib = _lib()
    d = _dims(L)                                                            # B*H*4 = 96 bytes of state
    assert _fake_call(lib, L, d, h0=1 << 30, hn=1 << 30) == -5             # h0 == h_n
    assert _fake_call(lib, L, d, h0=1 << 30, hn=(1 << 30) + 64) == -5      # partial overlap
    assert _fake_call(lib, L, d, h0=1 << 30, Y=(1 << 30) - 16, hn=0) == -5  # h0 inside Y


def _model():
    from windgnn_amd import GCN_GRU
    return GCN_GRU(13, 13, 13, 4 * 13, 12)


def test_forward_state_refuses_grad_mode_before_any_launch():
    m = _model()
    with pytest.raises(RuntimeError, match=r"torch\.no_grad"):
        m.forward_state(torch.rand(4, 4), torch.rand(1, 3, 4, 13))
    hx = torch.zeros(1, 1, 12, requires_grad=True)
    m.requires_grad_(False)
    with pytest.raises(RuntimeError, match=r"torch\.no_grad"):
        m.forward_state(torch.rand(4, 4), torch.rand(1, 3, 4, 13), hx)


def test_forward_state_refuses_bad_hx_and_cpu_tensors():
    m = _model()
    with torch.no_grad():
        with pytest.raises(RuntimeError, match=r"hx must be"):
            m.forward_state(torch.rand(4, 4), torch.rand(2, 3, 4, 13), torch.zeros(1, 3, 12))
        with pytest.raises(RuntimeError, match=r"hx must be"):
            m.forward_state(torch.rand(4, 4), torch.rand(2, 3, 4, 13), torch.zeros(2, 13))
        with pytest.raises(RuntimeError, match=r"MI355X|no CPU fallback"):
            m.forward_state(torch.rand(4, 4), torch.rand(2, 3, 4, 13), torch.zeros(1, 2, 12))
        with pytest.raises(RuntimeError, match=r"MI355X|no CPU fallback"):
            m.forward_state(torch.rand(4, 4), torch.rand(2, 3, 4, 13))


def test_forward_state_other_widths_are_out_of_scope():
    from windgnn_amd import GCN_GRU
    m = GCN_GRU(7, 9, 13, 4 * 13, 12)
    with torch.no_grad(), pytest.raises(RuntimeError, match=r"13 / 13"):
        m.forward_state(torch.rand(4, 4), torch.rand(1, 3, 4, 7))


def test_gcn_gru_state_refuses_cpu_tensors():
    from windgnn_amd.functional import gcn_gru_state
    params = [p.detach() for p in _model().hot_path_parameters()]
    with pytest.raises(RuntimeError, match=r"MI355X|no CPU fallback"):
        gcn_gru_state(torch.rand(4, 4), torch.rand(2, 3, 4, 13), params, 0)


def test_streaming_forecaster_is_exported():
    import windgnn_amd
    assert "StreamingForecaster" in windgnn_amd.__all__
    with pytest.raises(RuntimeError, match=r"13 / 13"):
        windgnn_amd.StreamingForecaster(windgnn_amd.GCN_GRU(7, 9, 13, 52, 12), torch.rand(4, 4), 0.0, 1.0)
