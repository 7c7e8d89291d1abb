"""Carried GRU state on the MI355X: wgnn_fwd_state over every recurrence path (zero state = the old forward bit for bit,
chunks compose, a random h0 against a host fp64 nn.GRU), the one-launch hourly step (csrc/gru_step.hip) against the
windowed forward, GCN_GRU.forward_state and StreamingForecaster."""
import pytest
import torch

from conftest import max_abs

pytestmark = pytest.mark.gpu

Y_TOL = 1e-4          # the suite's bars (tests/test_gpu_parity.py)
F16_Y_TOL = 2e-2
IO_ROUND = {torch.float32: 0.0, torch.float16: 2.5e-4, torch.bfloat16: 2.0e-3}
MATH = {"f32": 0, "f16x3": 1, "f16": 2, "f16x3g": 3}

# the path matrix of wgnn_fwd_state: (id, S, T, B, H, math, io dtype, CSR k-NN degree or 0)
CASES = [
    ("f32_small", 34, 24, 5, 102, "f32", torch.float32, 0),        # gru_small_fwd (B <= 768)
    ("f32_big", 34, 6, 800, 102, "f32", torch.float32, 0),         # gru_fwd (B > 768)
    ("f16x3", 34, 24, 8, 102, "f16x3", torch.float32, 0),          # grux_fwd behind the fused gcngi front end
    ("f16x3g", 34, 24, 8, 102, "f16x3g", torch.float32, 0),
    ("f16", 34, 24, 8, 102, "f16", torch.float32, 0),
    ("bf16_io", 34, 24, 8, 102, "f16x3", torch.bfloat16, 0),       # 16-bit I/O: h_n stays unrounded fp32
    ("f32_wide", 7, 8, 4, 200, "f32", torch.float32, 0),           # gru_gen_fwd (per-step GEMM)
    ("f16x3_wide", 7, 8, 4, 200, "f16x3", torch.float32, 0),       # gru_gen_fwd_x3 (per-step plane GEMM)
    ("csr_f32", 200, 6, 3, 102, "f32", torch.float32, 8),          # CSR front end
    ("csr_f16x3", 200, 6, 3, 102, "f16x3", torch.float32, 8),
]


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _setup(S, T, B, H, iodt, k, seed=0):
    from oracle import windgnn_oracle as orc
    g = torch.Generator().manual_seed(1000 + S + T + B + H + seed)
    if k:
        from windgnn_amd.graph import CsrAdjacency, build_knn_adjacency, synthetic_station_coords
        csr = CsrAdjacency(*build_knn_adjacency(synthetic_station_coords(S, seed=S), k))
        A_host, A_dev = csr.dense(), csr.to(_dev())
    else:
        A_host = torch.rand(S, S, generator=g) / S + 0.01
        A_dev = A_host.to(_dev())
    X = torch.rand(B, T, S, 13, generator=g).to(iodt)
    p = orc.init_params(S, 13, H, seed=S + H)
    params = [p[k_].to(_dev()).contiguous() for k_ in orc.PARAM_KEYS]
    return A_host, A_dev, X, p, params, g


def _fp64_forward(A, X, p, h0):
    """Host float64 restatement with nn.GRU called with hx: two relu(A X W + b) layers, then the GRU."""
    A, X = A.double(), X.double()
    h = torch.relu(torch.matmul(torch.matmul(A, X), p["conv1.weight"].double()) + p["conv1.bias"].double())
    h = torch.relu(torch.matmul(torch.matmul(A, h), p["conv2.weight"].double()) + p["conv2.bias"].double())
    B, T, S, F = X.shape
    H = p["gru.weight_hh_l0"].shape[1]
    gru = torch.nn.GRU(S * F, H, batch_first=True).double()
    with torch.no_grad():
        for name in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
            getattr(gru, name).copy_(p["gru." + name].double())
        Y, hn = gru(h.reshape(B, T, S * F), h0.double().unsqueeze(0))
    return Y, hn[0]


def _tol(math, iodt):
    return (F16_Y_TOL if math == "f16" else Y_TOL) + IO_ROUND[iodt]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_state_paths(case):
    from windgnn_amd.functional import gcn_gru_forward_raw, gcn_gru_state
    name, S, T, B, H, math, iodt, k = case
    dev = _dev()
    A_host, A, X, p, params, g = _setup(S, T, B, H, iodt, k)
    Xd = X.to(dev)
    m = MATH[math]
    tol = _tol(math, iodt)
    with torch.no_grad():
        # 1. zero state is the old forward, bit for bit; h_n is the last row (unrounded with 16-bit I/O)
        Y_ref, _, _ = gcn_gru_forward_raw(A, Xd, params, m, want_stash=False)
        Y0, hn0 = gcn_gru_state(A, Xd, params, m)
        torch.cuda.synchronize()
        assert torch.equal(Y0, Y_ref), name
        assert hn0.dtype == torch.float32 and tuple(hn0.shape) == (B, H)
        if iodt == torch.float32:
            assert torch.equal(hn0, Y0[:, -1]), name
        else:
            assert max_abs(hn0.cpu(), Y0[:, -1].float().cpu()) <= IO_ROUND[iodt], name
            assert not torch.equal(hn0, Y0[:, -1].float()), "h_n went through the rounded Y"
        _, hn_only = gcn_gru_state(A, Xd, params, m, want_y=False)       # Y = NULL: h_n alone, same bits
        assert torch.equal(hn_only, hn0), name
        # 2. chunks compose: h_n of the first chunk as h0 of the second
        T1 = max(1, T // 3)
        Y1, hn1 = gcn_gru_state(A, Xd[:, :T1].contiguous(), params, m)
        Y2, hn2 = gcn_gru_state(A, Xd[:, T1:].contiguous(), params, m, h0=hn1)
        e_chunk = max_abs(torch.cat([Y1, Y2], 1).float().cpu(), Y0.float().cpu())
        e_hn = max_abs(hn2.cpu(), hn0.cpu())
        print("%s: chunked vs whole max|dY| = %.2e, max|dh_n| = %.2e" % (name, e_chunk, e_hn))
        assert e_chunk <= tol and e_hn <= tol, (name, e_chunk, e_hn)
        # 3. a random h0 against the host fp64 nn.GRU called with hx
        h0 = (torch.rand(B, H, generator=g) * 2 - 1) * 0.8
        Yr, hnr = gcn_gru_state(A, Xd, params, m, h0=h0.to(dev))
        Yo, hno = _fp64_forward(A_host, X.float(), p, h0)
        e_y, e_h = max_abs(Yr.float().cpu(), Yo), max_abs(hnr.cpu(), hno)
        print("%s: random h0 vs fp64 max|dY| = %.2e, max|dh_n| = %.2e" % (name, e_y, e_h))
        assert e_y <= tol and e_h <= tol, (name, e_y, e_h)


def _profiled(fn):
    from windgnn_amd import _lib
    _lib.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        prof = {r["name"]: r["launches"] for r in _lib.profile_read()}
    finally:
        _lib.profile_enable(False)
    return out, prof


@pytest.mark.parametrize("math", ["f32", "f16x3"])
@pytest.mark.parametrize("B", [1, 256, 257])       # 256 = _lib.STEP_MAX_B: the step kernel's bound; 257 the fallback
def test_hourly_step_reproduces_the_windowed_forward(B, math):
    from windgnn_amd import _lib
    from windgnn_amd.functional import gcn_gru_forward_raw, gcn_gru_state
    assert _lib.STEP_MAX_B == 256
    S, T, H = 34, 12, 102
    dev = _dev()
    _, A, X, _, params, _ = _setup(S, T, B, H, torch.float32, 0, seed=B)
    Xd = X.to(dev)
    m = MATH[math]
    with torch.no_grad():
        Y_ref, _, _ = gcn_gru_forward_raw(A, Xd, params, m, want_stash=False)
        h = None
        worst = 0.0
        for t in range(T):
            x_t = Xd[:, t:t + 1].contiguous()
            (Y_t, h_next), prof = _profiled(lambda: gcn_gru_state(A, x_t, params, m, h0=h))
            if B <= _lib.STEP_MAX_B:
                assert prof == {"gru_step_kernel": 1}, prof        # the whole hour is ONE launch
            else:
                assert "gru_step_kernel" not in prof, prof
            assert torch.equal(Y_t[:, 0], h_next)
            worst = max(worst, max_abs(Y_t[:, 0].cpu(), Y_ref[:, t].cpu()))
            h = h_next
        print("step B=%d %s: max|step - windowed| over %d hours = %.2e" % (B, math, T, worst))
        assert worst <= Y_TOL, worst


def test_forward_state_follows_nn_gru_shapes():
    from oracle import windgnn_oracle as orc
    from windgnn_amd import GCN_GRU
    dev = _dev()
    S, T, H = 7, 5, 21
    p = orc.init_params(S, 13, H, seed=3)
    m = GCN_GRU(13, 13, 13, S * 13, H).to(dev)
    m.load_state_dict(p)
    A = (torch.rand(S, S) / S + 0.01).to(dev)
    with torch.no_grad():
        X1 = torch.rand(1, T, S, 13, device=dev)
        out, hn = m.forward_state(A, X1)
        assert tuple(out.shape) == (T, H) and tuple(hn.shape) == (1, 1, H)
        assert torch.equal(out, m(A, X1))
        assert torch.equal(hn[0, 0], out[-1])
        X3 = torch.rand(3, T, S, 13, device=dev)
        out3, hn3 = m.forward_state(A, X3)
        assert tuple(out3.shape) == (3, T, H) and tuple(hn3.shape) == (1, 3, H)
        hx = torch.rand(1, 3, H, device=dev)
        o_a, h_a = m.forward_state(A, X3, hx)
        o_b, h_b = m.forward_state(A, X3, hx[0])                 # hx as [B, H]
        assert torch.equal(o_a, o_b) and torch.equal(h_a, h_b)
        assert not torch.equal(o_a, out3)
    with pytest.raises(RuntimeError, match=r"torch\.no_grad"):
        m.forward_state(A, X3)


def test_state_buffers_may_not_alias():
    from windgnn_amd.functional import gcn_gru_state
    dev = _dev()
    _, A, X, _, params, _ = _setup(7, 3, 2, 21, torch.float32, 0)
    h = torch.zeros(2, 21, device=dev)
    with pytest.raises(RuntimeError, match=r"wgnn_fwd_state"):
        gcn_gru_state(A, X.to(dev), params, 0, h0=h, h_n=h)


@pytest.mark.parametrize("math", ["f32", "f16x3"])
def test_streaming_forecaster_matches_the_prefix_forward(math):
    """2 x 168 + 3 hours of a synthetic two-site series, pushed hour by hour: every forecast equals data.forward_last of
    the prefix of the current reference window, across the automatic reset at hour 168 and 336."""
    from oracle import windgnn_oracle as orc
    from windgnn_amd import GCN_GRU, StreamingForecaster
    from windgnn_amd.data import forward_last
    dev = _dev()
    S, H, W = 34, 102, 168
    p = orc.init_params(S, 13, H, seed=11)
    m = GCN_GRU(13, 13, 13, S * 13, H, math=math).to(dev)
    m.load_state_dict(p)
    m.requires_grad_(False)
    g = torch.Generator().manual_seed(5)
    A = (torch.rand(S, S, generator=g) / S + 0.01).to(dev)
    hours = 2 * W + 3
    tt = torch.arange(hours, dtype=torch.float32)[:, None, None]
    series = (0.5 + 0.4 * torch.sin(tt / 9.0 + torch.rand(2, 1, S, 13, generator=g) * 6)
              + 0.05 * torch.rand(2, hours, S, 13, generator=g)).clamp(0, 1).to(dev)     # [2 sites, hours, S, 13]
    wmin, wmax = 0.3, 14.0
    fc = StreamingForecaster(m, A, wmin, wmax, n_streams=2, window=W)
    worst = 0.0
    with torch.no_grad():
        for t in range(hours):
            got = fc.push(series[:, t])
            w0 = (t // W) * W
            ref = forward_last(m, A, series[:, w0:t + 1].contiguous(), wmin, wmax)
            worst = max(worst, max_abs(got.cpu(), ref.cpu()))
            assert fc.hours == t - w0 + 1
    print("forecaster %s: max|push - forward_last(prefix)| over %d hours = %.2e" % (math, hours, worst))
    assert worst <= Y_TOL * (wmax - wmin), worst
    fc.reset()
    assert fc.hours == 0 and float(fc.state.abs().max()) == 0.0
    with torch.no_grad():
        one = StreamingForecaster(m, A, wmin, wmax)          # one stream, [S, 13] input
        out = one.push(series[0, 0])
    assert tuple(out.shape) == (1, H)
