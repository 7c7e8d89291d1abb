"""Training through a carried GRU state on the MI355X (truncated BPTT): wgnn_fwd_state_stash + wgnn_bwd_state_part on every
recurrence path against a host fp64 nn.GRU with hx (all 8 gradients and dh0 of sum(Y dY) + sum(h_n dh_n)), the zero state
against wgnn_fwd + wgnn_bwd_part bit for bit, chunks composing into the whole window, GCN_GRU.forward_with_state under
autograd and TrainStep(carry_state=True) against an fp64 loop with torch.optim.Adam."""
import pytest
import torch

from conftest import PARAM_KEYS, max_abs, rel_to_max

pytestmark = pytest.mark.gpu

Y_TOL = 1e-4          # the suite's bars (tests/test_gpu_parity.py)
G_TOL = 1e-4
F16_Y_TOL = 2e-2
F16_G_TOL = 5e-2
IO_ROUND = {torch.float32: 0.0, torch.float16: 2.5e-4, torch.bfloat16: 2.0e-3}
MATH = {"f32": 0, "f16x3": 1, "f16": 2, "f16x3g": 3}

# (id, S, T, B, H, math, io dtype, CSR k-NN degree or 0): tests/test_gpu_state.py's path matrix, the large-B*T forms and T = 1
CASES = [
    ("f32_small", 34, 24, 5, 102, "f32", torch.float32, 0),        # gru_small (B <= 768), general fp32 dW_hh GEMM
    ("f32_big", 34, 6, 800, 102, "f32", torch.float32, 0),         # gru (register-resident MFMA)
    ("f16x3", 34, 24, 5, 102, "f16x3", torch.float32, 0),          # grux, pgemm_tn with per-window h0 rows
    ("f16x3g", 34, 24, 8, 102, "f16x3g", torch.float32, 0),
    ("f16", 34, 24, 8, 102, "f16", torch.float32, 0),
    ("bf16_io", 34, 24, 8, 102, "f16x3", torch.bfloat16, 0),       # 16-bit I/O: the stash keeps the unrounded h
    ("f32_wide", 7, 8, 4, 200, "f32", torch.float32, 0),           # general per-step GEMM recurrences
    ("f16x3_wide", 7, 8, 4, 200, "f16x3", torch.float32, 0),
    ("csr_f32", 200, 6, 3, 102, "f32", torch.float32, 8),          # CSR front end
    ("csr_f16x3", 200, 6, 3, 102, "f16x3", torch.float32, 8),
    ("f32_g32", 34, 24, 200, 102, "f32", torch.float32, 0),        # B*T = 4800: gemm32_tn on the [Hprev | 1] rows
    ("f32_g32_dghn", 34, 6, 800, 102, "f32", torch.float32, 0),    # B*T = 4800, gru + two-source dGHn operand
    ("f16x3g_big", 34, 24, 200, 102, "f16x3g", torch.float32, 0),  # single-plane dGI / dGHn
    ("f32_t1", 34, 1, 5, 102, "f32", torch.float32, 0),            # T = 1 through the windowed kernels
    ("f16x3_t1", 34, 1, 5, 102, "f16x3", torch.float32, 0),
    ("f32_wide_t1", 7, 1, 3, 200, "f32", torch.float32, 0),
    ("f16x3_wide_t1", 7, 1, 3, 200, "f16x3", torch.float32, 0),
]


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _setup(S, T, B, H, iodt, k, seed=0):
    from oracle import windgnn_oracle as orc
    g = torch.Generator().manual_seed(2000 + S + T + B + H + seed)
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


def _fp64_model(p):
    """The 8 tensors as fp64 leaves, and f(A, X, h0) -> (Y, h_n): two relu(A X W + b) layers, then nn.GRU with hx."""
    leaves = {k: p[k].double().clone().requires_grad_(True) for k in PARAM_KEYS}

    def f(A, X, h0):
        A, X = A.double(), X.double()
        h = torch.relu(torch.matmul(torch.matmul(A, X), leaves["conv1.weight"]) + leaves["conv1.bias"])
        h = torch.relu(torch.matmul(torch.matmul(A, h), leaves["conv2.weight"]) + leaves["conv2.bias"])
        B, T, S, F = X.shape
        Y, hn = torch._VF.gru(h.reshape(B, T, S * F), h0.unsqueeze(0),
                              [leaves["gru.weight_ih_l0"], leaves["gru.weight_hh_l0"], leaves["gru.bias_ih_l0"],
                               leaves["gru.bias_hh_l0"]], True, 1, 0.0, False, False, True)
        return Y, hn[0]
    return leaves, f


def _tols(name, math, iodt):
    if math == "f16":
        return F16_Y_TOL + IO_ROUND[iodt], F16_G_TOL
    g = 1e-3 if name == "f16x3g_big" else G_TOL
    return Y_TOL + IO_ROUND[iodt], g


def _grads(params):
    return [torch.empty_like(q) for q in params]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_state_backward_against_fp64(case):
    """Random h0, dY and dh_n: Y, h_n, the 8 gradients and dh0 against fp64 autograd of sum(Y dY) + sum(h_n dh_n)."""
    from windgnn_amd.functional import gcn_gru_state_backward_raw, gcn_gru_state_forward_raw
    name, S, T, B, H, math, iodt, k = case
    dev = _dev()
    A_host, A, X, p, params, g = _setup(S, T, B, H, iodt, k)
    h0 = (torch.rand(B, H, generator=g) * 1.6 - 0.8)
    dY = torch.randn(B, T, H, generator=g) * 1e-3
    dhn = torch.randn(B, H, generator=g) * 1e-3
    y_tol, g_tol = _tols(name, math, iodt)
    Y, hn, stash, d = gcn_gru_state_forward_raw(A, X.to(dev), params, MATH[math], h0.to(dev))
    grads = _grads(params)
    dh0 = torch.empty(B, H, device=dev)
    gcn_gru_state_backward_raw(d, A, X.to(dev), params, Y, dY.to(dev), dhn.to(dev), stash, grads, dh0)
    torch.cuda.synchronize()
    leaves, f = _fp64_model(p)
    h0r = h0.double().requires_grad_(True)
    Yr, hnr = f(A_host, X.float(), h0r)
    ((Yr * dY.double()).sum() + (hnr * dhn.double()).sum()).backward()
    assert max_abs(Y.float().cpu(), Yr.detach()) <= y_tol, name
    assert max_abs(hn.cpu(), hnr.detach()) <= y_tol - IO_ROUND[iodt], name
    for key, gk in zip(PARAM_KEYS, grads):
        assert rel_to_max(gk.cpu(), leaves[key].grad) <= g_tol, (name, key)
    assert rel_to_max(dh0.cpu(), h0r.grad) <= g_tol, (name, "dh0")


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_zero_state_is_the_plain_training_step_bitwise(case):
    """h0 = dh_n = dh0 = NULL: wgnn_fwd_state_stash + wgnn_bwd_state_part equal wgnn_fwd + wgnn_bwd_part bit for bit."""
    from windgnn_amd.functional import (gcn_gru_backward_raw, gcn_gru_forward_raw, gcn_gru_state_backward_raw,
                                        gcn_gru_state_forward_raw)
    name, S, T, B, H, math, iodt, k = case
    dev = _dev()
    _, A, X, _, params, g = _setup(S, T, B, H, iodt, k)
    Xd = X.to(dev)
    dY = (torch.randn(B, T, H, generator=g) * 1e-3).to(dev)
    Y0, stash0, d0 = gcn_gru_forward_raw(A, Xd, params, MATH[math])
    g0 = _grads(params)
    gcn_gru_backward_raw(d0, A, Xd, params, Y0, dY, stash0, g0)
    Y1, hn1, stash1, d1 = gcn_gru_state_forward_raw(A, Xd, params, MATH[math])
    g1 = _grads(params)
    gcn_gru_state_backward_raw(d1, A, Xd, params, Y1, dY, None, stash1, g1)
    torch.cuda.synchronize()
    assert torch.equal(Y0, Y1), name
    for key, a, b in zip(PARAM_KEYS, g0, g1):
        assert torch.equal(a, b), (name, key)


@pytest.mark.parametrize("case", [c for c in CASES if c[2] >= 2], ids=[c[0] for c in CASES if c[2] >= 2])
def test_chunks_compose(case):
    """Forward X[:, :T1] then X[:, T1:] from its h_n; backward chunk 2, then chunk 1 with chunk 2's dh0 as its dh_n: the
    summed gradients and chunk 1's dh0 equal those of the whole window."""
    from windgnn_amd.functional import gcn_gru_state_backward_raw, gcn_gru_state_forward_raw
    name, S, T, B, H, math, iodt, k = case
    dev = _dev()
    _, A, X, _, params, g = _setup(S, T, B, H, iodt, k)
    _, g_tol = _tols(name, math, iodt)
    m = MATH[math]
    h0 = (torch.rand(B, H, generator=g) * 1.6 - 0.8).to(dev)
    dY = (torch.randn(B, T, H, generator=g) * 1e-3).to(dev)
    dhn = (torch.randn(B, H, generator=g) * 1e-3).to(dev)
    T1 = T // 2
    Xd = X.to(dev)
    Y, hn, st, d = gcn_gru_state_forward_raw(A, Xd, params, m, h0)
    gw, dh0w = _grads(params), torch.empty(B, H, device=dev)
    gcn_gru_state_backward_raw(d, A, Xd, params, Y, dY, dhn, st, gw, dh0w)
    X1, X2 = Xd[:, :T1].contiguous(), Xd[:, T1:].contiguous()
    Y1, hn1, st1, d1 = gcn_gru_state_forward_raw(A, X1, params, m, h0)
    Y2, hn2, st2, d2 = gcn_gru_state_forward_raw(A, X2, params, m, hn1)
    g2, dh0_2 = _grads(params), torch.empty(B, H, device=dev)
    gcn_gru_state_backward_raw(d2, A, X2, params, Y2, dY[:, T1:].contiguous(), dhn, st2, g2, dh0_2)
    g1, dh0_1 = _grads(params), torch.empty(B, H, device=dev)
    gcn_gru_state_backward_raw(d1, A, X1, params, Y1, dY[:, :T1].contiguous(), dh0_2, st1, g1, dh0_1)
    torch.cuda.synchronize()
    y_tol = (F16_Y_TOL if math == "f16" else Y_TOL) + IO_ROUND[iodt]
    assert max_abs(torch.cat([Y1, Y2], 1).float().cpu(), Y.float().cpu()) <= y_tol, name
    assert max_abs(hn2.cpu(), hn.cpu()) <= y_tol, name
    for key, a, b, w in zip(PARAM_KEYS, g1, g2, gw):
        assert rel_to_max((a + b).cpu(), w.cpu()) <= g_tol, (name, key)
    assert rel_to_max(dh0_1.cpu(), dh0w.cpu()) <= g_tol, (name, "dh0")


@pytest.mark.parametrize("math", ["f32", "f16x3"])
def test_forward_with_state_autograd(math):
    """GCN_GRU.forward_with_state: .grad of the 8 parameters and of hx with a loss on both out and h_n, against fp64; under
    torch.no_grad() it is forward_state."""
    from windgnn_amd import GCN_GRU
    dev = _dev()
    S, T, B, H = 34, 12, 5, 102
    A_host, A, X, p, _, g = _setup(S, T, B, H, torch.float32, 0, seed=7)
    L = torch.rand(B, T, H, generator=g)
    hx = (torch.rand(1, B, H, generator=g) * 1.6 - 0.8)
    m = GCN_GRU(13, 13, 13, S * 13, H, math=math).to(dev)
    m.load_state_dict(p)
    hxd = hx.to(dev).requires_grad_(True)
    out, h_n = m.forward_with_state(A, X.to(dev), hxd)
    assert tuple(h_n.shape) == (1, B, H)
    loss = ((out - L.to(dev)) ** 2).mean() + (h_n ** 2).sum() * 1e-3
    loss.backward()
    leaves, f = _fp64_model(p)
    hr = hx[0].double().requires_grad_(True)
    Yr, hnr = f(A_host, X, hr)
    (((Yr - L.double()) ** 2).mean() + (hnr ** 2).sum() * 1e-3).backward()
    for key, prm in m.named_parameters():
        assert rel_to_max(prm.grad.cpu(), leaves[key].grad) <= G_TOL, (math, key)
    assert rel_to_max(hxd.grad[0].cpu(), hr.grad) <= G_TOL, (math, "hx")
    with torch.no_grad():
        o1, h1 = m.forward_with_state(A, X.to(dev), hx.to(dev))
        o2, h2 = m.forward_state(A, X.to(dev), hx.to(dev))
    assert torch.equal(o1, o2) and torch.equal(h1, h2)


@pytest.mark.parametrize("math", ["f32", "f16x3"])
def test_trainstep_carry_state_against_fp64_adam(math):
    """TrainStep(carry_state=True), 3 steps over consecutive chunks of a seeded series, against an fp64 loop that carries a
    detached hx and steps torch.optim.Adam: the losses, the parameters after every step and the carried state."""
    from windgnn_amd import GCN_GRU
    from windgnn_amd.trainer import TrainStep
    dev = _dev()
    S, T, B, H, steps = 34, 8, 4, 102, 3
    A_host, A, _, p, _, g = _setup(S, T, B, H, torch.float32, 0, seed=11)
    series = torch.rand(B, steps * T + 1, S, 13, generator=g)           # B streams, consecutive chunks of T hours
    labels = torch.rand(B, steps * T, H, generator=g)
    m = GCN_GRU(13, 13, 13, S * 13, H, math=math).to(dev)
    m.load_state_dict(p)
    # eps = 1e-3 (both sides): Adam's first steps are ~lr sign(g), and a gradient element that is zero within fp32 rounding
    # would flip a parameter by 2 lr; with this eps the update is a smooth function of g
    tr = TrainStep(m, lr=1e-3, eps=1e-3, carry_state=True)
    assert tr.state is None
    leaves, f = _fp64_model(p)
    opt = torch.optim.Adam(list(leaves.values()), lr=1e-3, eps=1e-3)
    h = torch.zeros(B, H, dtype=torch.float64)
    for s in range(steps):
        X, L = series[:, s * T:(s + 1) * T].contiguous(), labels[:, s * T:(s + 1) * T].contiguous()
        loss, _ = tr.step(A, X.to(dev), L.to(dev))
        loss = float(loss)
        opt.zero_grad()
        Yr, hn = f(A_host, X, h)
        lr_ = ((Yr - L.double()) ** 2).mean()
        lr_.backward()
        opt.step()
        h = hn.detach()
        ref = float(lr_.detach())
        assert abs(loss - ref) <= 2e-4 * max(1.0, abs(ref)), (math, s, loss, ref)
        for key, prm in m.named_parameters():
            assert rel_to_max(prm.detach().cpu(), leaves[key].detach()) <= 1e-4, (math, s, key)
        assert max_abs(tr.state.cpu(), h) <= 1e-4, (math, s)
    st = tr.state
    st.zero_()                                       # a copy: the carried state is untouched
    assert float(tr.state.abs().max()) > 0
    tr.reset_state()
    assert tr.state is None
