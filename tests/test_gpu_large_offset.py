"""Parity at the largest batches the entry points accept: operands of a kernel launch past 2^31 and 2^32 bytes.

tests/large_offset_cases.py has the table and the method (a batch of period 48 against an fp64 oracle run on 48 windows; series
of period 45; layers over tiles of period 48; closed-form references for the element-wise entries);
tests/test_large_offset_host.py proves without a GPU that every case is accepted, crosses the threshold it names and that its
inputs would show a wrapped address.  Here, per case and math mode, on every row and never a sample:
  1. Y is prefilled with NaN, the stash and the workspace with NAN_WORD (status block zeroed): no NaN is left in Y;
  2. max |Y - Y_ref| is within the mode's existing bar;
  3. Y[48:] == Y[:-48] bit for bit;
  4. the loss and the 8 gradients meet the existing bars after wgnn_finish;
  5. check_range_status is clean.
A mismatch in 1-3 is an addressing defect; a gradient beyond its bar with 1-3 intact is a finding about summation."""
import ctypes as C
import os

import pytest
import torch

import large_offset_cases as lc
from conftest import PARAM_KEYS, rel_to_max
from guarded import NAN_WORD
from test_gpu_finish_regimes import X2_G_TOL          # f16x3g gradients from 4096 rows on
from test_gpu_gcn_loops import LAYER_TOL               # one GraphConvLayer: out and dX
from test_gpu_parity import F16_G_TOL, F16_Y_TOL, G_TOL, IO_ROUND, Y_TOL

pytestmark = pytest.mark.gpu

GIB = 2.0 ** 30
MEMORY_LIMIT_GIB = 64.0     # every case stays below it, comparisons included: measured per test, printed and asserted


@pytest.fixture(autouse=True)
def _peak_device_memory(request):
    """torch's peak of allocated device memory over the test (every buffer here is a torch tensor), printed and held to the limit."""
    torch.cuda.reset_peak_memory_stats()
    yield
    peak = torch.cuda.max_memory_allocated() / GIB
    print("large-offset %s: peak device memory %.1f GiB" % (request.node.name, peak))
    assert peak < MEMORY_LIMIT_GIB, peak


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _bars(math, io):
    """(Y, gradient, loss) bars of a mode: the suite's own (tests/test_gpu_parity.py)."""
    y = (F16_Y_TOL if math == "f16" else Y_TOL) + (IO_ROUND[lc.IO_DTYPE[io]] if io != "f32" else 0.0)
    g = {"f16": F16_G_TOL, "f16x3g": X2_G_TOL}.get(math, G_TOL)
    return y, g, (2e-3 if math == "f16" else 1e-5)


def _nan_scratch(d, dev, state=False):
    """The stash and the shared workspace of dims d, every word NAN_WORD, the status block zeroed."""
    from windgnn_amd import _lib
    from windgnn_amd.functional import _Workspace
    lib = _lib.load()
    nst = (lib.wgnn_state_stash_bytes if state else lib.wgnn_stash_bytes)(C.byref(d))
    nws = lib.wgnn_workspace_bytes(C.byref(d))
    assert nst > 0 and nws > 0 and nst % 4 == 0 and nws % 4 == 0
    stash = torch.empty(nst, dtype=torch.uint8, device=dev)
    stash.view(torch.int32).fill_(NAN_WORD)
    ws = _Workspace.get(dev, nws)
    ws.view(torch.int32)[_lib.STATUS_BYTES // 4:].fill_(NAN_WORD)
    ws[:_lib.STATUS_BYTES].zero_()
    return stash, nst + ws.numel()


def _release():
    from windgnn_amd.functional import _Workspace
    _Workspace._bufs.clear()
    torch.cuda.empty_cache()


class _env:
    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.prev = os.environ.get(self.name)
        if self.value is not None:
            os.environ[self.name] = self.value

    def __exit__(self, *exc):
        if self.value is not None:
            if self.prev is None:
                del os.environ[self.name]
            else:
                os.environ[self.name] = self.prev


def _adjacency(c, dev):
    return lc.csr_of(c.id).to(dev) if c.csr_k else lc.base_draw(c.id).A.to(dev)


def _report(run, ey, eloss, worst):
    print("large-offset %s: Y %.2e, loss %.2e, grads %s" % (lc.run_id(run), ey, eloss, {k: "%.1e" % v for k, v in worst.items()}))


def _raw_step(run):
    """wgnn_fwd_loss, wgnn_bwd_mse_part(7 | 8 | DEFER), wgnn_finish(6) at the case's full batch."""
    from windgnn_amd import _lib
    from windgnn_amd.functional import (_forward_setup, _params_struct, _ptr, _stash_ptr, _stream, check_range_status,
                                        finish_step, gcn_gru_backward_mse_raw, prepared_weights)
    cid, math, io, route = run
    c, dev, lib = lc.STEP_BY_ID[cid], _dev(), _lib.load()
    draw, ref, dt = lc.base_draw(cid), lc.step_reference(cid, io), lc.IO_DTYPE[io]
    y_tol, g_tol, l_tol = _bars(math, io)
    A = _adjacency(c, dev)
    X = lc.periodic(draw.X.to(dt).to(dev), c.B)
    L = lc.periodic(draw.L.to(dt).to(dev), c.B)
    params = [draw.p[k].to(dev).contiguous() for k in PARAM_KEYS]
    with _env("WGNN_GHN_RECOMPUTE", "0" if route == "raw_ghn3" else None):
        stash, scratch_bytes = _nan_scratch(c.dims(math, io), dev)
        peak = (X.numel() * X.element_size() + 2 * L.numel() * L.element_size() + scratch_bytes) / GIB
        A_, d, ws, ws_bytes = _forward_setup(A, X, params, lc.MATH[math], labels=L)      # the workspace just filled
        img = prepared_weights(d, params, dev)
        Y = torch.full((c.B, c.T, c.H), float("nan"), dtype=dt, device=dev)
        ps = _params_struct(_lib.Params, params, img)
        rc = lib.wgnn_fwd_loss(C.byref(d), _ptr(A_), _ptr(X), C.byref(ps), _ptr(L), _ptr(Y), _stash_ptr(stash), _ptr(ws), ws_bytes,
                               _stream())
        _lib.check(rc, "wgnn_fwd_loss")
        grads = [torch.full_like(q, float("nan")) for q in params]
        loss = torch.full((), float("nan"), device=dev)
        gcn_gru_backward_mse_raw(d, A, X, params, Y, L, stash, grads, loss, 1.0, part=7 | 8 | _lib.BWD_DEFER, prepared=img)
        finish_step(d, params, grads, 6, None, img, dev)
    torch.cuda.synchronize()
    ey = lc.check_periodic(Y, ref["Y"], y_tol, lc.run_id(run))                                   # 1, 2, 3
    eloss = abs(float(loss) - ref["loss"])
    worst = {k: rel_to_max(gk.cpu(), ref["grads"][k]) for k, gk in zip(PARAM_KEYS, grads)}
    _report(run, ey, eloss, worst)
    print("large-offset %s: device memory of the operands and scratch %.1f GiB" % (lc.run_id(run), peak))
    assert eloss <= l_tol * max(1.0, ref["loss"]), (float(loss), ref["loss"])                    # 4
    assert max(worst.values()) <= g_tol, worst
    check_range_status(dev)                                                                      # 5
    del X, L, Y, stash, ws, grads, img
    _release()


def _trainstep(run):
    """TrainStep.step + check(): bench.py's own schedule.  The workspace is prefilled; the step's forward is handed a NaN-filled
    stash (gcn_gru_forward_raw's stash=, the one argument added to TrainStep's own call); Y is allocated inside that call: a block
    of its size is filled with NaN and freed just before it, and the test requires that Y came back at that address."""
    import windgnn_amd.trainer as trainer
    from windgnn_amd import GCN_GRU
    from windgnn_amd.trainer import TrainStep
    cid, math, io, route = run
    c, dev = lc.STEP_BY_ID[cid], _dev()
    draw, ref = lc.base_draw(cid), lc.step_reference(cid, io)
    y_tol, g_tol, l_tol = _bars(math, io)
    model = GCN_GRU(13, 13, 13, c.S * 13, c.H, math=math)
    model.load_state_dict({k: v.clone() for k, v in draw.p.items()})
    tr = TrainStep(model.to(dev), lr=1e-3)
    A = _adjacency(c, dev)
    X = lc.periodic(draw.X.to(dev), c.B)
    L = lc.periodic(draw.L.to(dev), c.B)
    stash, _ = _nan_scratch(c.dims(math, io), dev)
    forward_raw, y_ptr = trainer.gcn_gru_forward_raw, []

    def forward(*a, **k):                # Y is the next allocation of its size: the block freed here
        y_ptr.append(torch.full((c.B, c.T, c.H), float("nan"), device=dev).data_ptr())
        return forward_raw(*a, stash=stash, **k)
    try:
        trainer.gcn_gru_forward_raw = forward
        loss, Y = tr.step(A, X, L)
    finally:
        trainer.gcn_gru_forward_raw = forward_raw
    assert y_ptr == [Y.data_ptr()], "the NaN prefill did not reach the step's stash / Y"
    tr.check()                                                                                   # 5
    ey = lc.check_periodic(Y, ref["Y"], y_tol, lc.run_id(run))                                   # 1, 2, 3
    eloss = abs(float(loss) - ref["loss"])
    worst = {k: rel_to_max(gk.cpu(), ref["grads"][k]) for k, gk in zip(PARAM_KEYS, tr.g_views)}
    _report(run, ey, eloss, worst)
    assert eloss <= l_tol * max(1.0, ref["loss"]), (float(loss), ref["loss"])                    # 4
    assert max(worst.values()) <= g_tol, worst
    del X, L, Y, tr, model, stash
    _release()


def _state_step(run):
    """wgnn_fwd_state_stash + wgnn_bwd_state_part with h0, dh_n and dh0, against test_gpu_state_train's fp64 nn.GRU with hx:
    the gradients of sum(Y dY) + sum(h_n dh_n) add over windows (R times the period's plus those of its first r windows)."""
    from test_gpu_state_train import _fp64_model
    from windgnn_amd import _lib
    from windgnn_amd.functional import (_forward_setup, _params_struct, _ptr, _stash_ptr, _stream, check_range_status,
                                        gcn_gru_state_backward_raw)
    cid, math, io, route = run
    c, dev, lib = lc.STEP_BY_ID[cid], _dev(), _lib.load()
    draw = lc.base_draw(cid)
    y_tol, g_tol, _ = _bars(math, io)
    # fp64: the period, and its first r windows
    sums = []
    for n in (lc.P, c.r):
        leaves, f = _fp64_model(draw.p)
        h0r = draw.h0[:n].double().requires_grad_(True)
        Yr, hnr = f(draw.A, draw.X[:n], h0r)
        ((Yr * draw.dY[:n].double()).sum() + (hnr * draw.dhn[:n].double()).sum()).backward()
        sums.append((Yr.detach(), hnr.detach(), {k: leaves[k].grad for k in PARAM_KEYS}, h0r.grad))
    (YP, hnP, gP, dh0P), (_, _, gr, _) = sums
    gref = {k: c.R * gP[k] + gr[k] for k in PARAM_KEYS}
    A = _adjacency(c, dev)
    X = lc.periodic(draw.X.to(dev), c.B)
    h0, dY, dhn = (lc.periodic(t.to(dev), c.B) for t in (draw.h0, draw.dY, draw.dhn))
    params = [draw.p[k].to(dev).contiguous() for k in PARAM_KEYS]
    stash, _ = _nan_scratch(c.dims(math, io), dev, state=True)
    A_, d, ws, ws_bytes = _forward_setup(A, X, params, lc.MATH[math], h0=h0)              # the workspace just filled
    Y = torch.full((c.B, c.T, c.H), float("nan"), device=dev)
    hn = torch.full((c.B, c.H), float("nan"), device=dev)
    dh0 = torch.full((c.B, c.H), float("nan"), device=dev)
    ps = _params_struct(_lib.Params, params)
    rc = lib.wgnn_fwd_state_stash(C.byref(d), _ptr(A_), _ptr(X), C.byref(ps), _ptr(h0), _ptr(Y), _ptr(hn), _stash_ptr(stash),
                                  _ptr(ws), ws_bytes, _stream())
    _lib.check(rc, "wgnn_fwd_state_stash")
    grads = [torch.full_like(q, float("nan")) for q in params]
    gcn_gru_state_backward_raw(d, A, X, params, Y, dY, dhn, stash, grads, dh0)
    torch.cuda.synchronize()
    ey = lc.check_periodic(Y, YP, y_tol, lc.run_id(run) + " Y")
    eh = lc.check_periodic(hn, hnP, y_tol, lc.run_id(run) + " h_n")
    ed = lc.check_periodic(dh0, dh0P, g_tol * float(dh0P.abs().max()), lc.run_id(run) + " dh0")
    worst = {k: rel_to_max(gk.cpu(), gref[k]) for k, gk in zip(PARAM_KEYS, grads)}
    print("large-offset %s: Y %.2e, h_n %.2e, dh0 %.2e of max, grads %s"
          % (lc.run_id(run), ey, eh, ed / float(dh0P.abs().max()), {k: "%.1e" % v for k, v in worst.items()}))
    assert max(worst.values()) <= g_tol, worst
    check_range_status(dev)
    del X, Y, hn, dh0, h0, dY, dhn, stash, ws, grads
    _release()


@pytest.mark.parametrize("run", lc.STEP_RUNS, ids=[lc.run_id(r) for r in lc.STEP_RUNS])
def test_step_at_the_largest_accepted_batch(run):
    """One case and mode per test.  Peak device memory, comparisons included (measured by the module's fixture, which holds every
    test below 64 GiB): x4g 14.9 GiB (16-bit I/O 12.8), gi4g 21.9 (carried state 25.9), bench60k 16.3, wide 29.0 in f32 and 34.2 in
    f16x3, csr 40.0.  Observed errors: DESIGN.md section 2e."""
    {"raw": _raw_step, "raw_ghn3": _raw_step, "state": _state_step, "trainstep": _trainstep}[run[3]](run)


# ---- element-wise entries: closed-form fp64 references from a period of 48 values
def _period_values(seed):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(lc.P, generator=g, dtype=torch.float64)


def test_mse_loss_grad_past_2_32_bytes():
    """wgnn_mse_loss_grad on n = 2^31 + 4097 elements (Y, L and dY: 8 GiB each; peak 24.3 GiB): dY[i] = 2 (Y - L)[i mod 48] / n exactly
    as fp32 forms it (one subtraction, one product with the fp32 coefficient), every element; the loss against the fp64 mean."""
    from windgnn_amd.functional import mse_loss_grad
    dev, n = _dev(), lc.ELEMENTWISE["mse_loss_grad"]["n"]
    yP, lP = _period_values(1).float(), _period_values(2).float()
    Y, L = lc.periodic(yP.to(dev), n), lc.periodic(lP.to(dev), n)
    loss, dY = mse_loss_grad(Y, L)
    torch.cuda.synchronize()
    R, r = divmod(n, lc.P)
    dP = yP.double() - lP.double()
    want_loss = float((R * (dP * dP).sum() + (dP[:r] * dP[:r]).sum()) / n)
    coef = torch.tensor(2.0, dtype=torch.float32) / torch.tensor(float(n), dtype=torch.float32)    # 2.0f * scale / (float)n
    want = ((yP - lP) * coef).double()                                                             # fp32 arithmetic, exact
    e = lc.check_periodic(dY, want, 2.0 ** -24 * float(want.abs().max()), "mse_loss_grad dY")   # one fp32 rounding
    print("large-offset mse_loss_grad: dY %.1e, loss %.9f vs %.9f" % (e, float(loss), want_loss))
    assert abs(float(loss) - want_loss) <= 1e-5 * max(1.0, want_loss)
    del Y, L, dY
    _release()


def test_adam_step_past_2_32_bytes():
    """wgnn_adam_step on n = 2^31 + 169 elements (p, g, m, v: 8 GiB each; peak 32.3 GiB): one step from a mid-training state of period
    48 against fp64 Adam, every element; a second visit or a missed element is off by orders of magnitude more than the bar."""
    from windgnn_amd.functional import adam_step_
    dev, n = _dev(), lc.ELEMENTWISE["adam_step"]["n"]
    pP, gP = _period_values(3).float() - 0.5, (_period_values(4).float() - 0.5) * 1e-2
    mP, vP = (_period_values(5).float() - 0.5) * 1e-3, _period_values(6).float() * 1e-6
    p, g, m, v = (lc.periodic(t.to(dev), n) for t in (pP, gP, mP, vP))
    step, lr, b1, b2, eps = 3, 1e-3, 0.9, 0.999, 1e-8
    adam_step_(p, g, m, v, step, lr, b1, b2, eps)
    torch.cuda.synchronize()
    m64 = b1 * mP.double() + (1 - b1) * gP.double()
    v64 = b2 * vP.double() + (1 - b2) * gP.double() ** 2
    p64 = pP.double() - lr / (1 - b1 ** step) * (m64 / (v64.sqrt() / (1 - b2 ** step) ** 0.5 + eps))
    ep = lc.check_periodic(p, p64, 2e-7, "adam_step param")          # the suite's bar (test_finish_kernel_equals_...)
    em = lc.check_periodic(m, m64, 1e-6 * float(m64.abs().max()), "adam_step exp_avg")
    ev = lc.check_periodic(v, v64, 1e-6 * float(v64.abs().max()), "adam_step exp_avg_sq")
    assert lc.check_periodic(g, gP.double(), 0.0, "adam_step grad") == 0.0                        # the gradient is read only
    print("large-offset adam_step: p %.1e, m %.1e, v %.1e" % (ep, em, ev))
    del p, g, m, v
    _release()


def test_predict_last_past_2_32_bytes():
    """wgnn_predict_last on Y [1 400 021, 7, 127] (4.98e9 B; the header sets no limit on Y, out [B, H] stays below 2^31 elements):
    out[b] = Y[b mod 48, T - 1] * (wmax - wmin) + wmin as fp32 forms it, every row.  Peak 5.5 GiB."""
    from windgnn_amd import _lib
    from windgnn_amd.functional import _ptr, _stream
    dev, (B, T, H) = _dev(), (lc.PREDICT_LAST[k] for k in "BTH")
    assert B * T * H * 4 > lc.T32
    g = torch.Generator().manual_seed(11)
    YP = torch.rand(lc.P, T, H, generator=g)
    Y = lc.periodic(YP.to(dev), B)
    out = torch.full((B, H), float("nan"), device=dev)
    wmin, wmax = 0.25, 21.5
    _lib.check(_lib.load().wgnn_predict_last(_ptr(Y), B, T, H, wmin, wmax, _ptr(out), _stream()), "wgnn_predict_last")
    torch.cuda.synchronize()
    want = (YP[:, T - 1] * torch.tensor(wmax - wmin, dtype=torch.float32) + torch.tensor(wmin, dtype=torch.float32)).double()
    # y * range + wmin in fp32, fused or not: one or two roundings of a value below 32
    e = lc.check_periodic(out, want, 2 * 2.0 ** -24 * 32, "predict_last")
    print("large-offset predict_last: %.1e" % e)
    del Y, out
    _release()


def test_make_windows_past_2_32_bytes():
    """wgnn_make_windows: X [432 021, 3, 64, 13] (4.31e9 B) and L [B, 3, 192] gathered from a series of 48-row period: bit-exact
    copies, every element.  Peak 9.2 GiB (feat, X and L)."""
    from windgnn_amd import _lib
    from windgnn_amd.functional import _ptr, _stream
    dev = _dev()
    B, seq, S, Ttot = (lc.MAKE_WINDOWS[k] for k in ("B", "seq", "S", "Ttot"))
    assert B * seq * S * 13 * 4 > lc.T32 and lc.P % seq == 0
    g = torch.Generator().manual_seed(12)
    fP = torch.rand(lc.P, S, 13, generator=g)
    feat = lc.periodic(fP.to(dev), Ttot)                                  # feat[t] = fP[t mod 48]
    X = torch.full((B, seq, S, 13), float("nan"), device=dev)
    L = torch.full((B, seq, 3 * S), float("nan"), device=dev)
    rc = _lib.load().wgnn_make_windows(_ptr(feat), Ttot, S, 13, seq, 11, None, None, B, _ptr(X), _ptr(L), _stream())
    _lib.check(rc, "wgnn_make_windows")
    torch.cuda.synchronize()
    # window b starts at row b * seq: windows repeat every 48 / seq = 16, so they do every 48 as well
    wP = lc.P                                                             # the first 48 windows cover rows 0 .. 48 seq + 3
    f3 = torch.cat([fP] * (seq + 1))
    XP = torch.stack([f3[b * seq:(b + 1) * seq] for b in range(wP)])
    LP = torch.stack([torch.cat([f3[b * seq + k + 1:(b + 1) * seq + k + 1, :, 11] for k in range(3)], dim=1) for b in range(wP)])
    ex = lc.check_periodic(X, XP.double(), 0.0, "make_windows X")
    el = lc.check_periodic(L, LP.double(), 0.0, "make_windows L")
    print("large-offset make_windows: X %.1e L %.1e" % (ex, el))
    del feat, X, L
    _release()


def test_eval_accum_past_2_32_bytes():
    """wgnn_eval_accum on labels [1 400 021, 7, 127] (4.98e9 B), pred and abs_err [B, 127]: abs_err = (float)|truth - pred| per
    element against fp64, the five header rows against R times the period's sums plus the first r windows'.  Peak 6.2 GiB."""
    from windgnn_amd.evaluate import eval_accum, eval_buffer
    dev, (B, T, H) = _dev(), (lc.PREDICT_LAST[k] for k in "BTH")
    g = torch.Generator().manual_seed(13)
    LP = torch.rand(lc.P, T, H, generator=g) * 0.8 + 0.1                  # truth stays away from 0
    pP = (LP[:, T - 1] * 21.25 + 0.25) * (0.9 + 0.2 * torch.rand(lc.P, H, generator=g))      # within 10 % of the truth: a > 0
    labels, pred = lc.periodic(LP.to(dev), B), lc.periodic(pP.to(dev), B)
    abs_err = torch.full((B, H), float("nan"), device=dev)
    acc = eval_buffer(H, dev)
    wmin, wmax = 0.25, 21.5
    eval_accum(pred, labels, wmin, wmax, acc, abs_err)
    torch.cuda.synchronize()
    truth = LP[:, T - 1].double() * (float(torch.tensor(wmax)) - float(torch.tensor(wmin))) + float(torch.tensor(wmin))
    e = truth - pP.double()
    a = 1.0 - e.abs() / truth
    R, r = divmod(B, lc.P)
    ea = lc.check_periodic(abs_err, e.abs().float().double(), 0.0, "eval_accum abs_err")
    head = acc[:5 * H].view(5, H).cpu()
    worst = 0.0
    for k, v in enumerate((torch.ones_like(e), e * e, e.abs(), a, a * a)):
        want = R * v.sum(0) + v[:r].sum(0)
        worst = max(worst, float(((head[k] - want).abs() / want.abs()).max()))
    print("large-offset eval_accum: abs_err %.1e, header %.1e relative" % (ea, worst))
    assert worst <= B * 2.0 ** -52, worst                                 # fp64 sums of B terms of one sign (a: nearly)
    del labels, pred, abs_err, acc
    _release()


# ---- GraphConvLayer
LAYER_SUM_TOL = G_TOL       # dW and db: sums over millions of rows, the suite's gradient bar


def _layer_call(c, A, X, W, b, dout, want_dx, dev):
    from windgnn_amd import _lib
    from windgnn_amd.functional import _ptr, _scratch, _stream
    lib = _lib.load()
    out = torch.full((c.nt, c.S, c.Fo), float("nan"), device=dev)
    dW, db = torch.full_like(W, float("nan")), torch.full_like(b, float("nan"))
    dX = torch.full((c.nt, c.S, c.Fi), float("nan"), device=dev) if want_dx else None
    if c.csr_k:
        blob, nnz = A.blob, A.nnz
        _lib.check(lib.wgnn_gcn_layer_csr_fwd(c.nt, c.S, c.Fi, nnz, _ptr(blob), _ptr(X), _ptr(W), _ptr(b), _ptr(out), _stream()),
                   "wgnn_gcn_layer_csr_fwd")
        nbytes = lib.wgnn_gcn_layer_csr_workspace_bytes(c.nt, c.S, c.Fi)
    else:
        _lib.check(lib.wgnn_gcn_layer_fwd(c.nt, c.S, c.Fi, c.Fo, _ptr(A), _ptr(X), _ptr(W), _ptr(b), _ptr(out), _stream()),
                   "wgnn_gcn_layer_fwd")
        nbytes = lib.wgnn_gcn_layer_workspace_bytes(c.nt, c.S, c.Fi, c.Fo)
    assert nbytes > 0
    wsp, wsn = _scratch(dev, nbytes)
    torch.cuda.synchronize()
    from windgnn_amd.functional import _Workspace
    ws = _Workspace.get(dev, nbytes + _lib.STATUS_BYTES)
    ws.view(torch.int32)[_lib.STATUS_BYTES // 4:].fill_(NAN_WORD)
    if c.csr_k:
        rc = lib.wgnn_gcn_layer_csr_bwd(c.nt, c.S, c.Fi, nnz, _ptr(blob), _ptr(X), _ptr(W), _ptr(out), _ptr(dout), _ptr(dW), _ptr(db),
                                        _ptr(dX), wsp, nbytes, _stream())
    else:
        rc = lib.wgnn_gcn_layer_bwd(c.nt, c.S, c.Fi, c.Fo, _ptr(A), _ptr(X), _ptr(W), _ptr(out), _ptr(dout), _ptr(dW), _ptr(db),
                                    _ptr(dX), wsp, nbytes, _stream())
    _lib.check(rc, "wgnn_gcn_layer_bwd")
    torch.cuda.synchronize()
    return out, dW, db, dX


@pytest.mark.parametrize("cid", [c.id for c in lc.LAYERS])
def test_graph_conv_layer_past_2_32_bytes(cid):
    """One GraphConvLayer over ntiles tiles of period 48, forward and backward, with and without dX, against fp64 autograd on the
    period: out and dX on every tile (NaN prefill, period bit for bit, LAYER_TOL), dW and db at the suite's 1e-4 (sums over
    millions of rows).  Peak device memory, comparisons included: l_13_200 12.8 GiB, l_200_13 12.5, l_64_64 31.7, l_13_13 23.5,
    l_csr 40.0."""
    c, dev = lc.LAYER_BY_ID[cid], _dev()
    d, ref = lc.layer_draw(cid), lc.layer_reference(cid)
    A = lc.layer_csr(cid).to(dev) if c.csr_k else d.A.to(dev)
    X, dout = lc.periodic(d.X.to(dev), c.nt), lc.periodic(d.dout.to(dev), c.nt)
    W, b = d.W.to(dev).contiguous(), d.b.to(dev).contiguous()
    first = None
    for want_dx in (False, True):
        out, dW, db, dX = _layer_call(c, A, X, W, b, dout, want_dx, dev)
        e = {"out": lc.check_periodic(out, ref["out"], LAYER_TOL, cid + " out"),
             "dW": rel_to_max(dW.cpu(), ref["dW"]), "db": rel_to_max(db.cpu(), ref["db"])}
        if want_dx:
            scale = float(ref["dX"].abs().max())
            e["dX"] = lc.check_periodic(dX, ref["dX"], LAYER_TOL * scale, cid + " dX") / scale
            assert torch.equal(dW, first[0]) and torch.equal(db, first[1])      # the same sums with and without dX
        print("large-offset layer %s (dX %s): %s" % (cid, want_dx, " ".join("%s=%.2e" % kv for kv in e.items())))
        assert e["dW"] <= LAYER_SUM_TOL and e["db"] <= LAYER_SUM_TOL, e
        first = (dW, db)
        del out, dX
    del X, dout
    _release()


# ---- series mode (exact fp32)
def _series_scratch(sd, dev, table=False, *more_bytes):
    """The series workspace of dims sd filled with NAN_WORD (both status blocks zeroed), and blocks of the sizes the raw calls
    are about to allocate (stash, then Y) filled with NaN and freed: the caching allocator hands the same blocks back, and the
    callers require it (the addresses are the third result)."""
    from windgnn_amd import _lib
    from windgnn_amd.functional import _Workspace
    lib = _lib.load()
    q = "at_" if table else ""
    nws = max(getattr(lib, "wgnn_series_%sworkspace_bytes" % q)(C.byref(sd)), lib.wgnn_series_val_workspace_bytes(C.byref(sd)))
    off = getattr(lib, "wgnn_series_%sstatus_offset" % q)(C.byref(sd))
    assert nws > 0 and nws % 4 == 0
    ws = _Workspace.get(dev, nws)
    ws.view(torch.int32).fill_(NAN_WORD)
    ws[:_lib.STATUS_BYTES].zero_()
    ws[off:off + _lib.STATUS_BYTES].zero_()
    blocks = []                          # held together, freed together: none is carved out of another
    for n in (getattr(lib, "wgnn_series_%sstash_bytes" % q)(C.byref(sd)),) + more_bytes:
        blocks.append(torch.empty(n, dtype=torch.uint8, device=dev))
        blocks[-1].view(torch.int32).fill_(NAN_WORD)
    ptrs = [t.data_ptr() for t in blocks]
    del blocks
    return ws, off, ptrs


def _series_status_clean(ws, off):
    assert int(ws[:4].view(torch.int32).item()) == 0 and int(ws[off:off + 4].view(torch.int32).item()) == 0


def _series_inputs(c, dev):
    d = lc.series_draw(c.id)
    Xs = lc.periodic(d.Xs.to(dev), c.rows, lc.Q)
    Ls = lc.periodic(d.Ls.to(dev), c.rows, lc.Q)
    return d, d.A.to(dev), Xs, Ls, [d.p[k].to(dev).contiguous() for k in PARAM_KEYS]


@pytest.mark.parametrize("cid", [c.id for c in lc.SERIES])
def test_series_strided_past_2_32_bytes(cid):
    """wgnn_series_fwd then wgnn_series_bwd on a series of period 45: series_gi (4 000 000 hours, stride 4, n = 1 000 000: GI_s is
    5.72 GiB; peak 26.3 GiB) and series_x (1 296 063 hours of 64 stations, stride 3, n = 432 021: Xs and g_s past 2^32
    bytes; peak 15.4 GiB).  Y on every window against the oracle's at most 45 distinct windows (NaN prefill, period in w bit for bit,
    Y_TOL); the 8 gradients of sum(Y dY) by phase counts at G_TOL."""
    from windgnn_amd.functional import check_range_status
    from windgnn_amd.series import series_backward_raw, series_forward_raw
    c, dev = lc.SERIES_BY_ID[cid], _dev()
    d, A, Xs, Ls, params = _series_inputs(c, dev)
    w = lc.series_windows(cid)
    order = (torch.arange(c.period) * c.stride) % lc.Q                    # window k starts at phase (k stride) mod 45
    ws, off, ptrs = _series_scratch(c.sdims(), dev, False, c.n * c.T * c.H * 4)
    Y, stash, sd = series_forward_raw(A, Xs, c.T, c.stride, params, n_windows=c.n)
    assert [stash.data_ptr(), Y.data_ptr()] == ptrs, "the NaN prefill did not reach the call's stash / Y"
    torch.cuda.synchronize()
    ey = lc.check_periodic(Y, w["Y"][order], Y_TOL, cid + " Y", P=c.period)
    dY = lc.periodic(d.dY[order].to(dev), c.n, c.period)
    grads = [torch.full_like(q, float("nan")) for q in params]
    series_backward_raw(sd, A, Xs, params, Y, dY, stash, grads)
    torch.cuda.synchronize()
    _, gref = lc.series_grads(cid, (torch.arange(c.n) * c.stride) % lc.Q, mse=False)
    worst = {k: rel_to_max(gk.cpu(), gref[k]) for k, gk in zip(PARAM_KEYS, grads)}
    print("large-offset %s strided: Y %.2e, grads %s" % (cid, ey, {k: "%.1e" % v for k, v in worst.items()}))
    assert max(worst.values()) <= G_TOL, worst
    _series_status_clean(ws, off)
    check_range_status(dev)
    del Xs, Ls, Y, dY, stash, ws
    _release()


def test_series_table_of_starts_past_2_32_bytes():
    """series_gi with a sorted table of 100 021 starts -- row 0, the rows either side of the 2^31- and 2^32-byte crossings of
    GI_s, rows - T and a fixed draw in between: wgnn_series_fwd_loss_at then wgnn_series_bwd_mse_at (Y of every window against the
    oracle's window of its phase, windows of one phase equal bit for bit, the loss and the 8 gradients by phase counts), then
    wgnn_series_val on the same table (its loss has the training pair's bits, `last` is Y[:, -1]).  Peak 17.4 GiB."""
    from windgnn_amd.functional import check_range_status
    from windgnn_amd.series import series_backward_mse_raw, series_forward_loss_raw, series_val_raw
    c, dev = lc.SERIES_BY_ID["series_gi"], _dev()
    d, A, Xs, Ls, params = _series_inputs(c, dev)
    w = lc.series_windows(c.id)
    starts = c.table()
    assert set(c.crossing_rows() + [0, c.rows - c.T]) <= set(starts.tolist()) and len(c.crossing_rows()) == 6
    phase = (starts.long() % lc.Q)
    ws, off, ptrs = _series_scratch(c.sdims(True), dev, True, c.n_table * c.T * c.H * 4)
    Y, stash, loss_buf, sd, table = series_forward_loss_raw(A, Xs, Ls, c.T, None, params, starts=starts)
    assert [stash.data_ptr(), Y.data_ptr()] == ptrs, "the NaN prefill did not reach the call's stash / Y"
    torch.cuda.synchronize()
    assert not bool(torch.isnan(Y).any()), "check 1 (NaN prefill)"
    first = torch.full((lc.Q,), -1, dtype=torch.int64)
    for i in range(len(phase) - 1, -1, -1):
        first[phase[i]] = i
    assert int(first.min()) >= 0
    assert torch.equal(Y, Y[first[phase].to(dev)]), "check 3: windows of one phase differ bit for bit"
    ey = float((Y.double() - w["Y"].to(dev)[phase.to(dev)]).abs().max())
    assert ey <= Y_TOL, ey
    grads = [torch.full_like(q, float("nan")) for q in params]
    loss = torch.full((), float("nan"), device=dev)
    series_backward_mse_raw(sd, A, Xs, params, Y, Ls, stash, loss_buf, grads, loss, starts=table)
    torch.cuda.synchronize()
    lref, gref = lc.series_grads(c.id, phase, mse=True)
    worst = {k: rel_to_max(gk.cpu(), gref[k]) for k, gk in zip(PARAM_KEYS, grads)}
    print("large-offset series_gi table: Y %.2e, loss %.2e, grads %s" % (ey, abs(float(loss) - lref), {k: "%.1e" % v for k, v in worst.items()}))
    assert abs(float(loss) - lref) <= 1e-5 * max(1.0, lref), (float(loss), lref)
    assert max(worst.values()) <= G_TOL, worst
    _series_status_clean(ws, off)
    last = torch.full((c.n_table, c.H), float("nan"), device=dev)
    vloss = torch.full((1,), float("nan"), device=dev)
    series_val_raw(A, Xs, params, Ls, c.T, starts=starts, last=last, out_loss=vloss)      # (its workspace has a layout of its own)
    torch.cuda.synchronize()
    assert torch.equal(last, Y[:, -1]) and float(vloss) == float(loss), (float(vloss), float(loss))
    check_range_status(dev)
    del Xs, Ls, Y, stash, ws, last
    _release()


def test_predict_last_at_its_largest_output():
    """wgnn_predict_last with out [16 909 320, 127] = 2^31 - 8 elements, inside the last 255 below its limit, where a block count
    formed in 32 bits wraps (the launch then failed: WGNN_ERR_HIP); T = 1, so Y has out's size: every element, as above.  Peak 16.3 GiB."""
    from windgnn_amd import _lib
    from windgnn_amd.functional import _ptr, _stream
    dev, (B, T, H) = _dev(), (lc.PREDICT_LAST_EDGE[k] for k in "BTH")
    assert lc.T31 - 256 < B * H < lc.T31
    g = torch.Generator().manual_seed(14)
    YP = torch.rand(lc.P, T, H, generator=g)
    Y = lc.periodic(YP.to(dev), B)
    out = torch.full((B, H), float("nan"), device=dev)
    wmin, wmax = 0.25, 21.5
    _lib.check(_lib.load().wgnn_predict_last(_ptr(Y), B, T, H, wmin, wmax, _ptr(out), _stream()), "wgnn_predict_last")
    torch.cuda.synchronize()
    want = (YP[:, T - 1] * torch.tensor(wmax - wmin, dtype=torch.float32) + torch.tensor(wmin, dtype=torch.float32)).double()
    e = lc.check_periodic(out, want, 2 * 2.0 ** -24 * 32, "predict_last, largest output")
    print("large-offset predict_last at 2^31 - 8 elements: %.1e" % e)
    del Y, out
    _release()
