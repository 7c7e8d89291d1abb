"""GraphConvLayer wider than 64 features on the GPU (csrc/gcn_wide.hip): parity on lattice inputs against fp64 autograd, bitwise
repeats, the footprint and the dirty-workspace contract through the C ABI, a side stream, and GCN_GRU(13, hid, 13, ...) with
hid > 64 against the fp64 oracle.  tests/test_layer_wide_host.py qualifies the inputs on the CPU.

Observed on an MI355X (worst over tests/layer_wide_cases.py's TABLE, with and without dX): out 0.0 on every row; relative to
the tensor's maximum dX 5.2e-7, dW 2.6e-7, db 2.1e-7 (bar 1e-4).  The model shapes: Y 1.2e-7, loss 2.5e-8, gradients 2.2e-7."""
import ctypes as C

import pytest
import torch

import lattice_inputs as li
import layer_wide_cases as lw
from conftest import PARAM_KEYS, max_abs, rel_to_max
from guarded import FILLS, Arena
from test_gpu_parity import G_TOL, Y_TOL

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


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


def _layer_step(d, Fi, Fo, want_dx, dev):
    """One forward + backward through GraphConvLayer: (out, dX or None, dW, db) on the device."""
    from windgnn_amd import GraphConvLayer
    layer = GraphConvLayer(Fi, Fo)
    layer.load_state_dict({"weight": d.W, "bias": d.b})
    layer = layer.to(dev)
    X = d.X.to(dev).requires_grad_(want_dx)
    out = layer(d.A.to(dev), X)
    out.backward(d.dout.to(dev))
    return out.detach(), X.grad, layer.weight.grad, layer.bias.grad


@pytest.mark.parametrize("want_dx", [True, False], ids=["dX", "no_dX"])
@pytest.mark.parametrize("row", lw.TABLE, ids=lw.IDS)
def test_wide_layer_parity_and_repeat(row, want_dx):
    """out is held to equality (every partial sum of the forward is a dyadic number of fewer than 24 bits), the gradients of the
    signed random dout to the suite's bar; a second run gives the same bits in every output."""
    S, Fi, Fo, nt = row
    dev = _dev()
    d, out_r, dX_r, dW_r, db_r = lw.layer_reference(*row)
    got, prof = _profiled(lambda: _layer_step(d, Fi, Fo, want_dx, dev))
    out, dX, dW, db = got
    err = {"out": max_abs(out.cpu(), out_r), "dW": rel_to_max(dW.cpu(), dW_r), "db": rel_to_max(db.cpu(), db_r)}
    if want_dx:
        err["dX"] = rel_to_max(dX.cpu(), dX_r)
    print("wide layer S%d %d -> %d x%d%s: %s" % (S, Fi, Fo, nt, "" if want_dx else " (no dX)",
                                                " ".join("%s=%.2e" % kv for kv in err.items())))
    fwd = lw.FWD_KERNELS[Fo <= lw.TB]
    assert set(lw.wide_kernels(Fo)) <= set(prof) and not any(k.startswith("gcn_any") for k in prof), prof
    assert lw.FWD_KERNELS[Fo > lw.TB] not in prof, prof
    assert prof[fwd] == 1 and prof["gcn_wide_bwd_agg_kernel"] == 1 and prof["gcn_wide_sum_kernel"] == 2, prof
    assert (dX is None) == (not want_dx)
    assert err["out"] == 0.0, err
    for what in ("dX", "dW", "db"):
        assert err.get(what, 0.0) <= G_TOL, (what, err)
    again = _layer_step(d, Fi, Fo, want_dx, dev)
    for name, a, b in zip(("out", "dX", "dW", "db"), got, again):
        assert (a is None and b is None) or torch.equal(a, b), name


def test_the_route_changes_between_64_and_65_features():
    """64 -> 64 stays on gcn_any.hip, no new kernel runs; one feature more on either side is gcn_wide.hip's."""
    dev = _dev()
    d = li.draw_layer(3, 64, 64, 5)
    _, prof = _profiled(lambda: _layer_step(d, 64, 64, True, dev))
    assert set(li.LAYER_KERNELS) <= set(prof) and not any(k.startswith("gcn_wide") for k in prof), prof
    for Fi, Fo in ((64, 65), (65, 64)):
        d = li.draw_layer(3, Fi, Fo, 5)
        _, prof = _profiled(lambda: _layer_step(d, Fi, Fo, True, dev))
        assert set(lw.wide_kernels(Fo)) <= set(prof) and not any(k.startswith("gcn_any") for k in prof), (Fi, Fo, prof)


def _abi_run(fill, row, want_dx, stream=None):
    """wgnn_gcn_layer_fwd / _bwd inside a guarded arena: the output bytes, after the guard and poison checks."""
    from windgnn_amd import _lib
    lib = _lib.load()
    S, Fi, Fo, nt = row
    d = lw.layer_reference(*row)[0]
    wsb = lib.wgnn_gcn_layer_workspace_bytes(nt, S, Fi, Fo)
    assert wsb == 4 * lw.workspace_floats(nt, S, Fi, Fo) and wsb % 256 == 0
    a = Arena(_dev(), fill)
    for name, t in (("A", d.A), ("X", d.X), ("W", d.W), ("b", d.b), ("dout", d.dout)):
        a.buf(name, t.numel() * 4, data=t)
    a.buf("out", nt * S * Fo * 4)
    a.buf("dW", Fi * Fo * 4)
    a.buf("db", Fo * 4)
    a.buf("dX", nt * S * Fi * 4)
    a.buf("ws", wsb)
    a.commit()
    P = lambda n: C.c_void_p(a[n].ptr) if n else C.c_void_p(0)     # noqa: E731
    st = C.c_void_p(stream or 0)
    rc = lib.wgnn_gcn_layer_fwd(nt, S, Fi, Fo, P("A"), P("X"), P("W"), P("b"), P("out"), st)
    assert rc == 0, rc
    rc = lib.wgnn_gcn_layer_bwd(nt, S, Fi, Fo, P("A"), P("X"), P("W"), P("out"), P("dout"), P("dW"), P("db"),
                                P("dX" if want_dx else None), P("ws"), C.c_size_t(wsb), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert a.check() == {}, (fill, a.check())
    names = ["out", "dW", "db"] + (["dX"] if want_dx else [])
    res = {n: a[n].host() for n in names}
    if fill != "zero":
        for n in names:
            assert a[n].unwritten(4) == 0, (fill, n)
        if not want_dx:
            assert a["dX"].unwritten(4) == nt * S * Fi                     # not an argument: still the fill
    return res


@pytest.mark.parametrize("want_dx", [True, False], ids=["dX", "no_dX"])
@pytest.mark.parametrize("row", lw.FOOTPRINT_ROWS, ids=[lw.IDS[lw.TABLE.index(r)] for r in lw.FOOTPRINT_ROWS])
def test_wide_layer_footprint_and_dirty_workspace(row, want_dx):
    S, Fi, Fo, nt = row
    _, out_r, dX_r, dW_r, db_r = lw.layer_reference(*row)
    base = None
    for fill in FILLS:
        res = _abi_run(fill, row, want_dx)
        if base is None:
            base = res
            assert max_abs(res["out"].view(torch.float32).reshape(out_r.shape), out_r) == 0.0
            assert rel_to_max(res["dW"].view(torch.float32).reshape(dW_r.shape), dW_r) <= G_TOL
            assert rel_to_max(res["db"].view(torch.float32), db_r) <= G_TOL
            if want_dx:
                assert rel_to_max(res["dX"].view(torch.float32).reshape(dX_r.shape), dX_r) <= G_TOL
            continue
        for n in base:
            assert torch.equal(base[n], res[n]), "%s under the %s fill differs from the zero-fill run" % (n, fill)


def test_wide_layer_on_a_side_stream():
    """Inputs produced on the side stream, the layer run under it: the default stream's bits."""
    from windgnn_amd import GraphConvLayer
    row = lw.TABLE[4]
    S, Fi, Fo, nt = row
    dev = _dev()
    d = lw.layer_reference(*row)[0]
    base = _layer_step(d, Fi, Fo, True, dev)
    torch.cuda.synchronize()
    host = [t.pin_memory() for t in (d.A, d.X, d.W, d.b, d.dout)]
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        A, X, W, b, dout = (t.to(dev, non_blocking=True) * 1.0 for t in host)
        layer = GraphConvLayer(Fi, Fo).to(dev)
        with torch.no_grad():
            layer.weight.copy_(W)
            layer.bias.copy_(b)
        X.requires_grad_(True)
        out = layer(A, X)
        out.backward(dout)
        got = (out.detach(), X.grad, layer.weight.grad, layer.bias.grad)
    s.synchronize()
    torch.cuda.synchronize()
    for name, x, y in zip(("out", "dX", "dW", "db"), base, got):
        assert torch.equal(x, y), name


@pytest.mark.parametrize("shape", lw.MODEL_SHAPES, ids=lw.MODEL_IDS)
def test_wide_gcn_gru_against_the_fp64_oracle(shape):
    from windgnn_amd import GCN_GRU
    S, hid, T, B, H = shape
    dev = _dev()
    d, Y_r, loss_r, g_r = lw.model_reference(*shape)
    model = GCN_GRU(13, hid, 13, S * 13, H)
    assert tuple(model.state_dict().keys()) == tuple(PARAM_KEYS)
    model.load_state_dict(d.p)
    model = model.to(dev)

    def run():
        Y = model(d.A.to(dev), d.X.to(dev))
        loss = ((Y - d.L.to(dev)) ** 2).mean()
        loss.backward()
        return Y.detach(), loss.detach()

    (Y, loss), prof = _profiled(run)
    assert prof["gcn_wide_fwd_kernel"] == 1 and prof["gcn_wide_fwd_thin_kernel"] == 1 and prof["gcn_wide_bwd_agg_kernel"] == 2, prof
    got = dict(zip(PARAM_KEYS, (p.grad.cpu() for p in model.hot_path_parameters())))
    err = {"Y": max_abs(Y.cpu().reshape(Y_r.shape), Y_r), "loss": abs(float(loss) - loss_r)}
    err.update({k: rel_to_max(got[k], g_r[k]) for k in PARAM_KEYS})
    print("wide GCN_GRU S%d hid%d T%d B%d H%d: %s" % (shape + (" ".join("%s=%.2e" % kv for kv in err.items()),)))
    assert err["Y"] <= Y_TOL and err["loss"] <= 1e-5, err
    for k in PARAM_KEYS:
        assert err[k] <= G_TOL, (k, err)


def test_what_the_wide_widths_still_refuse():
    from windgnn_amd import GCN_GRU, GraphConvLayer
    from windgnn_amd.graph import CsrAdjacency
    from windgnn_amd.trainer import TrainStep
    dev = _dev()
    S, hid, T, B, H = lw.MODEL_SHAPES[3]
    d = lw.model_draw(S, hid, T, B, H)
    with pytest.raises(RuntimeError, match="exact fp32 only"):
        GCN_GRU(13, hid, 13, S * 13, H, math="f16x3")
    with pytest.raises(RuntimeError, match="output_dim must be 13"):
        GCN_GRU(13, hid, hid, S * 13, H)
    model = GCN_GRU(13, hid, 13, S * 13, H).to(dev)
    assert tuple(model(d.A.to(dev), d.X.to(dev)).shape) == (B, T, H)          # the widths themselves run ...
    with pytest.raises(RuntimeError, match="TrainStep drives the fused hot path"):              # ... what they refuse stays refused
        TrainStep(model)
    with pytest.raises(RuntimeError, match="13 / 13 widths"):
        model.forward_series(d.A.to(dev), d.X[0].to(dev), 2)
    with torch.no_grad(), pytest.raises(RuntimeError, match="13 / 13 widths"):
        model.forward_state(d.A.to(dev), d.X.to(dev))
    with pytest.raises(RuntimeError, match="13 / 13 widths"):
        model.forward_with_state(d.A.to(dev), d.X.to(dev))
    csr = CsrAdjacency.from_dense(d.A).to(dev)
    with pytest.raises(RuntimeError, match="13 -> 13"):
        GraphConvLayer(13, hid).to(dev)(csr, d.X.to(dev))
    # S > 64 over a dense adjacency stays refused at every width
    wide = GraphConvLayer(13, hid).to(dev)
    with pytest.raises(RuntimeError, match="wgnn_gcn_layer_fwd"):
        wide(torch.eye(65, device=dev), torch.zeros(2, 65, 13, device=dev))
