"""Parity on the lattice inputs of tests/lattice_inputs.py, on the MI355X: live ReLU masks that differ between stations, non-zero
conv biases and an asymmetric adjacency reach every GCN-side kernel family -- gcnx, gcn32 (12 and 16 waves), gcngi, the CSR
layers (the first test in which A != A^T reaches them), gcn_any, gru_step, the series front end and the carried-state entry
points.  A case runs one step under the library's profiler, asserts by name that the kernel it is there for was launched
(instance_cases.plan() for the dense routes, the literal names elsewhere) and holds Y, the loss and the 8 gradients (h_n / dh0, or
the last rows, where the route has them) to the fp64 reference at the suites' own bars, all imported.  Because every
pre-activation is an exact dyadic number, a miss is no tie (tests/test_lattice_inputs_host.py clears the inputs on the reference).
The observed errors are printed per case."""
import functools
import re

import pytest
import torch

import instance_cases as ic
import lattice_inputs as li
from conftest import PARAM_KEYS, max_abs, rel_to_max
from test_gpu_instances import IODT, _bounds, _option, _profiled
from test_gpu_parity import G_TOL, Y_TOL
from test_gpu_series import TOL as SERIES_TOL
from test_gpu_series import WIND_MAX, WIND_MIN
from test_gpu_series_instances import TABLED, windows
from test_gpu_series_train import TOL as LOSS_TOL
from test_gpu_state import _profiled as _profiled_counts
from test_gpu_state_train import MATH, _fp64_model, _tols

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _base(name):
    return re.match(r"[a-z0-9_]+", name).group(0)


@functools.lru_cache(maxsize=3)
def _reference(S, T, B, H, sparse, shift, io, state, seed=0):
    """The lattice draw of a shape (labels rounded to the I/O type; X is exact in it) and the fp64 reference's step on it."""
    from oracle import windgnn_oracle as orc
    d = li.draw(S, T, B, H, sparse, shift, seed) if seed else li.draw(S, T, B, H, sparse, shift)
    X, L = d.X.to(IODT[io]), d.L.to(IODT[io])
    assert torch.equal(X.float(), d.X)
    if not state:
        Yo, loss_o, go = orc.train_step(d.A.double(), X.double(), L.double(), {k: v.double() for k, v in d.p.items()})
        return dict(A=d.A, X=X, L=L, p=d.p, Y=Yo, loss=float(loss_o), grads=go)
    leaves, f = _fp64_model(d.p)
    h0r = d.h0.double().requires_grad_(True)
    Yr, hnr = f(d.A, X.float(), h0r)
    ((Yr * d.dY.double()).sum() + (hnr * d.dhn.double()).sum()).backward()
    return dict(A=d.A, X=X, p=d.p, h0=d.h0, dY=d.dY, dhn=d.dhn, Y=Yr.detach(), hn=hnr.detach(),
                grads={k: leaves[k].grad for k in PARAM_KEYS}, dh0=h0r.grad)


def _bars(cid, S, T, B, H, math, io, state, route):
    """test_gpu_instances' bars; f16x3g from 4096 rows: _tols' single-plane bar; one-pass fp16: the larger of the imported bar
    and twice the reference figure of lattice_inputs.F16_FIGURES."""
    b = dict(_bounds(S, T, B, H, math, io, state, route))
    if math == "f16x3g" and B * T >= 4096:
        g_tol = _tols("f16x3g_big", math, IODT[io])[1]
        b.update({k: g_tol for k in PARAM_KEYS}, dh0=g_tol)
    if math == "f16":
        fy, fl, fg = li.F16_FIGURES[cid]
        b.update({k: max(b[k], 2 * fg) for k in PARAM_KEYS}, Y=max(b["Y"], 2 * fy), loss=max(b["loss"], 2 * fl))
    return b


def _step(S, T, B, H, math, io, state, route, sparse, shift, seed=0):
    """One step of this call form on the GPU: the names it launched and its errors against the reference (seed: the draw's, for
    tests/test_gpu_gcn_loops.py's tabled shapes)."""
    from windgnn_amd import _lib
    from windgnn_amd.functional import (check_range_status, gcn_gru_backward_mse_raw, gcn_gru_forward_raw,
                                        gcn_gru_state_backward_raw, gcn_gru_state_forward_raw)
    from windgnn_amd.graph import CsrAdjacency
    dev = _dev()
    r = _reference(S, T, B, H, sparse, shift, io, state, seed) if seed else _reference(S, T, B, H, sparse, shift, io, state)
    A = CsrAdjacency.from_dense(r["A"]).to(dev) if sparse else r["A"].to(dev)
    X = r["X"].to(dev)
    ps = [r["p"][k].to(dev).contiguous() for k in PARAM_KEYS]
    mode = MATH[math]

    def run():
        gs = [torch.full_like(q, 7.0) for q in ps]
        if route == "infer":
            Y, _, _ = gcn_gru_forward_raw(A, X, ps, mode, want_stash=False)
            return dict(Y=Y)
        if state:
            dh0 = torch.full((B, H), 7.0, device=dev)
            Y, hn, stash, d = gcn_gru_state_forward_raw(A, X, ps, mode, r["h0"].to(dev))
            gcn_gru_state_backward_raw(d, A, X, ps, Y, r["dY"].to(dev), r["dhn"].to(dev), stash, gs, dh0)
            return dict(Y=Y, hn=hn, grads=gs, dh0=dh0)
        L = r["L"].to(dev)
        loss = torch.zeros((), device=dev)
        Y, stash, d = gcn_gru_forward_raw(A, X, ps, mode, labels=L)
        gcn_gru_backward_mse_raw(d, A, X, ps, Y, L, stash, gs, loss, 1.0, part=7 | 8)
        return dict(Y=Y, loss=loss, grads=gs)

    if route == "fused":
        with _option(_lib.OPT_FUSED_FWD, 2):
            out, names = _profiled(run)
    else:
        out, names = _profiled(run)
    check_range_status(dev)
    err = {"Y": max_abs(out["Y"].float().cpu().reshape(r["Y"].shape), r["Y"])}
    if "loss" in out:
        err["loss"] = abs(float(out["loss"]) - r["loss"]) / max(1.0, r["loss"])
    if "hn" in out:
        err["hn"] = max_abs(out["hn"].cpu(), r["hn"])
        err["dh0"] = rel_to_max(out["dh0"].cpu(), r["dh0"])
    for k, gk in zip(PARAM_KEYS, out.get("grads", [])):
        err[k] = rel_to_max(gk.cpu(), r["grads"][k])
    return names, err


@pytest.mark.parametrize("case", li.CASES, ids=[c[0] for c in li.CASES])
def test_lattice_step(case):
    cid, keys, S, T, B, H, math, io, state, route, sparse, shift = case
    names, err = _step(S, T, B, H, math, io, state, route, sparse, shift)
    print("%s S%d T%d B%d H%d %s %s state=%d %s: %s" % (cid, S, T, B, H, math, io, state, route,
                                                       " ".join("%s=%.2e" % kv for kv in err.items())))
    if sparse:
        assert set(keys) <= set(names), (cid, keys, names)
    else:
        expected = ic.plan(S, T, B, H, math, io, state, route)
        ran = sorted({n for n in names if _base(n) in TABLED})
        for key in keys:
            assert key in expected and ic.name_of(key) in ran, (cid, key, ran)
        assert ran == sorted({ic.name_of(k) for k in expected}), (cid, ran, expected)
    for what, e in err.items():
        bound = _bars(cid, S, T, B, H, math, io, state, route)[what]
        assert e <= bound, (cid, what, e, bound)


def test_csr_backward_reads_the_transposed_half_of_the_blob():
    """The control of the CSR cases: the same step with the A^T half of the blob overwritten by A's own rowptr | col | val (a
    valid CSR of the same size) must MISS the reference on the conv1 gradients by more than 100 bars -- dH1 = A^T dP2 is the
    only reader of that half -- while Y and the GRU gradients, which never see it, stay inside theirs.  With a symmetric
    adjacency the two blobs are the same words, which is why no earlier CSR test could tell."""
    from windgnn_amd.functional import gcn_gru_backward_mse_raw, gcn_gru_forward_raw
    from windgnn_amd.graph import CsrAdjacency
    S, T, B, H, shift = li.CSR_SHAPES[0]
    dev = _dev()
    r = _reference(S, T, B, H, True, shift, "f32", False)
    csr = CsrAdjacency.from_dense(r["A"])
    half = S + 1 + 2 * csr.nnz
    assert csr.blob.numel() == 2 * half
    csr.blob = torch.cat([csr.blob[:half], csr.blob[:half]]).contiguous()
    csr.to(dev)
    X, L = r["X"].to(dev), r["L"].to(dev)
    ps = [r["p"][k].to(dev).contiguous() for k in PARAM_KEYS]
    gs = [torch.full_like(q, 7.0) for q in ps]
    loss = torch.zeros((), device=dev)
    Y, stash, d = gcn_gru_forward_raw(csr, X, ps, MATH["f32"], labels=L)
    gcn_gru_backward_mse_raw(d, csr, X, ps, Y, L, stash, gs, loss, 1.0, part=7 | 8)
    torch.cuda.synchronize()
    err = {k: rel_to_max(gk.cpu(), r["grads"][k]) for k, gk in zip(PARAM_KEYS, gs)}
    err["Y"] = max_abs(Y.cpu(), r["Y"])
    print("csr S%d with A in the A^T half: %s" % (S, " ".join("%s=%.2e" % kv for kv in err.items())))
    assert min(err["conv1.weight"], err["conv1.bias"]) > 100 * G_TOL, err
    assert err["Y"] <= Y_TOL and all(err[k] <= G_TOL for k in PARAM_KEYS[4:]), err


@pytest.mark.parametrize("case", li.LAYER_CASES, ids=[c[0] for c in li.LAYER_CASES])
def test_lattice_graph_conv_layer_of_any_widths(case):
    """gcn_any.hip through GraphConvLayer against fp64 autograd of relu(A X W + b).  Every partial sum of the forward is a
    dyadic number of fewer than 24 bits (multiples of 1/32 below 128), so the output is exact in any summation order: it is held
    to equality, the gradients of the signed random dout to the suite's bar."""
    from windgnn_amd import GraphConvLayer
    cid, S, Fi, Fo, nt = case
    dev = _dev()
    d = li.draw_layer(S, Fi, Fo, nt)
    layer = GraphConvLayer(Fi, Fo)
    layer.load_state_dict({"weight": d.W, "bias": d.b})
    layer = layer.to(dev)
    X = d.X.to(dev).requires_grad_(True)

    def run():
        out = layer(d.A.to(dev), X)
        out.backward(d.dout.to(dev))
        return out

    out, prof = _profiled_counts(run)
    leaves = [t.double().clone().requires_grad_(True) for t in (d.X, d.W, d.b)]
    ref = torch.relu(torch.matmul(torch.matmul(d.A.double(), leaves[0]), leaves[1]) + leaves[2])
    ref.backward(d.dout.double())
    err = {"out": max_abs(out.detach().cpu(), ref.detach()), "dX": rel_to_max(X.grad.cpu(), leaves[0].grad),
           "dW": rel_to_max(layer.weight.grad.cpu(), leaves[1].grad), "db": rel_to_max(layer.bias.grad.cpu(), leaves[2].grad)}
    print("%s S%d %d -> %d: %s" % (cid, S, Fi, Fo, " ".join("%s=%.2e" % kv for kv in err.items())))
    assert set(li.LAYER_KERNELS) <= set(prof), (cid, prof)
    assert err["out"] == 0.0, (cid, err)
    for what in ("dX", "dW", "db"):
        assert err[what] <= G_TOL, (cid, what, err[what])


@pytest.mark.parametrize("S,B", li.STEP_CASES)
def test_lattice_hourly_step(S, B):
    """gru_step_kernel (wgnn_fwd_state at T = 1: both graph convolutions and the GRU cell in ONE launch) from a signed h0."""
    from windgnn_amd.functional import gcn_gru_state
    dev = _dev()
    H = li.H_
    d = li.draw(S, 1, B, H)
    ps = [d.p[k].to(dev).contiguous() for k in PARAM_KEYS]
    with torch.no_grad():
        (Y, hn), prof = _profiled_counts(lambda: gcn_gru_state(d.A.to(dev), d.X.to(dev), ps, MATH["f32"], h0=d.h0.to(dev)))
    assert prof == {"gru_step_kernel": 1}, prof
    _, f = _fp64_model(d.p)
    Yr, hnr = f(d.A, d.X, d.h0.double())
    err = {"Y": max_abs(Y.cpu(), Yr.detach()), "hn": max_abs(hn.cpu(), hnr.detach())}
    print("gru_step S%d B%d: %s" % (S, B, " ".join("%s=%.2e" % kv for kv in err.items())))
    assert err["Y"] <= Y_TOL and err["hn"] <= Y_TOL, err


@functools.lru_cache(maxsize=2)
def _series_reference(S, H, rows, T, stride, n, seed):
    """The lattice series cut into its windows and the fp64 oracle's results on them, for the three routes."""
    from oracle import windgnn_oracle as orc
    d = li.draw_series(S, H, rows, T, stride, n, seed)
    A, p64 = d.A.double(), {k: v.double() for k, v in d.p.items()}
    X, L = windows(d.Xs, T, stride, n).double(), windows(d.Ls, T, stride, n).double()
    Yo, cache = orc.forward(A, X, p64)
    go = orc.backward(A, X, p64, Yo, cache, d.dY.double())
    _, loss, gm = orc.train_step(A, X, L, p64)
    return d, Yo, go, float(loss), gm


@pytest.mark.parametrize("case", li.SERIES_CASES, ids=["S%d_%s" % (c[0], c[7]) for c in li.SERIES_CASES])
def test_lattice_series(case):
    from windgnn_amd import GCN_GRU
    from windgnn_amd.series import (forward_last_series, series_backward_mse_raw, series_backward_raw, series_forward_loss_raw,
                                    series_forward_raw)
    S, H, rows, T, stride, n, seed, route = case
    dev = _dev()
    d, Yo, go, loss_o, gm = _series_reference(S, H, rows, T, stride, n, seed)
    A, Xs = d.A.to(dev), d.Xs.to(dev)
    ps = [d.p[k].to(dev).contiguous() for k in PARAM_KEYS]

    def run():
        gs = [torch.full_like(q, 7.0) for q in ps]
        if route == "series_last":
            model = GCN_GRU(13, 13, 13, S * 13, H)
            model.load_state_dict({k: v.clone() for k, v in d.p.items()})
            with torch.no_grad():
                return dict(last=forward_last_series(model.to(dev), A, Xs, T, WIND_MIN, WIND_MAX, stride, n_windows=n))
        if route == "series":
            Y, stash, sd = series_forward_raw(A, Xs, T, stride, ps, n_windows=n)
            series_backward_raw(sd, A, Xs, ps, Y, d.dY.to(dev), stash, gs)
            return dict(Y=Y, grads=gs)
        Ls = d.Ls.to(dev)
        loss = torch.zeros((), device=dev)
        Y, stash, loss_buf, sd = series_forward_loss_raw(A, Xs, Ls, T, stride, ps, n_windows=n)
        series_backward_mse_raw(sd, A, Xs, ps, Y, Ls, stash, loss_buf, gs, loss)
        return dict(Y=Y, loss=loss, grads=gs)

    out, names = _profiled(run)
    err = {}
    if route == "series_last":
        err["last"] = rel_to_max(out["last"].cpu(), Yo[:, -1, :] * (WIND_MAX - WIND_MIN) + WIND_MIN)
    else:
        err["Y"] = rel_to_max(out["Y"].cpu(), Yo)
        ref = go if route == "series" else gm
        if route == "series_mse":
            err["loss"] = abs(float(out["loss"]) - loss_o) / loss_o
        for k, gk in zip(PARAM_KEYS, out["grads"]):
            err[k] = rel_to_max(gk.cpu(), ref[k])
    print("S%d H%d rows%d T%d stride%d n%d %s: %s" % (S, H, rows, T, stride, n, route, " ".join("%s=%.2e" % kv for kv in err.items())))
    expected = ic.series_plan(S, H, rows, T, stride, n, route)
    ran = sorted({x for x in names if _base(x) in TABLED})
    assert ran == sorted({ic.name_of(k) for k in expected}), (ran, expected)
    assert "gcn32_fwd_kernel<%d>" % ic.gcn_nt(S) in ran
    assert route == "series_last" or "gcn32_bwd_kernel<%d>" % ic.gcn_nt(S) in ran
    for what, e in err.items():
        assert e <= (LOSS_TOL if what == "loss" else SERIES_TOL), (route, what, e)
