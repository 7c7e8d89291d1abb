"""The general path's two loops past their first trip, on the MI355X.

A. The persistent LDS-tiled CSR layers (csrc/general.hip: csr_layer_fwd_kernel, csr_layer_bwd_kernel<1> / <2>) at
tests/general_cases.py's CSR_LOOP_SHAPES: 258 or 260 items on 256 blocks in each of the three item geometries, so that blocks
run a SECOND item -- a second csr_gather into the LDS buffer the copy-out or the MFMA contraction of the previous item has just
used, acc64 carried across items, a ragged last group met by a block that already ran a full one, the ones column of the planes
written for a later item.  Inputs are tests/lattice_inputs.py's sparse draw (live masks that differ between stations, A != A^T,
non-zero biases: a row or tile taken from the wrong item changes the numbers); a case asserts the launched names and holds Y, the
loss and the 8 gradients to the fp64 oracle at tests/test_gpu_instances.py's bars.  The one-layer API (GraphConvLayer with a
CsrAdjacency) runs at 258 items and at 16 385 tiles, where csr_spmm_kernel's tile loop takes its second trip.

B. gemm_f32_kernel (csrc/gemm.hip) past one K step: tests/instance_cases.py's GEMM_F32_KLOOP_CASES (seven steps where CASES
runs one) and GEMM_F32_FOLD_CASES (33 steps or more in one chunk: the two-level fold), through tests/test_gpu_instances.py's
_check -- the same launched-name assertion, references and bars.

Every bar is imported.  tests/test_general_loops_host.py re-derives the tables and qualifies the inputs without a GPU.  A
reference is computed once per shape and shared between the modes (functools.lru_cache, never written to)."""
import functools

import pytest
import torch

import general_cases as gc
import instance_cases as ic
import lattice_inputs as li
from conftest import PARAM_KEYS, max_abs, rel_to_max
from test_gpu_instances import _bounds, _check, _profiled
from test_gpu_state_train import MATH

pytestmark = pytest.mark.gpu

LAYER_TOL = 1e-5              # test_gpu_parity.py::test_graph_conv_layer_with_csr_adjacency's bar on out, dX, dW and db


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=2)
def _reference(S, T, B, H, shift, seed):
    """The sparse lattice draw of a shape and the fp64 oracle's step on it (dense A: the oracle has no other)."""
    from oracle import windgnn_oracle as orc
    d = li.draw(S, T, B, H, True, shift, seed)
    Yo, loss_o, go = orc.train_step(d.A.double(), d.X.double(), d.L.double(), {k: v.double() for k, v in d.p.items()})
    return dict(A=d.A, X=d.X, L=d.L, p=d.p, Y=Yo, loss=float(loss_o), grads=go)


def _csr_step(S, T, B, H, shift, seed, math, route):
    """One step over the CSR adjacency on the GPU: the names it launched and its errors against the reference."""
    from windgnn_amd.functional import check_range_status, gcn_gru_backward_mse_raw, gcn_gru_forward_raw
    from windgnn_amd.graph import CsrAdjacency
    dev = _dev()
    r = _reference(S, T, B, H, shift, seed)
    A = CsrAdjacency.from_dense(r["A"]).to(dev)
    X = r["X"].to(dev)
    ps = [r["p"][k].to(dev).contiguous() for k in PARAM_KEYS]

    def run():
        gs = [torch.full_like(q, 7.0) for q in ps]
        if route == "infer":
            Y, _, _ = gcn_gru_forward_raw(A, X, ps, MATH[math], want_stash=False)
            return dict(Y=Y)
        L = r["L"].to(dev)
        loss = torch.zeros((), device=dev)
        Y, stash, d = gcn_gru_forward_raw(A, X, ps, MATH[math], labels=L)
        gcn_gru_backward_mse_raw(d, A, X, ps, Y, L, stash, gs, loss, 1.0, part=7 | 8)
        return dict(Y=Y, loss=loss, grads=gs)

    out, names = _profiled(run)
    check_range_status(dev)
    err = {"Y": max_abs(out["Y"].float().cpu().reshape(r["Y"].shape), r["Y"])}
    if "loss" in out:
        err["loss"] = abs(float(out["loss"]) - r["loss"]) / max(1.0, r["loss"])
    for k, gk in zip(PARAM_KEYS, out.get("grads", [])):
        err[k] = rel_to_max(gk.cpu(), r["grads"][k])
    return names, err


@pytest.mark.parametrize("case", gc.CSR_LOOP_CASES, ids=[c[0] for c in gc.CSR_LOOP_CASES])
def test_csr_layers_with_several_items_per_block(case):
    cid, S, T, B, H, shift, seed, math, route = case
    plan = gc.csr_plan(S, B * T)
    assert plan["items"] > gc.CSR_BLOCKS and plan["max_items_per_block"] == 2 and plan["regime"] == gc.CSR_LOOP_REGIMES[S], plan
    names, err = _csr_step(S, T, B, H, shift, seed, math, route)
    print("%s S%d T%d B%d H%d %s %s (%d items, %s): %s" % (cid, S, T, B, H, math, route, plan["items"], plan["regime"],
                                                          " ".join("%s=%.2e" % kv for kv in err.items())))
    csr = sorted({n for n in names if n.startswith("csr_")})           # (the profiler reports a name once, however often it ran)
    assert csr == (["csr_layer_fwd_kernel"] if route == "infer" else sorted(gc.CSR_KERNELS)), (cid, names)
    bounds = _bounds(S, T, B, H, math, "f32", False, route)
    for what, e in err.items():
        assert e <= bounds[what], (cid, what, e, bounds[what])


@pytest.mark.parametrize("S,nt", gc.LAYER_LOOP_CASES)
def test_graph_conv_layer_csr_past_one_trip(S, nt):
    """GraphConvLayer over a CsrAdjacency (wgnn_gcn_layer_csr_fwd / _bwd: csr_layer_fwd_kernel, csr_layer_bwd_kernel<2> and, for
    dX, csr_spmm_kernel; these launches are not profiled, and a CSR adjacency has no other route -- any other width raises)
    against fp64 autograd of relu(A X W + b) on lattice_inputs.draw_layer, at test_graph_conv_layer_with_csr_adjacency's bars."""
    from windgnn_amd import GraphConvLayer
    from windgnn_amd.graph import CsrAdjacency
    dev = _dev()
    assert gc.csr_plan(S, nt)["max_items_per_block"] == 2 or gc.spmm_trips(nt) == 2
    d = li.draw_layer(S, 13, 13, nt)
    layer = GraphConvLayer(13, 13)
    layer.load_state_dict({"weight": d.W, "bias": d.b})
    layer = layer.to(dev)
    X = d.X.to(dev).requires_grad_(True)
    out = layer(CsrAdjacency.from_dense(d.A).to(dev), X)
    out.backward(d.dout.to(dev))
    leaves = [t.double().clone().requires_grad_(True) for t in (d.X, d.W, d.b)]
    ref = torch.relu(torch.matmul(torch.matmul(d.A.double(), leaves[0]), leaves[1]) + leaves[2])
    ref.backward(d.dout.double())
    err = {"out": max_abs(out.detach().cpu(), ref.detach()), "dX": rel_to_max(X.grad.cpu(), leaves[0].grad),
           "dW": rel_to_max(layer.weight.grad.cpu(), leaves[1].grad), "db": rel_to_max(layer.bias.grad.cpu(), leaves[2].grad)}
    print("csr layer S%d nt%d: %s" % (S, nt, " ".join("%s=%.2e" % kv for kv in err.items())))
    for what, e in err.items():
        assert e <= LAYER_TOL, (S, nt, what, e)


# a shape's cases run together: they share _reference's fp64 step
GEMM_LOOPS = sorted(ic.GEMM_F32_KLOOP_CASES + [c[:10] for c in ic.GEMM_F32_FOLD_CASES], key=lambda c: (c[2:6], c[1]))


@pytest.mark.parametrize("case", GEMM_LOOPS, ids=["%s-S%d-H%d" % (c[1], c[2], c[5]) for c in GEMM_LOOPS])
def test_gemm_f32_past_one_k_step(case):
    _check(case, exceptions={})
