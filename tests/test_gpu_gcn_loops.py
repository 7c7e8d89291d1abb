"""The dense graph-convolution kernels past one tile per wave, on the MI355X: tests/gcn_loop_cases.py's GCN_LOOP_CASES.

gcnx_fwd / gcnx_bwd / gcn32_fwd / gcn32_bwd are persistent over the (window, hour) tiles -- `for (tile = wave_id; tile < ntiles;
tile += nwaves)` with the next tile's X (in the backward also its g mask and dg) prefetched under the current tile's math -- and
gcngi_fwd over tiles of 32 or 48 rows with two g buffers.  At the per-instance table's 34 rows every wave runs the loop body
once.  Here every key of the five families runs at 8198 rows (gcngi: 16 386 or 24 578), where the keyed launch makes three or five
trips, some waves one fewer, and the last tile -- the private copy of odd S * 13 -- falls on the final trip; S = 34 and S = 64 add
the even-I branch of XLOAD.  Inputs are tests/lattice_inputs.py's draw (live ReLU masks that differ between stations and tiles,
non-zero biases, A != A^T: a tile, a mask or a partial sum from the wrong trip changes the numbers;
tests/test_gcn_loops_host.py plants exactly those mistakes into the fp64 reference).  A case runs one step through
tests/test_gpu_lattice.py's _step, asserts by name that plan()'s kernels and no others of the tabled families ran, that every
GCN launch of the step makes three trips or more, and holds Y, the loss and the 8 gradients to the fp64 oracle at that module's
bars: all imported, none new.  Cases that share a call form share the GPU step, cases that share a shape the reference.

The one-layer kernels (gcn.hip's 13 -> 13 pair, gcn_any.hip) run GraphConvLayer at three trips with a ragged third."""
import functools

import pytest
import torch

import gcn_loop_cases as gl
import instance_cases as ic
import lattice_inputs as li
import test_gpu_lattice as tgl
from conftest import PARAM_KEYS, max_abs, rel_to_max
from test_gpu_instances import _bounds

pytestmark = pytest.mark.gpu

LAYER_TOL = 1e-5              # test_gpu_parity.py::test_graph_conv_layer_with_csr_adjacency's bar on out, dX, dW and db

# a shape's cases run together, 16-bit I/O after fp32 I/O: they share tgl._reference's fp64 step
ORDERED = sorted(gl.ALL_LOOP_CASES, key=lambda c: (list(gl.loop_shapes()).index(c[2:6]), c[7], c[8], c[6], c[9], c[1]))


@functools.lru_cache(maxsize=None)
def _run(S, T, B, H, math, io, state, route):
    """One GPU step per call form: the names it launched and its errors (floats only)."""
    shift, seed = gl.inputs_of(S, T, B, H)
    names, err = tgl._step(S, T, B, H, math, io, state, route, False, shift, seed)
    return tuple(names), err


def _bars(S, T, B, H, math, io, state, route):
    """test_gpu_lattice._bars; a one-pass fp16 case looks its reference figure up in gl.F16_FIGURES (by shape) where that
    function looks in lattice_inputs.F16_FIGURES (by case id): the larger of the imported bar and twice the figure."""
    if math != "f16":
        return tgl._bars(None, S, T, B, H, math, io, state, route)
    b = dict(_bounds(S, T, B, H, math, io, state, route))
    fy, fl, fg = gl.F16_FIGURES[(S, T, B, H)]
    b.update({k: max(b[k], 2 * fg) for k in PARAM_KEYS}, Y=max(b["Y"], 2 * fy), loss=max(b["loss"], 2 * fl))
    return b


@pytest.mark.parametrize("case", ORDERED, ids=["%s-S%d" % (c[1], c[2]) for c in ORDERED])
def test_gcn_kernels_past_one_tile_per_wave(case):
    fam, key, S, T, B, H, math, io, state, route = case
    expected = ic.plan(S, T, B, H, math, io, state, route)
    launches = gl.gcn_launches(case)
    mine = [l for l in launches if l[0] == key]
    assert key in expected and len(mine) == 1 and mine[0][2] >= gl.LOOP_TRIPS and mine[0][2] % 2 == 1, (key, launches)
    names, err = _run(S, T, B, H, math, io, state, route)
    print("%s S%d T%d B%d H%d %s %s %s (%s): %s"
          % (key, S, T, B, H, math, io, route, ", ".join("%s %d trips on %d" % (ic.name_of(k), trips, n) for k, n, trips, _, _ in launches),
             " ".join("%s=%.2e" % kv for kv in err.items())))
    ran = sorted({n for n in names if tgl._base(n) in tgl.TABLED})
    assert ic.name_of(key) in ran, (key, ran)
    assert ran == sorted({ic.name_of(k) for k in expected}), (key, ran, expected)        # plan()'s kernels and no others
    for k, n, trips, cnt, last in launches:                                             # every GCN launch: three trips or more
        assert trips >= gl.LOOP_TRIPS and last == trips and cnt < n and ic.name_of(k) in ran, (key, k, trips)
    bars = _bars(S, T, B, H, math, io, state, route)
    for what, e in err.items():
        assert e <= bars[what], (key, what, e, bars[what])


@pytest.mark.parametrize("S,Fi,Fo,nt", gl.LAYER_LOOP_CASES)
def test_graph_conv_layer_past_one_trip(S, Fi, Fo, nt):
    """GraphConvLayer over a dense adjacency against fp64 autograd of relu(A X W + b) on lattice_inputs.draw_layer: gcn.hip's
    gcn_fwd_kernel<1> / gcn_bwd_kernel<1> (13 -> 13; these launches are not profiled) and gcn_any.hip's three kernels at three trips
    of the grid, the third ragged."""
    from windgnn_amd import GraphConvLayer
    from test_gpu_state import _profiled as _profiled_counts
    dev = tgl._dev()
    assert gl.layer_trips(Fi, Fo, nt)[1] == 3
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
    print("layer S%d %d -> %d, %d tiles: %s" % (S, Fi, Fo, nt, " ".join("%s=%.2e" % kv for kv in err.items())))
    if (Fi, Fo) == (13, 13):
        assert not set(li.LAYER_KERNELS) & set(prof), prof
    else:
        assert set(li.LAYER_KERNELS) <= set(prof), prof
    for what, e in err.items():
        assert e <= LAYER_TOL, (S, Fi, Fo, nt, what, e)
