"""Cost of one GraphConvLayer wider than 64 features (csrc/gcn_wide.hip) per layer of GCN_GRU(13, hid, 13, ...), in one process
on one device, at S = 34 and ntiles = 4096 * 24 tiles, for hid = 64 (gcn_any.hip, unchanged: the yardstick the library had
before), 128 and 256:

  (w)  this library      GraphConvLayer(Fi, Fo) through autograd: wgnn_gcn_layer_fwd / wgnn_gcn_layer_bwd
  (t)  torch eager       relu(A @ X @ W + b) with autograd on the same tensors -- the vendor GEMM path, a yardstick only
  floor                  the bytes the decomposition must move (each tensor once per launch that needs it) at the measured
                         6.29 TB/s copy rate of BASELINE.md

Layer 1 (13 -> hid) has no dX (the model's X needs no gradient), layer 2 (hid -> 13) has.  Forward alone (no graph recorded)
and forward + backward.  The clock is device events around each call with the routes alternated, their order rotated by one
from round to round (medians and minima of --reps calls after --warmup).  Then the library's per-kernel tally of one forward +
backward per layer.

    python tools/layer_wide_cost.py [--reps 30] [--warmup 5] [--tiles 98304] [--out profiles/r19_layer_wide_cost.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from windgnn_amd import GraphConvLayer  # noqa: E402
from series_train_cost import kernels, timed  # noqa: E402

COPY_TBS = 6.29                      # the device-to-device copy rate, TB/s
ORDER = ("w_f", "t_f", "w_fb", "t_fb")


def floor_us(rows, Fi, Fo, want_dx):
    """(forward, forward + backward) in us: X, out once in the forward; out, dout, V in the aggregation; X, V in the dW product;
    V, dX in the dX product."""
    fwd = 4.0 * rows * (Fi + Fo)
    bwd = 4.0 * rows * (3 * Fo + (Fi + Fo) + ((Fo + Fi) if want_dx else 0))
    return fwd / (COPY_TBS * 1e6), (fwd + bwd) / (COPY_TBS * 1e6)


def layer_run(S, nt, Fi, Fo, want_dx, reps, warmup, lines):
    dev = torch.device("cuda:0")
    g = torch.Generator(device=dev).manual_seed(11 + Fi + Fo)          # drawn on the device: the tensors are gigabytes
    A = torch.rand(S, S, generator=g, device=dev) / S + 0.01
    X = torch.rand(nt, S, Fi, generator=g, device=dev).requires_grad_(want_dx)
    dout = torch.randn(nt, S, Fo, generator=g, device=dev)
    layer = GraphConvLayer(Fi, Fo)
    with torch.no_grad():
        layer.weight.mul_(0.1)
    layer = layer.to(dev)
    W = layer.weight.detach().clone().requires_grad_(True)
    b = layer.bias.detach().clone().requires_grad_(True)

    def eager():
        return torch.relu(torch.matmul(torch.matmul(A, X), W) + b)

    def w_f():
        with torch.no_grad():
            layer(A, X)

    def t_f():
        with torch.no_grad():
            eager()

    def w_fb():
        layer(A, X).backward(dout)

    def t_fb():
        eager().backward(dout)

    routes = {"w_f": w_f, "t_f": t_f, "w_fb": w_fb, "t_fb": t_fb}
    t = {name: [] for name in ORDER}
    for i in range(warmup + reps):
        k = i % len(ORDER)
        for name in ORDER[k:] + ORDER[:k]:
            us = timed(routes[name])
            if i >= warmup:
                t[name].append(us)
            for leaf in (X, W, b, layer.weight, layer.bias):
                leaf.grad = None
    med = {name: statistics.median(v) for name, v in t.items()}
    f_f, f_fb = floor_us(nt * S, Fi, Fo, want_dx)
    with torch.no_grad():
        same = float((layer(A, X) - eager()).abs().max())
    lines.append("%3d -> %3d%s: forward  (w) %9.1f (%9.1f)  (t) %9.1f (%9.1f)  floor %8.1f   (w)/(t) %.2f  (w)/floor %.2f"
                 % (Fi, Fo, " +dX" if want_dx else "    ", med["w_f"], min(t["w_f"]), med["t_f"], min(t["t_f"]), f_f,
                    med["w_f"] / med["t_f"], med["w_f"] / f_f))
    lines.append("              fwd+bwd  (w) %9.1f (%9.1f)  (t) %9.1f (%9.1f)  floor %8.1f   (w)/(t) %.2f  (w)/floor %.2f"
                 "   max |out(w) - out(t)| %.1e"
                 % (med["w_fb"], min(t["w_fb"]), med["t_fb"], min(t["t_fb"]), f_fb, med["w_fb"] / med["t_fb"], med["w_fb"] / f_fb,
                    same))
    tally = kernels(w_fb)
    del X, dout, layer, W, b
    torch.cuda.empty_cache()
    return med, tally


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--S", type=int, default=34)
    ap.add_argument("--tiles", type=int, default=4096 * 24)
    ap.add_argument("--hid", type=int, nargs="+", default=[64, 128, 256])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["one GraphConvLayer, S = %d, %d tiles (%d rows), exact fp32; us per call; device events: %d alternated calls per route "
             "after %d warm-up, medians (min); %s" % (a.S, a.tiles, a.S * a.tiles, a.reps, a.warmup, torch.cuda.get_device_name(0)),
             "(w) this library  (t) torch eager relu(A @ X @ W + b) + autograd  floor: bytes of the decomposition at %.2f TB/s"
             % COPY_TBS]
    tallies = []
    for hid in a.hid:
        lines.append("hid = %d (%s)" % (hid, "gcn_any.hip, unchanged by gcn_wide.hip" if hid <= 64 else "gcn_wide.hip"))
        pair = {}
        for Fi, Fo, want_dx in ((13, hid, False), (hid, 13, True)):
            pair[(Fi, Fo)], tally = layer_run(a.S, a.tiles, Fi, Fo, want_dx, a.reps, a.warmup, lines)
            tallies.append(("%d -> %d" % (Fi, Fo), tally))
        both = {k: sum(m[k] for m in pair.values()) for k in ORDER}
        act = 4.0 * a.tiles * a.S * hid
        lines.append("  both layers: forward (w) %9.1f (t) %9.1f   fwd+bwd (w) %9.1f (t) %9.1f   hidden activation between the "
                     "two calls: %.2f GB written and read again in the forward" % (both["w_f"], both["t_f"], both["w_fb"],
                                                                                  both["t_fb"], act / 1e9))
    lines.append("per-kernel tally of one forward + backward (the library's own events, a separate call):")
    for name, tally in tallies:
        lines.append("  %s" % name)
        lines += tally
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
