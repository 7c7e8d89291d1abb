"""Cost of accumulating gradients over k calls (TrainStep.accumulate x k + apply on B / k windows each) against the one step on
the B windows it equals, in one process on one device:

  (s)  step                TrainStep.step(adj, X, L) on B windows: deferred partial sums, ONE wgnn_finish(6, adam)
  (s2) step again          a second instance of (s): what two identical routes differ by in this run (the noise floor)
  (a1) accumulate x 1      accumulate on the B windows + apply: the non-deferred backward, the copy, the scale, wgnn_finish(0, adam)
  (a2) accumulate x 2      two calls of B / 2 windows + apply
  (a4) accumulate x 4      four calls of B / 4 windows + apply

at S = 34, H = 102, T = 24, B = 4096 in "f32" and "f16x3", and the same for step_series against accumulate_series on the B
sliding windows of one series cut into k consecutive sub-series (exact fp32, as series mode is).  The clock is device events around
each route with the routes alternated, their order rotated by one from round to round so that no route always follows the same
one (medians and minima of --reps rounds after --warmup).  Then the wall time per route back to back, the library's per-kernel
tally of one (s) and one (a2), and torch's own launches of one (a2) as torch.profiler names them.

    python tools/accumulate_cost.py [--reps 30] [--warmup 5] [--B 4096] [--out profiles/r20_accumulate_cost.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import windgnn_oracle as orc  # noqa: E402
from windgnn_amd import GCN_GRU  # noqa: E402
from windgnn_amd.trainer import TrainStep  # noqa: E402
from series_train_cost import host_loop, kernels, timed  # noqa: E402
from validate_cost import torch_launches  # noqa: E402

ORDER = ("s", "s2", "a1", "a2", "a4")
K = {"a1": 1, "a2": 2, "a4": 4}
WHAT = {"s": "(s)  one step on B windows      ", "s2": "(s2) the same, 2nd instance     ", "a1": "(a1) accumulate x 1 + apply     ",
        "a2": "(a2) accumulate x 2 + apply     ", "a4": "(a4) accumulate x 4 + apply     "}


def measure(title, routes, tr, reps, warmup, lines):
    t = {name: [] for name in ORDER}
    for i in range(warmup + reps):
        k = i % len(ORDER)                  # the order rotates from round to round: every route follows every other equally often
        for name in ORDER[k:] + ORDER[:k]:
            us = timed(routes[name])
            if i >= warmup:
                t[name].append(us)
    med = {name: statistics.median(v) for name, v in t.items()}
    quart = statistics.quantiles(t["s"], n=4)
    lines.append("%s; us per optimiser step; device events: %d alternated rounds per route after %d warm-up rounds, medians (min)"
                 % (title, reps, warmup))
    lines.append("noise: (s)'s %d single steps spread over %.1f us (%.1f .. %.1f, quartiles %.1f .. %.1f); the two step instances' "
                 "medians differ by %+.1f us" % (len(t["s"]), max(t["s"]) - min(t["s"]), min(t["s"]), max(t["s"]), quart[0], quart[2],
                                                 med["s2"] - med["s"]))
    for name in ORDER:
        lines.append("  %s %8.1f (%8.1f)   this - (s) = %+8.1f us = %+6.2f %%"
                     % (WHAT[name], med[name], min(t[name]), med[name] - med["s"], 100.0 * (med[name] - med["s"]) / med["s"]))
    lines.append("losses after %d steps: %s" % (tr["s"].steps, "  ".join("(%s) %.6f" % (n, float(tr[n]._loss)) for n in ORDER)))
    lines.append("wall time per optimiser step, %d back to back (launch-bound where it exceeds the device time):" % reps)
    for name in ORDER:
        lines.append("  (%s) %8.1f us" % (name, host_loop(routes[name], reps)))
    for name in ("s", "a2"):
        lines += ["the library's kernels of one (%s) (per-kernel events serialise the launches):" % name] + kernels(routes[name])
    lines += ["torch's device kernels of one (a2), by torch.profiler:"] + torch_launches(routes["a2"])


def fresh(math, S, H, p0, dev):
    m = GCN_GRU(13, 13, 13, S * 13, H, math=math, validate=False).to(dev)
    m.load_state_dict(p0)
    return TrainStep(m, check_every=0)


def windows_run(math, S, T, H, B, reps, warmup, lines):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    A = (torch.rand(S, S, generator=g) / S + 0.01).to(dev)
    p0 = orc.init_params(S, 13, H, seed=1)
    X = torch.rand(B, T, S, 13, generator=g).to(dev)
    L = torch.rand(B, T, H, generator=g).to(dev)
    tr = {k: fresh(math, S, H, p0, dev) for k in ORDER}
    parts = {k: [(X[i * (B // k):(i + 1) * (B // k)], L[i * (B // k):(i + 1) * (B // k)]) for i in range(k)] for k in K.values()}

    def accumulated(name):
        def run():
            for Xi, Li in parts[K[name]]:
                tr[name].accumulate(A, Xi, Li)
            tr[name].apply()
        return run
    routes = {"s": lambda: tr["s"].step(A, X, L), "s2": lambda: tr["s2"].step(A, X, L)}
    routes.update((name, accumulated(name)) for name in K)
    measure("materialised windows, math=%s S=%d H=%d T=%d B=%d" % (math, S, H, T, B), routes, tr, reps, warmup, lines)


def series_run(S, T, H, B, reps, warmup, lines):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(6)
    A = (torch.rand(S, S, generator=g) / S + 0.01).to(dev)
    p0 = orc.init_params(S, 13, H, seed=1)
    rows = B + T - 1
    series = torch.rand(rows, S, 13, generator=g).to(dev)
    Ls = torch.rand(rows, H, generator=g).to(dev)
    tr = {k: fresh("f32", S, H, p0, dev) for k in ORDER}
    # k consecutive sub-series of B / k windows each: their rows overlap by T - 1
    parts = {k: [(series[i * (B // k):(i + 1) * (B // k) + T - 1].contiguous(), Ls[i * (B // k):(i + 1) * (B // k) + T - 1].contiguous())
                 for i in range(k)] for k in K.values()}

    def accumulated(name):
        def run():
            for si, li in parts[K[name]]:
                tr[name].accumulate_series(A, si, li, T)
            tr[name].apply()
        return run
    routes = {"s": lambda: tr["s"].step_series(A, series, Ls, T), "s2": lambda: tr["s2"].step_series(A, series, Ls, T)}
    routes.update((name, accumulated(name)) for name in K)
    measure("series mode (step_series / accumulate_series), math=f32 S=%d H=%d T=%d, %d windows at stride 1" % (S, H, T, B), routes, tr,
            reps, warmup, lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for math in ("f32", "f16x3"):
        windows_run(math, 34, 24, 102, a.B, a.reps, a.warmup, lines)
        lines.append("")
    series_run(34, 24, 102, a.B, a.reps, a.warmup, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
