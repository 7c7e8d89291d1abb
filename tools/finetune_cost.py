"""Cost of a training step with a frozen parameter group (TrainStep(trainable="gru" | "conv")) against the step on all eight
tensors, in one process on one device:

  (a)  all                 TrainStep.step(adj, X, L): parts 1, 2, 4 of the backward deferred, ONE wgnn_finish(6, adam)
  (a2) all again           a second instance of (a): what two identical routes differ by in this run (the noise yardstick)
  (g)  gru                 parts 1 and 4, wgnn_finish(4), wgnn_finish(WGNN_FINISH_ADAM_GRU): no dg GEMM, no GCN backward
  (c)  conv                parts 1 and 2, wgnn_finish(2), wgnn_finish(WGNN_FINISH_ADAM_CONV): no weight-gradient GEMMs
  (gn) gru, not deferred   TrainStep.FROZEN_DEFER = False: part 4 reduces its own partial sums, one wgnn_finish(ADAM_GRU)
  (cn) conv, not deferred  the same for part 2

at S = 34, H = 102, T = 24, B = 4096 and B = 256 in "f32" and "f16x3", and step_series on the B sliding windows of one series
(exact fp32; series mode has no parts, so a frozen group saves no backward time there).  The clock is device events around each
route with the routes alternated, their order rotated by one from round to round so that no route always follows the same one
(medians and minima of --reps rounds after --warmup).  Then the library's per-kernel tally of one (a), (g) and (c) -- per-kernel
events serialise the launches -- and, from it, what the feature is held to: (g) must beat (a) by at least half of the summed
event times of the kernels (a) launches and (g) does not, and (c) likewise.

    python tools/finetune_cost.py [--reps 30] [--warmup 5] [--out profiles/r23_finetune_cost.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import windgnn_oracle as orc  # noqa: E402
from windgnn_amd import GCN_GRU, _lib  # noqa: E402
from windgnn_amd.trainer import TrainStep  # noqa: E402
from series_train_cost import timed  # noqa: E402

ORDER = ("a", "a2", "g", "c", "gn", "cn")
GROUP = {"a": "all", "a2": "all", "g": "gru", "c": "conv", "gn": "gru", "cn": "conv"}
WHAT = {"a": "(a)  all                       ", "a2": "(a2) all, 2nd instance         ", "g": "(g)  gru                       ",
        "c": "(c)  conv                      ", "gn": "(gn) gru, part 4 not deferred  ", "cn": "(cn) conv, part 2 not deferred "}


def tally(fn):
    """{kernel name: (launches, us)} of one call of fn, by the library's profile aid."""
    _lib.profile_enable(True)
    try:
        fn()
        torch.cuda.synchronize()
        return {k["name"]: (k["launches"], 1e3 * k["ms"]) for k in _lib.profile_read() if k["launches"]}
    finally:
        _lib.profile_enable(False)


def measure(title, routes, tr, order, reps, warmup, lines):
    t = {name: [] for name in order}
    for i in range(warmup + reps):
        k = i % len(order)                  # the order rotates from round to round: every route follows every other equally often
        for name in order[k:] + order[:k]:
            us = timed(routes[name])
            if i >= warmup:
                t[name].append(us)
    med = {name: statistics.median(v) for name, v in t.items()}
    quart = statistics.quantiles(t["a"], n=4)
    yard = abs(med["a2"] - med["a"])
    lines.append("%s; us per optimiser step; device events: %d alternated rounds per route after %d warm-up rounds, medians (min)"
                 % (title, reps, warmup))
    lines.append("noise: (a)'s %d single steps spread over %.1f us (%.1f .. %.1f, quartiles %.1f .. %.1f); the two 'all' instances' "
                 "medians differ by %+.1f us (the yardstick)" % (len(t["a"]), max(t["a"]) - min(t["a"]), min(t["a"]), max(t["a"]),
                                                                 quart[0], quart[2], med["a2"] - med["a"]))
    for name in order:
        lines.append("  %s %8.1f (%8.1f)   this - (a) = %+8.1f us = %+6.2f %%"
                     % (WHAT[name], med[name], min(t[name]), med[name] - med["a"], 100.0 * (med[name] - med["a"]) / med["a"]))
    lines.append("losses after %d steps: %s" % (tr["a"].steps, "  ".join("(%s) %.6f" % (n, float(tr[n]._loss)) for n in order)))
    return med, yard


def held_to(routes, med, yard, lines):
    """The per-kernel tallies of one (a), (g), (c) and the rule of the module docstring."""
    tallies = {name: tally(routes[name]) for name in ("a", "g", "c")}
    for name in ("a", "g", "c"):
        lines.append("the library's kernels of one (%s) (per-kernel events serialise the launches): %.1f us in all"
                     % (name, sum(us for _, us in tallies[name].values())))
        lines += ["    %-34s x%d %8.1f us" % (k, n, us) for k, (n, us) in tallies[name].items()]
    for name, part in (("g", 2), ("c", 4)):
        # (a kernel that both launch, such as wgnn_finish's, counts by the launches (a) has more of, at (a)'s mean time)
        skipped = {k: us * (n - tallies[name].get(k, (0, 0.0))[0]) / n for k, (n, us) in tallies["a"].items()
                   if n > tallies[name].get(k, (0, 0.0))[0]}
        total = sum(skipped.values())
        saved = med["a"] - med[name]
        lines.append("(%s) skips part %d = %s: %.1f us by (a)'s tally; held to half of it, %.1f us: saved %.1f us (%.1f %% of (a)) "
                     "-> %s; yardstick %.1f us" % (name, part, " + ".join(sorted(skipped)) or "nothing", total, total / 2, saved,
                                                   100.0 * saved / med["a"], "MET" if saved >= total / 2 else "NOT MET", yard))
    for d, n in (("g", "gn"), ("c", "cn")):
        lines.append("deferral: (%s) deferred %.1f us, (%s) not deferred %.1f us: deferring is %+.1f us"
                     % (d, med[d], n, med[n], med[d] - med[n]))


def fresh(math, S, H, p0, dev, name):
    m = GCN_GRU(13, 13, 13, S * 13, H, math=math, validate=False).to(dev)
    m.load_state_dict(p0)
    tr = TrainStep(m, check_every=0, trainable=GROUP[name])
    if name in ("gn", "cn"):
        tr.FROZEN_DEFER = False             # (an instance attribute over the class's choice)
    return tr


def windows_run(math, S, T, H, B, reps, warmup, lines):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    A = (torch.rand(S, S, generator=g) / S + 0.01).to(dev)
    p0 = orc.init_params(S, 13, H, seed=1)
    X = torch.rand(B, T, S, 13, generator=g).to(dev)
    L = torch.rand(B, T, H, generator=g).to(dev)
    tr = {k: fresh(math, S, H, p0, dev, k) for k in ORDER}
    routes = {k: (lambda k=k: tr[k].step(A, X, L)) for k in ORDER}
    med, yard = measure("materialised windows, math=%s S=%d H=%d T=%d B=%d" % (math, S, H, T, B), routes, tr, ORDER, reps, warmup,
                        lines)
    held_to(routes, med, yard, lines)


def series_run(S, T, H, B, reps, warmup, lines):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(6)
    A = (torch.rand(S, S, generator=g) / S + 0.01).to(dev)
    p0 = orc.init_params(S, 13, H, seed=1)
    rows = B + T - 1
    series = torch.rand(rows, S, 13, generator=g).to(dev)
    Ls = torch.rand(rows, H, generator=g).to(dev)
    order = ORDER[:4]
    tr = {k: fresh("f32", S, H, p0, dev, k) for k in order}
    routes = {k: (lambda k=k: tr[k].step_series(A, series, Ls, T)) for k in order}
    measure("series mode (step_series: the backward runs whole, the frozen slots are zeroed after it), math=f32 S=%d H=%d T=%d, "
            "%d windows at stride 1" % (S, H, T, B), routes, tr, order, reps, warmup, lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for B in (4096, 256):
        for math in ("f32", "f16x3"):
            windows_run(math, 34, 24, 102, B, a.reps, a.warmup, lines)
            lines.append("")
    series_run(34, 24, 102, 4096, a.reps, a.warmup, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
