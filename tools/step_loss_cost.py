"""Cost of a training step on a loss spec on MATERIALISED windows (TrainStep.step(..., loss=...)) against the fused MSE step it
stands beside, on the same windows, in one process on one device, per math mode and I/O type:

  (d)  default step        TrainStep.step(adj, X, L): wgnn_fwd_loss + wgnn_bwd_mse_part, the loss fused into the recurrences
  (d2) default step again  a second instance of (d): what two identical routes differ by in this run (the noise floor)
  (l1) L1                  step(adj, X, L, loss="l1"): wgnn_fwd, functional.loss_spec_grad, wgnn_bwd_part on its dY
  (h)  Huber               the same with loss="huber", huber_delta=0.25
  (hn) Huber, NaN, warm-up the same with 10 % of the labels NaN, missing_labels=True and loss_from=12

at S = 34, H = 102, T = 24, B = 4096, and once more in "f16x3" with bf16 I/O, where a step on a spec runs on fp32 copies of X
and L.  The clock is device events around each step with the routes alternated, their order rotated by one from round to round so
that no route always follows the same one (medians and minima of --reps steps after --warmup).  Then the wall time per step back to back, the library's per-kernel tally of one step of (d),
(h) and (hn), and torch's own launches of one (hn) as torch.profiler names them.

    python tools/step_loss_cost.py [--reps 30] [--warmup 5] [--B 4096] [--out profiles/r18_step_loss_cost.txt]
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

ORDER = ("d", "d2", "l1", "h", "hn")
WHAT = {"d": "(d)  default step (fused MSE)   ", "d2": "(d2) default step, 2nd instance", "l1": "(l1) loss='l1'                 ",
        "h": "(h)  loss='huber'              ", "hn": "(hn) huber, 10 % NaN, from 12  "}


def shape_run(math, S, T, H, B, reps, warmup, lines, io=torch.float32):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    A = (torch.rand(S, S, generator=g) / S + 0.01).to(dev)
    p0 = orc.init_params(S, 13, H, seed=1)
    X = torch.rand(B, T, S, 13, generator=g).to(dev)
    L = torch.rand(B, T, H, generator=g).to(dev)
    Ln = torch.where(torch.rand(B, T, H, generator=g).to(dev) < 0.1, torch.full_like(L, float("nan")), L)
    X, L, Ln = X.to(io), L.to(io), Ln.to(io)          # 16-bit I/O: a step on a spec then runs on fp32 copies (TrainStep._spec_forward)

    def fresh():
        m = GCN_GRU(13, 13, 13, S * 13, H, math=math, validate=False).to(dev)
        m.load_state_dict(p0)
        return TrainStep(m, check_every=0)
    tr = {k: fresh() for k in ORDER}
    routes = {"d": lambda: tr["d"].step(A, X, L), "d2": lambda: tr["d2"].step(A, X, L),
              "l1": lambda: tr["l1"].step(A, X, L, loss="l1"),
              "h": lambda: tr["h"].step(A, X, L, loss="huber", huber_delta=0.25),
              "hn": lambda: tr["hn"].step(A, X, Ln, loss="huber", huber_delta=0.25, loss_from=T // 2, missing_labels=True)}
    t = {name: [] for name in ORDER}
    for i in range(warmup + reps):
        k = i % len(ORDER)                  # the order rotates from round to round: every route follows every other equally often
        for name in ORDER[k:] + ORDER[:k]:
            us = timed(routes[name])
            if i >= warmup:
                t[name].append(us)
    med = {name: statistics.median(v) for name, v in t.items()}
    quart = statistics.quantiles(t["d"], n=4)
    lines.append("math=%s I/O=%s S=%d H=%d T=%d B=%d; us per step; device events: %d alternated steps per route after %d warm-up steps, "
                 "medians (min)" % (math, str(io).replace("torch.", ""), S, H, T, B, reps, warmup))
    lines.append("noise: (d)'s %d single steps spread over %.1f us (%.1f .. %.1f, quartiles %.1f .. %.1f); the two default "
                 "instances' medians differ by %+.1f us" % (len(t["d"]), max(t["d"]) - min(t["d"]), min(t["d"]), max(t["d"]),
                                                            quart[0], quart[2], med["d2"] - med["d"]))
    for name in ORDER:
        lines.append("  %s %8.1f (%8.1f)   this - (d) = %+8.1f us = %+6.2f %%"
                     % (WHAT[name], med[name], min(t[name]), med[name] - med["d"], 100.0 * (med[name] - med["d"]) / med["d"]))
    lines.append("losses after %d steps: (d) %.6f (l1) %.6f (h) %.6f (hn) %.6f over %d labels"
                 % (tr["d"].steps, float(tr["d"]._loss), float(tr["l1"]._loss), float(tr["h"]._loss), float(tr["hn"]._loss),
                    int(tr["hn"].loss_count)))
    lines.append("wall time per step, %d steps back to back (launch-bound where it exceeds the device time):" % reps)
    for name in ORDER:
        lines.append("  (%s) %8.1f us" % (name, host_loop(routes[name], reps)))
    for name in ("d", "h", "hn"):
        lines += ["the library's kernels of one step of (%s) (per-kernel events serialise the launches):" % name] + kernels(routes[name])
    lines += ["torch's device kernels of one step of (hn), by torch.profiler:"] + torch_launches(routes["hn"])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for math, io in (("f32", torch.float32), ("f16x3", torch.float32), ("f16x3", torch.bfloat16)):
        shape_run(math, 34, 24, 102, a.B, a.reps, a.warmup, lines, io)
        lines.append("")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
