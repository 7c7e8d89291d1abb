"""Cost of keeping the best parameters on the device (include/windgnn_best.h): TrainStep.step with keep_best=None (the step as
it was), a threshold that never fires (1e-30: the decide launch and a copy launch whose workgroups return after one word) and
True on a fixed batch, where the loss falls on nearly every early step (the copy runs), at bench.py's shape (S = 34, T = 24,
B = 4096, f16x3).  Device events around each step, the three forms alternated in one process, medians of --reps steps; then
the library's own per-kernel tally of one step of each form (the keep_best=None step's kernel list must not change).

    python tools/best_cost.py [--reps 40] [--mode f16x3] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import windgnn_oracle as orc  # noqa: E402
from windgnn_amd import GCN_GRU, _lib  # noqa: E402
from windgnn_amd.trainer import TrainStep  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--mode", default="f16x3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    S, T, B, H = 34, 24, 4096, 102
    g = torch.Generator().manual_seed(5)
    A = (torch.rand(S, S, generator=g) / S + 0.01).to(dev)
    X = torch.rand(B, T, S, 13, generator=g).to(dev)
    L = torch.rand(B, T, H, generator=g).to(dev)
    p = orc.init_params(S, 13, H, seed=1)

    def trainer(keep_best):
        m = GCN_GRU(13, 13, 13, S * 13, H, math=a.mode).to(dev)
        m.load_state_dict(p)
        return TrainStep(m, check_every=0, keep_best=keep_best)

    forms = [("keep_best=None", trainer(None)), ("keep_best=1e-30", trainer(1e-30)), ("keep_best=True", trainer(True))]
    for _, tr in forms:
        for _ in range(3):
            tr.step(A, X, L)
    torch.cuda.synchronize()
    t = {name: [] for name, _ in forms}
    wins0 = {name: (0 if tr.keep_best is None else int(tr.state_dict()["best"]["improvements"])) for name, tr in forms}
    for _ in range(a.reps):
        for name, tr in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            tr.step(A, X, L)
            e1.record()
            e1.synchronize()
            t[name].append(1e3 * e0.elapsed_time(e1))
    lines = ["S=%d T=%d B=%d H=%d %s, TrainStep.step, %d alternated steps per form, device events; medians (min) in us"
             % (S, T, B, H, a.mode, a.reps),
             "wgnn_keep_best: best_decide_kernel (1 thread) + best_copy_kernel (8 tensors, %d floats)" % forms[0][1].flat_p.numel()]
    base = statistics.median(t[forms[0][0]])
    for name, tr in forms:
        med = statistics.median(t[name])
        extra = ""
        if tr.keep_best is not None:
            wins = int(tr.state_dict()["best"]["improvements"]) - wins0[name]
            extra = "   %d of the %d timed steps copied; best_loss %.6g at step %d" % (wins, a.reps, float(tr.best_loss),
                                                                                      int(tr.best_step))
        lines.append("%-18s %8.1f (%8.1f)   %+6.1f us  %+5.2f %%%s" % (name, med, min(t[name]), med - base,
                                                                    100.0 * (med / base - 1.0), extra))
    # kernel lists: one step of each form under the library's per-kernel events (serialises the launches: times are per kernel)
    for name, tr in forms:
        _lib.profile_enable(True)
        before = {k["name"]: (k["launches"], k["ms"]) for k in _lib.profile_read()}
        tr.step(A, X, L)
        after = _lib.profile_read()
        _lib.profile_enable(False)
        improved = "" if tr.keep_best is None else " (improved = %d)" % int(tr.improved)
        lines.append("kernels of one step, %s%s:" % (name, improved))
        for k in after:
            n0, ms0 = before.get(k["name"], (0, 0.0))
            if k["launches"] - n0:
                lines.append("    %-34s x%d %8.1f us" % (k["name"], k["launches"] - n0, 1e3 * (k["ms"] - ms0)))
    lines.append("BASELINE configs[4] (w_ih 12 288 x 53 248): one improving step moves 2 x 9.66 GB, about 5 ms at the copy rate "
                 "wgnn_finish reaches there -- an estimate, NOT measured.")
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
