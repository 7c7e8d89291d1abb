"""Cost of the on-device evaluation statistics (include/windgnn_eval.h), device events after warm-up:

  1. the wgnn_eval_accum and wgnn_eval_stats launches at (B 4096, S 34), (B 1, S 34) and (B 128, H 12 288), with and without
     the abs_err rows;
  2. the test loop at B = 1, T = 168, S = 34 over --windows windows, wall time per window with one synchronisation at the end:
     the reference-style loop (forward_last -> .cpu().numpy() -> three lists -> the numpy statistics of src/main.py:110-157)
     against Evaluator.update + compute, and forward_last's own device time for the accumulate launch's share of it.

    python tools/eval_cost.py [--windows 300] [--reps 50] [--mode f16x3] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import windgnn_oracle as orc  # noqa: E402
from windgnn_amd import GCN_GRU, Evaluator  # noqa: E402
from windgnn_amd.data import forward_last  # noqa: E402
from windgnn_amd.evaluate import eval_accum, eval_buffer, eval_stats  # noqa: E402


def _events(fn, reps):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        t.append(1e3 * e0.elapsed_time(e1))
    return statistics.median(t), min(t)


def _reference_stats(predictions, truth, losses, S):
    """src/main.py:115-157 (np.sqrt(np.mean(...)) for sklearn's retired squared=False)."""
    out = []
    for k in range(3):
        rows = []
        for i in range(S):
            p = [l[i + k * S] for l in predictions]
            t = [l[-1, i + k * S] for l in truth]
            e = np.array([l[i + k * S] for l in losses])
            acc = 1 - e / np.array(t)
            rows.append([np.sqrt(np.mean((np.array(t) - np.array(p)) ** 2)), np.average(e), np.average(acc), np.std(acc)])
        out.append(rows)
    return np.array(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=300)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--mode", default="f16x3")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(9)
    wmin, wmax = 0.0, 60.0
    lines = ["wgnn_eval_accum / wgnn_eval_stats, device events, %d repetitions after warm-up; medians (min) in us" % a.reps]
    for B, T, H in ((4096, 24, 102), (1, 168, 102), (128, 24, 12288)):
        labels = (torch.rand(B, T, H, generator=g) * 0.8 + 0.2).to(dev)
        pred = (labels[:, -1] * (wmax - wmin) * (1 + 0.3 * torch.randn(B, H, generator=g).to(dev))).contiguous()
        acc, err, out = eval_buffer(H, dev), torch.empty(B, H, device=dev), torch.empty(H, 4, device=dev)
        plain = _events(lambda: eval_accum(pred, labels, wmin, wmax, acc), a.reps)
        kept = _events(lambda: eval_accum(pred, labels, wmin, wmax, acc, err), a.reps)
        stats = _events(lambda: eval_stats(acc, H, out), a.reps)
        lines.append("B %5d T %3d H %5d   accum %7.1f (%7.1f)   accum + abs_err %7.1f (%7.1f)   stats %6.1f (%6.1f)"
                     % (B, T, H, *plain, *kept, *stats))

    S, T, H, N = 34, 168, 102, a.windows
    A = (torch.rand(S, S, generator=g) / S + 0.01).to(dev)
    m = GCN_GRU(13, 13, 13, S * 13, H, math=a.mode).to(dev)
    m.load_state_dict(orc.init_params(S, 13, H, seed=1))
    xs = [torch.rand(1, T, S, 13, generator=g).to(dev) for _ in range(8)]
    ys = [(torch.rand(1, T, H, generator=g) * 0.8 + 0.2).to(dev) for _ in range(8)]
    fwd = _events(lambda: forward_last(m, A, xs[0], wmin, wmax), a.reps)
    p0 = forward_last(m, A, xs[0], wmin, wmax).reshape(1, H)
    acc = eval_buffer(H, dev)
    accum1 = _events(lambda: eval_accum(p0, ys[0], wmin, wmax, acc), a.reps)

    def host_loop():
        predictions, truth, losses = [], [], []
        for i in range(N):
            out = forward_last(m, A, xs[i % 8], wmin, wmax)
            p = out.detach().cpu().numpy()                                        # main.py:103 (de-normalised on the device)
            t = ys[i % 8].detach().cpu().numpy() * (wmax - wmin) + wmin           # main.py:104
            losses.append(abs(t[0][-1] - p))                                      # main.py:105 (its last row)
            predictions.append(p)
            truth.append(t[0])
        return _reference_stats(predictions, truth, losses, S)

    ev = Evaluator(m, A, wmin, wmax)

    def device_loop():
        ev.reset()
        for i in range(N):
            ev.update(xs[i % 8], ys[i % 8])
        return ev.compute().stats.cpu().numpy()

    walls = {}
    for name, loop in (("host loop", host_loop), ("Evaluator", device_loop)):
        loop()
        t = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            res = loop()
            torch.cuda.synchronize()
            t.append((time.perf_counter() - t0) / N * 1e6)
        walls[name] = (statistics.median(t), res)
    ref, got = walls["host loop"][1], walls["Evaluator"][1]
    worst = float(np.max(np.abs(got - ref) / np.abs(ref)))
    lines += ["",
              "test loop, B = 1, T = %d, S = %d, %s, %d windows, wall time per window (median of 3 loops, statistics included)"
              % (T, S, a.mode, N),
              "forward_last -> .cpu().numpy() -> lists -> numpy statistics   %8.1f us / window" % walls["host loop"][0],
              "Evaluator.update ... compute()                               %8.1f us / window" % walls["Evaluator"][0],
              "ratio host loop / Evaluator                                  %8.2f" % (walls["host loop"][0] / walls["Evaluator"][0]),
              "forward_last alone, device events                            %8.1f us (%.1f)" % fwd,
              "wgnn_eval_accum at B = 1, device events                      %8.1f us (%.1f) = %.1f %% of forward_last"
              % (*accum1, 100.0 * accum1[0] / fwd[0]),
              "largest relative difference between the two loops' figures   %8.2e" % worst]
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
