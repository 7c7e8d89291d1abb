"""What a table of window starts costs series mode, in one process on one device, at S = 34, H = 102, T = 24, n = 4096, math = "f32":

  (1) strided     TrainStep.step_series(adj, series, Ls, T, stride=1)
  (2) table       TrainStep.step_series(adj, series, Ls, T, starts=arange(n)): the SAME windows, so (2) - (1) is the table's price
                  (the check of the table, the sort, the table reads in the recurrences, the binary-search fold)
  (3) outages     a series with two outages: step_series(starts=segment_starts(segments, T, horizon=3)) on the whole series
  (4) windows     TrainStep.step(adj, X, L) on (3)'s windows materialised once (make_windows(feat, T, starts=...))

Every route starts from the same parameters and takes the same number of steps.  The clocks are tools/series_train_cost.py's:
device events around each step with the routes alternated (medians and minima of --reps steps after --warmup), and a host clock
around --reps back-to-back steps of one route that end in one device synchronise.  Then the library's per-kernel tally of one step
of (1), (2) and (3).

    python tools/series_starts_cost.py [--reps 30] [--warmup 5] [--n 4096] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import windgnn_oracle as orc  # noqa: E402
from tools.series_train_cost import host_loop, kernels, timed  # noqa: E402
from windgnn_amd import GCN_GRU  # noqa: E402
from windgnn_amd.data import make_windows  # noqa: E402
from windgnn_amd.series import segment_starts, series_labels  # noqa: E402
from windgnn_amd.trainer import TrainStep  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    S, T, H, n = 34, 24, 102, a.n
    g = torch.Generator().manual_seed(5)
    A = (torch.rand(S, S, generator=g) / S + 0.01).to(dev)
    p0 = orc.init_params(S, 13, H, seed=1)

    def fresh():
        m = GCN_GRU(13, 13, 13, S * 13, H, math="f32").to(dev)
        m.load_state_dict(p0)
        return TrainStep(m)

    # (1), (2): the contiguous series of n windows at stride 1
    rows = n - 1 + T
    feat = torch.rand(rows + 3, S, 13, generator=g).to(dev)
    series, Ls = feat[:rows], series_labels(feat, T, 1, n_windows=n)[0]
    table = torch.arange(n, device=dev, dtype=torch.int32)
    # (3), (4): two outages (24 h and 50 h) in a longer series; the first n windows that lie, with their +3 h labels, inside a
    # clean segment
    gaps = ((rows // 3, 24), (2 * rows // 3, 50))
    rows_o = rows + sum(c for _, c in gaps) + 2 * (T + 2)          # what the outages and the windows across their edges take
    feat_o = torch.rand(rows_o + 3, S, 13, generator=g).to(dev)
    segments, at = [], 0
    for first, count in gaps:
        segments.append((at, first - at))
        at = first + count
    segments.append((at, rows_o + 3 - at))
    starts_o = [s for s in segment_starts(segments, T, 1, horizon=3) if s + T <= rows_o][:n]
    assert len(starts_o) == n, (len(starts_o), n)
    series_o, Ls_o = feat_o[:rows_o], series_labels(feat_o, T, 1, n_windows=1)[0]
    assert Ls_o.shape[0] == rows_o
    X, L = make_windows(feat_o, T, starts=starts_o)
    table_o = torch.tensor(starts_o, device=dev, dtype=torch.int32)

    t1, t2, t3, t4 = fresh(), fresh(), fresh(), fresh()
    routes = [("1", lambda: t1.step_series(A, series, Ls, T, 1, n_windows=n)),
              ("2", lambda: t2.step_series(A, series, Ls, T, starts=table)),
              ("3", lambda: t3.step_series(A, series_o, Ls_o, T, starts=table_o)),
              ("4", lambda: t4.step(A, X, L))]
    t = {name: [] for name, _ in routes}
    for i in range(a.warmup + a.reps):
        for name, step in routes:
            us = timed(step)
            if i >= a.warmup:
                t[name].append(us)

    def apart(u, v):
        return max(float((p.detach() - q.detach()).abs().max() / q.detach().abs().max())
                   for p, q in zip(u.model.parameters(), v.model.parameters()))

    same12 = all(torch.equal(p, q) for p, q in zip(t1.model.parameters(), t2.model.parameters()))
    host = {name: host_loop(step, a.reps) for name, step in routes}
    med = {name: statistics.median(v) for name, v in t.items()}
    lines = ["S=%d H=%d T=%d n=%d math=f32; us per training step; device events: %d alternated steps per route after %d warm-up "
             "steps, medians (min); host clock: %d back-to-back steps ending in one synchronise"
             % (S, H, T, n, a.reps, a.warmup, a.reps),
             "series [%d, %d, 13]; with outages %s: series [%d, %d, 13], %d clean segments, windows X + L = %.1f MB"
             % (rows, S, list(gaps), rows_o, S, len(segments), (X.numel() + L.numel()) * 4e-6),
             "parameters after %d steps: (2) %s (1)'s; (4) within %.1e of (3)'s, relative to max"
             % (a.warmup + a.reps, "bit-identical to" if same12 else "NOT bit-identical to", apart(t4, t3))]
    for name, what in (("1", "(1) step_series stride=1        "), ("2", "(2) step_series starts=arange(n)"),
                       ("3", "(3) step_series, two outages    "), ("4", "(4) step on (3)'s windows       ")):
        lines.append("  %s events %8.1f (%8.1f)   host clock %8.1f" % (what, med[name], min(t[name]), host[name]))
    lines.append("  the table's price, (2) - (1): events %+.1f us (%.3f x), host clock %+.1f us (%.3f x)"
                 % (med["2"] - med["1"], med["2"] / med["1"], host["2"] - host["1"], host["2"] / host["1"]))
    lines.append("  outages, (3) / (4): events %.3f, host clock %.3f" % (med["3"] / med["4"], host["3"] / host["4"]))
    tally = ["kernels of one step of (1) (per-kernel events serialise the launches):"] + kernels(routes[0][1])
    tally += ["kernels of one step of (2):"] + kernels(routes[1][1])
    tally += ["kernels of one step of (3):"] + kernels(routes[2][1])
    text = "\n".join(lines + tally)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
