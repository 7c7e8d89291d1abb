"""Cost of one series TRAINING step through missing labels (include/windgnn_series_masked.h), three routes on the SAME windows,
in one process on one device:

  (u) unmasked          TrainStep.step_series(adj, series, Ls, T, 1)                                   -- the yardstick
  (m) masked, no NaN    TrainStep.step_series(adj, series, Ls, T, 1, missing_labels=True) on the same Ls
  (g) masked, ~10 % NaN the same call on Ls with one label in ten (scattered) replaced by NaN

at S = 34, H = 102, T = 24, n = 4096 windows, stride 1, math = "f32".  Every route starts from the same parameters.  The clock is
device events around each step with the three routes alternated (medians and minima of --reps steps after --warmup).  Then the
library's per-kernel tally of one step of each route, which says where a difference comes from.  (u) and (m) must hold the
same parameters bit for bit after the same steps: with no NaN the masked kernels compute what the unmasked ones do.

    python tools/series_masked_cost.py [--reps 30] [--warmup 5] [--n 4096] [--out profiles/r14_series_masked_cost.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import windgnn_oracle as orc  # noqa: E402
from windgnn_amd import GCN_GRU  # noqa: E402
from windgnn_amd.series import series_labels  # noqa: E402
from windgnn_amd.trainer import TrainStep  # noqa: E402
from series_train_cost import kernels, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--n", type=int, default=4096)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    S, T, H, n, stride = 34, 24, 102, a.n, 1
    g = torch.Generator().manual_seed(5)
    A = (torch.rand(S, S, generator=g) / S + 0.01).to(dev)
    p0 = orc.init_params(S, 13, H, seed=1)
    rows = (n - 1) * stride + T
    feat = torch.rand(rows + 3, S, 13, generator=g).to(dev)
    series = feat[:rows]
    Ls, _ = series_labels(feat, T, stride, n_windows=n)
    Ls = Ls.contiguous()
    gaps = torch.rand(Ls.shape, generator=g).to(dev) < 0.10
    Lg = torch.where(gaps, torch.full_like(Ls, float("nan")), Ls)

    def fresh():
        m = GCN_GRU(13, 13, 13, S * 13, H, math="f32").to(dev)
        m.load_state_dict(p0)
        return m

    models = {"u": fresh(), "m": fresh(), "g": fresh()}
    tr = {k: TrainStep(m) for k, m in models.items()}
    routes = [("u", lambda: tr["u"].step_series(A, series, Ls, T, stride, n_windows=n)),
              ("m", lambda: tr["m"].step_series(A, series, Ls, T, stride, n_windows=n, missing_labels=True)),
              ("g", lambda: tr["g"].step_series(A, series, Lg, T, stride, n_windows=n, missing_labels=True))]
    t = {name: [] for name, _ in routes}
    for i in range(a.warmup + a.reps):
        for name, step in routes:
            us = timed(step)
            if i >= a.warmup:
                t[name].append(us)
    same = all(torch.equal(p, q) for p, q in zip(models["u"].parameters(), models["m"].parameters()))
    finite = all(bool(torch.isfinite(p).all()) for p in models["g"].parameters())
    med = {name: statistics.median(v) for name, v in t.items()}
    lines = ["S=%d H=%d T=%d n=%d stride=%d math=f32; us per training step; device events: %d alternated steps per route after %d "
             "warm-up steps, medians (min)" % (S, H, T, n, stride, a.reps, a.warmup),
             "series [%d, %d, 13], Ls [%d, %d], %.2f %% of the labels NaN in (g); parameters after %d steps: (m) %s (u)'s bit for "
             "bit; (g) all finite: %s" % (rows, S, Ls.shape[0], H, 100.0 * float(gaps.float().mean()), a.warmup + a.reps,
                                          "equal" if same else "DIFFER FROM", finite)]
    for name, what in (("u", "(u) step_series, unmasked          "), ("m", "(m) missing_labels=True, no NaN    "),
                       ("g", "(g) missing_labels=True, ~10 % NaN ")):
        lines.append("  %s %8.1f (%8.1f)   this / (u) = %.3f" % (what, med[name], min(t[name]), med[name] / med["u"]))
    for name, step in routes:
        lines += ["kernels of one step of (%s) (per-kernel events serialise the launches):" % name] + kernels(step)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if same and finite else 1


if __name__ == "__main__":
    sys.exit(main())
