"""Cost of one series VALIDATION pass (include/windgnn_series_val.h) against the two routes that bracket it, on the SAME windows,
in one process on one device:

  (v)  validate           TrainStep.validate_series(adj, series, Ls, T, 1): one call that opens and closes a pass
  (v') validate again     the same call on a second TrainStep: the spread of the route's single calls across the alternations,
                          and the distance of the two medians, are the run's two noise figures
  (b)  validate + best    the same under TrainStep(keep_best=True, best_on="validation"): wgnn_keep_best's two launches more
  (t)  training pair      TrainStep.forward_backward_series of the same run: the only fused way to this loss before
  (f)  floor              series.forward_last_series: the same launches minus the label reads and the finish

at S = 34, H = 102, T = 24, n = 4096 windows, stride 1, math = "f32", MSE from step 0.  The clock is device events around each
call with the routes alternated (medians and minima of --reps calls after --warmup); then the wall time per call of each route
called back to back, the library's per-kernel tally of one call of each route, and the bytes: the validation workspace against
the training pair's workspace + stash.  (v)'s loss word must equal (t)'s bit for bit.

    python tools/series_val_cost.py [--reps 30] [--warmup 5] [--n 4096] [--out profiles/r16_series_val_cost.txt]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import windgnn_oracle as orc  # noqa: E402
from windgnn_amd import GCN_GRU, _lib  # noqa: E402
from windgnn_amd.series import forward_last_series, series_labels  # noqa: E402
from windgnn_amd.trainer import TrainStep  # noqa: E402
from series_train_cost import host_loop, kernels, timed  # noqa: E402


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

    def fresh():
        m = GCN_GRU(13, 13, 13, S * 13, H, math="f32").to(dev)
        m.load_state_dict(p0)
        return m

    order = ["v", "b", "t", "f", "v'"]
    models = {k: fresh() for k in order}
    tr = {k: TrainStep(m, **({"keep_best": True, "best_on": "validation"} if k == "b" else {})) for k, m in models.items()}
    routes = {k: (lambda k=k: tr[k].validate_series(A, series, Ls, T, stride, n_windows=n)) for k in ("v", "v'", "b")}
    routes["t"] = lambda: tr["t"].forward_backward_series(A, series, Ls, T, stride, n_windows=n)
    routes["f"] = lambda: forward_last_series(models["f"], A, series, T, 0.0, 1.0, stride, n)
    t = {name: [] for name in order}
    for i in range(a.warmup + a.reps):
        for name in order:
            us = timed(routes[name])
            if i >= a.warmup:
                t[name].append(us)
    same = torch.equal(tr["v"].val_loss, tr["t"]._loss) and torch.equal(tr["v"].val_loss, tr["b"].val_loss)
    med = {name: statistics.median(v) for name, v in t.items()}
    both = t["v"] + t["v'"]
    quart = statistics.quantiles(both, n=4)
    sd = _lib.SeriesDims(rows, T, stride, n, S, 13, H, 0, 0, 0, 0)
    lib = _lib.load()
    ws_val = lib.wgnn_series_val_workspace_bytes(C.byref(sd))
    ws_train, st_train = lib.wgnn_series_workspace_bytes(C.byref(sd)), lib.wgnn_series_stash_bytes(C.byref(sd))
    lines = ["S=%d H=%d T=%d n=%d stride=%d math=f32, MSE from step 0; us per call; device events: %d alternated calls per route after "
             "%d warm-up calls, medians (min)" % (S, H, T, n, stride, a.reps, a.warmup),
             "series [%d, %d, 13], Ls [%d, %d]; the loss word of (v) %s (t)'s and (b)'s bit for bit (%.9g)"
             % (rows, S, Ls.shape[0], H, "equals" if same else "DIFFERS FROM", float(tr["v"].val_loss)),
             "noise, two figures: (v)'s %d single calls across the alternations spread over %.1f us (%.1f .. %.1f, quartiles "
             "%.1f .. %.1f); the medians of its two instances differ by %.1f us"
             % (len(both), max(both) - min(both), min(both), max(both), quart[0], quart[2], abs(med["v"] - med["v'"]))]
    for name, what in (("v", "(v)  validate_series                    "), ("v'", "(v') the same, second instance          "),
                       ("b", "(b)  validate_series, best_on=validation"), ("t", "(t)  forward_backward_series            "),
                       ("f", "(f)  forward_last_series (the floor)    ")):
        lines.append("  %s %8.1f (%8.1f)   this - (v) = %+7.1f us   this / (t) = %.3f"
                     % (what, med[name], min(t[name]), med[name] - med["v"], med[name] / med["t"]))
    lines.append("wall time per call, %d calls back to back (launch-bound where it exceeds the kernels' sum):" % a.reps)
    for name in order[:-1]:
        lines.append("  (%s) %8.1f us" % (name, host_loop(routes[name], a.reps)))
    lines.append("bytes: validation workspace %d (%.1f MB), no stash; training pair workspace %d + stash %d = %d (%.1f MB)"
                 % (ws_val, ws_val / 1e6, ws_train, st_train, ws_train + st_train, (ws_train + st_train) / 1e6))
    for name in order[:-1]:
        lines += ["kernels of one call of (%s) (per-kernel events serialise the launches):" % name] + kernels(routes[name])
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
