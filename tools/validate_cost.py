"""Cost of one validation call on MATERIALISED windows (TrainStep.validate) against the calls that bracket it, on the same
windows, in one process on one device, per math mode ("f32", "f16x3"):

  (v)  validate            TrainStep.validate(adj, X, L): one call that opens and closes a pass, MSE from step 0
  (l)  validate, last step the same with loss_from = T - 1: wgnn_fwd_last and the terms of B * H entries
  (f)  floor               the stash-less forward of the same run, model(adj, X) under torch.no_grad()
  (s)  training step       TrainStep.step(adj, X, L) on a second model
  (vs) validate_series     "f32" only: the same windows as the stride-1 windows of their series (wgnn_series_val)

at S = 34, H = 102, T = 24, B = 4096.  The clock is device events around each call with the routes alternated (medians and minima
of --reps calls after --warmup).  The reduction's share is ((v) - (f)) / (f).  Then the wall time per call back to back, the
library's per-kernel tally of one call of (v) and (l), and torch's own launches of one (v) as torch.profiler names them.
--c5: one BASELINE configs[4]-shaped call as well (S = 4096 8-NN in CSR, H = 12288, T = 24, B = 128, "f16x3"; --c5-reps calls).

    python tools/validate_cost.py [--reps 30] [--warmup 5] [--B 4096] [--c5 | --c5-only] [--out profiles/r17_validate_cost.txt]
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
from windgnn_amd.data import make_windows  # noqa: E402
from windgnn_amd.series import series_labels  # noqa: E402
from windgnn_amd.trainer import TrainStep  # noqa: E402
from series_train_cost import host_loop, kernels, timed  # noqa: E402


def torch_launches(fn):
    """torch's own device kernels of one call of fn, as torch.profiler names them: ["name xN  us"], or a note."""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        rows = [e for e in prof.key_averages() if getattr(e, "device_time_total", 0) > 0]
        rows.sort(key=lambda e: -e.device_time_total)
        return ["    %-110.110s x%d %8.1f us" % (e.key, e.count, e.device_time_total) for e in rows] or ["    (no device rows)"]
    except Exception as e:       # a build of torch without the device tracer
        return ["    unmeasured: torch.profiler gave no device rows here (%s: %s)" % (type(e).__name__, e)]


def shape_run(math, S, T, H, B, reps, warmup, lines):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    A = (torch.rand(S, S, generator=g) / S + 0.01).to(dev)
    p0 = orc.init_params(S, 13, H, seed=1)
    rows = B - 1 + T
    feat = torch.rand(rows + 3, S, 13, generator=g).to(dev)
    series = feat[:rows]
    Ls = series_labels(feat, T, 1, n_windows=B)[0].contiguous()
    X, L = make_windows(feat, T, starts=list(range(B)))

    def fresh():
        m = GCN_GRU(13, 13, 13, S * 13, H, math=math, validate=False).to(dev)
        m.load_state_dict(p0)
        return m
    order = ["v", "l", "f", "s"] + (["vs"] if math == "f32" else [])
    models = {k: fresh() for k in order}
    tr = {k: TrainStep(models[k]) for k in order if k != "f"}

    def floor():
        with torch.no_grad():
            return models["f"](A, X)
    routes = {"v": lambda: tr["v"].validate(A, X, L), "l": lambda: tr["l"].validate(A, X, L, loss_from=T - 1), "f": floor,
              "s": lambda: tr["s"].step(A, X, L)}
    if math == "f32":
        routes["vs"] = lambda: tr["vs"].validate_series(A, series, Ls, T, 1, n_windows=B)
    t = {name: [] for name in order}
    for i in range(warmup + reps):
        for name in order:
            us = timed(routes[name])
            if i >= warmup:
                t[name].append(us)
    med = {name: statistics.median(v) for name, v in t.items()}
    quart = statistics.quantiles(t["v"], n=4)
    what = {"v": "(v)  validate                  ", "l": "(l)  validate, loss_from = T-1 ", "f": "(f)  forward, no stash (floor) ",
            "s": "(s)  TrainStep.step            ", "vs": "(vs) validate_series           "}
    lines.append("math=%s S=%d H=%d T=%d B=%d, MSE; us per call; device events: %d alternated calls per route after %d warm-up "
                 "calls, medians (min)" % (math, S, H, T, B, reps, warmup))
    lines.append("noise: (v)'s %d single calls spread over %.1f us (%.1f .. %.1f, quartiles %.1f .. %.1f)"
                 % (len(t["v"]), max(t["v"]) - min(t["v"]), min(t["v"]), max(t["v"]), quart[0], quart[2]))
    for name in order:
        lines.append("  %s %8.1f (%8.1f)   this - (f) = %+8.1f us   this / (f) = %.3f   this / (s) = %.3f"
                     % (what[name], med[name], min(t[name]), med[name] - med["f"], med[name] / med["f"], med[name] / med["s"]))
    lines.append("the reduction (fp64 terms + the record's words): (v) - (f) = %.1f us = %.1f %% of the floor; at the last step alone "
                 "(l) - (f) = %+.1f us" % (med["v"] - med["f"], 100.0 * (med["v"] - med["f"]) / med["f"], med["l"] - med["f"]))
    if math == "f32":
        lines.append("the record's mean: (v) %.9g, (vs) %.9g (another forward and another summation: not the same bits)"
                     % (float(tr["v"]._val_word("val_loss", "mean")), float(tr["vs"]._val_word("val_loss", "mean"))))
    lines.append("wall time per call, %d calls back to back (launch-bound where it exceeds the device time):" % reps)
    for name in order:
        lines.append("  (%s) %8.1f us" % (name, host_loop(routes[name], reps)))
    for name in ("v", "l"):
        lines += ["the library's kernels of one call of (%s) (per-kernel events serialise the launches):" % name] + kernels(routes[name])
    lines += ["torch's device kernels of one call of (v), by torch.profiler:"] + torch_launches(routes["v"])


def c5_run(reps, lines):
    from windgnn_amd.graph import CsrAdjacency, build_knn_adjacency, synthetic_station_coords
    dev = torch.device("cuda:0")
    S, T, B, H = 4096, 24, 128, 12288
    csr = CsrAdjacency(*build_knn_adjacency(synthetic_station_coords(S, seed=7), 8)).to(dev)
    torch.manual_seed(11)
    with torch.device(dev):
        model = GCN_GRU(13, 13, 13, S * 13, H, math="f16x3", validate=False)
        X = torch.rand(B, T, S, 13) * (34.0 / S)
        L = torch.rand(B, T, H)
    tr = TrainStep(model)

    def floor():
        with torch.no_grad():
            return model(csr, X)
    routes = {"v": lambda: tr.validate(csr, X, L), "f": floor}
    t = {"v": [], "f": []}
    for i in range(1 + reps):
        for name in ("v", "f"):
            us = timed(routes[name])
            if i >= 1:
                t[name].append(us)
    mv, mf = statistics.median(t["v"]), statistics.median(t["f"])
    lines.append("configs[4]-shaped: S=%d (8-NN, CSR) H=%d T=%d B=%d math=f16x3; %d alternated calls after 1 warm-up, medians (min)"
                 % (S, H, T, B, reps))
    lines.append("  (v)  validate                  %10.1f (%10.1f) us" % (mv, min(t["v"])))
    lines.append("  (f)  forward, no stash (floor) %10.1f (%10.1f) us" % (mf, min(t["f"])))
    lines.append("  the reduction: (v) - (f) = %+.1f us = %+.2f %% of the floor; held-out loss %.9g over %d entries"
                 % (mv - mf, 100.0 * (mv - mf) / mf, float(tr.val_loss), int(tr.val_count)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--B", type=int, default=4096)
    ap.add_argument("--c5", action="store_true")
    ap.add_argument("--c5-reps", type=int, default=5)
    ap.add_argument("--c5-only", action="store_true", help="the configs[4]-shaped call alone; --out is appended to")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = []
    for math in () if a.c5_only else ("f32", "f16x3"):
        shape_run(math, 34, 24, 102, a.B, a.reps, a.warmup, lines)
        lines.append("")
    if a.c5 or a.c5_only:
        c5_run(a.c5_reps, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a" if a.c5_only else "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
