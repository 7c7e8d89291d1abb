"""Cost of series mode (include/windgnn_series.h) against the materialised path on the SAME windows, in one process on one device:

  step      GCN_GRU.forward_series(adj, series, T, stride) + Y.backward(dY)
            against make_windows(series, T, starts=...) once, then GCN_GRU.forward(adj, X) + Y.backward(dY) per step
  backtest  forward_last_series against forward_last on the materialised windows

at S = 34, H = 102, T = 24, n = 4096 windows, stride 1, 4 and 24, math = "f32".  Device events around each call, the two paths
alternated, medians of --reps calls after --warmup; the materialised path's window copy is timed apart (it is paid once per
epoch order, not per step).  Then the library's per-kernel tally of one step of each path at stride 1.

    python tools/series_cost.py [--reps 30] [--warmup 5] [--n 4096] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import windgnn_oracle as orc  # noqa: E402
from windgnn_amd import GCN_GRU, _lib  # noqa: E402
from windgnn_amd.data import forward_last, make_windows  # noqa: E402
from windgnn_amd.series import forward_last_series  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1)


def kernels(fn):
    _lib.profile_enable(True)
    before = {k["name"]: (k["launches"], k["ms"]) for k in _lib.profile_read()}
    fn()
    torch.cuda.synchronize()
    after = _lib.profile_read()
    _lib.profile_enable(False)
    out = []
    for k in after:
        n0, ms0 = before.get(k["name"], (0, 0.0))
        if k["launches"] - n0:
            out.append("    %-34s x%d %8.1f us" % (k["name"], k["launches"] - n0, 1e3 * (k["ms"] - ms0)))
    return out


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
    model = GCN_GRU(13, 13, 13, S * 13, H, math="f32").to(dev)
    model.load_state_dict(orc.init_params(S, 13, H, seed=1))
    dY = (torch.rand(n, T, H, generator=g) * 2 - 1).to(dev) * 1e-3
    lines = ["S=%d H=%d T=%d n=%d math=f32; device events, %d alternated calls per path after %d warm-up calls; medians (min) "
             "in us" % (S, H, T, n, a.reps, a.warmup)]
    tally = []
    for stride in (1, 4, 24):
        rows = (n - 1) * stride + T
        feat = torch.rand(rows + 3, S, 13, generator=g).to(dev)          # +3: make_windows also builds the labels
        series = feat[:rows]
        starts = [w * stride for w in range(n)]
        X, _ = make_windows(feat, T, starts=starts)
        t_copy = statistics.median(timed(lambda: make_windows(feat, T, starts=starts)) for _ in range(5))

        def step_series():
            model.zero_grad(set_to_none=True)
            model.forward_series(A, series, T, stride, n_windows=n).backward(dY)

        def step_mat():
            model.zero_grad(set_to_none=True)
            model(A, X).backward(dY)

        def last_series():
            with torch.no_grad():
                forward_last_series(model, A, series, T, 0.0, 30.0, stride, n_windows=n)

        def last_mat():
            with torch.no_grad():
                forward_last(model, A, X, 0.0, 30.0)

        # same numbers first: the two paths agree on Y and on the gradients
        step_mat()
        gm = [p.grad.clone() for p in model.parameters()]
        step_series()
        worst = max(float((p.grad - q).abs().max() / q.abs().max()) for p, q in zip(model.parameters(), gm))
        forms = [("series", step_series, last_series), ("materialised", step_mat, last_mat)]
        t = {(name, k): [] for name, _, _ in forms for k in ("step", "last")}
        for i in range(a.warmup + a.reps):
            for name, step, last in forms:
                ts, tl = timed(step), timed(last)
                if i >= a.warmup:
                    t[(name, "step")].append(ts)
                    t[(name, "last")].append(tl)
        lines.append("stride %d: series [%d, %d, 13] = %.1f MB against windows [%d, %d, %d, 13] = %.1f MB (%.1fx); gradients "
                     "agree to %.1e of max; window copy %.0f us (once, not in the step)"
                     % (stride, rows, S, series.numel() * 4e-6, n, T, S, X.numel() * 4e-6, X.numel() / series.numel(), worst,
                        t_copy))
        for k, what in (("step", "forward + backward"), ("last", "forward_last     ")):
            ms, mm = statistics.median(t[("series", k)]), statistics.median(t[("materialised", k)])
            lines.append("  %s  series %8.1f (%8.1f)   materialised %8.1f (%8.1f)   series / materialised = %.3f"
                         % (what, ms, min(t[("series", k)]), mm, min(t[("materialised", k)]), ms / mm))
        if stride == 1:
            tally = (["kernels of one step at stride 1, series (per-kernel events serialise the launches):"] + kernels(step_series)
                     + ["kernels of one step at stride 1, materialised:"] + kernels(step_mat))
        del X, feat, series
    text = "\n".join(lines + tally)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
