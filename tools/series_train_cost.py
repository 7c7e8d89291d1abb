"""Cost of one TRAINING step on the sliding windows of a series, three routes on the SAME windows, in one process on one device:

  (a) fused series    TrainStep.step_series(adj, series, Ls, T, stride): wgnn_series_fwd_loss + wgnn_series_bwd_mse + wgnn_finish
  (b) materialised    make_windows(feat, T, starts=...) once, then TrainStep.step(adj, X, L) per step (exact fp32)
  (c) unfused series  GCN_GRU.forward_series + nn.MSELoss on series_labels' window view + loss.backward() + torch.optim.Adam

at S = 34, H = 102, T = 24, n = 4096 windows, stride 1, 4 and 24, math = "f32".  Every route starts from the same parameters and
takes the same number of steps.  Two clocks: device events around each step with the three routes alternated (medians and minima
of --reps steps after --warmup), and a host clock around --reps back-to-back steps of one route that end in one device
synchronise (what a training loop pays, launch overhead of the framework's own kernels included).  Then the library's
per-kernel tally of one step of (a) at each stride.

    python tools/series_train_cost.py [--reps 30] [--warmup 5] [--n 4096] [--out FILE]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import windgnn_oracle as orc  # noqa: E402
from windgnn_amd import GCN_GRU, _lib  # noqa: E402
from windgnn_amd.data import make_windows  # noqa: E402
from windgnn_amd.series import series_labels  # noqa: E402
from windgnn_amd.trainer import TrainStep  # noqa: E402


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1)


def host_loop(fn, reps):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return 1e6 * (time.perf_counter() - t0) / reps


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
    p0 = orc.init_params(S, 13, H, seed=1)
    lines = ["S=%d H=%d T=%d n=%d math=f32; us per training step; device events: %d alternated steps per route after %d warm-up "
             "steps, medians (min); host clock: %d back-to-back steps ending in one synchronise"
             % (S, H, T, n, a.reps, a.warmup, a.reps)]
    tally = []
    for stride in (1, 4, 24):
        rows = (n - 1) * stride + T
        feat = torch.rand(rows + 3, S, 13, generator=g).to(dev)
        series = feat[:rows]
        Ls, Lview = series_labels(feat, T, stride, n_windows=n)
        starts = [w * stride for w in range(n)]
        X, L = make_windows(feat, T, starts=starts)
        assert torch.equal(Lview, L)                                   # the label view IS the materialised labels

        def fresh():
            m = GCN_GRU(13, 13, 13, S * 13, H, math="f32").to(dev)
            m.load_state_dict(p0)
            return m

        ma, mb, mc = fresh(), fresh(), fresh()
        tra, trb = TrainStep(ma), TrainStep(mb)
        opt = torch.optim.Adam(mc.parameters(), lr=1e-3)
        loss_fn = torch.nn.MSELoss()

        def step_a():
            tra.step_series(A, series, Ls, T, stride, n_windows=n)

        def step_b():
            trb.step(A, X, L)

        def step_c():
            opt.zero_grad(set_to_none=True)
            loss_fn(mc.forward_series(A, series, T, stride, n_windows=n), Lview).backward()
            opt.step()

        routes = [("a", step_a), ("b", step_b), ("c", step_c)]
        t = {name: [] for name, _ in routes}
        for i in range(a.warmup + a.reps):
            for name, step in routes:
                us = timed(step)
                if i >= a.warmup:
                    t[name].append(us)
        # same numbers: after the same steps from the same start the three routes hold the same parameters
        worst = {name: max(float((p - q).abs().max() / q.abs().max()) for p, q in zip(m.parameters(), ma.parameters()))
                 for name, m in (("b", mb), ("c", mc))}
        host = {name: host_loop(step, a.reps) for name, step in routes}
        lines.append("stride %d: series [%d, %d, 13] = %.1f MB, Ls [%d, %d] = %.1f MB, windows X + L = %.1f MB; parameters after "
                     "%d steps: (b) within %.1e, (c) within %.1e of (a)'s, relative to max"
                     % (stride, rows, S, series.numel() * 4e-6, Ls.shape[0], H, Ls.numel() * 4e-6,
                        (X.numel() + L.numel()) * 4e-6, a.warmup + a.reps, worst["b"], worst["c"]))
        med = {name: statistics.median(v) for name, v in t.items()}
        for name, what in (("a", "(a) step_series          "), ("b", "(b) step on windows      "), ("c", "(c) unfused series route ")):
            lines.append("  %s events %8.1f (%8.1f)   host clock %8.1f   (a) / this = %.3f events, %.3f host"
                         % (what, med[name], min(t[name]), host[name], med["a"] / med[name], host["a"] / host[name]))
        tally += ["kernels of one step of (a) at stride %d (per-kernel events serialise the launches):" % stride] + kernels(step_a)
        del X, L, feat, series, Ls, Lview
    text = "\n".join(lines + tally)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
