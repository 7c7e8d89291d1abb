"""Cost of one round of an ensemble -- every one of K = 4 members takes one optimiser step -- by three routes in one process on
one device:

  (a) Ensemble(streams=4)   the members' steps on four side streams, one fork and one join per round
  (b) Ensemble(streams=1)   the same fan-out on ONE side stream: what the fork, the join and the hand-back cost without overlap
  (c) K TrainSteps in a loop on the current stream: what a user does without windgnn_amd.Ensemble -- the yardstick

at S = 34, H = 102, T = 24: step_series in "f32" on the n = 256 / 1024 / 4096 sliding windows of one shared series, and the
materialised step in "f16x3" at B = 256.  Per route and round: device events on the caller's stream around the round (for (a) and
(b) the second event follows the join), and the host clock from the first call to the return of the last (the enqueue time).  The
routes are alternated, their order rotated by one from round to round; medians (minima) of --reps rounds after --warmup.  Then the
wall time per round back to back, and the memory: the side streams' workspaces and the peak of torch's allocator over one round
above what is allocated between rounds (stashes, Y, dY: freed after the step, cached per stream).

    python tools/ensemble_cost.py [--reps 30] [--warmup 5] [--out profiles/r21_ensemble_cost.txt]
"""
import argparse
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from oracle import windgnn_oracle as orc  # noqa: E402
from windgnn_amd import GCN_GRU, Ensemble  # noqa: E402
from windgnn_amd.functional import _Workspace  # noqa: E402
from windgnn_amd.trainer import TrainStep  # noqa: E402
from series_train_cost import host_loop  # noqa: E402

K = 4
ORDER = ("a", "b", "c")
WHAT = {"a": "(a) Ensemble(streams=4)      ", "b": "(b) Ensemble(streams=1)      ", "c": "(c) K TrainSteps in a loop   "}


def models(math, S, H, dev):
    out = []
    for k in range(K):
        m = GCN_GRU(13, 13, 13, S * 13, H, math=math, validate=False).to(dev)
        m.load_state_dict(orc.init_params(S, 13, H, seed=1 + k))
        out.append(m)
    return out


def timed(fn):
    """(device us between two events on the current stream around fn, host us from the call to its return)."""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    t0 = time.perf_counter()
    fn()
    host = 1e6 * (time.perf_counter() - t0)
    e1.record()
    e1.synchronize()
    return 1e3 * e0.elapsed_time(e1), host


def peak_over(fn):
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base


def measure(title, routes, objs, reps, warmup, lines):
    dev_us, host_us = {n: [] for n in ORDER}, {n: [] for n in ORDER}
    for i in range(warmup + reps):
        r = i % len(ORDER)
        for name in ORDER[r:] + ORDER[:r]:
            d, h = timed(routes[name])
            if i >= warmup:
                dev_us[name].append(d)
                host_us[name].append(h)
    med = {n: statistics.median(v) for n, v in dev_us.items()}
    lines.append("%s; us per round of K = %d steps; %d alternated rounds per route after %d warm-up rounds, medians (min)"
                 % (title, K, reps, warmup))
    for n in ORDER:
        lines.append("  %s device %8.1f (%8.1f)   host enqueue %8.1f (%8.1f)   device / (c) = %5.2f   (c) / this = %5.2f x"
                     % (WHAT[n], med[n], min(dev_us[n]), statistics.median(host_us[n]), min(host_us[n]), med[n] / med["c"],
                        med["c"] / med[n]))
    quart = statistics.quantiles(dev_us["c"], n=4)
    lines.append("  noise: (c)'s rounds spread over %.1f .. %.1f us (quartiles %.1f .. %.1f)"
                 % (min(dev_us["c"]), max(dev_us["c"]), quart[0], quart[2]))
    losses = {"a": objs["a"].loss.tolist(), "b": objs["b"].loss.tolist(), "c": [float(t._loss) for t in objs["c"]]}
    lines.append("  losses after %d rounds: %s" % (objs["c"][0].steps, "  ".join("(%s) %s" % (n, " ".join("%.6f" % x for x in v))
                                                                                   for n, v in losses.items())))
    lines.append("  wall time per round, %d back to back: %s" % (reps, "  ".join("(%s) %.1f us" % (n, host_loop(routes[n], reps))
                                                                                 for n in ORDER)))
    ws = {n: objs[n].workspace_bytes() for n in ("a", "b")}
    ws["c"] = _Workspace._bufs[(0, torch.cuda.current_stream().cuda_stream)].numel()
    lines.append("  memory: workspaces (a) %d x side streams = %.1f MiB, (b) %.1f MiB, (c) the current stream's %.1f MiB; peak of one "
                 "round above the resting allocation: %s" % (objs["a"].n_streams, ws["a"] / 2 ** 20, ws["b"] / 2 ** 20, ws["c"] / 2 ** 20,
                                                             "  ".join("(%s) %.1f MiB" % (n, peak_over(routes[n]) / 2 ** 20)
                                                                       for n in ORDER)))


def run(math, S, T, H, n, series_mode, reps, warmup, lines):
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(7)
    A = (torch.rand(S, S, generator=g) / S + 0.01).to(dev)
    objs = {"a": Ensemble(models(math, S, H, dev), streams=4, check_every=0),
            "b": Ensemble(models(math, S, H, dev), streams=1, check_every=0),
            "c": [TrainStep(m, check_every=0) for m in models(math, S, H, dev)]}
    if series_mode:
        rows = n + T - 1
        series = torch.rand(rows, S, 13, generator=g).to(dev)
        Ls = torch.rand(rows, H, generator=g).to(dev)

        def looped():
            for tr in objs["c"]:
                tr.step_series(A, series, Ls, T)
        routes = {"a": lambda: objs["a"].step_series(A, series, Ls, T), "b": lambda: objs["b"].step_series(A, series, Ls, T),
                  "c": looped}
        title = "series mode (step_series), math=%s S=%d H=%d T=%d, %d windows per member of one shared series" % (math, S, H, T, n)
    else:
        X = torch.rand(n, T, S, 13, generator=g).to(dev)
        L = torch.rand(n, T, H, generator=g).to(dev)

        def looped():
            for tr in objs["c"]:
                tr.step(A, X, L)
        routes = {"a": lambda: objs["a"].step(A, X, L), "b": lambda: objs["b"].step(A, X, L), "c": looped}
        title = "materialised windows (step), math=%s S=%d H=%d T=%d B=%d per member, shared" % (math, S, H, T, n)
    measure(title, routes, objs, reps, warmup, lines)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["hardware queues: GPU_MAX_HW_QUEUES=%s (unset: HIP's default, 4)" % os.environ.get("GPU_MAX_HW_QUEUES", "unset"), ""]
    for n in (256, 1024, 4096):
        run("f32", 34, 24, 102, n, True, a.reps, a.warmup, lines)
        lines.append("")
    run("f16x3", 34, 24, 102, 256, False, a.reps, a.warmup, lines)
    text = "\n".join(lines)
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
