"""What running the front end on the covered hours only (compact=) saves a series step on a table of starts, in one process on one
device, at S = 34, H = 102, T = 24, rows = 26 304 (three years of hourly rows), math = "f32".  Per table -- n random starts, and
one contiguous fifth of the series (a k-fold block) --

  (F)  TrainStep.step_series(starts=table)                      compact=False, twice: two identical instances F and F'
  (H)  TrainStep.step_series(starts=host table, compact=True)   compacted on the host to exactly the covered hours
  (D)  TrainStep.step_series(starts=device table, compact=True) compacted on the device to min(rows, n T) rows
  (W)  TrainStep.step on make_windows of the same windows       (materialised once, outside the clock)
  (V)  TrainStep.validate_series(starts=table)                  compact=False, and (VH) compact=True on the host table

Device events around each step, medians of --reps steps after --warmup, the routes alternated and their order rotated from round
to round; a host clock around --reps back-to-back steps of one route ending in one synchronise.  |F - F'| is the noise yardstick:
compaction pays at a coverage rows_c / rows where a compacted route's median is below min(F, F') by more than it.  theta is the
largest coverage of the sweep up to which that holds for (H) and for (D) without a break.  Then the front stash and workspace bytes
with and without compaction, from the size queries.

    python tools/series_compact_cost.py [--reps 30] [--warmup 5] [--out FILE]
"""
import argparse
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import windgnn_oracle as orc  # noqa: E402
from tools.series_train_cost import host_loop, timed  # noqa: E402
from windgnn_amd import GCN_GRU, _lib  # noqa: E402
from windgnn_amd.data import make_windows  # noqa: E402
from windgnn_amd.series import compact_table, series_labels  # noqa: E402
from windgnn_amd.trainer import TrainStep  # noqa: E402

S, T, H, ROWS = 34, 24, 102, 26304


def sizes(rows, n):
    lib = _lib.load()
    sd = _lib.SeriesDims(rows, T, 0, n, S, 13, H, 0, 0, 0, 0)
    return lib.wgnn_series_at_stash_bytes(C.byref(sd)), lib.wgnn_series_at_workspace_bytes(C.byref(sd))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    g = torch.Generator().manual_seed(5)
    A = (torch.rand(S, S, generator=g) / S + 0.01).to(dev)
    p0 = orc.init_params(S, 13, H, seed=1)
    feat = torch.rand(ROWS + 3, S, 13, generator=g).to(dev)
    series, Ls = feat[:ROWS].contiguous(), series_labels(feat, T, 1, n_windows=1)[0]
    assert Ls.shape[0] == ROWS

    def fresh():
        m = GCN_GRU(13, 13, 13, S * 13, H, math="f32").to(dev)
        m.load_state_dict(p0)
        return TrainStep(m)

    def measure(host_table, windows=True):
        n = len(host_table)
        dev_table = torch.from_numpy(host_table).to(dev)
        m = compact_table(np.sort(host_table), ROWS, T).rows_c
        rows_d = min(ROWS, n * T)
        tr = {k: fresh() for k in ("F", "F'", "H", "D", "W", "V", "VH")}
        routes = [("F", lambda: tr["F"].step_series(A, series, Ls, T, starts=host_table)),
                  ("F'", lambda: tr["F'"].step_series(A, series, Ls, T, starts=host_table)),
                  ("H", lambda: tr["H"].step_series(A, series, Ls, T, starts=host_table, compact=True)),
                  ("D", lambda: tr["D"].step_series(A, series, Ls, T, starts=dev_table, compact=True)),
                  ("V", lambda: tr["V"].validate_series(A, series, Ls, T, starts=host_table)),
                  ("VH", lambda: tr["VH"].validate_series(A, series, Ls, T, starts=host_table, compact=True))]
        if windows:
            X, L = make_windows(feat, T, starts=host_table.tolist())
            routes.append(("W", lambda: tr["W"].step(A, X, L)))
        t = {name: [] for name, _ in routes}
        for i in range(a.warmup + a.reps):
            k = i % len(routes)
            for name, step in routes[k:] + routes[:k]:          # the order rotates from round to round
                us = timed(step)
                if i >= a.warmup:
                    t[name].append(us)
        med = {name: statistics.median(v) for name, v in t.items()}
        host = {name: host_loop(step, a.reps) for name, step in routes}
        apart = max(float((p.detach() - q.detach()).abs().max() / q.detach().abs().max())
                    for p, q in zip(tr["H"].model.parameters(), tr["F"].model.parameters()))
        return dict(n=n, m=m, rows_d=rows_d, med=med, host=host, apart=apart)

    rng = np.random.default_rng(22)
    lines = ["S=%d H=%d T=%d rows=%d math=f32; us per call; device events: medians of %d alternated steps per route after %d warm-up "
             "steps, the order of the routes rotated from round to round; (host clock: %d back-to-back calls ending in one synchronise)"
             % (S, H, T, ROWS, a.reps, a.warmup, a.reps),
             "F, F': step_series(starts=), compact=False, two identical instances; H: compact=True on a host table (rows_c = m); "
             "D: compact=True on a device table (rows_c = min(rows, n T)); W: TrainStep.step on make_windows of the same windows; "
             "V / VH: validate_series with compact=False / True (host table)", ""]
    sweep = []
    for label, n in (("random", 128), ("random", 256), ("random", 512), ("random", 1024), ("random", 2048), ("random", 4096),
                     ("random", 8192), ("fifth", (ROWS // 5 - T + 1))):
        if label == "random":
            table = rng.integers(0, ROWS - T + 1, size=n).astype(np.int64)
        else:
            table = np.arange(2 * (ROWS // 5), 2 * (ROWS // 5) + n, dtype=np.int64)      # the third of five blocks
        q = measure(table, windows=n <= 6000)
        q["label"] = label
        sweep.append(q)
        med, host = q["med"], q["host"]
        yard = abs(med["F"] - med["F'"])
        base = min(med["F"], med["F'"])
        lines.append("%s n=%d: covered m=%d (%.3f of the rows), device-table rows_c=%d (%.3f); yardstick |F - F'| = %.1f us; after "
                     "%d steps H's parameters are within %.1e of F's (relative to max)"
                     % (label, q["n"], q["m"], q["m"] / ROWS, q["rows_d"], q["rows_d"] / ROWS, yard, a.warmup + a.reps, q["apart"]))
        for name in ("F", "F'", "H", "D", "W", "V", "VH"):
            if name in med:
                lines.append("    %-3s events %8.1f   (host clock %8.1f)%s"
                             % (name, med[name], host[name],
                                "" if name not in ("H", "D") else "   %+8.1f us, %.2f x against min(F, F')%s"
                                % (med[name] - base, base / med[name], "" if base - med[name] > yard else "   (inside the yardstick)")))
        lines.append("    VH against V: %+.1f us, %.2f x" % (med["VH"] - med["V"], med["V"] / med["VH"]))
    # theta: the largest coverage up to which both compacted routes beat min(F, F') by more than the yardstick, without a break
    theta = {}
    for route, cover in (("H", lambda q: q["m"] / ROWS), ("D", lambda q: q["rows_d"] / ROWS)):
        theta[route] = 0.0
        for q in sorted((q for q in sweep if q["label"] == "random"), key=cover):
            med = q["med"]
            if cover(q) >= 1.0 or min(med["F"], med["F'"]) - med[route] <= abs(med["F"] - med["F'"]):
                break
            theta[route] = cover(q)
    lines += ["", "theta: compaction pays up to rows_c / rows = %.3f on a host table and %.3f on a device table (the largest coverage "
              "of the sweep below which the compacted median is under min(F, F') by more than |F - F'|, without a break); "
              "compact='auto' takes each for its own kind of table, rounded down to two digits: %.2f and %.2f"
              % (theta["H"], theta["D"], int(100 * theta["H"]) / 100.0, int(100 * theta["D"]) / 100.0), ""]
    lines.append("front stash and workspace bytes (wgnn_series_at_stash_bytes / wgnn_series_at_workspace_bytes):")
    for q in sweep:
        full, host_c, dev_c = sizes(ROWS, q["n"]), sizes(q["m"], q["n"]), sizes(q["rows_d"], q["n"])
        lines.append("    %s n=%d: stash %.1f MB -> %.1f MB (host table) / %.1f MB (device table); workspace %.1f MB -> %.1f MB / %.1f MB; "
                     "the gathered series and labels add %.1f MB / %.1f MB"
                     % (q["label"], q["n"], full[0] / 1e6, host_c[0] / 1e6, dev_c[0] / 1e6, full[1] / 1e6, host_c[1] / 1e6,
                        dev_c[1] / 1e6, q["m"] * (S * 13 + H) * 4e-6, q["rows_d"] * (S * 13 + H) * 4e-6))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
