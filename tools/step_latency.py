"""Hourly forecast latency with a carried state: StreamingForecaster.push (one hour, wgnn_fwd_state with T = 1) against
data.forward_last of a T = 168 prefix (the re-run a stateless forecaster needs), S = 34, H = 102, in f32 and f16x3, at
B = 1 and B = 64 streams.  Times come from device events around N calls after warm-up (and a synchronise); the kernel
time of the step is read from the library's own per-launch events (wgnn_profile_*).

    python tools/step_latency.py [--out profiles/r6_step_latency.txt] [--rocprof DIR]

--rocprof DIR: afterwards run this script once more, as a fresh child process under
`rocprofv3 --kernel-trace --stats`, and copy its kernel statistics next to --out (r6_step_kernel_stats.csv)."""
import argparse
import glob
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from bench import adjacency_34  # noqa: E402
from windgnn_amd import GCN_GRU, StreamingForecaster, _lib  # noqa: E402
from windgnn_amd.data import forward_last  # noqa: E402

S, H, T = 34, 102, 168


def timed(fn, n):
    """Mean device time per call of n back-to-back calls (events on the current stream), after 20 warm-up calls."""
    for _ in range(20):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / n * 1e3


def kernels(fn, n):
    """{kernel: us per call} of the library's launches inside fn (hipEvent-bracketed: adds ~2 us per launch)."""
    fn()
    torch.cuda.synchronize()
    _lib.profile_enable(True)
    for _ in range(n):
        fn()
    torch.cuda.synchronize()
    recs = _lib.profile_read()
    _lib.profile_enable(False)
    return {r["name"]: (r["ms"] / n * 1e3, r["launches"] / n) for r in recs}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r6_step_latency.txt"))
    ap.add_argument("--rocprof", default=None, help="scratch directory for a rocprofv3 --kernel-trace --stats child run")
    ap.add_argument("--n", type=int, default=200)
    a = ap.parse_args(argv)
    dev = torch.device("cuda:0")
    A = adjacency_34().to(dev)
    g = torch.Generator().manual_seed(3)
    lines = ["# tools/step_latency.py: S = %d, H = %d; device time per call (events, %d calls after 20 warm-up calls)" % (S, H, a.n),
             "# push = StreamingForecaster.push (one hour); prefix = data.forward_last of a T = %d window (stateless re-run)" % T]
    with torch.no_grad():
        for math in ("f32", "f16x3"):
            m = GCN_GRU(13, 13, 13, S * 13, H, math=math, validate=False).to(dev)   # validate=False: no per-call sync
            m.requires_grad_(False)
            for B in (1, 64):
                x = torch.rand(B, S, 13, generator=g).to(dev)
                Xp = torch.rand(B, T, S, 13, generator=g).to(dev)
                fc = StreamingForecaster(m, A, 0.0, 20.0, n_streams=B, window=None)
                push_us = timed(lambda: fc.push(x), a.n)
                pre_us = timed(lambda: forward_last(m, A, Xp, 0.0, 20.0), max(20, a.n // 4))
                kp = kernels(lambda: fc.push(x), a.n)
                kf = kernels(lambda: forward_last(m, A, Xp, 0.0, 20.0), max(20, a.n // 4))
                step = kp.get("gru_step_kernel", (float("nan"), 0))
                lines.append("%-6s B=%-3d push %7.1f us  prefix(T=%d) %7.1f us  ratio %5.1fx | push kernels: %s | prefix kernels: %s" % (
                    math, B, push_us, T, pre_us, pre_us / push_us,
                    ", ".join("%s %.1f us x%.0f" % (k, v[0], v[1]) for k, v in sorted(kp.items())),
                    ", ".join("%s %.1f us" % (k, v[0]) for k, v in sorted(kf.items(), key=lambda kv: -kv[1][0]))))
                print(lines[-1], flush=True)
                assert step[1] == 1, kp               # one step launch per push
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    if a.rocprof:
        d = a.rocprof
        os.makedirs(d, exist_ok=True)
        cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", d, "-o", "step", "--",
               sys.executable, os.path.abspath(__file__), "--out", os.path.join(d, "under_rocprof.txt"), "--n", "50"]
        print(" ".join(cmd), flush=True)
        subprocess.run(cmd, check=True, timeout=600)
        stats = sorted(glob.glob(os.path.join(d, "**", "*kernel_stats.csv"), recursive=True))
        if not stats:
            raise RuntimeError("rocprofv3 wrote no kernel_stats.csv under %s" % d)
        dst = os.path.join(os.path.dirname(a.out), "r6_step_kernel_stats.csv")
        shutil.copyfile(stats[-1], dst)
        print("kernel statistics -> %s" % dst)


if __name__ == "__main__":
    main()
