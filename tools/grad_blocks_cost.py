"""Cost of the blocked gradient exchange on one GPU: TrainStep's step time at BASELINE configs[4]'s per-GPU shape (S = 4096 CSR
8-NN graph, H = 12288, T = 24, B = 128, fp32 I/O) with a one-rank RCCL group, grad_blocks = None (one bucket) against k blocks
per GRU weight.  A one-rank all-reduce moves no bytes between GPUs, so what this measures is the schedule's own cost: the
extra launches, one GEMM tail and one reduction per block, the per-block Adam.  Each setting gets a fresh TrainStep (same
seed) in turn, `--rounds` times, and host wall time over `--steps` synchronised steps after two warm-up steps.

    python tools/grad_blocks_cost.py [--math f16x3] [--blocks 8,16] [--steps 5] [--rounds 2] [--out FILE]
    python tools/grad_blocks_cost.py --trace-step 8     # one warm-up + one step at k = 8 (run it under rocprofv3)
"""
import argparse
import os
import statistics
import sys
import time

import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from windgnn_amd.distributed import ensure_rccl_env  # noqa: E402

S, H, T, B = 4096, 12288, 24, 128


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--math", default="f16x3")
    ap.add_argument("--blocks", default="8,16")
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--trace-step", type=int, default=None)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    ensure_rccl_env()
    from windgnn_amd import GCN_GRU
    from windgnn_amd.graph import CsrAdjacency, build_knn_adjacency, synthetic_station_coords
    from windgnn_amd.trainer import TrainStep
    os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
    os.environ.setdefault("MASTER_PORT", "29533")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    A = CsrAdjacency(*build_knn_adjacency(synthetic_station_coords(S, seed=7), 8)).to(dev)
    g = torch.Generator().manual_seed(0)
    X = torch.rand(B, T, S, 13, generator=g).to(dev)
    L = torch.rand(B, T, H, generator=g).to(dev)

    def trainer(k):
        torch.manual_seed(0)
        with torch.device(dev):
            m = GCN_GRU(13, 13, 13, S * 13, H, math=a.math)
        return TrainStep(m, process_group=dist.group.WORLD, grad_blocks=k)

    if a.trace_step is not None:
        tr = trainer(a.trace_step)
        for _ in range(2):
            tr.step(A, X, L)
        torch.cuda.synchronize()
        print("traced k = %d: %d blocks" % (a.trace_step, len(tr.plan.blocks)))
        dist.destroy_process_group()
        return
    settings = [None] + [int(k) for k in a.blocks.split(",")]
    ms = {k: [] for k in settings}
    losses = {}
    nblocks = {}
    for _ in range(a.rounds):
        for k in settings:
            tr = trainer(k)
            nblocks[k] = len(tr.plan.blocks) if tr.plan is not None else 0
            for _ in range(2):
                tr.step(A, X, L)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                loss, _ = tr.step(A, X, L)
            torch.cuda.synchronize()
            ms[k].append(1e3 * (time.perf_counter() - t0) / a.steps)
            losses[k] = float(loss)
            tr.check()
            del tr, loss
            torch.cuda.empty_cache()
    base = statistics.median(ms[None])
    lines = ["S=%d (CSR 8-NN) H=%d T=%d B=%d, math %s, one-rank RCCL group; %d steps after 2 warm-up, %d rounds; "
             "ms per step, median (all)" % (S, H, T, B, a.math, a.steps, a.rounds)]
    for k in settings:
        med = statistics.median(ms[k])
        lines.append("grad_blocks=%-5s blocks %3d  %8.2f ms  (%s)  %+.2f %%  loss after step %d: %.9g"
                     % (k, nblocks[k], med, ", ".join("%.2f" % x for x in ms[k]), 100.0 * (med / base - 1.0),
                        2 + a.steps, losses[k]))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    dist.destroy_process_group()


if __name__ == "__main__":
    main()
