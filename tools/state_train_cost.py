"""Cost of training through a carried state: wgnn_fwd_state_stash + wgnn_bwd_state_part (random h0, dh_n, dh0 written)
against wgnn_fwd + wgnn_bwd_part at bench.py's shape (S = 34, T = 24, B = 4096), per math mode.  Device events around each
pair, the two forms alternated in one process, medians of --reps pairs.

    python tools/state_train_cost.py [--reps 40] [--modes f16x3,f32] [--out FILE]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import windgnn_oracle as orc  # noqa: E402
from windgnn_amd import _lib  # noqa: E402
from windgnn_amd.functional import (gcn_gru_backward_raw, gcn_gru_forward_raw, gcn_gru_state_backward_raw,  # noqa: E402
                                    gcn_gru_state_forward_raw)

MATH = {"f32": _lib.MATH_F32, "f16x3": _lib.MATH_F16X3, "f16x3g": _lib.MATH_F16X3G, "f16": _lib.MATH_F16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=40)
    ap.add_argument("--modes", default="f16x3,f32")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    S, T, B, H = 34, 24, 4096, 102
    g = torch.Generator().manual_seed(5)
    A = (torch.rand(S, S, generator=g) / S + 0.01).to(dev)
    X = torch.rand(B, T, S, 13, generator=g).to(dev)
    dY = (torch.randn(B, T, H, generator=g) * 1e-6).to(dev)
    h0 = (torch.rand(B, H, generator=g) - 0.5).to(dev)
    dhn = (torch.randn(B, H, generator=g) * 1e-6).to(dev)
    dh0 = torch.empty(B, H, device=dev)
    p = orc.init_params(S, 13, H, seed=1)
    params = [p[k].to(dev).contiguous() for k in orc.PARAM_KEYS]
    grads = [torch.empty_like(q) for q in params]
    lines = ["S=%d T=%d B=%d H=%d, %d alternated pairs per mode, device events; medians (min) in us" % (S, T, B, H, a.reps)]

    def plain(m):
        Y, st, d = gcn_gru_forward_raw(A, X, params, m)
        gcn_gru_backward_raw(d, A, X, params, Y, dY, st, grads)

    def state(m):
        Y, hn, st, d = gcn_gru_state_forward_raw(A, X, params, m, h0)
        gcn_gru_state_backward_raw(d, A, X, params, Y, dY, dhn, st, grads, dh0)

    for mode in a.modes.split(","):
        m = MATH[mode]
        for _ in range(3):
            plain(m)
            state(m)
        torch.cuda.synchronize()
        t = {"plain": [], "state": []}
        for _ in range(a.reps):
            for name, fn in (("plain", plain), ("state", state)):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                fn(m)
                e1.record()
                e1.synchronize()
                t[name].append(1e3 * e0.elapsed_time(e1))
        mp, ms = statistics.median(t["plain"]), statistics.median(t["state"])
        lines.append("%-6s wgnn_fwd + wgnn_bwd_part %8.1f (%8.1f)   wgnn_fwd_state_stash + wgnn_bwd_state_part %8.1f (%8.1f)"
                     "   overhead %+.1f %%" % (mode, mp, min(t["plain"]), ms, min(t["state"]), 100.0 * (ms / mp - 1.0)))
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
