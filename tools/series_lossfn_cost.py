"""Cost of one series TRAINING step on a loss spec (include/windgnn_series_lossfn.h), six routes on the SAME windows, in one
process on one device:

  (d)  default            TrainStep.step_series(adj, series, Ls, T, 1)                 -- the unchanged route, the yardstick
  (d') default again      the same call on a second TrainStep: the spread of the default route's single steps across the
                          alternations, and the distance of the two medians, are the run's two noise figures
  (m)  lossfn, MSE        the `lossfn` instances on {MSE, t_from 0}: what the count and the selects cost by themselves
  (l)  lossfn, L1         step_series(..., loss="l1")
  (h)  lossfn, Huber      step_series(..., loss="huber", huber_delta=0.25)
  (g)  Huber, NaN, warm-up  loss="huber", huber_delta=0.25, loss_from=12, missing_labels=True on Ls with one label in ten NaN

at S = 34, H = 102, T = 24, n = 4096 windows, stride 1, math = "f32".  Every route starts from the same parameters.  The clock is
device events around each step with the routes alternated (medians and minima of --reps steps after --warmup); (d) and (d')
stand first and last in every round.  Then the library's per-kernel tally of one step of each route, which says where a
difference comes from.  (d), (d') and (m) must hold the same parameters bit for bit after the same steps.

(m) is not reachable through the public keywords -- loss="mse" from step 0 IS the default route -- so for that route alone the
tool replaces series.loss_spec by one that always builds the spec.

    python tools/series_lossfn_cost.py [--reps 30] [--warmup 5] [--n 4096] [--out profiles/r15_series_lossfn_cost.txt]
"""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from oracle import windgnn_oracle as orc  # noqa: E402
from windgnn_amd import GCN_GRU, _lib  # noqa: E402
from windgnn_amd import series as wseries  # noqa: E402
from windgnn_amd import trainer as wtrainer  # noqa: E402
from windgnn_amd.series import series_labels  # noqa: E402
from windgnn_amd.trainer import TrainStep  # noqa: E402
from series_train_cost import kernels, timed  # noqa: E402


def forced_spec(step):
    """`step` with the spec built even for {MSE, t_from 0}."""
    real = wseries.loss_spec

    def always(loss, huber_delta, loss_from, seq_len, missing_labels=False, who=""):
        return real(loss, huber_delta, loss_from, seq_len, missing_labels, who) or _lib.LossFn(
            _lib.LOSS_MSE, 0.0, 0, 1 if missing_labels else 0)

    def run():
        wseries.loss_spec = wtrainer.loss_spec = always
        try:
            return step()
        finally:
            wseries.loss_spec = wtrainer.loss_spec = real
    return run


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

    order = ["d", "m", "l", "h", "g", "d'"]
    models = {k: fresh() for k in order}
    tr = {k: TrainStep(m) for k, m in models.items()}

    def call(k, L=Ls, **kw):
        return lambda: tr[k].step_series(A, series, L, T, stride, n_windows=n, **kw)

    routes = {"d": call("d"), "d'": call("d'"), "m": forced_spec(call("m")), "l": call("l", loss="l1"),
              "h": call("h", loss="huber", huber_delta=0.25),
              "g": call("g", Lg, loss="huber", huber_delta=0.25, loss_from=12, missing_labels=True)}
    t = {name: [] for name in order}
    for i in range(a.warmup + a.reps):
        for name in order:
            us = timed(routes[name])
            if i >= a.warmup:
                t[name].append(us)
    same = all(torch.equal(p, q) and torch.equal(p, r) for p, q, r in
               zip(models["d"].parameters(), models["d'"].parameters(), models["m"].parameters()))
    finite = all(bool(torch.isfinite(p).all()) for k in ("l", "h", "g") for p in models[k].parameters())
    med = {name: statistics.median(v) for name, v in t.items()}
    noise = abs(med["d"] - med["d'"])
    both = t["d"] + t["d'"]
    spread = max(both) - min(both)
    quart = statistics.quantiles(both, n=4)
    lines = ["S=%d H=%d T=%d n=%d stride=%d math=f32; us per training step; device events: %d alternated steps per route after %d "
             "warm-up steps, medians (min)" % (S, H, T, n, stride, a.reps, a.warmup),
             "series [%d, %d, 13], Ls [%d, %d], %.2f %% of the labels NaN in (g); parameters after %d steps: (d') and (m) %s (d)'s "
             "bit for bit; (l), (h), (g) all finite: %s" % (rows, S, Ls.shape[0], H, 100.0 * float(gaps.float().mean()),
                                                           a.warmup + a.reps, "equal" if same else "DIFFER FROM", finite),
             "noise, two figures: the default route's %d single steps across the alternations spread over %.1f us (%.1f .. %.1f, "
             "quartiles %.1f .. %.1f); the medians of its two instances differ by %.1f us"
             % (len(both), spread, min(both), max(both), quart[0], quart[2], noise)]
    for name, what in (("d", "(d)  step_series, default               "), ("d'", "(d') the same, second instance          "),
                       ("m", "(m)  lossfn instances, MSE from step 0  "), ("l", "(l)  loss='l1'                          "),
                       ("h", "(h)  loss='huber', delta 0.25           "),
                       ("g", "(g)  huber, ~10 % NaN, loss_from=12     ")):
        lines.append("  %s %8.1f (%8.1f)   this - (d) = %+6.1f us   this / (d) = %.3f"
                     % (what, med[name], min(t[name]), med[name] - med["d"], med[name] / med["d"]))
    for name in order[:-1]:
        lines += ["kernels of one step of (%s) (per-kernel events serialise the launches):" % name] + kernels(routes[name])
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")
    return 0 if same and finite else 1


if __name__ == "__main__":
    sys.exit(main())
