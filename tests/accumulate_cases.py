"""The cases of accumulating gradients over several calls (TrainStep.accumulate / accumulate_series / apply), shared by
tests/test_accumulate_host.py and tests/test_gpu_accumulate.py.  No GPU is needed to import or to call anything here.

Shapes (S, H, T, B, the cut of B into calls, k of a k-NN graph in CSR or None) -- the smallest at which the bookkeeping can go
wrong, not the workload's:

    small  (7, 21, 5, 6, 1 + 2 + 3)       three calls of three sizes
    real   (34, 102, 6, 20, 16 + 4)       the real widths: a full and a ragged 16-window workgroup
    csr    (12, 21, 5, 6, 1 + 2 + 3)      a 4-NN graph handed over as CSR, three calls
    series rows 40, T = 5, S = 7, H = 21: tables of 17 and of 5 windows on two different series tensors (small's parameters and
           adjacency, so that a materialised call and a series call can share one step)

The reference is the fp64 oracle's training step on the UNION of the windows: orc.forward, the loss and dY of the spec over all
counted labels at once (tests/series_lossfn_cases.py's loss_and_dy), orc.backward, orc.adam_step.  Adam runs with eps = 1e-3 on
both sides (tests/step_loss_cases.py's EPS and its reason).

The loss-spec cases run on tests/step_loss_cases.py's own draws (its "small": S 7, T 12, B 4, H 21) cut 1 + 1 + 2; the L1 labels
there lie more than 1 away from Y, so sign(r) does not hang on the device's rounding, and that is a property of each element:
tests/test_accumulate_host.py checks that every cut keeps it.  The staggered mask makes the calls' counts differ: no label
missing in the first call, a tenth in the second, four tenths in the third."""
import functools

import torch

import series_lossfn_cases as lc
import step_loss_cases as sl

SHAPES = {"small": (7, 21, 5, 6, (1, 2, 3), None), "real": (34, 102, 6, 20, (16, 4), None), "csr": (12, 21, 5, 6, (1, 2, 3), 4)}
TOL = sl.TOL                    # 1e-4 of the tensor's max: the project's bar against the fp64 oracle
EPS = sl.EPS
LR = 1e-3
SPEC_CUT = (1, 1, 2)            # step_loss_cases' small case: B = 4
RATES = (0.0, 0.1, 0.4)         # labels missing per call of SPEC_CUT
SERIES = dict(rows=40, T=5, tables=((0, 0, 1, 2, 4, 5, 7, 9, 12, 13, 17, 20, 21, 26, 30, 35, 35), (3, 8, 8, 19, 33)))


class Case:
    pass


def spans(cut):
    out, lo = [], 0
    for n in cut:
        out.append((lo, lo + n))
        lo += n
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """Host tensors of a shape and the parameters: computed once, shared, never modified."""
    from oracle import windgnn_oracle as orc
    S, H, T, B, cut, k = SHAPES[name]
    c = Case()
    c.name, c.S, c.H, c.T, c.B, c.cut, c.csr = name, S, H, T, B, cut, None
    g = torch.Generator().manual_seed(6100 + 17 * S + 3 * T + B + 5 * H)
    if k:
        from windgnn_amd.graph import CsrAdjacency, build_knn_adjacency, synthetic_station_coords
        c.csr = CsrAdjacency(*build_knn_adjacency(synthetic_station_coords(S, seed=S), k))
        c.A = c.csr.dense()
    else:
        c.A = torch.rand(S, S, generator=g) / S + 0.01
    c.X = torch.rand(B, T, S, 13, generator=g)
    c.L = torch.rand(B, T, H, generator=g)
    c.p = orc.init_params(S, 13, H, seed=S + H)
    return c


@functools.lru_cache(maxsize=None)
def series_case():
    """Two series tensors with their label series and tables, on small's adjacency and parameters."""
    c = case("small")
    s = Case()
    s.T, s.tables = SERIES["T"], SERIES["tables"]
    g = torch.Generator().manual_seed(6200)
    s.series = [torch.rand(SERIES["rows"], c.S, 13, generator=g) for _ in s.tables]
    s.Ls = [torch.rand(SERIES["rows"], c.H, generator=g) for _ in s.tables]
    s.X = [torch.stack([x[r:r + s.T] for r in t]) for x, t in zip(s.series, s.tables)]
    s.L = [torch.stack([x[r:r + s.T] for r in t]) for x, t in zip(s.Ls, s.tables)]
    return s


class Ref:
    pass


def oracle_steps(A, X, L, p, kind="mse", delta=0.0, t_from=0, masked=0, steps=1, max_norm=None):
    """The fp64 oracle's `steps` Adam steps on the windows X with the labels L (a list of label tensors: one per step, the last
    repeated): per step the loss, the count, the 8 gradients, their norm and Y; and the parameters after each step."""
    from oracle import windgnn_oracle as orc
    A, X = A.double(), X.double()
    p = {k: v.double() for k, v in p.items()}
    state = orc.adam_init(p)
    q = Ref()
    q.loss, q.m, q.g, q.norm, q.Y, q.p = [], [], [], [], [], []
    Ls = L if isinstance(L, (list, tuple)) else [L]
    for s in range(steps):
        Lw = Ls[min(s, len(Ls) - 1)].double()
        Y, cache = orc.forward(A, X, p)
        loss, dY, m = lc.loss_and_dy(Y, Lw, kind, delta, t_from, masked)
        g = orc.backward(A, X, p, Y, cache, dY)
        norm = float(torch.sqrt(sum((v ** 2).sum() for v in g.values())))
        q.loss.append(float(loss)), q.m.append(m), q.g.append(g), q.norm.append(norm), q.Y.append(Y)
        if max_norm is not None:
            coef = min(1.0, max_norm / (norm + 1e-6))
            g = {k: v * coef for k, v in g.items()}
        p = orc.adam_step(p, g, state, lr=LR, eps=EPS)
        q.p.append(p)
    return q


@functools.lru_cache(maxsize=None)
def union(name, steps=1, max_norm=None):
    """The oracle on all B windows of a shape at once, MSE."""
    c = case(name)
    return oracle_steps(c.A, c.X, c.L, c.p, steps=steps, max_norm=max_norm)


@functools.lru_cache(maxsize=None)
def series_union():
    """The oracle on the 17 + 5 windows of the two series tensors."""
    c, s = case("small"), series_case()
    return oracle_steps(c.A, torch.cat(s.X), torch.cat(s.L), c.p)


@functools.lru_cache(maxsize=None)
def mixed_union():
    """The oracle on small's 6 materialised windows and the first table's 17 series windows."""
    c, s = case("small"), series_case()
    return oracle_steps(c.A, torch.cat([c.X, s.X[0]]), torch.cat([c.L, s.L[0]]), c.p)


@functools.lru_cache(maxsize=None)
def staggered_labels():
    """step_loss_cases' small L1 labels with RATES of them NaN per call of SPEC_CUT."""
    c = sl.case("small")
    L = c.L["l1"].clone()
    g = torch.Generator().manual_seed(6300)
    for (lo, hi), rate in zip(spans(SPEC_CUT), RATES):
        L[lo:hi][torch.rand(hi - lo, c.T, c.H, generator=g) < rate] = float("nan")
    return L


@functools.lru_cache(maxsize=None)
def staggered_union():
    """The oracle on step_loss_cases' small case with the staggered labels: L1 from step 2 over the labels that exist."""
    c = sl.case("small")
    return oracle_steps(c.A, c.X, staggered_labels(), c.p, "l1", 0.0, 2, 1)


def window_weighted(c, L, kind, delta, t_from, masked, cut):
    """What weighting the calls by their WINDOWS instead of their labels would give, in fp64: (loss, the 8 gradients)."""
    from oracle import windgnn_oracle as orc
    A, p = c.A.double(), {k: v.double() for k, v in c.p.items()}
    B = sum(cut)
    loss, grads = 0.0, None
    for lo, hi in spans(cut):
        X = c.X[lo:hi].double()
        Y, cache = orc.forward(A, X, p)
        li, dY, _ = lc.loss_and_dy(Y, L[lo:hi].double(), kind, delta, t_from, masked)
        g = orc.backward(A, X, p, Y, cache, dY)
        w = (hi - lo) / B
        loss += w * float(li)
        grads = {k: w * v for k, v in g.items()} if grads is None else {k: grads[k] + w * v for k, v in g.items()}
    return loss, grads
