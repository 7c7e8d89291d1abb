"""The cases of validation on materialised windows (TrainStep.validate, functional.validation_terms / val_add), shared by
tests/test_validate_host.py (which holds the helpers and qualifies the cases on the CPU) and tests/test_gpu_validate.py.  No GPU
is needed to import or to call anything here.

Shapes (S, T, B, H), the smallest that reach each path:

    tiny   (3, 2, 1, 9)        L handed over as [T, H], as the reference's loader yields it
    odd    (7, 12, 5, 21)      odd S * 13
    real   (34, 24, 4, 102)    the real widths
    call   (34, 168, 1, 102)   the reference's call shape
    wide   (7, 4, 4, 150)      the wide-GRU path
    csr    (65, 4, 3, 12)      a 6-NN graph in CSR (S > 64 has no dense path)

The loss of a spec over the counted set M = {t >= t_from, and (not masked or the label is not NaN)} is formed here in fp64 from
whatever Y it is given (the device's, or the fp64 oracle's): terms() returns (sum of rho, |M|, max |r| over M).  Labels are
U[0, 1), so r has both signs and the Huber delta 0.25 splits it into both arms; NaN masks: "none", "tenth" (a seeded 10 %) and
"all"."""
import functools

import torch

import series_lossfn_cases as lc

SHAPES = {"tiny": (3, 2, 1, 9), "odd": (7, 12, 5, 21), "real": (34, 24, 4, 102), "call": (34, 168, 1, 102),
          "wide": (7, 4, 4, 150), "csr": (65, 4, 3, 12)}
CSR_K = 6
MODES = ("f32", "f16x3", "f16x3g", "f16")
GRADE32 = ("f32", "f16x3", "f16x3g")        # the modes held to the project's 1e-4 bar against the fp64 oracle
KINDS = ("mse", "l1", "huber")
DELTA = lc.DELTA
MASKS = ("none", "tenth", "all")
TOL = 1e-4                                   # the project's bar against the fp64 oracle
SUM_TOL = 1e-10                              # fp64 summation order over <= 4e5 terms
LR = 1e-3                                    # the three-step scenario's learning rate: the reference's (src/main.py:52)
SHIFT = -4.0                                 # its third step trains on labels moved by this much: away from the held-out labels
STEPS = 3
SCENARIOS = (("odd", "f16x3"), ("csr", "f16x3"))


def t_froms(T):
    """loss_from in {0, 2, T - 1}, as far as the window has those steps."""
    return sorted({0, min(2, T - 1), T - 1})


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(name, seed=0):
    """Host tensors of a shape: A (dense; csr: the CsrAdjacency beside it), X, the clean labels, the parameters and the fp64
    oracle's Y.  Computed once, shared, never modified."""
    from oracle import windgnn_oracle as orc
    S, T, B, H = SHAPES[name]
    c = Case()
    c.name, c.S, c.T, c.B, c.H, c.csr = name, S, T, B, H, None
    g = torch.Generator().manual_seed(4100 + 31 * S + 7 * T + B + 101 * H + 1009 * seed)
    if name == "csr":
        from windgnn_amd.graph import CsrAdjacency, build_knn_adjacency, synthetic_station_coords
        c.csr = CsrAdjacency(*build_knn_adjacency(synthetic_station_coords(S, seed=S), CSR_K))
        c.A = c.csr.dense()
    else:
        c.A = torch.rand(S, S, generator=g) / S + 0.01
    c.X = torch.rand(B, T, S, 13, generator=g)
    c.L = torch.rand(B, T, H, generator=g)
    c.hit = torch.rand(B, T, H, generator=g) < 0.1
    c.p = orc.init_params(S, 13, H, seed=S + H + seed)
    c.p64 = {k: v.double() for k, v in c.p.items()}
    c.Yo = orc.forward(c.A.double(), c.X.double(), c.p64, want_cache=False)[0]
    return c


def labels(c, mask):
    """[B, T, H] fp32: the clean labels with the mask's entries NaN (a new tensor)."""
    L = c.L.clone()
    if mask == "tenth":
        L[c.hit] = float("nan")
    elif mask == "all":
        L[:] = float("nan")
    else:
        assert mask == "none"
    return L


def rho(r, kind, delta):
    a = r.abs()
    if kind == "mse":
        return r * r
    if kind == "l1":
        return a
    return torch.where(a <= delta, 0.5 * r * r, delta * (a - 0.5 * delta))


def terms(Y, L, kind, delta, t_from, masked):
    """(sum of rho over M, |M|, max |r| over M -- 0.0 for an empty M) as Python numbers, in fp64 on the host."""
    Y, L = Y.detach().cpu().double(), L.detach().cpu().double()
    on = lc.counted(L, t_from, masked)
    r = Y - L
    kept = r[on]
    return float(rho(kept, kind, delta).sum()), int(on.sum()), (float(kept.abs().max()) if kept.numel() else 0.0)


def rel(a, b):
    return abs(a - b) / max(abs(b), 1e-300)


@functools.lru_cache(maxsize=None)
def scenario(name):
    """The three-step scenario on the oracle alone: Adam (lr LR) on the shape's windows, the third step on labels moved by
    SHIFT, and the held-out MSE (another draw of the same shape) before the first step and after each.  Returns
    (held-out losses v0 .. v3, the training case, the held-out case)."""
    from oracle import windgnn_oracle as orc
    tr, held = case(name), case(name, seed=1)
    A = tr.A.double()
    p = dict(tr.p64)
    state = orc.adam_init(p)

    def held_out(p):
        s, m, _ = terms(orc.forward(A, held.X.double(), p, want_cache=False)[0], held.L, "mse", 0.0, 0, False)
        return s / m
    vals = [held_out(p)]
    for k in range(STEPS):
        Y, cache = orc.forward(A, tr.X.double(), p)
        _, dY, _ = lc.loss_and_dy(Y, tr.L.double() + (SHIFT if k == 2 else 0.0), "mse", 0.0, 0, 0)
        p = orc.adam_step(p, orc.backward(A, tr.X.double(), p, Y, cache, dY), state, lr=LR)
        vals.append(held_out(p))
    return vals, tr, held


def rule(losses, threshold=float("inf")):
    """The host restatement of `if loss < best: keep` with the patience counter, for passes closed at steps 0, 1, 2, ...:
    (best_step, improved, stale) after each pass."""
    best, best_step, stale, out = threshold, -1, 0, []
    for i, v in enumerate(losses):
        won = v < best
        if won:
            best, best_step, stale = v, i, 0
        else:
            stale += 1
        out.append((best_step, int(won), stale))
    return out
