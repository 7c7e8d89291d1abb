"""The cases of series training on a loss spec (include/windgnn_series_lossfn.h), shared by tests/test_series_lossfn_host.py
(which qualifies them on the fp64 oracle alone) and tests/test_gpu_series_lossfn.py.  No GPU is needed to import or to call
anything here.

Shapes, seeds, draws, tables and masks are tests/series_at_cases.py's and tests/series_masked_cases.py's; a case adds a row
mapping the masked suite does not have for the per-K shapes (K*_small at stride 2, K*_big at stride 1: the same window counts,
17 and 257, fit the same series), and a spec (kind, delta, t_from).  masked follows the mask: "e" (no NaN) runs with masked = 0,
every other mask with masked = 1.

The reference is the fp64 oracle on the materialised windows: orc.forward, then, with r = Y - L,

    M = {t >= t_from, and (not masked or L is not NaN)}    m = |M|
    loss = sum over M of rho(r) / m        dY = rho'(r) / m on M, 0 elsewhere        grads = orc.backward(..., dY)

    mse  rho = r^2, rho' = 2 r      l1  rho = |r|, rho' = sign(r)      huber  rho = r^2 / 2 if |r| <= delta else delta (|r| - delta / 2),
                                                                              rho' = clamp(r, -delta, delta)

L1 and the sign of a residual.  sign(r) must not hang on fp32 rounding, and the [0, 1) label draws hold residuals down to 6e-6.
The L1 cases therefore move the labels away from Y, which lies in (-1, 1): even columns of the label series go up by 2 (into
[2, 3): r < -1), odd columns down by 3 (into [-3, -2): r > 1).  Both signs occur, and |r| > 1 everywhere, whatever windows share
a row.  The Huber and MSE cases keep the [0, 1) draw, where r has both signs and delta = 0.25 splits it into both arms."""
import functools

import torch

import series_at_cases as sc
import series_masked_cases as mc
from test_gpu_series_train import SPARE

KINDS = {"mse": 0, "l1": 1, "huber": 2}
DELTA = 0.25
# per-K shapes strided: (stride, n) -- rows 36, T 3: 16 * 2 + 3 = 35; rows 272, T 16: 256 + 16 = 272
K_STRIDED = {"small": ("stride2", 2, 17), "big": ("stride1", 1, 257)}


def mapping(base, how):
    """(starts, stride or None): series_masked_cases.mapping, and the strided form of a per-K shape."""
    if how == "table" or base == "irregular":
        return mc.mapping(base, how)
    r = sc.reference(base)
    name, stride, n = K_STRIDED[base.rsplit("_", 1)[1]]
    assert how == name and n == r.n and (n - 1) * stride + r.T <= r.rows < n * stride + r.T
    return [w * stride for w in range(n)], stride


def label_series(base, how, kind):
    """[rows, H]: series_masked_cases.label_series' draw for this mapping (SPARE in the rows no window covers), moved away from
    Y for an L1 case (module docstring); no NaN yet."""
    r = sc.reference(base)
    starts, _ = mapping(base, how)
    g = torch.Generator().manual_seed(8800 + 131 * r.seed + r.S * 7 + r.rows + r.H + len(how))
    Ls = torch.rand(r.rows, r.H, generator=g)
    if how == "table" or base == "irregular":
        assert torch.equal(Ls[sc.covered_rows(r.rows, r.T, starts)], mc.label_series(base, how)[sc.covered_rows(r.rows, r.T, starts)])
    if kind == "l1":
        Ls[:, 0::2] += 2.0
        Ls[:, 1::2] -= 3.0
    Ls[~sc.covered_rows(r.rows, r.T, starts)] = SPARE
    return Ls


def missing(base, how, mask):
    """[rows, H] bool: series_masked_cases.missing; for a mapping it does not know, the masks that depend on the series alone."""
    if how == "table" or base == "irregular":
        return mc.missing(base, how, mask)
    assert mask in "abef"
    return mc.missing(base, "table", mask)


class Ref:
    pass


@functools.lru_cache(maxsize=None)
def forward(base, how):
    """The oracle's forward of a mapping's materialised windows (shared by all its specs and masks)."""
    if how == "table" or base == "irregular":
        return mc.forward(base, how)
    from oracle import windgnn_oracle as orc
    r = sc.reference(base)
    starts, _ = mapping(base, how)
    X = sc.windows_at(r.Xs, r.T, starts)
    Yo, cache = orc.forward(r.A.double(), X.double(), r.p64)
    return X, Yo, cache


def counted(L, t_from, masked):
    """[n, T, H] bool: the set M on the window-major labels L."""
    on = torch.zeros(L.shape, dtype=torch.bool)
    on[:, t_from:] = True
    return on & ~torch.isnan(L) if masked else on


def loss_and_dy(Yo, L, kind, delta, t_from, masked, plant=None):
    """(loss, dY, m) in fp64 on the window-major labels L.  plant: one of PLANTED, the mistake to make on purpose."""
    on = counted(L, t_from, masked)
    m = int(on.sum())
    r = torch.where(on, Yo - torch.where(on, L, torch.zeros_like(L)), torch.zeros_like(Yo))     # 0 outside M: no NaN leaks
    a = r.abs()
    if kind == "mse":
        rho, g = r * r, 2.0 * r
    elif kind == "l1":
        rho, g = a, torch.sign(r) * (2.0 if plant == "l1 gradient with the factor 2" else 1.0)
    else:
        quad = (1.0 if plant == "quadratic arm without the half" else 0.5) * r * r
        lin = delta * a if plant == "linear arm without its constant" else delta * (a - 0.5 * delta)
        rho, g = torch.where(a <= delta, quad, lin), r.clamp(-delta, delta)
        if plant == "quadratic arm without the half":            # ... and its derivative: 2 r there
            g = torch.where(a <= delta, 2.0 * r, g)
    div = L.numel() if plant == "m taken as n T H" else m
    if div == 0:
        return torch.tensor(float("nan"), dtype=torch.float64), torch.zeros_like(Yo), m
    loss = torch.where(on, rho, torch.zeros_like(rho)).sum() / div
    if plant == "t_from on the loss but not on dY":
        every = counted(L, 0, masked)
        r0 = torch.where(every, Yo - torch.where(every, L, torch.zeros_like(L)), torch.zeros_like(Yo))
        g0 = {"mse": 2.0 * r0, "l1": torch.sign(r0), "huber": r0.clamp(-delta, delta)}[kind]
        return loss, g0 / div, m
    return loss, torch.where(on, g, torch.zeros_like(g)) / div, m


# the five planted mistakes, and the cases each can show on
PLANTED = {"quadratic arm without the half": lambda q: q.kind == "huber",
           "l1 gradient with the factor 2": lambda q: q.kind == "l1",
           "linear arm without its constant": lambda q: q.kind == "huber",
           "m taken as n T H": lambda q: q.t_from > 0,
           "t_from on the loss but not on dY": lambda q: q.t_from > 0}


@functools.lru_cache(maxsize=None)
def reference(base, how, mask, kind, delta, t_from):
    """Host tensors of a case and the oracle's training step on its spec: computed once, shared, never modified."""
    from oracle import windgnn_oracle as orc
    r = sc.reference(base)
    starts, stride = mapping(base, how)
    q = Ref()
    q.id = "%s-%s-%s-%s-from%d" % (base, how, mask, kind, t_from)
    q.base, q.how, q.mask, q.r = base, how, mask, r
    q.kind, q.delta, q.t_from, q.masked = kind, float(delta), t_from, 0 if mask == "e" else 1
    q.S, q.H, q.rows, q.T, q.n, q.starts, q.stride = r.S, r.H, r.rows, r.T, len(starts), starts, stride
    q.A, q.Xs, q.p, q.p64, q.margin = r.A, r.Xs, r.p, r.p64, r.margin
    q.clean = label_series(base, how, kind)
    q.hit = missing(base, how, mask)
    q.Ls = q.clean.clone()
    q.Ls[q.hit] = float("nan")
    q.X, q.Yo, cache = forward(base, how)
    q.L = sc.windows_at(q.Ls, q.T, starts)
    assert not (q.L == SPARE).any()
    loss, dY, q.m = loss_and_dy(q.Yo, q.L.double(), kind, q.delta, t_from, q.masked)
    q.loss_o = float(loss)
    q.dY = dY
    q.gm = orc.backward(q.A.double(), q.X.double(), q.p64, q.Yo, cache, dY)
    on = counted(q.L, t_from, q.masked)
    q.counts = [int(on[16 * b:16 * b + 16].sum()) for b in range(-(-q.n // 16))]            # per workgroup of 16 windows
    return q


def planted(q, what):
    """(loss, grads) of the planted mistake `what` on the reference q, in the oracle."""
    from oracle import windgnn_oracle as orc
    _, _, cache = forward(q.base, q.how)
    loss, dY, _ = loss_and_dy(q.Yo, q.L.double(), q.kind, q.delta, q.t_from, q.masked, plant=what)
    return float(loss), orc.backward(q.A.double(), q.X.double(), q.p64, q.Yo, cache, dY)


# ---- the GPU parity cases: id -> (base, how, mask, kind, delta, t_from) -------------------------------------------------------
PARITY = {}


def _add(base, how, mask, kind, t_from):
    PARITY["%s-%s-%s-%s-from%d" % (base, how, mask, kind, t_from)] = (base, how, mask, kind, DELTA if kind == "huber" else 0.0, t_from)


for _how in ("table", "stride2"):
    for _kind in ("l1", "huber"):
        for _t in (0, 2, 4):                                     # T = 5: every step, past a warm-up, the last step alone
            for _m in "eb":
                _add("irregular", _how, _m, _kind, _t)
for _kind in ("mse", "l1", "huber"):
    _add("real_widths", "table", "a", _kind, 12)
# every K of both recurrences under both row mappings: K*_small (n 17, T 3: a ragged second workgroup) and K*_big (n 257, T 16:
# the dGHn form) take opposite mappings, so the 18 cases launch each of the 36 instances by name; kinds and masks alternate
INSTANCES = []
for _i, _K in enumerate(sc.FWD_KS):
    _kind = ("l1", "huber", "mse")[_i % 3]
    _add("K%d_small" % _K, "table" if _i % 2 == 0 else "stride2", "b" if _i % 2 == 0 else "e", _kind, 1)
    INSTANCES.append(list(PARITY)[-1])
    _kind = ("huber", "mse", "l1")[_i % 3]
    _add("K%d_big" % _K, "stride1" if _i % 2 == 0 else "table", "e" if _i % 2 == 0 else "b", _kind, 8)
    INSTANCES.append(list(PARITY)[-1])
del _how, _kind, _t, _m, _i, _K
