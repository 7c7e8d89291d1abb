"""The cases of series training through missing labels (include/windgnn_series_masked.h), shared by
tests/test_series_masked_host.py (which qualifies them on the fp64 oracle alone) and tests/test_gpu_series_masked.py.  No GPU is
needed to import or to call anything here.

Shapes, seeds, draws and tables are tests/series_at_cases.py's (and through it tests/test_gpu_series.py's _draw): a case here is
one of its references, a row mapping (its table, or a stride over the same series), and a MASK -- the rows and columns of the
label series that hold NaN.  The reference is the fp64 oracle on the materialised windows: orc.forward, then, with M the set of
labels that are not NaN and m = |M|,

    loss = sum over M of (Y - L)^2 / m        dY = 2 (Y - L) / m on M, 0 elsewhere        grads = orc.backward(..., dY)

The label series is random in [0, 1) with test_gpu_series_train.py's SPARE (1e3) in every row no window covers, drawn before
the mask is laid over it, so a mask never changes the labels that remain."""
import functools

import torch

import series_at_cases as sc
from test_gpu_series_train import SPARE

MASKS = ("a", "b", "c", "d", "e", "f")
# the issue's second case: the irregular shape (S 7, H 21, rows 40, T 5) strided.  19 windows at stride 2 would need 41 rows, so
# stride 2 takes the 18 that fit: still a ragged second workgroup (2 windows)
STRIDED = {"stride1": (1, 19), "stride2": (2, 18)}


def mapping(base, how):
    """(starts, stride or None) of a case: how = "table" (the base case's own table) or a key of STRIDED."""
    r = sc.reference(base)
    if how == "table":
        return list(r.starts), None
    stride, n = STRIDED[how]
    assert base == "irregular" and (n - 1) * stride + r.T <= r.rows and (n == 19 or n * stride + r.T > r.rows)
    return [w * stride for w in range(n)], stride


def label_series(base, how):
    """[rows, H] labels in [0, 1), SPARE in the rows no window of this mapping covers; no NaN yet."""
    r = sc.reference(base)
    starts, _ = mapping(base, how)
    g = torch.Generator().manual_seed(8800 + 131 * r.seed + r.S * 7 + r.rows + r.H + len(how))
    Ls = torch.rand(r.rows, r.H, generator=g)
    Ls[~sc.covered_rows(r.rows, r.T, starts)] = SPARE
    return Ls


def missing(base, how, mask):
    """[rows, H] bool: where the label series holds NaN under `mask`."""
    r = sc.reference(base)
    starts, _ = mapping(base, how)
    rows, H, S, T = r.rows, r.H, r.S, r.T
    hit = torch.zeros(rows, H, dtype=torch.bool)
    if mask == "a":
        # station s reads nothing during hours [h0, h1): Ls[tau] = [y[tau + 1] | y[tau + 2] | y[tau + 3]], so column k * S + s is
        # missing at the rows tau with h0 <= tau + k + 1 < h1
        s, h0, h1 = S // 2, rows // 5, rows // 5 + max(6, rows // 3)
        for k in range(3):
            lo, hi = max(h0 - k - 1, 0), max(h1 - k - 1, 0)
            hit[lo:hi, k * S + s] = True
    elif mask == "b":
        g = torch.Generator().manual_seed(4242 + rows + H)
        hit = torch.rand(rows, H, generator=g) < 0.10
    elif mask == "c":
        assert len(starts) > 16
        for s in starts[:16]:                       # every row the first workgroup's 16 windows read
            hit[s:s + T] = True
    elif mask == "d":
        for s in starts[1::3]:                      # the last row of every third window
            hit[s + T - 1] = True
    elif mask == "f":
        hit[:] = True
    else:
        assert mask == "e"
    return hit


class Ref:
    pass


@functools.lru_cache(maxsize=None)
def forward(base, how):
    """The oracle's forward of a mapping's materialised windows (shared by all its masks)."""
    from oracle import windgnn_oracle as orc
    r = sc.reference(base)
    starts, stride = mapping(base, how)
    X = sc.windows_at(r.Xs, r.T, starts)
    if how == "table":
        assert torch.equal(X, r.X)
    Yo, cache = orc.forward(r.A.double(), X.double(), r.p64)
    return X, Yo, cache


def masked_loss(Yo, L, divide_by=None, missing_as=None, mask_dy=True):
    """(loss, dY, m) in fp64 on the window-major labels L (NaN = no label).  The three keywords plant the three mistakes:
    divide_by: a count other than m; missing_as: the value a missing label is read as (it then counts); mask_dy=False: the loss
    skips the missing labels but dY is formed against them as zeros."""
    have = ~torch.isnan(L)
    Lz = torch.where(have, L, torch.zeros_like(L))
    if missing_as is not None:
        Lz = torch.where(have, L, torch.full_like(L, missing_as))
        have = torch.ones_like(have)
    m = int(have.sum())
    div = m if divide_by is None else divide_by
    d = torch.where(have, Yo - Lz, torch.zeros_like(Yo))
    loss = (d * d).sum() / div if div else torch.tensor(float("nan"), dtype=torch.float64)
    dY = 2.0 * (d if mask_dy else Yo - Lz) / div if div else torch.zeros_like(Yo)
    return loss, dY, m


@functools.lru_cache(maxsize=None)
def reference(base, how, mask):
    """Host tensors of a case and the oracle's masked training step: computed once, shared, never modified."""
    from oracle import windgnn_oracle as orc
    r = sc.reference(base)
    starts, stride = mapping(base, how)
    q = Ref()
    q.id = "%s-%s-%s" % (base, how, mask)
    q.base, q.how, q.mask, q.r = base, how, mask, r
    q.S, q.H, q.rows, q.T, q.n, q.starts, q.stride = r.S, r.H, r.rows, r.T, len(starts), starts, stride
    q.A, q.Xs, q.p, q.p64, q.margin = r.A, r.Xs, r.p, r.p64, r.margin
    q.clean = label_series(base, how)
    q.hit = missing(base, how, mask)
    q.Ls = q.clean.clone()
    q.Ls[q.hit] = float("nan")
    q.X, q.Yo, cache = forward(base, how)
    q.L = sc.windows_at(q.Ls, q.T, starts)
    assert not (q.L == SPARE).any()
    loss, dY, q.m = masked_loss(q.Yo, q.L.double())
    q.loss_o = float(loss)
    q.dY = dY
    q.gm = orc.backward(q.A.double(), q.X.double(), q.p64, q.Yo, cache, dY)
    nb = -(-q.n // 16)
    q.counts = [int((~torch.isnan(q.L[16 * b:16 * b + 16])).sum()) for b in range(nb)]     # per workgroup of 16 windows
    return q


def planted(q):
    """{mistake: (loss, grads)} of the three planted mistakes on the reference q, in the oracle."""
    from oracle import windgnn_oracle as orc
    _, _, cache = forward(q.base, q.how)
    A, X, L = q.A.double(), q.X.double(), q.L.double()
    out = {}
    for what, kw in (("divide by nTH", {"divide_by": q.n * q.T * q.H}), ("missing as 0", {"missing_as": 0.0}),
                     ("loss masked, dY not", {"mask_dy": False})):
        loss, dY, _ = masked_loss(q.Yo, L, **kw)
        out[what] = (float(loss), orc.backward(A, X, q.p64, q.Yo, cache, dY))
    return out


# the GPU parity cases: id -> (base, how, mask)
PARITY = {}
for _m in "abcd":
    PARITY["irregular-table-" + _m] = ("irregular", "table", _m)
for _how in STRIDED:
    for _m in "abcd":
        PARITY["irregular-%s-%s" % (_how, _m)] = ("irregular", _how, _m)
PARITY["real_widths-table-a"] = ("real_widths", "table", "a")
for _K in sc.FWD_KS:
    PARITY["K%d_small-table-b" % _K] = ("K%d_small" % _K, "table", "b")
for _K in sc.FWD_KS:
    PARITY["K%d_big-table-b" % _K] = ("K%d_big" % _K, "table", "b")
del _m, _how, _K
