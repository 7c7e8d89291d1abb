"""The cases of series mode on a table of window starts (include/windgnn_series_at.h), shared by tests/test_series_at_host.py (which
qualifies the inputs on the CPU) and tests/test_gpu_series_at.py: shapes, tables, seeds, and the fp64 oracle's results on the
MATERIALISED windows X[w, t] = Xs[starts[w] + t].  No GPU is needed to import or to call anything here.

Inputs are tests/test_gpu_series.py's _draw with the seed of the table.  The label series is random in [0, 1) with
tests/test_gpu_series_train.py's SPARE (1e3) in every row no window covers: read once, such a row moves the loss far past the bar.
It has exactly `rows` rows, the least the table entry points accept."""
import functools

import torch

from test_gpu_series import WIND_MAX, WIND_MIN, _draw, preact_margin
from test_gpu_series_train import SPARE

FWD_KS = (4, 8, 12, 16, 20, 24, 26, 28, 32)          # gru.hip's instances; BPTT's are KS3 below, bracket for bracket
BWD_KS3 = (12, 24, 36, 48, 60, 72, 78, 84, 96)

# The issue's irregular table: S 7, H 21, rows 40, T 5, n 19 -- a ragged second workgroup of 3, first start > 0, last start =
# rows - T, duplicates, coverage 6 > T at hour 9, uncovered rows 0-1, 18-19 and 27-29.
IRREGULAR = (7, 21, 40, 5, (2, 2, 3, 5, 5, 6, 7, 8, 9, 10, 11, 12, 13, 20, 21, 22, 30, 34, 35))
SMALL_TABLE = (0, 0, 1, 3, 4, 4, 5, 9, 10, 11, 15, 16, 20, 21, 30, 33, 33)        # rows 36, T 3, n 17: duplicates, gaps, both ends
# rows 272, T 16, n 257 (n * T = 4112 >= 4096): pairs of duplicates, gaps, first start 0, last start rows - T = 256
BIG_TABLE = tuple(sorted((7 * w * w + 3 * w) % 257 for w in range(256))) + (256,)


def real_widths():
    """S 34, H 102, rows 66, T 24 and the table of two clean segments (an outage at rows 30-33)."""
    from windgnn_amd.series import segment_starts
    return 34, 102, 66, 24, tuple(segment_starts([(0, 30), (34, 32)], 24))


def fwd_ks(H):
    return next(k for k in FWD_KS if 4 * k >= H)


def bwd_ks3(H):
    return next(k for k in BWD_KS3 if 4 * k >= 3 * H)


def first_h(K):
    """The smallest H that selects the forward instance K (and, bracket for bracket, the BPTT instance)."""
    i = FWD_KS.index(K)
    return 1 if i == 0 else 4 * FWD_KS[i - 1] + 1


# seed per case, chosen on the CPU (tests/test_series_at_host.py re-checks): no ReLU pre-activation within 1e-5 of zero, and for
# the irregular case the two planted mistakes visible a hundred times above the bar
SEEDS = {"irregular": 1, "real_widths": 4, "K4_big": 13, "K8_big": 6, "K12_small": 1, "K20_big": 5, "K26_big": 2}   # others: 0
INSTANCE_CASES = {}         # id -> (S, H, rows, T, starts, seed)
for _K in FWD_KS:
    INSTANCE_CASES["K%d_small" % _K] = (3, 4 * _K, 36, 3, SMALL_TABLE, SEEDS.get("K%d_small" % _K, 0))
    INSTANCE_CASES["K%d_big" % _K] = (3, first_h(_K), 272, 16, BIG_TABLE, SEEDS.get("K%d_big" % _K, 0))
del _K


def case(cid):
    if cid == "irregular":
        return IRREGULAR + (SEEDS[cid],)
    if cid == "real_widths":
        return real_widths() + (SEEDS[cid],)
    return INSTANCE_CASES[cid]


class Ref:
    pass


def windows_at(series, T, starts):
    return torch.stack([series[s:s + T] for s in starts])


def covered_rows(rows, T, starts):
    hit = torch.zeros(rows, dtype=torch.bool)
    for s in starts:
        hit[s:s + T] = True
    return hit


@functools.lru_cache(maxsize=None)
def reference(cid):
    """Host tensors of a case and the fp64 oracle's results on the materialised windows, for every route: computed once, shared,
    never modified."""
    from oracle import windgnn_oracle as orc
    S, H, rows, T, starts, seed = case(cid)
    n = len(starts)
    assert all(0 <= s <= rows - T for s in starts) and list(starts) == sorted(starts)
    r = Ref()
    r.id, r.S, r.H, r.rows, r.T, r.n, r.starts, r.seed = cid, S, H, rows, T, n, list(starts), seed
    r.A, r.feat, r.dY, r.p = _draw(S, H, rows, T, 1, n, seed)
    r.Xs = r.feat[:rows].contiguous()
    g = torch.Generator().manual_seed(7700 + 131 * seed + S * 7 + rows + H)
    r.Ls = torch.rand(rows, H, generator=g)
    r.Ls[~covered_rows(rows, T, starts)] = SPARE
    r.X, r.L = windows_at(r.Xs, T, starts), windows_at(r.Ls, T, starts)
    assert float(r.L.max()) < 1.0
    A, X, r.p64 = r.A.double(), r.X.double(), {k: v.double() for k, v in r.p.items()}
    r.margin = preact_margin(A, r.Xs.double().unsqueeze(0), r.p64)
    r.Yo, cache = orc.forward(A, X, r.p64)
    r.go = orc.backward(A, X, r.p64, r.Yo, cache, r.dY.double())
    r.last_o = r.Yo[:, -1, :] * (WIND_MAX - WIND_MIN) + WIND_MIN
    _, loss, r.gm = orc.train_step(A, X, r.L.double(), r.p64)
    r.loss_o = float(loss)
    return r
