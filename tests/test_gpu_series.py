"""Series mode on the GPU (include/windgnn_series.h, windgnn_amd/series.py) against the fp64 oracle on the MATERIALISED windows
X[w, t] = Xs[w * stride + t]: Y, the rolling-backtest rows and the 8 gradients for a random signed dY, at the project's bar
for fp32-grade modes (conftest.rel_to_max <= 1e-4 each; the observed maxima are printed and lie near 1e-6).

Inputs are drawn as the existing fixtures draw them (seeded torch.rand features; A from tests/golden/graph_7_34.npz, or
rand / S + 0.01 for other station counts; oracle.init_params).  Every seed below was checked on the CPU, and _case() asserts
it again: in the fp64 oracle the smallest |pre-activation| of either graph convolution is above 1e-5 of that layer's largest,
so no ReLU mask sits on a rounding boundary and a flipped mask cannot hide in, or be blamed on, the tolerance.

Which recurrence runs: series mode launches gru.hip's 16-window kernels (their SeriesRows instances) at EVERY n -- it does not
consult gru_small_supported -- so every case here runs them: forward, last_only and BPTT, with dGHn (n * T >= 4096) and with the
full dGH (below).  The thresholds it does consult are gemm32_nt_supported / gemm32_tn_supported (rows, resp. n * T, >= 4096:
csrc/gemm32.hip) in the front layout {1, rows} and in the recurrence layout {n, T}; THRESHOLD_CASES stands on both sides of
each, in each layout.  forward_last_series is produced by the last_only form of the recurrence kernel while predict_last is
another kernel, so it is held to the bar against the oracle, not to bit equality with predict_last(Y)."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PARAM_KEYS, max_abs, rel_to_max
from guarded import FILLS, Arena

pytestmark = pytest.mark.gpu

TOL = 1e-4
F = 13
STATUS = 256
WIND_MIN, WIND_MAX = 0.25, 31.5

# id -> (S, H, rows, T, stride, n, seed)
CASES = {
    "ragged_wg": (7, 21, 23, 5, 1, 17, 0),          # a ragged second workgroup, H no multiple of 16, two spare rows
    "cover_1_2": (7, 21, 14, 5, 3, 4, 0),           # coverage alternates between 1 and 2
    "disjoint": (3, 9, 12, 4, 4, 3, 0),             # non-overlapping windows
    "gaps": (7, 21, 13, 3, 5, 3, 0),                # rows no window covers: the fold's zero rows
    "T1": (3, 9, 6, 1, 1, 6, 0),
    "B1": (7, 21, 12, 12, 1, 1, 0),                 # the reference's B = 1 call shape
    "real_widths": (34, 102, 66, 24, 1, 40, 4),     # the model's real widths; few rows: the split-K projection GEMMs
}
# 4096 = the BT of gemm32_nt_supported / gemm32_tn_supported; rows decides the front layout, n * T the recurrence layout
THRESHOLD_CASES = {
    "rows802_nT2400": (7, 21, 802, 3, 1, 800, 68),        # both below (and n > 768: past gru_small_supported, which is not consulted)
    "rows1367_nT4095": (7, 21, 1367, 3, 1, 1365, 141),     # recurrence layout one row block below ...
    "rows1368_nT4098": (7, 21, 1368, 3, 1, 1366, 13),     # ... and just above: dGHn + [Hprev | 1] rows, front still small
    "rows4094_nT8186": (7, 21, 4094, 2, 1, 4093, 2538),  # front layout below (no tie-free seed among 20000 at 4095 rows), recurrence above
    "rows4096_nT8190": (7, 21, 4096, 2, 1, 4095, 10434),     # front layout at the threshold
    "rows4100_nT8198": (7, 21, 4100, 2, 1, 4099, 5300),     # both above
    "rows4096_nT2048": (7, 21, 4096, 2, 4, 1024, 10434),     # front above, recurrence below
}
ALL = dict(CASES, **THRESHOLD_CASES)


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def preact_margin(A, X, p):
    """min |Z| / max |Z| over the pre-activations of conv1 and of conv2 (the smaller of the two layers' ratios), in fp64."""
    from oracle import windgnn_oracle as orc
    Z1 = torch.matmul(torch.matmul(A, X), p["conv1.weight"]) + p["conv1.bias"]
    H1, _ = orc.gcn_layer_fwd(A, X, p["conv1.weight"], p["conv1.bias"])
    Z2 = torch.matmul(torch.matmul(A, H1), p["conv2.weight"]) + p["conv2.bias"]
    return min(float(Z.abs().min() / Z.abs().max()) for Z in (Z1, Z2))


class Case:
    pass


def _draw(S, H, rows, T, stride, n, seed):
    """(A, feat [rows + 3, S, 13], dY, params) of a case, seeded."""
    from oracle import windgnn_oracle as orc
    g = torch.Generator().manual_seed(9100 + 131 * seed + S * 7 + rows + H)
    if S in (7, 34):
        A = torch.from_numpy(np.load(os.path.join(GOLDEN, "graph_7_34.npz"))["A%d" % S]).float()
    else:
        A = torch.rand(S, S, generator=g) / S + 0.01
    feat = torch.rand(rows + 3, S, F, generator=g)                   # three more hours: the labels of the last window
    dY = (torch.rand(n, T, H, generator=g) * 2 - 1) * 1e-2           # random, signed
    return A, feat, dY, orc.init_params(S, F, H, seed=S + H + seed)


@functools.lru_cache(maxsize=None)
def _case(cid):
    """Host tensors of a case and its fp64 oracle results on the materialised windows: computed once, shared, never modified."""
    from oracle import windgnn_oracle as orc
    S, H, rows, T, stride, n, seed = ALL[cid]
    assert (n - 1) * stride + T <= rows
    c = Case()
    c.id, c.S, c.H, c.rows, c.T, c.stride, c.n = cid, S, H, rows, T, stride, n
    c.A, c.feat, c.dY, c.p = _draw(S, H, rows, T, stride, n, seed)
    c.Xs = c.feat[:rows].contiguous()
    p64 = {k: v.double() for k, v in c.p.items()}
    margin = preact_margin(c.A.double(), c.Xs.double().unsqueeze(0), p64)
    assert margin > 1e-5, "case %s: a ReLU pre-activation within %.1e of zero (relative): pick another seed" % (cid, margin)
    c.starts = [w * stride for w in range(n)]
    c.X = torch.stack([c.Xs[s:s + T] for s in c.starts])             # the materialised windows [n, T, S, 13]
    c.Yo, cache = orc.forward(c.A.double(), c.X.double(), p64)
    c.go = orc.backward(c.A.double(), c.X.double(), p64, c.Yo, cache, c.dY.double())
    c.last_o = c.Yo[:, -1, :] * (WIND_MAX - WIND_MIN) + WIND_MIN
    return c


def _model(c, math="f32"):
    from windgnn_amd import GCN_GRU
    m = GCN_GRU(13, 13, 13, c.S * 13, c.H, math=math)
    m.load_state_dict({k: v.clone() for k, v in c.p.items()})
    return m.to(_dev())


def _run(c, model=None):
    """(Y, grads) through GCN_GRU.forward_series and autograd, on the CPU."""
    dev = _dev()
    model = model or _model(c)
    model.zero_grad()
    Y = model.forward_series(c.A.to(dev), c.Xs.to(dev), c.T, c.stride, n_windows=c.n)
    assert tuple(Y.shape) == (c.n, c.T, c.H)
    Y.backward(c.dY.to(dev))
    return Y.detach().cpu(), {k: q.grad.detach().cpu().clone() for k, q in model.named_parameters()}


@pytest.mark.parametrize("cid", list(ALL))
def test_series_matches_the_oracle_on_the_materialised_windows(cid):
    from windgnn_amd.series import forward_last_series
    c = _case(cid)
    model = _model(c)
    Y, grads = _run(c, model)
    seen = {"Y": rel_to_max(Y, c.Yo)}
    with torch.no_grad():
        last = forward_last_series(model, c.A.to(_dev()), c.Xs.to(_dev()), c.T, WIND_MIN, WIND_MAX, c.stride, n_windows=c.n).cpu()
    assert tuple(last.shape) == (c.n, c.H)
    seen["last"] = rel_to_max(last, c.last_o)
    for k in PARAM_KEYS:
        seen[k] = rel_to_max(grads[k], c.go[k])
    print("\n%s: " % cid + "  ".join("%s %.2e" % kv for kv in seen.items()))
    for k, e in seen.items():
        assert e <= TOL, (cid, k, e)


def test_disjoint_windows_equal_the_materialised_path():
    """stride = T: the windows are make_windows' own; GCN_GRU.forward on them meets the same bar, and series mode agrees with it
    to twice the bar."""
    from windgnn_amd.data import make_windows
    c = _case("disjoint")
    dev = _dev()
    model = _model(c)
    X, L = make_windows(c.feat.to(dev), c.T)
    assert X.shape[0] >= c.n and torch.equal(X[:c.n].cpu(), c.X)
    model.zero_grad()
    Ym = model(c.A.to(dev), X[:c.n].contiguous())
    Ym.backward(c.dY.to(dev))
    gm = {k: q.grad.detach().cpu().clone() for k, q in model.named_parameters()}
    Y, gs = _run(c, model)
    assert rel_to_max(Ym.detach().cpu(), c.Yo) <= TOL and rel_to_max(Y, Ym.detach().cpu()) <= TOL
    for k in PARAM_KEYS:
        assert rel_to_max(gm[k], c.go[k]) <= TOL and rel_to_max(gs[k], gm[k]) <= TOL, k


@pytest.mark.parametrize("cid", ["ragged_wg", "rows4100_nT8198"])
def test_two_runs_are_bit_identical(cid):
    c = _case(cid)
    model = _model(c)
    Y1, g1 = _run(c, model)
    Y2, g2 = _run(c, model)
    assert torch.equal(Y1, Y2)
    for k in PARAM_KEYS:
        assert torch.equal(g1[k], g2[k]), k


def test_three_adam_steps_follow_the_oracle_trajectory():
    """loss.backward() + torch.optim.Adam through forward_series and series_labels, against the oracle's train_step + adam_step
    on the materialised windows and labels: the parameters after 3 steps at the bar."""
    from oracle import windgnn_oracle as orc
    from windgnn_amd.series import n_series_windows, series_labels
    c = _case("cover_1_2")
    assert c.H == 3 * c.S
    dev = _dev()
    assert n_series_windows(c.rows, c.T, c.stride) == c.n            # (so n_windows is not needed below)
    Ls, L = series_labels(c.feat, c.T, c.stride, n_windows=c.n)
    Lo = torch.stack([torch.cat([c.feat[s + k + 1:s + k + 1 + c.T, :, 11] for k in range(3)], dim=1) for s in c.starts])
    assert torch.equal(L, Lo)
    p = {k: v.double() for k, v in c.p.items()}
    state = orc.adam_init(p)
    for _ in range(3):
        _, _, g = orc.train_step(c.A.double(), c.X.double(), Lo.double(), p)
        p = orc.adam_step(p, g, state)
    model = _model(c)
    opt = torch.optim.Adam(model.parameters(), lr=1e-3)
    loss_fn = torch.nn.MSELoss()
    A, Xs = c.A.to(dev), c.Xs.to(dev)
    _, Ld = series_labels(c.feat.to(dev), c.T, c.stride, n_windows=c.n)
    for _ in range(3):
        opt.zero_grad()
        loss = loss_fn(model.forward_series(A, Xs, c.T, c.stride), Ld)
        loss.backward()
        opt.step()
    seen = {k: rel_to_max(q.detach().cpu(), p[k]) for k, q in model.named_parameters()}
    print("\nadam x3: " + "  ".join("%s %.2e" % kv for kv in seen.items()))
    for k, e in seen.items():
        assert e <= TOL, (k, e)
        assert max_abs(model.state_dict()[k].cpu(), c.p[k]) > 0          # the step moved it


def test_error_paths_raise_with_the_reason():
    from windgnn_amd import GCN_GRU
    from windgnn_amd.graph import CsrAdjacency, build_knn_adjacency, synthetic_station_coords
    from windgnn_amd.series import forward_last_series
    c = _case("cover_1_2")
    dev = _dev()
    A, Xs = c.A.to(dev), c.Xs.to(dev)
    model = _model(c)
    with pytest.raises(RuntimeError, match=r"requires_grad"):
        model.forward_series(A, Xs.clone().requires_grad_(True), c.T, c.stride)
    with pytest.raises(RuntimeError, match=r"requires_grad"):
        model.forward_series(A.clone().requires_grad_(True), Xs, c.T, c.stride)
    other = GCN_GRU(7, 9, 13, c.S * 13, c.H).to(dev)
    with pytest.raises(RuntimeError, match=r"13 / 13.*make_windows"):
        other.forward_series(A, torch.rand(c.rows, c.S, 7, device=dev), c.T, c.stride)
    with pytest.raises(RuntimeError, match=r"exact fp32.*make_windows"):
        _model(c, "f16x3").forward_series(A, Xs, c.T, c.stride)
    csr = CsrAdjacency(*build_knn_adjacency(synthetic_station_coords(c.S, seed=3), 3)).to(dev)
    with pytest.raises(RuntimeError, match=r"dense adjacency.*make_windows"):
        model.forward_series(csr, Xs, c.T, c.stride)
    with pytest.raises(RuntimeError, match=r"dense adjacency.*make_windows"):
        forward_last_series(model, csr, Xs, c.T, 0.0, 1.0, c.stride)
    with pytest.raises(RuntimeError, match=r"no window of"):
        model.forward_series(A, Xs[:c.T - 1], c.T, c.stride)
    with pytest.raises(RuntimeError, match=r"holds 1 \.\. %d windows" % c.n):
        model.forward_series(A, Xs, c.T, c.stride, n_windows=c.n + 1)
    wide = GCN_GRU(13, 13, 13, c.S * 13, 129).to(dev)                       # H = 129: refused by the library, named here
    with pytest.raises(RuntimeError, match=r"make_windows.*not supported"):
        wide.forward_series(A, Xs, c.T, c.stride)


# ---- footprint: every entry point inside guarded arenas --------------------------------------------------------------------
def _fit(src, n):
    src = src.reshape(-1)
    return src.repeat((n + src.numel() - 1) // src.numel())[:n].contiguous()


def _arena_run(c, fill, dirty=None, gate=None):
    """wgnn_series_fwd, wgnn_series_bwd (on a re-poisoned workspace) and wgnn_series_fwd_last on buffers of exactly their ABI
    lengths.  Returns (outputs on the CPU, the final stash and workspace bytes).  gate (tests/stream_cases.py): the calls go
    to its side stream, nothing synchronises in between, and guards and status word are looked at once, at the end."""
    from windgnn_amd import _lib as L
    lib = L.load()
    sd = L.SeriesDims(c.rows, c.T, c.stride, c.n, c.S, F, c.H, 0, 0, 0, 0)
    ws_bytes, st_bytes = lib.wgnn_series_workspace_bytes(C.byref(sd)), lib.wgnn_series_stash_bytes(C.byref(sd))
    assert ws_bytes > STATUS and st_bytes > 0
    a = Arena(_dev(), fill)
    dirty = dirty or {}

    def add(name, t=None, shape=None, **kw):
        n = (t.numel() if t is not None else int(np.prod(shape))) * 4
        return a.buf(name, n, data=t, **kw)

    add("A", c.A)
    add("Xs", c.Xs)
    add("dY", c.dY)
    for k in PARAM_KEYS:
        add("p." + k, c.p[k])
        add("g." + k, shape=c.p[k].shape)
    add("Y", shape=(c.n, c.T, c.H))
    add("last", shape=(c.n, c.H))
    a.buf("stash", st_bytes, data=_fit(dirty["stash"], st_bytes) if "stash" in dirty else None)
    a.buf("ws", ws_bytes, data=_fit(dirty["ws"], ws_bytes) if "ws" in dirty else None, zero_head=STATUS)
    a.commit()
    P = lambda name: C.c_void_p(a[name].ptr)
    ps, gs = L.Params(), L.Grads()
    for (field, _), k in zip(L.Grads._fields_, PARAM_KEYS):
        setattr(ps, field, a["p." + k].ptr)
        setattr(gs, field, a["g." + k].ptr)
    outs = ["Y", "last"] + ["g." + k for k in PARAM_KEYS]
    st = gate.handle if gate is not None else None
    if gate is not None:
        gate.begin(a)

    def after(what):
        if gate is not None:
            return
        torch.cuda.synchronize()
        assert a.check() == {}, (what, fill, a.check())
        assert int(a["ws"].view(torch.int32)[0]) == 0, (what, "status word")

    assert lib.wgnn_series_fwd(C.byref(sd), P("A"), P("Xs"), C.byref(ps), P("Y"), P("stash"), P("ws"), ws_bytes, st) == 0
    after("wgnn_series_fwd")
    if gate is not None:
        gate.repoison(a["ws"], STATUS)
    elif "ws" not in dirty:
        a["ws"].poison()                                   # the workspace carries nothing from the forward to the backward
    assert lib.wgnn_series_bwd(C.byref(sd), P("A"), P("Xs"), C.byref(ps), P("Y"), P("dY"), P("stash"), C.byref(gs), P("ws"),
                               ws_bytes, st) == 0
    after("wgnn_series_bwd")
    assert lib.wgnn_series_fwd_last(C.byref(sd), P("A"), P("Xs"), C.byref(ps), WIND_MIN, WIND_MAX, P("last"), P("ws"), ws_bytes,
                                    st) == 0
    after("wgnn_series_fwd_last")
    if gate is not None:
        gate.close(a)
    if fill != "zero" and not dirty:
        for name in outs:
            assert a[name].unwritten(4) == 0, (name, fill, a[name].unwritten(4))
    for name in ("A", "Xs", "dY") + tuple("p." + k for k in PARAM_KEYS):      # inputs are read only
        assert a[name].unwritten(1) == a[name].nbytes, name
    return {name: a[name].host() for name in outs}, {"stash": a["stash"].host(), "ws": a["ws"].host()}


def test_footprint_guards_fills_and_dirty_scratch():
    c = _case("cover_1_2")
    base, _ = _arena_run(c, FILLS[0])
    assert FILLS[0] == "zero"
    Y = base["Y"].view(torch.float32).reshape(c.n, c.T, c.H)
    assert rel_to_max(Y, c.Yo) <= TOL
    assert rel_to_max(base["last"].view(torch.float32).reshape(c.n, c.H), c.last_o) <= TOL
    for k in PARAM_KEYS:
        assert rel_to_max(base["g." + k].view(torch.float32).reshape(c.go[k].shape), c.go[k]) <= TOL, k
    for fill in FILLS[1:]:
        out, _ = _arena_run(c, fill)
        for name, v in out.items():
            assert torch.equal(v, base[name]), (name, fill)
    # scratch another shape's calls left behind (its stash and workspace bytes, tiled to this case's sizes)
    _, left = _arena_run(_case("ragged_wg"), "nan")
    for fill in ("finite", "nan"):
        out, _ = _arena_run(c, fill, dirty=left)
        for name, v in out.items():
            assert torch.equal(v, base[name]), (name, fill, "dirty")
