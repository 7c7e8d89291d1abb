"""Every instance the series entry points can select, on the MI355X: one case per key of instance_cases.SERIES_FAMILIES -- gru.hip's
gru_fwd_kernel<K, false, SeriesRows> in its three call forms and gru_bwd_kernel<K3, SeriesRows> in its four, for all nine K,
and series_fold_kernel at its three coverage patterns.  A case runs one series step under the library's profiler, proves by the
launched names that its K ran behind a wgnn_series_* entry point (with exactly the siblings instance_cases.series_plan says), and
holds Y (or the de-normalised last rows), the loss and the 8 gradients to the fp64 oracle on the MATERIALISED windows
X[w, t] = Xs[w * stride + t] at the series suites' own bars, imported: conftest.rel_to_max <= TOL each, the loss relative to the
oracle's loss.  The observed errors are printed per case.

Inputs: tests/test_gpu_series.py's _draw with the seed of the table; for the MSE route a random label series [rows + 5, H] in
[0, 1) whose rows past (n - 1) * stride + T -- which no window covers -- hold tests/test_gpu_series_train.py's SPARE (1e3: read
once, such a row moves the loss far past the bar).  reference() needs no GPU; tests/test_instance_table_host.py measures the
input conditions on it.

The calls are the C entry points the raw wrappers of windgnn_amd/series.py call, made directly because those wrappers allocate
Y, the stash and loss_buf themselves: here every buffer has exactly its ABI length inside a guarded.Arena filled with NaN words,
the workspace is poisoned again between the forward and the backward, the guard bands must come back intact and no output
word may keep its poison.  Cases that share the call form share the GPU step (functools.lru_cache)."""
import ctypes as C
import functools
import re

import numpy as np
import pytest
import torch

import instance_cases as ic
from conftest import PARAM_KEYS, rel_to_max
from guarded import Arena
from test_gpu_series import F, STATUS, TOL, WIND_MAX, WIND_MIN, _draw, preact_margin
from test_gpu_series_train import SPARE
from test_gpu_series_train import TOL as LOSS_TOL

pytestmark = pytest.mark.gpu

LS_EXTRA = 5            # label rows past the series' own (ls_rows > rows): all of them hold SPARE
TABLED = (set(ic.FAMILIES) | set(ic.SERIES_FAMILIES)) - {"pgemm_tn2_kernel"}      # kernel base names


class Ref:
    pass


def windows(series, T, stride, n, first=0):
    """The materialised windows [n, T, ...] of a series: window w = rows first + w * stride .. + T - 1."""
    return torch.stack([series[first + w * stride:first + w * stride + T] for w in range(n)])


@functools.lru_cache(maxsize=None)
def reference(S, H, rows, T, stride, n, seed):
    """Host tensors of a shape and the fp64 oracle's results on the materialised windows, for every route: computed once,
    shared, never modified."""
    from oracle import windgnn_oracle as orc
    r = Ref()
    r.S, r.H, r.rows, r.T, r.stride, r.n = S, H, rows, T, stride, n
    r.need = (n - 1) * stride + T
    assert r.need <= rows
    r.A, r.feat, r.dY, r.p = _draw(S, H, rows, T, stride, n, seed)
    r.Xs = r.feat[:rows].contiguous()
    g = torch.Generator().manual_seed(5300 + 131 * seed + S * 7 + rows + H)
    r.Ls = torch.rand(rows + LS_EXTRA, H, generator=g)
    r.Ls[r.need:] = SPARE
    r.X, r.L = windows(r.Xs, T, stride, n), windows(r.Ls, T, stride, n)
    A, X, p64 = r.A.double(), r.X.double(), {k: v.double() for k, v in r.p.items()}
    r.margin = preact_margin(A, r.Xs.double().unsqueeze(0), p64)
    r.Yo, cache = orc.forward(A, X, p64)
    r.go = orc.backward(A, X, p64, r.Yo, cache, r.dY.double())
    r.last_o = r.Yo[:, -1, :] * (WIND_MAX - WIND_MIN) + WIND_MIN
    _, loss, r.gm = orc.train_step(A, X, r.L.double(), p64)
    r.loss_o = float(loss)
    return r


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _step(S, H, rows, T, stride, n, seed, route):
    """One series step of this route on the GPU: the names it launched and its errors against the reference (floats only)."""
    from windgnn_amd import _lib as L
    lib = L.load()
    r = reference(S, H, rows, T, stride, n, seed)
    assert r.margin > 1e-5, "a ReLU pre-activation within %.1e of zero (relative): pick another seed" % r.margin
    sd = L.SeriesDims(rows, T, stride, n, S, F, H, 0, 0, 0, 0)
    ws_bytes, st_bytes = lib.wgnn_series_workspace_bytes(C.byref(sd)), lib.wgnn_series_stash_bytes(C.byref(sd))
    lb_bytes = lib.wgnn_series_loss_bytes(C.byref(sd))
    assert ws_bytes > STATUS and st_bytes > 0 and lb_bytes > 0
    a = Arena(_dev(), "nan")

    def add(name, t=None, shape=None):
        return a.buf(name, (t.numel() if t is not None else int(np.prod(shape))) * 4, data=t)

    add("A", r.A)
    add("Xs", r.Xs)
    add("dY", r.dY)
    add("Ls", r.Ls)
    for k in PARAM_KEYS:
        add("p." + k, r.p[k])
        add("g." + k, shape=r.p[k].shape)
    add("Y", shape=(n, T, H))
    add("last", shape=(n, H))
    add("loss", shape=(1,))
    a.buf("stash", st_bytes)
    a.buf("loss_buf", lb_bytes)
    a.buf("ws", ws_bytes, zero_head=STATUS)
    a.commit()
    P = lambda name: C.c_void_p(a[name].ptr)   # noqa: E731
    ps, gs = L.Params(), L.Grads()
    for (field, _), k in zip(L.Grads._fields_, PARAM_KEYS):
        setattr(ps, field, a["p." + k].ptr)
        setattr(gs, field, a["g." + k].ptr)
    ls_rows = r.Ls.shape[0]

    def after(what):
        torch.cuda.synchronize()
        assert a.check() == {}, (what, a.check())
        assert int(a["ws"].view(torch.int32)[0]) == 0, (what, "status word")

    def run():
        if route == "series_last":
            assert lib.wgnn_series_fwd_last(C.byref(sd), P("A"), P("Xs"), C.byref(ps), WIND_MIN, WIND_MAX, P("last"), P("ws"),
                                            ws_bytes, None) == 0
            after("wgnn_series_fwd_last")
            return ["last"]
        if route == "series":
            assert lib.wgnn_series_fwd(C.byref(sd), P("A"), P("Xs"), C.byref(ps), P("Y"), P("stash"), P("ws"), ws_bytes, None) == 0
            after("wgnn_series_fwd")
            a["ws"].poison()                               # the workspace carries nothing from the forward to the backward
            assert lib.wgnn_series_bwd(C.byref(sd), P("A"), P("Xs"), C.byref(ps), P("Y"), P("dY"), P("stash"), C.byref(gs),
                                       P("ws"), ws_bytes, None) == 0
            after("wgnn_series_bwd")
            return ["Y"] + ["g." + k for k in PARAM_KEYS]
        assert lib.wgnn_series_fwd_loss(C.byref(sd), P("A"), P("Xs"), C.byref(ps), P("Ls"), ls_rows, P("Y"), P("stash"),
                                        P("loss_buf"), P("ws"), ws_bytes, None) == 0
        after("wgnn_series_fwd_loss")
        a["ws"].poison()
        assert lib.wgnn_series_bwd_mse(C.byref(sd), P("A"), P("Xs"), C.byref(ps), P("Y"), P("Ls"), ls_rows, 1.0, P("stash"),
                                       P("loss_buf"), P("loss"), C.byref(gs), P("ws"), ws_bytes, None) == 0
        after("wgnn_series_bwd_mse")
        return ["Y", "loss"] + ["g." + k for k in PARAM_KEYS]

    L.profile_enable(True)
    try:
        outs = run()
        names = tuple(rec["name"] for rec in L.profile_read())
    finally:
        L.profile_enable(False)
    for name in outs:
        assert a[name].unwritten(4) == 0, (name, a[name].unwritten(4))
    for name in ("A", "Xs", "dY", "Ls") + tuple("p." + k for k in PARAM_KEYS):      # inputs are read only
        assert a[name].unwritten(1) == a[name].nbytes, name
    get = lambda name, shape: a[name].host().view(torch.float32).reshape(shape)   # noqa: E731
    err = {}
    if route == "series_last":
        err["last"] = rel_to_max(get("last", (n, H)), r.last_o)
        return names, err
    grads_o = r.go if route == "series" else r.gm
    err["Y"] = rel_to_max(get("Y", (n, T, H)), r.Yo)
    if route == "series_mse":
        err["loss"] = abs(float(get("loss", (1,))[0]) - r.loss_o) / r.loss_o
    for k in PARAM_KEYS:
        err[k] = rel_to_max(get("g." + k, grads_o[k].shape), grads_o[k])
    return names, err


def _check(case):
    fam, key, S, H, rows, T, stride, n, seed, route = case
    expected = ic.series_plan(S, H, rows, T, stride, n, route)
    assert key in expected, (key, expected)                    # (tests/test_instance_table_host.py checks this without a GPU)
    names, err = _step(S, H, rows, T, stride, n, seed, route)
    ran = sorted({x for x in names if re.match(r"[a-z0-9_]+", x).group(0) in TABLED})
    print("%s S%d H%d rows%d T%d stride%d n%d seed%d %s: %s" % (key, S, H, rows, T, stride, n, seed, route,
                                                                " ".join("%s=%.2e" % kv for kv in err.items())))
    # the instance ran behind a series entry point, and so did exactly the siblings the two layouts imply
    assert ic.name_of(key) in ran, (key, ran)
    assert ran == sorted({ic.name_of(k) for k in expected}), (key, ran, expected)
    if route != "series_last":
        assert "series_fold_kernel" in ran, (key, ran)
    for what, e in err.items():
        assert e <= (LOSS_TOL if what == "loss" else TOL), (key, what, e)


def _family_test(fam):
    cases = [c for c in ic.SERIES_CASES if c[0] == fam]

    @pytest.mark.parametrize("case", cases, ids=[c[1] for c in cases])
    def test(case):
        _check(case)
    test.__name__ = test.__qualname__ = "test_series_" + fam
    return test


for _fam in ic.SERIES_FAMILIES:
    globals()["test_series_" + _fam] = _family_test(_fam)
del _fam
