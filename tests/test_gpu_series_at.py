"""Series mode on a table of window starts, on the MI355X (include/windgnn_series_at.h, windgnn_amd/series.py, GCN_GRU.forward_series
and TrainStep.step_series with starts=) against the fp64 oracle on the MATERIALISED windows X[w, t] = Xs[starts[w] + t], at the
project's bar for fp32-grade modes: conftest.rel_to_max <= 1e-4 on Y, the de-normalised last rows and each of the 8 gradients,
the loss relative to the oracle's loss.  The observed errors are printed per case.

Cases, tables, seeds and references are tests/series_at_cases.py's; tests/test_series_at_host.py qualifies them on the CPU (ReLU
margins, planted mistakes).  The C entry points are called directly on buffers of exactly their ABI lengths inside a
guarded.Arena -- the label series has exactly `rows` rows, and every label row no window covers holds 1e3 -- under the library's
profiler, so a case also proves by the launched names that the table instances and series_fold_at_kernel ran."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import series_at_cases as sc
from conftest import PARAM_KEYS, rel_to_max
from guarded import FILLS, Arena
from test_gpu_series import ALL, F, STATUS, TOL, WIND_MAX, WIND_MIN, _case, _dev, _fit
from test_gpu_series_train import TOL as LOSS_TOL
from test_gpu_series_train import _train

pytestmark = pytest.mark.gpu

WINDOW_START = 16                      # WGNN_STATUS_WINDOW_START
ROUTES = ("last", "series", "mse")     # wgnn_series_fwd_last_at | _fwd_at + _bwd_at | _fwd_loss_at + _bwd_mse_at


def _arena_step(r, fill="nan", dirty=None, table=None, status=0, routes=ROUTES, gate=None):
    """The five table entry points on the reference r inside an arena.  table: the int32 table to pass (default: r's own);
    status: the bits every call must leave in the status word (it is zeroed again after each).  Returns (outputs as host bytes
    per route, launched names, final scratch bytes).  gate (tests/stream_cases.py): the calls go to its side stream, nothing
    is read or synchronised in between (so "series" and "mse", which share Y and the gradients, do not go together), no kernel
    names are collected, and guards and status word are looked at once, at the end."""
    from windgnn_amd import _lib as L
    lib = L.load()
    assert gate is None or not ("series" in routes and "mse" in routes)
    n, T, H, rows = r.n, r.T, r.H, r.rows
    sd = L.SeriesDims(rows, T, 0, n, r.S, F, H, 0, 0, 0, 0)
    ws_bytes, st_bytes = lib.wgnn_series_at_workspace_bytes(C.byref(sd)), lib.wgnn_series_at_stash_bytes(C.byref(sd))
    lb_bytes = lib.wgnn_series_at_loss_bytes(C.byref(sd))
    assert ws_bytes > STATUS and st_bytes > 0 and lb_bytes == 4 * (2 * -(-n // 16) + 4)
    a = Arena(_dev(), fill)
    dirty = dirty or {}

    def add(name, t=None, shape=None):
        return a.buf(name, (t.numel() if t is not None else int(np.prod(shape))) * 4, data=t)

    add("A", r.A)
    add("Xs", r.Xs)
    add("dY", r.dY)
    add("Ls", r.Ls)                                        # exactly rows rows: a read past them hits the guard
    add("starts", torch.tensor(r.starts if table is None else table, dtype=torch.int32))
    for k in PARAM_KEYS:
        add("p." + k, r.p[k])
        add("g." + k, shape=r.p[k].shape)
    add("Y", shape=(n, T, H))
    add("last", shape=(n, H))
    add("loss", shape=(1,))
    for name, nbytes in (("stash", st_bytes), ("loss_buf", lb_bytes)):
        a.buf(name, nbytes, data=_fit(dirty[name], nbytes) if name in dirty else None)
    a.buf("ws", ws_bytes, data=_fit(dirty["ws"], ws_bytes) if "ws" in dirty else None, zero_head=STATUS)
    a.commit()
    P = lambda name: C.c_void_p(a[name].ptr)   # noqa: E731
    ps, gs = L.Params(), L.Grads()
    for (field, _), k in zip(L.Grads._fields_, PARAM_KEYS):
        setattr(ps, field, a["p." + k].ptr)
        setattr(gs, field, a["g." + k].ptr)
    word = a["ws"].view(torch.int32)
    st = gate.handle if gate is not None else None
    if gate is not None:
        gate.begin(a, ints=("starts",))

    def after(what):
        if gate is not None:
            gate.repoison(a["ws"], STATUS)
            return
        torch.cuda.synchronize()
        assert a.check() == {}, (what, fill, a.check())
        assert int(word[0]) == status, (what, "status word", int(word[0]))
        word[0] = 0
        if "ws" not in dirty:
            a["ws"].poison()                               # the workspace carries nothing from one call to the next

    def call(name, *args):
        assert getattr(lib, name)(C.byref(sd), P("A"), P("Xs"), P("starts"), C.byref(ps), *args, P("ws"), ws_bytes, st) == 0, name
        after(name)

    def read(names):
        return (lambda: {name: a[name].host() for name in names}) if gate is not None else {name: a[name].host() for name in names}

    grads = ["g." + k for k in PARAM_KEYS]
    out = {}
    if gate is None:
        L.profile_enable(True)
    try:
        if "last" in routes:
            call("wgnn_series_fwd_last_at", WIND_MIN, WIND_MAX, P("last"))
            out["last"] = read(["last"])
        if "series" in routes:
            call("wgnn_series_fwd_at", P("Y"), P("stash"))
            call("wgnn_series_bwd_at", P("Y"), P("dY"), P("stash"), C.byref(gs))
            out["series"] = read(["Y"] + grads)
        if "mse" in routes:
            if gate is None:
                for name in ["Y"] + grads:
                    a[name].poison()
            call("wgnn_series_fwd_loss_at", P("Ls"), rows, P("Y"), P("stash"), P("loss_buf"))
            call("wgnn_series_bwd_mse_at", P("Y"), P("Ls"), rows, 1.0, P("stash"), P("loss_buf"), P("loss"), C.byref(gs))
            out["mse"] = read(["Y", "loss"] + grads)
        names = tuple(rec["name"] for rec in L.profile_read()) if gate is None else ()
    finally:
        if gate is None:
            L.profile_enable(False)
    if gate is not None:
        gate.close(a)
        out = {route: get() for route, get in out.items()}
        return out, names, {k: a[k].host() for k in ("stash", "ws", "loss_buf")}
    if fill != "zero" and not dirty and not status:
        for name in ["Y", "last", "loss"] + grads:
            assert a[name].unwritten(4) == 0, (name, fill, a[name].unwritten(4))
    for name in ("A", "Xs", "dY", "Ls", "starts") + tuple("p." + k for k in PARAM_KEYS):      # inputs are read only
        assert a[name].unwritten(1) == a[name].nbytes, name
    return out, names, {k: a[k].host() for k in ("stash", "ws", "loss_buf")}


def _f32(b, shape):
    return b.view(torch.float32).reshape(shape)


def _errors(r, out):
    err = {}
    if "last" in out:
        err["last"] = rel_to_max(_f32(out["last"]["last"], (r.n, r.H)), r.last_o)
    for route, ref in (("series", r.go), ("mse", r.gm)):
        if route not in out:
            continue
        o = out[route]
        err[route + ".Y"] = rel_to_max(_f32(o["Y"], (r.n, r.T, r.H)), r.Yo)
        if route == "mse":
            err["loss"] = abs(float(_f32(o["loss"], (1,))[0]) - r.loss_o) / r.loss_o
        for k in PARAM_KEYS:
            err[route + "." + k] = rel_to_max(_f32(o["g." + k], ref[k].shape), ref[k])
    return err


def _assert_bar(what, err):
    print("\n%s: " % what + "  ".join("%s %.2e" % kv for kv in err.items()))
    for k, e in err.items():
        assert e <= (LOSS_TOL if k == "loss" else TOL), (what, k, e)


def _assert_names(r, names):
    """The table instances of this H ran, with the fold and the check of the table, and no strided sibling did."""
    want = {"gru_fwd_kernel<%d,starts>" % sc.fwd_ks(r.H), "gru_bwd_kernel<%d,starts>" % sc.bwd_ks3(r.H), "series_fold_at_kernel",
            "series_starts_check_kernel"}
    assert want <= set(names), (want - set(names), names)
    rec = {x for x in names if x.startswith(("gru_fwd_kernel", "gru_bwd_kernel", "series_fold"))}
    assert rec == want - {"series_starts_check_kernel"}, rec


@functools.lru_cache(maxsize=None)
def _checked(cid):
    r = sc.reference(cid)
    assert r.margin > 1e-5, "a ReLU pre-activation within %.1e of zero (relative): pick another seed" % r.margin
    return r


# ---- same windows, same bits ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["ragged_wg", "cover_1_2", "gaps"])
def test_a_table_of_w_times_stride_gives_the_strided_entry_points_bits(cid):
    """starts[w] = w * stride: the arithmetic and the summation order are those of the strided kernels, so Y, the last rows, the
    loss and all 8 gradients of both backwards are torch.equal."""
    from windgnn_amd.series import (forward_last_series, series_backward_mse_raw, series_backward_raw, series_forward_loss_raw,
                                    series_forward_raw)
    from test_gpu_series import _model
    c, t = _case(cid), _train(cid)
    assert cid in ALL and c.starts == [w * c.stride for w in range(c.n)]
    dev = _dev()
    A, Xs, dY = c.A.to(dev), c.Xs.to(dev), c.dY.to(dev)
    Ls = t.Ls[:c.rows].to(dev).contiguous()
    assert Ls.shape[0] == c.rows
    params = [c.p[k].to(dev).contiguous() for k in PARAM_KEYS]
    model = _model(c)

    def run(at):
        kw = {"starts": c.starts} if at else {"n_windows": c.n}
        stride = None if at else c.stride
        Y, stash, sd, *tab = series_forward_raw(A, Xs, c.T, stride, params, **kw)
        g = [torch.full_like(q, float("nan")) for q in params]
        series_backward_raw(sd, A, Xs, params, Y, dY, stash, g, *tab)
        with torch.no_grad():
            last = forward_last_series(model, A, Xs, c.T, WIND_MIN, WIND_MAX, stride, **kw)
        Y2, stash2, loss_buf, sd2, *tab2 = series_forward_loss_raw(A, Xs, Ls, c.T, stride, params, **kw)
        g2 = [torch.full_like(q, float("nan")) for q in params]
        loss = torch.full((), float("nan"), device=dev)
        series_backward_mse_raw(sd2, A, Xs, params, Y2, Ls, stash2, loss_buf, g2, loss, 1.0, None, *tab2)
        return [Y, last, Y2, loss] + g + g2

    strided, table = run(False), run(True)
    assert not torch.isnan(strided[3]).item()
    for i, (u, v) in enumerate(zip(strided, table)):
        assert u.shape == v.shape and torch.equal(u, v), (cid, i, float((u - v).abs().max()))


# ---- oracle parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", ["irregular", "real_widths"])
def test_table_matches_the_oracle_on_the_materialised_windows(cid):
    r = _checked(cid)
    out, names, _ = _arena_step(r)
    _assert_names(r, names)
    _assert_bar(cid, _errors(r, out))
    assert torch.equal(out["series"]["Y"], out["mse"]["Y"])       # the statistics do not enter h


@pytest.mark.parametrize("cid", list(sc.INSTANCE_CASES))
def test_every_instance(cid):
    r = _checked(cid)
    # dGHn and the [Hprev | 1] rows, or dGH whole (tests/test_series_at_host.py: the stash holds the rows exactly then)
    assert (r.n * r.T >= 4096) == cid.endswith("_big")
    out, names, _ = _arena_step(r)
    _assert_names(r, names)
    _assert_bar(cid, _errors(r, out))


# ---- footprint -------------------------------------------------------------------------------------------------------------
def test_footprint_guards_fills_and_dirty_scratch():
    r = _checked("irregular")
    assert FILLS[0] == "zero"
    base, _, _ = _arena_step(r, FILLS[0])
    _assert_bar("arena zero", _errors(r, base))
    flat = lambda out: {(route, k): v for route, o in out.items() for k, v in o.items()}   # noqa: E731
    for fill in FILLS[1:]:
        out, _, _ = _arena_step(r, fill)
        for key, v in flat(out).items():
            assert torch.equal(v, flat(base)[key]), (key, fill)
    _, _, left = _arena_step(_checked("K8_small"), "nan")        # scratch another shape's calls left behind
    for fill in ("finite", "nan"):
        out, _, _ = _arena_step(r, fill, dirty=left)
        for key, v in flat(out).items():
            assert torch.equal(v, flat(base)[key]), (key, fill, "dirty")


# ---- a bad table: reported, in bounds ------------------------------------------------------------------------------------------
def _bad_tables(r):
    past, negative, descending = list(r.starts), list(r.starts), list(r.starts)
    past[-1] = r.rows - r.T + 1
    negative[0] = -1
    descending[3], descending[6] = descending[6], descending[3]
    assert descending != sorted(descending) and min(descending) >= 0 and max(descending) <= r.rows - r.T
    return {"past": past, "negative": negative, "descending": descending}


@pytest.mark.parametrize("which", ["past", "negative", "descending"])
def test_a_bad_table_is_reported_and_stays_in_bounds(which):
    """Every entry point returns WGNN_OK, sets WGNN_STATUS_WINDOW_START and leaves every guard band and every input as it was
    (_arena_step asserts all three after each call); the values of the outputs are unspecified."""
    r = _checked("irregular")
    _arena_step(r, "nan", table=_bad_tables(r)[which], status=WINDOW_START)


def test_the_python_layer_raises_for_a_bad_device_table():
    from windgnn_amd.functional import check_range_status
    from windgnn_amd.series import series_forward_raw
    r = _checked("irregular")
    dev = _dev()
    params = [r.p[k].to(dev).contiguous() for k in PARAM_KEYS]
    check_range_status(dev)
    for table in _bad_tables(r).values():
        bad = torch.tensor(table, dtype=torch.int32, device=dev)          # a device table: checked by the kernel, not the host
        series_forward_raw(r.A.to(dev), r.Xs.to(dev), r.T, None, params, want_stash=False, starts=bad)
        with pytest.raises(RuntimeError, match=r"window starts") as e:
            check_range_status(dev)
        assert "fp16 planes" not in str(e.value)                          # the advice about the math modes is not for this bit
        check_range_status(dev)                                            # reported once
    with pytest.raises(ValueError, match=r"starts\[18\] = 36"):          # the same table from the host is refused before upload
        series_forward_raw(r.A.to(dev), r.Xs.to(dev), r.T, None, params, want_stash=False, starts=_bad_tables(r)["past"])


# ---- GCN_GRU.forward_series(starts=) in any order --------------------------------------------------------------------------------
def _model_of(r):
    from windgnn_amd import GCN_GRU
    m = GCN_GRU(13, 13, 13, r.S * 13, r.H, math="f32")
    m.load_state_dict({k: v.clone() for k, v in r.p.items()})
    return m.to(_dev())


def test_forward_series_takes_the_table_in_any_order():
    r = _checked("irregular")
    dev = _dev()
    A, Xs = r.A.to(dev), r.Xs.to(dev)
    model = _model_of(r)
    perm = torch.randperm(r.n, generator=torch.Generator().manual_seed(5)).tolist()
    assert perm != sorted(perm)

    def run(starts, dY):
        model.zero_grad()
        Y = model.forward_series(A, Xs, r.T, starts=starts)
        Y.backward(dY.to(dev))
        return Y.detach().cpu(), {k: q.grad.detach().cpu().clone() for k, q in model.named_parameters()}

    Ys, gs = run(r.starts, r.dY)
    err = {"Y": rel_to_max(Ys, r.Yo)}
    err.update({k: rel_to_max(gs[k], r.go[k]) for k in PARAM_KEYS})
    _assert_bar("forward_series(starts)", err)
    shuffled = [r.starts[i] for i in perm]
    for table in (shuffled, torch.tensor(shuffled, device=dev), torch.tensor(shuffled, dtype=torch.int32)):
        Yp, gp = run(table, r.dY[perm])
        # duplicated starts are interchangeable windows: compare row by row with the sorted call's window of the same start
        assert torch.equal(Yp, torch.stack([Ys[r.starts.index(s)] for s in shuffled]))
        Y2, g2 = run(table, r.dY[perm])
        assert torch.equal(Y2, Yp)
        for k in PARAM_KEYS:
            assert torch.equal(g2[k], gp[k]), k                             # two runs: bit-identical
    # the parameter gradients do not depend on the order: the kernels see the sorted table and dY's rows in its order (a
    # stable sort keeps duplicates in the caller's order, so give every duplicate pair the same dY rows)
    dY = r.dY.clone()
    for w in range(1, r.n):
        if r.starts[w] == r.starts[w - 1]:
            dY[w] = dY[w - 1]
    _, g_sorted = run(r.starts, dY)
    _, g_perm = run(torch.tensor(shuffled, device=dev), dY[perm])
    for k in PARAM_KEYS:
        assert torch.equal(g_perm[k], g_sorted[k]), k
    from windgnn_amd.series import forward_last_series
    with torch.no_grad():
        last = forward_last_series(model, A, Xs, r.T, WIND_MIN, WIND_MAX, starts=shuffled).cpu()
    assert rel_to_max(last, r.last_o[[r.starts.index(s) for s in shuffled]]) <= TOL


# ---- TrainStep.step_series(starts=) --------------------------------------------------------------------------------------------
STEPS = 3


@functools.lru_cache(maxsize=None)
def _trajectory(cid):
    from oracle import windgnn_oracle as orc
    r = _checked(cid)
    p = dict(r.p64)
    state = orc.adam_init(p)
    losses, g1 = [], None
    for _ in range(STEPS):
        _, loss, g = orc.train_step(r.A.double(), r.X.double(), r.L.double(), p)
        g1 = g if g1 is None else g1
        losses.append(float(loss))
        p = orc.adam_step(p, g, state)
    return losses, g1, p


def _steps(r, tr, starts, steps=STEPS):
    dev = _dev()
    A, Xs, Ls = r.A.to(dev), r.Xs.to(dev), r.Ls.to(dev)
    losses = []
    for _ in range(steps):
        loss, Y = tr.step_series(A, Xs, Ls, r.T, starts=starts)
        assert tuple(Y.shape) == (r.n, r.T, r.H) and loss.dim() == 0
        losses.append(float(loss))
    return losses


def test_three_steps_on_a_shuffled_table_follow_the_oracle_trajectory():
    from windgnn_amd.trainer import TrainStep
    r = _checked("irregular")
    lo, _, po = _trajectory("irregular")
    model = _model_of(r)
    tr = TrainStep(model)
    perm = torch.randperm(r.n, generator=torch.Generator().manual_seed(6)).tolist()
    losses = _steps(r, tr, torch.tensor([r.starts[i] for i in perm], device=_dev()))
    assert tr.steps == STEPS
    seen = {k: rel_to_max(q.detach().cpu(), po[k]) for k, q in model.named_parameters()}
    for i, (a, b) in enumerate(zip(losses, lo)):
        seen["loss%d" % (i + 1)] = abs(a - b) / b
    _assert_bar("step_series(starts) x3", seen)


def test_max_grad_norm_and_keep_best_are_reachable():
    from windgnn_amd.trainer import TrainStep
    r = _checked("irregular")
    lo, g1, _ = _trajectory("irregular")
    norm_o = float(torch.sqrt(sum((g.double() ** 2).sum() for g in g1.values())))
    tr = TrainStep(_model_of(r), max_grad_norm=0.5 * norm_o, keep_best=True)
    loss = _steps(r, tr, r.starts, steps=1)[0]
    norm, coef = float(tr.grad_norm), float(tr.clip_coef)
    print("\ngrad_norm %.6e (oracle %.6e)  clip_coef %.6f" % (norm, norm_o, coef))
    assert abs(norm - norm_o) <= TOL * norm_o and coef < 1 and abs(coef - 0.5 * norm_o / (norm_o + 1e-6)) <= TOL
    assert int(tr.best_step) == 1 and float(tr.best_loss) == loss and abs(loss - lo[0]) <= TOL * lo[0]
    loss, Y = tr.forward_backward_series(r.A.to(_dev()), r.Xs.to(_dev()), r.Ls.to(_dev()), r.T, starts=r.starts)
    assert tr.steps == 1 and tuple(Y.shape) == (r.n, r.T, r.H)
