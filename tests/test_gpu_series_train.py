"""Series training on the GPU (include/windgnn_series_train.h, TrainStep.step_series) against the fp64 oracle's train_step (+
adam_step) on the MATERIALISED windows and labels, at the project's bar for fp32-grade modes (conftest.rel_to_max <= 1e-4 each;
the loss relative to the oracle's loss).  The observed maxima are printed.

Shapes, seeds and inputs are tests/test_gpu_series.py's (its _case asserts that no ReLU pre-activation sits on a rounding
boundary); the labels are series_labels(c.feat, T, stride, n_windows=n), c.feat having the three extra hours.  The raw pair is
always run on a label series whose rows past (n - 1) * stride + T -- which no window covers -- hold 1e3: read once, such a row
would move the loss (labels lie in [0, 1]) far past the bar."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import PARAM_KEYS, max_abs, rel_to_max
from guarded import FILLS, Arena
from test_gpu_series import F, _case, _dev, _fit, _model

pytestmark = pytest.mark.gpu

TOL = 1e-4
STATUS = 256
NO_LOSS_STATS = 8
SPARE = 1e3            # what the label rows no window covers hold
PARITY = ["ragged_wg", "cover_1_2", "gaps", "T1", "B1", "real_widths"]


class Train:
    pass


@functools.lru_cache(maxsize=None)
def _train(cid):
    """Host labels of a case and the fp64 oracle's training step on the materialised windows: computed once, shared, never
    modified."""
    from oracle import windgnn_oracle as orc
    from windgnn_amd.series import series_labels
    c = _case(cid)
    assert c.H == 3 * c.S
    t = Train()
    t.need = (c.n - 1) * c.stride + c.T
    Ls, L = series_labels(c.feat, c.T, c.stride, n_windows=c.n)
    assert Ls.shape == (c.rows, c.H) and L.shape == (c.n, c.T, c.H) and t.need <= c.rows
    t.L = L.contiguous()                                              # the materialised labels [n, T, H]
    t.Ls = torch.cat([Ls[:t.need], torch.full((c.rows - t.need + 5, c.H), SPARE)]).contiguous()   # spare rows: poison
    p64 = {k: v.double() for k, v in c.p.items()}
    Yo, t.loss_o, t.go = orc.train_step(c.A.double(), c.X.double(), t.L.double(), p64)
    assert max_abs(Yo, c.Yo) == 0
    t.loss_o = float(t.loss_o)
    return t


def _params(c, dev):
    return [c.p[k].to(dev).contiguous() for k in PARAM_KEYS]


def _raw(c, t, grad_scale=1.0, Ls=None):
    """wgnn_series_fwd_loss + wgnn_series_bwd_mse through the raw wrappers: (Y, loss, {grads}) on the CPU."""
    from windgnn_amd.series import series_backward_mse_raw, series_forward_loss_raw
    dev = _dev()
    A, Xs, Ls = c.A.to(dev), c.Xs.to(dev), (t.Ls if Ls is None else Ls).to(dev)
    params = _params(c, dev)
    grads = [torch.full_like(q, float("nan")) for q in params]
    loss = torch.full((), float("nan"), device=dev)
    Y, stash, loss_buf, sd = series_forward_loss_raw(A, Xs, Ls, c.T, c.stride, params, n_windows=c.n)
    assert tuple(Y.shape) == (c.n, c.T, c.H) and (sd.rows, sd.n) == (c.rows, c.n)
    series_backward_mse_raw(sd, A, Xs, params, Y, Ls, stash, loss_buf, grads, loss, grad_scale)
    return Y.cpu(), loss.cpu(), {k: g.cpu() for k, g in zip(PARAM_KEYS, grads)}


def _errors(c, t, Y, loss, grads, scale=1.0):
    seen = {"Y": rel_to_max(Y, c.Yo), "loss": abs(float(loss) - t.loss_o) / t.loss_o}
    for k in PARAM_KEYS:
        seen[k] = rel_to_max(grads[k], t.go[k] * scale)
    return seen


def _assert_bar(what, seen, tol=TOL):
    print("\n%s: " % what + "  ".join("%s %.2e" % kv for kv in seen.items()))
    for k, e in seen.items():
        assert e <= tol, (what, k, e)


@pytest.mark.parametrize("cid", PARITY)
def test_raw_pair_matches_the_oracle_training_step(cid):
    c, t = _case(cid), _train(cid)
    Y, loss, grads = _raw(c, t)
    _assert_bar(cid, _errors(c, t, Y, loss, grads))


@pytest.mark.parametrize("cid", ["ragged_wg", "gaps", "real_widths"])
def test_y_is_that_of_the_plain_series_forward_bit_for_bit(cid):
    from windgnn_amd.series import series_forward_loss_raw, series_forward_raw
    c, t = _case(cid), _train(cid)
    dev = _dev()
    A, Xs, params = c.A.to(dev), c.Xs.to(dev), _params(c, dev)
    Y0, _, _ = series_forward_raw(A, Xs, c.T, c.stride, params, n_windows=c.n)
    Y1, _, _, _ = series_forward_loss_raw(A, Xs, t.Ls.to(dev), c.T, c.stride, params, n_windows=c.n)
    assert torch.equal(Y0, Y1)                           # the statistics do not enter h


@pytest.mark.parametrize("cid", ["ragged_wg", "cover_1_2", "real_widths"])
def test_fused_loss_agrees_with_the_unfused_entry_points(cid):
    """wgnn_series_fwd + wgnn_mse_loss_grad on the contiguous materialised labels + wgnn_series_bwd: the same quantities at the
    bar (not bit for bit: the two form dY in different rounding orders)."""
    from windgnn_amd.functional import mse_loss_grad
    from windgnn_amd.series import series_backward_raw, series_forward_raw
    c, t = _case(cid), _train(cid)
    dev = _dev()
    A, Xs, params = c.A.to(dev), c.Xs.to(dev), _params(c, dev)
    Y0, stash0, sd = series_forward_raw(A, Xs, c.T, c.stride, params, n_windows=c.n)
    loss0, dY = mse_loss_grad(Y0, t.L.to(dev))
    g0 = [torch.empty_like(q) for q in params]
    series_backward_raw(sd, A, Xs, params, Y0, dY, stash0, g0)
    Y, loss, grads = _raw(c, t)
    seen = {"Y": max_abs(Y, Y0.cpu()), "loss": abs(float(loss) - float(loss0)) / float(loss0)}
    for k, g in zip(PARAM_KEYS, g0):
        seen[k] = rel_to_max(grads[k], g.cpu())
    assert seen["Y"] == 0
    _assert_bar(cid + " fused vs unfused", seen)
    _assert_bar(cid + " unfused vs oracle", _errors(c, t, Y0.cpu(), loss0.cpu(), dict(zip(PARAM_KEYS, [g.cpu() for g in g0]))))


def test_grad_scale_scales_the_gradients_and_not_the_loss():
    c, t = _case("ragged_wg"), _train("ragged_wg")
    Y1, loss1, _ = _raw(c, t)
    Y, loss, grads = _raw(c, t, grad_scale=0.25)
    _assert_bar("ragged_wg grad_scale 0.25", _errors(c, t, Y, loss, grads, scale=0.25))
    assert torch.equal(loss, loss1) and torch.equal(Y, Y1)


@pytest.mark.parametrize("cid", ["ragged_wg", "rows1368_nT4098"])
def test_two_runs_are_bit_identical(cid):
    c, t = _case(cid), _train(cid)
    assert cid == "ragged_wg" or c.n * c.T >= 4096
    Y1, loss1, g1 = _raw(c, t)
    Y2, loss2, g2 = _raw(c, t)
    assert torch.equal(Y1, Y2) and torch.equal(loss1, loss2) and not torch.isnan(loss1)
    for k in PARAM_KEYS:
        assert torch.equal(g1[k], g2[k]), k
    _assert_bar(cid, _errors(c, t, Y1, loss1, g1))


def test_backward_without_the_forwards_statistics_is_loud():
    """A loss_buf no wgnn_series_fwd_loss wrote (zeros: no tag): NaN loss and WGNN_STATUS_NO_LOSS_STATS in the status block of the
    workspace's window-major half -- an error path, as wgnn_bwd_mse_part(part | 8) on a stash without statistics."""
    from windgnn_amd import _lib as L
    from windgnn_amd.functional import _Workspace
    from windgnn_amd.series import series_backward_mse_raw, series_forward_loss_raw
    c, t = _case("cover_1_2"), _train("cover_1_2")
    dev = _dev()
    lib = L.load()
    A, Xs, Ls, params = c.A.to(dev), c.Xs.to(dev), t.Ls.to(dev), _params(c, dev)
    grads = [torch.empty_like(q) for q in params]
    loss = torch.zeros((), device=dev)
    Y, stash, loss_buf, sd = series_forward_loss_raw(A, Xs, Ls, c.T, c.stride, params, n_windows=c.n)
    off = lib.wgnn_series_status_offset(C.byref(sd))
    ws = _Workspace.get(dev, lib.wgnn_series_workspace_bytes(C.byref(sd)))
    word = ws[off:off + 4].view(torch.int32)
    word.zero_()                                     # kernels only OR into the block: the caller zeroes it once
    series_backward_mse_raw(sd, A, Xs, params, Y, Ls, stash, loss_buf, grads, loss)
    assert int(word.item()) & NO_LOSS_STATS == 0 and abs(float(loss) - t.loss_o) <= TOL * t.loss_o    # tagged: quiet
    series_backward_mse_raw(sd, A, Xs, params, Y, Ls, stash, torch.zeros_like(loss_buf), grads, loss)
    torch.cuda.synchronize()
    assert torch.isnan(loss).item()
    assert int(word.item()) & NO_LOSS_STATS
    assert int(ws[:4].view(torch.int32).item()) == 0             # the hour-major half's block is not involved
    word.zero_()
    assert lib.wgnn_strerror(-7).decode().count("loss statistics")   # what a binding that reads the word reports


# ---- TrainStep.step_series -------------------------------------------------------------------------------------------------
STEPS = 3


@functools.lru_cache(maxsize=None)
def _trajectory(cid):
    """The oracle's STEPS training steps with Adam on the materialised windows: (losses, gradients of step 1, parameters after)."""
    from oracle import windgnn_oracle as orc
    c, t = _case(cid), _train(cid)
    p = {k: v.double() for k, v in c.p.items()}
    state = orc.adam_init(p)
    losses, g1 = [], None
    for _ in range(STEPS):
        _, loss, g = orc.train_step(c.A.double(), c.X.double(), t.L.double(), p)
        g1 = g if g1 is None else g1
        losses.append(float(loss))
        p = orc.adam_step(p, g, state)
    return losses, g1, p


def _series_steps(c, t, tr, steps=STEPS, **kw):
    dev = _dev()
    A, Xs, Ls = c.A.to(dev), c.Xs.to(dev), t.Ls.to(dev)
    losses = []
    for _ in range(steps):
        loss, Y = tr.step_series(A, Xs, Ls, c.T, c.stride, n_windows=c.n, **kw)
        assert tuple(Y.shape) == (c.n, c.T, c.H) and loss.dim() == 0
        assert loss.data_ptr() == tr._gbuf.data_ptr() + 3 * 4        # the view of the bucket's header word
        losses.append(float(loss))
    return losses


def _param_errors(model, p):
    return {k: rel_to_max(q.detach().cpu(), p[k]) for k, q in model.named_parameters()}


def test_three_steps_follow_the_oracle_trajectory_and_the_materialised_step():
    from windgnn_amd.trainer import TrainStep
    c, t = _case("cover_1_2"), _train("cover_1_2")
    lo, _, po = _trajectory("cover_1_2")
    dev = _dev()
    model = _model(c)
    tr = TrainStep(model)
    losses = _series_steps(c, t, tr)
    assert tr.steps == STEPS
    seen = _param_errors(model, po)
    for i, (a, b) in enumerate(zip(losses, lo)):
        seen["loss%d" % (i + 1)] = abs(a - b) / b
    _assert_bar("step_series x3", seen)
    for k in PARAM_KEYS:
        assert max_abs(model.state_dict()[k].cpu(), c.p[k]) > 0          # the step moved it
    # the same three steps through TrainStep.step on the materialised windows and labels
    mat = _model(c)
    tm = TrainStep(mat)
    A, X, Lm = c.A.to(dev), c.X.to(dev), t.L.to(dev)
    lm = [float(tm.step(A, X, Lm)[0]) for _ in range(STEPS)]
    both = {k: rel_to_max(q.detach().cpu(), mat.state_dict()[k].cpu()) for k, q in model.named_parameters()}
    for i, (a, b) in enumerate(zip(losses, lm)):
        both["loss%d" % (i + 1)] = abs(a - b) / b
    _assert_bar("step_series vs step", both, 2 * TOL)


def test_forward_backward_series_leaves_the_gradients_in_the_bucket_and_takes_no_step():
    from windgnn_amd.trainer import TrainStep
    c, t = _case("ragged_wg"), _train("ragged_wg")
    dev = _dev()
    model = _model(c)
    tr = TrainStep(model)
    before = tr.flat_p.clone()
    loss, Y = tr.forward_backward_series(c.A.to(dev), c.Xs.to(dev), t.Ls.to(dev), c.T, c.stride, n_windows=c.n)
    grads = {k: q.grad.detach().cpu() for k, q in model.named_parameters()}
    _assert_bar("forward_backward_series", _errors(c, t, Y.cpu(), loss.cpu(), grads))
    assert tr.steps == 0 and torch.equal(tr.flat_p, before)


def test_max_grad_norm_measures_the_oracles_norm_and_clips():
    from windgnn_amd.trainer import TrainStep
    c, t = _case("cover_1_2"), _train("cover_1_2")
    _, g1, _ = _trajectory("cover_1_2")
    norm_o = float(torch.sqrt(sum((g.double() ** 2).sum() for g in g1.values())))
    threshold = 0.5 * norm_o                                         # half the oracle's norm: the clip is active
    tr = TrainStep(_model(c), max_grad_norm=threshold)
    _series_steps(c, t, tr, steps=1)
    norm, coef = float(tr.grad_norm), float(tr.clip_coef)
    print("\ngrad_norm %.6e (oracle %.6e)  clip_coef %.6f" % (norm, norm_o, coef))
    assert abs(norm - norm_o) <= TOL * norm_o
    assert coef < 1 and abs(coef - threshold / (norm_o + 1e-6)) <= TOL
    for k, q in zip(PARAM_KEYS, tr.g_views):                         # the bucket keeps the unclipped gradient
        assert rel_to_max(q.cpu(), g1[k]) <= TOL, k


def test_keep_best_follows_the_losses():
    from windgnn_amd.trainer import TrainStep
    c, t = _case("cover_1_2"), _train("cover_1_2")
    lo, _, _ = _trajectory("cover_1_2")
    tr = TrainStep(_model(c), keep_best=True)
    best, best_step = float("inf"), -1
    for i in range(STEPS):
        loss = _series_steps(c, t, tr, steps=1)[0]
        if loss < best:
            best, best_step = loss, i + 1
        assert int(tr.best_step) == best_step and float(tr.best_loss) == best and int(tr.improved) == int(best_step == i + 1)
    assert abs(best - min(lo)) <= TOL * min(lo) and best_step == 1 + lo.index(min(lo))
    assert tr.best_state_dict() is not None


def test_one_rank_process_group_runs_the_collective_schedule(tmp_path):
    """An explicitly passed one-rank group: shard_weight(n, n_global = n), the backward, ONE all-reduce of the bucket, the tail."""
    import torch.distributed as dist
    from windgnn_amd.trainer import TrainStep
    c, t = _case("cover_1_2"), _train("cover_1_2")
    lo, _, po = _trajectory("cover_1_2")
    assert not dist.is_initialized()
    dist.init_process_group("gloo", init_method="file://" + str(tmp_path / "store"), rank=0, world_size=1)
    try:
        model = _model(c)
        tr = TrainStep(model, process_group=dist.group.WORLD)
        assert tr.collective
        losses = _series_steps(c, t, tr, n_global=c.n)
        torch.cuda.synchronize()
        tr.close()
    finally:
        dist.destroy_process_group()
    seen = _param_errors(model, po)
    for i, (a, b) in enumerate(zip(losses, lo)):
        seen["loss%d" % (i + 1)] = abs(a - b) / b
    _assert_bar("step_series, one-rank group", seen)


def test_checkpoint_round_trip_continues_bit_identically():
    from windgnn_amd.trainer import TrainStep
    c, t = _case("cover_1_2"), _train("cover_1_2")
    whole = TrainStep(_model(c))
    l_whole = _series_steps(c, t, whole)
    first_model = _model(c)
    first = TrainStep(first_model)
    l_first = _series_steps(c, t, first, steps=1)
    ckpt = {"model": {k: v.clone() for k, v in first_model.state_dict().items()}, "step": first.state_dict()}
    from windgnn_amd import GCN_GRU
    resumed_model = GCN_GRU(13, 13, 13, c.S * 13, c.H, math="f32").to(_dev())
    resumed_model.load_state_dict(ckpt["model"])
    resumed = TrainStep(resumed_model)
    resumed.load_state_dict(ckpt["step"])
    assert resumed.steps == 1
    l_rest = _series_steps(c, t, resumed, steps=STEPS - 1)
    assert l_first + l_rest == l_whole
    assert torch.equal(resumed.flat_p, whole.flat_p)
    assert torch.equal(resumed.exp_avg, whole.exp_avg) and torch.equal(resumed.exp_avg_sq, whole.exp_avg_sq)


# ---- footprint: both entry points inside guarded arenas -------------------------------------------------------------------
def _arena_run(c, t, fill, dirty=None, gate=None):
    """wgnn_series_fwd_loss and wgnn_series_bwd_mse (on a re-poisoned workspace) on buffers of exactly their ABI lengths.
    Returns (outputs on the CPU, the final stash / workspace / loss_buf bytes).  gate: as in test_gpu_series._arena_run."""
    from windgnn_amd import _lib as L
    lib = L.load()
    sd = L.SeriesDims(c.rows, c.T, c.stride, c.n, c.S, F, c.H, 0, 0, 0, 0)
    ws_bytes, st_bytes = lib.wgnn_series_workspace_bytes(C.byref(sd)), lib.wgnn_series_stash_bytes(C.byref(sd))
    lb_bytes = lib.wgnn_series_loss_bytes(C.byref(sd))
    assert ws_bytes > STATUS and st_bytes > 0 and lb_bytes > 0
    a = Arena(_dev(), fill)
    dirty = dirty or {}

    def add(name, t=None, shape=None, **kw):
        n = (t.numel() if t is not None else int(np.prod(shape))) * 4
        return a.buf(name, n, data=t, **kw)

    add("A", c.A)
    add("Xs", c.Xs)
    Ls = t.Ls[:t.need].contiguous()                     # exactly the rows the windows cover: a read past them hits the guard
    add("Ls", Ls)
    for k in PARAM_KEYS:
        add("p." + k, c.p[k])
        add("g." + k, shape=c.p[k].shape)
    add("Y", shape=(c.n, c.T, c.H))
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
    outs = ["Y", "loss"] + ["g." + k for k in PARAM_KEYS]
    st = gate.handle if gate is not None else None
    if gate is not None:
        gate.begin(a)

    def after(what):
        if gate is not None:
            return
        torch.cuda.synchronize()
        assert a.check() == {}, (what, fill, a.check())
        assert int(a["ws"].view(torch.int32)[0]) == 0, (what, "status word")

    assert lib.wgnn_series_fwd_loss(C.byref(sd), P("A"), P("Xs"), C.byref(ps), P("Ls"), t.need, P("Y"), P("stash"),
                                    P("loss_buf"), P("ws"), ws_bytes, st) == 0
    after("wgnn_series_fwd_loss")
    if gate is not None:
        gate.repoison(a["ws"], STATUS)
    elif "ws" not in dirty:
        a["ws"].poison()                                   # the workspace carries nothing from the forward to the backward
    assert lib.wgnn_series_bwd_mse(C.byref(sd), P("A"), P("Xs"), C.byref(ps), P("Y"), P("Ls"), t.need, 1.0, P("stash"),
                                   P("loss_buf"), P("loss"), C.byref(gs), P("ws"), ws_bytes, st) == 0
    after("wgnn_series_bwd_mse")
    if gate is not None:
        gate.close(a)
    if fill != "zero" and not dirty:
        for name in outs:
            assert a[name].unwritten(4) == 0, (name, fill, a[name].unwritten(4))
    for name in ("A", "Xs", "Ls") + tuple("p." + k for k in PARAM_KEYS):      # inputs are read only
        assert a[name].unwritten(1) == a[name].nbytes, name
    return ({name: a[name].host() for name in outs},
            {"stash": a["stash"].host(), "ws": a["ws"].host(), "loss_buf": a["loss_buf"].host()})


def test_footprint_guards_fills_and_dirty_scratch():
    c, t = _case("cover_1_2"), _train("cover_1_2")
    assert FILLS[0] == "zero"
    base, _ = _arena_run(c, t, FILLS[0])
    Y = base["Y"].view(torch.float32).reshape(c.n, c.T, c.H)
    grads = {k: base["g." + k].view(torch.float32).reshape(t.go[k].shape) for k in PARAM_KEYS}
    _assert_bar("arena", _errors(c, t, Y, base["loss"].view(torch.float32)[0], grads))
    for fill in FILLS[1:]:
        out, _ = _arena_run(c, t, fill)
        for name, v in out.items():
            assert torch.equal(v, base[name]), (name, fill)
    # scratch another shape's calls left behind (its stash, workspace and loss_buf bytes, tiled to this case's sizes)
    _, left = _arena_run(_case("ragged_wg"), _train("ragged_wg"), "nan")
    for fill in ("finite", "nan"):
        out, _ = _arena_run(c, t, fill, dirty=left)
        for name, v in out.items():
            assert torch.equal(v, base[name]), (name, fill, "dirty")
