"""TrainStep(trainable=) / set_trainable and transfer.adopt_convs on the host (no GPU, no shared object): every raw binding the
trainer calls is replaced by a recorder (restated from tests/test_trainstep_schedule_host.py), and a step with a frozen group must
enqueue exactly the sequence written here -- BPTT and the ONE part of the backward whose products are the trained group's
gradients, the reduce-only wgnn_finish of that part, (the one all-reduce,) the optimiser's launch of that group alone, with the
group's own Adam step number.  "all" must record what a TrainStep built without the keyword records."""
import ast
import copy
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import windgnn_amd
from conftest import PARAM_KEYS, load_fixture
from windgnn_amd import _lib, trainer
from windgnn_amd.distributed import HEADER, LOSS_SLOT, grad_block_plan
from windgnn_amd.trainer import TrainStep
from windgnn_amd.transfer import adopt_convs

D, G, C = _lib.BWD_DEFER, _lib.FINISH_ADAM_GRU, _lib.FINISH_ADAM_CONV
W = 0.5                         # the stand-in's shard weight: a gradient weight dropped on the way would show as 1.0
S, T, B, H = 7, 5, 4, 21
PART = {"gru": 4, "conv": 2}    # the part of the backward a group's gradients come from, = its reduce bit of wgnn_finish
ADAM = {"gru": G, "conv": C}
SKIPPED = {"gru": 2, "conv": 4}


class Recorder:
    def __init__(self):
        self.events = []

    def __call__(self, *event):
        self.events.append(event)


class Work:
    def __init__(self, rec, tag):
        self.rec, self.tag = rec, tag

    def wait(self):
        self.rec("wait", self.tag)


class Exchange:
    """BucketExchange's interface towards TrainStep, recording."""
    direct = None

    def __init__(self, rec, plan=None):
        self.rec, self.plan = rec, plan

    def shard_weight(self, n_local, n_global=None):
        self.rec("shard_weight", n_local)
        return W if n_local else 0.0

    def all_reduce_all(self, weight):
        self.rec("all_reduce_all", weight)

    def start_gru(self):
        self.rec("start_gru")
        return Work(self.rec, "gru")

    def start_conv(self, weight):
        self.rec("start_conv", weight)
        return Work(self.rec, "conv")

    def start_block(self, block):
        i = self.plan.blocks.index(block)
        self.rec("start_block", i)
        return Work(self.rec, i)

    def start_tail(self, plan, weight):
        self.rec("start_tail", weight)
        return Work(self.rec, "tail")


def _bindings(rec, H):
    """Recording replacements of the names trainer.py takes from functional.py / series.py."""
    def dims(X, math, B=None):
        return _lib.Dims(X.shape[0] if B is None else B, X.shape[1], X.shape[2], 13, H, math, _lib.ADJ_DENSE, 0, _lib.IO_F32)

    def _forward_setup(A, X, params, math, labels=None, h0=None, h_n=None, B=None):
        rec("setup")
        return A, dims(X, math, B), None, 0

    def prepared_weights(d, params, device):
        rec("images")
        return torch.zeros(1)

    def gcn_gru_forward_raw(A, X, params, math=0, want_stash=True, labels=None, prepared=None):
        assert want_stash and prepared is not None
        rec("forward")
        return torch.zeros(X.shape[0], X.shape[1], H), None, dims(X, math)

    def gcn_gru_state_forward_raw(A, X, params, math=0, h0=None, h_n=None, prepared=None):
        assert h_n is not None and prepared is not None
        rec("state_forward", h0 is not None)
        return torch.zeros(X.shape[0], X.shape[1], H), h_n, None, dims(X, math)

    def gcn_gru_backward_mse_raw(d, A, X, params, Y, L, stash, grads, loss, grad_scale=1.0, part=7, prepared=None):
        assert prepared is not None
        rec("bwd_mse", part, grad_scale)

    def gcn_gru_backward_raw(d, A, X, params, Y, dY, stash, grads, part=7, stream=None, prepared=None):
        assert prepared is not None
        rec("bwd", part)

    def gcn_gru_state_backward_raw(d, A, X, params, Y, dY, dh_n, stash, grads, dh0=None, part=7, stream=None, prepared=None):
        assert prepared is not None and dh_n is None and dh0 is None
        rec("bwd_state", part)

    def mse_loss_grad(Y, L, grad_scale=1.0, want_grad=True, loss=None):
        assert loss is not None
        rec("mse_loss_grad", grad_scale)
        return loss, torch.zeros_like(Y)

    def loss_spec_grad(Y, L, kind, delta, t0, missing, grad_scale=1.0, loss_out=None, who=None):
        assert loss_out is not None
        rec("loss_spec_grad", kind, grad_scale)
        return loss_out, torch.zeros_like(Y), torch.tensor(Y.numel())

    def finish_step(d, params, grads, which, adam=None, prepared=None, device=None):
        assert (adam is None) == (prepared is None)
        rec("finish", which, adam and adam["step"])

    def finish_norm(d, grads, which, max_norm, clip, device=None):
        rec("finish_norm", which, max_norm)

    def finish_clipped(d, params, grads, adam, clip, prepared=None, device=None):
        rec("finish_clipped", adam["step"])

    def bwd_rows(d, Y, stash, grads, which, row0, rows, device=None):
        rec("bwd_rows", which, row0, rows)

    def finish_rows(d, params, grads, which, row0, rows, adam, prepared=None, device=None):
        rec("finish_rows", which, row0, rows, adam["step"])

    def series_forward_loss_raw(A, series, Ls, seq_len, stride, params, math=0, n_windows=None, prepared=None):
        assert prepared is not None
        rec("series_forward_loss", n_windows)
        return torch.zeros(n_windows, seq_len, H), None, None, None

    def series_backward_mse_raw(sd, A, series, params, Y, Ls, stash, loss_buf, grads, loss, grad_scale=1.0, prepared=None):
        assert prepared is not None
        rec("series_bwd_mse", grad_scale)
        for g in grads:             # wgnn_series_bwd_mse has no parts: it writes all eight gradients
            g.fill_(1.0)

    return dict(_forward_setup=_forward_setup, prepared_weights=prepared_weights, gcn_gru_forward_raw=gcn_gru_forward_raw,
                gcn_gru_state_forward_raw=gcn_gru_state_forward_raw, gcn_gru_backward_mse_raw=gcn_gru_backward_mse_raw,
                gcn_gru_backward_raw=gcn_gru_backward_raw, gcn_gru_state_backward_raw=gcn_gru_state_backward_raw,
                mse_loss_grad=mse_loss_grad, loss_spec_grad=loss_spec_grad, finish_step=finish_step,
                finish_norm=finish_norm, finish_clipped=finish_clipped, bwd_rows=bwd_rows, finish_rows=finish_rows,
                series_forward_loss_raw=series_forward_loss_raw, series_backward_mse_raw=series_backward_mse_raw,
                _require_gpu=lambda *t, **kw: rec("require_gpu"),
                refresh_prepared=lambda d, params, prepared: rec("refresh_images"),
                keep_best_launch=lambda args, step: rec("keep_best", step),
                clip_bytes=lambda d: 64, clip_buffer=lambda d, device: torch.zeros(16),
                check_range_status=lambda device=None: rec("check"))


def _make(patch, exchange=None, H=H, steps=41, **kw):
    """A CPU-constructed TrainStep on recorders; patch(name, fn) replaces a name of trainer.py.  exchange: None, "bucket",
    "overlap" or "blocked"."""
    rec = Recorder()
    for name, fn in _bindings(rec, H).items():
        assert hasattr(trainer, name), name
        patch(name, fn)
    tr = TrainStep(windgnn_amd.GCN_GRU(13, 13, 13, S * 13, H), check_every=0, **kw)
    if exchange is not None:      # a process group cannot be had here: the schedule is chosen by these four attributes
        tr.collective = True
        tr.overlap_collectives = exchange == "overlap"
        tr.plan = grad_block_plan(S, H, 2, 128) if exchange == "blocked" else None
        tr.exchange = Exchange(rec, tr.plan)
    tr.steps = steps
    return tr, rec


def _patch(monkeypatch):
    return lambda name, fn: monkeypatch.setattr(trainer, name, fn)


def _run(tr, kind="step", n=B):
    A = torch.rand(S, S)
    X, L = torch.rand(n, T, S, 13), torch.rand(n, T, tr.p_views[5].shape[1])
    if kind == "step":
        return tr.step(A, X, L)
    if kind == "l1":
        return tr.step(A, X, L, loss="l1")
    if kind == "forward_backward":
        return tr.forward_backward(A, X, L)
    if kind == "forward_backward_l1":
        return tr.forward_backward(A, X, L, loss="l1")
    if kind == "accumulate":                # two calls, then the one optimiser step
        tr.accumulate(A, X[:1], L[:1])
        tr.accumulate(A, X[1:], L[1:])
        return tr.apply()
    if kind == "accumulate_series":
        tr.accumulate_series(A, torch.rand(14, S, 13), torch.rand(14, tr.p_views[5].shape[1]), T, 3, n_windows=n)
        return tr.apply()
    assert kind == "series"
    return tr.step_series(A, torch.rand(14, S, 13), torch.rand(14, tr.p_views[5].shape[1]), T, 3, n_windows=n)


START = [("setup",), ("images",), ("forward",)]
STATE_START = [("setup",), ("images",), ("state_forward", False)]


def _want(kind, group):
    """The events of one step of `kind` from steps = 41 with `group` trained."""
    p, a = PART[group], ADAM[group]
    tail = [("finish", p, None), ("finish", a, 42)]
    return {
        "plain": (dict(), "step", B, START + [("bwd_mse", 1 | 8 | D, 1.0), ("bwd_mse", p | D, 1.0)] + tail),
        "state": (dict(carry_state=True), "step", B,
                  STATE_START + [("mse_loss_grad", 1.0), ("bwd_state", 1 | D), ("bwd_state", p | D)] + tail),
        "l1": (dict(), "l1", B, START + [("loss_spec_grad", "l1", 1.0), ("bwd", 1 | D), ("bwd", p | D)] + tail),
        "state-l1": (dict(carry_state=True), "l1", B,
                     STATE_START + [("loss_spec_grad", "l1", 1.0), ("bwd_state", 1 | D), ("bwd_state", p | D)] + tail),
        "bucket": (dict(exchange="bucket"), "step", B,
                   [("shard_weight", B)] + START + [("bwd_mse", 1 | 8 | D, W), ("bwd_mse", p | D, W), ("finish", p, None),
                                                    ("all_reduce_all", W), ("finish", a, 42)]),
        "state-bucket": (dict(exchange="bucket", carry_state=True), "step", B,
                         [("shard_weight", B)] + STATE_START +
                         [("mse_loss_grad", W), ("bwd_state", 1 | D), ("bwd_state", p | D), ("finish", p, None),
                          ("all_reduce_all", W), ("finish", a, 42)]),
        "empty-bucket": (dict(exchange="bucket"), "step", 0,
                         [("setup",), ("images",), ("shard_weight", 0), ("all_reduce_all", 0.0), ("finish", a, 42)]),
        "series": (dict(), "series", B,
                   [("require_gpu",), ("images",), ("series_forward_loss", B), ("series_bwd_mse", 1.0), ("finish", a, 42)]),
        "series-bucket": (dict(exchange="bucket"), "series", B,
                          [("shard_weight", B), ("require_gpu",), ("images",), ("series_forward_loss", B), ("series_bwd_mse", W),
                           ("all_reduce_all", W), ("finish", a, 42)]),
        "series-empty-bucket": (dict(exchange="bucket"), "series", 0,
                                [("setup",), ("images",), ("shard_weight", 0), ("all_reduce_all", 0.0), ("finish", a, 42)]),
    }[kind]


KINDS = ["plain", "state", "l1", "state-l1", "bucket", "state-bucket", "empty-bucket", "series", "series-bucket",
         "series-empty-bucket"]


def _masks(events):
    """The part masks of every backward call among the events."""
    return [e[1] for e in events if e[0] in ("bwd_mse", "bwd", "bwd_state")]


@pytest.mark.parametrize("group", ["gru", "conv"])
@pytest.mark.parametrize("kind", KINDS)
def test_a_step_with_a_frozen_group_enqueues_exactly_this_sequence(monkeypatch, kind, group):
    kw, call, n, want = _want(kind, group)
    tr, rec = _make(_patch(monkeypatch), trainable=group, **kw)
    tr._best_call = ("marshalled once",)
    _run(tr, call, n)
    assert rec.events == want + [("keep_best", 42)]          # `steps` is what keep_best records, after the increment
    assert tr.steps == 42
    assert all(not m & SKIPPED[group] for m in _masks(rec.events))
    frozen, trained = (tr.g_views[:4], tr.g_views[4:]) if group == "gru" else (tr.g_views[4:], tr.g_views[:4])
    for g in frozen:                                          # +0, also where series mode's whole backward wrote there
        assert torch.equal(g, torch.zeros_like(g)) and not torch.signbit(g).any()
    if call == "series" and n:
        assert all(bool((g == 1.0).all()) for g in trained)


@pytest.mark.parametrize("group", ["gru", "conv"])
@pytest.mark.parametrize("call", ["forward_backward", "forward_backward_l1"])
def test_forward_backward_runs_bptt_and_the_trained_groups_part_in_one_call(monkeypatch, call, group):
    tr, rec = _make(_patch(monkeypatch), trainable=group)
    _run(tr, call)
    p = PART[group]
    want = [("bwd_mse", 1 | p | 8, 1.0)] if call == "forward_backward" else [("loss_spec_grad", "l1", 1.0), ("bwd", 1 | p)]
    assert rec.events == START + want and tr.steps == 41


ALL_KINDS = [(dict(), "step", B), (dict(max_grad_norm=2.0), "step", B), (dict(carry_state=True), "step", B),
             (dict(), "l1", B), (dict(), "forward_backward", B), (dict(), "series", B), (dict(max_grad_norm=2.0), "series", B),
             (dict(exchange="bucket"), "step", B), (dict(exchange="bucket", max_grad_norm=2.0), "step", B),
             (dict(exchange="overlap"), "step", B), (dict(exchange="bucket", carry_state=True), "step", B),
             (dict(exchange="overlap", carry_state=True), "step", B), (dict(exchange="blocked", H=200), "step", B),
             (dict(exchange="bucket"), "step", 0), (dict(exchange="overlap"), "step", 0),
             (dict(exchange="blocked", H=200), "step", 0), (dict(exchange="bucket"), "series", B),
             (dict(exchange="bucket"), "series", 0),
             (dict(), "accumulate", B), (dict(exchange="bucket"), "accumulate", B), (dict(max_grad_norm=2.0), "accumulate", B),
             (dict(), "accumulate_series", B), (dict(exchange="bucket"), "accumulate_series", B)]


@pytest.mark.parametrize("row", range(len(ALL_KINDS)))
def test_all_records_what_a_trainstep_without_the_keyword_records(monkeypatch, row):
    kw, call, n = ALL_KINDS[row]
    was, rec_was = _make(_patch(monkeypatch), **kw)
    _run(was, call, n)
    tr, rec = _make(_patch(monkeypatch), trainable="all", **kw)
    _run(tr, call, n)
    _run(tr, call, n)                                         # (and a second step: the counts stay equal)
    k = len(rec_was.events)
    assert k > 0 and rec.events[:k] == rec_was.events
    if call != "forward_backward":
        assert [e for e in rec.events[k:] if e[0].startswith("finish")] == \
               [e[:-1] + (43,) if e[-1] == 42 else e for e in rec_was.events if e[0].startswith("finish")]
        assert tr.steps == 43 and tr._sat_out == {"gru": 0, "conv": 0}
    tr.set_trainable("all")                                   # a no-op that touches nothing
    assert len(rec.events) > k and tr.trainable == "all"


def test_the_frozen_schedule_without_deferral_lets_the_part_reduce_its_own_sums(monkeypatch):
    """TrainStep.FROZEN_DEFER = False, the alternative include/windgnn.h allows: no WGNN_BWD_DEFER, no reduce-only launch."""
    monkeypatch.setattr(TrainStep, "FROZEN_DEFER", False)
    tr, rec = _make(_patch(monkeypatch), trainable="gru")
    _run(tr)
    assert rec.events == START + [("bwd_mse", 1 | 8, 1.0), ("bwd_mse", 4, 1.0), ("finish", G, 42)]
    tr, rec = _make(_patch(monkeypatch), trainable="conv", exchange="bucket")
    _run(tr)
    assert rec.events == [("shard_weight", B)] + START + [("bwd_mse", 1 | 8, W), ("bwd_mse", 2, W), ("all_reduce_all", W),
                                                          ("finish", C, 42)]
    tr, rec = _make(_patch(monkeypatch))                      # "all" defers whatever the switch says
    _run(tr)
    assert rec.events == START + [("bwd_mse", 1 | 8 | D, 1.0), ("bwd_mse", 2 | D, 1.0), ("bwd_mse", 4 | D, 1.0), ("finish", 6, 42)]


# ---- refusals -------------------------------------------------------------------------------------------------------------------

def test_an_unknown_group_is_a_value_error_naming_the_three(monkeypatch):
    for make in (lambda: _make(_patch(monkeypatch), trainable="GRU"), lambda: _make(_patch(monkeypatch))[0].set_trainable("convs"),
                 lambda: _make(_patch(monkeypatch))[0].set_trainable(None)):
        with pytest.raises(ValueError, match=r"'all'.*'gru'.*'conv'"):
            make()


@pytest.mark.parametrize("kw, name", [(dict(max_grad_norm=1.0), "max_grad_norm"), (dict(overlap_collectives=True), "overlap_collectives")])
@pytest.mark.parametrize("group", ["gru", "conv"])
def test_the_constructor_refuses_these_options_with_a_frozen_group(monkeypatch, kw, name, group):
    with pytest.raises(RuntimeError, match=r"trainable='%s'.*%s" % (group, name)):
        _make(_patch(monkeypatch), trainable=group, **kw)
    tr, rec = _make(_patch(monkeypatch), **kw)                # and set_trainable on a TrainStep that has them
    with pytest.raises(RuntimeError, match=r"set_trainable\('%s'\).*%s" % (group, name)):
        tr.set_trainable(group)
    assert tr.trainable == "all" and rec.events == []
    tr.set_trainable("all")


def test_grad_blocks_is_refused_with_a_frozen_group(monkeypatch):
    tr, rec = _make(_patch(monkeypatch), exchange="blocked", H=200)
    with pytest.raises(RuntimeError, match=r"set_trainable\('gru'\).*grad_blocks"):
        tr.set_trainable("gru")
    assert tr.trainable == "all" and rec.events == []


@pytest.mark.parametrize("group", ["gru", "conv"])
def test_accumulation_is_refused_under_a_frozen_group_before_any_call(monkeypatch, group):
    tr, rec = _make(_patch(monkeypatch), trainable=group)
    A = torch.rand(S, S)
    with pytest.raises(RuntimeError, match=r"accumulate with trainable='%s'" % group):
        tr.accumulate(A, torch.rand(B, T, S, 13), torch.rand(B, T, H))
    with pytest.raises(RuntimeError, match=r"accumulate_series with trainable='%s'" % group):
        tr.accumulate_series(A, torch.rand(14, S, 13), torch.rand(14, H), T, 3)
    with pytest.raises(RuntimeError, match=r"apply\(\) with trainable='%s'" % group):
        tr.apply()
    assert rec.events == [] and tr.steps == 41 and tr.accumulated == 0


def test_set_trainable_is_refused_while_an_accumulation_or_a_validation_pass_is_open(monkeypatch):
    tr, rec = _make(_patch(monkeypatch))

    class Open:
        calls = 2
    tr._acc = Open()
    with pytest.raises(RuntimeError, match=r"set_trainable while an accumulation is open"):
        tr.set_trainable("gru")
    tr._acc = None
    tr._val_open = True
    with pytest.raises(RuntimeError, match=r"set_trainable\('conv'\) while a validation pass is open"):
        tr.set_trainable("conv")
    assert tr.trainable == "all" and rec.events == []
    tr._val_open = False
    tr.set_trainable("conv")
    assert tr.trainable == "conv"


def test_set_trainable_zeroes_the_newly_frozen_slots_once(monkeypatch):
    tr, _ = _make(_patch(monkeypatch))
    tr._gbuf.fill_(3.0)
    tr.set_trainable("gru")
    assert all(bool((g == 0).all()) for g in tr.g_views[:4]) and all(bool((g == 3).all()) for g in tr.g_views[4:])
    assert bool((tr._gbuf[:HEADER] == 3).all())               # the header (the loss word) is not a gradient slot
    tr._gbuf[HEADER:] = 5.0
    tr.set_trainable("gru")                                   # nothing newly frozen: nothing written
    assert bool((tr._gbuf[HEADER:] == 5).all())
    tr.set_trainable("conv")
    assert all(bool((g == 5).all()) for g in tr.g_views[:4]) and all(bool((g == 0).all()) for g in tr.g_views[4:])
    tr.set_trainable("all")
    assert all(bool((g == 0).all()) for g in tr.g_views[4:])


# ---- the groups' own Adam step numbers ------------------------------------------------------------------------------------------

def _finishes(rec):
    return [e[1:] for e in rec.events if e[0] == "finish"]


def test_two_steps_on_gru_then_two_on_all_step_each_group_at_its_own_count(monkeypatch):
    tr, rec = _make(_patch(monkeypatch), steps=0, trainable="gru")
    _run(tr), _run(tr)
    tr.set_trainable("all")
    _run(tr), _run(tr)
    assert _finishes(rec) == [(4, None), (G, 1), (4, None), (G, 2),
                              (6, None), (G, 3), (C, 1), (6, None), (G, 4), (C, 2)]   # reduce bits first, then one launch per group
    assert _masks(rec.events) == [1 | 8 | D, 4 | D] * 2 + [1 | 8 | D, 2 | D, 4 | D] * 2
    assert tr.steps == 4 and tr._group_count("gru") == 4 and tr._group_count("conv") == 2


def test_equal_counts_under_all_take_the_one_launch(monkeypatch):
    tr, rec = _make(_patch(monkeypatch), steps=0, trainable="gru")
    _run(tr)
    tr.set_trainable("conv")
    _run(tr)
    tr.set_trainable("all")                                   # both groups have taken one step: they step together again
    _run(tr)
    assert _finishes(rec) == [(4, None), (G, 1), (2, None), (C, 1), (6, 2)]
    assert tr.steps == 3 and tr._sat_out == {"gru": 1, "conv": 1}


def test_a_checkpoint_after_gru_then_conv_then_all_round_trips(monkeypatch):
    """One step on "gru", one on "conv", one on "all": `steps` is 3 while every tensor is at Adam step 2, under "all" with equal
    counts -- a state no TrainStep without the feature can be in, so the checkpoint says so ("trainable") and loads again."""
    for phases in (("gru", "conv", "all"), ("conv", "gru", "all"), ("gru", "conv")):
        tr, _ = _make(_patch(monkeypatch), steps=0, trainable=phases[0])
        for group in phases:
            tr.set_trainable(group)
            _run(tr)
        n = len(phases)
        sd = tr.state_dict()
        assert sd["trainable"] == phases[-1] and sd["steps"] == n
        assert [float(sd["optimizer"]["state"][i]["step"]) for i in range(8)] == [float(n - 1)] * 8
        tr2, rec2 = _make(_patch(monkeypatch), steps=0)
        tr2.load_state_dict(copy.deepcopy(sd))
        assert tr2.steps == n and tr2._sat_out == {"gru": 1, "conv": 1} == tr._sat_out and tr2.trainable == phases[-1]
        tr2.set_trainable("all")
        _run(tr2)
        assert _finishes(rec2) == [(6, n)] and tr2.steps == n + 1      # the groups step together again: the one launch
        again = tr2.state_dict()
        assert again["trainable"] == "all" and again["steps"] == n + 1
        assert float(again["optimizer"]["state"][0]["step"]) == float(again["optimizer"]["state"][7]["step"]) == float(n)
        with pytest.raises(ValueError, match=r"steps = %d but the Adam state is at step %d" % (n - 2, n - 1)):
            tr2.load_state_dict(dict(sd, steps=n - 2))
        plain = dict(sd)                    # the same dict without the key claims that no group ever sat out: steps must agree
        del plain["trainable"]
        if phases[-1] == "all":
            with pytest.raises(ValueError, match=r"steps = %d but the Adam state is at step %d" % (n, n - 1)):
                tr2.load_state_dict(plain)


@pytest.mark.parametrize("exchange", ["bucket", "overlap", "blocked"])
def test_unequal_counts_under_all_in_the_collective_schedules(monkeypatch, exchange):
    tr, rec = _make(_patch(monkeypatch), steps=5, exchange=exchange, H=200 if exchange == "blocked" else H)
    tr._sat_out = {"gru": 0, "conv": 2}                       # as a checkpoint of a "gru" phase leaves them
    _run(tr)
    fin = [e for e in rec.events if e[0] in ("finish", "finish_rows") and e[-1] is not None]
    assert [e[-1] for e in fin if e[0] == "finish_rows" or e[1] == G] == [6] * (len(fin) - 1)
    assert fin[-1] == ("finish", C, 4) and len(fin) >= 2
    if exchange == "bucket":
        assert rec.events[-4:] == [("finish", 6, None), ("all_reduce_all", W), ("finish", G, 6), ("finish", C, 4)]


# ---- checkpoints ----------------------------------------------------------------------------------------------------------------

def test_the_checkpoint_without_the_feature_in_use_has_the_keys_it_had(monkeypatch):
    tr, _ = _make(_patch(monkeypatch), steps=0)
    _run(tr)
    sd = tr.state_dict()
    assert set(sd) == {"optimizer", "steps", "best", "carry"}
    assert [float(sd["optimizer"]["state"][i]["step"]) for i in range(8)] == [1.0] * 8
    tr2, _ = _make(_patch(monkeypatch), trainable="all")
    tr2.load_state_dict(sd)
    assert tr2.trainable == "all" and tr2.steps == 1 and tr2._sat_out == {"gru": 0, "conv": 0}


def test_a_checkpoint_with_a_frozen_group_round_trips(monkeypatch):
    tr, _ = _make(_patch(monkeypatch), steps=0, trainable="gru")
    _run(tr), _run(tr)
    tr.set_trainable("all")
    _run(tr)
    tr.set_trainable("conv")
    tr.exp_avg.uniform_(), tr.exp_avg_sq.uniform_()
    sd = tr.state_dict()
    assert set(sd) == {"optimizer", "steps", "best", "carry", "trainable"} and sd["trainable"] == "conv" and sd["steps"] == 3
    assert [float(sd["optimizer"]["state"][i]["step"]) for i in range(8)] == [1.0] * 4 + [3.0] * 4
    tr2, rec2 = _make(_patch(monkeypatch))
    tr2._gbuf.fill_(7.0)
    tr2.load_state_dict(copy.deepcopy(sd))
    assert tr2.trainable == "conv" and tr2.steps == 3 and tr2._group_count("gru") == 3 and tr2._group_count("conv") == 1
    assert torch.equal(tr2.exp_avg, tr.exp_avg) and torch.equal(tr2.exp_avg_sq, tr.exp_avg_sq)
    assert all(bool((g == 0).all()) for g in tr2.g_views[4:])          # the newly frozen slots
    _run(tr2)
    assert _finishes(rec2) == [(2, None), (C, 2)]
    sd2 = tr2.state_dict()
    assert sd2["steps"] == 4 and [float(sd2["optimizer"]["state"][i]["step"]) for i in range(8)] == [2.0] * 4 + [3.0] * 4
    # torch.optim.Adam takes the optimiser part as its own
    opt = torch.optim.Adam(tr2.model.parameters())
    opt.load_state_dict(sd2["optimizer"])
    assert float(opt.state[tr2.params[0]]["step"]) == 2.0 and float(opt.state[tr2.params[7]]["step"]) == 3.0
    # "all" with unequal counts still says so; and a key of another spelling is refused
    tr2.set_trainable("all")
    assert tr2.state_dict()["trainable"] == "all"
    with pytest.raises(ValueError, match=r"'all'.*'gru'.*'conv'"):
        tr2.load_state_dict(dict(sd, trainable="GRU"))
    with pytest.raises(ValueError, match=r"steps = 2 but the Adam state is at step 3"):
        tr2.load_state_dict(dict(sd, steps=2))


def _adam_dict(model, phases):
    """torch.optim.Adam's own state dict after `phases`: a list of (group, steps) run with the other group's .grad None."""
    opt = torch.optim.Adam(model.parameters())
    params = list(model.parameters())
    saved = [p.grad for p in params]
    for group, k in phases:
        for i, p in enumerate(params):
            on = group == "all" or (group == "conv") == (i < 4)
            p.grad = torch.ones_like(p) if on else None
        for _ in range(k):
            opt.step()
    for p, g in zip(params, saved):
        p.grad = g
    return copy.deepcopy(opt.state_dict())


def test_a_bare_adam_dict_with_groupwise_differing_steps_loads(monkeypatch):
    tr, rec = _make(_patch(monkeypatch))
    sd = _adam_dict(tr.model, [("gru", 2), ("all", 1)])
    assert [float(sd["state"][i]["step"]) for i in range(8)] == [1.0] * 4 + [3.0] * 4
    tr.load_state_dict(sd)
    assert tr.trainable == "all" and tr.steps == 3 and tr._group_count("gru") == 3 and tr._group_count("conv") == 1
    for i in range(8):
        assert torch.equal(tr.m_views[i], sd["state"][i]["exp_avg"]) and torch.equal(tr.v_views[i], sd["state"][i]["exp_avg_sq"])
    _run(tr)
    assert _finishes(rec) == [(6, None), (G, 4), (C, 2)]
    # Adam makes a tensor's state at its first gradient: after a "gru" phase alone the dict holds the GRU tensors only
    tr, rec = _make(_patch(monkeypatch))
    tr.exp_avg.fill_(9.0)
    sd = _adam_dict(tr.model, [("gru", 2)])
    assert sorted(sd["state"]) == [4, 5, 6, 7]
    tr.load_state_dict(sd)
    assert tr.steps == 2 and tr._group_count("gru") == 2 and tr._group_count("conv") == 0
    assert all(bool((m == 0).all()) for m in tr.m_views[:4]) and torch.equal(tr.m_views[5], sd["state"][5]["exp_avg"])
    # clipping steps all eight tensors with one number
    tr, _ = _make(_patch(monkeypatch), max_grad_norm=1.0)
    with pytest.raises(RuntimeError, match=r"GRU tensors are at optimiser step 2 and the conv tensors at 0.*max_grad_norm"):
        tr.load_state_dict(sd)


def test_a_step_that_differs_inside_a_group_is_refused_with_the_parameters_name(monkeypatch):
    tr, _ = _make(_patch(monkeypatch))
    good = _adam_dict(tr.model, [("gru", 2), ("all", 1)])
    before = (tr.exp_avg.clone(), tr.steps)
    for i, key in ((1, r"conv1\.bias"), (5, r"gru\.weight_hh_l0")):
        sd = copy.deepcopy(good)
        sd["state"][i]["step"] = torch.tensor(7.0)
        with pytest.raises(ValueError, match=r"step.*disagree.*" + key):
            tr.load_state_dict(sd)
    sd = copy.deepcopy(good)
    del sd["state"][2]
    with pytest.raises(ValueError, match=r"Adam state for parameters"):
        tr.load_state_dict(sd)
    assert torch.equal(tr.exp_avg, before[0]) and tr.steps == before[1] and tr._sat_out == {"gru": 0, "conv": 0}


# ---- a real process group: gloo, two ranks, one of them without windows in the first step ---------------------------------------

def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    for group in ("gru", "conv"):
        rec = Recorder()
        for name, fn in _bindings(rec, H).items():
            setattr(trainer, name, fn)
        tr = TrainStep(windgnn_amd.GCN_GRU(13, 13, 13, S * 13, H), check_every=0, process_group=dist.group.WORLD, trainable=group)
        assert tr.collective and tr.world == 2
        reduce = tr.exchange.all_reduce_all

        def all_reduce_all(weight, reduce=reduce, rec=rec):
            rec("all_reduce_all", weight)
            reduce(weight)
        tr.exchange.all_reduce_all = all_reduce_all
        A = torch.rand(S, S)
        for n in ((3, 0)[rank], 2):                           # global batches of 3 (shards 3 | 0) and 4 (2 | 2)
            tr._gbuf[LOSS_SLOT] = 1.0          # the loss word of this rank's shard
            tr.step(A, torch.rand(n, T, S, 13), torch.rand(n, T, H), n_global=3 if n != 2 else 4)
        with open(os.path.join(out_dir, "%s_rank%d.txt" % (group, rank)), "w") as f:
            f.write(repr((rec.events, tr.steps, tr._sat_out, float(tr._loss), float(tr._gbuf[HEADER:].abs().sum()))))
    dist.barrier()
    dist.destroy_process_group()


def test_the_one_bucket_schedule_over_gloo_with_an_empty_shard(tmp_path):
    mp.spawn(_worker, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    for group in ("gru", "conv"):
        p, a = PART[group], ADAM[group]
        def step(w, n):
            return [("forward",), ("bwd_mse", 1 | 8 | D, w), ("bwd_mse", p | D, w), ("finish", p, None), ("all_reduce_all", w),
                    ("finish", a, n)]
        for rank in (0, 1):
            with open(os.path.join(str(tmp_path), "%s_rank%d.txt" % (group, rank))) as f:
                events, steps, sat_out, loss, gsum = ast.literal_eval(f.read())
            if rank == 0:
                want = [("setup",), ("images",)] + step(1.0, 1) + step(0.5, 2)
            else:                                             # the empty shard: a zero bucket, the same collective, the same tail
                want = [("setup",), ("images",), ("all_reduce_all", 0.0), ("finish", a, 1)] + step(0.5, 2)
            assert events == want, (group, rank)
            assert all(not m & SKIPPED[group] for m in _masks(events))
            assert steps == 2 and sat_out == {"gru": 0, "conv": 0, SKIPPED_NAME[group]: 2}
            assert loss == 1.0 and gsum == 0.0                # the weighted shard means, summed; the recorders wrote no gradient


SKIPPED_NAME = {"gru": "conv", "conv": "gru"}


# ---- transfer.adopt_convs -------------------------------------------------------------------------------------------------------

def _golden_model():
    fx = load_fixture("f2_s7_t12_b32_ckpt")
    src = windgnn_amd.GCN_GRU(13, 13, 13, 7 * 13, 21)
    src.load_state_dict({k: fx["params"][k].clone() for k in PARAM_KEYS})
    return src, fx["params"]


@pytest.mark.parametrize("how", ["model", "state_dict", "file"])
def test_adopt_convs_copies_the_four_conv_tensors_across_station_counts(tmp_path, how):
    src, params = _golden_model()                             # S = 7, H = 21
    torch.manual_seed(5)
    model = windgnn_amd.GCN_GRU(13, 13, 13, 34 * 13, 102)      # S = 34, H = 102
    gru_before = [p.detach().clone() for p in model.hot_path_parameters()[4:]]
    source = src
    if how == "state_dict":
        source = src.state_dict()
    elif how == "file":
        source = os.path.join(str(tmp_path), "trained.pt")
        torch.save(src.state_dict(), source)
    keys = adopt_convs(model, source)
    assert keys == ["conv1.weight", "conv1.bias", "conv2.weight", "conv2.bias"] == list(PARAM_KEYS[:4])
    got = model.state_dict()
    for k in keys:
        assert torch.equal(got[k], params[k]) and float(params[k].abs().sum()) > 0
    for p, was in zip(model.hot_path_parameters()[4:], gru_before):
        assert torch.equal(p.detach(), was)
    assert tuple(model.gru.weight_ih_l0.shape) == (306, 442)


def test_adopt_convs_refuses_other_widths_and_incomplete_sources():
    src, _ = _golden_model()
    wide = windgnn_amd.GCN_GRU(13, 20, 13, 7 * 13, 21)
    with pytest.raises(RuntimeError, match=r"adopt_convs: model has convolutions of 13 -> 20 -> 13"):
        adopt_convs(wide, src)
    model = windgnn_amd.GCN_GRU(13, 13, 13, 34 * 13, 102)
    before = copy.deepcopy(model.state_dict())
    with pytest.raises(RuntimeError, match=r"adopt_convs: source has convolutions of 13 -> 20 -> 13"):
        adopt_convs(model, wide)
    with pytest.raises(RuntimeError, match=r"conv1\.weight is \(13, 20\)"):
        adopt_convs(model, wide.state_dict())
    sd = src.state_dict()
    del sd["conv2.bias"]
    with pytest.raises(KeyError, match=r"conv2\.bias"):
        adopt_convs(model, sd)
    with pytest.raises(TypeError):
        adopt_convs(model, 3)
    assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())


def test_a_trainstep_made_earlier_sees_adopted_convs_through_the_version_counters(monkeypatch):
    """No tr.refresh(): the copy goes through the nn.Parameters, torch counts it, and the next step rebuilds the W_ih images."""
    src, params = _golden_model()
    tr, rec = _make(_patch(monkeypatch), trainable="gru")
    _run(tr), _run(tr)
    assert [e for e in rec.events if "images" in e[0]] == [("images",)]          # built once, then kept current by wgnn_finish
    adopt_convs(tr.model, src)
    for k, v in zip(PARAM_KEYS[:4], tr.p_views[:4]):          # the parameters are views of the flat bucket: it holds the copy
        assert torch.equal(v, params[k])
    assert torch.equal(tr.flat_p[:tr.n_conv], torch.cat([params[k].reshape(-1) for k in PARAM_KEYS[:4]]))
    _run(tr)
    assert [e for e in rec.events if "images" in e[0]] == [("images",), ("refresh_images",)]
    assert "adopt_convs" in windgnn_amd.__all__ and windgnn_amd.adopt_convs is adopt_convs


# ---- Ensemble -------------------------------------------------------------------------------------------------------------------

def test_ensemble_hands_trainable_out_per_member_and_each_reaches_set_trainable():
    from windgnn_amd import Ensemble, PerMember, ensemble

    class Stream:
        def wait_event(self, event):
            pass

    class Event:
        def record(self, stream=None):
            pass

    class Cuda:                                               # ensemble._cuda: the stream operations of the fan-out, as no-ops
        new_stream = staticmethod(lambda device: Stream())
        current_stream = staticmethod(lambda device: Stream())
        event = staticmethod(Event)
        set_stream = staticmethod(lambda stream: None)
        hand_back = staticmethod(lambda t, stream: None)
    was = ensemble._cuda
    ensemble._cuda = Cuda
    try:
        ens = Ensemble([windgnn_amd.GCN_GRU(13, 13, 13, S * 13, H) for _ in range(3)], trainable=PerMember(["all", "gru", "conv"]))
        assert [tr.trainable for tr in ens.members] == ["all", "gru", "conv"]
        ens.each(lambda k, tr: tr.set_trainable("gru"))
        assert [tr.trainable for tr in ens.members] == ["gru"] * 3
        with pytest.raises(ValueError, match=r"'all'.*'gru'.*'conv'"):
            Ensemble([windgnn_amd.GCN_GRU(13, 13, 13, S * 13, H)], trainable="none")
    finally:
        ensemble._cuda = was
