"""TrainStep's step schedules as call sequences (no GPU, no shared object): every raw binding the trainer calls is replaced
by a recorder and the exchange by a recording stand-in, and one step of every schedule -- one rank, one bucket, two collectives,
blocked; plain, carried-state, clipped, empty-shard and series steps -- must enqueue exactly the sequence written here, with each
call's part / which / row arguments, its gradient weight and Adam's step number.  This pins what the GPU tests cannot on one
GPU: the empty-shard step of the two-collective and blocked schedules, and the blocked schedule's ordering hazard (no
wgnn_finish_rows before part 2 of the backward)."""
import pytest
import torch

import windgnn_amd
from windgnn_amd import _lib, trainer
from windgnn_amd.distributed import grad_block_plan
from windgnn_amd.trainer import TrainStep

D, G, C = _lib.BWD_DEFER, _lib.FINISH_ADAM_GRU, _lib.FINISH_ADAM_CONV
IH, HH = _lib.ROWS_IH, _lib.ROWS_HH
W = 0.5                         # the stand-in's shard weight: a gradient weight dropped on the way would show as 1.0
S, T, B = 7, 5, 4


class Boom(Exception):
    pass


class Recorder:
    def __init__(self):
        self.events = []
        self.fail_at = None      # raise Boom instead of recording event number fail_at

    def __call__(self, *event):
        if self.fail_at == len(self.events):
            raise Boom(event)
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
        assert plan is self.plan
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
        assert want_stash and labels is not None and prepared is not None
        rec("forward")
        return torch.zeros(X.shape[0], X.shape[1], H), None, dims(X, math)

    def gcn_gru_state_forward_raw(A, X, params, math=0, h0=None, h_n=None, prepared=None):
        assert h_n is not None and prepared is not None
        rec("state_forward", h0 is not None)
        return torch.zeros(X.shape[0], X.shape[1], H), h_n, None, dims(X, math)

    def gcn_gru_backward_mse_raw(d, A, X, params, Y, L, stash, grads, loss, grad_scale=1.0, part=7, prepared=None):
        assert prepared is not None
        rec("bwd_mse", part, grad_scale)

    def gcn_gru_state_backward_raw(d, A, X, params, Y, dY, dh_n, stash, grads, dh0=None, part=7, stream=None, prepared=None):
        assert prepared is not None and dh_n is None and dh0 is None
        rec("bwd_state", part)

    def mse_loss_grad(Y, L, grad_scale=1.0, want_grad=True, loss=None):
        assert loss is not None
        rec("mse_loss_grad", grad_scale)
        return loss, torch.zeros_like(Y)

    def finish_step(d, params, grads, which, adam=None, prepared=None, device=None):
        assert (adam is None) == (prepared is None)
        rec("finish", which, adam and adam["step"])

    def finish_norm(d, grads, which, max_norm, clip, device=None):
        rec("finish_norm", which, max_norm)

    def finish_clipped(d, params, grads, adam, clip, prepared=None, device=None):
        assert prepared is not None
        rec("finish_clipped", adam["step"])

    def bwd_rows(d, Y, stash, grads, which, row0, rows, device=None):
        rec("bwd_rows", which, row0, rows)

    def finish_rows(d, params, grads, which, row0, rows, adam, prepared=None, device=None):
        assert prepared is not None
        rec("finish_rows", which, row0, rows, adam["step"])

    def series_forward_loss_raw(A, series, Ls, seq_len, stride, params, math=0, n_windows=None, prepared=None):
        assert prepared is not None
        rec("series_forward_loss", n_windows)
        return torch.zeros(n_windows, seq_len, H), None, None, None

    def series_backward_mse_raw(sd, A, series, params, Y, Ls, stash, loss_buf, grads, loss, grad_scale=1.0, prepared=None):
        assert prepared is not None
        rec("series_bwd_mse", grad_scale)

    return dict(_forward_setup=_forward_setup, prepared_weights=prepared_weights, gcn_gru_forward_raw=gcn_gru_forward_raw,
                gcn_gru_state_forward_raw=gcn_gru_state_forward_raw, gcn_gru_backward_mse_raw=gcn_gru_backward_mse_raw,
                gcn_gru_state_backward_raw=gcn_gru_state_backward_raw, mse_loss_grad=mse_loss_grad, finish_step=finish_step,
                finish_norm=finish_norm, finish_clipped=finish_clipped, bwd_rows=bwd_rows, finish_rows=finish_rows,
                series_forward_loss_raw=series_forward_loss_raw, series_backward_mse_raw=series_backward_mse_raw,
                _require_gpu=lambda *t, **kw: rec("require_gpu"),
                refresh_prepared=lambda d, params, prepared: rec("refresh_images"),
                keep_best_launch=lambda args, step: rec("keep_best", step),
                clip_bytes=lambda d: 64, clip_buffer=lambda d, device: torch.zeros(16),
                check_range_status=lambda device=None: rec("check"))


def _step(monkeypatch, exchange=None, empty=False, series=False, keep_best=False, H=21, math="f32", fail_at=None, **kw):
    """One step of a CPU-constructed TrainStep on recorders.  exchange: None, "bucket", "overlap" or "blocked".  Returns
    (the step, the recorder); fail_at: event number fail_at raises Boom, which the step must pass on."""
    rec = Recorder()
    for name, fn in _bindings(rec, H).items():
        assert hasattr(trainer, name), name
        monkeypatch.setattr(trainer, name, fn)
    tr = TrainStep(windgnn_amd.GCN_GRU(13, 13, 13, S * 13, H, math=math), check_every=1, **kw)
    if exchange is not None:      # a process group cannot be had here: the schedule is chosen by these four attributes
        tr.collective = True
        tr.overlap_collectives = exchange == "overlap"
        tr.plan = grad_block_plan(S, H, 2, 128) if exchange == "blocked" else None
        tr.exchange = Exchange(rec, tr.plan)
    if keep_best:
        tr._best_call = ("marshalled once",)
    tr.steps = 41
    rec.fail_at = fail_at
    A = torch.rand(S, S)
    n = 0 if empty else B
    if series:
        call = lambda: tr.step_series(A, torch.rand(14, S, 13), torch.rand(14, H), T, 3, n_windows=n)   # noqa: E731
    else:
        call = lambda: tr.step(A, torch.rand(n, T, S, 13), torch.rand(n, T, H))                          # noqa: E731
    if fail_at is None:
        loss, Y = call()
        assert loss is tr._loss and tuple(Y.shape) == (n, T, H)
    else:
        with pytest.raises(Boom):
            call()
    return tr, rec


START = [("setup",), ("images",), ("forward",)]
STATE_START = [("setup",), ("images",), ("state_forward", False)]
BLOCKS = [(IH, 0, 600), (HH, 0, 256), (HH, 256, 344)]        # grad_block_plan(7, 200, 2, 128): 91 vs 200 columns

# kind -> (arguments of _step, the events of one step from steps = 41)
ROWS = {
    "plain": (dict(), START + [("bwd_mse", 1 | 8 | D, 1.0), ("bwd_mse", 2 | D, 1.0), ("bwd_mse", 4 | D, 1.0), ("finish", 6, 42)]),
    "plain-clipped": (dict(max_grad_norm=2.0),
                      START + [("bwd_mse", 1 | 8 | D, 1.0), ("bwd_mse", 2 | D, 1.0), ("bwd_mse", 4 | D, 1.0),
                               ("finish_norm", 6, 2.0), ("finish_clipped", 42)]),
    "state": (dict(carry_state=True),
              STATE_START + [("mse_loss_grad", 1.0), ("bwd_state", 1 | D), ("bwd_state", 2 | D), ("bwd_state", 4 | D),
                             ("finish", 6, 42)]),
    "plain-bucket": (dict(exchange="bucket"),
                     [("shard_weight", B)] + START +
                     [("bwd_mse", 1 | 8 | D, W), ("bwd_mse", 2 | D, W), ("bwd_mse", 4 | D, W), ("finish", 6, None),
                      ("all_reduce_all", W), ("finish", 0, 42)]),
    "plain-bucket-clipped": (dict(exchange="bucket", max_grad_norm=2.0),
                             [("shard_weight", B)] + START +
                             [("bwd_mse", 1 | 8 | D, W), ("bwd_mse", 2 | D, W), ("bwd_mse", 4 | D, W), ("finish", 6, None),
                              ("all_reduce_all", W), ("finish_norm", 0, 2.0), ("finish_clipped", 42)]),
    "plain-overlap": (dict(exchange="overlap"),
                      [("shard_weight", B)] + START +
                      [("bwd_mse", 1 | 4 | 8 | D, W), ("finish", 4, None), ("start_gru",), ("bwd_mse", 2 | D, W),
                       ("finish", 2, None), ("start_conv", W), ("wait", "gru"), ("finish", G, 42), ("wait", "conv"),
                       ("finish", C, 42)]),
    "state-bucket": (dict(exchange="bucket", carry_state=True),
                     [("shard_weight", B)] + STATE_START +
                     [("mse_loss_grad", W), ("bwd_state", 1 | D), ("bwd_state", 2 | D), ("bwd_state", 4 | D),
                      ("finish", 6, None), ("all_reduce_all", W), ("finish", 0, 42)]),
    "state-overlap": (dict(exchange="overlap", carry_state=True),
                      [("shard_weight", B)] + STATE_START +
                      [("mse_loss_grad", W), ("bwd_state", 1 | 4 | D), ("finish", 4, None), ("start_gru",),
                       ("bwd_state", 2 | D), ("finish", 2, None), ("start_conv", W), ("wait", "gru"), ("finish", G, 42),
                       ("wait", "conv"), ("finish", C, 42)]),
    "plain-blocked": (dict(exchange="blocked", H=200),
                      [("shard_weight", B)] + START + [("bwd_mse", 1 | 8 | D, W)] +
                      [e for i, b in enumerate(BLOCKS) for e in (("bwd_rows",) + b, ("start_block", i))] +
                      [("bwd_mse", 2 | D, W), ("finish", 2, None), ("start_tail", W), ("wait", "tail")] +
                      [e for i, b in enumerate(BLOCKS) for e in (("wait", i), ("finish_rows",) + b + (42,))] +
                      [("finish", C, 42)]),
    "empty-bucket": (dict(exchange="bucket", empty=True),
                     [("setup",), ("images",), ("shard_weight", 0), ("all_reduce_all", 0.0), ("finish", 0, 42)]),
    "empty-bucket-clipped": (dict(exchange="bucket", empty=True, max_grad_norm=2.0),
                             [("setup",), ("images",), ("shard_weight", 0), ("all_reduce_all", 0.0), ("finish_norm", 0, 2.0),
                              ("finish_clipped", 42)]),
    "empty-overlap": (dict(exchange="overlap", empty=True),
                      [("setup",), ("images",), ("shard_weight", 0), ("start_gru",), ("start_conv", 0.0), ("wait", "gru"),
                       ("finish", G, 42), ("wait", "conv"), ("finish", C, 42)]),
    "empty-blocked": (dict(exchange="blocked", empty=True, H=200),
                      [("setup",), ("images",), ("shard_weight", 0)] + [("start_block", i) for i in range(3)] +
                      [("start_tail", 0.0), ("wait", "tail")] +
                      [e for i, b in enumerate(BLOCKS) for e in (("wait", i), ("finish_rows",) + b + (42,))] +
                      [("finish", C, 42)]),
    "series": (dict(series=True),
               [("require_gpu",), ("images",), ("series_forward_loss", B), ("series_bwd_mse", 1.0), ("finish", 0, 42)]),
    "series-clipped": (dict(series=True, max_grad_norm=2.0),
                       [("require_gpu",), ("images",), ("series_forward_loss", B), ("series_bwd_mse", 1.0),
                        ("finish_norm", 0, 2.0), ("finish_clipped", 42)]),
    "series-bucket": (dict(series=True, exchange="bucket"),
                      [("shard_weight", B), ("require_gpu",), ("images",), ("series_forward_loss", B), ("series_bwd_mse", W),
                       ("all_reduce_all", W), ("finish", 0, 42)]),
    "series-empty-bucket": (dict(series=True, exchange="bucket", empty=True),
                            [("setup",), ("images",), ("shard_weight", 0), ("all_reduce_all", 0.0), ("finish", 0, 42)]),
}


@pytest.mark.parametrize("kind", list(ROWS))
def test_one_step_enqueues_exactly_this_sequence(monkeypatch, kind):
    kw, want = ROWS[kind]
    tr, rec = _step(monkeypatch, **kw)
    assert rec.events == want
    assert tr.steps == 42
    if kw.get("carry_state"):
        assert (tr._hcur, tr._has_state) == (1, True)


@pytest.mark.parametrize("kind", list(ROWS))
def test_keep_best_follows_the_last_optimiser_launch(monkeypatch, kind):
    kw, want = ROWS[kind]
    tr, rec = _step(monkeypatch, keep_best=True, **kw)
    assert rec.events == want + [("keep_best", 42)]          # step = `steps` after the increment
    assert tr.steps == 42


@pytest.mark.parametrize("kind", ["plain-blocked", "empty-blocked"])
def test_no_block_steps_adam_before_part_two_of_the_backward(monkeypatch, kind):
    kw, _ = ROWS[kind]
    _, rec = _step(monkeypatch, **kw)
    names = [e[0] for e in rec.events]
    first = names.index("finish_rows")
    assert names.count("finish_rows") == 3
    if kind == "plain-blocked":
        assert rec.events.index(("bwd_mse", 2 | D, W)) < first      # wgnn_finish_rows rewrites the W_ih part 2 reads
    assert rec.events.index(("wait", "tail")) < first                # every block's Adam reads the biases of the tail
    for i in range(3):
        assert names[rec.events.index(("wait", i)) + 1] == "finish_rows"


@pytest.mark.parametrize("kind", list(ROWS))
def test_the_range_check_follows_a_nonempty_f16x3_step_only(monkeypatch, kind):
    kw, want = ROWS[kind]
    if kw.get("series"):
        return                                               # series mode refuses f16x3 before any launch
    _, rec = _step(monkeypatch, math="f16x3", keep_best=True, **kw)
    end = [("keep_best", 42)] + ([] if kw.get("empty") else [("check",)])
    assert rec.events == want + end
    _, rec = _step(monkeypatch, **kw)                        # exact fp32 without a direct communicator: nothing to check
    assert ("check",) not in rec.events


@pytest.mark.parametrize("kind", list(ROWS))
def test_a_step_that_raises_is_not_counted(monkeypatch, kind):
    kw, want = ROWS[kind]
    for fail_at in range(len(want)):
        tr, rec = _step(monkeypatch, fail_at=fail_at, **kw)
        assert rec.events == want[:fail_at], fail_at
        assert tr.steps == 41, fail_at
        assert (tr._hcur, tr._has_state) == (0, False), fail_at
