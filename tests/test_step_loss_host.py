"""Training on a loss spec on materialised windows, the part that needs no GPU and no shared object: functional.loss_spec_grad
(plain torch) against fp64 autograd of its formulas, the refusals of TrainStep.step / forward_backward by the argument's name
(each before any call), and the step's call sequences in every schedule, on the recorders of
tests/test_trainstep_schedule_host.py.

The bars of the arithmetic.  dY: three fp32 roundings per element (the residual, the coefficient, the product), <= 4 * 2^-24
relative: held to 1e-6 of max |dY_ref|.  The sign of an fp32 difference is exact, so L1's dY is sign * float32(grad_scale / m)
exactly.  The loss: a sum of N non-negative fp32 terms in any order, then one division: (N + 4) * 2^-24 relative."""
import math

import pytest
import torch

import series_lossfn_cases as lc
import step_loss_cases as sl
import test_trainstep_schedule_host as sched
import windgnn_amd
from windgnn_amd import _lib, trainer
from windgnn_amd.distributed import grad_block_plan
from windgnn_amd.trainer import TrainStep

D = _lib.BWD_DEFER
W = sched.W
S, T, B = sched.S, sched.T, sched.B
GS = 0.5


# ---- 1. functional.loss_spec_grad --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("io", list(sl.DTYPES))
@pytest.mark.parametrize("mask", sl.HOST_MASKS)
@pytest.mark.parametrize("t_from", [0, 2, sl.HOST_SHAPE[1] - 1])
@pytest.mark.parametrize("kind", sl.HOST_KINDS)
def test_loss_spec_grad_is_fp64_autograd_of_the_formulas(kind, t_from, mask, io):
    from windgnn_amd.functional import loss_spec_grad
    Y, L = sl.host_draw(io, mask)
    masked = mask != "none"
    slot = torch.full((4,), 7.0)
    loss, dY, count = loss_spec_grad(Y, L, kind, sl.DELTA, t_from, masked, grad_scale=GS, loss_out=slot[3])
    assert loss.data_ptr() == slot[3].data_ptr() and slot[:3].tolist() == [7.0] * 3        # the caller's word, and only it
    assert dY.dtype == torch.float32 and dY.is_contiguous() and tuple(dY.shape) == sl.HOST_SHAPE
    assert count.dtype == torch.int64 and count.dim() == 0 and loss.dim() == 0 and loss.dtype == torch.float32
    ref, dref, m = sl.autograd_spec(Y, L, kind, sl.DELTA, t_from, masked, GS)
    on = lc.counted(L.double(), t_from, masked)
    assert int(count) == m == int(on.sum())
    assert not torch.isnan(dY).any() and (dY[~on] == 0).all()            # exactly zero before loss_from and at a missing label
    if mask == "all":
        assert m == 0 and math.isnan(float(loss)) and (dY == 0).all()
        return
    assert m > 0 and (dY[on] != 0).any()
    err = float((dY.double() - dref).abs().max()) / float(dref.abs().max())
    assert err <= 1e-6, err
    assert abs(float(loss) - ref) <= (m + 4) * 2.0 ** -24 * abs(ref), (float(loss), ref)
    if kind == "l1":
        coef = torch.tensor(GS / m, dtype=torch.float64).float()
        sign = torch.where(on, torch.sign(Y.double() - torch.nan_to_num(L.double())), torch.zeros(sl.HOST_SHAPE, dtype=torch.float64))
        assert torch.equal(dY, sign.float() * coef)


@pytest.mark.parametrize("kind", sl.HOST_KINDS)
def test_a_nan_label_without_missing_labels_poisons_the_loss_and_one_before_loss_from_does_not(kind):
    from windgnn_amd.functional import loss_spec_grad
    Y, L = (t.clone() for t in sl.host_draw("fp32", "none"))
    L[1, 1, 3] = float("nan")
    loss, dY, count = loss_spec_grad(Y, L, kind, sl.DELTA, 0)
    assert math.isnan(float(loss)) and int(count) == Y.numel()
    loss, dY, count = loss_spec_grad(Y, L, kind, sl.DELTA, 2)            # sliced away: it reaches nothing
    ref, dref, m = sl.autograd_spec(Y, torch.nan_to_num(L), kind, sl.DELTA, 2, False)
    assert int(count) == m and abs(float(loss) - ref) <= (m + 4) * 2.0 ** -24 * ref and not torch.isnan(dY).any()
    # the defaults are nn.MSELoss and its gradient, without a loss_out
    Y, L = sl.host_draw("fp32", "none")
    loss, dY, count = loss_spec_grad(Y, L)
    assert abs(float(loss) - float(torch.nn.functional.mse_loss(Y.double(), L.double()))) <= 1e-6
    assert float((dY.double() - 2.0 * (Y.double() - L.double()) / Y.numel()).abs().max()) <= 1e-9 and int(count) == Y.numel()


def test_loss_spec_grad_refuses_by_the_arguments_name():
    from windgnn_amd.functional import loss_spec_grad
    Y, L = sl.host_draw("fp32", "none")
    for kw, text in ((dict(loss="mae"), "loss='mae'"), (dict(loss_from=5), "loss_from=5"), (dict(loss_from=1.5), "loss_from=1.5"),
                     (dict(loss="huber", huber_delta=0.0), "huber_delta=0.0")):
        with pytest.raises(ValueError, match="my caller: " + text):
            loss_spec_grad(Y, L, who="my caller", **kw)
    with pytest.raises(ValueError, match="one shape"):
        loss_spec_grad(Y, L[:, :4])
    with pytest.raises(ValueError, match="float32 or Y's dtype"):
        loss_spec_grad(Y, L.double())
    with pytest.raises(ValueError, match="loss_out"):
        loss_spec_grad(Y, L, loss_out=torch.zeros(1))


# ---- 2. the step on recorders ------------------------------------------------------------------------------------------------------
SPEC = dict(loss="huber", huber_delta=0.25, loss_from=2, missing_labels=False)
SPEC_EVENT = ("huber", 0.25, 2, False)


def _bindings(rec, H, tr_of):
    """The schedule suite's recorders, with the forward telling whether it got labels, and recorders of the two bindings a step
    on a loss spec adds."""
    b = sched._bindings(rec, H)
    dims = lambda X, math: _lib.Dims(X.shape[0], X.shape[1], X.shape[2], 13, H, math, _lib.ADJ_DENSE, 0, _lib.IO_F32)  # noqa: E731

    def gcn_gru_forward_raw(A, X, params, math=0, want_stash=True, labels=None, prepared=None):
        assert want_stash and prepared is not None
        rec("forward") if labels is not None else rec("forward", "no labels")
        return torch.zeros(X.shape[0], X.shape[1], H), None, dims(X, math)

    def loss_spec_grad(Y, L, loss="mse", huber_delta=1.0, loss_from=0, missing_labels=False, grad_scale=1.0, loss_out=None,
                       who=None):
        assert loss_out is tr_of()._loss and tuple(L.shape) == tuple(Y.shape) and who.startswith("windgnn_amd: TrainStep.")
        rec("loss_spec_grad", loss, huber_delta, loss_from, missing_labels, grad_scale)
        return loss_out, torch.zeros_like(Y), torch.tensor(Y[:, loss_from:].numel())

    def gcn_gru_backward_raw(d, A, X, params, Y, dY, stash, grads, part=7, stream=None, prepared=None):
        assert prepared is not None and stream is None and dY.dtype == torch.float32
        rec("bwd", part)

    b.update(gcn_gru_forward_raw=gcn_gru_forward_raw, loss_spec_grad=loss_spec_grad, gcn_gru_backward_raw=gcn_gru_backward_raw)
    return b


def _step(monkeypatch, spec, exchange=None, empty=False, keep_best=False, H=21, math="f32", fail_at=None, method="step",
          labels=None, series=False, **kw):
    """sched._step with the keywords `spec` on the call (None: a call without keywords)."""
    assert not series
    rec = sched.Recorder()
    box = []
    for name, fn in _bindings(rec, H, lambda: box[0]).items():
        assert hasattr(trainer, name), name
        monkeypatch.setattr(trainer, name, fn)
    tr = TrainStep(windgnn_amd.GCN_GRU(13, 13, 13, S * 13, H, math=math), check_every=1, **kw)
    box.append(tr)
    if exchange is not None:
        tr.collective = True
        tr.overlap_collectives = exchange == "overlap"
        tr.plan = grad_block_plan(S, H, 2, 128) if exchange == "blocked" else None
        tr.exchange = sched.Exchange(rec, tr.plan)
    if keep_best:
        tr._best_call = ("marshalled once",)
    tr.steps = 41
    rec.fail_at = fail_at
    n = 0 if empty else B
    L = torch.rand(n, T, H) if labels is None else labels
    call = lambda: getattr(tr, method)(torch.rand(S, S), torch.rand(n, T, S, 13), L, **(spec or {}))   # noqa: E731
    if fail_at is None:
        loss, Y = call()
        assert loss is tr._loss and tuple(Y.shape) == (n, T, H)
    else:
        with pytest.raises(sched.Boom):
            call()
    return tr, rec


def _with_spec(events):
    """The events of a step on SPEC from those of the default step: the forward without labels, one loss_spec_grad with the
    shard weight in place of the loss the MSE entry points form, the same parts through gcn_gru_backward_raw, the same tail."""
    out = []
    for e in events:
        if e == ("forward",):
            out.append(("forward", "no labels"))
        elif e[0] == "mse_loss_grad":
            out.append(("loss_spec_grad",) + SPEC_EVENT + (e[1],))
        elif e[0] == "bwd_mse":
            if e[1] & 8:                                         # part 1 of the MSE entry point also finalises the loss
                out.append(("loss_spec_grad",) + SPEC_EVENT + (e[2],))
            out.append(("bwd", e[1] & ~8))
        else:
            out.append(e)
    return out


KINDS = [k for k, (kw, _) in sched.ROWS.items() if not kw.get("series")]


def test_guard_the_imported_rows_keep_their_names():
    """A guard on the table imported from tests/test_trainstep_schedule_host.py, not a test of the new code (it passes without
    it): the sequences below are derived from these rows, so a row renamed or dropped there must show here."""
    assert set(KINDS) == {"plain", "plain-clipped", "state", "plain-bucket", "plain-bucket-clipped", "plain-overlap",
                          "state-bucket", "state-overlap", "plain-blocked", "empty-bucket", "empty-bucket-clipped",
                          "empty-overlap", "empty-blocked"}


@pytest.mark.parametrize("kind", KINDS)
def test_the_defaults_record_exactly_the_events_of_a_step_without_keywords(monkeypatch, kind):
    kw, want = sched.ROWS[kind]
    _, rec = _step(monkeypatch, None, **kw)
    assert rec.events == want
    tr, rec = _step(monkeypatch, dict(loss="mse", huber_delta=1.0, loss_from=0, missing_labels=False), **kw)
    assert rec.events == want and tr.steps == 42
    with pytest.raises(RuntimeError, match="loss_count is written by a step on a loss spec"):
        tr.loss_count


@pytest.mark.parametrize("kind", KINDS)
def test_a_step_on_a_spec_enqueues_exactly_this_sequence(monkeypatch, kind):
    kw, default = sched.ROWS[kind]
    want = _with_spec(default)
    tr, rec = _step(monkeypatch, SPEC, keep_best=True, **kw)
    assert rec.events == want + [("keep_best", 42)] and tr.steps == 42
    if kw.get("empty"):
        assert want == default                                   # an empty shard: the keywords are checked, the step is the one it was
        return
    assert want != default and [e[0] for e in want].count("loss_spec_grad") == 1
    assert not any(e[0] in ("bwd_mse", "mse_loss_grad") for e in want)
    assert int(tr.loss_count) == B * (T - 2) * kw.get("H", 21) and tr.loss_count.dtype == torch.int64
    if not kw.get("carry_state"):
        masks = [e[1] for e in want if e[0] == "bwd"]
        assert masks == [e[1] & ~8 for e in default if e[0] == "bwd_mse"] and all(m & D for m in masks)
    else:
        assert (tr._hcur, tr._has_state) == (1, True)
    weight = W if kw.get("exchange") else 1.0
    assert ("loss_spec_grad",) + SPEC_EVENT + (weight,) in want


def test_in_the_blocked_schedule_no_block_steps_adam_before_part_two(monkeypatch):
    kw, _ = sched.ROWS["plain-blocked"]
    _, rec = _step(monkeypatch, SPEC, **kw)
    names = [e[0] for e in rec.events]
    assert names.count("finish_rows") == 3 and rec.events.index(("bwd", 2 | D)) < names.index("finish_rows")
    assert rec.events.index(("bwd", 1 | D)) < names.index("bwd_rows")


@pytest.mark.parametrize("kind", ["plain", "state", "plain-bucket", "plain-blocked"])
def test_a_spec_step_that_raises_is_not_counted(monkeypatch, kind):
    kw, default = sched.ROWS[kind]
    want = _with_spec(default)
    for fail_at in range(len(want)):
        tr, rec = _step(monkeypatch, SPEC, fail_at=fail_at, **kw)
        assert rec.events == want[:fail_at] and tr.steps == 41, fail_at
        assert (tr._hcur, tr._has_state) == (0, False), fail_at


def test_the_range_check_follows_a_spec_step_in_f16x3(monkeypatch):
    kw, default = sched.ROWS["plain"]
    _, rec = _step(monkeypatch, SPEC, math="f16x3", **kw)
    assert rec.events == _with_spec(default) + [("check",)]


def test_forward_backward_on_a_spec_is_the_whole_backward_in_one_call(monkeypatch):
    tr, rec = _step(monkeypatch, SPEC, method="forward_backward")
    assert rec.events == sched.START[:2] + [("forward", "no labels"), ("loss_spec_grad",) + SPEC_EVENT + (1.0,), ("bwd", 7)]
    assert tr.steps == 41
    _, rec = _step(monkeypatch, None, method="forward_backward")
    assert rec.events == sched.START + [("bwd_mse", 7 | 8, 1.0)]


def test_labels_of_one_window_may_come_as_t_by_h(monkeypatch):
    rec = sched.Recorder()
    box = []
    for name, fn in _bindings(rec, 21, lambda: box[0]).items():
        monkeypatch.setattr(trainer, name, fn)
    tr = TrainStep(windgnn_amd.GCN_GRU(13, 13, 13, S * 13, 21))
    box.append(tr)
    tr.step(torch.rand(S, S), torch.rand(1, T, S, 13), torch.rand(T, 21), **SPEC)
    assert ("loss_spec_grad",) + SPEC_EVENT + (1.0,) in rec.events and int(tr.loss_count) == (T - 2) * 21


def test_a_spec_step_on_16_bit_windows_runs_on_fp32_copies_and_returns_y_in_the_windows_type(monkeypatch):
    """The loss is formed from the unrounded Y: the forward, loss_spec_grad and the backward see fp32 X, Y and L."""
    rec = sched.Recorder()
    box, seen = [], []
    b = _bindings(rec, 21, lambda: box[0])
    fwd, lsg, bwd = b["gcn_gru_forward_raw"], b["loss_spec_grad"], b["gcn_gru_backward_raw"]
    b["gcn_gru_forward_raw"] = lambda A, X, *a, **kw: (seen.append(("X", X.dtype)), fwd(A, X, *a, **kw))[1]
    b["loss_spec_grad"] = lambda Y, L, *a, **kw: (seen.append(("YL", Y.dtype, L.dtype)), lsg(Y, L, *a, **kw))[1]
    b["gcn_gru_backward_raw"] = lambda d, A, X, *a, **kw: (seen.append(("bX", X.dtype)), bwd(d, A, X, *a, **kw))[1]
    for name, fn in b.items():
        monkeypatch.setattr(trainer, name, fn)
    tr = TrainStep(windgnn_amd.GCN_GRU(13, 13, 13, S * 13, 21, math="f16x3"), check_every=0)
    box.append(tr)
    for method, n_bwd in (("step", 3), ("forward_backward", 1)):
        del seen[:]
        loss, Y = getattr(tr, method)(torch.rand(S, S), torch.rand(B, T, S, 13).bfloat16(), torch.rand(B, T, 21).bfloat16(), **SPEC)
        f32 = torch.float32
        assert Y.dtype == torch.bfloat16 and seen == [("X", f32), ("YL", f32, f32)] + [("bX", f32)] * n_bwd
    assert rec.events[0] == ("setup",) and rec.events.count(("forward", "no labels")) == 2     # the size query on the 16-bit X first
    del seen[:]
    tr.step(torch.rand(S, S), torch.rand(B, T, S, 13).bfloat16(), torch.rand(B, T, 21).bfloat16())      # the default step: as it was
    assert seen == [("X", torch.bfloat16)]


# ---- 3. refusals, each before any call ----------------------------------------------------------------------------------------------
BAD = [(dict(loss="mae"), ValueError, "TrainStep.step: loss='mae'"),
       (dict(loss="l1", loss_from=1.5), ValueError, "loss_from=1.5"),
       (dict(loss_from=-1), ValueError, "loss_from=-1"),
       (dict(loss_from=T), ValueError, "loss_from=%d" % T),
       (dict(loss="huber", huber_delta=0.0), ValueError, "huber_delta=0.0"),
       (dict(loss="huber", huber_delta=-1.0), ValueError, "huber_delta=-1.0"),
       (dict(loss="huber", huber_delta=float("inf")), ValueError, "huber_delta=inf"),
       (dict(loss="huber", huber_delta=float("nan")), ValueError, "huber_delta=nan"),
       (dict(loss="l1", labels=torch.rand(B, T - 1, 21)), ValueError, "L must be X's windows x H"),
       (dict(loss="l1", labels=torch.rand(T, 21)), ValueError, r"\[T, H\] is taken at B = 1"),
       (dict(loss="l1", labels=torch.rand(B, T, 21, dtype=torch.float64)), ValueError, "L must be float32 or X's dtype"),
       (dict(missing_labels=True, exchange="bucket"), RuntimeError, "missing_labels=True under a process group"),
       (dict(missing_labels=True, exchange="blocked", H=200), RuntimeError, "missing_labels=True under a process group"),
       (dict(missing_labels=True, exchange="bucket", empty=True), RuntimeError, "missing_labels=True under a process group"),
       (dict(loss="mae", exchange="bucket", empty=True), ValueError, "loss='mae'")]


# (an empty shard is step's alone: forward_backward has no empty-shard form)
BAD_CALLS = [(i, m) for i in range(len(BAD)) for m in ("step", "forward_backward")
             if not (m == "forward_backward" and BAD[i][0].get("empty"))]


@pytest.mark.parametrize("case,method", BAD_CALLS, ids=["%d-%s" % cm for cm in BAD_CALLS])
def test_refusals_name_the_argument_and_come_before_any_call(monkeypatch, case, method):
    kw, exc, text = BAD[case]
    kw = dict(kw)
    if method == "forward_backward":
        text = text.replace("TrainStep.step", "TrainStep.forward_backward")
    run = {k: kw.pop(k) for k in ("exchange", "empty", "H", "labels") if k in kw}
    rec = sched.Recorder()
    box = []
    H = run.get("H", 21)
    for name, fn in _bindings(rec, H, lambda: box[0]).items():
        monkeypatch.setattr(trainer, name, fn)
    tr = TrainStep(windgnn_amd.GCN_GRU(13, 13, 13, S * 13, H))
    box.append(tr)
    if "exchange" in run:
        tr.collective = True
        tr.plan = grad_block_plan(S, H, 2, 128) if run["exchange"] == "blocked" else None
        tr.exchange = sched.Exchange(rec, tr.plan)
    n = 0 if run.get("empty") else B
    L = run.get("labels", torch.rand(n, T, H))
    with pytest.raises(exc, match=text):
        getattr(tr, method)(torch.rand(S, S), torch.rand(n, T, S, 13), L, **kw)
    assert rec.events == [] and tr.steps == 0
    with pytest.raises(RuntimeError, match="loss_count"):
        tr.loss_count


def test_a_process_group_takes_every_spec_but_missing_labels(monkeypatch):
    kw, default = sched.ROWS["plain-bucket"]
    for spec in (dict(loss="l1"), dict(loss_from=T - 1), dict(loss="huber", huber_delta=2.0, loss_from=1)):
        tr, rec = _step(monkeypatch, spec, **kw)
        assert [e for e in rec.events if e[0] == "loss_spec_grad"] == [
            ("loss_spec_grad", spec.get("loss", "mse"), spec.get("huber_delta", 1.0), spec.get("loss_from", 0), False, W)]
        assert rec.events[-2:] == [("all_reduce_all", W), ("finish", 0, 42)]
