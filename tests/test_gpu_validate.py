"""Validation on materialised windows on the MI355X (TrainStep.validate): the stash-less forward of every math mode, adjacency
format and I/O type, the loss terms of functional.validation_terms and the record of include/windgnn_series_val.h updated by
functional.val_add.  tests/test_validate_host.py holds the helpers and qualifies the cases (tests/validate_cases.py) on the CPU.

The bars.  The record against the test's own fp64 loss formed from model(A, X)'s Y of the same mode: the forward is the same
call, so the residuals are the same numbers and only the order of an fp64 sum over <= 4e5 terms differs -- relative `sum` error
<= 1e-10, `count` the exact integer, `max_abs` the exact float32, `mean` and `loss` re-derived from the record's own words.
Against the fp64 oracle's forward, in the fp32-grade modes: relative `mean` error <= 1e-4, the project's bar; the one-pass f16
mode's forward precision is tests/test_gpu_parity.py's subject.  The observed errors are printed."""
import functools
import math

import pytest
import torch

import series_val_cases as sv
import validate_cases as vc
from conftest import PARAM_KEYS
from test_gpu_series import WIND_MAX, WIND_MIN, _dev
from test_gpu_series_at import _model_of

pytestmark = pytest.mark.gpu

WORDS = ("sum", "count", "mean", "max_abs", "loss", "calls")       # the words of an open pass


def _model(c, mode):
    from windgnn_amd import GCN_GRU
    m = GCN_GRU(13, 13, 13, c.S * 13, c.H, math=mode, validate=False)
    m.load_state_dict({k: v.clone() for k, v in c.p.items()})
    return m.to(_dev())


def _adj(c):
    return c.csr.to(_dev()) if c.csr is not None else c.A.to(_dev())


def _words(tr):
    """The record's public words as host tensors (one synchronisation)."""
    from windgnn_amd import _lib as L
    from windgnn_amd.functional import val_word
    rec = tr._val.cpu()
    return {name: val_word(rec, name).clone() for name in L.VAL_WORDS}


def _bytes(t):
    return t.reshape(1).contiguous().view(torch.uint8).tolist()


def _same(a, b, names=WORDS):
    """Bit equality of two records' words (the bytes are compared: NaN equals NaN)."""
    return all(_bytes(a[k]) == _bytes(b[k]) for k in names)


def _consistent(w):
    """mean == sum / count and loss == float32(mean), from the record's own words."""
    if int(w["count"]) == 0:
        return math.isnan(float(w["mean"])) and math.isnan(float(w["loss"]))
    mean = w["sum"] / w["count"]
    return _same({"mean": mean, "loss": mean.float()}, w, ("mean", "loss"))


def _assert_record(w, Y, L, kind, t_from, masked, what):
    s, m, a = vc.terms(Y, L, kind, vc.DELTA, t_from, masked)
    assert int(w["count"]) == m, what
    assert _consistent(w), what
    if math.isnan(s):
        assert math.isnan(float(w["sum"])) and math.isnan(float(w["loss"])), what
        return 0.0
    assert torch.equal(w["max_abs"], torch.tensor(a, dtype=torch.float64).float()), (what, float(w["max_abs"]), a)
    err = vc.rel(float(w["sum"]), s) if m else abs(float(w["sum"]))
    assert err <= vc.SUM_TOL, (what, err)
    return err


@functools.lru_cache(maxsize=None)
def _device_y(name, mode, io="fp32"):
    """model(A, X)'s Y of a mode under torch.no_grad(), on the host ([B, T, H]): the reference of the accumulation check."""
    c = vc.case(name)
    dt = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[io]
    with torch.no_grad():
        Y = _model(c, mode)(_adj(c), c.X.to(_dev()).to(dt))
    return Y.reshape(c.B, c.T, c.H).cpu()


IO_CASES = [("real", "f16", "bf16"), ("odd", "f16x3", "fp16")]


@pytest.mark.parametrize("name,mode,io", [(n, m, "fp32") for n in vc.SHAPES for m in vc.MODES] + IO_CASES)
def test_the_record_is_the_fp64_loss_of_the_same_forward(name, mode, io):
    from windgnn_amd.trainer import TrainStep
    c = vc.case(name)
    dev = _dev()
    dt = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}[io]
    Y = _device_y(name, mode, io)
    A, X = _adj(c), c.X.to(dev).to(dt)
    tr = TrainStep(_model(c, mode), keep_best=True, best_on="validation")
    worst, passes, stale, won = 0.0, 0, 0, False
    for mask in vc.MASKS:
        Lh = vc.labels(c, mask).to(dt)                           # what the device reads: rounded to the I/O type
        Ld = Lh.to(dev)
        if name == "tiny":
            Ld = Ld[0]                                           # [T, H], as the reference's loader yields it
        elif io == "bf16":
            Ld = Ld.float()                                      # fp32 labels beside 16-bit X: the same values
        for kind in vc.KINDS:
            for t_from in vc.t_froms(c.T):
                what = (name, mode, io, mask, kind, t_from)
                masked = mask != "none"
                v = tr.validate(A, X, Ld, missing_labels=masked, loss=kind, huber_delta=vc.DELTA, loss_from=t_from)
                assert v.dim() == 0 and v.dtype == torch.float32 and v.data_ptr() == tr.val_loss.data_ptr()
                w = _words(tr)
                worst = max(worst, _assert_record(w, Y, Lh, kind, t_from, masked, what))
                passes += 1
                if mask == "all":                                # no label at all: count 0, NaN, and the pass does not win
                    assert int(w["count"]) == 0 and math.isnan(float(v)) and int(tr.improved) == 0
                stale = 0 if int(tr.improved) else stale + 1
                won = won or bool(int(tr.improved))
                assert (int(w["passes"]), int(w["stale"]), int(w["calls"])) == (passes, stale, 1), what
    assert won and stale >= len(vc.KINDS) * len(vc.t_froms(c.T))       # val_stale grew over the label-less passes
    tr.check()
    print("\n%s %s %s: %d passes, worst relative sum error %.2e" % (name, mode, io, passes, worst))


def test_a_nan_label_without_missing_labels_poisons_the_record_and_does_not_win():
    from windgnn_amd.trainer import TrainStep
    c = vc.case("odd")
    dev = _dev()
    A, X = _adj(c), c.X.to(dev)
    tr = TrainStep(_model(c, "f16x3"), keep_best=True, best_on="validation")
    L = c.L.clone()
    L[2, 1, 3] = float("nan")                                    # step 1: outside M from step 2 on, inside it from step 0
    v = tr.validate(A, X, L.to(dev), loss_from=2)
    w = _words(tr)
    assert math.isfinite(float(v)) and int(w["count"]) == c.B * (c.T - 2) * c.H and int(tr.improved) == 1
    _assert_record(w, _device_y("odd", "f16x3"), c.L, "mse", 2, False, "a NaN before loss_from")
    v = tr.validate(A, X, L.to(dev))
    w = _words(tr)
    assert math.isnan(float(v)) and math.isnan(float(w["sum"])) and math.isnan(float(w["max_abs"]))
    assert int(w["count"]) == c.B * c.T * c.H and (int(tr.improved), int(w["stale"]), int(tr.best_step)) == (0, 1, 0)


@pytest.mark.parametrize("name", list(vc.SHAPES))
@pytest.mark.parametrize("mode", vc.GRADE32)
def test_the_mean_is_the_fp64_oracles_within_the_projects_bar(name, mode):
    from windgnn_amd.trainer import TrainStep
    c = vc.case(name)
    dev = _dev()
    A, X = _adj(c), c.X.to(dev)
    tr = TrainStep(_model(c, mode))
    worst = 0.0
    for mask in ("none", "tenth"):
        L = vc.labels(c, mask)
        for kind in vc.KINDS:
            for t_from in vc.t_froms(c.T):
                s, m, _ = vc.terms(c.Yo, L, kind, vc.DELTA, t_from, mask != "none")
                tr.validate(A, X, L.to(dev), missing_labels=mask != "none", loss=kind, huber_delta=vc.DELTA, loss_from=t_from)
                w = _words(tr)
                err = vc.rel(float(w["mean"]), s / m)
                worst = max(worst, err)
                assert int(w["count"]) == m and err <= vc.TOL, (name, mode, mask, kind, t_from, err)
    print("\n%s %s: worst relative mean error against the fp64 oracle %.2e" % (name, mode, worst))


@pytest.mark.parametrize("mode", ["f32", "f16x3"])
def test_a_pass_over_several_calls_counts_exactly_and_two_passes_give_the_same_bits(mode):
    from windgnn_amd.trainer import TrainStep
    c = vc.case("odd")
    dev = _dev()
    A, X = _adj(c), c.X.to(dev)
    L = vc.labels(c, "tenth").to(dev)
    tr = TrainStep(_model(c, mode))
    kw = dict(missing_labels=True, loss="huber", huber_delta=vc.DELTA, loss_from=2)
    tr.validate(A, X, L, **kw)
    one = _words(tr)
    tr.validate(A, X, L, **kw)
    again = _words(tr)
    assert _same(one, again) and int(again["passes"]) == 2       # two identical passes: identical bits
    for cuts in ((0, 2, 5), (0, 1, 3, 5)):
        for lo, hi in zip(cuts, cuts[1:]):
            tr.validate(A, X[lo:hi], L[lo:hi], more=hi < c.B, **kw)
        w = _words(tr)
        assert int(w["count"]) == int(one["count"]) and int(w["calls"]) == len(cuts) - 1 and _consistent(w)
        assert torch.equal(w["max_abs"], one["max_abs"])
        assert vc.rel(float(w["sum"]), float(one["sum"])) <= vc.SUM_TOL
    assert int(w["passes"]) == 4


def test_a_pass_may_mix_series_calls_and_materialised_windows():
    from windgnn_amd.trainer import TrainStep
    q = sv.reference("irregular-table-e-huber-from2")
    dev = _dev()
    A, Xs, Ls = q.A.to(dev), q.Xs.to(dev), q.Ls.to(dev)
    cut = 9
    tr = TrainStep(_model_of(q.r))
    kw = dict(loss="huber", huber_delta=q.delta, loss_from=q.t_from)
    tr.validate_series(A, Xs, Ls, q.T, starts=q.starts[:cut], more=True, **kw)
    first = _words(tr)
    v = tr.validate(A, q.X[cut:].to(dev), q.L[cut:].to(dev), **kw)
    w = _words(tr)
    m2 = (q.n - cut) * (q.T - q.t_from) * q.H
    assert int(first["count"]) == cut * (q.T - q.t_from) * q.H and int(w["count"]) == int(first["count"]) + m2 == q.m
    assert (int(w["calls"]), int(w["passes"])) == (2, 1) and _consistent(w)
    err = vc.rel(float(w["mean"]), q.loss_o)
    print("\nmixed pass: relative mean error against the oracle over the union %.2e" % err)
    assert err <= vc.TOL and float(v) == float(w["loss"])
    # ... and the other way round: the record does not care who wrote it first
    tr.validate(A, q.X[cut:].to(dev), q.L[cut:].to(dev), more=True, **kw)
    tr.validate_series(A, Xs, Ls, q.T, starts=q.starts[:cut], **kw)
    w2 = _words(tr)
    assert int(w2["count"]) == q.m and vc.rel(float(w2["mean"]), q.loss_o) <= vc.TOL and _consistent(w2)


@pytest.mark.parametrize("name,mode", vc.SCENARIOS)
def test_the_best_model_and_the_patience_counter_follow_the_held_out_loss(name, mode):
    from oracle import windgnn_oracle as orc
    from windgnn_amd.trainer import TrainStep
    vals, ct, ch = vc.scenario(name)
    want = vc.rule(vals + vals[-1:])                             # a fifth pass on unchanged parameters: equal, so no win
    dev = _dev()
    A = _adj(ct)
    Xt, Lt, Xv, Lv = ct.X.to(dev), ct.L.to(dev), ch.X.to(dev), ch.L.to(dev)
    tr = TrainStep(_model(ct, mode), lr=vc.LR, keep_best=True, best_on="validation")
    got, own, seq, snaps = [], [], [], []

    def held_out():
        """A closed pass; beside it the fp64 oracle's held-out loss at the DEVICE's current parameters, which is what check 2's
        bar speaks of (the oracle's own trajectory differs from the device's by the training step's error, not validate's)."""
        snaps.append(tr.flat_p.clone())
        got.append(float(tr.validate(A, Xv, Lv)))
        seq.append((int(tr.best_step), int(tr.improved), int(tr.val_stale)))
        p = {k: v.detach().cpu().double() for k, v in zip(PARAM_KEYS, tr.p_views)}
        s, m, _ = vc.terms(orc.forward(ct.A.double(), ch.X.double(), p, want_cache=False)[0], ch.L, "mse", 0.0, 0, False)
        own.append(s / m)
    held_out()
    for k in range(vc.STEPS):
        before = int(tr.best_step)
        tr.step(A, Xt, Lt + vc.SHIFT if k == 2 else Lt)
        assert int(tr.best_step) == before                       # a training step decides nothing
        held_out()
    held_out()
    err = [vc.rel(a, b) for a, b in zip(got, own)]
    drift = [vc.rel(a, b) for a, b in zip(got, vals + vals[-1:])]
    print("\n%s %s: held-out losses %s; against the oracle at the same parameters %s; against the oracle's own trajectory %s"
          % (name, mode, got, " ".join("%.2e" % e for e in err), " ".join("%.2e" % e for e in drift)))
    assert max(err) <= vc.TOL, err
    assert max(drift) < 1e-3 / 2, drift                          # the losses are >= 1e-3 apart: the sequence is the oracle's
    assert seq == want and int(tr.val_passes) == vc.STEPS + 2 and tr.steps == vc.STEPS
    best = want[-1][0]
    assert float(tr.best_loss) == got[best] and best != vc.STEPS
    assert torch.equal(tr._best_p, snaps[best]) and not torch.equal(tr._best_p, tr.flat_p)
    tr.restore_best()
    assert torch.equal(tr.flat_p, snaps[best])                   # the winning step's parameters, bit for bit
    tr.check()


def _state(tr):
    out = [tr.flat_p, tr.exp_avg, tr.exp_avg_sq, tr._gbuf, tr._best, tr._best_p, tr._prepared]
    if tr.carry_state:
        out += [tr._hbuf, torch.tensor([tr._hcur, int(tr._has_state)])]
    return [t.clone() for t in out] + [torch.tensor(tr.steps)]


@pytest.mark.parametrize("name,mode,carry", [("odd", "f16x3", False), ("odd", "f32", True), ("csr", "f16x3g", False)])
def test_validate_changes_nothing_a_step_owns(name, mode, carry):
    from windgnn_amd.evaluate import Evaluator
    from windgnn_amd.trainer import TrainStep
    c, ch = vc.case(name), vc.case(name, seed=1)
    dev = _dev()
    A, X, L, Xv, Lv = _adj(c), c.X.to(dev), c.L.to(dev), ch.X.to(dev), ch.L.to(dev)
    runs = []
    for validate in (False, True):
        model = _model(c, mode)
        tr = TrainStep(model, keep_best=True, best_on="train", max_grad_norm=1.0, carry_state=carry)
        ev = Evaluator(model, A, WIND_MIN, WIND_MAX)
        losses = []
        for k in range(3):
            loss, _ = tr.step(A, X, L)
            losses.append(loss.clone())
            if validate:
                before = _state(tr)
                tr.validate(A, Xv[:2], Lv[:2], more=True, loss="huber", huber_delta=vc.DELTA, loss_from=1)
                tr.validate(A, Xv, Lv, evaluator=ev, loss="huber", huber_delta=vc.DELTA, loss_from=c.T - 1)
                for a, b in zip(before, _state(tr)):
                    assert torch.equal(a, b)
        runs.append(_state(tr) + [torch.stack(losses)])
        if validate:
            assert int(tr.val_passes) == 3 and int(tr.val_stale) == 0 and int(tr.val_count) == (2 * (c.T - 1) + c.B) * c.H
    for a, b in zip(*runs):                                      # a step after a validate: the bits of a step without it
        assert torch.equal(a, b)


@pytest.mark.parametrize("name,mode", [("odd", "f32"), ("odd", "f16x3"), ("real", "f16x3g"), ("wide", "f16x3"), ("csr", "f32"),
                                       ("tiny", "f16")])
def test_the_evaluator_gets_the_bits_update_gives_it(name, mode):
    from windgnn_amd.evaluate import Evaluator
    from windgnn_amd.trainer import TrainStep
    c = vc.case(name)
    dev = _dev()
    A, X, L = _adj(c), c.X.to(dev), c.L.to(dev)
    model = _model(c, mode)
    tr = TrainStep(model)
    for t_from in (0, c.T - 1):                                  # the full route and the last-step route
        ev1, ev2 = (Evaluator(model, A, WIND_MIN, WIND_MAX, keep_errors=True) for _ in range(2))
        tr.validate(A, X, L, loss_from=t_from, evaluator=ev1)
        ev2.update(X, L)
        assert bool(ev1.acc.any()) and torch.equal(ev1.acc, ev2.acc), (name, mode, t_from)
        assert torch.equal(ev1.errors(), ev2.errors())


@pytest.mark.parametrize("name,mode", [(n, m) for n in ("odd", "real", "wide", "csr") for m in vc.MODES])
def test_the_last_step_route_gives_the_full_routes_record(name, mode):
    """loss_from = T - 1 with fp32 X runs wgnn_fwd_last with (0, 1); the full route's record of the same spec is formed here
    from model(A, X)'s Y through the same two helpers."""
    from windgnn_amd.functional import val_add, val_begin, val_buffer, val_word, validation_terms
    from windgnn_amd import _lib as LB
    from windgnn_amd.trainer import TrainStep
    c = vc.case(name)
    dev = _dev()
    A, X = _adj(c), c.X.to(dev)
    model = _model(c, mode)
    tr = TrainStep(model)
    for mask, kind in (("none", "mse"), ("tenth", "huber"), ("tenth", "l1")):
        Lh = vc.labels(c, mask)
        L = Lh.to(dev)
        masked = mask != "none"
        tr.validate(A, X, L, missing_labels=masked, loss=kind, huber_delta=vc.DELTA, loss_from=c.T - 1)
        w = _words(tr)
        with torch.no_grad():
            Y = model(A, X).reshape(c.B, c.T, c.H)
        rec = val_buffer(dev)
        val_begin(rec)
        val_add(rec, *validation_terms(Y, L, kind, vc.DELTA, c.T - 1, masked))
        full = {k: val_word(rec.cpu(), k).clone() for k in LB.VAL_WORDS}
        if mode == "f32":
            assert _same(w, full), (name, mode, mask, kind)      # bit for bit
        _assert_record(w, Y, Lh, kind, c.T - 1, masked, (name, mode, mask, kind))


def test_a_side_stream_gives_the_default_streams_bits():
    from windgnn_amd.trainer import TrainStep
    c = vc.case("real")
    dev = _dev()
    A, X = _adj(c), c.X.to(dev)
    L = vc.labels(c, "tenth").to(dev)
    kw = dict(missing_labels=True, loss="l1", loss_from=2)

    def run():
        tr = TrainStep(_model(c, "f16x3"), keep_best=True, best_on="validation")
        tr.validate(A, X[:1], L[:1], more=True, **kw)
        tr.validate(A, X[1:], L[1:], **kw)
        return tr
    ref = _words(run())
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        tr = run()
    side.synchronize()
    w = _words(tr)
    assert _same(w, ref, tuple(ref)) and int(w["calls"]) == 2 and int(w["passes"]) == 1 and int(tr.best_step) == 0
