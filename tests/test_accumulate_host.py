"""TrainStep.accumulate / accumulate_series / apply / discard without a GPU: the refusals, the call sequences on the recorders of
tests/test_trainstep_schedule_host.py, the weight arithmetic of windgnn_amd/accumulate.py on CPU tensors against an fp64
evaluation, and two and three ranks over gloo with the fp64 oracle as the compute and the real BucketExchange
(as tests/test_distributed_cpu.py runs it).  Every test calls accumulate* / apply, or the Accumulation they are built on."""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist

import test_trainstep_schedule_host as sh
import windgnn_amd
from conftest import PARAM_KEYS, load_fixture, rel_to_max
from windgnn_amd import _lib, trainer
from windgnn_amd.accumulate import Accumulation
from windgnn_amd.distributed import HEADER, LOSS_SLOT, grad_block_plan
from windgnn_amd.trainer import TrainStep

S, T, B, W = sh.S, sh.T, sh.B, sh.W
H = 21
FULL = 7 | 8                    # forward_backward's one backward: every part and the loss, nothing deferred


def _spec_bindings(rec):
    """The recorders' forward and series calls taking a loss spec as well (the shared ones pin the MSE defaults), and recorders
    for what a step on a spec calls besides: functional.loss_spec_grad (the count is the real one) and wgnn_bwd_part."""
    shared = sh._bindings(rec, H)

    def gcn_gru_forward_raw(A, X, params, math=0, want_stash=True, labels=None, prepared=None):
        if labels is not None:
            return shared["gcn_gru_forward_raw"](A, X, params, math, want_stash, labels, prepared)
        rec("forward_without_labels")
        return (torch.zeros(X.shape[0], X.shape[1], H), None,
                _lib.Dims(X.shape[0], X.shape[1], X.shape[2], 13, H, math, _lib.ADJ_DENSE, 0, _lib.IO_F32))

    def loss_spec_grad(Y, L, loss="mse", huber_delta=1.0, loss_from=0, missing_labels=False, grad_scale=1.0, loss_out=None,
                       who=""):
        rec("spec_loss", loss, grad_scale)
        counted = L[:, loss_from:]
        return loss_out, torch.zeros_like(Y), (~torch.isnan(counted)).sum() if missing_labels else torch.tensor(counted.numel())

    def gcn_gru_backward_raw(d, A, X, params, Y, dY, stash, grads, part=7, stream=None, prepared=None):
        rec("bwd", part)

    def series_forward_loss_raw(A, series, Ls, seq_len, stride, params, math=0, n_windows=None, prepared=None, **spec):
        return shared["series_forward_loss_raw"](A, series, Ls, seq_len, stride, params, math, n_windows, prepared)

    def series_backward_mse_raw(sd, A, series, params, Y, Ls, stash, loss_buf, grads, loss, grad_scale=1.0, prepared=None, **spec):
        shared["series_backward_mse_raw"](sd, A, series, params, Y, Ls, stash, loss_buf, grads, loss, grad_scale, prepared)

    return dict(gcn_gru_forward_raw=gcn_gru_forward_raw, loss_spec_grad=loss_spec_grad, gcn_gru_backward_raw=gcn_gru_backward_raw,
                series_forward_loss_raw=series_forward_loss_raw, series_backward_mse_raw=series_backward_mse_raw)


def _tr(monkeypatch, exchange=None, keep_best=False, math="f32", **kw):
    """A CPU-constructed TrainStep on the recorders, at steps = 41."""
    rec = sh.Recorder()
    for name, fn in dict(sh._bindings(rec, H), **_spec_bindings(rec)).items():
        monkeypatch.setattr(trainer, name, fn)
    tr = TrainStep(windgnn_amd.GCN_GRU(13, 13, 13, S * 13, H, math=math), check_every=1, **kw)
    if exchange is not None:
        tr.collective = True
        tr.overlap_collectives = exchange == "overlap"
        tr.plan = grad_block_plan(S, 200, 2, 128) if exchange == "blocked" else None
        tr.exchange = sh.Exchange(rec, tr.plan)
    if keep_best:
        tr._best_call = ("marshalled once",)
    tr.steps = 41
    return tr, rec


def _windows(n, t=T):
    return torch.rand(S, S), torch.rand(n, t, S, 13), torch.rand(n, t, H)


def _series(rows=14):
    return torch.rand(S, S), torch.rand(rows, S, 13), torch.rand(rows, H)


# ---- 1. refusals ---------------------------------------------------------------------------------------------------------------
def _refused(tr, rec, call, match, exc=RuntimeError):
    before, n_events, open_calls = tr._gbuf.clone(), len(rec.events), tr.accumulated
    with pytest.raises(exc, match=match):
        call()
    assert len(rec.events) == n_events, rec.events[n_events:]           # before any recorded call
    assert tr.steps == 41 and torch.equal(tr._gbuf, before) and tr.accumulated == open_calls


@pytest.mark.parametrize("how,match", [("blocked", "grad_blocks.*step\\(\\) per batch"),
                                       ("overlap", "overlap_collectives=True.*step\\(\\) per batch"),
                                       ("carry", "carry_state=True.*truncated BPTT.*follow-up.*step\\(\\) per chunk")])
@pytest.mark.parametrize("series", [False, True])
def test_schedules_that_step_before_the_whole_bucket_exists_are_refused_by_name(monkeypatch, how, match, series):
    tr, rec = _tr(monkeypatch, exchange=how if how != "carry" else None, carry_state=how == "carry")
    if series:
        A, ser, Ls = _series()
        _refused(tr, rec, lambda: tr.accumulate_series(A, ser, Ls, T, 3), "accumulate_series with " + match)
    else:
        A, X, L = _windows(B)
        _refused(tr, rec, lambda: tr.accumulate(A, X, L), "accumulate with " + match)


def test_a_call_on_another_loss_than_the_open_accumulation_is_refused(monkeypatch):
    tr, rec = _tr(monkeypatch)
    A, X, L = _windows(B)
    tr.accumulate(A, X, L, loss="huber", huber_delta=0.25)
    _refused(tr, rec, lambda: tr.accumulate(A, X, L, loss="l1"), "loss='l1'.*holds calls on loss='huber', huber_delta=0.25.*one loss.*"
                                                                 "apply\\(\\) or discard\\(\\)")
    _refused(tr, rec, lambda: tr.accumulate(A, X, L, loss="huber", huber_delta=0.5), "huber_delta=0.5.*huber_delta=0.25")
    As, ser, Ls = _series()
    _refused(tr, rec, lambda: tr.accumulate_series(As, ser, Ls, T, 3), "accumulate_series: loss='mse'.*loss='huber'")
    tr.accumulate(A, X, L, loss="huber", huber_delta=0.25, loss_from=2)       # one rank: another loss_from is still one loss
    assert tr.accumulated == 2
    tr.discard()
    tr.accumulate(A, X, L)
    tr.accumulate(A, X, L, huber_delta=3.0)                                   # huber_delta counts with loss="huber" only
    assert tr.accumulated == 2


def test_missing_labels_under_a_process_group_keeps_todays_refusal(monkeypatch):
    tr, rec = _tr(monkeypatch, exchange="bucket")
    A, X, L = _windows(B)
    _refused(tr, rec, lambda: tr.accumulate(A, X, L, missing_labels=True),
             "forward_backward with missing_labels=True under a process group.*label counts would have to be exchanged")
    As, ser, Ls = _series()
    _refused(tr, rec, lambda: tr.accumulate_series(As, ser, Ls, T, 3, missing_labels=True),
             "missing_labels=True under a process group.*label counts")


def test_under_a_process_group_the_calls_share_T_and_loss_from(monkeypatch):
    tr, rec = _tr(monkeypatch, exchange="bucket")
    A, X, L = _windows(B)
    tr.accumulate(A, X, L, loss="l1", loss_from=2)
    _refused(tr, rec, lambda: tr.accumulate(*_windows(B, 4), loss="l1", loss_from=2), "\\(4, 2\\).*\\(5, 2\\)")
    _refused(tr, rec, lambda: tr.accumulate(A, X, L, loss="l1", loss_from=1), "\\(5, 1\\).*\\(5, 2\\)")
    As, ser, Ls = _series()
    _refused(tr, rec, lambda: tr.accumulate_series(As, ser, Ls, 4, 3, loss="l1", loss_from=2), "\\(4, 2\\).*\\(5, 2\\)")
    tr.accumulate_series(As, ser, Ls, T, 3, loss="l1", loss_from=2)
    assert tr.accumulated == 2
    one, _ = _tr(monkeypatch)                                                 # one rank: the labels weigh, any T goes
    one.accumulate(A, X, L)
    one.accumulate(*_windows(B, 4))
    assert one.accumulated == 2


def test_apply_with_nothing_accumulated_is_refused_on_one_rank(monkeypatch):
    tr, rec = _tr(monkeypatch)
    _refused(tr, rec, tr.apply, "apply\\(\\): nothing was accumulated.*accumulate\\(\\) or accumulate_series\\(\\) first")
    tr.accumulate(*_windows(B))
    tr.discard()
    _refused(tr, rec, tr.apply, "nothing was accumulated")


def test_whatever_writes_the_bucket_is_refused_while_an_accumulation_is_open(monkeypatch):
    tr, rec = _tr(monkeypatch)
    A, X, L = _windows(B)
    As, ser, Ls = _series()
    tr.accumulate(A, X, L)
    for name, call in (("step", lambda: tr.step(A, X, L)), ("step_series", lambda: tr.step_series(As, ser, Ls, T, 3)),
                       ("forward_backward", lambda: tr.forward_backward(A, X, L)),
                       ("forward_backward_series", lambda: tr.forward_backward_series(As, ser, Ls, T, 3)),
                       ("state_dict\\(\\)", tr.state_dict), ("load_state_dict\\(\\)", lambda: tr.load_state_dict({}))):
        _refused(tr, rec, call, "TrainStep.%s while an accumulation is open \\(1 call .*apply\\(\\).*discard\\(\\)" % name)
    tr.discard()
    n = len(rec.events)
    tr.step(A, X, L)                                                           # and after discard() they run again
    assert tr.steps == 42 and len(rec.events) > n


def test_what_forward_backward_refuses_stays_refused_with_its_message(monkeypatch):
    tr, rec = _tr(monkeypatch)
    A, X, L = _windows(B)
    _refused(tr, rec, lambda: tr.accumulate(A, X, L, loss="quantile"), "forward_backward: loss='quantile'", ValueError)
    _refused(tr, rec, lambda: tr.accumulate(A, X, L, loss_from=T), "loss_from", ValueError)
    _refused(tr, rec, lambda: tr.accumulate(A, X[:0], L[:0]), "accumulate needs at least one window.*still calls apply\\(\\)")
    As, ser, Ls = _series()
    _refused(tr, rec, lambda: tr.accumulate_series(As, ser, Ls, T, 3, n_windows=0), "needs at least one window")
    f16, rec16 = _tr(monkeypatch, math="f16x3")
    _refused(f16, rec16, lambda: f16.accumulate_series(As, ser, Ls, T, 3), "step_series with math != 'f32'")


# ---- 2. call sequences ---------------------------------------------------------------------------------------------------------
FIRST = [("setup",), ("images",), ("forward",), ("bwd_mse", FULL, 1.0)]
LATER = [("forward",), ("bwd_mse", FULL, 1.0)]
SER = lambda n: [("require_gpu",), ("series_forward_loss", n), ("series_bwd_mse", 1.0)]        # noqa: E731

TAILS = {"one": (dict(), [("finish", 0, 42)]),
         "one-clipped": (dict(max_grad_norm=2.0), [("finish_norm", 0, 2.0), ("finish_clipped", 42)]),
         "bucket": (dict(exchange="bucket"), [("all_reduce_all", W), ("finish", 0, 42)]),
         "bucket-clipped": (dict(exchange="bucket", max_grad_norm=2.0),
                            [("all_reduce_all", W), ("finish_norm", 0, 2.0), ("finish_clipped", 42)])}


@pytest.mark.parametrize("keep_best", [False, True])
@pytest.mark.parametrize("tail", list(TAILS))
@pytest.mark.parametrize("k", [1, 3])
def test_k_calls_record_k_forward_backward_pairs_and_apply_one_tail(monkeypatch, k, tail, keep_best):
    kw, want_tail = TAILS[tail]
    tr, rec = _tr(monkeypatch, keep_best=keep_best, **kw)
    A = torch.rand(S, S)
    sizes = [4, 1, 2][:k]
    for i, n in enumerate(sizes):
        loss, Y = tr.accumulate(A, torch.rand(n, T, S, 13), torch.rand(n, T, H))
        assert loss.dim() == 0 and loss.data_ptr() != tr._loss.data_ptr() and tuple(Y.shape) == (n, T, H)     # a clone
        assert tr.accumulated == i + 1 and tr.steps == 41
    assert rec.events == FIRST + LATER * (k - 1)            # no exchange and no finish event, with or without a group
    assert int(tr.accumulated_count) == sum(sizes) * T * H
    del rec.events[:]
    out = tr.apply()
    assert out is tr._loss and tr.steps == 42 and tr.accumulated == 0
    head = [("shard_weight", sum(sizes))] if "bucket" in tail else []           # this rank's windows over all its calls
    assert rec.events == head + want_tail + ([("keep_best", 42)] if keep_best else [])


def test_materialised_and_series_calls_alternate_within_one_accumulation(monkeypatch):
    tr, rec = _tr(monkeypatch, exchange="bucket", keep_best=True)
    A, X, L = _windows(3)
    As, ser, Ls = _series()
    tr.accumulate_series(As, ser, Ls, T, 3, n_windows=4)
    tr.accumulate(A, X, L)
    tr.accumulate_series(As, ser, Ls, T, 3, n_windows=2)
    assert rec.events == ([("require_gpu",), ("images",)] + SER(4)[1:] + LATER + SER(2))
    assert int(tr.accumulated_count) == (4 + 3 + 2) * T * H and tr.accumulated == 3
    del rec.events[:]
    tr.apply(n_global=20)
    assert rec.events == [("shard_weight", 9), ("all_reduce_all", W), ("finish", 0, 42), ("keep_best", 42)]


def test_calls_on_a_spec_weigh_by_their_labels_and_missing_labels_by_a_device_count(monkeypatch):
    tr, rec = _tr(monkeypatch)
    A, X, L = _windows(3)
    tr.accumulate(A, X, L, loss="l1", loss_from=2)
    assert rec.events == [("setup",), ("images",), ("forward_without_labels",), ("spec_loss", "l1", 1.0), ("bwd", 7)]
    assert tr._acc._host == (3 * (T - 2) * H,) * 2                           # a host integer: no device count was needed
    L2 = L.clone()
    L2[0, :, ::2] = float("nan")
    L2[1, 1] = float("nan")                                                   # before loss_from: not counted either way
    want = int((~torch.isnan(L2[:, 2:])).sum())
    tr.accumulate(A, X, L2, loss="l1", loss_from=2, missing_labels=True)
    assert tr._acc._host is None and int(tr.accumulated_count) == 3 * (T - 2) * H + want
    assert tr.accumulated_count.dtype == torch.int64 and tr.accumulated_count.dim() == 0
    As, ser, Ls = _series()
    tr.accumulate_series(As, ser, Ls, T, 3, n_windows=2, loss="l1", loss_from=1)     # one rank: another loss_from goes
    assert int(tr.accumulated_count) == 3 * (T - 2) * H + want + 2 * (T - 1) * H
    tr.apply()
    assert rec.events[-1] == ("finish", 0, 42) and tr.accumulated == 0


def test_a_rank_that_accumulated_nothing_joins_the_same_collectives(monkeypatch):
    tr, rec = _tr(monkeypatch, exchange="bucket", keep_best=True, math="f16x3")
    tr._gbuf.fill_(3.0)
    tr.apply()
    assert rec.events == [("images",), ("shard_weight", 0), ("all_reduce_all", 0.0), ("finish", 0, 42), ("keep_best", 42)]
    assert tr.steps == 42 and not tr._gbuf.any()                        # a zero bucket, and no host read (no check)
    tr.accumulate(*_windows(B))                                         # the same object then takes part with windows
    del rec.events[:]
    tr.apply()
    assert rec.events == [("shard_weight", B), ("all_reduce_all", W), ("finish", 0, 43), ("keep_best", 43), ("check",)]


def test_the_range_check_follows_apply_in_the_fp16_plane_modes(monkeypatch):
    tr, rec = _tr(monkeypatch, math="f16x3")
    tr.accumulate(*_windows(B))
    assert ("check",) not in rec.events
    tr.apply()
    assert rec.events[-2:] == [("finish", 0, 42), ("check",)]


def test_an_apply_that_raises_is_not_counted(monkeypatch):
    for tail in TAILS:
        kw, want_tail = TAILS[tail]
        head = 1 if "bucket" in tail else 0
        for fail_at in range(head + len(want_tail)):
            tr, rec = _tr(monkeypatch, keep_best=True, **kw)
            tr.accumulate(*_windows(B))
            n = len(rec.events)
            rec.fail_at = n + fail_at
            with pytest.raises(sh.Boom):
                tr.apply()
            assert len(rec.events) == n + fail_at and tr.steps == 41 and tr.accumulated == 1, (tail, fail_at)
            tr.discard()
            assert tr.accumulated == 0 and tr.steps == 41


def test_a_call_that_raises_leaves_the_accumulation_as_it_was(monkeypatch):
    tr, rec = _tr(monkeypatch)
    A, X, L = _windows(B)
    tr._gbuf.copy_(torch.randn(tr._gbuf.numel()))
    tr.accumulate(A, X, L)
    tr._gbuf.copy_(torch.randn(tr._gbuf.numel()))
    As, ser, Ls = _series()
    tr.accumulate_series(As, ser, Ls, T, 3, n_windows=3)
    G, words = tr._acc.buf.clone(), tr._acc._words.clone()
    for series in (False, True):
        for fail_at in range(2):
            rec.fail_at = len(rec.events) + fail_at
            tr._gbuf.copy_(torch.randn(tr._gbuf.numel()))
            with pytest.raises(sh.Boom):
                tr.accumulate_series(As, ser, Ls, T, 3) if series else tr.accumulate(A, X, L)
            assert torch.equal(tr._acc.buf.view(torch.int32), G.view(torch.int32)) and torch.equal(tr._acc._words, words)
            assert tr.accumulated == 2 and int(tr.accumulated_count) == (B + 3) * T * H and tr._acc_windows == B + 3
    rec.fail_at = None


# ---- 3. the weight arithmetic on CPU tensors, against fp64 ---------------------------------------------------------------------
N = HEADER + 1000


def _buckets(k, seed=0):
    g = torch.Generator().manual_seed(900 + seed)
    return [(torch.rand(N, generator=g) * 2 - 1) * 10.0 ** float(torch.randint(-3, 3, (1,), generator=g)) for _ in range(k)]


def _fp64(buckets, counts, weight=1.0):
    """The bucket of one call on the union, in fp64: sum c_i b_i / C, the gradients times the shard's weight."""
    C = float(sum(counts))
    out = sum(float(c) * b.double() for c, b in zip(counts, buckets)) / C
    mag = sum(float(c) * b.double().abs() for c, b in zip(counts, buckets)) / C
    loss = out[LOSS_SLOT].clone()
    out, mag = out * weight, mag * weight
    out[LOSS_SLOT] = loss
    mag[LOSS_SLOT] = mag[LOSS_SLOT] / weight
    return out, mag


def _run(buckets, counts, weight=1.0, as_tensor=()):
    acc = Accumulation(buckets[0])
    for i, (b, c) in enumerate(zip(buckets, counts)):
        acc.add(b, torch.tensor(c, dtype=torch.int64) if i in as_tensor else c)
    out = torch.full((N,), float("nan"))
    acc.write(out, LOSS_SLOT, weight)
    return acc, out


@pytest.mark.parametrize("counts", [(1, 2, 3), (4096, 1, 17), (7,)])
@pytest.mark.parametrize("weight", [1.0, 0.375])
def test_the_accumulated_bucket_is_the_count_weighted_mean_of_the_calls(counts, weight):
    """Error bound, per element and relative to sum |c_i b_i| / C: the weight's rounding, the product's and the k - 1 partial
    sums' (2^-24 each; fewer where the multiply-add is fused), then c_1 / C's rounding and the final product's, and with a
    shard weight its product with c_1 / C: at most (k + 5) roundings of 2^-24.  The bar is (k + 5) * 2^-23, twice that."""
    k = len(counts)
    buckets = _buckets(k, sum(counts))
    acc, out = _run(buckets, counts, weight)
    ref, mag = _fp64(buckets, counts, weight)
    err = float(((out.double() - ref).abs() / mag.clamp_min(1e-300)).max())
    print("counts %s weight %g: worst error %.2e of sum |c_i b_i| / C (bar %.2e)" % (counts, weight, err, (k + 5) * 2.0 ** -23))
    assert err <= (k + 5) * 2.0 ** -23
    assert int(acc.count) == sum(counts) and acc.calls == k
    # the window-weighted (plain) mean is another number wherever the counts differ
    if len(set(counts)) > 1:
        plain = sum(b.double() for b in buckets) / k
        assert float(((plain - ref).abs() / mag)[HEADER:].max()) > 1e-3


def test_one_call_alone_has_factors_of_exactly_one_and_returns_its_bucket_bit_for_bit():
    b = _buckets(1, 5)[0]
    b[HEADER] = -0.0                                        # (a copy keeps the sign of a zero; 0 + 1.0 * -0 would not)
    for count in (1, 3, 4096 * 24 * 102, torch.tensor(77)):
        acc, out = _run([b], [count])
        assert torch.equal(acc.buf.view(torch.int32), b.view(torch.int32))
        assert torch.equal(out.view(torch.int32), b.view(torch.int32))
        assert int(acc.count) == int(count)
    from windgnn_amd.accumulate import _weight
    assert float(_weight(5, 5, "cpu")) == 1.0 and float(_weight(torch.tensor(5), torch.tensor(5), "cpu")) == 1.0


@pytest.mark.parametrize("counts", [(1, 2, 3), (4096, 1, 17), (3, 3)])
def test_device_scalar_counts_take_the_path_of_host_integers(counts):
    buckets = _buckets(len(counts), 11)
    _, host = _run(buckets, counts)
    for as_tensor in [range(len(counts)), (0,), (len(counts) - 1,), (1,)]:
        acc, dev = _run(buckets, counts, as_tensor=tuple(as_tensor))
        assert torch.equal(dev.view(torch.int32), host.view(torch.int32)), as_tensor
        assert acc.count.dtype == torch.int64 and acc.count.dim() == 0 and int(acc.count) == sum(counts)


def test_reset_reuses_the_buffer_and_forgets_the_calls():
    buckets = _buckets(3, 2)
    acc = Accumulation(buckets[0])
    acc.add(buckets[0], 5)
    acc.add(buckets[1], torch.tensor(9))
    ptr = acc.buf.data_ptr()
    acc.reset()
    assert acc.calls == 0
    acc.add(buckets[2], 2)
    out = torch.empty(N)
    acc.write(out, LOSS_SLOT)
    assert torch.equal(out, buckets[2]) and acc.buf.data_ptr() == ptr and int(acc.count) == 2


# ---- 4. two and three ranks over gloo: the oracle computes, BucketExchange is the real one ------------------------------------------
CUTS = {0: ((0, 5), (5, 7)), 1: ((7, 16),), 2: ()}           # rank -> its calls' window ranges: 2, 1 and 0 calls, unequal sizes
N_GLOBAL = {2: 16, 3: 16}


def _oracle_bindings(counter):
    from oracle import windgnn_oracle as orc

    def dims(X, math, Bn=None):
        return _lib.Dims(X.shape[0] if Bn is None else Bn, X.shape[1], X.shape[2], 13, 1, math, _lib.ADJ_DENSE, 0, _lib.IO_F32)

    def _forward_setup(A, X, params, math, labels=None, h0=None, h_n=None, B=None):
        return A, dims(X, math, B), None, 0

    def gcn_gru_forward_raw(A, X, params, math=0, want_stash=True, labels=None, prepared=None):
        p = {k: v.double() for k, v in zip(PARAM_KEYS, params)}
        Y, cache = orc.forward(A.double(), X.double(), p)
        return Y.float(), (p, Y, cache), dims(X, math)

    def gcn_gru_backward_mse_raw(d, A, X, params, Y, L, stash, grads, loss, grad_scale=1.0, part=7, prepared=None):
        assert part == FULL and grad_scale == 1.0
        p, Y64, cache = stash
        value, dY = orc.mse_loss_and_grad(Y64, L.double())
        g = orc.backward(A.double(), X.double(), p, Y64, cache, dY)
        for k, view in zip(PARAM_KEYS, grads):
            view.copy_(g[k])
        loss.copy_(value)

    def finish_step(d, params, grads, which, adam=None, prepared=None, device=None):
        assert which == 0 and adam is not None
        counter["finish"] += 1

    return dict(_forward_setup=_forward_setup, prepared_weights=lambda d, params, device: torch.zeros(1),
                gcn_gru_forward_raw=gcn_gru_forward_raw, gcn_gru_backward_mse_raw=gcn_gru_backward_mse_raw, finish_step=finish_step)


def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    fx = load_fixture("f2_s7_t12_b32_ckpt")
    A, X, L = (torch.from_numpy(fx[k]) for k in ("A", "X", "L"))
    counter = {"finish": 0, "all_reduce": 0}
    for name, fn in _oracle_bindings(counter).items():
        setattr(trainer, name, fn)
    real = dist.all_reduce

    def counted(*a, **kw):
        counter["all_reduce"] += 1
        return real(*a, **kw)
    dist.all_reduce = counted
    Hm = fx["params"]["gru.weight_hh_l0"].shape[1]
    model = windgnn_amd.GCN_GRU(13, 13, 13, X.shape[2] * 13, Hm, math="f32")
    model.load_state_dict({k: v.clone() for k, v in fx["params"].items()})
    tr = TrainStep(model, process_group=dist.group.WORLD)
    for step, n_global in enumerate((None, N_GLOBAL[world])):
        for lo, hi in CUTS[rank]:
            tr.accumulate(A, X[lo:hi], L[lo:hi])
            assert counter["all_reduce"] == (0, 2)[step]                    # accumulate issues no collective, ever
        assert tr.accumulated == len(CUTS[rank])
        loss = tr.apply(n_global)
        assert loss is tr._loss and tr.steps == step + 1 and tr.accumulated == 0
        np.save(os.path.join(out_dir, "acc_%d_rank%d.npy" % (step, rank)), tr._gbuf.numpy())
    # the count collective + the bucket's in the first step, the bucket's alone in the second: the same on every rank
    np.save(os.path.join(out_dir, "calls_rank%d.npy" % rank), np.array([counter["all_reduce"], counter["finish"]]))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_ranks_accumulating_two_one_and_no_calls_end_with_the_big_batch_step(tmp_path, world):
    from oracle import windgnn_oracle as orc
    from test_distributed_cpu import _free_port, _spawn_with_deadline
    _spawn_with_deadline(_worker, (world, _free_port(), str(tmp_path)), world, 120)
    fx = load_fixture("f2_s7_t12_b32_ckpt")
    A, X, L = (torch.from_numpy(fx[k]) for k in ("A", "X", "L"))
    n = N_GLOBAL[world]
    _, loss, g = orc.train_step(A, X[:n], L[:n], fx["params"])
    ref = torch.cat([g[k].reshape(-1) for k in PARAM_KEYS])
    for rank in range(world):
        for step in range(2):
            b = torch.from_numpy(np.load(os.path.join(str(tmp_path), "acc_%d_rank%d.npy" % (step, rank))))
            eg, el = rel_to_max(b[HEADER:], ref), abs(float(b[LOSS_SLOT]) - float(loss))
            print("world %d rank %d step %d: bucket %.2e of its max (bar 2e-5), loss off by %.2e" % (world, rank, step, eg, el))
            assert eg <= 2e-5, (step, rank)                              # tests/test_distributed_cpu.py's bars
            assert el <= 1e-6 * max(1.0, float(loss)), (step, rank)
        assert np.load(os.path.join(str(tmp_path), "calls_rank%d.npy" % rank)).tolist() == [3, 2], rank


# ---- 5. the inputs of tests/test_gpu_accumulate.py's loss-spec cases, checked where no GPU is needed -------------------------------------
def test_every_cut_of_the_l1_draws_keeps_its_residuals_away_from_a_tie():
    """tests/step_loss_cases.py moved its L1 labels more than 1 away from Y so that sign(r) does not hang on the device's
    rounding; Huber's derivative is continuous.  Both are properties of each element, so each call of the cut has them -- and
    each call of the Huber cut reaches both arms."""
    import accumulate_cases as ac
    import step_loss_cases as sl
    c = sl.case("small")
    assert sum(ac.SPEC_CUT) == c.B
    for L in (c.L["l1"], ac.staggered_labels()):
        for lo, hi in ac.spans(ac.SPEC_CUT):
            r = (c.Yo[lo:hi] - L[lo:hi].double())
            assert float(r[~torch.isnan(r)].abs().min()) > 1.0, (lo, hi)
    for lo, hi in ac.spans(ac.SPEC_CUT):
        a = (c.Yo[lo:hi] - c.L["huber"][lo:hi].double()).abs()
        assert bool((a < sl.DELTA).any()) and bool((a > sl.DELTA).any()), (lo, hi)


def test_on_the_staggered_labels_the_window_weighted_answer_misses_the_bar():
    """The calls of the missing-label case count 210, about 190 and about 250 labels on 1, 1 and 2 windows: weighting them by
    their windows is another gradient than the mean over all labels, by far more than the bar the GPU test holds."""
    import accumulate_cases as ac
    import step_loss_cases as sl
    c, q = sl.case("small"), ac.staggered_union()
    L = ac.staggered_labels()
    counts = [int((~torch.isnan(L[lo:hi, 2:])).sum()) for lo, hi in ac.spans(ac.SPEC_CUT)]
    assert sum(counts) == q.m[0] and len({n / (hi - lo) for n, (lo, hi) in zip(counts, ac.spans(ac.SPEC_CUT))}) == 3
    wl, wg = ac.window_weighted(c, L, "l1", 0.0, 2, 1, ac.SPEC_CUT)
    el = abs(wl - q.loss[0]) / q.loss[0]
    eg = {k: rel_to_max(wg[k], q.g[0][k]) for k in PARAM_KEYS}
    print("counts %s; window-weighted against label-weighted: loss %.2e, gradients %s" % (counts, el, eg))
    assert el > 10 * ac.TOL and min(eg.values()) > 10 * ac.TOL
