"""windgnn_amd.ensemble without a GPU: PerMember resolution and the refusals, the fork / join plan of a fan-out on recording
stand-ins for streams and events (the members on the recorders of tests/test_trainstep_schedule_host.py), series.kfold_starts
against brute force, the mean / std arithmetic on CPU tensors against numpy fp64, and the layout of the state dict."""
import numpy as np
import pytest
import torch

import test_trainstep_schedule_host as sh
import windgnn_amd
from windgnn_amd import Ensemble, PerMember, ensemble, trainer
from windgnn_amd.series import kfold_starts

S, T, B, H = sh.S, sh.T, sh.B, 21


# ---- stand-ins ------------------------------------------------------------------------------------------------------------------
class FakeStream:
    def __init__(self, log, name):
        self.log, self.name, self.cuda_stream = log, name, hash(name)

    def wait_event(self, e):
        self.log.append(("wait", self.name, e.n))


class FakeEvent:
    def __init__(self, log, n):
        self.log, self.n = log, n

    def record(self, stream):
        self.log.append(("record", self.n, stream.name))


class FakeCuda:
    """ensemble._cuda, recording: log = fork / join events and, through `rec`, every recorded call with the stream it ran under."""

    def __init__(self):
        self.log, self.made, self.events = [], 0, 0
        self.caller = self.active = FakeStream(self.log, "caller")

    def new_stream(self, device):
        self.made += 1
        return FakeStream(self.log, "side%d" % (self.made - 1))

    def current_stream(self, device):
        return self.active

    def event(self):
        self.events += 1
        return FakeEvent(self.log, self.events - 1)

    def set_stream(self, stream):
        self.active = stream

    def hand_back(self, t, stream):
        self.log.append(("hand_back", stream.name))


def _ens(monkeypatch, K, streams=None, math="f32", **kw):
    """K CPU-constructed members on the recorders; member k stands at steps = 100 k + 41, so the optimiser's step number in a
    recorded event says whose call it was."""
    fake = FakeCuda()
    monkeypatch.setattr(ensemble, "_cuda", fake)
    rec = sh.Recorder()
    for name, fn in sh._bindings(lambda *e: (rec(*e), fake.log.append(("call", fake.active.name) + e)), H).items():
        monkeypatch.setattr(trainer, name, fn)
    models = [windgnn_amd.GCN_GRU(13, 13, 13, S * 13, H, math=math) for _ in range(K)]
    ens = Ensemble(models, streams=streams, **kw)
    for k, tr in enumerate(ens.members):
        tr.steps = 100 * k + 41
    del fake.log[:]
    return ens, fake


def _windows(n=B):
    return torch.rand(S, S), torch.rand(n, T, S, 13), torch.rand(n, T, H)


# ---- 1. PerMember and the refusals ---------------------------------------------------------------------------------------------
def test_a_per_member_keyword_reaches_each_member_and_a_scalar_all_of_them(monkeypatch):
    ens, _ = _ens(monkeypatch, 3, lr=PerMember([1e-2, 1e-3, 1e-4]), max_grad_norm=PerMember([None, 1.0, float("inf")]), eps=1e-7)
    assert [tr.lr for tr in ens.members] == [1e-2, 1e-3, 1e-4]
    assert [tr.max_grad_norm for tr in ens.members] == [None, 1.0, float("inf")]
    assert [tr.eps for tr in ens.members] == [1e-7] * 3
    assert ens.K == 3 and ens.n_streams == 3 and len(ens.side) == 3
    assert all(tr.check_every == 0 for tr in ens.members) and ens.check_every == 100
    assert _ens(monkeypatch, 6)[0].n_streams == 4 and _ens(monkeypatch, 6, streams=7)[0].n_streams == 7


def test_a_per_member_argument_is_handed_out_member_by_member(monkeypatch):
    ens, fake = _ens(monkeypatch, 3, streams=2)
    A = torch.rand(S, S)
    batches = [_windows(n)[1:] for n in (1, 2, 3)]
    out = ens.step(A, PerMember([x for x, _ in batches]), PerMember([l for _, l in batches]))
    assert [tuple(Y.shape) for _, Y in out] == [(1, T, H), (2, T, H), (3, T, H)]
    assert [loss is tr._loss for (loss, _), tr in zip(out, ens.members)] == [True] * 3
    seen = []
    assert ens.each(lambda k, tr: seen.append((k, tr is ens.members[k], fake.active.name)) or k) == [0, 1, 2]
    assert seen == [(0, True, "side0"), (1, True, "side1"), (2, True, "side0")]


@pytest.mark.parametrize("name", ["process_group", "direct_rccl", "overlap_collectives", "grad_blocks"])
def test_collectives_are_refused_at_construction_by_name(monkeypatch, name):
    with pytest.raises(RuntimeError, match="Ensemble\\(%s=.*collectives issued from several streams are a follow-up" % name):
        _ens(monkeypatch, 2, **{name: None})


def test_the_other_refusals_at_construction_name_their_argument(monkeypatch):
    with pytest.raises(ValueError, match="lr=PerMember\\(...\\) holds 2 entries for 3 members"):
        _ens(monkeypatch, 3, lr=PerMember([1e-3, 1e-4]))
    for bad in (0, -1, 1.5):
        with pytest.raises(ValueError, match="streams=%r.*at least one side stream" % (bad,)):
            _ens(monkeypatch, 3, streams=bad)
    with pytest.raises(ValueError, match="check_every=PerMember"):
        _ens(monkeypatch, 2, check_every=PerMember([1, 2]))
    with pytest.raises(ValueError, match="at least one model"):
        _ens(monkeypatch, 0)
    fake = FakeCuda()
    monkeypatch.setattr(ensemble, "_cuda", fake)
    a, b = (windgnn_amd.GCN_GRU(13, 13, 13, S * 13, H) for _ in range(2))
    b.to("meta")
    with pytest.raises(RuntimeError, match="members must be on one device.*models\\[0\\] on cpu.*models\\[1\\] on meta"):
        Ensemble([a, b])
    assert fake.made == 0                                              # refused before a stream was made
    with pytest.raises(TypeError, match="models\\[1\\] is Linear"):
        Ensemble([a, torch.nn.Linear(2, 2)])


def test_a_per_member_of_another_length_is_refused_before_any_call(monkeypatch):
    ens, fake = _ens(monkeypatch, 3, streams=2)
    A, X, L = _windows()
    with pytest.raises(ValueError, match="Ensemble.step: X=PerMember\\(...\\) holds 2 entries for 3 members"):
        ens.step(A, PerMember([X, X]), L)
    with pytest.raises(ValueError, match="Ensemble.step_series: starts=PerMember\\(...\\) holds 4 entries for 3 members"):
        ens.step_series(A, torch.rand(14, S, 13), torch.rand(14, H), T, starts=PerMember([[0]] * 4))
    with pytest.raises(ValueError, match="Ensemble.validate_series: loss=PerMember"):
        ens.validate_series(A, torch.rand(14, S, 13), torch.rand(14, H), T, loss=PerMember(["l1"]))
    with pytest.raises(ValueError, match="Ensemble.forward_last_series: starts=PerMember"):
        ens.forward_last_series(A, torch.rand(14, S, 13), T, 0.0, 1.0, starts=PerMember([[0]]))
    assert fake.log == [] and [tr.steps for tr in ens.members] == [41, 141, 241]


# ---- 2. the fork / join plan ---------------------------------------------------------------------------------------------------
def _plan(fake, K, streams):
    """The log of one fan-out, split and checked: the fork, member k's calls whole and in order under side[k % streams], one
    join per used stream; returns the members' call lists."""
    log, used = fake.log, min(K, streams)
    fork = log[:1 + used]
    assert fork == [("record", fork[0][1], "caller")] + [("wait", "side%d" % s, fork[0][1]) for s in range(used)]
    calls = [e for e in log if e[0] == "call"]
    first, last = log.index(calls[0]), len(log) - 1 - log[::-1].index(calls[-1])
    assert first == len(fork) and log[first:last + 1] == calls              # nothing between the members' calls
    join = [e for e in log[last + 1:] if e[0] != "hand_back"]
    assert len(join) == 2 * used
    for s in range(used):                                                   # one join per used stream, after the last call
        rec_e, wait_e = join[2 * s], join[2 * s + 1]
        assert rec_e == ("record", rec_e[1], "side%d" % s) and wait_e == ("wait", "caller", rec_e[1]) and rec_e[1] != fork[0][1]
    assert all(e == ("hand_back", "caller") for e in log[last + 1 + len(join):])
    # whose call: every member's step ends with ("finish", 6, 100 k + 42); the calls up to it are that member's
    per, cur = [], []
    for e in calls:
        cur.append(e)
        if e[2] == "finish":
            per.append(cur)
            cur = []
    assert cur == [] and len(per) == K
    for k, mine in enumerate(per):
        assert mine[-1][2:] == ("finish", 6, 100 * k + 42), (k, mine[-1])    # issued in order k = 0 .. K - 1
        assert {e[1] for e in mine} == {"side%d" % (k % streams)}, (k, mine)  # the whole call under its own stream
    return per


@pytest.mark.parametrize("K,streams", [(3, 2), (5, 4), (2, 4), (3, 1)])
def test_a_step_forks_issues_the_members_whole_and_in_order_and_joins(monkeypatch, K, streams):
    ens, fake = _ens(monkeypatch, K, streams=streams)
    A, X, L = _windows()
    out = ens.step(A, X, L)
    per = _plan(fake, K, streams)
    want = sh.ROWS["plain"][1]
    for k, mine in enumerate(per):
        assert [e[2:] for e in mine][:-1] == want[:-1]                        # TrainStep's own schedule, launch for launch
    assert [tr.steps for tr in ens.members] == [100 * k + 42 for k in range(K)] and len(out) == K
    assert fake.log.count(("hand_back", "caller")) == 2 * K                   # loss and Y of every member


def test_a_series_step_follows_the_same_plan(monkeypatch):
    ens, fake = _ens(monkeypatch, 3, streams=2)
    ens.step_series(torch.rand(S, S), torch.rand(14, S, 13), torch.rand(14, H), T, stride=3, n_windows=4)
    calls = [e for e in fake.log if e[0] == "call"]
    assert [e[1] for e in calls if e[2] == "series_forward_loss"] == ["side0", "side1", "side0"]
    assert [e[2:] for e in calls if e[2] == "finish"] == [("finish", 0, 42), ("finish", 0, 142), ("finish", 0, 242)]
    assert fake.log[0][0] == "record" and [e for e in fake.log if e[0] == "wait" and e[1] == "caller"].__len__() == 2


def test_a_member_that_raises_still_leaves_the_streams_joined(monkeypatch):
    ens, fake = _ens(monkeypatch, 3, streams=2)

    def fn(k, tr):
        if k == 1:
            raise sh.Boom(k)
    with pytest.raises(sh.Boom):
        ens.each(fn)
    assert [e for e in fake.log if e[0] == "wait" and e[1] == "caller"].__len__() == 2 and fake.active is fake.caller


def test_the_range_check_runs_from_the_ensemble_after_the_join(monkeypatch):
    ens, fake = _ens(monkeypatch, 3, streams=2, math="f16x3", check_every=1)
    monkeypatch.setattr(ensemble._F, "check_range_status", lambda device=None: fake.log.append(("ensemble_check", fake.active.name)))
    A, X, L = _windows()
    ens.step(A, X, L)
    assert not [e for e in fake.log if e[0] == "call" and e[2] == "check"]    # no member checked inside its call
    assert fake.log[-1] == ("ensemble_check", "caller")
    last_join = max(i for i, e in enumerate(fake.log) if e[0] == "wait" and e[1] == "caller")
    assert fake.log.index(("ensemble_check", "caller")) > last_join
    n = len(fake.log)
    ens.each(lambda k, tr: None)                                              # (a call that takes no step does not check)
    assert ("ensemble_check", "caller") not in fake.log[n:]
    f32, fake32 = _ens(monkeypatch, 2, check_every=1)
    f32.step(A, X, L)
    assert not [e for e in fake32.log if e[0] == "ensemble_check"]            # exact fp32 reports nothing, as in TrainStep


def test_a_report_names_the_members_of_the_stream_that_reported(monkeypatch):
    ens, fake = _ens(monkeypatch, 5, streams=2)
    ens.device = torch.device("cpu")
    bufs = {(None, ens.side[1].cuda_stream): torch.zeros(256, dtype=torch.uint8)}
    bufs[(None, ens.side[1].cuda_stream)][:4].view(torch.int32)[0] = 4
    monkeypatch.setattr(ensemble._F._Workspace, "_bufs", bufs)
    with pytest.raises(RuntimeError, match="members 1, 3 \\(side stream 1 of 2\\) reported status 4: a gradient came out inf / NaN"):
        ens.check()
    assert int(bufs[(None, ens.side[1].cuda_stream)][:4].view(torch.int32)[0]) == 0
    assert ens.members_of(0) == [0, 2, 4] and ens.stream_of(3) is ens.side[1]


# ---- 3. kfold_starts against brute force ---------------------------------------------------------------------------------------
def _table():
    """Starts of every window of 5 rows + 3 label rows inside the clean stretches of a series with two outages."""
    from windgnn_amd.series import segment_starts
    return segment_starts([(0, 40), (47, 31), (90, 52)], 5, 1, 3)


@pytest.mark.parametrize("k", [2, 3, 5, 7])
@pytest.mark.parametrize("seq_len,horizon", [(5, 3), (1, 0), (9, 3)])
def test_kfold_starts_is_blocked_in_time_and_purged(k, seq_len, horizon):
    table = _table()
    folds = kfold_starts(table[::-1], k, seq_len, horizon)                    # (any order in: the table is sorted first)
    assert len(folds) == k
    assert sorted(np.concatenate([val for _, val in folds]).tolist()) == table        # every start in exactly one validation fold
    sizes = [len(val) for _, val in folds]
    assert max(sizes) - min(sizes) <= 1
    prev_hi = -1
    for train, val in folds:
        assert train.dtype == np.int64 and val.dtype == np.int64
        assert val.tolist() == sorted(val.tolist()) and val[0] > prev_hi              # contiguous in time, in order
        prev_hi = val[-1]
        span = seq_len + horizon
        val_rows = set(r for v in val.tolist() for r in range(v, v + span))
        kept, purged = [], []
        for s in table:
            if s in set(val.tolist()):
                continue
            (purged if val_rows & set(range(s, s + span)) else kept).append(s)
        assert train.tolist() == kept                                                 # brute force: no shared row, nothing else dropped
        assert sorted(kept + purged + val.tolist()) == table
        if seq_len > 1:
            assert purged                                                             # (the windows next to the block's ends)


def test_kfold_starts_refusals():
    table = _table()
    for k in (1, 0):
        with pytest.raises(ValueError, match="k=%d: at least two folds" % k):
            kfold_starts(table, k, 5)
    with pytest.raises(ValueError, match="k=%d folds of a table of %d starts" % (len(table) + 1, len(table))):
        kfold_starts(table, len(table) + 1, 5)
    with pytest.raises(ValueError, match="1-D sequence of integers"):
        kfold_starts([0.5, 1.5], 2, 5)
    with pytest.raises(ValueError, match="seq_len must be >= 1 and horizon >= 0"):
        kfold_starts(table, 2, 0)
    folds = kfold_starts(table, len(table), 5)                                        # k = len(starts): one window per fold
    assert [len(v) for _, v in folds] == [1] * len(table)


def test_a_duplicate_of_a_validation_start_does_not_train():
    folds = kfold_starts([0, 10, 10, 30], 2, 2, 0)
    assert folds[0][1].tolist() == [0, 10] and folds[0][0].tolist() == [30]
    assert folds[1][1].tolist() == [10, 30] and folds[1][0].tolist() == [0]


# ---- 4. mean and std -----------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    """Distance in fp32 ulps between two fp32 arrays of non-negative or same-signed finite values (bit patterns)."""
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return int(np.abs(ia - ib).max())


@pytest.mark.parametrize("K", [2, 3, 5])
def test_mean_and_std_are_fp64_evaluations_rounded_once(K):
    g = torch.Generator().manual_seed(40 + K)
    base = torch.rand(1, 17, 21, generator=g) * 20 + 1
    members = (base + torch.randn(K, 17, 21, generator=g) * 10.0 ** torch.randint(-6, 1, (1, 17, 21), generator=g).float()).float()
    mean, std = ensemble.mean_std(members)
    assert mean.dtype == torch.float32 and std.dtype == torch.float32 and tuple(mean.shape) == (17, 21) == tuple(std.shape)
    x = members.numpy().astype(np.float64)
    want_mean = x.mean(axis=0).astype(np.float32)
    want_std = np.sqrt(((x - x.mean(axis=0)) ** 2).mean(axis=0)).astype(np.float32)
    um, us = _ulps(mean.numpy(), want_mean), _ulps(std.numpy(), want_std)
    print("K = %d: mean off by %d ulp, std by %d ulp (bar 1: both are fp64 evaluations rounded once)" % (K, um, us))
    assert um <= 1 and us <= 1


def test_one_member_is_its_own_mean_with_a_spread_of_exactly_zero():
    members = torch.randn(1, 9, 21) * 30
    mean, std = ensemble.mean_std(members)
    assert torch.equal(mean, members[0]) and torch.equal(std, torch.zeros(9, 21)) and not torch.signbit(std).any()


def test_the_chunks_follow_the_64_mib_rule_and_do_not_change_the_result(monkeypatch):
    members = torch.randn(3, 50, 21)
    whole = ensemble.mean_std(members)
    seen, validation_chunk_windows = [], ensemble._F.validation_chunk_windows

    def chunk(n, K, C, cap=None):
        seen.append((n, K, C))
        return 7
    monkeypatch.setattr(ensemble._F, "validation_chunk_windows", chunk)
    cut = ensemble.mean_std(members)
    assert seen == [(50, 3, 21)] and torch.equal(cut[0], whole[0]) and torch.equal(cut[1], whole[1])
    rows =validation_chunk_windows(4096 * 64, 4, 3 * 34 * 64)                 # a configs[4]-sized output: far from one temporary
    assert rows * 4 * 3 * 34 * 64 * 8 <= 64 << 20 < (rows + 1) * 4 * 3 * 34 * 64 * 8
    with pytest.raises(ValueError, match="members \\[K >= 1, n, C\\]"):
        ensemble.mean_std(torch.zeros(3, 4))


# ---- 5. the state dict -----------------------------------------------------------------------------------------------------------
def test_the_state_dict_is_the_members_dicts_plus_k_and_another_k_is_refused(monkeypatch):
    ens, _ = _ens(monkeypatch, 3, streams=2, lr=PerMember([1e-2, 1e-3, 1e-4]))
    for k, tr in enumerate(ens.members):
        tr.exp_avg.fill_(k + 1.0)
    sd = ens.state_dict()
    assert sorted(sd) == ["K", "members"] and sd["K"] == 3 and len(sd["members"]) == 3
    assert [sorted(m) for m in sd["members"]] == [["best", "carry", "optimizer", "steps"]] * 3
    assert [m["steps"] for m in sd["members"]] == [41, 141, 241]
    other, _ = _ens(monkeypatch, 3, streams=1)
    other.load_state_dict(sd)
    assert [tr.steps for tr in other.members] == [41, 141, 241] and [tr.lr for tr in other.members] == [1e-2, 1e-3, 1e-4]
    assert [float(tr.exp_avg[0]) for tr in other.members] == [1.0, 2.0, 3.0]
    two, _ = _ens(monkeypatch, 2)
    with pytest.raises(RuntimeError, match="the checkpoint holds K = 3 members, this ensemble 2"):
        two.load_state_dict(sd)
    assert [tr.steps for tr in two.members] == [41, 141]
    with pytest.raises(ValueError, match="'K': K, 'members'"):
        other.load_state_dict({"K": 3, "members": sd["members"][:2]})


def test_the_views_are_k_vectors_stacked_without_a_host_read(monkeypatch):
    ens, _ = _ens(monkeypatch, 3, streams=2, max_grad_norm=PerMember([None, 1.0, float("inf")]))
    for k, tr in enumerate(ens.members):
        tr._gbuf[trainer.LOSS_SLOT] = k + 0.5
        if tr.max_grad_norm is not None:
            tr._clip = torch.full((16,), 10.0 * k)
    assert ens.loss.tolist() == [0.5, 1.5, 2.5] and ens.loss.data_ptr() != ens.members[0]._loss.data_ptr()
    assert ens.steps.tolist() == [41, 141, 241] and ens.steps.dtype == torch.int64
    gn = ens.grad_norm
    assert tuple(gn.shape) == (3,) and gn[0] != gn[0] and gn[1:].tolist() == [10.0, 20.0]
    plain, _ = _ens(monkeypatch, 2)
    with pytest.raises(RuntimeError, match="max_grad_norm=None"):
        plain.grad_norm
    with pytest.raises(RuntimeError, match="no validation call has run"):
        plain.val_loss
