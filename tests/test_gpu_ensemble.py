"""windgnn_amd.Ensemble on the MI355X: K members on side streams against the same members driven alone on the default stream.

Shapes: S = 7, H = 21, T = 5, a series of 40 rows, 17 windows per member (two recurrence workgroups, the second ragged).  The lone
twins of a configuration run once per module (_lone) and every test compares bit patterns against them: the kernels are
bit-reproducible and a member's launches are the lone TrainStep's, so the only thing that can differ is what the ensemble adds --
the streams, the fork and the join, the hand-back of tensors, the stacked views, the forecast's reduction.
tests/test_ensemble_host.py has the plan on recording streams, the refusals and the arithmetic.

Observed on the MI355X: every comparison bit-identical; one round of K = 3 behind the 70 ms blocker took the host 2.1 ms to
enqueue; mean and std 0 ulp from numpy's fp64 evaluation (bar 1); the module runs in under 4 s."""
import gc
import time

import numpy as np
import pytest
import torch

import stream_cases as sc

pytestmark = pytest.mark.gpu

S, H, T, ROWS, N = 7, 21, 5, 40, 17
LR, EPS = 1e-2, 1e-7
WMIN, WMAX = 3.0, 25.0
# The blocker of test 2.  One round of K = 3 is a step and a validation pass on a table per member; DESIGN.md 2d has their host
# enqueue times alone (py:step_series_table-s7 1.8 ms with its first-use work, py:validate_series_table-s7 0.5 ms), so the round
# takes the host at most 3 * 2.3 = 6.9 ms plus the fork and the join.  stream_cases.blocker_ms of that -- ten times the host
# time, rounded up to 5 ms -- is 70.
BLOCKER_MS = sc.blocker_ms([3 * (1.816 + 0.501)])


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


_DATA = {}


def _data():
    """The shared inputs, built once and never written: the adjacency, the series and its label series, per member a table of 17
    training starts (any order, over rows 0 .. 28) and of 4 to 6 validation starts (rows 30 .. 35), and the materialised
    windows of the same tables' first 4 starts."""
    if not _DATA:
        from windgnn_amd.data import make_windows
        from windgnn_amd.series import series_labels
        dev, g = _dev(), torch.Generator().manual_seed(21)
        feat = torch.rand(ROWS + 3, S, 13, generator=g)
        Ls, _ = series_labels(feat, T, 1, ROWS - T + 1)
        d = dict(A=(torch.rand(S, S, generator=g) / S + 0.01).to(dev), series=feat[:ROWS].contiguous().to(dev), Ls=Ls.contiguous().to(dev))
        assert d["Ls"].shape[0] == ROWS
        d["train"] = [torch.randperm(29, generator=g)[:N].tolist() for _ in range(5)]
        d["val"] = [(30 + torch.randperm(6, generator=g)[:4 + k % 3]).tolist() for k in range(5)]
        d["X"], d["L"], d["Xv"], d["Lv"] = [], [], [], []
        feat = feat.to(dev)
        for k in range(5):
            x, l = make_windows(feat, T, starts=d["train"][k][:4])
            xv, lv = make_windows(feat, T, starts=d["val"][k][:4])
            d["X"].append(x), d["L"].append(l), d["Xv"].append(xv), d["Lv"].append(lv)
        torch.cuda.synchronize()
        _DATA.update(d)
    return _DATA


def _models(K, math):
    from oracle import windgnn_oracle as orc
    from windgnn_amd import GCN_GRU
    out = []
    for k in range(K):
        m = GCN_GRU(13, 13, 13, S * 13, H, math=math, validate=False)
        m.load_state_dict(orc.init_params(S, 13, H, seed=100 + k))
        out.append(m.to(_dev()))
    return out


# configuration -> (K, streams, math, route, the members' keywords: a value or a list of K)
BEST = dict(keep_best=True, best_on="validation")
CONFIGS = {
    "series-k3": (3, 2, "f32", "series", BEST),
    "series-k5": (5, 4, "f32", "series", BEST),
    "windows-k3": (3, 2, "f16x3", "windows", BEST),
    "windows-k5": (5, 4, "f16x3", "windows", BEST),
    "sweep": (3, 2, "f32", "series", dict(lr=[3e-2, 1e-2, 3e-3], max_grad_norm=[None, 1.0, float("inf")])),
}


def _kwargs(cfg, k=None):
    """The keywords of CONFIGS[cfg]: for member k alone, or (k=None) for the ensemble, lists wrapped in PerMember."""
    from windgnn_amd import PerMember
    kw = dict(lr=LR, eps=EPS)
    kw.update(CONFIGS[cfg][4])
    return {n: (v[k] if k is not None else PerMember(v)) if isinstance(v, list) else v for n, v in kw.items()}


def _snap(tr):
    """Everything a member owns that a round writes, as device clones on the current stream."""
    out = {"p": tr.flat_p, "m": tr.exp_avg, "v": tr.exp_avg_sq, "loss": tr._loss}
    if tr._val is not None:
        out.update(val_loss=tr.val_loss, val_stale=tr.val_stale, val_count=tr.val_count)
    if tr._best_p is not None:
        out.update(best_p=tr._best_p, best_loss=tr.best_loss, best_step=tr.best_step)
    if tr._clip is not None:
        out.update(grad_norm=tr.grad_norm, clip_coef=tr.clip_coef)
    return {n: t.detach().clone() for n, t in out.items()}


def _bytes(t):
    return t.detach().reshape(-1).contiguous().view(torch.uint8).cpu()


def _same(ref, got, tag):
    assert set(ref) == set(got), (tag, sorted(ref), sorted(got))
    for n in ref:
        assert ref[n].dtype == got[n].dtype and torch.equal(_bytes(ref[n]), _bytes(got[n])), \
            "%s: %s differs from the member driven alone (%s against %s)" % (tag, n, got[n].flatten()[:4].tolist(),
                                                                           ref[n].flatten()[:4].tolist())


def _lone_round(cfg, tr, k):
    d, route = _data(), CONFIGS[cfg][3]
    if route == "series":
        loss, Y = tr.step_series(d["A"], d["series"], d["Ls"], T, starts=d["train"][k])
        if "keep_best" in CONFIGS[cfg][4]:
            tr.validate_series(d["A"], d["series"], d["Ls"], T, starts=d["val"][k])
    else:
        loss, Y = tr.step(d["A"], d["X"][k], d["L"][k])
        tr.validate(d["A"], d["Xv"][k], d["Lv"][k])
    return Y


def _ens_round(cfg, ens, d=None):
    from windgnn_amd import PerMember
    d, route, K = d or _data(), CONFIGS[cfg][3], CONFIGS[cfg][0]
    if route == "series":
        out = ens.step_series(d["A"], d["series"], d["Ls"], T, starts=PerMember(d["train"][:K]))
        if "keep_best" in CONFIGS[cfg][4]:
            ens.validate_series(d["A"], d["series"], d["Ls"], T, starts=PerMember(d["val"][:K]))
    else:
        out = ens.step(d["A"], PerMember(d["X"][:K]), PerMember(d["L"][:K]))
        ens.validate(d["A"], PerMember(d["Xv"][:K]), PerMember(d["Lv"][:K]))
    return [Y for _, Y in out]


_LONE = {}


def _lone(cfg):
    """[round][k] -> (snapshot, Y) of member k driven alone on the default stream for three rounds; computed once."""
    if cfg not in _LONE:
        from windgnn_amd.trainer import TrainStep
        K, _, math, _, _ = CONFIGS[cfg]
        assert torch.cuda.current_stream().cuda_stream == 0
        trs = [TrainStep(m, **_kwargs(cfg, k)) for k, m in enumerate(_models(K, math))]
        rounds = []
        for _ in range(3):
            ys = [_lone_round(cfg, tr, k).clone() for k, tr in enumerate(trs)]
            rounds.append([(_snap(tr), y) for tr, y in zip(trs, ys)])
        torch.cuda.synchronize()
        _LONE[cfg] = rounds
    return _LONE[cfg]


def _ensemble(cfg, **kw):
    from windgnn_amd import Ensemble
    K, streams, math, _, _ = CONFIGS[cfg]
    return Ensemble(_models(K, math), streams=streams, **dict(_kwargs(cfg), **kw))


# ---- 1. bit-identity under concurrency ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cfg", ["series-k3", "series-k5", "windows-k3", "windows-k5"])
def test_members_in_flight_together_are_the_members_driven_alone_bit_for_bit(cfg):
    ref = _lone(cfg)
    ens = _ensemble(cfg)
    K = CONFIGS[cfg][0]
    for r in range(3):
        ys = _ens_round(cfg, ens)
        views = {n: getattr(ens, n).clone() for n in ("loss", "val_loss", "val_stale", "val_count", "best_loss", "best_step", "steps")}
        for k, tr in enumerate(ens.members):
            _same(ref[r][k][0], _snap(tr), "%s round %d member %d" % (cfg, r + 1, k))
            assert torch.equal(_bytes(ys[k]), _bytes(ref[r][k][1])), (cfg, r, k, "Y")
        for n, v in views.items():                      # the [K] views are the members' words, stacked
            assert tuple(v.shape) == (K,), (n, v.shape)
            if n != "steps":
                assert torch.equal(_bytes(v), torch.cat([_bytes(ref[r][k][0][n]) for k in range(K)])), (cfg, r, n)
        assert views["steps"].tolist() == [r + 1] * K and views["steps"].dtype == torch.int64
    assert int(ens.members[0].best_step) >= 1                               # a validation pass did decide
    stale = [int(ref[2][k][0]["val_stale"]) for k in range(K)]
    print("%s: losses %s, val_stale %s" % (cfg, [round(float(ref[2][k][0]["loss"]), 6) for k in range(K)], stale))
    ens.check()


# ---- 2. the stream contract of the fan-out -----------------------------------------------------------------------------------------
_RATE = []


def _cycles(ms):
    """torch.cuda._sleep cycles of `ms`, calibrated once with events (two lengths: the slope), as tests/test_gpu_streams.py."""
    if not _RATE:
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        took = []
        for cyc in (2_000_000, 20_000_000):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(cyc)
            e1.record()
            torch.cuda.synchronize()
            took.append(e0.elapsed_time(e1))
        _RATE.append(sc.cycles_per_ms(2_000_000, took[0], 20_000_000, took[1]))
    return sc.sleep_cycles(ms, _RATE[0])


def test_a_fan_out_from_a_side_stream_behind_a_blocker_with_late_inputs():
    """Rounds 1 and 2 from a non-default stream (first-use allocations behind us), then every floating-point input is NaN until
    a copy on that stream, behind a blocker, produces it; round 3 follows, its results are cloned on the same stream, and when
    the host comes back the blocker has not ended: nothing waited.  The results are those of the lone members; every C call of
    member k carried side[k % streams]'s handle."""
    from windgnn_amd import _lib as L
    cfg = "series-k3"
    ref, src = _lone(cfg), _data()
    caller = torch.cuda.Stream()
    cycles = _cycles(BLOCKER_MS)
    late = dict(src, **{n: src[n].clone() for n in ("A", "series", "Ls")})
    with torch.cuda.stream(caller):
        ens = _ensemble(cfg)
        for r in range(2):
            _ens_round(cfg, ens, late)
    torch.cuda.synchronize()
    for k, tr in enumerate(ens.members):
        _same(ref[1][k][0], _snap(tr), "round 2 from a side stream, member %d" % k)
    # whose C call: the members' methods note the span of recorded calls each of their calls made
    real = L.load()
    rec = sc.RecordingLib(real, sc.stream_prototypes())
    spans = []

    def marked(k, fn):
        def call(*a, **kw):
            i0 = len(rec.calls)
            try:
                return fn(*a, **kw)
            finally:
                spans.append((k, i0, len(rec.calls)))
        return call
    for k, tr in enumerate(ens.members):
        tr.step_series, tr.validate_series = marked(k, tr.step_series), marked(k, tr.validate_series)
    for n in ("A", "series", "Ls"):
        late[n].fill_(float("nan"))
    torch.cuda.synchronize()
    L._lib = rec
    try:
        with torch.cuda.stream(caller):
            torch.cuda._sleep(cycles)
            e_block = torch.cuda.Event()
            e_block.record(caller)
            gc.disable()
            t0 = time.perf_counter()
            for n in ("A", "series", "Ls"):
                late[n].copy_(src[n], non_blocking=True)
            ys = _ens_round(cfg, ens, late)
            got = [_snap(tr) for tr in ens.members]                         # consumed on the caller's stream, unsynchronised
            ys = [y.clone() for y in ys]
            views = {n: getattr(ens, n).clone() for n in ("loss", "val_loss", "val_stale")}
            host_ms = (time.perf_counter() - t0) * 1e3
            early = e_block.query()
            gc.enable()
        torch.cuda.synchronize()
    finally:
        L._lib = real
        gc.enable()
    print("one round of K = 3 behind a blocker of %d ms: host enqueue %.3f ms" % (BLOCKER_MS, host_ms))
    assert early is False, ("the blocker (%d ms) had already ended when the host came back from the round, %.2f ms after its "
                            "first call: some call waited for a stream" % (BLOCKER_MS, host_ms))
    for k in range(3):
        _same(ref[2][k][0], got[k], "round 3 behind the blocker, member %d" % k)
        assert torch.equal(_bytes(ys[k]), _bytes(ref[2][k][1]))
    for n, v in views.items():
        assert torch.equal(_bytes(v), torch.cat([_bytes(ref[2][k][0][n]) for k in range(3)])), n
    assert len(spans) == 6 and rec.calls
    covered = 0
    for k, i0, i1 in spans:
        want = ens.stream_of(k).cuda_stream
        assert want != 0 and want != caller.cuda_stream and i1 > i0
        assert {h for _, h in rec.calls[i0:i1]} == {want}, (k, rec.calls[i0:i1], want)
        covered += i1 - i0
    assert covered == len(rec.calls) and all(h != 0 for _, h in rec.calls)  # nothing ran outside a member's call, none on NULL
    assert len({ens.stream_of(k).cuda_stream for k in range(3)}) == 2


# ---- 3. the forecast ---------------------------------------------------------------------------------------------------------------
def _ulps(a, b):
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    return int(np.abs(ia - ib).max())


@pytest.mark.parametrize("use_best", [False, True])
def test_the_forecast_holds_each_members_own_rows_and_their_fp64_mean_and_spread(use_best):
    from windgnn_amd import GCN_GRU
    from windgnn_amd.data import forward_last, make_windows
    from windgnn_amd.series import forward_last_series
    cfg, d = "series-k3", _data()
    ens = _ensemble(cfg)
    for r in range(3):
        _ens_round(cfg, ens)
    ens.step_series(d["A"], d["series"], d["Ls"], T, stride=2)               # (past the last pass: the snapshot is not the current model)
    table = [31, 0, 17, 35, 8, 8, 22] + list(range(10, 20))                  # 17 windows, any order, a duplicate
    fc = ens.forward_last_series(d["A"], d["series"], T, WMIN, WMAX, starts=table, use_best=use_best)
    fs = ens.forward_last_series(d["A"], d["series"], T, WMIN, WMAX, stride=2, use_best=use_best)
    Xw = d["X"][0]
    fm = ens.forward_last(d["A"], Xw, WMIN, WMAX, use_best=use_best)
    torch.cuda.synchronize()
    assert tuple(fc.members.shape) == (3, 17, H) and tuple(fc.mean.shape) == (17, H) == tuple(fc.std.shape)
    assert tuple(fs.members.shape) == (3, 18, H) and tuple(fm.members.shape) == (3, 4, H)
    for k, tr in enumerate(ens.members):
        model = tr.model
        if use_best:
            model = GCN_GRU(13, 13, 13, S * 13, H, math="f32", validate=False)
            model.load_state_dict(tr.best_state_dict())
            model = model.to(_dev())
            assert not torch.equal(tr._best_p, tr.flat_p)                    # (the snapshot is not the current parameters)
        assert torch.equal(_bytes(fc.members[k]), _bytes(forward_last_series(model, d["A"], d["series"], T, WMIN, WMAX, starts=table)))
        assert torch.equal(_bytes(fs.members[k]), _bytes(forward_last_series(model, d["A"], d["series"], T, WMIN, WMAX, stride=2)))
        assert torch.equal(_bytes(fm.members[k]), _bytes(forward_last(model, d["A"], Xw, WMIN, WMAX)))
    for f in (fc, fs, fm):
        x = f.members.cpu().numpy().astype(np.float64)
        want_mean = x.mean(axis=0).astype(np.float32)
        want_std = np.sqrt(((x - x.mean(axis=0)) ** 2).mean(axis=0)).astype(np.float32)
        um, us = _ulps(f.mean.cpu().numpy(), want_mean), _ulps(f.std.cpu().numpy(), want_std)
        print("use_best=%s: mean off by %d ulp, std by %d ulp (bar 1); spread up to %.3f m/s around %.2f"
              % (use_best, um, us, float(f.std.max()), float(f.mean.mean())))
        assert um <= 1 and us <= 1 and float(f.std.min()) > 0.0


# ---- 4. a sweep --------------------------------------------------------------------------------------------------------------------
def test_a_sweep_over_lr_and_max_grad_norm_gives_each_member_its_lone_twin():
    cfg = "sweep"
    ref = _lone(cfg)
    ens = _ensemble(cfg)
    assert [tr.lr for tr in ens.members] == CONFIGS[cfg][4]["lr"]
    assert [tr.max_grad_norm for tr in ens.members] == [None, 1.0, float("inf")]
    for r in range(3):
        _ens_round(cfg, ens)
        gn = ens.grad_norm.clone()
        for k, tr in enumerate(ens.members):
            _same(ref[r][k][0], _snap(tr), "sweep round %d member %d" % (r + 1, k))
        assert tuple(gn.shape) == (3,) and gn.dtype == torch.float32
        assert bool(torch.isnan(gn[0]))                                     # max_grad_norm=None measures nothing: NaN
        for k in (1, 2):                                                    # clipped at 1.0; float("inf"): measured, unclipped
            assert torch.equal(_bytes(gn[k]), _bytes(ref[r][k][0]["grad_norm"])), (r, k)
    assert float(ref[2][2][0]["clip_coef"]) == 1.0 and float(ref[2][1][0]["grad_norm"]) > 0.0
    p = [ref[2][k][0]["p"] for k in range(3)]
    assert not torch.equal(p[0], p[1]) and not torch.equal(p[1], p[2])


# ---- 5. checkpoints ----------------------------------------------------------------------------------------------------------------
def test_a_checkpoint_after_two_rounds_resumes_bit_for_bit():
    cfg = "series-k3"
    ref = _lone(cfg)
    ens = _ensemble(cfg)
    for r in range(2):
        _ens_round(cfg, ens)
    sd = ens.state_dict()
    params = [{n: v.clone() for n, v in tr.model.state_dict().items()} for tr in ens.members]
    assert sd["K"] == 3 and len(sd["members"]) == 3 and "val" in sd["members"][0]
    del ens
    fresh = _ensemble(cfg)
    for tr, p in zip(fresh.members, params):
        tr.model.load_state_dict(p)
    fresh.load_state_dict(sd)
    ys = _ens_round(cfg, fresh)
    for k, tr in enumerate(fresh.members):
        _same(ref[2][k][0], _snap(tr), "round 3 after a checkpoint, member %d" % k)
        assert torch.equal(_bytes(ys[k]), _bytes(ref[2][k][1]))
    from windgnn_amd import Ensemble
    with pytest.raises(RuntimeError, match="K = 3 members, this ensemble 2"):
        Ensemble(_models(2, "f32"), **BEST).load_state_dict(sd)


# ---- 6. each -----------------------------------------------------------------------------------------------------------------------
def test_each_runs_an_accumulation_per_member():
    from windgnn_amd import Ensemble
    from windgnn_amd.trainer import TrainStep
    d, K = _data(), 3
    cuts = [(d["train"][k][:9], d["train"][k][9:]) for k in range(K)]
    lone = [TrainStep(m, lr=LR, eps=EPS) for m in _models(K, "f32")]
    ens = Ensemble(_models(K, "f32"), streams=2, lr=LR, eps=EPS)
    for r in range(2):
        want = []
        for k, tr in enumerate(lone):
            for part in cuts[k]:
                tr.accumulate_series(d["A"], d["series"], d["Ls"], T, starts=part)
            want.append(tr.apply().clone())
        for i in range(2):
            out = ens.each(lambda k, tr: tr.accumulate_series(d["A"], d["series"], d["Ls"], T, starts=cuts[k][i]))
            assert len(out) == K and [tuple(Y.shape) for _, Y in out] == [(len(cuts[k][i]), T, H) for k in range(K)]
        losses = ens.each(lambda k, tr: tr.apply())
        for k in range(K):
            _same(_snap(lone[k]), _snap(ens.members[k]), "accumulated round %d member %d" % (r + 1, k))
            assert torch.equal(_bytes(losses[k]), _bytes(want[k]))
    assert ens.steps.tolist() == [2] * K
