"""Frozen parameter groups on the MI355X: TrainStep(trainable="gru" | "conv") / set_trainable against the step on all eight tensors
(bit for bit: include/windgnn.h says the fused and the split forms of the backward and of wgnn_finish give identical results) and
against the fp64 oracle with Adam on the trained tensors only, each group at its own step number.  Inputs are
tests/lattice_inputs.py's draw (live ReLU masks, non-zero conv biases, an asymmetric A); Adam runs at lr 1e-3 and
tests/step_loss_cases.py's eps on both sides, the bar is the project's 1e-4 of the tensor's max.  tests/test_trainable_host.py has the
call sequences, the refusals and the checkpoints.  Every figure is printed before it is asserted."""
import functools
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import lattice_inputs as li
import step_loss_cases as sl
from conftest import PARAM_KEYS, rel_to_max

pytestmark = pytest.mark.gpu

LR, EPS, TOL = 1e-3, sl.EPS, sl.TOL
# name -> S, H, T, B, sparse (a CsrAdjacency: the general path)
SHAPES = {"s7": (7, 21, 12, 4, False),          # f2b's shape
          "s34": (34, 102, 5, 17, False),       # one full workgroup of 16 windows plus a ragged one
          "csr12": (12, 36, 4, 3, True),
          "s43": (43, 129, 3, 2, False)}        # the wide-GRU path (H > 128 in f32)
COMBOS = [("s7", "f32"), ("s7", "f16x3"), ("s34", "f32"), ("s34", "f16x3"), ("csr12", "f16x3"), ("s43", "f32")]
IDS = ["%s-%s" % c for c in COMBOS]
GROUPS = ["gru", "conv"]
KEYS = {"conv": PARAM_KEYS[:4], "gru": PARAM_KEYS[4:]}


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _case(name):
    S, H, T, B, sparse = SHAPES[name]
    return li.draw(S, T, B, H, sparse=sparse)


@functools.lru_cache(maxsize=None)
def _oracle(name, phases):
    """The fp64 oracle's steps on a shape, step i training the group phases[i]: Adam (oracle.adam_step) on the sub-dictionary of
    the trained tensors, its state made at a group's first step as torch.optim.Adam makes it, so each group has its own step
    number.  A list of (Y, loss, gradients, parameters after): computed once, shared, never modified."""
    from oracle import windgnn_oracle as orc
    c = _case(name)
    A, X, L = c.A.double(), c.X.double(), c.L.double()
    p = {k: v.double() for k, v in c.p.items()}
    state, out = {}, []
    for group in phases:
        Y, loss, g = orc.train_step(A, X, L, p)
        for name_g, keys in KEYS.items():
            if group in ("all", name_g):
                sub = {k: p[k] for k in keys}
                if name_g not in state:
                    state[name_g] = orc.adam_init(sub)
                p = dict(p, **orc.adam_step(sub, g, state[name_g], lr=LR, eps=EPS))
        out.append((Y, float(loss), g, p))
    return out


def _model(name, mode, p=None):
    from windgnn_amd import GCN_GRU
    S, H, _, _, _ = SHAPES[name]
    m = GCN_GRU(13, 13, 13, S * 13, H, math=mode, validate=False)
    m.load_state_dict({k: v.clone() for k, v in (p or _case(name).p).items()})
    return m.to(_dev())


def _step(model, **kw):
    from windgnn_amd.trainer import TrainStep
    return TrainStep(model, lr=LR, eps=EPS, **kw)


def _inputs(name):
    c = _case(name)
    A = c.A
    if SHAPES[name][4]:
        from windgnn_amd.graph import CsrAdjacency
        A = CsrAdjacency.from_dense(c.A)
    return A.to(_dev()), c.X.to(_dev()), c.L.to(_dev())


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _slices(tr, group):
    """(the trained group's, the frozen group's) slice of the flat buffers [conv | GRU]."""
    conv, gru = slice(0, tr.n_conv), slice(tr.n_conv, None)
    return (gru, conv) if group == "gru" else (conv, gru)


def _same_as_all(what, ta, tg, group, p0, out_a, out_g):
    """One step of tg (trainable=group) against the same step of ta (all eight tensors) from the same state p0: Y, the loss and
    everything of the trained group bit for bit; everything of the frozen group untouched, its gradient slots +0."""
    torch.cuda.synchronize()
    on, off = _slices(tg, group)
    same = {"Y": torch.equal(_bits(out_a[1]), _bits(out_g[1])), "loss": torch.equal(_bits(out_a[0]), _bits(out_g[0]))}
    for name in ("flat_g", "flat_p", "exp_avg", "exp_avg_sq"):
        a, g = getattr(ta, name), getattr(tg, name)
        same["trained " + name] = torch.equal(_bits(a[on]), _bits(g[on]))
    same["frozen parameters keep their bits"] = torch.equal(_bits(tg.flat_p[off]), _bits(p0[off]))
    same["frozen moments keep their bits"] = not _bits(tg.exp_avg[off]).any() and not _bits(tg.exp_avg_sq[off]).any()
    same["frozen gradients read +0"] = not _bits(tg.flat_g[off]).any()
    moved = float((tg.flat_p[on] - p0[on]).abs().max())
    print("%s %s: %s; the trained parameters moved by up to %.2e; gradients differ from 'all' by at most %.2e"
          % (what, group, same, moved, float((ta.flat_g[on] - tg.flat_g[on]).abs().max())))
    assert all(same.values()), same
    assert moved > 0 and bool(tg.flat_g[on].abs().max() > 0)


# ---- 1. the first step against the step on all eight tensors ------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name,mode", COMBOS, ids=IDS)
def test_the_first_step_is_the_all_step_on_the_trained_group_bit_for_bit(name, mode, group):
    A, X, L = _inputs(name)
    ta, tg = _step(_model(name, mode)), _step(_model(name, mode), trainable=group)
    p0 = tg.flat_p.clone()
    out_a = ta.step(A, X, L)
    out_g = tg.step(A, X, L)
    _same_as_all("%s %s" % (name, mode), ta, tg, group, p0, out_a, out_g)
    assert ta.steps == tg.steps == 1
    tg.check()


# ---- 2. three steps and a change of phase against the fp64 oracle --------------------------------------------------------------------
def _follow(name, mode, phases):
    """Run `phases` (one group per step, set_trainable between them) and return the worst errors against the oracle."""
    A, X, L = _inputs(name)
    model = _model(name, mode)
    tr = _step(model, trainable=phases[0])
    p0 = tr.flat_p.clone()
    ref = _oracle(name, tuple(phases))
    worst = {"Y": 0.0, "loss": 0.0, "grad": 0.0, "params": 0.0}
    ever = set()
    for s, group in enumerate(phases):
        tr.set_trainable(group)
        loss, Y = tr.step(A, X, L)
        Yo, lo, go, po = ref[s]
        ever |= set(KEYS) if group == "all" else {group}
        trained = [k for g in (KEYS if group == "all" else [group]) for k in KEYS[g]]
        ey, el = rel_to_max(Y.cpu(), Yo), abs(float(loss) - lo) / lo
        eg = max(rel_to_max(v.cpu(), go[k]) for k, v in zip(PARAM_KEYS, tr.g_views) if k in trained)
        ep = max(rel_to_max(v.detach().cpu(), po[k]) for k, v in model.named_parameters())
        print("%s %s step %d on %s: Y %.2e  loss %.2e  worst trained gradient %.2e  worst parameter %.2e (bar %.1e)"
              % (name, mode, s + 1, group, ey, el, eg, ep, TOL))
        worst = {"Y": max(worst["Y"], ey), "loss": max(worst["loss"], el), "grad": max(worst["grad"], eg),
                 "params": max(worst["params"], ep)}
        for g in set(KEYS) - ever:          # a group that has never trained: parameters and moments keep their bits
            _, off = _slices(tr, "gru" if g == "conv" else "conv")
            assert torch.equal(_bits(tr.flat_p[off]), _bits(p0[off])), (s, g)
            assert not _bits(tr.exp_avg[off]).any() and not _bits(tr.exp_avg_sq[off]).any(), (s, g)
        if group != "all":
            _, off = _slices(tr, group)
            assert not _bits(tr.flat_g[off]).any(), (s, group)
    tr.check()
    print("%s %s: worst over %s: %s" % (name, mode, "/".join(phases), "  ".join("%s %.2e" % kv for kv in worst.items())))
    return tr, worst


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("name,mode", COMBOS, ids=IDS)
def test_three_steps_follow_the_oracles_adam_on_the_trained_tensors_only(name, mode, group):
    tr, worst = _follow(name, mode, [group] * 3)
    assert tr.steps == 3 and tr._group_count(group) == 3 and tr._group_count("conv" if group == "gru" else "gru") == 0
    assert max(worst.values()) <= TOL, worst


@pytest.mark.parametrize("name,mode", COMBOS, ids=IDS)
def test_a_gru_phase_then_all_steps_each_group_at_its_own_adam_step(name, mode):
    """Two steps on "gru", then two on "all": the conv tensors take their first Adam step (bias correction 1) while the GRU
    tensors are at 3, as torch.optim.Adam's lazily made state has it.  One shared step number misses the bar: at step 3 the conv
    update would be lr * (1 - b1) / (1 - b1^3) / sqrt((1 - b2) / (1 - b2^3)) = 0.64 of the right one."""
    tr, worst = _follow(name, mode, ["gru", "gru", "all", "all"])
    assert tr.steps == 4 and tr._group_count("gru") == 4 and tr._group_count("conv") == 2
    assert max(worst.values()) <= TOL, worst
    sd = tr.state_dict()
    assert sd["trainable"] == "all" and [float(sd["optimizer"]["state"][i]["step"]) for i in (0, 3, 4, 7)] == [2.0, 2.0, 4.0, 4.0]


# ---- 3. the skipped part is not launched ----------------------------------------------------------------------------------------------
def _profiled(fn):
    from windgnn_amd import _lib
    _lib.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        prof = {r["name"]: r["launches"] for r in _lib.profile_read()}
    finally:
        _lib.profile_enable(False)
    return out, prof


@pytest.mark.parametrize("mode", ["f32", "f16x3"])
def test_a_frozen_groups_part_of_the_backward_is_never_launched(mode):
    from windgnn_amd.functional import gcn_gru_backward_raw, gcn_gru_forward_raw
    name = "s34"
    A, X, L = _inputs(name)
    c = _case(name)
    model = _model(name, mode)
    params = [p.detach() for p in model.hot_path_parameters()]
    grads = [torch.zeros_like(p) for p in params]
    (Y, stash, d), fwd = _profiled(lambda: gcn_gru_forward_raw(A, X, params, model.math, want_stash=True))
    dY = c.dY.to(_dev())
    names = {}
    for part in (1, 2, 4):                  # parts 2 and 4 read what part 1 left in the same workspace
        _, names[part] = _profiled(lambda: gcn_gru_backward_raw(d, A, X, params, Y, dY, stash, grads, part=part))
    only = {2: set(names[2]) - set(names[1]) - set(names[4]), 4: set(names[4]) - set(names[1]) - set(names[2])}
    print("%s forward: %s\n  part 1: %s\n  part 2 alone: %s\n  part 4 alone: %s"
          % (mode, sorted(fwd), sorted(names[1]), sorted(only[2]), sorted(only[4])))
    assert only[2] - set(fwd) and only[4] - set(fwd)
    ta = _step(_model(name, mode))
    ta.step(A, X, L)                        # (the first step builds the W_ih images)
    _, whole = _profiled(lambda: ta.step(A, X, L))
    assert only[2] & set(whole) and only[4] & set(whole)                # the step on all eight tensors launches both
    for group, skipped in (("gru", 2), ("conv", 4)):
        tr = _step(_model(name, mode), trainable=group)
        tr.step(A, X, L)
        _, prof = _profiled(lambda: tr.step(A, X, L))
        print("%s a %r step launches %s" % (mode, group, sorted(prof.items())))
        for n in only[skipped]:
            if n in fwd:                    # a symbol the forward shares (a split-K sum): the forward's launches, no more
                assert prof.get(n, 0) <= fwd[n], (group, n, prof.get(n, 0), fwd[n], whole.get(n, 0))
            else:
                assert n not in prof, (group, n)
        assert only[6 - skipped] & set(prof)


# ---- 4. the other routes, at S = 7 ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", GROUPS)
def test_the_carried_state_step_with_a_frozen_group(group):
    A, X, L = _inputs("s7")
    ta, tg = _step(_model("s7", "f32"), carry_state=True), _step(_model("s7", "f32"), carry_state=True, trainable=group)
    p0 = tg.flat_p.clone()
    _same_as_all("carry_state step 1", ta, tg, group, p0, ta.step(A, X, L), tg.step(A, X, L))
    assert torch.equal(_bits(ta.state), _bits(tg.state))
    on, off = _slices(tg, group)
    tg.step(A, X, L)                        # from the carried state
    torch.cuda.synchronize()
    assert torch.equal(_bits(tg.flat_p[off]), _bits(p0[off])) and not _bits(tg.flat_g[off]).any()
    assert tg.steps == 2 and tg._has_state


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("mode", ["f32", "f16x3"])
def test_l1_with_missing_labels_with_a_frozen_group(mode, group):
    A, X, L = _inputs("s7")
    gen = torch.Generator().manual_seed(11)
    L = L.clone()
    L[(torch.rand(L.shape, generator=gen) < 0.1).to(L.device)] = float("nan")       # 10 % of the labels are missing
    kw = dict(loss="l1", missing_labels=True)
    ta, tg = _step(_model("s7", mode)), _step(_model("s7", mode), trainable=group)
    p0 = tg.flat_p.clone()
    on, off = _slices(tg, group)
    # without an optimiser step first: BPTT and the trained group's part in one call, not deferred, against all three parts
    ref, out = ta.forward_backward(A, X, L, **kw), tg.forward_backward(A, X, L, **kw)
    torch.cuda.synchronize()
    same = {"loss": torch.equal(_bits(ref[0]), _bits(out[0])), "Y": torch.equal(_bits(ref[1]), _bits(out[1])),
            "trained gradients": torch.equal(_bits(ta.flat_g[on]), _bits(tg.flat_g[on])),
            "frozen gradients read +0": not _bits(tg.flat_g[off]).any(), "no step": tg.steps == 0 and torch.equal(_bits(tg.flat_p), _bits(p0))}
    print("forward_backward l1 / 10 %% NaN %s %s: %s" % (mode, group, same))
    assert all(same.values()) and bool(tg.flat_g[on].abs().max() > 0), same
    _same_as_all("l1 / 10 %% NaN %s" % mode, ta, tg, group, p0, ta.step(A, X, L, **kw), tg.step(A, X, L, **kw))
    assert int(tg.loss_count) == int(ta.loss_count) == int((~torch.isnan(L)).sum())
    assert not torch.isnan(tg.flat_g).any() and tg.steps == 1


def _series_case():
    d = li.draw_series(7, 21, 40, 12, 3, 9)
    return d, 12


@pytest.mark.parametrize("group", GROUPS)
@pytest.mark.parametrize("how", ["strided", "starts"])
def test_step_series_with_a_frozen_group_matches_the_oracle_on_the_materialised_windows(how, group):
    """Series mode has no parts: the backward runs whole, the frozen slots are zeroed after it, the trained group alone is stepped."""
    from oracle import windgnn_oracle as orc
    from windgnn_amd import GCN_GRU
    d, T = _series_case()
    starts = [3 * w for w in range(9)] if how == "strided" else [17, 0, 28, 5, 17, 9]
    idx = torch.tensor(starts)[:, None] + torch.arange(T)[None, :]
    Xw, Lw = d.Xs[idx], d.Ls[idx]                           # the materialised windows [n, T, S, 13] and labels [n, T, H]
    p64 = {k: v.double() for k, v in d.p.items()}
    Yo, lo, go = orc.train_step(d.A.double(), Xw.double(), Lw.double(), p64)
    sub = {k: p64[k] for k in KEYS[group]}
    po = dict(p64, **orc.adam_step(sub, go, orc.adam_init(sub), lr=LR, eps=EPS))
    model = GCN_GRU(13, 13, 13, 7 * 13, 21, validate=False)
    model.load_state_dict({k: v.clone() for k, v in d.p.items()})
    tr = _step(model.to(_dev()), trainable=group)
    p0 = tr.flat_p.clone()
    A, Xs, Ls = d.A.to(_dev()), d.Xs.to(_dev()), d.Ls.to(_dev())
    where = dict(stride=3, n_windows=9) if how == "strided" else dict(starts=starts)
    loss, Y = tr.step_series(A, Xs, Ls, T, **where)
    torch.cuda.synchronize()
    on, off = _slices(tr, group)
    seen = {"Y": rel_to_max(Y.cpu(), Yo), "loss": abs(float(loss) - float(lo)) / float(lo)}
    for k, g, v in zip(PARAM_KEYS, tr.g_views, tr.p_views):
        if k in KEYS[group]:
            seen["d " + k] = rel_to_max(g.cpu(), go[k])
        seen[k] = rel_to_max(v.cpu(), po[k])
    print("step_series %s %s: %s" % (how, group, "  ".join("%s %.2e" % kv for kv in seen.items())))
    assert not _bits(tr.flat_g[off]).any() and torch.equal(_bits(tr.flat_p[off]), _bits(p0[off]))
    assert not _bits(tr.exp_avg[off]).any() and not _bits(tr.exp_avg_sq[off]).any()
    assert max(seen.values()) <= TOL, seen
    assert tr.steps == 1 and tr._group_count(group) == 1


@pytest.mark.parametrize("group", GROUPS)
def test_keep_best_keeps_the_frozen_slice_and_restores(group):
    A, X, L = _inputs("s7")
    tr = _step(_model("s7", "f16x3"), trainable=group, keep_best=True)
    p0 = tr.flat_p.clone()
    on, off = _slices(tr, group)
    for s in range(3):
        tr.step(A, X, L)
        torch.cuda.synchronize()
        assert int(tr.best_step) >= 1
        assert torch.equal(_bits(tr._best_p[off]), _bits(p0[off])), s          # the snapshot's frozen slice: the same bits
    kept, at = tr._best_p.clone(), int(tr.best_step)
    print("keep_best %s: best_step %d of 3, best_loss %.6f" % (group, at, float(tr.best_loss)))
    tr.restore_best()
    torch.cuda.synchronize()
    assert torch.equal(_bits(tr.flat_p), _bits(kept)) and torch.equal(_bits(tr.flat_p[off]), _bits(p0[off]))
    tr.step(A, X, L)                        # the images are rebuilt; the frozen group stays frozen
    torch.cuda.synchronize()
    assert torch.equal(_bits(tr.flat_p[off]), _bits(p0[off])) and tr.steps == 4


def _one_rank(rank, port, out_dir):
    from windgnn_amd.distributed import ensure_rccl_env
    ensure_rccl_env()                     # before this process touches the GPU
    A, X, L = _inputs("s7")
    res = []
    plain = {g: _step(_model("s7", "f16x3"), trainable=g) for g in GROUPS}
    for g in GROUPS:
        for _ in range(2):
            plain[g].step(A, X, L)
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    calls = {"n": 0}
    real = dist.all_reduce

    def counted(*a, **kw):
        calls["n"] += 1
        return real(*a, **kw)
    dist.all_reduce = counted
    for g in GROUPS:
        tr = _step(_model("s7", "f16x3"), process_group=dist.group.WORLD, trainable=g)
        assert tr.collective and tr.exchange.direct is None
        before = calls["n"]
        for _ in range(2):
            tr.step(A, X, L, n_global=X.shape[0])
        torch.cuda.synchronize()
        ok = (torch.equal(_bits(plain[g].flat_p), _bits(tr.flat_p)) and torch.equal(_bits(plain[g]._gbuf), _bits(tr._gbuf))
              and torch.equal(_bits(plain[g].exp_avg), _bits(tr.exp_avg)) and torch.equal(_bits(plain[g].exp_avg_sq), _bits(tr.exp_avg_sq)))
        res += [calls["n"] - before, int(ok)]
    np.save(os.path.join(out_dir, "one_rank.npy"), np.array(res))
    dist.barrier()
    dist.destroy_process_group()


def test_a_one_rank_group_all_reduces_once_per_step_and_changes_no_bit(tmp_path):
    from test_distributed_gpu import _free_port
    mp.spawn(_one_rank, args=(_free_port(), str(tmp_path)), nprocs=1, join=True)
    got = np.load(os.path.join(str(tmp_path), "one_rank.npy")).tolist()
    print("[all-reduces of two steps, every bit equal to the group-less steps] for gru, conv: %s" % got)
    assert got == [2, 1, 2, 1]


@pytest.mark.parametrize("group", GROUPS)
def test_a_side_stream_gives_the_default_streams_bits(group):
    A, X, L = _inputs("s7")
    ta, tb = _step(_model("s7", "f16x3"), trainable=group), _step(_model("s7", "f16x3"))
    for _ in range(2):
        ta.step(A, X, L)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(_dev())
    side.wait_stream(torch.cuda.current_stream(_dev()))
    with torch.cuda.stream(side):
        tb.set_trainable(group)             # its zeroing runs on the current stream, which is the side stream here
        for _ in range(2):
            tb.step(A, X, L)
    torch.cuda.synchronize()
    for name in ("flat_p", "_gbuf", "exp_avg", "exp_avg_sq"):
        assert torch.equal(_bits(getattr(ta, name)), _bits(getattr(tb, name))), name


# ---- 5. Ensemble --------------------------------------------------------------------------------------------------------------------------
def test_ensemble_members_on_three_groups_are_the_trainsteps_driven_alone():
    from windgnn_amd import Ensemble, PerMember
    A, X, L = _inputs("s7")
    groups = ["all", "gru", "conv"]
    alone = [_step(_model("s7", "f16x3"), trainable=g) for g in groups]
    for tr in alone:
        for _ in range(2):
            tr.step(A, X, L)
    ens = Ensemble([_model("s7", "f16x3") for _ in groups], lr=LR, eps=EPS, trainable=PerMember(groups))
    assert [tr.trainable for tr in ens.members] == groups
    for _ in range(2):
        ens.step(A, X, L)
    torch.cuda.synchronize()
    for g, a, b in zip(groups, alone, ens.members):
        for name in ("flat_p", "_gbuf", "exp_avg", "exp_avg_sq"):
            assert torch.equal(_bits(getattr(a, name)), _bits(getattr(b, name))), (g, name)
    ens.each(lambda k, tr: tr.set_trainable("gru"))         # and a change of phase through each()
    for tr in alone:
        tr.set_trainable("gru")
        tr.step(A, X, L)
    ens.step(A, X, L)
    torch.cuda.synchronize()
    for g, a, b in zip(groups, alone, ens.members):
        assert b.trainable == "gru" and b.steps == 3
        assert torch.equal(_bits(a.flat_p), _bits(b.flat_p)) and torch.equal(_bits(a._gbuf), _bits(b._gbuf)), g
