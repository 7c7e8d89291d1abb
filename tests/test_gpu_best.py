"""Keeping the best parameters on the device, on the MI355X (include/windgnn_best.h): the C ABI call by call inside guard bands,
the fp64 comparison, TrainStep(keep_best=...) against the reference's rule (src/main.py:83-86) run on the host for every
schedule and for two ranks, restore_best(), and stopping and resuming a TrainStep through state_dict() / load_state_dict()."""
import ctypes as C
import io
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PARAM_KEYS
from guarded import FILLS, Arena

pytestmark = pytest.mark.gpu

# (S, H, csr): the first three have every tensor misaligned and of odd length inside the flat buffer (offsets 169, 182, 351,
# 364, ...); the last has a w_ih of 624 000 floats: 610 workgroups for that tensor, one vector per thread (the grid is not yet
# scaled down and no thread wraps: test_the_copy_with_a_scaled_down_grid_and_wrapping_threads does that)
SHAPES = [(3, 9, False), (7, 21, False), (34, 102, False), (100, 160, True)]
LOSSES = [0.5, 0.7, 0.3, float("nan"), 0.3, 0.1, float("inf")]
WORDS = ("best_loss", "best_step", "calls", "improvements", "improved")


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _sizes(S, H):
    return [169, 13, 169, 13, 3 * H * S * 13, 3 * H * H, 3 * H, 3 * H]


def _dims(S, H, csr):
    from windgnn_amd import _lib
    return _lib.Dims(1, 1, S, 13, H, _lib.MATH_F32, _lib.ADJ_CSR if csr else _lib.ADJ_DENSE, 600 if csr else 0, _lib.IO_F32)


def _struct(base, sizes):
    from windgnn_amd import _lib
    s, off = _lib.Params(), 0
    for name, n in zip(_lib._SLOTS, sizes):
        setattr(s, name, base + 4 * off)
        off += n
    return s


def _words(rec):
    """The five public words of a record (a uint8 tensor, any device) as Python numbers."""
    from windgnn_amd import _lib
    from windgnn_amd.functional import best_word
    host = rec.cpu()
    assert set(_lib.BEST_WORDS) == set(WORDS)
    return {k: best_word(host, k).item() for k in WORDS}


def _rule(threshold, losses, steps):
    """The reference's rule on the host, call by call: [(public words, improved)]."""
    best, best_step, wins, out = threshold, -1, 0, []
    for k, (loss, step) in enumerate(zip(losses, steps)):
        loss = float(np.float32(loss))                   # loss.item(): the fp32 word as a Python float
        won = loss < best
        if won:
            best, best_step, wins = loss, step, wins + 1
        out.append(dict(best_loss=best, best_step=best_step, calls=k + 1, improvements=wins, improved=int(won)))
    return out


# -------------------------------------------------------------------------------------------------------------- the C ABI
@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("S,H,csr", SHAPES)
def test_keep_best_call_by_call_inside_guard_bands(S, H, csr, fill):
    """wgnn_best_init + 7 wgnn_keep_best calls, thresholds +inf and 0.4, the snapshot at the parameters' own offsets inside
    16 bytes and one float off them (the single-float form): snapshot, public words, guards and bystanders after every call."""
    from windgnn_amd import _lib
    lib = _lib.load()
    dev = _dev()
    sizes = _sizes(S, H)
    N = sum(sizes)
    d = _dims(S, H, csr)
    nrec = lib.wgnn_best_bytes()
    base = (torch.arange(N, dtype=torch.float32) % 8191.0) * 1e-3 + 1.0

    def pattern(k):                                      # the parameters before call k: differs from call to call everywhere
        return base + float(k)
    for threshold, shift in ((float("inf"), 0), (0.4, 0), (float("inf"), 4)):
        a = Arena(dev, fill, seed=S)
        pb = a.buf("p", 4 * N, data=pattern(0))
        bb = a.buf("best_p", 4 * N, offset=shift)
        rb = a.buf("record", nrec)
        lb = a.buf("loss", 4, data=torch.zeros(1))
        other = a.buf("bystander", 1024)
        a.commit()
        ps, bs = _struct(pb.ptr, sizes), _struct(bb.ptr, sizes)
        assert lib.wgnn_best_init(C.c_void_p(rb.ptr), threshold, None) == 0
        torch.cuda.synchronize()
        assert _words(rb.bytes()) == dict(best_loss=threshold, best_step=-1, calls=0, improvements=0, improved=0)
        assert int(rb.bytes()[36:].max()) == 0           # every byte written, whatever the fill was
        assert bb.unwritten(4) == N
        want = _rule(threshold, LOSSES, [10 + k for k in range(len(LOSSES))])
        snap = None
        for k, loss in enumerate(LOSSES):
            pb.write(pattern(k + 1))
            lb.write(torch.tensor([loss], dtype=torch.float32))
            if not want[k]["improved"]:
                bb.poison()
            rc = lib.wgnn_keep_best(C.byref(d), C.c_void_p(lb.ptr), C.byref(ps), C.byref(bs), 10 + k, C.c_void_p(rb.ptr), None)
            assert rc == 0, (k, rc)
            torch.cuda.synchronize()
            got = _words(rb.bytes())
            assert got == want[k], (threshold, shift, k, got, want[k])
            if want[k]["improved"]:
                snap = pattern(k + 1)
                assert torch.equal(bb.view(torch.float32).cpu(), snap), (threshold, shift, k)
            else:
                assert bb.unwritten(4) == N, (threshold, shift, k, "a non-improving call wrote the snapshot")
                if snap is not None:
                    bb.write(snap)                       # (the poison was the test's: put the kept parameters back)
            assert a.check() == {}, (threshold, shift, k, a.check())
            assert torch.equal(pb.view(torch.float32).cpu(), pattern(k + 1)), (k, "p was written")
            assert other.unwritten(1) == 1024 and int(rb.bytes()[36:].max()) == 0
            assert lb.view(torch.float32).cpu().view(torch.int32).item() == torch.tensor([loss]).view(torch.int32).item()
        wins = [k + 1 for k, w in enumerate(want) if w["improved"]]
        assert wins == ([1, 3, 6] if threshold == float("inf") else [3, 6])
        if threshold == 0.4:
            assert want[0]["best_step"] == want[1]["best_step"] == -1


def test_the_copy_with_a_scaled_down_grid_and_wrapping_threads():
    """S = 100, H = 2200 (CSR dims): w_ih 8 580 000 and w_hh 14 520 000 floats, 92 MB in all.  One vector per thread would take
    22 577 workgroups, so wgnn_keep_best scales the grid down to 2044 of its 2048 (w_ih 757, w_hh 1281, one each for the small tensors)
    and every thread of the two matrices walks its tensor 11 times: two rounds of the four-deep loop and three of the remainder
    loop, with a last, partial wrap (nv = 2 145 000 and 3 630 000 vectors against strides of 193 792 and 327 936).  An improving
    call bit for bit, then a non-improving call on a re-poisoned snapshot; guards after both."""
    from windgnn_amd import _lib
    lib = _lib.load()
    dev = _dev()
    S, H = 100, 2200
    sizes = _sizes(S, H)
    N = sum(sizes)
    want_wgs = [max(1, (n // 4 + 255) // 256) for n in sizes]
    assert sum(want_wgs) > 2048                          # the scale-down branch
    for t in (4, 5):
        wgs = want_wgs[t] * (2048 - 8) // sum(want_wgs)
        wraps = (sizes[t] // 4) / (wgs * 256)
        assert wraps > 8 and int(wraps) % 4 != 0 and wraps != int(wraps), (t, wgs, wraps)
    d = _dims(S, H, True)
    assert lib.wgnn_workspace_bytes(C.byref(d)) > 0
    g = torch.Generator().manual_seed(5)
    p1 = torch.rand(N, generator=g) + 1.0
    a = Arena(dev, "nan", seed=1)
    pb = a.buf("p", 4 * N, data=p1)
    bb = a.buf("best_p", 4 * N)
    rb = a.buf("record", lib.wgnn_best_bytes())
    lb = a.buf("loss", 4, data=torch.tensor([0.25]))
    a.commit()
    ps, bs = _struct(pb.ptr, sizes), _struct(bb.ptr, sizes)
    assert lib.wgnn_best_init(C.c_void_p(rb.ptr), float("inf"), None) == 0
    assert lib.wgnn_keep_best(C.byref(d), C.c_void_p(lb.ptr), C.byref(ps), C.byref(bs), 1, C.c_void_p(rb.ptr), None) == 0
    torch.cuda.synchronize()
    assert _words(rb.bytes()) == dict(best_loss=0.25, best_step=1, calls=1, improvements=1, improved=1)
    assert bb.unwritten(4) == 0                          # (no parameter is the NaN poison)
    assert torch.equal(bb.view(torch.float32), p1.to(dev))
    assert a.check() == {} and torch.equal(pb.view(torch.float32), p1.to(dev))
    bb.poison()
    pb.write(p1 + 1.0)
    lb.write(torch.tensor([0.25]))                       # equal is not below
    assert lib.wgnn_keep_best(C.byref(d), C.c_void_p(lb.ptr), C.byref(ps), C.byref(bs), 2, C.c_void_p(rb.ptr), None) == 0
    torch.cuda.synchronize()
    assert _words(rb.bytes()) == dict(best_loss=0.25, best_step=1, calls=2, improvements=1, improved=0)
    assert bb.unwritten(4) == N and a.check() == {}


def test_the_comparison_is_fp64_as_pythons():
    """loss.item() < 0.03 with a loss word of float32(0.03) = 0.02999999932944774 is True in Python; an fp32 comparison with
    float32(0.03) says False.  The next fp32 above it is above 0.03 either way."""
    from windgnn_amd.functional import best_bytes, best_init, keep_best
    dev = _dev()
    S, H = 3, 9
    sizes = _sizes(S, H)
    d = _dims(S, H, False)
    at = np.float32(0.03)
    above = np.nextafter(at, np.float32(1))
    assert float(at) < 0.03 < float(above)
    for word, wins in ((at, True), (above, False)):
        p = torch.arange(sum(sizes), dtype=torch.float32, device=dev)
        best = torch.full_like(p, -1.0)
        rec = torch.empty(best_bytes(), dtype=torch.uint8, device=dev)
        best_init(rec, 0.03)
        loss = torch.tensor(float(word), dtype=torch.float32, device=dev)
        keep_best(d, loss, list(p.split(sizes)), list(best.split(sizes)), 5, rec)
        torch.cuda.synchronize()
        w = _words(rec)
        assert w["improved"] == int(wins) and w["best_step"] == (5 if wins else -1), (word, w)
        assert w["best_loss"] == (float(word) if wins else 0.03)
        assert torch.equal(best, p) if wins else bool((best == -1.0).all())


# ------------------------------------------------------------------------------------------------------------- TrainStep
def _batches(S, T, B, H, scales, seed):
    """One random batch per entry of `scales`, its labels scaled by it: the loss (~ scale^2 / 3 for outputs in (-1, 1)) goes
    up as well as down whatever the parameters do."""
    g = torch.Generator().manual_seed(seed)
    return [(torch.rand(B, T, S, 13, generator=g), torch.rand(B, T, H, generator=g) * s) for s in scales]


def _adjacency(S, dev, csr=False):
    if csr:
        from windgnn_amd.graph import CsrAdjacency, build_knn_adjacency, synthetic_station_coords
        return CsrAdjacency(*build_knn_adjacency(synthetic_station_coords(S, seed=3), 6)).to(dev)
    g = torch.Generator().manual_seed(S)
    return (torch.rand(S, S, generator=g) / S + 0.01).to(dev)


def _trainer(S, H, math_mode, dev, seed=1, **kw):
    from oracle import windgnn_oracle as orc
    from windgnn_amd import GCN_GRU
    from windgnn_amd.trainer import TrainStep
    m = GCN_GRU(13, 13, 13, S * 13, H, math=math_mode).to(dev)
    m.load_state_dict(orc.init_params(S, 13, H, seed=seed))
    return TrainStep(m, check_every=0, **kw)


def _precondition(losses, wins, stale):
    """At least `wins` improvements, and at least `stale` non-improving steps after the first improvement."""
    rule = _rule(float("inf"), losses, range(1, len(losses) + 1))
    first = next(k for k, w in enumerate(rule) if w["improved"])
    assert rule[-1]["improvements"] >= wins, losses
    assert sum(1 for w in rule[first + 1:] if not w["improved"]) >= stale, losses


def _against_the_host_rule(kept, plain, A, batches, dev, threshold=float("inf"), tag=""):
    """Step `kept` (keep_best set) and `plain` (keep_best=None, the rule run on the host after every step) side by side."""
    best, best_step, snap, losses = threshold, -1, None, []
    for k, (X, L) in enumerate(batches):
        X, L = X.to(dev), L.to(dev)
        kept.step(A, X, L)
        loss, _ = plain.step(A, X, L)
        won = float(loss) < best                         # src/main.py:83
        if won:
            snap = plain.flat_p.clone()                  # :84, the parameters after optimizer.step()
            best, best_step = float(loss), plain.steps   # :85
        losses.append(float(loss))
        for name in ("flat_p", "exp_avg", "exp_avg_sq"):
            assert torch.equal(getattr(kept, name), getattr(plain, name)), (tag, k, name)
        assert float(kept.best_loss) == best and int(kept.best_step) == best_step and int(kept.improved) == int(won), (tag, k)
        bsd = kept.best_state_dict()
        if snap is None:
            assert bsd is None, (tag, k)
        else:
            assert list(bsd) == PARAM_KEYS, (tag, k)
            assert torch.equal(torch.cat([v.reshape(-1) for v in bsd.values()]), snap), (tag, k)
            assert all(v.shape == p.shape for v, p in zip(bsd.values(), kept.params)), (tag, k)
    return losses


def test_keep_best_options_and_the_record_through_state_dict():
    """What tests/test_best_host.py cannot do without a record: the option values, the views, and a record + snapshot through
    state_dict() / load_state_dict(), its refusals included (they leave the step as it was)."""
    dev = _dev()
    S, H = 7, 21
    assert _trainer(S, H, "f32", dev, keep_best=False).keep_best is None
    for value, want in ((True, float("inf")), (0.03, 0.03), (1, 1.0)):
        tr = _trainer(S, H, "f32", dev, keep_best=value, max_grad_norm=1.0, carry_state=True)
        assert tr.keep_best == want
        assert tr.best_loss.dtype == torch.float64 and tr.best_step.dtype == torch.int64 and tr.improved.dtype == torch.int32
        assert tr.best_loss.dim() == 0 and float(tr.best_loss) == want and int(tr.best_step) == -1 and int(tr.improved) == 0
        assert tr.best_loss.data_ptr() == tr._best.data_ptr()            # views of the record, not copies
        assert tr.best_state_dict() is None
        with pytest.raises(RuntimeError, match="no step has beaten"):
            tr.restore_best()
        assert tr._best_p.shape == tr.flat_p.shape
    a = _trainer(S, H, "f32", dev, keep_best=0.5)
    sd = a.state_dict()
    from windgnn_amd import _lib
    assert set(sd["best"]) == set(_lib.BEST_WORDS) | set(PARAM_KEYS)
    sd["best"].update(best_loss=torch.tensor(0.125, dtype=torch.float64), best_step=torch.tensor(7), calls=torch.tensor(9),
                      improvements=torch.tensor(3), improved=torch.tensor(1, dtype=torch.int32))
    for k in PARAM_KEYS:
        sd["best"][k] = torch.full_like(sd["best"][k], 2.5)
    b = _trainer(S, H, "f32", dev, keep_best=True)
    b.load_state_dict(sd)
    assert _words(b._best) == dict(best_loss=0.125, best_step=7, calls=9, improvements=3, improved=1)
    bsd = b.best_state_dict()
    assert list(bsd) == PARAM_KEYS and all(bool((v == 2.5).all()) for v in bsd.values())
    # refusals: nothing of the step is written
    b.exp_avg.fill_(3.0)
    for mutate, match in ((lambda q: q.update({"conv2.bias": torch.zeros(12)}), r"best conv2\.bias is \(12,\), expected \(13,\)"),
                          (lambda q: q.update(best_loss=torch.tensor(float("nan"))), "best_loss is NaN"),
                          (lambda q: q.pop("calls"), "lacks calls")):
        bad = dict(sd, best=dict(sd["best"]))
        mutate(bad["best"])
        with pytest.raises(ValueError, match=match):
            b.load_state_dict(bad)
        assert b.steps == 0 and bool((b.exp_avg == 3.0).all()) and _words(b._best)["best_step"] == 7
    sd["best"] = None                                                     # a checkpoint without one: back to the threshold
    b.load_state_dict(sd)
    assert float(b.best_loss) == float("inf") and int(b.best_step) == -1 and b.best_state_dict() is None


SCALES12 = [2.0, 1.5, 1.8, 1.0, 1.2, 0.7, 0.9, 1.1, 0.5, 0.8, 0.6, 0.4]
SCALES6 = [2.0, 1.0, 1.5, 0.6, 0.9, 0.4]


@pytest.mark.parametrize("math_mode", ["f32", "f16x3"])
def test_trainstep_keep_best_against_the_rule_on_the_host(math_mode):
    dev = _dev()
    S, T, B, H = 34, 6, 4, 102
    A = _adjacency(S, dev)
    kept, plain = _trainer(S, H, math_mode, dev, keep_best=True), _trainer(S, H, math_mode, dev)
    losses = _against_the_host_rule(kept, plain, A, _batches(S, T, B, H, SCALES12, 21), dev, tag=math_mode)
    print(math_mode, "losses", ["%.4f" % v for v in losses])
    _precondition(losses, 3, 3)
    assert kept.steps == 12 and _words(kept._best)["calls"] == 12


def test_the_kernel_tally_of_a_step_with_and_without_keep_best():
    from windgnn_amd import _lib
    dev = _dev()
    S, T, B, H = 7, 4, 3, 21
    A = _adjacency(S, dev)
    (X, L), = _batches(S, T, B, H, [1.0], 2)
    X, L = X.to(dev), L.to(dev)
    names = {}
    for kb in (None, True):
        tr = _trainer(S, H, "f32", dev, keep_best=kb)
        tr.step(A, X, L)
        _lib.profile_enable(True)
        try:
            before = {k["name"]: k["launches"] for k in _lib.profile_read()}
            tr.step(A, X, L)
            after = {k["name"]: k["launches"] for k in _lib.profile_read()}
        finally:
            _lib.profile_enable(False)
        names[kb] = {n: c - before.get(n, 0) for n, c in after.items() if c - before.get(n, 0)}
    assert not [n for n in names[None] if n.startswith("best_")], names[None]
    assert names[True].get("best_decide_kernel") == 1 and names[True].get("best_copy_kernel") == 1, names[True]
    assert {n: c for n, c in names[True].items() if not n.startswith("best_")} == names[None]   # the step itself: launch for launch


def test_carry_state_and_clipped_steps_take_keep_best():
    dev = _dev()
    S, T, B, H = 7, 4, 3, 21
    A = _adjacency(S, dev)
    batches = _batches(S, T, B, H, SCALES6, 4)
    for math_mode in ("f32", "f16x3"):
        kw = dict(carry_state=True)
        losses = _against_the_host_rule(_trainer(S, H, math_mode, dev, keep_best=True, **kw), _trainer(S, H, math_mode, dev, **kw),
                                        A, batches, dev, tag="carry " + math_mode)
        _precondition(losses, 3, 2)
        watch = _trainer(S, H, math_mode, dev, max_grad_norm=float("inf"))
        watch.step(A, batches[0][0].to(dev), batches[0][1].to(dev))
        kw = dict(max_grad_norm=1e-3 * float(watch.grad_norm))
        kept = _trainer(S, H, math_mode, dev, keep_best=True, **kw)
        losses = _against_the_host_rule(kept, _trainer(S, H, math_mode, dev, **kw), A, batches, dev, tag="clip " + math_mode)
        _precondition(losses, 3, 2)
        assert float(kept.clip_coef) < 1.0


def _one_rank_schedules(rank, port):
    """An explicit one-rank RCCL group: the one-bucket collective step, overlap_collectives, and grad_blocks = 2 at H = 200."""
    from windgnn_amd.distributed import ensure_rccl_env
    ensure_rccl_env()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    grp = dist.group.WORLD
    try:
        for tag, S, H, csr, kw in (("plain", 7, 21, False, {}), ("overlap", 7, 21, False, dict(overlap_collectives=True)),
                                   ("blocks", 20, 200, True, dict(grad_blocks=2))):
            A = _adjacency(S, dev, csr)
            batches = _batches(S, 4, 3, H, SCALES6, 6)
            kept = _trainer(S, H, "f32", dev, keep_best=True, process_group=grp, **kw)
            plain = _trainer(S, H, "f32", dev, process_group=grp, **kw)
            assert kept.collective and (kept.plan is not None) == (tag == "blocks")
            _precondition(_against_the_host_rule(kept, plain, A, batches, dev, tag=tag), 3, 2)
        dist.barrier()
    finally:
        dist.destroy_process_group()


def test_the_collective_schedules_take_keep_best():
    mp.spawn(_one_rank_schedules, args=(_free_port(),), nprocs=1, join=True)


SCHED2 = ((31, 2.0), (32, 1.0), (1, 1.5), (29, 0.6), (32, 0.9), (1, 0.3))    # (global batch, label scale): unequal, empty shards


def _two_ranks(rank, world, port, out_dir):
    from windgnn_amd.distributed import shard_windows
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    dev = torch.device("cuda:0")
    S, T, H = 7, 4, 21
    A = _adjacency(S, dev)
    tr = _trainer(S, H, "f16x3", dev, keep_best=True)
    assert tr.world == world and tr.collective
    g = torch.Generator().manual_seed(9)
    losses, empty, best, host_snap = [], 0, float("inf"), None
    for n_glob, scale in SCHED2:
        X, L = torch.rand(n_glob, T, S, 13, generator=g), torch.rand(n_glob, T, H, generator=g) * scale
        Xs, Ls = shard_windows(X, L, rank, world)
        empty += int(Xs.shape[0] == 0)
        loss, _ = tr.step(A, Xs.to(dev), Ls.to(dev), n_global=n_glob)
        losses.append(float(loss))
        if losses[-1] < best:                            # the rule on the host, on this rank
            best, host_snap = losses[-1], tr.flat_p.clone()
    torch.cuda.synchronize()
    np.savez(os.path.join(out_dir, "rank%d.npz" % rank), record=tr._best.cpu().numpy(), snap=tr._best_p.cpu().numpy(),
             host_snap=host_snap.cpu().numpy(), losses=np.array(losses), empty=np.array(empty))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_keep_the_same_best(tmp_path):
    """Two gloo ranks on the one device, unequal shards, and steps in which rank 1 has no windows: record and snapshot are
    bit-identical on both ranks, and what the rule gives for the (all-reduced) losses."""
    mp.spawn(_two_ranks, args=(2, _free_port(), str(tmp_path)), nprocs=2, join=True)
    r0, r1 = (np.load(os.path.join(str(tmp_path), "rank%d.npz" % r)) for r in (0, 1))
    assert int(r0["empty"]) == 0 and int(r1["empty"]) == 2
    assert np.array_equal(r0["record"], r1["record"]) and np.array_equal(r0["snap"], r1["snap"])
    assert np.array_equal(r0["losses"].astype(np.float32).view(np.int32), r1["losses"].astype(np.float32).view(np.int32))
    want = _rule(float("inf"), r0["losses"], range(1, len(SCHED2) + 1))
    _precondition(list(r0["losses"]), 3, 2)
    assert _words(torch.from_numpy(r0["record"])) == want[-1]
    assert np.array_equal(r0["snap"], r0["host_snap"]) and np.array_equal(r1["snap"], r1["host_snap"])


def test_restore_best_rebuilds_the_staged_images():
    from windgnn_amd import GCN_GRU
    from windgnn_amd.trainer import TrainStep
    dev = _dev()
    S, T, B, H = 34, 6, 4, 102
    A = _adjacency(S, dev)
    batches = [(X.to(dev), L.to(dev)) for X, L in _batches(S, T, B, H, [1.0, 0.5, 1.5, 1.2], 13)]
    tr = _trainer(S, H, "f16x3", dev, keep_best=True)
    for X, L in batches:
        tr.step(A, X, L)
    assert int(tr.best_step) == 2 and tr.steps == 4 and tr._prepared is not None
    last = tr.flat_p.clone()
    bsd = tr.best_state_dict()
    buf = io.BytesIO()
    torch.save(bsd, buf)                                 # what the reference's load_state_dict(torch.load(PATH)) takes
    buf.seek(0)
    loaded = torch.load(buf)
    assert list(loaded) == PARAM_KEYS and all(torch.equal(loaded[k], bsd[k]) for k in PARAM_KEYS)
    m, v, steps = tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr.steps
    tr.restore_best()
    assert not torch.equal(tr.flat_p, last)
    assert torch.equal(tr.flat_p, torch.cat([t.reshape(-1) for t in bsd.values()]))
    assert torch.equal(tr.exp_avg, m) and torch.equal(tr.exp_avg_sq, v) and tr.steps == steps     # the optimiser is untouched
    X, L = batches[0]
    loss, Y = tr.forward_backward(A, X, L)               # reads W_ih through the staged images
    loss, Y = loss.clone(), Y.clone()
    fresh = GCN_GRU(13, 13, 13, S * 13, H, math="f16x3").to(dev)
    fresh.load_state_dict(loaded)
    loss2, Y2 = TrainStep(fresh, check_every=0).forward_backward(A, X, L)
    assert torch.equal(Y, Y2) and torch.equal(loss, loss2)
    with torch.no_grad():
        assert torch.equal(tr.model(A, X), fresh(A, X))


RESUME = [("f32", {}), ("f16x3", {}), ("f32", dict(carry_state=True, keep_best=0.5))]


@pytest.mark.parametrize("math_mode,kw", RESUME, ids=["f32", "f16x3", "f32-carry-threshold"])
def test_stop_and_resume_is_the_straight_run(math_mode, kw):
    """5 straight steps against 3 steps, model.state_dict() + TrainStep.state_dict() into a fresh model and TrainStep, 2 more."""
    from windgnn_amd import GCN_GRU
    from windgnn_amd.trainer import TrainStep
    dev = _dev()
    S, T, B, H = 34, 6, 4, 102
    A = _adjacency(S, dev)
    kw = dict(dict(keep_best=True), **kw)
    batches = [(X.to(dev), L.to(dev)) for X, L in _batches(S, T, B, H, [2.0, 1.0, 1.5, 0.6, 0.9], 17)]
    straight = _trainer(S, H, math_mode, dev, lr=2e-3, betas=(0.85, 0.995), **kw)
    losses = [float(straight.step(A, X, L)[0]) for X, L in batches]
    first = _trainer(S, H, math_mode, dev, lr=2e-3, betas=(0.85, 0.995), **kw)
    for X, L in batches[:3]:
        first.step(A, X, L)
    buf = io.BytesIO()
    torch.save({"model": first.model.state_dict(), "step": first.state_dict()}, buf)     # through a file, as a user would
    buf.seek(0)
    ckpt = torch.load(buf)
    assert ckpt["step"]["steps"] == 3 and (ckpt["step"]["carry"] is not None) == bool(kw.get("carry_state"))
    model = GCN_GRU(13, 13, 13, S * 13, H, math=math_mode).to(dev)
    model.load_state_dict(ckpt["model"])
    resumed = TrainStep(model, check_every=0, **kw)      # lr / betas come back from the checkpoint
    resumed.load_state_dict(ckpt["step"])
    assert resumed.steps == 3 and (resumed.lr, resumed.betas) == (2e-3, (0.85, 0.995))
    opt = torch.optim.Adam(model.parameters())
    opt.load_state_dict(ckpt["step"]["optimizer"])
    for p, m, v in zip(model.parameters(), resumed.m_views, resumed.v_views):
        assert torch.equal(opt.state[p]["exp_avg"], m) and torch.equal(opt.state[p]["exp_avg_sq"], v)
        assert float(opt.state[p]["step"]) == 3.0
    for X, L in batches[3:]:
        resumed.step(A, X, L)
    torch.cuda.synchronize()
    assert resumed.steps == straight.steps == 5
    for name in ("flat_p", "exp_avg", "exp_avg_sq", "_best_p"):
        assert torch.equal(getattr(resumed, name), getattr(straight, name)), name
    assert _words(resumed._best) == _words(straight._best)
    want = _rule(float("inf") if kw["keep_best"] is True else kw["keep_best"], losses, range(1, 6))
    print(math_mode, kw, "losses", ["%.4f" % v for v in losses])
    assert _words(straight._best) == want[-1]
    # keep_best=True: the checkpoint held a kept model; in every case the resumed steps replaced what it held
    assert (want[2]["best_step"] > 0 or kw["keep_best"] is not True) and want[-1]["best_step"] > 3, want
    assert math.isfinite(want[-1]["best_loss"])
    if kw.get("carry_state"):
        assert torch.equal(resumed.state, straight.state) and float(straight.state.abs().max()) > 0
    else:
        assert resumed.state is None
