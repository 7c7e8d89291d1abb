"""On-device evaluation statistics on the MI355X (include/windgnn_eval.h, windgnn_amd/evaluate.py) against a numpy fp64
restatement of the reference's test loop and statistics (src/main.py:103-157), applied to the SAME fp32 predictions the device
read.

Bars (derived, not tuned):
  header rows   n exact; the four sums relative 1e-10 (linear fp64 accumulation: n 2^-53 <= 6e-13 at n = 5000, margin for order)
  stats         relative 2.4e-7 = two fp32 ulps (one rounding of an fp64 result, plus slack)
  abs_err       bit-equal to np.float32(|e|)
The accuracy's standard deviation is formed as sqrt(Σa²/n - (Σa/n)²): its absolute error in the variance is a few 2^-53 E[a²]
~ 4e-16, so the relative bar holds from std ~ 5e-5 upwards.  The inputs below give std ~ 0.18 (>= 1e-2 in every column from
B = 37; asserted); at B = 3 the smallest of the 12 288 columns' stds is ~2e-4 (asserted >= 1e-4), and at B = 1 both sides give
exactly 0 (a*a - a*a with contraction off)."""
import ctypes as C
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import load_fixture
from guarded import FILLS, Arena

pytestmark = pytest.mark.gpu

SHAPES = [(1, 1, 3), (1, 168, 102), (37, 5, 21), (1000, 2, 102), (3, 2, 12288), (5000, 1, 102)]
WINDS = [(0.0, 60.0), (1.5, 83.25)]
SUM_TOL, STAT_TOL, MERGE_TOL = 1e-10, 2.4e-7, 1e-12


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _gpu(a):
    return torch.from_numpy(np.array(a)).to(_dev())


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _oracle(pred, labels, wind_min, wind_max):
    """src/main.py:103-157 in fp64 on pred [N,H] fp32 (de-normalised) and labels [N,T,H] fp32 (normalised): the header sums, the
    four figures per column [H,4] and the absolute errors as fp32."""
    wmin, wmax = np.float64(np.float32(wind_min)), np.float64(np.float32(wind_max))
    truth = labels[:, -1, :].astype(np.float64) * (wmax - wmin) + wmin                    # main.py:104
    diff = truth - pred.astype(np.float64)
    err = np.abs(diff)                                                                    # main.py:105
    with np.errstate(divide="ignore", invalid="ignore"):
        acc = 1 - err / truth                                                             # main.py:123
        stats = np.stack([np.sqrt(np.mean(diff ** 2, axis=0)), np.average(err, axis=0), np.average(acc, axis=0),
                          np.std(acc, axis=0)], axis=1)
        header = np.stack([np.full(pred.shape[1], float(pred.shape[0])), (diff ** 2).sum(0), err.sum(0), acc.sum(0),
                           (acc ** 2).sum(0)])
    return dict(header=header, stats=stats, abs_err=err.astype(np.float32))


@functools.lru_cache(maxsize=None)
def _inputs(B, T, H, wind):
    """labels ~ U[0.2, 1), pred = truth (1 + 0.3 N(0,1)) rounded to fp32; numpy arrays and their oracle, computed once."""
    rng = np.random.default_rng(1000003 * B + 1009 * T + H + int(10 * wind[1]))
    labels = rng.uniform(0.2, 1.0, size=(B, T, H)).astype(np.float32)
    labels = np.maximum(labels, np.float32(0.2))
    truth = labels[:, -1, :].astype(np.float64) * (np.float64(wind[1]) - np.float64(wind[0])) + np.float64(wind[0])
    pred = (truth * (1.0 + 0.3 * rng.standard_normal((B, H)))).astype(np.float32)
    for a in (labels, pred):
        a.setflags(write=False)
    return labels, pred, _oracle(pred, labels, *wind)


def _close(got, want, tol, what):
    """|got - want| <= tol |want| elementwise; non-finite entries must agree exactly (inf with inf of the same sign, NaN with NaN)."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(np.isnan(got), np.isnan(want)), (what, "NaNs differ")
    assert np.array_equal(got[~fin & ~np.isnan(want)], want[~fin & ~np.isnan(want)]), (what, "infinities differ")
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(fin & (want != 0), np.abs(got - want) / np.abs(want), np.abs(got - want))
    worst = float(rel[fin].max()) if fin.any() else 0.0
    print("%s: worst relative error %.3e (bar %.1e)" % (what, worst, tol))
    assert worst <= tol, (what, worst)


def _header(acc, H):
    return acc[:5 * H].view(5, H).cpu().numpy()


def _check_against_oracle(acc, H, orc, what):
    from windgnn_amd.evaluate import eval_stats
    hdr = _header(acc, H)
    assert np.array_equal(hdr[0], orc["header"][0]), (what, "n")
    _close(hdr[1:], orc["header"][1:], SUM_TOL, what + " header sums")
    _close(eval_stats(acc, H).cpu().numpy(), orc["stats"], STAT_TOL, what + " stats")


# ------------------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("wind", WINDS)
@pytest.mark.parametrize("B,T,H", SHAPES)
def test_accum_and_stats_against_numpy(B, T, H, wind):
    from windgnn_amd.evaluate import eval_accum, eval_buffer
    dev = _dev()
    labels, pred, orc = _inputs(B, T, H, wind)
    std = orc["stats"][:, 3]
    print("B %d T %d H %d wind %s: accuracy std min %.3e median %.3e" % (B, T, H, wind, std.min(), np.median(std)))
    if B >= 37:
        assert std.min() >= 1e-2
    elif B > 1:
        assert std.min() >= 1e-4
    else:
        assert (std == 0).all()
    acc = eval_buffer(H, dev)
    err = torch.full((B, H), float("nan"), device=dev)
    eval_accum(_gpu(pred), _gpu(labels), wind[0], wind[1], acc, err)
    _check_against_oracle(acc, H, orc, "B%d T%d H%d" % (B, T, H))
    assert np.array_equal(err.cpu().numpy().view(np.int32), orc["abs_err"].view(np.int32)), "abs_err is not np.float32(|e|)"
    # without abs_err: the same accumulator, bit for bit
    acc2 = eval_buffer(H, dev)
    eval_accum(_gpu(pred), _gpu(labels), wind[0], wind[1], acc2)
    assert torch.equal(acc[:5 * H].view(torch.int64), acc2[:5 * H].view(torch.int64))


def test_three_calls_equal_one_call_on_the_concatenation_and_repeat_bit_for_bit():
    from windgnn_amd.evaluate import eval_accum, eval_buffer, eval_stats
    dev = _dev()
    T, H, wind = 3, 102, WINDS[1]
    parts = [_inputs(b, T, H, wind) for b in (5, 1, 37)]
    labels = np.concatenate([p[0] for p in parts])
    pred = np.concatenate([p[1] for p in parts])

    def sequence():
        acc = eval_buffer(H, dev)
        for lab, prd, _ in parts:
            eval_accum(_gpu(prd), _gpu(lab), wind[0], wind[1], acc)
        return acc
    a1, a2 = sequence(), sequence()
    assert torch.equal(a1[:5 * H].view(torch.int64), a2[:5 * H].view(torch.int64)), "the same sequence gave different bytes"
    assert torch.equal(eval_stats(a1, H).view(torch.int32), eval_stats(a2, H).view(torch.int32))
    one = eval_buffer(H, dev)
    eval_accum(_gpu(pred), _gpu(labels), wind[0], wind[1], one)
    h3, h1 = _header(a1, H), _header(one, H)
    assert np.array_equal(h3[0], h1[0]) and (h1[0] == 43).all()
    _close(h3[1:], h1[1:], MERGE_TOL, "three calls vs one")
    _check_against_oracle(a1, H, _oracle(pred, labels, *wind), "three calls")


def test_a_zero_truth_poisons_its_own_column_only():
    from windgnn_amd.evaluate import eval_accum, eval_buffer, eval_stats
    dev = _dev()
    B, T, H, wind = 37, 5, 21, WINDS[0]
    labels0, pred0, _ = _inputs(B, T, H, wind)
    b, c = 11, 8
    pred = pred0.copy()
    pred[b, c] = 3.0
    out = {}
    for value in (0.0, 0.5):
        labels = labels0.copy()
        labels[b, T - 1, c] = value
        acc = eval_buffer(H, dev)
        eval_accum(_gpu(pred), _gpu(labels), wind[0], wind[1], acc)
        orc = _oracle(pred, labels, *wind)
        stats = eval_stats(acc, H).cpu().numpy()
        _close(_header(acc, H)[1:], orc["header"][1:], SUM_TOL, "label %g header" % value)
        _close(stats, orc["stats"], STAT_TOL, "label %g stats" % value)
        out[value] = (_header(acc, H), stats)
    h0, s0 = out[0.0]
    assert s0[c, 2] == -np.inf and np.isnan(s0[c, 3]) and np.isfinite(s0[c, :2]).all()
    assert h0[3, c] == -np.inf and h0[4, c] == np.inf
    others = np.arange(H) != c
    assert np.array_equal(h0[:, others].view(np.int64), out[0.5][0][:, others].view(np.int64))
    assert np.array_equal(s0[others].view(np.int32), out[0.5][1][others].view(np.int32))
    assert np.isfinite(out[0.5][1]).all()


def test_an_empty_accumulator_gives_nan_everywhere():
    from windgnn_amd.evaluate import eval_buffer, eval_stats
    for H in (3, 102):
        out = torch.zeros(H, 4, device=_dev())
        assert eval_stats(eval_buffer(H, _dev()), H, out) is out
        assert out.isnan().all()


# ---------------------------------------------------------------------------------------------------------------- footprint
@pytest.mark.parametrize("B,T,H", [(5, 2, 102), (37, 5, 21), (1000, 2, 102)])
def test_footprint_of_eval_accum_and_eval_stats(B, T, H):
    """acc, abs_err and out of their exact ABI lengths inside poisoned guard bands; abs_err, out and the PRIVATE part of acc
    start as zeros, finite noise and NaNs (acc's header zeroed: the empty accumulator); the guards stay intact, every element
    of abs_err and out is written and all results are bit-identical across the fills.  One- and two-launch decompositions."""
    from windgnn_amd import _lib
    lib = _lib.load()
    dev = _dev()
    wind = WINDS[1]
    labels, pred, orc = _inputs(B, T, H, wind)
    nacc = lib.wgnn_eval_bytes(H)
    assert nacc >= 40 * H and nacc % 256 == 0
    base = None
    for fill in FILLS:
        a = Arena(dev, fill)
        bp = a.buf("pred", pred.nbytes, data=torch.from_numpy(pred.copy()))
        bl = a.buf("labels", labels.nbytes, data=torch.from_numpy(labels.copy()))
        ba = a.buf("acc", nacc, zero_head=40 * H)
        be = a.buf("abs_err", 4 * B * H)
        bo = a.buf("out", 16 * H)
        a.commit()
        V = C.c_void_p
        for _ in range(2):                                                # two calls: the second reads what the first left
            rc = lib.wgnn_eval_accum(V(bp.ptr), V(bl.ptr), B, T, H, wind[0], wind[1], V(ba.ptr), V(be.ptr), None)
            assert rc == 0, rc
        assert lib.wgnn_eval_stats(V(ba.ptr), H, V(bo.ptr), None) == 0
        torch.cuda.synchronize()
        assert a.check() == {}, (fill, a.check())
        if fill != "zero":
            assert be.unwritten(4) == 0 and bo.unwritten(4) == 0, (fill, be.unwritten(4), bo.unwritten(4))
        res = (ba.host()[:40 * H].clone(), be.host(), bo.host())
        if base is None:
            base = res
            hdr = res[0].view(torch.float64).view(5, H).numpy()
            assert (hdr[0] == 2 * B).all()
            _close(hdr[1:], 2 * orc["header"][1:], SUM_TOL, "footprint header (two calls)")
            assert np.array_equal(res[1].view(torch.int32).view(B, H).numpy(), orc["abs_err"].view(np.int32))
            _close(res[2].view(torch.float32).view(H, 4).numpy()[:, :3], orc["stats"][:, :3], STAT_TOL, "footprint stats")
        else:
            for x, y, name in zip(base, res, ("acc header", "abs_err", "out")):
                assert torch.equal(x, y), (fill, name)


# --------------------------------------------------------------------------------------------------------------- end to end
def _model(fx, math, dev):
    from windgnn_amd import GCN_GRU
    m = GCN_GRU(13, 13, 13, 34 * 13, 102, math=math).to(dev)
    m.load_state_dict({k: v.clone() for k, v in fx["params"].items()})
    return m


@pytest.mark.parametrize("math", ["f32", "f16x3"])
@pytest.mark.parametrize("name", ["f3_s34_t24_b4_ckpt", "f4_s34_t168_b1_ckpt"])
def test_evaluator_against_forward_last_and_numpy(name, math):
    from windgnn_amd import Evaluator
    from windgnn_amd.data import forward_last
    dev = _dev()
    fx = load_fixture(name)
    A, X, L = (torch.from_numpy(fx[k]).to(dev) for k in ("A", "X", "L"))
    wind = WINDS[1]
    m = _model(fx, math, dev)
    ev = Evaluator(m, A, wind[0], wind[1], keep_errors=True)
    # the loader's shapes: [B,T,3S] batches, a [1,T,3S] batch and a bare [T,3S] window
    if X.shape[0] == 4:
        batches = [(X[:3].contiguous(), L[:3].contiguous()), (X[3:].contiguous(), L[3])]
    else:
        batches = [(X, L), (X, L[0])]
    preds = []
    for bx, by in batches:
        got = ev.update(bx, by)
        want = forward_last(m, A, bx, wind[0], wind[1])
        assert got.shape == want.shape and (got.dim() == 1) == (bx.shape[0] == 1)
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), "update's prediction is not forward_last's"
        preds.append(got.reshape(-1, 102).cpu().numpy())
    pred = np.concatenate(preds)
    labels = np.concatenate([by.reshape(-1, by.shape[-2], 102).cpu().numpy() for _, by in batches])
    orc = _oracle(pred, labels, *wind)
    r = ev.compute()
    assert r.stats.is_cuda and tuple(r.stats.shape) == (3, 34, 4) and int(r.count) == pred.shape[0]
    _close(r.stats.view(102, 4).cpu().numpy(), orc["stats"], STAT_TOL, "%s %s stats" % (name, math))
    hdr = r.header.cpu().numpy()
    assert np.array_equal(hdr[0], orc["header"][0])
    _close(hdr[1:], orc["header"][1:], SUM_TOL, "%s %s header" % (name, math))
    n, S, rng = pred.shape[0], 34, np.float64(wind[1]) - np.float64(wind[0])
    want_mse = orc["header"][1].reshape(3, S).sum(1) / (n * S * rng * rng)
    assert tuple(r.mse_normalised.shape) == (3,)
    _close(r.mse_normalised.cpu().numpy(), want_mse, SUM_TOL, "mse_normalised")
    # ... which is the training loss of the last rows: ((y - label)^2).mean() per horizon, in normalised units
    y = (pred.astype(np.float64) - wind[0]) / rng
    lab = labels[:, -1, :].astype(np.float64)
    _close(r.mse_normalised.cpu().numpy(), ((y - lab) ** 2).reshape(n, 3, S).mean(axis=(0, 2)), 1e-6, "mse vs the loss's form")
    assert np.array_equal(ev.errors().cpu().numpy().view(np.int32), orc["abs_err"].view(np.int32))
    one, two, three = ev.frames(["st%d" % i for i in range(S)])
    assert np.array_equal(two.to_numpy(), r.stats[1].cpu().numpy(), equal_nan=True) and list(one.index)[:2] == ["st0", "st1"]
    ev.reset()
    assert not bool(ev.acc.view(torch.int64).any()) and tuple(ev.errors().shape) == (0, 102)
    assert ev.compute().stats.isnan().all() and int(ev.compute().count) == 0
    ev.update(*batches[0])                                                 # and it accumulates again from empty
    first = _oracle(preds[0], labels[:preds[0].shape[0]], *wind)
    _close(ev.compute().stats.view(102, 4).cpu().numpy(), first["stats"], STAT_TOL, "after reset")


# ------------------------------------------------------------------------------------------------------------ data parallel
def _evaluate(rank, world, port, out_dir, tag, shards):
    """Evaluate fixture f3's 4 windows split as `shards` (windows per rank) and save compute()'s header and stats."""
    from windgnn_amd.distributed import ensure_rccl_env
    ensure_rccl_env()
    from windgnn_amd import Evaluator
    group = None
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        group = dist.group.WORLD
    dev = torch.device("cuda:0")
    fx = load_fixture("f3_s34_t24_b4_ckpt")
    A, X, L = (torch.from_numpy(fx[k]).to(dev) for k in ("A", "X", "L"))
    ev = Evaluator(_model(fx, "f16x3", dev), A, *WINDS[1], process_group=group)
    for round_, split in enumerate(shards):
        lo = sum(split[:rank])
        hi = lo + split[rank]
        ev.reset()
        ev.update(X[lo:hi].contiguous(), L[lo:hi].contiguous())           # (no windows on this rank: a no-op)
        r = ev.compute()
        local_n = int(ev.acc[0])
        assert local_n == hi - lo, "compute() changed the local accumulator"
        torch.cuda.synchronize()
        np.save(os.path.join(out_dir, "hdr_%s_%d_rank%d.npy" % (tag, round_, rank)), r.header.cpu().numpy())
        np.save(os.path.join(out_dir, "stats_%s_%d_rank%d.npy" % (tag, round_, rank)), r.stats.cpu().numpy())
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


def test_two_rank_evaluation_equals_single_process(tmp_path):
    """Two gloo ranks on cuda:0 over shards of 3 + 1 and then 4 + 0 windows: compute() on both ranks is the single-process
    result (n exact, sums relative 1e-12; the stats kernel then sees the same header), and the empty rank neither hangs nor
    raises."""
    out = str(tmp_path)
    _evaluate(0, 1, 0, out, "ref", [(4,)])
    mp.spawn(_evaluate, args=(2, _free_port(), out, "world2", [(3, 1), (4, 0)]), nprocs=2, join=True)
    h1 = np.load(os.path.join(out, "hdr_ref_0_rank0.npy"))
    s1 = np.load(os.path.join(out, "stats_ref_0_rank0.npy"))
    assert (h1[0] == 4).all() and np.isfinite(s1).all()
    for round_ in (0, 1):
        got = []
        for rank in (0, 1):
            h2 = np.load(os.path.join(out, "hdr_world2_%d_rank%d.npy" % (round_, rank)))
            s2 = np.load(os.path.join(out, "stats_world2_%d_rank%d.npy" % (round_, rank)))
            assert np.array_equal(h2[0], h1[0]), (round_, rank)
            _close(h2[1:], h1[1:], MERGE_TOL, "round %d rank %d header" % (round_, rank))
            _close(s2.reshape(102, 4), s1.reshape(102, 4), STAT_TOL, "round %d rank %d stats" % (round_, rank))
            got.append((h2, s2))
        assert np.array_equal(got[0][0], got[1][0]) and np.array_equal(got[0][1], got[1][1])   # both ranks, to the bit
    # 4 + 0: rank 0 holds everything, so the merged header IS the single-process one
    assert np.array_equal(np.load(os.path.join(out, "hdr_world2_1_rank0.npy")), h1)
