"""Host side of the blocked gradient exchange (no GPU): the block planner, BucketExchange's blocked collectives on gloo with
the oracle as compute (world 2 and 3, an empty shard included), the row-range entry points' refusals before any launch, and
TrainStep(grad_blocks=...)'s option checks."""
import ctypes
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PARAM_KEYS, load_fixture


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


# ------------------------------------------------------------------------------------------------------------ the planner
@pytest.mark.parametrize("S,H,k,align", [(7, 21, 1, 8), (7, 21, 2, 8), (7, 21, 5, 16), (200, 600, 2, 320), (200, 600, 7, 320),
                                         (200, 600, 7, 128), (4096, 12288, 16, 320), (34, 102, 3, 1)])
def test_plan_partitions_the_bucket(S, H, k, align):
    from windgnn_amd.distributed import HEADER, LOSS_SLOT, grad_block_plan
    plan = grad_block_plan(S, H, k, align)
    G3, I = 3 * H, S * 13
    sizes = [169, 13, 169, 13, G3 * I, G3 * H, G3, G3]
    assert [n for _, n in plan.slots] == sizes
    assert plan.numel == HEADER + sum(sizes)
    # the tail is [loss | conv | b_ih | b_hh], then the blocks cover the rest exactly, in order, without overlap
    assert plan.tail == (LOSS_SLOT, HEADER - LOSS_SLOT + 364 + 2 * G3)
    assert plan.slots[6][0] == HEADER + 364 and plan.slots[7][0] == HEADER + 364 + G3
    pos = plan.tail[0] + plan.tail[1]
    for name, t, ncols in (("ih", 4, I), ("hh", 5, H)):
        mine = [b for b in plan.blocks if b.tensor == name]
        assert 1 <= len(mine) <= k
        assert len(mine) == min(-(-G3 // align), max(1, round(k * ncols / max(I, H))))   # about equal blocks
        assert mine[0].row0 == 0 and mine[-1].row0 + mine[-1].rows == G3
        assert pos == plan.slots[t][0]
        for b in mine:
            assert b.offset == pos and b.numel == b.rows * ncols and b.rows > 0
            assert b.row0 % align == 0 and ((b.row0 + b.rows) % align == 0 or b.row0 + b.rows == G3)
            pos += b.numel
    assert pos == plan.numel
    names = [b.tensor for b in plan.blocks]
    assert names == ["ih"] * names.count("ih") + ["hh"] * names.count("hh")          # w_ih's blocks first, then w_hh's
    assert plan == grad_block_plan(S, H, k, align)                                     # pure


def test_plan_clamps_k_and_refuses_k_below_one():
    from windgnn_amd.distributed import grad_block_plan
    plan = grad_block_plan(7, 21, 1000, 8)                 # 63 rows in units of 8: 8 blocks per weight
    assert len(plan.blocks) == 16
    assert len(grad_block_plan(7, 21, 1000, 1).blocks) == 2 * 63
    assert [b.tensor for b in grad_block_plan(7, 21, 4, 1).blocks] == ["ih"] * 4 + ["hh"] * 1     # 91 vs 21 columns
    assert len(grad_block_plan(7, 21, 3, 64).blocks) == 2  # one unit of rows: one block per weight
    for bad in (0, -1, 2.0, True, "4"):
        with pytest.raises(ValueError):
            grad_block_plan(7, 21, bad, 8)
    with pytest.raises(ValueError):
        grad_block_plan(7, 21, 2, 0)


# ------------------------------------------------------------------------------------------- blocked collectives on gloo
def _worker(rank, world, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
    dist.init_process_group("gloo", rank=rank, world_size=world)
    torch.set_num_threads(2)
    from oracle import windgnn_oracle as orc
    from windgnn_amd import distributed as wd
    fx = load_fixture("f2_s7_t12_b32_ckpt")
    A, X, L = (torch.from_numpy(fx[k]) for k in ("A", "X", "L"))
    p = {k: v.clone() for k, v in fx["params"].items()}
    plan = wd.grad_block_plan(7, 21, 3, 8)
    blocked = torch.zeros(plan.numel)
    whole = torch.zeros(plan.numel)
    ex = wd.BucketExchange(blocked, 364)
    ex.record = []
    ref = wd.BucketExchange(whole, 364)
    # global batches of 32 and 31 windows, then 2 (world 3: shards 1, 1, 0 -- an empty shard issues every collective too)
    for step, n_glob in enumerate((32, 31, 2)):
        Xs, Ls = wd.shard_windows(X[:n_glob], L[:n_glob], rank, world)
        w = ex.shard_weight(Xs.shape[0], n_glob)
        blocked.zero_()
        if Xs.shape[0] > 0:
            Y, cache = orc.forward(A, Xs, p)
            loss_local, dY = orc.mse_loss_and_grad(Y, Ls)
            grads = orc.backward(A, Xs, p, Y, cache, dY * w)
            blocked[wd.LOSS_SLOT] = loss_local
            for (o, n), key in zip(plan.slots, PARAM_KEYS):
                blocked[o:o + n] = grads[key].reshape(-1)
        whole.copy_(blocked)
        works = [ex.start_block(b) for b in plan.blocks]
        tail = ex.start_tail(plan, w)
        tail.wait()
        for work in works:
            work.wait()
        ref.all_reduce_all(w)                                   # the one-bucket form on the same data
        np.save(os.path.join(out_dir, "blocked_%d_rank%d.npy" % (step, rank)), blocked.numpy())
        np.save(os.path.join(out_dir, "whole_%d_rank%d.npy" % (step, rank)), whole.numpy())
    np.save(os.path.join(out_dir, "record_rank%d.npy" % rank), np.array(ex.record))
    dist.barrier()
    dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_blocked_exchange_equals_one_all_reduce(tmp_path, world):
    from windgnn_amd import distributed as wd
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    plan = wd.grad_block_plan(7, 21, 3, 8)
    rec0 = np.load(os.path.join(str(tmp_path), "record_rank0.npy"))
    want = [(b.offset, b.numel) for b in plan.blocks] + [plan.tail]
    assert rec0.tolist() == [list(x) for x in want] * 3         # the plan's slices, in plan order, the tail last, every step
    for r in range(world):
        assert np.array_equal(rec0, np.load(os.path.join(str(tmp_path), "record_rank%d.npy" % r))), r
        for step in range(3):
            b = np.load(os.path.join(str(tmp_path), "blocked_%d_rank%d.npy" % (step, r)))
            w = np.load(os.path.join(str(tmp_path), "whole_%d_rank%d.npy" % (step, r)))
            assert np.abs(b - w).max() <= 1e-6 * np.abs(w).max(), (step, r)
            assert np.array_equal(b[:wd.LOSS_SLOT], np.zeros(wd.LOSS_SLOT))
            assert b[wd.LOSS_SLOT] > 0                          # the big-batch mean loss, on every rank
            if r > 0:
                assert np.array_equal(b, np.load(os.path.join(str(tmp_path), "blocked_%d_rank0.npy" % step))), (step, r)


# --------------------------------------------------------------------------------------- the entry points, before a launch
def _dims(L, S=200, H=600, math=1, fmt=1, nnz=1600):
    return L.Dims(8, 6, S, 13, H, math, fmt, nnz, 0)


def test_row_entry_points_refuse_before_any_launch():
    from windgnn_amd import _lib as L
    lib = L.load()
    V = ctypes.c_void_p
    g, p, ad = L.Grads(), L.Params(), L.Adam()
    for i, n in enumerate(L._SLOTS):
        setattr(g, n, 0x9000000 + 0x100000 * i)
        setattr(p, n, 0x1000 + 0x100000 * i)
    ad.step = 1
    Y, stash, ws = V(0x4000000), V(0xA000000), V(0xE000000)
    big = 1 << 40
    assert lib.wgnn_bwd_rows_align(ctypes.byref(_dims(L, math=1))) == 320         # the TN GEMM's M tile
    assert lib.wgnn_bwd_rows_align(ctypes.byref(_dims(L, math=3))) == 320
    assert lib.wgnn_bwd_rows_align(ctypes.byref(_dims(L, math=0))) == 128
    assert lib.wgnn_bwd_rows_align(ctypes.byref(_dims(L, math=2))) == 0           # one-pass fp16: not offered
    assert lib.wgnn_bwd_rows_align(ctypes.byref(_dims(L, S=34, H=102, fmt=0, nnz=0))) == 0   # register-resident GRU
    assert lib.wgnn_bwd_rows_align(ctypes.byref(_dims(L, S=0))) == 0

    def both(d, which, r0, n):
        a = lib.wgnn_bwd_rows(ctypes.byref(d), Y, stash, ctypes.byref(g), which, r0, n, ws, big, None)
        b = lib.wgnn_finish_rows(ctypes.byref(d), ctypes.byref(p), ctypes.byref(g), which, r0, n, ctypes.byref(ad), ws, big,
                                 None)
        return a, b
    d = _dims(L)
    for r0, n in ((8, 320), (320, 328), (1800, 1), (-320, 320), (0, 0), (0, 1801), (1600, 100)):
        for which in (L.ROWS_IH, L.ROWS_HH):
            assert both(d, which, r0, n) == (-2, -2), (r0, n, which)
    for which in (0, 3, 8, L.ROWS_STATE):
        assert both(d, which, 0, 320) == (-2, -2), which
    assert both(d, L.ROWS_HH | L.ROWS_STATE, 0, 320) == (-5, -5)                 # the state stash
    assert both(_dims(L, S=34, H=102, fmt=0, nnz=0), L.ROWS_IH, 0, 306) == (-5, -5)
    assert both(_dims(L, math=2), L.ROWS_IH, 0, 320) == (-5, -5)
    assert both(_dims(L, math=0), L.ROWS_IH, 64, 128) == (-2, -2)                 # f32: multiples of 128
    # small workspace, null pointers
    d = _dims(L)
    assert lib.wgnn_bwd_rows(ctypes.byref(d), Y, stash, ctypes.byref(g), L.ROWS_IH, 0, 320, ws, 1024, None) == -4
    assert lib.wgnn_bwd_rows(ctypes.byref(d), None, stash, ctypes.byref(g), L.ROWS_IH, 0, 320, ws, big, None) == -1
    assert lib.wgnn_finish_rows(ctypes.byref(d), ctypes.byref(p), ctypes.byref(g), L.ROWS_IH, 0, 320, None, ws, big,
                                None) == -1
    ad.step = 0
    assert lib.wgnn_finish_rows(ctypes.byref(d), ctypes.byref(p), ctypes.byref(g), L.ROWS_IH, 0, 320, ctypes.byref(ad), ws,
                                big, None) == -2


# ------------------------------------------------------------------------------------------------- TrainStep's option checks
def test_trainstep_grad_blocks_needs_a_process_group():
    from windgnn_amd import GCN_GRU
    from windgnn_amd.trainer import TrainStep
    with pytest.raises(RuntimeError, match="process group"):
        TrainStep(GCN_GRU(13, 13, 13, 7 * 13, 200), grad_blocks=2)
    with pytest.raises(ValueError):
        TrainStep(GCN_GRU(13, 13, 13, 7 * 13, 200), grad_blocks="many")


def _options_worker(rank, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    dist.init_process_group("gloo", rank=0, world_size=1)
    from windgnn_amd import GCN_GRU
    from windgnn_amd.trainer import TrainStep
    grp = dist.group.WORLD
    out = []
    for kw in (dict(carry_state=True), dict(overlap_collectives=True), dict(direct_rccl=True)):
        try:
            TrainStep(GCN_GRU(13, 13, 13, 7 * 13, 200), process_group=grp, grad_blocks=2, **kw)
            out.append("accepted")
        except RuntimeError as e:
            out.append(str(e))
    for H, math, k in ((102, "f16x3", 2), (200, "f16", 2), (128, "f32", 2)):
        try:
            TrainStep(GCN_GRU(13, 13, 13, 7 * 13, H, math=math), process_group=grp, grad_blocks=k)
            out.append("accepted")
        except RuntimeError as e:
            out.append(str(e))
    auto_small = TrainStep(GCN_GRU(13, 13, 13, 7 * 13, 200), process_group=grp, grad_blocks="auto")   # 0.9 MB: one bucket
    auto_reg = TrainStep(GCN_GRU(13, 13, 13, 7 * 13, 102), process_group=grp, grad_blocks="auto")
    blocked = TrainStep(GCN_GRU(13, 13, 13, 7 * 13, 200), process_group=grp, grad_blocks=100)
    out.append(repr((auto_small.plan, auto_reg.plan, len(blocked.plan.blocks),
                     [tuple(g.shape) for g in blocked.g_views] == [tuple(q.shape) for q in blocked.params])))
    with open(os.path.join(out_dir, "options.txt"), "w") as f:
        f.write("\n".join(out))
    dist.destroy_process_group()


def test_trainstep_grad_blocks_option_checks(tmp_path):
    mp.spawn(_options_worker, args=(_free_port(), str(tmp_path)), nprocs=1, join=True)
    lines = open(os.path.join(str(tmp_path), "options.txt")).read().split("\n")
    assert "carry_state" in lines[0]
    assert "overlap_collectives" in lines[1]
    assert "direct_rccl" in lines[2]
    for line in lines[3:6]:
        assert "wide-GRU path" in line, line
    assert lines[6] == repr((None, None, 2 * 5, True))      # H = 200 in f32: 600 rows in units of 128 -> 5 per weight
