"""The blocked gradient exchange on the GPU: wgnn_bwd_rows / wgnn_finish_rows against part 4 and wgnn_finish bit for bit,
TrainStep(grad_blocks=k) against the one-bucket schedule (one RCCL rank: bitwise; gloo with 2 and 3 ranks: against the
single-process big batch), and the ordering hazard of the blocked Adam (it must come after part 2).

Shape: a reduced configs[4] -- CSR graph, S = 200, H = 600 (the wide-GRU path), T = 6, B = 8."""
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import max_abs

pytestmark = pytest.mark.gpu

S, H, T, B = 200, 600, 6, 8
MODES = ("f32", "f16x3", "f16x3g")
MATH = {"f32": 0, "f16x3": 1, "f16x3g": 3}          # windgnn_amd._lib.MATH_*


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _graph(dev):
    from windgnn_amd.graph import CsrAdjacency, build_knn_adjacency, synthetic_station_coords
    return CsrAdjacency(*build_knn_adjacency(synthetic_station_coords(S, seed=3), 8)).to(dev)


def _data(n, seed=1):
    g = torch.Generator().manual_seed(seed)
    return torch.rand(n, T, S, 13, generator=g), torch.rand(n, T, H, generator=g)


def _model(math, dev):
    from windgnn_amd import GCN_GRU
    torch.manual_seed(0)
    return GCN_GRU(13, 13, 13, S * 13, H, math=math).to(dev)


def _state(tr):
    """Everything a step leaves behind, as host arrays: parameters, both moments, the prepared W_ih images."""
    torch.cuda.synchronize()
    out = {"p": tr.flat_p.cpu().numpy().copy(), "m": tr.exp_avg.cpu().numpy().copy(),
           "v": tr.exp_avg_sq.cpu().numpy().copy()}
    if tr._prepared is not None:
        out["img"] = tr._prepared.cpu().numpy().copy()
    return out


# ---------------------------------------------------------------------------------------------------------------- the ABI
@pytest.mark.parametrize("mode", MODES)
def test_row_ranges_equal_part4_and_finish_bit_for_bit(mode):
    """Row blocks of wgnn_bwd_rows give part 4's gradients, and wgnn_finish_rows over them (then the conv tensors' Adam)
    gives wgnn_finish(0, adam)'s parameters, moments and images -- which are wgnn_prepare_weights' images of the new
    weights."""
    from windgnn_amd import _lib
    from windgnn_amd.distributed import _row_blocks
    from windgnn_amd.functional import (bwd_rows, finish_rows, finish_step, gcn_gru_backward_mse_raw, gcn_gru_forward_raw,
                                        prepared_weights, rows_align)
    dev = torch.device("cuda:0")
    A = _graph(dev)
    X, L = (t.to(dev) for t in _data(B))
    params = [p.detach().clone() for p in _model(mode, dev).hot_path_parameters()]
    Y, stash, d = gcn_gru_forward_raw(A, X, params, MATH[mode], labels=L)
    align = rows_align(d)
    assert align > 0 and align % 8 == 0
    loss = torch.zeros((), device=dev)
    g_ref = [torch.full_like(p, float("nan")) for p in params]
    gcn_gru_backward_mse_raw(d, A, X, params, Y, L, stash, g_ref, loss, 1.0, part=1 | 8)
    gcn_gru_backward_mse_raw(d, A, X, params, Y, L, stash, g_ref, loss, 1.0, part=2)
    gcn_gru_backward_mse_raw(d, A, X, params, Y, L, stash, g_ref, loss, 1.0, part=4)   # part 1's output is still there
    G3 = 3 * H
    for k in (2, 7):
        blocks = _row_blocks(G3, k, align)
        assert blocks[0][0] == 0 and blocks[-1][1] == G3
        g_blk = [g.clone() for g in g_ref[:4]] + [torch.full_like(g, float("nan")) for g in g_ref[4:]]
        for which in (_lib.ROWS_IH, _lib.ROWS_HH):
            for r0, r1 in blocks:
                bwd_rows(d, Y, stash, g_blk, which, r0, r1 - r0)
        torch.cuda.synchronize()
        for t in range(4, 8):
            assert torch.equal(g_blk[t], g_ref[t]), (mode, k, t)

    # Adam: the whole-tensor launch against row ranges + the conv tensors' launch, from the same state
    def adam_state():
        torch.manual_seed(2)
        m = [torch.rand_like(p) * 1e-3 for p in params]
        v = [torch.rand_like(p) * 1e-6 for p in params]
        return dict(exp_avg=m, exp_avg_sq=v, step=3, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
    p1, p2 = [p.clone() for p in params], [p.clone() for p in params]
    a1, a2 = adam_state(), adam_state()
    pre1, pre2 = prepared_weights(d, p1, dev), prepared_weights(d, p2, dev)
    assert (pre1 is None) == (mode == "f32")
    finish_step(d, p1, g_ref, 0, a1, pre1, dev)
    for which in (_lib.ROWS_HH, _lib.ROWS_IH):
        for r0, r1 in reversed(_row_blocks(G3, 7, align)):          # any order: the ranges are disjoint
            finish_rows(d, p2, g_ref, which, r0, r1 - r0, a2, pre2, dev)
    finish_step(d, p2, g_ref, _lib.FINISH_ADAM_CONV, a2, pre2, dev)
    torch.cuda.synchronize()
    for t in range(8):
        assert torch.equal(p1[t], p2[t]), (mode, "param", t)
        assert torch.equal(a1["exp_avg"][t], a2["exp_avg"][t]), (mode, "exp_avg", t)
        assert torch.equal(a1["exp_avg_sq"][t], a2["exp_avg_sq"][t]), (mode, "exp_avg_sq", t)
    assert not torch.equal(p2[4], params[4])                          # the step moved the weights
    if pre1 is not None:
        assert torch.equal(pre1, pre2), mode
        assert torch.equal(pre2, prepared_weights(d, p2, dev)), mode


def test_row_ranges_refuse_bad_rows_and_unsupported_shapes():
    from windgnn_amd import _lib
    from windgnn_amd.functional import bwd_rows, finish_rows, gcn_gru_backward_mse_raw, gcn_gru_forward_raw, rows_align
    dev = torch.device("cuda:0")
    A = _graph(dev)
    X, L = (t.to(dev) for t in _data(B))
    params = [p.detach().clone() for p in _model("f16x3", dev).hot_path_parameters()]
    Y, stash, d = gcn_gru_forward_raw(A, X, params, MATH["f16x3"], labels=L)
    grads = [torch.zeros_like(p) for p in params]
    gcn_gru_backward_mse_raw(d, A, X, params, Y, L, stash, grads, torch.zeros((), device=dev), 1.0, part=1 | 8)
    al = rows_align(d)
    adam = dict(exp_avg=[torch.zeros_like(p) for p in params], exp_avg_sq=[torch.zeros_like(p) for p in params], step=1,
                lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
    for r0, n, code in ((8, al, -2), (al, al + 8, -2), (3 * H, 1, -2), (-al, al, -2), (0, 0, -2), (0, 3 * H + 1, -2)):
        for which in (_lib.ROWS_IH, _lib.ROWS_HH):
            with pytest.raises(RuntimeError, match="status %d" % code):
                bwd_rows(d, Y, stash, grads, which, r0, n)
            with pytest.raises(RuntimeError, match="status %d" % code):
                finish_rows(d, params, grads, which, r0, n, adam)
    with pytest.raises(RuntimeError, match="status -5"):
        bwd_rows(d, Y, stash, grads, _lib.ROWS_HH | _lib.ROWS_STATE, 0, al)
    # the register-resident recurrence (S = 34, H = 102): refused, and no alignment
    d34 = _lib.Dims(B, T, 34, 13, 102, _lib.MATH_F16X3, _lib.ADJ_DENSE, 0, _lib.IO_F32)
    assert rows_align(d34) == 0
    with pytest.raises(RuntimeError, match="status -5"):
        bwd_rows(d34, Y, stash, grads, _lib.ROWS_IH, 0, 306)
    torch.cuda.synchronize()
    assert torch.count_nonzero(grads[4]) == 0 and torch.count_nonzero(grads[5]) == 0     # nothing was launched


# ------------------------------------------------------------------------------------------------ TrainStep, one RCCL rank
def _one_rank(rank, port, out_dir):
    from windgnn_amd.distributed import ensure_rccl_env
    ensure_rccl_env()
    from windgnn_amd.trainer import TrainStep
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    torch.cuda.set_device(0)
    dev = torch.device("cuda:0")
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=dev)
    A = _graph(dev)
    X, L = (t.to(dev) for t in _data(B))
    for mode in MODES:
        for k in (None, 2, 7):
            tr = TrainStep(_model(mode, dev), process_group=dist.group.WORLD, grad_blocks=k)
            assert (tr.plan is None) == (k is None)
            losses = [float(tr.step(A, X, L)[0]) for _ in range(3)]
            st = _state(tr)
            st["loss"] = np.array(losses)
            np.savez(os.path.join(out_dir, "%s_%s.npz" % (mode, k)), **st)
            del tr
    dist.barrier()
    dist.destroy_process_group()


def test_grad_blocks_one_rccl_rank_is_the_one_bucket_step_bit_for_bit(tmp_path):
    """3 steps with grad_blocks = 2 and 7 against the default one-bucket schedule, one-rank RCCL group (a one-rank sum is the
    identity): parameters, both moments, losses and the prepared images identical, in every supported math mode."""
    mp.spawn(_one_rank, args=(_free_port(), str(tmp_path)), nprocs=1, join=True)
    for mode in MODES:
        ref = np.load(os.path.join(str(tmp_path), "%s_None.npz" % mode))
        for k in (2, 7):
            got = np.load(os.path.join(str(tmp_path), "%s_%d.npz" % (mode, k)))
            assert sorted(ref.files) == sorted(got.files)
            for key in ref.files:
                assert np.array_equal(ref[key], got[key]), (mode, k, key)


# ------------------------------------------------------------------------------------------------ gloo, 2 and 3 ranks
def _multi(rank, world, port, out_dir, batches, k, tag):
    from windgnn_amd.distributed import shard_windows
    from windgnn_amd.trainer import TrainStep
    group = None
    if world > 1:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        group = dist.group.WORLD
    dev = torch.device("cuda:0")
    A = _graph(dev)
    X, L = _data(max(batches))
    tr = TrainStep(_model("f32", dev), process_group=group, grad_blocks=k if world > 1 else None)
    if world > 1:
        tr.exchange.record = []
    losses = []
    for n_glob in batches:
        Xs, Ls = shard_windows(X[:n_glob], L[:n_glob], rank, world)
        losses.append(float(tr.step(A, Xs.to(dev), Ls.to(dev))[0]))
    torch.cuda.synchronize()
    np.save(os.path.join(out_dir, "p_%s_rank%d.npy" % (tag, rank)), tr.flat_p.cpu().numpy())
    np.save(os.path.join(out_dir, "loss_%s_rank%d.npy" % (tag, rank)), np.array(losses))
    if world > 1:
        np.save(os.path.join(out_dir, "rec_%s_rank%d.npy" % (tag, rank)), np.array(tr.exchange.record))
        dist.barrier()
        dist.destroy_process_group()


@pytest.mark.parametrize("world", [2, 3])
def test_grad_blocks_multi_rank_equals_the_big_batch(tmp_path, world):
    """gloo ranks on the one GPU, grad_blocks = 3: equal (8), unequal (7) and empty-shard (2 windows over 3 ranks) global
    batches.  Losses and parameters match the single-process big-batch run, and every rank issued the same collectives."""
    sched = (8, 7, 2)
    _multi(0, 1, 0, str(tmp_path), sched, None, "ref")
    mp.spawn(_multi, args=(world, _free_port(), str(tmp_path), sched, 3, "w%d" % world), nprocs=world, join=True)
    p1 = torch.from_numpy(np.load(os.path.join(str(tmp_path), "p_ref_rank0.npy")))
    l1 = np.load(os.path.join(str(tmp_path), "loss_ref_rank0.npy"))
    from windgnn_amd.distributed import grad_block_plan
    rec0 = np.load(os.path.join(str(tmp_path), "rec_w%d_rank0.npy" % world))
    plan = grad_block_plan(S, H, 3, 128)                               # f32: 3 blocks of w_ih, 1 of w_hh
    assert len(plan.blocks) == 4
    assert rec0.tolist() == ([[b.offset, b.numel] for b in plan.blocks] +
                                                                             [list(plan.tail)]) * len(sched)
    for r in range(world):
        p2 = torch.from_numpy(np.load(os.path.join(str(tmp_path), "p_w%d_rank%d.npy" % (world, r))))
        assert max_abs(p1, p2) <= 3e-5, (world, r)                     # three Adam steps of ~1e-3
        l2 = np.load(os.path.join(str(tmp_path), "loss_w%d_rank%d.npy" % (world, r)))
        assert np.abs(l1 - l2).max() <= 1e-6 * max(1.0, float(np.abs(l1).max())), (world, r)
        assert np.array_equal(rec0, np.load(os.path.join(str(tmp_path), "rec_w%d_rank%d.npy" % (world, r)))), (world, r)


# ------------------------------------------------------------------------------------------------ the ordering hazard
def test_block_adam_before_part2_differs_and_the_schedule_does_not():
    """Part 2 reads W_ih through its W_ih^T image.  A step composed with every block's Adam enqueued BEFORE part 2 must
    differ from the one-bucket step (the test can see the hazard); the blocked schedule's order must equal it bit for bit."""
    from windgnn_amd import _lib
    from windgnn_amd.distributed import _row_blocks
    from windgnn_amd.functional import (bwd_rows, finish_rows, finish_step, gcn_gru_backward_mse_raw, gcn_gru_forward_raw,
                                        prepared_weights, rows_align)
    from windgnn_amd.trainer import TrainStep
    dev = torch.device("cuda:0")
    A = _graph(dev)
    X, L = (t.to(dev) for t in _data(B))
    tr = TrainStep(_model("f16x3", dev))
    tr.step(A, X, L)
    ref = [p.detach().clone() for p in tr.params]

    def composed(adam_first):
        params = [p.detach().clone() for p in _model("f16x3", dev).hot_path_parameters()]
        grads = [torch.zeros_like(p) for p in params]
        adam = dict(exp_avg=[torch.zeros_like(p) for p in params], exp_avg_sq=[torch.zeros_like(p) for p in params],
                    step=1, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
        pre = prepared_weights(_lib.Dims(B, T, S, 13, H, _lib.MATH_F16X3, _lib.ADJ_CSR, A.nnz, _lib.IO_F32), params, dev)
        Y, stash, d = gcn_gru_forward_raw(A, X, params, _lib.MATH_F16X3, labels=L, prepared=pre)
        loss = torch.zeros((), device=dev)
        gcn_gru_backward_mse_raw(d, A, X, params, Y, L, stash, grads, loss, 1.0, part=1 | 8 | _lib.BWD_DEFER, prepared=pre)
        blocks = [(w, r0, r1 - r0) for w in (_lib.ROWS_IH, _lib.ROWS_HH) for r0, r1 in _row_blocks(3 * H, 4, rows_align(d))]
        for w, r0, n in blocks:
            bwd_rows(d, Y, stash, grads, w, r0, n)

        def adam_blocks():
            for w, r0, n in blocks:
                finish_rows(d, params, grads, w, r0, n, adam, pre, dev)
        if adam_first:
            adam_blocks()
        gcn_gru_backward_mse_raw(d, A, X, params, Y, L, stash, grads, loss, 1.0, part=2 | _lib.BWD_DEFER, prepared=pre)
        finish_step(d, params, grads, 2, device=dev)
        if not adam_first:
            adam_blocks()
        finish_step(d, params, grads, _lib.FINISH_ADAM_CONV, adam, pre, dev)
        torch.cuda.synchronize()
        return params

    good, bad = composed(False), composed(True)
    for t in range(8):
        assert torch.equal(good[t], ref[t]), t
    assert not all(torch.equal(bad[t], ref[t]) for t in range(4)), "the early Adam went unseen"
    assert all(torch.equal(bad[t], ref[t]) for t in range(4, 8))      # the GRU tensors' gradients came before either Adam
