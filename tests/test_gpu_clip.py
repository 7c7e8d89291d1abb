"""Clipping by the global gradient norm inside the step tail, on the MI355X (include/windgnn_optim.h): wgnn_finish_norm's
reduction against wgnn_finish's bit for bit, its norm against the fp64 norm of the library's own gradients, an inactive clip
against wgnn_finish(adam) bit for bit, an active one against the flat Adam on g * coef, TrainStep(max_grad_norm) against an fp64
loop with clip_grad_norm_ + torch.optim.Adam, two ranks against one, and the footprint of the two entry points."""
import ctypes as C
import functools
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import PARAM_KEYS, load_fixture, max_abs, rel_to_max
from guarded import FILLS

pytestmark = pytest.mark.gpu

MATH = {"f32": 0, "f16x3": 1, "f16": 2, "f16x3g": 3}
# the smallest shapes that reach each partial layout of csrc/finish.hip (tests/test_gpu_parity.py's finish test): pgemm_tn's
# layout and plain [z][M][N], the wide GRU, CSR, the wide image stores, and B*T >= 4096 (the LDS-DMA fp32 GEMMs' pitch, f16x3g's
# single plane)
SHAPES = [(7, 12, 32, 21, False), (5, 3, 17, 9, False), (20, 4, 6, 200, False), (100, 3, 4, 60, True), (8, 5, 9, 12, False),
          (34, 24, 256, 102, False)]
NORM_TOL = 1e-5       # fp32 squares + pairwise fp32 sums: <= (log2 N + 2) 2^-24 ~ 2e-6 for N <= 2^32, halved by the square root;
#                       the rest is room for the short sequential runs per thread (4 values) and per block


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _fp64_norm(tensors):
    return float(torch.sqrt(sum((t.detach().double() ** 2).sum() for t in tensors)))


# ------------------------------------------------------------------------------------------------------------ kernel level
@pytest.mark.parametrize("math", ["f32", "f16x3", "f16x3g", "f16"])
@pytest.mark.parametrize("S,T,B,H,csr", SHAPES)
def test_finish_norm_and_finish_clipped_against_finish(S, T, B, H, csr, math):
    from oracle import windgnn_oracle as orc
    from windgnn_amd import _lib
    from windgnn_amd.functional import (adam_step_, check_range_status, clip_buffer, finish_clipped, finish_norm, finish_step,
                                        gcn_gru_backward_mse_raw, gcn_gru_forward_raw, prepared_weights)
    from windgnn_amd.graph import CsrAdjacency, build_knn_adjacency, synthetic_station_coords
    dev = _dev()
    g = torch.Generator().manual_seed(31 * S + H)
    if csr:
        A = CsrAdjacency(*build_knn_adjacency(synthetic_station_coords(S, seed=3), 6)).to(dev)
    else:
        A = (torch.rand(S, S, generator=g) / S + 0.01).to(dev)
    X = torch.rand(B, T, S, 13, generator=g).to(dev)
    L = torch.rand(B, T, H, generator=g).to(dev)
    p0 = orc.init_params(S, 13, H, seed=S + H)
    mode = MATH[math]
    hyper = dict(step=3, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)
    DEFER = _lib.BWD_DEFER

    def fresh():
        ps = [p0[k].clone().to(dev) for k in PARAM_KEYS]
        gg = torch.Generator().manual_seed(5)
        ms = [(torch.rand(q.shape, generator=gg) * 1e-3).to(dev) for q in ps]       # a mid-training optimiser state
        vs = [(torch.rand(q.shape, generator=gg) * 1e-6).to(dev) for q in ps]
        return ps, [torch.full_like(q, 7.0) for q in ps], ms, vs

    def run(tail, parts=False):
        """Forward, deferred backward (as 7, or as 1 | 4 then 2 with the tail's two reductions in between), then tail(...)."""
        ps, gs, ms, vs = fresh()
        loss = torch.zeros((), device=dev)
        Y, stash, d = gcn_gru_forward_raw(A, X, ps, mode, labels=L)
        img = prepared_weights(d, ps, dev)
        adam = dict(exp_avg=ms, exp_avg_sq=vs, **hyper)
        clip = clip_buffer(d, dev)
        clip.fill_(float("nan"))                                          # clip may be dirty
        if parts:
            gcn_gru_backward_mse_raw(d, A, X, ps, Y, L, stash, gs, loss, 1.0, part=1 | 4 | 8 | DEFER, prepared=img)
            finish_norm(d, gs, 4, float("inf"), clip)
            gcn_gru_backward_mse_raw(d, A, X, ps, Y, L, stash, gs, loss, 1.0, part=2 | DEFER, prepared=img)
            finish_norm(d, gs, 2, float("inf"), clip)
        else:
            gcn_gru_backward_mse_raw(d, A, X, ps, Y, L, stash, gs, loss, 1.0, part=7 | 8 | DEFER, prepared=img)
        out = tail(d, ps, gs, adam, img, clip)
        return dict(d=d, p=ps, g=gs, m=ms, v=vs, img=img, clip=clip, out=out)

    ref = run(lambda d, ps, gs, adam, img, clip: finish_step(d, ps, gs, 6, adam, img))     # wgnn_finish(6, adam)

    def same_state(r, what):
        for k, a, b in zip(PARAM_KEYS * 3, r["p"] + r["m"] + r["v"], ref["p"] + ref["m"] + ref["v"]):
            assert torch.equal(a, b), (what, k)
        assert (r["img"] is None and ref["img"] is None) or torch.equal(r["img"], ref["img"]), what

    # 1. the reduce half is wgnn_finish's, bit for bit; 2. the norm
    reduced = run(lambda d, ps, gs, adam, img, clip: finish_step(d, ps, gs, 6))           # wgnn_finish(6, NULL): reduce only
    for k, a, b in zip(PARAM_KEYS, reduced["g"], ref["g"]):
        assert torch.equal(a, b), k
    totals = []

    def measure(d, ps, gs, adam, img, clip):
        finish_norm(d, gs, 6, float("inf"), clip)
        return clip[:2].clone()
    for _ in range(2):
        r = run(measure)
        for k, a, b in zip(PARAM_KEYS, r["g"], reduced["g"]):
            assert torch.equal(a, b), k
        totals.append(r["out"][0].view(torch.int32).item())
        assert float(r["out"][1]) == 1.0
    assert totals[0] == totals[1], "two runs on identical inputs gave different norms"
    total = float(r["out"][0])
    want = _fp64_norm(ref["g"])
    print("%s S%d T%d B%d H%d: total %.9g, fp64 norm of the fp32 gradients %.9g, rel %.2e"
          % (math, S, T, B, H, total, want, abs(total - want) / want))
    assert want > 0 and abs(total - want) <= NORM_TOL * want
    pure = clip_buffer(r["d"], dev)
    finish_norm(r["d"], r["g"], 0, float("inf"), pure)                    # the data-parallel form: a pure pass over g
    assert abs(float(pure[0]) - want) <= NORM_TOL * want and abs(float(pure[0]) - total) <= NORM_TOL * want
    assert float(pure[1]) == 1.0
    r = run(lambda d, ps, gs, adam, img, clip: clip[:2].clone(), parts=True)      # 4, then 2
    for k, a, b in zip(PARAM_KEYS, r["g"], reduced["g"]):
        assert torch.equal(a, b), ("4 then 2", k)
    assert abs(float(r["out"][0]) - want) <= NORM_TOL * want and float(r["out"][1]) == 1.0

    # 3. an inactive clip is wgnn_finish(adam), bit for bit
    for max_norm in (float("inf"), 1e6):
        def inactive(d, ps, gs, adam, img, clip):
            finish_norm(d, gs, 6, max_norm, clip)
            finish_clipped(d, ps, gs, adam, clip, img)
            return clip[:2].clone()
        r = run(inactive)
        assert float(r["out"][1]) == 1.0 and r["out"][0].view(torch.int32).item() == totals[0]
        same_state(r, "max_norm = %r" % max_norm)
        for k, a, b in zip(PARAM_KEYS, r["g"], ref["g"]):
            assert torch.equal(a, b), k

    # 4. an active clip: Adam on g * coef
    def active(d, ps, gs, adam, img, clip):
        finish_norm(d, gs, 6, total / 8, clip)
        torch.cuda.synchronize()
        before = [q.clone() for q in gs]
        finish_clipped(d, ps, gs, adam, clip, img)
        return clip[:2].clone(), before
    r = run(active)
    (tc, before) = r["out"]
    coef = float(tc[1])
    assert tc[0].view(torch.int32).item() == totals[0]
    assert abs(coef - (total / 8) / (total + 1e-6)) <= 2e-7 and coef < 0.126
    for k, a, b in zip(PARAM_KEYS, r["g"], before):
        assert torch.equal(a, b) and torch.equal(a, ref["g"][PARAM_KEYS.index(k)]), ("g was rewritten", k)
    ps, _, ms, vs = fresh()
    for q, gq, m, v in zip(ps, ref["g"], ms, vs):
        adam_step_(q, gq * tc[1], m, v, hyper["step"], hyper["lr"], hyper["beta1"], hyper["beta2"], hyper["eps"])
    for k, a, b in zip(PARAM_KEYS, r["p"], ps):
        assert max_abs(a.cpu(), b.cpu()) <= 2e-7, k                       # the existing finish test's bars
    for a, b in zip(r["m"] + r["v"], ms + vs):
        assert rel_to_max(a.cpu(), b.cpu()) <= 1e-6
    moved = max(max_abs(a.cpu(), b.cpu()) for a, b in zip(r["m"], ref["m"]))
    assert moved > 0, "the clipped step equals the unclipped one"
    if r["img"] is not None:
        assert torch.equal(r["img"], prepared_weights(r["d"], r["p"], dev))
    check_range_status(dev)


def test_a_nonfinite_norm_is_reported_and_follows_torchs_formula():
    from windgnn_amd import _lib
    from windgnn_amd.functional import check_range_status, clip_buffer, finish_norm
    dev = _dev()
    d = _lib.Dims(2, 3, 5, 13, 9, 0, 0, 0, 0)
    sizes = [169, 13, 169, 13, 27 * 65, 27 * 9, 27, 27]
    gs = [torch.full((n,), 0.5, device=dev) for n in sizes]
    clip = clip_buffer(d, dev)
    finish_norm(d, gs, 0, 2.0, clip)
    want = 0.5 * float(sum(sizes)) ** 0.5
    assert abs(float(clip[0]) - want) <= NORM_TOL * want and abs(float(clip[1]) - 2.0 / (want + 1e-6)) <= 1e-7
    check_range_status(dev)
    gs[5][17] = float("inf")
    finish_norm(d, gs, 0, 2.0, clip)
    assert float(clip[0]) == float("inf") and float(clip[1]) == 0.0
    with pytest.raises(RuntimeError, match="gradient came out inf / NaN"):
        check_range_status(dev)
    gs[5][17] = float("nan")
    finish_norm(d, gs, 0, 2.0, clip)
    assert clip[0].isnan() and clip[1].isnan()                            # torch.clamp(nan, max=1) is nan
    with pytest.raises(RuntimeError, match="gradient came out inf / NaN"):
        check_range_status(dev)


# ---------------------------------------------------------------------------------------------------- trajectories vs torch
def _fp64_model(p):
    """tests/test_gpu_state_train.py's reference: the 8 tensors as fp64 leaves, f(A, X, h0) -> (Y, h_n)."""
    leaves = {k: p[k].double().clone().requires_grad_(True) for k in PARAM_KEYS}

    def f(A, X, h0):
        A, X = A.double(), X.double()
        h = torch.relu(torch.matmul(torch.matmul(A, X), leaves["conv1.weight"]) + leaves["conv1.bias"])
        h = torch.relu(torch.matmul(torch.matmul(A, h), leaves["conv2.weight"]) + leaves["conv2.bias"])
        B, T, S, F = X.shape
        Y, hn = torch._VF.gru(h.reshape(B, T, S * F), h0.unsqueeze(0),
                              [leaves["gru.weight_ih_l0"], leaves["gru.weight_hh_l0"], leaves["gru.bias_ih_l0"],
                               leaves["gru.bias_hh_l0"]], True, 1, 0.0, False, False, True)
        return Y, hn[0]
    return leaves, f


def _fp64_loop(A, p, batches, max_norm, carry, lr=1e-3, eps=1e-3):
    """clip_grad_norm_ + torch.optim.Adam in fp64 over `batches` [(X, L)]: per step (loss, norm before clipping, parameters,
    exp_avg, exp_avg_sq)."""
    leaves, f = _fp64_model(p)
    opt = torch.optim.Adam(list(leaves.values()), lr=lr, eps=eps)
    B, H = batches[0][0].shape[0], p["gru.weight_hh_l0"].shape[1]
    h = torch.zeros(B, H, dtype=torch.float64)
    out = []
    for X, L in batches:
        opt.zero_grad()
        Y, hn = f(A, X, h if carry else torch.zeros(X.shape[0], H, dtype=torch.float64))
        loss = ((Y - L.double()) ** 2).mean()
        loss.backward()
        norm = float(torch.nn.utils.clip_grad_norm_(list(leaves.values()), max_norm))
        opt.step()
        h = hn.detach()
        out.append((float(loss.detach()), norm, {k: v.detach().clone() for k, v in leaves.items()},
                    {k: opt.state[v]["exp_avg"].clone() for k, v in leaves.items()},
                    {k: opt.state[v]["exp_avg_sq"].clone() for k, v in leaves.items()}))
    return out


@functools.lru_cache(maxsize=None)
def _carried_setting():
    """tests/test_gpu_state_train.py's test_trainstep_carry_state_against_fp64_adam: S 34, T 8, B 4, H 102, seed 11, 3 chunks."""
    from oracle import windgnn_oracle as orc
    S, T, B, H, steps = 34, 8, 4, 102, 3
    g = torch.Generator().manual_seed(2000 + S + T + B + H + 11)
    A = torch.rand(S, S, generator=g) / S + 0.01
    torch.rand(B, T, S, 13, generator=g)                                 # (that test's _setup draws an X first)
    p = orc.init_params(S, 13, H, seed=S + H)
    series = torch.rand(B, steps * T + 1, S, 13, generator=g)
    labels = torch.rand(B, steps * T, H, generator=g)
    batches = [(series[:, s * T:(s + 1) * T].contiguous(), labels[:, s * T:(s + 1) * T].contiguous()) for s in range(steps)]
    return A, p, batches


@functools.lru_cache(maxsize=None)
def _carried_reference(max_norm):
    A, p, batches = _carried_setting()
    return _fp64_loop(A, p, batches, max_norm, carry=True)


def _against_reference(tr, m, A, batches, ref, tag):
    dev = _dev()
    names = [k for k, _ in m.named_parameters()]
    assert names == PARAM_KEYS
    for s, ((X, L), (loss_r, norm_r, p_r, m_r, v_r)) in enumerate(zip(batches, ref)):
        loss, _ = tr.step(A.to(dev), X.to(dev), L.to(dev))
        loss, norm, coef = float(loss), float(tr.grad_norm), float(tr.clip_coef)
        print("%s step %d: loss %.8f vs %.8f, norm %.6f vs %.6f, coef %.6f" % (tag, s, loss, loss_r, norm, norm_r, coef))
        assert abs(loss - loss_r) <= 2e-4 * max(1.0, abs(loss_r)), (tag, s, loss, loss_r)
        assert abs(norm - norm_r) <= 1e-4 * norm_r, (tag, s, norm, norm_r)
        assert abs(coef - min(1.0, tr.max_grad_norm / (norm_r + 1e-6))) <= 1e-4, (tag, s, coef)
        for i, (key, prm) in enumerate(m.named_parameters()):
            assert rel_to_max(prm.detach().cpu(), p_r[key]) <= 1e-4, (tag, s, key)
            assert rel_to_max(tr.m_views[i].cpu(), m_r[key]) <= 1e-4, (tag, s, key, "exp_avg")
            assert rel_to_max(tr.v_views[i].cpu(), v_r[key]) <= 2e-4, (tag, s, key, "exp_avg_sq")   # squares: twice the bar


@pytest.mark.parametrize("max_norm", [0.2, 1.9])
@pytest.mark.parametrize("math", ["f32", "f16x3"])
def test_trainstep_carry_state_clipped_against_fp64_clip_grad_norm_and_adam(math, max_norm):
    """TrainStep(carry_state=True, max_grad_norm) over 3 consecutive chunks against clip_grad_norm_ + torch.optim.Adam in fp64.
    0.2 clips every step (the reference's unclipped norms are 2.026, 1.727, 1.662); 1.9 clips the first step only."""
    from windgnn_amd import GCN_GRU
    from windgnn_amd.trainer import TrainStep
    A, p, batches = _carried_setting()
    ref = _carried_reference(max_norm)
    norms = [r[1] for r in ref]
    if max_norm == 0.2:
        assert min(norms) > 1.0                                           # active in all three steps
        free = _carried_reference(float("inf"))
        # a missing or wrong coefficient cannot pass: the unclipped trajectory is far outside the bars below
        assert rel_to_max(free[-1][2]["gru.weight_hh_l0"], ref[-1][2]["gru.weight_hh_l0"]) > 5e-3
        assert rel_to_max(free[-1][2]["conv1.weight"], ref[-1][2]["conv1.weight"]) >= 3e-4
    else:
        assert norms[0] > 1.9 > norms[1] and 1.9 > norms[2], norms        # both branches of min(1, .) are taken
    m = GCN_GRU(13, 13, 13, 34 * 13, 102, math=math).to(_dev())
    m.load_state_dict(p)
    tr = TrainStep(m, lr=1e-3, eps=1e-3, carry_state=True, max_grad_norm=max_norm)
    _against_reference(tr, m, A, batches, ref, "%s max_norm %g" % (math, max_norm))
    tr.check()


@pytest.mark.parametrize("math", ["f32", "f16x3"])
def test_trainstep_clipped_against_fp64_clip_grad_norm_and_adam(math):
    """The non-carried step (wgnn_fwd_loss + wgnn_bwd_mse_part + wgnn_finish_norm(6) + wgnn_finish_clipped) on fixture f2:
    three steps on its 32 windows, max_grad_norm = half the fp64 reference's first unclipped norm."""
    from windgnn_amd import GCN_GRU
    from windgnn_amd.trainer import TrainStep
    fx = load_fixture("f2_s7_t12_b32_ckpt")
    A, X, L = (torch.from_numpy(fx[k]) for k in ("A", "X", "L"))
    p = {k: v.clone() for k, v in fx["params"].items()}
    batches = [(X, L), (X[:17].contiguous(), L[:17].contiguous()), (X, L)]
    free = _fp64_loop(A, p, batches, float("inf"), carry=False)
    max_norm = 0.5 * free[0][1]
    ref = _fp64_loop(A, p, batches, max_norm, carry=False)
    assert ref[0][1] > max_norm
    m = GCN_GRU(13, 13, 13, 7 * 13, 21, math=math).to(_dev())
    m.load_state_dict(p)
    tr = TrainStep(m, lr=1e-3, eps=1e-3, max_grad_norm=max_norm)
    _against_reference(tr, m, A, batches, ref, "f2 %s" % math)
    # the bucket keeps the unclipped gradient: its own norm is the reported one
    assert abs(_fp64_norm(tr.g_views) - float(tr.grad_norm)) <= NORM_TOL * float(tr.grad_norm)


def test_trainstep_without_max_grad_norm_runs_the_unclipped_tail_and_inf_only_measures():
    """max_grad_norm=None launches what it launched before (the library's own per-kernel tally shows one finish_kernel<1> and
    no clip kernel); float('inf') measures and steps to the same bits."""
    from windgnn_amd import GCN_GRU, _lib
    from windgnn_amd.trainer import TrainStep
    dev = _dev()
    fx = load_fixture("f2_s7_t12_b32_ckpt")
    A, X, L = (torch.from_numpy(fx[k]).to(dev) for k in ("A", "X", "L"))

    def trainer(**kw):
        m = GCN_GRU(13, 13, 13, 7 * 13, 21, math="f16x3").to(dev)
        m.load_state_dict({k: v.clone() for k, v in fx["params"].items()})
        return TrainStep(m, **kw)
    plain, watched = trainer(), trainer(max_grad_norm=float("inf"))
    tally = {}
    for name, tr in (("plain", plain), ("watched", watched)):
        tr.step(A, X, L)                                                  # (builds the images outside the tally)
        _lib.profile_enable(True)
        try:
            before = {k["name"]: k["launches"] for k in _lib.profile_read()}
            tr.step(A, X, L)
            after = {k["name"]: k["launches"] for k in _lib.profile_read()}
        finally:
            _lib.profile_enable(False)
        tally[name] = {k: n - before.get(k, 0) for k, n in after.items() if n - before.get(k, 0)}
    print(tally)
    clip_kernels = {"finish_norm_kernel", "clip_coef_kernel", "finish_clipped_kernel"}
    assert tally["plain"]["finish_kernel<1>"] == 1 and not (clip_kernels & set(tally["plain"]))
    assert {k: tally["watched"][k] for k in clip_kernels} == {k: 1 for k in clip_kernels}
    assert "finish_kernel<1>" not in tally["watched"]
    rest = lambda t: {k: n for k, n in t.items() if k not in clip_kernels and k != "finish_kernel<1>"}   # noqa: E731
    assert rest(tally["plain"]) == rest(tally["watched"])
    assert torch.equal(plain.flat_p, watched.flat_p) and torch.equal(plain.exp_avg_sq, watched.exp_avg_sq)
    assert float(watched.clip_coef) == 1.0 and float(watched.grad_norm) > 0


# ------------------------------------------------------------------------------------------------------------ data parallel
def _train(rank, world, port, out_dir, tag, max_norm, explicit=False, batches=(32, 1, 32)):
    from windgnn_amd.distributed import ensure_rccl_env, shard_windows
    ensure_rccl_env()
    from windgnn_amd import GCN_GRU
    from windgnn_amd.trainer import TrainStep
    group = None
    if world > 1 or explicit:
        os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world))
        dist.init_process_group("gloo", rank=rank, world_size=world)
        group = dist.group.WORLD if explicit else None
    dev = torch.device("cuda:0")
    fx = load_fixture("f2_s7_t12_b32_ckpt")
    m = GCN_GRU(13, 13, 13, 7 * 13, 21, math="f16x3")
    m.load_state_dict({k: v.clone() for k, v in fx["params"].items()})
    tr = TrainStep(m.to(dev), process_group=group, max_grad_norm=max_norm)
    assert tr.collective == (world > 1 or explicit)
    A = torch.from_numpy(fx["A"]).to(dev)
    X, L = torch.from_numpy(fx["X"]), torch.from_numpy(fx["L"])
    rows = []
    for n_glob in batches:
        Xs, Ls = shard_windows(X[:n_glob], L[:n_glob], rank, world)
        loss, _ = tr.step(A, Xs.to(dev), Ls.to(dev), n_global=n_glob)
        rows.append((float(loss), float(tr.grad_norm), float(tr.clip_coef), Xs.shape[0]))
    torch.cuda.synchronize()
    np.save(os.path.join(out_dir, "p_%s_rank%d.npy" % (tag, rank)), tr.flat_p.cpu().numpy())
    np.save(os.path.join(out_dir, "rows_%s_rank%d.npy" % (tag, rank)), np.array(rows, dtype=np.float64))
    if world > 1 or explicit:
        dist.barrier()
        tr.close()
        dist.destroy_process_group()


def test_two_rank_clipped_training_equals_single_process(tmp_path):
    """Two gloo ranks on cuda:0, global batches of 32, 1 and 32 windows (rank 1 is empty in step 2): every rank takes the norm of
    the summed bucket itself, with no further collective, and must land on the single-process clipped run; a one-rank explicit
    group (finish(6), all-reduce, finish_norm(0), finish_clipped) too."""
    out = str(tmp_path)
    _train(0, 1, 0, out, "watch", float("inf"))
    first = np.load(os.path.join(out, "rows_watch_rank0.npy"))[0, 1]
    max_norm = 0.5 * float(first)
    _train(0, 1, 0, out, "ref", max_norm)
    mp.spawn(_train, args=(2, _free_port(), out, "world2", max_norm), nprocs=2, join=True)
    mp.spawn(_train, args=(1, _free_port(), out, "group1", max_norm, True), nprocs=1, join=True)
    p1 = torch.from_numpy(np.load(os.path.join(out, "p_ref_rank0.npy")))
    r1 = np.load(os.path.join(out, "rows_ref_rank0.npy"))
    assert r1[0, 1] == first and abs(r1[0, 2] - max_norm / (first + 1e-6)) <= 1e-6   # active, on the norm that was measured
    for tag, ranks in (("world2", (0, 1)), ("group1", (0,))):
        for rank in ranks:
            p2 = torch.from_numpy(np.load(os.path.join(out, "p_%s_rank%d.npy" % (tag, rank))))
            r2 = np.load(os.path.join(out, "rows_%s_rank%d.npy" % (tag, rank)))
            print(tag, rank, "max|p - p_ref| %.3e" % max_abs(p1, p2), r2.tolist())
            assert max_abs(p1, p2) <= 3e-5, (tag, rank)                  # tests/test_distributed_gpu.py's three-step bar
            assert (np.abs(r1[:, 0] - r2[:, 0]) <= 1e-6 * np.abs(r1[:, 0])).all(), (tag, rank, r1[:, 0], r2[:, 0])   # relative, per step
            assert (np.abs(r1[:, 1] - r2[:, 1]) <= 1e-5 * r1[:, 1]).all(), (tag, rank, r1[:, 1], r2[:, 1])
    w0 = np.load(os.path.join(out, "rows_world2_rank0.npy"))
    w1 = np.load(os.path.join(out, "rows_world2_rank1.npy"))
    assert w1[1, 3] == 0 and w0[1, 3] == 1                               # rank 1 had no windows in step 2
    assert np.array_equal(w0[:, :3], w1[:, :3])                          # the same loss, norm and coefficient on both ranks, to the bit
    assert np.array_equal(np.load(os.path.join(out, "p_world2_rank0.npy")), np.load(os.path.join(out, "p_world2_rank1.npy")))


# ---------------------------------------------------------------------------------------------------------------- footprint
FOOT = {"clip-f16x3": ("f16x3", torch.float32, 7, 12, 32, 21, 0), "clip-f32-wide": ("f32", torch.float32, 20, 4, 6, 200, 0)}


def _clip_flow(r):
    """wgnn_fwd_loss, wgnn_bwd_mse_part(7 | 8 | DEFER), wgnn_finish_norm(6), wgnn_finish_norm(0), wgnn_finish_clipped; `prepared`
    kept where the configuration has images.  max_norm = half the fp64 oracle's norm: the clip is active."""
    lib, d, gs = r.lib, C.byref(r.d), r.grads()
    kept = r.prep_bytes > 0
    ps = r.params("prepared" if kept else None)
    if kept:
        r.ok(lib.wgnn_prepare_weights(d, C.byref(ps), *r.ws), "wgnn_prepare_weights")
        r.repoison_ws()
    r.ok(lib.wgnn_fwd_loss(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("L"), r.ptr("Y"), r.ptr("stash"), *r.ws), "wgnn_fwd_loss")
    r.repoison_ws()
    part = 7 | 8 | r.L.BWD_DEFER
    r.ok(lib.wgnn_bwd_mse_part(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("Y"), r.ptr("L"), C.c_float(1.0), r.ptr("loss"),
                               r.ptr("stash"), C.byref(gs), *r.ws, part), "wgnn_bwd_mse_part(%d)" % part)
    max_norm = C.c_float(0.5 * _fp64_norm(r.c.go.values()))
    r.ok(lib.wgnn_finish_norm(d, C.byref(gs), 6, max_norm, r.ptr("clip"), *r.ws), "wgnn_finish_norm(6)")
    side = r.tstream is not None                     # on a side stream nothing is read back between the calls
    r.heads = [] if side else [r.a["clip"].host()[:8].clone()]
    r.ok(lib.wgnn_finish_norm(d, C.byref(gs), 0, max_norm, r.ptr("clip"), *r.ws), "wgnn_finish_norm(0)")
    if not side:
        r.heads.append(r.a["clip"].host()[:8].clone())
    ad = r.adam()
    r.ok(lib.wgnn_finish_clipped(d, C.byref(ps), C.byref(gs), C.byref(ad), r.ptr("clip"), *r.ws), "wgnn_finish_clipped")
    outs = ["Y", "loss"] + ["g." + k for k in PARAM_KEYS] + [pre + k for pre in ("p.", "m.", "v.") for k in PARAM_KEYS]
    if kept:
        ps2 = r.params("prepared2")                                      # the images of the NEW weights, built from scratch
        r.ok(lib.wgnn_prepare_weights(d, C.byref(ps2), *r.ws), "wgnn_prepare_weights(new weights)")
        outs += ["prepared", "prepared2"]
    return outs


@pytest.mark.parametrize("cid", sorted(FOOT))
def test_footprint_of_finish_norm_and_finish_clipped(cid):
    """tests/test_gpu_footprint.py's method on the two new entry points: every buffer -- clip included -- of its exact ABI
    length inside poisoned guard bands; clip, stash, workspace and outputs start as zeros, finite noise, NaNs and then as the
    bytes another case left behind; the guards stay intact, the status word 0, and every output, clip[0] and clip[1] included,
    is bit-identical across the four."""
    import test_gpu_footprint as fp
    c = fp._build(cid, FOOT[cid])
    L = fp._lib()
    lib = L.load()
    d = L.Dims(c.B, c.T, c.S, 13, c.H, fp.MATH[c.math], 0, 0, 0)
    nclip = lib.wgnn_clip_bytes(C.byref(d))
    assert nclip >= 512 and nclip % 256 == 0
    extra = (("clip", torch.uint8, (nclip,)),)
    poison_free = set(["Y", "loss", "prepared", "prepared2"] + ["g." + k for k in PARAM_KEYS])
    donor = fp._case(fp.DONOR[c.math])
    dd = L.Dims(donor.B, donor.T, donor.S, 13, donor.H, fp.MATH[donor.math], 0, 0, 0)
    rd = fp.Run(donor, "finite", seed=3, extra=(("clip", torch.uint8, (lib.wgnn_clip_bytes(C.byref(dd)),)),))
    _clip_flow(rd)
    torch.cuda.synchronize()
    left = dict(rd.leftovers(), clip=rd.a["clip"].host())
    base = heads = None
    for fill, dirty in [(f, None) for f in FILLS] + [("finite", left)]:
        r = fp.Run(c, fill, dirty=dirty, seed=1 if dirty else 0, extra=extra)
        if dirty:
            r.a["clip"].write(fp._fit(dirty["clip"], nclip))
        res = r.collect(_clip_flow(r), poison_free)
        tag = "%s [%s%s]" % (cid, fill, ", on the leftovers of %s" % donor.id if dirty else "")
        if base is None:
            base, heads = res, r.heads
            total, coef = (float(x) for x in heads[0].view(torch.float32))
            want = _fp64_norm(c.go.values())
            assert abs(total - want) <= 1e-4 * want and abs(coef - 0.5) <= 1e-4, (total, want, coef)   # the suite's G_TOL
            t0 = float(heads[1].view(torch.float32)[0])
            assert abs(t0 - total) <= NORM_TOL * total
            fp._check_Y(r, res)
            fp._check_grads(r, res)                                      # g keeps the unclipped gradient
            for k in PARAM_KEYS:                                         # Adam's first step on g * coef (fp64, from the GPU's g)
                g = r.tensor("g." + k, res).double() * float(heads[1].view(torch.float32)[1])
                assert rel_to_max(r.tensor("m." + k, res), (1 - fp.B1) * g) <= 1e-6, k
                assert rel_to_max(r.tensor("v." + k, res), (1 - fp.B2) * g * g) <= 1e-6, k
            if "prepared" in res:
                assert torch.equal(res["prepared"], res["prepared2"]), "wgnn_finish_clipped did not keep the W_ih images current"
        else:
            fp._same(base, res, tag)
            for a, b in zip(heads, r.heads):
                assert torch.equal(a, b), (tag, "clip[0] / clip[1] differ from the zero-fill run")
