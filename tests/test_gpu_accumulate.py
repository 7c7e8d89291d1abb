"""Gradients accumulated over several calls on the MI355X: TrainStep.accumulate / accumulate_series / apply / discard against the
fp64 oracle's training step on the UNION of the windows (tests/accumulate_cases.py has the shapes and the references;
tests/test_accumulate_host.py the refusals, the call sequences, the weight arithmetic and the ranks over gloo).  Every figure is
printed before it is asserted.

Observed on the MI355X (bar 1e-4 of the tensor's max), worst over three accumulated steps, Y / loss / gradient / parameters:
    small 1 + 2 + 3:  f32 5.4e-7 / 1.6e-7 / 2.9e-7 / 7.8e-7; f16x3 6.2e-7 / 2.6e-7 / 7.9e-7 / 1.1e-6
    real 16 + 4:      f32 1.1e-6 / 6.9e-8 / 5.4e-7 / 2.0e-7; f16x3 3.0e-6 / 1.5e-7 / 1.9e-6 / 4.7e-7
    csr 1 + 2 + 3:    f16x3 1.8e-6 / 1.3e-7 / 1.2e-6 / 2.2e-6
    against forward_backward on the B windows at once (no bar of its own): 2.4e-7 (small f32), 5.3e-7 (real f32), 3.1e-7 (csr)
    one call + apply against step: every bit equal (Y, loss, gradients, parameters, both moments, best record), two steps,
    f32 and f16x3, small and real
    L1 from step 2 / Huber 0.25, cut 1 + 1 + 2: gradients 2.3e-7 / 1.9e-7 (f32), 5.7e-7 / 1.5e-6 (f16x3)
    labels missing at 0 / 10 / 40 % per call: 649 labels, gradient 1.6e-7 of the label-weighted oracle; the window-weighted
    answer is off by 5.4e-2 (loss 2.3e-3)
    two series tensors 1.0e-6; a materialised + a series call 2.6e-6; clipped norms 1.710331 / 1.674478 = the oracle's"""
import os

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import accumulate_cases as ac
import step_loss_cases as sl
from conftest import PARAM_KEYS, rel_to_max

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _model(c, mode):
    from windgnn_amd import GCN_GRU
    m = GCN_GRU(13, 13, 13, c.S * 13, c.H, math=mode, validate=False)
    m.load_state_dict({k: v.clone() for k, v in c.p.items()})
    return m.to(_dev())


def _step(model, **kw):
    from windgnn_amd.trainer import TrainStep
    return TrainStep(model, lr=ac.LR, eps=ac.EPS, **kw)


def _adj(c):
    return c.csr.to(_dev()) if c.csr is not None else c.A.to(_dev())


def _grad_errors(tr, g):
    return {k: rel_to_max(v.detach().cpu(), g[k]) for k, v in zip(PARAM_KEYS, tr.g_views)}


def _param_errors(model, p):
    return {k: rel_to_max(v.detach().cpu(), p[k]) for k, v in model.named_parameters()}


def _bits(t):
    return t.detach().contiguous().view(torch.int32).cpu()


def _accumulate_cut(tr, A, X, L, cut, **kw):
    out = []
    for lo, hi in ac.spans(cut):
        loss, Y = tr.accumulate(A, X[lo:hi], L[lo:hi], **kw)
        assert loss.dim() == 0 and loss.data_ptr() != tr._loss.data_ptr()          # a clone, not the header view
        out.append((loss, Y))
    return out


# ---- 1. against the fp64 oracle on the union ------------------------------------------------------------------------------------------
PARITY = [("small", "f32"), ("small", "f16x3"), ("real", "f32"), ("real", "f16x3"), ("csr", "f16x3")]


@pytest.mark.parametrize("name,mode", PARITY, ids=["%s-%s" % c for c in PARITY])
def test_apply_is_the_oracles_step_on_the_union_of_the_windows(name, mode):
    c = ac.case(name)
    q = ac.union(name, steps=3)
    A, X, L = _adj(c), c.X.to(_dev()), c.L.to(_dev())
    model = _model(c, mode)
    tr = _step(model)
    twin = _step(_model(c, mode))
    worst = {"Y": 0.0, "loss": 0.0, "grad": 0.0, "params": 0.0}
    for s in range(3):
        calls = _accumulate_cut(tr, A, X, L, c.cut)
        assert tr.accumulated == len(c.cut) and int(tr.accumulated_count) == c.B * c.T * c.H and tr.steps == s
        loss = tr.apply()
        assert loss.data_ptr() == tr._loss.data_ptr() and tr.steps == s + 1 and tr.accumulated == 0
        ey = rel_to_max(torch.cat([Y for _, Y in calls]).cpu(), q.Y[s])
        el = abs(float(loss) - q.loss[s]) / q.loss[s]
        eg, ep = _grad_errors(tr, q.g[s]), _param_errors(model, q.p[s])
        print("%s %s step %d: Y %.2e  loss %.2e  worst gradient %.2e  worst parameter %.2e (bar %.1e)"
              % (name, mode, s + 1, ey, el, max(eg.values()), max(ep.values()), ac.TOL))
        worst = {"Y": max(worst["Y"], ey), "loss": max(worst["loss"], el), "grad": max(worst["grad"], max(eg.values())),
                 "params": max(worst["params"], max(ep.values()))}
        if s == 0:                  # against ONE call on the B windows at once: reported, no bar of its own
            l1, _ = twin.forward_backward(A, X, L)
            d = {k: rel_to_max(a.cpu(), b.cpu()) for k, a, b in zip(PARAM_KEYS, tr.g_views, twin.g_views)}
            print("%s %s: the bucket of %s against forward_backward on the %d windows at once: worst %.2e of the tensor's max, "
                  "loss %.8f against %.8f" % (name, mode, " + ".join(map(str, c.cut)), c.B, max(d.values()), float(loss), float(l1)))
            wsum = sum((hi - lo) * float(li) for (lo, hi), (li, _) in zip(ac.spans(c.cut), calls)) / c.B
            assert abs(wsum - float(loss)) <= 1e-6 * float(loss)        # the calls' own losses came back, each a clone
    tr.check()
    print("%s %s: worst over 3 accumulated steps: %s" % (name, mode, "  ".join("%s %.2e" % kv for kv in worst.items())))
    assert max(worst.values()) <= ac.TOL, worst


# ---- 2. one call + apply is the step it replaces ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", PARITY[:4], ids=["%s-%s" % c for c in PARITY[:4]])
def test_one_accumulated_call_is_bit_identical_to_step(name, mode):
    """step reduces its deferred partial sums and steps Adam in ONE wgnn_finish(6, adam); accumulate + apply runs the
    non-deferred backward and wgnn_finish(0, adam): include/windgnn_optim.h promises the same bits from both forms."""
    c = ac.case(name)
    A, X, L = _adj(c), c.X.to(_dev()), c.L.to(_dev())
    ma, mb = _model(c, mode), _model(c, mode)
    ta, tb = _step(ma, keep_best=True), _step(mb, keep_best=True)
    for s in range(2):
        la, Ya = ta.step(A, X, L)
        li, Yb = tb.accumulate(A, X, L)
        lb = tb.apply()
        same = {"Y": torch.equal(_bits(Ya), _bits(Yb)), "loss": torch.equal(_bits(la), _bits(lb)),
                "call's loss": torch.equal(_bits(la), _bits(li)), "gradients": torch.equal(_bits(ta.flat_g), _bits(tb.flat_g)),
                "parameters": torch.equal(_bits(ta.flat_p), _bits(tb.flat_p)),
                "exp_avg": torch.equal(_bits(ta.exp_avg), _bits(tb.exp_avg)),
                "exp_avg_sq": torch.equal(_bits(ta.exp_avg_sq), _bits(tb.exp_avg_sq)),
                "best": float(ta.best_loss) == float(tb.best_loss) and int(ta.best_step) == int(tb.best_step)}
        print("%s %s step %d: %s; gradients differ by at most %.2e, parameters by %.2e"
              % (name, mode, s + 1, same, float((ta.flat_g - tb.flat_g).abs().max()), float((ta.flat_p - tb.flat_p).abs().max())))
        assert all(same.values()), same
    assert ta.steps == tb.steps == 2


# ---- 3. loss specs: the calls weigh by their labels -------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,t_from", [("l1", 2), ("huber", 0)])
@pytest.mark.parametrize("mode", ["f32", "f16x3"])
def test_l1_and_huber_accumulate_to_the_oracles_gradient(kind, t_from, mode):
    c = sl.case("small")
    delta = sl.DELTA if kind == "huber" else 0.0
    q = sl.reference("small", "fp32", kind, delta, t_from, "none")
    tr = _step(_model(c, mode))
    A, X, L = c.A.to(_dev()), c.X.to(_dev()), q.L.to(_dev())
    _accumulate_cut(tr, A, X, L, ac.SPEC_CUT, loss=kind, huber_delta=sl.DELTA, loss_from=t_from)
    assert int(tr.accumulated_count) == q.m
    loss = tr.apply()
    el, eg = abs(float(loss) - q.loss) / abs(q.loss), _grad_errors(tr, q.gm)
    print("%s from %d %s, cut %s: loss %.2e  worst gradient %.2e (bar %.1e)" % (kind, t_from, mode, ac.SPEC_CUT, el,
                                                                                max(eg.values()), ac.TOL))
    assert el <= ac.TOL and max(eg.values()) <= ac.TOL, (el, eg)


def test_missing_labels_weigh_the_calls_by_the_labels_that_exist():
    c = sl.case("small")
    q = ac.staggered_union()
    Lh = ac.staggered_labels()
    wl, wg = ac.window_weighted(c, Lh, "l1", 0.0, 2, 1, ac.SPEC_CUT)
    tr = _step(_model(c, "f32"))
    _accumulate_cut(tr, c.A.to(_dev()), c.X.to(_dev()), Lh.to(_dev()), ac.SPEC_CUT, loss="l1", loss_from=2, missing_labels=True)
    count = tr.accumulated_count
    assert count.dtype == torch.int64 and count.dim() == 0 and count.is_cuda and int(count) == q.m[0]
    loss = tr.apply()
    el, eg = abs(float(loss) - q.loss[0]) / q.loss[0], _grad_errors(tr, q.g[0])
    other = {k: rel_to_max(v.detach().cpu(), wg[k]) for k, v in zip(PARAM_KEYS, tr.g_views)}
    print("staggered NaN labels: %d labels; loss %.2e  worst gradient %.2e of the count-weighted oracle (bar %.1e); against the "
          "WINDOW-weighted answer: loss %.2e, worst gradient %.2e" % (q.m[0], el, max(eg.values()), ac.TOL,
                                                                      abs(float(loss) - wl) / wl, max(other.values())))
    assert el <= ac.TOL and max(eg.values()) <= ac.TOL, (el, eg)
    assert abs(float(loss) - wl) / wl > ac.TOL and max(other.values()) > ac.TOL


# ---- 4. series calls, and both kinds in one step ----------------------------------------------------------------------------------------
def test_two_series_tensors_share_one_step():
    c, s, q = ac.case("small"), ac.series_case(), ac.series_union()
    model = _model(c, "f32")
    tr = _step(model)
    A = c.A.to(_dev())
    Ys = []
    for series, Ls, table in zip(s.series, s.Ls, s.tables):
        loss, Y = tr.accumulate_series(A, series.to(_dev()), Ls.to(_dev()), s.T, starts=list(table))
        Ys.append(Y.cpu())
    n = sum(len(t) for t in s.tables)
    assert tr.accumulated == 2 and int(tr.accumulated_count) == n * s.T * c.H
    loss = tr.apply()
    ey, el = rel_to_max(torch.cat(Ys), q.Y[0]), abs(float(loss) - q.loss[0]) / q.loss[0]
    eg, ep = _grad_errors(tr, q.g[0]), _param_errors(model, q.p[0])
    print("series 17 + 5 windows of two tensors: Y %.2e  loss %.2e  worst gradient %.2e  worst parameter %.2e (bar %.1e)"
          % (ey, el, max(eg.values()), max(ep.values()), ac.TOL))
    assert max(ey, el, max(eg.values()), max(ep.values())) <= ac.TOL


def test_series_calls_with_missing_labels_count_on_the_device():
    c, s = ac.case("small"), ac.series_case()
    Ls = [x.clone() for x in s.Ls]
    Ls[1][::3, ::2] = float("nan")
    L = torch.cat([torch.stack([x[r:r + s.T] for r in t]) for x, t in zip(Ls, s.tables)])
    q = ac.oracle_steps(c.A, torch.cat(s.X), L, c.p, "mse", 0.0, 0, 1)
    tr = _step(_model(c, "f32"))
    A = c.A.to(_dev())
    for series, ls, table in zip(s.series, Ls, s.tables):
        tr.accumulate_series(A, series.to(_dev()), ls.to(_dev()), s.T, starts=list(table), missing_labels=True)
    assert int(tr.accumulated_count) == q.m[0] < L.numel()
    loss = tr.apply()
    el, eg = abs(float(loss) - q.loss[0]) / q.loss[0], _grad_errors(tr, q.g[0])
    print("series, NaN labels in the second tensor: %d of %d labels; loss %.2e  worst gradient %.2e (bar %.1e)"
          % (q.m[0], L.numel(), el, max(eg.values()), ac.TOL))
    assert el <= ac.TOL and max(eg.values()) <= ac.TOL


def test_a_materialised_call_and_a_series_call_share_one_step():
    c, s, q = ac.case("small"), ac.series_case(), ac.mixed_union()
    model = _model(c, "f32")
    tr = _step(model)
    A = c.A.to(_dev())
    tr.accumulate(A, c.X.to(_dev()), c.L.to(_dev()))
    tr.accumulate_series(A, s.series[0].to(_dev()), s.Ls[0].to(_dev()), s.T, starts=list(s.tables[0]))
    assert int(tr.accumulated_count) == (c.B + len(s.tables[0])) * c.T * c.H
    loss = tr.apply()
    el, eg, ep = abs(float(loss) - q.loss[0]) / q.loss[0], _grad_errors(tr, q.g[0]), _param_errors(model, q.p[0])
    print("6 materialised + 17 series windows: loss %.2e  worst gradient %.2e  worst parameter %.2e (bar %.1e)"
          % (el, max(eg.values()), max(ep.values()), ac.TOL))
    assert max(el, max(eg.values()), max(ep.values())) <= ac.TOL


# ---- 5. clipping, keep_best, discard ------------------------------------------------------------------------------------------------------
def test_clipping_sees_the_norm_of_the_union_gradient():
    c = ac.case("small")
    free = ac.union("small", steps=3)
    max_norm = 0.5 * free.norm[0]
    q = ac.union("small", steps=2, max_norm=max_norm)
    model = _model(c, "f16x3")
    tr = _step(model, max_grad_norm=max_norm)
    A, X, L = c.A.to(_dev()), c.X.to(_dev()), c.L.to(_dev())
    for s in range(2):
        _accumulate_cut(tr, A, X, L, c.cut)
        tr.apply()
        norm, coef, want = float(tr.grad_norm), float(tr.clip_coef), min(1.0, max_norm / (q.norm[s] + 1e-6))
        ep = _param_errors(model, q.p[s])
        print("clipped step %d: norm %.6f against %.6f, coefficient %.6f against %.6f, worst parameter %.2e"
              % (s + 1, norm, q.norm[s], coef, want, max(ep.values())))
        assert abs(norm - q.norm[s]) <= ac.TOL * q.norm[s] and abs(coef - want) <= ac.TOL and max(ep.values()) <= ac.TOL
    assert want < 1.0


def test_keep_best_follows_the_accumulated_losses():
    c = ac.case("small")
    model = _model(c, "f32")
    tr = _step(model, keep_best=True)
    A, X = c.A.to(_dev()), c.X.to(_dev())
    labels = [c.L.to(_dev()), (c.L + 4.0).to(_dev()), c.L.to(_dev())]          # the second step's loss is far larger
    losses, best, step = [], float("inf"), -1
    for s, L in enumerate(labels):
        calls = _accumulate_cut(tr, A, X, L, c.cut)
        losses.append(float(tr.apply()))
        won = losses[-1] < best
        if won:
            best, step = losses[-1], s + 1
        assert int(tr.improved) == int(won) and float(tr.best_loss) == best and int(tr.best_step) == step, (s, losses)
        assert float(calls[0][0]) != losses[-1]                         # the accumulated loss decides, not a call's
        if won:
            assert all(torch.equal(a, b) for a, b in zip(tr.best_state_dict().values(), tr.p_views))
    print("keep_best over three applies: losses %s, best %.6f at step %d" % (losses, best, step))
    assert losses[1] > losses[0] and step in (1, 3)


def test_discard_leaves_everything_but_the_accumulator_untouched():
    c = ac.case("small")
    A, X, L = c.A.to(_dev()), c.X.to(_dev()), c.L.to(_dev())
    ma, mb = _model(c, "f16x3"), _model(c, "f16x3")
    ta, tb = _step(ma, keep_best=True), _step(mb, keep_best=True)
    ta.step(A, X, L)
    tb.step(A, X, L)
    snap = lambda: [t.detach().cpu().clone().view(torch.uint8) for t in (ta.flat_p, ta.exp_avg, ta.exp_avg_sq, ta._best, ta._best_p)]  # noqa: E731
    before = snap()
    _accumulate_cut(ta, A, X, L + 1.0, c.cut)
    with pytest.raises(RuntimeError, match="step while an accumulation is open"):
        ta.step(A, X, L)
    with pytest.raises(RuntimeError, match="state_dict\\(\\) while an accumulation is open"):
        ta.state_dict()
    assert ta.accumulated == 3 and ta.steps == 1
    ta.discard()
    assert ta.accumulated == 0 and ta.steps == 1 and all(torch.equal(a, b) for a, b in zip(before, snap()))
    la, _ = ta.step(A, X, L)
    lb, _ = tb.step(A, X, L)
    assert torch.equal(_bits(la), _bits(lb)) and torch.equal(_bits(ta.flat_p), _bits(tb.flat_p))
    assert torch.equal(_bits(ta.exp_avg_sq), _bits(tb.exp_avg_sq)) and ta.steps == tb.steps == 2
    with pytest.raises(RuntimeError, match="nothing was accumulated"):
        ta.apply()


# ---- 6. a one-rank process group: one all-reduce per apply, none during accumulate -----------------------------------------------------
def _one_rank(rank, port, out_dir):
    from windgnn_amd.distributed import ensure_rccl_env
    ensure_rccl_env()                     # before this process touches the GPU
    c = ac.case("small")
    A, X, L = c.A.to(_dev()), c.X.to(_dev()), c.L.to(_dev())
    plain = _step(_model(c, "f16x3"))
    for _ in range(2):
        _accumulate_cut(plain, A, X, L, c.cut)
        plain.apply()
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", rank=0, world_size=1, device_id=torch.device("cuda:0"))
    calls = {"n": 0}
    real = dist.all_reduce

    def counted(*a, **kw):
        calls["n"] += 1
        return real(*a, **kw)
    dist.all_reduce = counted
    tr = _step(_model(c, "f16x3"), process_group=dist.group.WORLD)
    assert tr.collective and tr.exchange.direct is None
    seen = []
    for n_global in (c.B, None):          # stated: the bucket's all-reduce alone; counted: the count collective before it
        _accumulate_cut(tr, A, X, L, c.cut)
        seen.append(calls["n"])
        tr.apply(n_global)
        seen.append(calls["n"])
    empty = _step(_model(c, "f16x3"), process_group=dist.group.WORLD)      # a rank that has never run a forward
    p0 = _bits(empty.flat_p).clone()
    loss = empty.apply(n_global=c.B)
    seen.append(calls["n"])
    torch.cuda.synchronize()
    ok = (torch.equal(_bits(plain.flat_p), _bits(tr.flat_p)) and torch.equal(_bits(plain._gbuf), _bits(tr._gbuf))
          and torch.equal(_bits(plain.exp_avg_sq), _bits(tr.exp_avg_sq)))
    np.save(os.path.join(out_dir, "one_rank.npy"),
            np.array(seen + [int(ok), int(torch.equal(p0, _bits(empty.flat_p))), empty.steps, int(float(loss) == 0.0)]))
    dist.barrier()
    dist.destroy_process_group()


def test_a_one_rank_group_all_reduces_once_per_apply_and_changes_no_bit(tmp_path):
    from test_distributed_gpu import _free_port
    mp.spawn(_one_rank, args=(_free_port(), str(tmp_path)), nprocs=1, join=True)
    got = np.load(os.path.join(str(tmp_path), "one_rank.npy")).tolist()
    print("all-reduces after [3 accumulates, apply(n_global), 3 accumulates, apply(), an empty rank's apply]: %s" % got[:5])
    assert got[:5] == [0, 1, 1, 3, 4]
    assert got[5:] == [1, 1, 1, 1], got[5:]      # bit-identical to no group; the empty rank: parameters kept, one step, loss 0
