"""Training on a loss spec on materialised windows on the MI355X: TrainStep.step / forward_backward with loss= / huber_delta= /
loss_from= / missing_labels= in every math mode, on a dense and a CSR adjacency, on the wide-GRU path and with 16-bit I/O
(tests/step_loss_cases.py has the shapes, the references and the bars; tests/test_step_loss_host.py the arithmetic of
functional.loss_spec_grad and the call sequences).  Every figure is printed before it is asserted.

Observed on the MI355X, worst over the 12 specs of a case (Y; loss relative to the oracle's; gradient / tensor max):
    fp32 I/O, bar 1e-4:  small f32 4.6e-7 / 1.2e-7 / 4.4e-7; small f16x3 = f16x3g 7.5e-7 / 1.2e-7 / 2.0e-6; real f32 1.1e-6 /
                         8.1e-8 / 4.7e-7; real f16x3 = f16x3g 2.4e-6 / 8.1e-8 / 2.6e-6; wide f32 1.5e-6 / 1.3e-7 / 1.4e-6; wide f16x3
                         2.4e-6 / 9.9e-8 / 3.8e-6; csr f16x3 5.9e-6 / 1.5e-7 / 9.0e-6; call f32 3.8e-7 / 7.7e-8 / 4.2e-7; call f16x3
                         5.4e-7 / 9.8e-8 / 2.2e-6
    one-pass f16:        small 1.8e-3 / 3.6e-5 / 1.5e-2; real 2.8e-3 / 3.4e-5 / 1.1e-2; real with fp16 I/O 2.8e-3 / 3.4e-5 / 9.7e-3
                         (bars 2e-2 (+ 2.5e-4), 2e-3 max(1, loss), 5e-2)
    three Adam steps:    parameters and losses within 1.4e-7 (dense), 4.0e-6 (CSR), 2.5e-6 (clipped), 1.3e-7 (carried state)
16-bit I/O: a step on a spec runs on fp32 copies of X and L, so the loss is formed from the unrounded Y, as the fused MSE step
forms its own from the unrounded state; Y comes back rounded once to X's type, bit-identical to the 16-bit forward's.
    real f16x3 + bf16 I/O: Y 1.95e-3 (bar 1e-4 + 2e-3) / 8.1e-8 / 1.9e-6 (bar 1e-4); 2 x the Huber-1e6 gradients equal the fused
                           step's exactly, 2 x loss 1.06996000 against 1.06995988
    (formed from the bf16-rounded Y instead, the same case gave Huber gradients within 7.7e-4 and missed that bar.)"""
import math

import pytest
import torch

import series_lossfn_cases as lc
import step_loss_cases as sl
from conftest import PARAM_KEYS, max_abs, rel_to_max

pytestmark = pytest.mark.gpu


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _model(c, mode):
    from windgnn_amd import GCN_GRU
    m = GCN_GRU(13, 13, 13, c.S * 13, c.H, math=mode, validate=False)
    m.load_state_dict({k: v.clone() for k, v in c.p.items()})
    return m.to(_dev())


def _adj(c):
    return c.csr.to(_dev()) if c.csr is not None else c.A.to(_dev())


def _x(c):
    return c.X.to(sl.DTYPES[c.io]).to(_dev())


def _l(c, L, fused=False):
    """The labels as the call takes them: [T, H] for the one-window shape; fp32 beside bf16 X (the same values) unless the fused
    MSE entry points read them, which take X's dtype."""
    L = L if c.io == "bf16" and not fused else L.to(sl.DTYPES[c.io])
    return (L[0] if c.name == "call" else L).to(_dev())


def _step(model, **kw):
    from windgnn_amd.trainer import TrainStep
    return TrainStep(model, lr=1e-3, eps=sl.EPS, **kw)


def _grads(tr):
    return {k: g.detach().cpu().clone() for k, g in zip(PARAM_KEYS, tr.g_views)}


def _y_err(Y, Yo, how):
    Y = Y.float().cpu().reshape(Yo.shape)
    return rel_to_max(Y, Yo) if how == "rel_to_max" else max_abs(Y, Yo)


IDS = ["%s-%s-%s" % c for c in sl.CASES]


# ---- 1. against the fp64 oracle ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode,io", sl.CASES, ids=IDS)
def test_every_spec_matches_the_oracle_fed_the_fp64_dy_of_the_spec(name, mode, io):
    c = sl.case(name, io)
    (how, y_bar), g_bar, loss_bar = sl.bars(mode, io)
    A, X = _adj(c), _x(c)
    tr = _step(_model(c, mode))
    with pytest.raises(RuntimeError, match="loss_count"):
        tr.loss_count
    worst = {"Y": 0.0, "loss": 0.0, "grad": 0.0}
    failed = []
    for kind in sl.KINDS:
        for t_from in sl.t_froms(c.T):
            for mask in sl.MASKS:
                q = sl.reference(name, io, kind, sl.DELTA if kind == "huber" else 0.0, t_from, mask)
                loss, Y = tr.forward_backward(A, X, _l(c, q.L), loss=kind, huber_delta=sl.DELTA, loss_from=t_from,
                                              missing_labels=mask != "none")
                assert loss.data_ptr() == tr._loss.data_ptr() and Y.dtype == sl.DTYPES[io] and tr.steps == 0
                assert int(tr.loss_count) == q.m
                ey = _y_err(Y, c.Yo, how)
                el = abs(float(loss) - q.loss)
                g = _grads(tr)
                eg = {k: rel_to_max(g[k], q.gm[k]) for k in PARAM_KEYS}
                what = "%s %s %s %s from %d %s" % (name, mode, io, kind, t_from, mask)
                print("%s: Y %.2e (bar %.1e)  loss %.2e (bar %.1e)  worst gradient %.2e (bar %.1e)"
                      % (what, ey, y_bar, el, loss_bar(q.loss), max(eg.values()), g_bar))
                worst = {"Y": max(worst["Y"], ey), "loss": max(worst["loss"], el / max(abs(q.loss), 1e-300)),
                         "grad": max(worst["grad"], max(eg.values()))}
                if not (ey <= y_bar and el <= loss_bar(q.loss) and max(eg.values()) <= g_bar):
                    failed.append((what, ey, el, eg))
                for k in PARAM_KEYS:
                    assert torch.isfinite(g[k]).all(), (what, k)
                if t_from == c.T - 1:                            # the last step alone is counted: BPTT still runs every step
                    for k in ("gru.weight_hh_l0", "conv1.weight", "conv2.weight"):
                        assert float(g[k].abs().max()) > 0 and float(q.gm[k].abs().max()) > 0, (what, k)
    print("%s %s %s: worst Y %.2e, loss (relative) %.2e, gradient / tensor max %.2e" % (name, mode, io, worst["Y"], worst["loss"],
                                                                                      worst["grad"]))
    tr.check()
    assert not failed, failed


# ---- 2. the new route against the fused MSE route -----------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode,io", sl.CASES, ids=IDS)
def test_huber_with_every_residual_in_the_quadratic_arm_is_half_the_fused_mse_step(name, mode, io):
    c = sl.case(name, io)
    _, g_bar, loss_bar = sl.bars(mode, io)
    A, X = _adj(c), _x(c)
    L = c.L["mse"]
    assert float((c.Yo - L.double()).abs().max()) < 2.0
    tr = _step(_model(c, mode))
    loss0, Y0 = tr.forward_backward(A, X, _l(c, L, fused=True))
    loss0, g0 = float(loss0), _grads(tr)
    loss1, Y1 = tr.forward_backward(A, X, _l(c, L), loss="huber", huber_delta=sl.HALF_DELTA)
    loss1, g1 = float(loss1), _grads(tr)
    assert torch.equal(Y0, Y1) and int(tr.loss_count) == L.numel()
    eg = {k: rel_to_max(2.0 * g1[k], g0[k]) for k in PARAM_KEYS}
    print("%s %s %s: 2 x loss %.8f against %.8f; 2 x gradients against the fused route's, worst %.2e (bar %.1e)"
          % (name, mode, io, 2.0 * loss1, loss0, max(eg.values()), g_bar))
    assert abs(2.0 * loss1 - loss0) <= loss_bar(loss0)
    assert max(eg.values()) <= g_bar, eg


def test_exact_fp32_math_still_refuses_16_bit_windows_on_a_spec_step():
    c = sl.case("small")
    tr = _step(_model(c, "f32"))
    with pytest.raises(RuntimeError):
        tr.step(_adj(c), c.X.bfloat16().to(_dev()), c.L["huber"].to(_dev()), loss="huber")
    assert tr.steps == 0


# ---- 3. no label at all ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name,mode", [("small", "f32"), ("small", "f16x3"), ("real", "f16"), ("wide", "f16x3"), ("csr", "f16x3")])
def test_without_any_label_the_loss_is_nan_and_a_step_changes_no_parameter(name, mode):
    c = sl.case(name)
    A, X = _adj(c), _x(c)
    tr = _step(_model(c, mode), keep_best=True)
    before = tr.flat_p.clone()
    loss, Y = tr.step(A, X, _l(c, sl.labels(c, "l1", "all")), loss="l1", loss_from=2, missing_labels=True)
    assert math.isnan(float(loss)) and int(tr.loss_count) == 0 and tr.steps == 1
    for k, g in _grads(tr).items():
        assert (g == 0).all(), (k, "not exactly zero")
    assert torch.equal(tr.flat_p, before) and int(tr.best_step) == -1            # bit-identical; a NaN loss wins nothing
    assert torch.isfinite(Y.float()).all()
    tr.check()


# ---- 4. three Adam steps on the oracle's trajectory ----------------------------------------------------------------------------------
def _assert_trajectory(what, losses, lo, model, po):
    seen = {k: rel_to_max(p.detach().cpu(), po[k]) for k, p in model.named_parameters()}
    for i, (a, b) in enumerate(zip(losses, lo)):
        seen["loss%d" % (i + 1)] = abs(a - b) / abs(b)
    print("%s: worst %.2e  " % (what, max(seen.values())) + "  ".join("%s %.2e" % kv for kv in seen.items()))
    for k, e in seen.items():
        assert e <= sl.TOL, (what, k, e)


@pytest.mark.parametrize("name,kw", [("small", {}), ("csr", {}), ("small", {"max_grad_norm": 1.0}), ("small", {"keep_best": True})],
                         ids=["dense", "csr", "clipped", "keep_best"])
def test_three_steps_follow_the_oracle_trajectory(name, kw):
    c = sl.case(name)
    lo, po, norms = sl.trajectory(name, kw.get("max_grad_norm"))
    A, X = _adj(c), _x(c)
    L = _l(c, sl.labels(c, "l1", "tenth"))
    model = _model(c, "f16x3")
    tr = _step(model, **kw)
    losses = []
    for s in range(sl.STEPS):
        loss, Y = tr.step(A, X, L, **sl.TRAIN)
        losses.append(float(loss))
        if "max_grad_norm" in kw:
            norm, coef = float(tr.grad_norm), float(tr.clip_coef)
            print("step %d: gradient norm %.6f against %.6f, clip coefficient %.6f" % (s + 1, norm, norms[s], coef))
            assert abs(norm - norms[s]) <= sl.TOL * norms[s] and abs(coef - min(1.0, 1.0 / (norms[s] + 1e-6))) <= sl.TOL
    assert tr.steps == sl.STEPS and int(tr.loss_count) == lc.counted(sl.labels(c, "l1", "tenth"), 2, 1).sum()
    if "keep_best" in kw:
        best, step = float("inf"), -1
        for i, v in enumerate(lo):                               # the oracle's losses decide
            if v < best:
                best, step = v, i + 1
        assert int(tr.best_step) == step and float(tr.best_loss) == losses[step - 1]
    tr.check()
    _assert_trajectory("step(%s) x3 %s f16x3 %r" % (", ".join("%s=%r" % kv for kv in sl.TRAIN.items()), name, kw), losses, lo,
                       model, po)


def test_three_carried_state_steps_follow_fp64_autograd_of_the_spec():
    from test_gpu_state_train import _fp64_model
    c = sl.case("small")
    A, X = _adj(c), _x(c)
    Lh = sl.labels(c, "l1", "tenth")
    model = _model(c, "f32")
    tr = _step(model, carry_state=True)
    leaves, f = _fp64_model(c.p)
    opt = torch.optim.Adam(list(leaves.values()), lr=1e-3, eps=sl.EPS)
    on = lc.counted(Lh, sl.TRAIN["loss_from"], 1)
    h = torch.zeros(c.B, c.H, dtype=torch.float64)
    losses, lo = [], []
    for s in range(sl.STEPS):
        loss, _ = tr.step(A, X, _l(c, Lh), **sl.TRAIN)
        losses.append(float(loss))
        opt.zero_grad()
        Yr, hn = f(c.A, c.X, h)
        ref = (Yr[on] - Lh.double()[on]).abs().sum() / int(on.sum())
        ref.backward()
        opt.step()
        h = hn.detach()
        lo.append(float(ref.detach()))
        assert max_abs(tr.state.cpu(), h) <= sl.TOL, s
    _assert_trajectory("carried state x3 small f32", losses, lo, model, {k: v.detach() for k, v in leaves.items()})


# ---- 5. repeatability ---------------------------------------------------------------------------------------------------------------
def _two_steps(c, mode, A, X, L, spec):
    tr = _step(_model(c, mode))
    out = []
    for _ in range(2):
        loss, Y = tr.step(A, X, L, **spec)
        out += [loss.clone(), Y.clone(), tr._gbuf.clone(), tr.flat_p.clone(), tr.loss_count.clone()]
    return out + [tr.exp_avg.clone(), tr.exp_avg_sq.clone()]


@pytest.mark.parametrize("name,mode", [("real", "f16x3"), ("small", "f32")])
def test_identical_steps_give_identical_bits_on_the_default_and_on_a_side_stream(name, mode):
    c = sl.case(name)
    dev = _dev()
    A, X = _adj(c), _x(c)
    L = _l(c, sl.labels(c, "huber", "tenth"))
    spec = dict(loss="huber", huber_delta=sl.DELTA, loss_from=2, missing_labels=True)
    one = _two_steps(c, mode, A, X, L, spec)
    two = _two_steps(c, mode, A, X, L, spec)
    for a, b in zip(one, two):
        assert torch.equal(a, b)
    side = torch.cuda.Stream(dev)
    side.wait_stream(torch.cuda.current_stream(dev))
    with torch.cuda.stream(side):
        three = _two_steps(c, mode, A, X, L, spec)
    side.synchronize()
    for a, b in zip(one, three):
        assert torch.equal(a, b)
    assert not torch.equal(one[3], one[8])                       # (the second step moved the parameters)


# ---- 6. the default step is untouched ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["f32", "f16x3"])
def test_a_default_step_around_a_spec_step_elsewhere_gives_the_bits_it_always_gave(mode):
    c = sl.case("real")
    A, X = _adj(c), _x(c)
    L = _l(c, c.L["mse"])
    Ln = _l(c, sl.labels(c, "huber", "tenth"))

    def run(between):
        tr = _step(_model(c, mode))
        out = []
        for k in range(2):
            loss, Y = tr.step(A, X, L)
            out += [loss.clone(), Y.clone(), tr._gbuf.clone(), tr.flat_p.clone()]
            if between and k == 0:
                other = _step(_model(c, mode))
                other.step(A, X, Ln, loss="huber", huber_delta=sl.DELTA, loss_from=2, missing_labels=True)
                assert int(other.loss_count) > 0
        return out
    for a, b in zip(run(False), run(True)):
        assert torch.equal(a, b)
