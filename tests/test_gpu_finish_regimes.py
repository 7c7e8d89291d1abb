"""The fused step tail in every split-K and partial-row regime, on the MI355X: tests/finish_cases.py's CASES.

finish_kernel / finish_norm_kernel (csrc/finish.hip) close every TrainStep step: they sum the split-K partials of the two GRU
weight-gradient products and the per-workgroup partial rows of the GCN backward in unrolled loops whose shape depends on the
split-K count and the row count alone, run Adam and rewrite the staged W_ih images.  The older finish tests reach seg_tn at
split-K 1, 3, 6 and 96 and never a conv row count that puts the tail behind the unrolled body
(tests/test_finish_regimes_host.py has the table).  Here a ladder of B at T = 2 takes seg_tn, seg_plain and seg_conv through
every regime reachable below 4200 rows, each rung once with 2-byte and once with the wide (8-byte, quad-transposed) image
stores, plus gemm32.hip's padded partials with and without the row remap, the wide-GRU path and a CSR adjacency.  Inputs are
tests/lattice_inputs.py's draw (live ReLU masks, non-zero biases, A != A^T); the host test plants a dropped tail and a doubled
chunk into the fp64 oracle and shows that they move a gradient by more than ten bars.

Per case, from a mid-training optimiser state (non-zero m and v, step 3): the deferred backward and wgnn_finish(6, adam), then
  gradients   against the fp64 oracle's step, relative to max: 1e-4 (f16x3g from 4096 rows: 1e-3).  This is the comparison that
              holds the loops: a dropped or doubled chunk moves a gradient by ten bars or more (the host test).  One-pass fp16
              has its own bar only (F16_G_TOL = 5e-2), which tells a tail that never ran but not one chunk of 24;
  undeferred  wgnn_bwd_mse_part(7 | 8): GRU gradients bit for bit, conv gradients within 2e-6, the loss identical.  The
              undeferred call reduces through the SAME kernel in its reduce-only form (finish_kernel<0>; api.hip bwd_weights,
              bwd_dg), so this line holds the Adam instantiation to the reduce-only one, not the loops to anything else;
  Adam        an fp64 evaluation of torch.optim.Adam's formulas on the device's own fp32 gradients, state and hyper-parameters:
              p within 2e-7, m and v within 1e-6 of max;
  images      byte-identical to wgnn_prepare_weights of the stepped parameters, and a forward through them within 1e-4 of the
              oracle's Y at those parameters (one-pass fp16: its own bar, F16_Y_TOL);
  split forms finish(4), finish(2), finish(0, adam) and the FINISH_ADAM_GRU + FINISH_ADAM_CONV pair: bit for bit the fused launch;
  clipping    finish_norm's gradients bit for bit, its norm within NORM_TOL of the fp64 norm of them; finish_clipped = Adam on
              g * coef under the bars above, g keeping the unclipped bits;
  clean exit  the status word stays clear and a second run gives the same bits.
Every bar is imported or restated from the older finish tests; none is new."""
import functools

import numpy as np
import pytest
import torch

import finish_cases as fc
import lattice_inputs as li
from conftest import PARAM_KEYS, max_abs, rel_to_max
from test_gpu_clip import NORM_TOL
from test_gpu_parity import F16_G_TOL, F16_Y_TOL, G_TOL, Y_TOL

pytestmark = pytest.mark.gpu

MATH = {"f32": 0, "f16x3": 1, "f16": 2, "f16x3g": 3}
CONV_TOL = 2e-6               # deferred against undeferred conv gradients: another (fixed) order of the partial rows
P_TOL, MV_TOL = 2e-7, 1e-6    # tests/test_gpu_parity.py's finish test: p absolute, m and v relative to max
X2_G_TOL = 1e-3               # f16x3g from 4096 rows: the single fp16 plane of dGI / dGHn (tests/test_gpu_state_train.py _tols)
HYPER = dict(step=3, lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8)


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=2)
def _reference(shape):
    """The lattice draw of a shape and the fp64 oracle's training step on it (shared by the shape's modes: never written to)."""
    from oracle import windgnn_oracle as orc
    S, T, B, H, csr = shape
    shift, seed = fc.inputs_of(shape)
    d = li.draw(S, T, B, H, csr, shift, seed)
    Y, loss, grads = orc.train_step(d.A.double(), d.X.double(), d.L.double(), {k: v.double() for k, v in d.p.items()})
    return d, Y, float(loss), grads


def adam64(p, g, m, v, coef=None):
    """torch.optim.Adam's single-tensor formulas in fp64 on fp32 inputs, with the hyper-parameters as the C structure holds
    them (fp32); coef: the clip coefficient, applied to g in fp32 as wgnn_finish_clipped does."""
    f = lambda x: float(np.float32(x))
    b1, b2, lr, eps, step = f(HYPER["beta1"]), f(HYPER["beta2"]), f(HYPER["lr"]), f(HYPER["eps"]), HYPER["step"]
    g = (g if coef is None else g * coef).double()
    m = b1 * m.double() + (1.0 - b1) * g
    v = b2 * v.double() + (1.0 - b2) * g * g
    denom = v.sqrt() / (1.0 - b2 ** step) ** 0.5 + eps
    return p.double() - lr / (1.0 - b1 ** step) * m / denom, m, v


IDS = ["S%d-T%d-B%d-H%d%s-%s" % (c[:4] + ("-csr" if c[4] else "", c[5])) for c in fc.CASES]


@pytest.mark.parametrize("case", fc.CASES, ids=IDS)
def test_finish_in_every_regime(case):
    from oracle import windgnn_oracle as orc
    from windgnn_amd import _lib
    from windgnn_amd.functional import (check_range_status, clip_buffer, finish_clipped, finish_norm, finish_step,
                                        gcn_gru_backward_mse_raw, gcn_gru_forward_raw, prepared_weights)
    from windgnn_amd.graph import CsrAdjacency
    S, T, B, H, csr, math = case
    shape = case[:5]
    seg = fc.segments(S, T, B, H, math, csr)
    dev = _dev()
    dr, Yo, loss_o, go = _reference(shape)
    A = CsrAdjacency.from_dense(dr.A).to(dev) if csr else dr.A.to(dev)
    X, L = dr.X.to(dev), dr.L.to(dev)
    mode = MATH[math]
    DEFER = _lib.BWD_DEFER

    def fresh():
        ps = [dr.p[k].clone().to(dev).contiguous() for k in PARAM_KEYS]
        gg = torch.Generator().manual_seed(5)
        ms = [(torch.rand(q.shape, generator=gg) * 1e-3).to(dev) for q in ps]       # a mid-training optimiser state
        vs = [(torch.rand(q.shape, generator=gg) * 1e-6).to(dev) for q in ps]
        return ps, [torch.full_like(q, 7.0) for q in ps], ms, vs

    # ---- the undeferred passes
    ps, gs, ms, vs = fresh()
    loss = torch.zeros((), device=dev)
    Y, stash, d = gcn_gru_forward_raw(A, X, ps, mode, labels=L)
    gcn_gru_backward_mse_raw(d, A, X, ps, Y, L, stash, gs, loss, 1.0, part=7 | 8)
    g_und, loss_und = [q.clone() for q in gs], float(loss)
    p0, m0, v0 = [q.cpu() for q in ps], [q.cpu() for q in ms], [q.cpu() for q in vs]

    def run(form, tail=None):
        """Forward and deferred backward, then: 0 finish(6, adam); 1 / 2 the split forms; 'tail' tail(d, ps, gs, adam, img)."""
        ps, gs, ms, vs = fresh()
        img = prepared_weights(d, ps, dev)
        loss = torch.zeros((), device=dev)
        adam = dict(exp_avg=ms, exp_avg_sq=vs, **HYPER)
        Y, stash, d2 = gcn_gru_forward_raw(A, X, ps, mode, labels=L, prepared=img)
        out = None
        if form in (1, 2):
            gcn_gru_backward_mse_raw(d2, A, X, ps, Y, L, stash, gs, loss, 1.0, part=1 | 4 | 8 | DEFER, prepared=img)
            finish_step(d2, ps, gs, 4)
            gcn_gru_backward_mse_raw(d2, A, X, ps, Y, L, stash, gs, loss, 1.0, part=2 | DEFER, prepared=img)
            finish_step(d2, ps, gs, 2)
            if form == 2:
                finish_step(d2, ps, gs, _lib.FINISH_ADAM_GRU, adam, img)
                finish_step(d2, ps, gs, _lib.FINISH_ADAM_CONV, adam, img)
            else:
                finish_step(d2, ps, gs, 0, adam, img)
        else:
            gcn_gru_backward_mse_raw(d2, A, X, ps, Y, L, stash, gs, loss, 1.0, part=7 | 8 | DEFER, prepared=img)
            if form == 0:
                finish_step(d2, ps, gs, 6, adam, img)
            else:
                out = tail(d2, ps, gs, adam, img)
        return dict(p=ps, g=gs, m=ms, v=vs, img=img, loss=float(loss), out=out)

    def same_bits(a, b, what):
        for k, x, y in zip(PARAM_KEYS * 4, a["p"] + a["g"] + a["m"] + a["v"], b["p"] + b["g"] + b["m"] + b["v"]):
            assert torch.equal(x, y), (what, k)
        assert (a["img"] is None and b["img"] is None) or torch.equal(a["img"], b["img"]), what
        assert a["loss"] == b["loss"], what

    fused = run(0)
    fig = {}
    # ---- gradients against the fp64 oracle
    g_dev = [q.cpu() for q in fused["g"]]
    fig["gru"] = max(rel_to_max(g_dev[i], go[PARAM_KEYS[i]]) for i in range(4, 8))
    fig["conv"] = max(rel_to_max(g_dev[i], go[PARAM_KEYS[i]]) for i in range(4))
    fig["loss"] = abs(fused["loss"] - loss_o) / max(1.0, loss_o)
    # ---- against the undeferred passes
    fig["conv_und"] = max(rel_to_max(g_dev[i], g_und[i].cpu()) for i in range(4))
    # ---- Adam in fp64 on the device's own gradients and state
    want = [adam64(p, g, m, v) for p, g, m, v in zip(p0, g_dev, m0, v0)]
    fig["p"] = max(max_abs(q.cpu(), w[0]) for q, w in zip(fused["p"], want))
    fig["m"] = max(rel_to_max(q.cpu(), w[1]) for q, w in zip(fused["m"], want))
    fig["v"] = max(rel_to_max(q.cpu(), w[2]) for q, w in zip(fused["v"], want))
    # ---- a forward on the stepped parameters through the images finish wrote
    with torch.no_grad():
        Y2, _, _ = gcn_gru_forward_raw(A, X, fused["p"], mode, want_stash=False, prepared=fused["img"])
    p1 = {k: q.cpu().double() for k, q in zip(PARAM_KEYS, fused["p"])}
    fig["Y"] = max_abs(Y2.cpu(), orc.forward(dr.A.double(), dr.X.double(), p1, want_cache=False)[0])
    # ---- the norm and the clipped step on the same partials

    def measure(d2, ps, gs, adam, img):
        clip = clip_buffer(d2, dev)
        clip.fill_(float("nan"))
        finish_norm(d2, gs, 6, float("inf"), clip)
        return clip[:2].clone()

    normed = run("tail", measure)
    total = float(normed["out"][0])
    norm64 = float(torch.sqrt(sum((q.double() ** 2).sum() for q in g_dev)))
    fig["norm"] = abs(total - norm64) / norm64

    def clipped(d2, ps, gs, adam, img):
        clip = clip_buffer(d2, dev)
        finish_norm(d2, gs, 6, total / 8, clip)
        before = [q.clone() for q in gs]
        finish_clipped(d2, ps, gs, adam, clip, img)
        return clip[:2].clone(), before

    cl = run("tail", clipped)
    tc, before = cl["out"]
    coef = tc[1].cpu()
    want_c = [adam64(p, g, m, v, coef) for p, g, m, v in zip(p0, g_dev, m0, v0)]
    fig["p_clip"] = max(max_abs(q.cpu(), w[0]) for q, w in zip(cl["p"], want_c))
    fig["m_clip"] = max(rel_to_max(q.cpu(), w[1]) for q, w in zip(cl["m"], want_c))
    fig["v_clip"] = max(rel_to_max(q.cpu(), w[2]) for q, w in zip(cl["v"], want_c))
    print("finish %s: ih %s sk %d (%d live), hh %s sk %d%s, conv_rows %d, wide %d: %s"
          % (IDS[fc.CASES.index(case)], seg["ih"]["family"], seg["ih"]["sk"], seg["ih"]["chunks"], seg["hh"]["family"], seg["hh"]["sk"],
             " remap" if seg["hh"]["remap"] else "", seg["conv_rows"], seg["wide"], " ".join("%s=%.2e" % kv for kv in fig.items())))

    g_tol = F16_G_TOL if math == "f16" else (X2_G_TOL if (math == "f16x3g" and B * T >= 4096) else G_TOL)
    assert fig["gru"] <= g_tol and fig["conv"] <= g_tol, (case, fig)
    if math != "f16":
        assert fig["loss"] <= 1e-5, (case, fig)
    for k, a, b in zip(PARAM_KEYS, fused["g"], g_und):
        if k.startswith("gru"):
            assert torch.equal(a, b), (case, k)                   # finish_kernel<1> against finish_kernel<0>: one summation tree
    assert fig["conv_und"] <= CONV_TOL and fused["loss"] == loss_und, (case, fig, fused["loss"], loss_und)
    assert fig["p"] <= P_TOL and fig["m"] <= MV_TOL and fig["v"] <= MV_TOL, (case, fig)
    if fused["img"] is not None:
        assert torch.equal(fused["img"], prepared_weights(d, fused["p"], dev)), case
    else:
        assert math == "f32" and not seg["wide"]
    assert fig["Y"] <= (F16_Y_TOL if math == "f16" else Y_TOL), (case, fig)
    for form in (1, 2):
        same_bits(run(form), fused, "split form %d" % form)
    for k, a, b in zip(PARAM_KEYS, normed["g"], fused["g"]):
        assert torch.equal(a, b), (case, "finish_norm", k)
    assert float(normed["out"][1]) == 1.0 and norm64 > 0 and fig["norm"] <= NORM_TOL, (case, fig)
    assert tc[0].view(torch.int32).item() == normed["out"][0].view(torch.int32).item()
    assert abs(float(coef) - (total / 8) / (total + 1e-6)) <= 2e-7 and float(coef) < 0.126, (case, float(coef))
    for k, a, b, c in zip(PARAM_KEYS, cl["g"], before, fused["g"]):
        assert torch.equal(a, b) and torch.equal(a, c), (case, "g was rewritten by the clipped step", k)
    assert fig["p_clip"] <= P_TOL and fig["m_clip"] <= MV_TOL and fig["v_clip"] <= MV_TOL, (case, fig)
    assert max(max_abs(a.cpu(), b.cpu()) for a, b in zip(cl["m"], fused["m"])) > 0, "the clipped step equals the unclipped one"
    if cl["img"] is not None:
        assert torch.equal(cl["img"], prepared_weights(d, cl["p"], dev)), case
    # ---- clean exit: no status bit, and the same bits again
    check_range_status(dev)
    same_bits(run(0), fused, "repeat")
    check_range_status(dev)
