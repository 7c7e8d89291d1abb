"""The two GRU weight-gradient plane GEMMs as one launch (WGNN_OPT_TN_MERGED, csrc/pgemm.hip pgemm_tn2_kernel), on the MI355X:
the merged launch against the two launches bit for bit (all 8 gradients, deferred and not, f16x3 / f16x3g / f16, and the state
stash's per-window rows), and the gradients against the fp64 oracle at tests/test_gpu_parity.py's tolerances.

Shapes (S, T, B, H) and what each can break:
  (34, 3, 48, 102)    B*T = 144: chunks end in partial 32-row stages; a T = 7 and a T = 4 role in one launch
  (34, 3, 32, 102)    B*T = 96, below two chunks of 64 rows: sk_ih = sk_hh = 1
  (7, 5, 33, 20)      one M block far below 320 rows, narrow N tiles (T = 3 and T = 1), odd B*T = 165
  (34, 2, 16, 127)    the largest H of this path: two M blocks, msplit padding, the two-source A operand at its edge
  (64, 2, 40, 102)    I + 1 = 833: four N blocks of dW_ih
  (34, 24, 176, 102)  B*T = 4224 crosses f16x3g's switch to a single plane of dGI (dW_ih one pass, dW_hh two)
  (64, 2, 2048, 102)  256 dW_ih items (four N blocks x 64 chunks) fill every CU, 64 dW_hh items: most workgroups run one role
  (40, 8, 2048, 102)  B*T = 16 384: 240 dW_ih items against 256 dW_hh items (sk_hh = 256, 64-row chunks): the other way round
The merged launch pairs item w of dW_ih with item w of dW_hh in workgroup w, so the last two are the shapes at which the
two item counts differ and the launch has as many workgroups as the device has CUs (checked below against the layout)."""
import functools

import pytest
import torch

from conftest import PARAM_KEYS, max_abs, rel_to_max
from test_gpu_parity import F16_G_TOL, F16_Y_TOL, G_TOL, Y_TOL

pytestmark = pytest.mark.gpu

MATH = {"f16x3": 1, "f16": 2, "f16x3g": 3}
SHAPES = [(34, 3, 48, 102), (34, 3, 32, 102), (7, 5, 33, 20), (34, 2, 16, 127), (64, 2, 40, 102), (34, 24, 176, 102),
          (64, 2, 2048, 102), (40, 8, 2048, 102)]
TOL = {"f16x3": (Y_TOL, G_TOL), "f16x3g": (Y_TOL, G_TOL), "f16": (F16_Y_TOL, F16_G_TOL)}


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(S, T, B, H):
    """Inputs and the fp64 oracle's step for one shape: computed once, shared by the three math modes, never written to."""
    from oracle import windgnn_oracle as orc
    g = torch.Generator().manual_seed(977 * S + 31 * H + B)
    A = torch.rand(S, S, generator=g) / S + 0.01
    X = torch.rand(B, T, S, 13, generator=g)
    L = torch.rand(B, T, H, generator=g)
    p = orc.init_params(S, 13, H, seed=S + H)
    Yo, loss_o, go = orc.train_step(A.double(), X.double(), L.double(), {k: v.double() for k, v in p.items()})
    return A, X, L, p, Yo, float(loss_o), go


class _merged:
    def __init__(self, on):
        self.on = on

    def __enter__(self):
        from windgnn_amd import _lib
        self.prev = _lib.set_option(_lib.OPT_TN_MERGED, self.on)

    def __exit__(self, *exc):
        from windgnn_amd import _lib
        _lib.set_option(_lib.OPT_TN_MERGED, self.prev)


def _tn_names(fn):
    """fn() under the library's profiler: its result and the names of the TN plane GEMMs it launched."""
    from windgnn_amd import _lib
    _lib.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        names = sorted(r["name"] for r in _lib.profile_read() if r["name"].startswith("pgemm_tn_kernel<"))
    finally:
        _lib.profile_enable(False)
    return out, names


def test_the_shapes_produce_the_splits_they_are_here_for():
    from windgnn_amd import _lib
    dev = _dev()
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    i = _lib.tn_split(_lib.Dims(48, 3, 34, 13, 102, MATH["f16x3"], 0, 0))
    assert i.merged == 1 and i.sk_ih > 1 and i.kchunk_ih * i.sk_ih > 144        # a partial last stage
    i = _lib.tn_split(_lib.Dims(32, 3, 34, 13, 102, MATH["f16x3"], 0, 0))
    assert i.merged == 1 and i.sk_ih == 1 and i.sk_hh == 1
    i = _lib.tn_split(_lib.Dims(2048, 2, 64, 13, 102, MATH["f16x3"], 0, 0))
    assert i.merged == 1 and i.workgroups == cus == 4 * i.sk_ih > i.sk_hh, (i.sk_ih, i.sk_hh, cus)   # four N blocks of dW_ih
    i = _lib.tn_split(_lib.Dims(2048, 8, 40, 13, 102, MATH["f16x3"], 0, 0))
    assert i.merged == 1 and i.workgroups == cus == i.sk_hh > 3 * i.sk_ih, (i.sk_ih, i.sk_hh, cus)   # three N blocks
    i = _lib.tn_split(_lib.Dims(40, 2, 64, 13, 102, MATH["f16x3"], 0, 0))
    assert i.workgroups == 4 * i.sk_ih > i.sk_hh                                         # four N blocks of dW_ih
    i = _lib.tn_split(_lib.Dims(16, 2, 34, 13, 127, MATH["f16x3"], 0, 0))
    assert i.workgroups == 4 * i.sk_ih > 2 * i.sk_hh                                     # two M blocks each


@pytest.mark.parametrize("math", ["f16x3", "f16x3g", "f16"])
@pytest.mark.parametrize("S,T,B,H", SHAPES)
def test_merged_launch_against_two_launches_and_the_oracle(S, T, B, H, math):
    from windgnn_amd import _lib
    from windgnn_amd.functional import (check_range_status, finish_step, gcn_gru_backward_mse_raw, gcn_gru_forward_raw)
    dev = _dev()
    A, X, L, p, Yo, loss_o, go = _case(S, T, B, H)
    Ad, Xd, Ld = A.to(dev), X.to(dev), L.to(dev)
    ps = [p[k].clone().to(dev) for k in PARAM_KEYS]
    mode = MATH[math]

    def run(deferred):
        gs = [torch.full_like(q, 7.0) for q in ps]
        loss = torch.zeros((), device=dev)
        Y, stash, d = gcn_gru_forward_raw(Ad, Xd, ps, mode, labels=Ld)
        if deferred:
            gcn_gru_backward_mse_raw(d, Ad, Xd, ps, Y, Ld, stash, gs, loss, 1.0, part=7 | 8 | _lib.BWD_DEFER)
            finish_step(d, ps, gs, 6)
        else:
            gcn_gru_backward_mse_raw(d, Ad, Xd, ps, Y, Ld, stash, gs, loss, 1.0, part=7 | 8)
        return Y, float(loss), gs

    results = {}
    for merged in (0, 1):
        for deferred in (False, True):
            with _merged(merged):
                results[merged, deferred], names = _tn_names(lambda: run(deferred))
            # the form under test really ran: one launch named <Tih+Thh..>, or the two stand-alone instances
            assert len(names) == (1 if merged else 2) and all(("+" in n) == bool(merged) for n in names), (merged, names)
    check_range_status(dev)
    Yr, lr, gr = results[0, False]
    for key, (Y, l, gs) in results.items():
        assert torch.equal(Y, Yr) and l == lr, key
        for k, a, b in zip(PARAM_KEYS, gs, gr):
            assert torch.equal(a, b), (key, k)
    # the fp64 oracle
    y_tol, g_tol = TOL[math]
    Y, l, gs = results[1, True]
    ey = max_abs(Y.cpu().reshape(Yo.shape), Yo)
    errs = {k: rel_to_max(gk.cpu(), go[k]) for k, gk in zip(PARAM_KEYS, gs)}
    print("%s S%d T%d B%d H%d: max|Y - oracle| %.2e, loss %.8f vs %.8f, gradients rel. to max %s"
          % (math, S, T, B, H, ey, l, loss_o, " ".join("%s=%.1e" % kv for kv in errs.items())))
    assert ey <= y_tol, ey
    assert abs(l - loss_o) <= (2e-3 if math == "f16" else 1e-5) * max(1.0, loss_o)
    for k, e in errs.items():
        assert e <= g_tol, (k, e)


def test_state_stash_rows_per_window_merged_against_two_launches():
    """wgnn_bwd_state_part: dW_hh's B operand takes window b's own [h0 | 1] row at every window start (the PW instances)."""
    from windgnn_amd.functional import gcn_gru_state_backward_raw, gcn_gru_state_forward_raw
    dev = _dev()
    S, T, B, H = 34, 3, 48, 102
    A, X, L, p, Yo, loss_o, go = _case(S, T, B, H)
    Ad, Xd = A.to(dev), X.to(dev)
    ps = [p[k].clone().to(dev) for k in PARAM_KEYS]
    g = torch.Generator().manual_seed(5)
    h0 = (torch.rand(B, H, generator=g) - 0.5).to(dev)
    dY = ((torch.rand(B, T, H, generator=g) - 0.5) * 1e-3).to(dev)
    dhn = ((torch.rand(B, H, generator=g) - 0.5) * 1e-3).to(dev)

    def run():
        gs = [torch.full_like(q, 7.0) for q in ps]
        dh0 = torch.full((B, H), 7.0, device=dev)
        Y, h_n, stash, d = gcn_gru_state_forward_raw(Ad, Xd, ps, MATH["f16x3"], h0=h0)
        gcn_gru_state_backward_raw(d, Ad, Xd, ps, Y, dY, dhn, stash, gs, dh0=dh0)
        return gs + [dh0]

    out = {}
    for merged in (0, 1):
        with _merged(merged):
            out[merged], names = _tn_names(run)
        assert len(names) == (1 if merged else 2) and all(("+" in n) == bool(merged) for n in names), (merged, names)
    for k, a, b in zip(PARAM_KEYS + ["dh0"], out[1], out[0]):
        assert torch.equal(a, b), k
    assert float(out[1][5].abs().max()) > 0                  # W_hh's gradient is there at all
