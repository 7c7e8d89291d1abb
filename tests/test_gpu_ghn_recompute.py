"""The gate records without gh_n (csrc/grux.hip, the RC instances; api.hip ghn_recompute) on the MI355X: in the stateless
fp32-I/O step of the split-fp16 modes the forward recurrence stores r | z and the BPTT kernel recomputes
gh_n = b_hn + W_hn h_{t-1} from the Y it loads anyway, with the forward's own fragments and product.  The environment variable
WGNN_GHN_RECOMPUTE = 0 keeps the three-component record r | z | gh_n; the library reads it at every call, so one process runs
both forms.  Everything the step computes must be the same BITS in both.

Shapes, S = 3 throughout (the recurrences never see S):
  H  15, 16, 17   the last wave's column tail: one wave short of a column, exactly full, a second wave with one column
     31, 32       the ones column at k = 31, the last of a 32-deep K step, and at k = 32, the first of the next (KS 1 -> 2)
     102          the benchmark's width (KS = 4, the BPTT instance <10>)
     127          the top of the widest bracket: every K slot of KS = 4 but the ones column's holds a hidden unit
  T  1            h_{-1} = 0 only: the prologue's tile is [0 | 1] and no step recomputes anything
     2            one recomputed step, from the one real h
     5            odd, and the tile parity wraps more than once (tiles of steps 4, 3, 2, 1, 0 in slots 0, 1, 0, 1, 0)
  B  16, 17, 33   one full workgroup; a second one with 15 empty rows; three workgroups
f16x3g runs the same kernels as f16x3 at these sizes (its single-plane dGI starts at B*T = 4096); both are run.
Tolerances of the oracle cases: those of tests/test_gpu_parity.py for these modes (imported, none added)."""
import ctypes
import functools
import os

import pytest
import torch

from conftest import PARAM_KEYS, load_fixture, max_abs, rel_to_max
from test_gpu_parity import G_TOL, Y_TOL

pytestmark = pytest.mark.gpu

MATH = {"f16x3": 1, "f16x3g": 3}
S = 3
HS = [15, 16, 17, 31, 32, 102, 127]
TS = [1, 2, 5]
BS = [16, 17, 33]
ORACLE_CASE = (5, 33, 102)                         # (T, B, H) of the case that is also held to the fp64 oracle, per mode
FILL = 0x5A                                        # what a stash holds before the forward: no kernel writes this byte pattern
ENV = "WGNN_GHN_RECOMPUTE"
assert ORACLE_CASE[0] in TS and ORACLE_CASE[1] in BS and ORACLE_CASE[2] in HS


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


class _form:
    """form 1: the r | z record (the library's default); form 0: r | z | gh_n."""

    def __init__(self, on):
        self.on = on

    def __enter__(self):
        self.prev = os.environ.get(ENV)
        os.environ[ENV] = str(self.on)

    def __exit__(self, *exc):
        if self.prev is None:
            del os.environ[ENV]
        else:
            os.environ[ENV] = self.prev


@functools.lru_cache(maxsize=None)
def _inputs(T, B, H):
    """Inputs of one shape: drawn once, shared by the math modes, never written to.  W_hh and b_hh are scaled up from the
    reference's initialisation so that gh_n is not small beside gi_n and h moves from step to step."""
    from oracle import windgnn_oracle as orc
    g = torch.Generator().manual_seed(7919 * H + 31 * B + T)
    A = torch.rand(S, S, generator=g) / S + 0.01
    X = torch.rand(B, T, S, 13, generator=g)
    L = torch.rand(B, T, H, generator=g)
    p = orc.init_params(S, 13, H, seed=H + T)
    p["gru.weight_hh_l0"] = p["gru.weight_hh_l0"] * 3.0
    p["gru.bias_hh_l0"] = p["gru.bias_hh_l0"] * 3.0 + 0.25
    return A, X, L, p


@functools.lru_cache(maxsize=None)
def _oracle(T, B, H):
    from oracle import windgnn_oracle as orc
    A, X, L, p = _inputs(T, B, H)
    Yo, loss_o, go = orc.train_step(A.double(), X.double(), L.double(), {k: v.double() for k, v in p.items()})
    return Yo, float(loss_o), go


def _filled_stash(d, dev, state=False):
    from windgnn_amd import _lib
    lib = _lib.load()
    n = (lib.wgnn_state_stash_bytes if state else lib.wgnn_stash_bytes)(ctypes.byref(d))
    return torch.full((n,), FILL, dtype=torch.uint8, device=dev)


def _step(form, Ad, Xd, Ld, ps, mode, d, poison=None):
    """One forward (wgnn_fwd_loss into a stash of FILL) and one deferred backward in `form`.  poison(stash), if given, runs
    between the two.  Returns Y, the forward's stash, the workspace the backward left (the dGI and dGHn planes and every
    split-K partial sum among it), the loss and the eight gradients after wgnn_finish."""
    from windgnn_amd import _lib
    from windgnn_amd.functional import _workspace, finish_step, gcn_gru_backward_mse_raw, gcn_gru_forward_raw
    dev = Xd.device
    with _form(form):
        Y, stash, d = gcn_gru_forward_raw(Ad, Xd, ps, mode, labels=Ld, stash=_filled_stash(d, dev))
        kept = stash.clone()
        if poison is not None:
            poison(stash)
        gs = [torch.full_like(q, 7.0) for q in ps]
        loss = torch.zeros((), device=dev)
        gcn_gru_backward_mse_raw(d, Ad, Xd, ps, Y, Ld, stash, gs, loss, 1.0, part=7 | 8 | _lib.BWD_DEFER)
        ws, ws_bytes = _workspace(d, dev)
        part = ws[:ws_bytes].clone()
        finish_step(d, ps, gs, 6)
    return Y, kept, part, float(loss), gs


@pytest.mark.parametrize("math", ["f16x3", "f16x3g"])
@pytest.mark.parametrize("B", BS)
@pytest.mark.parametrize("T", TS)
@pytest.mark.parametrize("H", HS)
def test_both_record_forms_give_the_same_bits(H, T, B, math):
    from windgnn_amd import _lib
    from windgnn_amd.functional import check_range_status
    dev = _dev()
    A, X, L, p = _inputs(T, B, H)
    Ad, Xd, Ld = A.to(dev), X.to(dev), L.to(dev)
    ps = [p[k].clone().to(dev) for k in PARAM_KEYS]
    mode = MATH[math]
    d = _lib.Dims(B, T, S, 13, H, mode, 0, 0)

    Y0, stash0, part0, loss0, g0 = _step(0, Ad, Xd, Ld, ps, mode, d)

    # ---- where the records are: the forms differ inside the gate region only, whose used part (three 1 KB components per
    # workgroup, step and wave) ends with the last gh_n of the three-component form
    Y1, stash1, _, _, _ = _step(1, Ad, Xd, Ld, ps, mode, d)
    differ = (stash0 != stash1).nonzero().flatten()
    assert differ.numel() > 0                                           # the switch does select another record
    region = ((B + 15) // 16) * T * ((H + 15) // 16) * 3 * 1024
    hi = int(differ[-1]) + 1
    lo = hi - region
    assert int(differ[0]) >= lo
    freed = slice(lo + region // 3 * 2, hi)                             # r | z records fill two thirds; the rest is left alone
    assert bool((stash1[freed] == FILL).all())
    assert not bool((stash0[freed] == FILL).all())

    # ---- the step in the new form, its freed third NaN between forward and backward
    def poison(stash):
        stash[freed] = 0xFF                                             # fp32 0xFFFFFFFF: NaN

    Y1, _, part1, loss1, g1 = _step(1, Ad, Xd, Ld, ps, mode, d, poison)
    check_range_status(dev)
    assert torch.equal(Y0, Y1)
    assert loss0 == loss1
    assert torch.equal(part0, part1)                                    # dGI / dGHn planes, every split-K partial sum
    for k, a, b in zip(PARAM_KEYS, g1, g0):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), k

    if (T, B, H) == ORACLE_CASE:
        Yo, loss_o, go = _oracle(T, B, H)
        ey = max_abs(Y1.cpu().reshape(Yo.shape), Yo)
        errs = {k: rel_to_max(gk.cpu(), go[k]) for k, gk in zip(PARAM_KEYS, g1)}
        print("%s T%d B%d H%d: max|Y - oracle| %.2e, loss %.8f vs %.8f, gradients rel. to max %s"
              % (math, T, B, H, ey, loss1, loss_o, " ".join("%s=%.1e" % kv for kv in errs.items())))
        assert ey <= Y_TOL, ey
        assert abs(loss1 - loss_o) <= 1e-5 * max(1.0, loss_o)
        for k, e in errs.items():
            assert e <= G_TOL, (k, e)


def _golden_step(name):
    fx = load_fixture(name)
    A, X, L = (torch.from_numpy(fx[k]) for k in ("A", "X", "L"))
    if X.dim() == 3:
        X, L = X.unsqueeze(0), L.unsqueeze(0)
    return fx, A, X, L.reshape(X.shape[0], X.shape[1], -1)


def test_16bit_io_keeps_the_three_component_record():
    """Y is rounded on the wire, so the BPTT kernel has no fp32 h_{t-1} to split as the forward did: the dispatcher stays on
    the stored gh_n.  The golden fixture's step with bf16 X / labels: the same stash bytes and the same results with the switch
    either way."""
    from windgnn_amd import _lib
    from windgnn_amd.functional import gcn_gru_backward_mse_raw, gcn_gru_forward_raw
    dev = _dev()
    fx, A, X, L = _golden_step("f1b_tiny_s3_t5_b3_h5")
    iodt = torch.bfloat16
    Ad, Xd, Ld = A.to(dev), X.to(iodt).to(dev), L.to(iodt).to(dev)
    ps = [fx["params"][k].clone().to(dev) for k in PARAM_KEYS]
    B, T, H = L.shape
    out = {}
    for form in (0, 1):
        with _form(form):
            d = _lib.Dims(B, T, X.shape[2], 13, H, MATH["f16x3"], 0, 0, _lib.IO_BF16)
            Y, stash, d = gcn_gru_forward_raw(Ad, Xd, ps, MATH["f16x3"], labels=Ld, stash=_filled_stash(d, dev))
            kept = stash.clone()
            gs = [torch.full_like(q, 7.0) for q in ps]
            loss = torch.zeros((), device=dev)
            gcn_gru_backward_mse_raw(d, Ad, Xd, ps, Y, Ld, stash, gs, loss, 1.0, part=7 | 8)
        out[form] = (Y, kept, float(loss), gs)
    assert out[0][0].dtype == iodt and torch.equal(out[0][0], out[1][0])
    assert torch.equal(out[0][1], out[1][1])                            # the same record, byte for byte
    assert out[0][2] == out[1][2]
    for k, a, b in zip(PARAM_KEYS, out[1][3], out[0][3]):
        assert torch.equal(a, b), k


def test_carried_state_keeps_the_three_component_record():
    """wgnn_fwd_state_stash / wgnn_bwd_state_part: h_{-1} is the caller's h0, which Y does not hold, and the state instances
    are out of scope as a whole.  With a random h0, dh_n and dh0: the same results with the switch either way."""
    from windgnn_amd.functional import gcn_gru_state_backward_raw, gcn_gru_state_forward_raw
    dev = _dev()
    fx, A, X, L = _golden_step("f1b_tiny_s3_t5_b3_h5")
    B, T, H = L.shape
    Ad, Xd = A.to(dev), X.to(dev)
    ps = [fx["params"][k].clone().to(dev) for k in PARAM_KEYS]
    g = torch.Generator().manual_seed(11)
    h0 = (torch.rand(B, H, generator=g) - 0.5).to(dev)
    dhn = (torch.rand(B, H, generator=g) - 0.5).to(dev)
    out = {}
    for form in (0, 1):
        with _form(form):
            gs = [torch.full_like(q, 7.0) for q in ps]
            dh0 = torch.full((B, H), 7.0, device=dev)
            Y, h_n, stash, d = gcn_gru_state_forward_raw(Ad, Xd, ps, MATH["f16x3"], h0=h0)
            dY = (2.0 * (Y - L.to(dev)) / Y.numel()).contiguous()
            gcn_gru_state_backward_raw(d, Ad, Xd, ps, Y, dY, dhn, stash, gs, dh0=dh0)
        out[form] = (Y, h_n, dh0, gs)
    for a, b in zip(out[0][:3], out[1][:3]):
        assert torch.equal(a, b)
    for k, a, b in zip(PARAM_KEYS, out[1][3], out[0][3]):
        assert torch.equal(a, b), k
