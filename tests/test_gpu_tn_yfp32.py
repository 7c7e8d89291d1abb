"""The dW_hh plane GEMM of the merged launch with its B rows taken from the caller's fp32 Y (csrc/pgemm.hip, TnProd::By;
api.hip hh_from_y) instead of the fp16 Y planes of the stash, on the MI355X.  WGNN_OPT_TN_MERGED selects, as in
tests/test_gpu_tn_merged.py: 0 is the plane form (two launches, the forward writes the planes), 1 the merged launch, which
in the stateless fp32-I/O step of the split-fp16 modes reads Y (and whose forward leaves the plane region alone).

Shapes (S, T, B, H) and what each can break:
  (3, 2, 1, 5)       a one-row Hprev, H far from a multiple of 8
  (3, 5, 3, 5)       t = 0 rows inside a stage, at rows 0, 5 and 10
  (7, 12, 4, 20)     48 rows: a stage boundary falls mid-window, with an odd shift
  (34, 24, 17, 102)  408 rows: five K chunks of 96 rows (wgnn_tn_split: sk = 6), the last a ragged 24, at the bench's H
  (7, 3, 11, 101)    33 rows: odd H, so the stage blocks start on 4-byte boundaries only; one row past a stage
  (3, 3, 16491, 5)   49 473 rows: 221 chunks of seven stages (sk = 256, kchunk = 224), the last with a one-row tail; T = 3, so
                     y_rem moves by 32 % 3 = 2 a stage and wraps inside a chunk, and both ring slots are rewritten after a read
  (3, 24, 2062, 101) 49 488 rows: seven stages again, a 16-row tail; odd H (4-byte stage boundaries, y_d4 realigned) and
                     y_step = 32 % 24 = 8
The last two hold the Y form to the plane form bit for bit past three stages (tests/instance_cases.py tn_products()).
f16x3g runs the same kernels as f16x3 at these sizes: its single-plane dGI, and with it the two-pass dW_hh, starts at
B*T = 4096, where tests/test_gpu_tn_merged.py (34, 24, 176, 102) compares the merged launch -- the Y form -- with the plane
form's two launches bit for bit.
Tolerances: those of tests/test_gpu_parity.py for these modes (imported, none added).  db_hh is the column sum of the
oracle's dGH (the GEMM's ones column), so its bound is the parity bound of gru.bias_hh_l0."""
import functools

import pytest
import torch

from conftest import PARAM_KEYS, load_fixture, max_abs, rel_to_max
from test_gpu_parity import G_TOL, IO_ROUND, Y_TOL

pytestmark = pytest.mark.gpu

MATH = {"f16x3": 1, "f16x3g": 3}
SHAPES = [(3, 2, 1, 5), (3, 5, 3, 5), (7, 12, 4, 20), (34, 24, 17, 102), (7, 3, 11, 101), (3, 3, 16491, 5), (3, 24, 2062, 101)]
FILL = 0x5A                                        # what a stash holds before the forward: no kernel writes this byte pattern


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


@functools.lru_cache(maxsize=None)
def _case(S, T, B, H):
    """Inputs and the fp64 oracle's step for one shape: computed once, shared by the math modes, never written to."""
    from oracle import windgnn_oracle as orc
    g = torch.Generator().manual_seed(613 * S + 17 * H + B)
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


def _filled_stash(d, dev):
    from windgnn_amd import _lib
    import ctypes
    n = _lib.load().wgnn_stash_bytes(ctypes.byref(d))
    return torch.full((n,), FILL, dtype=torch.uint8, device=dev)


@pytest.mark.parametrize("math", ["f16x3", "f16x3g"])
@pytest.mark.parametrize("S,T,B,H", SHAPES)
def test_y_form_against_the_plane_form_and_the_oracle(S, T, B, H, math):
    from windgnn_amd import _lib
    from windgnn_amd.functional import (_workspace, check_range_status, finish_step, gcn_gru_backward_mse_raw,
                                        gcn_gru_forward_raw)
    dev = _dev()
    A, X, L, p, Yo, loss_o, go = _case(S, T, B, H)
    Ad, Xd, Ld = A.to(dev), X.to(dev), L.to(dev)
    ps = [p[k].clone().to(dev) for k in PARAM_KEYS]
    mode = MATH[math]
    d = _lib.Dims(B, T, S, 13, H, mode, 0, 0)

    # ---- the forwards: the plane form writes the planes, the Y form leaves their region as it found it
    with _merged(0):
        Y, stash, d = gcn_gru_forward_raw(Ad, Xd, ps, mode, labels=Ld, stash=_filled_stash(d, dev))
    with _merged(1):
        Y1, stash1, _ = gcn_gru_forward_raw(Ad, Xd, ps, mode, labels=Ld, stash=_filled_stash(d, dev))
    assert torch.equal(Y, Y1)
    differ = (stash != stash1).nonzero().flatten()
    assert differ.numel() > 0                                           # the plane form wrote planes the other did not
    lo, hi = int(differ[0]), int(differ[-1]) + 1                        # the plane region (up to bytes that equal FILL)
    Hp = 32 * ((H + 1 + 31) // 32)
    assert hi - lo <= 2 * (B * T + 1) * Hp * 2                          # two planes of B*T + 1 rows of Hp halfs
    assert hi - lo > (B * T) * Hp * 2                                   # ... and it reaches into the second one
    assert bool((stash1[lo:hi] == FILL).all())

    def backward(form, st):
        """One deferred backward in `form` on the plane form's forward: the workspace it leaves (the dW_hh / db_hh partial
        sums among it), then the eight gradients and the loss."""
        gs = [torch.full_like(q, 7.0) for q in ps]
        loss = torch.zeros((), device=dev)
        with _merged(form):
            _, names = _tn_names(lambda: gcn_gru_backward_mse_raw(d, Ad, Xd, ps, Y, Ld, st, gs, loss, 1.0,
                                                                  part=7 | 8 | _lib.BWD_DEFER))
        assert len(names) == (1 if form else 2) and all(("+" in n) == bool(form) for n in names), (form, names)
        ws, ws_bytes = _workspace(d, dev)
        part = ws[:ws_bytes].clone()
        finish_step(d, ps, gs, 6)
        return part, float(loss), gs

    part0, loss0, g0 = backward(0, stash)
    part1, loss1, g1 = backward(1, stash)
    check_range_status(dev)
    assert torch.equal(part0, part1)                                    # every partial sum, dW_hh's and db_hh's among them
    assert loss0 == loss1
    for k, a, b in zip(PARAM_KEYS, g1, g0):
        assert torch.equal(a, b), k

    # ---- the planes are unread: NaN all over them changes nothing in the Y form (and everything in the plane form)
    poisoned = stash.clone()
    poisoned[lo:hi] = 0xFF                                              # fp16 0xFFFF: NaN
    _, _, gp = backward(1, poisoned)
    for k, a, b in zip(PARAM_KEYS, gp, g0):
        assert bool(torch.isfinite(a).all()) and torch.equal(a, b), k
    _, _, gq = backward(0, poisoned)
    assert bool(torch.isnan(gq[5]).any())                               # W_hh's gradient: the plane form does read them
    try:
        check_range_status(dev)                                         # (whatever that run reported is not the next test's)
    except RuntimeError:
        pass

    # ---- the fp64 oracle
    ey = max_abs(Y.cpu().reshape(Yo.shape), Yo)
    errs = {k: rel_to_max(gk.cpu(), go[k]) for k, gk in zip(PARAM_KEYS, g1)}
    print("%s S%d T%d B%d H%d: max|Y - oracle| %.2e, loss %.8f vs %.8f, gradients rel. to max %s"
          % (math, S, T, B, H, ey, loss1, loss_o, " ".join("%s=%.1e" % kv for kv in errs.items())))
    assert ey <= Y_TOL, ey
    assert abs(loss1 - loss_o) <= 1e-5 * max(1.0, loss_o)
    for k, e in errs.items():
        assert e <= G_TOL, (k, e)
    assert errs["gru.bias_hh_l0"] <= G_TOL                              # the ones column: column sums of dGH


def _golden_step(name):
    fx = load_fixture(name)
    A, X, L = (torch.from_numpy(fx[k]) for k in ("A", "X", "L"))
    if X.dim() == 3:
        X, L = X.unsqueeze(0), L.unsqueeze(0)
    return fx, A, X, L.reshape(X.shape[0], X.shape[1], -1)


def test_16bit_io_keeps_the_planes():
    """Y is rounded on the wire: the planes hold what it was rounded from, so the dispatcher stays on them (a B operand read
    from Y as fp32 would be noise).  The golden fixture's step with fp16 X / labels: the merged launch against the plane
    form's two launches bit for bit, and against the fp64 oracle on the rounded inputs at the bounds of
    tests/test_gpu_parity.py::test_16bit_io_against_oracle_on_the_rounded_inputs."""
    from oracle import windgnn_oracle as orc
    from windgnn_amd.functional import gcn_gru_backward_mse_raw, gcn_gru_forward_raw
    dev = _dev()
    fx, A, X, L = _golden_step("f1b_tiny_s3_t5_b3_h5")
    iodt = torch.float16
    X, L = X.to(iodt), L.to(iodt)
    Yo, loss_o, go = orc.train_step(A.double(), X.double(), L.double(), {k: v.double() for k, v in fx["params"].items()})
    Ad, Xd, Ld = A.to(dev), X.to(dev), L.to(dev)
    ps = [fx["params"][k].clone().to(dev) for k in PARAM_KEYS]
    out = {}
    for form in (0, 1):
        with _merged(form):
            Y, stash, d = gcn_gru_forward_raw(Ad, Xd, ps, MATH["f16x3"], labels=Ld)
            gs = [torch.full_like(q, 7.0) for q in ps]
            loss = torch.zeros((), device=dev)
            _, names = _tn_names(lambda: gcn_gru_backward_mse_raw(d, Ad, Xd, ps, Y, Ld, stash, gs, loss, 1.0, part=7 | 8))
        assert len(names) == (1 if form else 2), (form, names)
        out[form] = (Y, stash, gs)
    assert Y.dtype == iodt and torch.equal(out[0][0], out[1][0])
    assert max_abs(out[1][0].float().cpu().reshape(Yo.shape), Yo) <= Y_TOL + IO_ROUND[iodt]
    for k, a, b in zip(PARAM_KEYS, out[1][2], out[0][2]):
        assert torch.equal(a, b), k
        assert rel_to_max(a.cpu(), go[k]) <= G_TOL, k


def test_carried_state_keeps_the_planes():
    """wgnn_fwd_state_stash / wgnn_bwd_state_part: window b's t = 0 row is its own [h0 | 1] plane row, which Y does not hold.
    With h0 = None (zeros) the gradients are the golden fixture's; with a random h0 the merged launch equals the two launches
    bit for bit (a B operand formed from Y would have zeros at t = 0)."""
    from windgnn_amd.functional import gcn_gru_state_backward_raw, gcn_gru_state_forward_raw
    dev = _dev()
    fx, A, X, L = _golden_step("f1b_tiny_s3_t5_b3_h5")
    B, T, H = L.shape
    Ad, Xd = A.to(dev), X.to(dev)
    ps = [fx["params"][k].clone().to(dev) for k in PARAM_KEYS]
    g = torch.Generator().manual_seed(11)
    h0 = (torch.rand(B, H, generator=g) - 0.5).to(dev)

    def run(h0, dY_of):
        gs = [torch.full_like(q, 7.0) for q in ps]
        Y, h_n, stash, d = gcn_gru_state_forward_raw(Ad, Xd, ps, MATH["f16x3"], h0=h0)
        _, names = _tn_names(lambda: gcn_gru_state_backward_raw(d, Ad, Xd, ps, Y, dY_of(Y), None, stash, gs))
        return Y, gs, names

    mse = lambda Y: (2.0 * (Y - L.to(dev)) / Y.numel()).contiguous()
    Y, gs, names = run(None, mse)
    assert len(names) == 1 and "+" in names[0], names
    assert max_abs(Y.cpu().reshape(fx["Y"].shape), fx["Y"]) <= Y_TOL
    for k, gk in zip(PARAM_KEYS, gs):
        assert rel_to_max(gk.cpu(), fx["grads"][k]) <= G_TOL, k
    out = {}
    for form in (0, 1):
        with _merged(form):
            out[form] = run(h0, mse)
        assert len(out[form][2]) == (1 if form else 2), out[form][2]
    assert torch.equal(out[0][0], out[1][0])
    for k, a, b in zip(PARAM_KEYS, out[1][1], out[0][1]):
        assert torch.equal(a, b), k
    assert not torch.equal(out[1][1][5], gs[5])                         # h0 matters to W_hh's gradient
