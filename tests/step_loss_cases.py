"""The cases of training on a loss spec on materialised windows (TrainStep.step / forward_backward with loss= / huber_delta= /
loss_from= / missing_labels=, functional.loss_spec_grad), shared by tests/test_step_loss_host.py and
tests/test_gpu_step_loss.py.  No GPU is needed to import or to call anything here.

Shapes (S, T, B, H, k of a k-NN graph in CSR or None), the smallest that reach each recurrence and backward path:

    small  (7, 12, 4, 21)      odd S * 13, the register-resident recurrences
    real   (34, 24, 4, 102)    the real widths; also with 16-bit I/O
    wide   (34, 5, 4, 129)     the wide-GRU path
    csr    (65, 5, 4, 150)     a 6-NN graph in CSR (S > 64 has no dense path), wide
    call   (7, 168, 1, 21)     the reference's call length, L handed over as [T, H]

The reference is the fp64 oracle on the inputs the device reads (rounded to the I/O type first): orc.forward, the loss and dY of
the spec formed by tests/series_lossfn_cases.py's loss_and_dy on the oracle's Y, orc.backward fed that dY.

Labels are U[0, 1) for Huber (delta 0.25 splits the residuals into both arms, and rho' = clamp is continuous).  sign(r) must not
hang on the device's rounding of Y, so the L1 labels are moved away from Y, which lies in (-1, 1), as the series suite moves
them: even columns up by 2, odd columns down by 3 -- both signs occur and |r| > 1 everywhere.

The bars.  The fp32-grade modes (f32, f16x3, f16x3g; B * T is below 4096 rows in every shape, so f16x3g runs f16x3's kernels) on
fp32 I/O: validate_cases.TOL = 1e-4 on Y and each of the 8 gradients relative to the tensor's max, and on the loss relative to
the oracle's.  The one-pass f16 mode and the 16-bit I/O cases take the bars tests/test_gpu_parity.py holds that mode's MSE step
to, restated below with the line each comes from."""
import functools

import torch

import series_lossfn_cases as lc
import validate_cases as vc

SHAPES = {"small": (7, 12, 4, 21, None), "real": (34, 24, 4, 102, None), "wide": (34, 5, 4, 129, None),
          "csr": (65, 5, 4, 150, 6), "call": (7, 168, 1, 21, None)}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16, "fp16": torch.float16}
DELTA = lc.DELTA
TOL = vc.TOL
KINDS = ("l1", "huber")
MASKS = ("none", "tenth")
HALF_DELTA = 1e6                             # Huber with every residual in the quadratic arm: half the mean square

# tests/test_gpu_parity.py, the bars of the MSE step in the one-pass mode and with 16-bit I/O
Y_TOL = 1e-4                                 # :13   max-abs on Y, the fp32-grade modes
G_TOL = 1e-4                                 # :14   gradients relative to the tensor's max, the fp32-grade modes
F16_Y_TOL = 2e-2                             # :463  max-abs on Y, math "f16"
F16_G_TOL = 5e-2                             # :464  gradients relative to the tensor's max, math "f16"
IO_ROUND = {"fp32": 0.0, "fp16": 2.5e-4, "bf16": 2.0e-3}       # :925  Y is rounded once to the I/O type: added to Y's bar (:943)
LOSS_F16 = 2e-3                              # :650, :951  |loss - oracle| <= 2e-3 * max(1, oracle) with math "f16" ...
LOSS_IO = 1e-5                               # :951  ... and 1e-5 * max(1, oracle) with f16x3 on 16-bit I/O

# (shape, math mode, I/O type) of the parity grid
CASES = ([("small", m, "fp32") for m in vc.MODES] + [("real", m, "fp32") for m in vc.MODES] +
         [("real", "f16x3", "bf16"), ("real", "f16", "fp16"), ("wide", "f32", "fp32"), ("wide", "f16x3", "fp32"),
          ("csr", "f16x3", "fp32"), ("call", "f32", "fp32"), ("call", "f16x3", "fp32")])


def bars(mode, io):
    """(Y's error measure and bar, the gradients' bar relative to the tensor's max, loss bar as a function of the oracle's
    loss) of a math mode and I/O type (module docstring)."""
    if mode != "f16" and io == "fp32":
        return ("rel_to_max", TOL), TOL, lambda ref: TOL * abs(ref)
    if mode == "f16":
        return ("max_abs", F16_Y_TOL + IO_ROUND[io]), F16_G_TOL, lambda ref: LOSS_F16 * max(1.0, abs(ref))
    return ("max_abs", Y_TOL + IO_ROUND[io]), G_TOL, lambda ref: LOSS_IO * max(1.0, abs(ref))


def t_froms(T):
    return sorted({0, 2, T - 1})


class Case:
    pass


@functools.lru_cache(maxsize=None)
def case(name, io="fp32"):
    """Host tensors of a shape as the device reads them (X and the labels rounded to the I/O type, held as fp32), the
    parameters and the fp64 oracle's forward.  Computed once, shared, never modified."""
    from oracle import windgnn_oracle as orc
    S, T, B, H, k = SHAPES[name]
    dt = DTYPES[io]
    c = Case()
    c.name, c.io, c.S, c.T, c.B, c.H, c.csr = name, io, S, T, B, H, None
    g = torch.Generator().manual_seed(5200 + 31 * S + 7 * T + B + 101 * H)
    if k:
        from windgnn_amd.graph import CsrAdjacency, build_knn_adjacency, synthetic_station_coords
        c.csr = CsrAdjacency(*build_knn_adjacency(synthetic_station_coords(S, seed=S), k))
        c.A = c.csr.dense()
    else:
        c.A = torch.rand(S, S, generator=g) / S + 0.01
    c.X = torch.rand(B, T, S, 13, generator=g).to(dt).float()
    draw = torch.rand(B, T, H, generator=g)
    far = draw.clone()
    far[:, :, 0::2] += 2.0
    far[:, :, 1::2] -= 3.0
    c.L = {"mse": draw.to(dt).float(), "huber": draw.to(dt).float(), "l1": far.to(dt).float()}
    c.hit = torch.rand(B, T, H, generator=g) < 0.1
    c.p = orc.init_params(S, 13, H, seed=S + H)
    c.p64 = {key: v.double() for key, v in c.p.items()}
    c.Yo, c.cache = orc.forward(c.A.double(), c.X.double(), c.p64)
    return c


def labels(c, kind, mask):
    """[B, T, H] fp32: the labels of a kind with the mask's entries NaN (a new tensor)."""
    L = c.L[kind].clone()
    if mask == "tenth":
        L[c.hit] = float("nan")
    elif mask == "all":
        L[:] = float("nan")
    else:
        assert mask == "none"
    return L


class Ref:
    pass


@functools.lru_cache(maxsize=None)
def reference(name, io, kind, delta, t_from, mask):
    """The oracle's loss, count and 8 gradients of a spec on a case: computed once, shared, never modified."""
    from oracle import windgnn_oracle as orc
    c = case(name, io)
    q = Ref()
    q.L = labels(c, kind, mask)
    loss, dY, q.m = lc.loss_and_dy(c.Yo, q.L.double(), kind, delta, t_from, int(mask != "none"))
    q.loss = float(loss)
    q.gm = orc.backward(c.A.double(), c.X.double(), c.p64, c.Yo, c.cache, dY)
    return q


TRAIN = dict(loss="l1", loss_from=2, missing_labels=True)      # the three-step runs: L1 with 10 % NaN from step 2
STEPS = 3
# Adam's update lr * g / (|g| + eps) is sign-like where a gradient element is rounding noise (tests/test_gpu_parity.py:1089);
# with this eps on both sides the update is a smooth function of g, as tests/test_gpu_state_train.py:215 has it
EPS = 1e-3


@functools.lru_cache(maxsize=None)
def trajectory(name, max_norm=None):
    """The oracle's STEPS Adam steps (lr 1e-3, eps EPS) on a case with the loss of TRAIN: (losses, parameters after, the
    unclipped gradient norms).  max_norm: torch.nn.utils.clip_grad_norm_'s coefficient on the gradients before Adam."""
    from oracle import windgnn_oracle as orc
    c = case(name)
    A, X, L = c.A.double(), c.X.double(), labels(c, "l1", "tenth").double()
    p = dict(c.p64)
    state = orc.adam_init(p)
    losses, norms = [], []
    for _ in range(STEPS):
        Y, cache = orc.forward(A, X, p)
        loss, dY, _ = lc.loss_and_dy(Y, L, "l1", 0.0, TRAIN["loss_from"], 1)
        losses.append(float(loss))
        g = orc.backward(A, X, p, Y, cache, dY)
        norms.append(float(torch.sqrt(sum((v ** 2).sum() for v in g.values()))))
        if max_norm is not None:
            coef = min(1.0, max_norm / (norms[-1] + 1e-6))
            g = {k: v * coef for k, v in g.items()}
        p = orc.adam_step(p, g, state, eps=EPS)
    return losses, p, norms


# ---- the host grid of functional.loss_spec_grad --------------------------------------------------------------------------------
HOST_SHAPE = (3, 5, 21)                      # B, T, H
HOST_MASKS = ("none", "tenth", "column", "all")
HOST_KINDS = ("mse", "l1", "huber")


@functools.lru_cache(maxsize=None)
def host_draw(io, mask):
    """(Y, L) [B, T, H] in the I/O type: Y in (-1, 1), L in [0, 1) with the mask's entries NaN."""
    B, T, H = HOST_SHAPE
    g = torch.Generator().manual_seed(77)
    Y = (torch.rand(B, T, H, generator=g) * 2 - 1).to(DTYPES[io])
    L = torch.rand(B, T, H, generator=g).to(DTYPES[io])
    hit = torch.rand(B, T, H, generator=g) < 0.1
    if mask == "tenth":
        L[hit] = float("nan")
    elif mask == "column":
        L[:, :, 4] = float("nan")
    elif mask == "all":
        L[:] = float("nan")
    return Y, L


def autograd_spec(Y, L, kind, delta, t_from, masked, grad_scale=1.0):
    """(loss, dY, m) of the spec by fp64 autograd of its formulas: loss = sum over M of rho(Y - L) / m, dY = grad_scale *
    d loss / d Y.  m = 0: (NaN, zeros, 0)."""
    Y64 = Y.detach().double().clone().requires_grad_(True)
    L64 = L.detach().double()
    on = lc.counted(L64, t_from, masked)
    m = int(on.sum())
    if m == 0:
        return float("nan"), torch.zeros_like(L64), 0
    r = Y64[on] - L64[on]
    loss = vc.rho(r, kind, delta).sum() / m
    loss.backward()
    return float(loss.detach()), Y64.grad * grad_scale, m
