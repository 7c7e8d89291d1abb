"""Lattice inputs for the parity suites: every graph-convolution input and parameter lies on a coarse dyadic grid, so every
pre-activation of both layers is an exact dyadic number -- bit-identical under any summation order in fp32 and in fp16 hi / lo
planes -- and, being an ODD multiple of its grid step, bounded away from zero at every problem size.  The ReLU masks are live
(they differ between stations), the conv biases are not zero and A is not symmetric, yet no mask can sit on a rounding
boundary: a wrong kernel cannot be blamed on a tie and a tie cannot hide a wrong kernel.  A plain module: nothing here is
collected.  tests/test_lattice_inputs_host.py qualifies every shape below on the fp64 oracle alone, tests/test_gpu_lattice.py
runs the cases on the GPU.

The grids (F = 13 features):
  X            multiples of 1/2 in [-1, 1]                         (sparse draw: of 1)
  A            rows of 1 .. 3 non-zeros at random columns, {1}, {1/2, 1/2} or {1/2, 1/4, 1/4}: row sums 1, asymmetric
               (sparse draw: 1 .. 6 non-zeros, multiples of 1/8, row sums 7/8 or 1: ragged rows, empty rows in A^T)
  conv weights round(2 randn).clamp(-3, 3) / 2                     (sparse draw, conv2: round(1.5 randn).clamp(-2, 2))
  conv1.bias   odd multiples of 1/32 in (-1/2, 1/2);  conv2.bias   odd multiples of 1/512 in (-1/4, 1/4)
  GRU tensors  oracle.init_params' own; gru.weight_ih_l0 times 2^shift where the table says so
so A X W1 is a multiple of 1/16 and Z1 an odd multiple of 1/32; H1 is a multiple of 1/32, A H1 W2 one of 1/256 and Z2 an odd
multiple of 1/512 (the sparse draw trades the halves of X and W2 for the eighths of A).  X, A, A X, H1, A H1 and both weights
are exact in fp16, so the forward masks of the one-pass fp16 mode are exact too."""
import functools

import torch

F = 13
ROW_VALUES = {1: [1.0], 2: [0.5, 0.5], 3: [0.5, 0.25, 0.25], 4: [0.25, 0.25, 0.25, 0.125],
              5: [0.25, 0.25, 0.125, 0.125, 0.125], 6: [0.25, 0.125, 0.125, 0.125, 0.125, 0.125]}


def _randint(g, lo, hi, shape):
    return torch.randint(lo, hi + 1, shape, generator=g).double()


def lattice_adjacency(S, g, sparse=False):
    """Dense fp32 [S, S]: each row 1 .. 3 (sparse: 1 .. 6) non-zeros of ROW_VALUES at random distinct columns."""
    A = torch.zeros(S, S, dtype=torch.float64)
    kmax = min(6 if sparse else 3, S)
    ks = torch.randint(1, kmax + 1, (S,), generator=g).tolist()
    for i, k in enumerate(ks):
        A[i, torch.randperm(S, generator=g)[:k]] = torch.tensor(ROW_VALUES[k], dtype=torch.float64)
    return A.float()


def lattice_features(g, shape, sparse=False):
    return (_randint(g, -1, 1, shape) if sparse else _randint(g, -2, 2, shape) / 2).float()


def lattice_conv(g, Fi=F, Fo=F, sparse=False, layer=1):
    """(W [Fi, Fo], b [Fo]) of one layer on the grid of `layer` (1: bias on odd 32nds, 2: on odd 512ths)."""
    if sparse and layer == 2:
        W = torch.round(1.5 * torch.randn(Fi, Fo, generator=g, dtype=torch.float64)).clamp(-2, 2)
    else:
        W = torch.round(2 * torch.randn(Fi, Fo, generator=g, dtype=torch.float64)).clamp(-3, 3) / 2
    b = (2 * _randint(g, -8, 7, (Fo,)) + 1) / 32 if layer == 1 else (2 * _randint(g, -64, 63, (Fo,)) + 1) / 512
    return W.float(), b.float()


def lattice_params(S, H, g, seed, sparse=False, shift=0):
    from oracle import windgnn_oracle as orc
    p = orc.init_params(S, F, H, seed=seed)
    p["conv1.weight"], p["conv1.bias"] = lattice_conv(g, sparse=sparse, layer=1)
    p["conv2.weight"], p["conv2.bias"] = lattice_conv(g, sparse=sparse, layer=2)
    p["gru.weight_ih_l0"] = p["gru.weight_ih_l0"] * 2.0 ** shift
    return p


class Draw:
    pass


@functools.lru_cache(maxsize=4)
def draw(S, T, B, H, sparse=False, shift=0, seed=0):
    """The window-major draw of a shape: A (dense fp32; sparse: to be handed over with CsrAdjacency.from_dense), X [B, T, S, 13],
    labels in [0, 1), the 8 parameters, and the signed h0 / dY / dh_n of the carried-state route (tests/test_gpu_state_train.py's).
    Shared: never written to."""
    d = Draw()
    g = torch.Generator().manual_seed(7000 + 31 * S + 7 * T + B + 101 * H + 977 * seed)
    d.A = lattice_adjacency(S, g, sparse)
    d.X = lattice_features(g, (B, T, S, F), sparse)
    d.p = lattice_params(S, H, g, S + H + seed, sparse, shift)
    d.L = torch.rand(B, T, H, generator=g)
    d.h0 = torch.rand(B, H, generator=g) * 1.6 - 0.8
    d.dY = torch.randn(B, T, H, generator=g) * 1e-3
    d.dhn = torch.randn(B, H, generator=g) * 1e-3
    return d


@functools.lru_cache(maxsize=4)
def draw_series(S, H, rows, T, stride, n, seed=0):
    """The series draw: A, the feature series [rows, S, 13] on the grid, a signed dY [n, T, H] (tests/test_gpu_series.py's), a
    label series [rows, H] in [0, 1) and the parameters."""
    d = Draw()
    g = torch.Generator().manual_seed(7100 + 131 * seed + S * 7 + rows + H)
    d.A = lattice_adjacency(S, g)
    d.Xs = lattice_features(g, (rows, S, F))
    d.p = lattice_params(S, H, g, S + H + seed)
    d.dY = (torch.rand(n, T, H, generator=g) * 2 - 1) * 1e-2
    d.Ls = torch.rand(rows, H, generator=g)
    return d


def draw_layer(S, Fi, Fo, nt, seed=0):
    """One general GraphConvLayer: A, X [nt, S, Fi], W, b (odd 32nds: Z is an odd multiple of 1/32) and a signed dout."""
    d = Draw()
    g = torch.Generator().manual_seed(7200 + 31 * S + 7 * Fi + Fo + 977 * seed)
    d.A = lattice_adjacency(S, g)
    d.X = lattice_features(g, (nt, S, Fi))
    d.W, d.b = lattice_conv(g, Fi, Fo, layer=1)
    d.dout = torch.randn(nt, S, Fo, generator=g)
    return d


# ---- measurements on the fp64 reference ---------------------------------------------------------------------------------
def preacts(A, X, W1, b1, W2=None, b2=None):
    """fp64 pre-activations [Z1] or [Z1, Z2] and, ahead of them, the tensors the one-pass fp16 mode holds as fp16."""
    A, X = A.double(), X.double()
    P1 = torch.matmul(A, X)
    Z1 = torch.matmul(P1, W1.double()) + b1.double()
    if W2 is None:
        return [Z1], [X, A, P1, W1]
    H1 = torch.relu(Z1)
    P2 = torch.matmul(A, H1)
    Z2 = torch.matmul(P2, W2.double()) + b2.double()
    return [Z1, Z2], [X, A, P1, H1, P2, W1, W2]


def measure(Zs, steps):
    """Per layer: is Z / step an odd integer below 2^24, min |Z| / max |Z|, the share of (.., column) pairs whose mask differs
    between stations (dim -2) and the live fraction."""
    out = []
    for Z, step in zip(Zs, steps):
        q = Z / step
        live = Z > 0
        varies = live.any(-2) & ~live.all(-2)
        out.append(dict(odd=bool((q == q.round()).all() and (q.round().long() % 2 == 1).all()),
                        qmax=float(q.abs().max()), margin=float(Z.abs().min() / Z.abs().max()),
                        varies=float(varies.double().mean()), live=float(live.double().mean())))
    return out


def round16(t):
    return t.half().to(t.dtype)


def fp64_step(A, X, L, p, f16_operands=False):
    """Y, loss and the 8 gradients of mean((Y - L)^2) by fp64 autograd.  f16_operands: g and the four GRU tensors enter the
    recurrence rounded to fp16 (straight through in the backward) -- the operand rounding of the one-pass fp16 mode, whose
    masks are exact on these inputs; its distance from the plain step is the reference figure of an 'f16' case."""
    from oracle.windgnn_oracle import PARAM_KEYS
    ste = (lambda t: t + (round16(t) - t).detach()) if f16_operands else (lambda t: t)
    leaves = {k: p[k].double().clone().requires_grad_(True) for k in PARAM_KEYS}
    A, X, L = A.double(), X.double(), L.double()
    h = torch.relu(torch.matmul(torch.matmul(A, X), leaves["conv1.weight"]) + leaves["conv1.bias"])
    h = torch.relu(torch.matmul(torch.matmul(A, h), leaves["conv2.weight"]) + leaves["conv2.bias"])
    B, T, S, _ = X.shape
    H = p["gru.weight_hh_l0"].shape[1]
    Y, _ = torch._VF.gru(ste(h.reshape(B, T, S * F)), torch.zeros(1, B, H, dtype=torch.float64),
                         [ste(leaves[k]) for k in PARAM_KEYS[4:]], True, 1, 0.0, False, False, True)
    loss = ((Y - L) ** 2).mean()
    loss.backward()
    return Y.detach(), float(loss), {k: leaves[k].grad for k in PARAM_KEYS}


def dg_of_mse(g, p, L):
    """d mean((Y - L)^2) / d g by fp64 autograd through the recurrence alone (g [B, T, S * 13] as a leaf)."""
    from oracle.windgnn_oracle import PARAM_KEYS
    gl = g.detach().double().clone().requires_grad_(True)
    B, H = g.shape[0], p["gru.weight_hh_l0"].shape[1]
    Y, _ = torch._VF.gru(gl, torch.zeros(1, B, H, dtype=torch.float64), [p[k].double() for k in PARAM_KEYS[4:]],
                         True, 1, 0.0, False, False, True)
    (dg,) = torch.autograd.grad(((Y - L.double()) ** 2).mean(), gl)
    return dg


MUTATIONS = ("conv1 mask of the next station", "conv2 mask of the next station", "conv1 bias dropped", "conv2 bias dropped",
             "conv2 bias rolled by one column", "A in place of A^T")


def mutation_effects(A, X, L, p):
    """What each wrong kernel of MUTATIONS would do, on the fp64 oracle: the largest of max |dY| and the relative-to-max change
    of any gradient.  The three backward mutations leave the forward alone and move the four conv gradients only."""
    from conftest import max_abs, rel_to_max
    from oracle import windgnn_oracle as orc
    A, X, L = A.double(), X.double(), L.double()
    p = {k: v.double() for k, v in p.items()}
    Y, loss, grads = orc.train_step(A, X, L, p)
    g, cache = orc.gcn2_forward(A, X, p)
    dg = dg_of_mse(g, p, L).reshape(X.shape)
    conv = [k for k in orc.PARAM_KEYS if k.startswith("conv")]
    base = orc.gcn2_backward(A, p, cache, dg)
    assert max(rel_to_max(base[k], grads[k]) for k in conv) < 1e-10       # the autograd dg is the oracle's own
    B, T, S, _ = X.shape

    def bwd(A_=A, **swap):
        got = orc.gcn2_backward(A_, p, dict(cache, **swap), dg)
        return max(rel_to_max(got[k], base[k]) for k in conv)

    def fwd(**swap):
        Ym, _, gm = orc.train_step(A, X, L, dict(p, **swap))
        return max([max_abs(Ym, Y)] + [rel_to_max(gm[k], grads[k]) for k in orc.PARAM_KEYS])

    return {
        MUTATIONS[0]: bwd(H1=torch.roll(cache["H1"], -1, 2)),
        MUTATIONS[1]: bwd(g=torch.roll(cache["g"].reshape(B, T, S, F), -1, 2).reshape(B, T, S * F)),
        MUTATIONS[2]: fwd(**{"conv1.bias": torch.zeros_like(p["conv1.bias"])}),
        MUTATIONS[3]: fwd(**{"conv2.bias": torch.zeros_like(p["conv2.bias"])}),
        MUTATIONS[4]: fwd(**{"conv2.bias": torch.roll(p["conv2.bias"], 1)}),
        MUTATIONS[5]: bwd(A_=A.t()),
    }


# ---- the cases ----------------------------------------------------------------------------------------------------------
def _nt(S):
    return (S + 15) // 16


T_, B_, H_ = 3, 17, 9
BIG_B = 1366              # 3 x 1366 = 4098 >= 4096: f16x3g's single-plane dGI / dg
W16 = (2, 8192, 4)        # T, B, H of gcn32_bwd_kernel's 16-wave form: 2 x 8192 = 16 384 rows
# ... and its gru.weight_ih_l0 shift per S: at S = 34, H = 4 (weights up to 1/2, 442 inputs up to 30) the oracle's own fp32 Y is
# 1.5e-5 off its fp64 one with the weights as drawn, above a tenth of the bar
W16_SHIFT = {5: 0, 17: 0, 34: -2}

# One-pass fp16 cases: (Y, loss, worst gradient) of fp64_step(f16_operands=True) against fp64_step() on the case's inputs -- the
# mode's operand rounding measured on the reference alone (tests/test_lattice_inputs_host.py recomputes them).  A case's bar is
# the larger of the imported bar (F16_Y_TOL = 2e-2, 2e-3 on the loss, F16_G_TOL = 5e-2) and twice its figure.
F16_FIGURES = {                      # every figure is below its imported bar: the bars of the 'f16' cases are the imported ones
    "gcnx1_f16": (2.70e-3, 3.33e-6, 1.21e-3), "gcnx2_f16": (4.13e-3, 5.29e-6, 3.90e-3),
    "gcnx3_f16": (5.71e-3, 2.51e-5, 7.80e-3), "gcnx4_f16": (4.03e-3, 7.46e-5, 4.11e-3),
    "gcngi1_fused_f16": (2.70e-3, 3.33e-6, 1.21e-3), "gcngi2_fused_f16": (4.13e-3, 5.29e-6, 3.90e-3),
    "gcngi3_fused_f16": (5.71e-3, 2.51e-5, 7.80e-3), "csr200_f16": (1.61e-3, 8.10e-6, 2.22e-3),
}

# Window-major cases: (id, keys, S, T, B, H, math, io, state, route, sparse, shift).  keys: instance keys of
# instance_cases.plan() for the dense routes, literal profiler names for CSR.
CASES = []


def _case(cid, keys, S, T, B, H, math, io="f32", state=False, route="train", sparse=False, shift=0):
    CASES.append((cid, tuple(keys), S, T, B, H, math, io, state, route, sparse, shift))


for _S in (5, 17, 34, 64):                                             # NT = 1 .. 4; 64 = the full last tile
    _n = _nt(_S)
    _case("gcnx%d_f16x3" % _n, ["gcnx_fwd_kernel<%d>|io=32" % _n, "gcnx_bwd_kernel<%d>|io=32|dg16=0" % _n], _S, T_, B_, H_, "f16x3")
    _case("gcnx%d_f16" % _n, ["gcnx_fwd_kernel<%d,f16>|io=32" % _n, "gcnx_bwd_kernel<%d,f16>|io=32|dg16=1" % _n], _S, T_, B_, H_,
          "f16")
    _case("gcn32_%d" % _n, ["gcn32_fwd_kernel<%d>" % _n, "gcn32_bwd_kernel<%d>|w=12" % _n], _S, T_, B_, H_, "f32")
for _S in (5, 34):
    _n = _nt(_S)
    _case("gcnx%d_f16x3g_4098rows" % _n, ["gcnx_fwd_kernel<%d>|io=32" % _n, "gcnx_bwd_kernel<%d>|io=32|dg16=1" % _n], _S, T_, BIG_B,
          H_, "f16x3g")
    for _io in ("f16", "bf16"):
        _case("gcnx%d_%s_io" % (_n, _io), ["gcnx_fwd_kernel<%d>|io=16" % _n, "gcnx_bwd_kernel<%d>|io=16|dg16=0" % _n], _S, T_, B_, H_,
              "f16x3", io=_io)
for _S in (5, 17, 34):
    _n = _nt(_S)
    _case("gcn32_%d_16waves" % _n, ["gcn32_fwd_kernel<%d>" % _n, "gcn32_bwd_kernel<%d>|w=16" % _n], _S, *W16, "f32",
          shift=W16_SHIFT[_S])
    _case("gcngi%d_fused_f16x3" % _n, ["gcngi_fwd_kernel<%d>|io=32|planes=2" % _n], _S, T_, B_, H_, "f16x3", route="fused")
    _case("gcngi%d_fused_f16" % _n, ["gcngi_fwd_kernel<%d,f16>|io=32|planes=1" % _n], _S, T_, B_, H_, "f16", route="fused")
    _case("gcngi%d_infer" % _n, ["gcngi_fwd_kernel<%d>|io=32|planes=0" % _n], _S, T_, B_, H_, "f16x3", route="infer")
_case("state_f32", ["gcn32_fwd_kernel<3>", "gcn32_bwd_kernel<3>|w=12"], 34, T_, B_, H_, "f32", state=True)
_case("state_f16x3", ["gcnx_fwd_kernel<3>|io=32", "gcnx_bwd_kernel<3>|io=32|dg16=0"], 34, T_, B_, H_, "f16x3", state=True)
CSR_KERNELS = ["csr_layer_fwd_kernel", "csr_layer_bwd_kernel<1>", "csr_layer_bwd_kernel<2>"]
# shift: gru.weight_ih_l0 times 2^shift, so that the gate pre-activations of S * 13 inputs stay of order one
CSR_SHAPES = [(34, 3, 5, 9, 0), (200, 3, 4, 12, -2), (2500, 2, 2, 6, -4)]
for _S, _T, _B, _H, _shift in CSR_SHAPES:
    for _math in ("f32", "f16x3") + (("f16",) if _S == 200 else ()):
        _case("csr%d_%s" % (_S, _math), CSR_KERNELS, _S, _T, _B, _H, _math, sparse=True, shift=_shift)

# General GraphConvLayer widths: (id, S, Fi, Fo, nt); the last is the narrow-to-wide pair
LAYER_CASES = [("l_6_9", 7, 6, 9, 5), ("l_13_40", 34, 13, 40, 5), ("l_64_64", 3, 64, 64, 5), ("l_3_64", 17, 3, 64, 5)]
LAYER_KERNELS = ["gcn_any_fwd_kernel", "gcn_any_bwd_kernel", "gcn_any_reduce_kernel"]

# gru_step_kernel: wgnn_fwd_state at T = 1 (dense A, fp32 I/O) with a signed h0: (S, B), H = 9
STEP_CASES = [(S, B) for S in (5, 34, 64) for B in (1, 17)]

# Series: tests/instance_cases.py's shape A (rows 36, T 3, stride 2, n 17), H = 16: (S, H, rows, T, stride, n, seed, route)
SERIES_CASES = [(S, 16, 36, 3, 2, 17, 0, route) for S in (5, 34) for route in ("series", "series_mse", "series_last")]


def window_shapes():
    """The distinct (S, T, B, H, sparse, shift) of CASES and STEP_CASES with, per shape, the maths and I/O types run on it."""
    out = {}
    for cid, keys, S, T, B, H, math, io, state, route, sparse, shift in CASES:
        out.setdefault((S, T, B, H, sparse, shift), set()).add((math, io))
    for S, B in STEP_CASES:
        out.setdefault((S, 1, B, H_, False, 0), set()).add(("f32", "f32"))
    return out
