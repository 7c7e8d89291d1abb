"""Case table of tests/test_large_offset_host.py and tests/test_gpu_large_offset.py: the largest batches the entry points accept,
where an operand of a kernel launch lies past 2^31 or 2^32 BYTES although every element count stays below 2^31.

The method is a periodic batch.  P = 48 base windows are drawn once per case (tests/lattice_inputs.py's signed, tie-free draws:
live ReLU masks) and the big batch is X[b] = X_P[b mod P], built on the device.  The fp64 oracle then runs on 48 windows and on
the first r = B mod 48 of them; Y_ref[b] = Yo[b mod P], and the loss and every gradient of the mean loss over B windows are
(R P v_P + r v_r) / B of the two mean-normalised results (B = 48 R + r).  48 = 3 x 16 windows: three workgroups of the
recurrences, and its factor 3 puts a read or write that wrapped by 2^31 or 2^32 bytes on another phase (window in period, step)
even where a row pitch is a power of two -- tests/test_large_offset_host.py proves that per case and operand, and that two phases
differ by far more than the bar.  Every B is 48 R + r with r in {5, 21, 37}: a ragged last period and a partial last workgroup.

Y itself never reaches 2^31 bytes: check_dims keeps B*T*4H below 2^31 elements, so Y is below 2^31 bytes of fp32.
16-bit X never reaches 2^32 bytes: B*T*S*13 < 2^31 elements of 2 bytes.

Series mode has an hour series of period Q = 45 (odd: coprime to every power-of-two wrap) and the oracle runs on the at most 45
distinct windows, gradients combined by phase counts; the one-layer entry points run on tiles of period 48 against fp64 autograd;
the element-wise entries have closed-form fp64 references built from a period of 48 values.

Nothing here touches a GPU; the shapes were sized with the library's own wgnn_*_bytes functions."""
import functools

import torch

P = 48
RAGGED = (5, 21, 37)
T31, T32 = 2 ** 31, 2 ** 32
F = 13
MATH = {"f32": 0, "f16x3": 1, "f16": 2, "f16x3g": 3}
IO = {"f32": 0, "f16": 1, "bf16": 2}
IO_DTYPE = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
IO_BYTES = {"f32": 4, "f16": 2, "bf16": 2}


def rup(x, a):
    return (x + a - 1) // a * a


class Step:
    """One dense-step case.  runs: (math, io, route) with route 'raw' (wgnn_fwd_loss, wgnn_bwd_mse_part(7 | 8 | DEFER),
    wgnn_finish(6)), 'raw_ghn3' (the same with WGNN_GHN_RECOMPUTE=0: three-component gate records), 'state' (wgnn_fwd_state_stash
    + wgnn_bwd_state_part with h0, dh_n and dh0) or 'trainstep' (TrainStep.step + check()).
    crosses: (operand, threshold, io or None = every I/O type of the case) -- the operands this case exists for; the host test
    recomputes each from the header formulas and refuses a case whose claim does not hold."""

    def __init__(self, cid, S, T, H, B, runs, crosses, csr_k=0, shift=0, note=""):
        self.id, self.S, self.T, self.H, self.B = cid, S, T, H, B
        self.runs, self.crosses, self.csr_k, self.shift, self.note = runs, crosses, csr_k, shift, note
        self.R, self.r = divmod(B, P)

    @property
    def nnz(self):
        return csr_of(self.id).nnz if self.csr_k else 0

    @property
    def rows(self):
        return self.B * self.T

    def dims(self, math, io="f32", B=None):
        from windgnn_amd import _lib
        return _lib.Dims(self.B if B is None else B, self.T, self.S, F, self.H, MATH[math], 1 if self.csr_k else 0, self.nnz,
                         IO[io])

    # ---- row pitches in bytes (csrc/api.hip make_layout; include/windgnn.h "Sizes"): every operand below is [B*T] rows
    def pitch(self, operand, io="f32"):
        I = self.S * F
        return {"X": I * IO_BYTES[io],                 # [B, T, S, 13] in the I/O type
                "g": rup(I + 1, 32) * 4,               # fp32 g, or its hi + lo fp16 planes taken together
                "g_plane": rup(I + 1, 32) * 2,         # ONE fp16 plane of g
                "dg": rup(I, 16) * 4,
                "GI": rup(3 * self.H, 32) * 4,         # GI and dGI: fp32 rows, or hi + lo planes taken together
                "h1": I * 4, "du": I * 4}[operand]     # CSR front end: layer-1 activations and their gradient

    def bytes(self, operand, io="f32"):
        return self.rows * self.pitch(operand, io)


_RAW4 = [("f32", "f32", "raw"), ("f16x3", "f32", "raw"), ("f16x3g", "f32", "raw"), ("f16", "f32", "raw")]

STEPS = [
    Step("x4g", 64, 3, 31, 432021,
         _RAW4 + [("f16x3", "bf16", "raw"), ("f16", "f16", "raw")],
         [("X", T32, "f32"), ("g", T32, None), ("X", T31, "f16"), ("X", T31, "bf16"), ("g_plane", T31, None)],
         note="16-bit X cannot reach 2^32 bytes below the element limit: it crosses 2^31"),
    Step("gi4g", 3, 2, 127, 1400021,
         _RAW4 + [("f16x3", "f32", "raw_ghn3"), ("f32", "f32", "state"), ("f16x3", "f32", "state")],
         [("GI", T32, None)]),
    Step("bench60k", 34, 24, 102, 60021,
         [("f32", "f32", "trainstep"), ("f16x3", "f32", "trainstep"), ("f16x3g", "f32", "trainstep")],
         [("X", T31, "f32"), ("g", T31, None)],
         note="the advertised workload at 15 times the batch (GI, 1.84e9 B, stays below 2^31 at this B)"),
    Step("wide", 3, 2, 200, 1300021, [("f32", "f32", "raw"), ("f16x3", "f32", "raw")],
         [("GI", T32, None)], note="B*T*4H = 2.08e9, just under the limit"),
    Step("csr", 4096, 2, 4, 20021, [("f32", "f32", "raw"), ("f16x3", "f32", "raw")],
         [("X", T32, "f32"), ("h1", T32, None), ("du", T32, None), ("dg", T32, None)], csr_k=8,
         note="2.132e9 elements in only 40 042 rows; the symmetric 8-NN graph of graph.build_knn_adjacency, uniform draws"),
]
STEP_BY_ID = {c.id: c for c in STEPS}
STEP_RUNS = [(c.id, m, io, route) for c in STEPS for m, io, route in c.runs]


def run_id(run):
    cid, math, io, route = run
    return "%s-%s%s%s" % (cid, math, "" if io == "f32" else "-" + io, "" if route in ("raw", "trainstep") else "-" + route)


# ---- element-wise entries: n elements of fp32, closed-form fp64 references from a period of 48 values
ELEMENTWISE = {
    "mse_loss_grad": dict(n=2 ** 31 + 4097, crosses=[("Y", T32), ("L", T32), ("dY", T32)]),
    "adam_step": dict(n=2 ** 31 + 169, crosses=[("param", T32), ("grad", T32), ("exp_avg", T32), ("exp_avg_sq", T32)]),
}
# wgnn_predict_last / wgnn_eval_accum read row T - 1 of every window of Y / labels [B, T, H]; neither header limits that tensor
# (wgnn_predict_last: out [B, H] below 2^31 elements), so it is taken past 2^32 bytes.  wgnn_make_windows: X [B, seq, S, 13] of x4g
PREDICT_LAST = dict(B=1400021, T=7, H=127)          # Y / labels: 1 244 618 669 elements = 4.98e9 B
# ... and out [B, H] at 2^31 - 8 elements, inside the last 255 below the limit, where a 32-bit block count would have wrapped
PREDICT_LAST_EDGE = dict(B=16909320, T=1, H=127)
MAKE_WINDOWS = dict(B=432021, seq=3, S=64, Ttot=432021 * 3 + 3)   # X of x4g: 4.31e9 B


# ---- GraphConvLayer: ntiles tiles of period 48; fp64 torch autograd on the period
class Layer:
    """(ntiles, S, Fi -> Fo) of wgnn_gcn_layer_* (dense A) or wgnn_gcn_layer_csr_* (csr_k-NN graph): forward and backward, with
    and without dX.  Operands are [ntiles] tiles of S * F floats."""

    def __init__(self, cid, nt, S, Fi, Fo, kernels, crosses, csr_k=0):
        self.id, self.nt, self.S, self.Fi, self.Fo, self.kernels, self.crosses, self.csr_k = cid, nt, S, Fi, Fo, kernels, crosses, csr_k
        self.R, self.r = divmod(nt, P)
        self.T = 1                                   # a tile is one row of its operands

    @property
    def rows(self):
        return self.nt

    def pitch(self, operand, io="f32"):
        return {"X": self.S * self.Fi * 4, "dX": self.S * self.Fi * 4, "out": self.S * self.Fo * 4, "dout": self.S * self.Fo * 4}[operand]

    def bytes(self, operand, io="f32"):
        return self.nt * self.pitch(operand)


LAYERS = [
    Layer("l_13_200", 1800021, 3, 13, 200, "gcn_wide.hip, thin forward", [("out", T32), ("dout", T32)]),
    Layer("l_200_13", 2500021, 3, 200, 13, "gcn_wide.hip", [("X", T32), ("dX", T32)]),
    Layer("l_64_64", 11000021, 3, 64, 64, "gcn_any.hip", [("X", T32), ("out", T32), ("dout", T32), ("dX", T32)]),
    Layer("l_13_13", 40000021, 3, 13, 13, "gcn.hip", [("X", T32), ("out", T32), ("dout", T32), ("dX", T32)]),
    Layer("l_csr", 40021, 4096, 13, 13, "general.hip, CSR", [("X", T32), ("out", T32), ("dout", T32), ("dX", T32)], csr_k=8),
]
LAYER_BY_ID = {c.id: c for c in LAYERS}


@functools.lru_cache(maxsize=None)
def layer_draw(cid):
    import lattice_inputs as li
    c = LAYER_BY_ID[cid]
    if not c.csr_k:
        return li.draw_layer(c.S, c.Fi, c.Fo, P, seed=31)
    from windgnn_amd.graph import CsrAdjacency
    d = li.Draw()                                    # tests/test_gpu_parity.py::test_graph_conv_layer_with_csr_adjacency's draws
    g = torch.Generator().manual_seed(4096 + 13)
    d.A = CsrAdjacency(*_knn_graph(c.S, c.csr_k)).dense()
    d.X = torch.rand(P, c.S, c.Fi, generator=g)
    d.W = torch.randn(c.Fi, c.Fo, generator=g)
    d.b = torch.rand(c.Fo, generator=g) - 0.5
    d.dout = torch.rand(P, c.S, c.Fo, generator=g)
    return d


def layer_csr(cid):
    from windgnn_amd.graph import CsrAdjacency
    c = LAYER_BY_ID[cid]
    return CsrAdjacency(*_knn_graph(c.S, c.csr_k))


@functools.lru_cache(maxsize=None)
def layer_reference(cid):
    """fp64 autograd of relu(A X W + b) on the 48 tiles: out and dX per tile, dW and db of all ntiles tiles (sums: R times the
    period's plus those of its first r tiles)."""
    c, d = LAYER_BY_ID[cid], layer_draw(cid)
    res = []
    for n in (P, c.r):
        X, W, b = (t.double().clone().requires_grad_(True) for t in (d.X[:n], d.W, d.b))
        out = torch.relu(torch.matmul(torch.matmul(d.A.double(), X), W) + b)
        out.backward(d.dout[:n].double())
        res.append((out.detach(), X.grad, W.grad, b.grad))
    (out, dX, dWP, dbP), (_, _, dWr, dbr) = res
    return dict(out=out, dX=dX, dW=c.R * dWP + dWr, db=c.R * dbP + dbr)


# ---- series mode (exact fp32): the hour series has period Q = 45, coprime to 2 and so to every power-of-two wrap
Q = 45


class Series:
    """rows hours of period 45, windows of T hours at a stride (n of them) or at a table of starts.  Window w of the strided
    calls starts at phase (w * stride) mod 45: the windows have period 45 / gcd(stride, 45) in w.  Operands are [rows] rows."""

    def __init__(self, cid, rows, S, T, H, stride, n, crosses, n_table=0):
        self.id, self._rows, self.S, self.T, self.H, self.stride, self.n, self.crosses, self.n_table = cid, rows, S, T, H, stride, n, crosses, n_table
        import math
        self.period = Q // math.gcd(stride, Q)

    rows = property(lambda self: self._rows)

    def pitch(self, operand, io="f32"):
        I = self.S * F
        return {"Xs": I * 4, "g_s": rup(I + 1, 32) * 4, "GI_s": rup(3 * self.H, 32) * 4}[operand]

    def bytes(self, operand, io="f32"):
        return self._rows * self.pitch(operand)

    def sdims(self, table=False):
        from windgnn_amd import _lib
        return _lib.SeriesDims(self._rows, self.T, 0 if table else self.stride, self.n_table if table else self.n, self.S, F, self.H,
                               0, 0, 0, 0)

    def crossing_rows(self):
        """The rows either side of the 2^31-byte and 2^32-byte crossings of GI_s."""
        q = self.pitch("GI_s")
        return [r for th in (T31, T32) for r in (th // q - 1, th // q, th // q + 1) if r + self.T <= self._rows]

    def table(self):
        """The sorted table of starts of the _at calls: row 0, the crossings, rows - T, and n_table - 8 more spread over the
        series by a fixed generator."""
        g = torch.Generator().manual_seed(4500 + self._rows % 1000)
        fixed = [0, self._rows - self.T] + self.crossing_rows()
        more = torch.randint(0, self._rows - self.T + 1, (self.n_table - len(fixed),), generator=g)
        return torch.sort(torch.cat([torch.tensor(fixed), more]))[0].to(torch.int32)


SERIES = [
    Series("series_gi", 4000000, 3, 2, 127, 4, 1000000, [("GI_s", T32)], n_table=100021),
    Series("series_x", 1296063, 64, 3, 31, 3, 432021, [("Xs", T32), ("g_s", T32)]),
]
SERIES_BY_ID = {c.id: c for c in SERIES}


@functools.lru_cache(maxsize=None)
def series_draw(cid):
    """A, the 45 hours Xs_Q [45, S, 13] and Ls_Q [45, H], a signed dY_Q [45, T, H] (one per start phase) and the parameters."""
    import lattice_inputs as li
    c = SERIES_BY_ID[cid]
    return li.draw_series(c.S, c.H, Q, c.T, 1, Q, seed=31)


def phase_counts(phases):
    """How many windows start at each of the 45 phases."""
    return torch.bincount(torch.as_tensor(phases, dtype=torch.int64) % Q, minlength=Q).double()


@functools.lru_cache(maxsize=None)
def series_windows(cid):
    """fp64 oracle on the 45 windows, one per start phase f: hours f .. f + T - 1 (mod 45).  Y [45, T, H], the cache (g and GI of
    hour f are row 0 of window f), and the windows' X and labels."""
    from oracle import windgnn_oracle as orc
    c, d = SERIES_BY_ID[cid], series_draw(cid)
    idx = (torch.arange(Q)[:, None] + torch.arange(c.T)[None, :]) % Q
    X, L = d.Xs[idx].double(), d.Ls[idx].double()
    p = {k: v.double() for k, v in d.p.items()}
    Y, cache = orc.forward(d.A.double(), X, p)
    return dict(X=X, L=L, Y=Y, cache=cache, p=p, A=d.A.double())


def series_grads(cid, phases, mse):
    """The loss and the 8 gradients of a call whose windows start at `phases` (any number of them): mse = False, the gradients of
    sum(Y dY) with dY[w] = dY_Q[phase of w]; mse = True, of mean((Y - labels)^2) over all windows.  One oracle backward on the
    45 windows with each window's dY weighted by the number of windows at its phase."""
    from oracle import windgnn_oracle as orc
    c, d, w = SERIES_BY_ID[cid], series_draw(cid), series_windows(cid)
    cnt = phase_counts(phases)
    n = float(cnt.sum())
    if mse:
        diff = w["Y"] - w["L"]
        loss = float((cnt[:, None, None] * diff * diff).sum() / (n * c.T * c.H))
        dY = cnt[:, None, None] * 2.0 * diff / (n * c.T * c.H)
    else:
        loss, dY = None, cnt[:, None, None] * d.dY.double()
    return loss, orc.backward(w["A"], w["X"], w["p"], w["Y"], w["cache"], dY)


# ---- the draws and the fp64 references (host, cached: one per case and I/O type for the whole session)
@functools.lru_cache(maxsize=None)
def base_draw(cid):
    """A (dense fp32), X_P [48, T, S, 13], L_P [48, T, H], the 8 parameters, and the signed h0_P / dY_P / dhn_P of the state
    route.  Never written to."""
    import lattice_inputs as li
    c = STEP_BY_ID[cid]
    if not c.csr_k:
        return li.draw(c.S, c.T, P, c.H, shift=c.shift, seed=31)
    # the CSR front end runs no dense GCN kernel: the suite's usual generators (tests/test_gpu_parity.py's 4096-station case)
    from oracle import windgnn_oracle as orc
    d = li.Draw()
    g = torch.Generator().manual_seed(4096 + c.H)
    d.A = csr_of(cid).dense()
    d.X = torch.rand(P, c.T, c.S, F, generator=g)
    d.L = torch.rand(P, c.T, c.H, generator=g)
    d.p = orc.init_params(c.S, F, c.H, seed=9)
    d.p["gru.weight_ih_l0"] = d.p["gru.weight_ih_l0"] * (c.H / 12288.0) ** 0.5      # the projection's scale at H = 12 288
    return d


@functools.lru_cache(maxsize=None)
def _knn_graph(S, k):
    from windgnn_amd.graph import build_knn_adjacency, synthetic_station_coords
    return build_knn_adjacency(synthetic_station_coords(S, seed=7), k)


def _knn(cid):
    c = STEP_BY_ID[cid]
    return _knn_graph(c.S, c.csr_k)


def csr_of(cid):
    """A fresh CsrAdjacency of the case's graph (its .to(device) moves the buffer: one per use)."""
    from windgnn_amd.graph import CsrAdjacency
    return CsrAdjacency(*_knn(cid))


def combine(c, vP, vr):
    """The mean over B = 48 R + r windows from the means over the period and over its first r windows."""
    return (c.R * P * vP + c.r * vr) / c.B


@functools.lru_cache(maxsize=None)
def step_reference(cid, io="f32"):
    """fp64 oracle on the 48 windows and on the first r (the inputs rounded to the I/O type first): Yo [48, T, H], the cache
    of the period (g, GI: the operands' own rows), and loss / gradients of the big batch."""
    from oracle import windgnn_oracle as orc
    c, d = STEP_BY_ID[cid], base_draw(cid)
    dt = IO_DTYPE[io]
    A = d.A.double()
    X, L = d.X.to(dt).double(), d.L.to(dt).double()
    p = {k: v.double() for k, v in d.p.items()}
    Yo, cache = orc.forward(A, X, p)
    lossP, dY = orc.mse_loss_and_grad(Yo, L)
    gP = orc.backward(A, X, p, Yo, cache, dY)
    Yr, lossr, gr = orc.train_step(A, X[:c.r], L[:c.r], p)
    assert float((Yr - Yo[:c.r]).abs().max()) <= 1e-12            # (BLAS blocks a batch of r and of 48 differently)
    return dict(Y=Yo, g=cache["g"], GI=cache["GI"], H1=cache["H1"], loss=float(combine(c, lossP, lossr)),
                grads={k: combine(c, gP[k], gr[k]) for k in orc.PARAM_KEYS})


# ---- the comparisons (any device): shared by the GPU module and by the planted wraps of the host module
CHUNK_BYTES = 256 << 20        # fp64 bytes of one comparison chunk: the comparison's own device memory, whatever the row size


def check_periodic(Y, Yo, tol, what, chunk_periods=None, P=P):
    """Checks 1-3 of a [B, ...] result whose rows are those of the period Yo [48, ...] (fp64), over EVERY row, chunk by chunk on
    Y's device: no NaN left from the prefill; Y[48:] == Y[:-48] bit for bit (windows are independent and a row's arithmetic
    does not depend on its position: an addressing error shows here without any tolerance); max |Y - Yo[b mod 48]| <= tol.
    A chunk is as many whole periods as make CHUNK_BYTES of fp64 (at least one), and the difference is formed in place: the
    comparison holds one fp64 chunk (and a bool chunk of an eighth of it) at a time.
    Returns the worst error.  The messages name the check, the first offending window and its phase."""
    B = Y.shape[0]
    R, r = divmod(B, P)
    assert tuple(Y.shape[1:]) == tuple(Yo.shape[1:]) and Yo.shape[0] == P and R >= 2
    inner = tuple(range(1, Y.dim()))
    if chunk_periods is None:
        chunk_periods = max(1, CHUNK_BYTES // (P * max(1, Yo[0].numel()) * 8))
    step = chunk_periods * P
    for b0 in range(0, B, step):
        bad = torch.isnan(Y[b0:b0 + step]).any(dim=inner) if inner else torch.isnan(Y[b0:b0 + step])
        if bool(bad.any()):
            b = b0 + int(bad.nonzero()[0])
            raise AssertionError("%s: check 1 (NaN prefill): window %d of %d (phase %d) still holds a NaN: it was never written "
                                 "or was computed from unwritten scratch" % (what, b, B, b % P))
        del bad
    for b0 in range(P, B, step):
        a, b_ = Y[b0:b0 + step], Y[b0 - P:min(b0 + step, B) - P]
        ne = (a != b_).any(dim=inner) if inner else (a != b_)
        if bool(ne.any()):
            b = b0 + int(ne.nonzero()[0])
            raise AssertionError("%s: check 3 (period): window %d of %d (phase %d) differs from window %d bit for bit: an "
                                 "addressing error, no tolerance involved" % (what, b, B, b % P, b - P))
        del ne
    ref = Yo.to(Y.device)
    worst = 0.0
    for p0 in range(0, R, chunk_periods):
        blk = Y[p0 * P:min(p0 + chunk_periods, R) * P].double().reshape((-1, P) + tuple(Y.shape[1:]))
        worst = max(worst, float(blk.sub_(ref).abs_().max()))
        del blk
    if r:
        worst = max(worst, float(Y[R * P:].double().sub_(ref[:r]).abs_().max()))
    assert worst <= tol, "%s: check 2: max|Y - Y_ref| = %.3e over all %d windows exceeds %.1e" % (what, worst, B, tol)
    return worst


def periodic(tP, B, P=None):
    """t[b] = tP[b mod 48] for b < B, built where tP lives (on the device: never on the host at full size)."""
    P = tP.shape[0] if P is None else P
    assert tP.shape[0] == P
    reps = (B + P - 1) // P
    return tP.repeat((reps,) + (1,) * (tP.dim() - 1))[:B]
