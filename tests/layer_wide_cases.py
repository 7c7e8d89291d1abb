"""GraphConvLayer wider than 64 features (csrc/gcn_wide.hip): the shapes, the launch geometry restated, the draws and their fp64
references.  A plain module: nothing here is collected.  tests/test_layer_wide_host.py qualifies all of it on the CPU,
tests/test_gpu_layer_wide.py runs it on the GPU."""
import functools

import torch

import lattice_inputs as li

# (S, Fi, Fo, tiles): what each reaches is in tests/test_layer_wide_host.py's loop table
TABLE = [
    (34, 13, 128, 5),        # the model's layer 1 at hidden_dim = 128
    (34, 128, 13, 5),        # its layer 2
    (64, 64, 65, 3),         # first width past gcn_any.hip, S at its bound
    (7, 65, 65, 3),          # K and N one past a multiple of 4 / 16
    (64, 200, 72, 3),        # several K chunks and column blocks, both ragged
    (5, 257, 129, 9),        # the same, odd everywhere, S below one MFMA row tile
    (3, 512, 1, 4),          # wide -> 1
    (17, 1, 300, 3),         # 1 -> wide
    (34, 96, 80, 2100),      # 2100 = 2 x 1024 + 52 tiles: a third trip of the busiest workgroups, ragged
    (34, 65, 2, 40),         # 40 partial rows of db and 21 of dW: the summing threads' third / second trip, ragged
    (5, 70, 13, 2100),       # the thin forward (F_out <= 32) in a third trip over its tiles, three K chunks, both ragged
]
IDS = ["S%d-%dto%d-x%d" % r for r in TABLE]
FOOTPRINT_ROWS = [TABLE[0], TABLE[5], TABLE[6]]
# GCN_GRU(13, hid, 13, S * 13, H): (S, hid, T, B, H)
MODEL_SHAPES = [(34, 128, 3, 2, 102), (7, 200, 4, 3, 21), (64, 65, 2, 2, 9), (5, 70, 5, 3, 7)]
MODEL_IDS = ["S%d-hid%d-T%d-B%d-H%d" % m for m in MODEL_SHAPES]
WIH_SHIFT = -6               # gru.weight_ih_l0 times 2^-6: the wide g would otherwise saturate every gate (max |Y| = 1)
FWD_KERNELS = {False: "gcn_wide_fwd_kernel", True: "gcn_wide_fwd_thin_kernel"}     # by F_out <= TB


def wide_kernels(Fo):
    """The library's own kernels of one forward + backward (gemm.hip's carry the products against W in the backward)."""
    return [FWD_KERNELS[Fo <= TB], "gcn_wide_bwd_agg_kernel", "gcn_wide_sum_kernel"]


# ---- gcn_wide.hip's geometry, restated (tests/test_layer_wide_host.py holds it against the source text) ------------------------
THREADS, ROWS, KC, NB, CB, MAXGRID, SUM_ROWS, TB = 256, 64, 32, 128, 64, 1024, 16, 32
GEMM_BK = 16                 # gemm.hip: a split-K chunk is a multiple of its K step


def cdiv(a, b):
    return (a + b - 1) // b


def grid(nt):
    return min(nt, MAXGRID)


def gemm_f32_tiles(M, N):
    """gemm.hip's gemm_f32_tile / gemm_f32_tiles."""
    if cdiv(M, 128) * cdiv(N, 128) >= 1024:
        return cdiv(M, 128) * cdiv(N, 128)
    bn = 64 if cdiv(N, 64) * 64 < cdiv(N, 128) * 128 else 128
    bm = 64 if (cdiv(M, 64) * 64 < cdiv(M, 128) * 128 or cdiv(M, 128) * cdiv(N, bn) < 512) else 128
    return cdiv(M, bm) * cdiv(N, bn)


def splitk(nt, S, Fi, Fo):
    rows = nt * S
    return max(1, min(cdiv(1024, gemm_f32_tiles(Fi, Fo)), rows // 64))


def workspace_floats(nt, S, Fi, Fo):
    up = lambda n: cdiv(n, 64) * 64                                                          # noqa: E731
    return up(nt * S * Fo) + up(grid(nt) * Fo) + up(splitk(nt, S, Fi, Fo) * Fi * Fo)


def loops(S, Fi, Fo, nt):
    """{loop: (trips, ragged last trip)} of one forward + backward.  Grid dimensions that walk a tensor count as loops."""
    sk = splitk(nt, S, Fi, Fo)
    kchunk = cdiv(cdiv(nt * S, sk), GEMM_BK) * GEMM_BK
    thin = Fo <= TB
    none = (0, False)
    return {
        "tiles per workgroup": (cdiv(nt, grid(nt)), nt % grid(nt) != 0),
        "tiles per workgroup of the thin forward": (cdiv(nt, grid(nt)), nt % grid(nt) != 0) if thin else none,
        "tiles per workgroup of the general forward": none if thin else (cdiv(nt, grid(nt)), nt % grid(nt) != 0),
        "K chunks of the thin forward": (cdiv(Fi, KC), Fi % KC != 0) if thin else none,
        "K chunks of the general forward": none if thin else (cdiv(Fi, KC), Fi % KC != 0),
        "station steps of 4": (cdiv(S, 4), S % 4 != 0),
        "row tiles of 16": (cdiv(S, 16), S % 16 != 0),
        "K chunks of X": (cdiv(Fi, KC), Fi % KC != 0),
        "forward column blocks": (cdiv(Fo, NB), Fo % NB != 0),
        "backward column blocks": (cdiv(Fo, CB), Fo % CB != 0),
        "split-K chunks of dW": (cdiv(nt * S, kchunk), (nt * S) % kchunk != 0),
        "partial rows of dW per summing thread": (cdiv(sk, SUM_ROWS), sk % SUM_ROWS != 0),
        "partial rows of db per summing thread": (cdiv(grid(nt), SUM_ROWS), grid(nt) % SUM_ROWS != 0),
    }


# ---- draws and fp64 references (computed once, shared, never written to) ------------------------------------------------------
@functools.lru_cache(maxsize=None)
def layer_reference(S, Fi, Fo, nt):
    """The lattice draw of a row and fp64 autograd of relu(A X W + b) on it: (draw, out, dX, dW, db)."""
    d = li.draw_layer(S, Fi, Fo, nt)
    leaves = [t.double().clone().requires_grad_(True) for t in (d.X, d.W, d.b)]
    ref = torch.relu(torch.matmul(torch.matmul(d.A.double(), leaves[0]), leaves[1]) + leaves[2])
    ref.backward(d.dout.double())
    return d, ref.detach(), leaves[0].grad, leaves[1].grad, leaves[2].grad


@functools.lru_cache(maxsize=None)
def model_draw(S, hid, T, B, H):
    """A, X [B, T, S, 13], labels and the 8 parameters of GCN_GRU(13, hid, 13, S * 13, H): conv tensors on the lattice, the GRU
    tensors of oracle.init_params(S, 13, H, seed=3), gru.weight_ih_l0 times 2^WIH_SHIFT."""
    from oracle import windgnn_oracle as orc
    d = li.Draw()
    g = torch.Generator().manual_seed(7300 + 31 * S + 7 * hid + T + B + 101 * H)
    d.A = li.lattice_adjacency(S, g)
    d.X = li.lattice_features(g, (B, T, S, li.F))
    d.p = {k: v.float() for k, v in orc.init_params(S, li.F, H, seed=3).items()}
    d.p["conv1.weight"], d.p["conv1.bias"] = li.lattice_conv(g, li.F, hid, layer=1)
    d.p["conv2.weight"], d.p["conv2.bias"] = li.lattice_conv(g, hid, li.F, layer=2)
    d.p["gru.weight_ih_l0"] = d.p["gru.weight_ih_l0"] * 2.0 ** WIH_SHIFT
    d.L = torch.rand(B, T, H, generator=g)
    return d


@functools.lru_cache(maxsize=None)
def model_reference(S, hid, T, B, H):
    """(draw, Y, loss, gradients) of the fp64 oracle's forward / mse_loss_and_grad / backward."""
    from oracle import windgnn_oracle as orc
    d = model_draw(S, hid, T, B, H)
    A, X, L = d.A.double(), d.X.double(), d.L.double()
    p = {k: v.double() for k, v in d.p.items()}
    Y, cache = orc.forward(A, X, p)
    loss, dY = orc.mse_loss_and_grad(Y, L)
    return d, Y, float(loss), orc.backward(A, X, p, Y, cache, dY)
