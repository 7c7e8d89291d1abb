"""GraphConvLayer wider than 64 features, checked without a GPU: the dispatch of wgnn_gcn_layer_workspace_bytes / _fwd / _bwd on
fake device pointers (every call is refused on the host, before any launch), the lattice qualification of
tests/layer_wide_cases.py's table and model shapes on the fp64 reference, the launch geometry restated against the text of
csrc/gcn_wide.hip with the trips every loop makes per table row, and three planted mistakes that a loop's last trip could make.
A failure of tests/test_gpu_layer_wide.py on these inputs is therefore a finding about the kernels."""
import ctypes as C
import os
import re

import pytest
import torch

import lattice_inputs as li
import layer_wide_cases as lw
from conftest import PARAM_KEYS, ROOT, max_abs, rel_to_max
from test_gpu_parity import G_TOL, Y_TOL

OK, ERR_NULL, ERR_SHAPE, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, -1, -2, -4, -5
BAR = 1e-4
assert BAR == G_TOL == Y_TOL
STEPS = (1 / 32, 1 / 512)                           # Z1 is an odd multiple of 1/32, Z2 (layer-2 grid) of 1/512


def _lib():
    from windgnn_amd import _lib as L
    from windgnn_amd import build
    build.build(verbose=False)
    return L.load()


FWD_ARGS = ("A", "X", "W", "b", "out")
BWD_ARGS = ("A", "X", "W", "out", "dout", "dW", "db", "dX", "workspace")


def _fwd(lib, nt, S, Fi, Fo, null=None):
    p = [C.c_void_p(0 if n == null else (i + 1) << 32) for i, n in enumerate(FWD_ARGS)]
    return lib.wgnn_gcn_layer_fwd(nt, S, Fi, Fo, *p, None)


def _bwd(lib, nt, S, Fi, Fo, ws_bytes, null=None):
    p = [C.c_void_p(0 if n == null else (i + 1) << 32) for i, n in enumerate(BWD_ARGS)]
    return lib.wgnn_gcn_layer_bwd(nt, S, Fi, Fo, *p, C.c_size_t(ws_bytes), None)


# ==== 1. the dispatch ==============================================================================================================
@pytest.mark.parametrize("row", lw.TABLE, ids=lw.IDS)
def test_the_wide_domain_is_accepted_and_refused_in_the_documented_order(row):
    lib = _lib()
    S, Fi, Fo, nt = row
    wsb = lib.wgnn_gcn_layer_workspace_bytes(nt, S, Fi, Fo)
    assert wsb > 0 and wsb % 256 == 0 and wsb == 4 * lw.workspace_floats(nt, S, Fi, Fo)
    for n in FWD_ARGS:
        assert _fwd(lib, nt, S, Fi, Fo, null=n) == ERR_NULL, n
    for n in BWD_ARGS:
        if n != "dX":                                                   # dX == NULL is a request, not an error
            assert _bwd(lib, nt, S, Fi, Fo, wsb, null=n) == ERR_NULL, n
    assert _bwd(lib, nt, S, Fi, Fo, wsb - 1) == ERR_WORKSPACE and _bwd(lib, nt, S, Fi, Fo, wsb - 1, null="dX") == ERR_WORKSPACE
    # S > 64 stays unsupported; a shape error comes first, a NULL after
    assert lib.wgnn_gcn_layer_workspace_bytes(nt, 65, Fi, Fo) == 0
    assert _fwd(lib, nt, 65, Fi, Fo) == ERR_UNSUPPORTED and _bwd(lib, nt, 65, Fi, Fo, 1 << 40) == ERR_UNSUPPORTED
    assert _fwd(lib, nt, 65, Fi, Fo, null="X") == ERR_UNSUPPORTED and _fwd(lib, 0, 65, Fi, Fo, null="X") == ERR_SHAPE
    for bad in ((0, S, Fi, Fo), (nt, 0, Fi, Fo), (nt, S, 0, Fo), (nt, S, Fi, 0)):
        assert lib.wgnn_gcn_layer_workspace_bytes(*bad) == 0 and _fwd(lib, *bad) == ERR_SHAPE and _bwd(lib, *bad, 1 << 40) == ERR_SHAPE


def test_an_element_count_of_two_to_the_31_is_a_shape_error():
    lib = _lib()
    for S, Fi, Fo in ((64, 128, 13), (64, 13, 128), (1, 128, 1), (32, 512, 512)):
        nt = (1 << 31) // (S * max(Fi, Fo))
        assert nt * S * max(Fi, Fo) == 1 << 31
        assert lib.wgnn_gcn_layer_workspace_bytes(nt, S, Fi, Fo) == 0
        assert _fwd(lib, nt, S, Fi, Fo) == ERR_SHAPE and _bwd(lib, nt, S, Fi, Fo, 1 << 62) == ERR_SHAPE
        assert _fwd(lib, nt, 65, Fi, Fo) == ERR_SHAPE                      # shape before unsupported
        wsb = lib.wgnn_gcn_layer_workspace_bytes(nt - 1, S, Fi, Fo)        # one tile fewer is in the domain
        assert wsb == 4 * lw.workspace_floats(nt - 1, S, Fi, Fo) and _bwd(lib, nt - 1, S, Fi, Fo, wsb - 1) == ERR_WORKSPACE
    # F * F_out
    assert 65536 * 32768 == 1 << 31
    assert lib.wgnn_gcn_layer_workspace_bytes(1, 1, 65536, 32768) == 0 and _fwd(lib, 1, 1, 65536, 32768) == ERR_SHAPE
    assert lib.wgnn_gcn_layer_workspace_bytes(1, 1, 65536, 32767) == 4 * lw.workspace_floats(1, 1, 65536, 32767)


def test_widths_up_to_64_keep_their_workspace_sizes():
    """gcn_any_bwd_partial_floats restated: min(ntiles, 1024) rows of F * F_out + F_out floats (13 -> 13 has gcn.hip's own)."""
    lib = _lib()
    for nt in (1, 5, 1024, 1025, 2100):
        for S in (1, 34, 64):
            for Fi, Fo in ((6, 9), (13, 40), (64, 64), (1, 1), (3, 64), (64, 1), (13, 12)):
                assert lib.wgnn_gcn_layer_workspace_bytes(nt, S, Fi, Fo) == 4 * min(nt, 1024) * (Fi * Fo + Fo), (nt, S, Fi, Fo)
    assert lib.wgnn_gcn_layer_workspace_bytes(5, 34, 13, 13) > 0
    assert lib.wgnn_gcn_layer_workspace_bytes(5, 65, 13, 13) == 0 and _fwd(lib, 5, 65, 64, 64) == ERR_UNSUPPORTED
    # the threshold itself
    assert lib.wgnn_gcn_layer_workspace_bytes(5, 34, 64, 65) == 4 * lw.workspace_floats(5, 34, 64, 65)
    assert lib.wgnn_gcn_layer_workspace_bytes(5, 34, 65, 64) == 4 * lw.workspace_floats(5, 34, 65, 64)


# ==== 2. / 3. the inputs ===========================================================================================================
@pytest.mark.parametrize("row", lw.TABLE, ids=lw.IDS)
def test_table_rows_qualify_on_the_lattice(row):
    d = lw.layer_reference(*row)[0]
    (Z,), _ = li.preacts(d.A, d.X, d.W, d.b)
    (r,) = li.measure([Z], STEPS[:1])
    print("S%d %d -> %d x%d: %s" % (row + (r,)))
    assert r["odd"] and r["qmax"] < 2 ** 24 and 0.3 <= r["live"] <= 0.7, r
    assert not torch.equal(d.A, d.A.t())
    # fp32 torch in both association orders is the fp64 Z exactly
    Zf = torch.matmul(torch.matmul(d.A, d.X), d.W) + d.b
    Zg = torch.matmul(d.A, torch.matmul(d.X, d.W)) + d.b
    assert torch.equal(Zf.double(), Z) and torch.equal(Zg.double(), Z)


@pytest.mark.parametrize("shape", lw.MODEL_SHAPES, ids=lw.MODEL_IDS)
def test_model_shapes_qualify_and_the_oracle_is_autograd(shape):
    d, Y, loss, grads = lw.model_reference(*shape)
    p = d.p
    Zs, _ = li.preacts(d.A, d.X, p["conv1.weight"], p["conv1.bias"], p["conv2.weight"], p["conv2.bias"])
    for r in li.measure(Zs, STEPS):
        assert r["odd"] and r["qmax"] < 2 ** 24 and 0.3 <= r["live"] <= 0.7, (shape, r)
    ymax = float(Y.abs().max())
    Ya, lossa, ga = li.fp64_step(d.A, d.X, d.L, p)
    worst = max(rel_to_max(grads[k], ga[k]) for k in PARAM_KEYS)
    gmin = min(float(ga[k].abs().max()) for k in PARAM_KEYS)
    print("S%d hid%d T%d B%d H%d: max |Y| %.3f, oracle vs autograd %.1e, smallest gradient maximum %.1e" % (shape + (ymax, worst, gmin)))
    assert ymax < 0.9
    assert max_abs(Y, Ya) <= 1e-12 and abs(loss - lossa) <= 1e-12 and worst <= 1e-12
    assert gmin > 100 * 1e-7                        # no gradient so small that relative-to-max hides an fp32 error
    assert tuple(p.keys()) == tuple(PARAM_KEYS)


# ==== 4. the geometry ==============================================================================================================
def _src():
    with open(os.path.join(ROOT, "windgnn_amd", "csrc", "gcn_wide.hip")) as f:
        return f.read()


def test_the_geometry_restates_the_source():
    src = _src()
    const = lambda name: int(re.search(r"constexpr int %s = (\d+);" % name, src).group(1))               # noqa: E731
    assert [const(n) for n in ("GW_THREADS", "GW_ROWS", "GW_KC", "GW_NB", "GW_CB", "GW_MAXGRID")] == \
        [lw.THREADS, lw.ROWS, lw.KC, lw.NB, lw.CB, lw.MAXGRID]
    assert "constexpr int GW_SUM_COLS = 16, GW_SUM_ROWS = %d;" % lw.SUM_ROWS in src
    assert const("GW_TB") == lw.TB and "if (Fo <= GW_TB) {" in src                                      # the thin forward's domain
    assert "int gw_grid(int ntiles) { return ntiles < GW_MAXGRID ? ntiles : GW_MAXGRID; }" in src
    assert src.count("for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {") == 3                    # every kernel walks tiles so
    assert src.count("const int nch = (Fi + GW_KC - 1) / GW_KC;") == 2 and src.count("for (int ch = 0; ch < nch; ++ch) {") == 2
    assert "const int n0 = blockIdx.y * GW_NB;" in src and "dim3(gw_grid(ntiles), nb)" in src and "const int nb = cdiv_i(Fo, GW_NB);" in src
    assert "const int c0 = blockIdx.y * GW_CB;" in src and "dim3(grid, cdiv_i(Fo, GW_CB))" in src
    assert "for (int k = 0; k < ks; k += 4)" in src and "S4 = (S + 3) & ~3" in src and "nrt = (S + 15) >> 4" in src
    assert "for (int r = q; r < rows; r += GW_SUM_ROWS) s += partial[(size_t)r * n + i];" in src
    assert src.count("for (int pr = wave; pr < nrt * ncj; pr += GW_THREADS / 64) {") == 3
    # the split-K rule and the workspace plan
    for line in ("const int tiles = gemm_f32_tiles(Fi, Fo);", "int64_t sk = (1024 + tiles - 1) / tiles;",
                 "if (sk > rows / 64) sk = rows / 64;", "return sk < 1 ? 1 : (int)sk;",
                 "p.dbpart = p.v + align_up((size_t)ntiles * S * Fo, 64);",
                 "p.dwpart = p.dbpart + align_up((size_t)gw_grid(ntiles) * Fo, 64);",
                 "p.total = p.dwpart + align_up((size_t)gw_splitk(ntiles, S, Fi, Fo) * Fi * Fo, 64);"):
        assert line in src, line
    with open(os.path.join(ROOT, "windgnn_amd", "csrc", "gemm.hip")) as f:
        gemm = f.read()
    assert "constexpr int BK = 16" in gemm and "p.kchunk = cdiv_i(cdiv_i(g.K, p.splitk), BK) * BK;" in gemm
    assert "*bn = cdiv_i(N, 64) * 64 < cdiv_i(N, 128) * 128 ? 64 : 128;" in gemm
    assert "*bm = (cdiv_i(M, 64) * 64 < cdiv_i(M, 128) * 128 || cdiv_i(M, 128) * cdiv_i(N, *bn) < 512) ? 64 : 128;" in gemm
    # no floating-point atomics in the new file
    assert "atomic" not in src.lower().replace("no floating-point atomics", "")


def test_every_loop_makes_two_trips_with_a_ragged_last_one_somewhere():
    table = {row: lw.loops(*row) for row in lw.TABLE}
    for row, lp in table.items():
        print("S%d %d -> %d x%d: %s" % (row + ("  ".join("%s %d%s" % (k, v[0], "r" if v[1] else "") for k, v in lp.items()),)))
    for loop in next(iter(table.values())):
        rows = [r for r, lp in table.items() if lp[loop][0] >= 2 and lp[loop][1]]
        assert rows, "no table row runs '%s' for two trips with a ragged last one" % loop
    # the figures the table was chosen for
    assert table[lw.TABLE[8]]["tiles per workgroup"] == (3, True) and 2100 - 2 * 1024 == 52
    assert table[lw.TABLE[4]]["K chunks of X"] == (7, True) and table[lw.TABLE[5]]["K chunks of X"] == (9, True)
    assert table[lw.TABLE[5]]["forward column blocks"] == (2, True) and table[lw.TABLE[7]]["forward column blocks"] == (3, True)
    assert table[lw.TABLE[4]]["backward column blocks"] == (2, True) and table[lw.TABLE[2]]["backward column blocks"] == (2, True)
    assert table[lw.TABLE[0]]["split-K chunks of dW"] == (2, True) and lw.splitk(5, 34, 13, 128) == 2
    assert table[lw.TABLE[8]]["partial rows of dW per summing thread"] == (32, False) and lw.splitk(2100, 34, 96, 80) == 512
    assert table[lw.TABLE[8]]["partial rows of db per summing thread"] == (64, False)
    assert table[lw.TABLE[9]]["partial rows of dW per summing thread"] == (2, True) and lw.splitk(40, 34, 65, 2) == 21
    assert table[lw.TABLE[9]]["partial rows of db per summing thread"] == (3, True)
    assert table[lw.TABLE[10]]["tiles per workgroup of the thin forward"] == (3, True) and table[lw.TABLE[10]]["K chunks of the thin forward"] == (3, True)
    assert table[lw.TABLE[9]]["K chunks of the thin forward"] == (3, True) and table[lw.TABLE[1]]["K chunks of the thin forward"] == (4, False)
    assert table[lw.TABLE[8]]["tiles per workgroup of the general forward"] == (3, True)
    assert table[lw.TABLE[5]]["row tiles of 16"] == (1, True) and table[lw.TABLE[2]]["row tiles of 16"] == (4, False)


# ==== 5. planted mistakes ==========================================================================================================
def _step(d, keep_k=None, keep_n=None, keep_tiles=None):
    """fp64 out and dW of relu(A X W + b) with the K range, the output columns or the tiles of a last trip left out."""
    A, X, W, b, dout = (t.double() for t in (d.A, d.X, d.W, d.b, d.dout))
    Z = torch.matmul(torch.matmul(A, X), W) + b
    if keep_k is not None:
        Zm = torch.matmul(torch.matmul(A, X[..., :keep_k]), W[:keep_k]) + b
    else:
        Zm = Z
    out = torch.relu(Zm).clone()
    dZ = dout * (Zm > 0)
    if keep_n is not None:
        out[..., keep_n:] = 0
        dZ = dZ.clone()
        dZ[..., keep_n:] = 0
    if keep_tiles is not None:
        out[keep_tiles:] = 0
        dZ = dZ.clone()
        dZ[keep_tiles:] = 0
    dW = torch.einsum("tsi,tso->io", torch.matmul(A, X), dZ)
    return out, dW


@pytest.mark.parametrize("row", lw.TABLE, ids=lw.IDS)
def test_a_dropped_last_trip_shows_on_the_rows_that_claim_the_loop(row):
    S, Fi, Fo, nt = row
    d, out_r, _, dW_r, _ = lw.layer_reference(*row)
    out, dW = _step(d)
    assert torch.equal(out, out_r) and rel_to_max(dW, dW_r) <= 1e-12
    lp = lw.loops(*row)
    plants = []
    if lp["K chunks of X"][0] >= 2:
        plants.append(("last K chunk", dict(keep_k=(lp["K chunks of X"][0] - 1) * lw.KC)))
    if lp["forward column blocks"][0] >= 2:
        plants.append(("last forward column block", dict(keep_n=(lp["forward column blocks"][0] - 1) * lw.NB)))
    if lp["backward column blocks"][0] >= 2:
        plants.append(("last backward column block", dict(keep_n=(lp["backward column blocks"][0] - 1) * lw.CB)))
    if lp["tiles per workgroup"][0] >= 2:
        plants.append(("last trip's tiles", dict(keep_tiles=(lp["tiles per workgroup"][0] - 1) * lw.grid(nt))))
    for name, kw in plants:
        om, dWm = _step(d, **kw)
        moved = (max_abs(om, out), rel_to_max(dWm, dW))
        print("S%d %d -> %d x%d, %s dropped: out moves %.2g, dW %.2g" % (row + (name,) + moved))
        assert max(moved) > 100 * BAR, (row, name, moved)
    claimed = {name for name, _ in plants}
    if row in (lw.TABLE[8], lw.TABLE[10]):
        assert "last trip's tiles" in claimed
    if row in (lw.TABLE[4], lw.TABLE[5]):
        assert {"last K chunk", "last backward column block"} <= claimed
