"""Host side of series mode (no GPU): include/windgnn_series.h against _lib.EXPORTS_SERIES and the exports of the shared
object, every refusal of the three entry points before any launch (fake device pointers), the stash size against the layout the
header documents, the fold's window ranges against brute force, and series_labels against the reference's windows."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT, WINDOW_FIXTURES
from test_abi_and_host import _c_kind, _ctype_kind
from test_optim_host import _prototypes

OK, ERR_NULL, ERR_SHAPE, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, -1, -2, -4, -5


def _lib():
    from windgnn_amd import _lib as L
    from windgnn_amd import build
    build.build(verbose=False)
    return L, L.load()


def _sd(L, rows=14, T=5, stride=3, n=4, S=7, F=13, H=21, math=0, adj=0, nnz=0, io=0):
    return L.SeriesDims(rows, T, stride, n, S, F, H, math, adj, nnz, io)


def test_series_prototypes_match_the_header_argument_for_argument():
    L, lib = _lib()
    protos = _prototypes("windgnn_series.h")
    assert set(protos) == set(L.EXPORTS_SERIES), set(protos) ^ set(L.EXPORTS_SERIES)
    assert {"wgnn_series_version", "wgnn_series_workspace_bytes", "wgnn_series_stash_bytes", "wgnn_series_fwd",
            "wgnn_series_fwd_last", "wgnn_series_bwd"} == set(protos)
    for name, (ret, args) in protos.items():
        res, argtypes = L.EXPORTS_SERIES[name]
        assert len(args) == len(argtypes), (name, args, argtypes)
        for i, (decl, t) in enumerate(zip(args, argtypes)):
            assert _c_kind(decl) == _ctype_kind(t), (name, i, decl, t)
        want = "ptr" if "*" in ret else {"int": "i32", "size_t": "size"}[ret.replace("const", "").strip()]
        assert _ctype_kind(res) == want, (name, ret, res)
        assert hasattr(lib, name), name                      # exported by the shared object
        assert getattr(lib, name).argtypes == argtypes       # and bound by load()
    assert lib.wgnn_series_version() == L.SERIES_VERSION == 1
    assert lib.wgnn_version() == 122                         # the first header and its version are as they were
    hdr = open(os.path.join(ROOT, "include", "windgnn_series.h")).read()
    assert re.search(r"#define\s+WGNN_SERIES_VERSION\s+1\b", hdr) and '#include "windgnn.h"' in hdr
    assert "wgnn_series" not in open(os.path.join(ROOT, "include", "windgnn.h")).read()
    for other in (L.EXPORTS, L.EXPORTS_OPTIM, L.EXPORTS_SCHED, L.EXPORTS_EVAL, L.EXPORTS_BEST):
        assert not set(other) & set(L.EXPORTS_SERIES)
    from windgnn_amd import build
    assert any(h.endswith("windgnn_series.h") for h in build.HEADERS) and "series.hip" in build.SOURCES
    fields = re.search(r"typedef struct wgnn_series_dims \{(.*?)\}", re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S), flags=re.S).group(1)
    names = [n.strip() for decl in fields.split(";") if decl.strip() for n in decl.replace("int32_t", "").split(",")]
    assert names == [n for n, _ in L.SeriesDims._fields_]


def _calls(lib, L, sd, ws_bytes=1 << 40, null=None):
    """The three entry points on non-NULL fake device pointers (null: the name of one argument passed as NULL): every call
    must be refused on the host before anything is launched.  Returns their three statuses."""
    def P(name, v):
        return C.c_void_p(0 if name == null else v)
    p = L.Params(*([4096] * 8), None)
    g = L.Grads(*([4096] * 8))
    if null == "p.w_hh":
        p.w_hh = None
    if null == "grads.b_ih":
        g.b_ih = None
    sdp = C.byref(sd) if null != "sd" else None
    pp = C.byref(p) if null != "p" else None
    gp = C.byref(g) if null != "grads" else None
    fwd = lib.wgnn_series_fwd(sdp, P("A", 8192), P("Xs", 1 << 20), pp, P("Y", 1 << 24), P("stash", 1 << 28), P("ws", 1 << 40),
                              ws_bytes, None)
    last = lib.wgnn_series_fwd_last(sdp, P("A", 8192), P("Xs", 1 << 20), pp, 0.0, 1.0, P("last", 1 << 24), P("ws", 1 << 40),
                                    ws_bytes, None)
    bwd = lib.wgnn_series_bwd(sdp, P("A", 8192), P("Xs", 1 << 20), pp, P("Y", 1 << 24), P("dY", 1 << 26), P("stash", 1 << 28),
                              gp, P("ws", 1 << 40), ws_bytes, None)
    return fwd, last, bwd


def test_null_arguments_are_refused_before_any_launch():
    L, lib = _lib()
    sd = _sd(L)
    for name in ("sd", "A", "Xs", "p", "p.w_hh", "ws"):
        assert _calls(lib, L, sd, null=name) == (ERR_NULL,) * 3, name
    assert _calls(lib, L, sd, null="Y")[0] == ERR_NULL and _calls(lib, L, sd, null="Y")[2] == ERR_NULL
    assert _calls(lib, L, sd, null="last")[1] == ERR_NULL
    for name in ("dY", "stash", "grads", "grads.b_ih"):
        assert _calls(lib, L, sd, null=name)[2] == ERR_NULL, name


def test_shapes_scope_and_workspace_are_refused_before_any_launch():
    L, lib = _lib()
    assert lib.wgnn_series_workspace_bytes(C.byref(_sd(L))) > 0 and lib.wgnn_series_stash_bytes(C.byref(_sd(L))) > 0
    # (n - 1) * stride + T = 14 = rows fits; one row fewer does not
    shape = [_sd(L, stride=0), _sd(L, n=0), _sd(L, T=0), _sd(L, rows=13), _sd(L, F=12), _sd(L, S=0), _sd(L, H=0), _sd(L, rows=0)]
    for bad in shape:
        assert _calls(lib, L, bad) == (ERR_SHAPE,) * 3, bytes(bad)
        assert lib.wgnn_series_workspace_bytes(C.byref(bad)) == 0 and lib.wgnn_series_stash_bytes(C.byref(bad)) == 0
    # the 2^31 element limits of check_dims, on the front layout (rows * S * 13) and on the recurrence layout (n * T * 4 H)
    for bad in (_sd(L, rows=1 << 22, S=64, T=2, stride=1, n=4), _sd(L, rows=1 << 24, T=1 << 10, stride=1, n=1 << 14, H=128)):
        assert _calls(lib, L, bad) == (ERR_SHAPE,) * 3, bytes(bad)
    # f16x3 / f16 / f16x3g, CSR, a wide GRU, a dense graph above 64 stations, 16-bit I/O: follow-ups, refused
    scope = [_sd(L, math=1), _sd(L, math=2), _sd(L, math=3), _sd(L, adj=1, nnz=20), _sd(L, H=129), _sd(L, S=65), _sd(L, io=1),
             _sd(L, io=2)]
    for bad in scope:
        assert _calls(lib, L, bad) == (ERR_UNSUPPORTED,) * 3, bytes(bad)
        assert lib.wgnn_series_workspace_bytes(C.byref(bad)) == 0 and lib.wgnn_series_stash_bytes(C.byref(bad)) == 0
    sd = _sd(L)
    need = lib.wgnn_series_workspace_bytes(C.byref(sd))
    assert _calls(lib, L, sd, ws_bytes=need - 1) == (ERR_WORKSPACE,) * 3


def _a64(x):
    return (x + 63) // 64 * 64


def _documented_stash_floats(rows, T, n, S, H):
    """The layout in the head comment of include/windgnn_series.h."""
    Ip, Gp, hq = 32 * -(-(13 * S + 1) // 32), 32 * -(-(3 * H) // 32), 16 * -(-(H + 1) // 16)
    big = n * T >= 4096 and Ip <= 512 and Gp <= 512
    g, gi = _a64(rows * Ip), _a64(rows * Gp)
    gates = _a64(-(-n // 16) * T * -(-H // 16) * 1024)
    hprev = _a64(n * T * hq if big else 0)
    return g, gi, gates, hprev


@pytest.mark.parametrize("rows,T,stride,n,S,H", [(4119, 24, 1, 4096, 34, 102), (14, 5, 3, 4, 7, 21), (802, 3, 1, 800, 7, 21),
                                               (4100, 2, 1, 4099, 7, 21), (200, 24, 1, 100, 40, 128)])
def test_stash_is_the_documented_layout_and_its_g_and_gi_scale_with_rows(rows, T, stride, n, S, H):
    L, lib = _lib()
    sd = _sd(L, rows, T, stride, n, S, 13, H)
    got = lib.wgnn_series_stash_bytes(C.byref(sd))
    g, gi, gates, hprev = _documented_stash_floats(rows, T, n, S, H)
    assert got == 4 * (g + gi + gates + hprev)
    # spare trailing rows grow g_s and GI_s alone, by `rows`; the window-major regions do not move
    more = lib.wgnn_series_stash_bytes(C.byref(_sd(L, rows + 64, T, stride, n, S, 13, H)))
    Ip, Gp = 32 * -(-(13 * S + 1) // 32), 32 * -(-(3 * H) // 32)
    assert more - got == 4 * 64 * (Ip + Gp)
    # against the materialised path: its g and GI regions alone hold n * T rows of the same widths
    d = L.Dims(n, T, S, 13, H, 0, 0, 0, 0)
    mat = lib.wgnn_stash_bytes(C.byref(d))
    assert mat >= 4 * (_a64(n * T * Ip) + _a64(n * T * Gp))
    if n * T > rows and n > 768:                             # (up to 768 windows the materialised path's one-window-per-
        assert got < mat                                     # workgroup recurrence keeps smaller gate records)
        assert mat - got >= 4 * (n * T - rows) * (Ip + Gp) - 4 * 4 * 64
    # ... and the workspace has no window-major g / GI / dg either: below the materialised one wherever windows overlap
    ws, ws_mat = lib.wgnn_series_workspace_bytes(C.byref(sd)), lib.wgnn_workspace_bytes(C.byref(d))
    assert ws > 0 and ws_mat > 0
    if n * T >= 2 * rows:
        assert ws < ws_mat, (ws, ws_mat)


def test_headline_shape_stash_is_smaller_than_the_materialised_one():
    L, lib = _lib()
    sd = _sd(L, 4119, 24, 1, 4096, 34, 13, 102)
    d = L.Dims(4096, 24, 34, 13, 102, 0, 0, 0, 0)
    s, m = lib.wgnn_series_stash_bytes(C.byref(sd)), lib.wgnn_stash_bytes(C.byref(d))
    assert 0 < s < m
    g, gi, _, _ = _documented_stash_floats(4119, 24, 4096, 34, 102)
    assert 4 * (g + gi) < 14e6 and m - s > 280e6             # 12.7 MB of g_s + GI_s against 98304 rows of them


@pytest.mark.parametrize("T,stride", [(5, 1), (5, 3), (4, 4), (3, 5), (1, 1)])
def test_coverage_helper_against_brute_force(T, stride):
    from windgnn_amd.series import n_series_windows, series_coverage
    for n in (1, 2, 5):
        for spare in (0, 2):
            rows = (n - 1) * stride + T + spare
            assert n_series_windows(rows, T, stride) >= n
            if spare < stride:
                assert n_series_windows(rows, T, stride) == n
            cov = series_coverage(rows, T, stride, n)
            assert len(cov) == rows
            brute = [[w for w in range(n) if w * stride <= tau < w * stride + T] for tau in range(rows)]
            for tau, (lo, hi) in enumerate(cov):
                assert list(range(lo, hi + 1)) == brute[tau], (tau, lo, hi, brute[tau])      # ascending, contiguous, exact
                assert hi - lo + 1 <= -(-T // stride)
            # uncovered rows are exactly the gaps between windows (stride > T) and the spare trailing rows
            predicted = {tau for tau in range(rows) if tau >= (n - 1) * stride + T or tau % stride >= T}
            assert {tau for tau, (lo, hi) in enumerate(cov) if lo > hi} == predicted
            assert sum(max(hi - lo + 1, 0) for lo, hi in cov) == n * T
    assert n_series_windows(4, 5, 1) == 0
    with pytest.raises(ValueError):
        series_coverage(10, 5, 3, 3)                           # (3 - 1) * 3 + 5 = 11 rows needed
    with pytest.raises(ValueError):
        n_series_windows(10, 5, 0)


@pytest.mark.parametrize("name", WINDOW_FIXTURES)
def test_series_labels_are_the_reference_windows_at_stride_seq_len(name):
    from oracle import windgnn_oracle as orc
    from windgnn_amd.series import n_series_windows, series_labels
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    data, seq, perm = z["data"], int(z["seq"]), z["perm"]
    feat = torch.from_numpy(np.ascontiguousarray(data[:, :, 2:15]))
    Ls, Lw = series_labels(feat, seq, seq)
    xo, yo = orc.make_windows(data, seq)
    assert Lw.shape == yo.shape and torch.equal(Lw, torch.from_numpy(yo))
    assert torch.equal(Lw[perm], torch.from_numpy(z["ys"]))                     # what the reference itself returned
    assert Lw.untyped_storage().data_ptr() == Ls.untyped_storage().data_ptr()   # a view of Ls, not a copy
    assert Ls.shape == (feat.shape[0] - 3, 3 * feat.shape[1])
    # the windows themselves: series row w * seq + t
    n = n_series_windows(feat.shape[0], seq, seq)
    assert n == xo.shape[0]
    assert torch.equal(feat[: n * seq].reshape(n, seq, *feat.shape[1:]), torch.from_numpy(xo))
    # stride 1: window w, row t is hour w + t
    _, L1 = series_labels(feat, seq, 1, n_windows=5)
    for w in range(5):
        assert torch.equal(L1[w], Ls[w:w + seq])
    with pytest.raises(RuntimeError, match=r"\+3 h label"):                     # every stride-1 window: the last ones' labels do not fit
        series_labels(feat, seq, 1)
    with pytest.raises(RuntimeError, match=r"\+3 h label"):
        series_labels(feat[: seq * 2 + 1], seq, seq)


def test_python_layers_refuse_what_is_out_of_scope_before_any_launch():
    import windgnn_amd
    from windgnn_amd.series import forward_last_series
    m = windgnn_amd.GCN_GRU(13, 13, 13, 4 * 13, 12)
    with pytest.raises(RuntimeError, match=r"MI355X|no CPU fallback"):
        m.forward_series(torch.rand(4, 4), torch.rand(9, 4, 13), 3)
    with pytest.raises(RuntimeError, match=r"series must be"):
        m.forward_series(torch.rand(4, 4), torch.rand(1, 9, 4, 13), 3)
    other = windgnn_amd.GCN_GRU(7, 9, 13, 4 * 13, 12)
    with pytest.raises(RuntimeError, match=r"13 / 13.*make_windows"):
        other.forward_series(torch.rand(4, 4), torch.rand(9, 4, 7), 3)
    with pytest.raises(RuntimeError, match=r"13 / 13.*make_windows"):
        forward_last_series(other, torch.rand(4, 4), torch.rand(9, 4, 7), 3, 0.0, 1.0)
    x3 = windgnn_amd.GCN_GRU(13, 13, 13, 4 * 13, 12, math="f16x3")
    with pytest.raises(RuntimeError, match=r"exact fp32.*make_windows"):
        x3.forward_series(torch.rand(4, 4), torch.rand(9, 4, 13), 3)
