"""Host side of series training (no GPU): include/windgnn_series_train.h against _lib.EXPORTS_SERIES_TRAIN and the exports of the
shared object, every refusal of wgnn_series_fwd_loss / wgnn_series_bwd_mse before any launch (fake device pointers), the size of
loss_buf, and the refusals of TrainStep.step_series / forward_backward_series on a CPU-constructed step."""
import ctypes as C
import math
import os
import re

import pytest
import torch

from conftest import ROOT
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


def test_series_train_prototypes_match_the_header_argument_for_argument():
    L, lib = _lib()
    protos = _prototypes("windgnn_series_train.h")
    assert set(protos) == set(L.EXPORTS_SERIES_TRAIN), set(protos) ^ set(L.EXPORTS_SERIES_TRAIN)
    assert {"wgnn_series_train_version", "wgnn_series_loss_bytes", "wgnn_series_fwd_loss", "wgnn_series_bwd_mse"} <= set(protos)
    for name, (ret, args) in protos.items():
        res, argtypes = L.EXPORTS_SERIES_TRAIN[name]
        assert len(args) == len(argtypes), (name, args, argtypes)
        for i, (decl, t) in enumerate(zip(args, argtypes)):
            assert _c_kind(decl) == _ctype_kind(t), (name, i, decl, t)
        want = "ptr" if "*" in ret else {"int": "i32", "size_t": "size"}[ret.replace("const", "").strip()]
        assert _ctype_kind(res) == want, (name, ret, res)
        assert hasattr(lib, name), name                      # exported by the shared object
        assert getattr(lib, name).argtypes == argtypes       # and bound by load()
    assert lib.wgnn_series_train_version() == L.SERIES_TRAIN_VERSION == 1
    assert lib.wgnn_version() == 122 and lib.wgnn_series_version() == 1      # the earlier headers and versions are as they were
    hdr = open(os.path.join(ROOT, "include", "windgnn_series_train.h")).read()
    assert re.search(r"#define\s+WGNN_SERIES_TRAIN_VERSION\s+1\b", hdr) and '#include "windgnn_series.h"' in hdr
    for other in ("windgnn.h", "windgnn_series.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert "wgnn_series_train" not in text and "wgnn_series_fwd_loss" not in text and "wgnn_series_bwd_mse" not in text
    for other in (L.EXPORTS, L.EXPORTS_OPTIM, L.EXPORTS_SCHED, L.EXPORTS_EVAL, L.EXPORTS_BEST, L.EXPORTS_SERIES):
        assert not set(other) & set(L.EXPORTS_SERIES_TRAIN)
    from windgnn_amd import build
    assert any(h.endswith("windgnn_series_train.h") for h in build.HEADERS)


def _calls(lib, L, sd, ws_bytes=1 << 40, null=None, ls_rows=14, grad_scale=1.0):
    """Both entry points on non-NULL fake device pointers (null: the name of one argument passed as NULL): every call must be
    refused on the host before anything is launched.  Returns their two statuses."""
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
    fwd = lib.wgnn_series_fwd_loss(sdp, P("A", 8192), P("Xs", 1 << 20), pp, P("Ls", 1 << 22), ls_rows, P("Y", 1 << 24),
                                   P("stash", 1 << 28), P("loss_buf", 1 << 30), P("ws", 1 << 40), ws_bytes, None)
    bwd = lib.wgnn_series_bwd_mse(sdp, P("A", 8192), P("Xs", 1 << 20), pp, P("Y", 1 << 24), P("Ls", 1 << 22), ls_rows,
                                  grad_scale, P("stash", 1 << 28), P("loss_buf", 1 << 30), P("loss", 1 << 32), gp,
                                  P("ws", 1 << 40), ws_bytes, None)
    return fwd, bwd


def test_null_arguments_are_refused_before_any_launch():
    L, lib = _lib()
    sd = _sd(L)
    for name in ("sd", "A", "Xs", "p", "p.w_hh", "ws", "Ls", "loss_buf", "Y"):
        assert _calls(lib, L, sd, null=name) == (ERR_NULL,) * 2, name
    for name in ("loss", "stash", "grads", "grads.b_ih"):
        assert _calls(lib, L, sd, null=name)[1] == ERR_NULL, name
    # the order is wgnn_series_fwd's / wgnn_series_bwd's: the forward reports a NULL Y before the dims, the backward after
    p = L.Params(*([4096] * 8), None)
    for bad, rc in ((_sd(L, F=12), ERR_SHAPE), (_sd(L, math=1), ERR_UNSUPPORTED)):
        assert _calls(lib, L, bad, null="Y") == (ERR_NULL, rc), bytes(bad)
        assert lib.wgnn_series_fwd(C.byref(bad), C.c_void_p(8192), C.c_void_p(1 << 20), C.byref(p), None, C.c_void_p(1 << 28),
                                   C.c_void_p(1 << 40), 1 << 40, None) == ERR_NULL
        assert _calls(lib, L, bad, null="Ls") == (rc,) * 2             # every other pointer comes after the dims


def test_shapes_scope_and_workspace_are_refused_before_any_launch():
    L, lib = _lib()
    # wgnn_series_fwd's own refusals, in its order: shape before scope
    shape = [_sd(L, stride=0), _sd(L, n=0), _sd(L, T=0), _sd(L, rows=13), _sd(L, F=12), _sd(L, S=0), _sd(L, H=0), _sd(L, rows=0),
             _sd(L, rows=1 << 22, S=64, T=2, stride=1, n=4), _sd(L, rows=1 << 24, T=1 << 10, stride=1, n=1 << 14, H=128)]
    for bad in shape:
        assert _calls(lib, L, bad, ls_rows=1 << 24) == (ERR_SHAPE,) * 2, bytes(bad)
        assert lib.wgnn_series_loss_bytes(C.byref(bad)) == 0 and lib.wgnn_series_status_offset(C.byref(bad)) == 0
    scope = [_sd(L, math=1), _sd(L, math=2), _sd(L, math=3), _sd(L, adj=1, nnz=20), _sd(L, H=129), _sd(L, S=65), _sd(L, io=1),
             _sd(L, io=2)]
    for bad in scope:
        assert _calls(lib, L, bad) == (ERR_UNSUPPORTED,) * 2, bytes(bad)
        assert lib.wgnn_series_loss_bytes(C.byref(bad)) == 0
    assert _calls(lib, L, _sd(L, math=1, F=12)) == (ERR_SHAPE,) * 2          # shape is reported before scope
    sd = _sd(L)
    # the label series: (n - 1) * stride + T = 14 rows are needed (spare series rows need no labels) ...
    assert _calls(lib, L, sd, ls_rows=13) == (ERR_SHAPE,) * 2
    assert _calls(lib, L, _sd(L, rows=20), ls_rows=14, null="ws") == (ERR_NULL,) * 2      # (14 is enough: the next check is reached)
    assert _calls(lib, L, sd, ls_rows=0) == (ERR_SHAPE,) * 2 and _calls(lib, L, sd, ls_rows=-1) == (ERR_SHAPE,) * 2
    # ... and its 32-bit offsets: ls_rows * H < 2^31
    assert _calls(lib, L, sd, ls_rows=-(-(1 << 31) // 21)) == (ERR_SHAPE,) * 2
    assert _calls(lib, L, sd, ls_rows=((1 << 31) - 1) // 21, null="ws") == (ERR_NULL,) * 2
    # grad_scale: finite and > 0 (the forward takes none)
    for bad in (0.0, -1.0, math.inf, math.nan):
        assert _calls(lib, L, sd, grad_scale=bad)[1] == ERR_SHAPE, bad
    # NULL is reported before the label rows, the label rows before the workspace
    assert _calls(lib, L, sd, ls_rows=13, null="Ls") == (ERR_NULL,) * 2
    need = lib.wgnn_series_workspace_bytes(C.byref(sd))
    assert _calls(lib, L, sd, ws_bytes=need - 1) == (ERR_WORKSPACE,) * 2
    assert _calls(lib, L, sd, ws_bytes=need - 1, ls_rows=13) == (ERR_SHAPE,) * 2
    assert _calls(lib, L, sd, ws_bytes=need - 1, grad_scale=0.0)[1] == ERR_SHAPE


def test_loss_bytes_depend_on_the_window_count_alone():
    L, lib = _lib()
    size = lambda **kw: lib.wgnn_series_loss_bytes(C.byref(_sd(L, **kw)))   # noqa: E731
    assert size() > 0
    for n in (1, 16, 17, 32, 33, 4096):
        rows = (n - 1) * 3 + 5
        got = size(rows=rows, n=n)
        assert got == 4 * (2 * -(-n // 16) + 4), (n, got)                    # the documented layout: pairs, tag, three spare words
        assert size(rows=rows + 64, n=n) == got                              # independent of rows
        assert size(rows=rows, n=n, S=34, H=102) == got                      # ... and of the widths
    assert size(rows=53, n=17) > size(rows=50, n=16) and size(rows=101, n=33) > size(rows=98, n=32)   # grows with ceil(n / 16)
    # the status block of the window-major half lies behind the hour-major half's workspace, inside the workspace
    sd = _sd(L)
    off = lib.wgnn_series_status_offset(C.byref(sd))
    assert 256 <= off <= lib.wgnn_series_workspace_bytes(C.byref(sd)) - 256 and off % 256 == 0


def _cpu_step(**kw):
    import windgnn_amd
    from windgnn_amd.trainer import TrainStep
    math_ = kw.pop("math", "f32")
    return TrainStep(windgnn_amd.GCN_GRU(13, 13, 13, 7 * 13, 21, math=math_), **kw)


def test_step_series_refuses_what_is_out_of_scope_with_the_option_and_the_alternative():
    from windgnn_amd.distributed import grad_block_plan
    A, series, Ls = torch.rand(7, 7), torch.rand(14, 7, 13), torch.rand(14, 21)
    for call in ("step_series", "forward_backward_series"):
        def go(tr, A=A, series=series, Ls=Ls, **kw):
            return getattr(tr, call)(A, series, Ls, 5, 3, **kw)
        with pytest.raises(RuntimeError, match=r"carry_state=True.*make_windows.*TrainStep\.step"):
            go(_cpu_step(carry_state=True))
        with pytest.raises(RuntimeError, match=r"overlap_collectives=True.*overlap_collectives=False.*make_windows"):
            go(_cpu_step(overlap_collectives=True))
        with pytest.raises(RuntimeError, match=r"math != 'f32'.*math='f32'.*make_windows"):
            go(_cpu_step(math="f16x3"))
        # a blocked TrainStep cannot be built without a process group; the refusal reads the plan alone
        blocked = _cpu_step()
        blocked.plan = grad_block_plan(7, 21, 2, 128)
        with pytest.raises(RuntimeError, match=r"grad_blocks.*make_windows.*TrainStep\.step"):
            go(blocked)

        class Csr:
            blob = torch.zeros(4, dtype=torch.int32)
        with pytest.raises(RuntimeError, match=r"CsrAdjacency.*dense.*make_windows"):
            go(_cpu_step(), A=Csr())
        unfused = _cpu_step()
        unfused.model.fused = False
        with pytest.raises(RuntimeError, match=r"13 / 13.*autograd"):
            go(unfused)
        # the label series: (n - 1) * stride + T = 14 rows of H = 21 values
        with pytest.raises(RuntimeError, match=r"label series Ls must be \[rows >= .* = 14, H = 21\].*series_labels"):
            go(_cpu_step(), Ls=torch.rand(13, 21))
        with pytest.raises(RuntimeError, match=r"label series Ls must be"):
            go(_cpu_step(), Ls=torch.rand(14, 20))
        with pytest.raises(RuntimeError, match=r"label series Ls must be"):
            go(_cpu_step(), Ls=torch.rand(4, 5, 21))              # the window view L is not what series mode takes
        with pytest.raises(RuntimeError, match=r"n_windows = 5.*holds 4 windows"):
            go(_cpu_step(), n_windows=5)
        with pytest.raises(RuntimeError, match=r"series must be \[rows, S, 13\]"):
            go(_cpu_step(), series=torch.rand(1, 14, 7, 13))
        # in scope: the first thing that needs the device says so (nothing was launched, no step counted)
        tr = _cpu_step()
        with pytest.raises(RuntimeError, match=r"MI355X|no CPU fallback"):
            go(tr)
        assert tr.steps == 0
    # no window on a rank without a process group: the step that has nothing to do says so
    with pytest.raises(RuntimeError, match=r"at least one window"):
        _cpu_step().step_series(A, series, Ls, 5, 3, n_windows=0)
    with pytest.raises(RuntimeError, match=r"at least one window"):
        _cpu_step().forward_backward_series(A, series[:4], Ls, 5, 3)
