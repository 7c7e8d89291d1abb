"""Host side of series mode on a table of window starts (no GPU): include/windgnn_series_at.h against _lib.EXPORTS_SERIES_AT and
the exports of the shared object, every refusal of the five entry points before any launch (fake device pointers), the host
helpers segment_starts / starts_coverage against brute force, the ValueErrors of the Python layer, TrainStep's refusals, and the
qualification on the fp64 oracle alone of the inputs tests/test_gpu_series_at.py runs."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import series_at_cases as sc
from conftest import PARAM_KEYS, ROOT, rel_to_max
from test_abi_and_host import _c_kind, _ctype_kind
from test_optim_host import _prototypes

OK, ERR_NULL, ERR_SHAPE, ERR_WORKSPACE, ERR_UNSUPPORTED = 0, -1, -2, -4, -5


def _lib():
    from windgnn_amd import _lib as L
    from windgnn_amd import build
    build.build(verbose=False)
    return L, L.load()


def _sd(L, rows=14, T=5, stride=0, n=4, S=7, F=13, H=21, math=0, adj=0, nnz=0, io=0):
    return L.SeriesDims(rows, T, stride, n, S, F, H, math, adj, nnz, io)


def test_series_at_prototypes_match_the_header_argument_for_argument():
    L, lib = _lib()
    protos = _prototypes("windgnn_series_at.h")
    assert set(protos) == set(L.EXPORTS_SERIES_AT), set(protos) ^ set(L.EXPORTS_SERIES_AT)
    assert {"wgnn_series_at_version", "wgnn_series_at_workspace_bytes", "wgnn_series_at_stash_bytes", "wgnn_series_at_loss_bytes",
            "wgnn_series_at_status_offset", "wgnn_series_fwd_at", "wgnn_series_fwd_last_at", "wgnn_series_bwd_at",
            "wgnn_series_fwd_loss_at", "wgnn_series_bwd_mse_at"} == set(protos)
    for name, (ret, args) in protos.items():
        res, argtypes = L.EXPORTS_SERIES_AT[name]
        assert len(args) == len(argtypes), (name, args, argtypes)
        for i, (decl, t) in enumerate(zip(args, argtypes)):
            assert _c_kind(decl) == _ctype_kind(t), (name, i, decl, t)
        want = "ptr" if "*" in ret else {"int": "i32", "size_t": "size"}[ret.replace("const", "").strip()]
        assert _ctype_kind(res) == want, (name, ret, res)
        assert hasattr(lib, name), name                      # exported by the shared object
        assert getattr(lib, name).argtypes == argtypes       # and bound by load()
    # the five compute entry points are the strided ones with `const int32_t* starts` after Xs
    strided = dict(_prototypes("windgnn_series.h"), **_prototypes("windgnn_series_train.h"))
    for name in ("fwd", "fwd_last", "bwd", "fwd_loss", "bwd_mse"):
        ret, args = protos["wgnn_series_%s_at" % name]
        ret0, args0 = strided["wgnn_series_" + name]
        assert ret == ret0 and args[:3] == args0[:3] and args[3] == "const int32_t* starts" and args[4:] == args0[3:], name
    assert lib.wgnn_series_at_version() == L.SERIES_AT_VERSION == 1
    assert lib.wgnn_version() == 122 and lib.wgnn_series_version() == 1 and lib.wgnn_series_train_version() == 1
    hdr = open(os.path.join(ROOT, "include", "windgnn_series_at.h")).read()
    assert re.search(r"#define\s+WGNN_SERIES_AT_VERSION\s+1\b", hdr) and re.search(r"#define\s+WGNN_STATUS_WINDOW_START\s+16u", hdr)
    assert L.STATUS_WINDOW_START == 16
    for other in ("windgnn.h", "windgnn_series.h", "windgnn_series_train.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert "series_at" not in text and "_at(" not in text and "WINDOW_START" not in text, other
    for other in (L.EXPORTS, L.EXPORTS_OPTIM, L.EXPORTS_SCHED, L.EXPORTS_EVAL, L.EXPORTS_BEST, L.EXPORTS_SERIES,
                  L.EXPORTS_SERIES_TRAIN):
        assert not set(other) & set(L.EXPORTS_SERIES_AT)
    from windgnn_amd import build
    assert any(h.endswith("windgnn_series_at.h") for h in build.HEADERS)


def _calls(lib, L, sd, ws_bytes=1 << 40, null=None, ls_rows=14, grad_scale=1.0):
    """The five entry points on non-NULL fake device pointers (null: the name of one argument passed as NULL): every call must
    be refused on the host before anything is launched.  Returns their statuses: fwd, fwd_last, bwd, fwd_loss, bwd_mse."""
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
    head = (sdp, P("A", 8192), P("Xs", 1 << 20), P("starts", 1 << 21), pp)
    tail = (P("ws", 1 << 40), ws_bytes, None)
    return (lib.wgnn_series_fwd_at(*head, P("Y", 1 << 24), P("stash", 1 << 28), *tail),
            lib.wgnn_series_fwd_last_at(*head, 0.0, 1.0, P("Y", 1 << 24), *tail),
            lib.wgnn_series_bwd_at(*head, P("Y", 1 << 24), P("dY", 1 << 26), P("stash", 1 << 28), gp, *tail),
            lib.wgnn_series_fwd_loss_at(*head, P("Ls", 1 << 22), ls_rows, P("Y", 1 << 24), P("stash", 1 << 28),
                                        P("loss_buf", 1 << 30), *tail),
            lib.wgnn_series_bwd_mse_at(*head, P("Y", 1 << 24), P("Ls", 1 << 22), ls_rows, grad_scale, P("stash", 1 << 28),
                                       P("loss_buf", 1 << 30), P("loss", 1 << 32), gp, *tail))


def test_every_refusal_comes_before_any_launch_in_the_strided_order():
    L, lib = _lib()
    sd = _sd(L)
    for name in ("sd", "A", "Xs", "starts", "p", "p.w_hh", "ws", "Y"):
        assert _calls(lib, L, sd, null=name) == (ERR_NULL,) * 5, name
    for name in ("Ls", "loss_buf"):
        assert _calls(lib, L, sd, null=name)[3:] == (ERR_NULL,) * 2, name
    for name in ("grads", "grads.b_ih"):
        got = _calls(lib, L, sd, null=name)
        assert got[2] == got[4] == ERR_NULL, name
    # stride = 0 means "table" here and nowhere else; T > rows; n may exceed rows - T + 1
    assert _calls(lib, L, _sd(L, stride=1)) == (ERR_SHAPE,) * 5 and _calls(lib, L, _sd(L, stride=-1)) == (ERR_SHAPE,) * 5
    p = L.Params(*([4096] * 8), None)
    assert lib.wgnn_series_fwd(C.byref(sd), C.c_void_p(8192), C.c_void_p(1 << 20), C.byref(p), C.c_void_p(1 << 24), None,
                               C.c_void_p(1 << 40), 1 << 40, None) == ERR_SHAPE           # the strided family still refuses it
    assert lib.wgnn_series_workspace_bytes(C.byref(sd)) == 0 and lib.wgnn_series_at_workspace_bytes(C.byref(_sd(L, stride=1))) == 0
    for bad in (_sd(L, T=15), _sd(L, n=0), _sd(L, T=0), _sd(L, rows=0), _sd(L, F=12), _sd(L, S=0), _sd(L, H=0),
                _sd(L, rows=1 << 22, S=64, T=2, n=4)):
        assert _calls(lib, L, bad, ls_rows=1 << 24) == (ERR_SHAPE,) * 5, bytes(bad)
        assert lib.wgnn_series_at_workspace_bytes(C.byref(bad)) == 0 and lib.wgnn_series_at_loss_bytes(C.byref(bad)) == 0
    need = lib.wgnn_series_at_workspace_bytes(C.byref(_sd(L, n=40)))
    assert need > 0 and _calls(lib, L, _sd(L, n=40), ws_bytes=need - 1) == (ERR_WORKSPACE,) * 5          # n = 40 > rows - T + 1 = 10
    for bad in (_sd(L, math=1), _sd(L, math=3), _sd(L, adj=1, nnz=20), _sd(L, H=129), _sd(L, S=65), _sd(L, io=1)):
        assert _calls(lib, L, bad) == (ERR_UNSUPPORTED,) * 5, bytes(bad)
    assert _calls(lib, L, _sd(L, math=1, F=12)) == (ERR_SHAPE,) * 5          # shape is reported before scope
    assert _calls(lib, L, _sd(L, math=1), null="starts") == (ERR_UNSUPPORTED,) * 5      # the dims before the pointers ...
    assert _calls(lib, L, _sd(L, math=1), null="Y")[:2] == (ERR_NULL,) * 2              # ... except the forward's NULL Y
    # the label series: a window may start anywhere, so `rows` rows are needed, and ls_rows * H < 2^31
    assert _calls(lib, L, sd, ls_rows=13)[3:] == (ERR_SHAPE,) * 2 and _calls(lib, L, sd, ls_rows=13)[:3] != (ERR_SHAPE,) * 3
    assert _calls(lib, L, sd, ls_rows=14, null="ws")[3:] == (ERR_NULL,) * 2
    assert _calls(lib, L, sd, ls_rows=-(-(1 << 31) // 21))[3:] == (ERR_SHAPE,) * 2
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert _calls(lib, L, sd, grad_scale=bad)[4] == ERR_SHAPE, bad
    need = lib.wgnn_series_at_workspace_bytes(C.byref(sd))
    assert _calls(lib, L, sd, ws_bytes=need - 1) == (ERR_WORKSPACE,) * 5
    assert _calls(lib, L, sd, ws_bytes=need - 1, null="starts") == (ERR_NULL,) * 5        # NULL before the workspace


def test_sizes_are_those_of_the_two_layouts_and_do_not_depend_on_a_table():
    L, lib = _lib()
    A64 = lambda x: -(-x // 64) * 64   # noqa: E731
    for cid in ("irregular", "real_widths", "K4_big", "K32_big", "K8_small"):
        S, H, rows, T, starts, _ = sc.case(cid)
        n = len(starts)
        at = _sd(L, rows=rows, T=T, n=n, S=S, H=H)
        Ip, Gp, hq = 32 * -(-(13 * S + 1) // 32), 32 * -(-3 * H // 32), 16 * -(-(H + 1) // 16)
        big = n * T >= 4096 and Ip <= 512 and Gp <= 512
        assert big == cid.endswith("_big")
        stash = A64(rows * Ip) + A64(rows * Gp) + A64(-(-n // 16) * T * -(-H // 16) * 1024) + A64(n * T * hq if big else 0)
        assert lib.wgnn_series_at_stash_bytes(C.byref(at)) == 4 * stash, cid                  # windgnn_series.h's layout
        assert lib.wgnn_series_at_loss_bytes(C.byref(at)) == 4 * (2 * -(-n // 16) + 4)
        off = lib.wgnn_series_at_status_offset(C.byref(at))
        assert 256 <= off <= lib.wgnn_series_at_workspace_bytes(C.byref(at)) - 256 and off % 256 == 0
        if n <= rows - T + 1:       # the strided dims of the same counts: the same plan
            st = _sd(L, rows=rows, T=T, stride=1, n=n, S=S, H=H)
            for q in ("workspace_bytes", "stash_bytes", "loss_bytes", "status_offset"):
                assert getattr(lib, "wgnn_series_at_" + q)(C.byref(at)) == getattr(lib, "wgnn_series_" + q)(C.byref(st)) > 0, (cid, q)


# ---- the host helpers ------------------------------------------------------------------------------------------------------
def test_segment_starts_agrees_with_brute_force():
    from windgnn_amd.series import segment_starts
    rng = np.random.default_rng(0)
    cases = [([(2, 10), (15, 3), (20, 12)], 5, 1, 3),        # a segment shorter than T, a horizon of 3
             ([(0, 30), (34, 32)], 24, 1, 0), ([(0, 30), (34, 32)], 24, 1, 3), ([(3, 9)], 9, 2, 0), ([(3, 9)], 7, 2, 0),
             ([(0, 4)], 5, 1, 0), ([], 5, 1, 0), ([(0, 12), (6, 12)], 4, 3, 1)]                       # overlapping: duplicates
    for _ in range(20):
        segs, at = [], 0
        for _ in range(int(rng.integers(1, 5))):
            at += int(rng.integers(0, 6))
            length = int(rng.integers(0, 15))
            segs.append((at, length))
            at += length
        cases.append((segs, int(rng.integers(1, 7)), int(rng.integers(1, 4)), int(rng.integers(0, 4))))
    for segs, T, stride, horizon in cases:
        want = []
        for first, count in segs:
            clean = set(range(first, first + count))
            want += [s for s in range(first, first + count, stride) if set(range(s, s + T + horizon)) <= clean]
        assert segment_starts(segs, T, stride, horizon) == sorted(want), (segs, T, stride, horizon)
    assert segment_starts([(2, 10), (15, 3), (20, 12)], 5, 1, 3) == [2, 3, 4, 20, 21, 22, 23, 24]
    assert segment_starts([(0, 12), (6, 12)], 4, 3, 1) == [0, 3, 6, 6, 9, 12]
    for bad in ((0, 1, 0), (3, 0, 0), (3, 1, -1)):
        with pytest.raises(ValueError, match="segment_starts"):
            segment_starts([(0, 9)], *bad)


def test_starts_coverage_agrees_with_brute_force():
    from windgnn_amd.series import starts_coverage
    S, H, rows, T, starts, _ = sc.case("irregular")
    tables = [(starts, T, rows), (sc.SMALL_TABLE, 3, 36), (sc.BIG_TABLE, 16, 272), (sc.real_widths()[4], 24, 66), ([], 3, 5),
              ([0, 0, 0, 0], 2, 3), ([4], 1, 5)]
    for st, T_, rows_ in tables:
        cov = starts_coverage(st, T_, rows_)
        assert cov.shape == (rows_, 2)
        for tau in range(rows_):
            want = [w for w, s in enumerate(st) if s <= tau < s + T_]
            lo, hi = cov[tau]
            assert list(range(lo, hi)) == want, (tau, lo, hi, want)
    cov = starts_coverage(starts, T, rows)
    depth = cov[:, 1] - cov[:, 0]
    assert depth[9] == 6 > T and [t for t in range(rows) if depth[t] == 0] == [0, 1, 18, 19, 27, 28, 29]   # what the issue lists
    assert len(starts) == 19 and len(starts) % 16 == 3 and starts[0] > 0 and starts[-1] == rows - T and len(set(starts)) < 19
    for bad in ([3, 2], [-1, 0], [0, rows - T + 1]):
        with pytest.raises(ValueError, match="starts_coverage"):
            starts_coverage(bad, T, rows)


def test_the_fold_restated_from_the_coverage_is_the_sum_over_the_materialised_windows():
    """dGIs[tau] = sum over w in [lo, hi) of D[w, tau - starts[w]] equals the scatter-add of every window's rows, and with it
    the hour-major weight-gradient product equals the window-major one: sum_w,t D[w, t]^T g[starts[w] + t] = dGIs^T g_s."""
    from windgnn_amd.series import starts_coverage
    S, H, rows, T, starts, _ = sc.case("irregular")
    rng = np.random.default_rng(1)
    D, g = rng.standard_normal((len(starts), T, 6)), rng.standard_normal((rows, 4))
    fold = np.zeros((rows, 6))
    for tau, (lo, hi) in enumerate(starts_coverage(starts, T, rows)):
        for w in range(lo, hi):
            fold[tau] += D[w, tau - starts[w]]
    brute = np.zeros((rows, 6))
    for w, s in enumerate(starts):
        brute[s:s + T] += D[w]
    assert np.array_equal(fold, brute)                    # the same terms in the same (ascending w) order
    windows = sum(D[w, t][:, None] * g[s + t][None, :] for w, s in enumerate(starts) for t in range(T))
    assert np.abs(fold.T @ g - windows).max() <= 1e-12 * np.abs(windows).max()


# ---- the Python layer's refusals -------------------------------------------------------------------------------------------
def test_host_tables_are_checked_before_upload_and_stride_with_starts_is_refused():
    import windgnn_amd
    from windgnn_amd.series import forward_last_series
    model = windgnn_amd.GCN_GRU(13, 13, 13, 7 * 13, 21)
    A, series = torch.rand(7, 7), torch.rand(14, 7, 13)
    for call in (lambda **kw: model.forward_series(A, series, 5, **kw),
                 lambda **kw: forward_last_series(model, A, series, 5, 0.0, 1.0, **kw)):
        with pytest.raises(ValueError, match=r"stride= or starts=, not both"):
            call(stride=1, starts=[0, 1])
        with pytest.raises(ValueError, match=r"n_windows= belongs to stride="):
            call(n_windows=2, starts=[0, 1])
        with pytest.raises(ValueError, match=r"starts\[1\] = 10.*0 \.\. 9"):
            call(starts=[0, 10])
        with pytest.raises(ValueError, match=r"starts\[0\] = -1"):
            call(starts=torch.tensor([-1, 3]))
        with pytest.raises(ValueError, match=r"integers"):
            call(starts=[0.0, 1.0])
        with pytest.raises(ValueError, match=r"integers"):
            call(starts=torch.tensor([0.5]))
        with pytest.raises(ValueError, match=r"1-D"):
            call(starts=[[0, 1]])
        with pytest.raises(RuntimeError, match=r"MI355X|no CPU fallback"):      # in scope: the device is the next thing asked for
            call(starts=[3, 0, 9, 3])
    # the raw wrappers take the table as the kernels do, non-decreasing; a host table that is not is refused before upload
    from windgnn_amd.series import _starts_table
    with pytest.raises(ValueError, match=r"non-decreasing.*starts\[1\] = 2 < starts\[0\] = 3"):
        _starts_table([3, 2], 14, 5, torch.device("cpu"), "series_forward_raw", ordered=True)
    assert _starts_table([3, 2], 14, 5, torch.device("cpu"), "x", ordered=False).tolist() == [3, 2]


def _cpu_step(**kw):
    import windgnn_amd
    from windgnn_amd.trainer import TrainStep
    math_ = kw.pop("math", "f32")
    return TrainStep(windgnn_amd.GCN_GRU(13, 13, 13, 7 * 13, 21, math=math_), **kw)


def test_step_series_with_a_table_refuses_what_is_out_of_scope_and_names_the_option():
    from windgnn_amd.distributed import grad_block_plan
    A, series, Ls = torch.rand(7, 7), torch.rand(14, 7, 13), torch.rand(14, 21)
    for call in ("step_series", "forward_backward_series"):
        def go(tr, A=A, series=series, Ls=Ls, starts=(0, 3, 3, 9), **kw):
            return getattr(tr, call)(A, series, Ls, 5, starts=list(starts), **kw)
        with pytest.raises(RuntimeError, match=r"carry_state=True.*make_windows.*TrainStep\.step"):
            go(_cpu_step(carry_state=True))
        with pytest.raises(RuntimeError, match=r"overlap_collectives=True.*overlap_collectives=False.*make_windows"):
            go(_cpu_step(overlap_collectives=True))
        with pytest.raises(RuntimeError, match=r"math != 'f32'.*math='f32'.*make_windows"):
            go(_cpu_step(math="f16x3"))
        blocked = _cpu_step()
        blocked.plan = grad_block_plan(7, 21, 2, 128)
        with pytest.raises(RuntimeError, match=r"grad_blocks.*make_windows.*TrainStep\.step"):
            go(blocked)
        with pytest.raises(ValueError, match=r"stride= or starts=, not both"):
            go(_cpu_step(), stride=1)
        with pytest.raises(ValueError, match=r"n_windows= belongs to stride="):
            go(_cpu_step(), n_windows=4)
        with pytest.raises(ValueError, match=r"starts\[2\] = 10"):
            go(_cpu_step(), starts=(0, 3, 10))
        # the label series needs a row for every row of the series: a window may start anywhere
        with pytest.raises(RuntimeError, match=r"with starts= the label series Ls must be \[rows >= the series' 14, H = 21\]"):
            go(_cpu_step(), Ls=torch.rand(13, 21))
        tr = _cpu_step()
        with pytest.raises(RuntimeError, match=r"MI355X|no CPU fallback"):       # in scope: nothing launched, no step counted
            go(tr)
        assert tr.steps == 0
    # an empty table is the empty shard: without a process group the step that has nothing to do says so
    with pytest.raises(RuntimeError, match=r"at least one window"):
        _cpu_step().step_series(A, series, Ls, 5, starts=[])
    with pytest.raises(RuntimeError, match=r"at least one window"):
        _cpu_step().forward_backward_series(A, series, Ls, 5, starts=torch.empty(0, dtype=torch.int64))


# ---- input qualification on the oracle alone ---------------------------------------------------------------------------------
def test_every_case_has_a_relu_margin_and_selects_its_instance():
    for cid in ["irregular", "real_widths"] + list(sc.INSTANCE_CASES):
        r = sc.reference(cid)
        assert r.margin > 1e-5, (cid, r.margin)
        assert not torch.isnan(r.Yo).any() and r.loss_o < 1.0, cid          # no uncovered (1e3) label row entered the loss
    assert sc.BWD_KS3 == tuple(sc.bwd_ks3(sc.first_h(k)) for k in sc.FWD_KS) == tuple(sc.bwd_ks3(4 * k) for k in sc.FWD_KS)
    for K in sc.FWD_KS:
        S, H, rows, T, starts, _ = sc.INSTANCE_CASES["K%d_small" % K]
        assert (H, rows, T, len(starts), sc.fwd_ks(H)) == (4 * K, 36, 3, 17, K) and len(set(starts)) < 17
        S, H, rows, T, starts, _ = sc.INSTANCE_CASES["K%d_big" % K]
        assert (rows, T, len(starts), sc.fwd_ks(H)) == (272, 16, 257, K) and len(starts) * T == 4112 and sc.fwd_ks(H - 1 or 1) <= K
        assert K == 4 or sc.fwd_ks(H - 1) < K                                 # the first H of the bracket
        assert min(starts) == 0 and max(starts) == rows - T and len(set(starts)) < len(starts)


def test_two_planted_mistakes_move_the_irregular_case_a_hundred_bars():
    """Windows taken at starts[w] + 1, and windows taken at w * 1 in place of the table: each moves Y or a gradient by at
    least 1e-2 of its maximum, a hundred times the bar the GPU test holds."""
    from oracle import windgnn_oracle as orc
    r = sc.reference("irregular")
    A = r.A.double()
    for what, wrong in (("starts + 1", [s + 1 for s in r.starts]), ("w * 1", list(range(r.n)))):
        X = sc.windows_at(r.feat, r.T, wrong).double()             # (feat has three more rows than the series)
        Y, cache = orc.forward(A, X, r.p64)
        g = orc.backward(A, X, r.p64, Y, cache, r.dY.double())
        moved = {"Y": rel_to_max(Y, r.Yo)}
        moved.update({k: rel_to_max(g[k], r.go[k]) for k in PARAM_KEYS})
        print(what, "  ".join("%s %.2e" % kv for kv in moved.items()))
        assert max(moved.values()) >= 1e-2, (what, moved)
