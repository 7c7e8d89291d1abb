"""Host side of series training through missing labels (no GPU): include/windgnn_series_masked.h against
_lib.EXPORTS_SERIES_MASKED and the exports of the shared object, every refusal of the three entry points before any launch (fake
device pointers), the Python layer's refusals, missing_labels=False reaching exactly today's raw calls, and the qualification on
the fp64 oracle alone of the cases tests/test_gpu_series_masked.py runs (ReLU margins, the masks, three planted mistakes)."""
import ctypes as C
import os
import re

import pytest
import torch

import series_at_cases as sc
import series_masked_cases as mc
from conftest import PARAM_KEYS, ROOT, rel_to_max
from test_abi_and_host import _c_kind, _ctype_kind
from test_optim_host import _prototypes
from test_series_at_host import ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED, ERR_WORKSPACE, _cpu_step, _lib, _sd


def test_masked_prototypes_match_the_header_argument_for_argument():
    L, lib = _lib()
    protos = _prototypes("windgnn_series_masked.h")
    assert set(protos) == set(L.EXPORTS_SERIES_MASKED) == {
        "wgnn_series_masked_version", "wgnn_series_masked_loss_bytes", "wgnn_series_fwd_loss_masked",
        "wgnn_series_bwd_mse_masked", "wgnn_eval_accum_series"}
    for name, (ret, args) in protos.items():
        res, argtypes = L.EXPORTS_SERIES_MASKED[name]
        assert len(args) == len(argtypes), (name, args, argtypes)
        for i, (decl, t) in enumerate(zip(args, argtypes)):
            assert _c_kind(decl) == _ctype_kind(t), (name, i, decl, t)
        want = "ptr" if "*" in ret else {"int": "i32", "size_t": "size"}[ret.replace("const", "").strip()]
        assert _ctype_kind(res) == want, (name, ret, res)
        assert hasattr(lib, name) and getattr(lib, name).argtypes == argtypes, name
    # the pair is the table pair, argument for argument: one signature serves both row mappings
    at = _prototypes("windgnn_series_at.h")
    assert protos["wgnn_series_fwd_loss_masked"] == at["wgnn_series_fwd_loss_at"]
    assert protos["wgnn_series_bwd_mse_masked"] == at["wgnn_series_bwd_mse_at"]
    assert lib.wgnn_series_masked_version() == L.SERIES_MASKED_VERSION == 1
    # the existing headers and their versions are as they were
    assert lib.wgnn_version() == 122 and lib.wgnn_series_version() == 1 and lib.wgnn_series_train_version() == 1
    assert lib.wgnn_series_at_version() == 1 and lib.wgnn_eval_version() == L.EVAL_VERSION
    hdr = open(os.path.join(ROOT, "include", "windgnn_series_masked.h")).read()
    assert re.search(r"#define\s+WGNN_SERIES_MASKED_VERSION\s+1\b", hdr) and re.search(r"#define\s+WGNN_STATUS_NO_LABELS\s+32u", hdr)
    assert '#include "windgnn_series_at.h"' in hdr and L.STATUS_NO_LABELS == 32
    for other in ("windgnn.h", "windgnn_series.h", "windgnn_series_train.h", "windgnn_series_at.h", "windgnn_eval.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert "masked" not in text and "NO_LABELS" not in text and "eval_accum_series" not in text, other
    for other in (L.EXPORTS, L.EXPORTS_OPTIM, L.EXPORTS_SCHED, L.EXPORTS_EVAL, L.EXPORTS_BEST, L.EXPORTS_SERIES,
                  L.EXPORTS_SERIES_TRAIN, L.EXPORTS_SERIES_AT):
        assert not set(other) & set(L.EXPORTS_SERIES_MASKED)
    from windgnn_amd import build
    assert any(h.endswith("windgnn_series_masked.h") for h in build.HEADERS)


def _pair(lib, L, sd, ws_bytes=1 << 40, null=None, ls_rows=14, grad_scale=1.0, starts=True):
    """Both masked entry points on non-NULL fake device pointers: (fwd_loss_masked, bwd_mse_masked) statuses.  Every call must
    be refused on the host: a launch on these pointers would fault."""
    def P(name, v):
        return C.c_void_p(0 if name == null else v)
    p = L.Params(*([4096] * 8), None)
    g = L.Grads(*([4096] * 8))
    if null == "p.w_hh":
        p.w_hh = None
    if null == "grads.b_ih":
        g.b_ih = None
    sdp = C.byref(sd) if null != "sd" else None
    head = (sdp, P("A", 8192), P("Xs", 1 << 20), P("starts", 1 << 21 if starts else 0), C.byref(p) if null != "p" else None)
    tail = (P("ws", 1 << 40), ws_bytes, None)
    return (lib.wgnn_series_fwd_loss_masked(*head, P("Ls", 1 << 22), ls_rows, P("Y", 1 << 24), P("stash", 1 << 28),
                                            P("loss_buf", 1 << 30), *tail),
            lib.wgnn_series_bwd_mse_masked(*head, P("Y", 1 << 24), P("Ls", 1 << 22), ls_rows, grad_scale, P("stash", 1 << 28),
                                           P("loss_buf", 1 << 30), P("loss", 1 << 32), C.byref(g) if null != "grads" else None,
                                           *tail))


def test_every_refusal_of_the_masked_pair_comes_before_any_launch():
    L, lib = _lib()
    for stride, starts in ((0, True), (1, False)):                # the table form and the strided form
        sd = _sd(L, stride=stride, n=4)
        kw = {"starts": starts}
        names = ["sd", "A", "Xs", "p", "p.w_hh", "ws", "Y", "Ls", "loss_buf"] + (["starts"] if starts else [])
        for name in names:
            assert _pair(lib, L, sd, null=name, **kw) == (ERR_NULL,) * 2, (stride, name)
        for name in ("grads", "grads.b_ih", "loss"):
            assert _pair(lib, L, sd, null=name, **kw)[1] == ERR_NULL, (stride, name)
        for bad in (_sd(L, stride=stride, T=15), _sd(L, stride=stride, n=0), _sd(L, stride=stride, T=0),
                    _sd(L, stride=stride, rows=0), _sd(L, stride=stride, F=12), _sd(L, stride=stride, S=0),
                    _sd(L, stride=stride, H=0)):
            assert _pair(lib, L, bad, ls_rows=1 << 24, **kw) == (ERR_SHAPE,) * 2, bytes(bad)
            assert lib.wgnn_series_masked_loss_bytes(C.byref(bad)) == 0
        for bad in (_sd(L, stride=stride, math=1), _sd(L, stride=stride, adj=1, nnz=20), _sd(L, stride=stride, H=129),
                    _sd(L, stride=stride, S=65), _sd(L, stride=stride, io=1)):
            assert _pair(lib, L, bad, **kw) == (ERR_UNSUPPORTED,) * 2, bytes(bad)
            assert lib.wgnn_series_masked_loss_bytes(C.byref(bad)) == 0
        short = 13 if stride == 0 else (4 - 1) * stride + 5 - 1                 # one label row too few
        assert _pair(lib, L, sd, ls_rows=short, **kw) == (ERR_SHAPE,) * 2
        assert _pair(lib, L, sd, ls_rows=-(-(1 << 31) // 21), **kw) == (ERR_SHAPE,) * 2
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert _pair(lib, L, sd, grad_scale=bad, **kw)[1] == ERR_SHAPE, bad
        q = "wgnn_series_at_workspace_bytes" if stride == 0 else "wgnn_series_workspace_bytes"
        need = getattr(lib, q)(C.byref(sd))
        assert need > 0 and _pair(lib, L, sd, ws_bytes=need - 1, **kw) == (ERR_WORKSPACE,) * 2
        # today's loss buffer plus one integer count per workgroup of 16 windows
        for n in ((1, 4, 16, 17, 40) if stride == 0 else (1, 4, 10)):     # (10 windows at stride 1 fill the 14 rows)
            d = _sd(L, stride=stride, n=n)
            plain = (lib.wgnn_series_at_loss_bytes if stride == 0 else lib.wgnn_series_loss_bytes)(C.byref(d))
            assert lib.wgnn_series_masked_loss_bytes(C.byref(d)) == plain + 4 * -(-n // 16) == 4 * (3 * -(-n // 16) + 4), n
    # the two forms do not mix: a stride with a table is a shape error, a table's dims without a table a NULL
    assert _pair(lib, L, _sd(L, stride=1, n=4), starts=True) == (ERR_SHAPE,) * 2
    assert _pair(lib, L, _sd(L, stride=0, n=4), starts=False) == (ERR_NULL,) * 2
    assert _pair(lib, L, _sd(L, stride=-1, n=4), starts=False) == (ERR_SHAPE,) * 2
    assert lib.wgnn_series_masked_loss_bytes(None) == 0


def test_every_refusal_of_eval_accum_series_comes_before_any_launch():
    L, lib = _lib()

    def go(pred=1 << 20, Ls=1 << 22, ls_rows=40, starts=0, stride=1, B=8, T=5, H=21, skip=1, acc=1 << 24):
        return lib.wgnn_eval_accum_series(C.c_void_p(pred), C.c_void_p(Ls), ls_rows, C.c_void_p(starts), stride, B, T, H, 0.0, 1.0,
                                          skip, C.c_void_p(acc), None, None)
    for null in ("pred", "Ls", "acc"):
        assert go(**{null: 0}) == ERR_NULL, null
    assert go(stride=0) == ERR_NULL                                   # a table's call without the table
    for bad in (dict(B=0), dict(T=0), dict(H=0), dict(stride=-1), dict(stride=1, starts=1 << 21),
                dict(ls_rows=4), dict(ls_rows=7 * 1 + 5 - 1), dict(stride=2, ls_rows=7 * 2 + 5 - 1),
                dict(stride=0, starts=1 << 21, ls_rows=4), dict(ls_rows=-(-(1 << 31) // 21))):
        assert go(**bad) == ERR_SHAPE, bad


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def test_missing_labels_is_refused_under_a_process_group_with_the_reason_and_the_alternative():
    A, series, Ls = torch.rand(7, 7), torch.rand(14, 7, 13), torch.rand(14, 21)
    for call in ("step_series", "forward_backward_series"):
        for kw in ({"stride": 3, "n_windows": 4}, {"starts": [0, 3, 3, 9]}):
            tr = _cpu_step()
            tr.collective = True                       # (a process group cannot be had here: this is what it sets)
            with pytest.raises(RuntimeError, match=r"missing_labels=True under a process group.*label counts.*exchanged.*"
                                                   r"out of scope.*segment_starts"):
                getattr(tr, call)(A, series, Ls, 5, missing_labels=True, **kw)
            assert tr.steps == 0
            # everything step_series refuses already is still refused, with the flag
            with pytest.raises(RuntimeError, match=r"carry_state=True.*make_windows"):
                getattr(_cpu_step(carry_state=True), call)(A, series, Ls, 5, missing_labels=True, **kw)
            with pytest.raises(RuntimeError, match=r"math != 'f32'"):
                getattr(_cpu_step(math="f16x3"), call)(A, series, Ls, 5, missing_labels=True, **kw)
            with pytest.raises(RuntimeError, match=r"MI355X|no CPU fallback"):        # in scope: the device is asked for next
                getattr(_cpu_step(), call)(A, series, Ls, 5, missing_labels=True, **kw)


@pytest.mark.parametrize("flag", [False, True])
def test_the_default_reaches_exactly_todays_raw_calls(monkeypatch, flag):
    """missing_labels=False: the raw wrappers are called with the arguments they had before the keyword existed (the recorders
    of tests/test_trainstep_schedule_host.py have those signatures and would raise on one more); True: the same two calls with
    missing_labels=True and nothing else."""
    import test_trainstep_schedule_host as ts
    from windgnn_amd import trainer
    rec = ts.Recorder()
    for name, fn in ts._bindings(rec, 21).items():
        monkeypatch.setattr(trainer, name, fn)
    seen = []
    if flag:
        strict_f, strict_b = trainer.series_forward_loss_raw, trainer.series_backward_mse_raw

        def fwd(*a, missing_labels, **kw):
            seen.append(("fwd", missing_labels))
            return strict_f(*a, **kw)

        def bwd(*a, missing_labels, **kw):
            seen.append(("bwd", missing_labels))
            return strict_b(*a, **kw)
        monkeypatch.setattr(trainer, "series_forward_loss_raw", fwd)
        monkeypatch.setattr(trainer, "series_backward_mse_raw", bwd)
    tr = _cpu_step(check_every=1)
    kw = {"missing_labels": True} if flag else {}
    loss, Y = tr.step_series(torch.rand(7, 7), torch.rand(14, 7, 13), torch.rand(14, 21), 5, 3, n_windows=4, **kw)
    assert tuple(Y.shape) == (4, 5, 21) and tr.steps == 1
    assert rec.events == [("require_gpu",), ("images",), ("series_forward_loss", 4), ("series_bwd_mse", 1.0), ("finish", 0, 1)]
    assert seen == ([("fwd", True), ("bwd", True)] if flag else [])
    tr.forward_backward_series(torch.rand(7, 7), torch.rand(14, 7, 13), torch.rand(14, 21), 5, 3, n_windows=4, **kw)
    assert rec.events[-2:] == [("series_forward_loss", 4), ("series_bwd_mse", 1.0)] and tr.steps == 1


def test_update_series_and_the_raw_wrapper_refuse_on_the_host():
    import windgnn_amd
    from windgnn_amd.evaluate import Evaluator, eval_accum_series
    model = windgnn_amd.GCN_GRU(13, 13, 13, 7 * 13, 21)
    ev = Evaluator(model, torch.rand(7, 7), 0.0, 1.0)
    series, Ls = torch.rand(14, 7, 13), torch.rand(14, 21)
    with pytest.raises(ValueError, match=r"stride= or starts=, not both"):
        ev.update_series(series, Ls, 5, stride=1, starts=[0, 1])
    with pytest.raises(ValueError, match=r"n_windows= belongs to stride="):
        ev.update_series(series, Ls, 5, n_windows=2, starts=[0, 1])
    with pytest.raises(ValueError, match=r"starts\[1\] = 10"):
        ev.update_series(series, Ls, 5, starts=[0, 10])
    with pytest.raises(RuntimeError, match=r"MI355X|no CPU fallback"):
        ev.update_series(series, Ls, 5, skip_missing=True)
    with pytest.raises(RuntimeError, match=r"MI355X|no CPU fallback"):
        eval_accum_series(torch.rand(4, 21), Ls, 5, 0.0, 1.0, torch.zeros(8, dtype=torch.float64))


# ---- qualification of the cases on the oracle alone ---------------------------------------------------------------------------
def test_every_case_keeps_its_relu_margin_and_its_masks_are_what_the_issue_describes():
    for cid, (base, how, mask) in mc.PARITY.items():
        if base.endswith("_big"):
            continue                                             # (their margins: tests/test_series_at_host.py; masks below)
        q = mc.reference(base, how, mask)
        assert q.margin > 1e-5, (cid, q.margin)
        assert 0 < q.m < q.n * q.T * q.H and q.m == sum(q.counts), cid
        assert torch.isfinite(torch.tensor(q.loss_o)) and q.loss_o < 1.0, cid          # no SPARE row entered the loss
        assert not torch.isnan(q.Yo).any() and all(torch.isfinite(g).all() for g in q.gm.values()), cid
    for how in ("table",) + tuple(mc.STRIDED):
        S, T, H = 7, 5, 21
        a = mc.reference("irregular", how, "a")
        cols = torch.nonzero(a.hit.any(dim=0)).flatten().tolist()
        assert cols == [S // 2, S + S // 2, 2 * S + S // 2]                            # one station, its three horizons
        first = [int(torch.nonzero(a.hit[:, c])[0]) for c in cols]
        assert first[0] - first[1] == first[1] - first[2] == 1                          # ... at the shifted rows
        b = mc.reference("irregular", how, "b")
        assert 0.05 < float(b.hit.float().mean()) < 0.15
        c = mc.reference("irregular", how, "c")
        assert c.counts[0] == 0 and all(x > 0 for x in c.counts[1:]) and len(c.counts) == 2   # one whole workgroup without labels
        d = mc.reference("irregular", how, "d")
        miss = torch.isnan(d.L).all(dim=2)                                               # [n, T]: rows of a window without labels
        assert miss[:, -1].sum() >= 6 and miss[1::3, -1].all()
        e = mc.reference("irregular", how, "e")
        assert e.m == e.n * T * H and not e.hit.any()
        f = mc.reference("irregular", how, "f")
        assert f.m == 0 and f.counts == [0, 0] and all(float(g.abs().max()) == 0 for g in f.gm.values())
    # with no NaN the masked reference IS the oracle's training step on the same labels
    from oracle import windgnn_oracle as orc
    e = mc.reference("irregular", "table", "e")
    _, loss, g = orc.train_step(e.A.double(), e.X.double(), e.L.double(), e.p64)
    assert abs(float(loss) - e.loss_o) <= 1e-15 and all(rel_to_max(e.gm[k], g[k]) <= 1e-14 for k in PARAM_KEYS)
    assert mc.mapping("irregular", "stride2") == ([2 * w for w in range(18)], 2)
    assert len(mc.PARITY) == 4 + 8 + 1 + 9 + 9
    for K in sc.FWD_KS:
        assert mc.PARITY["K%d_small-table-b" % K][0] in sc.INSTANCE_CASES and mc.PARITY["K%d_big-table-b" % K][0] in sc.INSTANCE_CASES


@pytest.mark.parametrize("how", ["table", "stride1", "stride2"])
def test_three_planted_mistakes_move_masks_a_to_d_a_hundred_bars(how):
    """Dividing by n T H instead of m, reading a missing label as 0, and masking the loss but not dY: each moves the loss or a
    gradient by at least 1e-2 of its maximum, a hundred times the bar the GPU test holds."""
    for mask in "abcd":
        q = mc.reference("irregular", how, mask)
        for what, (loss, g) in mc.planted(q).items():
            moved = {"loss": abs(loss - q.loss_o) / q.loss_o}
            moved.update({k: rel_to_max(g[k], q.gm[k]) for k in PARAM_KEYS})
            print(how, mask, what, "  ".join("%s %.2e" % kv for kv in moved.items()))
            assert max(moved.values()) >= 1e-2, (how, mask, what, moved)
