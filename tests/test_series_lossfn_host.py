"""Host side of series training on a loss spec (no GPU): include/windgnn_series_lossfn.h against _lib.EXPORTS_SERIES_LOSSFN and
the exports of the shared object, every refusal of the pair before any launch (fake device pointers), the Python layer's
refusals, the defaults reaching exactly today's raw calls, and the qualification on the fp64 oracle alone of the cases
tests/test_gpu_series_lossfn.py runs: the reference losses against torch.nn.functional, both Huber arms populated, the warm-up
steps visible, the L1 residuals away from zero, and five planted mistakes a hundred bars high."""
import ctypes as C
import os
import re

import pytest
import torch

import series_at_cases as sc
import series_lossfn_cases as lc
from conftest import PARAM_KEYS, ROOT, rel_to_max
from test_abi_and_host import _c_kind, _ctype_kind
from test_optim_host import _prototypes
from test_series_at_host import ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED, ERR_WORKSPACE, _cpu_step, _lib, _sd


def test_lossfn_prototypes_match_the_header_argument_for_argument():
    L, lib = _lib()
    protos = _prototypes("windgnn_series_lossfn.h")
    assert set(protos) == set(L.EXPORTS_SERIES_LOSSFN) == {
        "wgnn_series_lossfn_version", "wgnn_series_lossfn_bytes", "wgnn_series_fwd_lossfn", "wgnn_series_bwd_lossfn"}
    for name, (ret, args) in protos.items():
        res, argtypes = L.EXPORTS_SERIES_LOSSFN[name]
        assert len(args) == len(argtypes), (name, args, argtypes)
        for i, (decl, t) in enumerate(zip(args, argtypes)):
            assert _c_kind(decl) == _ctype_kind(t), (name, i, decl, t)
        want = "ptr" if "*" in ret else {"int": "i32", "size_t": "size"}[ret.replace("const", "").strip()]
        assert _ctype_kind(res) == want, (name, ret, res)
        assert hasattr(lib, name) and getattr(lib, name).argtypes == argtypes, name
    # the pair is the masked pair with `const wgnn_lossfn* fn` behind ls_rows resp. grad_scale
    masked = _prototypes("windgnn_series_masked.h")
    f, b = protos["wgnn_series_fwd_lossfn"][1], protos["wgnn_series_bwd_lossfn"][1]
    assert f[7] == b[9] == "const wgnn_lossfn* fn"
    assert f[:7] + f[8:] == masked["wgnn_series_fwd_loss_masked"][1] and b[:9] + b[10:] == masked["wgnn_series_bwd_mse_masked"][1]
    # the struct, field for field
    hdr = open(os.path.join(ROOT, "include", "windgnn_series_lossfn.h")).read()
    assert "typedef struct { int32_t kind; float delta; int32_t t_from; int32_t masked; } wgnn_lossfn;" in hdr
    assert [(n, _ctype_kind(t)) for n, t in L.LossFn._fields_] == [("kind", "i32"), ("delta", "float"), ("t_from", "i32"),
                                                                     ("masked", "i32")] and C.sizeof(L.LossFn) == 16
    for name, v in (("MSE", 0), ("L1", 1), ("HUBER", 2)):
        assert re.search(r"#define\s+WGNN_LOSS_%s\s+%d\b" % (name, v), hdr) and getattr(L, "LOSS_" + name) == v
    assert L.LOSS_KINDS == {"mse": 0, "l1": 1, "huber": 2} == lc.KINDS
    assert re.search(r"#define\s+WGNN_SERIES_LOSSFN_VERSION\s+1\b", hdr) and '#include "windgnn_series_masked.h"' in hdr
    assert lib.wgnn_series_lossfn_version() == L.SERIES_LOSSFN_VERSION == 1
    # every other header and version is as it was
    assert lib.wgnn_version() == 122 and lib.wgnn_series_version() == 1 and lib.wgnn_series_train_version() == 1
    assert lib.wgnn_series_at_version() == 1 and lib.wgnn_series_masked_version() == 1 and lib.wgnn_eval_version() == L.EVAL_VERSION
    for other in ("windgnn.h", "windgnn_series.h", "windgnn_series_train.h", "windgnn_series_at.h", "windgnn_series_masked.h",
                  "windgnn_eval.h"):
        text = open(os.path.join(ROOT, "include", other)).read()
        assert "lossfn" not in text and "HUBER" not in text, other
    for other in (L.EXPORTS, L.EXPORTS_OPTIM, L.EXPORTS_SCHED, L.EXPORTS_EVAL, L.EXPORTS_BEST, L.EXPORTS_SERIES,
                  L.EXPORTS_SERIES_TRAIN, L.EXPORTS_SERIES_AT, L.EXPORTS_SERIES_MASKED):
        assert not set(other) & set(L.EXPORTS_SERIES_LOSSFN)
    from windgnn_amd import build
    assert any(h.endswith("windgnn_series_lossfn.h") for h in build.HEADERS)


def _pair(lib, L, sd, ws_bytes=1 << 40, null=None, ls_rows=14, grad_scale=1.0, starts=True, fn=(1, 0.0, 0, 0)):
    """Both entry points on non-NULL fake device pointers: (fwd_lossfn, bwd_lossfn) statuses.  Every call must be refused on the
    host: a launch on these pointers would fault."""
    def P(name, v):
        return C.c_void_p(0 if name == null else v)
    p = L.Params(*([4096] * 8), None)
    g = L.Grads(*([4096] * 8))
    if null == "p.w_hh":
        p.w_hh = None
    if null == "grads.b_ih":
        g.b_ih = None
    spec = L.LossFn(*fn)
    fnp = C.byref(spec) if null != "fn" else None
    sdp = C.byref(sd) if null != "sd" else None
    head = (sdp, P("A", 8192), P("Xs", 1 << 20), P("starts", 1 << 21 if starts else 0), C.byref(p) if null != "p" else None)
    tail = (P("ws", 1 << 40), ws_bytes, None)
    return (lib.wgnn_series_fwd_lossfn(*head, P("Ls", 1 << 22), ls_rows, fnp, P("Y", 1 << 24), P("stash", 1 << 28),
                                       P("loss_buf", 1 << 30), *tail),
            lib.wgnn_series_bwd_lossfn(*head, P("Y", 1 << 24), P("Ls", 1 << 22), ls_rows, grad_scale, fnp, P("stash", 1 << 28),
                                       P("loss_buf", 1 << 30), P("loss", 1 << 32), C.byref(g) if null != "grads" else None,
                                       *tail))


def test_every_refusal_of_the_lossfn_pair_comes_before_any_launch():
    L, lib = _lib()
    for stride, starts in ((0, True), (1, False)):                # the table form and the strided form
        sd = _sd(L, stride=stride, n=4)
        kw = {"starts": starts}
        names = ["sd", "A", "Xs", "p", "p.w_hh", "ws", "Y", "Ls", "loss_buf", "fn"] + (["starts"] if starts else [])
        for name in names:
            assert _pair(lib, L, sd, null=name, **kw) == (ERR_NULL,) * 2, (stride, name)
        for name in ("grads", "grads.b_ih", "loss", "stash"):        # (the forward's stash is optional, the backward's is not)
            assert _pair(lib, L, sd, null=name, **kw)[1] == ERR_NULL, (stride, name)
        for bad in (_sd(L, stride=stride, T=15), _sd(L, stride=stride, n=0), _sd(L, stride=stride, T=0),
                    _sd(L, stride=stride, rows=0), _sd(L, stride=stride, F=12), _sd(L, stride=stride, S=0),
                    _sd(L, stride=stride, H=0)):
            assert _pair(lib, L, bad, ls_rows=1 << 24, **kw) == (ERR_SHAPE,) * 2, bytes(bad)
            assert lib.wgnn_series_lossfn_bytes(C.byref(bad)) == 0
        for bad in (_sd(L, stride=stride, math=1), _sd(L, stride=stride, adj=1, nnz=20), _sd(L, stride=stride, H=129),
                    _sd(L, stride=stride, S=65), _sd(L, stride=stride, io=1)):
            assert _pair(lib, L, bad, **kw) == (ERR_UNSUPPORTED,) * 2, bytes(bad)
            assert lib.wgnn_series_lossfn_bytes(C.byref(bad)) == 0
        short = 13 if stride == 0 else (4 - 1) * stride + 5 - 1                 # one label row too few
        assert _pair(lib, L, sd, ls_rows=short, **kw) == (ERR_SHAPE,) * 2
        assert _pair(lib, L, sd, ls_rows=-(-(1 << 31) // 21), **kw) == (ERR_SHAPE,) * 2
        for bad in (0.0, -1.0, float("inf"), float("nan")):
            assert _pair(lib, L, sd, grad_scale=bad, **kw)[1] == ERR_SHAPE, bad
        q = "wgnn_series_at_workspace_bytes" if stride == 0 else "wgnn_series_workspace_bytes"
        need = getattr(lib, q)(C.byref(sd))
        assert need > 0 and _pair(lib, L, sd, ws_bytes=need - 1, **kw) == (ERR_WORKSPACE,) * 2
        # the spec, each bad field on its own (T = 5): kind, masked, t_from, and Huber's delta
        for fn in ((-1, 0.0, 0, 0), (3, 0.0, 0, 0), (0, 0.0, 0, 2), (1, 0.0, 0, -1), (1, 0.0, -1, 0), (1, 0.0, 5, 0), (0, 0.0, 5, 1),
                   (2, 0.0, 0, 0), (2, -0.25, 0, 1), (2, float("inf"), 0, 0), (2, float("nan"), 2, 0)):
            assert _pair(lib, L, sd, fn=fn, **kw) == (ERR_SHAPE,) * 2, (stride, fn)
        # ... which comes last: a short workspace, a short label series and a NULL are reported first
        assert _pair(lib, L, sd, fn=(3, 0.0, 0, 0), ws_bytes=need - 1, **kw) == (ERR_WORKSPACE,) * 2
        assert _pair(lib, L, sd, fn=(3, 0.0, 0, 0), ls_rows=short, **kw) == (ERR_SHAPE,) * 2
        assert _pair(lib, L, sd, fn=(3, 0.0, 0, 0), null="Ls", **kw) == (ERR_NULL,) * 2
        # the loss buffer is the masked one: the counts are always there
        for n in ((1, 4, 16, 17, 40) if stride == 0 else (1, 4, 10)):
            d = _sd(L, stride=stride, n=n)
            assert lib.wgnn_series_lossfn_bytes(C.byref(d)) == lib.wgnn_series_masked_loss_bytes(C.byref(d)) == 4 * (3 * -(-n // 16) + 4)
    # the two forms do not mix
    assert _pair(lib, L, _sd(L, stride=1, n=4), starts=True) == (ERR_SHAPE,) * 2
    assert _pair(lib, L, _sd(L, stride=0, n=4), starts=False) == (ERR_NULL,) * 2
    assert _pair(lib, L, _sd(L, stride=-1, n=4), starts=False) == (ERR_SHAPE,) * 2
    assert lib.wgnn_series_lossfn_bytes(None) == 0


def test_a_valid_spec_on_fake_pointers_is_what_the_refusals_above_are_not():
    """The spec checks do refuse for their own reason: with delta ignored for MSE and L1, the same fake-pointer calls with a short
    workspace get as far as the workspace check for every valid spec (and never to a launch)."""
    L, lib = _lib()
    sd = _sd(L, stride=1, n=4)
    need = lib.wgnn_series_workspace_bytes(C.byref(sd))
    for fn in ((0, float("nan"), 0, 0), (1, -1.0, 4, 1), (2, 0.25, 2, 0), (2, 1e30, 0, 1)):
        assert _pair(lib, L, sd, fn=fn, starts=False, ws_bytes=need - 1) == (ERR_WORKSPACE,) * 2, fn


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
def test_the_python_layer_refuses_by_the_arguments_name_before_any_launch():
    from windgnn_amd.series import loss_spec, series_forward_loss_raw
    A, series, Ls = torch.rand(7, 7), torch.rand(14, 7, 13), torch.rand(14, 21)
    params = [torch.zeros(1)] * 8
    with pytest.raises(ValueError, match=r"loss='mae'.*'mse', 'l1' or 'huber'"):
        series_forward_loss_raw(A, series, Ls, 5, 1, params, loss="mae")
    for call in ("step_series", "forward_backward_series"):
        for kw in ({"stride": 3, "n_windows": 4}, {"starts": [0, 3, 3, 9]}):
            def go(tr=None, **more):
                return getattr(tr or _cpu_step(), call)(A, series, Ls, 5, **kw, **more)
            with pytest.raises(ValueError, match=r"TrainStep\.%s: loss='smooth_l1'.*'mse', 'l1' or 'huber'" % call):
                go(loss="smooth_l1")
            for bad in (-1, 5, 6, 2.5):
                with pytest.raises(ValueError, match=r"loss_from=.*\[0, seq_len = 5\)"):
                    go(loss_from=bad)
            for bad in (0.0, -0.25, float("inf"), float("nan")):
                with pytest.raises(ValueError, match=r"huber_delta=.*finite and > 0"):
                    go(loss="huber", huber_delta=bad)
            go_on = r"MI355X|no CPU fallback"                    # in scope: the device is asked for next
            with pytest.raises(RuntimeError, match=go_on):
                go(loss="l1", huber_delta=-1.0)                  # delta belongs to Huber alone
            with pytest.raises(RuntimeError, match=go_on):
                go(loss="huber", huber_delta=0.25, loss_from=4, missing_labels=True)
            # everything step_series refuses already is still refused
            with pytest.raises(RuntimeError, match=r"carry_state=True.*make_windows"):
                go(_cpu_step(carry_state=True), loss="l1")
            with pytest.raises(RuntimeError, match=r"math != 'f32'"):
                go(_cpu_step(math="f16x3"), loss="huber", loss_from=2)
            # under a process group: the new losses are in scope, missing labels stay refused for today's reason
            tr = _cpu_step()
            tr.collective = True                                   # (a process group cannot be had here: this is what it sets)
            with pytest.raises(RuntimeError, match=r"missing_labels=True under a process group.*label counts.*exchanged"):
                go(tr, loss="l1", missing_labels=True)
            if call == "forward_backward_series":                  # (step_series would ask the absent group for its weight)
                with pytest.raises(RuntimeError, match=go_on):
                    go(tr, loss="l1", loss_from=2)
            assert tr.steps == 0
    assert loss_spec("mse", float("nan"), 0, 5) is None and loss_spec("mse", 1.0, 0, 1, True) is None
    s = loss_spec("huber", 0.25, 3, 5, True)
    assert (s.kind, s.delta, s.t_from, s.masked) == (2, 0.25, 3, 1)
    s = loss_spec("l1", 7.0, 0, 5)
    assert (s.kind, s.delta, s.t_from, s.masked) == (1, 0.0, 0, 0)
    s = loss_spec("mse", 7.0, 4, 5)
    assert (s.kind, s.delta, s.t_from, s.masked) == (0, 0.0, 4, 0)


@pytest.mark.parametrize("spec", [{}, {"loss": "mse", "huber_delta": 3.0, "loss_from": 0}, {"loss": "l1"},
                                  {"loss": "huber", "huber_delta": 0.25, "loss_from": 2}, {"loss_from": 4}])
def test_the_defaults_reach_exactly_todays_raw_calls_and_a_spec_adds_its_three_keywords(monkeypatch, spec):
    """Defaults (spelled out or not): the raw wrappers are called with the arguments they had before the keywords existed (the
    recorders of tests/test_trainstep_schedule_host.py have those signatures and would raise on one more).  A spec: the same two
    calls with loss / huber_delta / loss_from and nothing else."""
    import test_trainstep_schedule_host as ts
    from windgnn_amd import trainer
    rec = ts.Recorder()
    for name, fn in ts._bindings(rec, 21).items():
        monkeypatch.setattr(trainer, name, fn)
    default = spec.get("loss", "mse") == "mse" and spec.get("loss_from", 0) == 0
    seen = []
    if not default:
        strict_f, strict_b = trainer.series_forward_loss_raw, trainer.series_backward_mse_raw

        def fwd(*a, loss, huber_delta, loss_from, **kw):
            seen.append(("fwd", loss, huber_delta, loss_from))
            return strict_f(*a, **kw)

        def bwd(*a, loss_kind, huber_delta, loss_from, **kw):
            seen.append(("bwd", loss_kind, huber_delta, loss_from))
            return strict_b(*a, **kw)
        monkeypatch.setattr(trainer, "series_forward_loss_raw", fwd)
        monkeypatch.setattr(trainer, "series_backward_mse_raw", bwd)
    tr = _cpu_step(check_every=1)
    loss, Y = tr.step_series(torch.rand(7, 7), torch.rand(14, 7, 13), torch.rand(14, 21), 5, 3, n_windows=4, **spec)
    assert tuple(Y.shape) == (4, 5, 21) and tr.steps == 1
    assert rec.events == [("require_gpu",), ("images",), ("series_forward_loss", 4), ("series_bwd_mse", 1.0), ("finish", 0, 1)]
    want = (spec.get("loss", "mse"), float(spec.get("huber_delta", 1.0)), spec.get("loss_from", 0))
    assert seen == ([] if default else [("fwd",) + want, ("bwd",) + want])
    tr.forward_backward_series(torch.rand(7, 7), torch.rand(14, 7, 13), torch.rand(14, 21), 5, 3, n_windows=4, **spec)
    assert rec.events[-2:] == [("series_forward_loss", 4), ("series_bwd_mse", 1.0)] and tr.steps == 1


# ---- qualification of the cases on the oracle alone ---------------------------------------------------------------------------
HOST_CASES = list(lc.PARITY)            # every case the GPU test runs is qualified here


def test_the_case_list_is_what_the_issue_asks_for():
    assert HOST_CASES == list(lc.PARITY) and len(lc.PARITY) == 24 + 3 + 18 and len(lc.INSTANCES) == 18
    fwd, bwd = set(), set()
    for cid in lc.INSTANCES:
        base, how, mask, kind, delta, t_from = lc.PARITY[cid]
        H = sc.case(base)[1]
        tag = ",starts,lossfn" if how == "table" else ",lossfn"
        fwd.add("gru_fwd_kernel<%d%s>" % (sc.fwd_ks(H), tag))
        bwd.add("gru_bwd_kernel<%d%s>" % (sc.bwd_ks3(H), tag))
        assert t_from == (1 if base.endswith("small") else 8) and lc.mapping(base, how)[1] == (None if how == "table" else
                                                                                                int(how[-1]))
    assert len(fwd) == 18 and len(bwd) == 18                     # 9 K x 2 row mappings each: all 36 new instances
    assert {lc.PARITY[c][3] for c in lc.INSTANCES} == {"mse", "l1", "huber"}
    assert lc.mapping("K12_small", "stride2") == ([2 * w for w in range(17)], 2)
    assert lc.mapping("K12_big", "stride1") == (list(range(257)), 1)


@pytest.mark.parametrize("cid", HOST_CASES)
def test_a_case_qualifies_on_the_oracle_alone(cid):
    import torch.nn.functional as F
    q = lc.reference(*lc.PARITY[cid])
    if not q.base.endswith("_big"):
        assert q.margin > 1e-5, (cid, q.margin)                  # (the big shapes' margins: tests/test_series_at_host.py)
    on = lc.counted(q.L, q.t_from, q.masked)
    assert q.m == int(on.sum()) == sum(q.counts) and 0 < q.m
    assert q.m == q.n * (q.T - q.t_from) * q.H if not q.masked else q.m <= q.n * (q.T - q.t_from) * q.H
    assert (q.masked == 1) == bool(torch.isnan(q.L).any()) or q.mask == "e"
    # the reference loss is torch's own on the gathered entries of M
    y, l = q.Yo[on], q.L.double()[on]
    want = {"mse": lambda: F.mse_loss(y, l), "l1": lambda: F.l1_loss(y, l),
            "huber": lambda: F.huber_loss(y, l, delta=q.delta)}[q.kind]()
    assert abs(q.loss_o - float(want)) <= 1e-12 * float(want), (cid, q.loss_o, float(want))
    assert torch.isfinite(torch.tensor(q.loss_o)) and q.loss_o < 4.0                 # no SPARE row, no NaN entered the loss
    assert not torch.isnan(q.Yo).any() and all(torch.isfinite(g).all() for g in q.gm.values()), cid
    assert (q.dY[~on] == 0).all() and bool((q.dY[on] != 0).all())
    r = (y - l).abs()
    if q.kind == "l1":
        assert float(r.min()) >= 1e-3, (cid, float(r.min()))      # the sign of no residual hangs on rounding (here: |r| > 1)
        assert float(r.min()) > 1.0
    if q.kind in ("l1", "huber"):
        assert bool((q.dY > 0).any()) and bool((q.dY < 0).any()), cid        # both signs of dY
    if q.kind == "huber":
        quad = float((r <= q.delta).double().mean())
        print(cid, "quadratic arm %.3f of M" % quad)
        assert 0.10 <= quad <= 0.90, (cid, quad)                  # both arms hold at least a tenth of M
    if q.t_from > 0:
        early = (q.Yo[:, :q.t_from] - q.L.double()[:, :q.t_from]).abs()
        early = early[~torch.isnan(early)]
        assert early.numel() and float(early.max()) > 0.1, cid    # a label the skip must skip


def test_with_mse_from_step_0_the_reference_is_the_masked_suites_and_the_oracles():
    import series_masked_cases as mc
    from oracle import windgnn_oracle as orc
    for how, mask in (("table", "e"), ("stride2", "b")):
        q, want = lc.reference("irregular", how, mask, "mse", 0.0, 0), mc.reference("irregular", how, mask)
        assert q.m == want.m and q.counts == want.counts and torch.equal(q.Ls.isnan(), want.Ls.isnan())
        assert abs(q.loss_o - want.loss_o) <= 1e-15 and all(rel_to_max(q.gm[k], want.gm[k]) <= 1e-14 for k in PARAM_KEYS)
    e = lc.reference("irregular", "table", "e", "mse", 0.0, 0)
    _, loss, g = orc.train_step(e.A.double(), e.X.double(), e.L.double(), e.p64)
    assert abs(float(loss) - e.loss_o) <= 1e-15 and all(rel_to_max(e.gm[k], g[k]) <= 1e-14 for k in PARAM_KEYS)


@pytest.mark.parametrize("how", ["table", "stride2"])
def test_five_planted_mistakes_move_a_case_a_hundred_bars(how):
    """Each planted mistake moves the loss or some gradient by at least 1e-2 of its maximum, a hundred times the bar the GPU test
    holds, on every irregular case it can show on."""
    shown = {what: 0 for what in lc.PLANTED}
    for cid, case in lc.PARITY.items():
        if case[0] != "irregular" or case[1] != how:
            continue
        q = lc.reference(*case)
        for what, applies in lc.PLANTED.items():
            if not applies(q):
                continue
            loss, g = lc.planted(q, what)
            moved = {"loss": abs(loss - q.loss_o) / q.loss_o}
            moved.update({k: rel_to_max(g[k], q.gm[k]) for k in PARAM_KEYS})
            print(cid, what, "  ".join("%s %.2e" % kv for kv in moved.items()))
            if what == "linear arm without its constant":
                assert moved["loss"] >= 1e-2, (cid, what, moved)          # visible in the loss alone
                assert max(v for k, v in moved.items() if k != "loss") <= 1e-14
            else:
                assert max(moved.values()) >= 1e-2, (cid, what, moved)
            shown[what] += 1
    assert all(n >= 2 for n in shown.values()), shown
