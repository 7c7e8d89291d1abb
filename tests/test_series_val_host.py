"""Host side of series validation (no GPU): include/windgnn_series_val.h against _lib.EXPORTS_SERIES_VAL and the exports of the
shared object, the record's public words against _lib.VAL_WORDS, every refusal of the entry points before any launch (fake device
pointers), the Python layer's refusals and launch order on recorder stubs, the best_on option, state_dict()'s keys, and the
qualification on the fp64 oracle alone of the cases tests/test_gpu_series_val.py runs.

Two planted mistakes.  (1) a loss taken at the last step only, (2) a mean over n T H although loss_from > 0.  Each must move the
oracle's loss by at least 1e-2 of itself on inputs the GPU test uses.  (2) does on every case with t_from > 0 (the factor is
(T - t_from) / T at most).  (1) does on every MSE and Huber case of the irregular shape with t_from < T - 1, and on the real
widths' MSE case over every step: the state starts from zero, so the early steps' residuals differ from the last step's.  It
is NOT claimed where the inputs cannot show it: the L1 cases move every label at least 1 away from Y so that no sign hangs on
rounding, which makes the loss about 2.3 at every step, and a loss from step 12 of 24 on the real widths averages over a state
that has settled.  Those cases are held by the bit-identity with the training pair instead, whose loss tests/
test_gpu_series_lossfn.py holds against the oracle at exactly these specs."""
import ctypes as C
import os
import re

import pytest
import torch

import series_val_cases as vc
from conftest import ROOT
from test_abi_and_host import _c_kind, _ctype_kind
from test_optim_host import _prototypes
from test_series_at_host import ERR_NULL, ERR_SHAPE, ERR_UNSUPPORTED, ERR_WORKSPACE, _cpu_step, _lib, _sd

NAMES = {"wgnn_series_val_version", "wgnn_val_bytes", "wgnn_val_init", "wgnn_val_begin", "wgnn_series_val_workspace_bytes",
         "wgnn_series_val", "wgnn_val_close"}


def test_val_prototypes_match_the_header_argument_for_argument():
    L, lib = _lib()
    protos = _prototypes("windgnn_series_val.h")
    assert set(protos) == set(L.EXPORTS_SERIES_VAL) == NAMES
    for name, (ret, args) in protos.items():
        res, argtypes = L.EXPORTS_SERIES_VAL[name]
        assert len(args) == len(argtypes), (name, args, argtypes)
        for i, (decl, t) in enumerate(zip(args, argtypes)):
            assert _c_kind(decl) == _ctype_kind(t), (name, i, decl, t)
        want = "ptr" if "*" in ret else {"int": "i32", "size_t": "size"}[ret.replace("const", "").strip()]
        assert _ctype_kind(res) == want, (name, ret, res)
        assert hasattr(lib, name) and getattr(lib, name).argtypes == argtypes, name
    # the entry point is wgnn_series_fwd_lossfn's head (up to the spec), then what a forward-only pass reports
    f = _prototypes("windgnn_series_lossfn.h")["wgnn_series_fwd_lossfn"][1]
    v = protos["wgnn_series_val"][1]
    assert v[:8] == f[:8] and v[8:] == ["float wind_min", "float wind_max", "float* last", "float* loss", "void* val", "void* workspace",
                                        "size_t workspace_bytes", "void* stream"]
    hdr = open(os.path.join(ROOT, "include", "windgnn_series_val.h")).read()
    assert re.search(r"#define\s+WGNN_SERIES_VAL_VERSION\s+1\b", hdr)
    assert '#include "windgnn_series_lossfn.h"' in hdr and '#include "windgnn_best.h"' in hdr
    assert lib.wgnn_series_val_version() == L.SERIES_VAL_VERSION == 1
    assert lib.wgnn_val_bytes() == 256
    # every other header, version and table is as it was
    assert lib.wgnn_version() == 122 and lib.wgnn_series_version() == 1 and lib.wgnn_series_train_version() == 1
    assert lib.wgnn_series_at_version() == 1 and lib.wgnn_series_masked_version() == 1 and lib.wgnn_series_lossfn_version() == 1
    assert lib.wgnn_best_version() == L.BEST_VERSION and lib.wgnn_eval_version() == L.EVAL_VERSION
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != "windgnn_series_val.h":
            text = open(os.path.join(ROOT, "include", other)).read()
            assert "wgnn_val" not in text and "series_val" not in text, other
    for other in (L.EXPORTS, L.EXPORTS_OPTIM, L.EXPORTS_SCHED, L.EXPORTS_EVAL, L.EXPORTS_BEST, L.EXPORTS_SERIES,
                  L.EXPORTS_SERIES_TRAIN, L.EXPORTS_SERIES_AT, L.EXPORTS_SERIES_MASKED, L.EXPORTS_SERIES_LOSSFN):
        assert not set(other) & set(L.EXPORTS_SERIES_VAL)
    from windgnn_amd import build
    assert any(h.endswith("windgnn_series_val.h") for h in build.HEADERS) and "series.hip" in build.SOURCES


def test_val_words_are_the_headers_table():
    """The offsets, C types and order of the public words: the header's table, _lib.VAL_WORDS, and the record in series.hip."""
    L, _ = _lib()
    hdr = open(os.path.join(ROOT, "include", "windgnn_series_val.h")).read()
    rows = re.findall(r"^ \*\s+offset\s+(\d+)\s+(double|uint64|float|int64)\s+(\w+)\s", hdr, flags=re.M)
    assert [(name, int(off), ctype) for off, ctype, name in rows] == [
        ("sum", 0, "double"), ("count", 8, "uint64"), ("mean", 16, "double"), ("max_abs", 24, "float"), ("loss", 28, "float"),
        ("calls", 32, "int64"), ("passes", 40, "int64"), ("stale", 48, "int64")]
    dtype = {"double": "float64", "uint64": "int64", "float": "float32", "int64": "int64"}
    assert L.VAL_WORDS == {name: (int(off), dtype[ctype]) for off, ctype, name in rows}
    assert list(L.VAL_WORDS) == [name for _, _, name in rows]
    # no two words overlap, all lie inside the record, and wgnn_keep_best is pointed at `loss`
    spans = sorted((off, off + torch.empty((), dtype=getattr(torch, dt)).element_size()) for off, dt in L.VAL_WORDS.values())
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and spans[-1][1] <= 256
    assert "(const float*)((char*)val + 28)" in hdr and L.BEST_WORDS["improved"] == (32, "int32")
    from windgnn_amd.functional import val_word
    rec = torch.arange(256, dtype=torch.uint8)
    assert val_word(rec, "loss").dim() == 0 and val_word(rec, "loss").dtype == torch.float32
    assert val_word(rec, "loss").data_ptr() == rec.data_ptr() + 28 and val_word(rec, "stale").data_ptr() == rec.data_ptr() + 48
    assert int(val_word(rec, "calls")) == int.from_bytes(bytes(range(32, 40)), "little")


def _val(lib, L, sd, ws_bytes=1 << 40, null=(), ls_rows=14, starts=True, fn=(1, 0.0, 0, 0), val=1 << 33):
    """wgnn_series_val on non-NULL fake device pointers.  Every call must be refused on the host: a launch on these pointers
    would fault."""
    null = (null,) if isinstance(null, str) else null

    def P(name, v):
        return C.c_void_p(0 if name in null else v)
    p = L.Params(*([4096] * 8), None)
    if "p.w_hh" in null:
        p.w_hh = None
    spec = L.LossFn(*fn)
    return lib.wgnn_series_val(C.byref(sd) if "sd" not in null else None, P("A", 8192), P("Xs", 1 << 20),
                               P("starts", 1 << 21 if starts else 0), C.byref(p) if "p" not in null else None, P("Ls", 1 << 22),
                               ls_rows, C.byref(spec) if "fn" not in null else None, 0.0, 1.0, P("last", 1 << 24),
                               P("loss", 1 << 32), P("val", val), P("ws", 1 << 40), ws_bytes, None)


def test_every_refusal_of_the_entry_points_comes_before_any_launch():
    L, lib = _lib()
    for stride, starts in ((0, True), (1, False)):                # the table form and the strided form
        sd = _sd(L, stride=stride, n=4)
        kw = {"starts": starts}
        for name in ["sd", "A", "Xs", "p", "p.w_hh", "ws", "Ls", "fn"] + (["starts"] if starts else []):
            assert _val(lib, L, sd, null=name, **kw) == ERR_NULL, (stride, name)
        assert _val(lib, L, sd, null=("loss", "val"), **kw) == ERR_NULL           # nothing to report
        for bad in (_sd(L, stride=stride, T=15), _sd(L, stride=stride, n=0), _sd(L, stride=stride, T=0),
                    _sd(L, stride=stride, rows=0), _sd(L, stride=stride, F=12), _sd(L, stride=stride, S=0),
                    _sd(L, stride=stride, H=0)):
            assert _val(lib, L, bad, ls_rows=1 << 24, **kw) == ERR_SHAPE, bytes(bad)
            assert lib.wgnn_series_val_workspace_bytes(C.byref(bad)) == 0
        for bad in (_sd(L, stride=stride, math=1), _sd(L, stride=stride, adj=1, nnz=20), _sd(L, stride=stride, H=129),
                    _sd(L, stride=stride, S=65), _sd(L, stride=stride, io=1)):
            assert _val(lib, L, bad, **kw) == ERR_UNSUPPORTED, bytes(bad)
            assert lib.wgnn_series_val_workspace_bytes(C.byref(bad)) == 0
        short = 13 if stride == 0 else (4 - 1) * stride + 5 - 1                 # one label row too few
        assert _val(lib, L, sd, ls_rows=short, **kw) == ERR_SHAPE
        assert _val(lib, L, sd, ls_rows=-(-(1 << 31) // 21), **kw) == ERR_SHAPE
        assert _val(lib, L, sd, val=(1 << 33) + 128, **kw) == ERR_SHAPE            # the record is 256-byte aligned
        need = lib.wgnn_series_val_workspace_bytes(C.byref(sd))
        assert need > 0 and _val(lib, L, sd, ws_bytes=need - 1, **kw) == ERR_WORKSPACE
        # forward-only: no stash beside it, and less than the training pair's workspace alone
        train = getattr(lib, "wgnn_series_at_workspace_bytes" if stride == 0 else "wgnn_series_workspace_bytes")(C.byref(sd))
        assert need < train
        for fn in ((-1, 0.0, 0, 0), (3, 0.0, 0, 0), (0, 0.0, 0, 2), (1, 0.0, 0, -1), (1, 0.0, -1, 0), (1, 0.0, 5, 0), (0, 0.0, 5, 1),
                   (2, 0.0, 0, 0), (2, -0.25, 0, 1), (2, float("inf"), 0, 0), (2, float("nan"), 2, 0)):
            assert _val(lib, L, sd, fn=fn, **kw) == ERR_SHAPE, (stride, fn)
        # ... the spec comes last: a short workspace, a short label series and a NULL are reported first
        assert _val(lib, L, sd, fn=(3, 0.0, 0, 0), ws_bytes=need - 1, **kw) == ERR_WORKSPACE
        assert _val(lib, L, sd, fn=(3, 0.0, 0, 0), ls_rows=short, **kw) == ERR_SHAPE
        assert _val(lib, L, sd, fn=(3, 0.0, 0, 0), null="Ls", **kw) == ERR_NULL
        # a valid spec, either output alone and a NULL `last` get as far as the workspace check (and never to a launch)
        for fn in ((0, float("nan"), 0, 0), (1, -1.0, 4, 1), (2, 0.25, 2, 0)):
            for null in ("loss", "val", "last", ("last", "val")):
                assert _val(lib, L, sd, fn=fn, null=null, ws_bytes=need - 1, **kw) == ERR_WORKSPACE, (fn, null)
    # the two forms do not mix
    assert _val(lib, L, _sd(L, stride=1, n=4), starts=True) == ERR_SHAPE
    assert _val(lib, L, _sd(L, stride=0, n=4), starts=False) == ERR_NULL
    assert _val(lib, L, _sd(L, stride=-1, n=4), starts=False) == ERR_SHAPE
    assert lib.wgnn_series_val_workspace_bytes(None) == 0
    # the record's own calls
    for fn in (lib.wgnn_val_init, lib.wgnn_val_begin):
        assert fn(None, None) == ERR_NULL
    assert lib.wgnn_val_close(None, C.c_void_p(1 << 33), None) == ERR_NULL


def test_the_workspace_holds_no_window_major_region():
    """Rows fixed, windows doubled: the workspace grows by the statistics and the last rows alone (12 bytes per 16 windows and
    4 H per window, in 256-byte steps), nothing like n T rows of 3 H floats."""
    L, lib = _lib()
    size = lambda n: lib.wgnn_series_val_workspace_bytes(C.byref(L.SeriesDims(9000, 24, 1, n, 34, 13, 102, 0, 0, 0, 0)))   # noqa: E731
    a, b = size(4096), size(8192)
    assert 0 < a < b and b - a <= 4096 * 102 * 4 + 4096 // 16 * 12 + 2 * 256 < 4096 * 24 * 102 * 4


# ---- the Python layer ---------------------------------------------------------------------------------------------------------
class Rec:
    def __init__(self):
        self.events = []

    def __call__(self, *e):
        self.events.append(e)


def _stubs(monkeypatch, rec):
    """Recording replacements of what trainer.py launches on behalf of validate_series."""
    from windgnn_amd import trainer

    def series_val_raw(A, series, params, Ls, seq_len, stride=None, n_windows=None, prepared=None, loss="mse", huber_delta=1.0,
                       loss_from=0, missing_labels=False, starts=None, last=None, val=None, wind_min=0.0, wind_max=1.0):
        assert prepared is not None and val is not None
        rec("series_val", stride, n_windows, None if starts is None else starts.tolist(), loss, huber_delta, loss_from,
            missing_labels, None if last is None else tuple(last.shape), wind_min, wind_max)

    stubs = dict(series_val_raw=series_val_raw, _require_gpu=lambda *t, **kw: rec("require_gpu"),
                 prepared_weights=lambda d, params, device: rec("images") or torch.zeros(1),
                 refresh_prepared=lambda d, params, prepared: rec("refresh_images"),
                 val_buffer=lambda device: rec("val_buffer") or torch.zeros(256, dtype=torch.uint8),
                 val_begin=lambda record: rec("val_begin"), val_init=lambda record: rec("val_init"),
                 val_close=lambda record, best=None: rec("val_close", best is not None),
                 best_init=lambda record, threshold: rec("best_init", threshold),
                 keep_best_args=lambda d, loss, params, best_params, record: ("marshalled", loss),
                 keep_best_launch=lambda args, step: rec("keep_best", step, args[1].data_ptr()))
    for name, fn in stubs.items():
        assert hasattr(trainer, name), name
        monkeypatch.setattr(trainer, name, fn)


A, SERIES, LS = torch.rand(7, 7), torch.rand(14, 7, 13), torch.rand(14, 21)


def test_validate_series_refuses_by_the_arguments_name_before_any_launch(monkeypatch):
    rec = Rec()
    _stubs(monkeypatch, rec)
    for kw in ({"stride": 3, "n_windows": 4}, {"starts": [0, 3, 3, 9]}):
        def go(tr=None, A=A, series=SERIES, Ls=LS, **more):
            return (tr or _cpu_step()).validate_series(A, series, Ls, 5, **kw, **more)
        with pytest.raises(ValueError, match=r"TrainStep\.validate_series: loss='smooth_l1'.*'mse', 'l1' or 'huber'"):
            go(loss="smooth_l1")
        for bad in (-1, 5, 6, 2.5):
            with pytest.raises(ValueError, match=r"loss_from=.*\[0, seq_len = 5\)"):
                go(loss_from=bad)
        for bad in (0.0, -0.25, float("inf"), float("nan")):
            with pytest.raises(ValueError, match=r"huber_delta=.*finite and > 0"):
                go(loss="huber", huber_delta=bad)
        for Ls in (torch.rand(14, 20), torch.rand(14), torch.rand(9, 21)):
            with pytest.raises(RuntimeError, match=r"TrainStep\.validate_series: .*the label series Ls must be \[rows >="):
                go(Ls=Ls)
        with pytest.raises(RuntimeError, match=r"validate_series with math != 'f32'.*torch\.no_grad"):
            go(_cpu_step(math="f16x3"))
        with pytest.raises(RuntimeError, match=r"series must be \[rows, S, 13\]"):
            go(series=torch.rand(14, 7, 12))
        with pytest.raises(ValueError, match=r"evaluator= must be an evaluate\.Evaluator of this model's 21 outputs"):
            go(evaluator=object())

        class Csr:
            blob = None
        with pytest.raises(RuntimeError, match=r"validate_series with a CsrAdjacency.*dense adjacency"):
            go(A=Csr())
    with pytest.raises(ValueError, match=r"pass stride= or starts=, not both"):
        _cpu_step().validate_series(A, SERIES, LS, 5, stride=2, starts=[0, 1])
    with pytest.raises(RuntimeError, match=r"validate_series: n_windows = 5, but a series of 14 rows holds 4 windows"):
        _cpu_step().validate_series(A, SERIES, LS, 5, stride=3, n_windows=5)
    with pytest.raises(RuntimeError, match=r"validate_series needs at least one window"):
        _cpu_step().validate_series(A, SERIES, LS, 5, starts=[])
    assert rec.events == []                                        # not one launch, not one buffer


def test_the_raw_wrapper_refuses_before_the_device_is_asked_for():
    from windgnn_amd.series import series_val_raw, val_spec
    params = [torch.zeros(1)] * 8
    with pytest.raises(ValueError, match=r"loss='mae'.*'mse', 'l1' or 'huber'"):
        series_val_raw(A, SERIES, params, LS, 5, 1, loss="mae", out_loss=torch.zeros(1))
    with pytest.raises(ValueError, match=r"needs out_loss= or val="):
        series_val_raw(A, SERIES, params, LS, 5, 1)
    with pytest.raises(RuntimeError, match=r"MI355X|no CPU fallback"):            # in scope: the device is asked for next
        series_val_raw(A, SERIES, params, LS, 5, 1, out_loss=torch.zeros(1))
    # always a spec: the defaults are {MSE, 0, step 0, masked}
    for missing in (False, True):
        s = val_spec("mse", float("nan"), 0, 5, missing)
        assert (s.kind, s.delta, s.t_from, s.masked) == (0, 0.0, 0, int(missing))
    s = val_spec("huber", 0.25, 3, 5, True)
    assert (s.kind, s.delta, s.t_from, s.masked) == (2, 0.25, 3, 1)


def test_the_views_raise_with_the_reason_before_any_validation_call():
    tr = _cpu_step()
    for name in ("val_loss", "val_count", "val_passes", "val_stale"):
        with pytest.raises(RuntimeError, match=r"TrainStep\.%s is kept by validate_series.*no validation call has run" % name):
            getattr(tr, name)


def test_best_on_option_checks(monkeypatch):
    with pytest.raises(ValueError, match=r"best_on='validation'\) needs keep_best"):
        _cpu_step(best_on="validation")
    with pytest.raises(ValueError, match=r"best_on='validation'\) needs keep_best"):
        _cpu_step(best_on="validation", keep_best=False)
    for bad in ("val", "Train", None, 1):
        with pytest.raises(ValueError, match=r"best_on=.*'train'.*or 'validation'"):
            _cpu_step(best_on=bad, keep_best=None)
    assert _cpu_step().best_on == "train" and _cpu_step(best_on="train").best_on == "train"
    rec = Rec()
    _stubs(monkeypatch, rec)
    assert _cpu_step(best_on="validation", keep_best=0.5).best_on == "validation" and rec.events == [("best_init", 0.5)]


def test_state_dict_has_exactly_its_four_keys_without_a_record(monkeypatch):
    from windgnn_amd import _lib as L
    tr = _cpu_step()
    assert list(tr.state_dict()) == ["optimizer", "steps", "best", "carry"]
    rec = Rec()
    _stubs(monkeypatch, rec)
    tr.validate_series(A, SERIES, LS, 5, stride=3, more=True)
    with pytest.raises(RuntimeError, match=r"state_dict\(\): a validation pass is open.*more=False"):
        tr.state_dict()
    tr.validate_series(A, SERIES, LS, 5, stride=3)
    sd = tr.state_dict()
    assert list(sd) == ["optimizer", "steps", "best", "carry", "val"] and list(sd["val"]) == list(L.VAL_WORDS)
    # and back: into a TrainStep that has no record yet, and over one that has
    sd["val"]["stale"] = torch.tensor(7)
    sd["val"]["passes"] = torch.tensor(9)
    for other in (_cpu_step(), tr):
        other.load_state_dict(sd)
        assert int(other.val_stale) == 7 and int(other.val_passes) == 9
    del sd["val"]["mean"]
    with pytest.raises(ValueError, match=r"the validation record lacks mean"):
        _cpu_step().load_state_dict(sd)


@pytest.mark.parametrize("best_on", ["train", "validation"])
def test_a_pass_opens_once_accumulates_and_closes_through_keep_best(monkeypatch, best_on):
    rec = Rec()
    _stubs(monkeypatch, rec)
    tr = _cpu_step(keep_best=True, best_on=best_on, check_every=1)
    before = (tr.flat_p.clone(), tr._gbuf.clone(), tr.exp_avg.clone())
    tr.steps = 41
    rec.events.clear()
    loss = tr.validate_series(A, SERIES, LS, 5, stride=3, n_windows=3, more=True)
    assert loss.dim() == 0 and loss.dtype == torch.float32 and loss.data_ptr() == tr._val.data_ptr() + 28
    val = ("series_val", 3, 3, None, "mse", 1.0, 0, False, None, 0.0, 1.0)
    assert rec.events == [("require_gpu",), ("images",), ("val_buffer",), ("val_begin",), val]
    rec.events.clear()
    tr.validate_series(A, SERIES, LS, 5, starts=[9, 0, 3], loss="huber", huber_delta=0.25, loss_from=2, missing_labels=True)
    close = [("keep_best", 41, tr._val.data_ptr() + 28), ("val_close", True)] if best_on == "validation" else [("val_close", False)]
    # the second call of the pass: no new record, no begin; the table sorted; then the decision and the close
    assert rec.events == [("require_gpu",), ("series_val", None, None, [0, 3, 9], "huber", 0.25, 2, True, None, 0.0, 1.0)] + close
    rec.events.clear()
    tr.validate_series(A, SERIES, LS, 5, stride=3)
    assert rec.events == [("require_gpu",), ("val_begin",), ("series_val", 3, 4, None, "mse", 1.0, 0, False, None, 0.0, 1.0)] + close
    # no optimiser, bucket or `steps` change
    assert tr.steps == 41 and all(torch.equal(a, b) for a, b in zip(before, (tr.flat_p, tr._gbuf, tr.exp_avg)))


def test_a_training_step_decides_under_train_and_not_under_validation(monkeypatch):
    import test_trainstep_schedule_host as ts
    from windgnn_amd import trainer
    for best_on, want in (("train", [("keep_best", 1)]), ("validation", [])):
        rec = ts.Recorder()
        for name, fn in ts._bindings(rec, 21).items():
            monkeypatch.setattr(trainer, name, fn)
        monkeypatch.setattr(trainer, "best_init", lambda record, threshold: None)
        monkeypatch.setattr(trainer, "keep_best_args", lambda *a: ("marshalled once",))
        tr = _cpu_step(keep_best=True, best_on=best_on, check_every=0)
        tr.step_series(A, SERIES, LS, 5, 3, n_windows=4)
        assert rec.events == [("require_gpu",), ("images",), ("series_forward_loss", 4), ("series_bwd_mse", 1.0), ("finish", 0, 1)] + want


# ---- qualification of the cases on the oracle alone ---------------------------------------------------------------------------
def test_the_case_list_is_what_the_issue_asks_for():
    import series_at_cases as sc
    assert len(vc.GRID) == 2 * 3 * 3 * 2 and len(vc.INSTANCES) == 9 and len(vc.CASES) == 36 + 5 + 9
    q = vc.reference("irregular-table-e-mse-from0")
    assert (q.S, q.H, q.rows, q.T, q.n, q.stride) == (7, 21, 40, 5, 19, None)
    q = vc.reference("irregular-stride2-b-huber-from4")
    assert (q.S, q.H, q.rows, q.T, q.n, q.stride, q.masked, q.delta) == (7, 21, 40, 5, 18, 2, 1, 0.25)
    q = vc.reference(vc.REAL[0])
    assert (q.S, q.H, q.rows, q.T) == (34, 102, 66, 24)
    seen = set()
    for cid, K in zip(vc.INSTANCES, sc.FWD_KS):
        q = vc.reference(cid)
        assert (q.rows, q.T, q.n, q.H) == (36, 3, 17, 4 * K) and sc.fwd_ks(q.H) == K
        seen.add("gru_fwd_kernel<%d%s,lossfn>" % (K, ",starts" if q.stride is None else ""))
    assert len(seen) == 9 and {vc.reference(c).kind for c in vc.INSTANCES} == {"mse", "l1", "huber"}
    assert {vc.reference(c).stride for c in vc.INSTANCES} == {None, 2} and {vc.reference(c).masked for c in vc.INSTANCES} == {0, 1}


@pytest.mark.parametrize("cid", list(vc.CASES))
def test_a_case_qualifies_on_the_oracle_alone(cid):
    q = vc.reference(cid)
    assert q.margin > 1e-5, (cid, q.margin)
    loss, m = vc.oracle_loss(q)
    assert loss == q.loss_o and m == q.m == sum(q.counts) and 0 < m
    assert m == q.n * (q.T - q.t_from) * q.H if not q.masked else m < q.n * (q.T - q.t_from) * q.H
    assert (q.masked == 1) == bool(torch.isnan(q.L).any())
    assert torch.isfinite(torch.tensor(q.loss_o)) and 0 < q.loss_o < 4.0


def test_two_planted_mistakes_are_visible_on_the_inputs_the_gpu_test_uses():
    """Module docstring: which cases each mistake is claimed on, and why not on the others."""
    shown = {"last step only": 0, "mean over n T H": 0}
    for cid in vc.CASES:
        q = vc.reference(cid)
        if q.t_from > 0:
            wrong, _ = vc.oracle_loss(q, divide_by=q.n * q.T * q.H)
            moved = abs(wrong - q.loss_o) / q.loss_o
            print(cid, "mean over n T H: %.3e" % moved)
            assert moved >= 1e-2, (cid, moved)
            shown["mean over n T H"] += 1
        if q.t_from < q.T - 1:
            wrong, _ = vc.oracle_loss(q, t_from=q.T - 1)
            moved = abs(wrong - q.loss_o) / q.loss_o
            print(cid, "last step only: %.3e" % moved)
            if (q.base == "irregular" and q.kind in ("mse", "huber")) or cid == "real_widths-table-a-mse-from0":
                assert moved >= 1e-2, (cid, moved)
                shown["last step only"] += 1
    assert shown == {"last step only": 2 * 2 * 2 * 2 + 1, "mean over n T H": 2 * 3 * 2 * 2 + 4 + 9}, shown
