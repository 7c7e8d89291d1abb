"""Series validation on the MI355X (include/windgnn_series_val.h, series.series_val_raw, TrainStep.validate_series): the held-out
loss of a spec, forward-only, accumulated in a device record that ends in wgnn_keep_best and a patience counter.
tests/test_series_val_host.py qualifies the cases (tests/series_val_cases.py) on the CPU.

Bit-identity is derivable, so it is exact: loss[0] is the word wgnn_series_fwd_lossfn + wgnn_series_bwd_lossfn write for the same
inputs and spec (the same partial sums, added in BPTT's order, times the same 1.0f / (float)m), `last` is wgnn_series_fwd_last's
output, and the record's count is the oracle's integer.  Against the fp64 oracle on the MATERIALISED windows, with the loss formed
in the test, the bar is the series suites' 1e-4: the record's mean relative to the oracle's loss, `last` by conftest.rel_to_max
against the de-normalised oracle rows.  The observed errors are printed per case.

The entry point runs on buffers of exactly their ABI lengths inside a guarded.Arena, the workspace at exactly
wgnn_series_val_workspace_bytes, under the library's profiler: a case also proves by the launched names that the `lossfn`
recurrence instance and series_val_finish_kernel ran and that no BPTT, fold or weight-gradient launch did."""
import ctypes as C
import functools

import pytest
import torch

import series_at_cases as sc
import series_lossfn_cases as lc
import series_val_cases as vc
from conftest import PARAM_KEYS, rel_to_max
from guarded import FILLS, Arena
from test_gpu_series import F, STATUS, TOL, WIND_MAX, WIND_MIN, _dev, _fit
from test_gpu_series_at import _model_of
from test_gpu_series_lossfn import _arena_step, _f32
from test_series_at_host import ERR_NULL

pytestmark = pytest.mark.gpu

NO_LOSS_STATS, NO_LABELS = 8, 32       # WGNN_STATUS_NO_LOSS_STATS, WGNN_STATUS_NO_LABELS
BACKWARD = ("gru_bwd_kernel", "series_fold", "gemm32_tn", "gemm_f32_tn", "finish", "gcn32_bwd", "gcn_partial")


@functools.lru_cache(maxsize=None)
def _checked(cid):
    q = vc.reference(cid)
    assert q.margin > 1e-5, "a ReLU pre-activation within %.1e of zero (relative): pick another seed" % q.margin
    return q


def _spec(q):
    return (lc.KINDS[q.kind], q.delta, q.t_from, q.masked)


def _words(rec):
    """The public words of a record's host bytes."""
    from windgnn_amd import _lib as L
    from windgnn_amd.functional import val_word
    return {name: val_word(rec, name).clone() for name in L.VAL_WORDS}


def _val_run(q, fill="nan", dirty=None, spec=None, Ls=None, starts=None, cuts=None, passes=1, null=(), status=0,
             wind=(WIND_MIN, WIND_MAX), gate=None):
    """wgnn_val_init on a dirty record, then `passes` passes of wgnn_val_begin + wgnn_series_val + wgnn_val_close(NULL) on the
    reference q inside an arena.  starts: another table than q's (table mapping); cuts: window indices at which the table is cut
    into several calls of one pass (table mapping; each call gets exactly its own workspace_bytes); null: outputs passed as NULL
    ("last", "loss", "val").  Returns (outputs as host tensors, the record's words after each pass, launched names, scratch).
    gate (tests/stream_cases.py): the calls go to its side stream, nothing synchronises between the passes (the record's words
    are those after the last one only), and no kernel names are collected."""
    from windgnn_amd import _lib as L
    lib = L.load()
    table = q.starts if starts is None else starts
    n, T, H, rows = len(table), q.T, q.H, q.rows
    assert cuts is None or q.stride is None
    edges = [0] + list(cuts or []) + [n]
    calls = [(a, b) for a, b in zip(edges, edges[1:])]

    def dims(k):
        return L.SeriesDims(rows, T, q.stride or 0, k, q.S, F, H, 0, 0, 0, 0)
    need = [lib.wgnn_series_val_workspace_bytes(C.byref(dims(b - a))) for a, b in calls]
    ws_bytes = max(need)
    assert min(need) > STATUS and lib.wgnn_val_bytes() == 256
    if cuts is None:      # forward-only: below the training pair's workspace alone, and no stash beside it
        fam = "wgnn_series_at_%s" if q.stride is None else "wgnn_series_%s"
        assert ws_bytes < getattr(lib, fam % "workspace_bytes")(C.byref(dims(n)))
    a = Arena(_dev(), fill)
    dirty = dirty or {}

    def add(name, t=None, shape=None):
        return a.buf(name, (t.numel() if t is not None else int(torch.tensor(shape).prod())) * 4, data=t)
    add("A", q.A)
    add("Xs", q.Xs)
    ls_rows = rows if q.stride is None else (n - 1) * q.stride + T       # the least each form accepts: a read past them hits the guard
    add("Ls", (q.Ls if Ls is None else Ls)[:ls_rows].contiguous())
    add("starts", torch.tensor(table, dtype=torch.int32))
    for k in PARAM_KEYS:
        add("p." + k, q.p[k])
    add("last", shape=(n, H))
    add("loss", shape=(len(calls),))
    a.buf("val", 256, data=_fit(dirty["val"], 256) if "val" in dirty else None)     # dirty before wgnn_val_init: the fill, or worse
    a.buf("ws", ws_bytes, data=_fit(dirty["ws"], ws_bytes) if "ws" in dirty else None, zero_head=STATUS)
    a.commit()
    ps = L.Params()
    for (field, _), k in zip(L.Grads._fields_, PARAM_KEYS):
        setattr(ps, field, a["p." + k].ptr)
    word = a["ws"].view(torch.int32)
    fn = L.LossFn(*(_spec(q) if spec is None else spec))

    def P(name, off=0):
        return None if name in null else C.c_void_p(a[name].ptr + off)
    records = []
    st = gate.handle if gate is not None else None
    if gate is not None:
        gate.begin(a, ints=("starts",))
    else:
        L.profile_enable(True)
    try:
        with_val = "val" not in null
        assert not with_val or lib.wgnn_val_init(P("val"), st) == 0
        for _ in range(passes):
            assert not with_val or lib.wgnn_val_begin(P("val"), st) == 0
            for i, (lo, hi) in enumerate(calls):
                sd = dims(hi - lo)
                rc = lib.wgnn_series_val(C.byref(sd), P("A"), P("Xs"), P("starts", 4 * lo) if q.stride is None else None,
                                         C.byref(ps), P("Ls"), ls_rows, C.byref(fn), wind[0], wind[1], P("last", 4 * lo * H),
                                         P("loss", 4 * i), P("val"), P("ws"), need[i], st)
                assert rc == 0, rc
            assert not with_val or lib.wgnn_val_close(P("val"), None, st) == 0
            if gate is None:
                torch.cuda.synchronize()
                records.append(_words(a["val"].host()))
        names = tuple(rec["name"] for rec in L.profile_read()) if gate is None else ()
    finally:
        if gate is None:
            L.profile_enable(False)
    if gate is not None:
        gate.end()
        records.append(_words(a["val"].host()))
    assert a.check() == {}, (fill, a.check())
    assert int(word[0]) == status, ("status word", int(word[0]), status)
    if fill != "zero" and "ws" not in dirty:
        for name in ("last", "loss"):
            if name not in null:
                assert a[name].unwritten(4) == 0, (name, fill)
        assert "val" in null or a["val"].unwritten(8) == 0, fill   # wgnn_val_init writes every byte
    for name in ("last", "loss", "val"):
        if name in null:
            assert a[name].unwritten(1) == a[name].nbytes, name
    for name in ("A", "Xs", "Ls", "starts") + tuple("p." + k for k in PARAM_KEYS):      # inputs are read only
        assert a[name].unwritten(1) == a[name].nbytes, name
    out = {"last": a["last"].host(), "loss": a["loss"].host(), "val": a["val"].host()}
    return out, records, names, {k: a[k].host() for k in ("ws", "val")}


def _assert_names(q, names):
    """The lossfn instance of this H and row mapping and the finish ran; no sibling instance and nothing of a backward did."""
    want = "gru_fwd_kernel<%d%s,lossfn>" % (sc.fwd_ks(q.H), ",starts" if q.stride is None else "")
    assert {x for x in names if x.startswith("gru_fwd_kernel")} == {want}, names
    assert "series_val_finish_kernel" in names
    assert not [x for x in names if x.startswith(BACKWARD)], names
    assert ("series_starts_check_kernel" in names) == (q.stride is None), names


def _fwd_last(q, starts=None):
    """wgnn_series_fwd_last (or its _at form) on the reference q, through forward_last_series: host [n, H]."""
    from windgnn_amd.series import forward_last_series
    dev = _dev()
    kw = {"starts": q.starts if starts is None else starts} if q.stride is None else {"stride": q.stride, "n_windows": q.n}
    return forward_last_series(_model_of(q.r), q.A.to(dev), q.Xs.to(dev), q.T, WIND_MIN, WIND_MAX, **kw).cpu()


def _max_abs(q):
    on = lc.counted(q.L, q.t_from, q.masked)
    return float((q.Yo - torch.nan_to_num(q.L.double()))[on].abs().max())


# ---- 1. the bits of the training pair, the rows of wgnn_series_fwd_last, the oracle's count and loss --------------------------------
@pytest.mark.parametrize("cid", list(vc.CASES))
def test_validation_is_the_training_pairs_loss_bit_for_bit_and_the_oracles_within_the_bar(cid):
    q = _checked(cid)
    pair, _, _ = _arena_step(q)                                    # wgnn_series_fwd_lossfn + wgnn_series_bwd_lossfn, q's own spec
    out, records, names, _ = _val_run(q)
    _assert_names(q, names)
    assert torch.equal(out["loss"], pair["loss"]), (cid, _f32(out["loss"], (1,)), _f32(pair["loss"], (1,)))
    assert torch.equal(_f32(out["last"], (q.n, q.H)), _fwd_last(q)), (cid, "last differs from wgnn_series_fwd_last")
    w = records[0]
    assert int(w["count"]) == q.m == sum(pair["counts"].tolist()), (cid, int(w["count"]), q.m)
    if not q.masked:
        assert int(w["count"]) == q.n * (q.T - q.t_from) * q.H
    assert (int(w["calls"]), int(w["passes"]), int(w["stale"])) == (1, 1, 0)
    assert float(w["loss"]) == float(torch.tensor(float(w["mean"]), dtype=torch.float64).float())      # loss = (float)mean
    assert float(w["mean"]) == float(w["sum"]) / q.m
    err = {"mean": abs(float(w["mean"]) - q.loss_o) / q.loss_o,
           "loss[0]": abs(float(_f32(out["loss"], (1,))[0]) - q.loss_o) / q.loss_o,
           "max_abs": abs(float(w["max_abs"]) - _max_abs(q)) / _max_abs(q),
           "last": rel_to_max(_f32(out["last"], (q.n, q.H)), vc.last_rows(q, WIND_MIN, WIND_MAX))}
    print("\n%s (m = %d of %d): worst %.2e  " % (cid, q.m, q.n * q.T * q.H, max(err.values())) +
          "  ".join("%s %.2e" % kv for kv in err.items()))
    for k, e in err.items():
        assert e <= TOL, (cid, k, e)


# ---- 2. accumulation ------------------------------------------------------------------------------------------------------------
TRIPLE = "irregular-table-b-huber-from2"      # its table three times over: 57 windows, four workgroups, the last one ragged


def _triple(q):
    return sorted(list(q.starts) * 3)


def test_a_pass_cut_at_workgroup_boundaries_adds_the_same_bits_and_off_them_the_same_count():
    q = _checked(TRIPLE)
    table = _triple(q)
    assert len(table) == 57
    one, rec1, _, _ = _val_run(q, starts=table, passes=2)
    w = rec1[0]
    # every window three times: the oracle's mean is the case's own, the count three times its count
    assert int(w["count"]) == 3 * q.m and abs(float(w["mean"]) - q.loss_o) <= TOL * q.loss_o
    # a second identical pass after wgnn_val_begin gives the same bits, and passes counts up
    for name in ("sum", "count", "mean", "max_abs", "loss", "calls"):
        assert torch.equal(rec1[1][name], w[name]), name
    assert (int(w["passes"]), int(rec1[1]["passes"]), int(w["calls"])) == (1, 2, 1)
    # three unequal calls cut at multiples of 16 windows: the same partial sums, added onto the running sum in the same order
    cut, rec3, _, _ = _val_run(q, starts=table, cuts=(16, 48))
    assert int(rec3[0]["calls"]) == 3
    for name in ("sum", "count", "mean", "max_abs", "loss"):
        assert torch.equal(rec3[0][name], w[name]), name
    assert torch.equal(cut["last"], one["last"])
    # ... once off a boundary: the same terms, but other windows share a workgroup, so they are grouped into other fp32
    # per-workgroup partial sums before the fp64 sum.  1e-6 relative on the mean: fp64 sums of fp32 partial sums -- the fp64
    # additions are exact to 2^-53, each fp32 partial sum is rounded at 2^-24 = 6e-8 over its dozen levels of additions
    off, rec_off, _, _ = _val_run(q, starts=table, cuts=(10, 40))
    assert int(rec_off[0]["count"]) == int(w["count"]) and int(rec_off[0]["calls"]) == 3
    moved = abs(float(rec_off[0]["mean"]) - float(w["mean"])) / float(w["mean"])
    print("\nmean off the workgroup boundaries: %.2e relative" % moved)
    assert moved <= 1e-6, moved
    assert torch.equal(off["last"], one["last"])
    # the per-call loss words are the training pair's on each sub-table (here: of the first call)
    assert torch.equal(cut["loss"][:4], _val_run(q, starts=table[:16])[0]["loss"])


# ---- 3. edge cases ----------------------------------------------------------------------------------------------------------------
def test_without_any_label_the_loss_is_nan_the_status_says_so_and_keep_best_does_not_win():
    from windgnn_amd import _lib as L
    from windgnn_amd.functional import best_init, best_word, keep_best, val_word
    q = lc.reference("irregular", "table", "f", "l1", 0.0, 2)
    assert q.m == 0 and q.masked == 1
    out, records, names, _ = _val_run(q, fill="finite", status=NO_LABELS)       # (not the NaN fill: the loss written is a NaN itself)
    _assert_names(q, names)
    w = records[0]
    assert torch.isnan(_f32(out["loss"], (1,))).all() and torch.isnan(w["loss"]) and torch.isnan(w["mean"])
    assert int(w["count"]) == 0 and float(w["sum"]) == 0.0 and float(w["max_abs"]) == 0.0 and int(w["passes"]) == 1
    assert torch.isfinite(_f32(out["last"], (q.n, q.H))).all()
    # wgnn_keep_best on the record's loss word, then wgnn_val_close with the best record: no win, stale counts
    dev = _dev()
    rec = out["val"].to(dev)
    best = torch.empty(256, dtype=torch.uint8, device=dev)
    best_init(best, float("inf"))
    p = [q.p[k].to(dev) for k in PARAM_KEYS]
    snap = [torch.full_like(t, 7.0) for t in p]
    d = L.Dims(1, 1, q.S, 13, q.H, 0, 1, 1, 0)
    for want in (1, 2):
        keep_best(d, val_word(rec, "loss"), p, snap, 3, best)
        assert L.load().wgnn_val_close(C.c_void_p(rec.data_ptr()), C.c_void_p(best.data_ptr()), None) == 0
        assert (int(best_word(best, "improved")), int(best_word(best, "best_step")), int(val_word(rec, "stale"))) == (0, -1, want)
    assert all(bool((t == 7.0).all()) for t in snap) and int(val_word(rec, "passes")) == 3
    # a finite loss word wins, and the close that follows resets stale
    val_word(rec, "loss").fill_(0.5)
    keep_best(d, val_word(rec, "loss"), p, snap, 4, best)
    assert L.load().wgnn_val_close(C.c_void_p(rec.data_ptr()), C.c_void_p(best.data_ptr()), None) == 0
    assert (int(best_word(best, "improved")), int(best_word(best, "best_step")), int(val_word(rec, "stale"))) == (1, 4, 0)
    assert all(torch.equal(a, b) for a, b in zip(snap, p)) and float(best_word(best, "best_loss")) == 0.5


def test_a_nan_label_without_masked_poisons_the_loss_and_the_record():
    q = _checked("irregular-table-e-huber-from2")
    Ls = q.Ls.clone()
    Ls[q.starts[3] + 3, 5] = float("nan")                          # step 3 >= t_from of window 3
    out, records, _, _ = _val_run(q, fill="finite", Ls=Ls)
    w = records[0]
    assert torch.isnan(_f32(out["loss"], (1,))).all() and torch.isnan(w["sum"]) and torch.isnan(w["mean"]) and torch.isnan(w["loss"])
    assert int(w["count"]) == q.n * (q.T - q.t_from) * q.H         # counted: masked = 0 knows no missing label
    assert torch.isfinite(_f32(out["last"], (q.n, q.H))).all()


def test_either_output_alone_and_a_null_last_give_the_bits_of_the_full_call():
    """loss without a record (and with the last rows in the workspace), and a record without loss.  (The finish kernel's refusal
    of statistics that are not its spec's cannot be reached through the entry point, whose forward always writes them.)"""
    q = _checked("irregular-stride2-b-l1-from2")
    base, rec, _, _ = _val_run(q)
    only_loss, _, _, _ = _val_run(q, null=("val", "last"))
    assert torch.equal(only_loss["loss"], base["loss"])
    only_val, rec2, _, _ = _val_run(q, null=("loss",))
    for name in ("sum", "count", "mean", "max_abs", "loss", "calls", "passes"):
        assert torch.equal(rec2[0][name], rec[0][name]), name
    assert torch.equal(only_val["last"], base["last"])


def test_loss_and_val_both_null_is_refused():
    from windgnn_amd import _lib as L
    lib = L.load()
    q = _checked("irregular-table-e-mse-from0")
    dev = _dev()
    sd = L.SeriesDims(q.rows, q.T, 0, q.n, q.S, F, q.H, 0, 0, 0, 0)
    t = {k: v.to(dev) for k, v in (("A", q.A), ("Xs", q.Xs), ("Ls", q.Ls), ("starts", torch.tensor(q.starts, dtype=torch.int32)))}
    p = [q.p[k].to(dev) for k in PARAM_KEYS]
    ps = L.Params(*[x.data_ptr() for x in p], None)
    ws = torch.zeros(lib.wgnn_series_val_workspace_bytes(C.byref(sd)), dtype=torch.uint8, device=dev)
    last = torch.full((q.n, q.H), -5.0, device=dev)
    fn = L.LossFn(0, 0.0, 0, 0)
    rc = lib.wgnn_series_val(C.byref(sd), *(C.c_void_p(t[k].data_ptr()) for k in ("A", "Xs", "starts")), C.byref(ps),
                             C.c_void_p(t["Ls"].data_ptr()), q.rows, C.byref(fn), 0.0, 1.0, C.c_void_p(last.data_ptr()), None, None,
                             C.c_void_p(ws.data_ptr()), ws.numel(), None)
    torch.cuda.synchronize()
    assert rc == ERR_NULL and bool((last == -5.0).all()) and not ws.any()          # refused before any launch


@pytest.mark.parametrize("cid", ["irregular-table-b-huber-from2", "irregular-stride2-e-l1-from0"])
def test_footprint_guards_fills_a_dirty_record_and_dirty_scratch(cid):
    q = _checked(cid)
    assert FILLS[0] == "zero"
    base, rec0, _, _ = _val_run(q, fill=FILLS[0])

    def same(out, rec, what):
        for key in ("last", "loss"):
            assert torch.equal(out[key], base[key]), (key, what)
        for name, v in rec[0].items():
            assert torch.equal(v, rec0[0][name]), (name, what)
    for fill in FILLS[1:] + FILLS[1:2]:                                             # (and a second run of one)
        out, rec, _, _ = _val_run(q, fill=fill)
        same(out, rec, fill)
    _, _, _, left = _val_run(_checked("K8_small-stride2-e-huber-from1"), fill="nan")    # another shape's left-over scratch and record
    for fill in ("finite", "nan"):
        out, rec, _, _ = _val_run(q, fill=fill, dirty=left)
        same(out, rec, (fill, "dirty"))
    # a record full of the largest counters before wgnn_val_init
    out, rec, _, _ = _val_run(q, fill="finite", dirty={"val": torch.full((64,), 0x7FFFFFFF, dtype=torch.int32).view(torch.uint8)})
    same(out, rec, "dirty record")


# ---- 4. TrainStep ----------------------------------------------------------------------------------------------------------------
BASE = "irregular-table-e-mse-from0"
SHIFT = -4.0          # the third training step runs on labels moved by this much: it moves the model AWAY from the held-out labels
STEPS = 3


def _split(q):
    """(training starts, held-out starts): the even and the odd entries of the irregular table."""
    return [s for i, s in enumerate(q.starts) if i % 2 == 0], [s for i, s in enumerate(q.starts) if i % 2 == 1]


@functools.lru_cache(maxsize=None)
def _oracle_run():
    """The oracle's three Adam steps on the training windows (the third on shifted labels) and the held-out MSE after each:
    (validation losses, parameters after each step)."""
    from oracle import windgnn_oracle as orc
    q = _checked(BASE)
    even = [i for i in range(q.n) if i % 2 == 0]
    odd = [i for i in range(q.n) if i % 2 == 1]
    A = q.A.double()
    Xt, Lt, Xv, Lv = q.X.double()[even], q.L.double()[even], q.X.double()[odd], q.L.double()[odd]
    p = dict(q.p64)
    state = orc.adam_init(p)
    vals, params = [], []
    for s in range(STEPS):
        Y, cache = orc.forward(A, Xt, p)
        _, dY, _ = lc.loss_and_dy(Y, Lt + (SHIFT if s == 2 else 0.0), "mse", 0.0, 0, 0)
        p = orc.adam_step(p, orc.backward(A, Xt, p, Y, cache, dY), state)
        vals.append(float(lc.loss_and_dy(orc.forward(A, Xv, p, want_cache=False)[0], Lv, "mse", 0.0, 0, 0)[0]))
        params.append(p)
    return vals, params


def _rule(losses, threshold=float("inf")):
    """The host restatement: (best_step, stale after each pass) of `if loss < best: keep` with the patience counter."""
    best, best_step, stale, out = threshold, -1, 0, []
    for i, v in enumerate(losses):
        if v < best:
            best, best_step, stale = v, i + 1, 0
        else:
            stale += 1
        out.append(stale)
    return best_step, out


def _device_inputs(q):
    dev = _dev()
    return q.A.to(dev), q.Xs.to(dev), q.Ls.to(dev)


def test_the_best_model_and_the_patience_counter_follow_the_held_out_loss():
    from windgnn_amd.trainer import TrainStep
    q = _checked(BASE)
    vo, po = _oracle_run()
    gaps = [abs(a - b) / max(a, b) for i, a in enumerate(vo) for b in vo[i + 1:]]
    assert min(gaps) > 1e-2, (vo, "the oracle's validation losses must be separated by far more than the 1e-4 bar")
    want_step, want_stale = _rule(vo + vo[-1:])                    # a fourth pass on unchanged parameters: equal, so no win
    assert want_step == 2 and want_stale == [0, 0, 1, 2]           # the best step is not the last one
    A, Xs, Ls = _device_inputs(q)
    train, held = _split(q)
    tr = TrainStep(_model_of(q.r), keep_best=True, best_on="validation")
    got, stale, snaps = [], [], []
    for s in range(STEPS):
        tr.step_series(A, Xs, Ls + SHIFT if s == 2 else Ls, q.T, starts=train)
        assert int(tr.best_step) == (-1 if s == 0 else _rule(vo[:s])[0])          # a training step decides nothing
        snaps.append(tr.flat_p.clone())
        v = tr.validate_series(A, Xs, Ls, q.T, starts=held)
        assert v.dim() == 0 and v.data_ptr() == tr.val_loss.data_ptr()
        got.append(float(v))
        stale.append(int(tr.val_stale))
        assert int(tr.val_passes) == s + 1 and int(tr.val_count) == len(held) * q.T * q.H
    tr.validate_series(A, Xs, Ls, q.T, starts=held)
    stale.append(int(tr.val_stale))
    err = {"val%d" % (i + 1): abs(a - b) / b for i, (a, b) in enumerate(zip(got, vo))}
    print("\nvalidation losses %s against the oracle's %s: " % (got, vo) + "  ".join("%s %.2e" % kv for kv in err.items()))
    assert max(err.values()) <= TOL, err
    assert (int(tr.best_step), stale, int(tr.val_passes)) == (want_step, want_stale, 4)
    assert float(tr.best_loss) == got[want_step - 1] and float(tr.val_loss) == got[-1]
    assert torch.equal(tr._best_p, snaps[want_step - 1]) and not torch.equal(tr._best_p, tr.flat_p)
    kept = tr.best_state_dict()
    for k in PARAM_KEYS:
        assert rel_to_max(kept[k].cpu(), po[want_step - 1][k]) <= TOL, k
    assert tr.steps == STEPS


def test_validation_touches_nothing_of_a_run_that_decides_on_the_training_loss():
    from windgnn_amd.evaluate import Evaluator
    from windgnn_amd.trainer import TrainStep
    q = _checked(BASE)
    A, Xs, Ls = _device_inputs(q)
    train, held = _split(q)
    runs = []
    for validate in (False, True):
        model = _model_of(q.r)
        tr = TrainStep(model, keep_best=True, best_on="train", max_grad_norm=1.0)
        ev = Evaluator(model, A, WIND_MIN, WIND_MAX)
        losses = []
        for s in range(STEPS):
            loss, _ = tr.step_series(A, Xs, Ls, q.T, starts=train)
            losses.append(loss.clone())
            if validate:
                tr.validate_series(A, Xs, Ls, q.T, starts=held[:4], more=True, loss="huber", huber_delta=0.25, loss_from=2)
                tr.validate_series(A, Xs, Ls, q.T, stride=2, evaluator=ev, loss="huber", huber_delta=0.25, loss_from=2)
        runs.append((torch.stack(losses), tr.flat_p.clone(), tr.exp_avg.clone(), tr.exp_avg_sq.clone(), tr._best.clone(),
                     tr._best_p.clone(), tr._gbuf.clone()))
        if validate:
            assert int(tr.val_passes) == STEPS and int(tr.val_stale) == 0 and tr.steps == STEPS
    for a, b in zip(*runs):
        assert torch.equal(a, b)


@pytest.mark.parametrize("how,mask", [("table", "b"), ("stride2", "e")])
def test_the_evaluator_gets_the_bits_update_series_gives_it(how, mask):
    from windgnn_amd.evaluate import Evaluator
    from windgnn_amd.trainer import TrainStep
    q = _checked("irregular-%s-%s-mse-from0" % (how, mask))
    A, Xs, Ls = _device_inputs(q)
    model = _model_of(q.r)
    tr = TrainStep(model)
    if q.stride is None:
        perm = torch.randperm(q.n, generator=torch.Generator().manual_seed(11)).tolist()
        kw = {"starts": [q.starts[i] for i in perm]}               # any order: the rows reach the accumulator in the caller's
    else:
        kw = {"stride": q.stride, "n_windows": q.n}
    ev1, ev2 = Evaluator(model, A, WIND_MIN, WIND_MAX, keep_errors=True), Evaluator(model, A, WIND_MIN, WIND_MAX, keep_errors=True)
    v = tr.validate_series(A, Xs, Ls, q.T, missing_labels=bool(q.masked), evaluator=ev1, **kw)
    ev2.update_series(Xs, Ls, q.T, skip_missing=bool(q.masked), **kw)
    assert torch.equal(ev1.acc, ev2.acc) and bool(ev1.acc.any())
    e1, e2 = ev1.errors(), ev2.errors()                            # (NaN where a truth is missing, in both)
    assert torch.equal(torch.isnan(e1), torch.isnan(e2)) and torch.equal(torch.nan_to_num(e1), torch.nan_to_num(e2))
    assert abs(float(v) - q.loss_o) <= TOL * q.loss_o              # ... and the loss the model is trained on, from the same forward


def test_a_checkpoint_carries_the_patience_counter():
    from windgnn_amd.trainer import TrainStep
    q = _checked(BASE)
    A, Xs, Ls = _device_inputs(q)
    train, held = _split(q)
    model = _model_of(q.r)
    tr = TrainStep(model, keep_best=True, best_on="validation")
    assert list(tr.state_dict()) == ["optimizer", "steps", "best", "carry"]
    tr.step_series(A, Xs, Ls, q.T, starts=train)
    for _ in range(3):                                              # one win, then two passes on the same parameters
        tr.validate_series(A, Xs, Ls, q.T, starts=held)
    assert (int(tr.val_stale), int(tr.val_passes)) == (2, 3)
    far = Ls + 3.0                                                  # labels 3 away: a mean square of about 10, which cannot win
    tr.validate_series(A, Xs, far, q.T, starts=held[:4], more=True)
    with pytest.raises(RuntimeError, match="a validation pass is open"):
        tr.state_dict()
    assert float(tr.validate_series(A, Xs, far, q.T, starts=held[4:])) > 4.0 > float(tr.best_loss)
    sd = tr.state_dict()
    assert list(sd)[-1] == "val" and int(sd["val"]["stale"]) == 3 and int(sd["val"]["passes"]) == 4
    model2 = _model_of(q.r)
    model2.load_state_dict(model.state_dict())
    tr2 = TrainStep(model2, keep_best=True, best_on="validation")
    tr2.load_state_dict(sd)
    assert (int(tr2.val_stale), int(tr2.val_passes), int(tr2.best_step)) == (3, 4, 1)
    assert torch.equal(tr2.val_loss, tr.val_loss) and int(tr2.val_count) == int(tr.val_count)
    for t in (tr, tr2):                                             # both go on alike: no win, then a step and a win
        t.validate_series(A, Xs, Ls, q.T, starts=held)
        assert int(t.val_stale) == 4
        t.step_series(A, Xs, Ls, q.T, starts=train)
        t.validate_series(A, Xs, Ls, q.T, starts=held)
        assert (int(t.val_stale), int(t.best_step), int(t.val_passes)) == (0, 2, 6)
    assert torch.equal(tr.val_loss, tr2.val_loss) and torch.equal(tr._best_p, tr2._best_p)


@pytest.mark.parametrize("how", ["table", "stride2"])
def test_validate_series_launches_the_forward_of_the_floor_and_a_finish(how):
    """The launched names: forward_last_series' own, with the recurrence's `lossfn` instance in the place of the plain one, plus
    the finish and the record's launches -- and with best_on="validation" wgnn_keep_best's two.  No BPTT, no fold, no GEMM or
    reduction of a backward."""
    from windgnn_amd import _lib as L
    from windgnn_amd.series import forward_last_series
    from windgnn_amd.trainer import TrainStep
    q = _checked("irregular-%s-e-l1-from2" % how)
    A, Xs, Ls = _device_inputs(q)
    model = _model_of(q.r)
    tr = TrainStep(model, keep_best=True, best_on="validation")
    kw = {"starts": q.starts} if q.stride is None else {"stride": q.stride, "n_windows": q.n}
    tr.validate_series(A, Xs, Ls, q.T, loss="l1", loss_from=2, **kw)      # (the images and the record exist from here on)

    def launched(call):
        L.profile_enable(True)
        try:
            call()
            torch.cuda.synchronize()
            return [rec["name"] for rec in L.profile_read() for _ in range(rec["launches"])]
        finally:
            L.profile_enable(False)
    floor = launched(lambda: forward_last_series(model, A, Xs, q.T, 0.0, 1.0, **kw))
    names = launched(lambda: tr.validate_series(A, Xs, Ls, q.T, loss="l1", loss_from=2, **kw))
    tag = ",starts" if q.stride is None else ""
    plain, spec = "gru_fwd_kernel<%d%s>" % (sc.fwd_ks(q.H), tag), "gru_fwd_kernel<%d%s,lossfn>" % (sc.fwd_ks(q.H), tag)
    assert plain in floor and spec not in floor
    want = [spec if x == plain else x for x in floor] + ["val_begin_kernel", "series_val_finish_kernel", "best_decide_kernel",
                                                         "best_copy_kernel", "val_close_kernel"]
    assert sorted(names) == sorted(want), (names, want)
    assert not [x for x in names if x.startswith(BACKWARD)], names
