"""Series tables on the covered hours only, without a GPU: series.compact_table through both of its code paths -- numpy for a host
table, torch operations for a device table, run here on CPU tensors (device="cpu"), which is exactly the arithmetic the GPU runs
-- against a brute-force construction; the bad device tables, which must come out as -1 entries and never as an index error; the
refusals of compact= by name; and, on the recorders of tests/test_trainstep_schedule_host.py and tests/test_series_val_host.py,
the raw calls the trainer issues with compact=False (today's), with compact=True on a fully covered table (today's) and with
compact=True on a sparse table (the same sequence on rows_c rows)."""
import numpy as np
import pytest
import torch

import series_at_cases as sc
import test_series_val_host as sv
import test_trainstep_schedule_host as ts

# (rows, T, starts): the shared tables, then tables built to break a wrong rank
TABLES = {
    "small": (36, 3, sc.SMALL_TABLE),
    "irregular": (sc.IRREGULAR[2], sc.IRREGULAR[3], sc.IRREGULAR[4]),
    "big": (272, 16, sc.BIG_TABLE),
    "duplicates": (30, 4, (5, 5, 5, 12, 12)),
    "overlap_T-1": (30, 5, (3, 4, 5, 6, 7)),
    "far_apart": (70, 5, (10, 60)),                    # two segments that become adjacent when compacted
    "both_ends": (50, 5, (0, 45)),                     # the first and the last legal start
    "single": (20, 5, (7,)),
    "covers_all": (12, 4, (0, 2, 4, 6, 8)),            # rows_c == rows
}


def _brute(rows, T, starts):
    """(C, table): the ascending covered hours and each start's rank among them, by sets and list.index."""
    C = sorted({s + t for s in starts for t in range(T)})
    return C, [C.index(s) for s in starts]


def _depth(starts, T, rows):
    from windgnn_amd.series import starts_coverage
    cov = starts_coverage(starts, T, rows)
    return cov[:, 1] - cov[:, 0]


def _as_int(t):
    return t.contiguous().view(torch.int32)


def _check(rows, T, starts, ct, rows_c, device_path):
    C, ranks = _brute(rows, T, starts)
    m, n = len(C), len(starts)
    assert ct.rows_c == rows_c and isinstance(ct.rows_c, int)
    assert ct.hours.dtype == torch.int64 and tuple(ct.hours.shape) == (rows_c,)
    assert ct.table.dtype == torch.int32 and tuple(ct.table.shape) == (n,)
    if device_path:
        assert isinstance(ct.covered, torch.Tensor) and ct.covered.dim() == 0 and int(ct.covered) == m
    else:
        assert isinstance(ct.covered, int) and ct.covered == m
    hours, table = ct.hours.tolist(), ct.table.tolist()
    assert hours[:m] == C and hours[m:] == [C[0]] * (rows_c - m)          # the padding repeats a real hour
    assert table == ranks and all(a <= b for a, b in zip(table, table[1:]))
    for w, s in enumerate(starts):
        assert table[w] + T <= m                                           # no window covers a padding row
        for t in range(T):
            assert hours[table[w] + t] == s + t, (w, t)
    depth_c, depth = _depth(table, T, rows_c), _depth(starts, T, rows)
    assert np.array_equal(depth_c[:m], depth[C]) and not depth_c[m:].any()
    # the materialised windows: bit-equal, NaN labels included
    g = torch.Generator().manual_seed(rows * 31 + T)
    series, Ls = torch.rand(rows, 3, 13, generator=g), torch.rand(rows + 2, 5, generator=g)
    Ls[torch.rand(rows + 2, 5, generator=g) < 0.2] = float("nan")
    series_c, Ls_c = ct.apply(series, Ls)
    assert tuple(series_c.shape) == (rows_c, 3, 13) and tuple(Ls_c.shape) == (rows_c, 5)
    assert torch.equal(_as_int(sc.windows_at(series_c, T, table)), _as_int(sc.windows_at(series, T, starts)))
    assert torch.equal(_as_int(sc.windows_at(Ls_c, T, table)), _as_int(sc.windows_at(Ls, T, starts)))
    assert torch.isnan(sc.windows_at(Ls, T, starts)).any() or n * T < 10


@pytest.mark.parametrize("tid", list(TABLES))
@pytest.mark.parametrize("form", ["list", "numpy", "tensor"])
def test_host_path_compacts_to_exactly_the_covered_hours(tid, form):
    from windgnn_amd.series import compact_table
    rows, T, starts = TABLES[tid]
    arg = {"list": list(starts), "numpy": np.asarray(starts, dtype=np.int64), "tensor": torch.tensor(starts, dtype=torch.int32)}[form]
    ct = compact_table(arg, rows, T)
    _check(rows, T, starts, ct, len(_brute(rows, T, starts)[0]), device_path=False)
    assert (ct.rows_c == rows) == (tid in ("covers_all", "big"))      # (the big table leaves no hour out either)


@pytest.mark.parametrize("tid", list(TABLES))
@pytest.mark.parametrize("bound", ["default", "exact", "loose"])
def test_device_path_on_cpu_tensors_compacts_to_the_bound(tid, bound):
    from windgnn_amd.series import compact_table
    rows, T, starts = TABLES[tid]
    m = len(_brute(rows, T, starts)[0])
    cover_bound = {"default": None, "exact": m, "loose": m + 3}[bound]
    rows_c = min(rows, len(starts) * T if cover_bound is None else cover_bound)
    for dtype in (torch.int32, torch.int64):
        ct = compact_table(torch.tensor(starts, dtype=dtype), rows, T, cover_bound, device="cpu")
        _check(rows, T, starts, ct, rows_c, device_path=True)
    assert rows_c >= m


BAD = {"negative": (40, 5, (-3, 4, 9, 30), None, {0}),
       "past_the_end": (40, 5, (2, 4, 9, 36), None, {3}),                   # rows - T + 1
       "int32_max": (40, 5, (2, 4, 9, 2 ** 31 - 1), None, {3}),
       "int64_far": (40, 5, (-2 ** 40, 4, 9, 2 ** 40), None, {0, 3}),
       "bound_one_short": (70, 5, (10, 11, 60), 10, {2}),                    # 11 hours are covered
       "all_bad": (40, 5, (-1, 36), None, {0, 1})}


@pytest.mark.parametrize("bid", list(BAD))
def test_bad_device_tables_give_minus_one_entries_and_no_exception(bid):
    """The good windows keep the ranks they have in the table of the good windows alone; every bad one gets -1; hours holds real
    rows of the series only, so the gather that follows cannot leave it (an out-of-range index is an IndexError on the CPU)."""
    from windgnn_amd.series import compact_table
    rows, T, starts, cover_bound, bad = BAD[bid]
    dtype = torch.int64 if bid == "int64_far" else torch.int32
    ct = compact_table(torch.tensor(starts, dtype=dtype), rows, T, cover_bound, device="cpu")
    in_range = [s for s in starts if 0 <= s <= rows - T]
    C, _ = _brute(rows, T, in_range) if in_range else ([0], [])
    rows_c = min(rows, len(starts) * T if cover_bound is None else cover_bound)
    assert ct.rows_c == rows_c and tuple(ct.hours.shape) == (rows_c,)
    hours, table = ct.hours.tolist(), ct.table.tolist()
    assert int(ct.covered) == (len(C) if in_range else 0)
    assert all(0 <= h < rows for h in hours)
    assert hours == (C + [C[0]] * rows_c)[:rows_c]
    for w, s in enumerate(starts):
        if w in bad:
            assert table[w] == -1, (w, table)
        else:
            assert table[w] == C.index(s) and hours[table[w]:table[w] + T] == list(range(s, s + T))
    ct.apply(torch.rand(rows, 2, 13), torch.rand(rows, 4))                    # in range: no IndexError
    if bid == "bound_one_short":
        with pytest.raises(ValueError, match=r"covers 11 hours, more than cover_bound=10"):      # the host knows, and says so
            compact_table(list(starts), rows, T, cover_bound)


def test_compact_table_refuses_what_starts_table_refuses():
    from windgnn_amd.series import compact_table
    with pytest.raises(ValueError, match=r"starts\[1\] = 36"):
        compact_table([2, 36], 40, 5)
    with pytest.raises(ValueError, match=r"non-decreasing"):
        compact_table([4, 2], 40, 5)
    with pytest.raises(ValueError, match=r"integers"):
        compact_table([0.5], 40, 5)
    with pytest.raises(ValueError, match=r"empty"):
        compact_table([], 40, 5)
    with pytest.raises(ValueError, match=r"no window of 5 rows fits into a series of 4 rows"):
        compact_table([0], 4, 5)
    for bad in (4, 0, -1, 7.5, True):
        with pytest.raises(ValueError, match=r"cover_bound=.*>= seq_len = 5"):
            compact_table([0], 40, 5, bad)
    with pytest.raises(ValueError, match=r"1-D int32 / int64 tensor"):
        compact_table(torch.tensor([0.0]), 40, 5, device="cpu")


# ---- compact= by name, before any launch ------------------------------------------------------------------------------------------
A, SERIES, LS = torch.rand(7, 7), torch.rand(40, 7, 13), torch.rand(40, 21)


def _model():
    import windgnn_amd
    return windgnn_amd.GCN_GRU(13, 13, 13, 7 * 13, 21)


def _entry_points():
    from windgnn_amd.evaluate import Evaluator
    from windgnn_amd.series import forward_last_series
    from windgnn_amd.trainer import TrainStep
    model = _model()
    calls = {}
    for name in ("step_series", "forward_backward_series", "validate_series", "accumulate_series"):
        calls["TrainStep." + name] = lambda name=name, **kw: getattr(TrainStep(_model()), name)(A, SERIES, LS, 5, **kw)
    calls["GCN_GRU.forward_series"] = lambda **kw: model.forward_series(A, SERIES, 5, **kw)
    calls["forward_last_series"] = lambda **kw: forward_last_series(model, A, SERIES, 5, 0.0, 1.0, **kw)
    ev = Evaluator(model, A, 0.0, 1.0)
    calls["Evaluator.update_series"] = lambda **kw: ev.update_series(SERIES, LS, 5, **kw)
    return calls


@pytest.mark.parametrize("who", ["TrainStep.step_series", "TrainStep.forward_backward_series", "TrainStep.validate_series",
                                 "TrainStep.accumulate_series", "GCN_GRU.forward_series", "forward_last_series",
                                 "Evaluator.update_series"])
def test_compact_is_refused_by_name_without_a_table_and_with_a_stride(who, monkeypatch):
    from windgnn_amd import series as ser
    call = _entry_points()[who]
    launched = []
    monkeypatch.setattr(ser, "_series_setup", lambda *a, **kw: launched.append(a))
    for compact in (True, "auto", 48):
        with pytest.raises(ValueError, match=r"compact=%r belongs to starts=.*no table of starts" % (compact,)):
            call(compact=compact)
        with pytest.raises(ValueError, match=r"compact=%r belongs to starts=.*stride=2" % (compact,)):
            call(compact=compact, stride=2)
        with pytest.raises(ValueError, match=r"stride= or starts=, not both|compact=%r belongs to starts=.*stride=1" % (compact,)):
            call(compact=compact, stride=1, starts=[0, 3])
    for bad in ("yes", 2.5, [1]):
        with pytest.raises(ValueError, match=r"compact=.*False, True, 'auto', or an int"):
            call(compact=bad, starts=[0, 3])
    with pytest.raises(ValueError, match=r"compact=4: a table covers at least the seq_len = 5 hours"):
        call(compact=4, starts=[0, 3])
    with pytest.raises(ValueError, match=r"covers 8 hours, more than cover_bound=7"):        # a host table is checked on the host
        call(compact=7, starts=[0, 3])
    with pytest.raises(ValueError, match=r"starts\[1\] = 36"):
        call(compact=True, starts=[0, 36])
    assert launched == []


# ---- the raw calls on the recorders ---------------------------------------------------------------------------------------------
SPARSE = [30, 2, 2, 11]            # any order, a duplicate: hours 2-6, 11-15, 30-34 -> 15 rows of 40
DENSE = list(range(0, 36, 5)) + [35]      # covers every one of the 40 hours
H = 21


def _trainer_on_recorders(monkeypatch):
    """The schedule suite's recorders; the two series calls also tell the rows of the series and the label series they got and
    the table (today's recorders take no table and would raise on one)."""
    from windgnn_amd import trainer
    rec = ts.Recorder()
    for name, fn in ts._bindings(rec, H).items():
        monkeypatch.setattr(trainer, name, fn)

    def series_forward_loss_raw(A, series, Ls, seq_len, stride, params, math=0, n_windows=None, prepared=None, starts=None):
        assert prepared is not None and stride is None and n_windows is None and starts.dtype == torch.int32
        rec("series_forward_loss", series.shape[0], Ls.shape[0], starts.tolist())
        return torch.zeros(starts.numel(), seq_len, H), None, None, None, starts

    def series_backward_mse_raw(sd, A, series, params, Y, Ls, stash, loss_buf, grads, loss, grad_scale=1.0, prepared=None,
                                starts=None):
        assert prepared is not None
        rec("series_bwd_mse", series.shape[0], Ls.shape[0], starts.tolist(), grad_scale)

    monkeypatch.setattr(trainer, "series_forward_loss_raw", series_forward_loss_raw)
    monkeypatch.setattr(trainer, "series_backward_mse_raw", series_backward_mse_raw)
    tr = trainer.TrainStep(_model(), check_every=1)
    return tr, rec


def _events(rows, table, step):
    return ([("require_gpu",), ("images",), ("series_forward_loss", rows, rows, table), ("series_bwd_mse", rows, rows, table, 1.0)]
            + ([("finish", 0, step)] if step else []))


@pytest.mark.parametrize("form", ["list", "cpu_tensor"])
def test_step_series_issues_todays_calls_unless_there_are_rows_to_drop(monkeypatch, form):
    from windgnn_amd.series import COMPACT_AUTO_THETA
    as_arg = (lambda t: list(t)) if form == "list" else (lambda t: torch.tensor(t))
    today = {}
    for compact in (False, True, 64, "auto"):
        for name, starts in (("sparse", SPARSE), ("dense", DENSE)):
            tr, rec = _trainer_on_recorders(monkeypatch)
            loss, Y = tr.step_series(A, SERIES, LS, 5, starts=as_arg(starts), compact=compact)
            assert loss is tr._loss and tuple(Y.shape) == (len(starts), 5, H) and tr.steps == 1
            if compact is False:
                assert rec.events == _events(40, sorted(starts), 1)
                today[name] = list(rec.events)
            drops = name == "sparse" and (compact in (True, 64) or (compact == "auto" and 15 <= COMPACT_AUTO_THETA * 40))
            assert 0.0 <= COMPACT_AUTO_THETA < 1.0
            # the same sequence on rows_c = 15 rows; with nothing to drop, or "auto" above the measured threshold, today's
            assert rec.events == (_events(15, [0, 0, 5, 10], 1) if drops else today[name])
            tr.forward_backward_series(A, SERIES, LS, 5, starts=as_arg(starts), compact=compact)
            assert rec.events[-2:] == rec.events[2:4] and tr.steps == 1


def test_the_compacted_call_gets_the_covered_rows_and_gives_y_back_in_the_callers_order(monkeypatch):
    from windgnn_amd import trainer
    tr, rec = _trainer_on_recorders(monkeypatch)
    seen = {}
    inner = trainer.series_forward_loss_raw

    def fwd(A, series, Ls, seq_len, stride, params, math=0, n_windows=None, prepared=None, starts=None):
        seen["series"], seen["Ls"] = series, Ls
        out = inner(A, series, Ls, seq_len, stride, params, math, n_windows, prepared, starts)
        return (torch.arange(4.0).view(4, 1, 1).expand(4, seq_len, H).contiguous(),) + out[1:]
    monkeypatch.setattr(trainer, "series_forward_loss_raw", fwd)
    Ls = LS.clone()
    Ls[3, 2] = float("nan")
    _, Y = tr.accumulate_series(A, SERIES, Ls, 5, starts=SPARSE, compact=True, missing_labels=False)
    hours = list(range(2, 7)) + list(range(11, 16)) + list(range(30, 35))
    assert torch.equal(seen["series"], SERIES[hours]) and torch.equal(_as_int(seen["Ls"]), _as_int(Ls[hours]))
    assert seen["series"].is_contiguous() and seen["Ls"].is_contiguous()
    assert Y[:, 0, 0].tolist() == [3.0, 0.0, 1.0, 2.0]                       # SPARSE = [30, 2, 2, 11] sorts to rows 1, 2, 3, 0
    assert tr.accumulated == 1 and rec.events[2][:3] == ("series_forward_loss", 15, 15)


def test_validate_series_on_the_recorders(monkeypatch):
    from windgnn_amd import trainer
    for compact, starts, rows, table in ((False, SPARSE, 40, sorted(SPARSE)), (True, DENSE, 40, DENSE), (True, SPARSE, 15, [0, 0, 5, 10]),
                                         (20, SPARSE, 15, [0, 0, 5, 10])):
        rec = sv.Rec()
        sv._stubs(monkeypatch, rec)
        inner, got = trainer.series_val_raw, []

        def series_val_raw(A, series, params, Ls, seq_len, **kw):
            got.append((series.shape[0], Ls.shape[0]))
            return inner(A, series, params, Ls, seq_len, **kw)
        monkeypatch.setattr(trainer, "series_val_raw", series_val_raw)
        tr = sv._cpu_step()
        tr.validate_series(A, SERIES, LS, 5, starts=starts, compact=compact)
        assert got == [(rows, rows)]
        val = [e for e in rec.events if e[0] == "series_val"]
        assert len(val) == 1 and val[0][1:4] == (None, None, table)
        assert [e[0] for e in rec.events] == ["require_gpu", "images", "val_buffer", "val_begin", "series_val", "val_close"]


def test_forward_series_compacts_outside_the_autograd_function(monkeypatch):
    from windgnn_amd import series as ser
    got = []

    def gcn_gru_series(A, series, seq_len, stride, params, math=0, n_windows=None, starts=None):
        got.append((series.shape[0], stride, starts.tolist()))
        return torch.arange(float(starts.numel())).view(-1, 1, 1).expand(-1, seq_len, H)
    monkeypatch.setattr(ser, "gcn_gru_series", gcn_gru_series)
    model = _model()
    for compact, want in ((False, (40, None, sorted(SPARSE))), (True, (15, None, [0, 0, 5, 10])), ("auto", None)):
        Y = model.forward_series(A, SERIES, 5, starts=SPARSE, compact=compact)
        assert want is None or got[-1] == want
        assert Y[:, 0, 0].tolist() == [3.0, 0.0, 1.0, 2.0]
    assert model.forward_series(A, SERIES, 5, starts=DENSE, compact=True).shape[0] == len(DENSE) and got[-1] == (40, None, DENSE)


def test_ensemble_passes_compact_through_to_every_member():
    import inspect
    from windgnn_amd.ensemble import Ensemble
    from windgnn_amd.trainer import TrainStep
    for name in ("step_series", "forward_backward_series", "validate_series", "accumulate_series"):
        assert "compact" in inspect.signature(getattr(TrainStep, name)).parameters, name
    for name in ("step_series", "forward_backward_series", "validate_series"):
        assert any(p.kind is p.VAR_KEYWORD for p in inspect.signature(getattr(Ensemble, name)).parameters.values()), name
    assert "compact" in inspect.signature(Ensemble.forward_last_series).parameters
    assert "compact" in Ensemble.step_series.__doc__


def test_auto_compacts_a_host_table_below_theta_and_nothing_else(monkeypatch):
    """The measured rule (profiles/r22_series_compact_cost.txt): a host table that covers at most COMPACT_AUTO_THETA of the rows
    on a training call; never a device-side table (here: the device path's threshold), never a forward-only call."""
    from windgnn_amd import series as ser
    assert ser.COMPACT_AUTO_THETA == 0.37 and ser.COMPACT_AUTO_THETA_DEVICE == 0.0
    big = torch.rand(100, 7, 13)
    for starts, rows_c in (([3, 50], 10), ([0, 10, 20, 30, 40, 50, 60], 35), ([0, 10, 20, 30, 40, 50, 60, 70], 40)):
        s, _, table, _ = ser.compacted_starts(starts, big, None, 5, "x", "auto")
        assert s.shape[0] == (rows_c if rows_c <= 37 else 100), (starts, s.shape)
        assert ser.compacted_starts(starts, big, None, 5, "x", "auto", forward_only=True)[0] is big
        assert ser.compacted_starts(starts, big, None, 5, "x", True, forward_only=True)[0].shape[0] == rows_c
    monkeypatch.setattr(ser, "_is_device_table", lambda t: isinstance(t, torch.Tensor))      # a CPU tensor down the device path
    assert ser.compacted_starts(torch.tensor([3, 50]), big, None, 5, "x", "auto")[0] is big
    s, _, table, _ = ser.compacted_starts(torch.tensor([50, 3]), big, None, 5, "x", True)
    assert s.shape[0] == 10 and table.tolist() == [0, 5]
