"""compact= on the MI355X: every series call that takes starts=, run on the covered hours only (series.compact_table), against the
fp64 oracle on the MATERIALISED windows at the series suites' bar -- conftest.rel_to_max <= 1e-4 on Y, the last rows and each of
the 8 gradients, the loss relative to the oracle's -- and against the compact=False call at the same bar (the observed difference
is printed; bit identity is not required: the weight-gradient sums are grouped over another row count, and a front layout on the
other side of 4096 rows takes the other GEMM instance).

Inputs are drawn as series_at_cases.reference draws them (test_gpu_series._draw with the seed of the case, the label series random
in [0, 1) with 1e3 in every row no window covers).  tests/test_series_compact_host.py has shown on the CPU that the index
arithmetic of the device path cannot leave its tensors for any table, so the bad-table case here provokes nothing.

Shapes, the smallest at which each thing can go wrong:
  small   S 7, H 21, T 5, rows 120, n 7: duplicates, an overlap of T - 1, both ends, far-apart segments
  wg16    S 7, H 21, T 3, rows 36, n 17 sparse: the 16-window workgroup boundary of the recurrences
  real    S 34, H 102, T 24, rows 400, n 6: the reference's widths
  gemm    S 34, H 102, T 24, rows 4200, n 20: the uncompacted front layout is above 4096 rows, the compacted one has 480"""
import functools

import pytest
import torch

import series_lossfn_cases as lc
import test_gpu_streams as gs
from conftest import PARAM_KEYS, rel_to_max
from series_at_cases import covered_rows, windows_at
from test_gpu_series import TOL, WIND_MAX, WIND_MIN, _dev, _draw, preact_margin
from test_gpu_series_train import SPARE
from test_gpu_series_train import TOL as LOSS_TOL
from test_gpu_streams import side  # noqa: F401  (the fixture)

pytestmark = pytest.mark.gpu

WINDOW_START = 16
# id -> (S, H, rows, T, starts, seed, cover_bound of the device-table run or None for min(rows, n * T))
SHAPES = {
    "small": (7, 21, 120, 5, (0, 0, 3, 40, 41, 100, 115), 1, None),
    "wg16": (7, 21, 36, 3, (0, 0, 0, 1, 1, 5, 5, 5, 12, 12, 13, 20, 20, 20, 21, 33, 33), 1, 20),      # 18 hours are covered
    "real": (34, 102, 400, 24, (0, 10, 10, 200, 300, 376), 20, None),
    "gemm": (34, 102, 4200, 24, tuple(range(100, 4100, 200)), 346, None),
}


class Ref:
    pass


@functools.lru_cache(maxsize=None)
def _ref(sid):
    """Host tensors of a shape and the fp64 oracle's results on the materialised windows: computed once, shared, never modified."""
    from oracle import windgnn_oracle as orc
    S, H, rows, T, starts, seed, bound = SHAPES[sid]
    n = len(starts)
    assert all(0 <= s <= rows - T for s in starts) and list(starts) == sorted(starts)
    r = Ref()
    r.id, r.S, r.H, r.rows, r.T, r.n, r.starts, r.bound = sid, S, H, rows, T, n, list(starts), bound
    r.A, r.feat, r.dY, r.p = _draw(S, H, rows, T, 1, n, seed)
    r.Xs = r.feat[:rows].contiguous()
    g = torch.Generator().manual_seed(7700 + 131 * seed + S * 7 + rows + H)
    r.Ls = torch.rand(rows, H, generator=g)
    r.hit = covered_rows(rows, T, starts)
    r.m = int(r.hit.sum())
    r.Ls[~r.hit] = SPARE
    r.X, r.L = windows_at(r.Xs, T, starts), windows_at(r.Ls, T, starts)
    A, X, r.p64 = r.A.double(), r.X.double(), {k: v.double() for k, v in r.p.items()}
    # the margin of the hours a window covers: the others enter no result (seeds searched on the CPU: 0 .. 59, gemm 0 .. 399)
    r.margin = preact_margin(A, r.Xs[r.hit].double().unsqueeze(0), r.p64)
    assert r.margin > 1e-5, "a ReLU pre-activation within %.1e of zero (relative): pick another seed" % r.margin
    r.Yo, r.cache = orc.forward(A, X, r.p64)
    r.last_o = r.Yo[:, -1, :] * (WIND_MAX - WIND_MIN) + WIND_MIN
    _, loss, r.gm = orc.train_step(A, X, r.L.double(), r.p64)
    r.loss_o = float(loss)
    r.rows_dev = min(rows, n * T if bound is None else bound)
    assert r.m < r.rows_dev < rows or (r.m <= r.rows_dev < rows and sid == "gemm")      # the device table has padding rows
    return r


def _model_of(r):
    from windgnn_amd import GCN_GRU
    m = GCN_GRU(13, 13, 13, r.S * 13, r.H, math="f32")
    m.load_state_dict({k: v.clone() for k, v in r.p.items()})
    return m.to(_dev())


def _step_of(r, **kw):
    from windgnn_amd.trainer import TrainStep
    model = _model_of(r)
    return TrainStep(model, **kw), model


def _on_dev(r, Ls=None):
    dev = _dev()
    return r.A.to(dev), r.Xs.to(dev), (r.Ls if Ls is None else Ls).to(dev)


def _tables(r):
    """The two forms of the table and the compact= each goes with: a host list, and a device tensor (with its cover_bound)."""
    return (("host", list(r.starts), True),
            ("device", torch.tensor(r.starts, dtype=torch.int64, device=_dev()), True if r.bound is None else r.bound))


def _assert_bar(what, err):
    print("\n%s: " % what + "  ".join("%s %.2e" % kv for kv in err.items()))
    for k, e in err.items():
        assert e <= (LOSS_TOL if k.startswith("loss") else TOL), (what, k, e)


def _grads(tr, model):
    return {k: q.clone().cpu() for k, q in zip(PARAM_KEYS, tr.g_views)}


def _fb(r, starts, compact, **kw):
    tr, model = _step_of(r)
    A, Xs, Ls = _on_dev(r, kw.pop("Ls", None))
    loss, Y = tr.forward_backward_series(A, Xs, Ls, r.T, starts=starts, compact=compact, **kw)
    return float(loss), Y.cpu(), _grads(tr, model), tr


# ---- forward_backward_series: the oracle, and the uncompacted call -----------------------------------------------------------------
@pytest.mark.parametrize("sid", list(SHAPES))
def test_compacted_forward_backward_matches_the_oracle_and_the_uncompacted_call(sid):
    from windgnn_amd.functional import check_range_status
    r = _ref(sid)
    loss0, Y0, g0, _ = _fb(r, list(r.starts), False)
    for form, table, compact in _tables(r):
        loss, Y, g, _ = _fb(r, table, compact)
        err = {"Y": rel_to_max(Y, r.Yo), "loss": abs(loss - r.loss_o) / r.loss_o}
        err.update({k: rel_to_max(g[k], r.gm[k]) for k in PARAM_KEYS})
        _assert_bar("%s, %s table, compact=%r vs the oracle" % (sid, form, compact), err)
        diff = {"Y": rel_to_max(Y, Y0), "loss": abs(loss - loss0) / loss0}
        diff.update({k: rel_to_max(g[k], g0[k]) for k in PARAM_KEYS})
        _assert_bar("%s, %s table, compact=%r vs compact=False" % (sid, form, compact), diff)
        if sid != "gemm":      # the same front GEMM instance on both sides: the recurrences see the same GI bits
            assert torch.equal(Y, Y0)
    check_range_status(_dev())


def test_the_compacted_call_runs_the_front_end_on_rows_c_rows():
    """By the launched kernels' work: the profiler's records of the two calls differ in the front kernels' sizes alone, and the
    compacted call's stash and workspace are those of a series of rows_c rows."""
    import ctypes as C
    from windgnn_amd import _lib as L
    r = _ref("small")
    lib = L.load()
    sizes = {}
    for rows in (r.rows, r.m, r.rows_dev):
        sd = L.SeriesDims(rows, r.T, 0, r.n, r.S, 13, r.H, 0, 0, 0, 0)
        sizes[rows] = (lib.wgnn_series_at_stash_bytes(C.byref(sd)), lib.wgnn_series_at_workspace_bytes(C.byref(sd)))
    assert sizes[r.m][0] < sizes[r.rows_dev][0] < sizes[r.rows][0] and sizes[r.m][1] <= sizes[r.rows][1]
    names = {}
    for compact in (False, True):
        L.profile_enable(True)
        try:
            _fb(r, list(r.starts), compact)
            torch.cuda.synchronize()
            names[compact] = [rec["name"] for rec in L.profile_read()]
        finally:
            L.profile_enable(False)
    assert names[True] == names[False] and "series_fold_at_kernel" in names[True], (names[True], names[False])


# ---- step_series: three Adam steps -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", ["small", "wg16"])
def test_three_compacted_steps_follow_the_oracle_trajectory(sid):
    from oracle import windgnn_oracle as orc
    r = _ref(sid)
    p, losses_o = dict(r.p64), []
    state = orc.adam_init(p)
    for _ in range(3):
        _, loss, g = orc.train_step(r.A.double(), r.X.double(), r.L.double(), p)
        losses_o.append(float(loss))
        p = orc.adam_step(p, g, state)
    perm = torch.randperm(r.n, generator=torch.Generator().manual_seed(6)).tolist()
    shuffled = [r.starts[i] for i in perm]
    for form, table, compact in (("host", shuffled, True),
                                 ("device", torch.tensor(shuffled, device=_dev()), True if r.bound is None else r.bound)):
        tr, model = _step_of(r)
        A, Xs, Ls = _on_dev(r)
        seen = {}
        for i in range(3):
            loss, Y = tr.step_series(A, Xs, Ls, r.T, starts=table, compact=compact)
            assert tuple(Y.shape) == (r.n, r.T, r.H)
            seen["loss%d" % (i + 1)] = abs(float(loss) - losses_o[i]) / losses_o[i]
        assert tr.steps == 3
        seen.update({k: rel_to_max(q.detach().cpu(), p[k]) for k, q in model.named_parameters()})
        _assert_bar("%s, step_series x3, %s table" % (sid, form), seen)


# ---- L1 / Huber with missing labels ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,delta,t_from", [("l1", 1.0, 2), ("huber", 0.25, 0)])
@pytest.mark.parametrize("sid", ["small", "wg16"])
def test_l1_and_huber_with_missing_labels_count_the_oracles_labels(sid, kind, delta, t_from):
    from oracle import windgnn_oracle as orc
    r = _ref(sid)
    g = torch.Generator().manual_seed(41 + r.rows)
    Ls = r.Ls.clone()
    Ls[(torch.rand(Ls.shape, generator=g) < 0.1) & r.hit[:, None]] = float("nan")
    L = windows_at(Ls, r.T, r.starts)
    loss_o, dY, m = lc.loss_and_dy(r.Yo, L.double(), kind, delta, t_from, True)
    assert 0 < m < r.n * (r.T - t_from) * r.H
    go = orc.backward(r.A.double(), r.X.double(), r.p64, r.Yo, r.cache, dY)
    for form, table, compact in _tables(r):
        loss, Y, grads, tr = _fb(r, table, compact, Ls=Ls, missing_labels=True, loss=kind, huber_delta=delta, loss_from=t_from)
        err = {"Y": rel_to_max(Y, r.Yo), "loss": abs(loss - float(loss_o)) / float(loss_o)}
        err.update({k: rel_to_max(grads[k], go[k]) for k in PARAM_KEYS})
        _assert_bar("%s, %s from %d, masked, %s table" % (sid, kind, t_from, form), err)
        # the counted labels: accumulate_series weighs the call by them, a device integer
        tr2, _ = _step_of(r)
        A, Xs, Ld = _on_dev(r, Ls)
        tr2.accumulate_series(A, Xs, Ld, r.T, starts=table, compact=compact, missing_labels=True, loss=kind, huber_delta=delta,
                              loss_from=t_from)
        assert int(tr2.accumulated_count) == m
        tr2.discard()


# ---- validate_series, forward_last_series, Evaluator ----------------------------------------------------------------------------------
@pytest.mark.parametrize("sid", ["small", "real"])
def test_validate_series_counts_exactly_and_means_within_the_bar(sid):
    r = _ref(sid)
    A, Xs, Ls = _on_dev(r)
    for form, table, compact in _tables(r):
        tr, _ = _step_of(r)
        val = float(tr.validate_series(A, Xs, Ls, r.T, starts=table, compact=compact))
        assert int(tr.val_count) == r.n * r.T * r.H
        tr0, _ = _step_of(r)
        val0 = float(tr0.validate_series(A, Xs, Ls, r.T, starts=table))
        _assert_bar("%s, validate_series, %s table" % (sid, form), {"loss": abs(val - r.loss_o) / r.loss_o,
                                                                   "loss_vs_uncompacted": abs(val - val0) / val0})


@pytest.mark.parametrize("sid", ["small", "real"])
def test_forward_last_series_and_the_evaluator(sid):
    from windgnn_amd.evaluate import Evaluator
    from windgnn_amd.series import forward_last_series
    r = _ref(sid)
    A, Xs, Ls = _on_dev(r)
    model = _model_of(r)
    perm = torch.randperm(r.n, generator=torch.Generator().manual_seed(3)).tolist()
    shuffled = [r.starts[i] for i in perm]
    with torch.no_grad():
        for form, table, compact in (("host", shuffled, True),
                                     ("device", torch.tensor(shuffled, device=_dev()), True if r.bound is None else r.bound)):
            last = forward_last_series(model, A, Xs, r.T, WIND_MIN, WIND_MAX, starts=table, compact=compact).cpu()
            last0 = forward_last_series(model, A, Xs, r.T, WIND_MIN, WIND_MAX, starts=table).cpu()
            _assert_bar("%s, forward_last_series, %s table" % (sid, form), {"last": rel_to_max(last, r.last_o[perm]),
                                                                          "last_vs_uncompacted": rel_to_max(last, last0)})
            ev, ev0 = Evaluator(model, A, WIND_MIN, WIND_MAX), Evaluator(model, A, WIND_MIN, WIND_MAX)
            ev.update_series(Xs, Ls, r.T, starts=table, compact=compact)
            ev0.update_series(Xs, Ls, r.T, starts=table)
            acc, acc0 = ev._acc().cpu(), ev0._acc().cpu()
            _assert_bar("%s, Evaluator accumulator, %s table" % (sid, form), {"acc": rel_to_max(acc, acc0)})
    Y = model.forward_series(A, Xs, r.T, starts=shuffled, compact=True)
    Y.backward(r.dY[perm].to(_dev()))
    from oracle import windgnn_oracle as orc
    go = orc.backward(r.A.double(), r.X.double(), r.p64, r.Yo, r.cache, r.dY.double())
    err = {"Y": rel_to_max(Y.detach().cpu(), r.Yo[perm])}
    err.update({k: rel_to_max(q.grad.cpu(), go[k]) for k, q in model.named_parameters()})
    _assert_bar("%s, GCN_GRU.forward_series(compact=True) through autograd" % sid, err)


# ---- accumulate_series from two tables, then apply ------------------------------------------------------------------------------
def test_two_compacted_tables_accumulate_to_the_step_on_their_union():
    from oracle import windgnn_oracle as orc
    r = _ref("small")
    A, Xs, Ls = _on_dev(r)
    p = dict(r.p64)
    _, loss_o, g = orc.train_step(r.A.double(), r.X.double(), r.L.double(), p)
    po = orc.adam_step(p, g, orc.adam_init(p))
    first, second = r.starts[:3], r.starts[3:]
    tr, model = _step_of(r)
    tr.accumulate_series(A, Xs, Ls, r.T, starts=first, compact=True)
    tr.accumulate_series(A, Xs, Ls, r.T, starts=torch.tensor(second, device=_dev()), compact=True)
    loss = tr.apply()
    loss = float(loss[0] if isinstance(loss, tuple) else loss)
    err = {"loss": abs(loss - float(loss_o)) / float(loss_o)}
    err.update({k: rel_to_max(q.detach().cpu(), po[k]) for k, q in model.named_parameters()})
    _assert_bar("accumulate_series x2 (compact=True) + apply", err)


# ---- an Ensemble on two folds ------------------------------------------------------------------------------------------------------
def test_an_ensemble_on_two_folds_is_its_members_driven_alone_bit_for_bit():
    from windgnn_amd.ensemble import Ensemble, PerMember
    from windgnn_amd.series import kfold_starts
    r = _ref("small")
    A, Xs, Ls = _on_dev(r)
    folds = kfold_starts(r.starts, 2, r.T, horizon=0)
    trains = [f[0].tolist() for f in folds]
    assert all(len(t) >= 1 for t in trains) and trains[0] != trains[1]

    def members():
        return [_step_of(r)[0] for _ in range(2)]
    alone = members()
    want = []
    for k, tr in enumerate(alone):
        for _ in range(2):
            loss, Y = tr.step_series(A, Xs, Ls, r.T, starts=trains[k], compact=True)
        want.append((loss.clone().cpu(), Y.cpu(), tr.flat_p.clone().cpu()))
    ens = Ensemble([_model_of(r) for _ in range(2)])
    for _ in range(2):
        out = ens.step_series(A, Xs, Ls, r.T, starts=PerMember(trains), compact=True)
    torch.cuda.synchronize()
    for k, (loss, Y) in enumerate(out):
        assert torch.equal(loss.cpu(), want[k][0]) and torch.equal(Y.cpu(), want[k][1]), k
        assert torch.equal(ens.members[k].flat_p.cpu(), want[k][2]), k


# ---- a bad device table stays a reported error ------------------------------------------------------------------------------------
def test_a_device_table_with_a_start_past_the_end_is_reported_and_the_next_call_passes():
    from windgnn_amd.functional import check_range_status
    r = _ref("small")
    A, Xs, Ls = _on_dev(r)
    dev = _dev()
    check_range_status(dev)
    bad = list(r.starts)
    bad[-1] = r.rows - r.T + 1
    tr, _ = _step_of(r)
    tr.forward_backward_series(A, Xs, Ls, r.T, starts=torch.tensor(bad, device=dev), compact=True)
    with pytest.raises(RuntimeError, match=r"window starts"):
        check_range_status(dev)
    check_range_status(dev)                                               # reported once
    tr.forward_backward_series(A, Xs, Ls, r.T, starts=torch.tensor(r.starts, device=dev), compact=r.m - 1)   # a bound too small
    with pytest.raises(RuntimeError, match=r"window starts"):
        check_range_status(dev)
    loss, Y = tr.forward_backward_series(A, Xs, Ls, r.T, starts=torch.tensor(r.starts, device=dev), compact=True)
    check_range_status(dev)
    _assert_bar("the good call after the bad ones", {"Y": rel_to_max(Y.cpu(), r.Yo), "loss": abs(float(loss) - r.loss_o) / r.loss_o})


# ---- no synchronisation ------------------------------------------------------------------------------------------------------------
def _sc_step_series_compact(py):
    """tests/test_gpu_streams.py's step_series scenario with a DEVICE table and compact=30: rows_c = 30 of the 43 / 31 rows, of
    which 16 / 28 are covered, so the compacted series has padding rows."""
    from windgnn_amd.trainer import TrainStep
    T = py.dims[1]
    tr = TrainStep(py.model("f32"))
    table = torch.tensor([4, 0, 0], device=_dev())

    def run(i):
        out = {}
        for k in range(2):
            loss, Y = tr.step_series(i["A"], i["Xs"], i["Ls"], T, starts=table, compact=30)
            out["loss%d" % k], out["Y%d" % k] = loss.clone(), Y.clone()
        return dict(out, **gs._trainer_outputs(tr))
    return run


@pytest.mark.parametrize("size", list(gs.PY_SIZES))
def test_a_compacted_device_table_step_behind_a_blocker_gives_the_default_streams_bits(size, side, monkeypatch):  # noqa: F811
    monkeypatch.setitem(gs.SCENARIOS, "step_series_compact",
                        (_sc_step_series_compact, True, "series.compact_table: 'no host read and no data-dependent shape'"))
    assert all(gs.PY_SIZES[s][1] + gs.PY_SIZES[s][2] - 1 > 30 for s in gs.PY_SIZES)      # rows > rows_c: rows are dropped
    gs.test_python_layer_on_a_side_stream_behind_a_blocker("step_series_compact", size, side)
