"""Validation on materialised windows, the part that needs no GPU: functional.validation_terms (the loss arithmetic, defined
once in torch) against torch's own losses and the series suites' loss former, functional.val_add on a CPU record laid out by the
header's offsets, TrainStep.validate's refusals (each before any launch), and the three-step scenario of
tests/test_gpu_validate.py qualified on the fp64 oracle alone."""
import math

import pytest
import torch

import series_lossfn_cases as lc
import validate_cases as vc

OFFSETS = {"sum": (0, 8), "count": (8, 8), "mean": (16, 8), "max_abs": (24, 4), "loss": (28, 4), "calls": (32, 8),
           "passes": (40, 8), "stale": (48, 8)}          # include/windgnn_series_val.h, "PUBLIC"


def _draw(T=5, B=3, H=4, seed=3):
    g = torch.Generator().manual_seed(seed)
    Y = torch.rand(B, T, H, generator=g) * 2 - 1
    L = torch.rand(B, T, H, generator=g)
    hit = torch.rand(B, T, H, generator=g) < 0.25
    return Y, L, hit


@pytest.mark.parametrize("nan", [False, True])
@pytest.mark.parametrize("t_from", [0, 2, 4])
@pytest.mark.parametrize("kind", vc.KINDS)
def test_validation_terms_are_torchs_losses_and_the_series_suites(kind, t_from, nan):
    from windgnn_amd.functional import validation_terms
    Y, L, hit = _draw()
    if nan:
        L[hit] = float("nan")
    s, m, a = validation_terms(Y, L, kind, vc.DELTA, t_from, missing_labels=nan)
    assert (s.dtype, m.dtype, a.dtype) == (torch.float64, torch.int64, torch.float64) and s.dim() == m.dim() == a.dim() == 0
    on = lc.counted(L, t_from, nan)
    fn = {"mse": torch.nn.MSELoss(reduction="sum"), "l1": torch.nn.L1Loss(reduction="sum"),
          "huber": torch.nn.HuberLoss(reduction="sum", delta=vc.DELTA)}[kind]
    want = float(fn(Y.double()[on], L.double()[on]))
    assert int(m) == int(on.sum()) and 0 < int(m) < Y.numel() + (t_from == 0 and not nan)
    assert vc.rel(float(s), want) <= 1e-14
    assert float(a) == float((Y.double() - L.double())[on].abs().max())
    loss, _, m2 = lc.loss_and_dy(Y.double(), L.double(), kind, vc.DELTA, t_from, int(nan))
    assert m2 == int(m) and vc.rel(float(s) / int(m), float(loss)) <= 1e-14
    s3, m3, a3 = vc.terms(Y, L, kind, vc.DELTA, t_from, nan)                       # the GPU suite's own former agrees as well
    assert m3 == int(m) and vc.rel(float(s), s3) <= 1e-14 and a3 == float(a)


@pytest.mark.parametrize("kind", vc.KINDS)
def test_a_nan_label_outside_the_counted_set_changes_nothing_and_one_inside_poisons(kind):
    from windgnn_amd.functional import validation_terms
    Y, L, hit = _draw()
    clean = validation_terms(Y, L, kind, vc.DELTA, 2)
    early = L.clone()
    early[:, :2] = float("nan")                                  # before loss_from: sliced away
    for got, ref in zip(validation_terms(Y, early, kind, vc.DELTA, 2), clean):
        assert torch.equal(got, ref)
    holes = L.clone()
    holes[hit] = float("nan")
    filled = torch.where(hit, Y, L)                              # the same entries with r = 0 instead
    s, m, a = validation_terms(Y, holes, kind, vc.DELTA, 0, missing_labels=True)
    s0, m0, a0 = validation_terms(Y, filled, kind, vc.DELTA, 0)
    assert torch.equal(s, s0) and torch.equal(a, a0) and int(m) == int(m0) - int(hit.sum())
    s, m, a = validation_terms(Y, holes, kind, vc.DELTA, 0, missing_labels=False)
    assert math.isnan(float(s)) and math.isnan(float(a)) and int(m) == Y.numel()
    s, m, a = validation_terms(Y, torch.full_like(L, float("nan")), kind, vc.DELTA, 0, missing_labels=True)
    assert (float(s), int(m), float(a)) == (0.0, 0, 0.0)
    bad = Y.clone()
    bad[1, 3, 2] = float("nan")                                  # a NaN output is not a missing label
    assert math.isnan(float(validation_terms(bad, holes, kind, vc.DELTA, 0, missing_labels=True)[0]))


def test_the_chunk_rule_depends_on_the_shape_alone_and_chunks_add_up():
    from windgnn_amd import functional as F
    assert F.VALIDATION_CHUNK_BYTES == 64 << 20
    assert F.validation_chunk_windows(4096, 24, 102) == (64 << 20) // (24 * 102 * 8) == 3426
    assert F.validation_chunk_windows(5, 12, 21) == 5 and F.validation_chunk_windows(3, 1 << 20, 4096) == 1
    Y, L, hit = _draw(T=4, B=7, H=5)
    L[hit] = float("nan")
    parts = [F.validation_terms(Y[b:b + 2], L[b:b + 2], "huber", vc.DELTA, 1, True) for b in range(0, 7, 2)]
    one = F.validation_terms(Y, L, "huber", vc.DELTA, 1, True)
    cap, F.VALIDATION_CHUNK_BYTES = F.VALIDATION_CHUNK_BYTES, 2 * 3 * 5 * 8          # two windows of 3 counted steps per chunk
    try:
        assert F.validation_chunk_windows(7, 3, 5, F.VALIDATION_CHUNK_BYTES) == 2
        cut = F.validation_terms(Y, L, "huber", vc.DELTA, 1, True)                   # four chunks: 2 + 2 + 2 + 1 windows
    finally:
        F.VALIDATION_CHUNK_BYTES = cap
    total = 0.0
    for p in parts:                                              # the chunks' sums, added in ascending order
        total = total + float(p[0])
    assert float(cut[0]) == total and int(cut[1]) == sum(int(p[1]) for p in parts) == int(one[1])
    assert float(cut[2]) == max(float(p[2]) for p in parts) == float(one[2])
    assert vc.rel(float(cut[0]), float(one[0])) <= 1e-14


def _record(fill=0xA5):
    rec = torch.full((256,), fill, dtype=torch.uint8)
    return rec


def _read(rec, name):
    off, n = OFFSETS[name]
    dt = {"sum": torch.float64, "mean": torch.float64, "max_abs": torch.float32, "loss": torch.float32}.get(name, torch.int64)
    return rec[off:off + n].clone().view(dt)[0]


def test_val_add_writes_the_six_words_by_the_headers_offsets_and_nothing_else():
    from windgnn_amd import _lib as L
    from windgnn_amd.functional import val_add, val_word
    assert {k: (off, torch.empty((), dtype=getattr(torch, dt)).element_size()) for k, (off, dt) in L.VAL_WORDS.items()} == OFFSETS
    rec = _record()
    for name in ("sum", "count", "max_abs", "calls"):            # what wgnn_val_begin leaves: zeros, and NaN in mean and loss
        val_word(rec, name).zero_()
    val_word(rec, "mean").fill_(float("nan"))
    val_word(rec, "loss").fill_(float("nan"))
    val_word(rec, "passes").fill_(7)
    val_word(rec, "stale").fill_(3)
    before = rec.clone()
    val_add(rec, torch.tensor(0.0, dtype=torch.float64), torch.tensor(0), torch.tensor(0.0, dtype=torch.float64))
    assert int(_read(rec, "count")) == 0 and int(_read(rec, "calls")) == 1
    assert math.isnan(float(_read(rec, "mean"))) and math.isnan(float(_read(rec, "loss")))       # count = 0: NaN, not 0 / 0 = error
    s1, s2, a1, a2 = 0.1 + 2.0 ** -40, 2.5, 0.7000000001, 0.3
    val_add(rec, torch.tensor(s1, dtype=torch.float64), torch.tensor(3), torch.tensor(a1, dtype=torch.float64))
    val_add(rec, torch.tensor(s2, dtype=torch.float64), 5, torch.tensor(a2, dtype=torch.float64))
    assert float(_read(rec, "sum")) == s1 + s2 and int(_read(rec, "count")) == 8 and int(_read(rec, "calls")) == 3
    assert float(_read(rec, "mean")) == (s1 + s2) / 8
    assert torch.equal(_read(rec, "loss"), torch.tensor((s1 + s2) / 8, dtype=torch.float64).float())
    assert torch.equal(_read(rec, "max_abs"), torch.tensor(a1, dtype=torch.float64).float())
    assert torch.equal(rec[40:], before[40:]) and int(_read(rec, "passes")) == 7 and int(_read(rec, "stale")) == 3


def _cpu_step(S=3, H=9, **kw):
    from windgnn_amd import GCN_GRU
    from windgnn_amd.trainer import TrainStep
    torch.manual_seed(0)
    return TrainStep(GCN_GRU(13, 13, 13, S * 13, H, math=kw.pop("math", "f32")), **kw)


def test_validate_refuses_by_the_arguments_name_before_any_launch():
    tr = _cpu_step()
    A, X, L = torch.rand(3, 3), torch.rand(2, 4, 3, 13), torch.rand(2, 4, 9)

    class Ev:
        H = 12
    with pytest.raises(ValueError, match="loss='hinge'.*'mse', 'l1' or 'huber'"):
        tr.validate(A, X, L, loss="hinge")
    for bad in (-1, 4, 1.5):
        with pytest.raises(ValueError, match="loss_from="):
            tr.validate(A, X, L, loss_from=bad)
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match="huber_delta="):
            tr.validate(A, X, L, loss="huber", huber_delta=bad)
    for bad in (torch.rand(2, 4, 8), torch.rand(2, 3, 9), torch.rand(3, 4, 9), torch.rand(4, 9), torch.rand(2, 4, 9, 1)):
        with pytest.raises(ValueError, match="L must be"):
            tr.validate(A, X, bad)
    with pytest.raises(ValueError, match="L must be float32 or X's dtype"):
        tr.validate(A, X, L.double())
    with pytest.raises(RuntimeError, match="X must be"):
        tr.validate(A, torch.rand(2, 4, 4, 13), L)
    with pytest.raises(ValueError, match="evaluator= must be an evaluate.Evaluator of this model's 9 outputs"):
        tr.validate(A, X, L, evaluator=Ev())
    Ev.H = 9
    with pytest.raises(ValueError, match="missing_labels=True.*update_series"):
        tr.validate(A, X, L, evaluator=Ev(), missing_labels=True)
    with pytest.raises(RuntimeError, match="There is no CPU fallback"):
        tr.validate(A, X, L)
    with pytest.raises(RuntimeError, match="There is no CPU fallback"):
        tr.validate(A, X[:1], L[0], loss_from=3)                 # [T, H] at B = 1 passes the shape check; the last-step route too
    assert tr._val is None and not tr._val_open and tr.steps == 0      # nothing was made, opened or counted
    with pytest.raises(RuntimeError, match="no validation call has run"):
        tr.val_loss


@pytest.mark.parametrize("name,mode", vc.SCENARIOS)
def test_the_three_step_scenario_separates_its_held_out_losses_on_the_oracle(name, mode):
    vals, _, _ = vc.scenario(name)
    gaps = [abs(a - b) / max(a, b) for i, a in enumerate(vals) for b in vals[i + 1:]]
    assert len(vals) == vc.STEPS + 1 and min(gaps) >= 1e-3, (vals, gaps)
    seq = vc.rule(vals)
    print("\n%s: held-out losses %s -> (best_step, improved, stale) %s" % (name, vals, seq))
    assert seq[0] == (0, 1, 0)                                   # the first finite loss wins
    assert seq[-1][0] != vc.STEPS and seq[-1][2] >= 1            # the shifted third step loses: the best step is not the last


def test_the_shapes_reach_what_they_are_there_for():
    for name, (S, T, B, H) in vc.SHAPES.items():
        c = vc.case(name)
        assert tuple(c.X.shape) == (B, T, S, 13) and tuple(c.Yo.shape) == (B, T, H) and c.Yo.dtype == torch.float64
        assert 0 < int(c.hit.sum()) < c.hit.numel()
    assert (vc.SHAPES["odd"][0] * 13) % 2 == 1 and vc.SHAPES["wide"][3] > 128 and vc.SHAPES["csr"][0] > 64
    assert vc.case("csr").csr is not None and vc.t_froms(2) == [0, 1] and vc.t_froms(12) == [0, 2, 11]
