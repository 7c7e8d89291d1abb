"""Series training and evaluation through missing labels on the MI355X (include/windgnn_series_masked.h, series.py,
TrainStep.step_series(missing_labels=True), Evaluator.update_series) against the fp64 oracle on the MATERIALISED windows with the
masked loss formed in the test (tests/series_masked_cases.py: dY = 2 (Y - L) mask / m, loss = sum over M of (Y - L)^2 / m), at
the bar of tests/test_gpu_series_at.py: conftest.rel_to_max <= 1e-4 on Y and each of the 8 gradients, the loss relative to the
oracle's.  The observed errors are printed per case.  tests/test_series_masked_host.py qualifies the cases on the CPU.

The C entry points are called directly on buffers of exactly their ABI lengths inside a guarded.Arena, under the library's
profiler: a case also proves by the launched names that the masked instance ran and no unmasked sibling did, that the
per-workgroup label counts in loss_buf are the exact integers, and that no gradient element is NaN or infinite (NaN * 0).
The evaluation tests hold tests/test_gpu_eval.py's bars (counts exact, sums 1e-10 relative, figures 2.4e-7) against numpy fp64 on
the valid entries of each column."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import series_at_cases as sc
import series_masked_cases as mc
from conftest import PARAM_KEYS, rel_to_max
from guarded import FILLS, Arena
from test_gpu_eval import STAT_TOL, SUM_TOL, _close, _gpu, _header
from test_gpu_series import F, STATUS, TOL, WIND_MAX, WIND_MIN, _dev, _fit
from test_gpu_series_at import _model_of
from test_gpu_series_train import NO_LOSS_STATS
from test_gpu_series_train import TOL as LOSS_TOL

pytestmark = pytest.mark.gpu

NO_LABELS = 32                         # WGNN_STATUS_NO_LABELS
GRADS = ["g." + k for k in PARAM_KEYS]


def _sd(q):
    from windgnn_amd import _lib as L
    return L.SeriesDims(q.rows, q.T, q.stride or 0, q.n, q.S, F, q.H, 0, 0, 0, 0)


def _sizes(lib, sd):
    fam = "wgnn_series_at_%s" if sd.stride == 0 else "wgnn_series_%s"
    return [getattr(lib, fam % name)(C.byref(sd)) for name in ("workspace_bytes", "stash_bytes", "status_offset")]


def _arena_step(q, fill="nan", dirty=None, status=0):
    """wgnn_series_fwd_loss_masked + wgnn_series_bwd_mse_masked on the reference q inside an arena, the workspace re-poisoned in
    between.  status: the bits the backward must leave in the window-major half's status block.  Returns (outputs as host bytes,
    launched names, final scratch bytes)."""
    from windgnn_amd import _lib as L
    lib = L.load()
    n, T, H, rows = q.n, q.T, q.H, q.rows
    sd = _sd(q)
    ws_bytes, st_bytes, off = _sizes(lib, sd)
    lb_bytes = lib.wgnn_series_masked_loss_bytes(C.byref(sd))
    nb = -(-n // 16)
    assert ws_bytes > off >= STATUS and st_bytes > 0 and lb_bytes == 4 * (3 * nb + 4)
    a = Arena(_dev(), fill)
    dirty = dirty or {}

    def add(name, t=None, shape=None):
        return a.buf(name, (t.numel() if t is not None else int(np.prod(shape))) * 4, data=t)

    add("A", q.A)
    add("Xs", q.Xs)
    ls_rows = rows if q.stride is None else (n - 1) * q.stride + T       # the least each form accepts: a read past them hits the guard
    add("Ls", q.Ls[:ls_rows].contiguous())
    add("starts", torch.tensor(q.starts, dtype=torch.int32))
    for k in PARAM_KEYS:
        add("p." + k, q.p[k])
        add("g." + k, shape=q.p[k].shape)
    add("Y", shape=(n, T, H))
    add("loss", shape=(1,))
    for name, nbytes in (("stash", st_bytes), ("loss_buf", lb_bytes)):
        a.buf(name, nbytes, data=_fit(dirty[name], nbytes) if name in dirty else None)
    a.buf("ws", ws_bytes, data=_fit(dirty["ws"], ws_bytes) if "ws" in dirty else None, zero_head=STATUS)
    a.commit()
    P = lambda name: C.c_void_p(a[name].ptr)   # noqa: E731
    ps, gs = L.Params(), L.Grads()
    for (field, _), k in zip(L.Grads._fields_, PARAM_KEYS):
        setattr(ps, field, a["p." + k].ptr)
        setattr(gs, field, a["g." + k].ptr)
    word = a["ws"].view(torch.int32)
    table = P("starts") if q.stride is None else None

    def after(what, want=0):
        torch.cuda.synchronize()
        assert a.check() == {}, (what, fill, a.check())
        assert int(word[0]) == 0, (what, "status word", int(word[0]))
        assert int(word[off // 4]) == want, (what, "window-major status", int(word[off // 4]))

    word[off // 4] = 0                                       # kernels only OR into the block: the caller zeroes it
    L.profile_enable(True)
    try:
        rc = lib.wgnn_series_fwd_loss_masked(C.byref(sd), P("A"), P("Xs"), table, C.byref(ps), P("Ls"), ls_rows, P("Y"), P("stash"),
                                             P("loss_buf"), P("ws"), ws_bytes, None)
        assert rc == 0, rc
        after("wgnn_series_fwd_loss_masked")
        if "ws" not in dirty:
            a["ws"].poison()                                 # the workspace carries nothing from the forward to the backward
            word[off // 4] = 0
        rc = lib.wgnn_series_bwd_mse_masked(C.byref(sd), P("A"), P("Xs"), table, C.byref(ps), P("Y"), P("Ls"), ls_rows, 1.0,
                                            P("stash"), P("loss_buf"), P("loss"), C.byref(gs), P("ws"), ws_bytes, None)
        assert rc == 0, rc
        after("wgnn_series_bwd_mse_masked", status)
        names = tuple(rec["name"] for rec in L.profile_read())
    finally:
        L.profile_enable(False)
    outs = ["Y", "loss"] + GRADS
    if fill != "zero" and not dirty:
        for name in outs + ["loss_buf"]:
            # (the three spare words of loss_buf are nobody's)
            assert a[name].unwritten(4) == (3 if name == "loss_buf" else 0), (name, fill, a[name].unwritten(4))
    for name in ("A", "Xs", "Ls", "starts") + tuple("p." + k for k in PARAM_KEYS):      # inputs are read only
        assert a[name].unwritten(1) == a[name].nbytes, name
    out = {name: a[name].host() for name in outs}
    out["counts"] = a["loss_buf"].host().view(torch.int32)[2 * nb + 4:]
    return out, names, {k: a[k].host() for k in ("stash", "ws", "loss_buf")}


def _f32(b, shape):
    return b.view(torch.float32).reshape(shape)


def _grads(q, out):
    return {k: _f32(out["g." + k], q.gm[k].shape) for k in PARAM_KEYS}


def _errors(q, out):
    err = {"Y": rel_to_max(_f32(out["Y"], (q.n, q.T, q.H)), q.Yo),
           "loss": abs(float(_f32(out["loss"], (1,))[0]) - q.loss_o) / q.loss_o}
    for k, g in _grads(q, out).items():
        err[k] = rel_to_max(g, q.gm[k])
    return err


def _assert_bar(what, err):
    print("\n%s: worst %.2e  " % (what, max(err.values())) + "  ".join("%s %.2e" % kv for kv in err.items()))
    for k, e in err.items():
        assert e <= (LOSS_TOL if k.startswith("loss") else TOL), (what, k, e)


def _assert_finite(what, out, q):
    for k, g in _grads(q, out).items():
        assert torch.isfinite(g).all(), (what, k, "a gradient element is NaN or infinite")
    assert torch.isfinite(_f32(out["Y"], (q.n, q.T, q.H))).all(), what


def _assert_names(q, names):
    """The masked instances of this H and row mapping ran, and no unmasked sibling (nor the other mapping's) did."""
    tag = ",starts,masked" if q.stride is None else ",masked"
    want = {"gru_fwd_kernel<%d%s>" % (sc.fwd_ks(q.H), tag), "gru_bwd_kernel<%d%s>" % (sc.bwd_ks3(q.H), tag),
            "series_fold_at_kernel" if q.stride is None else "series_fold_kernel"}
    rec = {x for x in names if x.startswith(("gru_fwd_kernel", "gru_bwd_kernel", "series_fold"))}
    assert rec == want, (rec, want)
    assert ("series_starts_check_kernel" in names) == (q.stride is None), names


@functools.lru_cache(maxsize=None)
def _checked(base, how, mask):
    q = mc.reference(base, how, mask)
    assert q.margin > 1e-5, "a ReLU pre-activation within %.1e of zero (relative): pick another seed" % q.margin
    return q


# ---- oracle parity ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(mc.PARITY))
def test_masked_pair_matches_the_oracle_with_the_masked_loss(cid):
    q = _checked(*mc.PARITY[cid])
    assert 0 < q.m < q.n * q.T * q.H
    out, names, _ = _arena_step(q)
    _assert_names(q, names)
    _assert_finite(cid, out, q)
    assert out["counts"].tolist() == q.counts, (cid, "per-workgroup label counts", out["counts"].tolist(), q.counts)
    _assert_bar("%s (m = %d of %d)" % (cid, q.m, q.n * q.T * q.H), _errors(q, out))


# ---- no NaN: the unmasked entry points' bits -----------------------------------------------------------------------------------
@pytest.mark.parametrize("base,how", [("irregular", "table"), ("irregular", "stride1"), ("irregular", "stride2"),
                                      ("real_widths", "table"), ("K8_big", "table")])
def test_without_a_nan_everything_is_bit_identical_to_the_unmasked_entry_points(base, how):
    """Mask (e): Y, the partial sums and maxima, the loss and all 8 gradients (which read the stash) are torch.equal."""
    from windgnn_amd.series import series_backward_mse_raw, series_forward_loss_raw
    q = _checked(base, how, "e")
    dev = _dev()
    A, Xs, Ls = q.A.to(dev), q.Xs.to(dev), q.Ls.to(dev)
    assert not torch.isnan(Ls).any()
    params = [q.p[k].to(dev).contiguous() for k in PARAM_KEYS]
    kw = {"starts": q.starts} if q.stride is None else {"n_windows": q.n}

    def run(flag):
        Y, stash, loss_buf, sd, *tab = series_forward_loss_raw(A, Xs, Ls, q.T, q.stride, params, missing_labels=flag, **kw)
        g = [torch.full_like(p, float("nan")) for p in params]
        loss = torch.full((), float("nan"), device=dev)
        series_backward_mse_raw(sd, A, Xs, params, Y, Ls, stash, loss_buf, g, loss, 0.75, None, *tab, missing_labels=flag)
        return [Y, loss] + g, loss_buf

    (plain, lb0), (masked, lb1) = run(False), run(True)
    nb = -(-q.n // 16)
    assert lb0.numel() == 2 * nb + 4 and lb1.numel() == 3 * nb + 4
    assert torch.equal(lb0[:2 * nb], lb1[:2 * nb]) and float(lb0[2 * nb]) != float(lb1[2 * nb])      # same statistics, another tag
    assert lb1[2 * nb + 4:].view(torch.int32).tolist() == q.counts and sum(q.counts) == q.n * q.T * q.H
    assert not torch.isnan(plain[1]).item()
    for i, (u, v) in enumerate(zip(plain, masked)):
        assert u.shape == v.shape and torch.equal(u, v), (base, how, i)
    _assert_bar("%s-%s-e" % (base, how), {"Y": rel_to_max(masked[0].cpu(), q.Yo),
                                          "loss": abs(float(masked[1]) - q.loss_o) / q.loss_o})


# ---- no label at all -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["table", "stride1"])
def test_without_any_label_the_loss_is_nan_the_gradients_are_zero_and_the_status_says_so(how):
    q = _checked("irregular", how, "f")
    assert q.m == 0
    out, names, left = _arena_step(q, "finite", status=NO_LABELS)      # (not the NaN fill: the loss written is a NaN itself)
    _assert_names(q, names)
    assert torch.isnan(_f32(out["loss"], (1,))).all()
    for k, g in _grads(q, out).items():
        assert (g == 0).all(), (k, "not exactly zero")
    assert out["counts"].tolist() == [0] * len(q.counts)
    Y = _f32(out["Y"], (q.n, q.T, q.H))
    assert torch.isfinite(Y).all() and rel_to_max(Y, q.Yo) <= TOL                   # nothing non-finite anywhere else
    nb = len(q.counts)
    stats = left["loss_buf"].view(torch.float32)[:2 * nb]
    assert (stats == 0).all()                                                       # sums and maxima over no label


def test_a_tag_mismatch_is_loud_in_both_directions():
    """A masked backward on an unmasked forward's statistics, and the reverse: NaN loss and WGNN_STATUS_NO_LOSS_STATS, not
    WGNN_STATUS_NO_LABELS."""
    from windgnn_amd import _lib as L
    from windgnn_amd.functional import _Workspace
    from windgnn_amd.series import series_backward_mse_raw, series_forward_loss_raw
    q = _checked("irregular", "stride1", "b")
    dev = _dev()
    lib = L.load()
    A, Xs, Ls = q.A.to(dev), q.Xs.to(dev), q.Ls.to(dev)
    clean = q.clean.to(dev)
    params = [q.p[k].to(dev).contiguous() for k in PARAM_KEYS]
    grads = [torch.empty_like(p) for p in params]
    loss = torch.zeros((), device=dev)
    Y, stash, lb_masked, sd = series_forward_loss_raw(A, Xs, Ls, q.T, 1, params, n_windows=q.n, missing_labels=True)
    off = lib.wgnn_series_status_offset(C.byref(sd))
    word = _Workspace.get(dev, lib.wgnn_series_workspace_bytes(C.byref(sd)))[off:off + 4].view(torch.int32)
    word.zero_()
    series_backward_mse_raw(sd, A, Xs, params, Y, Ls, stash, lb_masked, grads, loss, missing_labels=True)
    assert int(word.item()) == 0 and abs(float(loss) - q.loss_o) <= LOSS_TOL * q.loss_o                # matched: quiet
    series_backward_mse_raw(sd, A, Xs, params, Y, clean, stash, lb_masked, grads, loss)                # unmasked backward
    assert torch.isnan(loss).item() and int(word.item()) == NO_LOSS_STATS
    word.zero_()
    _, stash0, lb_plain, _ = series_forward_loss_raw(A, Xs, clean, q.T, 1, params, n_windows=q.n)
    room = torch.zeros(lb_masked.numel(), device=dev)
    room[:lb_plain.numel()] = lb_plain                       # (the masked backward's buffer has the masked length)
    series_backward_mse_raw(sd, A, Xs, params, Y, Ls, stash0, room, grads, loss, missing_labels=True)
    assert torch.isnan(loss).item() and int(word.item()) == NO_LOSS_STATS
    for g in grads:
        assert (g == 0).all()                                # no count to trust: dY = 0
    word.zero_()


# ---- TrainStep.step_series(missing_labels=True) -------------------------------------------------------------------------------
STEPS = 3


@functools.lru_cache(maxsize=None)
def _trajectory():
    """The oracle's STEPS Adam steps on the irregular table with the masked loss of mask (b): (losses, parameters after)."""
    from oracle import windgnn_oracle as orc
    q = _checked("irregular", "table", "b")
    A, X, L = q.A.double(), q.X.double(), q.L.double()
    p = dict(q.p64)
    state = orc.adam_init(p)
    losses = []
    for _ in range(STEPS):
        Y, cache = orc.forward(A, X, p)
        loss, dY, _ = mc.masked_loss(Y, L)
        losses.append(float(loss))
        p = orc.adam_step(p, orc.backward(A, X, p, Y, cache, dY), state)
    return losses, p


def test_three_masked_steps_follow_the_oracle_trajectory_and_repeat_bit_for_bit():
    from windgnn_amd.trainer import TrainStep
    q = _checked("irregular", "table", "b")
    lo, po = _trajectory()
    dev = _dev()
    A, Xs, Ls = q.A.to(dev), q.Xs.to(dev), q.Ls.to(dev)
    perm = torch.randperm(q.n, generator=torch.Generator().manual_seed(6)).tolist()
    table = torch.tensor([q.starts[i] for i in perm], device=dev)
    runs = []
    for _ in range(2):
        model = _model_of(q.r)
        tr = TrainStep(model, keep_best=True)
        losses = []
        for _ in range(STEPS):
            loss, Y = tr.step_series(A, Xs, Ls, q.T, starts=table, missing_labels=True)
            assert tuple(Y.shape) == (q.n, q.T, q.H) and loss.dim() == 0
            losses.append(float(loss))
        assert tr.steps == STEPS and float(tr.best_loss) == min(losses)
        runs.append((losses, tr.flat_p.clone(), model))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])          # the same steps from the same state
    seen = {k: rel_to_max(p.detach().cpu(), po[k]) for k, p in runs[0][2].named_parameters()}
    for i, (a, b) in enumerate(zip(runs[0][0], lo)):
        seen["loss%d" % (i + 1)] = abs(a - b) / b
    _assert_bar("step_series(missing_labels=True) x3", seen)
    # the strided form through forward_backward_series: the gradients in the bucket, no step
    s = _checked("irregular", "stride2", "b")
    tr = TrainStep(_model_of(s.r))
    loss, Y = tr.forward_backward_series(A, Xs, s.Ls.to(dev), s.T, 2, n_windows=s.n, missing_labels=True)
    err = {"Y": rel_to_max(Y.cpu(), s.Yo), "loss": abs(float(loss) - s.loss_o) / s.loss_o}
    err.update({k: rel_to_max(g.cpu(), s.gm[k]) for k, g in zip(PARAM_KEYS, tr.g_views)})
    _assert_bar("forward_backward_series(missing_labels=True)", err)
    assert tr.steps == 0


# ---- footprint -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["table", "stride2"])
def test_footprint_guards_fills_and_dirty_scratch(how):
    q = _checked("irregular", how, "b")
    assert FILLS[0] == "zero"
    base, _, _ = _arena_step(q, FILLS[0])
    _assert_bar("arena zero " + how, _errors(q, base))
    for fill in FILLS[1:]:
        out, _, _ = _arena_step(q, fill)
        for key, v in out.items():
            assert torch.equal(v, base[key]), (key, fill)
    _, _, left = _arena_step(_checked("K8_small", "table", "b"), "nan")        # scratch another shape's calls left behind
    for fill in ("finite", "nan"):
        out, _, _ = _arena_step(q, fill, dirty=left)
        for key, v in out.items():
            assert torch.equal(v, base[key]), (key, fill, "dirty")


# ---- evaluation over a label series ----------------------------------------------------------------------------------------------
WIND = (1.5, 83.25)


@functools.lru_cache(maxsize=None)
def _eval_inputs(B, T, H, how):
    """A label series in [0.2, 1) with ~15 % NaN scattered and one column that never has a truth, the rows of the B windows
    (strided, or a table in no order with duplicates), predictions around the clean truth, and numpy's figures in fp64 on the
    valid entries of each column."""
    rng = np.random.default_rng(7 + 1009 * B + 31 * T + H + len(how))
    stride = {"stride1": 1, "stride2": 2}.get(how)
    rows = (B - 1) * (stride or 1) + T + 3
    clean = rng.uniform(0.2, 1.0, size=(rows, H)).astype(np.float32)
    Ls = clean.copy()
    Ls[rng.uniform(size=Ls.shape) < 0.15] = np.nan
    dead = H // 2
    Ls[:, dead] = np.nan
    Ls[:, [dead - 1, dead + 1]] = clean[:, [dead - 1, dead + 1]]        # its neighbours have every truth
    starts = rng.integers(0, rows - T + 1, size=B).astype(np.int32) if stride is None else np.arange(B, dtype=np.int32) * stride
    truth_rows = starts.astype(np.int64) + T - 1
    wmin, wmax = np.float64(np.float32(WIND[0])), np.float64(np.float32(WIND[1]))
    pred = ((clean[truth_rows].astype(np.float64) * (wmax - wmin) + wmin) * (1.0 + 0.3 * rng.standard_normal((B, H)))).astype(np.float32)
    truth = Ls[truth_rows].astype(np.float64) * (wmax - wmin) + wmin
    header, stats = np.zeros((5, H)), np.full((H, 4), np.nan)
    err = np.abs(truth - pred.astype(np.float64))
    for c in range(H):
        ok = ~np.isnan(truth[:, c])
        d, t = (truth[ok, c] - pred[ok, c].astype(np.float64)), truth[ok, c]
        a = 1 - np.abs(d) / t
        header[:, c] = [ok.sum(), (d ** 2).sum(), np.abs(d).sum(), a.sum(), (a ** 2).sum()]
        if ok.any():
            stats[c] = [np.sqrt(np.mean(d ** 2)), np.mean(np.abs(d)), np.mean(a), np.std(a)]
    assert header[0, dead] == 0 and (header[0, [dead - 1, dead + 1]] == B).all()
    return dict(Ls=Ls, clean=clean, starts=starts, stride=stride, pred=pred, header=header, stats=stats, abs_err=err.astype(np.float32),
                dead=dead, rows=rows)


@pytest.mark.parametrize("how", ["stride1", "stride2", "table"])
@pytest.mark.parametrize("B,T,H", [(3, 5, 21), (70, 5, 21), (3, 24, 102), (70, 24, 102)])
def test_eval_accum_series_against_numpy_on_the_valid_entries(B, T, H, how):
    from windgnn_amd import _lib as L
    from windgnn_amd.evaluate import eval_accum, eval_accum_series, eval_buffer, eval_stats
    dev = _dev()
    e = _eval_inputs(B, T, H, how)
    kw = {"stride": e["stride"]} if e["stride"] else {"stride": None, "starts": _gpu(e["starts"])}
    pred, Ls = _gpu(e["pred"]), _gpu(e["Ls"])
    acc = eval_buffer(H, dev)
    err = torch.full((B, H), 7.0, device=dev)
    L.profile_enable(True)
    try:
        eval_accum_series(pred, Ls, T, WIND[0], WIND[1], acc, skip_missing=True, abs_err=err, **kw)
        names = {rec["name"] for rec in L.profile_read()}
    finally:
        L.profile_enable(False)
    assert names == ({"eval_accum_series_kernel<skip>", "eval_fold_count_kernel"} if B > 32 else {"eval_accum_series_kernel<skip>"})
    what = "B%d T%d H%d %s" % (B, T, H, how)
    hdr = _header(acc, H)
    assert np.array_equal(hdr[0], e["header"][0]), (what, "per-column counts")
    _close(hdr[1:], e["header"][1:], SUM_TOL, what + " header sums")
    stats = eval_stats(acc, H).cpu().numpy()
    if B > 32:       # (at B = 3 a column may hold one truth: std = 0 on both sides, and the relative bar needs std >= 1e-4)
        _close(stats, e["stats"], STAT_TOL, what + " stats")
    else:
        _close(stats[:, :3], e["stats"][:, :3], STAT_TOL, what + " stats")
    d = e["dead"]
    assert hdr[0, d] == 0 and (hdr[1:, d] == 0).all() and np.isnan(stats[d]).all()        # no truth: n = 0, NaN figures
    assert (hdr[0, [d - 1, d + 1]] == B).all() and np.isfinite(stats[[d - 1, d + 1], :3]).all()     # ... its neighbours untouched
    got = err.cpu().numpy()
    ok = ~np.isnan(e["abs_err"])
    assert np.array_equal(np.isnan(got), ~ok) and np.array_equal(got[ok].view(np.int32), e["abs_err"][ok].view(np.int32))
    # a second call accumulates: the same sums again (a doubling is exact)
    eval_accum_series(pred, Ls, T, WIND[0], WIND[1], acc, skip_missing=True, **kw)
    assert np.array_equal(_header(acc, H), 2 * hdr)
    # skip_missing = 0 on labels without NaN: wgnn_eval_accum's header on the gathered labels, bit for bit
    clean = _gpu(e["clean"])
    gathered = torch.stack([clean[s:s + T] for s in e["starts"].tolist()]).contiguous()
    a0, a1 = eval_buffer(H, dev), eval_buffer(H, dev)
    e0, e1 = torch.zeros(B, H, device=dev), torch.ones(B, H, device=dev)
    eval_accum(pred, gathered, WIND[0], WIND[1], a0, e0)
    eval_accum_series(pred, clean, T, WIND[0], WIND[1], a1, skip_missing=False, abs_err=e1, **kw)
    assert torch.equal(a0[:5 * H].view(torch.int64), a1[:5 * H].view(torch.int64)) and torch.equal(e0, e1)
    # ... and a NaN truth then poisons its column as it does there
    a2 = eval_buffer(H, dev)
    eval_accum_series(pred, Ls, T, WIND[0], WIND[1], a2, skip_missing=False, **kw)
    h2 = _header(a2, H)
    assert (h2[0] == B).all() and np.isnan(h2[1:, d]).all()


def test_update_series_is_forward_last_series_and_the_raw_call_and_accumulates():
    from windgnn_amd.evaluate import Evaluator, eval_accum_series, eval_buffer
    from windgnn_amd.series import forward_last_series
    q = _checked("irregular", "table", "b")
    dev = _dev()
    A, Xs, Ls = q.A.to(dev), q.Xs.to(dev), q.Ls.to(dev)
    model = _model_of(q.r)
    perm = torch.randperm(q.n, generator=torch.Generator().manual_seed(9)).tolist()
    shuffled = [q.starts[i] for i in perm]
    for kw in ({"starts": shuffled}, {"stride": 2, "n_windows": 17}, {}):
        ev = Evaluator(model, A, WIND_MIN, WIND_MAX, keep_errors=True)
        with torch.no_grad():
            pred = ev.update_series(Xs, Ls, q.T, skip_missing=True, **kw)
            want = forward_last_series(model, A, Xs, q.T, WIND_MIN, WIND_MAX, **kw)
        assert torch.equal(pred, want) and pred.is_contiguous()
        acc = eval_buffer(q.H, dev)
        err = torch.empty_like(pred)
        if "starts" in kw:
            raw = {"stride": None, "starts": torch.tensor(shuffled, dtype=torch.int32, device=dev)}
        else:
            raw = {"stride": kw.get("stride", 1)}
        eval_accum_series(want, Ls, q.T, WIND_MIN, WIND_MAX, acc, skip_missing=True, abs_err=err, **raw)
        H5 = 5 * q.H
        assert torch.equal(ev.acc[:H5].view(torch.int64), acc[:H5].view(torch.int64))
        assert torch.equal(ev.errors().view(torch.int32), err.view(torch.int32))
        # numpy on the valid entries: the truth of a window that starts at s is row s + T - 1
        st = shuffled if "starts" in kw else [w * raw["stride"] for w in range(pred.shape[0])]
        truth = q.Ls[[s + q.T - 1 for s in st]].double().numpy() * (np.float64(np.float32(WIND_MAX)) - np.float64(np.float32(WIND_MIN))) \
            + np.float64(np.float32(WIND_MIN))
        ok = ~np.isnan(truth)
        hdr = _header(ev.acc, q.H)
        assert np.array_equal(hdr[0], ok.sum(0))
        d = np.where(ok, truth - pred.cpu().double().numpy(), 0.0)
        _close(hdr[1], (d ** 2).sum(0), SUM_TOL, "update_series sum of squares %s" % sorted(kw))
        r1 = ev.compute()
        assert r1.header[0].tolist() == ok.sum(0).tolist() and int(r1.count) == int(ok[:, 0].sum())      # per column
        with torch.no_grad():
            ev.update_series(Xs, Ls, q.T, skip_missing=True, **kw)
        assert np.array_equal(_header(ev.acc, q.H), 2 * hdr) and ev.errors().shape[0] == 2 * pred.shape[0]
