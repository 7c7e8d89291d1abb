"""Series training on a loss spec on the MI355X (include/windgnn_series_lossfn.h, series.py's loss= / huber_delta= / loss_from=,
TrainStep.step_series(loss=...)) against the fp64 oracle on the MATERIALISED windows with the loss formed in the test
(tests/series_lossfn_cases.py), at the bars of tests/test_gpu_series.py and tests/test_gpu_series_train.py: conftest.rel_to_max
<= 1e-4 on Y and each of the 8 gradients, the loss relative to the oracle's.  The observed errors are printed per case.
tests/test_series_lossfn_host.py qualifies the cases on the CPU.

The C entry points are called directly on buffers of exactly their ABI lengths inside a guarded.Arena, under the library's
profiler, as tests/test_gpu_series_masked.py does it: a case also proves by the launched names that the `lossfn` instance ran and
no sibling did, that the per-workgroup counts in loss_buf are the exact integers, and that no gradient element is NaN or
infinite."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import series_at_cases as sc
import series_lossfn_cases as lc
from conftest import PARAM_KEYS, rel_to_max
from guarded import FILLS, Arena
from test_gpu_series import F, STATUS, TOL, _dev, _fit
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


def _spec(q, **over):
    """(kind, delta, t_from, masked) of the reference q, with fields replaced."""
    d = dict(kind=lc.KINDS[q.kind], delta=q.delta, t_from=q.t_from, masked=q.masked)
    d.update(over)
    return (d["kind"], d["delta"], d["t_from"], d["masked"])


def _arena_step(q, fwd="lossfn", bwd=None, fill="nan", dirty=None, status=0, grad_scale=1.0, Ls=None, short_buf=False,
                gate=None):
    """One forward + backward pair on the reference q inside an arena, the workspace re-poisoned in between.  fwd / bwd: "plain"
    (wgnn_series_fwd_loss / _bwd_mse or their _at forms), "masked" (the masked pair), "lossfn" (the new pair on q's own spec), or
    a spec tuple (the new pair on that spec); bwd defaults to fwd.  status: the bits the backward must leave in the window-major
    half's status block.  short_buf: loss_buf has the unmasked forward's own, shorter length whatever the backward is.
    Returns (outputs as host bytes, launched names, final scratch bytes).  gate (tests/stream_cases.py): the calls go to its
    side stream, nothing synchronises in between, no kernel names are collected, and guards and both status words are looked
    at once, at the end."""
    from windgnn_amd import _lib as L
    lib = L.load()
    bwd = fwd if bwd is None else bwd
    n, T, H, rows = q.n, q.T, q.H, q.rows
    sd = _sd(q)
    ws_bytes, st_bytes, off = _sizes(lib, sd)
    nb = -(-n // 16)
    lb_bytes = lib.wgnn_series_lossfn_bytes(C.byref(sd))
    assert ws_bytes > off >= STATUS and st_bytes > 0 and lb_bytes == 4 * (3 * nb + 4) == lib.wgnn_series_masked_loss_bytes(C.byref(sd))
    if fwd == "plain" and (bwd == "plain" or short_buf):
        lb_bytes = 4 * (2 * nb + 4)                              # the unmasked pair's own length
    a = Arena(_dev(), fill)
    dirty = dirty or {}

    def add(name, t=None, shape=None):
        return a.buf(name, (t.numel() if t is not None else int(np.prod(shape))) * 4, data=t)

    add("A", q.A)
    add("Xs", q.Xs)
    ls_rows = rows if q.stride is None else (n - 1) * q.stride + T       # the least each form accepts: a read past them hits the guard
    add("Ls", (q.Ls if Ls is None else Ls)[:ls_rows].contiguous())
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
    table = (P("starts"),) if q.stride is None else (None,)
    strided = () if q.stride is not None else table              # the unmasked strided entry points take no table argument

    st = gate.handle if gate is not None else None

    def after(what, want=0):
        if gate is not None:
            return
        torch.cuda.synchronize()
        assert a.check() == {}, (what, fill, a.check())
        assert int(word[0]) == 0, (what, "status word", int(word[0]))
        assert int(word[off // 4]) == want, (what, "window-major status", int(word[off // 4]))

    def forward(how):
        head = (C.byref(sd), P("A"), P("Xs"))
        tail = (P("Y"), P("stash"), P("loss_buf"), P("ws"), ws_bytes, st)
        if how == "plain":
            fn = lib.wgnn_series_fwd_loss_at if q.stride is None else lib.wgnn_series_fwd_loss
            return fn(*head, *strided, C.byref(ps), P("Ls"), ls_rows, *tail)
        if how == "masked":
            return lib.wgnn_series_fwd_loss_masked(*head, *table, C.byref(ps), P("Ls"), ls_rows, *tail)
        spec = L.LossFn(*(_spec(q) if how == "lossfn" else how))
        return lib.wgnn_series_fwd_lossfn(*head, *table, C.byref(ps), P("Ls"), ls_rows, C.byref(spec), *tail)

    def backward(how):
        head = (C.byref(sd), P("A"), P("Xs"))
        mid = (C.byref(ps), P("Y"), P("Ls"), ls_rows, grad_scale)
        tail = (P("stash"), P("loss_buf"), P("loss"), C.byref(gs), P("ws"), ws_bytes, st)
        if how == "plain":
            fn = lib.wgnn_series_bwd_mse_at if q.stride is None else lib.wgnn_series_bwd_mse
            return fn(*head, *strided, *mid, *tail)
        if how == "masked":
            return lib.wgnn_series_bwd_mse_masked(*head, *table, *mid, *tail)
        spec = L.LossFn(*(_spec(q) if how == "lossfn" else how))
        return lib.wgnn_series_bwd_lossfn(*head, *table, *mid, C.byref(spec), *tail)

    word[off // 4] = 0                                       # kernels only OR into the block: the caller zeroes it
    if gate is not None:
        assert fill == "zero" and not dirty and not status       # (re-poisoning with zeros is what clears the second status block)
        gate.begin(a, ints=("starts",))
    else:
        L.profile_enable(True)
    try:
        rc = forward(fwd)
        assert rc == 0, rc
        after("forward %r" % (fwd,))
        if gate is not None:
            gate.repoison(a["ws"], STATUS)
        elif "ws" not in dirty:
            a["ws"].poison()                                 # the workspace carries nothing from the forward to the backward
            word[off // 4] = 0
        rc = backward(bwd)
        assert rc == 0, rc
        after("backward %r" % (bwd,), status)
        names = tuple(rec["name"] for rec in L.profile_read()) if gate is None else ()
    finally:
        if gate is None:
            L.profile_enable(False)
    if gate is not None:
        gate.close(a, words=(0, off))
    outs = ["Y", "loss"] + GRADS
    if fill != "zero" and not dirty:
        spare = 0 if fwd not in ("plain", "masked") else 3       # the new forward writes its spec into the three spare words
        for name in outs + ["loss_buf"]:
            left = a[name].unwritten(4)
            if name == "loss_buf" and fwd == "plain" and lb_bytes == 4 * (3 * nb + 4):
                left -= nb                                       # (the unmasked forward in the longer buffer leaves the counts)
            assert left == (spare if name == "loss_buf" else 0), (name, fill, left)
    for name in ("A", "Xs", "Ls", "starts") + tuple("p." + k for k in PARAM_KEYS):      # inputs are read only
        assert a[name].unwritten(1) == a[name].nbytes, name
    out = {name: a[name].host() for name in outs}
    lb = a["loss_buf"].host()
    out["stats"] = lb.view(torch.int32)[:2 * nb].clone()                                 # sums | maxima, as bits
    out["tag"] = lb.view(torch.int32)[2 * nb:2 * nb + 4].clone()
    if lb_bytes == 4 * (3 * nb + 4):
        out["counts"] = lb.view(torch.int32)[2 * nb + 4:].clone()
    return out, names, {k: a[k].host() for k in ("stash", "ws", "loss_buf")}


def _f32(b, shape):
    return b.view(torch.float32).reshape(shape)


def _grads(q, out):
    return {k: _f32(out["g." + k], q.gm[k].shape) for k in PARAM_KEYS}


def _errors(q, out, loss_o=None, gm=None):
    loss_o, gm = q.loss_o if loss_o is None else loss_o, q.gm if gm is None else gm
    err = {"Y": rel_to_max(_f32(out["Y"], (q.n, q.T, q.H)), q.Yo),
           "loss": abs(float(_f32(out["loss"], (1,))[0]) - loss_o) / loss_o}
    for k, g in _grads(q, out).items():
        err[k] = rel_to_max(g, gm[k])
    return err


def _assert_bar(what, err):
    print("\n%s: worst %.2e  " % (what, max(err.values())) + "  ".join("%s %.2e" % kv for kv in err.items()))
    for k, e in err.items():
        assert e <= (LOSS_TOL if k.startswith("loss") else TOL), (what, k, e)


def _assert_finite(what, out, q):
    for k, g in _grads(q, out).items():
        assert torch.isfinite(g).all(), (what, k, "a gradient element is NaN or infinite")
    assert torch.isfinite(_f32(out["Y"], (q.n, q.T, q.H))).all(), what


def _assert_names(q, names, tag="lossfn"):
    """The instances of this H, row mapping and tag ran, and no sibling (nor the other mapping's) did."""
    tag = (",starts" if q.stride is None else "") + ("," + tag if tag else "")
    want = {"gru_fwd_kernel<%d%s>" % (sc.fwd_ks(q.H), tag), "gru_bwd_kernel<%d%s>" % (sc.bwd_ks3(q.H), tag),
            "series_fold_at_kernel" if q.stride is None else "series_fold_kernel"}
    rec = {x for x in names if x.startswith(("gru_fwd_kernel", "gru_bwd_kernel", "series_fold"))}
    assert rec == want, (rec, want)
    assert ("series_starts_check_kernel" in names) == (q.stride is None), names


@functools.lru_cache(maxsize=None)
def _checked(*case):
    q = lc.reference(*case)
    if not q.base.endswith("_big"):
        assert q.margin > 1e-5, "a ReLU pre-activation within %.1e of zero (relative): pick another seed" % q.margin
    return q


# ---- 1. with MSE from step 0 the new pair IS the old ones ---------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["table", "stride2"])
def test_mse_from_step_0_is_bit_identical_to_the_unmasked_and_the_masked_pair(how):
    """{MSE, 0, 0} against wgnn_series_fwd_loss + _bwd_mse (mask e), {MSE, 0, 1} against the masked pair (masks e and b): Y, the
    partial sums and maxima, the loss, the 8 gradients and the count words are torch.equal; delta is ignored."""
    for mask, old, masked in (("e", "plain", 0), ("e", "masked", 1), ("b", "masked", 1)):
        q = _checked("irregular", how, mask, "mse", 0.0, 0)
        want, names0, _ = _arena_step(q, old)
        _assert_names(q, names0, "masked" if old == "masked" else "")
        got, names1, _ = _arena_step(q, (0, 7.5 if mask == "b" else 0.0, 0, masked))
        _assert_names(q, names1)
        for key in ["Y", "loss", "stats"] + GRADS + (["counts"] if old == "masked" else []):
            assert torch.equal(got[key], want[key]), (how, mask, old, key)
        assert got["counts"].tolist() == q.counts and sum(q.counts) == q.m
        assert not torch.equal(got["tag"][:1], want["tag"][:1])                     # the same statistics under a third tag
        assert got["tag"][1:].tolist() == [masked << 8, 0, 0]                       # kind | masked << 8, delta's bits, t_from
        assert not torch.isnan(_f32(got["loss"], (1,))).any()
        _assert_bar("%s-%s-%s mse from 0" % (q.base, how, mask), _errors(q, got))


# ---- 2. oracle parity -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cid", list(lc.PARITY))
def test_lossfn_pair_matches_the_oracle_with_the_loss_formed_in_the_test(cid):
    q = _checked(*lc.PARITY[cid])
    out, names, _ = _arena_step(q)
    _assert_names(q, names)
    _assert_finite(cid, out, q)
    assert out["counts"].tolist() == q.counts, (cid, "per-workgroup counts", out["counts"].tolist(), q.counts)
    delta_bits = int(torch.tensor([q.delta], dtype=torch.float32).view(torch.int32)[0]) if q.kind == "huber" else 0
    assert out["tag"][1:].tolist() == [lc.KINDS[q.kind] | q.masked << 8, delta_bits, q.t_from], cid
    _assert_bar("%s (m = %d of %d)" % (cid, q.m, q.n * q.T * q.H), _errors(q, out))


# ---- 3. no label at all ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how,kind", [("table", "l1"), ("stride2", "huber")])
def test_without_any_label_the_loss_is_nan_the_gradients_are_zero_and_the_status_says_so(how, kind):
    q = _checked("irregular", how, "f", kind, lc.DELTA if kind == "huber" else 0.0, 2)
    assert q.m == 0 and q.masked == 1
    out, names, left = _arena_step(q, fill="finite", status=NO_LABELS)      # (not the NaN fill: the loss written is a NaN itself)
    _assert_names(q, names)
    assert torch.isnan(_f32(out["loss"], (1,))).all()
    for k, g in _grads(q, out).items():
        assert (g == 0).all(), (k, "not exactly zero")
    assert out["counts"].tolist() == [0] * len(q.counts)
    Y = _f32(out["Y"], (q.n, q.T, q.H))
    assert torch.isfinite(Y).all() and rel_to_max(Y, q.Yo) <= TOL                   # nothing non-finite anywhere else
    assert (_f32(out["stats"], (-1,)) == 0).all()                                   # sums and maxima over no label


# ---- 4. a backward must come with its forward's spec ---------------------------------------------------------------------------------
def test_a_mismatched_pairing_is_loud_in_every_direction():
    """Another kind, delta or t_from than the forward's; the two existing backwards on the new forward's buffer; the new backward
    on theirs: NaN loss and WGNN_STATUS_NO_LOSS_STATS (never WGNN_STATUS_NO_LABELS), and dY = 0 wherever the new or the masked
    backward runs."""
    q = _checked("irregular", "stride2", "b", "huber", lc.DELTA, 2)
    clean = q.clean                                                # (the unmasked backward must not meet a NaN label)
    base, _, _ = _arena_step(q, fill="finite")
    assert abs(float(_f32(base["loss"], (1,))[0]) - q.loss_o) <= LOSS_TOL * q.loss_o          # matched: quiet
    own = _spec(q)
    for fwd, bwd in ((own, _spec(q, kind=1)), (own, _spec(q, kind=0)), (own, _spec(q, delta=0.5)), (own, _spec(q, t_from=1)),
                     (own, _spec(q, masked=0)), (own, "masked"), ("masked", own), ("plain", own), (own, "plain"),
                     (_spec(q, masked=0), "plain")):
        nan_free = "plain" in (fwd, bwd) or (isinstance(bwd, tuple) and not bwd[3])
        out, names, _ = _arena_step(q, fwd, bwd, fill="finite", status=NO_LOSS_STATS, Ls=clean if nan_free else None)
        assert torch.isnan(_f32(out["loss"], (1,))).all(), (fwd, bwd)
        if bwd != "plain":
            for k, g in _grads(q, out).items():
                assert (g == 0).all(), (fwd, bwd, k, "dY was not zero")
        torch.testing.assert_close(_f32(out["Y"], (q.n, q.T, q.H)), _f32(base["Y"], (q.n, q.T, q.H)), rtol=0, atol=0)
    # the unmasked forward's loss_buf at its OWN length (no count words behind the spare ones): the new backward, masked or
    # not, refuses it on the tag alone, loads nothing past its end, and writes nothing there (the guard)
    for masked in (1, 0):
        out, _, _ = _arena_step(q, "plain", _spec(q, masked=masked), fill="finite", status=NO_LOSS_STATS, Ls=clean, short_buf=True)
        assert torch.isnan(_f32(out["loss"], (1,))).all() and "counts" not in out
        for k, g in _grads(q, out).items():
            assert (g == 0).all(), (masked, k, "dY was not zero")
    # MSE and L1 ignore delta: another one still pairs
    l1 = _checked("irregular", "stride2", "b", "l1", 0.0, 2)
    out, _, _ = _arena_step(l1, _spec(l1, delta=0.5), _spec(l1, delta=3.0), fill="finite")
    assert abs(float(_f32(out["loss"], (1,))[0]) - l1.loss_o) <= LOSS_TOL * l1.loss_o


# ---- 5. grad_scale -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,mask", [("l1", "e"), ("huber", "b")])
def test_grad_scale_halves_every_gradient_exactly_and_leaves_the_loss(kind, mask):
    q = _checked("irregular", "table", mask, kind, lc.DELTA if kind == "huber" else 0.0, 2)
    one, _, _ = _arena_step(q)
    half, _, _ = _arena_step(q, grad_scale=0.5)
    assert torch.equal(one["loss"], half["loss"]) and torch.equal(one["Y"], half["Y"])
    for k in PARAM_KEYS:
        g1, gh = _f32(one["g." + k], (-1,)), _f32(half["g." + k], (-1,))
        assert torch.equal(gh, 0.5 * g1) and float(g1.abs().max()) > 0, k


# ---- 6. Huber with every residual in the quadratic arm is half the mean square -----------------------------------------------------
def test_huber_with_a_delta_above_every_residual_is_half_of_mse():
    q = _checked("irregular", "table", "b", "mse", 0.0, 2)
    assert float((q.Yo - torch.nan_to_num(q.L.double())).abs().max()) < 4.0
    out, names, _ = _arena_step(q, (2, 4.0, 2, 1))
    _assert_names(q, names)
    _assert_bar("huber delta 4 against mse / 2", _errors(q, out, 0.5 * q.loss_o, {k: 0.5 * g for k, g in q.gm.items()}))


# ---- 7. footprint ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("how,kind", [("table", "huber"), ("stride2", "l1")])
def test_footprint_guards_fills_and_dirty_scratch(how, kind):
    q = _checked("irregular", how, "b", kind, lc.DELTA if kind == "huber" else 0.0, 2)
    assert FILLS[0] == "zero"
    base, _, _ = _arena_step(q, fill=FILLS[0])
    _assert_bar("arena zero %s %s" % (how, kind), _errors(q, base))
    for fill in FILLS[1:] + FILLS[1:2]:                                             # (and a second run of one: torch.equal)
        out, _, _ = _arena_step(q, fill=fill)
        for key, v in out.items():
            assert torch.equal(v, base[key]), (key, fill)
    _, _, left = _arena_step(_checked(*lc.PARITY["K8_small-stride2-e-huber-from1"]), fill="nan")   # another shape's scratch
    for fill in ("finite", "nan"):
        out, _, _ = _arena_step(q, fill=fill, dirty=left)
        for key, v in out.items():
            assert torch.equal(v, base[key]), (key, fill, "dirty")


# ---- 8. TrainStep.step_series(loss=...) ------------------------------------------------------------------------------------------------
STEPS = 3
TRAIN = {"l1": ("l1", 0.0, 0), "huber": ("huber", lc.DELTA, 2)}


@functools.lru_cache(maxsize=None)
def _trajectory(name, mask, max_norm=None):
    """The oracle's STEPS Adam steps on the irregular table with the loss of TRAIN[name] under `mask`: (losses, parameters after,
    the unclipped gradient norms).  max_norm: torch.nn.utils.clip_grad_norm_'s coefficient on the gradients before Adam."""
    from oracle import windgnn_oracle as orc
    kind, delta, t_from = TRAIN[name]
    q = _checked("irregular", "table", mask, kind, delta, t_from)
    A, X, L = q.A.double(), q.X.double(), q.L.double()
    p = dict(q.p64)
    state = orc.adam_init(p)
    losses, norms = [], []
    for _ in range(STEPS):
        Y, cache = orc.forward(A, X, p)
        loss, dY, _ = lc.loss_and_dy(Y, L, kind, delta, t_from, q.masked)
        losses.append(float(loss))
        g = orc.backward(A, X, p, Y, cache, dY)
        norms.append(float(torch.sqrt(sum((v ** 2).sum() for v in g.values()))))
        if max_norm is not None:
            coef = min(1.0, max_norm / (norms[-1] + 1e-6))
            g = {k: v * coef for k, v in g.items()}
        p = orc.adam_step(p, g, state)
    return losses, p, norms


@pytest.mark.parametrize("name,mask,clip", [("l1", "e", False), ("l1", "b", True), ("huber", "e", False), ("huber", "b", False)])
def test_three_steps_follow_the_oracle_trajectory_and_repeat_bit_for_bit(name, mask, clip):
    from windgnn_amd.trainer import TrainStep
    kind, delta, t_from = TRAIN[name]
    q = _checked("irregular", "table", mask, kind, delta, t_from)
    max_norm = 0.5 * _trajectory(name, mask)[2][0] if clip else None                # half the first norm: the clip is active
    lo, po, norms = _trajectory(name, mask, max_norm)
    dev = _dev()
    A, Xs, Ls = q.A.to(dev), q.Xs.to(dev), q.Ls.to(dev)
    perm = torch.randperm(q.n, generator=torch.Generator().manual_seed(6)).tolist()
    table = torch.tensor([q.starts[i] for i in perm], device=dev)
    kw = dict(loss=kind, loss_from=t_from, missing_labels=bool(q.masked))
    if kind == "huber":
        kw["huber_delta"] = delta
    runs = []
    for _ in range(2):
        model = _model_of(q.r)
        tr = TrainStep(model, keep_best=True, **({"max_grad_norm": max_norm} if clip else {}))
        losses = []
        for s in range(STEPS):
            loss, Y = tr.step_series(A, Xs, Ls, q.T, starts=table, **kw)
            assert tuple(Y.shape) == (q.n, q.T, q.H) and loss.dim() == 0
            losses.append(float(loss))
            if s == 0:                                             # Y comes back in the table's order
                assert rel_to_max(Y.cpu(), q.Yo[perm]) <= TOL
                if clip:
                    norm, coef = float(tr.grad_norm), float(tr.clip_coef)
                    assert abs(norm - norms[0]) <= TOL * norms[0] and coef < 1 and abs(coef - max_norm / (norms[0] + 1e-6)) <= TOL
        assert tr.steps == STEPS and float(tr.best_loss) == min(losses)
        runs.append((losses, tr.flat_p.clone(), model))
    assert runs[0][0] == runs[1][0] and torch.equal(runs[0][1], runs[1][1])          # the same steps from the same state
    seen = {k: rel_to_max(p.detach().cpu(), po[k]) for k, p in runs[0][2].named_parameters()}
    for i, (a, b) in enumerate(zip(runs[0][0], lo)):
        seen["loss%d" % (i + 1)] = abs(a - b) / b
    _assert_bar("step_series(%s) x3" % ", ".join("%s=%r" % kv for kv in kw.items()), seen)


def test_forward_backward_series_strided_leaves_the_specs_gradients_in_the_bucket():
    from windgnn_amd.trainer import TrainStep
    s = _checked("irregular", "stride2", "b", "huber", lc.DELTA, 2)
    dev = _dev()
    tr = TrainStep(_model_of(s.r))
    loss, Y = tr.forward_backward_series(s.A.to(dev), s.Xs.to(dev), s.Ls.to(dev), s.T, 2, n_windows=s.n, missing_labels=True,
                                         loss="huber", huber_delta=lc.DELTA, loss_from=2)
    err = {"Y": rel_to_max(Y.cpu(), s.Yo), "loss": abs(float(loss) - s.loss_o) / s.loss_o}
    err.update({k: rel_to_max(g.cpu(), s.gm[k]) for k, g in zip(PARAM_KEYS, tr.g_views)})
    _assert_bar("forward_backward_series(loss='huber', loss_from=2, missing_labels=True)", err)
    assert tr.steps == 0
