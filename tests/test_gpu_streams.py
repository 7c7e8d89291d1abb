"""The stream contract (include/windgnn.h: "asynchronous and ordered on `stream` ... re-entrant across streams ... safe from any
host thread"): every exported call that takes a stream, on a side stream, behind a blocker, with inputs that arrive late.

For each flow (one per entry-point family, on the smallest case of the suite that reaches it):
  (a) the flow as the other modules run it: stream 0, zero fill;
  (b) once on a side stream (first-use allocations and attributes behind us); already bitwise (a);
  (c) a fresh arena, its committed image kept on the device; every floating-point byte of the arena overwritten with NaN;
      then on the side stream: a spinning blocker, event e_block, the image copied back, the whole flow.  When the last call
      has returned, e_block must not have happened (no call waited for the stream); after the synchronise the outputs are
      bitwise (a), the guard bands intact, the status word 0.
A launch or helper copy on any other stream ran on NaN or was overwritten by the image: it differs from (a).  Index data (CSR
blobs, `starts` tables) is never poisoned: nothing here can address out of bounds.  A recording proxy around the library
asserts that every entry point of tests/stream_cases.py's table was called with the side stream's handle and none with 0.
DESIGN.md section 2d has the method, the measured host enqueue times and what it cannot see."""
import ctypes as C
import gc
import threading
import time

import numpy as np
import pytest
import torch

import stream_cases as sc
import test_gpu_footprint as fp
from conftest import PARAM_KEYS
from guarded import Arena
from stream_cases import Gate

pytestmark = pytest.mark.gpu

# The blocker.  HOST_MS: the host time in ms each flow takes to enqueue, from the first call to the return of the last one, as step
# (b) -- the warm-up on the side stream -- measured it on an MI355X host (16 CPUs, one run of this module; every test prints
# its own figures again).  "py:" marks the scenarios of section 3; "two_streams" is the two-thread form of section 2, which has
# no warm-up of its own: the longest of its four measured runs.  BLOCKER_MS is stream_cases.blocker_ms() of the table: ten
# times the longest, rounded up to 5 ms (tests/test_streams_host.py holds the constant to the rule).  DESIGN.md 2d has the same
# table.
HOST_MS = {
    "fwd_bwd-small_odd": 0.194, "fwd_bwd-x3-33x1x19x100": 0.129, "fwd_bwd-f16": 0.118, "fwd_bwd-x3g_dgi1": 0.278,
    "fwd_bwd-csr-f16x3": 0.182, "fwd_bwd-io16-f16-bf16": 0.193, "fwd_last": 0.044, "bwd_parts": 0.135, "gru": 0.116,
    "loss_defer_adam": 0.174, "split_finish": 0.126, "clip": 0.264, "state-f32_h129-h0": 0.243, "state-x3-h0": 0.182,
    "state-small_odd-null": 0.179, "hourly_step": 0.025, "rows": 0.496, "layer_dense": 0.052, "layer_csr": 0.099,
    "small_ops": 0.095, "eval": 0.063, "best": 0.043, "series_strided": 0.206, "series_strided_mse": 0.097,
    "series_at": 0.172, "series_at_mse": 0.249, "series_masked": 0.121, "series_lossfn-mse": 0.127,
    "series_lossfn-l1": 0.133, "series_lossfn-huber": 0.131, "series_val": 0.088, "py:step-s7": 0.468,
    "py:step-s34": 0.496, "py:step_max_grad_norm-s7": 0.479, "py:step_max_grad_norm-s34": 0.496,
    "py:step_keep_best-s7": 0.479, "py:step_keep_best-s34": 0.889, "py:step_series_huber-s7": 0.509,
    "py:step_series_huber-s34": 0.487, "py:validate_series-s7": 0.316, "py:validate_series-s34": 0.349,
    "py:evaluator-s7": 0.306, "py:evaluator-s34": 0.311, "py:make_windows-s7": 0.076, "py:make_windows-s34": 0.080,
    "py:forward_last-s7": 0.139, "py:forward_last-s34": 0.155, "py:streaming_push-s7": 0.296,
    "py:streaming_push-s34": 0.380, "py:autograd-s7": 0.796, "py:autograd-s34": 0.603, "two_streams": 1.811,
    "py:make_windows_starts-s7": 0.255, "py:make_windows_starts-s34": 0.119, "py:forward_validated-s7": 0.328,
    "py:forward_validated-s34": 0.324, "py:step_series_table-s7": 1.816, "py:step_series_table-s34": 1.094,
    "py:validate_series_table-s7": 0.501, "py:validate_series_table-s34": 0.485,
}
BLOCKER_MS = 20


# ------------------------------------------------------------------------------------------------------------------- plumbing
@pytest.fixture(scope="module")
def side():
    fp._dev()
    return torch.cuda.Stream()


_RATE = []


def _cycles():
    """torch.cuda._sleep cycles of BLOCKER_MS, calibrated once with events (two lengths: the slope)."""
    if not _RATE:
        torch.cuda._sleep(1000)
        torch.cuda.synchronize()
        ms = []
        for cyc in (2_000_000, 20_000_000):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            torch.cuda._sleep(cyc)
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        _RATE.append(sc.cycles_per_ms(2_000_000, ms[0], 20_000_000, ms[1]))
        print("blocker: %.0f cycles per ms" % _RATE[0])
    return sc.sleep_cycles(BLOCKER_MS, _RATE[0])


def _gate(s, blocked):
    return Gate(s, blocked, _cycles() if blocked else 0, BLOCKER_MS)


class _recording:
    """windgnn_amd._lib.load() hands out a RecordingLib while this is open."""

    def __enter__(self):
        self.L = fp._lib()
        self.real = self.L.load()
        self.rec = sc.RecordingLib(self.real, sc.stream_prototypes())
        self.L._lib = self.rec
        return self.rec

    def __exit__(self, *exc):
        self.L._lib = self.real


def _same(ref, out, tag):
    assert set(ref) == set(out), (tag, sorted(ref), sorted(out))
    for n in ref:
        if not torch.equal(ref[n], out[n]):
            nd = int((ref[n] != out[n]).sum())
            raise AssertionError("%s: %s differs from the stream-0 run in %d of %d elements" % (tag, n, nd, ref[n].numel()))


# --------------------------------------------------------------------------------------------------------------------- flows
FLOWS = {}          # id -> f(gate or None) -> {name: host tensor}


def _run_flow(cid, flow, gate, spec=None, **kw):
    """A tests/test_gpu_footprint.py flow on one case: its Run on the gate's stream, (a)-(c) of that module at the end."""
    c = fp._build(cid, spec) if spec else fp._case(cid)
    r = fp.Run(c, "zero", stream=gate.stream if gate else None, **kw)
    if gate:
        gate.begin(r.a, ints=("A",) if c.k else ())
    names = flow(r)
    if gate:
        gate.end()
    res = r.collect(names)
    assert r.final_status() == 0, (cid, "status word", r.final_status())
    return res


def _reg(fid, cid, flow, **kw):
    FLOWS[fid] = lambda gate: _run_flow(cid, flow, gate, **kw)


for _cid in ("small_odd", "x3-33x1x19x100", "f16", "x3g_dgi1", "csr-f16x3", "io16-f16-bf16"):
    _reg("fwd_bwd-" + _cid, _cid, fp.flow_fwd_bwd)
_reg("fwd_last", "small_odd", fp.flow_fwd_last)
_reg("bwd_parts", "csr-f32", fp.flow_bwd_parts)
_reg("gru", "small_odd", fp.flow_gru, extra=(("dg", torch.float32, (5, 12, 7 * fp.F)),))


def _flow_loss_kept(r):
    assert r.prep_bytes > 0                               # this flow is here for wgnn_prepare_weights and the kept images
    return fp.FLOW_LOSS[(1, 1)](r)


_reg("loss_defer_adam", "x3-34x24x37x102", _flow_loss_kept)


def flow_split(r):
    """The data-parallel form: part 1 | 4 | DEFER, finish(4), part 2 | DEFER, finish(2), finish(0, adam)."""
    lib, d, gs, ps, D = r.lib, C.byref(r.d), r.grads(), r.params(), r.L.BWD_DEFER
    r.ok(lib.wgnn_fwd_loss(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("L"), r.ptr("Y"), r.ptr("stash"), *r.ws), "wgnn_fwd_loss")
    r.repoison_ws()
    for part, which in ((1 | 4 | 8 | D, 4), (2 | D, 2)):
        r.ok(lib.wgnn_bwd_mse_part(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("Y"), r.ptr("L"), C.c_float(1.0), r.ptr("loss"),
                                   r.ptr("stash"), C.byref(gs), *r.ws, part), "wgnn_bwd_mse_part(%d)" % part)
        r.ok(lib.wgnn_finish(d, C.byref(ps), C.byref(gs), which, None, *r.ws), "wgnn_finish(%d)" % which)
    ad = r.adam()
    r.ok(lib.wgnn_finish(d, C.byref(ps), C.byref(gs), 0, C.byref(ad), *r.ws), "wgnn_finish(0, adam)")
    return ["Y", "loss"] + fp.GRAD_NAMES + [pre + k for pre in ("p.", "m.", "v.") for k in PARAM_KEYS]


_reg("split_finish", "small_odd", flow_split)


def _flow_clip(r):
    import test_gpu_clip as tc
    return tc._clip_flow(r) + ["clip"]


def _clip(gate):
    import test_gpu_clip as tc
    cid = "clip-f16x3"
    c = fp._build(cid, tc.FOOT[cid])
    L = fp._lib()
    nclip = L.load().wgnn_clip_bytes(C.byref(L.Dims(c.B, c.T, c.S, 13, c.H, fp.MATH[c.math], 0, 0, 0)))
    return _run_flow(cid, _flow_clip, gate, spec=tc.FOOT[cid], extra=(("clip", torch.uint8, (nclip,)),))


FLOWS["clip"] = _clip


def _flow_state(given):
    """wgnn_fwd_state into buffers of its own, then wgnn_fwd_state_stash + wgnn_bwd_state_part(7); h0, dh_n and dh0 all given
    (hipMemcpyAsync of h0 into the stash) or all NULL (hipMemsetAsync); a general recurrence adds the hipMemcpy2DAsync rows."""
    def flow(r):
        lib, d, ps, gs = r.lib, C.byref(r.d), r.params(), r.grads()
        h0, dhn, dh0 = (r.ptr("h0"), r.ptr("dh_n"), r.ptr("dh0")) if given else (r.ptr(None),) * 3
        r.ok(lib.wgnn_fwd_state(d, r.ptr("A"), r.ptr("X"), C.byref(ps), h0, r.ptr("Y.inf"), r.ptr("h_n.inf"), *r.ws),
             "wgnn_fwd_state")
        r.repoison_ws()
        r.ok(lib.wgnn_fwd_state_stash(d, r.ptr("A"), r.ptr("X"), C.byref(ps), h0, r.ptr("Y"), r.ptr("h_n"), r.ptr("stash"),
                                      *r.ws), "wgnn_fwd_state_stash")
        r.repoison_ws()
        r.ok(lib.wgnn_bwd_state_part(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("Y"), r.ptr("dY"), dhn, r.ptr("stash"),
                                     C.byref(gs), dh0, *r.ws, 7), "wgnn_bwd_state_part")
        return ["Y.inf", "h_n.inf", "Y", "h_n"] + fp.GRAD_NAMES + (["dh0"] if given else [])
    return flow


def _state_extra(cid):
    _m, _io, _S, T, B, H, _k = fp.CASES[cid]
    return (("Y.inf", torch.float32, (B, T, H)), ("h_n.inf", torch.float32, (B, H)))


_reg("state-f32_h129-h0", "f32_h129", _flow_state(1), state=True, extra=_state_extra("f32_h129"))
_reg("state-x3-h0", "x3-34x24x37x102", _flow_state(1), state=True, extra=_state_extra("x3-34x24x37x102"))
_reg("state-small_odd-null", "small_odd", _flow_state(0), state=True, extra=_state_extra("small_odd"))


def flow_step(r):
    ps = r.params()
    r.ok(r.lib.wgnn_fwd_state(C.byref(r.d), r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("h0"), r.ptr("Y"), r.ptr("h_n"), *r.ws),
         "wgnn_fwd_state(T = 1)")
    return ["Y", "h_n"]


_reg("hourly_step", "step-B1-H102", flow_step, spec=("f32", torch.float32, 34, 1, 1, 102, 0))


def flow_rows(r):
    """tests/test_gpu_footprint.py's row-range sequence without its reads in between: part 1, two ranges of each GRU pair,
    part 2, wgnn_finish_rows on the same ranges."""
    L = r.L
    lib, d, ps, gs, ad = r.lib, C.byref(r.d), r.params("prepared" if r.prep_bytes else None), r.grads(), r.adam()
    G3 = 3 * r.c.H
    align = lib.wgnn_bwd_rows_align(d)
    assert align > 0
    first = align * max(1, (G3 // align) // 2)
    ranges = [(0, first), (first, G3 - first)]
    if r.prep_bytes:
        r.ok(lib.wgnn_prepare_weights(d, C.byref(ps), *r.ws), "wgnn_prepare_weights")
        r.repoison_ws()
    r.ok(lib.wgnn_fwd_loss(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("L"), r.ptr("Y"), r.ptr("stash"), *r.ws), "wgnn_fwd_loss")
    r.repoison_ws()
    r.ok(lib.wgnn_bwd_mse_part(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("Y"), r.ptr("L"), C.c_float(1.0), r.ptr("loss"),
                               r.ptr("stash"), C.byref(gs), *r.ws, 1 | 8), "wgnn_bwd_mse_part(1 | 8)")
    for which in (L.ROWS_IH, L.ROWS_HH):
        for row0, rows in ranges:
            r.ok(lib.wgnn_bwd_rows(d, r.ptr("Y"), r.ptr("stash"), C.byref(gs), which, row0, rows, *r.ws), "wgnn_bwd_rows")
    r.ok(lib.wgnn_bwd_mse_part(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("Y"), r.ptr("L"), C.c_float(1.0), r.ptr("loss"),
                               r.ptr("stash"), C.byref(gs), *r.ws, 2), "wgnn_bwd_mse_part(2)")
    for which in (L.ROWS_IH, L.ROWS_HH):
        for row0, rows in ranges:
            r.ok(lib.wgnn_finish_rows(d, C.byref(ps), C.byref(gs), which, row0, rows, C.byref(ad), *r.ws), "wgnn_finish_rows")
    return (["Y", "loss"] + fp.GRAD_NAMES + [pre + k for pre in ("p.", "m.", "v.") for k in PARAM_KEYS[4:]]
            + (["prepared"] if r.prep_bytes else []))


_reg("rows", "rows-f16x3", flow_rows)


# ---- entry points that take no wgnn_dims: buffers of their own in a plain arena
def _plain(gate, bufs, enqueue, outs, ints=()):
    """bufs: [(name, nbytes, data or None)]; enqueue(P, lib, st) issues the calls (P(name) -> pointer) and returns their codes."""
    a = Arena(fp._dev(), "zero")
    for name, n, data in bufs:
        a.buf(name, n, data=data)
    a.commit()
    if gate:
        gate.begin(a, ints=ints, status=())
    for rc in enqueue(lambda n: C.c_void_p(a[n].ptr) if n else C.c_void_p(0), fp._lib().load(), gate.handle if gate else None):
        assert rc == 0, rc
    if gate:
        gate.end()
    torch.cuda.synchronize()
    assert a.check() == {}, a.check()
    return {n: a[n].host() for n in outs}


def _layer(csr_k, nt, S, Fi, Fo):
    def flow(gate):
        from windgnn_amd.graph import CsrAdjacency, build_knn_adjacency, synthetic_station_coords
        lib = fp._lib().load()
        g = torch.Generator().manual_seed(77 + S + Fi + Fo)
        if csr_k:
            csr = CsrAdjacency(*build_knn_adjacency(synthetic_station_coords(S, seed=3), csr_k))
            A, nnz = csr.blob, csr.nnz
            wsb = lib.wgnn_gcn_layer_csr_workspace_bytes(nt, S, Fi)
        else:
            A, nnz = torch.rand(S, S, generator=g) / S + 0.01, 0
            wsb = lib.wgnn_gcn_layer_workspace_bytes(nt, S, Fi, Fo)
        X, W = torch.rand(nt, S, Fi, generator=g), torch.randn(Fi, Fo, generator=g) * 0.5
        b, dout = torch.randn(Fo, generator=g) * 0.1, torch.randn(nt, S, Fo, generator=g)
        bufs = [(n, t.numel() * 4, t) for n, t in (("A", A), ("X", X), ("W", W), ("b", b), ("dout", dout))]
        bufs += [("out", nt * S * Fo * 4, None), ("dW", Fi * Fo * 4, None), ("db", Fo * 4, None), ("dX", nt * S * Fi * 4, None),
                 ("ws", wsb, None)]

        def enqueue(P, lib, st):
            if csr_k:
                yield lib.wgnn_gcn_layer_csr_fwd(nt, S, Fi, nnz, P("A"), P("X"), P("W"), P("b"), P("out"), st)
                yield lib.wgnn_gcn_layer_csr_bwd(nt, S, Fi, nnz, P("A"), P("X"), P("W"), P("out"), P("dout"), P("dW"), P("db"),
                                                 P("dX"), P("ws"), C.c_size_t(wsb), st)
            else:
                yield lib.wgnn_gcn_layer_fwd(nt, S, Fi, Fo, P("A"), P("X"), P("W"), P("b"), P("out"), st)
                yield lib.wgnn_gcn_layer_bwd(nt, S, Fi, Fo, P("A"), P("X"), P("W"), P("out"), P("dout"), P("dW"), P("db"),
                                             P("dX"), P("ws"), C.c_size_t(wsb), st)
        return _plain(gate, bufs, enqueue, ["out", "dW", "db", "dX"], ints=("A",) if csr_k else ())
    return flow


FLOWS["layer_dense"] = _layer(0, 5, 34, 13, 40)
FLOWS["layer_csr"] = _layer(8, 5, 200, 13, 13)


def _small_ops(gate):
    """wgnn_mse_loss_grad, wgnn_adam_step, wgnn_predict_last and wgnn_make_windows (default starts, then a table)."""
    g = torch.Generator().manual_seed(11)
    n, na, (B, T, H), (Ttot, S, seq) = 1023, 169, (5, 12, 21), (131, 7, 12)
    Y, Lb = torch.rand(n, generator=g), torch.rand(n, generator=g)
    p, gr = torch.randn(na, generator=g), torch.randn(na, generator=g) * 1e-2
    m, v = torch.randn(na, generator=g) * 1e-3, torch.rand(na, generator=g) * 1e-4
    Yp = torch.rand(B, T, H, generator=g)
    feat = torch.rand(Ttot, S, fp.F, generator=g)
    t0 = [(i * 7) % (Ttot - seq - 3) for i in range(6)]
    Bd = Ttot // seq
    host = (C.c_int32 * len(t0))(*t0)
    bufs = [("Y", 4 * n, Y), ("L", 4 * n, Lb), ("dY", 4 * n, None), ("loss", 4, None), ("ws", 4096, None),
            ("p", 4 * na, p), ("g", 4 * na, gr), ("m", 4 * na, m), ("v", 4 * na, v),
            ("Yp", 4 * Yp.numel(), Yp), ("last", 4 * B * H, None),
            ("feat", 4 * feat.numel(), feat), ("starts", 4 * len(t0), torch.tensor(t0, dtype=torch.int32)),
            ("Xd", 4 * Bd * seq * S * fp.F, None), ("Ld", 4 * Bd * seq * 3 * S, None),
            ("Xt", 4 * len(t0) * seq * S * fp.F, None), ("Lt", 4 * len(t0) * seq * 3 * S, None)]

    def enqueue(P, lib, st):
        yield lib.wgnn_mse_loss_grad(P("Y"), P("L"), n, C.c_float(0.5), P("dY"), P("loss"), P("ws"), C.c_size_t(4096), st)
        yield lib.wgnn_adam_step(P("p"), P("g"), P("m"), P("v"), na, 3, C.c_float(1e-3), C.c_float(0.9), C.c_float(0.999),
                                 C.c_float(1e-8), st)
        yield lib.wgnn_predict_last(P("Yp"), B, T, H, C.c_float(-2.5), C.c_float(31.0), P("last"), st)
        yield lib.wgnn_make_windows(P("feat"), Ttot, S, fp.F, seq, 11, None, P(None), Bd, P("Xd"), P("Ld"), st)
        yield lib.wgnn_make_windows(P("feat"), Ttot, S, fp.F, seq, 11, host, P("starts"), len(t0), P("Xt"), P("Lt"), st)
    return _plain(gate, bufs, enqueue, ["dY", "loss", "p", "m", "v", "last", "Xd", "Ld", "Xt", "Lt"], ints=("starts",))


FLOWS["small_ops"] = _small_ops


def _eval(gate):
    """wgnn_eval_accum in one slice and in several, wgnn_eval_accum_series strided with skip_missing and on a table without,
    wgnn_eval_stats of each accumulator."""
    import test_gpu_eval as te
    import test_gpu_series_masked as tm
    lib = fp._lib().load()
    wind = te.WINDS[1]
    one, many = te._inputs(5, 2, 102, wind), te._inputs(1000, 2, 102, wind)
    es, et = tm._eval_inputs(70, 5, 21, "stride2"), tm._eval_inputs(70, 5, 21, "table")
    T = lambda a: torch.from_numpy(np.array(a))          # noqa: E731
    bufs = [("pred1", one[1].nbytes, T(one[1])), ("lab1", one[0].nbytes, T(one[0])),
            ("predN", many[1].nbytes, T(many[1])), ("labN", many[0].nbytes, T(many[0])),
            ("acc", lib.wgnn_eval_bytes(102), None), ("err1", 4 * 5 * 102, None), ("errN", 4 * 1000 * 102, None),
            ("out", 16 * 102, None),
            ("pred_s", es["pred"].nbytes, T(es["pred"])), ("Ls_s", es["Ls"].nbytes, T(es["Ls"])),
            ("acc_s", lib.wgnn_eval_bytes(21), None), ("err_s", 4 * 70 * 21, None), ("out_s", 16 * 21, None),
            ("pred_t", et["pred"].nbytes, T(et["pred"])), ("Ls_t", et["clean"].nbytes, T(et["clean"])),
            ("starts", 4 * 70, T(et["starts"])),
            ("acc_t", lib.wgnn_eval_bytes(21), None), ("out_t", 16 * 21, None)]

    def enqueue(P, lib, st):
        yield lib.wgnn_eval_accum(P("pred1"), P("lab1"), 5, 2, 102, wind[0], wind[1], P("acc"), P("err1"), st)
        yield lib.wgnn_eval_accum(P("predN"), P("labN"), 1000, 2, 102, wind[0], wind[1], P("acc"), P("errN"), st)
        yield lib.wgnn_eval_stats(P("acc"), 102, P("out"), st)
        yield lib.wgnn_eval_accum_series(P("pred_s"), P("Ls_s"), es["rows"], None, 2, 70, 5, 21, tm.WIND[0], tm.WIND[1], 1,
                                         P("acc_s"), P("err_s"), st)
        yield lib.wgnn_eval_stats(P("acc_s"), 21, P("out_s"), st)
        yield lib.wgnn_eval_accum_series(P("pred_t"), P("Ls_t"), et["rows"], P("starts"), 0, 70, 5, 21, tm.WIND[0], tm.WIND[1], 0,
                                         P("acc_t"), None, st)
        yield lib.wgnn_eval_stats(P("acc_t"), 21, P("out_t"), st)
    res = _plain(gate, bufs, enqueue, ["acc", "err1", "errN", "out", "acc_s", "err_s", "out_s", "acc_t", "out_t"], ints=("starts",))
    for n, H in (("acc", 102), ("acc_s", 21), ("acc_t", 21)):           # the public header; what lies behind it is private scratch
        res[n] = res[n][:40 * H].clone()
    return res


FLOWS["eval"] = _eval


def _best(gate):
    """wgnn_best_init, a wgnn_keep_best that wins (the 8 tensors are copied) and one that does not."""
    import test_gpu_best as tb
    S, H = 7, 21
    sizes = tb._sizes(S, H)
    N = sum(sizes)
    d = tb._dims(S, H, False)
    nrec = fp._lib().load().wgnn_best_bytes()
    base = (torch.arange(N, dtype=torch.float32) % 8191.0) * 1e-3 + 1.0
    bufs = [("p", 4 * N, base), ("best_p", 4 * N, None), ("record", nrec, None), ("loss", 8, torch.tensor([0.5, 0.7]))]

    def enqueue(P, lib, st):
        ps = tb._struct(P("p").value, sizes)
        bs = tb._struct(P("best_p").value, sizes)
        yield lib.wgnn_best_init(P("record"), float("inf"), st)
        yield lib.wgnn_keep_best(C.byref(d), P("loss"), C.byref(ps), C.byref(bs), 10, P("record"), st)
        yield lib.wgnn_keep_best(C.byref(d), C.c_void_p(P("loss").value + 4), C.byref(ps), C.byref(bs), 11, P("record"), st)
    res = _plain(gate, bufs, enqueue, ["best_p", "record"])
    assert tb._words(res["record"]) == dict(best_loss=0.5, best_step=10, calls=2, improvements=1, improved=0)
    return res


FLOWS["best"] = _best


def _series_strided(gate):
    import test_gpu_series as ts
    return ts._arena_run(ts._case("cover_1_2"), "zero", gate=gate)[0]


def _series_strided_mse(gate):
    import test_gpu_series as ts
    import test_gpu_series_train as tt
    return tt._arena_run(ts._case("cover_1_2"), tt._train("cover_1_2"), "zero", gate=gate)[0]


def _series_at(routes):
    def flow(gate):
        import test_gpu_series_at as ta
        out, _, _ = ta._arena_step(ta._checked("irregular"), fill="zero", routes=routes, gate=gate)
        return {route + "." + n: v for route, d in out.items() for n, v in d.items()}
    return flow


def _series_pair(case, fwd):
    def flow(gate):
        import test_gpu_series_lossfn as tl
        return tl._arena_step(tl._checked(*case), fwd, fill="zero", gate=gate)[0]
    return flow


def _series_val(gate):
    import test_gpu_series_val as tv
    out, records, _, _ = tv._val_run(tv._checked("irregular-table-b-huber-from2"), fill="zero", passes=2, gate=gate)
    assert int(records[-1]["passes"]) == 2 and int(records[-1]["calls"]) == 1
    return out


FLOWS["series_strided"] = _series_strided
FLOWS["series_strided_mse"] = _series_strided_mse
FLOWS["series_at"] = _series_at(("last", "series"))
FLOWS["series_at_mse"] = _series_at(("mse",))
FLOWS["series_masked"] = _series_pair(("irregular", "table", "b", "mse", 0.0, 0), "masked")
FLOWS["series_lossfn-mse"] = _series_pair(("irregular", "table", "b", "mse", 0.0, 2), "lossfn")
FLOWS["series_lossfn-l1"] = _series_pair(("irregular", "stride2", "e", "l1", 0.0, 2), "lossfn")
FLOWS["series_lossfn-huber"] = _series_pair(("irregular", "table", "b", "huber", 0.25, 2), "lossfn")
FLOWS["series_val"] = _series_val


def test_every_flow_of_the_table_exists():
    assert set(sc.STREAM_FLOWS.values()) <= set(FLOWS)


# ------------------------------------------------------------------------------------------------- 1. late inputs behind a blocker
@pytest.mark.parametrize("fid", list(FLOWS))
def test_flow_on_a_side_stream_behind_a_blocker(fid, side):
    flow = FLOWS[fid]
    ref = flow(None)                                                      # (a)
    with _recording() as rec:
        warm = _gate(side, False)
        _same(ref, flow(warm), fid + " [warm-up on the side stream]")      # (b)
        gate = _gate(side, True)
        t0 = time.perf_counter()
        out = flow(gate)                                                  # (c)
        wall = time.perf_counter() - t0
    print("%s: host enqueue %.3f ms (warm-up), %.3f ms (behind the blocker of %d ms, which lasted %.1f ms); measured run %.3f s"
          % (fid, warm.host_ms, gate.host_ms, BLOCKER_MS, gate.block_ms(), wall))
    _same(ref, out, fid + " [late inputs behind the blocker]")
    rec.check(fid, side.cuda_stream)


def _control(gate, misroute):
    """wgnn_fwd -> wgnn_mse_loss_grad on dense f32 (small_odd); misroute: the harness hands stream 0 to wgnn_mse_loss_grad
    alone, an elementwise kernel over Y, the labels and dY of this arena (n comes from the case: nothing is addressed by data)."""
    def flow(r):
        lib, d, ps = r.lib, C.byref(r.d), r.params()
        n = r.c.B * r.c.T * r.c.H
        r.ok(lib.wgnn_fwd(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("Y"), r.ptr("stash"), *r.ws), "wgnn_fwd")
        st = C.c_void_p(0) if misroute else r.stream
        r.ok(lib.wgnn_mse_loss_grad(r.ptr("Y"), r.ptr("L"), n, C.c_float(1.0), r.ptr("dY2"), r.ptr("loss"), r.ptr("ws2"),
                                    C.c_size_t(4096), st), "wgnn_mse_loss_grad")       # (its workspace is plain scratch)
        return ["Y", "dY2", "loss"]
    return _run_flow("small_odd", flow, gate, extra=(("dY2", torch.float32, (5, 12, 21)), ("ws2", torch.uint8, (4096,))))


def test_positive_control_a_call_on_stream_0_is_seen(side):
    """The method sees what it is there for: with wgnn_mse_loss_grad alone on the null stream (torch's side streams do not
    block it), dY / loss differ from the stream-0 run -- it ran on NaN, and the image copy then overwrote what it wrote."""
    ref = _control(None, False)
    _same(ref, _control(_gate(side, False), False), "control [warm-up]")
    _same(ref, _control(_gate(side, True), False), "control [rightly routed]")
    out = _control(_gate(side, True), True)
    differs = sorted(n for n in ref if not torch.equal(ref[n], out[n]))
    print("positive control: differs in", differs)
    assert torch.equal(ref["Y"], out["Y"])
    assert "dY2" in differs and "loss" in differs, differs


# -------------------------------------------------------------------------------------- 2. two streams at once, two host threads
PAIRS = {"two_cases": ("small_splitk", "x3-34x24x37x102"), "same_case": ("x3-34x24x37x102", "x3-34x24x37x102")}
_SOLO = {}


def _solo(cid):
    if cid not in _SOLO:
        _SOLO[cid] = _run_flow(cid, fp.FLOW_LOSS[(1, 1)], None)
    return _SOLO[cid]


@pytest.mark.parametrize("threads", [False, True], ids=["one_thread", "two_threads"])
@pytest.mark.parametrize("pair", list(PAIRS))
def test_two_streams_inside_the_library_at_once(pair, threads, side):
    """fwd_loss / bwd_mse_part(DEFER) / finish(6, adam) of two cases (other math mode, other dims, own arenas; or the same case
    twice: the same keys of every function-local `done` flag) on two side streams, each behind its own blocker, both queued
    completely before either blocker ends -- from one thread, then each from a thread of its own (ctypes drops the GIL: the
    host code of the library runs twice at once).  Each equals its solo stream-0 run bit for bit."""
    flow = fp.FLOW_LOSS[(1, 1)]
    cids = PAIRS[pair]
    refs = [_solo(cid) for cid in cids]
    streams = [side, torch.cuda.Stream()]
    for cid, s in zip(cids, streams):                                    # warm-up of each on its stream
        _same(_solo(cid), _run_flow(cid, flow, _gate(s, False)), "%s [warm-up]" % cid)
    runs = [fp.Run(fp._case(cid), "zero", stream=s) for cid, s in zip(cids, streams)]
    gates = [_gate(s, True) for s in streams]
    names, errors = [None, None], []
    for r, g in zip(runs, gates):
        g.prepare(r.a, ints=("A",) if r.c.k else ())
    torch.cuda.synchronize()
    for g in gates:
        g.launch()

    def drive(i):
        try:
            names[i] = flow(runs[i])
        except BaseException as e:      # noqa: BLE001 -- re-raised below, in the test's own thread
            errors.append(e)
    if threads:
        ts = [threading.Thread(target=drive, args=(i,)) for i in range(2)]
        for t in ts:
            t.start()
        for t in ts:
            t.join()
    else:
        drive(0)
        drive(1)
    early = []
    for g in gates:
        g.host_ms = (time.perf_counter() - g.t0) * 1e3
        early.append(g.e_block.query())
    gc.enable()                                                          # (Gate.launch switched it off)
    torch.cuda.synchronize()
    print("two_streams %s %s: host enqueue %.3f ms; blockers lasted %.1f and %.1f ms"
          % (pair, "two threads" if threads else "one thread", max(g.host_ms for g in gates), gates[0].block_ms(), gates[1].block_ms()))
    if errors:
        raise errors[0]
    assert early == [False, False], ("a blocker (%d ms) had ended before both flows were queued" % BLOCKER_MS, early,
                                     [g.host_ms for g in gates])
    for cid, r, nm, ref in zip(cids, runs, names, refs):
        _same(ref, r.collect(nm), "%s [%s, %s]" % (cid, pair, "two threads" if threads else "one thread"))
        assert r.final_status() == 0


# ------------------------------------------------------------------------------------- 3. the Python layer under torch.cuda.stream(s)
PY_SIZES = {"s7": (7, 12, 32, 21), "s34": (34, 24, 8, 102)}              # S, T, B, H
WIND = (1.5, 83.25)

# Calls that may wait for the stream on the host, each with the line that says so; for these the e_block assertion is left out
# (everything else is still checked).  Every other scenario asserts it.
DOCUMENTED_SYNC = {
    "forward_validated": "functional.check_range_status: 'one 4-byte device-to-host copy each, so a synchronisation' (GCN_GRU with "
                         "validate=True calls it after every forward of an fp16-plane mode)",
}


class _Py:
    """Host tensors of one size: adjacency, windows, labels, a series with its label series, a feature table, parameters."""

    def __init__(self, size):
        from oracle import windgnn_oracle as orc
        S, T, B, H = self.dims = PY_SIZES[size]
        g = torch.Generator().manual_seed(515 + S + H)
        rows = T + B - 1
        self.host = {"A": torch.rand(S, S, generator=g) / S + 0.01, "X": torch.rand(B, T, S, fp.F, generator=g),
                     "L": torch.rand(B, T, H, generator=g), "Xs": torch.rand(rows, S, fp.F, generator=g),
                     "Ls": torch.rand(rows, H, generator=g), "feat": torch.rand(5 * T + 7, S, fp.F, generator=g),
                     "W": torch.randn(B, T, H, generator=g) * 1e-2}
        self.p = orc.init_params(S, fp.F, H, seed=S + H)

    def model(self, math):
        from windgnn_amd import GCN_GRU
        S, _T, _B, H = self.dims
        m = GCN_GRU(13, 13, 13, S * 13, H, math=math)
        m.load_state_dict({k: v.clone() for k, v in self.p.items()})
        return m.to(fp._dev())


_PY = {}


def _py(size):
    if size not in _PY:
        _PY[size] = _Py(size)
    return _PY[size]


def _trainer_outputs(tr):
    return {"p": tr.flat_p.clone(), "m": tr.exp_avg.clone(), "v": tr.exp_avg_sq.clone(), "g": tr._gbuf.clone()}


def _sc_step(**kw):
    def make(py):
        from windgnn_amd.trainer import TrainStep
        tr = TrainStep(py.model("f16x3"), **kw)

        def run(i):
            out = {}
            for k in range(2):
                loss, Y = tr.step(i["A"], i["X"], i["L"])
                out["loss%d" % k], out["Y%d" % k] = loss.clone(), Y.clone()
            if "max_grad_norm" in kw:
                out["norm"], out["coef"] = tr.grad_norm.clone(), tr.clip_coef.clone()
            if "keep_best" in kw:
                out["best"], out["best_p"] = tr._best.clone(), tr._best_p.clone()
            return dict(out, **_trainer_outputs(tr))
        return run
    return make


def _table(py):
    """A host table of window starts in no order, with a duplicate: uploaded (and sorted) inside the call."""
    B = py.dims[2]
    return [(5 * w) % B for w in range(B - 1)] + [0]


def _sc_step_series(table):
    def make(py):
        from windgnn_amd.trainer import TrainStep
        T = py.dims[1]
        tr = TrainStep(py.model("f32"))
        how = {"starts": _table(py)} if table else {"stride": 1}

        def run(i):
            out = {}
            for k in range(2):
                loss, Y = tr.step_series(i["A"], i["Xs"], i["Ls"], T, loss="huber", huber_delta=0.25, loss_from=2, **how)
                out["loss%d" % k], out["Y%d" % k] = loss.clone(), Y.clone()
            return dict(out, **_trainer_outputs(tr))
        return run
    return make


def _sc_validate_series(table):
    def make(py):
        from windgnn_amd.trainer import TrainStep
        T = py.dims[1]
        tr = TrainStep(py.model("f32"), keep_best=True, best_on="validation")
        first, second = ({"starts": _table(py)[:5]}, {"starts": _table(py)}) if table else ({"stride": 2}, {"stride": 1})

        def run(i):
            v0 = tr.validate_series(i["A"], i["Xs"], i["Ls"], T, more=True, **first).clone()
            v1 = tr.validate_series(i["A"], i["Xs"], i["Ls"], T, loss="l1", loss_from=1, **second).clone()
            return {"v0": v0, "v1": v1, "val": tr._val.clone(), "best": tr._best.clone(), "best_p": tr._best_p.clone()}
        return run
    return make


def _sc_evaluator(py):
    from windgnn_amd.evaluate import Evaluator
    model = py.model("f32")
    _S, T, _B, H = py.dims

    def run(i):
        ev = Evaluator(model, i["A"], *WIND, keep_errors=True)
        a = ev.update(i["X"], i["L"]).clone()
        b = ev.update_series(i["Xs"], i["Ls"], T, stride=1).clone()
        return {"pred": a, "pred_series": b, "header": ev.acc[:5 * H].clone(), "errors": ev.errors().clone()}
    return run


def _sc_make_windows(py):
    T = py.dims[1]

    def run(i):
        from windgnn_amd.data import make_windows
        X, L = make_windows(i["feat"], T)
        return {"X": X, "L": L}
    return run


def _sc_make_windows_starts(py):
    T = py.dims[1]
    starts = [(i * 7) % (4 * T) for i in range(6)]

    def run(i):
        from windgnn_amd.data import make_windows
        X, L = make_windows(i["feat"], T, starts=starts)
        return {"X": X, "L": L}
    return run


def _sc_forward_validated(py):
    model = py.model("f16x3")                            # validate=True: check_range_status after the forward

    def run(i):
        with torch.no_grad():
            return {"Y": model(i["A"], i["X"]).clone()}
    return run


def _sc_forward_last(py):
    model = py.model("f16x3")

    def run(i):
        from windgnn_amd.data import forward_last
        return {"last": forward_last(model, i["A"], i["X"], *WIND)}
    return run


def _sc_streaming(py):
    from windgnn_amd.streaming import StreamingForecaster
    model = py.model("f32")
    B = py.dims[2]

    def run(i):
        sf = StreamingForecaster(model, i["A"], *WIND, n_streams=B)
        out = {"hour%d" % t: sf.push(i["X"][:, t]).clone() for t in range(3)}
        out["state"] = sf.state
        return out
    return run


def _sc_autograd(py):
    model = py.model("f32")

    def run(i):
        model.zero_grad()
        out = model(i["A"], i["X"])
        (out * i["W"]).sum().backward()
        return dict({"Y": out.detach().clone()}, **{k: q.grad.clone() for k, q in model.named_parameters()})
    return run


# scenario -> (make(py) -> run(inputs on the device) -> outputs, uses the shared workspace,
#              the line that promises that no call of it waits for the device)
SCENARIOS = {
    "step": (_sc_step(), True, "trainer.py: 'The loss a step returns is a 0-dim VIEW of the bucket's header (no clone launch per step)'"),
    "step_max_grad_norm": (_sc_step(max_grad_norm=0.05), True, "functional.finish_norm: 'deterministic, no host synchronisation'"),
    "step_keep_best": (_sc_step(keep_best=True), True, "functional.keep_best: 'no host synchronisation'"),
    "step_series_huber": (_sc_step_series(False), True, "TrainStep.step_series: 'the loss is the same 0-dim VIEW of the bucket's header word'"),
    "step_series_table": (_sc_step_series(True), True, "series._starts_table: a host table is uploaded from pinned memory"),
    "validate_series": (_sc_validate_series(False), True, "TrainStep.validate_series: 'Nothing synchronises with the host.'"),
    "validate_series_table": (_sc_validate_series(True), True, "TrainStep.validate_series: 'Nothing synchronises with the host.'"),
    "evaluator": (_sc_evaluator, True, "evaluate.Evaluator: 'Nothing synchronises with the host before the caller reads a result.'"),
    "make_windows": (_sc_make_windows, False, "data.make_windows: one launch on the current stream"),
    "make_windows_starts": (_sc_make_windows_starts, False, "data.make_windows: the table is built on the host and copied"),
    "forward_validated": (_sc_forward_validated, True, "(none: see DOCUMENTED_SYNC)"),
    "forward_last": (_sc_forward_last, True, "data.forward_last: 'as one C-ABI call'"),
    "streaming_push": (_sc_streaming, True, "streaming.StreamingForecaster.push: exact fp32 reads no status word"),
    "autograd": (_sc_autograd, True, "modules.GCN_GRU.forward: only the fp16-plane modes with validate read the status word"),
}


def _py_outputs(out):
    return {k: v.detach().cpu().clone() for k, v in out.items()}


@pytest.mark.parametrize("size", list(PY_SIZES))
@pytest.mark.parametrize("name", list(SCENARIOS))
def test_python_layer_on_a_side_stream_behind_a_blocker(name, size, side):
    """The bindings under torch.cuda.stream(s): the same three runs as above from equal initial state.  The late inputs are
    every floating-point argument (NaN until a copy on s, behind the blocker, produces them); the parameters are real
    throughout.  Then: _Workspace holds a buffer for s and the default stream's buffer was not written."""
    from windgnn_amd.functional import _Workspace
    make, uses_ws, _promise = SCENARIOS[name]
    py, dev = _py(size), fp._dev()
    src = {k: v.to(dev) for k, v in py.host.items()}
    ref = _py_outputs(make(py)(src))                                                       # (a)
    torch.cuda.synchronize()
    key0, key = (dev.index, 0), (dev.index, side.cuda_stream)
    assert torch.cuda.current_stream().cuda_stream == 0
    before = _Workspace._bufs[key0].clone() if key0 in _Workspace._bufs else None
    with _recording() as rec:
        with torch.cuda.stream(side):                    # (b); a constructor's launches (wgnn_best_init) go to the stream it sees
            run = make(py)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            t0 = time.perf_counter()
            inp = {k: torch.empty_like(v).copy_(v) for k, v in src.items()}
            warm = run(inp)
            warm_ms = (time.perf_counter() - t0) * 1e3
        torch.cuda.synchronize()
        _same(ref, _py_outputs(warm), "%s-%s [warm-up on the side stream]" % (name, size))
        with torch.cuda.stream(side):                                                     # (c)
            run = make(py)
        inp = {k: torch.full_like(v, float("nan")) for k, v in src.items()}
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            torch.cuda._sleep(_cycles())
            e_block = torch.cuda.Event()
            e_block.record(side)
            gc.disable()
            t0 = time.perf_counter()
            for k, v in src.items():
                inp[k].copy_(v, non_blocking=True)
            out = run(inp)
            host_ms = (time.perf_counter() - t0) * 1e3
            early = e_block.query()
            gc.enable()
        torch.cuda.synchronize()
    print("%s-%s: host enqueue %.3f ms (warm-up), %.3f ms (behind the blocker of %d ms)" % (name, size, warm_ms, host_ms, BLOCKER_MS))
    if name not in DOCUMENTED_SYNC:
        assert early is False, ("the blocker (%d ms) had already ended when the host came back from the last call, %.2f ms after "
                                "the first: some call waited for the stream" % (BLOCKER_MS, host_ms))
    _same(ref, _py_outputs(out), "%s-%s [late inputs behind the blocker]" % (name, size))
    rec.check("(the python layer)", side.cuda_stream)
    assert rec.calls, "no entry point was called"
    if uses_ws:
        assert key in _Workspace._bufs, "no workspace was kept for the side stream"
        assert int(_Workspace._bufs[key][:4].view(torch.int32).item()) == 0
    if before is not None:
        assert torch.equal(_Workspace._bufs[key0], before), "the default stream's workspace was written"
