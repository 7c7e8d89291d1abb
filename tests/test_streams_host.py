"""The stream contract's bookkeeping, on the CPU: tests/stream_cases.py's table covers every exported function that takes a
`void* stream` (no exceptions), each of them has a flow in tests/test_gpu_streams.py, the recording proxy can fail, the blocker
rule and the calibration arithmetic do what DESIGN.md 2d says, and the poison ranges spare exactly the index data and the
status block."""
import ctypes as C

import pytest
import torch

import stream_cases as sc
from guarded import Arena


def _L():
    from windgnn_amd import _lib
    return _lib


def test_the_table_is_exactly_the_exported_functions_that_take_a_stream():
    protos = sc.stream_prototypes()
    bound = sc.binding_tables(_L())
    assert len(protos) >= 48
    assert set(sc.STREAM_FLOWS) == set(protos), (sorted(set(protos) - set(sc.STREAM_FLOWS)), sorted(set(sc.STREAM_FLOWS) - set(protos)))
    for name, (idx, nargs) in protos.items():
        assert name in bound, "%s is declared with a stream and not bound in windgnn_amd/_lib.py" % name
        res, args = bound[name]
        assert res is C.c_int and len(args) == nargs and args[idx] is C.c_void_p, (name, idx, nargs, len(args))
    # the stream is the last argument, or the last but one in front of `int part`: nothing the proxy could mistake
    for name, (idx, nargs) in protos.items():
        assert idx == nargs - 1 or (idx == nargs - 2 and name.endswith("_part")), (name, idx, nargs)


def test_a_bound_function_with_no_declared_stream_takes_none():
    """The other direction: what the headers declare without a stream is host-only (sizes, versions, options, the profile)."""
    protos = sc.stream_prototypes()
    for name in set(sc.binding_tables(_L())) - set(protos):
        assert (name.endswith(("_bytes", "_version", "_offset", "_align")) or
                name in ("wgnn_strerror", "wgnn_set_option", "wgnn_get_option", "wgnn_profile_enable", "wgnn_profile_read",
                         "wgnn_tn_split")), name


def test_every_flow_of_the_table_is_defined_and_the_blocker_follows_the_rule():
    import test_gpu_streams as gs
    assert set(sc.STREAM_FLOWS.values()) <= set(gs.FLOWS)
    scenarios = {"py:%s-%s" % (name, size) for name in gs.SCENARIOS for size in gs.PY_SIZES}
    assert set(gs.HOST_MS) == set(gs.FLOWS) | {"two_streams"} | scenarios
    assert gs.BLOCKER_MS == sc.blocker_ms(gs.HOST_MS.values())
    assert 10 <= gs.BLOCKER_MS < 100                     # "tens of milliseconds"


def test_blocker_rule():
    assert sc.blocker_ms([0.2, 1.3, 0.9]) == 15          # 13 ms, up to the next 5
    assert sc.blocker_ms([1.5]) == 15                    # exactly on a step stays
    assert sc.blocker_ms([1.51]) == 20
    assert sc.blocker_ms([0.01]) == 5
    with pytest.raises(AssertionError):
        sc.blocker_ms([0.0])


def test_calibration_arithmetic():
    # 100 cycles per microsecond and 0.2 ms of launch overhead in both measurements: the slope does not see the overhead
    rate = sc.cycles_per_ms(2_000_000, 20.2, 20_000_000, 200.2)
    assert abs(rate - 100_000.0) < 1e-6
    assert sc.sleep_cycles(50, rate) == 5_000_000
    assert sc.sleep_cycles(0.00001, rate) == 1
    with pytest.raises(AssertionError):
        sc.cycles_per_ms(2_000_000, 20.0, 2_000_000, 21.0)
    with pytest.raises(AssertionError):
        sc.cycles_per_ms(2_000_000, 20.0, 20_000_000, 20.0)           # a clock that did not move


class _Fake:
    """Stands in for the loaded library: two stream-taking functions and one without."""

    def __init__(self):
        self.log = []

    def wgnn_fwd(self, *a):
        self.log.append("fwd")
        return 0

    def wgnn_bwd_part(self, *a):
        self.log.append("bwd_part")
        return 0

    def wgnn_workspace_bytes(self, d):
        return 4096


def test_the_recording_proxy_sees_a_null_stream_and_a_call_that_never_came(monkeypatch):
    protos = {"wgnn_fwd": (8, 9), "wgnn_bwd_part": (10, 12)}
    monkeypatch.setattr(sc, "STREAM_FLOWS", {"wgnn_fwd": "f", "wgnn_bwd_part": "f"})
    h = 0x7F00DEAD0000

    def proxy():
        fake = _Fake()
        return sc.RecordingLib(fake, protos), fake
    rec, fake = proxy()
    assert rec.wgnn_workspace_bytes(None) == 4096 and rec.calls == []
    rec.wgnn_fwd(*([None] * 8), C.c_void_p(h))
    rec.wgnn_bwd_part(*([None] * 10), h, 7)
    assert fake.log == ["fwd", "bwd_part"] and rec.calls == [("wgnn_fwd", h), ("wgnn_bwd_part", h)]
    rec.check("f", h)
    with pytest.raises(AssertionError, match="wrong number|9"):
        rec.wgnn_fwd(*([None] * 7), C.c_void_p(h))
    for null in (None, 0, C.c_void_p(0), C.c_void_p(None)):
        rec, _ = proxy()
        rec.wgnn_fwd(*([None] * 8), C.c_void_p(h))
        rec.wgnn_bwd_part(*([None] * 10), h, 7)
        rec.wgnn_bwd_part(*([None] * 10), null, 7)                       # one call of several on stream 0
        with pytest.raises(AssertionError, match="wgnn_bwd_part: called with streams"):
            rec.check("f", h)
        rec.check("f", h, allowed_null=("wgnn_bwd_part",))              # the positive control's exemption
    rec, _ = proxy()
    rec.wgnn_fwd(*([None] * 8), C.c_void_p(h))
    with pytest.raises(AssertionError, match="wgnn_bwd_part: flow f never called it"):
        rec.check("f", h)
    rec.check("another flow", h)


def test_poison_ranges_spare_the_index_data_and_the_status_block_only():
    a = Arena("cpu", "zero")
    a.buf("A", 404, data=torch.arange(101, dtype=torch.int32))           # a CSR blob
    a.buf("X", 1000, data=torch.rand(250))
    a.buf("acc", 4096, zero_head=800)                                    # an fp64 header that starts as zeros: floating point
    a.buf("ws", 8192, zero_head=256)
    a.buf("odd", 6, data=torch.zeros(3, dtype=torch.bfloat16), offset=2)
    a.commit()
    ranges = sc.float_ranges(a, ints=("A",))
    assert ranges == sorted(ranges) and all(lo % 4 == 0 and hi % 4 == 0 and lo < hi for lo, hi in ranges)
    assert all(a_hi <= b_lo for (_, a_hi), (b_lo, _) in zip(ranges, ranges[1:]))
    hit = torch.zeros(a.mem.numel(), dtype=torch.bool)
    for lo, hi in ranges:
        hit[lo:hi] = True
    spared = ~hit
    want = torch.zeros_like(spared)
    want[a["A"].start:a["A"].start + 404] = True
    want[a["ws"].start:a["ws"].start + 256] = True
    assert torch.equal(spared, want)
    # what the measured run does with them, and that the committed image undoes all of it
    image = a.mem.clone()
    words = a.mem.view(torch.int32)
    for lo, hi in ranges:
        words[lo // 4:hi // 4] = sc.NAN_WORD
    assert torch.equal(a["A"].bytes(), image[a["A"].start:a["A"].start + 404])
    assert torch.isnan(a["X"].view(torch.float32)).all() and torch.isnan(a["odd"].view(torch.bfloat16)).all()
    assert torch.isnan(a["ws"].bytes()[256:].view(torch.float32)).all() and int(a["ws"].bytes()[:256].max()) == 0
    assert a.check() != {}                                               # the guard bands are poisoned too ...
    a.mem.copy_(image)
    assert a.check() == {}                                               # ... and come back with the image
