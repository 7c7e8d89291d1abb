"""The stream contract's bookkeeping (not collected by pytest: no test_ prefix).  tests/test_streams_host.py checks it on the
CPU, tests/test_gpu_streams.py runs it on the device; DESIGN.md section 2d has the method.

  STREAM_FLOWS       every exported function that takes `void* stream` -> the flow of test_gpu_streams.py that calls it
  stream_prototypes  the same set, read from the headers (name -> (position of the stream argument, number of arguments))
  RecordingLib       a proxy around the loaded library that notes the stream every such call was given
  blocker_ms ...     the rule that turns measured host enqueue times into the length of the blocker
  Gate               the measured run: poison, blocker, late inputs, "the host never waited"
"""
from __future__ import annotations

import ctypes as C
import gc
import math
import os
import re
import time

# entry point -> flow id (a key of test_gpu_streams.FLOWS).  An entry point that several flows reach is listed under the one
# that must call it; the flow's test asserts that it did, with the side stream's handle.
STREAM_FLOWS = {
    "wgnn_fwd": "fwd_bwd-small_odd",
    "wgnn_bwd": "fwd_bwd-small_odd",
    "wgnn_fwd_last": "fwd_last",
    "wgnn_fwd_loss": "loss_defer_adam",
    "wgnn_bwd_mse_part": "loss_defer_adam",
    "wgnn_finish": "loss_defer_adam",
    "wgnn_prepare_weights": "loss_defer_adam",
    "wgnn_finish_norm": "clip",
    "wgnn_finish_clipped": "clip",
    "wgnn_bwd_part": "bwd_parts",
    "wgnn_fwd_state": "state-f32_h129-h0",
    "wgnn_fwd_state_stash": "state-f32_h129-h0",
    "wgnn_bwd_state_part": "state-f32_h129-h0",
    "wgnn_bwd_rows": "rows",
    "wgnn_finish_rows": "rows",
    "wgnn_gru_fwd": "gru",
    "wgnn_gru_bwd": "gru",
    "wgnn_gcn_layer_fwd": "layer_dense",
    "wgnn_gcn_layer_bwd": "layer_dense",
    "wgnn_gcn_layer_csr_fwd": "layer_csr",
    "wgnn_gcn_layer_csr_bwd": "layer_csr",
    "wgnn_mse_loss_grad": "small_ops",
    "wgnn_adam_step": "small_ops",
    "wgnn_predict_last": "small_ops",
    "wgnn_make_windows": "small_ops",
    "wgnn_eval_accum": "eval",
    "wgnn_eval_accum_series": "eval",
    "wgnn_eval_stats": "eval",
    "wgnn_best_init": "best",
    "wgnn_keep_best": "best",
    "wgnn_series_fwd": "series_strided",
    "wgnn_series_bwd": "series_strided",
    "wgnn_series_fwd_last": "series_strided",
    "wgnn_series_fwd_loss": "series_strided_mse",
    "wgnn_series_bwd_mse": "series_strided_mse",
    "wgnn_series_fwd_at": "series_at",
    "wgnn_series_bwd_at": "series_at",
    "wgnn_series_fwd_last_at": "series_at",
    "wgnn_series_fwd_loss_at": "series_at_mse",
    "wgnn_series_bwd_mse_at": "series_at_mse",
    "wgnn_series_fwd_loss_masked": "series_masked",
    "wgnn_series_bwd_mse_masked": "series_masked",
    "wgnn_series_fwd_lossfn": "series_lossfn-huber",
    "wgnn_series_bwd_lossfn": "series_lossfn-huber",
    "wgnn_val_init": "series_val",
    "wgnn_val_begin": "series_val",
    "wgnn_series_val": "series_val",
    "wgnn_val_close": "series_val",
}

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")


def stream_prototypes(include_dir: str = INCLUDE) -> dict:
    """{name: (index of `void* stream`, number of arguments)} of every prototype in the headers whose argument list has one."""
    found = {}
    for fn in sorted(os.listdir(include_dir)):
        if not fn.endswith(".h"):
            continue
        with open(os.path.join(include_dir, fn)) as f:
            text = f.read()
        text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
        text = re.sub(r"//[^\n]*", " ", text)
        for m in re.finditer(r"\b(wgnn_\w+)\s*\(([^()]*)\)\s*;", text):
            args = [a.strip() for a in m.group(2).split(",")]
            hits = [i for i, a in enumerate(args) if re.fullmatch(r"void\s*\*\s*stream", a)]
            if hits:
                assert len(hits) == 1 and m.group(1) not in found, m.group(1)
                found[m.group(1)] = (hits[0], len(args))
    return found


def binding_tables(L) -> dict:
    """Every EXPORTS* table of windgnn_amd._lib merged: name -> (restype, argtypes)."""
    merged = {}
    for k, v in vars(L).items():
        if k.startswith("EXPORTS") and isinstance(v, dict):
            assert not (set(v) & set(merged)), k
            merged.update(v)
    return merged


def _handle(v) -> int:
    """What a ctypes call was given as a pointer argument, as an integer (NULL = 0)."""
    if v is None:
        return 0
    if isinstance(v, C.c_void_p):
        return v.value or 0
    return int(v)


class RecordingLib:
    """The loaded library with a note of every call of a stream-taking entry point: calls = [(name, stream handle)].
    Everything else passes through."""

    def __init__(self, lib, protos):
        self._lib, self._protos, self.calls = lib, protos, []

    def __getattr__(self, name):
        fn = getattr(self._lib, name)
        if name not in self._protos:
            return fn
        idx, nargs = self._protos[name]

        def call(*args):
            assert len(args) == nargs, (name, len(args), nargs)
            self.calls.append((name, _handle(args[idx])))
            return fn(*args)
        return call

    def check(self, flow: str, handle: int, allowed_null=()):
        """Every entry point the table gives to `flow` was called with `handle`; nothing but `allowed_null` ran on another."""
        assert handle != 0
        seen = {}
        for name, h in self.calls:
            seen.setdefault(name, set()).add(h)
        for name in (n for n, f in STREAM_FLOWS.items() if f == flow):
            assert handle in seen.get(name, ()), "%s: flow %s never called it on the side stream" % (name, flow)
        for name, hs in seen.items():
            if name not in allowed_null:
                assert hs == {handle}, "%s: called with streams %s, the side stream is %#x" % (name, sorted(hs), handle)


# ----------------------------------------------------------------------------------------------------------------- the blocker
BLOCKER_FACTOR = 10         # the blocker lasts this many times the longest host enqueue time of any flow
BLOCKER_STEP_MS = 5         # ... rounded up to a multiple of this


def blocker_ms(host_ms) -> int:
    """The rule: ten times the longest measured host enqueue time, rounded up to the next BLOCKER_STEP_MS."""
    worst = max(host_ms)
    assert worst > 0
    return int(math.ceil(BLOCKER_FACTOR * worst / BLOCKER_STEP_MS)) * BLOCKER_STEP_MS


def cycles_per_ms(c1: int, ms1: float, c2: int, ms2: float) -> float:
    """Two timed sleeps of c1 < c2 cycles: the slope, so that the launch overhead both carry drops out."""
    assert c2 > c1 and ms2 > ms1, (c1, ms1, c2, ms2)
    return (c2 - c1) / (ms2 - ms1)


def sleep_cycles(ms: float, rate: float) -> int:
    assert ms > 0 and rate > 0
    return int(math.ceil(ms * rate))


NAN_WORD = 0x7FC07FC0       # tests/guarded.py's NaN: one as fp32 and, half by half, as fp16 and bf16


def float_ranges(arena, ints=(), heads=None, status=("ws",)) -> list:
    """[lo, hi) byte ranges of the arena that the measured run poisons: everything (guard bands included: the image copy puts
    them back) except the buffers named in `ints` (index data, kept valid throughout) and the first heads[name] bytes of a
    buffer; the zero head of the buffers named in `status` (the status block of a workspace) is such a head.  Sorted,
    disjoint, multiples of 4."""
    heads = dict(heads or {})
    for b in arena.bufs.values():
        if b.zero_head and b.name in status:
            heads[b.name] = max(heads.get(b.name, 0), b.zero_head)
    keep = []
    for b in arena.bufs.values():
        if b.name in ints:
            keep.append((b.start // 4 * 4, -(-(b.start + b.nbytes) // 4) * 4))
        elif b.name in heads:
            keep.append((b.start // 4 * 4, -(-(b.start + min(heads[b.name], b.nbytes)) // 4) * 4))
    out, cur = [], 0
    for lo, hi in sorted(keep):
        if lo > cur:
            out.append((cur, lo))
        cur = max(cur, hi)
    total = arena.mem.numel()
    if total > cur:
        out.append((cur, total // 4 * 4))
    return out


class Gate:
    """One run of a flow on a side stream.  blocked = False: the warm-up (host enqueue time measured, nothing else).
    blocked = True: the measured run --

        begin(arena)   keep the committed image, poison every floating-point byte, synchronise; then on the stream: the
                       blocker, event e_block, the image copied back over the arena
        ... the flow enqueues everything on `handle` ...
        end()          event e_done; e_block must not have happened yet (the host waited nowhere); synchronise
    """

    def __init__(self, stream, blocked: bool, cycles: int = 0, limit_ms: float = 0.0):
        self.stream, self.blocked, self.cycles, self.limit_ms = stream, blocked, cycles, limit_ms
        self.handle = stream.cuda_stream
        self.host_ms = None

    def prepare(self, arena, ints=(), heads=None, status=("ws",)):
        """The measured run's first half (default stream, not synchronised): the image kept, the floats poisoned."""
        import torch
        if self.blocked:
            self.arena, self.image = arena, arena.mem.clone()
            words = arena.mem.view(torch.int32)
            for lo, hi in float_ranges(arena, ints, heads, status):
                words[lo // 4:hi // 4] = NAN_WORD

    def launch(self):
        """After a synchronise: blocker, e_block and the image copy on the stream; the host clock starts."""
        import torch
        if self.blocked:
            with torch.cuda.stream(self.stream):
                self.e_start = torch.cuda.Event(enable_timing=True)
                self.e_start.record(self.stream)
                torch.cuda._sleep(self.cycles)
                self.e_block = torch.cuda.Event(enable_timing=True)
                self.e_block.record(self.stream)
                self.arena.mem.copy_(self.image, non_blocking=True)
        gc.disable()                                      # (a collection in the middle of the calls is no wait for the stream)
        self.t0 = time.perf_counter()

    def begin(self, arena, ints=(), heads=None, status=("ws",)):
        import torch
        self.prepare(arena, ints, heads, status)
        if self.blocked:
            torch.cuda.synchronize()
        self.launch()

    def block_ms(self) -> float:
        """How long the blocker really lasted (after a synchronise)."""
        return self.e_start.elapsed_time(self.e_block)

    def repoison(self, buf, keep: int = 0):
        """buf back to what it held at commit(), past its first `keep` bytes (a status block keeps what the calls left in it);
        enqueued on the stream."""
        import torch
        a = buf.arena
        with torch.cuda.stream(self.stream):
            a.mem[buf.start + keep:buf.start + buf.nbytes].copy_(a.pristine[buf.start + keep:buf.start + buf.nbytes],
                                                                 non_blocking=True)

    def close(self, arena, words=(0,), buf="ws"):
        """end(), then what a runner on the null stream looks at after every call: guard bands intact, the status words
        (byte offsets into `buf`) 0."""
        import torch
        self.end()
        assert arena.check() == {}, arena.check()
        w = arena[buf].view(torch.int32)
        for off in words:
            assert int(w[off // 4]) == 0, ("status word at byte %d" % off, int(w[off // 4]))

    def end(self, sync=True):
        import torch
        self.host_ms = (time.perf_counter() - self.t0) * 1e3
        gc.enable()
        if self.blocked:
            e_done = torch.cuda.Event()
            e_done.record(self.stream)
            early = self.e_block.query()
            if sync:
                torch.cuda.synchronize()
            assert early is False, ("the blocker (%.0f ms) had already ended when the host came back from the last call, %.2f ms "
                                    "after the first: some call waited for the stream" % (self.limit_ms, self.host_ms))
        elif sync:
            torch.cuda.synchronize()
