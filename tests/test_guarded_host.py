"""tests/guarded.py can fail: planted faults in small Python stand-ins for a kernel, on CPU tensors, are each reported with
the right buffer name and offset, and a well-behaved stand-in passes under all three fills.  Also: every entry point of
include/windgnn.h that takes a device pointer is called by tests/test_gpu_footprint.py."""
import os
import re

import pytest
import torch

from conftest import ROOT
from guarded import ALIGN, FILLS, GUARD, NAN_WORD, Arena, fill_bytes

CPU = torch.device("cpu")
N = 37                      # floats of the stand-in's input: 148 bytes, a ragged last 256-byte line


def _arena(fill, out_bytes=4 * N, scratch_bytes=1000):
    a = Arena(CPU, fill)
    x = torch.arange(N, dtype=torch.float32) * 0.25 - 3.0
    a.buf("x", 4 * N, data=x)
    a.buf("out", out_bytes)
    a.buf("scratch", scratch_bytes, zero_head=256)
    return a.commit()


def _good_kernel(a):
    """out = 2 x + 1 through a scratch copy that it writes before it reads."""
    s = a["scratch"].bytes()[256:256 + 4 * N].view(torch.float32)
    s.copy_(a["x"].view(torch.float32))
    a["out"].view(torch.float32).copy_(2.0 * s + 1.0)


def _raw(a, buf, rel):
    """The arena byte at `rel` bytes from the first byte of `buf` (what a stray store hits)."""
    return a.mem[a[buf].start + rel:a[buf].start + rel + 1]


@pytest.mark.parametrize("fill", FILLS)
def test_well_behaved_stand_in_passes(fill):
    a = _arena(fill)
    _good_kernel(a)
    assert a.check() == {}
    if fill != "zero":                                          # (under "zero" a result of 0.0 equals the fill)
        assert a["out"].unwritten(4) == 0
    assert torch.equal(a["out"].view(torch.float32), 2.0 * (torch.arange(N, dtype=torch.float32) * 0.25 - 3.0) + 1.0)
    assert int(a["scratch"].bytes()[:256].sum()) == 0          # the status block started out zero and nobody set a bit


def test_results_of_a_well_behaved_stand_in_are_bitwise_equal_across_fills():
    outs = []
    for fill in FILLS:
        a = _arena(fill)
        _good_kernel(a)
        outs.append(a["out"].host())
    assert torch.equal(outs[0], outs[1]) and torch.equal(outs[0], outs[2])


def test_layout_alignment_and_guard_widths():
    a = Arena(CPU, "zero")
    sizes = [1, 3, 255, 256, 257, 4096, 10]
    for i, n in enumerate(sizes):
        a.buf("b%d" % i, n)
    a.buf("odd", 6, offset=2)
    a.commit()
    prev_end = 0
    for b in a.bufs.values():
        assert (b.start - b.offset) % ALIGN == 0
        assert b.start - b.guard_lo >= GUARD and b.guard_lo == prev_end
        end = b.start + b.nbytes
        assert b.guard_hi - end >= GUARD and b.guard_hi >= (end + ALIGN - 1) // ALIGN * ALIGN + GUARD
        assert b.bytes().numel() == b.nbytes                    # the exact length, not a rounded one
        prev_end = b.guard_hi
    assert a["odd"].start % ALIGN == 2 and a["odd"].ptr % 4 == 2
    assert a.mem.numel() >= prev_end


def test_fill_patterns():
    z = fill_bytes("zero", 4096, CPU)
    assert int(z.sum()) == 0
    n = fill_bytes("nan", 4096, CPU)
    assert bool((n.view(torch.int32) == NAN_WORD).all())
    assert bool(n.view(torch.float32).isnan().all()) and bool(n.view(torch.float16).isnan().all())
    assert bool(n.view(torch.bfloat16).isnan().all())
    f = fill_bytes("finite", 1 << 20, CPU)
    v = f.view(torch.float32)
    assert bool(v.isfinite().all()) and float(v.abs().max()) <= 1.0001e4 and float(v.abs().min()) >= 0.9e-4
    assert bool((v < 0).any()) and bool((v > 0).any())
    assert bool(f.view(torch.float16).isfinite().all()) and bool(f.view(torch.bfloat16).isfinite().all())
    assert torch.equal(f, fill_bytes("finite", 1 << 20, CPU))                 # seeded: the same bytes every time
    assert not torch.equal(f, fill_bytes("finite", 1 << 20, CPU, seed=1))
    with pytest.raises(ValueError):
        fill_bytes("ones", 16, CPU)


@pytest.mark.parametrize("fill", FILLS)
def test_one_byte_just_behind_a_buffer_is_reported(fill):
    a = _arena(fill)
    _good_kernel(a)
    _raw(a, "out", 4 * N)[0] ^= 0x5A
    assert a.check() == {"out": {"back": (4 * N, 4 * N, 1)}}


@pytest.mark.parametrize("fill", FILLS)
def test_one_byte_just_in_front_of_a_buffer_is_reported(fill):
    a = _arena(fill)
    _good_kernel(a)
    _raw(a, "scratch", -1)[0] ^= 0x5A
    assert a.check() == {"scratch": {"front": (-1, -1, 1)}}


def test_a_write_3_kib_behind_a_buffer_is_reported():
    a = _arena("nan")
    _good_kernel(a)
    rel = 4 * N + 3 * 1024
    a.mem[a["x"].start + rel:a["x"].start + rel + 8] = 0         # a stray 8-byte store far behind the input
    assert a.check() == {"x": {"back": (rel, rel + 7, 8)}}


def test_a_buffer_whose_length_is_not_a_multiple_of_4():
    """An fp16 tensor of 37 elements: 74 bytes.  A kernel that stores whole 4-byte words writes 2 bytes past it."""
    a = Arena(CPU, "nan")            # (no byte of fp16 1.5 = 0x3E00 equals a byte of the fill)
    y = a.buf("y16", 2 * N)
    a.commit()
    assert y.nbytes == 74 and y.bytes().numel() == 74
    y.view(torch.float16).fill_(1.5)                             # exactly the buffer: fine
    assert a.check() == {} and y.unwritten(2) == 0
    a.mem[y.start:y.start + 76].view(torch.float16).fill_(1.5)   # 19 words
    assert a.check() == {"y16": {"back": (74, 75, 2)}}


@pytest.mark.parametrize("fill", ["finite", "nan"])
def test_an_output_left_partly_unwritten_keeps_its_poison(fill):
    a = _arena(fill)
    _good_kernel(a)
    a["out"].poison()
    a["out"].view(torch.float32)[:N - 3].fill_(7.0)              # a ragged last tile that is never stored
    assert a.check() == {}
    assert a["out"].unwritten(4) == 3
    if fill == "nan":
        assert int(a["out"].view(torch.float32).isnan().sum()) == 3


def test_a_result_that_depends_on_scratch_differs_between_fills():
    def bad_kernel(a):
        """Adds into a partial sum it never cleared."""
        s = a["scratch"].bytes()[256:256 + 4 * N].view(torch.float32)
        s.add_(a["x"].view(torch.float32))
        a["out"].view(torch.float32).copy_(s)

    outs = {}
    for fill in FILLS:
        a = _arena(fill)
        bad_kernel(a)
        assert a.check() == {}                                   # inside its buffers: only the comparison can see it
        outs[fill] = a["out"].host()
    assert not torch.equal(outs["zero"], outs["finite"])
    assert not torch.equal(outs["zero"], outs["nan"])
    assert bool(outs["nan"].view(torch.float32).isnan().all())


def test_scratch_can_be_repoisoned_between_two_calls_and_start_dirty():
    a = _arena("nan")
    _good_kernel(a)
    left = a["scratch"].host()
    assert not bool(a["scratch"].bytes()[256:256 + 4 * N].view(torch.float32).isnan().any())
    a["scratch"].poison()
    assert bool(a["scratch"].bytes()[256:].view(torch.int32).eq(NAN_WORD).all())
    assert int(a["scratch"].bytes()[:256].sum()) == 0
    # a second arena whose scratch starts with what the first one's call left behind
    b = Arena(CPU, "finite")
    b.buf("x", 4 * N, data=torch.ones(N))
    b.buf("out", 4 * N)
    b.buf("scratch", 1000, data=left, zero_head=256)
    b.commit()
    assert torch.equal(b["scratch"].host(), left)
    _good_kernel(b)
    assert b.check() == {} and torch.equal(b["out"].view(torch.float32), torch.full((N,), 3.0))


# ---------------------------------------------------------------------------------------------------------------- coverage
NO_DEVICE_POINTER = {"wgnn_version", "wgnn_strerror", "wgnn_set_option", "wgnn_get_option", "wgnn_profile_enable",
                     "wgnn_profile_read"}


def test_footprint_file_calls_every_entry_point_that_takes_a_device_pointer():
    header = open(os.path.join(ROOT, "include", "windgnn.h")).read()
    body = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    protos = set(re.findall(r"\b(wgnn_[a-z0-9_]+)\s*\(", body))
    assert len(protos) >= 35, sorted(protos)
    src = open(os.path.join(ROOT, "tests", "test_gpu_footprint.py")).read()
    called = set(re.findall(r"\blib\.(wgnn_[a-z0-9_]+)\(", src))
    missing = sorted(protos - called - NO_DEVICE_POINTER)
    print("entry points the footprint file never calls:", missing)
    assert missing == []
