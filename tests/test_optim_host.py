"""Host side of gradient clipping in the step tail (no GPU): include/windgnn_optim.h against _lib.EXPORTS_OPTIM, the exports of
the shared object, wgnn_clip_bytes, the refusals of wgnn_finish_norm / wgnn_finish_clipped before any launch, and
TrainStep(max_grad_norm=...)'s option checks."""
import ctypes
import os
import re
import socket

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from conftest import ROOT
from test_abi_and_host import _c_kind, _ctype_kind


def _lib():
    from windgnn_amd import _lib as L
    from windgnn_amd import build
    build.build(verbose=False)
    return L, L.load()


def _prototypes(header):
    """{name: (return type, [argument type strings])} of every wgnn_* function a header declares (the parse of
    tests/test_abi_and_host.py's _header_prototypes, on another file)."""
    hdr = open(os.path.join(ROOT, "include", header)).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", " ", hdr)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ \*]*?)\b(wgnn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr):
        ret, name, args = " ".join(m.group(1).split()), m.group(2), " ".join(m.group(3).split())
        protos[name] = (ret, [] if args in ("", "void") else [a.strip() for a in args.split(",")])
    return protos


def test_optim_prototypes_match_the_header_argument_for_argument():
    L, lib = _lib()
    protos = _prototypes("windgnn_optim.h")
    assert set(protos) == set(L.EXPORTS_OPTIM), set(protos) ^ set(L.EXPORTS_OPTIM)
    assert {"wgnn_optim_version", "wgnn_clip_bytes", "wgnn_finish_norm", "wgnn_finish_clipped"} == set(protos)
    for name, (ret, args) in protos.items():
        res, argtypes = L.EXPORTS_OPTIM[name]
        assert len(args) == len(argtypes), (name, args, argtypes)
        for i, (decl, t) in enumerate(zip(args, argtypes)):
            assert _c_kind(decl) == _ctype_kind(t), (name, i, decl, t)
        want = "ptr" if "*" in ret else {"int": "i32", "size_t": "size"}[ret.replace("const", "").strip()]
        assert _ctype_kind(res) == want, (name, ret, res)
        assert hasattr(lib, name), name                      # exported by the shared object
        assert getattr(lib, name).argtypes == argtypes       # and bound by load()
    assert lib.wgnn_optim_version() == L.OPTIM_VERSION == 1
    hdr = open(os.path.join(ROOT, "include", "windgnn_optim.h")).read()
    assert re.search(r"#define\s+WGNN_OPTIM_VERSION\s+1\b", hdr) and '#include "windgnn.h"' in hdr


def test_the_first_header_and_its_table_are_as_they_were():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "windgnn.h")).read()
    declared = set(re.findall(r"\b(wgnn_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.EXPORTS)
    assert not (set(L.EXPORTS) & set(L.EXPORTS_OPTIM))
    assert lib.wgnn_version() == 122
    assert "clip" not in hdr.lower()
    from windgnn_amd import build
    assert any(h.endswith("windgnn_optim.h") for h in build.HEADERS)


REFUSED = [(0, 24, 34, 13, 102, 0, 0, 0), (4, 24, 34, 12, 102, 0, 0, 0), (4, 24, 65, 13, 195, 0, 0, 0),
           (4, 24, 4096, 13, 12288, 0, 1, 0), (4, 24, 34, 13, 102, 0, 2, 0), (4, 24, 34, 13, 102, 4, 0, 0),
           (4, 24, 34, 13, 102, 0, 0, 0, 1), (4, 24, 200, 13, 60, 1, 1, 1000, 2)]


def test_clip_bytes():
    L, lib = _lib()
    sizes = []
    for math in (L.MATH_F32, L.MATH_F16X3, L.MATH_F16, L.MATH_F16X3G):
        d = L.Dims(4, 24, 34, 13, 102, math, 0, 0)
        n = lib.wgnn_clip_bytes(ctypes.byref(d))
        # two result floats and at least one partial sum per 256 elements of the which = 0 pass over the 167 440 gradients
        assert n >= 256 + 4 * (167440 // 256) and n % 256 == 0, (math, n)
        sizes.append(n)
    wide = L.Dims(4, 3, 100, 13, 160, L.MATH_F16X3, 1, 600)                # CSR + wide GRU
    assert lib.wgnn_clip_bytes(ctypes.byref(wide)) > 256
    assert lib.wgnn_clip_bytes(ctypes.byref(L.Dims(4, 3, 100, 13, 160, L.MATH_F32, 1, 600))) > 256
    for spec in REFUSED:
        d = L.Dims(*spec)
        assert lib.wgnn_workspace_bytes(ctypes.byref(d)) == 0, spec
        assert lib.wgnn_clip_bytes(ctypes.byref(d)) == 0, spec
    assert lib.wgnn_clip_bytes(None) == 0
    from windgnn_amd.functional import clip_bytes
    assert clip_bytes(L.Dims(4, 24, 34, 13, 102, 1, 0, 0)) == sizes[1]


def test_norm_and_clipped_entry_points_refuse_before_any_launch():
    L, lib = _lib()
    V = ctypes.c_void_p
    d = L.Dims(4, 24, 34, 13, 102, 1, 0, 0)
    g, p, ad = L.Grads(), L.Params(), L.Adam()
    for i, n in enumerate(L._SLOTS):
        setattr(g, n, 0x9000000 + 0x100000 * i)
        setattr(p, n, 0x1000000 + 0x100000 * i)
        setattr(ad.exp_avg, n, 0x2000000 + 0x100000 * i)
        setattr(ad.exp_avg_sq, n, 0x3000000 + 0x100000 * i)
    ad.step = 1
    clip, ws, big = V(0x4000000), V(0xE000000), 1 << 40
    bd = ctypes.byref
    # NULL arguments
    assert lib.wgnn_finish_norm(bd(d), None, 6, 1.0, clip, ws, big, None) == -1
    assert lib.wgnn_finish_norm(bd(d), bd(g), 6, 1.0, None, ws, big, None) == -1
    assert lib.wgnn_finish_norm(bd(d), bd(g), 6, 1.0, clip, None, big, None) == -1
    assert lib.wgnn_finish_norm(bd(d), bd(L.Grads()), 0, 1.0, clip, ws, big, None) == -1        # an empty slot
    assert lib.wgnn_finish_norm(None, bd(g), 6, 1.0, clip, ws, big, None) == -1
    for hole in range(5):
        args = [bd(d), bd(p), bd(g), bd(ad), clip, ws]
        args[hole] = None
        assert lib.wgnn_finish_clipped(*args, big, None) == -1, hole
    assert lib.wgnn_finish_clipped(bd(d), bd(p), bd(g), bd(ad), clip, None, big, None) == -1
    assert lib.wgnn_finish_clipped(bd(d), bd(L.Params()), bd(g), bd(ad), clip, ws, big, None) == -1
    # which: 0, 2, 4 or 6 only
    for which in (1, 8, 16, 7, 22, -2):
        assert lib.wgnn_finish_norm(bd(d), bd(g), which, 1.0, clip, ws, big, None) == -2, which
    # max_norm: > 0 (inf allowed: it is refused below for the workspace, not for the norm)
    for bad in (0.0, -1.0, float("nan"), -float("inf")):
        for which in (0, 6):
            assert lib.wgnn_finish_norm(bd(d), bd(g), which, bad, clip, ws, big, None) == -2, bad
    assert lib.wgnn_finish_norm(bd(d), bd(g), 6, float("inf"), clip, ws, 1024, None) == -4
    assert lib.wgnn_finish_norm(bd(d), bd(g), 0, 1.0, clip, ws, 1024, None) == -4
    assert lib.wgnn_finish_clipped(bd(d), bd(p), bd(g), bd(ad), clip, ws, 1024, None) == -4
    ad.step = 0
    assert lib.wgnn_finish_clipped(bd(d), bd(p), bd(g), bd(ad), clip, ws, big, None) == -2
    bad = L.Dims(4, 24, 34, 12, 102, 1, 0, 0)
    assert lib.wgnn_finish_norm(bd(bad), bd(g), 6, 1.0, clip, ws, big, None) == -2
    assert lib.wgnn_finish_clipped(bd(bad), bd(p), bd(g), bd(ad), clip, ws, big, None) == -2


def test_host_bindings_refuse_a_wrong_clip_buffer():
    from windgnn_amd import _lib as L
    from windgnn_amd.functional import finish_norm
    d = L.Dims(4, 24, 34, 13, 102, 1, 0, 0)
    grads = [torch.zeros(4)] * 8
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        finish_norm(d, grads, 6, 1.0, torch.zeros(1024))


def test_trainstep_max_grad_norm_option_checks_without_a_group():
    from windgnn_amd import GCN_GRU
    from windgnn_amd.trainer import TrainStep
    model = lambda: GCN_GRU(13, 13, 13, 7 * 13, 21)                     # noqa: E731
    for bad in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="max_grad_norm"):
            TrainStep(model(), max_grad_norm=bad)
    for ok in (1.0, float("inf"), 3):
        tr = TrainStep(model(), max_grad_norm=ok, carry_state=True)
        assert tr.max_grad_norm == float(ok)
        with pytest.raises(RuntimeError, match="no such step"):
            tr.grad_norm
    tr = TrainStep(model())
    assert tr.max_grad_norm is None
    with pytest.raises(RuntimeError, match="max_grad_norm=None"):
        tr.clip_coef


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _options_worker(rank, port, out_dir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK="0", WORLD_SIZE="1")
    dist.init_process_group("gloo", rank=0, world_size=1)
    from windgnn_amd import GCN_GRU
    from windgnn_amd.trainer import TrainStep
    grp = dist.group.WORLD
    out = []
    for kw in (dict(overlap_collectives=True), dict(grad_blocks=2), dict(grad_blocks="auto"), dict(), dict(carry_state=True)):
        try:
            tr = TrainStep(GCN_GRU(13, 13, 13, 7 * 13, 200), process_group=grp, max_grad_norm=1.0, **kw)
            out.append("accepted %r %r" % (tr.max_grad_norm, tr.plan))
        except RuntimeError as e:
            out.append(str(e).replace("\n", " "))
    with open(os.path.join(out_dir, "options.txt"), "w") as f:
        f.write("\n".join(out))
    dist.destroy_process_group()


def test_trainstep_max_grad_norm_refuses_the_schedules_that_step_before_the_bucket_is_whole(tmp_path):
    mp.spawn(_options_worker, args=(_free_port(), str(tmp_path)), nprocs=1, join=True)
    lines = open(os.path.join(str(tmp_path), "options.txt")).read().split("\n")
    assert "max_grad_norm" in lines[0] and "overlap_collectives=True" in lines[0] and "whole gradient bucket" in lines[0]
    assert "max_grad_norm" in lines[1] and "grad_blocks=2" in lines[1] and "whole gradient bucket" in lines[1]
    assert lines[2] == "accepted 1.0 None"                 # "auto" on a 0.9 MB bucket is the one-bucket schedule
    assert lines[3] == "accepted 1.0 None" and lines[4] == "accepted 1.0 None"
