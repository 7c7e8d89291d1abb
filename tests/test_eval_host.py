"""Host side of the on-device evaluation statistics (no GPU): include/windgnn_eval.h against _lib.EXPORTS_EVAL, the exports of
the shared object, wgnn_eval_bytes, the refusals of wgnn_eval_accum / wgnn_eval_stats before any launch, the host bindings'
refusals, and the reference's three DataFrames from a hand-made stats tensor."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

from conftest import ROOT
from test_abi_and_host import _c_kind, _ctype_kind
from test_optim_host import _prototypes


def _lib():
    from windgnn_amd import _lib as L
    from windgnn_amd import build
    build.build(verbose=False)
    return L, L.load()


def test_eval_prototypes_match_the_header_argument_for_argument():
    L, lib = _lib()
    protos = _prototypes("windgnn_eval.h")
    assert set(protos) == set(L.EXPORTS_EVAL), set(protos) ^ set(L.EXPORTS_EVAL)
    assert {"wgnn_eval_version", "wgnn_eval_bytes", "wgnn_eval_accum", "wgnn_eval_stats"} == set(protos)
    for name, (ret, args) in protos.items():
        res, argtypes = L.EXPORTS_EVAL[name]
        assert len(args) == len(argtypes), (name, args, argtypes)
        for i, (decl, t) in enumerate(zip(args, argtypes)):
            assert _c_kind(decl) == _ctype_kind(t), (name, i, decl, t)
        want = "ptr" if "*" in ret else {"int": "i32", "size_t": "size"}[ret.replace("const", "").strip()]
        assert _ctype_kind(res) == want, (name, ret, res)
        assert hasattr(lib, name), name                      # exported by the shared object
        assert getattr(lib, name).argtypes == argtypes       # and bound by load()
    assert lib.wgnn_eval_version() == L.EVAL_VERSION == 1
    hdr = open(os.path.join(ROOT, "include", "windgnn_eval.h")).read()
    assert re.search(r"#define\s+WGNN_EVAL_VERSION\s+1\b", hdr) and '#include "windgnn.h"' in hdr


def test_the_other_headers_and_tables_are_as_they_were():
    L, lib = _lib()
    tables = [L.EXPORTS, L.EXPORTS_OPTIM, L.EXPORTS_SCHED, L.EXPORTS_EVAL]
    for i, a in enumerate(tables):
        for b in tables[i + 1:]:
            assert not (set(a) & set(b)), set(a) & set(b)
    hdr = open(os.path.join(ROOT, "include", "windgnn.h")).read()
    assert set(re.findall(r"\b(wgnn_[a-z0-9_]+)\s*\(", hdr)) == set(L.EXPORTS)
    assert "wgnn_eval" not in hdr
    assert lib.wgnn_version() == 122 and lib.wgnn_optim_version() == 1 and lib.wgnn_eval_version() == 1
    from windgnn_amd import build
    assert any(h.endswith("windgnn_eval.h") for h in build.HEADERS) and "eval.hip" in build.SOURCES


def test_eval_bytes():
    L, lib = _lib()
    for H in (0, -1, -102, -2 ** 31):
        assert lib.wgnn_eval_bytes(H) == 0, H
    for H in (1, 3, 21, 63, 64, 65, 102, 103, 4096, 12288, 12289, 1 << 20):
        n = lib.wgnn_eval_bytes(H)
        assert n >= 5 * 8 * H and n % 256 == 0, (H, n)
    from windgnn_amd.evaluate import eval_bytes
    assert eval_bytes(102) == lib.wgnn_eval_bytes(102) and eval_bytes(0) == 0


def test_eval_entry_points_refuse_before_any_launch():
    L, lib = _lib()
    V = ctypes.c_void_p
    pred, labels, acc, err, out = V(0x1000000), V(0x2000000), V(0x3000000), V(0x4000000), V(0x5000000)
    ok = dict(B=4, T=24, H=102)

    def accum(pred=pred, labels=labels, acc=acc, err=err, **kw):
        s = dict(ok, **kw)
        return lib.wgnn_eval_accum(pred, labels, s["B"], s["T"], s["H"], 0.0, 60.0, acc, err, None)
    assert accum(pred=None) == -1 and accum(labels=None) == -1 and accum(acc=None) == -1
    assert accum(pred=None, B=0) == -1                       # NULL is diagnosed whatever the shape
    for k in ("B", "T", "H"):
        for bad in (0, -1, -2 ** 31):
            assert accum(**{k: bad}) == -2, (k, bad)
            assert accum(err=None, **{k: bad}) == -2, (k, bad)
    assert lib.wgnn_eval_stats(None, 102, out, None) == -1
    assert lib.wgnn_eval_stats(acc, 102, None, None) == -1
    for bad in (0, -1, -2 ** 31):
        assert lib.wgnn_eval_stats(acc, bad, out, None) == -2, bad


def test_host_bindings_refuse_cpu_tensors_and_wrong_shapes():
    from windgnn_amd.evaluate import eval_accum, eval_stats
    pred, labels, acc = torch.zeros(2, 6), torch.zeros(2, 3, 6), torch.zeros(1024, dtype=torch.float64)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eval_accum(pred, labels, 0.0, 60.0, acc)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        eval_stats(acc, 6)


def test_evaluator_construction_and_frames_from_a_hand_made_stats_tensor():
    """Evaluator is constructible without a GPU (it allocates on the first update); the DataFrames are src/main.py:159-162's:
    columns RMSE, MAE, Average Accuracy, Accuracy Deviation, index = the station list, one frame per horizon."""
    import pandas as pd
    import windgnn_amd
    from windgnn_amd import GCN_GRU, Evaluator
    from windgnn_amd.evaluate import COL_LABELS, stats_frames
    assert "Evaluator" in windgnn_amd.__all__
    ev = Evaluator(GCN_GRU(13, 13, 13, 7 * 13, 21), torch.eye(7), 0.0, 60.0, keep_errors=True)
    assert (ev.H, ev.S, ev.acc) == (21, 7, None)
    assert tuple(ev.errors().shape) == (0, 21)
    ev.reset()
    with pytest.raises(RuntimeError, match="kept no error rows"):
        Evaluator(GCN_GRU(13, 13, 13, 7 * 13, 21), torch.eye(7), 0.0, 60.0).errors()
    with pytest.raises(ValueError, match="3 horizons"):
        Evaluator(GCN_GRU(13, 13, 13, 7 * 13, 20), torch.eye(7), 0.0, 60.0)
    S = 5
    stations = ["ST%02d" % i for i in range(S)]
    stats = torch.arange(3 * S * 4, dtype=torch.float32).view(3, S, 4)
    stats[1, 2, 2], stats[1, 2, 3] = float("-inf"), float("nan")
    frames = stats_frames(stats, stations)
    assert len(frames) == 3
    for k, df in enumerate(frames):
        assert isinstance(df, pd.DataFrame) and df.shape == (S, 4)
        assert list(df.columns) == COL_LABELS == ["RMSE", "MAE", "Average Accuracy", "Accuracy Deviation"]
        assert list(df.index) == stations
        assert np.array_equal(df.to_numpy(), stats[k].numpy(), equal_nan=True)
    assert frames[2].loc["ST03", "MAE"] == float(stats[2, 3, 1])
    csv = frames[0].to_csv()
    assert csv.splitlines()[0] == ",RMSE,MAE,Average Accuracy,Accuracy Deviation" and csv.splitlines()[1].startswith("ST00,")
    with pytest.raises(ValueError, match="stats_frames"):
        stats_frames(stats, stations[:-1])
    with pytest.raises(ValueError, match="stats_frames"):
        stats_frames(stats[0], stations)
