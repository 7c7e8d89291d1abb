"""Host side of the K splits of the two GRU weight-gradient GEMMs and their one-launch form (no GPU): include/windgnn_sched.h against
_lib.EXPORTS_SCHED, and wgnn_tn_split over a sweep of B*T from 1 to 131 072 -- positive splits, chunk lengths that are whole
32-row K steps, no more workgroups than an MI355X has CUs, the 64-row floor of small B*T, and the option key."""
import ctypes
import os
import re

import pytest

from conftest import ROOT
from test_abi_and_host import _c_kind, _ctype_kind

MATH = {"f32": 0, "f16x3": 1, "f16": 2, "f16x3g": 3}


def _lib():
    from windgnn_amd import _lib as L
    from windgnn_amd import build
    build.build(verbose=False)
    return L, L.load()


def test_sched_prototypes_match_the_header_argument_for_argument():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "windgnn_sched.h")).read()
    assert '#include "windgnn.h"' in hdr
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ \*]*?)\b(wgnn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr):
        protos[m.group(2)] = (" ".join(m.group(1).split()), [a.strip() for a in " ".join(m.group(3).split()).split(",")])
    assert set(protos) == set(L.EXPORTS_SCHED) == {"wgnn_tn_split"}
    assert not (set(L.EXPORTS_SCHED) & (set(L.EXPORTS) | set(L.EXPORTS_OPTIM)))
    for name, (ret, args) in protos.items():
        res, argtypes = L.EXPORTS_SCHED[name]
        assert len(args) == len(argtypes), (name, args, argtypes)
        for i, (decl, t) in enumerate(zip(args, argtypes)):
            assert _c_kind(decl) == _ctype_kind(t), (name, i, decl, t)
        assert ret == "int" and res is ctypes.c_int
        assert hasattr(lib, name) and getattr(lib, name).argtypes == argtypes
    fields = re.search(r"typedef struct wgnn_tn_split_info \{(.*?)\}", hdr, flags=re.S).group(1)
    names = [n.strip() for n in fields.replace("int32_t", "").replace(";", "").split(",")]
    assert names == [n for n, _ in L.TnSplitInfo._fields_]
    from windgnn_amd import build
    assert any(h.endswith("windgnn_sched.h") for h in build.HEADERS)


def test_option_key_is_known_and_defaults_to_the_merged_launch():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "windgnn.h")).read()
    assert re.search(r"#define\s+WGNN_OPT_TN_MERGED\s+6\b", hdr) and re.search(r"#define\s+WGNN_OPT_COUNT\s+7\b", hdr)
    assert L.OPT_TN_MERGED == 6
    assert L.get_option(L.OPT_TN_MERGED) == 1
    assert L.set_option(L.OPT_TN_MERGED, 0) == 1 and L.get_option(L.OPT_TN_MERGED) == 0
    assert L.set_option(L.OPT_TN_MERGED, 1) == 0
    assert lib.wgnn_set_option(L.OPT_TN_MERGED, 2) < 0 and lib.wgnn_set_option(7, 0) < 0
    assert L.get_option(L.OPT_TN_MERGED) == 1


def test_retired_option_keys_are_unknown_and_the_live_ones_keep_their_defaults():
    """Keys 1, 2, 3 and 5 named schedules that never measured better than the defaults and were removed with their code paths:
    the library refuses them, neither the header nor the bindings name them, and their numbers are not reused.  The live keys
    0, 4 and 6 answer 1 in a fresh process (key 0 takes its initial value from WGNN_FUSED_FWD: unset in the child)."""
    import subprocess
    import sys
    L, lib = _lib()
    WGNN_ERR_SHAPE = -2
    for k in (1, 2, 3, 5):
        assert lib.wgnn_set_option(k, 0) == WGNN_ERR_SHAPE, k
        assert lib.wgnn_get_option(k) == WGNN_ERR_SHAPE, k
    hdr = open(os.path.join(ROOT, "include", "windgnn.h")).read()
    assert re.search(r"WGNN_ERR_SHAPE\s*=\s*-2\b", hdr)
    keys = {m.group(1): int(m.group(2)) for m in re.finditer(r"#define\s+WGNN_OPT_(\w+)\s+(\d+)\b", hdr)}
    assert keys == {"FUSED_FWD": 0, "BIG_GEMM": 4, "TN_MERGED": 6, "COUNT": 7}, keys
    opts = {n: getattr(L, n) for n in dir(L) if n.startswith("OPT_")}               # the bindings name the live keys only
    assert opts == {"OPT_FUSED_FWD": 0, "OPT_BIG_GEMM": 4, "OPT_TN_MERGED": 6}, opts
    code = ("import sys; sys.path.insert(0, %r); from windgnn_amd import _lib as L; "
            "print('options', L.get_option(0), L.get_option(4), L.get_option(6))" % ROOT)
    env = {k: v for k, v in os.environ.items() if k != "WGNN_FUSED_FWD"}
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                       text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    assert [l for l in r.stdout.splitlines() if l.startswith("options")] == ["options 1 1 1"], r.stdout


def _bt_sweep():
    """B*T from 1 to 131 072: every small value, then powers of two and their neighbours, then odd strides."""
    vals = set(range(1, 300))
    for e in range(8, 18):
        vals.update({2 ** e - 1, 2 ** e, 2 ** e + 1, 2 ** e + 33})
    vals.update(range(300, 131072, 1777))
    vals.add(131072)
    return sorted(v for v in vals if v <= 131072)


@pytest.mark.parametrize("math", ["f16x3", "f16x3g", "f16"])
@pytest.mark.parametrize("S,H", [(34, 102), (7, 20), (64, 102), (34, 127), (1, 1)])
def test_split_sweep(S, H, math):
    L, lib = _lib()
    tiles_ih = -(-3 * H // 320) * -(-(S * 13 + 1) // 224)
    cus = 256                                                                         # MI355X: what the splits are made for
    for BT in _bt_sweep():
        T = 24 if BT % 24 == 0 else (3 if BT % 3 == 0 else 1)
        for state in (False, True):
            i = L.tn_split(L.Dims(BT // T, T, S, 13, H, MATH[math], 0, 0), state=state)
            tag = (S, H, math, BT, state, i.sk_ih, i.sk_hh)
            assert i.sk_ih >= 1 and i.sk_hh >= 1, tag
            for sk, kc in ((i.sk_ih, i.kchunk_ih), (i.sk_hh, i.kchunk_hh)):
                assert kc >= 32 and kc % 32 == 0 and sk * kc >= BT, tag         # whole K steps that cover every row
                assert sk == 1 or BT // sk >= 64, tag                           # the 64-row floor of small B*T
            # one launch, workgroup w takes item w of each product: as many workgroups as the longer list, at most one per CU
            assert i.merged == 1, tag
            assert max(tiles_ih * i.sk_ih, i.sk_hh) <= i.workgroups <= cus, tag   # (dW_hh has at least one tile)
    # the same dims give the same answer (the layout is a pure function of the dims)
    d = L.Dims(4096, 24, S, 13, H, MATH[math], 0, 0)
    a, b = L.tn_split(d), L.tn_split(d)
    assert (a.sk_ih, a.sk_hh, a.workgroups) == (b.sk_ih, b.sk_hh, b.workgroups)


def test_paths_without_the_merged_launch():
    """Exact fp32, and the wide-GRU path (H > 127: no register-resident recurrence), run one launch per product."""
    L, lib = _lib()
    for dims in (L.Dims(256, 24, 34, 13, 102, MATH["f32"], 0, 0), L.Dims(64, 3, 100, 13, 160, MATH["f16x3"], 1, 600)):
        i = L.tn_split(dims)
        assert i.merged == 0 and i.sk_ih >= 1 and i.sk_hh >= 1
    assert lib.wgnn_tn_split(None, 0, ctypes.byref(L.TnSplitInfo())) < 0
    assert lib.wgnn_tn_split(ctypes.byref(L.Dims(4, 24, 34, 13, 102, 1, 0, 0)), 0, None) < 0
    assert lib.wgnn_tn_split(ctypes.byref(L.Dims(0, 24, 34, 13, 102, 1, 0, 0)), 0, ctypes.byref(L.TnSplitInfo())) < 0
