"""Host side of keeping the best parameters on the device (no GPU): include/windgnn_best.h against _lib.EXPORTS_BEST, the exports
of the shared object, wgnn_best_bytes, every refusal of wgnn_best_init / wgnn_keep_best before any launch, and on a
CPU-constructed TrainStep the keep_best option checks that need no record and state_dict() / load_state_dict() against torch.optim.Adam."""
import copy
import ctypes
import os
import re

import pytest
import torch

from conftest import PARAM_KEYS, ROOT
from test_abi_and_host import _c_kind, _ctype_kind
from test_optim_host import REFUSED, _prototypes


def _lib():
    from windgnn_amd import _lib as L
    from windgnn_amd import build
    build.build(verbose=False)
    return L, L.load()


def test_best_prototypes_match_the_header_argument_for_argument():
    L, lib = _lib()
    protos = _prototypes("windgnn_best.h")
    assert set(protos) == set(L.EXPORTS_BEST), set(protos) ^ set(L.EXPORTS_BEST)
    assert {"wgnn_best_version", "wgnn_best_bytes", "wgnn_best_init", "wgnn_keep_best"} == set(protos)
    for name, (ret, args) in protos.items():
        res, argtypes = L.EXPORTS_BEST[name]
        assert len(args) == len(argtypes), (name, args, argtypes)
        for i, (decl, t) in enumerate(zip(args, argtypes)):
            assert _c_kind(decl) == _ctype_kind(t), (name, i, decl, t)
        want = "ptr" if "*" in ret else {"int": "i32", "size_t": "size"}[ret.replace("const", "").strip()]
        assert _ctype_kind(res) == want, (name, ret, res)
        assert hasattr(lib, name), name                      # exported by the shared object
        assert getattr(lib, name).argtypes == argtypes       # and bound by load()
    assert lib.wgnn_best_version() == L.BEST_VERSION == 1
    hdr = open(os.path.join(ROOT, "include", "windgnn_best.h")).read()
    assert re.search(r"#define\s+WGNN_BEST_VERSION\s+1\b", hdr) and '#include "windgnn.h"' in hdr


def test_the_other_headers_and_tables_are_as_they_were():
    L, lib = _lib()
    tables = [L.EXPORTS, L.EXPORTS_OPTIM, L.EXPORTS_SCHED, L.EXPORTS_EVAL, L.EXPORTS_BEST]
    for i, a in enumerate(tables):
        for b in tables[i + 1:]:
            assert not (set(a) & set(b)), set(a) & set(b)
    hdr = open(os.path.join(ROOT, "include", "windgnn.h")).read()
    assert set(re.findall(r"\b(wgnn_[a-z0-9_]+)\s*\(", hdr)) == set(L.EXPORTS)
    assert "wgnn_best" not in hdr and "wgnn_keep_best" not in hdr
    assert lib.wgnn_version() == 122 and lib.wgnn_optim_version() == 1 and lib.wgnn_eval_version() == 1
    from windgnn_amd import build
    assert any(h.endswith("windgnn_best.h") for h in build.HEADERS) and "best.hip" in build.SOURCES


def test_best_bytes_and_the_public_words():
    L, lib = _lib()
    n = lib.wgnn_best_bytes()
    assert n > 0 and n % 256 == 0
    from windgnn_amd.functional import best_bytes, best_word
    assert best_bytes() == n
    assert L.BEST_WORDS == {"best_loss": (0, "float64"), "best_step": (8, "int64"), "calls": (16, "int64"),
                            "improvements": (24, "int64"), "improved": (32, "int32")}
    rec = torch.zeros(n, dtype=torch.uint8)
    best_word(rec, "best_step").fill_(-1)                    # a view: the write lands in the record
    assert rec[8:16].tolist() == [255] * 8 and int(rec[:8].sum()) == 0 and int(rec[16:].sum()) == 0


def _structs(L, base_p=0x1000000, base_b=0x9000000):
    p, b = L.Params(), L.Params()
    for i, n in enumerate(L._SLOTS):
        setattr(p, n, base_p + 0x100000 * i)
        setattr(b, n, base_b + 0x100000 * i)
    return p, b


def test_best_entry_points_refuse_before_any_launch():
    L, lib = _lib()
    V, bd = ctypes.c_void_p, ctypes.byref
    d = L.Dims(4, 24, 34, 13, 102, 1, 0, 0)
    p, b = _structs(L)
    loss, rec = V(0x5000000), V(0x6000000)
    # wgnn_best_init
    assert lib.wgnn_best_init(None, 0.03, None) == -1
    assert lib.wgnn_best_init(rec, float("nan"), None) == -2
    assert lib.wgnn_best_init(None, float("nan"), None) == -1            # NULL is diagnosed first
    # NULL arguments
    ok = [bd(d), loss, bd(p), bd(b), 3, rec]
    for hole in (0, 1, 2, 3, 5):
        args = list(ok)
        args[hole] = None
        assert lib.wgnn_keep_best(*args, None) == -1, hole
    for n in L._SLOTS:                                                    # an empty tensor slot, on either side
        for which in (0, 1):
            q = _structs(L)
            setattr(q[which], n, None)
            assert lib.wgnn_keep_best(bd(d), loss, bd(q[0]), bd(q[1]), 3, rec, None) == -1, (n, which)
    assert lib.wgnn_keep_best(bd(d), loss, bd(L.Params()), bd(b), 3, rec, None) == -1
    # dims wgnn_workspace_bytes refuses
    for spec in REFUSED:
        bad = L.Dims(*spec)
        assert lib.wgnn_workspace_bytes(bd(bad)) == 0, spec
        assert lib.wgnn_keep_best(bd(bad), loss, bd(p), bd(b), 3, rec, None) == -2, spec
    # step < 0
    for step in (-1, -2 ** 40):
        assert lib.wgnn_keep_best(bd(d), loss, bd(p), bd(b), step, rec, None) == -2, step
    # best_p aliasing p: the same tensors, one tensor shared, and a partial overlap of w_ih (3 * 102 * 34 * 13 floats)
    assert lib.wgnn_keep_best(bd(d), loss, bd(p), bd(p), 3, rec, None) == -2
    q = _structs(L)
    q[1].conv1_bias = q[0].conv1_bias
    assert lib.wgnn_keep_best(bd(d), loss, bd(q[0]), bd(q[1]), 3, rec, None) == -2
    q = _structs(L)
    q[1].w_ih = q[0].w_ih + 4 * (3 * 102 * 34 * 13 - 1)                   # its first float is the source's last
    assert lib.wgnn_keep_best(bd(d), loss, bd(q[0]), bd(q[1]), 3, rec, None) == -2
    q[1].w_ih = q[0].w_ih - 4 * (3 * 102 * 34 * 13 - 1)                   # its last float is the source's first
    assert lib.wgnn_keep_best(bd(d), loss, bd(q[0]), bd(q[1]), 3, rec, None) == -2


def test_host_bindings_refuse_cpu_tensors():
    from windgnn_amd import _lib as L
    from windgnn_amd.functional import best_bytes, best_init, keep_best
    rec = torch.zeros(best_bytes(), dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        best_init(rec, 0.03)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        keep_best(L.Dims(1, 1, 7, 13, 21, 0, 1, 1), torch.zeros(()), [torch.zeros(4)] * 8, [torch.zeros(4)] * 8, 1, rec)


def _model():
    from windgnn_amd import GCN_GRU
    return GCN_GRU(13, 13, 13, 7 * 13, 21)


def test_trainstep_keep_best_option_checks():
    from windgnn_amd.trainer import TrainStep
    with pytest.raises(ValueError, match="keep_best"):
        TrainStep(_model(), keep_best=float("nan"))
    tr = TrainStep(_model())
    assert tr.keep_best is None and tr._best is None and tr._best_p is None
    for name in ("best_loss", "best_step", "improved"):
        with pytest.raises(RuntimeError, match="keep_best=None"):
            getattr(tr, name)
    with pytest.raises(RuntimeError, match="keep_best=None"):
        tr.best_state_dict()
    with pytest.raises(RuntimeError, match="keep_best=None"):
        tr.restore_best()
    assert tr.state_dict()["best"] is None
    assert TrainStep(_model(), keep_best=False).keep_best is None          # off, not the threshold 0.0
    # a step held on the CPU cannot keep a record: the record is initialised by the library (tests/test_gpu_best.py goes on)
    for value in (True, 0.03):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            TrainStep(_model(), keep_best=value)


def test_state_dict_is_torch_adams_and_loads_both_ways():
    from windgnn_amd.trainer import TrainStep
    torch.manual_seed(3)
    model = _model()
    tr = TrainStep(model, lr=2e-3, betas=(0.8, 0.99), eps=1e-7)
    sd = tr.state_dict()
    assert set(sd) == {"optimizer", "steps", "best", "carry"} and sd["steps"] == 0 and sd["best"] is None and sd["carry"] is None
    fresh = torch.optim.Adam(model.parameters(), lr=2e-3, betas=(0.8, 0.99), eps=1e-7).state_dict()
    assert sd["optimizer"]["param_groups"] == fresh["param_groups"]      # every key this torch emits, params = [0..7]
    assert sd["optimizer"]["param_groups"][0]["params"] == list(range(8))
    assert sd["optimizer"]["param_groups"][0]["weight_decay"] == 0 and sd["optimizer"]["param_groups"][0]["amsgrad"] is False
    assert sorted(sd["optimizer"]["state"]) == list(range(8))
    for i, p in enumerate(model.parameters()):
        st = sd["optimizer"]["state"][i]
        assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and float(st["step"]) == 0.0
        assert st["exp_avg"].shape == p.shape and st["exp_avg_sq"].shape == p.shape
        assert st["exp_avg"].data_ptr() != tr.m_views[i].data_ptr()      # clones
    opt = torch.optim.Adam(model.parameters())
    opt.load_state_dict(sd["optimizer"])                                  # step 0 loads into torch's Adam
    assert opt.param_groups[0]["lr"] == 2e-3 and opt.param_groups[0]["betas"] == (0.8, 0.99)

    # two torch steps on planted gradients, then into the TrainStep: steps == 2, the moments bit for bit, in place
    g = torch.Generator().manual_seed(11)
    params = list(model.parameters())
    assert [p.data_ptr() for p in params] == [p.data_ptr() for p in tr.params]     # hot_path_parameters() order
    saved_grads = [p.grad for p in params]
    for _ in range(2):
        for p in params:
            p.grad = torch.randn(p.shape, generator=g)
        opt.step()
    for p, gv in zip(params, saved_grads):
        p.grad = gv
    m_ptrs = [m.data_ptr() for m in tr.m_views]
    tr.load_state_dict(opt.state_dict())
    assert tr.steps == 2 and (tr.lr, tr.betas, tr.eps) == (2e-3, (0.8, 0.99), 1e-7)
    assert [m.data_ptr() for m in tr.m_views] == m_ptrs
    for i, p in enumerate(params):
        assert torch.equal(tr.m_views[i], opt.state[p]["exp_avg"]) and torch.equal(tr.v_views[i], opt.state[p]["exp_avg_sq"])
        assert float(tr.m_views[i].abs().max()) > 0
    assert torch.equal(tr.exp_avg, torch.cat([opt.state[p]["exp_avg"].reshape(-1) for p in params]))
    # ... and back out: its own output loads, into itself and into torch
    sd = tr.state_dict()
    assert sd["steps"] == 2 and all(float(sd["optimizer"]["state"][i]["step"]) == 2.0 for i in range(8))
    other = TrainStep(_model())
    other.load_state_dict(sd)
    assert other.steps == 2 and torch.equal(other.exp_avg, tr.exp_avg) and torch.equal(other.exp_avg_sq, tr.exp_avg_sq)
    assert (other.lr, other.betas, other.eps) == (2e-3, (0.8, 0.99), 1e-7)
    torch.optim.Adam(_model().parameters()).load_state_dict(sd["optimizer"])
    # an Adam that never stepped: empty state = step 0, zero moments
    other.load_state_dict(torch.optim.Adam(_model().parameters()).state_dict())
    assert other.steps == 0 and float(other.exp_avg.abs().max()) == 0 and float(other.exp_avg_sq.abs().max()) == 0


def test_load_state_dict_refusals_name_the_tensor():
    from windgnn_amd.trainer import TrainStep
    model = _model()
    tr = TrainStep(model)
    opt = torch.optim.Adam(model.parameters())
    saved = [p.grad for p in model.parameters()]
    for p in model.parameters():
        p.grad = torch.ones_like(p)
    opt.step()
    for p, gv in zip(model.parameters(), saved):
        p.grad = gv
    good = opt.state_dict()
    before = tr.exp_avg.clone()

    sd = copy.deepcopy(good)      # (state_dict() shares the optimizer's own per-parameter dicts)
    sd["state"][5]["step"] = torch.tensor(4.0)
    with pytest.raises(ValueError, match=r"step.*disagree.*gru\.weight_hh_l0"):
        tr.load_state_dict(sd)
    sd = copy.deepcopy(good)      # (state_dict() shares the optimizer's own per-parameter dicts)
    sd["state"][4]["exp_avg"] = torch.zeros(63, 90)
    with pytest.raises(ValueError, match=r"exp_avg of gru\.weight_ih_l0 is \(63, 90\), expected \(63, 91\)"):
        tr.load_state_dict(sd)
    sd = copy.deepcopy(good)      # (state_dict() shares the optimizer's own per-parameter dicts)
    sd["state"][7]["exp_avg_sq"] = torch.zeros(62)
    with pytest.raises(ValueError, match=r"exp_avg_sq of gru\.bias_hh_l0"):
        tr.load_state_dict(sd)
    sd = copy.deepcopy(good)      # (state_dict() shares the optimizer's own per-parameter dicts)
    sd["param_groups"][0]["weight_decay"] = 0.01
    with pytest.raises(ValueError, match="weight_decay"):
        tr.load_state_dict(sd)
    assert tr.steps == 0 and torch.equal(tr.exp_avg, before)              # a refused load wrote nothing
    # a best record given to a keep_best=None step
    full = {"optimizer": good, "steps": 1, "carry": None,
            "best": dict({k: torch.zeros(()) for k in _lib()[0].BEST_WORDS}, **{k: torch.zeros(1) for k in PARAM_KEYS})}
    with pytest.raises(RuntimeError, match="keep_best=None"):
        tr.load_state_dict(full)
    assert tr.steps == 0 and torch.equal(tr.exp_avg, before)
    with pytest.raises(RuntimeError, match="carry_state=False"):
        tr.load_state_dict({"optimizer": good, "steps": 1, "best": None, "carry": torch.zeros(4, 21)})
    tr.load_state_dict(good)
    assert tr.steps == 1
