"""Every kernel instance the launchers can select, on the MI355X: one case per instance key of tests/instance_cases.py.  A case
runs one step under the library's profiler, proves by the launched names that its instance (and the siblings its hidden
arguments imply) really ran, and compares the step with the fp64 reference at the suite's own tolerances: Y, the loss and the
8 gradients of orc.train_step, or Y, h_n, the 8 gradients and dh0 of tests/test_gpu_state_train.py's fp64 model for the
carried-state entry points.  16-bit inputs are rounded before the reference sees them.

Cases that share dims share the reference (functools.lru_cache, never written to), and cases that share the whole call form
share the GPU step: the table claims each key once, but one step launches about eight tabled kernels."""
import functools
import re

import pytest
import torch

import instance_cases as ic
from conftest import PARAM_KEYS, max_abs, rel_to_max
from test_gpu_parity import F16_G_TOL, F16_Y_TOL, G_TOL, Y_TOL
from test_gpu_state_train import IO_ROUND, MATH, _fp64_model, _tols

pytestmark = pytest.mark.gpu

IODT = {"f32": torch.float32, "f16": torch.float16, "bf16": torch.bfloat16}
TABLED = set(ic.FAMILIES) - {"pgemm_tn2_kernel"}          # kernel base names (the merged launch is named pgemm_tn_kernel<..>)


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _draw(S, T, B, H, io, state):
    """The suite's inputs for one shape, rounded to the I/O type: A, X, the labels and the model, and for the carried-state
    entry points tests/test_gpu_state_train.py's h0, dY and dh_n behind them."""
    from oracle import windgnn_oracle as orc
    iodt = IODT[io]
    g = torch.Generator().manual_seed(31 * S + 7 * T + B + 101 * H)
    A = torch.rand(S, S, generator=g) / S + 0.01
    X = torch.rand(B, T, S, 13, generator=g).to(iodt)
    L = torch.rand(B, T, H, generator=g).to(iodt)
    d = dict(A=A, X=X, L=L, p=orc.init_params(S, 13, H, seed=ic.param_seed(S, H)))
    if state:
        d["h0"] = torch.rand(B, H, generator=g) * 1.6 - 0.8
        d["dY"] = torch.randn(B, T, H, generator=g) * 1e-3
        d["dhn"] = torch.randn(B, H, generator=g) * 1e-3
    return d


@functools.lru_cache(maxsize=6)
def _reference(S, T, B, H, io, state):
    """The suite's inputs for one shape (rounded to the I/O type) and the fp64 reference's step on them."""
    from oracle import windgnn_oracle as orc
    d = _draw(S, T, B, H, io, state)
    A, X, L, p = d["A"], d["X"], d["L"], d["p"]
    if not state:
        Yo, loss_o, go = orc.train_step(A.double(), X.double(), L.double(), {k: v.double() for k, v in p.items()})
        return dict(A=A, X=X, L=L, p=p, Y=Yo, loss=float(loss_o), grads=go)
    h0, dY, dhn = d["h0"], d["dY"], d["dhn"]
    leaves, f = _fp64_model(p)
    h0r = h0.double().requires_grad_(True)
    Yr, hnr = f(A, X.float(), h0r)
    ((Yr * dY.double()).sum() + (hnr * dhn.double()).sum()).backward()
    return dict(A=A, X=X, p=p, h0=h0, dY=dY, dhn=dhn, Y=Yr.detach(), hn=hnr.detach(),
                grads={k: leaves[k].grad for k in PARAM_KEYS}, dh0=h0r.grad)


class _option:
    def __init__(self, key, value):
        self.key, self.value = key, value

    def __enter__(self):
        from windgnn_amd import _lib
        self.prev = _lib.set_option(self.key, self.value)

    def __exit__(self, *exc):
        from windgnn_amd import _lib
        _lib.set_option(self.key, self.prev)


def _profiled(fn):
    """fn() under the library's profiler: its result and the names of everything it launched."""
    from windgnn_amd import _lib
    _lib.profile_enable(True)
    try:
        out = fn()
        torch.cuda.synchronize()
        names = [r["name"] for r in _lib.profile_read()]
    finally:
        _lib.profile_enable(False)
    return out, names


@functools.lru_cache(maxsize=None)
def _step(S, T, B, H, math, io, state, route):
    """One step of this call form on the GPU: the names it launched and its errors against the reference (floats only)."""
    from windgnn_amd import _lib
    from windgnn_amd.functional import (check_range_status, gcn_gru_backward_mse_raw, gcn_gru_forward_raw,
                                        gcn_gru_state_backward_raw, gcn_gru_state_forward_raw)
    dev = _dev()
    r = _reference(S, T, B, H, io, state)
    A, X = r["A"].to(dev), r["X"].to(dev)
    ps = [r["p"][k].to(dev).contiguous() for k in PARAM_KEYS]
    mode = MATH[math]

    def run():
        gs = [torch.full_like(q, 7.0) for q in ps]
        if route == "infer":
            Y, _, _ = gcn_gru_forward_raw(A, X, ps, mode, want_stash=False)
            return dict(Y=Y)
        if state:
            dh0 = torch.full((B, H), 7.0, device=dev)
            Y, hn, stash, d = gcn_gru_state_forward_raw(A, X, ps, mode, r["h0"].to(dev))
            gcn_gru_state_backward_raw(d, A, X, ps, Y, r["dY"].to(dev), r["dhn"].to(dev), stash, gs, dh0)
            return dict(Y=Y, hn=hn, grads=gs, dh0=dh0)
        L = r["L"].to(dev)
        loss = torch.zeros((), device=dev)
        Y, stash, d = gcn_gru_forward_raw(A, X, ps, mode, labels=L)
        gcn_gru_backward_mse_raw(d, A, X, ps, Y, L, stash, gs, loss, 1.0, part=7 | 8)
        return dict(Y=Y, loss=loss, grads=gs)

    opt = {"unmerged": (_lib.OPT_TN_MERGED, 0), "fused": (_lib.OPT_FUSED_FWD, 2)}.get(route)
    if opt:
        with _option(*opt):
            out, names = _profiled(run)
    else:
        out, names = _profiled(run)
    check_range_status(dev)
    err = {"Y": max_abs(out["Y"].float().cpu().reshape(r["Y"].shape), r["Y"])}
    if "loss" in out:
        err["loss"] = abs(float(out["loss"]) - r["loss"]) / max(1.0, r["loss"])
    if "hn" in out:
        err["hn"] = max_abs(out["hn"].cpu(), r["hn"])
        err["dh0"] = rel_to_max(out["dh0"].cpu(), r["dh0"])
    for k, gk in zip(PARAM_KEYS, out.get("grads", [])):
        err[k] = rel_to_max(gk.cpu(), r["grads"][k])
    return tuple(names), err


def _bounds(S, T, B, H, math, io, state, route):
    """The suite's tolerance of every figure _step reports (imported, none restated)."""
    iodt = IODT[io]
    y_tol, g_tol = _tols("f16x3g_big" if (state and math == "f16x3g" and B * T >= 4096) else "", math, iodt)
    assert g_tol in (G_TOL, 1e-3, F16_G_TOL) and (Y_TOL, F16_Y_TOL)[math == "f16"] <= y_tol   # the bars of tests/test_gpu_parity.py
    b = {k: g_tol for k in PARAM_KEYS}
    b.update(Y=y_tol, hn=y_tol - IO_ROUND[iodt], dh0=g_tol, loss=2e-3 if math == "f16" else 1e-5)
    return b


def _check(case, exceptions=None):
    """exceptions: (key, tensor) -> the pinned bar of a one-pass fp16 figure above the imported one; ic.F16_EXCEPTIONS unless a
    module brings its own (the K-loop cases: the same keys at other dims)."""
    exceptions = ic.F16_EXCEPTIONS if exceptions is None else exceptions
    fam, key, S, T, B, H, math, io, state, route = case
    expected = ic.plan(S, T, B, H, math, io, state, route)
    assert key in expected, (key, expected)                    # (tests/test_instance_table_host.py checks this without a GPU)
    names, err = _step(S, T, B, H, math, io, state, route)
    ran = sorted({n for n in names if re.match(r"[a-z0-9_]+", n).group(0) in TABLED})
    print("%s S%d T%d B%d H%d %s %s state=%d %s: %s" % (key, S, T, B, H, math, io, state, route,
                                                       " ".join("%s=%.2e" % kv for kv in err.items())))
    # the instance ran, and so did exactly the siblings the hidden arguments of the key imply
    assert ic.name_of(key) in ran, (key, ran)
    assert ran == sorted({ic.name_of(k) for k in expected}), (key, ran, expected)
    bounds = _bounds(S, T, B, H, math, io, state, route)
    for what, e in err.items():
        bound = exceptions.get((key, what), bounds[what]) if math == "f16" else bounds[what]
        assert e <= bound, (key, what, e, bound)


def _family_test(fam):
    cases = [c for c in ic.CASES if c[0] == fam]

    @pytest.mark.parametrize("case", cases, ids=[c[1] for c in cases])
    def test(case):
        _check(case)
    test.__name__ = test.__qualname__ = "test_" + fam
    return test


for _fam in ic.FAMILIES:
    globals()["test_" + _fam] = _family_test(_fam)
del _fam
