"""Footprint tests: what every C entry point does OUTSIDE the numbers it is asked for, and what it takes in from bytes it never
wrote.  Every buffer comes from tests/guarded.py's arena with exactly the byte length the ABI prescribes (wgnn_*_bytes() for
workspace, stash, state stash, `prepared` and the layer workspaces; numel * itemsize for everything else), inside poisoned
guard bands; outputs, stash and workspace start out as the fill.  For each case, under the fills zero, finite, nan in that
order and then on the scratch bytes another case (other dims, other math mode) left behind:

  (a) every guard band is byte-identical to what it was before the call;
  (b) every output is bitwise equal to the zero-fill run and (finite / nan) holds no poison;
  (c) the status word is 0 after every call;
  (d) under the zero fill the outputs meet the fp64 oracle at the suite's tolerances for the mode.

The workspace is re-poisoned (status block apart) between a forward and its backward: it is live state only inside the
sequences the header marks "on the SAME workspace".  The calls go through the ctypes functions of windgnn_amd._lib directly,
not through functional._Workspace.  DESIGN.md section 2b has the case table and what the method cannot see."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from conftest import PARAM_KEYS, max_abs, rel_to_max
from guarded import FILLS, Arena
from test_gpu_parity import F16_G_TOL, F16_Y_TOL, G_TOL, IO_ROUND, Y_TOL

pytestmark = pytest.mark.gpu

MATH = {"f32": 0, "f16x3": 1, "f16": 2, "f16x3g": 3}
IO = {torch.float32: 0, torch.float16: 1, torch.bfloat16: 2}
F = 13
STATUS = 256                                    # WGNN_STATUS_BYTES

# id -> (math, io dtype, S, T, B, H, CSR k-NN degree or 0); the id names the branch of make_layout (csrc/api.hip) it is there for
CASES = {
    "small_odd": ("f32", torch.float32, 7, 12, 5, 21, 0),              # `small`, odd S*13 (xtail), tiny rows
    "small_splitk": ("f32", torch.float32, 11, 5, 3, 9, 0),            # ws_ntk_f/b: gemm_f32_nt_splitk > 1 (I = 143)
    "rec32": ("f32", torch.float32, 5, 3, 800, 9, 0),                  # rec32 (B > 768), B*T < 4096
    "g32_small": ("f32", torch.float32, 34, 24, 172, 102, 0),          # g32 / g32tn with small, st_hprev, B*T = 4128
    "g32_rec": ("f32", torch.float32, 33, 6, 770, 100, 0),             # g32tn with rec32, dghn, odd I
    "f32_h128": ("f32", torch.float32, 13, 4, 6, 128, 0),              # both sides of gru_shape_supported
    "f32_h129": ("f32", torch.float32, 13, 4, 6, 129, 0),
    "x3-34x24x37x102": ("f16x3", torch.float32, 34, 24, 37, 102, 0),   # register-resident path
    "x3-33x1x19x100": ("f16x3", torch.float32, 33, 1, 19, 100, 0),     # odd I, T = 1
    "x3-64x3x2x127": ("f16x3", torch.float32, 64, 3, 2, 127, 0),       # S and H limits
    "x3-1x1x1x1": ("f16x3", torch.float32, 1, 1, 1, 1, 0),
    "x3_h128": ("f16x3", torch.float32, 20, 5, 6, 128, 0),             # first gen_gru width in the plane family
    "x3g_dgi1": ("f16x3g", torch.float32, 34, 24, 171, 102, 0),        # dgi1, dg16 (B*T = 4104)
    "x3g_gen2p": ("f16x3g", torch.float32, 5, 3, 1024, 130, 0),        # gen2p
    "f16": ("f16", torch.float32, 7, 12, 32, 21, 0),                   # gi16, dg16
    "io16-f16x3-fp16": ("f16x3", torch.float16, 34, 24, 37, 102, 0),   # 16-bit X / Y / labels
    "io16-f16-bf16": ("f16", torch.bfloat16, 3, 2, 1, 9, 0),           # ... byte lengths that are not multiples of 4
    "csr-f32": ("f32", torch.float32, 200, 3, 4, 60, 8),               # gen_gcn
    "csr-f16x3": ("f16x3", torch.float32, 200, 3, 4, 60, 8),
    "csr_wide-f32": ("f32", torch.float32, 100, 3, 4, 160, 6),         # gen_gcn + gen_gru
    "csr_wide-f16x3": ("f16x3", torch.float32, 100, 3, 4, 160, 6),
    "big_gemm": ("f16x3", torch.float32, 200, 24, 48, 700, 8),         # ws_aimg_f/b (pgemm_big): test_large_plane_gemm_instance's
    "rows-f32": ("f32", torch.float32, 200, 6, 8, 600, 8),             # tests/test_gpu_grad_blocks.py's shape (wide-GRU path)
    "rows-f16x3": ("f16x3", torch.float32, 200, 6, 8, 600, 8),
}
# whose leftovers a case runs on in the dirty variant: another math mode and other dims, tiled to the recipient's sizes
DONOR = {"f32": "x3-34x24x37x102", "f16x3": "rec32", "f16": "rec32", "f16x3g": "rec32"}


def _dev():
    assert torch.cuda.is_available(), "gpu tests need an MI355X"
    return torch.device("cuda:0")


def _lib():
    from windgnn_amd import _lib as L
    return L


class Case:
    pass


def _case(cid):
    return _build(cid, CASES[cid])


@functools.lru_cache(maxsize=6)
def _build(cid, spec):
    """Host tensors of a case and its fp64 oracle step (computed once per case, not per fill)."""
    from oracle import windgnn_oracle as orc
    math, iodt, S, T, B, H, k = spec
    c = Case()
    c.id, c.math, c.iodt, c.S, c.T, c.B, c.H, c.k = cid, math, iodt, S, T, B, H, k
    g = torch.Generator().manual_seed(4100 + S * 7 + B + H)
    if k:
        from windgnn_amd.graph import CsrAdjacency, build_knn_adjacency, synthetic_station_coords
        csr = CsrAdjacency(*build_knn_adjacency(synthetic_station_coords(S, seed=3), k))
        c.A_host, c.A_bytes, c.nnz = csr.dense(), csr.blob.clone(), csr.nnz
        assert c.A_bytes.numel() == 2 * (S + 1) + 4 * csr.nnz
    else:
        c.A_host = torch.rand(S, S, generator=g) / S + 0.01
        c.A_bytes, c.nnz = c.A_host, 0
    c.X = torch.rand(B, T, S, F, generator=g).to(iodt)                 # what travels: already rounded (16-bit I/O)
    c.L = torch.rand(B, T, H, generator=g).to(iodt)
    c.p = orc.init_params(S, F, H, seed=S + H)
    if S >= 100:                                                       # keeps g (a sum over k neighbours) O(1), as the suite does
        c.p["conv1.weight"] *= 0.3
        c.p["conv2.weight"] *= 0.3
    p64 = {kk: v.double() for kk, v in c.p.items()}
    c.Yo, c.loss_o, c.go = orc.train_step(c.A_host.double(), c.X.double(), c.L.double(), p64)
    c.dY = (2.0 * (c.Yo - c.L.double()) / c.Yo.numel()).float()        # the MSE gradient, as an explicit fp32 dY
    c.h0 = torch.rand(B, H, generator=g) * 1.6 - 0.8
    c.dhn = torch.randn(B, H, generator=g) * 1e-3
    c.y_tol = (F16_Y_TOL if math == "f16" else Y_TOL) + (IO_ROUND[iodt] if iodt != torch.float32 else 0.0)
    c.g_tol = F16_G_TOL if math == "f16" else G_TOL
    c.loss_tol = (2e-3 if math == "f16" else 1e-5) * max(1.0, float(c.loss_o))
    return c


def _fit(src, n):
    """`src` bytes tiled / cut to n bytes: somebody else's leftovers in a buffer of another size."""
    src = src.reshape(-1)
    return src.repeat((n + src.numel() - 1) // src.numel())[:n].contiguous()


class Run:
    """All buffers of one case under one fill, each of its exact ABI length, and the calls on them."""

    def __init__(self, c, fill, state=False, dirty=None, off=0, seed=0, extra=(), stream=None):
        """stream: None (the null stream; every call is followed by a synchronise and a look at the status word) or a
        torch.cuda.Stream: every call and every fill in between is enqueued there, nothing synchronises, and the status word
        is read once, by final_status(), after the caller's own synchronise (tests/test_gpu_streams.py)."""
        L = self.L = _lib()
        lib = self.lib = L.load()
        self.tstream = stream
        self.c, self.fill, self.state = c, fill, state
        es = 4 if c.iodt == torch.float32 else 2
        self.d = L.Dims(c.B, c.T, c.S, F, c.H, MATH[c.math], 1 if c.k else 0, c.nnz, IO[c.iodt])
        d = C.byref(self.d)
        self.ws_bytes = lib.wgnn_workspace_bytes(d)
        self.stash_bytes = lib.wgnn_state_stash_bytes(d) if state else lib.wgnn_stash_bytes(d)
        self.prep_bytes = lib.wgnn_prepared_bytes(d)
        assert self.ws_bytes > STATUS and self.stash_bytes > 0
        if state:
            assert self.stash_bytes >= lib.wgnn_stash_bytes(d)
        a = self.a = Arena(_dev(), fill, seed)
        self.dirty = dirty = dirty or {}
        off_io, off_dy = (es, 4) if off else (0, 0)     # X / Y / labels and dY one element past a 256-byte boundary
        nY = c.B * c.T * c.H
        self.meta = {}

        def add(name, dtype, shape, data=None, **kw):
            n = int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size()
            self.meta[name] = (dtype, tuple(shape))
            return a.buf(name, n, data=data, **kw)

        add("A", torch.int32 if c.k else torch.float32, c.A_bytes.shape, c.A_bytes)
        add("X", c.iodt, c.X.shape, c.X, offset=off_io)
        add("L", c.iodt, c.L.shape, c.L, offset=off_io)
        add("dY", torch.float32, c.dY.shape, c.dY, offset=off_dy)
        add("h0", torch.float32, (c.B, c.H), c.h0)
        add("dh_n", torch.float32, (c.B, c.H), c.dhn)
        for kk in PARAM_KEYS:
            add("p." + kk, torch.float32, c.p[kk].shape, c.p[kk])
            add("m." + kk, torch.float32, c.p[kk].shape, torch.zeros_like(c.p[kk]))
            add("v." + kk, torch.float32, c.p[kk].shape, torch.zeros_like(c.p[kk]))
            add("g." + kk, torch.float32, c.p[kk].shape)
        add("Y", c.iodt, (c.B, c.T, c.H), offset=off_io)
        assert a["Y"].nbytes == nY * es
        add("h_n", torch.float32, (c.B, c.H))
        add("dh0", torch.float32, (c.B, c.H))
        add("last", torch.float32, (c.B, c.H))
        add("loss", torch.float32, (1,))
        for name, dtype, shape in extra:                                # further outputs of one flow
            add(name, dtype, shape)
        add("stash", torch.uint8, (self.stash_bytes,), _fit(dirty["stash"], self.stash_bytes) if "stash" in dirty else None)
        add("ws", torch.uint8, (self.ws_bytes,), _fit(dirty["ws"], self.ws_bytes) if "ws" in dirty else None, zero_head=STATUS)
        if self.prep_bytes:
            for nm in ("prepared", "prepared2"):
                add(nm, torch.uint8, (self.prep_bytes,), _fit(dirty["prepared"], self.prep_bytes) if "prepared" in dirty else None)
        a.commit()
        self.stream = C.c_void_p(stream.cuda_stream if stream is not None else 0)
        self.ws = (C.c_void_p(a["ws"].ptr), C.c_size_t(self.ws_bytes), self.stream)

    # ---- argument helpers
    def ptr(self, name):
        return C.c_void_p(self.a[name].ptr) if name else C.c_void_p(0)

    def params(self, prepared=None):
        ps = self.L.Params()
        for (field, _), kk in zip(self.L.Params._fields_, PARAM_KEYS):
            setattr(ps, field, self.a["p." + kk].ptr)
        if prepared:
            ps.prepared = self.a[prepared].ptr
        return ps

    def grads(self, prefix="g."):
        gs = self.L.Grads()
        for (field, _), kk in zip(self.L.Grads._fields_, PARAM_KEYS):
            setattr(gs, field, self.a[prefix + kk].ptr)
        return gs

    def adam(self, step=1):
        ad = self.L.Adam()
        ad.exp_avg, ad.exp_avg_sq = self.grads("m."), self.grads("v.")
        ad.step, ad.lr, ad.beta1, ad.beta2, ad.eps = step, 1e-3, 0.9, 0.999, 1e-8
        return ad

    def ok(self, rc, what):
        """(c): the call succeeded and, once it has run, the status word is still 0."""
        assert rc == 0, (self.c.id, self.fill, what, rc, self.lib.wgnn_strerror(rc).decode())
        if self.tstream is not None:
            return
        torch.cuda.synchronize()
        word = int(self.a["ws"].bytes()[:4].view(torch.int32).item())
        assert word == 0, (self.c.id, self.fill, what, "status word %d" % word)

    def repoison_ws(self):
        """Between a forward and its backward the workspace is not live state: everything but the status block is poisoned."""
        if self.tstream is not None:                    # stream-ordered, and the status block keeps what the calls left in it
            ws = self.a["ws"]
            with torch.cuda.stream(self.tstream):
                self.a.mem[ws.start + STATUS:ws.start + ws.nbytes].copy_(self.a.pristine[ws.start + STATUS:ws.start + ws.nbytes])
            return
        torch.cuda.synchronize()
        self.a["ws"].poison()

    def final_status(self):
        """The status word, for a run on a side stream: read once, after the caller has synchronised."""
        return int(self.a["ws"].bytes()[:4].view(torch.int32).item())

    def tensor(self, name, res=None):
        dtype, shape = self.meta[name]
        b = res[name] if res is not None else self.a[name].host()
        return b.view(dtype).reshape(shape)

    def collect(self, names, poison_free=None):
        """(a) and the no-poison half of (b); returns {name: bytes on the host} of the outputs."""
        torch.cuda.synchronize()
        rep = self.a.check()
        assert rep == {}, (self.c.id, self.fill, "guard bands changed (offsets from the buffer's first byte)", rep)
        res = {}
        for n in names:
            res[n] = self.a[n].host()
            item = torch.empty((), dtype=self.meta[n][0]).element_size()
            if self.meta[n][0] == torch.uint8:                           # raw images: judged word by word
                item = 4
            # (a 16-bit result equals the 16 random bits of the finite fill once in 65536 elements: those are judged under nan)
            # (on another case's leftovers equal words prove nothing: its zero pads are this case's zero pads)
            if (self.fill == "nan" or (self.fill == "finite" and item >= 4)) and (poison_free is None or n in poison_free) \
                    and not self.dirty:
                left = self.a[n].unwritten(item)
                assert left == 0, (self.c.id, self.fill, n, "%d elements still hold the fill" % left)
        return res

    def untouched(self):
        torch.cuda.synchronize()
        return torch.equal(self.a.mem, self.a.pristine)

    def leftovers(self):
        out = {"ws": self.a["ws"].host(), "stash": self.a["stash"].host()}
        if self.prep_bytes:
            out["prepared"] = self.a["prepared"].host()
        return out


GRAD_NAMES = ["g." + k for k in PARAM_KEYS]


def _same(base, res, tag):
    """(b): bitwise equality with the zero-fill run."""
    assert set(base) == set(res)
    for n in base:
        if not torch.equal(base[n], res[n]):
            nd = int((base[n] != res[n]).sum())
            raise AssertionError("%s: %s differs from the zero-fill run in %d of %d bytes" % (tag, n, nd, base[n].numel()))


@functools.lru_cache(maxsize=32)
def _donor_leftovers(flow, donor, kw):
    r = Run(_case(donor), "finite", seed=3, **dict(kw))
    flow(r)
    torch.cuda.synchronize()
    return r.leftovers()


def _footprint(cid, flow, oracle=None, poison_free=None, **kw):
    """One flow on one case: the three fills in order, then on another case's leftovers; (a)-(c) in every run, (b) against
    the zero fill, (d) once."""
    c = _case(cid)
    base = None
    for fill in FILLS:
        r = Run(c, fill, **kw)
        res = r.collect(flow(r), poison_free)
        if fill == "zero":
            base = res
            if oracle is not None:
                oracle(r, res)
        else:
            _same(base, res, "%s [%s]" % (cid, fill))
    left = _donor_leftovers(flow, DONOR[c.math], tuple(sorted(kw.items())))
    r = Run(c, "finite", dirty=left, seed=1, **kw)
    _same(base, r.collect(flow(r), poison_free), "%s [on the leftovers of %s]" % (cid, DONOR[c.math]))


# ---------------------------------------------------------------------------------------------------------------- oracles
def _check_Y(r, res, name="Y", ref=None):
    c = r.c
    e = max_abs(r.tensor(name, res).float(), c.Yo if ref is None else ref)
    print("%s: max|%s - oracle| = %.3e (bound %.1e)" % (c.id, name, e, c.y_tol))
    assert e <= c.y_tol, (c.id, name, e)


def _check_grads(r, res, ref=None):
    c = r.c
    ref = c.go if ref is None else ref
    for k in PARAM_KEYS:
        e = rel_to_max(r.tensor("g." + k, res), ref[k])
        print("%s: grad %s rel-to-max error %.3e (bound %.1e)" % (c.id, k, e, c.g_tol))
        assert e <= c.g_tol, (c.id, k, e)


def _check_loss(r, res):
    e = abs(float(r.tensor("loss", res)[0]) - float(r.c.loss_o))
    assert e <= r.c.loss_tol, (r.c.id, "loss", e)


def _fp64_model(c):
    """The 8 tensors as fp64 leaves, and f(X or g, h0) -> (Y, h_n): two relu(A X W + b) layers, then nn.GRU with hx
    (tests/test_gpu_state_train.py's reference)."""
    leaves = {k: c.p[k].double().clone().requires_grad_(True) for k in PARAM_KEYS}

    def f(X, h0, g_in=None):
        if g_in is None:
            A, X = c.A_host.double(), X.double()
            h = torch.relu(torch.matmul(torch.matmul(A, X), leaves["conv1.weight"]) + leaves["conv1.bias"])
            h = torch.relu(torch.matmul(torch.matmul(A, h), leaves["conv2.weight"]) + leaves["conv2.bias"])
            g_in = h.reshape(c.B, X.shape[1], c.S * F)
        Y, hn = torch._VF.gru(g_in, h0.unsqueeze(0),
                              [leaves["gru.weight_ih_l0"], leaves["gru.weight_hh_l0"], leaves["gru.bias_ih_l0"],
                               leaves["gru.bias_hh_l0"]], True, 1, 0.0, False, False, True)
        return Y, hn[0]
    return leaves, f


# ---------------------------------------------------------------------------------------------------------------- flows
def flow_fwd_bwd(r):
    """wgnn_fwd with a stash, then wgnn_bwd on a re-poisoned workspace."""
    lib, d, ps, gs = r.lib, C.byref(r.d), r.params(), r.grads()
    r.ok(lib.wgnn_fwd(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("Y"), r.ptr("stash"), *r.ws), "wgnn_fwd")
    r.repoison_ws()
    r.ok(lib.wgnn_bwd(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("Y"), r.ptr("dY"), r.ptr("stash"), C.byref(gs), *r.ws),
         "wgnn_bwd")
    return ["Y"] + GRAD_NAMES


def _oracle_fwd_bwd(r, res):
    _check_Y(r, res)
    _check_grads(r, res)


@pytest.mark.parametrize("cid", [k for k in CASES if not k.startswith("rows")])
def test_fwd_stash_bwd(cid):
    _footprint(cid, flow_fwd_bwd, _oracle_fwd_bwd)


@pytest.mark.parametrize("cid", ["small_odd", "g32_small", "x3-34x24x37x102", "csr_wide-f16x3"])
def test_a_workspace_one_word_short_is_refused_before_any_launch(cid):
    """wgnn_workspace_bytes() is the larger of the forward's and the backward's need: with 4 bytes less, the call that needs
    all of it returns WGNN_ERR_WORKSPACE and touches nothing; the other one (if it needs less) runs inside what it was given."""
    r = Run(_case(cid), "nan")
    lib, d, ps, gs = r.lib, C.byref(r.d), r.params(), r.grads()
    short = (r.ws[0], C.c_size_t(r.ws_bytes - 4), r.stream)
    refused = 0
    rc = lib.wgnn_fwd(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("Y"), r.ptr("stash"), *short)
    if rc != 0:
        assert rc == -4 and r.untouched()
        refused += 1
        rc = lib.wgnn_fwd(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("Y"), r.ptr("stash"), *r.ws)
    r.ok(rc, "wgnn_fwd")
    snap = r.a.mem.clone()
    rc = lib.wgnn_bwd(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("Y"), r.ptr("dY"), r.ptr("stash"), C.byref(gs), *short)
    torch.cuda.synchronize()
    if rc != 0:
        assert rc == -4 and torch.equal(snap, r.a.mem)
        refused += 1
    assert refused >= 1
    assert r.a.check() == {}


def _flow_fwd_nostash(opt):
    def flow(r):
        lib, d, ps = r.lib, C.byref(r.d), r.params()
        prev = r.L.set_option(r.L.OPT_FUSED_FWD, opt)
        try:
            r.ok(lib.wgnn_fwd(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("Y"), r.ptr(None), *r.ws), "wgnn_fwd(no stash)")
        finally:
            r.L.set_option(r.L.OPT_FUSED_FWD, prev)
        return ["Y"]
    flow.__name__ = "flow_fwd_nostash_%d" % opt
    return flow


FLOW_NOSTASH = {0: _flow_fwd_nostash(0), 2: _flow_fwd_nostash(2)}
NOSTASH_CASES = ["x3-34x24x37x102", "x3-33x1x19x100", "x3-64x3x2x127", "x3-1x1x1x1", "f16", "io16-f16x3-fp16", "io16-f16-bf16",
                 "small_odd", "csr-f32", "csr-f16x3"]


@pytest.mark.parametrize("opt", [0, 2])
@pytest.mark.parametrize("cid", NOSTASH_CASES)
def test_fwd_without_stash_under_fused_fwd_option(cid, opt):
    def oracle(r, res):
        _check_Y(r, res)
        assert r.a["stash"].unwritten(1) == r.stash_bytes               # no stash was passed: the buffer is no argument
    _footprint(cid, FLOW_NOSTASH[opt], oracle)
    assert _lib().get_option(_lib().OPT_FUSED_FWD) == 1


def flow_fwd_last(r):
    lib, d, ps = r.lib, C.byref(r.d), r.params()
    r.ok(lib.wgnn_fwd_last(d, r.ptr("A"), r.ptr("X"), C.byref(ps), C.c_float(-2.5), C.c_float(31.0), r.ptr("last"), *r.ws),
         "wgnn_fwd_last")
    return ["last"]


@pytest.mark.parametrize("cid", ["x3-34x24x37x102", "x3-64x3x2x127", "f16", "small_odd", "rec32", "f32_h129", "csr_wide-f32",
                                 "csr_wide-f16x3"])
def test_fwd_last(cid):
    def oracle(r, res):
        c = r.c
        ref = c.Yo[:, -1, :] * 33.5 - 2.5
        e = max_abs(r.tensor("last", res), ref)
        assert e <= c.y_tol * 33.5, (cid, e)                            # Y's bound through the read-out's multiplier
    _footprint(cid, flow_fwd_last, oracle)


def test_fwd_last_refuses_16bit_io_before_any_launch():
    r = Run(_case("io16-f16x3-fp16"), "nan")
    ps = r.params()
    rc = r.lib.wgnn_fwd_last(C.byref(r.d), r.ptr("A"), r.ptr("X"), C.byref(ps), C.c_float(0.0), C.c_float(1.0), r.ptr("last"),
                             *r.ws)
    assert rc == -5 and r.untouched()


def _flow_loss(defer, prepared):
    """wgnn_fwd_loss + wgnn_bwd_mse_part(7 | 8), or with WGNN_BWD_DEFER + wgnn_finish(6, adam); prepared: None (rebuilt inside
    every call) or a caller-kept buffer that wgnn_prepare_weights writes first."""
    def flow(r):
        lib, d, gs = r.lib, C.byref(r.d), r.grads()
        kept = prepared and r.prep_bytes > 0            # (a donor of leftovers may have no images: it runs without)
        ps = r.params("prepared" if kept else None)
        if kept:
            r.ok(lib.wgnn_prepare_weights(d, C.byref(ps), *r.ws), "wgnn_prepare_weights")
            r.repoison_ws()
        r.ok(lib.wgnn_fwd_loss(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("L"), r.ptr("Y"), r.ptr("stash"), *r.ws),
             "wgnn_fwd_loss")
        r.repoison_ws()
        part = 7 | 8 | (r.L.BWD_DEFER if defer else 0)
        r.ok(lib.wgnn_bwd_mse_part(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("Y"), r.ptr("L"), C.c_float(1.0), r.ptr("loss"),
                                   r.ptr("stash"), C.byref(gs), *r.ws, part), "wgnn_bwd_mse_part(%d)" % part)
        outs = ["Y", "loss"] + GRAD_NAMES
        if defer:       # live state: the partial sums stay in the workspace until wgnn_finish, on the SAME workspace
            ad = r.adam()
            r.ok(lib.wgnn_finish(d, C.byref(ps), C.byref(gs), 6, C.byref(ad), *r.ws), "wgnn_finish(6, adam)")
            outs += [pre + k for pre in ("p.", "m.", "v.") for k in PARAM_KEYS]
            if kept:
                outs.append("prepared")
                ps2 = r.params("prepared2")                              # the images of the NEW weights, built from scratch
                r.ok(lib.wgnn_prepare_weights(d, C.byref(ps2), *r.ws), "wgnn_prepare_weights(new weights)")
                outs.append("prepared2")
        return outs
    flow.__name__ = "flow_loss_%d_%d" % (defer, prepared)
    return flow


FLOW_LOSS = {(dfr, pre): _flow_loss(dfr, pre) for dfr in (0, 1) for pre in (0, 1)}
LOSS_CASES = ["x3-34x24x37x102", "x3g_dgi1", "g32_small", "small_odd", "csr_wide-f32", "csr_wide-f16x3", "io16-f16x3-fp16",
              "io16-f16-bf16"]
INPLACE = {pre + k for pre in ("p.", "m.", "v.") for k in PARAM_KEYS}      # updated in place: they never held the fill


# the hyper-parameters as the fp32 values that cross the ABI (wgnn_adam's fields are floats)
LR, B1, B2, EPS = (float(np.float32(x)) for x in (1e-3, 0.9, 0.999, 1e-8))


def _oracle_loss(r, res):
    c = r.c
    _check_Y(r, res)
    _check_loss(r, res)
    _check_grads(r, res)
    if "p." + PARAM_KEYS[0] not in res:
        return
    # torch.optim.Adam's first step in fp64 on the gradients the GPU produced: m = (1 - b1) g, v = (1 - b2) g^2,
    # p -= lr (m / bc1) / (sqrt(v / bc2) + eps) -- fp32 arithmetic of a handful of operations: 1e-6 of the tensor's scale
    for k in PARAM_KEYS:
        g = r.tensor("g." + k, res).double()
        m, v = (1 - B1) * g, (1 - B2) * g * g
        pn = c.p[k].double() - LR * (m / (1 - B1)) / ((v / (1 - B2)).sqrt() + EPS)
        assert rel_to_max(r.tensor("m." + k, res), m) <= 1e-6, k
        assert rel_to_max(r.tensor("v." + k, res), v) <= 1e-6, k
        assert max_abs(r.tensor("p." + k, res), pn) <= 1e-6 * max(1.0, float(pn.abs().max())), k
    if "prepared" in res:
        assert torch.equal(res["prepared"], res["prepared2"]), "wgnn_finish(adam) did not keep the W_ih images current"


@pytest.mark.parametrize("cid", LOSS_CASES)
def test_fwd_loss_bwd_mse_part(cid):
    _footprint(cid, FLOW_LOSS[(0, 0)], _oracle_loss)


@pytest.mark.parametrize("prepared", [0, 1], ids=["rebuilt", "kept"])
@pytest.mark.parametrize("cid", LOSS_CASES[:6])
def test_fwd_loss_bwd_defer_finish_adam(cid, prepared):
    c = _case(cid)
    if prepared and Run(c, "zero").prep_bytes == 0:
        # this configuration stages W_ih as it is: wgnn_prepared_bytes() is 0 and wgnn_prepare_weights is a documented
        # WGNN_ERR_UNSUPPORTED -- refused before any launch, nothing touched
        r = Run(c, "nan")
        ps = r.params()
        ps.prepared = r.a["stash"].ptr                                  # any non-NULL pointer
        assert r.lib.wgnn_prepare_weights(C.byref(r.d), C.byref(ps), *r.ws) == -5
        assert r.untouched()
        return
    _footprint(cid, FLOW_LOSS[(1, prepared)], _oracle_loss, poison_free=set(["Y", "loss"] + GRAD_NAMES + ["prepared", "prepared2"]))


def flow_bwd_parts(r):
    """wgnn_bwd_part as 1, then 2, then 4, on the SAME workspace (poisoned before part 1 only)."""
    lib, d, ps, gs = r.lib, C.byref(r.d), r.params(), r.grads()
    r.ok(lib.wgnn_fwd(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("Y"), r.ptr("stash"), *r.ws), "wgnn_fwd")
    r.repoison_ws()
    for part in (1, 2, 4):
        r.ok(lib.wgnn_bwd_part(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("Y"), r.ptr("dY"), r.ptr("stash"), C.byref(gs),
                               *r.ws, part), "wgnn_bwd_part(%d)" % part)
    return ["Y"] + GRAD_NAMES


@pytest.mark.parametrize("cid", ["x3-34x24x37x102", "rec32", "csr-f32", "csr-f16x3"])
def test_bwd_part_1_2_4(cid):
    _footprint(cid, flow_bwd_parts, _oracle_fwd_bwd)


def _flow_state(given):
    """wgnn_fwd_state (Y and h_n), then wgnn_fwd_state_stash + wgnn_bwd_state_part(7) with h0, dh_n and dh0 all given or all
    NULL."""
    def flow(r):
        lib, d, ps, gs = r.lib, C.byref(r.d), r.params(), r.grads()
        h0, dhn, dh0 = (r.ptr("h0"), r.ptr("dh_n"), r.ptr("dh0")) if given else (r.ptr(None),) * 3
        r.ok(lib.wgnn_fwd_state(d, r.ptr("A"), r.ptr("X"), C.byref(ps), h0, r.ptr("Y"), r.ptr("h_n"), *r.ws), "wgnn_fwd_state")
        torch.cuda.synchronize()
        keep = {"Y.inference": r.a["Y"].host(), "h_n.inference": r.a["h_n"].host()}
        r.a["Y"].poison()
        r.a["h_n"].poison()
        r.repoison_ws()
        r.ok(lib.wgnn_fwd_state_stash(d, r.ptr("A"), r.ptr("X"), C.byref(ps), h0, r.ptr("Y"), r.ptr("h_n"), r.ptr("stash"),
                                      *r.ws), "wgnn_fwd_state_stash")
        r.repoison_ws()
        r.ok(lib.wgnn_bwd_state_part(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("Y"), r.ptr("dY"), dhn, r.ptr("stash"),
                                     C.byref(gs), dh0, *r.ws, 7), "wgnn_bwd_state_part")
        r.inference = keep
        return ["Y", "h_n"] + GRAD_NAMES + (["dh0"] if given else [])
    flow.__name__ = "flow_state_%d" % given
    return flow


FLOW_STATE = {0: _flow_state(0), 1: _flow_state(1)}


@pytest.mark.parametrize("given", [1, 0], ids=["h0_dhn_dh0", "all_null"])
@pytest.mark.parametrize("cid", ["small_odd", "rec32", "g32_small", "x3-34x24x37x102", "x3_h128", "csr_wide-f32",
                                 "csr_wide-f16x3"])
def test_state_fwd_and_training_pair(cid, given):
    def oracle(r, res):
        c = r.c
        leaves, f = _fp64_model(c)
        h0 = (c.h0 if given else torch.zeros_like(c.h0)).double().requires_grad_(True)
        Yr, hnr = f(c.X.float(), h0)
        ((Yr * c.dY.double()).sum() + ((hnr * c.dhn.double()).sum() if given else 0.0)).backward()
        _check_Y(r, res, "Y", Yr.detach())
        _check_Y(r, res, "h_n", hnr.detach())
        _check_grads(r, res, {k: leaves[k].grad for k in PARAM_KEYS})
        if given:
            e = rel_to_max(r.tensor("dh0", res), h0.grad)
            assert e <= c.g_tol, (cid, "dh0", e)
        # the inference entry point against the same reference
        assert max_abs(r.inference["Y.inference"].view(torch.float32).reshape(Yr.shape), Yr.detach()) <= c.y_tol
        assert max_abs(r.inference["h_n.inference"].view(torch.float32).reshape(hnr.shape), hnr.detach()) <= c.y_tol

    _footprint(cid, FLOW_STATE[given], oracle, state=True)


def test_state_dh0_untouched_when_not_requested():
    """With dh0 = NULL the dh0 buffer is not an argument: it must still hold the fill."""
    r = Run(_case("small_odd"), "nan", state=True)
    FLOW_STATE[0](r)
    r.collect([])
    assert r.a["dh0"].unwritten(4) == r.c.B * r.c.H


@pytest.mark.parametrize("B", [1, 256])
@pytest.mark.parametrize("H", [102, 128])
def test_one_kernel_hourly_step(B, H):
    """wgnn_fwd_state with T = 1, S = 34, f32: the whole hour as one launch (csrc/gru_step.hip)."""
    cid = "step-B%d-H%d" % (B, H)

    def flow(r):
        ps = r.params()
        r.ok(r.lib.wgnn_fwd_state(C.byref(r.d), r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("h0"), r.ptr("Y"), r.ptr("h_n"),
                                  *r.ws), "wgnn_fwd_state(T = 1)")
        return ["Y", "h_n"]

    def oracle(r, res):
        _, f = _fp64_model(r.c)
        with torch.no_grad():
            Yr, hnr = f(r.c.X.float(), r.c.h0.double())
        _check_Y(r, res, "Y", Yr)
        _check_Y(r, res, "h_n", hnr)
        assert torch.equal(res["Y"], res["h_n"])                         # T = 1: the one output row is the new state

    c = _build(cid, ("f32", torch.float32, 34, 1, B, H, 0))
    base = None
    for fill in FILLS:
        r = Run(c, fill)
        res = r.collect(flow(r))
        if fill == "zero":
            base = res
            oracle(r, res)
        else:
            _same(base, res, "%s [%s]" % (cid, fill))


# ---------------------------------------------------------------------------------------------------------------- row ranges
@pytest.mark.parametrize("cid", ["rows-f32", "rows-f16x3"])
def test_bwd_rows_and_finish_rows(cid):
    """After part 1 on the SAME workspace: two row ranges of each GRU pair, the second ending at the last (ragged) row; "the
    rest of g is not touched" -- the gradient rows outside a range still hold the fill, bit for bit.  Then wgnn_finish_rows."""
    c = _case(cid)
    G3 = 3 * c.H
    L = _lib()
    base = None
    left = _donor_leftovers(FLOW_LOSS[(1, 1)], DONOR[c.math], ())
    for fill, dirty, seed in [(f, None, 0) for f in FILLS] + [("finite", left, 1)]:
        r = Run(c, fill, dirty=dirty, seed=seed)
        lib, d, ps, gs, ad = r.lib, C.byref(r.d), r.params("prepared" if r.prep_bytes else None), r.grads(), r.adam()
        align = lib.wgnn_bwd_rows_align(d)
        assert align > 0 and G3 % align != 0, (align, G3)                # the last range is ragged
        first = align * max(1, (G3 // align) // 2)
        ranges = [(0, first), (first, G3 - first)]
        if r.prep_bytes:
            r.ok(lib.wgnn_prepare_weights(d, C.byref(ps), *r.ws), "wgnn_prepare_weights")
            r.repoison_ws()
        r.ok(lib.wgnn_fwd_loss(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("L"), r.ptr("Y"), r.ptr("stash"), *r.ws), "wgnn_fwd_loss")
        r.repoison_ws()
        r.ok(lib.wgnn_bwd_mse_part(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("Y"), r.ptr("L"), C.c_float(1.0), r.ptr("loss"),
                                   r.ptr("stash"), C.byref(gs), *r.ws, 1 | 8), "wgnn_bwd_mse_part(1 | 8)")
        # refused before any launch: a state stash's ranges
        snap = r.a.mem.clone()
        assert lib.wgnn_bwd_rows(d, r.ptr("Y"), r.ptr("stash"), C.byref(gs), L.ROWS_IH | L.ROWS_STATE, 0, first, *r.ws) == -5
        torch.cuda.synchronize()
        assert torch.equal(snap, r.a.mem)
        for which, wname, bname, ncols in ((L.ROWS_IH, "g.gru.weight_ih_l0", "g.gru.bias_ih_l0", c.S * F),
                                           (L.ROWS_HH, "g.gru.weight_hh_l0", "g.gru.bias_hh_l0", c.H)):
            for row0, rows in ranges:
                before_w, before_b = r.a[wname].host().view(torch.int32), r.a[bname].host().view(torch.int32)
                r.ok(lib.wgnn_bwd_rows(d, r.ptr("Y"), r.ptr("stash"), C.byref(gs), which, row0, rows, *r.ws),
                     "wgnn_bwd_rows(%d, %d, %d)" % (which, row0, rows))
                after_w, after_b = r.a[wname].host().view(torch.int32), r.a[bname].host().view(torch.int32)
                keep = torch.ones(G3, dtype=torch.bool)
                keep[row0:row0 + rows] = False
                assert torch.equal(after_w.reshape(G3, ncols)[keep], before_w.reshape(G3, ncols)[keep]), (cid, fill, which, row0)
                assert torch.equal(after_b[keep], before_b[keep]), (cid, fill, which, row0)
        r.ok(lib.wgnn_bwd_mse_part(d, r.ptr("A"), r.ptr("X"), C.byref(ps), r.ptr("Y"), r.ptr("L"), C.c_float(1.0), r.ptr("loss"),
                                   r.ptr("stash"), C.byref(gs), *r.ws, 2), "wgnn_bwd_mse_part(2)")
        for which in (L.ROWS_IH, L.ROWS_HH):
            for row0, rows in ranges:
                r.ok(lib.wgnn_finish_rows(d, C.byref(ps), C.byref(gs), which, row0, rows, C.byref(ad), *r.ws),
                     "wgnn_finish_rows(%d, %d, %d)" % (which, row0, rows))
        names = ["Y", "loss"] + GRAD_NAMES + [pre + k for pre in ("p.", "m.", "v.") for k in PARAM_KEYS[4:]]
        names += ["prepared"] if r.prep_bytes else []
        res = r.collect(names, poison_free=set(["Y", "loss"] + GRAD_NAMES + ["prepared"]))
        if base is None:
            base = res
            _check_Y(r, res)
            _check_loss(r, res)
            _check_grads(r, res)
        else:
            _same(base, res, "%s [%s%s]" % (cid, fill, ", on the leftovers of %s" % DONOR[c.math] if dirty else ""))


# ---------------------------------------------------------------------------------------------------------------- the layers
def _layer_run(fill, nt, S, Fi, Fo, csr_k, want_dx):
    from windgnn_amd.graph import CsrAdjacency, build_knn_adjacency, synthetic_station_coords
    L = _lib()
    lib = L.load()
    g = torch.Generator().manual_seed(77 + S + Fi + Fo)
    if csr_k:
        csr = CsrAdjacency(*build_knn_adjacency(synthetic_station_coords(S, seed=3), csr_k))
        A_host, A_dat, nnz = csr.dense(), csr.blob, csr.nnz
    else:
        A_host = torch.rand(S, S, generator=g) / S + 0.01
        A_dat, nnz = A_host, 0
    X = torch.rand(nt, S, Fi, generator=g)
    W = torch.randn(Fi, Fo, generator=g) * 0.5
    b = torch.randn(Fo, generator=g) * 0.1
    dout = torch.randn(nt, S, Fo, generator=g)
    wsb = lib.wgnn_gcn_layer_csr_workspace_bytes(nt, S, Fi) if csr_k else lib.wgnn_gcn_layer_workspace_bytes(nt, S, Fi, Fo)
    assert wsb > 0
    a = Arena(_dev(), fill)
    for name, t in (("A", A_dat), ("X", X), ("W", W), ("b", b), ("dout", dout)):
        a.buf(name, t.numel() * 4, data=t)
    a.buf("out", nt * S * Fo * 4)
    a.buf("dW", Fi * Fo * 4)
    a.buf("db", Fo * 4)
    a.buf("dX", nt * S * Fi * 4)
    a.buf("ws", wsb)
    a.commit()
    P = lambda n: C.c_void_p(a[n].ptr) if n else C.c_void_p(0)     # noqa: E731
    st = C.c_void_p(0)
    if csr_k:
        rc = lib.wgnn_gcn_layer_csr_fwd(nt, S, Fi, nnz, P("A"), P("X"), P("W"), P("b"), P("out"), st)
        assert rc == 0, rc
        rc = lib.wgnn_gcn_layer_csr_bwd(nt, S, Fi, nnz, P("A"), P("X"), P("W"), P("out"), P("dout"), P("dW"), P("db"),
                                        P("dX" if want_dx else None), P("ws"), C.c_size_t(wsb), st)
    else:
        rc = lib.wgnn_gcn_layer_fwd(nt, S, Fi, Fo, P("A"), P("X"), P("W"), P("b"), P("out"), st)
        assert rc == 0, rc
        rc = lib.wgnn_gcn_layer_bwd(nt, S, Fi, Fo, P("A"), P("X"), P("W"), P("out"), P("dout"), P("dW"), P("db"),
                                    P("dX" if want_dx else None), P("ws"), C.c_size_t(wsb), st)
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert a.check() == {}, (fill, a.check())
    names = ["out", "dW", "db"] + (["dX"] if want_dx else [])
    res = {n: a[n].host() for n in names}
    if fill != "zero":
        for n in names:
            assert a[n].unwritten(4) == 0, (fill, n)
        if not want_dx:
            assert a["dX"].unwritten(4) == nt * S * Fi                     # not an argument: still the fill
    return res, (A_host, X, W, b, dout)


def _layer_case(nt, S, Fi, Fo, csr_k, want_dx):
    from oracle import windgnn_oracle as orc
    base = None
    for fill in FILLS:
        res, (A, X, W, b, dout) = _layer_run(fill, nt, S, Fi, Fo, csr_k, want_dx)
        if fill != "zero":
            _same(base, res, "layer %s [%s]" % ((nt, S, Fi, Fo, csr_k), fill))
            continue
        base = res
        X64, W64, b64 = (t.double().requires_grad_(True) for t in (X, W, b))
        out, _ = orc.gcn_layer_fwd(A.double(), X64, W64, b64)
        (out * dout.double()).sum().backward()
        assert max_abs(res["out"].view(torch.float32).reshape(out.shape), out.detach()) <= Y_TOL
        assert rel_to_max(res["dW"].view(torch.float32).reshape(W.shape), W64.grad) <= G_TOL
        assert rel_to_max(res["db"].view(torch.float32), b64.grad) <= G_TOL
        if want_dx:
            assert rel_to_max(res["dX"].view(torch.float32).reshape(X.shape), X64.grad) <= G_TOL


@pytest.mark.parametrize("want_dx", [True, False], ids=["dX", "no_dX"])
@pytest.mark.parametrize("Fi,Fo", [(6, 9), (13, 40), (64, 64), (1, 1), (13, 13)])
@pytest.mark.parametrize("S", [7, 34, 3, 64])
def test_gcn_layer_dense(S, Fi, Fo, want_dx):
    _layer_case(5, S, Fi, Fo, 0, want_dx)


@pytest.mark.parametrize("want_dx", [True, False], ids=["dX", "no_dX"])
def test_gcn_layer_csr(want_dx):
    _layer_case(5, 200, 13, 13, 8, want_dx)


def flow_gru(r):
    """wgnn_gru_fwd / wgnn_gru_bwd on a caller-supplied g (the X buffer: the same [B,T,S*13] fp32 bytes), conv slots NULL; dg
    is an output buffer of its own."""
    lib, d = r.lib, C.byref(r.d)
    ps, gs = r.params(), r.grads()
    for f in ("conv1_weight", "conv1_bias", "conv2_weight", "conv2_bias"):
        setattr(ps, f, 0)
        setattr(gs, f, 0)
    r.ok(lib.wgnn_gru_fwd(d, r.ptr("X"), C.byref(ps), r.ptr("Y"), r.ptr("stash"), *r.ws), "wgnn_gru_fwd")
    r.repoison_ws()
    r.ok(lib.wgnn_gru_bwd(d, r.ptr("X"), C.byref(ps), r.ptr("Y"), r.ptr("dY"), r.ptr("stash"), C.byref(gs), r.ptr("dg"), *r.ws),
         "wgnn_gru_bwd")
    return ["Y", "dg"] + GRAD_NAMES[4:]


@pytest.mark.parametrize("cid", ["small_odd", "rec32", "f32_h129"])
def test_gru_fwd_bwd_alone(cid):
    c = _case(cid)
    base = None
    for fill, on_leftovers, seed in [(f, False, 0) for f in FILLS] + [("finite", True, 1)]:
        dirty = _donor_leftovers(flow_fwd_bwd, DONOR[c.math], ()) if on_leftovers else None
        r = Run(c, fill, dirty=dirty, seed=seed, extra=(("dg", torch.float32, (c.B, c.T, c.S * F)),))
        res = r.collect(flow_gru(r))
        conv_untouched = all(r.a["g." + k].unwritten(4) == c.p[k].numel() for k in PARAM_KEYS[:4])
        if fill != "zero":
            assert conv_untouched                                          # NULL slots: not arguments
        if base is None:
            base = res
            leaves, f = _fp64_model(c)
            gin = c.X.double().reshape(c.B, c.T, c.S * F).requires_grad_(True)
            Yr, _hn = f(None, torch.zeros(c.B, c.H, dtype=torch.float64), g_in=gin)
            (Yr * c.dY.double()).sum().backward()
            _check_Y(r, res, "Y", Yr.detach())
            assert rel_to_max(r.tensor("dg", res), gin.grad) <= c.g_tol
            for k in PARAM_KEYS[4:]:
                assert rel_to_max(r.tensor("g." + k, res), leaves[k].grad) <= c.g_tol, k
        else:
            _same(base, res, "%s gru [%s%s]" % (cid, fill, " dirty" if dirty else ""))


# ---------------------------------------------------------------------------------------------------------------- small ops
def _simple(fill, bufs, call, outs):
    """bufs: [(name, nbytes, data or None)]; call(P) issues the entry point with P(name) -> pointer.  Outputs that start out
    as the fill (no data) must not hold it afterwards."""
    fresh = {name for name, _, data in bufs if data is None}
    a = Arena(_dev(), fill)
    for name, n, data in bufs:
        a.buf(name, n, data=data)
    a.commit()
    rc = call(lambda n: C.c_void_p(a[n].ptr) if n else C.c_void_p(0))
    assert rc == 0, rc
    torch.cuda.synchronize()
    assert a.check() == {}, (fill, a.check())
    if fill != "zero":
        for n in outs:
            assert n not in fresh or a[n].unwritten(4) == 0, (fill, n)
    return {n: a[n].host() for n in outs}


def _three_fills(bufs, call, outs):
    base = _simple("zero", bufs, call, outs)
    for fill in FILLS[1:]:
        _same(base, _simple(fill, bufs, call, outs), fill)
    return {n: v.view(torch.float32) for n, v in base.items()}


@pytest.mark.parametrize("n", [1, 1023, 4097])
def test_mse_loss_grad(n):
    lib = _lib().load()
    g = torch.Generator().manual_seed(n)
    Y, Lb = torch.rand(n, generator=g), torch.rand(n, generator=g)
    bufs = [("Y", 4 * n, Y), ("L", 4 * n, Lb), ("dY", 4 * n, None), ("loss", 4, None), ("ws", 4096, None)]
    res = _three_fills(bufs, lambda P: lib.wgnn_mse_loss_grad(P("Y"), P("L"), n, C.c_float(0.5), P("dY"), P("loss"), P("ws"),
                                                              C.c_size_t(4096), C.c_void_p(0)), ["dY", "loss"])
    dref = Y.double() - Lb.double()
    assert abs(float(res["loss"][0]) - float((dref * dref).mean())) <= 1e-5
    assert rel_to_max(res["dY"], dref * (2.0 * 0.5 / n)) <= 1e-6


@pytest.mark.parametrize("n", [1, 169, 4099])
def test_adam_step(n):
    lib = _lib().load()
    g = torch.Generator().manual_seed(n)
    p, gr = torch.randn(n, generator=g), torch.randn(n, generator=g) * 1e-2
    m, v = torch.randn(n, generator=g) * 1e-3, torch.rand(n, generator=g) * 1e-4
    bufs = [("p", 4 * n, p), ("g", 4 * n, gr), ("m", 4 * n, m), ("v", 4 * n, v)]
    res = _three_fills(bufs, lambda P: lib.wgnn_adam_step(P("p"), P("g"), P("m"), P("v"), n, 3, C.c_float(1e-3), C.c_float(0.9),
                                                          C.c_float(0.999), C.c_float(1e-8), C.c_void_p(0)), ["p", "m", "v", "g"])
    m2 = B1 * m.double() + (1 - B1) * gr.double()
    v2 = B2 * v.double() + (1 - B2) * gr.double() ** 2
    p2 = p.double() - LR / (1 - B1 ** 3) * m2 / ((v2 / (1 - B2 ** 3)).sqrt() + EPS)
    assert torch.equal(res["g"], gr)                                        # the gradient is an input
    assert rel_to_max(res["m"], m2) <= 1e-6 and rel_to_max(res["v"], v2) <= 1e-6
    assert max_abs(res["p"], p2) <= 1e-6


@pytest.mark.parametrize("B,T,H", [(1, 1, 1), (5, 12, 21), (37, 24, 102)])
def test_predict_last(B, T, H):
    lib = _lib().load()
    Y = torch.rand(B, T, H, generator=torch.Generator().manual_seed(B + H))
    bufs = [("Y", 4 * B * T * H, Y), ("out", 4 * B * H, None)]
    res = _three_fills(bufs, lambda P: lib.wgnn_predict_last(P("Y"), B, T, H, C.c_float(-2.5), C.c_float(31.0), P("out"),
                                                             C.c_void_p(0)), ["out"])
    assert rel_to_max(res["out"].reshape(B, H), Y[:, -1, :].double() * 33.5 - 2.5) <= 1e-6


@pytest.mark.parametrize("starts", [False, True], ids=["default_starts", "given_starts"])
@pytest.mark.parametrize("Ttot,S,seq", [(131, 7, 12), (75, 3, 24)], ids=["w1_t131_s7_seq12", "w2_t75_s3_seq24"])
def test_make_windows(Ttot, S, seq, starts):
    """The two window fixtures' sizes (feature array [Ttot, S, 13]); a pure gather: exact against host indexing."""
    lib = _lib().load()
    feat = torch.rand(Ttot, S, F, generator=torch.Generator().manual_seed(Ttot))
    t0 = [(i * 7) % (Ttot - seq - 3) for i in range(6)] if starts else [i * seq for i in range(Ttot // seq)]
    B = len(t0)
    host = (C.c_int32 * B)(*t0) if starts else None
    bufs = [("feat", 4 * feat.numel(), feat), ("starts", 4 * B, torch.tensor(t0, dtype=torch.int32)),
            ("X", 4 * B * seq * S * F, None), ("L", 4 * B * seq * 3 * S, None)]
    res = _three_fills(bufs, lambda P: lib.wgnn_make_windows(P("feat"), Ttot, S, F, seq, 11, host, P("starts" if starts else None),
                                                             B, P("X"), P("L"), C.c_void_p(0)), ["X", "L"])
    X = torch.stack([feat[t:t + seq] for t in t0])
    Lr = torch.stack([torch.cat([feat[t + k + 1:t + k + 1 + seq, :, 11] for k in range(3)], dim=1) for t in t0])
    assert torch.equal(res["X"].reshape(X.shape), X)
    assert torch.equal(res["L"].reshape(Lr.shape), Lr)


# ---------------------------------------------------------------------------------------------------------------- alignment
@pytest.mark.parametrize("cid", ["small_odd", "x3-33x1x19x100", "io16-f16x3-fp16", "io16-f16-bf16"])
def test_io_tensors_at_the_documented_minimum_alignment(cid):
    """include/windgnn.h: X, Y, labels and dY need the alignment of their element type only (4 bytes, 2 for 16-bit I/O).  X,
    labels, dY and Y one element past a 256-byte boundary: bitwise the aligned run, plus (a)-(c)."""
    c = _case(cid)
    es = 4 if c.iodt == torch.float32 else 2
    for flow in (flow_fwd_bwd, FLOW_LOSS[(0, 0)]):
        base = Run(c, "zero")
        ref = base.collect(flow(base))
        for fill in ("zero", "nan"):
            r = Run(c, fill, off=1)
            assert r.a["X"].ptr % 256 == es and r.a["Y"].ptr % 256 == es and r.a["L"].ptr % 256 == es
            assert r.a["dY"].ptr % 256 == 4
            _same(ref, r.collect(flow(r)), "%s at %d-byte alignment [%s]" % (cid, es, fill))


def test_host_bindings_refuse_a_stash_or_prepared_off_a_256_byte_boundary():
    """The raw bindings hand a misaligned stash / `prepared` to no kernel (include/windgnn.h, "Alignment"); tensors may start
    at any element: X[1:] of a (7, T = 1) batch, 364 bytes into its storage, gives the rows of the whole batch bit for bit."""
    from windgnn_amd.functional import gcn_gru_backward_raw, gcn_gru_forward_raw, prepared_weights, refresh_prepared
    dev = _dev()
    c = _case("small_odd")
    params = [c.p[k].to(dev) for k in PARAM_KEYS]
    A = c.A_host.to(dev)
    X = torch.rand(7, 1, c.S, F, generator=torch.Generator().manual_seed(5)).to(dev)
    assert (X[1:].data_ptr() - X.data_ptr()) == 364 and X[1:].is_contiguous()
    Yall, _, _ = gcn_gru_forward_raw(A, X, params, MATH["f32"], want_stash=False)
    Ytail, stash, d = gcn_gru_forward_raw(A, X[1:], params, MATH["f32"])
    assert torch.equal(Ytail, Yall[1:])
    grads = [torch.empty_like(q) for q in params]
    dY = torch.rand_like(Ytail)
    gcn_gru_backward_raw(d, A, X[1:], params, Ytail, dY, stash, grads)
    big = torch.empty(stash.numel() + 256, dtype=torch.uint8, device=dev)
    moved = big[4:4 + stash.numel()].copy_(stash)
    with pytest.raises(RuntimeError, match="stash must start on a 256-byte boundary"):
        gcn_gru_backward_raw(d, A, X[1:], params, Ytail, dY, moved, [torch.empty_like(q) for q in params])
    pre = prepared_weights(d, params, dev)
    assert pre is not None and pre.data_ptr() % 256 == 0
    big = torch.empty(pre.numel() + 256, dtype=torch.uint8, device=dev)
    with pytest.raises(RuntimeError, match="prepared must start on a 256-byte boundary"):
        refresh_prepared(d, params, big[16:16 + pre.numel()])
    torch.cuda.synchronize()
