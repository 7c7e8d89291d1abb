"""CPU-side checks: the C-ABI library loads and exports every symbol include/windgnn.h declares,
argument validation works without touching a GPU, and the module mirrors the reference's API."""
import ctypes
import os
import re

import pytest
import numpy as np
import torch

from conftest import PARAM_KEYS, ROOT, load_fixture


def _lib():
    from windgnn_amd import _lib as L
    from windgnn_amd import build
    build.build(verbose=False)
    return L, L.load()


def test_every_declared_symbol_is_exported():
    L, lib = _lib()
    hdr = open(os.path.join(ROOT, "include", "windgnn.h")).read()
    declared = set(re.findall(r"\b(wgnn_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(L.EXPORTS), (declared ^ set(L.EXPORTS))
    for name in declared:
        assert hasattr(lib, name), name
    assert lib.wgnn_version() == 122


def _header_prototypes():
    """{name: (return type, [argument type strings])} of every wgnn_* function include/windgnn.h declares."""
    hdr = open(os.path.join(ROOT, "include", "windgnn.h")).read()
    hdr = re.sub(r"/\*.*?\*/", " ", hdr, flags=re.S)
    hdr = re.sub(r"//[^\n]*", " ", hdr)
    protos = {}
    for m in re.finditer(r"([A-Za-z_][A-Za-z0-9_ \*]*?)\b(wgnn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;", hdr):
        ret, name, args = " ".join(m.group(1).split()), m.group(2), " ".join(m.group(3).split())
        protos[name] = (ret, [] if args in ("", "void") else [a.strip() for a in args.split(",")])
    return protos


def _ctype_kind(t):
    """Coarse class of a ctypes argument type, comparable with a C declaration."""
    if t in (ctypes.c_void_p, ctypes.c_char_p) or hasattr(t, "_type_") and not isinstance(t._type_, str):
        return "ptr"
    return {ctypes.c_float: "float", ctypes.c_double: "double", ctypes.c_int64: "i64", ctypes.c_size_t: "size",
            ctypes.c_int: "i32", ctypes.c_int32: "i32"}[t]


def _c_kind(decl):
    if "*" in decl:
        return "ptr"
    words = decl.replace("const", " ").split()
    base = " ".join(words[:-1]) if len(words) > 1 else words[0]      # drop the parameter name
    return {"float": "float", "double": "double", "int64_t": "i64", "size_t": "size", "int": "i32", "int32_t": "i32"}[base]


def test_ctypes_prototypes_match_the_header_argument_for_argument():
    """windgnn_amd/_lib.py mirrors include/windgnn.h by hand; an argument added to one and not the other would pass the
    name check above and corrupt the call on the GPU box.  Every prototype is parsed out of the header and compared with
    _lib.EXPORTS: argument count, and the class of every argument (pointer / float / double / int32 / int64 / size_t)."""
    from windgnn_amd import _lib as L
    protos = _header_prototypes()
    assert set(protos) == set(L.EXPORTS), set(protos) ^ set(L.EXPORTS)
    for name, (ret, args) in protos.items():
        res, argtypes = L.EXPORTS[name]
        assert len(args) == len(argtypes), (name, args, argtypes)
        for i, (decl, t) in enumerate(zip(args, argtypes)):
            assert _c_kind(decl) == _ctype_kind(t), (name, i, decl, t)
        want = "ptr" if "*" in ret else {"int": "i32", "size_t": "size"}[ret.replace("const", "").strip()]
        assert _ctype_kind(res) == want, (name, ret, res)


def test_dims_validation_no_gpu_needed():
    L, lib = _lib()
    ok = L.Dims(4, 24, 34, 13, 102, 0, 0, 0)
    assert lib.wgnn_workspace_bytes(ctypes.byref(ok)) > 0
    assert lib.wgnn_stash_bytes(ctypes.byref(ok)) > 0
    for bad in (L.Dims(0, 24, 34, 13, 102, 0, 0, 0), L.Dims(4, 24, 34, 12, 102, 0, 0, 0),
                L.Dims(4, 24, 65, 13, 195, 0, 0, 0),           # dense adjacency beyond the LDS-resident path
                L.Dims(4, 24, 4096, 13, 12288, 0, 1, 0),       # CSR without entries
                L.Dims(4, 24, 34, 13, 102, 0, 2, 0)):          # unknown adjacency format
        assert lib.wgnn_workspace_bytes(ctypes.byref(bad)) == 0
    c5 = L.Dims(128, 24, 4096, 13, 12288, 0, 1, 73000)        # BASELINE configs[4], one GPU's shard
    assert lib.wgnn_workspace_bytes(ctypes.byref(c5)) > (1 << 32) and lib.wgnn_stash_bytes(ctypes.byref(c5)) > 0
    assert lib.wgnn_workspace_bytes(ctypes.byref(L.Dims(4, 24, 34, 13, 400, 1, 0, 0))) > 0   # wide GRU: general path
    assert lib.wgnn_workspace_bytes(ctypes.byref(L.Dims(4096, 24, 34, 13, 102, L.MATH_F16X3G, 0, 0))) > 0   # bench.py's mode
    assert lib.wgnn_workspace_bytes(ctypes.byref(L.Dims(4, 24, 34, 13, 102, 4, 0, 0))) == 0                # unknown math mode
    # 16-bit X / Y / labels (wgnn_io): only with the fp16-plane kernels (math f16x3 / f16, dense adjacency, H <= 127)
    assert lib.wgnn_workspace_bytes(ctypes.byref(L.Dims(4, 24, 34, 13, 102, 1, 0, 0, L.IO_BF16))) > 0
    assert lib.wgnn_workspace_bytes(ctypes.byref(L.Dims(4, 24, 34, 13, 102, 2, 0, 0, L.IO_F16))) > 0
    for bad in (L.Dims(4, 24, 34, 13, 102, 0, 0, 0, L.IO_F16),       # exact-fp32 math has no 16-bit I/O
                L.Dims(4, 24, 34, 13, 400, 1, 0, 0, L.IO_F16),       # wide GRU: general path
                L.Dims(4, 24, 200, 13, 60, 1, 1, 1000, L.IO_BF16),   # CSR adjacency
                L.Dims(4, 24, 34, 13, 102, 1, 0, 0, 3)):             # unknown I/O type
        assert lib.wgnn_workspace_bytes(ctypes.byref(bad)) == 0
    p = L.Params()
    rc = lib.wgnn_fwd(ctypes.byref(ok), None, None, ctypes.byref(p), None, None, None, 0, None)
    assert rc == -1 and b"NULL" in lib.wgnn_strerror(rc)
    bad = L.Dims(4, 24, 34, 12, 102, 0, 0, 0)
    assert lib.wgnn_fwd(ctypes.byref(bad), None, None, ctypes.byref(p), None, None, None, 0, None) == -2


def test_finish_and_prepared_entry_points_validate_without_a_gpu():
    L, lib = _lib()
    x3 = L.Dims(4, 24, 34, 13, 102, 1, 0, 0)
    f32 = L.Dims(4, 24, 34, 13, 102, 0, 0, 0)
    wide = L.Dims(4, 24, 34, 13, 400, 0, 0, 0)            # wide GRU in exact fp32: W_ih is staged as it is
    nx, nf = lib.wgnn_prepared_bytes(ctypes.byref(x3)), lib.wgnn_prepared_bytes(ctypes.byref(f32))
    assert nx > 4 * 306 * 442 and nf > 8 * 306 * 442      # two images of W_ih each (fp16 hi+lo planes / padded fp32)
    assert lib.wgnn_prepared_bytes(ctypes.byref(wide)) == 0
    # the images depend on S, H and math only: one buffer serves every batch size
    assert lib.wgnn_prepared_bytes(ctypes.byref(L.Dims(4096, 24, 34, 13, 102, 1, 0, 0))) == nx
    assert lib.wgnn_prepared_bytes(ctypes.byref(L.Dims(4096, 24, 34, 13, 102, 0, 0, 0))) == nf
    p, g = L.Params(), L.Grads()
    assert p.prepared is None                              # the 9th slot of wgnn_params defaults to NULL
    assert lib.wgnn_finish(ctypes.byref(x3), ctypes.byref(p), None, 6, None, None, 0, None) == -1
    assert lib.wgnn_finish(ctypes.byref(x3), ctypes.byref(p), ctypes.byref(g), 8, None, None, 0, None) == -2
    assert lib.wgnn_finish(ctypes.byref(x3), ctypes.byref(p), ctypes.byref(g), 0, None, None, 0, None) == -2
    # the per-family optimiser step needs an optimiser, no reduce bit, and one family at a time
    assert lib.wgnn_finish(ctypes.byref(x3), ctypes.byref(p), ctypes.byref(g), L.FINISH_ADAM_GRU, None, None, 0, None) == -2
    ad = L.Adam()
    ad.step = 1
    for bad_which in (L.FINISH_ADAM_GRU | 4, L.FINISH_ADAM_CONV | 2, L.FINISH_ADAM_GRU | L.FINISH_ADAM_CONV, 64):
        assert lib.wgnn_finish(ctypes.byref(x3), ctypes.byref(p), ctypes.byref(g), bad_which, ctypes.byref(ad), None, 0, None) == -2
    assert lib.wgnn_prepare_weights(ctypes.byref(x3), ctypes.byref(p), None, 0, None) == -1
    bad = L.Dims(4, 24, 34, 12, 102, 1, 0, 0)
    assert lib.wgnn_finish(ctypes.byref(bad), ctypes.byref(p), ctypes.byref(g), 6, None, None, 0, None) == -2
    assert ctypes.sizeof(L.Adam) == 2 * 8 * ctypes.sizeof(ctypes.c_void_p) + 5 * 4 + 4   # wgnn_adam, padded to 8


def test_module_mirrors_reference_state_dict():
    from windgnn_amd import GCN_GRU
    m = GCN_GRU(input_dim=13, hidden_dim=13, output_dim=13, gru_input=34 * 13, gru_hidden_dim=102)
    sd = m.state_dict()
    assert list(sd.keys()) == PARAM_KEYS
    fx = load_fixture("f3_s34_t24_b4_ckpt")          # parameters of the shipped wind_gnn_34.pth
    m.load_state_dict(fx["params"])
    assert sum(p.numel() for p in m.parameters()) == 167440
    for k in PARAM_KEYS:
        assert sd[k].shape == fx["params"][k].shape


def test_no_cpu_fallback():
    from windgnn_amd import GCN_GRU
    m = GCN_GRU(13, 13, 13, 7 * 13, 21)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        m(torch.rand(7, 7), torch.rand(1, 12, 7, 13))


def test_product_does_not_import_oracle():
    pkg = os.path.join(ROOT, "windgnn_amd")
    for dp, _, fs in os.walk(pkg):
        for f in fs:
            if f.endswith((".py", ".hip", ".h")):
                src = open(os.path.join(dp, f)).read()
                assert "import oracle" not in src and "from oracle" not in src, f


def test_build_graph_matches_reference_output():
    """N1: windgnn_amd.graph against the adjacency the reference's build_graph produced (golden)."""
    import numpy as np
    import pandas as pd
    from conftest import GOLDEN
    from windgnn_amd.graph import build_adjacency, build_graph
    z = np.load(os.path.join(GOLDEN, "graph_7_34.npz"))
    assert np.abs(build_adjacency(z["coords34"]) - z["A34"]).max() <= 1e-12
    assert np.abs(build_adjacency(z["coords34"][:7]) - z["A7"]).max() <= 1e-12
    df = pd.DataFrame({"Station Name": ["s%d" % i for i in range(34)] * 2,
                       "Latitude": list(z["coords34"][:, 0]) * 2, "Longitude": list(z["coords34"][:, 1]) * 2})
    assert np.abs(build_graph(df) - z["A34"]).max() <= 1e-12      # duplicates dropped, first-appearance order


def test_knn_csr_adjacency_host_logic():
    """N1 (CSR emitter): symmetric k-NN sparsification of the reference's weights, normalised; the C-ABI blob
    holds A and A^T."""
    from windgnn_amd.graph import CsrAdjacency, build_adjacency, build_knn_adjacency, synthetic_station_coords
    c = synthetic_station_coords(60, seed=3)
    rp, col, val = build_knn_adjacency(c, 8)
    csr = CsrAdjacency(rp, col, val)
    D = csr.dense().double().numpy()
    assert np.abs(D - D.T).max() < 1e-7                      # symmetric by construction
    assert np.all(np.diag(D) > 0) and csr.nnz >= 60 * 9      # self loops + at least k neighbours per row
    assert np.all(np.diff(rp) >= 9)
    # with k = S-1 nothing is dropped: it must equal the reference's dense construction
    rp2, col2, val2 = build_knn_adjacency(c, 59)
    assert np.abs(CsrAdjacency(rp2, col2, val2).dense().double().numpy() - build_adjacency(c)).max() < 1e-6
    # blob layout of include/windgnn.h: A then A^T, each rowptr | col | val
    S, nnz = csr.S, csr.nnz
    b = csr.blob.numpy()
    assert b.shape[0] == 2 * (S + 1 + 2 * nnz)
    t = b[S + 1 + 2 * nnz:]
    trp, tcol, tval = t[:S + 1], t[S + 1:S + 1 + nnz], t[S + 1 + nnz:].view(np.float32)
    DT = np.zeros((S, S), np.float32)
    for r in range(S):
        DT[r, tcol[trp[r]:trp[r + 1]]] = tval[trp[r]:trp[r + 1]]
        assert np.all(np.diff(tcol[trp[r]:trp[r + 1]]) > 0)
    assert np.abs(DT - D.T.astype(np.float32)).max() == 0.0
    with pytest.raises(ValueError):
        CsrAdjacency([0, 1], [5], [1.0])


def test_csr_adjacency_for_another_graph_is_refused_on_the_host():
    """The kernels find rowptr / col / val inside the CSR buffer from S and nnz; a buffer built for a different
    station count (or a corrupted one) must never reach them (out-of-bounds device reads otherwise)."""
    from windgnn_amd.functional import _adj
    from windgnn_amd.graph import CsrAdjacency, build_knn_adjacency, synthetic_station_coords
    csr = CsrAdjacency(*build_knn_adjacency(synthetic_station_coords(20, seed=1), 4))
    with pytest.raises(RuntimeError, match="does not match 34 stations"):
        _adj(csr, 34)
    with pytest.raises(RuntimeError, match="no CPU fallback"):      # right graph, but still on the host
        _adj(csr, 20)
    csr.blob = csr.blob[:-1]
    with pytest.raises(RuntimeError, match="words"):
        _adj(csr, 20)
    csr.blob = torch.zeros(2 * 21 + 4 * csr.nnz, dtype=torch.int64)
    with pytest.raises(RuntimeError, match="int32"):
        _adj(csr, 20)


def test_scratch_buffers_off_a_256_byte_boundary_are_refused_on_the_host():
    """include/windgnn.h, "Alignment": tensors need their element's alignment (every torch view has it), but the stash and the
    `prepared` images are read by LDS-DMA and 16-byte loads at offsets laid out from a 256-byte-aligned base.  The bindings
    refuse a slice of a larger buffer before its pointer reaches a kernel; a buffer of its own passes, and so does None."""
    from windgnn_amd import _lib
    from windgnn_amd.functional import SCRATCH_ALIGN, _params_struct, _require_scratch_aligned, _stash_ptr
    assert SCRATCH_ALIGN == 256
    big = torch.empty(4096, dtype=torch.uint8)
    o = (-big.data_ptr()) % 256                                     # host allocations are 64-byte aligned only
    good = big[o:o + 1024]
    _require_scratch_aligned(stash=good, prepared=None)
    assert _stash_ptr(good).value == good.data_ptr() and _stash_ptr(None).value is None
    for off in (1, 4, 16, 64, 128):
        with pytest.raises(RuntimeError, match="stash must start on a 256-byte boundary"):
            _stash_ptr(big[o + off:o + off + 1024])
    params = [torch.zeros(4) for _ in range(8)]
    assert _params_struct(_lib.Params, params, good).prepared == good.data_ptr()
    with pytest.raises(RuntimeError, match="prepared must start on a 256-byte boundary"):
        _params_struct(_lib.Params, params, big[o + 364:o + 364 + 1024])      # e.g. 364 bytes into its storage
    # tensors: element alignment is the contract, so a contiguous slice of a batch is taken as it is
    X = torch.zeros(7, 1, 7, 13)
    assert X[1:].is_contiguous() and (X[1:].data_ptr() - X.data_ptr()) == 364
    assert _params_struct(_lib.Grads, [X[1:]] * 8).conv1_weight == X[1:].data_ptr()


def test_reference_import_header_resolves_with_the_documented_swap():
    """src/main.py gets `nn`, `torch`, `np` and GraphConvLayer only through its star
    imports (src/main.py:4-8; step6 does `import torch.nn as nn`).  With the documented replacement lines every
    name the loop body uses (src/main.py:41-52,64-108) must still resolve."""
    ns = {}
    exec("from windgnn_amd.dropin import *", ns)                      # the documented one-line swap
    for name in ("GCN_GRU", "GraphConvLayer", "nn", "torch"):
        assert name in ns, name
    assert ns["nn"].MSELoss is torch.nn.MSELoss                       # src/main.py:49
    m = ns["GCN_GRU"](input_dim=13, hidden_dim=13, output_dim=13, gru_input=7 * 13, gru_hidden_dim=21)
    assert list(m.state_dict().keys()) == PARAM_KEYS
    assert callable(ns["torch"].optim.Adam)                           # src/main.py:52


def test_host_asan_build_of_the_c_abi_is_clean():
    """the C-ABI library's host code (layouts, validation, launch wrappers) under AddressSanitizer
    (`hipcc -fsanitize=address -fno-gpu-sanitize`, CPU box only): 4032 shapes through every size function and every
    entry point's argument validation, no ASan report (tools/asan_host_check.py)."""
    import subprocess
    import sys
    if not os.path.exists("/opt/rocm/bin/hipcc"):
        pytest.skip("hipcc not available")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "asan_host_check.py")], stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:]
    assert "no report" in r.stdout
