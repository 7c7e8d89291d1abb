"""The host half of the largest-accepted-size tests (tests/large_offset_cases.py, tests/test_gpu_large_offset.py), no GPU:

  1. every case is accepted by the library's own size functions and by an entry point on fake pointers, and every operand a
     case names lies past the threshold it names -- recomputed from the layout formulas; a case that names none fails;
  2. for each limit of check_dims, series_plan, the layer entries and wgnn_predict_last the last accepted and the first refused
     shape (WGNN_ERR_SHAPE); the pair of the layers wider than 64 features is
     tests/test_layer_wide_host.py::test_an_element_count_of_two_to_the_31_is_a_shape_error;
  3. the inputs can show a wrap: a byte offset reduced mod 2^31 or 2^32 lands mid-row or on another phase for at least 99 % of
     the rows past the threshold (arithmetic only); on the oracle any two distinct phases differ by more than 10 x the case's
     bar, in Y and in the operand's own rows; one planted wrap per family (an X read, a GI read, a Y store) fails the
     comparison of the GPU module by message;
  4. every B is 48 R + r with r not in {0, 16, 32}.
The same four for the layer cases (tiles of period 48) and the series cases (hours of period 45).
A failure of tests/test_gpu_large_offset.py is therefore a finding about the kernels, not about the inputs."""
import ctypes as C

import numpy as np
import pytest
import torch

import large_offset_cases as lc
from test_gpu_gcn_loops import LAYER_TOL
from test_gpu_parity import F16_Y_TOL, IO_ROUND, Y_TOL

OK, ERR_NULL, ERR_SHAPE, ERR_WORKSPACE = 0, -1, -2, -4
T31, T32 = lc.T31, lc.T32


def _lib():
    from windgnn_amd import _lib as L
    from windgnn_amd import build
    build.build(verbose=False)
    return L.load()


def _fake_params():
    from windgnn_amd import _lib as L
    ps = L.Params()
    for i, (name, _) in enumerate(L.Params._fields_[:8]):
        setattr(ps, name, (i + 16) << 40)
    return ps


def _fwd_rc(lib, d):
    """wgnn_fwd on fake device pointers with a workspace of 0 bytes: the shape check comes first (WGNN_ERR_SHAPE), an accepted
    shape gets as far as the workspace check (WGNN_ERR_WORKSPACE); nothing is launched either way."""
    ps = _fake_params()
    p = [C.c_void_p((i + 1) << 40) for i in range(5)]
    return lib.wgnn_fwd(C.byref(d), p[0], p[1], C.byref(ps), p[2], p[3], p[4], C.c_size_t(0), None)


def _dims(B, T, S, H, math=0, csr=False, io=0):
    from windgnn_amd import _lib as L
    return L.Dims(B, T, S, 13, H, math, 1 if csr else 0, 8 * S if csr else 0, io)


def _case_bar(c, io="f32"):
    """The largest Y bar among the case's runs on this I/O type."""
    bars = [(F16_Y_TOL if m == "f16" else Y_TOL) + (IO_ROUND[lc.IO_DTYPE[i]] if i != "f32" else 0.0) for m, i, _ in c.runs if i == io]
    return max(bars)


# ==== 1. accepted, and past the thresholds =========================================================================================
@pytest.mark.parametrize("c", lc.STEPS, ids=[c.id for c in lc.STEPS])
def test_every_case_is_accepted_and_crosses_what_it_names(c):
    lib = _lib()
    assert c.B * c.T * c.S * 13 < T31 and c.B * c.T * 4 * c.H < T31 and c.B * c.T <= 1 << 30
    ios = sorted({io for _, io, _ in c.runs})
    for math, io, route in c.runs:
        d = c.dims(math, io)
        ws, st = lib.wgnn_workspace_bytes(C.byref(d)), lib.wgnn_stash_bytes(C.byref(d))
        assert ws > 0 and st > 0, (c.id, math, io)
        if route == "state":
            assert lib.wgnn_state_stash_bytes(C.byref(d)) > st
        assert _fwd_rc(lib, d) == ERR_WORKSPACE, (c.id, math, io)
        # the layout formulas of this table against the library's totals: g (and, split modes, GI) live in the stash, dGI and dg
        # in the workspace
        assert st >= c.bytes("g") and ws >= c.bytes("GI") + c.bytes("dg"), (c.id, math, io)
        if c.csr_k:
            assert st >= c.bytes("g") + c.bytes("h1") and ws >= c.bytes("du")
    assert c.crosses, "%s names no operand past a threshold" % c.id
    for op, th, io in c.crosses:
        assert th in (T31, T32)
        for i in ([io] if io else ios):
            assert i in ios, (c.id, op, i)
            assert c.bytes(op, i) > th, "%s: %s (%s I/O) is %d bytes, not past 2^%d" % (c.id, op, i, c.bytes(op, i), 31 if th == T31 else 32)
            # ... and by whole rows, so that there are rows past the threshold to check
            assert c.rows - -(-th // c.pitch(op, i)) >= c.T, (c.id, op)
    # 16-bit X cannot reach 2^32 bytes, Y cannot reach 2^31 bytes, at any accepted shape
    assert (T31 - 1) * 2 < T32 and ((T31 - 1) // 4) * 4 < T31
    print("%s: %s" % (c.id, ", ".join("%s %.3e B" % (op, c.bytes(op, io or ios[0])) for op, th, io in c.crosses)))


def test_elementwise_cases_cross_2_32_bytes():
    for name, e in lc.ELEMENTWISE.items():
        assert e["crosses"] and all(th == T32 and 4 * e["n"] > th for _, th in e["crosses"]), name
        assert e["n"] % lc.P not in (0, 16, 32)


# ==== 2. the limits: last accepted, first refused ==================================================================================
def _pair(lib, last, first, why):
    for d, want in ((last, True), (first, False)):
        ws = lib.wgnn_workspace_bytes(C.byref(d))
        assert (ws > 0) == want and (lib.wgnn_stash_bytes(C.byref(d)) > 0) == want, (why, want)
        assert _fwd_rc(lib, d) == (ERR_WORKSPACE if want else ERR_SHAPE), (why, want)


def test_check_dims_limits_last_accepted_and_first_refused():
    lib = _lib()
    # B*T*S*13 < 2^31 (X): S = 64, one row more is refused; the same with the rows in T and with 16-bit I/O (elements, not bytes)
    n = (T31 - 1) // (64 * 13)
    assert n * 832 < T31 <= (n + 1) * 832
    _pair(lib, _dims(n, 1, 64, 1), _dims(n + 1, 1, 64, 1), "X elements, B")
    _pair(lib, _dims(1, n, 64, 1), _dims(1, n + 1, 64, 1), "X elements, T")
    _pair(lib, _dims(n, 1, 64, 31, math=1, io=2), _dims(n + 1, 1, 64, 31, math=1, io=2), "X elements, bf16")
    # B*T*4H < 2^31 (the gate records): H = 127 and the general GRU's H = 200
    for H in (127, 200):
        n = (T31 - 1) // (4 * H)
        assert n * 4 * H < T31 <= (n + 1) * 4 * H and n * 3 * 13 < T31
        _pair(lib, _dims(n, 1, 3, H), _dims(n + 1, 1, 3, H), "gate records, H = %d" % H)
        _pair(lib, _dims(n // 2, 2, 3, H, math=1), _dims(n // 2 + 1, 2, 3, H, math=1), "gate records, T = 2, f16x3")
    # 3*H*S*13 < 2^31 (W_ih): the 4096-station graph
    H = (T31 - 1) // (3 * 4096 * 13)
    assert 3 * H * 53248 < T31 <= 3 * (H + 1) * 53248
    _pair(lib, _dims(1, 1, 4096, H, csr=True), _dims(1, 1, 4096, H + 1, csr=True), "W_ih")
    # 3*H*H < 2^31 (W_hh)
    H = int((T31 / 3) ** 0.5)
    assert 3 * H * H < T31 <= 3 * (H + 1) * (H + 1)
    _pair(lib, _dims(1, 1, 1, H), _dims(1, 1, 1, H + 1), "W_hh")
    # B*T <= 2^30 can never be the binding limit: 13 * 2^30 elements of X are past 2^31 at S = 1 already
    assert 13 * ((1 << 30) + 1) >= T31
    d = _dims((1 << 30) + 1, 1, 1, 1)
    assert lib.wgnn_workspace_bytes(C.byref(d)) == 0 and _fwd_rc(lib, d) == ERR_SHAPE


def test_series_plan_limit_last_accepted_and_first_refused():
    """rows * Gp < 2^31 (32-bit row offsets into GI_s, csrc/api.hip series_plan): binding where Gp = 32 ceil(3H / 32) exceeds
    4H, e.g. H = 11 (Gp = 64 > 44); at H = 127 (Gp = 384 < 508) check_dims' rows * 4H comes first."""
    from windgnn_amd import _lib as L
    lib = _lib()

    def sd(rows, H, stride=4, n=1000, T=2, S=3):
        return L.SeriesDims(rows, T, stride, n, S, 13, H, 0, 0, 0, 0)

    def accepted(d):
        a = lib.wgnn_series_workspace_bytes(C.byref(d)) > 0
        assert (lib.wgnn_series_stash_bytes(C.byref(d)) > 0) == a
        ps = _fake_params()
        p = [C.c_void_p((i + 1) << 40) for i in range(5)]
        rc = lib.wgnn_series_fwd(C.byref(d), p[0], p[1], C.byref(ps), p[2], p[3], p[4], C.c_size_t(0), None)
        assert rc == (ERR_WORKSPACE if a else ERR_SHAPE), rc
        return a

    rows = (T31 - 1) // 64
    assert rows * 64 < T31 <= (rows + 1) * 64 and (rows + 1) * 4 * 11 < T31 and (rows + 1) * 3 * 13 < T31
    assert accepted(sd(rows, 11)) and not accepted(sd(rows + 1, 11))
    rows = (T31 - 1) // (4 * 127)
    assert (rows + 1) * 384 < T31
    assert accepted(sd(rows, 127)) and not accepted(sd(rows + 1, 127))


# ==== 3. the inputs can show a wrap ================================================================================================
def _wrapped(c, op, io, th):
    """Rows i of the operand whose byte offset i * pitch is past th, the row j and the byte within it where that offset lands
    when reduced mod th, and whether that differs visibly: mid-row, or another phase (window in period, step)."""
    q = c.pitch(op, io)
    i = np.arange(-(-th // q), c.rows, dtype=np.int64)
    w = (i * q) % th
    j, mid = w // q, (w % q) != 0
    other = ((i // c.T) % lc.P != (j // c.T) % lc.P) | (i % c.T != j % c.T)
    return i, j, w, mid | other


@pytest.mark.parametrize("c", lc.STEPS, ids=[c.id for c in lc.STEPS])
def test_a_wrapped_offset_lands_mid_row_or_on_another_phase(c):
    ios = sorted({io for _, io, _ in c.runs})
    for op, th, io in c.crosses:
        for i_o in ([io] if io else ios):
            for t in ((T31, T32) if th == T32 else (T31,)):          # past 2^32 an offset can lose bit 31 or bit 32
                i, j, w, shows = _wrapped(c, op, i_o, t)
                assert len(i) >= c.T
                print("%s %s (%s) mod 2^%d: %d rows past it, %.2f %% land visibly elsewhere"
                      % (c.id, op, i_o, 31 if t == T31 else 32, len(i), 100.0 * shows.mean()))
                assert shows.mean() >= 0.99, (c.id, op, i_o, t)


def _min_pair_distance(rows):
    """min over pairs of distinct rows of max |row_a - row_b|."""
    rows = rows.reshape(-1, rows.shape[-1]).double()
    n, best = rows.shape[0], float("inf")
    blk = max(1, min(64, (1 << 26) // max(1, n * rows.shape[1])))
    for a in range(0, n, blk):
        dd = (rows[a:a + blk, None, :] - rows[None, :, :]).abs().amax(-1)
        k = torch.arange(a, min(a + blk, n))
        dd[k - a, k] = float("inf")
        best = min(best, float(dd.min()))
    return best


def _operand_rows(c, op, io):
    """The operand's own rows [48, T, .] on the fp64 oracle."""
    import lattice_inputs as li
    d, ref = lc.base_draw(c.id), lc.step_reference(c.id, io)
    if op == "X":
        return d.X.to(lc.IO_DTYPE[io]).double().reshape(lc.P, c.T, -1)
    if op in ("g", "g_plane"):
        return ref["g"]
    if op == "GI":
        return ref["GI"]
    if op == "h1":
        return ref["H1"].reshape(lc.P, c.T, -1)
    dg = li.dg_of_mse(ref["g"], d.p, d.L.to(lc.IO_DTYPE[io]))
    if op == "dg":
        return dg
    assert op == "du"           # csr_layer_bwd_kernel<true>: DU = dZ2 W2^T, dZ2 = dg (g > 0)
    dz2 = (dg * (ref["g"] > 0)).reshape(lc.P, c.T, c.S, 13)
    return torch.matmul(dz2, d.p["conv2.weight"].double().t()).reshape(lc.P, c.T, -1)


@pytest.mark.parametrize("c", lc.STEPS, ids=[c.id for c in lc.STEPS])
def test_distinct_phases_differ_by_ten_bars_on_the_oracle(c):
    ios = sorted({io for _, io, _ in c.runs})
    for io in ios:
        bar = _case_bar(c, io)
        dy = _min_pair_distance(lc.step_reference(c.id, io)["Y"])
        print("%s (%s): bar %.1e, closest two phases of Y %.3e" % (c.id, io, bar, dy))
        assert dy > 10 * bar, (c.id, io, dy)
    for op, th, io in c.crosses:
        for i_o in ([io] if io else ios):
            rows = _operand_rows(c, op, i_o)
            scale = float(rows.abs().max())
            dr = _min_pair_distance(rows)
            print("%s %s (%s): closest two phases %.3e (max |row| %.3e)" % (c.id, op, i_o, dr, scale))
            # gradients (dg, du) are small numbers: their rows are held to 10 bars of their own scale
            assert dr > 10 * _case_bar(c, i_o) * (scale if op in ("dg", "du") else 1.0), (c.id, op, i_o, dr)


def test_the_oracles_own_fp32_error_is_a_tenth_of_the_bar():
    """The reference's own error: the fp32 oracle against the fp64 one on each case's period."""
    from oracle import windgnn_oracle as orc
    for c in lc.STEPS:
        d = lc.base_draw(c.id)
        Y32, _ = orc.forward(d.A, d.X, d.p, want_cache=False)
        e = float((Y32.double() - lc.step_reference(c.id)["Y"]).abs().max())
        print("%s: fp32 oracle vs fp64 %.2e" % (c.id, e))
        assert e <= 0.1 * Y_TOL, (c.id, e)


def _gru_from_gi(GI, p):
    """Y [T, H] of one window from its input projection GI [T, 3H] (oracle.forward's recurrence, fp64, h0 = 0)."""
    Whh, bhh = p["gru.weight_hh_l0"].double(), p["gru.bias_hh_l0"].double()
    H = Whh.shape[1]
    h, out = torch.zeros(H, dtype=torch.float64), []
    for t in range(GI.shape[0]):
        gh = Whh @ h + bhh
        r = torch.sigmoid(GI[t, :H] + gh[:H])
        z = torch.sigmoid(GI[t, H:2 * H] + gh[H:2 * H])
        n = torch.tanh(GI[t, 2 * H:] + r * gh[2 * H:])
        h = (1.0 - z) * n + z * h
        out.append(h)
    return torch.stack(out)


def _read_wrapped(flat_rows, q_elems, width, i, th_elems):
    """What a read of `width` elements at element offset (i * q_elems) mod th_elems returns from the periodic operand whose
    period is flat_rows [48 T, q_elems] (padding columns included)."""
    e = (i * q_elems) % th_elems + np.arange(width, dtype=np.int64)
    rr, cc = (e // q_elems) % flat_rows.shape[0], e % q_elems
    return flat_rows[torch.from_numpy(rr), torch.from_numpy(cc)]


def test_planted_wraps_fail_the_comparison_by_message():
    """One wrap per family, planted into the fp64 reference of a full-size Y: the GPU module's comparison names the check."""
    from oracle import windgnn_oracle as orc
    # ---- an X read of x4g that lost bit 32 of its byte offset, and a Y store that went to the row such an offset gives
    c = lc.STEP_BY_ID["x4g"]
    d, ref = lc.base_draw(c.id), lc.step_reference(c.id)
    p64 = {k: v.double() for k, v in d.p.items()}
    Y = lc.periodic(ref["Y"].float(), c.B)
    assert lc.check_periodic(Y, ref["Y"], Y_TOL, "x4g clean") < 1e-6
    i, j, w, shows = _wrapped(c, "X", "f32", T32)
    k = int(np.flatnonzero(shows)[len(i) // 2])
    row, I = int(i[k]), c.S * 13
    b, t = row // c.T, row % c.T
    Xw = d.X[b % lc.P].double().clone()
    Xw[t] = _read_wrapped(d.X.double().reshape(lc.P * c.T, I), I, I, row, T32 // 4).reshape(c.S, 13)
    Yw, _ = orc.forward(d.A.double(), Xw[None], p64, want_cache=False)
    assert float((Yw[0] - ref["Y"][b % lc.P]).abs().max()) > 10 * Y_TOL
    keep = Y[b].clone()
    Y[b] = Yw[0].float()
    with pytest.raises(AssertionError, match=r"check 3 \(period\): window %d " % b):
        lc.check_periodic(Y, ref["Y"], Y_TOL, "x4g planted X read")
    Y[b] = keep
    jb, jt = int(j[k]) // c.T, int(j[k]) % c.T
    keep_j = Y[jb, jt].clone()
    Y[b, t] = float("nan")
    Y[jb, jt] = ref["Y"][b % lc.P, t].float()
    with pytest.raises(AssertionError, match=r"check 1 \(NaN prefill\): window %d " % b):
        lc.check_periodic(Y, ref["Y"], Y_TOL, "x4g planted Y store")
    Y[b], Y[jb, jt] = keep, keep_j
    Y[jb, jt] = ref["Y"][b % lc.P, t].float()                   # the stray store alone: the overwritten row shows
    with pytest.raises(AssertionError, match=r"check 3 \(period\)"):
        lc.check_periodic(Y, ref["Y"], Y_TOL, "x4g planted stray store")
    del Y
    # ---- a GI read of gi4g that lost bit 32
    c = lc.STEP_BY_ID["gi4g"]
    d, ref = lc.base_draw(c.id), lc.step_reference(c.id)
    Gp, G3 = c.pitch("GI") // 4, 3 * c.H
    i, j, w, shows = _wrapped(c, "GI", "f32", T32)
    row = int(i[int(np.flatnonzero(shows)[len(i) // 2])])
    b, t = row // c.T, row % c.T
    rows = torch.zeros(lc.P * c.T, Gp, dtype=torch.float64)
    rows[:, :G3] = ref["GI"].reshape(lc.P * c.T, G3)
    GIw = ref["GI"][b % lc.P].clone()
    GIw[t] = _read_wrapped(rows, Gp, G3, row, T32 // 4)
    Yw = _gru_from_gi(GIw, d.p)
    assert float((_gru_from_gi(ref["GI"][b % lc.P], d.p) - ref["Y"][b % lc.P]).abs().max()) < 1e-12
    assert float((Yw - ref["Y"][b % lc.P]).abs().max()) > 10 * Y_TOL
    # (the comparison itself at gi4g's 1.4 M windows is the GPU module's; here on the last 4800 + r windows, phases kept)
    n = 100 * lc.P + c.r
    Y = lc.periodic(ref["Y"].float(), n)
    Y[b - (c.B - n)] = Yw.float()
    assert (c.B - n) % lc.P == 0 and b >= c.B - n
    with pytest.raises(AssertionError, match=r"check 3 \(period\)"):
        lc.check_periodic(Y, ref["Y"], Y_TOL, "gi4g planted GI read")


# ==== 4. ragged batches ============================================================================================================
def test_every_batch_has_a_ragged_last_period_and_a_partial_last_workgroup():
    for c in lc.STEPS:
        assert c.B == lc.P * c.R + c.r and c.r in lc.RAGGED and c.r not in (0, 16, 32) and c.B % 16 != 0, c.id


# ==== layers and the element-wise entries ==========================================================================================
LAYER_FWD = ("A", "X", "W", "b", "out")


def _layer_fwd_rc(lib, c, nt, null="out"):
    """wgnn_gcn_layer_fwd / _csr_fwd with one NULL pointer: a refused shape is WGNN_ERR_SHAPE (checked first), an accepted one
    gets as far as the NULL check; nothing is launched."""
    p = [C.c_void_p(0 if n == null else (i + 1) << 40) for i, n in enumerate(LAYER_FWD)]
    if c.csr_k:
        return lib.wgnn_gcn_layer_csr_fwd(nt, c.S, c.Fi, 8 * c.S, *p, None)
    return lib.wgnn_gcn_layer_fwd(nt, c.S, c.Fi, c.Fo, *p, None)


def _layer_ws(lib, c, nt):
    return lib.wgnn_gcn_layer_csr_workspace_bytes(nt, c.S, c.Fi) if c.csr_k else lib.wgnn_gcn_layer_workspace_bytes(nt, c.S, c.Fi, c.Fo)


@pytest.mark.parametrize("c", lc.LAYERS, ids=[c.id for c in lc.LAYERS])
def test_every_layer_case_is_accepted_crosses_2_32_and_shows_a_wrap(c):
    lib = _lib()
    assert _layer_ws(lib, c, c.nt) > 0 and _layer_fwd_rc(lib, c, c.nt) == ERR_NULL
    assert c.nt == lc.P * c.R + c.r and c.r in lc.RAGGED and c.crosses
    if c.csr_k or max(c.Fi, c.Fo) > 64:
        assert c.nt * c.S * max(c.Fi, c.Fo) < T31              # the documented element limit of these two routes
    for op, th in c.crosses:
        assert c.bytes(op) > th, (c.id, op, c.bytes(op))
        for t in (T31, T32):
            i, j, w, shows = _wrapped(c, op, "f32", t)
            print("%s %s mod 2^%d: %d tiles past it, %.2f %% land visibly elsewhere"
                  % (c.id, op, 31 if t == T31 else 32, len(i), 100.0 * shows.mean()))
            assert len(i) >= 1 and shows.mean() >= 0.99, (c.id, op, t)


@pytest.mark.parametrize("c", lc.LAYERS, ids=[c.id for c in lc.LAYERS])
def test_distinct_layer_tiles_differ_by_ten_bars_on_the_reference(c):
    d, ref = lc.layer_draw(c.id), lc.layer_reference(c.id)
    for op, rows in (("X", d.X), ("dout", d.dout), ("out", ref["out"]), ("dX", ref["dX"])):
        rows = rows.reshape(lc.P, 1, -1)
        scale = float(rows.abs().max())
        dr = _min_pair_distance(rows)
        print("%s %s: closest two tiles %.3e (max %.3e)" % (c.id, op, dr, scale))
        assert dr > 10 * LAYER_TOL * max(1.0, scale), (c.id, op, dr)     # relative to the tensor's max for dX, as its bar is


def test_layer_limits_last_accepted_and_first_refused():
    """Every width: ntiles <= 2^31 - 4097 (the 32-bit tile counters of gcn.hip / gcn_any.hip run up to 4096 past the last tile).
    CSR: ntiles * S * 13 < 2^31.  Wider than 64: tests/test_layer_wide_host.py::test_an_element_count_of_two_to_the_31_is_a_shape_error."""
    lib = _lib()
    last = (1 << 31) - 1 - 4096
    for S, Fi, Fo in ((1, 1, 1), (3, 13, 13), (64, 64, 64), (5, 7, 64)):
        c = lc.Layer("limit", last, S, Fi, Fo, "", [])
        assert _layer_ws(lib, c, last) > 0 and _layer_fwd_rc(lib, c, last) == ERR_NULL, (S, Fi, Fo)
        assert _layer_ws(lib, c, last + 1) == 0 and _layer_fwd_rc(lib, c, last + 1) == ERR_SHAPE, (S, Fi, Fo)
    c = lc.LAYER_BY_ID["l_csr"]
    last = (T31 - 1) // (c.S * 13)
    assert last * c.S * 13 < T31 <= (last + 1) * c.S * 13
    assert _layer_ws(lib, c, last) > 0 and _layer_fwd_rc(lib, c, last) == ERR_NULL
    assert _layer_ws(lib, c, last + 1) == 0 and _layer_fwd_rc(lib, c, last + 1) == ERR_SHAPE


def test_predict_last_limit_last_accepted_and_first_refused():
    """out [B][H] below 2^31 elements; Y itself may be of any size.  2^31 - 1 elements are accepted: the block count is formed
    in 64 bits (B * H + 255 does not fit an int from 2^31 - 255 on) and the last thread's index, at most 2^31 - 1, fits the
    kernel's int -- held to the source here, and run at 2^31 - 8 elements by tests/test_gpu_large_offset.py."""
    import os
    import re
    from conftest import ROOT
    lib = _lib()

    def rc(B, H, null_out):
        return lib.wgnn_predict_last(C.c_void_p(1 << 40), B, 6, H, 0.0, 1.0, C.c_void_p(0 if null_out else 2 << 40), None)

    for B, H in (((1 << 31) - 1, 1), ((1 << 30) - 1, 2), ((T31 - 1) // 127, 127)):          # the last accepted ...
        assert T31 - 256 < B * H < T31 and rc(B, H, True) == ERR_NULL, (B, H)
    for B, H in ((1 << 30, 2), (1 << 24, 128), ((T31 - 1) // 127 + 1, 127)):                # ... and the first refused
        assert B * H >= T31 and rc(B, H, True) == ERR_SHAPE and rc(B, H, False) == ERR_SHAPE, (B, H)
    src = open(os.path.join(ROOT, "windgnn_amd", "csrc", "data_ops.hip")).read()
    entry = src[src.index("int wgnn_predict_last("):]
    assert re.search(r"dim3\(\(unsigned\)\(\(\(int64_t\)B \* H \+ 255\) / 256\)\)", entry) and "cdiv_i" not in entry
    kern = src[src.index("void predict_last_kernel("):src.index("}  // namespace")]
    assert "const int i = blockIdx.x * blockDim.x + threadIdx.x;" in kern and "if (i >= B * H) return;" in kern
    assert ((T31 - 1 + 255) // 256 - 1) * 256 + 255 <= T31 - 1                               # the last thread of the last block
    e = lc.PREDICT_LAST_EDGE
    assert T31 - 256 < e["B"] * e["H"] < T31 and e["B"] % lc.P not in (0, 16, 32)
    B, T, H = (lc.PREDICT_LAST[k] for k in "BTH")
    assert B * T * H * 4 > T32 and B * H < T31 and B % lc.P not in (0, 16, 32)
    m = lc.MAKE_WINDOWS
    assert m["B"] * m["seq"] * m["S"] * 13 * 4 > T32 and m["Ttot"] >= m["B"] * m["seq"] + 3


# ==== series mode ==================================================================================================================
@pytest.mark.parametrize("c", lc.SERIES, ids=[c.id for c in lc.SERIES])
def test_every_series_case_is_accepted_crosses_2_32_and_shows_a_wrap(c):
    lib = _lib()
    for table in ((False, True) if c.n_table else (False,)):
        sd, q = c.sdims(table), "at_" if table else ""
        assert getattr(lib, "wgnn_series_%sworkspace_bytes" % q)(C.byref(sd)) > 0
        st = getattr(lib, "wgnn_series_%sstash_bytes" % q)(C.byref(sd))
        assert st >= c.bytes("GI_s") + c.bytes("g_s") and lib.wgnn_series_val_workspace_bytes(C.byref(sd)) > 0
    assert (c.n - 1) * c.stride + c.T <= c.rows and c.rows * c.pitch("GI_s") // 4 < T31 and c.n % c.period != 0 and c.crosses
    for op, th in c.crosses:
        assert c.bytes(op) > th
        q = c.pitch(op)
        for t in (T31, T32):
            i = np.arange(-(-t // q), c.rows, dtype=np.int64)
            wr = (i * q) % t
            shows = ((wr % q) != 0) | ((wr // q) % lc.Q != i % lc.Q)
            print("%s %s mod 2^%d: %d hours past it, %.2f %% land visibly elsewhere" % (c.id, op, 31 if t == T31 else 32, len(i), 100.0 * shows.mean()))
            assert len(i) >= c.T and shows.mean() >= 0.99
    if c.n_table:
        t = c.table()
        assert len(t) == c.n_table and bool((t[1:] >= t[:-1]).all()) and int(t[0]) == 0 and int(t[-1]) == c.rows - c.T
        assert set(c.crossing_rows()) <= set(t.tolist()) and len(c.crossing_rows()) == 6 and c.n_table % 16 != 0
        assert len(set((t.long() % lc.Q).tolist())) == lc.Q                       # every phase occurs


@pytest.mark.parametrize("c", lc.SERIES, ids=[c.id for c in lc.SERIES])
def test_distinct_series_phases_differ_by_ten_bars_on_the_oracle(c):
    from oracle import windgnn_oracle as orc
    d, w = lc.series_draw(c.id), lc.series_windows(c.id)
    order = (torch.arange(c.period) * c.stride) % lc.Q
    dy = _min_pair_distance(w["Y"][order])
    Y32, _ = orc.forward(d.A, w["X"].float(), d.p, want_cache=False)
    e32 = float((Y32.double() - w["Y"]).abs().max())
    print("%s: closest two windows of Y %.3e, fp32 oracle vs fp64 %.2e" % (c.id, dy, e32))
    assert dy > 10 * Y_TOL and e32 <= 0.1 * Y_TOL
    hours = {"Xs": d.Xs.double().reshape(lc.Q, -1), "g_s": w["cache"]["g"][:, 0], "GI_s": w["cache"]["GI"][:, 0]}
    for op, th in c.crosses:
        dr = _min_pair_distance(hours[op].reshape(lc.Q, 1, -1))
        print("%s %s: closest two hours %.3e" % (c.id, op, dr))
        assert dr > 10 * Y_TOL
