"""The dense graph-convolution kernels' tile loops, checked without a GPU: tests/gcn_loop_cases.py's restatement of the launch
geometry against the text of csrc/gcnx.hip, gcn32.hip and gcngi.hip (and gcn.hip / gcn_any.hip for the one-layer cases) and
against instance_cases.plan(); the exact blind-spot table -- the most trips any tabled launch gives each instance key, anywhere
and on the lattice draw; GCN_LOOP_CASES re-derived by rule; and the inputs of tests/test_gpu_gcn_loops.py qualified on the fp64
oracle alone: invariants (a) to (f) of tests/test_lattice_inputs_host.py, and a restated fp64 step that walks the rows in trips of
one grid stride, equals lattice_inputs.fp64_step bit for bit and into which the mistakes a loop's later trip can make are
planted: each must move Y or a gradient by more than 10 x 1e-4.  A failure of a GPU case on these inputs is therefore a finding
about the kernel."""
import re

import pytest
import torch

import gcn_loop_cases as gl
import instance_cases as ic
import lattice_inputs as li
import test_instance_table_host as tith
import test_lattice_inputs_host as tli
from conftest import PARAM_KEYS, max_abs, rel_to_max
from test_gpu_parity import F16_G_TOL, F16_Y_TOL, G_TOL, Y_TOL

BAR = 1e-4                                          # the fp32-grade bar (Y_TOL, G_TOL); a planted mistake must exceed gl.PLANT_FACTOR x it
assert BAR == Y_TOL == G_TOL


# ==== A. the geometry ============================================================================================================
def test_gcn_trips_restates_the_sources():
    gcnx, gcn32, gcngi = (tith._read(n + ".hip") for n in ("gcnx", "gcn32", "gcngi"))
    const = lambda name, src: tith._ints(r"constexpr int %s = (\d+);" % name, src, name)
    assert const("FWD_WAVES", gcnx) == [gl.FWD_WAVES] and const("FWD_WAVES", gcn32) == [gl.FWD_WAVES]
    assert const("WGNN_BWD4_WAVES", gcnx) == [gl.BWD4_WAVES]
    # gcnx.hip bwd_waves: one return, (one-pass, NT <= 3, 16-bit dg) ? 16 : (NT >= 4 ? WGNN_BWD4_WAVES : 12)
    bw = re.search(r"return \(!X3 && NT <= (\d+) && DG16\) \? (\d+) : \(NT >= (\d+) \? WGNN_BWD4_WAVES : (\d+)\);", gcnx)
    assert bw, "gcnx.hip bwd_waves no longer reads as restated"
    assert [int(x) for x in bw.groups()] == [3, gl.BWD_WAVES_ONE_PASS, 4, gl.BWD_WAVES]
    grid_x = tith._body(gcnx, "int grid_x(int ntiles, int S, bool x3) {")
    assert "int g = cdiv_i(ntiles, bwd_waves((S + 15) / 16, x3));" in grid_x                 # DG16 defaulted: see gcnx_bwd_grid
    assert tith._ints(r"const int cap = (\d+);", grid_x, "grid_x's cap") == [gl.BWD_GRID_CAP]
    assert "return g < 1 ? 1 : (g > cap ? cap : g);" in grid_x
    assert "constexpr int bwd_waves(int NT, bool X3, bool DG16 = true) {" in gcnx
    for src, name in ((gcnx, "gcnx.hip"), (gcn32, "gcn32.hip")):
        assert "int gx = cdiv_i(ntiles, FWD_WAVES);" in src, name
        assert tith._ints(r"gx = gx < 1 \? 1 : \(gx > (\d+) \? \1 : gx\);", src, name + " forward cap") == [gl.FWD_GRID_CAP]
        assert src.count("for (int tile = wave_id; tile < ntiles; tile += nwaves) {") == 2, name
        assert src.count("const int nwaves = (gridDim.x * blockDim.x) >> 6;") == 2, name
        assert src.count("const int wave_id = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;") == 2, name
        assert "const bool more = tile + nwaves < ntiles;" in src and "XLOAD(tile + nwaves);" in src, name
        assert "if (tile + nwaves < ntiles) {" in src, name                                   # the backward's prefetch
    # the private copy of the last tile: XLOAD of gcn32.hip, and of gcnx_dev.h for gcnx.hip and gcngi.hip
    assert "(xtail != nullptr && (t) == ntiles - 1) ? xtail : X + (size_t)(t) * I" in gcn32
    assert "const bool tl_ = xtail != nullptr && (t) == ntiles - 1;" in tith._read("gcnx_dev.h")
    for src, odd in ((gcnx, "if ((I & 1) == 0) return nullptr;"), (gcn32, "if ((I & 1) == 0) return WGNN_OK;"), (gcngi, "if (I & 1) {")):
        assert "(size_t)(ntiles - 1) * I" in src and odd in src, odd                            # copied for odd S * 13 only
    assert "const dim3 grid(grid_x(ntiles, S, x3));" in gcnx and "dim3(64 * bwd_waves(NT, X3V, D16))" in gcnx
    assert "dim3(64 * FWD_WAVES)" in gcnx and "dim3(64 * FWD_WAVES)" in gcn32
    # gcn32.hip: bwd_waves_of and bwd_grid
    w = re.search(r"int bwd_waves_of\(int S, int ntiles\) \{ return \(S <= (\d+) && ntiles >= (\d+)\) \? (\d+) : (\d+); \}", gcn32)
    assert w, "gcn32.hip bwd_waves_of no longer reads as restated"
    assert [int(x) for x in w.groups()] == [gl.G32_W16_SMAX, gl.G32_W16_ROWS, 16, gl.BWD_WAVES]
    assert "int gx = cdiv_i(ntiles, bwd_waves_of(S, ntiles));" in gcn32
    assert tith._ints(r"return gx < 1 \? 1 : \(gx > (\d+) \? \1 : gx\);", gcn32, "bwd_grid's cap") == [gl.BWD_GRID_CAP]
    assert "const int gx = bwd_grid(ntiles, S);" in gcn32 and "const bool w16 = bwd_waves_of(S, ntiles) == 16;" in gcn32
    assert "dim3(gx), dim3(64 * W)" in gcn32
    # gcngi.hip: gg_cfg and the grid
    cfg = re.search(r"static GgCfg gg_cfg\(bool x3\) \{ return x3 \? GgCfg\{(\d+), (\d+), (\d+)\} : GgCfg\{(\d+), (\d+), (\d+)\}; \}", gcngi)
    assert cfg, "gcngi.hip gg_cfg no longer reads as restated"
    assert (int(cfg.group(3)), int(cfg.group(6))) == (gl.GI_ROWS[True], gl.GI_ROWS[False])
    assert "const int ntile_r = cdiv_i(ntiles, R);" in gcngi
    assert tith._ints(r"const int grid = ntile_r < (\d+) \? ntile_r : \1;", gcngi, "gcngi's grid cap") == [gl.GI_GRID_CAP]
    for line in ("const int nit = (int)blockIdx.x < ntile_r ? (ntile_r - 1 - (int)blockIdx.x) / (int)gridDim.x + 1 : 0;",
                 "for (int it = 0; it < nit; ++it) {", "const char* buf = gt + (it & 1) * buf_b;",
                 "const int m0 = ((int)blockIdx.x + it * (int)gridDim.x) * R;",
                 "return ((int)blockIdx.x + tp * (int)gridDim.x) * R + r;"):
        assert line in gcngi, "gcngi.hip no longer has %r" % line
    for R, ng, nm in ((32, 8, 8), (48, 12, 4)):
        assert re.search(r"GG_GO\(NT, (?:true|false), (?:true|false), %d, %d, %d," % (ng, nm, R), gcngi), R
    # the one-layer kernels
    gcn1, gany = tith._read("gcn.hip"), tith._read("gcn_any.hip")
    assert const("WAVES", gcn1) == [gl.GCN1_WAVES]
    grid_for = tith._body(gcn1, "int grid_for(int ntiles) {")
    assert "int g = cdiv_i(ntiles, WAVES);" in grid_for
    assert tith._ints(r"return g < 1 \? 1 : \(g > (\d+) \? \1 : g\);", grid_for, "grid_for's cap") == [gl.GCN1_GRID_CAP]
    assert gcn1.count("for (int base = blockIdx.x * WAVES; base < ntiles; base += gridDim.x * WAVES) {") == 2
    assert tith._ints(r"int ga_grid\(int ntiles\) \{ return ntiles < (\d+) \? ntiles : \1; \}", gany, "ga_grid") == [gl.GA_GRID_CAP]
    assert gany.count("for (int t = blockIdx.x; t < ntiles; t += gridDim.x) {") == 2


def _walk(n, tiles):
    """The loop itself: the trips of every wave (block) and the trip on which the last tile is met."""
    trips = [len(range(u, tiles, n)) for u in range(n)]
    last = next(i + 1 for u in range(n) for i, t in enumerate(range(u, tiles, n)) if t == tiles - 1)
    return max(trips), trips.count(max(trips)), last


def test_gcn_trips_counts_what_the_loops_do():
    """The figures of the issue's table, the thresholds one row either side, and a brute-force walk of the loop."""
    t = gl.gcn_trips
    assert t("gcnx_fwd_kernel<1>|io=32", 5, 4096)[:2] == (4096, 1) and t("gcnx_fwd_kernel<1>|io=32", 5, 4097) == (4096, 2, 1, 2)
    assert t("gcn32_fwd_kernel<4>", 49, 4096)[1] == 1 and t("gcn32_fwd_kernel<4>", 49, 4097)[1] == 2
    assert t("gcnx_bwd_kernel<2>|io=32|dg16=0", 17, 3072)[:2] == (3072, 1) and t("gcnx_bwd_kernel<2>|io=32|dg16=0", 17, 3073)[1] == 2
    assert t("gcnx_bwd_kernel<3,f16>|io=32|dg16=1", 33, 4096)[:2] == (4096, 1) and t("gcnx_bwd_kernel<3,f16>|io=32|dg16=1", 33, 4097)[1] == 2
    assert t("gcnx_bwd_kernel<4>|io=32|dg16=0", 49, 2048)[:2] == (2048, 1) and t("gcnx_bwd_kernel<4,f16>|io=32|dg16=1", 49, 2049)[1] == 2
    # one-pass with an fp32 dg: blocks of 12 waves on a grid counted for 16
    assert t("gcnx_bwd_kernel<1,f16>|io=32|dg16=0", 5, 34) == (36, 1, 34, 1) and t("gcnx_bwd_kernel<1,f16>|io=32|dg16=0", 5, 16) == (12, 2, 4, 2)
    assert t("gcnx_bwd_kernel<1,f16>|io=32|dg16=0", 5, 8198) == (3072, 3, 2054, 3)
    assert t("gcn32_bwd_kernel<1>|w=12", 5, 3072)[:2] == (3072, 1) and t("gcn32_bwd_kernel<1>|w=12", 5, 3073)[1] == 2
    assert t("gcn32_bwd_kernel<1>|w=12", 5, 16383) == (3072, 6, 1023, 6) and t("gcn32_bwd_kernel<1>|w=16", 5, 16384) == (4096, 4, 4096, 4)
    assert t("gcn32_bwd_kernel<4>|w=12", 49, 16384)[0] == 3072                       # S > 48 never takes the 16-wave form
    with pytest.raises(AssertionError):
        t("gcn32_bwd_kernel<1>|w=16", 5, 16383)
    assert t("gcngi_fwd_kernel<1>|io=32|planes=2", 5, 8192) == (256, 1, 256, 1) and t("gcngi_fwd_kernel<1>|io=32|planes=2", 5, 8193) == (256, 2, 1, 2)
    assert t("gcngi_fwd_kernel<1,f16>|io=32|planes=1", 5, 12288)[1] == 1 and t("gcngi_fwd_kernel<1,f16>|io=32|planes=1", 5, 12289)[1] == 2
    # the rule's row counts
    assert t("gcnx_fwd_kernel<1>|io=32", 5, 8198) == (4096, 3, 6, 3) and t("gcnx_bwd_kernel<1>|io=32|dg16=0", 5, 8198) == (3072, 3, 2054, 3)
    assert t("gcnx_bwd_kernel<4>|io=32|dg16=0", 49, 8198) == (2048, 5, 6, 5) and t("gcnx_bwd_kernel<1,f16>|io=32|dg16=1", 5, 8198) == (4096, 3, 6, 3)
    assert t("gcngi_fwd_kernel<3>|io=32|planes=2", 33, 16386) == (256, 3, 1, 3) and 16386 - 512 * 32 == 2
    assert t("gcngi_fwd_kernel<3,f16>|io=32|planes=1", 33, 24578) == (256, 3, 1, 3) and 24578 - 512 * 48 == 2
    for key, S in (("gcnx_fwd_kernel<1>|io=32", 5), ("gcnx_bwd_kernel<2>|io=32|dg16=0", 17), ("gcnx_bwd_kernel<2,f16>|io=32|dg16=1", 17),
                   ("gcnx_bwd_kernel<2,f16>|io=32|dg16=0", 17), ("gcnx_bwd_kernel<4>|io=16|dg16=1", 49), ("gcn32_bwd_kernel<3>", 33),
                   ("gcngi_fwd_kernel<2>|io=16|planes=0", 17), ("gcngi_fwd_kernel<2,f16>|io=16|planes=0", 17)):
        for rows in (1, 7, 34, 2047, 2049, 3073, 4097, 4098, 8198, 12289, 16383, 16384, 16386, 24578):
            kind, n, tiles = gl.gcn_geometry(key, S, rows)
            assert gl.gcn_trips(key, S, rows) == (n,) + _walk(n, tiles), (key, rows)
    assert gl.layer_trips(13, 13, 5) == (8, 1, 5) and gl.layer_trips(13, 13, 8195) == (4096, 3, 3) and gl.layer_trips(6, 9, 2051) == (1024, 3, 3)


def test_gcn_launches_follow_plan_over_every_table_and_around_each_threshold():
    """gcn_launches() names exactly plan()'s keys of the five families, and gcn32_bwd's key agrees with the rows' wave count."""
    for name, table in gl.window_tables() + (("GCN_LOOP_CASES", gl.ALL_LOOP_CASES),):
        for c in table:
            got = gl.gcn_launches(c)
            assert [g[0] for g in got] == [k for k in ic.plan(*c[2:10]) if ic.family_of(k) in gl.GCN_FAMILIES], (name, c)
            assert all(g[2] >= 1 and 1 <= g[3] <= g[1] and g[4] == g[2] for g in got), (name, c, got)
    for rows in (2047, 2048, 2049, 3071, 3072, 3073, 4095, 4096, 4097, 8191, 8192, 8193, 12287, 12288, 12289, 16383, 16384, 16385):
        for S in (5, 17, 33, 48, 49, 64):
            for H in (4, 128):
                for mth, io, route in (("f32", "f32", "train"), ("f16x3", "f32", "train"), ("f16x3", "bf16", "fused"), ("f16", "f32", "train"),
                                       ("f16", "bf16", "infer"), ("f16x3g", "f32", "fused"), ("f16x3g", "f16", "train")):
                    if ic.refusal(S, 1, rows, H, mth, io) is None:
                        assert gl.gcn_launches((None, None, S, 1, rows, H, mth, io, False, route)), (S, rows, H, mth)


# ==== B. the blind spot and the table ==============================================================================================
def test_the_blind_spot_table():
    """The most trips any tabled launch gives each key of the five families, anywhere and on the lattice draw, printed; the old
    blind spot asserted once."""
    anywhere, lattice = gl.most_trips(), gl.most_trips(gl.window_tables()[-1:])
    assert len(anywhere) == 16 + 28 + 30 + 4 + 7
    for k in anywhere:
        a, l = anywhere[k], lattice[k]
        print("%-44s most trips %2d (%s, S T B H = %s; %3d launches)   on the lattice draw %d%s"
              % (k, a[0], a[1], a[2], a[3], l[0], "" if k in gl.GCN_LOOP_ALREADY else "   -> a case"))
    # what the launchers and the tables say, against the issue's reading of them
    assert {k: lattice[k][0] for k in lattice if lattice[k][0] >= gl.LOOP_TRIPS} == {k: v[0] for k, v in gl.GCN_LOOP_ALREADY.items()}
    assert sorted(gl.GCN_LOOP_ALREADY) == sorted(["gcn32_bwd_kernel<%d>|w=16" % n for n in (1, 2, 3)] + ["gcn32_fwd_kernel<%d>" % n for n in (1, 2, 3)])
    assert all(v[0] == 4 and v[2][1] * v[2][2] == 16384 for v in gl.GCN_LOOP_ALREADY.values())
    # the issue's example holds for the io=16 twin, not for io=32: by-product launches of the 36 888-row GEMM cases reach 13 trips
    assert anywhere["gcnx_bwd_kernel<2>|io=16|dg16=0"][0] == 1 and anywhere["gcnx_bwd_kernel<2>|io=32|dg16=0"][:3] == (13, "CASES", (18, 24, 1537, 4))
    assert sum(1 for v in anywhere.values() if v[0] >= gl.LOOP_TRIPS) == 34
    # every gcngi key and every 16-bit-I/O key: at most two trips anywhere, except <4>|io=16|dg16=1 (three at 4098 rows on 2048 waves)
    assert max(v[0] for k, v in anywhere.items() if k.startswith("gcngi")) == 1
    assert {k: v[0] for k, v in anywhere.items() if "io=16" in k and v[0] > 2} == {"gcnx_bwd_kernel<4>|io=16|dg16=1": 3}
    # on the lattice draw: no w=12 backward and no gcnx / gcngi instance ran more than two trips
    assert max(v[0] for k, v in lattice.items() if "w=16" not in k and not k.startswith("gcn32_fwd")) == 2
    # the keyed launch of every key's own CASES entry, the 4098- and 16 419-row ones aside, makes ONE trip
    for c in ic.CASES:
        if c[0] in gl.GCN_FAMILIES and c[3] * c[4] == 34:
            assert [g[2] for g in gl.gcn_launches(c) if g[0] == c[1]] == [1], c


def gcn_loop_problems(cases, even=gl.GCN_LOOP_EVEN_CASES, already=gl.GCN_LOOP_ALREADY, impossible=gl.GCN_LOOP_IMPOSSIBLE):
    """What is wrong with `cases` as gl.GCN_LOOP_CASES (and `even` as the even-I cases): a list of sentences, empty when every key
    of the five families outside `already` is claimed once, on its key, at the rule's dims, with an odd count of at least three
    trips of the keyed launch, the last tile on the final trip and some wave making a trip fewer."""
    bad = []
    lattice = gl.most_trips(gl.window_tables()[-1:])
    need = [k for k in lattice if lattice[k][0] < gl.LOOP_TRIPS]
    bad += ["%s is listed as already at %d trips; the lattice tables give it %d" % (k, already[k][0], lattice[k][0])
            for k in already if k not in lattice or lattice[k][0] < gl.LOOP_TRIPS]
    claimed = [c[1] for c in cases]
    bad += ["%s is claimed %d times" % (k, claimed.count(k)) for k in dict.fromkeys(claimed) if claimed.count(k) > 1]
    for k in need:
        if k not in claimed and k not in impossible:
            bad.append("%s makes at most %d trips on the lattice draw and has no case" % (k, lattice[k][0]))
    for c in list(cases) + list(even):
        fam, key, S, T, B, H, mth, io, state, route = c
        is_even = c in even
        if key not in need and not is_even:
            bad.append("%s needs no case: a lattice launch already gives it %d trips" % (key, lattice.get(key, (0,))[0]))
            continue
        base = gl._FIRST.get(key)
        if base is None or (fam,) + c[5:] != (base[0],) + base[5:]:
            bad.append("%s: family, H, math, io, state and route are not those of its first case in CASES" % key)
            continue
        if ic.refusal(S, T, B, H, mth, io) is not None or key not in ic.plan(S, T, B, H, mth, io, state, route):
            bad.append("%s: plan() at S = %d, T = %d, B = %d does not contain the key" % (key, S, T, B))
            continue
        rows = B * T
        if "w=12" in key and rows >= gl.G32_W16_ROWS:
            bad.append("%s: %d rows select the 16-wave form" % (key, rows))
            continue
        n, trips, cnt, last = gl.gcn_trips(key, S, rows)
        if trips < gl.LOOP_TRIPS or trips % 2 == 0:
            bad.append("%s: the keyed launch makes %d trips at %d rows, not an odd count >= %d" % (key, trips, rows, gl.LOOP_TRIPS))
        if last != trips or cnt == n:
            bad.append("%s: at %d rows every one of the %d waves makes %d trips: no ragged last trip" % (key, rows, n, trips))
        want = gl.rule_case(key, S if is_even else None)
        if c != want:
            bad.append("%s: S, T, B = %d, %d, %d; the rule says %d, %d, %d" % ((key, S, T, B) + want[2:5]))
        if not is_even and (S * 13) % 2 == 0:
            bad.append("%s: S * 13 is even: no private copy of the last tile" % key)
    for S in gl.LOOP_S_EVEN:
        got = sorted(c[6] for c in even if c[2] == S)
        if got != ["f16x3", "f32"] or (S * 13) % 2:
            bad.append("S = %d runs %s; the even-I cases are one strict f16x3 and one f32" % (S, got))
    return bad


def test_gcn_loop_cases_follow_the_rule():
    assert gcn_loop_problems(gl.GCN_LOOP_CASES) == []
    assert gl.GCN_LOOP_IMPOSSIBLE == {}
    assert len(gl.GCN_LOOP_CASES) == 85 - 6 and len(gl.GCN_LOOP_EVEN_CASES) == 4 and len(gl.loop_shapes()) == 16
    assert len({c[2:10] for c in gl.ALL_LOOP_CASES}) == 66                              # call forms: that many GPU steps
    assert (gl.LOOP_T, gl.LOOP_B, gl.LOOP_B_GI, gl.LOOP_S) == (2, 4099, {True: 8193, False: 12289}, {1: 5, 2: 17, 3: 33, 4: 49})
    assert 2 * 4099 == 8198 == 2 * 4096 + 6 == 2 * 3072 + 2054 == 4 * 2048 + 6 < gl.G32_W16_ROWS
    # the keyed launch makes three or five trips; every other launch of the five families in the step three or more (the fused
    # route's backward, gcnx_bwd at gcngi's 16 386 or 24 578 rows, makes six to twelve)
    for c in gl.ALL_LOOP_CASES:
        for k, n, trips, cnt, last in gl.gcn_launches(c):
            assert (trips in (3, 5) if k == c[1] else 3 <= trips <= 12) and last == trips and cnt < n, (c, k, trips)
    # the largest case: 24 578 rows at S = 33
    assert max(c[2] * 13 * c[3] * c[4] for c in gl.ALL_LOOP_CASES) == 33 * 13 * 24578
    # the wide-GRU keys keep H = 128
    assert sorted(c[1] for c in gl.GCN_LOOP_CASES if c[5] == 128) == sorted("gcnx_bwd_kernel<%d,f16>|io=32|dg16=0" % n for n in (1, 2, 3, 4))


def test_the_checks_notice_a_mis_tabled_entry():
    K = gl.GCN_LOOP_CASES
    at = {c[1]: i for i, c in enumerate(K)}

    def with_(key, **kw):
        i = at[key]
        c = dict(zip(("fam", "key", "S", "T", "B", "H", "math", "io", "state", "route"), K[i]))
        c.update(kw)
        return K[:i] + [tuple(c.values())] + K[i + 1:]
    x2, w12, gi, f16 = ("gcnx_bwd_kernel<2>|io=32|dg16=0", "gcn32_bwd_kernel<1>|w=12", "gcngi_fwd_kernel<3>|io=16|planes=2",
                        "gcnx_bwd_kernel<3,f16>|io=16|dg16=1")
    # a deleted case (no lattice launch at all has the io=16 fused key: 0 trips)
    for k, most in ((x2, 1), (w12, 1), (gi, 0)):
        assert gcn_loop_problems(K[:at[k]] + K[at[k] + 1:]) == ["%s makes at most %d trips on the lattice draw and has no case" % (k, most)]
    # B = 17 put back: the CASES entry itself
    assert gcn_loop_problems(with_(x2, B=17)) == [
        "%s: the keyed launch makes 1 trips at 34 rows, not an odd count >= 3" % x2,
        "%s: S, T, B = 17, 2, 17; the rule says 17, 2, 4099" % x2]
    # an even trip count: 10 000 rows = 3 x 3072 + 784 on the 12-wave grid, 12 400 = 3 x 4096 + 112 on the one-pass 16-wave grid,
    # and gcngi's split modes at 24 578 rows: 769 tiles of 32 rows on 256 blocks
    assert gcn_loop_problems(with_(x2, B=5000))[0] == "%s: the keyed launch makes 4 trips at 10000 rows, not an odd count >= 3" % x2
    assert gcn_loop_problems(with_(f16, B=6200))[0] == "%s: the keyed launch makes 4 trips at 12400 rows, not an odd count >= 3" % f16
    assert gcn_loop_problems(with_(gi, B=12289))[0] == "%s: the keyed launch makes 4 trips at 24578 rows, not an odd count >= 3" % gi
    # a case whose key is not in its own plan(): f16x3g below 4096 rows has an fp32 dg; NT = 2 is not NT = 1
    g1 = "gcnx_bwd_kernel<1>|io=32|dg16=1"
    assert gcn_loop_problems(with_(g1, B=2047)) == ["%s: plan() at S = 5, T = 2, B = 2047 does not contain the key" % g1]
    assert gcn_loop_problems(with_(x2, S=5)) == ["%s: plan() at S = 5, T = 2, B = 4099 does not contain the key" % x2]
    # a w=12 case at 16 384 rows or more
    assert gcn_loop_problems(with_(w12, B=8192)) == ["%s: plan() at S = 5, T = 2, B = 8192 does not contain the key" % w12]
    w4 = "gcn32_bwd_kernel<4>|w=12"
    assert gcn_loop_problems(with_(w4, B=8195)) == ["%s: 16390 rows select the 16-wave form" % w4]
    # a full last trip, an even S * 13, another call form, a key claimed twice, one that needs no case
    assert gcn_loop_problems(with_(x2, B=4608))[0] == "%s: at 9216 rows every one of the 3072 waves makes 3 trips: no ragged last trip" % x2
    assert gcn_loop_problems(with_(x2, S=18)) == ["%s: S, T, B = 18, 2, 4099; the rule says 17, 2, 4099" % x2, "%s: S * 13 is even: no private copy of the last tile" % x2]
    assert gcn_loop_problems(with_(x2, math="f16x3g")) == ["%s: family, H, math, io, state and route are not those of its first case in CASES" % x2]
    assert gcn_loop_problems(K + [K[0]])[0] == "%s is claimed 2 times" % K[0][1]
    w16 = next(c for c in ic.CASES if c[1] == "gcn32_bwd_kernel<1>|w=16")
    assert gcn_loop_problems(K + [w16]) == ["gcn32_bwd_kernel<1>|w=16 needs no case: a lattice launch already gives it 4 trips"]
    assert gcn_loop_problems(K, already=dict(gl.GCN_LOOP_ALREADY, **{x2: (3, "CASES", (17, 2, 17, 4))}))[0].startswith("%s is listed as already at 3 trips" % x2)
    # the even-I cases
    assert gcn_loop_problems(K, even=gl.GCN_LOOP_EVEN_CASES[1:]) == ["S = 34 runs ['f32']; the even-I cases are one strict f16x3 and one f32"]


# ==== C. the inputs ================================================================================================================
def shape_strides(shape):
    """The grid strides, in rows, of the launches of the cases that run on `shape`: ('fwd' | 'bwd' | 'gi', rows per trip of the
    whole grid), sorted.  A row r of a later trip sits where row r - stride sat one trip earlier."""
    out = set()
    for c in gl.ALL_LOOP_CASES:
        if c[2:6] == shape:
            for k, n, trips, cnt, last in gl.gcn_launches(c):
                fam, NT, x3 = gl._parts(k)
                if fam == "gcngi_fwd_kernel":
                    out.add(("gi", n * gl.GI_ROWS[x3]))
                else:
                    out.add(("bwd" if "bwd" in fam else "fwd", n))
    return sorted(out)


def gcn_loop_step(A, X, L, params, stride=None, mistake=None):
    """lattice_inputs.fp64_step restated -- the same operations in the same order, so the same bits -- with the rows walked in
    trips of `stride` (the rows one launch of the grid covers per trip) and one of gl.MISTAKES planted."""
    leaves = {k: params[k].double().clone().requires_grad_(True) for k in PARAM_KEYS}
    A, X, L = A.double(), X.double(), L.double()
    B, T, S, F = X.shape
    rows = B * T
    prev = torch.arange(rows)                  # row -> the row at its place one trip earlier (itself on the first trip)
    first = torch.zeros(rows, dtype=torch.bool)
    if stride is not None:
        for trip, lo in enumerate(range(0, rows, stride)):             # the walk: trip 0 covers rows [0, stride), trip 1 the next ...
            hi = min(lo + stride, rows)
            if trip == 0:
                first[lo:hi] = True
            else:
                prev[lo:hi] = torch.arange(lo - stride, hi - stride)
    Xr = X.reshape(rows, S, F)
    if mistake == gl.MISTAKES[0]:
        Xr = Xr[prev]
    elif mistake == gl.MISTAKES[3]:
        Xr = torch.cat([Xr[:-1], Xr[prev[-1]][None]])

    def layer(In, W, b):
        if mistake not in gl.MISTAKES[1:3]:
            return torch.relu(torch.matmul(torch.matmul(A, In), W) + b)
        P = torch.matmul(A, In)
        Z = torch.matmul(P, W) + b
        if mistake == gl.MISTAKES[2]:          # the first trip's tiles add nothing to dW and db (dX / dH1 are per tile: unharmed)
            Z = torch.where(first[:, None, None], torch.matmul(P, W.detach()) + b.detach(), Z)
            return torch.relu(Z)
        mask = (Z.detach() > 0)[prev].double()                          # the backward's mask: the previous trip's tile
        return torch.relu(Z).detach() + (Z - Z.detach()) * mask        # the forward's value is untouched

    h = layer(Xr.reshape(B, T, S, F) if mistake is None else Xr, leaves["conv1.weight"], leaves["conv1.bias"])
    h = layer(h, leaves["conv2.weight"], leaves["conv2.bias"])
    g = h.reshape(rows, S * F)
    if mistake == gl.MISTAKES[4]:
        g = g[prev]                              # the projection reads the other buffer: the previous trip's tile of g
    H = params["gru.weight_hh_l0"].shape[1]
    Y, _ = torch._VF.gru(g.reshape(B, T, S * F), torch.zeros(1, B, H, dtype=torch.float64),
                         [leaves[k] for k in PARAM_KEYS[4:]], True, 1, 0.0, False, False, True)
    loss = ((Y - L) ** 2).mean()
    loss.backward()
    return Y.detach(), float(loss), {k: leaves[k].grad for k in PARAM_KEYS}


def _gi_max(d):
    from oracle import windgnn_oracle as orc
    _, cache = orc.forward(d.A.double(), d.X.double(), {k: v.double() for k, v in d.p.items()})
    return float(cache["GI"].abs().max())


def _margins(d):
    Zs, _ = li.preacts(d.A, d.X, d.p["conv1.weight"], d.p["conv1.bias"], d.p["conv2.weight"], d.p["conv2.bias"])
    return [r["margin"] for r in li.measure(Zs, tli.STEPS)]


def largest_shift(S, T, B, H, seed):
    """The largest shift <= 0 on gru.weight_ih_l0 that brings max |GI| of the draw below gl.LOOP_GI_MAX."""
    import math
    gi0 = _gi_max(li.draw.__wrapped__(S, T, B, H, False, 0, seed))
    if gi0 < gl.LOOP_GI_MAX:
        return 0
    shift = min(0, 1 - math.ceil(math.log2(gi0 / gl.LOOP_GI_MAX)))          # (b_ih is not scaled: start one above the estimate)
    while not _gi_max(li.draw.__wrapped__(S, T, B, H, False, shift, seed)) < gl.LOOP_GI_MAX:
        shift -= 1
    return shift


def seed_figures(shape, seed, bar):
    """(the seed's largest shift, why its draw at that shift does not qualify: sentences about invariants (b), (d) and (f))."""
    S, T, B, H = shape
    shift = largest_shift(S, T, B, H, seed)
    d = li.draw.__wrapped__(S, T, B, H, False, shift, seed)
    Zs, _ = li.preacts(d.A, d.X, d.p["conv1.weight"], d.p["conv1.bias"], d.p["conv2.weight"], d.p["conv2.bias"])
    why = []
    for layer, r in enumerate(li.measure(Zs, tli.STEPS), 1):
        if not r["margin"] > tli.MARGIN:
            why.append("(b): layer %d margin %.1e" % (layer, r["margin"]))
        if not r["varies"] >= tli.LIVENESS:
            why.append("(d): layer %d mask varies %.2f" % (layer, r["varies"]))
    if not why:
        why += ["(f): '%s' moves %.2g, not more than %.2g" % (name, e, 100 * bar)
                for name, e in li.mutation_effects(d.A, d.X, d.L, d.p).items() if not e > 100 * bar]
    return shift, why


def loop_input_problems(shape, inputs=None, factor=gl.PLANT_FACTOR, figures=None):
    """What is wrong with the inputs of one shape of gl.loop_shapes(), on the oracle alone: a list of sentences."""
    S, T, B, H = shape
    shift, seed = gl.inputs_of(*shape) if inputs is None else inputs
    runs = gl.loop_shapes()[shape]
    bad = []
    d = li.draw(S, T, B, H, False, shift, seed)
    assert not torch.equal(d.A, d.A.t()) and bool((d.p["conv1.bias"] != 0).all()) and bool((d.p["conv2.bias"] != 0).all())
    assert float(d.X.min()) < 0 < float(d.X.max())
    f16 = any(m == "f16" for m, _, _ in runs)
    bar = tli._fp32_grade_bar((S, T, B, H, {(m, io) for m, io, _ in runs})) if any(m != "f16" for m, _, _ in runs) else G_TOL
    # the tabled seed is the first of 0 .. 19 whose draw, at its own largest shift, meets invariants (b), (d) and (f)
    assert 0 <= seed < gl.LOOP_SEEDS
    for s in range(seed):
        sh, why = seed_figures(shape, s, bar)
        if not why:
            bad.append("%s: seed %d (shift %d) already meets invariants (b), (d) and (f); the table says %d" % (shape, s, sh, seed))
    # the tabled shift is the largest power of two that brings max |GI| below 8
    gi = _gi_max(d)
    if not gi < gl.LOOP_GI_MAX:
        bad.append("%s: max |GI| = %.1f at shift %d: the gates saturate" % (shape, gi, shift))
    if shift < 0 and _gi_max(li.draw.__wrapped__(S, T, B, H, False, shift + 1, seed)) < gl.LOOP_GI_MAX:
        bad.append("%s: shift %d would do" % (shape, shift + 1))
    if shift > 0:
        bad.append("%s: shift %d enlarges W_ih" % (shape, shift))
    if bad:
        return bad                               # (the invariants below are those of the tabled draw)
    # invariants (a) to (f), through the lattice test's own helper ((c) where a one-pass fp16 case runs on the shape); (e) is
    # fp32 against fp64 <= 1e-5
    tli._qualify("S%d T%d B%d H%d gcn loop" % shape, d.A, d.X, d.L, d.p, bar, f16)
    # the restated step is lattice_inputs.fp64_step, bit for bit, at every stride
    Y, loss, g = li.fp64_step(d.A, d.X, d.L, d.p)
    strides = shape_strides(shape)
    for stride in sorted({s for _, s in strides}) + [None]:
        Yr, lossr, gr = gcn_loop_step(d.A, d.X, d.L, d.p, stride)
        assert torch.equal(Yr, Y) and lossr == loss and all(torch.equal(gr[k], g[k]) for k in PARAM_KEYS), (shape, stride)
    lines = []
    for role, stride in strides:
        assert B * T > 2 * stride, (shape, role, stride)
        plant = {"fwd": (0, 3), "bwd": (0, 1, 2, 3), "gi": (0, 3, 4)}[role]
        moved = {}
        for i in plant:
            Ym, _, gm = gcn_loop_step(d.A, d.X, d.L, d.p, stride, gl.MISTAKES[i])
            moved[i] = (max_abs(Ym, Y), max(rel_to_max(gm[k], g[k]) for k in PARAM_KEYS))
            if i in (1, 2):
                assert moved[i][0] == 0.0                               # (a backward mistake: the forward is the oracle's)
            if not max(moved[i]) > factor * BAR:
                bad.append("%s: '%s' at a stride of %d rows moves Y by %.1e and no gradient by more than %.1e: pick another seed"
                           % ((shape, gl.MISTAKES[i], stride) + moved[i]))
        lines.append("%s %d: %s" % (role, stride, "  ".join("[%d] %.1e %.1e" % ((i,) + v) for i, v in moved.items())))
    print("gcn loop S%d T%d B%d H%d (seed %d, shift %d): max |GI| %.2f, max |Y| %.3f; planted [mistake] (Y, worst gradient): %s"
          % (shape + (seed, shift, gi, float(Y.abs().max()), "; ".join(lines))))
    if f16:
        Yh, lossh, gh = li.fp64_step(d.A, d.X, d.L, d.p, f16_operands=True)
        fig = (max_abs(Yh, Y), abs(lossh - loss) / max(1.0, loss), max(rel_to_max(gh[k], g[k]) for k in PARAM_KEYS))
        print("    one-pass fp16 operand rounding on the reference: Y %.2e (bar %.1e)  loss %.2e (2e-3)  gradients %.2e (%.1e)"
              % (fig[0], F16_Y_TOL, fig[1], fig[2], F16_G_TOL))
        tab = (gl.F16_FIGURES if figures is None else figures).get(shape)
        if tab is None:
            bad.append("%s: a one-pass fp16 case runs here and F16_FIGURES has no entry; measured (%.2e, %.2e, %.2e)" % ((shape,) + fig))
        elif any(abs(a - b) > 0.05 * b for a, b in zip(fig, tab)):
            bad.append("%s: F16_FIGURES says (%.2e, %.2e, %.2e), measured (%.2e, %.2e, %.2e)" % ((shape,) + tuple(tab) + fig))
    return bad


SHAPES = list(gl.loop_shapes())


@pytest.mark.parametrize("shape", SHAPES, ids=["S%d-B%d-H%d" % (s[0], s[2], s[3]) for s in SHAPES])
def test_loop_inputs_qualify_and_can_tell_the_planted_mistakes(shape):
    assert loop_input_problems(shape) == []


def test_the_input_tables_cover_the_shapes_and_nothing_else():
    assert set(gl.LOOP_INPUTS) == set(SHAPES)
    assert set(gl.F16_FIGURES) == {s for s, runs in gl.loop_shapes().items() if any(m == "f16" for m, _, _ in runs)}
    assert all(0 <= seed < gl.LOOP_SEEDS and shift <= 0 for shift, seed in gl.LOOP_INPUTS.values())
    # seeds other than 0 only where f16x3g's single-plane bar (1e-3) makes invariant (f) ask for 0.1
    assert sorted(s for s, (_, seed) in gl.LOOP_INPUTS.items() if seed) == [(5, 2, 4099, 4), (5, 2, 8193, 4), (17, 2, 4099, 4), (33, 2, 4099, 4), (33, 2, 8193, 4)]
    assert {s: sorted({r for r, _ in shape_strides(s)}) for s in SHAPES if s[2] != gl.LOOP_B} == {
        s: ["bwd", "gi"] for s in SHAPES if s[2] != gl.LOOP_B}                             # the fused route's backward is gcnx's
    assert shape_strides((5, 2, 4099, 4)) == [("bwd", 3072), ("bwd", 4096), ("fwd", 4096)]
    assert shape_strides((49, 2, 4099, 4)) == [("bwd", 2048), ("bwd", 3072), ("fwd", 4096)]
    assert shape_strides((33, 2, 12289, 4)) == [("bwd", 4096), ("gi", 12288)] and shape_strides((33, 2, 8193, 4)) == [("bwd", 3072), ("gi", 8192)]


def test_the_input_check_notices_a_mistake_that_stays_under_the_factor():
    """The smallest shape's own figures against a factor no mistake reaches, a missing figure, a wrong shift and a wrong seed: all
    fail by message."""
    shape = SHAPES[0]
    got = loop_input_problems(shape, factor=1e9)
    assert len(got) == 2 + 4 + 4 and all("pick another seed" in s for s in got), got
    got = loop_input_problems(shape, figures={})
    assert len(got) == 1 and "F16_FIGURES has no entry" in got[0], got
    shift, seed = gl.inputs_of(*shape)
    assert shift < 0 and seed > 0
    assert loop_input_problems(shape, inputs=(shift + 1, seed)) == ["%s: max |GI| = 10.1 at shift %d: the gates saturate" % (shape, shift + 1)]
    assert loop_input_problems(shape, inputs=(shift - 1, seed)) == ["%s: shift %d would do" % (shape, shift)]
    # an earlier seed put into the table fails invariant (f) inside the lattice test's own helper; a later one is not the first
    with pytest.raises(AssertionError, match="conv2 bias dropped"):
        loop_input_problems(shape, inputs=(-2, 0))
    later = next(s for s in range(seed + 1, gl.LOOP_SEEDS) if not seed_figures(shape, s, 1e-3)[1])
    got = loop_input_problems(shape, inputs=(largest_shift(*shape, later), later))
    assert got and got[0].startswith("%s: seed %d (shift %d) already meets invariants (b), (d) and (f)" % (shape, seed, shift)), got


def test_layer_loop_inputs_qualify():
    """The one-layer cases' draw: Z an odd multiple of 1/32 with live masks, three trips with a ragged third, and the tile one grid
    stride earlier differs from the tile itself in out, dX and the weight gradient."""
    for S, Fi, Fo, nt in gl.LAYER_LOOP_CASES:
        stride, trips, tail = gl.layer_trips(Fi, Fo, nt)
        assert trips == 3 and 0 < tail < (gl.GCN1_WAVES if (Fi, Fo) == (13, 13) else stride), (S, Fi, Fo, nt)
        d = li.draw_layer(S, Fi, Fo, nt)
        (Z,), _ = li.preacts(d.A, d.X, d.W, d.b)
        (r,) = li.measure([Z], tli.STEPS[:1])
        assert r["odd"] and r["margin"] > tli.MARGIN and r["varies"] >= tli.LIVENESS, (S, nt, r)
        assert not torch.equal(d.A, d.A.t())
        out = torch.relu(Z)
        dZ = d.dout.double() * (Z > 0)
        dX = torch.matmul(d.A.double().t(), torch.matmul(dZ, d.W.double().t()))
        P = torch.matmul(d.A.double(), d.X.double())
        dW = torch.einsum("tsi,tso->io", P, dZ)
        stale = torch.cat([torch.arange(stride), torch.arange(nt - stride)])
        dW_first_dropped = torch.einsum("tsi,tso->io", P[stride:], dZ[stride:])
        eff = (max_abs(out[stale], out), rel_to_max(dX[stale], dX), rel_to_max(dW_first_dropped, dW))
        print("layer S%d %d -> %d, %d tiles (stride %d): stale tile moves out %.2g, dX %.2g; first trip dropped from dW %.2g" % ((S, Fi, Fo, nt, stride) + eff))
        assert min(eff) > 100 * 1e-5, (S, Fi, Fo, nt, eff)
    assert [c[1:3] for c in gl.LAYER_LOOP_CASES] == [(13, 13), (6, 9)]
