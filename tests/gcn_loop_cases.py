"""The persistent tile loops of the dense graph-convolution kernels: the launch geometry of csrc/gcnx.hip, gcn32.hip and
gcngi.hip restated in Python, and a second case per instance key at which a wave (a block of gcngi) meets a THIRD tile.  A plain
module: nothing here is collected.  tests/test_gcn_loops_host.py holds the restatement to the source text, re-derives the table
and qualifies the inputs on the fp64 oracle alone; tests/test_gpu_gcn_loops.py runs the cases on the GPU.

gcnx_fwd / gcnx_bwd / gcn32_fwd / gcn32_bwd walk `for (tile = wave_id; tile < ntiles; tile += nwaves)`, one tile = one (window,
hour) row of S stations, and prefetch tile + nwaves under the current tile's math; gcngi_fwd walks `for (it = 0; it < nit; ++it)`
over tiles of R rows, block b taking tiles b, b + grid, ...  With tests/instance_cases.py's (T, B) = (2, 17) every wave runs the
loop body once: the `more` branch, the registers and LDS a prefetch lands in while the current tile still reads them, the
weight-gradient accumulators carried from a wave's tile into its next, the private copy of X's last tile (odd S * 13) met on a
later trip and gcngi's second g buffer never execute against a reference.  GCN_LOOP_CASES gives every key of the five families
that no launch on the lattice draw takes to three trips a case that does, on tests/lattice_inputs.py's draw -- live ReLU masks that differ
between stations and rows, non-zero biases, A != A^T: a tile, a mask or a partial sum taken from the wrong trip changes a number."""
import re

import instance_cases as ic
import lattice_inputs as li

GCN_FAMILIES = ("gcnx_fwd_kernel", "gcnx_bwd_kernel", "gcngi_fwd_kernel", "gcn32_fwd_kernel", "gcn32_bwd_kernel")

# ---- the launch geometry (tests/test_gcn_loops_host.py extracts the same figures from the sources) ---------------------------
FWD_WAVES = 8              # gcnx.hip and gcn32.hip: waves per forward block
FWD_GRID_CAP = 512         # ... and the cap of the forward grids: gx > 512 ? 512 : gx
BWD_GRID_CAP = 256         # gcnx.hip grid_x, gcn32.hip bwd_grid: one block per CU
BWD_WAVES = 12             # the backward block of both files, but for:
BWD_WAVES_ONE_PASS = 16    # gcnx.hip bwd_waves: the one-pass mode with NT <= 3 and a 16-bit dg
BWD4_WAVES = 8             # gcnx.hip WGNN_BWD4_WAVES: NT = 4 in every mode
G32_W16_ROWS = 16384       # gcn32.hip bwd_waves_of: 16 waves from this many rows on, with
G32_W16_SMAX = 48          # ... S <= 48
GI_ROWS = {True: 32, False: 48}   # gcngi.hip gg_cfg: rows per tile, split modes / one-pass
GI_GRID_CAP = 256          # gcngi.hip launch_gcngi_fwd: grid = min(ntile_r, 256)


def gcnx_bwd_waves(NT, x3, dg16=True):
    """gcnx.hip bwd_waves."""
    return BWD_WAVES_ONE_PASS if (not x3 and NT <= 3 and dg16) else (BWD4_WAVES if NT >= 4 else BWD_WAVES)


def gcnx_bwd_grid(rows, S, x3):
    """gcnx.hip grid_x: the divisor is bwd_waves(NT, x3) with its default DG16 = true -- the one-pass instances with an fp32 dg
    launch blocks of 12 waves on a grid counted for 16 (fewer waves, more trips; the loop strides by what was launched)."""
    return max(1, min(ic.cdiv(rows, gcnx_bwd_waves(ic.gcn_nt(S), x3)), BWD_GRID_CAP))


def gcn32_bwd_waves(S, rows):
    """gcn32.hip bwd_waves_of."""
    return 16 if (S <= G32_W16_SMAX and rows >= G32_W16_ROWS) else BWD_WAVES


def _parts(key):
    fam = ic.family_of(key)
    assert fam in GCN_FAMILIES, key
    return fam, int(re.search(r"<(\d+)", key).group(1)), ",f16>" not in key


def gcn_geometry(key, S, rows):
    """(what loops, how many of them, tiles) of the launch `key` over `rows` rows: waves over row tiles, or for gcngi blocks
    over tiles of R rows.  A bare profiler name will do where the name fixes the geometry (gcnx_bwd's dg16 defaults to 1)."""
    fam, NT, x3 = _parts(key)
    assert NT == ic.gcn_nt(S), (key, S)
    if fam in ("gcnx_fwd_kernel", "gcn32_fwd_kernel"):
        return "waves", FWD_WAVES * max(1, min(ic.cdiv(rows, FWD_WAVES), FWD_GRID_CAP)), rows
    if fam == "gcnx_bwd_kernel":
        return "waves", gcnx_bwd_waves(NT, x3, "dg16=0" not in key) * gcnx_bwd_grid(rows, S, x3), rows
    if fam == "gcn32_bwd_kernel":
        w = gcn32_bwd_waves(S, rows)
        assert "|w=" not in key or key.endswith("|w=%d" % w), (key, S, rows)
        return "waves", w * max(1, min(ic.cdiv(rows, w), BWD_GRID_CAP)), rows
    ntile_r = ic.cdiv(rows, GI_ROWS[x3])
    return "blocks", min(ntile_r, GI_GRID_CAP), ntile_r


def gcn_trips(key, S, rows):
    """(nwaves or blocks, trips of the busiest wave or block, how many waves or blocks make that many trips, the trip on which
    the last tile is met)."""
    _, n, tiles = gcn_geometry(key, S, rows)
    most = ic.cdiv(tiles, n)
    return n, most, tiles - (most - 1) * n, (tiles - 1) // n + 1


def gcn_launches(case):
    """The GCN-side launches of a case (family, key, S, T, B, H, math, io, state, route): (key, nwaves, trips, how many, the last
    tile's trip) of every key of the five families in instance_cases.plan(), in launch order."""
    S, T, B = case[2:5]
    return [(k,) + gcn_trips(k, S, B * T) for k in ic.plan(*case[2:10]) if ic.family_of(k) in GCN_FAMILIES]


def dense_lattice_cases():
    """lattice_inputs.CASES' dense entries in the form of instance_cases' tables (the key: the first the case names)."""
    return [(ic.family_of(c[1][0]), c[1][0]) + c[2:10] for c in li.CASES if not c[10]]


def window_tables():
    """Every table of window-major cases that was compared with the fp64 reference before this module: (name, cases)."""
    return (("CASES", ic.CASES), ("EDGE_CASES", ic.EDGE_CASES), ("KLOOP_CASES", ic.KLOOP_CASES),
            ("GEMM_F32_KLOOP_CASES", ic.GEMM_F32_KLOOP_CASES), ("GEMM_F32_FOLD_CASES", [c[:10] for c in ic.GEMM_F32_FOLD_CASES]),
            ("lattice_inputs.CASES", dense_lattice_cases()))


def most_trips(tables=None):
    """key -> (the most trips any launch of the tables gives the key, the table and the (S, T, B, H) that does, how many launches
    of the key there are), over every reachable key of the five families."""
    most = {k: (0, None, None, 0) for fam in GCN_FAMILIES for k in ic.FAMILIES[fam] if k not in ic.UNREACHABLE}
    for name, table in (window_tables() if tables is None else tables):
        for c in table:
            for k, n, trips, cnt, last in gcn_launches(c):
                best = most[k]
                most[k] = (trips, name, c[2:6], best[3] + 1) if trips > best[0] else best[:3] + (best[3] + 1,)
    return most


# ---- the rule ----------------------------------------------------------------------------------------------------------------
LOOP_TRIPS = 3                                    # a key needs a case where no lattice launch gives it this many trips
LOOP_T = 2
LOOP_B = 4099                                     # 8198 rows = 2 x 4096 + 6 = 2 x 3072 + 2054 = 4 x 2048 + 6, below 16 384
LOOP_B_GI = {True: 8193, False: 12289}            # gcngi: 16 386 rows = 512 x 32 + 2, 24 578 = 512 x 48 + 2: 513 tiles on 256 blocks
LOOP_S = {1: 5, 2: 17, 3: 33, 4: 49}              # NT -> S; S * 13 is odd: the private copy of the last tile, met on the last trip
LOOP_S_EVEN = (34, 64)                            # once each in strict f16x3 and in f32: XLOAD's even-I branch, four full row tiles

# Which keys need a case.  Over EVERY table (most_trips()) 34 of the 85 keys already make three trips or more somewhere -- not the
# three 16-wave keys alone: the threshold cases of the GEMM families (16 419, 24 483 and 36 888 rows) launch the fp32-I/O GCN
# kernels as by-products, and the NT = 4 backwards with a 16-bit dg make three trips at 4098 rows on 2048 waves.  All of those
# launches but the six at 16 384 rows are on tests/test_gpu_instances.py's draw (A > 0, X > 0: the ReLU masks are nearly all
# live), on which a mask taken from the wrong trip's tile changes little or nothing.  So the rule counts the launches of
# lattice_inputs.CASES alone: a key gets a case unless a LATTICE launch takes it to three trips.
# key -> (trips, the table, its (S, T, B, H)); the host test recomputes it and prints both columns.
GCN_LOOP_ALREADY = {}                             # filled below: the three 16-wave backwards and the gcn32 forwards beside them

# Keys that cannot follow the rule: key -> reason.  (None: plan() contains every key at the rule's dims.)
GCN_LOOP_IMPOSSIBLE = {}

_FIRST = {}
for _c in ic.CASES:
    _FIRST.setdefault(_c[1], _c)


def rule_case(key, S=None):
    """The rule's case of a key: T = 2, B = 4099 (gcngi: 8193 split modes, 12 289 one-pass), S = LOOP_S[NT] unless given, and H,
    math, I/O, state and route of the key's first case in instance_cases.CASES."""
    fam, NT, x3 = _parts(key)
    base = _FIRST[key]
    B = LOOP_B_GI[x3] if fam == "gcngi_fwd_kernel" else LOOP_B
    return (fam, key, LOOP_S[NT] if S is None else S, LOOP_T, B) + base[5:]


for _k, (_trips, _where, _dims, _n) in most_trips(window_tables()[-1:]).items():
    if _trips >= LOOP_TRIPS:
        GCN_LOOP_ALREADY[_k] = (_trips, _where, _dims)

# (family, key, S, T, B, H, math, io, state, route): one per key outside GCN_LOOP_ALREADY, in the order of instance_cases.FAMILIES
GCN_LOOP_CASES = [rule_case(k) for fam in GCN_FAMILIES for k in ic.FAMILIES[fam]
                  if k not in ic.UNREACHABLE and k not in GCN_LOOP_ALREADY and k not in GCN_LOOP_IMPOSSIBLE]
# ... and the even-I cases, carried by the backward's key (the step launches the forward of the same NT too)
GCN_LOOP_EVEN_CASES = [rule_case(k, S) for S in LOOP_S_EVEN
                       for k in ("gcnx_bwd_kernel<%d>|io=32|dg16=0" % ic.gcn_nt(S), "gcn32_bwd_kernel<%d>|w=12" % ic.gcn_nt(S))]
ALL_LOOP_CASES = GCN_LOOP_CASES + GCN_LOOP_EVEN_CASES

# ---- the inputs: lattice_inputs.draw(S, T, B, H, shift=, seed=) ---------------------------------------------------------------
# shift: gru.weight_ih_l0 times 2^shift, by general_cases.CSR_LOOP_SHAPES' rule: the largest shift that brings max |GI| on the
# oracle below 8 (13 S inputs of up to ~30 each against weights of order 1 / sqrt(H) saturate every gate unshifted), per seed.
# seed: the first of 0 .. 19 whose draw, at its own shift, meets invariants (b), (d) and (f) of tests/test_lattice_inputs_host.py:
# 0 except on the five shapes where an f16x3g case runs below 16 384 rows or at 16 386 -- its single-plane bar of 1e-3 makes (f) ask
# that 'conv2 bias dropped' move a figure by 0.1, and seed 0 gives 0.05 .. 0.095.  Every planted loop mistake (MISTAKES) must then
# move Y or a gradient by more than 10 x 1e-4 (none came near: the smallest is 0.098).  The host test re-derives both columns.
# (S, T, B, H) -> (shift, seed)
LOOP_GI_MAX = 8.0
LOOP_SEEDS = 20
LOOP_INPUTS = {
    (5, 2, 4099, 4): (-3, 4), (17, 2, 4099, 4): (-3, 2), (33, 2, 4099, 4): (-3, 1), (49, 2, 4099, 4): (-3, 0),
    (5, 2, 4099, 128): (0, 0), (17, 2, 4099, 128): (-1, 0), (33, 2, 4099, 128): (-1, 0), (49, 2, 4099, 128): (-2, 0),
    (5, 2, 8193, 4): (-2, 3), (5, 2, 12289, 4): (-3, 0), (17, 2, 8193, 4): (-3, 0), (17, 2, 12289, 4): (-3, 0),
    (33, 2, 8193, 4): (-3, 4), (33, 2, 12289, 4): (-4, 0), (34, 2, 4099, 4): (-4, 0), (64, 2, 4099, 4): (-4, 0),
}

# One-pass fp16 cases: (Y, loss, worst gradient) of lattice_inputs.fp64_step(f16_operands=True) against fp64_step() on the shape's
# inputs, as lattice_inputs.F16_FIGURES has them; a case's bar is the larger of the imported bar and twice its figure.
# (S, T, B, H) -> figures; the host test recomputes them
F16_FIGURES = {                      # every figure is below its imported bar (2e-2, 2e-3, 5e-2): the bars are the imported ones
    (5, 2, 4099, 4): (8.80e-4, 3.40e-6, 4.46e-4), (17, 2, 4099, 4): (1.24e-3, 1.27e-5, 4.06e-4),
    (33, 2, 4099, 4): (1.59e-3, 7.41e-5, 5.46e-4), (49, 2, 4099, 4): (1.18e-3, 3.76e-5, 4.57e-4),
    (5, 2, 4099, 128): (1.46e-3, 1.87e-5, 3.87e-4), (17, 2, 4099, 128): (9.93e-4, 3.44e-6, 3.56e-4),
    (33, 2, 4099, 128): (1.84e-3, 7.04e-6, 2.83e-4), (49, 2, 4099, 128): (9.92e-4, 1.30e-5, 3.98e-4),
    (5, 2, 12289, 4): (6.98e-4, 1.96e-5, 4.01e-4), (17, 2, 12289, 4): (2.03e-3, 1.54e-4, 6.05e-4),
    (33, 2, 12289, 4): (9.14e-4, 1.32e-5, 3.10e-4),
}

MISTAKES = ("a later-trip tile computed from the X of the tile one grid stride earlier",
            "the backward's ReLU masks of a later-trip tile taken from the previous trip's tile",
            "the conv gradients leave out each wave's first trip",
            "the last tile reads the tile one stride earlier",
            "gcngi: tile `it` consumed from g buffer (it + 1) & 1")
PLANT_FACTOR = 10            # each mistake must move Y or a gradient by more than PLANT_FACTOR x 1e-4


def loop_shapes():
    """The distinct (S, T, B, H) of ALL_LOOP_CASES -> the (math, io, key) run on it, in table order."""
    out = {}
    for c in ALL_LOOP_CASES:
        out.setdefault(c[2:6], []).append((c[6], c[7], c[1]))
    return out


def inputs_of(S, T, B, H):
    return LOOP_INPUTS.get((S, T, B, H), (0, 0))


# ---- the one-layer kernels (GraphConvLayer over a dense adjacency) -----------------------------------------------------------
# gcn.hip gcn_fwd_kernel<1> / gcn_bwd_kernel<1> (13 -> 13) and gcn_any.hip's trio are grid-stride over tiles too;
# lattice_inputs.LAYER_CASES gives them five tiles.  (S, Fi, Fo, nt) of lattice_inputs.draw_layer: three trips with a ragged
# remainder.  Filled in below the restated caps.
LAYER_LOOP_CASES = []
GCN1_WAVES = 4             # gcn.hip WAVES: tiles per block and trip
GCN1_GRID_CAP = 1024       # gcn.hip grid_for
GA_GRID_CAP = 1024         # gcn_any.hip ga_grid: one tile per block and trip


def layer_trips(Fi, Fo, nt):
    """(tiles per trip of the whole grid, trips of the busiest block, tiles of the last trip) of the one-layer kernels: 13 -> 13
    is gcn.hip's (four waves a block, one tile each), any other width pair gcn_any.hip's (one tile a block)."""
    if (Fi, Fo) == (13, 13):
        stride = GCN1_WAVES * max(1, min(ic.cdiv(nt, GCN1_WAVES), GCN1_GRID_CAP))
    else:
        stride = min(nt, GA_GRID_CAP)
    return stride, ic.cdiv(nt, stride), nt - (ic.cdiv(nt, stride) - 1) * stride


# 13 -> 13: 8195 = 2 x 4096 + 3 tiles -- a third trip in block 0 alone, with three of its four waves live;
# 6 -> 9: 2051 = 2 x 1024 + 3 tiles
LAYER_LOOP_CASES += [(7, 13, 13, 8195), (7, 6, 9, 2051)]
