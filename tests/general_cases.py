"""The general path's loops: the persistent LDS-tiled CSR layers of windgnn_amd/csrc/general.hip restated in Python, and the
shapes at which a block of them runs a SECOND item.  A plain module: nothing here is collected.  tests/test_general_loops_host.py
holds the restatement to the source text and qualifies the inputs on the fp64 oracle alone, tests/test_gpu_general_loops.py runs
the cases on the GPU.  (The other half of those two modules, gemm_f32_kernel past one K step, is tabled with the rest of the
per-instance table: tests/instance_cases.py's gemm_f32_products(), GEMM_F32_KLOOP_CASES and GEMM_F32_FOLD_CASES.)

csr_layer_fwd_kernel and csr_layer_bwd_kernel<1> / <2> are persistent -- at most CSR_BLOCKS = 256 blocks, `for (item =
blockIdx.x; item < nitems; item += gridDim.x)` -- and an item is up to CT * RPT = 2048 output rows that share one gather source
(csr_item): the rows of floor(2048 / S) whole tiles (S <= 1024: 'group'), one tile whose second row per thread is partly dead
(1024 < S < 2048: 'tile', the group branch with G = 1), or one row block of a tile, gathered over ceil(S / 2048) source chunks
of CH rows (S >= 2048: 'rowblock').  A block runs a second item only past 256 items, which no shape compared with the fp64
oracle had before CSR_LOOP_SHAPES (asserted once in the host test)."""

CT = 1024                  # general.hip: threads per block
CH = 2048                  # source rows per LDS chunk
CSR_BLOCKS = 256           # persistent blocks
CSR_FWD_RPT = 2            # output rows per thread and item of the forward
CSR_BWD_RPT = 2            # ... of the backward (csr_layer_bwd_kernel: constexpr int RPT = 2)
SPMM_GRID_Y = 16384        # launch_gcn1_csr_bwd: the cap of csr_spmm_kernel's grid.y; its tile loop strides by it


def cdiv(a, b):
    return -(-a // b)


def csr_items(ntiles, S, RB):
    """general.hip csr_items."""
    return ntiles * cdiv(S, RB) if S >= RB else cdiv(ntiles, RB // S)


def csr_item(item, ntiles, S, RB):
    """general.hip csr_item: (tile0, ng, row0, nrows, VC) -- first tile, tiles in the group, first row, output rows, source rows."""
    if S >= RB:
        nrb = cdiv(S, RB)
        tile0 = item // nrb
        row0 = (item - tile0 * nrb) * RB
        return tile0, 1, row0, min(RB, S - row0), S
    G = RB // S
    tile0 = item * G
    ng = min(G, ntiles - tile0)
    return tile0, ng, 0, ng * S, ng * S


def csr_grid(ntiles, S, rpt):
    """general.hip csr_grid (the forward; the backward always launches CSR_BLOCKS blocks, idle ones write zero partial rows)."""
    return max(1, min(csr_items(ntiles, S, CT * rpt), CSR_BLOCKS))


def csr_plan(S, ntiles, rpt=CSR_FWD_RPT):
    """One launch of a CSR layer kernel over `ntiles` tiles of S stations: the item count, the regime, tiles per (full) item,
    `ng` of the last item, row blocks and source chunks per item, the blocks launched, the largest number of items any block
    runs, and the items beyond a block's first (`later`: the second and later trips, in item order)."""
    RB = CT * rpt
    n = csr_items(ntiles, S, RB)
    regime = "rowblock" if S >= RB else ("group" if RB // S >= 2 else "tile")
    grid = csr_grid(ntiles, S, rpt)
    last = csr_item(n - 1, ntiles, S, RB)
    return dict(items=n, regime=regime, tiles_per_item=1 if S >= RB else RB // S, ng_last=last[1], last_rows=last[3],
                row_blocks=cdiv(S, RB) if S >= RB else 1, chunks=cdiv(csr_item(0, ntiles, S, RB)[4], CH), grid=grid,
                max_items_per_block=cdiv(n, grid), later=list(range(grid, n)))


def spmm_trips(ntiles):
    """csr_spmm_kernel (the one-layer API's dX): trips of `for (tile = blockIdx.y; tile < ntiles; tile += gridDim.y)`."""
    return cdiv(ntiles, min(ntiles, SPMM_GRID_Y))


# ---- CSR layers with several items per block --------------------------------------------------------------------------------
# One shape per regime, the smallest B at its T with 258 (260) items on 256 blocks: at least two blocks run two items and the last
# item is ragged.  (S, T, B, H, shift, seed) of lattice_inputs.draw(S, T, B, H, sparse=True, shift=shift, seed=seed):
#   S = 100   B*T = 5141 tiles, 20 per item, 258 items, the last has one tile; S * 13 is a multiple of 4: the 16-byte copy-out
#   S = 700   515 tiles, 2 per item (1400 rows: the second row per thread partly live), 258 items, the last has one tile
#   S = 1100  258 tiles, one per item through the group branch (ng = 1), 76 rows live in the second pass
#   S = 2049  130 tiles, 260 items of 2048 + 1 rows over chunks of 2048 + 1 source rows; S * 13 is odd: the scalar copy-out
# shift: the power of two on gru.weight_ih_l0 that brings max |GI| on the oracle below 8 (unshifted: 89, 218, 312, 533 -- every
# gate saturated, Y = +-1.00); the largest that does.  seed: the first of 0 .. 19 whose draw meets invariant (b) of
# tests/test_lattice_inputs_host.py, min |Z| / max |Z| > 5e-5, on both layers (S = 700: seeds 0 .. 7 give 3.3e-5 .. 5.0e-5, seed 8
# 5.8e-5; S = 2049: seeds 0 .. 8 give 3.6e-5 .. 4.7e-5, seed 9 5.1e-5).  The host test re-derives both columns.
CSR_LOOP_H = 6
CSR_LOOP_SHAPES = [(100, 1, 5141, CSR_LOOP_H, -4, 0), (700, 1, 515, CSR_LOOP_H, -5, 8), (1100, 2, 129, CSR_LOOP_H, -6, 0),
                   (2049, 2, 65, CSR_LOOP_H, -7, 9)]
CSR_LOOP_REGIMES = {100: "group", 700: "group", 1100: "tile", 2049: "rowblock"}
CSR_LOOP_GI_MAX = 8.0
CSR_LOOP_SEEDS = 20
CSR_KERNELS = ["csr_layer_fwd_kernel", "csr_layer_bwd_kernel<1>", "csr_layer_bwd_kernel<2>"]

# (id, S, T, B, H, shift, seed, math, route): f32 and f16x3 everywhere (the fp32 mask and the planes form), one-pass f16 at
# S = 700 (planes with no lo plane); the training route, and the stash-less forward once per shape
CSR_LOOP_CASES = []
for _S, _T, _B, _H, _shift, _seed in CSR_LOOP_SHAPES:
    for _math in ("f32", "f16x3") + (("f16",) if _S == 700 else ()):
        CSR_LOOP_CASES.append(("csr%d_%s" % (_S, _math), _S, _T, _B, _H, _shift, _seed, _math, "train"))
    CSR_LOOP_CASES.append(("csr%d_infer" % _S, _S, _T, _B, _H, _shift, _seed, "f16x3", "infer"))

# The one-layer API (GraphConvLayer with a CsrAdjacency, widths 13 -> 13): (S, nt) of lattice_inputs.draw_layer(S, 13, 13, nt).
# (700, 515): 258 items in csr_layer_fwd_kernel and csr_layer_bwd_kernel<2>; (7, 16 385): csr_spmm_kernel's tile loop takes a
# second trip in block row 0 (and the layer kernels run 292 tiles per item: 57 items)
LAYER_LOOP_CASES = [(700, 515), (7, 16385)]

MISTAKES = ("a later item's tiles read the source of the item one grid stride earlier",
            "the conv gradients leave out each block's first item",
            "a later item's last tile drops its column offset / its second source chunk")
PLANT_FACTOR = 10            # each mistake must move Y or a gradient by more than PLANT_FACTOR x 1e-4 (the K-loop half's factor)
