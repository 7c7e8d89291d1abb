"""The loop regimes of the fused step tail (csrc/finish.hip: finish_kernel, finish_norm_kernel) restated in Python, and a table
of cases that takes seg_tn, seg_plain and seg_conv through every one of them.  A plain module: nothing here is collected.
tests/test_finish_regimes_host.py holds the restatement to the source text, lists every regime reachable with B*T <= ROWS_MAX and
qualifies the inputs on the fp64 oracle alone (planted reduction mistakes); tests/test_gpu_finish_regimes.py runs the cases on
the GPU.

The three reductions are unrolled loops whose shape depends on run-time numbers alone:
  seg_tn     pgemm_tn_kernel's partials (the fp16-plane modes).  splitk < 4: one quad per thread, a plain z loop ('flat').  Else
             four z phases ty = 0 .. 3 ('phased'): a 16-stride body `for (; z + 12 < splitk; z += 16)` (four loads a trip), a tail
             `for (; z < splitk; z += 4)`, an LDS fold over the phases; wave 0 alone goes on to Adam and the image stores.
  seg_plain  [z][M][pitch] partials of gemm.hip and gemm32.hip (exact fp32): body `for (; z + 8 <= splitk; z += 8)`, then a tail
             of single chunks; gemm32.hip's rows are padded to `pitch`, and from B > 768 its dW_hh rows are remapped (msplit).
  seg_conv   the per-workgroup partial rows of the GCN backward: eight row phases ty = 0 .. 7, body `for (; b + 24 < conv_rows;
             b += 32)`, tail `for (; b < conv_rows; b += 8)`, an LDS fold over the phases.
  wide image stores (seg_tn, W_ih alone): 8-byte, quad-transposed stores where 13 S and 3 H are multiples of 4.
The split-K counts come from instance_cases.tn_products() / gemm_f32_products() (pick_splitk is restated there, once), conv_rows
from gcn_loop_cases' grids.

A *regime* of a segment is the trips its loops make, the body's capped at BODY_CAP (a third trip of an unrolled body runs the
code of the second): tn_regime(), plain_regime(), conv_regime()."""
import instance_cases as ic
import gcn_loop_cases as gl

BODY_CAP = 2
ROWS_MAX = 4200                                   # every case has B*T <= ROWS_MAX: the regime table is exact up to here
TN_FLAT_BELOW = 4                                 # finish.hip seg_tn: `if (s.splitk < 4)`
TN_PHASES, TN_BODY_STRIDE, TN_BODY_REACH, TN_TAIL_STRIDE = 4, 16, 12, 4       # z = ty; z + 12 < splitk; z += 16; then z += 4
PLAIN_BODY = 8                                    # seg_plain: z + 8 <= splitk; z += 8; then ++z
CONV_PHASES, CONV_BODY_STRIDE, CONV_BODY_REACH, CONV_TAIL_STRIDE = 8, 32, 24, 8   # b = ty; b + 24 < conv_rows; b += 32; then b += 8
CSR_ROWS = 256                                    # general.hip CSR_BLOCKS: the CSR backward's partial rows, whatever the size
GEMM_F32_BK = ic.GEMM_F32_BK


def _walk(phase, n, reach, body_stride, tail_stride):
    """(body trips, tail trips) of `for (i = phase; i + reach < n; i += body_stride) ..; for (; i < n; i += tail_stride) ..`."""
    i, body, tail = phase, 0, 0
    while i + reach < n:
        i += body_stride
        body += 1
    while i < n:
        i += tail_stride
        tail += 1
    return body, tail


def tn_trips(sk):
    """seg_tn at splitk = sk: None in the flat branch, else [(body trips, tail trips)] of the four z phases."""
    if sk < TN_FLAT_BELOW:
        return None
    return [_walk(ty, sk, TN_BODY_REACH, TN_BODY_STRIDE, TN_TAIL_STRIDE) for ty in range(TN_PHASES)]


def plain_trips(sk):
    """seg_plain at splitk = sk: [(body trips, tail trips)] of its one phase (`z + 8 <= splitk` is `z + 7 < splitk`)."""
    return [_walk(0, sk, PLAIN_BODY - 1, PLAIN_BODY, 1)]


def conv_trips(rows):
    """seg_conv at conv_rows = rows: [(body trips, tail trips)] of the eight row phases."""
    return [_walk(ty, rows, CONV_BODY_REACH, CONV_BODY_STRIDE, CONV_TAIL_STRIDE) for ty in range(CONV_PHASES)]


def _capped(trips):
    return tuple(min(b, BODY_CAP) for b, _ in trips), tuple(t for _, t in trips)


def tn_regime(sk):
    """('flat', splitk), or ('phased', body trips of the four phases capped at BODY_CAP, their tail trips)."""
    return ("flat", sk) if sk < TN_FLAT_BELOW else ("phased",) + _capped(tn_trips(sk))


def plain_regime(sk):
    """(body trips capped at BODY_CAP, tail trips)."""
    body, tail = _capped(plain_trips(sk))
    return body[0], tail[0]


def conv_regime(rows):
    """(body trips of the laziest and of the busiest row phase, capped; the tail: 'none', 'even' -- every phase the same trips --
    or 'ragged').  The tail's own trip count (up to four) is no regime: it is one rolled loop."""
    body, tail = _capped(conv_trips(rows))
    return min(body), max(body), "none" if max(tail) == 0 else ("even" if min(tail) == max(tail) else "ragged")


def tail_follows_body(trips):
    """Some phase runs the unrolled body and then the tail."""
    return trips is not None and any(b > 0 and t > 0 for b, t in trips)


def ragged(trips):
    """The phases do not all run the same trips."""
    return trips is not None and len(set(trips)) > 1


def tail_chunks(trips, stride, body_stride):
    """The indices the TAIL loops sum (per phase: after its body trips), sorted: what a tail that never ran would drop."""
    out = []
    for ph, (b, t) in enumerate(trips):
        out += [ph + b * body_stride + k * stride for k in range(t)]
    return sorted(out)


def last_of_phase(trips, stride, body_stride, phase):
    """The last index phase `phase` sums (None: it sums nothing)."""
    b, t = trips[phase]
    if t:
        return phase + b * body_stride + (t - 1) * stride
    return phase + (b - 1) * body_stride + (body_stride - stride) if b else None


def wide_stores(S, H, math):
    """seg_tn's wide image stores run for W_ih: fp16-plane images (every mode but exact fp32) and 13 S, 3 H multiples of 4."""
    return math != "f32" and (13 * S) % 4 == 0 and (3 * H) % 4 == 0


def conv_rows(S, T, B, H, math, csr=False):
    """api.hip fill_reduce, a.conv_rows."""
    if csr:
        return CSR_ROWS
    if math != "f32":
        return gl.gcnx_bwd_grid(B * T, S, math in ("f16x3", "f16x3g"))
    return max(1, min(ic.cdiv(B * T, gl.gcn32_bwd_waves(S, B * T)), gl.BWD_GRID_CAP))


def conv_waves(S, T, B, H, math):
    """Waves per workgroup of the dense GCN backward that writes the partial rows: tile t (one (window, hour) row) is summed
    into row (t % (waves x conv_rows)) // waves."""
    if math != "f32":
        return gl.gcnx_bwd_waves(ic.gcn_nt(S), math in ("f16x3", "f16x3g"))
    return gl.gcn32_bwd_waves(S, B * T)


def segments(S, T, B, H, math, csr=False):
    """What one deferred step hands finish: {'ih', 'hh': dict(family, sk, kchunk, chunks, regime, trips, remap), 'conv_rows',
    'conv', 'wide'}.  family: 'tn' (pgemm_tn_kernel's layout, seg_tn), 'gemm' (gemm.hip, seg_plain), 'gemm32' (gemm32.hip,
    seg_plain with padded rows).  kchunk: rows of the contraction per K chunk; chunks: the non-empty ones (the splitters round
    kchunk up to whole stages, so the last of the sk may start past the rows: they hold zeros).  remap: the msplit / rows1 row
    remap runs (dW_hh of the register-resident recurrences that store dGHn alone)."""
    BT = B * T
    out = {}
    tn = {p["role"]: p for p in ic.tn_products(S, T, B, H, math)}
    f32 = {p[1]: p for p in ic.gemm_f32_products(S, T, B, H, math) if p[1] in ("dW_ih", "dW_hh")}
    assert bool(tn) != bool(f32), (S, T, B, H, math)
    for seg, role in (("ih", "dW_ih"), ("hh", "dW_hh")):
        if tn:
            p = tn[role]
            fam = "gemm32" if ic.family_of(p["key"]) == "gemm32_tn_kernel" else "tn"
            sk, kchunk, chunks = p["sk"], p["kchunk"], p["chunks"]
            if fam == "tn":
                remap = role == "dW_hh" and H <= 127          # dghn: x3 && !gen_gru
            else:
                remap = role == "dW_hh" and B > 768           # dghn: rec32 && g32tn
        else:
            fam, sk = "gemm", f32[role][5]
            kchunk = ic.rup(ic.cdiv(BT, sk), GEMM_F32_BK)     # gemm.hip launch_gemm_f32's kchunk
            chunks, remap = ic.cdiv(BT, kchunk), False
        out[seg] = dict(family=fam, sk=sk, kchunk=kchunk, chunks=chunks, remap=remap,
                        regime=tn_regime(sk) if fam == "tn" else plain_regime(sk),
                        trips=tn_trips(sk) if fam == "tn" else plain_trips(sk))
    out["conv_rows"] = conv_rows(S, T, B, H, math, csr)
    out["conv"] = conv_regime(out["conv_rows"])
    out["wide"] = wide_stores(S, H, math) and out["ih"]["family"] == "tn"
    return out


# ---- the cases -------------------------------------------------------------------------------------------------------------------
# (S, T, B, H, csr): the shapes; MODES[shape kind] the math modes run on them.  T = 2 and a ladder of B; per rung (B*T: TN split-K,
# gemm.hip split-K, conv_rows at 12 waves / at the one-pass mode's 16), at S = 5, H = 9 and at S = 8, H = 12 alike (one tile a chunk):
#     48    96:  1  1    8 /   6     flat 1; conv tail only, all phases one trip
#     64   128:  2  1   11 /   8
#    100   200:  3  1   17 /  13
#    130   260:  4  2   22 /  17     four phases, one chunk each
#    160   320:  5  2   27 /  20     ragged phases; conv: body in phases 0 .. 2 only
#    190   380:  5  2   32 /  24     conv body exactly once, no tail
#    200   400:  6  3   34 /  25
#    224   448:  7  3   38 /  28     conv tail behind the body
#    240   480:  7  3   40 /  30     ... one tail trip in every phase
#    260   520:  8  4   44 /  33     TN tail twice per phase
#    360   720:  8  5   60 /  45     conv: second body trip in phases 0 .. 3 only
#    432   864:  8  6   72 /  54     conv body twice, tail once everywhere
#    450   900:  8  7   75 /  57
#    520  1040: 16  8   87 /  65     TN body exactly once, no tail; gemm.hip body exactly once
#    768  1536: 24  8  128 /  96     TN body then tail, every chunk live (kchunk = 64)
#    776  1552: 24  8  130 /  97     ... at kchunk = 96 only 17 of the 24 chunks hold rows: the others are zeros the GEMM wrote
#   1030  2060: 32 16  172 / 129     TN body twice, no tail
#   1280  2560: 40 16  214 / 160     TN body twice then tail, every chunk live
#   1290  2580: 40 16  215 / 162     ... 27 of 40 live: the whole tail sums zeros
#   1540  3080: 48 24  256 / 193     gemm.hip body three times; conv_rows at its cap
LADDER_T = 2
LADDER_B = (48, 64, 100, 130, 160, 190, 200, 224, 240, 260, 360, 432, 450, 520, 768, 776, 1030, 1280, 1290, 1540)
NARROW, WIDE = (5, 9), (8, 12)                     # (S, H); WIDE: 13 S = 104 and 3 H = 36 are multiples of 4
SPLIT_MODES = ("f32", "f16x3", "f16x3g")
SHAPES = [(S, LADDER_T, B, H, False) for S, H in (NARROW, WIDE) for B in LADDER_B]
# the wide stores once more at T = 3: TN split-K 4 and 8
WIDE_T3 = [(8, 3, 86, 12, False), (8, 3, 171, 12, False)]
# gemm32.hip's partials (B*T >= 4096, rows padded to 16 floats): with the msplit remap (B > 768) and without; split-K 64 both
G32 = [(5, 2, 2049, 9, False), (5, 6, 700, 9, False)]
# the wide-GRU path (H = 200: no row remap in either segment, two tiles a chunk) and a CsrAdjacency (conv_rows = 256), TN split-K 24
WIDE_GRU = [(5, 2, 776, 200, False)]
CSR = [(5, 2, 776, 9, True)]
SHAPES += WIDE_T3 + G32 + WIDE_GRU + CSR


def modes_of(shape):
    S, T, B, H, csr = shape
    narrow_ladder = (S, H) == NARROW and T == LADDER_T and not csr and B in LADDER_B
    return SPLIT_MODES + (("f16",) if narrow_ladder else ())


# (S, T, B, H, csr, math)
CASES = [shape + (m,) for shape in SHAPES for m in modes_of(shape)]

# the nine shapes of the two tests that compared finish with anything before this table (tests/test_gpu_parity.py
# test_finish_kernel_equals_..., tests/test_gpu_clip.py test_finish_norm_and_finish_clipped_...; the latter runs six of them)
LEGACY_SHAPES = [(34, 24, 256, 102, False), (7, 12, 32, 21, False), (5, 3, 17, 9, False), (20, 4, 6, 200, False),
                 (100, 3, 4, 60, True), (64, 2, 3, 127, False), (4, 3, 5, 4, False), (8, 5, 9, 12, False), (28, 6, 40, 100, False)]
LEGACY_MODES = ("f32", "f16x3", "f16x3g", "f16")

# ---- the inputs: lattice_inputs.draw(S, T, B, H, sparse=csr, shift=, seed=) ------------------------------------------------------
# By gcn_loop_cases.LOOP_INPUTS' rules: shift = the largest power of two on gru.weight_ih_l0 that brings max |GI| on the oracle
# below 8; seed = the first of 0 .. 19 whose draw, at its own shift, meets invariants (b), (d) and (f) of
# tests/test_lattice_inputs_host.py.  tests/test_finish_regimes_host.py re-derives both columns.
# (S, T, B, H, csr) -> (shift, seed)
GI_MAX = gl.LOOP_GI_MAX
SEEDS = gl.LOOP_SEEDS
INPUTS = {
    (5, 2, 48, 9, False): (-2, 0), (5, 2, 64, 9, False): (-2, 0), (5, 2, 100, 9, False): (-2, 0),
    (5, 2, 130, 9, False): (-3, 0), (5, 2, 160, 9, False): (-2, 0), (5, 2, 190, 9, False): (-2, 0),
    (5, 2, 200, 9, False): (-2, 0), (5, 2, 224, 9, False): (-2, 0), (5, 2, 240, 9, False): (-2, 0),
    (5, 2, 260, 9, False): (-2, 0), (5, 2, 360, 9, False): (-2, 0), (5, 2, 432, 9, False): (-2, 0),
    (5, 2, 450, 9, False): (-2, 0), (5, 2, 520, 9, False): (-2, 0), (5, 2, 768, 9, False): (-1, 0),
    (5, 2, 776, 9, False): (-2, 0), (5, 2, 1030, 9, False): (-2, 0), (5, 2, 1280, 9, False): (-2, 0),
    (5, 2, 1290, 9, False): (-2, 0), (5, 2, 1540, 9, False): (-2, 0), (8, 2, 48, 12, False): (-2, 0),
    (8, 2, 64, 12, False): (-2, 0), (8, 2, 100, 12, False): (-2, 0), (8, 2, 130, 12, False): (-1, 0),
    (8, 2, 160, 12, False): (-2, 0), (8, 2, 190, 12, False): (-3, 0), (8, 2, 200, 12, False): (-2, 0),
    (8, 2, 224, 12, False): (-2, 0), (8, 2, 240, 12, False): (-1, 0), (8, 2, 260, 12, False): (-2, 0),
    (8, 2, 360, 12, False): (-2, 0), (8, 2, 432, 12, False): (-2, 0), (8, 2, 450, 12, False): (-2, 0),
    (8, 2, 520, 12, False): (-2, 0), (8, 2, 768, 12, False): (-2, 0), (8, 2, 776, 12, False): (-2, 0),
    (8, 2, 1030, 12, False): (-2, 0), (8, 2, 1280, 12, False): (-2, 0), (8, 2, 1290, 12, False): (-2, 0),
    (8, 2, 1540, 12, False): (-1, 0), (8, 3, 86, 12, False): (-2, 0), (8, 3, 171, 12, False): (-2, 0),
    (5, 2, 2049, 9, False): (-2, 7), (5, 6, 700, 9, False): (-2, 0), (5, 2, 776, 200, False): (0, 0),
    (5, 2, 776, 9, True): (-2, 0),
}

PLANTS = ("the chunks summed by the tail after an unrolled body dropped",
          "the last chunk of one z phase added twice",
          "the partial rows summed by seg_conv's tail dropped")
PLANT_FACTOR = gl.PLANT_FACTOR                   # each planted mistake must move some gradient by more than PLANT_FACTOR x 1e-4 of max


def inputs_of(shape):
    return INPUTS.get(tuple(shape), (0, 0))
