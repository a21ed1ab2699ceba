"""Float64 restatement of the GEMM family (csrc/gemm.hip, gemm_core.hpp, gemm_dma.hpp, gemm_p8.hpp: pk_gemm_ex, pk_gemm, pk_gemm_splitk), the seeded cases that
reach every main loop and epilogue of the switch tables in gemm_ex / pk_gemm_splitk, and a per-element checker.  CPU only; tests/test_gemm_parity_host.py shows
what the checker rejects, tests/test_gemm_parity_gpu.py runs the kernels against it.

Operands.  Every case is strided, poisoned and guarded (geometry(), build()): lda > K, ldw > round_up(K, BK) (except the `w_tight` cases, which exist to make
pk_gemm fall back to the register-staged loops), ldc > N, ldr != ldc, ldc2 != ldc; A has more physical rows than M, W is the first N rows of a taller matrix,
bias / ln_s / ln_t / col_off are the first N entries of longer vectors.  Whatever the contract says is not read holds the poison (NaN, +Inf in a second pass):
A's columns K..lda and the rows no logical row maps to, W's rows >= N and its columns behind the k-tile padding (the padding itself is zero: the packers'
contract), the vectors' tails, the residual's columns N..ldr and rows >= M, ln_stats rows >= M.  Outputs (C, C2, stats_out, both copies under dup_rows, the
scatter target) sit in buffers pre-filled with a NaN-valued sentinel bit pattern with G guard rows in front and behind and slack columns; check() compares
every byte outside the result region with the sentinel AS INTEGERS and refuses a NaN / Inf inside it.

Two data sets.
  grid   dyadic rationals: A integers in [-8, 8], W multiples of 1/16 in [-1, 1], bias / residual multiples of 1/16 -- every partial sum of sum_k a w, in any
         order, is exact in f32 (build() asserts max_mn (sum_k |a||w| + |bias| + |res|) / grid step < 2^24).  split-bf16 has two forms so that each cross
         product is exercised and stays exact: gridA (A multiples of 2^-6: a non-zero low plane, W bf16-exact) and gridW (W multiples of 2^-10).  Wherever the
         epilogue is exact (no activation or ReLU, no LayerNorm fold) the result must EQUAL the f64 reference rounded once to the output type (values are
         compared, so the sign of a zero is free).
  rand   Gaussian A, W / sqrt(K); one row in eight of A is scaled by 1e3 and one by 1e-3, so a tensor-wide norm could not hide a bad small row.  Each element
         is held to a first-order bound computed in f64 from the case's own operands (reference()):
           accumulate  K 2^-23 S_mn, S_mn = sum_k |a_mk||w_nk|: the worst case of a K-term f32 sum in unknown order, one ulp (not half) per add since the
                       matrix unit's internal accumulation is not documented as round-to-nearest-even
           split       (2^-17 + 2^-17 + 2^-18) S_mn: the two operand splits x = hi + lo and the dropped lo.lo product (split-bf16)
           epilogue    one ulp (2^-23) of the running value per f32 operation: bias, the 0.1f product (and 2^-24 for 0.1f itself), the residual
           ln          the LayerNorm fold rstd (acc - mean s) + t against LN in f64 followed by the product: the f32 sums of the row statistics (K terms
                       in-loop; ceil(K / 32) handed-over partials, each rounded once), the cancellation of E[x^2] - mean^2, the 1-ulp v_rsq_f32, the rounding
                       of s, and the roundings of the expression itself; split-bf16 in-loop statistics see x as hi + lo (2^-16) and drop lo^2
           gelu        bf16 / split-bf16: the rational erf of common.hpp, 1.5e-7 absolute as documented there plus 8 2^-24 for its f32 evaluation (five
                       fmas, v_rcp, __expf and its argument); f32: erff, allowed ERFF_C = 4 ERFF_CPU_RATIO units of 2^-24, the CPU's erff measured against
                       a float64 erf by the host test; then the products 0.5 x (1 + erf) gate
         bf16 C: the value must be the round-to-nearest-even of some f32 inside the f32 bound (an interval check on the bf16 values).
stats_out is checked against the sum / sum of squares of the SAME launch's output as the consumer reads it (bf16-rounded when there is a C2 or a bf16 C) to
40 2^-24 (sum |x|, sum x^2) per 32-column chunk.  Bit for bit on both sets: C2 = RNE bf16 of C, the dup_rows copy = the original rows.

Cases name their branch (branch_of()): the main-loop instantiation, how it was reached, the epilogue.  The host test asserts the set reached equals the set
written out by hand from the switch tables.

On record (profiles/gemm_parity.txt): the split term is an average-case constant (an operand at the lower end of its binade loses 2^-16 to x = hi + lo, not
2^-17); at K = 4, where a single product dominates, the split-bf16 loops and the CPU emulation alike use 0.90 of the bound.  The constant stays as stated.

Not covered here: the write-through / non-temporal copies of the vector epilogue (bit-equality in tests/test_cache_policy_gpu.py), the tuning variables
PK_GEMM_PANEL / PK_GEMM_KROT / PK_GEMM_T128 (read once per process), the w_gap rows of GemmOperands (qkv kernels only), matrices near the 4 GiB descriptor
limit."""
import math
import zlib
from types import SimpleNamespace as NS

import torch

F32, BF16, BF16X3 = 0, 1, 2
ACT_NONE, ACT_GEGLU, ACT_LEAKY, ACT_RELU = 0, 1, 2, 3
TNAME = {F32: 'f32', BF16: 'bf16', BF16X3: 'x3'}
ANAME = {ACT_NONE: 'none', ACT_GEGLU: 'geglu', ACT_LEAKY: 'leaky', ACT_RELU: 'relu'}
EPI_NAME = {0: None, 1: 'OUT', 2: 'FF2A', 3: 'FF2B', 4: 'FF1'}
NAN, INF = float('nan'), float('inf')
POISONS = (NAN, INF)
U1, U24 = 2.0 ** -23, 2.0 ** -24
SPLIT = 2.0 ** -17 + 2.0 ** -17 + 2.0 ** -18
ERF_FAST_ABS = 1.5e-7 + 8 * U24
ERFF_CPU_RATIO = 1.0             # measured 1.000 (tests/test_gemm_parity_host.py::test_erff_allowance), recorded rounded up; factor 4 for the device library
ERFF_C = 4 * ERFF_CPU_RATIO
GELU_LIP = 1.13                  # max |gelu'|
STATS_ULPS = 40                  # 32 adds and the two shuffles of a chunk, with slack
LN_EPS = 1e-5
G = 2                            # guard rows in front of and behind every output
SENT32, SENT16 = 0x7FC5A5A5, 0x7FC5

VARIANTS = {F32: (1, 2, 3, 8, 9, 24), BF16: (1, 2, 8, 9, 24, 27, 33, 50), BF16X3: (3, 8, 9, 24, 27)}
_DMA_GEO = {3: (64, 64, 4, '4w'), 8: (64, 64, 2, '4w'), 9: (128, 128, 2, '4w'), 24: (128, 128, 2, '8w'), 27: (128, 64, 2, '4w'), 33: (64, 64, 3, '4w+2p'),
            50: (256, 256, 2, 'p8')}


def ceil_to(a, b):
    return -(-a // b) * b


def loop_of(dtype, variant, a_f32=True, ln=0):
    """the main loop gemm_ex launches for (dtype, variant): name, tile, k-tile, ring depth, whether it writes stats_out (TN = 2)"""
    T, bk = TNAME[dtype], 64 if dtype == BF16 else 32
    if variant in (1, 2):
        b = 64 * variant
        return NS(name=f'reg<{T},{"f32" if a_f32 else T},{b}x{b}>', BM=b, BN=b, BK=bk, ST=2, tn2=False, dma=False)
    if ln:                                                # the folded GEMM has its own two tiles per type (gemm_ex: `big`)
        big = variant in (24, 2, 9, 50)
        b, w = (128, '4w' if dtype == BF16X3 else '8w') if big else (64, '4w')
        return NS(name=f'dma<{T},{b}x{b},{w},2st,ln{ln}>', BM=b, BN=b, BK=bk, ST=2, tn2=not (big and dtype == BF16X3), dma=True)
    bm, bn, st, w = _DMA_GEO[variant]
    return NS(name=f'dma<{T},{bm}x{bn},{w},{st}st>', BM=bm, BN=bn, BK=bk, ST=st, dma=True,
              tn2=variant in (8, 24, 27, 33, 50) or (variant == 3 and dtype != BF16))


# ------------------------------------------------------------------------------------------------ cases

def _case(name, dtype, variant, M, N, K, *, entry='ex', a_f32=None, data='rand', bias=False, act=ACT_NONE, res=False, out_bf16=False, C2=False, dup=False,
          stats=False, scatter=False, ln=0, gather=False, trig=None, w_tight=False, splits=0, tile=0):
    """entry: 'ex' (pk_gemm_ex with the explicit variant) | 'gemm' (pk_gemm: `variant` is what it must resolve to) | 'splitk'; trig: the scalar epilogue's
    trigger, None | 'n' (N % 4 != 0) | 'ldc' (odd ldc) | 'c_off' (C 4 bytes off) | 'bias_off' | 'ldr' (ldr % 4 != 0)"""
    a_f32 = (dtype != BF16) if a_f32 is None else a_f32
    assert trig in (None, 'n', 'ldc', 'c_off', 'bias_off', 'ldr') and (trig == 'n') == (N % 4 != 0)
    assert (trig != 'bias_off' or bias) and (trig != 'ldr' or res) and not (out_bf16 and dtype != BF16)
    return NS(name=name, dtype=dtype, variant=variant, M=M, N=N, K=K, entry=entry, a_f32=a_f32, data=data, bias=bias, act=act, res=res, out_bf16=out_bf16,
              C2=C2, dup=dup, stats=stats, scatter=scatter, ln=ln, gather=gather, trig=trig, w_tight=w_tight, splits=splits, tile=tile)


def vec_ok(c):
    return c.N % 4 == 0 and c.trig is None


def form_of(c):
    """host mirror of pk_gemm_epilogue_form under the default cache policy with the hot forms on"""
    if c.entry != 'ex' or c.dtype != BF16 or not vec_ok(c) or c.bias or c.scatter or c.dup:
        return 0
    if c.variant == 8 and c.ln == 0 and c.act == ACT_NONE and not c.out_bf16 and c.res:
        return (1 if c.C2 else 0) if c.stats else (2 if c.C2 else 3)
    if c.variant == 24 and c.ln == 2 and c.act == ACT_GEGLU and c.out_bf16 and not c.res and not c.C2 and not c.stats:
        return 4
    return 0


def lp_of(c):
    if c.entry == 'splitk':
        b = (64, 128, 256)[c.tile]
        return NS(name=f'splitk<{TNAME[c.dtype]},{b}x{b}>', BM=b, BN=b, BK=64 if c.dtype == BF16 else 32, ST=2, tn2=False, dma=True)
    return loop_of(c.dtype, c.variant, c.a_f32, c.ln)


def branch_of(c):
    lp = lp_of(c)
    if c.entry == 'splitk':
        return lp.name
    pre = '' if c.entry == 'ex' else ('pk_gemm[gather]:' if c.gather else 'pk_gemm:')
    f = form_of(c)
    epi = 'scalar' if not vec_ok(c) else ('vec' if not f else f'form<{EPI_NAME[f]}>/{"full" if c.M % lp.BM == 0 and c.N % lp.BN == 0 else "edge"}')
    return f'{pre}{lp.name}/{epi}'


def options(c):
    """the atoms of the pair-coverage check"""
    o = {k for k in ('bias', 'res', 'out_bf16', 'C2', 'dup', 'stats', 'scatter') if getattr(c, k)}
    if c.act:
        o.add(ANAME[c.act])
    if c.ln:
        o.add(f'ln{c.ln}')
    return o


def legal(o):
    """gemm_ex's refusals among the options of the vector epilogue (bf16, an LDS-DMA loop with TN = 2, 64x64 or 128x128)"""
    acts = o & {'geglu', 'leaky', 'relu'}
    lns = o & {'ln1', 'ln2'}
    if len(acts) > 1 or len(lns) > 1:
        return False
    if 'geglu' in o and o & {'res', 'C2', 'scatter', 'stats', 'dup'}:
        return False
    if 'C2' in o and o & {'out_bf16', 'scatter'}:
        return False
    if 'scatter' in o and o & {'out_bf16', 'res', 'stats', 'dup'}:
        return False
    if 'dup' in o and 'stats' in o:
        return False
    if 'ln2' in o and 'stats' in o:
        return False
    return True


OPTION_ATOMS = ('bias', 'leaky', 'relu', 'geglu', 'res', 'out_bf16', 'C2', 'dup', 'stats', 'scatter', 'ln1', 'ln2')

# the covering list of the vector epilogue (every legal pair of OPTION_ATOMS appears in one: asserted by the host test)
VEC_COMBOS = (
    dict(),
    dict(bias=True, act=ACT_LEAKY, res=True, C2=True, stats=True),
    dict(bias=True, act=ACT_RELU, res=True, C2=True, dup=True),
    dict(bias=True, act=ACT_LEAKY, dup=True, out_bf16=True, res=True),
    dict(bias=True, act=ACT_RELU, scatter=True),
    dict(act=ACT_LEAKY, scatter=True),
    dict(bias=True, act=ACT_GEGLU),
    dict(act=ACT_GEGLU, out_bf16=True),
    dict(out_bf16=True),
    dict(act=ACT_LEAKY, out_bf16=True, res=True),
    dict(bias=True, act=ACT_RELU, out_bf16=True, stats=True, res=True),
    dict(act=ACT_RELU, res=True, stats=True),
    dict(res=True, C2=True, stats=True),
    dict(res=True, C2=True),
    dict(res=True),
    dict(act=ACT_RELU, dup=True, out_bf16=True),
)
LN_COMBOS = (
    dict(act=ACT_GEGLU, out_bf16=True),
    dict(bias=True, act=ACT_GEGLU),
    dict(bias=True, act=ACT_LEAKY, res=True),
    dict(act=ACT_RELU, res=True, C2=True, dup=True),
    dict(bias=True, scatter=True),
    dict(out_bf16=True, act=ACT_RELU, dup=True),
    dict(res=True, stats=True, C2=True, act=ACT_LEAKY),
    dict(out_bf16=True, stats=True, bias=True),
    dict(act=ACT_LEAKY, scatter=True),
    dict(act=ACT_RELU, scatter=True),
    dict(act=ACT_LEAKY, out_bf16=True, dup=True),
)


def _combo_ok(dtype, lp, kw, ln=0):
    if (kw.get('out_bf16') or kw.get('C2')) and dtype != BF16:
        return False
    if kw.get('stats') and (not lp.tn2 or ln == 2):
        return False
    return True


def _tag(kw):
    parts = [ANAME[kw.get('act', 0)]] + [k for k in ('bias', 'res', 'out_bf16', 'C2', 'dup', 'stats', 'scatter') if kw.get(k)]
    return '+'.join(parts)


def _piece(dtype):
    return 8 if dtype == BF16 else 4


def _grid(dtype, k):
    return 'grid' if dtype != BF16X3 else ('gridA', 'gridW')[k % 2]


def main_loops():
    """(dtype, variant, a_f32) of every plain main loop of gemm_ex"""
    out = [(dt, v, dt != BF16) for dt in (F32, BF16, BF16X3) for v in VARIANTS[dt]]
    return out + [(BF16, 1, True), (BF16, 2, True)]


def loop_id(dt, v, a_f32):
    return f'{TNAME[dt]}{"_af32" if dt == BF16 and a_f32 else ""}_v{v}'


def shape_cases(dt, v, a_f32):
    """the M x N cross at one K (with a tail), the K list at one edge (M, N) on both data sets, and the tile-map conditions"""
    lp, p, tag = loop_of(dt, v, a_f32), _piece(dt), loop_id(dt, v, a_f32)
    BM, BN, BK, ST = lp.BM, lp.BN, lp.BK, lp.ST
    kw = dict(a_f32=a_f32, bias=True, res=True)
    out, k = [], 0
    for M in (1, BM - 1, BM, BM + 1, 2 * BM + 3):
        for N in (4, BN - 4, BN, BN + 4):
            out.append(_case(f'{tag}_cross_m{M}_n{N}', dt, v, M, N, BK + p, data=_grid(dt, k) if k % 2 == 0 else 'rand', **kw))
            k += 1
    for K in dict.fromkeys((p, BK - p, BK, BK + p, (ST - 1) * BK, (ST + 2) * BK + p)):      # (a 2-stage ring is primed by one k-tile)
        for data in (_grid(dt, k), 'rand'):
            out.append(_case(f'{tag}_k{K}_{data}', dt, v, BM + 1, BN + 4, K, data=data, **kw))
        k += 1
    out.append(_case(f'{tag}_gather', dt, v, BM + 1, BN + 4, BK + p, data='rand', gather=True, **kw))
    if lp.dma:
        esz = 2 if dt == BF16 else 4
        out.append(_case(f'{tag}_mt9', dt, v, 8 * BM + 5, BN + 4, BK + p, data=_grid(dt, 0), **kw))                     # cmax = 2, uneven chunks
        out.append(_case(f'{tag}_panel', dt, v, 33 * BM + 1, BN + 4, (256 << 10) // (esz * BM), data=_grid(dt, 1), **kw))  # panel 4 < cmax 5, a last panel of 1
        out.append(_case(f'{tag}_krot', dt, v, BM + 6, 8196, 3 * BK + p, data=_grid(dt, 0), **kw))                     # N >= 8192: rotated k-tile order
    return out


SCALAR_FULL = {(F32, 8), (BF16, 8), (BF16X3, 8), (F32, 1), (BF16, 50)}


def epilogue_cases(dt, v, a_f32):
    """the covering list of the vector epilogue and the scalar epilogue at one edge shape"""
    lp, p, tag = loop_of(dt, v, a_f32), _piece(dt), loop_id(dt, v, a_f32)
    M, N, K = lp.BM + 1, lp.BN + 4, lp.BK + p
    out = []
    for k, kw in enumerate(VEC_COMBOS):
        if _combo_ok(dt, lp, kw):
            out.append(_case(f'{tag}_vec_{_tag(kw)}', dt, v, M, N, K, a_f32=a_f32, data='rand' if k % 3 else _grid(dt, k), **kw))
    for k, (Ns, act, res) in enumerate(((1, ACT_NONE, True), (2, ACT_GEGLU, False), (3, ACT_LEAKY, False), (6, ACT_RELU, True))):
        out.append(_case(f'{tag}_scalar_n{Ns}', dt, v, M, Ns, K, a_f32=a_f32, data='rand' if k % 2 else _grid(dt, k), bias=True, act=act, res=res, trig='n'))
    if (dt, v) in SCALAR_FULL and not (dt == BF16 and v == 1):
        k = 0
        for act in (ACT_NONE, ACT_GEGLU, ACT_LEAKY, ACT_RELU):
            for res in (False, True):
                if act == ACT_GEGLU and res:
                    continue
                for ob in ((False, True) if dt == BF16 else (False,)):
                    Ns = (6, 2)[k % 2] if act == ACT_GEGLU else (1, 2, 3, 6)[k % 4]
                    out.append(_case(f'{tag}_scalarfull_{ANAME[act]}{"_res" if res else ""}{"_bf16" if ob else ""}', dt, v, M, Ns, K, a_f32=a_f32,
                                     data='rand' if k % 2 else _grid(dt, k), bias=k % 3 != 0, act=act, res=res, out_bf16=ob, trig='n'))
                    k += 1
        for k, (trig, kw) in enumerate((('ldc', dict(act=ACT_LEAKY)), ('c_off', dict(res=True)), ('bias_off', dict(bias=True, act=ACT_RELU)),
                                        ('ldr', dict(res=True, bias=True)), ('ldc', dict(act=ACT_GEGLU, bias=True)))):
            out.append(_case(f'{tag}_scalartrig_{trig}_{ANAME[kw.get("act", 0)]}', dt, v, M, N, K, a_f32=a_f32, data='rand' if k % 2 else _grid(dt, k),
                             trig=trig, **kw))
    return out


def ln_loops():
    return [(dt, v, ln) for dt in (F32, BF16, BF16X3) for v in (8, 24) for ln in (1, 2)]


def ln_cases(dt, v, ln):
    """in-loop statistics on a K tail and a wrapped ring; handed-over statistics at K = 72, 96, 512, 544 (3, 3, 16, 17 partials: the last one enters the
    un-prefetched loop), 4 threads per row (64x64, 8-wave 128x128) and 2 (the 4-wave 128x128 tile of split-bf16)"""
    lp, p = loop_of(dt, v, dt != BF16, ln), _piece(dt)
    tag = f'{TNAME[dt]}_v{v}_ln{ln}'
    M, N = lp.BM + 1, lp.BN + 4
    out = []
    Ks = (lp.BK + p, 4 * lp.BK + p) if ln == 1 else (72, 96, 512, 544)
    for k, kw in enumerate(LN_COMBOS):
        if _combo_ok(dt, lp, kw, ln):
            out.append(_case(f'{tag}_{_tag(kw)}_k{Ks[k % len(Ks)]}', dt, v, M, N, Ks[k % len(Ks)], ln=ln, **kw))
    for K in Ks:
        for M2, N2 in ((lp.BM, lp.BN), (2 * lp.BM + 3, lp.BN - 4)):
            out.append(_case(f'{tag}_plain_m{M2}_n{N2}_k{K}', dt, v, M2, N2, K, ln=ln))
    return out


def form_cases():
    """OUT, FF2A, FF2B (bf16 variant 8) and FF1 (variant 24, handed-over statistics), each on full tiles only and with edge tiles"""
    out = []
    for name, v, kw in (('OUT', 8, dict(res=True, C2=True, stats=True)), ('FF2A', 8, dict(res=True, C2=True)), ('FF2B', 8, dict(res=True)),
                        ('FF1', 24, dict(act=ACT_GEGLU, out_bf16=True, ln=2))):
        b = 64 if v == 8 else 128
        for M, N in ((2 * b, b), (b + 1, b + 4), (b - 1, 2 * b)):
            for K, data in ((72, 'rand'), (512, 'rand')) + ((() if name == 'FF1' else ((136, 'grid'),))):
                out.append(_case(f'form_{name}_m{M}_n{N}_k{K}_{data}', BF16, v, M, N, K, data=data, **kw))
    return out


def pk_gemm_cases():
    """pk_gemm: the register-staged loops it falls back to (f32 A in bf16 mode; a W without the k-tile padding; a gather, whose row count it synthesises), 64x64
    and -- from 384 tiles of 128x128 on -- 128x128"""
    out = []
    for dt, a_f32, tight in ((F32, True, True), (BF16, False, True), (BF16, True, False)):
        tag = loop_id(dt, 1, a_f32).rsplit('_v', 1)[0]
        p, bk = _piece(dt), 64 if dt == BF16 else 32
        for v, M, N, K in ((1, 65, 68, bk + p), (2, 23 * 128 + 1, 16 * 128 + 4, 2 * p)):
            for gather in (False, True):
                for k, data in enumerate((_grid(dt, 0), 'rand')):
                    if v == 2 and k != int(gather):        # the large shape: the grid without, random data with the gather
                        continue
                    out.append(_case(f'pkgemm_{tag}_v{v}{"_gather" if gather else ""}_{data}', dt, v, M, N, K, entry='gemm', a_f32=a_f32, data=data, bias=True,
                                     res=True, act=ACT_RELU if k else ACT_NONE, gather=gather, w_tight=tight))
    return out


def splitk_cases():
    out = []
    for dt in (F32, BF16, BF16X3):
        bk = 64 if dt == BF16 else 32
        for tile in ((0, 1, 2) if dt == BF16 else (0, 1)):
            b = (64, 128, 256)[tile]
            for splits in (1, 3):
                for k, (M, N) in enumerate(((b + 1, b + 4), (2 * b + 3, b - 4), (b - 1, 4))):
                    for data in (_grid(dt, k), 'rand'):
                        out.append(_case(f'splitk_{TNAME[dt]}_t{tile}_s{splits}_m{M}_n{N}_{data}', dt, 0, M, N, splits * bk * (1 + k), entry='splitk', data=data,
                                         bias=k != 1, splits=splits, tile=tile))
    return out


def grouped_cases():
    """pytest id -> cases: one id per main loop for its shape list, one for its epilogue list"""
    out = {}
    for dt, v, a in main_loops():
        out[loop_id(dt, v, a) + '_shapes'] = [c for c in shape_cases(dt, v, a) if 2.0 * c.M * c.N * c.K <= 2e8]
        out[loop_id(dt, v, a) + '_tilemap'] = [c for c in shape_cases(dt, v, a) if 2.0 * c.M * c.N * c.K > 2e8]
        out[loop_id(dt, v, a) + '_epilogues'] = epilogue_cases(dt, v, a)
    for dt, v, ln in ln_loops():
        out[f'{TNAME[dt]}_v{v}_ln{ln}'] = ln_cases(dt, v, ln)
    out['forms'] = form_cases()
    out['pk_gemm'] = pk_gemm_cases()
    for c in splitk_cases():
        out.setdefault(f'splitk_{TNAME[c.dtype]}', []).append(c)
    return {k: v for k, v in out.items() if v}


def all_cases():
    return [c for cs in grouped_cases().values() for c in cs]


def expected_branches():
    """written out from the switch tables of gemm_ex, pk_gemm and pk_gemm_splitk"""
    want = set()
    reg = [f'reg<{t},{ta},{b}x{b}>' for t, ta in (('f32', 'f32'), ('bf16', 'bf16'), ('bf16', 'f32')) for b in (64, 128)]
    dma = [f'dma<f32,{g}>' for g in ('64x64,4w,4st', '64x64,4w,2st', '128x128,4w,2st', '128x128,8w,2st')]
    dma += [f'dma<bf16,{g}>' for g in ('64x64,4w,2st', '128x128,4w,2st', '128x128,8w,2st', '128x64,4w,2st', '64x64,4w+2p,3st', '256x256,p8,2st')]
    dma += [f'dma<x3,{g}>' for g in ('64x64,4w,4st', '64x64,4w,2st', '128x128,4w,2st', '128x128,8w,2st', '128x64,4w,2st')]
    for name in reg + dma:
        want |= {f'{name}/vec', f'{name}/scalar'}
    for name in reg:
        want |= {f'pk_gemm:{name}/vec', f'pk_gemm[gather]:{name}/vec'}
    for ln in (1, 2):
        want |= {f'dma<{t},64x64,4w,2st,ln{ln}>/vec' for t in ('f32', 'bf16', 'x3')}
        want |= {f'dma<f32,128x128,8w,2st,ln{ln}>/vec', f'dma<bf16,128x128,8w,2st,ln{ln}>/vec', f'dma<x3,128x128,4w,2st,ln{ln}>/vec'}
    want |= {f'dma<bf16,64x64,4w,2st>/form<{f}>/{e}' for f in ('OUT', 'FF2A', 'FF2B') for e in ('full', 'edge')}
    want |= {f'dma<bf16,128x128,8w,2st,ln2>/form<FF1>/{e}' for e in ('full', 'edge')}
    want |= {f'splitk<{t},{b}x{b}>' for t in ('f32', 'bf16', 'x3') for b in (64, 128)} | {'splitk<bf16,256x256>'}
    return want


# ------------------------------------------------------------------------------------------------ geometry and inputs

def geometry(c):
    lp = lp_of(c)
    g = NS(lp=lp)
    g.q = _piece(c.dtype)
    g.qa = 8 if (c.dtype == BF16 and not c.a_f32) else 4
    g.kpad = ceil_to(c.K, lp.BK)
    g.lda = c.K + 2 * g.qa
    g.ldw = c.K if c.w_tight else g.kpad + g.q
    g.NC = c.N // 2 if c.act == ACT_GEGLU else c.N
    n4 = ceil_to(g.NC, 4)
    g.ldc = g.NC + 5 if c.trig == 'ldc' else (g.NC + 3 if c.trig == 'n' else n4 + 8)
    g.coff = (2 if c.out_bf16 else 1) if c.trig == 'c_off' else 0
    g.ldr = c.N + 5 if c.trig == 'ldr' else (c.N + 7 if c.trig == 'n' else ceil_to(c.N, 4) + 4)
    g.ldc2 = ceil_to(c.N, 4) + 12
    g.dup = c.M + 3 if c.dup else 0
    g.RC = c.splits * c.M if c.entry == 'splitk' else g.dup + c.M
    g.ldS = c.N + 8                                        # row pitch of the scatter target
    g.np_out, g.np_in = -(-c.N // 32), -(-c.K // 32)
    g.boff = 1 if c.trig == 'bias_off' else 0
    g.rowsA = c.M + (9 if c.gather else 5)
    assert g.ldr != g.ldc and g.ldc2 != g.ldc and g.lda > c.K and g.ldc > g.NC
    return g


def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def bf(t):
    return t.to(torch.bfloat16).to(t.dtype)


def split_planes(w32):
    """the pre-split W image of split-bf16 (as _lib.split_planes: per block of 32 k-elements [hi x 32 | lo x 32], an f32-typed tensor of raw bits)"""
    n, k = w32.shape
    hi = w32.to(torch.bfloat16)
    lo = (w32 - hi.float()).to(torch.bfloat16)
    return torch.cat((hi.view(n, k // 32, 32), lo.view(n, k // 32, 32)), dim=-1).contiguous().view(n, 2 * k).view(torch.float32)


def build(c, poison=NAN):
    """the seeded operands of a case as CPU f32 tensors: the logical A (M, K), W (N, K), bias, res, ln vectors, and the physical buffers around them"""
    g, geo = _gen(c.name), geometry(c)
    M, N, K = c.M, c.N, c.K
    P = geo.rowsA
    x = NS(geo=geo, a_rows=None)
    if c.data == 'rand':
        Ap = torch.randn(P, K, generator=g) + (0.5 if c.ln else 0.0)
        if P >= 8:
            sc = torch.ones(P, 1)
            sc[3::8], sc[5::8] = 1e3, 1e-3
            Ap = Ap * sc
        W = torch.randn(N, K, generator=g) / math.sqrt(K)
        bias, res = torch.randn(N, generator=g), torch.randn(M, N, generator=g)
        x.step = None
    else:
        sa, sw = (2.0 ** -6 if c.data == 'gridA' else 1.0), (2.0 ** -10 if c.data == 'gridW' else 2.0 ** -4)
        Ap = torch.randint(-int(8 / sa), int(8 / sa) + 1, (P, K), generator=g).float() * sa
        W = torch.randint(-int(1 / sw), int(1 / sw) + 1, (N, K), generator=g).float() * sw
        bias, res = torch.randint(-64, 65, (N,), generator=g).float() / 16, torch.randint(-64, 65, (M, N), generator=g).float() / 16
        x.step = sa * sw
    if c.dtype == BF16:
        W = bf(W)
        if not c.a_f32:
            Ap = bf(Ap)
    x.A_buf = torch.full((P, geo.lda), poison)
    if c.gather:
        src = torch.randperm(P, generator=g)[:max(1, M - M // 4)]                    # fewer rows than M: repeats; the others stay poisoned
        x.a_rows = src[torch.randint(0, src.numel(), (M,), generator=g)].to(torch.int32)
        used = x.a_rows.long().unique()
        x.A_buf[used, :K] = Ap[used]
        x.A = Ap[x.a_rows.long()]
    else:
        x.A_buf[:M, :K] = Ap[:M]
        x.A = Ap[:M].clone()
    x.W = W
    x.W_buf = torch.full((N + 3, geo.ldw), poison)
    x.W_buf[:N, :min(geo.kpad, geo.ldw)] = 0.0
    x.W_buf[:N, :K] = W
    x.bias = bias if c.bias else None
    x.bias_buf = torch.full((N + 9,), poison)
    x.bias_buf[geo.boff:geo.boff + N] = bias
    x.res = res if c.res else None
    x.res_buf = torch.full((M + 3, geo.ldr), poison)
    x.res_buf[:M, :N] = res
    if c.ln:
        x.ln_t = torch.randn(N, generator=g) * 0.5
        x.ln_s = W.double().sum(1).float()
        x.s_buf, x.t_buf = torch.full((N + 8,), poison), torch.full((N + 8,), poison)
        x.s_buf[:N], x.t_buf[:N] = x.ln_s, x.ln_t
        a = torch.zeros(M, geo.np_in * 32, dtype=torch.float64)
        a[:, :K] = x.A.double()
        a = a.view(M, geo.np_in, 32)
        x.stats_in = torch.full((M + 3, geo.np_in, 2), poison)
        x.stats_in[:M] = torch.stack((a.sum(-1), (a * a).sum(-1)), dim=-1).float()
    if c.scatter:
        x.rperm = torch.randperm(M, generator=g)
        x.cperm = (torch.randperm(N // 4, generator=g)[:, None] * 4 + torch.arange(4)[None, :]).reshape(-1)
        x.row_off = ((G + x.rperm) * geo.ldS).to(torch.int32)
        x.col_off = torch.cat((x.cperm, N + torch.arange(8) % 4)).to(torch.int32)         # the tail points into the rows' slack columns: inside the buffer
    if x.step is not None:
        s = x.A.double().abs() @ W.double().abs().t() + (bias.abs() if c.bias else 0) + (res.abs() if c.res else 0)
        assert s.max().item() / x.step < 2 ** 24, f'{c.name}: the grid is not exact in f32 ({s.max().item() / x.step:.3g} steps)'
    return x


def exact(c):
    return c.data != 'rand' and c.act in (ACT_NONE, ACT_RELU) and c.ln == 0


# ------------------------------------------------------------------------------------------------ reference and bound

def gelu64(x):
    return 0.5 * x * (1 + torch.erf(x / math.sqrt(2)))


def reference(c, x, want_bound=None):
    """ref.out (rows, NC) f64; ref.terms: name -> (rows, NC) f64, the first-order terms of the module docstring (None where the exact check applies)"""
    M, N, K = c.M, c.N, c.K
    A = (bf(x.A) if (c.dtype == BF16 and c.a_f32) else x.A).double()
    W = x.W.double()
    want_bound = (not exact(c)) if want_bound is None else want_bound
    split = SPLIT if c.dtype == BF16X3 else 0.0
    if c.entry == 'splitk':
        Kc = K // c.splits
        outs, ts = [], {'accumulate': [], 'split': [], 'epilogue': []}
        for z in range(c.splits):
            a, w = A[:, z * Kc:(z + 1) * Kc], W[:, z * Kc:(z + 1) * Kc]
            v = a @ w.t()
            b = z == 0 and c.bias
            if b:
                v = v + x.bias.double()
            outs.append(v)
            if want_bound:
                S = a.abs() @ w.abs().t()
                ts['accumulate'].append(Kc * U1 * S)
                ts['split'].append(split * S)
                ts['epilogue'].append(U1 * v.abs() if b else torch.zeros_like(v))
        return NS(out=torch.cat(outs), terms={k: torch.cat(v) for k, v in ts.items()} if want_bound else None)
    acc = A @ W.t()
    t = {}
    if want_bound:
        S = A.abs() @ W.abs().t()
        t['accumulate'], t['split'] = K * U1 * S, split * S
    if c.ln:
        geo = x.geo
        mean, var = A.mean(1, keepdim=True), A.var(1, unbiased=False, keepdim=True)
        rstd = 1 / torch.sqrt(var + LN_EPS)
        S64 = W.sum(1)[None, :]
        inner = acc - mean * S64
        v = rstd * inner + x.ln_t.double()[None, :]
        if want_bound:
            sa, sq = A.abs().sum(1, keepdim=True), (A * A).sum(1, keepdim=True)
            if c.ln == 1:
                u_sum = K * U1 + (2.0 ** -16 if c.dtype == BF16X3 else 0.0)
                u_sq = K * U1 + (3 * 2.0 ** -16 if c.dtype == BF16X3 else 0.0)
            else:
                u_sum = u_sq = geo.np_in * U1 + U24
            d_mean = u_sum * sa / K + U1 * mean.abs()
            d_var = u_sq * sq / K + 2 * U1 * sq / K + 2 * mean.abs() * d_mean + d_mean ** 2 + U1 * mean ** 2
            rel_rstd = 0.5 * (d_var + U1 * (var + LN_EPS)) / (var + LN_EPS) + U1
            d_inner = S64.abs() * d_mean + mean.abs() * U24 * S64.abs() + U1 * (mean * S64).abs() + U1 * inner.abs()
            t['accumulate'], t['split'] = rstd * t['accumulate'], rstd * t['split']
            t['ln'] = rstd * d_inner + (rstd * inner).abs() * (rel_rstd + U1) + U1 * v.abs()
    else:
        v = acc
    epi = torch.zeros_like(v)
    if c.bias:
        v = v + x.bias.double()[None, :]
        epi = epi + U1 * v.abs()
    if c.act == ACT_GEGLU:
        val, gate = v[:, 0::2], v[:, 1::2]
        ge = gelu64(gate)
        out = ge * val
        if want_bound:
            t['epilogue'] = epi
            e_all = sum(t.values())
            t = {k: val.abs() * GELU_LIP * e[:, 1::2] + ge.abs() * e[:, 0::2] for k, e in t.items()}
            erf_abs = ERFF_C * U24 if c.dtype == F32 else ERF_FAST_ABS
            t['gelu'] = (val.abs() * (0.5 * gate.abs() * erf_abs + 2 * U1 * ge.abs()) + U1 * out.abs() + GELU_LIP * e_all[:, 0::2] * e_all[:, 1::2])
        return NS(out=out, terms=t if want_bound else None)
    if c.act == ACT_LEAKY:
        v = torch.where(v > 0, v, 0.1 * v)
        epi = epi + (U1 + U24) * v.abs()
    if c.act == ACT_RELU:
        v = v.clamp_min(0)
    if c.res:
        v = v + x.res.double()
        epi = epi + U1 * v.abs()
    if want_bound:
        t['epilogue'] = epi
    return NS(out=v, terms=t if want_bound else None)


# ------------------------------------------------------------------------------------------------ output buffers

def _sentinel(shape, dtype):
    if dtype == torch.float32:
        return torch.full(shape, SENT32, dtype=torch.int32).view(torch.float32)
    return torch.full(shape, SENT16, dtype=torch.int16).view(torch.bfloat16)


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def blank(c, x):
    """the sentinel-filled output buffers of a case"""
    geo, M, N = x.geo, c.M, c.N
    b = {}
    if c.scatter:
        b['C'] = _sentinel((G + M + G, geo.ldS), torch.float32)
    else:
        b['C'] = _sentinel((G + geo.RC + G, geo.ldc), torch.bfloat16 if c.out_bf16 else torch.float32)
    if c.C2:
        b['C2'] = _sentinel((G + geo.RC + G, geo.ldc2), torch.bfloat16)
    if c.stats:
        b['stats'] = _sentinel((G + M + G, 2 * geo.np_out), torch.float32)
    return b


def _row_blocks(c, x):
    return (0, x.geo.dup) if c.dup else (0,)


def regions(c, x, b):
    """name -> bool mask of the elements a correct launch writes"""
    geo, M, N = x.geo, c.M, c.N
    out = {}
    m = torch.zeros(b['C'].shape, dtype=torch.bool)
    if c.scatter:
        m[G:G + M, :N] = True
    elif c.entry == 'splitk':
        m[G:G + geo.RC, :N] = True
    else:
        for r0 in _row_blocks(c, x):
            m[G + r0:G + r0 + M, geo.coff:geo.coff + geo.NC] = True
    out['C'] = m
    if c.C2:
        m = torch.zeros(b['C2'].shape, dtype=torch.bool)
        for r0 in _row_blocks(c, x):
            m[G + r0:G + r0 + M, :N] = True
        out['C2'] = m
    if c.stats:
        m = torch.zeros(b['stats'].shape, dtype=torch.bool)
        m[G:G + M] = True
        out['stats'] = m
    return out


def read_C(c, x, b, r0=0):
    geo = x.geo
    if c.scatter:
        return b['C'][G + x.rperm][:, x.cperm]
    rows = geo.RC if c.entry == 'splitk' else c.M
    return b['C'][G + r0:G + r0 + rows, geo.coff:geo.coff + geo.NC]


def lay_out(c, x, Cv, C2v=None, stats=None, mutant=None):
    """the buffers a launch that computed Cv (rows, NC; the output type), C2v (M, N) bf16 and stats (M, np, 2) f32 leaves -- or a mutant's"""
    geo, M, N = x.geo, c.M, c.N
    b = blank(c, x)
    if c.scatter:
        tmp = torch.empty(M, N)
        tmp[:, x.cperm] = Cv
        b['C'][G + x.rperm, :N] = tmp
    else:
        for r0 in _row_blocks(c, x):
            r = M if (mutant == 'dup_at_M' and r0) else r0
            b['C'][G + r:G + r + Cv.shape[0], geo.coff:geo.coff + geo.NC] = Cv
    if c.C2:
        for r0 in _row_blocks(c, x):
            if mutant == 'c2_ldc':                        # the C2 rows laid down with C's pitch
                flat = b['C2'].view(-1)
                idx = (G * geo.ldc2 + (r0 + torch.arange(M))[:, None] * geo.ldc + torch.arange(N)[None, :]).reshape(-1)
                flat[idx] = C2v.reshape(-1)
            else:
                r = M if (mutant == 'dup_at_M' and r0) else r0
                b['C2'][G + r:G + r + M, :N] = C2v
    if c.stats:
        st = stats.reshape(M, 2 * geo.np_out)
        if mutant == 'stats_chunk_off1':
            b['stats'][G:G + M, 2:] = st[:, :-2]
        else:
            b['stats'][G:G + M] = st
    if mutant == 'store_slack':
        b['C'][G, geo.ldS - 1 if c.scatter else geo.coff + geo.NC] = 1.0
    if mutant == 'store_guard':
        b['C'][G - 1, 0] = 1.0
    if mutant == 'store_guard_behind':
        b['C'][-G, 0] = 1.0
    return b


def consumer_values(c, Cf):
    """the rows as the LayerNorm-folded consumer reads them (gemm_epilogue_vec: the bf16 rounding when there is a C2 or a bf16 C)"""
    return bf(Cf.float()) if (c.dtype == BF16 and (c.C2 or c.out_bf16)) else Cf.float()


def chunk_sums(c, x, xs, dtype=torch.float64):
    geo = x.geo
    a = torch.zeros(c.M, geo.np_out * 32, dtype=dtype)
    a[:, :c.N] = xs.to(dtype)
    a = a.view(c.M, geo.np_out, 32)
    return torch.stack((a.sum(-1), (a * a).sum(-1)), dim=-1), torch.stack((a.abs().sum(-1), (a * a).sum(-1)), dim=-1)


def ideal_outputs(c, x, ref):
    """what a kernel with exactly the reference's values would leave: rounded once to the output type"""
    Cv = ref.out.float().to(torch.bfloat16 if c.out_bf16 else torch.float32)
    C2v = Cv.to(torch.bfloat16) if c.C2 else None
    stats = chunk_sums(c, x, consumer_values(c, Cv))[0].float() if c.stats else None
    return lay_out(c, x, Cv, C2v, stats)


def check(c, x, ref, b, what=None):
    """every assertion of the module docstring on the buffers `b` a launch left.  Returns name -> (largest err / bound, dominating term)"""
    what = what or c.name
    geo, M, N = x.geo, c.M, c.N
    assert set(b) == set(blank(c, x)), f'{what}: buffers {sorted(b)}'
    for name, mask in regions(c, x, b).items():
        buf = b[name]
        assert buf.shape == mask.shape
        sent = SENT32 if buf.dtype == torch.float32 else SENT16
        touched = (_bits(buf) != sent) & ~mask
        assert not touched.any(), (f'{what}: {int(touched.sum())} stores outside the result region of {name} (guard rows / slack columns), first at '
                                   f'{touched.nonzero()[0].tolist()} of {tuple(buf.shape)}')
        bad = ~torch.isfinite(buf.float()) & mask
        assert not bad.any(), f'{what}: {int(bad.sum())} non-finite / unwritten elements in {name}, first at {bad.nonzero()[0].tolist()}'
    Cv = read_C(c, x, b)
    got = Cv.double()
    assert got.shape == ref.out.shape, f'{what}: {tuple(got.shape)} vs {tuple(ref.out.shape)}'
    res = {}
    if ref.terms is None:
        want = ref.out.float()
        assert torch.equal(want.double(), ref.out), f'{what}: the grid reference is not an f32 value'
        want = want.to(Cv.dtype)
        bad = want.double() != got
        if bad.any():
            r, col = bad.nonzero()[0].tolist()
            raise AssertionError(f'{what}: exact grid: element ({r}, {col}) is {got[r, col]:.9g}, the reference rounded once is {want[r, col].item():.9g}; '
                                 f'{int(bad.sum())} elements differ')
        res['C'] = (0.0, 'exact')
    else:
        names = list(ref.terms)
        bnd = sum(ref.terms.values()) + 1e-45
        err = (got - ref.out).abs()
        if c.out_bf16:
            lo = torch.nextafter((ref.out - bnd).float(), torch.tensor(-INF)).to(torch.bfloat16).double()
            hi = torch.nextafter((ref.out + bnd).float(), torch.tensor(INF)).to(torch.bfloat16).double()
            bad = (got < lo) | (got > hi)
            # on record: the share of the f32 bound the value needs -- the distance from the reference to the f32 values that round to it
            ratio = (err - 2.0 ** -8 * torch.exp2(torch.floor(torch.log2(got.abs().clamp_min(1e-300))))).clamp_min(0) / bnd
        else:
            ratio = err / bnd
            bad = ratio > 1
        k = int(ratio.argmax())
        r, col = divmod(k, got.shape[1])
        if bad.any():
            r, col = bad.nonzero()[0].tolist()
            raise AssertionError(f'{what}: element ({r}, {col}) is {got[r, col]:.9g}, reference {ref.out[r, col]:.9g}: error {err[r, col]:.3e} = '
                                 f'{(err[r, col] / bnd[r, col]):.2f} x bound {bnd[r, col]:.3e}; {int(bad.sum())} elements beyond their bound')
        res['C'] = (ratio.max().item(), max(names, key=lambda n: ref.terms[n][r, col].item()))
    if c.dup:
        assert torch.equal(_bits(read_C(c, x, b, geo.dup)), _bits(Cv)), f'{what}: the dup_rows copy of C differs from the original rows'
    if c.C2:
        C2v = b['C2'][G:G + M, :N]
        assert torch.equal(_bits(C2v), _bits(Cv.to(torch.bfloat16))), f'{what}: C2 is not the round-to-nearest-even bf16 of C'
        if c.dup:
            assert torch.equal(_bits(b['C2'][G + geo.dup:G + geo.dup + M, :N]), _bits(C2v)), f'{what}: the dup_rows copy of C2 differs'
        res['C2'] = (0.0, 'exact')
    if c.stats:
        want, mag = chunk_sums(c, x, consumer_values(c, Cv))
        st = b['stats'][G:G + M].view(M, geo.np_out, 2).double()
        ratio = (st - want).abs() / (STATS_ULPS * U24 * mag + 1e-45)
        assert ratio.max().item() <= 1, (f'{what}: stats_out {ratio.max().item():.2f} x bound at (row, chunk, sum | sumsq) '
                                         f'{[int(i) for i in torch.unravel_index(ratio.argmax(), ratio.shape)]}')
        res['stats'] = (ratio.max().item(), 'chunk sum')
    return res


# ------------------------------------------------------------------------------------------------ the honest f32 emulation and its mutants

MUTANTS = ('drop_last_piece', 'drop_last_ktile', 'first_ktile_twice', 'k_tail_not_cut', 'a_rows_ge_M', 'gather_ignored', 'bias_shift', 'clamped_read',
           'res_before_act', 'leaky_001', 'geglu_swapped', 'geglu_halves', 'c2_before_res', 'c2_ldc', 'dup_at_M', 'stats_unrounded', 'stats_chunk_off1',
           'ln_unbiased', 'ln_eps_outside', 'store_slack', 'store_guard', 'store_guard_behind', 'cut_mantissa', 'x3_drop_hilo')


def applies(m, c):
    """the worst-case bound grows with K, so the mutants that move a value by a relative 1 / K or by the low mantissa bits are asked for at K <= 96 only"""
    geo = geometry(c)
    sk = c.entry == 'splitk'
    rounded = c.dtype == BF16 and (c.C2 or c.out_bf16)
    return {'drop_last_piece': True, 'drop_last_ktile': True, 'first_ktile_twice': True,
            'k_tail_not_cut': c.K % geo.lp.BK != 0 and not c.w_tight,
            'a_rows_ge_M': not c.gather, 'gather_ignored': c.gather,
            'bias_shift': c.bias, 'clamped_read': (c.bias or c.res) and c.N >= 8 and not sk,
            'res_before_act': c.res and c.act != ACT_NONE, 'leaky_001': c.act == ACT_LEAKY,
            'geglu_swapped': c.act == ACT_GEGLU, 'geglu_halves': c.act == ACT_GEGLU and c.N >= 4,
            'c2_before_res': c.C2 and c.res, 'c2_ldc': c.C2, 'dup_at_M': c.dup,
            'stats_unrounded': c.stats and rounded and c.data == 'rand', 'stats_chunk_off1': c.stats,
            'ln_unbiased': c.ln and c.K <= 96, 'ln_eps_outside': c.ln and c.K <= 96 and c.M >= 8,
            'store_slack': True, 'store_guard': True, 'store_guard_behind': True,
            'cut_mantissa': c.data == 'rand' and c.K <= 96 and c.dtype != BF16 and c.K >= 16,
            'x3_drop_hilo': c.dtype == BF16X3 and c.data in ('rand', 'gridW')}[m]


def _cut10(t):
    return (t.view(torch.int32) & ~0x1FFF).view(torch.float32)


def gelu_fast32(x):
    """common.hpp gelu_erf_fast in f32 (Abramowitz-Stegun 7.1.26)"""
    z = x.abs() * 0.70710678118654752440
    t = 1.0 / (0.3275911 * z + 1.0)
    p = 1.061405429 * t - 1.453152027
    p = p * t + 1.421413741
    p = p * t - 0.284496736
    p = p * t + 0.254829592
    erfz = 1.0 - p * t * torch.exp(-z * z)
    return 0.5 * x * (1.0 + torch.copysign(erfz, x))


def gelu32(c, x):
    return 0.5 * x * (1.0 + torch.erf(x * 0.70710678118654752440)) if c.dtype == F32 else gelu_fast32(x)


def _mm32(c, A, W, mutant):
    if c.dtype != BF16X3:
        return A @ W.t()
    Ah, Wh = bf(A), bf(W)
    Al, Wl = bf(A - Ah), bf(W - Wh)
    acc = Ah @ Wh.t() + Al @ Wh.t()
    return acc if mutant == 'x3_drop_hilo' else acc + Ah @ Wl.t()


def emulate(c, x, order='natural', mutant=None):
    """a torch f32 product (natural or permuted k order) of what the PHYSICAL buffers hold where the kernel reads them, the epilogue in f32 in the kernel's
    order, laid out like a launch.  `mutant`: one planted defect."""
    geo, M, N, K = x.geo, c.M, c.N, c.K
    lp = geo.lp
    rows = torch.arange(M) if (x.a_rows is None or mutant == 'gather_ignored') else x.a_rows.long()
    if mutant == 'a_rows_ge_M':
        rows = rows.clone()
        rows[-1] = M
    Kr = min(geo.kpad, geo.lda, geo.ldw) if mutant == 'k_tail_not_cut' else K
    A, W = x.A_buf[rows, :Kr], x.W_buf[:N, :Kr]
    if c.dtype == BF16 and c.a_f32:
        A = bf(A)
    if mutant == 'cut_mantissa':
        A, W = _cut10(A.contiguous()), _cut10(W.contiguous())

    def product(k0, k1):
        a, w = A[:, k0:k1], W[:, k0:k1]
        if order == 'permuted':
            p = torch.randperm(k1 - k0, generator=_gen(c.name + 'perm'))
            a, w = a[:, p], w[:, p]
        return _mm32(c, a.contiguous(), w.contiguous(), mutant)

    stats_in = x.stats_in[:M] if c.ln == 2 else None
    outs = []
    for z in range(max(c.splits, 1)):
        Kc = K // c.splits if c.splits else Kr
        k0 = z * Kc
        acc = product(k0, k0 + Kc)
        nt = -(-Kc // lp.BK)
        if mutant == 'drop_last_piece':
            acc = acc - _mm32(c, A[:, k0 + Kc - geo.q:k0 + Kc], W[:, k0 + Kc - geo.q:k0 + Kc], None)
        if mutant == 'drop_last_ktile':
            acc = acc - _mm32(c, A[:, k0 + (nt - 1) * lp.BK:k0 + Kc], W[:, k0 + (nt - 1) * lp.BK:k0 + Kc], None)
        if mutant == 'first_ktile_twice':
            acc = acc + _mm32(c, A[:, k0:k0 + min(lp.BK, Kc)], W[:, k0:k0 + min(lp.BK, Kc)], None)
        outs.append(acc)
    v = torch.cat(outs)
    one = torch.ones((), dtype=torch.float32)
    if c.ln:
        if c.ln == 1:
            rsum, rsq = A.sum(1), (A * A).sum(1)
        else:
            rsum, rsq = stats_in[:, :, 0].sum(1), stats_in[:, :, 1].sum(1)
        inv_k = one / K
        mean = rsum * inv_k
        var = (rsq * inv_k - mean * mean).clamp_min(0)
        if mutant == 'ln_unbiased':
            var = var * (K / (K - 1))
        rstd = one / (var.sqrt() + LN_EPS) if mutant == 'ln_eps_outside' else one / (var + LN_EPS).sqrt()
        v = rstd[:, None] * (v - mean[:, None] * x.s_buf[:N][None, :]) + x.t_buf[:N][None, :]
    cols = torch.arange(N)
    if mutant == 'clamped_read':
        cols = torch.cat((cols[:N - 4], cols[N - 8:N - 4]))
    if c.bias:
        off = geo.boff + (1 if mutant == 'bias_shift' else 0)
        bvec = x.bias_buf[off + cols]
        if c.splits:
            v[:M] = v[:M] + bvec[None, :]
        else:
            v = v + bvec[None, :]
    resv = x.res_buf[:M][:, cols] if c.res else None
    if mutant == 'res_before_act':
        v = v + resv
    pre = v
    if c.act == ACT_GEGLU:
        val, gate = (v[:, :N // 2], v[:, N // 2:]) if mutant == 'geglu_halves' else (v[:, 0::2], v[:, 1::2])
        if mutant == 'geglu_swapped':
            val, gate = gate, val
        v = gelu32(c, gate) * val
    elif c.act == ACT_LEAKY:
        v = torch.where(v > 0, v, (0.01 if mutant == 'leaky_001' else 0.1) * v)
    elif c.act == ACT_RELU:
        v = v.clamp_min(0)
    pre_res = v
    if c.res and mutant != 'res_before_act':
        v = v + resv
    Cv = v.to(torch.bfloat16 if c.out_bf16 else torch.float32)
    C2v = (pre_res if mutant == 'c2_before_res' else v).to(torch.bfloat16) if c.C2 else None
    stats = None
    if c.stats:
        xs = v if mutant == 'stats_unrounded' else consumer_values(c, v)
        stats = chunk_sums(c, x, xs, torch.float32)[0]
    return lay_out(c, x, Cv, C2v, stats, mutant)


# ------------------------------------------------------------------------------------------------ the call

def operands(c, x, device='cpu'):
    """name -> tensor: the physical buffers in the types the entry point reads"""
    geo, N = x.geo, c.N
    a_t = torch.float32 if c.a_f32 else torch.bfloat16
    t = dict(A=x.A_buf.to(a_t).to(device))
    if c.dtype == BF16X3:
        img = x.W_buf.clone()
        img[:N, :geo.kpad] = split_planes(x.W_buf[:N, :geo.kpad].contiguous())
        t['W'] = img.to(device)
    else:
        t['W'] = x.W_buf.to(torch.bfloat16 if c.dtype == BF16 else torch.float32).to(device)
    for name, on, src in (('bias', c.bias, x.bias_buf), ('res', c.res, x.res_buf), ('a_rows', c.gather, x.a_rows)):
        if on:
            t[name] = src.to(device)
    if c.ln:
        t['ln_s'], t['ln_t'] = x.s_buf.to(device), x.t_buf.to(device)
        if c.ln == 2:
            t['ln_stats'] = x.stats_in.to(device)
    if c.scatter:
        t['row_off'], t['col_off'] = x.row_off.to(device), x.col_off.to(device)
    for name, buf in blank(c, x).items():
        t[name] = buf.to(device)
    return t


def ex_args(c, x, t):
    """pk_gemm_ex's arguments up to the stream, by name (a dict keeps their order), from the buffers of operands()"""
    geo = x.geo
    p = lambda name, off=0: (t[name].data_ptr() + off) if name in t else None
    esz = 2 if c.out_bf16 else 4
    return dict(dtype=c.dtype, a_is_f32=int(c.a_f32), A=p('A'), lda=geo.lda, W=p('W'), ldw=geo.ldw, M=c.M, N=c.N, K=c.K, bias=p('bias', 4 * geo.boff),
                res=p('res'), ldr=geo.ldr if c.res else 0, C=p('C') if c.scatter else p('C', (G * geo.ldc + geo.coff) * esz), ldc=c.N if c.scatter else geo.ldc,
                out_is_f32=int(not c.out_bf16), act=c.act, a_rows=p('a_rows'), a_nrows=geo.rowsA if c.gather else c.M, variant=c.variant,
                C2=p('C2', G * geo.ldc2 * 2), ldc2=geo.ldc2 if c.C2 else 0, ln_s=p('ln_s'), ln_t=p('ln_t'), ln_eps=LN_EPS if c.ln else 0.0,
                row_off=p('row_off'), col_off=p('col_off'), stats_out=p('stats', G * 2 * geo.np_out * 4), ln_stats=p('ln_stats'), dup_rows=geo.dup)


def gemm_args(c, x, t):
    """pk_gemm's arguments up to the stream"""
    a = ex_args(c, x, t)
    return tuple(a[k] for k in ('dtype', 'a_is_f32', 'A', 'lda', 'W', 'ldw', 'M', 'N', 'K', 'bias', 'res', 'ldr', 'C', 'ldc', 'out_is_f32', 'act', 'a_rows'))


def splitk_args(c, x, t):
    """pk_gemm_splitk's arguments up to the stream, by name"""
    a = ex_args(c, x, t)
    return dict(dtype=c.dtype, A=a['A'], lda=a['lda'], W=a['W'], ldw=a['ldw'], M=c.M, N=c.N, K=c.K, splits=c.splits, C=a['C'], ldc=a['ldc'], bias=a['bias'],
                tile=c.tile)


# ------------------------------------------------------------------------------------------------ refusals

def _base(kind):
    b = dict(plain=_case('refuse_plain', BF16, 8, 65, 68, 72, bias=True, res=True),
             af32=_case('refuse_af32', BF16, 1, 65, 68, 72, a_f32=True),
             f32=_case('refuse_f32', F32, 8, 65, 68, 36),
             f32_tight=_case('refuse_f32_tight', F32, 1, 65, 68, 36, w_tight=True),
             x3=_case('refuse_x3', BF16X3, 8, 65, 68, 36),
             geglu=_case('refuse_geglu', BF16, 8, 65, 68, 72, act=ACT_GEGLU),
             c2=_case('refuse_c2', BF16, 8, 65, 68, 72, res=True, C2=True),
             stats=_case('refuse_stats', BF16, 8, 65, 68, 72, stats=True),
             ln1=_case('refuse_ln1', BF16, 8, 65, 68, 72, ln=1),
             ln2=_case('refuse_ln2', BF16, 8, 65, 68, 72, ln=2),
             scatter=_case('refuse_scatter', BF16, 8, 65, 68, 72, scatter=True),
             dup=_case('refuse_dup', BF16, 8, 65, 68, 72, dup=True),
             gather=_case('refuse_gather', BF16, 8, 65, 68, 72, gather=True))
    return b[kind]


EINVAL, EALIGN = -1, -2


def _set(**kw):
    return lambda a, t: a.update(kw)


def _add(name, off):
    return lambda a, t: a.update({name: a[name] + off})


def _give(name, src, off=0):
    """pass the buffer `src` of the case as the optional operand `name` (any non-null, suitably aligned address: a refused call reads nothing)"""
    return lambda a, t: a.update({name: t[src].data_ptr() + off})


# every `return PK_EINVAL` / `return PK_EALIGN` of gemm_ex that comes before the epilogue form is reported: (label, error, base case, change of the arguments)
FORM_REFUSALS = (
    ('M = 0', EINVAL, 'plain', _set(M=0)), ('N = 0', EINVAL, 'plain', _set(N=0)), ('K = 0', EINVAL, 'plain', _set(K=0)),
    ('A null', EINVAL, 'plain', _set(A=None)), ('W null', EINVAL, 'plain', _set(W=None)), ('C null', EINVAL, 'plain', _set(C=None)),
    ('dtype 3', EINVAL, 'plain', _set(dtype=3)), ('act 4', EINVAL, 'plain', _set(act=4)), ('act -1', EINVAL, 'plain', _set(act=-1)),
    ('K not whole pieces', EALIGN, 'plain', _set(K=68)), ('ldw not whole pieces', EALIGN, 'plain', _add('ldw', 4)), ('lda not whole pieces', EALIGN, 'plain', _add('lda', 4)),
    ('f32: K % 4', EALIGN, 'f32', _set(K=34)), ('f32 A in bf16 mode: K % 8', EALIGN, 'af32', _set(K=68)),
    ('A 4 bytes off', EALIGN, 'plain', _add('A', 4)), ('W 8 bytes off', EALIGN, 'plain', _add('W', 8)),
    ('f32 mode with a bf16 A', EINVAL, 'f32', _set(a_is_f32=0)), ('split-bf16 mode with a bf16 A', EINVAL, 'x3', _set(a_is_f32=0)),
    ('split-bf16 with C2', EINVAL, 'x3', lambda a, t: a.update(C2=t['C'].data_ptr(), ldc2=80)),
    ('GEGLU with an odd N', EINVAL, 'geglu', _set(N=67)),
    ('GEGLU with a residual', EINVAL, 'geglu', lambda a, t: a.update(res=t['W'].data_ptr(), ldr=72)),
    ('gather with a_nrows = 0', EINVAL, 'gather', _set(a_nrows=0)),
    ('C2 with the scalar epilogue', EINVAL, 'c2', _add('ldc', 1)), ('C2 with a bf16 C', EINVAL, 'c2', _set(out_is_f32=0)),
    ('C2 with GEGLU', EINVAL, 'c2', _set(act=ACT_GEGLU, res=None)), ('C2 in f32 mode', EINVAL, 'f32', lambda a, t: a.update(C2=t['C'].data_ptr(), ldc2=80)),
    ('ldc2 % 4', EINVAL, 'c2', _add('ldc2', 2)), ('C2 4 bytes off', EINVAL, 'c2', _add('C2', 4)),
    ('ln_s without ln_t', EINVAL, 'ln1', _set(ln_t=None)), ('ln_t without ln_s', EINVAL, 'ln1', _set(ln_s=None)),
    ('row_off without col_off', EINVAL, 'scatter', _set(col_off=None)), ('col_off without row_off', EINVAL, 'scatter', _set(row_off=None)),
    ('scatter with the scalar epilogue', EINVAL, 'scatter', _add('C', 4)), ('scatter with a bf16 C', EINVAL, 'scatter', _set(out_is_f32=0)),
    ('scatter with GEGLU', EINVAL, 'scatter', _set(act=ACT_GEGLU)), ('scatter with a residual', EINVAL, 'scatter', lambda a, t: a.update(res=t['W'].data_ptr(), ldr=72)),
    ('scatter with C2', EINVAL, 'scatter', lambda a, t: a.update(C2=t['W'].data_ptr(), ldc2=80)),
    ('ln_stats without ln_s', EINVAL, 'ln2', _set(ln_s=None, ln_t=None)), ('ln_stats with stats_out', EINVAL, 'ln2', _give('stats_out', 'C')),
    ('ln_stats 4 bytes off', EINVAL, 'ln2', _add('ln_stats', 4)),
    ('stats_out with the scalar epilogue', EINVAL, 'stats', _add('ldc', 1)), ('stats_out with GEGLU', EINVAL, 'stats', _set(act=ACT_GEGLU)),
    ('stats_out with scatter', EINVAL, 'scatter', _give('stats_out', 'W')), ('stats_out 4 bytes off', EINVAL, 'stats', _add('stats_out', 4)),
    ('dup_rows < 0', EINVAL, 'plain', _set(dup_rows=-1)), ('dup_rows with the scalar epilogue', EINVAL, 'dup', _add('ldc', 1)),
    ('dup_rows with GEGLU', EINVAL, 'dup', _set(act=ACT_GEGLU)), ('dup_rows with scatter', EINVAL, 'scatter', _set(dup_rows=70)),
    ('dup_rows with stats_out', EINVAL, 'stats', _set(dup_rows=70)), ('dup_rows < M', EINVAL, 'dup', _set(dup_rows=64)),
    ('an LDS-DMA variant with an unpadded W', EINVAL, 'f32_tight', _set(variant=8)), ('an LDS-DMA variant with an f32 A in bf16 mode', EINVAL, 'af32', _set(variant=8)),
    ('fold with an unpadded W', EINVAL, 'f32_tight', lambda a, t: a.update(ln_s=t['W'].data_ptr(), ln_t=t['W'].data_ptr(), ln_eps=1e-5)),
    ('fold with the scalar epilogue', EINVAL, 'ln1', _add('ldc', 1)), ('fold with ln_s 4 bytes off', EINVAL, 'ln1', _add('ln_s', 4)),
    ('fold with ln_t 4 bytes off', EINVAL, 'ln1', _add('ln_t', 4)), ('fold with a gather', EINVAL, 'ln1', lambda a, t: a.update(a_rows=t['W'].data_ptr(), a_nrows=70)),
    ('stats_out on a TN = 4 tile', EINVAL, 'stats', _set(variant=9)), ('stats_out on a register-staged loop', EINVAL, 'stats', _set(variant=1)),
    ('stats_out on bf16 variant 3', EINVAL, 'stats', _set(variant=3)),
)
# the refusals behind the form report: a variant with no instantiation for the type (nothing is launched)
LATE_REFUSALS = (('bf16 variant 3', EINVAL, 'plain', _set(variant=3)), ('bf16 variant 7', EINVAL, 'plain', _set(variant=7)),
                 ('f32 variant 27', EINVAL, 'f32', _set(variant=27)), ('f32 variant 33', EINVAL, 'f32', _set(variant=33)), ('f32 variant 50', EINVAL, 'f32', _set(variant=50)),
                 ('split-bf16 variant 1', EINVAL, 'x3', _set(variant=1)), ('split-bf16 variant 33', EINVAL, 'x3', _set(variant=33)),
                 ('split-bf16 variant 50', EINVAL, 'x3', _set(variant=50)))
SPLITK_BASE = dict(f32=_case('refuse_splitk_f32', F32, 0, 65, 68, 96, entry='splitk', bias=True, splits=3, tile=0),
                   bf16=_case('refuse_splitk_bf16', BF16, 0, 65, 68, 192, entry='splitk', bias=True, splits=3, tile=0))
SPLITK_REFUSALS = (
    ('A null', EINVAL, 'bf16', _set(A=None)), ('W null', EINVAL, 'bf16', _set(W=None)), ('C null', EINVAL, 'bf16', _set(C=None)), ('M = 0', EINVAL, 'bf16', _set(M=0)),
    ('N = 0', EINVAL, 'bf16', _set(N=0)), ('K = 0', EINVAL, 'bf16', _set(K=0)), ('splits = 0', EINVAL, 'bf16', _set(splits=0)), ('splits = 65', EINVAL, 'bf16', _set(splits=65)),
    ('dtype 3', EINVAL, 'bf16', _set(dtype=3)), ('tile 3', EINVAL, 'bf16', _set(tile=3)), ('tile 2 in f32 mode', EINVAL, 'f32', _set(tile=2)),
    ('K not whole k-tiles per slice', EINVAL, 'bf16', _set(K=128)), ('N % 4', EINVAL, 'bf16', _set(N=66)), ('ldc % 4', EINVAL, 'bf16', _add('ldc', 2)),
    ('ldc < N', EINVAL, 'bf16', _set(ldc=64)), ('A 4 bytes off', EALIGN, 'bf16', _add('A', 4)), ('W 4 bytes off', EALIGN, 'bf16', _add('W', 4)),
    ('C 4 bytes off', EALIGN, 'bf16', _add('C', 4)), ('bias 4 bytes off', EALIGN, 'bf16', _add('bias', 4)), ('lda not whole pieces', EALIGN, 'bf16', _add('lda', 4)),
    ('ldw not whole pieces', EALIGN, 'bf16', _add('ldw', 4)), ('W without the k-tile padding', EINVAL, 'bf16', _set(ldw=184)),
)
