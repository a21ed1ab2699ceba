"""Float64 restatement of the vocabulary head (csrc/sampler.hip: vocab_sample_kernel, vocab_resident_kernel, vocab_reduce_kernel, vocab_ce_kernel), the
seeded cases that reach every build and work-split path, and per-element checkers.  CPU only; tests/test_vocab_parity_host.py shows what the checkers
accept and reject, tests/test_vocab_parity_gpu.py runs the kernels against them.  Style and helpers are those of tests/gemm_reference.py.

Operands (build(), device_operands()): lda > D with NaN behind column D; A has 5 more physical rows than M, all NaN (the resident kernel reads rows >= M as
0 through its buffer descriptor, the tiled kernel does not read them); W is the first V rows of a taller NaN matrix, zero-padded to the k-tile (the packers'
contract) and NaN behind the padding; bias is the head of a longer NaN vector; U is (total, V) under the row indirection with NaN in the rows no rows[m]
names; the partials buffer is pre-filled with the NaN sentinel and has GUARD words behind 5 ntiles M.  A launch without the log-sum-exp state must leave
p_max and p_sum untouched, compared as integers.

Logits.  l64[m][v] in float64 from the operands as the kernel reads them (bf16-rounded values; hi + lo of split_planes for the split-bf16 W; plain f32),
plus the bias.  E[m][v] = D 2^-23 S_mv (+ SPLIT S_mv for split-bf16) + 2^-23 |l64|, S = sum_k |a||w|: the GEMM rule of gemm_reference and one ulp for the
bias add.

Noise, restated as the kernel writes it (T = max(f32(temperature), 1e-10f)):
  PARITY   l / T - log(-log(x) + 1e-10f), x = f32(u + 1e-10f) rounded to f32 as the kernel rounds it
  FAST     l log2e / T - log2(-log2 u), u = uniform24x4_np(seed + *seed_dev, rows[m] V + n) with the index a 64-bit number; u = 0 gives -inf: never chosen
  no_noise l
B[m][v]: E / T pushed through the expression, one unit 2^-23 per f32 rounding on the intermediate's magnitude (the division or the three roundings of
log2e / T, the sum, x -> -log x + eps), and the device logarithms: an error d in a = -log x moves log(a) by d / a.
Device functions.  Neither the kernel guides nor the documentation shipped with the toolchain state an error for logf, __log2f (v_log_f32) or __expf
(v_exp_f32 of x log2e), so, as ERFF_C does, the allowance starts from the CPU's f32 function.  What torch's f32 log / log2 / exp measure against float64
depends on the vector library the host dispatches to (between 1.02 and 1.57 units of 2^-24 of the result on the AVX2 and AVX512 hosts tried), so the
figure on record is that library's own guarantee, the same on every host: 1 ulp = 2.0 units of 2^-24 (*_CPU_RATIO; the host test
test_transcendental_allowances asserts that the measurement stays under it).  The device library is allowed 4 times that: LOG_C = LOG2_C = EXP_C = 8 units
of 2^-24 (four ulps).  __expf's argument product adds |x| 2^-24 on top.  Never from what a kernel returned.

Checks, for every (tile t, row m), no row left out (check_partials()):
  p_idx    inside the tile's valid columns [128 t, min(128 t + 128, V)); noisy64[p_idx] >= max_tile(noisy64) - (B[p_idx] + B[argmax]): where the gap to the
           runner-up exceeds the bounds this is equality with the arg-max; among columns that tie with it EXACTLY in float64 it is the lowest
  p_val    within B of noisy64[m][p_idx];  p_logit within E of l64[m][p_idx]
  p_max    >= max_tile(l64) - E[argmax], <= max_v (l64 + E), and attained: some column of the tile has its l64 within E of it.  ("Within E of the
           tile's largest l64" made rigorous: the f32 maximum may belong to a runner-up column w whose own error lifts it past the true maximum, by at
           most E_w -- wider on the upper side than E[argmax] alone; the attained clause keeps it from admitting a value no column produced.)
  p_sum    against sum_v exp(l64 - p_max) with the p_max the kernel returned: sum_v exp(.) (E_v + exp error + rescale error) plus the any-order sum bound;
           columns >= V contribute nothing
  no_noise p_val and p_logit (and p_max) are the same bits
singleton_share() is the share of (tile, row) pairs whose accept set is a single column, from the reference and the bounds alone; the host test holds
it to >= 98 % on every random case, so the index check is an equality nearly everywhere.

The second data set is gemm_reference's dyadic grid (A integers in [-8, 8], W and bias multiples of 1/16, no_noise): every logit is exact in f32, E = 0.
W has groups of IDENTICAL rows lifted by the bias above every other column (TIE_GROUPS): equal maxima in different lane groups, column fragments, waves
(sub-blocks of the resident kernel) and vocabulary tiles.  The lowest index must win bit for bit in the partials and after the reduce.

resident_plan(M, V, nworkers, NW) mirrors the kernel's segment / next_tile split on the host: per (XCD, worker, wave) the (row tile, vocabulary tile) pairs
in visiting order, and the paths reached (PATHS).

reduce_case / reduce_ref / check_reduce and ce_case / ce_ref / check_ce drive pk_vocab_reduce and pk_vocab_ce from synthetic partials built on the CPU (tile
counts around the fold strides 8 x 8 and 64, exact ties across tiles); the folds' bound counts every rescale of the running sum as a rounded __expf.

Not covered: pk_vocab_eval, pk_vocab_ce_reg, pk_vocab_weight_mean, pk_ce_grad_slab (their own restatements), the PK_VOCAB_PANEL=0 order, the uninstantiated
TNW = 2 build, Philox indexes beyond what torch can materialise."""
import functools
import math
from types import SimpleNamespace as NS

import numpy as np
import torch

from tests.gemm_reference import F32, BF16, BF16X3, NAN, SENT32, SPLIT, TNAME, U1, U24, _gen, bf, ceil_to, split_planes
from tests.train_glue_reference import assert_same_bits, assert_untouched, assert_within, sum_bound   # noqa: F401  (re-exported to the tests)
from tests.util import uniform24x4_np

LOG_CPU_RATIO = LOG2_CPU_RATIO = EXP_CPU_RATIO = 2.0     # 1 ulp, the CPU vector library's guarantee, in units of 2^-24 (measured 1.02 - 1.57 by host); factor 4
LOG_C, LOG2_C, EXP_C = 4 * LOG_CPU_RATIO, 4 * LOG2_CPU_RATIO, 4 * EXP_CPU_RATIO
EPS32 = float(np.float32(1e-10))
LOG2E32 = float(np.float32(1.44269504088896340736))
GUARD = 64                        # sentinel words behind the partials
SENTINEL = -7                     # pre-fill of the integer outputs of the reduce
NRESC = 12                        # rescales of a tile's running sum: 8 sub-blocks + 2 shuffles (resident), 2 shuffles + 3 waves (tiled), with slack
PARITY, FAST, NONE, PHILOX = 'parity', 'fast', 'none', 'philox'
PATHS = ('sweep', 'left_a>0', 'left_b<CT', 'second_tile', 'first_tile_later', 'wave_no_tile', 'worker_nseg0', 'xcd_CT<=0', 'short_last_tile')
# columns that share one W row and one (lifted) bias on the grid data: lane groups | column fragments | waves / sub-blocks | tiles (same and other fold
# lane of the reduce) | inside a tile and across tiles at once.  Columns >= V are dropped.
TIE_GROUPS = ((5, 9), (2, 18), (40, 100), (131, 515, 1155), (300, 304, 428))


def ntiles_of(V):
    return (V + 127) // 128


# ------------------------------------------------------------------------------------------------ cases

def _case(name, dtype, M, V, D, noise, lse, *, T=1.0, rows=None, seed=0x1234567890ABCDEF, seed_dev=None, mode=0, workers=0, data='rand', scale=3.0):
    """rows: None | 'perm' (a permutation sample of total = 2 M + 5) | 'big' (up to 2^31 - 1: FAST only, no U)"""
    return NS(name=name, dtype=dtype, M=M, V=V, D=D, noise=noise, lse=bool(lse), T=T, rows=rows, seed=seed, seed_dev=seed_dev, mode=mode, workers=workers,
              data=data, scale=scale)


def temperature_of(c):
    """the temperature word of the launch: max(f32(T), 1e-10f)"""
    return max(float(np.float32(c.T)), EPS32)


NOISE_T = {PARITY: 0.45, FAST: 0.7, NONE: 1.0}


def _six(prefix, dtype, M, V, D, **kw):
    return [_case(f'{prefix}/{n}{"+lse" if l else ""}', dtype, M, V, D, n, l, T=NOISE_T[n], **kw) for n in (PARITY, FAST, NONE) for l in (0, 1)]


def tiled_groups():
    """pytest id -> cases of the tiled kernel (mode 0)"""
    g = {}
    for dt in (F32, BF16, BF16X3):
        t = TNAME[dt]
        g[f'{t}/130x132x96'] = _six(f'tiled/{t}/130x132x96', dt, 130, 132, 96)
        Db = 72 if dt == BF16 else 40
        g[f'{t}/257x1156x{Db}/rows'] = _six(f'tiled/{t}/257x1156x{Db}', dt, 257, 1156, Db, rows='perm')
    g['bf16/130x132x72'] = _six('tiled/bf16/130x132x72', BF16, 130, 132, 72)
    g['panel/bf16'] = [_case('tiled/panel/bf16', BF16, 1030, 17668, 64, NONE, 1)]
    g['panel/f32'] = [_case('tiled/panel/f32', F32, 1030, 17668, 64, NONE, 0)]
    g['counter64'] = [_case('tiled/counter64', BF16, 130, 65536, 32, FAST, 0, T=0.7, rows='big')]
    g['clamp'] = [_case(f'tiled/clamp/{n}/T={T:g}', F32, 130, 132, 96, n, 1, T=T) for n in (PARITY, FAST) for T in (0.0, 1e-12)]
    g['seed_carry'] = [_case('tiled/seed_carry', F32, 130, 132, 96, FAST, 0, T=0.7, seed=0xFFFFFFFF, seed_dev=1)]
    g['grid'] = ([_case(f'tiled/grid/{TNAME[dt]}/130x132', dt, 130, 132, 96, NONE, 1, data='grid') for dt in (F32, BF16, BF16X3)] +
                 [_case(f'tiled/grid/{TNAME[dt]}/257x1156', dt, 257, 1156, 72 if dt == BF16 else 40, NONE, l, rows='perm', data='grid')
                  for dt, l in ((F32, 0), (BF16, 1), (BF16X3, 0))])
    return g


def resident_groups():
    """pytest id -> cases of the resident kernel (bf16, D = 512); mode 1 = the 8-wave build, 2 = the 12-wave build, 3 = the measured rule"""
    g = {}
    for mode in (1, 2):
        g[f'mode{mode}/1030x1028'] = _six(f'res/m{mode}/1030x1028', BF16, 1030, 1028, 512, mode=mode)
    g['1300x1028/w3'] = [_case('res/m1/1300x1028/w3/parity+lse', BF16, 1300, 1028, 512, PARITY, 1, T=0.45, mode=1, workers=3, rows='perm'),
                         _case('res/m2/1300x1028/w3/fast', BF16, 1300, 1028, 512, FAST, 0, T=0.7, mode=2, workers=3),
                         _case('res/m2/1300x1028/w3/none+lse', BF16, 1300, 1028, 512, NONE, 1, mode=2, workers=3),
                         _case('res/m1/1300x1028/w3/fast', BF16, 1300, 1028, 512, FAST, 0, T=0.7, mode=1, workers=3)]
    g['1030x13316'] = [_case('res/m1/1030x13316/w2/fast+lse', BF16, 1030, 13316, 512, FAST, 1, T=1.0, mode=1, workers=2),
                       _case('res/m2/1030x13316/w2/none', BF16, 1030, 13316, 512, NONE, 0, mode=2, workers=2),
                       _case('res/m2/1030x13316/fast+lse', BF16, 1030, 13316, 512, FAST, 1, T=1.0, mode=2),
                       _case('res/m1/1030x13316/none', BF16, 1030, 13316, 512, NONE, 0, mode=1)]
    g['rule/2100x1028'] = [_case('res/m3/2100x1028/fast', BF16, 2100, 1028, 512, FAST, 0, T=0.7, mode=3),
                           _case('res/m3/2100x1028/none+lse', BF16, 2100, 1028, 512, NONE, 1, mode=3)]
    g['grid'] = [_case('res/m1/grid/1030x1028', BF16, 1030, 1028, 512, NONE, 1, mode=1, data='grid'),
                 _case('res/m2/grid/1300x1028/w3', BF16, 1300, 1028, 512, NONE, 0, mode=2, workers=3, data='grid', rows='perm')]
    return g


def below_rule_case():
    """mode 3 under 2048 rows stays on the tiled kernel"""
    return _case('tiled/m3/1030x1028/none+lse', BF16, 1030, 1028, 512, NONE, 1, mode=3)


def philox_cases():
    return [_case('philox/res/1030x1028', BF16, 1030, 1028, 512, PHILOX, 1, T=0.45, mode=1),
            _case('philox/tiled/130x132', F32, 130, 132, 96, PHILOX, 1, T=0.45, mode=0)]


def all_cases():
    out = [c for g in tiled_groups().values() for c in g] + [c for g in resident_groups().values() for c in g] + [below_rule_case()] + philox_cases()
    assert len({c.name for c in out}) == len(out)
    return out


def is_resident(c):
    """the dispatch of vocab_sample_launch"""
    if c.dtype != BF16 or c.D != 512 or not c.mode:
        return False
    return c.M >= (2048 if c.mode == 3 else 1024)


def resident_build(c):
    """(NW, PARITY, LSE) of the instantiation a resident case launches"""
    nw = 12 if (c.mode == 2 or (c.mode == 3 and not c.lse)) else 8
    return (nw, c.noise in (PARITY, PHILOX), c.lse)


# ------------------------------------------------------------------------------------------------ operands

def geometry(c):
    g = NS()
    g.q = 8 if c.dtype == BF16 else 4
    g.bk = 64 if c.dtype == BF16 else 32
    g.kpad = ceil_to(c.D, g.bk)
    g.lda = c.D + 2 * g.q
    g.ldw = g.kpad + g.q
    g.rowsA = c.M + 5
    g.nt = ntiles_of(c.V)
    g.total = 2 * c.M + 5 if c.rows == 'perm' else c.M
    return g


@functools.lru_cache(maxsize=3)
def _data(dtype, M, V, D, data, scale):
    g = _gen(f'vocab/{dtype}/{M}/{V}/{D}/{data}')
    if data == 'rand':
        A = torch.randn(M, D, generator=g)
        W = torch.randn(V, D, generator=g) / math.sqrt(D) * scale
        bias = torch.randn(V, generator=g) * 0.1
    else:
        A = torch.randint(-8, 9, (M, D), generator=g).float()
        W = torch.randint(-16, 17, (V, D), generator=g).float() / 16
        bias = torch.randint(-64, 65, (V,), generator=g).float() / 16
        lift = float(2 ** math.ceil(math.log2(8 * D + 8)))                          # above every other column's |logit| <= 8 D + 4
        for grp in TIE_GROUPS:
            cols = [v for v in grp if v < V]
            if not cols:
                continue
            W[cols] = W[cols[0]].clone()
            bias[cols] = lift + float(bias[cols[0]])
        assert (8.0 * D + lift + 8) * 16 < 2 ** 24
    if dtype == BF16:
        A, W = bf(A), bf(W)
    if dtype == BF16X3:                                                              # W as the kernels read it: hi + lo of the planes
        hi = bf(W)
        W64 = hi.double() + bf(W - hi).double()
    else:
        W64 = W.double()
    l64 = A.double() @ W64.t() + bias.double()
    if data == 'rand':
        S = A.double().abs() @ W64.abs().t()
        E = (D * U1 + (SPLIT if dtype == BF16X3 else 0.0)) * S + U1 * l64.abs()
    else:
        E = torch.zeros_like(l64)
    return NS(A=A, W=W, W64=W64, bias=bias, l64=l64, E=E)


def build(c):
    """the seeded operands of a case on the CPU: logical A, W, bias, rows, U, the float64 logits and their bound, and the physical buffers"""
    geo = geometry(c)
    d = _data(c.dtype, c.M, c.V, c.D, c.data, c.scale)
    x = NS(geo=geo, A=d.A, W=d.W, W64=d.W64, bias=d.bias, l64=d.l64, E=d.E, rows=None, U=None)
    g = _gen(c.name + '/noise')
    if c.rows == 'perm':
        x.rows = torch.randperm(geo.total, generator=g)[:c.M].to(torch.int32)
    elif c.rows == 'big':
        x.rows = torch.randint(0, 2 ** 31 - 1, (c.M,), generator=g).to(torch.int32)
        x.rows[0], x.rows[1], x.rows[2] = 2 ** 31 - 1, 0, 2 ** 16                    # the largest index, the smallest, and the first with a high word
    if c.noise == PARITY:
        x.U = torch.rand(c.M, c.V, generator=g)
        for t in range(geo.nt):                                                      # the ends of [0, 1): where the two 1e-10 terms matter
            v0 = 128 * t
            x.U[(7 * t + 3) % c.M, min(v0 + (5 * t) % 128, c.V - 1)] = 1.0 - 2.0 ** -24
            x.U[(7 * t + 4) % c.M, min(v0 + (11 * t + 1) % 128, c.V - 1)] = 0.0
    return x


def lrows(c, x):
    return x.rows.long() if x.rows is not None else torch.arange(c.M)


def seed_of(c):
    return (c.seed + (c.seed_dev or 0)) & 0xFFFFFFFFFFFFFFFF


def fast_uniforms(c, x, rows=None, mask32=False):
    r = (lrows(c, x) if rows is None else rows).numpy().astype(np.uint64)
    idx = r[:, None] * np.uint64(c.V) + np.arange(c.V, dtype=np.uint64)[None, :]
    if mask32:
        idx = idx & np.uint64(0xFFFFFFFF)
    return torch.from_numpy(uniform24x4_np(seed_of(c), idx.reshape(-1)).reshape(c.M, c.V))


def _buffer(shape, dtype, fill=NAN):
    return torch.full(shape, fill, dtype=dtype)


def blank_partials(c):
    return torch.full((5 * ntiles_of(c.V) * c.M + GUARD,), SENT32, dtype=torch.int32)


def device_operands(c, x, device='cpu', U=None):
    """the physical buffers of a launch: name -> tensor"""
    geo, td = x.geo, (torch.bfloat16 if c.dtype == BF16 else torch.float32)
    t = {}
    A = _buffer((geo.rowsA, geo.lda), torch.float32)
    A[:c.M, :c.D] = x.A
    Wl = torch.zeros(c.V, geo.kpad)
    Wl[:, :c.D] = x.W
    W = _buffer((c.V + 3, geo.ldw), torch.float32)
    if c.dtype == BF16X3:
        W[:c.V, :geo.kpad] = split_planes(Wl)
    else:
        W[:c.V, :geo.kpad] = Wl
    t['A'], t['W'] = A.to(td), (W if c.dtype == BF16X3 else W.to(td))
    t['bias'] = _buffer((c.V + 12,), torch.float32)
    t['bias'][:c.V] = x.bias
    if x.rows is not None:
        t['rows'] = x.rows.clone()
    U = x.U if U is None else U
    if c.noise == PARITY:
        if c.rows == 'perm':
            t['U'] = _buffer((geo.total, c.V), torch.float32)
            t['U'][x.rows.long()] = U
        else:
            t['U'] = U.clone()
    if c.seed_dev is not None:
        t['seed_dev'] = torch.tensor([c.seed_dev], dtype=torch.int64)
    t['partials'] = blank_partials(c)
    return {k: v.to(device) for k, v in t.items()}


def sample_args(c, x, t):
    """pk_vocab_sample's arguments up to (not including) the stream"""
    p = lambda k: t[k].data_ptr() if k in t else None
    return [c.dtype, p('A'), x.geo.lda, p('W'), x.geo.ldw, p('bias'), c.M, c.V, c.D, float(c.T), p('U'), p('rows'), c.seed, p('seed_dev'),
            (1 if c.lse else 0) | (2 if c.noise == NONE else 0), p('partials')]


# ------------------------------------------------------------------------------------------------ reference and bound

def reference(c, x, U=None, wrong=None):
    """ref.l64, ref.E, ref.noisy, ref.B: (M, V) float64.  U: the uniforms of a Philox case.  wrong: a named restatement error (host test)"""
    l, E = x.l64, x.E
    T = temperature_of(c)
    if c.noise == NONE:
        return NS(l64=l, E=E, noisy=l, B=E)
    if c.noise in (PARITY, PHILOX):
        u = x.U if U is None else U
        xx = (u + torch.tensor(EPS32, dtype=torch.float32)).double()                 # rounded to f32 first, as the kernel does
        a = -torch.log(xx)
        b = a + EPS32
        gum = -torch.log(b)
        lt = l / T
        noisy = lt + gum
        da = LOG_C * U24 * a.abs()
        db = da + U1 * b.abs()
        dg = db / b.abs() + LOG_C * U24 * gum.abs()
        B = E / T + U1 * lt.abs() + dg + U1 * noisy.abs()
        return NS(l64=l, E=E, noisy=noisy, B=B)
    u = fast_uniforms(c, x).double()
    k = LOG2E32 / T
    a = -torch.log2(u)                                                               # u = 0: inf
    gl = torch.log2(a)
    lk = l * k
    noisy = lk - gl                                                                  # u = 0: -inf, never chosen
    da = LOG2_C * U24 * a
    dg = da / (a * math.log(2)) + LOG2_C * U24 * gl.abs()
    B = E * k + 3 * U1 * lk.abs() + dg + U1 * noisy.abs()
    zero = u == 0
    noisy = torch.where(zero, torch.full_like(noisy, -math.inf), noisy)
    B = torch.where(zero | ~torch.isfinite(B), torch.zeros_like(B), B)
    return NS(l64=l, E=E, noisy=noisy, B=B)


def _tiles(t, V, fill):
    """(M, V) -> (M, ntiles, 128), the last tile filled up"""
    M, nt = t.shape[0], ntiles_of(V)
    out = torch.full((M, nt * 128), fill, dtype=t.dtype)
    out[:, :V] = t
    return out.view(M, nt, 128)


def accept_counts(c, ref):
    """per (row, tile): the number of columns the index check accepts"""
    n, B = _tiles(ref.noisy, c.V, -math.inf), _tiles(ref.B, c.V, 0.0)
    mx, am = n.max(-1)
    B_am = B.gather(-1, am[..., None])
    return (n >= mx[..., None] - (B + B_am)).sum(-1)


def singleton_share(c, ref):
    return float((accept_counts(c, ref) == 1).double().mean())


def split_partials(c, buf):
    """the five [tile][row] arrays of a partials buffer (int32 words) as (M, ntiles) tensors, and the guard words"""
    nt, M = ntiles_of(c.V), c.M
    sz = nt * M
    w = buf.detach().cpu().view(torch.int32)
    arr = [w[i * sz:(i + 1) * sz].view(nt, M).t().contiguous() for i in range(5)]
    f = lambda a: a.view(torch.float32)
    return NS(val=f(arr[0]), idx=arr[1], logit=f(arr[2]), max=f(arr[3]), sum=f(arr[4]), max_bits=arr[3], sum_bits=arr[4], guard=w[5 * sz:])


def _ratio(err, bound):
    return float(torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max()) if err.numel() else 0.


def check_partials(c, ref, buf, what=None):
    """every (tile, row) of a launch's partials against the reference; returns name -> largest error / bound"""
    what = what or c.name
    p = split_partials(c, buf)
    M, V, nt = c.M, c.V, ntiles_of(c.V)
    assert (p.guard == SENT32).all() and p.guard.numel() == GUARD, f'{what}: written behind the partials'
    lo = (torch.arange(nt) * 128)[None, :]
    hi = torch.clamp(lo + 128, max=V)
    idx = p.idx.long()
    bad = (idx < lo) | (idx >= hi)
    assert not bad.any(), f'{what}: p_idx outside its tile at (row, tile) {tuple(bad.nonzero()[0].tolist())}: {int(idx[bad][0])} ({int(bad.sum())} pairs)'
    loc = (idx - lo)[..., None]
    n, B = _tiles(ref.noisy, V, -math.inf), _tiles(ref.B, V, 0.0)
    l, E = _tiles(ref.l64, V, -math.inf), _tiles(ref.E, V, 0.0)
    mx, am = n.max(-1)
    n_at, B_at, B_am = n.gather(-1, loc)[..., 0], B.gather(-1, loc)[..., 0], B.gather(-1, am[..., None])[..., 0]
    bad = ~(n_at >= mx - (B_at + B_am))
    if bad.any():
        m, t = bad.nonzero()[0].tolist()
        raise AssertionError(f'{what}: row {m} tile {t} chose column {int(idx[m, t])} with reference value {n_at[m, t].item()!r}; column {128 * t + int(am[m, t])} '
                             f'has {mx[m, t].item()!r}, beyond the bounds {B_at[m, t].item():.3e} + {B_am[m, t].item():.3e} ({int(bad.sum())} of {bad.numel()} pairs)')
    first_tie = (n == n_at[..., None]).int().argmax(-1)
    bad = first_tie != loc[..., 0]
    assert not bad.any(), (f'{what}: {int(bad.sum())} pairs chose a later one of exactly equal maxima, first at (row, tile) {tuple(bad.nonzero()[0].tolist())}: '
                           f'column {int(idx[bad][0])}')
    out = {}
    fin = torch.isfinite(n_at)
    assert torch.equal(p.val[~fin].double(), n_at[~fin]), f'{what}: p_val where the reference is not finite'
    out['p_val'] = assert_within(p.val[fin], n_at[fin], B_at[fin], f'{what}: p_val')
    l_at, E_at = l.gather(-1, loc)[..., 0], E.gather(-1, loc)[..., 0]
    out['p_logit'] = assert_within(p.logit, l_at, E_at, f'{what}: p_logit')
    if c.noise == NONE:
        assert_same_bits(p.val, p.logit, f'{what}: no_noise, p_val against p_logit')
    if not c.lse:
        assert (p.max_bits == SENT32).all() and (p.sum_bits == SENT32).all(), f'{what}: p_max / p_sum written without the log-sum-exp state'
        return out
    if c.noise == NONE:
        assert_same_bits(p.max, p.val, f'{what}: no_noise, p_max against p_val')
    lmx, lam = l.max(-1)
    E_lam = E.gather(-1, lam[..., None])[..., 0]
    pm = p.max.double()
    assert torch.isfinite(pm).all(), f'{what}: p_max not finite'
    upper = (l + E).max(-1).values
    bad = ~((pm >= lmx - E_lam) & (pm <= upper))
    assert not bad.any(), (f'{what}: p_max out of bound at (row, tile) {tuple(bad.nonzero()[0].tolist())}: {pm[bad][0].item()!r} against {lmx[bad][0].item()!r} '
                           f'({int(bad.sum())} pairs)')
    attained = ((pm[..., None] - l).abs() <= E).any(-1)
    assert attained.all(), f'{what}: p_max is no column\'s logit at (row, tile) {tuple((~attained).nonzero()[0].tolist())}'
    out['p_max'] = _ratio((pm - lmx).abs(), torch.maximum(E_lam, upper - lmx))
    xarg = l - pm[..., None]                                                         # -inf in the padding: contributes nothing
    ex = torch.exp(xarg)
    xa = torch.where(torch.isfinite(xarg), xarg.abs(), torch.zeros_like(xarg))
    rel = E + (EXP_C + 3 * xa + 2 + NRESC * (EXP_C + 2)) * U24
    s = ex.sum(-1)
    out['p_sum'] = assert_within(p.sum, s, (ex * rel).sum(-1) + sum_bound(s, 128 + NRESC), f'{what}: p_sum')
    return out


# ------------------------------------------------------------------------------------------------ f32 emulation of the head (host test)

SAMPLE_MUTANTS = ('tile_local_index', 'last_max_wins', 'noise_by_m', 'noise_index_32bit', 'gumbel_no_eps', 'temperature_multiplied', 'unclamped_T',
                  'padding_in_sum', 'max_without_bias', 'sum_other_max')


def _mm32(c, x, order):
    A, W = x.A, x.W
    if order:
        A, W = A.flip(1), W.flip(1)
    if c.dtype == BF16X3:
        ah, wh = bf(A), bf(W)
        al, wl = bf(A - ah), bf(W - wh)
        return ah @ wh.t() + ah @ wl.t() + al @ wh.t()
    return A @ W.t()


def emulate(c, x, order=0, mutant=None, U=None):
    """the head in f32 on the CPU, in one of two summation orders, as a partials buffer; `mutant` plants one named error"""
    M, V, nt = c.M, c.V, ntiles_of(c.V)
    acc = _mm32(c, x, order)
    logit = acc + x.bias
    T = torch.tensor(temperature_of(c), dtype=torch.float32)
    if mutant == 'unclamped_T':
        T = torch.tensor(float(np.float32(c.T)), dtype=torch.float32)
    eps = torch.tensor(EPS32, dtype=torch.float32)
    rows = torch.arange(M) if mutant == 'noise_by_m' else None
    with np.errstate(divide='ignore', invalid='ignore'):
        if c.noise == NONE:
            noisy = logit.clone()
        elif c.noise in (PARITY, PHILOX):
            u = x.U if U is None else U
            if mutant == 'noise_by_m' and x.rows is not None:                        # U[m] instead of U[rows[m]]
                full = torch.zeros(x.geo.total, V)
                full[x.rows.long()] = u
                u = full[:M]
            gum = -torch.log(-torch.log(u)) if mutant == 'gumbel_no_eps' else -torch.log(-torch.log(u + eps) + eps)
            noisy = (logit * T if mutant == 'temperature_multiplied' else logit / T) + gum
        else:
            u = fast_uniforms(c, x, rows=rows, mask32=mutant == 'noise_index_32bit')
            k = (1.0 / T) * torch.tensor(LOG2E32, dtype=torch.float32)
            if mutant == 'temperature_multiplied':
                k = T * torch.tensor(LOG2E32, dtype=torch.float32)
            noisy = logit * k - torch.log2(-torch.log2(u))
    nz = _tiles(noisy, V, -math.inf)
    lz = _tiles(logit, V, -math.inf)
    if mutant == 'last_max_wins':
        loc = 127 - nz.flip(-1).argmax(-1)
    else:
        loc = nz.argmax(-1)                                                          # the first maximum
    val = nz.gather(-1, loc[..., None])[..., 0]
    lg = lz.gather(-1, loc[..., None])[..., 0]
    idx = loc + (0 if mutant == 'tile_local_index' else (torch.arange(nt) * 128)[None, :])
    buf = blank_partials(c)
    sz = nt * M
    put = lambda i, a: buf[i * sz:(i + 1) * sz].copy_(a.t().contiguous().view(torch.int32).reshape(-1))
    put(0, val.float())
    buf[sz:2 * sz] = idx.t().contiguous().to(torch.int32).reshape(-1)
    put(2, lg.float())
    if c.lse:
        mx = _tiles(acc if mutant == 'max_without_bias' else logit, V, -math.inf).max(-1).values
        ref_mx = lz.max(-1).values.max(-1, keepdim=True).values.expand_as(mx) if mutant == 'sum_other_max' else mx
        e = torch.exp(_tiles(logit, V, 0.0 if mutant == 'padding_in_sum' else -math.inf) - ref_mx[..., None])      # the padding's logit: acc 0 + bias 0
        if order:
            e = e.flip(-1)
        s = torch.zeros_like(mx)
        for j in range(128):                                                         # a sequential f32 sum in this order
            s = s + e[..., j]
        put(3, mx.float())
        put(4, s.float())
    return buf


# ------------------------------------------------------------------------------------------------ the work split of the resident kernel

@functools.lru_cache(maxsize=None)
def _xcd_plan(MT, CT, nworkers, NW):
    """one XCD's share of the split: ({(worker, wave): ((row tile, tile of the XCD's range), ...)}, paths); depends on the XCD only through CT"""
    plan, paths = {}, set()
    full = MT // nworkers
    R = MT - full * nworkers
    Pl = R * CT
    for s in range(nworkers):
        q0, q1 = s * Pl // nworkers, (s + 1) * Pl // nworkers
        lrow0 = q0 // CT
        nleft = (q1 - 1) // CT - lrow0 + 1 if q1 > q0 else 0
        nseg = full + nleft
        if nseg == 0:
            paths.add('worker_nseg0')
            continue

        def segment(k):
            if k < full:
                return k * nworkers + s, 0, CT
            l = lrow0 + (k - full)
            lo = l * CT
            return full * nworkers + l, max(q0, lo) - lo, min(q1, lo + CT) - lo

        segs = [segment(k) for k in range(nseg)]
        for wave in range(NW):
            def next_tile(k, cc):
                if cc + NW < segs[k][2]:
                    paths.add('second_tile')
                    return k, cc + NW
                for k2 in range(k + 1, nseg):
                    r, a, b = segs[k2]
                    if a + wave < b:
                        return k2, a + wave
                return nseg, 0

            r, a, b = segs[0]
            tk, tcc = (0, a + wave) if a + wave < b else next_tile(0, b)
            if tk >= nseg:
                paths.add('wave_no_tile')
            elif tk > 0:
                paths.add('first_tile_later')
            seq = []
            for k in range(nseg):
                r, a, b = segs[k]
                while tk == k:
                    seq.append((r, tcc))
                    if k < full:
                        paths.add('sweep')
                    else:
                        if a > 0:
                            paths.add('left_a>0')
                        if b < CT:
                            paths.add('left_b<CT')
                    tk, tcc = next_tile(tk, tcc)
            plan[(s, wave)] = tuple(seq)
    return plan, frozenset(paths)


def resident_plan(M, V, nworkers, NW):
    """host mirror of vocab_resident_kernel's segment / next_tile split: ({(xcd, worker, wave): [(row tile, vocabulary tile), ...]}, paths reached)"""
    MT, nt = (M + 127) // 128, ntiles_of(V)
    CTX = (nt + 7) // 8
    plan, paths = {}, set()
    if V % 128:
        paths.add('short_last_tile')
    for xcd in range(8):
        c_lo = xcd * CTX
        CT = min(c_lo + CTX, nt) - c_lo
        if CT <= 0:
            paths.add('xcd_CT<=0')
            continue
        xp, pp = _xcd_plan(MT, CT, nworkers, NW)
        paths |= pp
        for (s, wave), seq in xp.items():
            plan[(xcd, s, wave)] = [(r, c_lo + cc) for r, cc in seq]
    return plan, paths


# ------------------------------------------------------------------------------------------------ pk_vocab_reduce on synthetic partials

REDUCE_NT = (1, 7, 8, 9, 63, 64, 65, 72, 513)
REDUCE_M = (1, 31, 32, 33, 100)
REDUCE_MUTANTS = ('skip_tiles_ge_64', 'score_p', 'masked_score', 'ids_where_unmasked', 'pred_not_scattered', 'last_max_wins')


def reduce_case(nt, M, *, rows, mask, ids, scores, lse, seed=0):
    g = _gen(f'reduce/{nt}/{M}/{rows}/{mask}/{ids}/{scores}/{lse}/{seed}')
    c = NS(name=f'reduce/nt{nt}/M{M}/{"r" if rows else ""}{"m" if mask else ""}{"i" if ids else ""}{"s" if scores else ""}{"l" if lse else ""}',
           nt=nt, M=M, V=128 * nt - 4, has_rows=rows, has_mask=mask, has_ids=ids, has_scores=scores, lse=lse)
    c.val = torch.randint(0, 5, (nt, M), generator=g).float() / 4                    # few levels: exact ties across tiles in every row
    for m in range(0, M, 3):                                                         # every third row: ONE maximum, walking down from the last tile
        c.val[(nt - 1 - m // 3) % nt, m] = 2.0
    c.idx = (torch.arange(nt)[:, None] * 128 + torch.randint(0, 124, (nt, M), generator=g)).to(torch.int32)
    c.pmax = torch.randn(nt, M, generator=g) * 3
    c.logit = c.pmax - torch.rand(nt, M, generator=g) * 4
    c.psum = 1 + torch.rand(nt, M, generator=g) * 127
    c.total = 2 * M + 5 if rows else M
    c.rows = torch.randperm(c.total, generator=g)[:M].to(torch.int32) if rows else None
    c.mask = (torch.rand(c.total, generator=g) > 0.4).to(torch.uint8) if mask else None
    c.ids0 = torch.randint(0, c.V, (c.total,), generator=g)
    return c


def reduce_partials(c):
    nan = torch.full_like(c.pmax, NAN)
    parts = [c.val, c.idx.view(torch.float32), c.logit, c.pmax if c.lse else nan, c.psum if c.lse else nan]
    return torch.cat([p.reshape(-1) for p in parts])


def reduce_cases():
    """every tile count with every row count, the options rotating so that each appears on and off at every tile count"""
    out, i = [], 0
    for nt in REDUCE_NT:
        for M in REDUCE_M:
            o = [(i >> b) & 1 for b in range(5)]
            out.append(reduce_case(nt, M, rows=bool(o[0]), mask=bool(o[1]), ids=bool(o[2]), scores=bool(o[3]), lse=bool(o[4])))
            i += 7
    for nt in (9, 65, 513):                                                          # everything on, everything off
        out.append(reduce_case(nt, 33, rows=True, mask=True, ids=True, scores=True, lse=True, seed=1))
        out.append(reduce_case(nt, 33, rows=False, mask=False, ids=False, scores=False, lse=False, seed=1))
    return out


def fold_lse(pmax, psum, nfold):
    """(lmax, lsum64, bound on lsum) of the max / sum-exp fold over dim 0, every one of `nfold` rescales counted as a rounded __expf"""
    pm, ps = pmax.double(), psum.double()
    lmax = pm.max(0).values
    d = pm - lmax
    term = ps * torch.exp(d)
    lsum = term.sum(0)
    rel = (EXP_C + 3 * d.abs() + 2 + nfold * (EXP_C + 2)) * U24
    return lmax, lsum, (term * rel).sum(0) + sum_bound(lsum, pm.shape[0] + nfold)


def reduce_ref(c, mutant=None):
    """what pk_vocab_reduce must leave: pred, ids (bit for bit, SENTINEL where nothing is written), scores and their bound (NaN where nothing is written)"""
    nt, M = c.nt, c.M
    val, idx, pmax, psum = c.val.double(), c.idx.long(), c.pmax, c.psum
    if mutant == 'skip_tiles_ge_64':
        val, pmax, psum = val.clone(), pmax[:64], psum[:64]
        val[64:] = -math.inf
    tied = val == val.max(0).values
    if mutant == 'last_max_wins':
        win = torch.where(tied, idx, torch.full_like(idx, -1)).argmax(0)
    else:
        win = torch.where(tied, idx, torch.full_like(idx, 2 ** 40)).argmin(0)           # first maximum wins: the lowest index
    bidx = idx.gather(0, win[None])[0]
    r = c.rows.long() if c.rows is not None else torch.arange(M)
    if mutant == 'pred_not_scattered':
        r = torch.arange(M)
    mk = c.mask[r].bool() if c.mask is not None else torch.ones(M, dtype=torch.bool)
    pred = torch.full((c.total,), SENTINEL, dtype=torch.int64)
    pred[r] = bidx
    ids = c.ids0.clone()
    if c.has_ids:
        w = torch.ones_like(mk) if mutant == 'ids_where_unmasked' else mk
        ids[r[w]] = bidx[w]
    ref = NS(pred=pred, ids=ids, scores=None, bound=None, written=None)
    if c.has_scores and c.lse:
        blog = c.logit.double().gather(0, win[None])[0]
        lmax, lsum, dsum = fold_lse(pmax, psum, nt // 8 + 16)
        xx = blog - lmax
        P = torch.exp(xx) / lsum
        relP = (EXP_C + 3 * xx.abs() + 2) * U24 + dsum / lsum + 2 * U1
        sc = P if mutant == 'score_p' else 1 - P
        bound = P * relP + U1 * sc.abs()
        masked = torch.full_like(sc, 0.0 if mutant == 'masked_score' else -1e4)
        sc, bound = torch.where(mk, sc, masked), torch.where(mk, bound, torch.zeros_like(bound))
        ref.scores, ref.bound = torch.full((c.total,), NAN, dtype=torch.float64), torch.zeros(c.total, dtype=torch.float64)
        ref.scores[r], ref.bound[r] = sc, bound
        ref.written = torch.zeros(c.total, dtype=torch.bool)
        ref.written[r] = True
        ref.masked_out = torch.zeros(c.total, dtype=torch.bool)
        ref.masked_out[r] = ~mk
    return ref


def reduce_buffers(c, device='cpu'):
    t = dict(partials=reduce_partials(c), pred=torch.full((c.total,), SENTINEL, dtype=torch.int64), ids=c.ids0.clone(),
             scores=torch.full((c.total,), NAN, dtype=torch.float32))
    if c.rows is not None:
        t['rows'] = c.rows.clone()
    if c.mask is not None:
        t['mask'] = c.mask.clone()
    return {k: v.to(device) for k, v in t.items()}


def check_reduce(c, ref, pred, ids, scores, what=None):
    """pred / ids / the untouched entries bit for bit; scores per element; a masked-out row holds -1e4 exactly.  Returns the scores' error / bound"""
    what = what or c.name
    pred, ids, scores = pred.cpu(), ids.cpu(), scores.cpu()
    assert torch.equal(pred, ref.pred), f'{what}: pred differs at {(pred != ref.pred).nonzero().flatten()[:4].tolist()} ({int((pred != ref.pred).sum())} entries)'
    assert torch.equal(ids, ref.ids), f'{what}: ids differ at {(ids != ref.ids).nonzero().flatten()[:4].tolist()}'
    if ref.scores is None:
        assert_untouched(scores, f'{what}: scores')
        return 0.
    assert_untouched(scores[~ref.written], f'{what}: scores outside rows[]')
    mo = ref.masked_out
    assert (scores[mo] == -1e4).all() if mo.any() else True, f'{what}: a masked-out row\'s score is not -1e4'
    return assert_within(scores[ref.written], ref.scores[ref.written], ref.bound[ref.written], f'{what}: scores')


# ------------------------------------------------------------------------------------------------ pk_vocab_ce on synthetic (max, sum) partials

CE_NT = (1, 63, 64, 65, 130)
CE_D = (40, 72, 512)
CE_M = 37
CE_GUARD = 3
CE_MUTANTS = ('target_at_m', 'hi_plane_only')


def ce_case(dtype, nt, D, seed=0):
    V = 128 * nt - 4
    name = f'ce/{TNAME[dtype]}/nt{nt}/D{D}'
    g = _gen(f'{name}/{seed}')
    c = _case(name, dtype, CE_M, V, D, NONE, 1, rows='perm')
    x = build(c)
    x.pmax = torch.randn(nt, CE_M, generator=g) * 3
    x.psum = 1 + torch.rand(nt, CE_M, generator=g) * 127
    x.targets = torch.randint(0, V, (x.geo.total,), generator=g)
    return c, x


def ce_cases():
    return [(dt, nt, D) for dt in (F32, BF16, BF16X3) for nt in CE_NT for D in CE_D]


def ce_partials(c, x):
    nt = ntiles_of(c.V)
    nan = torch.full((3 * nt * c.M,), NAN)
    return torch.cat([nan, x.pmax.reshape(-1), x.psum.reshape(-1)])


def ce_ref(c, x, pmax=None, psum=None, mutant=None):
    """(lse64, its bound, loss64, its bound) per row from the (max, sum) partials and the operands"""
    pmax, psum = (x.pmax if pmax is None else pmax), (x.psum if psum is None else psum)
    nt = pmax.shape[0]
    lmax, lsum, dsum = fold_lse(pmax, psum, nt // 64 + 8)
    lg = torch.log(lsum)
    lse = lmax + lg
    dlse = dsum / lsum + LOG_C * U24 * lg.abs() + U1 * lse.abs()
    r = torch.arange(c.M) if mutant == 'target_at_m' else lrows(c, x)
    tgt = x.targets[r]
    A, W = x.A.double(), (bf(x.W).double() if mutant == 'hi_plane_only' else x.W64)[tgt]
    dot = (A * W).sum(1)
    S = (A.abs() * W.abs()).sum(1)
    z = dot + x.bias.double()[tgt]
    loss = lse - z
    dloss = dlse + (c.D + 8) * U1 * S + U1 * z.abs() + U1 * loss.abs()
    return NS(lse=lse, dlse=dlse, loss=loss, dloss=dloss)


# ------------------------------------------------------------------------------------------------ refusals of pk_vocab_sample / pk_vocab_sample_philox

EINVAL, EALIGN = -1, -2


def refusal_base(dtype):
    return _case(f'refuse/{TNAME[dtype]}', dtype, 130, 132, 96, FAST, 1, T=0.7)


# (label, dtype, expected code, change(args list a, geometry)); argument positions: 2 lda, 4 ldw, 7 V, 8 D, 1 A, 3 W, 5 bias, 10 U, 0 dtype
def _set(i, f):
    def change(a, geo):
        a[i] = f(a[i], geo)
    return change


SAMPLE_REFUSALS = (
    ('V % 4', F32, EALIGN, _set(7, lambda v, g: v - 2)),
    ('D off the element group (f32)', F32, EALIGN, _set(8, lambda v, g: v - 2)),
    ('D off the element group (bf16)', BF16, EALIGN, _set(8, lambda v, g: v - 4)),
    ('lda off the element group (f32)', F32, EALIGN, _set(2, lambda v, g: v + 2)),
    ('lda off the element group (bf16)', BF16, EALIGN, _set(2, lambda v, g: v + 4)),
    ('ldw off the element group (x3)', BF16X3, EALIGN, _set(4, lambda v, g: v + 2)),
    ('ldw off the element group (bf16)', BF16, EALIGN, _set(4, lambda v, g: v + 4)),
    ('ldw under the padded k-tile (f32)', F32, EINVAL, _set(4, lambda v, g: g.kpad - 4)),
    ('ldw under the padded k-tile (bf16)', BF16, EINVAL, _set(4, lambda v, g: g.kpad - 8)),
    ('A misaligned', F32, EALIGN, _set(1, lambda v, g: v + 4)),
    ('W misaligned', BF16, EALIGN, _set(3, lambda v, g: v + 2)),
    ('bias misaligned', F32, EALIGN, _set(5, lambda v, g: v + 4)),
    ('U misaligned', F32, EALIGN, lambda a, geo: a.__setitem__(10, a[5] + 4)),            # a device address 4 bytes off 16; pk_vocab_sample only
    ('dtype = 3', F32, EINVAL, _set(0, lambda v, g: 3)),
)


def reduce_case_of(c, x, buf, *, mask=True, ids=True, scores=True, seed=0):
    """the reduce of a sampling launch's own partials: a reduce case whose partial arrays are what the launch left"""
    p = split_partials(c, buf)
    g = _gen(f'{c.name}/reduce/{seed}')
    r = NS(name=c.name + '/reduce', nt=ntiles_of(c.V), M=c.M, V=c.V, has_rows=x.rows is not None, has_mask=mask, has_ids=ids, has_scores=scores, lse=c.lse,
           val=p.val.t().contiguous(), idx=p.idx.t().contiguous(), logit=p.logit.t().contiguous(), pmax=p.max.t().contiguous(), psum=p.sum.t().contiguous(),
           total=x.geo.total, rows=x.rows)
    r.mask = (torch.rand(r.total, generator=g) > 0.4).to(torch.uint8) if mask else None
    r.ids0 = torch.randint(0, c.V, (r.total,), generator=g)
    return r


# ------------------------------------------------------------------------------------------------ f32 emulation of the two folds (host test)

def _fold32(pmax, psum, groups):
    """the online (max, sum exp) fold in f32: every group of tile indices is folded in its order, then the groups are merged in theirs"""
    M = pmax.shape[1]
    neg = torch.full((M,), -math.inf)

    def step(lmax, lsum, om, os):
        nm = torch.maximum(lmax, om)
        a = torch.where(lmax == -math.inf, torch.zeros_like(lsum), lsum * torch.exp(lmax - nm))
        b = torch.where(om == -math.inf, torch.zeros_like(os), os * torch.exp(om - nm))
        return nm, a + b
    parts = []
    for grp in groups:
        lmax, lsum = neg.clone(), torch.zeros(M)
        for t in grp:
            lmax, lsum = step(lmax, lsum, pmax[t].float(), psum[t].float())
        parts.append((lmax, lsum))
    lmax, lsum = parts[0]
    for om, os in parts[1:]:
        lmax, lsum = step(lmax, lsum, om, os)
    return lmax, lsum


def fold_orders(nt, stride):
    """two orders of the tile fold: the kernel's own (`stride` lanes, each over every stride-th tile, merged in lane order) and one descending chain"""
    return [[list(range(g, nt, stride)) for g in range(min(stride, nt))], [list(range(nt - 1, -1, -1))]]


def reduce_f32(c, order=0):
    """(pred, ids, scores) as an f32 reduce in one of two fold orders would leave them (the stride of vocab_reduce_kernel is 8 thread groups)"""
    ref = reduce_ref(c)
    scores = torch.full((c.total,), NAN)
    if c.has_scores and c.lse:
        lmax, lsum = _fold32(c.pmax, c.psum, fold_orders(c.nt, 8)[order])
        r = c.rows.long() if c.rows is not None else torch.arange(c.M)
        bidx = ref.pred[r]
        win = (c.idx.long() == bidx[None]).int().argmax(0)
        blog = c.logit.float().gather(0, win[None])[0]
        sc = 1.0 - torch.exp(blog - lmax) / lsum
        mk = c.mask[r].bool() if c.mask is not None else torch.ones(c.M, dtype=torch.bool)
        scores[r] = torch.where(mk, sc, torch.full_like(sc, -1e4))
    return ref.pred.clone(), ref.ids.clone(), scores


def ce_f32(c, x, order=0):
    """(lse, loss) as an f32 cross entropy in one of two fold and dot-product orders would leave them (vocab_ce_kernel folds 64 lanes)"""
    lmax, lsum = _fold32(x.pmax, x.psum, fold_orders(x.pmax.shape[0], 64)[order])
    lse = lmax + torch.log(lsum)
    tgt = x.targets[lrows(c, x)]
    A, W = x.A.float(), x.W64[tgt].float()                                           # hi + lo is exact in f32
    if order:
        A, W = A.flip(1), W.flip(1)
    dot = torch.zeros(c.M)
    for k in range(c.D):
        dot = dot + A[:, k] * W[:, k]
    return lse, lse - (dot + x.bias[tgt])
