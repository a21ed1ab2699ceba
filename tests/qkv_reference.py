"""Float64 restatement of the fused projection kernels -- pk_qkv_project (csrc/qkv.hip), pk_qkv_attn and pk_q_attn_cached (csrc/qkv_attn.hip) -- the seeded
cases that reach every branch of their dispatch, and per-element checkers whose bounds are derived from the kernels' rounding points.  CPU only;
tests/test_qkv_parity_host.py shows what the checkers accept and reject, tests/test_qkv_parity_gpu.py runs the kernels against them.  The attention stage
(structure, terms, MASS, check, binade_top, pads, unsplit) is the one of tests/attn_fwd_reference.py.

Inputs.  Rows x and weights W hold values the kernel's operand type holds exactly: dtype 1 bf16 rows and weights, dtype 2 f32 rows and f32 weights (packed
with attention.pack_linear_weight / _lib.split_planes).  K has at least three k-tiles and a tail (K % 64 = 8 | K % 32 = 4), ld > K and the row slack is
poisoned (NaN, +Inf in a second pass).  The bf16 rows and weights are QUANTISED as well: every row of x is an integer multiple of a power of two qx
(|x| < 2^8 qx), every weight of qw, so that every product and every partial sum of a projection, in whatever order the matrix core adds them, is an integer
multiple of qx qw below 2^24 qx qw and therefore exact in f32 (`exact` below checks the condition per output element instead of assuming it).  That keeps
the bf16 images the kernel writes bit-identical to the rounded reference except next to a rounding tie (see Marks).  The split-bf16 inputs are quantised the same way with more than 8 significant bits in ONE operand (the rows of the
planted cases, the weights of the pk_qkv_project cases), so that both lo planes are exercised and the dropped lo.lo product is 0.

Planted attention (pk_qkv_attn, pk_q_attn_cached).  K splits into two halves, the half into one group of coordinates per head.  Per head a block B
(64 x K/2, non-zero on the head's group) is what Wk reads the FIRST half through and Wq the SECOND half; Wv is dense.  The key rows are xkv_t = a_t [u_t ; noise],
the query rows xq_i = a_i [noise ; c_i] with c_i restricted to a head's group = the sum of the u_t of that (row, head)'s targets and forbidden keys: q_i is
parallel to k_t and the cosine-sim score of a target is about scale / sqrt(components), against about 0 +- scale / sqrt(group size) for every other key.
Targets rotate with the row, the head and the sequence so that every visible key is some row's target (causal: the diagonal key and one earlier key;
otherwise one key of a rotated permutation; cached: a rotation over the visible keys).  Forbidden components, which would take a target's mass if the kernel
admitted them: the first key beyond the diagonal (causal), a key of the neighbouring sequence of the same 64-row tile (n < 64), a masked key
(pk_q_attn_cached).  For pk_q_attn_cached the K^ / V^T images are written by the reference: K^ = round(l2norm(B u_t) k_scale), V random; the pad
rows of K^ are poisoned, the pad columns of V^T are zero, which is the kernel's documented precondition (include/phenaki_hip.h: it stages them
unmasked and gives them the weight 0; poisoned, every output row of a case with nk < nk_pad is NaN).
planted_property() (attn_fwd_reference) is asserted by the host test.  pk_qkv_project needs no structure: its outputs are the images themselves; rows and
weights are random.  Folded cases add an offset to every second query row (bf16) or to every query row (split-bf16) so that mean / std of the row is about 4;
their err / bound is recorded separately (`mean4`).

Reference, following the kernels' rounding points:
  1 projection      acc = x W^T in f64.
  2 fold            acc = x (gamma.W)^T - mean(x) s with mean over K and s as attention.folded_weight builds it (qa_project_q / qkv_project_kernel:
                    `acc -= mean * s4`).
  3 l2norm, scales  acc / max(|acc|, 1e-12) * q_scale * scale | * k_scale; v stays (`inv = scale / fmaxf(sqrtf(ss), 1e-12f)`, `v[r] *= inv * sc[r]`).
  4 image rounding  q^, k^, v rounded to bf16 (pack_bf2 / f2bf; store4 / store_elem) or to hi + lo (qa_put4 / bf16x3p).
  5 attention       attn_fwd_reference's softmax(Q K^T + bias - ALiBi, masks) V on the ROUNDED images.

Bound of an image element (project_error, normed_error), first order; every consumer doubles it for the second-order terms:
  e_acc   the f32 accumulation of K products (MFMA, gemm_dma.hpp main loop): (K + 4) 2^-24 (sum_k |x_k| |w_k| + |mean| |s|).  Where `exact` holds (the
          seeded cases) the accumulation and the row sum are exact and what is left is the fold itself: the division by K, the product with s and the
          subtraction, 4 * 2^-24 (|x.w| + |mean| |s|); 0 without a fold.  Split-bf16 adds what its three products leave out, computed from the operands
          themselves (x = hi + lo + r): |lo_x| |lo_w| + |r_x| |w| + |x| |r_w| summed over k (at most 3 * 2^-16 of sum |x| |w|, attn_fwd_reference's
          U_SPLIT term; 0 where one operand fits 8 bits and the other 16), and |r_x| / K |s| for the row sum taken from the hi + lo planes.
  l2norm  d(acc / |acc|)_j <= e_j / |acc| + |unit_j| (sum_i |unit_i| e_i) / |acc|, plus the f32 arithmetic of the norm and the products: NORM_ULPS = 36 ulps
          of the element (attn_fwd_reference.PREP_NORM_ULPS), all times |q_scale_j| scale.
Marks (bf16).  The kernel rounds the f32 value, the reference the f64 value: the two images differ only where the error above crosses a bf16 rounding tie.
An element is MARKED when its f64 value lies within twice its error of a tie.  pk_qkv_project: an unmarked element equals the reference's rounded value bit
for bit, a marked one may be one bf16 ulp (2^-8 of its binade's top) off (an element no larger than its own error, such as a fold that comes out 0:
the error plus an ulp).  MARK_CAP: at most 2 % of the image elements of a case are marked (host test).
Split-bf16 images: |got - ref| <= 2^-18 binade_top + 2 error (hi + lo leaves 2^-9 of 2^-9).
Bound of an output element (pk_qkv_attn, pk_q_attn_cached): attn_fwd_reference.terms() of the running-max form on the rounded images (p_round, score, exp,
accumulate; the normaliser adds the unrounded p: `ls += pr`), plus the image terms, both absolute: with ds = dQ |K|^T + |Q| dK^T, d o_i = sum_j p_ij ds_ij (v_j - o_i), so
img_score = (P . ds) |V| + A rowsum(P . ds); img_v = P dV; dQ, dK, dV = one bf16 ulp on the marked elements (bf16) | 2^-18 binade_top + 2 error (split-bf16);
|o - ref| <= 2 (terms A + img_score + img_v) + u_out binade_top(ref).

Not covered: PK_QKV_TM (a tuning variable read once per process; the GPU test refuses to run with it set), the cache-policy forms of the O store
(tests/test_cache_policy_gpu.py)."""
import math
import zlib
from types import SimpleNamespace

import torch

from tests import attn_fwd_reference as R

BF16, BF16X3 = R.BF16, R.BF16X3
T_NAME = {BF16: 'bf16', BF16X3: 'x3'}
U_F32, U_BF16, U_SPLIT = R.U_F32, R.U_BF16, R.U_SPLIT
NORM_ULPS = R.PREP_NORM_ULPS
FOLD_ULPS = 4
MARK_CAP = 0.02
MASS = R.MASS
EPS = 1e-12
SCALE_PROJECT = 8.0
SCALE_ATTN = 16.0
SCALE_CACHED = 10.0
NAN_BITS = 0x7FC1            # the int16 pattern the images of pk_qkv_project are pre-filled with: a bf16 NaN (and, twice, an f32 NaN)
KTILE = {BF16: 64, BF16X3: 32}
N_CU_TILES = 4 * 256         # qkv_project_launch: 128-row tiles once ceil(M / 128) * NT reaches this


def scale_of(c):
    return {'project': SCALE_PROJECT, 'attn': SCALE_ATTN, 'cached': SCALE_CACHED}[c.kernel]


def recip_identity(n, x):
    """QkvAttnArgs::recip: x / n == (x * ceil(65536 / n)) >> 16 (claimed for x < 64)"""
    return (x * ((65536 + n - 1) // n)) >> 16 == x // n


# ------------------------------------------------------------------------------------------------ cases

def _k(dtype, h, big=False):
    if big:
        return 72 if dtype == BF16 else 68
    if h == 1:
        return 136 if dtype == BF16 else 132
    return 392 if dtype == BF16 else 388


def _case(kernel, name, dtype, S, n, h, branch, *, fold=False, K=None, **kw):
    K = K or _k(dtype, h)
    assert K % KTILE[dtype] == (8 if dtype == BF16 else 4) and K > 2 * KTILE[dtype] or kw.get('big')
    c = SimpleNamespace(kernel=kernel, name=f'{kernel}_{T_NAME[dtype]}_{name}', dtype=dtype, S=S, n=n, h=h, K=K, ld=K + (16 if dtype == BF16 else 8), fold=fold,
                        branch=branch, nq=n, n_kv=n, nnull=0, bias=None, mask=None, causal=False, slopes=False, kv=True, big=False, fix=None, lse=False,
                        out_f32=dtype != BF16)
    c.__dict__.update(kw)
    return c


def branch_of(c):
    """host mirror of the dispatch of the three entry points, from the host-visible conditions alone"""
    T = T_NAME[c.dtype]
    fold = ':fold' if c.fold else ''
    if c.kernel == 'project':
        NT = 3 * c.h if c.kv else c.h
        tm = 2 if -(-c.S * c.n // 128) * NT >= N_CU_TILES else 1
        return f'project<{T},{tm}>:{"qkv" if c.kv else "q"}{fold}'
    if c.kernel == 'attn':
        whole = c.n == 64 and not c.causal
        bias = 'none' if c.bias is None else ('vec' if (whole and c.bias_ld % 4 == 0) else 'scalar')
        return f'qkv_attn<{T}>:{"whole" if whole else "masked"}:bias={bias}{":alibi" if (c.causal and c.slopes) else ""}{fold}'
    return f'q_attn_cached<{T},{"nk64" if c.nk_pad > 32 else "nk32"}>{":mask" if c.mask else ""}{fold}'


def project_cases():
    out = []
    for dt in (BF16, BF16X3):
        T = T_NAME[dt]

        def add(name, S, n, h, tm, **kw):
            kw.setdefault('nq_pad', R.pads(n, n, 0)[0])
            kw.setdefault('nk_pad', R.pads(n, n, 0)[1])
            kv = kw.get('kv', True)
            out.append(_case('project', name, dt, S, n, h, f'project<{T},{tm}>:{"qkv" if kv else "q"}{":fold" if kw.get("fold") else ""}', **kw))
        add('n37_m111', 3, 37, 2, 1)                                       # sequences straddle the 64-row tiles, nq_pad = 48 > n, nk_pad = 64 > n
        add('n200_m400_fold', 2, 200, 2, 1, fold=True)
        add('n43_m129_fold', 3, 43, 2, 1, fold=True)                       # M % 64 = 1
        add('n191_m191', 1, 191, 3, 1)                                     # M % 64 = 63
        add('n37_query_only_fold', 3, 37, 2, 1, fold=True, kv=False)
        # 128-row tiles: ceil(M / 128) * NT >= 1024.  Full form h = 16 (NT = 48): 22 row tiles; the same shapes with 21 take the 64-row form
        K = _k(dt, 16, big=True)
        add('tm2_m2728', 8, 341, 16, 2, K=K, big=True, fold=True)          # M % 128 = 40
        add('tm2_m2788', 17, 164, 16, 2, K=K, big=True)                    # M % 128 = 100
        add('tm1_m2600', 8, 325, 16, 1, K=K, big=True, fold=True)
        add('tm1_m2660', 20, 133, 16, 1, K=K, big=True)
        add('tm2_query_only_m4000', 16, 250, 32, 2, K=K, big=True, kv=False, fold=True)     # h = 32 (NT = 32): 32 row tiles
        add('tm1_query_only_m3872', 16, 242, 32, 1, K=K, big=True, kv=False, fold=True)     # 31
    return out


ATTN_SHORT_N = (1, 7, 9, 10, 21, 32, 33, 63)


def attn_cases():
    out = []
    for dt in (BF16, BF16X3):
        T = T_NAME[dt]

        def add(name, S, n, h, form, **kw):
            out.append(_case('attn', name, dt, S, n, h, f'qkv_attn<{T}>:{form}{":fold" if kw.get("fold") else ""}', **kw))
        add('n64_plain', 1, 64, 3, 'whole:bias=none')                                                   # one tile
        add('n64_vbias_fold', 8, 64, 1, 'whole:bias=vec', bias='vec', bias_ld=64, fold=True)            # 8 tiles
        add('n64_sbias', 9, 64, 1, 'whole:bias=scalar', bias='scalar', bias_ld=65)                      # 9 tiles
        add('n64_causal_fold', 2, 64, 3, 'masked:bias=none:alibi', causal=True, slopes=True, fold=True)
        for k, n in enumerate(ATTN_SHORT_N):
            spt = 64 // n
            S = spt + 1 if spt > 1 else 3                  # not a multiple of the sequences per tile
            h = 3 if k % 2 else 1
            add(f'n{n}_causal_alibi', S, n, h, 'masked:bias=none:alibi', causal=True, slopes=True, fold=k % 2 == 0)
            add(f'n{n}_causal_noslopes', S, n, 1 if h == 3 else 3, 'masked:bias=none', causal=True, fold=k % 2 == 1)
        add('n9_bias_9tiles', 57, 9, 1, 'masked:bias=scalar', bias='scalar', bias_ld=9, fold=True)      # ceil(57 / 7) = 9 tiles, the last holds one sequence
        add('n33_bias', 3, 33, 3, 'masked:bias=scalar', bias='vec', bias_ld=36)
        add('n10_bias_causal', 7, 10, 1, 'masked:bias=scalar:alibi', bias='scalar', bias_ld=10, causal=True, slopes=True)
    return out


def cached_cases():
    out = []
    for dt in (BF16, BF16X3):
        T = T_NAME[dt]

        def add(name, S, n, h, n_kv, nnull, mask=None, **kw):
            nk_pad = R.pads(n, n_kv, nnull)[1]
            out.append(_case('cached', name, dt, S, n, h, f'q_attn_cached<{T},{"nk64" if nk_pad > 32 else "nk32"}>{":mask" if mask else ""}'
                             f'{":fold" if kw.get("fold") else ""}', n_kv=n_kv, nnull=nnull, mask=mask, nk_pad=nk_pad, **kw))
        add('nk1', 3, 64, 1, 1, 0)                                         # 3 tiles
        add('nk13_null_mask_fold', 2, 128, 3, 11, 2, 'mask', fold=True)
        add('nk31_allmasked', 3, 64, 1, 31, 0, 'full')                     # nnull = 0: the last sequence has every key masked
        add('nk32_null_fullmask_fold', 2, 192, 3, 30, 2, 'full', fold=True)        # only the null keys remain
        add('nk33', 5, 64, 1, 33, 0)
        add('nk62_null_mask_fold', 2, 128, 3, 60, 2, 'mask', fold=True)
        add('nk64_null_fullmask', 3, 64, 3, 62, 2, 'full')
        add('nk64_fold', 1, 192, 1, 64, 0, fold=True)
        add('nk13_null', 9, 64, 1, 11, 2)                                  # 9 tiles
    return out


PROJECT_CASES, ATTN_CASES, CACHED_CASES = project_cases(), attn_cases(), cached_cases()
CASES = PROJECT_CASES + ATTN_CASES + CACHED_CASES


# ------------------------------------------------------------------------------------------------ inputs

def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _quant(t, step, lim):
    return (t / step).round().clamp(-lim, lim) * step


def _rows(c, vals, poison):
    """(M, ld) f32 rows with the slack columns poisoned"""
    buf = torch.full((vals.shape[0], c.ld), poison, dtype=torch.float32)
    buf[:, :c.K] = vals.float()
    return buf


def _finish_weights(c, x, g, Wq, Wkv, gamma=None):
    """to_q with the LayerNorm folded in (gamma a power of two per column: gamma (.) W stays exact), its s as attention.folded_weight builds it"""
    from phenaki_pytorch_amd import attention as A
    x.wkv = Wkv.float() if Wkv is not None else None
    x.gamma = None
    if c.fold:
        x.gamma = gamma if gamma is not None else 2.0 ** torch.randint(-1, 2, (c.K,), generator=g).float()
        x.wq_raw = Wq.float()
        wg, s, _, beta_zero = A.folded_weight(SimpleNamespace(), 'q_ln', lambda: x.wq_raw, x.gamma, None, c.dtype, [x.wq_raw, x.gamma])
        assert beta_zero
        x.wq = (x.wq_raw * x.gamma[None, :]).float()
        x.wq_packed, x.s = wg, s
        if c.dtype == BF16:
            assert torch.equal(wg[:, :c.K].float(), x.wq), 'gamma (.) W is exact in bf16'
    else:
        x.wq, x.s = Wq.float(), None
    x.q_scale = (1 + 0.05 * torch.randn(64, generator=g)).float()
    x.k_scale = (1 + 0.05 * torch.randn(64, generator=g)).float()


def _offset(c, rows, g):
    """the rows of the folded cases with mean / std about 4: every second row (bf16) or every row (split-bf16); returns (rows, mean4 (M,) bool)"""
    M = rows.shape[0]
    mean4 = torch.zeros(M, dtype=torch.bool)
    if not c.fold:
        return rows, mean4
    mean4[:] = True
    if c.dtype == BF16:
        mean4[0::2] = False
    std = rows.std(dim=1, keepdim=True)
    off = 4 * std - rows.mean(dim=1, keepdim=True)
    off = (off * 8).round() / 8                            # stays on the rows' grid
    return torch.where(mean4[:, None], rows + off, rows), mean4


def _row_scale(M, g):
    return 2.0 ** torch.randint(-1, 2, (M, 1), generator=g).float()


_ATTEMPT = {}


def build(c, poison=float('nan')):
    """the seeded inputs of a case.  Planted cases: the first of eight seeds (name/0 ..) whose f64 reference has the planted property -- two targets of a
    row can come out a factor e apart, which leaves the weaker one below MASS; the choice depends on the case alone"""
    if c.kernel == 'project':
        return _build_project(c, _gen(c.name), poison)
    known = _ATTEMPT.get(c.name)
    for a in (range(8) if known is None else (known,)):
        x = _build_planted(c, _gen(f'{c.name}/{a}'), poison)
        if known is None:
            try:
                R.planted_property(c, x, reference(c, x))
            except AssertionError:
                continue
        _ATTEMPT[c.name] = a
        return x
    raise AssertionError(f'{c.name}: no seed with the planted property')


def _build_project(c, g, poison):
    M, K, h = c.S * c.n, c.K, c.h
    x = SimpleNamespace()
    if c.dtype == BF16:
        rows = lambda: _quant(torch.randn(M, K, generator=g), 1 / 8, 24)
        Wq = _quant(torch.randn(h * 64, K, generator=g) * 0.25, 1 / 64, 120)
        Wkv = _quant(torch.randn(2 * h * 64, K, generator=g) * 0.25, 1 / 64, 120)
    else:                                                  # split-bf16: here the WEIGHTS have more than 8 significant bits (lo plane of W), the rows do not
        rows = lambda: _quant(torch.randn(M, K, generator=g), 1 / 8, 24)
        Wq = _quant(torch.randn(h * 64, K, generator=g) * 0.25, 1 / 4096, 8000)
        Wkv = _quant(torch.randn(2 * h * 64, K, generator=g) * 0.25, 1 / 4096, 8000)
    xq, x.mean4 = _offset(c, rows(), g)
    xq = xq * _row_scale(M, g)
    xkv = rows() * _row_scale(M, g)
    x.xq, x.xkv = _rows(c, xq, poison), (_rows(c, xkv, poison) if c.kv else None)
    _finish_weights(c, x, g, Wq, Wkv if c.kv else None)
    return x


def hadamard64():
    H = torch.ones(1, 1)
    for _ in range(6):
        H = torch.cat((torch.cat((H, H), dim=1), torch.cat((H, -H), dim=1)), dim=0)
    return H


def is_weak(c, i):
    """rows that carry no planted component: their softmax is nearly uniform over what they see, so a key admitted with score 0 takes real mass"""
    if c.causal:
        return i == 0
    return i % 4 == 3 and c.kernel == 'cached'


def _build_planted(c, g, poison):
    """module docstring, 'Planted attention'"""
    S, n, h, K = c.S, c.n, c.h, c.K
    Kh = K // 2
    assert Kh >= 64 * h
    cached = c.kernel == 'cached'
    nk = c.nnull + c.n_kv
    bf = c.dtype == BF16
    xstep = 1 / 8 if bf else 1 / 256                       # split-bf16: the rows have more than 8 significant bits (lo plane of A), the weights do not
    x = SimpleNamespace(bias=None, bias_buf=None, kmask=None, slopes=None)
    weak = torch.tensor([is_weak(c, i) for i in range(n)])
    # structure
    if c.bias is not None:
        x.bias_buf = torch.full((h, n, c.bias_ld), poison, dtype=torch.float32)
        b = torch.randn(h, n, n, generator=g) * 0.5
        if not c.causal:
            b[:, 3::4] -= 14.0                             # every fourth row far down, its target at about 2: a key admitted WITHOUT its bias (score 0) takes real mass
        x.bias_buf[:, :, :n] = b
        x.bias = x.bias_buf[:, :, :n]
    if c.mask is not None:
        km = torch.rand(S, c.n_kv, generator=g) < 0.7
        km[:, -1] = True
        km[:, 0] = c.n_kv == 1
        if c.mask == 'full':
            km[-1] = False
        x.kmask = km
    if c.causal:
        x.slopes = (2.0 ** -(5 + torch.arange(h))).float() if c.slopes else torch.zeros(h)
    _, masked = R.structure(c, x)                                           # (P, n, nk)
    x.vis = ~masked
    # weights: per head an isometry B = P H D / 8 on the head's 64 coordinates of a half; sparse noise everywhere else
    H = hadamard64()
    B = torch.zeros(h, 64, Kh)
    for hh in range(h):
        sign = (torch.randint(0, 2, (64,), generator=g) * 2 - 1).float()
        B[hh, :, hh * 64:hh * 64 + 64] = H[torch.randperm(64, generator=g)] * sign[None, :] / 8
    noise_w = lambda rows: _quant(torch.randn(rows, K, generator=g) * 0.006, 1 / 64, 2)
    Wq = noise_w(h * 64)
    Wq[:, Kh:2 * Kh] += B.reshape(h * 64, Kh)
    Wk = noise_w(h * 64)
    Wk[:, :Kh] += B.reshape(h * 64, Kh)
    Wv = _quant(torch.randn(h * 64, K, generator=g) * 0.25, 1 / 64, 120)
    Wv[:, K - 1] = (torch.randint(0, 2, (h * 64,), generator=g) * 2 - 1).float() * 0.5      # with xkv[:, K - 1] = 2: every v shares an offset, |o| is about A
    # key vectors: per (sequence, key) and head group a signed Hadamard row (exactly orthogonal within a sequence) plus noise
    nkeys = nk if cached else n
    u = _quant(torch.randn(S, nkeys, Kh, generator=g) * 0.25, xstep, 1024)
    spt = 64 // n if not cached else 1
    for s0 in range(0, S, spt):                            # the sequences of one 64-row tile share a basis: a forbidden neighbour key is orthogonal too
        for hh in range(h):
            sign = (torch.randint(0, 2, (64,), generator=g) * 2 - 1).float()
            rows = H[torch.randperm(64, generator=g)] * sign[None, :]
            for s in range(s0, min(s0 + spt, S)):
                u[s, :, hh * 64:hh * 64 + 64] += 2 * rows[(s - s0) * nkeys:(s - s0 + 1) * nkeys]
    # targets and forbidden keys of every (sequence, head, row)
    x.targets = torch.zeros(S * h, n, nk, dtype=torch.bool)
    cvec = _quant(torch.randn(S, n, Kh, generator=g) * 0.5, xstep, 1024)
    strong = [i for i in range(n) if not weak[i]]
    for s in range(S):
        for hh in range(h):
            p_ = s * h + hh
            gsl = slice(hh * 64, hh * 64 + 64)
            vis = x.vis[p_]
            for r, i in enumerate(strong):
                comp = []
                if cached:
                    seen = vis[i].nonzero().flatten().tolist()
                    dead = (~vis[i]).nonzero().flatten().tolist()
                    if seen:
                        comp += [(s, seen[(2 * r + k + 5 * hh + s) % len(seen)]) for k in range(min(2, len(seen)))]
                    ntgt = len(comp)
                    if dead and seen:
                        comp.append((s, dead[(i + hh) % len(dead)]))
                elif c.causal:
                    comp.append((s, i))
                    if i % 2 == 1:
                        comp.append((s, i - 1 - (hh + s + i // 3) % i))
                    ntgt = len(comp)
                    if i + 1 < n:
                        comp.append((s, i + 1))                                # the first key beyond the diagonal
                else:
                    comp.append((s, (i + 1 + hh + 3 * s) % n))
                    if i % 4 == 3:                                             # a second target: mass shared by two keys, so that a sharper softmax shows
                        comp.append((s, (i + 17 + hh) % n))
                    ntgt = len(comp)
                for (_, t) in comp[:ntgt]:
                    x.targets[p_, i, t] = True
                if not cached and spt > 1:                                     # a key of the neighbouring sequence of the same tile
                    s2 = s + 1 if (s % spt < spt - 1 and s + 1 < S) else (s - 1 if s % spt > 0 else None)
                    if s2 is not None:
                        comp.append((s2, (i + 3) % n))
                if comp:
                    cvec[s, i, gsl] = 0
                for k, (sa, t) in enumerate(dict.fromkeys(comp)):
                    part = u[sa, t, gsl].clone()
                    if not cached and k == 1 and ntgt == 2:
                        part[:24] = 0                                          # the second target well behind the first, whatever the noise
                    cvec[s, i, gsl] += part
    M = S * n
    noise = lambda w: _quant(torch.randn(M, w, generator=g), xstep, 1024)
    xq = torch.cat((noise(Kh), cvec.reshape(M, Kh), noise(K - 2 * Kh)), dim=1)
    gamma = None
    if c.fold:                                             # gamma = +-1 per column; the planted half is divided by it, so that gamma (.) Wq reads c_i as planted
        gamma = (torch.randint(0, 2, (K,), generator=g) * 2 - 1).float()
        xq = xq / gamma[None, :]
    xq, x.mean4 = _offset(c, xq, g)
    x.xq = _rows(c, xq * _row_scale(M, g), poison)
    if cached:
        x.xkv = None
        _finish_weights(c, x, g, Wq, None, gamma)
        # the cached images, written by the reference: K^ = round(l2norm(B u) k_scale), V random around a common offset; K^ pad rows poisoned
        P = S * h
        k = torch.einsum('hdk,snk->shnd', B.double(), u.double()).reshape(P, nk, 64)
        Kimg = k / k.norm(dim=-1, keepdim=True).clamp_min(EPS) * x.k_scale.double()
        V = torch.randn(P, nk, 64, generator=g) + (torch.randint(0, 2, (1, 1, 64), generator=g) * 2 - 1).float() * 1.5
        rt = (lambda t: t.float().to(torch.bfloat16).float()) if bf else (lambda t: t.float())
        x.K = torch.full((P, c.nk_pad, 64), poison)
        x.K[:, :nk] = rt(Kimg)
        x.Vt = torch.zeros(P, 64, c.nk_pad)               # the precondition of pk_q_attn_cached: V^T pad columns finite (pk_attn_prep: zeros)
        x.Vt[:, :, :nk] = rt(V).transpose(1, 2)
    else:
        xkv = torch.cat((u.reshape(M, Kh), noise(K - Kh)), dim=1)
        xkv[:, K - 1] = 2.0
        x.xkv = _rows(c, xkv * _row_scale(M, g), poison)
        _finish_weights(c, x, g, Wq, torch.cat((Wk, Wv), dim=0), gamma)
    return x


# ------------------------------------------------------------------------------------------------ projection, images

def _quantum(t):
    """per row the largest power of two in 2^-20 .. 2^8 that divides every element"""
    q = torch.full((t.shape[0],), 2.0 ** -20, dtype=torch.float64)
    for e in range(-19, 9):
        q = torch.where(((t / 2.0 ** e) % 1 == 0).all(dim=1), torch.full_like(q, 2.0 ** e), q)      # divisibility by 2^e is monotone in e
    return q


def _split(t):
    """(lo, r) of the split-bf16 image of f32 values: t = hi + lo + r"""
    hi = t.float().to(torch.bfloat16).double()
    lo = (t - hi).float().to(torch.bfloat16).double()
    return lo, t - hi - lo


def _raw(c, x, which):
    """the mutant-independent pieces of a projection, computed once per built case: x W^T, sum |x| |w|, exactness, the split-bf16 remainder"""
    cache = x.__dict__.setdefault('_raw', {})
    if which not in cache:
        rows, w = (x.xq, x.wq) if which == 'q' else (x.xkv, x.wkv)
        X, W = rows[:, :c.K].double(), w.double()
        assert torch.isfinite(X).all()
        r = SimpleNamespace(xw=X @ W.t(), mag=X.abs() @ W.abs().t(), rowsum=X.sum(dim=1), split=0.0, rx=0.0)
        qx, qw = _quantum(X), _quantum(W)
        r.exact = (r.mag < (2.0 ** 24) * qx[:, None] * qw[None, :]) & (X.abs().sum(dim=1) < 2.0 ** 24 * qx)[:, None]
        if c.dtype == BF16X3:                              # x = hi + lo + r: the lo.lo product is dropped, r never reaches the matrix core (nor the row sum)
            (lx, rx), (lw, rw) = _split(X), _split(W)
            r.split = lx.abs() @ lw.abs().t() + rx.abs() @ W.abs().t() + X.abs() @ rw.abs().t()
            r.rx = rx.abs().sum(dim=1)
        cache[which] = r
    return cache[which]


def project_error(c, x, which, s=None, Kmean=None, no_mean=False):
    """(acc, e): rounding points 1 and 2 and the error e_acc of the module docstring, (M, N) f64 each; which: 'q' (xq, wq) | 'kv' (xkv, wkv)"""
    K = c.K
    r = _raw(c, x, which)
    acc, mag_all, e_exact = r.xw, r.mag, torch.zeros_like(r.xw)
    if s is not None:
        ms = (r.rowsum / (Kmean or K))[:, None] * s.double()[None, :]
        if not no_mean:
            acc = acc - ms
        mag_all = r.mag + ms.abs()
        e_exact = FOLD_ULPS * U_F32 * (r.xw.abs() + ms.abs())
    e = torch.where(r.exact, e_exact, (K + FOLD_ULPS) * U_F32 * mag_all) + r.split
    if s is not None and c.dtype == BF16X3:
        e = e + (r.rx / K)[:, None] * s.double().abs()[None, :]
    return acc, e


def normed_error(acc, e, sc, scale):
    """rounding point 3 on (M, h, 64): (image values, their error)"""
    nrm = acc.norm(dim=-1, keepdim=True).clamp_min(EPS)
    unit = acc / nrm
    E = e / nrm + unit.abs() * (unit.abs() * e).sum(dim=-1, keepdim=True) / nrm + NORM_ULPS * U_F32 * unit.abs()
    f = sc.double() * scale
    return unit * f, E * f.abs()


def bf16_round(v):
    return v.float().to(torch.bfloat16).double()


def ulp_bf16(v):
    """the spacing of bf16 around v: 2^-8 of the top of its binade"""
    return 2.0 ** -8 * R.binade_top(v)


def tie_distance(v):
    """distance of |v| to the nearest midpoint between two neighbouring bf16 values (inf for 0)"""
    a = v.abs()
    ulp = torch.exp2(torch.floor(torch.log2(a)) - 7)
    f = a / ulp
    d = ((f - torch.floor(f)) - 0.5).abs() * ulp
    return torch.where(a > 0, d, torch.full_like(d, math.inf))


def image(c, v, E):
    """rounding point 4: (rounded image, marked, d = what an element may differ from the rounded image by)"""
    if c.dtype == BF16:
        marked = (E > 0) & ((tie_distance(v) <= 2 * E) | (v == 0))         # E = 0: both sides round the same exact value, a tie included
        ulp = ulp_bf16(v.abs() + 2 * E)
        d = torch.where(2 * E <= ulp / 2, ulp, 2 * E + ulp)            # an element at or below its own error (a folded 0): wherever the error puts it, rounded
        return bf16_round(v), marked, torch.where(marked, d, torch.zeros_like(v))
    return v, torch.zeros_like(v, dtype=torch.bool), 2.0 ** -18 * R.binade_top(v) + 2 * E + 1e-45


def heads(c, t, n=None):
    """(S n, h 64) -> (S h, n, 64)"""
    n = n or c.n
    return t.view(c.S, n, c.h, 64).permute(0, 2, 1, 3).reshape(c.S * c.h, n, 64)


PROJ_MUTANTS = ('fold_no_mean', 'fold_mean_over_ldw', 'k_scale_on_v', 'scale_on_k', 'vt_block_untransposed', 'query_only_writes_k')
ATTN_MUTANTS = ('drop_last_key', 'admit_next_sequence_key', 'causal_diag_late', 'causal_diag_early', 'alibi_no_slope', 'bias_tile_row',
                'mask_no_null_shift', 'admit_pad_key')
MUTANTS = PROJ_MUTANTS + ATTN_MUTANTS


def applies(m, c):
    attn, cached, proj = c.kernel == 'attn', c.kernel == 'cached', c.kernel == 'project'
    nk = c.nnull + c.n_kv
    solo = attn and c.n == 1                               # a single key: the softmax is 1 whatever q is
    return {'fold_no_mean': c.fold and not solo, 'fold_mean_over_ldw': c.fold and not solo,
            'k_scale_on_v': not cached and c.kv, 'scale_on_k': (proj and c.kv) or (attn and c.n >= 2),
            'vt_block_untransposed': (proj and c.kv) or (attn and c.n >= 2),
            'query_only_writes_k': proj and not c.kv,
            'drop_last_key': not proj,
            'admit_next_sequence_key': attn and c.n < 64 and 64 // c.n > 1,
            'causal_diag_late': attn and c.causal and c.n >= 2, 'causal_diag_early': attn and c.causal and c.n >= 2,
            'alibi_no_slope': attn and c.causal and c.slopes and c.n >= 2,
            'bias_tile_row': attn and c.bias is not None and 64 // c.n > 1,
            'mask_no_null_shift': cached and c.mask is not None and c.nnull > 0,
            'admit_pad_key': (attn and c.n < 64) or (cached and nk < c.nk_pad)}[m]


def images(c, x, mutant=None):
    """rounding points 1-4: namespace of Q, K, V (S h, n, 64) f64 ROUNDED images with their marks (mQ ..) and allowed differences (dQ ..)"""
    r = SimpleNamespace(K=None, V=None)
    M, h = c.S * c.n, c.h
    Kmean = -(-c.K // KTILE[c.dtype]) * KTILE[c.dtype] if mutant == 'fold_mean_over_ldw' else None
    scale = scale_of(c)
    acc, e = project_error(c, x, 'q', x.s, Kmean, no_mean=mutant == 'fold_no_mean')
    q, Eq = normed_error(acc.view(M, h, 64), e.view(M, h, 64), x.q_scale, scale)
    r.Q, r.mQ, r.dQ = (heads(c, t.reshape(M, h * 64)) for t in image(c, q, Eq))
    if c.kernel == 'cached' or not c.kv:
        return r
    acc, e = project_error(c, x, 'kv')
    k, Ek = normed_error(acc[:, :h * 64].reshape(M, h, 64), e[:, :h * 64].reshape(M, h, 64), x.k_scale, scale if mutant == 'scale_on_k' else 1.0)
    v, Ev = acc[:, h * 64:], e[:, h * 64:]
    if mutant == 'k_scale_on_v':
        v = (v.view(M, h, 64) * x.k_scale.double()).reshape(M, h * 64)
    r.K, r.mK, r.dK = (heads(c, t.reshape(M, h * 64)) for t in image(c, k, Ek))
    r.V, r.mV, r.dV = (heads(c, t) for t in image(c, v, Ev))
    if mutant == 'vt_block_untransposed':
        b = min(16, c.n)
        r.V = r.V.clone()
        r.V[:, :b, :b] = r.V[:, :b, :b].transpose(1, 2).clone()
    return r


# ------------------------------------------------------------------------------------------------ pk_qkv_project: the images themselves

def _to_layout(c, t, width):
    """(rows, width) bool / values per element -> per int16 of the raw image (split-bf16: blocks of 32 elements, [hi x 32 | lo x 32])"""
    if c.dtype == BF16:
        return t
    rows = t.shape[0]
    b = t.view(rows, width // 32, 32)
    return torch.cat((b, b), dim=-1).reshape(rows, 2 * width)


def encode(c, vals, width):
    """(rows, width) f64 / f32 values -> the raw int16 image of the case's type (what a kernel with exactly these values would leave)"""
    if c.dtype == BF16:
        return vals.float().to(torch.bfloat16).view(torch.int16)
    from phenaki_pytorch_amd import _lib
    return _lib.split_planes(vals.float().contiguous()).view(torch.int16)


def decode(c, raw, width):
    """raw int16 (rows, width | 2 width) -> f64 values"""
    if c.dtype == BF16:
        return raw.view(torch.bfloat16).double()
    return R.unsplit(raw.contiguous().view(torch.float32), width)


def empty_images(c):
    """(Qp, Kp, Vt) int16 buffers of the NaN pattern, exactly as long as the contract names: (S h nq_pad, 64), (S h nk_pad, 64), (S h 64, nk_pad) elements"""
    P, e = c.S * c.h, 1 if c.dtype == BF16 else 2
    full = lambda rows, w: torch.full((rows, w * e), NAN_BITS, dtype=torch.int16)
    return full(P * c.nq_pad, 64), full(P * c.nk_pad, 64), full(P * 64, c.nk_pad)


def place(c, ref, bufs=None):
    """the reference's images laid into pattern-filled buffers: what a perfect pk_qkv_project leaves"""
    Qp, Kp, Vt = bufs or empty_images(c)
    P, n = c.S * c.h, c.n
    e = 1 if c.dtype == BF16 else 2
    Qp.view(P, c.nq_pad, 64 * e)[:, :n] = encode(c, ref.Q.reshape(P * n, 64), 64).view(P, n, 64 * e)
    if ref.K is not None:
        Kp.view(P, c.nk_pad, 64 * e)[:, :n] = encode(c, ref.K.reshape(P * n, 64), 64).view(P, n, 64 * e)
        vt = torch.zeros(P * 64, c.nk_pad, dtype=torch.float64)
        vt[:, :n] = ref.V.transpose(1, 2).reshape(P * 64, n)
        written = torch.zeros(P * 64, c.nk_pad, dtype=torch.bool)
        written[:, :n] = True
        Vt[:] = torch.where(_to_layout(c, written, c.nk_pad), encode(c, vt, c.nk_pad), Vt)
    return Qp, Kp, Vt


def check_project(c, ref, Qp, Kp, Vt):
    """Qp, Kp, Vt: the WHOLE raw int16 buffers (cpu).  Pad rows / columns (and, query-only, all of Kp / Vt) still hold the pattern bit for bit; every written
    element is finite; bf16: unmarked elements equal the reference bit for bit, marked ones within one ulp; split-bf16: within the image bound.
    Returns {image: (worst err / bound, share of marked elements)}."""
    P, n = c.S * c.h, c.n
    e = 1 if c.dtype == BF16 else 2
    out = {}

    def held(what, got, want, marked, d):
        bad = ~torch.isfinite(got)
        assert not bad.any(), f'{c.name} {what}: {int(bad.sum())} non-finite / unwritten elements, first at {bad.nonzero()[0].tolist()}'
        err = (got - want).abs()
        if c.dtype == BF16:
            wrong = (err > d)
            ratio = torch.where(marked, err / d.clamp_min(1e-300), (err > 0).double() * 2)
        else:
            wrong = err > d
            ratio = err / d
        if wrong.any():
            i = wrong.nonzero()[0].tolist()
            raise AssertionError(f'{c.name} {what}: element {i} is {got[tuple(i)]:.9g}, reference {want[tuple(i)]:.9g} ({"marked" if marked[tuple(i)] else "unmarked"}, '
                                 f'allowed {d[tuple(i)]:.3e}); {int(wrong.sum())} elements beyond their bound')
        out[what] = (ratio.max().item(), marked.double().mean().item())

    q = Qp.view(P, c.nq_pad, 64 * e)
    assert (q[:, n:] == NAN_BITS).all(), f'{c.name}: pad query rows {n} .. {c.nq_pad - 1} of Qp were written'
    held('Qp', decode(c, q[:, :n].reshape(P * n, 64 * e), 64).view(P, n, 64), ref.Q, ref.mQ, ref.dQ)
    if ref.K is None:
        assert (Kp == NAN_BITS).all() and (Vt == NAN_BITS).all(), f'{c.name}: the query-only form wrote a K^ / V^T image'
        return out
    k = Kp.view(P, c.nk_pad, 64 * e)
    assert (k[:, n:] == NAN_BITS).all(), f'{c.name}: pad key rows {n} .. {c.nk_pad - 1} of Kp were written'
    held('Kp', decode(c, k[:, :n].reshape(P * n, 64 * e), 64).view(P, n, 64), ref.K, ref.mK, ref.dK)
    written = torch.zeros(P * 64, c.nk_pad, dtype=torch.bool)
    written[:, :n] = True
    wl = _to_layout(c, written, c.nk_pad)
    assert (Vt[~wl] == NAN_BITS).all(), f'{c.name}: pad key columns {n} .. {c.nk_pad - 1} of Vt were written'
    vt = decode(c, torch.where(wl, Vt, torch.zeros_like(Vt)), c.nk_pad)[:, :n]
    tr = lambda t: t.transpose(1, 2).reshape(P * 64, n)
    held('Vt', vt, tr(ref.V), tr(ref.mV), tr(ref.dV))
    return out


def marked_share(ref):
    ms = [m for m in (ref.mQ, getattr(ref, 'mK', None), getattr(ref, 'mV', None)) if m is not None]
    return sum(int(m.sum()) for m in ms) / sum(m.numel() for m in ms)


# ------------------------------------------------------------------------------------------------ attention on the rounded images

def attend(c, x, Q, K, V, mutant=None):
    """attn_fwd_reference.attend with the mutants of the fused kernels: Q (P, n, 64), K, V (P, nk, 64) f64"""
    P, nk = c.S * c.h, K.shape[1]
    xs = x
    smut = mutant if mutant in ('causal_diag_late', 'causal_diag_early', 'mask_no_null_shift') else None
    if mutant == 'alibi_no_slope':
        xs = SimpleNamespace(**{**x.__dict__, 'slopes': torch.ones(c.h)})
    add, masked = R.structure(c, xs, smut)
    if mutant == 'bias_tile_row':                          # bias[h][row of the 64-row tile] in place of bias[h][position in the sequence]; rows past n: the last
        hh = torch.arange(P) % c.h
        first = (torch.arange(P) // c.h) % (64 // c.n) * c.n
        row = (first[:, None] + torch.arange(c.n)[None, :]).clamp_max(c.n - 1)                  # (P, n)
        add = add - x.bias.double()[hh] + x.bias.double()[hh[:, None], row]
    sim = Q @ K.transpose(1, 2) + add
    sim = torch.where(masked, torch.full_like(sim, R.NEG_MAX), sim)
    if mutant == 'drop_last_key':
        sim[:, :, -1] = -math.inf
    if mutant == 'admit_pad_key':
        sim = torch.cat((sim, torch.zeros_like(sim[:, :, :1])), dim=2)
        V = torch.cat((V, torch.zeros_like(V[:, :1])), dim=1)
    if mutant == 'admit_next_sequence_key':                # key 0 of the neighbouring sequence of the tile, same head
        spt, S, h = 64 // c.n, c.S, c.h
        s = torch.arange(P) // h
        s2 = torch.where((s % spt < spt - 1) & (s + 1 < S), s + 1, s - 1)
        ok = (s2 >= 0) & (s2 // spt == s // spt)
        p2 = s2.clamp_min(0) * h + torch.arange(P) % h
        key = (torch.arange(c.n) + 3) % c.n                # per query row the neighbour's key its forbidden component points at
        k2, v2 = K[p2][:, key], V[p2][:, key]              # (P, n, 64)
        s_x = (Q * k2).sum(-1, keepdim=True)
        s_x = torch.where(ok[:, None, None], s_x, torch.full_like(s_x, -math.inf))
        m = torch.maximum(sim.max(-1, keepdim=True).values, s_x)
        pe, px = (sim - m).exp(), (s_x - m).exp()
        den = pe.sum(-1, keepdim=True) + px
        prob = pe / den
        O = prob @ V + px / den * v2
        A = prob @ V.abs() + px / den * v2.abs()
        return SimpleNamespace(O=R.to_rows(c, O), A=R.to_rows(c, A), prob=prob, sim=sim, add=add, lse=torch.logsumexp(sim, dim=-1))
    prob = sim.softmax(-1)
    return SimpleNamespace(O=R.to_rows(c, prob @ V), A=R.to_rows(c, prob @ V.abs()), prob=prob, sim=sim, add=add, lse=torch.logsumexp(sim, dim=-1))


def reference(c, x, mutant=None):
    """the whole restatement.  project: the images namespace; attn / cached: the attention namespace (O, A (S n, h 64), prob, ...) with .img = the images"""
    img = images(c, x, mutant if mutant in PROJ_MUTANTS else None)
    if c.kernel == 'project':
        return img
    nk = c.nnull + c.n_kv
    if c.kernel == 'cached':
        K, V = x.K[:, :nk].double(), x.Vt[:, :, :nk].double().transpose(1, 2)
    else:
        K, V = img.K, img.V
    ref = attend(c, x, img.Q, K, V, mutant if mutant in ATTN_MUTANTS else None)
    ref.img, ref.K, ref.V = img, K, V
    return ref


def bound(c, x, ref):
    """(bound (S n, h 64), terms): module docstring, 'Bound of an output element'"""
    img = ref.img
    t = R.terms(c, x, ref, img.Q, ref.K)
    ds = img.dQ @ ref.K.abs().transpose(1, 2)
    dV = None
    if c.kernel == 'attn':
        ds = ds + img.Q.abs() @ img.dK.transpose(1, 2)
        dV = img.dV
    # d o_i = sum_j p_ij ds_ij (v_j - o_i): |d o| <= (P . ds) |V| + A rowsum(P . ds)
    w = ref.prob * ds
    t['img_score'] = R.to_rows(c, w @ ref.V.abs()) + R.to_rows(c, w.sum(-1, keepdim=True).expand(-1, -1, 64).contiguous()) * ref.A
    t['img_v'] = R.to_rows(c, ref.prob @ dV) if dV is not None else torch.zeros_like(ref.O)
    first = t['p_round'] + t['norm'] + t['score'] + t['exp'] + t['accumulate']
    u_out = 0.0 if c.out_f32 else U_BF16
    return 2 * (first * ref.A + t['img_score'] + t['img_v']) + u_out * R.binade_top(ref.O) + 1e-30, t


def largest_term(c, ref, t):
    rel = {k: (v if isinstance(v, float) else v.max().item()) for k, v in t.items() if k not in ('lse', 'img_v', 'img_score')}
    for k in ('img_v', 'img_score'):
        rel[k] = torch.where(ref.A > 0, t[k] / ref.A.clamp_min(1e-300), torch.zeros_like(ref.A)).max().item()
    return max(rel, key=rel.get), rel
