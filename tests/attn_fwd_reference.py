"""Float64 restatement of the inference attention forward (csrc/attn.hip: pk_attn_prep, pk_attn_fwd, pk_attn_small), the seeded cases that reach every
branch of attn_fwd_impl, and a per-element checker whose bound is derived from the kernels' rounding points.  CPU only; tests/test_attn_fwd_host.py shows
what the checker rejects, tests/test_attn_fwd_gpu.py runs the kernels against it.

Inputs.  For pk_attn_fwd the operand IMAGES are written here (Qp (S h, nq_pad, 64), Kp (S h, nk_pad, 64), Vt (S h, 64, nk_pad)), so no prep kernel sits
between the input and the check.  dtype 1: values exactly representable in bf16; dtypes 0 / 2: f32 values (the test lays dtype 2 down with
_lib.split_planes).  Pad query rows, pad key rows / columns and the slack columns of a bias matrix are poisoned (NaN, +Inf in a second pass).

Planted attention.  Random scores give near-uniform softmax rows, under which a dropped key hides below the rounding bound.  So a query row carries, on
top of noise, components along up to three keys' directions (`targets`), dealt from the LAST key backwards and rotated with the row and the pair; the last
8 head dims hold a constant that shifts every score by -GAMMA, so the targets score about +1, every other key about -7, and a row's normaliser is O(1)
(a pad key admitted with score 0 is then visible too).  Causal rows also carry a component along the first key BEYOND their diagonal and masked
sequences along a masked key (`forbidden`): were the kernel to admit it, it would take real mass.  planted_property() states what must hold and the host
test asserts it: every visible key of every pair holds >= MASS of the f64 softmax of some query row of that pair; where a pair has fewer query rows than
visible keys, every visible key of the pair's last 64-key tile does, and every key does in the union over the pairs.

Reference.  sim = Q K^T + bias (a matrix, or a table gathered through pos_code), ALiBi slope and causal mask with dj = j - (i + n_kv - nq) over the null
keys too (j < 0), key mask over the real keys only, masked scores = -finfo(float32).max as in the model (a fully masked sequence attends uniformly to
all its keys).  reference() returns O, lse and A = softmax @ |V|.

Bound.  |o - ref| <= 2 (sum of the first-order terms) A + u_out |ref| per element; the factor 2 covers the second-order terms.  The terms, each a
relative perturbation of o in units of A (terms() below; the kernel expression each comes from is named here):
  p_round    P is rounded to the MFMA operand type before the PV product (frag_from_f32 in attn_fwd_kernel / attn_fwd_lds_kernel): 2^-9 for bf16
             (RNE, v_cvt_pk_bf16_f32; a p at the lower end of its binade is off by up to 2^-8 of itself, which the factor 2 then pays for: the
             bf16 cases measure up to 0.8 of the bound where a row's weight sits on few keys), 0 for f32, 3 * 2^-16 for split-bf16 (x = hi + lo
             leaves 2^-8 of 2^-8 |x| at the lower ends of both binades: once for P, once for V, and the lo.lo product is dropped).
  norm       the normaliser.  Running-max forms add the UNROUNDED p in f32 (`ls += pr`): covered by `accumulate`.  Fixed-offset forms take it from
             the matrix core as the sum of the ROUNDED p (`lsum = mma(ones, fp)`): numerator and normaliser move separately, one more p_round
             (|o| <= A).
  score      the f32 accumulation of a 64-term score (MFMA; products of bf16 are exact in f32) and the f32 additions of the bias and the ALiBi term:
             (64 + 3) 2^-24 (sum_d |q_d| |k_d| + |bias| + |ALiBi|), maximised over the row's keys; split-bf16 adds 3 * 2^-16 of the same sum (two
             operand splits and the dropped lo.lo).  A score error d moves o by at most 2 d A (p_j and the normaliser).
  exp        __expf(x) = v_exp_f32(x * log2e): the product's rounding is |x| 2^-24 relative in p, the instruction 1 ulp, the constant 2^-25:
             (3 + |x|) 2^-24 with |x| <= 24 ln 2 for every key that keeps a weight above 2^-24 of the row's largest (smaller ones are below the
             bound by themselves).  The fixed-offset form rounds fma(s, log2e, tab - off2) at magnitude |s| log2e + off2 (+ the table entry's own
             rounding): its |x| is ln 2 (off2 + max |sim + bias| log2e), twice with the table.  Numerator and normaliser: twice.
  accumulate the f32 sums over the keys (PV accumulators, l), the alpha rescale of every tile (an __expf and a product, 3 roundings), 1 / l and the
             final product: (nk + 3 tiles + 3) 2^-24.
u_out = 2^-9 for bf16 output, 0 for f32 output.  The output term is taken at the upper end of ref's binade, u_out 2^ceil(log2 |ref|): round-to-nearest
to bf16's 8 significant bits is half an ulp, which is 2^-9 of the binade's upper end and up to 2^-8 of the value itself (1.0039 lies 2^-8 from both of
its neighbours); pk_attn_small with one key copies V, so no kernel could meet u_out |ref| there.
lse = m + log l is held to the ABSOLUTE bound 2 (score / 2 + exp / 2 + accumulate + norm + 2^-21 (v_log_f32 and the ln 2 product) + 2^-23 |lse|).
pk_attn_small runs every product in f32 VALU arithmetic: the same terms with p_round = norm = 0 and the l2norm of its operands in `score`
(SMALL_NORM_ULPS).

Not covered: the forms reachable only through the tuning environment variables PK_ATTN_LDS_QF, PK_ATTN_PF and PK_ATTN_MAX_QF (read once per process), the
dropout forward (tests/test_dropout_gpu.py), head widths 32 and 128 (tests/test_dim_head_gpu.py).  The backward kernels (csrc/attn_train.hip) are held the
same way by tests/attn_bwd_reference.py, which builds on this module.  The fused projection kernels of qkv.hip / qkv_attn.hip are held
the same way by tests/qkv_reference.py, which builds on this module."""
import math
import zlib
from types import SimpleNamespace

import numpy as np
import torch

F32, BF16, BF16X3 = 0, 1, 2
DTYPE_NAME = {F32: 'f32', BF16: 'bf16', BF16X3: 'x3'}
NEG_MAX = -torch.finfo(torch.float32).max
U_BF16, U_F32, U_SPLIT = 2.0 ** -9, 2.0 ** -24, 2.0 ** -16
MASS = 0.25                      # the planted property
G0, GAMMA, NOFF = 8.0, 7.0, 8    # planted score before the shift, the shift, head dims that carry it
MAX_TARGETS = 3
NOMINAL_CUS = 256                # the host tests build the CU-dependent cases for this count


def pads(nq, n_kv, nnull):
    """pk_attn_pads (the GPU test asserts the two agree)"""
    r = 64 if nq >= 256 else (32 if nq >= 128 else 16)
    return -(-nq // r) * r, -(-(nnull + n_kv) // 32) * 32


# ------------------------------------------------------------------------------------------------ cases

def _case(name, dtype, S, h, nq, n_kv, branch, *, nnull=0, bias=None, dims=None, run4=False, mask=None, causal=False, out_f32=None, lse=False, fix=None):
    """bias: None | 'vec' (16-byte loadable rows) | 'scalar' (bias_ld % 4 != 0) | 'table' (dims, run4); mask: None | 'mask' | 'full' (the last sequence fully
    masked); fix: None (running max) | 'tight' | 'loose' (score_bound + 12)"""
    assert bias in (None, 'vec', 'scalar', 'table') and mask in (None, 'mask', 'full') and fix in (None, 'tight', 'loose')
    if bias == 'table':
        assert dims[0] * dims[1] * dims[2] == nq == n_kv and nnull == 0 and (not run4 or dims[2] % 4 == 0)
    return SimpleNamespace(name=name, dtype=dtype, S=S, h=h, nq=nq, n_kv=n_kv, nnull=nnull, bias=bias, dims=dims, run4=run4, mask=mask, causal=causal,
                           out_f32=(dtype != BF16) if out_f32 is None else out_f32, lse=lse, fix=fix, branch=branch)


def branch_of(c, n_cu, pad=None):
    """host mirror of attn_fwd_impl's dispatch (dim_head 64, no dropout, no tuning variables): the instantiation a case launches, from the host-visible
    conditions alone.  lds<QF,PF,TAB,FIX,T> is attn_fwd_lds_kernel, free<T,QF> is attn_fwd_kernel."""
    nq_pad, nk_pad = pad or pads(c.nq, c.n_kv, c.nnull)
    nk = c.nnull + c.n_kv
    tab = c.bias == 'table'
    fix = c.fix is not None and c.mask is None and not c.causal and c.bias in (None, 'table')
    if c.dtype == BF16 and (not c.lse or (not tab and c.fix is None)) and nk >= 64 and c.nq >= 64:
        wgs16 = c.S * c.h * -(-nq_pad // 64)
        qf = 2 if (fix and wgs16 > 3 * n_cu and c.nq >= 128) else 1
        pf = qf == 1 and nk_pad >= 192
        if fix or tab:
            return f'lds<{qf},0,{int(tab)},{int(fix)},bf16>'
        return f'lds<{qf},{int(pf)},0,0,bf16>'
    if c.dtype == BF16X3 and not c.lse and nk >= 64 and c.nq >= 128 and fix and c.out_f32:
        return f'lds<2,0,{int(tab)},1,x3>'
    if (c.dtype == BF16X3 and c.lse and c.nnull == 0 and c.nq == c.n_kv and c.nq >= 128 and c.mask is None and not c.causal and c.out_f32 and not tab
            and c.bias in (None, 'vec')):
        wg2, wg3 = c.S * c.h * -(-nq_pad // 128), c.S * c.h * -(-nq_pad // 192)
        return f'lds<{3 if (wg2 > n_cu and wg3 <= n_cu) else 2},0,0,0,x3>'
    assert not tab, 'the table form exists in the LDS-staged kernel only'
    qf = min(4 if (c.nq >= 256 and c.dtype == BF16) else (2 if c.nq >= 128 else 1), 2)
    return f'free<{DTYPE_NAME[c.dtype]},{qf}>'


def _lds_cases():
    """dtype 1, LDS-staged, running max: nk in {64, 65, 96, 160, 191, 192, 224} x nq in {64, 65, 130, 200}; PF switches on at nk_pad >= 192"""
    B = BF16
    pf = lambda nk: int(pads(64, nk, 0)[1] >= 192)
    out = []
    k = 0

    def add(tag, nq, nk, **kw):
        nonlocal k
        nn = kw.get('nnull', 0)
        kw.setdefault('out_f32', k % 2 == 1)
        kw.setdefault('lse', k % 3 == 2)
        k += 1
        out.append(_case(f'lds_{tag}_q{nq}_k{nk}', B, 2, 3, nq, nk - nn, f'lds<1,{pf(nk)},0,0,bf16>', **kw))
    for nq, nk in ((64, 64), (65, 65), (130, 96), (200, 160), (64, 191), (65, 192), (130, 224), (200, 191)):
        add('plain', nq, nk)
    for nq, nk in ((64, 64), (65, 96), (130, 160), (200, 192), (130, 191), (64, 224), (65, 65)):
        add('vbias', nq, nk, bias='vec')
    for nq, nk in ((65, 65), (130, 191), (64, 192), (200, 160)):
        add('sbias', nq, nk, bias='scalar', nnull=2)
    for nq, nk in ((64, 65), (130, 160), (200, 224), (65, 192)):
        add('mask', nq, nk, mask='full')
    for nq, nk in ((64, 64), (65, 65), (64, 96), (130, 191), (200, 224), (65, 160)):
        add('causal', nq, nk, causal=True)
    add('causal_null', 65, 96, causal=True, nnull=2)
    add('causal_null', 192, 194, causal=True, nnull=2)
    for nq, nk in ((64, 64), (130, 160), (200, 224), (65, 191)):
        add('null_mask_bias', nq, nk, nnull=2, mask='mask', bias='scalar')
    add('null_fullmask_bias', 130, 192, nnull=2, mask='full', bias='scalar')
    return out


def _table_cases():
    out = []
    for dims in ((2, 5, 7), (3, 8, 8), (2, 9, 12)):
        n = dims[0] * dims[1] * dims[2]
        for run4 in ((False, True) if dims[2] % 4 == 0 else (False,)):
            for fix in (None, 'tight', 'loose'):
                out.append(_case(f'tab_{"x".join(map(str, dims))}_{"run4" if run4 else "gather"}_{fix or "runmax"}', BF16, 2, 3, n, n,
                                 f'lds<1,0,1,{int(fix is not None)},bf16>', bias='table', dims=dims, run4=run4, fix=fix, out_f32=(fix == 'loose')))
    for nq, nk, fix in ((64, 64, 'tight'), (65, 96, 'tight'), (130, 191, 'loose'), (200, 224, 'tight')):
        out.append(_case(f'fix_plain_q{nq}_k{nk}_{fix}', BF16, 2, 3, nq, nk, 'lds<1,0,0,1,bf16>', fix=fix, out_f32=(nq == 130)))
    return out


def wide_cases(n_cu):
    """dtype 1, fixed offset: the 128-row workgroups need S h ceil(nq_pad / 64) > 3 CUs; the same shape with S h at the threshold takes the 64-row form"""
    out = []
    for n, dims in ((128, (2, 8, 8)), (160, (5, 4, 8))):
        blocks = -(-pads(n, n, 0)[0] // 64)
        T = 3 * n_cu // blocks                             # S h <= T: 64-row workgroups
        for tab in (False, True):
            for wide in (True, False):
                S = T // 2 + (1 if wide else 0)
                out.append(_case(f'wide_n{n}_{"tab" if tab else "plain"}_{"128row" if wide else "64row"}', BF16, S, 2, n, n,
                                 f'lds<{2 if wide else 1},0,{int(tab)},1,bf16>', bias='table' if tab else None, dims=dims if tab else None,
                                 run4=tab, fix='tight'))
    return out


def train_cases(n_cu):
    """dtype 2 with lse, self-attention: the LDS-staged running-max kernel with 64 or 48 query rows per wave (48: wg2 > CUs >= wg3)"""
    out = [_case('x3_lse_q130_vbias', BF16X3, 2, 3, 130, 130, 'lds<2,0,0,0,x3>', bias='vec', lse=True)]
    S = n_cu // 4 + 1                                      # n = 130: nq_pad = 160, two 128-row or one 192-row workgroup per pair
    out.append(_case('x3_lse_q130_qf3', BF16X3, S, 2, 130, 130, 'lds<3,0,0,0,x3>', lse=True))
    return out


def _free_cases():
    """the LDS-free kernel, every dtype: fewer than 64 keys (16 and 32 query rows per wave) or fewer than 64 query rows"""
    out = []
    for dt in (F32, BF16, BF16X3):
        T = DTYPE_NAME[dt]
        f = lambda qf: f'free<{T},{qf}>'
        k = len(out)
        out += [
            _case(f'free_{T}_q9_k20_vbias', dt, 2, 3, 9, 20, f(1), bias='vec', lse=True),
            _case(f'free_{T}_q37_k50_null_mask_bias', dt, 2, 3, 37, 48, f(1), nnull=2, mask='full', bias='scalar'),
            _case(f'free_{T}_q130_k33_null_mask', dt, 2, 3, 130, 31, f(2), nnull=2, mask='mask', lse=True),
            _case(f'free_{T}_q260_k63_vbias', dt, 2, 2, 260, 63, f(2), bias='vec'),
            _case(f'free_{T}_q37_k200_causal', dt, 2, 3, 37, 200, f(1), causal=True),
            _case(f'free_{T}_q63_k200_null_mask_bias', dt, 2, 3, 63, 198, f(1), nnull=2, mask='full', bias='scalar', lse=True),
            _case(f'free_{T}_q37_k37_causal', dt, 2, 3, 37, 37, f(1), causal=True),
            _case(f'free_{T}_q40_k42_causal_null', dt, 2, 3, 40, 40, f(1), causal=True, nnull=2),
            _case(f'free_{T}_q130_k50_plain', dt, 2, 3, 130, 50, f(2)),
        ]
        if dt == BF16:
            for c in out[k::2]:
                c.out_f32 = True
    return out


def _x3_cases():
    return [_case('x3_fix_q128_k192', BF16X3, 2, 3, 128, 192, 'lds<2,0,0,1,x3>', fix='tight'),
            _case('x3_fix_q200_k191', BF16X3, 2, 3, 200, 191, 'lds<2,0,0,1,x3>', fix='loose'),
            _case('x3_fix_tab_2x9x12', BF16X3, 2, 3, 216, 216, 'lds<2,0,1,1,x3>', bias='table', dims=(2, 9, 12), run4=True, fix='tight'),
            _case('x3_fix_tab_2x5x13', BF16X3, 2, 2, 130, 130, 'lds<2,0,1,1,x3>', bias='table', dims=(2, 5, 13), fix='tight')]


FIXED_CASES = _lds_cases() + _table_cases() + _free_cases() + _x3_cases()


def cu_cases(n_cu):
    return wide_cases(n_cu) + train_cases(n_cu)


# ------------------------------------------------------------------------------------------------ inputs

def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _rt(c):
    """values the operand image of the case's dtype holds exactly"""
    return (lambda t: t.to(torch.bfloat16).to(torch.float32)) if c.dtype == BF16 else (lambda t: t.to(torch.float32))


def table_codes(dims):
    """(pos_code (n,) int64, offset, table length) of the relative-position form: bias[h][i][j] = tab[h][code[i] - code[j] + offset]"""
    strides, acc = [], 1
    for d in reversed(dims):
        strides.insert(0, acc)
        acc *= 2 * d - 1
    grids = torch.meshgrid(*[torch.arange(d) for d in dims], indexing='ij')
    code = sum(g.reshape(-1) * st for g, st in zip(grids, strides))
    return code, sum((d - 1) * st for d, st in zip(dims, strides)), acc


def structure(c, x, mutant=None):
    """(add, masked), both (S h, nq, nk): the additive score terms (bias, ALiBi) in f64 and the mask, as the model defines them -- or as a mutant would"""
    P, nk = c.S * c.h, c.nnull + c.n_kv
    hh = torch.arange(P) % c.h
    ss = torch.arange(P) // c.h
    add = torch.zeros(P, c.nq, nk, dtype=torch.float64)
    masked = torch.zeros(P, c.nq, nk, dtype=torch.bool)
    j = torch.arange(nk) - c.nnull                                                  # real-key index, < 0 on the null keys
    if x.bias is not None:
        b = x.bias.double()                                                         # (h, nq, n_kv)
        if mutant == 'bias_head0':
            b = b[:1].expand_as(b)
        if mutant == 'bias_col_null_shift':                                         # bias[i][key] in place of bias[i][j]
            b = torch.cat((b[:, :, c.nnull:], torch.zeros(c.h, c.nq, c.nnull, dtype=torch.float64)), dim=2)
        add[:, :, c.nnull:] += b[hh]
    if x.kmask is not None:
        km = x.kmask
        if mutant == 'mask_no_null_shift':                                          # kmask[key] in place of kmask[j]
            km = torch.cat((km[:, c.nnull:], torch.ones(c.S, c.nnull, dtype=torch.bool)), dim=1)
        masked[:, :, c.nnull:] |= ~km[ss][:, None, :]
    if c.causal:
        coff = 0 if mutant == 'causal_no_offset' else c.n_kv - c.nq
        dj = j[None, :] - (torch.arange(c.nq)[:, None] + coff)                      # (nq, nk)
        ali = dj.abs().double()[None] * x.slopes.double()[hh][:, None, None]
        if mutant == 'alibi_skips_null':
            ali[:, :, :c.nnull] = 0
        add -= ali
        masked |= (dj > 1 if mutant == 'causal_diag_late' else (dj >= 0 if mutant == 'causal_diag_early' else dj > 0))[None]
    return add, masked


def _assign(vis, max_targets):
    """targets (P, nq, nk) bool: the visible keys dealt to query rows from the LAST key backwards, at most max_targets per row, the row rotated with
    the key and the pair.  A pair with at least as many rows as visible keys covers them all; another covers its last 64-key tile, and the remaining keys
    are shared out over the pairs."""
    vis = vis.numpy()
    P, nq, nk = vis.shape
    vis_any = vis.any(1)
    whole = nq >= vis_any.sum(1)
    tail0 = 64 * ((nk - 1) // 64)
    load = np.zeros((P, nq), dtype=np.int64)
    tgt = np.zeros_like(vis)
    rows, pidx = np.arange(nq), np.arange(P)
    BIG = 1 << 40

    def place(key, pairs, r):
        cand = vis[:, :, key] & (load < max_targets) & pairs[:, None]
        cost = np.where(cand, load * nq + (rows[None, :] - r - 7 * pidx[:, None]) % nq, BIG)
        row = cost.argmin(1)
        ok = cost[pidx, row] < BIG
        tgt[pidx[ok], row[ok], key] = True
        load[pidx[ok], row[ok]] += 1

    for r in range(nk):
        key = nk - 1 - r
        place(key, vis_any[:, key] & (whole | (key >= tail0)), r)
    for r in range(nk):
        key = nk - 1 - r
        if vis_any[:, key].any() and not tgt[:, :, key].any():
            can = (vis[:, :, key] & (load < max_targets)).any(1)
            if can.any():
                p = np.where(can, load.sum(1), BIG).argmin()
                place(key, pidx == p, r)
    return torch.from_numpy(tgt)


def _forbidden(c, x, masked):
    """(P, nq, nk) bool: per row one key it must NOT see -- the first beyond the causal diagonal, else a key its sequence masks"""
    P, nk = c.S * c.h, c.nnull + c.n_kv
    forb = torch.zeros(P, c.nq, nk, dtype=torch.bool)
    i = torch.arange(c.nq)
    if c.causal:
        f = c.nnull + i + (c.n_kv - c.nq) + 1
        ok = f < nk
        forb[:, i[ok], f[ok]] = True
    elif x.kmask is not None:
        for p in range(P):
            dead = (~x.kmask[p // c.h]).nonzero().flatten()
            if 0 < dead.numel() < c.n_kv:
                forb[p, i, c.nnull + dead[(i + p) % dead.numel()]] = True
    return forb & masked


def build(c, poison=float('nan')):
    """the seeded inputs of a case: images Q (P, nq_pad, 64), K (P, nk_pad, 64), Vt (P, 64, nk_pad) as f32 values with poisoned pads, the bias as the
    kernel takes it (bias_buf (h, nq, ld) with poisoned slack columns | tab, codes, off), kmask (S, n_kv) bool, slopes (h,), score_bound, and the
    planting record (targets, vis)"""
    g = _gen(c.name)
    rt = _rt(c)
    P, nk = c.S * c.h, c.nnull + c.n_kv
    nq_pad, nk_pad = pads(c.nq, c.n_kv, c.nnull)
    x = SimpleNamespace(bias=None, bias_buf=None, tab=None, codes=None, off=0, kmask=None, slopes=None, score_bound=None)
    if c.bias in ('vec', 'scalar'):
        ld = -(-c.n_kv // 4) * 4 if c.bias == 'vec' else (c.n_kv if c.n_kv % 4 else c.n_kv + 1)
        x.bias_buf = torch.full((c.h, c.nq, ld), poison, dtype=torch.float32)
        x.bias_buf[:, :, :c.n_kv] = torch.randn(c.h, c.nq, c.n_kv, generator=g) * 0.5
        x.bias = x.bias_buf[:, :, :c.n_kv]
    elif c.bias == 'table':
        code, x.off, L = table_codes(c.dims)
        x.tab = (torch.randn(c.h, L, generator=g) * 0.5).float()
        x.codes = code.to(torch.int32)
        x.bias = x.tab[:, code[:, None] - code[None, :] + x.off]
    if c.mask is not None:
        km = torch.rand(c.S, c.n_kv, generator=g) < 0.75
        km[:, -1] = True                                   # the last real key stays visible: it is the key a short loop drops
        km[:, 0] = False
        if c.mask == 'full':
            assert c.S >= 2
            km[-1] = False
        x.kmask = km
    if c.causal:
        x.slopes = (2.0 ** -(6 + torch.arange(c.h))).float()
    D = 64 - NOFF
    K = torch.zeros(P, nk, 64)
    K[:, :, :D] = rt(torch.randn(P, nk, D, generator=g) * 0.35)
    K[:, :, D:] = 0.5
    V = rt(torch.randn(P, nk, 64, generator=g))
    noise = torch.randn(P, c.nq, D, generator=g) * 0.1
    add, masked = structure(c, x)
    vis = ~masked
    targets = _assign(vis, MAX_TARGETS)
    planted = targets | _forbidden(c, x, masked)
    Kd = K[:, :, :D].double()
    U = Kd / (Kd * Kd).sum(-1, keepdim=True)               # q . k_t = 1 per unit of coefficient
    coef = torch.where(planted, G0 - add, torch.zeros((), dtype=torch.float64))
    Q = torch.zeros(P, c.nq, 64)
    Q[:, :, D:] = -GAMMA / (NOFF * 0.5)
    want = 0.9 / targets.sum(-1, keepdim=True).clamp_min(1)       # a row's targets share 0.9 of its softmax: 0.9 | 0.45 | 0.3 each
    for _ in range(16):
        Q[:, :, :D] = rt((noise.double() + coef @ U).float())
        sim = Q.double() @ K.double().transpose(1, 2) + add
        prob = torch.where(masked, torch.full_like(sim, NEG_MAX), sim).softmax(-1)
        if not (targets & (prob < MASS + 0.02)).any():
            break
        zero = torch.zeros((), dtype=torch.float64)
        coef = coef + torch.where(targets, 0.8 * (want / prob.clamp_min(1e-30)).log().clamp(-2, 2), zero)
        # a key that correlates with a row's targets rides up with them: push it back down along its own direction
        coef = coef - torch.where(vis & ~targets & (prob > 0.03), 0.8 * (prob / 0.01).log().clamp(0, 2), zero)
    x.Q = torch.full((P, nq_pad, 64), poison)
    x.Q[:, :c.nq] = Q
    x.K = torch.full((P, nk_pad, 64), poison)
    x.K[:, :nk] = K
    x.Vt = torch.full((P, 64, nk_pad), poison)
    x.Vt[:, :, :nk] = V.transpose(1, 2)
    if c.fix is not None:
        x.score_bound = float((sim.max() + 0.3 + (12 if c.fix == 'loose' else 0)))
    x.targets, x.vis = targets, vis
    return x


# ------------------------------------------------------------------------------------------------ reference

MUTANTS = ('drop_last_key', 'admit_pad_key', 'causal_diag_late', 'causal_diag_early', 'causal_no_offset', 'mask_no_null_shift', 'bias_col_null_shift',
           'bias_head0', 'alibi_skips_null', 'masked_seq_zeros', 'v_row_next', 'swap_rows_15_16', 'lse_missing_key')


def applies(mutant, c):
    """with a single key the softmax is 1 whatever the score: the mutants that only move scores need two"""
    nk = c.nnull + c.n_kv
    return {'drop_last_key': True,
            'admit_pad_key': nk < pads(c.nq, c.n_kv, c.nnull)[1],
            'causal_diag_late': c.causal and c.nq >= 2, 'causal_diag_early': c.causal and nk >= 2, 'causal_no_offset': c.causal and c.nq != c.n_kv,
            'mask_no_null_shift': c.mask is not None and c.nnull > 0,
            'bias_col_null_shift': c.bias in ('vec', 'scalar') and c.nnull > 0,
            'bias_head0': c.bias is not None and c.h > 1 and nk >= 2,
            'alibi_skips_null': c.causal and c.nnull > 0,
            'masked_seq_zeros': c.mask == 'full',
            'v_row_next': nk >= 2, 'swap_rows_15_16': c.nq >= 17, 'lse_missing_key': c.lse}[mutant]


def to_rows(c, t):
    """(S h, nq, d) -> the output layout (S nq, h d)"""
    return t.view(c.S, c.h, c.nq, -1).permute(0, 2, 1, 3).reshape(c.S * c.nq, -1)


def attend(c, x, Q, K, V, mutant=None):
    """Q (P, nq, 64), K, V (P, nk, 64) in f64 -> ref namespace: O, A (S nq, h 64), lse (P, nq), prob (P, nq, nk), sim"""
    add, masked = structure(c, x, mutant)
    sim = Q @ K.transpose(1, 2) + add
    sim = torch.where(masked, torch.full_like(sim, NEG_MAX), sim)
    if mutant == 'drop_last_key':
        sim[:, :, -1] = -math.inf
    if mutant == 'admit_pad_key':                          # a zero-filled pad key with score 0
        sim = torch.cat((sim, torch.zeros_like(sim[:, :, :1])), dim=2)
        V = torch.cat((V, torch.zeros_like(V[:, :1])), dim=1)
    if mutant == 'v_row_next':
        V = torch.roll(V, -1, dims=1)
    prob = sim.softmax(-1)
    O, A = prob @ V, prob @ V.abs()
    lse = torch.logsumexp(sim[:, :, :-1] if mutant == 'lse_missing_key' else sim, dim=-1)
    if mutant == 'swap_rows_15_16':
        O = O.clone()
        O[:, [15, 16]] = O[:, [16, 15]]
    if mutant == 'masked_seq_zeros':
        O = O.clone()
        O[-c.h:] = 0
    return SimpleNamespace(O=to_rows(c, O), A=to_rows(c, A), lse=lse, prob=prob, sim=sim, add=add)


def reference(c, x, mutant=None):
    nk = c.nnull + c.n_kv
    return attend(c, x, x.Q[:, :c.nq].double(), x.K[:, :nk].double(), x.Vt[:, :, :nk].double().transpose(1, 2), mutant)


def planted_property(c, x, ref):
    """asserts the planted-mass property (module docstring) on the f64 softmax of the unmutated reference"""
    nk = c.nnull + c.n_kv
    vis_any = x.vis.any(1)                                 # (P, nk)
    cover = ((ref.prob >= MASS) & x.vis).any(1)
    whole = c.nq >= vis_any.sum(1)
    tail = torch.arange(nk) >= 64 * ((nk - 1) // 64)
    need = vis_any & (whole[:, None] | tail[None, :])
    miss = (need & ~cover).nonzero()
    assert miss.numel() == 0, f'{c.name}: (pair, key) without a query row that gives it {MASS} of its softmax: {miss[:8].tolist()}'
    union = vis_any.any(0) & ~cover.any(0)
    assert not union.any(), f'{c.name}: keys planted in no pair: {union.nonzero().flatten()[:8].tolist()}'
    assert vis_any.any(), f'{c.name}: no visible key'


# ------------------------------------------------------------------------------------------------ bound

def terms(c, x, ref, Q, K, *, small=False):
    """the first-order terms of the module docstring, each broadcastable to (S nq, h 64) in units of A; `lse` is the absolute lse bound (P, nq)"""
    nk = c.nnull + c.n_kv
    ntiles = -(-nk // 32)
    fixed = not small and c.fix is not None                 # every case with a score bound has no mask / causal / matrix bias: the fixed-offset form
    t = {}
    if small or c.dtype == F32:
        t['p_round'], t['norm'], split = 0.0, 0.0, 0.0
    elif c.dtype == BF16:
        t['p_round'], t['norm'], split = U_BF16, (U_BF16 if fixed else 0.0), 0.0
    else:
        t['p_round'], t['norm'], split = 3 * U_SPLIT, (U_SPLIT if fixed else 0.0), 3 * U_SPLIT
    mag = (Q.abs() @ K.abs().transpose(1, 2) + ref.add.abs()).amax(-1)                      # (P, nq)
    ulps = 64 + 3 + (SMALL_NORM_ULPS if small else 0)
    score = (ulps * U_F32 + split) * mag
    t['score'] = 2 * to_rows(c, score[:, :, None].expand(-1, -1, 64).contiguous())
    if fixed:
        xr = math.log(2) * (math.ceil(x.score_bound * math.log2(math.e)) + ref.sim[ref.sim > NEG_MAX].abs().max().item() * math.log2(math.e))
        xr *= 2 if c.bias == 'table' else 1
    else:
        xr = 24 * math.log(2)
    t['exp'] = 2 * (3 + xr) * U_F32
    t['accumulate'] = (nk + 3 * ntiles + 3) * U_F32
    t['lse'] = 2 * (score + t['exp'] / 2 + t['accumulate'] + t['norm'] + 2.0 ** -21 + 2.0 ** -23 * ref.lse.abs())
    return t


def bound(c, x, ref, Q=None, K=None, *, out_bf16=None, small=False):
    """(bound (S nq, h 64), lse bound (P, nq), terms)"""
    nk = c.nnull + c.n_kv
    if Q is None:
        Q, K = x.Q[:, :c.nq].double(), x.K[:, :nk].double()
    t = terms(c, x, ref, Q, K, small=small)
    first = t['p_round'] + t['norm'] + t['score'] + t['exp'] + t['accumulate']
    u_out = U_BF16 if (out_bf16 if out_bf16 is not None else not c.out_f32) else 0.0
    return 2 * first * ref.A + u_out * binade_top(ref.O), t['lse'], t


def binade_top(t):
    """the power of two at or above |t| (0 for 0): half an ulp of an 8-bit significand is 2^-9 of THIS, up to 2^-8 of |t| itself"""
    return torch.exp2(torch.ceil(torch.log2(t.abs())))


def check(what, out, ref_O, bnd, width):
    """out: the WHOLE output buffer (rows, ldo) with ldo > width, pre-filled with NaN before the launch.  Every element of the first `width` columns
    within its bound and finite, every slack column still NaN.  Returns the largest error / bound."""
    out = out.detach().double().cpu()
    assert out.shape[0] == ref_O.shape[0] and out.shape[1] > width == ref_O.shape[1], f'{what}: buffer {tuple(out.shape)} for an output {tuple(ref_O.shape)}'
    slack = out[:, width:]
    assert torch.isnan(slack).all(), f'{what}: {int((~torch.isnan(slack)).sum())} writes into the slack columns of the output rows'
    o = out[:, :width]
    bad = ~torch.isfinite(o)
    assert not bad.any(), f'{what}: {int(bad.sum())} non-finite / unwritten output elements, first at {bad.nonzero()[0].tolist()}'
    ratio = (o - ref_O).abs() / bnd
    worst = ratio.max().item()
    if worst > 1:
        r, col = divmod(int(ratio.argmax()), width)
        raise AssertionError(f'{what}: element ({r}, {col}) is {o[r, col]:.6g}, reference {ref_O[r, col]:.6g}: error {abs(o[r, col] - ref_O[r, col]):.3e} = '
                             f'{worst:.2f} x bound {bnd[r, col]:.3e}; {int((ratio > 1).sum())} elements beyond their bound')
    return worst


def check_lse(what, lse, ref_lse, bnd):
    lse = lse.detach().double().cpu().view(ref_lse.shape)
    assert torch.isfinite(lse).all(), f'{what}: non-finite / unwritten lse'
    ratio = (lse - ref_lse).abs() / bnd
    worst = ratio.max().item()
    assert worst <= 1, f'{what}: lse error {worst:.2f} x bound at {divmod(int(ratio.argmax()), ref_lse.shape[1])}'
    return worst


# ------------------------------------------------------------------------------------------------ pk_attn_small

SMALL_NORM_ULPS = 2 * (32 + 4)       # per operand: a 64-term f32 sum of squares under a square root (32 ulps), sqrt, divide, two products
SMALL_N = (1, 9, 32, 33, 63, 64)
SCALE = 8.0


def small_cases():
    out = []
    for n in SMALL_N:
        G = 64 // n
        S = G + 1 if G > 1 else 3                          # not a multiple of the sequences per wave (where a wave holds more than one)
        for k, (tag, kw) in enumerate((('plain', {}), ('mask', dict(mask='full')), ('causal', dict(causal=True)), ('bias', dict(bias='vec')),
                                       ('all', dict(mask='mask', causal=True, bias='scalar')))):
            if n == 1 and tag in ('mask', 'all'):
                continue                                   # one key: a masked sequence is all there is to mask
            out.append(_case(f'small_n{n}_{tag}', F32, S, 2, n, n, 'small', out_f32=(k + n) % 2 == 0, **kw))
    return out


def build_small(c):
    """raw projection outputs q (S n, h 64), kv (S n, 2 h 64) f32, q_scale / k_scale (64,), and the structure fields of build()"""
    g = _gen(c.name)
    P, n = c.S * c.h, c.nq
    x = SimpleNamespace(bias=None, bias_buf=None, kmask=None, slopes=None)
    if c.bias is not None:
        ld = -(-n // 4) * 4 if c.bias == 'vec' else (n if n % 4 else n + 1)
        x.bias_buf = torch.full((c.h, n, ld), float('nan'), dtype=torch.float32)
        x.bias_buf[:, :, :n] = torch.randn(c.h, n, n, generator=g) * 0.3
        x.bias = x.bias_buf[:, :, :n]
    if c.mask is not None:
        km = torch.rand(c.S, n, generator=g) < 0.75
        km[:, -1] = True
        km[:, 0] = n == 1
        if c.mask == 'full':
            km[-1] = False
        x.kmask = km
    if c.causal:
        x.slopes = (2.0 ** -(6 + torch.arange(c.h))).float()
    x.q_scale = (1 + 0.1 * torch.randn(64, generator=g)).float()
    x.k_scale = (1 + 0.1 * torch.randn(64, generator=g)).float()
    k = torch.randn(P, n, 64, generator=g) * (0.5 + torch.rand(P, n, 1, generator=g))      # rows of different lengths: the l2norm matters
    v = torch.randn(P, n, 64, generator=g)
    noise = torch.randn(P, n, 64, generator=g)
    _, masked = structure(c, x)
    x.vis = ~masked
    x.targets = _assign(x.vis, 2)
    planted = (x.targets | _forbidden(c, x, masked)).double()
    khat = (k / k.norm(dim=-1, keepdim=True)).double()
    sigma = torch.full((P, n, 1), 0.08, dtype=torch.float64)
    for _ in range(6):
        q = ((planted @ khat + sigma * noise.double()) * (0.5 + torch.arange(n)[None, :, None] % 3)).float()
        x.q = q.view(c.S, c.h, n, 64).permute(0, 2, 1, 3).reshape(c.S * n, c.h * 64).contiguous()
        kk = k.view(c.S, c.h, n, 64).permute(0, 2, 1, 3).reshape(c.S * n, c.h * 64)
        vv = v.view(c.S, c.h, n, 64).permute(0, 2, 1, 3).reshape(c.S * n, c.h * 64)
        x.kv = torch.cat((kk, vv), dim=1).contiguous()
        ref = reference_small(c, x)
        weak = (x.targets & (ref.prob < MASS + 0.05)).any(-1, keepdim=True)
        if not weak.any():
            break
        sigma = torch.where(weak, sigma / 2, sigma)
    return x


def small_images(c, x):
    """f64 l2norm(q) q_scale scale, l2norm(k) k_scale, v as (P, n, 64)"""
    n = c.nq
    heads = lambda t: t.double().view(c.S, n, c.h, 64).permute(0, 2, 1, 3).reshape(c.S * c.h, n, 64)
    q, k, v = heads(x.q), heads(x.kv[:, :c.h * 64]), heads(x.kv[:, c.h * 64:])
    qn = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12) * x.q_scale.double() * SCALE
    kn = k / k.norm(dim=-1, keepdim=True).clamp_min(1e-12) * x.k_scale.double()
    return qn, kn, v


def reference_small(c, x, mutant=None):
    qn, kn, v = small_images(c, x)
    ref = attend(c, x, qn, kn, v, mutant)
    ref.Q, ref.K = qn, kn
    return ref


# ------------------------------------------------------------------------------------------------ pk_attn_prep

PREP_NORM_ULPS = 32 + 4              # as SMALL_NORM_ULPS, one operand
PREP_CASES = [dict(name=f'prep_{DTYPE_NAME[dt]}_{tag}', dtype=dt, S=2, h=3, nq=nq, n_kv=n_kv, nnull=nnull, kv=kv, scales=scales)
              for dt in (F32, BF16, BF16X3)
              for tag, nq, n_kv, nnull, kv, scales in (('null0', 37, 70, 0, True, True), ('null2', 130, 61, 2, True, True), ('query_only', 65, 65, 0, False, True),
                                                       ('no_scale', 20, 33, 2, True, False))]


def build_prep(p):
    g = _gen(p['name'])
    S, h, nq, n_kv, nnull = p['S'], p['h'], p['nq'], p['n_kv'], p['nnull']
    x = SimpleNamespace()
    x.q = torch.randn(S * nq, h * 64, generator=g) * (0.2 + 2 * torch.rand(S * nq, 1, generator=g))
    x.kv = torch.randn(S * n_kv, 2 * h * 64, generator=g) * (0.2 + 2 * torch.rand(S * n_kv, 1, generator=g)) if p['kv'] else None
    x.null_kv = torch.randn(h, 2 * nnull, 64, generator=g) if nnull else None
    x.q_scale = (1 + 0.1 * torch.randn(64, generator=g)).float() if p['scales'] else None
    x.k_scale = (1 + 0.1 * torch.randn(64, generator=g)).float() if p['scales'] else None
    return x


def reference_prep(p, x):
    """f64 images (Q (P, nq, 64), K (P, nk, 64), V (P, nk, 64)) of attention.py:148-157: null keys prepended, l2norm after the concat, q * scale"""
    S, h, nq, n_kv, nnull = p['S'], p['h'], p['nq'], p['n_kv'], p['nnull']
    heads = lambda t, n: t.double().view(S, n, h, 64).permute(0, 2, 1, 3).reshape(S * h, n, 64)
    q = heads(x.q, nq)
    Q = q / q.norm(dim=-1, keepdim=True).clamp_min(1e-12) * x.q_scale.double() * SCALE if p['scales'] else q * SCALE
    if not p['kv']:
        return Q, None, None
    k, v = heads(x.kv[:, :h * 64], n_kv), heads(x.kv[:, h * 64:], n_kv)
    if nnull:
        nk_, nv_ = x.null_kv.double()[:, 0::2], x.null_kv.double()[:, 1::2]          # (h, nnull, 64) each
        k = torch.cat((nk_.repeat(S, 1, 1), k), dim=1)
        v = torch.cat((nv_.repeat(S, 1, 1), v), dim=1)
    K = k / k.norm(dim=-1, keepdim=True).clamp_min(1e-12) * x.k_scale.double() if p['scales'] else k
    return Q, K, v


def prep_bound(dtype, ref, normed):
    """one output ulp -- half an ulp of the image type at the upper end of ref's binade: bf16 2^-9, f32 2^-24, split-bf16 2^-18 (hi + lo: 2^-9 of 2^-9) -- plus
    the f32 error of the norm and the products on |ref|"""
    u = {F32: U_F32, BF16: U_BF16, BF16X3: 2.0 ** -18}[dtype]
    return u * binade_top(ref) + (PREP_NORM_ULPS if normed else 1) * U_F32 * ref.abs() + 1e-45


def unsplit(img, k):
    """inverse of _lib.split_planes: (N, k) raw-bit f32-typed image -> hi + lo as f64"""
    b = img.contiguous().view(torch.bfloat16).view(img.shape[0], k // 32, 64).double()
    return (b[:, :, :32] + b[:, :, 32:]).reshape(img.shape[0], k)
