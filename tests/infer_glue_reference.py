"""CPU float64 restatements of the small inference kernels (csrc/norm.hip, elementwise.hip, patch.hip and pk_cfg_mix / pk_topk_mask of sampler.hip), in plain
torch, with the seeded case builders and the checkers that tests/test_infer_glue_gpu.py runs on the kernels' outputs.  tests/test_infer_glue_host.py holds every
restatement to the project's oracle or a torch function, feeds every checker an f32 evaluation in two summation orders (the bound is not tighter than f32
arithmetic allows) and a list of named wrong kernels (a checker that cannot fail is itself a failure).

The rule of tests/train_glue_reference.py holds: every bound is derived from the operation, never from what a kernel returned, and every element is held to
its own bound.  Selects, copies and single rounded operations are bit for bit; an expression of several roundings gets one U per rounding on the magnitude of
the intermediate (the library is built with -ffp-contract=fast: a multiply-add may or may not be fused); a reduction gets the any-order bound sum_bound pushed
through the rest of the expression to first order; a bf16 output is the round-to-nearest-even of the f32 output of the same operation, bit for bit.  Every
output buffer is pre-filled with NaN (or a sentinel) and is longer / wider than the output, so unwritten elements and writes into gutters both show."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from tests.train_glue_reference import U, gen, sum_bound, assert_within, assert_same_bits, assert_untouched, assert_written, patchify

NAN = float('nan')
LN_EPS = 1e-5
RMS_EPS = 1e-6
BF16, F32 = torch.bfloat16, torch.float32
GUARD = 2                      # extra rows behind every output
SENTINEL = -7                  # pre-fill of the integer outputs


# ------------------------------------------------------------------------------------------------ shared pieces

def perm_rows(M, pb, pc):
    """output row of input row r = (a, b, c), extents (*, pb, pc): (a, c, b)"""
    r = torch.arange(M)
    if pb <= 0:
        return r
    c, b, a = r % pc, (r // pc) % pb, r // (pc * pb)
    return (a * pc + c) * pb + b


def grp_rows(M, grp, gstride, goff):
    r = torch.arange(M)
    return (r // grp) * gstride + goff + r % grp


def widen(t, pad, fill=NAN):
    """t in the first columns of a buffer `pad` columns wider"""
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype)
    buf[:, :t.shape[1]] = t
    return buf


def nan_buffer(rows, ld, dtype=F32, device='cpu'):
    return torch.full((rows, ld), NAN, dtype=dtype, device=device)


def place(buf, orows, y):
    """what a correct kernel leaves: y's rows at `orows`, first columns"""
    buf[orows, :y.shape[1]] = y.to(buf.dtype)
    return buf


def region(buf, orows, D, what):
    """rows `orows` x the first D columns of buf, after asserting that nothing else of buf was written"""
    b = buf.detach().cpu()
    rest = b.float().clone()
    rest[orows, :D] = NAN
    assert_untouched(rest, f'{what}: rows / columns outside the output')
    got = b[orows, :D].clone()
    assert_written(got, what)
    return got


def rne(t):
    return t.to(BF16)


def truncated_bf16(t):
    """the wrong rounding: the low 16 bits dropped"""
    return (t.contiguous().view(torch.int32) & -65536).view(F32).to(BF16)


def sum32(t, order=0):
    """an f32 sum over the last axis in one of two association orders"""
    if order == 0:
        return t.sum(-1)
    return t[..., 1::2].sum(-1) + t[..., 0::2].sum(-1)


def dot32(y, w, order=0):
    """(M, D) x (cd, D) -> (M, cd) in f32, in one of two association orders"""
    if order == 0:
        return y @ w.t()
    return y[:, 1::2] @ w[:, 1::2].t() + y[:, 0::2] @ w[:, 0::2].t()


def check_bf16_of(got, f32_same_launch, what):
    assert got.dtype == BF16
    assert_same_bits(got, rne(f32_same_launch), f'{what}: bf16 against the round-to-nearest-even of the f32 output')


def max_ratio(err, bound):
    return float(torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max()) if err.numel() else 0.


# ------------------------------------------------------------------------------------------------ LayerNorm (pk_layernorm, pk_layernorm_lfq, pk_patchify_ln)

def ln_ref(x, gamma, beta, eps=LN_EPS):
    """float64 y = (x - mean) rstd gamma + beta over the last axis (biased variance, eps inside the root) and its bound.  em bounds the mean (a D-term sum,
    the division), dv the variance (the D-term sum of squares and the rounding of every d = x - mean; a mean off by e adds exactly e^2, the cross term
    2 e sum(d) being zero: tighter than the 2 em mean|d| of a term-by-term estimate), er the relative error of rstd (half of dv's, the add of
    eps, root and reciprocal); y = d r g + beta then carries d's rounding and the mean's error, r's error on |d| and the roundings of the two products and
    the add"""
    x, g = x.double(), gamma.double()
    b = beta.double() if beta is not None else torch.zeros_like(g)
    D = x.shape[-1]
    mean = x.mean(-1, keepdim=True)
    d = x - mean
    v = (d * d).mean(-1, keepdim=True)
    r = 1.0 / torch.sqrt(v + eps)
    y = d * r * g + b
    em = (D + 2) * U * x.abs().mean(-1, keepdim=True)
    dv = (D + 6) * U * v + em * em
    er = dv / (2 * (v + eps)) + 3 * U
    bound = g.abs() * r * (U * d.abs() + em) + g.abs() * d.abs() * r * (er + 3 * U) + U * (y.abs() + b.abs())
    return y, bound


def ln_f32(x, gamma, beta, eps=LN_EPS, order=0, unbiased=False, eps_outside=False, width=None, no_beta=False, gamma_shift=False, center=True):
    """the formula in f32, every operation rounded once; the keywords are the named wrong kernels"""
    x = x.float()
    D = x.shape[-1]
    n = torch.tensor(float(width if width is not None else D))
    mean = sum32(x, order) / n if center else torch.zeros(x.shape[:-1])
    d = x - mean[..., None]
    q = sum32(d * d, order)
    v = q / (n - 1 if unbiased else n)
    rstd = 1.0 / (torch.sqrt(v) + eps) if eps_outside else 1.0 / torch.sqrt(v + eps)
    g = torch.roll(gamma, 4) if gamma_shift else gamma
    y = d * rstd[..., None] * g
    return y if (beta is None or no_beta) else y + beta


def small_variance_row(D, g):
    """variance 4 eps: the row that tells eps inside the root from eps outside it, and still 1 / D from 1 / (D - 1) at D = 2048"""
    return torch.randn(D, generator=g) * (4 * LN_EPS) ** 0.5


def ln_rows(M, D, *key):
    """(M, D) f32: rows 0 ... 3 have a variance of about eps, are constant, are zero, have mean 1e3 with unit deviation; the rest are random with their own
    mean and scale.  Row 0 is the one every shape has: it is sensitive to each of the named wrong kernels"""
    g = gen(20, M, D, *key)
    x = torch.randn(M, D, generator=g) * (0.5 + torch.rand(M, 1, generator=g)) + torch.randn(M, 1, generator=g)
    for i in range(min(M, 4)):
        if i == 0:
            x[i] = small_variance_row(D, g)
        elif i == 1:
            x[i] = 3.7
        elif i == 2:
            x[i] = 0.
        elif i == 3:
            x[i] = 1e3 + torch.randn(D, generator=g)
    return x


LN_D = [4, 252, 256, 260, 512, 516, 2048]
LN_M = [1, 3, 4, 5, 300]
# (outputs, out_kind, beta, wide leading dimensions, row map): every value of every option, on every (M, D)
LN_VARIANTS = [('out', 0, True, False, 'none'), ('out2', 0, False, True, 'grp'), ('out+out2', 1, True, True, 'perm'), ('out+out2+raw', 1, False, False, 'grp_off'),
               ('out+out2+raw', 0, True, True, 'grp'), ('out', 1, True, True, 'none'), ('out+raw', 1, False, True, 'perm'), ('out+out2', 0, False, False, 'grp_off')]


def ln_map(M, kind):
    """(remap (grp, gstride, goff), perm (pb, pc), output rows, rows of the output buffer)"""
    if kind in ('grp', 'grp_off'):
        grp = 7 if M > 7 else (2 if M % 2 else 3)
        assert M % grp != 0                                       # the last group is partial
        gstride, goff = grp + 3, (5 if kind == 'grp_off' else 0)
        orows = grp_rows(M, grp, gstride, goff)
        return (grp, gstride, goff), (0, 0), orows, int(orows.max()) + 1 + GUARD
    if kind == 'perm' and M % 100 == 0:
        pb, pc = 4, 25                                            # M / 100 outer blocks
        return (0, 0, 0), (pb, pc), perm_rows(M, pb, pc), M + GUARD
    if kind == 'perm' and M == 4:
        return (0, 0, 0), (2, 2), perm_rows(M, 2, 2), M + GUARD
    return (0, 0, 0), (0, 0), torch.arange(M), M + GUARD


def ln_case(M, D, variant, seed=0):
    outs, out_kind, has_beta, wide, mapk = variant
    g = gen(21, M, D, seed)
    x = ln_rows(M, D, seed)
    gamma = 1 + 0.3 * torch.randn(D, generator=g)
    beta = 0.3 * torch.randn(D, generator=g) if has_beta else None
    remap, perm, orows, nrows = ln_map(M, mapk)
    pad = dict(x=4, out=8, out2=12, raw=16) if wide else dict(x=0, out=0, out2=0, raw=0)
    return dict(M=M, D=D, outs=outs.split('+'), out_kind=out_kind, x=widen(x, pad['x']), gamma=gamma, beta=beta, remap=remap, perm=perm, orows=orows,
                nrows=nrows, ld={k: D + p for k, p in pad.items()}, mapk=mapk)


def ln_buffers(c, device='cpu'):
    t = BF16 if c['out_kind'] else F32
    return dict(out=nan_buffer(c['nrows'], c['ld']['out'], t, device) if 'out' in c['outs'] else None,
                out2=nan_buffer(c['nrows'], c['ld']['out2'], F32, device) if 'out2' in c['outs'] else None,
                raw=nan_buffer(c['nrows'], c['ld']['raw'], t, device) if 'raw' in c['outs'] else None)


def ln_check(c, out, out2, raw, f32_out=None):
    """the buffers of ln_buffers after the launch.  f32_out: the `out` region of the same case launched with out_kind 0, where a bf16 `out` has no out2 beside it"""
    D, orows = c['D'], c['orows']
    ref, bound = ln_ref(c['x'][:, :D], c['gamma'], c['beta'])
    ratio, y32 = 0., None
    if out2 is not None:
        y32 = region(out2, orows, D, 'layernorm out2')
        ratio = assert_within(y32, ref, bound, 'layernorm out2')
    if out is not None:
        got = region(out, orows, D, 'layernorm out')
        if got.dtype == F32:
            ratio = max(ratio, assert_within(got, ref, bound, 'layernorm out'))
            if y32 is not None:
                assert_same_bits(got, y32, 'layernorm out against out2 of the same launch')
        else:
            assert y32 is not None or f32_out is not None, 'a bf16 out needs the f32 output it rounds'
            check_bf16_of(got, y32 if y32 is not None else f32_out, 'layernorm out')
    if raw is not None:
        assert_same_bits(region(raw, orows, D, 'layernorm raw'), c['x'][:, :D].to(raw.dtype), 'layernorm raw (a copy of x)')
    return ratio


def ln_fake(c, y, orows=None, raw_from=None):
    """what a kernel computing y (M, D) f32 would leave in ln_buffers"""
    b = ln_buffers(c)
    orows = c['orows'] if orows is None else orows
    for k in ('out', 'out2'):
        if b[k] is not None:
            place(b[k], orows, y)
    if b['raw'] is not None:
        place(b['raw'], orows, c['x'][:, :c['D']] if raw_from is None else raw_from)
    return b


# ------------------------------------------------------------------------------------------------ LFQ ids (pk_lfq_encode, pk_layernorm_lfq)

def lfq_bits(ids, cd):
    """(M, cd) 0 / 1, MSB first"""
    sh = torch.arange(cd - 1, -1, -1)
    return (ids.long()[:, None] >> sh) & 1


def lfq_ids_of(bits):
    cd = bits.shape[1]
    return (bits.long() << torch.arange(cd - 1, -1, -1)).sum(1)


def lfq_band(P, pbound):
    """the bits whose float64 projection lies within its own bound of zero (strictly: an exact zero with a zero bound is NOT in the band)"""
    return P.abs() < pbound


def lfq_weights(cd, D, g, planted):
    wp = torch.randn(cd, D, generator=g) / D ** 0.5
    bp = 0.5 * torch.randn(cd, generator=g)
    if planted:                                                   # with an all-zero row the projection IS bp: 0.0, a small positive, a small negative
        special = torch.tensor([0., 1e-30, -1e-30])
        bp[:min(cd, 3)] = special[:min(cd, 3)]
    return wp, bp


def lfq_check_ids(ids_buf, orows, P, pbound, cd, proj_buf, what):
    """ids_buf (>= M + GUARD,) int64 pre-filled with SENTINEL; proj_buf (M + GUARD, cd) NaN-filled or None.  A bit may differ from the float64 sign only
    inside the band; with proj given the ids are also the signs of the kernel's own projections, bit for bit.  Returns the largest err / bound of proj"""
    M = P.shape[0]
    ib = ids_buf.detach().cpu()
    rest = ib.clone()
    rest[orows] = SENTINEL
    assert (rest == SENTINEL).all(), f'{what} ids: written outside the output rows'
    ids = ib[orows]
    bad_row = (ids < 0) | (ids >= 2 ** cd)
    assert not bad_row.any(), f'{what} ids: {int(bad_row.sum())} rows not written or out of range, first row {int(bad_row.nonzero()[0])}'
    bits = lfq_bits(ids, cd)
    wrong = (bits != (P > 0).long()) & ~lfq_band(P, pbound)
    if wrong.any():
        m, k = (int(v) for v in wrong.nonzero()[0])
        raise AssertionError(f'{what} ids: {int(wrong.sum())} bits differ from the float64 sign outside the band, first row {m} bit {k}: projection {P[m, k].item():.3e}, '
                             f'bound {pbound[m, k].item():.3e}')
    ratio = 0.
    if proj_buf is not None:
        pr = region(proj_buf.reshape(-1, cd), orows, cd, f'{what} proj')
        ratio = assert_within(pr, P, pbound, f'{what} proj')
        assert torch.equal(bits, (pr > 0).long()), f'{what}: ids are not the signs of the projections written beside them'
    return ratio


LFQ_ENC_CD = [4, 6, 8, 10, 12, 13, 14, 16, 18]
LFQ_ENC_D = [4, 252, 256, 260, 1024]
LFQ_ENC_M = [1, 5, 777]


def lfq_enc_case(M, D, cd, wide=True, seed=0):
    g = gen(22, M, D, cd, seed)
    x = torch.randn(M, D, generator=g)
    planted = M // 2 if M >= 2 else None
    if planted is not None:
        x[planted] = 0.
    wp, bp = lfq_weights(cd, D, g, True)
    return dict(M=M, D=D, cd=cd, x=widen(x, 4 if wide else 0), wp=wp, bp=bp, planted=planted, orows=torch.arange(M))


def lfq_enc_ref(c):
    x, wp, bp = c['x'][:, :c['D']].double(), c['wp'].double(), c['bp'].double()
    return x @ wp.t() + bp, sum_bound(x.abs() @ wp.abs().t() + bp.abs(), c['D'])


def lfq_enc_buffers(c, device='cpu'):
    return torch.full((c['M'] + GUARD,), SENTINEL, dtype=torch.int64, device=device), nan_buffer(c['M'] + GUARD, c['cd'], F32, device)


def lfq_planted_check(c, ids_buf, what):
    """the planted all-zero row: its projection is bp exactly, so its id is bits(bp > 0) with no band at all (v > 0 at v == 0 is 0)"""
    if c['planted'] is not None:
        got = int(ids_buf.detach().cpu()[c['orows'][c['planted']]])
        want = int(lfq_ids_of((c['bp'] > 0)[None])[0])
        assert got == want, f'{what}: the planted zero row gives id {got}, its bias alone gives {want}'


def lfq_enc_check(c, ids_buf, proj_buf):
    P, pb = lfq_enc_ref(c)
    ratio = lfq_check_ids(ids_buf, c['orows'], P, pb, c['cd'], proj_buf, 'lfq_encode')
    lfq_planted_check(c, ids_buf, 'lfq_encode')
    return ratio


def lfq_enc_f32(c, order=0):
    x = c['x'][:, :c['D']]
    return dot32(x, c['wp'], order) + c['bp']


def lfq_fake(c, P32, orows=None, reverse_bits=False, with_proj=True):
    """what a kernel whose projections are P32 would leave"""
    orows = c['orows'] if orows is None else orows
    ids_buf, proj_buf = lfq_enc_buffers(c)
    bits = (P32 > 0)
    ids_buf[orows] = lfq_ids_of(bits.flip(1) if reverse_bits else bits)
    place(proj_buf, orows, P32)
    return ids_buf, (proj_buf if with_proj else None)


# (M, D, cd, beta, tokens, proj, (pb, pc) permutation, the kernel the case exists for): <2,1> and <8,1> at every D with M in {1, 5, 1152}, the two-rows-per-wave
# <2,2> at M = 32768 / 32769 (the odd M's last row is a clamped tail), cd in {1, 2, 5, 13, 16}
LNLFQ_CASES = [
    (1, 64, 16, True, False, True, False, '<2,1>'), (5, 64, 13, False, True, False, False, '<2,1>'), (1152, 64, 5, True, True, True, True, '<2,1>'),
    (1, 512, 16, False, True, True, False, '<2,1>'), (5, 512, 13, True, True, False, False, '<2,1>'), (1152, 512, 5, False, False, True, False, '<2,1>'),
    (1, 516, 16, True, True, True, False, '<8,1>'), (5, 516, 13, False, False, False, False, '<8,1>'), (1152, 516, 5, True, True, True, True, '<8,1>'),
    (1, 2048, 16, False, False, True, False, '<8,1>'), (5, 2048, 13, True, True, False, False, '<8,1>'), (1152, 2048, 5, False, True, True, False, '<8,1>'),
    (32768, 64, 16, True, True, True, True, '<2,2>'), (32769, 64, 13, False, True, True, False, '<2,2>'), (32768, 512, 2, False, False, True, False, '<2,2>'),
    (32769, 512, 1, True, True, False, False, '<2,2>'), (5, 64, 1, False, True, True, False, '<2,1>'), (5, 516, 2, False, True, True, False, '<8,1>'),
]


def lnlfq_branch(M, D):
    """the kernel pk_layernorm_lfq launches, from the host-visible condition"""
    return '<2,2>' if (D <= 512 and M >= 32768) else ('<2,1>' if D <= 512 else '<8,1>')


def lnlfq_case(M, D, cd, has_beta, tokens, proj, perm, branch=None, seed=0):
    g = gen(23, M, D, cd, seed)
    x = torch.randn(M, D, generator=g) * (0.5 + torch.rand(M, 1, generator=g)) + torch.randn(M, 1, generator=g)
    x[0] = small_variance_row(D, g)
    gamma = 1 + 0.3 * torch.randn(D, generator=g)
    beta = 0.3 * torch.randn(D, generator=g) if has_beta else None
    planted = M // 2 if (not has_beta and M >= 2) else None      # LN of a zero row is beta: exactly zero only without beta
    if planted is not None:
        x[planted] = 0.
    wp, bp = lfq_weights(cd, D, g, not has_beta)
    pb, pc = ((8, M // 32) if M % 32 == 0 else (0, 0)) if perm else (0, 0)
    return dict(M=M, D=D, cd=cd, x=widen(x, 4), gamma=gamma, beta=beta, wp=wp, bp=bp, planted=planted, perm=(pb, pc), orows=perm_rows(M, pb, pc),
                tokens=tokens, proj=proj, ldt=D + 8)


def lnlfq_ref(c):
    """(y, ybound, P, pbound): the projection carries y's bound through |wp| and the D-term dot product's own"""
    y, yb = ln_ref(c['x'][:, :c['D']], c['gamma'], c['beta'])
    wp, bp = c['wp'].double(), c['bp'].double()
    return y, yb, y @ wp.t() + bp, yb @ wp.abs().t() + sum_bound(y.abs() @ wp.abs().t() + bp.abs(), c['D'])


def lnlfq_buffers(c, device='cpu'):
    ids, proj = lfq_enc_buffers(c, device)
    return ids, (nan_buffer(c['M'] + GUARD, c['ldt'], F32, device) if c['tokens'] else None), (proj if c['proj'] else None)


def lnlfq_check(c, ids_buf, tok_buf, proj_buf):
    y, yb, P, pb = lnlfq_ref(c)
    out = dict(tokens=0.)
    if tok_buf is not None:
        out['tokens'] = assert_within(region(tok_buf, c['orows'], c['D'], 'layernorm_lfq tokens'), y, yb, 'layernorm_lfq tokens')
    out['proj'] = lfq_check_ids(ids_buf, c['orows'], P, pb, c['cd'], proj_buf, 'layernorm_lfq')
    lfq_planted_check(c, ids_buf, 'layernorm_lfq')
    return out


def lnlfq_f32(c, order=0, **wrong):
    y = ln_f32(c['x'][:, :c['D']], c['gamma'], c['beta'], order=order, **wrong)
    return y, dot32(y, c['wp'], order) + c['bp']


def lnlfq_fake(c, y32, P32, orows=None, reverse_bits=False, drop_last=False):
    orows = c['orows'] if orows is None else orows
    ids_buf, tok_buf, proj_buf = lnlfq_buffers(c)
    bits = P32 > 0
    ids_buf[orows] = lfq_ids_of(bits.flip(1) if reverse_bits else bits)
    if tok_buf is not None:
        place(tok_buf, orows, y32)
    if proj_buf is not None:
        place(proj_buf, orows, P32)
    if drop_last:                                                 # the two-row kernel dropping the odd last row
        ids_buf[orows[-1]] = SENTINEL
        for b in (tok_buf, proj_buf):
            if b is not None:
                b[orows[-1]] = NAN
    return ids_buf, tok_buf, proj_buf


# ------------------------------------------------------------------------------------------------ pk_lfq_decode

def decode_fast(D, cd, out_ptr, bo_ptr, wo_ptr):
    """the five-part predicate of pk_lfq_decode's register-resident kernel, restated from the host code"""
    dv = D >> 2
    return D % 4 == 0 and dv <= 256 and (256 % dv == 0 or dv == 256) and cd in (8, 16) and out_ptr % 16 == 0 and bo_ptr % 16 == 0 and wo_ptr % 16 == 0


# (M, D, cd, prime (nb, n_prime, n) or None, perm (pb, pc), the operand offset by 4 bytes, the kernel the case exists for)
DECODE_CASES = [(5, 4, 8, None, (0, 0), None, 'fast'), (300, 4, 16, None, (3, 4), None, 'fast'), (37, 128, 16, None, (0, 0), None, 'fast'),
                (36, 128, 8, (3, 5, 7), (4, 3), None, 'fast'), (1, 512, 16, None, (0, 0), None, 'fast'), (1025, 512, 16, (25, 16, 25), (5, 41), None, 'fast'),
                (1025, 512, 8, None, (0, 0), None, 'fast'), (7, 1024, 8, None, (0, 0), None, 'fast'), (12, 1024, 16, (2, 2, 4), (2, 3), None, 'fast'),
                (7, 96, 16, None, (0, 0), None, 'generic'), (12, 96, 8, (2, 2, 4), (2, 3), None, 'generic'), (5, 1028, 16, None, (0, 0), None, 'generic'),
                (9, 128, 13, None, (3, 3), None, 'generic'), (11, 128, 62, None, (0, 0), None, 'generic'),
                (36, 128, 16, (3, 5, 7), (4, 3), 'bo', 'generic'), (36, 128, 16, (3, 5, 7), (4, 3), 'wo', 'generic'), (36, 128, 16, (3, 5, 7), (4, 3), 'out', 'generic'),
                (36, 128, 16, (3, 5, 7), (4, 3), None, 'fast')]


def decode_case(M, D, cd, prime, perm, misalign=None, branch=None, seed=0):
    g = gen(24, M, D, cd, seed)
    flat = torch.randint(0, 2 ** cd, (M,), generator=g, dtype=torch.int64)
    flat[0], flat[-1] = 0, 2 ** cd - 1                            # every bit off, every bit on (cd = 62: bit 61 is used)
    if M > 2:
        flat[1] = 2 ** (cd - 1)
    c = dict(M=M, D=D, cd=cd, perm=perm, orows=perm_rows(M, *perm), flat=flat, wo=torch.randn(D, cd, generator=g), bo=torch.randn(D, generator=g), misalign=misalign,
             ids=flat, ids_prime=None)
    if prime:
        nb, n_prime, n = prime
        assert nb * (n_prime + n) == M
        both = flat.reshape(nb, n_prime + n)
        c['ids_prime'], c['ids'] = both[:, :n_prime].contiguous(), both[:, n_prime:].contiguous()
    return c


def decode_ref(c, flip_bit=None):
    """f32, bo then +- wo[:, k] in ascending k: both kernels' order, and a multiply by +-1 is exact whether fused or not"""
    sgn = lfq_bits(c['flat'], c['cd']).float() * 2 - 1
    if flip_bit is not None:
        sgn[:, flip_bit] *= -1
    acc = c['bo'][None].repeat(c['M'], 1)
    for k in range(c['cd']):
        acc = acc + sgn[:, k, None] * c['wo'][None, :, k]
    return acc


def decode_check(c, out_buf):
    """out_buf (M + GUARD, D) pre-filled with NaN"""
    assert_same_bits(region(out_buf, c['orows'], c['D'], 'lfq_decode'), decode_ref(c), 'lfq_decode')


# ------------------------------------------------------------------------------------------------ pk_peg

PEG_W = [4, 8, 16, 1, 3, 5, 17]
PEG_THD = [(1, 1, 4), (2, 2, 132), (5, 8, 512), (1, 8, 132), (2, 1, 512), (5, 2, 4), (1, 2, 512), (2, 8, 4), (5, 1, 132)]     # every (T, H), every D with every T
PEG_BLOCKS = [((2, 1, 1, 4, 4), 1), ((2, 5, 8, 8, 80), 7), ((2, 5, 8, 16, 112), 9), ((2, 5, 8, 4, 88), 7)]                       # (B, T, H, W, D) -> row-kernel blocks
PEG_BIG = (4, 8, 32, 17, 1024)                                    # the generic kernel's second grid-stride pass


def peg_row_blocks(B, T, H, D):
    return (B * T * H * (D // 4) + 255) // 256


def peg_case(B, T, H, W, D, causal, seed=0):
    """every sequence sits at its own large offset, so a stencil that reads across a sequence boundary shows"""
    g = gen(25, B, T, H, W, D, int(causal), seed)
    x = torch.randn(B, T, H, W, D, generator=g) + 50. * (1 + torch.arange(B, dtype=torch.float32)).reshape(B, 1, 1, 1, 1)
    return dict(shape=(B, T, H, W, D), causal=causal, x=x, wt=0.2 * torch.randn(27, D, generator=g), bias=torch.randn(D, generator=g))


def peg_taps(causal, tfront=None):
    tf = (2 if causal else 1) if tfront is None else tfront
    return [(dt, dh, dw, dt - tf, dh - 1, dw - 1) for dt in range(3) for dh in range(3) for dw in range(3)]


def peg_eval(c, dtype=torch.float64, tfront=None, residual=True, mirror=None, leak=False, reverse=False, absolute=False):
    """out = bias + sum over the 27 taps of x[t + dt - tfront, h + dh - 1, w + dw - 1] wt[tap] (zero outside the sequence) + x.  absolute: the sum of the
    absolute terms.  The other keywords are the named wrong kernels"""
    B, T, H, W, D = c['shape']
    x, wt, bias = c['x'].to(dtype), c['wt'].to(dtype), c['bias'].to(dtype)
    if absolute:
        x, wt, bias = x.abs(), wt.abs(), bias.abs()
    if leak:
        x, B, T = x.reshape(1, B * T, H, W, D), 1, B * T
    xp = F.pad(x, (0, 0, 1, 1, 1, 1, 2, 2))
    acc = bias.expand(B, T, H, W, D).clone()
    taps = peg_taps(c['causal'], tfront)
    for dt, dh, dw, ot, oh, ow in (reversed(taps) if reverse else taps):
        tap = (dt * 3 + dh) * 3 + dw
        k = wt[26 - tap if tap == mirror else tap]
        acc = acc + xp[:, 2 + ot:2 + ot + T, 1 + oh:1 + oh + H, 1 + ow:1 + ow + W] * k
    if residual:
        acc = acc + x
    return acc.reshape(c['shape'])


def peg_ref(c):
    return peg_eval(c), sum_bound(peg_eval(c, absolute=True), 29)          # 27 taps, the bias, the residual


def peg_buffers(c, device='cpu', with_t=True):
    B, T, H, W, D = c['shape']
    rows = B * T * H * W + GUARD
    return nan_buffer(rows, D, F32, device), (nan_buffer(rows, D, BF16, device) if with_t else None)


def peg_check(c, out, out_t, ref=None):
    B, T, H, W, D = c['shape']
    rows = torch.arange(B * T * H * W)
    y, bound = peg_ref(c) if ref is None else ref
    got = region(out, rows, D, 'peg out')
    ratio = assert_within(got, y.reshape(-1, D), bound.reshape(-1, D), 'peg out')
    if out_t is not None:
        check_bf16_of(region(out_t, rows, D, 'peg out_t'), got, 'peg out_t')
    return ratio


def peg_fake(c, y32, trunc=False):
    out, out_t = peg_buffers(c)
    D = c['shape'][-1]
    rows = torch.arange(y32.numel() // D)
    place(out, rows, y32.reshape(-1, D))
    out_t[rows] = truncated_bf16(y32.reshape(-1, D)) if trunc else rne(y32.reshape(-1, D))
    return out, out_t


def peg_active_mirror(c):
    """a tap that is inside the grid somewhere and is not its own mirror (none when T = H = W = 1 without the causal pad)"""
    B, T, H, W, D = c['shape']
    for dt, dh, dw, ot, oh, ow in peg_taps(c['causal']):
        tap = (dt * 3 + dh) * 3 + dw
        if tap != 13 and abs(ot) < T and abs(oh) < H and abs(ow) < W:
            return tap
    return None


# ------------------------------------------------------------------------------------------------ pk_embed

EMBED_CASES = [(1, 1, 0, 3, 4, 5), (2, 2, 2, 5, 4, 9), (3, 1, 0, 7, 512, 11), (2, 2, 3, 6, 512, 64)]        # (nb, replicas, n_prime, n, D, V)
EMBED_BIG = (4, 2, 100, 2000, 1024, 50)                           # S n_tot D / 4 = 4.3 M vectors: a second grid-stride pass


def embed_case(nb, rep, n_prime, n, D, V, seed=0):
    g = gen(26, nb, rep, n_prime, n, D, V, seed)
    ids = torch.randint(0, V, (nb, n), generator=g, dtype=torch.int64)
    ids.view(-1)[0], ids.view(-1)[-1] = 0, V - 1
    ids_prime = torch.randint(0, V, (nb, n_prime), generator=g, dtype=torch.int64) if n_prime else None
    if n_prime:
        ids_prime.view(-1)[0], ids_prime.view(-1)[-1] = V - 1, 0
    return dict(nb=nb, S=rep * nb, n_prime=n_prime, n=n, D=D, V=V, ids=ids, ids_prime=ids_prime, tok=torch.randn(V, D, generator=g),
                pos=torch.randn(n_prime + n, D, generator=g))


def embed_ref(c):
    """(S n_tot, D) f32: one rounded add"""
    both = torch.cat([c['ids_prime'], c['ids']], 1) if c['n_prime'] else c['ids']
    rows = both.repeat(c['S'] // c['nb'], 1)                      # sequence s reads id row s % nb
    return (c['pos'][None] + c['tok'][rows]).reshape(-1, c['D'])


def embed_check(c, out, out_t):
    want = embed_ref(c)
    rows = torch.arange(want.shape[0])
    got = region(out, rows, c['D'], 'embed out')
    assert_same_bits(got, want, 'embed out')
    if out_t is not None:
        check_bf16_of(region(out_t, rows, c['D'], 'embed out_t'), got, 'embed out_t')


# ------------------------------------------------------------------------------------------------ pk_cfg_mix

# (nb, n_tot, n_prime, D, has_null, gather, scale, wide)
CFG_CASES = [(2, 10, 3, 128, 1, False, 5., False), (2, 10, 0, 128, 1, True, 5., True), (3, 7, 2, 4, 0, True, 5., True), (1, 5, 0, 516, 1, False, 0., True),
             (2, 6, 1, 260, 1, True, 1., False), (2, 6, 0, 64, 0, False, 1., False)]
CFG_BIG = (4, 30, 5, 2048, 1, 8200, 5.)                           # nrows D / 4 = 4.2 M vectors through a gather with repeats


def cfg_case(nb, n_tot, n_prime, D, has_null, gather, scale, wide, nrows=None, seed=0):
    g = gen(27, nb, n_tot, n_prime, D, has_null, seed)
    n = n_tot - n_prime
    x = torch.randn((1 + has_null) * nb * n_tot, D, generator=g)
    rows = None
    if gather:
        k = nrows or nb * n + 3
        rows = torch.randint(0, nb * n, (k,), generator=g, dtype=torch.int32)
        rows[0], rows[1], rows[2 % k] = nb * n - 1, 0, nb * n - 1     # not monotone, a repeated row
    return dict(nb=nb, n_tot=n_tot, n_prime=n_prime, D=D, has_null=has_null, rows=rows, nrows=rows.numel() if gather else nb * n, scale=scale,
                x=widen(x, 4 if wide else 0), ldo=D + (8 if wide else 0))


def cfg_ref(c):
    """null + (cond - null) scale: the difference, the product and the add are each rounded once (fused or not): U (2 |scale d| + |y|); without the null
    half a copy, bit for bit"""
    nb, n_tot, n_prime, D = c['nb'], c['n_tot'], c['n_prime'], c['D']
    n = n_tot - n_prime
    lr = c['rows'].long() if c['rows'] is not None else torch.arange(nb * n)
    src = (lr // n) * n_tot + lr % n + n_prime
    x = c['x'][:, :D].double()
    cond = x[src]
    if not c['has_null']:
        return cond, torch.zeros_like(cond)
    null = x[nb * n_tot + src]
    s = float(torch.tensor(c['scale'], dtype=F32))
    y = null + (cond - null) * s
    return y, U * (2 * abs(s) * (cond - null).abs() + y.abs())


def cfg_check(c, out, f32_out=None):
    """out (nrows + GUARD, ldo) NaN-filled; a bf16 out is checked against the f32 launch's region"""
    y, bound = cfg_ref(c)
    got = region(out, torch.arange(c['nrows']), c['D'], 'cfg_mix')
    if got.dtype == BF16:
        check_bf16_of(got, f32_out, 'cfg_mix')
        return 0., None
    if not c['has_null']:
        assert_same_bits(got, y.float(), 'cfg_mix without the null half (a copy)')
        return 0., got
    return assert_within(got, y, bound, 'cfg_mix'), got


# ------------------------------------------------------------------------------------------------ pk_critic_head

CRITIC_D = [4, 252, 256, 260, 1024]
CRITIC_SEED, CRITIC_SEED_DEV = 0x0123456789ABCDEF - 1000, 1000


def critic_case(D, has_null, n_prime, has_b, noise, seed=0):
    """nb * n = 5 output rows: a partial block.  noise: 'u' | 'hash' | 'none'"""
    from tests.util import uniform24_np
    g = gen(28, D, has_null, n_prime, seed)
    nb, n = (5, 1) if n_prime else (1, 5)
    n_tot = n + n_prime
    x = torch.randn((1 + has_null) * nb * n_tot, D, generator=g)
    u = torch.rand(nb * n, generator=g) if noise == 'u' else None
    if noise == 'hash':
        r = np.arange(nb * n, dtype=np.uint64) | (np.uint64(0xC817) << np.uint64(32))
        u_eff = torch.from_numpy(uniform24_np(CRITIC_SEED + CRITIC_SEED_DEV, r))
    else:
        u_eff = u
    return dict(D=D, nb=nb, n=n, n_tot=n_tot, n_prime=n_prime, has_null=has_null, x=widen(x, 4), w=torch.randn(D, generator=g) / D ** 0.5,
                b=torch.tensor([0.3]) if has_b else None, scale=5., u=u, u_eff=u_eff, noise=noise, noise_mult=0.5 if noise != 'none' else 0.)


def critic_ref(c):
    """s = x . w + b per half (sum_bound over D terms), null + (cond - null) scale (both halves' bounds, three roundings), + noise_mult (u - 0.5) (three more)"""
    nb, n, n_tot, n_prime, D = c['nb'], c['n'], c['n_tot'], c['n_prime'], c['D']
    r = torch.arange(nb * n)
    src = (r // n) * n_tot + r % n + n_prime
    x, w = c['x'][:, :D].double(), c['w'].double()
    b = float(c['b']) if c['b'] is not None else 0.
    dot = lambda rows: (x[rows] @ w + b, sum_bound(x[rows].abs() @ w.abs() + abs(b), D))
    s, sb = dot(src)
    if c['has_null']:
        sn, snb = dot(nb * n_tot + src)
        y = sn + (s - sn) * c['scale']
        s, sb = y, snb + abs(c['scale']) * (sb + snb) + U * (2 * abs(c['scale']) * (s - sn).abs() + y.abs())
    if c['u_eff'] is not None:
        nz = c['noise_mult'] * (c['u_eff'].double() - 0.5)
        s, sb = s + nz, sb + U * (2 * nz.abs() + (s + nz).abs())
    return s, sb


def critic_f32(c, order=0):
    """the formula in f32, the dot products in one of two association orders"""
    nb, n, n_tot, n_prime, D = c['nb'], c['n'], c['n_tot'], c['n_prime'], c['D']
    r = torch.arange(nb * n)
    src = (r // n) * n_tot + r % n + n_prime
    x, w = c['x'][:, :D], c['w'][None]
    b = c['b'] if c['b'] is not None else torch.zeros(1)
    s = dot32(x[src], w, order)[:, 0] + b
    if c['has_null']:
        sn = dot32(x[nb * n_tot + src], w, order)[:, 0] + b
        s = sn + (s - sn) * torch.tensor(c['scale'])
    if c['u_eff'] is not None:
        s = s + torch.tensor(c['noise_mult']) * (c['u_eff'] - 0.5)
    return s


def critic_check(c, out):
    """out (nb n + GUARD,) NaN-filled"""
    y, bound = critic_ref(c)
    o = out.detach().cpu()
    assert_untouched(o[y.numel():], 'critic_head beyond the output rows')
    return assert_within(o[:y.numel()], y, bound, 'critic_head')


# ------------------------------------------------------------------------------------------------ pk_topk_mask

TOPK_N = [1, 5, 63, 64, 65, 255, 257, 12288]
TOPK_KINDS = ['equal', 'few', 'zeros', 'inf', 'randn']
TOPK_MASK_ID = 100


def topk_scores(kind, n, g):
    if kind == 'equal':
        return torch.full((n,), 0.25)
    if kind == 'few':                                             # what the sampler feeds: -1e4 on every unmasked position
        s = torch.full((n,), -1e4)
        idx = torch.randperm(n, generator=g)[:max(1, n // 8)]
        s[idx] = torch.rand(idx.numel(), generator=g)
        return s
    if kind == 'zeros':
        s = torch.zeros(n)
        s[torch.rand(n, generator=g) < 0.5] = -0.
        s[torch.rand(n, generator=g) < 0.1] = 1.
        return s
    if kind == 'inf':
        s = torch.randn(n, generator=g)
        r = torch.rand(n, generator=g)
        s[r < 0.3], s[r > 0.7] = float('inf'), -float('inf')
        return s
    return torch.randn(n, generator=g)


def topk_case(n, k, seed=0):
    """one batch row per kind of score row"""
    g = gen(29, n, k, seed)
    B = len(TOPK_KINDS)
    return dict(B=B, n=n, k=k, scores=torch.stack([topk_scores(kind, n, g) for kind in TOPK_KINDS]), ids0=torch.randint(0, TOPK_MASK_ID, (B, n), generator=g, dtype=torch.int64))


def topk_ranks(scores, higher_first=False):
    """rank[b][i] = place of i in the stable descending sort of row b: the kernel's documented rule, lower index first on ties"""
    if higher_first:
        order = scores.shape[1] - 1 - torch.sort(scores.flip(1), dim=1, descending=True, stable=True).indices
    else:
        order = torch.sort(scores, dim=1, descending=True, stable=True).indices
    rank = torch.empty_like(order)
    rank.scatter_(1, order, torch.arange(scores.shape[1]).expand_as(order))
    return rank


def topk_buffers(c, device='cpu'):
    """mask (B n + GUARD) uint8 filled with 7, ids (B n + GUARD) int64: the ids before the call and SENTINEL behind them, rows_out (B k + GUARD) int32
    SENTINEL, scores_next (B n + GUARD) NaN"""
    Bn = c['B'] * c['n']
    ids = torch.full((Bn + GUARD,), SENTINEL, dtype=torch.int64)
    ids[:Bn] = c['ids0'].reshape(-1)
    return (torch.full((Bn + GUARD,), 7, dtype=torch.uint8, device=device), ids.to(device), torch.full((c['B'] * c['k'] + GUARD,), SENTINEL, dtype=torch.int32, device=device),
            torch.full((Bn + GUARD,), NAN, device=device))


def topk_check(c, mask, ids, rows_out, scores_next):
    B, n, k = c['B'], c['n'], c['k']
    Bn = B * n
    mask, ids, rows_out, scores_next = (t.detach().cpu() for t in (mask, ids, rows_out, scores_next))
    rank = topk_ranks(c['scores'])
    sel = rank < k
    assert (mask[Bn:] == 7).all() and (ids[Bn:] == SENTINEL).all() and (rows_out[B * k:] == SENTINEL).all(), 'topk_mask: written behind an output'
    assert_untouched(scores_next[Bn:], 'topk_mask scores_next beyond B n')
    assert torch.equal(mask[:Bn].reshape(B, n), sel.to(torch.uint8)), 'topk_mask mask'
    assert torch.equal(ids[:Bn].reshape(B, n), torch.where(sel, torch.tensor(TOPK_MASK_ID), c['ids0'])), 'topk_mask ids'
    order = torch.sort(c['scores'], dim=1, descending=True, stable=True).indices[:, :k] + torch.arange(B)[:, None] * n
    assert torch.equal(rows_out[:B * k].long(), order.reshape(-1)), 'topk_mask rows_out (rank order)'
    assert_same_bits(scores_next[:Bn], torch.full((Bn,), -1e4), 'topk_mask scores_next')


def topk_fake(c, higher_first=False, le=False):
    mask, ids, rows_out, nxt = topk_buffers(c)
    B, n, k = c['B'], c['n'], c['k']
    rank = topk_ranks(c['scores'], higher_first)
    sel = (rank <= k) if le else (rank < k)
    mask[:B * n] = sel.reshape(-1).to(torch.uint8)
    ids[:B * n] = torch.where(sel, torch.tensor(TOPK_MASK_ID), c['ids0']).reshape(-1)
    bb, ii = sel.nonzero(as_tuple=True)
    keep = rank[bb, ii] < k                                       # rows_out has B k entries
    rows_out[(bb * k + rank[bb, ii])[keep]] = (bb * n + ii)[keep].int()
    nxt[:B * n] = -1e4
    return mask, ids, rows_out, nxt


# ------------------------------------------------------------------------------------------------ pk_rmsnorm, pk_l2norm_rows, pk_gated_gelu_tanh

ROW_D = [4, 252, 256, 260, 4096]
ROW_M = [1, 5, 300]


def rms_case(M, D, masked, seed=0):
    """rows of magnitude 1e-3 (mean square about eps), 1 and 1e4"""
    g = gen(30, M, D, seed)
    x = torch.randn(M, D, generator=g) * torch.tensor([1e-3, 1., 1e4])[torch.arange(M) % 3][:, None]
    rowmask = (torch.arange(M) % 4 != 1).to(torch.uint8) if masked else None
    return dict(M=M, D=D, x=widen(x, 4), w=1 + 0.3 * torch.randn(D, generator=g), rowmask=rowmask, ldo=D + 8)


def rms_ref(c):
    """y = x w / sqrt(mean(x^2) + eps): the D positive terms of the mean square carry (D + 8) U relatively, the division, the add of eps, the root and the
    reciprocal one U each, all halved by the root except the last two; then two products"""
    D = c['D']
    x, w = c['x'][:, :D].double(), c['w'].double()
    y = x * w / torch.sqrt((x * x).mean(1, keepdim=True) + RMS_EPS)
    bound = y.abs() * (0.5 * (D + 10) * U + 4 * U)
    if c['rowmask'] is not None:
        keep = c['rowmask'].bool()[:, None]
        y, bound = torch.where(keep, y, torch.zeros_like(y)), torch.where(keep, bound, torch.zeros_like(bound))
    return y, bound


def rms_f32(c, order=0, center=False):
    D = c['D']
    x = c['x'][:, :D]
    if center:                                                    # the wrong kernel: a LayerNorm's mean subtraction
        x = x - (sum32(x, order) / D)[:, None]
    y = x * (1.0 / torch.sqrt(sum32(x * x, order) / D + RMS_EPS))[:, None] * c['w']
    return y if c['rowmask'] is None else torch.where(c['rowmask'].bool()[:, None], y, torch.zeros_like(y))


def rows_check(c, out, ref, what, f32_out=None, zero_rows=None):
    """out (M + GUARD, ldo) NaN-filled, f32 held to the float64 bound or bf16 held to the f32 launch; zero_rows: rows that are +0.0 bit for bit"""
    y, bound = ref
    got = region(out, torch.arange(c['M']), y.shape[1], what)
    if zero_rows is not None and zero_rows.any():
        assert_same_bits(got[zero_rows], torch.zeros_like(got[zero_rows]), f'{what}: the rows that are exact zeros')
    if got.dtype == BF16:
        check_bf16_of(got, f32_out, what)
        return 0., None
    return assert_within(got, y, bound, what), got


def rms_zero_rows(c):
    return ~c['rowmask'].bool() if c['rowmask'] is not None else None


def l2_case(M, D, seed=0):
    """row norms spread over 1e-6 ... 1e6; row 1 (where there is one) is an exact zero row"""
    g = gen(31, M, D, seed)
    x = torch.randn(M, D, generator=g)
    target = 10.0 ** (torch.arange(M) % 13 - 6.).double()
    x = (x.double() / x.double().norm(dim=1, keepdim=True) * target[:, None]).float()
    if M > 1:
        x[1] = 0.
    return dict(M=M, D=D, x=widen(x, 4), ldo=D + 8)


def l2_ref(c):
    """y = x / max(|x|, 1e-12): the D positive squares (D + 8) U relatively, halved by the root; the root, the reciprocal and the product one U each"""
    D = c['D']
    x = c['x'][:, :D].double()
    y = x / x.norm(dim=1, keepdim=True).clamp_min(1e-12)
    return y, y.abs() * (0.5 * (D + 8) * U + 4 * U)


def l2_f32(c, order=0):
    x = c['x'][:, :c['D']]
    return x * (1.0 / torch.sqrt(sum32(x * x, order)).clamp_min(1e-12))[:, None]


def l2_zero_rows(c):
    return (c['x'][:, :c['D']] == 0).all(1)


# the transcendental allowances: the largest err / (U scale) of torch's f32 CPU evaluation of the same formula against float64 on the case inputs, measured and
# asserted by tests/test_infer_glue_host.py, times 4 for the device library (a different implementation, allowed a few ulp of its own)
GELU_CPU_RATIO = 1.4           # measured 1.298 (tests/test_infer_glue_host.py::test_transcendental_allowances), recorded rounded up; factor 4
GELU_C = 4 * GELU_CPU_RATIO
CPB_CPU_RATIO = 1.6            # measured 1.521, recorded rounded up; factor 4
CPB_C = 4 * CPB_CPU_RATIO
GELU_K = 0.7978845608028654


def gelu_case(M, Fd, seed=0):
    """h (M, 2 F + 4): gate values across [-20, 20] with 0.0, -0.0 and +-1e4 among them, linear values random"""
    g = gen(32, M, Fd, seed)
    a = (torch.rand(M, Fd, generator=g) * 40 - 20)
    a[torch.rand(M, Fd, generator=g) < 0.3] *= 0.1                # more of them where tanh is not saturated
    special = torch.tensor([0., -0., 1e4, -1e4])
    if a.numel() >= 8:
        a.view(-1)[:4] = special
    b = torch.randn(M, Fd, generator=g)
    return dict(M=M, D=Fd, h=widen(torch.cat([a, b], 1), 4), ldo=Fd + 8)


def gelu_formula(a, b):
    return 0.5 * a * (1.0 + torch.tanh(GELU_K * (a + 0.044715 * a * a * a))) * b


def gelu_ref(c, cc=None):
    Fd = c['D']
    a, b = c['h'][:, :Fd].double(), c['h'][:, Fd:2 * Fd].double()
    y = gelu_formula(a, b)
    return y, (GELU_C if cc is None else cc) * U * (y.abs() + (a * b).abs())


def gelu_f32(c):
    Fd = c['D']
    return gelu_formula(c['h'][:, :Fd], c['h'][:, Fd:2 * Fd])


def unit_ratio(got, ref_with_unit_c):
    y, bound = ref_with_unit_c
    return max_ratio((got.double() - y).abs(), bound)


# ------------------------------------------------------------------------------------------------ pk_patchify_ln / pk_unpatchify

# (B, C, F, H, W, f0, nt, pt, ph, pw): P = 4, 4096 (P / 4 = 1024: the narrow template's end), 4112 (1028: the wide one's start), 8192 (its end)
PATCH_CASES = [(2, 1, 3, 2, 8, 1, 2, 1, 1, 4), (1, 1, 3, 64, 128, 1, 2, 1, 64, 64), (1, 1, 2, 257, 32, 1, 1, 1, 257, 16), (1, 2, 3, 64, 128, 1, 2, 1, 64, 64),
               (2, 3, 5, 8, 12, 1, 2, 2, 4, 4)]
UNPATCH_BIG = (8, 3, 8, 256, 256, 1, 3, 2, 8, 8)                  # 2.36 M vectors: more than 8192 blocks' worth


def patch_P(geom):
    B, C, Fr, H, W, f0, nt, pt, ph, pw = geom
    return C * pt * ph * pw


def patch_rows(geom):
    B, C, Fr, H, W, f0, nt, pt, ph, pw = geom
    return B * nt * (H // ph) * (W // pw)


def patch_case(geom, seed=0):
    B, C, Fr, H, W, f0, nt, pt, ph, pw = geom
    g = gen(33, *geom, seed)
    P = patch_P(geom)
    video = torch.randn(B, C, Fr, H, W, generator=g) * 0.5 + 0.3
    video[0, :, f0:f0 + pt] = torch.randn(C, pt, H, W, generator=g) * (4 * LN_EPS) ** 0.5          # the first temporal patch of sample 0: variance 4 eps
    return dict(geom=geom, P=P, rows=patch_rows(geom), video=video, weight=1 + 0.3 * torch.randn(P, generator=g), bias=0.3 * torch.randn(P, generator=g), ldo=P + 8)


def patch_src(c):
    B, C, Fr, H, W, f0, nt, pt, ph, pw = c['geom']
    return patchify(c['video'], f0, nt, pt, ph, pw)


def patch_check(c, out, with_ln, f32_out=None):
    """out (rows + GUARD, ldo) NaN-filled"""
    src = patch_src(c)
    got = region(out, torch.arange(c['rows']), c['P'], 'patchify_ln')
    if got.dtype == BF16:
        check_bf16_of(got, f32_out, 'patchify_ln')
        return 0., None
    if not with_ln:
        assert_same_bits(got, src.contiguous(), 'patchify_ln raw rows (a copy)')
        return 0., got
    y, bound = ln_ref(src, c['weight'], c['bias'])
    return assert_within(got, y, bound, 'patchify_ln'), got


def unpatch_case(geom, seed=0):
    P, rows = patch_P(geom), patch_rows(geom)
    return dict(geom=geom, P=P, rows=rows, pix=widen(torch.randn(rows, P, generator=gen(34, *geom, seed)), 4))


def unpatch_check(c, video):
    """video (B, C, F, H, W) NaN-filled before the call: the frames [f0, f0 + nt pt) hold the pixels, every other frame is still NaN"""
    B, C, Fr, H, W, f0, nt, pt, ph, pw = c['geom']
    v = video.detach().cpu()
    assert_same_bits(patchify(v, f0, nt, pt, ph, pw).contiguous(), c['pix'][:, :c['P']].contiguous(), 'unpatchify (a copy)')
    assert_untouched(v[:, :, :f0], 'unpatchify frames before f0')
    assert_untouched(v[:, :, f0 + nt * pt:], 'unpatchify frames after the group')


# ------------------------------------------------------------------------------------------------ pk_cpb_input

CPB_CASES = [((7,), 5), ((1, 6), 5), ((3, 4), 64), ((2, 1, 3), 64), ((3, 2, 2), 5)]           # (dims, D): nd 1, 2, 3, an extent of 1, D without vector alignment
CPB_BIG = ((9, 8, 8), 64)                                         # n^2 D = 21 M elements: a second grid-stride pass


def cpb_case(dims, D, seed=0):
    g = gen(35, *dims, D, seed)
    nd = len(dims)
    return dict(dims=dims, nd=nd, D=D, n=math.prod(dims), w0=torch.randn(D, nd, generator=g), b0=torch.randn(D, generator=g))


def cpb_rel(c, dtype):
    """(n, n, nd): sign(rel) log(|rel| + 1) of the 'ij' meshgrid positions"""
    grid = torch.stack(torch.meshgrid(*[torch.arange(d) for d in c['dims']], indexing='ij')).reshape(c['nd'], -1).t()
    rel = (grid[:, None, :] - grid[None, :, :]).to(dtype)
    return torch.sign(rel) * torch.log(rel.abs() + 1)


def cpb_ref(c, cc=None):
    """(n n, D): leaky_relu(W0 v + b0, 0.1) and CPB_C U (|acc| + sum |w0| log(|rel| + 1) + |b0|)"""
    v = cpb_rel(c, torch.float64)
    w0, b0 = c['w0'].double(), c['b0'].double()
    acc = v @ w0.t() + b0
    scale = acc.abs() + v.abs() @ w0.abs().t() + b0.abs()
    return F.leaky_relu(acc, 0.1).reshape(-1, c['D']), ((CPB_C if cc is None else cc) * U * scale).reshape(-1, c['D'])


def cpb_f32(c):
    v = cpb_rel(c, F32)
    acc = c['b0'].expand(c['n'], c['n'], c['D']).clone()
    for a in range(c['nd']):
        acc = acc + c['w0'][:, a] * v[..., a, None]
    return torch.where(acc > 0, acc, 0.1 * acc).reshape(-1, c['D'])


def cpb_check(c, out):
    """out (n n D + GUARD) NaN-filled"""
    y, bound = cpb_ref(c)
    o = out.detach().cpu()
    assert_untouched(o[y.numel():], 'cpb_input beyond the output')
    return assert_within(o[:y.numel()].reshape(y.shape), y, bound, 'cpb_input')
