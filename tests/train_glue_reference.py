"""CPU float64 restatements of the loss heads and glue kernels of the two training steps (csrc/train.hip, sampler.hip, patch.hip, attn_train.hip), in plain
torch, with the seeded inputs and the checkers that tests/test_train_glue_gpu.py runs on the kernels' outputs.  tests/test_train_glue_host.py holds the
restatements to float64 autograd and feeds every checker its own reference with one planted error, so a checker that cannot fail is itself a failure.

Every bound is derived from the operation, never from what a kernel returned: U = 2^-24 is the unit roundoff of f32, sum_bound is the any-order f32
summation bound, and the elementwise kernels (a select, a copy, one or two rounded operations) are held bit for bit to the same expression in f32."""
import torch
import torch.nn.functional as F

U = 2.0 ** -24
V_FULL = 448                 # the vocabulary of the cross-entropy cases: slabs of 192 leave a short last slab
NAN = float('nan')


def gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------ the two helpers and their bit-exact siblings

def sum_bound(terms_abs_sum, n, extra=8):
    """|fl(sum of n terms) - sum| <= n U sum|terms| in any order, plus `extra` elementwise roundings of the terms"""
    return (n + extra) * U * terms_abs_sum


def assert_within(a, ref64, bound, what):
    """EVERY element of a within its own bound of the float64 reference (no outlier share, no norm-relative fallback; NaN fails).
    Returns the largest err / bound."""
    a = torch.as_tensor(a).detach().cpu().double()
    ref = torch.as_tensor(ref64).detach().cpu().double()
    assert a.shape == ref.shape, f'{what}: shape {tuple(a.shape)} vs {tuple(ref.shape)}'
    bound = torch.as_tensor(bound, dtype=torch.float64).detach().cpu().broadcast_to(ref.shape)
    assert torch.isfinite(ref).all() and torch.isfinite(bound).all() and (bound >= 0).all(), f'{what}: the reference or its bound is not finite'
    if a.numel() == 0:
        return 0.
    err = (a - ref).abs()
    bad = ~(err <= bound)
    if bad.any():
        i = int(bad.reshape(-1).nonzero()[0])
        idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), ref.shape)) if ref.dim() else ()
        raise AssertionError(f'{what}: element {idx} is {a.reshape(-1)[i].item()!r}, reference {ref.reshape(-1)[i].item()!r}: error '
                             f'{err.reshape(-1)[i].item():.3e} beyond its bound {bound.reshape(-1)[i].item():.3e} ({int(bad.sum())} of {a.numel()} out of bound)')
    return float(torch.where(err > 0, err / bound.clamp_min(1e-300), torch.zeros_like(err)).max())


_INT_OF = {torch.float32: torch.int32, torch.bfloat16: torch.int16, torch.float64: torch.int64}


def _bits(t):
    t = t.detach().cpu().contiguous()
    return t.view(_INT_OF[t.dtype]) if t.dtype in _INT_OF else t


def assert_same_bits(a, want, what):
    """bit for bit: -0.0 is not 0.0, a NaN equals only the same NaN"""
    a, want = a.detach().cpu(), want.detach().cpu()
    assert a.shape == want.shape and a.dtype == want.dtype, f'{what}: {tuple(a.shape)} {a.dtype} vs {tuple(want.shape)} {want.dtype}'
    ne = _bits(a) != _bits(want)
    if ne.any():
        i = int(ne.reshape(-1).nonzero()[0])
        idx = tuple(int(x) for x in torch.unravel_index(torch.tensor(i), a.shape))
        raise AssertionError(f'{what}: {int(ne.sum())} of {a.numel()} elements differ bit for bit, first at {idx}: '
                             f'{a.reshape(-1)[i].item()!r} instead of {want.reshape(-1)[i].item()!r}')


def assert_untouched(buf, what):
    """a float region pre-filled with NaN still holds nothing else"""
    if buf.numel() and not torch.isnan(buf.detach().cpu().float()).all():
        raise AssertionError(f'{what}: written outside the output ({int((~torch.isnan(buf.detach().cpu().float())).sum())} elements)')


def assert_written(buf, what):
    if not torch.isfinite(buf.detach().cpu().double()).all():
        raise AssertionError(f'{what}: {int((~torch.isfinite(buf.detach().cpu().double())).sum())} elements not written (or not finite)')


def f32_scale(scale, dev):
    """scale * dev[0] as the kernels form it: one f32 product"""
    s = torch.tensor(scale, dtype=torch.float32)
    return float(s * torch.tensor(dev, dtype=torch.float32)) if dev is not None else float(s)


# ------------------------------------------------------------------------------------------------ pk_ce_grad_slab

CE_SHAPES = [(77, 100, 96), (77, 100, 128), (32, 64, 32), (33, 40, 128), (1, 1, 32), (300, 256, 320)]       # (M, Vs, ldgt)


def ce_full(M, seed=0):
    """(M, V_FULL) f32 logits and the f32 rounding of their float64 log-sum-exp"""
    full = (torch.randn(M, V_FULL, generator=gen(1, M, seed), dtype=torch.float64) * 3).float()
    lse = torch.logsumexp(full.double(), 1).float()
    assert (full.double() - lse.double()[:, None]).abs().max() <= 30
    return full, lse


def ce_case(M, Vs, ldgt, v0, wide=False, use_rows=False, use_dev=False, seed=0):
    """one call: the slab [v0, v0 + Vs) of the full rows.  Row m's target cycles through v0 - 1, v0, v0 + Vs - 1, v0 + Vs, a column inside, 0 and
    V_FULL - 1 (those that exist in [0, V_FULL)): below, on both edges, inside and above the slab.  rows: an injective non-identity gather into a
    longer `targets` (lse stays indexed by m)"""
    assert v0 + Vs <= V_FULL and ldgt >= M
    full, lse = ce_full(M, seed)
    g = gen(2, M, Vs, v0, seed)
    T = M + 5 if use_rows else M
    rows = ((torch.arange(M) * 3 + 2) % T).int() if use_rows else None
    assert rows is None or (rows.unique().numel() == M and not torch.equal(rows.long(), torch.arange(M)))
    cand = [t for t in (v0 - 1, v0, v0 + Vs - 1, v0 + Vs, None, 0, V_FULL - 1) if t is None or 0 <= t < V_FULL]
    inside = v0 + torch.randint(0, Vs, (M,), generator=g)
    tm = torch.tensor([int(inside[m]) if cand[m % len(cand)] is None else cand[m % len(cand)] for m in range(M)], dtype=torch.int64)
    targets = torch.randint(0, V_FULL, (T,), generator=g, dtype=torch.int64)
    targets[rows.long() if rows is not None else torch.arange(M)] = tm
    ld = Vs + 8 if wide else Vs
    logits = torch.full((M, ld), NAN, dtype=torch.float32)
    logits[:, :Vs] = full[:, v0:v0 + Vs]
    return dict(M=M, Vs=Vs, ldgt=ldgt, v0=v0, ld=ld, logits=logits, lse=lse, targets=targets, rows=rows, row_targets=tm, scale=1.0 / M,
                dev=0.37 if use_dev else None)


def ce_ref(c, onehot_offset=None, stated=False):
    """float64 g = (exp(l - lse) - onehot) * scale and its per-element bound.

    stated: |scale| (p (|l - lse| + 4) 2^-22 + 2^-24) with p = exp(l - lse) -- the rounding of the argument and of its product with log2(e) and the hardware
    exponential's last bit, all relative to p, plus one 2^-24.  That holds every element but the one-hot ones to what a correctly rounded evaluation gives.
    At a one-hot element with a small p the p-relative part vanishes and TWO roundings remain, p - 1 (half an ulp of a number in [1/2, 1]: 2^-25) and the
    product with scale (2^-24 |g|): up to 1.5 x 2^-24 |scale| where the stated bound allows 1.0.  The same expression evaluated in f32 on the CPU (ce_f32)
    misses the stated bound there too, at 52 of the 2576 one-hot elements of the GPU test's cases: its largest error is 1.24 x 2^-24 |scale| (the base;
    eight times that, 9.9 x 2^-24 |scale|, is what a measured allowance would be).  The bound used is the tighter derived one: at the one-hot elements
    only, the stated bound's 2^-24 |scale| becomes 2^-25 |scale| + 2^-24 |g| where that is larger (at most 1.5 x 2^-24 |scale|); every other element keeps
    the stated bound.  (scale is the f32 product scale * scale_dev the kernel forms: no rounding of its own against this reference)"""
    x = c['logits'][:, :c['Vs']].double() - c['lse'].double()[:, None]
    p = torch.exp(x)
    v0 = c['v0'] if onehot_offset is None else onehot_offset
    onehot = (c['row_targets'][:, None] == v0 + torch.arange(c['Vs'])[None]).double()
    s = f32_scale(c['scale'], c['dev'])
    g = (p - onehot) * s
    last = torch.full_like(p, U * abs(s))
    if not stated:
        last = torch.where(onehot > 0, torch.maximum(last, abs(s) * 2.0 ** -25 + U * g.abs()), last)
    return g, abs(s) * p * (x.abs() + 4) * 2.0 ** -22 + last


def ce_f32(c):
    """the restatement evaluated in f32 on the CPU, every operation rounded once (torch's expf is within an ulp)"""
    x = c['logits'][:, :c['Vs']] - c['lse'][:, None]
    onehot = (c['row_targets'][:, None] == c['v0'] + torch.arange(c['Vs'])[None]).float()
    return (torch.exp(x) - onehot) * torch.tensor(f32_scale(c['scale'], c['dev']), dtype=torch.float32)


def ce_check(c, g, gT, db, f32_out=None):
    """g (M, ld), gT (Vs + 2, ldgt), db (Vs + 3,) or None, all pre-filled with NaN.  f32_out = (g, gT) of the f32 call when g is bf16.
    Returns the largest err / bound of g and of db"""
    M, Vs = c['M'], c['Vs']
    ratios = dict(g=0., db=0.)
    if g.dtype == torch.float32:
        ref, bound = ce_ref(c)
        ratios['g'] = assert_within(g[:, :Vs], ref, bound, 'ce_grad_slab g')
    else:
        assert g.dtype == torch.bfloat16 and gT.dtype == torch.bfloat16 and f32_out is not None
        assert_same_bits(g[:, :Vs], f32_out[0][:, :Vs].to(torch.bfloat16), 'ce_grad_slab bf16 g against the rounding of the f32 g')
        assert_same_bits(gT[:Vs], f32_out[1][:Vs].to(torch.bfloat16), 'ce_grad_slab bf16 gT against the rounding of the f32 gT')
    assert_untouched(g[:, Vs:], 'ce_grad_slab g columns >= Vs')
    assert_same_bits(gT[:Vs, :M], g[:, :Vs].t().contiguous(), 'ce_grad_slab gT against the transpose of g')
    assert_same_bits(gT[:Vs, M:], torch.zeros_like(gT[:Vs, M:]), 'ce_grad_slab gT pad columns [M, ldgt)')
    assert_untouched(gT[Vs:], 'ce_grad_slab gT rows >= Vs')
    if db is not None:
        stored = g[:, :Vs].double()
        ratios['db'] = assert_within(db[:Vs], stored.sum(0), sum_bound(stored.abs().sum(0), M), 'ce_grad_slab db')
        assert_untouched(db[Vs:], 'ce_grad_slab db beyond Vs')
    return ratios


def ce_buffers(c, dtype=torch.float32, device='cpu'):
    return (torch.full((c['M'], c['ld']), NAN, dtype=dtype, device=device), torch.full((c['Vs'] + 2, c['ldgt']), NAN, dtype=dtype, device=device),
            torch.full((c['Vs'] + 3,), NAN, dtype=torch.float32, device=device))


def ce_fake(c, dtype=torch.float32, ref=None):
    """what a correct kernel would leave in ce_buffers (the reference rounded to f32): the planted-error tests start from here"""
    g, gT, db = ce_buffers(c, dtype)
    M, Vs = c['M'], c['Vs']
    g[:, :Vs] = (ce_ref(c)[0] if ref is None else ref).float().to(dtype)
    gT[:Vs] = 0
    gT[:Vs, :M] = g[:, :Vs].t()
    db[:Vs] = g[:, :Vs].double().sum(0).float()
    return g, gT, db


# ------------------------------------------------------------------------------------------------ pk_bce_head

BCE_SHAPES = [(1, 4), (7, 64), (77, 516), (9, 1024), (8200, 64)]          # (M, D)
BCE_Z = (100., -100., 40., -40., 1e-3, -1e-3, 0.)


def ln_bwd_parts(M):
    """pk_ln_bwd_parts: 8 rows per block, 1 ... 1024 blocks"""
    return min(max((M + 7) // 8, 1), 1024)


def bce_case(M, D, wide=False, has_b=True, use_dev=False, seed=0):
    """the first rows are multiples of w that put the logit at BCE_Z, row 7 is all zero; labels are 0 / 1"""
    g = gen(3, M, D, seed)
    e = torch.randn(M, D, generator=g)
    w = torch.randn(D, generator=g) / D ** 0.5
    b = torch.tensor([0.3]) if has_b else None
    w64 = w.double()
    for i, z in enumerate(BCE_Z[:M]):
        e[i] = (w64 * ((z - (0.3 if has_b else 0.)) / (w64 * w64).sum())).float()
    if M > 7:
        e[7] = 0.
    labels = (torch.rand(M, generator=g) < 0.5).float()
    ld = D + 4 if wide else D
    ebuf = torch.full((M, ld), NAN)
    ebuf[:, :D] = e
    return dict(M=M, D=D, ld=ld, e=ebuf, w=w, b=b, labels=labels, scale=1.0 / M, dev=0.37 if use_dev else None)


def bce_ref(c, with_labels=True):
    """logit = e . w + b; loss = max(z, 0) - z y + log(1 + exp(-|z|)); dz = (sigmoid(z) - y) scale; de = dz w; dw = sum_m dz e; db = sum_m dz.
    The logit bound zb = sum_bound(sum|e w|, D) is carried through the loss (|d loss / dz| <= 1) and, for de, through sigmoid (|d sigma / dz| <= 1/4);
    dw and db are held to sum_bound over their M terms alone"""
    M, D = c['M'], c['D']
    e, w = c['e'][:, :D].double(), c['w'].double()
    b = c['b'].double() if c['b'] is not None else torch.zeros(1, dtype=torch.float64)
    z = e @ w + b
    zb = sum_bound((e * w).abs().sum(1) + b.abs(), D)
    r = dict(z=z, zb=zb)
    if not with_labels:
        return r
    y = c['labels'].double()
    s = f32_scale(c['scale'], c['dev'])
    r['loss'] = z.clamp_min(0) - z * y + torch.log1p(torch.exp(-z.abs()))
    r['loss_bound'] = zb + 4 * U * r['loss'].abs().clamp_min(1.)
    dz = (torch.sigmoid(z) - y) * s
    dzb = abs(s) * zb / 4                                               # what the logit's error does to dz
    r['de'] = dz[:, None] * w[None]
    r['de_bound'] = dzb[:, None] * w.abs()[None] + 8 * U * r['de'].abs()
    r['dw'] = (dz[:, None] * e).sum(0)
    r['dw_bound'] = sum_bound((dz[:, None] * e).abs().sum(0), M)
    r['db'] = dz.sum().reshape(1)
    r['db_bound'] = sum_bound(dz.abs().sum(), M).reshape(1)
    return r


def bce_buffers(c, device='cpu'):
    """logits (M + 1), loss_rows (M + 1), de (M, ld), pw (P, D), pb (P,), all NaN"""
    M, D, P = c['M'], c['D'], ln_bwd_parts(c['M'])
    f = lambda *s: torch.full(s, NAN, dtype=torch.float32, device=device)
    return f(M + 1), f(M + 1), f(M, c['ld']), f(P, D), f(P)


def bce_check(c, logits, loss_rows, de, pw, pb, dw, db):
    """the buffers of bce_buffers after the call, plus the column sums dw (D,) / db (1,) of the partials.  Returns the largest err / bound per output"""
    M, D = c['M'], c['D']
    r = bce_ref(c)
    out = dict(logits=assert_within(logits[:M], r['z'], r['zb'], 'bce_head logits'),
               loss=assert_within(loss_rows[:M], r['loss'], r['loss_bound'], 'bce_head loss_rows'),
               de=assert_within(de[:, :D], r['de'], r['de_bound'], 'bce_head de'))
    assert_untouched(logits[M:], 'bce_head logits beyond M')
    assert_untouched(loss_rows[M:], 'bce_head loss_rows beyond M')
    assert_untouched(de[:, D:], 'bce_head de columns >= D')
    assert_written(pw, 'bce_head dw partials')
    assert_written(pb, 'bce_head db partials')
    P = ln_bwd_parts(M)
    rpb = (M + P - 1) // P
    idle = torch.arange(P) * rpb >= M                                   # trailing blocks that own no row: their partials are zero, not garbage
    assert_same_bits(pw[idle], torch.zeros_like(pw[idle]), 'bce_head dw partials of the blocks without rows')
    assert_same_bits(pb[idle], torch.zeros_like(pb[idle]), 'bce_head db partials of the blocks without rows')
    assert_within(pw.double().sum(0), r['dw'], r['dw_bound'], 'bce_head sum of the dw partials')
    out['dw'] = assert_within(dw, r['dw'], r['dw_bound'], 'bce_head dw')
    out['db'] = assert_within(db, r['db'], r['db_bound'], 'bce_head db')
    return out


def bce_fake(c):
    """what a correct kernel and column sum would leave behind"""
    M, D, P = c['M'], c['D'], ln_bwd_parts(c['M'])
    r = bce_ref(c)
    logits, loss_rows, de, pw, pb = bce_buffers(c)
    logits[:M], loss_rows[:M], de[:, :D] = r['z'].float(), r['loss'].float(), r['de'].float()
    rpb = (M + P - 1) // P
    dz = (r['de'][:, :1] / c['w'].double()[0]).reshape(M)
    blk = torch.arange(M) // rpb
    pw.zero_().index_add_(0, blk, (dz[:, None] * c['e'][:, :D].double()).float())
    pb.zero_().index_add_(0, blk, dz.float())
    return logits, loss_rows, de, pw, pb, r['dw'].float(), r['db'].float()


# ------------------------------------------------------------------------------------------------ pk_attn_train_prep / pk_attn_train_prep_bwd

PREP_SHAPES = [(1, 2, 5, 5, 0), (2, 2, 37, 13, 2), (3, 1, 1, 1, 1), (4, 8, 300, 300, 0)]       # (S, heads, n, n_kv, nnull)
PREP_EPS = 1e-12


def prep_case(S, h, n, n_kv, nnull, seed=0):
    """q (S n, 64 h), kv (S n_kv, 128 h) = k | v, null_kv (h, 2 nnull, 64) = (k, v) pairs; the first q row and the last k row of the last head are zero"""
    g = gen(4, S, h, n, n_kv, nnull, seed)
    inner, nkt = 64 * h, nnull + n_kv
    r = lambda *s: torch.randn(*s, generator=g)
    c = dict(S=S, h=h, n=n, n_kv=n_kv, nnull=nnull, q=r(S * n, inner), kv=r(S * n_kv, 2 * inner), null_kv=r(h, 2 * nnull, 64) if nnull else None,
             q_scale=1 + 0.1 * r(64), k_scale=1 + 0.1 * r(64), scale=8.0, dQh=r(S * h, n, 64), dKh=r(S * h, nkt, 64), dVh=r(S * h, nkt, 64))
    c['q'][0, :64] = 0.
    c['kv'][-1, inner - 64:inner] = 0.
    return c


def _heads(x, S, rows, h):
    """(S rows, 64 h) -> (S, h, rows, 64)"""
    return x.reshape(S, rows, h, 64).permute(0, 2, 1, 3)


def _rows(x4):
    S, h, rows, _ = x4.shape
    return x4.permute(0, 2, 1, 3).reshape(S * rows, h * 64)


def prep_operands(c, q=None, kv=None, null_kv=None):
    """(q, k, v) per head in float64: (S, h, n, 64), (S, h, nkt, 64) x 2, the null keys in front"""
    S, h, n, n_kv, nnull = c['S'], c['h'], c['n'], c['n_kv'], c['nnull']
    q = c['q'].double() if q is None else q
    kv = c['kv'].double() if kv is None else kv
    q4, k4, v4 = _heads(q, S, n, h), _heads(kv[:, :64 * h], S, n_kv, h), _heads(kv[:, 64 * h:], S, n_kv, h)
    if nnull:
        nk = (c['null_kv'].double() if null_kv is None else null_kv).reshape(h, nnull, 2, 64)
        k4 = torch.cat([nk[None, :, :, 0].expand(S, -1, -1, -1), k4], 2)
        v4 = torch.cat([nk[None, :, :, 1].expand(S, -1, -1, -1), v4], 2)
    return q4, k4, v4


def prep_forward(q4, k4, v4, q_scale, k_scale, scale):
    """the operation itself, as the model states it: Qh = l2norm(q) q_scale scale, Kh = l2norm(k) k_scale, Vh = v"""
    return F.normalize(q4, dim=-1, eps=PREP_EPS) * q_scale * scale, F.normalize(k4, dim=-1, eps=PREP_EPS) * k_scale, v4


def _l2norm_bwd(x, dn):
    """y = x / max(|x|, eps): dx = (dn - y <dn, y>) / |x| (a zero row: dn / eps), and the sum of the absolute terms of every element"""
    inv = 1.0 / x.norm(dim=-1, keepdim=True).clamp_min(PREP_EPS)
    y = x * inv
    dx = (dn - y * (dn * y).sum(-1, keepdim=True)) * inv
    terms = (dn.abs() + y.abs() * (dn * y).abs().sum(-1, keepdim=True)) * inv
    return y, dx, terms


def prep_ref(c):
    """forward and backward in closed form with the bounds: sum_bound over the 64-term norm and dot for the rows, over the row count for dq_scale / dk_scale
    (S heads n, S heads (nnull + n_kv) terms), over the S sequences for dnull"""
    S, h, n, n_kv, nnull = c['S'], c['h'], c['n'], c['n_kv'], c['nnull']
    q4, k4, v4 = prep_operands(c)
    qs, ks, sc = c['q_scale'].double(), c['k_scale'].double(), c['scale']
    Qh, Kh, Vh = prep_forward(q4, k4, v4, qs, ks, sc)
    r = dict(Qh=Qh.reshape(S * h, n, 64), Kh=Kh.reshape(S * h, -1, 64), Vh=Vh.reshape(S * h, -1, 64))
    r['Qh_bound'], r['Kh_bound'] = sum_bound(r['Qh'].abs(), 64), sum_bound(r['Kh'].abs(), 64)
    dQ, dK, dV = (c[k].double().reshape(S, h, -1, 64) for k in ('dQh', 'dKh', 'dVh'))
    xn, dq4, tq = _l2norm_bwd(q4, dQ * qs * sc)
    kn, dk4, tk = _l2norm_bwd(k4, dK * ks)
    r['dq'], r['dq_bound'] = _rows(dq4), sum_bound(_rows(tq), 64)
    r['dk'], r['dk_bound'] = _rows(dk4[:, :, nnull:]), sum_bound(_rows(tk[:, :, nnull:]), 64)
    r['dv'] = _rows(dV[:, :, nnull:])
    r['dq_scale'], r['dq_scale_bound'] = (dQ * xn * sc).sum((0, 1, 2)), sum_bound((dQ * xn * sc).abs().sum((0, 1, 2)), S * h * n)
    r['dk_scale'], r['dk_scale_bound'] = (dK * kn).sum((0, 1, 2)), sum_bound((dK * kn).abs().sum((0, 1, 2)), S * h * (nnull + n_kv))
    if nnull:
        nk = c['null_kv'].double().reshape(h, nnull, 2, 64)[:, :, 0]
        _, dnk, _ = _l2norm_bwd(nk, dK[:, :, :nnull].sum(0) * ks)
        _, _, tnk = _l2norm_bwd(nk, dK[:, :, :nnull].abs().sum(0) * ks.abs())
        dnv = dV[:, :, :nnull].sum(0)
        r['dnull'] = torch.stack([dnk, dnv], 2).reshape(h, 2 * nnull, 64)
        r['dnull_bound'] = torch.stack([sum_bound(tnk, S), sum_bound(dV[:, :, :nnull].abs().sum(0), S)], 2).reshape(h, 2 * nnull, 64)
    return r


def prep_check_fwd(c, Qh, Kh, Vh):
    r = prep_ref(c)
    out = dict(Qh=assert_within(Qh, r['Qh'], r['Qh_bound'], 'attn_train_prep Qh'), Kh=assert_within(Kh, r['Kh'], r['Kh_bound'], 'attn_train_prep Kh'))
    assert_same_bits(Vh, r['Vh'].float(), 'attn_train_prep Vh (a copy)')
    return out


def prep_check_bwd(c, dq, dkv, dq_scale, dk_scale, dnull, pq=None, pk=None):
    """dq (S n, >= 64 h), dkv (S n_kv, >= 128 h) pre-filled with NaN; pq / pk: the (1024, 64) partials where the caller holds them"""
    inner = 64 * c['h']
    r = prep_ref(c)
    out = dict(dq=assert_within(dq[:, :inner], r['dq'], r['dq_bound'], 'attn_train_prep_bwd dq'),
               dk=assert_within(dkv[:, :inner], r['dk'], r['dk_bound'], 'attn_train_prep_bwd dk'))
    assert_same_bits(dkv[:, inner:2 * inner], r['dv'].float(), 'attn_train_prep_bwd dv (a copy)')
    assert_untouched(dq[:, inner:], 'attn_train_prep_bwd dq columns beyond the heads')
    assert_untouched(dkv[:, 2 * inner:], 'attn_train_prep_bwd dkv columns beyond the heads')
    for p, name in ((pq, 'dq_scale'), (pk, 'dk_scale')):
        if p is not None:
            assert_written(p, f'attn_train_prep_bwd {name} partials')
    out['dq_scale'] = assert_within(dq_scale, r['dq_scale'], r['dq_scale_bound'], 'attn_train_prep_bwd dq_scale')
    out['dk_scale'] = assert_within(dk_scale, r['dk_scale'], r['dk_scale_bound'], 'attn_train_prep_bwd dk_scale')
    if c['nnull']:
        out['dnull'] = assert_within(dnull, r['dnull'], r['dnull_bound'], 'attn_train_prep_bwd dnull')
    return out


# ------------------------------------------------------------------------------------------------ pk_sqdiff_partials

SQDIFF_SHAPES = [(2, 3, 5, 8, 12), (1, 3, 6, 256, 256)]
SQDIFF_MASKS = ['none', 'all', 'empty', 'prefix', 'hole']
SQDIFF_BLOCKS = 1024


def frame_mask_of(kind, B, Fr):
    if kind == 'none':
        return None
    m = torch.ones(B, Fr, dtype=torch.uint8)
    if kind == 'empty':
        m.zero_()
    elif kind == 'prefix':
        for i in range(B):
            m[i, (i * 2) % Fr + 1:] = 0
    elif kind == 'hole':
        m[:, 1] = 0
        m[0, Fr - 2] = 0
    return m


def sqdiff_case(shape, mask_kind, seed=0):
    g = gen(5, *shape, seed)
    return dict(shape=shape, kind=mask_kind, a=torch.randn(*shape, generator=g), b=torch.randn(*shape, generator=g), mask=frame_mask_of(mask_kind, shape[0], shape[2]))


def sqdiff_ref(c):
    d = (c['a'].double() - c['b'].double()) ** 2
    if c['mask'] is not None:
        d = d * c['mask'].double()[:, None, :, None, None]
    return d.sum()


def sqdiff_check(c, partials):
    """partials (1024,) f64, pre-filled with NaN: every block writes its own, the idle ones a zero.  8 U: the difference, its square and the three adds of
    a 4-group are rounded in f32 (all terms are positive), the rest is added in double"""
    assert partials.dtype == torch.float64 and partials.shape == (SQDIFF_BLOCKS,)
    assert_written(partials, 'sqdiff partials')
    B, C, Fr, H, W = c['shape']
    total4 = B * C * Fr * H * W // 4
    idle = torch.arange(SQDIFF_BLOCKS) * 256 >= total4
    assert_same_bits(partials[idle], torch.zeros_like(partials[idle]), 'sqdiff partials of the idle blocks')
    if c['kind'] == 'empty':
        assert_same_bits(partials, torch.zeros_like(partials), 'sqdiff partials with no frame kept')
    ref = sqdiff_ref(c)
    return assert_within(partials.sum(), ref, 8 * U * ref, f'sqdiff sum ({c["kind"]})')


# ------------------------------------------------------------------------------------------------ pk_patch_frame_mask

FRAME_GEOMS = {'image': (0, 1, 1, 5), 'video': (1, 2, 2, 5), 'pt3': (1, 2, 3, 7)}          # name -> (f0, nt, pt, F)
FRAME_PATCHES = [(1, 4), (4, 4), (8, 16)]


def patchify(video, f0, nt, pt, ph, pw):
    """(B, C, F, H, W) -> (B nt nh nw, C pt ph pw): row (b, t, hh, ww), column (c, dt, y, x)"""
    B, C, _, H, W = video.shape
    nh, nw = H // ph, W // pw
    v = video[:, :, f0:f0 + nt * pt].reshape(B, C, nt, pt, nh, ph, nw, pw)
    return v.permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B * nt * nh * nw, C * pt * ph * pw)


def frame_mask_case(geom, ph, pw, seed=0):
    """B = 3, H != W.  Sample 0 keeps every frame, sample 1 keeps frames 0 and 1 only (frame 2t + 1 kept, 2t + 2 dropped: a temporal patch is split),
    sample 2 drops frames 0, 2 and 5.  The source holds NaN in every dropped frame"""
    f0, nt, pt, Fr = FRAME_GEOMS[geom]
    B, C, H, W = 3, 3, 2 * ph, 3 * pw
    video = torch.randn(B, C, Fr, H, W, generator=gen(6, f0, pt, ph, pw, seed))
    mask = torch.ones(B, Fr, dtype=torch.uint8)
    mask[1, 2:] = 0
    mask[2, [0, 2] + ([5] if Fr > 5 else [])] = 0
    keep = mask.bool()[:, None, :, None, None]
    want = patchify(torch.where(keep, video.double(), torch.zeros((), dtype=torch.float64)), f0, nt, pt, ph, pw).float()
    src = patchify(torch.where(keep, video, torch.full((), NAN)), f0, nt, pt, ph, pw).contiguous()
    return dict(geom=(f0, nt, pt, ph, pw), video_shape=(B, C, Fr, H, W), mask=mask, src=src, want=want, P=C * pt * ph * pw)


def frame_mask_check(c, dst):
    """dst (rows, >= P), pre-filled with NaN (in place: the source buffer)"""
    P = c['P']
    assert_same_bits(dst[:, :P], c['want'], 'patch_frame_mask')
    assert_untouched(dst[:, P:], 'patch_frame_mask columns >= P')


# ------------------------------------------------------------------------------------------------ the elementwise four

ELEMENTWISE_N = [4, 1028]


def scaled_diff_ref(a, b, scale, dev):
    """(the f32 expression the kernel is held to bit for bit, the float64 value, three roundings: the difference, scale * dev, their product)"""
    s32 = torch.tensor(scale, dtype=torch.float32)
    if dev is not None:
        s32 = s32 * torch.tensor(dev, dtype=torch.float32)
    ref = (a.double() - b.double()) * (scale * (dev if dev is not None else 1.0))
    return (a - b) * s32, ref, ((1 + U) ** 3 - 1) * ref.abs()


def sign_inputs(n, seed=0):
    """+0, -0, the smallest and largest denormals of both signs, the smallest normals, infinities and NaN among random values"""
    z = torch.randn(n, generator=gen(7, n, seed))
    special = torch.tensor([0., -0., 1e-45, -1e-45, 1.1754942e-38, -1.1754942e-38, 1.17549435e-38, -1.17549435e-38, float('inf'), -float('inf'), NAN])
    k = min(n, special.numel())
    z[:k] = special[:k]
    return z


def sign_ref(z, value):
    v = torch.tensor(value, dtype=torch.float32)
    return torch.where(z > 0, v, -v)


def leaky_from_output(y, dy, slope):
    """dz = dy * (y > 0 ? 1 : slope): the derivative of LeakyReLU read off its OUTPUT (an exact zero takes the slope branch)"""
    return dy * torch.where(y > 0, torch.ones((), dtype=dy.dtype), torch.tensor(slope, dtype=dy.dtype))


def leaky_case(M, N, seed=0):
    """y with exact zeros, negative zeros, negatives and positives"""
    g = gen(8, M, N, seed)
    y, dy = torch.randn(M, N, generator=g), torch.randn(M, N, generator=g)
    y[torch.rand(M, N, generator=g) < 0.25] = 0.
    y.view(-1)[::5] *= -1
    return y, dy


def strided(t, pad, device='cpu', fill=NAN):
    """(a view of t's shape inside a buffer whose rows are `pad` longer and filled with `fill`, that buffer)"""
    buf = torch.full((t.shape[0], t.shape[1] + pad), fill, dtype=t.dtype, device=device)
    buf[:, :t.shape[1]] = t
    return buf[:, :t.shape[1]], buf


# ------------------------------------------------------------------------------------------------ pk_bias_gather / pk_bias_scatter

BIAS_DIMS = [(2, 3, 3), (1, 4, 5), (3, 1, 1)]
BIAS_HEADS = [1, 2, 8]


def rel_code(dims):
    """the mixed-radix position code (n,) int32 of a grid, its offset and the number of relative positions Lt:
    0 <= code[i] - code[j] + off < Lt, one table row per relative position"""
    strides, acc = [], 1
    for d in reversed(dims):
        strides.insert(0, acc)
        acc *= 2 * d - 1
    grids = torch.meshgrid(*[torch.arange(d) for d in dims], indexing='ij')
    code = sum(g.reshape(-1) * st for g, st in zip(grids, strides))
    off = sum((d - 1) * st for d, st in zip(dims, strides))
    return code.int(), int(off), acc


def bias_case(dims, heads, seed=0):
    code, off, Lt = rel_code(dims)
    g = gen(9, *dims, heads, seed)
    n = code.numel()
    return dict(code=code, off=off, Lt=Lt, n=n, heads=heads, tab=torch.randn(Lt, heads, generator=g), G=torch.randn(heads, n, n, generator=g))


def bias_rel(c):
    code = c['code'].long()
    return code[:, None] - code[None, :] + c['off']


def bias_gather_ref(c, tab=None):
    """bias[h][i][j] = tab[code[i] - code[j] + off][h]"""
    tab = c['tab'] if tab is None else tab
    return tab[:, :c['heads']][bias_rel(c)].permute(2, 0, 1).contiguous()


def bias_scatter_ref(c, G=None):
    """(dtab (Lt, heads) float64 = the adjoint of the gather, its bound: sum_bound over the largest multiplicity of a table row)"""
    G = c['G'].double() if G is None else G
    rel = bias_rel(c).reshape(-1)
    rows = G.permute(1, 2, 0).reshape(-1, c['heads'])
    z = torch.zeros(c['Lt'], c['heads'], dtype=torch.float64)
    mult = int(torch.bincount(rel, minlength=c['Lt']).max())
    return z.clone().index_add_(0, rel, rows), sum_bound(z.clone().index_add_(0, rel, rows.abs()), mult, extra=0)


def bias_check(c, out, dtab):
    """out (heads, n, n) pre-filled with NaN; dtab (Lt, >= heads): zeros in the first `heads` columns, NaN beyond, before the scatter.
    Returns the scatter's largest err / bound and the adjointness defect over its bound"""
    heads = c['heads']
    assert_same_bits(out, bias_gather_ref(c), 'bias_gather')
    ref, bound = bias_scatter_ref(c)
    ratio = assert_within(dtab[:, :heads], ref, bound, 'bias_scatter')
    assert_untouched(dtab[:, heads:], 'bias_scatter columns >= heads')
    lhs = (out.double() * c['G'].double()).sum()
    rhs = (c['tab'].double() * dtab[:, :heads].double()).sum()
    adj = assert_within(lhs, rhs, (c['tab'].double().abs() * bound).sum(), 'bias gather / scatter adjointness')
    return dict(scatter=ratio, adjoint=adj)


# ------------------------------------------------------------------------------------------------ pk_reduce_multi

REDUCE_E4 = [1, 255, 256, 257]
REDUCE_COLS = [(1, 4), (9, 68), (8192, 4), (9, 512), (1, 68), (8192, 68), (9, 4), (1, 512)]          # (M, N): every M of {1, 9, 8192}, every N of {4, 68, 512}
REDUCE_COUNTS = [(1, 1), (8, 8), (3, 5)]


def reduce_case(nsum, ncol, seed=0):
    """sum jobs (part (S, E + 4) rows E used, S): out[e] = sum_s part[s][e]; column jobs (src (M, N + 4) rows N used): out[c] = sum_r src[r][c]"""
    g = gen(10, nsum, ncol, seed)
    sums = []
    for i in range(nsum):
        E, S = 4 * REDUCE_E4[(i + nsum) % 4], (1, 3, 5)[i % 3]
        sums.append(torch.randn(S, E + 4, generator=g))
    cols = []
    for i in range(ncol):
        M, N = REDUCE_COLS[(i + ncol) % len(REDUCE_COLS)]
        cols.append(torch.randn(M, N + 4, generator=g))
    return dict(sums=sums, cols=cols)


def reduce_check(c, sum_outs, col_outs):
    """outputs (E + 4,) / (N + 4,) pre-filled with NaN; the tail of each stays NaN"""
    worst = 0.
    for i, (p, o) in enumerate(zip(c['sums'], sum_outs)):
        E, S = p.shape[1] - 4, p.shape[0]
        worst = max(worst, assert_within(o[:E], p[:, :E].double().sum(0), sum_bound(p[:, :E].double().abs().sum(0), S, extra=0), f'reduce_multi sum job {i}'))
        assert_untouched(o[E:], f'reduce_multi sum job {i} beyond E')
    for i, (s, o) in enumerate(zip(c['cols'], col_outs)):
        N, M = s.shape[1] - 4, s.shape[0]
        worst = max(worst, assert_within(o[:N], s[:, :N].double().sum(0), sum_bound(s[:, :N].double().abs().sum(0), M, extra=0), f'reduce_multi column job {i}'))
        assert_untouched(o[N:], f'reduce_multi column job {i} beyond N')
    return worst


def reduce_fake(c):
    souts, couts = [], []
    for p in c['sums']:
        o = torch.full((p.shape[1],), NAN)
        o[:-4] = p[:, :-4].double().sum(0).float()
        souts.append(o)
    for s in c['cols']:
        o = torch.full((s.shape[1],), NAN)
        o[:-4] = s[:, :-4].double().sum(0).float()
        couts.append(o)
    return souts, couts
