"""Float64 twin, case table and checker of the patch embedding (csrc/patch_embed.hip): pk_patch_embed, pk_patch_embed_splitk, pk_patch_embed_finish and
pk_patch_embed_finish_groups.  Plain tensor code, no kernel launched; tests/test_patch_embed_parity_host.py shows what the checker rejects and
tests/test_patch_embed_parity_gpu.py holds the kernels to it.

The twin rounds where the kernels round.  Patch rows are (b, tt, hh, ww), features (c, dt, y, x), a frame group is (f0, nt, pt).  Every row is centred on
the mean of its first 32 features, computed in f32 IN THE KERNEL'S ORDER (four consecutive elements as (a+b)+(c+d), the eight pieces by the xor butterfly
1, 2, 4, times 1/32), so x' = f32(x - c) is bit-equal to the kernel's value; the operand is RNE-bf16(x'), the row statistics use the unrounded x'.

Two data sets.  `grid`: integer pixels, integer centres, W on a 1/16 grid -- every partial product and statistic is exact in f32 in any order, so `part` and
`stats` must EQUAL the float64 value and adding the integer 64 to the whole video must leave every byte alone.  `rand`: Gaussian video with patches scaled
by 1e3 / 1e-3 and one patch of variance ~4 eps1; second pass offset 40, contrast 0.05.  Each rand element is held to a first-order bound (u = 2^-23, one
ulp per f32 operation):
  accumulate   (K_acc / 32 + 32) u S_mn, S_mn = sum_k |bf16 x'||w|: v_mfma_f32_16x16x32_bf16 consumes 32 features per accumulator update -- one ulp per
               update of the running f32 value plus 32 for the sums inside one update (their rounding is not documented)
  statistics   n u sum|x'| for the sum, (n + 1) u sum x'^2 for the squares, n = terms of the slice (any order of n - 1 adds; the fma adds one)
  epilogue     the f32 slice sums ((ns - 1) u sum|.|), 1/K and the products of mean' (2 u), the cancellation in sq/K - mean'^2 (every operand's error
               and one ulp of each operand), sqrt and the reciprocal (4 u: v_rsq_f32 is 1 ulp, 1/sqrtf at most 1 + 2.5), one ulp per operation of
               rstd (acc - mean' s) + t; LayerNorm(dim): 8 + 6 adds deep lane and wave sums (14 u sum|.|), the same propagation through
               (y - m2) r2 gamma2 + beta2
The bf16 copy must be the RNE of some f32 inside the f32 bound; where the f32 row is written too it must be its RNE bit for bit.
Every operand is the head of a longer poisoned array (NaN in the first pass, +Inf in the second), every output sits in a sentinel-filled buffer with guard
rows and slack columns that the checker compares as integers."""
import math
import zlib
from types import SimpleNamespace as NS

import torch

U1 = 2.0 ** -23
PW_KS = 1024
EPS1 = EPS2 = 1e-5
SENT32, SENT16 = -7777.25, -7808.0          # finite and bf16-exact (the second): a store that never happened fails the bound, not the NaN screen
POISONS = (float('nan'), float('inf'))
GUARD = 4                                   # guard rows in front of and behind every output
PK_EINVAL, PK_EALIGN = -1, -2
CP_WT, CP_NT = 1, 2


def bf(x):
    assert x.dtype == torch.float32
    return x.to(torch.bfloat16).float()


def _bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


# ------------------------------------------------------------------------------------------------ gather, centre

def gather(video, f0, nt, pt, ph, pw):
    B, C, F, H, W = video.shape
    nh, nw = H // ph, W // pw
    fr = video[:, :, f0:f0 + nt * pt]
    return fr.reshape(B, C, nt, pt, nh, ph, nw, pw).permute(0, 2, 4, 6, 1, 3, 5, 7).reshape(B * nt * nh * nw, C * pt * ph * pw)


def scatter(video, pat, f0, nt, pt, ph, pw):
    """the inverse of gather: write the patch matrix into frames [f0, f0 + nt pt) of the video"""
    B, C, F, H, W = video.shape
    nh, nw = H // ph, W // pw
    video[:, :, f0:f0 + nt * pt] = pat.reshape(B, nt, nh, nw, C, pt, ph, pw).permute(0, 4, 1, 5, 2, 6, 3, 7).reshape(B, C, nt * pt, H, W)


def centre(pat, first=0):
    """f32, the kernel's order: lane p of a row's octet holds features 4p .. 4p + 3"""
    f = pat[:, first:first + 32].reshape(-1, 8, 4)
    v = (f[..., 0] + f[..., 1]) + (f[..., 2] + f[..., 3])
    lane = torch.arange(8)
    for off in (1, 2, 4):
        v = v + v[:, lane ^ off]
    assert bool((v == v[:, :1]).all())              # the butterfly is commutative: every lane holds the same value
    return v[:, 0] * torch.tensor(1.0 / 32.0)


# ------------------------------------------------------------------------------------------------ cases

def _groups(c, groups):
    B, C, F, H, W, pt, ph, pw, N = c.geo
    nh, nw = H // ph, W // pw
    hw = nh * nw
    if groups is None:                               # the module's split: frames 1.. in temporal patches (long K first), then the first frame
        nt = (F - 1) // pt
        T = 1 + nt
        spec = ([(1, nt, pt, (nt * hw, T * hw, hw))] if nt > 0 else []) + [(0, 1, 1, (hw, T * hw, 0) if nt > 0 else (0, 0, 0))]
        R = B * T * hw
    else:
        (f0, nt, ptg), = groups
        spec = [(f0, nt, ptg, (0, 0, 0))]
        R = B * nt * hw
    out = []
    for f0, nt, ptg, remap in spec:
        K, rows = C * ptg * ph * pw, B * nt * hw
        out.append(NS(f0=f0, nt=nt, pt=ptg, K=K, rows=rows, ns=-(-K // PW_KS), mtiles=-(-rows // 128), remap=remap))
    return out, R


def _case(name, kernel, geo, data, groups=None, pol='plain/plain', caught=None):
    c = NS(name=f'{name}/{data}' + ('' if pol == 'plain/plain' else '/' + pol.replace('/', '+')), kernel=kernel, geo=geo, data=data, pol=pol, caught=caught)
    c.N = geo[8]
    c.groups, c.R = _groups(c, groups)
    return c


# (B, C, F, H, W, pt, ph, pw, N)
_FUSED = [
    ('f_k192_c1_ph24', (2, 1, 1, 48, 16, 1, 24, 8, 72), None),             # K = 192: the prologue already wraps; C = 1, ph not a power of two, 64-col tile
    ('f_pw16_g2', (2, 3, 5, 32, 32, 2, 16, 16, 132), None),                # K = 1536 / 768, two groups, N off the 128-col tile
    ('f_ph1_pw64', (3, 3, 1, 6, 128, 1, 1, 64, 64), None),                 # ph = 1, one k-tile = one line, N on the 64-col tile
    ('f_pw128_g2', (1, 3, 3, 4, 256, 2, 2, 128, 128), None),               # one line = two k-tiles, N on the 128-col tile
    ('f_pt3_pw32', (2, 1, 7, 8, 64, 3, 2, 32, 260), ((1, 2, 3),)),         # pt = 3 alone, C = 1, three column tiles with a ragged last one
    ('f_rows320', (5, 3, 1, 64, 64, 1, 8, 8, 256), None),                  # rows ragged over three m-tiles
    ('f_rows576_g2', (9, 3, 3, 64, 64, 2, 8, 8, 72), None),                # 5 + 5 m-tiles: more than 8, no multiple of 8
    ('f_model_k', (1, 3, 3, 64, 64, 2, 32, 32, 132), None),                # K = 6144 / 3072
]
_SPLITK = [
    ('s_k64', (2, 1, 1, 16, 16, 1, 8, 8, 4), None),                        # one k-tile: the iteration round only issues and waits
    ('s_k1024', (1, 1, 1, 64, 64, 1, 32, 32, 260), None),                  # one full slice, 16 k-tiles (no multiple of 3)
    ('s_k1088', (1, 17, 1, 16, 16, 1, 8, 8, 512), None),                   # two slices, the second a single k-tile
    ('s_k1536_g2', (2, 3, 5, 32, 32, 2, 16, 16, 260), None),               # K = 1536 / 768, both groups
    ('s_model_k', (1, 3, 3, 64, 64, 2, 32, 32, 512), None),                # 6 + 3 slices: a work list of 9
    ('s_rows576_g2', (9, 3, 3, 64, 64, 2, 8, 8, 512), None),               # 5 + 5 row panels
    ('s_ph1_pw64', (2, 2, 1, 3, 128, 1, 1, 64, 8), None),
    ('s_pw128_pt3', (1, 1, 4, 2, 256, 3, 1, 128, 12), None),               # pt = 3 and pt = 1, one line = two k-tiles
    ('s_ph24_pw8', (1, 1, 1, 48, 16, 1, 24, 8, 4), None),
]
_POLICY_BASE = ('s_k1536_g2', 's_k1088')
POLICIES = {'plain/plain': {}, 'nt/plain': dict(ld_video=CP_NT), 'plain/wt': dict(patch_wide=CP_WT), 'nt/wt': dict(ld_video=CP_NT, patch_wide=CP_WT)}


def gemm_cases():
    out = []
    for data in ('grid', 'rand'):
        out += [_case(n, 'fused', geo, data, gr) for n, geo, gr in _FUSED]
        out += [_case(n, 'splitk', geo, data, gr) for n, geo, gr in _SPLITK]
        out += [_case(n, 'splitk', geo, data, gr, pol) for n, geo, gr in _SPLITK if n in _POLICY_BASE for pol in POLICIES if pol != 'plain/plain']
    return out


def branch_of(c):
    if c.kernel == 'fused':                          # pk_patch_embed: `wide = N >= 128` picks the build
        return 'fused/n128' if c.N >= 128 else 'fused/n64'
    if c.kernel == 'splitk':                         # pk_patch_embed_splitk: CPS_LD_VIDEO picks the build, CPS_PATCH_WIDE the emit() instantiation
        return 'splitk/' + c.pol
    return 'finish/' + ('pair' if len(c.g) == 2 else 'single')


def expected_branches():
    """written out from the dispatch code of csrc/patch_embed.hip"""
    return {'fused/n64', 'fused/n128', 'splitk/plain/plain', 'splitk/nt/plain', 'splitk/plain/wt', 'splitk/nt/wt', 'finish/single', 'finish/pair'}


def props_of(c):
    B, C, F, H, W, pt, ph, pw, N = c.geo
    p = {f'N{N}', f'pw{pw}', f'g{len(c.groups)}'} | {f'pt{G.pt}' for G in c.groups}
    Ks = '/'.join(str(G.K) for G in c.groups)
    p.add('K' + Ks)
    if ph == 1:
        p.add('ph1')
    if ph & (ph - 1):
        p.add('ph_not_pow2')
    if C == 1:
        p.add('C1')
    if c.kernel == 'fused':
        p.add('tile128' if N >= 128 else 'tile64')
        MT = sum(G.mtiles for G in c.groups)
        if all(G.rows < 128 for G in c.groups):
            p.add('rows<128')
        if any(G.rows > 256 and G.rows % 128 for G in c.groups):
            p.add('rows_ragged_tiles')
        p.add('mtiles<8' if MT < 8 else ('mtiles>8_not8' if MT % 8 else 'mtiles%8'))
    else:
        work = sum(G.mtiles * G.ns for G in c.groups)
        p.add('work<8' if work < 8 else ('work>8_not8' if work % 8 else 'work%8'))
        p.add('pol:' + c.pol)
    return p


REQUIRED_PROPS = {
    'fused': {'tile64', 'tile128', 'N72', 'N132', 'N260', 'N64', 'N128', 'N256', 'pw8', 'pw16', 'pw32', 'pw64', 'pw128', 'ph1', 'ph_not_pow2', 'pt1', 'pt2', 'pt3',
              'C1', 'K192', 'K6144/3072', 'g1', 'g2', 'rows<128', 'rows_ragged_tiles', 'mtiles<8', 'mtiles>8_not8'},
    'splitk': {'K64', 'K1024', 'K1088', 'K1536/768', 'K6144/3072', 'N4', 'N260', 'N512', 'pw8', 'pw16', 'pw32', 'pw64', 'pw128', 'ph1', 'ph_not_pow2', 'pt1', 'pt2',
               'pt3', 'C1', 'g1', 'g2', 'work<8', 'work>8_not8', 'pol:plain/plain', 'pol:nt/plain', 'pol:plain/wt', 'pol:nt/wt'},
}


# ------------------------------------------------------------------------------------------------ data

def _gen(name):
    return torch.Generator().manual_seed(zlib.crc32(name.encode()))


def _poisoned(head, extra_shape, poison):
    """`head` as the leading block of a larger array of shape head.shape + extra (per dim), the rest holding the poison"""
    full = torch.full([a + b for a, b in zip(head.shape, extra_shape)], poison, dtype=head.dtype)
    full[tuple(slice(0, a) for a in head.shape)] = head
    return full


def build(c):
    """x.video[p]: the two passes (B, C, F, H, W) f32; per group x.Wg (N, K) bf16, x.s, x.t, x.g2, x.b2 (N,) f32; x.flat / x.tail: the special grid rows"""
    B, C, F, H, W, pt, ph, pw, N = c.geo
    g = _gen(c.name.split('/')[0] + c.data)
    x = NS(Wg=[], s=[], s_unrounded=[], t=[], g2=[], b2=[], flat=[], tail=[])
    vid = torch.zeros(B, C, F, H, W)
    for G in c.groups:
        K, rows = G.K, G.rows
        if c.data == 'grid':
            pat = torch.randint(-4, 5, (rows, K), generator=g).float()
            flat, tail = (1 if rows > 1 else 0), (rows - 1 if rows > 2 else None)
            pat[flat] = 3.0                                              # x' = 0: part and stats exactly 0, the token row LayerNorm(t)
            if tail is not None:                                         # the only non-zero x' sits in the last k-tile
                pat[tail] = 0.0
                pat[tail, max(K - 64, 32):] = torch.randint(1, 5, (K - max(K - 64, 32),), generator=g).float()
            s31 = pat[:, :31].sum(1)
            pat[:, 31] = ((-s31 + 16) % 32) - 16                         # in [-16, 15]: the first 32 features sum to a multiple of 32
            wg = torch.randint(-16, 17, (N, K), generator=g).float() / 16
            t = torch.randint(-16, 17, (N,), generator=g).float() / 8
            x.flat.append(flat)
            x.tail.append(tail)
        else:
            pat = torch.randn(rows, K, generator=g)
            r = torch.arange(rows)
            pat[r % 8 == 1] *= 1e3
            pat[r % 8 == 5] *= 1e-3
            if rows > 2:
                pat[2] = torch.randn(K, generator=g) * math.sqrt(4 * EPS1) + 0.5
            gamma, beta = 1 + 0.1 * torch.randn(K, generator=g), 0.1 * torch.randn(K, generator=g)
            wl, bl = torch.randn(N, K, generator=g) / math.sqrt(K), 0.1 * torch.randn(N, generator=g)
            wg = wl * gamma[None, :]
            t = wl @ beta + bl
            x.flat.append(None)
            x.tail.append(None)
        scatter(vid, pat, G.f0, G.nt, G.pt, ph, pw)
        wgb = wg.to(torch.bfloat16)
        x.Wg.append(wgb)
        x.s.append(wgb.float().sum(1))                                   # the row sums of the ROUNDED operand
        x.s_unrounded.append(wg.sum(1))
        x.t.append(t)
        x.g2.append(1 + 0.1 * torch.randn(N, generator=g))
        x.b2.append(0.1 * torch.randn(N, generator=g))
    x.video = [vid, vid + 64.0] if c.data == 'grid' else [vid, vid * 0.05 + 40.0]
    if c.data == 'grid':
        grid_preconditions(c, x)
    return x


def grid_preconditions(c, x):
    """asserted, not assumed: integer centres, bf16-exact x', every sum below 2^24 steps of its grid.  Returns the largest figures."""
    B, C, F, H, W, pt, ph, pw, N = c.geo
    worst = NS(xp=0.0, steps=0.0, sq=0.0)
    for p, vid in enumerate(x.video):
        for gi, G in enumerate(c.groups):
            pat = gather(vid, G.f0, G.nt, G.pt, ph, pw)
            cen = centre(pat)
            assert bool((cen == cen.round()).all()), f'{c.name}: a centre is no integer'
            assert torch.equal(cen.double(), pat[:, :32].double().mean(1)), f'{c.name}: the f32 centre is not the exact mean'
            xp = pat - cen[:, None]
            assert torch.equal(bf(xp), xp), f'{c.name}: x\' is not bf16-exact'
            w = x.Wg[gi].double()
            assert torch.equal(w * 16, (w * 16).round()) and w.abs().max() <= 1
            steps = (xp.double().abs() @ w.abs().t()).max().item() * 16
            sq = (xp.double() ** 2).sum(1).max().item()
            assert steps < 2 ** 24 and sq < 2 ** 24, (c.name, steps, sq)
            worst = NS(xp=max(worst.xp, xp.abs().max().item()), steps=max(worst.steps, steps), sq=max(worst.sq, sq))
            assert bool((xp[x.flat[gi]] == 0).all())
            if x.tail[gi] is not None:
                nz = xp[x.tail[gi]].nonzero().flatten()
                assert nz.numel() > 0 and nz.min().item() >= G.K - 64
    return worst


# ------------------------------------------------------------------------------------------------ the float64 twin

def fold_reference(part, stats, K, s, t, eps1, d_part=None, d_stats=None):
    """y = rstd (sum_sl part - mean' s) + t from given part (ns, rows, N) / stats (ns, rows, 2), in float64, with its f32 bound; d_part / d_stats: the
    error the inputs already carry"""
    ns = part.shape[0]
    acc, su, sq = part.sum(0), stats[..., 0].sum(0), stats[..., 1].sum(0)
    d_acc = (ns - 1) * U1 * part.abs().sum(0) + (0 if d_part is None else d_part.sum(0))
    d_su = (ns - 1) * U1 * stats[..., 0].abs().sum(0) + (0 if d_stats is None else d_stats[..., 0].sum(0))
    d_sq = (ns - 1) * U1 * stats[..., 1].abs().sum(0) + (0 if d_stats is None else d_stats[..., 1].sum(0))
    mean, ex2 = su / K, sq / K
    d_mean = d_su / K + 2 * U1 * mean.abs()
    var = (ex2 - mean ** 2).clamp_min(0)
    d_var = d_sq / K + 2 * U1 * ex2.abs() + 2 * mean.abs() * d_mean + d_mean ** 2 + U1 * mean ** 2 + U1 * (ex2.abs() + mean ** 2) + U1 * (var + eps1)
    r = d_var / (var + eps1)
    assert r.max().item() < 0.5, f'the variance is lost in its own rounding ({r.max().item():.2f})'
    rstd = 1 / torch.sqrt(var + eps1)
    rel = 0.5 * r / (1 - r) + 4 * U1
    inner = acc - mean[:, None] * s[None, :]
    d_inner = d_acc + s.abs()[None, :] * d_mean[:, None] + U1 * (mean[:, None] * s[None, :]).abs() + U1 * inner.abs()
    y = rstd[:, None] * inner + t[None, :]
    dy = rstd[:, None] * d_inner + (rstd[:, None] * inner).abs() * (rel[:, None] + U1) + U1 * y.abs()
    return y, dy


def ln2_reference(y, dy, g2, b2, eps2):
    N = y.shape[1]
    m2 = y.mean(1, keepdim=True)
    d_m2 = (14 * U1 * y.abs().sum(1, keepdim=True) + dy.sum(1, keepdim=True)) / N + U1 * m2.abs()
    d = y - m2
    dd = dy + d_m2 + U1 * d.abs()
    v2 = (d * d).mean(1, keepdim=True)
    d_v2 = ((2 * d.abs() * dd + dd ** 2).sum(1, keepdim=True) + 15 * U1 * (d * d).sum(1, keepdim=True)) / N + 2 * U1 * (v2 + eps2)
    r = d_v2 / (v2 + eps2)
    assert r.max().item() < 0.5
    r2 = 1 / torch.sqrt(v2 + eps2)
    rel = 0.5 * r / (1 - r) + 4 * U1
    out = d * r2 * g2[None, :] + b2[None, :]
    d_out = g2.abs()[None, :] * r2 * (dd + d.abs() * (rel + 2 * U1)) + U1 * out.abs()
    return out, d_out


def finish_reference(part, stats, K, s, t, eps1, g2, b2, eps2, d_part=None, d_stats=None):
    y, dy = fold_reference(part, stats, K, s, t, eps1, d_part, d_stats)
    return ln2_reference(y, dy, g2, b2, eps2)


def remap_rows(rows, remap):
    r = torch.arange(rows)
    ri, ro, off = remap
    return (r // ri) * ro + off + r % ri if ri > 0 else r


def _patch_operands(c, x, p, gi):
    B, C, F, H, W, pt, ph, pw, N = c.geo
    G = c.groups[gi]
    xp = gather(x.video[p], G.f0, G.nt, G.pt, ph, pw)
    xp = xp - centre(xp)[:, None]
    return xp, x.Wg[gi].double()


def reference(c, x, p):
    """name -> NS(ref, bound, mapped): (R, cols) float64 arrays of every output of blank(c); bound = 0 where equality is required"""
    grid = c.data == 'grid'
    N, res = c.N, {}
    if c.kernel == 'splitk':
        tok = NS(ref=torch.zeros(c.R, N, dtype=torch.float64), bound=torch.zeros(c.R, N, dtype=torch.float64), mapped=torch.zeros(c.R, dtype=torch.bool))
    for gi, G in enumerate(c.groups):
        xp, w = _patch_operands(c, x, p, gi)
        xb, xd = bf(xp).double(), xp.double()
        s, t = x.s[gi].double(), x.t[gi].double()
        every = torch.ones(G.rows * (G.ns if c.kernel == 'splitk' else 1), dtype=torch.bool)
        if c.kernel == 'fused':
            acc, S = xb @ w.t(), xb.abs() @ w.abs().t()
            stats = torch.stack((xd.sum(1), (xd * xd).sum(1)), 1)
            d_part = torch.zeros_like(acc) if grid else (G.K / 32 + 32) * U1 * S
            d_stats = torch.zeros_like(stats) if grid else torch.stack((G.K * U1 * xd.abs().sum(1), (G.K + 1) * U1 * stats[:, 1]), 1)
            y, dy = fold_reference(acc[None], stats[None], G.K, s, t, EPS1, d_part[None], d_stats[None])
            res[f'out{gi}'] = NS(ref=y, bound=dy, mapped=every)
            continue
        parts, stats, d_parts, d_stats = [], [], [], []
        for sl in range(G.ns):
            k0, k1 = sl * PW_KS, min(G.K, (sl + 1) * PW_KS)
            a, ws, d = xb[:, k0:k1], w[:, k0:k1], xd[:, k0:k1]
            parts.append(a @ ws.t())
            stats.append(torch.stack((d.sum(1), (d * d).sum(1)), 1))
            n = k1 - k0
            d_parts.append(torch.zeros_like(parts[-1]) if grid else (n / 32 + 32) * U1 * (a.abs() @ ws.abs().t()))
            d_stats.append(torch.zeros_like(stats[-1]) if grid else torch.stack((n * U1 * d.abs().sum(1), (n + 1) * U1 * stats[-1][:, 1]), 1))
        parts, stats, d_parts, d_stats = (torch.stack(v) for v in (parts, stats, d_parts, d_stats))
        res[f'part{gi}'] = NS(ref=parts.reshape(-1, N), bound=d_parts.reshape(-1, N), mapped=every)
        res[f'stats{gi}'] = NS(ref=stats.reshape(-1, 2), bound=d_stats.reshape(-1, 2), mapped=every)
        out, d_out = finish_reference(parts, stats, G.K, s, t, EPS1, x.g2[gi].double(), x.b2[gi].double(), EPS2, d_parts, d_stats)
        o = remap_rows(G.rows, G.remap)
        tok.ref[o], tok.bound[o], tok.mapped[o] = out, d_out, True
    if c.kernel == 'splitk':
        res['tok'] = tok
        res['tok_t'] = tok
    return res


# ------------------------------------------------------------------------------------------------ buffers

def blank(c):
    """name -> NS(R, cols, ld, dtype): every output of the case, guard rows in front and behind, slack columns where the kernel takes a stride"""
    N = c.N
    if c.kernel == 'fused':
        return {f'out{gi}': NS(R=G.rows, cols=N, ld=N + 4, dtype=torch.float32) for gi, G in enumerate(c.groups)}
    b = {}
    if c.kernel == 'splitk':
        for gi, G in enumerate(c.groups):
            b[f'part{gi}'] = NS(R=G.ns * G.rows, cols=N, ld=N, dtype=torch.float32)          # dense by contract
            b[f'stats{gi}'] = NS(R=G.ns * G.rows, cols=2, ld=2, dtype=torch.float32)
    if c.kernel == 'splitk' or 'out2' in c.outs:
        b['tok'] = NS(R=c.R, cols=N, ld=N + 8, dtype=torch.float32)
    if c.kernel == 'splitk' or 'out' in c.outs:
        b['tok_t'] = NS(R=c.R, cols=N, ld=N + 4, dtype=torch.bfloat16)
    return b


def alloc(spec, device='cpu'):
    return torch.full((spec.R + 2 * GUARD, spec.ld), SENT16 if spec.dtype == torch.bfloat16 else SENT32, dtype=spec.dtype, device=device)


def window(full, spec):
    """the (R, ld) block the kernel is given (its first element is 16-byte aligned: GUARD ld elements in)"""
    return full[GUARD:GUARD + spec.R]


def f32_interval_to_bf16(ref, bound):
    """bf16 values (as float64) between which the RNE of any f32 inside [ref - bound, ref + bound] lies"""
    lo, hi = (ref - bound).float(), (ref + bound).float()
    lo = torch.where(lo.double() < ref - bound, torch.nextafter(lo, torch.full_like(lo, math.inf)), lo)
    hi = torch.where(hi.double() > ref + bound, torch.nextafter(hi, torch.full_like(hi, -math.inf)), hi)
    near = ref.float()
    empty = lo > hi                                                   # no f32 inside: the nearest f32 of the reference itself
    lo, hi = torch.where(empty, near, lo), torch.where(empty, near, hi)
    return bf(lo).double(), bf(hi).double()


def check(c, ref, out, what=None):
    """out: name -> full buffer (CPU).  Asserts guards, finiteness, equality / bound; returns name -> largest err / bound (0.0 where equality holds)"""
    what = what or c.name
    got = {}
    for name, spec in blank(c).items():
        full, r = out[name], ref[name]
        sent = torch.full((1,), SENT16 if spec.dtype == torch.bfloat16 else SENT32, dtype=spec.dtype)
        outside = torch.ones(full.shape, dtype=torch.bool)
        outside[GUARD:GUARD + spec.R, :spec.cols] = ~r.mapped[:, None]
        assert bool((_bits(full)[outside] == _bits(sent)).all()), f'{what}: {name}: a byte outside the result region lost its sentinel'
        v = window(full, spec)[:, :spec.cols][r.mapped].double()
        assert bool(torch.isfinite(v).all()), f'{what}: {name}: NaN or Inf inside the result region'
        want, bound = r.ref[r.mapped], r.bound[r.mapped]
        if spec.dtype == torch.bfloat16:
            lo, hi = f32_interval_to_bf16(want, bound)
            bad = (v < lo) | (v > hi)
            assert not bool(bad.any()), f'{what}: {name}: {int(bad.sum())} bf16 elements are the rounding of no f32 inside the bound'
            got[name] = 0.0
            if 'tok' in out and name == 'tok_t':
                f = window(out['tok'], blank(c)['tok'])[:, :spec.cols][r.mapped]
                assert torch.equal(_bits(f.to(torch.bfloat16)), _bits(window(full, spec)[:, :spec.cols][r.mapped])), f'{what}: the bf16 copy is not the RNE of the f32 row'
            continue
        err = (v - want).abs()
        exact = bound == 0
        assert bool((err[exact] == 0).all()), f'{what}: {name}: {int((err[exact] != 0).sum())} elements differ from the exact float64 value (max {err[exact].max().item():.3e})'
        ratio = (err[~exact] / bound[~exact]).max().item() if bool((~exact).any()) else 0.0
        assert ratio <= 1.0, f'{what}: {name}: error {ratio:.3f} x the bound'
        got[name] = ratio
    return got


def allowance_rms(ref):
    """name -> rms(bound) / rms(reference) over the mapped region"""
    return {name: (r.bound[r.mapped].pow(2).mean().sqrt() / r.ref[r.mapped].pow(2).mean().sqrt().clamp_min(1e-300)).item() for name, r in ref.items()}


# ------------------------------------------------------------------------------------------------ finish cases on synthetic partials

def _fcase(name, N, groups, outs, caught=None):
    """groups: (rows, ns, remap) x 1 or 2"""
    c = NS(name='fin_' + name, kernel='finish', N=N, outs=outs, data='synthetic', caught=caught)
    c.g = [NS(rows=rows, ns=ns, K=PW_KS * (ns - 1) + 64 * (1 + (rows + ns) % 16), remap=remap) for rows, ns, remap in groups]
    c.R = max(int(remap_rows(G.rows, G.remap).max()) + 1 for G in c.g)
    return c


def finish_cases():
    return [
        _fcase('n4_r1', 4, [(1, 1, (0, 0, 0))], ('out2',)),
        _fcase('n252_r3', 252, [(3, 2, (0, 0, 0))], ('out',)),
        _fcase('n256_r4', 256, [(4, 6, (2, 5, 1))], ('out', 'out2')),
        _fcase('n260_r5', 260, [(5, 2, (0, 0, 0))], ('out', 'out2')),
        _fcase('n512_r130', 512, [(130, 6, (13, 17, 2))], ('out2',)),
        _fcase('n260_r130_bf', 260, [(130, 1, (5, 5, 0))], ('out',)),
        _fcase('pair_6_10', 260, [(6, 2, (3, 8, 0)), (10, 1, (5, 8, 3))], ('out', 'out2')),       # rows0 % 4 = 2: the block that ends group 0 is half empty
        _fcase('pair_5_3', 512, [(5, 6, (5, 9, 0)), (3, 2, (3, 9, 6))], ('out2',)),
        _fcase('pair_130_1', 4, [(130, 1, (130, 131, 0)), (1, 1, (1, 131, 130))], ('out',)),
    ]


def build_finish(c):
    """per group: part (ns, rows, N), stats (ns, rows, 2) f32 and the vectors; row r % 5 == 0 has sq/K - mean'^2 slightly negative (the clamp),
    row r % 5 == 1 has the two terms agree to 1e-3"""
    g = _gen(c.name)
    x = NS(part=[], stats=[], s=[], s_unrounded=[], t=[], g2=[], b2=[])
    for G in c.g:
        rows, ns, K, N = G.rows, G.ns, G.K, c.N
        mean = 0.25 * torch.randn(rows, generator=g, dtype=torch.float64)
        var = torch.exp(torch.randn(rows, generator=g, dtype=torch.float64))
        r = torch.arange(rows)
        mean[r % 5 < 2] = 0.25
        var[r % 5 == 0] = -3e-7 * 0.0625
        var[r % 5 == 1] = 1e-3 * 0.0625
        wgt = torch.rand(ns, rows, generator=g, dtype=torch.float64) + 0.5
        wgt = wgt / wgt.sum(0, keepdim=True)
        stats = torch.stack((wgt * (K * mean), wgt * (K * (var + mean ** 2))), 2).float()
        scale = torch.sqrt((var.abs() + mean ** 2) / ns).float()             # x' (gamma.W)^T of a row has the size of the row's x'
        x.part.append(torch.randn(ns, rows, N, generator=g) * scale[None, :, None])
        x.stats.append(stats)
        w = torch.randn(N, K, generator=g) / math.sqrt(K)
        x.s.append(w.to(torch.bfloat16).float().sum(1))                  # the row sums of a rounded operand, as the product folds them
        x.s_unrounded.append(w.sum(1))
        x.t.append(0.1 * torch.randn(N, generator=g))
        x.g2.append(1 + 0.1 * torch.randn(N, generator=g))
        x.b2.append(0.1 * torch.randn(N, generator=g))
    return x


def reference_finish(c, x):
    tok = NS(ref=torch.zeros(c.R, c.N, dtype=torch.float64), bound=torch.zeros(c.R, c.N, dtype=torch.float64), mapped=torch.zeros(c.R, dtype=torch.bool))
    for gi, G in enumerate(c.g):
        out, d_out = finish_reference(x.part[gi].double(), x.stats[gi].double(), G.K, x.s[gi].double(), x.t[gi].double(), EPS1, x.g2[gi].double(),
                                      x.b2[gi].double(), EPS2)
        o = remap_rows(G.rows, G.remap)
        tok.ref[o], tok.bound[o], tok.mapped[o] = out, d_out, True
    return {'tok': tok, 'tok_t': tok}


# ------------------------------------------------------------------------------------------------ the f32 emulation and its planted defects

MUTANTS = ('stats_from_rounded', 'centre_from_32_63', 'no_centring', 'ktile_next_line', 'ktile_twice', 'slice_at_sentinel', 'slice_missing', 'rows_swapped',
           'row_one_past', 'bf16_truncated', 'mean_over_padded_k', 's_from_unrounded', 'guard_row_store', 'slack_column_store')


def applies(m, c, p=0):
    """the cases on which the defect changes a value beyond its bound, with the reason"""
    if c.kernel == 'finish':
        # s_from_unrounded: sum_k (w - bf16 w) ~ 2^-9 |w| sqrt(K) against a finish bound of a few ulps -- under the accumulate term of a whole case it
        # is about the size of the allowance, so the defect is planted where the partials are given
        return {'slice_missing': c.g[0].ns > 1, 'rows_swapped': c.g[0].rows > 2, 'row_one_past': True, 'bf16_truncated': 'out' in c.outs,
                'mean_over_padded_k': c.g[0].K % PW_KS != 0, 's_from_unrounded': c.g[0].rows > 1, 'guard_row_store': True, 'slack_column_store': True}.get(m, False)
    rand, K = c.data == 'rand', c.groups[0].K
    if m == 'stats_from_rounded':        # the squares move by ~2 x 0.29 x 2^-9 sqrt(3 / n) of their sum against an allowance of (n + 1) 2^-23 of it: 2^14 / n^1.5,
        return rand and min(G.K for G in c.groups) <= 192      # 32 x at n = 64, 6 x at 192 (the fused kernel's shortest row), below 1 from 768
    if m == 'centre_from_32_63':         # part and stats move with the centre; the fused output is invariant up to the operand's rounding, 0.29 sqrt(K)
        if c.kernel == 'splitk':         # 2^-9 against (K/32 + 32) K 2^-23: 30 x at K = 192, 5 x at 1536, 1 x at 6144; on the grid the centre moves by
            return True                  # k/32 and x' stays bf16-exact: the fused output is then rightly unchanged
        return rand and K <= 1536
    if m == 'no_centring':               # the offset-40 pass: bf16(x) keeps 8 bits of 40, the signal is 0.05
        return rand and p == 1
    if m in ('ktile_next_line', 'ktile_twice'):
        return K >= 128
    if m in ('slice_at_sentinel', 'slice_missing'):
        return c.kernel == 'splitk' and (m == 'slice_at_sentinel' or c.groups[0].ns > 1)
    if m == 'rows_swapped':
        return c.groups[0].rows > 3
    if m in ('row_one_past', 'bf16_truncated'):
        return c.kernel == 'splitk'
    if m == 'mean_over_padded_k':        # mean' is 0 on a flat row and small after centring: needs rand data and a ragged last slice
        return rand and c.kernel == 'splitk' and K % PW_KS != 0
    if m == 's_from_unrounded':
        return False
    return True


def _emu_stats(xp):
    """(rows, n) f32 -> f32 (sum, sum of squares) in the kernel's shape: lane p of the octet adds its 4 features of every 32 in turn (the squares by
    fma), then the xor butterfly"""
    rows, n = xp.shape
    f = xp.reshape(rows, n // 32, 8, 4)
    rs, rq = torch.zeros(rows, 8), torch.zeros(rows, 8)
    for i in range(n // 32):
        for e in range(4):
            v = f[:, i, :, e]
            rs = rs + v
            rq = (rq.double() + v.double() * v.double()).float()
    lane = torch.arange(8)
    for off in (1, 2, 4):
        rs, rq = rs + rs[:, lane ^ off], rq + rq[:, lane ^ off]
    return torch.stack((rs[:, 0], rq[:, 0]), 1)


def _emu_product(xb, w):
    """f32 running sum over exact 32-feature chunks"""
    acc = torch.zeros(xb.shape[0], w.shape[0])
    for k in range(0, xb.shape[1], 32):
        acc = (acc.double() + xb[:, k:k + 32].double() @ w[:, k:k + 32].double().t()).float()
    return acc


def _emu_fold(part, stats, K, s, t, eps1, mut=None):
    ns = part.shape[0]
    use = ns - 1 if mut == 'slice_missing' else ns
    acc, su, sq = part[0].clone(), stats[0, :, 0].clone(), stats[0, :, 1].clone()
    for sl in range(1, use):
        acc, su, sq = acc + part[sl], su + stats[sl, :, 0], sq + stats[sl, :, 1]
    inv_k = torch.tensor(1.0) / torch.tensor(float(-(-K // PW_KS) * PW_KS if mut == 'mean_over_padded_k' else K))
    mean = su * inv_k
    rstd = 1.0 / torch.sqrt((sq * inv_k - mean * mean).clamp_min(0) + torch.tensor(eps1))
    return rstd[:, None] * (acc - mean[:, None] * s[None, :]) + t[None, :]


def _emu_ln2(y, g2, b2, eps2):
    N = y.shape[1]
    m2 = y.sum(1, keepdim=True) / N
    d = y - m2
    r2 = 1.0 / torch.sqrt((d * d).sum(1, keepdim=True) / N + torch.tensor(eps2))
    return d * r2 * g2[None, :] + b2[None, :]


def _emu_place(c, out, rows, remap, v, mut):
    """the token rows into tok / tok_t; v (rows, N) f32"""
    o = remap_rows(rows, remap)
    if mut == 'row_one_past':
        o = o.clone()
        o[-1] += 1
    if mut == 'rows_swapped' and rows > 2:
        v = v.clone()
        v[[0, 2]] = v[[2, 0]]
    b = blank(c)
    if 'tok' in b:                                   # (through the whole buffer: a row one past the end lands in the guard)
        out['tok'][GUARD + o, :c.N] = v
    if 'tok_t' in b:
        vt = (v.contiguous().view(torch.int32) & -65536).view(torch.float32) if mut == 'bf16_truncated' else v
        out['tok_t'][GUARD + o, :c.N] = vt.to(torch.bfloat16)


def _emu_guards(c, out, mut):
    name = sorted(out)[0]
    if mut == 'guard_row_store':
        out[name][GUARD - 1, 0] = 1.0
    if mut == 'slack_column_store':
        spec = blank(c)[name]
        if spec.ld > spec.cols:
            out[name][GUARD, spec.cols] = 1.0
        else:
            out[name][GUARD + spec.R, 0] = 1.0


def emulate(c, x, p, mut=None):
    """the kernels' arithmetic in f32 on the CPU, into the buffers of blank(c); mut plants one defect"""
    B, C, F, H, W, pt, ph, pw, N = c.geo
    b = blank(c)
    out = {name: alloc(spec) for name, spec in b.items()}
    for gi, G in enumerate(c.groups):
        first = gi == 0
        pat = gather(x.video[p], G.f0, G.nt, G.pt, ph, pw)
        cen = centre(pat, 32 if mut == 'centre_from_32_63' else 0)
        xp = pat - (0 if mut == 'no_centring' else cen[:, None])
        K = G.K
        kt = (K // 64) - 1 if K // 64 < 3 else 1                       # the k-tile the defect hits (kt - 1 exists)
        if mut == 'ktile_next_line' and first and K >= 128:
            xp = xp.clone()
            xp[:, kt * 64:(kt + 1) * 64] = torch.roll(xp, -pw, 1)[:, kt * 64:(kt + 1) * 64]
        if mut == 'ktile_twice' and first and K >= 128:
            xp = xp.clone()
            xp[:, kt * 64:(kt + 1) * 64] = xp[:, (kt - 1) * 64:kt * 64]
        xb = bf(xp)
        w = x.Wg[gi].float()
        s = (x.s_unrounded[gi] if mut == 's_from_unrounded' else x.s[gi])
        src = xb if mut == 'stats_from_rounded' else xp
        if c.kernel == 'fused':
            y = _emu_fold(_emu_product(xb, w)[None], _emu_stats(src)[None], K, s, x.t[gi], EPS1)
            if mut == 'rows_swapped' and first and G.rows > 3:
                y[[0, 3]] = y[[3, 0]]
            window(out[f'out{gi}'], b[f'out{gi}'])[:, :N] = y
            continue
        part = torch.stack([_emu_product(xb[:, k:k + PW_KS], w[:, k:k + PW_KS]) for k in range(0, K, PW_KS)])
        stats = torch.stack([_emu_stats(src[:, k:k + PW_KS]) for k in range(0, K, PW_KS)])
        stored = part.clone()
        if mut == 'slice_at_sentinel' and first:
            stored[-1] = SENT32
        window(out[f'part{gi}'], b[f'part{gi}'])[:] = stored.reshape(-1, N)
        window(out[f'stats{gi}'], b[f'stats{gi}'])[:] = stats.reshape(-1, 2)
        v = _emu_ln2(_emu_fold(part, stats, K, s, x.t[gi], EPS1, mut if first else None), x.g2[gi], x.b2[gi], EPS2)
        _emu_place(c, out, G.rows, G.remap, v, mut if first else None)
    _emu_guards(c, out, mut)
    return out


def emulate_finish(c, x, mut=None):
    out = {name: alloc(spec) for name, spec in blank(c).items()}
    for gi, G in enumerate(c.g):
        m = mut if gi == 0 else None
        s = x.s_unrounded[gi] if m == 's_from_unrounded' else x.s[gi]
        v = _emu_ln2(_emu_fold(x.part[gi], x.stats[gi], G.K, s, x.t[gi], EPS1, m), x.g2[gi], x.b2[gi], EPS2)
        _emu_place(c, out, G.rows, G.remap, v, m)
    _emu_guards(c, out, mut)
    return out


# ------------------------------------------------------------------------------------------------ device operands and argument lists

def operands(c, x, p, device):
    """the poisoned operands and the sentinel-filled outputs of pass p on `device`.  t['video'] is a 16-byte aligned window 80 bytes into its allocation."""
    poison = POISONS[p]
    t = NS(out={name: alloc(spec, device) for name, spec in blank(c).items()})
    if c.kernel != 'finish':
        v = x.video[p]
        full = torch.full((20 + v.numel() + 4096,), poison)
        full[20:20 + v.numel()] = v.reshape(-1)
        t.video_full = full.to(device)
        t.video = t.video_full[20:20 + v.numel()].view(v.shape)
        t.W = [_poisoned(w, (8, 8), poison).to(device) for w in x.Wg]
    else:
        t.part = [a.to(device) for a in x.part]
        t.stats = [a.to(device) for a in x.stats]
    for k in ('s', 't', 'g2', 'b2'):
        setattr(t, k, [_poisoned(a, (8,), poison).to(device) for a in getattr(x, k)])
    return t


def _p(t):
    return None if t is None else t.data_ptr()


def fused_args(c, t):
    B, C, F, H, W, pt, ph, pw, N = c.geo
    b = blank(c)
    a = dict(video=_p(t.video), B=B, C=C, F=F, H=H, W=W, ph=ph, pw=pw, N=N, eps=EPS1, ngroups=len(c.groups))
    for gi in range(2):
        if gi < len(c.groups):
            G = c.groups[gi]
            a.update({f'W{gi}': _p(t.W[gi]), f'ldw{gi}': t.W[gi].stride(0), f's{gi}': _p(t.s[gi]), f't{gi}': _p(t.t[gi]),
                      f'out{gi}': _p(window(t.out[f'out{gi}'], b[f'out{gi}'])), f'f0{gi}': G.f0, f'nt{gi}': G.nt, f'pt{gi}': G.pt})
        else:
            a.update({f'W{gi}': None, f'ldw{gi}': 0, f's{gi}': None, f't{gi}': None, f'out{gi}': None, f'f0{gi}': 0, f'nt{gi}': 0, f'pt{gi}': 0})
    a['ldo'] = b['out0'].ld
    return a


def splitk_args(c, t):
    B, C, F, H, W, pt, ph, pw, N = c.geo
    b = blank(c)
    a = dict(video=_p(t.video), B=B, C=C, F=F, H=H, W=W, ph=ph, pw=pw, N=N, ngroups=len(c.groups))
    for gi in range(2):
        if gi < len(c.groups):
            G = c.groups[gi]
            a.update({f'W{gi}': _p(t.W[gi]), f'ldw{gi}': t.W[gi].stride(0), f'part{gi}': _p(window(t.out[f'part{gi}'], b[f'part{gi}'])),
                      f'stats{gi}': _p(window(t.out[f'stats{gi}'], b[f'stats{gi}'])), f'f0{gi}': G.f0, f'nt{gi}': G.nt, f'pt{gi}': G.pt})
        else:
            a.update({f'W{gi}': None, f'ldw{gi}': 0, f'part{gi}': None, f'stats{gi}': None, f'f0{gi}': 0, f'nt{gi}': 0, f'pt{gi}': 0})
    return a


def finish_args(c, t, gi, part, stats, G):
    """pk_patch_embed_finish of group gi; part / stats: device pointers of the dense (ns, rows, N) / (ns, rows, 2) arrays"""
    b = blank(c)
    o2, o = b.get('tok'), b.get('tok_t')
    return dict(part=part, stats=stats, nslices=G.ns, rows=G.rows, N=c.N, K=G.K, s=_p(t.s[gi]), t=_p(t.t[gi]), eps1=EPS1, gamma2=_p(t.g2[gi]), beta2=_p(t.b2[gi]),
                eps2=EPS2, out2=_p(window(t.out['tok'], o2)) if o2 else None, ldo2=o2.ld if o2 else 0, out=_p(window(t.out['tok_t'], o)) if o else None,
                ldo=o.ld if o else 0, remap_in=G.remap[0], remap_out=G.remap[1], remap_off=G.remap[2])


# refused calls: (label, entry, error, change(args)); every one returns before the launch and leaves the outputs at the sentinel
_FUSED_BASE = _case('refusal_base_fused', 'fused', (2, 3, 3, 32, 32, 2, 16, 16, 132), 'grid')
_SPLITK_BASE = _case('refusal_base_splitk', 'splitk', (2, 3, 3, 32, 32, 2, 16, 16, 132), 'grid')


def _set(**kw):
    return lambda a: a.update(kw)


def _bump(key, by):
    return lambda a: a.update({key: a[key] + by})


_BOTH = [
    ('pw_not_pow2', PK_EINVAL, _set(pw=12, W=24)), ('pw_below_8', PK_EINVAL, _set(pw=4)), ('pw_above_128', PK_EINVAL, _set(pw=256, W=256)),
    ('W_not_mult_4', PK_EINVAL, _set(W=30)), ('N_not_mult_4', PK_EINVAL, _set(N=130)), ('ph_splits_a_half', PK_EINVAL, _set(ph=1, pw=8)),
    ('frames_beyond_F', PK_EINVAL, _set(nt0=2)), ('ldw_below_K', PK_EINVAL, _set(ldw0=1528)), ('ldw_not_mult_8', PK_EINVAL, _bump('ldw0', 4)),
    ('video_misaligned', PK_EALIGN, _bump('video', 4)), ('W_misaligned', PK_EALIGN, _bump('W1', 8)),
]
REFUSALS = ([(f'fused/{n}', 'fused', e, ch) for n, e, ch in _BOTH] +
            [('fused/K_not_mult_192', 'fused', PK_EINVAL, _set(C=1)), ('fused/s_misaligned', 'fused', PK_EALIGN, _bump('s0', 4)),
             ('fused/out_misaligned', 'fused', PK_EALIGN, _bump('out1', 4)), ('fused/ldo_not_mult_4', 'fused', PK_EINVAL, _bump('ldo', 2))] +
            [(f'splitk/{n}', 'splitk', e, ch) for n, e, ch in _BOTH] +
            [('splitk/K_not_mult_64', 'splitk', PK_EINVAL, _set(C=1, ph=4, pw=8, nt0=1, pt0=1, ngroups=1)), ('splitk/N_above_512', 'splitk', PK_EINVAL, _set(N=516)),
             ('splitk/part_misaligned', 'splitk', PK_EALIGN, _bump('part0', 4)), ('splitk/stats_misaligned', 'splitk', PK_EALIGN, _bump('stats1', 4))])
FINISH_REFUSALS = [
    ('N_above_512', PK_EINVAL, _set(N=516)), ('N_not_mult_4', PK_EINVAL, _set(N=258)), ('no_output', PK_EINVAL, _set(out=None, out2=None)),
    ('remap_out_below_in', PK_EINVAL, _set(remap_in=4, remap_out=3)), ('negative_offset', PK_EINVAL, _set(remap_in=3, remap_out=8, remap_off=-1)),
    ('part_misaligned', PK_EALIGN, _bump('part', 4)), ('stats_misaligned', PK_EALIGN, _bump('stats', 4)), ('s_misaligned', PK_EALIGN, _bump('s', 4)),
    ('out2_misaligned', PK_EALIGN, _bump('out2', 4)), ('out_misaligned', PK_EALIGN, _bump('out', 2)), ('ldo2_not_mult_4', PK_EALIGN, _bump('ldo2', 2)),
]


def refusal_base(entry):
    return _FUSED_BASE if entry == 'fused' else _SPLITK_BASE


# ------------------------------------------------------------------------------------------------ the module's chain

def module_reference(video, groups, ph, pw, R):
    """Rearrange -> LayerNorm(P) -> Linear -> LayerNorm(dim) in float64 from the module's own parameters, the operands rounded where the kernels round them:
    x' (centred, bit-equal) to bf16 after the statistics, gamma (.) W (an f32 product) to bf16.  groups: (f0, nt, pt, remap, gamma, beta, eps1, W, b, gamma2,
    beta2, eps2), f32 CPU tensors.  The folded s and t of the product are f32 sums over K in an unknown order: (K - 1) 2^-24 sum|.| each, and one ulp for
    the bias add.  Returns NS(ref, bound, mapped) over the R token rows."""
    N = groups[0][7].shape[0]
    tok = NS(ref=torch.zeros(R, N, dtype=torch.float64), bound=torch.zeros(R, N, dtype=torch.float64), mapped=torch.zeros(R, dtype=torch.bool))
    for f0, nt, pt, remap, gamma, beta, eps1, W, b, g2, b2, eps2 in groups:
        pat = gather(video, f0, nt, pt, ph, pw)
        xp = pat - centre(pat)[:, None]
        xb, xd = bf(xp).double(), xp.double()
        K = xp.shape[1]
        wg = (W * gamma[None, :]).to(torch.bfloat16).double()
        mean, var = xd.mean(1, keepdim=True), xd.var(1, unbiased=False, keepdim=True)
        rstd = 1 / torch.sqrt(var + eps1)
        t = W.double() @ beta.double() + b.double()
        y = ((xb - mean) * rstd) @ wg.t() + t[None, :]
        # the same value as the kernels' fold computes it, for the bound: part / stats of one slice with the accumulate and statistics terms
        acc, S = xb @ wg.t(), xb.abs() @ wg.abs().t()
        stats = torch.stack((xd.sum(1), (xd * xd).sum(1)), 1)
        ns = -(-K // PW_KS)
        d_part = (K / 32 + 32 + ns - 1) * U1 * S                         # covers the fused kernel's K / 32 updates and the slices' 32 + 32 + their f32 sum
        d_stats = torch.stack((K * U1 * xd.abs().sum(1), (K + 1) * U1 * stats[:, 1]), 1)
        y2, dy = fold_reference(acc[None], stats[None], K, wg.sum(1), t, eps1, d_part[None], d_stats[None])
        d_s = (K - 1) * 2.0 ** -24 * wg.abs().sum(1)
        d_t = (K - 1) * 2.0 ** -24 * (W.double().abs() @ beta.double().abs()) + U1 * t.abs()
        dy = dy + (rstd * mean.abs()) * d_s[None, :] + d_t[None, :] + 1e-12 * y.abs().max()
        assert (y - y2).abs().max().item() <= 1e-9 * y.abs().max().item()      # LayerNorm-then-Linear and the fold are the same function of the rounded operands
        out, d_out = ln2_reference(y, dy, g2.double(), b2.double(), eps2)
        o = remap_rows(xp.shape[0], remap)
        tok.ref[o], tok.bound[o], tok.mapped[o] = out, d_out, True
    return tok
