"""Cache policy of the result stores / read-once loads (pk_set_cache_policy, csrc/common.hpp): only cache bits of the instructions
change, so every touched entry point must give bit-identical outputs under mask 0, under write-through stores + non-temporal loads,
and under non-temporal stores + loads.  Shapes: the smallest that reach every store form (16 / 8 / 4-byte pieces, C2, GEGLU pairs,
row statistics, scatter, duplicated rows) and every ragged edge (M = 130 = 2 tiles + 2 rows, N = 72 / 136 off the tile).  Needs a
real MI355X (-m gpu)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SENTINEL = -7.0          # finite fill of the outputs (rows a kernel must not touch compare equal too)


@pytest.fixture(scope='module')
def L():
    from phenaki_pytorch_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), 'these tests need the HIP device (no CPU fallback exists)'
    return _lib


def g(seed):
    return torch.Generator().manual_seed(seed)


def masks(L):
    stores, loads = L.CP_STORE_SITES, L.CP_LOAD_SITES
    wt = L.cache_policy_mask(**{s: L.CP_WT for s in stores}, **{s: L.CP_NT for s in loads})
    nt = L.cache_policy_mask(**{s: L.CP_NT for s in stores + loads})
    return 0, wt, nt


def same_under_every_policy(L, fn):
    """fn() launches on fresh outputs and returns them; run it under the three masks and compare every tensor bit for bit"""
    saved = L.get_cache_policy()
    runs = []
    try:
        for mask in masks(L):
            L.set_cache_policy(mask)
            assert L.get_cache_policy() == mask
            runs.append([t.clone() for t in fn()])
        torch.cuda.synchronize()
    finally:
        L.set_cache_policy(saved)
    assert L.get_cache_policy() == saved
    base = runs[0]
    assert any((t.float() != SENTINEL).any() for t in base), 'the kernel wrote nothing'
    for name, run in zip(('write-through', 'non-temporal'), runs[1:]):
        assert len(run) == len(base)
        for i, (a, b) in enumerate(zip(base, run)):
            assert torch.equal(a, b), f'output {i} differs under the {name} policy'


def full(shape, dtype=torch.float32):
    return torch.full(shape, SENTINEL, device='cuda', dtype=dtype)


def test_mask_layout(L):
    m0, wt, nt = masks(L)
    assert m0 == 0 and wt == 0b10_10_10_01_01_01_01_01_01 and nt == 0b10_10_10_10_10_10_10_10_10
    saved = L.get_cache_policy()
    for bad in (3, 1 << 12, 1 << 18):                   # policy 3, a write-through LOAD, a site that does not exist
        with pytest.raises(RuntimeError, match='PK_EINVAL'):
            L.set_cache_policy(bad)
        assert L.get_cache_policy() == saved


def _gemm_operands(L, dt, M, N, K, seed):
    from phenaki_pytorch_amd import attention as A
    td = L.tdtype(dt)
    x = (torch.randn(M, K, generator=g(seed)) * 1.2 + 0.1).cuda().to(td)
    W = (torch.randn(N, K, generator=g(seed + 1)) / math.sqrt(K)).cuda()
    return x, A.pack_linear_weight(W, dt)


def test_gemm_plain_f32_out(L):
    M, N, K = 130, 72, 136
    x, w = _gemm_operands(L, L.BF16, M, N, K, 10)

    def fn():
        C = full((M, N))
        L.gemm(L.BF16, x, w, M, N, K, C=C, variant=8)
        return [C]
    same_under_every_policy(L, fn)


def test_gemm_residual_copy_and_row_stats(L):
    M, N, K = 130, 128, 512
    x, w = _gemm_operands(L, L.BF16, M, N, K, 20)
    res = torch.randn(M, N, generator=g(22)).cuda()
    bias = torch.randn(N, generator=g(23)).cuda()

    def fn():
        C, C2, st = full((M, N)), full((M, N), torch.bfloat16), full((M, N // 32, 2))
        L.gemm(L.BF16, x, w, M, N, K, C=C, bias=bias, res=res, C2=C2, stats_out=st, variant=8)
        return [C, C2, st]
    same_under_every_policy(L, fn)


def test_gemm_geglu_bf16_out(L):
    M, N, K = 130, 136, 64
    x, w = _gemm_operands(L, L.BF16, M, N, K, 30)

    def fn():
        C = full((M, N // 2), torch.bfloat16)
        L.gemm(L.BF16, x, w, M, N, K, C=C, act=L.ACT_GEGLU)
        return [C]
    same_under_every_policy(L, fn)


def test_gemm_layernorm_fold_with_handed_over_stats(L):
    from torch import nn
    from phenaki_pytorch_amd import attention as A
    M, N, K = 130, 256, 512
    dt = L.BF16
    # the producer of the rows and of their statistics (plain policy: it only prepares the inputs)
    o, wo = _gemm_operands(L, dt, M, K, 64, 40)
    xt, st = full((M, K), torch.bfloat16), full((M, K // 32, 2))
    saved = L.get_cache_policy()
    L.set_cache_policy(0)
    try:
        L.gemm(dt, o, wo, M, K, 64, C=full((M, K)), C2=xt, stats_out=st, variant=8)
    finally:
        L.set_cache_policy(saved)
    gamma, beta = (1 + 0.2 * torch.randn(K, generator=g(42))).cuda(), (0.1 * torch.randn(K, generator=g(43))).cuda()
    Wd = (torch.randn(N, K, generator=g(44)) / math.sqrt(K)).cuda()
    wg, s, t, _ = A.folded_weight(nn.Linear(1, 1), 'k', lambda: Wd, gamma, beta, dt, [gamma])
    res = torch.randn(M, N, generator=g(45)).cuda()

    def fn():
        C, Cr = full((M, N), torch.bfloat16), full((M, N))
        L.gemm(dt, xt, wg, M, N, K, C=C, ln=(s, t, 1e-5), ln_stats=st, variant=24)
        L.gemm(dt, xt, wg, M, N, K, C=Cr, res=res, ln=(s, t, 1e-5), ln_stats=st, variant=24)     # the folded form's own residual load
        return [C, Cr]
    same_under_every_policy(L, fn)


def test_gemm_scatter_decode_geometry(L):
    from phenaki_pytorch_amd.cvivit import CViViT
    B, T, pt, hw, p, C, D = 1, 2, 2, 8, 8, 3, 64            # 3 frames of 64 x 64 = first frame + one temporal patch of 2
    net = CViViT(dim=D, codebook_size=16, image_size=hw * p, patch_size=p, temporal_patch_size=pt, spatial_depth=1, temporal_depth=1,
                 dim_head=64, heads=1, channels=C)
    x = torch.randn(B * T * hw * hw, D, generator=g(50)).cuda().to(torch.bfloat16)
    calls = []
    for f0, ntg, ptg, row0 in ((0, 1, 1, 0), (1, T - 1, pt, hw * hw)):
        P = C * ptg * p * p
        W = (torch.randn(P, D, generator=g(51 + ptg)) / math.sqrt(D)).cuda().to(torch.bfloat16)
        bias = torch.randn(P, generator=g(53)).cuda()
        calls.append((P, W, bias) + tuple(net._unpatch_maps(B, T, f0, ntg, ptg, row0, torch.device('cuda'))))

    def fn():
        video = full((B, C, 1 + (T - 1) * pt, hw * p, hw * p))
        for P, W, bias, idx, row_off, col_off in calls:
            L.gemm(L.BF16, x, W, idx.numel(), P, D, C=video, bias=bias, a_rows=idx, scatter=(row_off, col_off))
        return [video]
    same_under_every_policy(L, fn)


def test_gemm_dup_rows(L):
    M, N, K, gap = 130, 72, 136, 5
    x, w = _gemm_operands(L, L.BF16, M, N, K, 60)
    res = torch.randn(M, N, generator=g(62)).cuda()

    def fn():
        C, C2 = full((2 * M + gap, N)), full((2 * M + gap, N), torch.bfloat16)
        L.gemm(L.BF16, x, w, M, N, K, C=C, res=res, C2=C2, dup_rows=M + gap)
        return [C, C2]
    same_under_every_policy(L, fn)


def test_gemm_split_bf16(L):
    M, N, K = 130, 72, 136
    x, w = _gemm_operands(L, L.BF16X3, M, N, K, 70)
    res = torch.randn(M, N, generator=g(72)).cuda()

    def fn():
        C = full((M, N))
        L.gemm(L.BF16X3, x, w, M, N, K, C=C, res=res)
        return [C]
    same_under_every_policy(L, fn)


@pytest.mark.parametrize('S,n', [(3, 64), (15, 9)])
def test_qkv_attn(L, S, n):
    h, K = 2, 64
    M = S * n
    x = (torch.randn(M, K, generator=g(80 + n)) * 1.5 + 0.2).cuda()
    xq, xkv = x.to(torch.bfloat16), (x * 0.9).to(torch.bfloat16)
    wq = (torch.randn(h * 64, K, generator=g(81)) / math.sqrt(K)).cuda().to(torch.bfloat16)
    wkv = (torch.randn(2 * h * 64, K, generator=g(82)) / math.sqrt(K)).cuda().to(torch.bfloat16)
    qs, ks = (1 + 0.1 * torch.randn(64, generator=g(83))).cuda(), (1 + 0.1 * torch.randn(64, generator=g(84))).cuda()
    bias = torch.randn(h, n, n, generator=g(85)).cuda()

    def fn():
        O = full((M, h * 64), torch.bfloat16)
        L.qkv_attn(xq, xkv, wq, wkv, S, n, h, K, qs, ks, 8.0, O, bias=bias)
        return [O]
    same_under_every_policy(L, fn)


@pytest.mark.parametrize('with_copy', [False, True])
def test_peg(L, with_copy):
    B, T, H, W, D = 1, 3, 2, 8, 64
    x = torch.randn(B * T * H * W, D, generator=g(90)).cuda()
    wt, bias = (torch.randn(27, D, generator=g(91)) * 0.1).cuda(), (torch.randn(D, generator=g(92)) * 0.1).cuda()

    def fn():
        out = full(tuple(x.shape))
        out_t = full(tuple(x.shape), torch.bfloat16) if with_copy else None
        L.peg(x, wt, bias, out, B, T, H, W, D, True, out_t=out_t)
        return [out] + ([out_t] if with_copy else [])
    same_under_every_policy(L, fn)


@pytest.mark.parametrize('out_dtype', [torch.bfloat16, torch.float32])
def test_layernorm_perm_all_outputs(L, out_dtype):
    M, D, pb, pc = 70, 64, 5, 7
    x = (torch.randn(M, D, generator=g(100)) * 2 + 0.3).cuda()
    gamma, beta = (1 + 0.1 * torch.randn(D, generator=g(101))).cuda(), (0.1 * torch.randn(D, generator=g(102))).cuda()

    def fn():
        out, out2, raw = full((M, D), out_dtype), full((M, D)), full((M, D), out_dtype)
        L.layernorm(x, gamma, beta, M, D, out=out, out2=out2, raw=raw, perm=(pb, pc))
        return [out, out2, raw]
    same_under_every_policy(L, fn)


def test_layernorm_lfq(L):
    M, D, cd = 70, 64, 8
    x = (torch.randn(M, D, generator=g(110)) * 2 + 0.3).cuda()
    gamma, beta = (1 + 0.1 * torch.randn(D, generator=g(111))).cuda(), (0.1 * torch.randn(D, generator=g(112))).cuda()
    wp, bp = (torch.randn(cd, D, generator=g(113)) / math.sqrt(D)).cuda(), (torch.randn(cd, generator=g(114)) * 0.05).cuda()

    def fn():
        ids = torch.full((M,), -1, device='cuda', dtype=torch.int64)
        tok, proj = full((M, D)), full((M, cd))
        L.layernorm_lfq(x, gamma, beta, wp, bp, ids, M, D, cd, tokens=tok, proj=proj, perm=(5, 7))
        return [ids, tok, proj]
    same_under_every_policy(L, fn)


def test_patch_embed_splitk_and_finish(L):
    B, C, Fr, H, W, pt, ph, pw, N = 1, 3, 5, 64, 64, 2, 32, 32, 64
    nh, nw = H // ph, W // pw
    hw, nt = nh * nw, (Fr - 1) // pt
    T = 1 + nt
    video = torch.randn(B, C, Fr, H, W, generator=g(120)).cuda()
    groups = []
    for f0, ntg, ptg, seed, goff in ((1, nt, pt, 1, hw), (0, 1, 1, 2, 0)):
        P = C * ptg * ph * pw
        wg = (torch.randn(N, P, generator=g(121 + seed)) / math.sqrt(P)).to(torch.bfloat16).cuda()
        s, t = wg.float().sum(1), (0.1 * torch.randn(N, generator=g(123 + seed))).cuda()
        g2, b2 = (1 + 0.1 * torch.randn(N, generator=g(125 + seed))).cuda(), (0.1 * torch.randn(N, generator=g(127 + seed))).cuda()
        groups.append((wg, P, B * ntg * hw, f0, ntg, ptg, s, t, g2, b2, (ntg * hw, T * hw, goff)))

    def fn():
        outs, spec, fin = [], [], []
        for wg, P, rows, f0, ntg, ptg, s, t, g2, b2, remap in groups:
            part, stats = full((L.patch_embed_slices(P), rows, N)), full((L.patch_embed_slices(P), rows, 2))
            spec.append((wg, part, stats, f0, ntg, ptg))
            fin.append((part, stats, P, s, t, 1e-5, g2, b2, 1e-5, remap))
            outs += [part, stats]
        tokens, tokens_t = full((B * T * hw, N)), full((B * T * hw, N), torch.bfloat16)
        L.patch_embed_splitk(video, ph, pw, N, spec)
        L.patch_embed_finish_groups(fin, out2=tokens, out=tokens_t)
        return outs + [tokens, tokens_t]
    same_under_every_policy(L, fn)
