"""Head widths 32 and 128 on the MI355X: pk_attn_prep_dh + pk_attn_fwd_dh against a torch f32 statement of the same math, the
Attention / Transformer modules against the CPU oracle (which splits heads by `heads`, so it is width-agnostic; test_dim_head_host.py
pins it to the reference at these widths), the kv-cache of cross-attention, and the tokenizer / MaskGit / sample() end to end.
Tolerances are those of test_kernels_gpu.py::test_attention_block (tests/util.close, norm-relative): fp32 1e-4, bf16x3 2e-4, bf16 3e-2.
Needs a real MI355X (-m gpu)."""
import pytest
import torch
import torch.nn.functional as F

from oracle import phenaki_oracle as O
from oracle import weights
from oracle.configs import TINY, oracle_cfgs
from tests.util import close, ids_equal_with_margin

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

WIDTHS = (32, 128)
TOL = {'fp32': 1e-4, 'bf16x3': 2e-4, 'bf16': 3e-2}
NEG_MAX = -torch.finfo(torch.float32).max


@pytest.fixture(scope='module', autouse=True)
def _oracle_follows_product_ln_fold():
    """the bf16 oracle rounds where the product rounds: LayerNorm folded into the consuming GEMM unless PK_LN_FOLD=0"""
    from phenaki_pytorch_amd import attention
    O.LN_FOLD, O.LN_FOLD_FF, O.LN_FOLD_FF_MAX_ROWS = attention._LN_FOLD, bool(attention._LN_FOLD_FF), attention._LN_FOLD_FF_MAX_ROWS
    O.ATTN_FIXED_OFFSET = attention._ATTN_FIXED
    O.ATTN_FIXED_OFFSET_BIAS = attention._ATTN_FIXED and attention._BIAS_TABLE


@pytest.fixture(scope='module')
def L():
    from phenaki_pytorch_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), 'these tests need the HIP device (no CPU fallback exists)'
    return _lib


def g(seed):
    return torch.Generator().manual_seed(seed)


def bf(x):
    return x.to(torch.bfloat16).float()


# ------------------------------------------------------------------------------------------ 5. kernel level

# name -> (S, h, nq, n_kv, nnull, extras)
KERNEL_CASES = {
    'full_bias': (3, 2, 64, 64, 0, ('bias',)),                         # vector-bias fast path
    'null_mask_tail': (2, 2, 37, 13, 2, ('bias', 'mask_row')),              # null keys, tail tile, scalar bias path; one sequence fully masked
    'causal_alibi': (5, 2, 9, 9, 0, ('causal',)),
    'bias_mask_200': (1, 2, 200, 200, 0, ('bias', 'mask')),            # QF = 2 where built, nq_pad rounded to 32, V^T tail mask at 200 % 32 != 0
    'plain_130': (1, 1, 130, 130, 0, ()),                              # several key tiles, no per-element path
}


def _inputs(case, dh):
    S, h, nq, n_kv, nnull, extras = KERNEL_CASES[case]
    q = torch.randn(S * nq, h * dh, generator=g(1))
    kv = torch.randn(S * n_kv, 2 * h * dh, generator=g(2))
    null_kv = torch.randn(h, 2 * nnull, dh, generator=g(3))
    qs = 1 + 0.1 * torch.randn(dh, generator=g(4))
    ks = 1 + 0.1 * torch.randn(dh, generator=g(5))
    bias = torch.randn(h, nq, n_kv, generator=g(6)) if 'bias' in extras else None
    kmask = None
    if 'mask' in extras:
        kmask = torch.rand(S, n_kv, generator=g(7)) > 0.3
    if 'mask_row' in extras:
        kmask = torch.rand(S, n_kv, generator=g(7)) > 0.3
        kmask[1, :] = False                                              # only the null keys remain
    slopes = torch.tensor([0.5, 0.25][:h]) if 'causal' in extras else None
    return dict(S=S, h=h, nq=nq, n_kv=n_kv, nnull=nnull, q=q, kv=kv, null_kv=null_kv, qs=qs, ks=ks, bias=bias, kmask=kmask, slopes=slopes)


def _reference(a, dh, rnd, scale=8.):
    """attention.py:146-182 on the projection outputs, f32 -> (O (S nq, h dh), lse (S h nq)); rnd rounds the operand images"""
    S, h, nq, n_kv, nnull = a['S'], a['h'], a['nq'], a['n_kv'], a['nnull']
    q = a['q'].view(S, nq, h, dh).permute(0, 2, 1, 3)
    k, v = a['kv'].view(S, n_kv, 2, h, dh).permute(2, 0, 3, 1, 4)
    if nnull:
        k = torch.cat((a['null_kv'][:, 0::2].expand(S, -1, -1, -1), k), dim=-2)
        v = torch.cat((a['null_kv'][:, 1::2].expand(S, -1, -1, -1), v), dim=-2)
    q = rnd(F.normalize(q, dim=-1) * a['qs'] * scale)
    k = rnd(F.normalize(k, dim=-1) * a['ks'])
    sim = q @ k.transpose(-1, -2)
    if a['bias'] is not None:
        sim = sim + F.pad(a['bias'], (nnull, 0), value=0.)
    if a['kmask'] is not None:
        sim = sim.masked_fill(~F.pad(a['kmask'], (nnull, 0), value=True)[:, None, None, :], NEG_MAX)
    if a['slopes'] is not None:
        i, j = torch.arange(nq)[:, None], torch.arange(nnull + n_kv)[None, :] - nnull
        dj = j - (i + n_kv - nq)
        sim = sim - dj.abs().float() * a['slopes'][None, :, None, None]
        sim = sim.masked_fill(dj > 0, NEG_MAX)
    out = sim.softmax(dim=-1) @ rnd(v)
    return out.permute(0, 2, 1, 3).reshape(S * nq, h * dh), torch.logsumexp(sim, dim=-1).reshape(-1)


def _run_kernels(L, a, dh, dt, lse=False, fwd=None, prep=None):
    S, h, nq, n_kv, nnull = a['S'], a['h'], a['nq'], a['n_kv'], a['nnull']
    td = L.tdtype(dt)
    nq_pad, nk_pad = L.attn_pads(nq, n_kv, nnull)
    Qp = torch.empty(S * h * nq_pad * dh, device='cuda', dtype=td)
    Kp = torch.empty(S * h * nk_pad * dh, device='cuda', dtype=td)
    Vt = torch.full((S * h * nk_pad * dh,), float('nan'), device='cuda', dtype=td)    # the V^T pad columns are never written: the tail mask has to hide them
    dev = {k: (v.cuda() if isinstance(v, torch.Tensor) else v) for k, v in a.items()}
    km = dev['kmask'].to(torch.uint8).contiguous() if dev['kmask'] is not None else None
    (prep or L.attn_prep)(dt, dev['q'], dev['kv'], dev['null_kv'], dev['qs'], dev['ks'], 8., Qp, Kp, Vt, S, h, nq, n_kv, nnull, dim_head=dh)
    o = torch.empty(S * nq, h * dh, device='cuda', dtype=td)
    lse_buf = torch.empty(S * h * nq, device='cuda') if lse else None
    (fwd or L.attn_fwd)(dt, Qp, Kp, Vt, o, S, h, nq, n_kv, nnull, bias=dev['bias'], kmask=km, slopes=dev['slopes'], causal=dev['slopes'] is not None,
                        lse=lse_buf, dim_head=dh)
    torch.cuda.synchronize()
    return o, lse_buf


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3', 'bf16'])
@pytest.mark.parametrize('case', list(KERNEL_CASES))
@pytest.mark.parametrize('dh', WIDTHS)
def test_prep_and_fwd_kernels(L, dh, case, dtype):
    dt = {'fp32': L.F32, 'bf16x3': L.BF16X3, 'bf16': L.BF16}[dtype]
    a = _inputs(case, dh)
    ref, ref_lse = _reference(a, dh, bf if dtype == 'bf16' else (lambda t: t))
    o, _ = _run_kernels(L, a, dh, dt)
    close(o, ref, TOL[dtype], f'attn_prep + attn_fwd dim_head {dh} {case} {dtype}')
    # the training forward's entry point shares the kernel: same output, and every row's log-sum-exp
    o2, lse = _run_kernels(L, a, dh, dt, lse=True)
    assert torch.equal(o2, o)
    close(lse, ref_lse, TOL[dtype], f'lse dim_head {dh} {case} {dtype}')


def test_width_64_through_the_dh_entry_points_is_bit_identical(L):
    """pk_attn_prep / pk_attn_fwd are the dim_head = 64 calls of pk_attn_prep_dh / pk_attn_fwd_dh"""
    lib = L.load()

    def old_prep(dt, q, kv, null_kv, qs, ks, scale, Qp, Kp, Vt, S, h, nq, n_kv, nnull, dim_head):
        assert lib.pk_attn_prep(dt, q.data_ptr(), q.stride(0), kv.data_ptr(), kv.stride(0), None, qs.data_ptr(), ks.data_ptr(), scale,
                                Qp.data_ptr(), Kp.data_ptr(), Vt.data_ptr(), S, h, nq, n_kv, nnull, L.stream(q)) == 0

    def old_fwd(dt, Qp, Kp, Vt, o, S, h, nq, n_kv, nnull, bias, kmask, slopes, causal, lse, dim_head):
        assert lib.pk_attn_fwd(dt, Qp.data_ptr(), Kp.data_ptr(), Vt.data_ptr(), bias.data_ptr(), bias.stride(0), bias.stride(1), None, None, 0,
                               o.data_ptr(), o.stride(0), 1 if o.dtype == torch.float32 else 0, S, h, nq, n_kv, nnull, None, 0, None, 0, 0,
                               float('nan'), L.stream(o)) == 0
    a = _inputs('full_bias', 64)
    for dt in (L.F32, L.BF16X3, L.BF16):
        new, _ = _run_kernels(L, a, 64, dt)
        old, _ = _run_kernels(L, a, 64, dt, fwd=old_fwd, prep=old_prep)
        assert torch.equal(new, old)
    # and the widths that do not exist are refused by both
    q = torch.zeros(64, 96, device='cuda')
    buf = torch.zeros(4096, device='cuda')
    with pytest.raises(RuntimeError, match='PK_EINVAL'):
        L.attn_prep(L.F32, q, None, None, buf[:48], buf[:48], 8., buf, None, None, 1, 2, 64, 64, 0, dim_head=48)
    with pytest.raises(RuntimeError, match='PK_EINVAL'):
        L.attn_fwd(L.F32, buf, buf, buf, q, 1, 2, 64, 64, 0, dim_head=48)
    with pytest.raises(RuntimeError, match='PK_EINVAL'):                  # the fixed-offset softmax lives in the 64-wide LDS-staged kernel
        L.attn_fwd(L.BF16, buf.bfloat16(), buf.bfloat16(), buf.bfloat16(), torch.zeros(16, 64, device='cuda', dtype=torch.bfloat16), 1, 2, 16, 16, 0,
                   score_bound=10., dim_head=32)


# ------------------------------------------------------------------------------------------ 6. module level

def _attn_module(dim, heads, dh, causal, nnull, dim_context=None):
    from phenaki_pytorch_amd.attention import Attention
    torch.manual_seed(11)
    m = Attention(dim=dim, dim_head=dh, heads=heads, causal=causal, num_null_kv=nnull, dim_context=dim_context)
    m.q_scale.copy_(1 + 0.1 * torch.randn(dh))
    m.k_scale.copy_(1 + 0.1 * torch.randn(dh))
    m.norm.gamma.copy_(1 + 0.1 * torch.randn(dim))
    if dim_context:
        m.context_norm.gamma.copy_(1 + 0.1 * torch.randn(dim_context))
    return m


_BLOCK_REF = {}


def _block_ref(case, dh, m, x, ctx, kw):
    """the f32 oracle output of a case: computed once per (case, width), shared by the three dtypes and the kv-cache test"""
    if (case, dh) not in _BLOCK_REF:
        sd = {('a.' + k): v for k, v in m.state_dict().items()}
        _BLOCK_REF[case, dh] = O.attention(sd, 'a.', x, heads=2, causal=m.causal, context=ctx, **kw)
    return _BLOCK_REF[case, dh]


def _block_case(case, dh):
    """(module, x, ctx, kw) of test_kernels_gpu.py::test_attention_block at head width dh"""
    dim, heads = 128, 2
    S, n = 3, 64
    ctx, kw = None, {}
    if case == 'spatial_bias':
        m = _attn_module(dim, heads, dh, False, 0)
        kw['attn_bias'] = torch.randn(heads, n, n, generator=g(31))
    elif case == 'causal_alibi':
        S, n = 7, 9
        m = _attn_module(dim, heads, dh, True, 0)
    elif case == 'cross_null_mask':
        m = _attn_module(dim, heads, dh, False, 2, dim_context=96)
        ctx = torch.randn(S, 13, 96, generator=g(32))
        mask = torch.ones(S, 13, dtype=torch.bool)
        mask[1, 5:] = False
        mask[2, :] = False
        kw['mask'] = mask
    else:
        S, n = 2, 200
        m = _attn_module(dim, heads, dh, False, 0)
        kw['mask'] = torch.rand(S, n, generator=g(33)) > 0.3
        kw['attn_bias'] = torch.randn(heads, n, n, generator=g(34))
    x = torch.randn(S, n, dim, generator=g(35))
    return m, x, ctx, kw


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3', 'bf16'])
@pytest.mark.parametrize('case', ['spatial_bias', 'causal_alibi', 'cross_null_mask', 'self_mask_long'])
@pytest.mark.parametrize('dh', WIDTHS)
def test_attention_block(L, dh, case, dtype):
    from phenaki_pytorch_amd.attention import set_compute_dtype
    m, x, ctx, kw = _block_case(case, dh)
    ref = _block_ref(case, dh, m, x, ctx, kw)
    m = set_compute_dtype(m.cuda(), dtype)
    out = m(x.cuda(), context=ctx.cuda() if ctx is not None else None, mask=kw['mask'].cuda() if 'mask' in kw else None,
            attn_bias=kw['attn_bias'].cuda() if 'attn_bias' in kw else None)
    close(out, ref, TOL[dtype], f'attention dim_head {dh} {case} {dtype}')


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3', 'bf16'])
def test_transformer_with_peg_cross_and_ff(L, dtype):
    from phenaki_pytorch_amd.attention import Transformer, set_compute_dtype
    dim, heads, depth = 128, 2, 2
    m = Transformer(dim=dim, depth=depth, heads=heads, dim_head=32, dim_context=96, peg=True, has_cross_attn=True)
    weights.fill_module(m, salt=9)
    sd = {('t.' + k): v.clone() for k, v in m.state_dict().items()}
    S, vs, n = 2, (3, 4, 4), 48
    x = torch.randn(S, n, dim, generator=g(36))
    ctx = torch.randn(S, 7, 96, generator=g(37))
    cmask = torch.ones(S, 7, dtype=torch.bool)
    cmask[1, 4:] = False
    ref = O.transformer(sd, 't.', x, depth=depth, heads=heads, peg_on=True, cross=True, video_shape=(S, *vs), context=ctx,
                        cross_attn_context_mask=cmask)
    m = set_compute_dtype(m.cuda(), dtype)
    out = m(x.cuda(), video_shape=(S, *vs), context=ctx.cuda(), cross_attn_context_mask=cmask.cuda())
    close(out, ref, TOL[dtype], f'transformer dim_head 32 {dtype}')


# ------------------------------------------------------------------------------------------ 7. kv-cache

@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3', 'bf16'])
def test_cross_attention_kv_cache(L, dtype):
    from phenaki_pytorch_amd.attention import compute_dtype_of, set_compute_dtype
    m, x, ctx, kw = _block_case('cross_null_mask', 128)
    ref = _block_ref('cross_null_mask', 128, m, x, ctx, kw) + x
    m = set_compute_dtype(m.cuda(), dtype)
    S, n, D = x.shape
    x2, ctx2 = x.cuda().reshape(S * n, D), ctx.cuda().reshape(S * 13, 96)
    km = kw['mask'].cuda().to(torch.uint8).contiguous()
    cache = {}
    outs = [m.run(x2, S, n, compute_dtype_of(m), context2d=ctx2, n_ctx=13, kmask=km, kv_cache=cache) for _ in range(2)]
    assert id(m) in cache and cache[id(m)][0].numel() == S * 2 * 32 * 128            # (Kp, Vt) images of nk_pad = 32 keys, 128 wide
    assert torch.equal(outs[0], outs[1])
    for o in outs:
        close(o.reshape(S, n, D), ref, TOL[dtype], f'cross-attention with a kv_cache, dim_head 128 {dtype}')


# ------------------------------------------------------------------------------------------ 8. end to end

def _product(kind, cfg, salt, dtype):
    import phenaki_pytorch_amd as P
    m = P.CViViT(use_vgg_and_gan=False, **cfg) if kind == 'cvivit' else getattr(P, kind)(**cfg)
    weights.fill_module(m, salt=salt)
    sd = {k: v.clone() for k, v in m.state_dict().items()}
    return P.set_compute_dtype(m.cuda().eval(), dtype), sd


@pytest.fixture(scope='module')
def tokenizer_reference():
    """the oracle's 32-wide tiny tokenizer on video seed 0, once.  Seed 0 was chosen on the CPU: the f32 oracle against an f64 run of itself
    differs by 1.6e-6 of max|proj| and its smallest pre-sign projection is 8.2e-4 of it (max|proj| is above 1), so no bit sits under the
    margin.  The margin is an absolute |proj| of 1e-4, which here is tighter than 1e-4 of max|proj|."""
    import phenaki_pytorch_amd as P
    cvc, _, _ = oracle_cfgs(TINY)
    cv = P.CViViT(use_vgg_and_gan=False, **dict(TINY['cvivit'], dim_head=32))
    weights.fill_module(cv, salt=1)
    sd = {k: v.clone() for k, v in cv.state_dict().items()}
    video = weights.synthetic_video(2, 5, 64, 64, seed=0)
    ids, proj = O.cvivit_tokenize(sd, cvc, video, return_proj=True)
    rec = O.cvivit_decode_ids(sd, cvc, ids.flatten(1))
    return cvc, video, ids, proj, rec


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
def test_cvivit_dim_head_32(L, tokenizer_reference, dtype):
    cvc, video, ids_ref, proj_ref, rec_ref = tokenizer_reference
    under = (proj_ref.abs() <= 1e-4).float().mean().item()
    assert under <= 1e-3, f'{under:.2%} of the oracle code bits are under the 1e-4 margin'
    cv, _ = _product('cvivit', dict(TINY['cvivit'], dim_head=32), 1, dtype)
    ids, proj = cv.tokenize(video.cuda(), return_proj=True)
    ids_equal_with_margin(ids, ids_ref, proj_ref, tol=1e-4 / proj_ref.abs().max().item(), what=f'tokenizer ids dim_head 32 {dtype}')
    # pixels after 2 + 2 + 2 + 2 transformer layers: the project's end-to-end value tolerance for the f32-grade modes (test_modules_gpu.MODES)
    rec = cv.decode_from_codebook_indices(ids_ref.flatten(1).cuda())
    close(rec, rec_ref, 1e-3, f'tokenizer reconstruction dim_head 32 {dtype}')


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
def test_maskgit_dim_head_128_cfg_and_kv_cache(L, dtype):
    from phenaki_pytorch_amd.attention import compute_dtype_of
    from phenaki_pytorch_amd.phenaki import _cfg_masks
    _, mgc, _ = oracle_cfgs(TINY)
    mg, sd = _product('MaskGit', dict(TINY['maskgit'], dim_head=128), 2, dtype)
    B, vps = 2, (3, 4, 4)
    n = 48
    ids = torch.randint(0, 256, (B, n), generator=g(50))
    ctx = weights.synthetic_context(B, 6, 96, seed=2)
    tm = torch.ones(B, 6, dtype=torch.bool)
    tm[1, 4:] = False
    ref = O.maskgit_cfg(sd, mgc, ids, cond_scale=3., video_patch_shape=vps, context=ctx, text_mask=tm)
    out = mg.forward_with_cond_scale(ids.cuda(), video_patch_shape=vps, context=ctx.cuda(), text_mask=tm.cuda(), cond_scale=3.)
    close(out, ref, TOL[dtype], f'MaskGit CFG logits dim_head 128 {dtype}')
    # the way sample() runs it: cond | null replicas, prepared uint8 masks, one kv_cache over the steps
    cache = {}
    ctx_r, tm_r = torch.cat((ctx, ctx)).cuda(), _cfg_masks(tm.cuda(), B, True)
    dt = compute_dtype_of(mg)
    for step in range(2):
        e = mg.embeds(ids.cuda(), replicas=2, video_patch_shape=vps, context=ctx_r, text_mask=tm_r, kv_cache=cache)
        mixed = torch.empty((B * n, mg.dim), device='cuda', dtype=L.tdtype(dt))
        L.cfg_mix(e, B, n, 0, None, B * n, 3., True, mixed, mg.dim)
        close(mg._logits(mixed, B * n, B, n), ref, TOL[dtype], f'MaskGit CFG logits with the kv_cache, step {step}, dim_head 128 {dtype}')
    assert len(cache) == 2                                             # the two cross-attention layers


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
def test_sample_dim_head_32(L, dtype):
    import phenaki_pytorch_amd as P
    cv, _ = _product('cvivit', dict(TINY['cvivit'], dim_head=32), 1, dtype)
    mg, _ = _product('MaskGit', dict(TINY['maskgit'], dim_head=32), 2, dtype)
    cr, _ = _product('TokenCritic', dict(TINY['critic'], dim_head=32), 3, dtype)
    ph = P.Phenaki(maskgit=mg, cvivit=cv, critic=cr, steps=3, text_embed_dim=96).cuda().eval()
    P.set_compute_dtype(ph, dtype)
    ctx = weights.synthetic_context(2, 6, 96, seed=2).cuda()
    ph.encode_texts = lambda texts, output_device=None: ctx
    for graph in (False, True):
        if graph:
            ph.enable_sample_graph()
        vid = ph.sample(texts=['a', 'b'], num_frames=5, cond_scale=3.)
        torch.cuda.synchronize()
        assert tuple(vid.shape) == (2, 3, 5, 64, 64) and torch.isfinite(vid).all()
