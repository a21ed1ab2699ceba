"""GPU parity tests of the training kernels at the shapes where their dispatch changes branch: the training forward's query rows per wave
(QF = 2 / 3, derived from the CU count), the attention backward's packed and K-split (kv_split) forms, ragged key tiles, cross-attention tile
edges, the PEG adjoint row kernel and the 27-gather kernel, the embed backward's run merging, and the LayerNorm-folded GEMM on the 256 x 256
variant's shapes.  Every reference is the oracle's restatement (oracle/phenaki_oracle.py) in float64: CPU autograd for the blocks, torch on the
GPU for the large products.  Each test asserts the branch condition it was written for, so that a changed threshold cannot silently turn it into
a duplicate of another case."""
import functools

import pytest
import torch
import torch.nn.functional as F

from oracle import phenaki_oracle as O
from tests.util import close, record_parity

pytestmark = pytest.mark.gpu

MODES = [('fp32', 1e-3), ('bf16x3', 1e-3), ('bf16', 6e-2)]
D, HEADS = 512, 8


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    torch.cuda.set_device(0)
    with torch.enable_grad():                      # other test modules switch grad mode off process-wide at import
        yield


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


# ---- host-side mirrors of the dispatch rules (csrc/attn.hip attn_fwd_impl, csrc/attn_train.hip kv_split_of / pk_attn_bwd_ws)

def _train_fwd(S, h, n):
    """(nq_pad, wg2, wg3): the split-bf16 training forward's workgroup counts with 128 and 192 query rows; QF = 3 iff wg2 > n_cu >= wg3"""
    from phenaki_pytorch_amd import _lib as L
    nq_pad, _ = L.attn_pads(n, n, 0)
    return nq_pad, S * h * -(-nq_pad // 128), S * h * -(-nq_pad // 192)


def _kv_split(S, h, n, nkt):
    """(G, chunk) of kv_split_of: the query tiles (32 rows) of a key tile dealt to G workgroups, `chunk` tiles each"""
    ntl, nqt = -(-nkt // 64), -(-n // 32)
    G = 768 // max(S * h * ntl, 1)
    if G < 2 or nqt < 2:
        return 1, nqt
    G = min(G, nqt)
    chunk = -(-nqt // G)
    return -(-nqt // chunk), chunk


def _bwd_work(S, h, n, n_kv, nnull):
    from phenaki_pytorch_amd import _lib as L
    return L.load().pk_attn_bwd_work(S, h, n, n_kv, nnull)


def _first_S(pred, what):
    for S in range(1, 4097):
        if pred(S):
            return S
    raise AssertionError(f'no batch size selects {what} on {_n_cu()} CUs')


# ---- A. attention block, forward and backward

ATTN_CASES = (['qf3_ragged', 'qf3_ragged_bias', 'qf3_even', 'qf2_wide', 'kv_split_uneven'] +
              [f'keys{n}_{v}' for n in (129, 191, 257) for v in ('plain', 'null2', 'null2_mask', 'causal')] +
              [f'packed{n}_{v}' for n in (1, 21, 31, 32) for v in ('plain', 'dS')] +
              ['cross65_ctx64', 'cross65_ctx1', 'fullmask129'])


def _attn_spec(case):
    """the shape of a case, with the dispatch condition it exists for asserted"""
    n_cu = _n_cu()
    sp = dict(S=2, n=None, nnull=0, bias=False, mask=False, causal=False, n_ctx=None, full=False)
    if case.startswith('qf3'):
        n = 384 if case == 'qf3_even' else 320
        S = _first_S(lambda S: _train_fwd(S, HEADS, n)[1] > n_cu >= _train_fwd(S, HEADS, n)[2], 'the 48-row training forward')
        nq_pad, wg2, wg3 = _train_fwd(S, HEADS, n)
        assert wg2 > n_cu >= wg3
        if case == 'qf3_even':
            assert nq_pad % 48 == 0 and n != 576
        else:
            assert nq_pad % 48 != 0, 'the ragged case needs a last wave that reaches past the head'
        sp.update(S=S, n=n, bias=case.endswith('_bias'))
        sp['branch'] = dict(qf=3, nq_pad=nq_pad, wg2=wg2, wg3=wg3, n_cu=n_cu)
    elif case == 'qf2_wide':
        n = 200
        S = _first_S(lambda S: _train_fwd(S, HEADS, n)[1] > n_cu, 'the 32-row training forward above n_cu')
        nq_pad, wg2, wg3 = _train_fwd(S, HEADS, n)
        assert wg2 > n_cu and wg3 > n_cu, 'QF = 2 with more workgroups than CUs'
        assert _bwd_work(S, HEADS, n, n, 0) == 0 and n > 64, 'the backward must run with kv_split = 1'
        sp.update(S=S, n=n)
        sp['branch'] = dict(qf=2, nq_pad=nq_pad, wg2=wg2, wg3=wg3, n_cu=n_cu, kv_split=1)
    elif case == 'kv_split_uneven':
        n = 320
        S = _first_S(lambda S: _kv_split(S, HEADS, n, n)[0] > 1 and (-(-n // 32)) % _kv_split(S, HEADS, n, n)[1] != 0, 'an uneven kv_split')
        G, chunk = _kv_split(S, HEADS, n, n)
        work = _bwd_work(S, HEADS, n, n, 0)
        assert work > 0 and work == 2 * G * S * HEADS * n * 64, 'the host mirror of kv_split_of disagrees with pk_attn_bwd_work'
        assert (-(-n // 32)) % chunk != 0
        sp.update(S=S, n=n)
        sp['branch'] = dict(kv_split=G, chunk=chunk, nqt=-(-n // 32))
    elif case == 'fullmask129':
        sp.update(n=129, mask=True, full=True, bias=True)        # no null keys: every score row of the masked sequence is fully masked
        assert sp['nnull'] == 0 and sp['S'] >= 2
        sp['branch'] = dict(nk=129, fully_masked_sequences=1, rows=HEADS * 129)
    elif case.startswith('keys'):
        n, v = case[4:].split('_', 1)
        n = int(n)
        sp.update(n=n, nnull=0 if v == 'plain' else 2, mask=v == 'null2_mask', causal=v == 'causal')
        nk = sp['nnull'] + n
        assert nk % 32 != 0 and nk % 64 != 0, 'a ragged last key tile'
        sp['branch'] = dict(nk=nk, last_tile=nk % 64)
    elif case.startswith('packed'):
        n, v = case[6:].split('_')
        n = int(n)
        S = 5
        sp.update(S=S, n=n, bias=v == 'dS')
        pack_g = 64 // n
        packed = not sp['bias']                                  # pk_attn_bwd_ws: nnull == 0, n == n_kv, n <= 32, no dS
        assert n <= 32 and sp['nnull'] == 0
        sp['branch'] = dict(packed=packed, pack_g=pack_g, groups=S * HEADS, tiles=-(-S * HEADS // pack_g), rows_per_tile=pack_g * n)
    elif case.startswith('cross'):
        n_ctx = int(case.split('ctx')[1])
        sp.update(n=65, nnull=2, mask=True, n_ctx=n_ctx)
        assert sp['n'] != n_ctx
        sp['branch'] = dict(nq=65, nk=n_ctx + 2)
    else:
        raise KeyError(case)
    return sp


def _make_attn(sp, seed):
    import phenaki_pytorch_amd as P
    torch.manual_seed(seed)
    cross = sp['n_ctx'] is not None
    attn = P.attention.Attention(dim=D, dim_context=96 if cross else None, heads=HEADS, num_null_kv=sp['nnull'], causal=sp['causal'])
    with torch.no_grad():
        attn.q_scale.uniform_(0.5, 1.5)
        attn.k_scale.uniform_(0.5, 1.5)
        attn.norm.gamma.uniform_(0.5, 1.5)
        if cross:
            attn.context_norm.gamma.uniform_(0.5, 1.5)
    return attn


def _inputs(sp, seed):
    g = torch.Generator().manual_seed(seed)
    S, n = sp['S'], sp['n']
    x, G = torch.randn(S, n, D, generator=g), torch.randn(S, n, D, generator=g)
    ctx = mask = bias = None
    if sp['n_ctx'] is not None:
        ctx = torch.randn(S, sp['n_ctx'], 96, generator=g)
        mask = torch.rand(S, sp['n_ctx'], generator=g) > 0.3
        mask[:, 0] = True
    elif sp['mask']:
        mask = torch.rand(S, n, generator=g) > 0.2
        mask[:, 0] = True
        if sp.get('full'):
            mask[-1] = False
    if sp['bias']:
        bias = torch.randn(HEADS, n, n, generator=g)
    return x, G, ctx, mask, bias


def _grad_names(sp):
    return ('to_q.weight', 'to_kv.weight', 'to_out.weight', 'q_scale', 'k_scale', 'norm.gamma') + (('null_kv',) if sp['nnull'] else ()) + \
        (('context_norm.gamma',) if sp['n_ctx'] is not None else ())


@functools.lru_cache(maxsize=None)
def _attn_reference(case):
    """float64 CPU autograd of x + oracle.attention(x) for a case: (dx, {name: grad}, dbias | None); the same for every compute mode"""
    sp = _attn_spec(case)
    attn = _make_attn(sp, 11)
    x, G, ctx, mask, bias = _inputs(sp, 12)
    params = dict(attn.named_parameters())
    sd = {k: (v.detach().double().requires_grad_() if k in params else v.detach().double()) for k, v in attn.state_dict().items()}
    xl = x.double().requires_grad_()
    bl = bias.double().requires_grad_() if bias is not None else None
    y = O.attention(sd, '', xl, heads=HEADS, context=ctx.double() if ctx is not None else None, mask=mask, attn_bias=bl, causal=sp['causal']) + xl
    y.backward(G.double())
    return xl.grad, {k: sd[k].grad for k in _grad_names(sp)}, (bl.grad if bl is not None else None)


@pytest.mark.parametrize('dtype,tol', MODES)
@pytest.mark.parametrize('case', ATTN_CASES)
def test_attention_block_branches(case, dtype, tol):
    """x + Attention(x) (attention.py:89-182), D = 512, 8 heads, through attention_train in every compute mode, against float64 autograd of the
    oracle: dx and the gradients of to_q / to_kv / to_out, q_scale / k_scale, norm.gamma, null_kv, context_norm.gamma and the bias matrix.
    qf3_*: the split-bf16 training forward with 48 query rows per wave (wg2 > n_cu >= wg3), at n = 320 (nq_pad % 48 != 0: the last wave of a
    head reaches 32 rows past it -- the Q fragment rows are clamped there) with and without the bias matrix, and at n = 384 (nq_pad % 48 == 0);
    qf2_wide: 64 rows per wave above n_cu with the backward at kv_split = 1; kv_split_uneven: the backward's query tiles dealt to G workgroups
    with a short last chunk; keys*: ragged last key tiles with / without null keys, key mask, causal + ALiBi; packed*: pk_attn_bwd_ws's packed
    (sequence, head) groups at 64 / n per tile and, with dS wanted (the bias gradient), the unpacked path; cross*: n != n_kv at a tile edge;
    fullmask129: the last sequence's key mask is all False and there are no null keys -- uniform attention, no gradient to q, k or the bias from it."""
    from phenaki_pytorch_amd.attention import resolve_dtype
    from phenaki_pytorch_amd.train import attention_train
    sp = _attn_spec(case)
    dx_ref, g_ref, db_ref = _attn_reference(case)
    attn = _make_attn(sp, 11).cuda()
    x, G, ctx, mask, bias = _inputs(sp, 12)
    S, n = sp['S'], sp['n']
    n_ctx = sp['n_ctx']
    xc = x.reshape(S * n, D).cuda().requires_grad_()
    bc = bias.cuda().requires_grad_() if bias is not None else None
    with torch.enable_grad():
        y = attention_train(attn, xc, S, n, resolve_dtype(dtype), context2d=ctx.reshape(S * n_ctx, 96).cuda() if ctx is not None else None,
                            n_ctx=n_ctx, attn_bias=bc, kmask=mask.to(torch.uint8).cuda() if mask is not None else None)
    y.backward(G.reshape(S * n, D).cuda())
    errs = dict(dx=close(xc.grad, dx_ref.reshape(S * n, D), tol, f'{case} dx'))
    floor = g_ref['to_kv.weight'].abs().max().item()

    def cmp(got, ref, what):
        if ref.abs().max().item() == 0:
            # one key per row (n = 1, no null keys): softmax is 1 whatever the score is, so the scores and everything upstream of them (q^, k^,
            # the bias) have an exactly zero gradient -- held to rounding noise on the scale of the value-side weight gradient
            err = got.abs().max().item()
            assert err <= tol * floor, f'{case} {what}: {err:.3e} where the reference is exactly 0 (> {tol:g} * {floor:.3e})'
            return err / floor
        return close(got, ref, tol, f'{case} {what}')

    for name in _grad_names(sp):
        mod = attn
        for part in name.split('.'):
            mod = getattr(mod, part)
        errs[name] = cmp(mod.grad, g_ref[name], f'd {name}')
    if bc is not None:
        errs['bias'] = cmp(bc.grad, db_ref, 'd bias')
    record_parity('train_kernels_attention', dict(case=case, dtype=dtype, S=S, n=n, branch=sp['branch'], **errs))


# ---- B. PEG backward

@pytest.mark.parametrize('Dp', [64, 512])
@pytest.mark.parametrize('T', [1, 2, 5])
@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('W', [4, 8, 16, 3, 5])
def test_peg_backward_branches(W, causal, T, Dp):
    """x + PEG(x) (attention.py:57-85) against float64 autograd of the oracle: dx, dW, db.  W in {4, 8, 16}: dx by the forward's row kernel run
    as its own adjoint (mirrored taps, tfront' = 2 - tfront); W in {3, 5}: the 27-gather kernel."""
    import phenaki_pytorch_amd as P
    from phenaki_pytorch_amd.train import peg_train
    torch.manual_seed(40 + W)
    shape = (2, T, 3, W)
    peg = P.attention.PEG(dim=Dp, causal=causal)
    sd = {k: v.detach().double().requires_grad_() for k, v in peg.state_dict().items()}
    M = shape[0] * T * 3 * W
    g = torch.Generator().manual_seed(41)
    x, G = torch.randn(M, Dp, generator=g), torch.randn(M, Dp, generator=g)
    xl = x.double().requires_grad_()
    (O.peg(sd, '', xl.reshape(shape[0], -1, Dp), shape, causal).reshape(M, Dp) + xl).backward(G.double())
    peg = peg.cuda()
    xc = x.cuda().requires_grad_()
    with torch.enable_grad():
        y = peg_train(peg, xc, shape)
    y.backward(G.cuda())
    errs = dict(dx=close(xc.grad, xl.grad, 1e-4, 'peg dx'),
                dw=close(peg.dsconv.weight.grad, sd['dsconv.weight'].grad, 1e-4, 'peg d weight'),
                db=close(peg.dsconv.bias.grad, sd['dsconv.bias'].grad, 1e-4, 'peg d bias'))
    record_parity('train_kernels_peg', dict(W=W, causal=causal, T=T, D=Dp, dx_kernel='adjoint_row' if W in (4, 8, 16) else 'gather27', **errs))


@pytest.mark.parametrize('W', [4, 3])
def test_peg_backward_refuses_in_place(W):
    """pk_peg_bwd with dy == dx: both dx kernels read dy's neighbours while writing dx, so the call is refused with PK_EINVAL before any launch
    (it used to fall back from the adjoint's refusal to the gather kernel, which then raced on the in-place data)"""
    from phenaki_pytorch_amd import _lib as L
    B, T, H, Dp = 2, 2, 3, 64
    rows = B * T * H * W
    g = torch.Generator().manual_seed(42)
    dy = torch.randn(rows, Dp, generator=g).cuda()
    x = torch.randn(rows, Dp, generator=g).cuda()
    wt = torch.randn(27, Dp, generator=g).cuda()
    before = dy.clone()
    part = torch.empty((L.load().pk_peg_wgrad_parts(rows), 27 * Dp), device='cuda')
    rc = L.load().pk_peg_bwd(L.ptr(dy), L.ptr(x), L.ptr(wt), L.ptr(dy), L.ptr(part), B, T, H, W, Dp, 0, L.stream(dy))
    assert rc == -1, f'pk_peg_bwd(dy == dx) returned {rc}, expected PK_EINVAL'
    with pytest.raises(RuntimeError, match='PK_EINVAL'):
        L.peg_bwd(dy, x, wt, dy, B, T, H, W, Dp, False)
    torch.cuda.synchronize()
    assert torch.equal(dy, before), 'a refused call must not have touched dy'


# ---- C. embed backward run merging

@pytest.mark.parametrize('case', ['all_equal', 'one_run_per_position', 'alternating', 'mask_id', 'grid_wrap'])
def test_embed_backward_runs(case):
    """_Embed (tok[ids] + pos, gradient scaled by alpha) against a float64 reference where the runs of equal ids across the sequences decide
    how the kernel adds: one run over all 64 sequences (every id equal / the mask id everywhere / each position one id of its own), a run break
    at every sequence (alternating ids), and n * D / 4 beyond the grid's 65535 x 256 threads (the grid-stride loop wraps; float64 on the GPU)"""
    from phenaki_pytorch_amd.train import _Embed
    g = torch.Generator().manual_seed(50)
    alpha = 0.1
    if case == 'grid_wrap':
        S, n, Dp, V1 = 2, 1_100_000, 64, 4096
        assert n * (Dp // 4) > 65535 * 256
        dev = 'cuda'
    else:
        S, n, Dp, V1 = 64, 40, 64, 50
        dev = 'cpu'
    if case in ('all_equal', 'mask_id'):
        ids = torch.full((S, n), 7 if case == 'all_equal' else V1 - 1, dtype=torch.long)
    elif case == 'one_run_per_position':
        ids = (torch.arange(n) % V1).expand(S, n).contiguous()
    elif case == 'alternating':
        ids = torch.where((torch.arange(S) % 2 == 0)[:, None], torch.arange(n) % 7, V1 - 1 - torch.arange(n) % 5).long()
    else:
        ids = torch.randint(0, V1, (S, n), generator=g)
    tok, pos = torch.randn(V1, Dp, generator=g), torch.randn(n, Dp, generator=g)
    G = torch.randn(S * n, Dp, generator=g)
    tc, pc = tok.cuda().requires_grad_(), pos.cuda().requires_grad_()
    with torch.enable_grad():
        x = _Embed.apply(tc, pc, ids.cuda(), alpha)
    x.backward(G.cuda())
    G64, ids_d = G.to(dev).double(), ids.to(dev)
    dtok = torch.zeros(V1, Dp, dtype=torch.float64, device=dev).index_add_(0, ids_d.reshape(-1), G64) * alpha
    dpos = G64.reshape(S, n, Dp).sum(0) * alpha
    errs = dict(dtok=close(tc.grad, dtok, 1e-5, f'{case} d token_emb'), dpos=close(pc.grad, dpos, 1e-5, f'{case} d pos_emb'))
    record_parity('train_kernels_embed', dict(case=case, S=S, n=n, **errs))


# ---- E. LayerNorm-folded GEMM on the 256 x 256 variant's shape

def test_gemm_layernorm_fold_variant50_shape():
    """bf16, K = 2048, 512 tiles of 256 x 256: pk_gemm_auto_variant resolves to 50 (the two-group 256 x 256 loop, which has no folded form); the
    folded product takes the 128 x 128 tile there.  Against float64 on the GPU: the folded expression on the rounded operands (3e-5, the bf16
    tolerance of test_gemm_layernorm_fold_and_bf16_copy) and LayerNorm + Linear itself (3e-2)."""
    from torch import nn
    from phenaki_pytorch_amd import _lib as L
    from phenaki_pytorch_amd import attention as A
    dt = L.BF16
    M, N, K = 4096, 8192, 2048
    g = torch.Generator(device='cuda').manual_seed(60)
    x = torch.randn(M, K, generator=g, device='cuda') * 1.3 + 0.4
    gamma, beta = 1 + 0.2 * torch.randn(K, generator=g, device='cuda'), 0.1 * torch.randn(K, generator=g, device='cuda')
    W = torch.randn(N, K, generator=g, device='cuda') / K ** 0.5
    res = torch.randn(M, N, generator=g, device='cuda')
    wg, s, t, _ = A.folded_weight(nn.Linear(1, 1), 'k', lambda: W, gamma, beta, dt, [gamma])
    xa = x.to(torch.bfloat16)
    variant = L.load().pk_gemm_auto_variant(dt, 0, M, N, K, xa.stride(0), wg.stride(0), M)
    assert variant == 50, f'the shape resolves to variant {variant}, not 50'
    C = torch.full((M, N), float('nan'), device='cuda')
    L.gemm(dt, xa, wg, M, N, K, C=C, res=res, ln=(s, t, 1e-5))
    xb = xa.double()
    mean = xb.mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt((xb * xb).mean(-1, keepdim=True) - mean * mean + 1e-5)
    wgr = (W * gamma).to(torch.bfloat16).double()
    ref = rstd * (xb @ wgr.t() - mean * wgr.sum(-1)) + (W.double() @ beta.double()) + res.double()
    del xb, wgr
    e_fold = close(C, ref, 3e-5, 'ln-folded gemm vs the folded expression (variant-50 shape)')
    del ref
    true = F.layer_norm(x.double(), (K,), gamma.double(), beta.double()) @ W.double().t() + res.double()
    e_true = close(C, true, 3e-2, 'ln-folded gemm vs LayerNorm + Linear (variant-50 shape)')
    record_parity('train_kernels_ln_fold_gemm', dict(M=M, N=N, K=K, auto_variant=variant, folded=e_fold, layernorm_linear=e_true))
