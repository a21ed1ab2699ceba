"""GPU tests of attn_dropout / ff_dropout in the training kernels (reference attention.py:45-52, :177): the mask kernel against its NumPy mirror,
the attention and feed-forward blocks (forward and every gradient) against a float64 restatement that applies the dumped mask, the train / eval /
reseed switches, and whole training steps of Phenaki and C-ViViT built with dropout."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import phenaki_oracle as O
from oracle import weights
from oracle.configs import TINY, state_dicts
from phenaki_pytorch_amd import dropout as DR
from tests.test_train_kernels_gpu import D, HEADS, MODES, _bwd_work, _inputs, _make_attn, _n_cu, _train_fwd
from tests.util import close

pytestmark = pytest.mark.gpu

P_ATTN, P_FF = 0.25, 0.1
SEED = 77


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    torch.cuda.set_device(0)
    with torch.enable_grad():                      # other test modules switch grad mode off process-wide at import
        yield


def _generator_state():
    gen = torch.cuda.default_generators[0]
    return gen.initial_seed(), gen.get_offset()


# ---- the mask kernel

@pytest.mark.parametrize('rows,cols,p', [(3 * 8 * 70, 72, 0.25), (200, 1365, 0.1)])
def test_mask_kernel_equals_numpy_mirror(rows, cols, p):
    """pk_dropout_mask == dropout.keep_mask byte for byte on an attention-shaped range ((s h i) rows x 2 null + 70 keys) and a feed-forward range
    (inner width 1365: a last group of one column); another seed or offset gives another mask"""
    from phenaki_pytorch_amd import _lib as L
    seed, off = 0x1234567890ABCDEF, 4 * 12345
    got = L.dropout_mask(seed, off, rows, cols, p, 'cuda').cpu().numpy()
    want = DR.keep_mask(seed, off, rows, cols, p)
    assert got.dtype == np.uint8 and got.shape == (rows, cols)
    assert np.array_equal(got, want)
    assert 0 < got.sum() < got.size
    for s2, o2 in ((seed + 1, off), (seed, off + 4), (seed ^ (1 << 40), off), (seed, off + (1 << 32))):
        other = L.dropout_mask(s2, o2, rows, cols, p, 'cuda').cpu().numpy()
        assert np.array_equal(other, DR.keep_mask(s2, o2, rows, cols, p))
        assert not np.array_equal(other, got)


# ---- attention block

ATTN_CASES = ['self64_null2', 'self200_null2_mask', 'causal9', 'cross200_ctx14_null2_mask', 'self320_bias']


def _spec(case):
    sp = dict(S=2, n=None, nnull=0, bias=False, mask=False, causal=False, n_ctx=None)
    if case == 'self64_null2':                       # one key tile of the backward (66 keys: two 64-key tiles, three 32-key tiles of the forward)
        sp.update(n=64, nnull=2)
    elif case == 'self200_null2_mask':               # ragged tiles, key mask
        sp.update(n=200, nnull=2, mask=True)
    elif case == 'causal9':                          # the C-ViViT temporal transformer: causal + ALiBi; p = 0 takes the packed backward here
        sp.update(S=5, n=9, causal=True)
    elif case == 'cross200_ctx14_null2_mask':        # cross-attention on one key tile: the backward deals the query tiles out (workspace split)
        sp.update(n=200, nnull=2, n_ctx=14, mask=True)
        assert _bwd_work(sp['S'], HEADS, 200, 14, 2) > 0, 'the cross-attention case must take the kv_split workspace form'
    elif case == 'self320_bias':                     # S heads = 96: where p = 0 in bf16x3 takes the 48-row LDS-staged forward
        sp.update(S=12, n=320, bias=True)
        assert sp['S'] * HEADS == 96
        if _n_cu() == 256:
            _, wg2, wg3 = _train_fwd(sp['S'], HEADS, 320)
            assert wg2 > 256 >= wg3, 'on 256 CUs the p = 0 bf16x3 forward of this shape is the 48-row LDS-staged kernel'
    else:
        raise KeyError(case)
    return sp


def _case_inputs(case):
    sp = _spec(case)
    x, G, ctx, mask, bias = _inputs(sp, 12)
    if sp['n_ctx'] is not None:                      # a text mask with a short caption: sequence 0 full, sequence 1 three tokens
        mask = torch.zeros(sp['S'], sp['n_ctx'], dtype=torch.bool)
        mask[0] = True
        mask[1, :3] = True
    return sp, x, G, ctx, mask, bias


def _grad_names(sp):
    return ('to_q.weight', 'to_kv.weight', 'to_out.weight', 'q_scale', 'k_scale', 'norm.gamma') + (('null_kv',) if sp['nnull'] else ()) + \
        (('context_norm.gamma',) if sp['n_ctx'] is not None else ())


def attention_with_dropout_f64(sd, x, *, heads, keep, scale_keep, causal=False, mask=None, context=None, attn_bias=None, scale=8):
    """attention.py:128-182 restated in the dtype of its inputs (float64 here), dropout included: `keep` (b, heads, i, nnull + j) of {0, 1} multiplies
    the softmax probabilities, survivors are scaled by `scale_keep` = 1 / (1 - p_eff) (attention.py:177), then attn @ v.  K / V of
    self-attention come from the un-normalised x; null k / v rows are interleaved; l2norm of k after the null-k concat."""
    b = x.shape[0]
    if context is not None:
        context = F.layer_norm(context, context.shape[-1:], sd['context_norm.gamma'], sd['context_norm.beta'])
    kv_in = context if context is not None else x
    q = F.layer_norm(x, x.shape[-1:], sd['norm.gamma'], sd['norm.beta']) @ sd['to_q.weight'].t()
    k, v = (kv_in @ sd['to_kv.weight'].t()).chunk(2, dim=-1)

    def split(t):
        return t.reshape(t.shape[0], t.shape[1], heads, -1).permute(0, 2, 1, 3)
    q, k, v = split(q), split(k), split(v)
    null_kv = sd['null_kv']
    nnull = null_kv.shape[1] // 2
    k = torch.cat((null_kv[:, 0::2].unsqueeze(0).expand(b, -1, -1, -1), k), dim=-2)
    v = torch.cat((null_kv[:, 1::2].unsqueeze(0).expand(b, -1, -1, -1), v), dim=-2)
    q = F.normalize(q, dim=-1) * sd['q_scale']
    k = F.normalize(k, dim=-1) * sd['k_scale']
    sim = torch.einsum('bhid,bhjd->bhij', q, k) * scale
    i, j = sim.shape[-2:]
    if attn_bias is not None:
        sim = sim + F.pad(attn_bias, (nnull, 0), value=0.)
    if mask is not None:
        sim = sim.masked_fill(~F.pad(mask, (nnull, 0), value=True)[:, None, None, :], -torch.finfo(torch.float32).max)
    if causal:
        sim = sim + O.alibi_bias(heads, i, j).to(sim.dtype)
        sim = sim.masked_fill(torch.ones((i, j), dtype=torch.bool).triu(j - i + 1), -torch.finfo(torch.float32).max)
    attn = sim.softmax(dim=-1)
    attn = attn * keep * scale_keep                                      # nn.Dropout in training mode with the kernels' mask
    out = torch.einsum('bhij,bhjd->bhid', attn, v)
    return out.permute(0, 2, 1, 3).reshape(b, i, -1) @ sd['to_out.weight'].t()


@functools.lru_cache(maxsize=None)
def _attn_reference(case):
    """float64 CPU autograd of x + attention(x) with the mask of site (SEED, offset 0): (y, dx, dctx | None, {name: grad}, dbias | None); computed
    once per case and shared by the three compute modes"""
    sp, x, G, ctx, mask, bias = _case_inputs(case)
    attn = _make_attn(sp, 11)
    S, n = sp['S'], sp['n']
    nk = sp['nnull'] + (sp['n_ctx'] if sp['n_ctx'] is not None else n)
    thr, p_eff, scale_keep = DR.quantize(P_ATTN)
    keep = torch.from_numpy(DR.keep_mask(SEED, 0, S * HEADS * n, nk, P_ATTN)).reshape(S, HEADS, n, nk).double()
    params = dict(attn.named_parameters())
    sd = {k: (v.detach().double().requires_grad_() if k in params else v.detach().double()) for k, v in attn.state_dict().items()}
    xl = x.double().requires_grad_()
    cl = ctx.double().requires_grad_() if ctx is not None else None
    bl = bias.double().requires_grad_() if bias is not None else None
    y = attention_with_dropout_f64(sd, xl, heads=HEADS, keep=keep, scale_keep=scale_keep, context=cl, mask=mask, attn_bias=bl, causal=sp['causal']) + xl
    y.backward(G.double())
    return y.detach(), xl.grad, (cl.grad if cl is not None else None), {k: sd[k].grad for k in _grad_names(sp)}, (bl.grad if bl is not None else None)


@pytest.mark.parametrize('dtype,tol', MODES)
@pytest.mark.parametrize('case', ATTN_CASES)
def test_attention_block_with_dropout(case, dtype, tol):
    """x + Attention(x) with attn_dropout = 0.25 in training mode through attention_train, in every compute mode: the output and the gradients of
    x, context, norm.gamma, to_q, to_kv, null_kv, q_scale, k_scale, to_out, context_norm.gamma and the bias matrix against the float64
    restatement above, which applies the mask of the call's dropout site (NumPy mirror; the mask kernel is held to it byte for byte above).
    Tolerances: those of tests/test_train_kernels_gpu.py for the same mode at p = 0.  (The issue allows that tolerance times 1 / (1 - p_eff),
    because the survivor scale amplifies the absolute error by that factor; no case needed it.)"""
    from phenaki_pytorch_amd.attention import resolve_dtype
    from phenaki_pytorch_amd.train import attention_train
    sp, x, G, ctx, mask, bias = _case_inputs(case)
    y_ref, dx_ref, dctx_ref, g_ref, db_ref = _attn_reference(case)
    attn = _make_attn(sp, 11).cuda()
    attn.attn_dropout.p = P_ATTN
    assert attn.attn_dropout.training
    S, n, n_ctx = sp['S'], sp['n'], sp['n_ctx']
    xc = x.reshape(S * n, D).cuda().requires_grad_()
    cc = ctx.reshape(S * n_ctx, 96).cuda().requires_grad_() if ctx is not None else None
    bc = bias.cuda().requires_grad_() if bias is not None else None
    km = mask.to(torch.uint8).cuda() if mask is not None else None
    torch.manual_seed(SEED)
    assert _generator_state() == (SEED, 0)
    y = attention_train(attn, xc, S, n, resolve_dtype(dtype), context2d=cc, n_ctx=n_ctx, attn_bias=bc, kmask=km)
    assert _generator_state() == (SEED, 4), 'one dropout site advances the generator by 4'
    y.backward(G.reshape(S * n, D).cuda())
    errs = dict(y=close(y, y_ref.reshape(S * n, D), tol, f'{case} y'), dx=close(xc.grad, dx_ref.reshape(S * n, D), tol, f'{case} dx'))
    if cc is not None:
        errs['dctx'] = close(cc.grad, dctx_ref.reshape(S * n_ctx, 96), tol, f'{case} d context')
    for name in _grad_names(sp):
        mod = attn
        for part in name.split('.'):
            mod = getattr(mod, part)
        errs[name] = close(mod.grad, g_ref[name], tol, f'{case} d {name}')
    if bc is not None:
        errs['bias'] = close(bc.grad, db_ref, tol, f'{case} d bias')
    print(f'dropout attention {case} {dtype}: ' + ' '.join(f'{k}={v:.2e}' for k, v in errs.items()))


# ---- feed-forward block

@functools.lru_cache(maxsize=None)
def _ff_case():
    import phenaki_pytorch_amd as P
    torch.manual_seed(2)
    Dm, M = 64, 200
    ff = P.attention.FeedForward(dim=Dm, dropout=P_FF)
    with torch.no_grad():
        ff[0].weight.uniform_(0.5, 1.5)
        ff[0].bias.normal_(0, 0.3)
    g = torch.Generator().manual_seed(3)
    x, G = torch.randn(M, Dm, generator=g), torch.randn(M, Dm, generator=g)
    Fi = ff[4].weight.shape[1]
    assert Fi % 8 != 0, 'the inner width must need padding to the stored width'
    _, p_eff, scale_keep = DR.quantize(P_FF)
    keep = torch.from_numpy(DR.keep_mask(SEED, 0, M, Fi, P_FF)).double()
    sd = {k: v.detach().double().requires_grad_() for k, v in ff.state_dict().items()}
    xl = x.double().requires_grad_()
    h = F.layer_norm(xl, (Dm,), sd['0.weight'], sd['0.bias']) @ sd['1.weight'].t()
    val, gate = h.chunk(2, dim=-1)
    a = F.gelu(gate) * val * keep * scale_keep                           # attention.py:45-52: GEGLU, Dropout
    y = a @ sd['4.weight'].t() + xl
    y.backward(G.double())
    return ff, x, G, y.detach(), xl.grad, {k: v.grad for k, v in sd.items()}


@pytest.mark.parametrize('dtype,tol', MODES)
def test_feedforward_block_with_dropout(dtype, tol):
    """x + FeedForward(x) with ff_dropout = 0.1 in training mode (M = 200, dim 64, inner width 170 stored as 176): output and every gradient against
    float64 with the site's mask over the TRUE inner width; tolerances of the p = 0 test of the same mode"""
    import copy
    from phenaki_pytorch_amd.train import feedforward_train
    from phenaki_pytorch_amd.attention import resolve_dtype
    ff0, x, G, y_ref, dx_ref, g_ref = _ff_case()
    ff = copy.deepcopy(ff0).cuda()
    assert ff[3].training and ff[3].p == P_FF
    xc = x.cuda().requires_grad_()
    torch.manual_seed(SEED)
    y = feedforward_train(ff, xc, resolve_dtype(dtype))
    assert _generator_state() == (SEED, 4)
    y.backward(G.cuda())
    errs = dict(y=close(y, y_ref, tol, 'ff y'), dx=close(xc.grad, dx_ref, tol, 'ff dx'),
                dw1=close(ff[1].weight.grad, g_ref['1.weight'], tol, 'ff dW1'), dw2=close(ff[4].weight.grad, g_ref['4.weight'], tol, 'ff dW2'),
                dlnw=close(ff[0].weight.grad, g_ref['0.weight'], tol, 'ff d ln weight'), dlnb=close(ff[0].bias.grad, g_ref['0.bias'], tol, 'ff d ln bias'))
    print(f'dropout feed-forward {dtype}: ' + ' '.join(f'{k}={v:.2e}' for k, v in errs.items()))


# ---- the unified entry points

def test_entry_points_take_an_optional_site():
    """pk_geglu, pk_geglu_bwd, pk_attn_fwd_lse and pk_attn_bwd_ws each take the dropout site as an argument: without one the result is the p = 0 float64
    oracle's, with one the oracle's under dropout.keep_mask (both at the fp32 tolerance of MODES: the operands here are f32); a site whose keep_thr
    is 0 or 257 is PK_EINVAL and nothing is written; the attention forward with a site but no lse is refused.  Smallest shapes that launch: GEGLU
    M = 4, F = 8 (stored width 8); attention S = 1, heads = 2, n = n_kv = 20 (one ragged tile)."""
    import ctypes
    from types import SimpleNamespace
    from phenaki_pytorch_amd import _lib as L
    tol = dict(MODES)['fp32']
    thr, _, scale_keep = DR.quantize(P_ATTN)

    def site(keep_thr=thr):
        return SimpleNamespace(c=L.Dropout(SEED, 8, keep_thr, scale_keep))
    g = torch.Generator().manual_seed(5)

    def refused(call, *outs):
        for bad in (0, 257):
            for t in outs:
                t.fill_(-7.)
            with pytest.raises(RuntimeError, match='PK_EINVAL'):
                call(site(bad))
            torch.cuda.synchronize()
            assert all(bool((t == -7.).all()) for t in outs), 'a refused call must not launch'

    # GEGLU: h = value | gate
    M, Fw = 4, 8
    h, dout = torch.randn(M, 2 * Fw, generator=g), torch.randn(M, Fw, generator=g)
    hc, dc = h.cuda(), dout.cuda()
    out, dh = torch.empty(M, Fw, device='cuda'), torch.empty(M, 2 * Fw, device='cuda')
    keep_ff = torch.from_numpy(DR.keep_mask(SEED, 8, M, Fw, P_ATTN)).double()
    for drop, m in ((None, torch.ones(M, Fw, dtype=torch.float64)), (site(), keep_ff * scale_keep)):
        hl = h.double().requires_grad_()
        ref = hl[:, :Fw] * F.gelu(hl[:, Fw:]) * m
        ref.backward(dout.double())
        L.geglu(hc, Fw, out, M, Fw, drop)
        L.geglu_bwd(hc, Fw, dc, dh, M, Fw, drop)
        close(out, ref, tol, f'geglu site={drop is not None}')
        close(dh, hl.grad, tol, f'geglu_bwd site={drop is not None}')
    refused(lambda d: L.geglu(hc, Fw, out, M, Fw, d), out)
    refused(lambda d: L.geglu_bwd(hc, Fw, dc, dh, M, Fw, d), dh)

    # attention: the f32 operands of the backward (pk_attn_train_prep) are the oracle's inputs
    S, H, n = 1, 2, 20
    q, kv, dO = torch.randn(S * n, H * 64, generator=g).cuda(), torch.randn(S * n, 2 * H * 64, generator=g).cuda(), torch.randn(S * n, H * 64, generator=g).cuda()
    qs, ks = torch.rand(64, generator=g).cuda() + 0.5, torch.rand(64, generator=g).cuda() + 0.5
    nq_pad, nk_pad = L.attn_pads(n, n, 0)
    Qp, Kp, Vt = (torch.empty(S * H * pad * 64, device='cuda') for pad in (nq_pad, nk_pad, nk_pad))
    L.attn_prep(L.F32, q, kv, None, qs, ks, 8., Qp, Kp, Vt, S, H, n, n, 0)
    Qh, Kh, Vh = (torch.empty(S * H * n, 64, device='cuda') for _ in range(3))
    L.attn_train_prep(q, kv, None, qs, ks, 8., Qh, Kh, Vh, S, H, n, n, 0)
    o, lse = torch.empty(S * n, H * 64, device='cuda'), torch.empty(S * H * n, device='cuda')
    dQh, dKh, dVh = torch.empty_like(Qh), torch.empty_like(Kh), torch.empty_like(Vh)
    keep_at = torch.from_numpy(DR.keep_mask(SEED, 8, S * H * n, n, P_ATTN)).reshape(S * H, n, n).double()
    for drop, m in ((None, torch.ones(S * H, n, n, dtype=torch.float64)), (site(), keep_at * scale_keep)):
        Ql, Kl, Vl = (t.double().cpu().reshape(S * H, n, 64).requires_grad_() for t in (Qh, Kh, Vh))
        sim = Ql @ Kl.transpose(1, 2)
        ref = ((sim.softmax(dim=-1) * m) @ Vl).reshape(S, H, n, 64).permute(0, 2, 1, 3).reshape(S * n, H * 64)
        ref.backward(dO.double().cpu())
        L.attn_fwd(L.F32, Qp, Kp, Vt, o, S, H, n, n, 0, lse=lse, drop=drop)
        L.attn_bwd(Qh, Kh, Vh, o, dO, dQh, dKh, dVh, S, H, n, n, 0, lse=lse, drop=drop)
        close(o, ref, tol, f'attn_fwd site={drop is not None}')
        close(lse, sim.logsumexp(dim=-1).reshape(-1), tol, f'lse (of the undropped scores) site={drop is not None}')
        for got, want, name in ((dQh, Ql, 'dQ'), (dKh, Kl, 'dK'), (dVh, Vl, 'dV')):
            close(got, want.grad.reshape(S * H * n, 64), tol, f'attn_bwd {name} site={drop is not None}')
    refused(lambda d: L.attn_fwd(L.F32, Qp, Kp, Vt, o, S, H, n, n, 0, lse=lse, drop=d), o)
    refused(lambda d: L.attn_bwd(Qh, Kh, Vh, o, dO, dQh, dKh, dVh, S, H, n, n, 0, lse=lse, drop=d), dQh, dKh, dVh)
    o.fill_(-7.)
    with pytest.raises(AssertionError):                                  # the binding refuses it ...
        L.attn_fwd(L.F32, Qp, Kp, Vt, o, S, H, n, n, 0, lse=None, drop=site())
    rc = L.load().pk_attn_fwd_lse(L.F32, Qp.data_ptr(), Kp.data_ptr(), Vt.data_ptr(), None, 0, 0, None, None, 0, o.data_ptr(), o.stride(0), 1, S, H, n, n, 0,
                                  None, ctypes.byref(site().c), L.stream(o))
    torch.cuda.synchronize()
    assert rc == -1 and bool((o == -7.).all()), '... and so does the library (PK_EINVAL)'


# ---- switches

def _transformer_step(tr, x, ctx, G, S, n, n_ctx):
    from phenaki_pytorch_amd import _lib as L
    from phenaki_pytorch_amd.train import transformer_train
    for p in tr.parameters():
        p.grad = None
    xc = x.clone().requires_grad_()
    y = transformer_train(tr, xc, S, n, L.BF16X3, context2d=ctx, n_ctx=n_ctx)
    y.backward(G)
    grads = [p.grad.clone() for p in tr.parameters() if p.grad is not None]
    assert len(grads) >= 2 * 3 * 3                                      # per layer: two attentions (to_q, to_kv, to_out, ...) and the feed-forward
    return [y.detach().clone(), xc.grad.clone()] + grads


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(u, v) for u, v in zip(a, b))


# The parent's step accumulates two gradients with float atomicAdd, whose order of additions is not fixed: the token embedding's (pk_embed_bwd) and
# the relative-position table's behind the position-bias MLP (pk_bias_scatter).  With dropout off, two runs of the SAME step already differ in the
# last bits of exactly those gradients, so bit equality cannot be asked of them; they are held to 1e-6 of their scale (f32 sums of a few hundred
# terms in another order: ~sqrt(terms) * 2^-24), every other gradient and the loss to bit equality.  The scale of the position-bias MLP's gradients
# is the largest of them: they are all products of the same atomically summed table gradient, and the last bias's own gradient is a sum that
# cancels to rounding noise (a constant added to every score of a row leaves the softmax unchanged).
ATOMIC_SUMS = ('token_emb.weight', 'pos_bias.net.')


def _assert_reproduced(loss_a, grads_a, loss_b, grads_b):
    assert torch.equal(loss_a, loss_b), 'the same seed must give the same loss bit for bit'
    assert grads_a.keys() == grads_b.keys()
    for k in grads_a:
        tag = next((t for t in ATOMIC_SUMS if t in k), None)
        if tag is not None:
            group = k[:k.index(tag)] + tag
            scale = max(float(v.abs().max()) for kk, v in grads_a.items() if kk.startswith(group))
            err = float((grads_a[k] - grads_b[k]).abs().max())
            assert err <= 1e-6 * scale, f'gradient {k} (atomic sum) under the same seed: {err:.3e} > 1e-6 * {scale:.3e}'
        else:
            assert torch.equal(grads_a[k], grads_b[k]), f'gradient {k} differs between two runs under the same seed'


def test_train_eval_and_reseed_switches():
    """a Transformer (self-attention, cross-attention, feed-forward; two layers) with attn_dropout = ff_dropout = 0.25: in eval mode under autograd the
    output and every gradient are bit-identical to the same weights built with p = 0 (and the generator is not touched); in training mode they
    differ; two consecutive calls differ; reseeding reproduces the first call bit for bit; every site of every layer takes its own stream"""
    import phenaki_pytorch_amd as P
    S, n, n_ctx, Dm = 2, 40, 6, 128
    kw = dict(dim=Dm, depth=2, heads=2, dim_context=96, has_cross_attn=True)
    torch.manual_seed(5)
    tr0 = P.attention.Transformer(**kw).cuda()
    trd = P.attention.Transformer(attn_dropout=0.25, ff_dropout=0.25, **kw).cuda()
    trd.load_state_dict(tr0.state_dict())
    g = torch.Generator().manual_seed(6)
    x, G, ctx = torch.randn(S * n, Dm, generator=g).cuda(), torch.randn(S * n, Dm, generator=g).cuda(), torch.randn(S * n_ctx, 96, generator=g).cuda()
    torch.manual_seed(SEED)
    base = _transformer_step(tr0, x, ctx, G, S, n, n_ctx)
    assert _generator_state() == (SEED, 0), 'p = 0 must not touch the generator'
    trd.eval()
    assert _same(_transformer_step(trd, x, ctx, G, S, n, n_ctx), base), 'eval mode under autograd must make exactly the p = 0 calls'
    assert _generator_state() == (SEED, 0)
    trd.train()
    first = _transformer_step(trd, x, ctx, G, S, n, n_ctx)
    assert _generator_state() == (SEED, 4 * 3 * 2), 'two layers x (self-attention, cross-attention, feed-forward) sites'
    assert not torch.equal(first[0], base[0]) and not torch.equal(first[1], base[1])
    assert all(torch.isfinite(t).all() for t in first)
    second = _transformer_step(trd, x, ctx, G, S, n, n_ctx)
    assert not torch.equal(second[0], first[0]), 'consecutive calls draw new masks'
    torch.manual_seed(SEED)
    again = _transformer_step(trd, x, ctx, G, S, n, n_ctx)
    assert _same(again, first), 'torch.manual_seed must reproduce the step bit for bit'


def test_second_order_attention_refuses_dropout():
    """the gradient-penalty path of the discriminator's attention has no dropout: a clear error if p > 0 reaches it in training mode"""
    import phenaki_pytorch_amd as P
    from phenaki_pytorch_amd import _lib as L
    from phenaki_pytorch_amd.discriminator import _attention_second_order
    attn = P.attention.Attention(dim=64, heads=1, num_null_kv=0, dropout=0.25).cuda()
    x = torch.randn(2 * 16, 64, device='cuda', requires_grad=True)
    with pytest.raises(NotImplementedError, match='dropout'):
        _attention_second_order(attn, x, 2, 16, L.F32)


# ---- whole steps

def _phenaki(dropout):
    import phenaki_pytorch_amd as P
    cv_sd, mg_sd, cr_sd = state_dicts('tiny')
    kw = dict(attn_dropout=dropout, ff_dropout=dropout)
    cv = P.CViViT(use_vgg_and_gan=False, **TINY['cvivit'])
    mg = P.MaskGit(**TINY['maskgit'], **kw)
    cr = P.TokenCritic(**TINY['critic'], **kw)
    cv.load_state_dict(cv_sd)
    mg.load_state_dict(mg_sd)
    cr.load_state_dict(cr_sd)
    ph = P.Phenaki(cvivit=cv.eval(), maskgit=mg, critic=cr, steps=TINY['steps'], text_embed_dim=TINY['maskgit']['dim_context']).cuda()
    P.set_compute_dtype(ph, 'bf16x3')
    ph.maskgit.train()
    ph.critic.train()
    return ph, mg, cr


def test_phenaki_training_step_with_dropout():
    """loss = phenaki(ids, text_embeds); loss.backward() with MaskGit and TokenCritic built with attn_dropout = ff_dropout = 0.1 (the tiny
    configuration): it completes, every gradient is finite, the loss differs from the p = 0 loss on the same draws, and two runs under the same
    torch.manual_seed agree bit for bit (see ATOMIC_SUMS for the two gradients the parent's kernels add up atomically).  (Before dropout reached the training kernels this ended in an AssertionError.)"""
    batch, n = 2, 48
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, TINY['maskgit']['num_tokens'], (batch, 3, 4, 4), generator=g).cuda()
    ctx = weights.synthetic_context(batch, 6, TINY['maskgit']['dim_context'], seed=3, pad_last=2).cuda()
    draws = dict(rand_step=torch.tensor([1, 3]), perm_noise=weights.uniform_noise((batch, n), 710),
                 gumbel_u=weights.uniform_noise((batch, n, TINY['maskgit']['num_tokens']), 711))

    def step(ph, mg, cr):
        for p in list(mg.parameters()) + list(cr.parameters()):
            p.grad = None
        torch.manual_seed(SEED)
        loss = ph(video_codebook_ids=ids, text_embeds=ctx, _draws=draws)
        loss.backward()
        grads = {k: p.grad.clone() for k, p in list(mg.named_parameters()) + [('critic.' + k, p) for k, p in cr.named_parameters()] if p.grad is not None}
        return loss.detach().clone(), grads

    loss0, _ = step(*_phenaki(0.))
    ph, mg, cr = _phenaki(0.1)
    loss1, g1 = step(ph, mg, cr)
    assert torch.isfinite(loss1) and len(g1) > 20
    assert all(torch.isfinite(v).all() for v in g1.values())
    assert not torch.equal(loss1, loss0), 'dropout must change the loss'
    assert abs(float(loss1) - float(loss0)) < 0.5 * abs(float(loss0)), 'p = 0.1 perturbs the loss, it does not replace it'
    loss2, g2 = step(ph, mg, cr)
    _assert_reproduced(loss1, g1, loss2, g2)


def test_cvivit_training_step_with_dropout():
    """the tokenizer's reconstruction step with all four transformers built with attn_dropout = ff_dropout = 0.1 (spatial: null keys + position
    bias; temporal: causal + ALiBi on short sequences): completes, finite gradients, another loss than p = 0, reproducible under manual_seed"""
    import phenaki_pytorch_amd as P
    cv_sd = state_dicts('tiny')[0]
    H = TINY['cvivit']['image_size']
    video = weights.synthetic_video(2, 5, H, H, seed=8).cuda()

    def build(dropout):
        cv = P.CViViT(use_vgg_and_gan=False, attn_dropout=dropout, ff_dropout=dropout, **TINY['cvivit'])
        cv.load_state_dict(cv_sd)
        cv = cv.cuda().train()
        P.set_compute_dtype(cv, 'bf16x3')
        return cv

    def step(cv):
        for p in cv.parameters():
            p.grad = None
        torch.manual_seed(SEED)
        loss = cv(video)
        loss.backward()
        return loss.detach().clone(), {k: p.grad.clone() for k, p in cv.named_parameters() if p.grad is not None}

    loss0, _ = step(build(0.))
    cv = build(0.1)
    loss1, g1 = step(cv)
    assert torch.isfinite(loss1) and len(g1) > 20
    assert all(torch.isfinite(v).all() for v in g1.values())
    assert not torch.equal(loss1, loss0), 'dropout must change the loss'
    loss2, g2 = step(cv)
    _assert_reproduced(loss1, g1, loss2, g2)
