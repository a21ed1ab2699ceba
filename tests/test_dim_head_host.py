"""Head widths 32 and 128 on the CPU: the constructors and their parameter shapes, which wrappers the general attention route calls
and with which width and buffer sizes (recorder stubs in place of the `_lib` wrappers, so no kernel runs), the oracle's attention
against the reference's own module at those widths (where the reference is present), and the refusal of every training entry
point -- the backward kernels are 64-wide."""
import contextlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import pytest  # noqa: E402
import torch  # noqa: E402

import phenaki_pytorch_amd as P  # noqa: E402
from phenaki_pytorch_amd import _lib as L  # noqa: E402
from phenaki_pytorch_amd import attention as A  # noqa: E402

WIDTHS = (32, 128)
DT = {'f32': L.F32, 'bf16': L.BF16, 'bf16x3': L.BF16X3}
DIM, HEADS, DCTX, NCTX, S = 64, 2, 48, 12, 2
GRID = {9: (3, 3), 64: (8, 8), 200: (2, 10, 10)}
STUBBED = ('gemm', 'layernorm', 'qkv_attn', 'qkv_project', 'q_attn_cached', 'attn_prep', 'attn_fwd', 'attn_small', 'peg', 'cpb_input')
ALLOWED = {'layernorm', 'gemm', 'attn_prep', 'attn_fwd'}


# --------------------------------------------------------------------------- 1. constructors

def _tiny_cvivit(dh):
    return P.CViViT(dim=32, codebook_size=16, image_size=16, patch_size=8, temporal_patch_size=2, spatial_depth=1, temporal_depth=1,
                    dim_head=dh, heads=HEADS, use_vgg_and_gan=False)


def _tiny_maskgit(dh, dim=32):
    return P.MaskGit(dim=dim, num_tokens=16, max_seq_len=32, depth=1, heads=HEADS, dim_head=dh, dim_context=DCTX)


def _check_attention_shapes(sd, prefix, dh, heads, dim, dim_ctx, nnull):
    inner = dh * heads
    assert tuple(sd[prefix + 'null_kv'].shape) == (heads, 2 * nnull, dh)
    assert tuple(sd[prefix + 'q_scale'].shape) == (dh,) and tuple(sd[prefix + 'k_scale'].shape) == (dh,)
    assert tuple(sd[prefix + 'to_q.weight'].shape) == (inner, dim)
    assert tuple(sd[prefix + 'to_kv.weight'].shape) == (2 * inner, dim_ctx)
    assert tuple(sd[prefix + 'to_out.weight'].shape) == (dim, inner)


@pytest.mark.parametrize('dh', WIDTHS)
def test_constructors_take_the_width(dh):
    att = A.Attention(DIM, dim_context=DCTX, dim_head=dh, heads=HEADS, num_null_kv=3)
    _check_attention_shapes(att.state_dict(), '', dh, HEADS, DIM, DCTX, 3)
    tf = A.Transformer(DIM, depth=2, dim_context=DCTX, dim_head=dh, heads=HEADS, has_cross_attn=True, attn_num_null_kv=2)
    sd = tf.state_dict()
    for layer in range(2):
        _check_attention_shapes(sd, f'layers.{layer}.1.', dh, HEADS, DIM, DIM, 0)
        _check_attention_shapes(sd, f'layers.{layer}.2.', dh, HEADS, DIM, DCTX, 2)
    sd = _tiny_cvivit(dh).state_dict()
    for name in ('enc_spatial_transformer', 'enc_temporal_transformer', 'dec_spatial_transformer', 'dec_temporal_transformer'):
        _check_attention_shapes(sd, f'{name}.layers.0.1.', dh, HEADS, 32, 32, 0)
    sd = _tiny_maskgit(dh).state_dict()
    _check_attention_shapes(sd, 'transformer.layers.0.1.', dh, HEADS, 32, 32, 0)
    _check_attention_shapes(sd, 'transformer.layers.0.2.', dh, HEADS, 32, DCTX, 2)
    assert tuple(sd['continuous_pos_bias.net.0.0.weight'].shape) == (dh, 3)          # the position-bias MLP is dim_head wide
    assert tuple(sd['continuous_pos_bias.net.2.weight'].shape) == (HEADS, dh)


def test_other_widths_are_a_value_error():
    for build in (lambda: A.Attention(DIM, dim_head=48), lambda: A.Transformer(DIM, depth=1, dim_head=48), lambda: _tiny_cvivit(48),
                  lambda: _tiny_maskgit(48)):
        with pytest.raises(ValueError) as e:
            build()
        assert all(w in str(e.value) for w in ('32', '64', '128'))


# --------------------------------------------------------------------------- 2. dispatch

@pytest.fixture(scope='module')
def built_lib():
    from phenaki_pytorch_amd import build
    build.build(verbose=False)
    return L.load()                     # pk_attn_pads is host code: the route asks it for the pads


class Recorder:
    def __init__(self):
        self.calls = []

    def stub(self, name):
        def call(*args, **kwargs):
            self.calls.append((name, args, kwargs))
            return kwargs.get('C')
        return call


@contextlib.contextmanager
def recording(rec):
    saved = [(L, k, getattr(L, k)) for k in STUBBED + ('require_device',)] + [(A.ContinuousPositionBias, '_compute', A.ContinuousPositionBias._compute)]
    try:
        for k in STUBBED:
            setattr(L, k, rec.stub(k))
        L.require_device = lambda t, name='tensor': None

        def compute(self, dims):
            n = 1
            for d in dims:
                n *= d
            return torch.zeros(self.net[-1].weight.shape[0], n, n)
        A.ContinuousPositionBias._compute = compute
        with torch.no_grad():
            yield
    finally:
        for obj, k, v in saved:
            setattr(obj, k, v)


def _named(call, names):
    """positional and keyword arguments of a recorded attn_prep / attn_fwd call by parameter name"""
    _, args, kwargs = call
    out = dict(zip(names, args))
    out.update(kwargs)
    return out


PREP_ARGS = ('dtype', 'q', 'kv', 'null_kv', 'q_scale', 'k_scale', 'scale', 'Qp', 'Kp', 'Vt', 'S', 'h', 'nq', 'n_kv', 'nnull')
FWD_ARGS = ('dtype', 'Qp', 'Kp', 'Vt', 'O', 'S', 'h', 'nq', 'n_kv', 'nnull')


def _check_route(rec, dh, n, n_kv, nnull, launches):
    """`launches` attention launches were recorded, each through attn_prep + attn_fwd of the right width and buffer sizes"""
    names = [c[0] for c in rec.calls]
    assert set(names) <= ALLOWED, names
    preps = [_named(c, PREP_ARGS) for c in rec.calls if c[0] == 'attn_prep']
    fwds = [_named(c, FWD_ARGS) for c in rec.calls if c[0] == 'attn_fwd']
    assert len(preps) == len(fwds) == launches
    nq_pad, nk_pad = L.attn_pads(n, n_kv, nnull)
    for p, f in zip(preps, fwds):
        assert p['dim_head'] == dh and f['dim_head'] == dh
        assert f.get('bias_table') is None and f.get('score_bound') is None
        assert p['Qp'].numel() == S * HEADS * nq_pad * dh and p['Qp'] is f['Qp']
        assert f['Kp'].numel() == S * HEADS * nk_pad * dh and f['Vt'].numel() == S * HEADS * nk_pad * dh
        assert f['O'].shape == (S * n, HEADS * dh)
        assert p['q'].shape == (S * n, HEADS * dh)
        assert (p['nq'], p['n_kv'], p['nnull']) == (n, n_kv, nnull) == (f['nq'], f['n_kv'], f['nnull'])
    return preps, fwds


@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('n', [9, 64, 200])
@pytest.mark.parametrize('dh', WIDTHS)
def test_self_attention_with_a_bias_spec_takes_the_general_route(built_lib, dh, n, dt):
    torch.manual_seed(0)
    att = A.Attention(DIM, dim_head=dh, heads=HEADS).eval()
    cpb = A.ContinuousPositionBias(dim=dh, heads=HEADS, num_dims=len(GRID[n]))
    rec = Recorder()
    with recording(rec):
        out = att.run(torch.zeros(S * n, DIM), S, n, DT[dt], attn_bias=cpb.spec(*GRID[n]))
    assert out.shape == (S * n, DIM)
    preps, fwds = _check_route(rec, dh, n, n, 0, 1)
    assert preps[0]['kv'] is not None and preps[0]['kv'].shape == (S * n, 2 * HEADS * dh)
    assert fwds[0]['bias'].shape == (HEADS, n, n)                       # the BiasSpec arrives expanded to the full matrix
    folded = A.ln_fold_enabled(DT[dt])
    q_gemm = [c for c in rec.calls if c[0] == 'gemm'][0]
    assert (q_gemm[2].get('ln') is not None) == folded                  # the folded LayerNorm rides on the q GEMM
    assert ('layernorm' in [c[0] for c in rec.calls]) == (not folded)


@pytest.mark.parametrize('dt', list(DT))
@pytest.mark.parametrize('n', [9, 64, 200])
@pytest.mark.parametrize('dh', WIDTHS)
def test_cross_attention_fills_the_kv_cache_once(built_lib, dh, n, dt):
    torch.manual_seed(0)
    att = A.Attention(DIM, dim_context=DCTX, dim_head=dh, heads=HEADS, num_null_kv=2).eval()
    cache = {}
    kw = dict(context2d=torch.zeros(S * NCTX, DCTX), n_ctx=NCTX, kmask=torch.ones(S, NCTX, dtype=torch.uint8), kv_cache=cache)
    rec = Recorder()
    with recording(rec):
        for _ in range(2):
            att.run(torch.zeros(S * n, DIM), S, n, DT[dt], **kw)
    preps, fwds = _check_route(rec, dh, n, NCTX, 2, 2)
    assert preps[0]['kv'] is not None and preps[0]['Kp'] is not None and preps[0]['Vt'] is not None
    assert preps[1]['kv'] is None and preps[1]['Kp'] is None and preps[1]['Vt'] is None      # the query side only
    assert cache[id(att)][0] is fwds[0]['Kp'] and cache[id(att)][1] is fwds[0]['Vt']
    assert fwds[1]['Kp'] is fwds[0]['Kp'] and fwds[1]['Vt'] is fwds[0]['Vt']
    assert all(f['kmask'] is kw['kmask'] for f in fwds)


def test_width_64_passes_nothing_new(built_lib):
    att = A.Attention(DIM, heads=HEADS, num_null_kv=2, dim_context=DCTX).eval()
    rec = Recorder()
    with recording(rec):
        att.run(torch.zeros(S * 9, DIM), S, 9, L.F32, context2d=torch.zeros(S * NCTX, DCTX), n_ctx=NCTX)
    for c in rec.calls:
        if c[0] in ('attn_prep', 'attn_fwd'):
            assert c[2].get('dim_head', 64) == 64


# --------------------------------------------------------------------------- 3. the oracle against the reference, away from 64

def _ref_case(case, dh):
    from oracle import phenaki_oracle as O
    from oracle import ref_shim, weights
    ref = ref_shim.load().attention
    gen = torch.Generator().manual_seed(100 + dh)
    dim, heads, b, n = 48, 3, 2, 11
    kw, okw = {}, {}
    if case == 'self_null_bias':
        m = ref.Attention(dim=dim, dim_head=dh, heads=heads, num_null_kv=2)
        bias = torch.randn(heads, n, n, generator=gen)
        kw['attn_bias'] = okw['attn_bias'] = bias                        # over the real keys: both pad the null-key columns themselves
    elif case == 'cross_mask':
        m = ref.Attention(dim=dim, dim_context=40, dim_head=dh, heads=heads, num_null_kv=1)
        ctx = torch.randn(b, 7, 40, generator=gen)
        mask = torch.ones(b, 7, dtype=torch.bool)
        mask[1, 3:] = False
        kw.update(context=ctx, mask=mask)
        okw.update(context=ctx, mask=mask)
    else:
        m = ref.Attention(dim=dim, dim_head=dh, heads=heads, causal=True)
    weights.fill_module(m, salt=4)
    m.eval()
    x = torch.randn(b, n, dim, generator=gen)
    sd = {('a.' + k): v for k, v in m.state_dict().items()}
    with torch.no_grad():
        want = m(x, **kw)
        got = O.attention(sd, 'a.', x, heads=heads, causal=case == 'causal', **okw)
    return got, want


@pytest.mark.parametrize('case', ['self_null_bias', 'cross_mask', 'causal'])
@pytest.mark.parametrize('dh', WIDTHS)
def test_oracle_attention_equals_the_reference(dh, case):
    from oracle import ref_shim
    if not ref_shim.available():
        pytest.skip('the reference is not on this machine')
    got, want = _ref_case(case, dh)
    assert got.shape == want.shape
    err = (got - want).abs().max().item() / want.abs().max().item()
    assert err <= 1e-5, f'oracle vs reference at dim_head {dh}, {case}: {err:.3e}'


# --------------------------------------------------------------------------- 4. training is refused before anything launches

def test_training_entry_points_refuse_other_widths():
    with torch.enable_grad():            # (the GPU test modules switch grad mode off for the process when they are collected)
        _training_refusals()


def _training_refusals():
    cv = _tiny_cvivit(32).train()
    with pytest.raises(NotImplementedError, match='dim_head = 64 only'):
        cv(torch.zeros(1, 3, 3, 16, 16))                                     # the tokenizer's training step
    mg = _tiny_maskgit(128)
    ph = P.Phenaki(maskgit=mg, cvivit=_tiny_cvivit(64), steps=2, text_embed_dim=DCTX)
    with pytest.raises(NotImplementedError, match='dim_head = 64 only'):
        ph(video_codebook_ids=torch.zeros(1, 2, 2, 2, dtype=torch.long), text_embeds=torch.zeros(1, 3, DCTX))
    with pytest.raises(NotImplementedError, match='dim_head = 64 only'):
        mg(torch.zeros(1, 8, dtype=torch.long), video_patch_shape=(2, 2, 2), context=torch.zeros(1, 3, DCTX))
    att = A.Attention(DIM, dim_head=32, heads=HEADS)
    rec = Recorder()
    with recording(rec), torch.enable_grad(), pytest.raises(NotImplementedError, match='dim_head = 64 only'):
        att.run(torch.zeros(S * 9, DIM), S, 9, L.F32)
    assert rec.calls == []
    for p in att.parameters():
        p.requires_grad_(False)
    with recording(rec), torch.enable_grad():                                # frozen parameters: inference, whatever the grad mode
        att.run(torch.zeros(S * 9, DIM), S, 9, L.F32)
    assert [c[0] for c in rec.calls][-2:] == ['attn_fwd', 'gemm']
