"""pk_patch_embed, pk_patch_embed_splitk, pk_patch_embed_finish and pk_patch_embed_finish_groups (csrc/patch_embed.hip) held element by element to the
float64 twin of tests/patch_embed_reference.py: every dispatch branch at the smallest shapes that reach it, on a video that is a 16-byte aligned window of a
poisoned allocation (NaN, then +Inf), poisoned operand tails, sentinel-filled outputs with guard rows and slack columns.  On the grid data set `part` and
`stats` must EQUAL float64 and the pass with the integer 64 added to the video must leave the same bytes, under every cache policy that picks a build; every
rand element must sit inside its derived bound.  The finish kernels also run alone on synthetic partials, the pair launch against two single launches bit for
bit; every refused call must leave its outputs at the sentinel; and CViViT._patch_embed is held to the float64 chain of the module's own parameters on each
of its three routes.  The largest error / bound of every case and output goes to the parity record (profiles/patch_embed_parity.txt)."""
import pytest
import torch

from tests import patch_embed_reference as R
from tests.util import record_parity

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
CASES = R.gemm_cases()
FCASES = R.finish_cases()


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    torch.cuda.set_device(0)
    yield


@pytest.fixture(scope='module')
def L():
    from phenaki_pytorch_amd import _lib
    _lib.load()
    saved = _lib.get_cache_policy()
    _lib.set_cache_policy(0)
    yield _lib
    _lib.set_cache_policy(saved)


def _cpu(t):
    torch.cuda.synchronize()
    return {k: v.cpu() for k, v in t.out.items()}


def _finish_single(L, c, t, groups, parts, stats):
    lib = L.load()
    for gi, G in enumerate(groups):
        rc = lib.pk_patch_embed_finish(*R.finish_args(c, t, gi, parts[gi], stats[gi], G).values(), L.stream(t.s[0]))
        assert rc == 0, f'{c.name}: pk_patch_embed_finish returned {rc}'


def _launch(L, c, x, p):
    """the buffers the launches of pass p left, on the CPU"""
    t = R.operands(c, x, p, 'cuda')
    lib, st = L.load(), L.stream(t.video)
    if c.kernel == 'fused':
        rc = lib.pk_patch_embed(*R.fused_args(c, t).values(), st)
        assert rc == 0, f'{c.name}: pk_patch_embed returned {rc}'
        return _cpu(t)
    saved = L.get_cache_policy()
    L.set_cache_policy(L.cache_policy_mask(**R.POLICIES[c.pol]))
    try:
        a = R.splitk_args(c, t)
        rc = lib.pk_patch_embed_splitk(*a.values(), st)
    finally:
        L.set_cache_policy(saved)
    assert rc == 0, f'{c.name}: pk_patch_embed_splitk returned {rc}'
    _finish_single(L, c, t, c.groups, [a[f'part{gi}'] for gi in range(len(c.groups))], [a[f'stats{gi}'] for gi in range(len(c.groups))])
    return _cpu(t)


def _same_bytes(a, b):
    return all(torch.equal(R._bits(a[k]), R._bits(b[k])) for k in a)


@pytest.mark.parametrize('c', CASES, ids=[c.name for c in CASES])
def test_patch_embed_parity(L, c):
    x = R.build(c)
    first = None
    for p in range(2):
        ref = R.reference(c, x, p)
        out = _launch(L, c, x, p)
        got = R.check(c, ref, out, f'{c.name} (pass {p}, poison {R.POISONS[p]})')
        for name, ratio in got.items():
            record_parity('patch_embed_parity/gpu', dict(branch=R.branch_of(c), case=c.name, out=name, passno=p, err_over_bound=ratio))
        if c.data == 'grid':
            if first is None:
                first = out
            else:
                assert _same_bytes(first, out), f'{c.name}: adding the integer 64 to the video changed the output bytes'


def test_grid_values_do_not_depend_on_the_policy(L):
    """the four builds of the split-K kernel leave the same bytes on the exact data set"""
    by = {c.name: c for c in CASES}
    for base in R._POLICY_BASE:
        outs = []
        for pol in R.POLICIES:
            c = by[f'{base}/grid' + ('' if pol == 'plain/plain' else '/' + pol.replace('/', '+'))]
            outs.append(_launch(L, c, R.build(c), 0))
        assert all(_same_bytes(outs[0], o) for o in outs[1:]), base


@pytest.mark.parametrize('c', FCASES, ids=[c.name for c in FCASES])
def test_finish_alone(L, c):
    x = R.build_finish(c)
    ref = R.reference_finish(c, x)
    outs = []
    for p in range(2):
        t = R.operands(c, x, p, 'cuda')
        _finish_single(L, c, t, c.g, [a.data_ptr() for a in t.part], [a.data_ptr() for a in t.stats])
        out = _cpu(t)
        for name, ratio in R.check(c, ref, out, f'{c.name} (single launches, poison {R.POISONS[p]})').items():
            record_parity('patch_embed_parity/gpu', dict(branch=R.branch_of(c), case=c.name, out=name, passno=p, err_over_bound=ratio))
        outs.append(out)
        # the same groups in ONE launch (pk_patch_embed_finish_groups): bit for bit
        t = R.operands(c, x, p, 'cuda')
        b = R.blank(c)
        L.patch_embed_finish_groups([(t.part[gi], t.stats[gi], G.K, t.s[gi][:c.N], t.t[gi][:c.N], R.EPS1, t.g2[gi][:c.N], t.b2[gi][:c.N], R.EPS2, G.remap)
                                     for gi, G in enumerate(c.g)],
                                    out2=R.window(t.out['tok'], b['tok']) if 'tok' in b else None, out=R.window(t.out['tok_t'], b['tok_t']) if 'tok_t' in b else None)
        one = _cpu(t)
        R.check(c, ref, one, f'{c.name} (one launch)')
        assert _same_bytes(out, one), f'{c.name}: the group launch differs from the single launches'
    assert _same_bytes(outs[0], outs[1]), f'{c.name}: the NaN- and the +Inf-poisoned pass leave different bytes'


def _untouched(t, what):
    torch.cuda.synchronize()
    for name, full in t.out.items():
        sent = torch.full((1,), R.SENT16 if full.dtype == torch.bfloat16 else R.SENT32, dtype=full.dtype)
        assert bool((R._bits(full.cpu()) == R._bits(sent)).all()), f'{what}: a refused call wrote to {name}'


@pytest.mark.parametrize('label,entry,err,change', R.REFUSALS, ids=[r[0] for r in R.REFUSALS])
def test_refusals(L, label, entry, err, change):
    """only rejected calls are made: each returns its error before the launch and leaves the outputs at the sentinel"""
    c = R.refusal_base(entry)
    t = R.operands(c, R.build(c), 0, 'cuda')
    a = R.fused_args(c, t) if entry == 'fused' else R.splitk_args(c, t)
    before = dict(a)
    change(a)
    assert a != before, label
    fn = L.load().pk_patch_embed if entry == 'fused' else L.load().pk_patch_embed_splitk
    assert fn(*a.values(), L.stream(t.video)) == err, label
    _untouched(t, label)


@pytest.mark.parametrize('label,err,change', R.FINISH_REFUSALS, ids=[r[0] for r in R.FINISH_REFUSALS])
def test_finish_refusals(L, label, err, change):
    c = R.finish_cases()[2]
    assert c.outs == ('out', 'out2')
    t = R.operands(c, R.build_finish(c), 0, 'cuda')
    a = R.finish_args(c, t, 0, t.part[0].data_ptr(), t.stats[0].data_ptr(), c.g[0])
    change(a)
    assert L.load().pk_patch_embed_finish(*a.values(), L.stream(t.s[0])) == err, label
    _untouched(t, label)
    if err == R.PK_EINVAL:                                    # the same refusal of the group launch, through its wrapper
        g, N = c.g[0], a['N']
        kw = dict(out2=None, out=None) if a['out'] is None else dict(out2=R.window(t.out['tok'], R.blank(c)['tok']), out=R.window(t.out['tok_t'], R.blank(c)['tok_t']))
        vec = [torch.zeros(N, device='cuda') for _ in range(4)]
        part = torch.zeros(g.ns, g.rows, N, device='cuda')
        with pytest.raises(RuntimeError, match='PK_EINVAL'):
            L.patch_embed_finish_groups([(part, t.stats[0], g.K, vec[0], vec[1], R.EPS1, vec[2], vec[3], R.EPS2, (a['remap_in'], a['remap_out'], a['remap_off']))], **kw)
        _untouched(t, label + ' (group launch)')


# ------------------------------------------------------------------------------------------------ the module's routes

def _module(dim, patch=16):
    import phenaki_pytorch_amd as P
    torch.manual_seed(dim)
    cv = P.CViViT(dim=dim, codebook_size=256, image_size=32, patch_size=patch, temporal_patch_size=2, spatial_depth=1, temporal_depth=1, dim_head=32, heads=2,
                  use_vgg_and_gan=False)
    for seq in (cv.to_patch_emb, cv.to_patch_emb_first_frame):          # non-trivial gamma, beta, bias and LayerNorm(dim) parameters
        ln1, lin, ln2 = seq[1], seq[2], seq[3]
        ln1.weight.data = 1 + 0.1 * torch.randn_like(ln1.weight)
        ln1.bias.data = 0.1 * torch.randn_like(ln1.bias)
        lin.bias.data = 0.1 * torch.randn_like(lin.bias)
        ln2.weight.data = 1 + 0.1 * torch.randn_like(ln2.weight)
        ln2.bias.data = 0.1 * torch.randn_like(ln2.bias)
    cv = cv.cuda().eval()
    P.set_compute_dtype(cv, 'bf16')
    return cv


def _module_reference(cv, video):
    B, C, F, H, W = video.shape
    ph, pw = cv.patch_size
    pt, hw = cv.temporal_patch_size, (H // ph) * (W // pw)
    nt = (F - 1) // pt
    T = 1 + nt
    groups = []
    for seq, f0, ntg, ptg, goff in ((cv.to_patch_emb, 1, nt, pt, hw), (cv.to_patch_emb_first_frame, 0, 1, 1, 0)):
        ln1, lin, ln2 = seq[1], seq[2], seq[3]
        groups.append((f0, ntg, ptg, (ntg * hw, T * hw, goff)) + tuple(v.detach().float().cpu() if torch.is_tensor(v) else v for v in
                      (ln1.weight, ln1.bias, ln1.eps, lin.weight, lin.bias, ln2.weight, ln2.bias, ln2.eps)))
    return R.module_reference(video, groups, ph, pw, B * T * hw)


def _route(cv, video, monkeypatch, **flags):
    import phenaki_pytorch_amd.cvivit as M
    for k, v in flags.items():
        monkeypatch.setattr(M, k, v)
    tokens, T = cv._patch_embed(video.cuda())
    torch.cuda.synchronize()
    tt = cv.__dict__.get('_pk_tokens_t')
    return tokens.cpu(), None if tt is None else tt.cpu()


def _check_tokens(ref, tokens, tokens_t, what):
    assert bool(ref.mapped.all()) and bool(torch.isfinite(tokens).all())
    ratio = ((tokens.double() - ref.ref).abs() / ref.bound).max().item()
    record_parity('patch_embed_parity/gpu', dict(branch='module', case=what, out='tokens', passno=0, err_over_bound=ratio))
    assert ratio <= 1.0, f'{what}: error {ratio:.3f} x the bound'
    if tokens_t is not None:
        assert torch.equal(R._bits(tokens_t), R._bits(tokens.to(torch.bfloat16))), f'{what}: the bf16 token rows are not the RNE of the f32 ones'


def test_module_fold(L):
    """the folded operands themselves (attention.folded_weight, cvivit._pe_bias): Wg = bf16(gamma W) bit for bit, zero-padded; s the row sums of the ROUNDED
    operand and t = W beta + b, each an f32 sum of K terms in an unknown order ((K - 1) 2^-24 sum|.|).  At K = 192 / 384 the row sums of the unrounded
    product lie outside that allowance in some row (0.29 x 2^15 / K^1.5 of it on average: 3.6 / 1.3), so the check tells the two apart."""
    from phenaki_pytorch_amd.attention import folded_weight
    from phenaki_pytorch_amd.cvivit import _pe_bias
    cv = _module(72, patch=8)
    for seq in (cv.to_patch_emb, cv.to_patch_emb_first_frame):
        ln1, lin = seq[1], seq[2]
        wg, s_, t_, _ = folded_weight(lin, 'pe_ln', lambda lin=lin: lin.weight.detach(), ln1.weight, ln1.bias, L.BF16, [lin.weight, ln1.weight, ln1.bias])
        tb = _pe_bias(lin, t_)
        W, gamma, beta, b = (v.detach().float().cpu() for v in (lin.weight, ln1.weight, ln1.bias, lin.bias))
        K = W.shape[1]
        assert K in (192, 384)
        want = (W * gamma[None, :]).to(torch.bfloat16)
        assert torch.equal(R._bits(wg[:, :K].cpu()), R._bits(want)) and not bool(wg[:, K:].any())
        s64, allow = want.double().sum(1), (K - 1) * 2.0 ** -24 * want.double().abs().sum(1)
        assert bool(((s_.cpu().double() - s64).abs() <= allow).all()), 's is not the row sum of the rounded operand'
        assert bool((((W * gamma[None, :]).double().sum(1) - s64).abs() > allow).any()), 'the allowance cannot tell the unrounded row sums apart'
        t64 = W.double() @ beta.double() + b.double()
        allow_t = (K - 1) * 2.0 ** -24 * (W.double().abs() @ beta.double().abs()) + R.U1 * t64.abs()
        assert bool(((tb.cpu().double() - t64).abs() <= allow_t).all()), 't is not W beta + b'


@pytest.mark.parametrize('dim', [72, 520])
def test_module_routes(L, monkeypatch, dim):
    """CViViT._patch_embed against the float64 chain Rearrange -> LayerNorm(P) -> Linear -> LayerNorm(dim) of the module's own parameters: the host-side
    fold (Wg = bf16(gamma W), s from the rounded operand, t = W beta + b) on every route"""
    cv = _module(dim)
    video = torch.randn(2, 3, 5, 32, 32, generator=torch.Generator().manual_seed(7)) * 0.5 + 0.3
    ref = _module_reference(cv, video)
    if dim <= 512:
        pair = _route(cv, video, monkeypatch, _PATCH_FUSED=True, _PATCH_WIDE=True, _PATCH_FINISH_ONE=True)
        _check_tokens(ref, *pair, f'dim{dim}/splitk+pair')
        single = _route(cv, video, monkeypatch, _PATCH_FUSED=True, _PATCH_WIDE=True, _PATCH_FINISH_ONE=False)
        _check_tokens(ref, *single, f'dim{dim}/splitk+single')
        assert torch.equal(R._bits(pair[0]), R._bits(single[0])) and torch.equal(R._bits(pair[1]), R._bits(single[1])), 'the two split-K routes differ'
        _check_tokens(ref, *_route(cv, video, monkeypatch, _PATCH_FUSED=True, _PATCH_WIDE=False, _PATCH_FINISH_ONE=True), f'dim{dim}/fused+layernorm')
    else:                                                     # dim > 512: the 128 x 128 fused kernel + pk_layernorm whatever _PATCH_WIDE says
        _check_tokens(ref, *_route(cv, video, monkeypatch, _PATCH_FUSED=True, _PATCH_WIDE=True, _PATCH_FINISH_ONE=True), f'dim{dim}/fused+layernorm')
