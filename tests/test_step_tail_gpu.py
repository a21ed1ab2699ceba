"""GPU tests of the step tail (csrc/step_tail.hip, the scaled AdamW instantiations of csrc/train.hip, phenaki_pytorch_amd/step_tail.py): the global
gradient norm and clip against torch.nn.utils.clip_grad_norm_, the fused clipped update against clip-then-update bit for bit, and the EMA of a
model's weights against tests/step_tail_restatement.py (ema_pytorch's schedule restated from memory: upstream parity unpinned)."""
import copy

import pytest
import torch
from torch import nn

from oracle import phenaki_oracle as O
from oracle import weights
from oracle.configs import TINY, oracle_cfgs, state_dicts
from tests.step_tail_restatement import EmaRestatement, decay_closed_form, global_norm64
from tests.util import close, load_product

pytestmark = pytest.mark.gpu

# the packing of csrc/step_tail.hip: 2048-element chunks below 256 Ki elements; above, 1024-element chunks for the in-place scale / EMA and
# 8192-element chunks for the norm pass.  Sizes at chunk - 1, chunk, chunk + 1 of each, and both sides of the small / large threshold
SMALL_CHUNK, BIG_MIN, BIG_CHUNK, SUMSQ_BIG_CHUNK = 2048, 262144, 1024, 8192
# the tensor list of test_hip_adamw_matches_torch_adamw_and_bumps_versions: 45 small vectors (two launches), six 98-chunk tensors (a tensor split
# across launches), one matrix above the large-tensor threshold, odd sizes
ADAMW_SHAPES = [(33, 17), (129,), (4, 3, 3), (100, 90), (5000,), (7, 3), (1,)] + [(64,)] * 45 + [(200000,)] * 6 + [(600, 500)]
EDGE_SHAPES = [(1,), (8, 0, 64), (SMALL_CHUNK - 1,), (SMALL_CHUNK,), (SMALL_CHUNK + 1,), (BIG_MIN - 1,), (BIG_MIN,), (BIG_MIN + 1,),
               (BIG_MIN + BIG_CHUNK - 1,), (BIG_MIN + BIG_CHUNK + 1,), (BIG_MIN + SUMSQ_BIG_CHUNK - 1,), (BIG_MIN + SUMSQ_BIG_CHUNK,), (BIG_MIN + SUMSQ_BIG_CHUNK + 1,)]


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    torch.cuda.set_device(0)
    with torch.enable_grad():                      # other test modules switch grad mode off process-wide at import
        yield


def _params_with_grads(shapes, seed, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    ps = [nn.Parameter(torch.randn(*s, generator=g).cuda()) for s in shapes]
    for p, s in zip(ps, shapes):
        p.grad = (scale * torch.randn(*s, generator=g)).cuda()
    return ps


def test_norm_and_inplace_clip_match_torch():
    import phenaki_pytorch_amd as P
    from phenaki_pytorch_amd import _lib as L
    ps = _params_with_grads(ADAMW_SHAPES + EDGE_SHAPES, seed=11)
    ps.append(nn.Parameter(torch.randn(50).cuda()))                      # a parameter without a gradient
    orig = [None if p.grad is None else p.grad.clone() for p in ps]
    want = global_norm64([g for g in orig if g is not None])
    for max_norm in (0.5, 10 * want):
        for p, g in zip(ps, orig):
            p.grad = None if g is None else g.clone()
        v0 = [None if p.grad is None else p.grad._version for p in ps]
        norm = P.clip_grad_norm_(ps, max_norm)
        assert norm.shape == () and norm.dtype == torch.float32 and norm.is_cuda
        print(f'max_norm {max_norm}: norm {float(norm)!r} vs float64 {want!r} (rel {abs(float(norm) - want) / want:.2e})')
        assert abs(float(norm) - want) <= 1e-5 * want
        # the device's own coefficient: the norm pass alone on the same inputs (bit-reproducible), one f32 division of max_norm by norm + 1e-6
        _, out = L.grad_norm_coef([g for g in orig if g is not None and g.numel()], max_norm, norm.device)
        assert torch.equal(out[0], norm)
        coef = out[1]
        exact = min(max_norm / (float(norm) + 1e-6), 1.0)
        assert abs(float(coef) - exact) <= 2.0 ** -22 * exact, 'coef is min(max_norm / (norm + 1e-6), 1) to f32 rounding'
        if max_norm > want:
            assert float(coef) == 1.0
        else:
            assert float(coef) < 1.0
        for i, (p, g) in enumerate(zip(ps, orig)):
            if g is None:
                assert p.grad is None
                continue
            assert torch.equal(p.grad, torch.mul(g, coef)), f'gradient {i} {tuple(g.shape)} is not g * coef bit for bit (max_norm {max_norm})'
            if max_norm > want:
                assert torch.equal(p.grad, g), f'gradient {i} changed under a coefficient of 1'
            if g.numel():
                assert p.grad._version > v0[i]
        for p, g in zip(ps, orig):
            p.grad = None if g is None else g.clone()
        again = P.clip_grad_norm_(ps, max_norm)
        assert torch.equal(again, norm), 'two calls on the same inputs must give bit-identical norms'
    # a single parameter, and a generator of parameters
    one = _params_with_grads([(777,)], seed=12)[0]
    g0 = one.grad.clone()
    n1 = P.clip_grad_norm_(one, 1.0)
    assert abs(float(n1) - float(g0.double().norm())) <= 1e-5 * float(g0.double().norm())
    assert torch.equal(one.grad, g0 * L.grad_norm_coef([g0], 1.0, g0.device)[1][1])
    assert float(P.clip_grad_norm_((p for p in [one]), 1e9)) > 0


def test_clip_refuses_what_it_cannot_scale_in_place():
    import phenaki_pytorch_amd as P
    p = nn.Parameter(torch.randn(6, 4).cuda())
    p.grad = torch.randn(4, 6).cuda().t()
    with pytest.raises(RuntimeError, match='strided'):
        P.clip_grad_norm_([p], 1.0)
    q = nn.Parameter(torch.randn(6).cuda().double())
    q.grad = torch.randn(6).cuda().double()
    with pytest.raises(RuntimeError, match='float64'):
        P.clip_grad_norm_([q], 1.0)


@pytest.mark.parametrize('bad', [float('inf'), float('nan')])
def test_non_finite_gradients_behave_as_in_torch(bad):
    import phenaki_pytorch_amd as P
    shapes = [(5,), (3, 4), (70,)]
    ps = _params_with_grads(shapes, seed=13)
    ps[1].grad[1, 2] = bad
    ref = [nn.Parameter(p.detach().cpu().clone()) for p in ps]
    for r, p in zip(ref, ps):
        r.grad = p.grad.cpu().clone()
    want = torch.nn.utils.clip_grad_norm_(ref, 0.5)
    got = P.clip_grad_norm_(ps, 0.5).cpu()
    assert torch.isnan(got) == torch.isnan(want) and (torch.isnan(want) or got == want), f'{got} vs {want}'
    for r, p in zip(ref, ps):
        a, b = p.grad.cpu(), r.grad
        assert torch.equal(torch.isnan(a), torch.isnan(b))
        assert torch.equal(torch.nan_to_num(a, nan=0.0), torch.nan_to_num(b, nan=0.0))


@pytest.mark.parametrize('wd', [1e-2, 0.0])
def test_fused_clipped_update_matches_clip_then_update(wd):
    import phenaki_pytorch_amd as P
    shapes = ADAMW_SHAPES + [(8, 0, 64), (BIG_MIN + 1,)]
    g = torch.Generator().manual_seed(8)
    init = [torch.randn(*s, generator=g) for s in shapes]
    fused_p = [nn.Parameter(t.clone().cuda()) for t in init]
    plain_p = [nn.Parameter(t.clone().cuda()) for t in init]
    ref_p = [nn.Parameter(t.clone()) for t in init]
    c = 0.5
    fused = P.get_optimizer(fused_p, lr=3e-3, wd=wd, max_grad_norm=c)
    plain = P.get_optimizer(plain_p, lr=3e-3, wd=wd)
    if wd == 0:
        ref = torch.optim.Adam(ref_p, lr=3e-3, betas=(0.9, 0.99), eps=1e-8)
    else:
        ref = torch.optim.AdamW([{'params': [p for p in ref_p if p.ndim >= 2]}, {'params': [p for p in ref_p if p.ndim < 2], 'weight_decay': 0}],
                                lr=3e-3, weight_decay=wd, betas=(0.9, 0.99), eps=1e-8)
    assert fused.max_grad_norm == c and plain.max_grad_norm is None
    for it in range(3):
        grads = [torch.randn(*s, generator=g) for s in shapes]
        for a, b, r, gr in zip(fused_p, plain_p, ref_p, grads):
            a.grad, b.grad, r.grad = gr.cuda(), gr.cuda(), gr.clone()
        v0 = [a._version for a in fused_p]
        fused.step()
        norm = P.clip_grad_norm_(plain_p, c)
        plain.step()
        ref_norm = torch.nn.utils.clip_grad_norm_(ref_p, c)
        ref.step()
        assert torch.equal(fused.last_grad_norm, norm) and fused.last_grad_norm.shape == ()
        assert abs(float(norm) - float(ref_norm)) <= 1e-5 * float(ref_norm)
        for i, (a, b, r, gr) in enumerate(zip(fused_p, plain_p, ref_p, grads)):
            assert torch.equal(a.grad.cpu(), gr), f'step {it}: the fused form must leave .grad {i} untouched'
            if a.numel() == 0:
                continue
            assert a._version > v0[i]
            assert torch.equal(a.detach(), b.detach()), f'step {it} wd {wd}: parameter {i} {tuple(a.shape)} differs between fused and unfused'
            for key in ('exp_avg', 'exp_avg_sq'):
                assert torch.equal(fused.state[a][key], plain.state[b][key]), f'step {it} wd {wd}: {key} of parameter {i} differs'
            close(a.detach().cpu(), r.detach(), 1e-5, f'fused clipped adamw step {it} wd {wd} parameter {i}')
            close(b.detach().cpu(), r.detach(), 1e-5, f'unfused clipped adamw step {it} wd {wd} parameter {i}')
    assert list(fused.state_dict()['param_groups'][0]) == list(plain.state_dict()['param_groups'][0])


class _Small(nn.Module):
    def __init__(self):
        super().__init__()
        self.lin = nn.Linear(70, 300)
        self.big = nn.Parameter(torch.randn(520, 512))                   # above the large-tensor threshold
        self.edge = nn.Parameter(torch.randn(SMALL_CHUNK + 1))
        self.empty = nn.Parameter(torch.zeros(4, 0, 8))
        self.register_buffer('stat', torch.randn(5000))
        self.register_buffer('count', torch.arange(7))

    def forward(self, x):
        return self.lin(x)


def _redraw(model, gen):
    with torch.no_grad():
        for t in list(model.parameters()) + list(model.buffers()):
            if t.is_floating_point():
                t.copy_(torch.randn(*t.shape, generator=gen))
            else:
                t.copy_(torch.randint(0, 1000, tuple(t.shape), generator=gen))


def _tensors(model):
    return {**dict(model.named_parameters()), **dict(model.named_buffers())}


def test_ema_matches_the_restatement():
    import phenaki_pytorch_amd as P
    gen = torch.Generator().manual_seed(5)
    model = _Small().cuda()
    kw = dict(beta=0.9999, update_after_step=1, update_every=2)
    ema = P.EMA(model, **kw)
    want = EmaRestatement(_tensors(model), **kw)
    assert not any(p.requires_grad for p in ema.ema_model.parameters())
    decisions = []
    for call in range(8):
        _redraw(model, gen)
        v0 = {k: t._version for k, t in _tensors(ema.ema_model).items()}
        expect = want.update(_tensors(model))
        assert ema.next_decision() == expect
        ema.update()
        decisions.append(expect)
        got = _tensors(ema.ema_model)
        for k, t in got.items():
            if expect == 'skip':
                assert t._version == v0[k]
                continue
            if t.numel():
                assert t._version > v0[k], f'call {call}: {k} was written without a version bump'
            if not t.is_floating_point() or expect == 'copy':
                assert torch.equal(t, _tensors(model)[k]), f'call {call} ({expect}): {k} must equal the online tensor exactly'
            if t.numel():
                close(t, want.ema[k], 1e-5, f'call {call} ({expect}): {k}')
    assert decisions == ['copy', 'skip', 'copy', 'skip', 'lerp', 'skip', 'lerp', 'skip']
    assert ema.step == 8 and ema.initted
    assert ema.current_decay() == decay_closed_form(8, 1)
    fresh = P.EMA(model, **kw)
    fresh.load_state_dict(copy.deepcopy(ema.state_dict()))
    assert (fresh.step, fresh.initted) == (8, True) and fresh.current_decay() == ema.current_decay()
    for k, t in _tensors(fresh.ema_model).items():
        assert torch.equal(t, _tensors(ema.ema_model)[k])
    # the resumed copy takes the same next step
    _redraw(model, gen)
    ema.update(), fresh.update()
    for k, t in _tensors(fresh.ema_model).items():
        assert torch.equal(t, _tensors(ema.ema_model)[k])
    x = torch.randn(3, 70).cuda()
    assert torch.equal(ema(x), ema.ema_model(x))


def _perturb(model, gen, scale=0.05):
    """what training moves: the parameters and the persistent floating-point buffers (not constants such as the ALiBi slopes)"""
    with torch.no_grad():
        for t in model.state_dict().values():
            if t.is_floating_point() and t.numel():
                t.add_((scale * torch.randn(*t.shape, generator=gen)).to(t.device))


@pytest.mark.parametrize('lfq', [True, False])
def test_ema_copy_is_live(lfq):
    """the averaged weights must reach ema_model's forward: its packed-weight caches are keyed on the tensors' versions"""
    import phenaki_pytorch_amd as P
    if lfq:
        cv, _, _, _ = load_product('tiny', TINY)
        make = lambda: P.CViViT(use_vgg_and_gan=False, **TINY['cvivit'])
    else:
        cfg = {**TINY['cvivit'], 'codebook_size': 4096}
        make = lambda: P.CViViT(lookup_free_quantization=False, use_vgg_and_gan=False, **cfg)
        torch.manual_seed(3)
        cv = make().cuda().eval()
    video = weights.synthetic_video(1, 5, 64, 64, seed=0).cuda()
    gen = torch.Generator().manual_seed(17)
    ema = P.EMA(cv, update_after_step=0, update_every=1)
    ema.eval()
    with torch.no_grad():
        first = ema(video, return_recons_only=True).clone()             # packs the copy's weights
        start = {k: v.clone() for k, v in ema.ema_model.state_dict().items()}
        decisions = []
        for _ in range(3):
            _perturb(cv, gen)
            decisions.append(ema.next_decision())
            ema.update()
        assert decisions == ['copy', 'copy', 'lerp']
        sd = ema.ema_model.state_dict()
        moved = [k for k, v in sd.items() if v.is_floating_point() and v.numel() and not torch.equal(v, start[k])]
        assert len(moved) >= 50
        if not lfq:
            assert any('_codebook.embed' in k for k in moved), 'the codebook buffers are averaged too'
        online = cv.state_dict()
        assert any(not torch.equal(sd[k], online[k]) for k in moved), 'the last update is an average, not a copy'
        got = ema(video, return_recons_only=True)
        fresh = make()
        fresh.load_state_dict(sd)
        fresh = fresh.cuda().eval()
        want = fresh(video, return_recons_only=True)
    assert (got - first).abs().max() > 1e-4, 'the updates must change the reconstruction'
    assert torch.equal(got, want), 'ema_model ran on stale packed weights'


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
def test_training_loop_with_clipping_tracks_the_oracle(dtype):
    """the four-step loop of test_training_loop_tracks_torch_adamw_on_the_oracle with max_grad_norm = 0.5 (the tokenizer trainer's default) on the
    product and torch.nn.utils.clip_grad_norm_ on the oracle: every step clips by a factor of 4 to 8 (oracle norms 3.97, 1.96, 2.05, 2.34).
    Adam is nearly invariant to the gradient's scale, so the parameters alone would hardly notice a missing clip: the norm is the sharp check."""
    import phenaki_pytorch_amd as P
    cv, mg, cr, ph = load_product('tiny', TINY, dtype=dtype)
    _, mg_sd, cr_sd = state_dicts('tiny')
    _, mgc, crc = oracle_cfgs(TINY)
    leaf = lambda sd: {k: (v.clone().requires_grad_() if v.is_floating_point() and not k.endswith('.beta') else v) for k, v in sd.items()}
    mgl, crl = leaf(mg_sd), leaf(cr_sd)
    b, shape, n = 2, (3, 4, 4), 48
    g = torch.Generator().manual_seed(21)
    ids = torch.randint(0, TINY['maskgit']['num_tokens'], (b, *shape), generator=g)
    ctx = weights.synthetic_context(b, 6, TINY['maskgit']['dim_context'], seed=3, pad_last=2)
    hip_params = [p for p in list(mg.parameters()) + list(cr.parameters())]
    opt = P.get_optimizer(hip_params, lr=2e-3, wd=1e-2, max_grad_norm=0.5)
    ref_params = [v for sd in (mgl, crl) for v in sd.values() if v.requires_grad]
    ref_opt = torch.optim.AdamW([{'params': [p for p in ref_params if p.ndim >= 2]}, {'params': [p for p in ref_params if p.ndim < 2], 'weight_decay': 0}],
                                lr=2e-3, weight_decay=1e-2, betas=(0.9, 0.99), eps=1e-8)
    for it in range(4):
        draws = dict(rand_step=torch.tensor([1 + it, 3]), perm_noise=weights.uniform_noise((b, n), 720 + it),
                     gumbel_u=weights.uniform_noise((b, n, TINY['maskgit']['num_tokens']), 730 + it))
        opt.zero_grad(set_to_none=True)
        loss = ph(video_codebook_ids=ids.cuda(), text_embeds=ctx.cuda(), _draws=draws)
        loss.backward()
        opt.step()
        ref_opt.zero_grad(set_to_none=True)
        ref = O.phenaki_forward_loss(mgl, mgc, crl, crc, ids.flatten(1), patch_shape=shape, context=ctx, steps=TINY['steps'],
                                     mask_id=TINY['maskgit']['num_tokens'], **draws)['loss']
        ref.backward()
        ref_norm = float(torch.nn.utils.clip_grad_norm_([p for p in ref_params if p.grad is not None], 0.5))
        ref_opt.step()
        got_norm = float(opt.last_grad_norm)
        print(f'{dtype} step {it}: loss {float(loss.detach()):.6f} vs {float(ref.detach()):.6f}, norm {got_norm:.6f} vs {ref_norm:.6f}')
        assert ref_norm > 0.5, 'every step of this loop clips'
        assert abs(float(loss.detach()) - float(ref.detach())) <= 2e-3 * abs(float(ref.detach())), f'step {it}: {float(loss.detach())} vs {float(ref.detach())}'
        assert abs(got_norm - ref_norm) <= 2e-3 * ref_norm, f'step {it}: gradient norm {got_norm} vs {ref_norm}'
    for net, mod, sd in (('maskgit', mg, mgl), ('critic', cr, crl)):
        for k, v in mod.named_parameters():
            if v.numel() == 0 or not sd[k].requires_grad or sd[k].grad is None or k.endswith('continuous_pos_bias.net.2.bias'):
                continue
            got, want_p = v.detach().cpu(), sd[k].detach()
            if dtype == 'fp32':
                close(got, want_p, 2e-3, f'{net}.{k} after 4 clipped AdamW steps')
            else:
                # the bounds of the unclipped loop for split-bf16: no element more than three steps (lr) off, the tensor within 3e-3 rms
                d = (got - want_p)
                assert float(d.abs().max()) <= 3 * 2e-3, f'{net}.{k}: an element is more than three AdamW steps (lr) off'
                rel = float(d.pow(2).mean().sqrt() / want_p.pow(2).mean().sqrt().clamp_min(1e-12))
                assert rel <= 3e-3, f'{net}.{k} after 4 clipped AdamW steps: rms error {rel:.2e}'
