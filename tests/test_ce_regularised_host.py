"""tests/ce_regularised_restatement.py on its own, no kernel launched: (1) the restated loss and gradient against float64 autograd of
F.cross_entropy(z, t, label_smoothing=eps) + zeta mean(logsumexp(z)^2); (2) every checker of tests/test_ce_regularised_gpu.py fed its own reference with ONE
planted error and required to raise for that reason; (3) the argument checks and the declarations that need no GPU."""
import os
import re

import pytest
import torch

from tests import ce_regularised_restatement as S
from tests import train_glue_reference as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = float('nan')


@pytest.fixture(autouse=True)
def _grad():
    """other modules of the suite switch autograd off for the process"""
    with torch.enable_grad():
        yield


def same64(a, b, what, rtol=1e-12):
    a, b = a.double(), b.double()
    assert a.shape == b.shape, what
    assert (a - b).abs().max() <= rtol * max(b.abs().max().item(), 1e-300), f'{what}: {(a - b).abs().max().item():.3e} apart'


def _logits(M=23, V=R.V_FULL, seed=0):
    g = R.gen(51, M, V, seed)
    return torch.randn(M, V, generator=g, dtype=torch.float64) * 3, torch.randint(0, V, (M,), generator=g)


# ------------------------------------------------------------------------------------------------ the restatement is the definition

@pytest.mark.parametrize('eps,zeta', S.REGS)
def test_restated_loss_and_gradient_are_autograd_of_the_definition(eps, zeta):
    z, t = _logits()
    x = z.clone().requires_grad_(True)
    want = S.autograd_objective(x, t, eps, zeta)
    dz, = torch.autograd.grad(want, x)
    rows, lse = S.loss_rows(z, t, eps, zeta)
    same64(rows.mean(), want.detach(), 'restated loss')
    same64(lse, torch.logsumexp(z, 1), 'restated lse')
    same64(S.grad_logits(z, t, eps, zeta, 1.0 / z.shape[0]), dz, 'restated gradient')
    # the regularisers are not a no-op on these inputs: the plain cross entropy is somewhere else
    assert abs(float(rows.mean()) - float(S.loss_rows(z, t, 0., 0.)[0].mean())) > 1e-3


@pytest.mark.parametrize('eps,zeta', S.REGS)
def test_mean_logit_is_one_dot_product_with_the_column_means(eps, zeta):
    g = R.gen(52)
    A, W, b = torch.randn(9, 40, generator=g), torch.randn(264, 40, generator=g), torch.randn(264, generator=g)
    t = torch.randint(0, 264, (9,), generator=g)
    head, lse = S.loss_rows_head(A, W, b, t, eps, zeta)
    rows, lse2 = S.loss_rows(A.double() @ W.double().t() + b.double(), t, eps, zeta)
    same64(head, rows, 'loss through wbar / bbar')
    same64(lse, lse2, 'lse')


@pytest.mark.parametrize('eps,zeta', S.REGS)
def test_slab_gradients_summed_over_all_slabs_are_the_autograd_gradient(eps, zeta):
    """ce_ref on the slabs of 192 of ce_case's V_FULL = 448 logits, side by side, is d loss / d z of the definition: eps / V is over the WHOLE vocabulary"""
    M = 77
    c = R.ce_case(M, R.V_FULL, 96, 0, use_dev=True)
    full, _ = R.ce_full(M)
    x = full.double().requires_grad_(True)
    e32, z32 = S.f32(eps), S.f32(zeta)
    loss = S.autograd_objective(x, c['targets'], e32, z32) * M * R.f32_scale(c['scale'], c['dev'])
    want, = torch.autograd.grad(loss, x)
    exact = dict(c, lse=torch.logsumexp(full.double(), 1))
    parts = []
    for v0 in range(0, R.V_FULL, 192):
        Vs = min(192, R.V_FULL - v0)
        parts.append(S.ce_ref(dict(exact, Vs=Vs, v0=v0, ld=Vs, logits=c['logits'][:, v0:v0 + Vs].contiguous()), eps, zeta)[0])
    same64(torch.cat(parts, 1), want, 'slab gradients side by side')
    same64(torch.cat(parts, 1), S.grad_logits(full, c['targets'], e32, z32, R.f32_scale(c['scale'], c['dev'])), 'slab gradients against grad_logits')
    # each row sums to scale * 2 zeta lse (softmax sums to 1, the one-hot and the smoothing to (1 - eps) + eps)
    whole = torch.cat(parts, 1)
    row_sums = R.f32_scale(c['scale'], c['dev']) * 2 * z32 * exact['lse']
    assert ((whole.sum(1) - row_sums).abs() <= 1e-12 * whole.abs().sum(1)).all(), 'row sums'


def test_slab_reference_at_zero_is_the_plain_one():
    for M, Vs, ldgt in S.CE_SHAPES:
        c = R.ce_case(M, Vs, ldgt, 192 if Vs > 1 else 0, use_rows=True, use_dev=True)
        assert torch.equal(S.ce_ref(c, 0., 0.)[0], R.ce_ref(c)[0])
        assert (S.ce_ref(c, 0., 0.)[1] >= R.ce_ref(c)[1]).all(), 'the regularised bound only adds roundings'


@pytest.mark.parametrize('eps,zeta', S.REGS)
def test_slab_bound_holds_the_same_expression_in_f32(eps, zeta):
    """the kernel's expression evaluated in f32 on the CPU, every operation rounded once, is inside the derived bound -- and uses a fair share of it"""
    worst = 0.
    for (M, Vs, ldgt), v0 in ((s, v) for s in S.CE_SHAPES for v in (0, 192)):
        c = R.ce_case(M, Vs, ldgt, v0, use_rows=True, use_dev=True)
        ref, bound = S.ce_ref(c, eps, zeta)
        e, z = torch.tensor(eps, dtype=torch.float32), torch.tensor(zeta, dtype=torch.float32)
        lse = c['lse'][:, None]
        onehot = c['row_targets'][:, None] == v0 + torch.arange(Vs)[None]
        inv_v = torch.tensor(1.0, dtype=torch.float32) / R.V_FULL
        g32 = (torch.exp(c['logits'][:, :Vs] - lse) * (1 + 2 * z * lse) - torch.where(onehot, 1 - e, torch.zeros(())) - e * inv_v) \
            * torch.tensor(R.f32_scale(c['scale'], c['dev']), dtype=torch.float32)
        assert g32.dtype == torch.float32
        worst = max(worst, R.assert_within(g32, ref, bound, 'the f32 evaluation against the derived bound'))
    assert 0.02 < worst <= 1.0, f'largest err / bound of the f32 evaluation: {worst:.3f}'


# ------------------------------------------------------------------------------------------------ the checkers, one planted error each

def _ce(v0=192, **k):
    return R.ce_case(77, 100, 96, v0, wide=True, **k)


def test_slab_checker_accepts_the_reference():
    for eps, zeta in S.REGS:
        for dtype in (torch.float32, torch.bfloat16):
            c = _ce(use_rows=True, use_dev=True)
            f32 = S.ce_fake(c, eps, zeta)
            S.ce_check(c, eps, zeta, *S.ce_fake(c, eps, zeta, dtype), f32_out=f32[:2])


def test_slab_checker_planted_errors():
    eps, zeta = 0.1, 1e-2
    c = _ce()
    ref, bound = S.ce_ref(c, eps, zeta)
    g, gT, db = S.ce_fake(c, eps, zeta)
    g[5, 7] = float(ref[5, 7] + 4 * bound[5, 7])
    gT[7, 5] = g[5, 7]
    with pytest.raises(AssertionError, match=r'element \(5, 7\).*beyond its bound'):
        S.ce_check(c, eps, zeta, g, gT, db)
    # the plain gradient (no regulariser at all) is not the regularised one
    with pytest.raises(AssertionError, match='beyond its bound'):
        S.ce_check(c, eps, zeta, *R.ce_fake(c))
    # eps / V over the slab instead of the whole vocabulary
    with pytest.raises(AssertionError, match='beyond its bound'):
        S.ce_check(c, eps, 0., *S.ce_fake(c, eps, 0., ref=S.ce_ref(c, eps, 0., smooth_over=c['Vs'])[0]))
    # the one-hot at v instead of v0 + v
    with pytest.raises(AssertionError, match='beyond its bound'):
        S.ce_check(c, eps, zeta, *S.ce_fake(c, eps, zeta, ref=S.ce_ref(c, eps, zeta, onehot_offset=0)[0]))
    # a full one-hot: (1 - eps) forgotten
    hot = c['row_targets'][:, None] == c['v0'] + torch.arange(c['Vs'])[None]
    with pytest.raises(AssertionError, match='beyond its bound'):
        S.ce_check(c, eps, zeta, *S.ce_fake(c, eps, zeta, ref=ref - hot.double() * eps * R.f32_scale(c['scale'], c['dev'])))
    # 1 + zeta lse instead of 1 + 2 zeta lse
    with pytest.raises(AssertionError, match='beyond its bound'):
        S.ce_check(c, 0., zeta, *S.ce_fake(c, 0., zeta, ref=S.ce_ref(c, 0., zeta / 2)[0]))
    # a pad column of gT that is not zero, a write beyond the slab, a db that is not the column sum
    g, gT, db = S.ce_fake(c, eps, zeta)
    gT[3, c['M'] + 1] = 1e-9
    with pytest.raises(AssertionError, match='pad columns'):
        S.ce_check(c, eps, zeta, g, gT, db)
    g, gT, db = S.ce_fake(c, eps, zeta)
    g[0, c['Vs']] = 0.
    with pytest.raises(AssertionError, match='written outside'):
        S.ce_check(c, eps, zeta, g, gT, db)
    g, gT, db = S.ce_fake(c, eps, zeta)
    db[4] = db[4] + 4 * float(R.sum_bound(g[:, 4].double().abs().sum(), c['M']))
    with pytest.raises(AssertionError, match='db'):
        S.ce_check(c, eps, zeta, g, gT, db)
    # bf16 output that is not the rounding of the f32 output
    f32 = S.ce_fake(c, eps, zeta)
    g, gT, db = S.ce_fake(c, eps, zeta, torch.bfloat16)
    g[2, 2] = g[2, 2] * 1.01
    gT[2, 2] = g[2, 2]
    with pytest.raises(AssertionError, match='bit for bit'):
        S.ce_check(c, eps, zeta, g, gT, db, f32_out=f32[:2])


def _wmean_fake(c, pad=3):
    (wr, _), (br, _) = S.wmean_ref(c)
    wbar, bbar = torch.full((c['D'] + pad,), NAN), torch.full((1 + pad,), NAN)
    wbar[:c['D']] = wr.float()
    bbar[:1] = br.float()
    return wbar, bbar


@pytest.mark.parametrize('mode', S.MODES)
def test_weight_mean_checker_accepts_the_reference_and_sees_planted_errors(mode):
    c = S.wmean_case(264, 40, mode)
    S.wmean_check(c, *_wmean_fake(c))
    (wr, wb), (br, bb) = S.wmean_ref(c)
    wbar, bbar = _wmean_fake(c)
    wbar[11] = float(wr[11] + 4 * wb[11])
    with pytest.raises(AssertionError, match=r'wbar: element \(11,\).*beyond its bound'):
        S.wmean_check(c, wbar, bbar)
    wbar, bbar = _wmean_fake(c)
    bbar[0] = float(br[0] + 4 * bb[0])
    with pytest.raises(AssertionError, match='bbar.*beyond its bound'):
        S.wmean_check(c, wbar, bbar)
    wbar, bbar = _wmean_fake(c)
    wbar[c['D']] = 0.
    with pytest.raises(AssertionError, match='written outside'):
        S.wmean_check(c, wbar, bbar)
    # a sum that was not divided by V; a mean over V - 1 rows
    wbar, bbar = _wmean_fake(c)
    with pytest.raises(AssertionError, match='beyond its bound'):
        S.wmean_check(c, torch.cat((wbar[:c['D']] * c['V'], wbar[c['D']:])), bbar)
    with pytest.raises(AssertionError, match='beyond its bound'):
        S.wmean_check(c, torch.cat((c['img'][:-1].mean(0).float(), wbar[c['D']:])), bbar)
    if mode == 'bf16':
        # the mean of the UNROUNDED weights is not the mean of the image the head multiplies
        with pytest.raises(AssertionError, match='beyond its bound'):
            S.wmean_check(c, torch.cat((c['W'].double().mean(0).float(), wbar[c['D']:])), bbar)


@pytest.mark.parametrize('mode', S.MODES)
def test_loss_checker_accepts_the_reference_and_sees_a_missing_term(mode):
    g = R.gen(53)
    A, W, b = torch.randn(70, 96, generator=g), torch.randn(1000, 96, generator=g) / 96 ** 0.5 * 3 + 0.2, torch.randn(1000, generator=g) * 0.1 + 0.5
    t = torch.randint(0, 1000, (70,), generator=g)
    A64, W64 = S.rounded_operands(mode, A, W)
    for eps, zeta in S.REGS:
        ref, lse = S.loss_rows_head(A64, W64, b, t, eps, zeta)
        S.check_loss(mode, ref.float(), lse.float(), ref, lse, 'exact')
        plain, _ = S.loss_rows_head(A64, W64, b, t, 0., 0.)
        with pytest.raises(AssertionError, match='loss'):
            S.check_loss(mode, plain.float(), lse.float(), ref, lse, 'the plain loss')
        if eps > 0:
            # smoothing without the mean-logit term, and the bias mean forgotten
            z = A64 @ W64.t() + b.double()
            with pytest.raises(AssertionError, match='loss'):
                S.check_loss(mode, (ref + eps * z.mean(1)).float(), lse.float(), ref, lse, 'no zbar')
            with pytest.raises(AssertionError, match='loss'):
                S.check_loss(mode, (ref + eps * b.double().mean()).float(), lse.float(), ref, lse, 'no bbar')


def test_autograd_checker_accepts_the_reference_and_sees_planted_errors():
    c = S.autograd_case()
    ref = S.autograd_ref(c, 0.1, 1e-2)
    f = lambda k: ref[k].float()
    S.autograd_check(c, ref, 'fp32', ref['loss'], f('dE'), f('dW'), f('db'))
    with pytest.raises(AssertionError, match='loss'):
        S.autograd_check(c, ref, 'fp32', ref['loss'] * 1.01, f('dE'), f('dW'), f('db'))
    with pytest.raises(AssertionError, match='db'):
        S.autograd_check(c, ref, 'fp32', ref['loss'], f('dE'), f('dW'), f('db') + 0.1 * S.AG['upstream'] / S.AG['V'])       # the -eps / V of db forgotten
    with pytest.raises(AssertionError, match='dW'):
        S.autograd_check(c, ref, 'fp32', ref['loss'], f('dE'), S.autograd_ref(c, 0.1, 0.)['dW'].float(), f('db'))
    with pytest.raises(AssertionError, match='dE'):
        S.autograd_check(c, ref, 'fp32', ref['loss'], f('dE') / S.AG['upstream'], f('dW'), f('db'))                        # the upstream gradient dropped
    dE = f('dE').clone()
    rest = torch.ones(S.AG['R'], dtype=torch.bool)
    rest[c['rows'].long()] = False
    dE[rest.nonzero()[0, 0], 3] = 1e-12
    with pytest.raises(AssertionError, match='exactly zero'):
        S.autograd_check(c, ref, 'fp32', ref['loss'], dE, f('dW'), f('db'))


def test_same_step_checker_is_bitwise_except_for_the_two_atomic_sums():
    g = R.gen(54)
    grads = {'maskgit.to_logits.weight': torch.randn(8, 4, generator=g), 'maskgit.token_emb.weight': torch.randn(9, 4, generator=g),
             'maskgit.continuous_pos_bias.net.0.0.weight': torch.randn(4, 3, generator=g), 'maskgit.unused': None}
    loss = torch.tensor(7.25)
    clone = lambda: {k: (None if v is None else v.clone()) for k, v in grads.items()}
    assert S.assert_same_step(loss, clone(), loss.clone(), grads, 'same') == 2
    other = clone()
    other['maskgit.token_emb.weight'][3, 1] += 2e-7                           # a last bit of an atomic sum: allowed
    S.assert_same_step(loss, other, loss, grads, 'atomic order')
    other['maskgit.token_emb.weight'][3, 1] += 1e-4
    with pytest.raises(AssertionError, match='atomic sum'):
        S.assert_same_step(loss, other, loss, grads, 'atomic sum off')
    other = clone()
    w = other['maskgit.to_logits.weight']
    w[2, 2] = torch.nextafter(w[2, 2], torch.tensor(10.))                     # one ulp anywhere else: not allowed
    with pytest.raises(AssertionError, match='bit for bit'):
        S.assert_same_step(loss, other, loss, grads, 'one ulp')
    with pytest.raises(AssertionError, match='bit for bit'):
        S.assert_same_step(torch.nextafter(loss, torch.tensor(10.)), clone(), loss, grads, 'loss')
    other = clone()
    other['maskgit.unused'] = torch.zeros(1)
    with pytest.raises(AssertionError, match='one model only'):
        S.assert_same_step(loss, other, loss, grads, 'extra gradient')


# ------------------------------------------------------------------------------------------------ arguments and declarations

BAD = [dict(label_smoothing=1.), dict(label_smoothing=-0.1), dict(z_loss_weight=-1e-3), dict(label_smoothing=NAN), dict(z_loss_weight=NAN),
       dict(z_loss_weight=float('inf'))]


@pytest.mark.parametrize('bad', BAD, ids=lambda d: '-'.join(f'{k}={v}' for k, v in d.items()))
def test_bad_regularisers_are_refused(bad):
    """before anything touches a device: the public function and the constructor raise ValueError"""
    import phenaki_pytorch_amd as P
    from oracle.configs import TINY
    E, W, t = torch.zeros(8, 8), torch.zeros(8, 8), torch.zeros(8, dtype=torch.long)
    with pytest.raises(ValueError, match='label_smoothing|z_loss_weight'):
        P.vocab_cross_entropy(E, W, None, t, **bad)
    cv = P.CViViT(use_vgg_and_gan=False, **TINY['cvivit'])
    mg = P.MaskGit(**TINY['maskgit'])
    with pytest.raises(ValueError, match='label_smoothing|z_loss_weight'):
        P.Phenaki(maskgit=mg, cvivit=cv, text_embed_dim=TINY['maskgit']['dim_context'], **bad)


def test_phenaki_defaults_are_off():
    import phenaki_pytorch_amd as P
    from oracle.configs import TINY
    cv = P.CViViT(use_vgg_and_gan=False, **TINY['cvivit'])
    mg = P.MaskGit(**TINY['maskgit'])
    ph = P.Phenaki(maskgit=mg, cvivit=cv, text_embed_dim=TINY['maskgit']['dim_context'])
    assert ph.label_smoothing == 0. and ph.z_loss_weight == 0. and ph.train_cond_drop is False
    on = P.Phenaki(maskgit=mg, cvivit=cv, text_embed_dim=TINY['maskgit']['dim_context'], label_smoothing=0.1, z_loss_weight=1e-2, train_cond_drop=True)
    assert (on.label_smoothing, on.z_loss_weight, on.train_cond_drop) == (0.1, 1e-2, True)
    with pytest.raises(ValueError, match='train_cond_drop'):
        P.Phenaki(maskgit=mg, cvivit=cv, text_embed_dim=TINY['maskgit']['dim_context'], train_cond_drop=0.25)


def test_cond_drop_masks_follow_the_flag_without_a_device():
    """flag off: the text mask itself for both networks, no draw consumed; on: each network ANDs its own (b,) draw"""
    import phenaki_pytorch_amd as P
    from oracle.configs import TINY
    cv = P.CViViT(use_vgg_and_gan=False, **TINY['cvivit'])
    mg = P.MaskGit(**TINY['maskgit'])
    kw = dict(maskgit=mg, cvivit=cv, text_embed_dim=TINY['maskgit']['dim_context'], self_token_critic=True)
    tm = torch.tensor([[True, True, False], [True, False, False]])
    draws = dict(cond_keep=torch.tensor([True, False]), critic_cond_keep=torch.tensor([False, True]))
    off = P.Phenaki(**kw)
    state = torch.get_rng_state()
    a, b = off._cond_drop_masks(tm, None, draws, 2, True)
    assert a is tm and b is tm and torch.equal(torch.get_rng_state(), state)
    on = P.Phenaki(train_cond_drop=True, **kw)
    a, b = on._cond_drop_masks(tm, None, draws, 2, True)
    assert torch.equal(a, tm & torch.tensor([[True], [False]])) and torch.equal(b, tm & torch.tensor([[False], [True]]))
    a, b = on._cond_drop_masks(tm, None, draws, 2, False)                    # generator only: the critic draws nothing
    assert b is tm
    # the argument overrides the constructor's probability (the default() the reference's shadowing cut off): 1 drops everything, 0 nothing
    a, b = on._cond_drop_masks(tm, 1., {}, 2, True)
    assert not a.any() and not b.any()
    a, b = on._cond_drop_masks(tm, 0., {}, 2, True)
    assert a is tm and b is tm
    # own draws: two (b,) uniforms from the generator of the mask's device
    torch.manual_seed(5)
    a, b = on._cond_drop_masks(torch.ones(64, 3, dtype=torch.bool), 0.5, {}, 64, True)
    assert 8 < int(a[:, 0].sum()) < 56 and not torch.equal(a, b)
    assert on._cond_drop_masks(None, None, draws, 2, True) == (None, None)


def test_header_declares_the_three_entry_points():
    text = open(os.path.join(ROOT, 'include', 'phenaki_hip.h')).read()
    for name in ('pk_vocab_weight_mean', 'pk_vocab_ce_reg', 'pk_ce_grad_slab_reg'):
        assert re.search(rf'\bint {name}\(', text), f'{name} is not declared in include/phenaki_hip.h'
    from phenaki_pytorch_amd import _lib as L
    for name in ('pk_vocab_weight_mean', 'pk_vocab_ce_reg', 'pk_ce_grad_slab_reg'):
        assert name in L.SIGNATURES
    assert len(L.SIGNATURES['pk_vocab_ce_reg']) == len(L.SIGNATURES['pk_vocab_ce']) + 4
    assert len(L.SIGNATURES['pk_ce_grad_slab_reg']) == len(L.SIGNATURES['pk_ce_grad_slab']) + 3
