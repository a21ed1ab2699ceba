"""The regularised masked-token objective on the GPU: pk_vocab_weight_mean, pk_vocab_ce_reg and pk_ce_grad_slab_reg against the float64 restatement of
tests/ce_regularised_restatement.py (bounds and tolerances stated there), `vocab_cross_entropy(label_smoothing=, z_loss_weight=)` under autograd, and the whole
training step of Phenaki(label_smoothing=, z_loss_weight=, train_cond_drop=True) against torch autograd through the oracle."""
import itertools

import pytest
import torch
import torch.nn.functional as F

from oracle import phenaki_oracle as O
from oracle import weights
from oracle.configs import TINY, oracle_cfgs, state_dicts
from tests import ce_regularised_restatement as S
from tests import train_glue_reference as R
from tests.util import close, load_product, record_parity

pytestmark = pytest.mark.gpu

NAN = float('nan')
EINVAL = -1


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    torch.cuda.set_device(0)
    with torch.enable_grad():                      # other test modules switch grad mode off process-wide at import
        yield


def dev(t):
    return None if t is None else t.cuda()


def one(v):
    return None if v is None else torch.tensor([v], device='cuda', dtype=torch.float32)


def merge(worst, new):
    for k, v in new.items():
        worst[k] = max(worst.get(k, 0.), v)


def _image(L, mode, W, Kp):
    """the head's operand image of W (V, D): K zero-padded to Kp, bf16 / f32 / split-bf16 planes"""
    dt = {'f32': L.F32, 'bf16': L.BF16, 'bf16x3': L.BF16X3}[mode]
    Wp = torch.zeros(W.shape[0], Kp)
    Wp[:, :W.shape[1]] = W
    Wd = Wp.cuda().to(L.tdtype(dt))
    return dt, (L.split_planes(Wd) if mode == 'bf16x3' else Wd)


# ------------------------------------------------------------------------------------------------ pk_vocab_weight_mean

@pytest.mark.parametrize('mode', S.MODES)
@pytest.mark.parametrize('V,D', S.WMEAN_SHAPES)
def test_vocab_weight_mean(mode, V, D):
    """every element within the any-order summation bound of the float64 mean of the ROUNDED image, two calls bit for bit, nothing written beyond D"""
    from phenaki_pytorch_amd import _lib as L
    c = S.wmean_case(V, D, mode)
    dt, img = _image(L, mode, c['W'], c['Kp'])
    outs = []
    for _ in range(2):
        wbar, bbar = torch.full((D + 5,), NAN, device='cuda'), torch.full((4,), NAN, device='cuda')
        got = L.vocab_weight_mean(dt, img, c['b'].cuda(), V, D, wbar=wbar, bbar=bbar)
        assert got[0] is wbar and got[1] is bbar
        outs.append((wbar.cpu(), bbar.cpu()))
    ratios = S.wmean_check(c, *outs[0])
    R.assert_same_bits(outs[1][0], outs[0][0], 'weight_mean wbar, second call')
    R.assert_same_bits(outs[1][1], outs[0][1], 'weight_mean bbar, second call')
    wb, bb = L.vocab_weight_mean(dt, img, c['b'].cuda(), V, D)                # buffers of its own
    assert wb.shape == (D,) and bb.shape == (1,)
    R.assert_same_bits(wb.cpu(), outs[0][0][:D], 'weight_mean with its own buffers')
    print(f'weight_mean {mode} {V}x{D}: err / bound wbar {ratios["wbar"]:.3f} bbar {ratios["bbar"]:.3f}')
    record_parity('ce_reg_weight_mean', dict(mode=mode, shape=[V, D], err_over_bound=ratios))


def test_vocab_weight_mean_refuses_bad_arguments():
    from phenaki_pytorch_amd import _lib as L
    lib = L.load()
    W, b = torch.zeros(8, 32, device='cuda'), torch.zeros(8, device='cuda')
    wbar, bbar, ws = torch.zeros(8, device='cuda'), torch.zeros(1, device='cuda'), torch.zeros(4096, device='cuda')
    st = L.stream(W)
    call = lambda dtype=0, w=W, ldw=32, bias=b, V=8, D=8, wb=wbar, bb=bbar, work=ws: lib.pk_vocab_weight_mean(
        dtype, L.ptr(w), ldw, L.ptr(bias), V, D, L.ptr(wb), L.ptr(bb), L.ptr(work), st)
    assert call() == 0
    for kw in (dict(dtype=3), dict(w=None), dict(bias=None), dict(wb=None), dict(bb=None), dict(work=None), dict(V=0), dict(D=0), dict(ldw=4)):
        assert call(**kw) == EINVAL, kw
    assert call(D=6) == -2 and call(dtype=1, D=12) == -2 and call(dtype=2, ldw=48, D=8) == -2, 'alignment as the neighbours'
    assert lib.pk_vocab_weight_mean_words(0, 8, 8) > 0 and lib.pk_vocab_weight_mean_words(0, 0, 8) == 0


# ------------------------------------------------------------------------------------------------ pk_vocab_ce_reg

@pytest.mark.parametrize('mode', S.MODES)
@pytest.mark.parametrize('M,V,D,with_rows', [(5, 264, 40, False), (70, 1000, 96, True)])
def test_vocab_ce_reg(mode, M, V, D, with_rows):
    """M not a multiple of the 4 rows per workgroup, a V tail shorter than a 128-column tile, D below one 64-lane sweep: loss and lse against the restatement
    on operands rounded as the mode rounds them, at pk_vocab_ce's tolerances; at eps = zeta = 0 bit-identical to pk_vocab_ce"""
    from phenaki_pytorch_amd import _lib as L
    g = R.gen(61, M, V, D)
    e = torch.randn(M, D, generator=g)
    W = torch.randn(V, D, generator=g) / D ** 0.5 * 3 + torch.linspace(-0.4, 0.4, D)[None]
    b = torch.randn(V, generator=g) * 0.1 + 0.5
    total = 2 * M + 5
    rows = torch.randperm(total, generator=g)[:M].int() if with_rows else None
    targets_full = torch.randint(0, V, (total,), generator=g)
    tg = targets_full[rows.long()] if with_rows else targets_full[:M]
    q = 64 if mode == 'bf16' else 32
    dt, Wd = _image(L, mode, W, (D + q - 1) // q * q)
    A = e.cuda().to(L.tdtype(dt))
    bd, td, rd = b.cuda(), targets_full.cuda(), dev(rows)
    partials = torch.empty(5 * L.vocab_ntiles(V) * M, device='cuda')
    L.vocab_sample(dt, A, Wd, bd, M, V, D, 1.0, None, rd, 7, True, partials)
    wbar, bbar = L.vocab_weight_mean(dt, Wd, bd, V, D)
    A64, W64 = S.rounded_operands(mode, e, W)
    worst = {}
    for eps, zeta in S.REGS:
        loss, lse = torch.full((M,), NAN, device='cuda'), torch.full((M,), NAN, device='cuda')
        L.vocab_ce(dt, partials, M, V, A, Wd, bd, D, td, rd, loss, lse=lse, label_smoothing=eps, z_loss_weight=zeta,
                   wbar=wbar if eps > 0 else None, bbar=bbar if eps > 0 else None)
        ref, ref_lse = S.loss_rows_head(A64, W64, b, tg, S.f32(eps), S.f32(zeta))
        merge(worst, S.check_loss(mode, loss, lse, ref, ref_lse, f'vocab_ce_reg {mode} V={V} eps={eps} zeta={zeta}'))
    # the zero form IS the plain kernel: same bits through either entry point, with or without the means
    plain, plain_lse = torch.full((M,), NAN, device='cuda'), torch.full((M,), NAN, device='cuda')
    L.vocab_ce(dt, partials, M, V, A, Wd, bd, D, td, rd, plain, lse=plain_lse)
    lib = L.load()
    for wb, bb in ((None, None), (wbar, bbar)):
        zl, zs = torch.full((M,), NAN, device='cuda'), torch.full((M,), NAN, device='cuda')
        rc = lib.pk_vocab_ce_reg(dt, L.ptr(partials), M, V, L.ptr(A), A.stride(-2), L.ptr(Wd), Wd.stride(0), L.ptr(bd), D, L.ptr(td), L.ptr(rd), L.ptr(zl), L.ptr(zs),
                                 0., 0., L.ptr(wb), L.ptr(bb), L.stream(A))
        assert rc == 0
        R.assert_same_bits(zl.cpu(), plain.cpu(), 'pk_vocab_ce_reg(0, 0) loss against pk_vocab_ce')
        R.assert_same_bits(zs.cpu(), plain_lse.cpu(), 'pk_vocab_ce_reg(0, 0) lse against pk_vocab_ce')
    print(f'vocab_ce_reg {mode} {M}x{V}x{D}: rel err loss {worst["loss"]:.3e} lse {worst["lse"]:.3e}')
    record_parity('ce_reg_vocab_ce', dict(mode=mode, shape=[M, V, D], rel_err=worst))


def test_ce_reg_entry_points_refuse_bad_arguments():
    """eps outside [0, 1), zeta < 0 or not finite, eps > 0 without the means: PK_EINVAL from both kernels' entry points, nothing launched"""
    from phenaki_pytorch_amd import _lib as L
    lib = L.load()
    M, V, D = 4, 128, 32
    A, W, b = torch.zeros(M, D, device='cuda'), torch.zeros(V, D, device='cuda'), torch.zeros(V, device='cuda')
    t = torch.zeros(M, dtype=torch.long, device='cuda')
    partials = torch.zeros(5 * L.vocab_ntiles(V) * M, device='cuda')
    loss, wbar, bbar = torch.zeros(M, device='cuda'), torch.zeros(D, device='cuda'), torch.zeros(1, device='cuda')
    st = L.stream(A)
    ce = lambda eps, zeta, wb=wbar, bb=bbar: lib.pk_vocab_ce_reg(0, L.ptr(partials), M, V, L.ptr(A), D, L.ptr(W), D, L.ptr(b), D, L.ptr(t), None, L.ptr(loss), None,
                                                                  eps, zeta, L.ptr(wb), L.ptr(bb), st)
    logits, lse = torch.zeros(M, V, device='cuda'), torch.zeros(M, device='cuda')
    g, gT = torch.zeros(M, V, device='cuda'), torch.zeros(V, 32, device='cuda')
    slab = lambda eps, zeta, vt=V: lib.pk_ce_grad_slab_reg(0, L.ptr(logits), V, L.ptr(lse), L.ptr(t), None, M, V, 0, 1.0, None, L.ptr(g), V, L.ptr(gT), 32, None,
                                                           eps, zeta, vt, st)
    assert ce(0.1, 1e-2) == 0 and slab(0.1, 1e-2) == 0 and ce(0., 1e-2, None, None) == 0
    for eps, zeta in ((1., 0.), (-0.1, 0.), (NAN, 0.), (0., -1e-3), (0., NAN), (0., float('inf'))):
        assert ce(eps, zeta) == EINVAL and slab(eps, zeta) == EINVAL, (eps, zeta)
    assert ce(0.1, 0., None, bbar) == EINVAL and ce(0.1, 0., wbar, None) == EINVAL
    assert slab(0.1, 0., V - 1) == EINVAL, 'the slab must lie inside the whole vocabulary'
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ pk_ce_grad_slab_reg

@pytest.mark.parametrize('M,Vs,ldgt', S.CE_SHAPES)
def test_ce_grad_slab_reg(M, Vs, ldgt):
    """ce_case's inputs (targets below, on both edges of, inside and above the slab; rows gather; device scale) x the three (eps, zeta): f32 g within its derived
    bound, bf16 g / gT the rounding of the f32 call bit for bit, pads untouched, db against the stored g; the zero form bit-identical to pk_ce_grad_slab"""
    from phenaki_pytorch_amd import _lib as L
    worst = {}
    for v0, wide, (use_rows, use_dev) in itertools.product((0, 192), (False, True), ((False, False), (True, True))):
        c = R.ce_case(M, Vs, ldgt, v0, wide=wide, use_rows=use_rows, use_dev=use_dev)
        logits, lse, targets, rows, sd = dev(c['logits']), dev(c['lse']), dev(c['targets']), dev(c['rows']), one(c['dev'])
        for eps, zeta in S.REGS:
            f32 = None
            for dtype in (torch.float32, torch.bfloat16):
                g, gT, db = R.ce_buffers(c, dtype, 'cuda')
                L.ce_grad_slab(logits, lse, targets, rows, M, Vs, v0, c['scale'], g, gT, db=db, scale_dev=sd,
                               label_smoothing=eps, z_loss_weight=zeta, V_total=R.V_FULL)
                out = (g.cpu(), gT.cpu(), db.cpu())
                merge(worst, S.ce_check(c, eps, zeta, *out, f32_out=f32))
                if dtype == torch.float32:
                    f32 = out[:2]
        lib = L.load()
        for dtype in (torch.float32, torch.bfloat16):
            g, gT, db = R.ce_buffers(c, dtype, 'cuda')
            L.ce_grad_slab(logits, lse, targets, rows, M, Vs, v0, c['scale'], g, gT, db=db, scale_dev=sd)
            g0, gT0, db0 = R.ce_buffers(c, dtype, 'cuda')
            rc = lib.pk_ce_grad_slab_reg(1 if dtype == torch.bfloat16 else 0, L.ptr(logits), logits.stride(0), L.ptr(lse), L.ptr(targets), L.ptr(rows), M, Vs, v0,
                                         float(c['scale']), L.ptr(sd), L.ptr(g0), g0.stride(0), L.ptr(gT0), gT0.stride(0), L.ptr(db0), 0., 0., R.V_FULL, L.stream(logits))
            assert rc == 0
            for a, b, name in ((g0, g, 'g'), (gT0, gT, 'gT'), (db0, db, 'db')):
                R.assert_same_bits(a.cpu(), b.cpu(), f'pk_ce_grad_slab_reg(0, 0) {name} against pk_ce_grad_slab')
    print(f'ce_grad_slab_reg {M}x{Vs} ldgt {ldgt}: err / bound g {worst["g"]:.3f} db {worst["db"]:.3f}')
    record_parity('ce_reg_grad_slab', dict(shape=[M, Vs, ldgt], err_over_bound=worst))


# ------------------------------------------------------------------------------------------------ vocab_cross_entropy under autograd

@pytest.mark.parametrize('mode', ['fp32', 'bf16x3', 'bf16'])
@pytest.mark.parametrize('slab', [64, 320])
def test_vocab_cross_entropy_regularised_matches_float64_autograd(mode, slab):
    """R = 50 rows, 37 selected, V = 264 (slab 64: four slabs and a short one; 320: one slab), D = 40, bias, upstream gradient 1.7"""
    from phenaki_pytorch_amd.train import vocab_cross_entropy
    c = S.autograd_case()
    for eps, zeta in S.REGS:
        ref = S.autograd_ref(c, eps, zeta, mode)
        E, W, b = (c[k].cuda().requires_grad_() for k in ('E', 'W', 'b'))
        loss = vocab_cross_entropy(E, W, b, c['t'].cuda(), compute_dtype=mode, slab=slab, rows=c['rows'].cuda(), label_smoothing=eps, z_loss_weight=zeta)
        (loss * S.AG['upstream']).backward()
        errs = S.autograd_check(c, ref, mode, loss.detach().cpu(), E.grad.cpu(), W.grad.cpu(), b.grad.cpu())
        record_parity('ce_reg_autograd', dict(mode=mode, slab=slab, eps=eps, zeta=zeta, rel_err=errs))
    # off by default, and the zero keywords are the plain call bit for bit
    outs = []
    for kw in ({}, dict(label_smoothing=0., z_loss_weight=0.)):
        E, W, b = (c[k].cuda().requires_grad_() for k in ('E', 'W', 'b'))
        loss = vocab_cross_entropy(E, W, b, c['t'].cuda(), compute_dtype=mode, slab=slab, rows=c['rows'].cuda(), **kw)
        loss.backward()
        outs.append((loss.detach().cpu().reshape(1), E.grad.cpu(), W.grad.cpu(), b.grad.cpu()))
    for a, bb, name in zip(outs[1], outs[0], ('loss', 'dE', 'dW', 'db')):
        R.assert_same_bits(a, bb, f'vocab_cross_entropy(0, 0) {name} against the call without the keywords')


# ------------------------------------------------------------------------------------------------ the whole step, TINY config

EPS, ZETA = 0.1, 1e-2


def _leaf(sd):
    return {k: (v.clone().requires_grad_() if v.is_floating_point() and not k.endswith('.beta') else v) for k, v in sd.items()}


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('critic_kind', ['token_critic', 'self_critic'])
def test_regularised_training_step_matches_oracle_autograd(critic_kind, dtype):
    """Phenaki(label_smoothing=0.1, z_loss_weight=1e-2, train_cond_drop=True) with injected draws: MaskGit drops the text of sample 1, the critic of sample 0
    (each its own draw).  Reference: the oracle's logits and mask with the dropped sample's context rows zeroed (an all-False text mask is the same
    computation), the loss formed in torch from them and backpropagated through the oracle; the critic likewise on ITS dropped context."""
    import phenaki_pytorch_amd as P
    cv, mg, cr, _ = load_product('tiny', TINY, dtype=dtype)
    _, mg_sd, cr_sd = state_dicts('tiny')
    _, mgc, crc = oracle_cfgs(TINY)
    batch, n, shape = 2, 48, (3, 4, 4)
    V = TINY['maskgit']['num_tokens']
    g = torch.Generator().manual_seed(9)
    ids = torch.randint(0, V, (batch, *shape), generator=g)
    flat = ids.flatten(1)
    ctx = weights.synthetic_context(batch, 6, TINY['maskgit']['dim_context'], seed=3, pad_last=2)
    base = dict(rand_step=torch.tensor([1, 3]), perm_noise=weights.uniform_noise((batch, n), 710), gumbel_u=weights.uniform_noise((batch, n, V), 711))
    keep = dict(cond_keep=torch.tensor([True, False]), critic_cond_keep=torch.tensor([False, True]))
    draws = dict(base, **keep)
    common = dict(maskgit=mg, cvivit=cv, steps=TINY['steps'], text_embed_dim=TINY['maskgit']['dim_context'])
    if critic_kind == 'self_critic':
        common['self_token_critic'] = True
    else:
        common['critic'] = cr

    def build(**kw):
        ph = P.Phenaki(**common, **kw).cuda()
        P.set_compute_dtype(ph, dtype)
        return ph

    ph = build(label_smoothing=EPS, z_loss_weight=ZETA, train_cond_drop=True)
    mgl = _leaf(mg_sd)
    if critic_kind == 'self_critic':
        torch.manual_seed(0)
        with torch.no_grad():
            ph.critic.to_pred[0].weight.normal_(0, 0.1)
        crl = {'to_pred.0.weight': ph.critic.to_pred[0].weight.detach().cpu().clone().requires_grad_(),
               'to_pred.0.bias': ph.critic.to_pred[0].bias.detach().cpu().clone().requires_grad_()}
        cr_cfg = dict(self_critic=(mgl, mgc))
    else:
        crl, cr_cfg = _leaf(cr_sd), crc

    # ---- reference
    ctx_mg, ctx_cr = ctx.clone(), ctx.clone()
    ctx_mg[~keep['cond_keep']] = 0
    ctx_cr[~keep['critic_cond_keep']] = 0
    ref = O.phenaki_forward_loss(mgl, mgc, None, None, flat, patch_shape=shape, context=ctx_mg, steps=TINY['steps'], mask_id=V, only_train_generator=True, **base)
    logits, mask = ref['logits'], ref['mask']
    ce = S.autograd_objective(logits[mask], flat[mask], EPS, ZETA)
    pred = O.gumbel_argmax(logits.detach(), 1., base['gumbel_u'])
    critic_input = torch.where(mask, pred, flat)
    crit = O.critic_forward(crl, cr_cfg, critic_input, video_patch_shape=shape, context=ctx_cr, text_mask=torch.any(ctx_cr != 0, dim=-1))
    want = ce + F.binary_cross_entropy_with_logits(crit, (flat != pred).float())
    want.backward()
    assert abs(float(ce.detach()) - float(ref['ce'].detach())) > 1e-2, 'the regularisers must move the objective on this batch'

    # ---- product
    params = list(mg.parameters()) + (list(cr.parameters()) if critic_kind == 'token_critic' else list(ph.critic.to_pred.parameters()))

    def step(model, d):
        for p in params:
            p.grad = None
        loss = model(video_codebook_ids=ids.cuda(), text_embeds=ctx.cuda(), _draws=d)
        loss.backward()
        return loss.detach()

    loss = step(ph, draws)
    rel = abs(float(loss) - float(want.detach())) / abs(float(want.detach()))
    print(f'regularised step {critic_kind} {dtype}: loss {float(loss)!r} reference {float(want.detach())!r} (rel {rel:.3e})')
    assert rel <= 2e-4
    probes = [('to_logits.weight', mg.to_logits.weight, mgl['to_logits.weight']), ('to_logits.bias', mg.to_logits.bias, mgl['to_logits.bias']),
              ('token_emb.weight', mg.token_emb.weight, mgl['token_emb.weight']),
              ('cross-attention to_kv.weight', mg.transformer.layers[0][1].to_kv.weight, mgl['transformer.layers.0.1.to_kv.weight'])]
    if critic_kind == 'token_critic':
        probes.append(('critic cross-attention to_kv.weight', cr.transformer.layers[0][1].to_kv.weight, crl['transformer.layers.0.1.to_kv.weight']))
    errs = {name: close(got.grad.cpu(), w.grad, 1e-3, f'{critic_kind} {dtype} d {name}') for name, got, w in probes}
    with torch.no_grad():
        value = ph(video_codebook_ids=ids.cuda(), text_embeds=ctx.cuda(), _draws=draws)
    vrel = abs(float(value) - float(loss)) / abs(float(loss))
    print(f'objective_value {float(value)!r} against the graph\'s loss: rel {vrel:.3e}')
    assert not value.requires_grad and vrel <= 1e-6
    record_parity('ce_reg_training_step', dict(critic=critic_kind, dtype=dtype, loss_rel_err=rel, probes=errs, objective_value_rel=vrel))

    # ---- all three off, same draws (the two keep draws are then ignored): bit for bit the model built without the keywords
    if critic_kind == 'self_critic':
        head = ph.critic.to_pred[0]

        def build_like(**kw):
            m = build(**kw)
            with torch.no_grad():
                m.critic.to_pred[0].weight.copy_(head.weight)
                m.critic.to_pred[0].bias.copy_(head.bias)
            return m
    else:
        build_like = build
    # (the two gradients the step sums with float atomics are not bit-equal between two runs of ANY one model: S.assert_same_step holds them to the
    # tolerance tests/test_dropout_gpu.py holds two runs under one seed to, everything else to bit equality)
    outs = []
    for kw in ({}, dict(label_smoothing=0., z_loss_weight=0., train_cond_drop=False)):
        m = build_like(**kw)
        named = {f'maskgit.{k}': v for k, v in mg.named_parameters()}
        named.update({f'critic.{k}': v for k, v in (cr.named_parameters() if critic_kind == 'token_critic' else m.critic.to_pred.named_parameters())})
        for p in named.values():
            p.grad = None
        l = m(video_codebook_ids=ids.cuda(), text_embeds=ctx.cuda(), _draws=draws)
        l.backward()
        outs.append((l.detach().cpu(), {k: (p.grad.cpu() if p.grad is not None else None) for k, p in named.items()}))
    exact = S.assert_same_step(*outs[1], *outs[0], 'options off against the model built without the keywords')
    print(f'options off: loss and {exact - 1} of {len([v for v in outs[0][1].values() if v is not None])} gradients bit for bit, the atomic sums within 1e-6')
    assert abs(float(outs[0][0]) - float(loss)) > 1e-2 * abs(float(loss)), 'and that is not the regularised loss'
