"""The MaskGIT validation statistics on the GPU: pk_vocab_eval (csrc/sampler.hip) through L.vocab_eval against the float64 restatement
(tests/maskgit_metrics_restatement.py) fed the operands as each mode rounds them, against the existing vocab_sample + vocab_ce path, and
Phenaki.evaluate / MaskGitMetrics against the module's existing objective and its own logits.

Tolerances.  A rank is held to the band [rank_lo, rank_hi] the restatement derives from eps = rel * max|logits| (rel 2e-5 fp32 and bf16 on its
rounded operands, 4e-5 bf16x3) and to the exact rank wherever that band has zero width; pred to the arg-max except where the top two logits are
within eps; nll / lse to tests.util.close at 2e-5 / 4e-5 / 2e-3 (test_vocab_ce_matches_cross_entropy's figures; bf16 also at 2e-5 since the
restatement reads the rounded operands); entropy to rel * max|logits| absolute with the same three figures."""
import math

import pytest
import torch

from oracle import weights
from oracle.configs import TINY
from tests import maskgit_metrics_restatement as R
from tests.util import close, load_product

pytestmark = pytest.mark.gpu

MODES = ['fp32', 'bf16x3', 'bf16']


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    torch.cuda.set_device(0)
    with torch.no_grad():
        yield


@pytest.fixture(scope='module')
def L():
    from phenaki_pytorch_amd import _lib
    _lib.load()
    return _lib


def device_operands(L, mode, c, D):
    """A, W (K-padded, in the mode's operand image), bias, targets, rows on the device"""
    dt = {'fp32': L.F32, 'bf16': L.BF16, 'bf16x3': L.BF16X3}[mode]
    td = L.tdtype(dt)
    q = 64 if mode == 'bf16' else 32
    V = c['W'].shape[0]
    Wp = torch.zeros(V, (D + q - 1) // q * q)
    Wp[:, :D] = c['W']
    A, Wd = c['e'].cuda().to(td), Wp.cuda().to(td)
    if mode == 'bf16x3':
        Wd = L.split_planes(Wd)
    rows = c['rows'].cuda() if c['rows'] is not None else None
    return dt, A, Wd, c['b'].cuda(), c['targets_full'].cuda(), rows


def run_eval(L, dt, A, Wd, b, M, V, D, targets, rows, only=None):
    names = ('pred', 'lse', 'nll', 'rank', 'entropy')
    kinds = dict(pred=torch.int64, rank=torch.int32)
    out = {k: torch.full((M,), -7, device='cuda', dtype=kinds.get(k, torch.float32)) for k in names}
    L.vocab_eval(dt, A, Wd, b, M, V, D, targets, rows, **{k: v for k, v in out.items() if only is None or k in only})
    return out


def check_against_restatement(got, s, mode, what, planted=None):
    """got: dict of device tensors (pred, lse, nll, rank, entropy); s: head_stats of the restatement"""
    rank = got['rank'].cpu().long()
    exact = s['rank_lo'] == s['rank_hi']
    if planted is not None:
        share = float(exact[:planted].float().mean())
        assert share >= 0.95, f'{what}: only {share:.2f} of the planted rows have a rank the inputs determine (a condition on the inputs)'
    nll_rel = float((got['nll'].cpu().double() - s['nll']).abs().max() / s['nll'].abs().max())
    lse_rel = float((got['lse'].cpu().double() - s['lse']).abs().max() / s['lse'].abs().max())
    ent_err = float((got['entropy'].cpu().double() - s['entropy']).abs().max())
    print(f'{what}: rank exact on {int(exact.sum())}/{exact.numel()} determined rows, off-band {int(((rank < s["rank_lo"]) | (rank > s["rank_hi"])).sum())}; '
          f'nll rel {nll_rel:.2e} lse rel {lse_rel:.2e} entropy abs {ent_err:.2e} (max|l| {s["max_abs"]:.2f})')
    assert bool(((rank >= s['rank_lo']) & (rank <= s['rank_hi'])).all()), f'{what}: a rank outside [rank_lo, rank_hi]'
    assert torch.equal(rank[exact], s['rank'][exact]), f'{what}: rank differs where the band has zero width'
    safe = s['top2_gap'] > s['eps']                                    # near-ties may flip with the summation order
    assert torch.equal(got['pred'].cpu()[safe], s['pred'][safe]), f'{what}: arg-max differs outside near-ties'
    for k in ('nll', 'lse'):
        close(got[k], s[k].float(), R.CLOSE[mode], f'{what} {k}')
        if mode == 'bf16':
            close(got[k], s[k].float(), R.REL['bf16'], f'{what} {k} on the rounded operands')
    assert ent_err <= R.CLOSE[mode] * s['max_abs'], f'{what}: entropy off by {ent_err:.3e} > {R.CLOSE[mode]:g} * {s["max_abs"]:.3f}'
    assert torch.isfinite(got['entropy']).all() and float(got['entropy'].min()) >= 0.


@pytest.mark.parametrize('mode', MODES)
@pytest.mark.parametrize('M,V,D,with_rows', R.CASES)
def test_vocab_eval_matches_the_restatement(L, mode, M, V, D, with_rows):
    c = R.make_case(mode, M, V, D, with_rows)
    assert int((c['tg'] == 0).sum()) >= 1 and int((c['tg'] >= (V - 1) // 128 * 128).sum()) >= 1
    dt, A, Wd, b, targets, rows = device_operands(L, mode, c, D)
    got = run_eval(L, dt, A, Wd, b, M, V, D, targets, rows)
    again = run_eval(L, dt, A, Wd, b, M, V, D, targets, rows)
    for k in got:
        assert torch.equal(got[k], again[k]), f'{k}: two calls differ'
    check_against_restatement(got, c['stats'], mode, f'vocab_eval {mode} {M}x{V}x{D}', planted=c['planted'])
    # NULL outputs: only the rank is asked for, the other buffers stay untouched
    alone = run_eval(L, dt, A, Wd, b, M, V, D, targets, rows, only=('rank',))
    assert torch.equal(alone['rank'], got['rank'])
    for k in ('pred', 'lse', 'nll', 'entropy'):
        assert bool((alone[k] == -7).all()), f'{k} was written though not requested'
    # the existing path on the same operands: vocab_sample(need_lse) + vocab_ce
    partials = torch.empty(5 * L.vocab_ntiles(V) * M, device='cuda')
    L.vocab_sample(dt, A, Wd, b, M, V, D, 1.0, None, rows, 7, True, partials)
    loss = torch.full((M,), float('nan'), device='cuda')
    lse = torch.full((M,), float('nan'), device='cuda')
    L.vocab_ce(dt, partials, M, V, A, Wd, b, D, targets, rows, loss, lse)
    close(got['nll'], loss, R.CLOSE[mode], 'nll against vocab_sample + vocab_ce')
    close(got['lse'], lse, R.CLOSE[mode], 'lse against vocab_sample + vocab_ce')


# ------------------------------------------------------------------------------------------ Phenaki.evaluate / MaskGitMetrics (TINY)

F32_GRADE = ['fp32', 'bf16x3']


def tiny_batch(salt=0, batch=2):
    """random token ids (batch, 3, 4, 4), a padded text context and the two masking draws of the objective"""
    g = torch.Generator().manual_seed(40 + salt)
    ids = torch.randint(0, TINY['maskgit']['num_tokens'], (batch, 3, 4, 4), generator=g).cuda()
    ctx = weights.synthetic_context(batch, 6, TINY['maskgit']['dim_context'], seed=3 + salt, pad_last=2).cuda()
    draws = dict(rand_step=torch.tensor([1, 4][:batch]), perm_noise=weights.uniform_noise((batch, 48), 750 + salt))
    return ids, ctx, draws


def product(dtype, critic):
    """critic: None | 'token' | 'self'"""
    import phenaki_pytorch_amd as P
    cv, mg, cr, ph = load_product('tiny', TINY, dtype=dtype, with_critic=critic == 'token')
    if critic == 'self':
        torch.manual_seed(5)
        ph = P.Phenaki(maskgit=mg, cvivit=cv, self_token_critic=True, steps=TINY['steps'], text_embed_dim=TINY['maskgit']['dim_context']).cuda().eval()
        P.set_compute_dtype(ph, dtype)
    return mg, ph


def restate(mg, ph, ids, ctx, mask, dtype):
    """the restatement applied to MaskGit._logits of the embeddings of the same masked input -> head_stats over the masked rows (row-major)"""
    b, n = mask.shape
    flat = ids.reshape(b, n)
    masked_input = torch.where(mask, ph.mask_id, flat)
    e = mg.embeds(masked_input, video_patch_shape=tuple(ids.shape[1:]), context=ctx, text_mask=torch.any(ctx != 0, dim=-1))
    logits = mg._logits(e, b * n, b, n).reshape(b * n, -1).cpu().double()
    keep = mask.reshape(-1).cpu()
    return R.head_stats(logits[keep], flat.reshape(-1).cpu()[keep], R.REL[dtype])


def flags(ph):
    return [m.training for m in ph.modules()]


@pytest.mark.parametrize('dtype', F32_GRADE)
def test_evaluate_matches_the_objective_and_the_restatement(dtype):
    mg, ph = product(dtype, None)
    ids, ctx, draws = tiny_batch()
    b, n = ids.shape[0], ids[0].numel()
    ph.train()
    ph.maskgit.transformer.eval()                                       # a mixed state: every flag has to come back as it was
    before = flags(ph)
    r = ph.evaluate(video_codebook_ids=ids, text_embeds=ctx, _draws=draws)
    assert flags(ph) == before, 'evaluate changed a train / eval flag'
    ph.eval()
    # the mask objective_value derives from the same draws (phenaki_pytorch.py:620-628)
    rand_step, noise = draws['rand_step'].cuda(), draws['perm_noise'].cuda()
    num_masked = (torch.cos(rand_step * math.pi * 0.5 / ph.steps) * n).round().clamp(min=1)
    want_mask = noise.argsort(dim=-1) < num_masked[:, None]
    assert r['mask'].dtype == torch.bool and torch.equal(r['mask'], want_mask)
    assert torch.equal(r['rows'].long(), want_mask.reshape(-1).nonzero().reshape(-1)) and r['rows'].dtype == torch.int32
    M = int(want_mask.sum())
    for k, kind in (('nll', torch.float32), ('entropy', torch.float32), ('lse', torch.float32), ('rank', torch.int32), ('pred', torch.int64)):
        assert r[k].shape == (M,) and r[k].dtype == kind and r[k].is_cuda, k
    assert 'critic_logits' not in r and 'critic_labels' not in r
    loss = ph.objective_value(video_codebook_ids=ids, text_embeds=ctx, only_train_generator=True, _draws=dict(draws))
    got = float(r['nll'].double().mean())
    print(f'evaluate {dtype}: mean nll {got:.6f} vs objective {float(loss):.6f}')
    assert abs(got - float(loss)) <= 1e-4 * abs(float(loss))
    check_against_restatement(r, restate(mg, ph, ids, ctx, want_mask, dtype), dtype, f'evaluate {dtype}')


@pytest.mark.parametrize('critic', ['token', 'self'])
@pytest.mark.parametrize('dtype', F32_GRADE)
def test_evaluate_with_a_critic_fills_in_the_argmax(dtype, critic):
    mg, ph = product(dtype, critic)
    ids, ctx, draws = tiny_batch()
    b, n = ids.shape[0], ids[0].numel()
    before = flags(ph)
    r = ph.evaluate(video_codebook_ids=ids, text_embeds=ctx, _draws=draws)
    assert flags(ph) == before
    flat = ids.reshape(-1)
    filled = flat.clone()
    filled[r['rows'].long()] = r['pred']
    assert torch.equal(r['critic_labels'], (flat != filled).view(b, n)) and r['critic_labels'].dtype == torch.bool
    assert not bool(r['critic_labels'][~r['mask']].any()), 'an unmasked position keeps its id'
    direct = ph.critic(filled.view(ids.shape), cond_drop_prob=0., text_mask=torch.any(ctx != 0, dim=-1), context=ctx)
    assert r['critic_logits'].shape == (b, n) and torch.equal(r['critic_logits'], direct.reshape(b, n))
    again = ph.evaluate(video_codebook_ids=ids, text_embeds=ctx, _draws=draws)
    assert all(torch.equal(r[k], again[k]) for k in r), 'no noise is drawn: two calls agree bit for bit'


def test_mask_prob_and_generator():
    mg, ph = product('fp32', None)
    ids, ctx, _ = tiny_batch()
    b, n = ids.shape[0], ids[0].numel()
    r = ph.evaluate(video_codebook_ids=ids, text_embeds=ctx, mask_prob=1.0)
    assert bool(r['mask'].all()) and torch.equal(r['rows'], torch.arange(b * n, device='cuda', dtype=torch.int32))
    half = ph.evaluate(video_codebook_ids=ids, text_embeds=ctx, mask_prob=0.5)
    assert half['mask'].sum(dim=-1).tolist() == [n // 2] * b
    runs = []
    for _ in range(2):
        gen = torch.Generator(device='cuda').manual_seed(99)
        runs.append([ph.evaluate(video_codebook_ids=ids, text_embeds=ctx, generator=gen) for _ in range(2)])
    for first, second in zip(*runs):
        assert torch.equal(first['rows'], second['rows']) and torch.equal(first['nll'], second['nll'])
    assert not torch.equal(runs[0][0]['mask'], runs[0][1]['mask']), 'the generator advances between batches'
    with pytest.raises(ValueError, match='mask_prob'):
        ph.evaluate(video_codebook_ids=ids, text_embeds=ctx, mask_prob=0.)


def test_maskgit_metrics_pools_two_batches():
    import phenaki_pytorch_amd as P
    mg, ph = product('fp32', 'token')
    mm = P.MaskGitMetrics(ph)
    with pytest.raises(RuntimeError, match='before any update'):
        mm.compute()
    stats, critic = [], []
    for salt in (0, 1):
        ids, ctx, draws = tiny_batch(salt)
        assert mm.update(video_codebook_ids=ids, text_embeds=ctx, _draws=draws) is mm
        r = ph.evaluate(video_codebook_ids=ids, text_embeds=ctx, _draws=draws)
        s = restate(mg, ph, ids, ctx, r['mask'], 'fp32')
        # a rank the inputs leave undetermined (a column within eps of the target's logit) is taken from the kernel, inside its band
        rank = r['rank'].cpu().long()
        assert bool(((rank >= s['rank_lo']) & (rank <= s['rank_hi'])).all())
        s['rank'] = torch.where(s['rank_lo'] == s['rank_hi'], s['rank'], rank)
        stats.append(s)
        critic.append((r['critic_logits'].cpu(), r['critic_labels'].cpu()))
    got, want = mm.compute(), R.pooled(stats, critic)
    print(got)
    assert set(got) == set(want) and all(isinstance(v, (int, float)) for v in got.values())
    for k in ('tokens', 'top1', 'top5', 'top10', 'mean_rank', 'critic_accuracy', 'critic_positive_share'):
        assert got[k] == pytest.approx(want[k], rel=1e-12, abs=0), k                  # counts: exact up to the float64 division
    assert got['mrr'] == pytest.approx(want['mrr'], rel=1e-12)
    for k in ('loss', 'perplexity', 'entropy'):
        assert abs(got[k] - want[k]) <= 2e-5 * max(s['max_abs'] for s in stats), k    # the per-token figure of the kernel test
    assert got['critic_bce'] == pytest.approx(want['critic_bce'], rel=1e-6)           # f32 critic logits, float64 sums on both sides
    mm.reset()
    assert mm.state is None
