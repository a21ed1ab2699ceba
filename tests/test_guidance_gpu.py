"""Guided sampling on the MI355X (-m gpu): pk_guidance_mix and pk_critic_head_guided against their float64 restatements
(tests/guidance_restatement.py) and bit for bit against pk_cfg_mix / pk_critic_head at P = 1; the table path of `Phenaki.sample` end to end
on the two TINY configurations whose tie margins tests/test_guidance_host.py asserts; its equality with the scalar path; graph replay across
scales; the logits surface and the pass-through of `infill` / `make_video`."""
import functools

import pytest
import torch

from oracle import phenaki_oracle as O
from oracle import weights
from oracle.configs import TINY, oracle_cfgs, state_dicts
from phenaki_pytorch_amd import _lib as L
from phenaki_pytorch_amd import phenaki as PH
from tests import guidance_restatement as G
from tests.util import argmax_equal_with_margin, close, load_product, noise_fn_cuda, record_parity

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

OK, EINVAL = 0, -1
DCTX = TINY['maskgit']['dim_context']
N_TOT = 5
SENT = 768.                 # exactly representable in bf16


@pytest.fixture(scope='module')
def lib():
    from phenaki_pytorch_amd import build
    build.build(verbose=False)
    return L.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ pk_guidance_mix

def _rows_cases(nb, n, gen):
    """None, and compact lists of 1 and 7 logical rows that hold the first and the last one (repeats where nb n < 7: a gather may repeat)"""
    last = nb * n - 1
    seven = [0, last] + torch.randint(0, nb * n, (5,), generator=gen).tolist()
    return [None, [last], [seven[i] for i in torch.randperm(7, generator=gen).tolist()]]


def _coef(P, nb, gen):
    """blend weights in [0, 1] whose sum over k >= 1 stays <= 1 (a[0] = 1 - sum), scales in [-2, 8]"""
    w = torch.rand((P - 1, nb), generator=gen) / max(P - 1, 1)
    a0 = 1. - w.sum(0, keepdim=True)
    g = torch.rand((1, nb), generator=gen) * 10. - 2.
    return torch.cat((a0, w, g), dim=0).float().reshape(-1).contiguous()


@pytest.mark.parametrize('out_f32', [True, False])
@pytest.mark.parametrize('D', [4, 132, 512])
def test_guidance_mix_against_float64(lib, D, out_f32):
    gen = torch.Generator().manual_seed(100 + D)
    worst = 0.
    for nb in (1, 3):
        for n_prime in (0, 2):
            n = N_TOT - n_prime
            for rows in _rows_cases(nb, n, gen):
                nrows = nb * n if rows is None else len(rows)
                for P in (1, 2, 3):
                    for has_base in (0, 1):
                        if P == 1 and not has_base:
                            continue
                        x = torch.randn(((P + has_base) * nb * N_TOT, D), generator=gen)
                        coef = _coef(P, nb, gen)
                        ref, bound = G.guidance_mix_ref(x, nb, N_TOT, n_prime, rows, nrows, coef, P, has_base)
                        out = torch.full((nrows + 1, D), SENT, device='cuda', dtype=torch.float32 if out_f32 else torch.bfloat16)
                        rows_d = None if rows is None else torch.tensor(rows, dtype=torch.int32, device='cuda')
                        L.guidance_mix(x.cuda(), nb, N_TOT, n_prime, rows_d, nrows, coef.cuda(), P, bool(has_base), out, D)
                        got = out.cpu().double()
                        what = f'D={D} nb={nb} n_prime={n_prime} rows={rows} P={P} has_base={has_base}'
                        assert (got[nrows] == SENT).all(), f'{what}: wrote past the last output row'
                        if not out_f32:
                            bound = bound + 2.0 ** -8 * ref.abs()                     # half a bf16 ulp
                        err = (got[:nrows] - ref).abs()
                        assert (err <= bound).all(), f'{what}: max err / bound {(err / bound.clamp(min=1e-300)).max().item():.3f}'
                        worst = max(worst, (err / bound.clamp(min=1e-300)).max().item())
    record_parity('guidance_mix_vs_float64', dict(D=D, out='f32' if out_f32 else 'bf16', err_over_bound=worst))


@pytest.mark.parametrize('out_f32', [True, False])
@pytest.mark.parametrize('D', [4, 132, 512])
def test_guidance_mix_one_branch_is_cfg_mix_bit_for_bit(lib, D, out_f32):
    gen = torch.Generator().manual_seed(200 + D)
    nb = 3
    odt = torch.float32 if out_f32 else torch.bfloat16
    bits = lambda t: t.view(torch.int32 if out_f32 else torch.int16)
    for n_prime in (0, 2):
        n = N_TOT - n_prime
        for rows in _rows_cases(nb, n, gen):
            nrows = nb * n if rows is None else len(rows)
            rows_d = None if rows is None else torch.tensor(rows, dtype=torch.int32, device='cuda')
            x = torch.randn((2 * nb * N_TOT, D), generator=gen).cuda()

            def cfg(scale):
                out = torch.full((nrows, D), SENT, device='cuda', dtype=odt)
                L.cfg_mix(x, nb, N_TOT, n_prime, rows_d, nrows, scale, True, out, D)
                return out

            def guided(scales):
                coef = torch.tensor([1.] * nb + list(scales), dtype=torch.float32, device='cuda')
                out = torch.full((nrows, D), SENT, device='cuda', dtype=odt)
                L.guidance_mix(x, nb, N_TOT, n_prime, rows_d, nrows, coef, 1, True, out, D)
                return out

            assert torch.equal(bits(guided([5.] * nb)), bits(cfg(5.))), f'equal scales, n_prime={n_prime} rows={rows}'
            scales = [5., 2.5, -0.75]
            got = guided(scales)
            batch_of = torch.tensor(list(range(nb * n)) if rows is None else rows) // n
            for b, s in enumerate(scales):
                want = cfg(s)
                sel = (batch_of == b).cuda()
                assert torch.equal(bits(got)[sel], bits(want)[sel]), f'scale {s} of sample {b}, n_prime={n_prime} rows={rows}'


# ------------------------------------------------------------------------------------------------ pk_critic_head_guided

@pytest.mark.parametrize('D', [132, 512])
def test_critic_head_guided_one_branch_is_critic_head_bit_for_bit(lib, D):
    gen = torch.Generator().manual_seed(300 + D)
    nb = 3
    for n_prime in (0, 2):
        n = N_TOT - n_prime
        x = torch.randn((2 * nb * N_TOT, D), generator=gen).cuda()
        w, b = torch.randn((D,), generator=gen).cuda(), torch.randn((1,), generator=gen).cuda()
        u = torch.rand((nb, n), generator=gen).cuda()
        seed_dev = torch.tensor([12345], dtype=torch.int64, device='cuda')
        for noise in (dict(u=u, seed=0, seed_dev=None), dict(u=None, seed=99, seed_dev=seed_dev)):          # injected draws; the counter hash
            def plain(scale):
                out = torch.full((nb, n), SENT, device='cuda')
                L.critic_head(x, w, b, D, nb, N_TOT, n_prime, True, scale, noise['u'], 0.5, out, seed=noise['seed'], seed_dev=noise['seed_dev'])
                return out

            def guided(scales):
                coef = torch.tensor([1.] * nb + list(scales), dtype=torch.float32, device='cuda')
                out = torch.full((nb, n), SENT, device='cuda')
                L.critic_head_guided(x, w, b, D, nb, N_TOT, n_prime, coef, 1, True, noise['u'], 0.5, out, seed=noise['seed'], seed_dev=noise['seed_dev'])
                return out

            assert torch.equal(guided([5.] * nb).view(torch.int32), plain(5.).view(torch.int32))
            scales = [5., 2.5, -0.75]
            got = guided(scales)
            for bi, s in enumerate(scales):
                assert torch.equal(got[bi].view(torch.int32), plain(s)[bi].view(torch.int32)), f'scale {s} of sample {bi}'


@pytest.mark.parametrize('D', [132, 512])
@pytest.mark.parametrize('P', [2, 3])
def test_critic_head_guided_against_float64(lib, D, P):
    gen = torch.Generator().manual_seed(400 + D + P)
    nb, worst = 3, 0.
    for n_prime in (0, 2):
        n = N_TOT - n_prime
        for has_base in (0, 1):
            for with_bias, with_u in ((True, True), (False, False)):
                x = torch.randn(((P + has_base) * nb * N_TOT, D + 4), generator=gen)             # a strided x: ldx = D + 4
                w = torch.randn((D,), generator=gen)
                b = torch.randn((1,), generator=gen) if with_bias else None
                u = torch.rand((nb, n), generator=gen) if with_u else None
                coef = _coef(P, nb, gen)
                ref, bound = G.critic_head_guided_ref(x, w, b, D, nb, N_TOT, n_prime, coef, P, has_base, u, 0.5)
                out = torch.full((nb * n + 4,), SENT, device='cuda')
                L.critic_head_guided(x.cuda(), w.cuda(), None if b is None else b.cuda(), D, nb, N_TOT, n_prime, coef.cuda(), P, bool(has_base),
                                     None if u is None else u.cuda(), 0.5 if with_u else 0., out)
                got = out.cpu().double()
                assert (got[nb * n:] == SENT).all(), 'wrote past the last output row'
                err = (got[:nb * n].reshape(nb, n) - ref).abs()
                # the restatement's tree bound, and the looser ceiling it must stay under
                xs = x[:, :D].double().reshape(P + has_base, nb, N_TOT, D)[:, :, n_prime:]
                ceiling = D * 2.0 ** -24 * (1 + coef.double().reshape(P + 1, nb)[P].abs() * has_base)[:, None] * \
                    ((xs * w.double()).abs().sum(-1) + (0. if b is None else b.abs().item())).sum(0)
                if not with_u:
                    assert (bound <= ceiling).all()
                assert (err <= bound).all(), f'D={D} P={P} n_prime={n_prime} has_base={has_base}: err / bound {(err / bound).max().item():.3f}'
                worst = max(worst, (err / bound).max().item())
    record_parity('critic_head_guided_vs_float64', dict(D=D, P=P, err_over_bound=worst))


def test_refusals_of_both_kernels(lib):
    D, nb = 8, 2
    x = torch.zeros((4 * nb * N_TOT, D), device='cuda')
    coef = torch.ones((4 * nb,), device='cuda')
    out = torch.full((nb * N_TOT, D), SENT, device='cuda')
    w = torch.zeros((D,), device='cuda')
    sc = torch.full((nb * N_TOT,), SENT, device='cuda')

    def mix(P=2, has_base=1, coef_p=coef.data_ptr(), D_=D):
        return lib.pk_guidance_mix(x.data_ptr(), D, nb, N_TOT, 0, None, nb * N_TOT, coef_p, P, has_base, out.data_ptr(), D, 1, D_, stream())

    def head(P=2, has_base=1, coef_p=coef.data_ptr(), D_=D):
        return lib.pk_critic_head_guided(x.data_ptr(), D, w.data_ptr(), None, D_, nb, N_TOT, 0, coef_p, P, has_base, None, 0., 0, None, sc.data_ptr(), stream())

    for fn in (mix, head):
        assert fn(P=0) == EINVAL and fn(P=4) == EINVAL and fn(P=-1) == EINVAL
        assert fn(coef_p=None) == EINVAL
        assert fn(D_=6) == EINVAL
        assert fn(P=1, has_base=0) == EINVAL
    torch.cuda.synchronize()
    assert (out == SENT).all() and (sc == SENT).all(), 'a refused call wrote'
    assert mix() == OK and head() == OK and mix(P=3, has_base=1) == OK and head(P=2, has_base=0) == OK
    torch.cuda.synchronize()
    # the wrappers refuse what the C entry points cannot see: a short table, a short x
    with pytest.raises(ValueError, match='coef holds'):
        L.guidance_mix(x, nb, N_TOT, 0, None, nb * N_TOT, coef[:5], 2, True, out, D)
    with pytest.raises(ValueError, match='rows'):
        L.critic_head_guided(x[:3 * nb * N_TOT - 1], w, None, D, nb, N_TOT, 0, coef, 2, True, None, 0., sc)


# ------------------------------------------------------------------------------------------------ Phenaki.sample, the table path

def _contexts():
    """text -> (1, L, d) context row; 't0' / 't1' are the rows of the issue's `texts`, 'b*' the blend branch, 'n*' the negative prompt,
    'm*' a negative prompt of another length, 'z' the degenerate one (all-zero embeddings)"""
    out = {}
    for prefix, (L_, seed) in dict(t=(6, 2), b=(4, 3), n=(9, 4), m=(7, 5)).items():
        c = weights.synthetic_context(2, L_, DCTX, seed=seed)
        out[prefix + '0'], out[prefix + '1'] = c[0:1], c[1:2]
    out['z'] = torch.zeros((1, 5, DCTX))
    return out


def _with_encoder(ph):
    table = {k: v.cuda() for k, v in _contexts().items()}
    ph.encode_texts = lambda texts, output_device=None: torch.cat([table[t] for t in texts], dim=0)
    return ph


@functools.lru_cache(maxsize=None)
def product(dtype):
    return _with_encoder(load_product('tiny', TINY, dtype=dtype)[3])


@functools.lru_cache(maxsize=None)
def restated(name):
    """the f32 restatement of configuration `name`, once ('fp32' and 'bf16x3' are both held to the oracle's f32 arithmetic:
    O.precision('bf16x3') is O.precision('fp32'))"""
    with O.precision('fp32'):
        return G.run_config(name, decode=True)


T2, N2, B2 = ['t0', 't1'], ['n0', 'n1'], ['b0', 'b1']
SAMPLE_KW = dict(A=dict(cond_scale=[5., 2.5], guidance_schedule='linear', negative_texts=N2, blend=[(B2, [0.25, 0.75])]),
                 B=dict(cond_scale=[5., 2.5], negative_texts=N2))


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('name', ['A', 'B'])
def test_configuration_end_to_end(lib, name, dtype):
    ph = product(dtype)
    with O.precision(dtype):
        ref, vid_ref, ids_ref = restated(name)
    trace = []
    vid, ids = ph.sample(texts=T2, num_frames=5, starting_temperature=0.9, noise_K=1., _noise_fn=noise_fn_cuda(G.config(name)['base']), _trace=trace,
                         _return_ids=True, **SAMPLE_KW[name])
    assert len(trace) == len(ref) == TINY['steps']
    worst_scores = 0.
    for r, t in zip(ref, trace):
        assert torch.equal(t['masked_ids'].cpu(), r['masked_ids']), f"step {r['step']}: masked ids"
        flips = argmax_equal_with_margin(t['pred'], r['pred'], r['noisy'], tol=1e-4, what=f"{name} {dtype} step {r['step']}")
        assert flips == 0, f"step {r['step']}: {flips} predictions differ (the oracle has no tie within 1e-4)"
        if r['scores'] is not None:
            worst_scores = max(worst_scores, close(t['scores'], r['scores'], 1e-3, f"step {r['step']} scores"))
    assert torch.equal(ids.cpu(), ids_ref)
    e_pix = close(vid, vid_ref, 1e-3, 'pixels')
    record_parity('guided_sample_vs_restatement', dict(config=name, dtype=dtype, steps=len(ref), flips=0, scores_rel_err=worst_scores, pixels_rel_err=e_pix))


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3', 'bf16'])
def test_table_path_equals_scalar_path(lib, dtype):
    ph = product(dtype)
    kw = dict(texts=T2, num_frames=5, _seed=1234, _return_ids=True)
    vid5, ids5 = ph.sample(cond_scale=5., **kw)
    vid, ids = ph.sample(cond_scale=[5., 5.], **kw)
    assert torch.equal(ids, ids5) and torch.equal(vid.view(torch.int32), vid5.view(torch.int32))
    vid25, ids25 = ph.sample(cond_scale=2.5, **kw)
    vid, ids = ph.sample(cond_scale=[5., 2.5], **kw)
    assert torch.equal(ids[0], ids5[0]) and torch.equal(vid[0].view(torch.int32), vid5[0].view(torch.int32))
    assert torch.equal(ids[1], ids25[1]) and torch.equal(vid[1].view(torch.int32), vid25[1].view(torch.int32))
    assert not torch.equal(ids5[1], ids25[1]), 'the two scales sample the same clip: the comparison shows nothing'


def test_a_degenerate_negative_prompt_is_the_null_branch(lib):
    ph = product('fp32')
    kw = dict(texts=T2, num_frames=5, cond_scale=5., _seed=77, _return_ids=True)
    _, ids_plain = ph.sample(**kw)
    _, ids = ph.sample(negative_texts='z', **kw)                 # all-zero embeddings: the text mask is all False
    assert torch.equal(ids, ids_plain)


def test_self_critic_takes_the_guided_head(lib):
    """SelfCritic scores come from the MaskGit trunk, so it sees the text: the table path mixes its head outputs with pk_critic_head_guided.
    [3., 3.] samples what 3. samples, bit for bit; a blend under a negative prompt (J = 3, the unshared route) runs and is finite."""
    import phenaki_pytorch_amd as P
    cv, mg, _, _ = load_product('tiny', TINY)
    ph = _with_encoder(P.Phenaki(maskgit=mg, cvivit=cv, self_token_critic=True, steps=4, text_embed_dim=DCTX).cuda().eval())
    kw = dict(texts=T2, num_frames=5, _seed=31, _return_ids=True)
    vid3, ids3 = ph.sample(cond_scale=3., **kw)
    vid, ids = ph.sample(cond_scale=[3., 3.], **kw)
    assert torch.equal(ids, ids3) and torch.equal(vid.view(torch.int32), vid3.view(torch.int32))
    vid, ids = ph.sample(cond_scale=[3., 4.], negative_texts=N2, blend=[(B2, 0.5)], **kw)
    assert vid.shape == vid3.shape and torch.isfinite(vid).all() and int(ids.max()) < 256 and not torch.equal(ids, ids3)


# ------------------------------------------------------------------------------------------------ the logits surface

@pytest.mark.parametrize('dtype,tol', [('fp32', 1e-3), ('bf16x3', 1e-3), ('bf16', 2e-2)])
def test_forward_with_cond_scale_per_sample_scale_and_negative_context(lib, dtype, tol):
    _, mg, cr, _ = load_product('tiny', TINY, dtype=dtype)
    _, mg_sd, cr_sd = state_dicts('tiny')
    _, mgc, crc = oracle_cfgs(TINY)
    c = _contexts()
    ctx, neg = torch.cat((c['t0'], c['t1'])), torch.cat((c['n0'], c['n1']))
    gen = torch.Generator().manual_seed(5)
    ids = torch.randint(0, 257, (2, 48), generator=gen)
    scale = torch.tensor([5., 2.5])
    (cond,), base = G.pad_contexts([ctx], neg)
    with O.precision(dtype):
        fwd = lambda cm: O.maskgit_forward(mg_sd, mgc, ids, video_patch_shape=(3, 4, 4), context=cm[0], text_mask=cm[1]).double()
        ref = G.mix([fwd(cond)], fwd(base), None, scale.double())
        cfwd = lambda cm: O.critic_forward(cr_sd, crc, ids, video_patch_shape=(3, 4, 4), context=cm[0], text_mask=cm[1]).double()
        sref = G.mix([cfwd(cond)], cfwd(base), None, scale.double())
    kw = dict(video_patch_shape=(3, 4, 4), context=ctx.cuda(), text_mask=(ctx != 0).any(-1).cuda(), negative_context=neg.cuda(),
              negative_text_mask=(neg != 0).any(-1).cuda())
    out = mg.forward_with_cond_scale(ids.cuda(), cond_scale=scale, **kw)
    assert out.shape == (2, 48, 256)
    e_logits = close(out, ref, tol, f'guided logits {dtype}')
    e_critic = close(cr.forward_with_cond_scale(ids.cuda(), cond_scale=scale.tolist(), **kw), sref, tol, f'guided critic scores {dtype}')
    record_parity('guided_logits_vs_oracle', dict(dtype=dtype, logits_rel_err=e_logits, critic_rel_err=e_critic))


# ------------------------------------------------------------------------------------------------ graph replay, pass-through

def test_graph_replays_across_scales_and_schedules(lib):
    ph = _with_encoder(load_product('tiny', TINY, dtype='bf16')[3])
    # the second call differs in scales and schedule AND swaps the prompts of the two samples: the padded contexts are refilled, not captured
    calls = [dict(texts=T2, cond_scale=[5., 2.5], guidance_schedule='linear', negative_texts=N2, _seed=11),
             dict(texts=T2[::-1], cond_scale=[1.5, 7.], guidance_schedule=[0.2, 0.4, 0.4, 0.8, 1., 1.25], negative_texts=N2[::-1], _seed=12)]
    longer = dict(texts=T2, cond_scale=[5., 2.5], guidance_schedule='linear', negative_texts=['m0', 'm1'], _seed=11)
    eager = [ph.sample(num_frames=5, _return_ids=True, **kw) for kw in calls + [longer]]
    assert not torch.equal(eager[0][1], eager[1][1])
    ph.enable_sample_graph()
    try:
        for kw, (vid_e, ids_e) in zip(calls, eager):
            vid, ids = ph.sample(num_frames=5, _return_ids=True, **kw)
            assert torch.equal(ids, ids_e) and torch.equal(vid.view(torch.int32), vid_e.view(torch.int32))
        assert len(ph._pk_sample_graphs) == 1
        # a negative prompt of 7 rows instead of 9: the padded length L drops from 9 to 7, other launches, a second graph
        vid, ids = ph.sample(num_frames=5, _return_ids=True, **longer)
        assert torch.equal(ids, eager[2][1]) and torch.equal(vid.view(torch.int32), eager[2][0].view(torch.int32))
        assert len(ph._pk_sample_graphs) == 2
    finally:
        ph.enable_sample_graph(False)


def test_infill_and_make_video_forward_the_guidance_arguments(lib):
    ph = product('fp32')
    cv = ph.cvivit
    video = weights.synthetic_video(2, 5, 64, 64, seed=3).cuda()
    edit = torch.zeros((1, 3, 4, 4), dtype=torch.bool, device='cuda')
    edit[0, 1:] = True
    kw = dict(cond_scale=[4., 2.], negative_texts=N2, _seed=5)
    got = ph.infill(video, edit, texts=T2, mask_level='token', **kw)
    ids = cv(video, return_only_codebook_ids=True).reshape(2, -1)
    want = ph.sample(num_frames=5, texts=T2, batch_size=2, known_ids=ids, known_mask=~edit[0], **kw)
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    plain = ph.infill(video, edit, texts=T2, mask_level='token', cond_scale=4., _seed=5)
    assert not torch.equal(got, plain), 'the negative prompt changed nothing: the comparison shows nothing'

    kw = dict(cond_scale=4., negative_texts='n0', guidance_schedule='linear', _seed=7)
    full, scenes = PH.make_video(ph, ['t0', 'b1'], (5, 4), 3, **kw)
    first = ph.sample(texts='t0', num_frames=5, **kw)
    second = ph.sample(texts='b1', num_frames=4, prime_frames=first[:, :, -3:], **kw)
    assert torch.equal(scenes[0].view(torch.int32), first.view(torch.int32)) and torch.equal(scenes[1].view(torch.int32), second.view(torch.int32))
    assert full.shape[2] == 9
