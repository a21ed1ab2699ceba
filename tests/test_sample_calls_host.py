"""The wrapper calls of `Phenaki.sample` in the configurations the infilling and guidance recorder tests leave open: no critic, a SelfCritic, a
TokenCritic with and without cross-attention, cond_scale = 1 with texts, prime frames, a fixed seed, the three critic noise schedules, the
parity hooks, and infilling on the table path.  Recorder stubs stand in for the `_lib` wrappers, the trunks, the tokenizer and the decoder, so
nothing here launches a kernel.  Every expected name, order and argument is written down from the loop's definition, not read from a run."""
import contextlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import pytest  # noqa: E402
import torch  # noqa: E402

import phenaki_pytorch_amd as P  # noqa: E402
from oracle.configs import TINY  # noqa: E402
from phenaki_pytorch_amd import phenaki as PH  # noqa: E402
from tests import test_guidance_host as TG  # noqa: E402
from tests import test_infill_host as TI  # noqa: E402

torch.set_grad_enabled(False)
Recorder = TI.Recorder
B, N, STEPS, DCTX, MASK_ID = 2, 48, 4, TINY['maskgit']['dim_context'], TINY['maskgit']['num_tokens']
KS = PH.mask_schedule(N, STEPS)
M64 = 2 ** 64 - 1
# one step of the loop without / with a critic; the last step has no critic pass, steps >= 1 start with the re-masking
HEAD = ['embeds', 'cfg_mix', 'vocab_sample', 'vocab_reduce']
CRITIC = ['embeds', 'critic_head']


def make(critic):
    torch.manual_seed(0)
    cv = P.CViViT(use_vgg_and_gan=False, **TINY['cvivit'])
    mg = P.MaskGit(**TINY['maskgit'])
    kw = dict(self_token_critic=True) if critic == 'self' else dict(critic=P.TokenCritic(**TINY['critic']) if critic == 'token' else None)
    ph = P.Phenaki(maskgit=mg, cvivit=cv, steps=STEPS, text_embed_dim=DCTX, **kw).eval()
    ph.encode_texts = TG.fake_encoder
    return ph


@contextlib.contextmanager
def recording(rec):
    """tests/test_guidance_host.recording, with a decoder stub that decodes the prime tokens too (as the real one does)"""
    def decode(self, ids, _prime_indices=None):
        rec.calls.append(('decode', (ids,), dict(_prime_indices=_prime_indices)))
        T = (ids.shape[1] + (0 if _prime_indices is None else _prime_indices.shape[1])) // self.image_num_tokens
        return torch.zeros(ids.shape[0], 3, 1 + (T - 1) * self.temporal_patch_size, *self.image_size)

    with TG.recording(rec):
        saved = P.CViViT.decode_from_codebook_indices
        P.CViViT.decode_from_codebook_indices = decode
        try:
            yield
        finally:
            P.CViViT.decode_from_codebook_indices = saved


def run(ph, **kw):
    rec = Recorder()
    with recording(rec):
        out = ph.sample(**kw)
    return rec, out


def calls(rec, name):
    return [c for c in rec.calls if c[0] == name]


def loop_names(per_step, tail, remask='topk_mask', first_remask=False):
    names = []
    for s in range(STEPS):
        names += ([remask] if (s > 0 or first_remask) else []) + (per_step if s < STEPS - 1 else tail)
    return names + ['decode']


def test_no_critic_scores_come_from_the_vocabulary_head():
    rec, out = run(make(None), num_frames=5, batch_size=B)
    assert rec.names() == loop_names(HEAD, HEAD)                              # no critic embeds, no critic_head
    assert out.shape == (B, 3, 5, 64, 64)
    remasks = calls(rec, 'topk_mask')
    assert [c[1][1:5] for c in remasks] == [(B, N, KS[s], MASK_ID) for s in (1, 2, 3)]
    assert all(c[2]['scores_next'] is not None for c in remasks)
    # the head leaves the log-sum-exp (need_lse), the reduce turns it into the next step's scores
    assert all(c[1][11] is True for c in calls(rec, 'vocab_sample'))
    assert all(c[1][7] is not None and c[1][8] is True for c in calls(rec, 'vocab_reduce'))
    # the scores ping-pong: what step s writes (vocab_reduce) is what step s + 1 ranks (topk_mask), and it writes the other buffer
    reduces = calls(rec, 'vocab_reduce')
    for s, c in enumerate(remasks, start=1):
        assert c[1][0] is reduces[s - 1][1][7] and c[2]['scores_next'] is reduces[s][1][7] and c[1][0] is not c[2]['scores_next']
    for c in calls(rec, 'embeds'):
        assert c[2]['replicas'] == 1 and c[2]['context'] is None and c[2]['ids_prime'] is None


def test_with_a_critic_the_head_keeps_no_lse():
    rec, _ = run(make('token'), num_frames=5, batch_size=B)
    assert rec.names() == loop_names(HEAD + CRITIC, HEAD)
    assert all(c[2]['scores_next'] is None for c in calls(rec, 'topk_mask'))
    assert all(c[1][11] is False for c in calls(rec, 'vocab_sample'))
    assert all(c[1][7] is None and c[1][8] is False for c in calls(rec, 'vocab_reduce'))


@pytest.mark.parametrize('cond_scale,replicas', [(5., 2), (1., 1)])
def test_self_critic(cond_scale, replicas):
    ph = make('self')
    rec, _ = run(ph, num_frames=5, texts=['a', 'b'], cond_scale=cond_scale)
    assert rec.names() == loop_names(HEAD + CRITIC, HEAD)
    embeds = calls(rec, 'embeds')
    assert len(embeds) == 2 * STEPS - 1
    for c in embeds:                                                          # MaskGit's own passes and the critic's, through MaskGit.embeds
        assert c[2]['replicas'] == replicas and c[2]['context'].shape == (replicas * B, 6, DCTX)
        assert c[2]['text_mask'].dtype == torch.uint8 and c[2]['text_mask'].shape == (replicas * B, 6)
    heads = calls(rec, 'critic_head')
    assert len(heads) == STEPS - 1
    for c in heads:
        assert c[1][4:7] == (B, N, 0) and c[1][7] is (cond_scale != 1) and c[1][8] == cond_scale
    for c in calls(rec, 'cfg_mix'):
        assert c[1][6] == cond_scale and c[1][7] is (cond_scale != 1)
    assert ph._pk_last_sample_key[6] == cond_scale


@pytest.mark.parametrize('has_cross_attn', [True, False])
def test_token_critic_sees_the_doubled_context_only_with_cross_attention(has_cross_attn):
    ph = make('token')
    ph.critic.has_cross_attn = has_cross_attn
    rec, _ = run(ph, num_frames=5, texts=['a', 'b'], cond_scale=5.)
    assert rec.names() == loop_names(HEAD + CRITIC, HEAD)
    embeds = calls(rec, 'embeds')
    mg_embeds = embeds[0::2]
    cr_embeds = embeds[1::2]
    assert len(mg_embeds) == STEPS and len(cr_embeds) == STEPS - 1
    own = TG.fake_encoder(['a', 'b'])
    for c in mg_embeds:
        assert c[2]['replicas'] == 2 and torch.equal(c[2]['context'], torch.cat((own, own)))
    for c in cr_embeds:
        if has_cross_attn:
            assert c[2]['replicas'] == 2 and torch.equal(c[2]['context'], torch.cat((own, own)))
            tm = c[2]['text_mask']
            assert tm.dtype == torch.uint8 and tm[:B].all() and not tm[B:].any()          # [cond | all-False null]
        else:
            assert c[2]['replicas'] == 1 and c[2]['context'] is None and c[2]['text_mask'] is None
    for c in calls(rec, 'critic_head'):
        assert c[1][7] is has_cross_attn and c[1][8] == 5.
    assert all(c[1][7] is True for c in calls(rec, 'cfg_mix'))


def test_texts_with_cond_scale_one_run_one_pass():
    ph = make('token')
    rec, _ = run(ph, num_frames=5, texts=['a', 'b'], cond_scale=1.)
    assert rec.names() == loop_names(HEAD + CRITIC, HEAD)
    for c in calls(rec, 'embeds'):
        assert c[2]['replicas'] == 1 and c[2]['context'].shape == (B, 6, DCTX) and c[2]['text_mask'].shape == (B, 6)
    assert all(c[1][6] == 1. and c[1][7] is False for c in calls(rec, 'cfg_mix'))
    assert all(c[1][7] is False and c[1][8] == 1. for c in calls(rec, 'critic_head'))
    assert ph._pk_last_sample_key[6] == 1.0 and isinstance(ph._pk_last_sample_key[6], float)


def test_prime_frames():
    ph = make('token')
    prime_ids = (torch.arange(B * 16) * 5 % MASK_ID).reshape(B, 16)
    # 4 new frames after 1 prime frame: n = 2 token frames, the grid is that of the 5-frame clip
    rec, out = run(ph, num_frames=4, batch_size=B, prime_frames=torch.zeros(B, 3, 1, 64, 64), _prime_ids=prime_ids)
    n, n_prime = 32, 16
    assert rec.names() == ['tokenize'] + loop_names(HEAD + CRITIC, HEAD)
    for c in calls(rec, 'embeds'):
        assert c[1][0].shape == (B, n) and c[2]['video_patch_shape'] == (3, 4, 4)
        assert c[2]['ids_prime'].shape == (B, n_prime) and torch.equal(c[2]['ids_prime'], prime_ids)
    assert all(c[1][1:4] == (B, n + n_prime, n_prime) for c in calls(rec, 'cfg_mix'))
    assert all(c[1][4:7] == (B, n + n_prime, n_prime) for c in calls(rec, 'critic_head'))
    ks = PH.mask_schedule(n, STEPS)
    assert [c[1][1:4] for c in calls(rec, 'topk_mask')] == [(B, n, ks[s]) for s in (1, 2, 3)]
    dec = calls(rec, 'decode')[0]
    assert dec[1][0].shape == (B, n) and torch.equal(dec[2]['_prime_indices'], prime_ids)
    assert out.shape == (B, 3, 4, 64, 64)                                     # 5 decoded frames, the prime frame cut off
    key = ph._pk_last_sample_key
    assert key[:5] == (B, n, n_prime, 1, (3, 4, 4))


def test_a_given_seed_fixes_every_stream_seed():
    ph = make('token')
    rec, _ = run(ph, num_frames=5, batch_size=B, _seed=12345)
    assert ph._pk_last_seed == 12345
    heads = calls(rec, 'vocab_sample')
    assert [c[1][10] for c in heads] == [(12345 + s * 0x9E3779B97F4A7C15) & M64 for s in range(STEPS)]
    assert all(c[1][8] is None and c[2]['seed_dev'] is None for c in heads)    # no injected noise, eager: no device seed word
    crit = calls(rec, 'critic_head')
    assert [c[2]['seed'] for c in crit] == [(12345 + (2 * s + 1) * 0xD6E8FEB86659FD93) & M64 for s in range(STEPS - 1)]
    assert all(c[1][9] is None and c[2]['seed_dev'] is None for c in crit)


@pytest.mark.parametrize('name,mult', [('fixed', lambda s: 1.), ('decay', lambda s: (STEPS - s - 1) / STEPS), ('increase', lambda s: (s + 1) / STEPS)])
def test_critic_noise_schedules(name, mult):
    ph = make('token')
    ph.critic_noise_anneal_schedule = name
    rec, _ = run(ph, num_frames=5, batch_size=B, noise_K=0.5, starting_temperature=0.8)
    assert [c[1][10] for c in calls(rec, 'critic_head')] == [float(0.5 * mult(s)) for s in range(STEPS - 1)]
    # the head's temperature anneals to 0 at the last step whatever the critic's schedule
    assert [c[1][7] for c in calls(rec, 'vocab_sample')] == [float(0.8 * ((STEPS - s - 1) / STEPS)) for s in range(STEPS)]
    assert ph._pk_last_sample_key[13] == name


def test_an_unknown_noise_schedule_is_refused():
    ph = make('token')
    ph.critic_noise_anneal_schedule = 'cosine'
    with recording(Recorder()), pytest.raises(ValueError, match='invalid critic noise anneal schedule name'):
        ph.sample(num_frames=5, batch_size=B)


@pytest.mark.parametrize('hooks', ['trace', 'force', 'both'])
def test_the_parity_hooks_switch_compaction_off(hooks):
    ph = make('token')
    rec = Recorder()
    trace = [] if hooks in ('trace', 'both') else None
    forced = []

    def force(step, ids, mask):
        assert ids.shape == (B, N) and ids.dtype == torch.int64 and mask.shape == (B, N) and mask.dtype == torch.uint8
        forced.append(step)
        rec.calls.append(('force', (step,), {}))

    with recording(rec):
        ph.sample(num_frames=5, batch_size=B, _trace=trace, _force_fn=force if hooks in ('force', 'both') else None)
    names = [n for n in rec.names() if n != 'force']
    assert names == loop_names(HEAD + CRITIC, HEAD)
    M = B * N
    assert all(c[1][7] is None for c in calls(rec, 'topk_mask'))                         # no row list is written
    assert all(c[1][4] is None and c[1][5] == M for c in calls(rec, 'cfg_mix'))
    assert all(c[1][9] is None and c[1][4] == M for c in calls(rec, 'vocab_sample'))
    assert all(c[1][3] is None and c[1][1] == M for c in calls(rec, 'vocab_reduce'))
    if trace is not None:
        assert [r['step'] for r in trace] == list(range(STEPS))
        always = {'step', 'masked_ids', 'mask', 'prime_ids', 'pred', 'ids'}
        for r in trace:
            assert set(r) == (always | {'scores'} if r['step'] < STEPS - 1 else always)
            assert r['masked_ids'].shape == (B, N) and r['mask'].dtype == torch.bool and r['prime_ids'] is None
    if hooks != 'trace':
        assert forced == list(range(STEPS))
        # once per step, after that step's re-masking and right before its first trunk call
        full = rec.names()
        at = [i for i, n in enumerate(full) if n == 'force']
        assert all(full[i + 1] == 'embeds' for i in at)
        assert [full[i - 1] for i in at[1:]] == ['topk_mask'] * (STEPS - 1)


def test_infilling_on_the_table_path():
    ph = make('token')
    ids0, known = TI._known()
    rec, _ = run(ph, num_frames=5, texts=['a', 'b'], cond_scale=[5., 2.5], known_ids=ids0, known_mask=known)
    per = ['embeds', 'guidance_mix', 'vocab_sample', 'vocab_reduce']
    assert rec.names() == loop_names(per + ['embeds', 'critic_head_guided'], per, remask='topk_mask_keep', first_remask=True)
    ks, offs, totals = PH.infill_schedule([32, 36], STEPS)
    table = PH.guidance_table([5., 2.5], STEPS)
    mixes = calls(rec, 'guidance_mix')
    assert len(mixes) == STEPS
    for s, c in enumerate(mixes):
        assert c[1][1:4] == (B, N, 0) and c[1][4] is not None and c[1][5] == totals[s]
        assert torch.equal(c[1][6], table[s]) and c[1][7:9] == (1, True)
    for s, c in enumerate(calls(rec, 'critic_head_guided')):
        assert torch.equal(c[1][7], table[s]) and c[1][8:10] == (1, True)
    for s, c in enumerate(calls(rec, 'topk_mask_keep')):
        assert c[1][3].tolist() == ks[s] and c[1][4].tolist() == offs[s] and c[2]['k_host'] == ks[s] and c[2]['free_host'] == ks[0]
    assert [c[1][4] for c in calls(rec, 'vocab_sample')] == totals
    assert all(c[2]['replicas'] == 2 and c[2]['context'].shape == (2 * B, 6, DCTX) for c in calls(rec, 'embeds'))
    key = ph._pk_last_sample_key
    assert key[6] == ('guided', 1, False, 6) and key[14] == (32, 36)
