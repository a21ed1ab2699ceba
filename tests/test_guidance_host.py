"""Guided sampling on the CPU: the restatement against the oracle's plain sampler, the table builder by hand, the tie margins of the two GPU
parity configurations, which wrappers `sample` calls on the scalar and on the table path (recorder stubs in place of the `_lib` wrappers, so no
kernel runs), every ValueError before any call, the rank slices of `sample_sharded`, and the graph key."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import pytest  # noqa: E402
import torch  # noqa: E402

import phenaki_pytorch_amd as P  # noqa: E402
from oracle import phenaki_oracle as O  # noqa: E402
from oracle import weights  # noqa: E402
from oracle.configs import TINY, oracle_cfgs, state_dicts  # noqa: E402
from phenaki_pytorch_amd import _lib as L  # noqa: E402
from phenaki_pytorch_amd import dist as PD  # noqa: E402
from phenaki_pytorch_amd import phenaki as PH  # noqa: E402
from tests import guidance_restatement as G  # noqa: E402
from tests import test_infill_host as TI  # noqa: E402

torch.set_grad_enabled(False)
N, DCTX = 48, TINY['maskgit']['dim_context']


# --------------------------------------------------------------------------- 1. the restatement

def test_one_branch_null_base_constant_scale_is_the_oracles_sampler():
    cv_sd, mg_sd, cr_sd = state_dicts('tiny')
    cvc, mgc, crc = oracle_cfgs(TINY)
    ctx = weights.synthetic_context(2, 6, DCTX, seed=2)
    ref, got = [], []
    vid_ref, ids_ref = O.sample(cv_sd, cvc, mg_sd, mgc, cr_sd, crc, num_frames=5, batch_size=2, context=ctx, steps=TINY['steps'], cond_scale=5.,
                                noise_fn=G.oracle_noise(500), trace=ref)
    vid, ids = G.guided_sample(cv_sd, cvc, mg_sd, mgc, cr_sd, crc, num_frames=5, contexts=[ctx], cond_scale=[5., 5.], steps=TINY['steps'],
                               noise_fn=G.oracle_noise(500), trace=got)
    assert len(ref) == len(got) == TINY['steps']
    for a, b in zip(ref, got):
        for key in ('masked_ids', 'mask', 'pred', 'ids'):
            assert torch.equal(a[key], b[key]), f"step {b['step']}: {key}"
        assert (a['scores'] is None) == (b['scores'] is None)
        if a['scores'] is not None:
            assert torch.equal(a['scores'], b['scores']), f"step {b['step']}: scores"
    assert torch.equal(ids_ref, ids) and torch.equal(vid_ref, vid)


# --------------------------------------------------------------------------- 2. the table

def test_table_by_hand():
    # no schedule: the f32 entry IS float32(cond_scale[b]), at every step
    cs = [5., 2.5, 1. / 3., 7.1]
    for tab in (G.table(cs, 4)[1], PH.guidance_table(cs, 4).numpy()):
        assert tab.shape == (4, 2, 4) and tab.dtype == np.float32
        assert (tab[:, 1] == np.asarray(cs, dtype=np.float32)[None]).all()
        assert (tab[:, 0] == 1.).all()
    # 'linear' at steps = 6: m[s] = (s + 1) / 6, g = 1 + (c - 1) m in float64, rounded once
    t64, t32 = G.table([5., 2.5], 6, 'linear')
    for s in range(6):
        assert t64[s, 1].tolist() == [1. + 4. * ((s + 1) / 6), 1. + 1.5 * ((s + 1) / 6)]
    assert t64[5, 1].tolist() == [5., 2.5] and t64[2, 1].tolist() == [3., 1.75]
    assert (t32 == t64.astype(np.float32)).all()
    assert PH.guidance_multipliers('linear', 6) == [(s + 1) / 6 for s in range(6)]
    assert torch.equal(PH.guidance_table([5., 2.5], 6, PH.guidance_multipliers('linear', 6)), torch.from_numpy(t32))
    # a[0] = 1 - the sum of the others; a shared weight is broadcast
    t64, t32 = G.table([3., 3.], 2, None, [[0.25, 0.75], 0.125])
    assert t64.shape == (2, 4, 2)
    assert t64[0, 1].tolist() == [0.25, 0.75] and t64[0, 2].tolist() == [0.125, 0.125]
    assert t64[0, 0].tolist() == [1 - 0.25 - 0.125, 1 - 0.75 - 0.125] and (t64[1] == t64[0]).all()
    assert torch.equal(PH.guidance_table([3., 3.], 2, None, [[0.25, 0.75], [0.125, 0.125]]), torch.from_numpy(t32))
    # an explicit schedule
    t64, _ = G.table([4.], 3, [0., 0.5, 2.])
    assert t64[:, 1, 0].tolist() == [1., 2.5, 7.]
    assert torch.equal(PH.guidance_table([4.], 3, PH.guidance_multipliers([0., 0.5, 2.], 3))[:, 1, 0], torch.tensor([1., 2.5, 7.]))


def test_mix_by_hand():
    e = [torch.tensor([[1., 2.], [3., 4.]], dtype=torch.float64), torch.tensor([[10., 20.], [30., 40.]], dtype=torch.float64)]
    base = torch.tensor([[0.5, 0.5], [1., 1.]], dtype=torch.float64)
    a = torch.tensor([[0.75, 0.5], [0.25, 0.5]], dtype=torch.float64)
    g = torch.tensor([2., 3.], dtype=torch.float64)
    cbar = torch.tensor([[3.25, 6.5], [16.5, 22.]], dtype=torch.float64)
    assert torch.equal(G.mix(e, None, a, None), cbar)
    assert torch.equal(G.mix(e, base, a, g), base + (cbar - base) * g[:, None])
    assert torch.equal(G.mix(e[:1], base, None, g), base + (e[0] - base) * g[:, None])        # P == 1: no multiply, a is not read


# --------------------------------------------------------------------------- 3. the parity configurations have no near tie

@pytest.mark.parametrize('name', ['A', 'B'])
def test_parity_configuration_has_no_near_tie(name):
    """float64 restatement, TINY, B = 2, 5 frames, 6 steps, starting_temperature 0.9, noise_K 1, 'decay'.  Measured here:
    A (blend + negative + linear schedule, base 700): prediction gap 3.75e-4, top-k boundary gap 1.51e-3;
    B (negative only, per-sample scales, base 710):  prediction gap 4.13e-4, top-k boundary gap 4.42e-3."""
    trace, _, _ = G.run_config(name, double=True)
    pred_gap, score_gap = G.gaps(trace, TINY['steps'])
    print(f'configuration {name}: prediction gap {pred_gap:.3e}, top-k boundary gap {score_gap:.3e}')
    assert pred_gap >= 1.5e-4
    assert score_gap >= 4e-4
    # and the f32 restatement the GPU test compares with walks the same path
    t32, _, _ = G.run_config(name)
    for a, b in zip(trace, t32):
        assert torch.equal(a['pred'], b['pred']) and torch.equal(a['masked_ids'], b['masked_ids'])


# --------------------------------------------------------------------------- 4. dispatch and refusals, no kernel

Recorder = TI.Recorder


def recording(rec):
    """tests/test_infill_host.recording with the two new wrappers recorded too"""
    import contextlib

    @contextlib.contextmanager
    def ctx():
        saved = [(k, getattr(L, k)) for k in ('guidance_mix', 'critic_head_guided')]
        try:
            with TI.recording(rec):
                for k, _ in saved:
                    setattr(L, k, rec.stub(k))
                yield
        finally:
            for k, v in saved:
                setattr(L, k, v)
    return ctx()


TEXTS = {'a': (6, 2), 'b': (6, 2), 'other': (4, 3), 'bad': (9, 4), 'worse': (9, 5)}


def fake_encoder(texts, output_device=None):
    """a str -> synthetic_context row: every text of a call has one length (the table path pads across branches, not within one)"""
    L_, seed = TEXTS[texts[0]]
    assert all(TEXTS[t][0] == L_ for t in texts)
    return weights.synthetic_context(len(texts), L_, DCTX, seed=seed)


@pytest.fixture()
def phenaki():
    torch.manual_seed(0)
    cv = P.CViViT(use_vgg_and_gan=False, **TINY['cvivit'])
    mg = P.MaskGit(**TINY['maskgit'])
    cr = P.TokenCritic(**TINY['critic'])
    ph = P.Phenaki(maskgit=mg, cvivit=cv, critic=cr, steps=4, text_embed_dim=DCTX).eval()
    ph.encode_texts = fake_encoder
    return ph


def test_scalar_scale_and_no_new_argument_makes_todays_calls(phenaki):
    rec = Recorder()
    with recording(rec):
        phenaki.sample(num_frames=5, texts=['a', 'b'], cond_scale=5., _compact=True)
    names = rec.names()
    assert 'guidance_mix' not in names and 'critic_head_guided' not in names
    per = ['embeds', 'cfg_mix', 'vocab_sample', 'vocab_reduce', 'embeds', 'critic_head']
    assert names == per + (['topk_mask'] + per) * 2 + ['topk_mask'] + per[:4] + ['decode']
    for c in rec.calls:
        if c[0] == 'embeds':
            assert c[2]['replicas'] == 2 and c[2]['context'].shape == (4, 6, DCTX)
        if c[0] == 'cfg_mix':
            assert c[1][6] == 5. and c[1][7] is True
        if c[0] == 'critic_head':
            assert c[1][7] is True and c[1][8] == 5.
    assert phenaki._pk_last_sample_key[6] == 5.


@pytest.mark.parametrize('kw,P_,has_neg,Lmax', [
    (dict(cond_scale=[5., 2.5]), 1, False, 6),
    (dict(cond_scale=3., guidance_schedule='linear'), 1, False, 6),
    (dict(cond_scale=3., negative_texts='bad'), 1, True, 9),
    (dict(cond_scale=[5., 2.5], negative_texts=['bad', 'bad'], blend=[('other', [0.25, 0.75])], guidance_schedule='linear'), 2, True, 9),
    (dict(cond_scale=2., blend=[('other', 0.25), (['bad', 'bad'], 0.5)]), 3, False, 9),
])
def test_table_path_calls(phenaki, kw, P_, has_neg, Lmax):
    J = P_ + 1
    rec = Recorder()
    with recording(rec):
        phenaki.sample(num_frames=5, texts=['a', 'b'], _compact=True, **kw)
    names = rec.names()
    assert 'cfg_mix' not in names and 'critic_head' not in names
    per = ['embeds', 'guidance_mix', 'vocab_sample', 'vocab_reduce', 'embeds', 'critic_head_guided']
    assert names == per + (['topk_mask'] + per) * 2 + ['topk_mask'] + per[:4] + ['decode']
    embeds = [c for c in rec.calls if c[0] == 'embeds']
    for c in embeds:
        assert c[2]['replicas'] == J
        assert c[2]['context'].shape == (J * 2, Lmax, DCTX) and c[2]['text_mask'].shape == (J * 2, Lmax) and c[2]['text_mask'].dtype == torch.uint8
    ctx, tm = embeds[0][2]['context'], embeds[0][2]['text_mask']
    assert all(c[2]['context'] is ctx for c in embeds)                       # laid out once per call, shared by MaskGit and the critic
    own = weights.synthetic_context(2, 6, DCTX, seed=2)
    assert torch.equal(ctx[:2, :6], own) and (ctx[:2, 6:] == 0).all() and tm[:2, :6].all() and not tm[:2, 6:].any()
    if has_neg:
        assert torch.equal(ctx[-2:], weights.synthetic_context(2 if 'negative_texts' in kw and isinstance(kw['negative_texts'], list) else 1, 9, DCTX, seed=4).expand(2, -1, -1))
        assert tm[-2:].all()
    else:
        assert torch.equal(ctx[-2:], ctx[:2]) and not tm[-2:].any()           # the null base: cond_0's rows under an all-False mask
    cs = kw['cond_scale'] if isinstance(kw['cond_scale'], list) else [kw['cond_scale']] * 2
    weights_ = [w if isinstance(w, list) else [w, w] for _, w in kw.get('blend', [])]
    want = torch.from_numpy(G.table(cs, 4, kw.get('guidance_schedule'), weights_)[1])
    mixes = [c for c in rec.calls if c[0] == 'guidance_mix']
    heads = [c for c in rec.calls if c[0] == 'critic_head_guided']
    assert len(mixes) == 4 and len(heads) == 3
    for s, c in enumerate(mixes):                                             # the table's step row advances
        assert torch.equal(c[1][6], want[s]) and c[1][7:9] == (P_, True) and c[1][1] == 2
    for s, c in enumerate(heads):
        assert torch.equal(c[1][7], want[s]) and c[1][8:10] == (P_, True)
    assert mixes[1][1][6].data_ptr() != mixes[0][1][6].data_ptr()


def test_a_critic_without_cross_attention_keeps_critic_head(phenaki):
    phenaki.critic.has_cross_attn = False
    rec = Recorder()
    with recording(rec):
        phenaki.sample(num_frames=5, texts=['a', 'b'], cond_scale=[5., 2.5], negative_texts='bad')
    names = rec.names()
    assert names.count('guidance_mix') == 4 and names.count('critic_head') == 3 and 'critic_head_guided' not in names
    crit = [c for c in rec.calls if c[0] == 'critic_head']
    assert all(c[1][7] is False for c in crit)                                # no null half: one pass, no mix
    crit_embeds = [c for c in rec.calls if c[0] == 'embeds'][1::2]
    assert all(c[2]['replicas'] == 1 and c[2]['context'] is None for c in crit_embeds[:3])


def _refused(phenaki, match, **kw):
    rec = Recorder()
    args = dict(num_frames=5, texts=['a', 'b'])
    args.update(kw)
    with recording(rec), pytest.raises(ValueError, match=match):
        phenaki.sample(**args)
    assert rec.calls == [], f'{rec.names()} ran before the refusal'


def test_every_argument_error_is_raised_before_anything_is_called(phenaki):
    _refused(phenaki, 'cond_scale must hold 2', cond_scale=[5., 2.5, 1.])
    _refused(phenaki, 'cond_scale must hold 2', cond_scale=torch.tensor([5.]))
    _refused(phenaki, '1-D', cond_scale=torch.ones(2, 1))
    _refused(phenaki, 'finite', cond_scale=[5., float('nan')])
    _refused(phenaki, 'finite', cond_scale=[float('inf'), 1.])
    _refused(phenaki, 'guidance_schedule', guidance_schedule=[0.5] * 3)                                # steps = 4
    _refused(phenaki, 'guidance_schedule', guidance_schedule='cosine')
    _refused(phenaki, 'guidance_schedule', guidance_schedule=0.5)
    _refused(phenaki, 'finite', guidance_schedule=[0.5, 1., float('nan'), 1.])
    _refused(phenaki, 'negative_texts', negative_texts=['bad'])
    _refused(phenaki, 'negative_texts', negative_texts=['bad', 'bad', 'bad'])
    _refused(phenaki, 'negative_texts', negative_texts=[1, 2])
    _refused(phenaki, 'at most 2', blend=[('other', 0.1), ('bad', 0.1), ('worse', 0.1)])
    _refused(phenaki, r'blend\[0\] texts', blend=[(['other'], 0.1)])
    _refused(phenaki, r'blend\[1\] weight must hold 2', blend=[('other', 0.1), ('bad', [0.1, 0.2, 0.3])])
    _refused(phenaki, 'finite', blend=[('other', float('nan'))])
    _refused(phenaki, 'pair', blend=['other'])
    for kw in (dict(cond_scale=[3., 3.]), dict(guidance_schedule='linear'), dict(negative_texts='bad'), dict(blend=[('other', 0.5)])):
        _refused(phenaki, 'need texts', texts=None, batch_size=2, **kw)
    phenaki.maskgit.unconditional = phenaki.unconditional = True
    try:
        _refused(phenaki, 'conditional MaskGit', negative_texts='bad')
    finally:
        phenaki.maskgit.unconditional = phenaki.unconditional = False


# --------------------------------------------------------------------------- 5. sample_sharded

class _StubPhenaki:
    def __init__(self):
        self.calls = []

    def sample(self, **kw):
        self.calls.append(kw)
        return torch.zeros(kw['batch_size'], 1)


@pytest.mark.parametrize('rank,ws', [(0, 2), (1, 2), (2, 3)])
def test_sample_sharded_hands_each_rank_its_slice(monkeypatch, rank, ws):
    B = 5
    monkeypatch.setattr(PD, 'world', lambda: (rank, ws))
    lo, hi = PD.shard_batch(B, rank, ws)
    texts = [f't{i}' for i in range(B)]
    neg = [f'n{i}' for i in range(B)]
    bt = [f'b{i}' for i in range(B)]
    cs = [float(i) for i in range(B)]
    w = torch.arange(B, dtype=torch.float32) / 10
    stub = _StubPhenaki()
    PD.sample_sharded(stub, num_frames=5, texts=texts, gather=False, cond_scale=cs, negative_texts=neg, blend=[(bt, w), ('shared', 0.25)],
                      guidance_schedule='linear')
    kw = stub.calls[0]
    assert kw['texts'] == texts[lo:hi] and kw['batch_size'] == hi - lo
    assert kw['cond_scale'] == cs[lo:hi] and kw['negative_texts'] == neg[lo:hi]
    assert kw['blend'][0][0] == bt[lo:hi] and torch.equal(kw['blend'][0][1], w[lo:hi])
    assert kw['blend'][1] == ('shared', 0.25) and kw['guidance_schedule'] == 'linear'
    # values shared by the batch pass through as they are
    stub = _StubPhenaki()
    PD.sample_sharded(stub, num_frames=5, texts=texts, gather=False, cond_scale=4., negative_texts='n')
    assert stub.calls[0]['cond_scale'] == 4. and stub.calls[0]['negative_texts'] == 'n'
    stub = _StubPhenaki()
    PD.sample_sharded(stub, num_frames=5, texts=texts, gather=False, cond_scale=torch.tensor(cs))
    assert torch.equal(stub.calls[0]['cond_scale'], torch.tensor(cs[lo:hi]))


# --------------------------------------------------------------------------- 6. the graph key

def test_the_table_paths_graph_key_does_not_hold_the_scales(phenaki):
    keys = []
    for kw in (dict(cond_scale=[5., 2.5], guidance_schedule='linear', blend=[('other', 0.25)]),
               dict(cond_scale=[1.5, 7.75], guidance_schedule=[0.1, 0.2, 0.3, 0.4], blend=[('other', [0.5, 0.625])]),
               dict(cond_scale=9.5, blend=[('other', 0.)])):
        with recording(Recorder()):
            phenaki.sample(num_frames=5, texts=['a', 'b'], negative_texts='bad', **kw)
        keys.append(phenaki._pk_last_sample_key)
    assert keys[0] == keys[1] == keys[2]
    assert keys[0][6] == ('guided', 2, True, 9) and keys[0][5] == (6, 9, DCTX)
    flat = [v for item in keys[0] for v in (item if isinstance(item, tuple) else (item,))]
    scale_values = {5., 2.5, 1.5, 7.75, 9.5, 0.25, 0.625}
    assert not [v for v in flat if isinstance(v, float) and v in scale_values]
    # what changes the launches changes the key: another P, a negative prompt or not, another padded length
    with recording(Recorder()):
        phenaki.sample(num_frames=5, texts=['a', 'b'], cond_scale=[5., 2.5])
    assert phenaki._pk_last_sample_key[6] == ('guided', 1, False, 6) and phenaki._pk_last_sample_key != keys[0]
    with recording(Recorder()):
        phenaki.sample(num_frames=5, texts=['a', 'b'], cond_scale=[5., 2.5], negative_texts='other')
    assert phenaki._pk_last_sample_key[6] == ('guided', 1, True, 6)
