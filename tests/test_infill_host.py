"""Infilling on the CPU: the restatement against the oracle's plain sampler, the per-sample schedule, the pixel -> token reduction, every
ValueError of `sample(known_ids=, known_mask=)` / `infill` before any kernel wrapper is called, and which wrappers the loop calls with and
without known tokens (recorder stubs in place of the `_lib` wrappers, so no kernel runs)."""
import contextlib
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
from phenaki_pytorch_amd import phenaki as PH  # noqa: E402
from tests import infill_restatement as R  # noqa: E402

torch.set_grad_enabled(False)
GRID, N, V = (3, 4, 4), 48, TINY['maskgit']['num_tokens']


oracle_noise = R.oracle_noise


# --------------------------------------------------------------------------- 1. the restatement

@pytest.mark.parametrize('with_critic', [True, False])
def test_restatement_with_nothing_known_is_the_oracles_sampler(with_critic):
    cv_sd, mg_sd, cr_sd = state_dicts('tiny')
    cvc, mgc, crc = oracle_cfgs(TINY)
    ctx = weights.synthetic_context(2, 6, TINY['maskgit']['dim_context'], seed=2)
    cr = cr_sd if with_critic else None
    ref = []
    vid_ref, ids_ref = O.sample(cv_sd, cvc, mg_sd, mgc, cr, crc, num_frames=5, batch_size=2, context=ctx, steps=3, cond_scale=5.,
                                noise_fn=oracle_noise(40), trace=ref)
    got = []
    vid, ids = R.infill_sample(cv_sd, cvc, mg_sd, mgc, cr, crc, ids0=torch.zeros((2, N), dtype=torch.int64), known=torch.zeros((2, N), dtype=torch.bool),
                               patch_shape=GRID, steps=3, context=ctx, cond_scale=5., noise_fn=oracle_noise(40), trace=got)
    assert len(ref) == len(got) == 3
    for a, b in zip(ref, got):
        for key in ('masked_ids', 'mask', 'pred', 'ids'):
            assert torch.equal(a[key], b[key]), f"step {b['step']}: {key}"
        assert (a['scores'] is None) == (b['scores'] is None)
        if a['scores'] is not None:
            assert torch.equal(a['scores'], b['scores']), f"step {b['step']}: scores"
    assert torch.equal(ids_ref, ids) and torch.equal(vid_ref, vid)


def test_topk_mask_keep_restatement_by_hand():
    scores = np.array([[.5, .9, .9, .1, .9, .3]])
    known = np.array([[0, 1, 0, 0, 0, 0]], dtype=bool)                       # the best score sits on a known position: excluded by index
    r = R.topk_mask_keep(scores, [3], [2], known, 99, np.arange(6)[None], rows_out=np.full(7, R.SENTINEL))
    assert r['mask'].tolist() == [[1, 0, 1, 0, 1, 0]]                         # 2 and 4 tie at .9 (lower index first), then .5
    assert r['ids'].tolist() == [[99, 1, 99, 3, 99, 5]]
    assert r['rows_out'].tolist() == [R.SENTINEL, R.SENTINEL, 2, 4, 0, R.SENTINEL, R.SENTINEL]
    assert (r['scores_next'] == np.float32(-1e4)).all()
    r = R.topk_mask_keep(None, [2, 1], [0, 2], np.array([[1, 0, 0], [0, 0, 1]], dtype=bool), 9, np.zeros((2, 3)), rows_out=np.full(3, R.SENTINEL))
    assert r['mask'].tolist() == [[0, 1, 1], [1, 0, 0]] and r['rows_out'].tolist() == [1, 2, 3]


# --------------------------------------------------------------------------- 2. schedule, reduction

@pytest.mark.parametrize('free,steps', [((32, 36), 4), ((48, 1, 7, 48), 18), ((576,) * 3, 18)])
def test_schedule_is_the_mask_schedule_of_each_free_count(free, steps):
    ks, offs, totals = PH.infill_schedule(list(free), steps)
    assert len(ks) == len(offs) == len(totals) == steps
    for b, F in enumerate(free):
        want = PH.mask_schedule(F, steps)
        assert ks[0][b] == F
        assert [ks[s][b] for s in range(1, steps)] == want[1:]
        assert all(1 <= ks[s][b] <= F for s in range(steps))
    for s in range(steps):
        assert offs[s] == [sum(ks[s][:b]) for b in range(len(free))] and totals[s] == sum(ks[s])
    assert (ks, offs, totals) == R.schedule(list(free), steps)
    if len(set(free)) == 1:                                                   # nothing known: today's schedule
        assert [ks[s][0] for s in range(1, steps)] == PH.mask_schedule(free[0], steps)[1:]


@pytest.mark.parametrize('b', [1, 2])
def test_pixel_to_token_reduction_matches_brute_force(b):
    pt, ph, pw, F, H, W = 2, 4, 8, 5, 12, 16
    g = torch.Generator().manual_seed(3)
    pm = torch.rand((b, F, H, W), generator=g) < 0.02
    tm = PH.pixel_to_token_mask(pm, pt, (ph, pw))
    assert tm.shape == (b, 3, 3, 2) and tm.dtype == torch.bool
    assert torch.equal(tm, R.pixel_to_token_brute(pm, pt, ph, pw))
    assert tm.any() and not tm.all()
    # the first-frame rule: a pixel of frame 0 marks token frame 0 only; one of frame 1 or 2 marks token frame 1; 3 or 4 token frame 2
    for frame, tframe in ((0, 0), (1, 1), (2, 1), (3, 2), (4, 2)):
        one = torch.zeros((1, F, H, W), dtype=torch.bool)
        one[0, frame, 5, 9] = True
        tm = PH.pixel_to_token_mask(one, pt, (ph, pw))
        assert tm.nonzero().tolist() == [[0, tframe, 1, 1]]
        assert torch.equal(tm, R.pixel_to_token_brute(one, pt, ph, pw))
    # and back: the footprint of a token mask reduces to itself
    tm = torch.rand((b, 3, 3, 2), generator=g) < 0.4
    px = PH.token_to_pixel_mask(tm, pt, (ph, pw))
    assert px.shape == (b, F, H, W) and torch.equal(PH.pixel_to_token_mask(px, pt, (ph, pw)), tm)


# --------------------------------------------------------------------------- 3. dispatch and refusals, no kernel

WRAPPERS = ('topk_mask', 'topk_mask_keep', 'cfg_mix', 'vocab_sample', 'vocab_sample_philox', 'vocab_reduce', 'critic_head', 'composite_mask')


class Recorder:
    def __init__(self):
        self.calls = []

    def stub(self, name):
        def call(*args, **kwargs):
            self.calls.append((name, args, kwargs))
        return call

    def names(self):
        return [c[0] for c in self.calls]


@contextlib.contextmanager
def recording(rec):
    """the `_lib` wrappers of the sampling loop, the trunks, the tokenizer and the decoder replaced by recorders: sample() / infill() run on
    the CPU up to (and through) the loop without a kernel"""
    def embeds(self, ids, **kw):
        rec.calls.append(('embeds', (ids,), kw))
        return torch.zeros(1, self.dim if hasattr(self, 'dim') else 1)

    def decode(self, ids, _prime_indices=None):
        rec.calls.append(('decode', (ids,), {}))
        T = ids.shape[1] // self.image_num_tokens
        return torch.zeros(ids.shape[0], 3, 1 + (T - 1) * self.temporal_patch_size, *self.image_size)

    def tokenize(self, video, **kw):
        rec.calls.append(('tokenize', (video,), kw))
        f, h, w = self.get_video_patch_shape(video.shape[2])
        return (torch.arange(video.shape[0] * f * h * w) % V).reshape(video.shape[0], f, h, w)

    saved = [(L, k, getattr(L, k)) for k in WRAPPERS + ('require_device', 'vocab_ntiles')]
    saved += [(P.MaskGit, 'embeds', P.MaskGit.embeds), (P.TokenCritic, 'embeds', P.TokenCritic.embeds),
              (P.CViViT, 'decode_from_codebook_indices', P.CViViT.decode_from_codebook_indices), (P.CViViT, 'forward', P.CViViT.forward),
              (PH, 'linear_weight', PH.linear_weight)]
    try:
        for k in WRAPPERS:
            setattr(L, k, rec.stub(k))
        L.require_device = lambda t, name='tensor': None
        L.vocab_ntiles = lambda v: (v + 127) // 128
        P.MaskGit.embeds = embeds
        P.TokenCritic.embeds = embeds
        P.CViViT.decode_from_codebook_indices = decode
        P.CViViT.forward = tokenize
        PH.linear_weight = lambda lin, dt: lin.weight
        yield
    finally:
        for obj, k, v in saved:
            setattr(obj, k, v)


@pytest.fixture(scope='module')
def phenaki():
    torch.manual_seed(0)
    cv = P.CViViT(use_vgg_and_gan=False, **TINY['cvivit'])
    mg = P.MaskGit(**TINY['maskgit'])
    cr = P.TokenCritic(**TINY['critic'])
    return P.Phenaki(maskgit=mg, cvivit=cv, critic=cr, steps=4, text_embed_dim=TINY['maskgit']['dim_context']).eval()


def _known(B=2):
    known = torch.zeros((B, *GRID), dtype=torch.bool)
    known[0, 0] = True                                      # sample 0 keeps token frame 0: F = 32
    if B > 1:
        known[1, :, 1:3, 1:3] = True                        # sample 1 keeps a 2 x 2 block in every frame: F = 36
    ids0 = (torch.arange(B * N) * 7 % V).reshape(B, *GRID)
    return ids0, known


def test_plain_sample_makes_the_calls_it_always_made(phenaki):
    rec = Recorder()
    with recording(rec):
        phenaki.sample(num_frames=5, batch_size=2, _compact=True)
    names = rec.names()
    assert 'topk_mask_keep' not in names and names.count('topk_mask') == 3            # steps 1..3
    ks = PH.mask_schedule(N, 4)
    for s, c in enumerate(c for c in rec.calls if c[0] == 'topk_mask'):
        assert c[1][1:4] == (2, N, ks[s + 1])
    heads = [c for c in rec.calls if c[0] == 'vocab_sample']
    assert [c[1][4] for c in heads] == [2 * N] + [2 * k for k in ks[1:]]               # step 0: every row, rows = None
    assert heads[0][1][9] is None
    mixes = [c for c in rec.calls if c[0] == 'cfg_mix']
    assert mixes[0][1][4] is None and mixes[0][1][5] == 2 * N
    # per step: [topk_mask] embeds cfg_mix vocab_sample vocab_reduce [embeds critic_head]; then the decode
    per = ['embeds', 'cfg_mix', 'vocab_sample', 'vocab_reduce', 'embeds', 'critic_head']
    assert names == per + (['topk_mask'] + per) * 2 + ['topk_mask'] + per[:4] + ['decode']


@pytest.mark.parametrize('compact', [True, False])
def test_sample_with_known_tokens_takes_the_keep_kernel(phenaki, compact):
    ids0, known = _known()
    rec = Recorder()
    with recording(rec):
        phenaki.sample(num_frames=5, batch_size=2, known_ids=ids0, known_mask=known, _compact=compact)
    names = rec.names()
    assert 'topk_mask' not in names and names.count('topk_mask_keep') == 4            # step 0 too: it lays down mask, ids and the row list
    ks, offs, totals = PH.infill_schedule([32, 36], 4)
    assert totals[0] == 68
    keeps = [c for c in rec.calls if c[0] == 'topk_mask_keep']
    for s, c in enumerate(keeps):
        scores, B, n, k_dev, off_dev, kn = c[1][:6]
        assert (scores is None) == (s == 0) and (B, n) == (2, N)
        assert k_dev.dtype == torch.int32 and k_dev.tolist() == ks[s] and off_dev.tolist() == offs[s]
        assert kn.dtype == torch.uint8 and torch.equal(kn.bool(), known.reshape(2, N))
        assert (c[1][9] is not None) == compact
    heads = [c for c in rec.calls if c[0] == 'vocab_sample']
    assert [c[1][4] for c in heads] == (totals if compact else [2 * N] * 4)           # step 0's head: M = sum F_b = 68 rows, not B n = 96
    assert all((c[1][9] is not None) == compact for c in heads)
    for name, m_at in (('cfg_mix', 5), ('vocab_reduce', 1)):
        assert [c[1][m_at] for c in rec.calls if c[0] == name] == (totals if compact else [2 * N] * 4)
    # the loop starts from the caller's ids (the kernel of step 0 masks the free ones)
    first_ids = [c for c in rec.calls if c[0] == 'embeds'][0][1][0]
    assert first_ids.shape == (2, N)


def test_a_mask_shared_by_the_batch_and_flat_shapes(phenaki):
    ids0, known = _known()
    for km, ki in ((known[0], ids0), (known[0].reshape(N), ids0.reshape(2, N)), (known.reshape(2, N), ids0)):
        rec = Recorder()
        with recording(rec):
            phenaki.sample(num_frames=5, batch_size=2, known_ids=ki, known_mask=km)
        kn = [c for c in rec.calls if c[0] == 'topk_mask_keep'][0][1][5]
        want = known.reshape(2, N) if km.shape[0] == 2 and km.ndim != 3 else known[0].reshape(1, N).expand(2, N)
        assert torch.equal(kn.bool(), want)


def _refused(phenaki, match, **kw):
    rec = Recorder()
    args = dict(num_frames=5, batch_size=2)
    args.update(kw)
    with recording(rec), pytest.raises(ValueError, match=match):
        phenaki.sample(**args)
    assert rec.calls == [], f'{rec.names()} ran before the refusal'


def test_every_argument_error_is_raised_before_anything_is_called(phenaki):
    ids0, known = _known()
    _refused(phenaki, 'together', known_ids=ids0)
    _refused(phenaki, 'together', known_mask=known)
    _refused(phenaki, 'prime_frames', known_ids=ids0, known_mask=known, prime_frames=torch.zeros(2, 3, 3, 64, 64))
    _refused(phenaki, 'known_ids must be', known_ids=ids0[:1], known_mask=known)                       # batch
    _refused(phenaki, 'known_ids must be', known_ids=ids0[:, :2], known_mask=known)                    # grid
    _refused(phenaki, 'known_ids must be', known_ids=ids0[0], known_mask=known)                        # ids are never shared
    _refused(phenaki, 'known_mask must be', known_ids=ids0, known_mask=known[:, :2])
    _refused(phenaki, 'known_mask must be', known_ids=ids0, known_mask=known.reshape(2, 3, 16))
    _refused(phenaki, 'known_ids must be', known_ids=ids0, known_mask=known, num_frames=7)             # another clip length
    _refused(phenaki, 'int64', known_ids=ids0.int(), known_mask=known)
    _refused(phenaki, 'int64', known_ids=ids0.float(), known_mask=known)
    _refused(phenaki, 'bool', known_ids=ids0, known_mask=known.to(torch.uint8))
    _refused(phenaki, 'tensors', known_ids=ids0.tolist(), known_mask=known)
    bad = ids0.clone()
    bad[1, 0, 1, 1] = V                                                                                # the mask id itself, at a KNOWN position
    _refused(phenaki, 'outside', known_ids=bad, known_mask=known)
    bad[1, 0, 1, 1] = -1
    _refused(phenaki, 'outside', known_ids=bad, known_mask=known)
    full = known.clone()
    full[1] = True
    _refused(phenaki, 'at least one token', known_ids=ids0, known_mask=full)
    # out-of-range ids at FREE positions are nobody's business: they are masked before the trunk sees them
    free_bad = ids0.clone()
    free_bad[0, 1, 0, 0] = V + 5
    rec = Recorder()
    with recording(rec):
        phenaki.sample(num_frames=5, batch_size=2, known_ids=free_bad, known_mask=known)
    assert 'topk_mask_keep' in rec.names()


def test_the_wrapper_refuses_k_above_the_free_count():
    B, n = 2, 8
    z = lambda dt, *s: torch.zeros(s, dtype=dt)
    with pytest.raises(ValueError, match='free count'):
        L.topk_mask_keep(None, B, n, z(torch.int32, B), z(torch.int32, B), z(torch.uint8, B, n), 9, z(torch.uint8, B, n), z(torch.int64, B, n),
                         k_host=[3, 5], free_host=[8, 4])
    with pytest.raises(ValueError, match='k must be'):
        L.topk_mask_keep(None, B, n, z(torch.int64, B), z(torch.int32, B), None, 9, z(torch.uint8, B, n), z(torch.int64, B, n))


def test_infill_builds_the_known_tokens_and_composites(phenaki):
    video = torch.zeros(2, 3, 5, 64, 64)
    edit = torch.zeros((1, 5, 64, 64), dtype=torch.bool)
    edit[0, :, :, 32:] = True                                                   # outpaint the right half
    rec = Recorder()
    with recording(rec):
        out = phenaki.infill(video, edit, composite=True)
    assert out.shape == video.shape
    names = rec.names()
    assert names[0] == 'tokenize' and names[-2:] == ['decode', 'composite_mask'] and 'topk_mask' not in names
    kn = [c for c in rec.calls if c[0] == 'topk_mask_keep'][0][1][5].bool().reshape(2, *GRID)
    assert kn[:, :, :, :2].all() and not kn[:, :, :, 2:].any()
    comp = [c for c in rec.calls if c[0] == 'composite_mask'][0][1]
    assert comp[2].dtype == torch.uint8 and torch.equal(comp[2].bool(), edit)
    # a token mask: its footprint is the pixel mask of the composite
    tedit = torch.zeros((2, *GRID), dtype=torch.bool)
    tedit[:, 1] = True                                                          # interpolate token frame 1 = video frames 1 and 2
    rec = Recorder()
    with recording(rec):
        phenaki.infill(video, tedit, mask_level='token', composite=True)
    comp = [c for c in rec.calls if c[0] == 'composite_mask'][0][1]
    want = torch.zeros((2, 5, 64, 64), dtype=torch.bool)
    want[:, 1:3] = True
    assert torch.equal(comp[2].bool(), want)
    for bad_kw, match in ((dict(mask_level='frame'), 'mask_level'), (dict(mask_level='token'), 'edit_mask must be'),
                          (dict(prime_frames=video), 'not arguments')):
        rec = Recorder()
        with recording(rec), pytest.raises(ValueError, match=match):
            phenaki.infill(video, edit, **bad_kw)
        assert rec.calls == []
    rec = Recorder()
    with recording(rec), pytest.raises(ValueError, match='bool'):
        phenaki.infill(video, edit.float())
    assert rec.calls == []


# --------------------------------------------------------------------------- 4. the noise seed of the GPU parity test

def test_the_parity_seed_has_no_near_tie_between_f32_and_float64():
    """tests/test_infill_gpu.py teacher-forces the product with this file's restatement at R.PARITY_SEED; the seed is admissible when the f32
    restatement and a float64 run of itself, teacher-forced with the f32 run's inputs, pick the same token at every masked position"""
    for with_critic in (True, False):
        assert R.f32_vs_f64_flips(R.parity_case(with_critic), R.PARITY_SEED) == 0
