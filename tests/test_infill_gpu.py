"""Infilling on the MI355X (-m gpu): pk_topk_mask_keep bit for bit against its restatement (tests/infill_restatement.py), pk_composite_mask, the
sampling loop with known tokens at the TINY geometry (B = 2, n = 48, grid (3, 4, 4), 4 steps; sample 0 keeps token frame 0, F = 32, sample 1
keeps a 2 x 2 block in every frame, F = 36) and `Phenaki.infill`."""
import functools

import numpy as np
import pytest
import torch

from oracle import weights
from oracle.configs import TINY
from phenaki_pytorch_amd import _lib as L
from phenaki_pytorch_amd import phenaki as PH
from tests import infill_restatement as R
from tests.util import argmax_equal_with_margin, load_product, noise_fn_cuda

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

OK, EINVAL = 0, -1
MASK_ID = 1 << 40
SENT = R.SENTINEL
STEPS, GRID, N, V = R.PARITY_STEPS, R.PARITY_GRID, 48, TINY['maskgit']['num_tokens']
SEED = 0x1234567812345678 & 0x3FFFFFFFFFFFFFFF


@pytest.fixture(scope='module')
def lib():
    from phenaki_pytorch_amd import build
    build.build(verbose=False)
    lib = L.load()
    assert lib.pk_topk_mask_keep(None, 1, 1, None, None, None, 0, None, None, None, None, None) == EINVAL
    return lib


def stream():
    return torch.cuda.current_stream().cuda_stream


# ------------------------------------------------------------------------------------------------ pk_topk_mask_keep

def _known_with_free(n, free_counts, seed):
    g = np.random.default_rng(seed)
    known = np.ones((len(free_counts), n), dtype=bool)
    for b, F in enumerate(free_counts):
        known[b, g.permutation(n)[:F]] = False
    return known


def _quantised(B, n, seed, levels=4):
    return (np.random.default_rng(seed).integers(0, levels, (B, n)) / np.float32(levels)).astype(np.float32)


def _offsets(k):
    return [int(sum(k[:b])) for b in range(len(k))]


def _run_keep(scores, k, known, n, *, rows=True, nxt=True, off=None):
    """the kernel on sentinel-filled outputs against the restatement: mask, ids, rows_out (with its untouched tail and gaps) and scores_next"""
    B = len(k)
    off = _offsets(k) if off is None else off
    ids0 = np.arange(B * n, dtype=np.int64).reshape(B, n) + 1000
    total = max(o + kk for o, kk in zip(off, k)) + 5
    ref = R.topk_mask_keep(scores, k, off, known, MASK_ID, ids0, rows_out=np.full(total, SENT, dtype=np.int32) if rows else None)
    dev = lambda a, dt: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dt).cuda()
    mask = torch.full((B, n), 7, dtype=torch.uint8, device='cuda')
    ids = dev(ids0, torch.int64)
    rows_out = torch.full((total,), SENT, dtype=torch.int32, device='cuda') if rows else None
    scores_next = torch.full((B, n), 3., device='cuda') if nxt else None
    L.topk_mask_keep(dev(scores, torch.float32), B, n, dev(np.array(k), torch.int32), dev(np.array(off), torch.int32), dev(known, torch.uint8), MASK_ID,
                     mask, ids, rows_out, scores_next, k_host=k, free_host=[n] * B if known is None else (~known).sum(1).tolist())
    torch.cuda.synchronize()
    assert torch.equal(mask.cpu(), torch.from_numpy(ref['mask'])), 'mask'
    assert torch.equal(ids.cpu(), torch.from_numpy(ref['ids'])), 'ids (mask_id where masked, untouched elsewhere)'
    if rows:
        assert torch.equal(rows_out.cpu(), torch.from_numpy(ref['rows_out'])), 'rows_out (rank order, nothing outside [row_off, row_off + k))'
    if nxt:
        assert torch.equal(scores_next.cpu().view(torch.int32), torch.from_numpy(ref['scores_next']).view(torch.int32)), 'scores_next = -1e4 everywhere'
    if known is not None:
        assert not (mask.cpu().numpy().astype(bool) & known).any()
    return mask, ids, rows_out, scores_next


@pytest.mark.parametrize('with_scores', [True, False])
def test_keep_kernel_block_plus_tail_ties_decide(lib, with_scores):
    """B = 3, n = 70 (a 64-position block plus a tail), F = (70, 1, 37), k = (5, 1, 37); scores on 4 levels, or none at all"""
    known = _known_with_free(70, (70, 1, 37), seed=1)
    scores = _quantised(3, 70, seed=2) if with_scores else None
    _run_keep(scores, [5, 1, 37], known, 70)
    _run_keep(scores, [5, 1, 37], known, 70, rows=False, nxt=False)
    _run_keep(scores, [5, 1, 37], known, 70, off=[40, 0, 3])                       # offsets in any order, gaps stay untouched
    if with_scores:
        # excluded by index, not by value: the known positions hold the LARGEST scores of their rows
        s = scores.copy()
        s[known] = 9.
        _run_keep(s, [5, 1, 37], known, 70)
        s[known] = np.inf
        _run_keep(s, [5, 1, 37], known, 70)


@pytest.mark.parametrize('n', [9, 1])
def test_keep_kernel_small_rows(lib, n):
    free = (n, 1, max(n // 2, 1), 0)
    known = _known_with_free(n, free, seed=3)
    for k in (list(free), [1, 1, 1, 0], [0, 0, 0, 0]):
        _run_keep(_quantised(4, n, seed=4), k, known, n)
        _run_keep(None, k, known, n)


def test_keep_kernel_one_row_of_576(lib):
    known = _known_with_free(576, (288,), seed=5)
    _run_keep(_quantised(1, 576, seed=6, levels=16), [144], known, 576)
    _run_keep(np.random.default_rng(7).standard_normal((1, 576)).astype(np.float32), [288], known, 576)
    _run_keep(None, [288], known, 576)


@pytest.mark.parametrize('B,n,k', [(3, 70, 5), (2, 9, 9), (1, 576, 288), (2, 1, 1)])
def test_keep_kernel_without_known_is_topk_mask(lib, B, n, k):
    scores = torch.from_numpy(_quantised(B, n, seed=8)).cuda()
    outs = []
    for keep in (False, True):
        mask = torch.full((B, n), 7, dtype=torch.uint8, device='cuda')
        ids = torch.arange(B * n, device='cuda').reshape(B, n) + 1000
        rows = torch.full((B * k + 3,), SENT, dtype=torch.int32, device='cuda')
        nxt = torch.full((B, n), 3., device='cuda')
        if keep:
            kd = torch.full((B,), k, dtype=torch.int32, device='cuda')
            L.topk_mask_keep(scores, B, n, kd, torch.arange(B, dtype=torch.int32, device='cuda') * k, None, MASK_ID, mask, ids, rows, nxt)
        else:
            L.topk_mask(scores, B, n, k, MASK_ID, mask, ids, rows, scores_next=nxt)
        outs.append((mask, ids, rows, nxt.view(torch.int32)))
    for a, b, what in zip(outs[0], outs[1], ('mask', 'ids', 'rows_out', 'scores_next')):
        assert torch.equal(a, b), what


def test_keep_kernel_refusals_write_nothing(lib):
    B, n = 2, 5
    scores = torch.zeros((B, n), device='cuda')
    k = torch.ones((B,), dtype=torch.int32, device='cuda')
    off = torch.arange(B, dtype=torch.int32, device='cuda')
    known = torch.zeros((B, n), dtype=torch.uint8, device='cuda')
    mask = torch.full((B, n), 7, dtype=torch.uint8, device='cuda')
    ids = torch.full((B, n), SENT, dtype=torch.int64, device='cuda')
    rows = torch.full((B * n,), SENT, dtype=torch.int32, device='cuda')
    nxt = torch.full((B, n), 3., device='cuda')
    p = lambda t: None if t is None else t.data_ptr()
    good = dict(scores=scores, B=B, n=n, k=k, off=off, known=known, mask=mask, ids=ids, rows=rows, nxt=nxt)

    def call(**kw):
        a = dict(good)
        a.update(kw)
        return lib.pk_topk_mask_keep(p(a['scores']), a['B'], a['n'], p(a['k']), p(a['off']), p(a['known']), MASK_ID, p(a['mask']), p(a['ids']), p(a['rows']),
                                     p(a['nxt']), stream())
    for bad in (dict(k=None), dict(mask=None), dict(ids=None), dict(B=0), dict(B=-1), dict(n=0), dict(n=-3), dict(off=None), dict(n=12289),
                dict(nxt=scores)):
        assert call(**bad) == EINVAL, bad
    torch.cuda.synchronize()
    assert (mask == 7).all() and (ids == SENT).all() and (rows == SENT).all() and (nxt == 3.).all() and (scores == 0).all()
    assert call(off=None, rows=None) == OK and call(scores=None, known=None) == OK     # row_off only matters with rows_out; NULL scores / known are forms
    torch.cuda.synchronize()


# ------------------------------------------------------------------------------------------------ pk_composite_mask

@pytest.mark.parametrize('mb', [1, 2])
def test_composite_mask_is_a_select(lib, mb):
    g = torch.Generator().manual_seed(9)
    shape = (2, 3, 5, 6, 7)                                                       # odd sizes: 210 pixels per channel
    gen, src = torch.randn(shape, generator=g).cuda(), torch.randn(shape, generator=g).cuda()
    src[0, 0, 0, 0, :4] = torch.tensor([float('nan'), float('inf'), -0., 1e-42])  # bits, not values
    m = (torch.rand((mb, 5, 6, 7), generator=g) < 0.4).cuda()
    out = torch.full(shape, 5., device='cuda')
    L.composite_mask(gen, src, m.to(torch.uint8), out)
    want = torch.where(m[:, None], gen, src)
    assert torch.equal(out.view(torch.int32), want.view(torch.int32))
    z = torch.zeros_like(m, dtype=torch.uint8)
    assert lib.pk_composite_mask(gen.data_ptr(), src.data_ptr(), z.data_ptr(), out.data_ptr(), 2, 3, 210, 3, stream()) == EINVAL
    assert lib.pk_composite_mask(gen.data_ptr(), src.data_ptr(), None, out.data_ptr(), 2, 3, 210, 1, stream()) == EINVAL


# ------------------------------------------------------------------------------------------------ the loop, TINY

@functools.lru_cache(maxsize=None)
def _product(with_critic, dtype='fp32'):
    _, _, _, ph = load_product('tiny', TINY, with_critic=with_critic, steps=STEPS, dtype=dtype)
    ctx = weights.synthetic_context(2, 6, TINY['maskgit']['dim_context'], seed=2)
    ph.encode_texts = lambda texts, output_device=None: ctx.cuda()
    return ph


def _case(which=0):
    """(ids0, known) of the module docstring; which = 1: another mask with the SAME free counts (32, 36)"""
    ids0, known = R.parity_known()
    if which == 1:
        known = torch.zeros((2, *GRID), dtype=torch.bool)
        known[0, 2] = True
        known[1, :, 0:2, 0:2] = True
        known = known.reshape(2, N)
    assert (~known).sum(1).tolist() == [32, 36]
    return ids0.cuda(), known.cuda()


KW = dict(texts=['a', 'b'], num_frames=5, cond_scale=5., _return_ids=True)


def _check_invariants(trace, ids, ids0, known):
    """invariant 2 of the issue, at every step"""
    ks, _, _ = PH.infill_schedule([32, 36], STEPS)
    assert len(trace) == STEPS
    for s, t in enumerate(trace):
        assert torch.equal(t['masked_ids'][known], ids0[known]) and torch.equal(t['ids'][known], ids0[known]), f'step {s}: a known id changed'
        assert not (t['mask'] & known).any(), f'step {s}: a known position is masked'
        assert t['mask'].sum(1).tolist() == ks[s], f'step {s}: masked counts'
        assert torch.equal(t['masked_ids'] == V, t['mask']), f'step {s}: mask_id exactly at the masked positions'
    assert not (ids == V).any() and ((ids >= 0) & (ids < V)).all() and torch.equal(ids[known], ids0[known])


@pytest.mark.parametrize('with_critic', [True, False])
def test_nothing_known_is_plain_sample(with_critic):
    ph = _product(with_critic)
    none = dict(known_ids=torch.zeros((2, N), dtype=torch.int64), known_mask=torch.zeros((N,), dtype=torch.bool))
    vid_p, ids_p = ph.sample(_seed=SEED, **KW)
    vid_k, ids_k = ph.sample(_seed=SEED, **none, **KW)
    assert torch.equal(ids_p, ids_k) and torch.equal(vid_p, vid_k), 'eager'
    ph.enable_sample_graph(True)
    try:
        for _ in range(2):                                                        # capture, then a pure replay
            vid_g, ids_g = ph.sample(_seed=SEED, **none, **KW)
            assert torch.equal(ids_p, ids_g) and torch.equal(vid_p, vid_g), 'graph'
        assert torch.equal(ph.sample(_seed=SEED, **KW)[1], ids_p)                  # the plain graph, next to the infilling one
        assert len(ph.__dict__['_pk_sample_graphs']) == 2
    finally:
        ph.enable_sample_graph(False)


@pytest.mark.parametrize('with_critic', [True, False])
def test_known_tokens_stay_and_counts_follow_the_schedule(with_critic):
    ph = _product(with_critic)
    ids0, known = _case()
    trace = []
    _, ids = ph.sample(_seed=SEED, known_ids=ids0.reshape(2, *GRID), known_mask=known.reshape(2, *GRID), _trace=trace, **KW)
    _check_invariants(trace, ids, ids0, known)
    # row compaction on or off: the same ids
    outs = [ph.sample(_seed=SEED, known_ids=ids0, known_mask=known, _compact=c, **KW) for c in (True, False)]
    assert torch.equal(outs[0][1], outs[1][1]) and torch.equal(outs[0][1], ids) and torch.equal(outs[0][0], outs[1][0])


@pytest.mark.parametrize('compact', [True, False])
@pytest.mark.parametrize('with_critic', [True, False])
def test_free_running_remasking_is_the_restated_topk_of_its_own_scores(with_critic, compact):
    """the product's recorded scores of step s, through the restated top-k with exclusion, give its recorded mask and masked ids of step s + 1"""
    ph = _product(with_critic)
    ids0, known = _case()
    trace = []
    ph.sample(_seed=SEED + 1, known_ids=ids0, known_mask=known, _trace=trace, _compact=compact, **KW)
    ks, offs, _ = PH.infill_schedule([32, 36], STEPS)
    for s in range(STEPS - 1):
        r = R.topk_mask_keep(trace[s]['scores'].cpu().numpy(), ks[s + 1], offs[s + 1], known.cpu().numpy(), V, trace[s]['ids'].cpu().numpy())
        assert torch.equal(trace[s + 1]['mask'].cpu(), torch.from_numpy(r['mask']).bool()), f'mask of step {s + 1}'
        assert torch.equal(trace[s + 1]['masked_ids'].cpu(), torch.from_numpy(r['ids'])), f'masked ids of step {s + 1}'
    if not with_critic:
        assert all((t['scores'][~t['mask']] == -1e4).all() for t in trace[:-1])


@functools.lru_cache(maxsize=None)
def _restated(with_critic):
    return R.run_parity_case(R.parity_case(with_critic), R.PARITY_SEED)[0]


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
@pytest.mark.parametrize('with_critic', [True, False])
def test_teacher_forced_parity_with_the_restatement(with_critic, dtype):
    """every step's input is the restatement's recorded one; the predictions at the masked positions are the restatement's, or a near tie by its
    own noisy logits (argmax_equal_with_margin, tol 1e-4).  Noise: tests.util.noise_fn_cuda(R.PARITY_SEED), PARITY_SEED = 700 -- chosen on the
    CPU so that the f32 restatement against a float64 run of itself (teacher-forced alike) has no flip at any masked position, with and without
    critic; tests/test_infill_host.py asserts that (R.f32_vs_f64_flips == 0)."""
    ref = _restated(with_critic)
    ph = _product(with_critic, dtype)
    ids0, known = _case()

    def force(step, ids, mask):
        ids.copy_(ref[step]['masked_ids'].cuda())
        mask.copy_(ref[step]['mask'].to(mask.dtype).cuda())

    trace = []
    ph.sample(known_ids=ids0, known_mask=known, _noise_fn=noise_fn_cuda(R.PARITY_SEED), _trace=trace, _force_fn=force, **KW)
    assert len(trace) == STEPS
    flips = 0
    for s, (r, t) in enumerate(zip(ref, trace)):
        assert torch.equal(t['masked_ids'].cpu(), r['masked_ids']) and torch.equal(t['mask'].cpu(), r['mask'])
        flips += argmax_equal_with_margin(t['pred'], r['pred'], r['noisy'], tol=1e-4, what=f'{dtype} step {s} pred', rows=r['mask'])
        assert torch.equal(t['ids'].cpu()[known.cpu()], ids0.cpu()[known.cpu()])
    print(f'teacher-forced infill ({dtype}, critic {with_critic}): {flips} audited near-tie flips over {STEPS} steps')


def test_graph_replays_another_mask_with_the_same_counts():
    ph = _product(True)
    eager = []
    for which in (0, 1):
        ids0, known = _case(which)
        trace = []
        _, ids = ph.sample(_seed=SEED + which, known_ids=ids0, known_mask=known, _trace=trace, _compact=True, **KW)
        _check_invariants(trace, ids, ids0, known)
        eager.append(ids)
    ph.enable_sample_graph(True)
    try:
        graphs = None
        for which in (0, 1, 0):
            ids0, known = _case(which)
            vid, ids = ph.sample(_seed=SEED + which, known_ids=ids0, known_mask=known, **KW)
            assert torch.equal(ids, eager[which]), f'mask {which}: the replayed loop and the eager one (whose every step was checked) differ'
            assert vid.shape == (2, 3, 5, 64, 64)
            held = {k: e['graph'] for k, e in ph.__dict__['_pk_sample_graphs'].items()}
            assert len(held) == 1
            assert graphs is None or all(held[k] is graphs[k] for k in held), 'the same counts captured again'
            graphs = held
        # other counts: another configuration
        ids0, known = _case()
        known = known.clone()
        known[0, 47] = True
        ph.sample(_seed=SEED, known_ids=ids0, known_mask=known, **KW)
        assert len(ph.__dict__['_pk_sample_graphs']) == 2
    finally:
        ph.enable_sample_graph(False)


# ------------------------------------------------------------------------------------------------ infill

def test_infill_pixel_mask_and_composite():
    ph = _product(True)
    video = weights.synthetic_video(2, 5, 64, 64, seed=4).cuda()
    edit = torch.zeros((1, 5, 64, 64), dtype=torch.bool)
    edit[0, :, 3:40, 30:64] = True                                              # not on the patch grid: the tokens of columns 1 .. 3, rows 0 .. 2
    out = ph.infill(video, edit, texts=['a', 'b'], cond_scale=5., _seed=SEED)
    assert out.shape == video.shape and torch.isfinite(out).all()
    mixed, ids = ph.infill(video, edit, texts=['a', 'b'], cond_scale=5., _seed=SEED, composite=True, _return_ids=True)
    e = edit.cuda().expand(2, -1, -1, -1)[:, None].expand_as(video)
    assert torch.equal(mixed[~e].view(torch.int32), video[~e].view(torch.int32)), 'pixels outside the mask are the input, bit for bit'
    assert torch.equal(mixed[e], out[e])
    tok = ph.cvivit(video, return_only_codebook_ids=True)
    kept = ~PH.pixel_to_token_mask(edit, 2, (16, 16)).cuda().expand(2, -1, -1, -1)
    assert kept.sum().item() == 2 * (48 - 3 * 3 * 3)
    assert torch.equal(ids.reshape(2, *GRID)[kept], tok[kept])


def test_infill_token_mask_keeps_the_tokenizers_ids():
    ph = _product(False)
    video = weights.synthetic_video(2, 5, 64, 64, seed=5).cuda()
    tedit = torch.zeros((2, *GRID), dtype=torch.bool)
    tedit[0, 1] = True                                                          # interpolate the middle token frame of sample 0
    tedit[1, 1:] = True                                                         # extend sample 1 from its first frame
    out, ids = ph.infill(video, tedit, mask_level='token', _seed=SEED, _return_ids=True)
    assert out.shape == video.shape
    tok = ph.cvivit(video, return_only_codebook_ids=True)
    keep = ~tedit.cuda()
    assert torch.equal(ids.reshape(2, *GRID)[keep], tok[keep]) and not (ids == V).any()
    mixed = ph.infill(video, tedit, mask_level='token', _seed=SEED, composite=True)
    px = PH.token_to_pixel_mask(tedit, 2, (16, 16)).cuda()[:, None].expand_as(video)
    assert torch.equal(mixed[~px].view(torch.int32), video[~px].view(torch.int32)) and torch.equal(mixed[px], out[px])
