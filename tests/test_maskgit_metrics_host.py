"""CPU-only checks of the MaskGIT validation metrics: the float64 restatement (tests/maskgit_metrics_restatement.py) against torch's own
cross entropy, Categorical entropy and a sort-based rank; the refusals that happen before any launch; the MaskGitMetrics accumulator and its
merge over two gloo ranks, fed recorded `Phenaki.evaluate` dicts; the new symbols in the header and in _lib's table.  No kernel is launched.

The first section exercises the restatement alone: it guards the REFERENCE the GPU tests compare with.  The others need the product."""
import math
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from tests import maskgit_metrics_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement against torch's own formulations ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('M, V, scale, seed', [(7, 5, 1., 1), (33, 300, 4., 2), (64, 1000, 12., 3)])
def test_restatement_against_torch(M, V, scale, seed):
    g = R.g(seed)
    logits = torch.randn(M, V, generator=g, dtype=torch.float64) * scale
    tg = torch.randint(0, V, (M,), generator=g)
    s = R.head_stats(logits, tg, 2e-5)
    assert float((s['nll'] - F.cross_entropy(logits, tg, reduction='none')).abs().max()) < 1e-12
    assert float((s['lse'] - torch.logsumexp(logits, dim=1)).abs().max()) < 1e-12
    assert float((s['entropy'] - torch.distributions.Categorical(logits=logits).entropy()).abs().max()) < 1e-11
    order = logits.argsort(dim=1, descending=True, stable=True)
    position = (order == tg[:, None]).float().argmax(dim=1)             # continuous draws: no ties, the sort position IS the rank
    assert torch.equal(s['rank'], position) and torch.equal(s['pred'], order[:, 0])
    assert bool((s['rank_lo'] <= s['rank']).all()) and bool((s['rank'] <= s['rank_hi']).all())
    assert s['eps'] == 2e-5 * float(logits.abs().max())


def test_rank_leaves_the_target_out_by_index_and_counts_strictly():
    logits = torch.tensor([[1., 3., 3., 0., 3.], [2., 2., 2., 2., 2.], [0., 1., 2., 3., 4.]], dtype=torch.float64)
    s = R.head_stats(logits, torch.tensor([2, 3, 0]), 0.1)
    assert s['rank'].tolist() == [0, 0, 4]                              # ties with the target are not "greater"
    assert s['pred'].tolist() == [1, 0, 4]                              # first maximum
    assert s['rank_hi'].tolist() == [2, 4, 4] and s['rank_lo'].tolist() == [0, 0, 4] and abs(s['eps'] - 0.4) < 1e-15
    assert abs(float(s['entropy'][1]) - math.log(5)) < 1e-12 and abs(float(s['nll'][1]) - math.log(5)) < 1e-12


def test_planted_targets_of_the_gpu_cases():
    """the small GPU cases: the planted rows sit at rank 0, 2, 4, 5 in turn, a row targets column 0 and one the last tile; the share of planted rows
    whose rank the inputs determine is the condition the GPU test asserts (here: measured for the two small shapes, every mode)"""
    for mode in ('fp32', 'bf16x3', 'bf16'):
        for M, V, D, with_rows in R.CASES[:2]:
            c = R.make_case(mode, M, V, D, with_rows)
            s, p = c['stats'], c['planted']
            assert s['rank'][:p].tolist() == [R.PLANT[m % 4] for m in range(p)]
            assert int((c['tg'] == 0).sum()) >= 1 and int((c['tg'] >= (V - 1) // 128 * 128).sum()) >= 1
            assert float((s['rank_lo'][:p] == s['rank_hi'][:p]).float().mean()) >= 0.95
            if with_rows:
                assert c['targets_full'].numel() == 2 * M + 5 and torch.equal(c['targets_full'][c['rows'].long()], c['tg'])


def test_pooled_numbers():
    s = dict(nll=torch.tensor([1., 3.]), entropy=torch.tensor([0.5, 1.5]), rank=torch.tensor([0, 7]))
    x, y = torch.tensor([[2., -1., 0.5]]), torch.tensor([[True, False, False]])
    p = R.pooled([s, s], [(x, y), (x, y)])
    assert p['tokens'] == 4 and p['loss'] == 2. and abs(p['perplexity'] - math.exp(2.)) < 1e-12 and p['entropy'] == 1.
    assert (p['top1'], p['top5'], p['top10'], p['mean_rank']) == (0.5, 0.5, 1., 3.5) and abs(p['mrr'] - (1 + 1 / 8) / 2) < 1e-15
    assert abs(p['critic_bce'] - float(F.binary_cross_entropy_with_logits(x.double(), y.double()))) < 1e-12
    assert abs(p['critic_accuracy'] - 2 / 3) < 1e-15 and abs(p['critic_positive_share'] - 1 / 3) < 1e-15


# ---- refusals before any launch -------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def no_launch(monkeypatch):
    """any attempt to reach the library fails the test"""
    from phenaki_pytorch_amd import _lib

    def boom(*a, **k):
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'load', boom)


def test_vocab_eval_refusals(no_launch):
    from phenaki_pytorch_amd import _lib as L
    M, V, D = 4, 8, 32
    A, W, b = torch.zeros(M, D), torch.zeros(V, D), torch.zeros(V)
    tg = torch.zeros(M, dtype=torch.int64)
    call = lambda *a, **k: L.vocab_eval(*a, **k)
    with pytest.raises(ValueError, match='compute dtype'):
        call(7, A, W, b, M, V, D, tg, None)
    with pytest.raises(ValueError, match='A must be'):
        call(L.BF16, A, W, b, M, V, D, tg, None)                        # f32 rows handed to the bf16 kernel
    with pytest.raises(ValueError, match='A must be'):
        call(L.F32, A.t().contiguous().t(), W, b, M, V, D, tg, None)    # column stride
    with pytest.raises(ValueError, match='W must be'):
        call(L.F32, A, W[:4], b, M, V, D, tg, None)
    with pytest.raises(ValueError, match='targets must be'):
        call(L.F32, A, W, b, M, V, D, tg.int(), None)
    with pytest.raises(ValueError, match='targets must be'):
        call(L.F32, A, W, b, M, V, D, tg[:3], None)
    with pytest.raises(ValueError, match='rows must be'):
        call(L.F32, A, W, b, M, V, D, tg, torch.zeros(M, dtype=torch.int64))
    with pytest.raises(ValueError, match='rank must be'):
        call(L.F32, A, W, b, M, V, D, tg, None, rank=torch.zeros(M, dtype=torch.int64))
    with pytest.raises(ValueError, match='pred must be'):
        call(L.F32, A, W, b, M, V, D, tg, None, pred=torch.zeros(M - 1, dtype=torch.int64))
    with pytest.raises(ValueError, match='nll must be'):
        call(L.F32, A, W, b, M, V, D, tg, None, nll=torch.zeros(M, dtype=torch.float64))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        call(L.F32, A, W, b, M, V, D, tg, None, rank=torch.zeros(M, dtype=torch.int32))


def test_evaluate_refusals(no_launch):
    import phenaki_pytorch_amd as P
    from oracle.configs import TINY
    cv = P.CViViT(use_vgg_and_gan=False, **TINY['cvivit'])
    ph = P.Phenaki(maskgit=P.MaskGit(**TINY['maskgit']), cvivit=cv, text_embed_dim=TINY['maskgit']['dim_context']).train()
    ph.maskgit.transformer.eval()
    before = [m.training for m in ph.modules()]
    ids, ctx = torch.zeros(1, 3, 4, 4, dtype=torch.int64), torch.ones(1, 6, TINY['maskgit']['dim_context'])
    with pytest.raises(AssertionError, match='either raw video or video codebook ids'):
        ph.evaluate(text_embeds=ctx)
    with pytest.raises(AssertionError, match='either raw text'):
        ph.evaluate(video_codebook_ids=ids)
    for bad in (0., -0.5, 1.5):
        with pytest.raises(ValueError, match='mask_prob'):
            ph.evaluate(video_codebook_ids=ids, text_embeds=ctx, mask_prob=bad)
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ph.evaluate(video_codebook_ids=ids, text_embeds=ctx)
    assert [m.training for m in ph.modules()] == before, 'a refused call still leaves every train / eval flag as found'
    with pytest.raises(RuntimeError, match='before any update'):
        P.MaskGitMetrics(ph).compute()


def test_new_symbols_in_the_header_and_the_table():
    from phenaki_pytorch_amd import build, _lib
    header = open(os.path.join(ROOT, 'include', 'phenaki_hip.h')).read()
    for name, nargs in (('pk_vocab_eval_words', 1), ('pk_vocab_eval', 13), ('pk_vocab_eval_reduce', 9)):
        assert f'int {name}(' in header and len(_lib.SIGNATURES[name]) == nargs
        decl = header[header.index(f'int {name}('):]
        assert decl[:decl.index(')')].count(',') + 1 == nargs, f'{name}: the header and the signature table disagree'
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.pk_vocab_eval_words(65536) == 1 + 5 * 512 and lib.pk_vocab_eval_words(1000) == 1 + 5 * 8 and lib.pk_vocab_eval_words(128) == 6
    p = 4096                                                              # a non-null, aligned stand-in: every call below returns before using it
    assert lib.pk_vocab_eval(0, None, 32, p, 32, p, 4, 8, 32, p, None, p, None) == -1
    assert lib.pk_vocab_eval(0, p, 32, p, 32, p, 4, 8, 32, None, None, p, None) == -1        # no targets
    assert lib.pk_vocab_eval(0, p, 32, p, 32, p, 4, 8, 32, p, None, None, None) == -1        # no workspace
    assert lib.pk_vocab_eval(3, p, 32, p, 32, p, 4, 8, 32, p, None, p, None) == -1           # unknown dtype
    assert lib.pk_vocab_eval(0, p, 32, p, 32, p, 0, 8, 32, p, None, p, None) == -1
    assert lib.pk_vocab_eval(0, p, 32, p, 32, p, 4, 6, 32, p, None, p, None) != 0            # V % 4
    assert lib.pk_vocab_eval(0, p, 32, p, 16, p, 4, 8, 24, p, None, p, None) != 0            # W not padded to the k-tile
    assert lib.pk_vocab_eval_reduce(None, 4, 8, p, p, p, p, p, None) == -1
    assert lib.pk_vocab_eval_reduce(p, 0, 8, p, p, p, p, p, None) == -1


# ---- the accumulator, fed recorded evaluate dicts -------------------------------------------------------------------------------------------------

def _recorded(rank, batch, critic=True):
    """what Phenaki.evaluate returned for one batch, as a recording (CPU tensors of the documented dtypes)"""
    g = R.g(60 + 10 * rank + batch)
    M, b, n = 20 + 7 * rank + batch, 2, 24
    r = dict(nll=torch.rand(M, generator=g) * 8, entropy=torch.rand(M, generator=g) * 5, lse=torch.rand(M, generator=g),
             rank=torch.randint(0, 30, (M,), generator=g).int(), pred=torch.randint(0, 256, (M,), generator=g),
             rows=torch.arange(M, dtype=torch.int32), mask=torch.zeros(b, n, dtype=torch.bool))
    if critic:
        r.update(critic_logits=torch.randn(b, n, generator=g), critic_labels=torch.rand(b, n, generator=g) < 0.3)
    return r


class _Replay:
    """stands in for a Phenaki: evaluate() plays the recordings back"""

    def __init__(self, records):
        self.records = list(records)

    def evaluate(self, **kw):
        return self.records.pop(0)


def _want(records, critic=True):
    stats = [dict(nll=r['nll'], entropy=r['entropy'], rank=r['rank'].long()) for r in records]
    return R.pooled(stats, [(r['critic_logits'], r['critic_labels']) for r in records] if critic else None)


def _agree(got, want):
    return set(got) == set(want) and all(abs(got[k] - want[k]) <= 1e-12 * max(1., abs(want[k])) for k in want)


@pytest.mark.parametrize('critic', [True, False])
def test_accumulation_over_batches(critic):
    from phenaki_pytorch_amd import MaskGitMetrics
    records = [_recorded(0, i, critic) for i in range(3)]
    mm = MaskGitMetrics(_Replay(records))
    with pytest.raises(RuntimeError, match='before any update'):
        mm.compute()
    for _ in records:
        assert mm.update(video_codebook_ids=None) is mm
    st = mm.state
    assert all(st[k].dtype == torch.float64 for k in ('nll', 'entropy', 'rrank')) and all(v.ndim == 0 for v in st.values())
    assert all(st[k].dtype == torch.int64 for k in ('tokens', 'top1', 'top5', 'top10', 'rank'))
    if critic:
        assert st['critic_bce'].dtype == torch.float64 and all(st[k].dtype == torch.int64 for k in ('critic_correct', 'critic_labels', 'critic_positions'))
    got = mm.compute()
    assert _agree(got, _want(records, critic)) and isinstance(got['tokens'], int) and all(isinstance(v, float) for k, v in got.items() if k != 'tokens')
    assert ('critic_bce' in got) == critic
    assert _agree(mm.compute(merge=False), got), 'compute() leaves the state as it was'
    mm.reset()
    with pytest.raises(RuntimeError, match='before any update'):
        mm.compute()


def _merge_worker(rank, ws, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=ws)
    sys.path.insert(0, ROOT)
    from unittest import mock
    from phenaki_pytorch_amd import MaskGitMetrics
    mine = [_recorded(rank, i) for i in range(2)]
    mm = MaskGitMetrics(_Replay(mine))
    for _ in mine:
        mm.update()
    everyone = [_recorded(r, i) for r in range(ws) for i in range(2)]
    ok = _agree(mm.compute(), _want(everyone))                          # the collective: both ranks call it, both get the pooled numbers
    ok = ok and _agree(mm.compute(merge=False), _want(mine))            # ... and the rank-local form sends nothing
    sent = []
    with mock.patch.object(dist, 'all_reduce', lambda t, **kw: sent.append(tuple(t.shape))):
        mm.compute(merge=False)
        ok = ok and sent == []
        mm.compute()
        ok = ok and len(sent) == len(mm.state) == 12
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


def test_compute_world_size_2_gloo():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000) + 23
    procs = [ctx.Process(target=_merge_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(res) == [(0, True), (1, True)]


def test_example_validates_on_rank_0_without_a_collective():
    src = open(os.path.join(ROOT, 'examples', 'train_maskgit.py')).read()
    assert 'mm.compute(merge=False)' in src and 'mm.compute()' not in src and '--eval-every' in src and '--eval-batches' in src
