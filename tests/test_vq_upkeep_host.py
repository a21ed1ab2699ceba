"""CPU-only checks of the VectorQuantize upkeep surface (k-means initialisation, dead-code expiry, cross-rank statistics): keywords and
attributes, the state_dict contract, the row choice, the `_lib` calls a training-mode call issues, and the invariants of the restatement the
GPU tests compare against (tests/vq_upkeep_restatement.py).  No kernel is launched."""
import contextlib

import pytest
import torch
import torch.nn.functional as F

from tests import vq_upkeep_restatement as R

torch.set_grad_enabled(False)


def _vq(**kw):
    from phenaki_pytorch_amd.quantize import VectorQuantize
    return VectorQuantize(dim=64, codebook_size=32, **kw)


def test_keyword_defaults_and_attributes():
    vq = _vq()
    assert (vq.kmeans_init, vq.kmeans_iters, vq.threshold_ema_dead_code, vq.reset_cluster_size, vq.sync_codebook, vq.upkeep_seed) == \
        (False, 10, 0, None, None, 0)
    assert vq.last_upkeep is None
    vq = _vq(kmeans_init=True, kmeans_iters=3, threshold_ema_dead_code=2, reset_cluster_size=1.5, sync_codebook=False, upkeep_seed=7,
             some_other_published_keyword=1)                                         # unknown keywords keep being swallowed
    assert (vq.kmeans_init, vq.kmeans_iters, vq.threshold_ema_dead_code, vq.reset_cluster_size, vq.sync_codebook, vq.upkeep_seed) == \
        (True, 3, 2, 1.5, False, 7)
    vq = _vq()
    vq.threshold_ema_dead_code = 2                                                   # settable after construction (the reference passes no keyword)
    assert vq.begin_upkeep()['expire_b'] == R.mix(0, 0, R.EXPIRE)
    assert vq.begin_upkeep() == dict(call=1, kmeans_b=None, expire_b=R.mix(0, 1, R.EXPIRE)) == vq.last_upkeep


@pytest.mark.parametrize('kmeans_init', [False, True])
def test_state_dict_and_initted(kmeans_init):
    vq = _vq(kmeans_init=kmeans_init, threshold_ema_dead_code=2)
    sd = vq.state_dict()
    assert sorted(sd) == ['_codebook.cluster_size', '_codebook.embed', '_codebook.embed_avg', '_codebook.initted']
    assert bool(sd['_codebook.initted']) == (not kmeans_init)
    assert vq.needs_kmeans() == kmeans_init
    if kmeans_init:
        assert not sd['_codebook.embed'].any()                                      # zeros until the first training-mode call, as published
        done = _vq().state_dict()
        vq.load_state_dict(done)                                                    # a checkpoint with initted = True never re-initialises
        assert not vq.needs_kmeans()
    else:
        assert torch.allclose(sd['_codebook.embed'][0].norm(dim=-1), torch.ones(32), atol=1e-6)


def test_sync_codebook_without_a_process_group():
    assert _vq().sync_world() == 1 and _vq(sync_codebook=False).sync_world() == 1
    vq = _vq(sync_codebook=True).train()
    with pytest.raises(ValueError, match='process group'):
        vq.sync_world()
    with pytest.raises(ValueError, match='process group'):
        vq(torch.randn(1, 4, 64))


@pytest.mark.parametrize('n', [1, 2, 101, 4608])
def test_pick_is_a_bijection_and_wraps_evenly(n):
    from phenaki_pytorch_amd.quantize import pick
    for b in (0, 5, R.mix(0, 3, R.EXPIRE), 2 ** 62 - 1):
        first = [pick(b, j, n) for j in range(n)]
        assert sorted(first) == list(range(n))
        beyond = [pick(b, j, n) for j in range(3 * n + n // 2)]
        counts = torch.bincount(torch.tensor(beyond), minlength=n)
        assert int(counts.max()) - int(counts.min()) <= 1 and int(counts.min()) == 3
        assert beyond == [R.pick(b, j, n) for j in range(len(beyond))]


def test_mix_agrees_with_the_restatement():
    from phenaki_pytorch_amd import quantize as Q
    assert (Q.PICK_P, Q.UPKEEP_EXPIRE, Q.UPKEEP_KMEANS) == (R.P, R.EXPIRE, R.KMEANS)
    seen = set()
    for seed in (0, 1, 2 ** 63 + 11):
        for call in (0, 1, 1000):
            for purpose in (R.EXPIRE, R.KMEANS):
                b = Q.upkeep_mix(seed, call, purpose)
                assert b == R.mix(seed, call, purpose) and 0 <= b < 2 ** 62
                seen.add(b)
    assert len(seen) == 18


STUBBED = ('l2norm_rows', 'vocab_sample', 'vocab_reduce', 'vq_gather_commit', 'vq_ema_update', 'vq_ema_update_expire', 'vq_kmeans',
           'vq_compact_keep', 'colsum')


@contextlib.contextmanager
def recording(calls):
    from phenaki_pytorch_amd import _lib as L
    saved = {k: getattr(L, k) for k in STUBBED + ('require_device', 'vocab_ntiles')}

    def stub(name):
        def call(*args, **kwargs):
            calls.append((name, args, kwargs))
            return args[3] if name == 'colsum' else None
        return call
    try:
        for k in STUBBED:
            setattr(L, k, stub(k))
        L.require_device = lambda t, name='tensor': None
        L.vocab_ntiles = lambda V: 1
        yield
    finally:
        for k, v in saved.items():
            setattr(L, k, v)


def test_disabled_upkeep_issues_exactly_todays_lib_calls():
    """threshold = 0, kmeans_init = False, one process: l2norm, lookup (two launches), gather + commitment, the EMA chain, the loss reduction --
    with the arguments of before; with a threshold the EMA chain alone is replaced by its expiring form"""
    vq = _vq().train()
    cb = vq._codebook
    calls = []
    with recording(calls):
        vq(torch.randn(1, 4, 64))
    assert [c[0] for c in calls] == ['l2norm_rows', 'vocab_sample', 'vocab_reduce', 'vq_gather_commit', 'vq_ema_update', 'colsum']
    _, args, kwargs = calls[4]
    assert kwargs == {} and len(args) == 8 and args[2] is None and args[6:] == (0.8, 1e-5)
    assert args[0] is calls[0][1][1]                                                # xn: what l2norm_rows wrote
    for got, buf in zip(args[3:6], (cb.cluster_size, cb.embed_avg, cb.embed)):
        assert got.data_ptr() == buf.data_ptr() and got.shape == buf.shape[1:]
    assert vq.last_upkeep == dict(call=0, kmeans_b=None, expire_b=None)
    vq.threshold_ema_dead_code, vq.reset_cluster_size = 2, 0.5
    calls = []
    with recording(calls):
        vq(torch.randn(1, 4, 64))
    assert [c[0] for c in calls] == ['l2norm_rows', 'vocab_sample', 'vocab_reduce', 'vq_gather_commit', 'vq_ema_update_expire', 'colsum']
    assert calls[4][1][6:] == (0.8, 1e-5, 2.0, 0.5, R.mix(0, 1, R.EXPIRE))


def _state(g, V, D):
    embed = F.normalize(torch.randn(V, D, generator=g), dim=-1)
    return embed, embed * (1 + torch.rand(V, 1, generator=g)), 2 * torch.rand(V, generator=g)


@pytest.mark.parametrize('masked', [False, True])
@pytest.mark.parametrize('threshold,reset', [(0.5, None), (1.5, 0.25)])
def test_restatement_expiry_invariants(masked, threshold, reset):
    g = torch.Generator().manual_seed(9)
    M, V, D = 40, 64, 32
    x = torch.randn(M, D, generator=g)
    embed, embed_avg, cluster_size = _state(g, V, D)
    ids = (F.normalize(x, dim=-1) @ embed.t()).argmax(-1)
    keep = (torch.rand(M, generator=g) > 0.3) if masked else None
    b = R.mix(3, 0, R.EXPIRE)
    plain = R.vq_upkeep_step(x, embed, embed_avg, cluster_size, keep, ids)
    out = R.vq_upkeep_step(x, embed, embed_avg, cluster_size, keep, ids, threshold=threshold, reset=reset, b=b)
    ex = out['expired']
    value = threshold if reset is None else reset
    n_keep = M if keep is None else int(keep.sum())
    assert torch.equal(ex, plain['cluster_size'] < threshold) and ex.any() and not ex.all()
    assert (int(ex.sum()) > n_keep) == (threshold == 1.5)                            # both regimes: distinct rows, and wrapping beyond n_keep
    assert bool((out['cluster_size'][ex] == value).all())
    assert torch.equal(out['embed_avg'][ex], out['embed'][ex] * torch.tensor(value))
    assert torch.allclose(out['embed'].norm(dim=-1), torch.ones(V), atol=1e-6)
    for k in ('cluster_size', 'embed_avg', 'embed'):
        assert torch.equal(out[k][~ex], plain[k][~ex])
    kept = R.kept_rows(M, keep)
    assert set(out['rows'].tolist()) <= set(kept.tolist())
    first = out['rows'][:n_keep].tolist()
    assert len(set(first)) == len(first)
    assert torch.equal(out['embed'][ex], F.normalize(x, dim=-1)[out['rows']])


def test_restatement_kmeans_invariants():
    g = torch.Generator().manual_seed(4)
    M, V, D = 24, 32, 16                                                             # fewer rows than codes: duplicate seeds, empty codes
    xn = F.normalize(torch.randn(M, D, generator=g), dim=-1)
    keep = torch.rand(M, generator=g) > 0.25
    out = R.kmeans(xn, keep, V, 3, R.mix(0, 0, R.KMEANS))
    n = int(keep.sum())
    assert int(out['bins'].sum()) == n and (out['bins'] == 0).any()
    empty = out['bins'] == 0
    last_but_one = out['means'][-2]
    assert torch.equal(out['embed'][empty], last_but_one[empty])                    # a code with bins == 0 stays on its old mean
    assert torch.allclose(out['embed'].norm(dim=-1), torch.ones(V), atol=1e-6)
    assert torch.equal(out['embed_avg'], out['embed'] * out['cluster_size'][:, None])
    kept_set = {tuple(r.tolist()) for r in xn[keep]}
    assert all(tuple(r.tolist()) in kept_set for r in out['seeds'])                 # masked rows never enter the data
    again = R.kmeans(xn, keep, V, 3, R.mix(0, 0, R.KMEANS), ids=out['ids'])
    assert torch.equal(again['embed'], out['embed'])
