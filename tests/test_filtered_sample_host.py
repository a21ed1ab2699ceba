"""Top-k filtered sampling on the host: the restatement (tests/filtered_sample_restatement.py) against the reference's own top_k + gumbel_sample where
the reference is present, k_of against the reference's expression, every ValueError of Phenaki.sample(filter_thres=, top_k=) with nothing launched, the
wrapper calls of the filtered loop (recorder stubs, tests/test_sample_calls_host.recording), the slab split of _lib.vocab_sample_filtered, and the
margins the GPU end-to-end test relies on, from the oracle alone.  Nothing here launches a kernel."""
import contextlib
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import pytest  # noqa: E402
import torch  # noqa: E402

from oracle import phenaki_oracle as O  # noqa: E402
from oracle import weights  # noqa: E402
from oracle.configs import TINY, oracle_cfgs, state_dicts  # noqa: E402
from phenaki_pytorch_amd import _lib as L  # noqa: E402
from tests import filtered_sample_restatement as R  # noqa: E402
from tests import test_sample_calls_host as SC  # noqa: E402

torch.set_grad_enabled(False)
V, B, N, STEPS = SC.MASK_ID, SC.B, SC.N, SC.STEPS
NEW = ('vocab_sample_filtered', 'logits_topk_sample')


@contextlib.contextmanager
def recording(rec):
    """tests/test_sample_calls_host.recording with the two new wrappers recorded too"""
    saved = [(k, getattr(L, k)) for k in NEW]
    try:
        with SC.recording(rec):
            for k in NEW:
                setattr(L, k, rec.stub(k))
            yield
    finally:
        for k, v in saved:
            setattr(L, k, v)


def run(ph, **kw):
    rec = SC.Recorder()
    with recording(rec):
        out = ph.sample(**kw)
    return rec, out


# ------------------------------------------------------------------------------------------------ the restatement against the reference

@pytest.mark.parametrize('thres', [0., 0.5, 0.9, 0.999])
@pytest.mark.parametrize('Vv', [8, 256, 1000])
def test_restatement_equals_the_reference_helpers(Vv, thres):
    from oracle import ref_shim
    if not ref_shim.available():
        pytest.skip('the reference is not on this machine')
    m = ref_shim.load().module
    g = torch.Generator().manual_seed(1000 * Vv + int(1000 * thres))
    M, T = 16, 0.45
    l = torch.randn(M, Vv, generator=g, dtype=torch.float64) * 3               # continuous draws: tie-free
    assert all(l[r].unique().numel() == Vv for r in range(M))
    u = torch.rand(M, Vv, generator=g)
    k = R.k_of(thres, Vv)
    cut, kept = R.select64(l, k)
    filtered = m.top_k(l, thres=thres)
    assert torch.equal(filtered != -math.inf, kept) and (kept.sum(-1) == k).all()
    assert torch.equal(filtered[kept], l[kept])
    saved = m.gumbel_noise
    m.gumbel_noise = lambda t: -m.log(-m.log(u.double()))                      # the reference's expression on the injected draws
    try:
        want = m.gumbel_sample(filtered, temperature=T)
    finally:
        m.gumbel_noise = saved
    ref = R.noisy_ref(l, torch.zeros_like(l), R.PARITY, T, U=u)
    R.accept(ref, k, want, f'reference argmax, V = {Vv}, thres = {thres}')
    mine = torch.where(kept, ref.noisy, torch.full_like(ref.noisy, -math.inf)).argmax(-1)
    one = R.accept_counts(ref, k) == 1
    assert one.float().mean() >= 0.9 and torch.equal(mine[one], want[one])


def test_k_of_is_the_reference_expression():
    grid_V = (4, 8, 100, 256, 1000, 1156, 4100, 65536)
    thres = [0., 0.1, 0.3, 0.5, 0.7, 0.9, 0.99, 0.999, 0.9999, 0.99999]
    for Vv in grid_V:                                                            # (1 - thres) * V within an ulp of an integer j
        for j in (1, 2, 3, Vv // 10, Vv // 2, Vv - 1):
            if j >= 1:
                t = 1 - j / Vv
                thres += [t, float(np.nextafter(t, 0.)), float(np.nextafter(t, 1.))]
    thres = [t for t in thres if 0. <= t < 1.]
    from oracle import ref_shim
    ref_k = None
    if ref_shim.available():
        m = ref_shim.load().module
        ref_k = lambda t, Vv: int((m.top_k(torch.arange(Vv, dtype=torch.float64)[None], thres=t) != -math.inf).sum())
    seen = set()
    for Vv in grid_V:
        for t in thres:
            k = R.k_of(t, Vv)
            assert k == max(int((1 - t) * Vv), 1) and 1 <= k <= Vv
            seen.add(k == round((1 - t) * Vv))
            if ref_k is not None and (Vv <= 1156 or t in (0., 0.5, 0.9)):
                assert ref_k(t, Vv) == k, (t, Vv)
    assert seen == {True, False}                                                 # some of the near-integer products truncate below the integer
    assert R.k_of(0.9, 256) == 25 and R.k_of(0.9, 65536) == 6553 and R.k_of(0., 256) == 256 and R.k_of(0.9999, 256) == 1


def test_accept_rejects_what_it_should():
    l = torch.tensor([[0., 3., 1., 2., -1., 2.5, 0.5, 2.0]], dtype=torch.float64)
    ref = R.noisy_ref(l, torch.zeros_like(l), R.NONE, 1.0)
    cut, kept = R.select64(l, 3)
    assert cut.item() == 2.0 and kept.sum().item() == 4                          # the tie at the cut keeps both columns
    assert R.accept(ref, 3, torch.tensor([1])) == 0
    for wrong, msg in ((5, 'reaches'), (2, 'filter drops'), (9, 'outside')):
        with pytest.raises(AssertionError, match=msg):
            R.accept(ref, 3, torch.tensor([wrong]))
    tie = torch.tensor([[1., 5., 5., 0.]], dtype=torch.float64)
    rt = R.noisy_ref(tie, torch.zeros_like(tie), R.NONE, 1.0)
    assert R.accept(rt, 2, torch.tensor([1])) == 1                               # two columns in the accept set; the tie rule decides between them
    with pytest.raises(AssertionError, match='later one'):
        R.accept(rt, 2, torch.tensor([2]))
    # a bound that straddles the cut: the column just under it becomes possible, neither of the two is sure
    near = torch.tensor([[4., 3.0, 2.9999, 0.]], dtype=torch.float64)
    rn = R.noisy_ref(near, torch.full_like(near, 1e-3), R.NONE, 1.0)
    poss, sure = R.bands(rn, 2)
    assert poss.tolist() == [[True, True, True, False]] and sure.tolist() == [[True, False, False, False]]
    assert R.accept(rn, 1, torch.tensor([0])) == 0 and R.accept(rn, 2, torch.tensor([0])) == 0
    with pytest.raises(AssertionError, match='reaches'):
        R.accept(rn, 2, torch.tensor([2]))
    exact = R.noisy_ref(near, torch.zeros_like(near), R.NONE, 1.0)
    assert R.bands(exact, 2)[0].tolist() == R.bands(exact, 2)[1].tolist() == [[True, True, False, False]]
    zeros = torch.tensor([[1., 0., -0., -1.]], dtype=torch.float64)
    assert R.select64(zeros, 2)[1].tolist() == [[True, True, True, False]]
    sc, bound = R.score_ref(ref, torch.tensor([1]))
    assert abs(sc.item() - (1 - math.exp(3.) / l.exp().sum().item())) < 1e-12 and 0 < bound.item() < 1e-5


# ------------------------------------------------------------------------------------------------ Phenaki.sample: refusals and wrapper calls

@pytest.mark.parametrize('kw,msg', [
    (dict(filter_thres=0.9, top_k=3), 'not both'),
    (dict(filter_thres=1.0), 'filter_thres'), (dict(filter_thres=-0.1), 'filter_thres'), (dict(filter_thres=float('nan')), 'filter_thres'),
    (dict(filter_thres=float('inf')), 'filter_thres'), (dict(filter_thres='0.9'), 'filter_thres'), (dict(filter_thres=True), 'filter_thres'),
    (dict(top_k=0), 'top_k'), (dict(top_k=V + 1), 'top_k'), (dict(top_k=3.0), 'top_k'), (dict(top_k=True), 'top_k'), (dict(top_k=-1), 'top_k'),
    (dict(top_k=3, _noise_fn='torch'), 'torch'), (dict(filter_thres=0.5, _noise_fn='torch'), 'torch')])
def test_bad_filter_arguments_are_refused_before_anything_launches(kw, msg):
    ph = SC.make('token')
    rec = SC.Recorder()
    with recording(rec), pytest.raises(ValueError, match=msg):
        ph.sample(num_frames=5, batch_size=B, **kw)
    assert rec.calls == []


def _shape_of(a):
    if torch.is_tensor(a):
        return ('tensor', tuple(a.shape), a.dtype)
    if isinstance(a, (list, tuple)):
        return tuple(_shape_of(x) for x in a)
    return a


def _normalised(rec):
    return [(name, _shape_of(args), {k: _shape_of(v) for k, v in kw.items()}) for name, args, kw in rec.calls]


@pytest.mark.parametrize('critic', [None, 'token'])
def test_a_filter_that_keeps_everything_is_the_plain_path(critic):
    ph = SC.make(critic)
    plain, _ = run(ph, num_frames=5, batch_size=B, _seed=7)
    key = ph._pk_last_sample_key
    assert key[-1] is None and len(key) == 16
    for kw in (dict(filter_thres=None), dict(top_k=V), dict(filter_thres=0.), dict(filter_thres=0)):
        rec, _ = run(ph, num_frames=5, batch_size=B, _seed=7, **kw)
        assert _normalised(rec) == _normalised(plain), kw
        assert not any(n in rec.names() for n in NEW)
        assert ph._pk_last_sample_key == key


@pytest.mark.parametrize('critic', [None, 'token'])
@pytest.mark.parametrize('compact', [True, False])
def test_with_a_filter_every_step_is_one_filtered_head(critic, compact):
    ph = SC.make(critic)
    rec, out = run(ph, num_frames=5, batch_size=B, _seed=7, top_k=3, _compact=compact)
    head = ['embeds', 'cfg_mix', 'vocab_sample_filtered']
    assert rec.names() == SC.loop_names(head + (SC.CRITIC if critic else []), head)
    assert out.shape == (B, 3, 5, 64, 64)
    heads = SC.calls(rec, 'vocab_sample_filtered')
    need_lse = critic is None
    slab = heads[0][1][17]
    assert slab.shape == (B * N, V) and slab.dtype == torch.float32                                    # 128 MB holds far more than B n rows of V = 256
    for s, c in enumerate(heads):
        a = c[1]
        assert a[4:8] == (B * SC.KS[s] if (compact and s > 0) else B * N, V, TINY['maskgit']['dim'], 3)  # M, V, D, k
        assert a[8] == float(0.9 * ((STEPS - s - 1) / STEPS)) and a[9] is None                          # temperature; no injected noise
        assert (a[10] is not None) == (compact and s > 0)                                               # the compact row list
        assert a[11] == (7 + s * 0x9E3779B97F4A7C15) & SC.M64 and a[12] is need_lse
        assert a[13].shape == (B, N) and a[14].shape == (B, N) and a[15].shape == (B, N) and (a[16] is not None) == need_lse
        assert a[17] is slab and c[2] == dict(seed_dev=None)
    if need_lse:                                                                                        # the scores ping-pong as on the plain path
        for s, c in enumerate(SC.calls(rec, 'topk_mask'), start=1):
            assert c[1][0] is heads[s - 1][1][16] and c[2]['scores_next'] is heads[s][1][16]


def test_the_key_names_the_resolved_k():
    ph = SC.make('token')
    keys = {}
    for name, kw in (('k3', dict(top_k=3)), ('k25', dict(top_k=25)), ('t0.9', dict(filter_thres=0.9)), ('plain', {})):
        run(ph, num_frames=5, batch_size=B, **kw)
        keys[name] = ph._pk_last_sample_key
    assert keys['k3'] != keys['k25'] and keys['k25'] == keys['t0.9'] and keys['plain'] != keys['k25']
    assert (keys['k3'][-1], keys['k25'][-1], keys['plain'][-1]) == (3, 25, None)
    assert keys['k3'][:-1] == keys['plain'][:-1]


def test_infill_make_video_and_sample_images_forward_the_filter():
    from tests import test_infill_host as TI
    ph = SC.make('token')
    ids0, known = TI._known()
    rec, _ = run(ph, num_frames=5, batch_size=B, known_ids=ids0, known_mask=known, top_k=5)
    assert 'vocab_sample' not in rec.names() and len(SC.calls(rec, 'vocab_sample_filtered')) == STEPS
    _, _, totals = SC.PH.infill_schedule([32, 36], STEPS)
    assert [c[1][4] for c in SC.calls(rec, 'vocab_sample_filtered')] == totals and all(c[1][7] == 5 for c in SC.calls(rec, 'vocab_sample_filtered'))
    rec = SC.Recorder()
    with recording(rec):
        ph.sample_images(batch_size=B, filter_thres=0.9)
        SC.PH.make_video(ph, texts=['a', 'b'], num_frames=(5, 4), prime_lengths=1, filter_thres=0.9)
    heads = SC.calls(rec, 'vocab_sample_filtered')
    assert len(heads) == 3 * STEPS and all(c[1][7] == 25 for c in heads) and 'vocab_sample' not in rec.names()


# ------------------------------------------------------------------------------------------------ the slab split

@pytest.mark.parametrize('with_rows', [False, True])
def test_vocab_sample_filtered_walks_the_rows_slab_by_slab(with_rows):
    rec = SC.Recorder()
    saved = [(k, getattr(L, k)) for k in ('gemm', 'logits_topk_sample')]
    M, Vv, D = 130, 1156, 40
    A, W, bias = torch.zeros(M + 5, D + 8)[:, :D], torch.zeros(Vv, 64), torch.zeros(Vv)
    rows = torch.arange(M, dtype=torch.int32) * 2 if with_rows else None
    pred = torch.zeros(2 * M, dtype=torch.int64)
    try:
        for k, _ in saved:
            setattr(L, k, rec.stub(k))
        L.vocab_sample_filtered(L.F32, A, W, bias, M, Vv, D, 7, 0.5, None, rows, 11, True, None, None, pred, None, torch.zeros(64, Vv), seed_dev=None)
        n_split = len(rec.calls)
        L.vocab_sample_filtered(L.F32, A, W, bias, 50, Vv, D, 7, 0.5, None, rows, 11, True, None, None, pred, None, torch.zeros(64, Vv))
        L.vocab_sample_filtered(L.F32, A, W, bias, 64, Vv, D, 7, 0.5, None, rows, 11, True, None, None, pred, None, torch.zeros(64, Vv))
    finally:
        for k, v in saved:
            setattr(L, k, v)
    assert rec.names() == ['gemm', 'logits_topk_sample'] * 5 and n_split == 6
    gemms, sels = SC.calls(rec, 'gemm'), SC.calls(rec, 'logits_topk_sample')
    for i, (m0, Rc) in enumerate(((0, 64), (64, 64), (128, 2), (0, 50), (0, 64))):
        g, s = gemms[i], sels[i]
        assert g[1][0] == L.F32 and g[1][3:] == (Rc, Vv, D) and g[1][2] is W and g[2]['bias'] is bias
        assert g[1][1].shape == (Rc, D) and g[1][1].data_ptr() == A[m0:].data_ptr() and g[1][1].stride(0) == A.stride(0)
        assert g[2]['C'].shape == (Rc, Vv) and g[2]['C'].data_ptr() == s[1][0].data_ptr()               # the slab's first Rc rows, then sampled
        assert s[1][1:5] == (Rc, Vv, 7, 0.5) and s[1][8:10] == (11, True)
        if with_rows:
            assert torch.equal(s[1][6], rows[m0:m0 + Rc]) and s[1][6].data_ptr() == rows[m0:].data_ptr() and s[1][7] == 0
        else:
            assert s[1][6] is None and s[1][7] == m0


def test_slab_rows(monkeypatch):
    monkeypatch.delenv('PK_FILTER_SLAB_MB', raising=False)
    assert L.FILTER_SLAB_MB in (64, 128, 256)
    mb = L.FILTER_SLAB_MB
    assert L.filter_slab_rows(4608, 65536) == min(4608, mb * 4) and L.filter_slab_rows(96, 256) == 96 and L.filter_slab_rows(0, 256) == 1
    monkeypatch.setenv('PK_FILTER_SLAB_MB', '64')
    assert L.filter_slab_rows(4608, 65536) == 256
    monkeypatch.setenv('PK_FILTER_SLAB_MB', '0')
    assert L.filter_slab_rows(4608, 65536) == 1


# ------------------------------------------------------------------------------------------------ the margins of the GPU end-to-end test

@pytest.mark.parametrize('with_critic', [True, False])
@pytest.mark.parametrize('base', R.E2E_SEEDS)
def test_the_end_to_end_accept_sets_are_single_columns_nearly_everywhere(base, with_critic):
    """on the oracle's own filtered trajectory, TINY, k = 25: the share of (step, masked position) pairs whose accept set is not a single column"""
    cv_sd, mg_sd, cr_sd = state_dicts('tiny')
    _, mgc, crc = oracle_cfgs(TINY)
    ctx = weights.synthetic_context(2, 6, TINY['maskgit']['dim_context'], seed=2)
    nf = lambda kind, step, shape: weights.uniform_noise(tuple(shape), base + 2 * step + (1 if kind == 'critic' else 0))
    k = R.k_of(0.9, TINY['maskgit']['num_tokens'])
    assert k == 25
    steps = R.oracle_filtered_sample(O, mg_sd, mgc, cr_sd if with_critic else None, crc, batch=2, n=48, patch_shape=(3, 4, 4), context=ctx,
                                     steps=TINY['steps'], k=k, noise_fn=nf)
    amb = tot = 0
    for rec in steps:
        rows = rec['mask'].reshape(-1)
        amb += R.accept(rec['ref'], k, rec['pred'].reshape(-1), rows=rows)
        tot += int(rows.sum())
        _, kept = R.select64(rec['ref'].l64, k)
        assert kept.gather(-1, rec['pred'].reshape(-1, 1)).all()
    assert tot >= 2 * 48 + TINY['steps'] - 1
    assert amb <= R.E2E_AMBIGUOUS_CAP * tot, f'{amb} of {tot} pairs are not decided by the oracle alone'
