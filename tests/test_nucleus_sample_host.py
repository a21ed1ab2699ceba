"""Nucleus / min-p filtered sampling on the host: the restatement (tests/nucleus_sample_restatement.py) against designed rows, against the common
sort / cumsum / shift formulation of top-p and the per-element definition of min-p, what its band check rejects, every ValueError of
Phenaki.sample(top_p=, min_p=) with nothing launched, the wrapper calls with the filters off and on (recorder stubs,
tests/test_sample_calls_host.recording), the key, the forwarders, the slab walk of _lib.vocab_sample_nucleus, and the margins the GPU end-to-end
test relies on, from the oracle alone.  Nothing here launches a kernel."""
import contextlib
import math
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import pytest  # noqa: E402
import torch  # noqa: E402

from oracle import phenaki_oracle as O  # noqa: E402
from oracle import weights  # noqa: E402
from oracle.configs import TINY, oracle_cfgs, state_dicts  # noqa: E402
from phenaki_pytorch_amd import _lib as L  # noqa: E402
from phenaki_pytorch_amd import dist as D  # noqa: E402
from tests import filtered_sample_restatement as R  # noqa: E402
from tests import nucleus_sample_restatement as NR  # noqa: E402
from tests import test_filtered_sample_host as FH  # noqa: E402
from tests import test_sample_calls_host as SC  # noqa: E402

torch.set_grad_enabled(False)
V, B, N, STEPS = SC.MASK_ID, SC.B, SC.N, SC.STEPS
NEW = ('vocab_sample_nucleus', 'logits_nucleus_sample')


@contextlib.contextmanager
def recording(rec):
    """tests/test_filtered_sample_host.recording with the two nucleus wrappers recorded too"""
    saved = [(k, getattr(L, k)) for k in NEW]
    try:
        with FH.recording(rec):
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


# ------------------------------------------------------------------------------------------------ the restatement

@pytest.mark.parametrize('T', [1.0, 0.225])
@pytest.mark.parametrize('Vv', [8, 1000])
def test_designed_rows_keep_the_designed_counts(Vv, T):
    masses, cases = NR.DESIGNED
    row = NR.designed_row(masses, Vv, T)[None]
    for p, want in cases:
        cut, n = NR.nucleus64(row, T, Vv, p, 0.)
        assert n.item() == want and cut.item() == row[0, want - 1].item(), (p, want)
    tie, p, want = NR.DESIGNED_TIE
    cut, n = NR.nucleus64(NR.designed_row(tie, Vv, T)[None], T, Vv, p, 0.)
    assert n.item() == want                                                     # the cut falls inside the run of ties: all of it is kept
    const = torch.full((1, Vv), 1.5, dtype=torch.float64)
    for p, mp in ((1e-6, 0.), (0.5, 0.), (1., 0.5), (0.999, 0.05)):
        assert NR.nucleus64(const, T, Vv, p, mp)[1].item() == Vv                # a constant row keeps all V, whatever the filter
    assert NR.nucleus64(row, T, Vv, 1., 0.)[0].item() == -math.inf and NR.nucleus64(row, T, Vv, 1., 0.)[1].item() == Vv
    # at temperature 0 (the clamp) the nucleus is the maximum and its exact ties
    l = torch.tensor([[1., 3., 3., 2.9999999, -5., 3.]], dtype=torch.float64)
    assert NR.nucleus64(l, 0., 6, 0.999, 0.)[1].item() == 3 and NR.nucleus64(l, 0., 6, 1., 0.5)[1].item() == 3
    # the filters intersect: top-k 2 of (0.5, 0.3, 0.15, 0.05), then the nucleus on the top-k set's OWN mass 0.8: 0.5 / 0.8 < 0.7 keeps both
    assert NR.nucleus64(row, T, 2, 0.7, 0.)[1].item() == 2 and NR.nucleus64(row, T, 2, 0.6, 0.)[1].item() == 1
    assert NR.nucleus64(row, T, Vv, 0.97, 0.2)[1].item() == 3                   # min-p 0.2 of the largest 0.5: 0.15 passes, 0.05 does not


@pytest.mark.parametrize('T', [1.0, 0.225])
@pytest.mark.parametrize('p', [0.1, 0.5, 0.9, 0.999])
def test_restatement_equals_the_common_formulation_on_tie_free_rows(p, T):
    """sort descending, softmax, cumulative sum, drop where the cumulative sum BEFORE the column already reaches p (the shift): what sampling libraries
    write; and min-p by its per-element definition p[v] >= min_p max p"""
    g = torch.Generator().manual_seed(int(1000 * p) + int(100 * T))
    for Vv in (8, 256, 1156):
        l = torch.randn(16, Vv, generator=g, dtype=torch.float64) * 3
        assert all(l[r].unique().numel() == Vv for r in range(16))
        ls, order = l.sort(-1, descending=True)
        pr = (ls / NR.f32(T)).softmax(-1)
        cs = pr.cumsum(-1)
        drop = torch.zeros_like(cs, dtype=torch.bool)
        drop[:, 1:] = cs[:, :-1] >= NR.f32(p)
        want = (~drop).sum(-1)
        cut, n = NR.nucleus64(l, T, Vv, p, 0.)
        margin = (cs - NR.f32(p)).abs().min(-1).values > 1e-12                   # a cumulative sum that hits p to the last bit decides nothing
        assert margin.all() and torch.equal(n, want) and torch.equal(cut, ls.gather(-1, want[:, None] - 1)[:, 0])
        for mp in (0.05, 0.5):
            prob = (l / NR.f32(T)).softmax(-1)
            keep = prob >= NR.f32(mp) * prob.max(-1, keepdim=True).values
            assert ((prob / prob.max(-1, keepdim=True).values - NR.f32(mp)).abs() > 1e-12).all()
            cut, n = NR.nucleus64(l, T, Vv, 1., mp)
            assert torch.equal(n, keep.sum(-1)) and torch.equal(cut, torch.where(keep, l, torch.full_like(l, math.inf)).min(-1).values)
            both = NR.nucleus64(l, T, Vv, p, mp)[1]
            assert torch.equal(both, torch.minimum(want, keep.sum(-1)))          # upward-closed sets: the intersection is the smaller one


def test_the_band_check_rejects_what_it_should():
    g = torch.Generator().manual_seed(5)
    l = torch.randn(4, 256, generator=g).double()
    f = lambda x: x.float()
    i = lambda x: x.to(torch.int32)
    for k, p, mp in ((256, 0.5, 0.), (256, 1., 0.05), (25, 0.9, 0.), (25, 1., 0.), (256, 0.9, 0.05), (8, 0.9, 0.3)):
        cut, n = NR.nucleus64(l, 1.0, k, p, mp)
        ls = l.sort(-1, descending=True).values
        assert (n > 1).all() and (n < 256).all()
        NR.check_nucleus(l, 0., 1.0, k, p, mp, f(cut), i(n))
        higher, lower = ls.gather(-1, n[:, None] - 2)[:, 0], ls.gather(-1, n[:, None])[:, 0]     # one column fewer, one column more
        with pytest.raises(AssertionError, match='too high'):
            NR.check_nucleus(l, 0., 1.0, k, p, mp, f(higher), i(n - 1))
        with pytest.raises(AssertionError, match='too low'):
            NR.check_nucleus(l, 0., 1.0, k, p, mp, f(lower), i(n + 1))
        with pytest.raises(AssertionError, match='kept count'):
            NR.check_nucleus(l, 0., 1.0, k, p, mp, f(cut), i(n + 1))
        with pytest.raises(AssertionError, match='no row value'):
            NR.check_nucleus(l, 0., 1.0, k, p, mp, f(cut) + 1e-3, i(n))
    with pytest.raises(AssertionError, match='no filter is active'):
        NR.check_nucleus(l, 0., 1.0, 256, 1., 0., f(l.min(-1).values), i(torch.full((4,), 256)))
    NR.check_nucleus(l, 0., 1.0, 256, 1., 0., torch.full((4,), -math.inf), i(torch.full((4,), 256)))
    # a logit bound widens the band by what it must: the neighbouring cut passes once E covers the gap to it, and not before
    cut, n = NR.nucleus64(l, 1.0, 256, 0.5, 0.)
    lower = l.sort(-1, descending=True).values.gather(-1, n[:, None])[:, 0]
    gap = float((cut - lower).max())
    NR.check_nucleus(l, 1.01 * gap, 1.0, 256, 0.5, 0., f(lower), i(n + 1))
    # the draw: a nucleus draw is a top-k' draw at k' = the kept count
    ref = R.noisy_ref(l, torch.zeros_like(l), R.NONE, 1.0)
    assert NR.accept_draw(ref, n, l.argmax(-1)) == 0
    with pytest.raises(AssertionError, match='filter drops'):
        NR.accept_draw(ref, n, l.argmin(-1))


# ------------------------------------------------------------------------------------------------ Phenaki.sample: refusals and wrapper calls

@pytest.mark.parametrize('kw,msg', [
    (dict(top_p=0.), 'top_p'), (dict(top_p=0), 'top_p'), (dict(top_p=-0.1), 'top_p'), (dict(top_p=1.0001), 'top_p'), (dict(top_p=2), 'top_p'),
    (dict(top_p=float('nan')), 'top_p'), (dict(top_p=float('inf')), 'top_p'), (dict(top_p='0.9'), 'top_p'), (dict(top_p=True), 'top_p'),
    (dict(min_p=1.), 'min_p'), (dict(min_p=1), 'min_p'), (dict(min_p=-0.1), 'min_p'), (dict(min_p=float('nan')), 'min_p'),
    (dict(min_p=float('inf')), 'min_p'), (dict(min_p='0.1'), 'min_p'), (dict(min_p=False), 'min_p'),
    (dict(top_p=0.9, min_p=1.5), 'min_p'), (dict(top_p=0.9, top_k=0), 'top_k'), (dict(top_p=0.9, filter_thres=0.5, top_k=3), 'not both'),
    (dict(top_p=0.9, _noise_fn='torch'), 'torch'), (dict(min_p=0.1, _noise_fn='torch'), 'torch')])
def test_bad_nucleus_arguments_are_refused_before_anything_launches(kw, msg):
    ph = SC.make('token')
    rec = SC.Recorder()
    with recording(rec), pytest.raises(ValueError, match=msg):
        ph.sample(num_frames=5, batch_size=B, **kw)
    assert rec.calls == []


OFF = (dict(top_p=None, min_p=None), dict(top_p=1), dict(top_p=1.0), dict(min_p=0), dict(min_p=0.), dict(top_p=1.0, min_p=0.))


@pytest.mark.parametrize('critic', [None, 'token'])
@pytest.mark.parametrize('topk', [{}, dict(top_k=3)])
def test_the_off_values_are_the_path_without_the_arguments(critic, topk):
    ph = SC.make(critic)
    base, _ = run(ph, num_frames=5, batch_size=B, _seed=7, **topk)
    key = ph._pk_last_sample_key
    assert len(key) == 16 and key[-1] == (3 if topk else None) and (key[-1] is None or type(key[-1]) is int)
    assert ('vocab_sample_filtered' in base.names()) == bool(topk) and ('vocab_sample' in base.names()) == (not topk)
    for kw in OFF:
        rec, _ = run(ph, num_frames=5, batch_size=B, _seed=7, **topk, **kw)
        assert FH._normalised(rec) == FH._normalised(base), kw
        assert not any(n in rec.names() for n in NEW)
        assert ph._pk_last_sample_key == key and type(ph._pk_last_sample_key[-1]) is type(key[-1])


@pytest.mark.parametrize('critic', [None, 'token'])
@pytest.mark.parametrize('compact', [True, False])
@pytest.mark.parametrize('kw,want', [(dict(top_p=0.5), (V, 0.5, 0.)), (dict(min_p=0.05), (V, 1., 0.05)), (dict(top_k=3, top_p=0.9, min_p=0.25), (3, 0.9, 0.25)),
                                     (dict(filter_thres=0.9, min_p=0.5), (25, 1., 0.5)), (dict(top_k=V, top_p=0.5), (V, 0.5, 0.))])
def test_with_a_nucleus_filter_every_step_is_one_nucleus_head(critic, compact, kw, want):
    ph = SC.make(critic)
    rec, out = run(ph, num_frames=5, batch_size=B, _seed=7, _compact=compact, **kw)
    head = ['embeds', 'cfg_mix', 'vocab_sample_nucleus']
    assert rec.names() == SC.loop_names(head + (SC.CRITIC if critic else []), head)
    assert out.shape == (B, 3, 5, 64, 64)
    heads = SC.calls(rec, 'vocab_sample_nucleus')
    need_lse = critic is None
    slab = heads[0][1][19]
    assert slab.shape == (B * N, V) and slab.dtype == torch.float32
    for s, c in enumerate(heads):
        a = c[1]
        assert len(a) == 20
        assert a[4:7] == (B * SC.KS[s] if (compact and s > 0) else B * N, V, TINY['maskgit']['dim'])       # M, V, D
        assert a[7:10] == want and type(a[7]) is int and type(a[8]) is float and type(a[9]) is float      # k, top_p, min_p
        assert a[10] == float(0.9 * ((STEPS - s - 1) / STEPS)) and a[11] is None                          # temperature; no injected noise
        assert (a[12] is not None) == (compact and s > 0)                                                 # the compact row list
        assert a[13] == (7 + s * 0x9E3779B97F4A7C15) & SC.M64 and a[14] is need_lse
        assert a[15].shape == (B, N) and a[16].shape == (B, N) and a[17].shape == (B, N) and (a[18] is not None) == need_lse
        assert a[19] is slab and c[2] == dict(seed_dev=None)
    if need_lse:                                                                                          # the scores ping-pong as on the plain path
        for s, c in enumerate(SC.calls(rec, 'topk_mask'), start=1):
            assert c[1][0] is heads[s - 1][1][18] and c[2]['scores_next'] is heads[s][1][18]


def test_the_key_names_the_nucleus():
    ph = SC.make('token')
    keys = {}
    for name, kw in (('plain', {}), ('k3', dict(top_k=3)), ('p5', dict(top_p=0.5)), ('p9', dict(top_p=0.9)), ('m', dict(min_p=0.05)),
                     ('k3p5', dict(top_k=3, top_p=0.5)), ('t9p5m', dict(filter_thres=0.9, top_p=0.5, min_p=0.25)), ('kVp5', dict(top_k=V, top_p=0.5))):
        run(ph, num_frames=5, batch_size=B, **kw)
        keys[name] = ph._pk_last_sample_key
    assert all(len(k) == 16 for k in keys.values()) and len({k[:-1] for k in keys.values()}) == 1
    assert keys['plain'][-1] is None and keys['k3'][-1] == 3
    assert keys['p5'][-1] == ('nucleus', None, 0.5, 0.0) and keys['p9'][-1] == ('nucleus', None, 0.9, 0.0) and keys['m'][-1] == ('nucleus', None, 1.0, 0.05)
    assert keys['k3p5'][-1] == ('nucleus', 3, 0.5, 0.0) and keys['t9p5m'][-1] == ('nucleus', 25, 0.5, 0.25) and keys['kVp5'] == keys['p5']
    assert all(type(x) is float for x in keys['k3p5'][-1][2:])
    assert len(set(keys.values())) == 7


def test_the_forwarders_pass_the_nucleus_on():
    from tests import test_infill_host as TI
    ph = SC.make('token')
    ids0, known = TI._known()
    rec, _ = run(ph, num_frames=5, batch_size=B, known_ids=ids0, known_mask=known, top_p=0.5)
    heads = SC.calls(rec, 'vocab_sample_nucleus')
    assert 'vocab_sample' not in rec.names() and 'vocab_sample_filtered' not in rec.names() and len(heads) == STEPS
    _, _, totals = SC.PH.infill_schedule([32, 36], STEPS)
    assert [c[1][4] for c in heads] == totals and all(c[1][7:10] == (V, 0.5, 0.) for c in heads)
    rec = SC.Recorder()
    with recording(rec):
        ph.sample_images(batch_size=B, top_p=0.9, min_p=0.05)
        SC.PH.make_video(ph, texts=['a', 'b'], num_frames=(5, 4), prime_lengths=1, top_p=0.9, min_p=0.05)
        out = D.sample_sharded(ph, num_frames=5, batch_size=B, top_p=0.9, min_p=0.05)
        video = torch.zeros(B, 3, 5, 64, 64)
        edit = torch.ones(B, 3, 4, 4, dtype=torch.bool)
        ph.infill(video, edit, mask_level='token', top_p=0.9, min_p=0.05)
    heads = SC.calls(rec, 'vocab_sample_nucleus')
    assert out.shape == (B, 3, 5, 64, 64)
    assert len(heads) == 5 * STEPS and all(c[1][7:10] == (V, 0.9, 0.05) for c in heads)
    assert 'vocab_sample' not in rec.names() and 'vocab_sample_filtered' not in rec.names()


# ------------------------------------------------------------------------------------------------ the slab walk

@pytest.mark.parametrize('with_rows', [False, True])
def test_vocab_sample_nucleus_walks_the_rows_slab_by_slab(with_rows):
    rec = SC.Recorder()
    saved = [(k, getattr(L, k)) for k in ('gemm', 'logits_nucleus_sample', 'logits_topk_sample')]
    M, Vv, Dd = 130, 1156, 40
    A, W, bias = torch.zeros(M + 5, Dd + 8)[:, :Dd], torch.zeros(Vv, 64), torch.zeros(Vv)
    rows = torch.arange(M, dtype=torch.int32) * 2 if with_rows else None
    pred = torch.zeros(2 * M, dtype=torch.int64)
    try:
        for k, _ in saved:
            setattr(L, k, rec.stub(k))
        L.vocab_sample_nucleus(L.F32, A, W, bias, M, Vv, Dd, 7, 0.9, 0.05, 0.5, None, rows, 11, True, None, None, pred, None, torch.zeros(64, Vv), seed_dev=None)
        n_split = len(rec.calls)
        L.vocab_sample_nucleus(L.F32, A, W, bias, 50, Vv, Dd, 7, 0.9, 0.05, 0.5, None, rows, 11, True, None, None, pred, None, torch.zeros(64, Vv))
        L.vocab_sample_nucleus(L.F32, A, W, bias, 64, Vv, Dd, 7, 0.9, 0.05, 0.5, None, rows, 11, True, None, None, pred, None, torch.zeros(64, Vv))
    finally:
        for k, v in saved:
            setattr(L, k, v)
    assert rec.names() == ['gemm', 'logits_nucleus_sample'] * 5 and n_split == 6
    gemms, sels = SC.calls(rec, 'gemm'), SC.calls(rec, 'logits_nucleus_sample')
    for j, (m0, Rc) in enumerate(((0, 64), (64, 64), (128, 2), (0, 50), (0, 64))):
        g, s = gemms[j], sels[j]
        assert g[1][0] == L.F32 and g[1][3:] == (Rc, Vv, Dd) and g[1][2] is W and g[2]['bias'] is bias
        assert g[1][1].shape == (Rc, Dd) and g[1][1].data_ptr() == A[m0:].data_ptr() and g[1][1].stride(0) == A.stride(0)
        assert g[2]['C'].shape == (Rc, Vv) and g[2]['C'].data_ptr() == s[1][0].data_ptr()               # the slab's first Rc rows, then sampled
        assert s[1][1:7] == (Rc, Vv, 7, 0.9, 0.05, 0.5) and s[1][10:12] == (11, True) and s[2] == dict(seed_dev=None)
        if with_rows:
            assert torch.equal(s[1][8], rows[m0:m0 + Rc]) and s[1][8].data_ptr() == rows[m0:].data_ptr() and s[1][9] == 0
        else:
            assert s[1][8] is None and s[1][9] == m0


# ------------------------------------------------------------------------------------------------ the margins of the GPU end-to-end test

def _oracle_steps(base, with_critic, top_p):
    cv_sd, mg_sd, cr_sd = state_dicts('tiny')
    _, mgc, crc = oracle_cfgs(TINY)
    ctx = weights.synthetic_context(2, 6, TINY['maskgit']['dim_context'], seed=2)
    nf = lambda kind, step, shape: weights.uniform_noise(tuple(shape), base + 2 * step + (1 if kind == 'critic' else 0))
    return NR.oracle_nucleus_sample(O, mg_sd, mgc, cr_sd if with_critic else None, crc, batch=2, n=48, patch_shape=(3, 4, 4), context=ctx,
                                    steps=TINY['steps'], top_p=top_p, noise_fn=nf)


@pytest.mark.parametrize('with_critic', [True, False])
@pytest.mark.parametrize('base', NR.E2E_SEEDS)
def test_the_end_to_end_band_check_discriminates(base, with_critic):
    """from the oracle alone, TINY, top_p = 0.5: the acceptance the GPU test applies to the device's draws (a) takes every draw of the oracle's own
    nucleus loop, at every step, and (b) rejects at least a quarter of the UNFILTERED oracle draws at step 0: it cannot pass vacuously"""
    p = NR.E2E_TOP_P
    for rec in _oracle_steps(base, with_critic, p):
        ok = NR.e2e_accept(rec['ref'].l64, rec['E'], rec['temperature'], p, rec['pred'].reshape(-1))
        assert ok.all(), f'step with T = {rec["temperature"]}: {int((~ok).sum())} of the oracle\'s own nucleus draws are rejected'
    first = _oracle_steps(base, with_critic, None)[0]
    ok = NR.e2e_accept(first['ref'].l64, first['E'], first['temperature'], p, first['pred'].reshape(-1))
    assert first['mask'].all() and ok.numel() == 2 * 48
    assert (~ok).float().mean() >= 0.25, f'only {int((~ok).sum())} of {ok.numel()} unfiltered draws fall outside the nucleus band'
    # the greedy end: top_p = 1e-6 keeps the maximum and its ties, as top_k = 1 does
    l64 = first['ref'].l64
    assert torch.equal(NR.nucleus64(l64, first['temperature'], 256, 1e-6, 0.)[0], R.select64(l64, 1)[0])
