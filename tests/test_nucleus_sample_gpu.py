"""Nucleus / min-p filtered sampling on the MI355X (-m gpu): pk_logits_nucleus_sample on given logits -- its cut and count inside the restatement's
band (tests/nucleus_sample_restatement.py), exact on the designed rows, the bits of pk_logits_topk_sample with both filters off, bit-identical reruns,
the draw inside the accept set --, its refusals, the slabbed head from operands (_lib.vocab_sample_nucleus) and Phenaki.sample(top_p=, min_p=) end to
end on TINY against the oracle's logits of every recorded step."""
import math

import pytest
import torch

from oracle import phenaki_oracle as O
from oracle import weights
from oracle.configs import TINY, oracle_cfgs, state_dicts
from phenaki_pytorch_amd import _lib as L
from tests import filtered_sample_restatement as R
from tests import nucleus_sample_restatement as NR
from tests import vocab_reference as VR
from tests.gemm_reference import BF16X3, F32, NAN, TNAME
from tests.test_filtered_sample_gpu import GRID, Launch, _product, stream
from tests.util import noise_fn_cuda, record_parity

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

OK, EINVAL = 0, -1
SENT = VR.SENTINEL


@pytest.fixture(scope='module')
def lib():
    from phenaki_pytorch_amd import build
    build.build(verbose=False)
    return L.load()


class NLaunch(Launch):
    """tests/test_filtered_sample_gpu.Launch (sentinel-filled outputs, NaN-padded logits) for pk_logits_nucleus_sample"""

    def nargs(self, k, top_p, min_p, T, seed, seed_dev, flags):
        a = self.args(k, T, seed, seed_dev, flags)
        return a[:5] + [float(top_p), float(min_p)] + a[5:]

    def nrun(self, lib, k, top_p, min_p, T=1.0, seed=0, seed_dev=None, lse=False, no_noise=False):
        rc = lib.pk_logits_nucleus_sample(*self.nargs(k, top_p, min_p, T, seed, seed_dev, (1 if lse else 0) | (2 if no_noise else 0)), stream())
        torch.cuda.synchronize()
        assert rc == OK, f'pk_logits_nucleus_sample returned {rc}'
        return self


def _same_bits(x, y, what):
    assert torch.equal(x.pred, y.pred) and torch.equal(x.kept, y.kept), f'{what}: pred or kept_out differ'
    if x.ids is not None:
        assert torch.equal(x.ids, y.ids), f'{what}: ids differ'
    if x.scores is not None:
        VR.assert_same_bits(x.scores, y.scores, f'{what}: scores')
    VR.assert_same_bits(x.cut, y.cut, f'{what}: cut_out')


# ------------------------------------------------------------------------------------------------ the band check

@pytest.mark.parametrize('kind', NR.data_kinds())
@pytest.mark.parametrize('M,V', R.SELECT_SHAPES)
def test_cut_and_count_lie_in_the_band(lib, M, V, kind):
    """every row, every combination of temperature, top_p, min_p and k; nothing outside the named outputs is written; without noise the row's first
    maximum is kept and wins"""
    inside_ties = False
    for T in NR.TEMPERATURES:
        l = NR.nucleus_data(kind, M, V, T)
        l64 = l.double()
        first_max = l64.argmax(-1)
        for k in (V, max(V // 10, 1)):
            for top_p in NR.TOP_PS:
                for min_p in NR.MIN_PS:
                    what = f'{kind} {M}x{V} T={T} k={k} top_p={top_p} min_p={min_p}'
                    x = NLaunch(l).nrun(lib, k, top_p, min_p, T, no_noise=True)
                    NR.check_nucleus(l64, 0., T, k, top_p, min_p, x.cut[:M], x.kept[:M], what)
                    x.check_untouched(what)
                    assert torch.equal(x.pred_rows(), first_max), f'{what}: without noise the first maximum wins'
                    if kind == 'dyadic' and k == V and min_p == 0 and T > 0:
                        inside_ties |= bool((x.kept[:M].cpu().long() > NR.prefix_count64(l64, T, top_p)).any())
                    if kind == 'constant':
                        assert (x.kept[:M].cpu() == V).all() and (x.cut[:M].cpu() == 1.5).all(), f'{what}: a constant row keeps all V columns'
                    if kind == 'mixed' and V >= 1000:                            # every weight but the maximum's underflows
                        assert (x.kept[:M].cpu().long() == (l64 == l64.max(-1, keepdim=True).values).sum(-1)).all(), f'{what}: the kept set is the maximum'
    if kind == 'dyadic' and V >= 1000:
        assert inside_ties, 'the dyadic grid must put the cut inside a run of equal values somewhere'


@pytest.mark.parametrize('T', [1.0, 0.225])
@pytest.mark.parametrize('V', [8, 1000, 4100, 65536])
def test_designed_rows_give_the_exact_counts(lib, V, T):
    masses, cases = NR.DESIGNED
    g = VR._gen(f'nucleus/designed_exact/{V}')
    perm = torch.randperm(V, generator=g)
    row = NR.designed_row(masses, V, NR.f32(T)).float()
    tie = NR.designed_row(NR.DESIGNED_TIE[0], V, NR.f32(T)).float()
    l = torch.stack([row, row[perm], tie, tie[perm]])
    for p, want in cases + ((NR.DESIGNED_TIE[1], None),):
        x = NLaunch(l).nrun(lib, V, p, 0., T, no_noise=True)
        kept = x.kept[:4].cpu().tolist()
        assert kept[2:] == [NR.DESIGNED_TIE[2]] * 2 if want is None else kept[:2] == [want] * 2, f'V={V} T={T} top_p={p}: kept {kept}'
        assert torch.equal(x.pred_rows(), l.double().argmax(-1))
        NR.check_nucleus(l.double(), 0., T, V, p, 0., x.cut[:4], x.kept[:4], f'designed V={V} T={T} top_p={p}')
    # min-p 0.2 of the largest mass 0.5 keeps 0.3 and 0.15, not 0.05; on top of top-k 2 the nucleus is taken on the top-k set's own mass 0.8
    assert NLaunch(l).nrun(lib, V, 1., 0.2, T, no_noise=True).kept[:2].cpu().tolist() == [3, 3]
    assert NLaunch(l).nrun(lib, 2, 0.7, 0., T, no_noise=True).kept[:2].cpu().tolist() == [2, 2]
    assert NLaunch(l).nrun(lib, 2, 0.6, 0., T, no_noise=True).kept[:2].cpu().tolist() == [1, 1]


# ------------------------------------------------------------------------------------------------ both filters off: the top-k kernel's bits

@pytest.mark.parametrize('M,V', R.SELECT_SHAPES)
def test_with_both_filters_off_the_bits_are_the_top_k_kernels(lib, M, V):
    g = VR._gen(f'nucleus/off/{M}/{V}')
    l = R.select_data('normal', M, V)
    total = 2 * M + 5
    rows = torch.randperm(total, generator=g)[:M]
    mask = torch.rand(total, generator=g) > 0.4
    ids0 = torch.randint(0, V, (total,), generator=g)
    mk = lambda: NLaunch(l, rows=rows, total=total, mask=mask, ids0=ids0, scores=True)
    for k in R.select_ks(V):
        for T, seed, seed_dev in ((0.7, 0x1234567890ABCDEF, 0x1111), (0., 5, None)):
            x = mk().run(lib, k, T, seed, seed_dev, lse=True)
            y = mk().nrun(lib, k, 1., 0., T, seed, seed_dev, lse=True)
            _same_bits(x, y, f'{M}x{V} k={k} T={T}')
            y.check_untouched(f'{M}x{V} k={k} T={T}')
    U = torch.rand(M, V, generator=g)
    x = NLaunch(l, rows=rows, total=total, U=U, mask=mask, ids0=ids0, scores=True).run(lib, max(V // 10, 1), 0.45, lse=True)
    y = NLaunch(l, rows=rows, total=total, U=U, mask=mask, ids0=ids0, scores=True).nrun(lib, max(V // 10, 1), 1., 0., 0.45, lse=True)
    _same_bits(x, y, f'{M}x{V} injected noise')


@pytest.mark.parametrize('M,V', [(130, 1024), (2, 65536)])
def test_two_calls_agree_bit_for_bit(lib, M, V):
    g = VR._gen(f'nucleus/twice/{M}/{V}')
    l = R.select_data('normal', M, V)
    mask = torch.rand(M, generator=g) > 0.4
    ids0 = torch.randint(0, V, (M,), generator=g)
    for k, top_p, min_p in ((V, 0.9, 0.), (V, 1., 0.05), (max(V // 10, 1), 0.9, 0.05), (V, 0.5, 0.5)):
        run = lambda: NLaunch(l, mask=mask, ids0=ids0, scores=True).nrun(lib, k, top_p, min_p, 0.7, seed=99, lse=True)
        _same_bits(run(), run(), f'{M}x{V} k={k} top_p={top_p} min_p={min_p}')


# ------------------------------------------------------------------------------------------------ the draw

SM, SV = 37, 1156


@pytest.mark.parametrize('mode,T', [(R.PARITY, 0.45), (R.FAST, 0.7), (R.FAST, 0.), (R.PARITY, 1e-12)])
def test_draws_lie_in_the_accept_set(lib, mode, T):
    """pred inside R's accept set at k' = kept_out (the noise indexed by the logical row), scores within R.score_ref's bound, mask / ids as
    pk_vocab_reduce writes them"""
    g = VR._gen(f'nucleus/draw/{mode}/{T}')
    l = torch.randn(SM, SV, generator=g).float()
    total = 2 * SM + 5
    rows = torch.randperm(total, generator=g)[:SM]
    U = torch.rand(SM, SV, generator=g) if mode == R.PARITY else None
    mask = torch.rand(total, generator=g) > 0.4
    ids0 = torch.randint(0, SV, (total,), generator=g)
    seed, seed_dev = 0x1234567890ABCDEF, (0x1111 if mode == R.FAST else None)
    ref = R.noisy_ref(l.double(), torch.zeros(SM, SV, dtype=torch.float64), mode, T, U=U, seed=seed, seed_dev=seed_dev, rows=rows)
    shares = {}
    for k, top_p, min_p in ((SV, 0.5, 0.), (SV, 0.9, 0.), (SV, 1., 0.05), (115, 0.9, 0.05), (SV, 1e-6, 0.)):
        what = f'{mode} T={T} k={k} top_p={top_p} min_p={min_p}'
        x = NLaunch(l, rows=rows, total=total, U=U, mask=mask, ids0=ids0, scores=True).nrun(lib, k, top_p, min_p, T, seed, seed_dev, lse=True)
        NR.check_nucleus(l.double(), 0., T, k, top_p, min_p, x.cut[:SM], x.kept[:SM], what)
        x.check_untouched(what)
        pred = x.pred_rows()
        amb = NR.accept_draw(ref, x.kept[:SM], pred, what)
        shares[what] = 1 - amb / SM
        if top_p == 1e-6:
            assert torch.equal(pred, l.double().argmax(-1)), f'{what}: the nucleus of a tiny top_p is the arg-max whatever the noise'
        sc = x.scores.cpu()[x.lrows]
        on = x.mask.cpu().bool()[x.lrows]
        assert (sc[~on] == -1e4).all(), f'{what}: a masked-out row\'s score is not -1e4'
        want, bound = R.score_ref(ref, pred)
        VR.assert_within(sc[on], want[on], bound[on], f'{what}: scores')
    record_parity('nucleus_sample_given_logits', dict(mode=str(mode), T=T, singleton_share=shares))
    if T >= 0.4:
        assert min(shares.values()) >= 0.9


# ------------------------------------------------------------------------------------------------ return codes

def test_refusals_leave_the_outputs_untouched(lib):
    l = torch.randn(6, 132)
    base = dict(k=5, top_p=0.9, min_p=0.05, T=0.7, seed=1, seed_dev=None, flags=1)
    nan = float('nan')
    # argument positions: 0 logits, 1 ldl, 2 M, 3 V, 4 k, 5 top_p, 6 min_p, 9 rows, 10 row_base, 13 flags, 16 pred, 17 scores
    changes = [('top_p = 0', {5: 0.}), ('top_p < 0', {5: -0.5}), ('top_p > 1', {5: 1.5}), ('top_p NaN', {5: nan}), ('top_p inf', {5: math.inf}),
               ('min_p < 0', {6: -0.1}), ('min_p = 1', {6: 1.}), ('min_p > 1', {6: 2.}), ('min_p NaN', {6: nan}),
               ('k = 0', {4: 0}), ('k > V', {4: 133}), ('V < 4', {3: 0, 4: 1}), ('V % 4', {3: 130}), ('V > 65536', {3: 65540, 1: 65540}),
               ('ldl < V', {1: 128}), ('ldl % 4', {1: 134}), ('M = 0', {2: 0}), ('M < 0', {2: -1}), ('logits NULL', {0: None}), ('pred NULL', {16: None}),
               ('scores without bit 0', {13: 0}), ('scores with only bit 1', {13: 2}), ('rows with row_base', {10: 1})]
    for what, ch in changes:
        x = NLaunch(l, rows=torch.arange(6), total=9, mask=torch.ones(9, dtype=torch.bool), ids0=torch.arange(9), scores=True)
        a = x.nargs(**base)
        for i, v in ch.items():
            a[i] = v
        assert lib.pk_logits_nucleus_sample(*a, stream()) == EINVAL, what
        torch.cuda.synchronize()
        assert (x.pred.cpu() == SENT).all() and torch.equal(x.ids.cpu(), x.ids0) and (x.kept.cpu() == SENT).all(), what
        VR.assert_untouched(x.scores, what)
        VR.assert_untouched(x.cut, what)
    x = NLaunch(l, scores=True)
    assert lib.pk_logits_nucleus_sample(*x.nargs(**base), stream()) == OK


# ------------------------------------------------------------------------------------------------ the slabbed head from operands

@pytest.mark.parametrize('dtype', [F32, BF16X3])
def test_the_slabbed_nucleus_head_from_operands(lib, dtype):
    """L.vocab_sample_nucleus on 200 rows x V = 1156 x D = 40 in slabs of 64, 64, 64 and 8 rows at T = 1, with the logit bound E of
    tests/test_filtered_sample_gpu.py::test_the_slabbed_head_from_operands for the mode: every draw lies inside the band of the float64 logits, and
    the cut and count the kernel reports on the logits of the last slab lie in the restatement's band"""
    M, V, D, SLAB = 200, 1156, 40, 64
    for rows in (None, 'perm'):
        for noise in (VR.FAST, VR.PARITY):
            c = VR._case(f'nucleus/head/{TNAME[dtype]}/{rows}/{noise}', dtype, M, V, D, noise, 1, T=1.0, rows=rows)
            x = VR.build(c)
            t = VR.device_operands(c, x, 'cuda')
            ref = VR.reference(c, x)
            E = float(ref.E.max())
            total = x.geo.total
            lr = VR.lrows(c, x)
            named = torch.zeros(total, dtype=torch.bool)
            named[lr] = True
            mask = (torch.rand(total, generator=VR._gen(c.name + '/mask')) > 0.4).to(torch.uint8)
            for k, top_p, min_p in ((V, 0.5, 0.), (V, 0.9, 0.05), (115, 0.9, 0.), (V, 1., 0.25)):
                what = f'{c.name} k={k} top_p={top_p} min_p={min_p}'
                slab = torch.full((SLAB, V), NAN, device='cuda')
                pred = torch.full((total,), SENT, dtype=torch.int64).cuda()
                ids = torch.arange(total).cuda()
                scores = torch.full((total,), NAN).cuda()
                L.vocab_sample_nucleus(dtype, t['A'], t['W'], t['bias'], M, V, D, k, top_p, min_p, float(c.T), t.get('U'), t.get('rows'), c.seed, True,
                                       mask.cuda(), ids, pred, scores, slab)
                # the logits of the last slab are still there: the kernel's own cut and count on them
                last = M - M % SLAB
                cut = torch.full((M - last,), NAN).cuda()
                kept = torch.full((M - last,), SENT, dtype=torch.int32).cuda()
                scratch = torch.full((total,), SENT, dtype=torch.int64).cuda()
                L.logits_nucleus_sample(slab, M - last, V, k, top_p, min_p, float(c.T), None, None, 0, 0, False, None, None, scratch, None, no_noise=True,
                                        cut_out=cut, kept_out=kept)
                torch.cuda.synchronize()
                NR.check_nucleus(ref.l64[last:], E, c.T, k, top_p, min_p, cut, kept, what + ' (last slab)')
                p = pred.cpu()
                assert (p[~named] == SENT).all(), f'{what}: pred written outside the named rows'
                assert ((p[lr] >= 0) & (p[lr] < V)).all()
                # every draw: not surely outside any active filter's set
                if top_p < 1:
                    ok = NR.e2e_accept(ref.l64, E, c.T, top_p, p[lr])
                    assert ok.all(), f'{what}: {int((~ok).sum())} draws lie outside the nucleus'
                if min_p > 0:
                    arg = (ref.l64.gather(-1, p[lr][:, None])[:, 0] - ref.l64.max(-1).values) / c.T
                    assert (arg >= math.log(min_p) - NR._eps(min_p, E, c.T)).all(), f'{what}: a draw fails min-p'
                if k < V:
                    assert R.bands(ref, k)[0].gather(-1, p[lr][:, None]).all(), f'{what}: a draw outside the top-k'
                on = mask.bool()
                want_ids = torch.arange(total)
                want_ids[named & on] = p[named & on]
                assert torch.equal(ids.cpu(), want_ids), f'{what}: ids'
                sc = scores.cpu()
                VR.assert_untouched(sc[~named], f'{what}: scores outside the named rows')
                assert (sc[named & ~on] == -1e4).all()
                want, bound = R.score_ref(ref, p[lr])
                VR.assert_within(sc[lr][on[lr]], want[on[lr]], bound[on[lr]], f'{what}: scores')


# ------------------------------------------------------------------------------------------------ Phenaki.sample end to end

def _oracle_logits(t, ctx):
    _, mg_sd, _ = state_dicts('tiny')
    _, mgc, _ = oracle_cfgs(TINY)
    ids = t['masked_ids'].cpu()
    c = ctx[:ids.shape[0]]
    return O.maskgit_cfg(mg_sd, mgc, ids, cond_scale=5., video_patch_shape=GRID, context=c, text_mask=(c != 0).any(-1))


@pytest.mark.parametrize('base', NR.E2E_SEEDS)
@pytest.mark.parametrize('with_critic', [True, False])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
def test_sample_with_a_nucleus_draws_inside_it(dtype, with_critic, base):
    """greedy: top_p = 1e-6 returns what top_k = 1 returns at every traced step; band: at top_p = 0.5 every drawn token of every traced step satisfies
    share64{l > l[v] + 2E} exp(-4E/T) < 0.5 + DELTA against the oracle's logits of that step, E = R.E2E_REL max|logits| (what this rejects and takes
    on the oracle alone: tests/test_nucleus_sample_host.py::test_the_end_to_end_band_check_discriminates)"""
    ph, ctx = _product(with_critic, dtype)
    kw = dict(texts=['a', 'b'], num_frames=5, cond_scale=5., _return_ids=True)
    tg, t1 = [], []
    _, ids_g = ph.sample(top_p=1e-6, _noise_fn=noise_fn_cuda(base), _trace=tg, _seed=base, **kw)
    _, ids_1 = ph.sample(top_k=1, _noise_fn=noise_fn_cuda(base), _trace=t1, _seed=base, **kw)
    assert len(tg) == len(t1) == TINY['steps'] and torch.equal(ids_g, ids_1)
    for s, (a, b) in enumerate(zip(tg, t1)):
        assert torch.equal(a['ids'], b['ids']) and torch.equal(a['pred'], b['pred']), f'step {s}: the greedy nucleus and top-1 disagree'
    trace = []
    vid, ids = ph.sample(top_p=NR.E2E_TOP_P, _noise_fn=noise_fn_cuda(base), _trace=trace, **kw)
    assert vid.shape == (2, 3, 5, 64, 64) and torch.isfinite(vid).all() and ((ids >= 0) & (ids < 256)).all()
    steps, checked = TINY['steps'], 0
    assert len(trace) == steps
    with O.precision(dtype):
        for s, t in enumerate(trace):
            logits = _oracle_logits(t, ctx)
            l64 = logits.reshape(-1, logits.shape[-1]).double()
            E = R.E2E_REL * float(l64.abs().max())
            T = 0.9 * ((steps - (s + 1)) / steps)
            m = t['mask'].cpu().reshape(-1)
            ok = NR.e2e_accept(l64, E, T, NR.E2E_TOP_P, t['pred'].cpu().reshape(-1))
            assert ok[m].all(), f'{dtype} critic={with_critic} base={base} step {s}: {int((~ok[m]).sum())} of {int(m.sum())} draws lie outside the nucleus'
            checked += int(m.sum())
            mm = t['mask'].cpu()
            assert torch.equal(t['ids'].cpu()[mm], t['pred'].cpu()[mm]) and torch.equal(t['ids'].cpu()[~mm], t['masked_ids'].cpu()[~mm])
    assert checked >= 2 * 48 + steps - 1


def test_graph_replay_and_eager_agree_and_another_top_p_captures_another_graph():
    ph, _ = _product(True)
    kw = dict(texts=['a', 'b'], num_frames=5, cond_scale=5., _return_ids=True, _seed=0x1234567812345678 & 0x3FFFFFFFFFFFFFFF)
    v_e, ids_e = ph.sample(top_p=0.5, **kw)
    _, ids_plain = ph.sample(**kw)
    _, ids_m = ph.sample(top_p=0.5, min_p=0.25, top_k=25, **kw)
    ph.enable_sample_graph(True)
    try:
        for _ in range(2):                                                        # capture, then a pure replay
            v_g, ids_g = ph.sample(top_p=0.5, **kw)
            assert torch.equal(ids_g, ids_e) and torch.equal(v_g, v_e)
        assert len(ph.__dict__['_pk_sample_graphs']) == 1
        ph.sample(top_p=0.9, **kw)
        assert len(ph.__dict__['_pk_sample_graphs']) == 2
        assert torch.equal(ph.sample(top_p=0.5, min_p=0.25, top_k=25, **kw)[1], ids_m) and len(ph.__dict__['_pk_sample_graphs']) == 3
        assert torch.equal(ph.sample(top_p=0.5, top_k=256, **kw)[1], ids_e) and len(ph.__dict__['_pk_sample_graphs']) == 3
        assert torch.equal(ph.sample(top_p=1.0, min_p=0., **kw)[1], ids_plain) and len(ph.__dict__['_pk_sample_graphs']) == 4
    finally:
        ph.enable_sample_graph(False)
    assert torch.equal(ph.sample(top_p=0.5, **kw)[1], ids_e)


def test_infill_make_video_and_sample_images_take_the_nucleus():
    from phenaki_pytorch_amd import make_video
    ph, _ = _product(True)
    torch.manual_seed(3)
    video = torch.rand(2, 3, 5, 64, 64).cuda()
    edit = torch.zeros(2, *GRID, dtype=torch.bool)
    edit[:, 1:] = True                                                            # keep token frame 0
    tokens = ph.cvivit(video, return_only_codebook_ids=True).reshape(2, -1)
    out, ids = ph.infill(video, edit, texts=['a', 'b'], mask_level='token', top_p=0.9, min_p=0.05, _return_ids=True, _seed=11)
    keep = ~edit.reshape(2, -1).cuda()
    assert out.shape == video.shape and torch.equal(ids[keep], tokens[keep]) and ((ids >= 0) & (ids < 256)).all()
    whole, scenes = make_video(ph, texts=['a', 'b'], num_frames=(5, 4), prime_lengths=1, top_p=0.9)
    assert whole.shape == (1, 3, 9, 64, 64) and len(scenes) == 2 and torch.isfinite(whole).all()
    img = ph.sample_images(texts=['a', 'b'], cond_scale=5., top_k=64, top_p=0.9)
    assert img.shape == (2, 3, 64, 64)
