"""Top-k filtered sampling on the MI355X (-m gpu): pk_logits_topk_sample on given logits -- the select exact, the draw inside the restatement's accept
set (tests/filtered_sample_restatement.py) --, its refusals, the slabbed head from operands (_lib.vocab_sample_filtered) and
Phenaki.sample(filter_thres=, top_k=) end to end on TINY against the oracle's logits of every recorded step."""
import math

import pytest
import torch

from oracle import phenaki_oracle as O
from oracle import weights
from oracle.configs import TINY, oracle_cfgs, state_dicts
from phenaki_pytorch_amd import _lib as L
from phenaki_pytorch_amd import make_video
from tests import filtered_sample_restatement as R
from tests import vocab_reference as VR
from tests.gemm_reference import BF16, BF16X3, F32, NAN, TNAME
from tests.util import load_product, noise_fn_cuda, record_parity

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

OK, EINVAL = 0, -1
SENT = VR.SENTINEL
GUARD = 3                          # rows behind M in the logits buffer and entries behind M in cut_out / kept_out
PAD = 4                            # ldl = V + PAD, NaN behind column V


@pytest.fixture(scope='module')
def lib():
    from phenaki_pytorch_amd import build
    build.build(verbose=False)
    return L.load()


def stream():
    return torch.cuda.current_stream().cuda_stream


def _p(t):
    return None if t is None else t.data_ptr()


class Launch:
    """one pk_logits_topk_sample call on sentinel-filled outputs: logits (M, V) f32 on the CPU sit in an (M + GUARD, V + PAD) NaN buffer; `total`
    logical rows; U (M, V) is scattered to the logical rows of a (total, V) NaN buffer"""

    def __init__(self, l, *, rows=None, total=None, row_base=0, U=None, mask=None, ids0=None, scores=False, outs=True):
        self.M, self.V = l.shape
        self.total = total if total is not None else row_base + self.M
        self.lrows = rows.long() if rows is not None else torch.arange(row_base, row_base + self.M)
        buf = torch.full((self.M + GUARD, self.V + PAD), NAN)
        buf[:self.M, :self.V] = l
        self.logits = buf.cuda()
        self.rows = None if rows is None else rows.to(torch.int32).cuda()
        self.row_base = row_base
        self.U = None
        if U is not None:
            full = torch.full((self.total, self.V), NAN)
            full[self.lrows] = U
            self.U = full.cuda()
        self.mask = None if mask is None else mask.to(torch.uint8).cuda()
        self.ids0 = ids0
        self.ids = None if ids0 is None else ids0.clone().cuda()
        self.pred = torch.full((self.total,), SENT, dtype=torch.int64).cuda()
        self.scores = torch.full((self.total,), NAN).cuda() if scores else None
        self.cut = torch.full((self.M + GUARD,), NAN).cuda() if outs else None
        self.kept = torch.full((self.M + GUARD,), SENT, dtype=torch.int32).cuda() if outs else None

    def args(self, k, T, seed, seed_dev, flags):
        sd = None if seed_dev is None else torch.tensor([seed_dev], dtype=torch.int64).cuda()
        self._keep = sd
        return [_p(self.logits), self.V + PAD, self.M, self.V, k, float(T), _p(self.U), _p(self.rows), self.row_base, seed, _p(sd), flags,
                _p(self.mask), _p(self.ids), _p(self.pred), _p(self.scores), _p(self.cut), _p(self.kept)]

    def run(self, lib, k, T=1.0, seed=0, seed_dev=None, lse=False, no_noise=False):
        rc = lib.pk_logits_topk_sample(*self.args(k, T, seed, seed_dev, (1 if lse else 0) | (2 if no_noise else 0)), stream())
        torch.cuda.synchronize()
        assert rc == OK, f'pk_logits_topk_sample returned {rc}'
        return self

    def check_untouched(self, what, scores_written=True):
        """nothing outside [0, M) of cut_out / kept_out and the named pred / ids / scores positions is written"""
        named = torch.zeros(self.total, dtype=torch.bool)
        named[self.lrows] = True
        pred = self.pred.cpu()
        assert (pred[~named] == SENT).all(), f'{what}: pred written outside the named rows'
        assert ((pred[named] >= 0) & (pred[named] < self.V)).all(), f'{what}: pred not written or outside [0, V)'
        if self.cut is not None:
            VR.assert_untouched(self.cut[self.M:], f'{what}: cut_out behind M')
            assert (self.kept[self.M:].cpu() == SENT).all(), f'{what}: kept_out written behind M'
        if self.ids is not None:
            mk = self.mask.cpu().bool() if self.mask is not None else torch.ones(self.total, dtype=torch.bool)
            want = self.ids0.clone()
            w = named & mk
            want[w] = pred[w]
            assert torch.equal(self.ids.cpu(), want), f'{what}: ids != where(mask, pred, ids) on the named rows, untouched elsewhere'
        if self.scores is not None:
            sc = self.scores.cpu()
            VR.assert_untouched(sc[~named] if scores_written else sc, f'{what}: scores')

    def pred_rows(self):
        return self.pred.cpu()[self.lrows]


# ------------------------------------------------------------------------------------------------ the select, exact

@pytest.mark.parametrize('kind', R.SELECT_DATA)
@pytest.mark.parametrize('M,V', R.SELECT_SHAPES)
def test_select_is_exact(lib, M, V, kind):
    l = R.select_data(kind, M, V)
    ks = R.select_ks(V) + ([V // 2] if kind == 'zeros' else [])
    ref = R.noisy_ref(l.double(), torch.zeros(M, V, dtype=torch.float64), R.NONE, 1.0)
    more = False
    for k in ks:
        what = f'{kind} {M}x{V} k={k}'
        x = Launch(l).run(lib, k, no_noise=True)
        n = R.check_select(l, k, x.cut[:M], x.kept[:M], what)
        more |= bool((n > k).any())
        x.check_untouched(what)
        R.accept(ref, k, x.pred_rows(), what)
        assert torch.equal(x.pred_rows(), l.double().argmax(-1)), f'{what}: without noise the row maximum (its first column) is always kept and wins'
    if kind == 'dyadic' and V >= 1000:
        assert more, 'the dyadic grid must put the cut inside a run of equal values'
    if kind == 'zeros' and V >= 8:
        assert ((l == 0) & torch.signbit(l)).any() and ((l == 0) & ~torch.signbit(l)).any()


# ------------------------------------------------------------------------------------------------ sampling on given logits

SM, SV = 37, 1156
SAMPLE_CASES = {
    'parity': dict(mode=R.PARITY, T=0.45, rows=True),
    'parity/T=0': dict(mode=R.PARITY, T=0.0, rows=False),
    'parity/T=1e-12': dict(mode=R.PARITY, T=1e-12, rows=False),
    'fast': dict(mode=R.FAST, T=0.7, rows=False, seed=0x1234567890ABCDEF),
    'fast/rows': dict(mode=R.FAST, T=0.7, rows=True, seed=0x1234567890ABCDEF),
    'fast/seed_dev': dict(mode=R.FAST, T=0.7, rows=True, seed=0x1234567890ABCDEF, seed_dev=0x1111),
    'fast/seed_carry': dict(mode=R.FAST, T=0.7, rows=False, seed=0xFFFFFFFF, seed_dev=1),
    'fast/T=0': dict(mode=R.FAST, T=0.0, rows=False, seed=5),
    'fast/T=1e-12': dict(mode=R.FAST, T=1e-12, rows=True, seed=5),
    'none': dict(mode=R.NONE, T=1.0, rows=True),
}


@pytest.mark.parametrize('name', sorted(SAMPLE_CASES))
def test_sampling_on_given_logits(lib, name):
    """pred inside the accept set at E = 0 (equal to it where it is one column); rows[]: the noise is indexed by the LOGICAL row; mask / ids / scores as
    pk_vocab_reduce writes them; two calls agree bit for bit"""
    c = SAMPLE_CASES[name]
    g = VR._gen(f'filtered/sample/{name}')
    l = (torch.randn(SM, SV, generator=g) * 3).float()
    total = 2 * SM + 5
    rows = torch.randperm(total, generator=g)[:SM] if c['rows'] else None
    U = torch.rand(SM, SV, generator=g) if c['mode'] == R.PARITY else None
    if U is not None:
        U[3, 7], U[4, 9] = 1.0 - 2.0 ** -24, 0.0
    mask = torch.rand(total, generator=g) > 0.4
    ids0 = torch.randint(0, SV, (total,), generator=g)
    seed, seed_dev = c.get('seed', 0), c.get('seed_dev')
    ref = R.noisy_ref(l.double(), torch.zeros(SM, SV, dtype=torch.float64), c['mode'], c['T'], U=U, seed=seed, seed_dev=seed_dev, rows=rows)
    shares = {}
    for k in (1, 115, SV):
        what = f'{name} k={k}'
        mk = lambda: Launch(l, rows=rows, total=total if rows is not None else None, U=U, mask=mask[:total if rows is not None else SM],
                            ids0=ids0[:total if rows is not None else SM], scores=True)
        x = mk().run(lib, k, c['T'], seed, seed_dev, lse=True, no_noise=c['mode'] == R.NONE)
        R.check_select(l, k, x.cut[:SM], x.kept[:SM], what)
        x.check_untouched(what)
        pred = x.pred_rows()
        amb = R.accept(ref, k, pred, what)
        shares[k] = 1 - amb / SM
        if k == 1:
            assert torch.equal(pred, l.double().argmax(-1)), f'{what}: top-1 is the arg-max whatever the noise'
        # scores: -1e4 where the mask is off, 1 - p of the UNFILTERED softmax where it is on
        sc = x.scores.cpu()[x.lrows]
        on = x.mask.cpu().bool()[x.lrows]
        assert (sc[~on] == -1e4).all(), f'{what}: a masked-out row\'s score is not -1e4'
        want, bound = R.score_ref(ref, pred)
        VR.assert_within(sc[on], want[on], bound[on], f'{what}: scores')
        y = mk().run(lib, k, c['T'], seed, seed_dev, lse=True, no_noise=c['mode'] == R.NONE)
        assert torch.equal(x.pred, y.pred) and torch.equal(x.ids, y.ids) and torch.equal(x.kept, y.kept)
        VR.assert_same_bits(x.scores, y.scores, f'{what}: scores of two calls')
        VR.assert_same_bits(x.cut, y.cut, f'{what}: cut of two calls')
        # without bit 0 no score is written and the draw is the same
        z = Launch(l, rows=rows, total=total if rows is not None else None, U=U).run(lib, k, c['T'], seed, seed_dev, no_noise=c['mode'] == R.NONE)
        assert torch.equal(z.pred, x.pred)
    if rows is not None and c['mode'] != R.NONE and c['T'] >= 0.4:
        # the same call with the noise indexed by m instead of rows[m] must be refused by the check somewhere
        wrong = R.noisy_ref(l.double(), torch.zeros(SM, SV, dtype=torch.float64), c['mode'], c['T'], U=None if U is None else U.flip(0), seed=seed,
                            seed_dev=seed_dev, rows=None)
        with pytest.raises(AssertionError):
            R.accept(wrong, 115, Launch(l, rows=rows, total=total, U=U).run(lib, 115, c['T'], seed, seed_dev).pred_rows(), 'wrong rows')
    record_parity('filtered_sample_given_logits', dict(case=name, singleton_share={str(k): v for k, v in shares.items()}))
    if c['T'] >= 0.4:
        assert min(shares.values()) >= 0.98


def test_row_base_offsets_the_logical_row(lib):
    g = VR._gen('filtered/row_base')
    l = (torch.randn(5, 132, generator=g) * 3).float()
    x = Launch(l, row_base=64, ids0=torch.zeros(69, dtype=torch.int64)).run(lib, 13, 0.7, seed=99)
    ref = R.noisy_ref(l.double(), torch.zeros(5, 132, dtype=torch.float64), R.FAST, 0.7, seed=99, rows=torch.arange(64, 69))
    R.accept(ref, 13, x.pred_rows(), 'row_base')
    x.check_untouched('row_base')


def test_fast_noise_at_k_V_is_the_plain_head_s(lib):
    """on operands whose logits are exact in f32 (gemm_reference's dyadic grid) the filtered kernel at k = V and pk_vocab_sample + pk_vocab_reduce draw
    the same noise for the same (seed, logical row, column): exactly equal pred"""
    c = VR._case('filtered/plain_twin', F32, 130, 1156, 40, VR.FAST, 0, T=0.7, rows='perm', data='grid')
    x = VR.build(c)
    t = VR.device_operands(c, x, 'cuda')
    assert lib.pk_vocab_sample(*VR.sample_args(c, x, t), stream()) == OK
    pred = torch.full((x.geo.total,), SENT, dtype=torch.int64).cuda()
    assert lib.pk_vocab_reduce(t['partials'].data_ptr(), c.M, c.V, t['rows'].data_ptr(), None, None, pred.data_ptr(), None, 0, stream()) == OK
    l = x.l64.float()
    assert torch.equal(l.double(), x.l64)
    f = Launch(l, rows=x.rows, total=x.geo.total).run(lib, c.V, c.T, c.seed)
    assert torch.equal(f.pred, pred), 'the two heads disagree on exact logits: not the same noise'
    assert (f.cut[:c.M].cpu() == -math.inf).all() and (f.kept[:c.M].cpu() == c.V).all()


# ------------------------------------------------------------------------------------------------ return codes

def test_refusals_leave_the_outputs_untouched(lib):
    l = torch.randn(6, 132)
    base = dict(k=5, T=0.7, seed=1, seed_dev=None, flags=1)
    # argument positions: 0 logits, 1 ldl, 2 M, 3 V, 4 k, 7 rows, 8 row_base, 11 flags, 14 pred, 15 scores
    changes = [('k = 0', {4: 0}), ('k > V', {4: 133}), ('V < 4', {3: 0, 4: 1}), ('V % 4', {3: 130}), ('V > 65536', {3: 65540, 1: 65540}),
               ('ldl < V', {1: 128}), ('ldl % 4', {1: 134}), ('M = 0', {2: 0}), ('M < 0', {2: -1}), ('logits NULL', {0: None}), ('pred NULL', {14: None}),
               ('scores without bit 0', {11: 0}), ('scores with only bit 1', {11: 2}), ('rows with row_base', {8: 1})]
    for what, ch in changes:
        x = Launch(l, rows=torch.arange(6), total=9, mask=torch.ones(9, dtype=torch.bool), ids0=torch.arange(9), scores=True)
        a = x.args(**base)
        for i, v in ch.items():
            a[i] = v
        assert lib.pk_logits_topk_sample(*a, stream()) == EINVAL, what
        torch.cuda.synchronize()
        assert (x.pred.cpu() == SENT).all() and torch.equal(x.ids.cpu(), x.ids0) and (x.kept.cpu() == SENT).all(), what
        VR.assert_untouched(x.scores, what)
        VR.assert_untouched(x.cut, what)
    x = Launch(l, scores=True)
    assert lib.pk_logits_topk_sample(*x.args(**base), stream()) == OK


# ------------------------------------------------------------------------------------------------ the slabbed head from operands

@pytest.mark.parametrize('slab_rows', [64, 200])
@pytest.mark.parametrize('dtype', [F32, BF16, BF16X3])
def test_the_slabbed_head_from_operands(lib, dtype, slab_rows):
    """L.vocab_sample_filtered on M = 130, V = 1156: slabs of 64, 64 and 2 rows, or one slab; pred inside the accept set with E from the GEMM rule"""
    D = 72 if dtype == BF16 else 40
    shares = {}
    for rows in (None, 'perm'):
        for noise, T in ((VR.FAST, 0.7), (VR.PARITY, 0.45)):
            c = VR._case(f'filtered/head/{TNAME[dtype]}/{rows}/{noise}', dtype, 130, 1156, D, noise, 1, T=T, rows=rows)
            x = VR.build(c)
            t = VR.device_operands(c, x, 'cuda')
            ref = VR.reference(c, x)
            total = x.geo.total
            mask = (torch.rand(total, generator=VR._gen(c.name + '/mask')) > 0.4).to(torch.uint8)
            mask_dev = mask.cuda()
            for k in (1, 115, c.V):
                what = f'{c.name} slab {slab_rows} k={k}'
                slab = torch.full((slab_rows, c.V), NAN, device='cuda')
                pred = torch.full((total,), SENT, dtype=torch.int64).cuda()
                ids = torch.arange(total).cuda()
                scores = torch.full((total,), NAN).cuda()
                L.vocab_sample_filtered(dtype, t['A'], t['W'], t['bias'], c.M, c.V, c.D, k, float(c.T), t.get('U'), t.get('rows'), c.seed, True,
                                        mask_dev, ids, pred, scores, slab)
                torch.cuda.synchronize()
                lr = VR.lrows(c, x)
                named = torch.zeros(total, dtype=torch.bool)
                named[lr] = True
                p = pred.cpu()
                assert (p[~named] == SENT).all(), f'{what}: pred written outside the named rows'
                amb = R.accept(ref, k, p[lr], what)
                shares[f'{rows}/{noise}/k{k}'] = 1 - amb / c.M
                on = mask.bool()
                want_ids = torch.arange(total)
                want_ids[named & on] = p[named & on]
                assert torch.equal(ids.cpu(), want_ids), f'{what}: ids'
                sc = scores.cpu()
                VR.assert_untouched(sc[~named], f'{what}: scores outside the named rows')
                assert (sc[named & ~on] == -1e4).all()
                want, bound = R.score_ref(ref, p[lr])
                VR.assert_within(sc[lr][on[lr]], want[on[lr]], bound[on[lr]], f'{what}: scores')
    record_parity('filtered_head_from_operands', dict(dtype=TNAME[dtype], slab_rows=slab_rows, singleton_share=shares))
    assert min(shares.values()) >= 0.98


# ------------------------------------------------------------------------------------------------ Phenaki.sample end to end

K25 = R.k_of(0.9, TINY['maskgit']['num_tokens'])
GRID = (3, 4, 4)


def _product(with_critic, dtype='fp32'):
    _, _, _, ph = load_product('tiny', TINY, with_critic=with_critic, dtype=dtype)
    ctx = weights.synthetic_context(2, 6, TINY['maskgit']['dim_context'], seed=2)
    ph.encode_texts = lambda texts, output_device=None: ctx[:len(texts)].cuda()
    return ph, ctx


def _audit(trace, ctx, base, k, what, rows_of=lambda t: t['mask'].reshape(-1)):
    """every recorded step: the oracle's logits for the recorded masked ids through the restatement; returns (ambiguous pairs, checked pairs)"""
    _, mg_sd, _ = state_dicts('tiny')
    _, mgc, _ = oracle_cfgs(TINY)
    steps, amb, tot = TINY['steps'], 0, 0
    assert len(trace) == steps
    for s, t in enumerate(trace):
        ids = t['masked_ids'].cpu()
        c = ctx[:ids.shape[0]]
        logits = O.maskgit_cfg(mg_sd, mgc, ids, cond_scale=5., video_patch_shape=GRID, context=c, text_mask=(c != 0).any(-1))
        T = 0.9 * ((steps - (s + 1)) / steps)
        U = weights.uniform_noise(tuple(logits.shape), base + 2 * s)
        ref = R.e2e_ref(logits, T, U, k)
        rows = rows_of(t).cpu()
        amb += R.accept(ref, k, t['pred'].reshape(-1), f'{what} step {s}', rows=rows)
        tot += int(rows.sum())
        m = t['mask'].cpu()
        assert torch.equal(t['ids'].cpu()[m], t['pred'].cpu()[m]) and torch.equal(t['ids'].cpu()[~m], ids[~m]), f'{what} step {s}: ids != where(mask, pred, ids)'
    return amb, tot


@pytest.mark.parametrize('base', R.E2E_SEEDS)
@pytest.mark.parametrize('with_critic', [True, False])
@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
def test_sample_with_a_filter_draws_inside_the_top_k(dtype, with_critic, base):
    ph, ctx = _product(with_critic, dtype)
    trace = []
    vid, ids = ph.sample(texts=['a', 'b'], num_frames=5, cond_scale=5., filter_thres=0.9, _noise_fn=noise_fn_cuda(base), _trace=trace, _return_ids=True)
    assert vid.shape == (2, 3, 5, 64, 64) and torch.isfinite(vid).all() and ((ids >= 0) & (ids < 256)).all()
    with O.precision(dtype):
        amb, tot = _audit(trace, ctx, base, K25, f'{dtype} critic={with_critic} base={base}')
    record_parity('filtered_sample_tiny_vs_oracle', dict(dtype=dtype, with_critic=with_critic, base=base, audited_near_ties=amb, checked=tot))
    assert amb <= R.E2E_AMBIGUOUS_CAP * tot, f'{amb} of {tot} (step, position) pairs had more than one acceptable column'
    trace2 = []
    _, ids2 = ph.sample(texts=['a', 'b'], num_frames=5, cond_scale=5., top_k=K25, _noise_fn=noise_fn_cuda(base), _trace=trace2, _return_ids=True)
    assert torch.equal(ids, ids2), 'top_k = 25 and filter_thres = 0.9 resolve to the same k'


def test_top_1_is_the_arg_max_of_every_step():
    ph, ctx = _product(False)
    trace = []
    ph.sample(texts=['a', 'b'], num_frames=5, cond_scale=5., top_k=1, _noise_fn=noise_fn_cuda(R.E2E_SEEDS[0]), _trace=trace)
    amb, tot = _audit(trace, ctx, R.E2E_SEEDS[0], 1, 'top_k = 1')
    assert amb <= R.E2E_AMBIGUOUS_CAP * tot
    _, mg_sd, _ = state_dicts('tiny')
    _, mgc, _ = oracle_cfgs(TINY)
    same = n = 0
    for t in trace:
        logits = O.maskgit_cfg(mg_sd, mgc, t['masked_ids'].cpu(), cond_scale=5., video_patch_shape=GRID, context=ctx, text_mask=(ctx != 0).any(-1))
        m = t['mask'].cpu()
        same += int((logits.argmax(-1)[m] == t['pred'].cpu()[m]).sum())
        n += int(m.sum())
    assert same >= (1 - R.E2E_AMBIGUOUS_CAP) * n


def test_graph_replay_and_eager_agree_and_another_k_captures_another_graph():
    ph, _ = _product(True)
    kw = dict(texts=['a', 'b'], num_frames=5, cond_scale=5., _return_ids=True, _seed=0x1234567812345678 & 0x3FFFFFFFFFFFFFFF)
    v_e, ids_e = ph.sample(filter_thres=0.9, **kw)
    _, ids_plain = ph.sample(**kw)
    ph.enable_sample_graph(True)
    try:
        for _ in range(2):                                                        # capture, then a pure replay
            v_g, ids_g = ph.sample(filter_thres=0.9, **kw)
            assert torch.equal(ids_g, ids_e) and torch.equal(v_g, v_e)
        assert len(ph.__dict__['_pk_sample_graphs']) == 1
        _, ids_3 = ph.sample(top_k=3, **kw)
        assert len(ph.__dict__['_pk_sample_graphs']) == 2
        assert torch.equal(ph.sample(top_k=K25, **kw)[1], ids_e) and len(ph.__dict__['_pk_sample_graphs']) == 2
        assert torch.equal(ph.sample(**kw)[1], ids_plain) and len(ph.__dict__['_pk_sample_graphs']) == 3
    finally:
        ph.enable_sample_graph(False)
    assert torch.equal(ph.sample(top_k=3, **kw)[1], ids_3)


def test_infill_and_make_video_take_the_filter():
    ph, _ = _product(True)
    torch.manual_seed(3)
    video = torch.rand(2, 3, 5, 64, 64).cuda()
    edit = torch.zeros(2, *GRID, dtype=torch.bool)
    edit[:, 1:] = True                                                            # keep token frame 0
    tokens = ph.cvivit(video, return_only_codebook_ids=True).reshape(2, -1)
    out, ids = ph.infill(video, edit, texts=['a', 'b'], mask_level='token', top_k=K25, _return_ids=True, _seed=11)
    keep = ~edit.reshape(2, -1).cuda()
    assert out.shape == video.shape and torch.equal(ids[keep], tokens[keep]) and ((ids >= 0) & (ids < 256)).all()
    whole, scenes = make_video(ph, texts=['a', 'b'], num_frames=(5, 4), prime_lengths=1, filter_thres=0.9)
    assert whole.shape == (1, 3, 9, 64, 64) and len(scenes) == 2 and torch.isfinite(whole).all()
    img = ph.sample_images(texts=['a', 'b'], cond_scale=5., top_k=3)
    assert img.shape == (2, 3, 64, 64)
