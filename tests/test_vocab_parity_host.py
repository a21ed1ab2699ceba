"""tests/vocab_reference.py on the CPU: the restatement equals F.cross_entropy, softmax and tests/util.gumbel_noisy; the checkers accept an f32 emulation
of the head in two summation orders and reject every wrong kernel of a written-out list (a checker that cannot fail is itself a failure); the host mirror of
the resident kernel's work split covers every (row tile, vocabulary tile) pair exactly once; the case list reaches every path of that split and all eight
resident instantiations; and the index check is an equality on at least 98 % of the (tile, row) pairs of every random case."""
import itertools
import math

import pytest
import torch
import torch.nn.functional as F

from tests import vocab_reference as R
from tests.util import gumbel_noisy

torch.set_grad_enabled(False)
TILED, RESIDENT = R.tiled_groups(), R.resident_groups()
BY_NAME = {c.name: c for c in R.all_cases()}
HOST_ONLY = [R._case('host/bf16/300x1000x96/parity+lse', R.BF16, 300, 1000, 96, R.PARITY, 1, T=1.0)]
SMALL = [c for k, g in TILED.items() if k not in ('panel/bf16', 'panel/f32', 'counter64') for c in g] + HOST_ONLY


def _rejected(fn, *a, **kw):
    try:
        fn(*a, **kw)
    except AssertionError:
        return True
    return False


def test_transcendental_allowances():
    """the CPU's f32 log, log2 and exp against float64 in units of 2^-24 of the result stay under the vector library's guarantee of 1 ulp, which is the
    figure on record (*_CPU_RATIO: the measurement itself depends on the host's instruction set); the device library gets 4 times that"""
    g = torch.Generator().manual_seed(0)
    u = torch.randint(1, 2 ** 24, (4_000_000,), generator=g).double() / 2 ** 24
    xs = torch.cat([u, torch.exp(torch.rand(2_000_000, generator=g, dtype=torch.float64) * 30 - 25), 1 - torch.arange(1, 4096).double() / 2 ** 24])
    es = torch.rand(4_000_000, generator=g, dtype=torch.float64) * 107 - 87

    def worst(fn, x):
        x = x.float()
        got, ref = fn(x).double(), fn(x.double())
        ok = torch.isfinite(ref) & (ref != 0)
        return ((got - ref).abs()[ok] / (ref[ok].abs() * R.U24)).max().item()
    for name, fn, x, rec, c in (('log', torch.log, xs, R.LOG_CPU_RATIO, R.LOG_C), ('log2', torch.log2, xs, R.LOG2_CPU_RATIO, R.LOG2_C),
                                ('exp', torch.exp, es, R.EXP_CPU_RATIO, R.EXP_C)):
        w = worst(fn, x)
        print(f'{name}: f32 CPU evaluation err = {w:.3f} x 2^-24 of the result')
        assert w <= rec == 2.0 and c == 4 * rec


def test_restatement_equals_torch():
    for name in ('tiled/f32/257x1156x40/parity+lse', 'tiled/bf16/130x132x96/parity+lse', 'tiled/x3/130x132x96/none+lse'):
        c = BY_NAME[name]
        x = R.build(c)
        ref = R.reference(c, x)
        nt = R.ntiles_of(c.V)
        if c.noise == R.PARITY:
            want = gumbel_noisy(x.l64, c.T, x.U.double())
            inner = x.U < 0.999                                                      # at 1 - 2^-24 the f32 rounding of u + 1e-10 is the kernel's, not torch.double's
            assert torch.allclose(ref.noisy[inner], want[inner], rtol=1e-9, atol=1e-5)
        l = R._tiles(x.l64, c.V, -math.inf)
        pmax = l.max(-1).values
        psum = torch.exp(l - pmax[..., None]).sum(-1)
        g = torch.Generator().manual_seed(3)
        x.targets = torch.randint(0, c.V, (x.geo.total,), generator=g)
        ce = R.ce_ref(c, x, pmax.t(), psum.t())
        assert torch.allclose(ce.lse, torch.logsumexp(x.l64, -1), rtol=1e-12, atol=1e-12)
        assert torch.allclose(ce.loss, F.cross_entropy(x.l64, x.targets[R.lrows(c, x)], reduction='none'), rtol=1e-10, atol=1e-10)
        n = R._tiles(ref.noisy, c.V, -math.inf)
        loc = n.argmax(-1)
        rc = R.NS(nt=nt, M=c.M, V=c.V, has_rows=x.rows is not None, has_mask=False, has_ids=True, has_scores=True, lse=True, total=x.geo.total, rows=x.rows,
                  mask=None, ids0=torch.zeros(x.geo.total, dtype=torch.int64), val=n.gather(-1, loc[..., None])[..., 0].t(),
                  idx=(loc + torch.arange(nt) * 128).t().to(torch.int32), logit=l.gather(-1, loc[..., None])[..., 0].t(), pmax=pmax.t(), psum=psum.t())
        red = R.reduce_ref(rc)
        r = R.lrows(c, x)
        pred = ref.noisy.argmax(-1)
        assert torch.equal(red.pred[r], pred) and torch.equal(red.ids[r], pred)
        assert torch.allclose(red.scores[r], 1 - x.l64.softmax(-1).gather(1, pred[:, None])[:, 0], rtol=1e-10, atol=1e-12)


@pytest.mark.parametrize('c', SMALL, ids=[c.name for c in SMALL])
def test_checkers_accept_f32_in_two_orders(c):
    x = R.build(c)
    ref = R.reference(c, x)
    worst = {}
    for order in (0, 1):
        for k, v in R.check_partials(c, ref, R.emulate(c, x, order)).items():
            worst[k] = max(worst.get(k, 0.), v)
    assert all(v <= 1 for v in worst.values())
    print(c.name, {k: round(v, 4) for k, v in worst.items()})


# mutant -> the cases that must reject it
MUTANT_CASES = {
    'tile_local_index': ['tiled/f32/257x1156x40/parity+lse', 'tiled/bf16/130x132x96/none'],
    'last_max_wins': ['tiled/grid/f32/257x1156', 'tiled/grid/bf16/130x132', 'tiled/grid/x3/257x1156'],
    'noise_by_m': ['tiled/f32/257x1156x40/parity', 'tiled/bf16/257x1156x72/fast+lse'],
    'noise_index_32bit': ['tiled/counter64'],
    'gumbel_no_eps': ['tiled/f32/130x132x96/parity', 'tiled/x3/257x1156x40/parity+lse'],
    'temperature_multiplied': ['tiled/f32/130x132x96/parity+lse', 'tiled/bf16/130x132x72/fast'],
    'unclamped_T': ['tiled/clamp/parity/T=0', 'tiled/clamp/fast/T=0', 'tiled/clamp/parity/T=1e-12', 'tiled/clamp/fast/T=1e-12'],
    'padding_in_sum': ['tiled/f32/130x132x96/none+lse', 'tiled/bf16/257x1156x72/parity+lse'],
    'max_without_bias': ['tiled/f32/130x132x96/fast+lse', 'tiled/x3/257x1156x40/none+lse'],
    'sum_other_max': ['tiled/f32/130x132x96/parity+lse', 'tiled/bf16/257x1156x72/none+lse'],
}


def test_mutant_list_is_the_written_one():
    assert set(MUTANT_CASES) == set(R.SAMPLE_MUTANTS)
    assert set(R.REDUCE_MUTANTS) == {'skip_tiles_ge_64', 'score_p', 'masked_score', 'ids_where_unmasked', 'pred_not_scattered', 'last_max_wins'}
    assert set(R.CE_MUTANTS) == {'target_at_m', 'hi_plane_only'}


@pytest.mark.parametrize('mutant', sorted(MUTANT_CASES))
def test_checkers_reject_wrong_sampling_kernels(mutant):
    for name in MUTANT_CASES[mutant]:
        c = BY_NAME[name]
        x = R.build(c)
        ref = R.reference(c, x)
        R.check_partials(c, ref, R.emulate(c, x))                                    # the same emulation without the error passes
        assert _rejected(R.check_partials, c, ref, R.emulate(c, x, mutant=mutant)), f'{mutant} passes on {name}'


def _fake_reduce(c, ref):
    """what a correct f32 reduce would leave, from the reference itself"""
    sc = torch.full((c.total,), R.NAN) if ref.scores is None else ref.scores.float()
    return ref.pred.clone(), ref.ids.clone(), sc


def test_reduce_checker_accepts_and_rejects():
    cases = R.reduce_cases()
    hit = {m: 0 for m in R.REDUCE_MUTANTS}
    for c in cases:
        ref = R.reduce_ref(c)
        R.check_reduce(c, ref, *_fake_reduce(c, ref))
        for order in (0, 1):                                                         # an f32 fold in the kernel's order and in another
            R.check_reduce(c, ref, *R.reduce_f32(c, order))
        for m in R.REDUCE_MUTANTS:
            r = c.rows.long() if c.rows is not None else torch.arange(c.M)
            out = bool((c.mask[r] == 0).any()) if c.has_mask else False               # a named row that is masked out
            applies = dict(skip_tiles_ge_64=c.nt > 64, score_p=c.has_scores and c.lse, masked_score=c.has_scores and c.lse and out,
                           ids_where_unmasked=c.has_ids and out, pred_not_scattered=c.has_rows and not torch.equal(r, torch.arange(c.M)),
                           last_max_wins=bool(((c.val == c.val.max(0).values).sum(0) > 1).any()))[m]
            if applies:
                assert _rejected(R.check_reduce, c, ref, *_fake_reduce(c, R.reduce_ref(c, mutant=m))), f'{m} passes on {c.name}'
                hit[m] += 1
    assert all(hit.values()), hit
    for opt in ('has_rows', 'has_mask', 'has_ids', 'has_scores', 'lse'):               # every option on and off at every tile count
        for nt in R.REDUCE_NT:
            assert {getattr(c, opt) for c in cases if c.nt == nt} == {True, False}, (opt, nt)
    assert {(c.nt, c.M) for c in cases} >= {(nt, M) for nt in R.REDUCE_NT for M in R.REDUCE_M}


def test_ce_checker_accepts_and_rejects():
    for dt, nt, D in ((R.F32, 65, 40), (R.BF16, 130, 72), (R.BF16X3, 63, 512), (R.BF16X3, 1, 40)):
        c, x = R.ce_case(dt, nt, D)
        ref = R.ce_ref(c, x)
        R.assert_within(ref.loss.float(), ref.loss, ref.dloss, 'loss')
        for order in (0, 1):
            lse32, loss32 = R.ce_f32(c, x, order)
            R.assert_within(lse32, ref.lse, ref.dlse, f'{c.name}: f32 lse, order {order}')
            R.assert_within(loss32, ref.loss, ref.dloss, f'{c.name}: f32 loss, order {order}')
        for m in R.CE_MUTANTS:
            if m == 'hi_plane_only' and dt != R.BF16X3:
                continue
            wrong = R.ce_ref(c, x, mutant=m)
            assert _rejected(R.assert_within, wrong.loss.float(), ref.loss, ref.dloss, 'loss'), f'{m} passes on {c.name}'
        if nt > 1:                                                                   # a fold that loses the last tile
            short = R.ce_ref(c, x, pmax=x.pmax[:-1], psum=x.psum[:-1])
            assert _rejected(R.assert_within, short.lse.float(), ref.lse, ref.dlse, 'lse'), f'a dropped tile passes on {c.name}'


def test_resident_plan_covers_every_pair_once():
    for MT in range(1, 41):
        for nt in range(1, 141):
            want = {(r, t) for r in range(MT) for t in range(nt)}
            for NW in (8, 12):
                for nworkers in (1, 2, 3, 32):
                    plan, _ = R.resident_plan(128 * MT, 128 * nt, nworkers, NW)
                    assert sum(map(len, plan.values())) == MT * nt and set(itertools.chain.from_iterable(plan.values())) == want, (NW, nworkers, MT, nt)


def test_case_list_reaches_every_path_and_build():
    paths, builds = set(), set()
    for g in RESIDENT.values():
        for c in g:
            assert R.is_resident(c), c.name
            nw = R.resident_build(c)[0]
            paths |= R.resident_plan(c.M, c.V, c.workers or 32, nw)[1]
            builds.add(R.resident_build(c))
    for c in R.philox_cases():
        assert R.is_resident(c) == (c.mode != 0)
    assert paths == {'sweep', 'left_a>0', 'left_b<CT', 'second_tile', 'first_tile_later', 'wave_no_tile', 'worker_nseg0', 'xcd_CT<=0', 'short_last_tile'}
    assert paths == set(R.PATHS)
    assert builds == {(nw, par, lse) for nw in (8, 12) for par in (False, True) for lse in (False, True)}
    assert all(not R.is_resident(c) for g in TILED.values() for c in g) and not R.is_resident(R.below_rule_case())
    # what the named shapes are there for
    p = lambda M, V, w, nw: R.resident_plan(M, V, w, nw)[1]
    assert {'worker_nseg0', 'xcd_CT<=0', 'wave_no_tile', 'short_last_tile'} <= p(1030, 1028, 32, 8)
    assert {'sweep', 'left_a>0', 'left_b<CT'} <= p(1300, 1028, 3, 12)
    assert {'second_tile', 'sweep'} <= p(1030, 13316, 2, 12) and 'first_tile_later' in p(1030, 13316, 32, 8)


def test_tie_groups_sit_where_they_say():
    (a, b), (c_, d), (e, f), tiles, both = R.TIE_GROUPS
    assert a // 4 != b // 4 and a // 16 == b // 16                                   # lane groups of one fragment
    assert c_ // 16 != d // 16 and c_ // 32 == d // 32                               # column fragments of one wave (tiled), sub-blocks (resident)
    assert e // 32 != f // 32 and e // 128 == f // 128                               # waves of one tile
    assert len({v // 128 for v in tiles}) == 3 and (tiles[1] // 128 - tiles[0] // 128) % 8 != 0 and (tiles[2] // 128 - tiles[0] // 128) % 8 == 0
    assert both[0] // 128 == both[1] // 128 != both[2] // 128
    for name in ('tiled/grid/f32/257x1156', 'res/m1/grid/1030x1028'):
        c = BY_NAME[name]
        x = R.build(c)
        assert (x.E == 0).all()
        top = x.l64.max(-1, keepdim=True).values
        ties = (x.l64 == top).sum(-1)
        assert (ties >= 2).all()                                                     # every row's maximum is shared
        win = (x.l64 == top).int().argmax(-1)
        assert len({int(v) for v in win}) >= 3                                       # and more than one group wins somewhere


RANDOM = [c for c in R.all_cases() if c.data == 'rand' and c.noise != R.PHILOX] + HOST_ONLY


@pytest.mark.parametrize('c', RANDOM, ids=[c.name for c in RANDOM])
def test_index_check_is_an_equality_nearly_everywhere(c):
    """a condition, not a measurement: from the reference and the bounds alone"""
    x = R.build(c)
    share = R.singleton_share(c, R.reference(c, x))
    print(f'{c.name}: singleton share {share:.4%}')
    assert share >= 0.98
