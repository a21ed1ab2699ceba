"""What tests/gemm_reference.py promises, shown on the CPU with no kernel launched: the cases reach exactly the branches written out from the switch tables of
gemm_ex / pk_gemm / pk_gemm_splitk, every legal pair of vector-epilogue options meets in some case, the grid data set is exact in f32 in any order, the float64
reference passes its own checker under both poisons, an honest f32 emulation (torch product in natural and in permuted k order, the epilogue in f32) passes on
every case, each planted defect of the emulation is rejected on every case it applies to, and every refusal of gemm_ex that comes before the epilogue form is
reported returns its error (pk_gemm_ex_form on CPU tensors: nothing is launched, no operand is read)."""
import itertools

import pytest
import torch

from tests import gemm_reference as R

torch.set_grad_enabled(False)
CASES = R.all_cases()
GROUPS = R.grouped_cases()


@pytest.fixture(scope='module')
def L():
    from phenaki_pytorch_amd import _lib, build
    build.build(verbose=False)
    _lib.load()
    saved_forms, saved_pol = _lib.get_gemm_hot_forms(), _lib.get_cache_policy()
    _lib.set_gemm_hot_forms(1)
    _lib.set_cache_policy(0)
    yield _lib
    _lib.set_gemm_hot_forms(saved_forms)
    _lib.set_cache_policy(saved_pol)


def test_names_branches_and_mutants():
    names = [c.name for c in CASES]
    assert len(set(names)) == len(names)
    reached, want = {R.branch_of(c) for c in CASES}, R.expected_branches()
    assert reached == want, (sorted(reached - want), sorted(want - reached))
    for m in R.MUTANTS:
        assert any(R.applies(m, c) for c in CASES), f'no case for the mutant {m}'
    for dt, v, a in R.main_loops():                        # the bound is sharpest at small K: a random case at K <= 96 on every main loop
        tag = R.loop_id(dt, v, a)
        assert any(c.data == 'rand' and c.K <= 96 for c in CASES if c.name.startswith(tag + '_')), tag
    for c in CASES:                                        # the conditions the condition cases exist for
        lp = R.lp_of(c)
        MT, nt = -(-c.M // lp.BM), -(-c.K // lp.BK)
        if c.name.endswith('_mt9'):
            assert MT == 9 and (MT + 7) // 8 == 2
        if c.name.endswith('_panel'):
            esz = 2 if c.dtype == R.BF16 else 4
            panel, cmax = max(4, (1 << 20) // (lp.BM * c.K * esz)), (MT + 7) // 8
            assert 0 < panel < cmax and cmax % panel != 0, (c.name, panel, cmax)
        if c.name.endswith('_krot'):
            assert c.N >= 8192 and nt > 1 and c.K % lp.BK != 0
        assert 2.0 * c.M * c.N * c.K < 2.5e9, c.name


def test_every_legal_pair_of_vector_epilogue_options_meets():
    covered = set()
    for c in CASES:
        if c.entry == 'ex' and R.vec_ok(c):
            o = R.options(c)
            assert R.legal(o), (c.name, sorted(o))
            covered |= {frozenset(p) for p in itertools.combinations(sorted(o), 2)}
    legal = [p for p in itertools.combinations(R.OPTION_ATOMS, 2) if R.legal(set(p))]
    assert len(legal) > 30
    missing = [p for p in legal if frozenset(p) not in covered]
    assert not missing, missing
    # the combinations the suite never launched before
    for need in ({'bias', 'stats'}, {'leaky', 'C2'}, {'relu', 'dup'}, {'leaky', 'scatter'}, {'ln1', 'bias'}, {'ln2', 'leaky'}, {'ln1', 'res'}, {'ln2', 'res'},
                 {'relu', 'out_bf16'}, {'out_bf16'}):
        assert any(need <= R.options(c) for c in CASES if R.vec_ok(c)), need
    scalar = [c for c in CASES if not R.vec_ok(c)]
    for act in R.ANAME:
        for res in (False, True):
            for ob in (False, True):
                if not (act == R.ACT_GEGLU and res):
                    assert any(c.act == act and c.res == res and c.out_bf16 == ob for c in scalar), (act, res, ob)
    assert {c.trig for c in scalar} == {'n', 'ldc', 'c_off', 'bias_off', 'ldr'}
    assert {c.N for c in scalar if c.trig == 'n'} == {1, 2, 3, 6}
    assert {(c.K, R.geometry(c).np_in) for c in CASES if c.ln == 2} >= {(72, 3), (96, 3), (512, 16), (544, 17)}


def test_grid_sums_are_exact_in_any_order():
    """at K = 96 and K = 2048 an f32 product of the grid operands, in natural and in permuted k order, equals the float64 product bit for bit"""
    for K, data, dt in ((96, 'grid', R.BF16), (2048, 'grid', R.BF16), (96, 'gridA', R.BF16X3), (1024, 'gridW', R.BF16X3)):
        c = R._case(f'exactness_{data}_{K}', dt, 8, 70, 68, K, data=data, bias=True, res=True)
        x = R.build(c)
        want = x.A.double() @ x.W.double().t()
        span = torch.log2(want.abs().max() / x.step).item()
        assert 10 < span < 24, span
        for seed in range(3):
            p = torch.randperm(K, generator=torch.Generator().manual_seed(seed)) if seed else torch.arange(K)
            got = x.A[:, p] @ x.W[:, p].t()
            assert torch.equal(got.double(), want), (K, data, seed)
            chunks = sum((x.A[:, p[i:i + 32]] @ x.W[:, p[i:i + 32]].t()) for i in range(0, K, 32))
            assert torch.equal(chunks.double(), want)
        if dt == R.BF16X3:
            lo = x.A - R.bf(x.A) if data == 'gridA' else x.W - R.bf(x.W)
            assert (lo != 0).float().mean() > 0.2, 'the low plane of the split operand is exercised'
            assert torch.equal(R.bf(lo), lo), 'hi + lo holds the operand exactly'


def test_erff_allowance():
    """the f32-mode GEGLU allowance: the CPU's erff against a float64 erf, in units of 2^-24 (erf is at most 1), recorded as ERFF_CPU_RATIO"""
    xs = torch.linspace(-6, 6, 2_000_001, dtype=torch.float64).float()
    worst = ((torch.erf(xs).double() - torch.erf(xs.double())).abs() / R.U24).max().item()
    print(f'erff: f32 CPU evaluation err = {worst:.3f} x 2^-24')
    assert 0.25 * R.ERFF_CPU_RATIO <= worst <= R.ERFF_CPU_RATIO and R.ERFF_C == 4 * R.ERFF_CPU_RATIO


def _same_logical(a, b, c):
    for k in ('A', 'W'):
        assert torch.equal(getattr(a, k), getattr(b, k))
    assert torch.isnan(a.A_buf[:, c.K:]).all() and torch.isinf(b.A_buf[:, c.K:]).all()
    assert torch.isnan(a.W_buf[c.N:]).all() and torch.isinf(b.W_buf[c.N:]).all()
    g = a.geo
    if not c.w_tight:
        assert (a.W_buf[:c.N, c.K:g.kpad] == 0).all() and torch.isnan(a.W_buf[:c.N, g.kpad:]).all() and g.ldw > g.kpad
    if c.gather:
        used = torch.zeros(g.rowsA, dtype=torch.bool)
        used[a.a_rows.long()] = True
        assert torch.isnan(a.A_buf[~used]).all() and (~used).sum() >= 9 and a.a_rows.unique().numel() < max(c.M, 2)
    else:
        assert torch.isnan(a.A_buf[c.M:]).all() and g.rowsA > c.M
    assert torch.isnan(a.res_buf[c.M:]).all() and torch.isnan(a.res_buf[:, c.N:]).all() and torch.isnan(a.bias_buf[g.boff + c.N:]).all()
    if c.ln:
        assert torch.isnan(a.s_buf[c.N:]).all() and torch.isnan(a.t_buf[c.N:]).all() and torch.isnan(a.stats_in[c.M:]).all()


@pytest.mark.parametrize('group', sorted(GROUPS))
def test_reference_emulation_and_mutants(group):
    for c in GROUPS[group]:
        x = R.build(c)
        xi = R.build(c, R.INF)
        _same_logical(x, xi, c)
        ref = R.reference(c, x)
        assert (ref.terms is None) == R.exact(c) and torch.isfinite(ref.out).all()
        if ref.terms is not None:
            assert all(torch.isfinite(t).all() and (t >= 0).all() for t in ref.terms.values())
        got = R.check(c, x, ref, R.ideal_outputs(c, x, ref), f'{c.name} / reference')
        assert got['C'][0] < 1
        for xx, order in ((x, 'natural'), (xi, 'permuted')):
            R.check(c, xx, ref, R.emulate(c, xx, order), f'{c.name} / emulation ({order})')
        for m in R.MUTANTS:
            if R.applies(m, c):
                with pytest.raises(AssertionError):
                    R.check(c, x, ref, R.emulate(c, x, 'natural', m), f'{c.name} / {m}')


def test_checker_rejects_sentinel_damage_and_non_finite_values():
    c = next(c for c in CASES if c.name == 'bf16_v8_vec_leaky+bias+res+C2+stats')
    x = R.build(c)
    ref = R.reference(c, x)
    good = R.ideal_outputs(c, x, ref)
    R.check(c, x, ref, good)
    g = x.geo
    for name, r, col in (('C', 0, 0), ('C', R.G - 1, 3), ('C', R.G + c.M, 0), ('C', R.G, g.NC), ('C', R.G + 5, g.ldc - 1), ('C2', R.G + 1, c.N), ('C2', 1, 1),
                         ('stats', 0, 0), ('stats', R.G + c.M, 1)):
        for value in (0.0, 1.0, R.NAN):
            bad = {k: v.clone() for k, v in good.items()}
            bad[name][r, col] = value
            with pytest.raises(AssertionError, match='outside the result region'):
                R.check(c, x, ref, bad)
    for name in ('C', 'C2', 'stats'):
        for value in (R.NAN, R.INF):
            bad = {k: v.clone() for k, v in good.items()}
            bad[name][R.G + 2, 1] = value
            with pytest.raises(AssertionError, match='non-finite'):
                R.check(c, x, ref, bad)
    bad = {k: v.clone() for k, v in good.items()}
    bad['C2'][R.G + 2, 1] = bad['C2'][R.G + 2, 1] * 1.01
    with pytest.raises(AssertionError, match='C2 is not'):
        R.check(c, x, ref, bad)


def _form(L, c, change=None):
    x = R.build(c)
    t = R.operands(c, x)
    a = R.ex_args(c, x, t)
    if change:
        change(a, t)
    return L.load().pk_gemm_ex_form(*a.values())


def test_every_ex_case_is_accepted_with_its_form(L):
    """every pk_gemm_ex / pk_gemm case obeys the entry point's contract (the host checks accept it) and gets the epilogue form its branch names; pk_gemm's
    automatic choice is the variant the case declares"""
    lib = L.load()
    for c in CASES:
        if c.entry == 'splitk':
            continue
        x = R.build(c) if 2.0 * c.M * c.N * c.K < 2e8 else None
        if x is not None:
            rc = lib.pk_gemm_ex_form(*R.ex_args(c, x, R.operands(c, x)).values())
            assert rc == R.form_of(c), (c.name, rc)
        if c.entry == 'gemm':
            g = R.geometry(c)
            if c.gather:
                assert c.variant == (2 if ((c.M + 127) // 128) * ((c.N + 127) // 128) >= 384 else 1)
            else:
                assert lib.pk_gemm_auto_variant(c.dtype, int(c.a_f32), c.M, c.N, c.K, g.lda, g.ldw, c.M) == c.variant, c.name


@pytest.mark.parametrize('label,err,base,change', R.FORM_REFUSALS, ids=[r[0] for r in R.FORM_REFUSALS])
def test_refusals(L, label, err, base, change):
    c = R._base(base)
    assert _form(L, c) == R.form_of(c), 'the unchanged call is accepted'
    assert _form(L, c, change) == err


def test_refusal_list_covers_the_returns_of_gemm_ex():
    """one refusal case per `return PK_E*` condition of gemm_ex and pk_gemm_splitk (counted in the source)"""
    import os
    src = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'phenaki_pytorch_amd', 'csrc', 'gemm.hip')).read()
    body = src[src.index('static int gemm_ex('):src.index('extern "C" int pk_gemm_ex(')]
    returns = body.count('return PK_EINVAL') + body.count('return PK_EALIGN')
    assert returns == 25, f'gemm_ex now has {returns} refusing returns: add the new one to FORM_REFUSALS / LATE_REFUSALS'
    assert len(R.FORM_REFUSALS) + len(R.LATE_REFUSALS) >= 2 * returns
    sk = src[src.index('extern "C" int pk_gemm_splitk('):]
    assert sk.count('return PK_EINVAL') + sk.count('return PK_EALIGN') == 5 and len(R.SPLITK_REFUSALS) >= 20
