"""What tests/attn_fwd_reference.py promises, shown on the CPU: every case has the planted-mass property, the float64 reference passes its own checker with
the pads poisoned (NaN and +Inf give the same reference), each mutant of the reference is rejected on every case it applies to, and the checker rejects a
NaN anywhere and a write into the slack columns of the output rows.  The cases are the ones tests/test_attn_fwd_gpu.py launches (the CU-dependent ones
for a nominal CU count)."""
import pytest
import torch

from tests import attn_fwd_reference as R

CASES = R.FIXED_CASES + R.cu_cases(R.NOMINAL_CUS)
SMALL = R.small_cases()
SLACK = 8


@pytest.fixture(scope='module')
def built():
    cache = {}

    def get(c):
        if c.name not in cache:
            if c.branch == 'small':
                x = R.build_small(c)
                ref = R.reference_small(c, x)
                bnd, lse_bnd, _ = R.bound(c, x, ref, ref.Q, ref.K, small=True)
            else:
                x = R.build(c)
                ref = R.reference(c, x)
                bnd, lse_bnd, _ = R.bound(c, x, ref)
            cache.clear()                                  # the 128-row cases are large: keep one
            cache[c.name] = (x, ref, bnd, lse_bnd)
        return cache[c.name]
    return get


def as_output(c, O):
    """what a kernel with exactly the reference's values would leave: rounded to the output type, in a NaN-filled buffer with slack columns"""
    buf = torch.full((O.shape[0], O.shape[1] + SLACK), float('nan'), dtype=torch.float32 if c.out_f32 else torch.bfloat16)
    buf[:, :O.shape[1]] = O.to(buf.dtype)
    return buf


def mutant_ref(c, x, m):
    return R.reference_small(c, x, m) if c.branch == 'small' else R.reference(c, x, m)


def test_case_names_are_unique_and_branches_hold():
    names = [c.name for c in CASES + SMALL]
    assert len(set(names)) == len(names)
    for c in CASES:
        assert R.branch_of(c, R.NOMINAL_CUS) == c.branch, c.name
    reached = {c.branch for c in CASES}
    # every instantiation attn_fwd_impl launches without a dropout site, a tuning variable or another head width
    want = {f'lds<1,{pf},0,0,bf16>' for pf in (0, 1)} | {f'lds<{qf},0,{tab},1,bf16>' for qf in (1, 2) for tab in (0, 1)} | {'lds<1,0,1,0,bf16>'}
    want |= {'lds<2,0,0,1,x3>', 'lds<2,0,1,1,x3>', 'lds<2,0,0,0,x3>', 'lds<3,0,0,0,x3>'} | {f'free<{t},{qf}>' for t in ('f32', 'bf16', 'x3') for qf in (1, 2)}
    assert reached == want, (sorted(reached - want), sorted(want - reached))
    for m in R.MUTANTS:
        assert any(R.applies(m, c) for c in CASES), f'no case for the mutant {m}'


@pytest.mark.parametrize('c', CASES + SMALL, ids=lambda c: c.name)
def test_planted_reference_and_mutants(built, c):
    x, ref, bnd, lse_bnd = built(c)
    R.planted_property(c, x, ref)
    assert torch.isfinite(ref.O).all() and torch.isfinite(ref.lse).all() and (bnd > 0).all()
    worst = R.check(c.name, as_output(c, ref.O), ref.O, bnd, c.h * 64)
    assert worst < 1, 'the output rounding alone: half an output ulp'
    assert R.check_lse(c.name, ref.lse.float(), ref.lse, lse_bnd) <= 1
    if c.branch != 'small':
        inf = R.build(c, poison=float('inf'))
        nq_pad, nk_pad = R.pads(c.nq, c.n_kv, c.nnull)
        nk = c.nnull + c.n_kv
        assert torch.isinf(inf.Q).any() == (nq_pad > c.nq) and torch.isinf(inf.K).any() == (nk_pad > nk) == bool(torch.isinf(inf.Vt).any())
        assert torch.equal(R.reference(c, inf).O, ref.O)
        assert torch.isnan(x.Q[:, c.nq:]).all() and torch.isnan(x.K[:, nk:]).all() and torch.isnan(x.Vt[:, :, nk:]).all()
        assert x.Q.shape == (c.S * c.h, nq_pad, 64) and x.K.shape == (c.S * c.h, nk_pad, 64) and x.Vt.shape == (c.S * c.h, 64, nk_pad)
        if c.dtype == R.BF16:
            for t in (x.Q[:, :c.nq], x.K[:, :nk], x.Vt[:, :, :nk]):
                assert torch.equal(t.to(torch.bfloat16).float(), t), 'bf16 images hold their values exactly'
    for m in R.MUTANTS:
        if not R.applies(m, c) or (c.branch == 'small' and m in ('admit_pad_key', 'lse_missing_key')):
            continue
        mut = mutant_ref(c, x, m)
        if m == 'lse_missing_key':
            with pytest.raises(AssertionError):
                R.check_lse(c.name, mut.lse.float(), ref.lse, lse_bnd)
            continue
        with pytest.raises(AssertionError, match='beyond their bound|non-finite'):        # non-finite: the only key of an n = 1 sequence dropped
            R.check(f'{c.name} / {m}', as_output(c, mut.O), ref.O, bnd, c.h * 64)


def test_checker_rejects_nan_and_slack_writes(built):
    c = CASES[1]
    x, ref, bnd, _ = built(c)
    good = as_output(c, ref.O)
    R.check(c.name, good, ref.O, bnd, c.h * 64)
    for r, col in ((0, 0), (ref.O.shape[0] - 1, c.h * 64 - 1), (7, 64)):
        bad = good.clone()
        bad[r, col] = float('nan')
        with pytest.raises(AssertionError, match='non-finite'):
            R.check(c.name, bad, ref.O, bnd, c.h * 64)
        bad[r, col] = float('inf')
        with pytest.raises(AssertionError, match='non-finite'):
            R.check(c.name, bad, ref.O, bnd, c.h * 64)
    for r, col in ((0, c.h * 64), (5, c.h * 64 + SLACK - 1)):
        bad = good.clone()
        bad[r, col] = 0.0
        with pytest.raises(AssertionError, match='slack'):
            R.check(c.name, bad, ref.O, bnd, c.h * 64)
    with pytest.raises(AssertionError):
        R.check(c.name, good[:, :c.h * 64], ref.O, bnd, c.h * 64)          # no slack to watch
    lse = ref.lse.float().clone()
    lse[0, 0] = float('nan')
    with pytest.raises(AssertionError, match='non-finite'):
        R.check_lse(c.name, lse, ref.lse, built(c)[3])


def test_bound_is_dominated_by_the_named_term():
    """the bf16 bound is the P rounding (2^-9, twice with the fixed-offset normaliser) and little else; the f32 and split-bf16 bounds stay below it"""
    by = {c.name: c for c in CASES}
    for name, lo, hi in (('lds_plain_q65_k65', R.U_BF16, 1.1 * R.U_BF16), ('fix_plain_q65_k96_tight', 2 * R.U_BF16, 2.2 * R.U_BF16),
                         ('free_f32_q130_k50_plain', 0.0, 2e-4), ('free_x3_q130_k50_plain', 3 * R.U_SPLIT, R.U_BF16)):
        c = by[name]
        x = R.build(c)
        ref = R.reference(c, x)
        _, _, t = R.bound(c, x, ref)
        first = t['p_round'] + t['norm'] + t['score'].max().item() + t['exp'] + t['accumulate']
        assert lo <= first <= hi, (name, first, {k: (v if isinstance(v, float) else v.max().item()) for k, v in t.items()})


@pytest.mark.parametrize('p', R.PREP_CASES, ids=lambda p: p['name'])
def test_prep_reference(p):
    x = R.build_prep(p)
    Q, K, V = R.reference_prep(p, x)
    nk = p['nnull'] + p['n_kv']
    assert Q.shape == (p['S'] * p['h'], p['nq'], 64)
    if p['scales']:
        assert torch.allclose((Q / x.q_scale.double()).norm(dim=-1), torch.full(Q.shape[:2], R.SCALE, dtype=torch.float64))
    if p['kv']:
        assert K.shape == V.shape == (p['S'] * p['h'], nk, 64)
        if p['nnull']:
            assert torch.equal(V[p['h'] + 1, 1], x.null_kv[1, 3].double()) and torch.equal(V[1, p['nnull']], x.kv[0, (p['h'] + 1) * 64:(p['h'] + 2) * 64].double())
    img = torch.randn(6, 64)
    hi = img.to(torch.bfloat16)
    planes = torch.cat((hi.view(6, 2, 32), (img - hi.float()).to(torch.bfloat16).view(6, 2, 32)), dim=-1).contiguous().view(6, 128).view(torch.float32)
    assert ((R.unsplit(planes, 64) - img.double()).abs() <= R.U_SPLIT * img.double().abs()).all()
