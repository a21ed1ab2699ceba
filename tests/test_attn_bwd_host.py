"""What tests/attn_bwd_reference.py promises, shown on the CPU: every case has the planted property, the closed form agrees with torch autograd of a plain
float64 attention, the reference rounded to f32 passes its own checker in every product form with either lse source, each mutant of the reference is rejected on
every case it applies to (under the f32 bound and under the loosest, the bf16 one), every mutant and every dispatch branch has a case, the bound is dominated
by the term it is named after, and the checker rejects a NaN, an unwritten element and a write into a guard band.  The cases are the ones
tests/test_attn_bwd_gpu.py launches."""
import pytest
import torch

from tests import attn_bwd_reference as B

NAN, INF = float('nan'), float('inf')


@pytest.fixture(scope='module')
def built():
    cache = {}

    def get(c, rep):
        key = (c.name, rep)
        if key not in cache:
            if len(cache) >= 2:
                cache.clear()                                  # the kv_split cases are large: keep the two operand sets of one case
            x = B.build(c, rep)
            cache[key] = (x, B.reference(c, x))
        return cache[key]
    return get


def test_names_branches_and_mutants_have_cases():
    names = [c.name for c in B.CASES]
    assert len(set(names)) == len(names)
    br = {c.name: B.branch_of(c, 0, 1) for c in B.CASES}
    nqt = lambda c: -(-c.n // 32)
    assert any(b['packed'] for b in br.values()) and any(not b['packed'] for b in br.values())
    for n in (1, 9, 21, 31, 32):
        assert any(b['packed'] and c.n == n and (c.S * c.h) % b['pack_g'] != 0 for c, b in zip(B.CASES, br.values())), f'no packed case with a part tile at n = {n}'
    for v in ('causal', 'mask', 'bias'):
        assert any(b['packed'] and (c.causal if v == 'causal' else (c.mask if v == 'mask' else c.bias)) for c, b in zip(B.CASES, br.values())), f'packed {v}'
    for name in ('unpacked_n21_dS', 'unpacked_n21_null2', 'unpacked_n21_site'):
        assert not br[name]['packed'] and B.BY_NAME[name].n <= 32
    split = [(c, b) for c, b in zip(B.CASES, br.values()) if b['G'] > 1]
    assert any(b['chunk'] > 1 and nqt(c) % b['chunk'] == 0 for c, b in split), 'kv_split with an even deal of more than one tile'
    assert any(b['chunk'] > 1 and nqt(c) % b['chunk'] != 0 for c, b in split), 'kv_split with a short last chunk'
    assert any(b['chunk'] > 1 and nqt(c) % b['chunk'] != 0 and c.n % 32 != 0 for c, b in split), 'a ragged tile in the short last chunk'
    assert any(b['G'] == nqt(c) and 768 // (c.S * c.h * -(-(c.nnull + c.n_kv) // 64)) > nqt(c) for c, b in split), 'G capped at nqt'
    assert br['g1_product_n40']['G'] == 1 and B.BY_NAME['g1_product_n40'].work and nqt(B.BY_NAME['g1_product_n40']) >= 2
    assert br['g1_nowork_n65']['G'] == 1 and B.kv_split_of(2, 3, 65, 65)[0] > 1, 'G = 1 only because no workspace is given'
    assert {b['dS_store'] for b in br.values()} == {None, 'vector', 'scalar', 'scalar+vector'}
    assert br['null2_mask_bias_n62']['dS_store'] == 'scalar' and br['bias_dS_n64']['dS_store'] == 'vector' and br['dS_null4_n36']['dS_store'] == 'scalar+vector'
    assert {b['DROP'] for b in br.values()} == {0, 1} and all(not b['packed'] for b in br.values() if b['DROP'])
    assert {c.drop for c in B.CASES} >= {None, 1, 64, 255}
    assert sum(c.o_bf16 for c in B.CASES) == 3 and {(br[c.name]['packed'], br[c.name]['DROP']) for c in B.CASES if c.o_bf16} == {(False, 0), (True, 0), (False, 1)}
    assert sum(c.general2 for c in B.CASES) == 1
    kernels = {B.branch_of(c, X3, hl)['kernels'] for c in B.CASES for X3, hl in B.runs_of(c)}
    assert kernels == {f'attn_bwd_q_kernel<{X3},{d}> + attn_bwd_kv_kernel<{X3},{d}>' for X3 in B.FORMS for d in (0, 1)}, 'the twelve instantiations'
    assert all(hl == 1 for c in B.CASES if c.drop is not None for _, hl in B.runs_of(c))
    full = [c for c in B.CASES if B.has_full_rows(c)]
    assert {(br[c.name]['packed'], c.causal) for c in full} == {(False, False), (True, False), (False, True), (True, True)}
    for m in B.MUTANTS:
        assert any(B.applies(m, c) for c in B.CASES), f'no case for the mutant {m}'
    for name in B.DETERMINISM:
        assert name in B.BY_NAME
    assert br[B.DETERMINISM[0]]['G'] > 1 and br[B.DETERMINISM[1]]['packed']


@pytest.mark.parametrize('c', B.CASES, ids=lambda c: c.name)
def test_planted_autograd_reference_and_mutants(built, c):
    nk = c.nnull + c.n_kv
    for rep in (False, True):
        x, ref = built(c, rep)
        if rep:
            for t in (x.Q, x.K, x.V, x.dO):
                assert torch.equal(t.to(torch.bfloat16).float(), t), 'the X3 = 2 operands hold bf16 values exactly'
        assert x.Q.shape == (c.S * c.h, c.n, 64) and x.K.shape == x.V.shape == (c.S * c.h, nk, 64)
        assert B.fully_masked_rows(ref.masked).any() == B.has_full_rows(c)
        assert (ref.dS_all[ref.masked] == 0).all()
        # the closed form against autograd
        ex, ag = B.reference(c, x, exact_O=True), B.autograd_reference(c, x)
        assert torch.allclose(ag.O, x.O_exact, rtol=0, atol=1e-12)
        for k in ('dQ', 'dK', 'dV', 'dS'):
            a, b = getattr(ex, k), getattr(ag, k)
            assert (a - b).abs().max().item() <= 1e-11 * max(1.0, b.abs().max().item()), f'{c.name}: closed-form {k} differs from autograd'
        shift = -ref.prob * (ref.D - ex.D)[:, :, None]        # the stored O enters through D alone
        assert torch.allclose(ref.dS_all, torch.where(ref.masked, torch.zeros_like(shift), ex.dS_all + shift), rtol=0, atol=1e-12)
        o_store = torch.bfloat16 if c.o_bf16 else torch.float32
        assert torch.equal(x.O.to(o_store).double(), x.O) and torch.equal(ref.D, (x.dO.double() * x.O).sum(-1))
        # poisoned slack columns leave the data alone
        for poison in (NAN, INF):
            buf, view = B.merged(c, x.dO, poison)
            assert torch.equal(view, B.R.to_rows(c, x.dO)) and (torch.isnan(buf[:, c.h * 64:]) if poison != poison else torch.isinf(buf[:, c.h * 64:])).all()
            assert buf.shape[1] == c.h * 64 + B.SLACK
        forms = [(X3, hl) for X3, hl in B.runs_of(c) if B.rep_of(c, X3) == rep]
        bnds = {f: B.bound(c, x, ref, *f) for f in forms}
        if rep:
            B.planted_property(c, x, ref, B.bound(c, x, ref, 2, 1).dS_all)
        for (X3, hl), bnd in bnds.items():
            assert all(torch.isfinite(getattr(bnd, k)).all() and (getattr(bnd, k) > 0).all() for k in ('dQ', 'dK', 'dV', 'dS_all', 'D'))
            lse_in = x.lse32 if hl else None
            worst = B.check(f'{c.name} X3={X3} lse={hl}', B.as_output(c, ref, lse_in), c, ref, bnd, lse_in)
            assert max(worst.values()) < 1, 'the f32 rounding of the outputs alone'
            if hl:
                moved = B.as_output(c, ref, x.lse32 + 1)
                with pytest.raises(AssertionError, match='handed over'):
                    B.check(c.name, moved, c, ref, bnd, lse_in)
        for m in B.MUTANTS:
            if not B.applies(m, c):
                continue
            mut = B.reference(c, x, m)
            for (X3, hl), bnd in bnds.items():
                if hl != 1 or X3 == 1:
                    continue                               # the f32 bound (tightest) and the bf16 one (loosest); the lse is an input
                with pytest.raises(AssertionError, match='beyond their bound|non-finite'):      # non-finite: the only key of a row dropped
                    B.check(f'{c.name} / {m} X3={X3}', B.as_output(c, mut, x.lse32), c, ref, bnd, x.lse32)


def test_checker_rejects_nan_unwritten_and_guard_writes(built):
    c = B.BY_NAME['bias_dS_n65']
    x, ref = built(c, False)
    bnd = B.bound(c, x, ref, 0, 0)
    good = B.as_output(c, ref)
    B.check(c.name, good, c, ref, bnd)
    lay, total = B.layout(c)
    assert all(off % 4 == 0 for off, _ in lay.values())
    for k, (off, s) in lay.items():
        cnt = 1
        for d in s:
            cnt *= d
        for at in (off, off + cnt - 1, off + cnt // 2):
            for v in (NAN, INF):
                bad = good.clone()
                bad[at] = v
                with pytest.raises(AssertionError, match='non-finite'):
                    B.check(c.name, bad, c, ref, bnd)
        for at in (off - 1, off - B.GUARD, off + -(-cnt // 4) * 4, off + -(-cnt // 4) * 4 + B.GUARD - 1):
            bad = good.clone()
            bad[at] = 0.0
            with pytest.raises(AssertionError, match='guard'):
                B.check(c.name, bad, c, ref, bnd)
        bad = good.clone()
        bad[off + cnt // 3] += 1.0
        with pytest.raises(AssertionError, match='beyond their bound'):
            B.check(c.name, bad, c, ref, bnd)
    with pytest.raises(AssertionError):
        B.check(c.name, good[:-1], c, ref, bnd)
    with pytest.raises(AssertionError, match='non-finite'):         # an lse the kernel should have computed and did not
        B.check(c.name, B.as_output(c, SimpleNamespaceWithout(ref, 'lse')), c, ref, bnd)


def SimpleNamespaceWithout(ref, k):
    from types import SimpleNamespace
    d = dict(vars(ref))
    d[k] = torch.full_like(d[k], NAN)
    return SimpleNamespace(**d)


def test_bound_is_dominated_by_the_named_term():
    """f32: the 64-term accumulations and __expf, parts in 10^5 at most; split-bf16: the operand residue 3 * 2^-16 (scores and the LDS round trip); X3 = 2 on
    bf16 operands: the 2^-9 rounding of P / dS on their way back from LDS, and little else; with general operands the score's operand term takes over.  The
    f32 and split bounds stay below the bf16 one."""
    c = B.BY_NAME['plain_n65']
    rel = {}
    for X3, rep, want in ((0, False, ('score', 'exp', 'accumulate', 'dP')), (1, False, ('operand', 'lds_operand')), (2, True, ('lds_operand',)),
                          ('2g', False, ('operand',))):
        x = B.build(c, rep)
        ref = B.reference(c, x)
        bnd = B.bound(c, x, ref, 2 if X3 == '2g' else X3, 1)
        big = B.largest_term(bnd)
        for out in ('dQ', 'dK', 'dV'):
            assert big[out] in want, (X3, out, bnd.terms[out])
        scale = dict(dQ=ref.dS_all.abs() @ x.K.double().abs(), dK=ref.dS_all.abs().transpose(1, 2) @ x.Q.double().abs(),
                     dV=ref.Pm.transpose(1, 2) @ x.dO.double().abs())
        rel[X3] = {out: (getattr(bnd, out) / scale[out]).median().item() for out in scale}
    for out in ('dQ', 'dK', 'dV'):
        # on the same (general f32) operands: f32 below split-bf16 below single bf16 products; f32 stays below a quarter of ONE bf16 rounding
        assert rel[0][out] < B.U_BF16 / 2 and rel[0][out] < rel[1][out] < rel['2g'][out], rel
        assert 2 * 3 * B.U_SPLIT <= rel[1][out] and 2 * 2 * B.U_BF16 <= rel['2g'][out], rel
        # on bf16 operands the bf16 form pays for the P / dS rounding and little else
        assert 2 * B.U_BF16 <= rel[2][out] <= 1.25 * 2 * B.U_BF16, rel
    assert B.largest_term(B.bound(c, x, ref, 2, 1))['dS'] == 'operand' and B.operand_terms(2, False) == (2 * B.U_BF16, 2 * B.U_BF16)
    assert B.BY_NAME['general2_n65'].general2 and not B.rep_of(B.BY_NAME['general2_n65'], 2)
