"""What tests/patch_embed_reference.py promises, shown on the CPU with no kernel launched: the cases reach exactly the branches written out from the dispatch
code of csrc/patch_embed.hip and every listed property, the grid data set meets its preconditions (integer centres, bf16-exact x', sums below 2^24 grid
steps), the gather has an inverse, the float64 twin passes its own checker, an honest f32 emulation of the kernels' arithmetic (f32 running sum over exact
32-feature chunks, f32 statistics in the lanes' order, f32 epilogue) passes on every case and pass, the allowance is at most 1 % of the reference in rms on
every rand case, and each planted defect of the emulation is rejected on every case it applies to."""
import pytest
import torch

from tests import patch_embed_reference as R
from tests.util import record_parity

torch.set_grad_enabled(False)
CASES = R.gemm_cases()
FCASES = R.finish_cases()


@pytest.fixture(scope='module')
def built():
    """case name -> (x, [reference of pass 0, of pass 1]), computed once"""
    out = {}
    for c in CASES:
        x = R.build(c)
        out[c.name] = (x, [R.reference(c, x, p) for p in range(2)])
    return out


def test_names_branches_and_properties():
    names = [c.name for c in CASES + FCASES]
    assert len(set(names)) == len(names)
    reached, want = {R.branch_of(c) for c in CASES + FCASES}, R.expected_branches()
    assert reached == want, (sorted(reached - want), sorted(want - reached))
    for kernel, need in R.REQUIRED_PROPS.items():
        for data in ('grid', 'rand'):
            have = set().union(*(R.props_of(c) for c in CASES if c.kernel == kernel and c.data == data))
            assert need <= have, (kernel, data, sorted(need - have))
    for c in CASES:                                          # what the kernels' argument checks ask for
        B, C, F, H, W, pt, ph, pw, N = c.geo
        assert H % ph == 0 and W % pw == 0 and pw in (8, 16, 32, 64, 128) and N % 4 == 0 and (pw >= 32 or ph % (32 // pw) == 0)
        for G in c.groups:
            assert G.K % (192 if c.kernel == 'fused' else 64) == 0 and G.f0 + G.nt * G.pt <= F and G.rows >= 3
        assert c.kernel == 'fused' or N <= 512
        assert B * C * F * H * W * 4 <= 1.4e6
    # the conditions single cases exist for
    by = {c.name: c for c in CASES}
    assert [G.mtiles for G in by['f_rows576_g2/rand'].groups] == [5, 5]
    assert [G.ns for G in by['s_model_k/rand'].groups] == [6, 3] and [G.ns for G in by['s_k1088/rand'].groups] == [2]
    assert (by['s_k1024/rand'].groups[0].K // 64) % 3 != 0
    # the finish kernels alone
    assert {c.N for c in FCASES} == {4, 252, 256, 260, 512}
    assert {G.rows for c in FCASES for G in c.g} >= {1, 3, 4, 5, 130}
    assert {G.ns for c in FCASES for G in c.g} == {1, 2, 6}
    assert {c.outs for c in FCASES} == {('out',), ('out2',), ('out', 'out2')}
    assert any(G.remap == (0, 0, 0) for c in FCASES for G in c.g) and any(G.remap[1] > G.remap[0] > 0 for c in FCASES for G in c.g)
    assert any(len(c.g) == 2 and c.g[0].rows % 4 for c in FCASES)
    for m in R.MUTANTS:
        assert any(R.applies(m, c, p) for c in CASES + FCASES for p in range(2)), f'no case for the defect {m}'


def test_gather_has_an_inverse():
    v = torch.randn(2, 3, 5, 16, 32)
    for f0, nt, pt, ph, pw in ((1, 2, 2, 8, 16), (0, 1, 1, 4, 8), (2, 1, 3, 16, 32)):
        pat = R.gather(v, f0, nt, pt, ph, pw)
        assert pat.shape == (2 * nt * (16 // ph) * (32 // pw), 3 * pt * ph * pw)
        w = torch.zeros_like(v)
        R.scatter(w, pat, f0, nt, pt, ph, pw)
        assert torch.equal(w[:, :, f0:f0 + nt * pt], v[:, :, f0:f0 + nt * pt])
        assert not w[:, :, :f0].any() and not w[:, :, f0 + nt * pt:].any()
    # feature order (c, dt, y, x), row order (b, tt, hh, ww)
    pat = R.gather(v, 1, 2, 2, 8, 16)
    row, feat = ((1 * 2 + 1) * 2 + 1) * 2 + 1, ((2 * 2 + 1) * 8 + 5) * 16 + 7
    assert pat[row, feat] == v[1, 2, 1 + 1 * 2 + 1, 1 * 8 + 5, 1 * 16 + 7]


def test_grid_preconditions(built):
    worst = 0.0
    for c in CASES:
        if c.data == 'grid':
            x, refs = built[c.name]
            w = R.grid_preconditions(c, x)
            worst = max(worst, w.steps)
            for gi, G in enumerate(c.groups):                 # the flat patch: exact zeros, and the token row LayerNorm(t)
                if c.kernel == 'splitk':
                    fl = [sl * G.rows + x.flat[gi] for sl in range(G.ns)]
                    assert (refs[0][f'part{gi}'].ref[fl] == 0).all() and (refs[0][f'stats{gi}'].ref[fl] == 0).all()
                    t = x.t[gi].double()
                    ln = (t - t.mean()) / torch.sqrt(t.var(unbiased=False) + R.EPS2) * x.g2[gi].double() + x.b2[gi].double()
                    assert torch.allclose(refs[0]['tok'].ref[R.remap_rows(G.rows, G.remap)[x.flat[gi]]], ln, rtol=0, atol=1e-12)
                else:
                    assert torch.equal(refs[0][f'out{gi}'].ref[x.flat[gi]], x.t[gi].double())
            for name in refs[0]:                              # the integer offset changes no reference value
                assert torch.equal(refs[0][name].ref, refs[1][name].ref)
    assert 1000 < worst < 2 ** 24


def test_allowance_is_at_most_one_percent_of_the_reference(built):
    for c in CASES:
        if c.data == 'rand':
            for p in range(2):
                for name, frac in R.allowance_rms(built[c.name][1][p]).items():
                    assert frac <= 1e-2, f'{c.name} pass {p}: {name}: the allowance is {frac:.2e} of the reference (rms)'


def test_twin_and_emulation_pass_on_every_case(built):
    for c in CASES:
        x, refs = built[c.name]
        first = None
        for p in range(2):
            exact = {name: R.alloc(spec) for name, spec in R.blank(c).items()}
            for name, spec in R.blank(c).items():              # the float64 twin itself, rounded once to the buffer's type
                r = refs[p][name]
                R.window(exact[name], spec)[:, :spec.cols][r.mapped] = r.ref[r.mapped].float().to(spec.dtype)
            R.check(c, refs[p], exact, f'{c.name} (twin, pass {p})')
            out = R.emulate(c, x, p)
            for name, ratio in R.check(c, refs[p], out, f'{c.name} (emulation, pass {p})').items():
                record_parity('patch_embed_parity/emulation', dict(branch=R.branch_of(c), case=c.name, out=name, passno=p, err_over_bound=ratio))
            if c.data == 'grid':
                if first is None:
                    first = out
                else:
                    assert all(torch.equal(R._bits(first[k]), R._bits(out[k])) for k in out), f'{c.name}: the offset-64 pass differs'
    for c in FCASES:
        x = R.build_finish(c)
        ref = R.reference_finish(c, x)
        for name, ratio in R.check(c, ref, R.emulate_finish(c, x)).items():
            record_parity('patch_embed_parity/emulation', dict(branch=R.branch_of(c), case=c.name, out=name, passno=0, err_over_bound=ratio))
        # (the clamp rows are left out of the 1 % figure: at var = 0 the allowance is u sq/K over eps1, the conditioning of rstd itself)
        keep = ref['tok'].mapped.clone()
        for G in c.g:
            o = R.remap_rows(G.rows, G.remap)
            keep[o[torch.arange(G.rows) % 5 == 0]] = False
        if keep.any():
            frac = R.allowance_rms({'tok': R.NS(ref=ref['tok'].ref, bound=ref['tok'].bound, mapped=keep)})['tok']
            assert frac <= 1e-2, (c.name, frac)
        r = torch.arange(c.g[0].rows)                          # the rows the case exists for
        st = x.stats[0].double().sum(0)
        raw = st[:, 1] / c.g[0].K - (st[:, 0] / c.g[0].K) ** 2
        assert (raw[r % 5 == 0] < 0).all() and (raw[r % 5 == 0] > -1e-6).all(), 'the clamp row'
        if c.g[0].rows > 1:
            assert ((raw[r % 5 == 1] / (st[r % 5 == 1, 1] / c.g[0].K) - 1e-3).abs() < 1e-4).all(), 'the row whose two terms agree to 1e-3'


@pytest.mark.parametrize('mut', R.MUTANTS)
def test_planted_defect_is_rejected(built, mut):
    hit = 0
    for c in CASES:
        for p in range(2):
            if R.applies(mut, c, p):
                x, refs = built[c.name]
                with pytest.raises(AssertionError):
                    R.check(c, refs[p], R.emulate(c, x, p, mut), f'{c.name} ({mut})')
                hit += 1
    for c in FCASES:
        if R.applies(mut, c):
            x = R.build_finish(c)
            with pytest.raises(AssertionError):
                R.check(c, R.reference_finish(c, x), R.emulate_finish(c, x, mut), f'{c.name} ({mut})')
            hit += 1
    assert hit > 0


def test_bf16_interval():
    ref = torch.tensor([1.0, 1.00390625, 3.0], dtype=torch.float64)          # the second sits on a bf16 rounding boundary (tie to even: 1.0)
    lo, hi = R.f32_interval_to_bf16(ref, torch.tensor([0.0, 1e-6, 1e-6], dtype=torch.float64))
    assert lo.tolist() == [1.0, 1.0, 3.0] and hi.tolist() == [1.0, 1.0078125, 3.0]


def test_refusal_tables_change_one_thing():
    for label, entry, err, change in R.REFUSALS:
        assert entry in ('fused', 'splitk') and err in (R.PK_EINVAL, R.PK_EALIGN), label
    assert len({r[0] for r in R.REFUSALS}) == len(R.REFUSALS) and len({r[0] for r in R.FINISH_REFUSALS}) == len(R.FINISH_REFUSALS)
