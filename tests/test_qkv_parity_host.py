"""What tests/qkv_reference.py promises, shown on the CPU: every case names the branch it reaches and every branch of the table is reached; the planted cases
have the planted-mass property; the float64 reference passes its own checkers (outputs: less than half an output ulp; images: bit for bit) with the row
slack and the pads poisoned, NaN and +Inf alike; at most MARK_CAP of the image elements of a case may round either way; every mutant of the reference is
rejected on every case it applies to and every mutant has a case; the checkers reject a NaN, a write into the slack columns of the output rows and a write
into the pad rows of an image; the reciprocal division of pk_qkv_attn holds for every tile row.  The cases are the ones tests/test_qkv_parity_gpu.py launches."""
import pytest
import torch

from tests import attn_fwd_reference as R
from tests import qkv_reference as Q

SLACK = 8
NAN, INF = float('nan'), float('inf')


def as_output(c, O):
    """what a kernel with exactly the reference's values would leave: rounded to the output type, in a NaN-filled buffer with slack columns"""
    buf = torch.full((O.shape[0], O.shape[1] + SLACK), NAN, dtype=torch.float32 if c.out_f32 else torch.bfloat16)
    buf[:, :O.shape[1]] = O.to(buf.dtype)
    return buf


def test_recip_identity():
    """x / n == (x * ceil(65536 / n)) >> 16 for every sequence length and every row of the 64-row tile (QkvAttnArgs::recip)"""
    for n in range(1, 65):
        for x in range(64):
            assert Q.recip_identity(n, x), (n, x)
    assert not all(Q.recip_identity(3, x) for x in range(1 << 17)), 'the identity is one of the tile height, not of every x'


def test_names_branches_and_mutants():
    names = [c.name for c in Q.CASES]
    assert len(set(names)) == len(names)
    for c in Q.CASES:
        assert Q.branch_of(c) == c.branch, (c.name, Q.branch_of(c), c.branch)
    reached = {c.branch for c in Q.CASES}
    want = set()
    for T in ('bf16', 'x3'):
        want |= {f'project<{T},{tm}>:{form}{fold}' for tm in (1, 2) for form, fold in (('qkv', ''), ('qkv', ':fold'), ('q', ':fold'))}
        want |= {f'qkv_attn<{T}>:whole:bias={b}' for b in ('none', 'vec:fold', 'scalar')}
        want |= {f'qkv_attn<{T}>:masked:bias={b}{f}' for b in ('none', 'none:alibi', 'scalar', 'scalar:alibi') for f in ('', ':fold') if (b, f) != ('scalar:alibi', ':fold')}
        want |= {f'q_attn_cached<{T},{nk}>{m}{f}' for nk in ('nk32', 'nk64') for m, f in (('', ''), (':mask', ''), (':mask', ':fold'))}
    assert want <= reached, sorted(want - reached)
    for m in Q.MUTANTS:
        assert any(Q.applies(m, c) for c in Q.CASES), f'no case for the mutant {m}'
    # the shapes the table asks for
    attn = [c for c in Q.ATTN_CASES if c.dtype == Q.BF16]
    assert {c.n for c in attn} == {64, *Q.ATTN_SHORT_N} and {c.h for c in attn} == {1, 3}
    assert {-(-c.S // (64 // c.n)) for c in attn} >= {1, 8, 9} and any(c.S % (64 // c.n) for c in attn if c.n <= 32)
    for n in Q.ATTN_SHORT_N:
        assert {bool(c.slopes) for c in attn if c.n == n and c.causal} == {True, False}
    cached = [c for c in Q.CACHED_CASES if c.dtype == Q.BF16]
    assert {c.nnull + c.n_kv for c in cached} == {1, 13, 31, 32, 33, 62, 64} and {c.nk_pad for c in cached} == {32, 64}
    assert {c.n for c in cached} == {64, 128, 192} and {c.nnull for c in cached} == {0, 2} and any(c.S * c.n // 64 % 8 for c in cached)
    assert any(c.mask == 'full' and c.nnull == 0 for c in cached) and any(c.mask == 'full' and c.nnull == 2 for c in cached)
    proj = [c for c in Q.PROJECT_CASES if c.dtype == Q.BF16 and not c.big]
    assert {c.S * c.n % 64 for c in proj} >= {1, 63} and {c.n for c in proj} >= {37, 200} and all(c.nq_pad > c.n and c.nk_pad > c.n for c in proj if c.n == 37)
    big = {c.name.split('_', 2)[2]: c for c in Q.PROJECT_CASES if c.dtype == Q.BF16 and c.big}
    assert 0 < big['tm2_m2728'].S * big['tm2_m2728'].n % 128 <= 64 < big['tm2_m2788'].S * big['tm2_m2788'].n % 128


def _check_inputs(c, x, inf):
    K = c.K
    assert c.ld > K and K % Q.KTILE[c.dtype] == (8 if c.dtype == Q.BF16 else 4) and K > 64
    for name in ('xq', 'xkv'):
        t, ti = getattr(x, name), getattr(inf, name)
        if t is None:
            continue
        assert t.shape == (c.S * c.n, c.ld) and torch.isnan(t[:, K:]).all() and torch.isinf(ti[:, K:]).all() and torch.equal(t[:, :K], ti[:, :K])
        if c.dtype == Q.BF16:
            assert torch.equal(t[:, :K].to(torch.bfloat16).float(), t[:, :K]), 'bf16 rows hold their values exactly'
    if c.dtype == Q.BF16:
        for w in (x.wq, x.wkv):
            assert w is None or torch.equal(w.to(torch.bfloat16).float(), w), 'bf16 weights hold their values exactly'
    if c.fold:
        rows = x.xq[x.mean4][:, :K].double()
        ratio = rows.mean(dim=1).abs() / rows.std(dim=1)
        assert x.mean4.any() and (ratio > 3).all() and (ratio < 5).all(), (ratio.min().item(), ratio.max().item())
    if c.kernel == 'cached':
        nk = c.nnull + c.n_kv
        assert x.K.shape == (c.S * c.h, c.nk_pad, 64) and x.Vt.shape == (c.S * c.h, 64, c.nk_pad) and c.nk_pad == R.pads(c.n, c.n_kv, c.nnull)[1]
        assert torch.isnan(x.K[:, nk:]).all() and torch.isinf(inf.K[:, nk:]).all()
        assert (x.Vt[:, :, nk:] == 0).all() and (inf.Vt[:, :, nk:] == 0).all(), 'the precondition of pk_q_attn_cached: V^T pad columns finite'
    if c.bias is not None:
        assert torch.isnan(x.bias_buf[:, :, c.n:]).all() and torch.isinf(inf.bias_buf[:, :, c.n:]).all()


@pytest.mark.parametrize('c', Q.CASES, ids=lambda c: c.name)
def test_reference_and_mutants(c):
    x, inf = Q.build(c), Q.build(c, INF)
    _check_inputs(c, x, inf)
    ref = Q.reference(c, x)
    share = Q.marked_share(ref if c.kernel == 'project' else ref.img)
    assert share <= Q.MARK_CAP, f'{c.name}: {share:.2%} of the image elements may round either way'
    if c.kernel == 'project':
        worst = Q.check_project(c, ref, *Q.place(c, ref))
        assert all(w == 0 for w, _ in worst.values()) or c.dtype == Q.BF16X3, 'bf16: the rounded reference bit for bit'
        assert torch.equal(Q.reference(c, inf).Q, ref.Q)
        for m in Q.MUTANTS:
            if Q.applies(m, c):
                bufs = Q.empty_images(c)
                if m == 'query_only_writes_k':
                    bufs[1][3, 5] = 0x3F80
                with pytest.raises(AssertionError):
                    Q.check_project(c, ref, *Q.place(c, Q.reference(c, x, m), bufs))
        return
    R.planted_property(c, x, ref)
    bnd, _ = Q.bound(c, x, ref)
    assert torch.isfinite(ref.O).all() and (bnd > 0).all()
    assert R.check(c.name, as_output(c, ref.O), ref.O, bnd, c.h * 64) < 0.5, 'the output rounding alone: less than half an output ulp'
    assert torch.equal(Q.reference(c, inf).O, ref.O)
    for m in Q.MUTANTS:
        if Q.applies(m, c):
            with pytest.raises(AssertionError, match='beyond their bound|non-finite'):
                R.check(f'{c.name} / {m}', as_output(c, Q.reference(c, x, m).O), ref.O, bnd, c.h * 64)


def test_checkers_reject_nan_slack_and_pad_writes():
    c = next(c for c in Q.ATTN_CASES if c.name == 'attn_bf16_n9_bias_9tiles')
    x = Q.build(c)
    ref = Q.reference(c, x)
    bnd, _ = Q.bound(c, x, ref)
    good = as_output(c, ref.O)
    R.check(c.name, good, ref.O, bnd, c.h * 64)
    for bad_value in (NAN, INF):
        bad = good.clone()
        bad[7, 11] = bad_value
        with pytest.raises(AssertionError, match='non-finite'):
            R.check(c.name, bad, ref.O, bnd, c.h * 64)
    bad = good.clone()
    bad[5, c.h * 64 + SLACK - 1] = 0.0
    with pytest.raises(AssertionError, match='slack'):
        R.check(c.name, bad, ref.O, bnd, c.h * 64)
    for dt in ('bf16', 'x3'):
        c = next(c for c in Q.PROJECT_CASES if c.name == f'project_{dt}_n37_m111')
        ref = Q.reference(c, Q.build(c))
        Q.check_project(c, ref, *Q.place(c, ref))
        for which, what in ((0, 'pad query rows'), (1, 'pad key rows'), (2, 'pad key columns')):
            bufs = list(Q.place(c, ref))
            e = 1 if c.dtype == Q.BF16 else 2
            if which == 2:
                bufs[2][10, (c.nk_pad - 1) * e - (e - 1) * 31] = 0            # key nk_pad - 1 (split-bf16: its hi plane element)
            else:
                pad = (c.nq_pad, c.nk_pad)[which]
                bufs[which].view(c.S * c.h, pad, 64 * e)[1, c.n, 0] = 0
            with pytest.raises(AssertionError, match=what):
                Q.check_project(c, ref, *bufs)
        bufs = list(Q.place(c, ref))
        bufs[0].view(c.S * c.h, c.nq_pad, -1)[0, 3, 7] = Q.NAN_BITS            # an unwritten element
        with pytest.raises(AssertionError, match='non-finite'):
            Q.check_project(c, ref, *bufs)
        if c.dtype == Q.BF16:                                                  # one ulp on an unmarked element
            bufs = list(Q.place(c, ref))
            free = (~ref.mQ[0, 3]).nonzero()[0].item()
            bufs[0].view(c.S * c.h, c.nq_pad, -1)[0, 3, free] += 1
            with pytest.raises(AssertionError, match='unmarked'):
                Q.check_project(c, ref, *bufs)
