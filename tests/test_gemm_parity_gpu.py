"""pk_gemm_ex, pk_gemm and pk_gemm_splitk (csrc/gemm.hip, gemm_core.hpp, gemm_dma.hpp, gemm_p8.hpp) held element by element to the float64 reference of
tests/gemm_reference.py: every main loop and epilogue of the switch tables, at the smallest shapes that can go wrong, on strided, poisoned and guarded
operands (NaN, then +Inf: both passes must leave the same bytes).  The exact grid must come out bit for bit; random data within the derived bound; C2, the
dup_rows copy and the hot-form / generic pair bit for bit.  One pytest id per main loop and list (shapes, tile-map conditions, epilogues); the largest
error / bound of every branch and output goes to the parity record (profiles/gemm_parity.txt).

The refusals behind the epilogue-form report (a variant with no instantiation for the type), those of pk_gemm_splitk and GEGLU with a residual through the
phenaki_mi355x::gemm op run here; they launch nothing and leave the output untouched."""
import pytest
import torch

from tests import gemm_reference as R
from tests.util import record_parity

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
GROUPS = R.grouped_cases()


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    torch.cuda.set_device(0)
    yield


@pytest.fixture(scope='module')
def L():
    from phenaki_pytorch_amd import _lib
    _lib.load()
    saved_forms, saved_pol = _lib.get_gemm_hot_forms(), _lib.get_cache_policy()
    _lib.set_gemm_hot_forms(1)
    _lib.set_cache_policy(0)
    yield _lib
    _lib.set_gemm_hot_forms(saved_forms)
    _lib.set_cache_policy(saved_pol)


def _launch(L, c, x):
    """the buffers the launch left, on the CPU"""
    t = R.operands(c, x, 'cuda')
    lib, s = L.load(), L.stream(t['C'])
    if c.entry == 'ex':
        rc = lib.pk_gemm_ex(*R.ex_args(c, x, t).values(), s)
    elif c.entry == 'gemm':
        rc = lib.pk_gemm(*R.gemm_args(c, x, t), s)
    else:
        rc = lib.pk_gemm_splitk(*R.splitk_args(c, x, t).values(), s)
    assert rc == 0, f'{c.name}: the entry point returned {rc}'
    torch.cuda.synchronize()
    return {k: t[k].cpu() for k in R.blank(c, x)}


def _same_bytes(a, b):
    return all(torch.equal(R._bits(a[k]), R._bits(b[k])) for k in a)


def _run_group(L, group):
    table = {}
    for c in GROUPS[group]:
        branch = R.branch_of(c)
        x = R.build(c)
        ref = R.reference(c, x)
        if c.entry == 'ex':
            assert L.load().pk_gemm_ex_form(*R.ex_args(c, x, R.operands(c, x, 'cuda')).values()) == R.form_of(c), f'{c.name} no longer takes {branch}'
        first = None
        for poison in R.POISONS:
            xp = x if poison != poison else R.build(c, poison)
            out = _launch(L, c, xp)
            got = R.check(c, xp, ref, out, f'{c.name} (poison {poison})')
            if first is None:
                first = out
            else:
                assert _same_bytes(first, out), f'{c.name}: the NaN- and the +Inf-poisoned pass leave different bytes'
            for name, (ratio, term) in got.items():
                row = table.setdefault((branch, name, 'grid' if ref.terms is None else 'rand'), dict(cases=set(), worst=-1.0, term=term, case=c.name))
                row['cases'].add(c.name)
                if ratio > row['worst']:
                    row.update(worst=ratio, term=term, case=c.name)
        if R.form_of(c):                                  # the compile-time form against the generic epilogue: bit for bit
            L.set_gemm_hot_forms(0)
            try:
                generic = _launch(L, c, x)
            finally:
                L.set_gemm_hot_forms(1)
            assert _same_bytes(first, generic), f'{c.name}: the {branch} form differs from the generic epilogue'
    for (branch, name, data), row in sorted(table.items()):
        record_parity(f'gemm_parity/{group}', dict(branch=branch, out=name, data=data, cases=len(row['cases']), err_over_bound=row['worst'], term=row['term'],
                                                   worst_case=row['case']))


@pytest.mark.parametrize('group', sorted(GROUPS))
def test_gemm_parity(L, group):
    _run_group(L, group)


def test_split_planes_image(L):
    w = torch.randn(37, 96)
    assert torch.equal(R.split_planes(w).view(torch.int32), L.split_planes(w.cuda()).cpu().view(torch.int32))


def _refused(L, fn, args, t, err, what):
    before = t['C'].clone()
    assert fn(*args, L.stream(t['C'])) == err, what
    torch.cuda.synchronize()
    assert torch.equal(R._bits(before), R._bits(t['C'])), f'{what}: a refused call wrote to the output'


def test_late_refusals(L):
    """a variant with no instantiation for the type is refused behind the form report: pk_gemm_ex_form accepts the call, pk_gemm_ex returns PK_EINVAL"""
    lib = L.load()
    for label, err, base, change in R.LATE_REFUSALS:
        c = R._base(base)
        x = R.build(c)
        t = R.operands(c, x, 'cuda')
        a = R.ex_args(c, x, t)
        change(a, t)
        assert lib.pk_gemm_ex_form(*a.values()) == 0, label
        _refused(L, lib.pk_gemm_ex, a.values(), t, err, label)


@pytest.mark.parametrize('label,err,base,change', R.SPLITK_REFUSALS, ids=[r[0] for r in R.SPLITK_REFUSALS])
def test_splitk_refusals(L, label, err, base, change):
    c = R.SPLITK_BASE[base]
    x = R.build(c)
    t = R.operands(c, x, 'cuda')
    a = R.splitk_args(c, x, t)
    change(a, t)
    _refused(L, L.load().pk_gemm_splitk, a.values(), t, err, label)


def test_geglu_with_a_residual_is_refused(L):
    """both epilogues store the GEGLU pair before the residual add: the call is refused by pk_gemm_ex, by _lib.gemm and by the phenaki_mi355x::gemm op"""
    import phenaki_pytorch_amd.ops  # noqa: F401
    M, K, N = 65, 72, 68
    xa = torch.randn(M, K, device='cuda').to(torch.bfloat16)
    w = torch.zeros(N, 128, device='cuda', dtype=torch.bfloat16)
    res = torch.randn(M, N // 2, device='cuda')
    for out in (torch.full((M, N // 2), 7.0, device='cuda'), torch.full((M, N // 2), 7.0, device='cuda', dtype=torch.bfloat16)):
        with pytest.raises(RuntimeError, match='PK_EINVAL'):
            L.gemm(L.BF16, xa, w, M, N, K, C=out, res=res, act=L.ACT_GEGLU)
        with pytest.raises(RuntimeError, match='PK_EINVAL'):
            torch.ops.phenaki_mi355x.gemm(xa, w, None, res, out, L.BF16, L.ACT_GEGLU)
        torch.cuda.synchronize()
        assert (out == 7.0).all(), 'a refused call wrote to the output'
    out = torch.full((M, N // 2), 7.0, device='cuda')
    torch.ops.phenaki_mi355x.gemm(xa, w, None, None, out, L.BF16, L.ACT_GEGLU)      # the same call without the residual is accepted
    torch.cuda.synchronize()
    assert (out == 0.0).all()
