"""The vocabulary head (csrc/sampler.hip: pk_vocab_sample, pk_vocab_sample_philox, pk_vocab_reduce, pk_vocab_ce) held element by element to the float64
restatement of tests/vocab_reference.py: every (tile, row) partial of the tiled kernel in its twelve builds and of all eight builds of the resident kernel,
on strided, poisoned and guarded operands, no row left out; the folds on synthetic partials with exact ties; the refusals.  Every resident case asserts
that the launch counter moved, every tiled case that it did not.  The largest error / bound of every branch goes to the parity record
(profiles/vocab_parity.txt)."""
import pytest
import torch

from tests import vocab_reference as R
from tests.util import record_parity

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
TILED, RESIDENT = R.tiled_groups(), R.resident_groups()


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
    saved = _lib.get_vocab_resident()
    yield _lib
    _lib.set_vocab_resident_workers(0)
    _lib.set_vocab_resident(saved)


def branch_of(c):
    par, lse = c.noise in (R.PARITY, R.PHILOX), c.lse
    if R.is_resident(c):
        return 'resident<%d,%s,%s>' % (R.resident_build(c)[0], 'PARITY' if par else 'FAST', 'LSE' if lse else '-')
    return 'tiled<%s,%s,%s>' % (R.TNAME[c.dtype], 'PARITY' if par else 'FAST', 'LSE' if lse else '-')


def _launch(L, c, x, call=None):
    """the partials the launch left (int32 words, on the CPU) and the device buffers; asserts which kernel ran"""
    t = R.device_operands(c, x, 'cuda')
    saved = L.get_vocab_resident()
    L.set_vocab_resident(c.mode)
    L.set_vocab_resident_workers(c.workers)
    try:
        before = L.vocab_resident_launches()
        if call is None:
            rc = L.load().pk_vocab_sample(*R.sample_args(c, x, t), L.stream(t['A']))
        else:
            rc = call(t)
        made = L.vocab_resident_launches() - before
    finally:
        L.set_vocab_resident_workers(0)
        L.set_vocab_resident(saved)
    assert rc == 0, f'{c.name}: the entry point returned {rc}'
    torch.cuda.synchronize()
    assert made == (1 if R.is_resident(c) else 0), f'{c.name}: {"the tiled" if R.is_resident(c) else "the resident"} kernel ran'
    return t['partials'].cpu(), t


def _reduce(L, r, partials_dev):
    """pk_vocab_reduce on a reduce case; returns (pred, ids, scores) on the CPU"""
    t = R.reduce_buffers(r, 'cuda')
    p = lambda k, on=True: t[k].data_ptr() if (on and k in t) else None
    rc = L.load().pk_vocab_reduce(partials_dev.data_ptr() if partials_dev is not None else t['partials'].data_ptr(), r.M, r.V, p('rows'), p('mask'),
                                  p('ids', r.has_ids), p('pred'), p('scores', r.has_scores), 1 if r.lse else 0, L.stream(t['pred']))
    assert rc == 0, f'{r.name}: pk_vocab_reduce returned {rc}'
    torch.cuda.synchronize()
    return t['pred'].cpu(), t['ids'].cpu(), t['scores'].cpu()


def _run(L, cases, group):
    table = {}
    for c in cases:
        x = R.build(c)
        ref = R.reference(c, x)
        buf, t = _launch(L, c, x)
        got = R.check_partials(c, ref, buf)
        if c.data == 'grid':                                                         # the lowest index of equal maxima, after the reduce too
            r = R.reduce_case_of(c, x, buf, mask=False, scores=c.lse)
            pred, ids, scores = _reduce(L, r, t['partials'])
            R.check_reduce(r, R.reduce_ref(r), pred, ids, scores)
            first = (x.l64 == x.l64.max(-1, keepdim=True).values).int().argmax(-1)
            assert torch.equal(pred[R.lrows(c, x)], first), f'{c.name}: a later one of equal maxima won'
        for name, ratio in got.items():
            row = table.setdefault((branch_of(c), name, c.data), dict(cases=0, worst=-1.0, case=c.name))
            row['cases'] += 1
            if ratio > row['worst']:
                row.update(worst=ratio, case=c.name)
    for (branch, name, data), row in sorted(table.items()):
        record_parity(f'vocab_parity/{group}', dict(branch=branch, out=name, data=data, cases=row['cases'], err_over_bound=row['worst'], worst_case=row['case']))


@pytest.mark.parametrize('group', sorted(TILED))
def test_tiled_kernel(L, group):
    _run(L, TILED[group], 'tiled/' + group)


@pytest.mark.parametrize('group', sorted(RESIDENT))
def test_resident_kernel(L, group):
    _run(L, RESIDENT[group], 'resident/' + group)


def test_rule_keeps_the_tiled_kernel_below_2048_rows(L):
    _run(L, [R.below_rule_case()], 'tiled/below_rule')


def test_switches(L):
    lib = L.load()
    saved = L.get_vocab_resident()
    try:
        for mode in (0, 1, 2, 3):
            L.set_vocab_resident(mode)
            assert L.get_vocab_resident() == mode
        assert lib.pk_set_vocab_resident(4) == R.EINVAL and lib.pk_set_vocab_resident(-1) == R.EINVAL and L.get_vocab_resident() == 3
        assert lib.pk_set_vocab_resident_workers(-1) == R.EINVAL and lib.pk_set_vocab_resident_workers(257) == R.EINVAL
    finally:
        L.set_vocab_resident(saved)


@pytest.mark.parametrize('c', R.philox_cases(), ids=[c.name for c in R.philox_cases()])
def test_torch_philox(L, c):
    """the noise of torch's own generator at a non-zero offset: the partials against the materialised uniform_ fill, the generator where torch's op ends"""
    x = R.build(c)
    torch.manual_seed(20240229)
    torch.rand(1000, device='cuda')                                                  # a non-zero Philox offset
    spec = L.TorchPhilox(torch.device('cuda', 0), c.M * c.V)
    assert spec.offset > 0 and spec.offset % 4 == 0

    def call(t):
        return L.load().pk_vocab_sample_philox(c.dtype, t['A'].data_ptr(), x.geo.lda, t['W'].data_ptr(), x.geo.ldw, t['bias'].data_ptr(), c.M, c.V, c.D,
                                               float(c.T), None, spec.seed, spec.offset, spec.stride, 1 if c.lse else 0, t['partials'].data_ptr(),
                                               L.stream(t['A']))
    buf, _ = _launch(L, c, x, call)
    spec.advance()
    ours = spec.gen.get_offset()
    spec.gen.set_offset(spec.offset)
    U = torch.zeros(c.M, c.V, device='cuda').uniform_(0, 1)
    assert spec.gen.get_offset() == ours, 'the generator does not end where torch\'s uniform_ ends'
    got = R.check_partials(c, R.reference(c, x, U=U.cpu()), buf)
    for name, ratio in got.items():
        record_parity('vocab_parity/philox', dict(branch=branch_of(c), out=name, data='rand', cases=1, err_over_bound=ratio, worst_case=c.name))


@pytest.mark.parametrize('nt', R.REDUCE_NT)
def test_reduce_on_synthetic_partials(L, nt):
    worst, n = 0., 0
    for r in R.reduce_cases():
        if r.nt != nt:
            continue
        pred, ids, scores = _reduce(L, r, None)
        worst = max(worst, R.check_reduce(r, R.reduce_ref(r), pred, ids, scores))
        n += 1
    assert n >= len(R.REDUCE_M)
    record_parity('vocab_parity/reduce', dict(branch=f'reduce/ntiles={nt}', out='scores', data='synthetic', cases=n, err_over_bound=worst))


def _ce(L, c, x, partials_dev, targets):
    t = R.device_operands(c, x, 'cuda')
    loss = torch.full((c.M + R.CE_GUARD,), R.NAN, device='cuda')
    lse = torch.full((c.M + R.CE_GUARD,), R.NAN, device='cuda')
    rc = L.load().pk_vocab_ce(c.dtype, partials_dev.data_ptr(), c.M, c.V, t['A'].data_ptr(), x.geo.lda, t['W'].data_ptr(), x.geo.ldw, t['bias'].data_ptr(), c.D,
                              targets.data_ptr(), t['rows'].data_ptr() if 'rows' in t else None, loss.data_ptr(), lse.data_ptr(), L.stream(loss))
    assert rc == 0, f'{c.name}: pk_vocab_ce returned {rc}'
    torch.cuda.synchronize()
    loss, lse = loss.cpu(), lse.cpu()
    R.assert_untouched(loss[c.M:], f'{c.name}: loss guard rows')
    R.assert_untouched(lse[c.M:], f'{c.name}: lse guard rows')
    return loss[:c.M], lse[:c.M]


@pytest.mark.parametrize('dtype', (R.F32, R.BF16, R.BF16X3), ids=lambda d: R.TNAME[d])
def test_ce_on_synthetic_partials(L, dtype):
    worst = dict(lse=0., loss=0.)
    for dt, nt, D in R.ce_cases():
        if dt != dtype:
            continue
        c, x = R.ce_case(dt, nt, D)
        ref = R.ce_ref(c, x)
        loss, lse = _ce(L, c, x, R.ce_partials(c, x).cuda(), x.targets.cuda())
        worst['lse'] = max(worst['lse'], R.assert_within(lse, ref.lse, ref.dlse, f'{c.name}: lse'))
        worst['loss'] = max(worst['loss'], R.assert_within(loss, ref.loss, ref.dloss, f'{c.name}: loss'))
    for k, v in worst.items():
        record_parity('vocab_parity/ce', dict(branch=f'ce<{R.TNAME[dtype]}>', out=k, data='synthetic', cases=len(R.CE_NT) * len(R.CE_D), err_over_bound=v))


@pytest.mark.parametrize('name', ['tiled/f32/257x1156x40/parity+lse', 'res/m1/1300x1028/w3/parity+lse'])
def test_sample_reduce_ce(L, name):
    """end to end: the partials of a launch, their reduce and their cross entropy, each against the restatement"""
    c = {k.name: k for k in R.all_cases()}[name]
    x = R.build(c)
    buf, t = _launch(L, c, x)
    R.check_partials(c, R.reference(c, x), buf)
    r = R.reduce_case_of(c, x, buf)
    pred, ids, scores = _reduce(L, r, t['partials'])
    ratio = R.check_reduce(r, R.reduce_ref(r), pred, ids, scores)
    x.targets = torch.randint(0, c.V, (x.geo.total,), generator=R._gen(name + '/targets'))
    ref = R.ce_ref(c, x, r.pmax, r.psum)
    loss, lse = _ce(L, c, x, t['partials'], x.targets.cuda())
    out = dict(scores=ratio, lse=R.assert_within(lse, ref.lse, ref.dlse, f'{name}: lse'), loss=R.assert_within(loss, ref.loss, ref.dloss, f'{name}: loss'))
    for k, v in out.items():
        record_parity('vocab_parity/end_to_end', dict(branch=branch_of(c), out=k, data='rand', cases=1, err_over_bound=v, worst_case=name))


@pytest.mark.parametrize('label,dtype,err,change', R.SAMPLE_REFUSALS, ids=[r[0] for r in R.SAMPLE_REFUSALS])
def test_sample_refusals(L, label, dtype, err, change):
    c = R.refusal_base(dtype)
    x = R.build(c)
    t = R.device_operands(c, x, 'cuda')
    a = R.sample_args(c, x, t)
    change(a, x.geo)
    lib = L.load()
    assert lib.pk_vocab_sample(*a, L.stream(t['A'])) == err, label
    if not label.startswith('U '):                                                   # the Philox entry point takes no U
        ph = a[:10] + [None, 0, 0, 256, 1, a[15]]
        assert lib.pk_vocab_sample_philox(*ph, L.stream(t['A'])) == err, label + ' (philox)'
    torch.cuda.synchronize()
    assert (t['partials'].cpu() == R.SENT32).all(), f'{label}: a refused call wrote to the partials'


def test_philox_and_size_refusals(L):
    c = R.refusal_base(R.F32)
    x = R.build(c)
    t = R.device_operands(c, x, 'cuda')
    a = R.sample_args(c, x, t)
    lib, s = L.load(), L.stream(t['A'])
    ph = lambda off, stride: a[:10] + [None, 0, off, stride, 1, a[15]]
    assert lib.pk_vocab_sample_philox(*ph(0, 0), s) == R.EINVAL
    assert lib.pk_vocab_sample_philox(*ph(0, 384), s) == R.EINVAL                     # philox_stride % 256
    assert lib.pk_vocab_sample_philox(*ph(6, 256), s) == R.EINVAL                     # philox_offset % 4
    # the 4 GiB operand limit of the buffer descriptors, from the arguments alone: nothing of that size exists
    big = list(a)
    big[6] = 12_000_000                                                              # M * lda * 4 >= 2^32 - 16
    assert lib.pk_vocab_sample(*big, s) == R.EINVAL
    big = list(a)
    big[7] = 40_000_000                                                              # V * ldw * 4
    assert lib.pk_vocab_sample(*big, s) == R.EINVAL
    big[0] = R.BF16                                                                  # 2-byte elements: still over
    big[8], big[2], big[4] = 96, 104, 136
    assert lib.pk_vocab_sample(*big, s) == R.EINVAL
    torch.cuda.synchronize()
    assert (t['partials'].cpu() == R.SENT32).all(), 'a refused call wrote to the partials'
