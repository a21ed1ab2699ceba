"""ff1_resident_kernel (csrc/gemm_resident.hpp): the A-resident form of the first feed-forward GEMM -- bf16, K = 512, LayerNorm fold with handed-over
statistics, GEGLU, bf16 output -- against the tiled kernel it replaces (variant 24, form FF1) and against float64.

Every case is one pk_gemm_ex call on the strided, poisoned and guarded operands of tests/gemm_reference.py, launched with the switch on
(pk_set_ff1_resident) and with it off.  Asserted: the launch counter says which kernel ran; both launches leave the same bytes in the whole output
buffer, guard rows and slack columns included; the resident result passes gemm_reference.check -- the per-element float64 bound
tests/test_gemm_parity_gpu.py applies to the folded GEGLU form (accumulate + ln + gelu terms, interval check on the bf16 values), unchanged.

Shapes (K = 512), workers per panel forced through pk_set_ff1_resident_workers except in the last:
  128 x   48, 1 worker    3 sub-blocks on 8 waves: shared steps only, the first of them meeting the panel block by block
  130 x  400, 1 worker    a second panel with 2 live rows; 25 sub-blocks = 3 whole steps and one shared step
  272 x 2736, 7 workers   ranges of 24 and 25 sub-blocks, a 16-row last panel, 21 units over 8 XCD chunks
  4608 x 2736, default    variant 0 inside the dispatch window: 36 panels x 7 workers
Calls just outside the form (a bias; K = 448) and the switch at 0 must run the tiled kernel."""
import pytest
import torch

from tests import gemm_reference as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)


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
    saved = _lib.get_gemm_hot_forms(), _lib.get_cache_policy(), _lib.get_ff1_resident()
    _lib.set_gemm_hot_forms(1)
    _lib.set_cache_policy(0)
    yield _lib
    _lib.set_ff1_resident_workers(0)
    _lib.set_ff1_resident(saved[2])
    _lib.set_gemm_hot_forms(saved[0])
    _lib.set_cache_policy(saved[1])


def _ff1(name, M, N, K=512, variant=24, bias=False):
    return R._case(name, R.BF16, variant, M, N, K, act=R.ACT_GEGLU, out_bf16=True, ln=2, bias=bias)


def _launch(L, c, x, mode, workers):
    """(the buffers the launch left on the CPU, resident launches it made)"""
    t = R.operands(c, x, 'cuda')
    L.set_ff1_resident(mode)
    L.set_ff1_resident_workers(workers)
    try:
        before = L.ff1_resident_launches()
        rc = L.load().pk_gemm_ex(*R.ex_args(c, x, t).values(), L.stream(t['C']))
        made = L.ff1_resident_launches() - before
    finally:
        L.set_ff1_resident_workers(0)
        L.set_ff1_resident(1)
    assert rc == 0, f'{c.name}: pk_gemm_ex returned {rc}'
    torch.cuda.synchronize()
    return {k: t[k].cpu() for k in R.blank(c, x)}, made


def _same_bytes(a, b):
    return all(torch.equal(R._bits(a[k]), R._bits(b[k])) for k in a)


CASES = [('ff1res_128x48_w1', 128, 48, 24, 1), ('ff1res_130x400_w1', 130, 400, 24, 1), ('ff1res_272x2736_w7', 272, 2736, 24, 7),
         ('ff1res_4608x2736_auto', 4608, 2736, 0, 0)]


@pytest.mark.parametrize('name,M,N,variant,workers', CASES, ids=[c[0] for c in CASES])
def test_resident_equals_tiled_and_meets_the_float64_bound(L, name, M, N, variant, workers):
    c = _ff1(name, M, N, variant=variant)
    x = R.build(c)
    ref = R.reference(c, x)
    on, made_on = _launch(L, c, x, 1, workers)
    off, made_off = _launch(L, c, x, 0, workers)
    assert made_on == 1, f'{name}: the resident kernel was not taken'
    assert made_off == 0, f'{name}: switch off still launched the resident kernel'
    assert _same_bytes(on, off), f'{name}: the resident and the tiled kernel leave different bytes'
    ratio, term = R.check(c, x, ref, on, name)['C']
    print(f'{name}: err / bound {ratio:.3f} ({term})')


def test_explicit_variant_24_stays_tiled(L):
    """without the test override only variant 0 (the automatic choice) is replaced"""
    c = _ff1('ff1res_4608x2736_v24', 4608, 2736, variant=24)
    x = R.build(c)
    _, made = _launch(L, c, x, 1, 0)
    assert made == 0


@pytest.mark.parametrize('name,kw', [('ff1res_bias', dict(bias=True)), ('ff1res_k448', dict(K=448))], ids=['bias', 'k448'])
def test_calls_outside_the_form_run_the_tiled_kernel(L, name, kw):
    c = _ff1(name, 130, 400, **kw)
    x = R.build(c)
    ref = R.reference(c, x)
    on, made_on = _launch(L, c, x, 1, 1)
    off, made_off = _launch(L, c, x, 0, 1)
    assert made_on == 0 and made_off == 0, f'{name}: not the FF1 form at K = 512, yet the resident kernel ran'
    assert _same_bytes(on, off)
    R.check(c, x, ref, on, name)
