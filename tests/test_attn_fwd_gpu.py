"""pk_attn_prep, pk_attn_fwd and pk_attn_small (csrc/attn.hip) held element by element to the float64 reference and the derived bound of
tests/attn_fwd_reference.py, one case per dispatch branch at the smallest shape that reaches it.  Inputs are that module's seeded, planted operand images with
poisoned pads (NaN, then +Inf), exactly as long as the kernel may read; outputs are pre-filled with NaN and have slack columns (ldo > h * 64).  Every case
asserts the branch it exists for from the host-visible conditions (pk_attn_pads, the CU count, the thresholds of attn_fwd_impl mirrored by
reference.branch_of), so a changed threshold fails the test instead of moving the case.  The worst error / bound of every case goes to the parity record.

Instantiations launched by attn_fwd_impl, and the case that reaches each (lds<QF, PF, TAB, FIX, T> = attn_fwd_lds_kernel, free<T, QF> = attn_fwd_kernel):
  lds<1,0,0,0,bf16>   lds_*_k64 / k65 / k96 / k160 (nk_pad < 192): plain, vector bias, scalar bias, mask, causal, null keys
  lds<1,1,0,0,bf16>   lds_*_k191 / k192 / k224 (nk_pad >= 192 switches the bias prefetch on), the same variants
  lds<1,0,1,0,bf16>   tab_*_runmax
  lds<1,0,1,1,bf16>   tab_*_tight / tab_*_loose, run4 and gather; wide_*_tab_64row
  lds<1,0,0,1,bf16>   fix_plain_*; wide_*_plain_64row
  lds<2,0,1,1,bf16>   wide_*_tab_128row        (S h ceil(nq_pad / 64) > 3 CUs)
  lds<2,0,0,1,bf16>   wide_*_plain_128row
  lds<2,*,0,0,bf16>, lds<2,0,1,0,bf16>   not reachable: 128-row workgroups are chosen for the fixed-offset form only, or through PK_ATTN_LDS_QF
  lds<2,1,..>, lds<1,1,..> at nk_pad < 192 and the converse   only through PK_ATTN_PF
  lds<2,0,0,1,x3>     x3_fix_q128_k192, x3_fix_q200_k191
  lds<2,0,1,1,x3>     x3_fix_tab_*
  lds<2,0,0,0,x3>     x3_lse_q130_vbias      (the training forward: lse, self-attention, n >= 128)
  lds<3,0,0,0,x3>     x3_lse_q130_qf3        (wg2 > CUs >= wg3)
  free<bf16,1|2>, free<f32,1|2>, free<x3,1|2>   free_*: fewer than 64 keys with 9 / 37 (16 rows per wave) and 130 / 260 (32) query rows, fewer than 64 query rows
                      with 200 keys, null keys, mask, a fully masked sequence, causal
  free<bf16,4>        only through PK_ATTN_MAX_QF; the DROP = true and DH = 32 / 128 forms: tests/test_dropout_gpu.py, tests/test_dim_head_gpu.py"""
import pytest
import torch

from tests import attn_fwd_reference as R
from tests.util import record_parity

pytestmark = pytest.mark.gpu

NAN = float('nan')
SLACK = 8
POISONS = (NAN, float('inf'))


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
    return _lib


def _n_cu():
    return torch.cuda.get_device_properties(0).multi_processor_count


def _image(L, c, t, row):
    """the operand image of the case's dtype, flat and exactly as long as the (S h) pairs need"""
    if c.dtype == R.BF16:
        return t.to(torch.bfloat16).cuda().reshape(-1)
    if c.dtype == R.F32:
        return t.cuda().reshape(-1)
    return L.split_planes(t.reshape(-1, row).cuda()).reshape(-1)


def _out(c, rows):
    """(buffer, O): O is the kernel's output, a view of a NaN-filled buffer with SLACK more columns"""
    buf = torch.full((rows, c.h * 64 + SLACK), NAN, device='cuda', dtype=torch.float32 if c.out_f32 else torch.bfloat16)
    return buf, buf[:, :c.h * 64]


def _structure_kw(c, x):
    kw = {}
    if c.bias in ('vec', 'scalar'):
        kw['bias'] = x.bias_buf.cuda()[:, :, :c.n_kv]
        b = kw['bias']
        vec = c.nnull == 0 and b.stride(1) % 4 == 0 and b.stride(0) % 4 == 0 and b.data_ptr() % 16 == 0            # AttnArgs::bias_vec
        assert vec == (c.bias == 'vec'), 'the bias rows must be 16-byte loadable exactly in the vector-bias cases'
    if c.mask is not None:
        kw['kmask'] = x.kmask.to(torch.uint8).cuda()
    if c.causal:
        kw.update(causal=True, slopes=x.slopes.cuda())
    return kw


def _launch(L, c, x):
    nq_pad, nk_pad = L.attn_pads(c.nq, c.n_kv, c.nnull)
    Qp, Kp, Vt = _image(L, c, x.Q, 64), _image(L, c, x.K, 64), _image(L, c, x.Vt, nk_pad)
    buf, O = _out(c, c.S * c.nq)
    kw = _structure_kw(c, x)
    if c.bias == 'table':
        kw['bias_table'] = (x.tab.cuda(), x.codes.cuda(), x.off, None, None, c.run4)
    if c.fix is not None:
        kw['score_bound'] = x.score_bound
    lse = torch.full((c.S * c.h * c.nq,), NAN, device='cuda') if c.lse else None
    L.attn_fwd(c.dtype, Qp, Kp, Vt, O, c.S, c.h, c.nq, c.n_kv, c.nnull, lse=lse, **kw)
    torch.cuda.synchronize()
    return buf, lse


def _run_case(L, c):
    n_cu = _n_cu()
    pad = L.attn_pads(c.nq, c.n_kv, c.nnull)
    assert pad == R.pads(c.nq, c.n_kv, c.nnull)
    assert R.branch_of(c, n_cu, pad) == c.branch, f'{c.name} no longer reaches {c.branch} on {n_cu} CUs'
    worst, worst_lse, ref, bnd = 0.0, 0.0, None, None
    for poison in POISONS:
        x = R.build(c, poison)
        if ref is None:
            ref = R.reference(c, x)
            bnd, lse_bnd, terms = R.bound(c, x, ref)
        buf, lse = _launch(L, c, x)
        worst = max(worst, R.check(f'{c.name} (pads {poison})', buf, ref.O, bnd, c.h * 64))
        if c.lse:
            worst_lse = max(worst_lse, R.check_lse(f'{c.name} (pads {poison})', lse, ref.lse, lse_bnd))
    first = {k: (v if isinstance(v, float) else v.max().item()) for k, v in terms.items() if k != 'lse'}
    record_parity(f'attn_fwd/{c.name}', dict(branch=c.branch, cus=n_cu, err_over_bound=worst, lse_err_over_bound=worst_lse if c.lse else None,
                                             largest_term=max(first, key=first.get), out='f32' if c.out_f32 else 'bf16'))


@pytest.mark.parametrize('c', R.FIXED_CASES, ids=lambda c: c.name)
def test_attn_fwd(L, c):
    _run_case(L, c)


@pytest.mark.parametrize('name', [c.name for c in R.cu_cases(R.NOMINAL_CUS)])
def test_attn_fwd_cu_dependent(L, name):
    """the 128-row fixed-offset workgroups (and the same shapes at the threshold: 64-row), the training forward's 64 / 48 rows per wave: S from the CU count"""
    c = {c.name: c for c in R.cu_cases(_n_cu())}[name]
    if name.startswith('wide'):
        wgs16 = c.S * c.h * -(-L.attn_pads(c.nq, c.n_kv, 0)[0] // 64)
        assert (wgs16 > 3 * _n_cu()) == name.endswith('128row')
    _run_case(L, c)


@pytest.mark.parametrize('c', R.small_cases(), ids=lambda c: c.name)
def test_attn_small(L, c):
    n, G = c.nq, 64 // c.nq
    assert G == 1 or c.S % G != 0, 'the last wave holds fewer sequences than the others'
    x = R.build_small(c)
    ref = R.reference_small(c, x)
    bnd, _, terms = R.bound(c, x, ref, ref.Q, ref.K, small=True)
    buf, O = _out(c, c.S * n)
    L.attn_small(x.q.cuda(), x.kv.cuda(), x.q_scale.cuda(), x.k_scale.cuda(), R.SCALE, O, c.S, c.h, n, **_structure_kw(c, x))
    torch.cuda.synchronize()
    worst = R.check(c.name, buf, ref.O, bnd, c.h * 64)
    record_parity(f'attn_fwd/{c.name}', dict(branch='pk_attn_small', err_over_bound=worst, out='f32' if c.out_f32 else 'bf16'))


def _read_image(dtype, img, rows, row):
    """(rows, -1, row) f64 values of an image pk_attn_prep wrote"""
    if dtype == R.BF16X3:
        return R.unsplit(img.cpu().view(-1, row), row).view(rows, -1, row)
    return img.double().cpu().view(rows, -1, row)


@pytest.mark.parametrize('p', R.PREP_CASES, ids=lambda p: p['name'])
def test_attn_prep(L, p):
    """the operand images against l2norm * scale in f64, to one output ulp plus the f32 norm error; pad rows / columns zero as the header of attn.hip promises"""
    S, h, nq, n_kv, nnull, dt = p['S'], p['h'], p['nq'], p['n_kv'], p['nnull'], p['dtype']
    nk, P = nnull + n_kv, S * h
    nq_pad, nk_pad = L.attn_pads(nq, n_kv, nnull)
    assert (nq_pad, nk_pad) == R.pads(nq, n_kv, nnull) and nq_pad > nq and nk_pad > nk
    x = R.build_prep(p)
    Qr, Kr, Vr = R.reference_prep(p, x)
    td = torch.bfloat16 if dt == R.BF16 else torch.float32
    Qp = torch.full((P * nq_pad * 64,), NAN, device='cuda', dtype=td)
    Kp = torch.full((P * nk_pad * 64,), NAN, device='cuda', dtype=td) if p['kv'] else None
    Vt = torch.full((P * 64 * nk_pad,), NAN, device='cuda', dtype=td) if p['kv'] else None
    dev = lambda t: None if t is None else t.cuda()
    L.attn_prep(dt, x.q.cuda(), dev(x.kv), dev(x.null_kv), dev(x.q_scale), dev(x.k_scale), R.SCALE, Qp, Kp, Vt, S, h, nq, n_kv, nnull)
    torch.cuda.synchronize()
    worst = {}

    def held(what, got, ref, normed):
        assert torch.isfinite(got).all(), f'{p["name"]} {what}: non-finite / unwritten elements'
        ratio = (got - ref).abs() / R.prep_bound(dt, ref, normed)
        worst[what] = ratio.max().item()
        assert worst[what] <= 1, f'{p["name"]} {what}: {worst[what]:.2f} x bound at {ratio.argmax().item()}'

    Q = _read_image(dt, Qp, P, 64)
    held('Qp', Q[:, :nq], Qr, p['scales'])
    assert (Q[:, nq:] == 0).all(), 'pad query rows are zero-filled'
    if p['kv']:
        K = _read_image(dt, Kp, P, 64)
        V = _read_image(dt, Vt, P, nk_pad)                          # (P, 64, nk_pad)
        held('Kp', K[:, :nk], Kr, p['scales'])
        held('Vt', V[:, :, :nk], Vr.transpose(1, 2), False)
        assert (K[:, nk:] == 0).all() and (V[:, :, nk:] == 0).all(), 'pad key rows / V^T columns are zero-filled'
    record_parity(f'attn_fwd/{p["name"]}', dict(branch='pk_attn_prep', err_over_bound=worst))


def test_refusals(L):
    """table with mask, causal, null keys or nq != n_kv: PK_EINVAL; ldo % 4 != 0: PK_EALIGN; f32 / split-bf16 images with a bf16 output (the kernels
    store f32 rows: they would overrun it): PK_EINVAL; a refused call leaves the output as it was"""
    c = next(c for c in R.FIXED_CASES if c.name == 'tab_2x5x7_gather_runmax')
    x = R.build(c)
    n = c.nq
    Qp, Kp, Vt = _image(L, c, x.Q, 64), _image(L, c, x.K, 64), _image(L, c, x.Vt, R.pads(n, n, 0)[1])
    table = (x.tab.cuda(), x.codes.cuda(), x.off)
    km = torch.ones(c.S, n, dtype=torch.uint8, device='cuda')
    slopes = torch.full((c.h,), 0.01, device='cuda')
    bad = (('PK_EINVAL', dict(bias_table=table, kmask=km), {}), ('PK_EINVAL', dict(bias_table=table, causal=True, slopes=slopes), {}),
           ('PK_EINVAL', dict(bias_table=table), dict(nnull=2, n_kv=n - 2)), ('PK_EINVAL', dict(bias_table=table), dict(nq=n - 6)),
           ('PK_EINVAL', dict(bias_table=table, score_bound=9.0, kmask=km), {}), ('PK_EALIGN', {}, dict(ldo=c.h * 64 + 2)),
           ('PK_EALIGN', dict(bias_table=table), dict(ldo=c.h * 64 + 2)))
    for err, kw, geo in bad:
        nq, n_kv, nnull = geo.get('nq', n), geo.get('n_kv', n), geo.get('nnull', 0)      # smaller than the images: a launch would stay inside them
        buf = torch.full((c.S * n, geo.get('ldo', c.h * 64 + SLACK)), NAN, device='cuda', dtype=torch.bfloat16)
        with pytest.raises(RuntimeError, match=err):
            L.attn_fwd(c.dtype, Qp, Kp, Vt, buf[:, :c.h * 64], c.S, c.h, nq, n_kv, nnull, **kw)
        torch.cuda.synchronize()
        assert torch.isnan(buf).all(), f'{err} {sorted(kw)} {geo}: a refused call wrote to the output'
    for name in ('free_f32_q9_k20_vbias', 'free_x3_q9_k20_vbias', 'free_f32_q130_k50_plain'):
        c = next(c for c in R.FIXED_CASES if c.name == name)
        x = R.build(c)
        buf = torch.full((c.S * c.nq, c.h * 64 + SLACK), NAN, device='cuda', dtype=torch.bfloat16)
        with pytest.raises(RuntimeError, match='PK_EINVAL'):
            L.attn_fwd(c.dtype, _image(L, c, x.Q, 64), _image(L, c, x.K, 64), _image(L, c, x.Vt, R.pads(c.nq, c.n_kv, 0)[1]), buf[:, :c.h * 64], c.S, c.h,
                       c.nq, c.n_kv, 0)
        torch.cuda.synchronize()
        assert torch.isnan(buf).all(), f'{name}: a refused call wrote to the output'
