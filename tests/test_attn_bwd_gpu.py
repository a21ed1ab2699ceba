"""pk_attn_bwd_ws (csrc/attn_train.hip) held element by element to the float64 reference and the derived bound of tests/attn_bwd_reference.py, one case per
dispatch branch at the smallest shape that reaches it, through the C entry point itself (ctypes): inputs are that module's seeded, planted operands, flat and
exactly as long as the shape needs, dO and O with poisoned slack columns (NaN, then +Inf); dQh, dKh, dVh, dS, lse and Drow lie in ONE NaN-filled buffer with
guard bands.  Every structural case runs in the three product forms and with the lse handed over or recomputed (a dropout site: handed over only, as the
dropout forward always does).  Every launch asserts its branch from the host-visible conditions (reference.branch_of against pk_attn_bwd_work), so a changed
threshold fails the case instead of moving it.  The worst error / bound of every case goes to the parity record.

Instantiations (X3: 0 f32, 1 split-bf16, 2 single bf16 products) and the cases that reach them:
  attn_bwd_q_kernel<0|1|2, false> + attn_bwd_kv_kernel<0|1|2, false>   every case without a site, each in all three forms
  attn_bwd_q_kernel<0|1|2, true>  + attn_bwd_kv_kernel<0|1|2, true>    drop_*, unpacked_n21_site, obf16_site_n65, each in all three forms
Host branches:
  packed (n <= 32, nnull = 0, n = n_kv, no dS, no site)   packed_n{1,9,21,31,32}_plain (a partly filled last tile each), packed_*_causal, packed_*_mask,
                                                          packed_*_bias_nodS (score()'s pack_n branch), full_packed_n21, first2_causal_packed_n9, obf16_packed_n9
  packing switched off by dS / null keys / a site         unpacked_n21_dS, unpacked_n21_null2, unpacked_n21_site
  kv_split G > 1, even deal of two tiles                  split_even_q192
  kv_split with a short last chunk                        split_short_q160; ending in a ragged 32-row tile: split_tail_q150
  G capped at the number of query tiles (chunk = 1)       every unpacked case at S h = 4 .. 6 with n > 32, e.g. plain_n130 (5 workgroups per key tile)
  G = 1 as the product reaches it (768 // (S h ntl) < 2)  g1_product_n40;  G = 1 with work = NULL: g1_nowork_n65;  n <= 32 unpacked: one query tile, G = 1
  have_lse = 0 (pass 1 of kernel Q and its lane merge)    every case without a site;  have_lse = 1: every case
  o_bf16 = 1                                              obf16_plain_n65, obf16_packed_n9, obf16_site_n65
  dS stores: 16-byte | scalar | jr & 3 != 0 | jr < 0      bias_dS_n64 | bias_dS_n65, drop_bias_dS_n33 | null2_mask_bias_* , cross_q65_k63_* | dS_null4_n36
  key tiles: 33, 63, 64, 65, 130 keys; cross-attention    plain_n*; cross_q65_k14 / k62 (exactly one tile) / k63 (one key into the second), q40_k129, q1_k70, q70_k1
  fully masked rows                                       full_n65_bias_dS, full_packed_n21, first2_causal_n65_bias_dS, first2_causal_packed_n9; the control with two
                                                          null keys, where no row is fully masked: first2_causal_null2_n63_bias_dS
  X3 = 2 on general f32 operands                          general2_n65 (every other X3 = 2 launch reads bf16-representable operands)
Reachable only through the environment switches, read once per process, and not covered: PK_ATTN_BWD_PACK=0 (the short self-attention shapes through the
unpacked kernels) and PK_ATTN_BWD_SPLIT=0 (split-bf16 asked for, X3 = 0 launched)."""
import ctypes

import pytest
import torch

from tests import attn_bwd_reference as B
from tests.util import record_parity

pytestmark = pytest.mark.gpu

NAN = float('nan')
POISONS = (NAN, float('inf'))
PK_EINVAL, PK_EALIGN = -1, -2


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


def _call(L, c, x, X3, have_lse, poison, *, work='auto', geo=None, ldo_extra=B.SLACK, lddo_extra=B.SLACK, slopes='auto', causal=None):
    """one pk_attn_bwd_ws call -> (rc, the output buffer of B.layout(c), lse handed over | None).  geo / ldo_extra / lddo_extra / slopes / work bend single
    arguments for the refusal test; everything else is the case's"""
    lib = L.load()
    dev = 'cuda'
    lay, total = B.layout(c)
    buf = torch.full((total,), NAN, device=dev)
    seg = lambda k: buf[lay[k][0]:]
    Qh, Kh, Vh = (t.reshape(-1).to(dev) for t in (x.Q, x.K, x.V))
    dO_buf = torch.full((c.S * c.n, c.h * 64 + lddo_extra), poison, dtype=torch.float32)
    dO_buf[:, :c.h * 64] = B.R.to_rows(c, x.dO)
    o_type = torch.bfloat16 if c.o_bf16 else torch.float32
    O_buf = torch.full((c.S * c.n, c.h * 64 + ldo_extra), poison, dtype=o_type)
    O_buf[:, :c.h * 64] = B.R.to_rows(c, x.O.contiguous()).to(o_type)
    dO_buf, O_buf = dO_buf.to(dev), O_buf.to(dev)
    bias = x.bias.to(dev) if x.bias is not None else None
    kmask = x.kmask.to(torch.uint8).to(dev) if x.kmask is not None else None
    sl = (x.slopes.to(dev) if x.slopes is not None else None) if slopes == 'auto' else slopes
    lse_in = None
    if have_lse:
        lse_in = x.lse32.reshape(-1).clone()
        seg('lse')[:lse_in.numel()] = lse_in.to(dev)
    need = lib.pk_attn_bwd_work(c.S, c.h, c.n, c.n_kv, c.nnull)
    assert need == B.work_floats(c), f'{c.name}: pk_attn_bwd_work {need} != the host mirror {B.work_floats(c)}'
    wbuf, wlen = None, 0
    if work == 'auto' and c.work and need > 0:
        wbuf, wlen = torch.full((need,), NAN, device=dev), need
    elif isinstance(work, int):
        wbuf, wlen = torch.full((max(need, 4),), NAN, device=dev), work
    site = ctypes.byref(L.Dropout(B.SEED, B.OFFSET, c.drop, x.scale)) if c.drop is not None else None
    S, h, n, n_kv, nnull = geo or (c.S, c.h, c.n, c.n_kv, c.nnull)
    flags = (1 if X3 == 1 else 0) | (2 if have_lse else 0) | (4 if X3 == 2 else 0)
    rc = lib.pk_attn_bwd_ws(Qh.data_ptr(), Kh.data_ptr(), Vh.data_ptr(), O_buf.data_ptr(), O_buf.stride(0), 1 if c.o_bf16 else 0, dO_buf.data_ptr(), dO_buf.stride(0),
                            L.ptr(bias), L.ptr(kmask), L.ptr(sl), int(c.causal if causal is None else causal), seg('dQ').data_ptr(), seg('dK').data_ptr(),
                            seg('dV').data_ptr(), seg('dS').data_ptr() if c.dS else None, seg('lse').data_ptr(), seg('D').data_ptr(), S, h, n, n_kv, nnull, flags,
                            L.ptr(wbuf), wlen, site, L.stream(Qh))
    torch.cuda.synchronize()
    return rc, buf, lse_in


@pytest.mark.parametrize('c', B.CASES, ids=lambda c: c.name)
def test_attn_bwd(L, c):
    n_cu = _n_cu()
    worst, by_form, terms, branch = 0.0, {}, {}, None
    built = {}
    for X3, hl in B.runs_of(c):
        rep = B.rep_of(c, X3)
        if rep not in built:
            x = B.build(c, rep)
            built[rep] = (x, B.reference(c, x))
        x, ref = built[rep]
        br = B.branch_of(c, X3, hl)
        branch = {k: v for k, v in br.items() if k not in ('X3', 'have_lse', 'kernels')}
        bnd = B.bound(c, x, ref, X3, hl)
        for poison in POISONS:
            rc, buf, lse_in = _call(L, c, x, X3, hl, poison)
            assert rc == 0, f'{c.name}: pk_attn_bwd_ws returned {rc}'
            w = B.check(f'{c.name} X3={X3} have_lse={hl} (slack {poison})', buf, c, ref, bnd, lse_in)
            print(f'{c.name} X3={X3} have_lse={hl} slack={poison}: ' + ' '.join(f'{k}={v:.3f}' for k, v in w.items()))
            key = f'{B.FORM_NAME[X3]}{"" if rep or X3 != 2 else "_general"}'
            by_form[key] = max(by_form.get(key, 0.0), max(w.values()))
            worst = max(worst, max(w.values()))
        terms[B.FORM_NAME[X3]] = B.largest_term(bnd)['dQ']
    record_parity(f'attn_bwd/{c.name}', dict(branch=branch, cus=n_cu, err_over_bound=worst, by_form=by_form, largest_term=terms, o='bf16' if c.o_bf16 else 'f32'))


@pytest.mark.parametrize('name', B.DETERMINISM)
def test_gradients_are_bit_reproducible(L, name):
    """the header of attn_train.hip: every result is owned by one workgroup and the kv_split slabs are added in index order"""
    c = B.BY_NAME[name]
    x = B.build(c, False)
    lay, _ = B.layout(c)
    for X3 in B.FORMS:
        a, b = (_call(L, c, x, X3, 0, NAN)[1] for _ in range(2))
        for k in ('dQ', 'dK', 'dV'):
            off, s = lay[k]
            cnt = s[0] * s[1] * s[2]
            assert torch.isfinite(a[off:off + cnt]).all() and torch.equal(a[off:off + cnt], b[off:off + cnt]), f'{name} X3={X3}: {k} differs between two runs'


def test_refusals(L):
    """causal with n != n_kv or without slopes, lddo % 4 != 0, ldo % 8 != 0 with a bf16 O, a workspace shorter than pk_attn_bwd_work asks for: an error code,
    nothing launched, the NaN-filled outputs untouched"""
    c = B.BY_NAME['plain_n65']
    x = B.build(c, False)
    cb = B.BY_NAME['obf16_plain_n65']
    xb = B.build(cb, False)
    slopes = torch.full((c.h,), 0.01, device='cuda')
    assert B.work_floats(c) > 0
    bad = (('causal, n != n_kv', PK_EINVAL, c, x, dict(causal=1, slopes=slopes, geo=(c.S, c.h, c.n, c.n_kv - 1, 0))),
           ('causal without slopes', PK_EINVAL, c, x, dict(causal=1, slopes=None)),
           ('lddo % 4', PK_EALIGN, c, x, dict(lddo_extra=6)),
           ('ldo % 8 with bf16 O', PK_EALIGN, cb, xb, dict(ldo_extra=4)),
           ('short workspace', PK_EINVAL, c, x, dict(work=B.work_floats(c) - 4)))
    for what, err, cc, xx, kw in bad:
        rc, buf, _ = _call(L, cc, xx, 0, 0, NAN, **kw)
        assert rc == err, f'{what}: returned {rc}, expected {err}'
        assert torch.isnan(buf).all(), f'{what}: a refused call wrote to the outputs'
    rc, buf, _ = _call(L, c, x, 0, 0, NAN)                              # the same call, unbent, runs
    assert rc == 0 and torch.isfinite(buf[B.layout(c)[0]['dQ'][0]]).item()
