"""pk_qkv_project (csrc/qkv.hip), pk_qkv_attn and pk_q_attn_cached (csrc/qkv_attn.hip) held element by element to the float64 reference and the derived bounds
of tests/qkv_reference.py, launched through _lib.qkv_project / _lib.qkv_attn / _lib.q_attn_cached directly, one case per dispatch branch at the smallest shape
that reaches it.  Rows carry poisoned slack columns (ld > K; NaN, then +Inf), K has three k-tiles and a tail, every buffer is exactly as long as the contract
names.  Outputs are pre-filled with NaN and have slack columns (ldo > h * 64); the images pk_qkv_project writes are pre-filled with a NaN bit pattern that
the pad rows / columns must still hold afterwards; the cached images of pk_q_attn_cached are written by the reference, with poisoned K^ pad rows and zero V^T pad
columns (the kernel's precondition, include/phenaki_hip.h).
Every case asserts the branch it exists for (qkv_reference.branch_of); PK_QKV_TM must be unset.  The worst error / bound of every case, of its mean / std = 4
rows alone, and the share of image elements that may round either way go to the parity record.

Branches and the cases that reach them (T = bf16 | x3):
  project<T,1>:qkv[:fold]   project_T_n37_m111, _n200_m400_fold, _n43_m129_fold (M % 64 = 1), _n191_m191 (M % 64 = 63), _tm1_m2600, _tm1_m2660 (21 row tiles of 128)
  project<T,2>:qkv[:fold]   project_T_tm2_m2728 (M % 128 = 40), _tm2_m2788 (M % 128 = 100): h = 16, 22 row tiles of 128
  project<T,1|2>:q:fold     project_T_n37_query_only_fold, _tm1_query_only_m3872, _tm2_query_only_m4000 (h = 32); every small full case also runs its
                            query-only form, whose Q image must be bit-identical
  qkv_attn<T>:whole:*       attn_T_n64_plain (1 tile), _n64_vbias_fold (8 tiles, 16-byte bias loads), _n64_sbias (9 tiles, bias_ld = 65)
  qkv_attn<T>:masked:*      attn_T_n64_causal_fold; _n{1,7,9,10,21,32,33,63}_causal_alibi / _causal_noslopes (1 .. 64 sequences per tile, the last tile short);
                            _n9_bias_9tiles, _n33_bias, _n10_bias_causal
  q_attn_cached<T,nk32>     cached_T_nk1, _nk13_null_mask_fold, _nk13_null (9 tiles), _nk31_allmasked (no null keys, one sequence fully masked),
                            _nk32_null_fullmask_fold (only the null keys remain)
  q_attn_cached<T,nk64>     cached_T_nk33, _nk62_null_mask_fold, _nk64_null_fullmask, _nk64_fold"""
import os
from types import SimpleNamespace

import pytest
import torch

from tests import attn_fwd_reference as R
from tests import qkv_reference as Q
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
    assert 'PK_QKV_TM' not in os.environ, 'PK_QKV_TM overrides the tile height of pk_qkv_project: the branch assertions of this file need it unset'
    yield


@pytest.fixture(scope='module')
def L():
    from phenaki_pytorch_amd import _lib
    _lib.load()
    return _lib


def _operands(L, c, x):
    """rows in the operand type ((M, ld), slack poisoned), the packed weights, s, the scales -- on the GPU"""
    from phenaki_pytorch_amd import attention as A
    td = L.tdtype(c.dtype)
    g = SimpleNamespace()
    g.xq = x.xq.to(td).cuda()
    g.xkv = x.xkv.to(td).cuda() if x.xkv is not None else None
    g.wq = (x.wq_packed if c.fold else A.pack_linear_weight(x.wq, c.dtype)).cuda()
    g.wkv = A.pack_linear_weight(x.wkv, c.dtype).cuda() if x.wkv is not None else None
    g.s = x.s.cuda() if c.fold else None
    g.qs, g.ks = x.q_scale.cuda(), x.k_scale.cuda()
    assert g.xq.shape == (c.S * c.n, c.ld) and g.wq.stride(0) > c.K
    return g


def _out(c):
    buf = torch.full((c.S * c.n, c.h * 64 + SLACK), NAN, device='cuda', dtype=torch.float32 if c.out_f32 else torch.bfloat16)
    return buf, buf[:, :c.h * 64]


def _project(L, c, g, kv):
    bufs = [b.cuda() for b in Q.empty_images(c)]
    L.qkv_project(g.xq, g.xkv if kv else None, g.wq, g.wkv if kv else None, c.S, c.n, c.h, c.K, g.qs, g.ks if kv else None, Q.SCALE_PROJECT,
                  bufs[0], bufs[1], bufs[2], c.nq_pad, c.nk_pad, q_ln_s=g.s)
    torch.cuda.synchronize()
    return [b.cpu() for b in bufs]


@pytest.mark.parametrize('c', Q.PROJECT_CASES, ids=lambda c: c.name)
def test_qkv_project(L, c):
    assert Q.branch_of(c) == c.branch, f'{c.name} no longer reaches {c.branch}'
    assert (c.nq_pad, c.nk_pad) == L.attn_pads(c.n, c.n, 0)
    ref, worst = None, {}
    for poison in POISONS:
        x = Q.build(c, poison)
        if ref is None:
            ref = Q.reference(c, x)
        g = _operands(L, c, x)
        Qp, Kp, Vt = _project(L, c, g, c.kv)
        for what, (w, _) in Q.check_project(c, ref, Qp, Kp, Vt).items():
            worst[what] = max(worst.get(what, 0.0), w)
        if c.kv and not c.big:                             # the query-only form of the same inputs: the same Q image, no K^ / V^T image
            twin = Q._case('project', 'twin', c.dtype, c.S, c.n, c.h, '', fold=c.fold, K=c.K, kv=False, nq_pad=c.nq_pad, nk_pad=c.nk_pad)
            assert Q.branch_of(twin).startswith(f'project<{Q.T_NAME[c.dtype]},1>:q')
            Q2, K2, V2 = _project(L, twin, g, False)
            assert torch.equal(Q2, Qp), f'{c.name} (slack {poison}): the query-only form wrote another Q image'
            assert (K2 == Q.NAN_BITS).all() and (V2 == Q.NAN_BITS).all(), f'{c.name}: the query-only form wrote a K^ / V^T image'
    record_parity(f'qkv_parity/{c.name}', dict(branch=c.branch, err_over_bound=worst, marked_share=Q.marked_share(ref), mean4_rows=float(x.mean4.float().mean())))


def _attention_case(L, c, launch):
    assert Q.branch_of(c) == c.branch, f'{c.name} no longer reaches {c.branch}'
    ref, worst, worst4 = None, 0.0, None
    for poison in POISONS:
        x = Q.build(c, poison)
        if ref is None:
            ref = Q.reference(c, x)
            bnd, terms = Q.bound(c, x, ref)
        buf, O = _out(c)
        launch(x, _operands(L, c, x), O)
        torch.cuda.synchronize()
        worst = max(worst, R.check(f'{c.name} (poison {poison})', buf, ref.O, bnd, c.h * 64))
        if x.mean4.any():
            r4 = ((buf[:, :c.h * 64].double().cpu() - ref.O).abs() / bnd)[x.mean4].max().item()
            worst4 = max(worst4 or 0.0, r4)
    name, rel = Q.largest_term(c, ref, terms)
    record_parity(f'qkv_parity/{c.name}', dict(branch=c.branch, err_over_bound=worst, mean4_err_over_bound=worst4, marked_share=Q.marked_share(ref.img),
                                               largest_term=name, largest_term_over_A=rel[name], out='f32' if c.out_f32 else 'bf16'))


@pytest.mark.parametrize('c', Q.ATTN_CASES, ids=lambda c: c.name)
def test_qkv_attn(L, c):
    def launch(x, g, O):
        bias = x.bias_buf.cuda() if c.bias is not None else None          # (h, n, bias_ld) whole: the slack columns of its rows are poisoned
        if bias is not None:
            assert (bias.stride(0), bias.stride(1)) == (c.n * c.bias_ld, c.bias_ld)
        L.qkv_attn(g.xq, g.xkv, g.wq, g.wkv, c.S, c.n, c.h, c.K, g.qs, g.ks, Q.SCALE_ATTN, O, bias=bias,
                   slopes=x.slopes.cuda() if (c.causal and c.slopes) else None, causal=c.causal, q_ln_s=g.s)
    _attention_case(L, c, launch)


@pytest.mark.parametrize('c', Q.CACHED_CASES, ids=lambda c: c.name)
def test_q_attn_cached(L, c):
    assert c.nk_pad == L.attn_pads(c.n, c.n_kv, c.nnull)[1]
    P = c.S * c.h

    def image(t, row):
        """the cached image in the case's type, exactly S h nk_pad 64 elements long"""
        if c.dtype == Q.BF16:
            return t.to(torch.bfloat16).cuda().reshape(-1)
        return L.split_planes(t.reshape(-1, row).cuda()).reshape(-1)

    def launch(x, g, O):
        Kp, Vt = image(x.K, 64), image(x.Vt, c.nk_pad)
        assert Kp.numel() == Vt.numel() == P * c.nk_pad * 64
        L.q_attn_cached(g.xq, g.wq, c.S, c.n, c.h, c.K, g.qs, Q.SCALE_CACHED, Kp, Vt, c.nk_pad, c.n_kv, c.nnull, O,
                        kmask=x.kmask.to(torch.uint8).cuda() if c.mask is not None else None, q_ln_s=g.s)
    _attention_case(L, c, launch)
