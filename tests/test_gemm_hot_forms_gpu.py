"""Compile-time epilogue forms of pk_gemm_ex (csrc/gemm.hip: EPI_OUT, EPI_FF2A, EPI_FF2B, EPI_FF1) against the generic epilogue: every form
is launched with the forms on and with them off (pk_set_gemm_hot_forms) on the same inputs in one process, and C, C2 and stats_out must
be torch.equal -- the forms change no load, store or floating-point operation, so the comparison is bitwise.  Shapes: one interior
tile, M and N edges (N = 68 / 136: a last column tile of 4 / 8 columns), the K tail, several tiles, and for FF1 the product's N = 2736
with 16 partials per row; FF1's statistics come from an OUT-form launch on the same rows, which also tests the hand-over.  Calls the
forms must refuse (bias, scatter, dup_rows, a cache policy on the GEMM sites) must report form 0.  Needs a real MI355X (-m gpu)."""
import math

import pytest
import torch

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SENTINEL = -7.0          # finite fill of the outputs (elements a kernel must not touch compare equal too)


@pytest.fixture(scope='module')
def L():
    from phenaki_pytorch_amd import _lib
    _lib.load()
    assert torch.cuda.is_available(), 'these tests need the HIP device (no CPU fallback exists)'
    return _lib


@pytest.fixture(autouse=True)
def plain_policy_forms_on(L):
    saved_forms, saved_pol = L.get_gemm_hot_forms(), L.get_cache_policy()
    L.set_gemm_hot_forms(1)
    L.set_cache_policy(0)
    yield
    L.set_gemm_hot_forms(saved_forms)
    L.set_cache_policy(saved_pol)


def g(seed):
    return torch.Generator().manual_seed(seed)


def full(shape, dtype=torch.float32):
    return torch.full(shape, SENTINEL, device='cuda', dtype=dtype)


def operands(M, N, K, seed):
    from phenaki_pytorch_amd import attention as A
    from phenaki_pytorch_amd import _lib
    x = (torch.randn(M, K, generator=g(seed)) * 1.2 + 0.1).cuda().to(torch.bfloat16)
    W = (torch.randn(N, K, generator=g(seed + 1)) / math.sqrt(K)).cuda()
    return x, A.pack_linear_weight(W, _lib.BF16)


def on_and_off(L, fn, want_form):
    """fn() -> (form of its launch(es), outputs written into fresh buffers); with the forms on the form must be `want_form`, off 0, and
    every output identical bit for bit"""
    runs = []
    for on in (1, 0):
        L.set_gemm_hot_forms(on)
        form, outs = fn()
        assert form == (want_form if on else 0), f'forms {"on" if on else "off"}: form {form}'
        runs.append([t.clone() for t in outs])
    L.set_gemm_hot_forms(1)
    torch.cuda.synchronize()
    hot, generic = runs
    assert any((t.float() != SENTINEL).any() for t in generic), 'the kernel wrote nothing'
    for i, (a, b) in enumerate(zip(hot, generic)):
        assert a.dtype == b.dtype and torch.equal(a, b), f'output {i} differs between form {want_form} and the generic epilogue'
        if a.dtype == torch.bfloat16:                                 # bit for bit: torch.equal takes -0 for +0
            assert torch.equal(a.view(torch.int16), b.view(torch.int16)), f'output {i}: bit patterns differ'
        else:
            assert torch.equal(a.view(torch.int32), b.view(torch.int32)), f'output {i}: bit patterns differ'


RES_SHAPES = [(64, 64, 64), (80, 68, 64), (130, 512, 96), (192, 512, 512)]


def residual_call(L, form, M, N, K, **extra):
    """the to_out / second feed-forward Linear call in the form's shape: f32 residual in, f32 C [, bf16 C2 [, stats_out]]"""
    x, w = operands(M, N, K, 100 + N + K)
    res = torch.randn(M, N, generator=g(7 + M)).cuda()

    def fn():
        kw = dict(C=full((M, N)), res=res, variant=8)
        if form in (L.EPI_OUT, L.EPI_FF2A):
            kw['C2'] = full((M, N), torch.bfloat16)
        if form == L.EPI_OUT:
            kw['stats_out'] = full((M, (N + 31) // 32, 2))
        kw.update({k: (v() if callable(v) else v) for k, v in extra.items()})
        f = L.gemm_form(L.BF16, x, w, M, N, K, **kw)
        L.gemm(L.BF16, x, w, M, N, K, **kw)
        return f, [kw[k] for k in ('C', 'C2', 'stats_out') if kw.get(k) is not None]
    return fn


@pytest.mark.parametrize('M,N,K', RES_SHAPES)
def test_out_form(L, M, N, K):
    on_and_off(L, residual_call(L, L.EPI_OUT, M, N, K), L.EPI_OUT)


@pytest.mark.parametrize('M,N,K', RES_SHAPES)
def test_ff2a_form(L, M, N, K):
    on_and_off(L, residual_call(L, L.EPI_FF2A, M, N, K), L.EPI_FF2A)


@pytest.mark.parametrize('M,N,K', RES_SHAPES)
def test_ff2b_form(L, M, N, K):
    on_and_off(L, residual_call(L, L.EPI_FF2B, M, N, K), L.EPI_FF2B)


@pytest.mark.parametrize('M,N,K', [(128, 256, 64), (130, 136, 64), (256, 2736, 512)])
def test_ff1_form_fed_by_an_out_form_launch(L, M, N, K):
    from torch import nn
    from phenaki_pytorch_amd import attention as A
    dt = L.BF16
    o, wo = operands(M, K, 64, 40 + K)                      # the producer: rows of width K from a 64-deep product
    res = torch.randn(M, K, generator=g(41)).cuda()
    gamma, beta = (1 + 0.2 * torch.randn(K, generator=g(42))).cuda(), (0.1 * torch.randn(K, generator=g(43))).cuda()
    Wd = (torch.randn(N, K, generator=g(44)) / math.sqrt(K)).cuda()
    wg, s, t, _ = A.folded_weight(nn.Linear(1, 1), 'k', lambda: Wd, gamma, beta, dt, [gamma])

    def fn():
        rows, xt, st = full((M, K)), full((M, K), torch.bfloat16), full((M, K // 32, 2))
        kw_out = dict(C=rows, res=res, C2=xt, stats_out=st, variant=8)
        f_out = L.gemm_form(dt, o, wo, M, K, 64, **kw_out)
        L.gemm(dt, o, wo, M, K, 64, **kw_out)
        kw = dict(C=full((M, N // 2), torch.bfloat16), act=L.ACT_GEGLU, ln=(s, t, 1e-5), ln_stats=st, variant=24)
        f = L.gemm_form(dt, xt, wg, M, N, K, **kw)
        L.gemm(dt, xt, wg, M, N, K, **kw)
        assert f_out == (L.EPI_OUT if f else 0)
        return f, [rows, xt, st, kw['C']]
    on_and_off(L, fn, L.EPI_FF1)


def test_bias_is_refused(L):
    M, N, K = 130, 128, 96
    bias = torch.randn(N, generator=g(23)).cuda()
    for form in (L.EPI_OUT, L.EPI_FF2A, L.EPI_FF2B):
        on_and_off(L, residual_call(L, form, M, N, K, bias=bias), 0)


def test_dup_rows_is_refused(L):
    M, N, K, gap = 130, 128, 96, 5
    extra = dict(C=lambda: full((2 * M + gap, N)), C2=lambda: full((2 * M + gap, N), torch.bfloat16), dup_rows=M + gap)
    on_and_off(L, residual_call(L, L.EPI_FF2A, M, N, K, **extra), 0)


def test_scatter_is_refused(L):
    M, N, K = 130, 128, 96
    x, w = operands(M, N, K, 300)
    maps = ((torch.arange(M, dtype=torch.int32) * N).cuda(), torch.arange(N, dtype=torch.int32).cuda())      # the identity map

    def fn():
        kw = dict(C=full((M, N)), scatter=maps, variant=8)
        f = L.gemm_form(L.BF16, x, w, M, N, K, **kw)
        L.gemm(L.BF16, x, w, M, N, K, **kw)
        return f, [kw['C']]
    on_and_off(L, fn, 0)


@pytest.mark.parametrize('site,pol', [('gemm', 'CP_WT'), ('gemm', 'CP_NT'), ('ld_residual', 'CP_NT')])
def test_cache_policy_is_refused(L, site, pol):
    M, N, K = 130, 128, 96
    L.set_cache_policy(L.cache_policy_mask(**{site: getattr(L, pol)}))
    for form in (L.EPI_OUT, L.EPI_FF2B):
        on_and_off(L, residual_call(L, form, M, N, K), 0)
    # and the same call's result under the policy equals the hot form's under the plain one
    under = residual_call(L, L.EPI_OUT, M, N, K)()[1]
    L.set_cache_policy(0)
    f, plain = residual_call(L, L.EPI_OUT, M, N, K)()
    assert f == L.EPI_OUT
    for a, b in zip(under, plain):
        assert torch.equal(a, b)
