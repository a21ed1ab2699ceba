"""CPU-only: which epilogue form (pk_gemm_epilogue_form / pk_gemm_ex_form, csrc/gemm.hip) a GEMM call gets.  The three layer calls of a
bf16 transformer block, issued by attention.py itself on CPU tensors with L.gemm replaced by the form query, must get OUT, FF1 and
FF2A / FF2B; a bias, a scatter, duplicated rows, a cache policy, another dtype or another main-loop variant must get the generic
form 0, and so must everything while the switch is off.  No kernel is launched."""
import pytest
import torch

torch.set_grad_enabled(False)
M, D, HEADS = 4608, 512, 8          # rows of the batch-8 encode step, model width


@pytest.fixture(scope='module')
def L():
    from phenaki_pytorch_amd import _lib, build
    build.build(verbose=False)
    _lib.load()
    return _lib


@pytest.fixture
def hot(L):
    saved_forms, saved_pol = L.get_gemm_hot_forms(), L.get_cache_policy()
    L.set_gemm_hot_forms(1)
    L.set_cache_policy(0)
    yield L
    L.set_gemm_hot_forms(saved_forms)
    L.set_cache_policy(saved_pol)


def layer_forms(L, want_t):
    """forms of the GEMMs Attention._finish and FeedForwardSeq._run issue at M rows, in call order"""
    from phenaki_pytorch_amd import attention as A
    forms = []
    real = L.gemm

    def query(*a, **kw):
        forms.append(L.gemm_form(*a, **kw))
        return kw.get('C')
    attn, ff = A.Attention(D, heads=HEADS), A.FeedForward(D)
    x = torch.zeros(M, D)
    o = torch.zeros(M, HEADS * 64, dtype=torch.bfloat16)
    L.gemm = query
    try:
        out, out_t, stats = attn._finish(o, x, L.BF16, 'stats')
        assert out_t is not None and stats is not None and stats.shape == (M, D // 32, 2)
        ff._run(out, L.BF16, out_t, want_t, stats)
    finally:
        L.gemm = real
    return forms


def test_layer_calls_get_their_forms(hot):
    L = hot
    assert layer_forms(L, True) == [L.EPI_OUT, L.EPI_FF1, L.EPI_FF2A]
    assert layer_forms(L, False) == [L.EPI_OUT, L.EPI_FF1, L.EPI_FF2B]


def test_switch_forces_the_generic_form(hot):
    L = hot
    L.set_gemm_hot_forms(0)
    assert L.get_gemm_hot_forms() == 0
    assert layer_forms(L, True) == [0, 0, 0]
    L.set_gemm_hot_forms(1)
    assert L.get_gemm_hot_forms() == 1
    assert layer_forms(L, True) == [L.EPI_OUT, L.EPI_FF1, L.EPI_FF2A]


def _out_call(L, dt=None, **over):
    """a to_out-shaped call on CPU tensors; `over` replaces / adds keyword arguments of L.gemm"""
    dt = L.BF16 if dt is None else dt
    m, n, k = 130, 128, 64
    td = L.tdtype(dt)
    x, w = torch.zeros(m, k, dtype=td), torch.zeros(n, k, dtype=td)      # (split-bf16: the pre-split image has the f32 layout's strides)
    kw = dict(C=torch.zeros(m, n), res=torch.zeros(m, n), variant=8)
    if dt == L.BF16:
        kw.update(C2=torch.zeros(m, n, dtype=torch.bfloat16), stats_out=torch.zeros(m, n // 32, 2))
    kw.update(over)
    return L.gemm_form(dt, x, w, m, n, k, **kw)


def test_refusals_of_the_whole_call(hot):
    L = hot
    m, n = 130, 128
    assert _out_call(L) == L.EPI_OUT
    assert _out_call(L, stats_out=None) == L.EPI_FF2A
    assert _out_call(L, stats_out=None, C2=None) == L.EPI_FF2B
    assert _out_call(L, bias=torch.zeros(n)) == 0
    assert _out_call(L, stats_out=None, dup_rows=m, C=torch.zeros(2 * m, n), C2=torch.zeros(2 * m, n, dtype=torch.bfloat16)) == 0
    scatter = (torch.arange(m, dtype=torch.int32) * n, torch.arange(n, dtype=torch.int32))
    assert _out_call(L, res=None, C2=None, stats_out=None, scatter=scatter) == 0
    assert _out_call(L, C2=None) == 0                                 # statistics of the f32 rows: no such hot call
    assert _out_call(L, res=None) == 0
    assert _out_call(L, variant=33) == 0 and _out_call(L, variant=24) == 0 and _out_call(L, variant=27) == 0
    assert _out_call(L, stats_out=None, variant=9) == 0 and _out_call(L, stats_out=None, variant=1) == 0
    assert _out_call(L, C2=None, stats_out=None, C=torch.zeros(m, n + 2)[:, :n]) == 0        # ldc = 130: the scalar epilogue
    assert _out_call(L, L.F32) == 0 and _out_call(L, L.BF16X3) == 0
    for mask in (L.cache_policy_mask(gemm=L.CP_WT), L.cache_policy_mask(gemm=L.CP_NT), L.cache_policy_mask(ld_residual=L.CP_NT)):
        L.set_cache_policy(mask)
        assert _out_call(L) == 0 and _out_call(L, stats_out=None) == 0
    L.set_cache_policy(L.cache_policy_mask(peg=L.CP_WT, ld_video=L.CP_NT))      # other sites' policies do not matter
    assert _out_call(L) == L.EPI_OUT


def test_ff1_form_and_its_refusals(hot):
    L = hot
    m, n, k = 130, 136, 64
    xt, w = torch.zeros(m, k, dtype=torch.bfloat16), torch.zeros(n, k, dtype=torch.bfloat16)
    s, t, st = torch.zeros(n), torch.zeros(n), torch.zeros(m, k // 32, 2)

    def form(variant=24, **over):
        kw = dict(C=torch.zeros(m, n // 2, dtype=torch.bfloat16), act=L.ACT_GEGLU, ln=(s, t, 1e-5), ln_stats=st, variant=variant)
        kw.update(over)
        return L.gemm_form(L.BF16, xt, w, m, n, k, **kw)
    assert form() == L.EPI_FF1
    assert form(8) == 0 and form(9) == 0                              # the 64x64 / 4-wave folded tiles
    assert form(ln_stats=None) == 0                                   # in-loop statistics
    assert form(bias=torch.zeros(n)) == 0
    assert form(C=torch.zeros(m, n // 2)) == 0                        # f32 GEGLU output
    assert form(act=L.ACT_NONE, C=torch.zeros(m, n, dtype=torch.bfloat16)) == 0
    assert form(act=L.ACT_NONE, C=torch.zeros(m, n), res=torch.zeros(m, n)) == 0
    L.set_cache_policy(L.cache_policy_mask(gemm=L.CP_NT))
    assert form() == 0


def test_pure_form_function(L):
    """pk_gemm_epilogue_form on bare fields: independent of the switch and of the process mask"""
    f = L.gemm_epilogue_form
    out = dict(res=1, C2=1, stats_out=1)
    ff1 = dict(ln_kind=2, act=L.ACT_GEGLU, out_is_f32=0)
    saved = L.get_gemm_hot_forms()
    try:
        for on in (0, 1):
            L.set_gemm_hot_forms(on)
            assert f(L.BF16, 8, **out) == L.EPI_OUT
            assert f(L.BF16, 8, res=1, C2=1) == L.EPI_FF2A and f(L.BF16, 8, res=1) == L.EPI_FF2B
            assert f(L.BF16, 24, **ff1) == L.EPI_FF1
    finally:
        L.set_gemm_hot_forms(saved)
    for dt in (L.F32, L.BF16X3):
        assert f(dt, 8, **out) == 0 and f(dt, 8, res=1) == 0 and f(dt, 24, **ff1) == 0
    for v in (1, 2, 3, 9, 24, 27, 33, 50):
        assert f(L.BF16, v, **out) == 0 and f(L.BF16, v, res=1, C2=1) == 0 and f(L.BF16, v, res=1) == 0
    for v in (1, 2, 3, 8, 9, 27, 33, 50):
        assert f(L.BF16, v, **ff1) == 0
    for bad in (dict(vec_ok=0), dict(bias=1), dict(scatter=1), dict(dup_rows=130), dict(pol=L.CP_WT), dict(pol=L.CP_NT), dict(pol_res=L.CP_NT)):
        assert f(L.BF16, 8, **out, **bad) == 0 and f(L.BF16, 8, res=1, **bad) == 0 and f(L.BF16, 24, **ff1, **bad) == 0
    assert f(L.BF16, 8, **out, ln_kind=1) == 0 and f(L.BF16, 8, **out, act=L.ACT_RELU) == 0 and f(L.BF16, 8, **out, out_is_f32=0) == 0
    assert f(L.BF16, 24, ln_kind=1, act=L.ACT_GEGLU, out_is_f32=0) == 0 and f(L.BF16, 24, **ff1, res=1) == 0
    assert f(L.BF16, 24, **ff1, C2=1) == 0 and f(L.BF16, 24, **ff1, stats_out=1) == 0
    assert f(L.BF16, 24, ln_kind=2, act=L.ACT_GEGLU, out_is_f32=1) == 0
