"""The small inference kernels of csrc/norm.hip, elementwise.hip, patch.hip and pk_cfg_mix / pk_topk_mask of sampler.hip, each called directly at the shapes
where its host code or its kernel takes another branch, and held element by element to the float64 restatements of tests/infer_glue_reference.py.  Inputs come
from that module's seeded builders; every output buffer is pre-filled with NaN (or a sentinel) and is longer and, where the entry point takes a leading
dimension, wider than the output; the checkers are the reference module's, and what they reject is shown in tests/test_infer_glue_host.py.  The branch a case
exists for is asserted from the host-visible condition, so a later change of the dispatch fails the test instead of moving the case off its branch.  Each test
records its largest error / bound through tests.util.record_parity."""
import pytest
import torch

from tests import infer_glue_reference as R
from tests.util import record_parity

pytestmark = pytest.mark.gpu

NAN = float('nan')
OK, EINVAL, EALIGN = 0, -1, -2


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    torch.cuda.set_device(0)
    yield


@pytest.fixture(scope='module')
def lib():
    from phenaki_pytorch_amd import _lib as L
    return L.load()


def stream():
    from phenaki_pytorch_amd import _lib as L
    return L.stream()


def dev(t):
    return None if t is None else t.cuda()


def ptr(t):
    return None if t is None else t.data_ptr()


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device='cuda', dtype=dtype)


def off4(t):
    """t's values in device memory that starts 4 bytes past a 16-byte boundary"""
    buf = torch.empty(t.numel() + 1, device='cuda', dtype=t.dtype)
    v = buf[1:].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == 4
    return v


# ------------------------------------------------------------------------------------------------ pk_layernorm

def _ln_launch(lib, c, x, gamma, beta, b):
    ld = c['ld']
    return lib.pk_layernorm(x.data_ptr(), ld['x'], gamma.data_ptr(), ptr(beta), R.LN_EPS, ptr(b['out']), ld['out'] if b['out'] is not None else 0, c['out_kind'],
                            ptr(b['out2']), ld['out2'] if b['out2'] is not None else 0, ptr(b['raw']), ld['raw'] if b['raw'] is not None else 0,
                            c['M'], c['D'], *c['remap'], *c['perm'], stream())


@pytest.mark.parametrize('D', R.LN_D)
def test_layernorm(lib, D):
    """<T,2> / <T,8> on both sides of D = 512, the lane-count edges, M around the 4-rows-per-block edge; out / out2 / raw, f32 / bf16, beta or none, leading
    dimensions larger than D, the grp remap with a partial last group (with and without goff) and the (pb, pc) permutation; the special rows of ln_rows"""
    worst = 0.
    for M in R.LN_M:
        for variant in R.LN_VARIANTS:
            c = R.ln_case(M, D, variant)
            assert (D <= 512) == (D in (4, 252, 256, 260, 512))                    # ln_rows_kernel<T,2> up to 512, <T,8> beyond
            x, gamma, beta = dev(c['x']), dev(c['gamma']), dev(c['beta'])
            b = R.ln_buffers(c, 'cuda')
            assert _ln_launch(lib, c, x, gamma, beta, b) == OK
            f32_out = None
            if c['out_kind'] == 1 and 'out2' not in c['outs']:                    # a bf16 out alone: against the f32 launch of the same case
                c32 = dict(c, out_kind=0)
                b32 = R.ln_buffers(c32, 'cuda')
                assert _ln_launch(lib, c32, x, gamma, beta, b32) == OK
                worst = max(worst, R.ln_check(c32, b32['out'], b32['out2'], b32['raw']))
                f32_out = R.region(b32['out'], c['orows'], D, 'layernorm f32 launch')
            ratio = R.ln_check(c, b['out'], b['out2'], b['raw'], f32_out=f32_out)
            worst = max(worst, ratio)
            record_parity('infer_glue_layernorm', dict(shape=[M, D], branch=('<T,2>' if D <= 512 else '<T,8>') + f', {(M + 3) // 4} blocks', outputs=variant[0],
                                                       out_kind=variant[1], beta=variant[2], wide=variant[3], rows=c['mapk'], err_over_bound=ratio))
    print(f'layernorm D {D}: err / bound {worst:.3f}')


def test_layernorm_refusals(lib):
    x, g = nan(8, 2052), nan(2052)
    o = nan(8, 2052)
    call = lambda M, D, ld, remap, perm: lib.pk_layernorm(x.data_ptr(), ld, g.data_ptr(), None, R.LN_EPS, o.data_ptr(), ld, 0, None, 0, None, 0, M, D, *remap, *perm, stream())
    assert call(4, 2052, 2052, (0, 0, 0), (0, 0)) == EINVAL
    assert call(4, 512, 512, (2, 2, 0), (2, 2)) == EINVAL
    assert call(5, 512, 512, (0, 0, 0), (2, 2)) == EINVAL
    assert call(4, 6, 8, (0, 0, 0), (0, 0)) == EALIGN
    torch.cuda.synchronize()
    R.assert_untouched(o, 'a refused pk_layernorm')


# ------------------------------------------------------------------------------------------------ pk_layernorm_lfq

@pytest.mark.parametrize('case', R.LNLFQ_CASES, ids=lambda c: f'{c[0]}x{c[1]}cd{c[2]}{"b" if c[3] else ""}{"t" if c[4] else ""}{"p" if c[5] else ""}{"T" if c[6] else ""}')
def test_layernorm_lfq(lib, case):
    """<2,1>, <8,1> and the two-rows-per-wave <2,2> (even and odd M: the clamped tail row), cd 1 ... 16 through the halving butterfly"""
    c = R.lnlfq_case(*case)
    M, D, cd = c['M'], c['D'], c['cd']
    branch = '<2,2>' if (D <= 512 and M >= 32768) else ('<2,1>' if D <= 512 else '<8,1>')
    assert branch == case[7], 'the case is off the branch it exists for'
    x, gamma, beta, wp, bp = dev(c['x']), dev(c['gamma']), dev(c['beta']), dev(c['wp']), dev(c['bp'])
    ids, tok, proj = R.lnlfq_buffers(c, 'cuda')
    rc = lib.pk_layernorm_lfq(x.data_ptr(), D + 4, gamma.data_ptr(), ptr(beta), R.LN_EPS, wp.data_ptr(), bp.data_ptr(), ids.data_ptr(), ptr(tok), c['ldt'] if tok is not None else 0,
                              ptr(proj), M, D, cd, *c['perm'], stream())
    assert rc == OK
    out = R.lnlfq_check(c, ids, tok, proj)
    print(f'layernorm_lfq {M}x{D} cd {cd} {branch}: err / bound {out}')
    record_parity('infer_glue_layernorm_lfq', dict(shape=[M, D, cd], branch=branch, perm=list(c['perm']), err_over_bound=out))


def test_layernorm_lfq_refusal(lib):
    c = R.lnlfq_case(5, 64, 16, True, False, False, False)
    x, gamma, wp = dev(c['x']), dev(c['gamma']), nan(17, 64)
    bp = nan(17)
    ids = torch.full((7,), R.SENTINEL, device='cuda', dtype=torch.int64)
    assert lib.pk_layernorm_lfq(x.data_ptr(), 68, gamma.data_ptr(), None, R.LN_EPS, wp.data_ptr(), bp.data_ptr(), ids.data_ptr(), None, 0, None, 5, 64, 17, 0, 0, stream()) == EINVAL
    assert (ids.cpu() == R.SENTINEL).all()


# ------------------------------------------------------------------------------------------------ pk_lfq_encode

@pytest.mark.parametrize('D', R.LFQ_ENC_D)
def test_lfq_encode(lib, D):
    """every instantiated cd at every M; rows wider than D; with and without the projections"""
    worst = 0.
    for M in R.LFQ_ENC_M:
        for cd in R.LFQ_ENC_CD:
            c = R.lfq_enc_case(M, D, cd)
            x, wp, bp = dev(c['x']), dev(c['wp']), dev(c['bp'])
            for with_proj in (True, False):
                ids, proj = R.lfq_enc_buffers(c, 'cuda')
                assert lib.pk_lfq_encode(x.data_ptr(), D + 4, wp.data_ptr(), bp.data_ptr(), ids.data_ptr(), proj.data_ptr() if with_proj else None, M, D, cd, stream()) == OK
                ratio = R.lfq_enc_check(c, ids, proj if with_proj else None)
                if with_proj:
                    worst = max(worst, ratio)
                    record_parity('infer_glue_lfq_encode', dict(shape=[M, D, cd], branch=f'lfq_encode_kernel<{cd}>', err_over_bound=ratio))
                else:
                    R.assert_untouched(proj, 'lfq_encode proj = NULL')
    print(f'lfq_encode D {D}: err / bound {worst:.3f}')


def test_lfq_encode_refusals(lib):
    c = R.lfq_enc_case(5, 64, 18)
    x, wp, bp = dev(c['x']), nan(20, 64), nan(20)
    ids, proj = R.lfq_enc_buffers(c, 'cuda')
    for cd in (5, 20):
        assert lib.pk_lfq_encode(x.data_ptr(), 68, wp.data_ptr(), bp.data_ptr(), ids.data_ptr(), None, 5, 64, cd, stream()) == EINVAL
    assert (ids.cpu() == R.SENTINEL).all()


# ------------------------------------------------------------------------------------------------ pk_lfq_decode

@pytest.mark.parametrize('case', R.DECODE_CASES, ids=lambda c: f'{c[0]}x{c[1]}cd{c[2]}{"P" if c[3] else ""}{"T" if c[4][0] else ""}{c[5] or ""}-{c[6]}')
def test_lfq_decode(lib, case):
    """the register-resident kernel and the generic one, bit for bit against the f32 restatement; a fast-eligible shape with bo, wo or out 4 bytes off its
    alignment takes the generic kernel and gives the same bits"""
    c = R.decode_case(*case)
    M, D, cd, mis = c['M'], c['D'], c['cd'], c['misalign']
    wo = off4(c['wo']) if mis == 'wo' else dev(c['wo'])
    bo = off4(c['bo']) if mis == 'bo' else dev(c['bo'])
    out = off4(R.nan_buffer(M + R.GUARD, D)) if mis == 'out' else nan(M + R.GUARD, D)
    fast = R.decode_fast(D, cd, out.data_ptr(), bo.data_ptr(), wo.data_ptr())
    assert fast == (case[6] == 'fast'), 'the case is off the kernel it exists for'
    if mis:
        assert R.decode_fast(D, cd, 0, 0, 0)
    ids, ids_prime = dev(c['ids']), dev(c['ids_prime'])
    n_prime, n = (ids_prime.shape[1], ids.shape[1]) if ids_prime is not None else (0, 0)
    assert lib.pk_lfq_decode(ids.data_ptr(), wo.data_ptr(), bo.data_ptr(), out.data_ptr(), M, D, cd, ptr(ids_prime), n_prime, n, *c['perm'], stream()) == OK
    R.decode_check(c, out)
    if D == 512 and M == 1025:
        assert (M + 1) // 2 > 512                                 # more row pairs than the 512 blocks: the row loop takes a second pass
    record_parity('infer_glue_lfq_decode', dict(shape=[M, D, cd], branch=case[6] + (f' ({mis} + 4 bytes)' if mis else ''), prime=bool(case[3]), perm=list(c['perm']),
                                                err_over_bound=0., exact=True))


def test_lfq_decode_refusals(lib):
    c = R.decode_case(12, 128, 16, (2, 2, 4), (0, 0))
    ids, ids_prime, wo, bo, out = dev(c['ids']), dev(c['ids_prime']), nan(128, 63), dev(c['bo']), nan(14, 128)
    assert lib.pk_lfq_decode(ids.data_ptr(), wo.data_ptr(), bo.data_ptr(), out.data_ptr(), 12, 128, 63, None, 0, 0, 0, 0, stream()) == EINVAL
    assert lib.pk_lfq_decode(ids.data_ptr(), wo.data_ptr(), bo.data_ptr(), out.data_ptr(), 11, 128, 16, ids_prime.data_ptr(), 2, 4, 0, 0, stream()) == EINVAL
    torch.cuda.synchronize()
    R.assert_untouched(out, 'a refused pk_lfq_decode')


# ------------------------------------------------------------------------------------------------ pk_peg

def _peg(lib, c, with_t=True):
    B, T, H, W, D = c['shape']
    x, wt, bias = dev(c['x']), dev(c['wt']), dev(c['bias'])
    out, out_t = R.peg_buffers(c, 'cuda', with_t)
    assert lib.pk_peg(x.data_ptr(), wt.data_ptr(), bias.data_ptr(), out.data_ptr(), ptr(out_t), B, T, H, W, D, 1 if c['causal'] else 0, stream()) == OK
    return R.peg_check(c, out, out_t)


@pytest.mark.parametrize('causal', [False, True])
@pytest.mark.parametrize('W', R.PEG_W)
def test_peg(lib, W, causal):
    """peg_row_kernel<4|8|16> and the generic kernel (every other width) at T in {1, 2, 5} (shorter than the causal front pad), H in {1, 2, 8},
    D in {4, 132, 512}, two sequences at different offsets; out_t against the rounding of out"""
    worst = 0.
    for T, H, D in R.PEG_THD:
        ratio = _peg(lib, R.peg_case(2, T, H, W, D, causal))
        worst = max(worst, ratio)
        record_parity('infer_glue_peg', dict(shape=[2, T, H, W, D], causal=causal, branch=f'peg_row_kernel<{W}>' if W in (4, 8, 16) else 'peg_kernel', err_over_bound=ratio))
    print(f'peg W {W} causal {causal}: err / bound {worst:.3f}')


@pytest.mark.parametrize('shape,blocks', R.PEG_BLOCKS)
def test_peg_row_kernel_block_counts(lib, shape, blocks):
    """1, 7 and 9 blocks of work on a grid padded to a multiple of 8 and walked in XCD-contiguous order"""
    B, T, H, W, D = shape
    assert W in (4, 8, 16) and (B * T * H * (D // 4) + 255) // 256 == blocks
    worst = max(_peg(lib, R.peg_case(*shape, causal), with_t=causal) for causal in (False, True))
    record_parity('infer_glue_peg', dict(shape=list(shape), branch=f'peg_row_kernel<{W}>, {blocks} blocks', err_over_bound=worst))


def test_peg_generic_kernel_second_pass(lib):
    B, T, H, W, D = R.PEG_BIG
    assert W not in (4, 8, 16) and B * T * H * W * (D // 4) > 16384 * 256
    worst = _peg(lib, R.peg_case(B, T, H, W, D, True), with_t=False)
    record_parity('infer_glue_peg', dict(shape=list(R.PEG_BIG), branch='peg_kernel, second grid-stride pass', err_over_bound=worst))


def test_peg_refusals(lib):
    x, wt, bias, out = nan(2 * 8 * 8), nan(27 * 8), nan(8), nan(2 * 8 * 8)
    assert lib.pk_peg(x.data_ptr(), wt.data_ptr(), bias.data_ptr(), x.data_ptr(), None, 1, 1, 2, 4, 8, 0, stream()) == EINVAL
    assert lib.pk_peg(x.data_ptr(), wt.data_ptr(), bias.data_ptr(), out.data_ptr(), None, 1, 1, 2, 4, 6, 0, stream()) == EALIGN
    torch.cuda.synchronize()
    R.assert_untouched(out, 'a refused pk_peg')


# ------------------------------------------------------------------------------------------------ pk_embed

def _embed(lib, c, with_t=True):
    rows = c['S'] * (c['n_prime'] + c['n'])
    out, out_t = nan(rows + R.GUARD, c['D']), (nan(rows + R.GUARD, c['D'], dtype=torch.bfloat16) if with_t else None)
    ids, ids_prime, tok, pos = dev(c['ids']), dev(c['ids_prime']), dev(c['tok']), dev(c['pos'])
    assert lib.pk_embed(ptr(ids_prime), c['n_prime'], ids.data_ptr(), c['n'], c['nb'], tok.data_ptr(), pos.data_ptr(), out.data_ptr(), ptr(out_t), c['S'], c['D'], stream()) == OK
    R.embed_check(c, out, out_t)


@pytest.mark.parametrize('case', R.EMBED_CASES + [R.EMBED_BIG])
def test_embed(lib, case):
    """pos + tok, one rounded add, bit for bit; ids 0 and V - 1; S = 2 nb replicas reading the same id rows; primed ids; the last case takes a second
    grid-stride pass"""
    c = R.embed_case(*case)
    big = c['S'] * (c['n_prime'] + c['n']) * (c['D'] // 4) > 16384 * 256
    assert big == (case == R.EMBED_BIG)
    _embed(lib, c, with_t=not big)
    record_parity('infer_glue_embed', dict(shape=list(case), branch='second grid-stride pass' if big else 'one pass', err_over_bound=0., exact=True))


# ------------------------------------------------------------------------------------------------ pk_cfg_mix

def _cfg(lib, c):
    x, rows = dev(c['x']), dev(c['rows'])
    f32 = None
    ratio = 0.
    for t in (torch.float32, torch.bfloat16):
        out = nan(c['nrows'] + R.GUARD, c['ldo'], dtype=t)
        assert lib.pk_cfg_mix(x.data_ptr(), x.shape[1], c['nb'], c['n_tot'], c['n_prime'], ptr(rows), c['nrows'], c['scale'], c['has_null'], out.data_ptr(), c['ldo'],
                              1 if t == torch.float32 else 0, c['D'], stream()) == OK
        r, got = R.cfg_check(c, out, f32_out=f32)
        if t == torch.float32:
            ratio, f32 = r, got
    return ratio


@pytest.mark.parametrize('case', R.CFG_CASES)
def test_cfg_mix(lib, case):
    c = R.cfg_case(*case)
    ratio = _cfg(lib, c)
    record_parity('infer_glue_cfg_mix', dict(shape=list(case), branch='one pass', err_over_bound=ratio))


def test_cfg_mix_second_pass(lib):
    nb, n_tot, n_prime, D, has_null, nrows, scale = R.CFG_BIG
    assert nrows * (D // 4) > 16384 * 256
    c = R.cfg_case(nb, n_tot, n_prime, D, has_null, True, scale, False, nrows=nrows)
    x, rows = dev(c['x']), dev(c['rows'])
    out = nan(nrows + R.GUARD, D)
    assert lib.pk_cfg_mix(x.data_ptr(), D, nb, n_tot, n_prime, rows.data_ptr(), nrows, scale, has_null, out.data_ptr(), D, 1, D, stream()) == OK
    ratio, _ = R.cfg_check(c, out)
    record_parity('infer_glue_cfg_mix', dict(shape=list(R.CFG_BIG), branch='second grid-stride pass', err_over_bound=ratio))


# ------------------------------------------------------------------------------------------------ pk_critic_head

@pytest.mark.parametrize('D', R.CRITIC_D)
def test_critic_head(lib, D):
    """5 output rows (a partial block) at the lane-count edges of D; u given, hash noise (seed by value + device word), no noise; with and without the null
    half, the primed positions and the bias"""
    for has_null, n_prime, has_b, noise in [(1, 0, True, 'u'), (0, 2, False, 'hash'), (1, 3, True, 'none'), (1, 0, False, 'hash'), (0, 0, True, 'u'), (0, 1, True, 'none')]:
        c = R.critic_case(D, has_null, n_prime, has_b, noise)
        x, w, b, u = dev(c['x']), dev(c['w']), dev(c['b']), dev(c['u'])
        sd = torch.tensor([R.CRITIC_SEED_DEV], device='cuda', dtype=torch.int64) if noise == 'hash' else None
        out = nan(5 + R.GUARD)
        assert lib.pk_critic_head(x.data_ptr(), D + 4, w.data_ptr(), ptr(b), D, c['nb'], c['n_tot'], n_prime, has_null, c['scale'], ptr(u), c['noise_mult'],
                                  R.CRITIC_SEED if noise == 'hash' else 0, ptr(sd), out.data_ptr(), stream()) == OK
        ratio = R.critic_check(c, out)
        record_parity('infer_glue_critic_head', dict(shape=[c['nb'], c['n_tot'], n_prime, D], branch='partial block', has_null=has_null, bias=has_b, noise=noise, err_over_bound=ratio))


# ------------------------------------------------------------------------------------------------ pk_topk_mask

@pytest.mark.parametrize('n', R.TOPK_N)
def test_topk_mask(lib, n):
    """rows of ties (all equal, -1e4 everywhere but a few, 0.0 with -0.0, +-inf) and a random row, at k in {0, 1, n - 1, n}: mask, ids, the rank order of
    rows_out and scores_next exactly, each beside guards"""
    for k in sorted({0, 1, n - 1, n}):
        c = R.topk_case(n, k)
        scores = dev(c['scores'])
        mask, ids, rows_out, nxt = R.topk_buffers(c, 'cuda')
        assert lib.pk_topk_mask(scores.data_ptr(), c['B'], n, k, R.TOPK_MASK_ID, mask.data_ptr(), ids.data_ptr(), rows_out.data_ptr(), nxt.data_ptr(), stream()) == OK
        R.topk_check(c, mask, ids, rows_out, nxt)
        record_parity('infer_glue_topk_mask', dict(shape=[len(R.TOPK_KINDS), n], k=k, branch=f'{(n + 63) // 64} position blocks, quarter {(n + 3) >> 2}', err_over_bound=0., exact=True))


def test_topk_mask_refusals(lib):
    c = R.topk_case(5, 2)
    scores = nan(12289)
    mask, ids, rows_out, nxt = R.topk_buffers(c, 'cuda')
    assert lib.pk_topk_mask(scores.data_ptr(), 1, 12289, 2, 1, mask.data_ptr(), ids.data_ptr(), rows_out.data_ptr(), None, stream()) == EINVAL
    assert lib.pk_topk_mask(scores.data_ptr(), 1, 5, 2, 1, mask.data_ptr(), ids.data_ptr(), rows_out.data_ptr(), scores.data_ptr(), stream()) == EINVAL
    assert (mask.cpu() == 7).all() and (rows_out.cpu() == R.SENTINEL).all()


# ------------------------------------------------------------------------------------------------ pk_rmsnorm, pk_l2norm_rows, pk_gated_gelu_tanh

def _rows_launch(call, c, ref, what, zero_rows):
    """f32 launch against the float64 bound, bf16 launch against the rounding of the f32 launch"""
    f32, ratio = None, 0.
    for kind, t in ((0, torch.float32), (1, torch.bfloat16)):
        out = nan(c['M'] + R.GUARD, c['ldo'], dtype=t)
        assert call(out, kind) == OK
        r, got = R.rows_check(c, out, ref, what, f32_out=f32, zero_rows=zero_rows)
        if kind == 0:
            ratio, f32 = r, got
    return ratio


@pytest.mark.parametrize('D', R.ROW_D)
def test_rmsnorm(lib, D):
    """rows of magnitude 1e-3 (mean square about eps), 1 and 1e4; rowmask NULL and with zeros (those rows +0.0 bit for bit); f32 and bf16; ldx, ldo > D"""
    for M in R.ROW_M:
        for masked in (False, True):
            c = R.rms_case(M, D, masked)
            x, w, rm = dev(c['x']), dev(c['w']), dev(c['rowmask'])
            call = lambda out, kind: lib.pk_rmsnorm(x.data_ptr(), D + 4, w.data_ptr(), R.RMS_EPS, ptr(rm), out.data_ptr(), c['ldo'], kind, M, D, stream())
            ratio = _rows_launch(call, c, R.rms_ref(c), 'rmsnorm', R.rms_zero_rows(c))
            record_parity('infer_glue_rmsnorm', dict(shape=[M, D], branch=f'{(D + 255) // 256} column passes', rowmask=masked, err_over_bound=ratio))


@pytest.mark.parametrize('D', R.ROW_D)
def test_l2norm_rows(lib, D):
    """row norms over 1e-6 ... 1e6 and an exact zero row (exact zeros out); f32 and bf16; ldx, ldo > D"""
    for M in R.ROW_M:
        c = R.l2_case(M, D)
        x = dev(c['x'])
        call = lambda out, kind: lib.pk_l2norm_rows(x.data_ptr(), D + 4, out.data_ptr(), c['ldo'], kind, M, D, stream())
        ratio = _rows_launch(call, c, R.l2_ref(c), 'l2norm_rows', R.l2_zero_rows(c))
        record_parity('infer_glue_l2norm_rows', dict(shape=[M, D], branch=f'{(D + 255) // 256} column passes', err_over_bound=ratio))


@pytest.mark.parametrize('Fd', R.ROW_D)
def test_gated_gelu_tanh(lib, Fd):
    """gate values across [-20, 20] with 0.0, -0.0 and +-1e4; held to GELU_C U (|y| + |a b|), the kernel's own ratio on record"""
    worst = 0.
    for M in R.ROW_M:
        c = R.gelu_case(M, Fd)
        h = dev(c['h'])
        call = lambda out, kind: lib.pk_gated_gelu_tanh(h.data_ptr(), 2 * Fd + 4, out.data_ptr(), c['ldo'], kind, M, Fd, stream())
        ratio = _rows_launch(call, c, R.gelu_ref(c), 'gated_gelu_tanh', None)
        worst = max(worst, ratio)
        record_parity('infer_glue_gated_gelu_tanh', dict(shape=[M, Fd], branch='one pass', err_over_bound=ratio, err_over_U_scale=ratio * R.GELU_C,
                                                         cpu_f32_err_over_U_scale=R.GELU_CPU_RATIO))
    print(f'gated_gelu_tanh F {Fd}: err / bound {worst:.3f} = {worst * R.GELU_C:.3f} U scale (the CPU evaluation: {R.GELU_CPU_RATIO})')


def test_gated_gelu_tanh_second_pass(lib):
    M, Fd = 4100, 4096
    assert M * (Fd // 4) > 16384 * 256
    c = R.gelu_case(M, Fd)
    h = dev(c['h'])
    out = nan(M + R.GUARD, c['ldo'])
    assert lib.pk_gated_gelu_tanh(h.data_ptr(), 2 * Fd + 4, out.data_ptr(), c['ldo'], 0, M, Fd, stream()) == OK
    ratio, _ = R.rows_check(c, out, R.gelu_ref(c), 'gated_gelu_tanh')
    record_parity('infer_glue_gated_gelu_tanh', dict(shape=[M, Fd], branch='second grid-stride pass', err_over_bound=ratio, err_over_U_scale=ratio * R.GELU_C))


def test_row_kernel_refusals(lib):
    x, w, out = nan(4 * 72 + 4), nan(64), nan(6, 64)
    mis = x[1:]
    assert mis.data_ptr() % 16 == 4
    assert lib.pk_rmsnorm(mis.data_ptr(), 64, w.data_ptr(), R.RMS_EPS, None, out.data_ptr(), 64, 0, 4, 64, stream()) == EALIGN
    assert lib.pk_l2norm_rows(mis.data_ptr(), 64, out.data_ptr(), 64, 0, 4, 64, stream()) == EALIGN
    assert lib.pk_gated_gelu_tanh(mis.data_ptr(), 64, out.data_ptr(), 64, 0, 4, 32, stream()) == EALIGN
    assert lib.pk_gated_gelu_tanh(x.data_ptr(), 60, out.data_ptr(), 64, 0, 4, 32, stream()) == EINVAL
    torch.cuda.synchronize()
    R.assert_untouched(out, 'a refused row kernel')


# ------------------------------------------------------------------------------------------------ pk_patchify_ln / pk_unpatchify

def _patchify(lib, c, video, weight, bias, out, kind):
    B, C, Fr, H, W, f0, nt, pt, ph, pw = c['geom']
    return lib.pk_patchify_ln(video.data_ptr(), B, C, Fr, H, W, f0, nt, pt, ph, pw, ptr(weight), ptr(bias), R.LN_EPS, out.data_ptr(), c['ldo'], kind, stream())


@pytest.mark.parametrize('geom', R.PATCH_CASES, ids=lambda g: f'P{R.patch_P(g)}')
def test_patchify_ln(lib, geom):
    """P = 4, the narrow template's end (P / 4 = 1024), the wide one's start (1028) and end (8192); f0 > 0; ldo > P; raw rows; bf16 against the f32 launch"""
    c = R.patch_case(geom)
    P = c['P']
    branch = 'VMAX 4' if P // 4 <= 1024 else 'VMAX 8'
    assert {4: 'VMAX 4', 96: 'VMAX 4', 4096: 'VMAX 4', 4112: 'VMAX 8', 8192: 'VMAX 8'}[P] == branch and geom[5] > 0
    video, weight, bias = dev(c['video']), dev(c['weight']), dev(c['bias'])
    ratio = 0.
    for with_ln in (True, False):
        f32 = None
        for kind, t in ((0, torch.float32), (1, torch.bfloat16)):
            out = nan(c['rows'] + R.GUARD, c['ldo'], dtype=t)
            assert _patchify(lib, c, video, weight if with_ln else None, bias if with_ln else None, out, kind) == OK
            r, got = R.patch_check(c, out, with_ln, f32_out=f32)
            if kind == 0:
                ratio, f32 = max(ratio, r), got
    record_parity('infer_glue_patchify_ln', dict(shape=list(geom), P=P, branch=branch, err_over_bound=ratio))


@pytest.mark.parametrize('geom', R.PATCH_CASES + [R.UNPATCH_BIG], ids=lambda g: f'P{R.patch_P(g)}x{R.patch_rows(g)}')
def test_unpatchify(lib, geom):
    """a copy into a NaN-filled video: the frames outside [f0, f0 + nt pt) stay NaN; ldp > P; the last case has more than 8192 blocks' worth of vectors"""
    c = R.unpatch_case(geom)
    B, C, Fr, H, W, f0, nt, pt, ph, pw = geom
    big = c['rows'] * (c['P'] // 4) > 8192 * 256
    assert big == (geom == R.UNPATCH_BIG)
    pix, video = dev(c['pix']), nan(B, C, Fr, H, W)
    assert lib.pk_unpatchify(pix.data_ptr(), c['P'] + 4, video.data_ptr(), B, C, Fr, H, W, f0, nt, pt, ph, pw, stream()) == OK
    R.unpatch_check(c, video)
    record_parity('infer_glue_unpatchify', dict(shape=list(geom), branch='second grid-stride pass' if big else 'one pass', err_over_bound=0., exact=True))


def test_patchify_refusals(lib):
    video, w, out = nan(1, 1, 1, 513, 16), nan(8208), nan(4, 8216)
    call = lambda H, W, ph, pw, weight, bias: lib.pk_patchify_ln(video.data_ptr(), 1, 1, 1, H, W, 0, 1, 1, ph, pw, ptr(weight), ptr(bias), R.LN_EPS, out.data_ptr(), 8216, 0, stream())
    assert call(513, 16, 513, 16, w, w) == EINVAL                 # P = 8208
    assert call(8, 16, 8, 16, w, None) == EINVAL                  # weight without bias
    assert call(8, 12, 8, 6, w, w) == EALIGN
    torch.cuda.synchronize()
    R.assert_untouched(out, 'a refused pk_patchify_ln')


# ------------------------------------------------------------------------------------------------ pk_cpb_input

@pytest.mark.parametrize('dims,D', R.CPB_CASES + [R.CPB_BIG])
def test_cpb_input(lib, dims, D):
    c = R.cpb_case(dims, D)
    total = c['n'] * c['n'] * D
    big = total > 16384 * 256
    assert big == ((dims, D) == R.CPB_BIG)
    w0, b0, out = dev(c['w0']), dev(c['b0']), nan(total + R.GUARD)
    d = (1,) * (3 - len(dims)) + tuple(dims)
    assert lib.pk_cpb_input(w0.data_ptr(), b0.data_ptr(), out.data_ptr(), *d, len(dims), D, stream()) == OK
    ratio = R.cpb_check(c, out)
    print(f'cpb_input {dims} D {D}: err / bound {ratio:.3f} = {ratio * R.CPB_C:.3f} U scale (the CPU evaluation: {R.CPB_CPU_RATIO})')
    record_parity('infer_glue_cpb_input', dict(shape=[list(dims), D], branch='second grid-stride pass' if big else 'one pass', err_over_bound=ratio,
                                               err_over_U_scale=ratio * R.CPB_C, cpu_f32_err_over_U_scale=R.CPB_CPU_RATIO))
