"""The discriminator's kernels (csrc/conv.hip), each called directly through its _lib wrapper and held element by element to the float64 restatements of
tests/gan_kernels_reference.py: pk_row_softmax, pk_row_l2scale (modes 0, 1, 2 each), pk_row_ln_bwd2, pk_bmm, pk_im2col / pk_col2im, pk_nchw_to_rows /
pk_rows_to_nchw, pk_pick_frames, and the rungs of discriminator._mm_raw.  The autograd Functions built on the row kernels (_Softmax, _SoftmaxBwd, _L2Scale,
_L2ScaleBwd, _GammaLayerNorm, _GammaLayerNormBwd) are driven through torch.autograd.grad with chosen upstreams, which pins the order of their returned
gradients and the column sums of the per-row contributions.  Inputs come from seeded CPU generators; every output buffer is pre-filled with NaN and carries a
guard row or pad columns, so an element that was not written and an element written outside the output both show.  The checkers are the reference module's;
what they reject is shown in tests/test_gan_kernels_host.py.  Each test records its largest error / bound through tests.util.record_parity."""
import itertools

import pytest
import torch

from tests import gan_kernels_reference as R
from tests.util import record_parity

pytestmark = pytest.mark.gpu

NAN = R.NAN


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    torch.cuda.set_device(0)
    with torch.enable_grad():
        yield


def dev(t):
    return None if t is None else t.cuda()


def guarded(M, n):
    """(an (M, n) output inside a NaN-filled buffer, that buffer's guard row behind it)"""
    buf = torch.full((M + 1, n), NAN, device='cuda')
    return buf[:M], buf[M:]


def merge(worst, new):
    for k, v in new.items():
        worst[k] = max(worst.get(k, 0.), v)


def leaf(t):
    return t.cuda().requires_grad_(True)


# ------------------------------------------------------------------------------------------------ pk_row_softmax

@pytest.mark.parametrize('M,n', R.SOFTMAX_SHAPES)
def test_row_softmax_every_mode(M, n):
    from phenaki_pytorch_amd import _lib as L
    from phenaki_pytorch_amd.discriminator import _Softmax, _SoftmaxBwd
    worst = {}
    for data in R.SOFTMAX_DATA:
        c = R.softmax_case(M, n, data)
        x, y, dy, cc = (dev(c[k]) for k in ('x', 'y', 'dy', 'c'))
        outs, guards = {}, []
        for k, args, mode in (('y0', (x, None, None), 0), ('b1', (y, dy, None), 1), ('g_y', (y, dy, cc), 2), ('g_dy', (y, cc, None), 1)):
            o, g = guarded(M, n)
            L.row_softmax(*args, o, mode)
            outs[k] = o.cpu()
            guards.append(g)
        for g in guards:
            R.assert_untouched(g, f'row_softmax {data}: the row behind the output')
        merge(worst, R.softmax_check(c, outs))
        # the Functions: _SoftmaxBwd at the case's y returns (mode 1) and, differentiated at upstream c, (mode 2, mode 1 at c) in that order
        yl, dyl = leaf(c['y']), leaf(c['dy'])
        b1 = _SoftmaxBwd.apply(yl, dyl)
        g_y, g_dy = torch.autograd.grad(b1, (yl, dyl), cc)
        for k, t in (('b1', b1), ('g_y', g_y), ('g_dy', g_dy)):
            R.assert_same_bits(t.detach().cpu(), outs[k], f'_SoftmaxBwd {k} against the direct call')
        # _Softmax: the forward is mode 0, its backward is _SoftmaxBwd at ITS output
        xl = leaf(c['x'])
        y0 = _Softmax.apply(xl)
        R.assert_same_bits(y0.detach().cpu(), outs['y0'], '_Softmax forward against the direct call')
        dx, = torch.autograd.grad(y0, xl, dy, create_graph=True)
        R.assert_same_bits(dx.detach().cpu(), L.row_softmax(y0.detach(), dy, None, torch.empty_like(x), 1).cpu(), '_Softmax backward')
        # the second derivative through the whole chain (mode 2 and mode 1 at the kernel's own y0) against float64 autograd of x.softmax(-1)
        hx, = torch.autograd.grad(dx, xl, cc)
        merge(worst, R.softmax_check(c, dict(hx=hx.cpu())))
    print(f'row_softmax {M}x{n}: err / bound {worst}')
    record_parity('gan_row_softmax', dict(shape=[M, n], err_over_bound=worst))


# ------------------------------------------------------------------------------------------------ pk_row_l2scale

@pytest.mark.parametrize('M,d', R.L2_SHAPES)
def test_row_l2scale_every_mode(M, d):
    from phenaki_pytorch_amd import _lib as L
    from phenaki_pytorch_amd.discriminator import _L2Scale, _L2ScaleBwd
    worst = {}
    for c in R.l2_cases(M, d):
        x, sc, dz, gx, gsc = (dev(c[k]) for k in ('x', 'sc', 'dz', 'gx', 'gsc'))
        names = ('z', 'dx', 'dsc_rows', 'grad_x', 'grad_sc_rows', 'grad_dz')
        o = {k: guarded(M, d) for k in names}
        L.row_l2scale(x, sc, None, None, None, o['z'][0], None, None, 0)
        L.row_l2scale(x, sc, dz, None, None, o['dx'][0], o['dsc_rows'][0], None, 1)
        L.row_l2scale(x, sc, dz, gx, gsc, o['grad_x'][0], o['grad_sc_rows'][0], o['grad_dz'][0], 2)
        outs = {k: v[0].cpu() for k, v in o.items()}
        for k, v in o.items():
            R.assert_untouched(v[1], f'row_l2scale {k}: the row behind the output')
        # the Functions: _L2ScaleBwd returns (dx, dsc) and, differentiated at upstreams (gx, gsc), (grad_x, grad_sc, grad_dz) in that order
        xl, scl, dzl = leaf(c['x']), leaf(c['sc']), leaf(c['dz'])
        dx, dsc = _L2ScaleBwd.apply(xl, scl, dzl)
        grad_x, grad_sc, grad_dz = torch.autograd.grad((dx, dsc), (xl, scl, dzl), (gx, gsc))
        for k, t in (('dx', dx), ('grad_x', grad_x), ('grad_dz', grad_dz)):
            R.assert_same_bits(t.detach().cpu(), outs[k], f'_L2ScaleBwd {k} against the direct call')
        merge(worst, R.l2_check(c, outs, dsc=dsc.detach().cpu(), grad_sc=grad_sc.cpu()))
        # _L2Scale: the forward is mode 0, its backward is _L2ScaleBwd at (x, sc, dz)
        z = _L2Scale.apply(xl, scl)
        R.assert_same_bits(z.detach().cpu(), outs['z'], '_L2Scale forward against the direct call')
        dx2, dsc2 = torch.autograd.grad(z, (xl, scl), dzl, create_graph=True)
        R.assert_same_bits(dx2.detach().cpu(), outs['dx'], '_L2Scale backward dx')
        R.assert_same_bits(dsc2.detach().cpu(), dsc.detach().cpu(), '_L2Scale backward dsc')
        h = torch.autograd.grad((dx2, dsc2), (xl, scl, dzl), (gx, gsc))
        for t, want, k in zip(h, (grad_x, grad_sc, grad_dz), ('grad_x', 'grad_sc', 'grad_dz')):
            R.assert_same_bits(t.cpu(), want.cpu(), f'_L2Scale second order {k}')
    print(f'row_l2scale {M}x{d}: err / bound {worst}')
    record_parity('gan_row_l2scale', dict(shape=[M, d], err_over_bound=worst))


# ------------------------------------------------------------------------------------------------ pk_row_ln_bwd2

@pytest.mark.parametrize('M,D', R.LN_SHAPES)
@pytest.mark.parametrize('eps', R.LN_EPS)
def test_row_ln_bwd2(M, D, eps):
    from phenaki_pytorch_amd import _lib as L
    from phenaki_pytorch_amd.discriminator import _GammaLayerNorm, _GammaLayerNormBwd
    worst = {}
    for c in R.ln_cases(M, D):
        x, gamma, dy, u, w = (dev(c[k]) for k in ('x', 'gamma', 'dy', 'u', 'w'))
        o = {k: guarded(M, D) for k in ('grad_x', 'grad_gamma_rows', 'grad_dy')}
        L.row_ln_bwd2(x, gamma, dy, u, w, eps, o['grad_x'][0], o['grad_gamma_rows'][0], o['grad_dy'][0])
        outs = {k: v[0].cpu() for k, v in o.items()}
        for k, v in o.items():
            R.assert_untouched(v[1], f'row_ln_bwd2 {k}: the row behind the output')
        if D % 4:
            # pk_layernorm / pk_layernorm_bwd take D % 4 == 0 only: the Functions cannot be built at this width, the column sum is the one they would launch
            grad_gamma = L.colsum(o['grad_gamma_rows'][0], M, D, torch.full((D,), NAN, device='cuda'))
        else:
            # _GammaLayerNormBwd differentiated at upstreams (u, w) returns (grad_x, grad_gamma, grad_dy, None) in that order
            xl, gl, dyl = leaf(c['x']), leaf(c['gamma']), leaf(c['dy'])
            dx, dg = _GammaLayerNormBwd.apply(xl, gl, dyl, eps)
            grad_x, grad_gamma, grad_dy = torch.autograd.grad((dx, dg), (xl, gl, dyl), (u, w))
            R.assert_same_bits(grad_x.cpu(), outs['grad_x'], '_GammaLayerNormBwd grad_x against the direct call')
            R.assert_same_bits(grad_dy.cpu(), outs['grad_dy'], '_GammaLayerNormBwd grad_dy against the direct call')
            # _GammaLayerNorm: its backward is _GammaLayerNormBwd at (x, gamma, dy, eps)
            y = _GammaLayerNorm.apply(xl, gl, torch.zeros_like(gamma), eps)
            dx2, dg2 = torch.autograd.grad(y, (xl, gl), dyl, create_graph=True)
            R.assert_same_bits(dx2.detach().cpu(), dx.detach().cpu(), '_GammaLayerNorm backward dx')
            R.assert_same_bits(dg2.detach().cpu(), dg.detach().cpu(), '_GammaLayerNorm backward dgamma')
            h = torch.autograd.grad((dx2, dg2), (xl, gl, dyl), (u, w))
            for t, want, k in zip(h, (grad_x, grad_gamma, grad_dy), ('grad_x', 'grad_gamma', 'grad_dy')):
                R.assert_same_bits(t.cpu(), want.cpu(), f'_GammaLayerNorm second order {k}')
        merge(worst, R.ln_check(c, eps, outs, grad_gamma=grad_gamma.cpu()))
    print(f'row_ln_bwd2 {M}x{D} eps {eps:g}: err / bound {worst}')
    record_parity('gan_row_ln_bwd2', dict(shape=[M, D], eps=eps, err_over_bound=worst))


# ------------------------------------------------------------------------------------------------ pk_bmm

def _run_bmm(L, c, accumulate):
    """the operands as flat device buffers (behind `offset` NaN elements in the `views` layout); C pre-filled with NaN, or with C0 and NaN pads"""
    off = c['offset']

    def flat(t):
        buf = torch.full((off + t.numel(),), NAN, device='cuda')
        buf[off:] = t.reshape(-1).cuda()
        return buf[off:]
    A, B = flat(c['A']), flat(c['B'])
    C = c['C0'].cuda() if accumulate else torch.full(c['C0'].shape, NAN, device='cuda')
    L.bmm(A, B, C, c['tA'], c['tB'], c['Z'], c['M'], c['N'], c['K'], lda=c['lda'], ldb=c['ldb'], ldc=c['ldc'], sA=c['sA'], sB=c['sB'], sC=c['sC'],
          accumulate=accumulate)
    return R.bmm_check(c, C.cpu(), accumulate)


@pytest.mark.parametrize('Z,M,N,K', R.BMM_SHAPES)
def test_bmm_every_transposition_layout_and_pass(Z, M, N, K):
    """plain and padded leading dimensions for every case; one B shared by every batch (sB = 0) and operands that start inside a longer buffer at the
    batched odd shape; random data within sum_bound(sum|a||b|, K), the dyadic grid bit for bit; the accumulate pass from a random C"""
    from phenaki_pytorch_amd import _lib as L
    layouts = ['plain', 'padded'] + (['shared', 'views'] if (Z, M, N, K) == (3, 70, 33, 19) else [])
    worst = 0.
    for (tA, tB), layout, data, acc in itertools.product(itertools.product((False, True), repeat=2), layouts, ('rand', 'grid'), (False, True)):
        worst = max(worst, _run_bmm(L, R.bmm_case(Z, M, N, K, tA, tB, layout=layout, data=data), acc))
    print(f'bmm {Z}x{M}x{N}x{K}: err / bound {worst:.3f}')
    record_parity('gan_bmm', dict(shape=[Z, M, N, K], err_over_bound=worst))


# ------------------------------------------------------------------------------------------------ pk_im2col / pk_col2im

@pytest.mark.parametrize('size', R.CONV_SIZES)
def test_im2col_col2im(size):
    """im2col bit for bit (zeros outside the image included), col2im within sum_bound over the taps of each pixel and bit for bit on the grid, exact zeros
    where no patch reads; ldc = kh kw C and that plus 4 with the pad columns watched"""
    from phenaki_pytorch_amd import _lib as L
    B, H, W, C = size
    worst, ran = 0., 0
    for geom, data, pad in itertools.product(R.CONV_GEOMS, ('rand', 'grid'), (0, R.CONV_LD_PAD)):
        c = R.conv_case(size, geom, data)
        if c is None:
            continue
        kh, kw, stride, p = geom
        rows, width = B * c['Ho'] * c['Wo'], kh * kw * C
        assert L.conv_out_size(H, kh, stride, p) == c['Ho'] and L.conv_out_size(W, kw, stride, p) == c['Wo']
        cols = torch.full((rows, width + pad), NAN, device='cuda')
        L.im2col(c['x'].cuda(), B, H, W, C, kh, kw, stride, p, cols)
        d, dbuf = R.strided(c['d'], pad, device='cuda')
        dx, guard = guarded(B * H * W, C)
        L.col2im(d, B, H, W, C, kh, kw, stride, p, dx)
        R.assert_untouched(guard, 'col2im: the row behind the output')
        R.assert_untouched(dbuf[:, width:], 'col2im: the pad columns of its input')
        worst = max(worst, R.conv_check(c, cols.cpu(), dx.cpu(), pad))
        ran += 1
    assert ran >= 8
    if H == 1:
        # a kernel that does not fit the padded image has no output position (floor division gives 0 rows): refused, not run as if it had one
        x, big = torch.zeros(B * H * W, C, device='cuda'), torch.full((B * 4, 4 * C), NAN, device='cuda')
        for kh, kw in ((2, 2), (3, 1), (1, 3)):
            assert L.conv_out_size(H, kh, 2, 0) <= 0 or L.conv_out_size(W, kw, 2, 0) <= 0
            with pytest.raises(RuntimeError, match='pk_im2col'):
                L.im2col(x, B, H, W, C, kh, kw, 2, 0, big)
            with pytest.raises(RuntimeError, match='pk_col2im'):
                L.col2im(big, B, H, W, C, kh, kw, 2, 0, torch.full((B * H * W, C), NAN, device='cuda'))
        R.assert_untouched(big, 'a refused im2col wrote nothing')
    print(f'im2col / col2im {size}: err / bound {worst:.3f} over {ran} calls')
    record_parity('gan_im2col_col2im', dict(size=list(size), calls=ran, err_over_bound=worst))


# ------------------------------------------------------------------------------------------------ the layout maps and pk_pick_frames

@pytest.mark.parametrize('C,Cp', R.LAYOUT_C)
def test_layout_maps_and_frame_picks_are_copies(C, Cp):
    from phenaki_pytorch_amd import _lib as L
    for (H, W), F_ in itertools.product(R.LAYOUT_HW, R.PICK_F):
        B = 3
        g = R.gen(27, C, Cp, H, W, F_)
        img = torch.randn(B, C, H, W, generator=g)
        rows, guard = guarded(B * H * W, Cp)
        L.nchw_to_rows(img.cuda(), Cp, rows)
        R.assert_same_bits(rows.cpu(), R.rows_of_image(img, Cp), 'nchw_to_rows')
        R.assert_untouched(guard, 'nchw_to_rows: the row behind the output')
        src = torch.randn(B * H * W, Cp, generator=g)                     # the padding channels hold values: the adjoint drops them
        back = torch.full((B + 1, C, H, W), NAN, device='cuda')
        L.rows_to_nchw(src.cuda(), Cp, back[:B])
        R.assert_same_bits(back[:B].cpu(), src[:, :C].reshape(B, H, W, C).permute(0, 3, 1, 2).contiguous(), 'rows_to_nchw')
        R.assert_untouched(back[B:], 'rows_to_nchw: the image behind the output')
        video = torch.randn(B, C, F_, H, W, generator=g)
        frame = torch.tensor([F_ - 1, 0, F_ // 2], dtype=torch.int32)
        pick = torch.full((B + 1, C, H, W), NAN, device='cuda')
        L.pick_frames(video.cuda(), frame.cuda(), pick[:B])
        R.assert_same_bits(pick[:B].cpu(), R.pick_ref(video, frame), 'pick_frames')
        R.assert_untouched(pick[B:], 'pick_frames: the image behind the output')
        placed = L.pick_frames(torch.zeros(B, C, F_, H, W, device='cuda'), frame.cuda(), pick[:B].contiguous(), place=True)
        R.assert_same_bits(placed.cpu(), R.place_ref(R.pick_ref(video, frame), frame, F_), 'pick_frames place')
    record_parity('gan_layout_maps', dict(C=C, Cp=Cp, err_over_bound=0.))


# ------------------------------------------------------------------------------------------------ the product ladder of discriminator._mm_raw

def test_mm_ladder_every_rung(monkeypatch):
    """one case per rung of _mm_raw in fp32 mode, the rung asserted by counting the launches: value and the two products _MM.backward forms, each within
    sum_bound(sum|a||b|, K) of float64"""
    from phenaki_pytorch_amd import _lib as L
    from phenaki_pytorch_amd import discriminator as Dm
    calls = []
    for mod, name, tag in ((L, 'gemm', 'gemm'), (L, 'bmm', 'bmm'), (Dm, '_weight_grad_gemm', 'splitk')):
        def counted(*a, _f=getattr(mod, name), _tag=tag, **kw):
            calls.append(_tag)
            return _f(*a, **kw)
        monkeypatch.setattr(mod, name, counted)
    worst = {}
    for name, tA, tB, M, N, K, rung in R.MM_CASES:
        c = R.mm_case(tA, tB, M, N, K)
        assert Dm._fast_ok(M, N, K) == (name not in ('k12', 'n6')), name
        del calls[:]
        got = Dm.mm(c['A'].cuda(), c['B'].cuda(), tA, tB, L.F32)
        # (the split-K rung hands on to pk_gemm or pk_gemm_splitk inside _weight_grad_gemm)
        assert calls[:1] == [rung] and (rung == 'splitk' or len(calls) == 1), (name, calls)
        ref, bound = R.mm_ref(c['A'], c['B'], tA, tB)
        worst[name] = R.assert_within(got.cpu(), ref, bound, f'mm {name}')
        grads = R.mm_backward_ref(c)
        for g, X, Y, tX, tY in R.mm_backward_calls(c):
            r, bd = R.mm_ref(X, Y, tX, tY)
            worst[f'{name}_{g}'] = R.assert_within(Dm.mm(X.cuda(), Y.cuda(), tX, tY, L.F32).cpu(), grads[g], bd, f'mm {name} {g}')
    Z, M, N, K = R.MM_BATCHED
    for tA, tB in itertools.product((False, True), repeat=2):
        c = R.mm_case(tA, tB, M, N, K, Z=Z)
        del calls[:]
        got = Dm.mm(c['A'].cuda(), c['B'].cuda(), tA, tB, L.F32)
        assert calls == ['bmm'], calls
        ref, bound = R.mm_ref(c['A'], c['B'], tA, tB)
        worst[f'batched_{int(tA)}{int(tB)}'] = R.assert_within(got.cpu(), ref, bound, f'mm batched tA={tA} tB={tB}')
    print(f'mm ladder: err / bound {worst}')
    record_parity('gan_mm_ladder', dict(err_over_bound=worst))
