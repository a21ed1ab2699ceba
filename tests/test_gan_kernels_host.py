"""tests/gan_kernels_reference.py on its own, no kernel launched: (1) a float64 transcription of the formulas in csrc/conv.hip's header (softmax, l2norm x scale,
LayerNorm second order) against the autograd restatements, on the shapes tests/test_gan_kernels_gpu.py uses -- including the l2norm's branch under
F.normalize's clamp, where the formulas as they stood before the branch was added are shown to disagree; (2) every checker of the GPU tests fed its own
reference with ONE planted error and required to raise for that reason; (3) an f32 evaluation of every restatement on the CPU, in a second summation order
where there is one, inside its own bound; (4) the preconditions the cases promise."""
import itertools

import pytest
import torch

from tests import gan_kernels_reference as R

NAN = R.NAN


@pytest.fixture(autouse=True)
def _grad():
    """other modules of the suite switch autograd off for the process"""
    with torch.enable_grad():
        yield


def same_rows(a, b, what, rtol=1e-12, floor=None, cond=None):
    """every row of a within rtol of its own largest reference element (the rows of a case differ in scale by 1e12).
    cond (per row, >= 1): the amplification of float64's own rounding by a cancellation in the INPUT of both sides (x - mean, from |x| down to sigma): two
    correct float64 evaluations in different association orders agree to rtol cond only.
    floor (per row): the size of the terms where the result is what a cancellation leaves of them (P t at d = 1, y (dy - <y, dy>) at the peak of a row):
    float64 resolves such a result to a few roundings, 2^-53 each, of the terms -- 1e-15 floor is nine of them"""
    a, b = a.double(), b.double()
    assert a.shape == b.shape, what
    if a.numel() == 0:
        return
    err = (a - b).abs().reshape(a.shape[0], -1).max(1).values
    tol = rtol * b.abs().reshape(b.shape[0], -1).max(1).values
    if cond is not None:
        tol = tol * cond.double().reshape(-1)
    if floor is not None:
        tol = tol + 1e-15 * floor.double().reshape(-1)
    worst = (err / tol.clamp_min(1e-300)).max().item()
    assert torch.isfinite(a).all() and (err <= tol).all(), f'{what}: row {int((err / tol.clamp_min(1e-300)).argmax())} is {worst:.3e} of its tolerance apart'


def same_sum(total, rows, what, row_rtol=1e-12, cond=None, floor=None):
    """total (N,) against the column sum of rows (M, N), two float64 statements of one sum over M rows: each row of the two agrees to row_rtol (cond) of
    its own largest element plus its floor (same_rows), and two float64 sums of M terms in different orders are each within M 2^-53 sum|terms| of the exact one"""
    rows = rows.double()
    per_row = row_rtol * rows.abs().amax(1) * (cond.double().reshape(-1) if cond is not None else 1.)
    if floor is not None:
        per_row = per_row + 1e-15 * floor.double().reshape(-1)
    tol = per_row.sum() + (2 * rows.shape[0] + 16) * 2.0 ** -53 * rows.abs().sum(0)
    err = (total.double() - rows.sum(0)).abs()
    assert (err <= tol).all(), f'{what}: column {int((err / tol.clamp_min(1e-300)).argmax())} is {(err / tol.clamp_min(1e-300)).max().item():.3e} of its tolerance apart'


def norm_relative_ok(a, b, rtol):
    """the whole-tensor criterion the older kernel tests use, max|a - b| <= rtol max|b|: restated to show what it lets through"""
    return bool((a.double() - b.double()).abs().max() <= rtol * b.double().abs().max())


# ------------------------------------------------------------------------------------------------ conv.hip's formulas, transcribed in float64

def header_softmax(y, dy, u):
    """B(y, dy) = y (dy - <y, dy>);  d<u, B>/dy_in = u (dy - <y, dy>) - dy <u, y>,  d<u, B>/d dy = B(y, u)"""
    dot = lambda p, q: (p * q).sum(-1, keepdim=True)                        # noqa: E731
    return dict(b1=y * (dy - dot(y, dy)), g_y=u * (dy - dot(y, dy)) - dy * dot(u, y), g_dy=y * (u - dot(y, u)))


def header_l2(x, sc, dz, gx, gsc, clamp_branch):
    """x^ = x / |x|, t = dz sc, P = I - x^ x^T:  dx = P t / |x|, dsc rows dz x^;  grad_dz = sc P gx / |x| + gsc x^,  grad_sc rows dz P gx / |x|,
    grad_x = -[P (a gx + b t) + x^ <gx, t - x^ a>] / |x|^2 + P (gsc dz) / |x|, a = <x^, t>, b = <gx, x^>.
    clamp_branch: under the clamp |x| < eps the normaliser is eps and P = I, no curvature; without it the projection formulas run on max(|x|, eps)"""
    dot = lambda p, q: (p * q).sum(-1, keepdim=True)                        # noqa: E731
    root = x.norm(dim=-1, keepdim=True)
    below = root < R.L2_EPS
    n = root.clamp_min(R.L2_EPS)
    xh, t = x / n, dz * sc
    P = lambda v: v - xh * dot(xh, v)                                       # noqa: E731
    a, b = dot(xh, t), dot(gx, xh)
    out = dict(z=xh * sc, dx=P(t) / n, dsc_rows=dz * xh, grad_dz=sc * P(gx) / n + gsc * xh, grad_sc_rows=dz * P(gx) / n,
               grad_x=-(P(a * gx + b * t) + xh * dot(gx, t - xh * a)) / n ** 2 + P(gsc * dz) / n)
    if clamp_branch:
        lin = dict(dx=t / n, grad_dz=sc * gx / n + gsc * xh, grad_sc_rows=dz * gx / n, grad_x=gsc * dz / n)
        out.update({k: torch.where(below, v, out[k]) for k, v in lin.items()})
    return out, below.reshape(-1)


def header_ln(x, gamma, dy, u, w, eps):
    """second order (u for dx, w for dgamma): gg = (u - mean u - x^ mean(u x^)) / sigma, grad_dy = gamma gg + w x^, grad_gamma rows dy gg,
    v = -(m2 u + c2 g^) / sigma + w dy,  grad_x = (v - mean v - x^ mean(v x^)) / sigma - S x^ / (D sigma^2),  S = <u, g^> - D c1 m1 - D c2 m2"""
    D = x.shape[-1]
    mean = lambda t: t.mean(-1, keepdim=True)                               # noqa: E731
    cen = x - mean(x)
    sig = (mean(cen * cen) + eps).sqrt()
    xh, gh = cen / sig, dy * gamma
    c1, c2, m1, m2 = mean(u), mean(u * xh), mean(gh), mean(gh * xh)
    S = (u * gh).sum(-1, keepdim=True) - D * c1 * m1 - D * c2 * m2
    v = -(m2 * u + c2 * gh) / sig + w * dy
    gg = (u - c1 - xh * c2) / sig
    return dict(dx=(gh - m1 - xh * m2) / sig, dg_rows=dy * xh, grad_dy=gamma * gg + w * xh, grad_gamma_rows=dy * gg,
                grad_x=(v - mean(v) - xh * mean(v * xh)) / sig - S * xh / (D * sig ** 2))


@pytest.mark.parametrize('M,n', R.SOFTMAX_SHAPES)
def test_softmax_formulas_are_autograd_of_softmax(M, n):
    for data in R.SOFTMAX_DATA:
        c = R.softmax_case(M, n, data)
        ref = R.softmax_ref(c)
        got = header_softmax(c['y'].double(), c['dy'].double(), c['c'].double())
        # at the peak of a `spread` row y (dy - <y, dy>) is what is left of dy after a cancellation to 1e-26 of it
        mag = c['dy'].abs().amax(1) * (1 + c['c'].abs().amax(1))
        for k, v in got.items():
            same_rows(v, ref[k], f'softmax {k} {data}', floor=mag if data == 'spread' else None)
        # the output-form Jacobian is the vector-Jacobian product of x.softmax(-1) itself, at an exact softmax row
        x = c['x'].double().requires_grad_(True)
        y = x.softmax(-1)
        vjp, = torch.autograd.grad(y, x, c['dy'].double())
        same_rows(R.softmax_jvp_of_output(y.detach(), c['dy'].double()), vjp, f'softmax vjp {data}', floor=mag if data == 'spread' else None)
        # the chain from x: the backward of the backward hands mode 2's output to mode 1 again
        yd = y.detach()
        G = header_softmax(yd, c['dy'].double(), c['c'].double())['g_y']
        same_rows(header_softmax(yd, G, G)['b1'], ref['hx'], f'softmax second derivative from x {data}', floor=mag if data == 'spread' else None)


@pytest.mark.parametrize('M,d', R.L2_SHAPES)
def test_l2scale_formulas_are_autograd_of_normalize_times_scale(M, d):
    import torch.nn.functional as F
    for c in R.l2_cases(M, d):
        ref = R.l2_ref(c)
        ins = [c[k].double() for k in ('x', 'sc', 'dz', 'gx', 'gsc')]
        fixed, below = header_l2(*ins, clamp_branch=True)
        old, _ = header_l2(*ins, clamp_branch=False)
        assert set(c['planted'].values()) >= set(below.nonzero().reshape(-1).tolist()) and int(below.sum()) == sum(k in c['planted'] for k in ('zero', 'below'))
        # at or above the clamp the projected outputs are what P = I - x^ x^T leaves of terms of their own order (nothing at all at d = 1): base / |x| for
        # the first-order ones, base / |x|^2 for grad_x.  z and dsc_rows have no cancellation and no floor.  Under the clamp nothing cancels in any
        # output (every one is a product, or a sum of two): no floor there, those rows are held to 1e-12 of their own scale and to nothing else
        inv = 1 / ins[0].norm(dim=-1).clamp_min(R.L2_EPS)
        base = (1 + ins[2].abs().amax(1)) * (1 + ins[3].abs().amax(1)) * (1 + ins[4].abs().max()) * ins[1].abs().max()
        unclamped = (~below).double()
        floors = dict(z=None, dsc_rows=None, dx=base * inv * unclamped, grad_dz=base * inv * unclamped, grad_sc_rows=base * inv * unclamped,
                      grad_x=base * (inv ** 2 + inv) * unclamped)
        for k in ref:
            same_rows(fixed[k], ref[k], f'l2scale {k}, the branch under the clamp included', floor=floors[k])
            fl = None if floors[k] is None else floors[k][~below]
            same_rows(old[k][~below], ref[k][~below], f'l2scale {k}, rows at or above the clamp, formulas without the branch', floor=fl)
        # the two-branch statement IS F.normalize(x) * sc, value and first derivatives, wherever torch's own autograd is finite (everywhere but x = 0)
        x = c['x'].double().requires_grad_(True)
        sc = c['sc'].double().requires_grad_(True)
        z = F.normalize(x, dim=-1) * sc
        same_rows(ref['z'], z.detach(), 'l2scale value')
        dx, dsc = torch.autograd.grad((z * c['dz'].double()).sum(), (x, sc))
        nz = c['x'].double().norm(dim=-1) > 0
        same_rows(ref['dx'][nz], dx[nz], 'l2scale dx against F.normalize', floor=floors['dx'][nz])
        same_sum(dsc, ref['dsc_rows'], 'l2scale dsc against F.normalize')
        # why the branch exists: on the row under the clamp the SAME comparison rejects the formulas without it in every output they touch (grad_x by
        # ten orders of magnitude); z and the dsc rows never had the projection and agree
        if 'below' in c['planted']:
            i = c['planted']['below']
            for k in ('dx', 'grad_dz', 'grad_sc_rows', 'grad_x'):
                with pytest.raises(AssertionError, match='of its tolerance apart'):
                    same_rows(old[k][i:i + 1], ref[k][i:i + 1], f'l2scale {k} without the branch', floor=floors[k][i:i + 1])
            # a half-made fix is rejected too: the curvature dropped but the projection kept on the gsc dz term, P (gsc dz) / eps (off by |x / eps|^2)
            if d > 1:
                xh = ins[0][i:i + 1] / R.L2_EPS
                half = (ins[4] * ins[2][i:i + 1] - xh * (xh * ins[4] * ins[2][i:i + 1]).sum(-1, keepdim=True)) / R.L2_EPS
                with pytest.raises(AssertionError, match='of its tolerance apart'):
                    same_rows(half, ref['grad_x'][i:i + 1], 'l2scale grad_x with the projection left on gsc dz', floor=floors['grad_x'][i:i + 1])
            rel = lambda k: float((old[k][i] - ref[k][i]).abs().max() / ref[k][i].abs().max())      # noqa: E731
            assert rel('grad_x') > 1e6 and rel('dsc_rows') < 1e-12 and rel('z') < 1e-12, rel('grad_x')


@pytest.mark.parametrize('M,D', R.LN_SHAPES)
@pytest.mark.parametrize('eps', R.LN_EPS)
def test_layernorm_second_order_formulas_are_autograd_of_layer_norm(M, D, eps):
    import torch.nn.functional as F
    for c in R.ln_cases(M, D):
        ref = R.ln_ref(c, eps)
        got = header_ln(*(c[k].double() for k in ('x', 'gamma', 'dy', 'u', 'w')), eps)
        # x - mean takes |x| down to sigma on both sides, in different association orders: a row of mean 1e3 and unit spread keeps 1e3 times fewer digits
        # (cond); where x^ = 0 (D = 1, the constant row) the outputs are what cancellations leave of terms of their own order: base / sigma for the
        # first-order ones and the per-row second-order ones, base / sigma^2 for grad_x, base for dy x^ (floors)
        sig = (c['x'].double().var(-1, unbiased=False) + eps).sqrt()
        cond = 1 + c['x'].double().abs().amax(1) / sig
        base = (1 + c['dy'].abs().amax(1) * c['gamma'].abs().max()) * (1 + c['u'].abs().amax(1)) * (1 + c['w'].abs().max())
        floors = dict(dx=base / sig, dg_rows=base, grad_dy=base / sig, grad_gamma_rows=base / sig, grad_x=base * (1 / sig ** 2 + 1 / sig))
        for k in ref:
            same_rows(got[k], ref[k], f'layernorm {k} eps {eps:g}', cond=cond, floor=floors[k] * cond)
        # the per-row gamma copy changes nothing: the column sum of its gradient is F.layer_norm's own weight gradient
        x, g = c['x'].double().requires_grad_(True), c['gamma'].double().requires_grad_(True)
        dx, dg = torch.autograd.grad((F.layer_norm(x, (D,), g, None, eps) * c['dy'].double()).sum(), (x, g))
        same_rows(ref['dx'], dx, 'layernorm dx', cond=cond, floor=floors['dx'] * cond)
        same_sum(dg, ref['dg_rows'], 'layernorm dgamma', cond=cond, floor=floors['dg_rows'] * cond)


# ------------------------------------------------------------------------------------------------ the checkers can fail

def as_f32(ref):
    return {k: v.float() for k, v in ref.items()}


def off_by_4_bounds(out, ref, bound, k):
    """moves the element of out[k] whose bound is smallest against the tensor's largest element by 4x that bound; returns its index"""
    score = bound[k] / ref[k].abs().max().clamp_min(1e-300)
    score = torch.where(bound[k] > 0, score, torch.full_like(score, float('inf')))
    i = int(score.argmin())
    bad = {kk: v.clone() for kk, v in out.items()}
    bad[k].view(-1)[i] = float(ref[k].reshape(-1)[i] + 4 * bound[k].reshape(-1)[i])
    assert bad[k].view(-1)[i] != out[k].view(-1)[i], 'the planted error is below the f32 grid'
    return bad, i


def test_softmax_checker_rejects_planted_errors():
    c = R.softmax_case(37, 256, 'spread')
    ref, bound = R.softmax_ref(c), R.softmax_bounds(c)
    good = as_f32(ref)
    assert max(R.softmax_check(c, good).values()) < 1
    for k in good:
        bad, _ = off_by_4_bounds(good, ref, bound, k)
        assert norm_relative_ok(bad[k], ref[k], 2e-4), 'the whole-tensor criterion accepts this element'
        with pytest.raises(AssertionError, match=f'row_softmax {k}.*beyond its bound'):
            R.softmax_check(c, bad)
    # the -b <c, a> term of mode 2 left out (an f32 evaluation that is otherwise inside the bound)
    c = R.softmax_case(5, 65, 'normal')
    R.softmax_check(c, R.softmax_f32(c))
    with pytest.raises(AssertionError, match='row_softmax g_y'):
        R.softmax_check(c, R.softmax_f32(c, drop_q=True))
    # a row never written, two rows swapped
    good = as_f32(R.softmax_ref(c))
    bad = dict(good, y0=good['y0'].clone())
    bad['y0'][3] = NAN
    with pytest.raises(AssertionError, match=r'row_softmax y0.*element \(3, 0\)'):
        R.softmax_check(c, bad)
    bad = dict(good, b1=good['b1'][[1, 0, 2, 3, 4]])
    with pytest.raises(AssertionError, match=r'row_softmax b1.*element \(0,'):
        R.softmax_check(c, bad)


def test_l2scale_checker_rejects_planted_errors():
    c = R.l2_case(130, 64)
    ref, bound = R.l2_ref(c), R.l2_bounds(c)
    good = as_f32(ref)
    sums = dict(dsc=ref['dsc_rows'].sum(0).float(), grad_sc=ref['grad_sc_rows'].sum(0).float())
    assert max(R.l2_check(c, good, **sums).values()) < 1
    for k in good:
        bad, _ = off_by_4_bounds(good, ref, bound, k)
        assert norm_relative_ok(bad[k], ref[k], 2e-4), 'the whole-tensor criterion accepts this element'
        with pytest.raises(AssertionError, match=f'row_l2scale {k} .*beyond its bound'):
            R.l2_check(c, bad)
    # a whole row wrong in a tensor of mixed scales: the 1e-6 row's dx doubled is still nothing beside the 1e6 rows' ... and the other way round for z
    small = 4                                                   # 4 % 3 == 1: a row scaled by 1e-6
    bad = dict(good, z=good['z'].clone())
    bad['z'][small] *= 1.001
    with pytest.raises(AssertionError, match='row_l2scale z'):
        R.l2_check(c, bad)
    # a per-row contribution added into the wrong row: the column sum does not move, the rows do
    bad = dict(good, grad_sc_rows=good['grad_sc_rows'].clone())
    bad['grad_sc_rows'][9] += bad['grad_sc_rows'][8]
    bad['grad_sc_rows'][8] = 0
    R.assert_within(bad['grad_sc_rows'].double().sum(0), ref['grad_sc_rows'].sum(0), R.col_bound(ref['grad_sc_rows'], bound['grad_sc_rows']), 'the column sum')
    with pytest.raises(AssertionError, match=r'row_l2scale grad_sc_rows.*element \(8,'):
        R.l2_check(c, bad)
    # the formulas without the branch under the clamp, the returned sums in the wrong slots, a column sum that misses a row
    old, _ = header_l2(*(c[k].double() for k in ('x', 'sc', 'dz', 'gx', 'gsc')), clamp_branch=False)
    for k in ('dx', 'grad_x', 'grad_dz', 'grad_sc_rows'):
        with pytest.raises(AssertionError, match=rf'row_l2scale {k} .*element \({c["planted"]["below"]},'):
            R.l2_check(c, dict(good, **{k: old[k].float()}))
    with pytest.raises(AssertionError, match='row_l2scale dsc '):
        R.l2_check(c, good, dsc=sums['grad_sc'], grad_sc=sums['dsc'])
    with pytest.raises(AssertionError, match='row_l2scale grad_sc '):
        R.l2_check(c, good, grad_sc=(ref['grad_sc_rows'].sum(0) - ref['grad_sc_rows'][c['planted']['below']]).float())


def test_layernorm_checker_rejects_planted_errors():
    c = R.ln_case(133, 128)
    for eps in R.LN_EPS:
        ref, bound = R.ln_ref(c, eps), R.ln_bounds(c, eps)
        good = {k: ref[k].float() for k in ('grad_x', 'grad_gamma_rows', 'grad_dy')}
        assert max(R.ln_check(c, eps, good, grad_gamma=ref['grad_gamma_rows'].sum(0).float()).values()) < 1
        for k in good:
            bad, _ = off_by_4_bounds(good, ref, bound, k)
            assert norm_relative_ok(bad[k], ref[k], 2e-4), 'the whole-tensor criterion accepts this element'
            with pytest.raises(AssertionError, match=f'row_ln_bwd2 {k} .*beyond its bound'):
                R.ln_check(c, eps, bad)
        # eps ignored, or the other eps hard-coded: the constant row has sigma = sqrt(eps)
        with pytest.raises(AssertionError, match='row_ln_bwd2'):
            R.ln_check(c, eps, R.ln_f32(c, eps, no_eps=True))
        other = R.LN_EPS[1 - R.LN_EPS.index(eps)]
        with pytest.raises(AssertionError, match='row_ln_bwd2 grad_dy'):
            R.ln_check(c, eps, {k: R.ln_ref(c, other)[k].float() for k in ('grad_dy',)})
        with pytest.raises(AssertionError, match='row_ln_bwd2 grad_gamma '):
            R.ln_check(c, eps, good, grad_gamma=ref['grad_gamma_rows'][1:].sum(0).float())
    # w dropped (the upstream of dgamma): grad_dy loses w x^
    with pytest.raises(AssertionError, match='row_ln_bwd2 grad_dy'):
        R.ln_check(c, 1e-5, {'grad_dy': R.ln_ref(dict(c, w=torch.zeros_like(c['w'])), 1e-5)['grad_dy'].float()})


def bmm_fake(c, accumulate=False, ref=None):
    buf = torch.full((c['Z'], c['M'], c['ldc']), NAN)
    buf[:, :, :c['N']] = (R.bmm_ref(c, accumulate)[0] if ref is None else ref).float()
    return buf


@pytest.mark.parametrize('tA,tB', itertools.product((False, True), repeat=2))
def test_bmm_checker_rejects_planted_errors(tA, tB):
    for data in ('rand', 'grid'):
        c = R.bmm_case(3, 70, 33, 19, tA, tB, layout='padded', data=data)
        for acc in (False, True):
            assert R.bmm_check(c, bmm_fake(c, acc), acc) < 1
        ref, bound = R.bmm_ref(c)
        # an element off by 4x its bound (on the grid: by one grid step) that the whole-tensor criterion accepts
        bad = bmm_fake(c)
        i = (0, 5, 7)
        bad[i] = float(ref[i] + (4 * bound[i] if data == 'rand' else 1 / 16.))
        assert norm_relative_ok(bad[:, :, :33], ref, 1e-5) or data == 'grid'
        with pytest.raises(AssertionError, match=r'\(0, 5, 7\)'):
            R.bmm_check(c, bad)
        # a pad column of C written; a row left as NaN; B read with the other transposition flag; the accumulate pass that forgot C0
        bad = bmm_fake(c)
        bad[1, 69, 33] = 0.
        with pytest.raises(AssertionError, match='pad columns of C'):
            R.bmm_check(c, bad)
        bad = bmm_fake(c)
        bad[2, 69, :33] = NAN
        with pytest.raises(AssertionError, match=r'\(2, 69, 0\)'):
            R.bmm_check(c, bad)
        a, b = R.bmm_operands(c)
        wrong = b.transpose(1, 2).reshape(b.shape)                 # the (K, N) storage read as (N, K) or the other way round
        with pytest.raises(AssertionError):
            R.bmm_check(c, bmm_fake(c, ref=a @ wrong))
        with pytest.raises(AssertionError):
            R.bmm_check(c, bmm_fake(c), accumulate=True)
    # batch z reading batch 0's B where every batch has its own
    c = R.bmm_case(3, 70, 33, 19, tA, tB)
    a, b = R.bmm_operands(c)
    with pytest.raises(AssertionError, match=r'\(1, 0, 0\)'):
        R.bmm_check(c, bmm_fake(c, ref=a @ b[:1]))


@pytest.mark.parametrize('geom', R.CONV_GEOMS)
def test_conv_checker_rejects_planted_errors(geom):
    for data in ('rand', 'grid'):
        c = R.conv_case(R.CONV_SIZES[0], geom, data)
        kh, kw = geom[:2]
        width = kh * kw * 8
        unf, by_index = R.im2col_ref(c)
        R.assert_same_bits(unf, by_index, 'the two im2col references')
        fold, by_index, bound, taps = R.col2im_ref(c)
        # two float64 sums of at most 9 terms in different orders: 9 x 2^-53 of sum|terms| each, far inside 1e-13 (1 + |sum|) for N(0, 1) terms
        R.assert_within(by_index, fold, 1e-13 * (1 + fold.abs()), 'the two col2im references')
        assert int(taps.max()) <= kh * kw

        def fake():
            cols = torch.full((unf.shape[0], width + 4), NAN)
            cols[:, :width] = unf.float()
            return cols, fold.float()
        cols, dx = fake()
        assert R.conv_check(c, cols, dx, 4) < 1
        cols, dx = fake()
        cols[3, width] = 0.
        with pytest.raises(AssertionError, match='im2col.*pad columns'):
            R.conv_check(c, cols, dx, 4)
        cols, dx = fake()
        cols[[0, 1]] = cols[[1, 0]]
        if not torch.equal(cols[0, :width], cols[1, :width]):
            with pytest.raises(AssertionError, match='im2col.*bit for bit'):
                R.conv_check(c, cols, dx, 4)
        cols, dx = fake()
        dx[5] = NAN
        with pytest.raises(AssertionError, match='col2im.*not written'):
            R.conv_check(c, cols, dx, 4)
        # one tap missing from col2im; one element off by 4x its bound (grid: by one)
        cols, dx = fake()
        short = R.col2im_ref(c, skip_tap=kh * kw - 1)[1]
        assert not torch.equal(short, by_index)
        with pytest.raises(AssertionError, match='col2im'):
            R.conv_check(c, cols, short.float(), 4)
        i = int((bound.reshape(-1) + (taps[:, None] == 0).expand_as(bound).reshape(-1) * 1e30).argmin())
        dx.view(-1)[i] = float(fold.reshape(-1)[i] + (4 * bound.reshape(-1)[i] if data == 'rand' else 1.))
        with pytest.raises(AssertionError, match='col2im'):
            R.conv_check(c, cols, dx, 4)
    # a pixel no patch reads must come back as an exact zero
    c = R.conv_case(R.CONV_SIZES[1], (1, 1, 2, 0))
    fold, _, _, taps = R.col2im_ref(c)
    assert int((taps == 0).sum()) > 0
    cols = R.im2col_ref(c)[0].float()
    dx = fold.float()
    R.conv_check(c, cols, dx, 0)
    dx[int((taps == 0).nonzero()[0]), 1] = -0.
    with pytest.raises(AssertionError, match='pixels no patch reads'):
        R.conv_check(c, cols, dx, 0)


def test_layout_references_tell_rows_and_channels_apart():
    img = torch.randn(2, 3, 6, 8, generator=R.gen(30))
    rows = R.rows_of_image(img, 8)
    assert torch.equal(rows[:, :3], img.permute(0, 2, 3, 1).reshape(-1, 3)) and not rows[:, 3:].any()
    with pytest.raises(AssertionError, match='bit for bit'):
        R.assert_same_bits(rows[torch.arange(96) ^ 1], rows, 'two rows swapped')
    video = torch.randn(3, 2, 5, 2, 2, generator=R.gen(31))
    frame = torch.tensor([4, 0, 2])
    pick = R.pick_ref(video, frame)
    assert torch.equal(pick[0], video[0, :, 4]) and torch.equal(pick[2], video[2, :, 2])
    placed = R.place_ref(pick, frame, 5)
    assert torch.equal(R.pick_ref(placed, frame), pick) and int((placed != 0).sum()) == pick.numel()
    with pytest.raises(AssertionError, match='bit for bit'):
        R.assert_same_bits(R.pick_ref(video, torch.tensor([4, 1, 2])), pick, 'the wrong frame')


def test_mm_checker_rejects_a_wrong_transposition_and_a_dropped_k_tile():
    for name, tA, tB, M, N, K, _ in R.MM_CASES:
        c = R.mm_case(tA, tB, M, N, K)
        ref, bound = R.mm_ref(c['A'], c['B'], tA, tB)
        assert R.assert_within(ref.float(), ref, bound, name) < 1
        a = (c['A'].t() if tA else c['A']).double()
        b = (c['B'].t() if tB else c['B']).double()
        with pytest.raises(AssertionError):
            R.assert_within((a[:, :-1] @ b[:-1]).float(), ref, bound, f'{name} without the last k')
        grads = R.mm_backward_ref(c)
        for g, X, Y, tX, tY in R.mm_backward_calls(c):
            r, bd = R.mm_ref(X, Y, tX, tY)
            same_rows(r, grads[g], f'{name} {g}: the product _MM.backward forms is the autograd gradient')
            # the second operand's storage read with the other flag (its rows and columns exchanged in place: every shape stays valid)
            wrong = Y.t().reshape(Y.shape)
            with pytest.raises(AssertionError, match='beyond its bound'):
                R.assert_within(R.mm_ref(X, wrong, tX, tY)[0].float(), grads[g], bd, f'{name} {g} with the wrong flag')


# ------------------------------------------------------------------------------------------------ the bounds hold for an f32 evaluation on the CPU

@pytest.mark.parametrize('order', [0, 1])
def test_row_bounds_hold_for_an_f32_evaluation(order):
    worst = {}
    for (M, n), data in itertools.product(R.SOFTMAX_SHAPES, R.SOFTMAX_DATA):
        c = R.softmax_case(M, n, data)
        worst['softmax'] = max(worst.get('softmax', 0.), *R.softmax_check(c, R.softmax_f32(c, order)).values())
    for M, d in R.L2_SHAPES:
        for c in R.l2_cases(M, d):
            out = R.l2_f32(c, order)
            worst['l2'] = max(worst.get('l2', 0.), *R.l2_check(c, out, dsc=out['dsc_rows'].sum(0), grad_sc=out['grad_sc_rows'].sum(0)).values())
    for (M, D), eps in itertools.product(R.LN_SHAPES, R.LN_EPS):
        for c in R.ln_cases(M, D):
            out = R.ln_f32(c, eps, order)
            worst['ln'] = max(worst.get('ln', 0.), *R.ln_check(c, eps, out, grad_gamma=out['grad_gamma_rows'].sum(0)).values())
    print('f32 on the CPU, largest err / bound:', worst)
    assert all(0 < v < 1 for v in worst.values()), worst


def test_product_and_fold_bounds_hold_for_an_f32_evaluation():
    for (Z, M, N, K), (tA, tB) in itertools.product(R.BMM_SHAPES[:4] + R.BMM_SHAPES[5:], itertools.product((False, True), repeat=2)):
        for data, acc in itertools.product(('rand', 'grid'), (False, True)):
            c = R.bmm_case(Z, M, N, K, tA, tB, layout='padded', data=data)
            R.bmm_check(c, bmm_fake(c, acc, ref=R.bmm_f32(c, acc)), acc)
    c = R.bmm_case(1, 2, 1, 8192, False, False)                      # the logits layer's shape: one serial chain of 8192 terms
    assert 0 < R.bmm_check(c, bmm_fake(c, ref=R.bmm_f32(c))) < 1
    for size, geom, data in itertools.product(R.CONV_SIZES, R.CONV_GEOMS, ('rand', 'grid')):
        c = R.conv_case(size, geom, data)
        if c is None:
            continue
        # taps added last to first in f32
        idx = R.conv_tap_index(c)
        C = size[3]
        acc = torch.zeros(size[0] * size[1] * size[2] + 1, C)
        for tap in reversed(range(idx.shape[1])):
            rows = torch.where(idx[:, tap] >= 0, idx[:, tap], torch.full_like(idx[:, tap], acc.shape[0] - 1))
            acc = acc.index_add(0, rows, c['d'][:, tap * C:(tap + 1) * C])
        R.conv_check(c, R.im2col_ref(c)[1].float(), acc[:-1], 0)


# ------------------------------------------------------------------------------------------------ what the cases promise

def test_case_preconditions():
    tiny = torch.finfo(torch.float32).tiny
    for (M, n), data in itertools.product(R.SOFTMAX_SHAPES, R.SOFTMAX_DATA):
        c = R.softmax_case(M, n, data)
        assert (c['y'] >= tiny).all() and (c['x'].double().softmax(-1) >= 2 * tiny).all(), 'a subnormal softmax output'
        if data == 'spread' and n > 1:
            assert float(c['y'].min()) < 1e-25 and float((c['x'].max(1).values - c['x'].min(1).values).min()) > 59
        if data == 'offset' and M >= 4:
            assert float(c['x'].abs().max()) > 9e3
        if M > 1:
            s = c['dy'].abs().amax(1)
            assert float(s.max() / s.min()) > 100
    kinds = set()
    for M, d in R.L2_SHAPES:
        for c in R.l2_cases(M, d):
            nrm = c['x'].double().norm(dim=-1)
            assert ((nrm == 0) | (nrm < R.L2_EPS / 2) | (nrm > R.L2_EPS * 2)).all(), 'an l2 row within a factor 2 of the clamp'
            for kind, i in c['planted'].items():
                want = R.L2_PLANTED[kind]
                assert (nrm[i] == 0) if want == 0 else abs(float(nrm[i]) / want - 1) < 1e-3, (kind, float(nrm[i]))
                kinds.add((kind, M >= 5))
            if M >= 5:
                assert float(nrm.max() / nrm[nrm > 1e-9].min()) > 1e10, 'rows scaled by 1e6 and 1e-6'
    assert kinds >= {(k, big) for k in R.L2_PLANTED for big in (False, True)}
    for M, D in R.LN_SHAPES:
        cs = R.ln_cases(M, D)
        assert any('constant' in c['planted'] for c in cs)
        for c in cs:
            if 'constant' in c['planted']:
                assert float(c['x'][c['planted']['constant']].double().var(unbiased=False)) == 0
            if 'offset' in c['planted']:
                assert abs(float(c['x'][c['planted']['offset']].mean()) - 1e3) < 1
            assert D < 2 or (float(c['gamma'][0]) == 0 and float(c['gamma'].min()) < 0)
            assert float(c['w'].abs().min()) > 0
    # the dyadic grids: every sum of |terms| stays below 2^24 grid units, so every partial sum in any order is an exact f32
    for (Z, M, N, K), (tA, tB) in itertools.product(R.BMM_SHAPES, itertools.product((False, True), repeat=2)):
        c = R.bmm_case(Z, M, N, K, tA, tB, data='grid')
        a, b = R.bmm_operands(c)
        assert R.bmm_grid_units(c) < 2 ** 24 and torch.equal(a * 16, (a * 16).round()) and torch.equal(b * 16, (b * 16).round())
        assert torch.equal(R.bmm_ref(c, True)[0].float().double(), R.bmm_ref(c, True)[0])
    for size, geom in itertools.product(R.CONV_SIZES, R.CONV_GEOMS):
        c = R.conv_case(size, geom, 'grid')
        if c is not None:
            assert float(c['d'].abs().max()) * geom[0] * geom[1] < 2 ** 24 and torch.equal(c['d'], c['d'].round())
    # the stride-2 geometries leave a last row / column unread on the odd size
    assert int((R.col2im_ref(R.conv_case(R.CONV_SIZES[1], (2, 2, 2, 0)))[3] == 0).sum()) == 7 + 5 - 1
    # the ladder's cases sit where they claim to
    from phenaki_pytorch_amd.discriminator import _fast_ok
    for name, tA, tB, M, N, K, rung in R.MM_CASES:
        assert _fast_ok(M, N, K) == (name not in ('k12', 'n6')), name
        assert (rung == 'gemm') == (_fast_ok(M, N, K) and not tA), name
