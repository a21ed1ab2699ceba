"""CPU float64 restatements of the discriminator's kernels (csrc/conv.hip: pk_row_softmax, pk_row_l2scale, pk_row_ln_bwd2, pk_bmm, pk_im2col / pk_col2im, the
layout maps, pk_pick_frames) and of the product ladder of discriminator._mm_raw, in plain torch, with the seeded cases and the checkers that
tests/test_gan_kernels_gpu.py runs on the kernels' outputs.  tests/test_gan_kernels_host.py holds a float64 transcription of conv.hip's formulas to these
restatements, feeds every checker its own reference with one planted error, and evaluates every restatement in f32 on the CPU against its own bound.

Values: each operation as the reference model states it (x.softmax(-1), F.normalize(x) * sc, F.layer_norm, op(A) @ op(B), F.unfold / F.fold), its derivatives from
float64 autograd of that statement.  None of them is the kernels' algebra.

Bounds: none is taken from what a kernel returned.  U = 2^-24 is the unit roundoff of f32; a sum of n terms in any order is held to sum_bound(sum|terms|, n).
The row kernels evaluate expressions of several sums, so their bounds are pushed through those expressions by `Err`, a float64 value with a bound on the error
of its f32 evaluation: every rounded operation adds U times the magnitude of its result to what its operands carry, a row sum adds sum_bound of its terms, and
a factor in front of a sum (1 / |x|, 1 / |x|^2, 1 / sigma, S / (D sigma^2)) multiplies the sum's bound like any other operand.  The allowances:
  __expf       EXP_C units of 2^-24 plus |argument| units, the allowance on record in tests/vocab_reference.py (imported);
  1.0f / x     one U, and sqrtf one U: both are correctly rounded in the build (no fast-math flag), as tests/infer_glue_reference.py l2_ref / rms_ref count them
               ("the root, the reciprocal and the product one U each");
  constants    1e-12f, the f32 eps of the LayerNorm and 1.0f / D are f32 roundings of the numbers the reference takes in double: one U each."""
import torch
import torch.nn.functional as F

from tests.train_glue_reference import (NAN, U, assert_same_bits, assert_untouched, assert_within, assert_written, gen, strided,  # noqa: F401
                                        sum_bound)
from tests.vocab_reference import EXP_C

F64 = torch.float64
L2_EPS = 1e-12               # F.normalize's clamp


# ------------------------------------------------------------------------------------------------ error propagation

class Err:
    """v: the float64 value of an intermediate; e >= 0: a bound on |f32 evaluation - v|.  Every method that stands for a rounded f32 operation adds
    U |v| (round to nearest) to the first-order-and-beyond propagation of its operands' bounds; `exact` operations (negation, a select) add nothing."""

    def __init__(self, v, e=None):
        self.v = torch.as_tensor(v, dtype=F64)
        self.e = torch.zeros_like(self.v) if e is None else torch.as_tensor(e, dtype=F64) + torch.zeros_like(self.v)

    @staticmethod
    def of(x):
        return x if isinstance(x, Err) else Err(x)

    @staticmethod
    def const(c):
        """a double constant the kernel holds as its f32 rounding"""
        return Err(torch.tensor(c, dtype=F64), U * abs(c))

    def _rounded(self):
        return Err(self.v, self.e + U * self.v.abs())

    def __mul__(self, o):
        o = Err.of(o)
        return Err(self.v * o.v, self.v.abs() * o.e + o.v.abs() * self.e + self.e * o.e)._rounded()

    __rmul__ = __mul__

    def __add__(self, o):
        o = Err.of(o)
        return Err(self.v + o.v, self.e + o.e)._rounded()

    __radd__ = __add__

    def __sub__(self, o):
        o = Err.of(o)
        return Err(self.v - o.v, self.e + o.e)._rounded()

    def __neg__(self):
        return Err(-self.v, self.e)

    def recip(self):
        """1.0f / a: |1/(a + d) - 1/a| <= e / (|a| (|a| - e))"""
        assert (self.e < self.v.abs()).all(), 'a reciprocal whose operand may be zero'
        return Err(1.0 / self.v, self.e / (self.v.abs() * (self.v.abs() - self.e)))._rounded()

    def sqrt(self):
        """sqrtf(a), a >= 0: |sqrt(a + d) - sqrt(a)| <= e / (sqrt(a) + sqrt(max(a - e, 0))); an exact zero stays one"""
        assert (self.v >= 0).all()
        r = self.v.sqrt()
        den = r + (self.v - self.e).clamp_min(0).sqrt()
        return Err(r, torch.where(self.e > 0, self.e / den.clamp_min(1e-300), torch.zeros_like(r)))._rounded()

    def rowsum(self):
        """the f32 sum over the last axis in ANY order (lanes stride the row, then a butterfly): what the terms carry plus sum_bound(sum|terms|, n)"""
        n = self.v.shape[-1]
        return Err(self.v.sum(-1, keepdim=True), self.e.sum(-1, keepdim=True) + sum_bound(self.v.abs().sum(-1, keepdim=True), n))

    def expf(self):
        """__expf(a): the argument's error moves the value by expm1(e) relatively; the hardware exponential's own allowance is (EXP_C + |a|) U"""
        v = self.v.exp()
        return Err(v, v * (torch.expm1(self.e) + (EXP_C + self.v.abs()) * U))

    @staticmethod
    def where(cond, a, b):
        a, b = Err.of(a), Err.of(b)
        return Err(torch.where(cond, a.v, b.v), torch.where(cond, a.e + torch.zeros_like(b.e), b.e + torch.zeros_like(a.e)))


def col_bound(rows64, row_bound):
    """the two-stage column sum (pk_colsum) of M per-row contributions that each carry row_bound: their bounds add, and the sum itself is any-order over M"""
    return row_bound.sum(0) + sum_bound(rows64.abs().sum(0), rows64.shape[0])


def _grad(out, ins, create_graph=False):
    return torch.autograd.grad(out, ins, create_graph=create_graph, allow_unused=True)


def _z(g, like):
    return torch.zeros_like(like) if g is None else g


# ------------------------------------------------------------------------------------------------ pk_row_softmax

SOFTMAX_SHAPES = [(1, 1), (3, 63), (4, 64), (5, 65), (37, 256), (2, 1000)]
SOFTMAX_DATA = ['normal', 'offset', 'spread']
SOFTMAX_OFFSETS = (0., 30., -30., 1e4)
SOFTMAX_SPREAD = 60.


def softmax_case(M, n, data, seed=0):
    """x (M, n); y = the f32 rounding of its float64 softmax (what modes 1 and 2 are given); dy and c with scales 1 / 1e3 alternating between the rows (and
    the other way round for c)"""
    g = gen(21, M, n, SOFTMAX_DATA.index(data), seed)
    if data == 'normal':
        x = torch.randn(M, n, generator=g) * 1.5
    elif data == 'offset':
        x = torch.randn(M, n, generator=g) * 1.5 + torch.tensor(SOFTMAX_OFFSETS)[torch.arange(M) % 4][:, None]
    else:
        x = torch.randn(M, n, generator=g) * 0.1
        x[torch.arange(M), (torch.arange(M) * 7 + n - 1) % n] = SOFTMAX_SPREAD
    y = x.double().softmax(-1).float()
    s = torch.tensor([1., 1e3])[torch.arange(M) % 2][:, None]
    return dict(M=M, n=n, data=data, x=x, y=y, dy=torch.randn(M, n, generator=g) * s, c=torch.randn(M, n, generator=g) * (1e3 / s))


def softmax_jvp_of_output(y, dy):
    """the vector-Jacobian product of softmax written in its OUTPUT: J = diag(y) - y y^T (symmetric), applied as a matrix"""
    J = torch.diag_embed(y) - y[..., :, None] * y[..., None, :]
    return (J @ dy[..., None])[..., 0]


def softmax_ref(c):
    """float64: y0 = x.softmax(-1); b1 = J(y) dy; (g_y, g_dy) = the gradients of <c, J(y) dy> with respect to y (an independent input) and dy;
    hx = the gradient with respect to x of <c, dx>, dx = the vector-Jacobian product of x.softmax(-1) at dy: the whole chain _Softmax -> _SoftmaxBwd ->
    its backward -> _SoftmaxBwd runs when the penalty differentiates through the attention weights"""
    y0 = c['x'].double().softmax(-1)
    y = c['y'].double().requires_grad_(True)
    dy = c['dy'].double().requires_grad_(True)
    x = c['x'].double().requires_grad_(True)
    with torch.enable_grad():
        b1 = softmax_jvp_of_output(y, dy)
        g_y, g_dy = _grad((c['c'].double() * b1).sum(), (y, dy))
        dx, = torch.autograd.grad(x.softmax(-1), x, c['dy'].double(), create_graph=True)
        hx, = _grad((c['c'].double() * dx).sum(), (x,))
    return dict(y0=y0, b1=b1.detach(), g_y=g_y, g_dy=g_dy, hx=hx)


def softmax_bounds(c):
    """mode 0: d = x - max (one rounding), p = __expf(d), s = sum p, y = p (1 / s).  mode 1: r = sum(y dy), out = y (dy - r).
    mode 2: q = sum(c y), out = c (dy - r) - dy q; its second return is mode 1 at (y, c)"""
    x = Err(c['x'])
    d = x - Err(c['x'].double().max(-1, keepdim=True).values)
    p = d.expf()
    y0 = p * p.rowsum().recip()
    y, dy, cc = Err(c['y']), Err(c['dy']), Err(c['c'])
    r = (y * dy).rowsum()
    b1 = y * (dy - r)
    q = (cc * y).rowsum()
    g_y = cc * (dy - r) - dy * q
    g_dy = y * (cc - q)
    # the chain from x: the same three expressions at the kernel's OWN y0 (it carries mode 0's bound), then mode 1 at (y0, G)
    G = cc * (dy - (y0 * dy).rowsum()) - dy * (cc * y0).rowsum()
    hx = y0 * (G - (y0 * G).rowsum())
    return dict(y0=y0.e, b1=b1.e, g_y=g_y.e, g_dy=g_dy.e, hx=hx.e)


def softmax_f32(c, order=0, drop_q=False):
    """the restatement in f32 on the CPU, sums in one of two association orders; drop_q: the wrong kernel without the -b <c, a> term of mode 2"""
    from tests.infer_glue_reference import sum32
    x, y, dy, cc = c['x'], c['y'], c['dy'], c['c']
    p = torch.exp(x - x.max(-1, keepdim=True).values)
    r, q = sum32(y * dy, order)[:, None], sum32(cc * y, order)[:, None]
    y0 = p * (1.0 / sum32(p, order))[:, None]
    G = cc * (dy - sum32(y0 * dy, order)[:, None]) - (0 if drop_q else dy * sum32(cc * y0, order)[:, None])
    return dict(y0=y0, b1=y * (dy - r), g_y=cc * (dy - r) - (0 if drop_q else dy * q), g_dy=y * (cc - q), hx=y0 * (G - sum32(y0 * G, order)[:, None]))


def softmax_check(c, outs):
    """outs: any of y0, b1, g_y, g_dy, hx (M, n).  Returns the largest err / bound of each"""
    ref, bound = softmax_ref(c), softmax_bounds(c)
    return {k: assert_within(outs[k], ref[k], bound[k], f'row_softmax {k} ({c["data"]} {c["M"]}x{c["n"]})') for k in outs}


# ------------------------------------------------------------------------------------------------ pk_row_l2scale

L2_SHAPES = [(1, 1), (3, 4), (130, 64), (5, 70), (2, 200)]
L2_PLANTED = dict(zero=0., below=3e-14, above=1e-11)          # row norms: exactly 0, under the clamp, just over it


def l2_case(M, d, seed=0):
    """random rows, every third scaled by 1e-6 and every third by 1e6; with M >= 5 rows 0, 3 and M - 1 are the planted zero / below / above rows (rows 1 and 2 keep the scales 1e-6 and 1e6).  With M < 5 the
    planted rows REPLACE the random ones in a second case (l2_cases) so that the smallest shapes see them too"""
    g = gen(22, M, d, seed)
    x = torch.randn(M, d, generator=g) * torch.tensor([1., 1e-6, 1e6])[torch.arange(M) % 3][:, None]
    c = dict(M=M, d=d, x=x, sc=1 + 0.3 * torch.randn(d, generator=g), dz=torch.randn(M, d, generator=g), gx=torch.randn(M, d, generator=g),
             gsc=torch.randn(d, generator=g), planted={})
    if M >= 5:
        for i, (k, nrm) in zip((0, 3, M - 1), L2_PLANTED.items()):
            plant_l2_row(c, i, k, nrm)
    return c


def plant_l2_row(c, i, kind, nrm):
    r = c['x'][i].double()
    r = r / r.norm() * nrm if nrm else r * 0
    c['x'][i] = r.float()
    c['planted'][kind] = i


def l2_cases(M, d):
    """the case of the shape and, where the shape has fewer than 5 rows, one case per planted row kind (in row 0)"""
    out = [l2_case(M, d)]
    if M < 5:
        for k, (kind, nrm) in enumerate(L2_PLANTED.items()):
            c = l2_case(M, d, seed=k + 1)
            plant_l2_row(c, 0, kind, nrm)
            out.append(c)
    return out


def l2scale(x, sc, eps=L2_EPS):
    """F.normalize(x, dim=-1, eps) * sc = x / max(|x|, eps) * sc as two smooth branches: normalised where |x| >= eps, x sc / eps below (the normaliser is
    the constant there).  sc: (d,) or a per-row copy (M, d).  At x = 0 this is the reference's limit; its own double backward is NaN there"""
    nrm = x.detach().norm(dim=-1, keepdim=True)
    safe = torch.where(nrm >= eps, x, torch.ones_like(x))            # keeps the unused branch's autograd finite
    return torch.where(nrm >= eps, safe / safe.norm(dim=-1, keepdim=True), x / eps) * sc


def l2_ref(c):
    """float64, sc as a per-row copy so that the rows' contributions are separable: z; mode 1 (dx, dsc_rows) at dz; mode 2 (grad_x, grad_sc_rows, grad_dz) =
    the gradients of <gx, dx> + <gsc, sum_rows dsc_rows>"""
    M, d = c['M'], c['d']
    x = c['x'].double().requires_grad_(True)
    scr = c['sc'].double().expand(M, d).clone().requires_grad_(True)
    dz = c['dz'].double().requires_grad_(True)
    with torch.enable_grad():
        z = l2scale(x, scr)
        dx, dsc_rows = _grad((z * dz).sum(), (x, scr), create_graph=True)
        obj = (c['gx'].double() * dx).sum() + (c['gsc'].double() * dsc_rows).sum()
        grad_x, grad_sc_rows, grad_dz = _grad(obj, (x, scr, dz))
    return dict(z=z.detach(), dx=dx.detach(), dsc_rows=dsc_rows.detach(), grad_x=_z(grad_x, x), grad_sc_rows=_z(grad_sc_rows, x), grad_dz=_z(grad_dz, x))


def l2_bounds(c):
    """ss = sum x^2, |x| = max(sqrtf(ss), 1e-12f), inv = 1 / |x|, u = x inv, t = dz sc, a = sum(u dz sc), b = sum(gx u), gt = sum(gx t), e3 = sum(u gsc dz).
    At or above the clamp:  z = u sc;  dx = (t - u a) inv, dsc_rows = dz u;  grad_dz = sc (gx - u b) inv + gsc u,  grad_sc_rows = dz (gx - u b) inv,
      grad_x = -((a gx + b t) - u (a b + b a) + u (gt - b a)) inv inv + (gsc dz - u e3) inv  -- the sums a, b, gt, e3 enter grad_x times 1 / |x|^2 and 1 / |x|.
    Below it (inv = 1 / 1e-12f, a constant):  dx = t inv;  grad_dz = sc gx inv + gsc u,  grad_sc_rows = dz gx inv,  grad_x = gsc dz inv"""
    x, sc, dz, gx, gsc = (Err(c[k]) for k in ('x', 'sc', 'dz', 'gx', 'gsc'))
    root = (x * x).rowsum().sqrt()
    below = root.v < L2_EPS
    inv = Err.where(below, Err.const(L2_EPS), root).recip()
    u, t = x * inv, dz * sc
    z = u * sc
    a = (u * dz * sc).rowsum()
    b, gt, e3 = (gx * u).rowsum(), (gx * dz * sc).rowsum(), (u * gsc * dz).rowsum()
    pg = gx - u * b
    e1, e2 = a * b + b * a, gt - b * a
    pw = (a * gx + b * t) - u * e1
    out = dict(z=z, dsc_rows=dz * u,
               dx=Err.where(below, t * inv, (t - u * a) * inv),
               grad_dz=Err.where(below, sc * gx * inv + gsc * u, sc * pg * inv + gsc * u),
               grad_sc_rows=Err.where(below, dz * gx * inv, dz * pg * inv),
               grad_x=Err.where(below, gsc * dz * inv, -(pw + u * e2) * inv * inv + (gsc * dz - u * e3) * inv))
    return {k: v.e for k, v in out.items()}


def l2_f32(c, order=0):
    """the restatement's closed form in f32 on the CPU (F.normalize's own derivative: the projection above the clamp, the linear map below it)"""
    from tests.infer_glue_reference import sum32
    x, sc, dz, gx, gsc = (c[k] for k in ('x', 'sc', 'dz', 'gx', 'gsc'))
    s = lambda t: sum32(t, order)[:, None]                                    # noqa: E731
    root = torch.sqrt(s(x * x))
    below = root < L2_EPS
    inv = 1.0 / torch.where(below, torch.tensor(L2_EPS), root)
    u, t = x * inv, dz * sc
    a, b, e3 = s(u * t), s(gx * u), s(u * gsc * dz)
    pg = gx - u * b
    curv = -((a * gx + b * t) - u * (2 * a * b) + u * (s(gx * t) - a * b)) * inv * inv + (gsc * dz - u * e3) * inv
    return dict(z=u * sc, dsc_rows=dz * u, dx=torch.where(below, t * inv, (t - u * a) * inv),
                grad_dz=torch.where(below, sc * gx * inv, sc * pg * inv) + gsc * u, grad_sc_rows=torch.where(below, dz * gx * inv, dz * pg * inv),
                grad_x=torch.where(below, gsc * dz * inv, curv))


def l2_check(c, outs, dsc=None, grad_sc=None):
    """outs: any of z, dx, dsc_rows, grad_x, grad_sc_rows, grad_dz (M, d); dsc / grad_sc (d,): the column sums of the per-row outputs.
    Returns the largest err / bound of each"""
    ref, bound = l2_ref(c), l2_bounds(c)
    what = f'row_l2scale {{}} ({c["M"]}x{c["d"]})'
    got = {k: assert_within(outs[k], ref[k], bound[k], what.format(k)) for k in outs}
    for name, v, rows in (('dsc', dsc, 'dsc_rows'), ('grad_sc', grad_sc, 'grad_sc_rows')):
        if v is not None:
            got[name] = assert_within(v, ref[rows].sum(0), col_bound(ref[rows], bound[rows]), what.format(name))
    return got


# ------------------------------------------------------------------------------------------------ pk_row_ln_bwd2

LN_SHAPES = [(1, 1), (3, 64), (133, 128), (5, 70), (6, 512)]
LN_EPS = [1e-5, 1e-3]


def ln_case(M, D, seed=0):
    """random rows; row 0 constant (sigma = sqrt(eps), x^ = 0) in a second case of the single-row shape, row 1 constant and row 2 of mean 1e3 / unit spread
    otherwise; gamma with a zero and a negative entry (D >= 2); w not zero"""
    g = gen(23, M, D, seed)
    x = torch.randn(M, D, generator=g) * 1.5
    planted = {}
    if M > 2:
        x[1] = 0.7
        x[2] = 1e3 + torch.randn(D, generator=g)
        planted = dict(constant=1, offset=2)
    elif seed:
        x[0] = 0.7
        planted = dict(constant=0)
    gamma = 1 + 0.3 * torch.randn(D, generator=g)
    if D >= 2:
        gamma[0], gamma[D // 2] = 0., -0.8
    return dict(M=M, D=D, x=x, gamma=gamma, dy=torch.randn(M, D, generator=g), u=torch.randn(M, D, generator=g), w=torch.randn(D, generator=g),
                planted=planted)


def ln_cases(M, D):
    return [ln_case(M, D)] + ([ln_case(M, D, seed=1)] if M <= 2 else [])


def ln_ref(c, eps):
    """float64 F.layer_norm with a per-row copy of gamma: (dx, dgamma_rows) at dy, then the gradients of <u, dx> + <w, sum_rows dgamma_rows>"""
    M, D = c['M'], c['D']
    x = c['x'].double().requires_grad_(True)
    gr = c['gamma'].double().expand(M, D).clone().requires_grad_(True)
    dy = c['dy'].double().requires_grad_(True)
    with torch.enable_grad():
        xh = F.layer_norm(x, (D,), None, None, eps)
        dx, dg_rows = _grad((xh * gr * dy).sum(), (x, gr), create_graph=True)
        obj = (c['u'].double() * dx).sum() + (c['w'].double() * dg_rows).sum()
        grad_x, gg_rows, grad_dy = _grad(obj, (x, gr, dy))
    return dict(dx=dx.detach(), dg_rows=dg_rows.detach(), grad_x=_z(grad_x, x), grad_gamma_rows=_z(gg_rows, x), grad_dy=_z(grad_dy, x))


def ln_bounds(c, eps):
    """mu = sum(x) (1 / D), cen = x - mu, sigma = sqrtf(sum(cen^2) (1 / D) + eps), is = 1 / sigma, x^ = cen is, g^ = dy gamma; the five means c1 = mean u,
    c2 = mean(u x^), m1 = mean g^, m2 = mean(g^ x^) and ug = sum(u g^); S = ug - D c1 m1 - D c2 m2; v = -(m2 u + c2 g^) is + w dy, v1 = mean v, v2 = mean(v x^);
    gg = (u - c1 - x^ c2) is;  grad_dy = gamma gg + w x^,  grad_gamma_rows = dy gg,  grad_x = (v - v1 - x^ v2) is - S is is x^ (1 / D): every row sum's bound
    reaches the outputs times 1 / sigma, and S's times 1 / (D sigma^2)"""
    D = c['D']
    x, gamma, dy, u, w = (Err(c[k]) for k in ('x', 'gamma', 'dy', 'u', 'w'))
    invD, Df = Err.const(1.0 / D), float(D)
    mu = x.rowsum() * invD
    cen = x - mu
    isg = ((cen * cen).rowsum() * invD + Err.const(eps)).sqrt().recip()
    xh, gh = cen * isg, dy * gamma
    c1, c2, m1, m2 = u.rowsum() * invD, (u * xh).rowsum() * invD, gh.rowsum() * invD, (gh * xh).rowsum() * invD
    S = (u * gh).rowsum() - Df * c1 * m1 - Df * c2 * m2
    v = -(m2 * u + c2 * gh) * isg + w * dy
    v1, v2 = v.rowsum() * invD, (v * xh).rowsum() * invD
    gg = (u - c1 - xh * c2) * isg
    out = dict(grad_dy=gamma * gg + w * xh, grad_gamma_rows=dy * gg, grad_x=(v - v1 - xh * v2) * isg - S * isg * isg * xh * invD)
    return {k: t.e for k, t in out.items()}


def ln_f32(c, eps, order=0, no_eps=False):
    """F.layer_norm's second-order closed form in f32 on the CPU; no_eps: the wrong kernel that ignores eps"""
    from tests.infer_glue_reference import sum32
    D = c['D']
    x, gamma, dy, u, w = (c[k] for k in ('x', 'gamma', 'dy', 'u', 'w'))
    mean = lambda t: sum32(t, order)[:, None] / D                              # noqa: E731
    cen = x - mean(x)
    isg = 1.0 / torch.sqrt(mean(cen * cen) + (0. if no_eps else eps))
    xh, gh = cen * isg, dy * gamma
    c1, c2, m1, m2 = mean(u), mean(u * xh), mean(gh), mean(gh * xh)
    S = mean(u * gh) - c1 * m1 - c2 * m2
    v = -(m2 * u + c2 * gh) * isg + w * dy
    gg = (u - c1 - xh * c2) * isg
    return dict(grad_dy=gamma * gg + w * xh, grad_gamma_rows=dy * gg, grad_x=(v - mean(v) - xh * mean(v * xh)) * isg - S * isg * isg * xh)


def ln_check(c, eps, outs, grad_gamma=None):
    """outs: grad_x, grad_gamma_rows, grad_dy (M, D); grad_gamma (D,): the column sum of the per-row output"""
    ref, bound = ln_ref(c, eps), ln_bounds(c, eps)
    what = f'row_ln_bwd2 {{}} ({c["M"]}x{c["D"]} eps {eps:g})'
    got = {k: assert_within(outs[k], ref[k], bound[k], what.format(k)) for k in outs}
    if grad_gamma is not None:
        rows = ref['grad_gamma_rows']
        got['grad_gamma'] = assert_within(grad_gamma, rows.sum(0), col_bound(rows, bound['grad_gamma_rows']), what.format('grad_gamma'))
    return got


# ------------------------------------------------------------------------------------------------ pk_bmm

BMM_SHAPES = [(1, 1, 1, 1), (3, 70, 33, 19), (2, 64, 64, 16), (2, 65, 63, 17), (1, 2, 1, 8192), (4, 5, 130, 64)]          # (Z, M, N, K)
BMM_PADS = (3, 1, 2)                                                                                                      # lda, ldb, ldc
BMM_OFFSET = 5                # elements in front of A and B in the `views` layout


def bmm_case(Z, M, N, K, tA, tB, layout='plain', data='rand', seed=0):
    """layout: plain (leading dimensions = widths) | padded (lda / ldb / ldc wider by BMM_PADS, NaN in the pads) | shared (sB = 0: one B for every batch) |
    views (A and B start BMM_OFFSET elements into a longer NaN-filled buffer).  data: rand | grid (integers -8 .. 8 times multiples of 1/16 in -1 .. 1: every
    product is a multiple of 1/16 below 8, so every partial sum of K <= 8192 of them, with the grid C0 added, is exact in f32).
    A (Z, rows, lda) holds op(A)'s storage, C0 (Z, M, ldc) the random start of the accumulate pass"""
    g = gen(24, Z, M, N, K, int(tA), int(tB), ('plain', 'padded', 'shared', 'views').index(layout), int(data == 'grid'), seed)
    pa, pb, pc = BMM_PADS if layout == 'padded' else (0, 0, 0)
    ar, ac = (K, M) if tA else (M, K)
    br, bc = (N, K) if tB else (K, N)
    zb = 1 if layout == 'shared' else Z

    def draw(z, r, cols, ints):
        if data == 'grid':
            return (torch.randint(-8, 9, (z, r, cols), generator=g) if ints else torch.randint(-16, 17, (z, r, cols), generator=g) / 16.).float()
        return torch.randn(z, r, cols, generator=g)

    def widen(t, pad):
        buf = torch.full((t.shape[0], t.shape[1], t.shape[2] + pad), NAN)
        buf[:, :, :t.shape[2]] = t
        return buf
    A, B, C0 = widen(draw(Z, ar, ac, True), pa), widen(draw(zb, br, bc, False), pb), widen(draw(Z, M, N, True), pc)
    return dict(Z=Z, M=M, N=N, K=K, tA=tA, tB=tB, layout=layout, data=data, A=A, B=B, C0=C0, lda=ac + pa, ldb=bc + pb, ldc=N + pc,
                sA=ar * (ac + pa), sB=0 if layout == 'shared' else br * (bc + pb), sC=M * (N + pc), offset=BMM_OFFSET if layout == 'views' else 0)


def bmm_operands(c):
    """op(A[z]) (Z, M, K) and op(B[z]) (Z, K, N) in float64, read from the flat storage through lda / ldb / sA / sB as the kernel is told to"""
    def read(buf, ld, s, rows, cols, t):
        flat = buf.reshape(-1).double()
        z = torch.arange(c['Z'])[:, None, None]
        i, j = torch.arange(rows)[None, :, None], torch.arange(cols)[None, None, :]
        return flat[z * s + (j * ld + i if t else i * ld + j)]
    return read(c['A'], c['lda'], c['sA'], c['M'], c['K'], c['tA']), read(c['B'], c['ldb'], c['sB'], c['K'], c['N'], c['tB'])


def bmm_ref(c, accumulate=False):
    """(C, bound) (Z, M, N): sum_bound(sum_k |a| |b|, K); the accumulate pass adds C0 with one more rounding of the result"""
    a, b = bmm_operands(c)
    C = a @ b
    bound = sum_bound(a.abs() @ b.abs(), c['K'])
    if accumulate:
        C = C + c['C0'][:, :, :c['N']].double()
        bound = bound + U * C.abs()
    return C, bound


def bmm_grid_units(c):
    """the largest sum of |terms| (C0 included) in units of the grid, 1/16: below 2^24 every partial sum in any order is an exact f32"""
    a, b = bmm_operands(c)
    return float(((a.abs() @ b.abs()) + c['C0'][:, :, :c['N']].double().abs()).max() * 16)


def bmm_f32(c, accumulate=False):
    """a serial f32 chain, k descending (the kernel's runs ascending)"""
    a, b = (t.float() for t in bmm_operands(c))
    acc = torch.zeros(c['Z'], c['M'], c['N'])
    for k in reversed(range(c['K'])):
        acc = acc + a[:, :, k, None] * b[:, k, None, :]
    return c['C0'][:, :, :c['N']] + acc if accumulate else acc


def bmm_check(c, Cbuf, accumulate=False):
    """Cbuf (Z, M, ldc) after the call: pre-filled with NaN (plain pass) or holding C0 with NaN pads (accumulate pass)"""
    N = c['N']
    ref, bound = bmm_ref(c, accumulate)
    what = f'bmm {c["Z"]}x{c["M"]}x{c["N"]}x{c["K"]} tA={c["tA"]} tB={c["tB"]} {c["layout"]} {c["data"]}' + (' accumulate' if accumulate else '')
    assert_untouched(Cbuf[:, :, N:], f'{what}: the pad columns of C')
    if c['data'] == 'grid':
        assert_same_bits(Cbuf[:, :, :N].contiguous(), ref.float(), f'{what}: exact on the grid')
        return 0.
    return assert_within(Cbuf[:, :, :N], ref, bound, what)


# ------------------------------------------------------------------------------------------------ pk_im2col / pk_col2im

CONV_GEOMS = [(3, 3, 1, 1), (1, 1, 2, 0), (2, 2, 2, 0), (3, 3, 2, 1), (3, 1, 1, 0), (1, 3, 1, 0)]          # (kh, kw, stride, pad)
CONV_SIZES = [(2, 6, 10, 8), (1, 7, 5, 4), (2, 1, 1, 4)]                                                  # (B, H, W, C)
CONV_LD_PAD = 4


def conv_out(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def conv_case(size, geom, data='rand', seed=0):
    """None when the kernel does not fit the image.  x (B H W, C) pixel rows, d (B Ho Wo, kh kw C) an upstream patch matrix; grid: integers -8 .. 8 (at most
    kh kw = 9 taps of magnitude 8 per pixel: exact in f32 in any order)"""
    B, H, W, C = size
    kh, kw, stride, pad = geom
    Ho, Wo = conv_out(H, kh, stride, pad), conv_out(W, kw, stride, pad)
    if Ho <= 0 or Wo <= 0:
        return None
    g = gen(25, *size, *geom, int(data == 'grid'), seed)
    draw = (lambda *s: torch.randint(-8, 9, s, generator=g).float()) if data == 'grid' else (lambda *s: torch.randn(*s, generator=g))
    return dict(size=size, geom=geom, Ho=Ho, Wo=Wo, data=data, x=draw(B * H * W, C), d=draw(B * Ho * Wo, kh * kw * C))


def conv_tap_index(c):
    """(m, tap) -> the pixel row it reads, or -1 outside the image: the index arithmetic of a convolution, restated"""
    B, H, W, C = c['size']
    kh, kw, stride, pad = c['geom']
    Ho, Wo = c['Ho'], c['Wo']
    m = torch.arange(B * Ho * Wo)
    b, yo, xo = m // (Ho * Wo), (m // Wo) % Ho, m % Wo
    tap = torch.arange(kh * kw)
    y = yo[:, None] * stride + (tap // kw)[None] - pad
    x = xo[:, None] * stride + (tap % kw)[None] - pad
    inside = (y >= 0) & (y < H) & (x >= 0) & (x < W)
    return torch.where(inside, (b[:, None] * H + y) * W + x, torch.full_like(y, -1))


def im2col_ref(c):
    """(F.unfold in the column order (ky, kx, c), the same by index arithmetic): two references that must agree bit for bit -- a gather rounds nothing"""
    B, H, W, C = c['size']
    kh, kw, stride, pad = c['geom']
    u = F.unfold(c['x'].double().reshape(B, H, W, C).permute(0, 3, 1, 2), (kh, kw), padding=pad, stride=stride)
    a = u.reshape(B, C, kh * kw, c['Ho'] * c['Wo']).permute(0, 3, 2, 1).reshape(B * c['Ho'] * c['Wo'], kh * kw * C)
    idx = conv_tap_index(c)
    xz = torch.cat([c['x'].double(), torch.zeros(1, C, dtype=F64)])           # index -1 reads the zero row
    return a, xz[idx].reshape(idx.shape[0], kh * kw * C)


def col2im_ref(c, skip_tap=None):
    """(F.fold of d in float64, the same by index arithmetic, the bound, the number of taps that read each pixel).  The bound is sum_bound over those taps
    (extra = 0: the terms are inputs, nothing is rounded before the adds).  skip_tap: the wrong kernel that forgets one tap"""
    B, H, W, C = c['size']
    kh, kw, stride, pad = c['geom']
    d = c['d'].double()
    f = F.fold(d.reshape(B, c['Ho'] * c['Wo'], kh * kw, C).permute(0, 3, 2, 1).reshape(B, C * kh * kw, c['Ho'] * c['Wo']), (H, W), (kh, kw), padding=pad,
               stride=stride).permute(0, 2, 3, 1).reshape(B * H * W, C)
    idx = conv_tap_index(c)
    if skip_tap is not None:
        idx = idx.clone()
        idx[:, skip_tap] = -1
    flat = torch.where(idx >= 0, idx, torch.full_like(idx, B * H * W)).reshape(-1)
    terms = d.reshape(-1, C)
    z = torch.zeros(B * H * W + 1, C, dtype=F64)
    a = z.clone().index_add_(0, flat, terms)[:-1]
    taps = torch.bincount(flat, minlength=B * H * W + 1)[:-1]
    bound = sum_bound(z.clone().index_add_(0, flat, terms.abs())[:-1], 1, extra=0) * taps[:, None].clamp_min(1)
    return f, a, bound, taps


def conv_check(c, cols, dx, ld_pad):
    """cols (B Ho Wo, kh kw C + ld_pad) and dx (B H W, C) pre-filled with NaN.  Returns col2im's largest err / bound"""
    kh, kw = c['geom'][:2]
    width = kh * kw * c['size'][3]
    what = f'{c["size"]} {c["geom"]} ld + {ld_pad} {c["data"]}'
    assert_same_bits(cols[:, :width].contiguous(), im2col_ref(c)[0].float(), f'im2col {what}')
    assert_untouched(cols[:, width:], f'im2col {what}: the pad columns')
    fold, _, bound, taps = col2im_ref(c)
    assert_written(dx, f'col2im {what}')
    never = taps == 0
    assert_same_bits(dx[never], torch.zeros_like(dx[never]), f'col2im {what}: the pixels no patch reads')
    if c['data'] == 'grid':
        assert_same_bits(dx, fold.float(), f'col2im {what}: exact on the grid')
        return 0.
    return assert_within(dx, fold, bound, f'col2im {what}')


# ------------------------------------------------------------------------------------------------ the layout maps and pk_pick_frames

LAYOUT_C = [(1, 4), (3, 4), (4, 4), (1, 8), (3, 8), (4, 8)]          # (C, Cp)
LAYOUT_HW = [(2, 2), (6, 8)]                                         # H W = 4 and 48
PICK_F = [1, 5]


def rows_of_image(img, Cp):
    """(B, C, H, W) -> (B H W, Cp) pixel rows, the padding channels zero"""
    B, C, H, W = img.shape
    rows = torch.zeros(B * H * W, Cp, dtype=img.dtype)
    rows[:, :C] = img.permute(0, 2, 3, 1).reshape(-1, C)
    return rows


def pick_ref(video, frame):
    """img[b] = video[b, :, frame[b]]"""
    return torch.stack([video[b, :, int(frame[b])] for b in range(video.shape[0])])


def place_ref(img, frame, F_):
    B, C, H, W = img.shape
    v = torch.zeros(B, C, F_, H, W, dtype=img.dtype)
    for b in range(B):
        v[b, :, int(frame[b])] = img[b]
    return v


# ------------------------------------------------------------------------------------------------ the product ladder of discriminator._mm_raw

# (name, tA, tB, M, N, K, the rung that must take it): pk_gemm at the smallest admitted shape, the two shapes next to it that pk_gemm refuses, the split-K
# A^T B rung at its smallest admitted K = 4 k-tiles of 32 and one 8 below it, A^T B with M % 4 != 0
MM_CASES = [('gemm_min', False, False, 16, 8, 8, 'gemm'), ('gemm_min_tB', False, True, 16, 8, 8, 'gemm'), ('k12', False, False, 16, 8, 12, 'bmm'),
            ('n6', False, False, 16, 6, 8, 'bmm'), ('splitk_min', True, False, 16, 8, 128, 'splitk'), ('splitk_below', True, False, 16, 8, 120, 'bmm'),
            ('tA_m18', True, False, 18, 8, 128, 'bmm'), ('tA_tB', True, True, 16, 8, 128, 'bmm')]
MM_BATCHED = (3, 5, 9, 7)                 # (Z, M, N, K) of the 3-D rung


def mm_case(tA, tB, M, N, K, Z=None, seed=0):
    g = gen(26, int(tA), int(tB), M, N, K, Z or 0, seed)
    lead = () if Z is None else (Z,)
    return dict(tA=tA, tB=tB, M=M, N=N, K=K, Z=Z, A=torch.randn(*lead, *((K, M) if tA else (M, K)), generator=g),
                B=torch.randn(*lead, *((N, K) if tB else (K, N)), generator=g), dC=torch.randn(*lead, M, N, generator=g))


def _op(t, flag):
    return t.transpose(-1, -2) if flag else t


def mm_ref(A, B, tA, tB):
    """(op(A) @ op(B) in float64, sum_bound(sum|a||b|, K))"""
    a, b = _op(A.double(), tA), _op(B.double(), tB)
    return a @ b, sum_bound(a.abs() @ b.abs(), a.shape[-1])


def mm_backward_calls(c):
    """the two products _MM.backward forms for (A, B, tA, tB) at upstream dC, as (name, X, Y, tX, tY): dA and dB in the operands' own layouts"""
    A, B, dC, tA, tB = c['A'], c['B'], c['dC'], c['tA'], c['tB']
    return [('dA', dC, B, False, not tB) if not tA else ('dA', B, dC, tB, True), ('dB', A, dC, not tA, False) if not tB else ('dB', dC, A, True, tA)]


def mm_backward_ref(c):
    """dA, dB of <dC, op(A) op(B)> by float64 autograd"""
    A, B = c['A'].double().requires_grad_(True), c['B'].double().requires_grad_(True)
    with torch.enable_grad():
        return dict(zip(('dA', 'dB'), _grad((_op(A, c['tA']) @ _op(B, c['tB']) * c['dC'].double()).sum(), (A, B))))
