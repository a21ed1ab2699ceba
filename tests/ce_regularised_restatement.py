"""CPU float64 restatement of the regularised masked-token objective (label smoothing eps, z-loss weight zeta) of csrc/sampler.hip --
pk_vocab_weight_mean, pk_vocab_ce_reg, pk_ce_grad_slab_reg -- in plain torch, with the checkers tests/test_ce_regularised_gpu.py runs on the kernels'
outputs.  tests/test_ce_regularised_host.py holds the restatement to float64 autograd of F.cross_entropy(label_smoothing=) + zeta mean(logsumexp^2) and
feeds every checker its own reference with one planted error.

    loss_m = lse_m - (1 - eps) z_m[t_m] - eps zbar_m + zeta lse_m^2,      zbar_m = mean_v z_m[v] = A_m . wbar + bbar
    g_m[v] = scale (p_m[v] (1 + 2 zeta lse_m) - (1 - eps) [v = t_m] - eps / V),      p = exp(z - lse),  V the WHOLE vocabulary

Every bound is derived from the operation or is a tolerance the project already holds the plain kernels to, never what a kernel returned.  eps and zeta
reach the kernels as f32 arguments: the restatement takes their f32 values (an input, not an error of the kernel), as train_glue_reference does for scale."""
import torch
import torch.nn.functional as F

from tests import train_glue_reference as R
from tests.util import close

U = R.U
NAN = R.NAN
REGS = [(0.1, 0.), (0., 1e-2), (0.1, 1e-2)]                                   # (label_smoothing, z_loss_weight)
MODES = ['f32', 'bf16x3', 'bf16']
VOCAB_CE_TOL = {'f32': 2e-5, 'bf16x3': 4e-5, 'bf16': 2e-3}                  # tests/test_kernels_gpu.py::test_vocab_ce_matches_cross_entropy, through `close`
AUTOGRAD_TOL = {'fp32': 1e-3, 'bf16x3': 1e-3, 'bf16': 3e-2}                 # test_vocab_cross_entropy_backward_matches_reference_autograd


def f32(x):
    """the value of a python float as the f32 argument the C ABI passes"""
    return float(torch.tensor(x, dtype=torch.float32))


def bf(t):
    return t.to(torch.bfloat16).float()


# ------------------------------------------------------------------------------------------------ the objective and its gradient, from the logits

def autograd_objective(z, t, eps, zeta):
    """the definition: torch's label-smoothed cross entropy plus the PaLM z-loss, mean over the rows"""
    return F.cross_entropy(z, t, label_smoothing=eps) + zeta * (torch.logsumexp(z, 1) ** 2).mean()


def loss_rows(z, t, eps, zeta):
    """(loss_m, lse_m) in float64 from the (M, V) logits"""
    z = z.double()
    lse = torch.logsumexp(z, 1)
    return lse - (1 - eps) * z.gather(1, t[:, None]).squeeze(1) - eps * z.mean(1) + zeta * lse ** 2, lse


def loss_rows_head(A, W, b, t, eps, zeta):
    """the same, as the kernel forms it: the mean logit is ONE dot product with the column means of W (and the mean of b), no (M, V) row is averaged"""
    A, W, b = A.double(), W.double(), b.double()
    z = A @ W.t() + b
    lse = torch.logsumexp(z, 1)
    zbar = A @ W.mean(0) + b.mean()
    return lse - (1 - eps) * z.gather(1, t[:, None]).squeeze(1) - eps * zbar + zeta * lse ** 2, lse


def grad_logits(z, t, eps, zeta, scale):
    """g (M, V) float64: d (scale * sum_m loss_m) / d z"""
    z = z.double()
    lse = torch.logsumexp(z, 1, keepdim=True)
    onehot = F.one_hot(t, z.shape[1]).double()
    return scale * (torch.exp(z - lse) * (1 + 2 * zeta * lse) - (1 - eps) * onehot - eps / z.shape[1])


def rounded_operands(mode, e, W):
    """(A, W) in float64 as the mode's kernels read them: bf16 rounds both; split-bf16 keeps f32 rows and reads W as hi + lo of its two bf16 planes"""
    if mode == 'bf16':
        return bf(e).double(), bf(W).double()
    if mode == 'bf16x3':
        hi = bf(W)
        return e.double(), hi.double() + bf(W - hi).double()
    return e.double(), W.double()


def check_loss(mode, loss, lse, ref_loss, ref_lse, what):
    """per-row loss and lse against the restatement at the tolerance pk_vocab_ce is held to (the added terms: one more D-long dot product, one multiply)"""
    return dict(loss=close(loss, ref_loss.float(), VOCAB_CE_TOL[mode], f'{what} loss'), lse=close(lse, ref_lse.float(), VOCAB_CE_TOL[mode], f'{what} lse'))


# ------------------------------------------------------------------------------------------------ pk_vocab_weight_mean

WMEAN_SHAPES = [(8, 8), (264, 40), (1000, 96)]                              # (V, D)


def wmean_case(V, D, mode, seed=0):
    """W (V, D) f32 with a column offset (a mean that is not noise), bias (V,), the float64 image the kernel reads, and the K padding of the operand image"""
    g = R.gen(31, V, D, seed)
    W = torch.randn(V, D, generator=g) / D ** 0.5 * 3 + torch.linspace(-0.5, 0.5, D)[None]
    b = torch.randn(V, generator=g) * 0.1 + 0.05
    q = 64 if mode == 'bf16' else 32
    _, img = rounded_operands(mode, W[:1], W)
    return dict(V=V, D=D, mode=mode, W=W, b=b, img=img, Kp=(D + q - 1) // q * q)


def wmean_ref(c):
    """float64 means of the ROUNDED image and of the bias, each with the any-order f32 summation bound of its V terms over V"""
    img, b = c['img'], c['b'].double()
    return (img.mean(0), R.sum_bound(img.abs().sum(0), c['V']) / c['V']), (b.mean().reshape(1), R.sum_bound(b.abs().sum().reshape(1), c['V']) / c['V'])


def wmean_check(c, wbar, bbar):
    """wbar (D + pad,), bbar (1 + pad,), both pre-filled with NaN"""
    (wr, wb), (br, bb) = wmean_ref(c)
    D = c['D']
    ratios = dict(wbar=R.assert_within(wbar[:D], wr, wb, 'weight_mean wbar'), bbar=R.assert_within(bbar[:1], br, bb, 'weight_mean bbar'))
    R.assert_untouched(wbar[D:], 'weight_mean wbar beyond D')
    R.assert_untouched(bbar[1:], 'weight_mean bbar beyond its one element')
    return ratios


# ------------------------------------------------------------------------------------------------ pk_ce_grad_slab_reg

CE_SHAPES = [(77, 100, 96), (33, 40, 128), (1, 1, 32)]                      # (M, Vs, ldgt), inputs of train_glue_reference.ce_case (V_FULL = 448)


def ce_ref(c, eps, zeta, V_total=R.V_FULL, onehot_offset=None, smooth_over=None):
    """float64 g of one slab and its per-element bound.  With x = l - lse, p = exp(x), k = 1 + 2 zeta lse, a = 1 - eps, c0 = eps / V_total, s = scale:

        g = s (p k - a [v = t] - c0)

    The bound starts from train_glue_reference.ce_ref's: |s| (p (|x| + 4) 2^-22 + 2^-24) -- the rounding of the exponential's argument, of its product with
    log2(e) and the hardware exponential's last bit, all relative to p, plus one 2^-24 -- with the p-relative part multiplied by |k| (p enters g through
    p k).  Added, one unit roundoff U = 2^-24 each, relative to the value rounded:
        k:   2 zeta lse (U |2 zeta lse|) and the addition of 1 (U |k|), both carried into p k:            |s| p U (|2 zeta lse| + |k|)
        p k: the product                                                                                   |s| U |p k|
        a:   1 - eps, only at the one-hot element                                                           |s| U a [v = t]
        c0:  eps * (1 / V_total): the reciprocal and the product                                            |s| 2 U c0
        the two subtractions                                                                                |s| U (|p k - a [v = t]| + |p k - a [v = t] - c0|)
        the product with s                                                                                  U |g|
    First order in U; the second-order remainder is below 2^-20 of the bound and is covered by a factor 1 + 2^-16."""
    Vs = c['Vs']
    lse = c['lse'].double()[:, None]
    x = c['logits'][:, :Vs].double() - lse
    p = torch.exp(x)
    eps, zeta = f32(eps), f32(zeta)
    v0 = c['v0'] if onehot_offset is None else onehot_offset
    onehot = (c['row_targets'][:, None] == v0 + torch.arange(Vs)[None]).double()
    s = R.f32_scale(c['scale'], c['dev'])
    k = 1 + 2 * zeta * lse
    a, c0 = 1 - eps, eps / (V_total if smooth_over is None else smooth_over)
    pk = p * k
    t1 = pk - a * onehot
    t2 = t1 - c0
    g = s * t2
    bound = abs(s) * (p * (x.abs() + 4) * 2.0 ** -22 * k.abs() + U
                      + U * (p * ((2 * zeta * lse).abs() + k.abs()) + pk.abs() + a * onehot + 2 * c0 + t1.abs() + t2.abs())) + U * g.abs()
    return g, bound * (1 + 2.0 ** -16)


def ce_check(c, eps, zeta, g, gT, db, f32_out=None, V_total=R.V_FULL):
    """train_glue_reference.ce_check with the regularised reference: g (M, ld), gT (Vs + 2, ldgt), db (Vs + 3,), all pre-filled with NaN; f32_out = (g, gT) of
    the f32 call when g is bf16.  Returns the largest err / bound of g and of db"""
    M, Vs = c['M'], c['Vs']
    ratios = dict(g=0., db=0.)
    if g.dtype == torch.float32:
        ref, bound = ce_ref(c, eps, zeta, V_total)
        ratios['g'] = R.assert_within(g[:, :Vs], ref, bound, 'ce_grad_slab_reg g')
    else:
        assert g.dtype == torch.bfloat16 and gT.dtype == torch.bfloat16 and f32_out is not None
        R.assert_same_bits(g[:, :Vs], f32_out[0][:, :Vs].to(torch.bfloat16), 'ce_grad_slab_reg bf16 g against the rounding of the f32 g')
        R.assert_same_bits(gT[:Vs], f32_out[1][:Vs].to(torch.bfloat16), 'ce_grad_slab_reg bf16 gT against the rounding of the f32 gT')
    R.assert_untouched(g[:, Vs:], 'ce_grad_slab_reg g columns >= Vs')
    R.assert_same_bits(gT[:Vs, :M], g[:, :Vs].t().contiguous(), 'ce_grad_slab_reg gT against the transpose of g')
    R.assert_same_bits(gT[:Vs, M:], torch.zeros_like(gT[:Vs, M:]), 'ce_grad_slab_reg gT pad columns [M, ldgt)')
    R.assert_untouched(gT[Vs:], 'ce_grad_slab_reg gT rows >= Vs')
    if db is not None:
        stored = g[:, :Vs].double()
        ratios['db'] = R.assert_within(db[:Vs], stored.sum(0), R.sum_bound(stored.abs().sum(0), M), 'ce_grad_slab_reg db')
        R.assert_untouched(db[Vs:], 'ce_grad_slab_reg db beyond Vs')
    return ratios


def ce_fake(c, eps, zeta, dtype=torch.float32, ref=None):
    """what a correct kernel would leave in train_glue_reference.ce_buffers: the planted-error tests start from here"""
    g, gT, db = R.ce_buffers(c, dtype)
    M, Vs = c['M'], c['Vs']
    g[:, :Vs] = (ce_ref(c, eps, zeta)[0] if ref is None else ref).float().to(dtype)
    gT[:Vs] = 0
    gT[:Vs, :M] = g[:, :Vs].t()
    db[:Vs] = g[:, :Vs].double().sum(0).float()
    return g, gT, db


# ------------------------------------------------------------------------------------------------ vocab_cross_entropy under autograd

AG = dict(R=50, M=37, V=264, D=40, upstream=1.7)


def autograd_case(seed=0):
    """R = 50 rows of which 37 are selected (ascending, not a prefix), V = 264, D = 40, with bias; float64 autograd of the definition gives the reference"""
    g = R.gen(41, seed)
    Rn, M, V, D = AG['R'], AG['M'], AG['V'], AG['D']
    E = torch.randn(Rn, D, generator=g)
    W = torch.randn(V, D, generator=g) / D ** 0.5 * 3 + torch.linspace(-0.3, 0.3, D)[None]
    b = torch.randn(V, generator=g) * 0.1
    t = torch.randint(0, V, (Rn,), generator=g)
    rows = torch.randperm(Rn, generator=g)[:M].sort().values.int()
    assert not torch.equal(rows.long(), torch.arange(M))
    return dict(E=E, W=W, b=b, t=t, rows=rows)


def autograd_ref(c, eps, zeta, mode='fp32'):
    """loss and (dE, dW, db) of upstream * objective in float64; bf16 mode rounds the operands of the logits as the kernels do"""
    rnd = bf if mode == 'bf16' else (lambda x: x)
    E = rnd(c['E']).double().requires_grad_(True)
    W = rnd(c['W']).double().requires_grad_(True)
    b = c['b'].double().requires_grad_(True)
    sel = c['rows'].long()
    with torch.enable_grad():
        loss = autograd_objective(E[sel] @ W.t() + b, c['t'][sel], eps, zeta)
        dE, dW, db = torch.autograd.grad(loss * AG['upstream'], (E, W, b))
    return dict(loss=loss.detach(), dE=dE, dW=dW, db=db)


def autograd_check(c, ref, mode, loss, dE, dW, db):
    """the tolerances of test_vocab_cross_entropy_backward_matches_reference_autograd; rows that were not selected get exactly zero"""
    tol = AUTOGRAD_TOL[mode]
    assert abs(float(loss) - float(ref['loss'])) <= tol * abs(float(ref['loss'])), f'loss {float(loss)!r} vs {float(ref["loss"])!r} ({mode})'
    out = dict(dE=close(dE, ref['dE'].float(), tol, f'dE {mode}'), dW=close(dW, ref['dW'].float(), tol, f'dW {mode}'), db=close(db, ref['db'].float(), tol, f'db {mode}'))
    rest = torch.ones(AG['R'], dtype=torch.bool)
    rest[c['rows'].long()] = False
    assert (dE.detach().cpu()[rest] == 0).all(), 'rows that were not selected must get exactly zero gradient'
    return out


# ------------------------------------------------------------------------------------------------ the options-off step against the step without the keywords

# Two gradients of the training step are summed with float atomicAdd, in an order that is not fixed: the token embedding's (pk_embed_bwd) and the
# relative-position table's behind the position-bias MLP (pk_bias_scatter).  Two runs of the SAME model on the same draws already differ in the last bits of
# exactly those, so bit equality cannot be asked of them -- of no code, the parent's included.  The rule is the one tests/test_dropout_gpu.py holds two runs
# under one seed to: those groups within 1e-6 of the group's largest element, every other gradient and the loss bit for bit.
ATOMIC_SUMS = ('token_emb.weight', 'pos_bias.net.')


def assert_same_step(loss_a, grads_a, loss_b, grads_b, what):
    """grads: name -> tensor or None.  Returns the number of tensors held bit for bit"""
    R.assert_same_bits(loss_a.reshape(1), loss_b.reshape(1), f'{what}: loss')
    assert grads_a.keys() == grads_b.keys(), f'{what}: parameters differ'
    exact = 1
    for k in grads_a:
        a, b = grads_a[k], grads_b[k]
        assert (a is None) == (b is None), f'{what}: {k} has a gradient in one model only'
        if a is None:
            continue
        tag = next((t for t in ATOMIC_SUMS if t in k), None)
        if tag is None:
            R.assert_same_bits(a, b, f'{what}: d {k}')
            exact += 1
            continue
        group = k[:k.index(tag)] + tag
        scale = max(float(v.abs().max()) for kk, v in grads_a.items() if kk.startswith(group) and v is not None)
        err = float((a.double() - b.double()).abs().max())
        assert err <= 1e-6 * scale, f'{what}: d {k} (atomic sum): {err:.3e} > 1e-6 * {scale:.3e}'
    return exact
