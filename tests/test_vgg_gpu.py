"""The perceptual network on the GPU (csrc/vgg.hip, phenaki_pytorch_amd/vgg.py) against plain torch ops on the CPU in float64 (tests/vgg_reference.py):
the direct 3x3 convolution in its forward and backward-data forms, the pooling kernels, VGG16Features (features, input gradient, dropout, saved state)
and the perceptual term of a tokenizer GAN step.  fp32 and bf16x3 are held to tests.util.close at 1e-3; in bf16 the reference rounds the operands of
every product to bf16 where the kernels do."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle.configs import TINY
from tests import vgg_reference as R
from tests.util import close, kinked_close, record_parity

pytestmark = pytest.mark.gpu

DTYPES = ['fp32', 'bf16x3', 'bf16']
KINK_L2 = {'fp32': 5e-3, 'bf16x3': 2e-2}          # tests/test_gan_gpu.py: gradients through piecewise-linear units

# bf16, whole network: max |features - reference| / max |reference| against the reference that rounds every product's operands to bf16, measured on the
# inputs below (profiles/vgg16_perceptual.txt); the tests assert twice the value (near-tie rounding flips compound over 15 layers)
BF16_NET_MEASURED = {
    'narrow-3x32x32': 1.460e-3,
    'narrow-2x64x96': 3.594e-3,
    'narrow-1x256x256': 2.282e-3,
    'full-1x32x32': 4.217e-3,
}


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    torch.cuda.set_device(0)
    with torch.enable_grad():
        yield


def _dt(name):
    from phenaki_pytorch_amd.attention import resolve_dtype
    return resolve_dtype(name)


def g64(seed):
    return torch.Generator().manual_seed(seed)


def _r(t, dtype):
    return R.bf16_round(t) if dtype == 'bf16' else t


# ------------------------------------------------------------------------------------------------ pk_conv3x3

CONV_SHAPES = [(1, 1, 1, 8, 8), (3, 2, 2, 64, 64), (2, 5, 7, 8, 24), (1, 16, 16, 64, 128), (2, 12, 20, 128, 64), (1, 4, 4, 512, 512), (1, 33, 9, 16, 8)]


@functools.lru_cache(maxsize=None)
def _conv_case(B, H, W, C, Co):
    g = g64(B * 1000 + H * 100 + W * 10 + C)
    x = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    w = torch.randn(Co, C, 3, 3, generator=g, dtype=torch.float64) / (9 * C) ** 0.5
    b = torch.randn(Co, generator=g, dtype=torch.float64)
    gate = torch.randn(B, C, H, W, generator=g, dtype=torch.float64)
    gate[gate.abs() < 0.4] = 0.                                    # exact zeros, negatives and positives
    dy = torch.randn(B, Co, H, W, generator=g, dtype=torch.float64)
    return x, w, b, gate, dy


def _weight_image(m, dtype):
    from phenaki_pytorch_amd.train import pack_operand
    return pack_operand(m.float().cuda().contiguous(), _dt(dtype))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,H,W,C,Co', CONV_SHAPES)
def test_conv3x3_matches_conv2d(B, H, W, C, Co, dtype):
    """with and without bias, ReLU and gate, on every tile shape (64 x 64, 128 x 64, 128 x 128: all are predicated per row)"""
    from phenaki_pytorch_amd import _lib as L
    from phenaki_pytorch_amd.discriminator import _conv_matrix
    x, w, b, gate, _ = _conv_case(B, H, W, C, Co)
    Wimg = _weight_image(_conv_matrix(w, C), dtype)
    xr, gr, bias = R.rows_of(x).float().cuda(), R.rows_of(gate).float().cuda(), b.float().cuda()
    worst = 0.
    for use_bias, relu, use_gate in [(False, False, False), (True, True, False), (False, False, True), (True, True, True)]:
        xin = x * (gate > 0) if use_gate else x
        want = F.conv2d(_r(xin, dtype), _r(w, dtype), b.float().double() if use_bias else None, padding=1)
        want = R.rows_of(F.relu(want) if relu else want)
        for tile in (0, 1, 2, 3):
            y = torch.full((B * H * W, Co), float('nan'), device='cuda')
            L.conv3x3(_dt(dtype), xr, Wimg, B, H, W, C, Co, y, bias=bias if use_bias else None, relu=relu, gate=gr if use_gate else None, tile=tile)
            worst = max(worst, close(y, want, 1e-3, f'conv3x3 {dtype} bias={use_bias} relu={relu} gate={use_gate} tile={tile}'))
    if dtype == 'bf16':
        # activations in HBM as bf16: x and the gate read as bf16, y written as bf16 = the rounding of the f32 result of the same product
        xb, gb = xr.to(torch.bfloat16), gr.to(torch.bfloat16)
        want = R.rows_of(F.relu(F.conv2d(R.bf16_round(x * (gate > 0)), R.bf16_round(w), b.float().double(), padding=1)))
        y32 = L.conv3x3(_dt(dtype), xb, Wimg, B, H, W, C, Co, torch.empty((B * H * W, Co), device='cuda'), bias=bias, relu=True, gate=gb)
        worst = max(worst, close(y32, want, 1e-3, 'conv3x3 bf16 rows'))
        y16 = L.conv3x3(_dt(dtype), xb, Wimg, B, H, W, C, Co, torch.empty((B * H * W, Co), device='cuda', dtype=torch.bfloat16), bias=bias, relu=True, gate=gb)
        assert torch.equal(y16, y32.to(torch.bfloat16)), 'bf16 output is not the rounding of the f32 output'
    record_parity('vgg_conv3x3_forward', dict(dtype=dtype, shape=[B, H, W, C, Co], worst_rel_err=worst))


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('B,H,W,C,Co', CONV_SHAPES)
def test_conv3x3_backward_data_matches_autograd_of_relu_conv(B, H, W, C, Co, dtype):
    """dx = pk_conv3x3(dy, Wb, gate = relu(conv(x))) against float64 autograd of relu(conv2d(x)) (bf16: the same mask, operands rounded to bf16)"""
    from phenaki_pytorch_amd import _lib as L
    from phenaki_pytorch_amd.vgg import conv_matrix_bwd
    x, w, b, _, dy = _conv_case(B, H, W, C, Co)
    xg = x.clone().requires_grad_(True)
    y = F.relu(F.conv2d(xg, w, b, padding=1))
    if dtype == 'bf16':
        want, = torch.autograd.grad(F.conv2d(xg, R.bf16_round(w), padding=1), xg, R.bf16_round(dy * (y.detach() > 0)))
    else:
        want, = torch.autograd.grad(y, xg, dy)
    # the gate: the post-ReLU output, with every second dead unit written as a negative number instead of an exact zero (same mask)
    gate = y.detach().clone()
    dead = (gate <= 0).reshape(-1).nonzero().flatten()
    assert dead.numel() > 0 or gate.numel() < 16
    gate.view(-1)[dead[::2]] = -1.5
    gr = R.rows_of(gate).float().cuda()
    assert torch.equal(gr > 0, R.rows_of(y.detach() > 0).cuda()), 'f32 rounding changed the mask'
    if dtype == 'bf16':
        gr = gr.to(torch.bfloat16)
        assert torch.equal(gr > 0, R.rows_of(y.detach() > 0).cuda())
    Wb = _weight_image(conv_matrix_bwd(w, C), dtype)
    worst = 0.
    for tile in (0, 3):
        dx = torch.full((B * H * W, C), float('nan'), device='cuda')
        L.conv3x3(_dt(dtype), R.rows_of(dy).float().cuda(), Wb, B, H, W, Co, C, dx, gate=gr, tile=tile)
        worst = max(worst, close(dx, R.rows_of(want), 1e-3, f'conv3x3 backward-data {dtype} tile={tile}'))
    record_parity('vgg_conv3x3_backward_data', dict(dtype=dtype, shape=[B, H, W, C, Co], worst_rel_err=worst))


def test_conv3x3_refuses_bad_arguments():
    from phenaki_pytorch_amd import _lib as L
    x, y = torch.zeros(16, 8, device='cuda'), torch.zeros(16, 8, device='cuda')
    Wimg = torch.zeros(8, 96, device='cuda')
    lib, s = L.load(), L.stream(x)
    ok = lambda **k: lib.pk_conv3x3(*[k.get(n, d) for n, d in (('dtype', 0), ('a_is_f32', 1), ('x', x.data_ptr()), ('B', 1), ('H', 4), ('W', 4), ('C', 8),
                                                               ('Wm', Wimg.data_ptr()), ('ldw', 96), ('Co', 8), ('bias', None), ('act', 0), ('gate', None),
                                                               ('ldg', 0), ('gate_is_f32', 1), ('y', y.data_ptr()), ('ldy', 8), ('out_is_f32', 1), ('tile', 0),
                                                               ('stream', s))])
    assert ok() == 0
    assert ok(dtype=3) == -1 and ok(act=2) == -1 and ok(tile=4) == -1 and ok(H=0) == -1 and ok(x=None) == -1
    assert ok(ldw=72) == -1, 'W rows shorter than K rounded up to the k-tile'
    assert ok(a_is_f32=0) == -1 and ok(out_is_f32=0) == -1, 'exact f32 keeps every activation f32'
    assert ok(C=4, ldw=64) == -2 and ok(Co=6) == -2 and ok(x=x.data_ptr() + 4) == -2 and ok(gate=x.data_ptr(), ldg=12) == -2


# ------------------------------------------------------------------------------------------------ pooling

@pytest.mark.parametrize('C', [8, 64])
@pytest.mark.parametrize('H,W', [(2, 2), (6, 10), (7, 5)])
@pytest.mark.parametrize('act', [torch.float32, torch.bfloat16])
def test_maxpool_and_its_backward_are_torchs(H, W, C, act):
    """the input is the ReLU of a random tensor, so windows of four zeros occur: the backward must pick torch's element, element for element"""
    from phenaki_pytorch_amd import _lib as L
    B = 2
    g = g64(H * 10 + W + C)
    x = F.relu(torch.randn(B, C, H, W, generator=g)).to(act).double()
    assert ((F.max_pool2d(x, 2, 2) == 0).any()) or C * H * W < 64
    xg = x.clone().requires_grad_(True)
    y = F.max_pool2d(xg, 2, 2)
    dy = torch.randn(y.shape, generator=g, dtype=torch.float64).float().double()
    want_dx, = torch.autograd.grad(y, xg, dy)
    xr = R.rows_of(x).to(act).cuda()
    got = L.maxpool2x2(xr, B, H, W, C, torch.empty((B * (H // 2) * (W // 2), C), device='cuda', dtype=act))
    assert torch.equal(got.double().cpu(), R.rows_of(y.detach()))
    dx = L.maxpool2x2_bwd(xr, R.rows_of(dy).float().cuda(), B, H, W, C, torch.full((B * H * W, C), float('nan'), device='cuda'))
    assert torch.equal(dx.double().cpu(), R.rows_of(want_dx))


@pytest.mark.parametrize('H,W', [(1, 1), (2, 2), (4, 4), (7, 7), (8, 8), (8, 4)])
def test_adaptive_avgpool_and_its_backward_are_torchs(H, W):
    from phenaki_pytorch_amd import _lib as L
    B, C = 2, 16
    g = g64(H * 10 + W)
    x = torch.randn(B, C, H, W, generator=g).double().requires_grad_(True)
    y = F.adaptive_avg_pool2d(x, (7, 7))
    dy = torch.randn(y.shape, generator=g).double()
    want_dx, = torch.autograd.grad(y, x, dy)
    xr = R.rows_of(x.detach()).float().cuda()
    got = L.adaptive_avgpool(xr, B, H, W, C, torch.empty((B * 49, C), device='cuda'))
    close(got, R.rows_of(y.detach()), 1e-6, 'adaptive average pool')
    close(L.adaptive_avgpool(xr.to(torch.bfloat16), B, H, W, C, torch.empty((B * 49, C), device='cuda')),
          R.rows_of(F.adaptive_avg_pool2d(R.bf16_round(x.detach()), (7, 7))), 1e-6, 'adaptive average pool of bf16 rows')
    dx = L.adaptive_avgpool_bwd(R.rows_of(dy).float().cuda(), B, H, W, C, torch.full((B * H * W, C), float('nan'), device='cuda'))
    close(dx, R.rows_of(want_dx), 1e-6, 'adaptive average pool backward')


# ------------------------------------------------------------------------------------------------ VGG16Features

NET_CASES = {                                  # name -> (network, seed, (B, H, W))
    'narrow-3x32x32': ('narrow', 11, (3, 32, 32)),
    'narrow-2x64x96': ('narrow', 12, (2, 64, 96)),
    'narrow-1x256x256': ('narrow', 13, (1, 256, 256)),          # the 8 -> 7 adaptive pooling
    'full-1x32x32': ('full', 14, (1, 32, 32)),                  # K = 4608 and the 25088 -> 4096 Linear
}


@functools.lru_cache(maxsize=None)
def _state(kind):
    return R.random_state(**R.NARROW, seed=21) if kind == 'narrow' else R.random_state(seed=22)


@functools.lru_cache(maxsize=None)
def _net_reference(case, rounded):
    """(image, upstream gradient G, features, d <features, G> / d image) of the float64 CPU network; computed once per case, never modified"""
    kind, seed, (B, H, W) = NET_CASES[case]
    sd = _state(kind)
    g = g64(seed)
    img = torch.rand(B, 3, H, W, generator=g, dtype=torch.float64) * 2 - 1
    with torch.enable_grad():
        x = img.clone().requires_grad_(True)
        feat = R.forward(sd, x, round_bf16=rounded)
        G = torch.randn(feat.shape, generator=g, dtype=torch.float64)
        dimg, = torch.autograd.grad((feat * G).sum(), x)
    assert feat.abs().max() > 0 and dimg.abs().max() > 0
    return img, G, feat.detach(), dimg


@functools.lru_cache(maxsize=2)
def _product(kind):
    import phenaki_pytorch_amd as P
    net = P.VGG16Features(**R.NARROW) if kind == 'narrow' else P.VGG16Features()
    net.load_state_dict(_state(kind))
    return net.cuda().eval()


@pytest.mark.parametrize('dtype', DTYPES)
@pytest.mark.parametrize('case', list(NET_CASES))
def test_features_and_input_gradient(case, dtype):
    import phenaki_pytorch_amd as P
    kind = NET_CASES[case][0]
    net = P.set_compute_dtype(_product(kind), dtype)
    img, G, feat_ref, dimg_ref = _net_reference(case, dtype == 'bf16')
    x = img.float().cuda().requires_grad_(True)
    feat = net(x)
    assert feat.shape == feat_ref.shape and feat.dtype == torch.float32
    loss = (feat * G.float().cuda()).sum()
    g1, = torch.autograd.grad(loss, x, retain_graph=True)
    g2, = torch.autograd.grad(loss, x)
    assert torch.equal(g1, g2), 'two backward calls over one forward differ'
    assert g1.shape == x.shape and torch.isfinite(g1).all()
    rel_g = float((g1.double().cpu() - dimg_ref).norm() / dimg_ref.norm())
    if dtype == 'bf16':
        scale = feat_ref.abs().max().item()
        err = (feat.double().cpu() - feat_ref).abs().max().item() / scale
        record_parity('vgg_network', dict(case=case, dtype=dtype, features_rel_err_vs_rounded_reference=err, input_grad_rel_l2=rel_g))
        print(f'vgg bf16 {case}: features rel err {err:.3e} (rounded reference), input gradient rel L2 {rel_g:.3e}')
        assert torch.isfinite(feat).all()
        measured = BF16_NET_MEASURED[case]
        assert measured is not None and err <= 2 * measured, f'{case}: bf16 features {err:.3e} beyond twice the measured {measured}'
        return
    err = close(feat, feat_ref, 1e-3, f'features {case} {dtype}')
    print(f'vgg {dtype} {case}: features rel err {err:.3e}, input gradient rel L2 {rel_g:.3e}')
    record_parity('vgg_network', dict(case=case, dtype=dtype, features_rel_err=err, input_grad_rel_l2=rel_g))
    kinked_close(g1, dimg_ref, KINK_L2[dtype], f'input gradient {case} {dtype}', outliers=4 * KINK_L2[dtype])


def test_nothing_is_saved_for_an_input_without_gradient():
    import phenaki_pytorch_amd as P
    net = P.set_compute_dtype(_product('narrow'), 'fp32')
    img = _net_reference('narrow-2x64x96', False)[0].float().cuda()
    first_map = 2 * 64 * 96 * 8 * 4                                # bytes of ONE of the 13 saved activation maps (conv1_1)
    net(img)                                                       # packed weight images exist from here on
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    out = net(img)
    torch.cuda.synchronize()
    held = torch.cuda.memory_allocated() - base
    assert out.grad_fn is None and not out.requires_grad
    assert held < first_map // 8, f'{held} bytes stay allocated after a forward pass without gradient'
    with torch.no_grad():
        out2 = net(img.clone().requires_grad_(True))
    assert out2.grad_fn is None and torch.equal(out, out2)
    base = torch.cuda.memory_allocated()
    out3 = net(img.clone().requires_grad_(True))
    torch.cuda.synchronize()
    assert out3.grad_fn is not None and torch.equal(out3, out)
    assert torch.cuda.memory_allocated() - base > 2 * first_map, 'the gates of the backward pass should be held by the graph'


def test_training_mode_dropout():
    """classifier.3 = identity, so the output IS the dropped hidden row: kept fraction, survivors scaled by exactly 2, and the same mask in the backward"""
    import phenaki_pytorch_amd as P
    from phenaki_pytorch_amd.dropout import keep_mask
    sd = dict(_state('narrow'))
    hidden = R.NARROW['hidden']
    sd['classifier.3.weight'], sd['classifier.3.bias'] = torch.eye(hidden), torch.zeros(hidden)
    net = P.VGG16Features(**R.NARROW)
    net.load_state_dict(sd)
    net = P.set_compute_dtype(net.cuda(), 'fp32')
    img, G, _, _ = _net_reference('narrow-3x32x32', False)
    B = img.shape[0]
    x = img.float().cuda().requires_grad_(True)
    h1 = net.eval()(x).detach()
    assert (h1 > 0).float().mean() > 0.2
    net.train()
    torch.manual_seed(77)
    gen = torch.cuda.default_generators[0]
    seed, offset = gen.initial_seed(), gen.get_offset()
    out = net(x)
    assert gen.get_offset() == offset + 4, 'the site is drawn as the other dropout sites draw theirs'
    keep = torch.from_numpy(keep_mask(seed, offset, B, hidden, 0.5).astype(np.float32)).cuda()
    n, kept = keep.numel(), float(keep.sum())
    assert abs(kept - 0.5 * n) <= 5 * (0.25 * n) ** 0.5, f'{kept} of {n} kept at p = 128 / 256'
    assert torch.equal(out, h1 * keep * 2), 'survivors are scaled by exactly 2, the rest is zero'
    dimg, = torch.autograd.grad((out * G.float().cuda()).sum(), x)
    with torch.enable_grad():
        xr = img.clone().requires_grad_(True)
        want, = torch.autograd.grad((R.forward(sd, xr, keep=keep.double().cpu() * 2) * G).sum(), xr)
    kinked_close(dimg, want, KINK_L2['fp32'], 'input gradient under dropout', outliers=4 * KINK_L2['fp32'])
    torch.manual_seed(78)
    assert not torch.equal(net(x), out), 'another seed, another mask'
    net.eval()
    assert torch.equal(net(x), h1)


# ------------------------------------------------------------------------------------------------ the perceptual term of a tokenizer GAN step

class Recorder(torch.nn.Module):
    """clones its input, keeps the clone (with its gradient) and forwards"""

    def __init__(self, net):
        super().__init__()
        self.net, self.seen, self.grads = net, [], []

    def forward(self, x):
        x = x.clone()
        if x.requires_grad:
            x.retain_grad()
            x.register_hook(lambda g: self.grads.append(g.detach().clone()))
        self.seen.append(x)
        return self.net(x)


@pytest.mark.parametrize('dtype', DTYPES)
def test_perceptual_term_of_a_gan_step(dtype):
    import phenaki_pytorch_amd as P
    from oracle import weights
    torch.manual_seed(5)
    sd = _state('narrow')
    vgg = P.VGG16Features(**R.NARROW)
    vgg.load_state_dict(sd)
    rec = Recorder(vgg.eval())
    cv = P.CViViT(use_vgg_and_gan=True, vgg=rec, **TINY['cvivit']).cuda().train()
    vgg.eval()
    P.set_compute_dtype(cv, dtype)
    H = TINY['cvivit']['image_size']
    video = weights.synthetic_video(2, 5, H, H, seed=31).cuda()
    parts = cv.__dict__['_pk_loss_parts'] = {}
    loss = cv(video)
    loss.backward()
    assert torch.isfinite(loss)
    real, recon = rec.seen
    assert not real.requires_grad and recon.requires_grad and recon.grad is not None
    assert len(rec.grads) == 2, 'the adaptive weight differentiates the perceptual term once, loss.backward() once more'
    with torch.enable_grad():
        xr = recon.detach().double().cpu().requires_grad_(True)
        per_ref = F.mse_loss(R.forward(sd, real.detach().double().cpu()), R.forward(sd, xr))
        want, = torch.autograd.grad(per_ref, xr)
    aw = float(parts['adaptive_weight'])
    assert np.isfinite(aw) and aw != 0., 'adaptive weight'
    rel_p = abs(float(parts['perceptual']) - float(per_ref.detach())) / abs(float(per_ref.detach()))
    rel_g = float((rec.grads[1].double().cpu() - want).norm() / want.norm())
    record_parity('vgg_gan_step_perceptual', dict(dtype=dtype, perceptual=float(parts['perceptual']), ref=float(per_ref.detach()), rel_err=rel_p,
                                                  input_grad_rel_l2=rel_g, adaptive_weight=aw))
    print(f'vgg gan step {dtype}: perceptual rel err {rel_p:.3e}, input gradient rel L2 {rel_g:.3e}, adaptive weight {aw:.4g}')
    assert torch.isfinite(recon.grad).all() and torch.isfinite(parts['perceptual'])
    if dtype == 'bf16':
        return
    close(parts['perceptual'].reshape(1), per_ref.detach().reshape(1), 1e-3, 'perceptual loss')
    for gpass in rec.grads:                       # both passes see the same upstream gradient (d loss / d perceptual = 1)
        kinked_close(gpass, want, KINK_L2[dtype], f'd perceptual / d recon frame ({dtype})', outliers=4 * KINK_L2[dtype])
    assert torch.equal(recon.grad, rec.grads[0] + rec.grads[1]), 'the retained gradient accumulates both passes'
