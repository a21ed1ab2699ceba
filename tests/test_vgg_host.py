"""CPU-only checks of the perceptual network's host side (phenaki_pytorch_amd/vgg.py): the state_dict contract of torchvision's VGG16, the weight
re-orderings the kernels rely on (forward / backward-data convolution matrices in im2col column order, the classifier.0 column permutation) and the
adaptive-pool window table.  No kernel is launched here; references are plain torch ops in float64."""
import pytest
import torch
import torch.nn.functional as F

from tests import vgg_reference as R

# torchvision.models.vgg16().state_dict() with classifier = classifier[:-2] (reference cvivit.py:349-352), written out
TORCHVISION_VGG16 = [
    ('features.0.weight', (64, 3, 3, 3)), ('features.0.bias', (64,)),
    ('features.2.weight', (64, 64, 3, 3)), ('features.2.bias', (64,)),
    ('features.5.weight', (128, 64, 3, 3)), ('features.5.bias', (128,)),
    ('features.7.weight', (128, 128, 3, 3)), ('features.7.bias', (128,)),
    ('features.10.weight', (256, 128, 3, 3)), ('features.10.bias', (256,)),
    ('features.12.weight', (256, 256, 3, 3)), ('features.12.bias', (256,)),
    ('features.14.weight', (256, 256, 3, 3)), ('features.14.bias', (256,)),
    ('features.17.weight', (512, 256, 3, 3)), ('features.17.bias', (512,)),
    ('features.19.weight', (512, 512, 3, 3)), ('features.19.bias', (512,)),
    ('features.21.weight', (512, 512, 3, 3)), ('features.21.bias', (512,)),
    ('features.24.weight', (512, 512, 3, 3)), ('features.24.bias', (512,)),
    ('features.26.weight', (512, 512, 3, 3)), ('features.26.bias', (512,)),
    ('features.28.weight', (512, 512, 3, 3)), ('features.28.bias', (512,)),
    ('classifier.0.weight', (4096, 25088)), ('classifier.0.bias', (4096,)),
    ('classifier.3.weight', (4096, 4096)), ('classifier.3.bias', (4096,)),
]


def test_state_dict_keys_and_shapes_are_torchvisions():
    import phenaki_pytorch_amd as P
    with torch.device('meta'):
        net = P.VGG16Features()
    assert [(k, tuple(v.shape)) for k, v in net.state_dict().items()] == TORCHVISION_VGG16
    assert R.key_shapes() == TORCHVISION_VGG16
    assert not any(p.requires_grad for p in net.parameters()), 'the perceptual network is frozen: no weight gradient exists'
    assert isinstance(net, P.attention.PackedModule)


def test_full_torchvision_checkpoint_loads_without_its_last_layer():
    import phenaki_pytorch_amd as P
    net = P.VGG16Features(**R.NARROW)
    sd = R.random_state(**R.NARROW, seed=3, with_head=True)
    assert 'classifier.6.weight' in sd
    net._pk_cache = 'stale'
    res = net.load_state_dict(sd)
    assert not res.missing_keys and not res.unexpected_keys
    assert '_pk_cache' not in net.__dict__, 'load_state_dict must drop the packed device images'
    for k, v in net.state_dict().items():
        assert torch.equal(v, sd[k]), k
    assert not any(k.startswith('classifier.6') for k in net.state_dict())
    with pytest.raises(RuntimeError):
        net.load_state_dict({k: v for k, v in sd.items() if k != 'features.5.bias'})


@pytest.mark.parametrize('B,H,W,C,Co', [(1, 1, 1, 8, 8), (2, 5, 7, 8, 24), (3, 2, 2, 16, 8)])
def test_conv_matrix_in_im2col_order_is_conv2d(B, H, W, C, Co):
    from phenaki_pytorch_amd.discriminator import _conv_matrix
    g = torch.Generator().manual_seed(B * 100 + H)
    Cin = 3 if C == 8 else C                      # the first layer: 3 image channels padded to 8 pixel-row channels
    w = torch.randn(Co, Cin, 3, 3, generator=g, dtype=torch.float64)
    img = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64)
    rows = R.rows_of(F.pad(img, (0, 0, 0, 0, 0, C - Cin)))
    got = R.im2col(rows, B, H, W) @ _conv_matrix(w, C).T
    want = R.rows_of(F.conv2d(img, w, padding=1))
    assert (got - want).abs().max() <= 1e-12 * want.abs().max()


@pytest.mark.parametrize('B,H,W,C,Co', [(1, 1, 1, 8, 8), (2, 5, 7, 8, 24), (3, 2, 2, 16, 8)])
def test_backward_data_matrix_gives_the_autograd_input_gradient(B, H, W, C, Co):
    from phenaki_pytorch_amd.vgg import conv_matrix_bwd
    g = torch.Generator().manual_seed(B * 100 + W)
    Cin = 3 if C == 8 else C
    w = torch.randn(Co, Cin, 3, 3, generator=g, dtype=torch.float64)
    img = torch.randn(B, Cin, H, W, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(B, Co, H, W, generator=g, dtype=torch.float64)
    with torch.enable_grad():
        want, = torch.autograd.grad(F.conv2d(img, w, padding=1), img, dy)
    Wb = conv_matrix_bwd(w, C)
    assert tuple(Wb.shape) == (C, 9 * Co)
    got = R.im2col(R.rows_of(dy), B, H, W) @ Wb.T                 # (B H W, C): the padding channels come out zero
    assert (got[:, :Cin] - R.rows_of(want)).abs().max() <= 1e-12 * want.abs().max()
    assert (got[:, Cin:] == 0).all()


def test_classifier0_columns_follow_the_pixel_rows():
    from phenaki_pytorch_amd.vgg import classifier0_matrix
    g = torch.Generator().manual_seed(5)
    C, hidden, B = 16, 24, 2
    w = torch.randn(hidden, C * 49, generator=g, dtype=torch.float64)
    fmap = torch.randn(B, C, 7, 7, generator=g, dtype=torch.float64)
    want = F.linear(fmap.flatten(1), w)                                   # torchvision: flatten in (c, h, w) order
    rows = R.rows_of(fmap).reshape(B, 49 * C)                             # the kernels: pooled rows (b, i, j) x c
    got = rows @ classifier0_matrix(w, C).T
    assert (got - want).abs().max() <= 1e-12 * want.abs().max()


@pytest.mark.parametrize('H,W', [(1, 1), (2, 2), (4, 4), (7, 7), (8, 8), (9, 9), (8, 4)])
def test_adaptive_window_table_matches_torch(H, W):
    from phenaki_pytorch_amd.vgg import adaptive_windows
    g = torch.Generator().manual_seed(H * 10 + W)
    x = torch.randn(2, 3, H, W, generator=g, dtype=torch.float64)
    wy, wx = adaptive_windows(H), adaptive_windows(W)
    assert all(0 <= a < b <= H for a, b in wy) and all(0 <= a < b <= W for a, b in wx)
    got = torch.stack([torch.stack([x[:, :, y0:y1, x0:x1].mean(dim=(2, 3)) for x0, x1 in wx], dim=-1) for y0, y1 in wy], dim=-2)
    want = F.adaptive_avg_pool2d(x, (7, 7))
    assert (got - want).abs().max() <= 1e-12


def test_reference_restatement_is_the_module_tree():
    """tests/vgg_reference.forward against the nn.Module tree of VGG16Features run by torch itself on the CPU (float64, eval mode)"""
    import phenaki_pytorch_amd as P
    net = P.VGG16Features(**R.NARROW).double()
    sd = R.random_state(**R.NARROW, seed=4)
    net.load_state_dict({k: v.double() for k, v in sd.items()})
    net.eval()
    x = torch.randn(2, 3, 32, 48, generator=torch.Generator().manual_seed(1), dtype=torch.float64)
    want = net.classifier(net.avgpool(net.features(x)).flatten(1))
    got = R.forward(sd, x)
    assert got.abs().max() > 0 and (got - want).abs().max() <= 1e-12 * want.abs().max()
