"""CPU float64 restatement of the perceptual network (torchvision's VGG16 with classifier[:-2], reference cvivit.py:349-352) from plain torch ops
-- F.conv2d, F.max_pool2d, F.adaptive_avg_pool2d, F.linear -- on a torchvision-keyed state dict.  Shared by tests/test_vgg_host.py and
tests/test_vgg_gpu.py; torchvision itself is not needed."""
import torch
import torch.nn.functional as F

CONV_IDX = (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28)
POOL_AFTER = (2, 7, 14, 21, 28)            # a 2x2 max-pool follows the ReLU of these convolutions
NARROW = dict(widths=(8, 16, 32, 64, 64), hidden=128)


def key_shapes(widths=(64, 128, 256, 512, 512), hidden=4096, with_head=False):
    """[(key, shape)] of torchvision's vgg16 state dict, classifier[:-2] (with_head: plus the 1000-way classifier.6 of a full checkpoint)"""
    per_conv = [widths[0]] * 2 + [widths[1]] * 2 + [widths[2]] * 3 + [widths[3]] * 3 + [widths[4]] * 3
    out, cin = [], 3
    for idx, co in zip(CONV_IDX, per_conv):
        out += [(f'features.{idx}.weight', (co, cin, 3, 3)), (f'features.{idx}.bias', (co,))]
        cin = co
    out += [('classifier.0.weight', (hidden, cin * 49)), ('classifier.0.bias', (hidden,)),
            ('classifier.3.weight', (hidden, hidden)), ('classifier.3.bias', (hidden,))]
    if with_head:
        out += [('classifier.6.weight', (1000, hidden)), ('classifier.6.bias', (1000,))]
    return out


def random_state(widths=(64, 128, 256, 512, 512), hidden=4096, seed=0, with_head=False):
    """seeded f32 weights at He scale (activations neither vanish nor explode over 15 layers), biases that push some units below zero"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in key_shapes(widths, hidden, with_head):
        if k.endswith('weight'):
            fan_in = 1
            for s in shape[1:]:
                fan_in *= s
            sd[k] = torch.randn(shape, generator=g) * (2.0 / fan_in) ** 0.5
        else:
            sd[k] = torch.randn(shape, generator=g) * 0.1
    return sd


def bf16_round(t):
    return t.float().to(torch.bfloat16).to(t.dtype)


def forward(sd, img, round_bf16=False, keep=None):
    """(B, 3, H, W) -> (B, hidden) in the dtype of img (float64 in the tests).  round_bf16: the inputs of every convolution and Linear and the weights are
    rounded to bf16 (where the bf16 product rounds its operands); keep (B, hidden): the dropout mask times its scale, applied after classifier.1"""
    r = bf16_round if round_bf16 else (lambda t: t)
    x = img
    for idx in CONV_IDX:
        w, b = sd[f'features.{idx}.weight'].to(img.dtype), sd[f'features.{idx}.bias'].to(img.dtype)
        x = F.relu(F.conv2d(r(x), r(w), b, padding=1))
        if idx in POOL_AFTER:
            x = F.max_pool2d(x, 2, 2)
    x = F.adaptive_avg_pool2d(x, (7, 7)).flatten(1)
    x = F.relu(F.linear(r(x), r(sd['classifier.0.weight'].to(img.dtype)), sd['classifier.0.bias'].to(img.dtype)))
    if keep is not None:
        x = x * keep.to(img.dtype)
    return F.relu(F.linear(r(x), r(sd['classifier.3.weight'].to(img.dtype)), sd['classifier.3.bias'].to(img.dtype)))


def rows_of(img):
    """(B, C, H, W) -> channels-last pixel rows (B H W, C)"""
    B, C, H, W = img.shape
    return img.permute(0, 2, 3, 1).reshape(B * H * W, C).contiguous()


def image_of(rows, B, H, W):
    return rows.reshape(B, H, W, -1).permute(0, 3, 1, 2).contiguous()


def im2col(rows, B, H, W):
    """the patch matrix of pk_im2col for 3x3 / stride 1 / pad 1: cols[(b, y, x)][(ky * 3 + kx) * C + c] = x[b][y + ky - 1][x + kx - 1][c], zero outside"""
    C = rows.shape[1]
    x = F.pad(rows.reshape(B, H, W, C), (0, 0, 1, 1, 1, 1))
    taps = [x[:, ky:ky + H, kx:kx + W, :] for ky in range(3) for kx in range(3)]
    return torch.cat(taps, dim=-1).reshape(B * H * W, 9 * C)
