"""The validation metrics on the GPU (csrc/metrics.hip through phenaki_pytorch_amd/metrics.py) against the float64 restatement
(tests/metrics_restatement.py) fed the same f32-rounded inputs, CViViT.evaluate against the module's existing evaluation surface, and the
TokenizerMetrics accumulator.

Tolerances: per-frame SSIM 5e-6 absolute -- 10 x the worst error of the f32 run of the restatement itself (tests/test_metrics_host.py keeps that
measured), because the kernel sums in another order than torch; MSE 2e-6 relative, PSNR 2e-5 dB; identical frames exactly 1 and 100; counts exact,
entropy 1e-5 absolute, perplexity 1e-5 relative (the f32 formula errs by 5e-7)."""
import pytest
import torch

from oracle import weights
from oracle.configs import TINY
from tests import metrics_restatement as R
from tests.util import load_product

pytestmark = pytest.mark.gpu

SSIM_ATOL, MSE_RTOL, PSNR_ATOL = 5e-6, 2e-6, 2e-5


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    torch.cuda.set_device(0)
    with torch.no_grad():
        yield


def check_case(a, b, kw, what):
    """the three metrics of one pair of CPU videos on the device against the f64 restatement; two calls of each must be bit-identical"""
    import phenaki_pytorch_amd as P
    ad, bd = a.cuda(), b.cuda()
    ckw = {k: v for k, v in kw.items() if k == 'clamp'}
    frames = (a.shape[0], 1 if a.ndim == 4 else a.shape[2])
    got = dict(mse=P.frame_mse(ad, bd, **ckw), psnr=P.psnr(ad, bd, **kw), ssim=P.ssim(ad, bd, **kw))
    again = dict(mse=P.frame_mse(ad, bd, **ckw), psnr=P.psnr(ad, bd, **kw), ssim=P.ssim(ad, bd, **kw))
    ref = dict(mse=R.frame_mse(a, b, **ckw), psnr=R.psnr(a, b, **kw), ssim=R.ssim(a, b, **kw))
    for k in got:
        assert got[k].shape == frames and got[k].dtype == torch.float32 and got[k].is_cuda, f'{what} {k}: {tuple(got[k].shape)} {got[k].dtype}'
        assert torch.equal(got[k], again[k]), f'{what} {k}: two calls differ'
        assert torch.isfinite(got[k]).all(), f'{what} {k}: non-finite'
    mse_err = float(((got['mse'].cpu().double() - ref['mse']).abs() / ref['mse'].clamp(min=1e-300)).max())
    psnr_err = float((got['psnr'].cpu().double() - ref['psnr']).abs().max())
    ssim_err = float((got['ssim'].cpu().double() - ref['ssim']).abs().max())
    print(f'{what}: ssim err {ssim_err:.2e}  mse rel err {mse_err:.2e}  psnr err {psnr_err:.2e} dB')
    assert ssim_err <= SSIM_ATOL, f'{what}: SSIM off by {ssim_err:.3e}'
    assert mse_err <= MSE_RTOL, f'{what}: MSE off by {mse_err:.3e} relative'
    assert psnr_err <= PSNR_ATOL, f'{what}: PSNR off by {psnr_err:.3e} dB'
    return got


@pytest.mark.parametrize('content', R.CONTENTS)
@pytest.mark.parametrize('H, W', R.SHAPES)
def test_metrics_match_the_restatement(H, W, content):
    a, b, kw = R.make_case(content, H, W)                       # B, C, F = 2, 3, 3
    got = check_case(a, b, kw, f'{content} {H}x{W}')
    if content == 'same':
        assert torch.equal(got['ssim'], torch.ones_like(got['ssim'])), 'identical frames: SSIM must be exactly 1'
        assert torch.equal(got['psnr'], torch.full_like(got['psnr'], 100.)), 'identical frames: PSNR must be exactly 100'
        assert torch.equal(got['mse'], torch.zeros_like(got['mse']))


@pytest.mark.parametrize('content', ['noise', 'flat', 'same'])
def test_single_channel_and_image_batches(content):
    a, b, kw = R.make_case(content, 37, 45, B=2, C=1, Fr=3, seed=1)
    check_case(a, b, kw, f'{content} C=1')
    a, b, kw = R.make_case(content, 37, 45, B=3, C=3, Fr=None, seed=2)             # (B, C, H, W): one frame each
    got = check_case(a, b, kw, f'{content} 4-D')
    assert got['ssim'].shape == (3, 1)


def test_unaligned_views_and_strided_inputs_give_the_same_bits():
    """rows that do not start on 16 bytes take the 4-byte path: a copy of the same pixels at a 4-byte offset gives the same results bit for bit,
    and a strided view is made contiguous first"""
    import phenaki_pytorch_amd as P
    a, b, _ = R.make_case('noise', 64, 64)
    ad, bd = a.cuda(), b.cuda()
    n = ad.numel()
    buf_a, buf_b = torch.zeros(n + 1, device='cuda'), torch.zeros(n + 1, device='cuda')
    buf_a[1:].copy_(ad.reshape(-1))
    buf_b[1:].copy_(bd.reshape(-1))
    au, bu = buf_a[1:].view(ad.shape), buf_b[1:].view(bd.shape)
    assert au.data_ptr() % 16 == 4 and au.is_contiguous()
    for fn in (P.frame_mse, P.psnr, P.ssim):
        assert torch.equal(fn(au, bu), fn(ad, bd)), fn.__name__
        assert torch.equal(fn(ad.transpose(3, 4), bd.transpose(3, 4)), fn(ad.transpose(3, 4).contiguous(), bd.transpose(3, 4).contiguous())), fn.__name__


# ---- codebook usage ---------------------------------------------------------------------------------------------------------------------------

def check_usage(ids, V, keep, what):
    import phenaki_pytorch_amd as P
    got = P.codebook_usage(ids.cuda(), V, keep=None if keep is None else keep.cuda())
    again = P.codebook_usage(ids.cuda(), V, keep=None if keep is None else keep.cuda())
    ref = R.codebook_usage(ids, V, keep)
    assert set(got) == {'counts', 'used', 'usage', 'entropy', 'perplexity', 'max_share'}
    assert all(v.is_cuda for v in got.values()) and got['counts'].dtype == torch.int64 and got['counts'].shape == (V,)
    for k in got:
        assert torch.equal(got[k], again[k]), f'{what} {k}: two calls differ'
    assert torch.equal(got['counts'].cpu(), ref['counts']), f'{what}: counts'
    assert int(got['used']) == ref['used'] and abs(float(got['usage']) - ref['usage']) <= 1e-7
    ent_err, ppl_err = abs(float(got['entropy']) - ref['entropy']), abs(float(got['perplexity']) - ref['perplexity']) / ref['perplexity']
    print(f'{what}: entropy err {ent_err:.2e}  perplexity rel err {ppl_err:.2e}')
    assert ent_err <= 1e-5 and ppl_err <= 1e-5, f'{what}: entropy off by {ent_err:.3e}, perplexity by {ppl_err:.3e} relative'
    assert abs(float(got['max_share']) - ref['max_share']) <= 1e-6
    return got


@pytest.mark.parametrize('V, M', [(256, 5000), (65536, 5000), (65536, 1)])
def test_codebook_usage(V, M):
    g = torch.Generator().manual_seed(V + M)
    skewed = (torch.rand(M, generator=g) ** 3 * V).long().clamp(max=V - 1)              # a long-tailed histogram
    check_usage(skewed, V, None, f'skewed V={V} M={M}')
    check_usage(skewed.view(1, M), V, None, f'2-D ids V={V} M={M}')
    one = check_usage(torch.full((M,), V - 1), V, None, f'one code V={V} M={M}')
    assert int(one['used']) == 1 and float(one['entropy']) == 0. and float(one['perplexity']) == 1. and float(one['max_share']) == 1.
    half = torch.arange(M) % 2 == 0
    check_usage(skewed, V, half, f'half kept V={V} M={M}')
    none = check_usage(skewed, V, torch.zeros(M, dtype=torch.bool), f'nothing kept V={V} M={M}')
    assert (int(none['used']), float(none['entropy']), float(none['perplexity']), float(none['max_share'])) == (0, 0., 1., 0.)
    assert int(none['counts'].sum()) == 0


# ---- CViViT.evaluate ------------------------------------------------------------------------------------------------------------------------------

def lfq_tokenizer():
    cv, *_ = load_product('tiny', TINY, device='cuda:0')
    return cv


def vq_tokenizer():
    import phenaki_pytorch_amd as P
    torch.manual_seed(3)
    cv = P.CViViT(lookup_free_quantization=False, use_vgg_and_gan=False, **{**TINY['cvivit'], 'codebook_size': 4096}).cuda().train()
    cv.vq._codebook.cluster_size.uniform_(0., 3.)                                        # buffers a stray update would visibly move
    P.set_compute_dtype(cv, 'fp32')
    return cv


@pytest.mark.parametrize('make', [lfq_tokenizer, vq_tokenizer], ids=['lfq', 'vq'])
def test_evaluate_agrees_with_the_existing_evaluation_surface(make):
    import phenaki_pytorch_amd as P
    cv = make()
    training = cv.training
    video = weights.synthetic_video(2, 5, 64, 64, seed=0).cuda()
    ragged = torch.tensor([[True, True, True, False, False], [True] * 5], device='cuda')
    ids_ref = cv(video, return_only_codebook_ids=True)
    recon = cv(video, return_recons_only=True)
    V = cv.vq.codebook_size
    def untouched(call):
        """runs `call` between two snapshots of the quantizer's state and of the training flag: nothing but evaluate() lies between them"""
        before = {k: v.clone() for k, v in cv.vq.state_dict().items()}
        out = call()
        after = cv.vq.state_dict()
        assert set(after) == set(before) and all(torch.equal(after[k], before[k]) for k in before), 'evaluate() moved a quantizer buffer'
        assert cv.training == training, 'evaluate() changed the training flag'
        return out

    for mask in (None, ragged):
        r = untouched(lambda: cv.evaluate(video, mask=mask, clamp=False))
        assert torch.equal(r['ids'], ids_ref)
        loss = cv(video, mask=mask)
        rel = abs(float(r['mse_mean']) - float(loss)) / float(loss)
        print(f'mask {mask is not None}: mse_mean {float(r["mse_mean"]):.8f} forward {float(loss):.8f} rel {rel:.2e}')
        assert rel <= 1e-6, f'frame-mean mse {float(r["mse_mean"])} vs forward {float(loss)}'
        assert torch.equal(r['mse'], P.frame_mse(recon, video)) and torch.equal(r['psnr'], P.psnr(recon, video)) and torch.equal(r['ssim'], P.ssim(recon, video))
        keep = torch.ones(2, 5, dtype=torch.bool, device='cuda') if mask is None else mask
        assert int(r['frames']) == int(keep.sum())
        for k in ('mse', 'psnr', 'ssim'):
            want = float(r[k].double()[keep].mean())
            assert abs(float(r[k + '_mean']) - want) <= 1e-6 * abs(want)
        tok = None if mask is None else cv.calculate_video_token_mask(video, mask)
        u = R.codebook_usage(ids_ref.cpu(), V, None if tok is None else tok.cpu())
        assert torch.equal(r['codebook_usage']['counts'].cpu(), u['counts']) and int(r['codebook_usage']['used']) == u['used']
        assert abs(float(r['codebook_usage']['perplexity']) - u['perplexity']) <= 1e-5 * u['perplexity']
    clamped = untouched(lambda: cv.evaluate(video))                                       # clamp=True: the reconstruction read clamped to [0, 1]
    assert torch.equal(clamped['ssim'], P.ssim(recon.clamp(0., 1.), video)) and torch.equal(clamped['mse'], P.frame_mse(recon.clamp(0., 1.), video))
    image = untouched(lambda: cv.evaluate(video[:, :, 0], clamp=False))
    assert image['ssim'].shape == (2, 1) and torch.equal(image['ids'], cv(video[:, :, 0], return_only_codebook_ids=True))


def test_evaluate_ignores_grad_mode_and_the_compute_dtype_of_the_metrics():
    """called with grad mode on it still returns graph-free values, and the metric kernels are f32 whatever the model's compute dtype: the
    numbers of a bf16x3 model equal the f32 metrics of ITS reconstruction"""
    import phenaki_pytorch_amd as P
    cv = lfq_tokenizer()
    P.set_compute_dtype(cv, 'bf16x3')
    video = weights.synthetic_video(1, 5, 64, 64, seed=1).cuda()
    with torch.enable_grad():
        r = cv.evaluate(video, clamp=False)
    assert not any(v.requires_grad for v in r.values() if isinstance(v, torch.Tensor))
    recon = cv(video, return_recons_only=True)
    assert torch.equal(r['ssim'], P.ssim(recon, video)) and torch.equal(r['psnr'], P.psnr(recon, video))


# ---- the accumulator ------------------------------------------------------------------------------------------------------------------------------

def test_tokenizer_metrics_accumulates_like_one_call():
    import phenaki_pytorch_amd as P
    cv = vq_tokenizer()
    video = weights.synthetic_video(4, 5, 64, 64, seed=5).cuda()
    mask = torch.tensor([[True] * 5, [True, True, True, False, False], [True] * 5, [True, False, False, False, False]], device='cuda')
    whole = P.TokenizerMetrics(cv).update(video, mask)
    halves = P.TokenizerMetrics(cv).update(video[:2], mask[:2]).update(video[2:], mask[2:])
    assert torch.equal(whole.state['counts'], halves.state['counts']) and int(whole.state['frames']) == int(halves.state['frames']) == 14
    a, b = whole.compute(), halves.compute()
    assert whole.compute(merge=False) == a                                                # no process group: the rank-local form is the same
    assert set(a) == {'mse', 'psnr', 'ssim', 'frames', 'tokens', 'codes_used', 'codebook_size', 'usage', 'entropy', 'perplexity', 'max_share'}
    assert all(isinstance(v, (int, float)) for v in a.values())
    for k in ('mse', 'psnr', 'ssim'):
        print(f'{k}: whole {a[k]!r} halves {b[k]!r}')
        assert abs(a[k] - b[k]) <= 1e-12 * abs(a[k]), f'{k}: {a[k]} vs {b[k]}'
    for k in ('frames', 'tokens', 'codes_used', 'codebook_size', 'usage', 'entropy', 'perplexity', 'max_share'):
        assert a[k] == b[k], k
    r = cv.evaluate(video, mask=mask)
    assert a['frames'] == 14 and a['tokens'] == int(cv.calculate_video_token_mask(video, mask).sum()) and a['codebook_size'] == 4096
    assert abs(a['ssim'] - float(r['ssim_mean'])) <= 1e-6 and abs(a['perplexity'] - float(r['codebook_usage']['perplexity'])) <= 1e-5 * a['perplexity']
    whole.reset()
    assert whole.state is None
    with pytest.raises(RuntimeError, match='before any update'):
        whole.compute()
