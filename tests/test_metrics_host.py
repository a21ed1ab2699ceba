"""CPU-only checks of the validation metrics (phenaki_pytorch_amd/metrics.py): the float64 restatement against closed forms, the f32 yardstick
the GPU tolerances are derived from (kept measured here), the refusals that happen before any launch, and the TokenizerMetrics merge over two
gloo ranks.  No kernel is launched.

The tests of the first two sections (closed forms, the yardstick) exercise tests/metrics_restatement.py alone: they guard the REFERENCE the GPU tests
compare with and the case list their tolerances were derived on, and pass without the product.  The refusal, C-ABI and merge tests below them, and
all of tests/test_metrics_gpu.py, are the ones that need phenaki_pytorch_amd.metrics."""
import math
import os
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from tests import metrics_restatement as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement against closed forms ---------------------------------------------------------------------------------------------------------

def test_window_sums_to_one_and_is_the_outer_product():
    w = R.gaussian_window()
    assert w.shape == (11, 11) and w.dtype == torch.float64
    assert abs(float(w.sum()) - 1.) < 1e-15
    assert torch.equal(w, w.t()) and float(w[5, 5]) == float(w.max())
    assert abs(float(w[5, 5] / w[5, 4]) - math.exp(1 / (2 * 1.5 ** 2))) < 1e-12


def test_identical_inputs_give_exactly_one_and_100_db():
    a, _, _ = R.make_case('noise', 37, 45)
    assert torch.equal(R.ssim(a, a), torch.ones(2, 3, dtype=torch.float64))
    assert torch.equal(R.frame_mse(a, a), torch.zeros(2, 3, dtype=torch.float64))
    assert torch.equal(R.psnr(a, a).float(), torch.full((2, 3), 100.))
    assert torch.equal(R.psnr(255 * a, 255 * a, data_range=255.).float(), torch.full((2, 3), 100.))


@pytest.mark.parametrize('mu_a, mu_b, data_range', [(0.3, 0.7, 1.), (0.9, 0.9, 1.), (40., 200., 255.)])
def test_two_constant_frames(mu_a, mu_b, data_range):
    a, b = torch.full((1, 3, 2, 16, 12), mu_a), torch.full((1, 3, 2, 16, 12), mu_b)
    c1 = (0.01 * data_range) ** 2
    ma, mb = float(a[0, 0, 0, 0, 0]), float(b[0, 0, 0, 0, 0])                   # the f32-rounded levels
    want = (2 * ma * mb + c1) / (ma * ma + mb * mb + c1)
    for shift in (True, False):
        got = R.ssim(a, b, data_range=data_range, shift=shift)
        assert got.shape == (1, 2) and float((got - want).abs().max()) < 1e-12
    assert float((R.frame_mse(a, b) - (ma - mb) ** 2).abs().max()) <= 1e-12 * (ma - mb) ** 2
    assert R.ssim(a[:, :, 0], b[:, :, 0], data_range=data_range).shape == (1, 1)      # an image batch counts as one frame


def test_clamp_acts_on_the_first_operand_only():
    a, b = torch.full((1, 1, 1, 11, 11), 1.5), torch.full((1, 1, 1, 11, 11), 1.5)
    assert float(R.frame_mse(a, b, clamp=1.0)) == 0.25 and float(R.frame_mse(a, b)) == 0.


@pytest.mark.parametrize('k', [1, 7, 256])
def test_uniform_histogram_has_perplexity_k(k):
    ids = torch.arange(k).repeat(5)
    u = R.codebook_usage(ids, 256)
    assert u['used'] == k and abs(u['perplexity'] - k) < 1e-9 * k and abs(u['max_share'] - 1 / k) < 1e-15 and u['usage'] == k / 256
    assert int(u['counts'].sum()) == 5 * k
    keep = torch.zeros(5 * k, dtype=torch.bool)
    empty = R.codebook_usage(ids, 256, keep)
    assert (empty['used'], empty['entropy'], empty['perplexity'], empty['max_share']) == (0, 0., 1., 0.)


# ---- the yardstick: what f32 arithmetic costs these formulas --------------------------------------------------------------------------------------
# The GPU tests allow the kernels 5e-6 on SSIM (10 x the f32 yardstick's own worst error) and 2e-6 relative on MSE; this is where those yardstick
# figures stay measured.  Last measured: see the assertion messages (run with -s to print them).

def test_f32_yardstick_and_the_shift():
    worst_ssim, worst_mse, flat_raw = 0., 0., 0.
    for H, W in R.SHAPES:
        for content in R.CONTENTS:
            a, b, kw = R.make_case(content, H, W)
            ref = R.ssim(a, b, **kw)
            err = float((R.ssim(a, b, dtype=torch.float32, **kw).double() - ref).abs().max())
            worst_ssim = max(worst_ssim, err)
            mkw = {k: v for k, v in kw.items() if k == 'clamp'}
            mref = R.frame_mse(a, b, **mkw)
            merr = float(((R.frame_mse(a, b, dtype=torch.float32, **mkw).double() - mref).abs() / mref.clamp(min=1e-300)).max())
            worst_mse = max(worst_mse, merr)
            if content == 'flat':
                raw = float((R.ssim(a, b, dtype=torch.float32, shift=False, **kw).double() - ref).abs().max())
                flat_raw = max(flat_raw, raw)
                if (H, W) == (11, 11):
                    flat_raw_11 = raw
    print(f'f32 yardstick: ssim {worst_ssim:.2e}  mse rel {worst_mse:.2e}  raw moments on the flat case {flat_raw_11:.2e} (11 x 11), {flat_raw:.2e} (worst)')
    assert worst_ssim <= 1e-6, f'f32 SSIM with the shift errs by {worst_ssim:.2e}'
    assert worst_mse <= 2e-7, f'f32 MSE errs by {worst_mse:.2e} relative'
    assert flat_raw_11 > 5e-5, f'E[a^2] - E[a]^2 on raw f32 pixels errs by only {flat_raw_11:.2e} on the flat case: the case does not discriminate'


# ---- refusals before any launch -------------------------------------------------------------------------------------------------------------------

@pytest.fixture
def no_launch(monkeypatch):
    """any attempt to reach the library fails the test"""
    from phenaki_pytorch_amd import _lib

    def boom(*a, **k):
        raise AssertionError('the library was reached')
    monkeypatch.setattr(_lib, 'load', boom)


def test_refusals(no_launch):
    import phenaki_pytorch_amd as P
    ok = torch.zeros(2, 3, 3, 16, 12)
    for fn in (P.frame_mse, P.psnr, P.ssim):
        with pytest.raises(ValueError, match='shapes differ'):
            fn(ok, torch.zeros(2, 3, 3, 16, 13))
        with pytest.raises(ValueError, match='float32'):
            fn(ok.double(), ok.double())
        with pytest.raises(ValueError, match='float32'):
            fn(ok, ok.to(torch.bfloat16))
        with pytest.raises(ValueError, match='videos or'):
            fn(ok[0, 0], ok[0, 0])
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            fn(ok, ok)
    for shape in ((2, 3, 3, 10, 64), (2, 3, 3, 64, 10), (2, 3, 10, 10)):
        with pytest.raises(ValueError, match='smaller than the 11 x 11 window'):
            P.ssim(torch.zeros(shape), torch.zeros(shape))
        with pytest.raises(RuntimeError, match='no CPU fallback'):            # no window: any size >= 1 is accepted
            P.frame_mse(torch.zeros(shape), torch.zeros(shape))
    with pytest.raises(ValueError, match='data_range'):
        P.ssim(ok, ok, data_range=0.)
    with pytest.raises(ValueError, match='clamp'):
        P.psnr(ok, ok, clamp=-1.)
    ids = torch.zeros(8, dtype=torch.int64)
    with pytest.raises(ValueError, match='codebook_size'):
        P.codebook_usage(ids, 0)
    with pytest.raises(ValueError, match='int64'):
        P.codebook_usage(ids.float(), 16)
    with pytest.raises(ValueError, match='keep has'):
        P.codebook_usage(ids, 16, keep=torch.ones(7, dtype=torch.bool))
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        P.codebook_usage(ids, 16)


def test_evaluate_refuses_cpu_and_bad_masks(no_launch):
    import phenaki_pytorch_amd as P
    from oracle.configs import TINY
    cv = P.CViViT(use_vgg_and_gan=False, **TINY['cvivit']).train()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        cv.evaluate(torch.zeros(1, 3, 5, 64, 64))
    with pytest.raises(AssertionError):
        cv.evaluate(torch.zeros(1, 3, 4, 64, 64))                             # (frames - 1) % temporal_patch_size
    assert cv.training
    with pytest.raises(RuntimeError, match='before any update'):
        P.TokenizerMetrics(cv).compute()


def test_c_abi_refuses_bad_arguments_before_any_launch():
    """null pointers, non-positive sizes and frames below the window return PK_EINVAL; nothing is launched (there is no device here)"""
    from phenaki_pytorch_amd import build, _lib
    build.build(verbose=False)
    lib = _lib.load()
    assert lib.pk_frame_sqerr_parts(256, 256) == 16 and lib.pk_frame_sqerr_parts(1, 1) == 1 and lib.pk_frame_sqerr_parts(0, 4) == -1
    assert lib.pk_frame_ssim_parts(256, 256) == 64 and lib.pk_frame_ssim_parts(11, 11) == 1 and lib.pk_frame_ssim_parts(42, 42) == 1 and lib.pk_frame_ssim_parts(42, 43) == 2
    assert lib.pk_frame_ssim_parts(43, 43) == 4 and lib.pk_frame_ssim_parts(75, 140) == 3 * 5
    assert lib.pk_frame_ssim_parts(10, 64) == -1 and lib.pk_frame_ssim_parts(64, 10) == -1
    p = 4096                                                                   # a non-null, aligned stand-in: every call below must return before using it
    assert lib.pk_frame_sqerr(None, p, 1, 1, 1, 4, 4, 0., 1., p, 1, p, None, None) == -1
    assert lib.pk_frame_sqerr(p, p, 1, 1, 1, 4, 4, 0., 1., None, 1, p, None, None) == -1
    assert lib.pk_frame_sqerr(p, p, 1, 1, 1, 4, 4, 0., 1., p, 1, None, None, None) == -1
    assert lib.pk_frame_sqerr(p, p, 0, 1, 1, 4, 4, 0., 1., p, 0, p, None, None) == -1
    assert lib.pk_frame_sqerr(p, p, 1, 1, 1, 4, 0, 0., 1., p, 1, p, None, None) == -1
    assert lib.pk_frame_sqerr(p, p, 1, 1, 1, 4, 4, 0., 1., p, 2, p, None, None) == -1          # workspace of the wrong size
    assert lib.pk_frame_sqerr(p, p, 1, 1, 1, 4, 4, 0., 0., p, 1, p, p, None) == -1             # psnr wanted without a data range
    assert lib.pk_frame_ssim(None, p, 1, 1, 1, 16, 16, 0., 1., p, 1, p, None) == -1
    assert lib.pk_frame_ssim(p, p, 1, 1, 1, 16, 16, 0., 1., None, 1, p, None) == -1
    assert lib.pk_frame_ssim(p, p, 1, 1, 1, 16, 16, 0., 1., p, 1, None, None) == -1
    assert lib.pk_frame_ssim(p, p, 1, 1, 1, 10, 16, 0., 1., p, 1, p, None) == -1
    assert lib.pk_frame_ssim(p, p, 1, 1, 1, 16, 10, 0., 1., p, 1, p, None) == -1
    assert lib.pk_frame_ssim(p, p, 1, 0, 1, 16, 16, 0., 1., p, 0, p, None) == -1
    assert lib.pk_frame_ssim(p, p, 1, 1, 1, 16, 16, 0., 0., p, 1, p, None) == -1
    assert lib.pk_frame_ssim(p, p, 1, 1, 1, 16, 16, 0., 1., p, 3, p, None) == -1
    assert lib.pk_code_usage(None, 4, p, None) == -1 and lib.pk_code_usage(p, 4, None, None) == -1 and lib.pk_code_usage(p, 0, p, None) == -1


# ---- the accumulator's merge over ranks -----------------------------------------------------------------------------------------------------------

def _state(rank):
    g = torch.Generator().manual_seed(50 + rank)
    return dict(mse=torch.rand((), generator=g, dtype=torch.float64), psnr=30 * torch.rand((), generator=g, dtype=torch.float64),
                ssim=torch.rand((), generator=g, dtype=torch.float64), frames=torch.tensor(6 + 4 * rank),
                counts=torch.randint(0, 9, (256,), generator=g))


def _compute_sends(state, merge):
    """the number of collectives one TokenizerMetrics.compute(merge=...) on this state issues, counted on stand-ins (no kernel, nothing sent): both
    ranks call it, so the count is taken without leaving a rank waiting"""
    from unittest import mock
    from phenaki_pytorch_amd import _lib, metrics
    tm = metrics.TokenizerMetrics(None)
    tm.state = {k: v.clone() for k, v in state.items()}
    sent = []
    usage = lambda counts: torch.tensor([float(counts.sum()), float((counts > 0).sum()), 0., 1., 0.], dtype=torch.float64)
    with mock.patch.object(_lib, 'code_usage', usage), mock.patch.object(dist, 'all_reduce', lambda t, **kw: sent.append(tuple(t.shape))):
        out = tm.compute(merge=merge)
    assert out['frames'] == int(state['frames']) and out['tokens'] == int(state['counts'].sum()) and all(torch.equal(tm.state[k], state[k]) for k in state)
    return len(sent)


def _merge_worker(rank, ws, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=ws)
    sys.path.insert(0, ROOT)
    from phenaki_pytorch_amd.metrics import merge_states
    mine = _state(rank)
    merged = merge_states({k: v.clone() for k, v in mine.items()})
    want = {k: sum(_state(r)[k] for r in range(ws)) for k in mine}
    ok = set(merged) == set(want) and all(torch.equal(merged[k], want[k]) and merged[k].dtype == mine[k].dtype for k in want)
    ok = ok and _compute_sends(mine, merge=True) == 5 and _compute_sends(mine, merge=False) == 0
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


def test_merge_states_world_size_2_gloo():
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000) + 17
    procs = [ctx.Process(target=_merge_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(res) == [(0, True), (1, True)]


def test_example_validates_on_rank_0_without_a_collective():
    """examples/train_cvivit.py validates on rank 0 alone while the other ranks train on: its compute() must be the rank-local form"""
    src = open(os.path.join(ROOT, 'examples', 'train_cvivit.py')).read()
    assert 'tm.compute(merge=False)' in src and 'tm.compute()' not in src


def test_merge_states_without_a_process_group_is_the_identity():
    from phenaki_pytorch_amd.metrics import merge_states
    s = _state(0)
    out = merge_states(s)
    assert out is s and all(torch.equal(out[k], _state(0)[k]) for k in s)
