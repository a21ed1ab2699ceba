"""End-to-end parity AT THE BATCH SIZES bench.py TIMES.

The full-size module tests run at B = 1 / 2 / 4, where `auto_variant` (csrc/gemm.hip) picks the 64 x 64 tiles everywhere and
`pk_vocab_sample` stays on the tiled kernel.  The bench runs B = 8 (M = 4 608 / 9 216-row GEMMs: 128 x 64 four-wave tiles, other split-K
counts, `vocab_resident_kernel` from 2 048 masked rows on) and B = 32 (M = 18 432 / 36 864 rows: L2 panels).  These tests put exactly those
configurations inside a comparison with the CPU oracle (reference lines: cvivit.py:518-574, phenaki_pytorch.py:418-560):
  (a) BASELINE configs[1] encode at B = 8, every compute mode;
  (b) BASELINE configs[2] sample at B = 8: 2 free-running steps WITH the row compaction the bench uses + 2 teacher-forced steps at
      50 % / 20 % masked (one above, one below the resident kernel's row threshold);
  (c) one teacher-forced MaskGit step at B = 32.
Tolerances are the ones of tests/test_modules_gpu.py (north star: ids bit-exact under the margin audit, values 1e-3 in the f32-grade modes)."""
import pytest
import torch

from oracle import phenaki_oracle as O
from oracle import weights
from oracle.configs import FULL, oracle_cfgs, state_dicts
from tests.util import argmax_equal_with_margin, close, gumbel_noisy, ids_equal_with_margin, load_product, record_parity

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

# the tolerances of tests/test_modules_gpu.py (documented there)
BF16_E2E, BF16_GAP_SLACK = 2e-2, 1.1
MODES = [('fp32', 1e-3, 1e-4), ('bf16x3', 1e-3, 1e-4), ('bf16', BF16_E2E, BF16_E2E)]
F32_GRADE = ['fp32', 'bf16x3']


@pytest.fixture(scope='module', autouse=True)
def _oracle_follows_product_ln_fold():
    """the bf16 oracle rounds where the product rounds (same switchboard as tests/test_modules_gpu.py)"""
    from phenaki_pytorch_amd import attention
    from phenaki_pytorch_amd import cvivit as _cv
    O.LN_FOLD, O.LN_FOLD_FF, O.LN_FOLD_FF_MAX_ROWS = attention._LN_FOLD, bool(attention._LN_FOLD_FF), attention._LN_FOLD_FF_MAX_ROWS
    O.ATTN_FIXED_OFFSET = attention._ATTN_FIXED
    O.ATTN_FIXED_OFFSET_BIAS = attention._ATTN_FIXED and attention._BIAS_TABLE
    O.PATCH_FUSED = _cv._PATCH_FUSED


def closer_than_precision_gap(gpu, ref_same, ref_f32, what):
    rms = lambda a, b: ((a.detach().float().cpu() - b.detach().float().cpu()).pow(2).mean().sqrt() / b.detach().float().cpu().pow(2).mean().sqrt()).item()
    e, gap = rms(gpu, ref_same), rms(ref_same, ref_f32)
    assert e <= BF16_GAP_SLACK * gap, f'{what}: rms distance to the bf16 oracle {e:.3e} exceeds the bf16-vs-f32 gap {gap:.3e}'
    return e, gap

MASK_ID = FULL['maskgit']['num_tokens']
V = MASK_ID


@pytest.mark.parametrize('dtype,tol,mtol', MODES)
def test_encode_at_bench_batch_matches_oracle(dtype, tol, mtol):
    """configs[1] as benched: (8, 3, 17, 256, 256) -> ids (8, 9, 8, 8); 4 608-row projections, the split-K patch embedding at 204 workgroups"""
    cv_sd, _, _ = state_dicts('full')
    cvc, _, _ = oracle_cfgs(FULL)
    cv, _, _, _ = load_product('full', FULL, dtype=dtype)
    video = weights.synthetic_video(8, 17, 256, 256, seed=3)
    with O.precision(dtype):
        ids_ref, proj_ref = O.cvivit_tokenize(cv_sd, cvc, video, return_proj=True)
    ids, proj = cv.tokenize(video.cuda(), return_proj=True)
    assert ids.shape == (8, 9, 8, 8) and ids.dtype == torch.int64
    assert torch.equal(cv(video.cuda(), return_only_codebook_ids=True), ids), 'forward(return_only_codebook_ids) != tokenize'
    e_proj = close(proj, proj_ref, tol, f'lfq projection {dtype} B=8')
    flips = ids_equal_with_margin(ids, ids_ref, proj_ref, tol=mtol)
    assert flips <= (8 if dtype in F32_GRADE else ids.numel() * 16 // 100), f'{dtype}: {flips} audited sign flips of {ids.numel() * 16} bits'
    extra = {}
    if dtype == 'bf16':
        proj_f32 = O.cvivit_tokenize(cv_sd, cvc, video, return_proj=True)[1]
        extra['proj_rms_vs_gap'] = closer_than_precision_gap(proj, proj_ref, proj_f32, 'lfq projection B=8')
    # decode at the same batch (the bench's decode leg): pixels of the oracle's ids
    with O.precision(dtype):
        rec_ref = O.cvivit_decode_ids(cv_sd, cvc, ids_ref.flatten(1)[:2])
    rec = cv.decode_from_codebook_indices(ids_ref.flatten(1).cuda())
    assert rec.shape == (8, 3, 17, 256, 256)
    e_rec = close(rec[:2], rec_ref, tol, f'decoded pixels {dtype} B=8 (first two videos)')
    record_parity('encode_b8_vs_oracle', dict(dtype=dtype, batch=8, proj_rel_err=e_proj, pixel_rel_err=e_rec, audited_bit_flips=flips,
                                              ids_equal=bool(torch.equal(ids.cpu(), ids_ref)), **extra))


def _ctx(B):
    return weights.synthetic_context(B, 12, 768, seed=2)


@pytest.mark.parametrize('dtype,tol,mtol', MODES)
def test_sample_at_bench_batch_free_running_matches_oracle(dtype, tol, mtol):
    """configs[2] as benched: B = 8, CFG 5, TokenCritic, the vocabulary head on the COMPACT masked-row list (`_compact=True`, what an
    un-traced call does): 4 608 rows at step 0 and 3 258 at step 1 -> `vocab_resident_kernel` in bf16; trunk GEMMs at M = 9 216."""
    B = 8
    cv_sd, mg_sd, cr_sd = state_dicts('full')
    cvc, mgc, crc = oracle_cfgs(FULL)
    _, _, _, ph = load_product('full', FULL, steps=2, dtype=dtype)
    ctx = _ctx(B)
    ph.encode_texts = lambda texts, output_device=None: ctx.cuda()

    noise = {}

    def nf_cpu(kind, step, shape):
        if (kind, step) not in noise:
            noise[(kind, step)] = weights.uniform_noise(tuple(shape), 1300 + 2 * step + (1 if kind == 'critic' else 0))
        return noise[(kind, step)]

    trace_ref, trace = [], []
    with O.precision(dtype):
        vid_ref, ids_ref = O.sample(cv_sd, cvc, mg_sd, mgc, cr_sd, crc, num_frames=17, batch_size=B, context=ctx, steps=2,
                                    cond_scale=5., noise_fn=nf_cpu, trace=trace_ref, trace_logits=True)
    vid, ids = ph.sample(texts=['x'] * B, num_frames=17, cond_scale=5., _noise_fn=lambda k, s, sh: nf_cpu(k, s, sh).cuda(),
                         _trace=trace, _return_ids=True, _compact=True)
    flips, matched, topk_diverged = 0, 0, False
    for s, (a, b) in enumerate(zip(trace_ref, trace)):
        if not torch.equal(a['masked_ids'], b['masked_ids'].cpu()):
            # the re-masked set is a top-k over critic scores: in the f32-grade modes it must be the oracle's; in bf16 (scores off by ~1e-2 of
            # their scale, 4 608 candidates around the k-th rank) a boundary swap is a near tie of the same kind as an audited argmax flip
            assert dtype not in F32_GRADE, f'{dtype} step {s}: masked input ids differ'
            n_diff = int((a['mask'] != b['mask'].cpu()).sum())
            assert n_diff <= 2 * 8 * 6, f'bf16 step {s}: {n_diff} positions of the re-masked sets differ (more than boundary swaps)'
            topk_diverged = True
            break
        rows = a['mask']                                           # compact head: predictions exist at the masked positions only
        noisy = gumbel_noisy(a['logits'], a['temperature'], nf_cpu('gumbel', s, a['logits'].shape))
        f = argmax_equal_with_margin(b['pred'], a['pred'], noisy, tol=mtol, what=f'{dtype} B=8 step {s} pred', rows=rows)
        flips += f
        if f:
            break                                                  # an audited near tie changes the next step's input
        matched += 1
    e_pix = None
    if torch.equal(ids_ref, ids.cpu()):
        e_pix = close(vid[:2], vid_ref[:2], tol, f'sampled pixels {dtype} B=8')
    if dtype in F32_GRADE:
        assert flips <= 2, f'{dtype}: {flips} audited near-tie flips in two steps of 8 x 576 positions'
    record_parity('sample_b8_free_running_2step_vs_oracle', dict(dtype=dtype, batch=B, steps_bit_identical=matched, of=2, audited_argmax_flips=flips,
                                                                 topk_boundary_diverged=topk_diverged, final_ids_equal=bool(torch.equal(ids_ref, ids.cpu())), pixel_rel_err=e_pix))


def _forced_inputs(B, fractions, seed):
    """masked MaskGit inputs (B, 576) per step: random ids with the given fraction of positions masked (a different set per sequence)"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for frac in fractions:
        ids = torch.randint(0, V, (B, 576), generator=g)
        k = int(round(frac * 576))
        pick = torch.rand((B, 576), generator=g).argsort(dim=-1)[:, :k]
        ids.scatter_(1, pick, MASK_ID)
        out.append(ids)
    return out


def _teacher_forced(dtype, mtol, B, fractions, seed, chunk):
    _, mg_sd, _ = state_dicts('full')
    _, mgc, _ = oracle_cfgs(FULL)
    steps = len(fractions)
    _, _, _, ph = load_product('full', FULL, steps=max(steps, 2), dtype=dtype)
    ctx = _ctx(B)
    ph.encode_texts = lambda texts, output_device=None: ctx.cuda()
    inputs = _forced_inputs(B, fractions, seed)

    def force(step, ids, mask):
        inp = inputs[min(step, steps - 1)].cuda()
        ids.copy_(inp)
        mask.copy_((inp == MASK_ID).to(mask.dtype))

    noise = {}

    def nf_cpu(kind, step, shape):
        if (kind, step) not in noise:
            noise[(kind, step)] = weights.uniform_noise(tuple(shape), seed + 2 * step + (1 if kind == 'critic' else 0))
        return noise[(kind, step)]

    trace = []
    ph.sample(texts=['x'] * B, num_frames=17, cond_scale=5., _noise_fn=lambda k, s, sh: nf_cpu(k, s, sh).cuda(), _trace=trace, _force_fn=force)
    exact, flips, nsteps = 0, 0, max(steps, 2)
    for s in range(steps):
        t, inp = trace[s], inputs[s]
        assert torch.equal(t['masked_ids'].cpu(), inp)
        masked = inp == MASK_ID
        temperature = 0.9 * ((nsteps - (s + 1)) / nsteps)
        u = nf_cpu('gumbel', s, (B, 576, V))
        ok = True
        for c0 in range(0, B, chunk):                                 # the oracle is per sequence: bound its (chunk, 576, 65 536) buffers
            sl = slice(c0, c0 + chunk)
            with O.precision(dtype):
                logits = O.maskgit_cfg(mg_sd, mgc, inp[sl], cond_scale=5., video_patch_shape=(9, 8, 8), context=ctx[sl], text_mask=(ctx[sl] != 0).any(-1))
            noisy = gumbel_noisy(logits, temperature, u[sl])
            f = argmax_equal_with_margin(t['pred'][sl], noisy.argmax(-1), noisy, tol=mtol, what=f'{dtype} B={B} forced step {s} pred', rows=masked[sl])
            flips += f
            ok = ok and f == 0
        exact += int(ok)
    return exact, flips


@pytest.mark.parametrize('dtype,tol,mtol', MODES)
def test_sample_at_bench_batch_teacher_forced_matches_oracle(dtype, tol, mtol):
    """B = 8, two forced steps: 50 % masked (2 304 rows -> the resident vocabulary head in bf16) and 20 % masked (920 rows -> the tiled one)"""
    exact, flips = _teacher_forced(dtype, mtol, 8, (0.5, 0.2), 1500, chunk=8)
    if dtype in F32_GRADE:
        assert flips <= 2, f'{dtype}: {flips} audited near ties in 2 forced steps at B = 8'
    record_parity('sample_b8_teacher_forced_vs_oracle', dict(dtype=dtype, batch=8, steps_bit_identical=exact, of=2, audited_argmax_flips=flips))


@pytest.mark.parametrize('dtype,mtol', [('bf16x3', 1e-4), ('bf16', BF16_E2E)])
def test_sample_b32_one_teacher_forced_step_matches_oracle(dtype, mtol):
    """the `sample_b32` leg's shapes: M = 36 864-row trunk GEMMs (L2 panels), 18 432 masked rows in the vocabulary head; one forced step"""
    exact, flips = _teacher_forced(dtype, mtol, 32, (1.0,), 1700, chunk=8)
    if dtype in F32_GRADE:
        assert flips <= 4, f'{dtype}: {flips} audited near ties in one forced step at B = 32'
    record_parity('sample_b32_teacher_forced_vs_oracle', dict(dtype=dtype, batch=32, steps_bit_identical=exact, of=1, audited_argmax_flips=flips))


def test_bench_plain_run_times_its_steps_and_dumps_the_last_ids(tmp_path):
    """`bench.py --steps K --dump-outputs DIR`: the headline alone, K timed steps behind ms_per_step, and DIR/ids.npy holding the token ids of
    the last timed step -- the ids CViViT.forward(video, return_only_codebook_ids=True) returns for that step's input batch."""
    import importlib.util
    import json
    import os
    import subprocess
    import sys
    import numpy as np
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    steps = 4
    r = subprocess.run([sys.executable, os.path.join(root, 'bench.py'), '--gpus', '1', '--steps', str(steps), '--warmup', '1',
                        '--dump-outputs', str(tmp_path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    d = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith('{')][-1])
    assert d['metric'] == 'cvivit_encode_frames_per_sec' and d['unit'] == 'frames/s' and d['higher_is_better'] and d['dtype'] == 'bf16'
    assert d['steps'] == steps and d['ms_per_step'] > 0
    assert abs(d['value'] - 8 * 17 / (d['ms_per_step'] * 1e-3)) < 1e-3 * d['value']            # the line rounds ms_per_step to 0.1 us
    assert not {'roofline', 'kernels', 'sample', 'legs', 'parity', 'cpu_baseline', 'full_report'} & set(d), 'a plain run is the headline only'
    ids = np.load(os.path.join(str(tmp_path), 'ids.npy'))
    assert ids.dtype == np.float64 and ids.shape == (8, 9, 8, 8)
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(root, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    cv = bench.build_models('bf16', False)[0]
    video = bench.synthetic_video(8, 17, 256, seed=(steps - 1) % 3).cuda()            # the steps rotate through 3 input batches
    want = cv(video, return_only_codebook_ids=True).cpu().numpy().astype(np.float64)
    assert np.array_equal(ids, want), f'{int((ids != want).sum())} of {ids.size} dumped ids differ from a direct encode of the same batch'
