"""CPU-only checks: the C-ABI library loads and exports every symbol include/phenaki_hip.h declares, the module tree
reproduces the reference's state_dict contract, host-side logic (shape helpers, mask schedule, asserts, sharding),
and the world_size-2 gloo path of the batch-sharded sampler.  No kernel is launched here."""
import json
import os
import re
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import phenaki_oracle as O
from oracle.configs import TINY, FULL

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
torch.set_grad_enabled(False)      # inference surface; the loss-value forwards refuse to run where a caller could expect gradients


@pytest.fixture(scope='module')
def built_lib():
    from phenaki_pytorch_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_library_exports_every_declared_symbol(built_lib):
    from phenaki_pytorch_amd import _lib
    header = open(os.path.join(ROOT, 'include', 'phenaki_hip.h')).read()
    declared = set(re.findall(r'^int (pk_\w+)\(', header, flags=re.M))
    assert len(declared) >= 18
    assert declared == set(_lib.SIGNATURES), f'header / binding mismatch: {declared ^ set(_lib.SIGNATURES)}'
    for name in declared:
        assert hasattr(built_lib, name), f'{name} is declared but not exported'
    # argument counts of the ctypes table follow the header
    for name in declared:
        proto = re.search(r'^int ' + name + r'\((.*?)\);', header, flags=re.M | re.S).group(1)
        nargs = len([a for a in proto.split(',') if a.strip()])
        assert nargs == len(_lib.SIGNATURES[name]), f'{name}: header has {nargs} args, binding {len(_lib.SIGNATURES[name])}'


def test_pure_host_entry_points(built_lib):
    from phenaki_pytorch_amd import _lib
    assert _lib.vocab_ntiles(65536) == 512 and _lib.vocab_ntiles(256) == 2
    assert _lib.attn_pads(576, 576, 0) == (576, 576)
    assert _lib.attn_pads(9, 9, 0) == (16, 32)
    assert _lib.attn_pads(64, 12, 2) == (64, 32)
    assert _lib.attn_pads(640, 640, 0) == (640, 640)
    with pytest.raises(RuntimeError, match='PK_EINVAL'):
        _lib.attn_pads(0, 5, 0)


def test_no_cpu_fallback():
    import phenaki_pytorch_amd as P
    cv = P.CViViT(use_vgg_and_gan=False, **TINY['cvivit'])
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        cv(torch.randn(1, 3, 5, 64, 64), return_only_codebook_ids=True)
    # the product never imports the oracle (test infrastructure only)
    pkg = os.path.join(ROOT, 'phenaki_pytorch_amd')
    for f in os.listdir(pkg):
        if f.endswith('.py'):
            src = open(os.path.join(pkg, f)).read()
            assert not re.search(r'^\s*(from|import)\s+oracle', src, flags=re.M), f'{f} imports the oracle'


@pytest.mark.parametrize('tag,cfgs', [('tiny', TINY), ('full', FULL)])
def test_state_dict_contract(golden_dir, tag, cfgs):
    import phenaki_pytorch_amd as P
    keys = json.load(open(os.path.join(golden_dir, 'state_dict_keys.json')))
    with torch.device('meta'):
        mods = dict(cvivit=P.CViViT(use_vgg_and_gan=False, **cfgs['cvivit']), maskgit=P.MaskGit(**cfgs['maskgit']),
                    critic=P.TokenCritic(**cfgs['critic']))
    for kind, m in mods.items():
        ref = keys[f'{tag}.{kind}']
        got = {k: [list(v.shape), str(v.dtype)] for k, v in m.state_dict().items()}
        assert got == ref, f'{kind}: {set(got) ^ set(ref)}'


def test_reference_checkpoint_with_gan_keys_loads():
    import phenaki_pytorch_amd as P
    cv = P.CViViT(use_vgg_and_gan=False, **TINY['cvivit'])
    sd = dict(cv.state_dict())
    sd['discr.blocks.0.weight'] = torch.zeros(3)
    sd['vgg.features.0.weight'] = torch.zeros(3)
    cv.load_state_dict(sd)


def test_gan_tokenizer_state_dict_contract(golden_dir):
    """CViViT(use_vgg_and_gan=True, vgg=...) carries the reference's `discr.*` entries (names and shapes from the REAL reference,
    tests/golden/gan_tiny.pt) and never the perceptual network's (cvivit.py:35-49 @remove_vgg); copy_for_eval drops both (:412-421)"""
    import os
    import warnings
    import phenaki_pytorch_amd as P
    from oracle import weights
    from oracle.configs import gan_state_dict
    g = torch.load(os.path.join(golden_dir, 'gan_tiny.pt'), weights_only=False)
    cv = P.CViViT(use_vgg_and_gan=True, vgg=weights.stub_vgg(TINY['cvivit']['image_size']), **TINY['cvivit'])
    sd = cv.state_dict()
    assert {k: list(v.shape) for k, v in sd.items() if k.startswith('discr.')} == {k: list(v) for k, v in g['discr_keys'].items()}
    assert not any(k.startswith('vgg.') for k in sd) and isinstance(cv.vgg, torch.nn.Module)
    ref_sd = gan_state_dict('tiny', g['discr_keys'])
    assert set(ref_sd) == set(sd)
    cv.load_state_dict({**ref_sd, 'vgg.0.weight': torch.zeros(1)})         # a checkpoint that (wrongly) carries vgg entries still loads
    assert torch.equal(cv.discr.blocks[0].conv_res.weight, ref_sd['discr.blocks.0.conv_res.weight'])
    ev = cv.copy_for_eval()
    assert ev.discr is None and ev.vgg is None and not any(k.startswith('discr.') for k in ev.state_dict())
    # the default (no vgg=, no torchvision offline): the module still builds -- with its discriminator -- and says what the GAN step will need
    with warnings.catch_warnings(record=True) as w:
        warnings.simplefilter('always')
        d = P.CViViT(**TINY['cvivit'])
    assert d.discr is not None and (d.vgg is not None or any('vgg' in str(x.message) for x in w))


def test_bench_compact_line_is_what_the_driver_parses():
    """round 3's driver record had `parsed: null` because the stdout line had grown to 22 KB.  bench.compact_line on a REAL full report (the committed
    round-4 one) must stay under 4 KB, be one JSON object, and carry the contract's keys plus roofline and cpu_baseline."""
    import importlib.util
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    full_path = os.path.join(root, 'profiles', 'bench_r04.json')
    if not os.path.exists(full_path):
        pytest.skip('no committed full report')
    spec = importlib.util.spec_from_file_location('bench_mod', os.path.join(root, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    full = json.load(open(full_path))
    line = json.dumps(bench.compact_line(full), separators=(',', ':'))
    assert len(line) <= 4000 and '\n' not in line
    d = json.loads(line)
    for k in ('metric', 'value', 'unit', 'n_gpus', 'steps', 'warmup', 'ms_per_step', 'higher_is_better', 'scaling', 'vs_baseline', 'dtype', 'data', 'config'):
        assert k in d, k
    assert d['config']['workload'].startswith('BASELINE configs[1]') and 'model' not in d['config']
    assert {'bound', 'achieved', 'peak', 'unit', 'frac', 'traffic'} <= set(d['roofline'])
    assert abs(d['roofline']['frac'] - d['roofline']['achieved'] / d['roofline']['peak']) < 1e-3
    assert {'value', 'unit', 'cores', 'kind', 'sample'} <= set(d['cpu_baseline']) and d['cpu_baseline']['kind'] in ('port', 'reference')
    assert d['parity']['dtype'] == 'bf16x3' and d['sample']['unit'] == 'tokens/s'


def test_shape_helpers_and_schedule():
    import phenaki_pytorch_amd as P
    from phenaki_pytorch_amd.phenaki import mask_schedule
    cv = P.CViViT(use_vgg_and_gan=False, **{**TINY['cvivit'], 'image_size': 256, 'patch_size': 32})
    assert cv.image_num_tokens == 64 and cv.patch_height_width == (8, 8)
    assert cv.get_video_patch_shape(17) == (9, 8, 8)
    assert cv.get_video_patch_shape(19 + 5) == (12, 8, 8)
    assert cv.num_tokens_per_frames(17) == 576
    assert cv.num_tokens_per_frames(14, include_first_frame=False) == 448
    with pytest.raises(AssertionError):
        cv.num_tokens_per_frames(16)
    assert mask_schedule(576, 18)[1:] == [574, 567, 556, 541, 522, 499, 472, 441, 407, 370, 330, 288, 243, 197, 149, 100, 50]
    assert mask_schedule(448, 18)[1:] == [446, 441, 433, 421, 406, 388, 367, 343, 317, 288, 257, 224, 189, 153, 116, 78, 39]
    assert mask_schedule(576, 18) == O.mask_schedule(576, 18)
    fm = torch.ones(2, 5, dtype=torch.bool)
    fm[1, 3:] = False
    tm = cv.calculate_video_token_mask(torch.zeros(2, 3, 5, 256, 256), fm)
    assert tm.shape == (2, 3 * 64) and tm[0].all() and tm[1, :128].all() and not tm[1, 128:].any()


def test_phenaki_constructor_contract():
    import phenaki_pytorch_amd as P
    cv = P.CViViT(use_vgg_and_gan=False, **TINY['cvivit'])
    mg = P.MaskGit(**TINY['maskgit'])
    cr = P.TokenCritic(**TINY['critic'])
    ph = P.Phenaki(maskgit=mg, cvivit=cv, critic=cr)
    assert ph.text_embed_dim == 768 and ph.steps == 18 and ph.mask_id == 256
    assert ph.cvivit is not cv and not ph.cvivit.training           # copy_for_eval (phenaki_pytorch.py:361)
    with pytest.raises(AssertionError):
        P.Phenaki(maskgit=mg, cvivit=cv, critic=P.TokenCritic(**{**TINY['critic'], 'has_cross_attn': False}))
    with pytest.raises(AssertionError):
        P.Phenaki(maskgit=mg, cvivit=cv, cond_drop_prob=0.)
    with pytest.raises(AssertionError):
        mg(torch.zeros(1, 3, dtype=torch.long))                     # video patch shape must be given
    with pytest.raises(AssertionError):
        mg(torch.zeros(1, 500, dtype=torch.long), video_patch_shape=(5, 10, 10))   # n > max_seq_len
    # Phenaki.forward keeps the reference's argument asserts (phenaki_pytorch.py:574-579) and never falls back to the CPU
    with pytest.raises(AssertionError):
        ph(torch.zeros(1, 3, 5, 64, 64), video_codebook_ids=torch.zeros(1, 3, 4, 4, dtype=torch.long), texts=['a'])
    with pytest.raises(AssertionError):
        ph(video_codebook_ids=torch.zeros(1, 3, 4, 4, dtype=torch.long))            # neither texts nor text_embeds
    with pytest.raises(AssertionError):
        ph(video_codebook_ids=torch.zeros(1, 3, 4, 4, dtype=torch.long), text_embeds=torch.zeros(1, 4, 5))   # wrong text dim
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        ph(video_codebook_ids=torch.zeros(1, 3, 4, 4, dtype=torch.long), text_embeds=torch.zeros(1, 4, 768))


def test_shard_batch_partitions():
    from phenaki_pytorch_amd.dist import shard_batch
    for n, ws in [(32, 8), (8, 8), (10, 4), (3, 2), (7, 3)]:
        parts = [shard_batch(n, r, ws) for r in range(ws)]
        assert parts[0][0] == 0 and parts[-1][1] == n
        assert all(a[1] == b[0] for a, b in zip(parts, parts[1:]))
        assert max(h - l for l, h in parts) - min(h - l for l, h in parts) <= 1


class _FakePhenaki:
    """stands in for the GPU sampler: the 'video' encodes which text produced it, so the gather order is checkable."""

    def sample(self, *, num_frames, texts=None, prime_frames=None, batch_size=1, **kw):
        vals = torch.tensor([float(t) for t in texts])
        v = vals[:, None, None, None, None].expand(len(texts), 3, num_frames, 4, 4).clone()
        if prime_frames is not None:
            v = v + prime_frames[:, :, -1:].mean(dim=(1, 2, 3, 4), keepdim=True) * 0.001
        return v


def _worker(rank, ws, port, n_items, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=ws)
    sys.path.insert(0, ROOT)
    from phenaki_pytorch_amd.dist import sample_sharded, make_video_sharded, shard_batch
    texts = [str(i) for i in range(n_items)]
    full = sample_sharded(_FakePhenaki(), num_frames=5, texts=texts)
    local = sample_sharded(_FakePhenaki(), num_frames=5, texts=texts, gather=False)
    lo, hi = shard_batch(n_items, rank, ws)
    ok = full.shape == (n_items, 3, 5, 4, 4) and torch.equal(full[:, 0, 0, 0, 0], torch.arange(n_items).float())
    ok = ok and local.shape[0] == hi - lo and torch.equal(local, full[lo:hi])
    mv = make_video_sharded(_FakePhenaki(), [[str(i), str(i + 100)] for i in range(n_items)], (5, 4), 3)
    ok = ok and mv.shape == (n_items, 3, 9, 4, 4) and torch.allclose(mv[:, 0, 0, 0, 0], torch.arange(n_items).float())
    ok = ok and torch.allclose(mv[:, 0, 5, 0, 0], torch.arange(n_items).float() + 100 + torch.arange(n_items).float() * 0.001, atol=1e-4)
    q.put((rank, bool(ok)))
    dist.destroy_process_group()


@pytest.mark.parametrize('n_items', [4, 5])
def test_sharded_sampling_world_size_2_gloo(n_items):
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000) + n_items
    procs = [ctx.Process(target=_worker, args=(r, 2, port, n_items, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(res) == [(0, True), (1, True)]


def _grad_worker(rank, ws, port, q):
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port))
    dist.init_process_group('gloo', rank=rank, world_size=ws)
    sys.path.insert(0, ROOT)
    from phenaki_pytorch_amd.dist import all_reduce_gradients
    g = torch.Generator().manual_seed(7)
    shapes = [(300, 17), (5,), (1000, 33), (2, 3, 4), (70000,)]
    base = [torch.randn(s, generator=g) for s in shapes]
    params = [torch.nn.Parameter(torch.zeros(s)) for s in shapes] + [torch.nn.Parameter(torch.zeros(3))]     # the last one has no gradient
    for p_, b in zip(params, base):
        p_.grad = b * (rank + 1)                                   # rank r holds (r + 1) * base
    ncoll = all_reduce_gradients(params, bucket_mb=0.15)            # 39 321 floats per bucket: the tensors fall into several buckets
    mean_factor = sum(r + 1 for r in range(ws)) / ws
    ok = all(torch.allclose(p_.grad, b * mean_factor, rtol=1e-6, atol=1e-7) for p_, b in zip(params, base)) and params[-1].grad is None
    for p_, b in zip(params, base):
        p_.grad = b * (rank + 1)
    all_reduce_gradients(params, bucket_mb=64., average=False)      # one bucket, plain sum
    ok = ok and all(torch.allclose(p_.grad, b * sum(r + 1 for r in range(ws)), rtol=1e-6, atol=1e-7) for p_, b in zip(params, base))
    # the overlapped form: hooks start a bucket's all-reduce while backward is still producing the other gradients
    from phenaki_pytorch_amd.dist import GradientReducer
    mk = lambda: torch.nn.Sequential(torch.nn.Linear(40, 300), torch.nn.Tanh(), torch.nn.Linear(300, 300), torch.nn.Tanh(), torch.nn.Linear(300, 7))
    torch.manual_seed(11 + rank)                                   # the replicas are built from DIFFERENT seeds ...
    net = mk()
    unused = torch.nn.Parameter(torch.zeros(9))                    # never receives a gradient: its bucket is flushed by finish()
    plist = list(net.parameters()) + [unused]
    group = dist.new_group([0, 1])                                 # a caller-supplied group: its size (not the global world's) is the divisor
    red = GradientReducer(plist, bucket_mb=0.05, group=group)
    torch.manual_seed(11)
    ok = ok and red.broadcasts >= 1 and all(torch.equal(a, b) for a, b in zip(net.parameters(), mk().parameters()))   # ... and start from rank 0's weights
    ok = ok and all(p_.grad is None for p_ in plist)
    x = torch.randn(16, 40, generator=torch.Generator().manual_seed(100 + rank))
    with torch.enable_grad():
        net(x).square().mean().backward()
    started_early = red.collectives                                # buckets completed during backward were launched from the hooks
    nred = red.finish()
    mine = [p_.grad.clone() for p_ in net.parameters()]
    # reference: every rank recomputes both ranks' gradients locally and averages them
    want = [torch.zeros_like(p_) for p_ in net.parameters()]
    for r in range(ws):
        net.zero_grad()
        xr = torch.randn(16, 40, generator=torch.Generator().manual_seed(100 + r))
        with red.no_sync(), torch.enable_grad():
            net(xr).square().mean().backward()
        for w_, p_ in zip(want, net.parameters()):
            w_ += p_.grad / ws
    # (a parameter without a gradient on ANY rank keeps .grad = None, as under DDP's used-parameter bitmap -- no weight decay, no optimizer state)
    ok = ok and all(torch.allclose(a, b, rtol=1e-5, atol=1e-7) for a, b in zip(mine, want)) and unused.grad is None
    ok = ok and started_early >= 1 and nred == len(red.buckets) and red.collectives == 0
    # the gradients live in the flat arena: every .grad is a view of its bucket's buffer (the all-reduce ran in place, no flatten / copy-back)
    with torch.enable_grad():
        net(x).square().mean().backward()                          # accumulates INTO the views (zero_grad(set_to_none=False) regime)
    red.finish()
    ok = ok and all(p_.grad.data_ptr() == v.data_ptr() for p_, v in zip(red.params, red._views) if p_.grad is not None)
    red.remove()
    # a parameter with a gradient on ONE rank only must be stepped by every rank with the same averaged value
    lone = torch.nn.Parameter(torch.ones(5))
    both = torch.nn.Parameter(torch.ones(5))
    red2 = GradientReducer([both, lone], bucket_mb=64., group=group, broadcast=False)
    with torch.enable_grad():
        ((both * 2.).sum() + ((lone * 3.).sum() if rank == 1 else 0.)).backward()
    red2.finish()
    ok = ok and lone.grad is not None and torch.allclose(lone.grad, torch.full((5,), 1.5)) and torch.allclose(both.grad, torch.full((5,), 2.))
    red2.remove()
    # two reducers whose graphs overlap -- the GAN generator objective also reaches the discriminator's parameters
    # (examples/train_cvivit.py --gan).  Its backward runs under the discriminator reducer's no_sync(); the discriminator step then reduces normally.
    gen, disc = torch.nn.Linear(6, 6), torch.nn.Linear(6, 1)
    r_gen = GradientReducer(list(gen.parameters()), bucket_mb=64., group=group)
    r_disc = GradientReducer(list(disc.parameters()), bucket_mb=64., group=group)
    xin = torch.randn(4, 6, generator=torch.Generator().manual_seed(300 + rank))
    try:
        for _ in range(2):
            gen.zero_grad(set_to_none=True)
            with r_disc.no_sync(), torch.enable_grad():
                disc(gen(xin)).mean().backward()                    # gradients land in disc.* too: dropped below
            r_gen.finish()
            disc.zero_grad(set_to_none=True)
            with torch.enable_grad():
                disc(gen(xin).detach()).square().mean().backward()
            r_disc.finish()
        want_d = []
        for r in range(ws):
            xr = torch.randn(4, 6, generator=torch.Generator().manual_seed(300 + r))
            with torch.enable_grad():
                want_d.append(torch.autograd.grad(disc(gen(xr).detach()).square().mean(), list(disc.parameters())))
        ok = ok and all(torch.allclose(p_.grad, sum(w_[i] for w_ in want_d) / ws, rtol=1e-5, atol=1e-7) for i, p_ in enumerate(disc.parameters()))
    except RuntimeError:
        ok = False
    # ... and without the guard the second backward is refused loudly instead of corrupting a bucket in flight
    gen.zero_grad(set_to_none=True)
    disc.zero_grad(set_to_none=True)
    with torch.enable_grad():
        disc(gen(xin)).mean().backward()
    r_gen.finish()
    refused = False
    try:
        with torch.enable_grad():
            disc(gen(xin).detach()).square().mean().backward()
    except RuntimeError as e:
        refused = 'already being reduced' in str(e)
    r_disc.finish()
    ok = ok and refused
    q.put((rank, bool(ok), ncoll))
    dist.destroy_process_group()


def test_gradient_all_reduce_world_size_2_gloo():
    """the data-parallel gradient exchange of the trainers (cvivit_trainer.py:241-249, phenaki_trainer.py:378-386) as
    an explicit bucketed all-reduce: means / sums over 2 ranks, order-preserving buckets, parameters without a gradient skipped."""
    from phenaki_pytorch_amd.dist import bucket_plan
    assert bucket_plan([5, 5, 5, 20, 3], 10) == [[0, 1], [2], [3], [4]]
    assert bucket_plan([], 10) == [] and bucket_plan([3], 10) == [[0]]
    ctx = mp.get_context('spawn')
    q = ctx.Queue()
    port = 29500 + (os.getpid() % 2000) + 37
    procs = [ctx.Process(target=_grad_worker, args=(r, 2, port, q)) for r in range(2)]
    for p in procs:
        p.start()
    res = [q.get(timeout=120) for _ in procs]
    for p in procs:
        p.join(timeout=60)
    assert sorted(r[:2] for r in res) == [(0, True), (1, True)]
    assert res[0][2] == res[1][2] == 2                              # the same bucket plan on both ranks: [4 small tensors] [the 70 000-element one]


def test_packed_weight_cache_invalidation_and_pointer_checks():
    """packed weights must not go stale silently, and parameter pointers are dtype / layout checked."""
    import phenaki_pytorch_amd as P
    from phenaki_pytorch_amd import _lib
    from phenaki_pytorch_amd.attention import _cache, linear_weight, pack_linear_weight
    mg = P.MaskGit(**TINY['maskgit'])
    lin = mg.to_logits
    w1 = linear_weight(lin, _lib.BF16)
    assert w1.dtype == torch.bfloat16 and linear_weight(lin, _lib.BF16) is w1
    with torch.no_grad():
        lin.weight.mul_(2.)                                   # an optimizer-style in-place update bumps _version
    w2 = linear_weight(lin, _lib.BF16)
    assert w2 is not w1 and torch.equal(w2[:, :lin.weight.shape[1]].float(), lin.weight.detach().to(torch.bfloat16).float())
    lin.weight.data.mul_(0.5)                                 # a .data write does not: explicit invalidation is the contract
    assert linear_weight(lin, _lib.BF16) is w2
    P.invalidate_packed(mg)
    w3 = linear_weight(lin, _lib.BF16)
    assert w3 is not w2 and torch.equal(w3[:, :lin.weight.shape[1]].float(), lin.weight.detach().to(torch.bfloat16).float())
    mg.load_state_dict(mg.state_dict())                       # load_state_dict drops the caches of the whole tree
    assert '_pk_cache' not in lin.__dict__
    linear_weight(lin, _lib.BF16)
    mg.float()                                                # so does every _apply (.to / .cuda / .float)
    assert '_pk_cache' not in lin.__dict__
    # exact-f32 mode with K a multiple of the k-tile hands the kernel the LIVE weight (nothing to go stale)
    assert pack_linear_weight(lin.weight, _lib.F32).data_ptr() == lin.weight.data_ptr()
    # parameters reach the kernels as raw pointers: non-f32 or strided ones are refused
    with pytest.raises(RuntimeError, match='contiguous float32'):
        _lib.f32p(torch.zeros(4, dtype=torch.float16), 'gamma')
    with pytest.raises(RuntimeError, match='contiguous float32'):
        _lib.f32p(torch.zeros(4, 4)[:, 1], 'gamma')
    assert _lib.f32p(torch.zeros(4, 8)[:, :4], 'x', rows_ok=True) and _lib.f32p(None) is None


def test_loss_value_forwards_carry_a_raising_backward():
    """ADVICE r1 + r2: Phenaki.forward / CViViT.forward return loss VALUES.  `loss = model(...)` works with the reference signature in
    the default state (grad mode on, trainable parameters); what fails -- loudly -- is `.backward()` on it.  only_train_critic needs a critic."""
    import phenaki_pytorch_amd as P
    from phenaki_pytorch_amd.attention import value_without_graph
    cv = P.CViViT(use_vgg_and_gan=False, **TINY['cvivit'])
    mg = P.MaskGit(**TINY['maskgit'])
    ph = P.Phenaki(maskgit=mg, cvivit=cv, text_embed_dim=96)
    val = torch.tensor(1.25)
    with torch.enable_grad():
        out = value_without_graph(mg, 'Phenaki.forward', val)
        assert out.requires_grad and float(out.detach()) == 1.25
        with pytest.raises(RuntimeError, match='no backward kernels'):
            out.backward()
        tup = value_without_graph(mg, 'CViViT.forward', (val, torch.zeros(2)))          # (loss, recon): only the loss carries the node
        assert tup[0].requires_grad and not tup[1].requires_grad
        for p_ in mg.parameters():
            p_.requires_grad_(False)
        assert value_without_graph(mg, 'x', val) is val                                 # frozen module: plain value
        with pytest.raises(RuntimeError, match='no CPU fallback'):      # the forwards are not refused up front any more: they reach the device check
            cv(torch.randn(1, 3, 5, 64, 64))
        with pytest.raises(RuntimeError, match='no CPU fallback'):
            cv(torch.randn(1, 3, 5, 64, 64), return_only_codebook_ids=True)
    with torch.no_grad():
        assert value_without_graph(ph, 'x', val) is val
        with pytest.raises(AssertionError, match='needs a critic'):
            ph(video_codebook_ids=torch.zeros(1, 3, 4, 4, dtype=torch.long), text_embeds=torch.randn(1, 4, 96), only_train_critic=True)


def test_torch_library_ops_are_registered_without_a_cpu_kernel():
    """the core kernels as torch.library custom ops (phenaki_mi355x::*); schemas register without a GPU, and a CPU tensor
    finds no kernel (the product has no CPU fallback)"""
    import phenaki_pytorch_amd.ops as ops
    for name in ops.OPS:
        assert hasattr(torch.ops.phenaki_mi355x, name), name
    with pytest.raises((NotImplementedError, RuntimeError)):
        torch.ops.phenaki_mi355x.layernorm(torch.randn(4, 8), torch.ones(8), None, torch.empty(4, 8), 1e-5)


def test_data_io_gif_roundtrip_datasets_and_collate(tmp_path):
    """reference data.py:48-265 on PIL: GIF write / read of a (c, f, h, w) tensor, the image / video folder datasets (resize of the shorter
    side, centre crop, frame-count cast) and the string-aware collate"""
    from PIL import Image
    from phenaki_pytorch_amd import data as D
    g = torch.Generator().manual_seed(3)
    # a video with few distinct colours survives GIF's palette exactly
    frames = (torch.randint(0, 4, (3, 6, 1, 1), generator=g).float() / 3).expand(3, 6, 20, 28).contiguous()
    path = tmp_path / 'v.gif'
    D.video_tensor_to_gif(frames, str(path))
    back = D.gif_to_tensor(str(path))
    assert tuple(back.shape) == (3, 6, 20, 28) and (back - frames).abs().max() <= 1 / 255 + 1e-6
    ds = D.VideoDataset(str(tmp_path), image_size=16, num_frames=9)
    v = ds[0]
    assert len(ds) == 1 and tuple(v.shape) == (3, 9, 16, 16) and float(v[:, 6:].abs().max()) == 0.0       # padded to 9 frames
    assert (v[:, :6, 0, 0] - frames[:, :, 0, 0]).abs().max() <= 2 / 255
    assert tuple(D.cast_num_frames(v, frames=4).shape) == (3, 4, 16, 16)
    Image.fromarray((torch.rand(30, 50, 3, generator=g) * 255).byte().numpy()).save(tmp_path / 'a.png')
    Image.fromarray((torch.rand(40, 24, generator=g) * 255).byte().numpy(), mode='L').save(tmp_path / 'b.jpg')
    ids = D.ImageDataset(str(tmp_path), image_size=16)
    assert len(ids) == 2 and all(tuple(ids[i].shape) == (3, 16, 16) and 0 <= float(ids[i].min()) and float(ids[i].max()) <= 1 for i in range(2))
    out = D.collate_tensors_and_strings([(torch.zeros(2), 'a'), (torch.ones(2), 'b')])
    assert tuple(out[0].shape) == (2, 2) and out[1] == ['a', 'b']
    assert tuple(D.collate_tensors_and_strings([torch.zeros(2), torch.ones(2)])[0].shape) == (2, 2)
    dl = D.DataLoader(ids, batch_size=2)
    assert tuple(next(iter(dl))[0].shape) == (2, 3, 16, 16)
    if not _has('cv2'):
        with pytest.raises(ImportError, match='OpenCV'):
            D.video_to_tensor(str(tmp_path / 'x.mp4'))


class _FakeCv2:
    """an in-memory stand-in for the two OpenCV classes the MP4 helpers use (data.py:128-181): VideoWriter keeps the uint8 (h, w, c) frames
    it is given, VideoCapture plays them back -- a lossless "codec", so what is tested is the helpers' own frame / channel / crop logic"""
    store = {}

    @staticmethod
    def VideoWriter_fourcc(*chars):
        return sum(ord(c) << (8 * i) for i, c in enumerate(chars))

    class VideoWriter:
        def __init__(self, path, fourcc, fps, size):
            self.path, self.size = path, size
            _FakeCv2.store[path] = []

        def write(self, frame):
            assert frame.dtype.name == 'uint8' and frame.shape[:2] == (self.size[1], self.size[0])
            _FakeCv2.store[self.path].append(frame.copy())

        def release(self):
            pass

    class VideoCapture:
        def __init__(self, path):
            self.frames, self.i = _FakeCv2.store[path], 0

        def read(self):
            if self.i >= len(self.frames):
                return False, None
            self.i += 1
            return True, self.frames[self.i - 1].copy()

        def release(self):
            pass

    @staticmethod
    def destroyAllWindows():
        pass


# the clip and the read-back keyword sets of the MP4 test; oracle/make_golden.py (`mp4`) ran the reference's helpers on exactly these
_MP4_READS = (dict(), dict(num_frames=3), dict(num_frames=100, crop_size=16), dict(crop_size=(20, 10)))


def _mp4_clip():
    g = torch.Generator().manual_seed(11)
    return torch.randint(0, 256, (3, 7, 24, 40), generator=g).float()


def _fake_cv2():
    import importlib.machinery
    import types
    fake = types.ModuleType('cv2')
    fake.__spec__ = importlib.machinery.ModuleSpec('cv2', None)
    for k in ('VideoWriter_fourcc', 'VideoWriter', 'VideoCapture', 'destroyAllWindows'):
        setattr(fake, k, getattr(_FakeCv2, k))
    return fake


def test_mp4_helpers_match_the_reference_on_a_lossless_stand_in_codec(monkeypatch, golden_dir):
    """SURVEY.md 8f row 4 (video I/O): video_to_tensor / tensor_to_video (reference data.py:128-181) go through OpenCV, which this image lacks.
    With an in-memory cv2 stand-in the product's functions write and read the clip as the reference's own functions did on the same stand-in
    (tests/golden/mp4_helpers.pt): identical frames and tensors, incl. the reference's quirks (the last decoded frame is dropped,
    `[:num_frames]` with the default -1 drops one more, crop_size crops the centre, values stay 0..255 in OpenCV's channel order)."""
    monkeypatch.setitem(sys.modules, 'cv2', _fake_cv2())
    from phenaki_pytorch_amd import data as D
    clip = _mp4_clip()
    D.tensor_to_video(clip, 'mem://a.mp4')
    assert len(_FakeCv2.store['mem://a.mp4']) == 7
    full = D.video_to_tensor('mem://a.mp4', num_frames=100)
    assert tuple(full.shape) == (3, 6, 24, 40) and torch.equal(full, clip[:, :6])                  # the final decoded frame is left out
    assert tuple(D.video_to_tensor('mem://a.mp4').shape) == (3, 5, 24, 40)                          # default num_frames = -1: `[:, :-1]`
    crop = D.video_to_tensor('mem://a.mp4', num_frames=4, crop_size=16)
    assert tuple(crop.shape) == (3, 4, 16, 16) and torch.equal(crop, clip[:, :4, 4:20, 12:28])
    ref = torch.load(os.path.join(golden_dir, 'mp4_helpers.pt'))
    assert torch.equal(torch.stack([torch.from_numpy(f) for f in _FakeCv2.store['mem://a.mp4']]), ref['frames'])
    assert [kw for kw, _ in ref['reads']] == list(_MP4_READS)
    for kw, want in ref['reads']:
        assert torch.equal(D.video_to_tensor('mem://a.mp4', **kw), want.float()), kw


def _has(mod):
    import importlib.util
    return importlib.util.find_spec(mod) is not None


def test_tokenizer_training_row_maps_are_the_reference_rearranges():
    """train_cvivit._frame_indices: the int32 row maps of the tokenizer's training step against the reference's einops patterns
    ('b t h w d -> (b h w) t d' and back, cvivit.py:456-470; tokens[:, :1] / tokens[:, 1:], :505) on a tagged tensor.  Host logic only."""
    from phenaki_pytorch_amd.train_cvivit import _frame_indices
    b, t, h, w = 3, 4, 2, 5
    hw = h * w
    to_temporal, to_spatial, first, rest = (x.long() for x in _frame_indices(b, t, hw, torch.device('cpu')))
    x = torch.arange(b * t * hw, dtype=torch.float32).view(b, t, h, w, 1)
    spatial_rows = x.reshape(b * t * hw, 1)                                     # '(b t) (h w)' row order
    temporal_rows = x.permute(0, 2, 3, 1, 4).reshape(b * hw * t, 1)             # '(b h w) t'
    assert torch.equal(spatial_rows[to_temporal], temporal_rows)
    assert torch.equal(temporal_rows[to_spatial], spatial_rows)
    assert torch.equal(to_temporal[to_spatial], torch.arange(b * t * hw)) and torch.equal(to_spatial[to_temporal], torch.arange(b * t * hw))
    assert torch.equal(spatial_rows[first], x[:, :1].reshape(-1, 1)) and torch.equal(spatial_rows[rest], x[:, 1:].reshape(-1, 1))
    assert sorted(torch.cat((first, rest)).tolist()) == list(range(b * t * hw))
