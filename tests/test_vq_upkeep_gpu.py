"""VectorQuantize upkeep on the GPU -- dead-code expiry inside the EMA update's launches (pk_vq_scan_expire / pk_vq_codebook_update_expire /
pk_vq_compact_keep) and the k-means initialisation (pk_vq_pick_rows / pk_vq_kmeans_means) -- against the plain-torch restatement
tests/vq_upkeep_restatement.py (DESIGN.md "VectorQuantize upkeep"; written from memory of the published module, upstream parity unpinned).

Expiry cases (V, M, D, threshold, reset) reuse the data of tests/test_vq_train_gpu.py: the masked M = 150 case (about 101 kept rows, start
cluster_size = 2 rand) at thresholds 0.5 and 1.5 -- fewer expired codes than kept rows (distinct rows) and more (the choice wraps) --, the
unmasked M = 160 case, V = 4096 (four codes per scan thread; far more expired codes than rows), and (256, 200, 512) with 100 rows on one code.
Every case runs ONCE: at module level (three chained steps, a repeat, a no_grad repeat, the same step with threshold = 0, an eval call; b read
from vq.last_upkeep) and at kernel level (the _lib wrapper with an explicit b); the tests read that record.

k-means cases: M = 1000 clustered rows (24 centres, unit noise in a rank-3 subspace, 0.01 isotropic noise: assignments keep moving after
iteration 0 and no row sits on a near-tie) with a row mask, and M = 160 < V = 256 rows (duplicate seeds, codes that stay empty)."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests import vq_upkeep_restatement as R
from tests.util import close

pytestmark = pytest.mark.gpu

EXPIRY_CASES = [(256, 150, 128, 0.5, None), (256, 150, 128, 1.5, None), (256, 160, 128, 1.0, 0.3), (4096, 150, 128, 0.5, None),
                (256, 200, 512, 1.0, None)]
CLUSTER_CODES = (3, 101, 250)
BUFFERS = ('cluster_size', 'embed_avg', 'embed')
KERNEL_B = 123456789012345


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    torch.cuda.set_device(0)
    with torch.enable_grad():
        yield


def _state(vq):
    cb = vq._codebook
    return {k: getattr(cb, k)[0].detach().cpu().clone() for k in BUFFERS}


def _set_state(vq, state):
    cb = vq._codebook
    with torch.no_grad():
        for k in BUFFERS:
            getattr(cb, k)[0].copy_(state[k])


def _step(vq, x, keep, g):
    xg = x.cuda().requires_grad_()
    q, ids, commit = vq(xg[None], mask=None if keep is None else keep.cuda()[None])
    ((q[0] * g.cuda()).sum() + 0.7 * commit).backward()
    return dict(q=q[0].detach().cpu(), ids=ids[0].cpu(), commit=commit.detach().cpu(), dx=xg.grad.cpu(), after=_state(vq), draws=dict(vq.last_upkeep))


@functools.lru_cache(maxsize=None)
def run_expiry(V, M, D, threshold, reset):
    import phenaki_pytorch_amd as P
    from phenaki_pytorch_amd import _lib as L
    # the generator sequence of tests/test_vq_train_gpu.py::run_case: the same codebook state, mask and rows
    gen = torch.Generator().manual_seed(1000 * V + M)
    torch.manual_seed(V + M)
    vq = P.quantize.VectorQuantize(dim=D, codebook_size=V, threshold_ema_dead_code=threshold, reset_cluster_size=reset, upkeep_seed=5).cuda().train()
    E0 = vq._codebook.embed[0].cpu().clone()
    start = dict(cluster_size=2. * torch.rand(V, generator=gen), embed_avg=E0 * (0.5 + torch.rand(V, 1, generator=gen)), embed=E0)
    _set_state(vq, start)
    keep = (torch.rand(M, generator=gen) > 1. / 3.) if M == 150 else None
    xs, gs = [], []
    for _ in range(3):
        x = torch.randn(M, D, generator=gen)
        if M == 160:
            for n, j in enumerate(CLUSTER_CODES):
                x[20 * n + 5:20 * n + 25] = E0[j] + 0.05 * torch.randn(20, D, generator=gen)
        if M == 200:
            x[50:150] = E0[7] + 0.02 * torch.randn(100, D, generator=gen)
        xs.append(x)
        gs.append(torch.randn(M, D, generator=gen))
    xns = [vq.normalised(x.cuda()).cpu() for x in xs]
    steps = [_step(vq, x, keep, g) for x, g in zip(xs, gs)]
    _set_state(vq, start)
    vq.upkeep_calls = 0
    again = _step(vq, xs[0], keep, gs[0])
    _set_state(vq, start)
    vq.upkeep_calls = 0
    with torch.no_grad():
        q, ids, commit = vq(xs[0].cuda()[None], mask=None if keep is None else keep.cuda()[None])
    nograd = dict(q=q[0].cpu(), ids=ids[0].cpu(), commit=commit.cpu(), requires_grad=q.requires_grad or commit.requires_grad, after=_state(vq))
    # the same step with expiry switched off: what the non-expired codes must hold, bit for bit
    _set_state(vq, start)
    vq.threshold_ema_dead_code = 0
    plain = _step(vq, xs[0], keep, gs[0])
    vq.threshold_ema_dead_code = threshold
    # kernel level: the wrapper with an explicit b on the first step's rows and ids
    _set_state(vq, start)
    cb = vq._codebook
    keep8 = None if keep is None else keep.cuda().to(torch.uint8)
    counts, jrank = L.vq_ema_update_expire(xns[0].cuda(), steps[0]['ids'].cuda(), keep8, cb.cluster_size[0], cb.embed_avg[0], cb.embed[0], vq.decay, vq.eps,
                                           threshold, threshold if reset is None else reset, KERNEL_B)
    kernel = dict(after=_state(vq), counts=counts.cpu(), jrank=jrank.cpu())
    if keep8 is not None:
        kept, n_keep = L.vq_compact_keep(keep8)
        kernel.update(kept=kept.cpu(), n_keep=int(n_keep.cpu()))
    vq.eval()
    before_eval = _state(vq)
    q, ids, aux = vq(xs[1].cuda()[None])
    evalrun = dict(before=before_eval, after=_state(vq), aux=aux.cpu())
    # the restatement, chained over the three steps with the product's ids, its b and its normalised rows
    ref, state = [], start
    for x, xn, s in zip(xs, xns, steps):
        out = R.vq_upkeep_step(x, state['embed'], state['embed_avg'], state['cluster_size'], keep, s['ids'], threshold=threshold, reset=reset,
                               b=s['draws']['expire_b'], xn=xn)
        ref.append(out)
        state = {k: out[k] for k in BUFFERS}
    kref = R.vq_upkeep_step(xs[0], start['embed'], start['embed_avg'], start['cluster_size'], keep, steps[0]['ids'], threshold=threshold, reset=reset,
                            b=KERNEL_B, xn=xns[0])
    return dict(start=start, keep=keep, xs=xs, xns=xns, steps=steps, again=again, nograd=nograd, plain=plain, kernel=kernel, eval=evalrun, ref=ref,
                kref=kref)


def _check_expired(got, ref, xn, value, what):
    """got: the product's buffers; ref: the restatement's step.  Expired codes: the named normalised rows bit for bit, exact embed_avg and
    cluster_size; every buffer to 1e-5 overall."""
    ex, rows = ref['expired'], ref['rows']
    assert torch.equal(got['embed'][ex], xn[rows]), f'{what}: replaced embed rows are the chosen xn rows'
    assert torch.equal(got['embed_avg'][ex], xn[rows] * torch.tensor(value)), f'{what}: embed_avg of expired codes'
    assert bool((got['cluster_size'][ex] == value).all()), f'{what}: cluster_size of expired codes'
    for k in BUFFERS:
        err = close(got[k], ref[k], 1e-5, f'{what}: {k}')
        print(f'{what}: {k} rel err {err:.2e}')


@pytest.mark.parametrize('V,M,D,threshold,reset', EXPIRY_CASES)
def test_expiry_kernel_level(V, M, D, threshold, reset):
    r = run_expiry(V, M, D, threshold, reset)
    k, ref = r['kernel'], r['kref']
    value = threshold if reset is None else reset
    _check_expired(k['after'], ref, r['xns'][0], value, f'kernel V={V} M={M} T={threshold}')
    assert torch.equal(k['jrank'] >= 0, ref['expired'])
    assert torch.equal(k['jrank'][ref['expired']], torch.arange(int(ref['expired'].sum()), dtype=torch.int32))
    assert torch.equal(k['counts'].long(), ref['bins'])
    if r['keep'] is not None:
        kept = R.kept_rows(M, r['keep'])
        assert k['n_keep'] == kept.numel() and torch.equal(k['kept'][:k['n_keep']].long(), kept)
    for name in BUFFERS:                                           # non-expired codes: exactly the plain EMA step
        assert torch.equal(k['after'][name][~ref['expired']], r['plain']['after'][name][~ref['expired']]), name


@pytest.mark.parametrize('V,M,D,threshold,reset', EXPIRY_CASES)
def test_expiry_module_level_three_chained_steps(V, M, D, threshold, reset):
    r = run_expiry(V, M, D, threshold, reset)
    value = threshold if reset is None else reset
    n_keep = M if r['keep'] is None else int(r['keep'].sum())
    n_exp = int(r['ref'][0]['expired'].sum())
    print(f'V={V} M={M} T={threshold}: {n_exp} expired codes, {n_keep} kept rows')
    if (V, M) == (256, 150):                                       # the two regimes the thresholds were chosen for
        assert (n_exp < n_keep) == (threshold == 0.5) and (n_exp > n_keep) == (threshold == 1.5)
    assert 0 < n_exp < V
    for n, (s, ref, xn) in enumerate(zip(r['steps'], r['ref'], r['xns'])):
        assert s['draws'] == dict(call=n, kmeans_b=None, expire_b=R.mix(5, n, R.EXPIRE))
        _check_expired(s['after'], ref, xn, value, f'module V={V} M={M} T={threshold} step {n + 1}')
        rel = abs(float(s['commit']) - float(ref['commit'])) / abs(float(ref['commit']))
        assert rel <= 1e-6
        assert (s['after']['embed'].double().norm(dim=-1) - 1).abs().max() <= 1e-6
    sim = F.normalize(r['xs'][0], dim=-1) @ r['start']['embed'].t()          # ids: the CPU argmax wherever its top-2 margin exceeds 1e-5
    top2 = sim.topk(2, dim=-1).values
    safe = (top2[:, 0] - top2[:, 1]) > 1e-5
    assert safe.float().mean() >= 0.99 and torch.equal(r['steps'][0]['ids'][safe], sim.argmax(-1)[safe])
    ex = r['ref'][0]['expired']
    for name in BUFFERS:
        assert torch.equal(r['steps'][0]['after'][name][~ex], r['plain']['after'][name][~ex]), f'{name}: non-expired codes equal the threshold = 0 step'
    for k in ('q', 'ids', 'commit', 'dx'):                          # S, smoothed, q, the loss and the gradient are those of the plain step
        assert torch.equal(r['steps'][0][k], r['plain'][k]), k
    if M == 200:
        assert int(r['ref'][0]['bins'].max()) >= 100                # a segment longer than a wave, at two 16-byte chunks per lane


@pytest.mark.parametrize('V,M,D,threshold,reset', EXPIRY_CASES)
def test_expiry_repeat_no_grad_and_eval(V, M, D, threshold, reset):
    r = run_expiry(V, M, D, threshold, reset)
    first = r['steps'][0]
    for k in ('q', 'ids', 'commit', 'dx'):
        assert torch.equal(first[k], r['again'][k]), k
    assert not r['nograd']['requires_grad']
    for k in ('q', 'ids', 'commit'):
        assert torch.equal(first[k], r['nograd'][k]), k
    for k in BUFFERS:
        assert torch.equal(first['after'][k], r['again']['after'][k]), f'two runs from one state: {k}'
        assert torch.equal(first['after'][k], r['nograd']['after'][k]), f'a no_grad training call expires too: {k}'
        assert torch.equal(r['eval']['before'][k], r['eval']['after'][k]), f'eval() touches nothing: {k}'
    assert float(r['eval']['aux']) == 0.


# ---------------------------------------------------------------------------------------------------------------- k-means initialisation

def clustered_rows(M, D, seed, centres=24):
    """centres + unit-variance noise in a rank-3 subspace + 0.01 isotropic noise.  The centres are SHORT (0.1 per coordinate, norm about 1.1,
    like the spread around them): after l2 normalisation the rows of one centre still differ in direction, so neighbouring means are told
    apart by margins of 1e-4 and more while assignments keep moving for several iterations (measured on the float64 restatement)."""
    g = torch.Generator().manual_seed(seed)
    c = 0.1 * torch.randn(centres, D, generator=g)
    basis = F.normalize(torch.randn(3, D, generator=g), dim=-1)
    return c[torch.randint(0, centres, (M,), generator=g)] + torch.randn(M, 3, generator=g) @ basis + 0.01 * torch.randn(M, D, generator=g)


KMEANS_CASES = [(256, 1000, 128, 4, True, 0.), (256, 160, 128, 3, False, 0.5)]


@functools.lru_cache(maxsize=None)
def run_kmeans(V, M, D, iters, masked, threshold):
    import phenaki_pytorch_amd as P
    from phenaki_pytorch_amd import _lib as L
    gen = torch.Generator().manual_seed(77 + M)
    torch.manual_seed(3)
    vq = P.quantize.VectorQuantize(dim=D, codebook_size=V, kmeans_init=True, kmeans_iters=iters, threshold_ema_dead_code=threshold,
                                   upkeep_seed=11).cuda().train()
    fresh = dict(initted=bool(vq._codebook.initted.item()), embed_zero=not bool(vq._codebook.embed.any()))
    x = clustered_rows(M, D, seed=M)
    x2 = clustered_rows(M, D, seed=M + 1)
    keep = (torch.rand(M, generator=gen) > 0.25) if masked else None
    g = torch.randn(M, D, generator=gen)
    xn = vq.normalised(x.cuda())
    first = _step(vq, x, keep, g)
    initted_after = bool(vq._codebook.initted.item())
    second = _step(vq, x2, keep, g)
    # kernel level: the procedure as one function with the module's b, on buffers of its own
    keep8 = None if keep is None else keep.cuda().to(torch.uint8)
    means = torch.full((V, D), 7., device='cuda')
    ea, cs = torch.full((V, D), 7., device='cuda'), torch.full((V,), 7., device='cuda')
    b = first['draws']['kmeans_b']
    out_means, bins, ids, trace = L.vq_kmeans(xn, keep8, means, iters, b, vq.ids_of_normalised, embed_avg=ea, cluster_size=cs, trace=True)
    seeds = torch.empty((V, D), device='cuda')
    kept, n_keep = L.vq_compact_keep(keep8) if keep8 is not None else (None, None)
    assert L.load().pk_vq_pick_rows(L.ptr(xn), L.ptr(kept), L.ptr(n_keep), M, V, D, b, L.ptr(seeds), L.stream(xn)) == 0
    kernel = dict(means=out_means.cpu(), bins=bins.cpu(), ids=ids.cpu(), trace=trace.cpu(), embed_avg=ea.cpu(), cluster_size=cs.cpu(), seeds=seeds.cpu())
    xn = xn.cpu()
    ref = R.kmeans(xn, keep, V, iters, b, ids=kernel['ids'])
    pure = R.kmeans(xn, keep, V, iters, b)
    step1 = R.vq_upkeep_step(x, ref['embed'], ref['embed_avg'], ref['cluster_size'], keep, first['ids'], threshold=threshold,
                             b=first['draws']['expire_b'] or 0, xn=xn)
    step2 = R.vq_upkeep_step(x2, step1['embed'], step1['embed_avg'], step1['cluster_size'], keep, second['ids'], threshold=threshold,
                             b=second['draws']['expire_b'] or 0)
    return dict(fresh=fresh, x=x, xn=xn, keep=keep, first=first, second=second, initted_after=initted_after, kernel=kernel, ref=ref, pure=pure, step1=step1,
                step2=step2, b=b)


@pytest.mark.parametrize('V,M,D,iters,masked,threshold', KMEANS_CASES)
def test_kmeans_procedure(V, M, D, iters, masked, threshold):
    r = run_kmeans(V, M, D, iters, masked, threshold)
    k, ref, pure = r['kernel'], r['ref'], r['pure']
    assert r['b'] == R.mix(11, 0, R.KMEANS)
    assert torch.equal(k['seeds'], ref['seeds']), 'the seeds are the chosen kept rows, bit for bit'
    if masked:
        dropped = {tuple(row.tolist()) for row in r['xn'][~r['keep']]}
        assert not any(tuple(row.tolist()) in dropped for row in k['seeds']), 'masked rows never enter the data'
    moved = int((pure['ids'][0] != pure['ids'][1])[R.kept_rows(M, r['keep'])].sum())
    min_margin = min(float(m.min()) for m in pure['margin'])
    print(f'M={M}: {moved} assignments change between iterations 0 and 1; min top-2 margin {min_margin:.3e}; empty codes {int((ref["bins"] == 0).sum())}')
    if M == 1000:                                                   # the data makes the iterations do work, and no row sits on a near-tie
        assert moved >= 10
        assert min_margin >= 1e-5
    else:
        assert int((ref['bins'] == 0).sum()) >= 64                  # fewer rows than codes: duplicate seeds, codes that stay empty
    for it in range(iters):
        safe = ref['margin'][it] > 1e-5
        assert safe.float().mean() >= (0.99 if M == 1000 else 0.)
        sim = r['xn'].double() @ (ref['seeds'].double() if it == 0 else ref['means'][it - 1].double()).t()
        assert torch.equal(k['ids'][it][safe], sim.argmax(-1)[safe]), f'ids of iteration {it}'
        err = close(k['trace'][it], ref['means'][it], 1e-5, f'means after iteration {it}')
        print(f'M={M} iteration {it}: means rel err {err:.2e}, rows with a margin > 1e-5: {safe.float().mean():.4f}')
    if M != 1000:                                                   # identical seeds tie exactly: the lower index wins
        sim = r['xn'] @ ref['seeds'].t()
        assert torch.equal(k['ids'][0], (sim == sim.max(dim=-1, keepdim=True).values).float().argmax(-1))
    assert torch.equal(k['bins'].long(), ref['bins'])
    close(k['means'], ref['embed'], 1e-5, 'embed')
    close(k['embed_avg'], ref['embed_avg'], 1e-5, 'embed_avg')
    assert torch.equal(k['cluster_size'], ref['cluster_size'])
    assert torch.equal(k['embed_avg'], k['means'] * k['cluster_size'][:, None])
    empty = ref['bins'] == 0
    if empty.any() and iters >= 2:
        assert torch.equal(k['means'][empty], k['trace'][-2][empty]), 'a code with no row stays on its old mean'


@pytest.mark.parametrize('V,M,D,iters,masked,threshold', KMEANS_CASES)
def test_kmeans_module_initialises_once_then_steps(V, M, D, iters, masked, threshold):
    r = run_kmeans(V, M, D, iters, masked, threshold)
    assert r['fresh'] == dict(initted=False, embed_zero=True) and r['initted_after']
    first, second = r['first'], r['second']
    assert first['draws']['kmeans_b'] is not None and second['draws']['kmeans_b'] is None, 'a second training call does not re-initialise'
    # the step after initialisation: lookup against the NEW codebook, commitment loss, EMA update (and expiry) from the initialised state
    assert torch.equal(first['q'], r['kernel']['means'][first['ids']])
    for name, s, ref in (('first', first, r['step1']), ('second', second, r['step2'])):
        for k in BUFFERS:
            err = close(s['after'][k], ref[k], 1e-5, f'{name} call: {k}')
            print(f'M={M} {name} call: {k} rel err {err:.2e}')
        rel = abs(float(s['commit']) - float(ref['commit'])) / abs(float(ref['commit']))
        assert rel <= 1e-6
    if threshold > 0:
        ex = r['step1']['expired']
        assert ex.any() and torch.equal(first['after']['embed'][ex], r['xn'][r['step1']['rows']])
    assert torch.equal(second['q'], first['after']['embed'][second['ids']])


# ---------------------------------------------------------------------------------------------------------------------------- refusals

def test_entry_points_refuse_bad_arguments_before_launching():
    from phenaki_pytorch_amd import _lib as L
    lib = L.load()
    M, V, D = 8, 16, 128
    dev = 'cuda'
    x = torch.randn(M, D, device=dev)
    big = torch.randn(M * D + 4, device=dev)
    counts = torch.zeros(V, device=dev, dtype=torch.int32)
    offsets, cursor, jrank = (torch.full_like(counts, -7) for _ in range(3))
    rows, kept, n_keep = torch.full((M,), -7, device=dev, dtype=torch.int32), torch.full((M,), -7, device=dev, dtype=torch.int32), \
        torch.full((1,), -7, device=dev, dtype=torch.int32)
    keep = torch.ones(M, device=dev, dtype=torch.uint8)
    cs, S = torch.full((V,), -7., device=dev), torch.full((1,), -7., device=dev)
    avg, emb = torch.full((V, D), -7., device=dev), torch.full((V, D), -7., device=dev)
    st, p = L.stream(x), L.ptr
    EINVAL, EALIGN = -1, -2
    assert lib.pk_vq_scan_expire(p(counts), V, 0.8, -0.5, p(cs), p(offsets), p(cursor), p(S), p(jrank), st) == EINVAL       # negative threshold
    assert lib.pk_vq_scan_expire(p(counts), V, 0.8, 1.0, p(cs), p(offsets), p(cursor), p(S), None, st) == EINVAL
    assert lib.pk_vq_scan_expire(p(counts), 0, 0.8, 1.0, p(cs), p(offsets), p(cursor), p(S), p(jrank), st) == EINVAL
    assert lib.pk_vq_compact_keep(None, M, p(kept), p(n_keep), st) == EINVAL
    assert lib.pk_vq_compact_keep(p(keep), 0, p(kept), p(n_keep), st) == EINVAL
    assert lib.pk_vq_compact_keep(p(keep), M, p(kept) + 2, p(n_keep), st) == EALIGN

    def update(xn=p(x), D_=D, reset=1., b=3, jr=p(jrank), kp=None, nk=None, ea=p(avg)):
        return lib.pk_vq_codebook_update_expire(xn, p(counts), p(offsets), p(rows), p(cs), p(S), jr, kp, nk, M, V, D_, 0.8, 1e-5, reset, b, ea, p(emb), st)
    assert update(D_=D + 2) == EINVAL                                                 # D % 4 != 0
    assert update(reset=-1.) == EINVAL and update(b=-1) == EINVAL
    assert update(jr=None) == EINVAL and update(ea=None) == EINVAL
    assert update(kp=p(kept)) == EINVAL                                               # a kept list without its length
    assert update(xn=big.data_ptr() + 4) == EALIGN
    assert lib.pk_vq_pick_rows(p(x), None, None, M, V, D + 2, 3, p(emb), st) == EINVAL
    assert lib.pk_vq_pick_rows(p(x), None, None, M, V, D, -3, p(emb), st) == EINVAL
    assert lib.pk_vq_pick_rows(None, None, None, M, V, D, 3, p(emb), st) == EINVAL
    assert lib.pk_vq_kmeans_means(p(x), p(counts), p(offsets), p(rows), M, V, D + 2, p(emb), None, None, st) == EINVAL
    assert lib.pk_vq_kmeans_means(p(x), p(counts), p(offsets), p(rows), M, V, D, None, None, None, st) == EINVAL
    assert lib.pk_vq_kmeans_means(p(x), p(counts), p(offsets), p(rows), M, V, D, p(emb), p(avg), None, st) == EINVAL
    assert lib.pk_vq_kmeans_means(p(x), p(counts), p(offsets), p(rows), M, V, D, big.data_ptr() + 4, None, None, st) == EALIGN
    with pytest.raises(RuntimeError, match='PK_EINVAL'):                               # kmeans_iters < 1
        L.vq_kmeans(x, None, emb, 0, 3, lambda data, means: None)
    with pytest.raises(RuntimeError, match='PK_EINVAL'):
        L.vq_ema_update_expire(x, torch.zeros(M, device=dev, dtype=torch.int64), None, cs, avg, emb, 0.8, 1e-5, -1., 1., 3)
    import phenaki_pytorch_amd as P
    for kw in (dict(threshold_ema_dead_code=-1), dict(kmeans_init=True, kmeans_iters=0)):
        vq = P.quantize.VectorQuantize(dim=D, codebook_size=256, **kw).cuda().train()
        with pytest.raises(ValueError):
            vq(torch.randn(1, M, D, device=dev))
    torch.cuda.synchronize()
    for t in (offsets, cursor, jrank, rows, kept, n_keep, cs, S, avg, emb):
        assert bool((t == -7).all()), 'a refused call wrote something'
