"""Training-mode cosine-sim VectorQuantize on the pk_vq_* kernels (phenaki_pytorch_amd/csrc/vq_train.hip, train_cvivit._VQFn) against the plain-torch
restatement tests/vq_train_restatement.py -- the formulas of DESIGN.md "VectorQuantize training" (written from memory of the published module;
upstream parity unpinned).

Shapes: D = 128 (the TINY width); V in {256, 4096} (one / four codes per scan thread, both accepted by the f32 lookup kernel); M = 160 without a
mask -- 60 of its rows sit next to three fixed codes, so segments of ~20 rows exist beside single-row and empty codes -- and M = 150 (no multiple
of 64) with a row mask that drops about a third of the rows.  One more case, (V, M, D) = (256, 200, 512), plants 100 rows on ONE code (a segment
longer than a wave: the re-reading branch of the ascending-row walk) at the real width (two 16-byte chunks per lane).  Every case runs ONCE
(three consecutive steps, a repeat of the first from the same state, a no_grad repeat, an eval call); the tests read that record."""
import functools

import pytest
import torch
import torch.nn.functional as F

from tests.util import close
from tests.vq_train_restatement import vq_train_step

pytestmark = pytest.mark.gpu

CASES = [(256, 160, 128), (256, 150, 128), (4096, 160, 128), (4096, 150, 128), (256, 200, 512)]
D = 128
CLUSTER_CODES = (3, 101, 250)
BUFFERS = ('cluster_size', 'embed_avg', 'embed')


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
    return dict(q=q[0].detach().cpu(), ids=ids[0].cpu(), commit=commit.detach().cpu(), dx=xg.grad.cpu(), after=_state(vq))


@functools.lru_cache(maxsize=None)
def run_case(V, M, D):
    import phenaki_pytorch_amd as P
    gen = torch.Generator().manual_seed(1000 * V + M)
    torch.manual_seed(V + M)
    vq = P.quantize.VectorQuantize(dim=D, codebook_size=V).cuda().train()
    E0 = vq._codebook.embed[0].cpu().clone()
    # a codebook state in general position: non-zero cluster sizes, embed_avg no multiple of embed
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
    versions = [getattr(vq._codebook, k)._version for k in BUFFERS]
    steps = [_step(vq, x, keep, g) for x, g in zip(xs, gs)]
    bumped = [getattr(vq._codebook, k)._version > v for k, v in zip(BUFFERS, versions)]
    _set_state(vq, start)
    again = _step(vq, xs[0], keep, gs[0])
    _set_state(vq, start)
    with torch.no_grad():
        q, ids, commit = vq(xs[0].cuda()[None], mask=None if keep is None else keep.cuda()[None])
    nograd = dict(q=q[0].cpu(), ids=ids[0].cpu(), commit=commit.cpu(), requires_grad=q.requires_grad or commit.requires_grad, after=_state(vq))
    vq.eval()
    before_eval = _state(vq)
    q, ids, aux = vq(xs[1].cuda()[None])
    evalrun = dict(q=q[0].cpu(), ids=ids[0].cpu(), aux=aux.cpu(), before=before_eval, after=_state(vq))
    # the restatement, chained over the three steps from the same start with the product's ids
    ref, state = [], start
    for x, g, s in zip(xs, gs, steps):
        xr = x.clone().requires_grad_()
        out = vq_train_step(xr, state['embed'], state['embed_avg'], state['cluster_size'], keep, s['ids'])
        ((out['y'] * g).sum() + 0.7 * out['commit']).backward()
        out['dx'] = xr.grad
        ref.append({k: v.detach() for k, v in out.items()})
        state = {k: out[k] for k in BUFFERS}
    return dict(start=start, keep=keep, xs=xs, steps=steps, again=again, nograd=nograd, eval=evalrun, ref=ref, bumped=bumped)


@pytest.mark.parametrize('V,M,D', CASES)
def test_ids_are_the_cosine_argmax(V, M, D):
    """every row (masked ones included) gets the id of the inference lookup: equal to the CPU argmax wherever the CPU's top-2 margin exceeds 1e-5"""
    r = run_case(V, M, D)
    sim = F.normalize(r['xs'][0], dim=-1) @ r['start']['embed'].t()
    top2 = sim.topk(2, dim=-1).values
    safe = (top2[:, 0] - top2[:, 1]) > 1e-5
    print(f'V={V} M={M}: share of rows with a top-2 margin > 1e-5 = {safe.float().mean():.4f}')
    assert safe.float().mean() > 0.99
    assert torch.equal(r['steps'][0]['ids'][safe], sim.argmax(-1)[safe])
    if M == 160:                                                  # the planted clusters landed on their codes
        for n, j in enumerate(CLUSTER_CODES):
            assert (r['steps'][0]['ids'][20 * n + 5:20 * n + 25] == j).all()


@pytest.mark.parametrize('V,M,D', CASES)
def test_forward_values(V, M, D):
    """q is the codebook row of BEFORE the update, bit for bit; the commitment loss is the restatement's to 1e-6 relative"""
    r = run_case(V, M, D)
    state = r['start']
    for s, ref in zip(r['steps'], r['ref']):
        assert torch.equal(s['q'], state['embed'][s['ids']])
        rel = abs(float(s['commit']) - float(ref['commit'])) / abs(float(ref['commit']))
        print(f'V={V} M={M}: commit {float(s["commit"]):.8f} restatement {float(ref["commit"]):.8f} rel {rel:.2e}')
        assert rel <= 1e-6
        state = s['after']


@pytest.mark.parametrize('V,M,D', CASES)
def test_buffers_after_one_and_three_steps(V, M, D):
    r = run_case(V, M, D)
    assert all(r['bumped']), 'the in-place update must bump the buffers\' _version'
    for n in (0, 2):
        got, ref = r['steps'][n]['after'], r['ref'][n]
        for k in BUFFERS:
            err = close(got[k], ref[k], 1e-5, f'{k} after step {n + 1}')
            print(f'V={V} M={M} step {n + 1}: {k} rel err {err:.2e}')
        norms = got['embed'].double().norm(dim=-1)
        assert (norms - 1).abs().max() <= 1e-6, 'embed rows have unit norm'
    bins = r['ref'][0]['bins']
    assert (bins == 0).any() and (bins == 1).any()
    if M == 160:
        assert bins.max() >= 20
    if M == 200:
        assert bins.max() >= 100                                  # longer than a wave
    unused = bins == 0
    assert torch.equal(r['steps'][0]['after']['embed_avg'][unused], 0.8 * r['start']['embed_avg'][unused]), 'codes without a row: decay only, exactly'


@pytest.mark.parametrize('V,M,D', CASES)
def test_gradient(V, M, D):
    """dx of (y . g).sum() + 0.7 commit: straight through plus the commitment term on the kept rows"""
    r = run_case(V, M, D)
    for s, ref in zip(r['steps'], r['ref']):
        err = close(s['dx'], ref['dx'], 1e-5, 'dx')
        print(f'V={V} M={M}: dx rel err {err:.2e}')
    if r['keep'] is not None:                                    # dropped rows: the straight-through part alone
        dropped = ~r['keep']
        assert torch.equal(r['steps'][0]['dx'][dropped], r['ref'][0]['dx'][dropped])


@pytest.mark.parametrize('V,M,D', CASES)
def test_two_runs_from_one_state_are_bit_identical(V, M, D):
    r = run_case(V, M, D)
    first, again = r['steps'][0], r['again']
    for k in ('q', 'ids', 'commit', 'dx'):
        assert torch.equal(first[k], again[k]), k
    for k in BUFFERS:
        assert torch.equal(first['after'][k], again['after'][k]), k


@pytest.mark.parametrize('V,M,D', CASES)
def test_no_grad_gives_the_same_values_and_update(V, M, D):
    r = run_case(V, M, D)
    first, ng = r['steps'][0], r['nograd']
    assert not ng['requires_grad']
    for k in ('q', 'ids', 'commit'):
        assert torch.equal(first[k], ng[k]), k
    for k in BUFFERS:
        assert torch.equal(first['after'][k], ng['after'][k]), k


@pytest.mark.parametrize('V,M,D', CASES)
def test_eval_mode_is_untouched(V, M, D):
    r = run_case(V, M, D)
    e = r['eval']
    for k in BUFFERS:
        assert torch.equal(e['before'][k], e['after'][k]), k
    assert float(e['aux']) == 0. and e['aux'].ndim == 0
    assert torch.equal(e['q'], e['before']['embed'][e['ids']])


def test_mask_that_keeps_nothing_is_refused():
    import phenaki_pytorch_amd as P
    vq = P.quantize.VectorQuantize(dim=D, codebook_size=256).cuda().train()
    before = _state(vq)
    with pytest.raises(ValueError):
        vq(torch.randn(1, 8, D).cuda(), mask=torch.zeros(1, 8, dtype=torch.bool).cuda())
    after = _state(vq)
    assert all(torch.equal(before[k], after[k]) for k in BUFFERS)


def test_entry_points_refuse_bad_arguments_before_launching():
    """bad D -> PK_EINVAL, a misaligned pointer -> PK_EALIGN, an id outside [0, V) under check_ids -> PK_EINVAL; nothing is launched (the outputs
    keep their sentinel).  Without check_ids the kernels drop such a row on the device instead of indexing with it."""
    from phenaki_pytorch_amd import _lib as L
    lib = L.load()
    M, V = 8, 16
    dev = 'cuda'
    x, E = torch.randn(M, D, device=dev), torch.randn(V, D, device=dev)
    big = torch.randn(M * D + 4, device=dev)
    ids = torch.arange(M, device=dev, dtype=torch.int64)
    y, rowsq = torch.full((M, D), -7., device=dev), torch.full((M,), -7., device=dev)
    st = L.stream(x)
    p = L.ptr
    assert lib.pk_vq_gather_commit(p(x), p(E), p(ids), None, M, V, D - 2, p(y), p(rowsq), st) == -1
    assert lib.pk_vq_gather_commit(p(x), p(E), p(ids), None, M, V, 2048, p(y), p(rowsq), st) == -1
    assert lib.pk_vq_gather_commit(p(x), p(E), p(ids), None, 0, V, D, p(y), p(rowsq), st) == -1
    assert lib.pk_vq_gather_commit(p(x), p(E), p(ids), None, M, 0, D, p(y), p(rowsq), st) == -1
    assert lib.pk_vq_gather_commit(big.data_ptr() + 4, p(E), p(ids), None, M, V, D, p(y), p(rowsq), st) == -2
    assert lib.pk_vq_commit_bwd(p(x), p(x), p(x), None, M, D - 2, 1., None, p(y), st) == -1
    assert lib.pk_vq_commit_bwd(p(x), big.data_ptr() + 4, p(x), None, M, D, 1., None, p(y), st) == -2
    counts = torch.zeros(V, device=dev, dtype=torch.int32)
    offsets, cursor, rows = torch.full_like(counts, -7), torch.full_like(counts, -7), torch.full((M,), -7, device=dev, dtype=torch.int32)
    cs, S = torch.full((V,), -7., device=dev), torch.full((1,), -7., device=dev)
    avg, emb = torch.full((V, D), -7., device=dev), torch.full((V, D), -7., device=dev)
    assert lib.pk_vq_codebook_update(p(x), p(counts), p(offsets), p(rows), p(cs), p(S), M, V, D + 2, 0.8, 1e-5, p(avg), p(emb), st) == -1
    assert lib.pk_vq_codebook_update(big.data_ptr() + 4, p(counts), p(offsets), p(rows), p(cs), p(S), M, V, D, 0.8, 1e-5, p(avg), p(emb), st) == -2
    assert lib.pk_vq_scan(p(counts), 0, 0.8, p(cs), p(offsets), p(cursor), p(S), st) == -1
    assert lib.pk_vq_fill(p(ids), None, 0, V, p(cursor), p(rows), st) == -1
    bad = ids.clone()
    bad[5] = V
    assert lib.pk_vq_hist(p(bad), None, M, V, p(counts), 1, st) == -1
    bad[5] = -1
    assert lib.pk_vq_hist(p(bad), None, M, V, p(counts), 1, st) == -1
    torch.cuda.synchronize()
    for t in (y, rowsq, offsets, cursor, rows, cs, S, avg, emb):
        assert bool((t == -7).all()), 'a refused call wrote something'
    assert int(counts.sum()) == 0
    with pytest.raises(RuntimeError, match='PK_EINVAL'):
        L.vq_gather_commit(x[:, :D - 2].contiguous(), E[:, :D - 2].contiguous(), ids, None, y, rowsq)
    # check_ids = 0 (the training step): the device-side range test drops the row, the other seven are counted
    assert lib.pk_vq_hist(p(bad), None, M, V, p(counts), 0, st) == 0
    assert lib.pk_vq_hist(p(ids), None, M, V, p(counts), 1, st) == 0
    torch.cuda.synchronize()
    assert int(counts.sum()) == 2 * M - 1 and int(counts[5]) == 1
