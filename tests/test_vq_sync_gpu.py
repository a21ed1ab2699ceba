"""Cross-rank VectorQuantize statistics (sync_codebook): two ranks under an initialised process group -- RCCL with one rank per device when two
devices are visible, gloo with both ranks on the one GPU otherwise -- each quantise their own masked rows with k-means initialisation and
dead-code expiry switched on.  Every rank all-gathers xn, ids and keep and runs the same deterministic kernels over the rows of both in rank
order, so the codebook buffers must be bit-identical across the ranks and equal the restatement (tests/vq_upkeep_restatement.py) run on the
concatenation; q, the commitment loss and its gradient stay each rank's own.  ONE spawn serves every assertion."""
import os
import warnings

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
import torch.nn.functional as F

from tests import vq_upkeep_restatement as R
from tests.test_dist_gpu import _free_port
from tests.test_vq_upkeep_gpu import clustered_rows
from tests.util import close

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
V, D, M, ITERS, THRESHOLD, SEED = 256, 128, 500, 3, 1.9, 21       # (no sum 0.8 a + 0.2 b of bin counts equals 1.9: no code sits on the threshold)
BUFFERS = ('cluster_size', 'embed_avg', 'embed')


def _rows(rank, step):
    x = clustered_rows(M, D, seed=100 + 10 * rank + step)
    keep = torch.rand(M, generator=torch.Generator().manual_seed(200 + 10 * rank + step)) > 0.25
    return x, keep


def _sync_rank(rank, ws, port, out_dir):
    import sys
    sys.path.insert(0, ROOT)
    os.environ.update(MASTER_ADDR='127.0.0.1', MASTER_PORT=str(port), HSA_ENABLE_IPC_MODE_LEGACY='0')
    dev = rank % max(1, torch.cuda.device_count())
    torch.cuda.set_device(dev)
    if torch.cuda.device_count() >= 2:
        dist.init_process_group('nccl', rank=rank, world_size=ws, device_id=torch.device('cuda', dev))
    else:
        dist.init_process_group('gloo', rank=rank, world_size=ws)
    import phenaki_pytorch_amd as P
    from phenaki_pytorch_amd import _lib as L
    torch.manual_seed(rank)                                        # (nothing random may reach the codebook: it starts at zeros)
    vq = P.quantize.VectorQuantize(dim=D, codebook_size=V, kmeans_init=True, kmeans_iters=ITERS, threshold_ema_dead_code=THRESHOLD,
                                   upkeep_seed=SEED).to(f'cuda:{dev}').train()
    record = []
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        for step in range(2):
            x, keep = _rows(rank, step)
            xg = x.to(f'cuda:{dev}').requires_grad_()
            xn = vq.normalised(xg.detach())
            if step == 0:
                # the k-means assignments of every iteration, for the restatement: the procedure itself on the gathered rows, on scratch buffers
                keep8 = keep.to(f'cuda:{dev}').to(torch.uint8)
                gx, gk = (torch.empty((ws * M, *t.shape[1:]), device=t.device, dtype=t.dtype) for t in (xn, keep8))
                dist.all_gather_into_tensor(gx, xn)
                dist.all_gather_into_tensor(gk, keep8)
                scratch = torch.empty((V, D), device=f'cuda:{dev}')
                _, _, kmeans_ids = L.vq_kmeans(gx, gk, scratch, ITERS, R.mix(SEED, 0, R.KMEANS), vq.ids_of_normalised)
            with torch.enable_grad():
                q, ids, commit = vq(xg[None], mask=keep.to(f'cuda:{dev}')[None])
                commit.backward()
            cb = vq._codebook
            record.append(dict(ids=ids[0].cpu(), commit=commit.detach().cpu(), dx=xg.grad.cpu(), xn=xn.cpu(), draws=dict(vq.last_upkeep),
                               initted=bool(cb.initted.item()), **{k: getattr(cb, k)[0].cpu().clone() for k in BUFFERS}))
    torch.save(dict(steps=record, kmeans_ids=kmeans_ids.cpu(), runtime_warnings=[str(w.message) for w in caught if issubclass(w.category, RuntimeWarning)]),
               os.path.join(out_dir, f'vq{rank}.pt'))
    dist.barrier()
    dist.destroy_process_group()


def test_two_ranks_share_one_codebook(tmp_path):
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    ws = 2
    mp.spawn(_sync_rank, args=(ws, _free_port(), str(tmp_path)), nprocs=ws, join=True)
    r = [torch.load(os.path.join(str(tmp_path), f'vq{k}.pt'), weights_only=False) for k in range(ws)]
    assert r[0]['runtime_warnings'] == [] and r[1]['runtime_warnings'] == [], 'synced statistics must not warn'
    assert torch.equal(r[0]['kmeans_ids'], r[1]['kmeans_ids'])
    state = None
    for step in range(2):
        s = [r[k]['steps'][step] for k in range(ws)]
        for name in BUFFERS:
            assert torch.equal(s[0][name], s[1][name]), f'step {step + 1}: the ranks disagree about {name}'
        assert s[0]['draws'] == s[1]['draws'] and s[0]['initted'] and s[1]['initted']
        assert not torch.equal(s[0]['ids'], s[1]['ids']), 'the ranks must have seen different rows'
        rows = [_rows(k, step) for k in range(ws)]
        all_x, all_keep = torch.cat([x for x, _ in rows]), torch.cat([k for _, k in rows])
        all_xn, all_ids = torch.cat([t['xn'] for t in s]), torch.cat([t['ids'] for t in s])
        if step == 0:
            assert s[0]['draws'] == dict(call=0, kmeans_b=R.mix(SEED, 0, R.KMEANS), expire_b=R.mix(SEED, 0, R.EXPIRE))
            init = R.kmeans(all_xn, all_keep, V, ITERS, s[0]['draws']['kmeans_b'], ids=r[0]['kmeans_ids'])
            assert min(float(((m > 1e-5).float().mean())) for m in init['margin']) >= 0.99
            state = {k: init[k] for k in BUFFERS}
        else:
            assert s[0]['draws'] == dict(call=1, kmeans_b=None, expire_b=R.mix(SEED, 1, R.EXPIRE))
        for k in range(ws):                                        # per rank: its own loss and gradient, the shared statistics
            x, keep = rows[k]
            with torch.enable_grad():
                xr = x.clone().requires_grad_()
                ref = R.vq_upkeep_step(xr, state['embed'], state['embed_avg'], state['cluster_size'], keep, s[k]['ids'], threshold=THRESHOLD,
                                       b=s[k]['draws']['expire_b'], xn=all_xn, stat_x=all_x, stat_keep=all_keep, stat_ids=all_ids)
                ref['commit'].backward()
            rel = abs(float(s[k]['commit']) - float(ref['commit'].detach())) / abs(float(ref['commit'].detach()))
            print(f'step {step + 1} rank {k}: commit {float(s[k]["commit"]):.8f} restatement {float(ref["commit"].detach()):.8f} rel {rel:.2e}')
            assert rel <= 1e-6
            close(s[k]['dx'], xr.grad, 1e-5, 'dx')
        for name in BUFFERS:
            err = close(s[0][name], ref[name], 1e-5, f'step {step + 1}: {name}')
            print(f'step {step + 1}: {name} rel err {err:.2e}; expired {int(ref["expired"].sum())}')
        ex = ref['expired']
        assert ex.any() and not ex.all()
        if step == 0:                                              # the chosen rows come from both ranks' halves of the gathered list
            assert (ref['rows'] < M).any() and (ref['rows'] >= M).any()
        assert torch.equal(s[0]['embed'][ex], all_xn[ref['rows']]), 'expired codes take rows of EITHER rank, bit for bit'
        state = {k: ref[k] for k in BUFFERS}
    assert float(r[0]['steps'][0]['commit']) != float(r[1]['steps'][0]['commit'])


def test_sync_off_warns_once_and_stays_local(monkeypatch):
    """sync_codebook=False under a (stubbed) two-rank world: today's one-time RuntimeWarning, and the update from this rank's rows alone --
    no collective is issued (there is no process group to issue it on)"""
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    import phenaki_pytorch_amd as P
    from phenaki_pytorch_amd import train_cvivit as T
    from tests.vq_train_restatement import vq_train_step
    monkeypatch.setattr(dist, 'is_initialized', lambda: True)
    monkeypatch.setattr(dist, 'get_world_size', lambda group=None: 2)
    monkeypatch.setattr(T, '_WARNED_VQ_PER_RANK', False)
    torch.manual_seed(0)
    vq = P.quantize.VectorQuantize(dim=D, codebook_size=V, sync_codebook=False).cuda().train()
    assert vq.sync_world() == 1
    cb = vq._codebook
    start = {k: getattr(cb, k)[0].cpu().clone() for k in BUFFERS}
    x = torch.randn(64, D, generator=torch.Generator().manual_seed(1))
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter('always')
        with torch.no_grad():
            _, ids1, _ = vq(x.cuda()[None])
            _, ids2, _ = vq(x.cuda()[None])
    assert len([w for w in caught if issubclass(w.category, RuntimeWarning) and 'NOT all-reduced' in str(w.message)]) == 1
    ref = vq_train_step(x, start['embed'], start['embed_avg'], start['cluster_size'], None, ids1[0].cpu())
    ref = vq_train_step(x, ref['embed'], ref['embed_avg'], ref['cluster_size'], None, ids2[0].cpu())
    for k in BUFFERS:
        close(getattr(cb, k)[0], ref[k], 1e-5, k)
    monkeypatch.setattr(vq, 'sync_codebook', None)
    assert vq.sync_world() == 2
