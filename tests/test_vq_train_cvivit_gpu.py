"""The tokenizer's training step with the cosine-sim VectorQuantize (CViViT(lookup_free_quantization=False), train_cvivit._VQFn): TINY C-ViViT with
a 4096-entry codebook on a (1, 3, 5, 64, 64) video -- 3 token frames x 16 patches = 48 quantizer rows.  The quantizer's own numbers are held to
tests/vq_train_restatement.py (formulas restated from memory of the published module, upstream parity unpinned)."""
import pytest
import torch

from oracle import weights
from oracle.configs import TINY
from tests.vq_train_restatement import vq_train_step

pytestmark = pytest.mark.gpu

CFG = {**TINY['cvivit'], 'codebook_size': 4096}
BUFFERS = ('cluster_size', 'embed_avg', 'embed')


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    torch.cuda.set_device(0)
    with torch.enable_grad():
        yield


def make(dtype='fp32', gan=False):
    import phenaki_pytorch_amd as P
    torch.manual_seed(3)
    kw = dict(use_vgg_and_gan=True, vgg=weights.stub_vgg(CFG['image_size'])) if gan else dict(use_vgg_and_gan=False)
    cv = P.CViViT(lookup_free_quantization=False, **kw, **CFG).cuda().train()
    P.set_compute_dtype(cv, dtype)
    return cv


def video():
    return weights.synthetic_video(1, 5, 64, 64, seed=0).cuda()


def buffers(cv):
    return {k: getattr(cv.vq._codebook, k)[0].detach().cpu().clone() for k in BUFFERS}


@pytest.fixture
def spy(monkeypatch):
    """records the quantizer call of the step: its input rows, mask, ids, and the gradients that arrive at its output / leave through its input"""
    from phenaki_pytorch_amd import train_cvivit as TC
    rec = {}
    orig = TC._VQFn.apply

    def apply(x, vq, keep=None, want_commit=False):
        rec.update(x=x.detach().cpu(), keep=None if keep is None else keep.detach().bool().cpu(), before=buffers_of(vq))
        out = orig(x, vq, keep, want_commit)
        rec.update(ids=out[-1].cpu(), y=out[0].detach().cpu())
        if x.requires_grad:
            x.register_hook(lambda g: rec.__setitem__('dx', g.detach().cpu()))
            out[0].register_hook(lambda g: rec.__setitem__('dy', g.detach().cpu()))
        return out

    monkeypatch.setattr(TC._VQFn, 'apply', staticmethod(apply))
    return rec


def buffers_of(vq):
    return {k: getattr(vq._codebook, k)[0].detach().cpu().clone() for k in BUFFERS}


@pytest.mark.parametrize('dtype', ['fp32', 'bf16x3'])
def test_training_step_runs_and_reaches_every_parameter(dtype, spy):
    """loss = cv(video); loss.backward() (refused by an assert before VectorQuantize could train): finite non-zero gradients on the encoder and
    decoder side of the quantizer, an updated codebook, unchanged state_dict keys, and the straight-through identity at the quantizer"""
    cv = make(dtype)
    keys = list(cv.state_dict())
    before = buffers(cv)
    loss = cv(video())
    assert loss.requires_grad and loss.ndim == 0 and torch.isfinite(loss)
    loss.backward()
    # (a self-attention block owns a context_norm that no forward reads -- attention.py:134-138 normalises a CONTEXT only -- so it has no gradient in
    # the reference either; every other non-empty parameter is on the path)
    on_path = [(n, p) for n, p in cv.named_parameters() if p.numel() and '.context_norm.' not in n]
    missing = [n for n, p in on_path if p.grad is None or not torch.isfinite(p.grad).all() or not p.grad.abs().max() > 0]
    assert not missing, f'parameters without a finite non-zero gradient: {missing}'
    assert len(on_path) >= 90
    assert any(n.startswith('enc_') for n, _ in cv.named_parameters()) and any(n.startswith('dec_') for n, _ in cv.named_parameters())
    after = buffers(cv)
    assert all(not torch.equal(before[k], after[k]) for k in BUFFERS)
    assert list(cv.state_dict()) == keys
    # reconstruction-only objective: no commitment term, so what leaves the quantizer towards the encoder IS what the decoder handed it
    assert spy['keep'] is None and spy['x'].shape == (48, 128)
    assert torch.equal(spy['dx'], spy['dy']) and spy['dy'].abs().max() > 0
    assert torch.equal(spy['y'], before['embed'][spy['ids']])
    ref = vq_train_step(spy['x'], before['embed'], before['embed_avg'], before['cluster_size'], None, spy['ids'])
    for k in BUFFERS:
        assert (after[k] - ref[k]).abs().max() <= 1e-5 * ref[k].abs().max(), k


def test_frame_mask_selects_the_rows_of_the_statistics(spy):
    """mask [[1, 1, 1, 0, 0]]: token frames 0 and 1 kept, 2 dropped; the quantizer rows are '(b h w) t'"""
    cv = make()
    mask = torch.tensor([[True, True, True, False, False]]).cuda()
    cv(video(), mask=mask).backward()
    keep = (torch.arange(48) % 3) < 2
    assert torch.equal(spy['keep'], keep)
    bins = torch.bincount(spy['ids'][keep], minlength=4096).float()
    cs = buffers(cv)['cluster_size']                              # a fresh module starts from cluster_size = 0: after one step it is 0.2 bins
    assert (cs - 0.2 * bins).abs().max() <= 1e-6 and abs(float(cs.sum()) - 0.2 * 32) <= 1e-5


def test_three_optimiser_steps_reduce_the_reconstruction_loss():
    import phenaki_pytorch_amd as P
    cv = make()
    v = video()
    opt = P.get_optimizer(cv.parameters(), lr=3e-4, wd=0.)
    losses = []
    for _ in range(3):
        opt.zero_grad(set_to_none=True)
        loss = cv(v)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print('losses', losses)
    assert losses[0] > losses[1] > losses[2], losses


def test_eval_mode_quantizer_inside_a_training_step():
    """vq.eval() in a grad-mode step follows the LFQ branch: hard codes, no gradient to the encoder, no codebook update"""
    cv = make()
    cv.vq.eval()
    before = buffers(cv)
    cv(video()).backward()
    after = buffers(cv)
    assert all(torch.equal(before[k], after[k]) for k in BUFFERS)
    named = dict(cv.named_parameters())
    assert all(p.grad is None for n, p in named.items() if n.startswith('enc_') or n.startswith('to_patch_emb'))
    assert all(p.grad is not None and p.grad.abs().max() > 0 for n, p in named.items() if n.startswith('to_pixels'))


def test_gan_objectives_add_the_commitment_loss_and_update_the_codebook(spy):
    """generator objective: _pk_loss_parts['vq_aux'] is the restatement's commitment loss and the total is the sum of its recorded parts
    (cvivit.py:666); the discriminator objective detaches the reconstruction but still updates the codebook (cvivit.py:570 runs before :605)"""
    cv = make(gan=True)
    parts = cv.__dict__['_pk_loss_parts'] = {}
    torch.manual_seed(22)
    loss = cv(video())
    loss.backward()
    ref = vq_train_step(spy['x'], spy['before']['embed'], spy['before']['embed_avg'], spy['before']['cluster_size'], None, spy['ids'])
    aux = float(parts['vq_aux'])
    print('vq_aux', aux, 'restatement', float(ref['commit']))
    assert abs(aux - float(ref['commit'])) <= 1e-6 * float(ref['commit'])
    total = parts['recon_loss'] + parts['perceptual'] + parts['adaptive_weight'] * parts['gen_loss'] + parts['vq_aux']
    assert abs(float(loss.detach()) - float(total)) <= 1e-6 * abs(float(total))
    # the commitment term reaches the encoder: d x = d y + 2 (x - q) / (M D)
    want = spy['dy'] + 2. * (spy['x'] - spy['y']) / spy['x'].numel()
    assert (spy['dx'] - want).abs().max() <= 1e-5 * want.abs().max()
    before = buffers(cv)
    dloss = cv(video(), return_discr_loss=True)
    dloss.backward()
    after = buffers(cv)
    assert all(not torch.equal(before[k], after[k]) for k in BUFFERS)
    assert spy['x'].shape == (48, 128) and torch.equal(spy['y'], before['embed'][spy['ids']])
