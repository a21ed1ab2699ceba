"""Lookup-free quantizer with the module surface the reference expects from `vector_quantize_pytorch.LFQ`
(call sites /root/reference/phenaki_pytorch/cvivit.py:319, :570, :439; the package itself is not vendored --
behaviour restated from its published semantics, see oracle/lfq.py and SURVEY.md 8c).

state_dict keys: project_in.{weight (cd, dim), bias}, project_out.{weight (dim, cd), bias}, buffer `mask`.
Always exact f32: the ids are 16 sign bits, so this projection never runs in bf16.
"""
import math

import torch
from torch import nn

from . import _lib as L


class LFQ(nn.Module):
    def __init__(self, *, dim, codebook_size, codebook_scale=1.0, entropy_loss_weight=0.1, commitment_loss_weight=0.25, diversity_gamma=1.,
                 **_unused):
        """the keyword arguments are the published module's (they arrive through CViViT(lookup_free_quantization_kwargs=...), cvivit.py:319)"""
        super().__init__()
        self.entropy_loss_weight, self.commitment_loss_weight, self.diversity_gamma = entropy_loss_weight, commitment_loss_weight, diversity_gamma
        cd = int(math.log2(codebook_size))
        assert 2 ** cd == codebook_size, 'codebook size must be a power of two'
        assert dim != cd, 'the MI355X build expects dim != log2(codebook_size) (projections present)'
        assert codebook_scale == 1.0, 'only codebook_scale = 1 is built'
        self.dim, self.codebook_dim, self.codebook_size = dim, cd, codebook_size
        self.codebook_scale = codebook_scale
        self.project_in = nn.Linear(dim, cd)
        self.project_out = nn.Linear(cd, dim)
        self.register_buffer('mask', 2 ** torch.arange(cd - 1, -1, -1))

    def encode_ids(self, x2d, return_proj=False):
        """x2d (M, dim) f32 -> ids (M,) int64 [, proj (M, cd) f32]"""
        L.require_device(x2d, 'tokens')
        M, D = x2d.shape
        ids = torch.empty((M,), device=x2d.device, dtype=torch.int64)
        proj = torch.empty((M, self.codebook_dim), device=x2d.device, dtype=torch.float32) if return_proj else None
        L.lfq_encode(x2d, self.project_in.weight, self.project_in.bias, ids, proj, M, D, self.codebook_dim)
        return (ids, proj) if return_proj else ids

    def encode_ids_from_prenorm(self, x2d, norm, perm=(0, 0), return_proj=False):
        """ids of LayerNorm(x2d) with the (gamma, beta) of `norm` (the encoder's norm_out), rows permuted like pk_layernorm's
        (pb, pc): ONE fused launch, the normalised tokens never reach HBM (cvivit.py:472 + :570).  Needs cd <= 16."""
        L.require_device(x2d, 'tokens')
        M, D = x2d.shape
        ids = torch.empty((M,), device=x2d.device, dtype=torch.int64)
        proj = torch.empty((M, self.codebook_dim), device=x2d.device, dtype=torch.float32) if return_proj else None
        L.layernorm_lfq(x2d, norm.gamma, norm.beta, self.project_in.weight, self.project_in.bias, ids, M, D, self.codebook_dim,
                        proj=proj, perm=perm)
        return (ids, proj) if return_proj else ids

    def codes_2d(self, ids_flat, *, ids_prime=None, perm=(0, 0)):
        """ids (M,) int64 -> project_out(+-1 codes) (M, dim) f32.  ids_prime (nb, n_prime): primed tokens in front of every sequence of
        `ids_flat` given as (nb, n); perm = (pb, pc): output rows (a, b, c) -> (a, c, b) (see pk_lfq_decode)"""
        L.require_device(ids_flat, 'indices')
        M = ids_flat.numel() + (ids_prime.numel() if ids_prime is not None else 0)
        out = torch.empty((M, self.dim), device=ids_flat.device, dtype=torch.float32)
        ids = ids_flat if ids_flat.is_contiguous() else ids_flat.contiguous()
        L.lfq_decode(ids, self.project_out.weight, self.project_out.bias, out, M, self.dim, self.codebook_dim, ids_prime=ids_prime, perm=perm)
        return out

    def indices_to_codes(self, indices, project_out=True):
        assert project_out, 'raw +-1 codes are not exposed by the MI355X build'
        is_img_or_video = indices.ndim >= 3
        codes = self.codes_2d(indices.reshape(-1).long()).reshape(*indices.shape, self.dim)
        if is_img_or_video:
            codes = codes.movedim(-1, 1)
        return codes

    def aux_config(self, inv_temperature=100.):
        """keyword arguments of _lib.lfq_aux for this module (published forward default inv_temperature = 100)"""
        if not 2 <= self.codebook_dim <= 16:
            # the pk_lfq_aux_* kernels factorise the 2^cd codebook distribution over two halves of <= 8 bits each (256-entry LDS tables)
            raise ValueError(f'the LFQ training-mode auxiliary loss (entropy + commitment, pk_lfq_aux_*) is built for codebook sizes 4 .. 65536; '
                             f'codebook_size = {self.codebook_size} (codebook_dim {self.codebook_dim}) can be run for inference and for the '
                             'reconstruction-only objective (use_vgg_and_gan=False) only')
        return dict(inv_temperature=inv_temperature, codebook_scale=self.codebook_scale, entropy_loss_weight=self.entropy_loss_weight,
                    commitment_loss_weight=self.commitment_loss_weight, diversity_gamma=self.diversity_gamma)

    def forward(self, x, inv_temperature=100., **_unused):
        """(b, n, dim) -> (quantized (b, n, dim), indices (b, n) int64, aux_loss).  The published module's predicate is `self.training` alone
        (the same predicate as the tokenizer's training step, train_cvivit.py): eval mode -> the hard codes, NO straight-through
        gradient into project_in, aux = 0; training mode -> the straight-through output and the entropy + commitment auxiliary loss
        (differentiable under grad mode through train_cvivit._LFQFn / pk_lfq_aux_*; under no_grad the same VALUES without a graph)."""
        b, n, d = x.shape
        x2 = x.reshape(b * n, d).float().contiguous()
        if self.training:
            from .train_cvivit import _LFQFn
            q, aux, _ = _LFQFn.apply(x2, self.project_in.weight, self.project_in.bias, self.project_out.weight, self.project_out.bias,
                                     self.aux_config(inv_temperature))
            with torch.no_grad():
                ids = self.encode_ids(x2.detach())
            return q.reshape(b, n, d), ids.reshape(b, n), aux
        ids = self.encode_ids(x2)
        if torch.is_grad_enabled() and any(p.requires_grad for p in self.project_out.parameters()):
            from .train_cvivit import _LFQFn
            q = _LFQFn.apply(x2, self.project_in.weight, self.project_in.bias, self.project_out.weight, self.project_out.bias, None, False)
        else:
            q = self.codes_2d(ids)
        return q.reshape(b, n, d), ids.reshape(b, n), torch.zeros((), device=x.device)


PICK_P = 2 ** 31 - 1                     # prime: j -> (b + j P) mod n is a bijection of [0, n) for every n < P
UPKEEP_EXPIRE, UPKEEP_KMEANS = 1, 2      # the `purpose` word of upkeep_mix
_M64 = (1 << 64) - 1


def pick(b, j, n):
    """position of the j-th chosen row among n kept rows (the kernels' vq_pick_row: the same 64-bit integer arithmetic): distinct while
    j < n (the published randperm branch), wrapping evenly beyond (its randint branch)"""
    return ((b % n) + j * PICK_P) % n


def _splitmix64(z):
    z = (z + 0x9E3779B97F4A7C15) & _M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & _M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & _M64
    return z ^ (z >> 31)


def upkeep_mix(seed, call, purpose):
    """the host integer b of one upkeep draw: three chained splitmix64 finalisers over (upkeep_seed, call index, purpose), top 62 bits.  Ranks
    running the same script draw the same b without talking to each other."""
    z = _splitmix64(int(seed) & _M64)
    z = _splitmix64(z ^ (int(call) & _M64))
    z = _splitmix64(z ^ (int(purpose) & _M64))
    return z >> 2


class _CosineSimCodebook(nn.Module):
    """holder mirroring the library's `_codebook` sub-module: `embed` is (1, codebook_size, dim), unit-norm rows -- or, with kmeans_init, zeros
    and initted = False until the first training-mode call has run k-means on its rows (as published)."""

    def __init__(self, dim, codebook_size, kmeans_init=False):
        super().__init__()
        if kmeans_init:
            embed = torch.zeros(1, codebook_size, dim)
        else:
            embed = torch.nn.functional.normalize(torch.randn(1, codebook_size, dim), dim=-1)
        self.register_buffer('initted', torch.tensor([not kmeans_init]))
        self.register_buffer('cluster_size', torch.zeros(1, codebook_size))
        self.register_buffer('embed_avg', embed.clone())
        self.register_buffer('embed', embed)


class VectorQuantize(nn.Module):
    """`vector_quantize_pytorch.VectorQuantize(dim, codebook_size, use_cosine_sim=True)`
    (reference call sites cvivit.py:321 construct, :568-570 forward with `mask=`, :441 `.codebook[indices]`; the
    package is not vendored -- published behaviour: l2-normalise the input, argmax of its dot product with the
    unit-norm codebook, gather; the eval half restated in oracle/lfq.py, the training half in DESIGN.md
    "VectorQuantize training").  The lookup is the vocab-head kernel in its no-noise mode
    (one fused GEMM + argmax, the (M, 65536) similarity matrix is never written) and always runs in exact f32: ids are
    an argmax over 65 536 cosine similarities.

    Training mode (`self.training`, the predicate of LFQ.forward): the straight-through output, the commitment loss
    commitment_weight * mean (q - x)^2 and the EMA update (decay, eps) of the `_codebook` buffers cluster_size /
    embed_avg / embed from the rows `mask` keeps -- train_cvivit._VQFn on the pk_vq_* kernels.  One head, no
    projections.

    Upkeep (DESIGN.md "VectorQuantize upkeep"; every keyword is an attribute and may be set after construction, the defaults are off):
      threshold_ema_dead_code = T > 0: after the EMA update a code whose cluster_size fell below T is replaced by a kept row of the batch
        (cluster_size := reset_cluster_size, None = T), inside the update's own launches;
      kmeans_init: the codebook starts at zeros with initted = False, and the first training-mode call runs kmeans_iters rounds of spherical
        k-means on its kept rows before the ordinary step;
      sync_codebook: None = when a process group of more than one rank is initialised, the statistics are computed from every rank's rows
        (xn, ids and keep are all-gathered in rank order and each rank runs the same deterministic kernels: bit-identical buffers, no
        broadcast); every rank must pass the same number of rows.  False = per rank (warns once), True without a process group = ValueError.
      The rows upkeep draws are pick(b, j, n) with b = upkeep_mix(upkeep_seed, call index, purpose); `last_upkeep` records the b of the
      latest training-mode call.  The call index is a plain counter (not in the state_dict)."""

    def __init__(self, *, dim, codebook_size, use_cosine_sim=True, decay=0.8, eps=1e-5, commitment_weight=1.0, kmeans_init=False, kmeans_iters=10,
                 threshold_ema_dead_code=0, reset_cluster_size=None, sync_codebook=None, upkeep_seed=0, **_unused):
        super().__init__()
        assert use_cosine_sim, 'only the cosine-sim codebook (the reference construction, cvivit.py:321) is built'
        assert dim % 32 == 0 and codebook_size % 4 == 0
        assert 0. <= decay <= 1. and eps > 0.
        self.dim, self.codebook_size = dim, codebook_size
        self.decay, self.eps, self.commitment_weight = float(decay), float(eps), float(commitment_weight)
        self.kmeans_init, self.kmeans_iters = bool(kmeans_init), int(kmeans_iters)
        self.threshold_ema_dead_code, self.reset_cluster_size = threshold_ema_dead_code, reset_cluster_size
        self.sync_codebook, self.upkeep_seed = sync_codebook, int(upkeep_seed)
        self.upkeep_calls = 0
        self.last_upkeep = None
        self._initted_host = None                                   # the host's copy of `initted`, read from the buffer once
        self._codebook = _CosineSimCodebook(dim, codebook_size, self.kmeans_init)
        self.register_load_state_dict_post_hook(lambda module, _keys: setattr(module, '_initted_host', None))

    def sync_world(self):
        """the number of ranks whose rows enter the codebook statistics (1: this rank's alone)"""
        import torch.distributed as dist
        up = dist.is_available() and dist.is_initialized()
        if self.sync_codebook is None:
            return dist.get_world_size() if up else 1
        if not self.sync_codebook:
            return 1
        if not up:
            raise ValueError('VectorQuantize(sync_codebook=True) needs an initialised process group')
        return dist.get_world_size()

    def needs_kmeans(self):
        """True until the codebook is initialised (kmeans_init only).  `initted` is read from the device once and remembered on the host."""
        if not self.kmeans_init:
            return False
        if self._initted_host is None:
            self._initted_host = bool(self._codebook.initted.item())
        return not self._initted_host

    def begin_upkeep(self):
        """the draws of one training-mode call: dict(call, kmeans_b, expire_b) (None where that upkeep does not run); advances the call index"""
        threshold = float(self.threshold_ema_dead_code)
        if not threshold >= 0. or (self.kmeans_init and self.kmeans_iters < 1):
            raise ValueError('VectorQuantize: threshold_ema_dead_code must be >= 0 and kmeans_iters >= 1')
        call = self.upkeep_calls
        self.upkeep_calls += 1
        self.last_upkeep = dict(call=call,
                                kmeans_b=upkeep_mix(self.upkeep_seed, call, UPKEEP_KMEANS) if self.needs_kmeans() else None,
                                expire_b=upkeep_mix(self.upkeep_seed, call, UPKEEP_EXPIRE) if threshold > 0. else None)
        return self.last_upkeep

    def kmeans_done(self):
        self._codebook.initted.fill_(True)
        self._initted_host = True

    @property
    def codebook(self):
        return self._codebook.embed[0]

    def normalised(self, x2d):
        """x2d (M, dim) f32 -> its rows at unit l2 norm (the query side of the lookup, and what the EMA update averages)"""
        L.require_device(x2d, 'tokens')
        M, D = x2d.shape
        xn = torch.empty_like(x2d)
        L.l2norm_rows(x2d, xn, M, D)
        return xn

    def ids_of_normalised(self, xn, codebook=None):
        """the cosine argmax of unit-norm rows against the codebook (or another (V, dim) set of unit-norm rows: the k-means means)"""
        M, D = xn.shape
        V = self.codebook_size
        cb = (self.codebook if codebook is None else codebook).contiguous()
        zero_bias = torch.zeros((V,), device=xn.device, dtype=torch.float32)
        partials = torch.empty((5 * L.vocab_ntiles(V) * M,), device=xn.device, dtype=torch.float32)
        L.vocab_sample(L.F32, xn, cb, zero_bias, M, V, D, 1.0, None, None, 0, False, partials, no_noise=True)
        ids = torch.empty((M,), device=xn.device, dtype=torch.int64)
        L.vocab_reduce(partials, M, V, None, None, None, ids, None, False)
        return ids

    def encode_ids(self, x2d, return_proj=False):
        assert not return_proj, 'the margin audit projection exists for LFQ only'
        return self.ids_of_normalised(self.normalised(x2d))

    def codes_2d(self, ids_flat, *, ids_prime=None, perm=(0, 0)):
        if ids_prime is not None:
            ids_flat = torch.cat((ids_prime, ids_flat), dim=-1)
        codes = self.codebook.index_select(0, ids_flat.reshape(-1).long())
        if perm[0]:
            pb, pc = perm
            codes = codes.view(-1, pb, pc, codes.shape[-1]).transpose(1, 2).reshape(-1, codes.shape[-1])
        return codes

    def forward(self, x, mask=None, **_unused):
        """(b, n, dim) -> (quantized (b, n, dim), indices (b, n) int64, commitment loss).  mask (b, n) bool: the rows that enter the commitment
        loss and the codebook statistics (every row gets an id and a code).  eval mode: the hard codes, no gradient, no update, loss 0; training
        mode: straight-through gradient, the commitment loss and the in-place EMA update -- under no_grad the same values and the same update
        without a graph."""
        b, n, d = x.shape
        x2 = x.reshape(b * n, d).float().contiguous()
        if self.training:
            from .train_cvivit import _VQFn
            q, commit, ids = _VQFn.apply(x2, self, None if mask is None else mask.reshape(b * n), True)
            return q.reshape(b, n, d), ids.reshape(b, n), commit
        ids = self.encode_ids(x2)
        q = self.codes_2d(ids)
        return q.reshape(b, n, d), ids.reshape(b, n), torch.zeros((), device=x.device)
