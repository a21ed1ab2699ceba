"""ctypes binding of libphenaki_hip.so (include/phenaki_hip.h).

The product has NO CPU fallback: importing this module is harmless, but the first kernel call without the
built library (python -m phenaki_pytorch_amd.build) or without a HIP device raises.
PyTorch is used only as the owner of device memory and of the current HIP stream.
"""
import ctypes
import os

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
# PK_LIB_PATH: load another build of the same C ABI (A/B timing of two builds on one GPU box; never a fallback)
LIB_PATH = os.environ.get('PK_LIB_PATH') or os.path.join(_HERE, 'libphenaki_hip.so')

_P = ctypes.c_void_p
_I = ctypes.c_int
_F = ctypes.c_float
_L = ctypes.c_long
_LL = ctypes.c_longlong
_ULL = ctypes.c_ulonglong

# name -> argtypes, kept in the order of include/phenaki_hip.h (tests check every symbol is exported)
SIGNATURES = {
    'pk_gemm': [_I, _I, _P, _I, _P, _I, _I, _I, _I, _P, _P, _I, _P, _I, _I, _I, _P, _P],
    'pk_gemm_ex': [_I, _I, _P, _I, _P, _I, _I, _I, _I, _P, _P, _I, _P, _I, _I, _I, _P, _I, _I, _P, _I, _P, _P, _F, _P, _P, _P, _P, _I, _P],
    'pk_gemm_auto_variant': [_I, _I, _I, _I, _I, _I, _I, _I],
    'pk_layernorm': [_P, _I, _P, _P, _F, _P, _I, _I, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    'pk_rmsnorm': [_P, _I, _P, _F, _P, _P, _I, _I, _I, _I, _P],
    'pk_gated_gelu_tanh': [_P, _I, _P, _I, _I, _I, _I, _P],
    'pk_l2norm_rows': [_P, _I, _P, _I, _I, _I, _I, _P],
    'pk_patchify_ln': [_P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P, _F, _P, _I, _I, _P],
    'pk_patch_embed': [_P, _I, _I, _I, _I, _I, _I, _I, _I, _F, _I,
                       _P, _I, _P, _P, _P, _I, _I, _I,
                       _P, _I, _P, _P, _P, _I, _I, _I, _I, _P],
    'pk_patch_embed_slices': [_I],
    'pk_patch_embed_splitk': [_P, _I, _I, _I, _I, _I, _I, _I, _I, _I,
                              _P, _I, _P, _P, _I, _I, _I,
                              _P, _I, _P, _P, _I, _I, _I, _P],
    'pk_patch_embed_finish': [_P, _P, _I, _I, _I, _I, _P, _P, _F, _P, _P, _F, _P, _I, _P, _I, _I, _I, _I, _P],
    'pk_patch_embed_finish_groups': [_P, _I, _I, _P, _I, _P, _I, _P],
    'pk_patch_frame_mask': [_P, _LL, _P, _LL, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    'pk_unpatchify': [_P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _I, _I, _I, _P],
    'pk_sqdiff_partials': [_P, _P, _P, _I, _I, _I, _I, _I, _P, _P],
    'pk_peg': [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    'pk_lfq_encode': [_P, _I, _P, _P, _P, _P, _I, _I, _I, _P],
    'pk_lfq_decode': [_P, _P, _P, _P, _I, _I, _I, _P, _I, _I, _I, _I, _P],
    'pk_lfq_aux_parts': [_I],
    'pk_lfq_aux_prep': [_P, _I, _I, _F, _F, _P, _P, _P, _P, _P],
    'pk_lfq_aux_codebook': [_P, _I, _F, _F, _P, _P, _P],
    'pk_lfq_aux_grad': [_P, _P, _P, _I, _I, _F, _F, _F, _F, _P, _P],
    'pk_lfq_aux_finish': [_P, _P, _I, _P, _I, _F, _F, _F, _P, _P],
    'pk_vq_hist': [_P, _P, _I, _I, _P, _I, _P],
    'pk_vq_scan': [_P, _I, _F, _P, _P, _P, _P, _P],
    'pk_vq_fill': [_P, _P, _I, _I, _P, _P, _P],
    'pk_vq_codebook_update': [_P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _F, _P, _P, _P],
    'pk_vq_gather_commit': [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P],
    'pk_vq_commit_bwd': [_P, _P, _P, _P, _I, _I, _F, _P, _P, _P],
    'pk_vq_compact_keep': [_P, _I, _P, _P, _P],
    'pk_vq_scan_expire': [_P, _I, _F, _F, _P, _P, _P, _P, _P, _P],
    'pk_vq_codebook_update_expire': [_P, _P, _P, _P, _P, _P, _P, _P, _P, _I, _I, _I, _F, _F, _F, _LL, _P, _P, _P],
    'pk_vq_pick_rows': [_P, _P, _P, _I, _I, _I, _LL, _P, _P],
    'pk_vq_kmeans_means': [_P, _P, _P, _P, _I, _I, _I, _P, _P, _P, _P],
    'pk_layernorm_lfq': [_P, _I, _P, _P, _F, _P, _P, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P],
    'pk_embed': [_P, _I, _P, _I, _I, _P, _P, _P, _P, _I, _I, _P],
    'pk_cpb_input': [_P, _P, _P, _I, _I, _I, _I, _I, _P],
    'pk_attn_pads': [_I, _I, _I, ctypes.POINTER(_I), ctypes.POINTER(_I)],
    'pk_attn_prep': [_I, _P, _I, _P, _I, _P, _P, _P, _F, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    'pk_attn_prep_dh': [_I, _I, _P, _I, _P, _I, _P, _P, _P, _F, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    'pk_qkv_project': [_I, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _P, _P, _F, _P, _P, _P, _I, _I, _P, _P],
    'pk_qkv_attn': [_I, _P, _P, _I, _P, _P, _I, _I, _I, _I, _I, _P, _P, _F, _P, _L, _I, _P, _I, _P, _I, _P, _P],
    'pk_q_attn_cached': [_I, _P, _I, _P, _I, _I, _I, _I, _I, _P, _F, _P, _P, _P, _I, _I, _I, _P, _P, _I, _P],
    'pk_attn_fwd': [_I, _P, _P, _P, _P, _L, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P, _I, _I, _F, _P],
    'pk_attn_fwd_dh': [_I, _I, _P, _P, _P, _P, _L, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P, _I, _P, _I, _I, _F, _P],
    'pk_attn_fwd_lse': [_I, _P, _P, _P, _P, _L, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P],
    'pk_attn_fwd_lse_dh': [_I, _I, _P, _P, _P, _P, _L, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _I, _I, _P, _P, _P],
    'pk_attn_small': [_P, _I, _P, _I, _P, _P, _F, _P, _L, _I, _P, _P, _I, _P, _I, _I, _I, _I, _I, _P],
    'pk_cfg_mix': [_P, _I, _I, _I, _I, _P, _I, _F, _I, _P, _I, _I, _I, _P],
    'pk_guidance_mix': [_P, _I, _I, _I, _I, _P, _I, _P, _I, _I, _P, _I, _I, _I, _P],
    'pk_vocab_ntiles': [_I],
    'pk_vocab_sample_philox': [_I, _P, _I, _P, _I, _P, _I, _I, _I, _F, _P, _ULL, _ULL, ctypes.c_uint, _I, _P, _P],
    'pk_vocab_sample': [_I, _P, _I, _P, _I, _P, _I, _I, _I, _F, _P, _P, _ULL, _P, _I, _P, _P],
    'pk_vocab_reduce': [_P, _I, _I, _P, _P, _P, _P, _P, _I, _P],
    'pk_logits_topk_sample': [_P, _LL, _I, _I, _I, _F, _P, _P, _I, _ULL, _P, _I, _P, _P, _P, _P, _P, _P, _P],
    'pk_logits_nucleus_sample': [_P, _LL, _I, _I, _I, _F, _F, _F, _P, _P, _I, _ULL, _P, _I, _P, _P, _P, _P, _P, _P, _P],
    'pk_vocab_ce': [_I, _P, _I, _I, _P, _I, _P, _I, _P, _I, _P, _P, _P, _P, _P],
    'pk_vocab_ce_reg': [_I, _P, _I, _I, _P, _I, _P, _I, _P, _I, _P, _P, _P, _P, _F, _F, _P, _P, _P],
    'pk_vocab_weight_mean_words': [_I, _I, _I],
    'pk_vocab_weight_mean': [_I, _P, _I, _P, _I, _I, _P, _P, _P, _P],
    'pk_vocab_eval_words': [_I],
    'pk_vocab_eval': [_I, _P, _I, _P, _I, _P, _I, _I, _I, _P, _P, _P, _P],
    'pk_vocab_eval_reduce': [_P, _I, _I, _P, _P, _P, _P, _P, _P],
    'pk_ce_grad_slab': [_I, _P, _I, _P, _P, _P, _I, _I, _I, _F, _P, _P, _I, _P, _I, _P, _P],
    'pk_ce_grad_slab_reg': [_I, _P, _I, _P, _P, _P, _I, _I, _I, _F, _P, _P, _I, _P, _I, _P, _F, _F, _I, _P],
    'pk_topk_mask': [_P, _I, _I, _I, _LL, _P, _P, _P, _P, _P],
    'pk_topk_mask_keep': [_P, _I, _I, _P, _P, _P, _LL, _P, _P, _P, _P, _P],
    'pk_composite_mask': [_P, _P, _P, _P, _I, _I, _LL, _I, _P],
    'pk_critic_head': [_P, _I, _P, _P, _I, _I, _I, _I, _I, _F, _P, _F, _ULL, _P, _P, _P],
    'pk_critic_head_guided': [_P, _I, _P, _P, _I, _I, _I, _I, _P, _I, _I, _P, _F, _ULL, _P, _P, _P],
    'pk_pack': [_P, _LL, _P, _I, _I, _I, _P, _LL, _I, _I, _P],
    'pk_scatter_rows': [_P, _LL, _P, _P, _LL, _I, _I, _P],
    'pk_colsum_parts': [_I],
    'pk_colsum': [_P, _LL, _I, _I, _F, _P, _I, _P, _P],
    'pk_ln_bwd_parts': [_I],
    'pk_layernorm_bwd': [_P, _LL, _P, _P, _LL, _P, _LL, _P, _LL, _P, _P, _F, _I, _I, _P],
    'pk_geglu': [_P, _LL, _I, _P, _LL, _I, _I, _P, _P],
    'pk_geglu_bwd': [_P, _LL, _I, _P, _LL, _P, _LL, _I, _I, _P, _P],
    'pk_dropout_mask': [_ULL, _ULL, _I, _LL, _I, _P, _P],
    'pk_leaky_bwd': [_P, _LL, _P, _LL, _P, _LL, _I, _I, _F, _P],
    'pk_scaled_diff': [_P, _P, _F, _P, _P, _LL, _P],
    'pk_sign': [_P, _F, _P, _LL, _P],
    'pk_mul': [_P, _P, _P, _LL, _P],
    'pk_peg_wgrad_parts': [_LL],
    'pk_peg_bwd': [_P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    'pk_embed_bwd': [_P, _P, _F, _P, _P, _I, _I, _I, _P],
    'pk_bias_gather': [_P, _I, _P, _I, _P, _I, _I, _P],
    'pk_bias_scatter': [_P, _P, _I, _P, _I, _I, _I, _P],
    'pk_sum_batch': [_P, _LL, _I, _P, _LL, _P],
    'pk_sum_batch_multi': [_P, _I, _P],
    'pk_peg_adjoint': [_P, _P, _P, _I, _I, _I, _I, _I, _I, _P],
    'pk_colsum_multi': [_P, _I, _P],
    'pk_reduce_multi': [_P, _I, _P, _I, _P],
    'pk_pack_multi': [_P, _I, _P],
    'pk_pack_table_prepare': [_P, _I],
    'pk_pack_table': [_P, _I, _I, _P],
    'pk_bce_head': [_P, _LL, _P, _P, _P, _F, _P, _P, _P, _P, _LL, _P, _P, _I, _I, _P],
    'pk_attn_train_prep': [_P, _LL, _P, _LL, _P, _P, _P, _F, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    'pk_attn_train_prep_bwd': [_P, _LL, _P, _LL, _P, _P, _P, _F, _P, _P, _P, _P, _LL, _P, _LL, _P, _P, _P, _I, _I, _I, _I, _I, _P],
    'pk_gemm_splitk': [_I, _P, _I, _P, _I, _I, _I, _I, _I, _P, _I, _P, _I, _P],
    'pk_adamw': [_P, _P, _P, _P, _F, _F, _F, _F, _F, _I, _LL, _P],
    'pk_adamw_multi': [_P, _I, _F, _F, _F, _F, _F, _I, _P],
    'pk_grad_sumsq_parts': [_P, _I],
    'pk_grad_sumsq': [_P, _I, _P, _LL, _P],
    'pk_grad_clip_coef': [_P, _LL, _F, _P, _P],
    'pk_scale_multi': [_P, _I, _P, _P],
    'pk_adamw_multi_scaled': [_P, _I, _F, _F, _F, _F, _F, _I, _P, _P],
    'pk_ema_multi': [_P, _I, _F, _P],
    'pk_attn_bwd_ws': [_P, _P, _P, _P, _LL, _I, _P, _LL, _P, _P, _P, _I, _P, _P, _P, _P, _P, _P, _I, _I, _I, _I, _I, _I, _P, _LL, _P, _P],
    'pk_attn_bwd_work': [_I, _I, _I, _I, _I],
    'pk_im2col': [_P, _I, _I, _I, _I, _I, _I, _I, _I, _P, _LL, _P],
    'pk_col2im': [_P, _LL, _I, _I, _I, _I, _I, _I, _I, _I, _P, _P],
    'pk_nchw_to_rows': [_P, _I, _I, _I, _I, _I, _P, _P],
    'pk_rows_to_nchw': [_P, _I, _I, _I, _I, _I, _P, _P],
    'pk_pick_frames': [_P, _P, _I, _I, _I, _I, _I, _P, _I, _P],
    'pk_bmm': [_P, _LL, _LL, _I, _P, _LL, _LL, _I, _P, _LL, _LL, _I, _I, _I, _I, _I, _P],
    'pk_row_softmax': [_P, _P, _P, _P, _LL, _I, _I, _P],
    'pk_row_l2scale': [_P, _P, _P, _P, _P, _P, _P, _P, _LL, _I, _I, _P],
    'pk_row_ln_bwd2': [_P, _P, _P, _P, _P, _F, _P, _P, _P, _LL, _I, _P],
    'pk_conv3x3': [_I, _I, _P, _I, _I, _I, _I, _P, _I, _I, _P, _I, _P, _I, _I, _P, _I, _I, _I, _P],
    'pk_maxpool2x2': [_I, _P, _I, _I, _I, _I, _P, _P],
    'pk_maxpool2x2_bwd': [_I, _P, _P, _I, _I, _I, _I, _P, _P],
    'pk_adaptive_avgpool': [_I, _P, _I, _I, _I, _I, _P, _P],
    'pk_adaptive_avgpool_bwd': [_P, _I, _I, _I, _I, _P, _P],
    'pk_frame_sqerr_parts': [_I, _I],
    'pk_frame_ssim_parts': [_I, _I],
    'pk_frame_sqerr': [_P, _P, _I, _I, _I, _I, _I, _F, _F, _P, _LL, _P, _P, _P],
    'pk_frame_ssim': [_P, _P, _I, _I, _I, _I, _I, _F, _F, _P, _LL, _P, _P],
    'pk_code_usage': [_P, _I, _P, _P],
    'pk_set_cache_policy': [ctypes.c_uint],
    'pk_get_cache_policy': [],
    'pk_gemm_epilogue_form': [_I] * 14,
    'pk_gemm_ex_form': [_I, _I, _P, _I, _P, _I, _I, _I, _I, _P, _P, _I, _P, _I, _I, _I, _P, _I, _I, _P, _I, _P, _P, _F, _P, _P, _P, _P, _I],
    'pk_set_gemm_hot_forms': [_I],
    'pk_get_gemm_hot_forms': [],
    'pk_set_ff1_resident': [_I],
    'pk_get_ff1_resident': [],
    'pk_set_ff1_resident_workers': [_I],
    'pk_get_ff1_resident_launches': [],
    'pk_set_vocab_resident': [_I],
    'pk_get_vocab_resident': [],
    'pk_set_vocab_resident_workers': [_I],
    'pk_get_vocab_resident_launches': [],
}

_ERR = {-1: 'PK_EINVAL (bad shape/size/flag)', -2: 'PK_EALIGN (pointer/stride alignment)', -3: 'PK_ELAUNCH (HIP launch failed)'}

_lib = None
_AB_OPTIONAL = ('pk_set_cache_policy', 'pk_get_cache_policy', 'pk_gemm_epilogue_form', 'pk_gemm_ex_form', 'pk_set_gemm_hot_forms', 'pk_get_gemm_hot_forms',
                'pk_vocab_ce_reg', 'pk_ce_grad_slab_reg', 'pk_vocab_weight_mean', 'pk_vocab_weight_mean_words',
                'pk_set_ff1_resident', 'pk_get_ff1_resident', 'pk_set_ff1_resident_workers', 'pk_get_ff1_resident_launches',
                'pk_set_vocab_resident', 'pk_get_vocab_resident', 'pk_set_vocab_resident_workers', 'pk_get_vocab_resident_launches')


def load():
    """dlopen the library (once).  Raises if it has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(f'{LIB_PATH} is missing: run `python -m phenaki_pytorch_amd.build` '
                               '(the MI355X build has no CPU / eager fallback)')
        lib = ctypes.CDLL(LIB_PATH)
        for name, args in SIGNATURES.items():
            if name in _AB_OPTIONAL and 'PK_LIB_PATH' in os.environ and not hasattr(lib, name):
                continue                                   # an older build loaded for A/B timing: it has no policy switch (set / get then raise)
            fn = getattr(lib, name)
            fn.argtypes = args
            fn.restype = _I
        _lib = lib
    return _lib


def _check(rc, name):
    if rc != 0:
        raise RuntimeError(f'{name} failed: {_ERR.get(rc, rc)}')


def ptr(t):
    return None if t is None else t.data_ptr()


def f32p(t, name='parameter', rows_ok=False):
    """device pointer of an f32 parameter / buffer the kernels read as `const float*`: a module that went through
    .half() / .bfloat16() / .double(), or holds a strided view, must fail here instead of computing garbage."""
    if t is None:
        return None
    if t.dtype != torch.float32 or not (t.is_contiguous() or (rows_ok and t.stride(-1) == 1)):
        raise RuntimeError(f'{name}: the MI355X kernels read this tensor as contiguous float32, got {t.dtype} '
                           f'{"contiguous" if t.is_contiguous() else "strided"} (keep the module in float32; the compute '
                           'precision is chosen with set_compute_dtype, not with .half()/.bfloat16())')
    return t.data_ptr()


def stream(t=None):
    """the HIP stream of the operand's device.  Kernels are launched on the CURRENT device, so an operand living on another
    GPU of the process is refused (torch.cuda.set_device / one process per GPU) instead of being launched on the wrong stream."""
    if t is None:
        return torch.cuda.current_stream().cuda_stream
    idx = t.device.index
    cur = _current_device()
    if idx is not None and idx != cur:
        raise RuntimeError(f'operand on cuda:{idx} but the current device is cuda:{cur}: '
                           'call torch.cuda.set_device(...) first (one process per GPU)')
    # the raw handle straight from the C binding: torch.cuda.current_stream() builds a Stream object per call (5.7 us -- more than
    # a third of the host cost of a launch when the sampling loop is launch-bound at small batches)
    return _raw_stream(cur)


_raw_stream = getattr(torch._C, '_cuda_getCurrentRawStream', None) or (lambda i: torch.cuda.current_stream(i).cuda_stream)
_current_device = getattr(torch._C, '_cuda_getDevice', None) or torch.cuda.current_device


def require_device(t, name='tensor'):
    if not t.is_cuda:
        raise RuntimeError(f'{name} is on {t.device}: the MI355X build runs on HIP devices only (no CPU fallback)')


# compute dtypes of the C ABI: exact f32 MFMA | bf16 operands | split-bf16 ("bf16x3": every GEMM / attention product as
# hi.hi + hi.lo + lo.hi on the bf16 matrix cores, operands x = bf16(x) + bf16(x - bf16(x)); activations stay f32 in memory)
F32, BF16, BF16X3 = 0, 1, 2
ACT_NONE, ACT_GEGLU, ACT_LEAKY, ACT_RELU = 0, 1, 2, 3


def tdtype(dtype):
    """torch dtype of the activations a GEMM of this compute dtype reads / writes as `T`"""
    return torch.bfloat16 if dtype == BF16 else torch.float32


def split_planes(w32):
    """(N, K) f32, K % 32 == 0 -> the pre-split image the bf16x3 kernels read as W (csrc/common.hpp): per row and per block of 32
    k-elements 64 bf16 = [hi x 32 | lo x 32], hi = bf16(w), lo = bf16(w - hi); returned as an (N, K) float32-TYPED tensor of raw bits
    (same bytes per row as f32, so strides / the LDS-DMA ring are those of the f32 layout)."""
    n, k = w32.shape
    assert k % 32 == 0 and w32.dtype == torch.float32
    hi = w32.to(torch.bfloat16)
    lo = (w32 - hi.float()).to(torch.bfloat16)
    img = torch.cat((hi.view(n, k // 32, 32), lo.view(n, k // 32, 32)), dim=-1).contiguous()       # (n, k/32, 64) bf16
    return img.view(n, 2 * k).view(torch.float32)


# ----------------------------------------------------------------------------- wrappers

# cache-policy sites (include/phenaki_hip.h): two bits each, site i at bits 2 i .. 2 i + 1; stores 0 | 1 | 2, loads 0 | 2
CP_PLAIN, CP_WT, CP_NT = 0, 1, 2
CP_STORE_SITES = ('gemm', 'qkv_attn', 'peg', 'ln', 'patch_wide', 'patch_finish')
CP_LOAD_SITES = ('ld_video', 'ld_partials', 'ld_residual')
CP_SITES = CP_STORE_SITES + CP_LOAD_SITES


def cache_policy_mask(**sites):
    """mask of pk_set_cache_policy from site=policy pairs, e.g. cache_policy_mask(peg=CP_WT, ld_video=CP_NT)"""
    mask = 0
    for name, pol in sites.items():
        mask |= int(pol) << (2 * CP_SITES.index(name))
    return mask


def set_cache_policy(mask):
    """cache policy of the launches that follow (a captured graph keeps the one it was captured with)"""
    _check(load().pk_set_cache_policy(int(mask)), 'pk_set_cache_policy')


def get_cache_policy():
    return load().pk_get_cache_policy()


# epilogue forms of pk_gemm_ex (include/phenaki_hip.h)
EPI_GENERIC, EPI_OUT, EPI_FF2A, EPI_FF2B, EPI_FF1 = 0, 1, 2, 3, 4


def set_gemm_hot_forms(on):
    """0: every GEMM launch that follows takes the generic epilogue (a captured graph keeps the form it was captured with)"""
    _check(load().pk_set_gemm_hot_forms(1 if on else 0), 'pk_set_gemm_hot_forms')


def get_gemm_hot_forms():
    return load().pk_get_gemm_hot_forms()


def set_ff1_resident(mode):
    """A-resident form of the FF1 call (csrc/gemm_resident.hpp): 0 the tiled kernel, 1 inside the measured row window, 2 at every M; read at every
    launch (a captured graph keeps the kernel it was captured with)"""
    _check(load().pk_set_ff1_resident(int(mode)), 'pk_set_ff1_resident')


def get_ff1_resident():
    return load().pk_get_ff1_resident()


def set_ff1_resident_workers(n):
    """tests only: n > 0 workers per panel and the resident kernel for every FF1-form call at K = 512; 0: back to the dispatch rule"""
    _check(load().pk_set_ff1_resident_workers(int(n)), 'pk_set_ff1_resident_workers')


def ff1_resident_launches():
    """resident launches of this process so far"""
    return load().pk_get_ff1_resident_launches()


def set_vocab_resident(mode):
    """A-resident form of the vocabulary head (csrc/sampler.hip): 0 the tiled kernel, 1 / 2 force the 8- / 12-wave build (bf16, D = 512, M >= 1024),
    3 the measured rule; read at every launch (a captured graph keeps the kernel it was captured with)"""
    _check(load().pk_set_vocab_resident(int(mode)), 'pk_set_vocab_resident')


def get_vocab_resident():
    return load().pk_get_vocab_resident()


def set_vocab_resident_workers(n):
    """tests only: n > 0 workgroups per XCD in the resident vocabulary head (grid 8 n instead of 256); 0: the default"""
    _check(load().pk_set_vocab_resident_workers(int(n)), 'pk_set_vocab_resident_workers')


def vocab_resident_launches():
    """resident vocabulary-head launches of this process so far"""
    return load().pk_get_vocab_resident_launches()


def gemm_epilogue_form(dtype, variant, *, ln_kind=0, vec_ok=1, act=ACT_NONE, out_is_f32=1, bias=0, res=0, C2=0, stats_out=0, scatter=0,
                       dup_rows=0, pol=0, pol_res=0):
    """pk_gemm_epilogue_form: the form of a launch from its fields (flags: whether the operand is passed)"""
    return load().pk_gemm_epilogue_form(dtype, variant, ln_kind, int(vec_ok), act, int(out_is_f32), int(bool(bias)), int(bool(res)), int(bool(C2)),
                                        int(bool(stats_out)), int(bool(scatter)), int(dup_rows), int(pol), int(pol_res))


def _gemm_args(dtype, A, W, M, N, K, *, C, bias=None, res=None, act=ACT_NONE, a_rows=None, lda=None, ldc=None, variant=0, C2=None, ln=None,
               scatter=None, stats_out=None, ln_stats=None, dup_rows=0):
    """pk_gemm_ex's arguments up to (not including) the stream"""
    a_is_f32 = 1 if A.dtype == torch.float32 else 0
    out_is_f32 = 1 if C.dtype == torch.float32 else 0
    lda = A.stride(-2) if lda is None else lda
    ldc = (C.stride(-2) if scatter is None else N) if ldc is None else ldc
    ldr = res.stride(-2) if res is not None else 0
    return (dtype, a_is_f32, ptr(A), lda, ptr(W), W.stride(0), M, N, K, f32p(bias, 'bias'), f32p(res, 'residual'), ldr,
            ptr(C), ldc, out_is_f32, act, ptr(a_rows), A.shape[0] if a_rows is not None else M, variant,
            ptr(C2), C2.stride(-2) if C2 is not None else 0, ptr(ln[0]) if ln else None, ptr(ln[1]) if ln else None,
            float(ln[2]) if ln else 0., ptr(scatter[0]) if scatter else None, ptr(scatter[1]) if scatter else None,
            ptr(stats_out) if stats_out is not None else None, ptr(ln_stats) if ln_stats is not None else None, int(dup_rows))


def gemm_form(dtype, A, W, M, N, K, **kw):
    """the epilogue form (EPI_*) gemm() would launch for exactly these arguments now; launches nothing, reads no operand (any device)"""
    rc = load().pk_gemm_ex_form(*_gemm_args(dtype, A, W, M, N, K, **kw))
    if rc < 0:
        _check(rc, 'pk_gemm_ex_form')
    return rc


def gemm(dtype, A, W, M, N, K, *, C, bias=None, res=None, act=ACT_NONE, a_rows=None, lda=None, ldc=None, variant=0, C2=None, ln=None,
         scatter=None, stats_out=None, ln_stats=None, dup_rows=0):
    """C = act(A @ W^T + bias) (+ res).  A: (rows, K) f32 or T; W: (N, Kpad) T; C preallocated.
    act = ACT_GEGLU with a residual is refused (PK_EINVAL): the epilogues store the GEGLU pair before the residual add.
    a_rows gathers rows of A (A.shape[0] physical rows bound the DMA descriptor).
    C2: optional bf16 copy of an f32 C.  ln = (s, t, eps): the LayerNorm in front of this Linear folded in (A = the un-normalised
    rows, W = gamma (.) W, s / t its (N,) correction vectors).  scatter = (row_off (M,) int32, col_off (N,) int32): element (m, n) is
    written to C.view(-1)[row_off[m] + col_off[n]] (f32 C of any shape; the un-patchify map).  stats_out (M, ceil(N/32), 2) f32: per-chunk
    (sum, sum of squares) of every output row for the LayerNorm-folded GEMM that consumes it, which passes the same buffer as ln_stats.
    dup_rows: every output row m of C / C2 is also written at row m + dup_rows."""
    rc = load().pk_gemm_ex(*_gemm_args(dtype, A, W, M, N, K, C=C, bias=bias, res=res, act=act, a_rows=a_rows, lda=lda, ldc=ldc, variant=variant, C2=C2,
                                       ln=ln, scatter=scatter, stats_out=stats_out, ln_stats=ln_stats, dup_rows=dup_rows), stream(C))
    _check(rc, 'pk_gemm_ex')
    return C


def layernorm(x, gamma, beta, M, D, *, out=None, out2=None, raw=None, eps=1e-5, remap=(0, 0, 0), perm=(0, 0), ldx=None):
    """out (T) / out2 (f32) <- LN(x); raw (T, same type as out) <- x.  remap / perm: output row maps (see the header)."""
    tt = out if out is not None else raw
    out_kind = 1 if (tt is not None and tt.dtype == torch.bfloat16) else 0
    rc = load().pk_layernorm(f32p(x, 'x', rows_ok=True), x.stride(-2) if ldx is None else ldx, f32p(gamma, 'LayerNorm gamma'), f32p(beta, 'LayerNorm beta'), eps,
                             ptr(out), out.stride(-2) if out is not None else 0, out_kind,
                             ptr(out2), out2.stride(-2) if out2 is not None else 0,
                             ptr(raw), raw.stride(-2) if raw is not None else 0, M, D, *remap, *perm, stream(x))
    _check(rc, 'pk_layernorm')


def patchify_ln(video, f0, nt, pt, ph, pw, weight, bias, out, eps=1e-5):
    B, C, F, H, W = video.shape
    rc = load().pk_patchify_ln(f32p(video, 'video'), B, C, F, H, W, f0, nt, pt, ph, pw, f32p(weight, 'LayerNorm weight'), f32p(bias, 'LayerNorm bias'), eps,   # weight = bias = None: raw rows
                               ptr(out), out.stride(0), 1 if out.dtype == torch.bfloat16 else 0, stream(video))
    _check(rc, 'pk_patchify_ln')


def patch_embed(video, ph, pw, N, groups, eps=1e-5):
    """groups: 1 or 2 tuples (Wg (N, Kpad) bf16 = gamma (.) W, s (N,), t (N,), out (rows, N) f32, f0, nt, pt), long-K group first.
    out_g = LayerNorm_P(patches of frames [f0, f0 + nt*pt)) @ W^T + b, the patch rows gathered from the video inside the kernel."""
    B, C, F, H, W = video.shape
    flat = []
    for (Wg, s, t, out, f0, nt, pt) in groups:
        flat += [ptr(Wg), Wg.stride(0), f32p(s, 'folded s'), f32p(t, 'folded t'), ptr(out), f0, nt, pt]
    if len(groups) == 1:
        flat += [None, 0, None, None, None, 0, 0, 0]
    ldo = groups[0][3].stride(0)
    rc = load().pk_patch_embed(f32p(video, 'video'), B, C, F, H, W, ph, pw, N, eps, len(groups), *flat, ldo, stream(video))
    _check(rc, 'pk_patch_embed')


def patch_embed_slices(K):
    return load().pk_patch_embed_slices(int(K))


def patch_embed_splitk(video, ph, pw, N, groups):
    """row panels x all columns x K-slices (the header): groups = 1 or 2 tuples (Wg (N, Kpad) bf16, part (slices, rows, N) f32,
    stats (slices, rows, 2) f32, f0, nt, pt), long-K group first; finish every group with patch_embed_finish"""
    B, C, F, H, W = video.shape
    flat = []
    for (Wg, part, stats, f0, nt, pt) in groups:
        flat += [ptr(Wg), Wg.stride(0), ptr(part), ptr(stats), f0, nt, pt]
    if len(groups) == 1:
        flat += [None, 0, None, None, 0, 0, 0]
    rc = load().pk_patch_embed_splitk(f32p(video, 'video'), B, C, F, H, W, ph, pw, N, len(groups), *flat, stream(video))
    _check(rc, 'pk_patch_embed_splitk')


def patch_embed_finish(part, stats, K, s, t, eps1, gamma2, beta2, eps2, *, out2=None, out=None, remap=(0, 0, 0)):
    """tokens of one frame group from its K-slices: folded LayerNorm(P) + bias, then LayerNorm(N); out2 f32 / out bf16 rows (remapped)"""
    nslices, rows, N = part.shape
    rc = load().pk_patch_embed_finish(ptr(part), ptr(stats), nslices, rows, N, int(K), f32p(s, 'folded s'), f32p(t, 'folded t'), float(eps1),
                                      f32p(gamma2, 'LayerNorm weight'), f32p(beta2, 'LayerNorm bias'), float(eps2),
                                      ptr(out2), out2.stride(-2) if out2 is not None else 0, ptr(out), out.stride(-2) if out is not None else 0,
                                      *remap, stream(part))
    _check(rc, 'pk_patch_embed_finish')


class _PatchFinishGroup(ctypes.Structure):
    _fields_ = [('part', _P), ('stats', _P), ('nslices', _I), ('rows', _I), ('K', _I), ('s', _P), ('t', _P), ('eps1', _F), ('gamma2', _P), ('beta2', _P),
                ('eps2', _F), ('remap_in', _I), ('remap_out', _I), ('remap_off', _I)]


def patch_embed_finish_groups(groups, *, out2=None, out=None):
    """pk_patch_embed_finish for 1 or 2 frame groups in ONE launch; groups: tuples (part, stats, K, s, t, eps1, gamma2, beta2, eps2, remap)"""
    arr = (_PatchFinishGroup * len(groups))()
    for d, (part, stats, K, s, t, eps1, gamma2, beta2, eps2, remap) in zip(arr, groups):
        nslices, rows, N = part.shape
        d.part, d.stats, d.nslices, d.rows, d.K = ptr(part), ptr(stats), nslices, rows, int(K)
        d.s, d.t, d.eps1 = f32p(s, 'folded s'), f32p(t, 'folded t'), float(eps1)
        d.gamma2, d.beta2, d.eps2 = f32p(gamma2, 'LayerNorm weight'), f32p(beta2, 'LayerNorm bias'), float(eps2)
        d.remap_in, d.remap_out, d.remap_off = remap
    rc = load().pk_patch_embed_finish_groups(ctypes.cast(arr, _P), len(groups), N, ptr(out2), out2.stride(-2) if out2 is not None else 0,
                                             ptr(out), out.stride(-2) if out is not None else 0, stream(groups[0][0]))
    _check(rc, 'pk_patch_embed_finish_groups')


def patch_frame_mask(src, dst, fmask, video_shape, f0, nt, pt, ph, pw):
    """dst = src with the patch-layout elements of the frames `fmask` (B, F) uint8 drops set to zero"""
    B, C, F, H, W = video_shape
    rc = load().pk_patch_frame_mask(ptr(src), src.stride(0), ptr(dst), dst.stride(0), ptr(fmask), B, C, F, H, W, f0, nt, pt, ph, pw, stream(src))
    _check(rc, 'pk_patch_frame_mask')
    return dst


def unpatchify(pix, video, f0, nt, pt, ph, pw):
    B, C, F, H, W = video.shape
    rc = load().pk_unpatchify(ptr(pix), pix.stride(0), ptr(video), B, C, F, H, W, f0, nt, pt, ph, pw, stream(video))
    _check(rc, 'pk_unpatchify')


def sqdiff_sum(a, b, frame_mask=None):
    """sum((a - b)^2) over the frames `frame_mask` (B, F) keeps (all if None) of two (B, C, F, H, W) f32 videos -> 0-d f64."""
    B, C, F, H, W = a.shape
    lib = load()
    partials = torch.empty((1024,), device=a.device, dtype=torch.float64)            # PK_SQDIFF_BLOCKS
    fm = frame_mask.to(torch.uint8).contiguous() if frame_mask is not None else None
    _check(lib.pk_sqdiff_partials(ptr(a), ptr(b), ptr(fm), B, C, F, H, W, ptr(partials), stream(a)), 'pk_sqdiff_partials')
    return partials.sum()


def peg(x, wt, bias, out, B, T, H, W, D, causal, out_t=None):
    rc = load().pk_peg(f32p(x, 'x', rows_ok=True), f32p(wt, 'PEG weight'), f32p(bias, 'PEG bias'), ptr(out), ptr(out_t), B, T, H, W, D,
                       1 if causal else 0, stream(x))
    _check(rc, 'pk_peg')


def lfq_encode(x, wp, bp, ids, proj, M, D, cd):
    rc = load().pk_lfq_encode(ptr(x), x.stride(-2), f32p(wp, 'LFQ project_in.weight'), f32p(bp, 'LFQ project_in.bias'), ptr(ids), ptr(proj), M, D, cd, stream(x))
    _check(rc, 'pk_lfq_encode')


def lfq_decode(ids, wo, bo, out, M, D, cd, *, ids_prime=None, perm=(0, 0)):
    """out[orow] = project_out(+-1 bits of id[row]); ids_prime (nb, n_prime) int64: the primed tokens in front of every sequence of
    ids (nb, n) (M = nb * (n_prime + n)); perm = (pb, pc): rows (a, b, c) are written at (a, c, b)"""
    n_prime = ids_prime.shape[-1] if ids_prime is not None else 0
    n = ids.shape[-1] if ids_prime is not None else 0
    rc = load().pk_lfq_decode(ptr(ids), f32p(wo, 'LFQ project_out.weight'), f32p(bo, 'LFQ project_out.bias'), ptr(out), M, D, cd,
                              ptr(ids_prime), n_prime, n, perm[0], perm[1], stream(out))
    _check(rc, 'pk_lfq_decode')


def lfq_aux(proj, *, inv_temperature=100., codebook_scale=1., entropy_loss_weight=0.1, commitment_loss_weight=0.25, diversity_gamma=1.):
    """training-mode auxiliary loss of the LFQ for proj (M, cd) f32 = project_in(x) (the header's pk_lfq_aux_* group):
    returns (out (4,) f32 = [aux, per-sample entropy, codebook entropy, commitment], dproj (M, cd) = d aux / d proj)."""
    lib = load()
    M, cd = proj.shape
    dev = proj.device
    hi, lo = (cd + 1) // 2, cd // 2
    NA, NB = 1 << hi, 1 << lo
    f32 = lambda *shape: torch.empty(shape, device=dev, dtype=torch.float32)
    A, B, ent, commit = f32(M, NA), f32(M, NB), f32(M), f32(M)
    alpha = 4. * float(inv_temperature) * float(codebook_scale)
    st = stream(proj)
    _check(lib.pk_lfq_aux_prep(f32p(proj, 'LFQ projection'), M, cd, alpha, float(codebook_scale), ptr(A), ptr(B), ptr(ent), ptr(commit), st), 'pk_lfq_aux_prep')
    Q = bmm(A, B, f32(NA, NB), True, False, 1, NA, NB, M, lda=NA, ldb=NB, ldc=NB)                       # A^T B = M x the batch distribution
    G, hc = f32(NA, NB), f32(lib.pk_lfq_aux_parts(cd))
    w_e, w_c, gamma = float(entropy_loss_weight), float(commitment_loss_weight), float(diversity_gamma)
    _check(lib.pk_lfq_aux_codebook(ptr(Q), cd, 1. / M, -w_e * gamma / M, ptr(G), ptr(hc), st), 'pk_lfq_aux_codebook')
    GA = bmm(B, G, f32(M, NA), False, True, 1, M, NA, NB, lda=NB, ldb=NB, ldc=NA)                      # B G^T
    GB = bmm(A, G, f32(M, NB), False, False, 1, M, NB, NA, lda=NA, ldb=NB, ldc=NB)                     # A G
    dproj, out = f32(M, cd), f32(4)
    _check(lib.pk_lfq_aux_grad(ptr(proj), ptr(GA), ptr(GB), M, cd, alpha, float(codebook_scale), w_e / M, 2. * w_c / (M * cd), ptr(dproj), st), 'pk_lfq_aux_grad')
    _check(lib.pk_lfq_aux_finish(ptr(ent), ptr(commit), M, ptr(hc), cd, w_e, gamma, w_c, ptr(out), st), 'pk_lfq_aux_finish')
    return out, dproj


def vq_gather_commit(x, E, ids, keep, y, rowsq):
    """y[r] = E[ids[r]]; rowsq[r] = sum_d (y[r] - x[r])^2 for the rows `keep` (M,) uint8 keeps (None: all), 0 for the others"""
    M, D = x.shape
    rc = load().pk_vq_gather_commit(f32p(x, 'x'), f32p(E, 'codebook'), ptr(ids), ptr(keep), M, E.shape[0], D, ptr(y), ptr(rowsq), stream(x))
    _check(rc, 'pk_vq_gather_commit')


def vq_commit_bwd(dy, x, q, keep, coef, coef_dev, dx):
    """dx = dy + coef * coef_dev[0] * keep[r] * (x - q), q = the rows vq_gather_commit wrote"""
    M, D = x.shape
    rc = load().pk_vq_commit_bwd(f32p(dy, 'dy'), f32p(x, 'x'), f32p(q, 'q'), ptr(keep), M, D, float(coef), f32p(coef_dev, 'd commit'), ptr(dx), stream(x))
    _check(rc, 'pk_vq_commit_bwd')
    return dx


def vq_ema_update(xn, ids, keep, cluster_size, embed_avg, embed, decay, eps, check_ids=False):
    """EMA codebook update of the cosine-sim VectorQuantize, in place on cluster_size (V,), embed_avg (V, D), embed (V, D), from the kept rows of
    xn (M, D) = l2norm(x) and their ids: counting sort by id (pk_vq_hist / scan / fill), then one wave per code (pk_vq_codebook_update).
    Returns counts (V,) int32 = the bins of this step."""
    lib = load()
    M, D = xn.shape
    V = embed.shape[0]
    dev = xn.device
    st = stream(xn)
    counts = torch.zeros((V,), device=dev, dtype=torch.int32)
    offsets, cursor = torch.empty_like(counts), torch.empty_like(counts)
    rows = torch.empty((M,), device=dev, dtype=torch.int32)
    S = torch.empty((1,), device=dev, dtype=torch.float32)
    cs, ea, em = f32p(cluster_size, 'cluster_size'), f32p(embed_avg, 'embed_avg'), f32p(embed, 'embed')
    _check(lib.pk_vq_hist(ptr(ids), ptr(keep), M, V, ptr(counts), 1 if check_ids else 0, st), 'pk_vq_hist')
    _check(lib.pk_vq_scan(ptr(counts), V, float(decay), cs, ptr(offsets), ptr(cursor), ptr(S), st), 'pk_vq_scan')
    _check(lib.pk_vq_fill(ptr(ids), ptr(keep), M, V, ptr(cursor), ptr(rows), st), 'pk_vq_fill')
    _check(lib.pk_vq_codebook_update(f32p(xn, 'xn'), ptr(counts), ptr(offsets), ptr(rows), cs, ptr(S), M, V, D, float(decay), float(eps), ea, em, st),
           'pk_vq_codebook_update')
    return counts


def vq_compact_keep(keep):
    """keep (M,) uint8 -> (kept (M,) int32: the kept row indices, ascending, in its first n entries; n_keep (1,) int32 = n), both on the device"""
    M = keep.numel()
    kept = torch.empty((M,), device=keep.device, dtype=torch.int32)
    n_keep = torch.empty((1,), device=keep.device, dtype=torch.int32)
    _check(load().pk_vq_compact_keep(ptr(keep), M, ptr(kept), ptr(n_keep), stream(keep)), 'pk_vq_compact_keep')
    return kept, n_keep


def vq_ema_update_expire(xn, ids, keep, cluster_size, embed_avg, embed, decay, eps, threshold, reset, b, check_ids=False):
    """vq_ema_update followed by dead-code expiry in the same four launches (+ the compaction of `keep` when there is a mask): a code whose
    post-EMA cluster_size is < threshold takes the j-th chosen kept row, j = its rank among the expired codes (pick(b, j, n_keep), host integer b):
    embed = that row of xn, embed_avg = reset * it, cluster_size = reset.  Returns (counts, jrank) (V,) int32; jrank >= 0 marks the expired codes."""
    lib = load()
    M, D = xn.shape
    V = embed.shape[0]
    dev = xn.device
    st = stream(xn)
    counts = torch.zeros((V,), device=dev, dtype=torch.int32)
    offsets, cursor, jrank = torch.empty_like(counts), torch.empty_like(counts), torch.empty_like(counts)
    rows = torch.empty((M,), device=dev, dtype=torch.int32)
    S = torch.empty((1,), device=dev, dtype=torch.float32)
    if not (float(threshold) >= 0. and float(reset) >= 0. and int(b) >= 0):
        _check(-1, 'vq_ema_update_expire (threshold, reset_cluster_size and b must be >= 0)')
    kept, n_keep = vq_compact_keep(keep) if keep is not None else (None, None)
    cs, ea, em = f32p(cluster_size, 'cluster_size'), f32p(embed_avg, 'embed_avg'), f32p(embed, 'embed')
    _check(lib.pk_vq_hist(ptr(ids), ptr(keep), M, V, ptr(counts), 1 if check_ids else 0, st), 'pk_vq_hist')
    _check(lib.pk_vq_scan_expire(ptr(counts), V, float(decay), float(threshold), cs, ptr(offsets), ptr(cursor), ptr(S), ptr(jrank), st), 'pk_vq_scan_expire')
    _check(lib.pk_vq_fill(ptr(ids), ptr(keep), M, V, ptr(cursor), ptr(rows), st), 'pk_vq_fill')
    _check(lib.pk_vq_codebook_update_expire(f32p(xn, 'xn'), ptr(counts), ptr(offsets), ptr(rows), cs, ptr(S), ptr(jrank), ptr(kept), ptr(n_keep), M, V, D,
                                            float(decay), float(eps), float(reset), int(b), ea, em, st), 'pk_vq_codebook_update_expire')
    return counts, jrank


def vq_kmeans(data, keep, means, iters, b, lookup, *, embed_avg=None, cluster_size=None, trace=False):
    """Spherical k-means on the kept rows of data (M, D) unit-norm f32, in place on means (V, D): seeds means[c] = the c-th chosen kept row
    (pk_vq_pick_rows, host integer b), then `iters` times ids = lookup(data, means) (the exact-f32 cosine argmax, lower index on ties), counting
    sort, means[c] = l2norm(sum of its rows, ascending) where a code has rows.  embed_avg (V, D) / cluster_size (V,): written by the LAST
    iteration as means * bins and bins.  Returns (means, bins (V,) int32 of the last assignment, ids (iters, M) int64[, the means after every
    iteration (iters, V, D) with trace])."""
    lib = load()
    M, D = data.shape
    V = means.shape[0]
    dev = data.device
    st = stream(data)
    if int(iters) < 1:
        _check(-1, 'vq_kmeans (kmeans_iters < 1)')
    kept, n_keep = vq_compact_keep(keep) if keep is not None else (None, None)
    mp = f32p(means, 'means')
    _check(lib.pk_vq_pick_rows(f32p(data, 'data'), ptr(kept), ptr(n_keep), M, V, D, int(b), mp, st), 'pk_vq_pick_rows')
    offsets, cursor = (torch.empty((V,), device=dev, dtype=torch.int32) for _ in range(2))
    rows = torch.empty((M,), device=dev, dtype=torch.int32)
    S, scratch = torch.empty((1,), device=dev, dtype=torch.float32), torch.empty((V,), device=dev, dtype=torch.float32)
    all_ids, all_means, counts = [], [], None
    for it in range(int(iters)):
        ids = lookup(data, means)
        counts = torch.zeros((V,), device=dev, dtype=torch.int32)
        scratch.zero_()                                               # the scan's EMA of cluster_size lands here, never in the module's buffer
        last = it == int(iters) - 1 and embed_avg is not None
        _check(lib.pk_vq_hist(ptr(ids), ptr(keep), M, V, ptr(counts), 0, st), 'pk_vq_hist')
        _check(lib.pk_vq_scan(ptr(counts), V, 1.0, ptr(scratch), ptr(offsets), ptr(cursor), ptr(S), st), 'pk_vq_scan')
        _check(lib.pk_vq_fill(ptr(ids), ptr(keep), M, V, ptr(cursor), ptr(rows), st), 'pk_vq_fill')
        _check(lib.pk_vq_kmeans_means(f32p(data, 'data'), ptr(counts), ptr(offsets), ptr(rows), M, V, D, mp, f32p(embed_avg, 'embed_avg') if last else None,
                                      f32p(cluster_size, 'cluster_size') if last else None, st), 'pk_vq_kmeans_means')
        all_ids.append(ids)
        if trace:
            all_means.append(means.clone())
    out = (means, counts, torch.stack(all_ids))
    return out + (torch.stack(all_means),) if trace else out


def frame_sqerr(a, b, clamp_hi=0., data_range=None):
    """per-frame mean of (a - b)^2 over C H W of two contiguous f32 (B, C, F, H, W) videos -> mse (B, F) f32 [and, with data_range, psnr (B, F) f32].
    clamp_hi > 0: the first operand is read clamped to [0, clamp_hi]."""
    B, C, F, H, W = a.shape
    lib = load()
    parts = lib.pk_frame_sqerr_parts(H, W)
    if parts < 0:
        _check(parts, 'pk_frame_sqerr_parts')
    partials = torch.empty((B * C * F * parts,), device=a.device, dtype=torch.float64)
    mse = torch.empty((B, F), device=a.device, dtype=torch.float32)
    psnr = torch.empty_like(mse) if data_range is not None else None
    _check(lib.pk_frame_sqerr(f32p(a, 'a'), f32p(b, 'b'), B, C, F, H, W, float(clamp_hi), float(data_range or 0.), ptr(partials), partials.numel(),
                              ptr(mse), ptr(psnr), stream(a)), 'pk_frame_sqerr')
    return (mse, psnr) if psnr is not None else mse


def frame_ssim(a, b, data_range=1., clamp_hi=0.):
    """per-frame SSIM (11 x 11 Gaussian window, sigma 1.5, 'valid' positions) of two contiguous f32 (B, C, F, H, W) videos, H, W >= 11 -> (B, F) f32"""
    B, C, F, H, W = a.shape
    lib = load()
    parts = lib.pk_frame_ssim_parts(H, W)
    if parts < 0:
        _check(parts, 'pk_frame_ssim_parts')
    partials = torch.empty((B * C * F * parts,), device=a.device, dtype=torch.float64)
    out = torch.empty((B, F), device=a.device, dtype=torch.float32)
    _check(lib.pk_frame_ssim(f32p(a, 'a'), f32p(b, 'b'), B, C, F, H, W, float(clamp_hi), float(data_range), ptr(partials), partials.numel(), ptr(out),
                             stream(a)), 'pk_frame_ssim')
    return out


def code_hist(ids, keep, V):
    """counts (V,) int32 of the kept ids (pk_vq_hist; an id outside [0, V) is dropped on the device, nothing synchronises)"""
    M = ids.numel()
    counts = torch.zeros((V,), device=ids.device, dtype=torch.int32)
    _check(load().pk_vq_hist(ptr(ids), ptr(keep), M, V, ptr(counts), 0, stream(ids)), 'pk_vq_hist')
    return counts


def code_usage(counts):
    """(V,) int32 counts -> (5,) f64 on the device: total, used codes, entropy (nats), perplexity, largest share"""
    out = torch.empty((5,), device=counts.device, dtype=torch.float64)
    _check(load().pk_code_usage(ptr(counts), counts.numel(), ptr(out), stream(counts)), 'pk_code_usage')
    return out


def embed(ids, tok, pos, out, S, n, D, *, nb=None, ids_prime=None, out_t=None):
    """out[s*n_tot + i] = tok[id] + pos[i]; ids (nb, n) int64 shared by the S sequences (s % nb), ids_prime (nb, n_prime) optional"""
    n_prime = ids_prime.shape[-1] if ids_prime is not None else 0
    rc = load().pk_embed(ptr(ids_prime), n_prime, ptr(ids), n, S if nb is None else nb, f32p(tok, 'token_emb.weight'),
                         f32p(pos, 'pos_emb.weight'), ptr(out), ptr(out_t), S, D, stream(out))
    _check(rc, 'pk_embed')


def layernorm_lfq(x, gamma, beta, wp, bp, ids, M, D, cd, *, tokens=None, proj=None, eps=1e-5, perm=(0, 0)):
    """ids[orow] = LFQ(LayerNorm(x[row])): the encoder's final norm_out fused with the quantizer (cd <= 16)"""
    rc = load().pk_layernorm_lfq(f32p(x, 'x', rows_ok=True), x.stride(-2), f32p(gamma, 'LayerNorm gamma'), f32p(beta, 'LayerNorm beta'), eps,
                                 f32p(wp, 'LFQ project_in.weight'), f32p(bp, 'LFQ project_in.bias'), ptr(ids), ptr(tokens),
                                 tokens.stride(-2) if tokens is not None else 0, ptr(proj), M, D, cd, *perm, stream(x))
    _check(rc, 'pk_layernorm_lfq')


def cpb_input(w0, b0, out, dims, D):
    nd = len(dims)
    d = (1,) * (3 - nd) + tuple(dims)
    rc = load().pk_cpb_input(ptr(w0), ptr(b0), ptr(out), d[0], d[1], d[2], nd, D, stream(out))
    _check(rc, 'pk_cpb_input')


def attn_pads(nq, n_kv, nnull):
    a, b = _I(0), _I(0)
    _check(load().pk_attn_pads(nq, n_kv, nnull, ctypes.byref(a), ctypes.byref(b)), 'pk_attn_pads')
    return a.value, b.value


def attn_prep(dtype, q, kv, null_kv, q_scale, k_scale, scale, Qp, Kp, Vt, S, h, nq, n_kv, nnull, dim_head=64):
    """q_scale = k_scale = None: plain dot-product attention operands (no l2norm; q * scale) -- the T5 text encoder.
    dim_head: 32 | 64 | 128, the width of a head in q / kv / null_kv / the scales and of the image rows"""
    rc = load().pk_attn_prep_dh(dim_head, dtype, ptr(q), q.stride(-2), ptr(kv), kv.stride(-2) if kv is not None else 0, f32p(null_kv, 'null_kv') if nnull else None,
                             f32p(q_scale, 'q_scale'), f32p(k_scale, 'k_scale'), scale, ptr(Qp), ptr(Kp), ptr(Vt), S, h, nq, n_kv, nnull, stream(q))
    _check(rc, 'pk_attn_prep_dh')


def rmsnorm(x, w, M, D, out, eps=1e-6, rowmask=None):
    rc = load().pk_rmsnorm(f32p(x, 'x', rows_ok=True), x.stride(-2), f32p(w, 'T5LayerNorm weight'), eps, ptr(rowmask), ptr(out), out.stride(-2),
                           1 if out.dtype == torch.bfloat16 else 0, M, D, stream(x))
    _check(rc, 'pk_rmsnorm')


def gated_gelu_tanh(h, out, M, F):
    rc = load().pk_gated_gelu_tanh(ptr(h), h.stride(-2), ptr(out), out.stride(-2), 1 if out.dtype == torch.bfloat16 else 0, M, F, stream(h))
    _check(rc, 'pk_gated_gelu_tanh')


def _qkv_dtype(xq):
    """operand type of the fused projection kernels from the rows they read: bf16 rows -> 1 (bf16), f32 rows -> 2 (split-bf16)"""
    if xq.dtype == torch.bfloat16:
        return BF16
    if xq.dtype == torch.float32:
        return BF16X3
    raise RuntimeError(f'fused projection kernels take bf16 (bf16 mode) or f32 (bf16x3 mode) rows, got {xq.dtype}')


def qkv_project(xq, xkv, wq, wkv, S, nseq, h, K, q_scale, k_scale, scale, Qp, Kp, Vt, nq_pad, nk_pad, q_ln_s=None):
    rc = load().pk_qkv_project(_qkv_dtype(xq), ptr(xq), ptr(xkv), xq.stride(-2), ptr(wq), ptr(wkv), wq.stride(0), S, nseq, h, K, f32p(q_scale, 'q_scale'),
                                f32p(k_scale, 'k_scale'), scale, ptr(Qp), ptr(Kp), ptr(Vt), nq_pad, nk_pad, ptr(q_ln_s), stream(xq))
    _check(rc, 'pk_qkv_project')


def qkv_attn(xq, xkv, wq, wkv, S, n, h, K, q_scale, k_scale, scale, O, *, bias=None, slopes=None, causal=False, q_ln_s=None):
    """O (S*n, h*64) <- softmax(l2norm(xq Wq^T) l2norm(xkv Wk^T)^T * scale + bias) (xkv Wv^T), n <= 64 (one launch); bf16 rows / bf16 O, or
    f32 rows / f32 O with split-bf16 products"""
    bh, bld = (bias.stride(0), bias.stride(1)) if bias is not None else (0, 0)
    rc = load().pk_qkv_attn(_qkv_dtype(xq), ptr(xq), ptr(xkv), xq.stride(-2), ptr(wq), ptr(wkv), wq.stride(0), S, n, h, K, f32p(q_scale, 'q_scale'),
                            f32p(k_scale, 'k_scale'), scale, f32p(bias, 'attention bias'), bh, bld, f32p(slopes, 'ALiBi slopes'),
                            1 if causal else 0, ptr(O), O.stride(-2), ptr(q_ln_s), stream(xq))
    _check(rc, 'pk_qkv_attn')


def q_attn_cached(xq, wq, S, n, h, K, q_scale, scale, Kp, Vt, nk_pad, n_kv, nnull, O, *, kmask=None, q_ln_s=None):
    """O (S*n, h*64) <- cross-attention of the rows of xq against the cached K^ / V^T images (one launch; n % 64 == 0, <= 64 keys)"""
    rc = load().pk_q_attn_cached(_qkv_dtype(xq), ptr(xq), xq.stride(-2), ptr(wq), wq.stride(0), S, n, h, K, f32p(q_scale, 'q_scale'), scale, ptr(q_ln_s),
                                 ptr(Kp), ptr(Vt), nk_pad, n_kv, nnull, ptr(kmask), ptr(O), O.stride(-2), stream(xq))
    _check(rc, 'pk_q_attn_cached')


def attn_fwd(dtype, Qp, Kp, Vt, O, S, h, nq, n_kv, nnull, *, bias=None, kmask=None, slopes=None, causal=False, bias_table=None,
             score_bound=None, lse=None, drop=None, dim_head=64):
    """bias: full (h, nq, n_kv) f32 tensor, or bias_table = (tab (h, L) f32, pos_code (n,) int32, offset, ...): the relative-position
    form.  score_bound: upper bound of sim + bias (python float) -> fixed-offset softmax; None: running-max flash loop.
    lse ((S h nq,) f32; the training forward): also write every row's log-sum-exp for pk_attn_bwd_ws.
    dim_head: 32 | 64 | 128 as given to attn_prep; other than 64: the LDS-free kernel, no bias_table / score_bound / drop."""
    tab, codes, off = bias_table[:3] if bias_table is not None else (None, None, 0)
    run4 = 1 if (bias_table is not None and len(bias_table) > 5 and bias_table[5]) else 0
    if bias is not None:
        bh, bld = bias.stride(0), bias.stride(1)
    else:
        bh, bld = 0, 0
    if lse is not None or drop is not None:                               # the training forward; drop: the DropSite of attn_dropout > 0
        assert lse is not None and bias_table is None and score_bound is None
        rc = load().pk_attn_fwd_lse_dh(dim_head, dtype, ptr(Qp), ptr(Kp), ptr(Vt), ptr(bias), bh, bld, ptr(kmask), f32p(slopes, 'ALiBi slopes'),
                                    1 if causal else 0, ptr(O), O.stride(-2), 1 if O.dtype == torch.float32 else 0, S, h, nq, n_kv, nnull, ptr(lse),
                                    _site(drop), stream(O))
        _check(rc, 'pk_attn_fwd_lse_dh')
        return
    rc = load().pk_attn_fwd_dh(dim_head, dtype, ptr(Qp), ptr(Kp), ptr(Vt), ptr(bias), bh, bld, ptr(kmask), f32p(slopes, 'ALiBi slopes'),
                            1 if causal else 0, ptr(O), O.stride(-2), 1 if O.dtype == torch.float32 else 0,
                            S, h, nq, n_kv, nnull, f32p(tab, 'bias table'), tab.shape[1] if tab is not None else 0, ptr(codes), off, run4,
                            float('nan') if score_bound is None else float(score_bound), stream(O))
    _check(rc, 'pk_attn_fwd_dh')


def attn_small(q, kv, q_scale, k_scale, scale, O, S, h, n, *, bias=None, kmask=None, slopes=None, causal=False):
    bh, bld = (bias.stride(0), bias.stride(1)) if bias is not None else (0, 0)
    rc = load().pk_attn_small(ptr(q), q.stride(-2), ptr(kv), kv.stride(-2), f32p(q_scale, 'q_scale'), f32p(k_scale, 'k_scale'), scale, ptr(bias), bh, bld,
                              ptr(kmask), f32p(slopes, 'ALiBi slopes'), 1 if causal else 0, ptr(O), O.stride(-2),
                              1 if O.dtype == torch.bfloat16 else 0, S, h, n, stream(q))
    _check(rc, 'pk_attn_small')


def cfg_mix(x, nb, n_tot, n_prime, rows, nrows, scale, has_null, out, D):
    rc = load().pk_cfg_mix(ptr(x), x.stride(-2), nb, n_tot, n_prime, ptr(rows), nrows, scale, 1 if has_null else 0,
                           ptr(out), out.stride(-2), 1 if out.dtype == torch.float32 else 0, D, stream(x))
    _check(rc, 'pk_cfg_mix')


def _guidance_coef(coef, x, nb, n_tot, P, has_base, name):
    """the table row of pk_guidance_mix / pk_critic_head_guided: contiguous f32 [(P + 1) * nb] on x's device, and x long enough for the
    (P + has_base) * nb sequences the kernel reads (the C entry points cannot see either)"""
    if coef is None or coef.dtype != torch.float32 or not coef.is_contiguous() or coef.device != x.device:
        raise ValueError(f'{name}: coef must be a contiguous float32 tensor on {x.device}')
    if 1 <= P <= 3:
        if coef.numel() < (P + 1) * nb:
            raise ValueError(f'{name}: coef holds {coef.numel()} values, P = {P} and nb = {nb} need {(P + 1) * nb}')
        if x.shape[0] < (P + (1 if has_base else 0)) * nb * n_tot:
            raise ValueError(f'{name}: x has {x.shape[0]} rows, {P} + {int(bool(has_base))} branches of {nb} x {n_tot} tokens need more')
    return coef.data_ptr()


def guidance_mix(x, nb, n_tot, n_prime, rows, nrows, coef, P, has_base, out, D):
    """pk_guidance_mix: x ((P + has_base) * nb * n_tot, D) f32 laid out [cond_0 | .. | cond_{P-1} | base]; coef f32 [(P + 1) * nb] on the device
    (blend weights a[k][b] in rows 0..P-1, the guidance scale g[b] in row P)"""
    rc = load().pk_guidance_mix(ptr(x), x.stride(-2), nb, n_tot, n_prime, ptr(rows), nrows, _guidance_coef(coef, x, nb, n_tot, P, has_base, 'guidance_mix'),
                                P, 1 if has_base else 0, ptr(out), out.stride(-2), 1 if out.dtype == torch.float32 else 0, D, stream(x))
    _check(rc, 'pk_guidance_mix')


def vocab_ntiles(V):
    return load().pk_vocab_ntiles(V)


def l2norm_rows(x, out, M, D):
    rc = load().pk_l2norm_rows(ptr(x), x.stride(-2), ptr(out), out.stride(-2), 1 if out.dtype == torch.bfloat16 else 0, M, D, stream(x))
    _check(rc, 'pk_l2norm_rows')


def vocab_sample(dtype, A, W, bias, M, V, D, temperature, U, rows, seed, need_lse, partials, no_noise=False, seed_dev=None):
    rc = load().pk_vocab_sample(dtype, ptr(A), A.stride(-2), ptr(W), W.stride(0), f32p(bias, 'to_logits.bias'), M, V, D, temperature,
                                ptr(U), ptr(rows), seed & 0xFFFFFFFFFFFFFFFF, ptr(seed_dev), (1 if need_lse else 0) | (2 if no_noise else 0),
                                ptr(partials), stream(A))
    _check(rc, 'pk_vocab_sample')


def vocab_reduce(partials, M, V, rows, mask, ids, pred, scores, need_lse):
    rc = load().pk_vocab_reduce(ptr(partials), M, V, ptr(rows), ptr(mask), ptr(ids), ptr(pred), ptr(scores),
                                1 if need_lse else 0, stream(partials))
    _check(rc, 'pk_vocab_reduce')


def logits_topk_sample(logits, M, V, k, temperature, U, rows, row_base, seed, need_lse, mask, ids, pred, scores, *, no_noise=False, seed_dev=None,
                       cut_out=None, kept_out=None):
    """top-k filtered sampling on M rows of f32 logits (row stride logits.stride(-2)); see pk_logits_topk_sample in the header"""
    rc = load().pk_logits_topk_sample(f32p(logits, 'logits', rows_ok=True), logits.stride(-2), M, V, int(k), temperature, ptr(U), ptr(rows), int(row_base),
                                      seed & 0xFFFFFFFFFFFFFFFF, ptr(seed_dev), (1 if need_lse else 0) | (2 if no_noise else 0), ptr(mask), ptr(ids),
                                      ptr(pred), ptr(scores), ptr(cut_out), ptr(kept_out), stream(logits))
    _check(rc, 'pk_logits_topk_sample')


FILTER_SLAB_MB = 256          # the fastest of 64 / 128 / 256 at 4608 and 9216 rows x 65 536 (profiles/filtered_sample_time.txt): 1024 rows per slab


def filter_slab_rows(M, V):
    """rows of the f32 logits slab of the filtered head: min(M, PK_FILTER_SLAB_MB * 2^20 // (4 V)), at least 1"""
    mb = int(os.environ.get('PK_FILTER_SLAB_MB', FILTER_SLAB_MB))
    return max(1, min(int(M), (mb << 20) // (4 * int(V))))


def vocab_sample_filtered(dtype, A, W, bias, M, V, D, k, temperature, U, rows, seed, need_lse, mask, ids, pred, scores, slab, seed_dev=None):
    """the vocabulary head with a top-k filter, slab by slab of R = slab.shape[0] rows: logits = A[m0:m0+Rc] @ W^T + bias into the (R, V) f32
    slab (pk_gemm on the head's operand images), then logits_topk_sample on those rows under rows[m0:m0+Rc] (or row_base = m0).  Every size
    is known on the host and nothing synchronises: capturable in a hipGraph."""
    R = slab.shape[0]
    for m0 in range(0, M, R):
        Rc = min(R, M - m0)
        gemm(dtype, A[m0:m0 + Rc], W, Rc, V, D, C=slab[:Rc], bias=bias)
        logits_topk_sample(slab, Rc, V, k, temperature, U, rows[m0:m0 + Rc] if rows is not None else None, 0 if rows is not None else m0, seed,
                           need_lse, mask, ids, pred, scores, seed_dev=seed_dev)


def logits_nucleus_sample(logits, M, V, k, top_p, min_p, temperature, U, rows, row_base, seed, need_lse, mask, ids, pred, scores, *, no_noise=False,
                          seed_dev=None, cut_out=None, kept_out=None):
    """top-k / nucleus / min-p filtered sampling on M rows of f32 logits (row stride logits.stride(-2)); see pk_logits_nucleus_sample in the header"""
    rc = load().pk_logits_nucleus_sample(f32p(logits, 'logits', rows_ok=True), logits.stride(-2), M, V, int(k), float(top_p), float(min_p), temperature,
                                         ptr(U), ptr(rows), int(row_base), seed & 0xFFFFFFFFFFFFFFFF, ptr(seed_dev),
                                         (1 if need_lse else 0) | (2 if no_noise else 0), ptr(mask), ptr(ids), ptr(pred), ptr(scores), ptr(cut_out),
                                         ptr(kept_out), stream(logits))
    _check(rc, 'pk_logits_nucleus_sample')


def vocab_sample_nucleus(dtype, A, W, bias, M, V, D, k, top_p, min_p, temperature, U, rows, seed, need_lse, mask, ids, pred, scores, slab, seed_dev=None):
    """vocab_sample_filtered with the adaptive filters: the same slab walk, logits_nucleus_sample on each slab's rows (k = V: no top-k, top_p = 1:
    no nucleus, min_p = 0: no min-p).  Nothing synchronises: capturable in a hipGraph."""
    R = slab.shape[0]
    for m0 in range(0, M, R):
        Rc = min(R, M - m0)
        gemm(dtype, A[m0:m0 + Rc], W, Rc, V, D, C=slab[:Rc], bias=bias)
        logits_nucleus_sample(slab, Rc, V, k, top_p, min_p, temperature, U, rows[m0:m0 + Rc] if rows is not None else None,
                              0 if rows is not None else m0, seed, need_lse, mask, ids, pred, scores, seed_dev=seed_dev)


def check_ce_regularisers(label_smoothing, z_loss_weight, who='vocab_cross_entropy'):
    """(label_smoothing, z_loss_weight) as floats; ValueError unless 0 <= label_smoothing < 1 and 0 <= z_loss_weight < inf (NaN fails both)"""
    try:
        eps, zeta = float(label_smoothing), float(z_loss_weight)
    except (TypeError, ValueError):
        raise ValueError(f'{who}: label_smoothing and z_loss_weight must be numbers, got {label_smoothing!r} and {z_loss_weight!r}') from None
    if not (0. <= eps < 1.):
        raise ValueError(f'{who}: label_smoothing must be in [0, 1), got {label_smoothing!r}')
    if not (0. <= zeta < float('inf')):
        raise ValueError(f'{who}: z_loss_weight must be finite and >= 0, got {z_loss_weight!r}')
    return eps, zeta


def vocab_weight_mean(dtype, Wimg, bias, V, D, wbar=None, bbar=None, workspace=None):
    """(wbar (D,) f32, bbar (1,) f32): the means over the V rows of the head's operand image Wimg -- read as the main loop reads it (f32, bf16,
    or the split-bf16 planes as hi + lo) -- and over bias, on the device (pk_vocab_weight_mean; fixed summation order, no host read).
    wbar / bbar: buffers to write into (only wbar[:D] and bbar[0] are written), else allocated here."""
    if dtype not in (F32, BF16, BF16X3):
        raise ValueError(f'vocab_weight_mean: unknown compute dtype {dtype}')
    require_device(Wimg, 'W image')
    if Wimg.dtype != tdtype(dtype) or Wimg.ndim != 2 or Wimg.stride(-1) != 1 or Wimg.shape[0] < V or Wimg.shape[1] < D:
        raise ValueError(f'vocab_weight_mean: W image must be (>= {V}, >= {D}) {tdtype(dtype)} with unit column stride, got {tuple(Wimg.shape)} {Wimg.dtype}')
    if bias is None or bias.numel() < V or bias.device != Wimg.device:
        raise ValueError(f'vocab_weight_mean: bias must hold {V} float32 on {Wimg.device}')
    dev = Wimg.device
    if wbar is None:
        wbar = torch.empty((D,), device=dev, dtype=torch.float32)
    if bbar is None:
        bbar = torch.empty((1,), device=dev, dtype=torch.float32)
    if wbar.numel() < D or bbar.numel() < 1 or wbar.device != dev or bbar.device != dev:
        raise ValueError(f'vocab_weight_mean: wbar must hold {D} and bbar 1 float32 on {dev}')
    lib = load()
    words = lib.pk_vocab_weight_mean_words(dtype, V, D)
    if workspace is None:
        workspace = torch.empty((max(words, 1),), device=dev, dtype=torch.float32)
    elif workspace.dtype != torch.float32 or not workspace.is_contiguous() or workspace.numel() < words or workspace.device != dev:
        raise ValueError(f'vocab_weight_mean: workspace must be >= {words} contiguous float32 on {dev}')
    rc = lib.pk_vocab_weight_mean(dtype, ptr(Wimg), Wimg.stride(0), f32p(bias, 'to_logits.bias'), V, D, f32p(wbar, 'wbar'), f32p(bbar, 'bbar'),
                                  ptr(workspace), stream(Wimg))
    _check(rc, 'pk_vocab_weight_mean')
    return wbar, bbar


def vocab_ce(dtype, partials, M, V, A, W, bias, D, targets, rows, loss, lse=None, *, label_smoothing=0., z_loss_weight=0., wbar=None, bbar=None):
    """loss[m] = lse(logits[m]) - logits[m][targets[rows[m]]] from the partials of vocab_sample(..., need_lse=True); lse (M,) f32 optional.
    label_smoothing / z_loss_weight: loss[m] = lse - (1 - eps) logit[target] - eps mean_v logit[m][v] + zeta lse^2 (pk_vocab_ce_reg), with
    (wbar, bbar) of vocab_weight_mean on the same W / bias (needed when label_smoothing > 0); both zero: the plain call."""
    if label_smoothing == 0. and z_loss_weight == 0.:
        rc = load().pk_vocab_ce(dtype, ptr(partials), M, V, ptr(A), A.stride(-2), ptr(W), W.stride(0), f32p(bias, 'to_logits.bias'), D,
                                ptr(targets), ptr(rows), ptr(loss), ptr(lse), stream(A))
        _check(rc, 'pk_vocab_ce')
        return
    if wbar is not None and wbar.numel() < D:
        raise ValueError(f'vocab_ce: wbar must hold {D} float32, got {tuple(wbar.shape)}')
    rc = load().pk_vocab_ce_reg(dtype, ptr(partials), M, V, ptr(A), A.stride(-2), ptr(W), W.stride(0), f32p(bias, 'to_logits.bias'), D,
                                ptr(targets), ptr(rows), ptr(loss), ptr(lse), float(label_smoothing), float(z_loss_weight),
                                f32p(wbar, 'wbar'), f32p(bbar, 'bbar'), stream(A))
    _check(rc, 'pk_vocab_ce_reg')


def vocab_eval_words(M, V):
    """4-byte words of workspace vocab_eval needs for M rows of a V-way head"""
    return load().pk_vocab_eval_words(V) * M


def vocab_eval(dtype, A, W, bias, M, V, D, targets, rows, *, pred=None, lse=None, nll=None, rank=None, entropy=None, workspace=None):
    """validation statistics of the vocab head in one pass over the vocabulary, no logits written (pk_vocab_eval + pk_vocab_eval_reduce, see the
    header).  A / W / bias / rows as vocab_sample; targets int64, indexed by rows[m] (or m) as in vocab_ce.  Outputs, each (M,) on the device or
    None (not computed): pred int64 (arg-max), lse / nll / entropy f32 (nats), rank int32 (columns other than the target with a larger logit:
    top-k is rank < k).  workspace: f32, >= vocab_eval_words(M, V) elements, allocated here unless given (a captured graph keeps its own)."""
    if dtype not in (F32, BF16, BF16X3):
        raise ValueError(f'vocab_eval: unknown compute dtype {dtype}')
    if A.dtype != tdtype(dtype) or A.ndim != 2 or A.stride(-1) != 1 or A.shape[0] < M:
        raise ValueError(f'vocab_eval: A must be (>= {M}, D) {tdtype(dtype)} with unit column stride, got {tuple(A.shape)} {A.dtype}')
    if W.dtype != tdtype(dtype) or W.ndim != 2 or W.stride(-1) != 1 or W.shape[0] < V:
        raise ValueError(f'vocab_eval: W must be (>= {V}, K) {tdtype(dtype)} with unit column stride, got {tuple(W.shape)} {W.dtype}')
    if targets.dtype != torch.int64 or not targets.is_contiguous() or (rows is None and targets.numel() < M):
        raise ValueError(f'vocab_eval: targets must be contiguous int64 with an entry per logical row, got {tuple(targets.shape)} {targets.dtype}')
    if rows is not None and (rows.dtype != torch.int32 or not rows.is_contiguous() or rows.numel() < M or rows.device != A.device):
        raise ValueError(f'vocab_eval: rows must be {M} contiguous int32 on {A.device}, got {tuple(rows.shape)} {rows.dtype} on {rows.device}')
    outs = (('pred', pred, torch.int64), ('lse', lse, torch.float32), ('nll', nll, torch.float32), ('rank', rank, torch.int32),
            ('entropy', entropy, torch.float32))
    for name, t, want in outs:
        if t is not None and (t.dtype != want or not t.is_contiguous() or t.numel() < M or t.device != A.device):
            raise ValueError(f'vocab_eval: {name} must be {M} contiguous {want} on {A.device}, got {tuple(t.shape)} {t.dtype} on {t.device}')
    if targets.device != A.device or W.device != A.device:
        raise ValueError(f'vocab_eval: operands on {A.device}, {W.device} and {targets.device}')
    for t, name in ((A, 'A'), (W, 'W'), (targets, 'targets')):
        require_device(t, name)
    words = vocab_eval_words(M, V)
    if workspace is None:
        workspace = torch.empty((words,), device=A.device, dtype=torch.float32)
    elif workspace.dtype != torch.float32 or not workspace.is_contiguous() or workspace.numel() < words or workspace.device != A.device:
        raise ValueError(f'vocab_eval: workspace must be >= {words} contiguous float32 on {A.device}')
    lib = load()
    rc = lib.pk_vocab_eval(dtype, ptr(A), A.stride(-2), ptr(W), W.stride(0), f32p(bias, 'to_logits.bias'), M, V, D, ptr(targets), ptr(rows),
                           ptr(workspace), stream(A))
    _check(rc, 'pk_vocab_eval')
    rc = lib.pk_vocab_eval_reduce(ptr(workspace), M, V, ptr(pred), ptr(lse), ptr(nll), ptr(rank), ptr(entropy), stream(A))
    _check(rc, 'pk_vocab_eval_reduce')
    return workspace


def ce_grad_slab(logits, lse, targets, rows, M, Vs, v0, scale, g, gT, db=None, scale_dev=None, *, label_smoothing=0., z_loss_weight=0., V_total=0):
    """g / gT <- (softmax - onehot) * scale [* scale_dev[0]] of one slab of vocabulary columns (see the header); logits (M, >= Vs) f32.
    label_smoothing / z_loss_weight: g = (softmax (1 + 2 zeta lse) - (1 - eps) onehot - eps / V_total) * scale (pk_ce_grad_slab_reg), V_total the
    whole vocabulary; both zero: the plain call."""
    if label_smoothing == 0. and z_loss_weight == 0.:
        rc = load().pk_ce_grad_slab(1 if g.dtype == torch.bfloat16 else 0, ptr(logits), logits.stride(0), ptr(lse), ptr(targets), ptr(rows), M, Vs, v0,
                                    float(scale), ptr(scale_dev), ptr(g), g.stride(0), ptr(gT), gT.stride(0), ptr(db), stream(logits))
        _check(rc, 'pk_ce_grad_slab')
        return
    rc = load().pk_ce_grad_slab_reg(1 if g.dtype == torch.bfloat16 else 0, ptr(logits), logits.stride(0), ptr(lse), ptr(targets), ptr(rows), M, Vs, v0,
                                    float(scale), ptr(scale_dev), ptr(g), g.stride(0), ptr(gT), gT.stride(0), ptr(db),
                                    float(label_smoothing), float(z_loss_weight), int(V_total), stream(logits))
    _check(rc, 'pk_ce_grad_slab_reg')


def topk_mask(scores, B, n, k, mask_id, mask, ids, rows_out=None, scores_next=None):
    rc = load().pk_topk_mask(ptr(scores), B, n, k, mask_id, ptr(mask), ptr(ids), ptr(rows_out), ptr(scores_next), stream(scores))
    _check(rc, 'pk_topk_mask')


def topk_mask_keep(scores, B, n, k, row_off, known, mask_id, mask, ids, rows_out=None, scores_next=None, k_host=None, free_host=None):
    """pk_topk_mask_keep (see the header): per-row k and ragged row_off as device int32 (B,), known uint8 (B, n) or None, scores f32 (B, n) or
    None (all equal: rank = index among the free positions).  k_host / free_host: the host copies of k and of the rows' free counts, where the
    caller holds them -- k[b] > free count is refused here (the kernel cannot see it without a device read)."""
    for name, t, want, numel in (('k', k, torch.int32, B), ('row_off', row_off, torch.int32, B), ('known', known, torch.uint8, B * n),
                                 ('scores', scores, torch.float32, B * n), ('scores_next', scores_next, torch.float32, B * n),
                                 ('mask', mask, torch.uint8, B * n), ('ids', ids, torch.int64, B * n), ('rows_out', rows_out, torch.int32, 0)):
        if t is not None and (t.dtype != want or not t.is_contiguous() or t.numel() < numel or t.device != mask.device):
            raise ValueError(f'topk_mask_keep: {name} must be >= {numel} contiguous {want} on {mask.device}, got {tuple(t.shape)} {t.dtype} on {t.device}')
    if k_host is not None and free_host is not None:
        if len(k_host) != B or len(free_host) != B or any(kb < 0 or kb > fb for kb, fb in zip(k_host, free_host)):
            raise ValueError(f'topk_mask_keep: k = {list(k_host)} must lie in [0, free count] = {list(free_host)} per row')
        if rows_out is not None and rows_out.numel() < sum(k_host):
            raise ValueError(f'topk_mask_keep: rows_out holds {rows_out.numel()} entries, the rows need {sum(k_host)}')
    rc = load().pk_topk_mask_keep(ptr(scores), B, n, ptr(k), ptr(row_off), ptr(known), mask_id, ptr(mask), ptr(ids), ptr(rows_out), ptr(scores_next),
                                  stream(mask))
    _check(rc, 'pk_topk_mask_keep')


def composite_mask(gen, src, mask, out):
    """out = where(mask, gen, src): gen / src / out (B, C, F, H, W) contiguous f32, mask (B | 1, F, H, W) contiguous uint8 broadcast over the
    channels (pk_composite_mask).  A select: outside the mask the output holds src's bits."""
    if gen.shape != src.shape or out.shape != src.shape or src.ndim != 5:
        raise ValueError(f'composite_mask: gen / src / out must share one (B, C, F, H, W) shape, got {tuple(gen.shape)}, {tuple(src.shape)}, {tuple(out.shape)}')
    B, C = src.shape[:2]
    if mask.dtype != torch.uint8 or mask.ndim != 4 or mask.shape[0] not in (1, B) or tuple(mask.shape[1:]) != tuple(src.shape[2:]) or not mask.is_contiguous():
        raise ValueError(f'composite_mask: mask must be contiguous uint8 ({B} | 1, F, H, W) = (.., {tuple(src.shape[2:])}), got {tuple(mask.shape)} {mask.dtype}')
    for t, name in ((gen, 'gen'), (src, 'src'), (out, 'out')):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.device != src.device:
            raise ValueError(f'composite_mask: {name} must be contiguous float32 on {src.device}, got {t.dtype} on {t.device}')
        require_device(t, name)
    if mask.device != src.device or out.data_ptr() in (gen.data_ptr(), src.data_ptr()):
        raise ValueError('composite_mask: mask on the operands\' device and out a buffer of its own')
    rc = load().pk_composite_mask(ptr(gen), ptr(src), ptr(mask), ptr(out), B, C, src[0, 0].numel(), mask.shape[0], stream(src))
    _check(rc, 'pk_composite_mask')


def critic_head(x, w, b, D, nb, n_tot, n_prime, has_null, scale, u, noise_mult, out, seed=0, seed_dev=None):
    rc = load().pk_critic_head(ptr(x), x.stride(-2), f32p(w, 'critic head weight'), f32p(b, 'critic head bias'), D, nb, n_tot, n_prime, 1 if has_null else 0, scale,
                               ptr(u), noise_mult, seed & 0xFFFFFFFFFFFFFFFF, ptr(seed_dev), ptr(out), stream(x))
    _check(rc, 'pk_critic_head')


def critic_head_guided(x, w, b, D, nb, n_tot, n_prime, coef, P, has_base, u, noise_mult, out, seed=0, seed_dev=None):
    """pk_critic_head_guided: pk_critic_head with the table row of guidance_mix in place of scale / has_null"""
    rc = load().pk_critic_head_guided(ptr(x), x.stride(-2), f32p(w, 'critic head weight'), f32p(b, 'critic head bias'), D, nb, n_tot, n_prime,
                                      _guidance_coef(coef, x, nb, n_tot, P, has_base, 'critic_head_guided'), P, 1 if has_base else 0,
                                      ptr(u), noise_mult, seed & 0xFFFFFFFFFFFFFFFF, ptr(seed_dev), ptr(out), stream(x))
    _check(rc, 'pk_critic_head_guided')


# ----------------------------------------------------------------------------- training-step kernels (csrc/train.hip, attn_train.hip)

def kind_of(dtype):
    """pk_pack's `kind` of the W-side operand image of compute dtype `dtype`"""
    return {F32: 0, BF16: 1, BF16X3: 2}[dtype]


def pack(src, R, K, transpose, out, Kp, kind, rows=None):
    """out[r][k] = src[k][r] (transpose) / src[r][k] for r < R, k < K; zero for K <= k < Kp.  rows: int32 gather of SOURCE rows."""
    rc = load().pk_pack(ptr(src), src.stride(-2), ptr(rows), R, K, 1 if transpose else 0, ptr(out), out.stride(-2), Kp, kind, stream(src))
    _check(rc, 'pk_pack')
    return out


class PackJob(ctypes.Structure):
    """include/phenaki_hip.h PkPackJob"""
    _fields_ = [('src', ctypes.c_void_p), ('out', ctypes.c_void_p), ('lds', ctypes.c_longlong), ('ldo', ctypes.c_longlong), ('R', ctypes.c_int),
                ('K', ctypes.c_int), ('Kp', ctypes.c_int), ('flags', ctypes.c_int), ('tile0', ctypes.c_int), ('tiles_x', ctypes.c_int)]


class Dropout(ctypes.Structure):
    """include/phenaki_hip.h pk_dropout"""
    _fields_ = [('seed', ctypes.c_ulonglong), ('offset', ctypes.c_ulonglong), ('keep_thr', ctypes.c_int), ('scale', ctypes.c_float)]


def _site(drop):
    """the pk_dropout argument of a DropSite (None: no dropout)"""
    return ctypes.byref(drop.c) if drop is not None else None


class SumJob(ctypes.Structure):
    """include/phenaki_hip.h PkSumJob"""
    _fields_ = [('src', ctypes.c_void_p), ('out', ctypes.c_void_p), ('stride', ctypes.c_longlong), ('E4', ctypes.c_longlong), ('S', ctypes.c_int),
                ('blk0', ctypes.c_int)]


def pack_job(src, R, K, transpose, out, Kp, kind, *, src_ld=None, out_ptr=None, out_ld=None):
    """one job of pack_multi / PackTable: out (R rows, Kp columns) = src or src^T (the OUTPUT has R rows and K data columns).  out_ptr / out_ld:
    a block inside a larger image (byte address of its first element, row pitch in elements)."""
    return PackJob(src.data_ptr(), out.data_ptr() if out_ptr is None else out_ptr, src.stride(-2) if src_ld is None else src_ld,
                   out.stride(-2) if out_ld is None else out_ld, R, K, Kp, (1 if transpose else 0) | (kind << 1), 0, 0)


def pack_multi(jobs, like):
    """up to 8 pack jobs per launch (more: several launches)"""
    for i in range(0, len(jobs), 8):
        chunk = jobs[i:i + 8]
        arr = (PackJob * len(chunk))(*chunk)
        _check(load().pk_pack_multi(ctypes.addressof(arr), len(chunk), stream(like)), 'pk_pack_multi')


class PackTable:
    """a job list kept in device memory and replayed with ONE launch (`run`): the operand images of a module's weights, re-packed every step"""

    def __init__(self, jobs, device):
        arr = (PackJob * len(jobs))(*jobs)
        tiles = load().pk_pack_table_prepare(ctypes.addressof(arr), len(jobs))
        if tiles < 0:
            _check(int(tiles), 'pk_pack_table_prepare')
        self.count, self.tiles = len(jobs), int(tiles)
        self.table = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(device)

    def run(self):
        _check(load().pk_pack_table(ptr(self.table), self.count, self.tiles, stream(self.table)), 'pk_pack_table')


class ColsumJob(ctypes.Structure):
    """include/phenaki_hip.h PkColsumJob"""
    _fields_ = [('src', ctypes.c_void_p), ('out', ctypes.c_void_p), ('ld', ctypes.c_longlong), ('M', ctypes.c_int), ('N', ctypes.c_int), ('blk0', ctypes.c_int),
                ('scale', ctypes.c_float)]


def colsum_multi(jobs):
    """jobs: [(src (M, N) f32 rows, M, N, out (N,))]: out[c] = sum_r src[r][c] for each, up to 8 per launch (M <= 8192, N % 4 == 0)"""
    for i in range(0, len(jobs), 8):
        chunk = jobs[i:i + 8]
        arr = (ColsumJob * len(chunk))(*[ColsumJob(s_.data_ptr(), o.data_ptr(), s_.stride(-2), M, N, 0, 1.0) for s_, M, N, o in chunk])
        _check(load().pk_colsum_multi(ctypes.addressof(arr), len(chunk), stream(chunk[0][0])), 'pk_colsum_multi')


def reduce_multi(sum_jobs, col_jobs):
    """the K-slice sums (sum_batch_multi's job tuples) and the short column sums (colsum_multi's) of a backward block in ONE launch"""
    if len(sum_jobs) > 8 or len(col_jobs) > 8 or not sum_jobs or not col_jobs:
        if sum_jobs:
            sum_batch_multi(sum_jobs)
        if col_jobs:
            colsum_multi(col_jobs)
        return
    assert all(E % 4 == 0 for _, _, _, E in sum_jobs)
    sa = (SumJob * len(sum_jobs))(*[SumJob(p.data_ptr(), o.data_ptr(), p.stride(0), E // 4, S, 0) for p, S, o, E in sum_jobs])
    ca = (ColsumJob * len(col_jobs))(*[ColsumJob(s_.data_ptr(), o.data_ptr(), s_.stride(-2), M, N, 0, 1.0) for s_, M, N, o in col_jobs])
    _check(load().pk_reduce_multi(ctypes.addressof(sa), len(sum_jobs), ctypes.addressof(ca), len(col_jobs), stream(sum_jobs[0][0])), 'pk_reduce_multi')


def colsum_deferred(src, M, N, out, defer):
    """pk_colsum now, or -- when the caller collects the column sums of a whole backward block (defer: a list) and the shape fits the one-launch
    form -- queued for ONE colsum_multi launch"""
    if defer is not None and M <= 8192 and N % 4 == 0 and src.stride(-2) % 4 == 0:
        defer.append((src, M, N, out))
        return out
    return colsum(src, M, N, out)


def sum_batch_multi(jobs):
    """jobs: [(part (S, >= E) f32, S, out, E)]: out[e] = sum_s part[s][e], up to 8 per launch"""
    for i in range(0, len(jobs), 8):
        chunk = jobs[i:i + 8]
        arr = (SumJob * len(chunk))(*[SumJob(p.data_ptr(), o.data_ptr(), p.stride(0), E // 4, S, 0) for p, S, o, E in chunk])
        assert all(E % 4 == 0 for _, _, _, E in chunk)
        _check(load().pk_sum_batch_multi(ctypes.addressof(arr), len(chunk), stream(chunk[0][0])), 'pk_sum_batch_multi')


def scatter_rows(src, rows, dst, M, D):
    rc = load().pk_scatter_rows(ptr(src), src.stride(-2), ptr(rows), ptr(dst), dst.stride(-2), M, D, stream(src))
    _check(rc, 'pk_scatter_rows')


def colsum(src, M, N, out, *, scale=1.0, accumulate=False, ld=None):
    """out[c] (+)= scale * sum_r src[r][c] (deterministic two-stage reduction)"""
    P = load().pk_colsum_parts(M)
    work = torch.empty((P * N,), device=src.device, dtype=torch.float32)
    rc = load().pk_colsum(ptr(src), src.stride(-2) if ld is None else ld, M, N, float(scale), ptr(out), 1 if accumulate else 0, ptr(work), stream(src))
    _check(rc, 'pk_colsum')
    return out


def layernorm_bwd(x, gamma, dy, dx, M, D, *, add=None, want_beta=False, eps=1e-5, defer=None):
    """dx = [add +] LN backward; returns (dgamma, dbeta | None).  defer (list): the column sum of the partials is queued there (colsum_multi)"""
    P = load().pk_ln_bwd_parts(M)
    # dgamma | dbeta partials as the two halves of one (P, 2 D) buffer (the kernel recognises pb == pg + D): one column sum finishes both
    pgb = torch.empty((P, 2 * D if want_beta else D), device=x.device, dtype=torch.float32)
    rc = load().pk_layernorm_bwd(ptr(x), x.stride(-2), f32p(gamma, 'LayerNorm gamma'), ptr(dy), dy.stride(-2), ptr(add), add.stride(-2) if add is not None else 0,
                                 ptr(dx), dx.stride(-2), ptr(pgb), pgb.data_ptr() + 4 * D if want_beta else None, eps, M, D, stream(x))
    _check(rc, 'pk_layernorm_bwd')
    out = colsum_deferred(pgb, P, pgb.shape[1], torch.empty((pgb.shape[1],), device=x.device, dtype=torch.float32), defer)
    return (out[:D], out[D:]) if want_beta else (out, None)


def geglu(h, goff, out, M, F, drop=None):
    """drop: the DropSite of ff_dropout > 0 (out = geglu(h) o m / (1 - p_eff)), None: no dropout; geglu_bwd takes the forward's"""
    rc = load().pk_geglu(ptr(h), h.stride(-2), goff, ptr(out), out.stride(-2), M, F, _site(drop), stream(h))
    _check(rc, 'pk_geglu')


def geglu_bwd(h, goff, dout, dh, M, F, drop=None):
    rc = load().pk_geglu_bwd(ptr(h), h.stride(-2), goff, ptr(dout), dout.stride(-2), ptr(dh), dh.stride(-2), M, F, _site(drop), stream(h))
    _check(rc, 'pk_geglu_bwd')


def dropout_mask(seed, offset, rows, cols, p, device):
    """(rows, cols) uint8 on `device`, 1 = keep: the decisions the training kernels make for the site (seed, offset) at drop probability p
    (dropout.keep_mask is the NumPy mirror)"""
    from .dropout import quantize
    out = torch.empty((rows, cols), device=device, dtype=torch.uint8)
    rc = load().pk_dropout_mask(int(seed) & 0xFFFFFFFFFFFFFFFF, int(offset) & 0xFFFFFFFFFFFFFFFF, quantize(p)[0], rows, cols, ptr(out), stream(out))
    _check(rc, 'pk_dropout_mask')
    return out


class DropSite:
    """one dropout site of a training step: the stream (seed, offset) read from the device's default torch generator on the host (no sync; the pattern
    of TorchPhilox below) and the quantised probability (dropout.quantize: thr, p_eff, scale).  Taking a site advances the generator by 4 (its offset
    granularity): the site's stream IS its offset, so layers, self- and cross-attention and the feed-forward never share a mask, and
    torch.manual_seed(s) makes a step reproducible.  Held on the autograd ctx: the backward kernels regenerate the mask from it."""

    def __init__(self, device, p):
        from .dropout import quantize
        idx = device.index if device.index is not None else torch.cuda.current_device()
        gen = torch.cuda.default_generators[idx]
        self.seed = gen.initial_seed() & 0xFFFFFFFFFFFFFFFF
        self.offset = gen.get_offset()
        gen.set_offset(self.offset + 4)
        self.p = float(p)
        self.thr, self.p_eff, self.scale = quantize(p)
        self.c = Dropout(self.seed, self.offset, self.thr, self.scale)

    @staticmethod
    def of(module, device):
        """the site of an nn.Dropout module, or None when it is inactive: like torch, dropout acts iff the module is in training mode and p > 0
        (p below 2^-9 quantises to p_eff = 0: inactive)"""
        if not module.training or module.p <= 0.:
            return None
        site = DropSite(device, module.p)
        return site if site.thr > 0 else None


def scaled_diff(a, b, scale, out, scale_dev=None):
    """out = (a - b) * scale (* scale_dev[0]) over contiguous f32 tensors of the same size"""
    rc = load().pk_scaled_diff(f32p(a, 'a'), f32p(b, 'b'), float(scale), ptr(scale_dev), ptr(out), a.numel(), stream(a))
    _check(rc, 'pk_scaled_diff')
    return out


def mul(a, b, out):
    rc = load().pk_mul(f32p(a, 'a'), f32p(b, 'b'), ptr(out), a.numel(), stream(a))
    _check(rc, 'pk_mul')
    return out


def sign(z, out, value=1.0):
    rc = load().pk_sign(f32p(z, 'z'), float(value), ptr(out), z.numel(), stream(z))
    _check(rc, 'pk_sign')
    return out


def leaky_bwd(y, dy, dz, M, N, slope=0.1):
    rc = load().pk_leaky_bwd(ptr(y), y.stride(-2), ptr(dy), dy.stride(-2), ptr(dz), dz.stride(-2), M, N, slope, stream(y))
    _check(rc, 'pk_leaky_bwd')


def peg_bwd(dy, x, wt, dx, B, T, H, W, D, causal, want_wgrad=True, defer=None):
    """dx = dy + transposed stencil; returns the (27, D) tap gradient (or None)"""
    rows = B * T * H * W
    part = None
    if want_wgrad:
        P = load().pk_peg_wgrad_parts(rows)
        part = torch.empty((P, 27 * D), device=dy.device, dtype=torch.float32)
    rc = load().pk_peg_bwd(ptr(dy), ptr(x), f32p(wt, 'PEG taps'), ptr(dx), ptr(part), B, T, H, W, D, 1 if causal else 0, stream(dy))
    _check(rc, 'pk_peg_bwd')
    if part is None:
        return None
    return colsum_deferred(part, part.shape[0], 27 * D, torch.empty((27 * D,), device=dy.device, dtype=torch.float32), defer).view(27, D)


def embed_bwd(dy, ids, alpha, dtok, dpos, S, n, D):
    rc = load().pk_embed_bwd(ptr(dy), ptr(ids), float(alpha), ptr(dtok), ptr(dpos), S, n, D, stream(dy))
    _check(rc, 'pk_embed_bwd')


def bias_gather(tab, code, off, out, heads, n):
    rc = load().pk_bias_gather(ptr(tab), tab.stride(0), ptr(code), off, ptr(out), heads, n, stream(tab))
    _check(rc, 'pk_bias_gather')


def bias_scatter(dbias, code, off, dtab, heads, n):
    rc = load().pk_bias_scatter(ptr(dbias), ptr(code), off, ptr(dtab), dtab.stride(0), heads, n, stream(dbias))
    _check(rc, 'pk_bias_scatter')


def sum_batch(src, S, out, E):
    rc = load().pk_sum_batch(ptr(src), src.stride(0), S, ptr(out), E, stream(src))
    _check(rc, 'pk_sum_batch')


def bce_head(e, w, b, labels, M, D, *, scale=0.0, logits=None, loss_rows=None, de=None, scale_dev=None):
    """returns (dw (D,), db (1,)) when de is given, else None"""
    pw = pb = None
    P = load().pk_ln_bwd_parts(M)
    if de is not None:
        pw = torch.empty((P, D), device=e.device, dtype=torch.float32)
        pb = torch.empty((P, 1), device=e.device, dtype=torch.float32)
    rc = load().pk_bce_head(ptr(e), e.stride(-2), f32p(w, 'critic head weight'), f32p(b, 'critic head bias'), ptr(labels), float(scale), ptr(scale_dev), ptr(logits), ptr(loss_rows),
                            ptr(de), de.stride(-2) if de is not None else 0, ptr(pw), ptr(pb), M, D, stream(e))
    _check(rc, 'pk_bce_head')
    if de is None:
        return None
    dw = colsum(pw, P, D, torch.empty((D,), device=e.device, dtype=torch.float32))
    db = colsum(pb, P, 1, torch.empty((1,), device=e.device, dtype=torch.float32))
    return dw, db


ATTN_PREP_BWD_PARTS = 1024


def attn_train_prep(q, kv, null_kv, q_scale, k_scale, scale, Qh, Kh, Vh, S, h, n, n_kv, nnull):
    rc = load().pk_attn_train_prep(ptr(q), q.stride(-2), ptr(kv), kv.stride(-2), f32p(null_kv, 'null_kv') if nnull else None, f32p(q_scale, 'q_scale'),
                                   f32p(k_scale, 'k_scale'), scale, ptr(Qh), ptr(Kh), ptr(Vh), S, h, n, n_kv, nnull, stream(q))
    _check(rc, 'pk_attn_train_prep')


def attn_train_prep_bwd(q, kv, null_kv, q_scale, k_scale, scale, dQh, dKh, dVh, dq, dkv, S, h, n, n_kv, nnull, defer=None):
    """-> (dq_scale (64,), dk_scale (64,), dnull_kv | None); dq / dkv are overwritten"""
    dev = q.device
    pqk = torch.empty((ATTN_PREP_BWD_PARTS, 128), device=dev, dtype=torch.float32)     # dq_scale | dk_scale partials (the kernel recognises pk == pq + 64)
    dnull = torch.empty((h, 2 * nnull, 64), device=dev, dtype=torch.float32) if nnull else None
    rc = load().pk_attn_train_prep_bwd(ptr(q), q.stride(-2), ptr(kv), kv.stride(-2), f32p(null_kv, 'null_kv') if nnull else None, f32p(q_scale, 'q_scale'),
                                       f32p(k_scale, 'k_scale'), scale, ptr(dQh), ptr(dKh), ptr(dVh), ptr(dq), dq.stride(-2), ptr(dkv), dkv.stride(-2),
                                       ptr(pqk), pqk.data_ptr() + 256, ptr(dnull), S, h, n, n_kv, nnull, stream(q))
    _check(rc, 'pk_attn_train_prep_bwd')
    out = colsum_deferred(pqk, ATTN_PREP_BWD_PARTS, 128, torch.empty((128,), device=dev, dtype=torch.float32), defer)
    return out[:64], out[64:], dnull


def attn_bwd(Qh, Kh, Vh, O, dO, dQh, dKh, dVh, S, h, n, n_kv, nnull, *, bias=None, kmask=None, dS=None, slopes=None, causal=False, split_bf16=False, lse=None,
             bf16_products=False, drop=None):
    """lse ((S h n,) f32 from attn_fwd(lse=...)): the backward skips its own log-sum-exp pass.  bf16_products: single bf16 MFMA products (the bf16 mode).
    drop: the forward's DropSite (the mask is regenerated)"""
    dev = Qh.device
    flags = (1 if split_bf16 else 0) | (2 if lse is not None else 0) | (4 if bf16_products else 0)
    if lse is None:
        lse = torch.empty((S * h * n,), device=dev, dtype=torch.float32)
    drow = torch.empty((S * h * n,), device=dev, dtype=torch.float32)
    nwork = load().pk_attn_bwd_work(S, h, n, n_kv, nnull)                  # few key tiles: partial dK / dV slabs of the query-tile groups
    work = torch.empty((nwork,), device=dev, dtype=torch.float32) if nwork > 0 else None
    rc = load().pk_attn_bwd_ws(ptr(Qh), ptr(Kh), ptr(Vh), ptr(O), O.stride(-2), 1 if O.dtype == torch.bfloat16 else 0, ptr(dO), dO.stride(-2), ptr(bias), ptr(kmask),
                               f32p(slopes, 'ALiBi slopes') if causal else None, 1 if causal else 0, ptr(dQh), ptr(dKh), ptr(dVh), ptr(dS), ptr(lse), ptr(drow), S, h, n, n_kv, nnull, flags,
                               ptr(work), nwork if nwork > 0 else 0, _site(drop), stream(Qh))
    _check(rc, 'pk_attn_bwd_ws')


def adamw(p, g, m, v, lr, beta1, beta2, eps, wd, step):
    rc = load().pk_adamw(ptr(p), ptr(g), ptr(m), ptr(v), float(lr), float(beta1), float(beta2), float(eps), float(wd), int(step), p.numel(), stream(p))
    _check(rc, 'pk_adamw')


def adamw_multi(entries, lr, beta1, beta2, eps, wd, step, device):
    """entries: list of (p, g, m, v) contiguous f32 device tensors updated with one hyper-parameter set and step number"""
    import numpy as np
    table = np.empty((len(entries), 5), dtype=np.int64)
    for i, (p, g, m, v) in enumerate(entries):
        table[i] = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel())
    rc = load().pk_adamw_multi(table.ctypes.data, len(entries), float(lr), float(beta1), float(beta2), float(eps), float(wd), int(step),
                               torch.cuda.current_stream(device).cuda_stream)
    _check(rc, 'pk_adamw_multi')


def adamw_multi_scaled(entries, lr, beta1, beta2, eps, wd, step, gscale, device):
    """adamw_multi on gradients read as g * gscale[0] (gscale: f32 device tensor, the coefficient grad_norm_coef left there)"""
    import numpy as np
    table = np.empty((len(entries), 5), dtype=np.int64)
    for i, (p, g, m, v) in enumerate(entries):
        table[i] = (p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), p.numel())
    rc = load().pk_adamw_multi_scaled(table.ctypes.data, len(entries), float(lr), float(beta1), float(beta2), float(eps), float(wd), int(step),
                                      gscale.data_ptr(), torch.cuda.current_stream(device).cuda_stream)
    _check(rc, 'pk_adamw_multi_scaled')


def _grad_table(grads):
    import numpy as np
    table = np.empty((len(grads), 2), dtype=np.int64)
    for i, g in enumerate(grads):
        table[i] = (g.data_ptr(), g.numel())
    return table


_norm_partials = {}                                    # device index -> f32 workspace of the norm pass, grown when needed


def grad_norm_coef(grads, max_norm, device):
    """grads: non-empty contiguous f32 tensors on `device` -> (table, out): out (2,) f32 = {global L2 norm, min(max_norm / (norm + 1e-6), 1)},
    left on the device (no synchronisation); table is the {g, numel} host table for scale_multi"""
    table = _grad_table(grads)
    lib, s = load(), torch.cuda.current_stream(device).cuda_stream
    nparts = lib.pk_grad_sumsq_parts(table.ctypes.data, len(grads))
    if nparts < 0:
        _check(nparts, 'pk_grad_sumsq_parts')
    work = _norm_partials.get(device.index)
    if work is None or work.numel() < nparts:
        work = _norm_partials[device.index] = torch.empty((nparts,), device=device, dtype=torch.float32)
    out = torch.empty((2,), device=device, dtype=torch.float32)
    _check(lib.pk_grad_sumsq(table.ctypes.data, len(grads), work.data_ptr(), nparts, s), 'pk_grad_sumsq')
    _check(lib.pk_grad_clip_coef(work.data_ptr(), nparts, float(max_norm), out.data_ptr(), s), 'pk_grad_clip_coef')
    return table, out


def scale_multi(table, coef, device):
    _check(load().pk_scale_multi(table.ctypes.data, table.shape[0], coef.data_ptr(), torch.cuda.current_stream(device).cuda_stream), 'pk_scale_multi')


def ema_multi(pairs, weight, device):
    """pairs: list of (ema, src) contiguous f32 device tensors of equal, non-zero numel: ema += weight (src - ema); weight >= 1 copies"""
    import numpy as np
    table = np.empty((len(pairs), 3), dtype=np.int64)
    for i, (e, x) in enumerate(pairs):
        table[i] = (e.data_ptr(), x.data_ptr(), e.numel())
    _check(load().pk_ema_multi(table.ctypes.data, len(pairs), float(weight), torch.cuda.current_stream(device).cuda_stream), 'pk_ema_multi')


def gemm_splitk(dtype, A, W, M, N, K, splits, C, bias=None, tile=0):
    """C (splits, M, N) f32 <- the K-slices of A @ W^T (see the header; bias on slice 0; tile 1: 128 x 128 tiles); reduce with sum_batch"""
    rc = load().pk_gemm_splitk(dtype, ptr(A), A.stride(-2), ptr(W), W.stride(0), M, N, K, splits, ptr(C), N, f32p(bias, 'bias'), int(tile), stream(C))
    _check(rc, 'pk_gemm_splitk')


# ----------------------------------------------------------------------------- discriminator layout kernels (csrc/conv.hip)

def conv_out_size(n, k, stride, pad):
    return (n + 2 * pad - k) // stride + 1


def im2col(x, B, H, W, C, kh, kw, stride, pad, cols):
    """x (B H W, C) channels-last pixel rows -> cols (B Ho Wo, kh kw C), column (ky, kx, c)"""
    _check(load().pk_im2col(ptr(x), B, H, W, C, kh, kw, stride, pad, ptr(cols), cols.stride(0), stream(x)), 'pk_im2col')
    return cols


def col2im(cols, B, H, W, C, kh, kw, stride, pad, dx):
    """the adjoint of im2col: dx (B H W, C) <- sum of the patch-matrix entries that read each pixel"""
    _check(load().pk_col2im(ptr(cols), cols.stride(0), B, H, W, C, kh, kw, stride, pad, ptr(dx), stream(cols)), 'pk_col2im')
    return dx


def nchw_to_rows(img, Cp, rows):
    B, C, H, W = img.shape
    _check(load().pk_nchw_to_rows(ptr(img), B, C, H, W, Cp, ptr(rows), stream(img)), 'pk_nchw_to_rows')
    return rows


def rows_to_nchw(rows, Cp, img):
    B, C, H, W = img.shape
    _check(load().pk_rows_to_nchw(ptr(rows), B, C, H, W, Cp, ptr(img), stream(rows)), 'pk_rows_to_nchw')
    return img


def pick_frames(video, frame, img, place=False):
    """img (B, C, H, W) <- video[b, :, frame[b]] (cvivit.py:217-224), or the adjoint into a zeroed video when place"""
    B, C, F, H, W = video.shape
    # `frame` reaches the kernel as a raw `const int*`: an int64 tensor (what topk returns), a host tensor or a short one must fail here
    if frame.dtype != torch.int32 or frame.device != video.device or not frame.is_contiguous() or frame.numel() != B:
        raise RuntimeError(f'pick_frames: frame must be a contiguous int32 tensor of {B} indices on {video.device}, got {frame.dtype} '
                           f'{tuple(frame.shape)} on {frame.device}')
    _check(load().pk_pick_frames(ptr(video), ptr(frame), B, C, F, H, W, ptr(img), 1 if place else 0, stream(video)), 'pk_pick_frames')
    return video if place else img


def bmm(A, B, C, tA, tB, batch, M, N, K, *, lda, ldb, ldc, sA=0, sB=0, sC=0, accumulate=False):
    """C[z] = op(A[z]) op(B[z]) in exact f32 (any shape / stride); op = transpose when tA / tB"""
    _check(load().pk_bmm(ptr(A), lda, sA, 1 if tA else 0, ptr(B), ldb, sB, 1 if tB else 0, ptr(C), ldc, sC, batch, M, N, K,
                         1 if accumulate else 0, stream(A)), 'pk_bmm')
    return C


def row_softmax(a, b, c, out, mode):
    """rows of the last dimension (contiguous f32): mode 0 softmax(a); 1 a (b - <a, b>); 2 c (b - <a, b>) - b <c, a>  (see the header)"""
    n = a.shape[-1]
    _check(load().pk_row_softmax(ptr(a), ptr(b), ptr(c), ptr(out), a.numel() // n, n, mode, stream(a)), 'pk_row_softmax')
    return out


def row_l2scale(x, sc, dz, gx, gsc, o0, o1, o2, mode):
    d = x.shape[-1]
    _check(load().pk_row_l2scale(ptr(x), ptr(sc), ptr(dz), ptr(gx), ptr(gsc), ptr(o0), ptr(o1), ptr(o2), x.numel() // d, d, mode, stream(x)), 'pk_row_l2scale')


def row_ln_bwd2(x, gamma, dy, u, w, eps, grad_x, grad_gamma_rows, grad_dy):
    D = x.shape[-1]
    _check(load().pk_row_ln_bwd2(ptr(x), ptr(gamma), ptr(dy), ptr(u), ptr(w), float(eps), ptr(grad_x), ptr(grad_gamma_rows), ptr(grad_dy),
                                 x.numel() // D, D, stream(x)), 'pk_row_ln_bwd2')


# ----------------------------------------------------------------------------- perceptual network kernels (csrc/vgg.hip)

def _is_f32(t, what):
    if t.dtype not in (torch.float32, torch.bfloat16):
        raise RuntimeError(f'{what}: pixel rows are float32 or bfloat16, got {t.dtype}')
    return 1 if t.dtype == torch.float32 else 0


def conv3x3(dtype, x, W, B, H, Wd, C, Co, y, *, bias=None, relu=False, gate=None, tile=0):
    """y (B H Wd, Co) = act(bias + the 3x3 / stride 1 / pad 1 convolution of the pixel rows x (B H Wd, C)); W (Co, Kpad): the pk_gemm weight image of
    `dtype` over the 9 C columns in im2col order.  gate (B H Wd, C): x is read as 0 where gate <= 0 (the fused ReLU backward of the backward-data form)."""
    for t, c, what in ((x, C, 'x'), (y, Co, 'y')) + (((gate, C, 'gate'),) if gate is not None else ()):
        if not t.is_contiguous() or t.numel() != B * H * Wd * c:
            raise RuntimeError(f'pk_conv3x3: {what} must be contiguous ({B * H * Wd}, {c}) pixel rows, got {tuple(t.shape)}')
    rc = load().pk_conv3x3(dtype, _is_f32(x, 'x'), ptr(x), B, H, Wd, C, ptr(W), W.stride(0), Co, f32p(bias, 'bias'), 1 if relu else 0,
                           ptr(gate), C if gate is not None else 0, _is_f32(gate, 'gate') if gate is not None else 1, ptr(y), Co, _is_f32(y, 'y'),
                           int(tile), stream(x))
    _check(rc, 'pk_conv3x3')
    return y


def maxpool2x2(x, B, H, Wd, C, y):
    """nn.MaxPool2d(2, 2) on pixel rows: x (B H Wd, C) -> y (B (H // 2) (Wd // 2), C), same element type"""
    assert x.dtype == y.dtype and x.is_contiguous() and y.is_contiguous() and x.numel() == B * H * Wd * C and y.numel() == B * (H // 2) * (Wd // 2) * C
    _check(load().pk_maxpool2x2(_is_f32(x, 'x'), ptr(x), B, H, Wd, C, ptr(y), stream(x)), 'pk_maxpool2x2')
    return y


def maxpool2x2_bwd(x, dy, B, H, Wd, C, dx):
    """dx (B H Wd, C) f32 <- dy (B (H // 2) (Wd // 2), C) f32 routed to the first maximum of every window of the saved input x"""
    assert x.is_contiguous() and x.numel() == B * H * Wd * C and dx.numel() == x.numel() and dy.numel() == B * (H // 2) * (Wd // 2) * C
    _check(load().pk_maxpool2x2_bwd(_is_f32(x, 'x'), ptr(x), f32p(dy, 'dy'), B, H, Wd, C, f32p(dx, 'dx'), stream(x)), 'pk_maxpool2x2_bwd')
    return dx


def adaptive_avgpool(x, B, H, Wd, C, out):
    """nn.AdaptiveAvgPool2d((7, 7)) on pixel rows: x (B H Wd, C) f32 / bf16 -> out (B 49, C) f32, rows (b, i, j)"""
    assert x.is_contiguous() and x.numel() == B * H * Wd * C and out.numel() == B * 49 * C
    _check(load().pk_adaptive_avgpool(_is_f32(x, 'x'), ptr(x), B, H, Wd, C, f32p(out, 'out'), stream(x)), 'pk_adaptive_avgpool')
    return out


def adaptive_avgpool_bwd(dy, B, H, Wd, C, dx):
    assert dy.numel() == B * 49 * C and dx.numel() == B * H * Wd * C
    _check(load().pk_adaptive_avgpool_bwd(f32p(dy, 'dy'), B, H, Wd, C, f32p(dx, 'dx'), stream(dy)), 'pk_adaptive_avgpool_bwd')
    return dx


class TorchPhilox:
    """where torch's device generator stands for ONE `uniform_` fill of `numel` float32 elements (ATen's launch geometry on this device):
    seed, Philox offset, thread stride; `.advance()` moves the generator past the fill exactly as the real op would"""

    def __init__(self, device, numel):
        idx = device.index if device.index is not None else torch.cuda.current_device()
        self.gen = torch.cuda.default_generators[idx]
        props = torch.cuda.get_device_properties(idx)
        blocks = min(props.multi_processor_count * (props.max_threads_per_multi_processor // 256), (numel + 255) // 256)
        self.stride = 256 * blocks
        self.seed = self.gen.initial_seed() & 0xFFFFFFFFFFFFFFFF
        self.offset = self.gen.get_offset()
        self.increment = ((numel - 1) // (self.stride * 4) + 1) * 4

    def advance(self):
        self.gen.set_offset(self.offset + self.increment)


def vocab_sample_philox(dtype, A, W, bias, M, V, D, temperature, rows, spec, need_lse, partials):
    rc = load().pk_vocab_sample_philox(dtype, ptr(A), A.stride(-2), ptr(W), W.stride(0), f32p(bias, 'to_logits.bias'), M, V, D, temperature, ptr(rows),
                                       spec.seed, spec.offset, spec.stride, 1 if need_lse else 0, ptr(partials), stream(A))
    _check(rc, 'pk_vocab_sample_philox')
