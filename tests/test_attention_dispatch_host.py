"""Which kernel wrapper every (dtype, n, self / cross, bias form, mask, flag) combination of attention.py reaches, with which
arguments and in which order -- on the CPU: the `_lib` wrappers the transformer blocks call are replaced by recorders for the
duration of a case, so the remaining host code (weight packing, LayerNorm folding, the caches, the dispatch itself) runs on CPU
tensors and no kernel is launched.  tests/golden/attention_dispatch.json keeps, per case, the wrapper names in order and a
SHA-256 digest of the whole record (every argument of every call, and what run() returned);

    python tests/test_attention_dispatch_host.py --record

regenerates that file from the attention.py of the checkout it runs in, and `--dump CASE` prints the whole record of a case, to
compare two checkouts when a digest differs.

A recorded call is [wrapper, {parameter: argument}]: the positional and keyword arguments bound to the wrapper's signature, an
argument that equals the parameter's default left out, so a default that is spelled out and one that is omitted record alike.
Python scalars are stored as they are (floats as 'F' + repr, None as null), tuples element-wise, a tensor as
'T<label> <shape> <dtype> <stride>' (18x64 float32 64,1) where <label> is the running
index of the first appearance of its data_ptr() in the case: equal labels are the same buffer (xq and xkv of a self-attention,
K^ / V^T coming back out of the kv_cache, the residual being the block's input, the cached weight image that is passed).  Every
labelled tensor is kept alive until the case ends, so the allocator cannot hand one address to two of them."""
import contextlib
import hashlib
import inspect
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import pytest  # noqa: E402
import torch  # noqa: E402

from phenaki_pytorch_amd import _lib as L  # noqa: E402
from phenaki_pytorch_amd import attention as A  # noqa: E402

FIXTURE = os.path.join(ROOT, 'tests', 'golden', 'attention_dispatch.json')
STUBBED = ('gemm', 'layernorm', 'qkv_attn', 'qkv_project', 'q_attn_cached', 'attn_prep', 'attn_fwd', 'attn_small', 'peg', 'cpb_input')
DIM, HEADS, DCTX, NCTX, S = 64, 2, 64, 12, 2
DT = {'f32': L.F32, 'bf16': L.BF16, 'bf16x3': L.BF16X3}
LENGTHS = (9, 16, 17, 64, 65, 128, 256)        # the edges of: small (<= 16), short fused (<= 64), table (>= 64), x3_lds (>= 128), 64-row pad (>= 256)
GRID = {9: (3, 3), 16: (4, 4), 17: (17,), 64: (8, 8), 65: (5, 13), 72: (8, 9), 128: (2, 8, 8), 256: (4, 8, 8)}      # prod == n
# position-bias amplitudes: with q_scale = k_scale = 1, scale = 8 the fixed-offset condition of Attention.run reads
# (2 * 8.125 + hi - lo) * 1.4427 < 64, true for hi - lo = 2 and false for hi - lo = 200
BIAS_SMALL, BIAS_BIG = 1., 100.
SIGNATURES = {k: inspect.signature(getattr(L, k)) for k in STUBBED}


@pytest.fixture(scope='module')
def built_lib():
    from phenaki_pytorch_amd import build
    build.build(verbose=False)
    return L.load()


class Recorder:
    def __init__(self):
        self.calls, self.labels, self.keep = [], {}, []

    def enc(self, v):
        if isinstance(v, torch.Tensor):
            lab = self.labels.setdefault(v.data_ptr(), len(self.labels))
            self.keep.append(v)
            return f'T{lab} {"x".join(map(str, v.shape))} {str(v.dtype)[6:]} {",".join(map(str, v.stride()))}'
        if isinstance(v, float):
            return 'F' + repr(v)
        if isinstance(v, (tuple, list)):
            return [self.enc(e) for e in v]
        if v is None or isinstance(v, (bool, int)):
            return v
        raise TypeError(f'unexpected argument {type(v)}')

    def stub(self, name):
        def call(*args, **kwargs):
            sig = SIGNATURES[name]
            given = sig.bind(*args, **kwargs).arguments
            self.calls.append([name, {k: self.enc(v) for k, v in given.items() if not _is_default(v, sig.parameters[k].default)}])
            return kwargs.get('C')
        return call


def _is_default(v, default):
    return not isinstance(v, torch.Tensor) and type(v) is type(default) and v == default


def _noop(*args, **kwargs):
    return kwargs.get('C')


def _bias_values(self, dims):
    """ContinuousPositionBias._compute for the cases: the stubbed GEMMs would leave it uninitialised, and its extremes feed score_bound"""
    n = 1
    for d in dims:
        n *= d
    gen = torch.Generator().manual_seed(1234 + n)
    heads = self.net[-1].weight.shape[0]
    return torch.randint(-8, 9, (heads, n, n), generator=gen).float() * (self.amplitude / 8)


@contextlib.contextmanager
def patched(rec=None, **flags):
    """the stubbed wrappers (recording into `rec`, or no-ops), the deterministic position bias and the module flags of a case"""
    saved = [(L, k, getattr(L, k)) for k in STUBBED + ('require_device',)]
    saved += [(A.ContinuousPositionBias, '_compute', A.ContinuousPositionBias._compute)]
    saved += [(A, k, getattr(A, k)) for k in flags]
    try:
        for k in STUBBED:
            setattr(L, k, rec.stub(k) if rec is not None else _noop)
        L.require_device = lambda t, name='tensor': None           # the forward() entry points refuse CPU tensors
        A.ContinuousPositionBias._compute = _bias_values
        for k, v in flags.items():
            setattr(A, k, v)
        with torch.no_grad():
            yield
    finally:
        for obj, k, v in saved:
            setattr(obj, k, v)


# --------------------------------------------------------------------------- what a case runs

def _grid(n):
    return GRID[n]


def _cpb(n, amplitude):
    m = A.ContinuousPositionBias(dim=16, heads=HEADS, num_dims=len(_grid(n)))
    m.amplitude = amplitude
    return m


def _bias(kind, n):
    if kind is None:
        return None
    if kind == 'full':
        return torch.zeros(HEADS, n, n)
    if kind == 'strided':
        return torch.zeros(HEADS, n, 2 * n)[:, :, ::2]
    return _cpb(n, BIAS_BIG if kind == 'spec_big' else BIAS_SMALL).spec(*_grid(n))


def attn_run(dt, n, *, causal=False, kmask=False, bias=None, cross=False, nnull=0, norm_context=True, cache=False, calls=1,
             xt=False, want_t=False, dup=1, beta=0.):
    dtype = DT[dt]
    torch.manual_seed(0)
    if cross:
        att = A.Attention(DIM, dim_context=DCTX, heads=HEADS, num_null_kv=nnull, norm_context=norm_context).eval()
    else:
        att = A.Attention(DIM, heads=HEADS, causal=causal).eval()
    if beta:
        att.norm.beta.fill_(beta)
    x = torch.zeros(S * n, DIM)
    kw = dict(attn_bias=_bias(bias, n), want_t=want_t, dup=dup)
    if cross:
        kw.update(context2d=torch.zeros(S * NCTX, DCTX), n_ctx=NCTX)
        if cache:
            kw['kv_cache'] = {}
    if kmask:
        kw['kmask'] = torch.ones(S, NCTX if cross else n, dtype=torch.uint8)
    if xt:
        kw['xt'] = x.to(L.tdtype(dtype))
    return [att.run(x, S, n, dtype, **kw) for _ in range(calls)]


def ff_run(dt, rows, *, xt=False, want_t=False, stats=False):
    dtype = DT[dt]
    torch.manual_seed(0)
    ff = A.FeedForward(DIM).eval()
    x = torch.zeros(rows, DIM)
    return ff.run(x, dtype, xt=x.to(L.tdtype(dtype)) if xt else None, want_t=want_t,
                  stats=torch.zeros(rows, (DIM + 31) // 32, 2) if stats else None)


def peg_run(*, causal=False, want_t=False):
    torch.manual_seed(0)
    peg = A.PEG(DIM, causal=causal).eval()
    return peg.run(torch.zeros(S * 2 * 3 * 3, DIM), (S, 2, 3, 3), want_t=want_t)


def _transformer(peg, cross, depth=2):
    torch.manual_seed(0)
    return A.Transformer(DIM, depth=depth, dim_context=DCTX, heads=HEADS, peg=peg, has_cross_attn=cross, attn_num_null_kv=2).eval()


def tf_run(dt, n, *, peg=False, cross=False, context=None, replicas=1, bias=None, self_mask=False, ctx_mask=False, cache=False,
           calls=1, out=False, out_t=False, perm=(0, 0), skip_norm_out=False, xt=False):
    dtype = DT[dt]
    context = cross if context is None else context
    tf = _transformer(peg, cross)
    x = torch.zeros(S // replicas * n, DIM)
    g = _grid(n)
    kw = dict(video_shape=(S, *((1,) * (3 - len(g))), *g), attn_bias=_bias(bias, n), perm=perm, skip_norm_out=skip_norm_out, replicas=replicas)
    if context:
        kw.update(context2d=torch.zeros(S * NCTX, DCTX), n_ctx=NCTX)
    if cache:
        kw['kv_cache'] = {}
    if self_mask:
        kw['self_attn_mask'] = torch.ones(S, n, dtype=torch.uint8)
    if ctx_mask:
        kw['cross_attn_context_mask'] = torch.ones(S, NCTX, dtype=torch.uint8)
    if out:
        kw['out'] = torch.zeros(S * n, DIM)
    if out_t:
        kw['out_t'] = torch.zeros(S * n, DIM, dtype=L.tdtype(dtype))
    if xt:
        kw['xt'] = x.to(L.tdtype(dtype))
    return [tf.run(x, S, n, dtype, **kw) for _ in range(calls)]


def forward_run(which, dt):
    torch.manual_seed(0)
    if which == 'attention':
        m = A.Attention(DIM, dim_context=DCTX, heads=HEADS, num_null_kv=2).eval()
        args = (torch.zeros(S, 64, DIM),)
        kw = dict(mask=torch.ones(S, NCTX, dtype=torch.bool), context=torch.zeros(S, NCTX, DCTX))
    elif which == 'attention_bias':
        m = A.Attention(DIM, heads=HEADS).eval()
        args, kw = (torch.zeros(S, 65, DIM),), dict(attn_bias=torch.zeros(HEADS, 65, 65))
    elif which == 'ff':
        m, args, kw = A.FeedForward(DIM).eval(), (torch.zeros(S, 64, DIM),), {}
    elif which == 'peg':
        m, args, kw = A.PEG(DIM).eval(), (torch.zeros(S, 2, 3, 3, DIM),), {}
    elif which == 'peg_3d':
        m, args, kw = A.PEG(DIM).eval(), (torch.zeros(S, 18, DIM),), dict(shape=(S, 2, 3, 3))
    else:
        m = _transformer(True, True)
        args = (torch.zeros(S, 64, DIM),)
        kw = dict(video_shape=(S, 1, 8, 8), attn_bias=torch.zeros(HEADS, 64, 64), context=torch.zeros(S, NCTX, DCTX),
                  self_attn_mask=torch.ones(S, 64, dtype=torch.bool), cross_attn_context_mask=torch.ones(S, NCTX, dtype=torch.bool))
    A.set_compute_dtype(m, dt)
    return m(*args, **kw)


# --------------------------------------------------------------------------- the cases: name -> (function, arguments, module flags)

CASES = {}


def case(name, fn, *args, flags=None, **kw):
    assert name not in CASES, name
    CASES[name] = (fn, args, kw, flags or {})


def _cases():
    for dt in DT:
        for n in LENGTHS:
            case(f'self/{dt}/n{n}/plain', attn_run, dt, n)
            case(f'self/{dt}/n{n}/spec', attn_run, dt, n, bias='spec')
        for n in (65, 128):
            case(f'self/{dt}/n{n}/spec_big', attn_run, dt, n, bias='spec_big')
        for n in (9, 64, 128):
            case(f'self/{dt}/n{n}/causal', attn_run, dt, n, causal=True)
            case(f'self/{dt}/n{n}/kmask', attn_run, dt, n, kmask=True)
            case(f'self/{dt}/n{n}/full_bias', attn_run, dt, n, bias='full')
            case(f'self/{dt}/n{n}/strided_bias', attn_run, dt, n, bias='strided')
        case(f'self/{dt}/n128/spec_kmask', attn_run, dt, 128, bias='spec', kmask=True)
        case(f'self/{dt}/n64/beta_nonzero', attn_run, dt, 64, beta=0.1)
        # cross-attention
        for nnull in (0, 2):
            case(f'cross/{dt}/n64/null{nnull}/nocache', attn_run, dt, 64, cross=True, nnull=nnull, kmask=True)
            case(f'cross/{dt}/n64/null{nnull}/cache', attn_run, dt, 64, cross=True, nnull=nnull, cache=True, calls=2, kmask=True)
        case(f'cross/{dt}/n72/null2/cache', attn_run, dt, 72, cross=True, nnull=2, cache=True, calls=2)
        case(f'cross/{dt}/n72/null0/nocache', attn_run, dt, 72, cross=True)
        case(f'cross/{dt}/n64/null2/identity_norm/nocache', attn_run, dt, 64, cross=True, nnull=2, norm_context=False)
        case(f'cross/{dt}/n64/null2/identity_norm/cache', attn_run, dt, 64, cross=True, nnull=2, norm_context=False, cache=True, calls=2)
        case(f'cross/{dt}/n9/null2/cache', attn_run, dt, 9, cross=True, nnull=2, cache=True, calls=2)
        # Attention.run arguments
        for xt in (False, True):
            for want_t in (False, True, 'stats'):
                for dup in (1, 2):
                    case(f'args/{dt}/n128/xt{int(xt)}/want_{want_t}/dup{dup}', attn_run, dt, 128, xt=xt, want_t=want_t, dup=dup)
        case(f'args/{dt}/n64/xt1/want_stats/dup2', attn_run, dt, 64, xt=True, want_t='stats', dup=2)
        case(f'args/{dt}/cross/n64/xt1/want_stats', attn_run, dt, 64, cross=True, nnull=2, cache=True, calls=2, xt=True, want_t='stats')

    # flags, each where it changes the route
    off = dict(_LN_FOLD=False)
    for n in LENGTHS:
        case(f'flag/LN_FOLD0/bf16/n{n}/plain', attn_run, 'bf16', n, flags=off)
    for n in (9, 64):
        case(f'flag/LN_FOLD0/bf16x3/n{n}/plain', attn_run, 'bf16x3', n, flags=off)
        case(f'flag/LN_FOLD0/bf16/n{n}/kmask', attn_run, 'bf16', n, kmask=True, flags=off)
        case(f'flag/LN_FOLD0/bf16/n{n}/strided_bias', attn_run, 'bf16', n, bias='strided', flags=off)
        case(f'flag/LN_FOLD0/bf16/n{n}/causal', attn_run, 'bf16', n, causal=True, flags=off)
    case('flag/LN_FOLD0/bf16/n128/spec', attn_run, 'bf16', 128, bias='spec', flags=off)
    case('flag/LN_FOLD0/bf16/n128/want_stats', attn_run, 'bf16', 128, want_t='stats', flags=off)
    for dt in ('bf16', 'bf16x3'):
        case(f'flag/LN_FOLD0/{dt}/cross/n64/cache', attn_run, dt, 64, cross=True, nnull=2, cache=True, calls=2, kmask=True, flags=off)
        case(f'flag/LN_FOLD0/{dt}/cross/n64/nocache', attn_run, dt, 64, cross=True, nnull=2, flags=off)
    offx = dict(_LN_FOLD_X3=False)
    for n in (9, 16, 17, 64, 128):
        case(f'flag/LN_FOLD_X3_0/bf16x3/n{n}/plain', attn_run, 'bf16x3', n, flags=offx)
    case('flag/LN_FOLD_X3_0/bf16x3/n128/spec', attn_run, 'bf16x3', 128, bias='spec', flags=offx)
    case('flag/LN_FOLD_X3_0/bf16x3/cross/n64/cache', attn_run, 'bf16x3', 64, cross=True, nnull=2, cache=True, calls=2, flags=offx)
    case('flag/LN_FOLD_X3_0/bf16/n64/plain', attn_run, 'bf16', 64, flags=offx)
    for dt in ('bf16', 'bf16x3'):
        for n in (9, 64):
            case(f'flag/SHORT_FUSED0/{dt}/n{n}/plain', attn_run, dt, n, flags=dict(_SHORT_FUSED=False))
        case(f'flag/SHORT_FUSED0/{dt}/n64/spec', attn_run, dt, 64, bias='spec', flags=dict(_SHORT_FUSED=False))
        case(f'flag/CROSS_FUSED0/{dt}/cross/n64/cache', attn_run, dt, 64, cross=True, nnull=2, cache=True, calls=2, flags=dict(_CROSS_FUSED=False))
        case(f'flag/BIAS_TABLE0/{dt}/n128/spec', attn_run, dt, 128, bias='spec', flags=dict(_BIAS_TABLE=False))
        case(f'flag/ATTN_FIXED0/{dt}/n128/plain', attn_run, dt, 128, flags=dict(_ATTN_FIXED=False))
        case(f'flag/ATTN_FIXED0/{dt}/n128/spec', attn_run, dt, 128, bias='spec', flags=dict(_ATTN_FIXED=False))
    case('flag/SHORT_FUSED0+LN_FOLD0/bf16/n64/plain', attn_run, 'bf16', 64, flags=dict(_SHORT_FUSED=False, _LN_FOLD=False))

    # FeedForwardSeq.run / PEG.run
    for dt in DT:
        for mode in (0, 1, 2):
            fl = dict(_LN_FOLD_FF=mode)
            case(f'ff/{dt}/mode{mode}/bare', ff_run, dt, 24, flags=fl)
            case(f'ff/{dt}/mode{mode}/xt_stats_want_t', ff_run, dt, 24, xt=True, want_t=True, stats=True, flags=fl)
        case(f'ff/{dt}/max_rows', ff_run, dt, 24, xt=True, stats=True, flags=dict(_LN_FOLD_FF_MAX_ROWS=16))
    case('ff/bf16/LN_FOLD0', ff_run, 'bf16', 24, want_t=True, flags=off)
    for causal in (False, True):
        for want_t in (False, True):
            case(f'peg/causal{int(causal)}/want_t{int(want_t)}', peg_run, causal=causal, want_t=want_t)

    # Transformer.run, depth 2
    for dt in DT:
        for peg in (False, True):
            for cross in (False, True):
                case(f'tf/{dt}/n64/peg{int(peg)}/cross{int(cross)}', tf_run, dt, 64, peg=peg, cross=cross)
        case(f'tf/{dt}/n64/full', tf_run, dt, 64, peg=True, cross=True, bias='spec', self_mask=True, ctx_mask=True, cache=True, calls=2)
        case(f'tf/{dt}/n128/spec', tf_run, dt, 128, peg=True, cross=True, bias='spec', cache=True, calls=2)
        case(f'tf/{dt}/n64/cross_layers_no_context', tf_run, dt, 64, cross=True, context=False)
        case(f'tf/{dt}/n9/perm_out', tf_run, dt, 9, peg=True, perm=(2, 9), out=True)
        case(f'tf/{dt}/n9/perm_out_t', tf_run, dt, 9, peg=True, perm=(2, 9), out_t=True)
        case(f'tf/{dt}/n9/out_both', tf_run, dt, 9, out=True, out_t=True)
        case(f'tf/{dt}/n64/skip_norm_out', tf_run, dt, 64, cross=True, skip_norm_out=True)
        case(f'tf/{dt}/n64/xt', tf_run, dt, 64, cross=True, xt=True)
        case(f'tf/{dt}/n64/peg/xt', tf_run, dt, 64, peg=True, xt=True)
        for mode in (0, 1, 2):
            case(f'tf/{dt}/n64/ff_mode{mode}', tf_run, dt, 64, peg=True, cross=True, flags=dict(_LN_FOLD_FF=mode))
            case(f'tf/{dt}/n64/ff_mode{mode}/self_only', tf_run, dt, 64, flags=dict(_LN_FOLD_FF=mode))
        case(f'tf/{dt}/n64/ff_max_rows', tf_run, dt, 64, peg=True, cross=True, flags=dict(_LN_FOLD_FF_MAX_ROWS=16))
    for dt in ('bf16', 'bf16x3'):
        for peg in (False, True):
            case(f'tf/{dt}/n64/peg{int(peg)}/replicas2', tf_run, dt, 64, peg=peg, cross=True, replicas=2, bias='spec', cache=True)
            case(f'tf/{dt}/n64/peg{int(peg)}/replicas1_doubled', tf_run, dt, 64, peg=peg, cross=True, bias='spec', cache=True)
        case(f'tf/{dt}/n128/replicas2', tf_run, dt, 128, peg=True, cross=True, replicas=2, bias='spec', cache=True, calls=2)
        case(f'tf/{dt}/n64/LN_FOLD0', tf_run, dt, 64, peg=True, cross=True, bias='spec', cache=True, calls=2, flags=off)

    # module forward entry points (plain tensor in, plain tensor out)
    for which in ('attention', 'attention_bias', 'ff', 'peg', 'peg_3d', 'transformer'):
        for dt in ('fp32', 'bf16'):
            case(f'forward/{which}/{dt}', forward_run, which, dt)


_cases()


def run_case(name):
    fn, args, kw, flags = CASES[name]
    rec = Recorder()
    with patched(rec, **flags):
        ret = fn(*args, **kw)
        return {'calls': rec.calls, 'returns': rec.enc(ret)}


# --------------------------------------------------------------------------- every branch the cases have to reach

def _has(name, pred=lambda p: True):
    return lambda calls: any(c[0] == name and pred(c[1]) for c in calls)


def _seq(*names):
    return lambda calls: any([c[0] for c in calls[i:i + len(names)]] == list(names) for i in range(len(calls)))


BRANCHES = {
    'qkv_attn, LayerNorm folded': _has('qkv_attn', lambda p: p.get('q_ln_s') is not None),
    'qkv_attn behind a LayerNorm launch': _seq('layernorm', 'qkv_attn'),
    'qkv_attn with a bias': _has('qkv_attn', lambda p: p.get('bias') is not None),
    'qkv_attn causal': _has('qkv_attn', lambda p: p.get('causal') is True and p.get('slopes') is not None),
    'attn_small': _has('attn_small'),
    'q_attn_cached': _has('q_attn_cached'),
    'q_attn_cached with a key mask': _has('q_attn_cached', lambda p: p.get('kmask') is not None),
    'qkv_project self, folded': _has('qkv_project', lambda p: p.get('xkv') is not None and p.get('q_ln_s') is not None),
    'qkv_project self, unfolded': _has('qkv_project', lambda p: p.get('xkv') is not None and p.get('q_ln_s') is None),
    'qkv_project cached cross, folded': _has('qkv_project', lambda p: p.get('xkv') is None and p.get('q_ln_s') is not None),
    'qkv_project cached cross, unfolded': _has('qkv_project', lambda p: p.get('xkv') is None and p.get('q_ln_s') is None),
    'q GEMM with the folded LayerNorm': _has('gemm', lambda p: p.get('ln') is not None and 'act' not in p),
    'attn_prep q and k|v': _has('attn_prep', lambda p: p.get('kv') is not None),
    'attn_prep q only (cached k|v)': _has('attn_prep', lambda p: p.get('kv') is None),
    'attn_prep with null keys': _has('attn_prep', lambda p: p.get('nnull') == 2),
    'context_norm launch': _seq('layernorm', 'gemm', 'attn_prep'),
    'attn_fwd bias table + fixed offset': _has('attn_fwd', lambda p: p.get('bias_table') is not None and p.get('score_bound') is not None),
    'attn_fwd bias table, running max (bf16)': _has('attn_fwd', lambda p: p.get('dtype') == L.BF16 and p.get('bias_table') is not None and p.get('score_bound') is None),
    'attn_fwd fixed offset, no bias': _has('attn_fwd', lambda p: p.get('bias_table') is None and p.get('bias') is None and p.get('score_bound') is not None),
    'attn_fwd full bias': _has('attn_fwd', lambda p: p.get('bias') is not None and p.get('bias').endswith(',1')),
    'attn_fwd strided bias': _has('attn_fwd', lambda p: p.get('bias') is not None and p.get('bias').endswith(',2')),
    'attn_fwd key mask': _has('attn_fwd', lambda p: p.get('kmask') is not None),
    'attn_fwd causal': _has('attn_fwd', lambda p: p.get('causal') is True and p.get('slopes') is not None),
    'attn_fwd f32': _has('attn_fwd', lambda p: p.get('dtype') == L.F32),
    'attn_fwd split-bf16': _has('attn_fwd', lambda p: p.get('dtype') == L.BF16X3),
    'to_out with a bf16 copy': _has('gemm', lambda p: p.get('res') is not None and p.get('C2') is not None),
    'to_out with row statistics': _has('gemm', lambda p: p.get('stats_out') is not None),
    'to_out written twice': _has('gemm', lambda p: 'dup_rows' in p),
    'FF1 folded, statistics handed over': _has('gemm', lambda p: p.get('act') == L.ACT_GEGLU and p.get('ln_stats') is not None),
    'FF1 folded, own statistics': _has('gemm', lambda p: p.get('act') == L.ACT_GEGLU and p.get('ln') is not None and p.get('ln_stats') is None),
    'FF1 behind a LayerNorm launch': _has('gemm', lambda p: p.get('act') == L.ACT_GEGLU and p.get('ln') is None),
    'LayerNorm with the raw bf16 copy': _has('layernorm', lambda p: p.get('raw') is not None),
    'norm_out with a row permutation': _has('layernorm', lambda p: p.get('perm') == [2, 9] and p.get('out2') is not None),
    'norm_out into out_t only': _has('layernorm', lambda p: p.get('perm') == [2, 9] and p.get('out') is not None and p.get('out2') is None),
    'PEG with a bf16 copy': _has('peg', lambda p: p.get('out_t') is not None),
    'PEG on half a CFG batch': _has('peg', lambda p: p.get('B') == S // 2),
}
# the split-bf16 table that no single exponent offset covers falls back to the full matrix on the running-max kernel
X3_FALLBACK = ('self/bf16x3/n128/spec_big', 'flag/ATTN_FIXED0/bf16x3/n128/spec')


def summary(r):
    """what the fixture keeps of a case: the wrapper names in order, and a digest of the whole record (arguments and returns)"""
    blob = json.dumps(r, separators=(',', ':')).encode()
    return [' '.join(c[0] for c in r['calls']), hashlib.sha256(blob).hexdigest()[:16]]


@pytest.fixture(scope='module')
def golden():
    with open(FIXTURE) as f:
        return json.load(f)


@pytest.fixture(scope='module')
def recorded(built_lib):
    return {name: run_case(name) for name in CASES}


@pytest.mark.parametrize('name', list(CASES))
def test_dispatch_matches_the_recorded_calls(recorded, golden, name):
    got = summary(recorded[name])
    assert got[0] == golden[name][0]
    assert got[1] == golden[name][1], 'same wrappers, other arguments; this checkout records (compare with --dump on the old one):\n' + \
        '\n'.join(json.dumps(c) for c in recorded[name]['calls']) + '\nreturns ' + json.dumps(recorded[name]['returns'])


def test_cases_reach_every_wrapper_and_branch(recorded, golden):
    assert set(golden) == set(CASES)
    lists = [c['calls'] for c in recorded.values()]
    for name in STUBBED:
        if name != 'cpb_input':          # (only ContinuousPositionBias._compute calls it, which the cases replace)
            assert any(_has(name)(calls) for calls in lists), f'no case reaches {name}'
    for branch, pred in BRANCHES.items():
        assert any(pred(calls) for calls in lists), f'no case reaches: {branch}'
    for name in X3_FALLBACK:
        fwd = [c for c in recorded[name]['calls'] if c[0] == 'attn_fwd']
        assert len(fwd) == 1 and fwd[0][1].get('bias') is not None and 'bias_table' not in fwd[0][1] and 'score_bound' not in fwd[0][1]
    # attn_small exists in f32 and (LayerNorm not folded) split-bf16, never in bf16
    assert _has('attn_small')(recorded['flag/LN_FOLD_X3_0/bf16x3/n9/plain']['calls'])
    assert not any(_has('attn_small')(c['calls']) for k, c in recorded.items() if '/bf16/' in k)
    # the public run() methods return a plain tensor unless asked for more
    assert isinstance(recorded['self/bf16/n64/plain']['returns'][0], str)
    assert len(recorded['args/bf16/n128/xt0/want_True/dup1']['returns'][0]) == 2
    assert len(recorded['args/bf16/n128/xt0/want_stats/dup1']['returns'][0]) == 3


def test_the_wrappers_come_back(built_lib):
    before = {k: getattr(L, k) for k in STUBBED}
    flag = A._LN_FOLD
    run_case('flag/LN_FOLD0/bf16/n64/plain')
    assert all(getattr(L, k) is before[k] for k in STUBBED) and A._LN_FOLD is flag


def test_shares_cfg_prefix_refusals():
    x, ctx, mask = torch.zeros(S * 64, DIM), torch.zeros(S * NCTX, DCTX), torch.ones(S, 64, dtype=torch.uint8)
    tf = _transformer(True, True)
    assert tf.shares_cfg_prefix(L.BF16, ctx, None) and tf.shares_cfg_prefix(L.BF16X3, ctx, None)
    # 1. the shared prefix is switched off, or the dtype does not thread the folded path
    assert not tf.shares_cfg_prefix(L.F32, ctx, None)
    for flag in ('_CFG_SHARED_PREFIX', '_LN_FOLD'):
        with patched(**{flag: False}):
            assert not tf.shares_cfg_prefix(L.BF16, ctx, None)
    with patched(_LN_FOLD_X3=False):
        assert not tf.shares_cfg_prefix(L.BF16X3, ctx, None) and tf.shares_cfg_prefix(L.BF16, ctx, None)
    # 2. no cross-attention will run in layer 0
    assert not tf.shares_cfg_prefix(L.BF16, None, None)
    assert not _transformer(True, False).shares_cfg_prefix(L.BF16, ctx, None)
    # 3. a per-sequence self-attention mask
    assert not tf.shares_cfg_prefix(L.BF16, ctx, mask)
    with patched(), pytest.raises(AssertionError, match='shares_cfg_prefix'):
        tf.run(x[:64], S, 64, L.F32, video_shape=(S, 1, 8, 8), context2d=ctx, n_ctx=NCTX, replicas=2)


def record():
    from phenaki_pytorch_amd import build
    build.build(verbose=False)
    out = {name: summary(run_case(name)) for name in CASES}
    with open(FIXTURE, 'w') as f:
        f.write('{\n' + ',\n'.join(f' {json.dumps(k)}: {json.dumps(v)}' for k, v in out.items()) + '\n}\n')
    print(f'{len(out)} cases -> {FIXTURE}')


if __name__ == '__main__':
    if sys.argv[1:] == ['--record']:
        record()
    elif len(sys.argv) == 3 and sys.argv[1] == '--dump':
        r = run_case(sys.argv[2])
        print('\n'.join(json.dumps(c) for c in r['calls']) + '\nreturns ' + json.dumps(r['returns']))
    else:
        raise SystemExit('usage: python tests/test_attention_dispatch_host.py --record | --dump CASE')
