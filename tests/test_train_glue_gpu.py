"""The loss heads and glue kernels of the two training steps, each called directly and held element by element to the float64 restatements of
tests/train_glue_reference.py: pk_ce_grad_slab, pk_bce_head, pk_attn_train_prep / _bwd, pk_sqdiff_partials, pk_patch_frame_mask, pk_scaled_diff, pk_mul,
pk_sign, pk_leaky_bwd, pk_bias_gather / pk_bias_scatter and pk_reduce_multi.  Inputs come from seeded CPU generators; every output buffer is pre-filled with
NaN, so an element that was not written and an element written outside the output both show.  The checkers are the reference module's; what they reject is
shown in tests/test_train_glue_host.py.  Each test records its largest error / bound through tests.util.record_parity."""
import ctypes
import itertools

import pytest
import torch

from tests import train_glue_reference as R
from tests.util import record_parity

pytestmark = pytest.mark.gpu

NAN = float('nan')
EINVAL, EALIGN = -1, -2


@pytest.fixture(autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip('needs a GPU')
    torch.cuda.set_device(0)
    yield


def dev(t):
    return None if t is None else t.cuda()


def nan(*shape, dtype=torch.float32):
    return torch.full(shape, NAN, device='cuda', dtype=dtype)


def ptr(t):
    return None if t is None else t.data_ptr()


def one(v):
    return None if v is None else torch.tensor([v], device='cuda', dtype=torch.float32)


def column_slice(t, pad):
    """t as the LAST columns of a buffer `pad` columns wider, NaN in front (pad % 4 == 0 keeps the rows 16-byte aligned)"""
    if not pad:
        return t.cuda()
    buf = nan(t.shape[0], t.shape[1] + pad)
    buf[:, pad:] = t.cuda()
    return buf[:, pad:]


def merge(worst, new):
    for k, v in new.items():
        worst[k] = max(worst.get(k, 0.), v)


# ------------------------------------------------------------------------------------------------ pk_ce_grad_slab

@pytest.mark.parametrize('M,Vs,ldgt', R.CE_SHAPES)
def test_ce_grad_slab(M, Vs, ldgt):
    """every (v0, row pitch, rows gather, device scale) x (f32, bf16): g within its derived bound, gT its transpose bit for bit with zeroed pad columns,
    db the column sums of the stored g, nothing written outside"""
    from phenaki_pytorch_amd import _lib as L
    worst = {}
    for v0, wide, use_rows, use_dev in itertools.product((0, 192), (False, True), (False, True), (False, True)):
        c = R.ce_case(M, Vs, ldgt, v0, wide=wide, use_rows=use_rows, use_dev=use_dev)
        logits, lse, targets, rows, sd = dev(c['logits']), dev(c['lse']), dev(c['targets']), dev(c['rows']), one(c['dev'])
        f32 = None
        for dtype in (torch.float32, torch.bfloat16):
            g, gT, db = R.ce_buffers(c, dtype, 'cuda')
            L.ce_grad_slab(logits, lse, targets, rows, M, Vs, v0, c['scale'], g, gT, db=db, scale_dev=sd)
            out = (g.cpu(), gT.cpu(), db.cpu())
            merge(worst, R.ce_check(c, *out, f32_out=f32))
            if dtype == torch.float32:
                f32 = out[:2]
                g2, gT2, _ = R.ce_buffers(c, dtype, 'cuda')                          # without db: the same g
                L.ce_grad_slab(logits, lse, targets, rows, M, Vs, v0, c['scale'], g2, gT2, scale_dev=sd)
                R.assert_same_bits(g2.cpu(), out[0], 'ce_grad_slab without db')
    print(f'ce_grad_slab {M}x{Vs} ldgt {ldgt}: err / bound g {worst["g"]:.3f} db {worst["db"]:.3f}')
    record_parity('glue_ce_grad_slab', dict(shape=[M, Vs, ldgt], err_over_bound=worst))


def test_ce_grad_slab_loop_over_the_vocabulary():
    """slabs of 192 over V = 448 (the last one 64 wide), each on its own logits buffer as the trainer runs them: their g side by side is the single
    Vs = 448 call bit for bit, and every row of it sums to zero within sum_bound"""
    from phenaki_pytorch_amd import _lib as L
    M, V = 77, R.V_FULL
    c = R.ce_case(M, V, 96, 0, use_dev=True)
    lse, targets, sd = dev(c['lse']), dev(c['targets']), one(c['dev'])
    g, gT, db = R.ce_buffers(c, torch.float32, 'cuda')
    L.ce_grad_slab(dev(c['logits']), lse, targets, None, M, V, 0, c['scale'], g, gT, db=db, scale_dev=sd)
    whole = g.cpu()
    ratio = R.ce_check(c, whole, gT.cpu(), db.cpu())
    parts = []
    for v0 in range(0, V, 192):
        Vs = min(192, V - v0)
        cs = dict(c, Vs=Vs, v0=v0, ld=Vs, logits=c['logits'][:, v0:v0 + Vs].contiguous())
        gs, gTs, dbs = R.ce_buffers(cs, torch.float32, 'cuda')
        L.ce_grad_slab(dev(cs['logits']), lse, targets, None, M, Vs, v0, c['scale'], gs, gTs, db=dbs, scale_dev=sd)
        merge(ratio, R.ce_check(cs, gs.cpu(), gTs.cpu(), dbs.cpu()))
        R.assert_same_bits(dbs.cpu()[:Vs], db.cpu()[v0:v0 + Vs], f'db of the slab at {v0}')
        parts.append(gs.cpu())
    assert parts[-1].shape[1] == 64
    R.assert_same_bits(torch.cat(parts, 1), whole, 'the slabs side by side against the single call')
    w64 = whole.double()
    ratio['row_sum'] = R.assert_within(w64.sum(1), torch.zeros(M, dtype=torch.float64), R.sum_bound(w64.abs().sum(1), V), 'row sums of g over the vocabulary')
    record_parity('glue_ce_grad_slab_loop', dict(err_over_bound=ratio))


# ------------------------------------------------------------------------------------------------ pk_bce_head

def _bce_call(lib, L, c, e, w, b, labels, sd, bufs, M, D):
    logits, loss_rows, de, pw, pb = bufs
    return lib.pk_bce_head(e.data_ptr(), c['ld'], ptr(w), ptr(b), ptr(labels), c['scale'], ptr(sd), ptr(logits), ptr(loss_rows), ptr(de), c['ld'] if de is not None else 0,
                           ptr(pw), ptr(pb), M, D, L.stream(e))


@pytest.mark.parametrize('M,D', R.BCE_SHAPES)
def test_bce_head(M, D):
    """logits, loss rows, de and the dw / db partials on NaN-filled buffers (at M = 8200 the last 112 of the 1024 blocks own no row: zero partials),
    both row pitches, with and without bias and device scale; then the wrapper and the logits-only form"""
    from phenaki_pytorch_amd import _lib as L
    lib = L.load()
    worst = {}
    for wide, has_b, use_dev in itertools.product((False, True), (True, False), (False, True)):
        c = R.bce_case(M, D, wide=wide, has_b=has_b, use_dev=use_dev)
        e, w, b, labels, sd = dev(c['e']), dev(c['w']), dev(c['b']), dev(c['labels']), one(c['dev'])
        bufs = R.bce_buffers(c, 'cuda')
        assert _bce_call(lib, L, c, e, w, b, labels, sd, bufs, M, D) == 0
        logits, loss_rows, de, pw, pb = bufs
        P = pw.shape[0]
        dw = L.colsum(pw, P, D, nan(D))
        db = L.colsum(pb.view(P, 1), P, 1, nan(1))
        merge(worst, R.bce_check(c, logits.cpu(), loss_rows.cpu(), de.cpu(), pw.cpu(), pb.cpu(), dw.cpu(), db.cpu()))
        # the wrapper (its own partial buffers) gives the same bits
        lg2, lr2, de2 = nan(M + 1), nan(M + 1), nan(M, c['ld'])
        dw2, db2 = L.bce_head(e[:, :D], w, b, labels, M, D, scale=c['scale'], logits=lg2, loss_rows=lr2, de=de2[:, :D], scale_dev=sd)
        for got, want, what in ((lg2, logits, 'logits'), (lr2, loss_rows, 'loss_rows'), (de2, de, 'de'), (dw2, dw, 'dw'), (db2, db, 'db')):
            R.assert_same_bits(got.cpu(), want.cpu(), f'bce_head wrapper {what}')
        # labels = None: logits only, nothing else written, and a de is refused
        lg3 = nan(M + 1)
        assert L.bce_head(e[:, :D], w, b, None, M, D, logits=lg3) is None
        R.assert_same_bits(lg3.cpu(), logits.cpu(), 'bce_head logits without labels')
        only = (nan(M + 1), None, nan(M, c['ld']), None, None)
        assert _bce_call(lib, L, c, e, w, b, None, sd, only, M, D) == EINVAL, 'de without labels'
        R.assert_untouched(only[2], 'a refused call')
    print(f'bce_head {M}x{D}: err / bound {worst}')
    record_parity('glue_bce_head', dict(shape=[M, D], err_over_bound=worst))


def test_bce_head_refuses_bad_arguments():
    from phenaki_pytorch_amd import _lib as L
    lib = L.load()
    e, w, y = torch.zeros(4, 1028, device='cuda'), torch.zeros(1028, device='cuda'), torch.zeros(4, device='cuda')
    de, pw, pb, lg = nan(4, 1028), nan(1, 1028), nan(1), nan(4)
    call = lambda D, ld, de_, pw_, pb_: lib.pk_bce_head(e.data_ptr(), ld, w.data_ptr(), None, y.data_ptr(), 1.0, None, lg.data_ptr(), None, ptr(de_), ld, ptr(pw_), ptr(pb_),
                                                        4, D, L.stream(e))
    assert call(1024, 1028, de, pw, pb) == 0
    assert call(1028, 1028, de, pw, pb) == EINVAL, 'D beyond the 1024 columns a block holds'
    assert call(6, 1028, de, pw, pb) == EALIGN
    assert call(8, 1026, de, pw, pb) == EALIGN
    assert call(8, 1028, None, pw, pb) == EINVAL, 'dw partials without de'
    assert call(8, 1028, de, pw, None) == EINVAL, 'dw partials without db partials'


# ------------------------------------------------------------------------------------------------ pk_attn_train_prep / pk_attn_train_prep_bwd

@pytest.mark.parametrize('S,h,n,n_kv,nnull', R.PREP_SHAPES)
def test_attn_train_prep_and_backward(S, h, n, n_kv, nnull):
    """q / kv contiguous and as column slices of wider buffers, dq / dkv with NaN pad columns; the scale partials interleaved (the wrapper's (1024, 128)
    buffer) and as two (1024, 64) buffers; a zero q row and a zero k row.  (4, 8, 300, 300, 0): 19200 tasks on the backward's 1024 x 16 lanes"""
    from phenaki_pytorch_amd import _lib as L
    lib = L.load()
    c = R.prep_case(S, h, n, n_kv, nnull)
    inner, nkt = 64 * h, nnull + n_kv
    null_kv, qs, ks = dev(c['null_kv']), dev(c['q_scale']), dev(c['k_scale'])
    dQh, dKh, dVh = dev(c['dQh']), dev(c['dKh']), dev(c['dVh'])
    worst = {}
    for pad in (0, 64):
        q, kv = column_slice(c['q'], pad), column_slice(c['kv'], pad)
        Qh, Kh, Vh = nan(S * h, n, 64), nan(S * h, nkt, 64), nan(S * h, nkt, 64)
        L.attn_train_prep(q, kv, null_kv, qs, ks, c['scale'], Qh, Kh, Vh, S, h, n, n_kv, nnull)
        assert torch.isfinite(Qh).all() and torch.isfinite(Kh).all(), 'the zero rows'
        merge(worst, R.prep_check_fwd(c, Qh.cpu(), Kh.cpu(), Vh.cpu()))
        forms = {}
        for form in ('interleaved', 'separate'):
            dq, dkv = nan(S * n, inner + pad), nan(S * n_kv, 2 * inner + pad)
            dnull = nan(h, 2 * nnull, 64) if nnull else None
            if form == 'interleaved':
                pqk = nan(1024, 128)
                pq, pk, p_pq, p_pk = pqk[:, :64], pqk[:, 64:], pqk.data_ptr(), pqk.data_ptr() + 256
            else:
                pq, pk = nan(1024, 64), nan(1024, 64)
                p_pq, p_pk = pq.data_ptr(), pk.data_ptr()
            rc = lib.pk_attn_train_prep_bwd(q.data_ptr(), q.stride(0), kv.data_ptr(), kv.stride(0), ptr(null_kv), qs.data_ptr(), ks.data_ptr(), c['scale'],
                                            dQh.data_ptr(), dKh.data_ptr(), dVh.data_ptr(), dq.data_ptr(), dq.stride(0), dkv.data_ptr(), dkv.stride(0),
                                            p_pq, p_pk, ptr(dnull), S, h, n, n_kv, nnull, L.stream(q))
            assert rc == 0
            sums = L.colsum(torch.cat([pq, pk], 1).contiguous(), 1024, 128, nan(128)).cpu()
            forms[form] = (pq.cpu().contiguous(), pk.cpu().contiguous(), dq.cpu(), dkv.cpu())
            merge(worst, R.prep_check_bwd(c, dq.cpu(), dkv.cpu(), sums[:64], sums[64:], dnull.cpu() if nnull else None, pq=forms[form][0], pk=forms[form][1]))
        for a, b, what in zip(forms['interleaved'], forms['separate'], ('dq_scale partials', 'dk_scale partials', 'dq', 'dkv')):
            R.assert_same_bits(a, b, f'attn_train_prep_bwd {what}: interleaved against separate partial buffers')
        # the wrapper: the same dq / dkv, and sums within the same bounds
        dq, dkv = nan(S * n, inner + pad), nan(S * n_kv, 2 * inner + pad)
        dqs, dks, dnull = L.attn_train_prep_bwd(q, kv, null_kv, qs, ks, c['scale'], dQh, dKh, dVh, dq[:, :inner], dkv[:, :2 * inner], S, h, n, n_kv, nnull)
        R.assert_same_bits(dq.cpu(), forms['separate'][2], 'attn_train_prep_bwd wrapper dq')
        merge(worst, R.prep_check_bwd(c, dq.cpu(), dkv.cpu(), dqs.cpu(), dks.cpu(), dnull.cpu() if nnull else None))
    print(f'attn_train_prep {S, h, n, n_kv, nnull}: err / bound {worst}')
    record_parity('glue_attn_train_prep', dict(shape=[S, h, n, n_kv, nnull], err_over_bound=worst))


# ------------------------------------------------------------------------------------------------ pk_sqdiff_partials

@pytest.mark.parametrize('shape', R.SQDIFF_SHAPES)
def test_sqdiff_partials(shape):
    """(2, 3, 5, 8, 12): 720 float4 groups, 1021 idle blocks whose partial must be WRITTEN as zero; (1, 3, 6, 256, 256): 294912 groups, the second trip of the
    grid-stride loop.  Every frame mask of SQDIFF_MASKS"""
    from phenaki_pytorch_amd import _lib as L
    lib = L.load()
    worst = 0.
    for kind in R.SQDIFF_MASKS:
        c = R.sqdiff_case(shape, kind)
        a, b, m = dev(c['a']), dev(c['b']), dev(c['mask'])
        partials = nan(R.SQDIFF_BLOCKS, dtype=torch.float64)
        assert lib.pk_sqdiff_partials(a.data_ptr(), b.data_ptr(), ptr(m), *shape, partials.data_ptr(), L.stream(a)) == 0
        worst = max(worst, R.sqdiff_check(c, partials.cpu()))
        ref = R.sqdiff_ref(c)
        R.assert_within(L.sqdiff_sum(a, b, None if m is None else m.bool()).cpu(), ref, 8 * R.U * ref, f'sqdiff_sum wrapper ({kind})')
    print(f'sqdiff {shape}: err / bound {worst:.3f}')
    record_parity('glue_sqdiff_partials', dict(shape=list(shape), err_over_bound=worst))


def test_sqdiff_refuses_a_plane_that_is_no_multiple_of_four():
    from phenaki_pytorch_amd import _lib as L
    a, p = torch.zeros(12, device='cuda'), nan(R.SQDIFF_BLOCKS, dtype=torch.float64)
    assert L.load().pk_sqdiff_partials(a.data_ptr(), a.data_ptr(), None, 1, 1, 2, 2, 3, p.data_ptr(), L.stream(a)) == EALIGN
    R.assert_untouched(p, 'a refused call')


# ------------------------------------------------------------------------------------------------ pk_patch_frame_mask

@pytest.mark.parametrize('geom', list(R.FRAME_GEOMS))
@pytest.mark.parametrize('ph,pw', R.FRAME_PATCHES)
def test_patch_frame_mask(geom, ph, pw):
    """the image group, the video group (pt = 2) and pt = 3; the source holds NaN in every dropped frame, so a dropped element that is copied, multiplied or
    selected late shows; row pitches = P and > P on either side, and in place"""
    from phenaki_pytorch_amd import _lib as L
    c = R.frame_mask_case(geom, ph, pw)
    P, rows = c['P'], c['src'].shape[0]
    mask = dev(c['mask'])
    for lds_pad, ldd_pad, in_place in ((0, 0, False), (4, 4, False), (4, 0, False), (0, 8, False), (0, 0, True), (4, 4, True)):
        src, src_buf = R.strided(c['src'], lds_pad, 'cuda')
        dst_buf = src_buf if in_place else nan(rows, P + ldd_pad)
        assert L.patch_frame_mask(src, dst_buf[:, :P], mask, c['video_shape'], *c['geom']) is not None
        R.frame_mask_check(c, dst_buf.cpu())
        if not in_place:
            R.assert_same_bits(src_buf.cpu()[:, :P], c['src'], 'patch_frame_mask: the source')
    record_parity('glue_patch_frame_mask', dict(geom=geom, patch=[ph, pw], bit_exact=True, err_over_bound=0.))


# ------------------------------------------------------------------------------------------------ pk_scaled_diff, pk_mul, pk_sign, pk_leaky_bwd

@pytest.mark.parametrize('n', R.ELEMENTWISE_N)
def test_scaled_diff_mul_sign(n):
    """bit for bit against the same f32 expression.  The grid of these kernels is capped at 65535 blocks of 256 threads, so the second trip of their
    grid-stride loops is NOT reached by any test: pk_scaled_diff and pk_mul (a float4 per thread) would need more than 4 * 65535 * 256 floats = 268 MB per
    tensor, pk_sign and pk_leaky_bwd (a float per thread) more than 65535 * 256 floats = 67.1 MB per tensor, above the 64 MB a test tensor may take"""
    from phenaki_pytorch_amd import _lib as L
    a, b = torch.randn(n, generator=R.gen(20, n)), torch.randn(n, generator=R.gen(21, n))
    worst = 0.
    for dv in (None, 0.37):
        f32, ref, bound = R.scaled_diff_ref(a, b, 1.0 / 77, dv)
        out = nan(n + 4)
        L.scaled_diff(dev(a), dev(b), 1.0 / 77, out[:n], one(dv))
        R.assert_same_bits(out.cpu()[:n], f32, 'scaled_diff against (a - b) * (scale32 * dev32)')
        R.assert_untouched(out[n:], 'scaled_diff beyond n')
        worst = max(worst, R.assert_within(out.cpu()[:n], ref, bound, 'scaled_diff against float64, three roundings'))
    out = nan(n + 4)
    L.mul(dev(a), dev(b), out[:n])
    R.assert_same_bits(out.cpu()[:n], a * b, 'mul')
    R.assert_untouched(out[n:], 'mul beyond n')
    a2 = dev(a).clone()
    L.mul(a2, dev(b), a2)
    R.assert_same_bits(a2.cpu(), a * b, 'mul with out = a')
    z = R.sign_inputs(n)
    for value in (0.5, 1.0):
        out = nan(n + 4)
        L.sign(dev(z), out[:n], value)
        R.assert_same_bits(out.cpu()[:n], R.sign_ref(z, value), 'sign: z > 0 ? v : -v')
        R.assert_untouched(out[n:], 'sign beyond n')
    record_parity('glue_scaled_diff_mul_sign', dict(n=n, bit_exact=True, scaled_diff_err_over_three_roundings=worst))


def test_scaled_diff_and_mul_refuse_n_6():
    from phenaki_pytorch_amd import _lib as L
    lib = L.load()
    a, out = torch.ones(8, device='cuda'), nan(8)
    s = L.stream(a)
    assert lib.pk_scaled_diff(a.data_ptr(), a.data_ptr(), 1.0, None, out.data_ptr(), 6, s) == EALIGN
    assert lib.pk_mul(a.data_ptr(), a.data_ptr(), out.data_ptr(), 6, s) == EALIGN
    assert lib.pk_scaled_diff(a.data_ptr() + 4, a.data_ptr(), 1.0, None, out.data_ptr(), 4, s) == EALIGN
    R.assert_untouched(out, 'a refused call')
    assert lib.pk_sign(a.data_ptr(), 1.0, out.data_ptr(), 6, s) == 0, 'pk_sign has no alignment condition'
    R.assert_same_bits(out.cpu(), torch.tensor([1.] * 6 + [NAN] * 2), 'sign, n = 6')


@pytest.mark.parametrize('N', [1, 7, 64])
def test_leaky_bwd(N):
    """y with exact zeros of both signs (the slope branch), contiguous and with three different row pitches > N"""
    from phenaki_pytorch_amd import _lib as L
    for M in (1, 37):
        y, dy = R.leaky_case(M, N)
        want = R.leaky_from_output(y, dy, 0.1)
        for pads in ((0, 0, 0), (3, 1, 2)):
            (yv, _), (dyv, _), dz = R.strided(y, pads[0], 'cuda'), R.strided(dy, pads[1], 'cuda'), nan(M, N + pads[2])
            L.leaky_bwd(yv, dyv, dz[:, :N], M, N, 0.1)
            R.assert_same_bits(dz.cpu()[:, :N], want, f'leaky_bwd {M}x{N} pads {pads}')
            R.assert_untouched(dz[:, N:], 'leaky_bwd columns >= N')
    record_parity('glue_leaky_bwd', dict(N=N, bit_exact=True, err_over_bound=0.))


# ------------------------------------------------------------------------------------------------ pk_bias_gather / pk_bias_scatter

@pytest.mark.parametrize('dims', R.BIAS_DIMS)
@pytest.mark.parametrize('heads', R.BIAS_HEADS)
def test_bias_gather_and_scatter(dims, heads):
    """code / off as the trainer builds them; table pitch = heads and > heads; the gather bit for bit, the scatter (f32 atomics, any order) within sum_bound
    over the largest multiplicity of a table row, <gather(T), G> = <T, scatter(G)>, the pad columns of dtab untouched"""
    from phenaki_pytorch_amd import _lib as L
    from phenaki_pytorch_amd.train import _build_rel_table
    c = R.bias_case(dims, heads)
    _, code, off = _build_rel_table(dims, 'cuda')
    assert torch.equal(code.cpu().int(), c['code']) and int(off) == c['off'] and code.dtype == torch.int32
    worst = {}
    for pad in (0, 3):
        tab, _ = R.strided(c['tab'], pad, 'cuda')
        out = nan(heads, c['n'], c['n'])
        L.bias_gather(tab, code, c['off'], out, heads, c['n'])
        dtab = nan(c['Lt'], heads + pad)
        dtab[:, :heads] = 0.
        L.bias_scatter(dev(c['G']), code, c['off'], dtab[:, :heads], heads, c['n'])
        merge(worst, R.bias_check(c, out.cpu(), dtab.cpu()))
    record_parity('glue_position_bias', dict(dims=list(dims), heads=heads, err_over_bound=worst))


# ------------------------------------------------------------------------------------------------ pk_reduce_multi

def _reduce_jobs(c):
    sums = [(dev(p), p.shape[0], nan(p.shape[1]), p.shape[1] - 4) for p in c['sums']]                 # (part, S, out, E)
    cols = [(dev(s), s.shape[0], s.shape[1] - 4, nan(s.shape[1])) for s in c['cols']]                 # (src, M, N, out)
    return sums, cols


@pytest.mark.parametrize('nsum,ncol', R.REDUCE_COUNTS)
def test_reduce_multi(nsum, ncol):
    """every job of the one-launch form bit for bit the same job run alone (pk_sum_batch / pk_colsum_multi) and within sum_bound of float64; job sizes on both
    sides of the 256-float4 and 16-column block edges; then either list empty, which the header allows and the wrapper never sends"""
    from phenaki_pytorch_amd import _lib as L
    lib = L.load()
    c = R.reduce_case(nsum, ncol)
    sums, cols = _reduce_jobs(c)
    L.reduce_multi([(p, S, o[:E], E) for p, S, o, E in sums], [(s, M, N, o[:N]) for s, M, N, o in cols])
    souts, couts = [o.cpu() for _, _, o, _ in sums], [o.cpu() for _, _, _, o in cols]
    worst = R.reduce_check(c, souts, couts)
    for i, (p, S, _, E) in enumerate(sums):
        alone = nan(E + 4)
        L.sum_batch(p, S, alone[:E], E)
        R.assert_same_bits(souts[i], alone.cpu(), f'reduce_multi sum job {i} against pk_sum_batch')
    for i, (s, M, N, _) in enumerate(cols):
        alone = nan(N + 4)
        L.colsum_multi([(s, M, N, alone[:N])])
        R.assert_same_bits(couts[i], alone.cpu(), f'reduce_multi column job {i} against pk_colsum_multi')
    # one side empty
    s2, c2 = _reduce_jobs(c)
    sa = (L.SumJob * nsum)(*[L.SumJob(p.data_ptr(), o.data_ptr(), p.stride(0), E // 4, S, 0) for p, S, o, E in s2])
    ca = (L.ColsumJob * ncol)(*[L.ColsumJob(s.data_ptr(), o.data_ptr(), s.stride(0), M, N, 0, 1.0) for s, M, N, o in c2])
    st = L.stream(s2[0][0])
    assert lib.pk_reduce_multi(ctypes.addressof(sa), nsum, None, 0, st) == 0
    for i, (_, _, o, _) in enumerate(s2):
        R.assert_same_bits(o.cpu(), souts[i], f'reduce_multi without column jobs, sum job {i}')
    for _, _, _, o in c2:
        R.assert_untouched(o, 'reduce_multi without column jobs')
    assert lib.pk_reduce_multi(None, 0, ctypes.addressof(ca), ncol, st) == 0
    for i, (_, _, _, o) in enumerate(c2):
        R.assert_same_bits(o.cpu(), couts[i], f'reduce_multi without sum jobs, column job {i}')
    assert lib.pk_reduce_multi(None, 0, None, 0, st) == EINVAL
    assert lib.pk_reduce_multi(None, 1, ctypes.addressof(ca), ncol, st) == EINVAL
    record_parity('glue_reduce_multi', dict(jobs=[nsum, ncol], err_over_bound=worst))
