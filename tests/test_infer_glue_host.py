"""tests/infer_glue_reference.py on its own, no kernel launched: (1) every restatement in float64 against the project's oracle or a torch function; (2) every
checker fed its own reference rounded to f32 and an f32 evaluation of the formula in two summation orders, which it must accept: the bound is not tighter than
f32 arithmetic allows; (3) every checker fed a named wrong kernel, which it must reject: a checker that cannot fail is itself a failure; (4) the 1 % cap on LFQ
projections near zero and the measured allowance of the two transcendental kernels.  The second-pass shapes of the GPU tests (tens of MB each) are left to the
GPU tests: their checkers are the ones exercised here."""
import pytest
import torch
import torch.nn.functional as F

from oracle import phenaki_oracle as O
from tests import infer_glue_reference as R

NAN = float('nan')


def rejects(fn, what):
    try:
        fn()
    except AssertionError:
        return what
    pytest.fail(f'the checker accepted a wrong kernel: {what}')


# ------------------------------------------------------------------------------------------------ the restatements against the oracle / torch

def test_layernorm_restatement_is_torch_layer_norm():
    for D in R.LN_D:
        c = R.ln_case(5, D, R.LN_VARIANTS[0])
        x = c['x'][:, :D].double()
        y, bound = R.ln_ref(x, c['gamma'], c['beta'])
        want = F.layer_norm(x, (D,), c['gamma'].double(), c['beta'].double(), R.LN_EPS)
        assert (y - want).abs().max() <= 1e-12 * want.abs().max()
        assert (bound >= 0).all()


def test_peg_restatement_is_the_oracle_convolution():
    for causal in (False, True):
        for shape in [(2, 5, 8, 3, 4), (2, 1, 1, 1, 4), (2, 2, 2, 17, 8)]:
            c = R.peg_case(*shape, causal)
            B, T, H, W, D = shape
            sd = {'p.dsconv.weight': c['wt'].double().t().reshape(D, 1, 3, 3, 3).contiguous(), 'p.dsconv.bias': c['bias'].double()}
            want = O.peg(sd, 'p.', c['x'].double().reshape(B, T * H * W, D), (B, T, H, W), causal).reshape(shape)
            got = R.peg_eval(c, residual=False)
            assert (got - want).abs().max() <= 1e-12 * want.abs().max()
            assert (R.peg_eval(c) - (got + c['x'].double())).abs().max() <= 1e-12 * want.abs().max()          # + the residual


def test_lfq_restatements_are_the_oracle_quantizer():
    c = R.lfq_enc_case(777, 256, 13)
    sd = {'vq.project_in.weight': c['wp'].double(), 'vq.project_in.bias': c['bp'].double()}
    P, pb = R.lfq_enc_ref(c)
    want = O.lfq_project(sd, c['x'][:, :256].double())
    assert (P - want).abs().max() <= 1e-12
    assert torch.equal(R.lfq_ids_of(P > 0), O.lfq_ids(want))
    assert torch.equal(R.lfq_bits(R.lfq_ids_of(P > 0), 13), (P > 0).long())
    for case in R.DECODE_CASES:
        d = R.decode_case(*case)
        if d['cd'] > 52:
            continue                                              # the oracle's float mask is exact to 2^53
        sd = {'vq.project_in.weight': torch.zeros(d['cd'], 1), 'vq.project_out.weight': d['wo'], 'vq.project_out.bias': d['bo']}
        want = O.lfq_codes(sd, d['flat']).double()                # the oracle works in f32: both sides carry cd roundings
        absum = d['wo'].double().abs().sum(1) + d['bo'].double().abs()
        R.assert_within(R.decode_ref(d), want, R.sum_bound(absum, 2 * d['cd'] + 2, extra=0)[None].expand_as(want), 'decode_ref against the oracle')


def test_cpb_restatement_is_the_oracle_input_layer():
    for dims, D in R.CPB_CASES:
        c = R.cpb_case(dims, D)
        sd = {'p.net.0.weight': c['w0'].double(), 'p.net.0.bias': c['b0'].double()}
        grid = torch.stack(torch.meshgrid(*[torch.arange(d) for d in dims], indexing='ij')).reshape(len(dims), -1).t()
        rel = grid[:, None, :] - grid[None, :, :]
        v = torch.sign(rel).double() * torch.log(rel.abs().double() + 1)
        want = F.leaky_relu(v @ sd['p.net.0.weight'].t() + sd['p.net.0.bias'], 0.1)
        y, _ = R.cpb_ref(c)
        assert (y.reshape(want.shape) - want).abs().max() <= 1e-12
        # the oracle's own function with no hidden layer is the same affine map (its rel is rounded to f32 first)
        o = O.continuous_position_bias({'p.net.0.weight': c['w0'], 'p.net.0.bias': c['b0']}, 'p.', dims, nlayers=0).permute(1, 2, 0)
        assert (F.leaky_relu(o.double(), 0.1) - want).abs().max() <= 1e-4


def test_topk_restatement_is_torch_topk_without_ties():
    for n, k in [(5, 2), (65, 64), (257, 100)]:
        s = torch.randn(4, n, generator=R.gen(1, n))
        assert s.unique().numel() == s.numel()
        idx = s.topk(k, dim=-1).indices
        rank = R.topk_ranks(s)
        assert torch.equal(rank < k, torch.zeros(4, n).scatter(1, idx, 1).bool())
        assert torch.equal(rank.gather(1, idx), torch.arange(k).expand(4, k))
    ties = torch.tensor([[1., 0., 1., 0., 1.]])
    assert R.topk_ranks(ties).tolist() == [[0, 3, 1, 4, 2]] and R.topk_ranks(ties, higher_first=True).tolist() == [[2, 4, 1, 3, 0]]


def test_row_restatements_are_normalize_t5_norm_and_gelu_new():
    c = R.l2_case(300, 252)
    y, _ = R.l2_ref(c)
    x = c['x'][:, :252].double()
    assert (y - F.normalize(x, dim=-1, eps=1e-12)).abs().max() <= 1e-15
    c = R.rms_case(300, 260, False)
    y, _ = R.rms_ref(c)
    x = c['x'][:, :260].double()
    want = x * torch.rsqrt(x.pow(2).mean(-1, keepdim=True) + 1e-6) * c['w'].double()
    assert (y - want).abs().max() <= 1e-12 * want.abs().max()
    a = torch.linspace(-20, 20, 4001, dtype=torch.float64)
    assert (R.gelu_formula(a, torch.ones_like(a)) - F.gelu(a, approximate='tanh')).abs().max() <= 1e-14


def test_patch_layout_round_trips():
    for geom in R.PATCH_CASES:
        c = R.patch_case(geom)
        B, C, Fr, H, W, f0, nt, pt, ph, pw = geom
        src = R.patch_src(c)
        assert src.shape == (c['rows'], c['P'])
        u = dict(geom=geom, P=c['P'], rows=c['rows'], pix=R.widen(src.contiguous(), 4))
        video = torch.full_like(c['video'], NAN)
        video[:, :, f0:f0 + nt * pt] = c['video'][:, :, f0:f0 + nt * pt]
        R.unpatch_check(u, video)
        rejects(lambda: R.unpatch_check(u, c['video']), 'frames outside the group written')
        v2 = video.clone()
        v2[0, 0, f0, 0, :4] = v2[0, 0, f0, 0, :4].flip(0)
        rejects(lambda: R.unpatch_check(u, v2), 'a vector reversed')


# ------------------------------------------------------------------------------------------------ pk_layernorm

@pytest.mark.parametrize('D', R.LN_D)
def test_layernorm_checker(D):
    for M in R.LN_M:
        for vi, variant in enumerate(R.LN_VARIANTS):
            if (vi + M) % 2 and M == 300:
                continue                                          # half of the variants at the largest M: the checker is the same
            c = R.ln_case(M, D, variant)
            x, gm, bt = c['x'][:, :D], c['gamma'], c['beta']
            ref, _ = R.ln_ref(x, gm, bt)
            f32_out = ref.float()
            for y in (ref.float(), R.ln_f32(x, gm, bt, order=0), R.ln_f32(x, gm, bt, order=1)):
                b = R.ln_fake(c, y)
                ratio = R.ln_check(c, b['out'], b['out2'], b['raw'], f32_out=y)
                assert ratio <= 1
            wrong = dict(unbiased=dict(unbiased=True), eps_outside=dict(eps_outside=True), width=dict(width=D + 4))
            if bt is not None:
                wrong['beta dropped'] = dict(no_beta=True)
            if D > 4:
                wrong['gamma shifted'] = dict(gamma_shift=True)
            if c['out_kind'] == 0 or 'out2' in c['outs']:        # an f32 output exists to be held to the float64 bound
                for name, kw in wrong.items():
                    b = R.ln_fake(c, R.ln_f32(x, gm, bt, **kw))
                    rejects(lambda: R.ln_check(c, b['out'], b['out2'], b['raw'], f32_out=f32_out), name)
            if c['out_kind'] == 1:
                b = R.ln_fake(c, f32_out)
                b['out'][c['orows'], :D] = R.truncated_bf16(f32_out)
                if not torch.equal(R.truncated_bf16(f32_out).view(torch.int16), R.rne(f32_out).view(torch.int16)):
                    rejects(lambda: R.ln_check(c, b['out'], b['out2'], b['raw'], f32_out=f32_out), 'bf16 by truncation')
            moved = (c['orows'] != torch.arange(M)).nonzero()
            if moved.numel():
                o2 = c['orows'].clone()
                o2[int(moved[0])] = int(moved[0])
                b = R.ln_fake(c, f32_out, orows=o2)
                rejects(lambda: R.ln_check(c, b['out'], b['out2'], b['raw'], f32_out=f32_out), 'a row at its unpermuted place')
            if c['ld']['out'] > D:
                b = R.ln_fake(c, f32_out)
                first = next(v for v in b.values() if v is not None)
                first[int(c['orows'][0]), D] = 1.
                rejects(lambda: R.ln_check(c, b['out'], b['out2'], b['raw'], f32_out=f32_out), 'an element in the gutter')
            if 'raw' in c['outs']:
                b = R.ln_fake(c, f32_out, raw_from=f32_out)
                rejects(lambda: R.ln_check(c, b['out'], b['out2'], b['raw'], f32_out=f32_out), 'raw holding the normalised rows')


def test_layernorm_cases_cover_the_special_rows_and_maps():
    c = R.ln_case(300, 512, R.LN_VARIANTS[2])
    x = c['x'][:, :512]
    assert (x[1] == x[1, 0]).all() and (x[2] == 0).all() and abs(float(x[3].mean()) - 1e3) < 1 and 2 * R.LN_EPS < float(x[0].var()) < 8 * R.LN_EPS
    assert c['perm'] == (4, 25) and sorted(c['orows'].tolist()) == list(range(300)) and not torch.equal(c['orows'], torch.arange(300))
    kinds = {v[4] for v in R.LN_VARIANTS}
    assert kinds == {'none', 'grp', 'grp_off', 'perm'} and {v[1] for v in R.LN_VARIANTS} == {0, 1} and {v[2] for v in R.LN_VARIANTS} == {True, False}
    for M in R.LN_M:
        remap, _, orows, nrows = R.ln_map(M, 'grp_off')
        assert M % remap[0] != 0 and remap[2] > 0 and orows.unique().numel() == M and int(orows.max()) < nrows


# ------------------------------------------------------------------------------------------------ the LFQ pair

def test_lfq_projections_near_zero_stay_under_one_percent():
    """fewer than 1 % of the bits of any case lie inside their own bound of zero, so the band cannot hide a wrong kernel"""
    worst = 0.
    for M in R.LFQ_ENC_M:
        for D in R.LFQ_ENC_D:
            for cd in R.LFQ_ENC_CD:
                P, pb = R.lfq_enc_ref(R.lfq_enc_case(M, D, cd))
                band = R.lfq_band(P, pb)
                assert band.sum() <= max(0.01 * band.numel(), 0 if band.numel() > 200 else 1), (M, D, cd)
                worst = max(worst, float(band.float().mean()) if band.numel() > 200 else 0.)
    for case in R.LNLFQ_CASES:
        c = R.lnlfq_case(*case)
        _, _, P, pb = R.lnlfq_ref(c)
        band = R.lfq_band(P, pb)
        assert band.sum() <= max(0.01 * band.numel(), 0 if band.numel() > 200 else 1), case
        worst = max(worst, float(band.float().mean()) if band.numel() > 200 else 0.)
    assert worst < 0.01


@pytest.mark.parametrize('D', R.LFQ_ENC_D)
def test_lfq_encode_checker(D):
    for M in R.LFQ_ENC_M:
        for cd in R.LFQ_ENC_CD:
            c = R.lfq_enc_case(M, D, cd)
            P, _ = R.lfq_enc_ref(c)
            for p32 in (P.float(), R.lfq_enc_f32(c, 0), R.lfq_enc_f32(c, 1)):
                for with_proj in (True, False):
                    ids, proj = R.lfq_fake(c, p32, with_proj=with_proj)
                    assert R.lfq_enc_check(c, ids, proj) <= 1
            ids, proj = R.lfq_fake(c, P.float(), reverse_bits=True)
            if not torch.equal(ids, R.lfq_fake(c, P.float())[0]):
                rejects(lambda: R.lfq_enc_check(c, ids, None), 'bit order reversed')
            ids, proj = R.lfq_fake(c, P.float())
            ids[M - 1] = R.SENTINEL
            rejects(lambda: R.lfq_enc_check(c, ids, proj), 'the last row left unwritten')
            ids, proj = R.lfq_fake(c, P.float())
            ids[M] = 0
            rejects(lambda: R.lfq_enc_check(c, ids, proj), 'an id behind the output')
            if c['planted'] is not None:                          # v >= 0 instead of v > 0: only the planted exact zero tells
                ids, proj = R.lfq_fake(c, P.float())
                ids[c['planted']] |= 1 << (cd - 1)
                rejects(lambda: R.lfq_enc_check(c, ids, None), 'v >= 0 at v == 0')
            ids, proj = R.lfq_fake(c, (P + 4 * R.lfq_enc_ref(c)[1] + 1e-30).float())
            rejects(lambda: R.lfq_enc_check(c, ids, proj), 'projections off by four bounds')


@pytest.mark.parametrize('case', R.LNLFQ_CASES, ids=lambda c: f'{c[0]}x{c[1]}cd{c[2]}')
def test_layernorm_lfq_checker(case):
    c = R.lnlfq_case(*case)
    M, D = c['M'], c['D']
    assert R.lnlfq_branch(M, D) == case[7]
    y, yb, P, pb = R.lnlfq_ref(c)
    for y32, p32 in ((y.float(), P.float()), R.lnlfq_f32(c, 0), R.lnlfq_f32(c, 1)):
        out = R.lnlfq_check(c, *R.lnlfq_fake(c, y32, p32))
        assert max(out.values()) <= 1
    if M % 2 or M < 100:
        rejects(lambda: R.lnlfq_check(c, *R.lnlfq_fake(c, y.float(), P.float(), drop_last=True)), 'the last row left unwritten')
    rev = R.lnlfq_fake(c, y.float(), P.float(), reverse_bits=True)
    if not torch.equal(rev[0], R.lnlfq_fake(c, y.float(), P.float())[0]):
        rejects(lambda: R.lnlfq_check(c, *rev[:2], None), 'bit order reversed')
    if M > 5000:
        return                                                    # the LayerNorm mutants are shown at the smaller shapes
    if c['tokens']:                                               # the normalised rows themselves are held to their bound
        for name, kw in dict(unbiased=dict(unbiased=True), eps_outside=dict(eps_outside=True), width=dict(width=D + 4), shifted=dict(gamma_shift=True)).items():
            rejects(lambda: R.lnlfq_check(c, *R.lnlfq_fake(c, *R.lnlfq_f32(c, 0, **kw))), name)
    moved = (c['orows'] != torch.arange(M)).nonzero()
    if moved.numel():
        o2 = c['orows'].clone()
        o2[int(moved[0])] = int(moved[0])
        rejects(lambda: R.lnlfq_check(c, *R.lnlfq_fake(c, y.float(), P.float(), orows=o2)), 'a row at its unpermuted place')
    if c['tokens']:
        ids, tok, proj = R.lnlfq_fake(c, y.float(), P.float())
        tok[0, D] = 1.
        rejects(lambda: R.lnlfq_check(c, ids, tok, proj), 'an element in the gutter')


def test_lfq_decode_checker():
    for case in R.DECODE_CASES:
        c = R.decode_case(*case)
        out = R.place(R.nan_buffer(c['M'] + R.GUARD, c['D']), c['orows'], R.decode_ref(c))
        R.decode_check(c, out)
        bad = R.place(R.nan_buffer(c['M'] + R.GUARD, c['D']), c['orows'], R.decode_ref(c, flip_bit=c['cd'] // 2))
        rejects(lambda: R.decode_check(c, bad), 'sign inverted on one bit')
        moved = (c['orows'] != torch.arange(c['M'])).nonzero()
        if moved.numel():
            o2 = c['orows'].clone()
            o2[int(moved[0])] = int(moved[0])
            bad = R.place(R.nan_buffer(c['M'] + R.GUARD, c['D']), o2, R.decode_ref(c))
            rejects(lambda: R.decode_check(c, bad), 'a row at its unpermuted place')
        bad = out.clone()
        bad[c['M'], 0] = 0.
        rejects(lambda: R.decode_check(c, bad), 'a row behind the output')
    # the dispatch predicate
    assert R.decode_fast(512, 16, 0, 0, 0) and R.decode_fast(4, 8, 16, 32, 48) and R.decode_fast(1024, 8, 0, 0, 0)
    assert not R.decode_fast(96, 16, 0, 0, 0) and not R.decode_fast(1028, 16, 0, 0, 0) and not R.decode_fast(128, 13, 0, 0, 0)
    assert not R.decode_fast(128, 16, 4, 0, 0) and not R.decode_fast(128, 16, 0, 4, 0) and not R.decode_fast(128, 16, 0, 0, 4)


# ------------------------------------------------------------------------------------------------ pk_peg

@pytest.mark.parametrize('W', R.PEG_W)
def test_peg_checker(W):
    shapes = [(2, T, H, W, D) for T, H, D in R.PEG_THD] + [s for s, _ in R.PEG_BLOCKS if s[3] == W]
    for shape in shapes:
        for causal in (False, True):
            c = R.peg_case(*shape, causal)
            ref = R.peg_ref(c)
            for y32 in (ref[0].float(), R.peg_eval(c, torch.float32), R.peg_eval(c, torch.float32, reverse=True)):
                assert R.peg_check(c, *R.peg_fake(c, y32), ref=ref) <= 1
            wrong = {'the residual missing': dict(residual=False), 'a neighbour across the sequence boundary': dict(leak=True)}
            if causal:
                wrong['front pad 1 where causal needs 2'] = dict(tfront=1)
            tap = R.peg_active_mirror(c)
            if tap is not None:
                wrong["one tap's weight index mirrored"] = dict(mirror=tap)
            for name, kw in wrong.items():
                y32 = R.peg_eval(c, torch.float32, **kw)
                rejects(lambda: R.peg_check(c, *R.peg_fake(c, y32), ref=ref), name)
            y32 = ref[0].float()
            if not torch.equal(R.truncated_bf16(y32).view(torch.int16), R.rne(y32).view(torch.int16)):
                rejects(lambda: R.peg_check(c, *R.peg_fake(c, y32, trunc=True), ref=ref), 'bf16 by truncation')
            out, out_t = R.peg_fake(c, y32)
            out[-1, 0] = 0.
            rejects(lambda: R.peg_check(c, out, out_t, ref=ref), 'a row behind the output')


def test_peg_block_count_cases():
    for (B, T, H, W, D), blocks in R.PEG_BLOCKS:
        assert W in (4, 8, 16) and R.peg_row_blocks(B, T, H, D) == blocks
    assert {b for _, b in R.PEG_BLOCKS} == {1, 7, 9}
    B, T, H, W, D = R.PEG_BIG
    assert W not in (4, 8, 16) and B * T * H * W * (D // 4) > 16384 * 256


# ------------------------------------------------------------------------------------------------ pk_embed, pk_cfg_mix, pk_critic_head

def test_embed_checker():
    for case in R.EMBED_CASES:
        c = R.embed_case(*case)
        want = R.embed_ref(c)
        rows = torch.arange(want.shape[0])
        assert int(c['ids'].min()) == 0 and int(c['ids'].max()) == c['V'] - 1
        mk = lambda y: (R.place(R.nan_buffer(len(rows) + R.GUARD, c['D']), rows, y), R.place(R.nan_buffer(len(rows) + R.GUARD, c['D'], R.BF16), rows, R.rne(y)))
        R.embed_check(c, *mk(want))
        y = want.clone()
        y[-1, 0] = torch.nextafter(y[-1, 0], torch.tensor(9.))
        rejects(lambda: R.embed_check(c, *mk(y)), 'one ulp')
        if c['S'] > c['nb']:                                      # the replicas read the same id rows
            half = want.shape[0] // 2
            y = want.clone()
            y[half:] = want[:half].roll(1, 0)
            rejects(lambda: R.embed_check(c, *mk(y)), 'the second replica reading other ids')
        out, out_t = mk(want)
        out_t[rows] = R.truncated_bf16(want)
        rejects(lambda: R.embed_check(c, out, out_t), 'bf16 by truncation')


def test_cfg_mix_checker():
    for case in R.CFG_CASES:
        c = R.cfg_case(*case)
        y, bound = R.cfg_ref(c)
        rows = torch.arange(c['nrows'])
        mk = lambda v, t=R.F32: R.place(R.nan_buffer(c['nrows'] + R.GUARD, c['ldo'], t), rows, v)
        D, nb, n_tot, n = c['D'], c['nb'], c['n_tot'], c['n_tot'] - c['n_prime']
        lr = c['rows'].long() if c['rows'] is not None else rows
        src = (lr // n) * n_tot + lr % n + c['n_prime']
        x = c['x'][:, :D]
        evals = [y.float()]
        if c['has_null']:
            s = torch.tensor(c['scale'])
            evals += [x[nb * n_tot + src] + (x[src] - x[nb * n_tot + src]) * s, torch.addcmul(x[nb * n_tot + src], x[src] - x[nb * n_tot + src], s)]
        for v in evals:
            ratio, f32 = R.cfg_check(c, mk(v))
            assert ratio <= 1
            R.cfg_check(c, mk(R.rne(v), R.BF16), f32_out=v)
        rejects(lambda: R.cfg_check(c, mk(R.truncated_bf16(y.float()), R.BF16), f32_out=y.float()), 'bf16 by truncation')
        if c['has_null'] and c['scale'] != 1.:
            rejects(lambda: R.cfg_check(c, mk(x[src] + (x[nb * n_tot + src] - x[src]) * c['scale'])), 'cond and null swapped')
        if c['rows'] is not None:
            rejects(lambda: R.cfg_check(c, mk(y.float()[torch.argsort(lr, stable=True)])), 'the gather ignored')
        if c['ldo'] > D:
            bad = mk(y.float())
            bad[0, D] = 0.
            rejects(lambda: R.cfg_check(c, bad), 'an element in the gutter')
        if c['n_prime']:
            c2 = dict(c, n_prime=0, n_tot=n)
            rejects(lambda: R.cfg_check(c, mk(R.cfg_ref(dict(c2, x=c['x'][:(1 + c['has_null']) * nb * n]))[0].float())), 'the prime positions not skipped')


def test_critic_head_checker():
    for D in R.CRITIC_D:
        for has_null, n_prime, has_b, noise in [(1, 0, True, 'u'), (0, 2, False, 'hash'), (1, 3, True, 'none'), (1, 0, False, 'hash'), (0, 0, True, 'u')]:
            c = R.critic_case(D, has_null, n_prime, has_b, noise)
            y, bound = R.critic_ref(c)
            assert y.numel() == 5
            mk = lambda v: torch.cat([v.float(), torch.full((R.GUARD,), NAN)])
            for v in (y, R.critic_f32(c, 0), R.critic_f32(c, 1)):
                assert R.critic_check(c, mk(v)) <= 1
            rejects(lambda: R.critic_check(c, mk(y + 4 * bound + 1e-30)), 'off by four bounds')
            if noise != 'none':
                rejects(lambda: R.critic_check(c, mk(R.critic_ref(dict(c, u_eff=None))[0])), 'the noise missing')
                rejects(lambda: R.critic_check(c, mk(R.critic_ref(dict(c, u_eff=c['u_eff'].roll(1)))[0])), "another row's draw")
            if has_b:
                rejects(lambda: R.critic_check(c, mk(R.critic_ref(dict(c, b=None))[0])), 'the bias missing')
            bad = mk(y)
            bad[5] = 0.
            rejects(lambda: R.critic_check(c, bad), 'a score behind the output')


# ------------------------------------------------------------------------------------------------ pk_topk_mask

@pytest.mark.parametrize('n', R.TOPK_N)
def test_topk_mask_checker(n):
    for k in sorted({0, 1, n - 1, n}):
        c = R.topk_case(n, k)
        R.topk_check(c, *R.topk_fake(c))
        if 0 < k < n:
            rejects(lambda: R.topk_check(c, *R.topk_fake(c, higher_first=True)), 'ties resolved higher index first')
        if k < n:
            rejects(lambda: R.topk_check(c, *R.topk_fake(c, le=True)), 'rank <= k')
        if k == 0:
            mask, ids, rows_out, nxt = R.topk_fake(c)
            assert (rows_out == R.SENTINEL).all() and torch.equal(ids[:c['B'] * n], c['ids0'].reshape(-1))
            rows_out[0] = 0
            rejects(lambda: R.topk_check(c, mask, ids, rows_out, nxt), 'rows_out touched at k = 0')
        mask, ids, rows_out, nxt = R.topk_fake(c)
        nxt[n - 1] = 0.
        rejects(lambda: R.topk_check(c, mask, ids, rows_out, nxt), 'scores_next not -1e4')
        if k >= 2:
            mask, ids, rows_out, nxt = R.topk_fake(c)
            rows_out[:2] = rows_out[:2].flip(0)
            rejects(lambda: R.topk_check(c, mask, ids, rows_out, nxt), 'rows_out out of rank order')


# ------------------------------------------------------------------------------------------------ the row kernels

@pytest.mark.parametrize('D', R.ROW_D)
def test_row_kernel_checkers(D):
    for M in R.ROW_M:
        rows = torch.arange(M)
        for masked in (False, True):
            c = R.rms_case(M, D, masked)
            ref = R.rms_ref(c)
            mk = lambda v, t=R.F32: R.place(R.nan_buffer(M + R.GUARD, c['ldo'], t), rows, v)
            for v in (ref[0].float(), R.rms_f32(c, 0), R.rms_f32(c, 1)):
                ratio, f32 = R.rows_check(c, mk(v), ref, 'rmsnorm', zero_rows=R.rms_zero_rows(c))
                assert ratio <= 1
                R.rows_check(c, mk(R.rne(v), R.BF16), ref, 'rmsnorm', f32_out=v, zero_rows=R.rms_zero_rows(c))
            rejects(lambda: R.rows_check(c, mk(R.rms_f32(c, 0, center=True)), ref, 'rmsnorm'), 'mean subtracted')
            rejects(lambda: R.rows_check(c, mk(R.truncated_bf16(ref[0].float()), R.BF16), ref, 'rmsnorm', f32_out=ref[0].float()), 'bf16 by truncation')
            if masked and M > 1:
                bad = mk(ref[0].float())
                bad[1, 0] = -0.
                rejects(lambda: R.rows_check(c, bad, ref, 'rmsnorm', zero_rows=R.rms_zero_rows(c)), 'a masked row holding -0.0')
                c2 = dict(c, rowmask=None)
                rejects(lambda: R.rows_check(c, mk(R.rms_f32(c2, 0)), ref, 'rmsnorm', zero_rows=R.rms_zero_rows(c)), 'the row mask ignored')
            bad = mk(ref[0].float())
            bad[0, D] = 0.
            rejects(lambda: R.rows_check(c, bad, ref, 'rmsnorm'), 'an element in the gutter')
        c = R.l2_case(M, D)
        ref = R.l2_ref(c)
        mk = lambda v, t=R.F32: R.place(R.nan_buffer(M + R.GUARD, c['ldo'], t), rows, v)
        for v in (ref[0].float(), R.l2_f32(c, 0), R.l2_f32(c, 1)):
            ratio, _ = R.rows_check(c, mk(v), ref, 'l2norm_rows', zero_rows=R.l2_zero_rows(c))
            assert ratio <= 1
        x = c['x'][:, :D]
        rejects(lambda: R.rows_check(c, mk(x * (1.0 / (x * x).sum(1).clamp_min(1e-12))[:, None]), ref, 'l2norm_rows'), 'divided by the squared norm')
        if D > 4:
            rejects(lambda: R.rows_check(c, mk(x * (1.0 / torch.sqrt((x * x)[:, :D - 4].sum(1)).clamp_min(1e-12))[:, None]), ref, 'l2norm_rows'), 'the last vector left out of the norm')
        c = R.gelu_case(M, D)
        ref = R.gelu_ref(c)
        mk = lambda v, t=R.F32: R.place(R.nan_buffer(M + R.GUARD, c['ldo'], t), rows, v)
        for v in (ref[0].float(), R.gelu_f32(c)):
            ratio, _ = R.rows_check(c, mk(v), ref, 'gated_gelu_tanh')
            assert ratio <= 1
        a, b = c['h'][:, :D], c['h'][:, D:2 * D]
        rejects(lambda: R.rows_check(c, mk(F.gelu(a) * b), ref, 'gated_gelu_tanh'), 'the erf form of GELU')
        rejects(lambda: R.rows_check(c, mk(R.gelu_formula(b, a)), ref, 'gated_gelu_tanh'), 'gate and value swapped')
        rejects(lambda: R.rows_check(c, mk(0.5 * a * (1.0 + torch.tanh(R.GELU_K * (a + 0.044 * a * a * a))) * b), ref, 'gated_gelu_tanh'), 'the cubic coefficient cut short')


def test_transcendental_allowances():
    """the constants beside GELU_C and CPB_C are what torch's f32 CPU evaluation of the same formulas misses float64 by, in units of U scale, over the case
    inputs; the kernels get four times that"""
    worst = 0.
    for D in R.ROW_D:
        for M in R.ROW_M:
            c = R.gelu_case(M, D)
            worst = max(worst, R.unit_ratio(R.gelu_f32(c), R.gelu_ref(c, cc=1.)))
    print(f'gated_gelu_tanh: f32 CPU evaluation err / (U scale) = {worst:.3f}')
    assert 0.25 * R.GELU_CPU_RATIO <= worst <= R.GELU_CPU_RATIO and R.GELU_C == 4 * R.GELU_CPU_RATIO
    worst = 0.
    for dims, D in R.CPB_CASES + [R.CPB_BIG]:
        c = R.cpb_case(dims, D)
        worst = max(worst, R.unit_ratio(R.cpb_f32(c), R.cpb_ref(c, cc=1.)))
    print(f'cpb_input: f32 CPU evaluation err / (U scale) = {worst:.3f}')
    assert 0.25 * R.CPB_CPU_RATIO <= worst <= R.CPB_CPU_RATIO and R.CPB_C == 4 * R.CPB_CPU_RATIO


# ------------------------------------------------------------------------------------------------ pk_patchify_ln, pk_cpb_input

def test_patchify_checker():
    assert sorted({R.patch_P(g) for g in R.PATCH_CASES}) == [4, 96, 4096, 4112, 8192]
    for geom in R.PATCH_CASES:
        c = R.patch_case(geom)
        P, rows = c['P'], torch.arange(c['rows'])
        src = R.patch_src(c)
        mk = lambda v, t=R.F32: R.place(R.nan_buffer(c['rows'] + R.GUARD, c['ldo'], t), rows, v)
        R.patch_check(c, mk(src), False)
        ref, _ = R.ln_ref(src, c['weight'], c['bias'])
        for v in (ref.float(), R.ln_f32(src, c['weight'], c['bias'], order=0), R.ln_f32(src, c['weight'], c['bias'], order=1)):
            ratio, _ = R.patch_check(c, mk(v), True)
            assert ratio <= 1
            R.patch_check(c, mk(R.rne(v), R.BF16), True, f32_out=v)
        wrong = dict(eps_outside=dict(eps_outside=True), beta=dict(no_beta=True), width=dict(width=P + 8))
        if P < 4096:                                              # from P^2 U = 1 on a swap of 1 / P for 1 / (P - 1) is inside any-order f32 summation
            wrong['unbiased'] = dict(unbiased=True)
        for name, kw in wrong.items():
            rejects(lambda: R.patch_check(c, mk(R.ln_f32(src, c['weight'], c['bias'], **kw)), True), name)
        if P > 4:
            rejects(lambda: R.patch_check(c, mk(R.ln_f32(src, c['weight'], c['bias'], gamma_shift=True)), True), 'gamma shifted')
        B, C, Fr, H, W, f0, nt, pt, ph, pw = geom
        rejects(lambda: R.patch_check(c, mk(R.patchify(c['video'], f0 - 1, nt, pt, ph, pw)), False), 'f0 ignored')
        rejects(lambda: R.patch_check(c, mk(R.truncated_bf16(ref.float()), R.BF16), True, f32_out=ref.float()), 'bf16 by truncation')
        bad = mk(src)
        bad[0, P] = 0.
        rejects(lambda: R.patch_check(c, bad, False), 'an element in the gutter')


def test_cpb_input_checker():
    for dims, D in R.CPB_CASES:
        c = R.cpb_case(dims, D)
        y, bound = R.cpb_ref(c)
        mk = lambda v: torch.cat([v.reshape(-1).float(), torch.full((R.GUARD,), NAN)])
        assert R.cpb_check(c, mk(y)) <= 1 and R.cpb_check(c, mk(R.cpb_f32(c))) <= 1
        n = c['n']
        rejects(lambda: R.cpb_check(c, mk(y.reshape(n, n, D).transpose(0, 1))), 'pos_j - pos_i')
        acc = torch.where(y > 0, y, y / 0.1)
        rejects(lambda: R.cpb_check(c, mk(torch.where(acc > 0, acc, 0.01 * acc))), 'the wrong slope')
        if len(dims) == 2:
            c3 = R.cpb_case(dims[::-1], D)
            c3.update(w0=c['w0'], b0=c['b0'])
            rejects(lambda: R.cpb_check(c, mk(R.cpb_ref(c3)[0])), 'the axes of a 2-d grid taken in the other order')
    dims, D = R.CPB_BIG
    assert (dims[0] * dims[1] * dims[2]) ** 2 * D > 16384 * 256
