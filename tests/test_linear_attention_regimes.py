"""CPU checks of linear_attention_regimes.py: the generators are deterministic and produce the regimes they claim, the restatements with
mut=None ARE the oracle's, what they lose against float64 is what the table records (and within the condition under which a regime is
kept), every mutation the device test could catch is caught by a factor of two over the device budget - and those it cannot catch are
named, with the reason - and the one-pass LayerNorm's limit against the ratios the model reaches."""
import pytest
import torch
import torch.nn.functional as F

import geoformer_oracle as O
import golden_inputs as GI
import linear_attention_regimes as R

H16, BF16, F32 = R.H16, R.BF16, R.F32


def _id(e):
    return f'{e[0]}/{R.key(e[1], e[2])}/{R.NAME[e[3]]}'


def test_generators_deterministic():
    for make in (lambda: R.coarse_case('ln_offset', 32, BF16), lambda: R.fine_case('ramp', None, H16, 9, 17, True), lambda: R.tanh_case(H16)):
        a, b = make(), make()
        for k in ('x', 'src', 'msg'):
            if k in a:
                assert torch.equal(a[k], b[k])
        assert all(torch.equal(a['P'][k], b['P'][k]) for k in a['P'])
    assert all(torch.equal(x, y) for x, y in zip(R.window_operands('hot', None, BF16, 6, 32, 17), R.window_operands('hot', None, BF16, 6, 32, 17)))


@pytest.mark.parametrize('st', [H16, BF16])
def test_unmutated_restatements_are_the_oracle(st):
    """attention_restated / finish_restated / layer_restated exist only to carry the mutations: without one they return the oracle's bits."""
    case, _ = R.cached_coarse('few_keys', 6 if st == H16 else 2, st)
    P, x, src, xm, sm = case['P'], case['x'], case['src'], case['xm'], case['sm']
    assert torch.equal(R.layer_restated(case), O.encoder_layer_fused(P, '', x, src, 8, st, xm, sm, one_pass=True))
    fc, _ = R.cached_fine('cold_q', -12, st, 5, 32, False)
    assert torch.equal(R.layer_restated(fc, chain=True), O.encoder_layer_chain(fc['P'], '', fc['x'], fc['src'], 8, st, one_pass=True))
    q, k, v, xm, sm, _, _ = R.cached_k2('few_keys', 6 if st == H16 else 2, st)
    sp = lambda t: t.float().view(t.shape[0], -1, 8, 32)                         # noqa: E731
    assert torch.equal(R.k2_restated(q, k, v, st, 8, xm, sm), O.linear_attention_window(sp(q), sp(k), sp(v), st, xm, sm).reshape(q.shape))
    tc, _, _ = R.cached_tanh(st)
    assert torch.equal(R.finish_restated(tc['P'], tc['x'], tc['msg'], 'geo', st), O._finish_fused(tc['P'], '', tc['x'], tc['msg'], 'geo', st, one_pass=True))
    # the state restatement is the one tests/test_encoder_fused.py:test_kv_state_vs_oracle writes out
    KV, Ks = O.encoder_kv_state_fused(P, '', src, 8, st, sm)
    kk = F.linear(src, O.rt(P['k_proj.weight'], st)).view(4, -1, 8, 32)
    vv = F.linear(src, O.rt(P['v_proj.weight'], st)).view(4, -1, 8, 32)
    Kf = O._phi(kk) * sm[:, :, None, None]
    assert torch.equal(KV, torch.einsum('nshd,nshv->nhdv', O.rt(Kf, st), O.rt(vv, st))) and torch.equal(Ks, Kf.sum(1))


def test_one_pass_layer_norm_is_layer_norm_on_centred_rows():
    g = torch.Generator().manual_seed(1)
    x = torch.randn(64, 256, generator=g)
    w, b = 1 + 0.1 * torch.randn(256, generator=g), 0.1 * torch.randn(256, generator=g)
    torch.testing.assert_close(O.layer_norm_one_pass(x, w, b, 1e-5), F.layer_norm(x, (256,), w, b, 1e-5), rtol=1e-5, atol=2e-6)
    # plain rows (256 channels, fp32 against float64): the one-pass form loses about ratio^2 * 7e-7, the centred form stays below 1e-4
    x64 = torch.randn(4096, 256, generator=g, dtype=torch.float64)
    one = torch.ones(256)
    for ratio, lo, hi in ((10, 2e-5, 2e-4), (30, 2e-4, 2e-3), (100, 2e-3, 2e-2), (300, 2e-2, 2e-1)):
        ref = F.layer_norm(x64 + ratio, (256,), eps=1e-5)
        err = float((O.layer_norm_one_pass((x64 + ratio).float(), one, 0 * one, 1e-5).double() - ref).abs().max())
        assert lo < err < hi, (ratio, err)
        assert float((F.layer_norm((x64 + ratio).float(), (256,), eps=1e-5).double() - ref).abs().max()) < 1e-4


# ------------------------------------------------------------------------------------------------------------------- regime properties
def _finite_operands(case):
    st = case['st']
    assert all(bool(torch.isfinite(O.rt(w, st)).all()) for w in case['P'].values())
    q, k, v = R.projections64(case)
    for t in (q, k, v):
        assert bool(torch.isfinite(t.float().to(st).float()).all())               # k, v as the kernels round them
    return q, k, v


@pytest.mark.parametrize('regime,variant,st', [(r, v, st) for (r, v), types in R.COARSE.items() for st in types],
                         ids=lambda p: R.NAME.get(p, str(p)))
def test_coarse_regime_is_what_it_claims(regime, variant, st):
    case, ref = R.cached_coarse(regime, variant, st)
    q, k, v = _finite_operands(case)
    assert bool(torch.isfinite(ref).all())
    assert bool((case['x'][..., 0] == 1).all())
    if regime == 'control':
        assert not any(bool(case['P'][m + '.weight'][:, 0].any()) for m, _, _ in R._MATS)
    elif regime == 'hot':
        assert float(q.min()) > 0 and float(k.min()) > 0                           # phi on its linear branch, every element
    elif regime in ('cold_q', 'cold_qv'):
        assert float(q.max()) < 0 and abs(float(q.mean()) - variant) < 0.05
    elif regime == 'cold_k':
        assert float(k.max()) < 0 and abs(float(k.mean()) - variant) < 0.05
    elif regime == 'few_keys':
        sm = case['sm']
        assert tuple(int(c) for c in sm.sum(1)) == R.FEW_KEYS
        assert bool(sm[1, :3].all()) and int(sm[2].nonzero()[0, 0]) == 777          # a prefix, and a key in the middle of the seventh tile
        assert abs(float(k[1, :3].mean()) - R.FEW_KEYS_OFF3[st]) < 0.2 and abs(float(k[2, 777].mean()) - variant) < 0.2
        assert not bool(case['xm'].all()) and bool(case['xm'].any(1).all())
        # an image without keys and masked queries: the float64 message is an exact zero, the layer is the layer at msg = 0
        msg, A = R.attention64(q, k, v, case['xm'], sm)
        assert float(msg[3].abs().max()) == 0 and float(msg[0, 100:131].abs().max()) == 0 and float(A[3].max()) == 0
    elif regime == 'wide_v':
        kvs = float(R._kv_over_s(case).abs().max())
        assert 2.0 ** 13 <= kvs < 2.0 ** 15, kvs                                 # just below fp16 overflow
        assert float(v.abs().max()) < 65504 and float(k.min()) > 0
        assert int(case['sm'][1].sum()) == 640 and not bool(case['sm'][2, 1::3].any())
    elif regime == 'sparse_v':
        sm = case['sm']
        assert all(int(c) == R.SPARSE_KEYS for c in sm.sum(1)) and bool(sm[0, :R.SPARSE_KEYS].all()) and not bool(sm[1, 1:32].any())
        K = F.elu(k) + 1
        # every product phi(k) |v| of a valid key lies beyond fp16's range (so does their mean over the valid keys) ...
        assert float((K.amin(-1, keepdim=True) * v.abs())[sm].min()) > 65504
        # ... and the state scaled by the padded length, like v itself, well inside it
        assert 2.0 ** 11 <= float(R._kv_over_s(case).abs().max()) < 2.0 ** 13 and float(v.abs().max()) < 2.0 ** 14
    elif regime == 'ramp':
        eff = R.ramp_swap_effect(q, k, v, st)
        weakest = min(eff.items(), key=lambda kv: kv[1])
        print('weakest exchange', weakest)
        assert len(eff) == 28 + 8 and weakest[1] >= 50, weakest
        offs = case['P']['q_proj.weight'][:, 0].abs().max(), case['P']['k_proj.weight'][:, 0].abs().max()
        assert max(float(o) for o in offs) <= 6.0
    elif regime == 'ln_offset':
        for rows in R.ln_inputs64(case):
            r = R.mean_over_std(rows)
            assert abs(float(r.median()) / variant - 1) < 0.03 and float(r.min()) > 0.7 * variant, (float(r.median()), float(r.min()))


@pytest.mark.parametrize('regime,variant,st', [(r, v, st) for (r, v), types in R.FINE.items() for st in types], ids=lambda p: R.NAME.get(p, str(p)))
def test_fine_regime_is_what_it_claims(regime, variant, st):
    for Nw, Lw, cross in R.fine_shapes(regime):
        case, ref = R.cached_fine(regime, variant, st, Nw, Lw, cross)
        q, k, v = _finite_operands(case)
        assert bool(torch.isfinite(ref).all()) and (case['src'] is case['x']) == (not cross)
        if regime == 'hot':
            assert float(q.min()) > 0 and float(k.min()) > 0
        elif regime == 'cold_q':
            assert float(q.max()) < 0
        elif regime == 'cold_k':
            assert float(k.max()) < 0
        elif regime == 'ramp':
            weakest = min(R.ramp_swap_effect(q, k, v, st, halves=False).values())
            assert weakest >= 50, weakest
        elif regime == 'ln_offset':
            for rows in R.ln_inputs64(case):
                r = R.mean_over_std(rows)
                assert abs(float(r.median()) / variant - 1) < 0.05 and float(r.min()) > 0.7 * variant, (float(r.median()), float(r.min()))
    if regime == 'ramp':                                   # K2's window kernel gets the offsets on q, k, v directly
        for N, L, S in R.WINDOW_SHAPES:
            q, k, v, _, _ = R.cached_window(regime, variant, st, N, L, S)
            sp = lambda t: t.double().view(N, -1, 8, 16)                             # noqa: E731
            assert min(R.ramp_swap_effect(sp(q), sp(k), sp(v), st, halves=False).values()) >= 50


@pytest.mark.parametrize('st', [H16, BF16])
def test_tanh_regime_saturates(st):
    case, ref, pre = R.cached_tanh(st)
    assert float(pre.max()) > 90 and float(pre.min()) < -90                        # exp(2 x) overflows fp32 beyond 44
    assert float((pre[..., :171].abs() < 3).float().mean()) > 0.9                   # ... and the unscaled rows stay on tanh's slope
    assert bool(torch.isfinite(ref).all()) and torch.equal(ref[1], case['x'][1].double())


# ------------------------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize('entry', R.entries(), ids=_id)
def test_restatement_table(entry):
    """What the restatement alone loses against float64 is what REST records (never more; REST is the measurement rounded up, not a
    bound chosen afterwards: it may not be slack either), and a regime is kept for a 16-bit type only if that stays within KEEP."""
    got = R.restatement_error(*entry)
    rec = R.rest(*entry)
    print(_id(entry), 'measured', got, 'recorded', rec)
    assert got[0] <= rec[0] and got[1] <= rec[1], (got, rec)
    assert rec[0] <= 1.3 * got[0] + 0.1 and rec[1] <= 1.3 * got[1] + 0.005, (got, rec)
    if entry[3] != F32:                                     # (fp32: ulps of fp32; the condition is about the 16-bit types)
        keep = R.KEEP[R.kind_of(entry[0])]
        assert rec[0] <= keep[0] and rec[1] <= keep[1]


def test_cliffs():
    """Where the fp16 restatement leaves the message condition - the offsets the table stops short of (not run on the device in fp16)."""
    for regime, off in (('cold_q', -16), ('cold_k', -12)):
        q, k, v, xm, sm, ref, A = R.cached_k2(regime, off, H16)
        e = R.message_error(R.k2_restated(q, k, v, H16, 8), ref, A, H16)
        print(regime, off, e)
        assert e[0] > R.KEEP['message'][0] or e[1] > R.KEEP['message'][1], (regime, off, e)
    # few keys among 1280: -5 on the 3-key image, 0 on the 1-key image (the offsets bf16 keeps)
    case = R.coarse_case('few_keys', 0, BF16)
    q, k, v = (t.float().to(H16) for t in R.k2_operands(case, BF16))
    ref, A = R.k2_reference(q, k, v, 8, case['xm'], case['sm'])
    got = R.k2_restated(q, k, v, H16, 8, case['xm'], case['sm'])
    for b in (1, 2):
        assert R.message_error(got[b:b + 1], ref[b:b + 1], A[b:b + 1], H16)[0] > 2.0


# ------------------------------------------------------------------------------------------------------------------- mutations
# mutation -> the (entry, regime, variant, type) that exposes it; what the device test of that line would catch
CAUGHT = {'den_unrounded': ('k2', 'cold_qv', -13, H16), 'eps_unscaled': ('k2', 'few_keys', -8, BF16), 'inv_valid': ('k9', 'sparse_v', None, H16), 'mask_v_only': ('k9', 'few_keys', 6, H16),
          'swap_heads': ('k9', 'ramp', None, BF16), 'swap_halves': ('k9', 'ramp', None, BF16), 'phi_no_plus1': ('k2w', 'control', None, BF16),
          'ln_no_eps': ('k9', 'few_keys', 2, BF16)}
# mutations no regime within the kept ranges exposes, and why (the finding, not a failure):
NOT_CAUGHT = {
    # K is zero on a masked row, so v of that row multiplies zero: with finite v the result has the same bits (the fused form never masks v)
    'mask_k_only': 'identical bits for finite v',
    # the kernels are one-pass: a two-pass kernel is the more accurate one and stays inside a budget recorded from the one-pass restatement;
    # the reverse (a one-pass kernel against a two-pass budget) shows from a ratio of 96 in fp16 and 256 in bf16, beyond the kept 32 / 128
    'ln_two_pass': 'more accurate than the restatement',
}


def _factor(entry, mut):
    base = R.restatement_error(*entry)
    bud = R.budget(R.rest(*entry))
    assert base[0] <= bud[0] and base[1] <= bud[1]                                   # the unmutated restatement passes
    e = R.restatement_error(*entry, mut=mut)
    return max(e[0] / bud[0], e[1] / bud[1]), e


def test_every_mutation_is_listed():
    assert set(CAUGHT) | set(NOT_CAUGHT) == set(R.MUTATIONS) and not set(CAUGHT) & set(NOT_CAUGHT)


@pytest.mark.parametrize('mut', sorted(CAUGHT))
def test_mutation_exceeds_the_device_budget(mut):
    f, e = _factor(CAUGHT[mut], mut)
    print(mut, _id(CAUGHT[mut]), 'error', e, 'over budget by', f)
    assert f >= 2.0, (mut, f, e)


def test_inv_valid_shows_only_through_overflow():
    """1 / (valid keys) in place of 1 / S, used for KV, Ksum and eps alike, cancels in the quotient: it is caught where the scaling by the
    PADDED length is what keeps the fp16 state finite (sparse_v: KV / valid ~ 13 * 7900 overflows, in K2, in the K9 message and in the K9 layer),
    and nowhere else - in few_keys and wide_v it moves the state away from the subnormals and is the more accurate form; bf16 has the range."""
    for ent in ('k2', 'k9msg', 'k9'):
        assert _factor((ent, 'sparse_v', None, H16), 'inv_valid')[0] == float('inf')
    rest = [e for e in R.entries() if e[1] in ('few_keys', 'wide_v') or (e[1] == 'sparse_v' and e[3] == BF16)]
    assert len(rest) >= 15 and max(_factor(e, 'inv_valid')[0] for e in rest) < 2.0


def test_unrounded_denominator_is_below_the_k9_budget():
    """The finding for K9: with the layer behind it, the normaliser from the un-rounded phi(q) stays inside the layer budget at every kept
    offset (1.4 x at cold_qv -13, the regime that exposes it in K2) - only K2's message check sees it."""
    assert max(_factor(e, 'den_unrounded')[0] for e in R.entries() if e[0] in ('k9', 'k11')) < 2.0


@pytest.mark.parametrize('mut', sorted(NOT_CAUGHT))
def test_mutation_no_regime_exposes(mut):
    worst = 0.0
    for entry in R.entries():
        if entry[3] == F32 or (mut.startswith('ln_') and R.kind_of(entry[0]) == 'message'):
            continue
        if mut == 'mask_k_only':
            if entry[1] in ('few_keys', 'wide_v', 'sparse_v'):
                assert R.restatement_error(*entry, mut=mut) == R.restatement_error(*entry)
            continue
        worst = max(worst, _factor(entry, mut)[0])
    print(mut, 'worst factor over the device budget', worst)
    assert worst < 2.0


# ------------------------------------------------------------------------------------------------------------------- the LayerNorm question
# the first mean / std ratio of a LayerNorm input row (steps of the list below) at which the one-pass restatement of the K9 layer leaves
# the output condition KEEP['output'] - and the last one at which it holds
ONE_PASS_LIMIT = {H16: (64, 96), BF16: (128, 256)}      # (bf16 at 192: 3.7 ulp maximum, at the edge)
MODEL_RATIO_MAX = 0.5        # the largest ratio the model's LayerNorm inputs reach on the end-to-end fixtures (measured: 0.29)


@pytest.mark.parametrize('st', [H16, BF16])
def test_one_pass_layernorm_limit(st):
    ok, bad = ONE_PASS_LIMIT[st]
    keep = R.KEEP['output']
    for ratio, want in ((ok, True), (bad, False)):
        case = R.coarse_case('ln_offset', ratio, st, 256, 256)
        ref = R.layer64(case)
        one, two = R.output_error(R.layer_restated(case), ref, st), R.output_error(R.layer_restated(case, 'ln_two_pass'), ref, st)
        print(R.NAME[st], ratio, 'one-pass', one, 'two-pass', two)
        assert (one[0] <= keep[0] and one[1] <= keep[1]) == want
        assert two[0] <= keep[0] and two[1] <= keep[1]                               # the centred form is not the limit


def test_model_layernorm_inputs_are_far_from_the_limit(golden):
    """|mean| / std of every row that enters a LayerNorm in the oracle's forward of the end-to-end fixtures (g10a-d with make_weights;
    g3 and g4 layers): the layers have no bias, so the rows are centred up to noise.  (No trained checkpoint ships with the repository;
    geoformer_amd/weights.py builds deterministic ones.)"""
    W = O.make_weights()
    seen = []
    orig = F.layer_norm

    def spy(x, shape, *a, **k):
        seen.append(float(R.mean_over_std(x.double()).max()))
        return orig(x, shape, *a, **k)

    def replay(G):
        calls = iter(range(int(G['ransac_ncalls'])))

        def fn(a, b):
            i = next(calls)
            return (G[f'ransac{i}_M'].copy() if G[f'ransac{i}_valid'] else None), G[f'ransac{i}_mask'].copy()
        return fn
    F.layer_norm = spy
    try:
        for name, case in GI.g10_cases().items():
            cfg = O.default_geo_config()
            cfg.update(coarse_thr=case['coarse_thr'], fine_thr=case['fine_thr'])
            O.geoformer_forward(W, dict(case['data']), None, cfg, replay(golden(name)), {}, case['feats'])
        I, I4 = GI.g3_inputs(), GI.g4_inputs()
        O.encoder_layer(W, 'loftr_coarse.layers.0.', I['x'], I['src'], 8, 'loftr', I['x_mask'], I['src_mask'])
        O.encoder_layer(W, 'loftr_fine.layers.0.', I['xf'], I['sf'], 8, 'loftr')
        O.encoder_layer(W, 'geo_module.des_transformer.layers.0.', I4['x_self'], I4['src_self'], 4, 'geo')
        O.encoder_layer(W, 'geo_module.des_transformer.layers.1.', I4['x_cross'], I4['src_cross'], 4, 'geo', None, I4['kv_mask'])
    finally:
        F.layer_norm = orig
    print('LayerNorm calls', len(seen), 'largest |mean| / std', max(seen))
    assert len(seen) > 200 and max(seen) < MODEL_RATIO_MAX < min(v[0] for v in ONE_PASS_LIMIT.values()) / 100
