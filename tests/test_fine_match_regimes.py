"""CPU checks of fine_match_regimes.py: the generators are deterministic and produce what they claim, every match of every regime, type and
channel count has a clear decision (so the GPU tests compare all of them), the fp32 restatement of the scalar kernel lies within the derived
bound, and every mutation of it exceeds the bound or flips a clear decision on a named regime."""
import math

import pytest
import torch

import geoformer_oracle as O
import fine_match_regimes as R
import linear_attention_regimes as LA

CASES = [(regime, dtype) for regime in R.REGIMES for dtype in R.TYPES]


def _finite(ref):
    return ~torch.isnan(ref['conf'].flatten(1)).any(1)


def _restated_check(c, thr=None, mut=None):
    """(max error / bound over the finite windows, its mean, number of decisions that differ from the reference's) of the restatement."""
    thr = c['thr'] if thr is None else thr
    ref = c['ref'] if thr == c['thr'] else R.reference(c['f0'], c['f1'], thr)
    conf, sel = R.restated(c['f0'], c['f1'], thr, mut=mut)
    fin = _finite(ref)
    r = R.conf_error(conf[fin], ref['conf'][fin], c['tol'][fin])
    return float(r.max()), float(r.mean()), int((sel != ref['sel']).sum())


def test_generators_deterministic():
    tags = [('straddle', R.BF16, 64), ('ties', R.H16, 16), ('range', R.F32, 128), ('nonfinite', R.H16, 128)]

    def draw():
        LA._CACHE.clear()
        w = [R.windows(*t) for t in tags]
        c = R.compaction_case(1025, 'mixed')
        return [x[k] for x in w for k in ('f0', 'f1')] + [c['f0'], c['f1'], c['b_ids'], c['mkpts0_c'], c['mkpts1_c'], c['accept']]
    a, b = draw(), draw()
    bits = lambda t: t.view(torch.int16) if t.dtype in (R.H16, R.BF16) else t.view(torch.int32) if t.dtype == R.F32 else t   # noqa: E731
    assert all(torch.equal(bits(x), bits(y)) for x, y in zip(a, b))                    # bit patterns: NaN compares equal to itself


def test_first_index_rule_is_written_out():
    flat = torch.tensor([[0.1, 0.7, 0.7, 0.2], [0.5, 0.5, 0.5, 0.5], [0.1, math.nan, 0.9, 0.9]], dtype=torch.float64)
    top, first = R.first_max(flat)
    assert first.tolist() == [1, 0, -1] and math.isnan(float(top[2]))
    assert R.last_max(flat)[1].tolist()[:2] == [2, 3]


@pytest.mark.parametrize('regime,dtype', CASES, ids=str)
def test_reference_is_the_oracles_dual_softmax(regime, dtype):
    """dual_softmax64 (one summation order for every cell) against O.dual_softmax in float64: equal to a few float64 roundings of the
    logits (2e-16 * 800 nats), NaN in the same windows."""
    for C in R.regime_cs(regime, dtype):
        c = R.case(regime, dtype, C)
        o = O.dual_softmax(c['f0'].double(), c['f1'].double(), R.TEMP)
        fin = _finite(c['ref'])
        assert torch.equal(~torch.isnan(o.flatten(1)).any(1), fin)
        assert torch.allclose(c['ref']['conf'][fin], o[fin], rtol=1e-11, atol=1e-300)


@pytest.mark.parametrize('regime,dtype', CASES, ids=str)
def test_every_match_is_clear(regime, dtype):
    """No exclusions: the reference alone decides every match by more than the margin of its own bound."""
    for C in R.regime_cs(regime, dtype):
        c = R.case(regime, dtype, C)
        cl = R.clear(c['ref'], c['tol'], c['thr'])
        assert bool(cl.all()), (C, torch.nonzero(~cl)[:, 0].tolist())
        if regime == 'ties':                                      # the same windows at thr = 1: nothing can be accepted (ge_thr)
            assert bool(R.clear(R.reference(c['f0'], c['f1'], 1.0), c['tol'], 1.0).all())


@pytest.mark.parametrize('dtype', R.TYPES, ids=str)
def test_regimes_are_what_they_claim(dtype):
    for C in R.CS:
        x = lambda c: torch.einsum('mic,mjc->mij', c['f0'].double(), c['f1'].double()) / (C * R.TEMP)      # noqa: E731
        c = R.case('control', dtype, C)
        top, ok = c['ref']['top'], c['ref']['ok']
        assert float(top.min()) < 0.04 and float(top.max()) > 0.95 and 15 <= int(ok.sum()) <= 55, (float(top.min()), float(top.max()))
        c = R.case('range', dtype, C)
        assert float(x(c).abs().flatten(1).amax(1).min()) >= 300.0                      # every match; an unguarded exp overflows above 88
        ar = torch.arange(R.M_REG)
        assert torch.equal(c['ref']['first'], c['i'] * R.WW + c['j'])                       # the partner pair, not a saturated permutation
        assert int((c['ref']['conf'] == c['ref']['top'][:, None, None]).sum()) == R.M_REG   # one top cell each: no tie
        c = R.case('underflow', dtype, C)
        s = x(c)
        peak = s[ar, c['i'], c['j']].clone()
        s[ar, c['i'], c['j']] = -math.inf
        lead2 = (peak - s.flatten(1).amax(1)) / math.log(2.0)
        assert float(lead2.min()) >= 200.0, float(lead2.min())
        c = R.case('nonfinite', dtype, C)
        bad = c['bad']
        assert bad == [1, 6, 63, 65, 66] and not bool(c['ref']['ok'][bad].any()) and bool((c['ref']['sel'][bad] == -1).all())
        assert all(bool(torch.isnan(c['ref']['conf'][m]).any()) for m in bad)
        twin = R.reference(*c['twin'])
        good = [m for m in range(R.M_REG) if m not in bad]
        assert torch.equal(twin['sel'][good], c['ref']['sel'][good]) and int(twin['ok'][bad].sum()) >= 2   # their finite twins: a mix


@pytest.mark.parametrize('dtype', R.TYPES, ids=str)
@pytest.mark.parametrize('C', [128, 64])
def test_straddle_hits_its_targets(C, dtype):
    c = R.case('straddle', dtype, C)
    ref = c['ref']
    delta = c['delta']
    assert delta == R.straddle_delta(c['f0'], c['f1']) >= 2e-3
    off = (ref['top'] / c['target'] - 1).abs()
    print(f'straddle {dtype} C={C}: delta {delta:.2e}, worst landing {float(off.max()):.2e} (allowed {delta / 4:.2e})')
    assert float(off.max()) <= delta / 4
    assert torch.equal(ref['first'], c['i'] * R.WW + c['j'])
    second = ref['conf'].flatten(1).topk(2, dim=1)[0][:, 1]
    assert float((second / ref['top']).max()) <= 0.9
    ar = torch.arange(R.M_REG)
    assert torch.equal(ref['ok'], ar % 2 == 1)                                          # below thr on even matches, above on odd


@pytest.mark.parametrize('dtype', R.TYPES, ids=str)
def test_ties_are_exact_float64_ties(dtype):
    """(a) rows i < i' of f0 bit-identical, both partnered by one f1 row: cells (i, j), (i', j) tie;  (b) the same for columns;  (c) every row
    of f0 equal and every row of f1 equal: all 625 cells tie, cell 0 wins (offsets (-2, -2));  (d) a saturated permutation window: several
    cells exactly 1.0;  (e) zero rows as a border window has them, tied at the top of one column.  In each the reference's first index is
    the planted one."""
    for C in R.regime_cs('ties', dtype):
        c = R.case('ties', dtype, C)
        conf, top = c['ref']['conf'].flatten(1), c['ref']['top']
        tied = (conf == top[:, None]).sum(1)
        for m in range(R.M_REG):
            kind = R.KINDS[m % 5]
            want = {'a': 2, 'b': 2, 'c': 625, 'd': 2, 'e': 5}[kind]
            assert int(tied[m]) >= want and (kind in 'de' or int(tied[m]) == want), (C, m, kind, int(tied[m]))
            if kind == 'd':
                assert float(top[m]) == 1.0
            else:
                assert int(c['ref']['first'][m]) == int(c['first'][m]), (C, m, kind)
            if kind == 'c':
                assert int(c['ref']['first'][m]) == 0 and abs(float(top[m]) * 625 - 1) < 1e-12
        assert bool(c['ref']['ok'].all())
        # the last tied cell differs from the first everywhere: a last-index rule is visible on every match
        assert bool((R.last_max(conf)[1] != c['ref']['first']).all())


@pytest.mark.parametrize('regime,dtype', CASES, ids=str)
def test_restatement_within_the_bound(regime, dtype):
    for C in R.regime_cs(regime, dtype):
        c = R.case(regime, dtype, C)
        mx, mean, flips = _restated_check(c)
        print(f'{regime} {dtype} C={C}: restatement error / bound max {mx:.4f} mean {mean:.5f}; bound up to {float(torch.nan_to_num(c["tol"]).max()):.2e} nats')
        assert mx <= 1.0 and mean <= 0.5 and flips == 0, (C, mx, mean, flips)
        if regime == 'ties':
            assert _restated_check(c, thr=1.0)[2] == 0


# mutation -> the regimes that must catch it, and how ('bound': error / bound > 1; 'flip': a clear decision differs)
CAUGHT_BY = {'one_sided': (('control', 'bound'), ('straddle', 'flip')),
             'scale_sqrtC': (('control', 'bound'), ('range', 'bound')),
             'no_max': (('range', 'bound'),),
             'prob_bf16': (('control', 'bound'), ('straddle', 'bound'), ('underflow', 'bound')),
             'tie_last': (('ties', 'flip'),),
             'ge_thr': (('ties@1', 'flip'),)}


@pytest.mark.parametrize('mut', sorted(CAUGHT_BY))
def test_every_mutation_is_caught(mut):
    """On every type and channel count of the named regime.  no_max overflows to inf / NaN in the range regime (counted as an infinite
    error); prob_bf16 is a 2^-8 relative error: visible everywhere but in the range regime, whose bound is wider than that;  ge_thr: the
    saturated windows of the ties regime at thr = 1.0 hold cells that are exactly 1.0 in every arithmetic (exp(0) / 1), which '>' rejects
    and '>=' accepts (at thr = 0 no such input exists: a global maximum is >= 1 / 625)."""
    for regime, how in CAUGHT_BY[mut]:
        name, thr = (regime.split('@')[0], 1.0) if '@' in regime else (regime, None)
        for dtype in R.TYPES:
            for C in R.regime_cs(name, dtype):
                mx, _, flips = _restated_check(R.case(name, dtype, C), thr=thr, mut=mut)
                assert (mx > 1.0) if how == 'bound' else (flips > 0), (mut, regime, dtype, C, mx, flips)
    if mut == 'no_max':
        assert _restated_check(R.case('range', R.H16, 128), mut=mut)[0] == math.inf
    if mut == 'ge_thr':
        c = R.case('ties', R.H16, 128)
        assert int(R.reference(c['f0'], c['f1'], 1.0)['ok'].sum()) == 0


@pytest.mark.parametrize('dtype', R.TYPES, ids=str)
def test_launch_edge_cases_are_clear(dtype):
    for M in R.EDGE_MS:
        for C in R.EDGE_CS:
            c = R.case('control', dtype, C, M)
            assert c['f0'].shape == (M, R.WW, C) and bool(R.clear(c['ref'], c['tol'], c['thr']).all()), (M, C)


@pytest.mark.parametrize('dtype,C', R.COMPACT_FORMS, ids=str)
@pytest.mark.parametrize('M,pattern', [(2125, 'mixed'), (2125, 'empty1'), (1025, 'mixed'), (1024, 'mixed'), (1025, 'none')])
def test_compaction_cases_and_model(M, pattern, dtype, C):
    """The accept pattern is the reference's decision on every match (all clear); the compaction model reproduces ascending match order, and
    ignoring the chunk base does not wherever a second chunk holds a match."""
    c = R.compaction_case(M, pattern, dtype, C)
    ref, acc = c['ref'], c['accept']
    assert bool(R.clear(ref, c['tol'], R.THR).all())
    assert torch.equal(ref['ok'], acc) and torch.equal(ref['first'][acc], (c['i'] * R.WW + c['j'])[acc])      # the accepted cell: the partner pair
    if pattern != 'none':
        assert bool(acc[1023]) and bool(acc[M - 1]) and not bool(acc[64:128].any()) and bool(acc[128:192].all())
        assert bool(acc[1024:2048].any()) == (pattern == 'mixed' and M > 1024)
    want = torch.nonzero(ref['ok'])[:, 0]
    assert torch.equal(R.compaction_order(ref['sel']), want)
    assert torch.equal(R.compaction_order(R.restated(c['f0'], c['f1'])[1]), want)
    assert torch.equal(R.compaction_order(ref['sel'], mut='chunk_base'), want) == (M <= 1024 or pattern == 'none')


@pytest.mark.parametrize('scaled', [True, False])
def test_keypoint_reference_is_the_oracle_in_float64(scaled):
    c = R.compaction_case(1025, 'mixed')
    ref = c['ref']
    kw = {'scale0': c['scale0'], 'scale1': c['scale1']} if scaled else {}
    mk0, mk1, b0, b1 = R.keypoints64(ref['sel'], c['b_ids'], c['mkpts0_c'], c['mkpts1_c'], **kw)
    data = {'b_ids': c['b_ids'], 'mkpts0_c': c['mkpts0_c'].double(), 'mkpts1_c': c['mkpts1_c'].double(),
            'hw0_i': (640, 640), 'hw0_c': (80, 80), 'hw0_f': (320, 320)}
    data.update({k: v.double() for k, v in kw.items()})
    o = O.fine_match(c['f0'].double(), c['f1'].double(), data, R.TEMP, R.THR)
    assert torch.allclose(o['fine_matrix'], ref['conf'], rtol=1e-11, atol=1e-300) and torch.equal(o['m_bids'], c['b_ids'][ref['ok']])
    assert torch.allclose(o['mkpts0_f'], mk0, rtol=1e-14, atol=0) and torch.allclose(o['mkpts1_f'], mk1, rtol=1e-14, atol=0)
    assert b0.shape == mk0.shape and b1.shape == mk1.shape and float(torch.minimum(b0 / mk0.abs(), b1 / mk1.abs()).min()) >= 4 * R.U32 * (1 - 1e-12)
