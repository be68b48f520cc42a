"""CPU checks of backward_regimes.py: the generators are deterministic and produce the regimes they claim, the written-out gradient formula
whose terms give the per-element scales IS autograd's gradient, the restatements are the reference formula once nothing is rounded and
round where they say, what they lose against float64 is what the table records, every mutation listed for a kept line exceeds that line's
device budget by a factor of two - those no line can catch are named, with the reason - and the three findings about the linear-attention
backward (the image without a valid key, fp16's range at cold q, the subnormal dden) as the restatement of the FORMER kernel shows them."""
import math

import pytest
import torch

import backward_regimes as B
import linear_attention_regimes as R

H16, BF16, F32 = B.H16, B.BF16, B.F32


def _id(e):
    return f'{e[0]}/{R.key(e[1], e[2])}/{R.NAME[e[3]]}'


def test_generators_deterministic():
    R._CACHE.clear()
    a = (B.la_case('few_keys', 6, H16, 300, 1280)[:4], B.law_case('ramp', None, BF16, 7, 25)[:4], B.fa_operands('range', H16, 37, 33),
         B.fm_operands('peaked', BF16, 64), B.act_case(H16, 255)[:2], (B.ln_case(128, BF16)['y'], B.ln_case(128, BF16)['dout']))
    R._CACHE.clear()
    b = (B.la_case('few_keys', 6, H16, 300, 1280)[:4], B.law_case('ramp', None, BF16, 7, 25)[:4], B.fa_operands('range', H16, 37, 33),
         B.fm_operands('peaked', BF16, 64), B.act_case(H16, 255)[:2], (B.ln_case(128, BF16)['y'], B.ln_case(128, BF16)['dout']))
    assert all(torch.equal(x, y) for s, t in zip(a, b) for x, y in zip(s, t))


# ------------------------------------------------------------------------------------------------------------------- references and regimes
@pytest.mark.parametrize('regime,variant,st', [('few_keys', 6, H16), ('sparse_v', None, BF16), ('cold_q', -12, H16), ('hot', None, BF16)], ids=str)
def test_linear_attention_scales_come_from_the_gradient_formula(regime, variant, st):
    """The formula of k_train.hip's header, in float64, is autograd's gradient of O.linear_attention (so the sums of its terms' absolute values
    are scales of THAT gradient), and no scale is smaller than the gradient it belongs to."""
    ref = B.la_case(regime, variant, st, *B.la_shapes(regime)[0])[-1]
    for nm in B.GRADS:
        g, s = ref[nm]
        assert bool(torch.isfinite(g).all()) and bool((s >= g.abs() * (1 - 1e-9)).all())
        assert float((ref['manual'][nm] - g).abs().max()) <= 1e-12 * float(s.max())
        assert float(((ref['manual'][nm] - g).abs() / s.clamp_min(1e-300))[s > 0].max()) < 1e-9


def test_regimes_are_what_they_claim():
    q, k, v, dout, qm, km, ref = B.la_case('few_keys', 6, H16, 300, 1280)
    assert tuple(int(c) for c in km.sum(1)) == R.FEW_KEYS and not bool(qm.all())
    # the image without a valid key and the masked rows: the float64 gradients and their scales are exact zeros
    assert all(float(ref[nm][0][3].abs().max()) == 0 and float(ref[nm][1][3].max()) == 0 for nm in B.GRADS)
    assert float(ref['dq'][1][0, 100:131].max()) == 0 and float(ref['dk'][1][1, 3:].max()) == 0
    for st in (H16, BF16):
        q, k, v, dout, qm, km, ref = B.la_case('cold_q', -12, st, 300, 520)
        assert float(q.float().max()) < 0 and bool(torch.isfinite(ref['dk'][0]).all()) and 1e-3 < float(ref['dk'][0].abs().max()) < 10
    assert float(B.la_case('hot', None, H16, 300, 520)[0].float().min()) > 0
    # full attention: one-hot, flat, the maximum in the last tile, exp2 arguments beyond fp32's exponent range on both sides
    for L, S in ((37, 33), (130, 97)):
        sm = lambda t: torch.softmax(torch.einsum('nlhd,nshd->nhls', B._split(t[0].double(), 4), B._split(t[1].double(), 4)) * 0.125, -1)   # noqa: E731
        peaked, flat = sm(B.fa_operands('peaked', BF16, L, S)), sm(B.fa_operands('flat', H16, L, S))
        assert float(peaked.amax(-1).min()) > 1 - 1e-9 and {int(i) for i in peaked.argmax(-1).unique()} == {0, 32, S - 1}
        assert float((flat * S - 1).abs().max()) < 1e-9
        lq, lk = B.fa_operands('late_max', H16, L, S)[:2]
        late = torch.einsum('nlhd,nshd->nhls', B._split(lq.double(), 4), B._split(lk.double(), 4))
        assert float((late.argmax(-1) >= 32 * ((S - 1) // 32)).double().mean()) > 0.9
        rq, rk = B.fa_operands('range', BF16, L, S)[:2]
        x = torch.einsum('nlhd,nshd->nhls', B._split(rq.double(), 4), B._split(rk.double(), 4)) * 0.125 * B.LOG2E
        assert float(x.max()) > 150 and float(x.min()) < -150 and float((x.amax(-1) - x.amin(-1)).max()) > 300
    # fine matching: one-hot confidences, and all equal
    for C in B.FM_C:
        assert float((B.fm_case('peaked', F32, C)[-1]['conf'].amax(-1) > 0.99).double().mean()) > 0.8
        assert float((B.fm_case('flat', F32, C)[-1]['conf'] * 625 - 1).abs().max()) < 1e-9
    # LayerNorm: the ratios, the constant row, the row of zeros
    for st in (H16, BF16):
        y = B.ln_case(256, st)['y'].double()
        r = R.mean_over_std(y[3:])
        for i, want in enumerate(B.LN_RATIOS[st]):
            assert abs(float(r[i::7].median()) / want - 1) < 0.1
        assert float(y[0].std()) == 0 and float(y[2].abs().max()) == 0
    assert B.LN_T[2] > 4 * B.LN_BWD_WGS > B.LN_T[1] and B.LN_T[0] < 8


@pytest.mark.parametrize('entry', ['la', 'law', 'ln', 'fa', 'fm'])
def test_restatement_without_rounding_is_the_reference(entry):
    """With fp32 as the 'storage type' nothing is rounded and every restatement is the reference formula in fp32: within a few ulps OF FP32
    of float64 at the terms' scale - the restatements differ from the references by their rounding points and by nothing else."""
    if entry == 'la':
        q, k, v, dout, qm, km, ref = B.la_case('few_keys', 2, BF16, 300, 1280)
        errs = B.grad_errors(B.la_backward_restated(q, k, v, dout, F32, 8, qm, km), ref, F32)
    elif entry == 'law':
        q, k, v, dout, ref = B.law_case('control', None, BF16, 7, 25)
        errs = B.grad_errors(B.la_backward_restated(q, k, v, dout, F32, 8, form='window'), ref, F32)
    elif entry == 'ln':
        case = B.ln_case(256, BF16)
        got = B.ln_restated(256, F32, case=case)
        errs = tuple(B.term_error(got[nm], *case['ref'][max(B.LN_T)][nm], F32) for nm in B.LN_OUT)
    elif entry == 'fa':
        q, k, v, dout, ref = B.fa_case('control', BF16, 130, 97)
        got = B.fa_restated(q, k, v, dout, F32)
        errs = tuple(B.term_error(got[nm], ref[nm][0], ref[nm][1], F32) for nm in B.FA_OUT)
    else:
        f0, f1, dconf, ref = B.fm_case('control', BF16, 128)
        errs = B.fm_errors(B.fm_restated(f0, f1, dconf, F32), ref, F32)
    print(entry, errs)
    assert max(e[0] for e in errs) < 16 and max(e[1] for e in errs) < 1.5


@pytest.mark.parametrize('st', [H16, BF16])
def test_restatements_round_where_they_say(st):
    """Every output is a value of the storage type; the operand roundings are in force (the fp32 evaluation differs); the masks SELECT."""
    q, k, v, dout, qm, km, ref = B.la_case('few_keys', 6 if st == H16 else 2, st, 300, 1280)
    got = B.la_backward_restated(q, k, v, dout, st, 8, qm, km)
    plain = B.la_backward_restated(q, k, v, dout, F32, 8, qm, km)
    for x, y in zip(got, plain):
        assert torch.equal(R.rt(x, st), x) and not torch.equal(x, R.rt(y, st))
    assert float(got[0][~qm].abs().max()) == 0 and float(got[1][~km].abs().max()) == 0 and float(got[2][~km].abs().max()) == 0
    assert all(float(x[3].abs().max()) == 0 for x in got)
    q, k, v, dout, ref = B.fa_case('control', st, 37, 33)
    fa = B.fa_restated(q, k, v, dout, st)
    assert all(torch.equal(R.rt(fa[nm], st), fa[nm]) for nm in ('out', 'dq', 'dk', 'dv')) and fa['lse2'].dtype == torch.float32
    ln = B.ln_restated(128, st)
    assert torch.equal(R.rt(ln['out'], st), ln['out']) and torch.equal(R.rt(ln['dy'], st), ln['dy']) and float(ln['mean'][0]) == 3.25
    assert float(ln['rstd'][0]) == pytest.approx(B.LN_EPS ** -0.5, rel=1e-6)       # the constant row: variance 0


# ------------------------------------------------------------------------------------------------------------------- the table
@pytest.mark.parametrize('entry', B.entries(), ids=_id)
def test_restatement_table(entry):
    """What the restatement alone loses against float64 is what REST records: never more, and REST is the measurement rounded up, not slack.
    A kept line is finite."""
    got, rec = B.restatement_error(*entry), B.rest(*entry)
    print(_id(entry), 'measured', got, 'recorded', rec)
    assert len(got) == len(rec)
    for g, r in zip(got, rec):
        assert math.isfinite(g[0]) and g[0] <= r[0] and g[1] <= r[1], (got, rec)
        assert r[0] <= 1.3 * g[0] + 0.1 and r[1] <= 1.3 * g[1] + 0.005, (got, rec)


# ------------------------------------------------------------------------------------------------------------------- mutations
def listed(entry):
    """The mutations a kept (entry, regime, variant, type) must expose."""
    e, regime, _, st = entry
    if e == 'la':
        return (('drop_dden', 'swap_heads') + (('eps_dropped', 'mask_v_only') if regime == 'few_keys' else ()) + (('mask_v_only',) if regime == 'wide_v' else ())
                + (('swap_halves',) if regime == 'ramp' else ()) + (('inv_valid',) if (regime, st) == ('sparse_v', H16) else ())
                + (('z_in_operand',) if (regime, st) in (('few_keys', H16), ('cold_q', H16)) and entry[2] != -12 else ()))
    if e == 'law':
        return ('drop_dden', 'no_diag') + (('z_in_operand',) if (regime, entry[2], st) == ('cold_q', -14, H16) else ())
    if e == 'ln':
        return B.LN_MUTATIONS
    if e == 'fa':
        return ('odd_tiles_dropped',) if regime == 'peaked' else ('lse_natural_log', 'odd_tiles_dropped', 'tail_keys_counted')
    return B.FM_MUTATIONS


# mutations no kept line exposes, and why (findings, not failures)
NOT_CAUGHT = {
    # phi is x + 1 | exp(x) and phi' is 1 | exp(x): both branches give 1 at x = 0, so WHICH branch takes x == 0 changes no bit
    ('la', 'phi_prime_at_zero'): 'identical bits', ('law', 'phi_prime_at_zero'): 'identical bits',
    # phi(k) is zero on a masked row, so an unmasked finite v multiplies zero in the state, and the source pass selects by the mask
    ('la', 'mask_k_only'): 'identical bits',
    # the kernel no longer has a rounded dnum (z_in_operand is the former form, dnum_unrounded that form with dnum left in fp32): no line tells
    # the two apart - where the former form is over a budget (hot in fp16: its subnormal dden) both are, by the same factor
    ('la', 'dnum_unrounded'): 'not a property of the kernel',
    # P and dS in fp32, delta from the un-rounded output: the more accurate forms stay inside a budget recorded from the rounded ones
    ('fa', 'p_unrounded'): 'more accurate than the restatement', ('fa', 'delta_from_unrounded_out'): 'more accurate than the restatement',
}


def _factor(entry, mut):
    """max over the entry's outputs of (mutant's error / budget), max and mean alike."""
    e = B.restatement_error(*entry, mut=mut)
    return max(max(x[0] / b[0], x[1] / b[1]) for x, b in zip(e, B.budgets(*entry))), e


def test_every_mutation_is_listed():
    for e, muts in (('la', B.LA_MUTATIONS), ('law', B.LAW_MUTATIONS), ('ln', B.LN_MUTATIONS), ('fa', B.FA_MUTATIONS), ('fm', B.FM_MUTATIONS)):
        seen = {m for ent in B.entries() if ent[0] == e for m in listed(ent)}
        missing = {m for m in muts if (e, m) in NOT_CAUGHT}
        assert seen | missing >= set(muts) - ({'z_in_operand'} if e == 'law' else set()), (e, set(muts) - seen - missing)
        assert not seen & missing


@pytest.mark.parametrize('entry', B.entries(), ids=_id)
def test_listed_mutations_exceed_the_device_budget(entry):
    """The condition under which a line is kept: the restatement fits its own budget, and every mutation listed for the line is over the
    budget by a factor of two, in the maximum or in the mean of at least one output."""
    assert _factor(entry, None)[0] <= 1.0
    for mut in listed(entry):
        f, e = _factor(entry, mut)
        print(_id(entry), mut, 'over budget by', f)
        assert f >= 2.0, (mut, f, e)


def test_mutations_no_line_exposes():
    for (e, mut), why in NOT_CAUGHT.items():
        lines = [ent for ent in B.entries() if ent[0] == e]
        if why == 'identical bits':
            pick = [ent for ent in lines if ent[1] in ('control', 'few_keys', 'wide_v', 'sparse_v')]
            assert pick and all(B.restatement_error(*ent, mut=mut) == B.restatement_error(*ent) for ent in pick)
        else:
            if mut == 'dnum_unrounded':
                assert all(_factor(ent, mut)[0] <= 1.05 * max(1.0, _factor(ent, 'z_in_operand')[0]) for ent in lines)
                continue
            worst = max(_factor(ent, mut)[0] for ent in lines)
            print(e, mut, 'worst factor over the device budget', worst)
            assert worst < 2.0
    # 1 / (valid keys) in place of 1 / S cancels in the gradient as in the message: it shows only where the padded length keeps fp16 finite
    rest = [ent for ent in B.entries() if ent[0] == 'la' and (ent[1] in ('few_keys', 'wide_v') or (ent[1], ent[3]) == ('sparse_v', BF16))]
    assert len(rest) >= 6 and max(_factor(ent, 'inv_valid')[0] for ent in rest) < 2.0
    assert _factor(('la', 'sparse_v', None, H16), 'inv_valid')[0] == math.inf


# ------------------------------------------------------------------------------------------------------------------- the findings
def _former(regime, variant, st, form='coarse'):
    """(errors of the former kernel's restatement, of the present one) - z_in_operand: dnum = dout S / den and dden as 16-bit operands."""
    return tuple(B.restatement_error('la' if form == 'coarse' else 'law', regime, variant, st, mut=m) for m in ('z_in_operand', None))


def test_finding_image_without_valid_keys():
    """few_keys, fp16: den = eps, S / den = 1.3e9 is inf in fp16 and inf times the zero state is NaN in dq; dk, dv were saved by the mask.
    bf16 has the range.  With z applied in fp32 after the product every gradient of that image is an exact zero in both types."""
    old, new = _former('few_keys', 6, H16)
    assert old[0] == (math.inf, math.inf) and math.isfinite(old[1][0]) and math.isfinite(old[2][0]) and all(math.isfinite(e[0]) for e in new)
    q, k, v, dout, qm, km, _ = B.la_case('few_keys', 6, H16, 300, 1280)
    was = B.la_backward_restated(q, k, v, dout, H16, 8, qm, km, mut='z_in_operand')
    assert bool(torch.isnan(was[0][3]).any()) and bool(torch.isfinite(was[0][:3]).all())
    assert all(math.isfinite(e[0]) for e in _former('few_keys', 2, BF16)[0])


def test_finding_fp16_range_at_cold_q():
    """The former forms round dnum = dout S / den and dden = -(dout . num) S / den^2 to fp16.  Coarse: finite at -12 and at -13 (dden is of order 10
    there: the small dout . num ~ phi(q) cancels one factor 1 / den; the predicted loss of range between -12 and -13 is NOT reproduced), inf at -14
    (S / den = 4e4 times |dout| up to 4).  Window: finite at -12, inf from -13.  The float64 gradients stay of order 0.05 throughout, and the
    present forms are finite to -16; what grows there is the FORWARD's limit (phi(q) itself an fp16 subnormal)."""
    assert all(math.isfinite(e[0]) for e in _former('cold_q', -12, H16)[0] + _former('cold_q', -13, H16)[0] + _former('cold_q', -12, H16, 'window')[0])
    for off, form in ((-14, 'coarse'), (-16, 'coarse'), (-13, 'window'), (-16, 'window')):
        old, new = _former('cold_q', off, H16, form)
        print('cold_q', off, form, 'former', old, 'present', new)
        assert any(e[0] == math.inf for e in old) and all(math.isfinite(e[0]) for e in new)
    ref = B.la_case('cold_q', -14, H16, 300, 520)[-1]
    assert 1e-3 < float(ref['dk'][0].abs().max()) < 1.0


def test_finding_subnormal_dden():
    """At nominal inputs dden is about 1e-6, an fp16 subnormal.  What it cost the former form on dk, at the terms' scale (fp16, ulps: max, mean):
    control 0.062 / 0.0074 against 0.051 / 0.0064 now - nothing; hot 0.58 / 0.125 against 0.041 / 0.0053 - a factor of twenty in the mean (dKsum
    carries most of dk there); the window form's dv at hot 27.7 / 0.34 against 1.63 / 0.067."""
    dden = B.la_case('control', None, H16, 300, 520)[-1]['dden'].abs()
    assert 1e-7 < float(dden.median()) < 2.0 ** -14
    old, new = _former('control', None, H16)
    assert old[1][1] < 1.5 * new[1][1] + 0.002
    old, new = _former('hot', None, H16)
    assert old[1][1] > 10 * new[1][1] and new[1][1] < 0.01
    old, new = _former('hot', None, H16, 'window')
    assert old[2][0] > 10 * new[2][0]
