"""CPU checks of linear_regimes.py: the generators are deterministic and produce the regimes they claim, the restatement rounds where it says
and is bit-equal to float64 rounded once in the exact regime, what it loses against float64 is what the table records, and every wrong kernel
in linear_regimes.MUTATIONS exceeds the device budget of the lines named for it - those that no line can tell apart are named, with the
figures.  The refusal of a row-group bias on a ragged column tile is checked at the entry points, which decide before anything is launched."""
import math

import pytest
import torch

import linear_regimes as L

H16, BF16, F32 = L.H16, L.BF16, L.F32


def _line(text):
    form, regime, st = text.split('/')
    by_key = {L.key(r, v): (r, v) for r, v in L.FORMS[form][1]}
    return (form,) + by_key[regime] + ({v: k for k, v in L.NAME.items()}[st],)


def test_generators_deterministic():
    picks = [('ln', 'ln_offset', 100, H16, 1), ('rgbias', 'rgbias_cancelling', None, BF16, 0), ('upadd', 'up_ties', None, H16, 0), ('rows', 'control', None, BF16, 2)]
    def make():
        L.R._CACHE.clear()
        cases = [L.cached_case(L.specs(f, st, r)[i], r, v, st) for f, r, v, st, i in picks]
        return [c[k] for c in cases for k in ('a', 'w', 'ref')]
    assert all(torch.equal(x, y) for x, y in zip(make(), make()))


def test_regimes_are_what_they_claim():
    pre = lambda c: c['a'].double() @ c['w'].double().T + (0 if c['bias'] is None else c['bias'].double())     # noqa: E731
    for st in L.ALL:
        for ratio in (10, 100, 1000):
            for sp in L.specs('ln', st):
                r = L.R.mean_over_std(pre(L.cached_case(sp, 'ln_offset', ratio, st)))
                assert abs(float(r.median()) / ratio - 1) < 0.15
        for sp in L.specs('ln', st):
            x = pre(L.cached_case(sp, 'ln_flat', -5, st))
            var = x.var(-1, unbiased=False)
            assert float(var.max()) < 1e-6 and bool((var[::5] == 0).all()) and bool((var[1::5] > 0).all())
            for v in (-12, 17):
                mag = float(pre(L.cached_case(sp, 'ln_range', v, st)).abs().median()) / 2.0 ** v
                assert 0.3 < mag < 1.5
        span = pre(L.cached_case(L.specs('tanh2', st)[0], 'tanh_span', None, st)).abs()
        assert float(span.max()) > 59 and float(span[span > 0].min()) <= 2.0 ** -19
        for sp in L.specs('rgbias', st):
            c = L.cached_case(sp, 'rgbias_dominant', None, st)
            assert float(c['rgb'].double().abs().median()) > 20 * float((c['a'].double() @ c['w'].double().T).abs().median())
            c = L.cached_case(sp, 'rgbias_cancelling', None, st)
            repeat = torch.arange(300) % 3 != 1
            assert float((c['ref'][repeat].abs() / c['scale'][repeat]).max()) < 2 * L.EPS[st]
    # exact: every product and every sum of products is a multiple of 1 / 8 far below 2^24 eighths, the results inside fp16's range
    for form, _, _, st in L.lines(exact=True):
        for sp in L.specs(form, st):
            c = L.cached_case(sp, 'exact', None, st)
            assert bool((c['a'].double() * 1 == c['a'].double().round()).all()) and bool(((c['w'].double() * 8) == (c['w'].double() * 8).round()).all())
            assert float(c['scale'].max()) * 8 < 2 ** 24 and float(c['ref'].abs().max()) < 60000
    # the counts of rows_groups: tile 1 holds no wanted row, its neighbours do; a 128-row tile straddles groups of 25
    done = L.tile_rows_computed(L.GROUP_COUNTS, 300)
    assert bool(done[:128].all()) and not bool(done[128:256].any()) and bool(done[256:].all()) and 128 % L.GROUP_R
    assert not bool(L.tile_rows_computed(L.GROUP_COUNTS[:6], 150)[128:].any())
    # the flags change inside a 32-row wave, and every upadd path has its shape
    assert any(sp['fr'] == 7 for sp in L.specs('ln_res', H16)) and L.FLAG_PATTERN.count(0) >= 2
    geoms = [sp['geom'] for sp in L.specs('upadd', H16)]
    assert {g[2] for g in geoms} >= {5, 31, 32, 33} and any(g[1] == 1 for g in geoms) and any(g[3] == 1 and g[4] == 1 for g in geoms)
    assert any(g[0] > 1 and g[2] >= 32 and (g[1] * g[2]) % 32 for g in geoms) and any(g[0] > 1 and g[2] < 32 and (g[1] * g[2]) % 32 for g in geoms)


@pytest.mark.parametrize('st', [H16, BF16])
def test_restatement_rounds_where_it_says(st):
    """Outputs are values of the storage type; a zero-variance row is round(beta); a skipped row is the residual; the two roundings of the
    16-bit LN_RES are in force."""
    for form, regime, variant in (('plain', 'control', None), ('tanh2', 'tanh_span', None), ('ln', 'ln_flat', -5), ('ln_res', 'control', None), ('upadd', 'control', None)):
        for sp in L.specs(form, st, regime):
            case = L.cached_case(sp, regime, variant, st)
            out = L.restated(case)
            assert torch.equal(L.rt(out, st), out) and bool(torch.isfinite(out).all())
            if regime == 'ln_flat':
                assert torch.equal(out[::5], L.rt(case['beta'], st).expand_as(out[::5]))
            if form == 'ln_res':
                skip = ~L.keep_rows(case)
                assert torch.equal(out[skip], case['res'].float()[skip])
                assert sp['fr'] == 1000 or not torch.equal(out, L.restated(case, 'res_single_round'))


@pytest.mark.parametrize('line', L.lines(), ids=L.line_id)
def test_restatement_table(line):
    """What the restatement alone loses against float64 is what REST records: never more (so it is inside its own budget), and REST is the
    measurement rounded up, not slack.  A kept line is finite."""
    got, rec = L.restatement_error(*line), L.rest(*line)
    print(L.line_id(line), 'measured', got, 'recorded', rec, 'budget', L.budget(rec))
    assert math.isfinite(got[0]) and got[0] <= rec[0] and got[1] <= rec[1], (got, rec)
    assert rec[0] <= 1.3 * got[0] + 0.1 and rec[1] <= 1.3 * got[1] + 0.005, (got, rec)


def test_table_has_no_other_lines():
    assert set(L.REST) == {L.line_id(line) for line in L.lines()}


@pytest.mark.parametrize('line', L.lines(exact=True), ids=L.line_id)
def test_exact_restatement_is_float64_rounded_once(line):
    assert L.exact_mismatches(line[0], line[3]) == 0


# ------------------------------------------------------------------------------------------------------------------- mutations
ALL3, B16 = ('fp32', 'fp16', 'bf16'), ('fp16', 'bf16')
_each = lambda names, types: tuple(f'{n}/{t}' for n in names for t in types)     # noqa: E731
# mutation -> the lines whose device budget it exceeds (max or mean), every one of them checked below
CAUGHT = {
    'ln_unbiased': _each(('ln/control',), ALL3),
    'ln_no_eps': _each(('ln/ln_flat-5', 'ln/ln_flat-3'), ALL3),
    'ln_one_pass': _each(('ln/ln_offset+1000',), ALL3),
    'ln_stats_rounded': _each(('ln/ln_offset+100', 'ln/ln_offset+1000'), B16),
    'bias_after_act': _each(('relu2/control', 'relu2_nb4/control', 'tanh2/control', 'tanh_nb4/control'), ALL3),
    'acc_rounded_per_step': _each(('rgbias/rgbias_cancelling',), B16),
    'k_tail_dropped': _each(('plain/control', 'plain_wide/control'), ALL3) + _each(('rows/control', 'conv_s1/control', 'conv_s2/control', 'upadd/control'), B16),
    'a2_from_k1': _each(('relu2/control', 'relu2_nb4/control', 'tanh2/control'), ALL3),
    'rgbias_next_group': _each(('rgbias/control', 'rgbias/rgbias_dominant'), ALL3),
    'rgbias_after_round': _each(('rgbias/rgbias_cancelling',), B16),
    'flag_per_tile': _each(('ln_res/control', 'ln_res/res_dominant', 'ln_res/res_tiny'), ALL3),
    'up_taps_rounded': _each(('upadd/up_ties',), B16),
}
# ... and the exact lines whose bits it changes
CAUGHT_EXACT = {
    'acc_rounded_per_step': _each(('plain/exact', 'plain_wide/exact', 'relu2/exact', 'relu2_nb4/exact', 'rows/exact', 'conv_s1/exact', 'conv_s2/exact'), B16),
    'k_tail_dropped': _each(('plain/exact', 'plain_wide/exact', 'relu2/exact', 'relu2_nb4/exact'), ALL3) + _each(('rows/exact', 'conv_s1/exact', 'conv_s2/exact'), B16),
    'a2_from_k1': _each(('relu2/exact', 'relu2_nb4/exact'), ALL3),
    'bias_after_act': _each(('relu2/exact', 'relu2_nb4/exact'), ALL3),
}
# Mutations no line tells apart within its budget, and why (findings about the unit, not failures): each is ONE more - or one fewer - rounding
# to the storage type, at most half an ulp, against a margin of two ulps on the maximum and a mean that the final rounding already fills.
NOT_TOLD_APART = {
    # ReLU commutes with rounding: identical bits.  Tanh of the rounded pre-activation is a second rounding where tanh' ~ 1 (the worst line:
    # 0.96 ulp maximum against 2.5, 0.21 ulp mean against 0.31) and none where it saturates; no steering of x changes that - a rounded x is
    # itself a value the storage type holds, and tanh maps it within a few parts in 2^11 of one
    'act_after_round': 'a second rounding: at most one ulp',
    # what the 16-bit kernel does NOT do (it rounds the LayerNorm value, then the sum): the single rounding is the MORE accurate form and
    # stays inside a budget recorded from the two roundings
    'res_single_round': 'more accurate than the restatement',
}


def _factor(line, mut):
    e, b = L.restatement_error(*line, mut=mut), L.line_budget(*line)
    return max(e[0] / b[0], e[1] / b[1]), e, b


def test_every_mutation_is_listed():
    assert set(CAUGHT) | set(NOT_TOLD_APART) == set(L.MUTATIONS) and not set(CAUGHT) & set(NOT_TOLD_APART)
    assert set(CAUGHT_EXACT) <= set(CAUGHT)


@pytest.mark.parametrize('mut', sorted(CAUGHT))
def test_mutation_exceeds_the_budget_of_its_lines(mut):
    for text in CAUGHT[mut]:
        f, e, b = _factor(_line(text), mut)
        print(mut, text, 'error', e, 'budget', b, 'over by', f)
        assert f > 1.0, (mut, text, e, b)
    for text in CAUGHT_EXACT.get(mut, ()):
        line = _line(text)
        bad = L.exact_mismatches(line[0], line[3], mut)
        print(mut, text, 'elements that are not float64 rounded once:', bad)
        assert bad > 0, (mut, text)


def test_mutations_no_line_tells_apart():
    for mut in NOT_TOLD_APART:
        worst = max((_factor(line, mut)[0], L.line_id(line)) for line in L.lines())
        print(mut, 'worst factor over a device budget', worst)
        assert worst[0] < 1.0
    for st in L.ALL:                                            # ReLU after the rounding: the same bits
        for form in ('relu2', 'relu2_nb4'):
            for sp in L.specs(form, st):
                case = L.cached_case(sp, 'control', None, st)
                assert torch.equal(L.restated(case, 'act_after_round'), L.restated(case))
    # the single rounding of LN_RES is never further from float64 than the two, in the mean
    for st in (H16, BF16):
        for regime in ('control', 'res_dominant', 'res_tiny'):
            assert L.restatement_error('ln_res', regime, None, st, 'res_single_round')[1] <= L.restatement_error('ln_res', regime, None, st)[1]


# ------------------------------------------------------------------------------------------------------------------- the refusal
@pytest.mark.parametrize('N', [160, 224, 96])
def test_rowgroup_bias_needs_whole_column_tiles(N):
    """gf_linear and gf_linear_rows check their arguments before they touch the device: a row-group bias with N % 128 != 0 is an error (the
    epilogue would read the last column tile's 128 entries, up to 96 of them behind the row - in the last group behind the table), and the
    same call with N = 128, 256 or 384 gets past that check."""
    from geoformer_amd import _lib
    h = _lib.lib()
    fake = 4096                                                  # never dereferenced: the argument checks come first
    for dtype in (0, 1, 2):
        assert h.gf_linear(fake, 64, 64, None, 0, 0, fake, None, fake, 25, 0, None, None, 1e-5, None, 0, None, 0, fake, N, dtype, 50, N, None) == -1
        assert b'multiple of 128' in h.gf_last_error()
    for dtype in (1, 2):
        assert h.gf_linear_rows(fake, 16, None, 0, 0, 64, fake, None, fake, 25, 0, None, None, 1e-5, None, 0, None, 0, fake, N, dtype, 50, N, None) == -1
        assert b'multiple of 128' in h.gf_last_error()
    # the check is about the row-group bias alone: rowgroup_rows = 0 with a bias of whole tiles is the older error, not this one
    assert h.gf_linear(fake, 64, 64, None, 0, 0, fake, None, fake, 0, 0, None, None, 1e-5, None, 0, None, 0, fake, 128, 1, 50, 128, None) == -1
    assert b'rowgroup_rows' in h.gf_last_error()
