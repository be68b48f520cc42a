"""K2, K9 and K11 against float64 in the regimes of tests/linear_attention_regimes.py: offsets that put phi on one branch, phi(q) or the
state next to the fp16 subnormals or just below fp16 overflow, a few valid keys among 1280, heads and channels that do not look alike,
LayerNorm rows far from centred, a saturated tanh.

The reference is the float64 evaluation of the reference arithmetic on the kernel's own operands; the budget of every line is what the
restatement with the kernel's rounding points loses against float64 (linear_attention_regimes.REST, measured on the CPU by
tests/test_linear_attention_regimes.py) plus the stated margin (budget(): + 2 ulp on the maximum, 1.5 x + 0.05 ulp on the mean).  No element
is left out; rows a mask removes must be exact zeros; nothing may be inf or NaN; two launches give the same bits.  Which wrong kernels
these lines would catch is what the CPU file's mutation tests state."""
import pytest
import torch

import linear_attention_regimes as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H16, BF16, F32 = R.H16, R.BF16, R.F32


def _ids(p):
    return R.NAME.get(p, str(p))


def _dev(t, st=None):
    """To the device; a case's x / src / msg hold values already rounded to the storage type, as fp32: cast them (exact)."""
    return None if t is None else (t.to(DEV) if st is None else t.to(DEV).to(st))


def _layer(P, c, nhead, attention='linear', activation='relu'):
    from geoformer_amd.model.modules import LoFTREncoderLayer
    m = LoFTREncoderLayer(c, nhead, attention, activation)          # a fresh layer per regime: layer.weights(st) caches the packed streams
    m.load_state_dict(P)
    return m.to(DEV)


def _within(err, bud, what):
    print(what, 'error (max, mean) = (%.3f, %.4f) ulp, budget (%.3f, %.4f)' % (err + bud))
    assert err[0] <= bud[0] and err[1] <= bud[1], (what, err, bud)


def _twice(fn):
    with torch.no_grad():
        a, b = fn(), fn()
    assert torch.equal(a, b), 'two launches differ'
    assert bool(torch.isfinite(a).all())
    return a


# ------------------------------------------------------------------------------------------------------------------- K2
_K2 = [(r, v, st) for (r, v), types in R.COARSE.items() if r in R.ATTENTION_ONLY for st in types] + [('control', None, F32), ('hot', None, F32)]


@pytest.mark.parametrize('regime,variant,st', _K2, ids=_ids)
def test_k2_coarse_kernel(regime, variant, st):
    """ops.linear_attention at N = 3 or 4, L = 300, S = 1280, 8 heads of 32: la16_kv / la16_apply (16-bit), la_kv_partial / la_apply (fp32)."""
    from geoformer_amd import ops
    q, k, v, xm, sm, ref, A = R.cached_k2(regime, variant, st)
    got = _twice(lambda: ops.linear_attention(q.to(DEV), k.to(DEV), v.to(DEV), 8, _dev(xm), _dev(sm)))
    assert got.dtype == st
    _within(R.message_error(got, ref, A, st), R.budget(R.rest('k2', regime, variant, st)), f'k2 {R.key(regime, variant)} {R.NAME[st]}')


@pytest.mark.parametrize('regime,variant,st', [(r, v, st) for (r, v), types in R.FINE.items() if r != 'ln_offset' for st in types], ids=_ids)
def test_k2_window_kernel(regime, variant, st):
    """ops.linear_attention on windows of <= 32 tokens, 8 heads of 16 (la_window_mfma), 1 / S = 1 / 25, 1 / 17, 1 / 32."""
    from geoformer_amd import ops
    worst = (0.0, 0.0)
    for shape in R.WINDOW_SHAPES:
        q, k, v, ref, A = R.cached_window(regime, variant, st, *shape)
        got = _twice(lambda: ops.linear_attention(q.to(DEV), k.to(DEV), v.to(DEV), 8))
        e = R.message_error(got, ref, A, st)
        worst = (max(worst[0], e[0]), max(worst[1], e[1]))
    _within(worst, R.budget(R.rest('k2w', regime, variant, st)), f'k2w {R.key(regime, variant)} {R.NAME[st]}')


# ------------------------------------------------------------------------------------------------------------------- K9
@pytest.mark.parametrize('regime,variant,st', [(r, v, st) for (r, v), types in R.COARSE.items() for st in types], ids=_ids)
def test_k9_layer(regime, variant, st):
    """LoFTREncoderLayer.forward, fused form (gf_encoder_kv_state + gf_encoder_layer): three images of 300 queries (two full 128-token tiles
    and a ragged third) on 1280 keys (ten source tiles, 1 / S no power of two); control also at L = 256 and at S = 200 < L."""
    worst = (0.0, 0.0)
    for L, S in R.coarse_shapes(regime):
        case, ref = R.cached_coarse(regime, variant, st, L, S)
        layer = _layer(case['P'], 256, 8)
        x, src, xm, sm = _dev(case['x'], st), _dev(case['src'], st), _dev(case['xm']), _dev(case['sm'])
        assert layer.fusable(st)
        got = _twice(lambda: layer(x, src, xm, sm))
        e = R.output_error(got, ref, st)
        worst = (max(worst[0], e[0]), max(worst[1], e[1]))
    _within(worst, R.budget(R.rest('k9', regime, variant, st)), f'k9 {R.key(regime, variant)} {R.NAME[st]}')


_STATE = [('control', None, H16), ('control', None, BF16), ('hot', None, H16), ('cold_k', -8, H16), ('cold_k', -8, BF16), ('cold_k', -12, BF16),
          ('few_keys', 6, H16), ('few_keys', 2, BF16), ('few_keys', -8, BF16), ('wide_v', None, H16), ('wide_v', None, BF16),
          ('sparse_v', None, H16), ('sparse_v', None, BF16), ('ramp', None, BF16)]


@pytest.mark.parametrize('regime,variant,st', _STATE, ids=_ids)
def test_k9_state_per_entry(regime, variant, st):
    """fused.encoder_kv_state entry by entry against float64: Ksum (a sum of positive terms) to a relative bound, KV against
    sum_s |phi(k_s) v_s| (linear_attention_regimes.state_reference) - not against the largest entry of the state."""
    from geoformer_amd import fused
    case, _ = R.cached_coarse(regime, variant, st)
    layer = _layer(case['P'], 256, 8)
    w = layer.weights(st)
    state = _twice(lambda: fused.encoder_kv_state(_dev(case['src'], st), w['stream_kv'], _dev(case['sm'])))
    kv, ks = R.state_check(state, case)
    print(f'state {R.key(regime, variant)} {R.NAME[st]}: worst |error| / bound  KV {kv:.3f}  Ksum {ks:.3f}')
    assert kv <= 1.0 and ks <= 1.0
    rkv, rks = R.state_check(R.state_restated(case), case)                          # the restatement fits its own bound
    assert rkv <= 1.0 and rks <= 1.0


@pytest.mark.parametrize('regime,variant,st,tail_first', [('cold_k', -8, H16, 0), ('cold_k', -12, BF16, 1), ('few_keys', 6, H16, 1), ('few_keys', -8, BF16, 0)],
                         ids=_ids)
def test_k9_state_tail(regime, variant, st, tail_first):
    """gf_encoder_layer_kv: the layer's output keeps its bits with the tail, and the states the tail leaves for the images tail_first.. -
    the finished rows under the consumer's k / v weights (here the same regime's), the query mask as the source mask - are within the
    same per-entry bound."""
    case, ref = R.cached_coarse(regime, variant, st)
    layer, consumer = _layer(case['P'], 256, 8), _layer(case['P'], 256, 8)
    x, src, xm, sm = _dev(case['x'], st), _dev(case['src'], st), _dev(case['xm']), _dev(case['sm'])
    with torch.no_grad():
        state = layer.kv_state(src, sm)
        plain = layer.forward_state(x, state, src.shape[1], xm)
        out, tail = layer.forward_state(x, state, src.shape[1], xm, tail_layer=consumer, tail_first=tail_first)
    assert torch.equal(out, plain)
    _within(R.output_error(out, ref, st), R.budget(R.rest('k9', regime, variant, st)), f'k9 with tail {R.key(regime, variant)} {R.NAME[st]}')
    rows = out[tail_first:].float().cpu()
    kv, ks = R.state_check(tail, case, rows, None if case['xm'] is None else case['xm'][tail_first:])
    print(f'tail state {R.key(regime, variant)} {R.NAME[st]}: worst |error| / bound  KV {kv:.3f}  Ksum {ks:.3f}')
    assert kv <= 1.0 and ks <= 1.0


@pytest.mark.parametrize('st', [H16, BF16], ids=_ids)
def test_k9_finish_tanh_saturated(st):
    """layer.finish (the Geo form: attention output given, tanh MLP, skip flags) with pre-activations beyond +-90: tanh as
    1 - 2 rcp(exp(2 x) + 1) meets exp = inf and exp = 0; the skipped sample is copied bit for bit."""
    case, ref, _ = R.cached_tanh(st)
    layer = _layer(case['P'], 256, 4, 'full', 'tanh')
    x, msg, flag = _dev(case['x'], st), _dev(case['msg'], st), case['flag'].to(DEV)
    got = _twice(lambda: layer.finish(x, msg, flag, x.shape[1]))
    assert torch.equal(got[1], x[1])
    _within(R.output_error(got, ref, st), R.budget(R.rest('k9tanh', 'tanh_sat', None, st)), f'k9 finish tanh {R.NAME[st]}')


# ------------------------------------------------------------------------------------------------------------------- K11
@pytest.mark.parametrize('regime,variant,st', [(r, v, st) for (r, v), types in R.FINE_LAYER.items() for st in types], ids=_ids)
def test_k11_fine_layer(regime, variant, st):
    """gf_fine_layer, self (src is x) and cross forms, window counts that leave spare waves in a group (37, 3, 5, 9), full 32-token windows
    and short ones; 1 / S = 1 / Lw."""
    worst = (0.0, 0.0)
    for Nw, Lw, cross in R.fine_shapes(regime):
        case, ref = R.cached_fine(regime, variant, st, Nw, Lw, cross)
        layer = _layer(case['P'], 128, 8)
        x = _dev(case['x'], st)
        src = _dev(case['src'], st) if cross else x
        assert layer.fusable_window(st, Lw)
        got = _twice(lambda: layer(x, src))
        assert got.shape == (Nw, Lw, 128) and got.dtype == st
        e = R.output_error(got, ref, st)
        worst = (max(worst[0], e[0]), max(worst[1], e[1]))
    _within(worst, R.budget(R.rest('k11', regime, variant, st)), f'k11 {R.key(regime, variant)} {R.NAME[st]}')
