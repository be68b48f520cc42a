"""Off-nominal inputs for the linear-attention layers - K9 (k9_encoder_fused.hip), K11 (k11_fine_layer.hip), K2 (k2_linear_attention.hip) -
their float64 references, the restatements with the kernels' rounding points (with switchable mutations) and the error budgets
(imported by tests/test_linear_attention_regimes.py and tests/test_linear_attention_regimes_gpu.py, like tests/softmax_regimes.py).

How inputs are steered.  The layers have no bias, so channel 0 of x and of source is the constant 1.0 and column 0 of a weight matrix
is a per-output-channel offset: q = q_off + W_q[:, 1:] x[1:].  Everything else is seeded unit-scale noise (weights N(0, 1 / fan_in)), so
q, k, v are unit normal plus their offsets.  A case is a plain dict (weights P keyed like one encoder layer's state dict, x, src, masks);
nothing is read from disk.

References.  Always the float64 evaluation of the reference arithmetic (O.linear_attention, O.encoder_layer, the Geo finish) on exactly
the kernel's operands: x, source and the weight matrices rounded to the storage type, then cast to float64.
Restatements (O.linear_attention_fused / _window, O.encoder_layer_fused / _chain, O._finish_fused with the kernels' one-pass LayerNorm) are
the yardstick: what THEY lose against float64 is recorded in REST below, and a kernel may lose that plus a stated margin (budget()).

Units.  Messages: |got - ref| / (EPS_T * A) per element, A = sum_s w_s |v_s| the float64-weighted mean of |v| (>= |ref|; A == 0 only where
a mask removes the row or the image has no valid key, and there the output must be an exact zero).  Layer outputs:
|got - ref| / (EPS_T * max(1, |ref|)).  EPS_T is one ulp of the storage type at 1.0."""
import math

import torch
import torch.nn.functional as F

import geoformer_oracle as O

U32 = 2.0 ** -24
EPS = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7, torch.float32: 2.0 ** -23}
NAME = {torch.float16: 'fp16', torch.bfloat16: 'bf16', torch.float32: 'fp32'}
SUB = {torch.float16: 2.0 ** -25, torch.bfloat16: 2.0 ** -134, torch.float32: 0.0}     # half the spacing of each type's subnormal numbers
ATT_EPS, LN_EPS = 1e-6, 1e-5
H16, BF16, F32 = torch.float16, torch.bfloat16, torch.float32

# ---------------------------------------------------------------------------------------------------------------------------
# regimes: (name, variant) -> storage types.  variant = the offset (cold_*), the 1-key image's k offset (few_keys) or the
# mean / std ratio (ln_offset)
# ---------------------------------------------------------------------------------------------------------------------------
COARSE = {('control', None): (H16, BF16), ('hot', None): (H16, BF16),
          ('cold_q', -12): (H16, BF16), ('cold_q', -14): (BF16,),
          ('cold_qv', -13): (H16,),                                          # cold_q with the ramp regime's constant component of v
          ('cold_k', -8): (H16, BF16), ('cold_k', -12): (BF16,),
          ('few_keys', 6): (H16,), ('few_keys', 2): (BF16,), ('few_keys', -8): (BF16,),
          ('wide_v', None): (H16, BF16), ('sparse_v', None): (H16, BF16), ('ramp', None): (H16, BF16),
          ('ln_offset', 8): (H16, BF16), ('ln_offset', 32): (H16, BF16), ('ln_offset', 128): (BF16,)}
FINE = {('control', None): (H16, BF16), ('hot', None): (H16, BF16), ('cold_q', -12): (H16, BF16), ('cold_q', -14): (BF16,),
        ('cold_k', -8): (H16, BF16), ('cold_k', -12): (BF16,), ('ramp', None): (H16, BF16),
        ('ln_offset', 8): (H16, BF16), ('ln_offset', 32): (H16, BF16), ('ln_offset', 128): (BF16,)}
# K11 (the whole fine layer) leaves cold_k -12 out: the chain restatement alone is at 4.1 ulp maximum, 0.53 ulp mean there (-11: 4.4, 0.60;
# -10: 3.9, 0.50; -9: 3.5, 0.46 - no step between -8 and -12 clears the output condition with room); K2's window kernel keeps it
FINE_LAYER = {k: v for k, v in FINE.items() if k != ('cold_k', -12)}
ATTENTION_ONLY = ('control', 'hot', 'cold_q', 'cold_qv', 'cold_k', 'few_keys', 'wide_v', 'sparse_v', 'ramp')     # regimes that say something about K2
FINE_SHAPES = ((37, 25, True), (5, 32, False))                     # (Nw, Lw, cross): every fine regime runs both forms
FINE_SHAPES_CONTROL = ((37, 25, True), (3, 25, False), (5, 32, False), (9, 17, True))
WINDOW_SHAPES = ((7, 25, 25), (6, 32, 17), (3, 9, 32))             # tests/test_ops_gpu.py:test_linear_attention_fine_shape
COARSE_SHAPES_CONTROL = ((300, 1280), (256, 1280), (300, 200))     # ragged third tile; two full tiles; S < L, two source tiles
FEW_KEYS = (1280, 3, 1, 0)
# few_keys: the k offset of the 3-key image, and in fp16 of the 1-key image.  Offsets of -5 (3 keys) and 0 (1 key) leave the fp16
# restatement at 6.4 and 3.6 ulp: KV / S and Ksum / S of so few keys among 1280 are fp16 subnormals (phi(k) / 1280 < 2^-14 once k < -2.7), so
# fp16 runs the 3-key image at -2 (-3: 1.00 ulp, -4: 1.9) and the 1-key image at +6 (one key among 1280: an entry of KV / S is subnormal
# wherever phi(k) |v| < 2^-14 * 1280 = 0.078, and A = |v| there; +1: 1.4 ulp, +3: 2.1, +4: 2.9 on the smallest v; +6: 0.6); bf16 keeps -5
# and runs the 1-key image at +2 and at -8: with ONE key the message is a one-term quotient of two rounded state entries, rounded again, and the
# fused form (K9) lands between 0.85 and 1.03 ulp whatever the offset (0: 1.03, +1: 1.01, +2: 0.85, -8: 0.85)
# sparse_v: every image has SPARSE_KEYS valid keys of 1280 (a small image padded to a large S), k + 12, and v = a constant of +-SPARSE_V per channel
# plus 100 x noise: phi(k) |v| ~ 13 * 7900 lies beyond fp16's range, KV / S = that * 40 / 1280 ~ 3200 well inside it - the scaling by the PADDED length
# is what keeps the state finite (1 / valid in its place overflows).  7900: the message stays in the top of the binade below 8192.
SPARSE_KEYS, SPARSE_V, SPARSE_NOISE = 40, 7900.0, 100.0
FEW_KEYS_OFF3 = {H16: -2.0, BF16: -5.0}
TANH_ROW_SCALES = (1.0, 8.0, 24.0)       # 64 (|pre-activation| to 280) leaves the restatement at 5.1 / 5.6 ulp, 32 at 3.3 / 3.9; 24 reaches +-105


def key(regime, variant=None):
    return regime if variant is None else f'{regime}{variant:+d}'


def rt(x, st):
    return O.rt(x, st)


# ---------------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------------
_MATS = (('q_proj', 1, 1), ('k_proj', 1, 1), ('v_proj', 1, 1), ('merge', 1, 1), ('mlp.0', 2, 2), ('mlp.2', 1, 2))


def layer_weights(c, seed):
    """One encoder layer's state dict (no prefix): matrices N(0, 1 / fan_in) with a ZERO column 0 (the steering column), LayerNorm affine
    terms near identity."""
    g = torch.Generator().manual_seed(seed)
    P = {}
    for nm, o, i in _MATS:
        w = torch.randn(o * c, i * c, generator=g) / math.sqrt(i * c)
        w[:, 0] = 0.
        P[nm + '.weight'] = w
    for nm in ('norm1', 'norm2'):
        P[nm + '.weight'] = 1.0 + 0.05 * (2 * torch.rand(c, generator=g) - 1)
        P[nm + '.bias'] = 0.02 * (2 * torch.rand(c, generator=g) - 1)
    return P


# ramp: per head (q from, q to, k from, k to): the q and k offsets run linearly over the head's channels d between these ends, all within
# [-6, +6], every head with its own slopes and signs.  Found by a random search for the set whose WEAKEST exchange (any two heads' Ksum, or
# the two halves of one head's) moves the normaliser most: a head's own phi(q) . Ksum is small (its q and k ramps run against each other)
# and any other head's Ksum, or its own with the halves exchanged, in its place is several times larger or smaller.
RAMPS = ((-6.0, 6.0, -6.0, 0.25), (5.25, -3.0, 0.25, -6.0), (3.0, -6.0, -6.0, 3.0), (6.0, -2.75, 5.25, -5.5),
         (-4.0, 6.0, -6.0, -3.25), (2.0, -6.0, -0.75, -6.0), (-6.0, -0.5, -6.0, -1.75), (0.0, -6.0, 1.75, -4.0))
# ... and the constant component of v (one sign per channel) that makes the message as large as A: a wrong normaliser then moves it by a
# fraction of A, not of a mean of 1280 zero-mean values.  0.875: the message stays below 1.0, in the binade whose ulp is EPS_T / 2.
RAMP_V = 0.875
RAMP_V_FINE = 0.5         # the fine form (25 keys: the message spreads over more binades): 0.875 leaves the window restatement at 0.17 ulp mean


def ramp_offsets(nhead, d):
    t = torch.linspace(0.0, 1.0, d)
    q = torch.cat([RAMPS[h][0] + (RAMPS[h][1] - RAMPS[h][0]) * t for h in range(nhead)])
    k = torch.cat([RAMPS[h][2] + (RAMPS[h][3] - RAMPS[h][2]) * t for h in range(nhead)])
    return q, k


def ramp_swap_effect(q, k, v, st, halves=True):
    """The promise of the ramp regime on float64 q, k, v [N, *, H, D]: for every pair of heads whose Ksum is exchanged, and (halves) for every
    head whose Ksum has its two halves exchanged, the largest change of the float64 message per query in ulps of st at the scale A - its
    10th percentile over the queries (so 90 % of them move at least that much).  Returns {exchange: ulps}."""
    import itertools
    Q, K = F.elu(q) + 1, F.elu(k) + 1
    ks = K.sum(1)
    num = torch.einsum('nlhd,nhdv->nlhv', Q, torch.einsum('nshd,nshv->nhdv', K, v))
    den = torch.einsum('nlhd,nhd->nlh', Q, ks) + ATT_EPS
    A = torch.einsum('nlhd,nhdv->nlhv', Q, torch.einsum('nshd,nshv->nhdv', K, v.abs())) / den[..., None]
    ref = num / den[..., None]
    H, D = ks.shape[1], ks.shape[2]
    out = {}

    def moved(k2):
        d2 = torch.einsum('nlhd,nhd->nlh', Q, k2) + ATT_EPS
        e = ((num / d2[..., None] - ref).abs() / (EPS[st] * A)).flatten(2).amax(-1).flatten()
        return float(e.kthvalue(max(1, int(0.1 * e.numel())))[0])
    for a, b in itertools.combinations(range(H), 2):
        k2 = ks.clone()
        k2[:, [a, b]] = ks[:, [b, a]]
        out[(a, b)] = moved(k2)
    for a in range(H if halves else 0):
        k2 = ks.clone()
        k2[:, a] = torch.cat([ks[:, a, D // 2:], ks[:, a, :D // 2]], -1)
        out[(a, 'halves')] = moved(k2)
    return out


def _seed(*parts):
    import zlib
    return zlib.crc32(repr(parts).encode()) & 0x7FFFFFFF


def _steer(P, regime, variant, c, nhead):
    if regime == 'hot':
        P['q_proj.weight'][:, 0] = 12.0
        P['k_proj.weight'][:, 0] = 12.0
    elif regime in ('cold_q', 'cold_qv'):
        P['q_proj.weight'][:, 0] = float(variant)
    elif regime == 'cold_k':
        P['k_proj.weight'][:, 0] = float(variant)
    if regime == 'ramp':
        q, k = ramp_offsets(nhead, c // nhead)
        P['q_proj.weight'][:, 0] = q
        P['k_proj.weight'][:, 0] = k
    if regime in ('ramp', 'cold_qv'):
        # cold_qv: with a message of the size of A, a normaliser that does not see the rounding of phi(q) (fp16 subnormals at -13) shows
        g = torch.Generator().manual_seed(5)
        P['v_proj.weight'][:, 0] = torch.where(torch.rand(c, generator=g) < 0.5, -1.0, 1.0) * (RAMP_V if c == 256 else RAMP_V_FINE)


def coarse_case(regime, variant=None, st=H16, L=300, S=1280):
    """One K9 call: dict(P, x [N, L, 256], src [N, S, 256], xm, sm (bool masks or None), nhead, kind).  x, src are already rounded to st."""
    c, nhead = 256, 8
    N = 4 if regime == 'few_keys' else 3
    g = torch.Generator().manual_seed(_seed('coarse', regime, variant, L, S))
    P = layer_weights(c, _seed('w', regime, variant))
    x = torch.randn(N, L, c, generator=g)
    src = torch.randn(N, S, c, generator=g)
    x[..., 0] = 1.0
    src[..., 0] = 1.0
    xm = sm = None
    _steer(P, regime, variant, c, nhead)
    if regime == 'few_keys':
        # the k offset is per IMAGE here: k_proj's column 0 is 1 and the source's constant channel carries the offset
        P['k_proj.weight'][:, 0] = 1.0
        for b, off in enumerate((0.0, FEW_KEYS_OFF3[st], float(variant), 0.0)):
            src[b, :, 0] = off
        sm = torch.zeros(N, S, dtype=torch.bool)
        sm[0] = True
        sm[1, :3] = True                                         # a prefix
        sm[2, 777] = True                                        # scattered: one key in the seventh source tile
        xm = torch.ones(N, L, dtype=torch.bool)
        xm[0, 100:131] = False
        xm[3, L - 7:] = False
    elif regime == 'wide_v':
        P['k_proj.weight'][:, 0] = 12.0
        sm = torch.ones(N, S, dtype=torch.bool)
        sm[1, S // 2:] = False                                   # a prefix
        sm[2, 1::3] = False                                      # scattered
    elif regime == 'sparse_v':
        P['k_proj.weight'][:, 0] = 12.0
        P['v_proj.weight'] *= SPARSE_NOISE
        gs = torch.Generator().manual_seed(6)
        P['v_proj.weight'][:, 0] = torch.where(torch.rand(c, generator=gs) < 0.5, -SPARSE_V, SPARSE_V)
        sm = torch.zeros(N, S, dtype=torch.bool)
        sm[0, :SPARSE_KEYS] = True                                # a prefix
        sm[1, ::S // SPARSE_KEYS] = True                          # scattered: four keys in every source tile
        sm[2, 7::S // SPARSE_KEYS] = True
    x, src = rt(x, st), rt(src, st)
    case = dict(P=P, x=x, src=src, xm=xm, sm=sm, nhead=nhead, kind='loftr', regime=regime, variant=variant, st=st)
    if regime == 'wide_v':
        kvs = _kv_over_s(case).abs().max()
        P['v_proj.weight'] *= float(2.0 ** 13.5 / kvs)           # max |KV / S| = 11585 before the weights are rounded
    elif regime == 'ln_offset':
        _drive_layernorms(case, float(variant))
    return case


def fine_case(regime, variant=None, st=H16, Nw=37, Lw=25, cross=True):
    """One K11 call: windows x [Nw, Lw, 128], src (another tensor when cross, else x itself), no masks."""
    c, nhead = 128, 8
    g = torch.Generator().manual_seed(_seed('fine', regime, variant, Nw, Lw, cross))
    P = layer_weights(c, _seed('wf', regime, variant))
    x = torch.randn(Nw, Lw, c, generator=g)
    x[..., 0] = 1.0
    src = x
    if cross:
        src = torch.randn(Nw, Lw, c, generator=g)
        src[..., 0] = 1.0
    _steer(P, regime, variant, c, nhead)
    x = rt(x, st)
    src = rt(src, st) if cross else x
    case = dict(P=P, x=x, src=src, xm=None, sm=None, nhead=nhead, kind='loftr', regime=regime, variant=variant, st=st, cross=cross)
    if regime == 'ln_offset':
        _drive_layernorms(case, float(variant))
    return case


def tanh_case(st=H16, L=300):
    """The Geo finish form (layer.finish: attention output given, tanh MLP, per-sample skip flags): mlp.0's rows scaled by TANH_ROW_SCALES."""
    c = 256
    g = torch.Generator().manual_seed(_seed('tanh', L))
    P = layer_weights(c, _seed('wt'))
    P['mlp.0.weight'][:171] *= TANH_ROW_SCALES[0]
    P['mlp.0.weight'][171:342] *= TANH_ROW_SCALES[1]
    P['mlp.0.weight'][342:] *= TANH_ROW_SCALES[2]
    x = torch.randn(3, L, c, generator=g)
    x[..., 0] = 1.0
    msg = torch.randn(3, L, c, generator=g)
    return dict(P=P, x=rt(x, st), msg=rt(msg, st), flag=torch.tensor([1, 0, 5], dtype=torch.int32), kind='geo', st=st, regime='tanh_sat')


# ---------------------------------------------------------------------------------------------------------------------------
# float64 references
# ---------------------------------------------------------------------------------------------------------------------------
def weights64(case):
    """The kernel's operands in float64: matrices rounded to the storage type, LayerNorm terms as they are (fp32 in the kernels)."""
    st = case['st']
    return {k: (rt(v, st) if v.dim() == 2 else v).double() for k, v in case['P'].items()}


def projections64(case):
    P = weights64(case)
    n, _, c = case['x'].shape
    h = case['nhead']
    q = F.linear(case['x'].double(), P['q_proj.weight']).view(n, -1, h, c // h)
    k = F.linear(case['src'].double(), P['k_proj.weight']).view(n, -1, h, c // h)
    v = F.linear(case['src'].double(), P['v_proj.weight']).view(n, -1, h, c // h)
    return q, k, v


def _kv_over_s(case):
    _, k, v = projections64(case)
    K = F.elu(k) + 1
    if case['sm'] is not None:
        K = K * case['sm'][:, :, None, None]
    return torch.einsum('nshd,nshv->nhdv', K, v) / v.size(1)


def attention64(q, k, v, qm=None, km=None):
    """(message, A) in float64 from float64 q, k, v [N, *, H, D]: A = the same attention of |v|."""
    return O.linear_attention(q, k, v, qm, km, ATT_EPS), O.linear_attention(q, k, v.abs(), qm, km, ATT_EPS)


def layer64(case):
    return O.encoder_layer(weights64(case), '', case['x'].double(), case['src'].double(), case['nhead'], 'loftr', case['xm'], case['sm'])


def finish64(case):
    """The Geo layer behind its attention (geo_transformer/transformer.py:57-66) in float64; a skipped sample keeps x."""
    P, x, c = weights64(case), case['x'].double(), case['x'].shape[-1]
    m = F.layer_norm(F.linear(case['msg'].double(), P['merge.weight']), (c,), P['norm1.weight'], P['norm1.bias'])
    pre = F.linear(torch.cat([x, m], 2), P['mlp.0.weight'])
    o = F.layer_norm(F.linear(torch.tanh(pre), P['mlp.2.weight']), (c,), P['norm2.weight'], P['norm2.bias'])
    out = x + o
    out[case['flag'] == 0] = x[case['flag'] == 0]
    return out, pre


def ln_inputs64(case):
    """The rows that enter LayerNorm 1 and LayerNorm 2 of the float64 forward (rows of masked queries included)."""
    P, x = weights64(case), case['x'].double()
    n, _, c = x.shape
    q, k, v = projections64(case)
    msg = O.linear_attention(q, k, v, case['xm'], case['sm'], ATT_EPS).reshape(n, -1, c)
    m1 = F.linear(msg, P['merge.weight'])
    m = F.layer_norm(m1, (c,), P['norm1.weight'], P['norm1.bias'])
    m2 = F.linear(torch.relu(F.linear(torch.cat([x, m], 2), P['mlp.0.weight'])), P['mlp.2.weight'])
    return m1, m2


def mean_over_std(rows):
    return rows.mean(-1).abs() / rows.std(-1, unbiased=False).clamp_min(1e-300)


def _drive_layernorms(case, ratio):
    """LayerNorm inputs with |mean| / std = ratio per row.  LN1: v's channel 0 is the constant 1 (v_proj row 0 selects the constant channel
    of the source), so the message's channel 0 is 1 and merge's column 0 is a per-channel offset of LN1's input.  LN2: hidden unit 0 is
    relu(1) = 1 (mlp.0 row 0 selects the constant channel of x) and mlp.2's column 0 is the offset.  The offsets are `ratio` times the
    rows' own standard deviation, measured on the float64 forward."""
    P = case['P']
    P['v_proj.weight'][0] = 0.
    P['v_proj.weight'][0, 0] = 1.0
    P['mlp.0.weight'][0] = 0.
    P['mlp.0.weight'][0, 0] = 1.0
    m1, _ = ln_inputs64(case)
    P['merge.weight'][:, 0] = ratio * float(m1.std(-1, unbiased=False).median())
    _, m2 = ln_inputs64(case)                                    # LN1's output does not depend on a constant offset of its input
    P['mlp.2.weight'][:, 0] = ratio * float(m2.std(-1, unbiased=False).median())


# ---------------------------------------------------------------------------------------------------------------------------
# restatements with the kernels' rounding points, and their mutations
# ---------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ('den_unrounded', 'eps_unscaled', 'inv_valid', 'mask_k_only', 'mask_v_only', 'swap_heads', 'swap_halves', 'phi_no_plus1',
             'ln_no_eps', 'ln_two_pass')


def _phi_no_plus1(x):
    return torch.where(x > 0, x, torch.exp(torch.clamp(x, max=0)))


def attention_restated(q, k, v, st, qm=None, km=None, form='fused', mut=None, swap=(0, 1), eps=ATT_EPS):
    """O.linear_attention_fused (form 'fused': q, k, v the un-rounded fp32 projections, Ksum adds the un-rounded phi(k), the mask lies on
    phi(k) alone - K9) or O.linear_attention_window (form 'window': q, k, v as stored, Ksum adds the ROUNDED phi(k), the mask on phi(k) and v -
    K2's 16-bit kernels and K11), bit for bit when mut is None (tests/test_linear_attention_regimes.py checks that), else with one
    deliberate mistake:
      den_unrounded  the normaliser from phi(q) before it is rounded          eps_unscaled  eps in place of eps / S
      inv_valid      1 / (number of valid keys) in place of 1 / S             phi_no_plus1  phi(x) = x for x > 0
      mask_k_only    the mask on phi(k) but not on v (window form; the fused form IS that)      mask_v_only  on v but not on phi(k)
      swap_heads     Ksum of the heads `swap` exchanged                       swap_halves   Ksum of head swap[0]: its two halves exchanged"""
    phi = _phi_no_plus1 if mut == 'phi_no_plus1' else O._phi
    s_len = v.size(1)
    one = torch.tensor(1.0, dtype=torch.float32)
    inv_s = one / float(s_len)
    eps_s = torch.tensor(eps, dtype=torch.float32) / float(s_len) if form == 'fused' else torch.tensor(eps, dtype=torch.float32) * inv_s
    inv_kv = inv_ks = inv_s
    if mut == 'inv_valid' and km is not None:
        per = one / km.sum(1).clamp_min(1).float()
        inv_kv, inv_ks, eps_s = per[:, None, None, None], per[:, None, None], (eps * per)[:, None, None]
    if mut == 'eps_unscaled':
        eps_s = torch.tensor(eps, dtype=torch.float32)
    Qf, Kf = phi(q), phi(k)
    if km is not None and mut != 'mask_v_only':
        Kf = Kf * km[:, :, None, None]
    if km is not None and (mut == 'mask_v_only' or (form == 'window' and mut != 'mask_k_only')):
        v = v * km[:, :, None, None]
    Q, K, V = rt(Qf, st), rt(Kf, st), rt(v, st)
    if qm is not None:
        Q, Qf = Q * qm[:, :, None, None], Qf * qm[:, :, None, None]
    KV = rt(torch.einsum('nshd,nshv->nhdv', K, V) * inv_kv, st)
    ks = (Kf if form == 'fused' else K).sum(dim=1)
    if mut == 'swap_heads':
        ks = ks.clone()
        ks[:, list(swap)] = ks[:, list(swap[::-1])]
    elif mut == 'swap_halves':
        ks = ks.clone()
        half = ks.shape[-1] // 2
        ks[:, swap[0]] = torch.cat([ks[:, swap[0], half:], ks[:, swap[0], :half]], -1)
    Ks = rt(ks * inv_ks, st)
    num = torch.einsum('nlhd,nhdv->nlhv', Q, KV)
    den = torch.einsum('nlhd,nhd->nlh', Qf if mut == 'den_unrounded' else Q, Ks) + eps_s
    return rt(num * (1.0 / den)[..., None], st) if form == 'fused' else rt(num / den[..., None], st)


def layer_norm_restated(x, weight, bias, mut=None, eps=LN_EPS):
    """The kernels' one-pass LayerNorm (O.layer_norm_one_pass); ln_two_pass: F.layer_norm's centred statistics; ln_no_eps: eps dropped."""
    if mut == 'ln_two_pass':
        return F.layer_norm(x, x.shape[-1:], weight, bias, eps)
    return O.layer_norm_one_pass(x, weight, bias, 0.0 if mut == 'ln_no_eps' else eps)


def finish_restated(P, x, msg, kind, st, mut=None, chain=False):
    """O._finish_fused(one_pass=True), or with chain=True the tail of O.encoder_layer_chain(one_pass=True) (LN2's output rounded before the
    residual sum)."""
    W = lambda name: rt(P[name], st)                                             # noqa: E731
    m = rt(layer_norm_restated(F.linear(msg, W('merge.weight')), P['norm1.weight'], P['norm1.bias'], mut), st)
    hid = F.linear(torch.cat([x, m], dim=2), W('mlp.0.weight'))
    hid = rt(torch.relu(hid) if kind == 'loftr' else torch.tanh(hid), st)
    o = layer_norm_restated(F.linear(hid, W('mlp.2.weight')), P['norm2.weight'], P['norm2.bias'], mut)
    return rt(x + rt(o, st), st) if chain else rt(x + o, st)


def message_restated(case, mut=None, swap=(0, 1), chain=False):
    """The message [N, L, C] the K9 layer (chain=False: O.linear_attention_fused on the un-rounded fp32 projections) or the K11 layer
    (chain=True: O.linear_attention_window on the rounded ones) forms inside; not observable on the device."""
    P, x, src, st, h = case['P'], case['x'], case['src'], case['st'], case['nhead']
    n, _, c = x.shape
    W = lambda name: rt(P[name], st)                                             # noqa: E731
    r = (lambda t: rt(t, st)) if chain else (lambda t: t)
    q = r(F.linear(x, W('q_proj.weight'))).view(n, -1, h, c // h)
    k = r(F.linear(src, W('k_proj.weight'))).view(n, -1, h, c // h)
    v = r(F.linear(src, W('v_proj.weight'))).view(n, -1, h, c // h)
    return attention_restated(q, k, v, st, case['xm'], case['sm'], 'window' if chain else 'fused', mut, swap).reshape(n, -1, c)


def layer_restated(case, mut=None, swap=(0, 1), chain=False):
    """The K9 layer (chain=False: O.encoder_layer_fused) or the K11 layer (chain=True: O.encoder_layer_chain) with one-pass LayerNorms."""
    return finish_restated(case['P'], case['x'], message_restated(case, mut, swap, chain), 'loftr', case['st'], mut, chain)


def k2_operands(case, st):
    """q, k, v [N, *, C] of a case as K2 receives them: the projections of the case's float64 forward, stored in st (the same offsets, on q, k
    and v directly)."""
    n, _, c = case['x'].shape
    return tuple(t.reshape(n, -1, c).float().to(st) for t in projections64(case))


def window_operands(regime, variant, st, N, L, S):
    """q [N, L, 128], k, v [N, S, 128] in st for K2's window kernel (8 heads of 16): unit normal plus the regime's offsets, no masks."""
    g = torch.Generator().manual_seed(_seed('window', regime, variant, N, L, S))
    P = {nm + '.weight': torch.zeros(128, 1) for nm in ('q_proj', 'k_proj', 'v_proj')}
    _steer(P, regime, variant, 128, 8)
    q = torch.randn(N, L, 128, generator=g) + P['q_proj.weight'][:, 0]
    k = torch.randn(N, S, 128, generator=g) + P['k_proj.weight'][:, 0]
    v = torch.randn(N, S, 128, generator=g) + P['v_proj.weight'][:, 0]
    return q.to(st), k.to(st), v.to(st)


def k2_restated(q, k, v, st, nhead, qm=None, km=None, mut=None, swap=(0, 1)):
    """K2 on stored q, k, v [N, *, C]: the 16-bit kernels round like the window form at any sequence length (la16_kv adds the ROUNDED phi(k)
    into Ksum with the matrix cores); the fp32 parity kernels are the reference formula in fp32."""
    n, _, c = q.shape
    sp = lambda t: t.float().view(n, -1, nhead, c // nhead)                      # noqa: E731
    if st == F32:
        return O.linear_attention(sp(q), sp(k), sp(v), qm, km, ATT_EPS).reshape(n, -1, c)
    return attention_restated(sp(q), sp(k), sp(v), st, qm, km, 'window', mut, swap).reshape(n, -1, c)


def k2_reference(q, k, v, nhead, qm=None, km=None):
    n, _, c = q.shape
    sp = lambda t: t.double().view(n, -1, nhead, c // nhead)                     # noqa: E731
    ref, A = attention64(sp(q), sp(k), sp(v), qm, km)
    return ref.reshape(n, -1, c), A.reshape(n, -1, c)


# ---------------------------------------------------------------------------------------------------------------------------
# state (gf_encoder_kv_state and the state tail of gf_encoder_layer_kv): a derived per-entry bound
# ---------------------------------------------------------------------------------------------------------------------------
def state_reference(case, src=None, mask=None):
    """float64 (KV [N, C * D], Ksum [N, C]) of the source rows in the kernels' layout and the per-entry error bounds (bKV, bKs):
      * k is an fp32 sum of C products: |dk| <= (C + 2) u32 sum_c |W_kc x_c|, which moves phi(k) by phi'(k) |dk| (phi' = phi for k <= 0, 1
        above) plus the hardware exponential's 2 u32 phi(k);
      * Ksum adds S of them in fp32: (S + 8) u32 Ksum - a RELATIVE bound per entry, Ksum is a sum of positive terms;
      * KV multiplies round_T(phi(k)) by round_T(v) (EPS_T / 2 each, v itself an fp32 sum: (C + 2) u32 sum_c |W_vc x_c|) and adds S
        products in fp32: against sum_s |phi(k_s) v_s|, not the largest entry; below the storage type's normal range the rounding error
        of phi(k) or v is absolute, half the subnormal spacing SUB_T (fp16: 2^-25) times the other factor.
    What the Ksum bound does NOT resolve: it is a worst-case bound, dominated by (C + 2) u32 sum_c |W_kc x_c| (about 3e-4 relative; the kernels
    sit at 0.02 of it or less), so where many keys are valid a Ksum that added the ROUNDED phi(k) instead of the un-rounded one (a documented
    choice of K9: EPS_T / 2 per term, about EPS_T / sqrt(S) on the sum) would pass.  Only the one-key image of few_keys pins that choice
    (there Ksum IS one phi(k)); a mix-up of heads or channels, or a lost tile, is of order 1 and fails everywhere."""
    st, P, h = case['st'], weights64(case), case['nhead']
    src = case['src'] if src is None else src
    mask = case['sm'] if src is case['src'] and mask is None else mask
    n, S, c = src.shape
    d = c // h
    x = src.double()
    k, v = F.linear(x, P['k_proj.weight']), F.linear(x, P['v_proj.weight'])
    dk = (c + 2) * U32 * F.linear(x.abs(), P['k_proj.weight'].abs())
    dv = (c + 2) * U32 * F.linear(x.abs(), P['v_proj.weight'].abs())
    K = F.elu(k) + 1
    dK = torch.where(k > 0, torch.ones_like(K), K) * dk * math.e ** 1e-3 + 2 * U32 * K
    if mask is not None:
        K, dK = K * mask[:, :, None], dK * mask[:, :, None]
    K4, dK4, v4, dv4 = (t.view(n, S, h, d) for t in (K, dK, v, dv))
    KV = torch.einsum('nshd,nshv->nhdv', K4, v4)
    absKV = torch.einsum('nshd,nshv->nhdv', K4, v4.abs())
    bKV = (1.01 * EPS[st] + (S + 8) * U32) * absKV + torch.einsum('nshd,nshv->nhdv', dK4, v4.abs()) * 1.01 \
        + torch.einsum('nshd,nshv->nhdv', K4, dv4) * 1.01 \
        + SUB[st] * 1.01 * (torch.einsum('nshd,nshv->nhdv', (K4 > 0).double(), v4.abs()) + torch.einsum('nshd,nshv->nhdv', K4, torch.ones_like(v4)))
    Ks = K4.sum(1)
    bKs = (S + 8) * U32 * Ks + dK4.sum(1) * (1 + 1e-5)
    return KV.reshape(n, c * d), Ks.reshape(n, c), bKV.reshape(n, c * d), bKs.reshape(n, c)


def state_check(state, case, src=None, mask=None):
    """max over entries of |state - ref| / bound for KV and for Ksum (<= 1 passes); an entry whose bound is 0 must be an exact 0."""
    KV, Ks, bKV, bKs = state_reference(case, src, mask)
    c = Ks.shape[1]
    state = state.double().cpu()
    assert bool(torch.isfinite(state).all())
    out = []
    for got, ref, b in ((state[:, :-c], KV, bKV), (state[:, -c:], Ks, bKs)):
        e = (got - ref).abs()
        assert bool((e[b == 0] == 0).all())
        out.append(float((e / b.clamp_min(1e-300))[b > 0].max()) if bool((b > 0).any()) else 0.0)
    return tuple(out)


def state_restated(case):
    KV, Ks = O.encoder_kv_state_fused(case['P'], '', case['src'], case['nhead'], case['st'], case['sm'])
    n = KV.shape[0]
    return torch.cat([KV.reshape(n, -1), Ks.reshape(n, -1)], 1)


# ---------------------------------------------------------------------------------------------------------------------------
# errors and budgets
# ---------------------------------------------------------------------------------------------------------------------------
def message_error(got, ref, A, st):
    """(max, mean) of |got - ref| / (EPS_T A) over EVERY element; where A == 0 (masked query, image without keys) the output must be an
    exact zero, and counts as zero error.  Anything non-finite: (inf, inf)."""
    got = got.double().cpu()
    if not bool(torch.isfinite(got).all()):
        return math.inf, math.inf
    live = A > 0
    if not bool((got[~live] == 0).all()):
        return math.inf, math.inf
    e = torch.where(live, (got - ref).abs() / (EPS[st] * A.clamp_min(1e-300)), torch.zeros_like(ref))
    return float(e.max()), float(e.mean())


def output_error(got, ref, st):
    """(max, mean) of |got - ref| / (EPS_T max(1, |ref|)) over every element."""
    got = got.double().cpu()
    if not bool(torch.isfinite(got).all()):
        return math.inf, math.inf
    e = (got - ref).abs() / (EPS[st] * ref.abs().clamp_min(1.0))
    return float(e.max()), float(e.mean())


# The condition under which a regime is kept for a type: what the RESTATEMENT alone loses against float64
KEEP = {'message': (1.0, 0.15), 'output': (4.0, 0.5)}


def budget(rest):
    """(max, mean) a kernel may lose, from the restatement's recorded (max, mean): what separates the two is fp32 sums in another order, which
    flip values that sit on a rounding boundary (2 ulp for one layer, tests/test_encoder_fused.py:_ulp_close), and v_rcp_f32 / v_exp_f32
    (1 ulp of fp32 each): max + 2 ulp, 1.5 x mean + 0.05 ulp.  The same rule in ulps of fp32 for K2's fp32 kernels (nothing is rounded to a
    storage type there: the restatement is the reference formula in fp32, the kernel the same sums in another order, expm1f and a division)."""
    return rest[0] + 2.0, 1.5 * rest[1] + 0.05


# What the restatements lose against float64: 'entry/regime/type' -> (max, mean), measured by tests/test_linear_attention_regimes.py
# (test_restatement_table checks every line: the measured value may not exceed it, and it may not exceed KEEP) and rounded up.
#   k2      ops.linear_attention, coarse shape (N = 3 or 4, L = 300, S = 1280, 8 heads of 32): messages
#   k2w     ops.linear_attention, window kernel (8 heads of 16, <= 32 tokens): messages, worst of WINDOW_SHAPES
#   k9msg   the message inside the K9 layer, O.linear_attention_fused (not observable on the device: checked on the CPU only, to show that
#           the regime meets the message condition in the form K9 actually computes)
#   k9      LoFTREncoderLayer.forward, fused form: layer outputs           k9tanh  layer.finish, Geo form
#   k11     the fine layer, worst of its shapes and of self / cross
REST = {
    'k9/control/fp16': (1.95, 0.285), 'k2/control/fp16': (0.10, 0.008), 'k9msg/control/fp16': (0.20, 0.024),
    'k9/control/bf16': (2.10, 0.286), 'k2/control/bf16': (0.10, 0.008), 'k9msg/control/bf16': (0.20, 0.024),
    'k9/hot/fp16': (1.85, 0.283), 'k2/hot/fp16': (0.10, 0.006), 'k9msg/hot/fp16': (0.10, 0.009),
    'k9/hot/bf16': (2.00, 0.282), 'k2/hot/bf16': (0.10, 0.006), 'k9msg/hot/bf16': (0.10, 0.009),
    'k9/cold_q-12/fp16': (2.35, 0.357), 'k2/cold_q-12/fp16': (0.15, 0.018), 'k9msg/cold_q-12/fp16': (0.15, 0.019),
    'k9/cold_q-12/bf16': (1.75, 0.276), 'k2/cold_q-12/bf16': (0.10, 0.008), 'k9msg/cold_q-12/bf16': (0.15, 0.011),
    'k9/cold_q-14/bf16': (1.75, 0.286), 'k2/cold_q-14/bf16': (0.10, 0.008), 'k9msg/cold_q-14/bf16': (0.15, 0.010),
    'k9/cold_qv-13/fp16': (1.65, 0.259), 'k2/cold_qv-13/fp16': (0.70, 0.137), 'k9msg/cold_qv-13/fp16': (0.70, 0.137),
    'k9/cold_k-8/fp16': (2.10, 0.303), 'k2/cold_k-8/fp16': (0.10, 0.012), 'k9msg/cold_k-8/fp16': (0.10, 0.013),
    'k9/cold_k-8/bf16': (1.95, 0.287), 'k2/cold_k-8/bf16': (0.10, 0.009), 'k9msg/cold_k-8/bf16': (0.10, 0.012),
    'k9/cold_k-12/bf16': (1.80, 0.279), 'k2/cold_k-12/bf16': (0.10, 0.009), 'k9msg/cold_k-12/bf16': (0.15, 0.011),
    'k9/few_keys+6/fp16': (1.80, 0.258), 'k2/few_keys+6/fp16': (0.85, 0.036), 'k9msg/few_keys+6/fp16': (0.95, 0.095),
    'k9/few_keys+2/bf16': (1.95, 0.255), 'k2/few_keys+2/bf16': (0.75, 0.035), 'k9msg/few_keys+2/bf16': (1.00, 0.095),
    'k9/few_keys-8/bf16': (1.70, 0.259), 'k2/few_keys-8/bf16': (0.75, 0.037), 'k9msg/few_keys-8/bf16': (0.90, 0.096),
    'k9/wide_v/fp16': (1.70, 0.280), 'k2/wide_v/fp16': (0.10, 0.007), 'k9msg/wide_v/fp16': (0.10, 0.011),
    'k9/wide_v/bf16': (1.85, 0.278), 'k2/wide_v/bf16': (0.10, 0.007), 'k9msg/wide_v/bf16': (0.15, 0.011),
    'k9/sparse_v/fp16': (1.40, 0.241), 'k2/sparse_v/fp16': (0.50, 0.142), 'k9msg/sparse_v/fp16': (0.50, 0.142),
    'k9/sparse_v/bf16': (1.50, 0.243), 'k2/sparse_v/bf16': (0.55, 0.137), 'k9msg/sparse_v/bf16': (0.55, 0.137),
    'k9/ramp/fp16': (1.65, 0.254), 'k2/ramp/fp16': (0.70, 0.140), 'k9msg/ramp/fp16': (0.70, 0.141),
    'k9/ramp/bf16': (1.60, 0.253), 'k2/ramp/bf16': (0.65, 0.143), 'k9msg/ramp/bf16': (0.70, 0.145),
    'k9/ln_offset+8/fp16': (2.05, 0.287), 'k9/ln_offset+8/bf16': (2.00, 0.289), 'k9/ln_offset+32/fp16': (1.80, 0.289),
    'k9/ln_offset+32/bf16': (1.85, 0.285), 'k9/ln_offset+128/bf16': (2.35, 0.304), 'k2/control/fp32': (0.50, 0.039),
    'k2/hot/fp32': (0.40, 0.031), 'k11/control/fp16': (2.25, 0.329), 'k2w/control/fp16': (0.55, 0.059),
    'k11/control/bf16': (2.15, 0.330), 'k2w/control/bf16': (0.50, 0.060), 'k11/hot/fp16': (2.15, 0.317),
    'k2w/hot/fp16': (0.45, 0.048), 'k11/hot/bf16': (1.90, 0.307), 'k2w/hot/bf16': (0.55, 0.047),
    'k11/cold_q-12/fp16': (3.80, 0.456), 'k2w/cold_q-12/fp16': (0.90, 0.104), 'k11/cold_q-12/bf16': (3.05, 0.410),
    'k2w/cold_q-12/bf16': (0.60, 0.065), 'k11/cold_q-14/bf16': (2.65, 0.405), 'k2w/cold_q-14/bf16': (0.60, 0.065),
    'k11/cold_k-8/fp16': (2.75, 0.410), 'k2w/cold_k-8/fp16': (0.55, 0.068), 'k11/cold_k-8/bf16': (2.85, 0.404),
    'k2w/cold_k-8/bf16': (0.65, 0.067), 'k2w/cold_k-12/bf16': (0.60, 0.065), 'k11/ramp/fp16': (2.15, 0.314),
    'k2w/ramp/fp16': (0.90, 0.134), 'k11/ramp/bf16': (2.10, 0.314), 'k2w/ramp/bf16': (0.90, 0.134),
    'k11/ln_offset+8/fp16': (2.05, 0.317), 'k11/ln_offset+8/bf16': (2.30, 0.314), 'k11/ln_offset+32/fp16': (2.05, 0.326),
    'k11/ln_offset+32/bf16': (2.10, 0.321), 'k11/ln_offset+128/bf16': (2.35, 0.329), 'k9tanh/tanh_sat/fp16': (2.75, 0.220),
    'k9tanh/tanh_sat/bf16': (3.40, 0.219),
}


def rest(entry, regime, variant, st):
    return REST[f'{entry}/{key(regime, variant)}/{NAME[st]}']


# ---------------------------------------------------------------------------------------------------------------------------
# one call per (entry, regime, type): the restatement's (or a mutant's) error against float64, the worst of the entry's shapes
# ---------------------------------------------------------------------------------------------------------------------------
SWAP = (1, 5)            # swap_heads exchanges these two (the weakest pair of ramp_swap_effect in the fine form); swap_halves acts on head 2
SWAP_HALVES = (2, 2)     # (the weakest of the coarse form)
_CACHE = {}


def _cached(tag, make):
    if tag not in _CACHE:
        _CACHE[tag] = make()
    return _CACHE[tag]


def coarse_shapes(regime):
    return COARSE_SHAPES_CONTROL if regime == 'control' else ((300, 1280),)


def fine_shapes(regime):
    return FINE_SHAPES_CONTROL if regime == 'control' else FINE_SHAPES


def cached_coarse(regime, variant, st, L=300, S=1280):
    """(case, float64 layer output) - built once per process and shared by the tests (read only)."""
    def make():
        case = coarse_case(regime, variant, st, L, S)
        return case, layer64(case)
    return _cached(('coarse', regime, variant, st, L, S), make)


def cached_fine(regime, variant, st, Nw, Lw, cross):
    def make():
        case = fine_case(regime, variant, st, Nw, Lw, cross)
        return case, layer64(case)
    return _cached(('fine', regime, variant, st, Nw, Lw, cross), make)


def cached_k2(regime, variant, st):
    """(q, k, v in st, xm, sm, ref, A) at the coarse shape.  fp32 takes the fp16 case's float64 projections (unit normal plus offsets)."""
    def make():
        case, _ = cached_coarse(regime, variant, H16 if st == F32 else st)
        q, k, v = k2_operands(case, st)
        return (q, k, v, case['xm'], case['sm']) + k2_reference(q, k, v, 8, case['xm'], case['sm'])
    return _cached(('k2', regime, variant, st), make)


def cached_window(regime, variant, st, N, L, S):
    def make():
        q, k, v = window_operands(regime, variant, st, N, L, S)
        return (q, k, v) + k2_reference(q, k, v, 8)
    return _cached(('k2w', regime, variant, st, N, L, S), make)


def cached_tanh(st):
    def make():
        case = tanh_case(st)
        return (case,) + finish64(case)
    return _cached(('tanh', st), make)


def _worst(errs):
    errs = list(errs)
    return max(e[0] for e in errs), max(e[1] for e in errs)


def restatement_error(entry, regime, variant, st, mut=None):
    """(max, mean) error in ulps of the entry's restatement - or of its mutant - against float64, the worst of the entry's shapes."""
    swap = SWAP_HALVES if mut == 'swap_halves' else SWAP
    if entry == 'k2':
        q, k, v, xm, sm, ref, A = cached_k2(regime, variant, st)
        return message_error(k2_restated(q, k, v, st, 8, xm, sm, mut, swap), ref, A, st)
    if entry == 'k2w':
        def one(shape):
            q, k, v, ref, A = cached_window(regime, variant, st, *shape)
            return message_error(k2_restated(q, k, v, st, 8, None, None, mut, swap), ref, A, st)
        return _worst(one(s) for s in WINDOW_SHAPES)
    if entry == 'k9':
        def one(shape):
            case, ref = cached_coarse(regime, variant, st, *shape)
            return output_error(layer_restated(case, mut, swap), ref, st)
        return _worst(one(s) for s in coarse_shapes(regime))
    if entry == 'k9msg':
        def one(shape):
            case, _ = cached_coarse(regime, variant, st, *shape)
            n, _, c = case['x'].shape
            ref, A = _cached(('k9msg', regime, variant, st) + shape, lambda: attention64(*projections64(case), case['xm'], case['sm']))
            return message_error(message_restated(case, mut, swap), ref.reshape(n, -1, c), A.reshape(n, -1, c), st)
        return _worst(one(s) for s in coarse_shapes(regime))
    if entry == 'k11':
        def one(shape):
            case, ref = cached_fine(regime, variant, st, *shape)
            return output_error(layer_restated(case, mut, swap, chain=True), ref, st)
        return _worst(one(s) for s in fine_shapes(regime))
    if entry == 'k9tanh':
        case, ref, _ = cached_tanh(st)
        got = finish_restated(case['P'], case['x'], case['msg'], 'geo', st, mut)
        got[case['flag'] == 0] = case['x'][case['flag'] == 0]
        return output_error(got, ref, st)
    raise KeyError(entry)


def entries():
    """Every (entry, regime, variant, type) of the table."""
    out = []
    for (regime, variant), types in COARSE.items():
        for st in types:
            out.append(('k9', regime, variant, st))
            if regime in ATTENTION_ONLY:
                out.append(('k2', regime, variant, st))
                out.append(('k9msg', regime, variant, st))
    out += [('k2', regime, None, F32) for regime in ('control', 'hot')]
    for (regime, variant), types in FINE.items():
        for st in types:
            if (regime, variant) in FINE_LAYER:
                out.append(('k11', regime, variant, st))
            if regime != 'ln_offset':
                out.append(('k2w', regime, variant, st))
    out += [('k9tanh', 'tanh_sat', None, st) for st in (H16, BF16)]
    return out


def kind_of(entry):
    return 'message' if entry in ('k2', 'k2w', 'k9msg') else 'output'
