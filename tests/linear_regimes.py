"""Off-nominal inputs, shapes and forms for the K3 linear kernels (csrc/k3_linear.hip: ops.linear, ops.linear_rows, ops.conv1x1,
ops.conv1x1_upsample_add), their float64 references, a restatement with the kernels' rounding points (with switchable mutations), the
per-element error measure and the recorded table (imported by tests/test_linear_regimes.py and tests/test_linear_regimes_gpu.py; rt, EPS,
SPACING, NAME, budget() and term_error are those of tests/linear_attention_regimes.py and tests/backward_regimes.py).

A LINE is form / regime / storage type.  A form is one way into the kernels - an entry point, an epilogue, a list of launch shapes - a
regime says how the operands are steered.  A line's figure is the worst over the form's shapes and over the row counts M_ALL (the first
M rows of one 300-row case: 1 row, the 32 / 64 / 128 row edges of the wave and workgroup tiles of both kernels, 300 = a ragged third tile).

Forms, and the kernel instance each reaches (T = the storage type; w2 = linear_kernel_w2; NB = 32-channel blocks per wave):
  plain        ops.linear, bias, N = 32, 96, 128, 160, 224 (K = 64, 128, 512)     linear_kernel<T, 4, NONE>, ragged column tiles (all types)
  plain_wide   ops.linear, bias, N = 256, 512, 768                                 fp32: linear_kernel<float, 8, NONE>; 16-bit: w2<T, NONE>
  relu2        two-part operand (64|192, 192|64, 256|256; fp32 also 32|96), ReLU,   fp32: <float, 8, RELU>; 16-bit: w2<T, RELU>
               N = 256, 512, 768
  relu2_nb4    two-part operand, ReLU, N = 128, 96 (fp32 also 32|64 at N = 160)     linear_kernel<T, 4, RELU>
  tanh2        two-part operand, Tanh, N = 256, 512, 768                           fp32: <float, 8, TANH> (tanhf); 16-bit: w2<T, TANH>
  tanh_nb4     Tanh, N = 128, 160                                                  linear_kernel<T, 4, TANH>
  ln           LayerNorm, N = 128 and N = 256                                      linear_kernel<T, 4, LN> and <T, 8, LN>
  ln_res       LayerNorm + residual + flag (flag_rows 1, 7, 50, > M, no flag),      linear_kernel<T, 4, LN_RES> and <T, 8, LN_RES>
               the residual a row-strided view, N = 128 and 256
  rgbias       row-group bias (rowgroup_rows 25, 1, > M), N = 128, 256, 512, 384    linear_kernel<T, 4, NONE> and - at N = 256, 512, which
                                                                                   without the row-group bias are w2's - <T, 8, NONE>
  rgbias_act   row-group bias under ReLU and under Tanh at N = 256                  16-bit: linear_kernel<T, 8, RELU> and <T, 8, TANH>, which
                                                                                   gf_linear reaches in no other way
  rows         ops.linear_rows, a table with repeated rows and zero addresses       linear_kernel<T, 4 and 8, NONE, false, AROWS>
  rows_groups  ops.linear_rows with group_count (R = 25; counts 0, 1, 25; a tile    the same instances, the device-side counts
               without a wanted row)
  conv_s1/_s2  ops.conv1x1 at stride 1 (K = 32, 64, 224) and 2                      linear_kernel<T, 4, NONE, CONVX>
  upadd        ops.conv1x1_upsample_add: W = 5, 31, 32, 33; H = 1; h = 1; w = 1;    linear_kernel<T, 4, UPADD, CONVX>: the wrap path
               two images of H W = 99 (W >= 32) and 35 (W < 32) pixels              (up_W >= 32) and the division path
The AROWS instances of the other epilogues (ReLU, Tanh, LN, LN_RES, NB = 4 and 8) are reached by the GPU file on EVERY 16-bit line of the
ops.linear forms: ops.linear_rows on a table of the operand's own rows (a row of zeros: the zero address) must give ops.linear's bits -
which also pins w2's accumulation order to linear_kernel's (plain_wide, relu2, tanh2).  No dispatch branch of gf_linear, gf_linear_rows,
gf_conv1x1_nhwc or gf_conv1x1_upsample_add_nhwc is left without a line.

Reference.  float64 of the formula in k3_linear.hip's header on exactly the kernel's operands (A, W, row-group bias, residual, lo as
stored, cast to float64; bias, gamma, beta fp32): out = epi([A1|A2] W^T + bias + rowgroup_bias), LayerNorm = F.layer_norm in float64
with the caller's eps, LN_RES = res + LN where the flag is non-zero and res elsewhere, UPADD = W x + F.interpolate(lo, bilinear,
align_corners=True).

Unit.  |got - ref| / (EPS_T scale + floor) per element over EVERY element, (max, mean); scale = the sum of the absolute values of the
terms the element is made of: plain epilogues sum_k |a w| + |bias| + |rgb| (= S below); LayerNorm |x - mean| rstd |gamma| + |beta|
(+ |res|); Tanh |tanh|; UPADD sum_k |x w| + the bilinear weights on |lo|.  floor = SPACING_T, and where the element is a function of
the fp32 pre-activation x rather than x itself, what one fp32 rounding of x's terms (EPS_fp32 S) does to it:
  Tanh       EPS_fp32 (S tanh'(x) + 4): the 16-bit form 1 - 2 rcp(exp(2x) + 1) is evaluated at magnitude 1 - exp, the addition, rcp and the
             subtraction's operand are each good to one fp32 ulp AT 1, whatever the size of tanh(x) (fp32 storage, tanhf: no + 4)
  LayerNorm  EPS_fp32 rstd |gamma| (S + the row's mean S): x - mean inherits the absolute rounding of x and of the mean
Rows that a zero flag skips are compared with torch.equal by the tests, not through the unit.  Non-finite: inf.

Restatement (restated()).  Contractions and sums in float64, rounded to fp32 once; products, quotients, square roots fp32 IEEE.
  accumulation  16-bit products are exact; one fp32 accumulator over all K steps and both operand parts.  16-bit storage: the contraction
                rounded once (the order of the fp32 sums is 2^-13 of the unit).  fp32 storage: a chain of fused multiply-adds, one rounding
                per product, in the kernel's order of k - there the order IS the error
  epilogue      + bias (fp32), + the row-group bias converted to fp32; the activation, or LayerNorm: two-pass on the unrounded
                accumulators, both row sums in the lanes' own order (_lane_sum), rstd = 1 / sqrt(q / C + eps), (x - mean) rstd gamma + beta;
                ONE rounding to T.  16-bit Tanh = 1 - 2 / (exp(2x) + 1), fp32 tanh
  LN_RES        16-bit: the LayerNorm value rounded to T, the residual added in fp32, rounded again; fp32: one add
  UPADD         the product rounded to T, the four weighted taps added in fp32 (weights from the kernel's fp32 coordinates), rounded to T"""
import math

import torch
import torch.nn.functional as F

import backward_regimes as B
import linear_attention_regimes as R

H16, BF16, F32 = R.H16, R.BF16, R.F32
EPS, NAME, SPACING = R.EPS, R.NAME, B.SPACING
rt, budget, key, term_error = R.rt, R.budget, R.key, B.term_error
_ein, _fn = B._ein, B._fn
ALL, SIXTEEN = (F32, H16, BF16), (H16, BF16)
M_ALL = (1, 31, 32, 33, 64, 65, 97, 127, 128, 129, 300)
GROUP_R = 25                                              # rows_groups: the fine windows' 25 rows - a 128-row tile straddles groups
# rows_groups: counts per group of 25 (G = 12 and G = 6 take the first G).  Tile 1 (rows 128 .. 255: rows 3 .. 24 of group 5, groups 6 .. 9,
# rows 0 .. 5 of group 10) holds no wanted row and is skipped; tile 0 is wanted by its first row, tile 2 (G = 12) by group 11 alone
GROUP_COUNTS = (25, 1, 0, 25, 1, 1, 0, 0, 0, 0, 0, 25)
TANH_ROW_SCALES = (0.0, 2.0 ** -24, 2.0 ** -12, 2.0 ** -4, 1.0, 4.0)
FLAG_PATTERN = (1, 0, -3, 2, 0)


def _sp(entry, epi, k, n, **kw):
    k1, k2 = k if isinstance(k, tuple) else (k, 0)
    d = dict(entry=entry, epi=epi, k1=k1, k2=k2, n=n, rg=0, fr=None, only=None, skip=(), Ms=M_ALL, bias=True, geom=None)
    d.update(kw)
    return d


def _conv(nimg, H, W, stride, cin, cout):
    return _sp('conv', 'none', cin, cout, bias=False, geom=(nimg, H, W, stride), Ms=(nimg * (H // stride) * (W // stride),))


def _up(nimg, H, W, h, w, cin, cout, ties=False):
    # up_ties runs where the bilinear weights take many values (ties=True: fifteenths; halves times eighteenths): with weights of 0, 1 / 2, 1 the
    # tap sum is an integer or a tie itself in most pixels, with or without the extra rounding the regime is about
    return _sp('upadd', 'upadd', cin, cout, bias=False, geom=(nimg, H, W, h, w), Ms=(nimg * H * W,), skip=() if ties else ('up_ties',))


CONTROL, EXACT = ('control', None), ('exact', None)
# form -> (storage types, regimes, launch shapes)
FORMS = {
    'plain': (ALL, (CONTROL, EXACT), [_sp('linear', 'none', k, n) for k, n in ((64, 32), (128, 96), (512, 128), (128, 160), (64, 224))]),
    'plain_wide': (ALL, (CONTROL, EXACT), [_sp('linear', 'none', k, n) for k, n in ((64, 256), (128, 512), (512, 768))]),
    'relu2': (ALL, (CONTROL, EXACT), [_sp('linear', 'relu', k, n) for k, n in (((64, 192), 256), ((192, 64), 512), ((256, 256), 768))]
              + [_sp('linear', 'relu', (32, 96), 256, only=(F32,))]),
    'relu2_nb4': (ALL, (CONTROL, EXACT), [_sp('linear', 'relu', (64, 192), 128), _sp('linear', 'relu', (192, 64), 96),
                                          _sp('linear', 'relu', (32, 64), 160, only=(F32,))]),
    'tanh2': (ALL, (CONTROL, ('tanh_span', None)),
              [_sp('linear', 'tanh', k, n) for k, n in (((64, 192), 256), ((192, 64), 512), ((256, 256), 768))]),
    'tanh_nb4': (ALL, (CONTROL, ('tanh_span', None)), [_sp('linear', 'tanh', 128, 128), _sp('linear', 'tanh', 64, 160)]),
    'ln': (ALL, (CONTROL, ('ln_offset', 10), ('ln_offset', 100), ('ln_offset', 1000), ('ln_flat', -5), ('ln_flat', -3), ('ln_range', -12),
                 ('ln_range', 17)), [_sp('linear', 'ln', 128, 128), _sp('linear', 'ln', 512, 256), _sp('linear', 'ln', 64, 256)]),
    'ln_res': (ALL, (CONTROL, ('res_dominant', None), ('res_tiny', None)),
               [_sp('linear', 'ln_res', 256, 128, fr=7), _sp('linear', 'ln_res', 512, 256, fr=50), _sp('linear', 'ln_res', 256, 256, fr=1),
                _sp('linear', 'ln_res', 128, 128, fr=1000), _sp('linear', 'ln_res', 128, 128)]),
    'rgbias': (ALL, (CONTROL, ('rgbias_dominant', None), ('rgbias_cancelling', None)),
               [_sp('linear', 'none', 128, 128, rg=25), _sp('linear', 'none', 128, 256, rg=1), _sp('linear', 'none', 64, 512, rg=1000),
                _sp('linear', 'none', 128, 384, rg=25)]),
    'rgbias_act': (ALL, (CONTROL,), [_sp('linear', 'relu', 128, 256, rg=25), _sp('linear', 'tanh', 64, 256, rg=7)]),
    'rows': (SIXTEEN, (CONTROL, EXACT), [_sp('rows', 'none', 128, 128), _sp('rows', 'none', 64, 96), _sp('rows', 'none', 256, 512)]),
    'rows_groups': (SIXTEEN, (CONTROL,), [_sp('rows', 'none', 128, 128, groups=12, Ms=(300,)), _sp('rows', 'none', 64, 256, groups=6, Ms=(150,))]),
    'conv_s1': (SIXTEEN, (CONTROL, EXACT), [_conv(2, 5, 13, 1, 64, 96), _conv(1, 9, 15, 1, 224, 160), _conv(1, 3, 3, 1, 32, 32)]),
    'conv_s2': (SIXTEEN, (CONTROL, EXACT), [_conv(2, 6, 10, 2, 64, 128), _conv(2, 16, 20, 2, 128, 96)]),
    'upadd': (SIXTEEN, (CONTROL, ('up_ties', None)),
              [_up(2, 3, 33, 2, 17, 64, 128), _up(2, 7, 5, 4, 3, 64, 96), _up(1, 1, 31, 1, 16, 32, 128), _up(2, 5, 32, 1, 1, 128, 160),
               _up(1, 4, 33, 2, 1, 32, 32), _up(3, 2, 31, 1, 9, 64, 224, ties=True), _up(2, 3, 37, 2, 11, 32, 96, ties=True)]),
}
LN_EPS = 1e-5


def specs(form, st, regime=None):
    return [sp for sp in FORMS[form][2] if (sp['only'] is None or st in sp['only']) and regime not in sp['skip']]


def lines(exact=False):
    """(form, regime, variant, type) of every line with a budget (exact=True: of the bit-exact lines, which need none)."""
    return [(f, r, v, st) for f, (types, regimes, _) in FORMS.items() for r, v in regimes if (r == 'exact') == exact for st in types]


def line_id(line):
    return f'{line[0]}/{key(line[1], line[2])}/{NAME[line[3]]}'


# ---------------------------------------------------------------------------------------------------------------------------
# cases (built once per process, read only)
# ---------------------------------------------------------------------------------------------------------------------------
def _gen(*tag):
    return torch.Generator().manual_seed(R._seed('k3', *tag))


def _tag(sp):
    return tuple(sorted((k, v) for k, v in sp.items() if k not in ('Ms', 'only', 'skip')))


def tile_rows_computed(counts, M):
    """The rows of gf_linear_rows' 128-row tiles that hold a wanted row (group_count): the rule in LinArgs' comment."""
    rows = torch.arange(M)
    wanted = (rows % GROUP_R) < torch.tensor(counts)[rows // GROUP_R]
    tiles = torch.zeros((M + 127) // 128, dtype=torch.bool)
    tiles[(rows[wanted] // 128).unique()] = True
    return tiles[rows // 128]


def make_case(sp, regime, variant, st):
    """One launch shape at its largest M: dict of the operands as stored (a = [A1|A2], gathered for the row forms, the pixel rows of a
    convolution) plus what steers them.
      control            unit-normal A, W ~ N(0, 1 / K), bias 0.5 N(0, 1)
      exact              A integers in [-15, 15], W integers / 8, bias integers / 8: every partial sum is a multiple of 1 / 8 below 2^17
      ln_offset r        a constant input channel of +-1 (alternating by row) against a weight column of r: |mean| / std = r
      ln_flat e          A times 2^-12 under a constant bias of 1 (variance 6e-8), every fifth row zero (variance 0); eps = 10^e
      ln_range v         A and W times 2^(v / 2), the bias times 2^v: pre-LayerNorm magnitudes of 2^v
      tanh_span          rows scaled by TANH_ROW_SCALES (0: the pre-activation IS the bias) under a bias of +-2^-20 ... +-60 along the channels
      rgbias_dominant    row-group bias 64 N(0, 1)
      rgbias_cancelling  non-negative A and W (no cancellation inside the product: S = the product), no fp32 bias; two rows of three repeat
                         their group's first row, and the group's bias is minus that row's float64 product rounded to T
      res_dominant / res_tiny   residual 64 N(0, 1) / 2^-10 N(0, 1)
      up_ties            x = the constant channel, W's column 0 = 1 / 2 (the product is exactly 0.5), lo integers at the bottom of the binade whose ulp is 1"""
    g = _gen(_tag(sp), regime, variant)
    M, K, N = max(sp['Ms']), sp['k1'] + sp['k2'], sp['n']
    case = dict(sp=sp, st=st, regime=regime, eps=LN_EPS)
    a = torch.randn(M, K, generator=g)
    w = torch.randn(N, K, generator=g) / K ** 0.5
    bias = 0.5 * torch.randn(N, generator=g) if sp['bias'] else None
    gamma, beta = 1 + 0.2 * torch.randn(N, generator=g), 0.1 * torch.randn(N, generator=g)
    res = torch.randn(M, N, generator=g)
    groups = (M + sp['rg'] - 1) // sp['rg'] if sp['rg'] else 0
    rgb = torch.randn(groups, N, generator=g) if groups else None
    ints = lambda *shape: torch.randint(-15, 16, shape, generator=g).float()     # noqa: E731
    if regime == 'exact':
        a, w = ints(M, K), ints(N, K) / 8
        bias = None if bias is None else torch.randint(-128, 129, (N,), generator=g).float() / 8
    elif regime == 'ln_offset':
        a[:, 0] = torch.where(torch.arange(M) % 2 == 0, 1.0, -1.0)
        w[:, 0] = float(variant)
    elif regime == 'ln_flat':
        a = a * 2.0 ** -12
        a[::5] = 0
        bias = torch.ones(N)
        case['eps'] = 10.0 ** variant
    elif regime == 'ln_range':
        a, w, bias = a * 2.0 ** (variant / 2), w * 2.0 ** (variant / 2), bias * 2.0 ** variant
    elif regime == 'tanh_span':
        a = a * torch.tensor(TANH_ROW_SCALES)[torch.arange(M) % len(TANH_ROW_SCALES)][:, None]
        bias = 2.0 ** torch.linspace(-20, math.log2(60), N) * torch.where(torch.arange(N) % 2 == 0, 1.0, -1.0)
    elif regime == 'rgbias_dominant':
        rgb = rgb * 64
    elif regime == 'rgbias_cancelling':
        a, w, bias = a.abs(), w.abs(), torch.zeros(N)
        own = torch.arange(M) % 3 == 1
        a = torch.where(own[:, None], a, a[(torch.arange(M) // sp['rg']) * sp['rg']])
    elif regime == 'res_dominant':
        res = res * 64
    elif regime == 'res_tiny':
        res = res * 2.0 ** -10
    if sp['entry'] == 'rows':
        # 40 source rows named by a table with repeats; a block of nine zero addresses (not with groups: every row has an address)
        idx = torch.randint(0, 40, (M,), generator=g)
        zero = torch.zeros(M, dtype=torch.bool)
        if M > 2:
            idx[M - 1] = idx[0]
        if 'groups' not in sp:
            zero[M // 3:M // 3 + 9] = True
            zero[0] = True                                     # M = 1: the only row is the zero address
        else:
            case['counts'] = GROUP_COUNTS[:sp['groups']]
            case['computed'] = tile_rows_computed(case['counts'], M)
        case.update(src=a[:40].to(st), idx=idx, zero=zero)
        a = case['src'].float()[idx].masked_fill(zero[:, None], 0)
    if sp['entry'] == 'conv':
        nimg, H, W, stride = sp['geom']
        x = (ints(nimg, H, W, K) if regime == 'exact' else torch.randn(nimg, H, W, K, generator=g)).to(st)
        case['x'] = x                                           # NHWC as stored
        a = x[:, ::stride, ::stride].reshape(M, K).float()
    if sp['entry'] == 'upadd':
        nimg, H, W, h, wl = sp['geom']
        x = torch.randn(nimg, H, W, K, generator=g)
        lo = torch.randn(nimg, h, wl, N, generator=g)
        if regime == 'up_ties':
            x[..., 1:] = 0
            x[..., 0] = 1
            w[:, 0] = 0.5
            base = 1.0 / EPS[st]                                # fp16: [1024, 1152), bf16: [128, 144): EPS_T times the value is the ulp, 1
            lo = base + torch.randint(0, int(base) // 8, lo.shape, generator=g).float()
        case.update(x=x.to(st), lo=lo.to(st))
        a = case['x'].reshape(M, K).float()
    case.update(a=a.to(st), w=w.to(st), bias=bias, gamma=gamma, beta=beta)
    if sp['epi'] == 'ln_res':
        case['res'] = res.to(st)
        if sp['fr'] is not None:
            nf = (M + sp['fr'] - 1) // sp['fr']
            case['flag'] = torch.tensor(FLAG_PATTERN, dtype=torch.int32)[torch.arange(nf) % len(FLAG_PATTERN)] if nf > 1 else torch.zeros(1, dtype=torch.int32)
    if rgb is not None:
        if regime == 'rgbias_cancelling':
            first = torch.arange(groups) * sp['rg']
            rgb = -(case['a'].double()[first] @ case['w'].double().T)
        case['rgb'] = rgb.to(st)
    case.update(reference(case))
    return case


def cached_case(sp, regime, variant, st):
    return R._cached(('k3', _tag(sp), regime, variant, st), lambda: make_case(sp, regime, variant, st))


def keep_rows(case, M=None):
    """bool [M]: rows whose flag is non-zero (all, without a flag)."""
    M = case['a'].shape[0] if M is None else M
    if 'flag' not in case:
        return torch.ones(M, dtype=torch.bool)
    return case['flag'][torch.arange(M) // case['sp']['fr']] != 0


# ---------------------------------------------------------------------------------------------------------------------------
# the float64 reference with its per-element scale and floor
# ---------------------------------------------------------------------------------------------------------------------------
def upadd_geometry(geom):
    """The kernel's fp32 coordinates of the bilinear taps: (y0, y1, wy1) per output row, (x0, x1, wx1) per output column."""
    _, H, W, h, wl = geom
    out = []
    for size, lo in ((H, h), (W, wl)):
        r = torch.tensor(float(lo - 1)) / torch.tensor(float(size - 1)) if size > 1 else torch.tensor(0.0)
        f = r * torch.arange(size, dtype=torch.float32)
        i0 = f.to(torch.int64)
        out.append((i0, i0 + (i0 < lo - 1), f - i0.float()))
    return out


def reference(case):
    sp, st = case['sp'], case['st']
    A, W = case['a'].double(), case['w'].double()
    M, N = A.shape[0], W.shape[0]
    acc, S = A @ W.T, A.abs() @ W.abs().T
    if case['bias'] is not None:
        acc, S = acc + case['bias'].double(), S + case['bias'].double().abs()
    if 'rgb' in case:
        rows = case['rgb'].double()[torch.arange(M) // sp['rg']]
        acc, S = acc + rows, S + rows.abs()
    floor = torch.full_like(acc, SPACING[st])
    if sp['epi'] == 'none':
        ref, scale = acc, S
    elif sp['epi'] == 'relu':
        ref, scale = torch.relu(acc), S
    elif sp['epi'] == 'tanh':
        ref = torch.tanh(acc)
        scale = ref.abs()
        floor = floor + EPS[F32] * (S * (1 - ref * ref) + (0.0 if st == F32 else 4.0))
    elif sp['epi'] in ('ln', 'ln_res'):
        ga, be = case['gamma'].double(), case['beta'].double()
        ref = F.layer_norm(acc, (N,), ga, be, case['eps'])
        mean = acc.mean(-1, keepdim=True)
        rstd = 1 / torch.sqrt(((acc - mean) ** 2).mean(-1, keepdim=True) + case['eps'])
        scale = (acc - mean).abs() * rstd * ga.abs() + be.abs()
        floor = floor + EPS[F32] * rstd * ga.abs() * (S + S.mean(-1, keepdim=True))
        if sp['epi'] == 'ln_res':
            res, keep = case['res'].double(), keep_rows(case)[:, None]
            ref, scale = torch.where(keep, res + ref, res), torch.where(keep, scale + res.abs(), res.abs())
    else:
        nimg, H, Wd, h, wl = sp['geom']
        lo = case['lo'].double().permute(0, 3, 1, 2)
        up = lambda t: F.interpolate(t, size=(H, Wd), mode='bilinear', align_corners=True).permute(0, 2, 3, 1).reshape(M, N)   # noqa: E731
        ref, scale = acc + up(lo), S + up(lo.abs())
    return dict(ref=ref, scale=scale, floor=floor)


# ---------------------------------------------------------------------------------------------------------------------------
# the restatement and its mutations
# ---------------------------------------------------------------------------------------------------------------------------
MUTATIONS = ('ln_unbiased', 'ln_no_eps', 'ln_one_pass', 'ln_stats_rounded', 'act_after_round', 'bias_after_act', 'acc_rounded_per_step',
             'k_tail_dropped', 'a2_from_k1', 'rgbias_next_group', 'rgbias_after_round', 'flag_per_tile', 'res_single_round', 'up_taps_rounded')


def _accumulate(a, w, st, k1, mut):
    K = a.shape[1]
    bk = 32 if st == F32 else 64
    if mut == 'a2_from_k1' and k1 < K:
        a2 = a[:, k1:].reshape(-1)
        a = torch.cat([a[:, :k1], torch.roll(a2, -k1).reshape(a.shape[0], K - k1)], 1)      # the elements that lie k1 further on in memory
    if mut == 'k_tail_dropped':
        a, w = a[:, :K - bk], w[:, :K - bk]
    if mut == 'acc_rounded_per_step':
        acc = torch.zeros(a.shape[0], w.shape[0])
        for k0 in range(0, K, bk):
            acc = rt((acc.double() + torch.einsum('mk,nk->mn', a[:, k0:k0 + bk].double(), w[:, k0:k0 + bk].double())).float(), st)
        return acc
    if st == F32:
        # fp32 storage: the accumulation IS the arithmetic - a chain of fused multiply-adds, one rounding per product, in the order the
        # matrix instructions take k: v_mfma_f32_32x32x2_f32 number t of a group of eight adds element t, then element 4 + t (Mma32<float>:
        # element t of both lane halves' fragments)
        acc, ad, wd = torch.zeros(a.shape[0], w.shape[0]), a.double(), w.double()
        for k0 in range(0, a.shape[1], 8):
            for k in (k0, k0 + 4, k0 + 1, k0 + 5, k0 + 2, k0 + 6, k0 + 3, k0 + 7):
                acc = (acc.double() + ad[:, k, None] * wd[None, :, k]).float()
        return acc
    return _ein('mk,nk->mn', a, w)


def _lane_sum(x, square=False):
    """The LayerNorm epilogue's row sums as the kernel takes them, [M, 1]: a lane adds its 16 NB channels one after the other in fp32 (the sum
    of squares as fused multiply-adds), in register order - channel nb * 32 + gf_acc_row(r, h) - and the two lane halves are added last.  With
    |mean| / std in the hundreds the order of this sum is most of what a row loses, in every storage type."""
    M, C = x.shape
    halves = []
    for h in (0, 1):
        s = torch.zeros(M)
        for nb in range(C // 32):
            for r in range(16):
                v = x[:, nb * 32 + (r & 3) + 8 * (r >> 2) + 4 * h]
                s = (s.double() + v.double() * v.double()).float() if square else s + v
        halves.append(s)
    return (halves[0] + halves[1])[:, None]


def restated(case, mut=None):
    """The kernels' arithmetic with their rounding points (module docstring) -> fp32 [M, N] holding values of the storage type.  Mutations:
      ln_unbiased       q / (C - 1)                              ln_no_eps        rstd = 1 / sqrt(q / C)
      ln_one_pass       variance = E[x^2] - mean^2 in fp32       ln_stats_rounded mean and variance from the accumulators rounded to T
      act_after_round   the pre-activation rounded to T, then the activation       bias_after_act   act(product) + bias
      acc_rounded_per_step  the accumulators rounded to T after every K step (64 elements; fp32 storage: no effect)
      k_tail_dropped    the last K step never added              a2_from_k1       the second operand read k1 elements further on
      rgbias_next_group the group of row + 1                     rgbias_after_round  product + bias rounded to T, then the row-group bias
      flag_per_tile     the flag of the 128-row tile's first row for all its rows
      res_single_round  16-bit LN_RES without the intermediate rounding (what the kernel does NOT do)
      up_taps_rounded   the bilinear sum rounded to T before it is added"""
    sp, st = case['sp'], case['st']
    a, w = case['a'].float(), case['w'].float()
    M, N = a.shape[0], w.shape[0]
    if sp['epi'] == 'upadd':
        prod = rt(_accumulate(a, w, st, sp['k1'], mut), st)
        nimg, H, Wd, h, wl = sp['geom']
        (y0, y1, wy1), (x0, x1, wx1) = upadd_geometry(sp['geom'])
        wy0, wx0 = 1 - wy1, 1 - wx1
        lo = case['lo'].double()
        t = 0
        for yi, wy in ((y0, wy0), (y1, wy1)):
            for xi, wx in ((x0, wx0), (x1, wx1)):
                t = t + (wy[:, None] * wx[None, :]).double()[None, :, :, None] * lo[:, yi][:, :, xi]
        t = t.reshape(M, N)
        if mut == 'up_taps_rounded':
            t = rt(t.float(), st).double()
        return rt((prod.double() + t).float(), st)
    x = _accumulate(a, w, st, sp['k1'], mut)
    bias = case['bias'] if case['bias'] is not None else torch.zeros(N)
    if mut != 'bias_after_act':
        x = x + bias
    if 'rgb' in case:
        grp = (torch.arange(M) + (1 if mut == 'rgbias_next_group' else 0)) // sp['rg']
        if mut == 'rgbias_after_round':
            x = rt(x, st)
        x = x + case['rgb'].float()[grp.clamp_max(case['rgb'].shape[0] - 1)]
    if mut == 'act_after_round' and sp['epi'] in ('relu', 'tanh'):
        x = rt(x, st)
    if sp['epi'] == 'relu':
        x = torch.relu(x)
    elif sp['epi'] == 'tanh':
        x = _fn(torch.tanh, x) if st == F32 else 1.0 - 2.0 * (1.0 / (_fn(torch.exp, 2.0 * x) + 1.0))
    elif sp['epi'] in ('ln', 'ln_res'):
        C = torch.tensor(float(N))
        xs = rt(x, st) if mut == 'ln_stats_rounded' else x
        mean = _lane_sum(xs) / C
        if mut == 'ln_one_pass':
            q = _lane_sum(xs, square=True) - C * mean * mean
        else:
            q = _lane_sum(xs - mean, square=True)
        var = q / (C - 1 if mut == 'ln_unbiased' else C)
        rstd = 1.0 / torch.sqrt(var + (0.0 if mut == 'ln_no_eps' else torch.tensor(case['eps'], dtype=torch.float32)))
        x = (x - mean) * rstd * case['gamma'] + case['beta']
        if sp['epi'] == 'ln_res':
            keep = keep_rows(case)
            if mut == 'flag_per_tile':
                keep = keep[(torch.arange(M) // 128) * 128]
            res = case['res'].float()
            upd = res + (x if st == F32 or mut == 'res_single_round' else rt(x, st))
            x = torch.where(keep[:, None], upd, res)
    if mut == 'bias_after_act':
        x = x + bias
    return rt(x, st)


def case_error(got, case, M):
    """(max, mean) over every element of the first M rows (group_count: of the rows of the tiles that hold a wanted row)."""
    got = got.detach().double().cpu().reshape(M, -1)
    ref, scale, floor = case['ref'][:M], case['scale'][:M], case['floor'][:M]
    if 'computed' in case:
        sel = case['computed'][:M]
        got, ref, scale, floor = got[sel], ref[sel], scale[sel], floor[sel]
    return term_error(got, ref, scale, case['st'], floor)


def worse(worst, err):
    return err if worst is None else (max(worst[0], err[0]), max(worst[1], err[1]))


def restatement_error(form, regime, variant, st, mut=None):
    """The restatement's - or a mutant's - (max, mean) against float64: the worst of the form's shapes and row counts."""
    worst = None
    for sp in specs(form, st, regime):
        case = cached_case(sp, regime, variant, st)
        out = restated(case, mut)
        for M in sp['Ms']:
            worst = worse(worst, case_error(out[:M], case, M))
    return worst


def exact_mismatches(form, st, mut=None):
    """The exact regime: elements of the restatement (or a mutant) that are not the float64 result rounded once, over the form's shapes."""
    bad = 0
    for sp in specs(form, st):
        case = cached_case(sp, 'exact', None, st)
        bad += int((restated(case, mut) != rt(case['ref'].float(), st)).sum())
    return bad


# ---------------------------------------------------------------------------------------------------------------------------
# What the restatement loses against float64, (max, mean) per line, measured by tests/test_linear_regimes.py (test_restatement_table: the
# measured value may not exceed its line, and the line is not slack) and rounded up.  A kernel may lose budget() of its line - max + 2 ulp,
# 1.5 x mean + 0.05 ulp: fp32 sums in another order, v_exp_f32, v_rcp_f32, contracted multiply-adds.  Nothing here was measured against a kernel.
# The exact lines have no entry: their outputs are the float64 result rounded once, bit for bit.
# ---------------------------------------------------------------------------------------------------------------------------
REST = {
    'plain/control/fp32': (2.55, 0.195),
    'plain/control/fp16': (0.35, 0.031),
    'plain/control/bf16': (0.35, 0.031),
    'plain_wide/control/fp32': (2.45, 0.172),
    'plain_wide/control/fp16': (0.35, 0.030),
    'plain_wide/control/bf16': (0.35, 0.031),
    'relu2/control/fp32': (2.60, 0.093),
    'relu2/control/fp16': (0.20, 0.010),
    'relu2/control/bf16': (0.20, 0.010),
    'relu2_nb4/control/fp32': (1.90, 0.101),
    'relu2_nb4/control/fp16': (0.20, 0.009),
    'relu2_nb4/control/bf16': (0.20, 0.009),
    'tanh2/control/fp32': (1.50, 0.134),
    'tanh2/control/fp16': (0.50, 0.168),
    'tanh2/control/bf16': (0.50, 0.175),
    'tanh2/tanh_span/fp32': (1.90, 0.106),
    'tanh2/tanh_span/fp16': (0.50, 0.119),
    'tanh2/tanh_span/bf16': (0.50, 0.130),
    'tanh_nb4/control/fp32': (1.15, 0.124),
    'tanh_nb4/control/fp16': (0.50, 0.169),
    'tanh_nb4/control/bf16': (0.50, 0.171),
    'tanh_nb4/tanh_span/fp32': (1.35, 0.101),
    'tanh_nb4/tanh_span/fp16': (0.50, 0.121),
    'tanh_nb4/tanh_span/bf16': (0.50, 0.125),
    'ln/control/fp32': (1.15, 0.088),
    'ln/control/fp16': (0.50, 0.165),
    'ln/control/bf16': (0.50, 0.160),
    'ln/ln_offset+10/fp32': (4.35, 0.846),
    'ln/ln_offset+10/fp16': (0.50, 0.161),
    'ln/ln_offset+10/bf16': (0.50, 0.160),
    'ln/ln_offset+100/fp32': (8.75, 1.499),
    'ln/ln_offset+100/fp16': (1.15, 0.160),
    'ln/ln_offset+100/bf16': (0.70, 0.159),
    'ln/ln_offset+1000/fp32': (7.40, 1.454),
    'ln/ln_offset+1000/fp16': (1.30, 0.172),
    'ln/ln_offset+1000/bf16': (1.05, 0.167),
    'ln/ln_flat-5/fp32': (1.80, 0.318),
    'ln/ln_flat-5/fp16': (1.60, 0.177),
    'ln/ln_flat-5/bf16': (0.85, 0.154),
    'ln/ln_flat-3/fp32': (2.25, 0.371),
    'ln/ln_flat-3/fp16': (1.00, 0.163),
    'ln/ln_flat-3/bf16': (0.60, 0.187),
    'ln/ln_range-12/fp32': (1.00, 0.085),
    'ln/ln_range-12/fp16': (0.50, 0.144),
    'ln/ln_range-12/bf16': (0.50, 0.149),
    'ln/ln_range+17/fp32': (0.95, 0.140),
    'ln/ln_range+17/fp16': (0.50, 0.159),
    'ln/ln_range+17/bf16': (0.50, 0.163),
    'ln_res/control/fp32': (1.00, 0.094),
    'ln_res/control/fp16': (0.95, 0.174),
    'ln_res/control/bf16': (0.90, 0.170),
    'ln_res/res_dominant/fp32': (0.65, 0.130),
    'ln_res/res_dominant/fp16': (0.85, 0.192),
    'ln_res/res_dominant/bf16': (0.75, 0.182),
    'ln_res/res_tiny/fp32': (0.90, 0.082),
    'ln_res/res_tiny/fp16': (1.00, 0.224),
    'ln_res/res_tiny/bf16': (1.00, 0.207),
    'rgbias/control/fp32': (2.05, 0.157),
    'rgbias/control/fp16': (0.35, 0.037),
    'rgbias/control/bf16': (0.35, 0.037),
    'rgbias/rgbias_dominant/fp32': (1.60, 0.167),
    'rgbias/rgbias_dominant/fp16': (0.50, 0.150),
    'rgbias/rgbias_dominant/bf16': (0.50, 0.155),
    'rgbias/rgbias_cancelling/fp32': (3.10, 0.577),
    'rgbias/rgbias_cancelling/fp16': (0.15, 0.008),
    'rgbias/rgbias_cancelling/bf16': (0.15, 0.008),
    'rgbias_act/control/fp32': (2.00, 0.115),
    'rgbias_act/control/fp16': (0.50, 0.160),
    'rgbias_act/control/bf16': (0.50, 0.164),
    'rows/control/fp16': (0.50, 0.193),
    'rows/control/bf16': (0.50, 0.193),
    'rows_groups/control/fp16': (0.30, 0.029),
    'rows_groups/control/bf16': (0.25, 0.029),
    'conv_s1/control/fp16': (0.30, 0.042),
    'conv_s1/control/bf16': (0.35, 0.039),
    'conv_s2/control/fp16': (0.25, 0.029),
    'conv_s2/control/bf16': (0.25, 0.029),
    'upadd/control/fp16': (0.55, 0.058),
    'upadd/control/bf16': (0.60, 0.060),
    'upadd/up_ties/fp16': (0.50, 0.265),
    'upadd/up_ties/bf16': (0.50, 0.266),
}


def rest(form, regime, variant, st):
    return REST[line_id((form, regime, variant, st))]


def line_budget(form, regime, variant, st):
    return budget(rest(form, regime, variant, st))
