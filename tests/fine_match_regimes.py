"""Fine matching forward (K8: gf_fine_match in csrc/k_fine.hip - fine_match or fine_match_mfma, then fine_count and fine_compact) against
float64: deterministic window generators per regime, the float64 reference (confidence, decision, keypoints), the derived error bound, a CPU
restatement of the scalar kernel's arithmetic with mutation switches, a model of the ordered compaction and the "clear decision" classifier
(imported by tests/test_fine_match_regimes.py and tests/test_fine_match_regimes_gpu.py, like tests/softmax_regimes.py).

Everything is deterministic (seeded torch generators, no fixtures).  Windows are f0, f1 [M, 25, C] in the storage type; every reference is
computed in float64 on those ALREADY ROUNDED values, so storage rounding is no part of any error measured here."""
import math

import torch

from linear_attention_regimes import _cached, _seed

U32 = 2.0 ** -24                      # fp32 unit roundoff
EPS = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7, torch.float32: 2.0 ** -23}   # one ulp at 1.0 of each storage type
WW, W = 25, 5
TEMP, THR = 0.1, 0.1
F32, H16, BF16 = torch.float32, torch.float16, torch.bfloat16
TYPES = (H16, BF16, F32)
CS = (128, 64, 16)
C_ODD = 72                            # C % 16 != 0: 16-bit storage falls back onto the scalar kernel
M_REG = 67                            # 17 four-match MFMA workgroups with a ragged last one; two 64-lane ballots
REGIMES = ('control', 'range', 'underflow', 'straddle', 'ties', 'nonfinite')
MUTATIONS = ('one_sided', 'scale_sqrtC', 'no_max', 'prob_bf16', 'tie_last', 'ge_thr', 'chunk_base')
COARSE_SCALE, C2F_SCALE, FINE_SCALE = 8.0, 4.0, 2.0      # hw0_i / hw0_c, hw0_f / hw0_c, hw0_i / hw0_f

# ---- the terms of log_tolerance (see its docstring)
K_LOGIT = 6                           # roundings of a logit besides its C accumulations
K_ARG = 2                             # roundings of an exponent argument
K_TAIL = 5                            # two reciprocals or divisions, two products by them, the final product
HW_ALLOWANCE = 2 * 64 * U32           # hardware exp2 / reciprocal: an ALLOWANCE, not a measurement (64 ulps of fp32 per element, shared by
#                                       the six hardware results an element depends on: ~10.7 ulp per call)
FLOOR = 4 * 2.0 ** -126               # absolute: flushed subnormal results (exp2, the products p * 1/sum, the final product)
KINDS = ('a', 'b', 'c', 'd', 'e')     # the ties regime: match m is of kind KINDS[m % 5]
# the nonfinite regime: match -> (side, value); matches 1 and 6 sit in four-match workgroups with finite matches, 63 ends the first ballot,
# 65 and 66 share the ragged last workgroup and the second ballot with the finite match 64
NONFINITE = {1: (0, math.inf), 6: (0, -math.inf), 63: (0, math.nan), 65: (1, math.inf), 66: (1, math.nan)}


def regime_thr(regime):
    """ties run at thr = 0 (every global maximum is accepted, so the tie-break is observable, kind (c)'s 1 / 625 included)."""
    return 0.0 if regime == 'ties' else THR


def regime_cs(regime, dtype):
    """The channel counts of a regime: straddle leaves out C = 16 (too noisy to place), and the 16-bit types add C = 72 (the scalar fallback)
    where the windows are not placed by bisection."""
    if regime == 'straddle':
        return (128, 64)
    return CS + ((C_ODD,) if dtype != F32 and regime in ('control', 'range', 'ties') else ())


# ---------------------------------------------------------------------------------------------------------------------------
# generators
# ---------------------------------------------------------------------------------------------------------------------------
def _dirs(g, n, C, lo=0, hi=None):
    """n directions of squared norm C, supported on channels lo .. hi: a pair of rows a u, b u has the logit a b / temperature."""
    hi = C if hi is None else hi
    u = torch.zeros(n, C, dtype=torch.float64)
    u[:, lo:hi] = torch.randn(n, hi - lo, generator=g, dtype=torch.float64)
    return u * math.sqrt(C) / u.norm(dim=-1, keepdim=True)


def _background(g, M, C, sigma=0.3):
    return (sigma * torch.randn(M, WW, C, generator=g, dtype=torch.float64), sigma * torch.randn(M, WW, C, generator=g, dtype=torch.float64))


def _cells(g, M):
    return torch.randint(0, WW, (M,), generator=g), torch.randint(0, WW, (M,), generator=g)


def _control(g, M, C, logit=None):
    """Background N(0, 0.3^2); one partner pair (i, j) per match, both rows a u with a^2 / temperature = `logit` (drawn in [1.2, 12] unless
    given: the peak confidence (e^L / (e^L + 24))^2 spans about 0.02 to 1; a third of the draws lie below thr = 0.1)."""
    f0, f1 = _background(g, M, C)
    i, j = _cells(g, M)
    u = _dirs(g, M, C)
    draw = 1.2 + 10.8 * torch.rand(M, generator=g, dtype=torch.float64) ** 2
    a = torch.sqrt((draw if logit is None else logit) * TEMP)
    ar = torch.arange(M)
    f0[ar, i] = a[:, None] * u
    f1[ar, j] = a[:, None] * u
    return f0, f1, i, j


def _range(g, M, C):
    """Every logit of a window is about s L with L in [300, 750] nats per match and s = +1 (even matches) or -1 (odd): all rows carry the
    common direction e (channels 0 .. C/2) with coefficients b (1 + eps_i) and s b (1 + eps'_j), b^2 / temperature = L, |eps| <= 2 / L - the
    softmaxes see differences of a few nats on top of the offset, which is where a fused scale or a missing maximum goes wrong.  Noise and
    ONE partner pair (worth 12 + 0.024 L nats: above what rounding b to bf16 moves) live on channels C/2 .. C, where values stay small."""
    H = C // 2
    L = 300.0 + 450.0 * torch.rand(M, generator=g, dtype=torch.float64)
    s = torch.where(torch.arange(M) % 2 == 0, 1.0, -1.0).double()
    b = torch.sqrt(L * TEMP)
    e = torch.zeros(C, dtype=torch.float64)
    e[:H] = math.sqrt(2.0)
    eps0 = (2 * torch.rand(M, WW, generator=g, dtype=torch.float64) - 1) * 2 / L[:, None]
    eps1 = (2 * torch.rand(M, WW, generator=g, dtype=torch.float64) - 1) * 2 / L[:, None]
    f0 = (b[:, None] * (1 + eps0))[..., None] * e
    f1 = ((s * b)[:, None] * (1 + eps1))[..., None] * e
    n0, n1 = _background(g, M, C)
    f0[..., H:] = n0[..., H:]
    f1[..., H:] = n1[..., H:]
    i, j = _cells(g, M)
    w = _dirs(g, M, C, H, C)
    c = torch.sqrt((12.0 + 0.024 * L) * TEMP)
    ar = torch.arange(M)
    f0[ar, i] += c[:, None] * w
    f1[ar, j] += c[:, None] * w
    return f0, f1, i, j


def _ties(g, M, C, dtype):
    """Match m is of kind KINDS[m % 5] (the header of tests/test_fine_match_regimes.py's tie test lists them)."""
    f0, f1 = _background(g, M, C)
    first = torch.zeros(M, dtype=torch.int64)
    borders = ([0, 1, 2, 3, 4], [0, 5, 10, 15, 20], [20, 21, 22, 23, 24], [4, 9, 14, 19, 24], list(range(10)))
    for m in range(M):
        kind = KINDS[m % 5]
        u = _dirs(g, 1, C)[0]
        a = math.sqrt(6.0 * TEMP)
        if kind in ('a', 'b'):
            p = torch.randperm(WW, generator=g)
            lo, hi, k = int(min(p[0], p[1])), int(max(p[0], p[1])), int(p[2])
            x, y = (f0, f1) if kind == 'a' else (f1, f0)
            x[m, lo] = a * u
            x[m, hi] = a * u
            y[m, k] = a * u
            first[m] = lo * WW + k if kind == 'a' else k * WW + lo
        elif kind == 'c':
            f0[m] = f0[m, :1].clone()
            f1[m] = f1[m, :1].clone()
            first[m] = 0
        elif kind == 'd':
            # redrawn until, on the rounded values, at least two cells are exactly 1.0 in float64 and no other cell is above 1/2 (a cell
            # at 1 - 1e-12 would be a tie in fp32 only); a handful of draws at C = 16, one or two otherwise
            for _ in range(1000):
                f0[m] = 6.0 * torch.randn(WW, C, generator=g, dtype=torch.float64)
                f1[m] = f0[m, torch.randperm(WW, generator=g)]
                conf = dual_softmax64(f0[m:m + 1].to(dtype), f1[m:m + 1].to(dtype))
                if int((conf == 1.0).sum()) >= 2 and not bool(((conf != 1.0) & (conf > 0.5)).any()):
                    break
            else:
                raise AssertionError('no saturated window found')
            first[m] = -1                                                    # whichever saturated cell comes first: the reference says
        else:
            z0 = borders[(m // 5) % len(borders)]
            z1 = borders[(m // 5 + 1) % len(borders)]
            free = [r for r in range(WW) if r not in z1]
            k = free[int(torch.randint(0, len(free), (1,), generator=g))]
            f0[m] = a * u + 0.05 * torch.randn(WW, C, generator=g, dtype=torch.float64)
            f1[m] = 0.05 * torch.randn(WW, C, generator=g, dtype=torch.float64)
            f1[m, k] = -a * u
            f0[m, z0] = 0.0
            f1[m, z1] = 0.0
            first[m] = min(z0) * WW + k
    return f0, f1, first


def _peak_of(sim, f1, i, j, row):
    """float64 confidence of cell (i_m, j_m) with f0's row i_m replaced by `row` [M, C] (already rounded); sim: the logits of the other rows."""
    C = f1.shape[-1]
    ar = torch.arange(f1.shape[0])
    sim = sim.clone()
    sim[ar, i] = torch.einsum('mc,mjc->mj', row, f1) / (C * TEMP)
    return torch.softmax(sim[ar, i], -1)[ar, j] * torch.softmax(sim[ar, :, j], -1)[ar, i]


def _straddle(g, M, C, dtype):
    """control windows whose partner row of f0 is rescaled per match until the float64 peak confidence on the ROUNDED operands sits at
    thr (1 - delta) (even matches) or thr (1 + delta) (odd): bisection on the scale, then the closest of 401 neighbouring scales (in 16-bit
    storage the peak is a step function of the scale, each step one element rounding the other way), then single elements of that row moved
    by one step of the type while that brings the peak closer.  delta: straddle_delta."""
    f0, f1, i, j = _control(g, M, C, logit=torch.full((M,), 2.4, dtype=torch.float64))
    ar = torch.arange(M)
    u = f1[ar, j] / math.sqrt(2.4 * TEMP)
    q0, q1 = f0.to(dtype).double(), f1.to(dtype).double()
    sim = torch.einsum('mic,mjc->mij', q0, q1) / (C * TEMP)
    rnd = lambda s: (s[:, None] * u).to(dtype).double()                         # noqa: E731
    delta = 2e-3
    for _ in range(2):
        target = THR * torch.where(ar % 2 == 0, 1 - delta, 1 + delta).double()
        lo, hi = torch.full((M,), 0.05, dtype=torch.float64), torch.full((M,), 3.0, dtype=torch.float64)
        for _ in range(48):
            mid = (lo + hi) / 2
            up = _peak_of(sim, q1, i, j, rnd(mid)) < target
            lo, hi = torch.where(up, mid, lo), torch.where(up, hi, mid)
        best, err = lo.clone(), torch.full((M,), math.inf, dtype=torch.float64)
        for t in range(-200, 201):
            s = lo * (1 + 2e-5 * t)
            e = (_peak_of(sim, q1, i, j, rnd(s)) / target - 1).abs()
            best, err = torch.where(e < err, s, best), torch.minimum(e, err)
        row = rnd(best)
        for c in range(C):                                                      # ... then single elements one step of the type up or down
            for step in (1 + EPS[dtype], 1 - EPS[dtype]):
                cand = row.clone()
                cand[:, c] = (row[:, c] * step).to(dtype).double()
                e = (_peak_of(sim, q1, i, j, cand) / target - 1).abs()
                row, err = torch.where((e < err)[:, None], cand, row), torch.minimum(e, err)
        out = q0.clone()
        out[ar, i] = row
        need = straddle_delta(out.to(dtype), q1.to(dtype))
        if need <= delta:
            break
        delta = need
    return out, q1, i, j, delta


def straddle_delta(f0, f1):
    """Twice the decision margin expm1(2 max bound) of the input, and at least 2e-3."""
    return max(2e-3, 2 * math.expm1(2 * float(log_tolerance(f0, f1).max())))


def windows(regime, dtype, C, M=M_REG):
    """One call's operands: dict(f0, f1 [M, 25, C] in dtype, thr, temperature) plus what the regime planted: i, j (partner cells), first (ties:
    the expected flat index, -1 where only the reference knows), delta and target (straddle), twin (nonfinite: the same call with finite
    windows in place of the non-finite ones) and bad (the non-finite matches).
      control    background rows N(0, 0.3^2); one partner pair per match at a strength drawn per match: peak confidence about 0.02 to 1
      range      all logits near +L or -L, L in [300, 750] nats, a few nats of structure on top; one partner pair, not a permutation
      underflow  one partner pair at 160 to 260 nats over a 0.3 background: it leads every other cell by >= 200 log2 units
      straddle   peak confidence at thr (1 -+ delta), alternating per match (C = 128, 64)
      ties       (a) two bit-identical rows of f0 partnered by one f1 row; (b) the same for columns; (c) every row of f0 equal and every row
                 of f1 equal; (d) f1 a permutation of f0's rows at feature scale 6 (several cells exactly 1.0 in float64); (e) zero rows as a
                 border window has them, tied at the top of one column.  thr = 0
      nonfinite  control windows; the matches of NONFINITE hold +inf, -inf or NaN in one element"""
    assert regime in REGIMES

    def make():
        g = torch.Generator().manual_seed(_seed('fine_match', 'control' if regime == 'nonfinite' else regime, C, M))
        out = {'thr': regime_thr(regime), 'temperature': TEMP}
        if regime in ('control', 'nonfinite'):
            f0, f1, out['i'], out['j'] = _control(g, M, C)
        elif regime == 'range':
            f0, f1, out['i'], out['j'] = _range(g, M, C)
        elif regime == 'underflow':
            f0, f1, out['i'], out['j'] = _control(g, M, C, logit=160.0 + 100.0 * torch.rand(M, generator=g, dtype=torch.float64))
        elif regime == 'straddle':
            f0, f1, out['i'], out['j'], out['delta'] = _straddle(g, M, C, dtype)
            ar = torch.arange(M)
            out['target'] = THR * torch.where(ar % 2 == 0, 1 - out['delta'], 1 + out['delta']).double()
        else:
            f0, f1, out['first'] = _ties(g, M, C, dtype)
        out['f0'], out['f1'] = f0.to(dtype), f1.to(dtype)
        if regime == 'nonfinite':
            out['twin'] = (out['f0'].clone(), out['f1'].clone())
            out['bad'] = sorted(m for m in NONFINITE if m < M)
            for m in out['bad']:
                side, v = NONFINITE[m]
                out['f1' if side else 'f0'][m, (3 * m) % WW, (5 * m + 1) % C] = v
        return out
    return _cached(('fine_match', regime, dtype, C, M), make)


# ---------------------------------------------------------------------------------------------------------------------------
# float64 reference
# ---------------------------------------------------------------------------------------------------------------------------
def first_max(flat):
    """(top, first) of flat [M, n]: the maximum and the SMALLEST index holding exactly that value, written out (torch.argmax promises no
    order among equal values).  A row with a NaN has top = NaN and first = -1."""
    top = flat.max(dim=1)[0]                                                    # propagates NaN
    idx = torch.arange(flat.shape[1]).expand_as(flat)
    first = torch.where(flat == top[:, None], idx, flat.shape[1]).min(dim=1)[0]
    return top, torch.where(first == flat.shape[1], -1, first)


def last_max(flat):
    top = flat.max(dim=1)[0]
    idx = torch.arange(flat.shape[1]).expand_as(flat)
    return top, torch.where(flat == top[:, None], idx, -1).max(dim=1)[0]


def dual_softmax64(f0, f1, temperature=TEMP):
    """O.dual_softmax in float64, evaluated in ONE order for every cell: the dot products as a broadcast product summed over the channels, not
    as a matrix product - a BLAS kernel may sum two bit-identical rows in different orders (seen on one CPU: the two tied cells of a kind (a)
    window came out one ulp apart, and the 'tie' had a winner).  Here cells with identical operands get identical bits, so a tie of the
    formula is a tie of the reference.  tests/test_fine_match_regimes.py holds it against O.dual_softmax itself."""
    c = f0.shape[-1]
    a, b = f0.double() / c ** .5, f1.double() / c ** .5
    sim = torch.cat([(a[s:s + 64, :, None, :] * b[s:s + 64, None, :, :]).sum(-1) for s in range(0, a.shape[0], 64)]) / temperature

    def softmax_last(x):                       # every reduction runs over a contiguous last axis: the same code for each row of it
        e = torch.exp(x - x.amax(-1, keepdim=True))
        return e / e.sum(-1, keepdim=True)
    return softmax_last(sim.transpose(1, 2).contiguous()).transpose(1, 2) * softmax_last(sim)


def reference(f0, f1, thr=THR, temperature=TEMP):
    """conf = O.dual_softmax in float64 on the rounded windows (as dual_softmax64 evaluates it); candidate = the global maximum of the 625
    cells, among equal cells the smallest flat index i * 25 + j; accepted iff max > thr (NaN > thr is false).
    -> dict(conf, top, first, sel): sel = first or -1."""
    conf = dual_softmax64(f0, f1, temperature)
    top, first = first_max(conf.flatten(1))
    ok = top > thr
    return {'conf': conf, 'top': top, 'first': first, 'sel': torch.where(ok, first, -1), 'ok': ok}


def keypoints64(sel, b_ids, mk0c, mk1c, scale0=None, scale1=None):
    """fine_matching2.py:93-116 in float64 for the accepted matches in ascending match order -> (mkpts0_f, mkpts1_f, budget0, budget1), each
    [count, 2].  c = mkpts_c / (coarse_scale * scale[b]) * c2f;  mkpts_f = (offset + c) * (fine_scale * scale[b]), offset (x, y) =
    (i % 5 - 2, i // 5 - 2) of the cell index on that side.
    Budget: the kernel rounds the division, the product by c2f, the sum and the final product - four fp32 roundings, each at most u32 of an
    intermediate no larger than (|offset| + |c|) fs: 4 u32 (|offset| + |c|) fs per coordinate.  (coarse_scale * scale and fine_scale * scale are
    exact here: 8 and 2 are powers of two.  The inputs are fp32 values taken as they are.)  Derived, not measured."""
    keep = torch.nonzero(sel >= 0)[:, 0]
    o = sel[keep]
    b = b_ids[keep]
    res = []
    for cell, mk, sc in ((o // WW, mk0c, scale0), (o % WW, mk1c, scale1)):
        s = 1.0 if sc is None else sc.double()[b]
        c = mk.double()[keep] / (COARSE_SCALE * s) * C2F_SCALE
        off = torch.stack([cell % W - W // 2, cell // W - W // 2], 1).double()
        fs = FINE_SCALE * s
        res.append(((off + c) * fs, 4 * U32 * (off.abs() + c.abs()) * fs))
    return res[0][0], res[1][0], res[0][1], res[1][1]


# ---------------------------------------------------------------------------------------------------------------------------
# bound
# ---------------------------------------------------------------------------------------------------------------------------
def log_tolerance(f0, f1, temperature=TEMP):
    """Bound on |ln conf_k - ln conf_ref| per element [M, 25, 25] (nats), from fp32 arithmetic on the rounded windows; a function of the
    inputs alone.  ln conf = (x - cmax) - ln csum + (x - rmax) - ln rsum with x = f0 . f1 / (C temperature).
    * a logit is an fp32 sum of C products (exact products of 16-bit values; fused into the sum for fp32 storage): C accumulations, and
      K_LOGIT = 6 more roundings - the scalar kernel divides both operands by sqrtf(C) (2, and the root's own rounding twice: 2), divides by
      the temperature (1), which is fp32(temperature) (1); the MFMA kernel builds log2(e) / (C temperature) (3), multiplies once (1), fp32
      (temperature) (1): |error| <= dl = (C + 6) u32 sum_c |f0_c f1_c| / (C temperature), taken as the max over the row and over the column;
    * ln conf holds four logits (2 + 1 + 1 dl) and the two sums, whose terms carry two logit errors each (2 + 2 dl): 8 dl;
    * forming the exponent arguments: the subtraction of the maximum and the exponential's change of base, K_ARG = 2 roundings of an argument
      no larger than |x| + |max|, over both factors: 2 u32 (2 |x| + |rmax| + |cmax|);
    * two fp32 sums of 25 terms: 2 * 25 u32;
    * two reciprocals or divisions, the two products by them and the final product: K_TAIL = 5 u32;
    * HW_ALLOWANCE = 2 * 64 u32 for the hardware exp2 and reciprocal instructions of the MFMA kernel (and libm's expf of the scalar one),
      whose accuracy no text at hand states: the allowance k1_log_tolerance grants (its 2 (n + 64) u32 with n = 25 is the sum of this term
      and the one above it) - 64 ulps of fp32 per element over the six such results an element depends on (two numerators, two sums of
      them, two reciprocals), ~10.7 ulp per call.  An allowance, not a measurement.
    Absolute, beside this bound (conf_error): FLOOR = 4 * 2^-126 for results flushed below the normal range - a flushed exp2 (times a factor
    <= 1), a flushed p * (1 / sum), the flushed final product, and the reference's own value below fp32's range.
    At |logit| ~ 40, C = 128: 8 * 134 u32 * 40 = 2.6e-3 nats; at 750: 4.8e-2."""
    C = f0.shape[-1]
    a, b = f0.double(), f1.double()
    sab = torch.einsum('mic,mjc->mij', a.abs(), b.abs()) / (C * temperature)
    dl = (C + K_LOGIT) * U32 * torch.maximum(sab.amax(2, keepdim=True), sab.amax(1, keepdim=True))
    x = torch.einsum('mic,mjc->mij', a, b) / (C * temperature)
    arg = 2 * x.abs() + x.amax(2, keepdim=True).abs() + x.amax(1, keepdim=True).abs()
    return 8 * dl + K_ARG * U32 * arg + (2 * WW + K_TAIL) * U32 + HW_ALLOWANCE


def conf_error(got, ref, tol):
    """error / bound per element: conf_k must lie in [ref e^-tol - FLOOR, ref e^tol + FLOOR]; the distance from ref in units of the distance
    to that side's end.  NaN or inf where the reference is finite counts as infinite."""
    got = got.double()
    d = got - ref
    r = torch.where(d >= 0, d / (ref * torch.expm1(tol) + FLOOR), -d / (-ref * torch.expm1(-tol) + FLOOR))
    return torch.where(torch.isfinite(r), r, math.inf)


def report(what, r):
    mx, mean = float(r.max()), float(r.mean())
    print(f'  {what}: error / bound max {mx:.4f} mean {mean:.5f}')
    return mx, mean


def margins(tol):
    """Per match, the relative margin a decision needs to be taken alike by any confidence within the bound (both sides of a comparison may
    move by tol): expm1(2 max tol) over the match's cells, and at least 1e-4 (softmax_regimes.k1_match_rel)."""
    return torch.clamp(torch.expm1(2 * tol.flatten(1).amax(1)), min=1e-4)


def clear(ref, tol, thr):
    """[M] bool: the match's decision is the same for every confidence within the bound of ref['conf'] that keeps exact ties tied.
    (i) the top cell leads every cell that is not EXACTLY equal to it by the relative margin (equal cells are a tie, which the first-index rule
    decides; the kernels compute tied cells from identical operands in identical order);  (ii) the maximum lies outside thr (1 +- margin) -
    at thr = 0 that is max > 0 (a global maximum is its row's and its column's: >= 1 / 625), and at thr >= 1 nothing can be accepted (every
    factor is exp(<= 0) / (sum >= 1) <= 1 in any arithmetic), which is how '>' and '>=' are told apart.
    A window with a non-finite element is clear when the reference holds a NaN: rejected, under any evaluation order."""
    conf = ref['conf'].flatten(1)
    nan = torch.isnan(conf).any(1)
    mg = torch.where(nan, 0.0, margins(torch.nan_to_num(tol)))
    top = ref['top'][:, None]
    lead = ((conf == top) | (conf <= top * (1 - mg[:, None]))).all(1)
    if thr >= 1.0:
        away = torch.ones_like(lead)
    elif thr == 0.0:
        away = ref['top'] >= 1.0 / (WW * WW) * (1 - mg)
    else:
        away = (ref['top'] - thr).abs() > mg * thr
    return torch.where(nan, ~ref['ok'], lead & away)


# ---------------------------------------------------------------------------------------------------------------------------
# the scalar kernel restated in fp32 on the CPU, with mutations
# ---------------------------------------------------------------------------------------------------------------------------
def _fn(f, x):
    return f(x.double()).float()


def _sum32(x, dim):
    """fp32 sum in index order from 0 (s += x[k] in a kernel)."""
    acc = torch.zeros_like(x.select(dim, 0))
    for k in range(x.shape[dim]):
        acc = acc + x.select(dim, k)
    return acc


def restated(f0, f1, thr=THR, temperature=TEMP, mut=None):
    """fine_match<T> in fp32: operands divided by sqrtf(C), an fma loop over the channels in index order, division by the temperature, each
    softmax from its own maximum (expf, sums in index order, divisions), the product; the packed-key arg-max (largest bits, then smallest
    index; NaN bits beat every finite value) and v > thr.  -> (conf fp32 [M, 25, 25], sel int64 [M]).  Mutations:
      one_sided    conf = the row softmax alone             scale_sqrtC  only one operand divided by sqrt(C)
      no_max       no maximum subtracted                    prob_bf16    both probabilities rounded to bf16 before the product
      tie_last     the last index wins a tie                ge_thr       v >= thr"""
    C = f0.shape[-1]
    rs = torch.sqrt(torch.tensor(float(C)))
    temp = torch.tensor(temperature, dtype=torch.float32)
    s0, s1 = f0.float() / rs, f1.float() if mut == 'scale_sqrtC' else f1.float() / rs
    acc = torch.zeros(f0.shape[0], WW, WW)
    for c in range(C):
        acc = (acc.double() + s0[:, :, None, c].double() * s1[:, None, :, c].double()).float()
    sim = acc / temp
    zero = torch.zeros(())
    rmax = zero if mut == 'no_max' else sim.amax(2, keepdim=True)
    cmax = zero if mut == 'no_max' else sim.amax(1, keepdim=True)
    er, ec = _fn(torch.exp, sim - rmax), _fn(torch.exp, sim - cmax)
    pr, pc = er / _sum32(er, 2).unsqueeze(2), ec / _sum32(ec, 1).unsqueeze(1)
    if mut == 'prob_bf16':
        pr, pc = pr.bfloat16().float(), pc.bfloat16().float()
    conf = pr if mut == 'one_sided' else pc * pr
    top, idx = (last_max if mut == 'tie_last' else first_max)(conf.flatten(1))
    ok = (top >= thr) if mut == 'ge_thr' else (top > thr)
    return conf, torch.where(ok & (idx >= 0), idx, -1)


def compaction_order(sel, chunk=1024, mut=None):
    """fine_count / fine_compact on the CPU: a chunk's base is the sum of the counts of the chunks before it, an accepted match's slot its base
    plus the number of accepted matches before it in the chunk.  -> the match index written to each of the first `count` slots (-1: none).
    chunk_base: every chunk starts at slot 0."""
    M = sel.shape[0]
    ok = sel >= 0
    out = torch.full((M,), -1, dtype=torch.int64)
    base = 0
    for c0 in range(0, M, chunk):
        idx = torch.nonzero(ok[c0:c0 + chunk])[:, 0] + c0
        start = 0 if mut == 'chunk_base' else base
        out[start:start + len(idx)] = idx
        base += len(idx)
    return out[:int(ok.sum())]


# ---------------------------------------------------------------------------------------------------------------------------
# compaction and keypoint cases
# ---------------------------------------------------------------------------------------------------------------------------
COMPACT_M = (2125, 1025, 1024)        # large to small: the cached k8 workspace is reused at a smaller M
COMPACT_N = 3
COMPACT_FORMS = ((H16, 128), (F32, 16))                     # the MFMA kernel and the scalar one in front of fine_count / fine_compact
EDGE_MS, EDGE_CS = (5, 4, 3, 1), (128, 16)                  # launch edges: control windows at these M
SCALE0 = ((1.37, 0.81), (0.59, 1.93), (2.21, 1.12))          # per-sample (x, y); none of them 1
SCALE1 = ((0.73, 1.49), (1.81, 0.67), (1.07, 2.43))


def accept_pattern(M, pattern):
    """[M] bool, which matches get a strong partner.  'mixed': a seeded 50/50 mix, with chunk 0 holding whole 64-match runs of rejects
    (64 .. 127, 320 .. 383) and of accepts (128 .. 191, 448 .. 511), matches 1023, 1024 and M - 1 accepted.  'empty1' (M > 2048): the same
    with chunk 1 (1024 .. 2047) rejected entirely - at M = 2125 an empty chunk and an accepted match 1024 exclude each other, so that M
    runs both patterns.  'none': nothing is accepted."""
    g = torch.Generator().manual_seed(_seed('fine_match_accept', M))
    acc = torch.rand(M, generator=g) < 0.5
    for lo, v in ((64, False), (128, True), (320, False), (448, True)):
        acc[lo:lo + 64] = v
    for m in (1023, 1024, M - 1):
        if m < M:
            acc[m] = True
    if pattern == 'empty1':
        assert M > 2048
        acc[1024:2048] = False
    elif pattern == 'none':
        acc[:] = False
    else:
        assert pattern == 'mixed'
    return acc


def compaction_case(M, pattern, dtype=H16, C=128):
    """control-style windows whose partner strength is set per match: 4 to 12 nats where accept_pattern says so (peak confidence > 0.45),
    1.2 to 1.9 nats elsewhere (< 0.06); b_ids over N = 3 samples, non-integer coarse keypoints, per-sample scales.  With its float64
    reference and bound (cached)."""
    def make():
        g = torch.Generator().manual_seed(_seed('fine_match_compact', M, pattern, C))
        acc = accept_pattern(M, pattern)
        r = torch.rand(M, generator=g, dtype=torch.float64)
        f0, f1, i, j = _control(g, M, C, logit=torch.where(acc, 4.0 + 8.0 * r, 1.2 + 0.7 * r))
        out = {'f0': f0.to(dtype), 'f1': f1.to(dtype), 'thr': THR, 'temperature': TEMP, 'accept': acc, 'i': i, 'j': j,
               'b_ids': torch.randint(0, COMPACT_N, (M,), generator=g),
               'mkpts0_c': 640.0 * torch.rand(M, 2, generator=g), 'mkpts1_c': 640.0 * torch.rand(M, 2, generator=g),
               'scale0': torch.tensor(SCALE0), 'scale1': torch.tensor(SCALE1)}
        out['ref'] = reference(out['f0'], out['f1'], THR)
        out['tol'] = log_tolerance(out['f0'], out['f1'])
        return out
    return _cached(('fine_match_compact', M, pattern, dtype, C), make)


def case(regime, dtype, C, M=M_REG):
    """windows(...) with its float64 reference and bound (cached; shared by the tests and left unchanged)."""
    def make():
        w = dict(windows(regime, dtype, C, M))
        w['ref'] = reference(w['f0'], w['f1'], w['thr'])
        w['tol'] = log_tolerance(w['f0'], w['f1'])
        return w
    return _cached(('fine_match_case', regime, dtype, C, M), make)
