"""Off-nominal inputs for the backward kernels of the training step (csrc/k_train.hip, csrc/k4_attention_train.hip and their ops.* wrappers), their float64 references,
restatements with the kernels' rounding points (with switchable mutations), the per-element error measure and the recorded table
(imported by tests/test_backward_regimes.py and tests/test_backward_regimes_gpu.py; the generators, rt, EPS and budget() are those of
tests/linear_attention_regimes.py).

Entries.
  la    ops.linear_attention_backward (gf_linear_attention_backward: lb_state_partial, lb_query_pass, lb_source_pass), 8 heads of 32
  law   ops.window_linear_attention_backward (window_la_backward), 8 heads of 16, <= 32 tokens, no masks
  ln    ops.layernorm_forward / ops.layernorm_backward (ln_forward, ln_backward, ln_param_reduce)
  act   ops.activation_backward (no restatement: the float64 value rounded once IS the answer)
  fa    ops.full_attention_train_forward -> ops.full_attention_backward (tattn_fwd, tattn_delta, tattn_bwd_dq, tattn_bwd_dkv), 4 heads of 64
  fm    ops.fine_match_backward (fine_match_backward), 25 x 25 windows, fp32 arithmetic on fp32 / fp16 / bf16 features

References.  float64 autograd of the reference formula (O.linear_attention, O.full_attention, F.layer_norm, train/functional.py:dual_softmax)
on exactly the kernel's operands: q, k, v, dout as stored, cast to float64; dout is seeded noise rounded to the storage type.

Units.  |got - ref| / ulp per element over EVERY element, as (max, mean); ulp = EPS_T * scale + floor, scale the sum of the absolute
values of the terms the element is made of, from the float64 intermediates (the role of A in linear_attention_regimes.message_error).
Where scale == 0 (masked row, image without a valid key) the output must be an exact zero; anything non-finite is inf.
The floor is the storage type's own: below its normal range one ulp is the subnormal spacing SPACING_T (fp16 2^-24, bf16 2^-133), not
EPS_T times the value.  Every output stored in a 16-bit type carries SPACING_T; the attention entry adds the floor of P (SPACING_T, and no
less than fp32's smallest normal number: the hardware exp2 has no subnormal results) times the other operand's absolute sum where P and dS
enter a product (term_error's `floor`).  Gradients are where this shows: phi'(x) = exp(x) and a one-hot softmax put elements of dq, dk, dv many
orders below the largest - an element whose terms add up to 3e-7 is stored as 0 in fp16 - and EPS_T * scale alone would call that 33 ulp (la ramp),
210 ulp (law ramp), 1 / EPS_T (fa peaked) in the restatement and in any kernel.  For an element whose terms lie in the normal range nothing
changes: SPACING_T is the ulp of the type's smallest normal number."""
import math

import torch
import torch.nn.functional as F

import geoformer_oracle as O
import linear_attention_regimes as R

H16, BF16, F32 = R.H16, R.BF16, R.F32
EPS, NAME, ATT_EPS, LN_EPS = R.EPS, R.NAME, R.ATT_EPS, R.LN_EPS
rt, budget, key = R.rt, R.budget, R.key
GRADS = ('dq', 'dk', 'dv')
SPACING = {H16: 2.0 ** -24, BF16: 2.0 ** -133, F32: 0.0}       # the subnormal spacing (fp32 values here are never near theirs)


# fp32 arithmetic of the restatements, the same on every CPU: a contraction, a sum or a transcendental is evaluated in float64 and rounded
# to fp32 once (an fp32 sum in no particular order: torch's own order depends on the machine and its thread count, the kernels' is another
# one again - that difference is what budget()'s margin is for); products, quotients and square roots are IEEE operations in fp32.
def _ein(eq, *operands):
    return torch.einsum(eq, *(t.double() for t in operands)).float()


def _sum(x, dim, keepdim=False):
    return x.double().sum(dim, keepdim=keepdim).float()


def _fn(f, x):
    return f(x.double()).float()


def _phi32(x, at_zero=False):
    """elu(x) + 1 as the kernels evaluate it: x + 1 for x > 0 (at_zero: x >= 0), exp(x) otherwise."""
    return torch.where((x >= 0) if at_zero else (x > 0), x + 1, _fn(torch.exp, torch.clamp(x, max=0)))


def term_error(got, ref, scale, st, floor=None):
    """(max, mean) of |got - ref| / (EPS_T scale + floor) over EVERY element, floor = SPACING_T unless given; where scale == 0 the output must
    be an exact zero and counts as zero error.  Anything non-finite: (inf, inf)."""
    got = got.double().cpu()
    if not bool(torch.isfinite(got).all()):
        return math.inf, math.inf
    live = scale > 0
    if not bool((got[~live] == 0).all()):
        return math.inf, math.inf
    unit = EPS[st] * scale + (SPACING[st] if floor is None else floor)
    e = torch.where(live, (got - ref).abs() / unit.clamp_min(1e-300), torch.zeros_like(ref))
    return float(e.max()), float(e.mean())


# ---------------------------------------------------------------------------------------------------------------------------
# regimes: (name, variant) -> storage types
# ---------------------------------------------------------------------------------------------------------------------------
# la, law.  cold_q runs to -14 in fp16 too.  The forward table stops fp16 at -12 because round(phi(q)) is an fp16 subnormal below (phi(-14) = 8e-7,
# spacing 6e-8), and num = round(phi(q)) KV carries that into dden here: the restatement's dq is at 1.8 ulp at -13, 4.4 at -14, 15 at -15, 28 at
# -16 (window: 3.6, 8.4, 20, 72) - finite at every one, and -14 is kept, with the wide line that follows, because it is where the FORMER kernels
# left fp16's range: dnum = dout S / den and dden as fp16 operands are inf from -14 in the coarse form and from -13 in the window form
# (mutation z_in_operand; the present kernels keep S / den in fp32 and are finite to -16 and beyond).  cold_k in fp16 stops at -8 and few_keys
# runs the forward's offsets (FEW_KEYS_OFF3, +6 / +2 / -8 on the one-key image): the forward state KV, Ksum is the same state.
LA = {('control', None): (H16, BF16), ('hot', None): (H16, BF16),
      ('cold_q', -12): (H16, BF16), ('cold_q', -14): (H16, BF16), ('cold_qv', -13): (H16,),
      ('cold_k', -8): (H16, BF16), ('cold_k', -12): (BF16,),
      ('few_keys', 6): (H16,), ('few_keys', 2): (BF16,), ('few_keys', -8): (BF16,),
      ('wide_v', None): (H16, BF16), ('sparse_v', None): (H16, BF16), ('ramp', None): (H16, BF16)}
LA_SHAPES = ((300, 520),)                      # L2_TOK = 256: a ragged second L chunk; three S chunks, the last with 8 tokens
LA_SHAPES_CONTROL = ((300, 520), (256, 1))     # ... and one key: 1 / S = 1, a single chunk on both sides
LA_SHAPES_1280 = ((300, 1280),)                # few_keys and sparse_v place their keys among 1280
LAW = {('control', None): (H16, BF16), ('hot', None): (H16, BF16), ('cold_q', -12): (H16, BF16), ('cold_q', -14): (H16, BF16),
       ('cold_k', -8): (H16, BF16), ('cold_k', -12): (BF16,), ('ramp', None): (H16, BF16)}
LAW_SHAPES = ((7, 25), (6, 32), (3, 9), (5, 1))       # Nw no multiple of the four windows of a workgroup; Lw = 1 and 32: the ends of the range


def la_shapes(regime):
    return LA_SHAPES_1280 if regime in ('few_keys', 'sparse_v') else LA_SHAPES_CONTROL if regime == 'control' else LA_SHAPES


# ---------------------------------------------------------------------------------------------------------------------------
# linear attention: float64 reference with its per-element scales
# ---------------------------------------------------------------------------------------------------------------------------
def _dphi(x, at_zero=False):
    """phi'(x) of phi = elu + 1: 1 for x > 0, exp(x) otherwise."""
    return torch.where((x >= 0) if at_zero else (x > 0), torch.ones_like(x, dtype=torch.float64), torch.exp(torch.clamp(x.double(), max=0)))


def _split(t, h):
    return t.view(t.shape[0], t.shape[1], h, t.shape[2] // h)


def la_reference(q, k, v, dout, nhead, qm=None, km=None):
    """q, dout [N, L, C], k, v [N, S, C] as stored -> dict(dq, dk, dv: (float64 gradient, scale), each [N, *, C]).  The gradients are
    autograd's of O.linear_attention; the scales come from the written-out formula (k_train.hip's header), which is checked against
    autograd by tests/test_backward_regimes.py."""
    n, _, c = q.shape
    q64, k64, v64 = (_split(t.double(), nhead).clone().requires_grad_(True) for t in (q, k, v))
    g = _split(dout.double(), nhead)
    O.linear_attention(q64, k64, v64, qm, km, ATT_EPS).backward(g)
    qd, kd, vd = q64.detach(), k64.detach(), v64.detach()
    S = float(vd.size(1))
    qmf = 1.0 if qm is None else qm[:, :, None, None].double()
    kmf = 1.0 if km is None else km[:, :, None, None].double()
    Q, K, vs = O._phi(qd) * qmf, O._phi(kd) * kmf, vd * kmf / S
    KV, Ks = torch.einsum('nshd,nshv->nhdv', K, vs), K.sum(1)
    den = torch.einsum('nlhd,nhd->nlh', Q, Ks) + ATT_EPS
    num = torch.einsum('nlhd,nhdv->nlhv', Q, KV)
    z = S / den
    dnum = g * z[..., None]
    dden = -(g * num).sum(-1) * z / den
    s_dq = _dphi(qd) * qmf * (torch.einsum('nlhv,nhdv->nlhd', dnum.abs(), KV.abs()) + dden.abs()[..., None] * Ks[:, None])
    a_dkv = torch.einsum('nlhd,nlhv->nhdv', Q, dnum.abs())
    a_dks = torch.einsum('nlhd,nlh->nhd', Q, dden.abs())
    s_dk = _dphi(kd) * kmf * (torch.einsum('nshv,nhdv->nshd', vs.abs(), a_dkv) + a_dks[:, None])
    s_dv = kmf / S * torch.einsum('nshd,nhdv->nshv', K, a_dkv)
    manual = dict(dq=_dphi(qd) * qmf * (torch.einsum('nlhv,nhdv->nlhd', dnum, KV) + dden[..., None] * Ks[:, None]))
    dKV, dKs = torch.einsum('nlhd,nlhv->nhdv', Q, dnum), torch.einsum('nlhd,nlh->nhd', Q, dden)
    manual['dk'] = _dphi(kd) * kmf * (torch.einsum('nshv,nhdv->nshd', vs, dKV) + dKs[:, None])
    manual['dv'] = kmf / S * torch.einsum('nshd,nhdv->nshv', K, dKV)
    flat = lambda t: t.reshape(n, -1, c)                                          # noqa: E731
    out = {nm: (flat(gr.grad), flat(sc)) for nm, gr, sc in (('dq', q64, s_dq), ('dk', k64, s_dk), ('dv', v64, s_dv))}
    out['manual'] = {nm: flat(t) for nm, t in manual.items()}
    out['dden'] = dden
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# linear attention: the restatement
# ---------------------------------------------------------------------------------------------------------------------------
LA_MUTATIONS = ('drop_dden', 'phi_prime_at_zero', 'inv_valid', 'eps_dropped', 'mask_k_only', 'mask_v_only', 'dnum_unrounded', 'swap_heads',
                'swap_halves', 'z_in_operand')
LAW_MUTATIONS = ('drop_dden', 'phi_prime_at_zero', 'no_diag', 'z_in_operand')


def la_backward_restated(q, k, v, dout, st, nhead, qm=None, km=None, form='coarse', mut=None, swap=(1, 5), eps=ATT_EPS):
    """gf_linear_attention_backward (form 'coarse') and window_la_backward (form 'window') with their rounding points, fp32 elsewhere (sums
    as _ein / _sum take them).  q, dout [N, L, C], k, v [N, S, C] as stored -> (dq, dk, dv) fp32 holding values of st.
      state    K = round(phi(k) [mask]), vs = round(v / S [mask]) (1 / S an fp32 reciprocal); KV = K^T vs and Ksum = sum K in fp32
      query    den = phi(q) . Ksum + eps from the UN-rounded phi(q); num = round(KV)^T round(phi(q)); z = S / den;
               dden = -(dout . num) z / den in fp32;  dq = round((z (round(KV) dout) + dden Ksum) phi'(q)) - dout is stored in st, so the
               product has no rounded operand but KV, and z joins in fp32;
               gradient state: dKV = sum_l round(phi(q) z)^T dout, and
                 coarse  dKsum = sum_l round(phi(q) z) round(-(dout . num) / den)        window  dKsum = sum_l round(phi(q) dden)
      source   dk = round((round(dKV) vs + dKsum) phi'(k)) [mask], dv = round((round(dKV)^T round(phi(k))) / S) [mask]
    Mutations:
      z_in_operand   the kernels as they were before this suite: dnum = dout z and dden rounded to st as operands (round(dnum) against
                     round(KV) in dq, round(phi(q))^T round(dnum) in dKV, round(phi(q)) round(dden) in dKsum; window: round(phi(q) dden))
      drop_dden      no dden Ksum in dq and no dKsum in dk        phi_prime_at_zero  x >= 0 in place of x > 0 (phi and phi')
      inv_valid      1 / (valid keys) in place of 1 / S           eps_dropped        den without eps
      mask_k_only    the key mask on phi(k) but not on v          mask_v_only        on v but not on phi(k)   (in the state pass)
      dnum_unrounded z_in_operand with dnum left in fp32          no_diag            window: the two heads of a 32-channel block see each
      swap_heads / swap_halves  of the gradient state (dKV, dKsum): heads `swap` exchanged / the two halves of head swap[0]      other's state"""
    n, L, c = q.shape
    at0 = mut == 'phi_prime_at_zero'
    old = mut in ('z_in_operand', 'dnum_unrounded')
    phi = lambda x: _phi32(x, at0)                                               # noqa: E731
    qf, kf, vf, g = (_split(t.float(), nhead) for t in (q, k, v, dout))
    one = torch.tensor(1.0, dtype=torch.float32)
    S = torch.tensor(float(kf.shape[1]), dtype=torch.float32).expand(n)
    if mut == 'inv_valid' and km is not None:
        S = km.sum(1).clamp_min(1).float()
    inv_s = (one / S)[:, None, None, None]
    S3 = S[:, None, None]
    qmf = None if qm is None else qm[:, :, None, None].float()
    kmf = None if km is None else km[:, :, None, None].float()
    Kf, vsf = phi(kf), vf * inv_s
    K_src, vs_src = rt(Kf, st), rt(vsf, st)                                        # the source pass: its own (unmasked) operands
    if kmf is not None and mut != 'mask_v_only':
        Kf = Kf * kmf
    if kmf is not None and mut != 'mask_k_only':
        vsf = vsf * kmf
    K, vs = rt(Kf, st), rt(vsf, st)
    hd = K.shape[-1]
    blk = (lambda t: t.reshape(t.shape[0], t.shape[1], nhead // 2, 2 * hd)) if mut == 'no_diag' else (lambda t: t)
    unb = (lambda t: t.reshape(t.shape[0], t.shape[1], nhead, hd)) if mut == 'no_diag' else (lambda t: t)
    KV = _ein('nshd,nshv->nhdv', blk(K), blk(vs))
    Ks = _sum(K, 1)
    Qf = phi(qf)
    gl = g
    if qmf is not None:
        Qf, gl = Qf * qmf, g * qmf
    Qr, KVr = rt(Qf, st), rt(KV, st)
    den = _ein('nlhd,nhd->nlh', Qf, Ks) + (0.0 if mut == 'eps_dropped' else torch.tensor(eps, dtype=torch.float32))
    num = unb(_ein('nlhd,nhdv->nlhv', blk(Qr), KVr))
    dot = _sum(g * num, -1)
    z = S3 / den
    dden = -dot * z / den
    if qmf is not None:
        dden = dden * qmf[..., 0]
    dphi_q, dphi_k = _dphi(qf, at0).float(), _dphi(kf, at0).float()
    if old:
        dnum = gl * z[..., None]
        dnum_r = dnum if mut == 'dnum_unrounded' else rt(dnum, st)
        t = unb(_ein('nlhv,nhdv->nlhd', blk(dnum_r), KVr))
        dKV = _ein('nlhd,nlhv->nhdv', blk(Qr), blk(dnum_r))
        dKs = _ein('nlhd,nlh->nhd', Qr, rt(dden, st)) if form == 'coarse' else _sum(rt(Qf * dden[..., None], st), 1)
    else:
        t = unb(_ein('nlhv,nhdv->nlhd', blk(gl), KVr)) * z[..., None]
        Qz = rt(Qf * z[..., None], st)
        dKV = _ein('nlhd,nlhv->nhdv', blk(Qz), blk(gl))
        if form == 'coarse':
            w = -dot / den
            dKs = _ein('nlhd,nlh->nhd', Qz, rt(w if qmf is None else w * qmf[..., 0], st))
        else:
            dKs = _sum(rt(Qf * dden[..., None], st), 1)
    if mut == 'drop_dden':
        dden, dKs = torch.zeros_like(dden), torch.zeros_like(dKs)
    if mut == 'swap_heads':
        dKV, dKs = dKV.clone(), dKs.clone()
        dKV[:, list(swap)], dKs[:, list(swap)] = dKV[:, list(swap[::-1])], dKs[:, list(swap[::-1])]
    elif mut == 'swap_halves':
        a, half = swap[0], hd // 2
        dKV, dKs = dKV.clone(), dKs.clone()
        dKV[:, a] = torch.cat([dKV[:, a, half:], dKV[:, a, :half]], -2)
        dKs[:, a] = torch.cat([dKs[:, a, half:], dKs[:, a, :half]], -1)
    dq = (t + dden[..., None] * Ks[:, None]) * dphi_q
    if qmf is not None:
        dq = torch.where(qmf > 0, dq, torch.zeros_like(dq))                        # the kernel SELECTS: a dead row is zero whatever it computed
    dKVr = rt(dKV, st)
    dk = (unb(_ein('nshv,nhdv->nshd', blk(vs_src), dKVr)) + dKs[:, None]) * dphi_k
    dv = unb(_ein('nshd,nhdv->nshv', blk(K_src), dKVr)) * inv_s
    if kmf is not None:
        dk, dv = torch.where(kmf > 0, dk, torch.zeros_like(dk)), torch.where(kmf > 0, dv, torch.zeros_like(dv))
    return tuple(rt(x, st).reshape(n, -1, c) for x in (dq, dk, dv))


# ---------------------------------------------------------------------------------------------------------------------------
# cases (built once per process, read only)
# ---------------------------------------------------------------------------------------------------------------------------
def _noise(shape, st, *tag):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(R._seed('dout', *tag))).to(st)


def la_case(regime, variant, st, L, S):
    """(q, k, v, dout in st, qm, km, reference dict) of entry la: the projections of R.coarse_case's float64 forward, stored in st."""
    def make():
        case = R.coarse_case(regime, variant, st, L, S)
        q, k, v = R.k2_operands(case, st)
        dout = _noise(q.shape, st, 'la', regime, variant, L, S)
        return (q, k, v, dout, case['xm'], case['sm'], la_reference(q, k, v, dout, 8, case['xm'], case['sm']))
    return R._cached(('bwd_la', regime, variant, st, L, S), make)


def law_case(regime, variant, st, Nw, Lw):
    def make():
        q, k, v = R.window_operands(regime, variant, st, Nw, Lw, Lw)
        dout = _noise(q.shape, st, 'law', regime, variant, Nw, Lw)
        return (q, k, v, dout, la_reference(q, k, v, dout, 8))
    return R._cached(('bwd_law', regime, variant, st, Nw, Lw), make)


def grad_errors(got, ref, st):
    """((max, mean) of dq, of dk, of dv) from the kernel's or the restatement's (dq, dk, dv) and a reference dict."""
    return tuple(term_error(x, ref[nm][0], ref[nm][1], st) for nm, x in zip(GRADS, got))


def _worst(errs):
    errs = list(errs)
    return tuple((max(e[i][0] for e in errs), max(e[i][1] for e in errs)) for i in range(len(errs[0])))


def restatement_error(entry, regime, variant, st, mut=None):
    """The restatement's - or a mutant's - errors against float64, per gradient, the worst of the entry's shapes."""
    if entry == 'la':
        def one(shape):
            q, k, v, dout, qm, km, ref = la_case(regime, variant, st, *shape)
            return grad_errors(la_backward_restated(q, k, v, dout, st, 8, qm, km, 'coarse', mut, swap=(2, 2) if mut == 'swap_halves' else (1, 5)), ref, st)
        return _worst(one(s) for s in la_shapes(regime))
    if entry == 'law':
        def one(shape):
            q, k, v, dout, ref = law_case(regime, variant, st, *shape)
            return grad_errors(la_backward_restated(q, k, v, dout, st, 8, None, None, 'window', mut), ref, st)
        return _worst(one(s) for s in LAW_SHAPES)
    if entry == 'ln':
        return _worst(ln_errors(ln_restated(variant, st, mut, T), ln_case(variant, st), st, T) for T in LN_T)
    if entry == 'fa':
        def one(shape):
            q, k, v, dout, ref = fa_case(regime, st, *shape)
            return fa_errors(fa_restated(q, k, v, dout, st, mut), ref, st)
        return _worst(one(s) for s in fa_shapes())
    if entry == 'fm':
        def one(C):
            f0, f1, dconf, ref = fm_case(regime, st, C)
            return fm_errors(fm_restated(f0, f1, dconf, st, mut), ref, st)
        return _worst(one(C) for C in FM_C)
    raise KeyError(entry)


# ---------------------------------------------------------------------------------------------------------------------------
# LayerNorm: out, stats, dy, dgamma, dbeta
# ---------------------------------------------------------------------------------------------------------------------------
LN_BWD_WGS = 512                                   # k_train.hip: the backward's fixed number of workgroups, four rows each per step
LN_T = (5, 1003, 4 * LN_BWD_WGS + 5)               # parts = rows / 4 (< 512 workgroups) and parts = 512 with a second, ragged round of rows
LN_C = (128, 256, 512)
LN_RATIOS = {H16: (8.0, 32.0), BF16: (8.0, 32.0, 128.0)}
LN_MUTATIONS = ('two_term_dy', 'unbiased_variance', 'eps_dropped')
LN_OUT = ('out', 'dy', 'dgamma', 'dbeta', 'mean', 'rstd')


def ln_case(C, st):
    """T = sum(LN_T) rows in one tensor (the tests slice it): unit noise times 1.7 plus, on rows 1 .. , mean / std ratios of LN_RATIOS; row 0
    constant (variance 0: rstd = eps^-1/2), row 2 zeros.  Returns dict(y, dout in st, gamma, beta fp32, and the float64 reference per T)."""
    def make():
        g = torch.Generator().manual_seed(R._seed('ln', C))
        T = max(LN_T)
        y = torch.randn(T, C, generator=g) * 1.7
        ratios = LN_RATIOS[st]
        for i, r in enumerate(ratios):
            rows = slice(3 + i, None, 7)
            y[rows] += r * 1.7 * torch.where(torch.arange(y[rows].shape[0]) % 2 == 0, 1.0, -1.0)[:, None]
        y[0] = 3.25
        y[2] = 0.0
        y = y.to(st)
        gamma = 1 + 0.2 * torch.randn(C, generator=g)
        beta = 0.1 * torch.randn(C, generator=g)
        dout = torch.randn(T, C, generator=g).to(st)
        case = dict(y=y, dout=dout, gamma=gamma, beta=beta, C=C, st=st, ref={})
        for t in LN_T:
            case['ref'][t] = ln_reference(y[:t], dout[:t], gamma, beta)
        return case
    return R._cached(('bwd_ln', C, st), make)


def ln_reference(y, dout, gamma, beta):
    """float64 autograd of F.layer_norm on the stored y, dout -> name: (value, scale), with the mean and rstd of the stored y."""
    C = y.shape[-1]
    y64 = y.double().clone().requires_grad_(True)
    ga, be = gamma.double().clone().requires_grad_(True), beta.double().clone().requires_grad_(True)
    out = F.layer_norm(y64, (C,), ga, be, LN_EPS)
    d = dout.double()
    out.backward(d)
    yd = y64.detach()
    mean = yd.mean(-1, keepdim=True)
    rstd = 1 / torch.sqrt(((yd - mean) ** 2).mean(-1, keepdim=True) + LN_EPS)
    xh = (yd - mean) * rstd
    gg = d * gamma.double()
    s_out = (yd.abs() + mean.abs()) * rstd * gamma.double().abs() + beta.double().abs()
    s_dy = rstd * (gg.abs() + gg.abs().mean(-1, keepdim=True) + xh.abs() * (gg * xh).abs().mean(-1, keepdim=True))
    return dict(out=(out.detach(), s_out), dy=(y64.grad, s_dy), dgamma=(ga.grad, (d * xh).abs().sum(0)), dbeta=(be.grad, d.abs().sum(0)),
                mean=(mean[:, 0], yd.abs().mean(-1)), rstd=(rstd[:, 0], rstd[:, 0]))


def ln_restated(C, st, mut=None, T=None, case=None):
    """ln_forward / ln_backward in fp32: mean = sum / C, the CENTRED biased variance, rstd = 1 / sqrt(var + eps), out = round((y - mean) rstd
    gamma + beta); xhat = (y - mean) rstd from the saved statistics, g = dout gamma, dy = round(rstd (g - mean(g) - xhat mean(g xhat))),
    dgamma = sum dout xhat, dbeta = sum dout (fp32, not rounded).  two_term_dy drops xhat mean(g xhat); unbiased_variance divides by C - 1;
    eps_dropped: rstd = 1 / sqrt(var)."""
    case = case or ln_case(C, st)
    T = T or max(LN_T)
    y, d, ga, be = case['y'][:T].float(), case['dout'][:T].float(), case['gamma'], case['beta']
    mean = _sum(y, -1, True) * (1.0 / C)
    var = _sum((y - mean) ** 2, -1, True) * (1.0 / (C - 1 if mut == 'unbiased_variance' else C))
    rstd = _fn(torch.rsqrt, var + (0.0 if mut == 'eps_dropped' else LN_EPS))
    out = rt((y - mean) * rstd * ga + be, st)
    xh = (y - mean) * rstd
    g = d * ga
    m1, m2 = _sum(g, -1, True) * (1.0 / C), _sum(g * xh, -1, True) * (1.0 / C)
    dy = rt(rstd * (g - m1 - (0.0 if mut == 'two_term_dy' else xh * m2)), st)
    return dict(out=out, dy=dy, dgamma=_sum(d * xh, 0), dbeta=_sum(d, 0), mean=mean[:, 0], rstd=rstd[:, 0])


def ln_errors(got, case, st, T=None):
    """((max, mean) of out, dy in ulps of st; of dgamma, dbeta and the saved statistics (mean against mean |y|, rstd against itself) in
    ulps of FP32 - they are fp32 values, never rounded to st)."""
    ref = case['ref'][T or max(LN_T)]
    return tuple(term_error(got[nm], ref[nm][0], ref[nm][1], st if nm in ('out', 'dy') else F32) for nm in LN_OUT)


# ---------------------------------------------------------------------------------------------------------------------------
# activation backward
# ---------------------------------------------------------------------------------------------------------------------------
ACT_SIZES = (255, 4096 * 256 + 3)           # one ragged workgroup; the grid of 4096 workgroups of 256 plus a grid-stride tail of 3


def act_case(st, n):
    """(dh, h in st, float64 dz for 'relu' and 'tanh'): h in [-1, 1] (a tanh output; for ReLU its sign is what counts), with +-1 (saturated:
    the gradient is an exact zero), +-0, the smallest subnormals and the largest finite dh against h = 0, +-smallest and +-1 in front."""
    def make():
        g = torch.Generator().manual_seed(R._seed('act', n))
        h = (2 * torch.rand(n, generator=g) - 1).to(st)
        dh = (torch.randn(n, generator=g) * 2).to(st)
        tiny, big = torch.finfo(st).smallest_normal * 2.0 ** (-10 if st == H16 else -7), torch.finfo(st).max
        hs = torch.tensor([1.0, -1.0, 0.0, -0.0, tiny, -tiny, 0.0, tiny, 1.0, -1.0, 0.5, -0.5, tiny, 1 - EPS[st] / 2, -(1 - EPS[st] / 2)])
        ds = torch.tensor([1.5, -2.5, 3.0, 3.0, 1.0, 1.0, big, -big, big, -big, big, tiny, tiny, big, 1.0])
        h[:hs.numel()], dh[:ds.numel()] = hs.to(st), ds.to(st)
        h64, d64 = h.double(), dh.double()
        return dh, h, {'relu': torch.where(h64 > 0, d64, torch.zeros_like(d64)), 'tanh': d64 * (1 - h64 * h64)}
    return R._cached(('bwd_act', st, n), make)


def ordered(t):
    """A 16-bit float tensor as integers in value order (+0 and -0 both 0): neighbours differ by 1."""
    i = t.contiguous().view(torch.int16).to(torch.int32)
    return torch.where(i < 0, -(i & 0x7FFF), i)


# ---------------------------------------------------------------------------------------------------------------------------
# What the restatements lose against float64: 'entry/regime/type' -> ((max, mean) per output), measured by tests/test_backward_regimes.py
# (test_restatement_table: the measured value may not exceed its line, and the line is not slack) and rounded up.
#   la, law: (dq, dk, dv).     ln: (out, dy, dgamma, dbeta, mean, rstd), keyed 'ln/c+C/type', all but out and dy in ulps of fp32.
#   fa: (out, lse2, dq, dk, dv), lse2 in ulps of fp32, the worst of the fifteen shapes.     fm: (df0, df1), the worse of C = 128 and 64.
# A kernel may lose budget() of its line - max + 2 ulp, 1.5 x mean + 0.05 ulp - for the reasons stated there: fp32 sums in another order,
# v_exp_f32, v_rcp_f32.  Nothing here was measured against a kernel.
# ---------------------------------------------------------------------------------------------------------------------------
REST = {
    'la/control/fp16': ((0.50, 0.066), (0.10, 0.007), (0.20, 0.013)),
    'la/control/bf16': ((0.50, 0.067), (0.10, 0.007), (0.15, 0.013)),
    'la/hot/fp16': ((0.25, 0.039), (0.05, 0.006), (0.10, 0.011)),
    'la/hot/bf16': ((0.25, 0.040), (0.05, 0.006), (0.10, 0.011)),
    'la/cold_q-12/fp16': ((0.65, 0.092), (0.10, 0.009), (0.15, 0.014)),
    'la/cold_q-12/bf16': ((0.50, 0.068), (0.10, 0.008), (0.15, 0.014)),
    'la/cold_q-14/fp16': ((4.40, 0.461), (0.10, 0.009), (0.15, 0.014)),
    'la/cold_q-14/bf16': ((0.55, 0.068), (0.10, 0.008), (0.20, 0.014)),
    'la/cold_qv-13/fp16': ((1.05, 0.113), (0.10, 0.014), (0.15, 0.013)),
    'la/cold_k-8/fp16': ((0.85, 0.093), (0.05, 0.007), (0.20, 0.014)),
    'la/cold_k-8/bf16': ((0.55, 0.071), (0.10, 0.007), (0.20, 0.014)),
    'la/cold_k-12/bf16': ((0.50, 0.070), (0.10, 0.007), (0.20, 0.013)),
    'la/few_keys+6/fp16': ((0.45, 0.040), (0.05, 0.002), (0.15, 0.004)),
    'la/few_keys+2/bf16': ((0.65, 0.040), (0.10, 0.002), (0.15, 0.004)),
    'la/few_keys-8/bf16': ((0.60, 0.040), (0.10, 0.002), (0.15, 0.004)),
    'la/wide_v/fp16': ((0.25, 0.040), (0.10, 0.005), (0.15, 0.009)),
    'la/wide_v/bf16': ((0.25, 0.040), (0.10, 0.005), (0.10, 0.009)),
    'la/sparse_v/fp16': ((0.20, 0.029), (0.05, 0.001), (0.10, 0.001)),
    'la/sparse_v/bf16': ((0.20, 0.029), (0.05, 0.001), (0.10, 0.001)),
    'la/ramp/fp16': ((0.50, 0.044), (0.50, 0.021), (0.20, 0.014)),
    'la/ramp/bf16': ((0.25, 0.036), (0.10, 0.006), (0.25, 0.015)),
    'law/control/fp16': ((1.15, 0.095), (0.40, 0.080), (0.60, 0.074)),
    'law/control/bf16': ((0.80, 0.096), (0.35, 0.083), (0.65, 0.076)),
    'law/hot/fp16': ((0.35, 0.051), (0.40, 0.087), (1.60, 0.067)),
    'law/hot/bf16': ((0.30, 0.052), (0.45, 0.085), (0.55, 0.069)),
    'law/cold_q-12/fp16': ((1.10, 0.143), (0.65, 0.134), (0.75, 0.203)),
    'law/cold_q-12/bf16': ((0.70, 0.092), (0.35, 0.083), (0.70, 0.196)),
    'law/cold_q-14/fp16': ((8.40, 0.833), (2.90, 0.833), (0.75, 0.200)),
    'law/cold_q-14/bf16': ((1.00, 0.093), (0.45, 0.079), (0.95, 0.201)),
    'law/cold_k-8/fp16': ((0.90, 0.098), (0.40, 0.082), (0.70, 0.148)),
    'law/cold_k-8/bf16': ((0.80, 0.098), (0.45, 0.077), (0.65, 0.079)),
    'law/cold_k-12/bf16': ((0.70, 0.095), (0.40, 0.083), (0.80, 0.187)),
    'law/ramp/fp16': ((0.50, 0.079), (0.50, 0.075), (0.95, 0.089)),
    'law/ramp/bf16': ((0.45, 0.069), (0.40, 0.087), (0.75, 0.090)),
    'ln/c+128/fp16': ((0.50, 0.103), (0.40, 0.067), (1.10, 0.277), (0.05, 0.005), (0.15, 0.002), (0.70, 0.352)),
    'ln/c+128/bf16': ((0.50, 0.082), (0.40, 0.067), (1.45, 0.269), (0.05, 0.003), (0.10, 0.001), (0.65, 0.370)),
    'ln/c+256/fp16': ((0.50, 0.106), (0.40, 0.066), (0.90, 0.309), (0.05, 0.005), (0.10, 0.003), (0.65, 0.372)),
    'ln/c+256/bf16': ((0.50, 0.085), (0.40, 0.070), (1.20, 0.302), (0.05, 0.003), (0.10, 0.001), (0.65, 0.368)),
    'ln/c+512/fp16': ((0.50, 0.107), (0.40, 0.071), (1.30, 0.342), (0.05, 0.005), (0.10, 0.004), (0.65, 0.419)),
    'ln/c+512/bf16': ((0.50, 0.086), (0.45, 0.069), (1.25, 0.280), (0.05, 0.003), (0.05, 0.001), (0.65, 0.331)),
    'fa/control/fp16': ((0.80, 0.104), (0.60, 0.128), (0.15, 0.011), (0.15, 0.011), (0.75, 0.117)),
    'fa/control/bf16': ((0.70, 0.104), (0.55, 0.129), (0.15, 0.011), (0.15, 0.010), (0.75, 0.116)),
    'fa/peaked/fp16': ((0.05, 0.001), (0.85, 0.370), (0.05, 0.001), (0.05, 0.001), (0.45, 0.029)),
    'fa/peaked/bf16': ((0.05, 0.001), (0.90, 0.402), (0.05, 0.001), (0.95, 0.011), (0.75, 0.068)),
    'fa/flat/fp16': ((0.30, 0.035), (0.65, 0.125), (0.05, 0.005), (0.05, 0.005), (0.30, 0.040)),
    'fa/flat/bf16': ((0.30, 0.032), (0.85, 0.123), (0.05, 0.005), (0.05, 0.005), (0.30, 0.034)),
    'fa/late_max/fp16': ((0.75, 0.129), (0.75, 0.134), (0.10, 0.014), (0.20, 0.018), (0.90, 0.136)),
    'fa/late_max/bf16': ((0.80, 0.129), (0.70, 0.132), (0.15, 0.014), (0.20, 0.018), (0.95, 0.169)),
    'fa/range/fp16': ((0.85, 0.155), (4.15, 0.329), (0.10, 0.015), (0.15, 0.014), (0.80, 0.152)),
    'fa/range/bf16': ((0.90, 0.150), (3.70, 0.295), (0.10, 0.015), (0.20, 0.019), (0.85, 0.166)),
    'fm/control/fp32': ((6.25, 0.686), (6.65, 0.699)),
    'fm/control/fp16': ((0.25, 0.037), (0.25, 0.038)),
    'fm/control/bf16': ((0.25, 0.036), (0.30, 0.036)),
    'fm/peaked/fp32': ((62.05, 2.750), (64.90, 2.029)),
    'fm/peaked/fp16': ((0.50, 0.021), (0.50, 0.015)),
    'fm/peaked/bf16': ((0.50, 0.015), (0.50, 0.012)),
    'fm/flat/fp32': ((0.70, 0.078), (0.60, 0.088)),
    'fm/flat/fp16': ((0.45, 0.011), (0.30, 0.013)),
    'fm/flat/bf16': ((0.10, 0.009), (0.10, 0.010)),
}


def rest(entry, regime, variant, st):
    return REST[f'{entry}/{key(regime, variant)}/{NAME[st]}']


def budgets(entry, regime, variant, st):
    return tuple(budget(r) for r in rest(entry, regime, variant, st))


def entries():
    out = [('la', r, v, st) for (r, v), types in LA.items() for st in types]
    out += [('law', r, v, st) for (r, v), types in LAW.items() for st in types]
    out += [('ln', 'c', C, st) for C in LN_C for st in (H16, BF16)]
    out += [('fa', r, None, st) for r in FA_REGIMES for st in (H16, BF16)]
    out += [('fm', r, None, st) for r in FM_REGIMES for st in FM_TYPES]
    return out


# ---------------------------------------------------------------------------------------------------------------------------
# full attention of the training step (k4_attention_train.hip): out, lse2, dq, dk, dv
# ---------------------------------------------------------------------------------------------------------------------------
FA_S, FA_L = (1, 31, 32, 33, 97), (37, 128, 130)      # key tiles of 32: no odd tile, a ragged odd one, four with a ragged last; query tiles: two
FA_REGIMES = ('control', 'peaked', 'flat', 'late_max', 'range')                     # waves idle, full, wave 0 with a second, ragged tile
FA_MUTATIONS = ('delta_from_unrounded_out', 'lse_natural_log', 'p_unrounded', 'odd_tiles_dropped', 'tail_keys_counted')
FA_OUT = ('out', 'lse2', 'dq', 'dk', 'dv')
LOG2E = 1.4426950408889634


def fa_shapes():
    return [(L, S) for S in FA_S for L in FA_L]


def fa_operands(regime, st, L, S):
    """q [2, L, 256] (the caller makes it a row-strided view), k, v [2, S, 256], dout [2, L, 256] in st; 4 heads of 64.
      peaked    q_l = 4 k_t(l): the target's logit leads by tens of nats; targets cycle over key 0 (an even tile), key 32 (an odd tile) and the
                last key (the ragged tail) as far as S has them
      flat      every key row is the same row: all logits of a query are equal
      late_max  a common direction w in q, growing along the keys: the largest logit lies in the last tile and every tile before it is rescaled
      range     q = d_l w, k = c_s w + noise with |w|^2 / 8 * log2(e) = 1: the exp2 arguments are d_l c_s, d_l in [-250, 250], c_s in [-1, 1]"""
    g = torch.Generator().manual_seed(R._seed('fa', regime, L, S))
    N, C = 2, 256
    q, k = torch.randn(N, L, C, generator=g) * 1.5, torch.randn(N, S, C, generator=g) * 1.5
    v, dout = torch.randn(N, S, C, generator=g), torch.randn(N, L, C, generator=g) * 0.5
    if regime == 'peaked':
        cand = torch.tensor(sorted({0, min(32, S - 1), S - 1}))
        q = 4.0 * k[:, cand[torch.arange(L) % cand.numel()]]
    elif regime == 'flat':
        k = k[:, :1].expand(N, S, C).clone()
    elif regime == 'late_max':
        w = torch.where(torch.rand(C, generator=g) < 0.5, -0.5, 0.5)
        q = q + w
        ramp = 6.0 * (torch.arange(S) + 1.0) / S + 5.0 * (torch.arange(S) >= 32 * ((S - 1) // 32))     # ... and a step into the last tile
        k = k + ramp[None, :, None] * w
    elif regime == 'range':
        w = (8.0 / LOG2E / 64) ** 0.5
        d = torch.linspace(-250.0, 250.0, L)[None, :, None] * torch.where(torch.arange(N) % 2 == 0, 1.0, -1.0)[:, None, None]
        c = 2 * torch.rand(N, S, 1, generator=g) - 1
        q = (d * w).expand(N, L, C).clone()
        k = c * w + 0.05 * torch.randn(N, S, C, generator=g)
    return tuple(t.to(st) for t in (q, k, v, dout))


def fa_reference(q, k, v, dout):
    """float64: O.full_attention and its autograd, lse2 = log2 sum exp of the scaled logits, and the per-element scales:
      out   sum_s P |v|                 lse2  1 + sum_s P (c2 sum_d |q k|): the logits' own terms, weighted as lse2 depends on them
      dS = P (dP - delta) with |dS| <= P (sum_d |dO V| + sum_s' P sum_d |dO V|):  dq  temp sum_s |dS| |k|,  dk  temp sum_l |dS| |q|,
      dv   sum_l P |dO|.
    'floor': the other operand's absolute sum where round(p), round(P), round(dS) are operands (out: sum_s |v|, dq: temp sum_s |k|,
    dk: temp sum_l |q|, dv: sum_l |dO|), which fa_errors multiplies by the floor of P: SPACING_T, and no less than fp32's smallest
    normal number 2^-126 - P comes from v_exp_f32, which has no subnormal results, so in bf16 (whose own range reaches 2^-133) that is where P ends."""
    N, L, C = q.shape
    a = [_split(t.double(), 4).clone().requires_grad_(True) for t in (q, k, v)]
    g = _split(dout.double(), 4)
    out = O.full_attention(*a)
    out.backward(g)
    qd, kd, vd = (t.detach() for t in a)
    temp = 0.125
    logits = torch.einsum('nlhd,nshd->nhls', qd, kd) * temp
    lse2 = torch.logsumexp(logits, -1) * LOG2E
    P = torch.softmax(logits, -1)
    absdP = torch.einsum('nlhd,nshd->nhls', g.abs(), vd.abs())
    absdS = P * (absdP + (P * absdP).sum(-1, keepdim=True))
    flat = lambda t: t.reshape(N, -1, C)                                          # noqa: E731
    return dict(out=(flat(out.detach()), flat(torch.einsum('nhls,nshd->nlhd', P, vd.abs()))),
                lse2=(lse2, 1 + (P * torch.einsum('nlhd,nshd->nhls', qd.abs(), kd.abs())).sum(-1) * temp * LOG2E),
                dq=(flat(a[0].grad), flat(temp * torch.einsum('nhls,nshd->nlhd', absdS, kd.abs()))),
                dk=(flat(a[1].grad), flat(temp * torch.einsum('nhls,nlhd->nshd', absdS, qd.abs()))),
                dv=(flat(a[2].grad), flat(torch.einsum('nhls,nlhd->nshd', P, g.abs()))),
                floor=dict(out=flat(vd.abs().sum(1, keepdim=True).expand(N, L, 4, 64)), dq=flat(temp * kd.abs().sum(1, keepdim=True).expand(N, L, 4, 64)),
                           dk=flat(temp * qd.abs().sum(1, keepdim=True).expand_as(kd)), dv=flat(g.abs().sum(1, keepdim=True).expand_as(vd))))


def _exp2(x):
    """exp2 as the attention kernels take it (__builtin_amdgcn_exp2f, the bare v_exp_f32): a result below fp32's normal range is zero."""
    y = _fn(torch.exp2, x)
    return torch.where(y < 2.0 ** -126, torch.zeros_like(y), y)


def fa_restated(q, k, v, dout, st, mut=None):
    """tattn_fwd, tattn_delta, tattn_bwd_dq, tattn_bwd_dkv with their rounding points; fp32 elsewhere (sums as _ein / _sum take them).
      forward   x = (q . k) c2 in log2 units (c2 = fp32(temp) * fp32(log2 e)); key tiles of 32, the even tiles in one online softmax, the odd
                tiles in another: m' = max(m, tile max), the accumulators scaled by exp2(m - m'), p = exp2(x - m'), l += p (UN-rounded),
                (every exp2 the bare v_exp_f32: no fp32 subnormals - the floor of P in fa_errors)
                o += round(p) v; the two halves merged by exp2(m_i - max); out = round(o / l), lse2 = m + log2(l)
      backward  delta = sum_d dO . out (the STORED out), P = exp2(x - lse2), dP = dO V^T, dS = P (dP - delta);
                dq = round(temp (round(dS) k)), dk = round(temp (round(dS)^T q)), dv = round(round(P)^T dO)
    Mutations: delta_from_unrounded_out (o / l before it is rounded), lse_natural_log (m + ln(l)), p_unrounded (P and p enter their second
    products in fp32), odd_tiles_dropped (the second online softmax is lost), tail_keys_counted (the zero rows that pad the last tile count
    as keys: logit 0)."""
    N, L, C = q.shape
    S = k.shape[1]
    qf, kf, vf, g = (_split(t.float(), 4) for t in (q, k, v, dout))
    c2 = torch.tensor(0.125, dtype=torch.float32) * torch.tensor(LOG2E, dtype=torch.float32)
    Sp = S
    if mut == 'tail_keys_counted' and S % 32:
        pad = 32 - S % 32
        kf, vf = (torch.cat([t, t.new_zeros(N, pad, 4, 64)], 1) for t in (kf, vf))
        Sp = S + pad
    sc = _ein('nlhd,nshd->nhls', qf, kf)
    x = sc * c2
    rp = (lambda t: t) if mut == 'p_unrounded' else (lambda t: rt(t, st))
    halves = []
    for grp in (0, 1):
        m = torch.full((N, 4, L), -math.inf)
        l = torch.zeros(N, 4, L)
        o = torch.zeros(N, 4, L, 64)
        for t0 in range(32 * grp, Sp, 64):
            xt = x[..., t0:t0 + 32]
            mn = torch.maximum(m, xt.amax(-1))
            alpha = _exp2(m - mn)
            p = _exp2(xt - mn[..., None])
            l = l * alpha + _sum(p, -1)
            o = o * alpha[..., None] + _ein('nhls,nshd->nhld', rp(p), vf[:, t0:t0 + 32])
            m = mn
        halves.append((m, l, o))
    (m0, l0, o0), (m1, l1, o1) = halves
    if mut == 'odd_tiles_dropped':
        m, l, o = m0, l0, o0
    else:
        m = torch.maximum(m0, m1)
        a0, a1 = _exp2(m0 - m), _exp2(m1 - m)
        l, o = l0 * a0 + l1 * a1, o0 * a0[..., None] + o1 * a1[..., None]
    of = o * _fn(torch.reciprocal, l)[..., None]
    out = rt(of, st)
    lse = m + _fn(torch.log if mut == 'lse_natural_log' else torch.log2, l)
    go = g.permute(0, 2, 1, 3)                                                   # [N, H, L, D]
    delta = _sum(go * (of if mut == 'delta_from_unrounded_out' else out), -1)
    P = _exp2(x - lse[..., None])
    dP = _ein('nhld,nshd->nhls', go, vf)
    dS = P * (dP - delta[..., None])
    temp = torch.tensor(0.125, dtype=torch.float32)
    dq = _ein('nhls,nshd->nlhd', rp(dS) if mut == 'p_unrounded' else rt(dS, st), kf) * temp
    dk = _ein('nhls,nlhd->nshd', rp(dS) if mut == 'p_unrounded' else rt(dS, st), qf) * temp
    dv = _ein('nhls,nhld->nshd', rp(P), go)
    flat = lambda t: t.reshape(N, -1, C)                                          # noqa: E731
    return dict(out=flat(out.permute(0, 2, 1, 3)), lse2=lse, dq=rt(flat(dq), st), dk=rt(flat(dk[:, :S]), st), dv=rt(flat(dv[:, :S]), st))


def fa_case(regime, st, L, S):
    def make():
        ops_ = fa_operands(regime, st, L, S)
        return ops_ + (fa_reference(*ops_),)
    return R._cached(('bwd_fa', regime, st, L, S), make)


def fa_errors(got, ref, st):
    return tuple(term_error(got[nm], ref[nm][0], ref[nm][1], F32 if nm == 'lse2' else st, None if nm == 'lse2' else SPACING[st] + max(SPACING[st], 2.0 ** -126) * ref['floor'][nm])
                 for nm in FA_OUT)


# ---------------------------------------------------------------------------------------------------------------------------
# fine matching (fine_match_backward): df0, df1
# ---------------------------------------------------------------------------------------------------------------------------
FM_REGIMES = ('control', 'peaked', 'flat')
FM_C = (128, 64)
FM_TYPES = (F32, H16, BF16)
FM_MUTATIONS = ('one_sided', 'no_factor_two')
FM_TEMP = 0.1


def fm_operands(regime, st, C):
    """f0, f1 [3, 25, C] in st, dconf fp32 [3, 25, 25].  peaked: f1 a permutation of f0's rows, scaled until conf is one-hot in most rows;
    flat: every row of f0 and of f1 is the same row."""
    g = torch.Generator().manual_seed(R._seed('fm', regime, C))
    M = 3
    f0, f1 = torch.randn(M, 25, C, generator=g), torch.randn(M, 25, C, generator=g)
    if regime == 'peaked':
        f0 = f0 * 3.0
        f1 = torch.stack([f0[i, torch.randperm(25, generator=g)] for i in range(M)])
        f1[:, :3] = torch.randn(M, 3, C, generator=g)                               # ... and three rows without a partner
    elif regime == 'flat':
        f0, f1 = f0[:, :1].expand(M, 25, C).clone(), f1[:, :1].expand(M, 25, C).clone()
    return f0.to(st), f1.to(st), torch.randn(M, 25, 25, generator=g)


def fm_reference(f0, f1, dconf, temperature=FM_TEMP):
    """float64 autograd of train/functional.py:dual_softmax and the scales: dsim = (2 T - A colsum(T) - B rowsum(T)) / temperature with
    T = dconf conf; |dsim| <= (2 |T| + A colsum |T| + B rowsum |T|) / temperature; df0 = dsim f1 / C: scale sum_j |dsim|_ij |f1_jc| / C."""
    from geoformer_amd.train import functional as TF
    C = f0.shape[-1]
    a, b = f0.double().clone().requires_grad_(True), f1.double().clone().requires_grad_(True)
    conf = TF.dual_softmax(a, b, temperature)
    conf.backward(dconf.double())
    sim = torch.einsum('nlc,nsc->nls', a.detach(), b.detach()) / C / temperature
    A, B = torch.softmax(sim, 1), torch.softmax(sim, 2)
    T = (dconf.double() * A * B).abs()
    ads = (2 * T + A * T.sum(1, keepdim=True) + B * T.sum(2, keepdim=True)) / temperature
    return dict(df0=(a.grad, torch.einsum('nls,nsc->nlc', ads, b.detach().abs()) / C),
                df1=(b.grad, torch.einsum('nls,nlc->nsc', ads, a.detach().abs()) / C), conf=conf.detach())


def _fma_sum(a, b, dim):
    """sum over `dim` of a * b as a loop of fp32 fused multiply-adds in index order (acc += a * b in a kernel), from 0."""
    acc = torch.zeros_like((a * b).select(dim, 0))
    for i in range(a.shape[dim] if a.shape[dim] > 1 else b.shape[dim]):
        ai = a.select(dim, i if a.shape[dim] > 1 else 0)
        bi = b.select(dim, i if b.shape[dim] > 1 else 0)
        acc = (acc.double() + ai.double() * bi.double()).float()
    return acc


def fm_restated(f0, f1, dconf, st, mut=None, temperature=FM_TEMP):
    """fine_match_backward: the header's formula in fp32 in the kernel's order - f / sqrt(C) on both sides, the product, / temperature; the two
    softmaxes from their own maxima; T = dconf A B; dsim = (2 T - A colsum(T) - B rowsum(T)) / temperature; df = round((dsim f') / sqrt(C))
    with f' the ALREADY divided rows.  Every sum is the kernel's own loop: fp32, in index order (the products fused) - in fp32 storage these
    ARE the rounding points, and where 2 T - A ct - B rt cancels their order is what the error is made of.
    one_sided: conf = B alone (dsim = T - B rowsum(T), T = dconf B); no_factor_two: T in place of 2 T."""
    C = f0.shape[-1]
    rs = torch.sqrt(torch.tensor(float(C)))
    temp = torch.tensor(temperature, dtype=torch.float32)
    one = torch.ones(1)
    s0, s1 = f0.float() / rs, f1.float() / rs
    sim = _fma_sum(s0[:, :, None, :], s1[:, None, :, :], 3) / temp
    ea, eb = _fn(torch.exp, sim - sim.amax(1, keepdim=True)), _fn(torch.exp, sim - sim.amax(2, keepdim=True))
    A = ea / _fma_sum(ea, one.view(1, 1, 1), 1).unsqueeze(1)
    B = eb / _fma_sum(eb, one.view(1, 1, 1), 2).unsqueeze(2)
    if mut == 'one_sided':
        T = dconf * B
        ds = (T - B * _fma_sum(T, one.view(1, 1, 1), 2).unsqueeze(2)) / temp
    else:
        T = dconf * A * B
        ct, rowt = _fma_sum(T, one.view(1, 1, 1), 1).unsqueeze(1), _fma_sum(T, one.view(1, 1, 1), 2).unsqueeze(2)
        ds = ((1.0 if mut == 'no_factor_two' else 2.0) * T - A * ct - B * rowt) / temp
    df0 = _fma_sum(ds[:, :, :, None], s1[:, None, :, :], 2) / rs
    df1 = _fma_sum(ds[:, :, :, None], s0[:, :, None, :], 1) / rs
    return rt(df0, st), rt(df1, st)


def fm_case(regime, st, C):
    def make():
        ops_ = fm_operands(regime, st, C)
        return ops_ + (fm_reference(*ops_),)
    return R._cached(('bwd_fm', regime, st, C), make)


def fm_errors(got, ref, st):
    return tuple(term_error(x, ref[nm][0], ref[nm][1], st) for nm, x in zip(('df0', 'df1'), got))
