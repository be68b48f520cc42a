"""Inputs that force the rare branches of the two lazily tracked softmax maxima, their float64 references and the branch counters
(imported by tests/test_softmax_regimes.py and tests/test_softmax_branches_gpu.py, like tests/parity_band.py).

K4 (k4_attention.hip, 16-bit modes): a query's softmax reference m moves only when a 32-key tile's maximum exceeds it by more than
K4_DEFER = 8 log2 units (and in the first tile).  Logits here are in those units: x = q' . k with the prescaled, rounded query
q' = round_T(fp32(q) * fp32(log2(e) / 8)), exactly the operand the kernel multiplies.
K1 (k1_stats_panel, k1_stats_panel.hip): one lazily moved reference per row slot of a lane, LAZY = 64 log2 units; a lane rescales
when a tile's maximum passes its smallest reference by more than 64, and a tile is 'deep' when some column's maximum lies more than 64
below kappa, the lane's largest reference.

Everything is deterministic (seeded torch generators, no fixtures)."""
import math

import torch

U32 = 2.0 ** -24                      # fp32 unit roundoff
EPS = {torch.float16: 2.0 ** -10, torch.bfloat16: 2.0 ** -7, torch.float32: 2.0 ** -23}   # one ulp at 1.0 of each storage type
LN2 = math.log(2.0)

# ---------------------------------------------------------------------------------------------------------------------------
# K4 inference self attention
# ---------------------------------------------------------------------------------------------------------------------------
K4_C, K4_H, K4_D, K4_TILE, K4_DEFER = 256, 4, 64, 32, 8.0
# key counts of the nine images of one call: the ring's prologue (1, 31, 32, 33), main loop and tail (97, 224, 225, 1195; NS = 4,
# D = 3), ragged last tiles, and an image without keys
K4_KEYS = (1, 31, 32, 33, 97, 224, 225, 1195, 0)
K4_REGIMES = ('spike', 'staircase', 'straddle', 'tile0', 'range')
# the kernel's query scale: softmax_temp = 1 / sqrtf(64) = 0.125 (exact) times fp32(log2 e)
K4_C2 = float(torch.tensor(math.log2(math.e), dtype=torch.float32)) * 0.125


def k4_prescale(q, dtype):
    """q' = round_T(fp32(q) * fp32(c2)) as float64: the query operand of the kernel's S product (16-bit modes)."""
    return (q.float() * torch.tensor(K4_C2, dtype=torch.float32)).to(dtype).double()


def k4_spike_positions(K):
    """List positions (not tokens) of the spike keys: tile 1, a middle full tile, the last full tile before the tail, the ragged
    last tile - those that exist for K keys, tile 0 excluded, ascending."""
    nfull = K // K4_TILE
    pos = set()
    if nfull >= 2:
        pos.add(K4_TILE + 5)                                              # tile 1
    if nfull >= 3:
        pos.add(K4_TILE * (nfull // 2) + 7)                               # a middle full tile
    if nfull >= 2:
        pos.add(K4_TILE * (nfull - 1) + 11)                               # the last full tile
    if K % K4_TILE and K > K4_TILE:
        pos.add(K - 1)                                                    # the ragged last tile
    return sorted(p for p in pos if K4_TILE <= p < K)


def k4_rule(x, defer=K4_DEFER, tile=K4_TILE):
    """The kernel's deferred reference restated on float64 logits x [..., K] (log2 units, the key axis last).  Returns (m, moves, jumps):
    the final reference, the number of decisions after tile 0 that moved it, and every tile's maximum relative to the reference it
    was compared with (tiles >= 1; a tensor [..., ntiles - 1])."""
    K = x.shape[-1]
    m = None
    moves = 0
    jumps = []
    for t0 in range(0, K, tile):
        tmax = x[..., t0:t0 + tile].max(dim=-1)[0]
        if m is None:
            m = tmax
            continue
        d = tmax - m
        jumps.append(d)
        need = d > defer
        moves += int(need.sum())
        m = torch.where(need, tmax, m)
    if m is None:
        m = x.new_zeros(x.shape[:-1])
    return m, moves, (torch.stack(jumps, -1) if jumps else x.new_zeros(x.shape[:-1] + (0,)))


def k4_inputs(regime, dtype, L, seed=0):
    """One call's operands: q [9, L, 256], kv [9, L, 512] (K | V) in `dtype`, idx int32 [9, L] (ascending token lists), nkeys int32 [9].
    Channel 0 of every head is the control channel (k of it 0 unless the regime sets it); the other 63 are unit normal noise.
      spike     chosen queries (every third) meet keys at k4_spike_positions whose logits climb 9 to 40 above everything before them
      staircase key control values grow with the list position: the reference moves in consecutive tiles (every tile for the
                steepest queries, every second or third for the others)
      straddle  one key per image in a middle tile lands 7.9 (declined) or 8.1 (taken) above the query's reference at that point
      tile0     tile 0 leads every other key by 30 or more (the later probabilities underflow in fp16)
      range     q, k scaled by 6.5: logits spread over about +-240 nats (an unguarded exp overflows beyond 88)"""
    assert regime in K4_REGIMES
    g = torch.Generator().manual_seed(1000 * K4_REGIMES.index(regime) + seed + L)
    N, C, H, D = len(K4_KEYS), K4_C, K4_H, K4_D
    q = torch.randn(N, L, C, generator=g)
    kmap = torch.randn(N, L, C, generator=g)
    vmap = torch.randn(N, L, C, generator=g)
    idx = torch.zeros(N, L, dtype=torch.int32)
    for b, K in enumerate(K4_KEYS):
        idx[b, :K] = torch.sort(torch.randperm(L, generator=g)[:K])[0].int()
    ctl = torch.arange(H) * D                                             # the control channel of each head
    if regime == 'range':
        q *= 6.5
        kmap *= 6.5
    else:
        q[:, :, ctl] = 0.
        kmap[:, :, ctl] = 0.
    lq = torch.arange(L, dtype=torch.float64)
    frac = torch.remainder(lq * 0.6180339887, 1.0)                        # a per-query spread in [0, 1)
    for b, K in enumerate(K4_KEYS):
        if K == 0:
            continue
        tok = idx[b, :K].long()
        if regime == 'spike':
            chosen = (torch.arange(L) % 3) == 0
            tau = 0.6 + frac                                               # the chosen queries' slope, 0.6 .. 1.6
            for n, p in enumerate(k4_spike_positions(K)):
                kmap[b, tok[p], ctl] = (16.0 + 24.0 * n) / K4_C2          # logit tau * (16, 40, 64, 88)
            for hh in range(H):
                q[b, :, ctl[hh]] = torch.where(chosen, tau * (1.0 + 0.05 * hh), torch.zeros(L, dtype=torch.float64)).float()
        elif regime == 'staircase':
            pos = torch.arange(K, dtype=torch.float32)
            for hh in range(H):
                kmap[b, tok, ctl[hh]] = 0.5 * pos
                q[b, :, ctl[hh]] = (4.5 * frac * (1.0 - 0.1 * hh)).float()   # rise per tile up to c2 * 4.5 * 16 = 13 log2
        elif regime == 'tile0':
            first = tok[:min(K, K4_TILE)]
            kmap[b, first[:, None], ctl[None, :]] = 44.0 / K4_C2 + 2.0 * torch.rand(len(first), H, generator=g)
            for hh in range(H):
                q[b, :, ctl[hh]] = (1.0 + 0.6 * frac).float()              # tile 0 at 44 .. 72 log2, the rest about N(0, 1.4^2)
    if regime == 'straddle':
        # the query control value is set after the rest: the target is relative to the reference the rule holds at the straddle tile
        for b, K in enumerate(K4_KEYS):
            ntiles = (K + K4_TILE - 1) // K4_TILE
            if ntiles < 2:
                continue
            tok = idx[b, :K].long()
            ts = max(1, ntiles // 2)
            p = ts * K4_TILE + 3 if ts * K4_TILE + 3 < K else K - 1
            kmap[b, tok[p], ctl] = 1.0
            qq = k4_prescale(q[b].to(dtype).float(), dtype).view(L, H, D)
            kk = kmap[b, tok].to(dtype).double().view(K, H, D)
            x = torch.einsum('lhd,khd->hlk', qq, kk)                         # control channel of q is still 0 here
            m, _, _ = k4_rule(x[..., :ts * K4_TILE])
            want = torch.where(torch.arange(L) % 2 == 0, 7.9, 8.1).double()
            rest = x[..., p]                                                 # the key's logit without the control channel
            for hh in range(H):
                target = m[hh] + want - rest[hh]                              # q'_0 * 1.0 must equal this
                q[b, :, ctl[hh]] = (target / K4_C2).float()
    kv = torch.cat([kmap, vmap], -1).to(dtype)
    return q.to(dtype), kv, idx, torch.tensor(K4_KEYS, dtype=torch.int32)


def k4_train_inputs(regime, dtype, N, L, S, seed=0):
    """q [N, L, 256], k, v [N, S, 256] in `dtype` for the training attention (keys in their natural order, no token list), with the
    control channel of k4_inputs: spike keys at k4_spike_positions(S) met by every third query, the staircase k = 0.5 * position, or
    q, k scaled by 6.5 (range)."""
    assert regime in ('spike', 'staircase', 'range')
    g = torch.Generator().manual_seed(77 * K4_REGIMES.index(regime) + 7 * L + S + seed)
    C, H, D = K4_C, K4_H, K4_D
    q = torch.randn(N, L, C, generator=g)
    k = torch.randn(N, S, C, generator=g)
    v = torch.randn(N, S, C, generator=g)
    ctl = torch.arange(H) * D
    frac = torch.remainder(torch.arange(L, dtype=torch.float64) * 0.6180339887, 1.0)
    if regime == 'range':
        q *= 6.5
        k *= 6.5
    else:
        q[:, :, ctl] = 0.
        k[:, :, ctl] = 0.
    if regime == 'spike':
        for n, p in enumerate(k4_spike_positions(S)):
            k[:, p, ctl] = (16.0 + 24.0 * n) / K4_C2
        chosen = (torch.arange(L) % 3) == 0
        for hh in range(H):
            q[:, :, ctl[hh]] = torch.where(chosen, (0.6 + frac) * (1.0 + 0.05 * hh), torch.zeros(L, dtype=torch.float64)).float()
    elif regime == 'staircase':
        for hh in range(H):
            k[:, :, ctl[hh]] = 0.5 * torch.arange(S, dtype=torch.float32)
            q[:, :, ctl[hh]] = (4.5 * frac * (1.0 - 0.1 * hh)).float()
    return q.to(dtype), k.to(dtype), v.to(dtype)


def k4_reference(q, kv, idx, nkeys, device='cpu'):
    """Float64 attention of every image, head and query on exactly the kernel's operands -> (out [N, L, 256], A [N, L, 256], the error
    bound [N, L, 256] of _k4_bound, its subnormal floor [N, L, 256], logits per image [H, L, K]).  16-bit modes: logits x = q' . k (log2
    units, q' = k4_prescale);
    fp32: x = q . k / 8 in nats.  A = sum p |v| / sum p, the scale of the terms the kernel sums (>= |out|).  delta bounds the
    kernel's fp32 error of one logit: 66 u32 (max_k sum_d |q'_d k_d| + max_k |x|) - the S chain adds 64 products to -m' (16-bit),
    or 64 products, one scale and one subtraction (fp32)."""
    dtype = q.dtype
    N, L, C = q.shape
    H, D = K4_H, K4_D
    f32 = dtype == torch.float32
    out = torch.zeros(N, L, C, dtype=torch.float64)
    A = torch.zeros(N, L, C, dtype=torch.float64)
    delta = torch.zeros(N, L, H, dtype=torch.float64)
    vsum = torch.zeros(N, 1, C, dtype=torch.float64)
    logits = []
    for b in range(N):
        K = int(nkeys[b])
        if K == 0:
            logits.append(None)
            continue
        vsum[b, 0] = kv[b, idx[b, :K].long(), C:].double().abs().sum(0)
        tok = idx[b, :K].long()
        qq = (q[b].double() if f32 else k4_prescale(q[b], dtype)).to(device).view(L, H, D)
        kk = kv[b, tok, :C].double().to(device).view(K, H, D)
        vv = kv[b, tok, C:].double().to(device).view(K, H, D)
        x = torch.einsum('lhd,khd->hlk', qq, kk)
        sabs = torch.einsum('lhd,khd->hlk', qq.abs(), kk.abs()).amax(-1)
        if f32:
            x = x / 8.0
            sabs = sabs / 8.0
        mx = x.amax(-1, keepdim=True)
        p = torch.exp(x - mx) if f32 else torch.exp2(x - mx)
        l = p.sum(-1, keepdim=True)
        o = torch.einsum('hlk,khd->lhd', p / l, vv)
        a = torch.einsum('hlk,khd->lhd', p / l, vv.abs())
        out[b] = o.reshape(L, C).cpu()
        A[b] = a.reshape(L, C).cpu()
        delta[b] = (66 * U32 * (sabs + x.abs().amax(-1))).T.cpu()
        logits.append(x.cpu())
    floor = SUB[dtype] / 2 * vsum.expand(N, L, C)
    return out, A, _k4_bound(dtype, nkeys, delta, A, floor), floor, logits


# half the spacing of the subnormal numbers of each storage type: the absolute rounding error of a probability below the normal range
SUB = {torch.float16: 2.0 ** -24, torch.bfloat16: 2.0 ** -133, torch.float32: 0.0}


def _k4_bound(dtype, nkeys, delta, A, floor):
    """Per-element bound on |kernel - ref| in units of the output, with A = sum p |v| / sum p >= |ref| the stated floor of the scale.
    16-bit modes: the probabilities are rounded to T for the P.V product (<= u_T p each, or half the subnormal spacing below T's
    normal range: the largest probability is >= 1, so sum p >= 1 and those add up to <= SUB / 2 sum_k |v_k| = `floor`) and the output
    is rounded once (<= u_T |ref| <= u_T A): together one ulp of T (EPS = 2 u_T) at the scale A, plus the floor.  fp32 (nothing rounded
    to storage): one ulp of fp32.  Both: fp32 sums of K products and K probabilities (<= (K + 4) u32 A), and the logit error delta,
    which moves every probability by a factor 2^(+-delta) (e^(+-delta) for the fp32 form's nats) in numerator and denominator
    (<= 2 ln2 delta A).  A wrong rescale of the deferred reference weighs old keys by 2^8 to 2^64 too much (or too little): errors of
    order A, hundreds of ulps."""
    lam = 1.0 if dtype == torch.float32 else LN2
    K = nkeys.double().view(-1, 1, 1)
    per = EPS[dtype] + (K + 4) * U32 + 2 * lam * delta                     # [N, L, H]
    return per.repeat_interleave(K4_D, dim=-1) * A + floor


def k4_branch_counts(logits, defer=K4_DEFER):
    """Decisions after tile 0 that move the reference, over all images, heads and queries; and the straddle counts: decisions whose
    jump lies in (defer - 0.2, defer - 0.01) (declined) and (defer + 0.01, defer + 0.2) (taken), and the smallest |jump - defer|."""
    moves, near_dec, near_take, closest = 0, 0, 0, float('inf')
    for x in logits:
        if x is None:
            continue
        _, mv, j = k4_rule(x, defer)
        moves += mv
        if j.numel():
            near_dec += int(((j > defer - 0.2) & (j < defer - 0.01)).sum())
            near_take += int(((j > defer + 0.01) & (j < defer + 0.2)).sum())
            closest = min(closest, float((j - defer).abs().min()))
    return {'moves': moves, 'near_declined': near_dec, 'near_taken': near_take, 'closest': closest}


# ---------------------------------------------------------------------------------------------------------------------------
# K1 dual softmax (panel form) and the coarse loss
# ---------------------------------------------------------------------------------------------------------------------------
K1_C, K1_TEMP, K1_BN, K1_BM, K1_RUN, K1_LAZY = 256, 0.1, 64, 128, 10, 64.0
K1_MULT2 = 1.0 / (K1_C * K1_TEMP) / LN2                                  # raw dot product -> log2 units
K1_REGIMES = ('growth', 'deep', 'boundary', 'range', 'control')
K1_SHAPES = ((2, 512, 1344), (1, 1280, 640), (1, 256, 6400))
TINY = 1e-30


def _k1_rank_one(N, L, S, beta, gamma, g, noise=0.3, planted=1.0, beta2=None, gamma2=None):
    """f0_i = beta_i e + beta2_i e2 + n_i, f1_j = gamma_j e + gamma2_j e2 + n'_j.  e and e2 are orthogonal directions of norm sqrt(C) on
    channels 0 .. 127 (e = sqrt 2 there, e2 = +-sqrt 2), so sim_ij = 10 (beta_i gamma_j + beta2_i gamma2_j) nats (14.4 ... in log2
    units); the noise n lives on channels 128 .. 255, where the values stay small and keep their 16-bit resolution: it makes every
    pair's logit distinct (about noise^2 * 0.64 log2 units) instead of being rounded away on the large rank-one channels.  Planted
    pairs (i, pi(i)) share a component on the noise channels, worth 7.2 planted^2 log2 units."""
    C, H = K1_C, K1_C // 2
    r2 = math.sqrt(2.0)
    e = torch.cat([torch.full((H,), r2), torch.zeros(H)])
    e2 = torch.cat([torch.full((H // 2,), r2), torch.full((H // 2,), -r2), torch.zeros(H)])
    pad = lambda t: torch.cat([torch.zeros(t.shape[:-1] + (H,)), t], -1)                     # noqa: E731
    f0 = beta[..., None] * e + noise * pad(torch.randn(N, L, H, generator=g))
    f1 = gamma[..., None] * e + noise * pad(torch.randn(N, S, H, generator=g))
    if beta2 is not None:
        f0 += beta2[..., None] * e2
        f1 += gamma2[..., None] * e2
    if planted:
        k = min(L, S) // 2
        for b in range(N):
            u = pad(torch.randn(k, H, generator=g))
            pi = torch.randperm(L, generator=g)[:k]
            pj = torch.randperm(S, generator=g)[:k]
            f0[b, pi] += planted * u
            f1[b, pj] += planted * u
    return f0, f1


# boundary regime: per 32-row block the odd rows' reference offset below kappa (cycled), and per tile of a run the offset of the column
# maxima below kappa - tile 0 sets the references, tiles 1 .. 5 are deep (c > 64, no rescale), tiles 6 .. 9 are the window
# c in [r - 64, 64) in which, for r > 126, exp2(ref - kappa) is subnormal while the tile is neither deep nor rescaled
K1_BOUNDARY_R = (120.0, 124.0, 126.4, 126.6, 126.8)
K1_BOUNDARY_C = (0.0, 68.0, 67.0, 66.0, 65.0, 64.5, 63.6, 63.4, 63.2, 63.0)


def k1_features(regime, shape, dtype, seed=0):
    """(f0 [N, L, 256], f1 [N, S, 256]) in `dtype` for one regime:
      growth    beta in [1, 1.5]; gamma rises by 6 per 64-column tile inside each 640-column run: every row's logits in a tile lie
                more than 64 log2 units above everything before them in the run
      deep      strong (even) and weak (odd) rows alternate; the first half of each run's tiles has gamma > 0 (the strong rows set
                kappa), the second half gamma < 0, whose column maxima come from the weak rows, > 150 below kappa
      boundary  tile 0 of each run puts the even rows at kappa ~ 144 and the odd rows K1_BOUNDARY_R below it (one value per 32-row
                block); tile t = 1 .. 9 puts the odd rows K1_BOUNDARY_C[t] below kappa, the even rows near 0: deep tiles first, then
                the narrow window of non-deep tiles without a rescale in which exp2(ref - kappa) is subnormal (k1_panel_sim counts it)
      range     beta, gamma in [-4.4, 4.4]: |logits| up to about 200 nats
      control   the planted features of tests/test_k1_dual_softmax_gpu.py (scale 1.3, noise 0.35)"""
    N, L, S = shape
    g = torch.Generator().manual_seed(7919 * K1_REGIMES.index(regime) + 31 * L + S + seed)
    jj = torch.arange(S)
    tile_in_run = (jj // K1_BN) % K1_RUN
    col = (jj % K1_BN).double()
    ii = torch.arange(L)
    if regime == 'control':
        f0 = torch.randn(N, L, K1_C, generator=g) * 1.3
        f1 = torch.randn(N, S, K1_C, generator=g) * 1.3
        k = min(L, S) * 2 // 3
        for b in range(N):
            pi = torch.randperm(L, generator=g)[:k]
            pj = torch.randperm(S, generator=g)[:k]
            f1[b, pj] = f0[b, pi] + 0.35 * 1.3 * torch.randn(k, K1_C, generator=g)
    elif regime == 'growth':
        beta = (1.0 + 0.5 * torch.rand(N, L, generator=g)).double()
        gamma = (-27.0 + 6.0 * tile_in_run + 0.3 * col / 63).double().expand(N, S) + 0.002 * torch.randn(N, S, generator=g).double()
        f0, f1 = _k1_rank_one(N, L, S, beta.float(), gamma.float(), g)
    elif regime == 'deep':
        strong = (ii % 2 == 0)
        beta = torch.where(strong, 1.0 + 0.2 * torch.rand(N, L, generator=g), 0.2 + 0.1 * torch.rand(N, L, generator=g))
        sign = torch.where(tile_in_run < K1_RUN // 2, 1.0, -1.0)
        gamma = sign * (10.0 + 2.0 * torch.rand(N, S, generator=g))
        f0, f1 = _k1_rank_one(N, L, S, beta, gamma, g)
    elif regime == 'boundary':
        s = 1.0 / (K1_MULT2 * K1_C)                                     # 1 / 14.43: log2 units -> coefficient products
        kappa = 144.0
        r = torch.tensor(K1_BOUNDARY_R, dtype=torch.float64)[(ii // 32) % len(K1_BOUNDARY_R)]
        c = torch.tensor(K1_BOUNDARY_C, dtype=torch.float64)[tile_in_run]
        even = (ii % 2 == 0)
        beta = torch.where(even, torch.ones(L, dtype=torch.float64), 1.0 - r / kappa).expand(N, L)
        beta2 = torch.where(even, torch.zeros(L, dtype=torch.float64), torch.ones(L, dtype=torch.float64)).expand(N, L)
        ramp = 0.002 * col / 63
        gamma = torch.where(tile_in_run == 0, kappa * s + ramp, 0 * ramp).expand(N, S)
        gamma2 = torch.where(tile_in_run == 0, 0 * ramp, (kappa - c) * s - ramp).expand(N, S)
        f0, f1 = _k1_rank_one(N, L, S, beta.float(), gamma.float(), g, noise=0.1, planted=0, beta2=beta2.float(), gamma2=gamma2.float())
    elif regime == 'range':
        beta = 8.8 * torch.rand(N, L, generator=g) - 4.4
        gamma = 8.8 * torch.rand(N, S, generator=g) - 4.4
        f0, f1 = _k1_rank_one(N, L, S, beta, gamma, g)
    else:
        raise KeyError(regime)
    return f0.to(dtype), f1.to(dtype)


def k1_logits2(f0, f1):
    """float64 logits in log2 units on the rounded features: sim / ln 2, sim = f0 . f1 / C / temperature."""
    return torch.einsum('nlc,nsc->nls', f0.double(), f1.double()) * K1_MULT2


def k1_growth_margin(x2, bn=K1_BN, run=K1_RUN):
    """min over rows and non-first tiles of a run of (min of the row's logits in the tile - max of its logits in the run's earlier
    tiles): > 64 means every lane rescales at every tile whatever the register layout."""
    N, L, S = x2.shape
    nt = S // bn
    t = x2.view(N, L, nt, bn)
    tmin, tmax = t.amin(-1), t.amax(-1)
    worst = float('inf')
    for t0 in range(0, nt, run):
        for tt in range(t0 + 1, min(t0 + run, nt)):
            worst = min(worst, float((tmin[..., tt] - tmax[..., t0:tt].amax(-1)).min()))
    return worst


_ACC_ROWS = torch.tensor([[(r & 3) + 8 * (r >> 2) + 4 * h for r in range(16)] for h in range(2)])   # gf_acc_row(r, h)


def k1_panel_sim(x2, bn=K1_BN, run=K1_RUN, lazy=K1_LAZY):
    """k1_stats_panel's decisions stepped through every run of every 32-row wave block on float64 logits x2 [N, L, S] (log2 units).
    Lane (h, lr) holds the 16 row slots gf_acc_row(r, h) and the columns lr, 32 + lr of each 64-column tile; per slot a running
    maximum rmx and a reference ref, per lane minref = min ref and kappa = max ref.  Per tile, wave-wide (__any over the lanes):
      rescale  some lane's tile maximum exceeds its minref by more than LAZY -> every lane: ref = rmx (including this tile)
      deep     some lane has kappa - min(its two column maxima over the wave's 32 rows) > LAZY
    and the boundary event: a tile after the run's first that is neither deep nor rescaled, in which a slot with ref - kappa < -126
    (exp2(ref - kappa) subnormal) holds, in the lane's column, a logit within 24 log2 units of that column's maximum (a term an fp32
    column sum registers).  Returns counts over the non-first tiles of the runs: (wave tiles, rescales, deep tiles, boundary events)."""
    N, L, S = x2.shape
    nt, B = S // bn, L // 32
    X = x2.view(N, B, 32, nt, 2, 32)[:, :, _ACC_ROWS]                     # [N, B, h, r, nt, ni, lr]
    X = X.permute(0, 1, 2, 6, 3, 4, 5)                                    # [N, B, h, lr, r, nt, ni]
    tiles = resc_n = deep_n = events = 0
    for t0 in range(0, nt, run):
        rmx = torch.full(X.shape[:5], -math.inf, dtype=x2.dtype)
        ref = rmx.clone()
        minref = torch.full(X.shape[:4], -math.inf, dtype=x2.dtype)
        kappa = minref.clone()
        for t in range(t0, min(t0 + run, nt)):
            a = X[..., t, :]                                               # [N, B, h, lr, r, 2]
            rmx = torch.maximum(rmx, a.amax(-1))
            resc = (a.amax((-1, -2)) - minref > lazy).flatten(2).any(-1)   # [N, B]
            w = resc[:, :, None, None]
            ref = torch.where(w[..., None], rmx, ref)
            minref = torch.where(w, ref.amin(-1), minref)
            kappa = torch.where(w, ref.amax(-1), kappa)
            cmax = a.amax((2, 4))                                          # [N, B, lr, 2] over the wave's 32 rows
            deep = (kappa - cmax.amin(-1)[:, :, None] > lazy).flatten(2).any(-1)
            sub = (ref - kappa[..., None] < -126)[..., None]               # [N, B, h, lr, r, 1]
            near = a >= cmax[:, :, None, :, None, :] - 24
            ev = (sub & near).flatten(2).any(-1) & ~deep & ~resc
            if t > t0:
                tiles += N * B
                resc_n += int(resc.sum())
                deep_n += int(deep.sum())
                events += int(ev.sum())
    return {'tiles': tiles, 'rescales': resc_n, 'deep': deep_n, 'boundary': events}


def k1_conf64(f0, f1, mask0=None, mask1=None):
    """O.dual_softmax in float64 on the rounded features."""
    import geoformer_oracle as O
    m0 = None if mask0 is None else mask0.bool()
    m1 = None if mask1 is None else mask1.bool()
    return O.dual_softmax(f0.double(), f1.double(), K1_TEMP, m0, m1)


def k1_log_tolerance(f0, f1, conf_shape):
    """Bound on |ln conf_k - ln conf_ref| per element (nats), from fp32 arithmetic on the rounded features:
    * each logit is an fp32 sum of C = 256 products: |error| <= dl = 257 u32 sum_c |f0_c f1_c| * mult2 (log2 units; taken as the max
      over the row and over the column);
    * ln conf = ln2 (2 x - rmax - cmax) - ln rsum - ln csum: four logits (2 + 1 + 1 dl) and the two sums, whose terms carry two
      logit errors each (2 + 2 dl) -> 8 ln2 dl;
    * forming the exponent's argument in fp32 (products by log2 e, two adds, one fma): <= 4 u32 (2 |x| + |rmax| + |cmax|) log2 units;
    * the two sums of up to max(L, S) terms and their partial combinations in fp32, hardware exp2: <= 2 (max(L, S) + 64) u32.
    A skipped rescale or a wrong column path is off by a factor 2^64 or more: 44 nats."""
    a0, a1 = f0.double().abs(), f1.double().abs()
    sab = torch.einsum('nlc,nsc->nls', a0, a1) * K1_MULT2
    dl = 257 * U32 * torch.maximum(sab.amax(2, keepdim=True), sab.amax(1, keepdim=True))
    x2 = k1_logits2(f0, f1)
    arg = 2 * x2.abs() + x2.amax(2, keepdim=True).abs() + x2.amax(1, keepdim=True).abs()
    N, L, S = conf_shape
    return LN2 * (8 * dl + 4 * U32 * arg) + 2 * (max(L, S) + 64) * U32


def k1_assert_regime(regime, x2):
    """The branch counts k1_panel_sim finds on the float64 logits, with the floor each regime promises; returns the counts."""
    sim = k1_panel_sim(x2)
    if regime == 'growth':
        assert k1_growth_margin(x2) > K1_LAZY and sim['rescales'] == sim['tiles'] > 0, sim        # every wave, every tile after a run start
    elif regime == 'deep':
        assert 9 * sim['deep'] >= 5 * sim['tiles'] > 0, sim                                     # the five gamma < 0 tiles of every run
    elif regime == 'boundary':
        assert sim['rescales'] == 0 and sim['boundary'] >= 90, sim
    return sim


def k1_match_rel(tol):
    """The relative margin a match decision needs to be decided alike by any confidence within the ln bound `tol` of conf (both
    entries of a comparison may move by tol): expm1(2 max tol), and at least 1e-4."""
    return max(1e-4, math.expm1(2 * float(tol.max())))


def k1_clear_rows(conf, thr, rel=1e-4, tiny=TINY):
    """(clear, significant) [N, L] for coarse_match on the float64 `conf`: a row is significant when its maximum is >= 4 tiny (the
    kernel resolves it: its error there is far below rel), and clear when moreover its runner-up lies `rel` below the maximum, the
    maximum's column has its runner-up `rel` below its own maximum, and (thr > 0) the maximum is `rel` away from thr.  A clear row's
    match decision is the same for any confidence within rel of conf.  Rows below 4 tiny hold only values the kernel keeps tiny,
    possibly zero (at thr = 0 a mutual maximum among them is no comparable decision)."""
    top2r = conf.topk(2, dim=2)
    top2c = conf.topk(2, dim=1)[0]
    jbest = top2r.indices[..., 0]
    rmax, r2 = top2r.values[..., 0], top2r.values[..., 1]
    cgap = 1 - top2c[:, 1] / top2c[:, 0]
    significant = rmax >= 4 * tiny
    clear = significant & (1 - r2 / rmax >= rel) & (torch.gather(cgap, 1, jbest) >= rel)
    if thr > 0:
        clear &= (rmax - thr).abs() >= rel * torch.clamp(rmax, min=thr)
    return clear, significant
