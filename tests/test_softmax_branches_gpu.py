"""The rare branches of the lazily tracked softmax maxima against float64 references on every image, head, query, row and column:
K4's deferred reference (head form, fallback attn_self with one and two query blocks per wave, fp32 parity form) and K1's panel
statistics (rescale, deep tiles, subnormal column factors).  Inputs, references, tolerances and branch counters: softmax_regimes.py,
whose docstrings derive the bounds.  Each regime prints the number of decisions that took its branch and asserts a floor on it."""
import pytest
import torch

import geoformer_oracle as O
import softmax_regimes as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
C = R.K4_C

# reference matches on clear rows (softmax_regimes.k1_clear_rows) that every shape compares at thr = 0 (the inputs are fixed, so these
# counts are those of the float64 reference); the boundary regime's rows share their values by design and is a statistics check only
K1_COMPARED = {'growth': 1, 'deep': 23, 'boundary': 0, 'range': 3, 'control': 252}
# floors on the decisions (over all images, heads and queries of one call) that move the reference after tile 0 / near-threshold jumps
K4_FLOORS = {'spike': {'moves': 5000}, 'staircase': {'moves': 50000}, 'range': {'moves': 5000},
             'straddle': {'near_declined': 5000, 'near_taken': 5000}, 'tile0': {}}


def _k4_check(out, ref, bound, nkeys, what):
    """max |out - ref| / bound <= 1 and its mean <= 1/2 over the images with keys; images without keys give exact zeros."""
    out = out.double().cpu()
    for b, K in enumerate(nkeys.tolist()):
        if K == 0:
            assert float(out[b].abs().max()) == 0.0, what
    keep = nkeys.bool()
    assert torch.isfinite(out).all(), what
    r = ((out - ref).abs() / bound)[keep]
    print(f'  {what}: max {float(r.max()):.3f} mean {float(r.mean()):.4f} of the bound')
    assert float(r.max()) <= 1.0, what
    assert float(r.mean()) <= 0.5, what


def _k4_forms(q, kv, idx, nkeys, dtype):
    """(default form, fallback form): a K map whose row stride (8448 elements) is beyond the head form's descriptor field forces the
    gather pass + attn_self (two query blocks per wave once N ceil(L / 64) >= 512)."""
    from geoformer_amd import ops
    N, L, _ = q.shape
    qd, kvd, idxd, nkd = q.to(DEV), kv.to(DEV), idx.to(DEV), nkeys.to(DEV)
    head = ops.self_attention_gathered(qd, kvd[..., :C], kvd[..., C:], idxd, nkd, R.K4_H)
    huge = torch.zeros(N, L, 8192 + C, device=DEV, dtype=dtype)
    huge[..., 8192:] = kvd[..., :C]
    fb = ops.self_attention_gathered(qd, huge[..., 8192:], kvd[..., C:], idxd, nkd, R.K4_H)
    torch.cuda.synchronize()
    del huge
    return head, fb


@pytest.mark.parametrize('regime', R.K4_REGIMES)
@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_k4_deferred_reference(dtype, regime):
    """Head form and fallback (QB = 1 at L = 1200, QB = 2 at L = 3648) against float64, both bit-identical to each other; at L = 1200
    the threshold sweep: the oracle's restatement with defer = 8 and defer = 0 meets the same float64 bound, and the kernel lies
    within two ulps (one for the output rounding, one for a probability that rounds the other way) of the defer = 8 restatement at
    the scale A."""
    for L in (1200, 3648):
        N = len(R.K4_KEYS)
        assert (L == 3648) == (N * ((L + 63) // 64) >= 512)
        q, kv, idx, nkeys = R.k4_inputs(regime, dtype, L)
        ref, A, bound, floor, logits = R.k4_reference(q, kv, idx, nkeys, device=DEV)
        counts = R.k4_branch_counts(logits)
        print(f'{regime} {dtype} L={L}: {counts}')
        for k, least in K4_FLOORS[regime].items():
            assert counts[k] >= least, (k, counts[k])
        if regime == 'straddle':
            assert counts["closest"] > 1e-3
        if regime == 'tile0':
            lead = min(float(x[..., :32].amax(-1).min() - x[..., 32:].amax(-1).max()) for x in logits if x is not None and x.shape[-1] > 32)
            print(f'  tile 0 leads by {lead:.1f}')
            assert lead >= 30
        head, fb = _k4_forms(q, kv, idx, nkeys, dtype)
        _k4_check(head, ref, bound, nkeys, f'head L={L}')
        _k4_check(fb, ref, bound, nkeys, f'fallback QB={2 if L == 3648 else 1}')
        assert torch.equal(head, fb)
        if L != 1200:
            continue
        eps = R.EPS[dtype]
        for defer in (8.0, 0.0):
            flash = torch.zeros(N, L, C, dtype=torch.float64)
            for b, K in enumerate(R.K4_KEYS):
                if K == 0:
                    continue
                tok = idx[b, :K].long()
                qq = q[b].float().to(DEV).view(L, R.K4_H, R.K4_D)
                kk = kv[b, tok, :C].float().to(DEV).view(K, R.K4_H, R.K4_D)
                vv = kv[b, tok, C:].float().to(DEV).view(K, R.K4_H, R.K4_D)
                flash[b] = O._flash_self_attention(qq, kk, vv, dtype, defer=defer).reshape(L, C).double().cpu()
            _k4_check(flash, ref, bound, nkeys, f'restatement defer={defer:g}')
            if defer == 8.0:
                keep = nkeys.bool()
                d = ((head.double().cpu() - flash).abs() / (eps * torch.maximum(flash.abs(), A) + floor))[keep]
                print(f'  kernel vs restatement: max {float(d.max()):.3f} ulp, mean {float(d.mean()):.4f}')
                assert float(d.max()) <= 2.0


def test_k4_fp32_range():
    """fp32 parity form (attn_self<float>, a running maximum rescaled whenever it moves, expf) with logits over +-150 nats, where an
    unguarded exponential overflows; one and two query blocks per wave."""
    from geoformer_amd import ops
    for L in (1200, 3648):
        q, kv, idx, nkeys = R.k4_inputs('range', torch.float32, L)
        ref, A, bound, floor, logits = R.k4_reference(q, kv, idx, nkeys, device=DEV)
        span = max(float(x.abs().max()) for x in logits if x is not None)
        print(f'range fp32 L={L}: |logit| up to {span:.0f} nats')
        assert span > 120
        out = ops.self_attention_gathered(q.to(DEV), kv.to(DEV)[..., :C], kv.to(DEV)[..., C:], idx.to(DEV), nkeys.to(DEV), R.K4_H)
        _k4_check(out, ref, bound, nkeys, f'fp32 L={L}')


# ---------------------------------------------------------------------------------------------------------------------------
# K1
# ---------------------------------------------------------------------------------------------------------------------------
def _grid(n, w):
    return (n // w, w)


def _k1_run(f0, f1, thr, hw0, hw1, **kw):
    from geoformer_amd import ops
    out = ops.dual_softmax_match(f0, f1, R.K1_TEMP, thr, hw0, hw1, 8.0, **kw)
    torch.cuda.synchronize()
    M = int(out['counts'][0])
    res = {k: out[k][:M].cpu() for k in ('b_ids', 'i_ids', 'j_ids', 'mconf', 'mkpts0_c', 'mkpts1_c')}
    res['counts'] = out['counts'].cpu()
    res['conf'] = None if out['conf_matrix'] is None else out['conf_matrix'].cpu()
    return res


def _k1_conf_check(conf_k, conf64, tol, what, valid=None):
    """ln-space comparison where conf64 >= 1e-30; below it the kernel's value must be below 2e-30; no inf / NaN anywhere."""
    ck = conf_k.double()
    assert torch.isfinite(ck).all(), what
    big = conf64 >= R.TINY
    small = ~big
    if valid is not None:
        big &= valid
        small &= valid
    assert bool((ck[big] > 0).all()), f'{what}: zeros where conf >= 1e-30 ({int((ck[big] <= 0).sum())})'
    r = (ck[big].log() - conf64[big].log()).abs() / tol.expand_as(conf64)[big]
    print(f'  {what}: ln-error max {float(r.max()):.4f} of the bound over {int(big.sum())} entries; tiny entries {int(small.sum())}')
    assert float(r.max()) <= 1.0, what
    if small.any():
        assert float(ck[small].max()) < 2 * R.TINY, what


def _k1_match_check(res, conf64, thr, hw0, hw1, what, rel):
    """b / i / j ids and keypoints equal to O.coarse_match on the float64 conf on every row whose decision is clear by `rel`: row maximum
    >= 4e-30 with its runner-up `rel` below, the same for that column, and a mutual maximum `rel` away from thr (softmax_regimes.
    k1_clear_rows; rel = k1_match_rel of the confidence bound, so that no confidence within the bound decides a clear row otherwise).
    Returns the number of reference matches on clear rows that were compared (the caller asserts a floor)."""
    N, L, S = conf64.shape
    data = {'hw0_i': torch.tensor([hw0[0] * 8, hw0[1] * 8]), 'hw1_i': torch.tensor([hw1[0] * 8, hw1[1] * 8]),
            'hw0_c': torch.tensor(hw0), 'hw1_c': torch.tensor(hw1)}
    ref = O.coarse_match(conf64, data, thr)
    clear, significant = R.k1_clear_rows(conf64, thr, rel)
    kj = torch.full((N, L), -1, dtype=torch.int64)
    rj = torch.full((N, L), -1, dtype=torch.int64)
    kj[res['b_ids'], res['i_ids']] = res['j_ids']
    rj[ref['b_ids'], ref['i_ids']] = ref['j_ids']
    bad = clear & (kj != rj)
    unclear = int((significant & ~clear).sum())
    compared = int((clear & (rj >= 0)).sum())
    print(f'  {what}: {len(res["b_ids"])} matches (ref {len(ref["b_ids"])}, {compared} of them on clear rows), rows with a maximum >= '
          f'4e-30: {int(significant.sum())} of {N * L}, not clear by {rel:.3g}: {unclear}')
    assert not bool(bad.any()), f'{what}: {int(bad.sum())} clear rows disagree'
    # every kernel match on a row whose maximum is below 4e-30 has a tiny confidence
    tiny_rows = ~significant[res['b_ids'], res['i_ids']]
    assert bool((res['mconf'][tiny_rows] < 2 * R.TINY).all())
    # keypoints of every kernel match are those of its ids
    w0, w1 = hw0[1], hw1[1]
    assert torch.equal(res['mkpts0_c'], torch.stack([res['i_ids'] % w0, res['i_ids'] // w0], 1).float() * 8)
    assert torch.equal(res['mkpts1_c'], torch.stack([res['j_ids'] % w1, res['j_ids'] // w1], 1).float() * 8)
    return compared


@pytest.mark.parametrize('regime', R.K1_REGIMES)
@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_k1_panel_regimes(dtype, regime):
    """Panel form (16-bit, unmasked, L % 128 == 0, S % 64 == 0, C = 256) at three shapes, thr 0.2 (sparse candidates) and 0.0 (dense),
    contract and match-only modes, against O.dual_softmax in float64 on the rounded features."""
    from geoformer_amd import ops
    for shape in R.K1_SHAPES:
        N, L, S = shape
        assert L % R.K1_BM == 0 and S % R.K1_BN == 0
        f0, f1 = R.k1_features(regime, shape, dtype)
        x2 = R.k1_logits2(f0, f1)
        sim = R.k1_assert_regime(regime, x2)
        print(f'{regime} {dtype} {shape}: |logit| up to {float(x2.abs().max()) * R.LN2:.0f} nats; wave tiles after a run start '
              f'{sim["tiles"]}: rescales {sim["rescales"]}, deep {sim["deep"]}, non-deep unrescaled with a subnormal factor {sim["boundary"]}')
        conf64 = R.k1_conf64(f0, f1)
        tol = R.k1_log_tolerance(f0, f1, shape)
        hw0, hw1 = _grid(L, 16), _grid(S, 64)
        f0d, f1d = f0.to(DEV), f1.to(DEV)
        for thr in (0.2, 0.0):
            a = _k1_run(f0d, f1d, thr, hw0, hw1)
            _k1_conf_check(a['conf'], conf64, tol, f'conf thr={thr}')
            compared = _k1_match_check(a, conf64, thr, hw0, hw1, f'matches thr={thr}', R.k1_match_rel(tol[conf64 >= R.TINY]))
            assert compared >= (K1_COMPARED[regime] if thr == 0.0 else 0), (compared, K1_COMPARED[regime])
            b = _k1_run(f0d, f1d, thr, hw0, hw1, materialize=False)
            assert b['conf'] is None
            assert torch.equal(a['counts'], b['counts'])
            for k in ('b_ids', 'i_ids', 'j_ids', 'mconf', 'mkpts0_c', 'mkpts1_c'):
                assert torch.equal(a[k], b[k]), k
            M = len(a['b_ids'])
            if M:
                assert torch.equal(a['mconf'], a['conf'][a['b_ids'], a['i_ids'], a['j_ids']])
                got = ops.dual_softmax_conf_at(f0d, f1d, R.K1_TEMP, a['b_ids'], a['i_ids'], a['j_ids']).cpu()
                assert torch.equal(got, a['mconf'])


@pytest.mark.parametrize('form', ['fp32', 'f16_ragged', 'f16_masked'])
def test_k1_tile_form_range(form):
    """The range regime through the tile form: fp32 (exact expf), fp16 with L % 128 != 0, fp16 masked (compared on the valid block)."""
    dtype = torch.float32 if form == 'fp32' else torch.float16
    shape = (1, 500, 1344) if form == 'f16_ragged' else (2, 512, 1344)
    N, L, S = shape
    f0, f1 = R.k1_features('range', shape, dtype)
    kw, valid = {}, None
    m0 = m1 = None
    if form == 'f16_masked':
        m0 = torch.arange(L)[None].expand(N, L) < torch.tensor([480, 500])[:, None]
        m1 = torch.arange(S)[None].expand(N, S) < torch.tensor([1300, 1280])[:, None]
        kw = {'mask0': m0.to(DEV), 'mask1': m1.to(DEV)}
        valid = m0[:, :, None] & m1[:, None, :]
    conf64 = R.k1_conf64(f0, f1, m0, m1)
    tol = R.k1_log_tolerance(f0, f1, shape)
    hw0, hw1 = _grid(L, 20 if L == 500 else 16), _grid(S, 64)
    a = _k1_run(f0.to(DEV), f1.to(DEV), 0.2, hw0, hw1, **kw)
    print(f'range {form}: |logit| up to {float(R.k1_logits2(f0, f1).abs().max()) * R.LN2:.0f} nats')
    _k1_conf_check(a['conf'], conf64, tol, form, valid)
    if valid is None:
        _k1_match_check(a, conf64, 0.2, hw0, hw1, form, R.k1_match_rel(tol[conf64 >= R.TINY]))


@pytest.mark.parametrize('regime', ['growth', 'deep'])
def test_coarse_focal_loss_regimes(regime):
    """The training loss's statistics (k1_stats_panel, unmasked fp16) in the growth and deep regimes: loss and per-positive confidences
    against float64 autograd on the same rounded features to 2e-3, gradients to 2e-2 in norm (the bounds of
    test_fused_coarse_focal_loss_matches_autograd); positives are entries with float64 conf in (0.02, 0.98), one per row and column."""
    from geoformer_amd import ops
    for shape in ((1, 1280, 640), (2, 512, 1280)):                     # the loss's backward needs S % 128 == 0
        N, L, S = shape
        f0, f1 = R.k1_features(regime, shape, torch.float16)
        sim = R.k1_assert_regime(regime, R.k1_logits2(f0, f1))
        conf64 = R.k1_conf64(f0, f1)
        cand = (conf64 > 0.02) & (conf64 < 0.98)
        pb, pi, pj = torch.nonzero(cand, as_tuple=True)
        keep, ri, cj = [], set(), set()
        for t in range(len(pb)):
            key = (int(pb[t]), int(pi[t])), (int(pb[t]), int(pj[t]))
            if key[0] not in ri and key[1] not in cj:
                ri.add(key[0]); cj.add(key[1]); keep.append(t)
        pb, pi, pj = pb[keep], pi[keep], pj[keep]
        print(f'{regime} {shape}: {sim}; {len(pb)} positives')
        assert len(pb) >= 1
        a0 = f0.double().requires_grad_(True)
        a1 = f1.double().requires_grad_(True)
        simm = torch.einsum('nlc,nsc->nls', a0 / 16.0, a1 / 16.0) / R.K1_TEMP
        conf = torch.softmax(simm, 1) * torch.softmax(simm, 2)
        p = torch.clamp(conf, 1e-6, 1 - 1e-6)[pb, pi, pj]
        ref = (-0.25 * (1 - p) ** 2.0 * p.log()).sum()
        (ref * 0.37).backward()
        h0 = f0.to(DEV).clone().requires_grad_(True)
        h1 = f1.to(DEV).clone().requires_grad_(True)
        loss, pk = ops.coarse_focal_loss(h0, h1, pb.to(DEV), pi.to(DEV), pj.to(DEV), R.K1_TEMP, 0.25, 2.0)
        (loss * 0.37).backward()
        assert 0.02 < float(pk.median()) < 0.98, float(pk.median())
        torch.testing.assert_close(pk.double().cpu(), conf[pb, pi, pj].detach(), rtol=2e-3, atol=1e-7)
        torch.testing.assert_close(loss.detach().double().cpu(), ref.detach(), rtol=2e-3, atol=1e-6)
        for got, want in ((h0.grad.double().cpu(), a0.grad), (h1.grad.double().cpu(), a1.grad)):
            rel = (got - want).norm() / want.norm()
            print(f'  gradient relative error {float(rel):.2e}')
            assert rel < 2e-2, float(rel)
            assert (got - want).abs().max() < 3e-2 * want.abs().max()


@pytest.mark.parametrize('regime', ['spike', 'staircase', 'range'])
@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_k4_train_regimes(dtype, regime):
    """K4 training attention (every tile rescaled; lse kept in log2 units; two key halves merged) in the spike, staircase and range
    regimes against float64 autograd on the same 16-bit inputs: out to 3 eps max(1, max |ref|), dq / dk / dv to 4 eps in norm (the
    bounds of test_full_attention_train_forward_backward; dq relative to the norm of its absolute terms), lse to 2e-3 plus the fp32 logit error 66 u32 sum |q k| / 8 log2 e."""
    from geoformer_amd import ops
    from geoformer_amd.train import hip_autograd as HA
    eps = R.EPS[dtype]
    for N, L, S in ((1, 300, 33), (2, 130, 64), (1, 1200, 1195)):
        q, k, v = R.k4_train_inputs(regime, dtype, N, L, S)
        g = torch.Generator().manual_seed(L + S)
        dout = (torch.randn(N, L, C, generator=g) * 0.5).to(dtype)
        a = [t.double().to(DEV).requires_grad_(True) for t in (q, k, v)]
        x = torch.einsum('nlhd,nshd->nhls', a[0].view(N, L, 4, 64), a[1].view(N, S, 4, 64)) / 8.0
        ref = torch.einsum('nhls,nshd->nlhd', torch.softmax(x, -1), a[2].view(N, S, 4, 64)).reshape(N, L, C)
        ref.backward(dout.double().to(DEV))
        want_lse = (torch.logsumexp(x, -1) / R.LN2).detach()
        sabs = torch.einsum('nlhd,nshd->nhls', a[0].detach().abs().view(N, L, 4, 64), a[1].detach().abs().view(N, S, 4, 64)).amax(-1)
        moves = sum(R.k4_rule(x[n].detach().cpu() / R.LN2)[1] for n in range(N))
        print(f'{regime} {dtype} ({N}, {L}, {S}): |logit| up to {float(x.abs().max()) / R.LN2:.0f} log2 units, reference moves after tile 0 '
              f'under the deferred rule: {moves}')
        b = [t.to(DEV).clone().requires_grad_(True) for t in (q, k, v)]
        out = HA.full_attention(*b, 4)
        out.backward(dout.to(DEV))
        err = float((out.double() - ref).abs().max())
        print(f'  out error {err:.3g} (bound {3 * eps * max(1.0, float(ref.abs().max())):.3g})')
        assert err < 3 * eps * max(1.0, float(ref.abs().max()))
        # dq = sum_s P_s (dP_s - D) k_s / 8 cancels where a few large keys dominate (spike, staircase): its rounding errors scale with the
        # sum of the absolute terms, the scale A of the forward check, not with |dq|
        with torch.no_grad():
            P = torch.softmax(x, -1)
            dP = torch.einsum('nlhd,nshd->nhls', dout.double().to(DEV).view(N, L, 4, 64), a[2].view(N, S, 4, 64))
            Dl = (P * dP).sum(-1, keepdim=True)
            dq_abs = torch.einsum('nhls,nshd->nlhd', P * (dP - Dl).abs(), a[1].abs().view(N, S, 4, 64)).reshape(N, L, C) / 8.0
        for name, x_, y_ in zip(('dq', 'dk', 'dv'), b, a):
            floor = max(1e-2 * float(dout.double().norm()), float(dq_abs.norm()) if name == 'dq' else 0.0)
            rel = float((x_.grad.double() - y_.grad).norm() / y_.grad.norm().clamp_min(floor))
            print(f'  {name} relative error {rel:.3g}')
            assert rel < 4 * eps, (name, rel)
        _, lse = ops.full_attention_train_forward(q.to(DEV), k.to(DEV), v.to(DEV), 4)
        bound = 2e-3 + 66 * R.U32 * sabs / 8.0 / R.LN2
        r = float(((lse.double() - want_lse).abs() / bound).max())
        print(f'  lse error max {r:.3f} of the bound')
        assert r <= 1.0
