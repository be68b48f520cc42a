"""K8 forward (ops.fine_match: fine_match or fine_match_mfma, then fine_count and fine_compact) against float64 on every match of every regime
of fine_match_regimes.py, whose docstrings derive the bound: confidences within the bound (max <= 1, mean <= 1/2 of it), decisions (arg-max with
the first-index rule, threshold) equal to the reference's on ALL matches (tests/test_fine_match_regimes.py shows every one of them clear),
ordered compaction across 1024-match chunks, and the keypoint arithmetic to its own four-rounding budget.

Forms: 16-bit storage runs the MFMA kernel (C % 16 == 0, 16-byte aligned windows) and the scalar fallback - reached by C = 72 and, for every
16-bit input, by a contiguous copy that starts 8 bytes past a 16-byte boundary; fp32 storage runs the scalar kernel.  Both forms of an input are
compared against float64 and must agree in every decision and compacted keypoint.

Observed on an MI355X, error / bound as (max, mean) over the regime's types and channel counts at their worst:
  regime                 MFMA kernel (max, mean)   scalar kernel (max, mean)
  control                0.021  0.0032             0.030  0.0039
  control, M = 1 .. 5    0.017  0.0038             0.028  0.0047
  range                  0.023  0.0051             0.074  0.0139
  underflow              0.012  0.0010             0.021  0.0013
  straddle               0.009  0.0017             0.014  0.0023
  ties                   0.020  0.0019             0.036  0.0023
  nonfinite              0.021  0.0032             0.030  0.0040
  compaction cases       0.009  0.0011             0.032  0.0043
keypoints: at most 0.50 of their budget.  The bound is a worst case over C + 6 roundings per logit; the kernels' errors behave like a few of them.
What the bound does not see, the decisions do: before its contraction pragma, fine_match_mfma formed exp2's argument as fma(acc, scale2, -max),
half an ulp of the logit off at the maximum itself (0.02 of the bound) - confidences up to 1.00002, found by the saturated ties (d)."""
import pytest
import torch

import fine_match_regimes as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = [(regime, dtype) for regime in R.REGIMES for dtype in R.TYPES]


def _place(t, form):
    """The window tensor on the device: 'aligned' as the allocator returns it, 'shifted' a contiguous view 4 elements (8 bytes) into a flat
    buffer - no 16-byte pieces can be read from it, so 16-bit storage takes the scalar kernel."""
    if form == 'aligned':
        d = t.to(DEV)
        assert d.data_ptr() % 16 == 0
        return d
    assert t.element_size() == 2
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=DEV)
    d = buf[4:4 + t.numel()].view(t.shape)
    d.copy_(t)
    assert d.is_contiguous() and d.data_ptr() % 16 == 8
    return d


def _forms(dtype):
    return ('aligned',) if dtype == R.F32 else ('aligned', 'shifted')


def _run(f0, f1, thr, form, b_ids=None, mk0=None, mk1=None, scale0=None, scale1=None):
    """One call -> outputs on the CPU, the compacted ones cut to count.  Without keypoint inputs: b_ids = the match index and zero coarse
    keypoints, so that m_bids names the accepted matches and the fine keypoints are the cell offsets times two."""
    from geoformer_amd import ops
    M = f0.shape[0]
    b_ids = torch.arange(M) if b_ids is None else b_ids
    mk0 = torch.zeros(M, 2) if mk0 is None else mk0
    mk1 = torch.zeros(M, 2) if mk1 is None else mk1
    kw = {} if scale0 is None else {'scale0': scale0.to(DEV), 'scale1': scale1.to(DEV)}
    out = ops.fine_match(_place(f0, form), _place(f1, form), R.TEMP, thr, b_ids.to(DEV), mk0.to(DEV), mk1.to(DEV), R.COARSE_SCALE,
                         R.C2F_SCALE, R.FINE_SCALE, **kw)
    torch.cuda.synchronize()
    n = int(out['count'][0])
    assert 0 <= n <= M
    res = {k: out[k][:n].cpu() for k in ('mkpts0_f', 'mkpts1_f', 'mconf', 'm_bids')}
    res['fine_matrix'], res['count'] = out['fine_matrix'].cpu(), n
    return res


def _same_bits(a, b, what):
    assert a['count'] == b['count'], what
    for k in ('fine_matrix', 'mkpts0_f', 'mkpts1_f', 'mconf', 'm_bids'):
        x, y = a[k], b[k]
        if x.dtype == torch.float32:
            x, y = x.view(torch.int32), y.view(torch.int32)
        assert torch.equal(x, y), (what, k)


def _kernel_sel(res, M):
    """The kernel's decision per match from a _run without keypoint inputs: -1 or the flat cell index."""
    sel = torch.full((M,), -1, dtype=torch.int64)
    cell = lambda mk: (mk[:, 1] / 2 + 2).long() * R.W + (mk[:, 0] / 2 + 2).long()      # noqa: E731
    assert torch.equal(res['m_bids'], torch.sort(res['m_bids'])[0]) and len(torch.unique(res['m_bids'])) == res['count']
    sel[res['m_bids']] = cell(res['mkpts0_f']) * R.WW + cell(res['mkpts1_f'])
    return sel


def _conf_check(res, c, what, rows=None):
    """fine_matrix within the bound on the finite windows (`rows`: those to compare), mconf the bits of its cell."""
    ref, tol = c['ref'], c['tol']
    rows = torch.nonzero(~torch.isnan(ref['conf'].flatten(1)).any(1))[:, 0] if rows is None else rows
    got = res['fine_matrix'][rows]
    assert torch.isfinite(got).all() and float(got.max()) <= 1.0 and float(got.min()) >= 0.0, what      # a product of two probabilities
    r = R.conf_error(got, ref['conf'][rows], tol[rows])
    mx, mean = R.report(what, r)
    assert mx <= 1.0 and mean <= 0.5, (what, mx, mean)
    return mx, mean


def _check_regime(c, res, what):
    M = c['f0'].shape[0]
    ref = c['ref']
    _conf_check(res, c, what)
    sel = _kernel_sel(res, M)
    assert torch.equal(sel, ref['sel']), (what, torch.nonzero(sel != ref['sel'])[:, 0].tolist()[:10])
    assert res['count'] == int(ref['ok'].sum())
    assert torch.equal(res['m_bids'], torch.nonzero(ref['ok'])[:, 0])
    assert torch.equal(res['mconf'].view(torch.int32), res['fine_matrix'].flatten(1)[res['m_bids'], ref['sel'][res['m_bids']]].view(torch.int32))


@pytest.mark.parametrize('regime,dtype', CASES, ids=str)
def test_fine_match_regimes(regime, dtype):
    """Every regime, type and channel count at M = 67 (17 MFMA workgroups, the last ragged; two ballots), each 16-bit input through both forms."""
    for C in R.regime_cs(regime, dtype):
        c = R.case(regime, dtype, C)
        results = []
        for form in _forms(dtype):
            what = f'{regime} {dtype} C={C} {form}'
            res = _run(c['f0'], c['f1'], c['thr'], form)
            _check_regime(c, res, what)
            results.append(res)
            if regime == 'ties':
                # cell 0 of the all-equal windows: offsets (-2, -2); and the same windows at thr = 1.0, where the saturated cells are exactly
                # 1.0: '>' accepts nothing
                flat = [m for m in range(R.M_REG) if R.KINDS[m % 5] == 'c']
                pos = torch.searchsorted(res['m_bids'], torch.tensor(flat))
                assert torch.equal(res['mkpts0_f'][pos], torch.full((len(flat), 2), -4.0)) and torch.equal(res['mkpts1_f'][pos], torch.full((len(flat), 2), -4.0))
                assert _run(c['f0'], c['f1'], 1.0, form)['count'] == 0, what
            if regime == 'nonfinite':
                # the other matches: the bits of the same call with finite windows in place of the non-finite ones
                twin = _run(c['twin'][0], c['twin'][1], c['thr'], form)
                good = torch.tensor([m for m in range(R.M_REG) if m not in c['bad']])
                assert torch.equal(res['fine_matrix'][good].view(torch.int32), twin['fine_matrix'][good].view(torch.int32)), what
                keep = ~torch.isin(twin['m_bids'], torch.tensor(c['bad']))
                assert int((~keep).sum()) >= 2 and res['count'] == int(keep.sum()), what
                for k in ('mkpts0_f', 'mkpts1_f', 'mconf', 'm_bids'):
                    assert torch.equal(res[k], twin[k][keep]), (what, k)
        if len(results) == 2:                                                    # MFMA (or C = 72's scalar) form against the shifted copy's
            a, b = results
            assert a['count'] == b['count'] and all(torch.equal(a[k], b[k]) for k in ('m_bids', 'mkpts0_f', 'mkpts1_f')), (regime, C)


@pytest.mark.parametrize('dtype', R.TYPES, ids=str)
def test_fine_match_launch_edges(dtype):
    """M = 1, 3, 4, 5: less than one MFMA workgroup, exactly one, one and a ragged second."""
    for M in R.EDGE_MS:
        for C in R.EDGE_CS:
            c = R.case('control', dtype, C, M)
            for form in _forms(dtype):
                _check_regime(c, _run(c['f0'], c['f1'], c['thr'], form), f'control M={M} {dtype} C={C} {form}')


@pytest.mark.parametrize('dtype,C', R.COMPACT_FORMS, ids=str)
def test_fine_match_compaction_and_keypoints(dtype, C):
    """M = 2125 (three chunks, the last ragged, 2125 % 4 == 1; once with chunk 1 empty, once with match 1024 accepted), 1025, 1024, from large
    to small so that the cached workspace is reused at a smaller M; N = 3 samples with distinct per-sample scales, and without scales;
    non-integer coarse keypoints.  count, order, confidences, keypoints against float64; a second call gives the same bits; a call in which
    nothing passes gives count == 0."""
    for M in R.COMPACT_M:
        for pattern in (('empty1', 'mixed') if M > 2048 else ('mixed',)):
            c = R.compaction_case(M, pattern, dtype, C)
            ref = c['ref']
            want = torch.nonzero(ref['ok'])[:, 0]
            assert torch.equal(ref['ok'], c['accept']) and len(want) > 0
            for scaled in (True, False):
                what = f'compaction M={M} {pattern} {dtype} C={C} scaled={scaled}'
                sc = (c['scale0'], c['scale1']) if scaled else (None, None)
                res = _run(c['f0'], c['f1'], c['thr'], 'aligned', c['b_ids'], c['mkpts0_c'], c['mkpts1_c'], *sc)
                assert res['count'] == len(want), (what, res['count'], len(want))
                assert torch.equal(res['m_bids'], c['b_ids'][want]), what
                cells = ref['sel'][want]
                assert torch.equal(res['mconf'].view(torch.int32), res['fine_matrix'].flatten(1)[want, cells].view(torch.int32)), what
                if scaled:
                    _conf_check(res, c, what)
                r = R.conf_error(res['mconf'], ref['conf'].flatten(1)[want, cells], c['tol'].flatten(1)[want, cells])
                assert float(r.max()) <= 1.0, what
                mk0, mk1, b0, b1 = R.keypoints64(ref['sel'], c['b_ids'], c['mkpts0_c'], c['mkpts1_c'], *sc)
                e0, e1 = (res['mkpts0_f'].double() - mk0).abs() / b0, (res['mkpts1_f'].double() - mk1).abs() / b1
                print(f'  {what}: keypoint error / budget max {float(torch.maximum(e0, e1).max()):.3f}')
                assert float(e0.max()) <= 1.0 and float(e1.max()) <= 1.0, what
                again = _run(c['f0'], c['f1'], c['thr'], 'aligned', c['b_ids'], c['mkpts0_c'], c['mkpts1_c'], *sc)
                _same_bits(res, again, what)
    c = R.compaction_case(1025, 'none', dtype, C)
    assert not bool(c['ref']['ok'].any())
    res = _run(c['f0'], c['f1'], c['thr'], 'aligned', c['b_ids'], c['mkpts0_c'], c['mkpts1_c'], c['scale0'], c['scale1'])
    assert res['count'] == 0 and len(res['m_bids']) == 0
    _conf_check(res, c, f'nothing accepted {dtype} C={C}')
