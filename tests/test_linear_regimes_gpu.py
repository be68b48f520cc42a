"""The K3 linear kernels (ops.linear, ops.linear_rows, ops.conv1x1, ops.conv1x1_upsample_add) against float64 on the lines of
tests/linear_regimes.py: every dispatch branch of the four entry points, row counts at the edges of the wave and workgroup tiles, ragged
column tiles, single-step and two-part K, and operands steered to where a kernel's rounding points show.

The reference is float64 of the header's formula on the kernel's own operands, the unit of error one ulp of the storage type at the size of
the TERMS an element is made of, and the budget of a line what the restatement with the kernel's rounding points loses against float64
(linear_regimes.REST, measured on the CPU by tests/test_linear_regimes.py) plus the project's margin (budget(): + 2 ulp on the maximum,
1.5 x + 0.05 ulp on the mean).  No element is left out; nothing may be inf or NaN; every call is made twice and gives the same bits; the
77s around outputs, operands and inside skipped tiles stay; rows a zero flag skips are bit copies of the residual; on every 16-bit line of
ops.linear, ops.linear_rows on a table of the operand's rows gives the same bits (linear_kernel_w2 and linear_kernel share their
accumulation order).  Which wrong kernels these lines would catch is what the CPU file's mutation tests state."""
import pytest
import torch

import linear_regimes as L

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CANARY = 77.0
EPI = {'none': 0, 'relu': 1, 'tanh': 2, 'ln': 3, 'ln_res': 4}


def _within(err, bud, what):
    print(what, 'error (max, mean) = (%.3f, %.4f) ulp, budget (%.3f, %.4f)' % (err + bud))
    assert err[0] <= bud[0] and err[1] <= bud[1], (what, err, bud)


def _canaried(M, N, st):
    """(the whole buffer, its rows 1 .. M): a row of 77s before and behind the output."""
    big = torch.full((M + 2, N), CANARY, dtype=st, device=DEV)
    return big, big[1:M + 1]


def _intact(big):
    return bool((big[0] == CANARY).all()) and bool((big[-1] == CANARY).all())


def _strided(t):
    """t [M, K] (device) as a row-strided view of a wider, longer buffer of 77s: eight elements before and behind every row."""
    M, K = t.shape
    wide = torch.full((M + 2, K + 16), CANARY, dtype=t.dtype, device=DEV)
    wide[1:M + 1, 8:8 + K] = t
    return wide[1:M + 1, 8:8 + K]


def _table(view, idx=None, zero=None):
    """The address table of a row-strided view's rows (idx: of those rows, repeats allowed; zero: entries replaced by the zero address)."""
    M = view.shape[0]
    idx = torch.arange(M) if idx is None else idx
    table = view.data_ptr() + idx * (view.stride(0) * view.element_size())
    if zero is not None:
        table = table.masked_fill(zero, 0)
    return table.to(DEV)


def _device(case):
    return {k: v.to(DEV) for k, v in case.items() if isinstance(v, torch.Tensor) and k in ('a', 'w', 'bias', 'gamma', 'beta', 'res', 'rgb', 'flag', 'src', 'x', 'lo')}


def _kwargs(case, d, M):
    """The keyword arguments ops.linear and ops.linear_rows share, for the first M rows of the case."""
    sp = case['sp']
    kw = dict(bias=d.get('bias'), epilogue=EPI[sp['epi']], eps=case['eps'])
    if 'rgb' in d:
        kw.update(rowgroup_bias=d['rgb'][:(M + sp['rg'] - 1) // sp['rg']], rowgroup_rows=sp['rg'])
    if sp['epi'] in ('ln', 'ln_res'):
        kw['ln'] = (d['gamma'], d['beta'])
    if sp['epi'] == 'ln_res':
        kw['residual'] = _strided(d['res'][:M])
        if 'flag' in d:
            kw.update(row_flag=d['flag'][:(M + sp['fr'] - 1) // sp['fr']], flag_rows=sp['fr'])
    return kw


def _same_twice(fn, M, N, st):
    """fn(out) run into two fresh canaried buffers: the same bits, finite, the canaries intact -> the first result."""
    outs = []
    for _ in range(2):
        big, out = _canaried(M, N, st)
        fn(out)
        assert _intact(big), 'a row before or behind the output was written'
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), 'two launches differ'
    assert bool(torch.isfinite(outs[0]).all())
    return outs[0]


def _run_linear(case, d, M):
    from geoformer_amd import ops
    sp, st = case['sp'], case['st']
    k1, N = sp['k1'], sp['n']
    a1 = _strided(d['a'][:M, :k1])
    a2 = _strided(d['a'][:M, k1:]) if sp['k2'] else None
    kw = _kwargs(case, d, M)
    out = _same_twice(lambda o: ops.linear(a1, d['w'], a2=a2, out=o, **kw), M, N, st)
    if sp['epi'] == 'ln_res':
        skip = ~L.keep_rows(case, M).to(DEV)
        assert torch.equal(out[skip], d['res'][:M][skip]), 'a skipped row is not a bit copy of the residual'
    if st != L.F32:
        # the rows named by a table, both operand parts side by side: linear_kernel's AROWS instance of the same epilogue must give the bits of
        # whichever kernel ops.linear took (linear_kernel_w2 at N % 256 == 0 without LayerNorm and row-group bias)
        both = _strided(d['a'][:M])
        table = _table(both, zero=(case['a'][:M] == 0).all(1))                  # a row of zeros (ln_flat, tanh_span) is named by the zero address
        rows = _same_twice(lambda o: ops.linear_rows(table, d['w'], out=o, **kw), M, N, st)
        assert torch.equal(rows, out), 'linear_rows on the operand\'s own rows differs from linear'
    return out


def _run_rows(case, d, M):
    from geoformer_amd import ops
    sp, st = case['sp'], case['st']
    N = sp['n']
    src = _strided(d['src'])
    kw = _kwargs(case, d, M)
    if 'counts' not in case:
        table = _table(src, case['idx'][:M], case['zero'][:M])
        out = _same_twice(lambda o: ops.linear_rows(table, d['w'], out=o, **kw), M, N, st)
        gathered = d['a'][:M].contiguous()
        assert torch.equal(out, ops.linear(gathered, d['w'], **kw)), 'linear_rows differs from linear on the gathered copy'
        return out
    G = sp['groups']
    table = _table(src, case['idx']).view(G, L.GROUP_R)
    counts = torch.zeros(G, 2, dtype=torch.int32, device=DEV)                    # the counts as a strided view
    counts[:, 0] = torch.tensor(case['counts'], dtype=torch.int32)
    outs = []
    for _ in range(2):
        big, out = _canaried(M, N, st)
        ops.linear_rows(table, d['w'], out=out.view(G, L.GROUP_R, N), group_count=counts[:, 0], **kw)
        assert _intact(big)
        outs.append(out)
    assert torch.equal(outs[0], outs[1]), 'two launches differ'
    done = case['computed'].to(DEV)
    assert 0 < int(done.sum()) < M
    assert bool((outs[0][~done] == CANARY).all()), 'a tile without a wanted row was written'
    assert bool(torch.isfinite(outs[0]).all())
    full = ops.linear(d['a'].contiguous(), d['w'], **kw)
    assert torch.equal(outs[0][done], full[done])
    return outs[0]


def _run_conv(case, d, M):
    from geoformer_amd import _lib, ops
    sp, st = case['sp'], case['st']
    nimg, H, W, stride = sp['geom']
    x = d['x'].permute(0, 3, 1, 2)                                              # channels_last [n, Cin, H, W]
    out = ops.conv1x1(x, d['w'], stride)
    assert out.shape == (nimg, sp['n'], H // stride, W // stride) and out.dtype == st
    out = out.permute(0, 2, 3, 1).reshape(M, sp['n'])
    big, again = _canaried(M, sp['n'], st)
    ops.check(_lib.lib().gf_conv1x1_nhwc(ops._p(d['x']), ops._p(d['w']), ops._p(again), nimg, H, W, sp['k1'], sp['n'], stride, ops._dt(d['x']),
                                         ops._stream()), 'gf_conv1x1_nhwc')
    assert _intact(big) and torch.equal(out, again) and bool(torch.isfinite(out).all())
    return out


def _run_upadd(case, d, M):
    from geoformer_amd import _lib, ops
    sp, st = case['sp'], case['st']
    nimg, H, W, h, wl = sp['geom']
    out = ops.conv1x1_upsample_add(d['x'].permute(0, 3, 1, 2), d['w'], d['lo'].permute(0, 3, 1, 2))
    assert out.shape == (nimg, sp['n'], H, W) and out.dtype == st
    out = out.permute(0, 2, 3, 1).reshape(M, sp['n'])
    big, again = _canaried(M, sp['n'], st)
    ops.check(_lib.lib().gf_conv1x1_upsample_add_nhwc(ops._p(d['x']), ops._p(d['w']), ops._p(d['lo']), ops._p(again), nimg, h, wl, H, W, sp['k1'],
                                                      sp['n'], ops._dt(d['x']), ops._stream()), 'gf_conv1x1_upsample_add_nhwc')
    assert _intact(big) and torch.equal(out, again) and bool(torch.isfinite(out).all())
    return out


RUN = {'linear': _run_linear, 'rows': _run_rows, 'conv': _run_conv, 'upadd': _run_upadd}


@pytest.mark.parametrize('line', L.lines(), ids=L.line_id)
def test_line_within_budget(line):
    """One line of linear_regimes.REST: every shape and row count of the form, the worst (max, mean) against the line's budget."""
    form, regime, variant, st = line
    worst = None
    for sp in L.specs(form, st, regime):
        case = L.cached_case(sp, regime, variant, st)
        d = _device(case)
        for M in sp['Ms']:
            out = RUN[sp['entry']](case, d, M)
            assert out.dtype == st and out.shape == (M, sp['n'])
            if regime == 'ln_flat':                                            # the rows of zero variance: round(beta), exactly
                flat = out[::5]
                assert torch.equal(flat, d['beta'].to(st).expand_as(flat))
            worst = L.worse(worst, L.case_error(out, case, M))
    _within(worst, L.line_budget(*line), L.line_id(line))


@pytest.mark.parametrize('line', L.lines(exact=True), ids=L.line_id)
def test_exact_line_is_float64_rounded_once(line):
    """Integer operands, weights and bias in eighths: fp32 accumulation is exact in any order, so the output is the float64 result rounded
    once, bit for bit - whatever K chunk, row or column a kernel dropped, doubled or misrouted."""
    form, regime, variant, st = line
    for sp in L.specs(form, st, regime):
        case = L.cached_case(sp, regime, variant, st)
        d = _device(case)
        want = case['ref'].to(st)
        for M in sp['Ms']:
            out = RUN[sp['entry']](case, d, M)
            assert torch.equal(out.cpu(), want[:M]), (L.line_id(line), sp['k1'], sp['k2'], sp['n'], M)


@pytest.mark.parametrize('N', [160, 224])
@pytest.mark.parametrize('st', L.SIXTEEN + (L.F32,), ids=lambda t: L.NAME[t])
def test_rowgroup_bias_on_a_ragged_column_tile_is_refused(st, N):
    """The epilogue reads whole column tiles of the row-group bias: N % 128 != 0 would read behind the table.  Both entry points refuse it
    before anything is launched."""
    from geoformer_amd import _lib, ops
    a = torch.zeros(50, 64, dtype=st, device=DEV)
    w = torch.zeros(N, 64, dtype=st, device=DEV)
    rg = torch.zeros(2, N, dtype=st, device=DEV)
    big, out = _canaried(50, N, st)
    with pytest.raises(_lib.GeoFormerHipError, match='multiple of 128'):
        ops.linear(a, w, rowgroup_bias=rg, rowgroup_rows=25, out=out)
    if st != L.F32:
        with pytest.raises(_lib.GeoFormerHipError, match='multiple of 128'):
            ops.linear_rows(_table(a), w, rowgroup_bias=rg, rowgroup_rows=25, out=out)
    torch.cuda.synchronize()
    assert bool((big == CANARY).all())
    ops.linear(a, w, out=out)                                   # without the row-group bias the shape is served
    assert bool((out == 0).all()) and _intact(big)
