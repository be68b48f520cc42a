"""The backward kernels of the training step against float64 in the regimes of tests/backward_regimes.py: offsets that put phi on one
branch, S / den beyond fp16's range, a few valid keys among 1280 and an image without any, heads that do not look alike, LayerNorm rows far
from centred or constant, saturated activations, one-hot and flat softmaxes.

The reference is float64 autograd of the reference formula on the kernel's own operands, the unit of error one ulp of the storage type at
the size of the TERMS an element is made of; the budget of every line is what the restatement with the kernel's rounding points loses
against float64 (backward_regimes.REST, measured on the CPU by tests/test_backward_regimes.py) plus the stated margin (budget(): + 2 ulp on
the maximum, 1.5 x + 0.05 ulp on the mean).  No element is left out; rows a mask removes must be exact zeros; nothing may be inf or NaN; two
launches give the same bits.  Which wrong kernels these lines would catch is what the CPU file's mutation tests state."""
import pytest
import torch

import backward_regimes as B
import linear_attention_regimes as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
H16, BF16, F32 = B.H16, B.BF16, B.F32


def _ids(p):
    return R.NAME.get(p, str(p))


def _within(errs, buds, names, what):
    for nm, err, bud in zip(names, errs, buds):
        print(what, nm, 'error (max, mean) = (%.3f, %.4f) ulp, budget (%.3f, %.4f)' % (err + bud))
    for nm, err, bud in zip(names, errs, buds):
        assert err[0] <= bud[0] and err[1] <= bud[1], (what, nm, err, bud)


def _twice(fn):
    a, b = fn(), fn()
    for x, y in zip(a, b):
        assert torch.equal(x, y), 'two launches differ'
        assert bool(torch.isfinite(x).all())
    return a


def _worse(worst, errs):
    return errs if worst is None else tuple((max(w[0], e[0]), max(w[1], e[1])) for w, e in zip(worst, errs))


# ------------------------------------------------------------------------------------------------------------------- linear attention
@pytest.mark.parametrize('regime,variant,st', [(r, v, st) for (r, v), types in B.LA.items() for st in types], ids=_ids)
def test_linear_attention_backward(regime, variant, st):
    """ops.linear_attention_backward, 8 heads of 32, N = 3 (few_keys: 4, one image without a valid key): L = 300 on S = 520 (chunks of 256
    tokens: a ragged second query chunk, three source chunks, the last with 8 tokens), control also L = 256 on one key, few_keys and
    sparse_v on their 1280 keys; k and v are row-strided views of one buffer."""
    from geoformer_amd import ops
    worst = None
    for L, S in B.la_shapes(regime):
        q, k, v, dout, qm, km, ref = B.la_case(regime, variant, st, L, S)
        kv = torch.cat([k, v], -1).to(DEV)
        kd, vd = kv[..., :256], kv[..., 256:]
        qd, gd = q.to(DEV), dout.to(DEV)
        qmd, kmd = (None if m is None else m.to(DEV) for m in (qm, km))
        got = _twice(lambda: ops.linear_attention_backward(qd, kd, vd, gd, 8, qmd, kmd))
        assert all(x.dtype == st for x in got)
        if qm is not None:
            assert float(got[0][~qmd].abs().max()) == 0.0
        if km is not None:
            assert float(got[1][~kmd].abs().max()) == 0.0 and float(got[2][~kmd].abs().max()) == 0.0
        if regime == 'few_keys':                             # the image without a valid key: every gradient an exact zero
            assert all(float(x[3].abs().max()) == 0.0 for x in got)
        worst = _worse(worst, B.grad_errors(got, ref, st))
    _within(worst, B.budgets('la', regime, variant, st), B.GRADS, f'la {R.key(regime, variant)} {R.NAME[st]}')


@pytest.mark.parametrize('regime,variant,st', [(r, v, st) for (r, v), types in B.LAW.items() for st in types], ids=_ids)
def test_window_linear_attention_backward(regime, variant, st):
    """ops.window_linear_attention_backward, 8 heads of 16: (Nw, Lw) = (7, 25), (6, 32), (3, 9), (5, 1) - a last workgroup with spare waves,
    full windows, and a window of one token."""
    from geoformer_amd import ops
    worst = None
    for Nw, Lw in B.LAW_SHAPES:
        q, k, v, dout, ref = B.law_case(regime, variant, st, Nw, Lw)
        qd, kd, vd, gd = (t.to(DEV) for t in (q, k, v, dout))
        got = _twice(lambda: ops.window_linear_attention_backward(qd, kd, vd, gd))
        assert all(x.dtype == st and x.shape == (Nw, Lw, 128) for x in got)
        worst = _worse(worst, B.grad_errors(got, ref, st))
    _within(worst, B.budgets('law', regime, variant, st), B.GRADS, f'law {R.key(regime, variant)} {R.NAME[st]}')


# ------------------------------------------------------------------------------------------------------------------- LayerNorm
def _ln_backward(dout, y, stats, gamma, dg, db, accumulate):
    """gf_layernorm_backward with the caller's dgamma / dbeta (ops.layernorm_backward always overwrites fresh ones)."""
    from geoformer_amd import _lib, ops
    C = y.shape[-1]
    dy = torch.empty_like(y)
    L_ = _lib.lib()
    ws = ops._ws.get('lnbwd', L_.gf_layernorm_backward_workspace_bytes(C), y.device)
    ops.check(L_.gf_layernorm_backward(ops._p(dout), ops._p(y), ops._p(stats), ops._dt(y), y.shape[0], C, ops._p(gamma), ops._p(dy), ops._p(dg),
                                       ops._p(db), int(accumulate), ops._p(ws), ws.numel(), ops._stream()), 'gf_layernorm_backward')
    return dy


@pytest.mark.parametrize('st', [H16, BF16], ids=_ids)
@pytest.mark.parametrize('C', B.LN_C)
def test_layernorm_forward_backward(C, st):
    """ops.layernorm_forward / ops.layernorm_backward at T = 5, 1003 and 4 x 512 + 5 rows (the backward's 512 workgroups: fewer than that,
    and a ragged second round), rows with |mean| / std of 8, 32 (bf16: 128), a constant row and a row of zeros: out, the saved mean and
    rstd, dy, dgamma, dbeta; dgamma and dbeta once more in accumulate mode."""
    from geoformer_amd import ops
    case = B.ln_case(C, st)
    gamma, beta = case['gamma'].to(DEV), case['beta'].to(DEV)
    worst = None
    for T in B.LN_T:
        y, dout = case['y'][:T].to(DEV), case['dout'][:T].to(DEV)
        out, stats = _twice(lambda: ops.layernorm_forward(y, gamma, beta, B.LN_EPS))
        dy, dg, db = _twice(lambda: ops.layernorm_backward(dout, y, stats, gamma))
        assert out.dtype == st and dy.dtype == st and dg.dtype == torch.float32
        got = dict(out=out, dy=dy, dgamma=dg, dbeta=db, mean=stats[:, 0], rstd=stats[:, 1])
        worst = _worse(worst, B.ln_errors(got, case, st, T))
        assert float(stats[0, 0]) == 3.25 and float(out[2].float().sub(beta).abs().max()) <= B.EPS[st] * float(beta.abs().max())
        # accumulate mode: one fp32 addition onto what the buffers held
        g = torch.Generator().manual_seed(T)
        dg0, db0 = torch.randn(C, generator=g).to(DEV), torch.randn(C, generator=g).to(DEV)
        dg1, db1 = dg0.clone(), db0.clone()
        dy1 = _ln_backward(dout, y, stats, gamma, dg1, db1, True)
        assert torch.equal(dy1, dy) and torch.equal(dg1, dg0 + dg) and torch.equal(db1, db0 + db)
        _ln_backward(dout, y, stats, gamma, dg1, db1, False)
        assert torch.equal(dg1, dg) and torch.equal(db1, db)
    _within(worst, B.budgets('ln', 'c', C, st), B.LN_OUT, f'ln C = {C} {R.NAME[st]}')


# ------------------------------------------------------------------------------------------------------------------- activation backward
@pytest.mark.parametrize('st', [H16, BF16], ids=_ids)
@pytest.mark.parametrize('n', B.ACT_SIZES)
def test_activation_backward(n, st):
    """ops.activation_backward: dz = round(dh act'(h)) from the float64 product is exact to half an ulp - ReLU bit for bit, tanh within one
    ulp (neighbouring values of the storage type, subnormals included); h = +-1, +-0, the smallest subnormal, the largest finite dh."""
    from geoformer_amd import ops
    dh, h, ref = B.act_case(st, n)
    dhd, hd = dh.to(DEV), h.to(DEV)
    relu, = _twice(lambda: (ops.activation_backward(dhd, hd, 'relu'),))
    assert torch.equal(relu.cpu(), ref['relu'].to(st))
    tanh, = _twice(lambda: (ops.activation_backward(dhd, hd, 'tanh'),))
    want = ref['tanh'].to(st)
    assert bool(torch.isfinite(want).all())
    step = (B.ordered(tanh.cpu()) - B.ordered(want)).abs()
    print(f'act tanh {R.NAME[st]} n = {n}: elements one ulp off {int((step == 1).sum())}, more {int((step > 1).sum())}')
    assert int(step.max()) <= 1
    assert float(tanh[:2].abs().max()) == 0.0                  # h = +-1: saturated


# ------------------------------------------------------------------------------------------------------------------- full attention
@pytest.mark.parametrize('st', [H16, BF16], ids=_ids)
@pytest.mark.parametrize('regime', B.FA_REGIMES)
def test_full_attention_train_forward_backward(regime, st):
    """ops.full_attention_train_forward -> ops.full_attention_backward (the backward takes the forward's own out and lse2), 4 heads of 64,
    N = 2, S in {1, 31, 32, 33, 97} x L in {37, 128, 130}, q a row-strided view: out, lse2 (log2 units), dq, dk, dv."""
    from geoformer_amd import ops
    worst = None
    for L, S in B.fa_shapes():
        q, k, v, dout, ref = B.fa_case(regime, st, L, S)
        wide = torch.zeros(2, L, 768, dtype=st, device=DEV)
        wide[..., 256:512] = q.to(DEV)
        qd, kd, vd, gd = wide[..., 256:512], k.to(DEV), v.to(DEV), dout.to(DEV)
        out, lse = _twice(lambda: ops.full_attention_train_forward(qd, kd, vd, 4))
        dq, dk, dv = _twice(lambda: ops.full_attention_backward(qd, kd, vd, out, gd, lse, 4))
        assert out.dtype == st and lse.dtype == torch.float32 and lse.shape == (2, 4, L)
        worst = _worse(worst, B.fa_errors(dict(out=out, lse2=lse, dq=dq, dk=dk, dv=dv), ref, st))
    _within(worst, B.budgets('fa', regime, None, st), B.FA_OUT, f'fa {regime} {R.NAME[st]}')


# ------------------------------------------------------------------------------------------------------------------- fine matching
@pytest.mark.parametrize('st', B.FM_TYPES, ids=_ids)
@pytest.mark.parametrize('regime', B.FM_REGIMES)
def test_fine_match_backward(regime, st):
    """ops.fine_match_backward, three matches of 25 x 25, C = 128 and 64; the budget in ulps of the type df0 / df1 are stored in."""
    from geoformer_amd import ops
    worst = None
    for C in B.FM_C:
        f0, f1, dconf, ref = B.fm_case(regime, st, C)
        f0d, f1d, gd = f0.to(DEV), f1.to(DEV), dconf.to(DEV)
        got = _twice(lambda: ops.fine_match_backward(f0d, f1d, B.FM_TEMP, gd))
        assert all(x.dtype == st and x.shape == (3, 25, C) for x in got)
        worst = _worse(worst, B.fm_errors(got, ref, st))
    _within(worst, B.budgets('fm', regime, None, st), ('df0', 'df1'), f'fm {regime} {R.NAME[st]}')
