"""CPU checks of softmax_regimes.py: the generators are deterministic and produce the regimes they claim (branch counts under the
kernels' rules on float64 logits), and the oracle's restatement of K4's deferred reference matches float64 at any threshold."""
import pytest
import torch

import geoformer_oracle as O
import softmax_regimes as R


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_k4_generators_deterministic(dtype):
    a = R.k4_inputs('straddle', dtype, 1200)
    b = R.k4_inputs('straddle', dtype, 1200)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    f = R.k1_features('boundary', (1, 256, 6400), dtype)
    g = R.k1_features('boundary', (1, 256, 6400), dtype)
    assert torch.equal(f[0], g[0]) and torch.equal(f[1], g[1])


def test_k4_spike_positions():
    assert R.k4_spike_positions(1) == [] and R.k4_spike_positions(33) == [32]
    assert R.k4_spike_positions(1195) == [37, 583, 1163, 1194]
    for K in R.K4_KEYS:
        assert all(R.K4_TILE <= p < K for p in R.k4_spike_positions(K))


@pytest.mark.parametrize('regime,floors', [('spike', {'moves': 5000}), ('staircase', {'moves': 50000}), ('range', {'moves': 5000}),
                                           ('straddle', {'near_declined': 5000, 'near_taken': 5000})])
def test_k4_branch_counts(regime, floors):
    """The decisions after tile 0 that move the reference (or fall within 0.2 of the threshold) under the restated rule."""
    q, kv, idx, nkeys = R.k4_inputs(regime, torch.float16, 1200)
    logits = R.k4_reference(q, kv, idx, nkeys)[-1]
    c = R.k4_branch_counts(logits)
    print(regime, c)
    for k, v in floors.items():
        assert c[k] >= v, (k, c[k])
    if regime == 'straddle':
        assert c["closest"] > 1e-3


def test_k4_tile0_dominant():
    q, kv, idx, nkeys = R.k4_inputs('tile0', torch.float16, 1200)
    logits = R.k4_reference(q, kv, idx, nkeys)[-1]
    assert R.k4_branch_counts(logits)['moves'] == 0
    lead = min(float(x[..., :32].amax(-1).min() - x[..., 32:].amax(-1).max()) for x in logits if x is not None and x.shape[-1] > 32)
    assert lead >= 30


@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
@pytest.mark.parametrize('shape', R.K1_SHAPES)
def test_k1_regimes_force_their_branches(shape, dtype):
    """k1_stats_panel's rule stepped through every run (softmax_regimes.k1_panel_sim): growth rescales every wave at every tile after a
    run start, deep makes the gamma < 0 tiles deep, boundary reaches non-deep, unrescaled tiles with a subnormal exp2(ref - kappa)
    that carries column maxima; the control regime takes none of the branches."""
    for regime in ('growth', 'deep', 'boundary'):
        R.k1_assert_regime(regime, R.k1_logits2(*R.k1_features(regime, shape, dtype)))
    sim = R.k1_panel_sim(R.k1_logits2(*R.k1_features('control', shape, dtype)))
    assert sim['rescales'] == sim['deep'] == sim['boundary'] == 0


def test_k1_panel_sim_rules():
    """The simulator on hand-made logits: a jump of 65 after tile 0 rescales, 63 does not; a column 65 below kappa is deep."""
    x = torch.zeros(1, 32, 128, dtype=torch.float64)
    assert R.k1_panel_sim(x)['rescales'] == 0
    x[0, 5, 64 + 7] = 65.0
    assert R.k1_panel_sim(x)['rescales'] == 1
    x[0, 5, 64 + 7] = 63.0
    assert R.k1_panel_sim(x)['rescales'] == 0
    y = torch.zeros(1, 32, 128, dtype=torch.float64)
    y[:, :, 64:] = -65.0
    assert R.k1_panel_sim(y)['deep'] == 1 and R.k1_panel_sim(y)['rescales'] == 0


@pytest.mark.parametrize('defer', [8.0, 0.0])
@pytest.mark.parametrize('dtype', [torch.float16, torch.bfloat16])
def test_flash_restatement_matches_fp64(dtype, defer):
    """O._flash_self_attention at threshold 8 and 0 on a small spike / staircase input: within the float64 bound of
    softmax_regimes._k4_bound."""
    for regime in ('spike', 'staircase'):
        q, kv, idx, nkeys = R.k4_inputs(regime, dtype, 1200)
        sel = [4, 5]                                                        # 97 and 224 keys
        q, kv, idx, nkeys = q[sel], kv[sel], idx[sel], nkeys[sel]
        ref, _, bound, _, _ = R.k4_reference(q, kv, idx, nkeys)
        L, C = q.shape[1], R.K4_C
        for b in range(len(sel)):
            K = int(nkeys[b])
            tok = idx[b, :K].long()
            f = O._flash_self_attention(q[b].float().view(L, 4, 64), kv[b, tok, :C].float().view(K, 4, 64),
                                        kv[b, tok, C:].float().view(K, 4, 64), dtype, defer=defer).reshape(L, C).double()
            r = (f - ref[b]).abs() / bound[b]
            assert float(r.max()) <= 1.0 and float(r.mean()) <= 0.5, (regime, float(r.max()))
