"""K28, the workgroup tier of the effect-size gate (pooled windows of up to
8,192 points): the kernel against the numpy reference, bit for bit, at the
16-key chunk boundary, on both walking sides and their tie, at the first
shapes past K19, lopsided, at 16 walkers per thread and one over, at the
power-of-two tail and the pooled cap; the routing of ``pairwise_effect`` and
of a gated scorer; the CPU path."""
import numpy as np
import pytest
import torch

from foremast_amd.config import BrainConfig
from foremast_amd.engine.resident import ResidentHistory
from foremast_amd.engine.scorer import CanaryScorer
from foremast_amd.ops import canary as C
from foremast_amd.ops import reference as ref

from test_effect_ops import BOUND3, GATES, PATTERNS, _check_gpu, _pattern, _same

F = np.float32


def _expect(eff, gate, pv, bound=BOUND3):
    want = ref.effect_gate(eff, bound[np.arange(len(eff)) % len(bound)], gate.min_effect, gate.min_shift,
                           gate.min_shift_abs, gate.directional)
    return want, np.where(want[:, None] != 0, pv, F(np.nan))


@pytest.mark.gpu
@pytest.mark.parametrize("n1,n2", [(1, 1), (1, 40), (40, 1), (15, 17), (16, 16), (17, 16), (255, 257), (513, 512),
                                   (1040, 24), (24, 1040)])
@pytest.mark.parametrize("name", PATTERNS)
def test_gpu_wide_tier_matches_reference(cuda, name, n1, n2):
    cur, base = _pattern(name, n1, n2, 5)
    eff, cnt = ref.pairwise_effect(cur, base)
    pv = np.random.default_rng(5).random((5, 6)).astype(F)
    want, gated = _expect(eff, GATES[4], pv)
    C.reset_effect_route_rows()
    c, b = (torch.from_numpy(np.array(a, order="C")).to(cuda) for a in (cur, base))     # (row-major copies)
    r = C.pairwise_effect(c, b, GATES[4], torch.from_numpy(BOUND3).to(cuda), 3, torch.from_numpy(pv).to(cuda),
                          tier="wide")
    torch.cuda.synchronize()
    assert C.effect_route_rows() == {"wave": 0, "wide": 5, "oracle": 0}
    _same(r.effect.cpu().numpy(), eff)
    _same(r.counts.cpu().numpy(), cnt)
    _same(r.passed.cpu().numpy(), want)
    _same(r.pvals_gated.cpu().numpy(), gated)


@pytest.mark.gpu
@pytest.mark.parametrize("n1,n2", [(2049, 2047), (4095, 4097), (4096, 4096), (8191, 1), (1, 8191)])
@pytest.mark.parametrize("name", ["random", "three_values", "nan_inf"])
def test_gpu_large_shapes_take_the_wide_tier(cuda, name, n1, n2):
    cur, base = _pattern(name, n1, n2, 2)
    C.reset_effect_route_rows()
    _check_gpu(cuda, cur, base, *ref.pairwise_effect(cur, base))
    assert C.effect_route_rows() == {"wave": 0, "wide": 2 * len(GATES), "oracle": 0}


@pytest.mark.gpu
def test_gpu_padded_batch_is_bucketed_into_three_tiers(cuda):
    """Padded to 5,000 + 5,000 columns: rows of up to 100 points per side (K19),
    600 + 650 and 3,000 + 3,000 (K28), 5,000 + 4,000 (the host)."""
    rng = np.random.default_rng(28)
    R, W = 9, 5000
    used = [(int(rng.integers(1, 101)), int(rng.integers(1, 101))) for _ in range(R)]
    used[2], used[5], used[7] = (600, 650), (3000, 3000), (5000, 4000)
    cur = np.full((R, W), np.nan, F)
    base = np.full((R, W), np.nan, F)
    eff, cnt = np.empty((R, 4), F), np.empty((R, 2), np.int32)
    for r, (a, b) in enumerate(used):
        cur[r, :a] = rng.normal(10, 3, a)
        base[r, :b] = rng.normal(10.5, 3, b)
        eff[r], cnt[r] = (v[0] for v in ref.pairwise_effect(cur[r:r + 1, :a], base[r:r + 1, :b]))
    C.reset_effect_route_rows()
    _check_gpu(cuda, cur, base, eff, cnt, gates=[GATES[4]])
    assert C.effect_route_rows() == {"wave": R - 3, "wide": 2, "oracle": 1}


@pytest.mark.gpu
def test_gpu_gated_scorer_ticks_on_the_wide_tier(cuda):
    """The resident tick (the scorer's path for windows beyond the wave kernels)."""
    M, S, T, n_cur, n_base = 3, 3, 64, 600, 700
    R = S * M
    rng = np.random.default_rng(4)
    hist = (100 + 3 * rng.standard_normal((R, T))).astype(F)
    base = (100 + rng.standard_normal((R, n_base))).astype(F)
    cur = (100 + rng.standard_normal((R, n_cur)) + np.array([0.0, 3.0, -3.0], F)[np.arange(R) % 3][:, None]).astype(F)
    cfg = BrainConfig(threshold=3.0, bound=1, pairwise_min_shift=0.02, pairwise_directional=True)
    sc = CanaryScorer(["err", "lat", "cpu_x"], cfg, cuda)
    b, c = torch.from_numpy(base).to(cuda), torch.from_numpy(cur).to(cuda)
    C.reset_effect_route_rows()
    store = ResidentHistory(T, cuda)
    rows, _ = store.rows_for([("k", i) for i in range(R)], owner=("ns", "app"))
    store.write_static(rows, list(hist), np.zeros(R))
    o = sc.score_resident(store.view(), torch.from_numpy(rows.astype(np.int32)).to(cuda), c, b)
    torch.cuda.synchronize()
    assert C.effect_route_rows() == {"wave": 0, "wide": R, "oracle": 0}
    eff, cnt = ref.pairwise_effect(cur, base)
    want, gated = _expect(eff, sc.gate, o.pvals.cpu().numpy(), sc.bound.cpu().numpy())
    assert 0 < want.sum() < R
    _same(o.effect.cpu().numpy(), eff)
    _same(o.effect_counts.cpu().numpy(), cnt)
    _same(o.effect_passed.cpu().numpy(), want)
    _same(o.pvals_gated.cpu().numpy(), gated)


def test_cpu_tier_argument():
    cur, base = _pattern("random", 20, 21, 5)
    c, b = torch.from_numpy(cur), torch.from_numpy(base)
    with pytest.raises(ValueError):
        C.pairwise_effect(c, b, tier="nope")
    eff, cnt = ref.pairwise_effect(cur, base)
    r = C.pairwise_effect(c, b, GATES[1], tier="wide")
    _same(r.effect.numpy(), eff)
    _same(r.counts.numpy(), cnt)
    _same(r.passed.numpy(), ref.effect_gate(eff, None, 0.3, 0.0, 0.0, False))
