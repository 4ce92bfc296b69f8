"""CanaryScorer with the pairwise effect gate (K19): for both models, ``score``
in every eager mode and ``score_resident`` over a small static store.

With the gate on, the p-values and statistics are what the tests computed,
``diff`` is the ungated verdict AND the gate, and the decision equals that of an
ungated scorer over inputs in which the failing rows' baselines were replaced
by their own current windows (so their tests see no difference).  With the gate
off -- by default or with explicit zeros -- nothing changes and no effect
output exists.  The captured / raw-pointer paths refuse a gated scorer."""
import numpy as np
import pytest
import torch

from foremast_amd.config import BrainConfig, MetricRule
from foremast_amd.engine.resident import ResidentHistory
from foremast_amd.engine.scorer import CanaryScorer
from foremast_amd.ops import reference as ref

MA, ROBUST = "moving_average_all", "robust_moving_average_all"
ALIASES = ["err", "lat", "low", "cpu_x", "m4", "lat2", "low2", "m7"]     # bound codes 1 3 2 1 1 3 2 1
S, T, N = 9, 64, 50                                                       # 10 points x 5 pods per side
SHIFT = np.array([0.0, 1.0, 3.0, -3.0], np.float32)                       # per row class, level 100


def _cfg(**kw):
    c = BrainConfig(threshold=3.0, bound=1, **kw)
    c.metric_rules = {"lat": MetricRule(4.0, 3, 0.0), "low": MetricRule(4.0, 2, 0.0)}
    return c


GATE = dict(pairwise_min_shift=0.02, pairwise_directional=True)
ZEROS = dict(pairwise_min_effect=0.0, pairwise_min_shift=0.0, pairwise_min_shift_abs=0.0, pairwise_directional=False)


def _inputs(M, model):
    """History N(100, 3); baseline 100 + 0.1 N(0, 1); current = the row's own
    baseline samples reordered, plus the class shift: class 0 has the same
    multiset on both sides but for one point (never "different"), the others
    differ by >= 10 sigma (every p-value tiny: no verdict near the p
    threshold).  Shift +1 is 1 % of the baseline median -- under the 2 % gate;
    -3 passes the size gate and fails the direction on upper-only metrics, +3
    on lower-only ones.  Every shifted window stays inside the lowered band
    (>= 0.8 * 3 * ~3 wide); one current point per row sits at 0.9 thresholds
    from the band centre, on the judged side: anomalous exactly when the row's
    threshold was lowered."""
    rng = np.random.default_rng(100 + M)
    R = S * M
    hist = (100 + 3 * rng.standard_normal((R, T))).astype(np.float32)
    base = (100 + 0.1 * rng.standard_normal((R, N))).astype(np.float32)
    cls = (np.arange(R) + 2 * (np.arange(R) // M)) % 4        # every class meets every metric
    cur = np.stack([b[rng.permutation(N)] for b in base]) + SHIFT[cls][:, None]
    cur = cur.astype(np.float32)
    sc = CanaryScorer(ALIASES[:M], _cfg(), "cpu", model=model)
    st = sc.score(torch.from_numpy(hist), None, torch.from_numpy(cur), T).decide.stats.numpy()
    rules = [sc.cfg.rule_for(ALIASES[r % M]) for r in range(R)]
    thr = np.array([r.threshold for r in rules], np.float32)
    side = np.array([-1.0 if r.bound == 2 else 1.0 for r in rules], np.float32)
    cur[:, 3] = st[:, 0] + side * 0.9 * thr * st[:, 1]
    return hist, base, cur, cls


def _tick(sc, kind, hist, base, cur, device):
    h, b, c = (torch.from_numpy(a).to(device) for a in (hist, base, cur))
    if kind == "score":
        o = sc.score(h, b, c, T)
    else:
        R = hist.shape[0]
        store = ResidentHistory(T, device)
        prow, _ = store.rows_for([("k", i) for i in range(R + 2)], owner=("ns", "app"))
        pick = np.random.default_rng(3).permutation(R + 2)[:R]
        rows = prow[pick]
        store.write_static(rows, list(hist), np.zeros(R))
        o = sc.score_resident(store.view(), torch.from_numpy(rows.astype(np.int32)).to(device), c, b)
        o2 = sc.score_resident(store.view(), torch.from_numpy(rows.astype(np.int32)).to(device), c, b)   # all hits
        assert o2.packed.cpu().equal(o.packed.cpu())
    if device != "cpu":
        torch.cuda.synchronize()
    g = lambda t: None if t is None else t.detach().cpu().numpy().copy()
    d = o.decide
    return dict(pvals=g(o.pvals), pstats=g(o.pstats), diff=g(o.diff), stats=g(d.stats), flags=g(d.flags),
                count=g(d.count), score=g(d.score), valid=g(d.valid), packed=g(o.packed), effect=g(o.effect),
                effect_counts=g(o.effect_counts), effect_passed=g(o.effect_passed))


DECISION = ("diff", "stats", "flags", "count", "score", "valid", "packed")


def _same(a, b, keys):
    for k in keys:
        np.testing.assert_array_equal(a[k], b[k], err_msg=k)      # (NaN == NaN here)


def _check(device, model, mode, kind, M):
    aliases = ALIASES[:M]
    hist, base, cur, cls = _inputs(M, model)
    R = S * M
    mk = lambda **kw: CanaryScorer(aliases, _cfg(**kw), device, mode=mode, model=model)
    on = _tick(mk(**GATE), kind, hist, base, cur, device)
    off = _tick(mk(), kind, hist, base, cur, device)
    zero = _tick(mk(**ZEROS), kind, hist, base, cur, device)
    # gate off: by default and with explicit zeros the same arrays, no effect output
    assert off["effect"] is None and off["effect_counts"] is None and off["effect_passed"] is None
    assert zero["effect"] is None
    _same(off, zero, DECISION + ("pvals", "pstats"))
    # gate on: the tests' own numbers stay, the verdict is gated
    _same(on, off, ("pvals", "pstats"))
    eff, cnt = ref.pairwise_effect(cur, base)
    np.testing.assert_array_equal(on["effect"], eff)
    np.testing.assert_array_equal(on["effect_counts"], cnt)
    bound = np.array([_cfg().rule_for(aliases[r % M]).bound for r in range(R)])
    passed = ref.effect_gate(eff, bound, 0.0, 0.02, 0.0, True)
    np.testing.assert_array_equal(on["effect_passed"], passed)
    # what the fixture is for: ungated, exactly the shifted rows differ; the gate clears the 1 % rows and
    # the shifts that point away from a one-sided bound, and keeps the rest
    np.testing.assert_array_equal(off["diff"], (cls != 0).astype(np.int8))
    want = (cls == 2) & (bound != 2) | (cls == 3) & (bound != 1)
    np.testing.assert_array_equal(passed != 0, want)
    np.testing.assert_array_equal(on["diff"], off["diff"] & passed)
    assert on["diff"].any() and (on["diff"] != off["diff"]).any()
    # the decision: an ungated tick in which the failing rows' baselines are their own current windows
    base2 = base.copy()
    base2[passed == 0] = cur[passed == 0]
    exp = _tick(mk(), kind, hist, base2, cur, device)
    _same(on, exp, DECISION)
    # the point at 0.9 thresholds is anomalous exactly where the threshold was lowered
    np.testing.assert_array_equal(on["count"], on["diff"].astype(np.int32))
    np.testing.assert_array_equal(off["count"], off["diff"].astype(np.int32))
    return on


@pytest.mark.parametrize("M", [8, 3])
@pytest.mark.parametrize("kind", ["score", "resident"])
@pytest.mark.parametrize("model", [MA, ROBUST])
def test_cpu_gated_scorer(model, kind, M):
    _check("cpu", model, None, kind, M)


def test_gated_scorer_without_baseline_has_no_effect_outputs():
    hist, base, cur, _ = _inputs(3, MA)
    for model in (MA, ROBUST):
        on = CanaryScorer(ALIASES[:3], _cfg(**GATE), "cpu", model=model)
        off = CanaryScorer(ALIASES[:3], _cfg(), "cpu", model=model)
        a = on.score(torch.from_numpy(hist), None, torch.from_numpy(cur), T)
        b = off.score(torch.from_numpy(hist), None, torch.from_numpy(cur), T)
        assert a.effect is None and a.effect_passed is None
        assert torch.equal(a.packed, b.packed) and torch.equal(a.decide.count, b.decide.count)


def test_captured_paths_refuse_the_gate():
    """They raise before touching a tensor, on any device."""
    with pytest.raises(ValueError, match="effect gate"):
        CanaryScorer(ALIASES[:3], _cfg(**GATE), "cpu", mode="fused")
    CanaryScorer(ALIASES[:3], _cfg(), "cpu", mode="fused")
    sc = CanaryScorer(ALIASES[:3], _cfg(pairwise_min_effect=0.2), "cpu")
    assert sc.gate.enabled
    x = torch.zeros((3, 8))
    for name in ("capture", "capture_front", "split_launchers", "front_only"):
        with pytest.raises(ValueError, match="effect gate"):
            getattr(sc, name)(x, x, x)
    with pytest.raises(ValueError):
        CanaryScorer(ALIASES[:3], _cfg(pairwise_min_effect=1.5), "cpu")


# ---------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("M", [8, 3])
@pytest.mark.parametrize("kind", ["score", "resident"])
@pytest.mark.parametrize("model,mode", [(MA, "front"), (MA, "overlap"), (MA, "serial"), (ROBUST, None)])
def test_gpu_gated_scorer(cuda, model, mode, kind, M):
    on = _check(cuda, model, mode, kind, M)
    cpu = _check("cpu", model, None, kind, M)
    _same(on, cpu, ("diff", "flags", "count", "valid", "effect", "effect_counts", "effect_passed"))
    np.testing.assert_array_equal(on["packed"][:, [0, 2, 3]], cpu["packed"][:, [0, 2, 3]])
    np.testing.assert_allclose(on["stats"], cpu["stats"], rtol=2e-5, atol=1e-5)


@pytest.mark.gpu
def test_gpu_captured_paths_unchanged_without_the_gate(cuda):
    M = 3
    hist, base, cur, _ = _inputs(M, MA)
    h, b, c = (torch.from_numpy(a).to(cuda) for a in (hist, base, cur))
    sc = CanaryScorer(ALIASES[:M], _cfg(), cuda)
    want = sc.score(h, b, c, T).packed.clone()
    o = sc.decide_only(c, sc.front_only(h, b, c, T, slot=1))
    torch.cuda.synchronize()
    assert torch.equal(o.packed, want) and o.effect is None
    front, decide, o = sc.split_launchers(h, b, c, T, slot=2)
    front(); decide()
    torch.cuda.synchronize()
    assert torch.equal(o.packed, want)
    replay, o = sc.capture_front(h, b, c, T, slot=3)
    replay()
    sc.decide_only(c, o)
    torch.cuda.synchronize()
    assert torch.equal(o.packed, want)
    out = CanaryScorer(ALIASES[:M], _cfg(), cuda).capture(h, b, c, T)()
    torch.cuda.synchronize()
    assert torch.equal(out.packed, want)
