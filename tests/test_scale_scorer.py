"""CanaryScorer with the pairwise scale test (K27): for the mean/std, robust
and band-mix models, ``score`` in every eager mode and ``score_resident`` over
a small static store.

With the test on, the p-values and statistics are what the tests computed,
``diff`` is the op-by-op composition -- the tests' verdict, AND the effect gate
where it is on, OR the scale verdict -- and the decision equals that of a scorer
without the test over inputs whose baselines were replaced so that the location
tests alone give that verdict (a copy of the current window: no difference; the
current window moved far away: every test differs).  With the test off -- by
default, or ``OFF`` -- nothing changes and no scale output exists.  The
captured / raw-pointer paths refuse a scorer with the test on."""
import numpy as np
import pytest
import torch

from foremast_amd.engine.resident import ResidentHistory
from foremast_amd.engine.scorer import CanaryScorer
from foremast_amd.ops import canary as C
from foremast_amd.ops import reference as ref

from test_effect_scorer import ALIASES, DECISION, S, T, N, _cfg, _same

MA, ROBUST, MIX = "moving_average_all", "robust_moving_average_all", "band_mix"
ON = dict(pairwise_scale_test="BROWN_FORSYTHE")
GATE = dict(pairwise_min_shift=0.02)
SHIFT = np.array([0.0, 1.5, 0.0, 1.5], np.float32)       # per row class, level 100: 1.5 % of the baseline median
SPREAD = np.array([1.0, 1.0, 3.0, 3.0], np.float32)      # class 2: the spread alone; class 3: both


def _mk(aliases, device, mode, model, **kw):
    extra = dict(codes=tuple((2, 1, 0)[m % 3] for m in range(len(aliases)))) if model == MIX else {}
    return CanaryScorer(aliases, _cfg(**kw), device, mode=mode, model=model, **extra)


def _inputs(M, model):
    """History N(100, 3); baseline 100 + 0.5 N(0, 1); current = the row's own
    baseline samples reordered, spread about 100 by the class factor, plus the
    class shift.  Class 0 is never "different"; class 1 differs in level only
    (every location p-value tiny, the shift under the 2 % gate); class 2 has the
    baseline's centre and three times its spread (the location tests see
    nothing); class 3 both.  One current point per row sits at 0.9 thresholds
    from the band centre, on the judged side: anomalous exactly when the row's
    threshold was lowered; every other point stays inside the lowered band."""
    rng = np.random.default_rng(200 + M)
    R = S * M
    hist = (100 + 3 * rng.standard_normal((R, T))).astype(np.float32)
    base = (100 + 0.5 * rng.standard_normal((R, N))).astype(np.float32)
    cls = (np.arange(R) + 2 * (np.arange(R) // M)) % 4        # every class meets every metric
    cur = np.stack([b[rng.permutation(N)] for b in base])
    cur = (100 + SPREAD[cls][:, None] * (cur - 100) + SHIFT[cls][:, None]).astype(np.float32)
    sc = _mk(ALIASES[:M], "cpu", None, model)
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
        rows = prow[np.random.default_rng(3).permutation(R + 2)[:R]]
        store.write_static(rows, list(hist), np.zeros(R))
        rm = torch.from_numpy(rows.astype(np.int32)).to(device)
        o = sc.score_resident(store.view(), rm, c, b)
        o2 = sc.score_resident(store.view(), rm, c, b)        # all hits
        assert o2.packed.cpu().equal(o.packed.cpu())
    if device != "cpu":
        torch.cuda.synchronize()
    g = lambda t: None if t is None else t.detach().cpu().numpy().copy()
    d = o.decide
    return dict(pvals=g(o.pvals), pstats=g(o.pstats), diff=g(o.diff), stats=g(d.stats), flags=g(d.flags),
                count=g(d.count), score=g(d.score), valid=g(d.valid), packed=g(o.packed), effect=g(o.effect),
                effect_passed=g(o.effect_passed), scale=g(o.scale), scale_diff=g(o.scale_diff),
                pvals_scaled=g(o.pvals_scaled))


def _check(device, model, mode, kind, M, gate=False):
    aliases = ALIASES[:M]
    hist, base, cur, cls = _inputs(M, model)
    R = S * M
    g = GATE if gate else {}
    mk = lambda **kw: _mk(aliases, device, mode, model, **kw)
    on = _tick(mk(**ON, **g), kind, hist, base, cur, device)
    off = _tick(mk(**g), kind, hist, base, cur, device)
    named_off = _tick(mk(pairwise_scale_test="OFF", **g), kind, hist, base, cur, device)
    # test off: by default and by name the same arrays, no scale output
    assert off["scale"] is None and off["scale_diff"] is None and off["pvals_scaled"] is None
    assert named_off["scale"] is None
    _same(off, named_off, DECISION + ("pvals", "pstats"))
    # test on: the tests' own numbers stay
    _same(on, off, ("pvals", "pstats", "effect", "effect_passed"))
    want_scale = ref.pairwise_scale(cur, base, 20)
    flagged = ref.scale_verdict(want_scale, 0.05)
    with np.errstate(invalid="ignore"):
        assert not (np.abs(want_scale[:, 1] - np.float32(0.05)) <= 1e-3 * 0.05).any()
    if device == "cpu":
        np.testing.assert_array_equal(on["scale"], want_scale)
    else:
        np.testing.assert_array_equal(on["scale"][:, 3:], want_scale[:, 3:])
        np.testing.assert_allclose(on["scale"][:, [0, 2]], want_scale[:, [0, 2]], rtol=1e-5, atol=1e-5)
        np.testing.assert_allclose(on["scale"][:, 1], want_scale[:, 1], rtol=2e-4, atol=2e-6)
    np.testing.assert_array_equal(on["scale_diff"], flagged)
    # what the fixture is for
    mask, anyc = C.PairwiseConfig("ALL").mask_and_combine()
    _, _, loc = ref.pairwise_tests(cur, base, mask, anyc, 0.05, 20, 20, 5)
    np.testing.assert_array_equal(loc, np.isin(cls, (1, 3)).astype(np.int8))
    np.testing.assert_array_equal(flagged, np.isin(cls, (2, 3)).astype(np.int8))
    if gate:
        eff, _ = ref.pairwise_effect(cur, base)
        passed = ref.effect_gate(eff, None, 0.0, 0.02, 0.0, False)
        assert not passed[np.isin(cls, (1, 3))].any()             # the gate clears every 1.5 % shift ...
        np.testing.assert_array_equal(off["diff"], np.zeros(R, np.int8))
        loc = loc & passed
    else:
        np.testing.assert_array_equal(off["diff"], loc)
    want = loc | flagged                                           # ... and never a scale verdict
    np.testing.assert_array_equal(on["diff"], want)
    assert (on["diff"] != off["diff"]).any()
    # the p-values the decision read
    src = off["pvals"] if not gate else np.where(passed[:, None] != 0, off["pvals"], np.float32(np.nan))
    np.testing.assert_array_equal(on["pvals_scaled"], np.where(flagged[:, None] != 0, np.float32(0), src))
    # the decision: a tick without the test (and the gate) whose location tests give `want`
    base2 = np.where(want[:, None] != 0, cur - np.float32(50), cur).astype(np.float32)
    exp = _tick(_mk(aliases, device, mode, model), kind, hist, base2, cur, device)
    np.testing.assert_array_equal(exp["diff"], want)
    _same(on, exp, DECISION)
    if model != MIX:
        # the point at 0.9 thresholds is anomalous exactly where the threshold was lowered
        np.testing.assert_array_equal(on["count"], on["diff"].astype(np.int32))
        np.testing.assert_array_equal(off["count"], off["diff"].astype(np.int32))
    else:
        assert (on["count"] != off["count"]).any()
    return on


@pytest.mark.parametrize("gate", [False, True])
@pytest.mark.parametrize("M", [8, 3])
@pytest.mark.parametrize("kind", ["score", "resident"])
@pytest.mark.parametrize("model", [MA, ROBUST, MIX])
def test_cpu_scorer_with_the_scale_test(model, kind, M, gate):
    _check("cpu", model, None, kind, M, gate)


def test_scale_scorer_without_baseline_has_no_scale_outputs():
    hist, base, cur, _ = _inputs(3, MA)
    for model in (MA, ROBUST, MIX):
        a = _mk(ALIASES[:3], "cpu", None, model, **ON).score(torch.from_numpy(hist), None, torch.from_numpy(cur), T)
        b = _mk(ALIASES[:3], "cpu", None, model).score(torch.from_numpy(hist), None, torch.from_numpy(cur), T)
        assert a.scale is None and a.scale_diff is None and a.pvals_scaled is None
        assert torch.equal(a.packed, b.packed) and torch.equal(a.decide.count, b.decide.count)


def test_captured_paths_refuse_the_scale_test():
    """They raise before touching a tensor, on any device."""
    with pytest.raises(ValueError, match="scale test"):
        CanaryScorer(ALIASES[:3], _cfg(**ON), "cpu", mode="fused")
    CanaryScorer(ALIASES[:3], _cfg(pairwise_scale_test="off"), "cpu", mode="fused")
    sc = CanaryScorer(ALIASES[:3], _cfg(pairwise_scale_test="levene"), "cpu")
    assert sc.scale.enabled and not sc.gate.enabled
    x = torch.zeros((3, 8))
    for name in ("capture", "capture_front", "split_launchers", "front_only"):
        with pytest.raises(ValueError, match="scale test"):
            getattr(sc, name)(x, x, x)
    with pytest.raises(ValueError):
        CanaryScorer(ALIASES[:3], _cfg(pairwise_scale_test="MOOD"), "cpu")
    with pytest.raises(ValueError):
        CanaryScorer(ALIASES[:3], _cfg(**ON, pairwise_scale_min_ratio=0.5), "cpu")


# ---------------------------------------------------------------------- GPU
@pytest.mark.gpu
@pytest.mark.parametrize("M,gate", [(8, False), (3, True)])
@pytest.mark.parametrize("kind", ["score", "resident"])
@pytest.mark.parametrize("model,mode", [(MA, "front"), (MA, "overlap"), (MA, "serial"), (ROBUST, None), (MIX, None)])
def test_gpu_scorer_with_the_scale_test(cuda, model, mode, kind, M, gate):
    on = _check(cuda, model, mode, kind, M, gate)
    cpu = _check("cpu", model, None, kind, M, gate)
    _same(on, cpu, ("diff", "flags", "count", "valid", "scale_diff"))
    # (pvals_scaled is each device's own p-values with the flagged rows at 0: checked against those in _check)
    np.testing.assert_array_equal(on["pvals_scaled"] == 0, cpu["pvals_scaled"] == 0)
    np.testing.assert_array_equal(on["packed"][:, [0, 2, 3]], cpu["packed"][:, [0, 2, 3]])
    np.testing.assert_allclose(on["stats"], cpu["stats"], rtol=2e-5, atol=1e-5)


@pytest.mark.gpu
def test_gpu_captured_paths_unchanged_without_the_scale_test(cuda):
    M = 3
    hist, base, cur, _ = _inputs(M, MA)
    h, b, c = (torch.from_numpy(a).to(cuda) for a in (hist, base, cur))
    sc = CanaryScorer(ALIASES[:M], _cfg(), cuda)
    want = sc.score(h, b, c, T).packed.clone()
    front, decide, o = sc.split_launchers(h, b, c, T, slot=2)
    front(); decide()
    torch.cuda.synchronize()
    assert torch.equal(o.packed, want) and o.scale is None
    out = CanaryScorer(ALIASES[:M], _cfg(), cuda).capture(h, b, c, T)()
    torch.cuda.synchronize()
    assert torch.equal(out.packed, want)
