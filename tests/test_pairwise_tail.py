"""K32 (csrc/kernels/pairwise_tail.hip) against the numpy definition
``reference.pairwise_tail`` / ``tail_verdict`` (docs/BRAIN_SPEC.md 4.6): every
wave-tier instance at its widest row and one column short of it, the workgroup
tier at 1,025, 2,500 and 8,192 pooled columns, every kind of content in one
batch per shape, bound codes 1, 2, 3 cycling over the rows.

The integers (a, b, k per side and level, n, J, which), the NaN placement and
the threshold compare exactly; p, p_min and the excess to 1e-5 relative (fp64
statistics stored as fp32; device and definition share the log-factorial table
and differ by the rounding of ``exp`` and the order of the sum).  ``tail_diff``
compares on every row, which needs a reference whose p-values keep 1e-5
relative off the threshold and stay above 1e-30, whose excesses keep 1e-5
relative off the floor, and both verdicts in every batch: asserted on the
reference."""
import numpy as np
import pytest
import torch

from foremast_amd.ops import canary as C
from foremast_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
TEST = C.TailTest("EXCEEDANCE", 0.05, (0.9, 0.95, 0.99), "BOUND", 12, 5, 0.02)
BOUND = np.array([1, 2, 3], np.int32)
# (current columns, baseline columns); 12 = exactly min_points
SHAPES = {
    "wave-64": (12, 52), "wave-63": (23, 40), "wave-128": (64, 64), "wave-127": (27, 100), "wave-256": (40, 216),
    "wave-255": (128, 127), "wave-512": (112, 400), "wave-511": (300, 211), "wave-1024": (128, 896),
    "wave-1023": (512, 511), "wide-1025": (12, 1013), "wide-2500": (500, 2000), "wide-8192": (1024, 7168),
}
KINDS = ("stretched", "collapsed", "clean", "zeros", "holes", "constant", "separated")


def _batch(nc, nb, seed=0):
    """One row per kind: (cur [7, nc], base [7, nb]); row r is judged by bound code BOUND[r % 3]."""
    rng = np.random.default_rng(seed)
    cur, base = np.empty((len(KINDS), nc), np.float32), np.empty((len(KINDS), nb), np.float32)
    for i, kind in enumerate(KINDS):
        c, b = rng.lognormal(4, 0.3, nc), rng.lognormal(4, 0.3, nb)
        if kind == "stretched":                                # the upper fifth moves out (upper side only: code 1)
            c = np.where(c > np.quantile(c, 0.8), c * (1 + min(0.3, 2.5 / np.sqrt(nc))), c)
        if kind == "collapsed":                                # the lower fifth collapses (lower side only: code 2)
            c = np.where(c < np.quantile(c, 0.2), c * (1 - min(0.3, 2.5 / np.sqrt(nc))), c)
        if kind == "clean":                                    # H0 with holes on both sides (both sides: code 3)
            c[::7], b[3::11], b[5::13] = np.nan, np.inf, -np.inf
        if kind == "zeros":                                    # 96 % zeros of both signs: two thresholds inside the run
            for x in (c, b):
                at = rng.permutation(len(x))[len(x) // 25:]
                x[at] = np.copysign(0.0, rng.standard_normal(len(at)))
        if kind == "holes":                                    # the current side one sample short of min_points
            c[rng.permutation(nc)[TEST.min_points - 1:]] = np.nan
            b[::5], b[1::9] = np.nan, -np.inf
        if kind == "constant":                                 # m = 0 at every level: J = 0
            c[:], b[:] = 7.0, 7.0
        if kind == "separated":                                # min_points current samples, all above the baseline
            c = b.max() + 1 + rng.random(nc)
            c[rng.permutation(nc)[TEST.min_points:]] = np.nan
        cur[i], base[i] = c, b
    return cur, base


def _check(got: C.TailResult, want, test=TEST):
    tail, which, J, n, counts = want
    diff = ref.tail_verdict(tail, test.p_threshold, test.min_excess)
    # the preconditions of comparing tail_diff, on the reference
    p, ex = tail[:, 0].astype(np.float64), tail[:, 2].astype(np.float64)
    assert not (np.abs(p - test.p_threshold) <= 1e-5 * test.p_threshold).any()
    assert not (np.abs(ex - test.min_excess) <= 1e-5 * test.min_excess).any()
    assert not (tail[:, :2] < 1e-30).any() and set(diff) == {0, 1}
    g = [t.cpu().numpy() for t in got.tensors()]
    for a, b in zip(g[1:5], (which, J, n, counts)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(np.isnan(g[0]), np.isnan(tail))
    np.testing.assert_array_equal(g[0][:, 3], tail[:, 3])
    np.testing.assert_allclose(g[0][:, :3], tail[:, :3], rtol=1e-5, atol=0)
    np.testing.assert_array_equal(g[5], diff)


@pytest.mark.parametrize("name", list(SHAPES))
def test_tail_kernel_matches_definition(cuda, name):
    cur, base = _batch(*SHAPES[name])
    want = ref.pairwise_tail(cur, base, TEST.q_i, TEST.sides, BOUND[np.arange(len(cur)) % 3], TEST.min_points,
                             TEST.min_tail_points)
    # the batch holds what it is meant to: the zero-inflated row's first two levels in one run of ties (one test),
    # J = 0 on the constant row, a row short of min_points, and the separated row's current samples all beyond the
    # first threshold
    assert want[4][3, 0, 0, :2].sum() == want[4][3, 0, 1, :2].sum() and want[2][3] <= 2
    assert want[2][5] == 0 and want[3][4, 0] == TEST.min_points - 1 and np.isnan(want[0][[4, 5]]).all()
    assert want[4][6, 0, 0, 0] == min(TEST.min_points, want[4][6, 0, 0, :2].sum())
    C.reset_tail_route_rows()
    t = lambda a: torch.from_numpy(a).to(cuda)  # noqa: E731
    _check(C.pairwise_tail(t(cur), t(base), TEST, t(BOUND), 3), want)
    assert C.tail_route_rows()[name.split("-")[0]] == len(KINDS)
    if name.startswith("wave"):
        _check(C.pairwise_tail(t(cur), t(base), TEST, t(BOUND), 3, tier="wide"), want)
        assert C.tail_route_rows() == {"wave": len(KINDS), "wide": len(KINDS), "host": 0}


def test_tail_padded_batch_routes_by_row(cuda):
    """Rows of a batch padded to 9,000 columns go down the route their own
    width asks for; a row really wider than 8,192 runs the definition on the
    host."""
    parts = [_batch(*SHAPES[k]) for k in ("wave-127", "wide-2500")] + [tuple(a[:1] for a in _batch(4500, 4400))]
    rows = sum(len(p[0]) for p in parts)
    cur, base = np.full((rows, 9000), np.nan, np.float32), np.full((rows, 4500), np.nan, np.float32)
    r = 0
    for c, b in parts:
        cur[r:r + len(c), :c.shape[1]], base[r:r + len(c), :b.shape[1]] = c, b
        r += len(c)
    want = ref.pairwise_tail(cur, base, TEST.q_i, TEST.sides, BOUND[np.arange(rows) % 3], TEST.min_points,
                             TEST.min_tail_points)
    C.reset_tail_route_rows()
    t = lambda a: torch.from_numpy(a).to(cuda)  # noqa: E731
    _check(C.pairwise_tail(t(cur), t(base), TEST, t(BOUND), 3), want)
    assert C.tail_route_rows() == {"wave": len(KINDS), "wide": len(KINDS), "host": 1}
