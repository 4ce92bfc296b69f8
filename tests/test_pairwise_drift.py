"""K31 (csrc/kernels/pairwise_drift.hip) against the numpy definition
``reference.pairwise_drift`` / ``drift_verdict`` (docs/BRAIN_SPEC.md 4.5): every
wave-tier instance at its widest row and one column short of it, the workgroup
tier at each of its block sizes, every kind of content in one batch per shape.

The integers (S, P, Tx2, V18 per side, the pods' S and n, k) and the NaN
placement compare exactly; the z and tau to 1e-5 relative and the p-value to
2e-4 relative (the tolerances of the per-pod test, BRAIN_SPEC 4.3).
``drift_diff`` compares on every row, which needs a reference whose p-values
keep 2e-4 relative off the threshold and whose |tau_c| keep 1e-5 relative off
the floor: asserted on the reference."""
import numpy as np
import pytest
import torch

from foremast_amd.ops import canary as C
from foremast_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
TEST = C.DriftTest("MANN_KENDALL", 0.05, 10, 0.1)
# (pod lengths, columns of no pod after them, baseline length); 9 = one sample short of min_points
SHAPES = {
    "wave-64": ([10, 13, 9], 0, 32),
    "wave-63": ([10, 13, 9], 0, 31),
    "wave-128": ([9, 0, 30, 25], 0, 64),
    "wave-127": ([9, 0, 30, 25], 3, 60),
    "wave-256": ([100], 0, 156),                       # G = 1
    "wave-255": ([], 55, 200),                         # G = 0: no column of the window belongs to a pod
    "wave-512": ([5] * 60 + [11, 12, 13, 14], 0, 162),  # G = 64
    "wave-511": ([70, 130, 60], 0, 251),
    "wave-1024": ([1000], 0, 24),
    "wave-1023": ([333, 200, 90], 0, 400),
    "wide-1025": ([300, 213], 0, 512),                 # blocks of 64 columns
    "wide-2500": ([700, 333, 467], 0, 1000),           # blocks of 128
    "wide-8192": ([8000], 0, 192),                     # blocks of 256, one long pod
}
KINDS = ("ramp", "creep", "ties", "monotone", "flat")


def _batch(lens, tail, nb, seed=0):
    """One row per kind: (cur [5, n], seg_end [5, G] int32, base [5, nb])."""
    rng = np.random.default_rng(seed)
    seg = np.cumsum(lens).astype(np.int32)
    n = int(seg[-1]) + tail if len(lens) else tail
    lo = np.concatenate([[0], seg[:-1]]) if len(lens) else seg
    cur, base = np.empty((len(KINDS), n), np.float32), np.empty((len(KINDS), nb), np.float32)
    for i, kind in enumerate(KINDS):
        c, b = rng.normal(100, 5, n), rng.normal(100, 5, nb)
        if kind == "ramp":                                     # the same ramp on both sides
            c, b = c + np.arange(n) * (10.0 / max(n, 1)), b + np.arange(nb) * (10.0 / nb)
        if kind == "creep":                                    # every pod creeps upward, with holes
            for a, e in zip(lo, seg):
                c[a:e] += np.linspace(0, 15, e - a)
            c[::7], c[3::11], c[5::13] = np.nan, np.inf, -np.inf
            if len(lens):
                c[max(seg[0] - 1, 0):seg[0] + 1] = np.nan      # across a pod boundary
            b[::5], b[1::9] = np.nan, np.inf
        if kind == "ties":                                     # four levels, -0.0 and 0.0 among them
            lv = np.array([-1.0, -0.0, 0.0, 2.0])
            c, b = lv[rng.integers(0, 4, n)], lv[rng.integers(0, 4, nb)]
            c[2::9], b[4::9] = np.nan, -np.inf
        if kind == "monotone":                                 # S == -P in the longest pod; a constant baseline
            if len(lens):
                g = int(np.argmax(lens))
                c[lo[g]:seg[g]] = -np.arange(lens[g])
            b[:] = 7.0
        if kind == "flat":                                     # a constant current side: not applicable
            c[:] = 7.0
        cur[i], base[i] = c, b
    return cur, np.tile(seg, (len(KINDS), 1)), base


def _check(got: C.DriftResult, want, test=TEST):
    drift, counts, pod_S, pod_n, k = want
    # the precondition of comparing drift_diff, on the reference
    p, tau = drift[:, 1].astype(np.float64), np.abs(drift[:, 3].astype(np.float64))
    assert not (np.abs(p - test.p_threshold) <= 2e-4 * test.p_threshold).any()
    assert not (np.abs(tau - test.min_tau) <= 1e-5 * test.min_tau).any()
    g = [t.cpu().numpy() for t in got.tensors()]
    for a, b in zip(g[1:5], (counts, pod_S, pod_n, k)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(np.isnan(g[0]), np.isnan(drift))
    np.testing.assert_allclose(g[0][:, [0, 2, 3, 4, 5]], drift[:, [0, 2, 3, 4, 5]], rtol=1e-5, atol=0)
    np.testing.assert_allclose(g[0][:, 1], drift[:, 1], rtol=2e-4, atol=0)
    np.testing.assert_array_equal(g[5], ref.drift_verdict(drift, test.p_threshold, test.min_tau))


@pytest.mark.parametrize("name", list(SHAPES))
def test_drift_kernel_matches_definition(cuda, name):
    cur, seg, base = _batch(*SHAPES[name])
    want = ref.pairwise_drift(cur, seg, base, TEST.min_points)
    lens = SHAPES[name][0]
    if lens:                    # the batch holds what it is meant to: the monotone pod, verdicts both ways
        g, n = int(np.argmax(lens)), max(lens)
        assert want[2][3, g] == -(n * (n - 1) // 2)
        assert set(ref.drift_verdict(want[0], TEST.p_threshold, TEST.min_tau)) == {0, 1}
    C.reset_drift_route_rows()
    t = lambda a: torch.from_numpy(a).to(cuda)  # noqa: E731
    _check(C.pairwise_drift(t(cur), t(seg), t(base), TEST), want)
    assert C.drift_route_rows()[name.split("-")[0]] == len(KINDS)
    if name.startswith("wave"):
        _check(C.pairwise_drift(t(cur), t(seg), t(base), TEST, tier="wide"), want)


def test_drift_padded_batch_routes_by_row(cuda):
    """Rows of a batch padded to 9,000 columns and 65 pod columns go down the
    route their own width and pods ask for: a row really wider than 8,192 and
    a row with 65 non-empty pods run the definition on the host."""
    parts = [_batch(*SHAPES[k]) for k in ("wave-127", "wide-2500")]
    parts += [tuple(a[1:2] for a in _batch([4500, 4400], 0, 100)), tuple(a[1:2] for a in _batch([12] * 65, 0, 60))]
    rows = sum(len(p[0]) for p in parts)
    cur, base = np.full((rows, 9000), np.nan, np.float32), np.full((rows, 1000), np.nan, np.float32)
    seg = np.zeros((rows, 65), np.int32)
    r = 0
    for c, s, b in parts:
        k = len(c)
        cur[r:r + k, :c.shape[1]], base[r:r + k, :b.shape[1]] = c, b
        seg[r:r + k] = np.pad(s, ((0, 0), (0, 65 - s.shape[1])), mode="edge")
        r += k
    C.reset_drift_route_rows()
    t = lambda a: torch.from_numpy(a).to(cuda)  # noqa: E731
    _check(C.pairwise_drift(t(cur), t(seg), t(base), TEST), ref.pairwise_drift(cur, seg, base, TEST.min_points))
    assert C.drift_route_rows() == {"wave": len(KINDS), "wide": len(KINDS), "host": 2}
