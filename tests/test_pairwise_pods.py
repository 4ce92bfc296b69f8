"""K29 (csrc/kernels/pairwise_pods.hip) against the numpy definition
``reference.pairwise_pods`` / ``pods_verdict`` (docs/BRAIN_SPEC.md 4.3): both
tiers at their edge shapes, every kind of content in one batch per shape.

The integers (counts, doubled rank sums, tie term, k) and the NaN / -1
placement compare exactly; H and the z to 1e-5 relative and the p-values to
2e-4 relative (the finishing arithmetic runs in another order; the tolerances
of the scale test, BRAIN_SPEC 4.2).  ``worst`` and ``pod_diff`` compare on
every row, which needs a reference whose two largest |z| differ by more than
1e-6 relative and whose p-values keep 2e-4 relative off the threshold: asserted
on the reference, and the seeds below are the first that meet it."""
import numpy as np
import pytest
import torch

from foremast_amd.ops import canary as C
from foremast_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
TEST = C.PodTest("KRUSKAL_DUNN", 0.05, 5)
UNEVEN = [0, 4, 5, 0] + [12] * 55 + [11] * 5
# (pod lengths, baseline length, seed)
SHAPES = {
    "wave-5+5": ([5, 5], 10, 0),
    "wave-64": ([10, 12, 10], 32, 0),
    "wave-65": ([10, 12, 11], 32, 0),
    "wave-1024-uneven": (UNEVEN, 300, 0),
    "wide-1025": ([300, 213], 512, 0),
    "wide-64x64": ([64] * 64, 4096, 0),
    "wide-8191+1": ([8191, 0], 1, 0),          # one LDS side of 8,192: an empty second pod, so k < 2
    "wide-2x2000": ([2000, 2000], 4192, 0),
}
KINDS = ("normal", "shifted", "ties", "specials", "equal", "nobase")


def _batch(lens, nb, seed):
    """One row per kind: (cur [6, n], seg_end [6, G] int32, base [6, nb])."""
    rng = np.random.default_rng(seed)
    seg = np.cumsum(lens)
    n = int(seg[-1])
    cur, base = np.empty((len(KINDS), n), np.float32), np.empty((len(KINDS), nb), np.float32)
    for i, kind in enumerate(KINDS):
        c, b = rng.normal(100, 5, n), rng.normal(100, 5, nb)
        if kind == "ties":
            c, b = rng.integers(0, 4, n).astype(float), rng.integers(0, 4, nb).astype(float)
        if kind in ("shifted", "specials"):
            c[seg[-2]:] += 10.0                                # the last pod, 2 sigma
        if kind == "specials":
            c[::7], c[3::11], c[5::13], c[1::17], c[2::17] = np.nan, np.inf, -np.inf, -0.0, 0.0
            c[seg[0] - 1:seg[0] + 1] = np.nan                  # across a pod boundary
            b[::5], b[1::9], b[2::9] = np.nan, -0.0, 0.0
        if kind == "equal":
            c[:], b[:] = 7.0, 7.0
        if kind == "nobase":
            b[:] = np.nan
        cur[i], base[i] = c, b
    return cur, np.tile(seg.astype(np.int32), (len(KINDS), 1)), base


def _check(got: C.PodResult, want, thr=TEST.p_threshold):
    pods, pod_z, pod_n, pod_rank2, base_rank2, tie = want
    # the precondition of comparing worst and pod_diff, on the reference
    az = np.sort(np.nan_to_num(np.abs(pod_z.astype(np.float64)), nan=-1.0), axis=1)
    if az.shape[1] >= 2:
        assert (az[:, -1] - az[:, -2] > 1e-6 * az[:, -1])[pods[:, 4] >= 0].all()
    p = pods[:, [1, 3]].astype(np.float64)
    assert not (np.abs(p - thr) <= 2e-4 * thr).any()
    g = [t.cpu().numpy() for t in got.tensors()]
    for a, b in zip(g[2:6], (pod_n, pod_rank2, base_rank2, tie)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(g[0][:, 4:], pods[:, 4:])                       # worst, k
    np.testing.assert_array_equal(np.isnan(g[0]), np.isnan(pods))
    np.testing.assert_array_equal(np.isnan(g[1]), np.isnan(pod_z))
    np.testing.assert_allclose(g[0][:, [0, 2]], pods[:, [0, 2]], rtol=1e-5, atol=0)
    np.testing.assert_allclose(g[1], pod_z, rtol=1e-5, atol=0)
    np.testing.assert_allclose(g[0][:, [1, 3]], pods[:, [1, 3]], rtol=2e-4, atol=0)
    np.testing.assert_array_equal(g[6], ref.pods_verdict(pods, thr))


@pytest.mark.parametrize("name", list(SHAPES))
def test_pods_kernel_matches_definition(cuda, name):
    cur, seg, base = _batch(*SHAPES[name])
    want = ref.pairwise_pods(cur, seg, base, TEST.min_points)
    C.reset_pod_route_rows()
    t = lambda a: torch.from_numpy(a).to(cuda)  # noqa: E731
    _check(C.pairwise_pods(t(cur), t(seg), t(base), TEST), want)
    assert C.pod_route_rows()[name.split("-")[0]] == len(KINDS)
    if name == "wave-64":
        _check(C.pairwise_pods(t(cur), t(seg), t(base), TEST, tier="wide"), want)


def test_pods_padded_batch_routes_by_row(cuda):
    """Rows of a batch padded to 9,000 columns go down the route their own width asks for."""
    parts = [_batch(*SHAPES[k]) for k in ("wave-65", "wide-2x2000")] + [_batch([4500, 4400], 100, 0)]
    rows = sum(len(p[0]) for p in parts)
    cur, base = np.full((rows, 9000), np.nan, np.float32), np.full((rows, 4192), np.nan, np.float32)
    seg = np.zeros((rows, 3), np.int32)
    r = 0
    for c, s, b in parts:
        k = len(c)
        cur[r:r + k, :c.shape[1]], base[r:r + k, :b.shape[1]] = c, b
        seg[r:r + k] = np.pad(s, ((0, 0), (0, 3 - s.shape[1])), mode="edge")
        r += k
    C.reset_pod_route_rows()
    t = lambda a: torch.from_numpy(a).to(cuda)  # noqa: E731
    _check(C.pairwise_pods(t(cur), t(seg), t(base), TEST), ref.pairwise_pods(cur, seg, base, TEST.min_points))
    # the rows without one finite sample ("specials" keeps some) are as narrow as a row gets: none here
    assert C.pod_route_rows() == {"wave": len(KINDS), "wide": len(KINDS), "host": len(KINDS)}


def test_pods_more_than_64_pod_columns(cuda):
    """G = 65: rows whose 65th pod is empty lose only that column; a row with 65 pods runs on the host."""
    cur, _, base = _batch([6] * 65, 60, 0)
    cur, base = cur[:3], base[:3]
    seg = np.tile(np.cumsum([6] * 65).astype(np.int32), (3, 1))
    seg[:2, 64] = seg[:2, 63]                                  # rows 0 and 1: the last six columns belong to no pod
    C.reset_pod_route_rows()
    t = lambda a: torch.from_numpy(a).to(cuda)  # noqa: E731
    _check(C.pairwise_pods(t(cur), t(seg), t(base), TEST), ref.pairwise_pods(cur, seg, base, TEST.min_points))
    assert C.pod_route_rows() == {"wave": 2, "wide": 0, "host": 1}
