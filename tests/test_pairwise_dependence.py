"""K33 (csrc/kernels/pairwise_dependence.hip) against the numpy definition
``reference.pairwise_dependence`` / ``dependence_verdict`` (docs/BRAIN_SPEC.md
4.7), every kind of content in one batch per shape.  Integers, NaN placement and
``dep_keep`` compare exactly; rho and the VIFs to 1e-5 relative plus 1e-6
absolute, z and z_adj to 1e-5 relative, p_adj to 2e-4 relative (K29 - K31's
tolerances); the reference's p-values keep 2e-4 relative off the threshold."""
import numpy as np
import pytest
import torch

from foremast_amd.ops import canary as C
from foremast_amd.ops import reference as ref

from test_dependence_ops import _ar1

pytestmark = pytest.mark.gpu
GATE = C.DependenceGate("RANK_ACF", 0.05, 8, 4)
# (pod lengths, baseline length, tier, L)
SHAPES = {
    "wave-10": ([5], 5, "auto", 8),                    # L_s = 1
    "wave-64": ([63], 1, "auto", 8),                   # n2 < 2: the gate does not apply
    "wave-65": ([64], 1, "auto", 8),
    "wave-127": ([13, 3, 21], 90, "auto", 8),          # a pod below min_points, pods with n_s / 4 < L
    "wave-511": ([70, 130, 60], 251, "auto", 16),      # sixteen lags
    "wave-1024": ([37] * 8, 728, "auto", 8),
    "wide-1024": ([37] * 8, 728, "wide", 8),
    "wide-1025": ([1000], 25, "auto", 8),
    "wide-8192": ([2048, 2048], 4096, "auto", 8),      # a pod boundary at a multiple of 64
    "wide-8192b": ([8191], 1, "auto", 8),
}
KINDS = ("noise", "ar", "anti", "ties", "constpod", "const", "nocur", "resplit", "unsorted")
G = 8


def _batch(lens, nb, seed=0):
    """One row per kind: (cur [9, n], seg_end [9, G] int32, base [9, nb])."""
    rng = np.random.default_rng(seed)
    n = sum(lens)
    ends = np.pad(np.cumsum(lens), (0, G - len(lens)), mode="edge")
    cur, base = np.empty((len(KINDS), n), np.float32), np.empty((len(KINDS), nb), np.float32)
    seg = np.tile(ends.astype(np.int32), (len(KINDS), 1))
    for i, kind in enumerate(KINDS):
        c, b = rng.normal(100, 5, n), rng.normal(100, 5, nb)
        if kind == "noise":                                    # gaps inside the pods: pairs break
            c[2::7], c[3::11], c[5::13] = np.nan, np.inf, -np.inf
            b[1::5] = np.nan
        if kind == "ar":                                       # strongly autocorrelated, shifted
            c, b = 100 + 5 * _ar1(rng, 0.95, (n,)) + 4, 100 + 5 * _ar1(rng, 0.95, (nb,))
        if kind == "anti":                                     # anticorrelated: the VIF floors at 1
            c = 100 + 5 * (-1.0) ** np.arange(n) + rng.normal(0, 0.5, n) + 1
            b = 100 + 5 * (-1.0) ** np.arange(nb) + rng.normal(0, 0.5, nb)
        if kind == "ties":                                     # four levels, -0.0 and 0.0 among them
            lv = np.array([-1.0, -0.0, 0.0, 2.0])
            c, b = lv[rng.integers(0, 4, n)], lv[rng.integers(0, 4, nb)]
            c[4::9] = np.nan
        if kind == "constpod":                                 # c0_s = 0 in the first pod
            c[:lens[0]] = 250.0
        if kind == "const":                                    # A = 0
            c[:], b[:] = 7.0, 7.0
        if kind == "nocur":                                    # an all-missing side
            c[:] = np.nan
        if kind == "resplit":                                  # a boundary at 64, an empty pod, a short one, a tail
            a = min(64, n // 2)
            seg[i] = np.maximum.accumulate(np.minimum([a, a, a + 3] + [n - n // 5] * (G - 3), n))
        if kind == "unsorted":                                 # ends that decrease, a negative one, one past n_cur
            seg[i] = [n // 2, n // 3, -3, n - n // 4, n // 5, n + 9] + [n - 1] * (G - 6)
        cur[i], base[i] = c, b
    return cur, seg, base


def _check(got: C.DependenceResult, want, gate=GATE):
    dep, rho, n, TA, kept, pairs = want
    assert not (np.abs(dep[:, 0].astype(np.float64) - gate.p_threshold) <= 2e-4 * gate.p_threshold).any()
    g = [t.cpu().numpy() for t in got.tensors()]
    for a, b in zip(g[2:6], (n, TA, kept, pairs)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(np.isnan(g[0]), np.isnan(dep))
    np.testing.assert_array_equal(g[0][:, 5], dep[:, 5])
    np.testing.assert_allclose(g[1], rho, rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(g[0][:, 3:5], dep[:, 3:5], rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(g[0][:, 1:3], dep[:, 1:3], rtol=1e-5, atol=0)
    np.testing.assert_allclose(g[0][:, 0], dep[:, 0], rtol=2e-4, atol=0)
    np.testing.assert_array_equal(g[6], ref.dependence_verdict(dep, gate.p_threshold))


@pytest.mark.parametrize("name", list(SHAPES))
def test_dependence_kernel_matches_definition(cuda, name):
    lens, nb, tier, L = SHAPES[name]
    gate = C.DependenceGate("RANK_ACF", 0.05, L, 4)
    cur, seg, base = _batch(lens, nb)
    want = ref.pairwise_dependence(cur, seg, base, L, gate.min_points)
    if nb >= 5:                 # the batch holds what it is meant to: an inflated and a floored VIF, both verdicts
        assert want[0][2, 3:5].max() == 1.0 and want[0][1, 3:5].max() > 1.5
        assert set(ref.dependence_verdict(want[0], gate.p_threshold)) == {0, 1}
    C.reset_dependence_route_rows()
    t = lambda a: torch.from_numpy(a).to(cuda)  # noqa: E731
    _check(C.pairwise_dependence(t(cur), t(seg), t(base), gate, tier=tier), want)
    assert C.dependence_route_rows()[name.split("-")[0]] == len(KINDS)


def test_dependence_padded_batch_routes_by_row(cuda):
    """Rows of a batch padded to 9,000 columns take the route of their own width; one really wider runs on the host."""
    parts = [_batch(*SHAPES[k][:2]) for k in ("wave-127", "wide-1025")]
    parts.append(tuple(a[1:2] for a in _batch([4500, 4400], 100)))
    rows = sum(len(p[0]) for p in parts)
    cur, base = np.full((rows, 9000), np.nan, np.float32), np.full((rows, 1000), np.nan, np.float32)
    seg = np.zeros((rows, G), np.int32)
    r = 0
    for c, s, b in parts:
        k = len(c)
        cur[r:r + k, :c.shape[1]], base[r:r + k, :b.shape[1]], seg[r:r + k] = c, b, s
        r += k
    C.reset_dependence_route_rows()
    t = lambda a: torch.from_numpy(a).to(cuda)  # noqa: E731
    buf = C.alloc_dependence(rows, cuda)
    C.pairwise_dependence(t(cur), t(seg), t(base), GATE, out=buf)          # (``out`` takes the bucketed routes' result)
    _check(buf, ref.pairwise_dependence(cur, seg, base, GATE.max_lag, GATE.min_points))
    # (the wide batch's row without a current sample uses 25 columns: it goes with the narrow rows)
    assert C.dependence_route_rows() == {"wave": len(KINDS) + 1, "wide": len(KINDS) - 1, "host": 1}


def test_dependence_no_rows(cuda):
    r = C.pairwise_dependence(*(torch.zeros((0, n), dtype=dt, device=cuda) for n, dt in
                                ((40, torch.float32), (2, torch.int32), (50, torch.float32))), GATE)
    assert r.dep.shape == (0, 6) and r.rho.shape == (0, 2, 16) and r.dep_keep.shape == (0,)
