"""K30 (csrc/kernels/pairwise_joint.hip) against the numpy definition
``reference.pairwise_joint`` / ``joint_verdict`` (docs/BRAIN_SPEC.md 4.4) at
the register tiers' edge widths, every kind of group in one batch per shape.

T, A, n12, dof, worst, N and the NaN placement compare exactly; L and the z to
1e-5 relative and p to 2e-4 relative (K29's tolerances: the same fp64 finish
rounded to fp32 and the same tail function).  dof, worst and the verdict
compare on every group, which needs pivots well away from the 1e-9 rule
(independent members, or an exact copy / negation whose pivot is 0 up to
rounding), largest |z| that are apart or exactly equal, and p-values 2e-4
relative off the threshold: the last two are asserted on the reference."""
import numpy as np
import pytest
import torch

from foremast_amd.ops import canary as C
from foremast_amd.ops import reference as ref

pytestmark = pytest.mark.gpu
TEST = C.JointTest("RANK_SUM", 0.05, 5)
SHAPES = [(5, 5), (63, 1), (64, 1), (37, 90), (300, 724)]


def _batch(nc, nb, seed=0):
    """(cur [R, nc], base [R, nb], rows [G, 8] int32, K [G]): one group per kind, the rows shuffled."""
    rng = np.random.default_rng(seed)
    n = nc + nb

    def block(k, shift=0.0):
        """k members sharing a common factor; member 0's current side shifted by ``shift`` sigma."""
        x = 100 + 5 * (0.7 * rng.normal(0, 1, n) + rng.normal(0, 1, (k, n)))
        x[0, :nc] += 5 * shift
        return x

    kinds = []                                                 # (members' data, their order in ``rows``)
    kinds.append((block(1, 0.8), [0]))
    kinds.append((block(2), [1, 0]))
    kinds.append((block(3, 0.5), [2, 0, 1]))
    kinds.append((block(8, 0.5), [7, 0, 1, 2, 3, 4, 5, 6]))
    x = block(3, 0.5)                                          # missing samples in different columns of different members
    x[0, ::7], x[1, 3::11], x[2, 5::13], x[1, 1] = np.nan, np.inf, -np.inf, np.nan
    kinds.append((x, [0, 1, 2]))
    x = block(3)
    x[1] = np.nan                                              # one member all-NaN: no column is kept
    kinds.append((x, [0, 1, 2]))
    x = np.round(rng.normal(0, 0.3, (8, n)), 1)                # heavy ties, signed zeros among them
    x[::2][x[::2] == 0] = -0.0
    kinds.append((x, list(range(8))))
    x = block(3, 0.5)
    x[1] = 7.0                                                 # a constant member
    kinds.append((x, [0, 1, 2]))
    x = block(2, 0.5)
    kinds.append((np.stack([x[0], x[1], x[0]]), [0, 1, 2]))    # an exact copy: dof = K - 1
    kinds.append((np.stack([x[0], x[1], -x[0]]), [0, 1, 2]))   # a negation: dof = K - 1
    x = block(2, 0.5)
    x[:, nc + 3:] = np.nan                                     # a baseline below min_points
    kinds.append((x, [1, 0]))

    R = sum(len(x) for x, _ in kinds)
    at = rng.permutation(R)
    data = np.empty((R, n), np.float32)
    rows = np.full((len(kinds), 8), -1, np.int32)
    r = 0
    for g, (x, order) in enumerate(kinds):
        data[at[r:r + len(x)]] = x
        rows[g, :len(order)] = at[r + np.asarray(order)]
        r += len(x)
    return data[:, :nc].copy(), data[:, nc:].copy(), rows, np.asarray([len(o) for _, o in kinds], np.int64)


def _check(got: C.JointResult, want, thr=TEST.p_threshold):
    joint, n12, T, A, member_z = want
    az = np.sort(np.nan_to_num(np.abs(member_z.astype(np.float64)), nan=-1.0), axis=1)
    ok = (az[:, -1] == az[:, -2]) | (az[:, -1] - az[:, -2] > 1e-6 * az[:, -1])
    assert ok[joint[:, 4] >= 0].all()
    assert not (np.abs(joint[:, 1].astype(np.float64) - thr) <= 2e-4 * thr).any()
    g = [t.cpu().numpy() for t in got.tensors()]
    for a, b in zip(g[1:4], (n12, T, A)):
        np.testing.assert_array_equal(a, b)
    np.testing.assert_array_equal(g[0][:, [2, 4, 5]], joint[:, [2, 4, 5]])          # dof, worst, N
    np.testing.assert_array_equal(np.isnan(g[0]), np.isnan(joint))
    np.testing.assert_array_equal(np.isnan(g[4]), np.isnan(member_z))
    np.testing.assert_allclose(g[0][:, [0, 3]], joint[:, [0, 3]], rtol=1e-5, atol=0)
    np.testing.assert_allclose(g[4], member_z, rtol=1e-5, atol=0)
    np.testing.assert_allclose(g[0][:, 1], joint[:, 1], rtol=2e-4, atol=0)
    np.testing.assert_array_equal(g[5], ref.joint_verdict(joint, thr))


@pytest.mark.parametrize("nc,nb", SHAPES)
def test_joint_kernel_matches_definition(cuda, nc, nb):
    cur, base, rows, K = _batch(nc, nb)
    want = ref.pairwise_joint(cur, base, rows, K, TEST.min_points)
    if nb >= TEST.min_points:
        assert (want[0][[8, 9], 2] == 2).all() and np.isfinite(want[0][:4, 0]).all()   # the copy, the negation
    t = lambda a: torch.from_numpy(a).to(cuda)  # noqa: E731
    C.reset_joint_route_rows()
    _check(C.pairwise_joint(t(cur), t(base), t(rows), t(K), TEST), want)
    assert C.joint_route_rows() == {"wave": len(K), "host": 0}


def test_joint_no_groups(cuda):
    cur, base, rows, K = _batch(5, 5)
    t = lambda a: torch.from_numpy(a).to(cuda)  # noqa: E731
    got = C.pairwise_joint(t(cur), t(base), t(rows[:0]), t(K[:0]), TEST)
    assert [len(x) for x in got.tensors()] == [0] * 6
    diff = torch.ones(len(cur), dtype=torch.int8, device=cuda)
    assert C.joint_diff(diff, t(cur), t(base), t(rows[:0]), t(K[:0]), TEST) is diff


def test_joint_padded_batch_is_narrowed_and_the_wider_group_runs_on_the_host(cuda):
    """A batch padded to 1,500 columns: the groups of the 37 + 90 batch fit K30 once cut to their used widths; a
    group of 800 + 400 really is wider."""
    c, b, rows, K = _batch(37, 90)
    rng = np.random.default_rng(1)
    R = len(c)
    cur, base = np.full((R + 2, 1000), np.nan, np.float32), np.full((R + 2, 500), np.nan, np.float32)
    cur[:R, :37], base[:R, :90] = c, b
    cur[R:, :800], base[R:, :400] = rng.normal(100, 5, (2, 800)), rng.normal(100, 5, (2, 400))
    rows = np.concatenate([rows, [[R + 1, R] + [-1] * 6]]).astype(np.int32)
    K = np.concatenate([K, [2]])
    t = lambda a: torch.from_numpy(a).to(cuda)  # noqa: E731
    C.reset_joint_route_rows()
    _check(C.pairwise_joint(t(cur), t(base), t(rows), t(K), TEST), ref.pairwise_joint(cur, base, rows, K, TEST.min_points))
    assert C.joint_route_rows() == {"wave": len(K) - 1, "host": 1}
