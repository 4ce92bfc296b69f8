"""The decision kernel (fm_decide_services, csrc/kernels/decide.hip) at its edge
shapes against the CPU reference the canary tests use (ops/reference.py
through ``C.stats_decide`` / ``C.service_reduce`` on CPU tensors, the path of
``CanaryScorer(device="cpu")``): the lane-per-metric forms M = 8 and M = 4 with
the window in one wave, and M = 3 (the generic loop) as the control.

The history statistics come from fm_hist_stats, so ``stats`` carry the fp32
tolerance of the existing canary tests (rtol 2e-5, atol 1e-5).  Every current
point is placed further than boundary.B_EPS (1e-4 of |mean| + thr std, above
that tolerance) from an active band edge -- test_reference_places_points_off_
the_band_edges checks that on the CPU for every case -- so flags, count,
valid, diff and the packed verdict must match exactly.

``score`` is (x - edge) / std: with the stats tolerance tol(v) = 2e-5 |v| +
1e-5 on the edge and on std its error is at most (tol(edge) + |z| tol(std)) /
std, plus the 1-ulp reciprocal and two roundings (< 1e-6 |z|); where std == 0
it is the constant 1e30 on both sides."""
import numpy as np
import pytest
import torch

from foremast_amd.ops import canary as C

from boundary import B_EPS, point_boundary

T = 24                                        # history points per row (ld = T)
MIN_HIST = 5
FACTOR = 0.8
P_THR = float(np.float32(0.05))               # what the kernel compares against, as a double
SERVICES = (1, 3, 4, 5)
METRICS = (8, 4, 3)
WINDOWS = (1, 50, 64)
# (test_mask, combine_any, pvals given)
CONFIGS = ((63, 0, True), (63, 1, True), (0b000100, 0, True), (0b101010, 1, True), (0b101010, 0, True),
           (0, 1, True), (63, 0, False))


def _tables(M):
    thr = np.array([2.0, 3.0, 2.5, 1.5, 2.0, 4.0, 1.0, 3.5], np.float32)[:M]
    bound = np.array([3, 1, 2, 3, 1, 2, 3, 1], np.int32)[:M]          # 1 upper, 2 lower, 3 both
    minlb = np.array([0.0, 0.0, 9.5, -5.0, 0.0, 9.0, 9.75, 0.0], np.float32)[:M]   # 9.x: above mean - thr std
    return thr, bound, minlb


def _combine(P, mask, combine_any):
    """reference.pairwise_tests' combination of the masked p-values (NaN =
    test not applicable), on the fp32 p-values the kernel is given."""
    sel = np.array([(mask >> i) & 1 for i in range(C.N_TESTS)], dtype=bool)
    app = ~np.isnan(P[:, sel])
    sig = app & (np.nan_to_num(P[:, sel].astype(np.float64), nan=1.0) < P_THR)
    na, ns = app.sum(1), sig.sum(1)
    return np.where(na > 0, (ns > 0) if combine_any else (ns == na), False).astype(np.int8)


def _inputs(S, M, n_cur):
    rng = np.random.default_rng(1000 * S + 10 * M + n_cur)
    R = S * M
    hist = rng.normal(10.0, 2.0, (R, T)).astype(np.float32)
    cur = rng.normal(10.0, 5.0, (R, n_cur)).astype(np.float32)
    cur[rng.random(cur.shape) < 0.08] = np.nan                         # NaN points
    # a service with nothing to report (status 0) and one that is only unknown (status 2: a row without history)
    calm = range(M, 3 * M) if S >= 4 else (range(M, 2 * M) if S >= 3 else ())
    for r in calm:
        cur[r] = np.where(np.isnan(cur[r]), np.nan, 10.0 + rng.uniform(0.1, 0.6, n_cur)).astype(np.float32)
    for r in range(R):
        k = -1 if r in calm else r % 7
        if k == 1:
            hist[r, 3:] = np.nan                                       # n = 3 < min_hist
        elif k == 2 and r % 2 == 0:
            hist[r, :] = np.nan                                        # n = 0
        elif k == 3:
            hist[r, :] = 7.0                                           # sd = 0: the band is the point 7
            cur[r] = np.where(np.isnan(cur[r]), np.nan, 7.0 + np.sign(cur[r] - 10.0) * (1.0 + np.abs(cur[r] - 10.0)))
        elif k == 5:
            hist[r, ::3] = np.nan                                      # a masked row, n = 16
    if S >= 4:
        hist[2 * M, :] = np.nan
    cur[R - 1, :] = np.nan                                             # an all-NaN window
    pv = rng.uniform(0.0, 0.12, (R, C.N_TESTS)).astype(np.float32)
    pv[rng.random(pv.shape) < 0.2] = np.nan
    pv[rng.random(pv.shape) < 0.15] = np.float32(0.05)                 # equal to the threshold: not significant
    pv[R - 2, :] = np.nan                                              # no applicable test
    pv[0, :] = np.float32(0.01)                                        # every test significant
    return hist, cur, pv


def _reference(hist, cur, pv, M, mask, combine_any, with_pv):
    thr, bound, minlb = _tables(M)
    diff = _combine(pv, mask, combine_any) if with_pv else None
    t = torch.from_numpy
    dec = C.stats_decide(t(hist), t(cur), T, M, t(thr), t(bound), t(minlb), None if diff is None else t(diff),
                         FACTOR, MIN_HIST)
    packed = C.service_reduce(dec.count, dec.score, dec.valid, M)
    return dec, packed.numpy(), diff


def _placed(S, M, n_cur, mask, combine_any, with_pv):
    """The case's inputs with every point that the reference finds within
    B_EPS of an active edge moved off it (as test_canary_ops does), its
    reference outputs, and the points still near an edge (none may be)."""
    hist, cur, pv = _inputs(S, M, n_cur)
    thr, bound, _ = _tables(M)
    for _ in range(2):
        dec, packed, diff = _reference(hist, cur, pv, M, mask, combine_any, with_pv)
        th_rows = np.tile(thr, S) * (np.where(diff.astype(bool), FACTOR, 1.0) if diff is not None else 1.0)
        stats = dec.stats.numpy()
        near = point_boundary(cur, stats, th_rows, np.tile(bound, S))
        if not near.any():
            break
        scale = np.abs(stats[:, 0:1]) + th_rows[:, None] * np.abs(stats[:, 1:2]) + 1e-6
        cur = np.where(near, cur + (1e3 * B_EPS * scale).astype(np.float32), cur).astype(np.float32)
    return hist, cur, pv, dec, packed, diff, near


def _cases():
    for S in SERVICES:
        for mask, combine_any, with_pv in CONFIGS:
            yield S, mask, combine_any, with_pv


@pytest.mark.parametrize("M", METRICS)
@pytest.mark.parametrize("n_cur", WINDOWS)
def test_reference_places_points_off_the_band_edges(M, n_cur):
    """CPU only: for every case no finite point is within B_EPS of an active
    band edge, and the cases do exercise what they are meant to."""
    seen = dict(flag=0, lowhist=0, nohist=0, sd0=0, clamp=0, diff=0, nodiff=0, allnan=0, unknown=0, clean=0)
    for S, mask, combine_any, with_pv in _cases():
        hist, cur, pv, dec, packed, diff, near = _placed(S, M, n_cur, mask, combine_any, with_pv)
        assert not near.any(), (S, M, n_cur, mask, combine_any)
        n = np.isfinite(hist).sum(1)
        st = dec.stats.numpy()
        _, _, minlb = _tables(M)
        seen["flag"] += int(dec.count.sum())
        seen["lowhist"] += int(((n > 0) & (n < MIN_HIST)).sum())
        seen["nohist"] += int((n == 0).sum())
        seen["sd0"] += int(((st[:, 1] == 0) & (n >= MIN_HIST) & (dec.count.numpy() > 0)).sum())
        seen["clamp"] += int((st[:, 3] == np.tile(minlb, S)).sum())
        seen["allnan"] += int((~np.isfinite(cur)).all(1).sum())
        if diff is not None:
            seen["diff"] += int(diff.sum())
            seen["nodiff"] += int((diff == 0).sum())
        seen["unknown"] += int((packed[:, 0] == 2).sum())
        seen["clean"] += int((packed[:, 0] == 0).sum())
    missing = [k for k, v in seen.items() if v == 0]
    assert not missing, (missing, seen)


def _gpu_decide(cuda, hist, cur, pv, S, M, mask, combine_any, with_pv):
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    thr, bound, minlb = _tables(M)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    R, n_cur = cur.shape
    h, c, p = t(hist), t(cur), (t(pv) if with_pv else None)
    thr_d, bound_d, minlb_d = t(thr), t(bound), t(minlb)
    hs = torch.full((R, 3), float("nan"), device=cuda)
    o = C.alloc_decide(R, n_cur, cuda)
    for x in (o.stats, o.score):
        x.fill_(float("nan"))
    for x in (o.flags, o.count, o.valid):
        x.fill_(-7)
    diff = torch.full((R,), -7, dtype=torch.int8, device=cuda)
    packed = torch.full((S, 4), float("nan"), device=cuda)
    st = stream_of(h)
    LIB.call("fm_hist_stats", ptr(h), h.stride(0), T, R, ptr(hs), st)
    LIB.call("fm_decide_services", ptr(hs), ptr(c), c.stride(0), n_cur, S, M, ptr(thr_d), ptr(bound_d), ptr(minlb_d),
             FACTOR, ptr(p), mask, combine_any, P_THR, MIN_HIST, ptr(o.stats), ptr(o.flags), o.flags.shape[1],
             ptr(o.count), ptr(o.score), ptr(o.valid), ptr(diff), ptr(packed), st)
    torch.cuda.synchronize()
    return o, diff.cpu().numpy(), packed.cpu().numpy()


def _score_tol(stats, z):
    tol = lambda v: 2e-5 * np.abs(v) + 1e-5
    sd = stats[:, 1].astype(np.float64)
    edge = np.maximum(np.abs(stats[:, 2]), np.abs(stats[:, 3])).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(sd > 0, (tol(edge) + np.abs(z) * tol(sd)) / sd + 1e-6 * np.abs(z), 0.0)


@pytest.mark.gpu
@pytest.mark.parametrize("M", METRICS)
@pytest.mark.parametrize("n_cur", WINDOWS)
def test_gpu_decide_services_matches_reference(cuda, M, n_cur):
    for S, mask, combine_any, with_pv in _cases():
        what = f"S={S} M={M} n_cur={n_cur} mask={mask} any={combine_any} pvals={with_pv}"
        hist, cur, pv, dec, want_packed, want_diff, near = _placed(S, M, n_cur, mask, combine_any, with_pv)
        assert not near.any(), what
        o, diff, packed = _gpu_decide(cuda, hist, cur, pv, S, M, mask, combine_any, with_pv)
        stats, want_stats = o.stats.cpu().numpy(), dec.stats.numpy()
        print(what, "max |stats - ref|", float(np.abs(stats - want_stats).max()))
        np.testing.assert_allclose(stats, want_stats, rtol=2e-5, atol=1e-5, err_msg=what)
        np.testing.assert_array_equal(o.flags.cpu().numpy()[:, 0], dec.flags.numpy()[:, 0], err_msg=what)
        np.testing.assert_array_equal(o.count.cpu().numpy(), dec.count.numpy(), err_msg=what)
        np.testing.assert_array_equal(o.valid.cpu().numpy(), dec.valid.numpy(), err_msg=what)
        if with_pv:
            np.testing.assert_array_equal(diff, want_diff, err_msg=what)
        else:
            assert (diff == -7).all(), what                          # not written without p-values
        score, want_score = o.score.cpu().numpy().astype(np.float64), dec.score.numpy().astype(np.float64)
        tol = _score_tol(want_stats, want_score)
        print(what, "max score error / bound", float(np.max(np.abs(score - want_score) / np.maximum(tol, 1e-30),
                                                              where=tol > 0, initial=0.0)))
        assert (np.abs(score - want_score) <= tol).all(), what
        # the packed verdict: status, anomalous-metric mask and point count exactly, the score as the rows'
        np.testing.assert_array_equal(packed[:, [0, 2, 3]], want_packed[:, [0, 2, 3]], err_msg=what)
        np.testing.assert_array_equal(packed[:, 1], np.maximum(score.reshape(S, M).max(1), 0).astype(np.float32),
                                      err_msg=what)
