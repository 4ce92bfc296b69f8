"""K35 robust_holt_winters: the Huber-clipped additive Holt-Winters fit
(ops.smoothing.ref_es_fit_robust is the definition, csrc/kernels/hw_robust_scan.hip
the GPU kernel)."""
import functools

import numpy as np
import pytest
import torch

from foremast_amd.config import BrainConfig
from foremast_amd.models import zoo
from foremast_amd.ops import misc as MI
from foremast_amd.ops import smoothing as SM

INF = np.float32(np.inf)


def _series(R, T, m, seed, sigma=1.0):
    """Daily-cyclic rows: level 100, amplitude 20, N(0, sigma) noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)
    return (100 + 20 * np.sin(2 * np.pi * t / m)[None, :] + sigma * rng.standard_normal((R, T))).astype(np.float32)


def test_infinite_clip_is_the_plain_fit():
    m, T, grid = 24, 200, SM.default_grid(2)
    x = _series(4, T, m, 1)
    x[1, :7] = np.nan          # ragged
    x[2, 90:97] = np.nan       # gap
    x[3, :] = np.nan           # empty
    fc0, sig0, best0, sse0, st0 = SM.ref_es_fit(x, 2, 6, m, grid, return_state=True)
    fc, sig, best, sse, ncl, st = SM.ref_es_fit_robust(x, 6, m, grid, np.full(4, INF), return_state=True)
    for a, b in ((fc, fc0), (sig, sig0), (best, best0), (sse, sse0)) + tuple((st[k], st0[k]) for k in st0):
        np.testing.assert_array_equal(a, b)
    assert not ncl.any()
    # a threshold that is not finite or not positive leaves the row unclipped too
    assert np.array_equal(SM.ref_es_fit_robust(x, 6, m, grid, np.array([0, -1, np.nan, 1], np.float32))[3][:3], sse0[:3])


def test_incident_in_the_history_moves_the_plain_fit_not_the_robust_one():
    # alpha = 0.1 candidates only: a clipped step moves the level by alpha * c = 0.3 sigma, so over 60 steps it
    # cannot reach the incident's 20 sigma and every incident step is clipped (alpha = 0.3 catches up in ~22)
    m, T, H, grid = 144, 6 * 144 + 30, 20, SM.default_grid(2)[:9]
    clean = _series(1, T, m, 2)
    dirty = clean.copy()
    dirty[0, 3 * m + 40:3 * m + 100] += 20           # 60 steps of +20 sigma in lap 3
    plain_c = SM.es_fit(torch.from_numpy(clean), T, 2, H, m, grid=grid)
    plain_d = SM.es_fit(torch.from_numpy(dirty), T, 2, H, m, grid=grid)
    rob_d = SM.es_fit_robust(torch.from_numpy(dirty), T, H, m, grid=grid, k=3.0)
    err = lambda f: (f.forecast - plain_c.forecast).abs().mean().item()
    assert err(rob_d) < err(plain_d)
    assert plain_c.sigma.item() <= rob_d.sigma.item() <= plain_d.sigma.item()
    assert rob_d.nclip[0, rob_d.best[0]].item() >= 60


def test_clip_threshold():
    m, T = 24, 200
    x = _series(4, T, m, 3)
    x[0, 50:60] = np.nan
    x[1, :] = 7.0                                      # constant: sigma_d == 0
    x[2, :T - m - 1] = np.nan                          # one finite difference at the most
    d = x[:, m:] - x[:, :-m]
    _, sd, _ = MI.ref_robust_stats(d, T - m)
    c = SM.hw_robust_clip(torch.from_numpy(x), T, m, 2.5).numpy()
    np.testing.assert_allclose(c[[0, 3]], 2.5 * sd[[0, 3]] / np.sqrt(2.0), rtol=1e-6)
    assert c[1] == INF and c[2] == INF


def test_decide_flags_what_the_widened_plain_band_misses():
    m, T, n = 144, 6 * 144, 10
    hist = _series(2, T, m, 4)
    hist[:, 2 * m + 30:2 * m + 90] += 60               # past incidents: they widen the plain fit's sigma
    hist[:, 4 * m + 60:4 * m + 120] -= 60
    cur = _series(2, T + n, m, 5, sigma=0.0)[:, T:].copy()
    cur[0] += 7                                         # 7 sigma of the noise above the cycle
    tables = zoo.make_tables(["requests"] * 2, BrainConfig(), "cpu")
    hor = torch.arange(1, n + 1, dtype=torch.int64)[None, :].repeat(2, 1)
    count = lambda algo: zoo.decide(algo, torch.from_numpy(hist), T, torch.from_numpy(cur), hor, 2, tables,
                                    period=m).count.tolist()
    assert count("holt_winters") == [0, 0]
    assert count("robust_hw") == [n, 0]
    fc, sig = zoo.forecast("hw_robust", torch.from_numpy(hist), T, n, period=m)
    assert fc.shape == (2, n) and (sig < 3).all()        # (the plain fit: 5.2)


GPU_SHAPES = [(192, 5 * 192 + 17), (200, 5 * 200 + 17), (1536, 2 * 1536 + 40)]


@functools.lru_cache(maxsize=None)
def _gpu_case(m, T):
    """The 8 rows of a GPU case and their reference fit (computed once)."""
    Cn = -(-m // 64)
    x = _series(8, T, m, 100 + m)
    x[1, m + m // 2] += 40                              # a single-sample spike
    x[2, m + m // 3:m + m // 3 + int(2.5 * Cn)] += 40   # an incident across chunk borders
    x[3, 2 * m - 10:2 * m + 10] -= 40                   # an incident across a lap boundary
    x[4, T // 2:] += 40                                 # a level shift: many consecutive clipped chunks
    x[5, m + 50:m + 60] = np.nan                        # a gap, and an incident right after it
    x[5, m + 60:m + 80] += 40
    x[6, :11] = np.nan                                  # a ragged start with a spike
    x[6, m + 100] -= 40
    x[7, :] = np.nan
    clip = SM.hw_robust_clip(torch.from_numpy(x), T, m, 3.0).numpy()
    return x, clip, SM.ref_es_fit_robust(x, 10, m, SM.default_grid(2), clip, return_state=True)


def _check_fit(fit, x, ref):
    """The scan fit's tolerances (test_model_ops.py::test_gpu_hw_scan_fit_matches_references)."""
    fc0, sig0, best0, sse0, _, st0 = ref
    sse, best = fit.sse.cpu().numpy(), fit.best.cpu().numpy()
    ok = np.isfinite(sse0) & (sse0 > 0)
    np.testing.assert_allclose(sse[ok], sse0[ok], rtol=2e-3)
    two = np.sort(np.where(np.isfinite(sse0), sse0, np.inf), axis=1)[:, :2]
    clear = two[:, 1] - two[:, 0] > 4e-3 * two[:, 1]
    np.testing.assert_array_equal(best[clear], best0[clear])
    same = np.flatnonzero((best == best0) & np.isfinite(fc0).all(1))
    amp = np.abs(np.nan_to_num(x[same])).mean(1, keepdims=True)
    np.testing.assert_allclose(fit.forecast.cpu().numpy()[same] / amp, fc0[same] / amp, atol=2e-3)
    np.testing.assert_allclose(fit.model.season.cpu().numpy()[same] / amp, st0["season"][same] / amp, atol=2e-3)
    np.testing.assert_allclose(fit.sigma.cpu().numpy()[same], sig0[same], rtol=1e-3 + 4e-7)
    np.testing.assert_array_equal(fit.model.nobs.cpu().numpy()[same], st0["nobs"][same])
    return same


@pytest.mark.gpu
@pytest.mark.parametrize("m,T", GPU_SHAPES)
def test_gpu_robust_fit_matches_the_definition(cuda, m, T):
    x, clip, ref = _gpu_case(m, T)
    assert SM.hw_robust_supported(T, 27, m) and np.isfinite(clip[:7]).all() and clip[7] == INF
    fit = SM.es_fit_robust(torch.from_numpy(x).to(cuda), T, 10, m, clip=torch.from_numpy(clip), keep_state=True)
    same = _check_fit(fit, x, ref)
    assert len(same) >= 5
    # the all-NaN row: the reference's NaN / 0 outputs
    assert torch.isnan(fit.forecast[7]).all() and fit.sigma[7].item() == 0 and fit.best[7].item() == 0
    assert (fit.sse[7] == 0).all() and (fit.nclip[7] == 0).all()
    np.testing.assert_array_equal(fit.nfin.cpu().numpy(), np.isfinite(x).sum(1))
    assert (fit.nclip[4] > 0).all()            # every candidate clips the level shift's first steps


@pytest.mark.gpu
def test_gpu_robust_fit_unclipped_is_the_scan_fit(cuda):
    m, T = GPU_SHAPES[0]
    x = _gpu_case(m, T)[0]
    xt = torch.from_numpy(x).to(cuda)
    fit = SM.es_fit_robust(xt, T, 10, m, clip=torch.full((8,), float("inf")), keep_state=True)
    sc = SM.es_fit(xt, T, 2, 10, m, method="scan", keep_state=True)
    ref = (sc.forecast.cpu().numpy(), sc.sigma.cpu().numpy(), sc.best.cpu().numpy(), sc.sse.cpu().numpy(), None,
           {"season": sc.model.season.cpu().numpy(), "nobs": sc.model.nobs.cpu().numpy()})
    assert len(_check_fit(fit, x, ref)) >= 7 and not fit.nclip.any()
    out = torch.ops.foremast.es_fit_robust(xt, T, 10, m, torch.from_numpy(SM.default_grid(2)),
                                           torch.full((8,), float("inf"), device=cuda))
    assert torch.equal(out[3], fit.sse) and torch.equal(out[0][:7], fit.forecast[:7])
