"""K36 robust_prophet: Huber IRLS on prophet's design with a Gram matrix per row
(ops.lsq.ref_prophet_fit_robust is the definition, csrc/kernels/lsq_robust.hip
the GPU kernel)."""
import functools

import numpy as np
import pytest
import torch

from foremast_amd.config import BrainConfig
from foremast_amd.models import zoo
from foremast_amd.ops import lsq as LQ
from foremast_amd.ops._lib import LIB, ptr, stream_of

from test_fastpath_models import FAULTS, _brain, _compare, _submit

INF = float("inf")
H = 10


def _series(R, T, seed, sigma=1.0):
    """Daily-cyclic rows at 60 s: level 100, amplitude 20, N(0, sigma) noise."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)
    return (100 + 20 * np.sin(2 * np.pi * t / 1440)[None, :] + sigma * rng.standard_normal((R, T))).astype(np.float32)


# ------------------------------------------------------------------ definition
def test_infinite_k_without_gaps_is_prophet():
    T = 2 * 1440 + 17
    y = _series(3, T, 1)
    ref = LQ.ref_prophet_fit_robust(y, T, H, k=INF)
    plain = LQ.prophet_fit(torch.from_numpy(y), T, H)
    np.testing.assert_allclose(ref[1], plain.forecast.numpy(), rtol=1e-5)      # (the ridge is the only difference)
    assert (ref[4] == T).all() and not ref[5].any()


@functools.lru_cache(maxsize=None)
def _gap_case():
    """A week (the design has full rank) with 10 % missing in one block: the
    row, the design, numpy's least squares over the finite samples and the fit."""
    T = 7 * 1440
    y = _series(1, T, 2)
    y[0, 3000:3000 + T // 10] = np.nan
    X = LQ.design_matrix(T, H)
    f = np.isfinite(y[0])
    coef = np.linalg.lstsq(X[:T][f], y[0, f].astype(np.float64), rcond=None)[0]
    return T, y, X, coef, LQ.ref_prophet_fit_robust(y, T, H, k=INF)


def test_gaps_get_the_least_squares_fit_prophet_does_not():
    T, y, X, coef, ref = _gap_case()
    truth = X[T:] @ coef
    np.testing.assert_allclose(ref[1][0], truth, rtol=1e-5)
    plain = LQ.prophet_fit(torch.from_numpy(y), T, H).forecast.numpy()[0]
    assert np.abs(ref[1][0] - truth).max() < np.abs(plain - truth).max()


def test_gaps_beta_is_the_least_squares_solution():
    """The ridge conditions the solves but does not bias their limit: S^-1
    (singular values 130 ... 0.07 over a week) would carry a ridge solution's
    1e-6 into beta as 1e-3."""
    T, y, X, coef, ref = _gap_case()
    np.testing.assert_allclose(ref[0][0], coef, rtol=1e-5)


# -------------------------------------------------------------------- incident
def test_incident_moves_the_plain_fit_not_the_robust_one():
    T, n = 4 * 1440, 10
    clean = _series(1, T, 3)
    dirty = clean.copy()
    dirty[0, 2 * 1440 + 300:2 * 1440 + 360] += 20                              # 60 samples at +20 sigma
    plain_c = LQ.prophet_fit(torch.from_numpy(clean), T, n)
    plain_d = LQ.prophet_fit(torch.from_numpy(dirty), T, n)
    rob_d = LQ.prophet_fit_robust(torch.from_numpy(dirty), T, n)
    err = lambda f: (f.forecast - plain_c.forecast).abs().max().item()
    assert err(rob_d) < err(plain_d)
    assert plain_c.sigma.item() <= rob_d.sigma.item() < plain_d.sigma.item()
    assert (rob_d.nfin - rob_d.wsum).item() >= 40
    # a current window 5 robust sigmas above the forecast is flagged
    cur = rob_d.forecast + 5 * rob_d.sigma[:, None]
    tables = zoo.make_tables(["requests"], BrainConfig(), "cpu")
    hor = torch.arange(1, n + 1, dtype=torch.int64)[None, :]
    dec = zoo.decide("robust_prophet", torch.from_numpy(dirty), T, cur, hor, 1, tables)
    assert dec.count.tolist() == [n]


# ---------------------------------------------------------------------- wiring
def test_aliases_and_settings():
    assert {zoo.canonical(a) for a in ("robust_prophet", "prophet_robust", "huber_prophet")} == {"robust_prophet"}
    assert "robust_prophet" in zoo.ALGORITHMS and "robust_prophet" in zoo.FORECASTERS
    cfg = BrainConfig.from_env({"ML_PROPHET_ROBUST_K": "2.5", "ML_PROPHET_ROBUST_ITERS": "40"})
    assert (cfg.prophet_robust_k, cfg.prophet_robust_iters) == (2.5, 16)
    assert BrainConfig.from_env({"ML_PROPHET_ROBUST_ITERS": "-3"}).prophet_robust_iters == 0
    assert (BrainConfig().prophet_robust_k, BrainConfig().prophet_robust_iters) == (3.0, 5)


def test_brain_cycle_ends_with_the_zoo_verdict(device="cpu"):
    """ML_ALGORITHM=robust_prophet: the resident fast path (op by op) and the
    general path, which calls zoo.decide, reach the same verdicts and bands."""
    a = _brain(True, "robust_prophet", FAULTS, device)
    b = _brain(False, "robust_prophet", FAULTS, device)
    assert a[3]._model_args("huber_prophet") == {"prophet_k": 3.0, "prophet_iters": 5}
    ids = _submit(a[2], "static")
    assert ids == _submit(b[2], "static")
    ra, rb = a[3].run_once(), b[3].run_once()
    assert ra["claimed"] == rb["claimed"] == len(ids)
    _compare(a, b, ids, 0)


# ------------------------------------------------------------------------- GPU
GPU_T = (100, 160, 2017, 4100)
# forecast (rtol, atol), sigma and wsum rtol: K10's own GPU-against-host tolerances
# (tests/test_model_edges.py::test_gpu_lsq_edges); docs/PERF.md K36 has the fp32 mirror's errors
FC_TOL, REL_TOL = (1e-3, 2e-3), 1e-3


@functools.lru_cache(maxsize=None)
def _gpu_case(T, k):
    """The 9 rows of a GPU case, padded to a 16-B row pitch, and their fp64
    reference (computed once)."""
    p = LQ._basis(T, H, 60.0)[3]
    y = _series(9, T, 100 + T)
    y[1, T // 2:T // 2 + max(4, T // 40)] += 20                                # an incident
    y[2, 0] = np.nan                                                           # c = 0
    y[3, T // 3:T // 3 + T // 10] = np.nan                                     # a block gap
    y[4] += 1e4
    y[5] = 7.0                                                                 # constant: s == 0 stops it
    keep = np.linspace(0, T - 1, 2 * p).round().astype(int)                    # 2 p samples spread over the row
    for row, idx in ((6, keep[1:]), (7, keep)):                                # 2 p - 1: fallback; 2 p: fitted
        v = y[row, idx].copy()
        y[row] = np.nan
        y[row, idx] = v
    y[8] = np.nan
    buf = np.full((9, (T + 3) // 4 * 4), np.nan, np.float32)
    buf[:, :T] = y
    return buf, p, LQ.ref_prophet_fit_robust(y, T, H, k=k)


def _check(fit, ref):
    beta, fc, sigma, nfin, wsum, fb = ref
    np.testing.assert_array_equal(fit.nfin.cpu().numpy(), nfin)
    np.testing.assert_array_equal(fit.fallback.cpu().numpy(), fb)
    np.testing.assert_allclose(fit.forecast.cpu().numpy(), fc, rtol=FC_TOL[0], atol=FC_TOL[1])
    np.testing.assert_allclose(fit.sigma.cpu().numpy(), sigma, rtol=REL_TOL)
    np.testing.assert_allclose(fit.wsum.cpu().numpy(), wsum, rtol=REL_TOL)


@pytest.mark.gpu
@pytest.mark.parametrize("rows", (1, 2))
@pytest.mark.parametrize("k", (3.0, INF))
@pytest.mark.parametrize("T", GPU_T)
def test_gpu_kernel_matches_the_definition(cuda, T, k, rows):
    buf, p, ref = _gpu_case(T, k)
    assert LQ.lsq_robust_supported(T) and p == {100: 15, 160: 17, 2017: 28, 4100: 32}[T]   # dropped columns, and none
    assert ref[5].tolist() == [False] * 6 + [True, False, True] and np.isnan(ref[1][8]).all()
    fit = LQ.prophet_fit_robust(torch.from_numpy(buf).to(cuda), T, H, k=k, rows=rows)
    _check(fit, ref)


@pytest.mark.gpu
def test_gpu_routing_and_refusals(cuda):
    T = 2017
    buf, p, ref = _gpu_case(T, 3.0)
    Y = torch.from_numpy(buf).to(cuda)
    # the op and the zoo on the GPU give the CPU call's result
    out = torch.ops.foremast.prophet_fit_robust(Y, T, H, 60.0, 3.0, 5)
    np.testing.assert_allclose(out[1].cpu().numpy(), ref[1], rtol=FC_TOL[0], atol=FC_TOL[1])
    fc, sg = zoo.forecast("robust_prophet", Y, T, H)
    fc0, sg0 = zoo.forecast("robust_prophet", torch.from_numpy(buf), T, H)
    np.testing.assert_allclose(fc.cpu().numpy(), fc0.numpy(), rtol=FC_TOL[0], atol=FC_TOL[1])
    np.testing.assert_allclose(sg.cpu().numpy(), sg0.numpy(), rtol=REL_TOL)
    # a history beyond the kernel's LDS goes to the reference
    T2 = 14000
    assert not LQ.lsq_robust_supported(T2) and LQ.lsq_robust_supported(10080)
    y2 = _series(2, T2, 7)
    y2[1, 5000:5060] += 20
    long_ = LQ.prophet_fit_robust(torch.from_numpy(y2).to(cuda), T2, H, iters=1)
    assert long_.forecast.is_cuda
    np.testing.assert_allclose(long_.forecast.cpu().numpy(), LQ.ref_prophet_fit_robust(y2, T2, H, iters=1)[1], rtol=1e-6)
    # the launcher refuses a misaligned Y and iters = 17 without launching
    XT = LQ._XT_CACHE[(T, H, 60.0, str(Y.device))]
    o = [torch.full((9 * 32,), -1.0, device=cuda) for _ in range(6)]
    call = lambda y, iters: LIB.load().fm_lsq_robust_fit(ptr(y), Y.stride(0), T, 9, ptr(XT), XT.stride(0), p, 3.0, iters,
                                                         0, *map(ptr, o), stream_of(Y))
    assert call(Y.view(-1)[1:], 5) != 0 and call(Y, 17) != 0
    torch.cuda.synchronize()
    assert all((x == -1).all() for x in o)
    assert call(Y, 16) == 0
    torch.cuda.synchronize()
    assert (o[1][:9] != -1).all()                                               # (the shifts: it ran)


@pytest.mark.gpu
def test_gpu_brain_cycle_ends_with_the_zoo_verdict():
    test_brain_cycle_ends_with_the_zoo_verdict(device="cuda")
