"""K10 prophet-lite: one streaming f32-MFMA pass computes X^T y and y.y for
every series against a shared design matrix (trend + changepoint hinges +
daily/weekly Fourier terms); the F x F solve is shared (csrc/kernels/lsq.hip)."""
from __future__ import annotations

from dataclasses import dataclass
from functools import lru_cache

import numpy as np
import torch

from ._lib import LIB, check, ptr, require_native, stream_of

F = 32


@lru_cache(maxsize=8)
def design_matrix(T: int, H: int, step_s: float = 60.0, n_changepoints: int = 6, k_daily: int = 6,
                  k_weekly: int = 6) -> np.ndarray:
    """[T+H, 32] float64: 1, t, 6 hinges at quantiles of the first 80% (Prophet's
    default changepoint range), daily & weekly Fourier pairs."""
    assert 2 + n_changepoints + 2 * (k_daily + k_weekly) == F
    t = np.arange(T + H, dtype=np.float64)
    tt = t / max(T, 1)
    cols = [np.ones_like(tt), tt]
    for c in np.linspace(0.8 / (n_changepoints + 1), 0.8, n_changepoints):
        cols.append(np.maximum(tt - c, 0.0))
    for period, K in ((86400.0 / step_s, k_daily), (7 * 86400.0 / step_s, k_weekly)):
        for k in range(1, K + 1):
            cols.append(np.sin(2 * np.pi * k * t / period))
            cols.append(np.cos(2 * np.pi * k * t / period))
    return np.stack(cols, 1)


@dataclass
class LsqFit:
    beta: torch.Tensor      # [R, 32]
    forecast: torch.Tensor  # [R, H]
    sigma: torch.Tensor     # [R]
    fitted_sse: torch.Tensor


def lsq_project(Y: torch.Tensor, T: int, XT: torch.Tensor):
    """Z = X^T (y - c), yy = |y - c|^2, c = y[0] per row (NaN samples contribute 0)."""
    R = Y.shape[0]
    if not Y.is_cuda:
        y = Y.numpy()[:, :T].astype(np.float64)
        c = np.where(np.isfinite(y[:, 0]), y[:, 0], 0.0)
        yc = np.where(np.isfinite(y), y - c[:, None], 0.0)
        Z = yc @ XT.numpy()[:, :T].astype(np.float64).T
        t = lambda a, dt=np.float32: torch.from_numpy(np.asarray(a).astype(dt))
        return t(Z), t((yc ** 2).sum(1)), t(c), t(np.isfinite(y).sum(1), np.int32)
    require_native(Y)
    check(Y.stride(0) % 4 == 0 and Y.data_ptr() % 16 == 0, "Y rows must be 16-B aligned")
    d = Y.device
    Z = torch.empty((R, F), dtype=torch.float32, device=d)
    yy = torch.empty((R,), dtype=torch.float32, device=d)
    sh = torch.empty((R,), dtype=torch.float32, device=d)
    nv = torch.empty((R,), dtype=torch.int32, device=d)
    LIB.call("fm_lsq_project", ptr(Y), Y.stride(0), T, R, ptr(XT), XT.stride(0), ptr(Z), ptr(yy), ptr(sh), ptr(nv),
             stream_of(Y))
    return Z, yy, sh, nv


_XT_CACHE: dict = {}


@lru_cache(maxsize=8)
def _basis(T: int, H: int, step_s: float):
    """Orthonormal basis of the history design (thin SVD X_h = U S V^T, rank-
    truncated) so the kernel projects onto orthonormal columns: G = I, no
    normal-equation conditioning blow-up of the fp32 MFMA sums.  Returns
    (U^T padded [F, ld] f32, forecast map X_f V S^-1 [H, F], coef map V S^-1 [F, F])."""
    X = design_matrix(T, H, step_s)
    Xh, Xf = X[:T], X[T:]
    U, S, Vt = np.linalg.svd(Xh, full_matrices=False)
    keep = S > S[0] * 1e-10
    Sinv = np.where(keep, 1.0 / np.where(keep, S, 1.0), 0.0)
    U = U * keep[None, :]
    ld = (T + 3) // 4 * 4
    ut = np.zeros((F, ld), np.float32)
    ut[:, :T] = U.T
    vs = Vt.T * Sinv[None, :]
    return ut, Xf @ vs, vs, int(keep.sum())


def lsq_residual(Y: torch.Tensor, T: int, XT: torch.Tensor, Z: torch.Tensor, shift: torch.Tensor) -> torch.Tensor:
    """SSE of every row's fit from a direct residual pass: sum over finite
    samples of (y - c - U z)^2, fp32 residuals accumulated in fp64 (not the
    cancellation-prone |y - c|^2 - |z|^2)."""
    R = Y.shape[0]
    if not Y.is_cuda:
        y = Y.numpy()[:, :T].astype(np.float64)
        fit = Z.numpy().astype(np.float64) @ XT.numpy()[:, :T].astype(np.float64)
        r = y - shift.numpy().astype(np.float64)[:, None] - fit
        return torch.from_numpy(np.where(np.isfinite(y), r * r, 0.0).sum(1))
    require_native(Y)
    check(Z.is_contiguous() and Z.shape == (R, F) and Z.dtype == torch.float32, "Z must be a contiguous [R, 32] f32")
    sse = torch.empty((R,), dtype=torch.float64, device=Y.device)
    LIB.call("fm_lsq_residual", ptr(Y), Y.stride(0), T, R, ptr(XT), XT.stride(0), ptr(Z), ptr(shift), ptr(sse),
             stream_of(Y))
    return sse


def prophet_fit(Y: torch.Tensor, T: int, H: int, step_s: float = 60.0) -> LsqFit:
    """Least-squares fit of the shared design to every row (projection pass),
    residual sigma from a second, direct residual pass (lsq_residual)."""
    ut, fmap, vs, rank = _basis(T, H, step_s)
    d = Y.device
    key = (T, H, step_s, str(d))
    if key not in _XT_CACHE:
        _XT_CACHE[key] = torch.from_numpy(ut).to(d)
    XT = _XT_CACHE[key]
    Z, yy, sh, nv = lsq_project(Y, T, XT)
    Zd = Z.to(torch.float64)
    sse = lsq_residual(Y, T, XT, Z, sh).to(d)
    fc = Zd @ torch.from_numpy(fmap.T.copy()).to(d) + sh.to(torch.float64)[:, None]
    beta = Zd @ torch.from_numpy(vs.T.copy()).to(d)
    beta[:, 0] += sh.to(torch.float64)
    dof = (nv.to(torch.float64) - rank).clamp(min=1)
    sigma = torch.sqrt(sse / dof)
    return LsqFit(beta.to(torch.float32), fc.to(torch.float32), sigma.to(torch.float32), sse.to(torch.float32))


# --------------------------------------------------------------------------- K36
LSQ_ROBUST_RIDGE = 1e-6     # csrc/kernels/lsq_robust.hip kRidge mirrors it
LSQ_ROBUST_MAX_ITERS = 16


@dataclass
class LsqRobustFit:
    beta: torch.Tensor      # [R, 32]
    forecast: torch.Tensor  # [R, H]
    sigma: torch.Tensor     # [R] MAD sigma of the final residuals (no dof correction)
    nfin: torch.Tensor      # [R] int32
    wsum: torch.Tensor      # [R] sum of the final weights; nfin - wsum is the mass set aside
    fallback: torch.Tensor  # [R] bool: fewer than 2 p finite samples, the robust constant model


def _mad_sigma(r: np.ndarray, dt) -> float:
    """K13's sigma rule (``ops.misc.ref_robust_stats``) over the finite
    residuals ``r`` (at least one), in ``dt``."""
    n = r.size
    mid = lambda v: dt(0.5) * v[(n - 1) // 2] + dt(0.5) * v[n // 2]
    d = np.abs(r - mid(np.sort(r)))
    mad = mid(np.sort(d))
    return float(dt(1.4826) * mad if mad > 0 else dt(1.2533) * dt(d.astype(np.float64).sum() / n))


def ref_prophet_fit_robust(Y, T: int, H: int, step_s: float = 60.0, k: float = 3.0, iters: int = 5,
                           dtype=np.float64):
    """The definition of ``robust_prophet``: per row, least squares over the
    finite samples and then ``iters`` Huber-reweighted passes on K10's basis,
    each a correction ``z += (U^T W U + ridge)^-1 U^T W r``, ``r -= U dz``, with
    ``w = f min(1, k s / |r|)`` from K13's sigma ``s`` of the finite residuals
    (``s == 0`` stops the row with ``w = f``; ``k`` not finite or ``<= 0``
    keeps ``w = f``).  The ridge only conditions the solve: the right-hand side
    carries no ``- ridge z``, so the corrections converge to the unregularised
    solution (a pass leaves 1e-6 of the distance to it) instead of stopping at
    the ridge solution, whose bias ``S^-1`` carries into ``beta`` a thousandfold.
    A row with fewer than ``2 p`` finite samples (``p`` the kept rank) gets
    ``robust_moving_average_all``'s constant forecast, sigma and count.  ->
    (beta [R,32], forecast [R,H], sigma [R], nfin [R] int32, wsum [R],
    fallback [R] bool) as float64 arrays.  In fp64 ``U`` is the basis before
    ``_basis`` rounds it to fp32 for the kernels (the rounded columns only
    nearly span the design, which ``beta`` shows at 1e-5).  ``dtype=np.float32``
    takes the rounded basis and keeps ``r``, ``w``, ``G`` and ``g`` in fp32
    (the solve stays fp64): the mirror of the kernel's precision."""
    from . import misc as MI
    dt = np.dtype(dtype).type
    ut, fmap, vs, p = _basis(T, H, step_s)
    if dt is np.float64:
        Uf, S, _ = np.linalg.svd(design_matrix(T, H, step_s)[:T], full_matrices=False)     # (as in _basis)
        U = Uf * (S > S[0] * 1e-10)[None, :]
    else:
        U = ut[:, :T].T.astype(dtype)                             # [T, 32], zero columns beyond p
    y = np.asarray(Y, np.float32)[:, :T]
    R = y.shape[0]
    huber = bool(np.isfinite(k) and k > 0)
    Z = np.zeros((R, F))
    shift = np.zeros(R)
    sigma = np.full(R, np.nan)
    wsum = np.zeros(R)
    nfin = np.isfinite(y).sum(1).astype(np.int32)
    fallback = nfin < 2 * p
    ridge = LSQ_ROBUST_RIDGE * np.eye(F)
    for row in range(R):
        f = np.isfinite(y[row])
        c = y[row, 0] if f[0] else np.float32(0)
        shift[row] = c
        if fallback[row]:
            continue
        r = np.where(f, y[row].astype(dtype) - dt(c), 0).astype(dtype)
        z = np.zeros(F)
        w = f.astype(dtype)
        s = 0.0
        for _ in range(1 + int(iters)):
            wu = U * w[:, None]
            G = (wu.T @ U).astype(np.float64) + ridge
            G[np.arange(p, F), np.arange(p, F)] = 1.0
            g = (wu.T @ r).astype(np.float64)
            L = np.linalg.cholesky(G)
            dz = np.linalg.solve(L.T, np.linalg.solve(L, g))
            z += dz
            r = np.where(f, r - U @ dz.astype(dtype), 0).astype(dtype)
            s = _mad_sigma(r[f], dt)
            w = f.astype(dtype)
            if s == 0:
                break
            if huber:
                with np.errstate(divide="ignore"):
                    w = (f * np.minimum(1, dt(k * s) / np.abs(r))).astype(dtype)
        Z[row], sigma[row], wsum[row] = z, s, w.astype(np.float64).sum()
    fc = Z @ fmap.T + shift[:, None]
    beta = Z @ vs.T
    beta[:, 0] += shift
    if fallback.any():
        cen, sg, _ = MI.ref_robust_stats(y[fallback], T)
        fc[fallback] = cen[:, None]
        beta[fallback] = 0
        beta[fallback, 0] = cen
        sigma[fallback] = sg
    return beta, fc, sigma, nfin, wsum, fallback


def lsq_robust_supported(T: int) -> bool:
    """Whether the kernel holds a history of ``T`` samples in LDS."""
    return bool(LIB.load().fm_lsq_robust_supported(int(T)))


def prophet_fit_robust(Y: torch.Tensor, T: int, H: int, step_s: float = 60.0, k: float = 3.0, iters: int = 5,
                       rows: int = 0) -> LsqRobustFit:
    """K36: :func:`ref_prophet_fit_robust` on the GPU (csrc/kernels/lsq_robust.hip:
    a workgroup per ``rows`` rows, 0 = the default).  A CPU tensor, or a history
    longer than :func:`lsq_robust_supported`, goes to the reference."""
    d = Y.device
    iters = int(iters)
    check(0 <= iters <= LSQ_ROBUST_MAX_ITERS, "iters must lie in 0 ... 16")
    if not Y.is_cuda or not lsq_robust_supported(T):
        out = ref_prophet_fit_robust(Y.detach().cpu().numpy(), T, H, step_s, k, iters)
        t = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt)).to(d)
        return LsqRobustFit(t(out[0], np.float32), t(out[1], np.float32), t(out[2], np.float32), t(out[3], np.int32),
                            t(out[4], np.float32), t(out[5], np.bool_))
    require_native(Y)
    check(Y.stride(0) % 4 == 0 and Y.data_ptr() % 16 == 0, "Y rows must be 16-B aligned")
    ut, fmap, vs, rank = _basis(T, H, step_s)
    key = (T, H, step_s, str(d))
    if key not in _XT_CACHE:
        _XT_CACHE[key] = torch.from_numpy(ut).to(d)
    XT = _XT_CACHE[key]
    R = Y.shape[0]
    Z = torch.empty((R, F), dtype=torch.float32, device=d)
    sh, sigma, wsum = (torch.empty((R,), dtype=torch.float32, device=d) for _ in range(3))
    nfin, fb = (torch.empty((R,), dtype=torch.int32, device=d) for _ in range(2))
    LIB.call("fm_lsq_robust_fit", ptr(Y), Y.stride(0), int(T), R, ptr(XT), XT.stride(0), rank, float(k), iters,
             int(rows), ptr(Z), ptr(sh), ptr(sigma), ptr(nfin), ptr(wsum), ptr(fb), stream_of(Y))
    Zd, shd = Z.to(torch.float64), sh.to(torch.float64)
    fc = (Zd @ torch.from_numpy(fmap.T.copy()).to(d) + shd[:, None]).to(torch.float32)
    beta = Zd @ torch.from_numpy(vs.T.copy()).to(d)
    beta[:, 0] += shd
    beta = beta.to(torch.float32)
    fb = fb.bool()
    if bool(fb.any()):
        # the constant model of the rows that were not fitted, over those rows only
        from . import misc as MI
        idx = fb.nonzero()[:, 0]
        cen, sg, _ = MI.robust_stats(Y[idx][:, :T].contiguous(), T)
        fc[idx] = cen[:, None]
        beta[idx] = 0
        beta[idx, 0] = cen
        sigma[idx] = sg
    return LsqRobustFit(beta, fc, sigma, nfin, wsum, fb)
