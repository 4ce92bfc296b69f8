"""Edge shapes of the K2 smoothing kernels (csrc/kernels/smoothing.hip): SES,
Holt, additive / multiplicative Holt-Winters, the packed fp16 fit, the
incremental update and the fused steady step.

The reference is ``spec_es`` / ``spec_update``: a loop over the samples of one
row in fp64, written from the kernel's header comment and docs/BRAIN_SPEC.md
§3.2.  CPU tests hold the library's fp32 mirror (``SM.ref_es_fit``,
``SM.ref_es_update``) against it; GPU tests hold the kernels against it.  Every
tolerance is computed in the test from the two CPU references:

  serial   err_ref = largest relative SSE error of the fp32 mirror against the
           fp64 loop over all rows and candidates; the kernel's SSEs must be
           within max(8 err_ref, 1e-5) of the fp64 loop on every row and
           candidate.  Forecast, state and season follow the same rule with
           err_ref taken on those quantities (floor 2e-6, relative to the
           largest |forecast| of the row).
  packed   the reference is ``spec_es(park=True)`` in fp64, err_ref = largest
           relative SSE difference between that loop in fp32 and in fp64 (fp16
           roundings that fall on opposite sides of a tie), tol = 4 err_ref,
           and tol < 1e-2 is asserted on the CPU.

Winner rule: a row is near-tied when the runner-up's fp64 SSE is within 4 tol
of the best.  Exact ties go to the lowest index, other near-tied rows may take
any candidate within the margin, every other row must match ``best`` exactly;
near-tied rows are at most 25 % of a case (asserted on the fp64 loop alone).
Integer outputs (best, nobs, nfin, phase) are compared exactly.  Rows are laid
out with a row stride > T and 1e30 in the padding: a load that escapes a bound
ruins a mean.

Which GPU test enters which path, with the SSE err_ref measured for the case:

serial fit: es_fit_kernel<KIND, float>, es_forecast_kernel<float> ........... test_gpu_es_fit_edges[kind-m-T]
  0-1-97, 1-1-97       SES / Holt: Holt's trend beside a NaN neighbour, a
                       one-step row ............................. err_ref 4.6e-06, 4.7e-06
  2-2-64, 2-5-131      the plain loop (m <= 16), the 64-step flush ........ 4.2e-06, 4.1e-06
  2-12-150, 2-16-200   ..................................................... 2.2e-05, 1.6e-05
  2-17-203, 2-24-333   one 16-step chunk plus a wrap in every chunk, tails
                       with (T - t0) % 16 != 0 ............................ 1.7e-05, 1.2e-05
  2-40-421             chunks with and without a wrap ..................... 3.5e-05
  3-12-150, 3-17-203,
  3-24-333, 3-40-421   the multiplicative step, its 1e-6 guards ... 2.5e-05, 2.7e-05, 4.9e-05, 5.4e-05
  every case           row 1 shorter than two seasons (lo + m > T), row 2 ragged
                       beside uniform neighbours (GATED, materialised seasons),
                       an all-NaN row, NaN in the first season and the lap after
                       it (LAP1 reads x[t - m]), +-inf samples, a row that starts
                       at T - 2; H in {1, 6, m + 3} (H >= m: t_store_end = T);
                       keep_state both ways (NOSTORE), forecasts bit-equal; row
                       stride > T with 1e30 behind the row
  g1                   G = 1, R = 70: 64 rows a wave, a partial second wave whose
                       shadow lanes run ................................... 3.4e-06
  g64                  G = 64: one row a wave, a ragged row on the uniform path  3.4e-05
  small                G = 27 with R G < 64 ............................... 6.6e-06
  overflow             every SSE of one row past fp32: candidate 0 ........ 1.7e-05
packed fit: hw2_fit_kernel, hw2_forecast_kernel ............ test_gpu_es_fit_packed_edges[m-T-G]
  8-83, 16-163,        below the production threshold (HALF_SEASON_MIN_M
  24-250, 40-421       patched): about 10 laps, the alignment prologue on the
                       gated and on the uniform path (starts with base % 8 != 0),
                       G = 27 (odd: an idle second candidate) and 2, float4 loads
                       against xal = 0 (bit-equal), rows scaled 1e-3 .. 1e5
                       (sscale) ..................... err_ref 2.4e-04, 2.5e-04, 1.6e-04, 3.2e-04
  1000-2500, 1008-3100 the production threshold, 1.5 and 2 laps .......... 2.6e-05, 5.2e-05
update: es_update_kernel .......................................... test_gpu_es_update_edges[kind-m]
  0-1, 1-1, 2-2 .. 3-40  with and without ``slots`` (the in-place slab, untouched
                       slots bit-equal), t_new = T (nothing changes), T - 1,
                       T - 15 / 16 / 17, T - 64, T - (2 m + 3), -5 and T + 9
                       (clipped), NaN / inf among the new samples, cached phases
                       up to m - 1, H = 1 and m + 3, row stride > T, R = 257
                       (a second block) ............................ err_ref 8.0e-07 .. 1.2e-05
fused steady step: es_band_step_kernel<-1 .. 3> ................... test_gpu_es_band_step_edges[name]
  hw12   kind 2, m = 12, kmax = 17 (k > m: the LDS copy holds a phase twice), M = 5,
         S = 3, n = 65, fc written with Hf > H, cur its own tensor
  mul2   kind 3, m = 2, kmax = 16, M = 16, S = 1, n = 1, no fc, cur in place (cur_rm)
  hw17   kind 2, m = 17, kmax = 64 (the prefetch chunk on LDS), M = 1, n = 256, cap
         below the total
  mul40  kind 3, m = 40, kmax = 64, n = 64, H = 43, cur in place
  ses    kind 0, kmax = 1, S = 1, no ``diff``;  holt  kind 1, kmax = 17, M = 16
  given  kind -1: forecast and sigma are inputs, Hf > H
  every case: t_new = 0, kmax, negative, above kmax; shift != dk; lim cutting the two
         newest columns; a tail wholly off the grid; horizons below 1 and above H,
         on rewritten (d < k) and untouched seasons; NaN in the new samples and in
         the window; a NaN level (dead flag); nobs = 1 (sigma 0, score 1e30); diff;
         bound 0 .. 3; an active minlb clamp; valid 0 .. 3; lastk 0, n - 1, -1;
         par 0 then 1 (ctr[par ^ 1] comes back 0) ....... err_ref (SSE) <= 2.4e-06
launchers: the error returns of fm_es_fit and fm_es_band_step, nothing launched
         ......................................... test_smoothing_launchers_reject_bad_shapes

CPU: test_ref_es_matches_fp64_spec, test_ref_es_update_matches_fp64_spec and
test_packed_spec_tolerances hold the mirrors against the loops and yield err_ref;
test_es_bounds_reject_wrong_variants, test_step_bounds_reject_wrong_outputs and
test_step_case_reference show that the tolerances reject a loop with one rule broken.

Not reached, because nothing instantiates it: ``es_fit_kernel<KIND, _Float16>``,
``es_run_blk``, ``season_init_blk`` and ``es_forecast_kernel<_Float16>`` --
``fm_es_fit`` sends every ``season_half`` fit to ``hw2_fit_kernel``.  The scan fit
(hw_scan.hip) has its own tests; every fit here runs ``method="serial"``."""
import functools
import math

import numpy as np
import pytest
import torch

from foremast_amd.ops import reference as REF
from foremast_amd.ops import smoothing as SM
from foremast_amd.ops._lib import LIB, ptr

F32 = np.float32
F32_MAX = float(np.finfo(np.float32).max)
EPS = float(np.float32(1e-6))            # kDivEps / DIV_EPS
PAD = 1e30

FIT_CASES = [(0, 1, 97), (1, 1, 97), (2, 2, 64), (2, 5, 131), (2, 12, 150), (2, 16, 200), (2, 17, 203),
             (2, 24, 333), (2, 40, 421), (3, 12, 150), (3, 17, 203), (3, 24, 333), (3, 40, 421)]
R_FIT = 24
ROW_SHORT, ROW_RAGGED, ROW_NONE, ROW_HOLES, ROW_INF, ROW_LATE = 1, 2, 5, 7, 9, 11


# =========================================================================== the fp64 loop
def _r16(v):
    """Round to fp16, saturated at +-65504, back in the dtype of ``v``."""
    return np.clip(v, -65504.0, 65504.0).astype(np.float16).astype(v.dtype)


def spec_es(x_row, kind, m, grid, H, dtype=np.float64, park=False, park_round_init=True, broken=None):
    """One row, all candidates.  Returns a dict: sse [G] (fp64), fc [G, H], nobs
    [G], level [G], trend [G], phase (T % m) and season [G, m] (by absolute
    phase), sc (the row scale of ``park``), t0 (the first step).

    Start at the first finite sample.  Kinds >= 2: level = finite mean of the
    first season, trend = (finite mean of the second - first) / m (0 if the second
    has no finite sample), indices x - s1 or x / s1 (1 when |s1| <= 1e-6) at
    absolute phase t % m, missing -> 0 / 1.  Kinds < 2: level = first sample,
    Holt's trend = next sample - first if finite, else 0.  A missing sample:
    level += trend, nothing else changes.  ``park`` (additive only) emulates the
    packed kernel: the row in units of sc = mean |x| of the first season's finite
    samples, the closed-form updates, every stored seasonal index rounded to fp16
    (``park_round_init`` [G]: the first season's too, as threads that share a wave
    with a ragged row materialise them; a wave of rows that start together computes
    them on the fly and stores only the updated ones).
    ``broken`` breaks one rule (test_es_bounds_reject_wrong_variants)."""
    D = dtype
    x = np.asarray(x_row, F32).astype(D)
    T = x.shape[0]
    G = grid.shape[0]
    al, be, ga = (np.asarray(grid, F32)[:, i].astype(D) for i in range(3))
    if park and broken == "swap":
        sw = np.arange(G) ^ 1
        sw[sw >= G] = G - 1
        al, be, ga = al[sw], be[sw], ga[sw]
    one = D(1)
    mm = m if kind >= 2 else 1
    fin = np.isfinite(x)
    lvl = np.zeros(G, D)
    tr = np.zeros(G, D)
    S = np.zeros((G, mm), D)
    sse = np.zeros(G, np.float64)
    n = 0
    sc = D(1)
    if not fin.any():
        lvl[:] = np.nan
        t0 = T
    elif kind >= 2:
        base = int(fin.argmax())
        e1, e2 = min(base + m, T), min(base + 2 * m, T)
        f1 = x[base:e1][fin[base:e1]]
        f2 = x[e1:e2][fin[e1:e2]]
        if park:
            a1 = np.abs(f1).sum(dtype=D) / D(len(f1))
            sc = a1 if a1 > 1e-20 else one
            x = x / sc
        f1s = f1 / sc
        s1 = f1s.sum(dtype=D) / D(len(f1))
        lvl[:] = s1
        if len(f2):
            tr[:] = ((f2 / sc).sum(dtype=D) / D(len(f2)) - s1) / D(m)
            if broken == "trend":
                tr[:] = tr * D(m)
        for i in range(m):
            t = base + i
            ok = t < T and fin[t]
            if kind == 3:
                v = x[t] / s1 if ok and abs(s1) > EPS else one
            else:
                v = x[t] - s1 if ok else D(0)
            S[:, (i if broken == "init_phase" else t) % m] = v
        if park:
            S = np.where(np.broadcast_to(np.asarray(park_round_init, bool), (G,))[:, None], _r16(S), S)
        t0 = base + m
    else:
        base = int(fin.argmax())
        lvl[:] = x[base]
        if kind == 1 and base + 1 < T and fin[base + 1]:
            tr[:] = x[base + 1] - x[base]
        t0 = base + 1
    for t in range(t0, T):
        ph = t % mm
        s = S[:, ph]
        if not fin[t] and broken != "missing":
            lvl = lvl + tr
            if park:
                S[:, ph] = _r16(s)
            continue
        xt = x[t] if fin[t] else D(0)
        lt = lvl + tr
        pred = lt * s if kind == 3 else lt + s
        e = xt - pred
        sse += e.astype(np.float64) ** 2
        n += 1
        lprev = lvl
        if park:
            lvl = lt + al * e
            tr = tr + al * be * e
            s = s + ga * (one - al) * e
            if not (broken == "store" and ph == 0):
                S[:, ph] = _r16(s)
            continue
        if kind == 0:
            lvl = al * xt + (one - al) * lvl
        elif kind == 1:
            lvl = al * xt + (one - al) * lt
            tr = be * (lvl - lprev) + (one - be) * tr
        elif kind == 2:
            lvl = al * (xt - s) + (one - al) * lt
            tr = be * (lvl - lprev) + (one - be) * tr
            s = ga * (xt - lvl) + (one - ga) * s
        else:
            with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
                ds = np.where(np.abs(s) > EPS, xt / s, xt)
                lvl = al * ds + (one - al) * lt
                tr = be * (lvl - lprev) + (one - be) * tr
                dl = np.where(np.abs(lvl) > EPS, xt / lvl, one)
            s = ga * dl + (one - ga) * s
        if kind >= 2 and not (broken == "store" and ph == 0):
            S[:, ph] = s
    h = np.arange(1, H + 1)
    fc = lvl[:, None] + (h[None, :] * tr[:, None] if kind >= 1 else np.zeros((1, H), D))
    if kind >= 2:
        sv = S[:, (T + h - 1 + (1 if broken == "fc_phase" else 0)) % m]
        fc = fc * sv if kind == 3 else fc + sv
    scf = float(sc)
    return {"sse": sse * scf * scf, "fc": fc.astype(np.float64) * scf, "nobs": np.full(G, n, np.int64),
            "level": lvl.astype(np.float64) * scf, "trend": tr.astype(np.float64) * scf, "phase": T % mm,
            "season": S.astype(np.float64) * scf, "sc": scf, "t0": t0}


def spec_rows(x, T, kind, m, grid, H, rows=None, **kw):
    """``spec_es`` over the rows of x[:, :T], stacked: sse [R, G], fc [R, G, H], ..."""
    rows = range(x.shape[0]) if rows is None else rows
    ri = kw.pop("park_round_init", True)
    out = [spec_es(x[r, :T], kind, m, grid, H, park_round_init=ri[r] if np.ndim(ri) == 2 else ri, **kw) for r in rows]
    return {k: np.stack([np.asarray(o[k]) for o in out]) for k in out[0]}


# =========================================================================== inputs
def es_rows(R, T, m, seed):
    """10 + amp sin(2 pi t / max(m, 6) + phi) + 0.002 t + N(0, 0.05), amp ~ U(0.5, 2),
    a level shift of U(-1, 1) from T / 2 on (what separates the candidates), 2 %
    of the samples NaN."""
    rng = np.random.default_rng(seed)
    t = np.arange(T)
    x = (10 + rng.uniform(0.5, 2, (R, 1)) * np.sin(2 * np.pi * t / max(m, 6) + rng.uniform(0, 2 * np.pi, (R, 1)))
         + 0.002 * t + rng.normal(0, 0.05, (R, T)))
    x[:, T // 2:] += rng.uniform(-1, 1, (R, 1))
    x[rng.random((R, T)) < 0.02] = np.nan
    return x.astype(F32)


def _padded(x, pad=5):
    R, T = x.shape
    out = np.full((R, T + pad), PAD, F32)
    out[:, :T] = x
    return out


def _place(x, m, T):
    """The rows placed on purpose (see the module docstring); the clean value of a
    sample that must be finite comes from the row's neighbourhood."""
    def finite(r, t):
        if not np.isfinite(x[r, t]):
            x[r, t] = F32(10.0 + 0.002 * t)
    R = x.shape[0]
    if R > ROW_SHORT:
        x[ROW_SHORT, :T - m - 3] = np.nan
        finite(ROW_SHORT, T - m - 3)
    if R > ROW_RAGGED:
        x[ROW_RAGGED, :7] = np.nan
        finite(ROW_RAGGED, 7)
    if R > ROW_NONE:
        x[ROW_NONE] = np.nan
    if R > ROW_HOLES:
        finite(ROW_HOLES, 0)
        holes = (1, 2) if m == 1 else (m - 1, m, 2 * m - 1)
        x[ROW_HOLES, list(holes)] = np.nan
    if R > ROW_INF:
        x[ROW_INF, T // 3] = np.inf
        x[ROW_INF, T // 3 + 5] = -np.inf
    if R > ROW_LATE:
        x[ROW_LATE, :T - 2] = np.nan
        finite(ROW_LATE, T - 2)
        finite(ROW_LATE, T - 1)
    return x


def fit_rows(kind, m, T, R=R_FIT, seed=0):
    return _padded(_place(es_rows(R, T, m, 100 * kind + m + T + seed), m, T))


GRID64 = np.array([(a, b, g) for a in (0.1, 0.3, 0.6, 0.8) for b in (0.01, 0.05, 0.2, 0.4)
                   for g in (0.05, 0.2, 0.5, 0.7)], F32)
# (kind, m, T, R, grid)
WAVE_CASES = {"g1": (2, 12, 150, 70, SM.default_grid(2)[13:14]), "g64": (2, 17, 203, 12, GRID64),
              "small": (3, 12, 150, 2, None), "overflow": (2, 12, 150, R_FIT, None)}
ROW_HUGE = 3


def _case_args(case):
    """(kind, m, T, x [R, ld], grid) of a FIT_CASES tuple or a WAVE_CASES name."""
    if isinstance(case, str):
        kind, m, T, R, grid = WAVE_CASES[case]
        x = fit_rows(kind, m, T, R=R, seed=7)
        if case == "small":                           # two rows, neither tied: one clean, one ragged
            x = _padded(es_rows(R, T, m, 7))
            x[0, 0], x[1, :7], x[1, 7] = 10.0, np.nan, 10.0
        if case == "overflow":                        # every candidate's SSE of this row is past fp32
            x[ROW_HUGE, :T] *= F32(1e20)
        if case == "g1":                              # ragged rows in both waves
            x[[20, 66], :9] = np.nan
            x[[33, 68], :m + 1] = np.nan
    else:
        kind, m, T = case
        grid, x = None, fit_rows(kind, m, T)
    return kind, m, T, x, SM.default_grid(kind) if grid is None else grid


# =========================================================================== comparison
def _scale(spec, best):
    """Largest |forecast| of each row's candidate ``best`` (1 for a row without one)."""
    R = spec["fc"].shape[0]
    with np.errstate(invalid="ignore"):
        sc = np.abs(spec["fc"][np.arange(R), best]).max(1)
    return np.where(np.isfinite(sc) & (sc > 0), sc, 1.0)


def _errors(got, spec, kind, m):
    """Errors of ``got`` (sse [R, G], best, fc [R, H], and with a model: level, trend,
    season) against the fp64 loop, in the units the tolerances are stated in.  SSE:
    relative, over every row and candidate with a nonzero SSE.  The rest is taken at
    the candidate ``got`` picked, relative to the row's largest |forecast|: the trend
    times the longest horizon (what it moves a forecast by), a multiplicative index
    times the level."""
    R, G = spec["sse"].shape
    rows = np.arange(R)
    b = np.asarray(got["best"]).astype(np.int64)
    s0 = spec["sse"]
    nz = (s0 > 0) & np.isfinite(s0)
    out = {}
    gs = np.asarray(got["sse"], np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        out["sse"] = float(np.max(np.abs(gs - s0)[nz] / s0[nz], initial=0.0))
    assert not gs[s0 == 0].any(), "a candidate without a step has SSE 0"
    assert not np.isfinite(gs[~np.isfinite(s0)]).any(), "an SSE past the fp32 range is not finite"
    sc = _scale(spec, b)
    H = got["fc"].shape[1]
    f0 = spec["fc"][rows, b, :H]
    gf = np.asarray(got["fc"], np.float64)
    np.testing.assert_array_equal(np.isfinite(gf), np.isfinite(f0))
    ok = np.isfinite(f0)
    out["fc"] = float(np.max((np.abs(np.where(ok, gf - f0, 0)) / sc[:, None]), initial=0.0))
    if "level" in got:
        l0, t0 = spec["level"][rows, b], spec["trend"][rows, b]
        okr = np.isfinite(l0)
        np.testing.assert_array_equal(np.isfinite(np.asarray(got["level"])), okr)
        Hm = spec["fc"].shape[2]
        st = np.abs(np.where(okr, got["level"] - l0, 0)) / sc
        st = np.maximum(st, Hm * np.abs(np.where(okr, got["trend"] - t0, 0)) / sc)
        out["state"] = float(st.max(initial=0.0))
        if kind >= 2:
            d = np.abs(np.asarray(got["season"], np.float64) - spec["season"][rows, b])
            w = np.abs(l0)[:, None] if kind == 3 else 1.0
            d = np.where(okr[:, None], d * w, 0) / sc[:, None]     # the all-NaN row's scratch is never written
            out["season"] = float(d.max(initial=0.0))
    return out


def _winner_tol(spec, tol):
    """(best of the fp64 loop [R], near-tied [R]); non-finite SSEs are never selected,
    none finite -> candidate 0."""
    s = np.where(np.isfinite(spec["sse"]), spec["sse"], np.inf)
    best = s.argmin(1)
    if s.shape[1] == 1:
        return best, np.zeros(len(best), bool)
    two = np.sort(s, 1)[:, :2]
    with np.errstate(invalid="ignore"):
        near = ~(two[:, 1] > two[:, 0] * (1 + 4 * tol))
    return best, near


def assert_winner(best, spec, tol, what=""):
    b0, near = _winner_tol(spec, tol)
    assert near.mean() <= 0.25, f"{what}: {near.sum()} near-tied rows of {len(near)}"
    s = np.where(np.isfinite(spec["sse"]), spec["sse"], np.inf)
    best = np.asarray(best).astype(np.int64)
    for r in range(len(b0)):
        if best[r] == b0[r]:
            continue
        assert near[r], f"{what}: row {r} picked {best[r]}, the fp64 loop {b0[r]} with a clear margin"
        assert s[r, best[r]] != s[r, b0[r]], f"{what}: row {r}: an exact tie goes to the lowest index"
        assert s[r, best[r]] <= s[r, b0[r]] * (1 + 4 * tol), f"{what}: row {r} picked {best[r]} outside the margin"


def assert_fit_close(got, spec, tols, kind, m, what=""):
    """``got`` against the fp64 loop: SSEs, the winner rule, forecast, sigma, and with
    a model its state, season, SSE and the integer outputs."""
    err = _errors(got, spec, kind, m)
    print(f"{what}: errors {err} tolerances {tols}")
    assert err["sse"] <= tols["sse"], (what, "sse", err["sse"], tols["sse"])
    assert_winner(got["best"], spec, tols["sse"], what)
    R = spec["sse"].shape[0]
    rows = np.arange(R)
    b = np.asarray(got["best"]).astype(np.int64)
    for k in ("fc", "state", "season"):
        if k in err:
            assert err[k] <= tols[k], (what, k, err[k], tols[k])
    n = spec["nobs"][rows, b]
    s = spec["sse"][rows, b]
    sig0 = np.where(n > 1, np.sqrt(s / np.maximum(n - 1, 1)), 0)
    # sigma = sqrt(sse / (n - 1)): half the SSE's relative error and three fp32 roundings
    np.testing.assert_allclose(got["sigma"], sig0, rtol=0.5 * tols["sse"] + 4e-7, atol=0)
    if "nobs" in got:
        np.testing.assert_array_equal(got["nobs"], n)
        np.testing.assert_array_equal(got["phase"], np.full(R, spec["phase"][0]))
        np.testing.assert_array_equal(np.asarray(got["model_sse"]), np.asarray(got["sse"])[rows, b])
    return err


def _got_of_ref(x, T, kind, m, grid, H):
    fc, sig, best, sse, st = SM.ref_es_fit(x[:, :T], kind, H, m, grid, return_state=True)
    return {"sse": sse, "best": best, "fc": fc, "sigma": sig, "level": st["state"][:, 0], "trend": st["state"][:, 1],
            "phase": st["state"][:, 2].astype(np.int64), "season": st["season"], "nobs": st["nobs"],
            "model_sse": st["sse"]}


def _got_of_fit(r):
    g = {"sse": r.sse.cpu().numpy(), "best": r.best.cpu().numpy(), "fc": r.forecast.cpu().numpy(),
         "sigma": r.sigma.cpu().numpy()}
    if r.model is not None:
        st = r.model.state.cpu().numpy()
        g.update(level=st[:, 0], trend=st[:, 1], phase=st[:, 2].astype(np.int64), nobs=r.model.nobs.cpu().numpy(),
                 model_sse=r.model.sse.cpu().numpy(),
                 season=None if r.model.season is None else r.model.season.cpu().numpy())
    return g


def _got_of_spec(sp, best=None):
    """A (broken) loop's outputs in the shape of a fit's, rounded to fp32."""
    R, G = sp["sse"].shape
    rows = np.arange(R)
    b = _winner_tol(sp, 0.0)[0] if best is None else best
    n, s = sp["nobs"][rows, b], sp["sse"][rows, b]
    return {"sse": sp["sse"].astype(F32), "best": b, "fc": sp["fc"][rows, b].astype(F32),
            "sigma": np.where(n > 1, np.sqrt(s / np.maximum(n - 1, 1)), 0).astype(F32),
            "level": sp["level"][rows, b].astype(F32), "trend": sp["trend"][rows, b].astype(F32),
            "phase": np.full(R, sp["phase"][0]), "season": sp["season"][rows, b].astype(F32), "nobs": n,
            "model_sse": sp["sse"].astype(F32)[rows, b]}


@functools.lru_cache(maxsize=None)
def serial_case(case):
    """(kind, m, T, x, grid, the fp64 loop at H = m + 3, tolerances, err_ref) of a
    case; computed once and shared (nothing writes to it)."""
    kind, m, T, x, grid = _case_args(case)
    H = max(6, m + 3)
    spec = spec_rows(x, T, kind, m, grid, H)
    spec["sse"] = np.where(spec["sse"] > F32_MAX, np.inf, spec["sse"])      # the SSEs are fp32 outputs
    ref = _got_of_ref(x, T, kind, m, grid, H)
    err = _errors(ref, spec, kind, m)
    tols = {"sse": max(8 * err["sse"], 1e-5)}
    for k in ("fc", "state", "season"):
        if k in err:
            tols[k] = max(8 * err[k], 2e-6)
    for v in (x, *spec.values()):
        v.setflags(write=False)
    return kind, m, T, x, grid, spec, tols, err, ref


def _ids(c):
    return c if isinstance(c, str) else "-".join(map(str, c))


# =========================================================================== 1: the mirror against the loop
@pytest.mark.parametrize("case", FIT_CASES + list(WAVE_CASES), ids=_ids)
def test_ref_es_matches_fp64_spec(case):
    """The fp32 mirror and the fp64 loop are two evaluations of one recursion.  Per
    step the mirror's error in e is a few roundings of |x| <= 13: with u = 2^-24 and
    a residual of about the noise's 0.05, 16 u |x| / 0.05 = 2.5e-4 bounds the
    relative SSE error (twice that of e); a forecast is an fp32 average of the
    samples, 32 u = 1.9e-6 of the row's scale.  The measured err_ref is printed."""
    kind, m, T, x, grid, spec, tols, err, ref = serial_case(case)
    print(f"err_ref {case}: {err}")
    assert err["sse"] <= 2.5e-4 and err["fc"] <= 1.9e-6, err
    rows = np.arange(x.shape[0])
    b0, near = _winner_tol(spec, tols["sse"])
    assert near.mean() <= 0.25
    # both CPU references pick the same winner: the 4 tol margin is never needed here
    np.testing.assert_array_equal(ref["best"], b0)
    np.testing.assert_array_equal(ref["nobs"], spec["nobs"][rows, b0])
    np.testing.assert_array_equal(ref["phase"], np.full(len(rows), T % m if kind >= 2 else 0))
    assert_fit_close(ref, spec, tols, kind, m, f"mirror {case}")
    if case == "overflow":
        assert not np.isfinite(spec["sse"][ROW_HUGE]).any() and b0[ROW_HUGE] == 0 and ref["best"][ROW_HUGE] == 0
    if not isinstance(case, str):
        t0 = spec["t0"]
        assert t0[ROW_NONE] == T and (spec["nobs"][ROW_LATE] == (kind < 2)).all()
        assert t0[ROW_SHORT] + m > T or m <= 3                    # lo + m > T: no whole lap after the first


# =========================================================================== 4: the bounds reject wrong variants
VARIANT_ROWS = [0, ROW_RAGGED, 3, ROW_HOLES, ROW_INF, 4]
VARIANTS = [("fc_phase", 2), ("missing", 0), ("trend", 2), ("init_phase", 2), ("store", 2)]


@pytest.mark.parametrize("case", FIT_CASES, ids=_ids)
def test_es_bounds_reject_wrong_variants(case):
    """The loop with one rule broken falls outside the tolerances of the case: the
    forecast's phase off by one, a missing sample taken as 0, the trend without its
    / m, the first season's indices at phase i instead of (base + i) % m, the
    seasonal store dropped for phase 0."""
    kind, m, T, x, grid, spec, tols, err, ref = serial_case(case)
    sub = {k: v[VARIANT_ROWS] for k, v in spec.items()}
    assert_fit_close(_got_of_spec(sub), sub, tols, kind, m, "the loop itself")
    for name, kmin in VARIANTS:
        if kind < kmin:
            continue
        bad = spec_rows(x, T, kind, m, grid, max(6, m + 3), rows=VARIANT_ROWS, broken=name)
        with pytest.raises(AssertionError):
            assert_fit_close(_got_of_spec(bad), sub, tols, kind, m, f"{name} {case}")


# =========================================================================== 2: the serial fit
@pytest.mark.gpu
@pytest.mark.parametrize("case", FIT_CASES + list(WAVE_CASES), ids=_ids)
def test_gpu_es_fit_edges(cuda, case):
    """es_fit_kernel<KIND, float> + es_forecast_kernel<float> against the fp64 loop;
    "overflow": a row whose SSEs all overflow fp32 takes candidate 0, the rest of
    the batch is unaffected."""
    kind, m, T, x, grid, spec, tols, err, ref = serial_case(case)
    xd = torch.from_numpy(np.array(x)).to(cuda)
    nfin = np.isfinite(x[:, :T]).sum(1)
    for H in (1, 6, m + 3):
        keep = SM.es_fit(xd, T, kind, H, m, grid, keep_state=True, half_season=False, method="serial")
        drop = SM.es_fit(xd, T, kind, H, m, grid, keep_state=False, half_season=False, method="serial")
        gk, gd = _got_of_fit(keep), _got_of_fit(drop)
        assert_fit_close(gk, spec, tols, kind, m, f"{case} H={H} keep_state")
        assert_fit_close(gd, spec, tols, kind, m, f"{case} H={H}")
        # NOSTORE skips only stores that nothing reads: the same forecast bit for bit (the SSEs'
        # fp32 partial sums are flushed at other steps when the run is split at t_store_end)
        np.testing.assert_array_equal(gk["best"], gd["best"])
        np.testing.assert_array_equal(gk["fc"], gd["fc"])
        for r in (keep, drop):
            np.testing.assert_array_equal(r.nfin.cpu().numpy(), nfin)
        assert keep.best.dtype == torch.int32 and keep.model.nobs.dtype == torch.int32
    if case == "overflow":
        assert not np.isfinite(gk["sse"][ROW_HUGE]).any() and gk["best"][ROW_HUGE] == 0


# =========================================================================== 7: the launchers' error returns
@pytest.mark.gpu
def test_smoothing_launchers_reject_bad_shapes(cuda):
    """Shapes the launchers refuse before any launch."""
    x = torch.zeros((4, 64), device=cuda)
    for T, kind, m in ((23, 2, 12), (23, 3, 12), (1, 0, 1), (1, 1, 1)):           # 2 m > T; T < 2
        with pytest.raises(RuntimeError):
            SM.es_fit(x, T, kind, 3, m, half_season=False, method="serial")
    d = torch.zeros((4096,), device=cuda)
    p = ptr(d)
    st = torch.cuda.current_stream(cuda).cuda_stream

    def fit(m, kind, half):
        LIB.call("fm_es_fit", p, 64, 64, 4, p, 3, m, kind, p, p, p, p, 3, p, p, p, 0, half, p, p, st)

    for m, kind in ((12, 2), (20, 2), (16, 3)):                                     # season_half: additive, m % 8 == 0
        with pytest.raises(RuntimeError):
            fit(m, kind, 1)

    def step(M=2, n=8, kmax=4, T=64, kind=2):
        LIB.call("fm_es_band_step", p, 64, p, p, p, 0, T, kmax, p, p, p, 12, kind, p, p, p, p, p, 8, n, p, 3, 1, M,
                 p, p, p, None, 0.8, p, p, p, p, p, None, 0, p, 16, p, 0, p, p, None, None, st)

    for kw in ({"M": 17}, {"n": 257}, {"kmax": 65}, {"kmax": 8, "T": 7}, {"M": 0}, {"n": 0}, {"kmax": 0}):
        with pytest.raises(RuntimeError):
            step(**kw)
    torch.cuda.synchronize()


# =========================================================================== 3: the packed fp16 fit
PACKED_CASES = [(8, 83), (16, 163), (24, 250), (40, 421), (1000, 2500), (1008, 3100)]
PACKED_G = (27, 2)
PACKED_SEED = {8: 4000}       # drawn again where the first draw had more than 25 % near-tied rows


def _ceil4(T):
    return (T + 3) // 4 * 4


def packed_rows(m, T):
    """The rows of the serial cases scaled by geomspace(1e-3, 1e5) across the batch.
    Small m: rows 13..18 start together at sample 3 -- with G = 27 (14 threads a
    row) threads 192..255, a whole wave, lie in them, so that wave takes the
    uniform path with the alignment prologue (phase 3).  Production m: 6 rows, row
    1 starts at sample 13."""
    if m < 1000:
        x = es_rows(R_FIT, T, m, 31 * m + T + PACKED_SEED.get(m, 0))
        x[13:19, :3], x[13:19, 3] = np.nan, 10.0
        x = _place(x, m, T)
    else:
        x = es_rows(6, T, m, 31 * m + T)
        x[1, :13], x[1, 13] = np.nan, 10.0
    return (x * np.geomspace(1e-3, 1e5, x.shape[0])[:, None]).astype(F32)


def packed_round_init(t0, T, m, G):
    """[R, G]: whether the thread of (row, candidate) materialises its first season
    in the fp16 scratch.  Thread row * ceil(G / 2) + j runs candidates 2 j, 2 j + 1;
    a wave (64 threads, the last one padded with copies of the last thread) whose
    threads all start at the same step, a season before the end, does not."""
    R, GP = len(t0), (G + 1) // 2
    NT = R * GP
    out = np.ones((R, 2 * GP), bool)
    for w0 in range(0, NT, 64):
        tid = np.minimum(np.arange(w0, w0 + 64), NT - 1)
        ts = t0[tid // GP]
        if ts.min() == ts.max() and ts.min() + m <= T:
            out[tid // GP, 2 * (tid % GP)] = out[tid // GP, 2 * (tid % GP) + 1] = False
    return out[:, :G]


@functools.lru_cache(maxsize=None)
def packed_case(m, T, G):
    """(x, grid, H, the packed fp64 loop, tolerances, err_ref) of a case."""
    grid = SM.default_grid(2) if G == 27 else SM.default_grid(2)[[4, 22]]
    x = packed_rows(m, T)
    H = m + 3 if m < 1000 else 6
    fin = np.isfinite(x)
    base = np.where(fin.any(1), fin.argmax(1), T)
    ri = packed_round_init(np.where(base < T, base + m, T), T, m, G)
    s64 = spec_rows(x, T, 2, m, grid, H, park=True, park_round_init=ri)
    s32 = spec_rows(x, T, 2, m, grid, H, park=True, park_round_init=ri, dtype=np.float32)
    err = _errors(_got_of_spec(s32), s64, 2, m)
    if G != 27:
        # two candidates are too few to meet a tie: err_ref is the one of the same rows under the whole grid
        err = packed_case(m, T, 27)[5]
    rel = float((s64["sc"] / _scale(s64, _winner_tol(s64, 0.0)[0])).max())
    # a seasonal index is stored to one fp16 step of the row scale: 2^-11 sc (indices are below sc)
    step = 2.0 ** -11 * rel
    # level and indices share the first season's mean s1 with opposite signs (the forecast is free of
    # it, and of its error, for good); both loops sum pairwise, a kernel may add the m samples in
    # order: (m - 1) u of mean |x| bounds what that moves s1 by
    mean = (m - 1) * 2.0 ** -24 * rel
    tols = {"sse": 4 * err["sse"], "state": max(4 * err["state"], 2e-6) + mean, "season": step + mean,
            "fc": max(4 * err["fc"], 2e-6) + step}
    for v in (x, *s64.values()):
        v.setflags(write=False)
    return x, grid, H, s64, tols, err


@pytest.mark.parametrize("G", PACKED_G)
@pytest.mark.parametrize("m,T", PACKED_CASES)
def test_packed_spec_tolerances(m, T, G):
    """The packed tolerance is usable (tol < 1e-2, otherwise draw another seed), the
    near-tie cap holds, and the loop with the two candidates of a thread swapped
    falls outside it."""
    x, grid, H, spec, tols, err = packed_case(m, T, G)
    print(f"err_ref packed {m}-{T}-{G}: {err}")
    assert 0 < tols["sse"] < 1e-2
    assert_fit_close(_got_of_spec(spec), spec, tols, 2, m, "the loop itself")
    assert spec["sc"].min() > 0
    if m < 1000:
        rows = [0, ROW_RAGGED, 14, ROW_INF]
        sub = {k: v[rows] for k, v in spec.items()}
        bad = spec_rows(x, T, 2, m, grid, H, rows=rows, park=True, broken="swap")
        with pytest.raises(AssertionError):
            assert_fit_close(_got_of_spec(bad), sub, tols, 2, m, "swap")


@pytest.mark.gpu
@pytest.mark.parametrize("G", PACKED_G)
@pytest.mark.parametrize("m,T", PACKED_CASES)
def test_gpu_es_fit_packed_edges(cuda, monkeypatch, m, T, G):
    """hw2_fit_kernel + hw2_forecast_kernel against the packed fp64 loop, from a
    16-byte-aligned tensor (float4 loads) and from a view with an odd row stride
    (xal = 0): bit-identical."""
    if m < 1000:
        monkeypatch.setattr(SM, "HALF_SEASON_MIN_M", 8)
    x, grid, Hmax, spec, tols, err = packed_case(m, T, G)
    R = x.shape[0]
    xt = torch.from_numpy(np.array(x)).to(cuda)
    al = torch.full((R, _ceil4(T) + 4), PAD, device=cuda)
    al[:, :T] = xt
    big = torch.full((R, T + 7 - T % 2), PAD, device=cuda)
    un = big[:, 1:1 + T]
    un.copy_(xt)
    assert al.data_ptr() % 16 == 0 and al.stride(0) % 4 == 0 and un.data_ptr() % 16 == 4 and un.stride(0) % 2 == 1
    nfin = np.isfinite(x).sum(1)
    for H in ((1, 6, Hmax) if m < 1000 else (Hmax,)):
        got = {}
        for keep in (True, False):
            ra = SM.es_fit(al, T, 2, H, m, grid, keep_state=keep, half_season=True, method="serial")
            ru = SM.es_fit(un, T, 2, H, m, grid, keep_state=keep, half_season=True, method="serial")
            ga, gu = _got_of_fit(ra), _got_of_fit(ru)
            for k in ga:                          # (a row without a sample never writes its scratch)
                a, u = (v[nfin > 0] if k == "season" else v for v in (ga[k], gu[k]))
                np.testing.assert_array_equal(a, u, err_msg=f"aligned against unaligned: {k}")
            np.testing.assert_array_equal(ra.nfin.cpu().numpy(), nfin)
            np.testing.assert_array_equal(ru.nfin.cpu().numpy(), nfin)
            assert_fit_close(ga, spec, tols, 2, m, f"packed {m}-{T}-{G} H={H} keep={keep}")
            got[keep] = ga
        np.testing.assert_array_equal(got[True]["best"], got[False]["best"])
        np.testing.assert_array_equal(got[True]["fc"], got[False]["fc"])
    # sscale = mean |x| of the first season's finite samples (1 for a row without one), to the (m - 1) u of
    # a sum in order and the division; nobs of every candidate; an odd G's idle candidate stores nothing
    sscale, nobs, guards = _packed_raw(al, T, m, grid, 1)
    np.testing.assert_allclose(sscale, spec["sc"], rtol=(m + 2) * 2.0 ** -24, atol=0)
    np.testing.assert_array_equal(nobs, spec["nobs"])
    assert guards == [7.0, 7.0, 7.0, 7.0, 7]


def _packed_raw(x, T, m, grid, H):
    """The launch of ``SM.es_fit`` for the packed kernel with its buffers handed back:
    (sscale [R], nobs [R, G], the guard elements behind sse / state / nobs)."""
    d, R, G = x.device, x.shape[0], grid.shape[0]
    P, GP = R * G, (G + 1) // 2
    cand = torch.from_numpy(grid).to(d)
    season = torch.empty((m // 8, R * GP, 16), dtype=torch.float16, device=d)
    sse, state = torch.full((P + 1,), 7.0, device=d), torch.full((P + 1, 3), 7.0, device=d)
    nobs = torch.full((P + 1,), 7, dtype=torch.int32, device=d)
    sscale, fc, sig = torch.empty((R,), device=d), torch.empty((R, H), device=d), torch.empty((R,), device=d)
    best, nfin = (torch.empty((R,), dtype=torch.int32, device=d) for _ in range(2))
    LIB.call("fm_es_fit", ptr(x), x.stride(0), T, R, ptr(cand), G, m, 2, ptr(season), ptr(sse), ptr(state), ptr(nobs),
             H, ptr(fc), ptr(sig), ptr(best), 1, 1, ptr(sscale), ptr(nfin), torch.cuda.current_stream(d).cuda_stream)
    torch.cuda.synchronize()
    guards = [float(sse[P]), *state[P].tolist(), int(nobs[P])]
    return sscale.cpu().numpy(), nobs[:P].reshape(R, G).cpu().numpy(), guards


# =========================================================================== 5: the incremental update
UPDATE_CASES = [(k, m) for k in (0, 1) for m in (1,)] + [(k, m) for k in (2, 3) for m in (2, 12, 17, 40)]
R_UPD = 257


def spec_update(x_row, t_new, kind, m, par, level, trend, phase, season, sse, nobs, H):
    """One cached model over its new samples x_row[t_new:], in fp64; the first new
    sample has the cached phase.  Returns (level, trend, phase, season, sse, nobs,
    forecast [H], sigma)."""
    T = len(x_row)
    t0 = min(max(int(t_new), 0), T)
    al, be, ga = (float(v) for v in par)
    lvl, tr, e2, n = float(level), float(trend), float(sse), int(nobs)
    ph = int(phase) if kind >= 2 else 0
    S = [float(v) for v in season] if kind >= 2 else [0.0]
    for t in range(t0, T):
        xt = float(x_row[t])
        s = S[ph] if kind >= 2 else 0.0
        if math.isfinite(xt):
            lt = lvl + tr
            e = xt - (lt * s if kind == 3 else lt + s)
            e2 += e * e
            n += 1
            lprev = lvl
            if kind == 0:
                lvl = al * xt + (1 - al) * lvl
            elif kind == 3:
                lvl = al * (xt / s if abs(s) > EPS else xt) + (1 - al) * lt
            else:
                lvl = al * (xt - s) + (1 - al) * lt
            if kind >= 1:
                tr = be * (lvl - lprev) + (1 - be) * tr
            if kind == 2:
                S[ph] = ga * (xt - lvl) + (1 - ga) * s
            elif kind == 3:
                S[ph] = ga * (xt / lvl if abs(lvl) > EPS else 1.0) + (1 - ga) * s
        else:
            lvl = lvl + tr
        if kind >= 2:
            ph = (ph + 1) % m
    fc = []
    for h in range(1, H + 1):
        f = lvl + (h * tr if kind >= 1 else 0.0)
        if kind >= 2:
            sv = S[(ph + h - 1) % m]
            f = f * sv if kind == 3 else f + sv
        fc.append(f)
    return lvl, tr, ph, S, e2, n, fc, (math.sqrt(e2 / (n - 1)) if n > 1 else 0.0)


@functools.lru_cache(maxsize=None)
def update_case(kind, m):
    """Models of a CPU fit with phases spread over 0 .. m - 1, new samples [R, T]
    with NaN and inf among them, t_new cycling through its edge values; the fp64
    update, the mirror's, and the tolerances."""
    R, H = R_UPD, m + 3
    Th = 3 * m + 20
    T = max(64, 2 * m + 3) + 5
    rng = np.random.default_rng(50 + 10 * kind + m)
    y = es_rows(R, Th + T, m, 700 + 10 * kind + m)
    y[:, 0] = 10.0
    fit = SM.es_fit(torch.from_numpy(y[:, :Th].copy()), Th, kind, H, m, keep_state=True)
    md = fit.model
    if kind >= 2:
        md.state[:, 2] = torch.from_numpy(((m - 1 - np.arange(R)) % m).astype(F32))     # rows 0, m, ..: phase m - 1
    x = y[:, Th:].copy()
    x[rng.random((R, T)) < 0.05] = np.nan
    x[rng.random((R, T)) < 0.01] = np.inf
    x[rng.random((R, T)) < 0.01] = -np.inf
    x = _padded(x)
    edges = [T, T - 1, T - 15, T - 16, T - 17, T - 64, T - (2 * m + 3), -5, T + 9]
    t_new = np.array([edges[r % len(edges)] for r in range(R)], np.int32)
    par, st0 = md.params.numpy(), md.state.numpy()
    sea0 = md.season.numpy() if kind >= 2 else np.zeros((R, 1), F32)
    spec = _spec_update_rows(x, T, t_new, kind, m, par, st0, sea0, md.sse.numpy(), md.nobs.numpy(), H)
    fc, sig, new = SM.es_update(torch.from_numpy(x), T, torch.from_numpy(t_new), md, H)
    err = _update_errors(_got_of_update(fc, sig, new), spec, kind)
    tols = {"sse": max(8 * err["sse"], 1e-5), "fc": max(8 * err["fc"], 2e-6), "state": max(8 * err["state"], 2e-6),
            "season": max(8 * err.get("season", 0), 2e-6)}
    return x, T, t_new, md, H, spec, tols, err


def _got_of_update(fc, sig, md):
    st = md.state.cpu().numpy()
    return {"fc": fc.cpu().numpy(), "sigma": sig.cpu().numpy(), "level": st[:, 0], "trend": st[:, 1],
            "phase": st[:, 2].astype(np.int64), "sse": md.sse.cpu().numpy(), "nobs": md.nobs.cpu().numpy(),
            "season": None if md.season is None else md.season.cpu().numpy()}


def _update_errors(got, spec, kind):
    """As ``_errors``: the SSE relative, the rest relative to the row's largest
    |forecast| of the fp64 update."""
    H = got["fc"].shape[1]
    sc = np.abs(spec["fc"]).max(1)
    nz = spec["sse"] > 0
    out = {"sse": float(np.max(np.abs(got["sse"].astype(np.float64) - spec["sse"])[nz] / spec["sse"][nz], initial=0)),
           "fc": float((np.abs(got["fc"] - spec["fc"][:, :H]) / sc[:, None]).max())}
    Hm = spec["fc"].shape[1]
    out["state"] = float(np.maximum(np.abs(got["level"] - spec["level"]),
                                    Hm * np.abs(got["trend"] - spec["trend"])).__truediv__(sc).max())
    if kind >= 2:
        w = np.abs(spec["level"])[:, None] if kind == 3 else 1.0
        out["season"] = float((np.abs(got["season"] - spec["season"]) * w / sc[:, None]).max())
    return out


def assert_update_close(got, spec, tols, kind, what):
    err = _update_errors(got, spec, kind)
    print(f"{what}: errors {err} tolerances {tols}")
    for k, v in err.items():
        assert v <= tols[k], (what, k, v, tols[k])
    np.testing.assert_array_equal(got["nobs"], spec["nobs"])
    np.testing.assert_array_equal(got["phase"], spec["phase"])
    np.testing.assert_allclose(got["sigma"], spec["sigma"], rtol=0.5 * tols["sse"] + 4e-7, atol=0)


@pytest.mark.parametrize("kind,m", UPDATE_CASES)
def test_ref_es_update_matches_fp64_spec(kind, m):
    """``SM.ref_es_update`` against the fp64 update: the err_ref of the update's
    tolerances, with the bounds of test_ref_es_matches_fp64_spec."""
    x, T, t_new, md, H, spec, tols, err = update_case(kind, m)
    print(f"err_ref update {kind}-{m}: {err}")
    assert err["sse"] <= 2.5e-4 and err["fc"] <= 1.9e-6, err
    assert np.isfinite(spec["fc"]).all() and (spec["nobs"] > 1).all()


def _to(md, dev):
    return SM.ESState(md.kind, md.m, *(None if t is None else t.to(dev).contiguous() for t in
                                       (md.params, md.state, md.season, md.sse, md.nobs)))


@pytest.mark.gpu
@pytest.mark.parametrize("kind,m", UPDATE_CASES)
def test_gpu_es_update_edges(cuda, kind, m):
    """es_update_kernel row by row and through ``slots`` into a slab, against the
    fp64 update."""
    x, T, t_new, md, Hmax, spec, tols, err = update_case(kind, m)
    R = x.shape[0]
    xd = torch.from_numpy(np.array(x)).to(cuda)
    tn = torch.from_numpy(t_new)
    dm = _to(md, cuda)
    same = t_new >= T                                    # no new sample (T and the clipped T + 9)
    assert same.sum() >= 2 * (R // 9)
    fields = ("params", "state", "sse", "nobs") + (("season",) if kind >= 2 else ())
    for H in (1, Hmax):
        fc, sig, new = SM.es_update(xd, T, tn, dm, H)
        got = _got_of_update(fc, sig, new)
        assert_update_close(got, spec, tols, kind, f"update {kind}-{m} H={H}")
        for f in fields:                                 # untouched models: bit-identical
            np.testing.assert_array_equal(getattr(new, f).cpu().numpy()[same], getattr(md, f).numpy()[same], err_msg=f)
            np.testing.assert_array_equal(getattr(dm, f).cpu().numpy(), getattr(md, f).numpy(), err_msg=f)
        # the slab the model cache uses: C = R + 7 slots, row r advances slot slots[r] in place
        C = R + 7
        rng = np.random.default_rng(m)
        slots = torch.from_numpy(rng.permutation(C)[:R].astype(np.int64))
        slab = SM.ESState(kind, m, *(None if t is None else
                                     torch.full((C,) + tuple(t.shape[1:]), 7, dtype=t.dtype, device=cuda)
                                     for t in (dm.params, dm.state, dm.season, dm.sse, dm.nobs)))
        for f in fields:
            getattr(slab, f)[slots.to(cuda)] = getattr(dm, f)
        before = {f: getattr(slab, f).cpu().numpy().copy() for f in fields}
        fc2, sig2, out = SM.es_update(xd, T, tn, slab, H, slots=slots)
        assert out is slab
        np.testing.assert_array_equal(fc2.cpu().numpy(), got["fc"])
        np.testing.assert_array_equal(sig2.cpu().numpy(), got["sigma"])
        free = np.setdiff1d(np.arange(C), slots.numpy())
        for f in fields:
            after = getattr(slab, f).cpu().numpy()
            np.testing.assert_array_equal(after[free], before[f][free], err_msg=f"untouched slots: {f}")
            np.testing.assert_array_equal(after[slots.numpy()], getattr(new, f).cpu().numpy(), err_msg=f)


# =========================================================================== 6: the fused steady step
PAIR_FACTOR = 0.8
STEP_MARGIN = 0.05
STEP_CASES = {   # Hf = 0: no forecast output; cap = None: room for every anomaly
    "hw12": dict(kind=2, m=12, M=5, S=3, kmax=17, n=65, H=6, Hf=8, inplace=False, cap=None),
    "mul2": dict(kind=3, m=2, M=16, S=1, kmax=16, n=1, H=3, Hf=0, inplace=True, cap=None),
    "hw17": dict(kind=2, m=17, M=1, S=3, kmax=64, n=256, H=20, Hf=20, inplace=False, cap=40),
    "mul40": dict(kind=3, m=40, M=5, S=3, kmax=64, n=64, H=43, Hf=0, inplace=True, cap=None),
    "ses": dict(kind=0, m=1, M=5, S=1, kmax=1, n=64, H=4, Hf=4, inplace=False, cap=None),
    "holt": dict(kind=1, m=1, M=16, S=3, kmax=17, n=65, H=5, Hf=7, inplace=True, cap=None),
    "given": dict(kind=-1, m=1, M=5, S=3, kmax=1, n=65, H=5, Hf=7, inplace=False, cap=None),
}
ROW_DEAD, ROW_SIG0, ROW_EMPTY = 1, 2, 4          # NaN level; nobs 1 and no new sample; a tail wholly off the grid


def _spec_update_rows(x, T, t_new, kind, m, par, st0, sea0, sse0, nobs0, H):
    sp = [spec_update(x[r, :T], t_new[r], kind, m, par[r], st0[r, 0], st0[r, 1], st0[r, 2], sea0[r], sse0[r],
                      nobs0[r], H) for r in range(x.shape[0])]
    keys = ("level", "trend", "phase", "season", "sse", "nobs", "fc", "sigma")
    return {k: np.array([o[i] for o in sp]) for i, k in enumerate(keys)}


@functools.lru_cache(maxsize=None)
def step_case(name):
    """Inputs of one fm_es_band_step launch and its reference: the tail from the
    grid by the kernel comment's rule, the fp64 update, the centre at clamp(hor, 1,
    H), ``SM.ref_band_decide`` with the history gate, ``reference.service_reduce``."""
    c = dict(STEP_CASES[name])
    kind, m, M, S, kmax, n, H, Hf = (c[k] for k in ("kind", "m", "M", "S", "kmax", "n", "H", "Hf"))
    R = S * M
    rng = np.random.default_rng(sum(map(ord, name)))
    T, dk = kmax + 9, 2
    Rg, wc = R + 2, T + 16                       # grid rows; first column of the current window (in place)
    ld = wc + n + 3
    buf = rng.normal(10, 0.3, (Rg, ld)).astype(F32)
    buf[:, :wc][rng.random((Rg, wc)) < 0.05] = np.nan
    rm = rng.permutation(Rg)[:R].astype(np.int32)
    off = rng.integers(-2, 3, R)
    lim = np.full(R, T + 8 - dk)
    cut = np.arange(R) % 7 == 3
    lim[cut] = (T - 2 + off - dk)[cut]           # lim cuts the two newest columns off
    if R > ROW_EMPTY:
        off[ROW_EMPTY] = -(T + 5)
    shift = (dk - off).astype(np.int32)
    edges = [0, kmax, -3, kmax + 5, kmax // 2, min(1, kmax - 1), kmax - 1]
    t_new = np.array([edges[r % len(edges)] for r in range(R)], np.int32)
    col = T - kmax + np.arange(kmax)[None, :] + off[:, None]
    okc = (col >= 0) & (col < (lim + dk)[:, None])
    xs = np.where(okc, buf[rm[:, None], np.clip(col, 0, ld - 1)], np.nan).astype(F32)
    Hx = max(H, Hf)
    c.update(R=R, T=T, dk=dk, ld=ld, wc=wc, buf=buf, rm=rm, shift=shift, lim=lim.astype(np.int32), t_new=t_new,
             xs=xs, Hx=Hx)
    if kind >= 0:
        Th = 3 * m + 20
        y = es_rows(R, Th, m, 900 + sum(map(ord, name)))
        y[:, 0] = 10.0
        md = SM.es_fit(torch.from_numpy(y), Th, kind, Hx, m, keep_state=True).model
        par, st0 = md.params.numpy().copy(), md.state.numpy().copy()
        sea0 = md.season.numpy().copy() if kind >= 2 else np.zeros((R, 1), F32)
        sse0, nobs0 = md.sse.numpy().copy(), md.nobs.numpy().copy()
        if kind >= 2:
            st0[:, 2] = (m - 1 - np.arange(R)) % m
        st0[ROW_DEAD, 0] = np.nan
        nobs0[ROW_SIG0], t_new[ROW_SIG0] = 1, kmax
        spec = _spec_update_rows(xs, kmax, t_new, kind, m, par, st0, sea0, sse0, nobs0, Hx)
        st = {"state": st0.copy(), "season": sea0.copy(), "sse": sse0.astype(np.float64),
              "nobs": nobs0.astype(np.int64)}
        with np.errstate(invalid="ignore"):
            fcm, sgm = SM.ref_es_update(xs, t_new, kind, m, par, st, Hx)
        live = np.isfinite(spec["level"])
        assert live.sum() == R - 1
        mir = {"fc": fcm, "sigma": sgm, "level": st["state"][:, 0], "trend": st["state"][:, 1], "sse": st["sse"],
               "season": st["season"]}
        err = _update_errors({k: v[live] for k, v in mir.items()}, {k: v[live] for k, v in spec.items()}, kind)
        tols = {"sse": max(8 * err["sse"], 1e-5), "fc": max(8 * err["fc"], 2e-6),
                "state": max(8 * err["state"], 2e-6), "season": max(8 * err.get("season", 0), 2e-6)}
        C = R + 3
        slots = rng.permutation(C)[:R].astype(np.int64)
        slab = {k: np.full((C,) + v.shape[1:], 7, v.dtype) for k, v in
                (("params", par), ("state", st0), ("season", sea0), ("sse", sse0), ("nobs", nobs0))}
        for k, v in (("params", par), ("state", st0), ("season", sea0), ("sse", sse0), ("nobs", nobs0)):
            slab[k][slots] = v
        c.update(spec=spec, slots=slots, slab=slab, live=live, C=C)
        fc64, sig64 = spec["fc"], spec["sigma"]
    else:
        fc_in = (10 + rng.normal(0, 1, (R, Hf))).astype(F32)
        sig_in = rng.uniform(0.05, 0.3, R).astype(F32)
        sig_in[ROW_SIG0], fc_in[ROW_DEAD] = 0, np.nan
        tols = {"sse": 0.0, "fc": 0.0}
        c.update(fc_in=fc_in, sig_in=sig_in, live=np.ones(R, bool))
        fc64, sig64 = fc_in.astype(np.float64), sig_in.astype(np.float64)
    hor = rng.integers(-2, H + 4, (R, n)).astype(np.int64)
    cen = np.take_along_axis(fc64, np.clip(hor, 1, H) - 1, 1)
    thr = rng.choice([1.0, 2.0, 3.0], M).astype(F32)
    bound = (np.arange(M) % 4)[::-1].astype(np.int32).copy()          # 3, 2, 1, 0, ...
    if M == 1:
        bound[:] = 3
    minlb = np.full(M, -1e9, F32)
    minlb[M // 2] = 9.5                                               # an active clamp
    diff = (np.arange(R) % 3 == 1).astype(np.int8) if name != "ses" else None
    valid = np.where(np.arange(R) % 5 == 4, np.arange(R) // 5 % 3, 3).astype(np.int32)     # rows 4, 9, 14: 0, 1, 2
    lastk = np.array([(0, n - 1, -1, n // 2)[r % 4] for r in range(R)], np.int64)
    c32, s32 = cen.astype(F32), sig64.astype(F32)

    def band(cur):
        return tuple(v.numpy() for v in SM.ref_band_decide(cur, c32, s32, M, thr, bound, minlb, diff, PAIR_FACTOR))

    with np.errstate(invalid="ignore"):
        up, lo = band(c32)[:2]
        th = (up - c32) / np.where(s32 > 0, s32, 1)[:, None]
        q = (0.25 * th * s32[:, None]).astype(np.float64)             # centre +- j q, j = 4 is the cut
        d = rng.choice([-3, -2, -1, 1, 2, 3, 4], (R, n))
        cur = np.where(rng.random((R, n)) < 0.5, up + d * q, lo - d * q)
        flat = ~(s32 > 0)[:, None] & np.ones((1, n), bool)
        cur = np.where(flat, c32 + rng.choice([-1.0, 1.0], (R, n)), cur)
        room = 2 * STEP_MARGIN * s32[:, None]
        near = (np.abs(cur - up) <= room) | (np.abs(cur - lo) <= room)
        cur = np.where(near & ~flat, np.maximum(up, lo) + 2 * q + 0.5 * s32[:, None], cur).astype(F32)
    cur[rng.random((R, n)) < 0.05] = np.nan
    cur[0, 0] = np.inf if n > 1 else cur[0, 0]
    cur[R - 1, n - 1] = np.nan                                        # a newest point that is not finite
    up, lo, words, count, score = band(cur)
    fin = np.isfinite(cur) & np.isfinite(c32)
    with np.errstate(invalid="ignore"):
        gap = np.minimum(np.abs(cur - up), np.abs(cur - lo))
        assert (gap[fin] > (STEP_MARGIN * np.broadcast_to(s32[:, None], gap.shape))[fin]).all()
    flag = _unpack_words(words, n)
    gate = (valid & 1) != 0
    flag &= gate[:, None]
    count = np.where(gate, count, 0).astype(np.int32)
    c.update(hor=hor, thr=thr, bound=bound, minlb=minlb, diff=diff, valid=valid, lastk=lastk, cur=cur, cen=cen,
             sig64=sig64, up=up, lo=lo, flag=flag, count=count, score=score, tols=tols,
             packed=REF.service_reduce(count, score, valid, M))
    assert flag.sum() > 0 or n == 1
    return c


def _unpack_words(words, n):
    w = np.ascontiguousarray(words).view(np.uint64)
    bits = np.unpackbits(w.view(np.uint8).reshape(w.shape[0], -1), axis=1, bitorder="little")
    return bits[:, :n].astype(bool)


def _band_step(dev, c, par, ctr, slab=None):
    """One launch, in the argument order of engine/fp_models.py::_fused_launch;
    hostv is unpacked as there: packed [S, 4] | stats [R, 4] | count [R] | dead [R]."""
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    R, S, M, n, kind = c["R"], c["S"], c["M"], c["n"], c["kind"]
    buf = t(c["buf"])
    rm = t(c["rm"])
    if c["inplace"]:
        buf[rm.long(), c["wc"]:c["wc"] + n] = t(c["cur"])
        cur, cur_p, ld_c, cur_rm = None, buf.data_ptr() + 4 * c["wc"], c["ld"], ptr(rm)
    else:
        cur = torch.full((R, n + 3), PAD, device=dev)
        cur[:, :n] = t(c["cur"])
        cur_p, ld_c, cur_rm = ptr(cur), n + 3, None
    g = {k: t(c[k]) for k in ("shift", "lim", "t_new", "hor", "thr", "bound", "minlb", "diff", "valid", "lastk")}
    if kind >= 0:
        slab = {k: t(v) for k, v in c["slab"].items()} if slab is None else slab
        slots = t(c["slots"])
        sig = torch.full((R,), 7.0, device=dev)
        fc = torch.full((R, c["Hf"]), 7.0, device=dev) if c["Hf"] else None
    else:
        slots, sig, fc = None, t(c["sig_in"]), t(c["fc_in"])
    up, lo = (torch.full((R, n), 7.0, device=dev) for _ in range(2))
    hostv = torch.full((S * 4 + R * 6 + 2,), 7.0, device=dev)
    total = int(c["count"].sum())
    cap = c["cap"] or max(total, 1) + 5
    out_idx = torch.full((cap + 8, 4), -7, dtype=torch.int32, device=dev)
    out_val = torch.full((cap + 8,), 7.0, device=dev)
    last3 = torch.full((3, R), 7.0, device=dev)
    sp = (lambda k: ptr(slab[k]) if slab is not None else None)       # noqa: E731
    LIB.call("fm_es_band_step", ptr(buf), c["ld"], ptr(rm), ptr(g["shift"]), ptr(g["lim"]), c["dk"], c["T"],
             c["kmax"], ptr(g["t_new"]) if kind >= 0 else None, ptr(slots), sp("params"), c["m"], kind,
             sp("season") if kind >= 2 else None, sp("sse"), sp("state"), sp("nobs"), cur_p, ld_c, n, ptr(g["hor"]),
             c["H"], S, M, ptr(g["thr"]), ptr(g["bound"]), ptr(g["minlb"]), ptr(g["diff"]), PAIR_FACTOR,
             ptr(g["valid"]), ptr(g["lastk"]), ptr(up), ptr(lo), ptr(sig), ptr(fc), c["Hf"] if fc is not None else 0,
             ptr(hostv), cap, ptr(ctr), par, ptr(out_idx), ptr(out_val), ptr(last3), cur_rm,
             torch.cuda.current_stream(dev).cuda_stream)
    torch.cuda.synchronize()
    hn = hostv.cpu().numpy()
    ints = hn[S * 4 + R * 4:].view(np.int32)
    return {"packed": hn[:S * 4].reshape(S, 4), "stats": hn[S * 4:S * 4 + R * 4].reshape(R, 4), "count": ints[:R],
            "dead": ints[R:2 * R], "up": up.cpu().numpy(), "lo": lo.cpu().numpy(), "sigma": sig.cpu().numpy(),
            "fc": None if fc is None else fc.cpu().numpy(), "idx": out_idx.cpu().numpy(), "val": out_val.cpu().numpy(),
            "last3": last3.cpu().numpy(), "ctr": ctr.cpu().numpy(), "cap": cap, "slab": slab}


def _assert_step(c, g, what):
    R, S, M, n, kind, H = c["R"], c["S"], c["M"], c["n"], c["kind"], c["H"]
    tols, live, sig, cen = c["tols"], c["live"], c["sig64"], c["cen"]
    with np.errstate(invalid="ignore"):
        scale = np.where(live, np.abs(c["spec"]["fc"]).max(1), 1.0) if kind >= 0 else np.ones(R)
    tsig = 0.5 * tols["sse"] + 4e-7
    # ---- the integer outputs: exact
    np.testing.assert_array_equal(g["count"], c["count"], err_msg=what)
    dead = ~live if kind >= 0 else np.zeros(R, bool)
    np.testing.assert_array_equal(g["dead"], dead.astype(np.int32))
    np.testing.assert_array_equal(g["packed"][:, [0, 2, 3]], c["packed"][:, [0, 2, 3]])
    # ---- sigma, forecast, bands: the serial rule
    if kind >= 0:
        np.testing.assert_array_equal(np.isfinite(g["sigma"]), np.isfinite(sig))
        np.testing.assert_allclose(g["sigma"][live], sig[live], rtol=tsig, atol=0)
        if g["fc"] is not None:
            f0 = c["spec"]["fc"][:, :c["Hf"]]
            np.testing.assert_array_equal(np.isfinite(g["fc"]), np.isfinite(f0))
            assert (np.abs(g["fc"] - f0)[live] <= tols["fc"] * scale[live, None]).all()
    else:
        np.testing.assert_array_equal(g["sigma"], c["sig_in"])
        np.testing.assert_array_equal(g["fc"], c["fc_in"])
    # a band is centre +- th sigma: the centre's and sigma's errors and two fp32 roundings
    with np.errstate(invalid="ignore"):
        th = np.abs(c["up"] - cen.astype(F32)) / np.where(sig > 0, sig, 1)[:, None]
    btol = tols["fc"] * scale[:, None] + th * sig[:, None] * tsig + 2.0 ** -22 * (np.abs(c["up"]) + np.abs(c["lo"]))
    for k in ("up", "lo"):
        np.testing.assert_array_equal(np.isfinite(g[k]), np.isfinite(c[k]), err_msg=k)
        ok = np.isfinite(c[k])
        assert (np.abs(g[k].astype(np.float64) - c[k])[ok] <= btol[ok]).all(), (what, k)
    # a service's score: the largest excess over a band in sigmas (1e30 where sigma is 0)
    sr = c["packed"][:, 1]
    big = sr >= 1e29
    np.testing.assert_array_equal(g["packed"][big, 1], sr[big])
    with np.errstate(invalid="ignore", divide="ignore"):
        stol = np.where(sig > 0, np.nanmax(np.where(np.isfinite(btol), btol, 0), 1) / np.where(sig > 0, sig, 1), 0)
    stol = stol.reshape(S, M).max(1) + sr * (tsig + 1e-6)
    assert (np.abs(g["packed"][~big, 1] - sr[~big]) <= stol[~big]).all(), (what, g["packed"][:, 1], sr)
    # ---- stats and last3 at lastk; rows without one keep what the buffers held
    lk = c["lastk"]
    has = (lk >= 0) & (lk < n)
    rows = np.arange(R)
    assert np.isnan(g["stats"][has][:, :2]).all() and (g["stats"][~has] == 7.0).all()
    np.testing.assert_array_equal(g["stats"][has, 2], g["up"][rows[has], lk[has]])
    np.testing.assert_array_equal(g["stats"][has, 3], g["lo"][rows[has], lk[has]])
    assert (g["last3"][:, ~has] == 7.0).all()
    x = c["cur"][rows[has], lk[has]]
    np.testing.assert_array_equal(g["last3"][0, has], x)
    np.testing.assert_array_equal(g["last3"][1, has], np.where(np.isfinite(x), g["up"][rows[has], lk[has]], np.nan))
    np.testing.assert_array_equal(g["last3"][2, has], np.where(np.isfinite(x), g["lo"][rows[has], lk[has]], np.nan))
    # ---- compaction: the anomaly list as a set of (row, point, upper bits, lower bits) and values
    rr, pp = np.nonzero(c["flag"])
    total = len(rr)
    assert total == c["count"].sum()
    want = {(int(r), int(p), int(g["up"][r, p].view(np.int32)), int(g["lo"][r, p].view(np.int32))): c["cur"][r, p]
            for r, p in zip(rr, pp)}
    nw = min(total, g["cap"])
    got = {tuple(int(v) for v in g["idx"][i]): g["val"][i] for i in range(nw)}
    assert len(got) == nw and (g["idx"][g["cap"]:] == -7).all() and (g["val"][g["cap"]:] == 7.0).all()
    if total <= g["cap"]:
        assert got.keys() == want.keys() and (g["idx"][nw:] == -7).all()
    assert all(k in want and want[k] == v for k, v in got.items()), what


@pytest.mark.parametrize("name", list(STEP_CASES))
def test_step_case_reference(name):
    """The reference of the fused step is sound: every finite point keeps 0.05 sigma
    from its cut (asserted while it is built), anomalies exist on both sides, the
    history gate and the clamp are active, and ``cap`` overflows where it is set."""
    c = step_case(name)
    if c["n"] > 1:
        assert (c["cur"][c["flag"]] > c["up"][c["flag"]]).any() and (c["cur"][c["flag"]] < c["lo"][c["flag"]]).any()
        assert ((c["lo"] == 9.5).any() or c["S"] == 1) and (((c["valid"] & 1) == 0).any() or c["R"] < 5)
    if c["cap"]:
        assert c["count"].sum() > c["cap"]
    if c["kind"] >= 0:
        assert c["R"] < 5 or (np.isnan(c["xs"][ROW_EMPTY]).all() and np.isnan(c["xs"][3, -2:]).all())
        print(f"err_ref step {name}: {c['tols']}")


def _g_of_reference(c):
    """The outputs a launch must give, from the reference alone."""
    R, S, n, kind = c["R"], c["S"], c["n"], c["kind"]
    rows, lk = np.arange(R), c["lastk"]
    has = (lk >= 0) & (lk < n)
    up, lo = c["up"].copy(), c["lo"].copy()
    stats = np.full((R, 4), 7.0, F32)
    stats[has, :2] = np.nan
    stats[has, 2], stats[has, 3] = up[rows[has], lk[has]], lo[rows[has], lk[has]]
    last3 = np.full((3, R), 7.0, F32)
    x = c["cur"][rows[has], lk[has]]
    last3[0, has] = x
    last3[1, has] = np.where(np.isfinite(x), stats[has, 2], np.nan)
    last3[2, has] = np.where(np.isfinite(x), stats[has, 3], np.nan)
    rr, pp = np.nonzero(c["flag"])
    cap = c["cap"] or len(rr) + 5
    idx = np.full((cap + 8, 4), -7, np.int32)
    val = np.full(cap + 8, 7.0, F32)
    k = min(len(rr), cap)
    idx[:k] = np.stack([rr, pp, up[rr, pp].view(np.int32), lo[rr, pp].view(np.int32)], 1)[:k]
    val[:k] = c["cur"][rr, pp][:k]
    return {"packed": c["packed"].copy(), "stats": stats, "count": c["count"].copy(),
            "dead": (~c["live"]).astype(np.int32), "up": up, "lo": lo, "sigma": c["sig64"].astype(F32),
            "fc": (c["spec"]["fc"][:, :c["Hf"]].astype(F32) if c["Hf"] else None) if kind >= 0 else c["fc_in"],
            "idx": idx, "val": val, "last3": last3, "cap": cap}


@pytest.mark.parametrize("name", ["hw12", "hw17", "given"])
def test_step_bounds_reject_wrong_outputs(name):
    """The comparison of the fused step passes the reference's own outputs and fails
    on: a band moved by a tenth of sigma, the history gate left out of a count, a
    status taken without the unknown rule, an anomaly missing from the list, one
    listed twice, stats taken one point off, a dead flag missing."""
    c = step_case(name)
    _assert_step(c, _g_of_reference(c), "the reference itself")
    flagged = int(np.nonzero(c["count"])[0][0])

    def moved(g):
        g["up"] += (0.1 * c["sig64"][:, None]).astype(F32)

    def ungated(g):
        g["count"][np.nonzero((c["valid"] & 1) == 0)[0][:1]] += 1

    def status(g):
        g["packed"][:, 0] = np.where(g["packed"][:, 3] > 0, 1, 0)

    def missing(g):
        g["idx"][0] = g["idx"][1]

    def stats(g):
        g["stats"][:, 2] = np.roll(g["stats"][:, 2], 1)

    def dead(g):
        g["dead"][:] = 0

    def count(g):
        g["count"][flagged] -= 1

    for bad in (moved, ungated, status, missing, stats, dead, count):
        if (bad is ungated and c["R"] < 5) or (bad is dead and c["kind"] < 0):
            continue
        if bad is status and (c["packed"][:, 0] != 2).all():
            continue
        g = _g_of_reference(c)
        bad(g)
        with pytest.raises(AssertionError):
            _assert_step(c, g, bad.__name__)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(STEP_CASES))
def test_gpu_es_band_step_edges(cuda, name):
    """es_band_step_kernel against the composition on the CPU; par 0, then par 1
    from the same state: the same outputs, and the other counter comes back 0."""
    c = step_case(name)
    kind = c["kind"]
    ctr = torch.tensor([5, 5, 0, 0], dtype=torch.int32, device=cuda)
    total = int(c["count"].sum())
    for par in (0, 1):
        if par == 0:
            ctr[0] = 0                               # the launch before zeroed this cycle's counter
        g = _band_step(cuda, c, par, ctr)
        _assert_step(c, g, f"{name} par={par}")
        assert g["ctr"][par] == total and g["ctr"][par ^ 1] == 0
        if kind < 0:
            continue
        # the slab: as in test_gpu_es_update_edges
        sl, sp, live = c["slots"], c["spec"], c["live"]
        free = np.setdiff1d(np.arange(c["C"]), sl)
        new = {k: v.cpu().numpy() for k, v in g["slab"].items()}
        for k in new:
            np.testing.assert_array_equal(new[k][free], c["slab"][k][free], err_msg=f"untouched slots: {k}")
        np.testing.assert_array_equal(new["params"], c["slab"]["params"])
        got = {"fc": sp["fc"][live], "level": new["state"][sl, 0][live], "trend": new["state"][sl, 1][live],
               "sse": new["sse"][sl][live], "season": new["season"][sl][live]}
        err = _update_errors(got, {k: v[live] for k, v in sp.items()}, kind)
        for k in ("sse", "state") + (("season",) if kind >= 2 else ()):
            assert err[k] <= c["tols"][k], (name, k, err[k], c["tols"][k])
        np.testing.assert_array_equal(new["nobs"][sl], sp["nobs"])
        np.testing.assert_array_equal(new["state"][sl, 2].astype(np.int64), sp["phase"])
        assert np.isnan(new["state"][sl[~live], 0]).all()
        same = c["t_new"] >= c["kmax"]               # no new sample: the slot is bit-identical
        for k in new:
            np.testing.assert_array_equal(new[k][sl[same]], c["slab"][k][sl[same]], err_msg=k)
