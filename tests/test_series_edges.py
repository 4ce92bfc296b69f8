"""Edge shapes of the series kernels: K1 rolling bands (rolling.hip), K3 FFT
seasonal analysis and the phase profile (fft.hip).

Every family has a fixture builder that returns numpy inputs, used twice: a
CPU test holds the library reference against a scalar fp64 spec written here,
and a GPU test holds the kernel against an fp64 reference.  Pad columns past T
hold 1e30, so a load that escapes the tail mask ruins the result instead of
reading "missing".

Which GPU test enters which path:

K1   r = (-w) & 7 = 7, 6, 5, 4, 3, 2, 1, 0 at segback 1 (w = 1 .. 8), 7 at
     segback 2 (w = 9), 1, 0 at segback 2 (w = 15, 16), 7 at segback 3
     (w = 17), 7 .. 0 at segback 256 (w = 2041 .. 2048); three tiles, so the
     ring half is reused; the window sums straight from the ring (w <= 16)
     and from the prefixes (w > 16) .......................................... test_gpu_rolling_every_rotation
     T = 1, T < 8, T % 8 != 0, T = one tile +- 1, two tiles + 1, w > T, the
     scalar-store path (T % 4 != 0) and the 16-B store path .................. test_gpu_rolling_tile_edges
     the window count against min_count at the median count, 0, w, w + 1 ..... test_gpu_rolling_count_is_exact
K3   run-time radix pairs 3.2, 5.2, 7.2, 9.2 (N = 6, 10, 14, 18), N < 256
     (also 70, 250), radix 5 first / middle / last (250), radix 4 and 2
     (256, 2048), 7, 9, 3 (630, 2058), the MAXN = 2048 bucket (N <= 2048),
     the 5120 bucket (2058, 3125, 5120), the 8192 bucket (5145, 5625, 8100,
     8192), the fixed plans (720, 1008, 5040), the ``spec`` output and the
     periodogram, k == N in the unpack (full output) ......................... test_gpu_fft_spectrum_every_plan
     the band-only unpack with kmax = N (k == N), the production band, a
     single-bin band ......................................................... test_gpu_fft_band_edges
     an 8-byte-aligned column view with the parent's row stride ............. test_gpu_fft_unaligned_view
     constant and linear rows (the rounding floor of ``strength``) .......... test_gpu_fft_flat_rows_have_no_season,
                                                                               test_gpu_detect_period_ignores_flat_rows
prof per-row periods 1, 7, 288, maxp, maxp + 1, 0, -3, NaN / inf, an empty
     row, a slope ............................................................ test_gpu_phase_profile_edges
     maxp = 8192 and 16384 (64 and 128 KB of dynamic LDS) .................... test_gpu_phase_profile_large_maxp

Tolerances.  u = 2^-24 is the fp32 unit roundoff.

K1: the kernel rounds d = x - c once to fp32 (c = the mean of the finite
samples among the first min(T, 2048)) and sums d and d^2 in fp64.  A window's
mean and population std are 1-Lipschitz in the sup norm of its samples, so the
rounding of d moves either by at most u max|x - c|.  The mean is returned as
c + fl32(m): u (|m| + |mean|) more, |m| <= max|x - c|; the std as
sqrtf(fl32(var)): 1.5 u std.  With a factor 2 of slack for the fp32
reciprocal seed and sqrtf:
    |mean - ref| <= 2 u (max_row|x - c| + |c| + |ref|)
    |sd   - ref| <= 2 u (max_row|x - c| + 4 ref_sd)
test_rolling_bound_rejects_off_by_one shows that a window one sample too long
or too short misses this bound in every case.

K3: e = max_k |X - X_ref| / sqrt(mean_k |X_ref|^2) per row, X_ref the fp64
transform of the fp64-detrended row.  FFT_B = 16 e32, where e32 is the same
figure for torch.fft.rfft in float32 on the CPU over the same rows
(test_fft_bound_covers_fp32_transform measures it): the kernel's twiddles
come from v_sin_f32 / v_cos_f32 and up to eight chained complex products per
butterfly over up to seven passes, a library transform reads exact tables.
|X|^2 then differs by at most |X - X_ref| (2 |X_ref| + |X - X_ref|).

Phase profile: a phase's mean is a sum of ``count`` fp32 atomicAdds in any
order over ``count``: at most count u max|v| off, times 2 for the fp32
evaluation of v = x - mean - slope (t - tb).

What these tests found on an MI355X, and what was changed for it:

K1   With fp32 squares and fp32 per-thread partial sums, a 1-ulp reciprocal
     and var = q / n - m^2 the kernel missed the std bound in every case: a
     one-sample window on unit noise had a std of 6.4e-4 instead of 0 (bound
     4.4e-7); the row that starts with 2048 missing samples, so that c = 0
     and d = 1e3, was off by 5.4e-2 at w = 2043 (bound 1.2e-4); the constant
     0.37 had a std of 7e-12 instead of 0.  NaN masks and counts were right,
     and so were all rotations.  The kernel now sums d and d^2 in fp64
     throughout, refines the reciprocal, forms (n q - s^2) / n^2 and sums
     windows of w <= 16 straight from the ring; it keeps the bound.
K3   The transform itself was within 3.3e-5 of the rms spectrum (the peak bin
     of the sinusoid rows; 2.3e-6 on the noise row) at every plan.  The row
     at offset 1e4 missed FFT_B at every length, with e = 4.5e-4 .. 2.4e-2 at
     bins 0 and 1: one-pass fp32 sums of x and t x left a line in the
     detrended row.
     The constant rows 0.37, 123.456 and 1e6 + 0.5 came out with strength
     0.140 .. 0.152 at bin 2 (0 and 5 with 0), and _detect_period returned
     5040 = nr / 2 for the fleet of flat rows.  The kernel now sums
     about a pivot and gives such rows strength 0 (FLAT_RMS).
     N = 8192 (65,744 B of LDS) and the phase profile at maxp = 16384 (128 KB)
     launch without a raised dynamic-LDS limit.  ref_phase_profile subtracted
     the mean in fp32 when given fp32 arrays; it is fp64 now."""
import functools
import math

import numpy as np
import pytest
import torch
from numpy.lib.stride_tricks import sliding_window_view

from foremast_amd.models import zoo
from foremast_amd.ops import fft as FF
from foremast_amd.ops import misc as MI

F32 = np.float32
U = 2.0 ** -24
PAD = 1e30


def _ceil4(T):
    return (T + 3) // 4 * 4


def _padded(x, extra=4):
    """Rows as the kernels take them: ld = ceil4(T) + extra, 1e30 at and past T."""
    R, T = x.shape
    out = np.full((R, _ceil4(T) + extra), PAD, F32)
    out[:, :T] = x
    return out


def _np(t):
    return t.cpu().numpy() if isinstance(t, torch.Tensor) else np.asarray(t)


# =========================================================================== K1
ROLL_T = 4200                                          # three tiles of 2048
ROLL_W = list(range(1, 10)) + [15, 16, 17] + list(range(2041, 2049))
EDGE_T = [1, 7, 8, 9, 2047, 2048, 2049, 4096, 4097]
EDGE_W = [5, 2043]
COUNT_W = [9, 17, 60, 2041, 2047]
NOISY, HALF_NAN, ALL_NAN, LATE, CONST, SHIFT, INFS, FIRST_ONLY = range(8)


@functools.lru_cache(maxsize=None)
def rolling_rows(T):
    """[8, T] fp32: noise; 50 % NaN; all NaN; 2048 NaN then data at 1e3 (so c = 0);
    a constant; a level shift from 0 to 1e4 after the first tile; +-inf samples;
    only sample 0 finite."""
    rng = np.random.default_rng(5000 + T)
    x = np.empty((8, T), F32)
    x[NOISY] = rng.normal(0, 1, T)
    x[HALF_NAN] = rng.normal(2, 1, T)
    x[HALF_NAN, rng.random(T) < 0.5] = np.nan
    x[ALL_NAN] = np.nan
    x[LATE] = 1e3 + rng.normal(0, 1, T)
    x[LATE, :2048] = np.nan
    x[CONST] = 0.37
    x[SHIFT] = rng.normal(0, 1, T)
    x[SHIFT, 2048:] += 1e4
    x[INFS] = rng.normal(-3, 2, T)
    x[INFS, rng.random(T) < 0.05] = np.inf
    x[INFS, rng.random(T) < 0.05] = -np.inf
    x[FIRST_ONLY] = np.nan
    x[FIRST_ONLY, 0] = 1234.567
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def count_rows(T):
    """[6, T] fp32, every sample missing with probability 1 / 2."""
    rng = np.random.default_rng(6000 + T)
    x = rng.normal(1, 2, (6, T)).astype(F32)
    x[rng.random((6, T)) < 0.5] = np.nan
    x.setflags(write=False)
    return x


def spec_rolling(x, w, min_count, first=None, length=None):
    """The fp64 spec: for every t the finite samples of the window [t - w + 1, t]
    (``first`` / ``length`` move it for the mutants), their count n, their mean
    and, in a second pass about that mean, their population std; NaN where
    n < max(min_count, 1).  Returns (mean, std, n), fp64."""
    R, T = x.shape
    L = w if length is None else length
    first = -(w - 1) if first is None else first       # window = [t + first, t + first + L - 1]
    mean = np.full((R, T), np.nan)
    sd = np.full((R, T), np.nan)
    cnt = np.zeros((R, T), np.int64)
    if L <= 0:
        return mean, sd, cnt
    lead, trail = max(0, -first), max(0, first + L - 1)
    for r in range(R):
        row = np.concatenate([np.full(lead, np.nan), x[r].astype(np.float64), np.full(trail, np.nan)])
        win = sliding_window_view(row, L)[lead + first: lead + first + T]
        f = np.isfinite(win)
        n = f.sum(1)
        if not n.any():
            continue
        nn = np.maximum(n, 1)
        with np.errstate(invalid="ignore"):
            m = np.where(f, win, 0.0).sum(1) / nn
            dev = np.where(f, win - m[:, None], 0.0)
        var = (dev * dev).sum(1) / nn
        ok = (n >= min_count) & (n > 0)
        mean[r], sd[r], cnt[r] = np.where(ok, m, np.nan), np.where(ok, np.sqrt(var), np.nan), n
    return mean, sd, cnt


@functools.lru_cache(maxsize=None)
def _roll_oracle(kind, T, w, min_count):
    x = rolling_rows(T) if kind == "rows" else count_rows(T)
    return spec_rolling(x, w, min_count)


def _row_centre(x):
    """c and max |x - c| per row, as the tolerance takes them: c = the fp64 mean of
    the finite samples among the first min(T, 2048), 0 when there are none."""
    x = x.astype(np.float64)
    f = np.isfinite(x)
    head = f[:, :2048]
    c = np.where(head.any(1), np.where(head, x[:, :2048], 0).sum(1) / np.maximum(head.sum(1), 1), 0.0)
    with np.errstate(invalid="ignore"):
        D = np.where(f, np.abs(x - c[:, None]), 0).max(1)
    return c, D


def assert_rolling_close(m, s, ref, x, rows=None, what=""):
    """The derived K1 bound (module docstring) and an exact NaN mask."""
    mr, sr = ref[0], ref[1]
    rows = range(x.shape[0]) if rows is None else rows
    c, D = _row_centre(x)
    for r in rows:
        nan = np.isnan(mr[r])
        assert np.array_equal(np.isnan(m[r]), nan) and np.array_equal(np.isnan(s[r]), nan), f"{what} row {r}: NaN mask"
        ok = ~nan
        if not ok.any():
            continue
        em = np.abs(m[r].astype(np.float64) - mr[r])[ok]
        es = np.abs(s[r].astype(np.float64) - sr[r])[ok]
        bm = 2 * U * (D[r] + abs(c[r]) + np.abs(mr[r][ok]))
        bs = 2 * U * (D[r] + 4 * sr[r][ok])
        i, j = int(np.argmax(em - bm)), int(np.argmax(es - bs))
        assert (em <= bm).all(), f"{what} row {r}: mean off by {em[i]:.3e}, bound {bm[i]:.3e}"
        assert (es <= bs).all(), f"{what} row {r}: std off by {es[j]:.3e} (ref {sr[r][ok][j]:.3e}), bound {bs[j]:.3e}"


ROLL_CASES = [(ROLL_T, w) for w in ROLL_W]
EDGE_CASES = [(T, w) for T in EDGE_T for w in EDGE_W]


@pytest.mark.parametrize("T,w", ROLL_CASES + EDGE_CASES)
def test_ref_rolling_matches_windowed_spec(T, w):
    """MI.ref_rolling_stats against the two-pass window loop: the NaN mask, the
    mean to the bound the kernel is held to, the std to that bound wherever the
    reference can keep it.  It cannot everywhere: it takes prefix sums over the
    whole row of d^2 with d about the ROW mean, so a window is the difference of
    two sums of up to T d^2 and its variance carries their rounding, which a
    std near 0 shows as its square root: 3e-6 at w = 1 on unit noise, 4e-3 on
    the level rows (1e3 after 2048 NaN, 0 -> 1e4), against 5e-7 and 1e-3 for
    the kernel.  Such windows are held in the variance, to the worst-case
    rounding of a T-term fp64 prefix sum, 2 T^2 2^-53 max d^2 / n.  The GPU
    tests therefore use the window loop, not this reference."""
    x = rolling_rows(T)
    ref = _roll_oracle("rows", T, w, 1)
    m, s = MI.ref_rolling_stats(x, w, 1)
    x64 = x.astype(np.float64)
    c, D = _row_centre(x)
    loose = 0
    for r in range(8):
        f = np.isfinite(x64[r])
        np.testing.assert_array_equal(np.isnan(m[r]), np.isnan(ref[0][r]))
        np.testing.assert_array_equal(np.isnan(s[r]), np.isnan(ref[0][r]))
        ok = ~np.isnan(ref[0][r])
        if not ok.any():
            continue
        mr, sr = ref[0][r][ok], ref[1][r][ok]
        assert (np.abs(m[r].astype(np.float64)[ok] - mr) <= 2 * U * (D[r] + abs(c[r]) + np.abs(mr))).all(), r
        d2 = np.abs(x64[r][f] - x64[r][f].mean()).max() ** 2
        s64 = s[r].astype(np.float64)[ok]
        tight = np.abs(s64 - sr) <= 2 * U * (D[r] + 4 * sr)
        held = np.abs(s64 ** 2 - sr ** 2) <= 2 * T * T * 2.0 ** -53 * d2 / ref[2][r][ok] + 4 * U * sr ** 2
        assert (tight | held).all(), (r, np.abs(s64 - sr).max())
        loose += int((~tight).sum())
        if r in (CONST, FIRST_ONLY):
            assert tight.all() and (s64 == 0).all()
    print(f"ref_rolling_stats T={T} w={w}: {loose} std outputs past the kernel's bound")


@pytest.mark.parametrize("T,w", [c for c in ROLL_CASES + EDGE_CASES if c[1] <= c[0]])
def test_rolling_bound_rejects_off_by_one(T, w):
    """The window [t - w, t] and the window [t - w + 2, t] both miss the bound on
    the noisy row, so it would catch a leaving sample taken one place off."""
    x = rolling_rows(T)
    ref = _roll_oracle("rows", T, w, 1)
    assert_rolling_close(ref[0].astype(F32), ref[1].astype(F32), ref, x, what="the spec itself")
    for first, length in ((-w, w + 1), (-(w - 2), w - 1)):
        mm, ms, _ = spec_rolling(x[NOISY:NOISY + 1], w, 1, first=first, length=length)
        with pytest.raises(AssertionError):
            assert_rolling_close(mm.astype(F32), ms.astype(F32), tuple(v[NOISY:NOISY + 1] for v in ref), x[NOISY:NOISY + 1])


def _count_case(w, kind):
    """(T, w, min_count) and the reference; ``kind`` picks min_count."""
    T = ROLL_T
    full = _roll_oracle("count", T, w, 1)[2][:, w - 1:]
    mc = {"median": int(np.median(full)), "zero": 0, "w": w, "w+1": w + 1}[kind]
    return T, mc, _roll_oracle("count", T, w, mc)


COUNT_CASES = [(w, "median") for w in COUNT_W] + [(17, k) for k in ("zero", "w", "w+1")] + [(2047, "w")]


@pytest.mark.parametrize("w,kind", COUNT_CASES)
def test_ref_rolling_count_is_sharp(w, kind):
    """At the median count between 15 % and 85 % of the full windows are NaN, so a
    count off by one anywhere in the kernel flips outputs; min_count = 0 behaves
    as 1, min_count = w needs a window without a hole, w + 1 gives NaN everywhere."""
    T, mc, ref = _count_case(w, kind)
    x = count_rows(T)
    nan = np.isnan(ref[0][:, w - 1:])
    if kind == "median":
        assert 0.15 <= nan.mean() <= 0.85, nan.mean()
    elif kind == "zero":
        np.testing.assert_array_equal(np.isnan(ref[0]), ref[2] == 0)
    elif kind == "w":
        np.testing.assert_array_equal(~np.isnan(ref[0]), ref[2] == w)
    else:
        assert np.isnan(ref[0]).all()
    m, s = MI.ref_rolling_stats(x, w, mc)
    assert_rolling_close(m, s, ref, x, what=f"w={w} mc={mc}")


def _gpu_rolling(cuda, x, w, mc):
    T = x.shape[1]
    xg = torch.from_numpy(_padded(x)).to(cuda)
    m, s = MI.rolling_stats(xg, T, w, mc)
    torch.cuda.synchronize()
    assert m.shape == (x.shape[0], T) and s.shape == m.shape
    return m.cpu().numpy(), s.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("T,w", ROLL_CASES)
def test_gpu_rolling_every_rotation(cuda, T, w):
    """All eight rotations of the leaving samples at segback 1, 2, 3 and 256 over
    three tiles, on the eight rows of ``rolling_rows``."""
    x = rolling_rows(T)
    m, s = _gpu_rolling(cuda, x, w, 1)
    assert_rolling_close(m, s, _roll_oracle("rows", T, w, 1), x, what=f"w={w}")


@pytest.mark.gpu
@pytest.mark.parametrize("T,w", EDGE_CASES)
def test_gpu_rolling_tile_edges(cuda, T, w):
    """Row lengths around 8 samples, one tile and two tiles, w > T, and both store
    paths (ld_o = T)."""
    x = rolling_rows(T)
    m, s = _gpu_rolling(cuda, x, w, 1)
    assert_rolling_close(m, s, _roll_oracle("rows", T, w, 1), x, what=f"T={T} w={w}")


@pytest.mark.gpu
@pytest.mark.parametrize("w,kind", COUNT_CASES)
def test_gpu_rolling_count_is_exact(cuda, w, kind):
    T, mc, ref = _count_case(w, kind)
    x = count_rows(T)
    m, s = _gpu_rolling(cuda, x, w, mc)
    np.testing.assert_array_equal(np.isnan(m), np.isnan(ref[0]))
    np.testing.assert_array_equal(np.isnan(s), np.isnan(ref[0]))
    assert_rolling_close(m, s, ref, x, what=f"w={w} mc={mc}")


# =========================================================================== K3
FFT_N = [6, 10, 14, 18, 70, 250, 256, 630, 2048, 2058, 3125, 5120, 5145, 5625, 8100, 8192, 720, 1008, 5040]
FFT_SMALL_N = [6, 10, 14, 18, 70]                      # Nr <= 140: the O(N^2) DFT pins the reference
# 16 e32, rounded up; e32 = 1.109e-5 as test_fft_bound_covers_fp32_transform measures it.  Its maximum is at
# N = 8192 on the sinusoid rows, at the peak bin: 85 times the rms spectrum there, so 1.3e-7 of the peak itself.
FFT_B = 1.78e-4
NOISE, TONE, HOLES, OFFSET, EMPTY = range(5)
TONE_ROWS = (TONE, HOLES, OFFSET)


def tone_bin(nr):
    """The sinusoid's bin: inside the production band [2, nr / 12] where that band exists."""
    return max(2, nr // 24)


@functools.lru_cache(maxsize=None)
def fft_rows(nr):
    """[5, nr] fp32: white noise; noise plus a sinusoid at ``tone_bin``; that row with
    30 % NaN and a few +-inf; that row plus 1e4; all NaN."""
    rng = np.random.default_rng(7000 + nr)
    t = np.arange(nr)
    x = np.empty((5, nr), F32)
    x[NOISE] = rng.normal(0, 1, nr)
    tone = 2.0 * np.sin(2 * np.pi * tone_bin(nr) * t / nr + rng.uniform(0, 2 * np.pi)) + rng.normal(0, 0.5, nr)
    x[TONE] = tone
    x[HOLES] = tone
    x[HOLES, rng.random(nr) < 0.3] = np.nan
    k = max(1, nr // 500)
    x[HOLES, rng.choice(nr, k, replace=False)] = np.inf
    x[HOLES, rng.choice(nr, k, replace=False)] = -np.inf
    x[OFFSET] = (1e4 + tone).astype(F32)
    x[EMPTY] = np.nan
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def _fft_ref(nr):
    """fp64: the detrended rows, their transform, mean, slope."""
    xc, mu, sl, flat = FF.ref_detrend(fft_rows(nr))
    assert not flat[:EMPTY].any() and flat[EMPTY]
    return xc, np.fft.rfft(xc, axis=1), mu, sl


def _rms(X):
    return np.sqrt((np.abs(X) ** 2).mean(1))


def _spectrum_error(X, Xr):
    """max_k |X - X_ref| / sqrt(mean_k |X_ref|^2) per row; rows with X_ref = 0 must be 0 exactly."""
    rms = _rms(Xr)
    err = np.abs(X.astype(np.complex128) - Xr).max(1)
    assert (err[rms == 0] == 0).all()
    return err / np.where(rms > 0, rms, 1)


def spec_fft_seasonal(x, kmin, kmax):
    """docs/BRAIN_SPEC.md 3 and ref_fft_seasonal's contract, one row and one bin at
    a time: the least-squares line through the finite samples is removed, missing
    samples become 0, X_k = sum_t e_t exp(-2 pi i k t / Nr); strength = the largest
    band power over sum_{k >= 1} |X_k|^2, 0 for a row that is a line to rounding."""
    R, nr = x.shape
    out = []
    for r in range(R):
        tv = [(t, float(v)) for t, v in enumerate(x[r]) if math.isfinite(v)]
        n = len(tv)
        mu = math.fsum(v for _, v in tv) / n if n else 0.0
        tbar = math.fsum(t for t, _ in tv) / n if n else 0.0
        vt = math.fsum((t - tbar) ** 2 for t, _ in tv) / n if n else 0.0
        sl = math.fsum((t - tbar) * (v - mu) for t, v in tv) / n / vt if vt > 0 else 0.0
        e = [0.0] * nr
        for t, v in tv:
            e[t] = v - mu - sl * (t - tbar)
        X = [complex(math.fsum(e[t] * math.cos(2 * math.pi * ((k * t) % nr) / nr) for t in range(nr)),
                     -math.fsum(e[t] * math.sin(2 * math.pi * ((k * t) % nr) / nr) for t in range(nr)))
             for k in range(nr // 2 + 1)]
        pw = [abs(z) ** 2 for z in X]
        kb = max(range(kmin, kmax + 1), key=lambda k: (pw[k], -k))
        tot = math.fsum(pw[1:])
        tmid = 0.5 * (nr - 1)
        line = abs(mu + sl * (tmid - tbar)) + abs(sl) * tmid
        flat = math.fsum(v * v for v in e) <= max(n, 1) * (2.0 ** -20 * line) ** 2
        out.append((mu, sl, np.array(X), kb, 0.0 if flat or tot <= 0 else pw[kb] / tot))
    return out


@pytest.mark.parametrize("N", FFT_SMALL_N)
def test_ref_fft_matches_direct_dft(N):
    nr = 2 * N
    x = fft_rows(nr)
    kmin, kmax = 1, N
    s = FF.fft_seasonal(torch.from_numpy(x.copy()), nr, min_period=2, max_period=nr, return_power=True, return_spectrum=True)
    assert s.spectrum.dtype == torch.complex64 and s.spectrum.shape == (5, N + 1)
    Xr = _fft_ref(nr)[1]
    for r, (mu, sl, X, kb, st) in enumerate(spec_fft_seasonal(x, kmin, kmax)):
        scale = max(1.0, float(np.abs(X).max()))
        np.testing.assert_allclose(Xr[r], X, rtol=0, atol=1e-12 * scale * max(1.0, abs(mu)))
        np.testing.assert_allclose(s.spectrum[r].numpy(), X, rtol=0, atol=2 * U * scale)
        np.testing.assert_allclose(s.power[r].numpy(), np.abs(X) ** 2, rtol=4 * U, atol=(1e-9 * scale * max(1.0, abs(mu))) ** 2)
        np.testing.assert_allclose(float(s.mean[r]), mu, rtol=U, atol=1e-30)
        np.testing.assert_allclose(float(s.slope[r]), sl, rtol=1e-6, atol=1e-12 * max(1.0, abs(mu)))
        np.testing.assert_allclose(float(s.strength[r]), st, rtol=1e-6)
        if r in TONE_ROWS:
            assert int(s.period_bin[r]) == kb
    assert float(s.strength[EMPTY]) == 0 and float(s.mean[EMPTY]) == 0


def _e32(nr):
    xc, Xr = _fft_ref(nr)[:2]
    X32 = torch.fft.rfft(torch.from_numpy(xc.astype(F32)), dim=1).numpy()
    return float(_spectrum_error(X32, Xr).max())


def test_fft_bound_covers_fp32_transform():
    """e32: the error figure of a float32 library transform over the rows of every
    length, measured here; FFT_B is 16 times its maximum."""
    e = {N: _e32(2 * N) for N in FFT_N}
    worst = max(e, key=e.get)
    assert 16 * e[worst] <= FFT_B, f"e32 = {e[worst]:.3e} at N = {worst}; 16 e32 = {16 * e[worst]:.3e}, FFT_B = {FFT_B:.3e}"
    assert FFT_B <= 16 * e[worst] * 1.05, f"FFT_B = {FFT_B:.3e} is more than 16 e32 = {16 * e[worst]:.3e}"


def _band_margin(nr, kmin, kmax, rows=TONE_ROWS):
    """On the reference the top band bin beats the runner-up by 1 % on the sinusoid rows."""
    Xr = _fft_ref(nr)[1]
    for r in rows:
        pw = np.sort(np.abs(Xr[r, kmin:kmax + 1]) ** 2)
        if pw.size > 1:
            assert pw[-1] >= 1.01 * pw[-2], (nr, r, pw[-1] / pw[-2])


def _strength_tol(nr, kb):
    """|strength - ref| allowed per row: strength = P_b / total with |P_b - ref|
    <= B rms (2 |X_b| + B rms) (module docstring) and the total, Parseval over
    fp32 samples summed in chains of at most 70 terms, to 80 u relative."""
    Xr = _fft_ref(nr)[1]
    rms = _rms(Xr)
    tot = (np.abs(Xr[:, 1:]) ** 2).sum(1)
    ab = np.abs(Xr[np.arange(5), kb])
    dp = FFT_B * rms * (2 * ab + FFT_B * rms)
    st = np.where(tot > 0, ab ** 2 / np.where(tot > 0, tot, 1), 0)
    return np.where(tot > 0, dp / np.where(tot > 0, tot, 1), 0) + 80 * U * st + 1e-30


def _moments_tol(nr):
    """|mean - ref|, |slope - ref| allowed: fp32 sums in chains of at most 70 terms
    (64 per thread, 6 wave steps) err by 70 u sum|term| at worst, the output
    rounding adds u."""
    x = fft_rows(nr).astype(np.float64)
    ok = np.isfinite(x)
    n = np.maximum(ok.sum(1), 1)
    _, _, mu, _ = _fft_ref(nr)
    absx = np.where(ok, np.abs(np.where(ok, x, 0)), 0).sum(1) / n
    tmid = 0.5 * (nr - 1)
    tc = np.arange(nr) - tmid
    tbar = np.where(ok, tc, 0).sum(1) / n
    vt = np.where(ok, (tc - tbar[:, None]) ** 2, 0).sum(1) / n
    tm = 80 * U * absx
    ts = 80 * U * absx * (tmid + np.abs(tbar)) / np.where(vt > 0, vt, 1)
    return tm + 1e-30, ts + 1e-30


@functools.lru_cache(maxsize=None)
def _cpu_fft(nr, min_period, max_period):
    return FF.fft_seasonal(torch.from_numpy(fft_rows(nr).copy()), nr, min_period=min_period, max_period=max_period)


@pytest.mark.parametrize("N", FFT_N)
def test_ref_fft_rows_are_sharp(N):
    """What the GPU tests assume of the rows: the tone wins its band by 1 % in the
    reference, over the full band and the production band, and the library
    reference returns that bin."""
    nr = 2 * N
    _band_margin(nr, 1, N)
    c = _cpu_fft(nr, 2, nr)
    # 12 to 36 samples with a third of them missing need not keep the tone on top; the margin is what counts
    want = [tone_bin(nr)] * 3
    assert N < 70 or [int(c.period_bin[r]) for r in TONE_ROWS] == want
    assert [int(c.period_bin[r]) for r in (TONE, OFFSET)] == want[:2]
    if nr >= 24:
        _band_margin(nr, 2, nr // 12)
        c = _cpu_fft(nr, 12, nr / 2)
        assert N < 70 or [int(c.period_bin[r]) for r in TONE_ROWS] == want


def _gpu_fft(cuda, x, nr, **kw):
    s = FF.fft_seasonal(torch.from_numpy(np.ascontiguousarray(x)).to(cuda), nr, **kw)
    torch.cuda.synchronize()
    return s


@pytest.mark.gpu
@pytest.mark.parametrize("N", FFT_N)
def test_gpu_fft_spectrum_every_plan(cuda, N):
    """The complex spectrum and the periodogram of every row at every plan, to
    FFT_B of the row's rms spectrum (not of its peak: the noise bins count)."""
    nr = 2 * N
    x = fft_rows(nr)
    xc, Xr, mu, sl = _fft_ref(nr)
    g = _gpu_fft(cuda, x, nr, min_period=2, max_period=nr, return_power=True, return_spectrum=True)
    X = _np(g.spectrum)
    assert X.dtype == np.complex64 and X.shape == (5, N + 1)
    e = _spectrum_error(X, Xr)
    k = np.abs(X - Xr).argmax(1)
    print(f"K3 N={N} e =", " ".join(f"{v:.2e}@{int(b)}" for v, b in zip(e, k)), f"B = {FFT_B:.2e}")
    tm, ts = _moments_tol(nr)
    print("   mean err", np.abs(_np(g.mean) - mu) / tm, "slope err", np.abs(_np(g.slope) - sl) / ts)
    assert (e <= FFT_B).all(), (N, e.tolist())
    rms = _rms(Xr)[:, None]
    dp = np.abs(_np(g.power).astype(np.float64) - np.abs(Xr) ** 2)
    assert (dp <= FFT_B * rms * (2 * np.abs(Xr) + FFT_B * rms) + 4 * U * np.abs(Xr) ** 2).all()
    assert (np.abs(_np(g.mean) - mu) <= tm).all() and (np.abs(_np(g.slope) - sl) <= ts).all()
    c = _cpu_fft(nr, 2, nr)
    _band_margin(nr, 1, N)
    pb = _np(g.period_bin)
    np.testing.assert_array_equal(pb[list(TONE_ROWS)], _np(c.period_bin)[list(TONE_ROWS)])
    assert (np.abs(_np(g.strength) - _np(c.strength)) <= _strength_tol(nr, _np(c.period_bin))).all()
    assert _np(g.strength)[EMPTY] == 0 and _np(g.mean)[EMPTY] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("N", FFT_N)
def test_gpu_fft_band_edges(cuda, N):
    """The band-only unpack against the full unpack (same bin, same strength, bit
    for bit) and against the reference: the production band [2, nr / 12], the band
    [1, N] whose last bin takes the k == N branch, and a single-bin band."""
    nr = 2 * N
    x = fft_rows(nr)
    kb = tone_bin(nr)
    bands = [(2, nr, 1, N), (nr / (kb + 0.5), nr / (kb - 0.5), kb, kb)]
    if nr >= 24:
        bands.append((12, nr / 2, 2, nr // 12))
    for lo, hi, kmin, kmax in bands:
        _band_margin(nr, kmin, kmax)
        c = _cpu_fft(nr, lo, hi)
        b = _gpu_fft(cuda, x, nr, min_period=lo, max_period=hi)
        f = _gpu_fft(cuda, x, nr, min_period=lo, max_period=hi, return_power=True)
        assert b.power is None and b.spectrum is None
        np.testing.assert_array_equal(_np(b.period_bin), _np(f.period_bin))
        np.testing.assert_array_equal(_np(b.strength), _np(f.strength))
        pb = _np(b.period_bin)
        assert ((pb >= kmin) & (pb <= kmax)).all()
        np.testing.assert_array_equal(pb[list(TONE_ROWS)], _np(c.period_bin)[list(TONE_ROWS)])
        assert N < 70 or (pb[list(TONE_ROWS)] == kb).all()
        # the noise row's peak may be a near tie: its strength is held at the reference's bin
        tol = _strength_tol(nr, _np(c.period_bin))
        rows = list(TONE_ROWS) + [EMPTY]
        assert (np.abs(_np(b.strength) - _np(c.strength))[rows] <= tol[rows]).all(), (lo, hi)
        np.testing.assert_allclose(_np(b.period), nr / np.maximum(pb, 1), rtol=1e-6)


@pytest.mark.gpu
@pytest.mark.parametrize("nr", [140, 4116, 10080])
def test_gpu_fft_unaligned_view(cuda, nr):
    """The column view hist[:, 2:2 + nr] of a wider buffer, as _detect_period passes
    it (an 8-byte-aligned pointer, the parent's row stride): bit for bit what a
    contiguous copy gives."""
    hist = np.full((5, nr + 6), PAD, F32)
    hist[:, 2:2 + nr] = fft_rows(nr)
    hg = torch.from_numpy(hist).to(cuda)
    view = hg[:, 2:2 + nr]
    assert view.data_ptr() % 16 == 8 and view.stride(0) == nr + 6
    a = FF.fft_seasonal(view, nr, min_period=12, max_period=nr / 2, return_power=True, return_spectrum=True)
    b = FF.fft_seasonal(view.contiguous(), nr, min_period=12, max_period=nr / 2, return_power=True,
                        return_spectrum=True)
    c = FF.fft_seasonal(view, nr, min_period=12, max_period=nr / 2)
    torch.cuda.synchronize()
    for name in ("period_bin", "strength", "mean", "slope", "power"):
        np.testing.assert_array_equal(_np(getattr(a, name)), _np(getattr(b, name)), err_msg=name)
    np.testing.assert_array_equal(_np(torch.view_as_real(a.spectrum)), _np(torch.view_as_real(b.spectrum)))
    np.testing.assert_array_equal(_np(c.period_bin), _np(b.period_bin))
    np.testing.assert_array_equal(_np(c.strength), _np(b.strength))
    ref = _cpu_fft(nr, 12, nr / 2)
    np.testing.assert_array_equal(_np(a.period_bin)[list(TONE_ROWS)], _np(ref.period_bin)[list(TONE_ROWS)])


FLAT_NR = [10080, 4116]                                # the fixed plan 5040 and the run-time plan 2058


def flat_rows(nr, part):
    """Rows without a season.  Part 0: the constants 0, 5, 0.37, 123.456, 1e6 + 0.5.
    Part 1: the line 100 + 0.013 t rounded to fp32, and 123.456 with 30 % NaN."""
    if part == 0:
        return np.tile(np.array([[0.0], [5.0], [0.37], [123.456], [1e6 + 0.5]], F32), (1, nr))
    rng = np.random.default_rng(8000 + nr)
    x = np.empty((2, nr), F32)
    x[0] = (100 + 0.013 * np.arange(nr)).astype(F32)
    x[1] = 123.456
    x[1, rng.random(nr) < 0.3] = np.nan
    return x


def season_rows(nr):
    """The other side of the floor: a season of 1e-3 relative on a level and on a line."""
    t = np.arange(nr)
    tone = np.sin(2 * np.pi * tone_bin(nr) * t / nr)
    return np.stack([123.456 * (1 + 1e-3 * tone), (100 + 0.013 * t) * (1 + 1e-3 * tone)]).astype(F32)


@pytest.mark.parametrize("nr", FLAT_NR)
def test_ref_fft_flat_rows_have_no_season(nr):
    for part in (0, 1):
        s = FF.fft_seasonal(torch.from_numpy(flat_rows(nr, part)), nr, min_period=12, max_period=nr / 2)
        assert (s.strength.numpy() == 0).all(), s.strength
    s = FF.fft_seasonal(torch.from_numpy(season_rows(nr)), nr, min_period=12, max_period=nr / 2)
    assert (s.strength.numpy() > 0.9).all() and (s.period_bin.numpy() == tone_bin(nr)).all()


@pytest.mark.gpu
@pytest.mark.parametrize("nr", FLAT_NR)
def test_gpu_fft_flat_rows_have_no_season(cuda, nr):
    """Constant and linear rows leave a rounding-sized ramp after the fp32 detrend;
    its 1 / k^2 spectrum must not read as a season (strength 0, as the reference).
    A season of 1e-3 relative on the same level keeps its strength."""
    for part in (0, 1):
        x = flat_rows(nr, part)
        g = _gpu_fft(cuda, x, nr, min_period=12, max_period=nr / 2)
        print("K3 flat rows", nr, part, _np(g.strength).tolist(), _np(g.period_bin).tolist())
        assert (_np(g.strength) == 0).all(), _np(g.strength)
    x = season_rows(nr)
    g = _gpu_fft(cuda, x, nr, min_period=12, max_period=nr / 2)
    c = FF.fft_seasonal(torch.from_numpy(x), nr, min_period=12, max_period=nr / 2)
    np.testing.assert_array_equal(_np(g.period_bin), _np(c.period_bin))
    # the tone is 1e-3 of a level of 123 and 230: its samples carry fp32 rounding of up to 2^-24 / 1e-3 = 6e-5 of it
    np.testing.assert_allclose(_np(g.strength), _np(c.strength), rtol=2e-3)


def _flat_fleet(T=10080):
    return np.concatenate([flat_rows(T, 0)[1:], flat_rows(T, 1)])          # 6 rows


def test_detect_period_ignores_flat_rows():
    assert zoo._detect_period(torch.from_numpy(_flat_fleet()), 10080) == 1440
    both = np.concatenate([_flat_fleet()[:4], season_rows(10080)])
    assert zoo._detect_period(torch.from_numpy(both), 10080) == 10080 // tone_bin(10080)


@pytest.mark.gpu
def test_gpu_detect_period_ignores_flat_rows(cuda):
    assert zoo._detect_period(torch.from_numpy(_flat_fleet()).to(cuda), 10080) == 1440
    both = np.concatenate([_flat_fleet()[:4], season_rows(10080)])
    assert zoo._detect_period(torch.from_numpy(both).to(cuda), 10080) == 10080 // tone_bin(10080)


def test_fft_rejects_empty_band():
    x = torch.zeros((2, 12))
    with pytest.raises(ValueError):
        FF.fft_seasonal(x, 12, min_period=12, max_period=6)            # kmin = 2 > kmax = 1
    with pytest.raises(ValueError):
        FF.fft_seasonal(torch.zeros((2, 140)), 140, min_period=20.5, max_period=21.5)   # no bin between
    assert FF.fft_seasonal(x, 12, min_period=2).period_bin.shape == (2,)


# ================================================================ phase profile
PROF_T, PROF_MAXP = 1000, 300
PROF_P = [1, 7, 288, PROF_MAXP, PROF_MAXP + 1, 0, -3]


def profile_case(T=PROF_T, periods=PROF_P, slopes=(0.004, -0.002, 0.001)):
    """Rows: noise on a slope; NaN and +-inf among noise; all NaN; noise on a slope
    at p = maxp; three rows whose period is out of range.  |slope| T / 2 stays
    below max |v|, as the tolerance assumes of the terms of v."""
    R = len(periods)
    rng = np.random.default_rng(9000 + T)
    t = np.arange(T)
    sl = np.zeros(R, F32)
    sl[0::3] = slopes[:len(sl[0::3])]
    x = (rng.normal(1.5, 1, (R, T)) + sl[:, None] * t).astype(F32)
    if R > 2:
        x[1, rng.random(T) < 0.2] = np.nan
        x[1, rng.random(T) < 0.02] = np.inf
        x[1, rng.random(T) < 0.02] = -np.inf
        x[2] = np.nan
    ok = np.isfinite(x)
    mean = (np.where(ok, x, 0).sum(1, dtype=np.float64) / np.maximum(ok.sum(1), 1)).astype(F32)
    return x, np.asarray(periods, np.int32), mean, sl


def spec_phase_profile(x, period, mean, slope, maxp):
    """out[r, i] = the mean over the finite samples at t % p == i of
    x - mean - slope (t - (T - 1) / 2); 0 for an empty phase, for i >= p and for
    a period outside [1, maxp].  Also the count and max |v| per row."""
    R, T = x.shape
    out = np.zeros((R, maxp))
    cnt = np.zeros((R, maxp), np.int64)
    vmax = np.zeros(R)
    for r in range(R):
        p = int(period[r])
        if p <= 0 or p > maxp:
            continue
        acc = [[] for _ in range(p)]
        for t in range(T):
            v = float(x[r, t])
            if math.isfinite(v):
                acc[t % p].append(v - float(mean[r]) - float(slope[r]) * (t - 0.5 * (T - 1)))
        for i, a in enumerate(acc):
            if a:
                out[r, i], cnt[r, i] = math.fsum(a) / len(a), len(a)
                vmax[r] = max(vmax[r], max(abs(v) for v in a))
    return out, cnt, vmax


def test_ref_phase_profile_matches_scalar_spec():
    x, p, mean, sl = profile_case()
    ref = FF.phase_profile(torch.from_numpy(x), PROF_T, torch.from_numpy(p), torch.from_numpy(mean), PROF_MAXP,
                           torch.from_numpy(sl)).numpy()
    out, cnt, vmax = spec_phase_profile(x, p, mean, sl, PROF_MAXP)
    assert ref.shape == (len(PROF_P), PROF_MAXP) and ref.dtype == np.float32
    np.testing.assert_allclose(ref, out, rtol=2 * U, atol=1e-12)
    assert not ref[[2, 4, 5, 6]].any() and not ref[1, 7:].any() and ref[3].all()
    assert cnt[1, :7].min() < cnt[0, 0] and PROF_T % 7 and PROF_T % 288 and PROF_T % PROF_MAXP


def _gpu_profile(cuda, x, T, p, mean, sl, maxp):
    xg = torch.from_numpy(_padded(x)).to(cuda)
    out = FF.phase_profile(xg, T, torch.from_numpy(p).to(cuda), torch.from_numpy(mean).to(cuda), maxp,
                           torch.from_numpy(sl).to(cuda))
    torch.cuda.synchronize()
    return out.cpu().numpy()


def _assert_profile_close(g, x, p, mean, sl, maxp):
    ref = FF.ref_phase_profile(x, p, mean, maxp, sl)
    R, T = x.shape
    for r in range(R):
        pr = int(p[r])
        if pr <= 0 or pr > maxp:
            assert not g[r].any()
            continue
        tt = np.arange(T)
        v = x[r].astype(np.float64) - float(mean[r]) - float(sl[r]) * (tt - 0.5 * (T - 1))
        ok = np.isfinite(v)
        cnt = np.bincount((tt % pr)[ok], minlength=pr)
        vmax = np.abs(v[ok]).max() if ok.any() else 0.0
        assert not g[r, pr:].any()
        tol = 2 * cnt * U * vmax + U * np.abs(ref[r, :pr])
        err = np.abs(g[r, :pr].astype(np.float64) - ref[r, :pr])
        assert (err <= tol).all(), (r, pr, float((err - tol).max()))
        assert (g[r, :pr][cnt == 0] == 0).all()


@pytest.mark.gpu
def test_gpu_phase_profile_edges(cuda):
    x, p, mean, sl = profile_case()
    g = _gpu_profile(cuda, x, PROF_T, p, mean, sl, PROF_MAXP)
    assert g.shape == (len(PROF_P), PROF_MAXP)
    _assert_profile_close(g, x, p, mean, sl, PROF_MAXP)


@pytest.mark.gpu
@pytest.mark.parametrize("maxp", [8192, 16384])
def test_gpu_phase_profile_large_maxp(cuda, maxp):
    """One row at the largest profiles: 2 maxp floats of dynamic LDS, 64 and 128 KB."""
    T = 2 * maxp + 5
    x, p, mean, sl = profile_case(T, [maxp], slopes=(1e-4,))
    g = _gpu_profile(cuda, x, T, p, mean, sl, maxp)
    _assert_profile_close(g, x, p, mean, sl, maxp)
    assert g[0].all()
