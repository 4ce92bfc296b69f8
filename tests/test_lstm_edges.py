"""Edge shapes of the K6 LSTM kernels (csrc/kernels/lstm.hip, lstm_stack.hip,
csrc/include/fm_lstm_cell.h): the register-resident forward in its five launch
forms, the history kernel, the stacked kernels, the head and the two feature
kernels.

The reference is ``spec_lstm``: a plain loop over the steps in fp64 (numpy),
written from the kernels' header comments.  Gate order i, f, g, o, b = b_ih +
b_hh, c' = sigm(f) c + sigm(i) tanh(g), h = sigm(o) tanh(c') with libm's exp and
tanh.  It rounds to bf16 exactly where the kernels do: the weights after the gate
scale (``LS.gate_scales``; the exact scale is divided out again), the inputs, and
every h that feeds a GEMM (the recurrent h, h0, layer 0's h into layer 1).  c is
never rounded.  ``spec_features`` / ``spec_features_mv`` are the feature spec in
fp64: finite mean of the window, population standard deviation floored at 1e-6,
z = (v - mu) / sd with missing -> 0, the phase 2 pi c / period of the dense
column c, 1.0 at k = I (k = M + 2), zeros above.  Every history has a row stride
> T and 1e30 in the padding and in front of the window.

Tolerances, all computed in the tests from the fp32 and the fp64 run of the same
reference (u = 2^-24):

  rule 1   teacher-forced, where the kernel returns ``hseq``: at step t the
           reference takes the kernel's own hseq[:, t - 1] (exact bf16) as the
           recurrent input and keeps its own fp64 c.  err_ref = the largest
           difference between that loop in fp32 and in fp64;
           eps_h = max(8 err_ref_h, 32 u = 2e-6),
           eps_c = max(8 err_ref_c, 32 u max(1, max |c|)).
           The floor: ``lstm_cell`` is 19 issues on values of at most 1 (c: of at
           most max |c|), each within one ulp (v_exp_f32 and v_rcp_f32 are 1-ulp
           instructions, libm's are below 1): 19 u < 32 u.  The final h (fp32) is
           held to eps_h, the final c to eps_c, and hseq[:, t] must be the bf16
           rounding of a value within eps_h of the reference:
           bf16(h_ref - eps_h) <= hseq <= bf16(h_ref + eps_h), which is half a
           bf16 ulp for the kernel's own store plus the smooth term.  (Half a bf16
           ulp is 2^-9 |h| only at the top of a binade and 2^-8 |h| at its bottom,
           so a flat 2^-9 |h| would refuse a correctly rounded store; the bracket
           is never wider than half an ulp + eps_h.)  The bound does not grow
           with L.
  rule 2   free-running, for the stacked kernels and the history kernel (no
           sequence comes back): err_ref = the largest difference between the
           fp32 and the fp64 run, bf16 roundings that fall on opposite sides of
           a boundary included: the fp32 run meets only a few such roundings, so
           two more fp64 runs add + / - 32 u (the floor of rule 1, the cell's own
           error) to every h before it is rounded for a GEMM, which flips every
           h that close to a boundary, and err_ref is the largest difference of
           the three from the plain fp64 run; tol = 8 err_ref, with rule 1's floor under it for
           h and c: where no bf16 rounding lies between the inputs and the
           output (one layer at L = 1) or every row is the same (I = 0), err_ref
           is fp32 rounding relative to a small |h|, while ``lstm_cell`` forms
           h = r - E_c r from terms near 1 and has an absolute error.  The stacked
           cases take err_ref over all 130 rows of their inputs, the case's rows
           being a prefix.  mu, sd and the head follow 8 err_ref without a floor
           (mu / sd of the feature kernels: err_ref over a pool of 64 rows of the
           case's generator, so that a one-row case does not rest on one
           rounding).
  features a bf16 feature equals the bf16 rounding of the fp64 spec, except where
           an fp32 evaluation can fall on the other side: with band = 8 x the
           largest |fp32 - fp64| of the feature kind (z, sin, cos) over the
           pool, an element whose bf16(v - band) != bf16(v + band) may take
           either; the two are one bf16 ulp apart and such elements are at most
           1 % of a case, both asserted on the CPU references alone.  A missing
           sample's 0, the 1.0 slot, the zero columns and memory behind the
           tensors are compared exactly.  (A constant window is 3.0: its fp32 sum
           is exact, so mu is, and every evaluation floors sd.  A constant such as
           10.3 sums with a rounding, and then fp32 gives sd ~ 1e-6 and z ~ +-1
           where the spec says 0 -- the mirror as much as the kernel.)

Which GPU test enters which path, with the err_ref measured on the CPU (rule 1:
with the fp64 loop's own rounded sequence as the teacher):

lstm_fwd_pipe_kernel<H, HSEQ> (XaSource, lstm_pipe_body) ..... test_gpu_lstm_forward_edges[H-I-L-B]
  L = 1      no ``L > 1`` prefetch, the first step is ``last``;  L = 2: no
             ``t + 2 < L`` prefetch;  L = 3, 5, 37: every branch
  B = 1, 31, 32   the second column tile is all clamped rows (bb = B - 1)
  B = 33, 64, 65, 130   one row in tile 1; a full workgroup; one row in a second
  I = 0      the augmented k-step is the bias alone;  I = 15: it is full
  every case h0 / c0 given and null; HSEQ = false bit-equal; rows at and past B
             untouched in h_out, c_out, hseq; B = n bit-equal to the first n rows
             of B = 130 ........................... err_ref h 6.1e-09 .. 2.2e-07, c 8.5e-09 .. 2.9e-07
lstm_fwd_kernel<H, NCT, CELL> .......................... test_gpu_lstm_forward_variants[H-nct-cell]
  nct 1 / 2 (tiles of 32 / 64 sequences), cell 0 (separate sigm / tanh) / 1, B = 33,
  L = 3, I = 3 ............................................. err_ref h <= 1.7e-07, c <= 1.6e-07
fm_lstm_cell.h saturation .......................................... test_gpu_lstm_cell_saturation
  pre-activations of every gate past +-90 (an overflowing E_i / E_f / E_o, the
  +-60 clamp on E_g) and within +-1, |c| past 21 (the clamp on E_c) from a c0 of
  +-25 / +-30 ................................................ err_ref h 1.5e-06, c 2.8e-06
lstm_fwd_hist_kernel<H> (HistSource) ............................ test_gpu_lstm_hist_edges[H-I-L]
  32-3-2049  L > kLstmPhaseTab: the per-lane phase, no LDS table . err_ref h 2.6e-04, c 6.0e-04
  64-2-65    I = 2; the prologue's lane loop one past 64 .................... 4.3e-04, 6.6e-04
  128-1-64   the lane loop at 64 ............................................. 1.7e-04, 3.9e-04
  32-0-1     one step, no feature but the bias ............................... 5.5e-09, 9.7e-09
  64-3-120   the production shape ............................................ 3.0e-04, 5.1e-04
  every case B = 70 (6 sequences in the second workgroup), T - L = 37; an all-NaN
             window (n = 0, sd floored), a constant window, one finite sample,
             +-inf, NaN runs at both ends; plain, and through rm / shift / lim / dk
             (lim cutting the newest 0, 1 and L columns, a shift with bc < 0, rm a
             permutation with a repeated row) bit-equal; mu, sd, h and c_out
lstm_features_kernel, lstm_features_mv_kernel ................... test_gpu_lstm_features_edges
  I 0 .. 3, L 1 / 64 / 65 / 130 (the lane loop's edges), R 1 / 5 (a partial block);
  M 1 / 2 / 13 (no empty column above M + 2), S 1 / 3 (S M = 1 .. 39, partial last
  block), L 1 / 65 ................ err_ref mu <= 7.4e-08, sd <= 1.1e-07, z <= 4.3e-07, sin / cos <= 7.2e-07
lstm_stack_kernel<H, RT, 2, layers>, lstm_stack2_rs_kernel<256> .. test_gpu_lstm_stack_edges[...]
  32 / 64 / 128 x 1 / 2 layers (2 x 2), 256 x 1 (4 x 2), 256 x 2 (row-streamed, tile
  64), I 0 / 3 / 15, L 1 / 2 / 3 / 5, B 1 / 33 / 64 / 65; h and c, rows past B, the
  prefix of B = 130 ............................... err_ref h 5.9e-09 .. 4.2e-04, c 1.5e-08 .. 6.7e-04
  4:1p / 8:216 / 4:214 x B  lstm_stack2_pipe_kernel<256, 4, 0 / 4> (tile 32) and
  lstm_stack2_t16_kernel<256> (tile 48) at B 1 / 32 / 33 / 48 / 49, L = 2 .... h 1.2e-04, c 2.5e-04
lstm_head_kernel<H, 16 / 64> ........................................ test_gpu_lstm_head_edges
  Hz 16 / 17 (the NZ switch), Hout < Hz, Hout = 70 (the run-time tail loop), B 256 /
  257 (the block edge), H = 256 with Hz = 64 (65,792 bytes of dynamic LDS, more than
  64 KiB: the launch is accepted and correct) ..... err_ref 3.6e-07 (H = 32, Hz = 1) .. 4.2e-06 (H = 256)
launchers: the error returns of the seven entry points, nothing launched
  ........................................................ test_lstm_launchers_reject_bad_shapes

CPU: test_ref_lstm_matches_fp64_loop holds ``LS.ref_lstm_forward`` and
``LS.ref_lstm_stack`` against the loop; test_forward_bounds_reject_wrong_variants and
test_stack_bounds_reject_wrong_variants show that the measured tolerances refuse the
loop with one rule broken (the g-gate scale taken as -log2 e, the i-gate's bias
dropped, units 8 rt + 3 and 8 rt + 4 of row tile 1 swapped, x column I - 1 read
from column I, h0 ignored, layer 1 fed layer 0's h_{t-1});
test_feature_spec_near_boundary_cap asserts the 1 % cap.

Not reached, because no launcher selects it: ``lstm_stack_kernel`` at H = 256 with
(rt, nct) = (4, 1), (2, 2), (2, 1) and ``lstm_stack2_pipe_kernel<256, 2>`` run only in
test_model_ops.py's tilings test; the ablations ``lstm_stack2_pipe_kernel<256, 4, 1 ..
3>`` (nct 211-213) are wrong by design and run nowhere; the ``FM_LSTM_CELL_AB``
branches of ``lstm_cell`` exist only in A/B builds."""
import functools

import numpy as np
import pytest
import torch

from foremast_amd.ops import lstm as LS
from foremast_amd.ops._lib import LIB, ptr

F32 = np.float32
F64 = np.float64
U = 2.0 ** -24
FLOOR = 32 * U           # the absolute error allowed to lstm_cell on values of at most 1 (module docstring)
PAD = 1e30
SD_FLOOR = float(np.float32(1e-6))
LOG2E = 1.4426950408889634
PERIOD = 144.7          # 4 c / 144.7 = 40 c / 1447 (prime): no phase of a column 0 < c < 1447 is a multiple of pi / 2
SENT = 7.0              # sentinel of the rows behind a batch (exact in bf16)
B_BIG = 130


# =========================================================================== bf16
def bf(v):
    """Round to bf16 (nearest even), in the dtype of ``v``."""
    a = np.asarray(v)
    f = np.ascontiguousarray(a, dtype=F32)
    u = f.view(np.uint32).astype(np.uint64)
    r = (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(F32)
    return np.where(np.isfinite(f), r, f).astype(a.dtype)


def bf_key(v):
    """bf16 values -> integers in the order of the values (+-0 -> 0): a difference
    of keys is a distance in bf16 ulps."""
    i = (np.ascontiguousarray(v, dtype=F32).view(np.uint32) >> 16).astype(np.int64)
    return np.where(i & 0x8000, -(i & 0x7FFF), i)


# =========================================================================== the fp64 loop
def kernel_weights(w, H, D=F64):
    """Gate rows [4H, ...] as the kernels hold them: times the fp32 gate scale,
    rounded to bf16, the exact scale (what exp2 undoes) divided out again."""
    w = np.asarray(w, F32)
    s = LS.gate_scales(H)
    exact = np.repeat(np.array([-LOG2E, -LOG2E, -2 * LOG2E, -LOG2E]), H)
    if w.ndim == 2:
        s, exact = s[:, None], exact[:, None]
    return (bf((w * s).astype(F32)).astype(F64) / exact).astype(D)


def _sigm(x):
    with np.errstate(over="ignore"):
        return 1 / (1 + np.exp(-x))


def spec_lstm(x, layers, h0=None, c0=None, D=F64, teacher=None, broken=None, nudge=0.0):
    """x [B, L, I], layers [(w_ih [4H, I or H], w_hh [4H, H], b [4H])] in fp32 ->
    (hs [B, L, H]: the top layer's h of every step, unrounded; h [B, H]; c [B, H]).
    h0 / c0 belong to layer 0.  ``teacher`` [B, L, H] (bf16 values, one layer): step
    t >= 1 takes teacher[:, t - 1] as its recurrent input in place of the loop's own
    rounded h.  ``nudge`` is added to every computed h before it is rounded for a
    GEMM: an h within |nudge| of a bf16 boundary falls on its other side.
    ``broken`` breaks one rule (the *_reject_wrong_variants tests)."""
    x = np.asarray(x, F32)
    B, L, I = x.shape
    H = layers[0][1].shape[1]
    xs = bf(x).astype(D)
    if broken == "xcol" and I > 0:
        xs[..., I - 1] = 1.0                               # column I of the augmented step holds the bias' 1.0
    Ws = []
    for wi, wh, b in layers:
        wi, wh, b = (np.array(a, F32) for a in (wi, wh, b))
        if broken == "bias":
            b[:H] = 0
        if broken == "swap":
            for a in (wi, wh, b):
                for g in range(4):
                    a[[g * H + 11, g * H + 12]] = a[[g * H + 12, g * H + 11]]
        Ws.append((kernel_weights(wi, H, D), kernel_weights(wh, H, D), kernel_weights(b, H, D)))
    n = len(layers)
    h = [np.zeros((B, H), D) for _ in range(n)]
    c = [np.zeros((B, H), D) for _ in range(n)]
    if h0 is not None and broken != "h0":
        h[0] = np.asarray(h0, F32).astype(D)
    if c0 is not None:
        c[0] = np.asarray(c0, F32).astype(D)
    hr = [bf(v) for v in h]
    hs = np.zeros((B, L, H), D)
    for t in range(L):
        inp = xs[:, t]
        for l, (Wi, Wh, b) in enumerate(Ws):
            rec = hr[l]
            if teacher is not None and t > 0:
                rec = np.asarray(teacher[:, t - 1]).astype(D)
            g = rec @ Wh.T + inp @ Wi.T + b
            gi, gf, gg, go = (g[:, k * H:(k + 1) * H] for k in range(4))
            c[l] = _sigm(gf) * c[l] + _sigm(gi) * np.tanh(gg * D(0.5) if broken == "gscale" else gg)
            h[l] = _sigm(go) * np.tanh(c[l])
            prev = hr[l]
            hr[l] = bf(h[l] + D(nudge)) if nudge else bf(h[l])
            inp = prev if broken == "stale" else hr[l]
        hs[:, t] = h[-1]
    return hs, h[-1], c[-1]


def _feature_moments(win, D):
    """(mu [R], sd [R], z [R, L], computed [R, L]: z is neither a missing sample's 0
    nor an exact 0) of windows [R, L]."""
    v = np.asarray(win, F32).astype(D)
    fin = np.isfinite(v)
    n = np.maximum(fin.sum(1), 1).astype(D)
    with np.errstate(invalid="ignore", over="ignore"):
        mu = (np.where(fin, v, 0).sum(1, dtype=D) / n).astype(D)
        d = np.where(fin, v - mu[:, None], 0).astype(D)
        sd = np.sqrt((d * d).sum(1, dtype=D) / n).astype(D)
        sd = np.maximum(sd, D(SD_FLOOR))
        z = np.where(fin, d / sd[:, None], 0).astype(D)
    # a sample equal to an exactly summed mean (a constant window, a single sample) is 0 in every evaluation
    return mu, sd, z, fin & (z != 0)


def _phase(c_first, L, period, D):
    ph = (D(2 * np.pi) / D(period)) * np.arange(c_first, c_first + L).astype(D)
    return np.sin(ph).astype(D), np.cos(ph).astype(D)


def spec_features(win, c_first, period, I, D=F64):
    """Univariate features of windows [R, L] whose first sample is dense column
    ``c_first`` -> (f [R, L, 16], mu [R], sd [R], exact [R, L, 16]: the elements every
    evaluation gives exactly)."""
    mu, sd, z, fin = _feature_moments(win, D)
    R, L = z.shape
    f = np.zeros((R, L, 16), D)
    exact = np.ones((R, L, 16), bool)
    sn, cs = _phase(c_first, L, period, D)
    for k, col in enumerate((z, sn[None], cs[None])[:I]):
        f[..., k] = col
        exact[..., k] = ~fin if k == 0 else False
    f[..., I] = 1.0
    return f, mu, sd, exact


def spec_features_mv(win, S, M, c_first, period, D=F64):
    """Multivariate features: series s M + m of windows [S M, L] is column m of
    service s; sin, cos, 1.0 at M, M + 1, M + 2 -> (f [S, L, 16], mu [S M], sd [S M], exact)."""
    mu, sd, z, fin = _feature_moments(win, D)
    L = z.shape[1]
    f = np.zeros((S, L, 16), D)
    exact = np.ones((S, L, 16), bool)
    f[..., :M] = z.reshape(S, M, L).transpose(0, 2, 1)
    exact[..., :M] = ~fin.reshape(S, M, L).transpose(0, 2, 1)
    sn, cs = _phase(c_first, L, period, D)
    f[..., M], f[..., M + 1], f[..., M + 2] = sn[None], cs[None], 1.0
    exact[..., M:M + 2] = False
    return f, mu, sd, exact


# =========================================================================== inputs
def lstm_weights(H, I, seed, layers=1):
    """[(w_ih, w_hh, b)] in fp32: w_ih ~ 0.3 N, w_hh ~ N / sqrt(H), b ~ 0.1 N."""
    rng = np.random.default_rng(seed)
    out = []
    for l in range(layers):
        K = I if l == 0 else H
        out.append(((rng.normal(0, 0.3 if l == 0 else 1 / np.sqrt(H), (4 * H, K))).astype(F32),
                    (rng.normal(0, 1 / np.sqrt(H), (4 * H, H))).astype(F32), rng.normal(0, 0.1, 4 * H).astype(F32)))
    return out


def _t(a):
    return torch.from_numpy(np.array(a))


def pack1(ws):
    wi, wh, b = ws[0]
    return LS.pack_lstm(_t(wi), _t(wh), _t(b))


def window_rows(R, L, seed):
    """N(0.3, 1) plus a slow wave: small enough that v - mu keeps its digits."""
    rng = np.random.default_rng(seed)
    return (0.3 + rng.normal(0, 1, (R, L)) + np.sin(np.arange(L) / 7.0 + rng.uniform(0, 6, (R, 1)))).astype(F32)


def special_row(kind, row, L):
    """The rows placed on purpose, in place: 0 NaN runs at both ends, 1 +-inf
    samples, 2 a constant window, 3 one finite sample, 4 an all-NaN window."""
    k = min(3, L // 3)
    if kind == 0 and k:
        row[:k] = np.nan
        row[L - k:] = np.nan
    elif kind == 1 and L >= 3:
        row[L // 3], row[L // 2] = np.inf, -np.inf
    elif kind == 2:
        row[:] = 3.0
    elif kind == 3:
        v = row[L // 2]
        row[:] = np.nan
        row[L // 2] = v
    elif kind == 4:
        row[:] = np.nan
    return row


def padded_history(win, T, pad=5):
    """[R, T + pad] with the windows in columns [T - L, T) and 1e30 everywhere else."""
    R, L = win.shape
    x = np.full((R, T + pad), PAD, F32)
    x[:, T - L:T] = win
    return x


# =========================================================================== comparison
def rule1_errors(hseq, h, c, x, ws, h0, c0):
    """The kernel's (hseq [B, L, H] bf16 values, h, c) against the teacher-forced
    loop.  -> (violations of the hseq bracket, |h - ref|, |c - ref|, eps_h, eps_c,
    err_ref h, err_ref c), each the largest over the batch."""
    hs64, h64, c64 = spec_lstm(x, ws, h0, c0, F64, teacher=hseq)
    hs32, h32, c32 = spec_lstm(x, ws, h0, c0, F32, teacher=hseq)
    err_h = float(np.abs(hs32.astype(F64) - hs64).max())
    err_c = float(np.abs(c32.astype(F64) - c64).max())
    eps_h = max(8 * err_h, FLOOR)
    eps_c = max(8 * err_c, FLOOR * max(1.0, float(np.abs(c64).max())))
    key = bf_key(np.asarray(hseq, F32))
    bad = int(((key < bf_key(bf(hs64 - eps_h))) | (key > bf_key(bf(hs64 + eps_h))) | ~np.isfinite(hseq)).sum())
    with np.errstate(invalid="ignore"):
        dh = float(np.nan_to_num(np.abs(np.asarray(h, F64) - h64), nan=np.inf).max())
        dc = float(np.nan_to_num(np.abs(np.asarray(c, F64) - c64), nan=np.inf).max())
    return bad, dh, dc, eps_h, eps_c, err_h, err_c


def assert_rule1(hseq, h, c, x, ws, h0, c0, what=""):
    bad, dh, dc, eps_h, eps_c, err_h, err_c = rule1_errors(hseq, h, c, x, ws, h0, c0)
    print(f"{what}: hseq outside its bracket {bad}, |dh| {dh:.3g} (eps {eps_h:.3g}), |dc| {dc:.3g} (eps {eps_c:.3g}), "
          f"err_ref h {err_h:.3g} c {err_c:.3g}")
    assert bad == 0, (what, "hseq", bad)
    assert dh <= eps_h, (what, "h", dh, eps_h)
    assert dc <= eps_c, (what, "c", dc, eps_c)
    # the last step of the sequence is the bf16 rounding of the fp32 h
    np.testing.assert_array_equal(np.asarray(hseq, F32)[:, -1], bf(np.asarray(h, F32)), err_msg=what)


def rule2_tol(x, ws, h0=None, c0=None):
    """(h64, c64, tol_h, tol_c, err_ref h, err_ref c) of a free-running case."""
    _, h64, c64 = spec_lstm(x, ws, h0, c0, F64)
    eh = ec = 0.0
    for D, nudge in ((F32, 0.0), (F64, FLOOR), (F64, -FLOOR)):
        _, h, c = spec_lstm(x, ws, h0, c0, D, nudge=nudge)
        eh = max(eh, float(np.abs(h.astype(F64) - h64).max()))
        ec = max(ec, float(np.abs(c.astype(F64) - c64).max()))
    return h64, c64, max(8 * eh, FLOOR), max(8 * ec, FLOOR * max(1.0, float(np.abs(c64).max()))), eh, ec


def assert_rule2(h, c, ref, what=""):
    h64, c64, th, tc, eh, ec = ref
    with np.errstate(invalid="ignore"):
        dh = float(np.nan_to_num(np.abs(np.asarray(h, F64) - h64), nan=np.inf).max())
        dc = float(np.nan_to_num(np.abs(np.asarray(c, F64) - c64), nan=np.inf).max())
    print(f"{what}: |dh| {dh:.3g} (tol {th:.3g}), |dc| {dc:.3g} (tol {tc:.3g}), err_ref h {eh:.3g} c {ec:.3g}")
    assert dh <= th, (what, "h", dh, th)
    assert dc <= tc, (what, "c", dc, tc)


def _ids(c):
    return c if isinstance(c, str) else "-".join(map(str, c))


# =========================================================================== forward cases
FWD_CASES = [(32, 0, 1, 1), (32, 1, 2, 31), (32, 7, 3, 32), (32, 15, 5, 33), (32, 7, 2, 64), (32, 1, 37, 65),
             (64, 1, 1, 64), (64, 7, 2, 65), (64, 15, 3, 1), (64, 0, 5, 130), (64, 0, 3, 31), (64, 1, 5, 33),
             (128, 15, 1, 33), (128, 0, 2, 32), (128, 1, 3, 65), (128, 7, 5, 31), (128, 1, 2, 1), (128, 7, 1, 130)]


@functools.lru_cache(maxsize=None)
def fwd_inputs(H, I, L):
    """(x [130, L, I], weights, h0, c0); a case takes the first B rows."""
    rng = np.random.default_rng(1000 * H + 10 * I + L)
    x = bf(rng.normal(0, 1, (B_BIG, L, I)).astype(F32))
    h0 = rng.normal(0, 0.3, (B_BIG, H)).astype(F32)
    c0 = rng.normal(0, 0.5, (B_BIG, H)).astype(F32)
    ws = lstm_weights(H, I, 77 + H + I)
    for a in (x, h0, c0, *ws[0]):
        a.setflags(write=False)
    return x, ws, h0, c0


def _as_got(x, ws, h0, c0, broken=None):
    """A (broken) free-running fp64 loop in the shape of a kernel's outputs."""
    hs, h, c = spec_lstm(x, ws, h0, c0, F64, broken=broken)
    return bf(hs).astype(F32), h.astype(F32), c.astype(F32)


FWD_VARIANTS = ("gscale", "bias", "swap", "xcol", "h0")


@pytest.mark.parametrize("case", FWD_CASES, ids=_ids)
def test_forward_bounds_reject_wrong_variants(case):
    """Rule 1 accepts the loop itself (rounded as a kernel would store it) and
    refuses it with one rule broken, at every case's shape, with and without h0 /
    c0.  The printed err_ref is the one of the module docstring."""
    H, I, L, B = case
    x, ws, h0, c0 = fwd_inputs(H, I, L)
    x, h0, c0 = x[:B], h0[:B], c0[:B]
    for init in ((h0, c0), (None, None)):
        assert_rule1(*_as_got(x, ws, *init), x, ws, *init, what=f"the loop itself {case}")
        for name in FWD_VARIANTS:
            if (name == "xcol" and I == 0) or (name == "h0" and init[0] is None):
                continue
            with pytest.raises(AssertionError):
                assert_rule1(*_as_got(x, ws, *init, broken=name), x, ws, *init, what=f"{name} {case}")


@pytest.mark.parametrize("H,I,L,B", [(32, 15, 5, 33), (64, 0, 3, 31), (128, 1, 37, 9)])
def test_ref_lstm_matches_fp64_loop(H, I, L, B):
    """``LS.ref_lstm_forward`` and ``LS.ref_lstm_stack`` (fp32, torch) are further
    evaluations of the loop: within rule 2's tolerance of it, one and two layers."""
    x, ws, h0, c0 = fwd_inputs(H, I, L)
    x, h0, c0 = x[:B], h0[:B], c0[:B]
    ref = rule2_tol(x, ws, h0, c0)
    wi, wh, b = (_t(a) for a in ws[0])
    hr, cr = LS.ref_lstm_forward(_t(x), wi, wh, b, _t(h0), _t(c0), emulate_bf16=True)
    assert_rule2(hr.numpy(), cr.numpy(), ref, f"ref_lstm_forward {H}-{I}-{L}")
    ws2 = lstm_weights(H, I, 5 + H, layers=2)
    for ly in (ws2[:1], ws2):
        ref = rule2_tol(x[:, :5], ly)
        hr, cr = LS.ref_lstm_stack(_t(x[:, :5]), [tuple(_t(a) for a in w) for w in ly], emulate_bf16=True)
        assert_rule2(hr.numpy(), cr.numpy(), ref, f"ref_lstm_stack {H}-{I} x {len(ly)}")


def _run_forward(cuda, x, pk, H, h0, c0, seq=True, nct=None, cell=None):
    """fm_lstm_forward (or fm_lstm_forward_v) with outputs 3 rows larger than the
    batch -> (hseq [B, L, H] fp32 values or None, h, c), the spare rows checked."""
    B, L, _ = x.shape
    xa = LS.augment(_t(x).to(cuda))
    hT = torch.full((B + 3, H), SENT, device=cuda)
    cT = torch.full((B + 3, H), SENT, device=cuda)
    sq = torch.full((B + 3, L, H), SENT, dtype=torch.bfloat16, device=cuda) if seq else None
    hd = None if h0 is None else _t(h0).to(cuda)
    cd = None if c0 is None else _t(c0).to(cuda)
    st = torch.cuda.current_stream(cuda).cuda_stream
    if nct is None:
        LIB.call("fm_lstm_forward", ptr(xa), B, L, H, ptr(pk), ptr(hd), ptr(cd), ptr(hT), ptr(cT), ptr(sq), st)
    else:
        LIB.call("fm_lstm_forward_v", ptr(xa), B, L, H, ptr(pk), ptr(hd), ptr(cd), ptr(hT), ptr(cT), ptr(sq), nct,
                 cell, st)
    torch.cuda.synchronize()
    for o in (hT, cT) + ((sq,) if seq else ()):
        assert bool((o[B:] == SENT).all()), "rows at and past B are untouched"
    return (sq[:B].float().cpu().numpy() if seq else None), hT[:B].cpu().numpy(), cT[:B].cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("case", FWD_CASES, ids=_ids)
def test_gpu_lstm_forward_edges(cuda, case):
    """lstm_fwd_pipe_kernel<H, true / false> against the teacher-forced loop: every
    step of hseq, the final h and c; HSEQ = false bit-equal; the batch a prefix of
    B = 130 bit-equal."""
    H, I, L, B = case
    xb, ws, h0b, c0b = fwd_inputs(H, I, L)
    pk = pack1(ws).to(cuda)
    for given in (True, False):
        h0, c0 = (h0b[:B], c0b[:B]) if given else (None, None)
        sq, h, c = _run_forward(cuda, xb[:B], pk, H, h0, c0)
        assert_rule1(sq, h, c, xb[:B], ws, h0, c0, what=f"{case} h0/c0 {'given' if given else 'null'}")
        _, h1, c1 = _run_forward(cuda, xb[:B], pk, H, h0, c0, seq=False)
        np.testing.assert_array_equal(h1, h)
        np.testing.assert_array_equal(c1, c)
        sqb, hb, cb = _run_forward(cuda, xb, pk, H, h0b if given else None, c0b if given else None)
        np.testing.assert_array_equal(sqb[:B], sq)
        np.testing.assert_array_equal(hb[:B], h)
        np.testing.assert_array_equal(cb[:B], c)


@pytest.mark.gpu
@pytest.mark.parametrize("H,nct,cell", [(H, n, c) for H in (32, 64, 128) for n in (1, 2) for c in (0, 1)])
def test_gpu_lstm_forward_variants(cuda, H, nct, cell):
    """lstm_fwd_kernel<H, NCT, CELL>, the A/B baselines of tools/lstm_ab.py, under
    rule 1 at B = 33 (a second workgroup of one row at nct = 1), L = 3."""
    xb, ws, h0b, c0b = fwd_inputs(H, 3, 3)
    B = 33
    pk = pack1(ws).to(cuda)
    for h0, c0 in ((h0b[:B], c0b[:B]), (None, None)):
        sq, h, c = _run_forward(cuda, xb[:B], pk, H, h0, c0, nct=nct, cell=cell)
        assert_rule1(sq, h, c, xb[:B], ws, h0, c0, what=f"variant {H}-{nct}-{cell}")


# =========================================================================== saturation
@functools.lru_cache(maxsize=None)
def saturation_case():
    """H = 32, L = 6, B = 33, I = 3.  Rows 11 .. 32 carry inputs of N(0, 300): their
    pre-activations are +-150; units 5 and 21 have biases of +95 / -95 in every
    gate; rows 0 .. 10 are ordinary.  Rows 2, 3, 15, 16 start from c0 = +-25, +-30."""
    H, L, B, I = 32, 6, 33, 3
    rng = np.random.default_rng(42)
    wi, wh, b = lstm_weights(H, I, 43)[0]
    b = b.copy()
    for g in range(4):
        b[g * H + 5], b[g * H + 21] = 95.0, -95.0
    x = rng.normal(0, 1, (B, L, I))
    x[11:] *= 300.0
    x = bf(x.astype(F32))
    h0 = rng.normal(0, 0.3, (B, H)).astype(F32)
    c0 = rng.normal(0, 0.5, (B, H)).astype(F32)
    c0[2], c0[3], c0[15], c0[16] = 25.0, -25.0, 30.0, -30.0
    return x, [(wi, wh, b)], h0, c0


def test_saturation_case_reaches_every_regime():
    """On the fp64 loop: every gate has pre-activations below -90, above +90 and
    within +-1, and some |c| passes 21 (E_c = 2^60 is |c| = 20.8)."""
    x, ws, h0, c0 = saturation_case()
    H = 32
    Wi, Wh, b = (kernel_weights(a, H) for a in ws[0])
    hs, h, c = spec_lstm(x, ws, h0, c0)
    hr = np.concatenate([bf(h0.astype(F64))[:, None], bf(hs)[:, :-1]], 1)
    g = hr @ Wh.T + bf(x).astype(F64) @ Wi.T + b
    for k in range(4):
        gk = g[..., k * H:(k + 1) * H]
        assert gk.min() < -90 and gk.max() > 90 and (np.abs(gk) < 1).any(), k
    assert np.abs(c).max() > 21 and np.isfinite(hs).all()
    assert_rule1(*_as_got(x, ws, h0, c0), x, ws, h0, c0, what="saturation: the loop itself")
    for name in ("gscale", "bias", "swap", "xcol", "h0"):
        with pytest.raises(AssertionError):
            assert_rule1(*_as_got(x, ws, h0, c0, broken=name), x, ws, h0, c0, what=f"saturation {name}")


@pytest.mark.gpu
def test_gpu_lstm_cell_saturation(cuda):
    """fm_lstm_cell.h where its exponentials overflow or are clamped: every output
    finite and within rule 1 of the loop's exact sigmoid and tanh."""
    x, ws, h0, c0 = saturation_case()
    sq, h, c = _run_forward(cuda, x, pack1(ws).to(cuda), 32, h0, c0)
    assert np.isfinite(sq).all() and np.isfinite(h).all() and np.isfinite(c).all()
    assert_rule1(sq, h, c, x, ws, h0, c0, what="saturation")


# =========================================================================== the history kernel
HIST_CASES = [(32, 3, 2049), (64, 2, 65), (128, 1, 64), (32, 0, 1), (64, 3, 120)]
B_HIST = 70
ROW_NONE, ROW_CONST, ROW_ONE, ROW_INF, ROW_ENDS, ROW_CUT1, ROW_LEFT, ROW_ENDS2, ROW_TWIN = 3, 5, 8, 10, 12, 14, 20, 66, 69


@functools.lru_cache(maxsize=None)
def hist_case(H, I, L):
    """(plain history [70, ld], T, weights, fp64 spec (mu, sd), rule 2 reference,
    (err_ref mu, sd), the uncut windows)."""
    T = L + 37
    win = window_rows(B_HIST, L, 7 * H + I + L)
    for kind, r in ((2, ROW_CONST), (3, ROW_ONE), (1, ROW_INF), (0, ROW_ENDS), (0, ROW_ENDS2)):
        special_row(kind, win[r], L)
    win[ROW_TWIN] = win[ROW_TWIN - 1]
    full = win.copy()                                       # what a resident grid holds
    win[ROW_NONE] = np.nan                                  # lim cuts all L columns
    win[ROW_CUT1, L - 1] = np.nan                           # lim cuts the newest column
    win[ROW_LEFT, :min(3, L)] = np.nan                      # the shift puts these at bc < 0
    ws = lstm_weights(H, I, 900 + H + I)
    f64, mu64, sd64, _ = spec_features(win, T - L, PERIOD, I, F64)
    f32, mu32, sd32, _ = spec_features(win, T - L, PERIOD, I, F32)
    _, h64, c64 = spec_lstm(f64[..., :I], ws, D=F64)
    eh = ec = 0.0
    for f, D, nudge in ((f32, F32, 0.0), (f64, F64, FLOOR), (f64, F64, -FLOOR)):
        _, h, c = spec_lstm(f[..., :I], ws, D=D, nudge=nudge)
        eh, ec = max(eh, float(np.abs(h - h64).max())), max(ec, float(np.abs(c - c64).max()))
    em, es = float(np.abs(mu32 - mu64).max()), float(np.abs(sd32 - sd64).max())
    tol = (max(8 * eh, FLOOR), max(8 * ec, FLOOR * max(1.0, float(np.abs(c64).max()))))
    return padded_history(win, T), T, ws, (mu64, sd64), (h64, c64, *tol, eh, ec), (em, es), full


@pytest.mark.parametrize("case", HIST_CASES, ids=_ids)
def test_hist_case_reference(case):
    """The history cases on the CPU: the special rows are what they are meant to
    be, and rule 2 refuses the loop with one rule broken."""
    H, I, L = case
    x, T, ws, (mu, sd), ref, (em, es), full = hist_case(*case)
    print(f"err_ref hist {case}: h {ref[4]:.3g} c {ref[5]:.3g} mu {em:.3g} sd {es:.3g}")
    assert mu[ROW_NONE] == 0 and sd[ROW_NONE] == SD_FLOOR and sd[ROW_CONST] == SD_FLOOR and sd[ROW_ONE] == SD_FLOOR
    assert mu[ROW_CONST] == 3.0
    f64 = spec_features(x[:, T - L:T], T - L, PERIOD, I)[0][..., :I]
    assert_rule2(*spec_lstm(f64, ws)[1:], ref, "the loop itself")
    for name in ("gscale", "bias", "swap") + (("xcol",) if I else ()):
        with pytest.raises(AssertionError):
            assert_rule2(*spec_lstm(f64, ws, broken=name)[1:], ref, f"{name} {case}")


@pytest.mark.gpu
@pytest.mark.parametrize("case", HIST_CASES, ids=_ids)
def test_gpu_lstm_hist_edges(cuda, case):
    """lstm_fwd_hist_kernel<H>: mu and sd against the fp64 spec, h and c_out against
    the fp64 recurrence on the spec's features (rule 2); the same rows through rm /
    shift / lim / dk bit-equal."""
    H, I, L = case
    x, T, ws, (mu64, sd64), ref, (em, es), full = hist_case(*case)
    B = B_HIST
    pk = pack1(ws).to(cuda)
    hist = _t(x).to(cuda)
    h1, c1, mu1, sd1 = LS.lstm_forward_hist(hist, T, L, PERIOD, I, pk, H, B=B)
    torch.cuda.synchronize()
    got = [t.cpu().numpy() for t in (h1, c1, mu1, sd1)]
    dm, ds = np.abs(got[2] - mu64).max(), np.abs(got[3] - sd64).max()
    print(f"hist {case}: |dmu| {dm:.3g} (tol {8 * em:.3g}) |dsd| {ds:.3g} (tol {8 * es:.3g})")
    assert dm <= 8 * em and ds <= 8 * es
    assert_rule2(got[0], got[1], ref, f"hist {case}")
    # a resident grid: row rm[b], the dense column c at grid column c + o[b], everything else 1e30
    rng = np.random.default_rng(L)
    dk = 3
    o = rng.integers(0, 40, B)
    nleft = min(3, L)
    o[ROW_LEFT] = -(T - L) - nleft
    cut = np.zeros(B, np.int64)
    cut[ROW_CUT1], cut[ROW_NONE] = 1, L
    rm = rng.permutation(B)
    rm[ROW_TWIN], o[ROW_TWIN] = rm[ROW_TWIN - 1], o[ROW_TWIN - 1]
    grid = np.full((B + 5, T + 48), PAD, F32)
    for b in range(B):
        i0 = nleft if b == ROW_LEFT else 0
        grid[rm[b], T - L + i0 + o[b]:T + o[b]] = full[b, i0:]
    t32 = lambda a: _t(np.asarray(a, np.int32)).to(cuda)    # noqa: E731
    h2, c2, mu2, sd2 = LS.lstm_forward_hist(_t(grid).to(cuda), T, L, PERIOD, I, pk, H, t32(rm), t32(dk - o),
                                            t32(o + T - cut - dk), dk)
    torch.cuda.synchronize()
    for a, b_ in zip((h2, c2, mu2, sd2), got):
        np.testing.assert_array_equal(a.cpu().numpy(), b_)


# =========================================================================== the feature kernels
FEAT_UNI = [(I, L, R) for I in (0, 1, 2, 3) for L in (1, 64, 65, 130) for R in (1, 5)]
FEAT_MV = [(M, S, L) for M in (1, 2, 13) for S in (1, 3) for L in (1, 65)]
T_OFF = 37              # T - L
FEAT_SEED = {65: 4004}          # drawn again where a |z| of the first draw was below the band: no bf16 ulp is that small


@functools.lru_cache(maxsize=None)
def feature_pool(L):
    """64 rows of the generator with the five special rows in front, and the
    reference errors over them: (windows, err mu, err sd, band z, band sin / cos)."""
    win = window_rows(64, L, FEAT_SEED.get(L, 300 + L))
    for k in range(5):
        special_row(k, win[k], L)
    f64, mu64, sd64, _ = spec_features(win, T_OFF, PERIOD, 3, F64)
    f32, mu32, sd32, _ = spec_features(win, T_OFF, PERIOD, 3, F32)
    d = np.abs(f32.astype(F64) - f64)
    win.setflags(write=False)
    return (win, float(np.abs(mu32 - mu64).max()), float(np.abs(sd32 - sd64).max()), 8 * float(d[..., 0].max()),
            8 * float(d[..., 1:3].max()))


def feature_bracket(f64, exact, L, zcols):
    """(lo, hi): the bf16 values an element may take; ``zcols`` are the z columns."""
    _, _, _, bz, bp = feature_pool(L)
    band = np.full(f64.shape, bp)
    band[..., np.asarray(zcols, np.int64)] = bz
    band[exact] = 0
    return bf(f64 - band), bf(f64 + band)


def assert_features(got, f64, exact, L, zcols, what=""):
    lo, hi = feature_bracket(f64, exact, L, zcols)
    k = bf_key(got)
    bad = (k < bf_key(lo)) | (k > bf_key(hi)) | ~np.isfinite(got)
    assert not bad.any(), (what, int(bad.sum()), np.argwhere(bad)[:5])
    np.testing.assert_array_equal(got[exact], f64[exact].astype(F32), err_msg=what)


def _uni_windows(L, R):
    return feature_pool(L)[0][:R]


def _mv_windows(L, n):
    """n series: the pool's rows, so that every service meets special rows."""
    return feature_pool(L)[0][:n]


def test_feature_spec_near_boundary_cap():
    """On the two CPU references alone: the elements that may take either of two
    bf16 values are at most 1 % of a case's computed features, the two values are
    one ulp apart, and the fp32 mirror itself lies in the bracket."""
    for I, L, R in FEAT_UNI:
        win = _uni_windows(L, R)
        f64, _, _, ex = spec_features(win, T_OFF, PERIOD, I)
        f32 = spec_features(win, T_OFF, PERIOD, I, F32)[0]
        lo, hi = feature_bracket(f64, ex, L, [0] if I else [])
        gap = bf_key(hi) - bf_key(lo)
        assert gap.max() <= 1, (I, L, R)
        assert (gap > 0).sum() <= 0.01 * max((~ex).sum(), 1), (I, L, R, int((gap > 0).sum()))
        assert_features(bf(f32.astype(F32)), f64, ex, L, [0] if I else [], f"mirror {I}-{L}-{R}")
    for M, S, L in FEAT_MV:
        win = _mv_windows(L, S * M)
        f64, _, _, ex = spec_features_mv(win, S, M, T_OFF, PERIOD)
        f32 = spec_features_mv(win, S, M, T_OFF, PERIOD, F32)[0]
        lo, hi = feature_bracket(f64, ex, L, list(range(M)))
        gap = bf_key(hi) - bf_key(lo)
        assert gap.max() <= 1, (M, S, L)
        assert (gap > 0).sum() <= 0.01 * (~ex).sum(), (M, S, L, int((gap > 0).sum()))
        assert_features(bf(f32.astype(F32)), f64, ex, L, list(range(M)), f"mirror mv {M}-{S}-{L}")
    for L in (1, 64, 65, 130):
        print(f"err_ref features L={L}: mu {feature_pool(L)[1]:.3g} sd {feature_pool(L)[2]:.3g} "
              f"z {feature_pool(L)[3] / 8:.3g} sin/cos {feature_pool(L)[4] / 8:.3g}")


@pytest.mark.gpu
def test_gpu_lstm_features_edges(cuda):
    """lstm_features_kernel and lstm_features_mv_kernel: the bf16 layout by the
    feature rule, the exact elements, mu and sd by rule 2, nothing written behind
    the outputs."""
    st = torch.cuda.current_stream(cuda).cuda_stream

    def run(name, win, rows, nsvc, L, *mid):
        T = L + T_OFF
        hist = _t(padded_history(win, T)).to(cuda)
        xa = torch.full((nsvc + 1, L, 16), SENT, dtype=torch.bfloat16, device=cuda)
        mu = torch.full((rows + 1,), SENT, device=cuda)
        sd = torch.full((rows + 1,), SENT, device=cuda)
        LIB.call(name, ptr(hist), hist.stride(0), T, *mid, ptr(xa), ptr(mu), ptr(sd), st)
        torch.cuda.synchronize()
        assert bool((xa[nsvc] == SENT).all()) and float(mu[rows]) == SENT and float(sd[rows]) == SENT
        return xa[:nsvc].float().cpu().numpy(), mu[:rows].cpu().numpy(), sd[:rows].cpu().numpy()

    def moments(mu, sd, mu64, sd64, L, what):
        _, em, es, _, _ = feature_pool(L)
        dm, ds = np.abs(mu - mu64).max(), np.abs(sd - sd64).max()
        print(f"{what}: |dmu| {dm:.3g} (tol {8 * em:.3g}) |dsd| {ds:.3g} (tol {8 * es:.3g})")
        assert dm <= 8 * em and ds <= 8 * es, what

    for I, L, R in FEAT_UNI:
        win = _uni_windows(L, R)
        xa, mu, sd = run("fm_lstm_features", win, R, R, L, R, L, PERIOD, I)
        f64, mu64, sd64, ex = spec_features(win, T_OFF, PERIOD, I)
        assert_features(xa, f64, ex, L, [0] if I else [], f"features {I}-{L}-{R}")
        moments(mu, sd, mu64, sd64, L, f"features {I}-{L}-{R}")
    for M, S, L in FEAT_MV:
        win = _mv_windows(L, S * M)
        xa, mu, sd = run("fm_lstm_features_mv", win, S * M, S, L, S, M, L, PERIOD)
        f64, mu64, sd64, ex = spec_features_mv(win, S, M, T_OFF, PERIOD)
        assert_features(xa, f64, ex, L, list(range(M)), f"features_mv {M}-{S}-{L}")
        moments(mu, sd, mu64, sd64, L, f"features_mv {M}-{S}-{L}")


# =========================================================================== the stacked kernels
STACK_CASES = [(32, 1, 0, 1, 1), (32, 2, 3, 2, 33), (32, 2, 15, 5, 64), (64, 1, 15, 3, 64), (64, 2, 0, 5, 65),
               (64, 1, 3, 1, 33), (128, 1, 3, 2, 65), (128, 2, 15, 1, 33), (128, 2, 3, 3, 1),
               (256, 1, 3, 2, 33), (256, 1, 0, 1, 65), (256, 1, 15, 5, 1), (256, 2, 3, 1, 33), (256, 2, 15, 2, 65),
               (256, 2, 0, 3, 64), (256, 2, 3, 5, 1)]
TILING_CASES = [f"{t}-{B}" for t in ("4:1p", "8:216", "4:214") for B in (1, 32, 33, 48, 49)]


def _stack_args(case):
    """(H, layers, I, L, B, tiling or None) of a STACK_CASES tuple or a TILING_CASES name."""
    if isinstance(case, str):
        t, B = case.rsplit("-", 1)
        return 256, 2, 3, 2, int(B), t
    return (*case, None)


@functools.lru_cache(maxsize=None)
def stack_inputs(H, layers, I, L):
    rng = np.random.default_rng(31 * H + 7 * layers + I + 1000 * L)
    x = bf(rng.normal(0, 1, (B_BIG, L, I)).astype(F32))
    x.setflags(write=False)
    return x, lstm_weights(H, I, 500 + H + layers + I, layers=layers)


@functools.lru_cache(maxsize=None)
def stack_ref(H, layers, I, L, B):
    """Rule 2's reference of the first B rows; err_ref is taken over all 130 rows of
    the case's inputs (the rows are independent: a batch of one would rest its
    tolerance on 8 H values and, without a bf16 flip among them, on fp32 alone)."""
    h64, c64, th, tc, eh, ec = _stack_ref_all(H, layers, I, L)
    return h64[:B], c64[:B], th, tc, eh, ec


@functools.lru_cache(maxsize=None)
def _stack_ref_all(H, layers, I, L):
    return rule2_tol(*stack_inputs(H, layers, I, L))


STACK_VARIANTS = ("gscale", "bias", "swap", "xcol", "stale")


@pytest.mark.parametrize("case", STACK_CASES + TILING_CASES[:1], ids=_ids)
def test_stack_bounds_reject_wrong_variants(case):
    """Rule 2 accepts the loop itself and refuses it with one rule broken at every
    stacked case's shape.  The printed err_ref is the one of the module docstring."""
    H, layers, I, L, B, _ = _stack_args(case)
    x, ws = stack_inputs(H, layers, I, L)
    ref = stack_ref(H, layers, I, L, B)
    assert_rule2(*spec_lstm(x[:B], ws)[1:], ref, f"the loop itself {case}")
    for name in STACK_VARIANTS:
        if (name == "xcol" and I == 0) or (name == "stale" and layers == 1):
            continue
        with pytest.raises(AssertionError):
            assert_rule2(*spec_lstm(x[:B], ws, broken=name)[1:], ref, f"{name} {case}")


def _run_stack(cuda, x, pk, H):
    B, L, _ = x.shape
    xa = LS.augment(_t(x).to(cuda))
    hT = torch.full((B + 3, H), SENT, device=cuda)
    cT = torch.full((B + 3, H), SENT, device=cuda)
    rt, nct = LS.stack_tiling(H, len(pk))
    LIB.call("fm_lstm_stack", ptr(xa), B, L, H, len(pk), ptr(pk[0]), ptr(pk[1]) if len(pk) > 1 else None, ptr(hT),
             ptr(cT), rt, nct, torch.cuda.current_stream(cuda).cuda_stream)
    torch.cuda.synchronize()
    assert bool((hT[B:] == SENT).all()) and bool((cT[B:] == SENT).all()), "rows at and past B are untouched"
    return hT[:B].cpu().numpy(), cT[:B].cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("case", STACK_CASES + TILING_CASES, ids=_ids)
def test_gpu_lstm_stack_edges(cuda, monkeypatch, case):
    """fm_lstm_stack on the default route (tuples H-layers-I-L-B) and on the other
    H = 256 two-layer tilings that compute a correct h (names tiling-B, L = 2): h and
    c by rule 2, rows past B untouched, the batch a prefix of B = 130 bit-equal."""
    H, layers, I, L, B, tiling = _stack_args(case)
    if tiling is not None:
        monkeypatch.setenv("FM_LSTM_STACK_TILING", tiling)
    x, ws = stack_inputs(H, layers, I, L)
    pk = [p.to(cuda) for p in LS.pack_stack([tuple(_t(a) for a in w) for w in ws], H)]
    h, c = _run_stack(cuda, x[:B], pk, H)
    assert_rule2(h, c, stack_ref(H, layers, I, L, B), f"stack {case}")
    hb, cb = _run_stack(cuda, x, pk, H)
    np.testing.assert_array_equal(hb[:B], h)
    np.testing.assert_array_equal(cb[:B], c)


# =========================================================================== the head
HEAD_HZ = (1, 16, 17, 64)


@pytest.mark.gpu
def test_gpu_lstm_head_edges(cuda):
    """lstm_head_kernel<H, 16 / 64> against mu + sd (h W^T + b) in fp64, the last step
    repeated past Hz; tol = 8 x the largest error of the same expression in fp32."""
    rng = np.random.default_rng(9)
    st = torch.cuda.current_stream(cuda).cuda_stream
    Bm = 257
    for H in (32, 64, 128, 256):
        h = rng.normal(0, 0.5, (Bm, H)).astype(F32)
        mu = rng.normal(0, 2, Bm).astype(F32)
        sd = rng.uniform(0.1, 3, Bm).astype(F32)
        hd, mud, sdd = (_t(a).to(cuda) for a in (h, mu, sd))
        for Hz in HEAD_HZ:
            W = rng.normal(0, 0.1, (Hz, H)).astype(F32)
            b = rng.normal(0, 1, Hz).astype(F32)
            Wd, bd = _t(W).to(cuda), _t(b).to(cuda)
            z64 = mu[:, None].astype(F64) + sd[:, None].astype(F64) * (h.astype(F64) @ W.T.astype(F64) + b)
            z32 = mu[:, None] + sd[:, None] * (h @ W.T + b)
            tol = 8 * float(np.abs(z32 - z64).max())
            for Hout in sorted({1, max(Hz - 1, 1), Hz, Hz + 5, 70}):
                want = z64[:, np.minimum(np.arange(Hout), Hz - 1)]
                for B in (1, 256, 257):
                    fc = torch.full((B + 1, Hout), SENT, device=cuda)
                    LIB.call("fm_lstm_head", ptr(hd), B, H, ptr(Wd), ptr(bd), Hz, ptr(mud), ptr(sdd), Hout, ptr(fc), st)
                    torch.cuda.synchronize()
                    assert bool((fc[B] == SENT).all())
                    d = float(np.abs(fc[:B].cpu().numpy() - want[:B]).max())
                    assert d <= tol, (H, Hz, Hout, B, d, tol)
            print(f"head H={H} Hz={Hz}: tol {tol:.3g}")


# =========================================================================== the launchers' error returns
@pytest.mark.gpu
def test_lstm_launchers_reject_bad_shapes(cuda):
    """Shapes the seven entry points refuse before any launch, and B <= 0, which
    returns 0 without one."""
    d = torch.zeros((1 << 16,), device=cuda)
    p = ptr(d)
    st = torch.cuda.current_stream(cuda).cuda_stream

    def fwd(B=4, L=2, H=32):
        LIB.call("fm_lstm_forward", p, B, L, H, p, None, None, p, p, None, st)

    def fwd_nct(B=4, H=32):
        LIB.call("fm_lstm_forward_nct", p, B, 2, H, p, None, None, p, p, None, 1, st)

    def fwd_v(B=4, H=32):
        LIB.call("fm_lstm_forward_v", p, B, 2, H, p, None, None, p, p, None, 1, 1, st)

    def hist(B=4, L=8, T=16, I=1, period=144.0, shift=None, lim=None, H=32):
        LIB.call("fm_lstm_forward_hist", p, 32, T, None, shift, lim, 0, B, L, H, period, I, p, p, p, p, p, st)

    def stack(B=4, H=128, layers=2, W1=p, rt=0, nct=0):
        LIB.call("fm_lstm_stack", p, B, 2, H, layers, p, W1, p, p, rt, nct, st)

    def head(B=4, H=32, Hz=4, Hout=4):
        LIB.call("fm_lstm_head", p, B, H, p, p, Hz, p, p, Hout, p, st)

    def feat(R=4, L=8, T=16, I=1):
        LIB.call("fm_lstm_features", p, 32, T, R, L, 144.0, I, p, p, p, st)

    def feat_mv(S=2, M=2, L=8, T=16):
        LIB.call("fm_lstm_features_mv", p, 32, T, S, M, L, 144.0, p, p, p, st)

    bad = [(fwd, {"H": 48}), (fwd, {"H": 256}), (fwd_nct, {"H": 16}), (fwd_v, {"H": 96}),
           (hist, {"L": 17}), (hist, {"I": 4}), (hist, {"period": 0.0}), (hist, {"period": -1.0}), (hist, {"shift": p}),
           (hist, {"H": 256}),
           (stack, {"layers": 3}), (stack, {"W1": None}), (stack, {"rt": 4, "nct": 1}), (stack, {"H": 48}),
           (stack, {"H": 256, "rt": 8, "nct": 2}),
           (head, {"Hz": 0}), (head, {"Hz": 65}), (head, {"Hout": 0}), (head, {"H": 48}),
           (feat, {"L": 17}), (feat, {"I": 4}), (feat_mv, {"M": 14}), (feat_mv, {"M": 0}), (feat_mv, {"L": 17})]
    for fn, kw in bad:
        with pytest.raises(RuntimeError):
            fn(**kw)
    for fn in (fwd, fwd_nct, fwd_v, hist, stack, head):
        fn(B=0)
        fn(B=-3)
    feat(R=0)
    feat_mv(S=0)
    torch.cuda.synchronize()
    assert not d.any()
