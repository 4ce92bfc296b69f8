"""The run-free path of the pairwise rank rows (avg_ranks skips the tie-run
scans when a sorted array has no tie): exact sufficient statistics of the sort
form against the numpy oracle of test_pairwise_lean (bit for bit), against the
counting form (which has no such path) and the Welch columns as that file
checks them, on rows built to take each path.

A sorted array takes the run-free path if and only if its tie term is 0, the
pooled sample and the Wilcoxon |d| each on their own, so every test first
asserts through the oracle (on the CPU) that each row is in the state its
name claims: that fixes the path the row takes on the device."""
import numpy as np
import pytest
import torch

import test_pairwise_lean as lean
from foremast_amd.ops import canary as C
from foremast_amd.ops import reference as ref

R = lean.R                                   # 37: not a multiple of the 4 rows per workgroup
N1, N2, NW, R1, TIE, DMAX, RPLUS, TIEW, NPOS, NZERO = range(10)      # columns of the oracle (lean.EXACT order)
FLT_MAX = np.finfo(np.float32).max

RUNFREE_SHAPES = [(1, 1), (2, 63), (50, 50), (64, 64), (65, 63), (33, 31), (130, 100), (300, 200), (512, 512)]
TIE_SHAPES = [(50, 50), (64, 64), (130, 100)]


# ---------------------------------------------------------------------------
# inputs


def _d32(c, b):
    npair = min(len(c), len(b))
    with np.errstate(invalid="ignore", over="ignore"):
        return (c[:npair] - b[:npair]).astype(np.float32)


def _distinct_row(rng, n1, n2, draw=None):
    """One row whose pooled values are all distinct and whose fp32 differences
    are non-zero with distinct |d|: drawn, and redrawn where a duplicate shows."""
    draw = draw or (lambda k: rng.normal(10.0, 3.0, k).astype(np.float32))
    while True:
        v = draw(n1 + n2)
        c, b = v[:n1].copy(), v[n1:].copy()
        ad = np.abs(_d32(c, b))
        if len(np.unique(v)) == n1 + n2 and (ad != 0).all() and len(np.unique(ad)) == len(ad):
            return c, b


def _distinct(seed, n1, n2, rows=R, draw=None):
    rng = np.random.default_rng(seed)
    rows_ = [_distinct_row(rng, n1, n2, (lambda k: draw(rng, k)) if draw else None) for _ in range(rows)]
    return np.stack([c for c, _ in rows_]), np.stack([b for _, b in rows_])


def _tie_runs(x):
    """Start positions (in sorted order) of the runs of equal neighbours among the finite x."""
    s = np.sort(x[np.isfinite(x)].astype(np.float64))
    return np.flatnonzero(s[1:] == s[:-1])


def _one_pooled_tie(rng, n1, n2, pos, kind):
    """A row whose only tie is one pooled run of two at sorted positions
    (pos, pos + 1), between one current and one baseline value (kind "cross")
    or inside one sample ("cur" / "base"); all |d| stay distinct and non-zero."""
    n = n1 + n2
    while True:
        c, b = _distinct_row(rng, n1, n2)
        s = np.sort(np.concatenate([c, b]))
        s[pos + 1] = s[pos]
        rest = np.delete(s, [pos, pos + 1])
        rng.shuffle(rest)
        if kind == "cross":
            i, j = int(rng.integers(n1)), n1 + int(rng.integers(n2))
        elif kind == "cur":
            i, j = (int(x) for x in rng.choice(n1, 2, replace=False))
        else:
            i, j = (n1 + int(x) for x in rng.choice(n2, 2, replace=False))
        v = np.empty(n, np.float32)
        free = np.ones(n, bool)
        free[[i, j]] = False
        v[i] = v[j] = s[pos]
        v[free] = rest
        c, b = v[:n1].copy(), v[n1:].copy()
        ad = np.abs(_d32(c, b))
        if (ad != 0).all() and len(np.unique(ad)) == len(ad):
            return c, b


def _grid_row(rng, n1, n2):
    """Distinct multiples of 2^-6 (differences are exact), distinct non-zero |d|."""
    return _distinct_row(rng, n1, n2, lambda k: (rng.choice(np.arange(1, 1 << 16), k, replace=False) / 64.0)
                         .astype(np.float32))


def _state_row(rng, n1, n2, state):
    """Rows in which the pooled sample and the Wilcoxon |d| are in different states."""
    npair = min(n1, n2)
    while True:
        c, b = _grid_row(rng, n1, n2)
        j1, j2 = (int(x) for x in rng.choice(npair, 2, replace=False))
        if state == "d_tie_same_sign":            # pooled distinct, |d| of two pairs equal, same signs
            c[j2] = b[j2] + (c[j1] - b[j1])
        elif state == "d_tie_opposite_sign":      # ... opposite signs
            c[j2] = b[j2] - (c[j1] - b[j1])
        elif state == "pooled_tie_only":          # one current value equals one baseline value of another pair
            c[j1] = b[j2]
        elif state == "zero_difference":          # a pooled tie inside one pair: d == 0 leaves the |d| sample
            c[j1] = b[j1]
        else:
            raise KeyError(state)
        pooled_runs, d = _tie_runs(np.concatenate([c, b])), _d32(c, b)
        d_runs = _tie_runs(np.abs(d[d != 0]))
        want = {"d_tie_same_sign": (0, 1, 0), "d_tie_opposite_sign": (0, 1, 0), "pooled_tie_only": (1, 0, 0),
                "zero_difference": (1, 0, 1)}[state]
        if (len(pooled_runs), len(d_runs), int((d == 0).sum())) == want and (c > 0).all():
            return c, b


STATES = ["d_tie_same_sign", "d_tie_opposite_sign", "pooled_tie_only", "zero_difference"]


def _states_case(n1, n2):
    rng = np.random.default_rng(9000 + n1 * 7 + n2)
    rows = [_state_row(rng, n1, n2, STATES[r % len(STATES)]) for r in range(R)]
    return np.stack([c for c, _ in rows]), np.stack([b for _, b in rows])


def _assert_states(o):
    for r in range(R):
        st = STATES[r % len(STATES)]
        tie, tiew, nzero = o[r, TIE], o[r, TIEW], o[r, NZERO]
        if st.startswith("d_tie"):
            assert (tie, tiew, nzero) == (0, 6, 0), (r, st)
        elif st == "pooled_tie_only":
            assert (tie, tiew, nzero) == (6, 0, 0), (r, st)
        else:
            assert (tie, tiew, nzero) == (6, 0, 1), (r, st)


def _places(n1, n2):
    n = n1 + n2
    p = {"first": 0, "last": n - 2, "63|64": 63}
    if n > 129:
        p["127|128"] = 127
    return p


def _one_tie_case(n1, n2):
    """Row r: one pooled tie at place r % #places, kind (r // #places) % 3."""
    rng = np.random.default_rng(7000 + n1 * 7 + n2)
    places, kinds = list(_places(n1, n2).values()), ["cross", "cur", "base"]
    want = [(places[r % len(places)], kinds[(r // len(places)) % 3]) for r in range(R)]
    rows = [_one_pooled_tie(rng, n1, n2, pos, kind) for pos, kind in want]
    return np.stack([c for c, _ in rows]), np.stack([b for _, b in rows]), want


def _assert_one_tie(cur, base, want, o):
    n1 = cur.shape[1]
    for r, (pos, kind) in enumerate(want):
        v = np.concatenate([cur[r], base[r]])
        assert list(_tie_runs(v)) == [pos], (r, pos)
        x = np.sort(v)[pos]
        where = np.flatnonzero(v == x)
        assert len(where) == 2
        side = (where < n1).sum()
        assert side == {"cross": 1, "cur": 2, "base": 0}[kind]
        assert o[r, TIE] == 6 and o[r, TIEW] == 0 and o[r, NZERO] == 0


def _equality_case(n1, n2):
    """Row r % 3 == 0: the only pooled tie is -0.0 against +0.0; 1: subnormal
    values and differences, distinct as bit patterns; 2: FLT_MAX is the largest
    real value, beside pads."""
    rng = np.random.default_rng(5000 + n1 * 7 + n2)
    npair = min(n1, n2)
    tiny = np.float32(2.0 ** -149)
    rows = []
    for r in range(R):
        if r % 3 == 0:
            while True:
                c, b = _distinct_row(rng, n1, n2)
                j1, j2 = (int(x) for x in rng.choice(npair, 2, replace=False))
                c[j1], b[j2] = np.float32(-0.0), np.float32(0.0)
                ad = np.abs(_d32(c, b))
                if (ad != 0).all() and len(np.unique(ad)) == len(ad):
                    break
        elif r % 3 == 1:
            c, b = _distinct_row(rng, n1, n2, lambda k: (rng.choice(np.arange(1, 1 << 15), k, replace=False) * tiny)
                                 .astype(np.float32))
            assert (np.concatenate([c, b]) < np.finfo(np.float32).tiny).all()
        else:
            c, b = _distinct_row(rng, n1, n2)
            c[int(rng.integers(n1))] = FLT_MAX               # baselines are ~10 +- 3: the difference stays finite
            c[int(rng.integers(n1))] = np.nan                # (may replace FLT_MAX's neighbour or a value: a pad)
            b[int(rng.integers(n2))] = np.inf
            if not (c == FLT_MAX).any():
                c[int(np.flatnonzero(np.isfinite(c))[0])] = FLT_MAX
            assert np.isfinite(_d32(c, b)[np.isfinite(c[:npair]) & np.isfinite(b[:npair])]).all()
        rows.append((c, b))
    return np.stack([c for c, _ in rows]), np.stack([b for _, b in rows])


def _assert_equality(cur, base, o):
    for r in range(R):
        if r % 3 == 0:
            v = np.concatenate([cur[r], base[r]])
            z = v[v == 0]
            assert sorted(np.signbit(z)) == [False, True]
            assert len(np.unique(v.view(np.uint32))) == len(v)          # distinct as bit patterns
            assert (o[r, TIE], o[r, TIEW], o[r, NZERO]) == (6, 0, 0)
        else:
            assert (o[r, TIE], o[r, TIEW], o[r, NZERO]) == (0, 0, 0)
        if r % 3 == 2:
            assert np.nanmax(np.where(np.isfinite(cur[r]), cur[r], np.nan)) == FLT_MAX
            assert o[r, N1] < cur.shape[1] and o[r, N2] < base.shape[1]


def _missing_case(n1, n2, n_real=None):
    """Distinct rows with missing samples.  Row r % 4 == 0: NaN, +inf and -inf
    entries (pads next to the largest real value); 1: the current sample all
    NaN (n1 = 0); 2: both samples all NaN (n = 0); 3: nothing missing.  With
    n_real every row of kinds 0 and 3 keeps exactly n_real finite values."""
    rng = np.random.default_rng(3000 + n1 * 7 + n2)
    cur, base = _distinct(3001 + n1 * 7 + n2, n1, n2)
    for r in range(R):
        v = np.concatenate([cur[r], base[r]])
        if r % 4 == 1:
            v[:n1] = np.nan
        elif r % 4 == 2:
            v[:] = np.nan
        elif r % 4 == 0 or n_real is not None:
            k = (n1 + n2 - n_real) if n_real is not None else max(1, (n1 + n2) // 8)
            where = rng.choice(n1 + n2, k, replace=False)
            v[where] = np.array([np.nan, np.inf, -np.inf], np.float32)[np.arange(k) % 3]
        cur[r], base[r] = v[:n1], v[n1:]
    return cur, base


def _assert_missing(cur, base, o, n_real=None):
    for r in range(R):
        assert o[r, TIE] == 0 and o[r, TIEW] == 0
        if r % 4 == 1:
            assert o[r, N1] == 0 and o[r, N2] == base.shape[1]
        elif r % 4 == 2:
            assert o[r, N1] == 0 and o[r, N2] == 0 and o[r, NW] == 0
        elif n_real is not None:
            assert o[r, N1] + o[r, N2] == n_real
        elif r % 4 == 0:
            assert 0 < o[r, N1] + o[r, N2] < cur.shape[1] + base.shape[1]
        else:
            assert o[r, N1] + o[r, N2] == cur.shape[1] + base.shape[1]


MISSING = [(50, 50, None), (33, 31, None), (130, 100, None), (32, 32, None), (64, 64, None), (40, 40, 64), (70, 70, 128)]


def _interleaved_case(n1, n2, first_tied, stride):
    """Run-free and tied rows alternate along the rows ONE wave ranks (a wave
    takes every stride-th row): run-free / tied / run-free ... or the reverse.
    Tied rows: long runs in both sorts (three values), or a single pooled tie."""
    rng = np.random.default_rng(1000 + n1 * 7 + n2 + first_tied)
    cur, base = _distinct(1001 + n1 * 7 + n2, n1, n2)
    three_c, three_b = lean._pattern("three_values", n1, n2)
    tied = np.zeros(R, bool)
    for r in range(R):
        visit = r // stride
        tied[r] = (visit % 2 == 0) == bool(first_tied)
        if tied[r]:
            if visit % 4 < 2:
                cur[r], base[r] = three_c[r], three_b[r]
            else:
                cur[r], base[r] = _one_pooled_tie(rng, n1, n2, int(rng.integers(n1 + n2 - 1)), "cross")
    return cur, base, tied


def _assert_interleaved(o, tied):
    assert ((o[:, TIE] > 0) == tied).all()
    assert (o[~tied, TIEW] == 0).all()
    assert tied.any() and (~tied).any()


# ---------------------------------------------------------------------------
# CPU: the oracle agrees with the reference on these inputs


def _cpu_cases():
    yield _distinct(11, 50, 50)
    yield _distinct(12, 65, 63)
    yield _one_tie_case(130, 100)[:2]
    yield _states_case(50, 50)
    yield _equality_case(50, 50)
    yield _missing_case(33, 31)
    yield _missing_case(70, 70, 128)
    yield _interleaved_case(50, 50, 1, 4)[:2]


def test_oracle_matches_reference_on_runfree_inputs():
    for cur, base in _cpu_cases():
        o = lean.oracle_suff(cur, base)
        s = ref.pairwise_suff(cur, base)
        np.testing.assert_array_equal(o, s[:, lean.EXACT])


def test_inputs_are_what_they_claim():
    """The state assertions of the GPU tests, where there is no GPU."""
    cur, base = _distinct(21, 50, 50)
    o = lean.oracle_suff(cur, base)
    assert (o[:, TIE] == 0).all() and (o[:, TIEW] == 0).all() and (o[:, NZERO] == 0).all()
    cur, base, want = _one_tie_case(64, 64)
    _assert_one_tie(cur, base, want, lean.oracle_suff(cur, base))
    _assert_states(lean.oracle_suff(*_states_case(50, 50)))
    cur, base = _equality_case(50, 50)
    _assert_equality(cur, base, lean.oracle_suff(cur, base))
    cur, base = _missing_case(40, 40, 64)
    _assert_missing(cur, base, lean.oracle_suff(cur, base), 64)
    cur, base, tied = _interleaved_case(50, 50, 0, 4)
    _assert_interleaved(lean.oracle_suff(cur, base), tied)


# ---------------------------------------------------------------------------
# GPU


def _suff(cuda, cur, base, variant, max_blocks=0):
    from foremast_amd.ops._lib import LIB, ptr, stream_of
    c, b = torch.from_numpy(cur).to(cuda), torch.from_numpy(base).to(cuda)
    suff = torch.full((cur.shape[0], C.SUFF), -1.0, dtype=torch.float64, device=cuda)
    LIB.call("fm_pairwise_suff_v", ptr(c), c.stride(0), cur.shape[1], ptr(b), b.stride(0), base.shape[1],
             cur.shape[0], ptr(suff), max_blocks, variant, stream_of(c))
    torch.cuda.synchronize()
    return suff.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("n1,n2", RUNFREE_SHAPES)
def test_gpu_runfree_rows(cuda, n1, n2):
    cur, base = _distinct(n1 * 1031 + n2, n1, n2)
    o = lean.oracle_suff(cur, base)
    assert (o[:, TIE] == 0).all() and (o[:, TIEW] == 0).all() and (o[:, NZERO] == 0).all()
    assert (o[:, N1] == n1).all() and (o[:, N2] == n2).all()
    lean._check(cuda, cur, base)


@pytest.mark.gpu
@pytest.mark.parametrize("n1,n2", TIE_SHAPES)
def test_gpu_one_tie_at_each_place(cuda, n1, n2):
    """One run of two at sorted positions (0, 1), (n - 2, n - 1), across the
    register boundaries 63 | 64 and 127 | 128, between the samples and inside
    either: the places a neighbour test can miss."""
    cur, base, want = _one_tie_case(n1, n2)
    assert {p for p, _ in want} == set(_places(n1, n2).values()) and {k for _, k in want} == {"cross", "cur", "base"}
    _assert_one_tie(cur, base, want, lean.oracle_suff(cur, base))
    lean._check(cuda, cur, base)


@pytest.mark.gpu
@pytest.mark.parametrize("n1,n2", [(50, 50), (130, 100)])
def test_gpu_pooled_and_wilcoxon_decide_separately(cuda, n1, n2):
    cur, base = _states_case(n1, n2)
    _assert_states(lean.oracle_suff(cur, base))
    lean._check(cuda, cur, base)


@pytest.mark.gpu
@pytest.mark.parametrize("n1,n2", [(50, 50), (33, 31), (130, 100)])
def test_gpu_equality_semantics(cuda, n1, n2):
    cur, base = _equality_case(n1, n2)
    _assert_equality(cur, base, lean.oracle_suff(cur, base))
    lean._check(cuda, cur, base)


@pytest.mark.gpu
@pytest.mark.parametrize("n1,n2,n_real", MISSING)
def test_gpu_missing_samples(cuda, n1, n2, n_real):
    cur, base = _missing_case(n1, n2, n_real)
    _assert_missing(cur, base, lean.oracle_suff(cur, base), n_real)
    lean._check(cuda, cur, base)


@pytest.mark.gpu
@pytest.mark.parametrize("first_tied", [0, 1])
@pytest.mark.parametrize("n1,n2", [(50, 50), (130, 100)])
def test_gpu_interleaved_paths(cuda, n1, n2, first_tied):
    """One workgroup ranks all 37 rows, so each of its four waves takes rows r,
    r + 4, ... and alternates between the two paths: nothing may carry over
    from one row to the next."""
    cur, base, tied = _interleaved_case(n1, n2, first_tied, 4)
    want = lean.oracle_suff(cur, base)
    _assert_interleaved(want, tied)
    one_wg, count = _suff(cuda, cur, base, 0, max_blocks=1), _suff(cuda, cur, base, 1)
    np.testing.assert_array_equal(one_wg[:, lean.EXACT], want)
    np.testing.assert_array_equal(one_wg[:, lean.EXACT], count[:, lean.EXACT])
    np.testing.assert_array_equal(one_wg, _suff(cuda, cur, base, 0))      # a wave per row: all 14 columns
    lean._check(cuda, cur, base)


ALIASES = ["error5xx", "latency", "traffic", "error4xx", "cpu", "memory", "tomcat_threads", "jvm_heap"]


@pytest.mark.gpu
def test_gpu_front_kernels_equal_serial_and_standalone(cuda):
    """Both front kernels (the streaming tick runs the static pairwise role, the
    cached tick the dynamic one) on a fleet of run-free rows with a few tied
    ones, also with few workgroups that take many rows each."""
    from foremast_amd.engine.scorer import CanaryScorer
    h, b, c = C.synth_fleet(9, 8, 300, 5, 10, device=cuda)
    bn, cn = b.cpu().numpy(), c.cpu().numpy()
    three_c, three_b = lean._pattern("three_values", 50, 50)
    rng = np.random.default_rng(77)
    for k, r in enumerate((0, 5, 6, 7, 30, 41, 71)):         # neighbours in one workgroup, first and last row
        if k % 2 == 0:
            cn[r], bn[r] = three_c[k], three_b[k]
        else:
            cn[r], bn[r] = _one_pooled_tie(rng, 50, 50, (0, 98, 63)[k // 2], "cross")
    o = lean.oracle_suff(cn, bn)
    tied = (o[:, TIE] > 0) | (o[:, TIEW] > 0)
    assert tied[[0, 5, 6, 7, 30, 41, 71]].all() and (~tied).sum() >= 36       # both paths, in number
    b, c = torch.from_numpy(bn).to(cuda), torch.from_numpy(cn).to(cuda)
    want = CanaryScorer(ALIASES, device=cuda, mode="serial").score(h, b, c, 300)
    alone = _suff(cuda, cn, bn, 0)
    np.testing.assert_array_equal(alone[:, lean.EXACT], o)
    for kw in ({}, {"front_wgs": (0.02, 0.1)}):
        sc = CanaryScorer(ALIASES, device=cuda, mode="front", **kw)
        for _ in range(2):                  # a tick that streams the history, then a cached one
            out = sc.score(h, b, c, 300)
            torch.cuda.synchronize()
            torch.testing.assert_close(out.pvals, want.pvals, rtol=0, atol=0, equal_nan=True)
            torch.testing.assert_close(out.pstats, want.pstats, rtol=0, atol=0, equal_nan=True)
            assert torch.equal(out.packed, want.packed)
            np.testing.assert_array_equal(out.suff.cpu().numpy(), alone)
