#!/usr/bin/env python3
"""Bit-for-bit A/B of the seasonal and trend robust kernels (K14, K16, K20,
K22) between two builds of the HIP library.

``python tools/seasonal_dump.py dump OUT.npz`` runs the four ops on the GPU
with the library the process loads (``FOREMAST_HIP_LIB`` selects another
build) and saves every output array.  The inputs are the GPU tests' own:
the ``SHAPES`` and the row generators of ``tests/test_seasonal_ops.py``,
``test_trend_ops.py``, ``test_seasonal_trend_ops.py`` and
``test_seasonal_scale_ops.py``, with their seeds.  Each seasonal shape runs
at H = 3 and H = m + 5, with the smoothing widths at 0 and at their defaults,
and once on a view that starts off a 16-byte boundary in an odd-stride buffer.

``python tools/seasonal_dump.py compare A.npz B.npz [C.npz ...]`` compares
every file with the first: the same arrays, NaN in the same places and equal
bits elsewhere.  It prints one line per file and exits 1 on any difference.
Run each dump in a fresh process, one per library.
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path[:0] = [str(ROOT), str(ROOT / "tests")]


def _view(torch, x, T, off, dev):
    """x as the view that starts at column off of an odd-stride buffer."""
    ld = T + 5 + T % 2
    buf = np.full((x.shape[0], ld), 1e9, np.float32)
    buf[:, off:off + T] = x
    return torch.from_numpy(buf).to(dev)[:, off:]


def dump(out: str) -> None:
    import torch

    import test_seasonal_ops as t14
    import test_seasonal_scale_ops as t22
    import test_seasonal_trend_ops as t20
    import test_trend_ops as t16
    from foremast_amd.ops import misc as MI

    dev = torch.device("cuda")
    arrays = {}

    def keep(tag, got):
        for i, t in enumerate(got):
            arrays[f"{tag}/{i}"] = t.cpu().numpy()

    for i, (m, T, R) in enumerate(t14.SHAPES):
        x = t14._batch(R, T, m, 1000 + T + m)
        d = torch.from_numpy(x).to(dev)
        for H in (3, m + 5):
            for smooth in (0, 5):
                keep(f"K14/m{m}_T{T}/H{H}_k{smooth}", MI.seasonal_robust(d, T, m, H, smooth, want_profile=True))
        off = 1 + i % 3
        keep(f"K14/m{m}_T{T}/view{off}", MI.seasonal_robust(_view(torch, x, T, off, dev), T, m, m + 5, 5,
                                                              want_profile=True))

    for i, (T, L) in enumerate(t16.SHAPES):
        x, _ = t16._gpu_batch(T, L)
        keep(f"K16/T{T}_L{L}/dense", MI.trend_robust(torch.from_numpy(x.copy()).to(dev), T, L))
        keep(f"K16/T{T}_L{L}/mb2", MI.trend_robust(torch.from_numpy(x.copy()).to(dev), T, L, 2))
        off = 1 + i % 3
        keep(f"K16/T{T}_L{L}/view{off}", MI.trend_robust(_view(torch, x, T, off, dev), T, L))

    for i, (m, T, R) in enumerate(t20.SHAPES):
        x = t20._batch(R, T, m, 2000 + T + m)
        d = torch.from_numpy(x).to(dev)
        for H in (3, m + 5):
            for smooth in (0, 5):
                keep(f"K20/m{m}_T{T}/H{H}_k{smooth}", MI.seasonal_trend_robust(d, T, m, H, smooth, want_profile=True))
        keep(f"K20/m{m}_T{T}/mb2", MI.seasonal_trend_robust(d, T, m, 3, 5, 2, want_profile=True))
        off = 1 + i % 3
        keep(f"K20/m{m}_T{T}/view{off}", MI.seasonal_trend_robust(_view(torch, x, T, off, dev), T, m, m + 5, 5,
                                                                    want_profile=True))

    for i, (m, T, R) in enumerate(t22.SHAPES):
        x = t22._batch(R, T, m, 2000 + T + m)
        d = torch.from_numpy(x).to(dev)
        for H in (3, m + 5):
            for smooth, ss in ((0, 0), (5, 30), (0, 30), (5, 0)):
                keep(f"K22/m{m}_T{T}/H{H}_k{smooth}_w{ss}",
                     MI.seasonal_scale_robust(d, T, m, H, smooth, ss, t22.FLOOR, want_profile=True))
        off = 1 + i % 3
        keep(f"K22/m{m}_T{T}/view{off}", MI.seasonal_scale_robust(_view(torch, x, T, off, dev), T, m, m + 5, 5, 30,
                                                                    t22.FLOOR, want_profile=True))

    torch.cuda.synchronize()
    np.savez(out, **arrays)
    print(f"{out}: {len(arrays)} arrays, {sum(a.size for a in arrays.values())} values")


def _same_bits(a, b) -> bool:
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool(np.array_equal(a, b))
    na, nb = np.isnan(a), np.isnan(b)
    bits = np.dtype(f"u{a.dtype.itemsize}")
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(bits)[~na], b.view(bits)[~nb]))


def compare(paths: list[str]) -> int:
    first = np.load(paths[0])
    bad = 0
    for p in paths[1:]:
        other = np.load(p)
        names = sorted(set(first.files) | set(other.files))
        diff = [n for n in names if n not in first.files or n not in other.files or not _same_bits(first[n], other[n])]
        per = {k: sum(n.startswith(k + "/") for n in names) for k in ("K14", "K16", "K20", "K22")}
        print(f"{paths[0]} vs {p}: {len(names)} arrays ({', '.join(f'{k} {v}' for k, v in per.items())}), "
              f"{sum(first[n].size for n in first.files)} values, {len(diff)} differ"
              + ("" if not diff else ": " + ", ".join(diff[:20])))
        bad += len(diff)
    print("every array equal" if bad == 0 else f"{bad} arrays differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) >= 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2:]))
    else:
        sys.exit(__doc__)
