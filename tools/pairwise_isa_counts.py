#!/usr/bin/env python3
"""Instruction histogram of the pairwise row bodies in a gfx950 assembly file.

    hipcc --offload-arch=gfx950 -O3 -fPIC -std=c++17 -ffp-contract=fast \
        -munsafe-fp-atomics -Icsrc/include -mllvm -pragma-unroll-threshold=1000000 \
        --cuda-device-only -S -o pairwise.s csrc/kernels/pairwise.hip
    python tools/pairwise_isa_counts.py pairwise.s pairwise_kernelILi2E

A kernel's instruction stream is cut at every wave-uniform branch (``s_branch``,
``s_cbranch_scc*``, ``s_cbranch_vcc*``; the ``s_cbranch_execz`` skips of
divergent ifs stay inside a piece).  A piece with at least ten
``v_permlane*_swap`` is a sorted row body: ``pw_row<2>`` has two, the split
layout (each sample <= 64 values; the smaller piece, its tags join only for the
last merge) and the pooled one.  Counts are static, one pass of the body = one
row.

``--paths`` (first argument) follows a row body through the wave-uniform
branches inside it.  Since the tie handling has a run-free path (avg_ranks
decides by ballot whether a sorted array has any tie run and skips the scans
when it has none), a row body is no longer one piece: each of the two sorts is
followed by a two-way scalar branch whose arms meet again.  The walk starts at
the piece that holds the layout's first permlane swaps; at a conditional
uniform branch whose two arms are straight-line code that meets again further
down, it takes the arm with fewer VALU for the "run-free" total and the arm
with more for the "tied" total (that arm must hold the scans: at least eight
DPP add/min/max), and goes on from the meeting point; any other uniform branch
ends the body, as it ends the single piece of an assembly
without such branches (there both totals are that piece's).  Per path the
counts are those of the default mode (whose own pieces, on such an assembly, end
at the first of these branches: the sort and the detection, not the row).

    python tools/pairwise_isa_counts.py --paths pairwise.s pairwise_kernelILi2E

``--loop`` (first argument) counts the whole row loop instead: every block of
the outermost loop that holds the permlane swaps, i.e. both layouts plus what
they share (a row's tail behind the last wave-uniform branch -- the queue
kernel's read-back of its next index -- is cut off the row-body pieces above,
and the compiler may merge the two layouts' tails into one).  It adds the
fp64, global-store and LDS-write counts of that loop.
"""
from __future__ import annotations

import re
import sys

UNIFORM = ("s_branch", "s_cbranch_scc", "s_cbranch_vcc", "s_endpgm", "s_setpc", "s_swappc")


def kernel_body(text: str, sub: str):
    for m in re.finditer(r"^([A-Za-z_][\w.$]*):\s*; @\1\n(.*?)^\.Lfunc_end", text, re.S | re.M):
        if sub in m.group(1):
            yield m.group(1), m.group(2)


def pieces(body: str):
    cur = []
    for raw in body.split("\n"):
        ln = raw.strip()
        if not ln or ln.startswith((".", ";")) or ln.split(";")[0].strip().endswith(":"):
            continue
        cur.append(ln)
        if ln.startswith(UNIFORM):
            yield cur
            cur = []
    if cur:
        yield cur


def hist(ins: list[str]) -> dict:
    op = [i.split()[0] for i in ins]
    n = lambda f: sum(1 for i in ins if f(i))
    valu = [i for i in ins if i.startswith("v_")]
    return {
        "all": len(ins),
        "s_nop": n(lambda i: i.startswith("s_nop")),
        "SALU": n(lambda i: i.startswith("s_") and not i.startswith(("s_nop", "s_waitcnt"))),
        "s_xor_b64": op.count("s_xor_b64"),
        "VALU": len(valu),
        "v_mov_b32 dpp": n(lambda i: i.startswith("v_mov_b32") and "dpp" in i.split(";")[0]),
        "v_mov_b32 plain": n(lambda i: i.startswith("v_mov_b32") and "dpp" not in i.split(";")[0]),
        "v_cndmask": n(lambda i: i.startswith("v_cndmask")),
        "v_cmp_lt_f32": n(lambda i: i.startswith("v_cmp_lt_f32")),
        "v_cmp_neq_f32": n(lambda i: i.startswith("v_cmp_neq_f32")),
        "v_cmp (other)": n(lambda i: i.startswith("v_cmp") and not i.startswith(("v_cmp_lt_f32", "v_cmp_neq_f32"))),
        "v_permlane swap": n(lambda i: i.startswith("v_permlane")),
        "v_readlane": n(lambda i: i.startswith(("v_readlane", "v_readfirstlane"))),
        "dpp add/min/max": n(lambda i: i.startswith(("v_add", "v_min", "v_max")) and "dpp" in i.split(";")[0]),
        "vmem": n(lambda i: i.startswith(("global_", "buffer_", "flat_", "scratch_"))),
    }


def segments(body: str):
    """Straight-line segments, cut at labels and behind uniform branches:
    [labels, instructions, branch target or None, conditional?]."""
    segs, labels, cur = [], [], []

    def close(target=None, cond=False):
        nonlocal labels, cur
        if labels or cur:
            segs.append([labels, cur, target, cond])
        labels, cur = [], []

    for raw in body.split("\n"):
        ln = raw.strip()
        m = re.match(r"^(\.LBB\d+_\d+):", ln)
        if m:
            if cur:
                close()
            labels.append(m.group(1))
            continue
        if not ln or ln.startswith((".", ";")) or ln.split(";")[0].strip().endswith(":"):
            continue
        cur.append(ln)
        if ln.startswith(UNIFORM + ("s_cbranch_execnz",)):
            tgt = ln.split(";")[0].split()
            close(tgt[1] if len(tgt) > 1 and tgt[1].startswith(".LBB") else None, ln.startswith("s_cbranch"))
    close()
    return segs


def row_paths(body: str):
    """[(run-free path, tied path)] per layout, as instruction lists."""
    segs = segments(body)
    at = {lab: k for k, s in enumerate(segs) for lab in s[0]}
    uniform_end = lambda k: bool(segs[k][1]) and segs[k][1][-1].startswith(UNIFORM)
    # s_cbranch_execnz closing a segment of an arm: exec is not empty there, so it is taken
    # (inside a piece it stays a fall-through, like s_cbranch_execz)
    taken = lambda k: bool(segs[k][1]) and segs[k][1][-1].startswith("s_cbranch_execnz") and segs[k][2] in at

    def chain(k):
        """Segments reached from k by unconditional flow (falling into a label,
        s_branch, a closing s_cbranch_execnz), up to and including the first one
        that ends in a two-way uniform branch or leaves the kernel."""
        out = []
        while k < len(segs) and k not in out and len(out) < 8:
            out.append(k)
            if taken(k):
                k = at[segs[k][2]]
            elif not uniform_end(k):                    # falls into a label
                k += 1
            elif segs[k][1][-1].startswith("s_branch") and segs[k][2] in at:
                k = at[segs[k][2]]
            else:
                break
        return out

    swaps = lambda k: sum(i.startswith("v_permlane") for i in segs[k][1])
    out = []
    # a layout starts at the piece (run of segments up to a uniform branch) that holds its first swaps
    starts, piece0 = [], 0
    nswap = 0
    for k in range(len(segs)):
        nswap += swaps(k)
        if uniform_end(k):
            if nswap >= 10:
                starts.append(piece0)
            piece0, nswap = k + 1, 0
    covered = set()
    for st in starts:
        if st in covered:
            continue
        lo, hi, k, walked = [], [], st, set()
        while k < len(segs) and k not in walked:
            covered.add(k)
            walked.add(k)
            lo += segs[k][1]; hi += segs[k][1]
            if not uniform_end(k):
                k += 1
                continue
            tgt, cond = segs[k][2], segs[k][3]
            if not cond or tgt not in at or k + 1 >= len(segs):
                break
            ca, cb = chain(at[tgt]), chain(k + 1)      # taken arm, fall-through arm
            join = next((j for j in ca if j in cb), None)
            if join is None or join in walked:
                break
            x = [i for j in ca[:ca.index(join)] for i in segs[j][1]]
            y = [i for j in cb[:cb.index(join)] for i in segs[j][1]]
            vx, vy = hist(x)["VALU"], hist(y)["VALU"]
            # the tied arm holds the tie-run scans; any other split ends the body
            if hist(x if vx > vy else y)["dpp add/min/max"] < 8:
                break
            lo += x if vx <= vy else y
            hi += y if vx <= vy else x
            covered.update(ca[:ca.index(join)] + cb[:cb.index(join)])
            k = join
        if sum(i.startswith("v_permlane") for i in hi) >= 10:
            out.append((lo, hi))
    return out


def row_loop(body: str) -> list[str]:
    """Instructions of the outermost loop that holds the permlane swaps."""
    blocks, cur = [], None
    for raw in body.split("\n"):
        if re.match(r"^(\.LBB\d+_\d+:|; %bb\.\d+:)", raw):
            cur = (raw, [])
            blocks.append(cur)
            continue
        ln = raw.strip()
        if cur is not None and ln and not ln.startswith((".", ";")):
            cur[1].append(ln)
    heads: dict[str, int] = {}
    for hdr, ins in blocks:
        m = re.search(r"Header=(BB\d+_\d+) Depth=1", hdr)
        if m:
            heads[m.group(1)] = heads.get(m.group(1), 0) + sum(i.startswith("v_permlane") for i in ins)
    if not heads:
        return []
    head = max(heads, key=heads.get)
    return [i for hdr, ins in blocks if f"Header={head} " in hdr or hdr.startswith(f".L{head}:") for i in ins]


def main() -> None:
    if sys.argv[1] == "--loop":
        text = open(sys.argv[2]).read()
        for name, body in kernel_body(text, sys.argv[3]):
            ins = row_loop(body)
            h = hist(ins)
            h["fp64"] = sum("f64" in i.split()[0] for i in ins)
            h["global_store"] = sum(i.startswith("global_store") for i in ins)
            h["ds_write"] = sum(i.startswith("ds_write") for i in ins)
            print(name)
            print("  row loop (both layouts + shared tail): " + "  ".join(f"{a}={b}" for a, b in h.items()))
        return
    if sys.argv[1] == "--paths":
        text = open(sys.argv[2]).read()
        for name, body in kernel_body(text, sys.argv[3]):
            rows = sorted(row_paths(body), key=lambda p: len(p[1]))
            print(name)
            for k, (lo, hi) in enumerate(rows):
                label = ("split" if k == 0 else "pooled") if len(rows) == 2 else f"row body {k}"
                print(f"  {label}, run-free path: " + "  ".join(f"{a}={b}" for a, b in hist(lo).items()))
                print(f"  {label}, tied path:     " + "  ".join(f"{a}={b}" for a, b in hist(hi).items()))
        return
    text = open(sys.argv[1]).read()
    sub = sys.argv[2] if len(sys.argv) > 2 else "pairwise_kernelILi2E"
    for name, body in kernel_body(text, sub):
        rows = [p for p in pieces(body) if sum(i.startswith("v_permlane") for i in p) >= 10]
        rows.sort(key=len)
        print(name)
        for k, p in enumerate(rows):
            label = "split row body" if (len(rows) == 2 and k == 0) else ("pooled row body" if len(rows) == 2 else f"row body {k}")
            print(f"  {label}: " + "  ".join(f"{a}={b}" for a, b in hist(p).items()))


if __name__ == "__main__":
    main()
