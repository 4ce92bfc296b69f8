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
