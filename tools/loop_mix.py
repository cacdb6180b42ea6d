#!/usr/bin/env python3
"""Static instruction mix of the panel-pair solve loops (runs without a GPU).

  python3 tools/loop_mix.py [--kernel 'gpad_panel2_kernel<13, 2, false>'] [--asm FILE] [-v]

Compiles csrc/gpad_pairs.hip to gfx950 assembly (hipcc --cuda-device-only -S; --asm reads an
assembly file made earlier instead), takes one kernel, and finds its loops: a label that a later
branch jumps back to opens a loop body, the last such branch closes it.  A solve loop is the
innermost loop that holds both MFMAs and workgroup barriers; there is one per wave role, in the
order of the role dispatch.  For each it prints the count of every mnemonic class twice:

  body : every instruction between the loop's labels (the test, results-out and verification
         blocks that the compiler laid out inside the loop included)
  iter : one plain iteration of a solve to a tolerance (two GEMMs, two epilogues with the u
         recursion, two barriers, no test): the path from the loop's head to a back branch
         through blocks that neither compute in fp64 nor store to global memory (the test does
         the first, results-out the second), with the most MFMAs, then the most packed-f32 ops
         (the u recursion's branch taken), then the fewest instructions; inner loops (spin
         waits, runtime-length GEMMs) are walked once

Classes (by mnemonic only): mfma; pk_f32 (v_pk_*_f32); f32 (other f32/f64 arithmetic, max/min,
conversions); mov (v_mov, v_accvgpr); int (integer, shift, logic and address arithmetic);
sel (v_cmp*, v_cndmask); lane (v_readlane, v_readfirstlane, v_writelane, DPP/permute moves);
then the non-VALU classes lds, vmem, salu, smem, wait (s_waitcnt, s_nop, s_barrier, ...), branch.
`valu/mfma` is (pk_f32 + f32 + mov + int + sel + lane) / mfma, the static counterpart of the
SQ_INSTS_VALU-less-MFMA ratio of tools/profile.sh.
"""
import argparse
import os
import re
import subprocess
import sys
import tempfile
from collections import Counter

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gpu-dualgradient-mpc_amd")
VALU = ("pk_f32", "f32", "mov", "int", "sel", "lane")
ORDER = ("mfma",) + VALU + ("lds", "vmem", "salu", "smem", "wait", "branch", "other")


def classify(mn: str) -> str:
    if mn.startswith("v_mfma") or mn.startswith("v_smfma"):
        return "mfma"
    if mn.startswith("v_"):
        if re.match(r"v_pk_\w+_f32", mn):
            return "pk_f32"
        if re.match(r"v_(readlane|readfirstlane|writelane|permlane|swap|mov_b32_dpp|bpermute)", mn) or mn.endswith("_dpp"):
            return "lane"
        if re.match(r"v_(mov|accvgpr)", mn):
            return "mov"
        if re.match(r"v_(cmp|cmpx|cndmask)", mn):
            return "sel"
        if re.search(r"_(f32|f64|f16)(_e32|_e64)?$", mn) or re.match(r"v_cvt", mn):
            return "f32"
        return "int"
    if mn.startswith("ds_"):
        return "lds"
    if re.match(r"(buffer|global|flat|scratch)_", mn):
        return "vmem"
    if re.match(r"s_(cbranch|branch|setpc|endpgm|call)", mn):
        return "branch"
    if re.match(r"s_(waitcnt|nop|barrier|sleep|setprio|sethalt)", mn):
        return "wait"
    if re.match(r"s_(load|buffer_load|memtime|memrealtime|dcache_inv)", mn):
        return "smem"
    if mn.startswith("s_"):
        return "salu"
    return "other"


def mangled(kernel: str) -> str:
    m = re.fullmatch(r"\s*(\w+)\s*<\s*(\d+)\s*,\s*(\d+)\s*(?:,\s*(true|false)\s*)?>\s*", kernel)
    if not m:
        return kernel  # already a symbol
    name, t, kq, drop = m.group(1), m.group(2), m.group(3), m.group(4) or "false"
    return f"_ZN4gpad{len(name)}{name}ILi{t}ELi{kq}ELb{1 if drop == 'true' else 0}EEEvNS_9SolveArgsIfEE"


def compile_asm(out: str) -> None:
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    cmd = [hipcc, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-I../include",
           "--cuda-device-only", "-S", "-o", out, "csrc/gpad_pairs.hip"]
    subprocess.run(cmd, check=True, cwd=PKG, stderr=subprocess.DEVNULL)


def kernel_lines(path: str, sym: str):
    out, on = [], False
    with open(path) as f:
        for ln in f:
            if not on:
                on = ln.startswith(sym + ":")
                continue
            if ln.startswith(".Lfunc_end"):
                break
            out.append(ln)
    if not out:
        sys.exit(f"loop_mix: no kernel {sym} in {path}")
    return out


class Block:
    __slots__ = ("label", "ins", "succ", "start")

    def __init__(self, label, start):
        self.label, self.ins, self.succ, self.start = label, [], [], start


def parse(lines):
    """Basic blocks in layout order: a label or the instruction after a branch opens one."""
    blocks = [Block(None, 0)]
    n = 0
    for ln in lines:
        s = ln.split(";")[0].strip()
        if not s or s.startswith("."):
            m = re.match(r"(\.LBB\w+):", s)
            if not m:
                continue
        m = re.match(r"(\.LBB\w+):", s)
        if m:
            if blocks[-1].ins or blocks[-1].label:
                blocks.append(Block(m.group(1), n))
            else:
                blocks[-1].label = m.group(1)
            continue
        mn = s.split()[0]
        blocks[-1].ins.append((mn, s))
        n += 1
        if classify(mn) == "branch":
            blocks.append(Block(None, n))
    index = {b.label: i for i, b in enumerate(blocks) if b.label}
    for i, b in enumerate(blocks):
        last = b.ins[-1] if b.ins else None
        tgt = None
        if last and classify(last[0]) == "branch":
            m = re.search(r"(\.LBB\w+)", last[1])
            tgt = index.get(m.group(1)) if m else None
        if last and last[0] in ("s_endpgm", "s_setpc_b64"):
            continue
        if tgt is not None:
            b.succ.append(tgt)
        if not (last and last[0] == "s_branch") and i + 1 < len(blocks):
            b.succ.append(i + 1)
    return blocks


def loops(blocks):
    """(head, tail) block ranges: head is a branch target of a block at or after it."""
    tail = {}
    for i, b in enumerate(blocks):
        for s in b.succ:
            if s <= i:
                tail[s] = max(tail.get(s, i), i)
    return sorted(tail.items())


def count(blocks, idxs) -> Counter:
    c = Counter()
    for i in idxs:
        for mn, _ in blocks[i].ins:
            c[classify(mn)] += 1
    return c


def test_block(b) -> bool:
    return any(re.search(r"_f64", mn) or re.match(r"(global|buffer|flat)_(store|atomic)", mn) for mn, _ in b.ins)


def plain_iteration(blocks, head, tail):
    def n(cls):
        return [sum(1 for mn, _ in b.ins if classify(mn) == cls) for b in blocks]

    nm, npk = n("mfma"), n("pk_f32")
    # block -> ((mfma, packed f32, -instructions), previous block)
    best = {head: ((nm[head], npk[head], -len(blocks[head].ins)), None)}
    end = None
    for i in range(head, tail + 1):
        if i not in best:
            continue
        (mf, pk, ni), _ = best[i]
        for s in blocks[i].succ:
            if s == head:
                if end is None or (mf, pk, ni) > best[end][0]:
                    end = i
            elif i < s <= tail and not test_block(blocks[s]):
                cand = (mf + nm[s], pk + npk[s], ni - len(blocks[s].ins))
                if s not in best or cand > best[s][0]:
                    best[s] = (cand, i)
    path = []
    while end is not None:
        path.append(end)
        end = best[end][1]
    return path[::-1]


def fmt(c: Counter) -> str:
    valu = sum(c[k] for k in VALU)
    r = f"{valu / c['mfma']:.3f}" if c["mfma"] else "-"
    return " ".join(f"{k}={c[k]}" for k in ORDER if c[k] or k in VALU or k == "mfma") + f" | valu/mfma={r}"


def main() -> None:
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--kernel", default="gpad_panel2_kernel<13, 2, false>")
    ap.add_argument("--asm", help="assembly file to read instead of compiling")
    ap.add_argument("-v", action="store_true", help="list the blocks of each plain iteration")
    a = ap.parse_args()
    path = a.asm
    tmp = None
    if not path:
        tmp = tempfile.NamedTemporaryFile(suffix=".s", delete=False)
        tmp.close()
        path = tmp.name
        compile_asm(path)
    try:
        lines = kernel_lines(path, mangled(a.kernel))
    finally:
        if tmp:
            os.unlink(tmp.name)
    blocks = parse(lines)
    allc = count(blocks, range(len(blocks)))
    print(f"kernel {a.kernel}: {sum(allc.values())} instructions, {len(blocks)} blocks")
    print(f"  whole kernel: {fmt(allc)}")
    lp = loops(blocks)
    # a solve loop: its plain iteration exists and carries MFMAs and both workgroup barriers
    paths = {}
    for h, t in lp:
        path = plain_iteration(blocks, h, t)
        ins = [mn for i in path for mn, _ in blocks[i].ins]
        if any(classify(mn) == "mfma" for mn in ins) and ins.count("s_barrier") >= 2:
            paths[(h, t)] = path
    sel, seen = [], set()
    for h, t in paths:
        if any((h2, t2) != (h, t) and h <= h2 and t2 <= t for h2, t2 in paths):
            continue
        # two heads one block apart can close on the same body (overlapping, not nested): once
        key = frozenset(i for i in paths[(h, t)] if any(classify(mn) == "mfma" for mn, _ in blocks[i].ins))
        if key not in seen:
            seen.add(key)
            sel.append((h, t))
    for k, (h, t) in enumerate(sel):
        body = count(blocks, range(h, t + 1))
        path = paths[(h, t)]
        it = count(blocks, path)
        print(f"loop {k} {blocks[h].label} .. block {t} ({sum(body.values())} instructions)")
        print(f"  body: {fmt(body)}")
        print(f"  iter: {fmt(it)}")
        if a.v:
            for i in path:
                print(f"    {blocks[i].label or '(fallthrough)':<14} @{blocks[i].start:<6} {fmt(count(blocks, [i]))}")


if __name__ == "__main__":
    main()
