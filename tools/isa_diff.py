#!/usr/bin/env python3
"""Compare the gfx950 machine code of two builds kernel by kernel (no GPU needed).

A refactor that only moves kernel text between units must leave every kernel's code as it was.
For each side the device assembly of the given .hip units is produced with the Makefile's flags
(hipcc --cuda-device-only -S), cut per kernel symbol (body and .amdhsa_kernel descriptor) with the
local label numbers normalised, and pooled by kernel name whatever unit it now lives in:

    tools/isa_diff.py OLD_TREE NEW_TREE --old gpad_panel.hip ... --new gpad_panel.hip gpad_pairs.hip ...

OLD_TREE / NEW_TREE are the gpu-dualgradient-mpc_amd directories of the two checkouts.  Prints one
line per kernel of the old side -- name, lines, equal / differs / missing -- and exits non-zero
unless all are equal.  --keep DIR keeps the .s files (and reuses the ones already there).
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-Wno-unused-result",
         "-I../include", "--cuda-device-only", "-S"]
LOCAL = re.compile(r"\.L(BB|func_end|func_begin|tmp|JTI)\d+")


def assemble(tree, unit, out):
    if not os.path.exists(out):
        subprocess.run([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), *FLAGS, "-o", out,
                        os.path.join("csrc", unit)], cwd=tree, check=True)
    return out


def kernels(path):
    """{kernel symbol: normalised lines of its body and its descriptor}"""
    lines = open(path).read().splitlines()
    names = [ln.split()[1] for ln in lines if ln.strip().startswith(".amdhsa_kernel ")]
    out = {}
    for name in names:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        d0 = next(i for i in range(start, len(lines)) if lines[i].strip() == ".amdhsa_kernel " + name)
        end = next(i for i in range(d0, len(lines)) if lines[i].strip() == ".end_amdhsa_kernel")
        text = []
        for ln in lines[start:end]:  # (the descriptor follows the body, before .Lfunc_end)
            ln = LOCAL.sub(lambda m: ".L" + m.group(1), ln.split(";")[0]).strip()
            if ln:
                text.append(ln)
        out[name] = text
    return out


def side(tree, units, keep, tag):
    d = os.path.join(keep, tag)
    os.makedirs(d, exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(max_workers=8) as ex:
        files = list(ex.map(lambda u: assemble(tree, u, os.path.join(d, u.replace(".hip", ".s"))), units))
    pool = {}
    for f in files:
        for k, v in kernels(f).items():
            assert k not in pool, f"{k} defined twice"
            pool[k] = v
    return pool


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old_tree")
    ap.add_argument("new_tree")
    ap.add_argument("--old", nargs="+", required=True, help=".hip units of the old tree")
    ap.add_argument("--new", nargs="+", required=True, help=".hip units of the new tree")
    ap.add_argument("--keep", help="directory for the .s files")
    a = ap.parse_args()
    keep = a.keep or tempfile.mkdtemp(prefix="isa_diff_")
    old, new = side(a.old_tree, a.old, keep, "old"), side(a.new_tree, a.new, keep, "new")
    bad = 0
    for name in sorted(old):
        verdict = "missing" if name not in new else ("equal" if old[name] == new[name] else "differs")
        bad += verdict != "equal"
        print(f"{name} {len(old[name])} {verdict}")
    extra = sorted(set(new) - set(old))
    print(f"# {len(old)} kernels of the old side, {len(old) - bad} equal, {bad} not; "
          f"{len(extra)} only on the new side{': ' + ' '.join(extra) if extra else ''}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
