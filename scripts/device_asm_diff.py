#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two checkouts, translation unit by translation unit (host only, no GPU).

    scripts/device_asm_diff.py [--per-kernel] <checkout A> <checkout B>

The compile commands are the ones csrc/Makefile itself would run (`make -n -B`: every file of SRCS, FLAGS with the per-file
exceptions), with `-c ... -o obj` replaced by `--cuda-device-only -S`.  The only line that differs between two compilations of
the same device code is the `__hip_cuid_<hash>` symbol, a hash of the compilation: it is replaced by a fixed token.
Prints one line per file, `identical` or the number of differing lines; exits non-zero if any file differs.

A change of the host code can move the kernels inside a file (the order of instantiation) without touching an instruction.
--per-kernel compares the files that differ as a whole a second time: the assembly is cut at the function symbols, local labels
lose the function's running number (.LBB12_3 -> .LBBN_3, in the loop comments too, whose column moves with it), the kernel records of the metadata are taken one by one, and the
pieces are compared by name whatever their order.  Such a file is reported as `identical per kernel (order differs)`; a kernel
whose own lines differ is named and the run still fails.
"""
import argparse
import difflib
import re
import shlex
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor
from pathlib import Path

CUID = re.compile(r"__hip_cuid_[0-9a-f]+")


def commands(checkout, tmp):
    """{source name: argv that writes its device assembly to stdout}, run from the checkout's csrc directory"""
    csrc = Path(checkout).resolve() / "difformer_amd" / "csrc"
    dry = subprocess.run(["make", "-C", str(csrc), "-n", "-B", f"OBJDIR={tmp}/obj", f"OUT={tmp}/lib.so"],
                         check=True, capture_output=True, text=True).stdout
    out = {}
    for line in dry.splitlines():
        argv = shlex.split(line)
        if "-c" not in argv:
            continue
        c, o = argv.index("-c"), argv.index("-o")
        src = argv[c + 1]
        keep = [a for i, a in enumerate(argv) if i not in (c, c + 1, o, o + 1) and a not in ("-MMD", "-MP")]
        out[src] = (keep + ["--cuda-device-only", "-S", src, "-o", "-"], csrc)
    return out


def assembly(cmd):
    argv, cwd = cmd
    text = subprocess.run(argv, cwd=cwd, check=True, capture_output=True, text=True).stdout
    return CUID.sub("__hip_cuid_X", text).splitlines()


LOCAL_LABEL = re.compile(r"(\.L[A-Za-z_]+?|\bBB)\d+")           # .LBB12_3, .Lfunc_end12, and `BB12_3` in the loop comments
COMMENT_PAD = re.compile(r"[ \t]+;")                              # the comment column moves with the label's length
FUNCTION = re.compile(r"^\t\.type\t(\S+),@function")
LEAD_IN = re.compile(r"^\t\.(section|text|globl|protected|weak|hidden|p2align)\b")


def pieces(lines):
    """{name: lines} of one assembly file: every function from its lead-in directives to the next function's, every kernel
    record of the metadata, and what is left (the head of the file, the tail after the last function, the rest of the metadata)"""
    lines = [COMMENT_PAD.sub(" ;", LOCAL_LABEL.sub(r"\1N", x)) for x in lines]
    starts = []
    for i, x in enumerate(lines):
        m = FUNCTION.match(x)
        if m:
            j = i
            while j > 0 and LEAD_IN.match(lines[j - 1]):
                j -= 1
            starts.append((j, m.group(1)))
    tail = next((i for i, x in enumerate(lines) if x.startswith("\t.ident") or x.startswith("\t.amdgpu_metadata")), len(lines))
    if starts:
        tail = max(tail, starts[-1][0])
        # the last function ends where the sections that belong to no function begin
        for i in range(starts[-1][0], len(lines)):
            if lines[i].startswith("\t.section\t.AMDGPU.gpr_maximums") or lines[i].startswith("\t.ident") or \
                    lines[i].startswith("\t.amdgpu_metadata"):
                tail = i
                break
    out = {"<head>": lines[:starts[0][0]] if starts else lines[:tail]}
    for (a, name), nxt in zip(starts, starts[1:] + [(tail, None)]):
        out[name] = lines[a:nxt[0]]
    rest, item = [], None
    for x in lines[tail:]:
        if x.startswith("  - "):                    # a record of amdhsa.kernels (or of another top-level list)
            item = [x]
            rest.append(item)
        elif item is not None and x.startswith("    "):
            item.append(x)
        else:
            item = None
            rest.append([x])
    records = sorted(r for r in rest if r[0].startswith("  - "))
    out["<tail>"] = [x for r in rest if not r[0].startswith("  - ") for x in r] + [x for r in records for x in r]
    return out


def per_kernel(x, y):
    """-> names whose lines differ between the two files (missing on one side included)"""
    a, b = pieces(x), pieces(y)
    return sorted(n for n in set(a) | set(b) if a.get(n) != b.get(n))


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--per-kernel", action="store_true",
                    help="compare the files that differ as a whole kernel by kernel, whatever the kernels' order")
    ap.add_argument("a")
    ap.add_argument("b")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        a, b = commands(args.a, tmp), commands(args.b, tmp)
    bad = sorted(set(a) ^ set(b))
    for src in bad:
        print(f"{src}: only in {'A' if src in a else 'B'}")
    srcs = [s for s in a if s in b]
    reordered = []
    with ThreadPoolExecutor(max_workers=16) as pool:
        fa, fb = [pool.submit(assembly, a[s]) for s in srcs], [pool.submit(assembly, b[s]) for s in srcs]
        for s, x, y in zip(srcs, fa, fb):
            x, y = x.result(), y.result()
            n = sum(1 for d in difflib.unified_diff(x, y, n=0, lineterm="") if d[0] in "+-" and d[:3] not in ("+++", "---"))
            if n and args.per_kernel:
                names = per_kernel(x, y)
                reordered += [s] * (not names)
                print(f"{s}: " + (f"{len(names)} kernels differ: {' '.join(names[:8])}" if names else
                                  "identical per kernel (order differs)") + f" ({len(y)} lines)")
                bad += [s] * bool(names)
                continue
            print(f"{s}: {'identical' if n == 0 else f'{n} differing lines'} ({len(y)} lines)")
            bad += [s] * (n != 0)
    print(f"{len(srcs) - len(set(bad) & set(srcs))} of {len(srcs)} translation units identical")
    if reordered:
        print(f"needed the per-kernel comparison: {' '.join(reordered)}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
