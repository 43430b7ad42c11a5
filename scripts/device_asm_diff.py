#!/usr/bin/env python3
"""Compare the gfx950 device assembly of two checkouts, translation unit by translation unit (host only, no GPU).

    scripts/device_asm_diff.py <checkout A> <checkout B>

The compile commands are the ones csrc/Makefile itself would run (`make -n -B`: every file of SRCS, FLAGS with the per-file
exceptions), with `-c ... -o obj` replaced by `--cuda-device-only -S`.  The only line that differs between two compilations of
the same device code is the `__hip_cuid_<hash>` symbol, a hash of the compilation: it is replaced by a fixed token.
Prints one line per file, `identical` or the number of differing lines; exits non-zero if any file differs.
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


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("a")
    ap.add_argument("b")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        a, b = commands(args.a, tmp), commands(args.b, tmp)
    bad = sorted(set(a) ^ set(b))
    for src in bad:
        print(f"{src}: only in {'A' if src in a else 'B'}")
    srcs = [s for s in a if s in b]
    with ThreadPoolExecutor(max_workers=16) as pool:
        fa, fb = [pool.submit(assembly, a[s]) for s in srcs], [pool.submit(assembly, b[s]) for s in srcs]
        for s, x, y in zip(srcs, fa, fb):
            x, y = x.result(), y.result()
            n = sum(1 for d in difflib.unified_diff(x, y, n=0, lineterm="") if d[0] in "+-" and d[:3] not in ("+++", "---"))
            print(f"{s}: {'identical' if n == 0 else f'{n} differing lines'} ({len(y)} lines)")
            bad += [s] * (n != 0)
    print(f"{len(srcs) - len(set(bad) & set(srcs))} of {len(srcs)} translation units identical")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
