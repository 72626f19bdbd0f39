"""Is the gfx950 code of a csrc unit's kernels the same text at two commits?  One-off gate for refactors that must not touch
device code (needs the other commit's tree, so it is no test of the suite).

    python tools/isa_identity.py [--rev HEAD] [--unit stats_kernels] [--expect N] [-D MACRO ...]

Compiles pybnesian_amd/csrc/<unit>.hip of the working tree and of --rev (exported with git archive) as tests/helpers.py::unit_asm
does, splits the assembly into functions, replaces the block / temporary labels' numbers (they carry the function's ordinal in the
unit) and compares every function the working tree still has, and its .amdhsa_kernel descriptor, with the revision's.  Exit
status 0 = all equal (and --expect of them, when given).  The comment behind a block label is padded to a column, so a function whose
ordinal changes its number of digits differs by one space per label: keep the order of instantiation, or read the diff."""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import KDE_UNITS  # noqa: E402


def asm(csrc, unit, defines):
    extra = ["-fno-slp-vectorize"] if unit in KDE_UNITS else []
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, unit + ".s")
        subprocess.run(["/opt/rocm/bin/hipcc", "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", *extra, *["-D" + d for d in defines],
                        "-S", "--cuda-device-only", unit + ".hip", "-o", out], cwd=csrc, check=True, timeout=1800)
        with open(out) as f:
            return f.read()


def norm(s):
    return re.sub(r"\.Ltmp\d+", ".Ltmp", re.sub(r"BB\d+_", "BBn_", s))


def functions(text):
    """name -> (normalised body up to .Lfunc_end, normalised kernel descriptor)"""
    out = {}
    for part in re.split(r"\n(?=_Z[A-Za-z0-9_]+:)", text)[1:]:
        name = part[:part.index(":")]
        out[name] = [norm(part[:part.index(".Lfunc_end")]), None]
    for m in re.finditer(r"\.amdhsa_kernel (\S+)\n.*?\.end_amdhsa_kernel", text, re.S):
        out[m.group(1)][1] = norm(m.group(0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rev", default="HEAD")
    ap.add_argument("--unit", default="stats_kernels")
    ap.add_argument("--expect", type=int, default=None)
    ap.add_argument("-D", dest="defines", action="append", default=[])
    o = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        ar = subprocess.run(["git", "archive", o.rev, "pybnesian_amd/csrc", "include"], cwd=ROOT, check=True, capture_output=True).stdout
        subprocess.run(["tar", "-x", "-C", tmp], input=ar, check=True)
        old = functions(asm(os.path.join(tmp, "pybnesian_amd", "csrc"), o.unit, o.defines))
    new = functions(asm(os.path.join(ROOT, "pybnesian_amd", "csrc"), o.unit, o.defines))
    rev = subprocess.run(["git", "rev-parse", "--short", o.rev], cwd=ROOT, check=True, capture_output=True, text=True).stdout.strip()
    print(f"{o.unit}.hip, defines {o.defines or 'none'}: working tree against {rev}")
    print(f"functions: {len(old)} at {rev}, {len(new)} in the working tree; gone: {len(set(old) - set(new))}, new: {len(set(new) - set(old))}")
    bad = len(set(new) - set(old))
    same = 0
    for name in sorted(new):
        if name not in old:
            print(f"NEW        {name}")
            continue
        filt = shutil.which("c++filt")
        demangled = subprocess.run([filt, name], capture_output=True, text=True).stdout.strip() if filt else name
        code, desc = new[name][0] == old[name][0], new[name][1] == old[name][1] and new[name][1] is not None
        bad += not (code and desc)
        same += code and desc
        print(f"{'equal' if code else 'DIFFERS'} code, {'equal' if desc else 'DIFFERS'} descriptor  {demangled}")
    for name in sorted(set(old) - set(new)):
        print(f"gone       {name}")
    kept = len(set(new) & set(old))
    print(f"{same} of {kept} kept functions and descriptors equal")
    if o.expect is not None and kept != o.expect:
        print(f"expected {o.expect} kept functions")
        bad += 1
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
