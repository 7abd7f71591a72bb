#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel by kernel.

    python scripts/compare_kernel_asm.py OLD_TREE NEW_TREE [-j N] [--keep DIR]

Every csrc/kernels/*.hip of both trees is compiled to device-only assembly with
the flags of the build (parsec_amd/_build.py: hipflags). Functions are matched
by mangled name, wherever they live in either tree, and two things must be
equal: the instruction sequence (comments dropped, local labels renumbered in
order of appearance, so a function's position in its file does not matter) and
the kernel's resource block (.amdhsa_kernel directives: registers, LDS,
scratch, kernarg size) plus its metadata entry (spill counts, argument list).
Prints one verdict per function and a summary; exits 1 unless all are equal
and both trees hold the same functions.
"""
import argparse
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile

ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
ARCH = os.environ.get("PYTORCH_ROCM_ARCH", "gfx950")
LABEL = re.compile(r"\.L[A-Za-z_]+\d+(?:_\d+)?")


def compile_asm(tree, src, outdir):
    out = os.path.join(outdir, os.path.basename(src) + ".s")
    cmd = [os.path.join(ROCM, "bin", "hipcc"), "-std=c++20", "-O3", "-fPIC", f"--offload-arch={ARCH}", "-D__HIP_PLATFORM_AMD__",
           f"-I{tree}/csrc", "-Wno-unused-result", "--cuda-device-only", "-S", src, "-o", out]
    subprocess.run(cmd, check=True)
    return out


def strip(line):
    return line.split(";", 1)[0].rstrip()


def renumber(lines):
    names = {}
    return [LABEL.sub(lambda m: names.setdefault(m.group(0), f".L{len(names)}"), l) for l in lines]


def parse(path):
    """{name: (code lines, resource lines)} of one assembly file."""
    text = open(path).read().splitlines()
    funcs, code, res = set(), {}, {}
    for l in text:
        m = re.match(r"\s*\.type\s+(\S+),@function", l)
        if m:
            funcs.add(m.group(1))
    cur = None
    for l in text:
        s = strip(l)
        if cur is None:
            if s.endswith(":") and s[:-1] in funcs:
                cur = s[:-1]
                code[cur] = []
            continue
        if re.match(r"\.Lfunc_end\d+:", s):
            code[cur] = renumber(code[cur])
            cur = None
        elif s.strip() and not re.match(r"\s*\.(p2align|section|text)\b", s):
            code[cur].append(s.strip())
    cur = None
    for l in text:
        s = strip(l).strip()
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", s)
        if m:
            cur = m.group(1)
            res[cur] = []
        elif s == ".end_amdhsa_kernel":
            cur = None
        elif cur is not None and s:
            res[cur].append(s)
    # metadata: the YAML list entry that names the kernel
    entry = []
    for l in text + ["  - ."]:
        if re.match(r"\s{2}- \.", l) or l.startswith("amdhsa."):
            name = next((re.match(r"\s+\.name:\s+(\S+)", e).group(1) for e in entry if re.match(r"\s+\.name:\s+_Z", e)), None)
            if name in res:
                res[name] += [e.strip() for e in entry]
            entry = []
        entry.append(l)
    return {n: (code[n], res.get(n, [])) for n in code}


def tree_functions(tree, outdir, jobs):
    srcs = sorted(glob.glob(os.path.join(tree, "csrc", "kernels", "*.hip")))
    os.makedirs(outdir, exist_ok=True)
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        outs = list(ex.map(lambda s: compile_asm(tree, s, outdir), srcs))
    found = {}
    for src, out in zip(srcs, outs):
        for name, body in parse(out).items():
            found.setdefault(name, []).append((os.path.basename(src), body))
    return found


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("-j", type=int, default=4)
    ap.add_argument("--keep", help="keep the assembly files under this directory")
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix="kernel_asm_")
    old = tree_functions(os.path.abspath(a.old), os.path.join(tmp, "old"), a.j)
    new = tree_functions(os.path.abspath(a.new), os.path.join(tmp, "new"), a.j)
    bad = 0
    for name in sorted(set(old) | set(new)):
        o, n = old.get(name, []), new.get(name, [])
        where = f"{','.join(f for f, _ in o) or '-'} -> {','.join(f for f, _ in n) or '-'}"
        if not o or not n:
            verdict = "ONLY IN " + ("OLD" if o else "NEW")
        elif len(o) != len(n):
            verdict = f"COUNT {len(o)} != {len(n)}"
        else:
            ob, nb = sorted(b for _, b in o), sorted(b for _, b in n)
            code = all(x[0] == y[0] for x, y in zip(ob, nb))
            rsrc = all(x[1] == y[1] for x, y in zip(ob, nb))
            verdict = "equal" if code and rsrc else "DIFFERS (" + " ".join(w for w, ok in (("code", code), ("resources", rsrc)) if not ok) + ")"
        bad += verdict != "equal"
        kind = "kernel" if any(b[1] for _, b in o + n) else "function"
        print(f"{verdict:<12} {kind:<8} {sum(len(b[0]) for _, b in n or o):>6} lines  {where:<44} {name}")
    print(f"\n{len(set(old) | set(new))} functions, {bad} not equal")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
