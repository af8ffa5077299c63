#!/usr/bin/env python
"""Do two builds of some .hip sources compile to the same kernels?  For every kernel instantiation (paired by name and template arguments, namespaces
dropped) compares VGPRs, AGPRs, SGPRs, scratch, LDS bytes, occupancy and the sequence of instruction mnemonics (operands -- kernel-argument offsets,
symbol names -- are not compared).

  python tools/isa_compare.py dump OUTDIR file.hip ...     # in the csrc directory of each tree: OUTDIR/<file>.s and OUTDIR/<file>.remarks
  python tools/isa_compare.py diff OLDDIR NEWDIR           # the table; exit status 1 if any kernel differs or is unpaired
"""
import os, re, subprocess, sys

HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -I../../include -I. -Wno-unused-value -Wno-c++20-extensions".split()      # csrc/Makefile's CXXFLAGS
FIELDS = [("VGPRs", r"VGPRs: (\d+)"), ("AGPRs", r"AGPRs: (\d+)"), ("SGPRs", r"SGPRs: (\d+)"), ("scratch", r"ScratchSize \[bytes/lane\]: (\d+)"),
          ("LDS", r"LDS Size \[bytes/block\]: (\d+)"), ("occ", r"Occupancy \[waves/SIMD\]: (\d+)")]


def dump(outdir, files):
    os.makedirs(outdir, exist_ok=True)
    for f in files:
        stem = os.path.join(outdir, os.path.splitext(os.path.basename(f))[0])
        r = subprocess.run([HIPCC, *FLAGS, "--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", f, "-o", stem + ".s"], stderr=subprocess.PIPE, text=True)
        open(stem + ".remarks", "w").write(r.stderr)
        if r.returncode:
            sys.exit(r.stderr)


def demangle(names):
    out = subprocess.run(["c++filt"], input="\n".join(names), stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
    # "void ns::kernel<64, false>(ns::Args)" -> "kernel<64, false>"
    return [re.sub(r"\w+::", "", re.sub(r"^void |\(.*\)$", "", d)) for d in out[:len(names)]]


def kernels(d):
    """{paired name: (resources, [mnemonics])} of every kernel under directory d"""
    res, seq = {}, {}
    for fn in sorted(os.listdir(d)):
        txt = open(os.path.join(d, fn)).read()
        if fn.endswith(".remarks"):
            for blk in re.split(r"remark: [^\n]*Function Name: ", txt)[1:]:
                res[blk.split()[0]] = tuple(int(re.search(p, blk).group(1)) for _, p in FIELDS)
        elif fn.endswith(".s"):
            for m in re.finditer(r"^(\w+):\s*; @\1\n(.*?)^\.Lfunc_end", txt, re.S | re.M):
                seq[m.group(1)] = [ln.split()[0] for ln in m.group(2).split("\n") if re.match(r"\s+[a-z]", ln)]
    names = sorted(n for n in seq if n in res)
    return {p: (res[n], seq[n]) for n, p in zip(names, demangle(names))}


def diff(old, new):
    a, b = kernels(old), kernels(new)
    bad = 0
    print(f"{'kernel':<58} " + " ".join(f"{n:>7}" for n, _ in FIELDS) + "  instructions")
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            print(f"{k:<58} only in {'old' if k in a else 'new'}"); bad += 1
            continue
        (ra, sa), (rb, sb) = a[k], b[k]
        first = next((i for i, (x, y) in enumerate(zip(sa, sb)) if x != y), None if len(sa) == len(sb) else min(len(sa), len(sb)))
        same = ra == rb and first is None
        bad += not same
        print(f"{k:<58} " + " ".join(f"{v:>7}" for v in ra) + f"  {len(sa):>6}  " +
              ("same" if same else "DIFFERS: new " + " ".join(str(v) for v in rb) + (f", {len(sb)} instructions, first at {first}: {sa[first:first + 1]} -> {sb[first:first + 1]}" if first is not None else "")))
    print(f"{len(set(a) | set(b))} kernels, {bad} differ")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) >= 4 and sys.argv[1] == "dump":
        dump(sys.argv[2], sys.argv[3:])
    elif len(sys.argv) == 4 and sys.argv[1] == "diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
