"""Compare the device assembly of two builds of csrc/*.hip, file by file and kernel by kernel.

    for f in csrc/*.hip: hipcc <the Makefile's HIPFLAGS> --cuda-device-only -S $f -o DIR/$(basename $f .hip).s
    python compare_device_asm.py PARENT_DIR CHILD_DIR

A file is `identical` when it matches line for line once the .file / .ident lines are dropped and the compilation-unit id (__hip_cuid_<hash>,
which follows the path the file was compiled at) is masked.  Otherwise every kernel (its label up to
.end_amdhsa_kernel: the instructions and the kernel descriptor) is looked up by name in ANY file of the other build and compared after
comments are dropped and the per-function ordinal in local labels (.LBB<n>_k) is masked -- the only thing that changes when kernels are
emitted in another order or move to another file."""
import glob
import os
import re
import sys


def lines_of(path):
    return [re.sub(r"__hip_cuid_\w+", "__hip_cuid", l) for l in open(path) if not re.match(r"\s*\.(file|ident)\b", l)]


def kernels_of(lines):
    out = {}
    for m in re.finditer(r"^(\S+):\s*; @\1\n(.*?)^\s*\.end_amdhsa_kernel", "".join(lines), re.S | re.M):
        body = re.sub(r"\s*;.*", "", m.group(2))
        out[m.group(1)] = re.sub(r"(\.LBB|\.Lfunc_end|\.Lfunc_begin)\d+", r"\1N", body)
    return out


def main(parent, child):
    names = sorted({os.path.basename(p) for d in (parent, child) for p in glob.glob(d + "/*.s")})
    P = {n: lines_of(f"{parent}/{n}") for n in names if os.path.exists(f"{parent}/{n}")}
    C = {n: lines_of(f"{child}/{n}") for n in names if os.path.exists(f"{child}/{n}")}
    pk = {k: (n, v) for n in P for k, v in kernels_of(P[n]).items()}
    ck = {k: (n, v) for n in C for k, v in kernels_of(C[n]).items()}
    bad = 0
    for n in names:
        np_, nc = sum(f == n for f, _ in pk.values()), sum(f == n for f, _ in ck.values())
        if P.get(n) == C.get(n):
            print(f"{n}: identical ({np_} kernels)")
            continue
        mine = [k for k, (f, _) in ck.items() if f == n] + [k for k, (f, _) in pk.items() if f == n and k not in ck]
        diff = [k for k in mine if k not in pk or k not in ck or pk[k][1] != ck[k][1]]
        moved = sorted({pk[k][0] for k in mine if k in pk and k in ck and pk[k][0] != ck[k][0]})
        bad += len(diff)
        print(f"{n}: parent {np_} kernels, child {nc}; bodies that differ or are missing on one side: {len(diff)}" + (f"; kernels moved here from {moved}" if moved and nc else ""))
    print(f"kernels: parent {len(pk)}, child {len(ck)}, same names: {set(pk) == set(ck)}, differing bodies: {bad}")
    return 1 if bad or set(pk) != set(ck) else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
