#!/usr/bin/env python3
"""Compare two sets of hipcc -Rpass-analysis=kernel-resource-usage remarks, kernel by kernel.

  hipcc ... --offload-device-only -Rpass-analysis=kernel-resource-usage -c csrc/spmv_kernels.hip -o /dev/null 2> new.txt
  tools/resource_usage_diff.py --old old1.txt [old2.txt ...] --new new1.txt [new2.txt ...]

Prints one line per kernel of the new set that the old set lacks (its registers, scratch and LDS), then the kernels both sets have whose
figures differ, then the counts.  Kernels are matched by demangled name; --trailing-default TYPE also matches a new kernel to the old one
it was before it gained a trailing template argument 0 and a trailing parameter of TYPE (a defaulted template parameter is part of the
mangled name, so such a kernel cannot keep its symbol).  Exit status 1 when a kernel of the old set is missing from the new one or differs, or when a kernel
only the new set has uses scratch.  Needs no GPU."""
import argparse
import re
import subprocess
import sys

KEYS = ["TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]"]


def parse(paths):
    out, cur = {}, None
    for p in paths:
        for line in open(p, errors="replace"):
            m = re.search(r"remark: Function Name: (\S+)", line)
            if m:
                cur = out.setdefault(m.group(1), {})
                continue
            m = re.search(r"remark:\s+([A-Za-z][^:]*): (\S+) \[-Rpass-analysis", line)
            if m and cur is not None:
                cur[m.group(1).strip()] = m.group(2)
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except Exception:
        return {n: n for n in names}


def normalise(name, ptype):
    """the name a kernel had before `, 0>` and `, ptype<...>)` were appended to its template arguments and parameters"""
    m = re.match(r"^(.*), 0>\((.*), " + re.escape(ptype) + r"(<[^()]*>)?\)$", name)
    return f"{m.group(1)}>({m.group(2)})" if m else name


def fmt(d):
    return "  ".join(f"{k.split(' [')[0]}={d.get(k, '?')}" for k in KEYS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--old", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--trailing-default", default=None, metavar="TYPE")
    a = ap.parse_args()
    old, new = parse(a.old), parse(a.new)
    dn = demangle(sorted(set(old) | set(new)))
    old = {dn[k]: v for k, v in old.items()}
    new = {dn[k]: v for k, v in new.items()}
    if a.trailing_default:
        renamed = {k: normalise(k, a.trailing_default) for k in new}
        n_ren = sum(1 for k, v in renamed.items() if k != v and v in old)
        new = {(renamed[k] if renamed[k] in old else k): v for k, v in new.items()}
        print(f"# kernels matched to their old name without the trailing `0` / {a.trailing_default} argument: {n_ren}")
    added = sorted(set(new) - set(old))
    missing = sorted(set(old) - set(new))
    names = {n: n for n in list(old) + list(new)}
    bad = 0
    print(f"# kernels only in the new build: {len(added)}")
    for n in added:
        scratch = new[n].get("ScratchSize [bytes/lane]", "?") != "0" or new[n].get("VGPRs Spill", "0") != "0"
        bad += scratch
        print(f"{'SCRATCH ' if scratch else ''}{names[n]}\n    {fmt(new[n])}")
    print(f"# kernels of the old build missing from the new one: {len(missing)}")
    for n in missing:
        bad += 1
        print(f"MISSING {names[n]}")
    same = diff = 0
    for n in sorted(set(old) & set(new)):
        if all(old[n].get(k) == new[n].get(k) for k in KEYS):
            same += 1
        else:
            diff += 1
            print(f"DIFFERS {names[n]}\n    old {fmt(old[n])}\n    new {fmt(new[n])}")
    bad += diff
    print(f"# kernels in both builds (same name): {same + diff}; identical {', '.join(k.split(' [')[0] for k in KEYS)}: {same}; differing: {diff}")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
