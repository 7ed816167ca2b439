#!/usr/bin/env python3
"""Do two builds of the library hold the same device kernels, compiled to the same code?

  python scripts/diff_kernel_isa.py <old device .s files> -- <new device .s files>

The .s files are what `hipcc ... --save-temps -c file.hip` leaves as file-hip-amdgcn-amd-amdhsa-gfx950.s.  Kernels are matched by
demangled name (without `(anonymous namespace)::`, as scripts/kernel_table.py prints them).  Per kernel the tool compares the
resource fields of the code object's metadata and the instruction stream, after normalising what legitimately differs between
translation units: comments and the numbers of local labels.
Prints a markdown table (profiles/lbs_split.md holds one) and exits non-zero on any difference.  Plain text comparison."""
import re
import subprocess
import sys

FIELDS = (".vgpr_count", ".sgpr_count", ".vgpr_spill_count", ".private_segment_fixed_size", ".group_segment_fixed_size")


def demangle(syms):
    out = subprocess.run(["c++filt"], input="\n".join(syms) + "\n", capture_output=True, text=True, check=True).stdout.split("\n")
    return [re.sub(r"\(anonymous namespace\)::", "", d) for d in out[:len(syms)]]


def parse(path):
    """{mangled symbol: (fields, instruction lines)} of one device assembly file"""
    lines = open(path).read().split("\n")
    kernels = {}
    for i, l in enumerate(lines):
        if l.startswith("\t.amdhsa_kernel "):
            kernels[l.split()[1]] = None
    bodies = {}
    i = 0
    while i < len(lines):
        m = re.match(r"^([A-Za-z_][\w$.]*):", lines[i])
        if m and m.group(1) in kernels:
            body = []
            i += 1
            while i < len(lines) and not lines[i].startswith(("\t.section", "\t.amdhsa_kernel", ".Lfunc_end")):
                body.append(lines[i])
                i += 1
            bodies[m.group(1)] = body
        else:
            i += 1
    meta = {}
    cur = None
    in_meta = False
    for l in lines:
        if l.startswith("amdhsa.kernels:"):
            in_meta = True
        elif in_meta and l.startswith("  - "):
            cur = {}
            l = "    " + l[4:]
        elif in_meta and l and not l.startswith(" "):
            in_meta = False
        if in_meta and cur is not None:
            m = re.match(r"^    (\.\w+):\s+(\S+)\s*$", l)
            if m:
                cur[m.group(1)] = m.group(2)
                if m.group(1) == ".name":
                    meta[m.group(2)] = cur
    res = {}
    for sym in kernels:
        res[sym] = ({f: meta[sym][f] for f in FIELDS}, bodies[sym])
    return res


def normalise(body):
    """instruction lines of a kernel body: no comments, labels renumbered in order of appearance"""
    labels = {}

    def lab(m):
        return labels.setdefault(m.group(0), ".L%d" % len(labels))
    out = []
    for l in body:
        l = l.split(";")[0].rstrip()
        if not l.strip():
            continue
        l = re.sub(r"\.L\w+", lab, l)
        out.append(l)
    return out


def instructions(norm):
    return [l for l in norm if l.startswith("\t") and not l.lstrip().startswith(".")]


def load(paths):
    ks = {}
    for p in paths:
        for sym, v in parse(p).items():
            ks[sym] = v
    syms = sorted(ks)
    return {d: ks[s] for s, d in zip(syms, demangle(syms))}


def main(argv):
    if "--" not in argv:
        print(__doc__)
        return 2
    old, new = load(argv[:argv.index("--")]), load(argv[argv.index("--") + 1:])
    bad = 0
    print("| kernel | VGPRs | SGPRs | spilled VGPRs | scratch bytes | static LDS bytes | instructions | identical |")
    print("|---|---|---|---|---|---|---|---|")
    total = [0, 0]
    for name in sorted(set(old) | set(new)):
        short = re.sub(r"\(.*", "", name).replace("void ", "")
        if name not in old or name not in new:
            print(f"| `{short}` | only in the {'old' if name in old else 'new'} build | | | | | | no |")
            bad += 1
            continue
        (fo, bo), (fn, bn) = old[name], new[name]
        no, nn = normalise(bo), normalise(bn)
        io, inn = instructions(no), instructions(nn)
        total[0] += len(io)
        total[1] += len(inn)
        same_fields = fo == fn and len(io) == len(inn)
        ndiff = sum(a != b for a, b in zip(no, nn)) + abs(len(no) - len(nn))
        cell = lambda f: fo[f] if fo[f] == fn[f] else f"{fo[f]} -> {fn[f]}"
        count = str(len(io)) if len(io) == len(inn) else f"{len(io)} -> {len(inn)}"
        verdict = "yes" if same_fields and ndiff == 0 else (f"no ({ndiff} lines differ)" if same_fields else "NO: resources differ")
        bad += verdict != "yes"
        print(f"| `{short}` | " + " | ".join(cell(f) for f in FIELDS) + f" | {count} | {verdict} |")
    print(f"\n{len(old)} kernels in the old build, {len(new)} in the new; {total[0]} and {total[1]} instruction lines; "
          f"{bad} kernel(s) differ.")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
