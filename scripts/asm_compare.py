#!/usr/bin/env python3
"""Compare two `make asm` outputs of montecarlopredictivecoding_amd/csrc kernel by kernel.

    python3 scripts/asm_compare.py <parent.s> <new.s> [<parent.log> <new.log>]

For every kernel symbol (`.amdhsa_kernel`) of either file, one line:
    identical                     the same instructions in the same order
    reordered                     the same instructions (opcode and operands) in another order
    changed  N -> M               instruction counts before and after, then the difference of the opcode multisets
Comments, directives and labels are dropped; the numbers of local labels in branch operands are not compared.
With the two stderr logs of `make asm` (-Rpass-analysis=kernel-resource-usage) every difference in a kernel's remark block
(registers, spills, scratch, occupancy, LDS) is listed too.  Whole instruction streams are compared: nothing is searched for.
"""
import collections
import re
import sys


def kernels(path):
    """{symbol: [instruction, ...]} for the kernels of an AMDGPU assembly file."""
    names, bodies, cur = set(), {}, None
    for raw in open(path, errors="replace"):
        line = raw.split(";", 1)[0].strip()
        if not line:
            continue
        m = re.match(r"\.amdhsa_kernel\s+(\S+)", line)
        if m:
            names.add(m.group(1))
            continue
        m = re.match(r"\.type\s+(\S+),@function", line)
        if m:
            cur = m.group(1)
            bodies[cur] = []
            continue
        if line.startswith(".Lfunc_end"):
            cur = None
            continue
        if cur is None or line.startswith(".") or re.match(r"[\w.$]+:$", line):
            continue
        bodies[cur].append(re.sub(r"\.LBB\d+_\d+", ".LBB", " ".join(line.split())))
    return {k: v for k, v in bodies.items() if k in names}


def remarks(path):
    """{symbol: {field: value}} from the resource-usage remarks of a `make asm` log."""
    usage, name = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark: Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            usage[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z ]+?(?: \[[^\]]+\])?): (\S+) \[-Rpass", line)
        if m and name:
            usage[name][m.group(1).strip()] = m.group(2)
    return usage


def main(argv):
    if len(argv) not in (3, 5):
        sys.exit(__doc__)
    old, new = kernels(argv[1]), kernels(argv[2])
    rem = (remarks(argv[3]), remarks(argv[4])) if len(argv) == 5 else None
    tally = collections.Counter()
    for k in sorted(set(old) | set(new)):
        if k not in old or k not in new:
            verdict = "only in " + ("parent" if k in old else "new")
        elif old[k] == new[k]:
            verdict = "identical"
        elif collections.Counter(old[k]) == collections.Counter(new[k]):
            verdict = "reordered"
        else:
            a = collections.Counter(i.split()[0] for i in old[k])
            b = collections.Counter(i.split()[0] for i in new[k])
            diff = ", ".join(f"{op} {b[op] - a[op]:+d}" for op in sorted(set(a) | set(b)) if a[op] != b[op])
            verdict = f"changed  {len(old[k])} -> {len(new[k])}  opcodes: {diff or 'the same multiset (operands differ)'}"
        tally[verdict.split()[0]] += 1
        print(f"{k}\n    {verdict}")
        if rem and k in rem[0] and k in rem[1]:
            ra, rb = rem[0][k], rem[1][k]
            moved = [f"{f}: {ra.get(f)} -> {rb.get(f)}" for f in sorted(set(ra) | set(rb)) if ra.get(f) != rb.get(f)]
            print("    remarks: " + ("; ".join(moved) if moved else "identical"))
            tally["remarks " + ("differ" if moved else "identical")] += 1
    print("summary: " + ", ".join(f"{v} {k}" for k, v in sorted(tally.items())))


if __name__ == "__main__":
    main(sys.argv)
