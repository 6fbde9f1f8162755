#!/usr/bin/env python3
"""Compare the kernels of two `make asm` outputs one by one: asm_units_diff.py OLD.s NEW.s

A kernel's machine code must not depend on the translation unit it is compiled in.  For every `.amdhsa_kernel` name this takes the text
from the kernel's label to its `.Lfunc_end`, without comments and with the function's index dropped from its `.LBB<n>_` labels (the index
counts the functions of the unit), and the `.amdhsa_kernel ... .end_amdhsa_kernel` block as it stands.  The number of a `.Lpost_getpc<n>`
label is likewise counted from the kernel's first one, where the label is defined and where it is used: the compiler numbers the
long-branch expansions through the whole unit, so a kernel that has some (mcpc_steps_u_kernel) gets other numbers when other kernels
are compiled in front of it, around the same instructions.  It reports the two sets of names,
names that occur more than once, and every kernel whose text or block differs; the exit status is 0 when there is nothing to report."""
import re
import sys


def kernels(path):
    """name -> list of (text, block), one entry per occurrence in the file"""
    lines = open(path).read().splitlines()
    label = {}
    for i, ln in enumerate(lines):
        m = re.match(r"([A-Za-z_$.][\w$.]*):", ln)
        if m and not m.group(1).startswith("."):
            label.setdefault(m.group(1), []).append(i)
    out = {}
    for i, ln in enumerate(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", ln)
        if not m:
            continue
        name = m.group(1)
        end = next(j for j in range(i, len(lines)) if lines[j].strip() == ".end_amdhsa_kernel")
        block = "\n".join(x.strip() for x in lines[i:end + 1])
        start = max(s for s in label[name] if s < i)          # the kernel's code precedes its descriptor
        stop = next(j for j in range(start, len(lines)) if re.match(r"\.Lfunc_end\d+:", lines[j]))
        text, getpc = [], {}
        for x in lines[start:stop]:
            x = re.sub(r"\s*;.*$", "", x).rstrip()
            x = re.sub(r"\.LBB\d+_", ".LBB_", x)
            x = re.sub(r"\.Lpost_getpc(\d+)", lambda m: ".Lpost_getpc#%d" % getpc.setdefault(m.group(1), len(getpc)), x)
            if x:
                text.append(x)
        out.setdefault(name, []).append(("\n".join(text), block))
    return out


def main(old_path, new_path):
    old, new = kernels(old_path), kernels(new_path)
    bad = 0
    print(f"kernels: {len(old)} in {old_path}, {len(new)} in {new_path}")
    for name in sorted(set(old) - set(new)):
        print(f"MISSING in the new tree: {name}"); bad += 1
    for name in sorted(set(new) - set(old)):
        print(f"NEW in the new tree: {name}"); bad += 1
    for tag, ks in (("old", old), ("new", new)):
        for name in sorted(k for k, v in ks.items() if len(v) > 1):
            print(f"{len(ks[name])} TIMES in the {tag} tree: {name}"); bad += 1
    same = 0
    for name in sorted(set(old) & set(new)):
        (t0, b0), (t1, b1) = old[name][0], new[name][0]
        if t0 == t1 and b0 == b1:
            same += 1
        else:
            print(f"DIFFERS ({'text' if t0 != t1 else ''}{' block' if b0 != b1 else ''}): {name}"); bad += 1
    print(f"identical text and .amdhsa_kernel block: {same} of {len(set(old) & set(new))}")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
