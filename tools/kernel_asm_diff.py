#!/usr/bin/env python3
"""Do two builds hold the same gfx950 kernels?  Compares device assembly function by function.

    hipcc <HIPFLAGS of the Makefile> --offload-device-only -S -o <unit>.s h263-rs_amd/csrc/<unit>.hip     (both trees)
    python tools/kernel_asm_diff.py <old.s>... -- <new.s>...

A function is the text from its symbol label to its .Lfunc_end.  The numbers of branch labels (.LBB<n>_, Lfunc_begin<n>,
Lfunc_end<n>) count the functions of the file, so they are normalised; comments and trailing blanks are dropped.  Prints
SAME or DIFF per kernel and a count; exits 1 on any DIFF and on a kernel that only one side has.  Text comparison only.
"""
import re
import sys


def functions(paths):
    found = {}
    for path in paths:
        text = open(path).read()
        for m in re.finditer(r"^\s*\.type\s+(\S+),@function\s*$", text, re.M):
            start = text.index("\n%s:" % m.group(1), m.end())
            lines = [re.sub(r"\s*;.*", "", line).rstrip() for line in text[start:text.index(".Lfunc_end", start)].splitlines()]
            body = "\n".join(line for line in lines if line)
            found[m.group(1)] = re.sub(r"(\.LBB|Lfunc_begin|Lfunc_end)\d+", r"\1N", body)
    return found


def main():
    if sys.argv.count("--") != 1:
        sys.exit(__doc__)
    cut = sys.argv.index("--")
    old, new = functions(sys.argv[1:cut]), functions(sys.argv[cut + 1:])
    verdicts = {name: "only old" if name not in new else "only new" if name not in old else
                "SAME" if old[name] == new[name] else "DIFF" for name in sorted(set(old) | set(new))}
    for name, verdict in verdicts.items():
        print("%-8s %s" % (verdict, name))
    same = sum(v == "SAME" for v in verdicts.values())
    print("%d kernels: %d SAME, %d not" % (len(verdicts), same, len(verdicts) - same))
    return 0 if verdicts and same == len(verdicts) else 1


if __name__ == "__main__":
    sys.exit(main())
