#!/usr/bin/env python
"""Two step sequences (tools/rocpd_sequence.py output, same launch list) set side by side, per kernel family: the sum of the family's
launches AND of the launch behind each of them.  rocprofv3's begin stamp of a dependent dispatch is its predecessor's end, so what a
producer's stores leave for the kernel boundary shows in its SUCCESSOR's dur_us: a change of a kernel's store policy is judged by the pair.
    tools/sequence_pairs.py PARENT_step_sequence.txt TREE_step_sequence.txt [FAMILY_SUBSTR ...]
Without family arguments every kernel name (template arguments dropped) is a family.  A launch that follows a launch of its own family is
counted once."""
import re
import sys


def load(path):
    rows = []
    for line in open(path):
        m = re.match(r"\s*(\d+) (.{70}) +(\d*) +([\d.]+) +([\d.]+) +(-?[\d.]+)\s*$", line)
        if m:
            rows.append((m.group(2).strip(), float(m.group(5))))
    return rows


def main():
    a, b = load(sys.argv[1]), load(sys.argv[2])
    if [n for n, _ in a] != [n for n, _ in b]:
        sys.exit("the two sequences are not the same launch list")
    fams = sys.argv[3:] or sorted({re.sub(r"<.*$", "", n) for n, _ in a})
    print("%-34s %8s %12s %12s %9s   %12s %12s %9s" % ("family", "launches", "own parent", "own tree", "d own", "pairs parent", "pairs tree", "d pairs"))
    for f in fams:
        own = [i for i, (n, _) in enumerate(a) if f in n]
        idx = sorted(set(own) | {i + 1 for i in own if i + 1 < len(a)})
        oa, ob = sum(a[i][1] for i in own), sum(b[i][1] for i in own)
        pa, pb = sum(a[i][1] for i in idx), sum(b[i][1] for i in idx)
        print("%-34s %8d %12.2f %12.2f %+9.2f   %12.2f %12.2f %+9.2f" % (f, len(own), oa, ob, ob - oa, pa, pb, pb - pa))
    ta, tb = sum(d for _, d in a), sum(d for _, d in b)
    print("%-34s %8d %12.2f %12.2f %+9.2f" % ("whole step (sum of dur_us)", len(a), ta, tb, tb - ta))


if __name__ == "__main__":
    main()
