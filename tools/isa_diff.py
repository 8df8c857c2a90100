#!/usr/bin/env python3
"""Compare device assembly per function: tools/isa_diff.py A.s [A2.s ...] -- B.s [B2.s ...]

Each side is a set of listings as written by `hipcc ... --cuda-device-only -S`. Every function (kernel or
device function) is keyed by its mangled symbol; its text runs from its label to its .Lfunc_end, with the
function index in local labels normalised (.LBB<n>_ -> .LBB_) and comments dropped. A kernel's
.amdhsa_kernel descriptor block (VGPRs, SGPRs, LDS, scratch) is compared separately from its instructions.
Prints the symbols that are missing, extra or different, and exits 1 on any difference. A device function
that several files of one side hold (each code object has its own copy) is accepted if the copies are equal.
Text comparison only: no instruction is looked for.
"""
import re
import sys

LABEL = re.compile(r"^([A-Za-z_$][\w$.]*):")
LBB = re.compile(r"\.LBB\d+_")


def functions(text):
    """{symbol: (body lines, descriptor lines)} of one listing"""
    out, sym, body, desc, in_desc = {}, None, [], [], False
    for raw in text.splitlines():
        line = LBB.sub(".LBB_", raw.split(";")[0].rstrip())
        if not line.strip():
            continue
        m = LABEL.match(line)
        if sym is None:
            if m and not m.group(1).startswith(".L"):
                sym, body, desc, in_desc = m.group(1), [], [], False
            continue
        if line.startswith(".Lfunc_end"):
            if body:                      # (a data label is followed by no .Lfunc_end of its own)
                out[sym] = (body, desc)
            sym = None
        elif m and not m.group(1).startswith(".L"):
            sym, body, desc, in_desc = m.group(1), [], [], False
        elif line.strip().startswith(".amdhsa_kernel"):
            in_desc = True
        elif line.strip().startswith(".end_amdhsa_kernel"):
            in_desc = False
        else:
            (desc if in_desc else body).append(line.strip())
    return out


def side(texts, name, problems):
    merged = {}
    for text in texts:
        for sym, f in functions(text).items():
            if sym in merged and merged[sym] != f:
                problems.append("%s: copies of %s differ between its files" % (name, sym))
            merged[sym] = f
    return merged


def compare(a_texts, b_texts):
    """(number of functions equal on both sides, list of problem lines)"""
    problems = []
    a, b = side(a_texts, "A", problems), side(b_texts, "B", problems)
    problems += ["missing in B: " + s for s in sorted(set(a) - set(b))]
    problems += ["extra in B: " + s for s in sorted(set(b) - set(a))]
    same = 0
    for s in sorted(set(a) & set(b)):
        what = [w for w, i in (("body", 0), ("descriptor", 1)) if a[s][i] != b[s][i]]
        if what:
            problems.append("differs (%s; body %d -> %d lines): %s" % (", ".join(what), len(a[s][0]), len(b[s][0]), s))
        else:
            same += 1
    return same, problems, sum(1 for s in a if a[s][1]), sum(1 for s in b if b[s][1])


def main(argv):
    if "--" not in argv:
        sys.exit(__doc__)
    k = argv.index("--")
    read = lambda paths: [open(p).read() for p in paths]
    same, problems, ka, kb = compare(read(argv[:k]), read(argv[k + 1:]))
    print("kernels: A %d, B %d; functions equal in body and descriptor: %d" % (ka, kb, same))
    for p in problems:
        print(p)
    return 1 if problems else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
