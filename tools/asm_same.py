#!/usr/bin/env python3
"""Are the kernels two builds share the same code?  Compares, function by function, two assembly
files of one source as `make asm` writes them (uvhttp_amd/build/<name>.s), e.g. a parent
revision's and the tree's:

    python tools/asm_same.py PARENT.s THIS.s [--as OLD=NEW ...]

A function's text is everything from its label to its end marker.  Two things that move when a
kernel is added beside it are taken out before comparing: the function's ordinal in the
compiler's block labels (.LBB12_3, "Header=BB12_3") with the padding between such a label and its
comment, which follows the label's length, and the __hip_cuid lines.  Nothing else is
normalised: one different instruction, register or operand is a difference.  `--as OLD=NEW` pairs a
function that was renamed (a kernel that became a template instance), its own name replaced in its
text.  One line per function: SAME, DIFF (with the first differing lines), GONE or NEW; exit
status 1 if any shared function differs or is gone."""
import argparse
import difflib
import re
import sys


def functions(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^([A-Za-z_][\w$.]*):\s*; @", line)
        if m:
            cur = m.group(1)
            out[cur] = []
            continue
        if cur is None or "__hip_cuid" in line:
            continue
        line = re.sub(r"BB\d+_(?=\d)", "BB_", line)
        out[cur].append(re.sub(r"^(\.LBB_\d+:) +;", r"\1 ;", line))
        if line.startswith(".Lfunc_end"):
            out[cur][-1] = ".Lfunc_end\n"
            cur = None
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("parent")
    ap.add_argument("this")
    ap.add_argument("--as", dest="renamed", action="append", default=[], metavar="OLD=NEW")
    args = ap.parse_args()
    a, b = functions(args.parent), functions(args.this)
    renamed = dict(x.split("=", 1) for x in args.renamed)
    bad = 0
    for name, body in a.items():
        other = renamed.get(name, name)
        if other not in b:
            print("GONE", name)
            bad = 1
            continue
        mine = [line.replace(name, other) for line in body]
        if mine == b[other]:
            print("SAME", name + (" as " + other if other != name else ""), len(body), "lines")
        else:
            bad = 1
            print("DIFF", name)
            sys.stdout.writelines(list(difflib.unified_diff(mine, b[other], n=0))[:40])
    for name in b:
        if name not in a and name not in renamed.values():
            print("NEW ", name, len(b[name]), "lines")
    return bad


if __name__ == "__main__":
    sys.exit(main())
