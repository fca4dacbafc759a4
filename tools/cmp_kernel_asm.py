#!/usr/bin/env python
"""Compares the device assembly of two builds kernel by kernel: for a change that must leave the kernels alone (host-side work).

    python tools/cmp_kernel_asm.py [--rename OLD=NEW] <old csrc/build> <new csrc/build> [file.s ...]     (default: the four depthwise sources)

The .s files are atomnas_amd.build.assemble's.  For every kernel symbol present in both builds the function body must be the same
text after two normalisations: the function's ordinal in its basic-block labels (.LBB<ordinal>_<n>, which shifts when instances
before it come or go) is dropped, and every run of blanks and tabs in the body becomes one blank (the labels' trailing comments are
padded to a column, so their padding shifts with the ordinal's width; this also hides any other change of spacing).  Prints the kernel counts per file and the symbols that
exist on one side only; exit status 1 if a common kernel differs.  --rename OLD=NEW: for kernels that lost or gained a template
parameter -- in the old build's symbols that contain OLD, OLD becomes NEW in the name and in the body (which names the symbol again)
before the two sides are matched.
"""
import os
import re
import sys


def kernels(path, rename=None):
    out, cur, body = {}, None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and cur is None:
            cur, body = m.group(1), []
        elif cur is not None:
            if line.startswith(".Lfunc_end"):
                text = re.sub(r"[ \t]+", " ", re.sub(r"BB\d+_", "BB_", "".join(body)))
                if rename and rename[0] in cur:
                    cur, text = cur.replace(*rename), text.replace(*rename)
                out[cur] = text
                cur = None
            else:
                body.append(line)
    return out


def main():
    args, rename = sys.argv[1:], None
    if args[0] == "--rename":
        rename, args = args[1].split("=", 1), args[2:]
    old, new = args[:2]
    files = args[2:] or ["dwconv.s", "dwconv_cw.s", "dwconv_mm.s", "dwconv_mm2.s"]
    bad = 0
    for f in files:
        a, b = kernels(os.path.join(old, f), rename), kernels(os.path.join(new, f))
        diff = sorted(k for k in set(a) & set(b) if a[k] != b[k])
        bad += len(diff)
        print("%-14s kernels: %d -> %d, %d in both, %d of them differ" % (f, len(a), len(b), len(set(a) & set(b)), len(diff)))
        for tag, ks in (("differs", diff), ("removed", sorted(set(a) - set(b))), ("added", sorted(set(b) - set(a)))):
            for k in ks:
                print("   %s %s" % (tag, k))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
