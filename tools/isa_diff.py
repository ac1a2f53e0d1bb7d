"""Compare the ISA of every kernel of a parent build's listing with the same kernel in a new listing (the device .s of
`hipcc -save-temps`): each kernel's text from its label to its .Lfunc_end, with __hip_cuid_* lines and assembler
comments dropped and the function number of local labels (.LBB<f>_<b>, .LCPI<f>_<c>: <f> counts the functions before it
in the file) removed.  Prints one
line per parent kernel (same / DIFFERENT / missing) and the kernels only the new listing has; exit status 1 if any
parent kernel changed.

    python3 tools/isa_diff.py parent-gfx950.s new-gfx950.s"""
import re
import sys


def kernels(path):
    text = open(path).read().splitlines()
    out, name, body = {}, None, []
    for line in text:
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = [re.sub(r"\.L(BB|CPI)\d+_", r".L\1_", l.split(";")[0].rstrip())
                             for l in body if "__hip_cuid_" not in l and l.split(";")[0].strip()]
                name = None
            else:
                body.append(line)
    return out


def main(a, b):
    pa, pb = kernels(a), kernels(b)
    changed = 0
    for k in sorted(pa):
        if k not in pb:
            print("missing    %s" % k)
            changed += 1
        elif pa[k] != pb[k]:
            print("DIFFERENT  %s" % k)
            changed += 1
        else:
            print("same       %s (%d lines)" % (k, len(pa[k])))
    for k in sorted(set(pb) - set(pa)):
        print("new        %s (%d lines)" % (k, len(pb[k])))
    print("%d parent kernels, %d changed" % (len(pa), changed))
    return 1 if changed else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2]))
