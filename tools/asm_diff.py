#!/usr/bin/env python3
"""Development aid: compare two `hipcc -S --cuda-device-only` outputs function by function.

    tools/asm_diff.py parent.s this.s [--md]

Comments and directives are dropped and local labels are renumbered in order of appearance, so two functions are SAME exactly
when their instruction streams are.  One row per kernel: SAME / DIFF / ONLY-A / ONLY-B, both instruction counts and the resource
lines (VGPRs, SGPRs, LDS bytes, scratch bytes, occupancy) of both sides.  Exit status 1 if any row is not SAME.
A function is a `_Z...` label up to the `; Occupancy` line of its resource block: unmangled (extern "C") kernels are not listed, and
a function without that line would run into the next one.
"""
import re
import subprocess
import sys

RES = ("NumVgprs", "TotalNumSgprs", "LDSByteSize", "ScratchSize", "Occupancy")


def functions(path):
    out, name, body, labels = {}, None, [], {}
    for raw in open(path):
        if name is None:
            m = re.match(r"^(_Z\w+):", raw)
            if m:
                name, body, labels, res = m.group(1), [], {}, {}
            continue
        m = re.match(r"^; (\w+): (\d+)", raw)
        if m and m.group(1) in RES:
            res[m.group(1)] = int(m.group(2))
            if m.group(1) == "Occupancy":       # the last line of a function's resource block
                out[name] = (body, res)
                name = None
            continue
        line = raw.split(";")[0].strip()
        if not line or (line.startswith(".") and not line.endswith(":")) or line.startswith(".Lfunc"):
            continue
        line = re.sub(r"\.L\w+", lambda t: labels.setdefault(t.group(0), ".L%d" % len(labels)), line)
        body.append(line)
    return out


def main():
    a, b = functions(sys.argv[1]), functions(sys.argv[2])
    names = sorted(set(a) | set(b))
    plain = subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.split("\n")
    md, bad = "--md" in sys.argv, 0
    for n, p in zip(names, plain):
        p = re.sub(r"\(.*", "", p.replace("(anonymous namespace)::", "")).replace("f3dgs::", "").replace("void ", "")
        fa, fb = a.get(n), b.get(n)
        state = "ONLY-B" if fa is None else "ONLY-A" if fb is None else "SAME" if fa[0] == fb[0] else "DIFF"
        bad += state != "SAME"
        count = lambda f: sum(not l.endswith(":") for l in f[0]) if f else "-"
        res = lambda f: "/".join(str(f[1].get(k, "?")) for k in RES) if f else "-"
        row = (p, state, count(fa), count(fb), res(fa), res(fb))
        print(("| `%s` | %s | %s | %s | %s | %s |" if md else "%-72s %-6s %6s %6s  %-22s %s") % row)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
