#!/usr/bin/env python3
"""tools/dev/isa_same.py --parent-csrc DIR [--csrc DIR] [-j N] > profiles/<name>.txt

Proof that a change which only moves code between translation units leaves every kernel's instructions alone (no GPU needed).
Every unit of csrc/Makefile's SRC, in this tree and in the parent's csrc directory (e.g. a worktree of the parent commit), is
compiled for the device with the Makefile's flags plus --cuda-device-only -S.  Each function's text -- from its label to its
.Lfunc_end, comments dropped, local .LBB labels renumbered in order of appearance -- and each kernel's descriptor block are then
compared by mangled name.  Exit status 0 iff
  * both trees have the same set of kernels, each defined exactly once,
  * every kernel's text and descriptor are identical in both trees,
  * every other device function that appears in both trees has the same copies in both: as many, with the same texts.  (Not "one
    text wherever it appears": a function that is not inlined is register-allocated per unit, and the parent's own units differ.)"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

from resource_table import FLAGS, HERE, makefile_sources


def functions(asm):
    """{mangled name: normalised text}, {kernel name: descriptor text} of one unit's assembly"""
    funcs, kernels = {}, {}
    for m in re.finditer(r"^\.Lfunc_end\d+:\n\t\.size\t([^,\s]+),", asm, re.M):
        name = m.group(1)
        start = re.compile(r"^%s:" % re.escape(name), re.M).search(asm).start()
        labels, lines = {}, []
        for line in asm[start:m.start()].split("\n"):
            line = line.split(";")[0].rstrip()
            if line:
                lines.append(re.sub(r"\.LBB\d+_\d+", lambda l: labels.setdefault(l.group(0), ".LBB_%d" % len(labels)), line))
        funcs[name] = "\n".join(lines)
    for m in re.finditer(r"^\t\.amdhsa_kernel (\S+)\n(.*?)^\t\.end_amdhsa_kernel", asm, re.M | re.S):
        kernels[m.group(1)] = m.group(2)
    return funcs, kernels


def tree(csrc, jobs):
    def unit(src):
        with tempfile.TemporaryDirectory() as tmp:
            out = os.path.join(tmp, "unit.s")
            p = subprocess.run(["hipcc"] + FLAGS + ["--cuda-device-only", "-S", src, "-o", out], cwd=csrc, capture_output=True, text=True)
            if p.returncode != 0:
                raise RuntimeError("%s: hipcc failed\n%s" % (src, p.stderr[-2000:]))
            return (src,) + functions(open(out).read())
    with concurrent.futures.ThreadPoolExecutor(jobs) as ex:
        return list(ex.map(unit, makefile_sources(csrc)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(HERE, "..", "..", "lte-gnu-radio-code_amd", "csrc"))
    ap.add_argument("--parent-csrc", required=True)
    ap.add_argument("-j", type=int, default=8)
    a = ap.parse_args()
    new, old = tree(os.path.abspath(a.csrc), a.j), tree(os.path.abspath(a.parent_csrc), a.j)
    bad = []

    def where(units, kernel_only):           # name -> [(unit, text, descriptor or None)]
        out = {}
        for src, funcs, kernels in units:
            for name, text in funcs.items():
                if (name in kernels) == kernel_only:
                    out.setdefault(name, []).append((src, text, kernels.get(name)))
        return out
    nk, ok_ = where(new, True), where(old, True)
    for name in sorted(set(nk) ^ set(ok_)):
        bad.append("kernel only in the %s tree: %s" % ("new" if name in nk else "parent", name))
    for name in sorted(set(nk) | set(ok_)):
        for side, t in (("new", nk), ("parent", ok_)):
            if len(t.get(name, [0])) != 1:
                bad.append("kernel defined %d times in the %s tree: %s" % (len(t[name]), side, name))
    same_k = [n for n in sorted(set(nk) & set(ok_)) if nk[n][0][1:] == ok_[n][0][1:]]
    bad += ["kernel differs (%s vs parent %s): %s" % (nk[n][0][0], ok_[n][0][0], n) for n in sorted(set(nk) & set(ok_)) if n not in same_k]
    nf, of = where(new, False), where(old, False)
    both = sorted(set(nf) & set(of))
    for n in both:
        if sorted(t for _, t, _ in nf[n]) != sorted(t for _, t, _ in of[n]):
            bad.append("device function: the %d copies of the new tree are not the %d of the parent: %s" % (len(nf[n]), len(of[n]), n))
    print("# hipcc %s --cuda-device-only -S, every unit of SRC in both trees; functions compared by mangled name" % " ".join(FLAGS))
    print("units: %d new, %d parent" % (len(new), len(old)))
    print("kernels: %d new, %d parent, %d with identical text and descriptor" % (len(nk), len(ok_), len(same_k)))
    print("other device functions in both trees: %d (%d copies new, %d parent)" % (len(both), sum(len(nf[n]) for n in both), sum(len(of[n]) for n in both)))
    for src, funcs, kernels in new:
        if not any(src == s for s, _, _ in old):
            print("new unit %-20s %3d kernels, %d other device functions" % (src, len(kernels), len(funcs) - len(set(funcs) & set(kernels))))
    for line in bad:
        print("DIFF " + line)
    print("RESULT: " + ("identical" if not bad else "%d differences" % len(bad)))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
