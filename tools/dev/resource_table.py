#!/usr/bin/env python3
"""tools/dev/resource_table.py [--csrc DIR] [--label TEXT] [-j N] [file.hip ...] > profiles/<name>.txt

Register / spill / scratch / occupancy table of every kernel of the library, straight from the compiler (no GPU needed):
each translation unit of csrc/Makefile's SRC is compiled for the device with the Makefile's flags plus
-Rpass-analysis=kernel-resource-usage, and the figures are read from the remarks.  For the rx_demod_kernel instantiations
the generated assembly is read too: `rdlane` is the number of v_readlane_b32 inside the symbol loop (the innermost loop with
the most instructions), which is what SGPR spill reloads cost per wave and symbol -- wave_sum's own read-lanes included.

--csrc points at another checkout's csrc directory (e.g. a worktree of the parent commit) to print its table beside this one."""
import argparse
import concurrent.futures
import os
import re
import shutil
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
FLAGS = ["-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-fno-slp-vectorize", "-Wno-unused-function"]
KEYS = (("VGPRs", "vgpr"), ("AGPRs", "agpr"), ("TotalSGPRs", "sgpr"), ("VGPRs Spill", "vspill"), ("SGPRs Spill", "sspill"),
        ("ScratchSize [bytes/lane]", "scratch"), ("Occupancy [waves/SIMD]", "occ"), ("LDS Size [bytes/block]", "lds"))


def makefile_sources(csrc):
    text = open(os.path.join(csrc, "Makefile")).read().replace("\\\n", " ")
    return re.search(r"^SRC\s*=\s*(.*)$", text, re.M).group(1).split()


def demangle(names):
    tool = shutil.which("llvm-cxxfilt") or shutil.which("c++filt") or "/opt/rocm/llvm/bin/llvm-cxxfilt"
    try:
        out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(name):
    name = re.sub(r"^void ", "", name).replace("(anonymous namespace)::", "")
    name = re.sub(r"\(.*$", "", name)
    return name.replace("ofdm::", "").replace("(ofdm::DemodFlags)", "").replace("(DemodFlags)", "")


def loop_readlanes(asm, sym):
    """v_readlane_b32 count of the innermost loop with the most instructions in kernel `sym` (None if it has no inner loop).
    The blocks of a loop are taken from the compiler's own block remarks ("in Loop: Header=BBx_y Depth=d"), not from the
    layout: a loop's latch may be placed in front of its header."""
    m = re.search(r"^%s:" % re.escape(sym), asm, re.M)
    if not m:
        return None
    body = asm[m.end():]
    body = body[:body.index(".Lfunc_end")].split("\n")
    loops, cur = {}, None                     # header label -> [instructions, readlanes]
    for i, line in enumerate(body):
        blk = re.match(r"^(?:\.L(BB\d+_\d+)|; %bb\.\d+):", line)
        if blk:
            member = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", line)
            if member:
                cur = member.group(1) if int(member.group(2)) >= 2 else None
            else:                             # a header: "=>This Inner Loop Header" on this line or on the comment lines below it
                remark = line
                for nxt in body[i + 1:i + 4]:
                    if not nxt.startswith(" "):
                        break
                    remark += nxt
                cur = blk.group(1) if ("Inner Loop Header" in remark and "Depth=1" not in remark.split("Inner Loop Header")[1][:12]) else None
            continue
        if cur and line.startswith("\t") and line.strip() and not line.lstrip().startswith((";", ".")):
            ent = loops.setdefault(cur, [0, 0])
            ent[0] += 1
            ent[1] += line.split()[0].startswith("v_readlane")
    return max(loops.values())[1] if loops else None


def one_unit(csrc, src):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "unit.s")
        p = subprocess.run(["hipcc"] + FLAGS + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage", src, "-o", out],
                           cwd=csrc, capture_output=True, text=True)
        if p.returncode != 0:
            raise RuntimeError("%s: hipcc failed\n%s" % (src, p.stderr[-2000:]))
        asm = open(out).read()
    rows, cur = [], None
    for line in p.stderr.split("\n"):
        m = re.search(r"remark:\s+(.*?) \[-Rpass", line)
        if not m:
            continue
        key, _, val = m.group(1).strip().partition(":")
        key, val = key.strip(), val.strip()
        if key in ("Function Name", "Name"):
            cur = {"sym": val, "unit": src}
            rows.append(cur)
        elif cur is not None:
            for k, n in KEYS:
                if key == k:
                    cur[n] = val
    rows = [r for r in rows if re.search(r"^\s*\.amdhsa_kernel %s\s*$" % re.escape(r["sym"]), asm, re.M)]
    for r in rows:
        r["rdlane"] = loop_readlanes(asm, r["sym"]) if "rx_demod_kernel" in r["sym"] else None
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--csrc", default=os.path.join(HERE, "..", "..", "lte-gnu-radio-code_amd", "csrc"))
    ap.add_argument("--label", default="")
    ap.add_argument("-j", type=int, default=8)
    ap.add_argument("files", nargs="*")
    a = ap.parse_args()
    csrc = os.path.abspath(a.csrc)
    srcs = a.files or makefile_sources(csrc)
    with concurrent.futures.ThreadPoolExecutor(a.j) as ex:
        rows = [r for unit in ex.map(lambda s: one_unit(csrc, s), srcs) for r in unit]
    names = demangle([r["sym"] for r in rows])
    if a.label:
        print("# " + a.label)
    print("# hipcc %s -Rpass-analysis=kernel-resource-usage; rdlane = v_readlane_b32 in the symbol loop (demod kernels)" % " ".join(FLAGS))
    print("# rx_demod_kernel<N, MOD, BMODE, MINW, FLAGS, KD>: KD = 0 is the runtime-Kd kernel")
    print("%-22s %-78s %5s %5s %6s %6s %7s %4s %6s %6s" % ("unit", "kernel", "vgpr", "sgpr", "vspill", "sspill", "scratch", "occ", "lds", "rdlane"))
    for r in rows:
        print("%-22s %-78s %5s %5s %6s %6s %7s %4s %6s %6s" % (r["unit"], short(names[r["sym"]])[:78], r.get("vgpr", "?"), r.get("sgpr", "?"),
                                                             r.get("vspill", "?"), r.get("sspill", "?"), r.get("scratch", "?"), r.get("occ", "?"),
                                                             r.get("lds", "?"), "-" if r["rdlane"] is None else r["rdlane"]))
    return 0


if __name__ == "__main__":
    sys.exit(main())
