#!/usr/bin/env python
"""Is the device code of a refactor the device code it started from?

    python tools/isa_compare.py BEFORE_TREE AFTER_TREE FILE.hip[:+exp] ... [--map before_name=after_name ...]

Compiles csrc/FILE.hip of both trees for the device only, with the flags build.py gives that file (":+exp" adds
-DY3_EXPERIMENTS), and compares kernel by kernel: the instruction stream (comments dropped; labels and the kernel's own symbol
renamed) and the compiler's resource report (registers, scratch, occupancy, LDS).  Kernels pair by demangled name without the
argument list; --map pairs a kernel that was renamed.  Prints one line per kernel; exit status 1 if any differs or is missing.
Needs hipcc and c++filt; no GPU.
"""
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from yolov3_tensorflow_amd import build as y3build  # noqa: E402

FIELDS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]", "SGPRs Spill", "VGPRs Spill",
          "LDS Size [bytes/block]")


def demangle(names):
    out = subprocess.run(["c++filt"] + names, stdout=subprocess.PIPE, check=True).stdout.decode().splitlines()
    short = []
    for d in out:
        d = d.replace("(anonymous namespace)::", "")
        depth, cut = 0, len(d)
        for i, ch in enumerate(d):      # the argument list starts at the first '(' outside the template brackets
            depth += ch == "<"
            depth -= ch == ">"
            if ch == "(" and depth == 0:
                cut = i
                break
        short.append(d[:cut].replace("void ", "", 1) if d.startswith("void ") else d[:cut])
    return short


def compile_kernels(tree, src, exp, tmp):
    csrc = os.path.join(tree, "yolov3_tensorflow_amd", "csrc")
    extra = dict(y3build.SOURCES)[src] + (["-DY3_EXPERIMENTS"] if exp else [])
    asm = os.path.join(tmp, "out.s")
    cmd = [y3build._hipcc()] + y3build.COMMON + extra + ["--cuda-device-only", "-S", "-Rpass-analysis=kernel-resource-usage",
                                                         os.path.join(csrc, src), "-o", asm]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
    if p.returncode != 0:
        raise SystemExit("hipcc failed on %s:\n%s" % (os.path.join(csrc, src), p.stderr.decode(errors="replace")))
    res, cur = {}, None
    for line in p.stderr.decode(errors="replace").splitlines():
        m = re.search(r"remark: .*Function Name: (\S+)", line)
        if m:
            cur = res.setdefault(m.group(1), {})
            continue
        m = re.search(r"remark: .*?\s{2,}(.+?): (\d+)\s*\[-Rpass-analysis", line)
        if m and cur is not None and m.group(1) in FIELDS:
            cur[m.group(1)] = int(m.group(2))
    text = open(asm).read()
    kernels = re.findall(r"^\s*\.amdhsa_kernel (\S+)", text, re.M)
    body = {}
    for k in kernels:
        m = re.search(r"^%s:[^\n]*\n(.*?)^\.Lfunc_end\d+:" % re.escape(k), text, re.M | re.S)
        lines, labels = [], {}
        for ln in m.group(1).splitlines():
            ln = ln.split(";")[0].strip().replace(k, "KERNEL")
            ln = re.sub(r"\.L\w+", lambda t: labels.setdefault(t.group(0), "L%d" % len(labels)), ln)
            if ln:
                lines.append(ln)
        body[k] = lines
    return dict(zip(demangle(kernels), [(body[k], res.get(k, {})) for k in kernels]))


def main():
    args = sys.argv[1:]
    renamed = {}
    if "--map" in args:
        i = args.index("--map")
        renamed = dict(a.split("=", 1) for a in args[i + 1:])
        args = args[:i]
    before, after, files = args[0], args[1], args[2:]
    bad = 0
    for spec in files:
        src, exp = (spec[:-5], True) if spec.endswith(":+exp") else (spec, False)
        with tempfile.TemporaryDirectory() as tmp:
            a = compile_kernels(before, src, exp, tmp)
            b = compile_kernels(after, src, exp, tmp)
        print("== %s%s: %d kernels before, %d after" % (src, " -DY3_EXPERIMENTS" if exp else "", len(a), len(b)))
        for name in sorted(a):
            to = renamed.get(name, name)
            if to not in b:
                print("%-110s MISSING after" % name)
                bad += 1
                continue
            (la, ra), (lb, rb) = a[name], b[to]
            same = la == lb and ra == rb
            bad += not same
            regs = " ".join("%s %s->%s" % (f.split(" [")[0].replace(" ", ""), ra.get(f), rb.get(f)) for f in FIELDS)
            print("%-110s lines %5d / %5d  identical %-3s  %s" % (name if to == name else name + "  =>  " + to, len(la), len(lb),
                                                                 "yes" if same else "NO", regs))
    print("all identical" if not bad else "%d kernels differ or are missing" % bad)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
