#!/usr/bin/env python3
"""isa_same.py <tree_a> <tree_b>: is the gfx950 device code of two trees the same?  CPU only.

Each of vamd_hip, vamd_feed and vamd_batcher is compiled in both trees with build_hip's flags plus
--cuda-device-only -S -cuid=0 (a fixed unit id, so the __hip_cuid_ symbol does not differ), and the assembly is compared as
text: whole files first, then -- if only the order of functions moved -- per symbol with local label numbers normalised and comments dropped.  Prints
the symbols that differ; exits non-zero unless every unit is the same.  A comparison compiles for several minutes."""
import os
import re
import shutil
import subprocess
import sys
import tempfile

UNITS = ("vamd_hip", "vamd_feed", "vamd_batcher")


def compile_asm(tree, unit, out):
    csrc = os.path.join(tree, "vorbis_amd", "csrc")
    # (the flags of __graft_entry__.build_hip)
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-fPIC", "-I" + os.path.join(tree, "include"), "-I" + csrc]
    return subprocess.Popen([shutil.which("hipcc") or "/opt/rocm/bin/hipcc"] + flags + ["--cuda-device-only", "-S", "-cuid=0", "-c", os.path.join(csrc, unit + ".hip"), "-o", out])


def symbols(text):
    """{symbol: body} of the function bodies (from `name:` to its .Lfunc_end), local labels renumbered in order of appearance;
    plus the kernel names (.amdhsa_kernel)."""
    bodies = {}
    func = re.compile(r"^([A-Za-z_][\w.$]*):[^\n]*\n(.*?)^\.Lfunc_end\d+:", re.M | re.S)
    for m in func.finditer(text):
        names = {}
        # (comments are no code, and the loop comments name basic blocks by the function's number in the file, which moves
        # when a kernel is added in front)
        body = re.sub(r"[ \t]*;[^\n]*", "", m.group(2))
        bodies[m.group(1)] = re.sub(r"\.L[A-Za-z_]*\d+(?:_\d+)?", lambda l: names.setdefault(l.group(0), ".L%d" % len(names)), body)
    # what is no function body (data, kernel descriptors, metadata) is held as a bag of lines
    bodies["(outside the functions)"] = sorted(re.sub(r"\.L[A-Za-z_]*\d+(?:_\d+)?", ".L", func.sub("", text)).split("\n"))
    return bodies, set(re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", text, re.M))


def main(a, b):
    bad = 0
    with tempfile.TemporaryDirectory() as tmp:
        jobs = [(u, t, os.path.join(tmp, "%s_%d.s" % (u, i))) for u in UNITS for i, t in enumerate((a, b))]
        procs = [compile_asm(t, u, out) for u, t, out in jobs]
        if any(p.wait() != 0 for p in procs):
            sys.exit("isa_same: hipcc failed")
        for u in UNITS:
            ta, tb = (open(os.path.join(tmp, "%s_%d.s" % (u, i))).read() for i in (0, 1))
            (sa, ka), (sb, kb) = symbols(ta), symbols(tb)
            head = "%s: %d lines, %d kernel symbols / %d lines, %d kernel symbols:" % (u, ta.count("\n"), len(ka), tb.count("\n"), len(kb))
            if ta == tb:
                print(head, "identical files")
                continue
            diff = sorted(s for s in set(sa) | set(sb) if sa.get(s) != sb.get(s)) + sorted("kernel " + k for k in ka ^ kb)
            if diff:
                bad += 1
                print(head, "%d symbols DIFFER" % len(diff))
                print("\n".join("  " + s for s in diff))
            else:
                print(head, "same per symbol (order or label numbers moved)")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
