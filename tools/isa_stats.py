"""Static instruction mix per kernel of a HIP source (gfx950 device assembly).

  python tools/isa_stats.py roboken-fmskf-robot-controller_amd/csrc/kernels_kf6.hip [filter] [--dump | --hash]

Compiles the source with the HIPFLAGS of the package's Makefile and counts every instruction
between a kernel's label and its .Lfunc_end (a kernel may hold several s_endpgm), grouped by
class (VALU / SALU / VMEM / LDS / branch), with the most frequent opcodes.  --dump also writes
the kernel's assembly to /tmp/<short>.s for reading.

--hash prints one JSON line per kernel instead: the demangled name, the instruction count,
the sha1 of the body (comments stripped, .LBB<n>_ labels normalised), the sha1 of its mnemonic
sequence alone (`ops`: equal where two bodies differ only in operands, such as register
numbers) and the .amdhsa_ resource values.  Two instantiations with one hash are the same code;
tools/body_compare.py compares two such listings.
"""
import collections
import hashlib
import json
import os
import re
import subprocess
import sys

MAKEFILE = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..",
                        "roboken-fmskf-robot-controller_amd", "Makefile")
AMDHSA = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size",
          "private_segment_fixed_size", "kernarg_size")


def make_var(text, name):
    return re.search(rf"^{name}\s*\??=\s*(.*)$", text, re.M).group(1).strip()


def hip_command():
    """hipcc and HIPFLAGS as the Makefile sets them (the environment overrides, as in make)."""
    text = open(MAKEFILE).read()
    var = {n: os.environ.get(n) or make_var(text, n) for n in ("HIPCC", "ARCH", "HIPFLAGS")}
    return [var["HIPCC"]] + var["HIPFLAGS"].replace("$(ARCH)", var["ARCH"]).split()


src = sys.argv[1]
args = [a for a in sys.argv[2:] if not a.startswith("--")]
flt = args[0] if args else ""
dump = "--dump" in sys.argv
asm = subprocess.run(hip_command() + ["-x", "hip", "--cuda-device-only", "-S", src, "-o", "-"],
                     capture_output=True, text=True, check=True).stdout

funcs = {}   # symbol -> instructions
bodies = {}  # symbol -> instructions and labels, normalised
meta = collections.defaultdict(dict)  # symbol -> .amdhsa_ values
cur = hsa = None
for line in asm.splitlines():
    s = line.split(";")[0].strip()
    m = re.match(r"^(_Z\S+):", s)
    if m:
        cur = m.group(1)
        funcs[cur], bodies[cur] = [], []
        continue
    if s.startswith(".amdhsa_kernel "):
        hsa = s.split()[1]
    elif s == ".end_amdhsa_kernel":
        hsa = None
    elif hsa and s.startswith(".amdhsa_") and s.split()[0][8:] in AMDHSA:
        meta[hsa][s.split()[0][8:]] = s.split()[1]
    if cur is None or not s:
        continue
    if s.startswith(".Lfunc_end"):
        cur = None
        continue
    if s.endswith(":"):
        bodies[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", s))
    elif not s.startswith((".", "//")):
        funcs[cur].append(s)
        bodies[cur].append(re.sub(r"\.LBB\d+_", ".LBB_", " ".join(s.split())))


def klass(op):
    if op.startswith(("buffer_", "global_", "flat_", "scratch_")):
        return "VMEM"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith(("s_cbranch", "s_branch")):
        return "branch"
    if op.startswith("s_waitcnt"):
        return "waitcnt"
    if op.startswith("s_"):
        return "SALU"
    if op.startswith("v_"):
        return "VALU"
    return "other"


names = list(funcs)
dems = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True).stdout.splitlines()
for name, dem in zip(names, dems):
    ins = funcs[name]
    if flt not in dem:
        continue
    if "--hash" in sys.argv:
        print(json.dumps({"name": dem, "n": len(ins),
                          "hash": hashlib.sha1("\n".join(bodies[name]).encode()).hexdigest()[:16],
                          "ops": hashlib.sha1(" ".join(i.split()[0] for i in ins).encode()).hexdigest()[:16],
                          **meta[name]}))
        continue
    ops = [i.split()[0] for i in ins]
    cls = collections.Counter(klass(o) for o in ops)
    print(f"{dem[:120]}\n  total {len(ops)}  " + "  ".join(f"{k} {v}" for k, v in cls.most_common()))
    print("  top:", ", ".join(f"{o} {c}" for o, c in collections.Counter(ops).most_common(24)))
    if dump:
        short = re.sub(r"\W+", "_", dem)[:60]
        with open(f"/tmp/{short}.s", "w") as f:
            f.write("\n".join(ins))
        print("  ->", f"/tmp/{short}.s")
