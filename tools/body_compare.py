"""Compare the kernel bodies of two builds from their `isa_stats.py --hash` listings.

  for f in csrc/kernels_*.hip: python tools/isa_stats.py $f --hash > DIR/$(basename $f .hip).jsonl
  python tools/body_compare.py PARENT_DIR HEAD_DIR > profiles/<name>.json

Per source file: the kernel symbols and distinct bodies on either side, the groups of head
symbols that share one body, the parent bodies no head kernel of the same base name has, the
head bodies no parent kernel of the same base name has, and the head kernels whose .amdhsa_
resource values differ from every parent kernel with the same base name and body.  Both listings
go into the output as one table (a row that is equal on both sides is written once; columns:
side, name, instructions, body hash, then the RES values).  Exit status 1
when a head body is new or a resource value differs.
"""
import collections
import glob
import json
import os
import re
import sys

RES = ("next_free_vgpr", "next_free_sgpr", "group_segment_fixed_size", "private_segment_fixed_size",
       "kernarg_size")


def base(name):
    """`void fmskf::k_kf6t<4, ...>(...)` -> `k_kf6t`"""
    return re.split(r"[<(]", name, 1)[0].split()[-1].split("::")[-1]


def load(d):
    out = {}
    for p in sorted(glob.glob(os.path.join(d, "*.jsonl"))):
        out[os.path.basename(p)[:-6]] = [json.loads(line) for line in open(p) if line.strip()]
    return out


def short(name):
    """the demangled name without `void `, `fmskf::`, the parameter list and spaces, true / false as 1 / 0"""
    n, depth = name.replace("void ", "").replace("fmskf::", ""), 0
    for i, c in enumerate(n):  # the parameter list opens at the first `(` outside the template arguments
        depth += (c == "<") - (c == ">")
        if c == "(" and depth == 0:
            n = n[:i]
            break
    return re.sub(r"\btrue\b", "1", re.sub(r"\bfalse\b", "0", n)).replace(" ", "")


parent, head = load(sys.argv[1]), load(sys.argv[2])
files, tables = {}, {}
bad = False
for f in sorted(set(parent) | set(head)):
    pk, hk = parent.get(f, []), head.get(f, [])
    pres = collections.defaultdict(set)  # (base, hash) -> resource tuples at the parent
    for k in pk:
        pres[base(k["name"]), k["hash"]].add(tuple(k.get(r) for r in RES))
    hbodies = {(base(k["name"]), k["hash"]) for k in hk}
    groups = collections.defaultdict(list)
    for k in hk:
        groups[base(k["name"]), k["hash"]].append(short(k["name"]))
    gone = collections.defaultdict(list)
    for k in pk:
        if (base(k["name"]), k["hash"]) not in hbodies:
            gone[base(k["name"]), k["hash"]].append(short(k["name"]))
    new = [short(k["name"]) for k in hk if (base(k["name"]), k["hash"]) not in pres]
    res = [short(k["name"]) for k in hk if (base(k["name"]), k["hash"]) in pres
           and tuple(k.get(r) for r in RES) not in pres[base(k["name"]), k["hash"]]]
    bad = bad or bool(new) or bool(res)
    files[f] = {
        "parent": {"kernels": len(pk), "distinct_bodies": len(pres)},
        "head": {"kernels": len(hk), "distinct_bodies": len(hbodies)},
        "head_duplicate_groups": [v for v in groups.values() if len(v) > 1],
        "parent_bodies_missing_at_head": [{"hash": h, "parent_names": v} for (b, h), v in gone.items()],
        "head_bodies_new": new,
        "head_resource_mismatch": res,
    }
    # both listings as one table: a row that is the same on both sides is written once
    row = lambda k: (short(k["name"]), k["n"], k["hash"], *(int(k[r]) for r in RES))  # noqa: E731
    prow, hrow = [row(k) for k in pk], [row(k) for k in hk]
    assert len(set(prow)) == len(prow) and len(set(hrow)) == len(hrow), "short names collide"
    tables[f] = collections.defaultdict(list)
    for r in prow:
        tables[f][base(r[0])].append(["both" if r in hrow else "parent", *r])
    for r in hrow:
        if r not in prow:
            tables[f][base(r[0])].append(["head", *r])
tot = lambda side, key: sum(v[side][key] for v in files.values())  # noqa: E731
out = {"totals": {s: {"kernels": tot(s, "kernels"), "distinct_bodies": tot(s, "distinct_bodies")}
                  for s in ("parent", "head")},
       "names": short.__doc__, "files": files, "columns": ["side", "name", "n", "hash", *RES]}
text = json.dumps(out, indent=1)[:-2] + ',\n "tables": {\n'  # the tables: one line per base kernel name
text += ",\n".join(f'  {json.dumps(f)}: {{\n' + ",\n".join(
    f"   {json.dumps(b)}: {json.dumps(rows, separators=(',', ':'))}" for b, rows in t.items()) + "\n  }"
    for f, t in tables.items())
print(text + "\n }\n}")
sys.exit(1 if bad else 0)
