#!/usr/bin/env python3
"""Same work enqueued?  Per case, the ordered kernel launches (name, grid and block in work-items)
and copies (direction) of each stream under two builds of the library, from the CSVs of
  rocprofv3 --kernel-trace --memory-copy-trace -f csv -d <src>/<parent|new>/<case> -- <command>
(one process per case and build).  Copies the runtime makes with its own kernels show as those
kernels, their grid following the byte count; the copy trace itself carries no byte count.
Streams are compared one by one, in the order of their first use.
  python tools/trace_cmp.py <src> <out>
writes <out>/<case>.parent.txt, <case>.new.txt and <case>.diff; exit status 1 if any differ.  Two
equal listings of more than 120 lines are written in brief: per stream the number of operations,
the SHA-256 of their ordered list and the count of each distinct operation."""
import csv
import difflib
import glob
import hashlib
import os
import sys

src, out = sys.argv[1], sys.argv[2]
os.makedirs(out, exist_ok=True)


def col(row, *names):
    for n in names:
        if n in row:
            return row[n]
    return "?"


def listing(d):
    ev = []
    for f in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            grid = "x".join(col(r, "Grid_Size_" + a, "Grid_Size") for a in "XYZ")
            blk = "x".join(col(r, "Workgroup_Size_" + a, "Workgroup_Size") for a in "XYZ")
            name = col(r, "Kernel_Name").split("(")[0]
            ev.append((col(r, "Stream_Id", "Queue_Id"), int(col(r, "Start_Timestamp")),
                       f"kernel {name} grid {grid} block {blk}"))
    for f in glob.glob(os.path.join(d, "**", "*memory_copy_trace.csv"), recursive=True):
        for r in csv.DictReader(open(f)):
            ev.append((col(r, "Stream_Id", "Queue_Id"), int(col(r, "Start_Timestamp")),
                       "copy " + col(r, "Direction")))
    streams = {}
    for s, t, what in sorted(ev, key=lambda e: (e[0], e[1])):
        streams.setdefault(s, []).append(what)
    # streams are numbered by first use, so two runs' streams line up by their content order
    lines = []
    for i, s in enumerate(sorted(streams, key=lambda s: min(t for ss, t, _ in ev if ss == s))):
        lines.append(f"# stream {i} ({len(streams[s])} operations)")
        lines += streams[s]
    return lines


def brief(lines):
    out, cur = [], []

    def close():
        if cur:
            out.append("ordered list sha256 " + hashlib.sha256("\n".join(cur).encode()).hexdigest())
            out.extend(f"{cur.count(x)} x {x}" for x in sorted(set(cur)))

    for x in lines:
        if x.startswith("#"):
            close()
            cur = []
            out.append(x)
        else:
            cur.append(x)
    close()
    return out


bad = 0
for case in sorted(os.listdir(os.path.join(src, "parent"))):
    a = listing(os.path.join(src, "parent", case))
    b = listing(os.path.join(src, "new", case))
    d = list(difflib.unified_diff(a, b, "parent", "new", lineterm=""))
    short = not d and len(a) > 120
    open(os.path.join(out, case + ".parent.txt"), "w").write("\n".join(brief(a) if short else a) + "\n")
    open(os.path.join(out, case + ".new.txt"), "w").write("\n".join(brief(b) if short else b) + "\n")
    open(os.path.join(out, case + ".diff"), "w").write("\n".join(d) + ("\n" if d else ""))
    nk = sum(1 for x in a if x.startswith("kernel"))
    nc = sum(1 for x in a if x.startswith("copy"))
    print(f"{case}: parent {nk} kernels {nc} copies; new {sum(1 for x in b if x.startswith('kernel'))} "
          f"kernels {sum(1 for x in b if x.startswith('copy'))} copies; "
          f"{'EQUAL' if not d else 'DIFFERENT (%d diff lines)' % len(d)}")
    bad += bool(d)
sys.exit(1 if bad else 0)
