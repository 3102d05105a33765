"""The order of operations in a rocprofv3 --kernel-trace --memory-copy-trace output tree (csv): every kernel's name
and every copy's direction (and size, where the trace has one) by start time, runs of the same operation folded
into one line with a count.  Two builds that enqueue the same work print the same text, so `diff` of two outputs
compares their sequences (tools/copy_trace_summary.py gives the totals of the same tree).

    python3 tools/trace_sequence.py <prof_dir>
"""
import csv
import glob
import os
import sys


def rows(root, suffix):
    return [r for f in sorted(glob.glob(os.path.join(root, "**", "*" + suffix), recursive=True)) for r in csv.DictReader(open(f))]


def short(name):
    """The kernel's name without its argument list (the last parenthesis, matched from the end)."""
    if not name.endswith(")"):
        return name
    depth = 0
    for i in range(len(name) - 1, -1, -1):
        depth += (name[i] == ")") - (name[i] == "(")
        if depth == 0:
            return name[:i]
    return name


def main() -> None:
    root = sys.argv[1]
    ops = [(int(r["Start_Timestamp"]), "kernel " + short(r["Kernel_Name"])) for r in rows(root, "kernel_trace.csv")]
    for r in rows(root, "memory_copy_trace.csv"):
        size = next((r[k] for k in ("Bytes", "Size", "Copy_Bytes") if r.get(k)), "")
        ops.append((int(r["Start_Timestamp"]), f"copy {r.get('Direction') or r.get('Operation') or r.get('Kind')} {size}".rstrip()))
    ops.sort()
    last, count = None, 0
    for _, op in ops + [(0, None)]:
        if op == last:
            count += 1
            continue
        if last is not None:
            print(last if count == 1 else f"{last}  x{count}")
        last, count = op, 1


if __name__ == "__main__":
    main()
