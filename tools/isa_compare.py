#!/usr/bin/env python3
"""Compares two ISA listings of one source file kernel by kernel (`make -C quantum_amd/csrc isa`).

    tools/isa_compare.py OLD.s NEW.s [--resources OLD_resource.txt NEW_resource.txt] [--hunks]

Each kernel's stream is what lies between its label and its .Lfunc_end, without comments, .loc/.file/.cfi
directives and the compiler's temporary labels (.Ltmp*, .Lfunc*), which carry source line numbers.  Prints a
Markdown table: kernel, instructions old and new, same or different; with --resources the SGPR / VGPR / scratch /
LDS / occupancy figures of the two -Rpass-analysis=kernel-resource-usage reports beside them; with --hunks a
unified diff of every stream that differs.  Whole streams only.  Exit status 1 when any stream differs.
"""
import argparse
import difflib
import re
import subprocess
import sys

DROP = re.compile(r"^\s*\.(loc|file|cfi_\w+)\b|^\.L(tmp|func)\w*:")
FIELDS = ("TotalSGPRs", "VGPRs", "ScratchSize [bytes/lane]", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")


def kernels(path):
    """{mangled name: [normalised lines]} in file order"""
    out, name, body = {}, None, None
    for line in open(path, errors="replace"):
        m = re.match(r"^\s*\.type\s+(\S+),@function", line)
        if m:
            name = m.group(1)
            body = out[name] = []
            continue
        if name is None:
            continue
        if line.startswith(".Lfunc_end") or line.lstrip().startswith(".section"):  # the kernel descriptor follows
            name = None
            continue
        line = re.sub(r"\s*;.*$", "", line.rstrip("\n")).rstrip()
        if not line.strip() or DROP.match(line) or line == name + ":":
            continue
        body.append(re.sub(r"\s+", " ", line.strip()))
    return out


def instructions(lines):
    return sum(1 for l in lines if not l.endswith(":") and not l.startswith("."))


def resources(path):
    out, name = {}, None
    for line in open(path):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
            out[name] = {}
            continue
        m = re.search(r":\s+([A-Za-z][^:]*): (\S+) \[-Rpass", line)
        if m and name:
            out[name][m.group(1).strip()] = m.group(2)
    return out


def demangle(names):
    try:
        r = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True)
        return dict(zip(names, r.stdout.splitlines()))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def short(name):
    name = re.sub(r"^void ", "", name)
    name = re.sub(r"\(.*$", "", name)
    return name.replace("qgcm::", "").replace("(anonymous namespace)::", "")


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--resources", nargs=2, metavar=("OLD", "NEW"))
    ap.add_argument("--hunks", action="store_true")
    a = ap.parse_args()
    ko, kn = kernels(a.old), kernels(a.new)
    ro, rn = (resources(a.resources[0]), resources(a.resources[1])) if a.resources else ({}, {})
    names = list(ko) + [n for n in kn if n not in ko]
    pretty = demangle(names)
    head = ["kernel", "instructions old", "new", "stream"]
    if a.resources:
        head += ["SGPR / VGPR / scratch / LDS / occupancy old", "new"]
    print("| " + " | ".join(head) + " |")
    print("|" + "---|" * len(head))
    differ = []
    for n in names:
        o, w = ko.get(n), kn.get(n)
        same = o == w
        if not same:
            differ.append(n)
        row = [f"`{short(pretty[n])}`", str(instructions(o)) if o is not None else "-",
               str(instructions(w)) if w is not None else "-",
               "same" if same else "only old" if w is None else "only new" if o is None else "different"]
        if a.resources:
            for r in (ro, rn):
                row.append(" / ".join(r.get(n, {}).get(f, "-") for f in FIELDS))
        print("| " + " | ".join(row) + " |")
    print(f"\n{len(names) - len(differ)} of {len(names)} streams identical.")
    if a.hunks:
        for n in differ:
            if n in ko and n in kn:
                print(f"\n### `{short(pretty[n])}`\n\n```diff")
                print("\n".join(difflib.unified_diff(ko[n], kn[n], "old", "new", lineterm="", n=4)))
                print("```")
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
