#!/usr/bin/env python3
"""Instruction streams of the kernels whose name contains SUBSTRING in two gfx950 assembly listings (hipcc -save-temps ... *.s),
compared kernel by kernel as plain text: comments dropped, local labels renumbered in order of appearance.  Kernels are paired
by demangled name, with the renames of tools/kernel_resources_diff.py.  Per kernel: instruction counts; the lines a text diff
reports, split into those that differ only in the last immediate of a scalar load (a kernarg offset), those whose text stands
on both sides (the same instruction at another place), and the rest, counted by mnemonic on each side (equal counts on both
sides: the same operations on other registers); and the mnemonics whose count in the whole kernel changed.

    python tools/isa_diff.py BEFORE.s AFTER.s SUBSTRING OUT.json"""
import collections
import difflib
import json
import re
import subprocess
import sys

from kernel_resources_diff import parse, renamed


def streams(path):
    """{demangled kernel name: [instruction and label lines]}"""
    txt = open(path).read()
    out = {}
    for m in re.finditer(r"^(\w+):\s*(?:;[^\n]*)?\n(.*?)^\.Lfunc_end\d+:", txt, re.S | re.M):
        lines = [ln.split(";")[0].strip() for ln in m.group(2).split("\n")]
        lines = [ln for ln in lines if ln and (not ln.startswith(".") or re.match(r"\.LBB\d+_\d+:", ln))]
        labels = {}
        for lab in re.findall(r"\.LBB\d+_\d+", "\n".join(lines)):
            labels.setdefault(lab, f".L{len(labels)}")
        out[m.group(1)] = [re.sub(r"\.LBB\d+_\d+", lambda x: labels[x.group(0)], ln) for ln in lines]
    names = list(out)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    return {d: out[n] for n, d in zip(names, dem)}


def compare(a, b):
    offsets, gone, come = 0, collections.Counter(), collections.Counter()
    for tag, i0, i1, j0, j1 in difflib.SequenceMatcher(None, a, b, autojunk=False).get_opcodes():
        if tag == "equal":
            continue
        x, y = a[i0:i1], b[j0:j1]
        if len(x) == len(y) and all(p.startswith("s_load") and p.rsplit(",", 1)[0] == q.rsplit(",", 1)[0] for p, q in zip(x, y)):
            offsets += len(x)
        else:
            gone.update(x); come.update(y)
    moved = gone & come
    mnemonics = lambda c: dict(sorted(collections.Counter(ln.split()[0] for ln in c.elements()).items()))  # noqa: E731
    count = lambda s: sum(not ln.endswith(":") for ln in s)   # noqa: E731  (labels are compared, not counted)
    ma, mb = (collections.Counter(ln.split()[0] for ln in s if not ln.endswith(":")) for s in (a, b))
    return {"instructions_before": count(a), "instructions_after": count(b),
            "mnemonics_whose_count_changed": {m: [ma[m], mb[m]] for m in sorted(set(ma) | set(mb)) if ma[m] != mb[m]},
            "lines_differing_in_a_scalar_load_offset_only": offsets,
            "lines_at_another_place": sum(moved.values()),
            "lines_only_before": sum((gone - moved).values()), "lines_only_after": sum((come - moved).values()),
            "only_before_by_mnemonic": mnemonics(gone - moved), "only_after_by_mnemonic": mnemonics(come - moved)}


def main():
    before_s, after_s, sub, out_path = sys.argv[1:5]
    before, after = streams(before_s), streams(after_s)
    new_of = renamed(parse(before_s), parse(after_s))
    res = {}
    for old in sorted(k for k in before if sub in k):
        new = new_of.get(old, old)
        r = res[old] = {"now": new} | compare(before[old], after[new])
        print(f"{new[:72]:72s} {r['instructions_before']:6d} -> {r['instructions_after']:6d}  offset only "
              f"{r['lines_differing_in_a_scalar_load_offset_only']}  moved {r['lines_at_another_place']}  "
              f"only before {r['only_before_by_mnemonic']}  only after {r['only_after_by_mnemonic']}")
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
