#!/usr/bin/env python3
"""Registers, spills, scratch and static LDS of every kernel in two gfx950 assembly listings -- the fields
tools/kernel_resources.py prints, read the same way -- compared kernel by kernel and written as JSON.

    cd spline_trajectory_optimization_amd/csrc
    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S -o BEFORE.s rl_mincurv.hip     # in a checkout of the parent
    hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S -o AFTER.s rl_mincurv.hip      # in this tree
    python tools/kernel_resources_diff.py BEFORE.s AFTER.s profiles/<topic>/kernel_resources_before_after.json

Kernel names are demangled with c++filt."""
import json
import re
import subprocess
import sys


def parse(path):
    txt = open(path).read()
    meta = txt[txt.index("amdhsa.kernels:"):]
    out = {}
    for blk in re.split(r"\n  - \.agpr_count:", meta)[1:]:
        blk = ".agpr_count:" + blk
        f = dict(re.findall(r"\.(\w+):\s+([^\n]+)", blk))
        out[f["name"]] = {"vgpr": int(f["vgpr_count"]), "agpr": int(f["agpr_count"]), "sgpr": int(f["sgpr_count"]),
                          "vgpr_spill": int(f["vgpr_spill_count"]), "sgpr_spill": int(f["sgpr_spill_count"]),
                          "scratch_bytes": int(f["private_segment_fixed_size"]),
                          "static_lds_bytes": int(f["group_segment_fixed_size"])}
    names = list(out)
    dem = subprocess.run(["c++filt"] + names, capture_output=True, text=True, check=True).stdout.split("\n")
    return {d: out[n] for n, d in zip(names, dem)}


def renamed(before, after):
    """A kernel that became a template over the type of one of its parameters has another demangled name with the same body:
    `k(T, S)` -> `void k<T>(T, S)`, `void k<1>(T, S)` -> `void k<1, T>(T, S)`.  Such an instance is compared with the parent's
    kernel of the old name when that name is gone from the new listing.  Returns {old name: new name}."""
    out = {}
    for name in after:
        m = re.match(r"^void ([\w:]+)<(.*)>\((.*)\)$", name)
        if name in before or not m:
            continue
        fn, targs, params = m.group(1), [a.strip() for a in m.group(2).split(",")], m.group(3)
        if targs[-1] in ("true", "false"):
            # a pair `k<A>(P)` / `k_weighted<A>(P, w)` that became one template over a trailing flag: `k<A, false>` / `k<A, true>`
            head = f"void {fn}{'_weighted' if targs[-1] == 'true' else ''}<{', '.join(targs[:-1])}>("
            old = [b for b in before if b.startswith(head) and b not in after]
            if len(old) == 1:
                out[old[0]] = name
            continue
        first = params.split(",")[0].strip()
        if targs[-1] != first:
            continue
        old = f"{fn}({params})" if len(targs) == 1 else f"void {fn}<{', '.join(targs[:-1])}>({params})"
        if old in before and old not in after:
            out[old] = name
    return out


def main():
    before, after = parse(sys.argv[1]), parse(sys.argv[2])
    same_body = renamed(before, after)
    after = {k: v for k, v in after.items() if k not in same_body.values()} | {old: after[new] for old, new in same_body.items()}
    changed = [k for k in before if k not in after or after[k] != before[k]]
    new = [k for k in after if k not in before]
    res = {
        "what": "registers, spills, scratch and static LDS of every kernel of librl_mincurv, the parent commit against this one: "
                "the amdhsa.kernels metadata of `hipcc -O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S rl_mincurv.hip` "
                "on each tree, read and compared by tools/kernel_resources_diff.py (the fields tools/kernel_resources.py prints); "
                "the LDS of k_sweep is dynamic (static 0)",
        "flags": "-O3 -std=c++17 --offload-arch=gfx950 --cuda-device-only -S",
        "kernels_before": len(before), "kernels_after": len(after),
        "existing_kernels_unchanged": not changed, "existing_kernels_changed": changed,
        "kernels_now_templates": same_body,   # listed under their old names in "after"
        "new_kernels": new, "new_kernels_resources": {k: after[k] for k in new},
        "before": before, "after": after,
    }
    with open(sys.argv[3], "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"{len(before)} kernels before, {len(after)} after; existing kernels changed: {changed}")
    for k in new:
        print("new:", k, after[k])


if __name__ == "__main__":
    main()
