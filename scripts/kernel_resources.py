#!/usr/bin/env python3
"""Register and scratch use of the gfx950 kernels in a compiled object, from the code object's metadata notes: VGPRs, SGPRs, scratch bytes, spilled
VGPRs per kernel.  With two objects (before, after) it pairs the kernels by demangled name -- an instantiation that gained a trailing defaulted
template argument (", 0" / ", false") pairs with its old name -- and prints the ones that differ.
    scripts/kernel_resources.py [--match attn] before.o after.o      |      scripts/kernel_resources.py [--match attn] object.o"""
import argparse
import json
import os
import re
import subprocess
import tempfile

B = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin")


def kernels(path):
    with tempfile.TemporaryDirectory() as d:
        fb, co = os.path.join(d, "fb"), os.path.join(d, "co")
        subprocess.run([os.path.join(B, "llvm-objcopy"), "--dump-section", ".hip_fatbin=" + fb, path, os.path.join(d, "o")], check=True)
        lst = subprocess.run([os.path.join(B, "clang-offload-bundler"), "--list", "--type=o", "--input=" + fb], capture_output=True, text=True).stdout
        tgt = [t for t in lst.split() if "gfx950" in t][0]
        subprocess.run([os.path.join(B, "clang-offload-bundler"), "--unbundle", "--type=o", "--input=" + fb, "--targets=" + tgt, "--output=" + co], check=True)
        txt = subprocess.run([os.path.join(B, "llvm-readelf"), "--notes", co], capture_output=True, text=True).stdout
    out = {}
    for blk in re.split(r"\n\s*- \.agpr_count:", txt)[1:]:
        g = lambda k: re.search(r"\." + k + r":\s+(\S+)", blk).group(1)
        name = subprocess.run(["c++filt", g("name")], capture_output=True, text=True).stdout.strip()
        name = re.sub(r"\((?!anonymous).*$", "", name).replace("void ", "").replace("(anonymous namespace)::", "")
        out[name] = dict(vgpr=int(g("vgpr_count")), sgpr=int(g("sgpr_count")), scratch=int(g("private_segment_fixed_size")), spills=int(g("vgpr_spill_count")))
    return out


ap = argparse.ArgumentParser()
ap.add_argument("--match", default="")
ap.add_argument("objects", nargs="+")
a = ap.parse_args()
if len(a.objects) == 1:
    print(json.dumps({k: v for k, v in sorted(kernels(a.objects[0]).items()) if a.match in k}, indent=1))
else:
    old, new = kernels(a.objects[0]), kernels(a.objects[1])
    res = dict(compared=0, identical=0, differ=[], missing=[])
    for k, v in sorted(old.items()):
        if a.match not in k:
            continue
        hit = [c for c in (k, k[:-1] + ", 0>", k[:-1] + ", false>", k + "<0>") if c in new]
        res["compared"] += 1
        if not hit:
            res["missing"].append(k)
        elif new[hit[0]] == v:
            res["identical"] += 1
        else:
            res["differ"].append(dict(kernel=k, before=v, after=new[hit[0]]))
    res["new_kernels"] = len([k for k in new if a.match in k]) - res["compared"] + len(res["missing"])
    res["new_with_scratch"] = {k: v for k, v in sorted(new.items()) if a.match in k and (v["scratch"] or v["spills"]) and
                               not any(c in old for c in (k, re.sub(r", (0|false)>$", ">", k)))}
    print(json.dumps(res, indent=1))
