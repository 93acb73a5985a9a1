#!/usr/bin/env python3
"""Build a VARIANT of libyawhip.so for same-box A/B runs:

    python tools/build_variant.py waves8 -DSOME_FLAG=8
    python tools/build_variant.py diag1 --patch tools/experiments/band_diagnostics.patch -D<a mode of its header>=1
        ->  yet_another_wizz_amd/build/variants/libyawhip_diag1.so
    YAW_AMD_LIB=yet_another_wizz_amd/build/variants/libyawhip_diag1.so python bench.py ...

Only the kernel units (build.KERNEL_UNITS: csrc/yawhip_kernel_*.hip, one per count-kernel family, and csrc/yawhip.hip -- the
planner and the entry points are yawhip_count.hip's and never see a -D flag) are recompiled, side by side, and linked with the
product's other objects -- unless the patch changes a file other than those units and what they alone include
(build.KERNEL_HEADERS: yawhip_count_device.h, yawhip_band32.inc), i.e. a header such as yawhip_count_kernels.h or another unit:
then every unit is compiled from the patched copy, so that all of them agree on the shared records. With --patch FILE the
units are compiled from a patched COPY of csrc/ and include/yawhip.h under variants/src_<tag>/: neither the working tree nor
the in-tree product library is touched."""
import argparse
import os
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from yet_another_wizz_amd import build  # noqa: E402

ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
ap.add_argument("tag")
ap.add_argument("--patch", metavar="FILE", help="unified diff against the repository root, applied to a copy of the sources")
args, flags = ap.parse_known_args()  # everything else goes to hipcc

out_dir = os.path.join(build.OBJ_DIR, "variants")
os.makedirs(out_dir, exist_ok=True)
build.build_library()  # the objects of the other translation units come from the regular build
csrc, include = build.CSRC, build.INCLUDE
everything = False
if args.patch:
    src_dir = os.path.join(out_dir, f"src_{args.tag}")
    shutil.rmtree(src_dir, ignore_errors=True)
    csrc = os.path.join(src_dir, os.path.relpath(build.CSRC, ROOT))
    include = os.path.join(src_dir, os.path.relpath(build.INCLUDE, ROOT))
    shutil.copytree(build.CSRC, csrc)
    os.makedirs(include)
    shutil.copy(os.path.join(build.INCLUDE, "yawhip.h"), include)
    subprocess.check_call(["patch", "-p1", "--no-backup-if-mismatch", "-d", src_dir, "-i", os.path.abspath(args.patch)])
    kernel_only = {os.path.basename(p) for p in (*build.KERNEL_UNITS, *build.KERNEL_HEADERS)}
    with open(args.patch) as f:
        everything = not {line.split()[1].split("/")[-1] for line in f if line.startswith("+++ ")} <= kernel_only
todo, objects = [], []
for src in build.SOURCES:
    name, is_kernels = os.path.basename(src), src in build.KERNEL_UNITS
    obj = os.path.join(build.OBJ_DIR, name + ".o")  # as the regular build made it
    if is_kernels or everything:
        obj = os.path.join(out_dir, f"{os.path.splitext(name)[0]}_{args.tag}.o")
        todo.append((os.path.join(csrc, name), obj, flags if is_kernels else []))
    objects.append(obj)
lib = os.path.join(out_dir, f"libyawhip_{args.tag}.so")
build.compile_and_link(todo, objects, lib, csrc=csrc, include=include)
print(lib)
