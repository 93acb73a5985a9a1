#!/usr/bin/env python3
"""Build a VARIANT of libyawhip.so for same-box A/B runs:

    python tools/build_variant.py waves8 -DSOME_FLAG=8
    python tools/build_variant.py diag1 --patch tools/experiments/band_diagnostics.patch -D<a mode of its header>=1
        ->  yet_another_wizz_amd/build/variants/libyawhip_diag1.so
    YAW_AMD_LIB=yet_another_wizz_amd/build/variants/libyawhip_diag1.so python bench.py ...

Only the kernel translation unit (build.KERNEL_UNIT, csrc/yawhip.hip: the count kernels and the functions that launch them,
nothing else -- the planner and the entry points are yawhip_count.hip's and never see a -D flag) is recompiled and linked
with the product's other objects -- unless the patch changes a file other than that unit and its yawhip_band32.inc (a
private header such as yawhip_count_kernels.h, another unit): then every unit is compiled from the patched copy, so that all
of them agree on the shared records. With --patch FILE the unit is
compiled from a patched COPY of csrc/ and include/yawhip.h under variants/src_<tag>/: neither the working tree nor the
in-tree product library is touched."""
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
if args.patch:
    src_dir = os.path.join(out_dir, f"src_{args.tag}")
    shutil.rmtree(src_dir, ignore_errors=True)
    csrc = os.path.join(src_dir, os.path.relpath(build.CSRC, ROOT))
    include = os.path.join(src_dir, os.path.relpath(build.INCLUDE, ROOT))
    shutil.copytree(build.CSRC, csrc)
    os.makedirs(include)
    shutil.copy(os.path.join(build.INCLUDE, "yawhip.h"), include)
    subprocess.check_call(["patch", "-p1", "--no-backup-if-mismatch", "-d", src_dir, "-i", os.path.abspath(args.patch)])
kernel_only = {os.path.basename(build.KERNEL_UNIT), "yawhip_band32.inc"}  # what only the kernel unit is compiled from
everything = False
if args.patch:
    with open(args.patch) as f:
        touched = {line.split()[1].split("/")[-1] for line in f if line.startswith("+++ ")}
    everything = not touched <= kernel_only
lib = os.path.join(out_dir, f"libyawhip_{args.tag}.so")
hipcc = build.hipcc_path()
objects = []
for src in build.SOURCES:
    name = os.path.basename(src)
    is_kernels = src == build.KERNEL_UNIT
    if not (is_kernels or everything):
        objects.append(os.path.join(build.OBJ_DIR, name + ".o"))  # as the regular build made it
        continue
    obj = os.path.join(out_dir, f"{os.path.splitext(name)[0]}_{args.tag}.o")
    subprocess.check_call([hipcc, *build.HIPCC_FLAGS, *(flags if is_kernels else []), f"-I{include}", f"-I{csrc}", "-c",
                           os.path.join(csrc, name), "-o", obj])
    objects.append(obj)
subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", lib, *objects])
print(lib)
