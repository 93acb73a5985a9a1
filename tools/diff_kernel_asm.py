#!/usr/bin/env python3
"""Compare the device code of two builds function by function:

    hipcc <product flags> --cuda-device-only -S csrc/UNIT.hip -o before/UNIT.s     (every kernel unit, both trees)
    python tools/diff_kernel_asm.py before/ after/        (directories of .s files, or single files)

A kernel is keyed by its mangled name, wherever it sits: its instruction stream, its resource lines (`.set <name>.num_vgpr`
...) and every `.amdhsa_*` line of its descriptor (registers, LDS, scratch, occupancy hints) must be equal, and each side must
define it exactly once. A device function that is no kernel (kept out of line) may be defined once per unit that uses it:
every copy must equal the other side's. Only what a unit renumbers is normalised: local labels (`.LBB<n>_<m>`,
`.Lfunc_end<n>`, `.Ltmp<n>`), the `__hip_cuid_*` symbol and the order of the functions. Prints what differs, is missing or is
defined twice; exit status 1 if there is any."""
import glob
import os
import re
import sys

LOCAL = re.compile(r"\.L(BB|func_end|func_begin|tmp)\d+")
SKIP = re.compile(r"\.(p2align|type|size|globl|protected|weak|hidden|section|text)\b")


def functions(path):
    """({name: [normalised text of each definition]}, names of the kernels) over the .s files under path."""
    files = sorted(glob.glob(os.path.join(path, "*.s"))) if os.path.isdir(path) else [path]
    out, kernel_names = {}, set()
    for file in files:
        # (comments carry no code; the descriptor and the .set lines say what the summary comments say)
        lines = [ln.split(";")[0].strip() for ln in open(file).read().split("\n")]
        lines = [re.sub(r"__hip_cuid_\w+", "__hip_cuid", ln) for ln in lines if ln and not SKIP.match(ln)]
        funcs = {m.group(1) for ln in open(file) if (m := re.match(r"\s*\.type\s+(\S+),@function", ln))}
        text, name, inside = {}, None, False
        for ln in lines:
            if ln.endswith(":") and ln[:-1] in funcs:  # a function begins: code up to its .Lfunc_end label
                name, inside = ln[:-1], True
                text[name] = []
            elif inside and re.fullmatch(r"\.Lfunc_end\d+:", ln):
                inside = False
            elif inside:  # (a kernel's descriptor sits between its last instruction and that label)
                if m := re.match(r"\.amdhsa_kernel\s+(\S+)", ln):
                    kernel_names.add(m.group(1))
                text[name].append(LOCAL.sub(lambda g: ".L" + g.group(1), ln))
            elif m := re.match(r"\.set (?:\.L)?(\S+)\.\w+, ", ln):  # resources of a function, behind its code
                if m.group(1) in text:
                    text[m.group(1)].append(ln)
        for name, body in text.items():
            out.setdefault(name, []).append(body)
    return out, kernel_names


def main(before, after):
    a, a_kernels = functions(before)
    b, b_kernels = functions(after)
    bad = []
    bad += [f"only in {before}: {n}" for n in sorted(set(a) - set(b))]
    bad += [f"only in {after}: {n}" for n in sorted(set(b) - set(a))]
    bad += [f"kernel on one side only: {n}" for n in sorted(a_kernels ^ b_kernels)]
    for side, funcs, kern in ((before, a, a_kernels), (after, b, b_kernels)):
        bad += [f"kernel defined {len(funcs[n])} times in {side}: {n}" for n in sorted(kern) if len(funcs[n]) != 1]
    common = sorted(set(a) & set(b))
    for n in common:
        for x in a[n]:
            for y in b[n]:
                if x != y:
                    at = next((i for i, (p, q) in enumerate(zip(x, y)) if p != q), min(len(x), len(y)))
                    bad.append(f"differs: {n}\n   line {at} of {len(x)} / {len(y)}: {x[at:at + 1]} != {y[at:at + 1]}")
    print("\n".join(bad))
    n_kernels = len(a_kernels & b_kernels)
    print(f"{n_kernels} kernels and {len(common) - n_kernels} other device functions compared, {len(bad)} findings "
          f"({sum(len(x) for v in a.values() for x in v)} lines before, {sum(len(y) for v in b.values() for y in v)} after)")
    return 1 if bad else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(sys.argv[1], sys.argv[2]))
