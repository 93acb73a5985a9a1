#!/usr/bin/env python3
"""Instruction account of the PER-ITEM path of a float32 band kernel -- everything outside its walk loops: item record, lane
objects, cap bounds, band search, share-out, flush, statistics -- and the register table of a kernel family, both read from the
compiler's assembly (the sibling of tools/walk_loop_account.py, which accounts the walk loop's trip):

    hipcc <product flags> --cuda-device-only -S csrc/yawhip_kernel_band32_one.hip -o one.s
    python tools/item_path_account.py one.s 'k_count_band32_oneILi2ELi512ELb0ELi2ELb1ELb1E'
    python tools/item_path_account.py --table one.s three.s fine.s

The first form counts the instructions of the kernel by class -- vector ALU, LDS, vector memory, scalar memory, waits, nops,
scalar ALU, branches -- in three places: in front of the item loop (once per workgroup), in the item loop outside the walk
loops, and in the walk loops (whose cheapest trip walk_loop_account.py sums). The count is STATIC: every instruction of the
item loop once, the blocks of the exact path (behind a call) and of rarely taken sides included, the steps of the band search
once although up to ten run (ceil(log2 n) halvings and the last read: ten for a chunk of 257 to 511 entries). It compares two builds of one variant; it is not the number of instructions an item issues.

The second form prints, for every k_count_band32* kernel of the files, next_free_vgpr, the VGPRs allocated (granule 8),
next_free_sgpr, the SGPRs with VCC and the rest (TotalNumSgprs), scratch bytes, and the waves per SIMD the two register files
allow: min(8, floor(512 / allocated VGPRs)) and floor(800 / (ceil(sgpr / 16) * 16 + 16)) ("Registers";
the LDS limit depends on the launch and is not in the assembly)."""
import re
import sys

from walk_loop_account import blocks_of, function_lines

CLASSES = ("VALU", "LDS", "VMEM", "SMEM", "wait", "nop", "SALU", "branch", "call")


def classify(op: str) -> str:
    if op.startswith("s_waitcnt"):
        return "wait"
    if op == "s_nop":
        return "nop"
    if op.startswith("s_cbranch") or op in ("s_branch", "s_endpgm", "s_trap"):
        return "branch"
    if op in ("s_swappc_b64", "s_setpc_b64", "s_getpc_b64"):
        return "call"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "SMEM"
    if op.startswith("s_"):
        return "SALU"
    return "VMEM"  # global_*, flat_*, scratch_*, buffer_*


def account(path: str, key: str) -> None:
    body, _ = function_lines(path, key)
    blocks = blocks_of(body)
    header, parent_of = {}, {}  # loop headers with their depth; block -> header of the innermost loop it belongs to
    for lab, com, _ in blocks:
        if m := re.search(r"Loop Header: Depth=(\d+)", com):
            header[lab] = int(m.group(1))
            parent_of[lab] = lab
        elif m := re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", com):
            parent_of[lab] = ".L" + m.group(1)
    walks = set()
    for head in header:
        ins = [i for lab, _, code in blocks if parent_of.get(lab) == head for i in code]
        if any(i.startswith("ds_read") for i in ins) and any(re.match(r"v_(pk_)?fma", i) for i in ins):
            if "Inner Loop" in next(com for lab, com, _ in blocks if lab == head):
                walks.add(head)
    if not walks:
        sys.exit("no walk loop found")
    places = {p: dict.fromkeys(CLASSES, 0) for p in ("once per workgroup", "item loop outside the walk", "walk loops")}
    for lab, _, code in blocks:
        head = parent_of.get(lab)
        place = "once per workgroup" if head is None else ("walk loops" if head in walks else "item loop outside the walk")
        for i in code:
            places[place][classify(i.split()[0])] += 1
    print(key)
    for place, acc in places.items():
        print(f"  {place:28s} " + " ".join(f"{c} {acc[c]}" for c in CLASSES) + f"  = {sum(acc.values())}")


def table(paths) -> None:
    print("kernel | next_free_vgpr | allocated | next_free_sgpr | SGPRs in all | scratch | waves/SIMD by VGPRs | by SGPRs")
    print("---|---|---|---|---|---|---|---")
    for path in paths:
        name, row = None, {}
        for ln in open(path):
            if m := re.match(r"\s*\.amdhsa_kernel (\S+)", ln):
                name, row = m.group(1), {}
            elif name and (m := re.match(r"\s*\.amdhsa_(next_free_vgpr|next_free_sgpr|private_segment_fixed_size) (\d+)", ln)):
                row[m.group(1)] = int(m.group(2))
            elif name and (m := re.match(r"; TotalNumSgprs: (\d+)", ln)):
                row["total_sgpr"] = int(m.group(1))
            elif name and (m := re.match(r"; ScratchSize: (\d+)", ln)):
                if "k_count_band32" in name:
                    alloc = (row["next_free_vgpr"] + 7) // 8 * 8
                    by_v = min(8, 512 // alloc)
                    by_s = 800 // ((row["total_sgpr"] + 15) // 16 * 16 + 16)
                    short = re.sub(r"^_ZN\d+_GLOBAL__N_1\d+", "", name).split("EEvPK")[0]
                    print(f"{short} | {row['next_free_vgpr']} | {alloc} | {row['next_free_sgpr']} | {row['total_sgpr']} | "
                          f"{max(int(m.group(1)), row['private_segment_fixed_size'])} | {by_v} | {by_s}")
                name = None


if __name__ == "__main__":
    if len(sys.argv) >= 3 and sys.argv[1] == "--table":
        table(sys.argv[2:])
    elif len(sys.argv) == 3:
        account(sys.argv[1], sys.argv[2])
    else:
        sys.exit(__doc__)
