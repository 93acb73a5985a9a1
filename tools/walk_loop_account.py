#!/usr/bin/env python3
"""Instruction account of the walk loop of a float32 band kernel, read from the compiler's assembly:

    hipcc <product flags> --cuda-device-only -S csrc/yawhip_kernel_band32_one.hip -o one.s
    python tools/walk_loop_account.py one.s 'k_count_band32_oneILi2ELi512ELb0ELi2ELb1ELb1E' [--print]

The walk loop is the innermost loop of the kernel that holds a packed (or, one object per lane, scalar) float32 fma and LDS
reads (a kernel with three chunks per round has three). Its blocks are listed with their instructions by class -- VALU /
LDS / wait / nop / SALU / branch / call / other (global memory: the exact path) -- and the trip every entry takes is summed:
the cheapest way from the loop's header back to it, each block counted up to the branch that leaves it, with the number of
taken branches on the way. Below that the kernel's resources: VGPRs, scratch, occupancy. The vector instructions bound the
loop and every other instruction takes an issue turn of the wave (DESIGN.md sections 4 and 8): both numbers count."""
import re
import sys

CLASSES = ("VALU", "LDS", "wait", "nop", "SALU", "branch", "call", "other")


def classify(op: str) -> str:
    if op.startswith("s_waitcnt"):
        return "wait"
    if op == "s_nop":
        return "nop"
    if op.startswith("s_cbranch") or op == "s_branch":
        return "branch"
    if op in ("s_swappc_b64", "s_setpc_b64", "s_getpc_b64"):
        return "call"
    if op.startswith("ds_"):
        return "LDS"
    if op.startswith("v_"):
        return "VALU"
    if op.startswith("s_load") or op.startswith("s_buffer_load"):
        return "other"
    if op.startswith("s_"):
        return "SALU"
    return "other"  # global_*, flat_*, scratch_*, buffer_*


def function_lines(path: str, key: str):
    lines = open(path).read().split("\n")
    start = next(i for i, ln in enumerate(lines) if re.match(r"^_Z\S*" + re.escape(key) + r"\S*:", ln))
    end = next(i for i in range(start, len(lines)) if re.match(r"^\.Lfunc_end\d+:", lines[i]))
    return lines[start:end], lines[end:end + 400]


def blocks_of(body):
    """[(label, comment, [instruction lines])] of a function, the entry block first."""
    out = [["entry", "", []]]
    for ln in body[1:]:
        m = re.match(r"^(\.LBB\d+_\d+|; %bb\.\d+):\s*(;.*)?$", ln)
        if m:
            out.append([m.group(1).lstrip("; "), m.group(2) or "", []])
        elif re.match(r"^\s+;", ln) and not out[-1][2]:  # a loop header's comment runs over several lines
            out[-1][1] += " " + ln.strip()
        elif ln.startswith("\t") and not ln.startswith("\t.") and not ln.startswith("\t;"):
            out[-1][2].append(ln.split(";")[0].strip())
    return out


def main(path, key, show):
    body, tail = function_lines(path, key)
    blocks = blocks_of(body)
    # loop headers and their depth; a block belongs to the loop named in its comment
    depth = {lab: int(m.group(1)) for lab, com, _ in blocks if (m := re.search(r"Loop Header: Depth=(\d+)", com))}
    member = {}
    for lab, com, _ in blocks:
        if lab in depth:
            member[lab] = lab
        elif m := re.search(r"in Loop: Header=(BB\d+_\d+) Depth=(\d+)", com):
            member[lab] = ".L" + m.group(1)
    walks = []
    for head in depth:
        ins = [i for lab, _, code in blocks if member.get(lab) == head for i in code]
        if any(i.startswith("ds_read") for i in ins) and any(re.match(r"v_(pk_)?fma(c|_)?_?f32", i) or i.startswith("v_pk_fma_f32") for i in ins):
            if "Inner Loop" in next(com for lab, com, _ in blocks if lab == head):
                walks.append(head)
    if not walks:
        sys.exit("no walk loop found")
    order = [lab for lab, _, _ in blocks]
    code_of = {lab: code for lab, _, code in blocks}
    for head in walks:
        print(f"walk loop {head} (depth {depth[head]})")
        for lab, _, code in blocks:
            if member.get(lab) != head:
                continue
            acc = dict.fromkeys(CLASSES, 0)
            for i in code:
                acc[classify(i.split()[0])] += 1
            print(f"  {lab:12s} " + " ".join(f"{c} {acc[c]}" for c in CLASSES if acc[c]) + f"  = {sum(acc.values())}")
            if show:
                print("\n".join("      " + i for i in code))
        # the trip every entry takes: the cheapest way from the header back to it (the exact path is never on it)
        best = {head: (0, [])}  # block -> (instructions before it, [(block, instructions of it issued, left by a taken branch)])
        todo, trip = [head], None
        while todo:
            lab = todo.pop(0)
            before, way = best[lab]
            code = code_of[lab]
            nxt = [(i.split()[1], k + 1, True) for k, i in enumerate(code) if i.startswith("s_cbranch") or i.startswith("s_branch")]
            if not (code and code[-1].startswith("s_branch")) and order.index(lab) + 1 < len(order):
                nxt.append((order[order.index(lab) + 1], len(code), False))
            for to, issued, taken in nxt:
                cost = before + issued
                if to == head:
                    if trip is None or cost < trip[0]:
                        trip = (cost, way + [(lab, issued, taken)])
                elif member.get(to) == head and (to not in best or cost < best[to][0]):
                    best[to] = (cost, way + [(lab, issued, taken)])
                    todo.append(to)
        acc = dict.fromkeys(CLASSES, 0)
        path = [lab for lab, _, _ in trip[1]]
        for lab, issued, _ in trip[1]:
            for i in code_of[lab][:issued]:
                acc[classify(i.split()[0])] += 1
        print("  per trip (" + " -> ".join(path) + "): " + " ".join(f"{c} {acc[c]}" for c in CLASSES if acc[c])
              + f"  = {sum(acc.values())}, taken branches {sum(t for _, _, t in trip[1])}")
    for ln in tail:
        if re.search(r"; (NumVgprs|NumAgprs|ScratchSize|Occupancy|SGPRBlocks|NumSgprs|LDSByteSize|sgpr_spill_count|vgpr_spill_count)\b", ln) or \
                re.search(r"\.(sgpr_spill_count|vgpr_spill_count|private_segment_fixed_size):", ln):
            print(" ", ln.strip("; \t"))
        if re.match(r"^_Z", ln):
            break


if __name__ == "__main__":
    args = [a for a in sys.argv[1:] if a != "--print"]
    if len(args) != 2:
        sys.exit(__doc__)
    main(args[0], args[1], "--print" in sys.argv)
