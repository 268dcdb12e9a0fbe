#!/usr/bin/env python3
"""Static opcode histogram of one kernel in a hipcc -S listing, per basic block
(developer utility: where do the VALU slots of a register-resident kernel go?).

usage: isa_hist.py listing.s mangled-name-substring [--slots] [--min N]

A block starts at a label or behind a branch instruction (the piece behind the n-th branch of block L is 'L+n'), so
that the path a wave takes through a block with a branch in the middle can be read off.
Per block: VALU instructions, 's_nop' instructions and their sum -- the issue slots a wave spends on the block (an
's_nop' is a hazard wait the assembler inserted between dependent VALU instructions, one slot each, whatever its
count) -- 'slots' weighting the half-rate VALU operations twice, 'salu' (scalar ALU: s_* without waits, nops, branches,
priority and memory instructions) and 'vmem' (vector memory loads).  Blocks that head a loop are marked, and every loop
gets a line of its own summed over all blocks of its body (one trip: all paths taken, as a wave whose lanes diverge runs
them).
--slots prints only the block table (no opcode histogram); --min sets the VALU count below which a block is not
listed (default 20).

Listing of one instantiation, e.g. the headline sigma kernel (128 frames, zonal, plain sigma, TIGHT):
  hipcc <Makefile FLAGS> --offload-device-only -S nightlight_amd/csrc/stack_fast.hip -o /tmp/stack_fast.s
  isa_hist.py /tmp/stack_fast.s stack_sigma_fast_kernelILi128ELb1ELb0ELb1ELb0ELb0E --slots
The clipping pass of that kernel is the loop right after the sort (the block with ~2,300 VALU)."""
import collections
import re
import sys

HALF = ("v_min_f32", "v_max_f32", "v_med3", "v_min3", "v_max3", "v_cmp", "v_min_i32", "v_max_i32",
        "v_min_u32", "v_max_u32", "v_bfe", "v_perm", "v_alignbit")
NOT_ALU = ("s_nop", "s_waitcnt", "s_cbranch", "s_branch", "s_load", "s_buffer_load", "s_barrier", "s_endpgm",
           "s_sleep", "s_setprio", "s_memtime", "s_memrealtime", "s_dcache_inv", "s_icache_inv")


def blocks_of(lines, key):
    """[(label, innermost loop's header label or None, Counter of opcodes)] of the first kernel whose mangled name
    contains key (the loop comes from the compiler's '; in Loop: Header=...' annotations)"""
    start = next(i for i, l in enumerate(lines) if re.match(r"_Z\w+:", l) and key in l)
    end = next(i for i in range(start, len(lines)) if lines[i].startswith(".Lfunc_end"))
    out, name, loop, cur = [], "entry", None, collections.Counter()
    base, piece = name, 0
    for l in lines[start + 1:end]:
        m = re.match(r"(\.LBB\d+_\d+):(.*)", l)
        if m:
            out.append((name, loop, cur))
            name, cur = m.group(1), collections.Counter()
            base, piece = name, 0
            h = re.search(r"Header=(BB\d+_\d+)", m.group(2))
            loop = name if "Loop Header" in m.group(2) else (".L" + h.group(1) if h else None)
            continue
        m = re.match(r"\s*([vs]_\w+|ds_\w+|buffer_\w+|global_\w+|flat_\w+|scratch_\w+)", l)
        if m:
            cur[m.group(1)] += 1
            if m.group(1).startswith(("s_cbranch", "s_branch")):      # the block goes on behind a branch: a piece of its own
                out.append((name, loop, cur))
                piece += 1
                name, cur = "%s+%d" % (base, piece), collections.Counter()
    out.append((name, loop, cur))
    return out


def counts(c):
    valu = sum(n for op, n in c.items() if op.startswith("v_"))
    nop = c.get("s_nop", 0)
    slots = sum(n * (2 if op.startswith(HALF) else 1) for op, n in c.items() if op.startswith("v_"))
    salu = sum(n for op, n in c.items() if op.startswith("s_") and not op.startswith(NOT_ALU))
    vmem = sum(n for op, n in c.items() if op.startswith(("buffer_load", "global_load", "flat_load")))
    return valu, nop, slots, salu, vmem


def main(argv):
    args = [a for a in argv[1:] if not a.startswith("--")]
    only_slots = "--slots" in argv
    min_valu = 20
    if "--min" in argv:
        min_valu = int(argv[argv.index("--min") + 1])
        args.remove(str(min_valu))
    lines = open(args[0]).read().split("\n")
    blocks = blocks_of(lines, args[1])
    total = collections.Counter()
    print("%-12s %6s %6s %12s %6s %6s %6s" % ("block", "valu", "s_nop", "valu+s_nop", "slots", "salu", "vmem"))
    loops = collections.OrderedDict()
    for name, loop, c in blocks:
        total.update(c)
        if loop:
            loops.setdefault(loop, collections.Counter()).update(c)
        valu, nop, slots, salu, vmem = counts(c)
        if valu >= min_valu:
            print("%-12s %6d %6d %12d %6d %6d %6d  %s%s" % (name, valu, nop, valu + nop, slots, salu, vmem,
                                                     "(loop header) " if loop == name else "",
                                                     "" if only_slots else c.most_common(7)))
    valu, nop, slots, salu, vmem = counts(total)
    print("%-12s %6d %6d %12d %6d %6d %6d" % ("TOTAL", valu, nop, valu + nop, slots, salu, vmem))
    # a loop's body = its header block and every block the compiler annotates as inside it (innermost loop only)
    for head, c in loops.items():
        valu, nop, slots, _, _ = counts(c)
        if valu >= min_valu:
            print("loop %-7s %6d %6d %12d %6d  (all blocks of the loop body)" % (head, valu, nop, valu + nop, slots))
    if not only_slots:
        print(total.most_common(25))


if __name__ == "__main__":
    main(sys.argv)
