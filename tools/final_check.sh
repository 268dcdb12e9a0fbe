#!/bin/bash
# The gate a library commit has to pass (ON THE GPU BOX, from the repo root; rule since round 6: no library commit after the
# last run of this script that ended "ok"):   tools/final_check.sh [out-dir]
#   0. (static, needs hipcc) the headline sigma kernel's registers, LDS and barriers   1. the -m gpu suite through the C ABI   2. smoke()
#   3. the default bench line with --full   4. tools/check_bench.py on it
# Stops at the first step that fails, faults or runs out of time.  The suite runs in ONE pytest process: parallel workers
# plus the ranks the distributed tests start would put more than six processes on the shared device.
cd "$(dirname "$0")/.." && export TMPDIR=/tmp
O=${1:-gpurun_out/final}; mkdir -p $O
# The headline kernel holds three waves per SIMD up to 168 VGPRs, and its count hangs on where the compiler places one
# branch (stack_fast_sigma_impl.hpp, the peeled first pass): 164 today, 191 - 199 when it goes wrong.  No spills either.
# It is wave-owned: no workgroup barrier, which would tie its waves together again.  Its LDS is the
# lookup rows of section 16, which a thread shares with nobody: at most 53 248 bytes, so that three workgroups fit a compute
# unit's 160 KiB as the registers allow.
make -s -C nightlight_amd/csrc kernel-info SRC=stack_fast.hip > $O/kernel_info.txt || exit 1
make -s -C nightlight_amd/csrc kernel-disasm > $O/kernel_disasm.txt || exit 1
python3 - $O/kernel_info.txt $O/kernel_disasm.txt <<'PY' || exit 1
import re, sys
key = "stack_sigma_fast_kernelILi128ELb1ELb0ELb1ELb0ELb0E"
line = [l for l in open(sys.argv[1]) if key in l]
assert len(line) == 1, "headline kernel not in the listing"
f = dict(re.findall(r"\.(\w+): +(\d+)", line[0]))
body, inside = [], False
for l in open(sys.argv[2]):
    m = re.match(r"[0-9a-f]+ <(\S+)>:", l)
    if m: inside = key in m.group(1)
    elif inside: body.append(l)
assert body, "headline kernel not in the disassembly"
barriers = sum(1 for l in body if re.search(r"\bs_barrier\b", l))
print("headline kernel: %s VGPRs, %s spilled, %s bytes of LDS, %d s_barrier in %d instructions"
      % (f["vgpr_count"], f["vgpr_spill_count"], f["group_segment_fixed_size"], barriers, len(body)))
sys.exit(0 if int(f["vgpr_count"]) <= 168 and int(f["vgpr_spill_count"]) == 0 and int(f["private_segment_fixed_size"]) == 0
         and int(f["group_segment_fixed_size"]) <= 53248 and barriers == 0 else 1)
PY
timeout -k 10 3000 python -m pytest tests -m gpu -x -q > $O/tests_gpu.log 2>&1; rc=$?; echo "rc=$rc" >> $O/tests_gpu.log; tail -3 $O/tests_gpu.log
[ $rc -eq 0 ] || exit $rc
timeout -k 10 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1; rc=$?; echo "rc=$rc" >> $O/smoke.log; tail -2 $O/smoke.log
[ $rc -eq 0 ] || exit $rc
t0=$(date +%s)
timeout -k 10 900 python bench.py --full --steps 20 --warmup 5 > $O/bench_default.json 2> $O/bench_default.err || exit $?
echo "bench: $(( $(date +%s) - t0 )) s"
python tools/check_bench.py $O/bench_default.json | tee $O/check_bench.txt
