#!/bin/bash
# A/B library with ONE source compiled under extra flags:   tools/build_variant.sh <name> <source.hip> <flags...>
# -> build/<name>/libnlstack.so (every other object is the default build's; run with NLSTACK_LIB=$PWD/build/<name>/libnlstack.so)
# The compiler, its flags and the list of objects are the Makefile's own (make print-HIPCC / print-FLAGS / print-OBJS), so the
# variant differs from the default library in <flags...> only.  The build switches the sources still read:
#   -DNL_ROUND_STATS    round / hand-over counters of the sigma engines   tools/round_stats.py, tools/mlg_stats.py
#   -DNL_PROBE          cycle probes of the wave-per-pixel replay         tools/coop_probe.py   (stack_exact_coop.hip)
#   -DNL_PLAIN_STORES   plain instead of non-temporal result stores       (NL_STORE_RESULT, stack_kernels.h; profiles/r06_nt_stores_ab.txt)
# Limits: <flags...> travel through make's EXTRA and an unquoted echo, so a flag with spaces or quotes does not survive --
# plain -DNAME and -DNAME=value do.  print-FLAGS_<unit> is empty while the Makefile defines no per-unit flags.
set -e
name=$1; src=$2; shift 2
root=$(cd "$(dirname "$0")/.." && pwd)
cs=$root/nightlight_amd/csrc
unit=${src%.hip}
mkdir -p $root/build/$name
make -s -C $cs -j8
hipcc=$(make -s -C $cs print-HIPCC)
flags="$(make -s -C $cs print-FLAGS EXTRA="$*") $(make -s -C $cs print-FLAGS_$unit)"
(cd $cs && $hipcc $flags -c $src -o $root/build/$name/$unit.o)
objs=$(make -s -C $cs print-OBJS | tr ' ' '\n' | grep -v "^$unit\.o$" | sed "s|^|$cs/|")
$hipcc $(make -s -C $cs print-ARCH | sed 's/^/--offload-arch=/') -shared -fPIC $objs $root/build/$name/$unit.o -o $root/build/$name/libnlstack.so -lpthread
echo built $root/build/$name/libnlstack.so
