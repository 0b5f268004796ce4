#!/bin/bash
# Builds an A/B variant of libbtba.so into /tmp/ab/<name>/ with the ISA kept, prints the cost model of the dense loop.
#   scripts/ab_build.sh <name> [-DMACRO ...]
name=$1; shift
root=$(cd "$(dirname "$0")/.." && pwd)
cd "$root" || exit 1
python -c "import sys; from bundletrack_amd import _lib; _lib.build(force=True, out='/tmp/ab/$name/libbtba.so', extra_flags=['-save-temps'] + sys.argv[1:])" "$@" 2>&1 | grep -v warning | grep -B2 -A6 "error" | head -30
S=/tmp/ab/$name/build/libbtba/btba_api-hip-amdgcn-amd-amdhsa-gfx950.s
echo "== $name $*"
python scripts/isa_cost.py $S k_fused_sweepsILi1E --loop ${LOOP:-1} | head -1
grep "k_fused_sweepsILi1E.*\.num_vgpr\|k_fused_sweepsILi1E.*private_seg" $S | sed 's/.*PKi//'
