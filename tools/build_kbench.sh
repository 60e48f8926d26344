#!/bin/bash
# Builds the A/B binaries of tools/kbench.hip against the CURRENT kernel source, with the flags the library's scan2 object is
# built with (csrc/Makefile SCAN2_FLAGS): kb_cur = the round-1 scalar-validity k = 21 build, kb_s2_hb14 = the shipped sv2
# kernel, kb_a_* = its ablations (tools/profile_round.sh runs them), kb_a_floor = the floor kernel (window words + per-position
# work on synthetic register-resident words: no loads, no encode, no validity), kb_v_clocks = the per-wave clock census,
# kb_s2_default = the shipped kernel under the default scheduler, plus the instruction micro-benchmarks.
# The ablation switches are not in the product headers: kbench_ablations.patch puts them into a copy under var/kbench_src/, and
# kbench.hip is compiled against that copy.  Needs no GPU.  Exits non-zero, naming it, if any binary failed to build.
set -eu
cd "$(dirname "$0")"
SRC=var/kbench_src
rm -rf $SRC
mkdir -p $SRC/needletail_amd/csrc
cp ../needletail_amd/csrc/ntk_kernels.hpp ../needletail_amd/csrc/ntk_tile.hpp ../needletail_amd/csrc/ntk_plan.hpp $SRC/needletail_amd/csrc/
patch -p1 --fuzz=0 -d $SRC < kbench_ablations.patch   # a hunk that no longer fits stops the build here
B="--offload-arch=gfx950 -O3 -std=c++17"
F="$B -I$SRC/needletail_amd/csrc -DNTK_KB_FIX -DNTK_KB_SV"
S="$F -DNTK_KB_SV2 -DNTK_KB_HB=14 -mllvm -amdgpu-sched-strategy=iterative-ilp"
rm -f kb_* ubench ubench3
all=(); names=(); pids=(); failed=()
reap() { wait "${pids[0]}" || failed+=("${names[0]}"); pids=("${pids[@]:1}"); names=("${names[@]:1}"); }
# -cuid (new with the patch step): the compilation-unit id names one symbol of the code object, __hip_cuid_<id>, and is otherwise a hash of
# the source path and the whole command line.  With it fixed, one variant built from two trees, or with another -I, gives the same code
# object byte for byte exactly when the kernels are the same, which is what an A/B tool wants to be able to check.  It is safe here because
# the id only has to differ between translation units that are linked together, and every binary below is a single one.
build() {   # build <binary> <source> <flags ...>: in the background, at most 16 compiles at a time
    [ ${#pids[@]} -lt 16 ] || reap
    local out=$1 src=$2; shift 2
    hipcc "$@" -cuid="$out" -o "$out" "$src" &
    pids+=($!); names+=("$out"); all+=("$out")
}
build kb_cur kbench.hip $F
build kb_s2_hb14 kbench.hip $S
build kb_s2_default kbench.hip $F -DNTK_KB_SV2 -DNTK_KB_HB=14
build kb_a_nolds kbench.hip $S -DNTK_ABL_NOLDS
build kb_a_loads kbench.hip $S -DNTK_ABL_LOADSONLY
build kb_a_floor kbench.hip $S -DNTK_ABL_FLOOR
build kb_a_nomaskalg kbench.hip $S -DNTK_ABL_NOMASKALG
build kb_a_nosdwa kbench.hip $S -DNTK_ABL_NOSDWA -DNTK_ABL_NOMASKALG
build kb_a_nodigest kbench.hip $S -DNTK_ABL_NODIGEST
build kb_a_noemit kbench.hip $S -DNTK_ABL_NODIGEST -DNTK_ABL_NOLDS
build kb_a_noexec kbench.hip $S -DNTK_ABL_NOEXEC
build kb_v_clocks kbench.hip $S -DNTK_V_CLOCKS
build ubench ubench.hip $B
build ubench3 ubench3.hip $B
while [ ${#pids[@]} -gt 0 ]; do reap; done
for b in "${all[@]}"; do [ -x "$b" ] || failed+=("$b"); done
if [ ${#failed[@]} -gt 0 ]; then echo "build_kbench.sh: NOT built:" $(printf '%s\n' "${failed[@]}" | sort -u) >&2; exit 1; fi
ls "${all[@]}"
