#!/bin/bash
# Build librlrep_hip.so for gfx950 (MI355X).  Cross-compiles without a GPU.
set -e
HERE="$(cd "$(dirname "$0")" && pwd)"
OUT="$HERE/../lib"
# RLREP_BUILD_EXPERIMENTS=1: the opt-in engines that were measured and NOT adopted (row-block programs rowprog.hip, per-XCD persistent
# chains xchain.hip, first layers fused into the second, superseded noise-critic forward kernels) are compiled in as well, into a library
# of their own (librlrep_hip_exp.so; RLREP_LIB selects it).  The product library carries stubs that report them as not built.
if [ -n "$RLREP_BUILD_EXPERIMENTS" ]; then
  EXTRA_FLAGS="$EXTRA_FLAGS -DRL_EXPERIMENTS"; EXP_SRCS="rowprog xchain"; OBJDIR="${OBJDIR:-.obj_exp}"; OUTNAME="${OUTNAME:-librlrep_hip_exp.so}"
else
  EXP_SRCS="experiments_off"
fi
OBJ="$HERE/${OBJDIR:-.obj}"          # OBJDIR / OUTNAME: instrumented variants beside the product library (EXTRA_FLAGS=-DRL_TIMING_NC ...)
LIBNAME="${OUTNAME:-librlrep_hip.so}"
mkdir -p "$OUT" "$OBJ"
HIPCC=${HIPCC:-/opt/rocm/bin/hipcc}
FLAGS="--offload-arch=gfx950 -O3 -fPIC -std=c++17 -Wall -Wno-unused-function $EXTRA_FLAGS"
SRCS="gemm16 gemm_lds noisecritic elementwise per per_group nstep nstep_targets actor_tile group_clone group_env sim_step sim_jit sim_jit_check replearn comm $EXP_SRCS engine agents1 agents2 group_api $EXTRA_SRCS"
# sim_jit.h is also carried in the library as text, for the run-time compile of a user's simulator kind (sim_jit.hip includes this file)
{ printf 'R"SIMJIT('; cat "$HERE/sim_jit.h"; printf ')SIMJIT"\n'; } > "$OBJ/sim_jit_text.inc.new"
if cmp -s "$OBJ/sim_jit_text.inc.new" "$OBJ/sim_jit_text.inc"; then rm -f "$OBJ/sim_jit_text.inc.new"; else mv "$OBJ/sim_jit_text.inc.new" "$OBJ/sim_jit_text.inc"; fi
pids=()
for f in $SRCS; do
  if [ ! -f "$OBJ/$f.o" ] || [ "$HERE/$f.hip" -nt "$OBJ/$f.o" ] || [ -n "$(find "$HERE" -maxdepth 1 -name '*.h' -newer "$OBJ/$f.o")" ] || [ "$HERE/../../include/rlrep.h" -nt "$OBJ/$f.o" ] || { [ "$f" = sim_jit_check ] && [ -n "$(find "$HERE/../envs/kinds" -name '*.h' -newer "$OBJ/$f.o")" ]; }; then
    PF=""; { [ "$f" = gemm16 ] || [ "$f" = elementwise ] || [ "$f" = gemm_lds ]; } && PF="-mllvm -amdgpu-kernarg-preload-count=14"     # gemm16_kernel / adam_kernel / the gemm_lds kernels: leading scalars preloaded into SGPRs
    [ "$f" = sim_jit ] && PF="-I$OBJ"                        # sim_jit_text.inc
    [ "$f" = sim_jit_check ] && PF="-ffp-contract=off -I$HERE/../envs/kinds"   # the example kinds, compiled as the run-time compile compiles them
    $HIPCC $FLAGS $PF -c "$HERE/$f.hip" -o "$OBJ/$f.o" &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
LINK=""; for f in $SRCS; do LINK="$LINK $OBJ/$f.o"; done
$HIPCC --offload-arch=gfx950 -shared -fPIC -o "$OUT/$LIBNAME" $LINK -L"${ROCM_PATH:-/opt/rocm}/lib" -lhiprtc
echo "built $OUT/$LIBNAME"
