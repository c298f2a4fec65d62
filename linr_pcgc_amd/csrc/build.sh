#!/bin/bash
# Builds liblinr_hip.so (gfx950 code objects + C-ABI) in-tree.  hipcc cross-compiles without a GPU.
set -e
cd "$(dirname "$0")"
OUT=../liblinr_hip.so
mkdir -p _obj
FLAGS="--offload-arch=gfx950 -O3 -fPIC -std=c++17 -fvisibility=hidden -Wall"
# the ONE list of sources: compiled below, linked in this order
HIP="kmap spconv linear loss_optim prof bwd_tail net fused wgrad fused_bwd occ_wgrad net_bf16 train_bf16 decode octree wide wide_mul wide_bf16 wide_fwd wide_train ac_codes ac_device ac_device_dec ply_format ply_parse fake_quant params_avg overfit digest"
CPP="ac ply digest_host params_avg_host"
# stale <name> <dependencies>: the object is missing or older than one of them
stale() {
  [ ! -f _obj/$1.o ] && return 0
  for d in "${@:2}"; do [ $d -nt _obj/$1.o ] && return 0; done
  return 1
}
pids=()
objs=()
for f in $HIP; do
  objs+=(_obj/$f.o)
  if stale $f $f.hip *.h ../../include/linr_hip.h; then          # its source, ANY header of this directory, the C-ABI header
    # fused_bwd / net_bf16: accumulators and destinations of the matrix instructions in VGPRs - fewer AGPR <-> VGPR copies in the
    # one-wave-per-SIMD kernels (same box: 1.6445 -> 1.629 ms/step; bf16 forward 0.436 -> 0.422 ms); no gain for the other files
    EXTRA=""
    if [ $f = fused_bwd ] || [ $f = net_bf16 ] || [ $f = train_bf16 ]; then EXTRA="-mllvm -amdgpu-mfma-vgpr-form"; fi
    if [ $f = occ_wgrad ]; then EXTRA="-mllvm -amdgpu-sched-strategy=max-ilp"; fi          # -5 us/step (same box, twice); slower for fused.hip
    hipcc $FLAGS $EXTRA -c $f.hip -o _obj/$f.o &
    pids+=($!)
  fi
done
for f in $CPP; do
  objs+=(_obj/$f.o)
  if stale $f $f.cpp *.h ../../include/linr_hip.h; then          # as above: ac.cpp includes rc_body.h
    EXTRA=""
    # ac: the coder loops on 64-byte boundaries, so that their speed does not depend on what is linked in front of them (the
    # decoder, same instructions, at offset 0x30 of a cache line: 5.06 -> 5.37 ns per symbol; profiles/host_coder_one_body.txt)
    if [ $f = ac ]; then EXTRA="-fno-math-errno -falign-functions=64"; fi
    g++ -O3 $EXTRA -fPIC -std=c++17 -fvisibility=hidden -Wall -c $f.cpp -o _obj/$f.o &
    pids+=($!)
  fi
done
for p in "${pids[@]}"; do wait $p; done
hipcc --offload-arch=gfx950 -shared -fPIC -o $OUT "${objs[@]}" -lpthread
echo "built $(realpath $OUT)"
