#!/bin/bash
# Compile-time ablations of the f16x3 convolution kernels (OMNI_CONV_ABL in csrc/omni_conv_sh_common.h): builds one library variant per bit set HERE
# (no GPU needed), then `tools/convabl.sh run` on the GPU box times tools/convbench.py with each.   BITS="0 112 128 ..." ONLY=0,2,4
cd "$(dirname "$0")/.."
BITS=${BITS:-"0 112 128 256 512 640 752 4"}
C=omnifusion_amd/csrc
FL="--offload-arch=gfx950 -O3 -std=c++20 -munsafe-fp-atomics -fPIC -fno-gpu-rdc -ffp-contract=off -Xclang -target-feature -Xclang -packed-fp32-ops -Wno-unused-function"
if [ "$1" != run ]; then
  python -m omnifusion_amd.build > /dev/null 2>&1
  mkdir -p abl_build
  # every unit that includes omni_conv_sh_common.h is compiled with the flag (the bits live in tile, halo and up2 kernels); the link takes the OTHER units' product
  # objects — named from today's sources, so a stale *.o left by an older build is never linked
  UNITS=$(grep -l 'omni_conv_sh_common.h' $C/*.hip | xargs -n1 basename | sed 's/\.hip$//')
  REST=$(for s in $C/*.hip; do n=$(basename $s .hip); [ $n = omni_debug ] || echo "$UNITS" | grep -qx $n || echo $C/$n.o; done)
  for b in $BITS; do ( objs=""; for u in $UNITS; do /opt/rocm/bin/hipcc $FL -DOMNI_CONV_ABL=$b -c $C/$u.hip -o abl_build/${u}_$b.o 2>/dev/null || exit 1; objs="$objs abl_build/${u}_$b.o"; done
      /opt/rocm/bin/hipcc --offload-arch=gfx950 -shared -fPIC -o abl_build/libabl_$b.so $objs $REST && rm $objs ) & done
  wait; ls abl_build
else
  for b in $BITS; do echo "== bits=$b"; LIBPATH=abl_build/libabl_$b.so python tools/convbench.py; done
fi
