"""The old and the new launch of the two 64 -> 64 up-sampling stages, alone, at 144 patches (8 panoramas) — for a profiler:

    rocprofv3 --pmc SQ_INSTS_MFMA SQ_INSTS_LDS SQ_INSTS_VALU -- python tools/taps_fused_launches.py      (counters: a run of their own, no tracing)
    rocprofv3 --kernel-trace --stats -- python tools/taps_fused_launches.py                               (times alone)

de_conv2_0: 16 x 16 -> 32 x 32, de_conv3_0: 32 x 32 -> 64 x 64; each form --reps times (default 5), random inputs and weights.
conv3x3_halo_sh_kernel<64, 4, true, 0, false> is omni_conv3x3_up2_sh_f16x3; up2_taps_fused_kernel<..> is omni_conv3x3_up2_taps_sh_f16x3 under option
conv_up2_taps_walk = 0 and up2_taps_walk_kernel<..> the same entry point under --walk (default 2: the new kernel for both forms; 1: the forms that ship);
the template arguments tell the stages apart (the halo kernel's: the grid)."""
import argparse
import ctypes
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch

from omnifusion_amd import _lib
from omnifusion_amd.model._engine import split_weights_f16x3

ap = argparse.ArgumentParser(); ap.add_argument("--patches", type=int, default=144); ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--walk", type=int, default=2)
a = ap.parse_args()
lib = _lib.load()
p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None
s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
g = torch.Generator().manual_seed(3)
w = torch.randn(64, 64, 3, 3, generator=g) / 24.0
b = torch.randn(64, generator=g).cuda()
w16 = split_weights_f16x3(w.permute(0, 2, 3, 1).reshape(64, -1).contiguous()).cuda()
w16t = split_weights_f16x3(w.permute(2, 3, 0, 1).reshape(9 * 64, 64).contiguous()).cuda()
M = a.patches
for Hl in (16, 32):
    x = torch.randn(M, Hl, Hl, 64, generator=g).cuda()
    xs = torch.empty_like(x)
    _lib.check(lib.omni_sh_from_f32(p(x), p(xs), ctypes.c_size_t(x.numel()), s), "sh_from_f32")
    old, new, walk = (torch.empty((M, 2 * Hl, 2 * Hl, 64), device="cuda") for _ in range(3))
    shipped = _lib.get_option("conv_up2_taps_walk")
    for _ in range(a.reps):
        _lib.check(lib.omni_conv3x3_up2_sh_f16x3(p(xs), p(w16), p(b), p(old), 1, M, Hl, Hl, 64, 64, 1, s), "old")
        _lib.set_option("conv_up2_taps_walk", 0)
        _lib.check(lib.omni_conv3x3_up2_taps_sh_f16x3(p(xs), p(w16t), p(b), p(new), 1, M, Hl, Hl, 64, 64, 1, s), "new")
        _lib.set_option("conv_up2_taps_walk", a.walk)
        _lib.check(lib.omni_conv3x3_up2_taps_sh_f16x3(p(xs), p(w16t), p(b), p(walk), 1, M, Hl, Hl, 64, 64, 1, s), "walk")
    _lib.set_option("conv_up2_taps_walk", shipped)
    torch.cuda.synchronize()
    print(f"{Hl} x {Hl}: max |new - old| (SH words as floats) = {(new - old).abs().max().item():.3g}; walk has the bits of new: {torch.equal(walk.view(torch.int32), new.view(torch.int32))}")
print("done")
