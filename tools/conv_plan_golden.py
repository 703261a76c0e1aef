"""The kernel choice of omni_conv2d_sh_f16x3_ws as DATA: the case set of tests/test_conv_plan_cpu.py, the recorder that wrote
tests/golden/conv_plan_parent.json, and the random sweep of a recording library against omni_conv2d_sh_plan.  No GPU needed.

    python tools/conv_plan_golden.py --record LIBREC.so [--out tests/golden/conv_plan_parent.json]
    python tools/conv_plan_golden.py --sweep LIBREC.so [--pairs 200000] [--lib LIB.so]

LIBREC.so is a throwaway build of the revision whose decisions are to be pinned (for the committed file: the parent of the change that
introduced conv_sh_plan), patched so that its four launch sites — launch_sh, omni_halo_launch, omni_conv_pm_launch, omni_halo2_launch —
write (family, bm, bn, wm, wn, nst, nl, pp, th, iw, grid_x, grid_y, threads, splitk) to an exported `int omni_rec[16]` and return without
launching, and conv2d_sh_impl returns right behind the choice.  The convolution entry points are then driven with dummy non-null pointers.
The patch is never committed; the expected values therefore never come from the code under test.
"""
import argparse
import ctypes
import json
import os
import random
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIELDS = ["family", "bm", "bn", "wm", "wn", "nst", "nl", "pp", "th", "iw", "grid_x", "grid_y", "threads", "splitk"]
OPTIONS = ["conv_sh_tile", "conv_pingpong", "conv_big_blocks", "conv_nohalo", "conv_halo_th", "conv_halo_bn", "conv_halo_bn_lat", "conv_img",
           "conv_deep_loaders", "conv_nodeep", "conv_epi_lds", "conv_pm", "conv_halo2"]


def option_sets():
    """Every OPTION_SETS entry of tests/test_precision_f16x1_gpu.py, then each value of the three- and four-valued options"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_precision_f16x1_gpu import OPTION_SETS
    return [dict(o) for o in OPTION_SETS] + [dict(conv_halo2=v) for v in (0, 1, 2, 300)] + [dict(conv_pm=v) for v in (0, 1, 2, 3, 4)] + \
        [dict(conv_img=v) for v in (0, 1, 2)] + [dict(conv_halo_bn_lat=64)]


def engine_shapes(bs, splitk):
    """(label, fmt, M, H, W, C1, C2, Cout, KH, KW, stride, pad, splitk) of every omni_conv2d_sh_f16x3[_post]_ws call of Engine.network and
    Engine.transformer at patch size 128 and `bs` panoramas (model/_engine.py: _Forward.conv, .gemm_sh, .fc2), with the engine's own split-K plan
    (`splitk` = omni_conv2d_splitk_plan at the nominal batch 8, or 4 for a lone panorama) and fmt (bit 2 for a lone panorama's convolutions, bit 1 for the GEMMs' fp32 residual)."""
    M, lat, plan_bs = 18 * bs, (4 if bs == 1 else 0), (4 if bs == 1 else 8)
    out = []

    def conv(label, H, C1, C2, Cout, k, stride, pad, f32=False):
        Ho = (H + 2 * pad - k) // stride + 1
        S = splitk(M * Ho * Ho // bs * plan_bs, Cout, k * k * (C1 + C2) // 32)
        out.append((label, (0 if f32 else 1) | lat, M, H, H, C1, C2, Cout, k, k, stride, pad, S))

    cin, size = 64, 32
    for name, cout, stride in (("layer1", 64, 1), ("layer2", 128, 2), ("layer3", 256, 2), ("layer4", 512, 2)):
        if stride == 2:
            conv(name + ".0.ds", size, cin, 0, cout, 1, 2, 0)
            conv(name + ".0.c1", size, cin, 0, cout, 3, 2, 1)
            size //= 2
        conv(name + ".c", size, cout, 0, cout, 3, 1, 1)
        cin = cout
    conv("down", 4, 512, 0, 32, 1, 1, 0, f32=True)
    conv("de_conv0_0.taps", 4, 512, 0, 9 * 256, 1, 1, 0, f32=True)
    conv("de_conv0_1", 8, 256, 256, 128, 3, 1, 1)
    conv("de_conv1_0", 16, 128, 0, 128, 3, 1, 1)
    conv("de_conv1_1", 16, 128, 128, 64, 3, 1, 1)
    conv("de_conv2_1", 32, 64, 64, 64, 3, 1, 1)
    conv("de_conv3_1", 64, 64, 64, 32, 3, 1, 1)
    for label, K, N, sh in (("qkv", 512, 1536, 0), ("proj", 512, 512, 0), ("fc1", 512, 2048, 1), ("fc2", 2048, 512, 0)):
        S = 1 if K <= 512 else splitk(M // bs * plan_bs, N, K // 32)
        out.append((label, sh | 2, M, 1, 1, K, 0, N, 1, 1, 1, 0, S))
    return [(f"b{bs} {s[0]}",) + s[1:] for s in out]


def shapes(splitk):
    out = []
    for bs in (1, 4, 8):
        out += engine_shapes(bs, splitk)
    # the "must not take" shapes of tests/test_conv_halo2_gpu.py (dims, S, fmt bit 2) and of tests/test_conv_pm_gpu.py
    for i, (d, S, f4) in enumerate([((2, 12, 32, 64, 0, 64, 3, 1, 1), 1, 0), ((2, 8, 48, 64, 0, 64, 3, 1, 1), 1, 0), ((2, 16, 64, 64, 0, 64, 3, 2, 1), 1, 0),
                                    ((2, 8, 32, 64, 0, 64, 1, 1, 0), 1, 0), ((2, 8, 32, 64, 0, 64, 3, 1, 1), 2, 0), ((2, 8, 32, 64, 0, 32, 3, 1, 1), 1, 0),
                                    ((4, 8, 8, 64, 0, 64, 3, 1, 1), 1, 0), ((2, 8, 32, 64, 0, 64, 3, 1, 1), 1, 4)]):
        out.append((f"halo2 must-not {i}", 1 | f4) + d[:6] + (d[6], d[6], d[7], d[8], S))
    for i, d in enumerate([(18, 8, 8, 64, 0, 64, 3, 2, 1), (18, 8, 8, 64, 0, 64, 1, 1, 0), (5, 16, 16, 64, 0, 64, 3, 1, 1), (18, 4, 8, 64, 0, 64, 3, 1, 1)]):
        for S in sorted({1, min(3, d[6] * d[6] * 2)}):
            out.append((f"pm must-not {i} S{S}", 1) + d[:6] + (d[6], d[6], d[7], d[8], S))
    # 8 x 8 and 4 x 4 images
    for W in (8, 4):
        for Cout in (64, 128, 256):
            for M in (36, 144):
                for S in (1, 2):
                    out.append((f"img{W} {Cout} M{M} S{S}", 1, M, W, W, 128, 0, Cout, 3, 3, 1, 1, S))
    # Cout = 32 and 96: small images, wide images, a GEMM
    for Cout in (32, 96):
        out += [(f"cout{Cout} img16", 1, 18, 16, 16, 64, 0, Cout, 3, 3, 1, 1, 1), (f"cout{Cout} wide", 1, 4, 8, 32, 64, 0, Cout, 3, 3, 1, 1, 1),
                (f"cout{Cout} lat", 5, 4, 8, 32, 64, 0, Cout, 3, 3, 1, 1, 1), (f"cout{Cout} 1x1", 0, 300, 1, 1, 256, 0, Cout, 1, 1, 1, 0, 1)]
    # rows no multiple of 128
    out += [("odd rows 3x3", 1, 5, 7, 9, 64, 0, 64, 3, 3, 1, 1, 1), ("odd rows 17x13", 0, 2, 17, 13, 32, 0, 32, 3, 3, 1, 1, 1),
            ("odd rows gemm", 2, 1000, 1, 1, 512, 0, 128, 1, 1, 1, 0, 1), ("odd rows gemm S2", 2, 1000, 1, 1, 512, 0, 128, 1, 1, 1, 0, 2)]
    # exactly 255 / 256 / 257 halo2 blocks: 8 x 32 images are one 256-pixel tile each, 64 channels one channel tile
    for M in (255, 256, 257):
        out.append((f"halo2 {M} blocks", 1, M, 8, 32, 64, 0, 64, 3, 3, 1, 1, 1))
    for M in (127, 128, 129):                                       # ... and of the whole-image form, two channel tiles
        out.append((f"halo2 img16 {2 * M} blocks", 1, M, 16, 16, 64, 0, 128, 3, 3, 1, 1, 1))
    # exactly 127 / 128 blocks of each 128-row tile: GEMM rows (128 x 128, 128 x 64, 256 x 128 counted in 256-row tiles), the position-major shapes, split-K
    for n in (127, 128):
        out += [(f"tile128x128 {n}", 0, 128 * n, 1, 1, 256, 0, 128, 1, 1, 1, 0, 1), (f"tile128x64 {n}", 0, 128 * n, 1, 1, 256, 0, 64, 1, 1, 1, 0, 1),
                (f"tile128x128 {n} rows-1", 0, 128 * n - 127, 1, 1, 256, 0, 128, 1, 1, 1, 0, 1), (f"tile128x64 {n} rows-1", 0, 128 * n - 127, 1, 1, 256, 0, 64, 1, 1, 1, 0, 1),
                (f"tile256x128 {n}", 0, 256 * n, 1, 1, 256, 0, 128, 1, 1, 1, 0, 1),
                (f"pm128 {n}", 1, 2 * n, 8, 8, 128, 0, 128, 3, 3, 1, 1, 1), (f"pm64 {n}", 1, 2 * n, 8, 8, 128, 0, 64, 3, 3, 1, 1, 1),
                (f"pm128 img4 {n}", 1, 8 * n, 4, 4, 128, 0, 128, 3, 3, 1, 1, 1), (f"pm64 img4 {n}", 1, 8 * n, 4, 4, 128, 0, 64, 3, 3, 1, 1, 1)]
    out += [("tile128x128 127 S", 0, 128 * 127, 1, 1, 256, 0, 256, 1, 1, 1, 0, 1), ("tile128x128 2x64 S2", 0, 128 * 32, 1, 1, 256, 0, 256, 1, 1, 1, 0, 2),
            ("tile128x128 2x63 S2 +1", 0, 128 * 31 + 1, 1, 1, 256, 0, 256, 1, 1, 1, 0, 2), ("tile128x128 127 S2 -", 0, 128 * 31, 1, 1, 256, 0, 256, 1, 1, 1, 0, 2)]
    # the 64 x 64 tiles' one-round rule: 256 / 257 blocks, 7 / 8 K-steps
    for rows in (64 * 256, 64 * 256 + 1):
        for K in (224, 256):
            out.append((f"deep {rows} K{K}", 0, rows, 1, 1, K, 0, 64, 1, 1, 1, 0, 1))
    return out


class Lib:
    """a library through ctypes alone (no torch: nothing here touches a device)"""

    def __init__(self, path, recording):
        self.lib = ctypes.CDLL(path)
        self.rec = (ctypes.c_int * 16).in_dll(self.lib, "omni_rec") if recording else None
        self.defaults = {o: self.get(o) for o in OPTIONS}
        if not recording:
            self.lib.omni_conv2d_sh_plan.argtypes = [ctypes.c_int] * 13 + [ctypes.POINTER(ctypes.c_int), ctypes.c_int]

    def get(self, name):
        v = ctypes.c_int(0)
        assert self.lib.omni_get_option(name.encode(), ctypes.byref(v)) == 0, name
        return v.value

    def splitk_plan(self, rows, Cout, ksteps):
        return int(self.lib.omni_conv2d_splitk_plan(ctypes.c_longlong(rows), Cout, ksteps))

    def options(self, opts):
        for o in OPTIONS:
            assert self.lib.omni_set_option(o.encode(), int(opts.get(o, self.defaults[o]))) == 0, o

    def plan(self, fmt, dims, post):
        """the 14 integers, or (-status,)"""
        M, H, W, C1, C2, Cout, KH, KW, stride, pad, S = dims
        if self.rec is None:
            out = (ctypes.c_int * 14)()
            rc = self.lib.omni_conv2d_sh_plan(fmt, M, H, W, C1, C2, Cout, KH, KW, stride, pad, S, 1 if post else 0, out, 14)
            return tuple(out) if rc == 0 else (-rc,)
        p = ctypes.c_void_p(0x10000)
        for i in range(16):
            self.rec[i] = -1
        args = (p, p if C2 else None, p, None, None, p, fmt, M, H, W, C1, C2, Cout, KH, KW, stride, pad, 0, S, p, ctypes.c_size_t(1 << 62))
        if post:
            rc = self.lib.omni_conv2d_sh_f16x3_post_ws(*args, p, ctypes.c_size_t(Cout), None)
        else:
            rc = self.lib.omni_conv2d_sh_f16x3_ws(*args, None)
        return tuple(self.rec[:14]) if rc == 0 else (-rc,)


def record(path, out_path):
    lib = Lib(path, True)
    sets, shp = option_sets(), shapes(lib.splitk_plan)
    plans, index, answers = [], {}, []
    for s in shp:
        rows = []
        for post in (0, 1):
            row = []
            for opts in sets:
                lib.options(opts)
                got = lib.plan(s[1], s[2:], post)
                assert got == lib.plan(s[1] | 8, s[2:], post), ("the arithmetic mode changed the parent's choice", s, opts)
                if len(got) == 1:
                    row.append(got[0])
                else:
                    assert min(got) >= 0, (s, opts, got)
                    row.append(index.setdefault(got, len(index)))
                    if len(plans) < len(index):
                        plans.append(list(got))
            rows.append(row)
        answers.append(rows)
    lib.options({})
    doc = {"fields": FIELDS, "defaults": lib.defaults, "option_sets": sets, "shapes": [list(s) for s in shp], "plans": plans, "answers": answers}
    with open(out_path, "w") as f:
        f.write("{\n" + ",\n".join(f' "{k}": ' + (json.dumps(v) if k not in ("shapes", "plans", "answers") else
                                                   "[\n  " + ",\n  ".join(json.dumps(e, separators=(",", ":")) for e in v) + "\n ]") for k, v in doc.items()) + "\n}\n")
    print(f"{len(shp)} shapes x {len(sets)} option sets x post 0 / 1 (x both arithmetic modes): {len(plans)} distinct plans -> {out_path}, {os.path.getsize(out_path)} bytes")


def sweep(rec_path, lib_path, pairs, seed=1):
    a, b = Lib(rec_path, True), Lib(lib_path, False)
    rng = random.Random(seed)
    sets = option_sets()
    ranges = dict(conv_sh_tile=(-1, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9), conv_pingpong=(0, 1), conv_big_blocks=(0, 1, 64, 128, 256, 512), conv_nohalo=(0, 0, 0, 1), conv_halo_th=(4, 8),
                  conv_halo_bn=(64, 32), conv_halo_bn_lat=(32, 64), conv_img=(0, 1, 2), conv_deep_loaders=(0, 1), conv_nodeep=(0, 0, 1), conv_pm=(0, 1, 2, 3, 4),
                  conv_halo2=(0, 1, 2, 3, 100, 300))
    sizes = (1, 2, 4, 7, 8, 12, 16, 17, 32, 48, 64)
    ndiff = nerr = 0
    families = {}
    for i in range(pairs):
        opts = dict(rng.choice(sets)) if rng.random() < 0.3 else {k: rng.choice(v) for k, v in ranges.items() if rng.random() < 0.35}
        a.options(opts), b.options(opts)
        kind = rng.random()
        k = rng.choice((1, 3, 3, 3, 2))
        if kind < 0.2:                                              # a GEMM
            dims = (rng.choice((18, 72, 144, rng.randint(1, 40000))), 1, 1, rng.choice((32, 256, 512, 2048)), 0, rng.choice((32, 64, 96, 128, 512, 1536)), 1, 1, 1, 0, rng.choice((1, 1, 2, 4, 16)))
        elif kind < 0.6:                                            # the shapes the halo, halo2 and position-major kernels serve, and their near misses
            H = rng.choice((4, 8, 8, 16, 16, 32, 64, 12))
            W = H if rng.random() < 0.7 else rng.choice((32, 64, 48, 8))
            M = rng.choice((1, 2, 4, 16, 18, 36, 72, 144, 254, 256, rng.randint(1, 600)))
            dims = (M, H, W, rng.choice((32, 64, 128)), rng.choice((0, 0, 64)), rng.choice((32, 64, 64, 128, 128, 256)), 3, 3, 1, 1, rng.choice((1, 1, 1, 1, 2)))
        else:
            H = rng.choice(sizes)
            W = H if rng.random() < 0.6 else rng.choice(sizes)
            M = rng.choice((1, 2, 5, 18, 72, 144, rng.randint(1, 600)))
            dims = (M, H, W, rng.choice((32, 64, 128, 256)), rng.choice((0, 0, 32, 64, 256)), rng.choice((32, 64, 96, 128, 192, 256, 512)),
                    k, k if rng.random() < 0.9 else rng.choice((1, 2, 3)), rng.choice((1, 1, 1, 2)), rng.choice((0, 1, 1, 1, 2)) if k > 1 else rng.choice((0, 0, 1)), rng.choice((1, 1, 1, 2, 3, 8, 40)))
        fmt, post = rng.choice((0, 1, 2, 4, 5, 8, 9, 12, 13)), rng.random() < 0.25
        pa, pb = a.plan(fmt, dims, post), b.plan(fmt, dims, post)
        nerr += len(pa) == 1
        families[pa[0]] = families.get(pa[0], 0) + 1
        if pa != pb:
            ndiff += 1
            if ndiff <= 20:
                print("DIFFERENT:", fmt, dims, post, opts, pa, pb)
    print(f"{pairs} (shape, option) pairs compared, {nerr} of them rejected by both, {ndiff} differences; by family / -status: {dict(sorted(families.items()))}")
    return ndiff


if __name__ == "__main__":
    ap = argparse.ArgumentParser(usage=__doc__)
    ap.add_argument("--record")
    ap.add_argument("--sweep")
    ap.add_argument("--out", default=os.path.join(ROOT, "tests", "golden", "conv_plan_parent.json"))
    ap.add_argument("--lib", default=os.path.join(ROOT, "omnifusion_amd", "csrc", "libomnifusion_hip.so"))
    ap.add_argument("--pairs", type=int, default=200000)
    opt = ap.parse_args()
    if opt.record:
        record(opt.record, opt.out)
    if opt.sweep:
        sys.exit(1 if sweep(opt.sweep, opt.lib, opt.pairs) else 0)
