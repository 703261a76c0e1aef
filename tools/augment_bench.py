"""Augmentation timing: `augment_rgb` + `augment_depth` (csrc/omni_augment.hip) against the plain `preprocess_rgb` + `preprocess_depth`
they extend and against the torch-eager chain a user would otherwise write, on the same GPU in the same run.

    python tools/augment_bench.py [--rounds 9] [--reps 8] [--bufs 3] [--out profiles/r15a_augment.json] [--quick]

Method (as tools/chamfer_bench.py): the legs ALTERNATE — every round times each leg once, the median over the rounds is reported with
its minimum and maximum — and every call takes the next of `--bufs` copies of the inputs and of the rgb output.  Each leg is `reps x bufs`
calls captured once in a graph and replayed between two device events: the time per call is the kernels' (a 20 us pass is shorter than the
host's enqueue of it, which an eager loop would measure instead).

Shapes: B = 8 at 512 x 1024 from frames of the same size, and from 2048 x 4096 frames.
Legs:  a         preprocess_rgb + preprocess_depth (no augmentation: what the same bytes cost before this unit)
       b         augment_rgb + augment_depth: flip, roll dx = 3 W / 4, permutation (2, 0, 1), gamma 1 / 1.7 on every item
       b_mis     the same with dx = 3 W / 4 + 1 (the same-size quad path then loads from odd byte offsets and one quad per row straddles the seam)
       b_nogamma b with every exponent 1 (the block-uniform branch skips the table)
       b_direct  b with option augment_lut = 0: powf per value instead of the 256-entry table per block
       c         a, then torch.flip, torch.roll, channel indexing and ** on the batch (the eager chain)
       *_rgb     the rgb kernel of a / b / b_mis / b_direct alone (for the fraction of the floor)
Floor: bytes / 8 TB/s.  The rgb pass moves 3 + 12 bytes per pixel (62.9 MB at 8 x 512 x 1024 from same-size frames: 7.9 us), the depth
pass 2 + 5; from larger frames the source bytes are the frames'.
Gamma error: max |device - float32(float64(v32) ** float64(g32))| over the timed batch, v32 the output without gamma.
--quick: B = 2 at 64 x 128 (and from 128 x 256), few rounds: a rehearsal of the tool, not a measurement.
"""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

DEV = "cuda:0"
HBM_BYTES_PER_S = 8e12
PERM = (2, 0, 1)
GAMMA = 1.0 / 1.7


def make_aug(B, dx, gamma):
    from omnifusion_amd.data import Augmentation
    return Augmentation([1] * B, [dx] * B, [list(PERM)] * B, [gamma] * B).to(DEV)


def bench_shape(B, src, dst, a):
    from omnifusion_amd import _lib
    from omnifusion_amd.data import augment_depth, augment_rgb, preprocess_depth, preprocess_rgb
    H, W = dst
    n = a.bufs
    g = torch.Generator(device=DEV).manual_seed(1500)
    frs = [torch.randint(0, 256, (B,) + src + (3,), device=DEV, generator=g, dtype=torch.uint8) for _ in range(n)]
    dzs = [torch.randint(0, 6000, (B,) + src, device=DEV, generator=g, dtype=torch.int16) for _ in range(n)]
    outs = [torch.empty((B, 3, H, W), device=DEV) for _ in range(n)]
    dx = 3 * W // 4
    aug, aug_mis, aug_one = make_aug(B, dx, GAMMA), make_aug(B, dx + 1, GAMMA), make_aug(B, dx, 1.0)
    gam = aug.gamma.view(B, 1, 1, 1)
    perm_t = torch.tensor(PERM, device=DEV)                                     # (an index made from a Python list is copied to the device per call: not capturable)

    def plain(k):
        return preprocess_rgb(frs[k], dst, out=outs[k]), preprocess_depth(dzs[k], dst)

    def both(t):
        return lambda k: (augment_rgb(frs[k], dst, t, out=outs[k]), augment_depth(dzs[k], dst, t))

    def eager(k):
        rgb, (d, m) = plain(k)
        rgb = torch.roll(torch.flip(rgb, dims=[-1]), dx, dims=-1)[:, perm_t] ** gam
        return rgb, torch.roll(torch.flip(d, dims=[-1]), dx, dims=-1), torch.roll(torch.flip(m, dims=[-1]), dx, dims=-1)

    legs = {"a": plain, "b": both(aug), "b_mis": both(aug_mis), "b_nogamma": both(aug_one), "b_direct": both(aug), "c": eager,
            "a_rgb": lambda k: preprocess_rgb(frs[k], dst, out=outs[k]), "b_rgb": lambda k: augment_rgb(frs[k], dst, aug, out=outs[k]),
            "b_mis_rgb": lambda k: augment_rgb(frs[k], dst, aug_mis, out=outs[k]), "b_direct_rgb": lambda k: augment_rgb(frs[k], dst, aug, out=outs[k])}
    lut_of = lambda name: 0 if "direct" in name else 1

    # ---- results first: b against the eager chain, the table against the direct form, gamma against float64
    want = eager(0)
    want = tuple(t.clone() for t in want)
    got = both(aug)(0)
    v32 = augment_rgb(frs[0], dst, aug_one).clone()
    got_rgb = got[0].clone()
    _lib.set_option("augment_lut", 0)
    direct = augment_rgb(frs[0], dst, aug).clone()
    _lib.set_option("augment_lut", 1)
    ref = (v32.double() ** aug.gamma.double().view(B, 1, 1, 1)).float()
    parity = dict(map_equals_eager_chain_without_gamma=bool(torch.equal(v32, torch.roll(torch.flip(plain(0)[0], dims=[-1]), dx, dims=-1)[:, perm_t])),
                  depth_equals_eager_chain=bool(torch.equal(got[1][0], want[1]) and torch.equal(got[1][1], want[2])),
                  table_equals_direct_powf=bool(torch.equal(got_rgb, direct)),
                  gamma_max_abs_err_vs_f64=float((got_rgb.double() - ref.double()).abs().max()),
                  torch_pow_max_abs_err_vs_f64=float((want[0].double() - ref.double()).abs().max()))

    # ---- one graph per leg: reps x bufs calls on one stream
    graphs = {}
    side = torch.cuda.Stream()
    for name, fn in legs.items():
        _lib.set_option("augment_lut", lut_of(name))
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for k in range(n):
                fn(k)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        gr = torch.cuda.CUDAGraph()
        with torch.cuda.graph(gr):
            for r in range(a.reps):
                for k in range(n):
                    fn(k)
        graphs[name] = gr
    _lib.set_option("augment_lut", 1)
    calls = a.reps * n
    for gr in graphs.values():
        gr.replay()
    torch.cuda.synchronize()
    times = {k: [] for k in legs}
    for _ in range(a.rounds):
        for name, gr in graphs.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.replays):
                gr.replay()
            e1.record()
            torch.cuda.synchronize()
            times[name].append(e0.elapsed_time(e1) / (calls * a.replays) * 1e3)          # us per call
    med = {k: statistics.median(v) for k, v in times.items()}
    px_src, px = B * src[0] * src[1], B * H * W
    rgb_bytes, depth_bytes = 3 * px_src + 12 * px, 2 * px_src + 5 * px
    floor_rgb, floor_both = rgb_bytes / HBM_BYTES_PER_S * 1e6, (rgb_bytes + depth_bytes) / HBM_BYTES_PER_S * 1e6
    row = dict(B=B, src=list(src), dst=list(dst), rounds=a.rounds, replays=a.replays, calls_per_graph=calls, bufs=n, dx=dx, dx_misaligned=dx + 1, perm=list(PERM),
               gamma=GAMMA, parity=parity, rgb_bytes=rgb_bytes, depth_bytes=depth_bytes, floor_rgb_us=round(floor_rgb, 2), floor_rgb_depth_us=round(floor_both, 2))
    for name, v in times.items():
        row[name + "_us"] = round(med[name], 2)
        row[name + "_us_min_max"] = [round(min(v), 2), round(max(v), 2)]
    row["a_spread_us"] = round(max(times["a"]) - min(times["a"]), 2)
    for name in ("b", "b_mis", "b_nogamma", "b_direct"):
        row[name + "_minus_a_us"] = round(med[name] - med["a"], 2)
        row[name + "_within_a_min_max"] = bool(min(times["a"]) <= med[name] <= max(times["a"]))
    row["c_over_b"] = round(med["c"] / med["b"], 2)
    row["table_vs_direct_powf_us"] = [row["b_rgb_us"], row["b_direct_rgb_us"]]
    for name in ("a_rgb", "b_rgb", "b_mis_rgb", "b_direct_rgb"):
        row[name + "_frac_of_floor"] = round(floor_rgb / med[name], 4)
    row["b_frac_of_floor"] = round(floor_both / med["b"], 4)
    print(json.dumps(row), flush=True)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--reps", type=int, default=8, help="passes over the buffers captured in one graph")
    ap.add_argument("--replays", type=int, default=4, help="graph replays per timed window")
    ap.add_argument("--bufs", type=int, default=3)
    ap.add_argument("--out", default=None)
    ap.add_argument("--quick", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "augment_bench measures on an MI355X; there is no CPU timing"
    from omnifusion_amd.build import source_hash
    if a.quick:
        a.rounds, a.reps, a.replays = 2, 2, 1
        shapes = [(2, (64, 128), (64, 128)), (2, (128, 256), (64, 128))]
    else:
        shapes = [(8, (512, 1024), (512, 1024)), (8, (2048, 4096), (512, 1024))]
    rows = [bench_shape(B, src, dst, a) for B, src, dst in shapes]
    res = dict(build=source_hash(), device=torch.cuda.get_device_name(0), hbm_bytes_per_s=HBM_BYTES_PER_S, quick=bool(a.quick), rows=rows)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)


if __name__ == "__main__":
    main()
