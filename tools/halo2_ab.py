"""Interleaved A/B of the library option conv_halo2 — halo2_sh_kernel (omni_conv_halo2.hip: 64-channel halo blocks on 256-pixel tiles with
64 x 64 wave tiles) against the parent halo kernels — in ONE process, the pattern of tools/conv_pm_ab.py.

    python tools/halo2_ab.py [--rounds 6] [--seconds 3] [--cases off,on] [--json out.json]

Cases: off (conv_halo2 0), on (1: launches of at least 256 new blocks), n128 / n512 (128 / 512: the rule with another least block count), all (2:
wherever the shape allows).  Legs, each run for --seconds per case and round, the case order
reversed every other round (ABBA...): pipelined (8 panoramas per forward, net.pipelined(3): the launch bench.py times), plain (8 panoramas,
plain calls), single (one panorama per forward).  `separated` = every round of the case beats every round of "off"; `below` = every round of the case is under every round of "off".  The outputs of all
cases must be equal bit for bit (asserted)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from omnifusion_amd import _lib as L
from omnifusion_amd.model.spherical_model import spherical_fusion
from omnifusion_amd.weights import make_state_dict

ALL_CASES = {"off": 0, "on": 1, "n128": 128, "n512": 512, "all": 2}


def _timed(fn, seconds, per_call):
    """run fn back to back for `seconds` (after a warm-up) -> panoramas/s"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds:
        fn()
        n += 1
    torch.cuda.synchronize()
    return n * per_call / (time.perf_counter() - t0)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--cases", default="off,on")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    CASES = {c: ALL_CASES[c] for c in ["off"] + [c for c in args.cases.split(",") if c != "off"]}
    assert torch.cuda.is_available(), "tools/halo2_ab.py needs an MI355X"
    dev = "cuda:0"
    net = spherical_fusion(4, 18, (128, 128), (80, 80)).cuda()
    net.load_state_dict(make_state_dict(42, 18, False))
    g = torch.Generator(device=dev).manual_seed(7)
    rgb = torch.rand((args.batch, 3, 512, 1024), device=dev, generator=g)
    rgb = F.avg_pool2d(F.pad(rgb, (7, 7, 7, 7), mode="replicate"), 15, stride=1)          # a smooth panorama (the class the parity gates use)
    one = rgb[:1].contiguous()
    shipped = L.get_option("conv_halo2")
    run, pend = net.pipelined(3), []

    def piped():
        pend.append(run(rgb))
        if len(pend) > 3:
            pend.pop(0).get()

    def drain():
        while pend:
            pend.pop(0).get()
    legs = {"pipelined": (piped, args.batch), "plain": (lambda: net(rgb), args.batch), "single": (lambda: net(one), 1)}
    try:
        outs = {}
        for case, v in CASES.items():                            # the same bits on the same inputs
            L.set_option("conv_halo2", v)
            outs[case] = (net(rgb).clone(), net(one).clone())
        for case, o in outs.items():
            assert torch.equal(o[0], outs["off"][0]) and torch.equal(o[1], outs["off"][1]), case
        res = {(leg, c): [] for leg in legs for c in CASES}
        order = list(CASES)
        for r in range(args.rounds):
            for leg, (fn, per) in legs.items():
                for c in (order if r % 2 == 0 else order[::-1]):
                    L.set_option("conv_halo2", CASES[c])
                    res[(leg, c)].append(_timed(fn, args.seconds, per))
                    drain()
    finally:
        L.set_option("conv_halo2", shipped)
    summary = {"rounds": args.rounds, "seconds": args.seconds, "batch": args.batch, "shipped_default": shipped, "bits_equal": True}
    print(f"{'leg':10s} {'halo2':8s} {'panoramas/s (median)':>22s} {'min':>8s} {'max':>8s} {'ratio':>7s}  separated from off / below off")
    for (leg, c), v in res.items():
        a, base = np.array(v), np.array(res[(leg, "off")])
        sep = bool(a.min() > base.max()) if c != "off" else None
        below = bool(a.max() < base.min()) if c != "off" else None
        summary[f"{leg}_{c}_pps"] = [round(float(x), 1) for x in a]
        summary[f"{leg}_{c}_median"] = float(np.median(a))
        summary[f"{leg}_{c}_ratio"] = float(np.median(a) / np.median(base))
        summary[f"{leg}_{c}_separated"] = sep
        summary[f"{leg}_{c}_below"] = below
        print(f"{leg:10s} {c:8s} {np.median(a):22.1f} {a.min():8.1f} {a.max():8.1f} {np.median(a) / np.median(base):7.4f}  {'' if sep is None else f'{sep} / {below}'}")
    print(json.dumps(summary))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
