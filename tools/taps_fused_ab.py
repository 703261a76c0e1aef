"""Interleaved A/B of Engine.taps_fused — the decoder stages de_conv2_0 / de_conv3_0 as nine 1x1 tap products on the low-resolution map summed
in LDS (omni_conv3x3_up2_taps_sh_f16x3, one launch), against the up-sampling halo kernel — in ONE process (operator table).  The
sibling of tools/taps_ab.py.

    python tools/taps_fused_ab.py [--rounds 6] [--seconds 3] [--legs pipelined,plain,single] [--json out.json]

One module (make_state_dict(42), nrows 4, P = 128, 512 x 1024 panoramas); cases: no layer, each layer alone, both.  Legs, each run for
--seconds per case and round, the case order reversed every other round (ABBA...) so that clock / power drift hits all alike:
  pipelined  8 panoramas per forward, net.pipelined(3) (the launch bench.py times)
  plain      8 panoramas per forward, plain calls
  single     one panorama per forward, plain calls
Per leg and case: panoramas/s of every round, median, min, max; `separated` = every round of the case beats every round of "none" (the
project's standard for "not noise").  Accuracy: max |depth(case) - depth(none)| on the same inputs.  Prints a table and one JSON line."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from omnifusion_amd.model._engine import Engine
from omnifusion_amd.model.spherical_model import spherical_fusion
from omnifusion_amd.weights import make_state_dict

CASES = {"none": frozenset(), "de_conv3_0": frozenset(("de_conv3_0",)), "de_conv2_0": frozenset(("de_conv2_0",)),
         "both": frozenset(("de_conv2_0", "de_conv3_0"))}


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
    ap.add_argument("--legs", default="pipelined,plain,single")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/taps_fused_ab.py needs an MI355X"
    dev = "cuda:0"
    net = spherical_fusion(4, 18, (128, 128), (80, 80)).cuda()
    net.load_state_dict(make_state_dict(42, 18, False))
    g = torch.Generator(device=dev).manual_seed(7)
    rgb = torch.rand((args.batch, 3, 512, 1024), device=dev, generator=g)
    rgb = F.avg_pool2d(F.pad(rgb, (7, 7, 7, 7), mode="replicate"), 15, stride=1)          # a smooth panorama (the class the parity gates use)
    one = rgb[:1].contiguous()
    shipped = Engine.taps_fused
    run, pend = net.pipelined(3), []

    def piped():
        pend.append(run(rgb))
        if len(pend) > 3:
            pend.pop(0).get()

    def drain():
        while pend:
            pend.pop(0).get()
    legs = {"pipelined": (piped, args.batch), "plain": (lambda: net(rgb), args.batch), "single": (lambda: net(one), 1)}
    legs = {k: v for k, v in legs.items() if k in args.legs.split(",")}
    try:
        outs = {}
        for case, layers in CASES.items():                       # accuracy on the same inputs
            Engine.taps_fused = layers
            outs[case] = (net(rgb).clone(), net(one).clone())
        diff = {c: (float((o[0] - outs["none"][0]).abs().max()), float((o[1] - outs["none"][1]).abs().max())) for c, o in outs.items()}
        res = {(leg, c): [] for leg in legs for c in CASES}
        order = list(CASES)
        for r in range(args.rounds):
            for leg, (fn, per) in legs.items():
                for c in (order if r % 2 == 0 else order[::-1]):
                    Engine.taps_fused = CASES[c]
                    res[(leg, c)].append(_timed(fn, args.seconds, per))
                    drain()
    finally:
        Engine.taps_fused = shipped
    summary = {"rounds": args.rounds, "seconds": args.seconds, "batch": args.batch, "shipped_default": sorted(shipped),
               "depth_max": float(outs["none"][0].max())}
    print(f"{'leg':10s} {'taps_fused':11s} {'panoramas/s (median)':>22s} {'min':>8s} {'max':>8s}  separated from none")
    for (leg, c), v in res.items():
        a, base = np.array(v), np.array(res[(leg, "none")])
        sep = bool(a.min() > base.max()) if c != "none" else None
        summary[f"{leg}_{c}_pps"] = [round(float(x), 1) for x in a]
        summary[f"{leg}_{c}_median"] = float(np.median(a))
        summary[f"{leg}_{c}_separated"] = sep
        print(f"{leg:10s} {c:11s} {np.median(a):22.1f} {a.min():8.1f} {a.max():8.1f}  {'' if sep is None else sep}")
    for c in CASES:
        summary[f"maxdiff_batch_{c}_m"], summary[f"maxdiff_single_{c}_m"] = diff[c]
        print(f"{c}: max |depth - depth(none)| = {diff[c][0]:.3g} m at {args.batch} panoramas, {diff[c][1]:.3g} m for a lone one")
    print(json.dumps(summary))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
