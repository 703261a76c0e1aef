"""Interleaved A/B of the two fp16 arithmetic modes of the network, f16x3 against f16x1, in ONE process (arithmetic modes).

    python tools/precision_ab.py [--rounds 6] [--seconds 3] [--json out.json]

Two modules with the same weights (make_state_dict(42)), nrows 4, P = 128, 512 x 1024 panoramas.  Legs, each run for --seconds per mode and round,
modes alternating (ABBA...) so that clock / power drift hits both alike:
  pipelined  8 panoramas per forward, net.pipelined(3) (the launch bench.py times)
  single     one panorama per forward, plain calls
Per leg and mode: panoramas/s (median over rounds) and joules per panorama (mean board power from the amdgpu hwmon readout of
tools/clocks_under_load.py, sampled every 50 ms during the leg, times its duration over its panoramas; NaN where the container shows no hwmon).
Accuracy: max / mean |f16x1 - f16x3| of the depth maps on the same inputs (metres), both legs.  Prints a table and one JSON line."""
import argparse
import glob
import json
import os
import sys
import threading
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

from omnifusion_amd.model.spherical_model import spherical_fusion
from omnifusion_amd.weights import make_state_dict

_HW = None


def _hwmon():
    """the amdgpu hwmon directory of the GPU torch runs on (as tools/clocks_under_load.py finds it), or None"""
    global _HW
    if _HW is None:
        _HW = ""
        try:
            p = torch.cuda.get_device_properties(0)
            bdf = f"{p.pci_domain_id:04x}:{p.pci_bus_id:02x}:{p.pci_device_id:02x}.0"
            c = [d for d in sorted(glob.glob(f"/sys/bus/pci/devices/{bdf}/hwmon/hwmon*")) if os.path.exists(d + "/freq1_input")]
            _HW = c[0] if c else ""
        except Exception:
            pass
    return _HW or None


def _power_w():
    hw = _hwmon()
    if not hw:
        return float("nan")
    try:
        pf = hw + ("/power1_average" if os.path.exists(hw + "/power1_average") else "/power1_input")
        return float(open(pf).read()) / 1e6
    except Exception:
        return float("nan")


def _timed(fn, seconds, per_call):
    """run fn back to back for `seconds` (after a warm-up) -> (panoramas/s, joules per panorama, mean W)"""
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    stop, watts = threading.Event(), []

    def watcher():
        while not stop.is_set():
            watts.append(_power_w())
            time.sleep(0.05)
    th = threading.Thread(target=watcher)
    th.start()
    t0, n = time.perf_counter(), 0
    while time.perf_counter() - t0 < seconds:
        fn()
        n += 1
    torch.cuda.synchronize()
    dt = time.perf_counter() - t0
    stop.set()
    th.join()
    w = float(np.nanmean(watts[2:] if len(watts) > 4 else watts)) if watts and not all(np.isnan(watts)) else float("nan")
    pans = n * per_call
    return pans / dt, w * dt / pans, w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=6)
    ap.add_argument("--seconds", type=float, default=3.0)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    assert torch.cuda.is_available(), "tools/precision_ab.py needs an MI355X"
    dev = "cuda:0"
    sd = make_state_dict(42, 18, False)
    nets = {}
    for prec in ("f16x3", "f16x1"):
        n = spherical_fusion(4, 18, (128, 128), (80, 80), precision=prec).cuda()
        n.load_state_dict(sd)
        nets[prec] = n
    g = torch.Generator(device=dev).manual_seed(7)
    rgb = torch.rand((args.batch, 3, 512, 1024), device=dev, generator=g)
    rgb = F.avg_pool2d(F.pad(rgb, (7, 7, 7, 7), mode="replicate"), 15, stride=1)          # a smooth panorama (the class the parity gates use)
    one = rgb[:1].contiguous()

    # accuracy on the same inputs
    acc = {}
    outs = {p: n.pipelined(3)(rgb).get() for p, n in nets.items()}
    d = (outs["f16x1"] - outs["f16x3"]).abs()
    acc["pipelined"] = (d.max().item(), d.mean().item())
    outs = {p: n(one) for p, n in nets.items()}
    d = (outs["f16x1"] - outs["f16x3"]).abs()
    acc["single"] = (d.max().item(), d.mean().item())

    legs = {}
    for p, n in nets.items():
        run, pend = n.pipelined(3), []

        def piped(run=run, pend=pend):
            pend.append(run(rgb))
            if len(pend) > 3:
                pend.pop(0).get()
        legs[("pipelined", p)] = (piped, args.batch)
        legs[("single", p)] = ((lambda n=n: n(one)), 1)
    res = {k: [] for k in legs}
    order = ["f16x3", "f16x1"]
    for r in range(args.rounds):
        for leg in ("pipelined", "single"):
            for p in (order if r % 2 == 0 else order[::-1]):
                fn, per = legs[(leg, p)]
                res[(leg, p)].append(_timed(fn, args.seconds, per))
    summary = {"hwmon": _hwmon() or None, "rounds": args.rounds, "seconds": args.seconds, "batch": args.batch}
    print(f"{'leg':10s} {'mode':6s} {'panoramas/s (median)':>22s} {'min':>8s} {'max':>8s} {'J/panorama':>11s} {'W':>7s}")
    for (leg, p), v in res.items():
        a = np.array(v)
        summary[f"{leg}_{p}_pps"] = float(np.median(a[:, 0]))
        summary[f"{leg}_{p}_j_per_pan"] = float(np.nanmedian(a[:, 1])) if not np.all(np.isnan(a[:, 1])) else None
        summary[f"{leg}_{p}_w"] = float(np.nanmedian(a[:, 2])) if not np.all(np.isnan(a[:, 2])) else None
        print(f"{leg:10s} {p:6s} {np.median(a[:, 0]):22.1f} {a[:, 0].min():8.1f} {a[:, 0].max():8.1f} {np.nanmedian(a[:, 1]) if not np.all(np.isnan(a[:, 1])) else float('nan'):11.4f} "
              f"{np.nanmedian(a[:, 2]) if not np.all(np.isnan(a[:, 2])) else float('nan'):7.0f}")
    for leg in ("pipelined", "single"):
        summary[f"{leg}_speedup"] = summary[f"{leg}_f16x1_pps"] / summary[f"{leg}_f16x3_pps"]
        summary[f"{leg}_maxdiff_m"], summary[f"{leg}_meandiff_m"] = acc[leg]
        print(f"{leg}: f16x1 / f16x3 = {summary[f'{leg}_speedup']:.3f}x panoramas/s; |f16x1 - f16x3| max {acc[leg][0]:.4g} m, mean {acc[leg][1]:.4g} m")
    print(json.dumps(summary))
    if args.json:
        with open(args.json, "w") as f:
            json.dump(summary, f, indent=1)


if __name__ == "__main__":
    main()
