"""The bits of whole forwards, one line per configuration (after tools/bits_digest.py):

    python tools/engine_bits.py [--out FILE]          ->  model precision batch [pipelined] sha256(outputs)

single-pass and iterative (iter 2) models in f16x3, f16x1 and fp32 at 1, 3 and 8 panoramas of 3 x 128 x 256 with the weights of
make_state_dict(42, ...), and for the single-pass f16x3 model at 1 and 8 panoramas also four forwards through `pipelined(2, graphs=True)` (each slot
captured once and replayed once).  Nothing printed depends on the run, so two revisions of the host code over the same library print the same
file: run it on each in a fresh process and compare.  A difference then is an ordering or lifetime error of the Python side.
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def main():
    from omnifusion_amd.model.spherical_model import spherical_fusion
    from omnifusion_amd.model.spherical_model_iterative import spherical_fusion as spherical_fusion_it
    from omnifusion_amd.model._engine import PRECISIONS
    from omnifusion_amd.weights import make_state_dict
    ap = argparse.ArgumentParser()
    ap.add_argument("--out")
    opt = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("engine_bits needs an MI355X: nothing is computed without one")
    rgb = torch.from_numpy(np.random.default_rng(7).random((8, 3, 128, 256), dtype=np.float32)).cuda()
    lines = []
    for model, cls, iterative in (("single", spherical_fusion, False), ("iterative", spherical_fusion_it, True)):
        sd = make_state_dict(42, 18, iterative)
        for prec in PRECISIONS:
            net = cls(4, 18, (128, 128), (80, 80), precision=prec).cuda().eval()
            net.load_state_dict(sd)
            for bs in (1, 3, 8):
                out = net(rgb[:bs], iter=2, confidence=True) if iterative else [net(rgb[:bs], confidence=True)]
                new = [f"{model} {prec} bs{bs} {digest(out)}"]
                if (model, prec) == ("single", "f16x3") and bs != 3:
                    run = net.pipelined(2, graphs=True)
                    pending = [run(rgb[:bs], confidence=True) for _ in range(4)]
                    new.append(f"{model} {prec} bs{bs} pipelined(2, graphs=True) {digest([p.get() for p in pending])}")
                print("\n".join(new), flush=True)
                lines += new
            torch.cuda.synchronize()
    if opt.out:
        with open(opt.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
