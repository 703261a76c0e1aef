"""The bits of the training operators whose sums cross blocks (csrc/omni_partials.h), one line per operator:

    python tools/bits_digest.py [--only batch_norm,conv2d]          ->  operator case sha256(outputs and gradients)

at the test cases in which a finish thread adds more than one partial, with the inputs of the tests' own builders.  Nothing printed depends on
the run, so two builds that add in the same order print the same lines: run it in two fresh processes, one of them with OMNI_LIB_VARIANT set
to the other build's library, and compare.  This is the instrument the note in csrc/omni_reduce.h asks for when a reduction moves.
"""
import argparse
import hashlib
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def digest(tensors):
    h = hashlib.sha256()
    for t in tensors:
        h.update(b"-" if t is None else t.detach().contiguous().cpu().numpy().tobytes())
    return h.hexdigest()


def batch_norm():
    import test_batchnorm_gpu as t
    out = t.run("rows131200", d=t.inputs("rows131200"))
    return "rows131200", [out[k] for k in t.OUTS]


def layer_norm():
    import test_transformer_bwd_gpu as t
    rows, C, eps = 2 * t.FINISH_THREADS * t.LN_SLAB_ROWS + 5, 100, 1e-5          # test_layernorm_many_slabs
    return f"rows{rows}", t.ln_device(*t.ln_case(rows, C, eps, "unit"), eps, True)


def stem_conv2d():
    import test_spatial_ops_gpu as t
    out = t.stem_run(t.stem_reference("rows10240", True)[0], True)
    return "rows10240", [out[k] for k in ("y", "dw", "db")]


def depth_heads():
    import test_heads_bwd_gpu as t
    out = t.run(t.case_inputs("rows40960"), "conf-both")
    return "rows40960", [out[k] for k in ("a", "c") + tuple("d" + p for p in t.PARAMS)]


def conv2d():
    import test_conv_bwd_gpu as t
    out = t.run("rows16641", d=t.inputs("rows16641"))
    return "rows16641", [out[k] for k in t.KINDS]


OPERATORS = (batch_norm, layer_norm, stem_conv2d, depth_heads, conv2d)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    only = [s for s in ap.parse_args().only.split(",") if s]
    if not torch.cuda.is_available():
        raise SystemExit("bits_digest needs an MI355X: nothing is computed without one")
    for op in OPERATORS:
        if not only or op.__name__ in only:
            case, tensors = op()
            print(op.__name__, case, digest(tensors), flush=True)


if __name__ == "__main__":
    main()
